"""The render kernels on the GPU (docs/RENDER.md): body poses against model.fk, frames against the numpy restatement
(tests/np_render.py) with the tolerances of tests/test_render_host.py, determinism and batch independence, read-only-ness, argument
checks, hipGraph capture, and the Python surface (render / get_images / make_env(render=True) / python -m steppingstone_amd.enjoy)."""
import ctypes as C

import numpy as np
import pytest
import torch

import np_render as nr

pytestmark = pytest.mark.gpu
ENVS = {"walker3d": "Walker3DStepperEnv-v0", "mike": "MikeStepperEnv-v0"}


def _env(kind, n, seed=3, cur=0, steps=0):
    from steppingstone_amd.envs import SteppingStoneVecEnv
    e = SteppingStoneVecEnv(ENVS[kind], n, seed=seed, device="cuda:0", return_numpy=False)
    e.update_curriculum(cur)
    e.reset()
    if steps:
        e.rollout_random(steps, t0=0, steps_per_launch=1)
    torch.cuda.synchronize()
    return e


def _cam(**kw):
    from steppingstone_amd.envs import make_camera
    d = dict(nr.DEFAULT_CAMERA, **kw)
    return make_camera(d["mode"], d["eye"], d["target"], d["fov_y_deg"], d["far_m"], d["shadows"])


@pytest.mark.parametrize("kind", ["walker3d", "mike"])
def test_body_poses_match_model_fk(kind):
    from steppingstone_amd import model
    e = _env(kind, 1024, cur=5, steps=50)
    got = e.body_poses().cpu().numpy()
    st = e.get_state().cpu().numpy().astype(np.float64)
    e.close()
    m = model.build(kind)
    worst = 0.0
    for i in range(st.shape[0]):
        R, p = model.fk(m, st[i, 13:34], st[i, 0:3], nr.quat_matrix(st[i, 3:7]))
        ref = np.array([np.concatenate([p[b], R[b].reshape(-1)]) for b in range(model.NB)])
        worst = max(worst, float(np.abs(got[i] - ref).max()))
    assert got.shape == (1024, 22, 12) and worst < 2e-5, worst


@pytest.mark.parametrize("kind", ["walker3d", "mike"])
@pytest.mark.parametrize("cur", [0, 5])
def test_frames_match_numpy(kind, cur):
    e = _env(kind, 256, seed=7, cur=cur, steps=40)
    ids = np.random.default_rng(cur).choice(256, 16, replace=False)
    st = e.get_state().cpu().numpy().astype(np.float64)
    for shadows in (True, False):
        rgb, depth, seg = e.render(env_ids=ids, width=128, height=128, camera=_cam(shadows=shadows), depth=True, seg=True)
        rgb, depth, seg = rgb.cpu().numpy(), depth.cpu().numpy(), seg.cpu().numpy()
        for m, i in enumerate(ids):
            ref = nr.render(kind, st[i], 128, 128, dict(nr.DEFAULT_CAMERA, shadows=shadows))
            nr.compare((rgb[m], depth[m], seg[m]), ref, "%s c%d env %d shadows %s" % (kind, cur, i, shadows))
    e.close()


def test_deterministic_and_independent_of_batching():
    e = _env("walker3d", 64, cur=5, steps=30)
    cam = _cam(mode=nr.CHASE)
    ids = [5, 63, 0, 17, 5]
    a = e.render(env_ids=ids, width=96, height=64, camera=cam, depth=True, seg=True)
    b = e.render(env_ids=ids, width=96, height=64, camera=cam, depth=True, seg=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for m, i in enumerate(ids):
        alone = e.render(env_ids=[i], width=96, height=64, camera=cam, depth=True, seg=True)
        assert all(torch.equal(x[m], y[0]) for x, y in zip(a, alone))
    e.close()


def test_render_is_read_only():
    e, twin = _env("mike", 128, seed=9, cur=5, steps=20), _env("mike", 128, seed=9, cur=5, steps=20)
    before = e.get_state().clone()
    e.render(width=64, height=48, depth=True, seg=True)
    e.body_poses()
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int32), e.get_state().view(torch.int32))
    for t in range(10):
        a = e.random_actions(100 + t)
        o1, r1, d1, _ = e.step(a)
        o2, r2, d2, _ = twin.step(a)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
        e.render(env_ids=[t], width=32, height=32)
    assert torch.equal(e.get_state().view(torch.int32), twin.get_state().view(torch.int32))
    e.close()
    twin.close()


def test_invalid_arguments_and_out_of_range_ids():
    from steppingstone_amd import _lib
    e = _env("walker3d", 8)
    lib, h = e.backend.lib, e.backend.h
    dev = torch.device("cuda:0")
    ids = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    rgb = torch.zeros((2, 32, 32, 3), dtype=torch.uint8, device=dev)
    cam = _lib.default_camera()
    p = lambda t: C.c_void_p(t.data_ptr())
    ok = lambda **kw: lib.ss_render(h, p(ids), kw.get("m", 2), kw.get("w", 32), kw.get("h", 32), C.byref(kw.get("cam", cam)),
                                    kw.get("rgb", p(rgb)), None, None, None)
    assert ok() == 0
    torch.cuda.synchronize()
    bad_mode, bad_fov = _lib.default_camera(), _lib.default_camera()
    bad_mode.mode, bad_fov.fov_y_deg = 3, 0.0
    for kw in (dict(m=0), dict(m=-1), dict(w=30), dict(h=18), dict(w=2052), dict(h=4096), dict(w=0), dict(rgb=None), dict(cam=bad_mode),
               dict(cam=bad_fov)):
        assert ok(**kw) == -1, kw                            # SS_ERR_INVALID
        assert lib.ss_last_error()
    assert lib.ss_render(h, p(ids), 2, 32, 32, None, p(rgb), None, None, None) == -1
    assert lib.ss_body_poses(h, None, None) == -1
    # ids outside [0, N) are drawn as background
    rgb, depth, seg = e.render(env_ids=[-5, 8, 1 << 30, 3], width=32, height=16, depth=True, seg=True)
    ref = nr.render("walker3d", None, 32, 16)
    for m in range(3):
        assert (seg[m] == 0).all() and (depth[m] == cam.far_m).all()
        assert np.abs(rgb[m].cpu().numpy().astype(int) - ref[0]).max() <= 1
    assert (seg[3] > 0).any()
    e.close()


def test_graph_capture_of_step_and_render_replays_like_eager_calls():
    eager, graphed = _env("walker3d", 256, seed=4, cur=3), _env("walker3d", 256, seed=4, cur=3)
    act = torch.rand((256, 21), device="cuda:0") * 2 - 1
    ids = torch.arange(0, 256, 16, dtype=torch.int32, device="cuda:0")
    cam = _cam(mode=nr.CHASE)
    outs = [torch.zeros((16, 48, 64, 3), dtype=torch.uint8, device="cuda:0"), torch.zeros((16, 48, 64), device="cuda:0"),
            torch.zeros((16, 48, 64), dtype=torch.uint8, device="cuda:0")]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        graphed.backend.step(act, graphed._obs, graphed._rew, graphed._done, graphed._info)
        graphed.backend.render(ids, 64, 48, cam, *outs)
    torch.cuda.synchronize()
    for _ in range(3):
        eager.backend.step(act, eager._obs, eager._rew, eager._done, eager._info)
        want = eager.render(env_ids=ids, width=64, height=48, camera=cam, depth=True, seg=True)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(want, outs))
    eager.close()
    graphed.close()


def test_python_surface():
    from steppingstone_amd.envs import SteppingStoneVecEnv, make_env
    e = _env("mike", 3)
    f = e.render("rgb_array")
    assert f.dtype == torch.uint8 and f.shape == (3, 192, 256, 3) and f.device.type == "cuda"
    rgb, depth, seg = e.render(width=64, height=32, depth=True, seg=True)
    assert depth.dtype == torch.float32 and depth.shape == (3, 32, 64) and seg.dtype == torch.uint8 and seg.shape == (3, 32, 64)
    assert e.render(width=64, height=32, rgb=False, depth=True).shape == (3, 32, 64)
    imgs = e.get_images()
    assert len(imgs) == 3 and all(isinstance(i, np.ndarray) and i.shape == (192, 256, 3) and i.dtype == np.uint8 for i in imgs)
    assert e.body_poses().shape == (3, 22, 12)
    with pytest.raises(NotImplementedError):
        e.render("human")
    e.close()
    n = SteppingStoneVecEnv("Walker3DStepperEnv-v0", 2, seed=1, device="cuda:0", return_numpy=True)
    n.reset()
    fr = n.render(width=32, height=32, camera={"mode": "chase", "shadows": False})
    assert isinstance(fr, np.ndarray) and fr.shape == (2, 32, 32, 3)
    n.close()
    env = make_env("Walker3DStepperEnv-v0", render=True, device="cuda:0")
    env.reset()
    env.step(np.zeros(21, np.float32))
    img = env.render("rgb_array")
    assert isinstance(img, np.ndarray) and img.shape == (192, 256, 3) and img.dtype == np.uint8 and img.std() > 0
    with pytest.raises(NotImplementedError):
        env.render("human")
    env.close()


def test_enjoy_module(tmp_path, capsys):
    from steppingstone_amd import enjoy, ppo
    torch.manual_seed(0)
    net = tmp_path / "policy.pt"
    torch.save(ppo.ActorCritic().state_dict(), net)
    out = tmp_path / "walk.npy"
    rc = enjoy.main(["--env", "Walker3DStepperEnv-v0", "--net", str(net), "--envs", "2", "--steps", "60", "--size", "64x48",
                     "--out", str(out)])
    assert rc == 0
    anim = np.load(out)
    assert anim.shape == (60, 48, 128, 3) and anim.dtype == np.uint8
    assert "Model: policy.pt" in capsys.readouterr().out
    ck = tmp_path / "ck.pt"
    ppo.save_checkpoint(ppo.ActorCritic(), str(ck))
    anim = enjoy.run("MikeStepperEnv-v0", str(ck), envs=1, steps=5, size=(32, 32), camera="chase", log=lambda *a: None)
    assert anim.shape == (5, 32, 32, 3)
