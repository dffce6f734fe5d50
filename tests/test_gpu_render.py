"""The render kernels on the GPU (docs/RENDER.md): body poses against model.fk, frames against the numpy restatement
(tests/np_render.py) with the tolerances of tests/test_render_host.py, determinism and batch independence, read-only-ness, argument
checks, hipGraph capture, and the Python surface (render / get_images / make_env(render=True) / python -m steppingstone_amd.enjoy).
The second half holds render_kernel's own write-out: frame sizes whose last tiles are partial under the cameras of tests/render_cases.py,
ss_render itself on pre-filled buffers with canary tails, each output alone, repeated and invalid ids."""
import ctypes as C

import numpy as np
import pytest
import torch

import np_render as nr
import render_cases as rc

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
    no_view = _cam(eye=(0.0, 0.0, 0.0))                                             # TRACK: the eye offset is the view vector
    no_view_fixed = _cam(mode=nr.FIXED, eye=(1.0, 2.0, 3.0), target=(1.0, 2.0, 3.0 + 5e-7))
    nan_eye = _cam(mode=nr.CHASE, eye=(-0.9, float("nan"), 0.45))
    for kw in (dict(m=0), dict(m=-1), dict(w=30), dict(h=18), dict(w=2052), dict(h=4096), dict(w=0), dict(rgb=None), dict(cam=bad_mode),
               dict(cam=bad_fov), dict(cam=no_view), dict(cam=no_view_fixed), dict(cam=nan_eye)):
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


# ---------------------------------------------------------------------------------------------------------------------------------------
# render_kernel's own write-out (LDS staging, dword stores of partial tiles) and the cameras of tests/render_cases.py
TAIL = 64                                                     # canary bytes (rgb, seg) / words (depth) behind each buffer
PART_N, PART_IDS = 8, [6, 1]


def _np_cam(cam):
    from steppingstone_amd.envs import make_camera
    return make_camera(cam["mode"], cam["eye"], cam["target"], cam["fov_y_deg"], cam["far_m"], cam["shadows"])


def _raw(e, ids, W, H, cam, fill, which=("rgb", "depth", "seg")):
    """ss_render itself on buffers pre-filled with the byte `fill`, each with a canary tail: -> (rc, {name: array with its tail})"""
    from steppingstone_amd.envs import _ptr, _stream
    m = len(ids)
    count = {"rgb": m * H * W * 3, "depth": m * H * W, "seg": m * H * W}
    kind = {"rgb": torch.uint8, "depth": torch.int32, "seg": torch.uint8}
    bufs = {k: torch.full((count[k] + TAIL,), fill if k != "depth" else (-1 if fill else 0), dtype=kind[k], device="cuda:0") for k in which}
    dev_ids = torch.as_tensor(ids, dtype=torch.int32).to("cuda:0")
    ptr = lambda k: _ptr(bufs[k]) if k in bufs else None
    rc = e.backend.lib.ss_render(e.backend.h, _ptr(dev_ids), m, W, H, C.byref(_np_cam(cam)), ptr("rgb"), ptr("depth"), ptr("seg"),
                                 _stream(e.device))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in bufs.items()}


def _frames(e, ids, W, H, cam, which=("rgb", "depth", "seg")):
    """the call with fill 0x00 and with fill 0xFF: the tails intact and the two results identical -- every byte inside was written and none
    outside -- -> {rgb [m,H,W,3] u8, depth [m,H,W] f32, seg [m,H,W] u8} of those asked for"""
    m = len(ids)
    shape = {"rgb": (m, H, W, 3), "depth": (m, H, W), "seg": (m, H, W)}
    outs = []
    for fill in (0x00, 0xFF):
        rc, bufs = _raw(e, ids, W, H, cam, fill, which)
        assert rc == 0
        out = {}
        for k, v in bufs.items():
            canary = v.dtype.type(fill if k != "depth" else (-1 if fill else 0))
            assert (v[-TAIL:] == canary).all(), "%dx%d: the words behind %s were written" % (W, H, k)
            body = v[:-TAIL].reshape(shape[k])
            out[k] = body.view(np.float32) if k == "depth" else body
        outs.append(out)
    for k in outs[0]:
        assert np.array_equal(outs[0][k].view(np.uint8), outs[1][k].view(np.uint8)), "%dx%d: %s depends on what the buffer held" % (W, H, k)
    return outs[0]


@pytest.fixture(scope="module", params=["walker3d", "mike"])
def partial_scene(request):
    """(kind, an 8-env instance at curriculum 5 after 40 random steps, its packed states)"""
    kind = request.param
    e = _env(kind, PART_N, seed=7, cur=5, steps=40)
    st = e.get_state().cpu().numpy()
    yield kind, e, st
    e.close()


@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: "%dx%d" % s)
def test_partial_tiles_and_other_cameras_match_numpy(partial_scene, size):
    import render_host_lib as rh
    kind, e, st = partial_scene
    W, H = size
    same = {"rgb": [], "depth": [], "seg": []}
    for name, cam in rc.cameras(st[PART_IDS[0], 0:3]):
        got = _frames(e, PART_IDS, W, H, cam)
        host = dict(zip(("rgb", "depth", "seg"), rh.render(["walker3d", "mike"].index(kind), st, PART_IDS, W, H, cam)))
        for m, i in enumerate(PART_IDS):
            ref = nr.render(kind, st[i].astype(np.float64), W, H, cam)
            nr.compare((got["rgb"][m], got["depth"][m], got["seg"][m]), ref, "%s %dx%d %s env %d" % (kind, W, H, name, i))
        for k in same:
            same[k].append(float((got[k].view(np.uint8) == host[k].view(np.uint8)).mean()))
    print("render device-vs-host %s %dx%d: share of equal bytes over %d cameras: %s"
          % (kind, W, H, len(same["rgb"]), {k: "%.4f (least %.4f)" % (np.mean(v), min(v)) for k, v in same.items()}))


def test_each_output_alone_equals_the_full_call(partial_scene):
    kind, e, st = partial_scene
    for name, cam in rc.cameras(st[PART_IDS[0], 0:3])[:4]:
        full = _frames(e, PART_IDS, 52, 36, cam)
        for k in ("rgb", "depth", "seg"):
            alone = _frames(e, PART_IDS, 52, 36, cam, which=(k,))
            assert set(alone) == {k} and np.array_equal(alone[k].view(np.uint8), full[k].view(np.uint8)), "%s alone, %s" % (k, name)


def test_repeated_and_invalid_ids_under_a_fixed_camera(partial_scene):
    kind, e, st = partial_scene
    ids = [3, -1, 3, PART_N, 0]
    name, cam = rc.cameras(st[3, 0:3])[0]
    assert cam["mode"] == nr.FIXED
    got = _frames(e, ids, 52, 36, cam)
    for k in got:
        assert np.array_equal(got[k][0].view(np.uint8), got[k][2].view(np.uint8)), "a repeated id gives another %s frame" % k
    back = nr.render(kind, None, 52, 36, cam)
    for m in (1, 3):
        assert (got["seg"][m] == 0).all() and (got["depth"][m] == np.float32(cam["far_m"])).all()
        assert np.abs(got["rgb"][m].astype(int) - back[0]).max() <= 1
    for m, i in enumerate(ids):
        alone = _frames(e, [i], 52, 36, cam)
        for k in got:
            assert np.array_equal(got[k][m].view(np.uint8), alone[k][0].view(np.uint8)), "row %d (id %d) of %s differs from the env drawn alone" % (m, i, k)
    assert (got["seg"][0] > 0).any()
