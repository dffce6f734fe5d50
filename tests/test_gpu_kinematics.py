"""ss_kinematics on the GPU (docs/PHYSICS.md 9): both robots, N = 70 envs (more than a wavefront, less than two, not a multiple of the
8 envs of a workgroup or of the 64-env padding), curriculum 5 after 30 random control steps.
  * all three outputs against the fp64 restatement with the K of tests/kinematics_cases.py, the carrier equal to the host build's;
  * a row's bits do not depend on the batch size, its position, the ids' order, a repeated id, or the outputs asked for;
  * rows of ids outside [0, N), everything at m == 0 and the words behind each buffer are never written;
  * bad host arguments answer SS_ERR_INVALID; the call leaves the state and the next step's results as they were."""
import ctypes as C

import numpy as np
import pytest
import torch

import kinematics_cases as kc
import kinematics_host_lib as kh
import np_kinematics as nk

pytestmark = pytest.mark.gpu
ENVS = {"walker3d": "Walker3DStepperEnv-v0", "mike": "MikeStepperEnv-v0"}
N = 70
WIDTH = {"body_twist": 22 * 6, "summary": 12, "corners": 8 * 8}
FILL = 0x5A5A5A5A
TAIL = 64                       # canary words behind each buffer


def _env(kind, n, seed=3, steps=30):
    from steppingstone_amd.envs import SteppingStoneVecEnv
    e = SteppingStoneVecEnv(ENVS[kind], n, seed=seed, device="cuda:0", return_numpy=False)
    e.update_curriculum(5)
    e.reset()
    if steps:
        e.rollout_random(steps, t0=0, steps_per_launch=1)
    return e


def _call(e, ids, m, which=("body_twist", "summary", "corners")):
    """ss_kinematics itself on pre-filled buffers with a canary tail: -> (rc, {name: int32 bit pattern [m * width + TAIL]})"""
    from steppingstone_amd.envs import _ptr, _stream
    bufs = {k: torch.full((max(m, 0) * WIDTH[k] + TAIL,), FILL, dtype=torch.int32, device="cuda:0") for k in which}
    dev_ids = None if ids is None else torch.as_tensor(ids, dtype=torch.int32).to("cuda:0")
    ptr = lambda k: _ptr(bufs[k]) if k in bufs else None
    rc = e.backend.lib.ss_kinematics(e.backend.h, None if dev_ids is None else _ptr(dev_ids), m, ptr("body_twist"), ptr("summary"),
                                     ptr("corners"), _stream(e.device))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in bufs.items()}


def _rows(buf, k, m):
    assert (buf[m * WIDTH[k]:] == FILL).all(), "the words behind %s were written" % k
    return buf[:m * WIDTH[k]].reshape(m, WIDTH[k])


@pytest.fixture(scope="module", params=kc.KINDS)
def scene(request):
    """(kind, env, packed rows [70,186], the whole batch's outputs as bit patterns): the env holds the rows through set_state, as
    every instance they are compared with does"""
    kind = request.param
    e = _env(kind, N)
    st = e.get_state().clone()
    e.set_state(st)
    rc, out = _call(e, None, N)
    assert rc == 0
    yield kind, e, st, {k: _rows(v, k, N) for k, v in out.items()}
    e.close()


def test_outputs_match_the_restatement_and_the_host_build(scene):
    kind, e, st, full = scene
    rows = st.cpu().numpy()
    as_f = {"body_twist": full["body_twist"].view(np.float32).reshape(N, 22, 6), "summary": full["summary"].view(np.float32),
            "corners": full["corners"].view(np.float32).reshape(N, 8, 8)}
    got = nk.split_outputs(as_f)
    m = kc.model(kind)
    refs = [nk.readout(m, r) for r in rows]
    worst = nk.worst_ratios(got, refs)
    print("kinematics device %s: worst err/(2^-24 B) per group: %s" % (kind, {g: round(w, 4) for g, w in worst.items()}))
    over = {g: (w, kc.K[g]) for g, w in worst.items() if not w <= kc.K[g]}
    assert set(worst) == set(nk.GROUPS) and not over, "%s: groups outside their K: %s" % (kind, over)
    host = nk.split_outputs(kh.kinematics(kc.KINDS.index(kind), rows))
    assert (got["corner_carrier"] == host["corner_carrier"]).all()
    same = {k: float((host[k] == got[k]).mean()) for k in nk.GROUPS}
    print("kinematics device-vs-host %s: share of bit-equal words per group: %s" % (kind, {k: round(v, 3) for k, v in same.items()}))
    # the Python surface returns the same words
    d = e.kinematics()
    assert torch.equal(d["com"].cpu(), torch.from_numpy(got["com"].copy())) and d["corner_carrier"].dtype == torch.int32
    assert (d["corner_carrier"].cpu().numpy() == got["corner_carrier"]).all()


def test_rows_do_not_depend_on_batch_position_or_requested_outputs(scene):
    kind, e, st, full = scene
    rng = np.random.default_rng(5)
    # (instance size, rows of st injected, at which positions)
    layouts = [(1, [37], [0]), (1, [69], [0]), (64, list(range(69, 5, -1)), list(range(64))), (130, list(range(N)), list(range(60, 130)))]
    for n2, src, pos in layouts:
        e2 = _env(kind, n2, seed=11, steps=0)
        e2.set_state(st[src], env_ids=pos)
        ids = rng.permutation(pos).tolist()
        ids.append(ids[0])                                      # one id twice
        row_of = {p: s for p, s in zip(pos, src)}
        want = [row_of[i] for i in ids]
        rc, out = _call(e2, ids, len(ids))
        assert rc == 0
        for k in WIDTH:
            assert (_rows(out[k], k, len(ids)) == full[k][want]).all(), "%s differs in a %d-env instance" % (k, n2)
            rc, one = _call(e2, ids, len(ids), which=(k,))
            assert rc == 0 and (_rows(one[k], k, len(ids)) == full[k][want]).all(), "%s differs when asked for alone" % k
        e2.close()


def test_rows_of_invalid_ids_and_everything_at_m_0_stay_untouched(scene):
    kind, e, st, full = scene
    ids = [3, -1, 64, N, 69, -1, N + 1000, 0]
    rc, out = _call(e, ids, len(ids))
    assert rc == 0
    for k in WIDTH:
        rows = _rows(out[k], k, len(ids))
        for r, i in enumerate(ids):
            if 0 <= i < N:
                assert (rows[r] == full[k][i]).all()
            else:
                assert (rows[r] == FILL).all(), "row %d (id %d) of %s was written" % (r, i, k)
    rc, out = _call(e, [], 0)
    assert rc == 0 and all((v == FILL).all() for v in out.values())
    rc, out = _call(e, None, 0)
    assert rc == 0 and all((v == FILL).all() for v in out.values())


def test_bad_arguments_are_refused(scene):
    from steppingstone_amd.envs import _ptr, _stream
    kind, e, st, full = scene
    lib, h, s = e.backend.lib, e.backend.h, _stream(e.device)
    ids = torch.arange(4, dtype=torch.int32, device="cuda:0")
    buf = torch.full((N * WIDTH["body_twist"] + TAIL,), FILL, dtype=torch.int32, device="cuda:0")
    p = _ptr(buf)
    off = C.c_void_p(buf.data_ptr() + 4)
    assert lib.ss_kinematics(h, _ptr(ids), 4, None, None, None, s) == -1                 # all outputs NULL with m > 0
    assert lib.ss_kinematics(h, None, 4, p, None, None, s) == -1                         # NULL ids with m != N
    assert lib.ss_kinematics(h, None, N + 1, p, None, None, s) == -1
    for args in ((off, None, None), (None, off, None), (None, None, off), (p, off, p)):  # a misaligned pointer
        assert lib.ss_kinematics(h, _ptr(ids), 4, *args, s) == -1
    assert lib.ss_kinematics(h, _ptr(ids), -1, p, None, None, s) == -1                   # m < 0
    assert b"ss_kinematics" in lib.ss_last_error()
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == FILL).all()                                             # nothing was launched
    assert lib.ss_kinematics(h, None, N, p, None, None, s) == 0
    torch.cuda.synchronize()
    assert (_rows(buf.cpu().numpy(), "body_twist", N) == full["body_twist"]).all()


@pytest.mark.parametrize("kind", kc.KINDS)
def test_the_call_only_reads(kind):
    a, b = _env(kind, N), _env(kind, N)
    before = a.get_state().clone()
    a.kinematics()
    a.kinematics(env_ids=[5, 2], twists=False)
    assert torch.equal(a.get_state().view(torch.int32), before.view(torch.int32))
    act = (torch.rand((N, 21), generator=torch.Generator().manual_seed(9)) * 2 - 1).to("cuda:0")     # one action tensor for both
    outs = []
    for e in (a, b):
        obs, rew, done, _ = e.step(act)
        outs.append((obs.clone(), rew.clone(), done.clone(), e.get_state().clone()))
        e.close()
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


def test_enjoy_trace_on_the_device(tmp_path):
    """--trace over the HIP backend: the recorded corner heights and carriers are the readout's, the contact flags the observation's"""
    from steppingstone_amd import enjoy, ppo
    torch.manual_seed(0)
    net = tmp_path / "policy.pt"
    torch.save(ppo.ActorCritic().state_dict(), net)
    enjoy.run("Walker3DStepperEnv-v0", str(net), envs=2, steps=12, size=(32, 32), trace=str(tmp_path / "t.npz"), log=lambda *a: None)
    tr = np.load(tmp_path / "t.npz")
    assert tr["com"].shape == (12, 2, 3) and tr["corner_carrier"].shape == (12, 2, 8) and tr["corner_carrier"].dtype == np.int32
    assert np.isfinite(tr["com"]).all() and np.isin(tr["corner_carrier"], (-1, 0, 1, 2)).all()
    assert tr["contact"].shape == (12, 2, 2) and (tr["next_step_index"] >= 1).all()
    held = (tr["corner_carrier"] == 1)
    assert ((tr["corner_height"][held] < 0) & (tr["corner_height"][held] > -0.10)).all()     # carried by the target: inside its contact set
