"""ss_eom on the GPU (docs/PHYSICS.md 11): both robots, N = 70 envs (more than a wavefront, less than two, not a multiple of the 8 envs
of a workgroup or of the 64-env padding), curriculum 5 after 30 random control steps.
  * all three outputs against the fp64 restatement with the K of tests/eom_cases.py; the share of words bit-equal to the host build;
  * a row's bits do not depend on the instance size, its position, the ids' order, a repeated id, or the outputs asked for;
  * rows of ids outside [0, N), everything at m == 0 and the words behind each buffer are never written;
  * bad host arguments answer SS_ERR_INVALID; the call leaves the state and the next step's results as they were;
  * on one instance holding forces_cases.cases(kind): the readout agrees with ss_kinematics and closes the substep identity against
    ss_step_forces, with the assertions of tests/test_eom.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import eom_cases as ec
import eom_host_lib as eh
import forces_cases as fc
import np_eom as ne
import np_kinematics as nk

pytestmark = pytest.mark.gpu
ENVS = {"walker3d": "Walker3DStepperEnv-v0", "mike": "MikeStepperEnv-v0"}
N = 70
WIDTH = {"mass": 27 * 27, "forces": 3 * 27, "corner_jac": 8 * 3 * 27}
SHAPE = {"mass": (27, 27), "forces": (3, 27), "corner_jac": (8, 3, 27)}
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


def _call(e, ids, m, which=("mass", "forces", "corner_jac")):
    """ss_eom itself on pre-filled buffers with a canary tail: -> (rc, {name: int32 bit pattern [m * width + TAIL]})"""
    from steppingstone_amd.envs import _ptr, _stream
    bufs = {k: torch.full((max(m, 0) * WIDTH[k] + TAIL,), FILL, dtype=torch.int32, device="cuda:0") for k in which}
    dev_ids = None if ids is None else torch.as_tensor(ids, dtype=torch.int32).to("cuda:0")
    ptr = lambda k: _ptr(bufs[k]) if k in bufs else None
    rc = e.backend.lib.ss_eom(e.backend.h, None if dev_ids is None else _ptr(dev_ids), m, ptr("mass"), ptr("forces"), ptr("corner_jac"),
                              _stream(e.device))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in bufs.items()}


def _rows(buf, k, m):
    assert (buf[m * WIDTH[k]:] == FILL).all(), "the words behind %s were written" % k
    return buf[:m * WIDTH[k]].reshape(m, WIDTH[k])


def _floats(full):
    return {k: v.view(np.float32).reshape((v.shape[0],) + SHAPE[k]) for k, v in full.items()}


@pytest.fixture(scope="module", params=ec.KINDS)
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


def test_outputs_match_the_restatement(scene):
    kind, e, st, full = scene
    rows = st.cpu().numpy()
    assert not any((v == FILL).any() for v in full.values()), "a word of a valid row was not written"
    got = ne.split_outputs(_floats(full))
    m = ec.model(kind)
    refs = [ne.readout(m, r) for r in rows]
    over, worst = ec.outside(got, refs)
    print("eom device %s: worst err/(2^-24 B) per group: %s" % (kind, {g: float("%.4g" % w) for g, w in worst.items()}))
    assert set(worst) == set(ne.GROUPS) and not over, "%s: groups outside their K: %s" % (kind, over)
    assert np.array_equal(got["mass"], got["mass"].transpose(0, 2, 1)), "mass == mass^T bit for bit"
    assert (got["passive"][:, :6] == 0).all()
    host = ne.split_outputs(eh.eom(ec.KINDS.index(kind), rows))
    same = {k: float((host[k] == got[k]).mean()) for k in ne.GROUPS}
    print("eom device-vs-host %s: share of bit-equal words per group: %s" % (kind, {k: round(v, 3) for k, v in same.items()}))
    # the Python surface returns the same words
    d = e.equation_of_motion()
    for k in ne.GROUPS:
        assert torch.equal(d[k].cpu(), torch.from_numpy(np.ascontiguousarray(got[k]))), k


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
    buf = torch.full((N * WIDTH["mass"] + TAIL,), FILL, dtype=torch.int32, device="cuda:0")
    p = _ptr(buf)
    off = C.c_void_p(buf.data_ptr() + 4)
    assert lib.ss_eom(h, _ptr(ids), 4, None, None, None, s) == -1                 # all outputs NULL with m > 0
    assert lib.ss_eom(h, None, 4, p, None, None, s) == -1                         # NULL ids with m != N
    assert lib.ss_eom(h, None, N + 1, p, None, None, s) == -1
    for args in ((off, None, None), (None, off, None), (None, None, off), (p, off, p)):  # a misaligned pointer
        assert lib.ss_eom(h, _ptr(ids), 4, *args, s) == -1
    assert lib.ss_eom(h, _ptr(ids), -1, p, None, None, s) == -1                   # m < 0
    assert b"ss_eom" in lib.ss_last_error()
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == FILL).all()                                      # nothing was launched
    assert lib.ss_eom(h, None, N, p, None, None, s) == 0
    torch.cuda.synchronize()
    assert (_rows(buf.cpu().numpy(), "mass", N) == full["mass"]).all()


@pytest.mark.parametrize("kind", ec.KINDS)
def test_the_call_only_reads(kind):
    a, b = _env(kind, N), _env(kind, N)
    before = a.get_state().clone()
    a.equation_of_motion()
    a.equation_of_motion(env_ids=[5, 2], mass=False)
    assert torch.equal(a.get_state().view(torch.int32), before.view(torch.int32))
    act = (torch.rand((N, 21), generator=torch.Generator().manual_seed(9)) * 2 - 1).to("cuda:0")     # one action tensor for both
    outs = []
    for e in (a, b):
        obs, rew, done, _ = e.step(act)
        outs.append((obs.clone(), rew.clone(), done.clone(), e.get_state().clone()))
        e.close()
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


@pytest.mark.parametrize("kind", ec.KINDS)
def test_agrees_with_the_other_readouts_on_the_device(kind):
    """tests/test_eom.py's agreement with ss_kinematics and closing against ss_step_forces, all three kernels on one instance that
    holds forces_cases.cases(kind); the yardstick of the closing is recomputed from the device's own ss_step_forces output"""
    c = fc.cases(kind)
    n = c["st"].shape[0]
    e = _env(kind, n, seed=5, steps=0)
    e.set_state(torch.from_numpy(c["st"].copy()).to("cuda:0"))
    before = e.get_state().clone()
    np_ = lambda d: {k: v.cpu().numpy() for k, v in d.items()}
    got = np_(e.equation_of_motion())
    kin = np_(e.kinematics())
    new = lambda *shape: torch.empty((n,) + shape, dtype=torch.float32, device="cuda:0")
    contacts, joints = new(4, 8, 8), new(4, 4, 21)
    e.backend.step_forces(None, n, torch.from_numpy(c["act"].copy()).to("cuda:0"), contacts, joints, None)
    torch.cuda.synchronize()
    assert torch.equal(e.get_state().view(torch.int32), before.view(torch.int32))
    e.close()
    m = ec.model(kind)
    eom_refs = ec.closing_references(kind)
    kin_refs = [nk.readout(m, r) for r in c["st"]]
    over, worst = ec.outside(got, eom_refs)
    assert not over, "%s: groups outside their K: %s" % (kind, over)
    ec.judge_against_kinematics(kind, c["st"], got, kin, eom_refs, kin_refs)
    ec.judge_closing(kind, c["st"], dict(contacts=contacts.cpu().numpy(), joints=joints.cpu().numpy()), got, "eom device")
