"""ss_step_forces on the GPU (docs/PHYSICS.md 10): both robots, the case set of tests/forces_cases.py tiled onto N = 70 envs (three
wavefronts of 32 rows, the last with 6), auto-reset off.
  * next_state is, bit for bit, the state ss_step leaves (the library's default kernel variant at 70 envs, and the 4096-env variant);
  * the call only reads: the state and the next step's results are as without it;
  * a row's bits do not depend on the batch size, its position, the ids' order, a repeated id or the outputs asked for; rows of ids
    outside [0, N) and the words behind each buffer are never written;
  * substep 0 agrees with ss_kinematics on the carriers; cone, zeros and world vector; the fp64 oracle; joint torques; the C API.
The clause "-pen equals corners word 6 bit for bit where slot 1 carries" holds on the case set without a witness: three steps after a
reset the robot stands on stone n-1, no corner is carried by slot 1.  With the stones n-1 and n swapped under the robot the CPU builds of
the two readouts give 68 .. 115 such corners per set and differ by up to 2.8e-7 m (15 of 68 bit-equal at best): ss_kinematics walks each
body's chain in the world frame (render::walk_chain), the detection composes rotations link by link (fk_detect), two roundings of one
number.  test_carriers_on_swapped_stones holds what is exact there, the carriers, and prints the distance."""
import ctypes as C
import itertools
import time

import numpy as np
import pytest
import torch

import forces_cases as fc
import oracle_lib as ol

pytestmark = pytest.mark.gpu
ENVS = {"walker3d": "Walker3DStepperEnv-v0", "mike": "MikeStepperEnv-v0"}
N = 70
WIDTH = {"contacts": 4 * 8 * 8, "joints": 4 * 4 * 21, "next_state": 56}
NAMES = tuple(WIDTH)
FILL = 0x5A5A5A5A
TAIL = 64                       # canary words behind each buffer
SRC = np.arange(N) % fc.N_ENVS  # env e of the 70 holds case e % 64


def _env(kind, n, seed=11):
    from steppingstone_amd.envs import SteppingStoneVecEnv
    e = SteppingStoneVecEnv(ENVS[kind], n, seed=seed, device="cuda:0", return_numpy=False)
    e.update_curriculum(5)
    e.set_auto_reset(False)
    e.reset()
    return e


def _call(e, ids, m, act, which=NAMES):
    """ss_step_forces itself on pre-filled buffers with a canary tail: -> (rc, {name: int32 bit pattern [m * width + TAIL]})"""
    from steppingstone_amd.envs import _ptr, _stream
    bufs = {k: torch.full((max(m, 0) * WIDTH[k] + TAIL,), FILL, dtype=torch.int32, device="cuda:0") for k in which}
    dev_ids = None if ids is None else torch.as_tensor(ids, dtype=torch.int32).to("cuda:0")
    dev_act = None if act is None else torch.from_numpy(np.array(act, np.float32)).to("cuda:0")
    ptr = lambda k: _ptr(bufs[k]) if k in bufs else None
    rc = e.backend.lib.ss_step_forces(e.backend.h, None if dev_ids is None else _ptr(dev_ids), m, None if dev_act is None else _ptr(dev_act),
                                      ptr("contacts"), ptr("joints"), ptr("next_state"), _stream(e.device))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in bufs.items()}


def _rows(buf, k, m):
    assert (buf[m * WIDTH[k]:] == FILL).all(), "the words behind %s were written" % k
    return buf[:m * WIDTH[k]].reshape(m, WIDTH[k])


def _as_float(full, n=N):
    return {"contacts": full["contacts"].view(np.float32).reshape(n, 4, 8, 8), "joints": full["joints"].view(np.float32).reshape(n, 4, 4, 21),
            "next_state": full["next_state"].view(np.float32).reshape(n, 56)}


@pytest.fixture(scope="module", params=fc.KINDS)
def scene(request):
    """(kind, env holding the 70 states, states [70,186] as a device tensor, actions [70,21], the whole batch's outputs as bit patterns)"""
    kind = request.param
    c = fc.cases(kind)
    e = _env(kind, N)
    st = torch.from_numpy(c["st"][SRC].copy()).to("cuda:0")
    act = c["act"][SRC].copy()
    e.set_state(st)
    rc, out = _call(e, None, N, act)
    assert rc == 0
    yield kind, e, st, act, {k: _rows(v, k, N) for k, v in out.items()}
    e.close()


@pytest.mark.parametrize("n", [N, 4096])
@pytest.mark.parametrize("kind", fc.KINDS)
def test_next_state_is_the_step_itself_bit_for_bit(kind, n):
    """70 envs: the library's default kernel variant there; 4096: the size where the helper variant runs"""
    t0 = time.perf_counter()
    c = fc.cases(kind)
    src = np.arange(n) % fc.N_ENVS
    e = _env(kind, n)
    st = torch.from_numpy(c["st"][src].copy()).to("cuda:0")
    act = torch.from_numpy(c["act"][src].copy()).to("cuda:0")
    e.set_state(st)
    before = e.get_state().clone()
    dry = e.step_forces(act)
    e.step(act)
    after = e.get_state()
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(dry["next_state"]), bits(after[:, 0:55]))
    flags = after[:, 64].to(torch.int32)
    assert torch.equal(dry["next_contact"], torch.stack([flags & 1, (flags >> 1) & 1], 1).bool())
    assert torch.equal(bits(dry["joint_q"][:, 0]), bits(before[:, 13:34])) and torch.equal(bits(dry["joint_qd"][:, 0]), bits(before[:, 34:55]))
    assert bool(dry["next_contact"].any()) and not torch.equal(bits(after[:, 0:55]), bits(before[:, 0:55]))
    e.close()
    print("bitwise against the step, %s, %d envs: %.2f s" % (kind, n, time.perf_counter() - t0))


@pytest.mark.parametrize("kind", fc.KINDS)
def test_the_call_only_reads(kind):
    c = fc.cases(kind)
    st = torch.from_numpy(c["st"][SRC].copy()).to("cuda:0")
    act = torch.from_numpy(c["act"][SRC].copy()).to("cuda:0")
    a, b = _env(kind, N), _env(kind, N)
    outs = []
    for e, dry in ((a, True), (b, False)):
        e.set_state(st)
        before = e.get_state().clone()
        if dry:
            e.step_forces(act)
            e.step_forces(act[[5, 2]], env_ids=[5, 2], joints=False)
            assert torch.equal(e.get_state().view(torch.int32), before.view(torch.int32)), "step_forces changed the state"
        obs, rew, done, _ = e.step(act)
        outs.append((obs.clone(), rew.clone(), done.clone(), e._info.clone(), e.get_state().clone()))
        e.close()
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


def test_rows_do_not_depend_on_batch_position_ids_or_requested_outputs(scene):
    kind, e, st, act, full = scene
    rng = np.random.default_rng(5)
    subsets = [s for r in (1, 2, 3) for s in itertools.combinations(NAMES, r)]

    def check(env, ids, row_of, which=NAMES):
        a = np.stack([act[row_of[i]] if i in row_of else np.zeros(21, np.float32) for i in ids])
        rc, out = _call(env, ids, len(ids), a, which)
        assert rc == 0
        for k in which:
            rows = _rows(out[k], k, len(ids))
            for r, i in enumerate(ids):
                if i in row_of:
                    assert (rows[r] == full[k][row_of[i]]).all(), "%s row %d (id %d) differs: ids %s, outputs %s" % (k, r, i, ids[:8], which)
                else:
                    assert (rows[r] == FILL).all(), "row %d (id %d) of %s was written" % (r, i, k)
    same = {i: i for i in range(N)}
    for ids in ([37], list(range(33)), list(range(N))[::-1], [3, 3, 69, 3, 64, 69], list(rng.permutation(N)[:40]),
                [3, -1, 64, N, 69, -1, N + 1000, 0]):                 # ids -1, N and beyond, mixed in, leave their rows as they were
        check(e, [int(i) for i in ids], same)
    for which in subsets:                                          # every subset of the outputs
        check(e, [69, 0, 64, -1, 31, 32], same, which)
    # the same states inside instances of 1, 64 and 130 envs: (size, rows of the 70 injected, at which positions)
    for n2, src, pos in [(1, [37], [0]), (1, [69], [0]), (64, list(range(69, 5, -1)), list(range(64))), (130, list(range(N)), list(range(60, 130)))]:
        e2 = _env(kind, n2)
        e2.set_state(st[src], env_ids=pos)
        row_of = dict(zip(pos, src))
        ids = [int(i) for i in rng.permutation(pos)]
        check(e2, ids + ids[:1], row_of)
        e2.close()


def test_substep_0_agrees_with_the_kinematic_readout(scene):
    kind, e, st, act, full = scene
    co = e.kinematics(twists=False, summary=False)
    c0 = _as_float(full)["contacts"][:, 0]
    carrier = co["corner_carrier"].cpu().numpy()
    assert (c0[..., 0] == carrier).all() and (carrier >= 0).any()
    on = c0[..., 0] >= 0
    assert ((-c0[..., 1][on] > -0.10) & (-c0[..., 1][on] < 0)).all()
    one = c0[..., 0] == 1
    h = co["corner_height"].cpu().numpy()
    print("%s: corners carried at substep 0: %d, by slot 1: %d" % (kind, int(on.sum()), int(one.sum())))
    assert ((-c0[..., 1][one]).view(np.int32) == h[one].view(np.int32)).all()


@pytest.mark.parametrize("kind", fc.KINDS)
def test_carriers_on_swapped_stones(kind):
    """stones n-1 and n change places under the robot, so that slot 1 carries: the carriers of substep 0 are ss_kinematics' exactly"""
    c = fc.cases(kind)
    st = c["st"][SRC].copy()
    terr = st[:, ol.S_TERRAIN].reshape(N, 20, 6).copy()
    terr[:, [0, 1]] = terr[:, [1, 0]]
    st[:, ol.S_TERRAIN] = terr.reshape(N, 120)
    e = _env(kind, N)
    e.set_state(torch.from_numpy(st).to("cuda:0"))
    dry = e.step_forces(torch.from_numpy(c["act"][SRC].copy()).to("cuda:0"), joints=False)
    co = e.kinematics(twists=False, summary=False)
    slot = dry["contact_slot"][:, 0].cpu().numpy()
    assert (slot == co["corner_carrier"].cpu().numpy()).all() and (slot == 1).sum() >= 32
    one = slot == 1
    d = np.abs(-dry["contact_pen"][:, 0].cpu().numpy()[one].astype(np.float64) - co["corner_height"].cpu().numpy()[one])
    last = dry["contact_slot"][:, 3].cpu().numpy().reshape(N, 2, 4)
    on_target = dry["next_on_target"].cpu().numpy()
    assert (on_target == (last == 1).any(2)).all() and on_target.any(), "the target flags are the last detection's slot-1 carriers"
    assert (dry["next_contact"].cpu().numpy() == (last >= 0).any(2)).all()
    print("%s, stones swapped: %d corners carried by slot 1, |-pen - corner height| at most %.3g m" % (kind, int(one.sum()), d.max()))
    e.close()


def test_cone_zeros_and_world_vector(scene):
    kind, e, st, act, full = scene
    got = _as_float(full)
    fc.judge_cone_and_zeros(kind, got["contacts"], st.cpu().numpy(), "device")
    assert (fc.judge_flags(got["contacts"], got["next_state"]) & 3).any()


@pytest.mark.parametrize("kind", fc.KINDS)
def test_tilted_stones(kind):
    c = fc.tilted_cases(kind)
    e = _env(kind, fc.N_ENVS)
    e.set_state(torch.from_numpy(c["st"].copy()).to("cuda:0"))
    rc, out = _call(e, None, fc.N_ENVS, c["act"])
    assert rc == 0
    got = _as_float({k: _rows(v, k, fc.N_ENVS) for k, v in out.items()}, fc.N_ENVS)
    e.close()
    assert (got["contacts"][..., 0] >= 0).sum() >= 64
    fc.judge_cone_and_zeros(kind, got["contacts"], c["st"], "device, tilted stones")
    fc.judge_joint_torques(kind, got["joints"], got["next_state"], c["act"], "device, tilted stones")


def test_forces_against_the_fp64_oracle(scene):
    kind, e, st, act, full = scene
    fc.judge_against_oracle(kind, _as_float(full)["contacts"][:fc.N_ENVS], "device")


def test_joint_torques(scene):
    kind, e, st, act, full = scene
    got = _as_float(full)
    fc.judge_joint_torques(kind, got["joints"], got["next_state"], act, "device")


def test_bad_arguments_are_refused_and_m_0_does_nothing(scene):
    from steppingstone_amd.envs import _ptr, _stream
    kind, e, st, act, full = scene
    lib, h, s = e.backend.lib, e.backend.h, _stream(e.device)
    ids = torch.arange(4, dtype=torch.int32, device="cuda:0")
    a = torch.from_numpy(act).to("cuda:0")
    buf = torch.full((N * WIDTH["joints"] + TAIL,), FILL, dtype=torch.int32, device="cuda:0")
    p = _ptr(buf)
    off = C.c_void_p(buf.data_ptr() + 4)
    assert lib.ss_step_forces(h, _ptr(ids), 4, _ptr(a), None, None, None, s) == -1             # all outputs NULL with m > 0
    assert lib.ss_step_forces(h, _ptr(ids), -1, _ptr(a), None, p, None, s) == -1               # m < 0
    assert lib.ss_step_forces(h, None, 4, _ptr(a), None, p, None, s) == -1                     # NULL ids with m != N
    assert lib.ss_step_forces(h, None, N + 1, _ptr(a), None, p, None, s) == -1
    assert lib.ss_step_forces(h, _ptr(ids), 4, None, None, p, None, s) == -1                   # no actions with m > 0
    for args in ((off, None, None), (None, off, None), (None, None, off), (p, off, p)):        # a misaligned output
        assert lib.ss_step_forces(h, _ptr(ids), 4, _ptr(a), *args, s) == -1
    assert b"ss_step_forces" in lib.ss_last_error()
    assert lib.ss_step_forces(h, _ptr(ids), 0, _ptr(a), None, p, None, s) == 0                 # m == 0 is fine, whatever else
    assert lib.ss_step_forces(h, None, 0, None, None, None, None, s) == 0
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == FILL).all()                                                   # nothing was launched
    assert lib.ss_step_forces(h, None, N, _ptr(a), None, p, None, s) == 0
    torch.cuda.synchronize()
    assert (_rows(buf.cpu().numpy(), "joints", N) == full["joints"]).all()


def test_capture_into_a_graph_next_to_a_step(scene):
    """one graph, one linear stream: the dry run, then the step it predicts; replayed from a second state"""
    kind, e, st, act, full = scene
    c = fc.cases(kind)
    e2 = _env(kind, N)
    a = torch.from_numpy(act).to("cuda:0")
    co = torch.zeros((N, 4, 8, 8), device="cuda:0")
    jo = torch.zeros((N, 4, 4, 21), device="cuda:0")
    ns = torch.zeros((N, 56), device="cuda:0")
    obs, rew = torch.zeros((N, 60), device="cuda:0"), torch.zeros(N, device="cuda:0")
    done, info = torch.zeros(N, dtype=torch.uint8, device="cuda:0"), torch.zeros((N, 6), dtype=torch.int32, device="cuda:0")
    e2.set_state(st)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                     # (warm-up outside the capture, as torch asks for)
        e2.backend.step_forces(None, N, a, co, jo, ns)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        e2.backend.step_forces(None, N, a, co, jo, ns)
        e2.backend.step(a, obs, rew, done, info)
    for rows in (SRC, SRC[::-1].copy()):
        state = torch.from_numpy(c["st"][rows].copy()).to("cuda:0")
        a.copy_(torch.from_numpy(c["act"][rows].copy()))
        e2.set_state(state)
        g.replay()
        torch.cuda.synchronize()
        after = e2.get_state()
        assert torch.equal(ns[:, :55].contiguous().view(torch.int32), after[:, :55].contiguous().view(torch.int32))
        want = full["joints"] if rows is SRC else full["joints"][::-1]
        assert (jo.cpu().numpy().view(np.int32).reshape(N, -1) == want).all()
    e2.close()
