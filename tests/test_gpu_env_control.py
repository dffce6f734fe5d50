"""Per-env episode control on the MI355X: ss_reset_masked, ss_get_state_envs / ss_set_state_envs and what SteppingStoneVecEnv builds on
them.  The rule that holds them together: stepping with auto-reset off and resetting the finished envs behind each step gives exactly
the bits of stepping with auto-reset on.  Curriculum 5 and random actions make falls frequent; a quarter of the envs start two steps
short of the time limit, so that time-limit ends (bad_transition) are in the sample too."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ENV_IDS = ["Walker3DStepperEnv-v0", "MikeStepperEnv-v0"]
N = 256
STEPS = 200


@contextlib.contextmanager
def helpers(h):
    old = os.environ.get("SS_HELPERS")
    os.environ["SS_HELPERS"] = h
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SS_HELPERS", None)
        else:
            os.environ["SS_HELPERS"] = old


def make(env_id, n=N, seed=11, **kw):
    from steppingstone_amd.envs import SteppingStoneVecEnv
    e = SteppingStoneVecEnv(env_id, n, seed=seed, device="cuda:0", **kw)
    e.update_curriculum(5)
    e.reset()
    return e


def start_state(env):
    """The reset state with elapsed = 998 (state word 61) in a quarter of the envs."""
    st = env.get_state().clone()
    st[: env.num_envs // 4, 61] = 998.0
    return st


def describe_obs_mismatch(a, b):
    bad = (a != b) & ~(torch.isnan(a) & torch.isnan(b))
    cols = torch.nonzero(bad.any(0)).flatten().tolist()
    return "obs entries differ: %s (max |diff| %s)" % (cols, [float((a[:, c] - b[:, c]).abs().max()) for c in cols])


@pytest.mark.parametrize("env_id", ENV_IDS)
def test_reset_of_finished_envs_equals_auto_reset(env_id):
    """Env A auto-resets inside the step; env B steps with auto-reset off and calls reset(done) after every step.  Every step's
    obs / rew / done / info words and the state at checkpoints must be equal, for every kernel variant (SS_HELPERS 0, 1, 3)."""
    for h in ("0", "1", "3"):
        with helpers(h):
            A, B = make(env_id), make(env_id)
        B.set_auto_reset(False)
        st = start_state(A)
        A.set_state(st)
        B.set_state(st)
        finished = timeouts = 0
        for t in range(STEPS):
            a = A.random_actions(t)
            oa, ra, da, _ = A.step(a)
            ob, rb, db, _ = B.step(a)
            assert torch.equal(ra, rb) and torch.equal(da, db), (h, t)
            assert torch.equal(A._info, B._info), (h, t)            # all six ss_info words, bitwise
            B.reset(db)
            assert torch.equal(oa, ob), (h, t, describe_obs_mismatch(oa, ob))
            finished += int(da.sum())
            timeouts += int(A._info[:, 2].sum())
            if t % 50 == 49:
                assert torch.equal(A.get_state(), B.get_state()), (h, t)
        assert finished >= 300 and timeouts >= N // 8, (finished, timeouts)
        A.close()
        B.close()


@pytest.mark.parametrize("env_id", ENV_IDS)
def test_keep_terminal_obs_matches_auto_reset_and_reports_the_terminal_rows(env_id):
    """keep_terminal_obs=True (tensor mode, and numpy mode through the pinned packed path): obs / rew / done / info / state bitwise those
    of auto-reset; the terminal rows are the rows an env with auto-reset off returned before its reset."""
    A, B = make(env_id), make(env_id)
    K = make(env_id, keep_terminal_obs=True)
    P = make(env_id, keep_terminal_obs=True, return_numpy=True)
    B.set_auto_reset(False)
    st = start_state(A)
    for e in (A, B, K, P):
        e.set_state(st)
    finished = 0
    for t in range(STEPS):
        a = A.random_actions(t)
        oa, ra, da, _ = A.step(a)
        ob, rb, db, _ = B.step(a)
        terminal = ob.clone()
        B.reset(db)
        ok, rk, dk, ik = K.step(a)
        assert torch.equal(ok, oa) and torch.equal(rk, ra) and torch.equal(dk, da) and torch.equal(K._info, A._info), t
        assert torch.equal(ik["terminal_obs"][da], terminal[da]), t
        op, rp, dp, ip = P.step(a.cpu().numpy())
        assert np.array_equal(op, oa.cpu().numpy()) and np.array_equal(rp, ra.cpu().numpy().astype(np.float64)), t
        assert np.array_equal(dp, da.cpu().numpy()) and np.array_equal(P._info_host, A._info.cpu().numpy()), t
        term_host = terminal.cpu().numpy()
        for i, info in enumerate(ip):
            if dp[i]:
                assert info["terminal_observation"].dtype == np.float32 and np.array_equal(info["terminal_observation"], term_host[i])
            else:
                assert "terminal_observation" not in info
        finished += int(da.sum())
        if t % 50 == 49:
            s = A.get_state()
            assert torch.equal(K.get_state(), s) and torch.equal(P.get_state(), s), t
    assert finished >= 300, finished


@pytest.mark.parametrize("env_id", ENV_IDS)
def test_partial_reset_touches_only_the_named_envs(env_id):
    E = make(env_id)
    for t in range(30):
        E.step(E.random_actions(t))
    snap = E.get_state().clone()
    ids = [200, 3, 77, 0, N - 1, 128]
    sel = torch.zeros(N, dtype=torch.bool, device="cuda:0")
    sel[ids] = True
    # the reset rows: those of a full reset of a copy restored from the same snapshot
    R = make(env_id)
    R.set_state(snap)
    full_obs = R.reset().clone()
    full = R.get_state()
    results = []
    for form in (ids, torch.tensor(ids, dtype=torch.int64, device="cuda:0"), sel, sel.to(torch.uint8)):
        E.set_state(snap)
        out = E.reset(form)
        after = E.get_state()
        assert torch.equal(after[~sel], snap[~sel])                   # every other env unchanged, bit for bit
        assert torch.equal(after[sel], full[sel])
        rows = out if out.shape[0] == len(ids) else out[ids]          # the mask form returns all N rows
        assert torch.equal(rows, full_obs[ids]) and torch.equal(E._obs[ids], full_obs[ids])
        results.append((rows.clone(), after.clone()))
    assert all(torch.equal(a, b) for r in results[1:] for a, b in zip(results[0], r))


@pytest.mark.parametrize("env_id", ENV_IDS)
def test_subset_state_get_and_set(env_id):
    E, F = make(env_id), make(env_id, seed=99)
    for t in range(25):
        E.step(E.random_actions(t))
        F.step(F.random_actions(t + 1000))
    full = E.get_state().clone()
    ids = [9, 250, 2, 130]
    assert torch.equal(E.get_state(ids), full[ids])
    assert torch.equal(E.get_state(torch.tensor(ids, device="cuda:0")), full[ids])
    rows = F.get_state([1, 4, 7, 255])
    E.set_state(rows, ids)
    want = full.clone()
    want[ids] = rows
    assert torch.equal(E.get_state(), want)
    R = make(env_id)
    R.set_state(want)
    assert torch.equal(E.get_obs(), R.get_obs())


def test_step_and_mask_reset_capture():
    """step() followed by reset(done) captured into a graph and replayed: bitwise the same steps run eagerly."""
    env_id = ENV_IDS[0]
    G, E = make(env_id), make(env_id)
    for e in (G, E):
        e.set_auto_reset(False)
    st = start_state(E)
    G.set_state(st)
    E.set_state(st)
    act = torch.zeros((N, 21), device="cuda:0")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):              # warm-up step outside the capture, the same on both envs
        act.copy_(E.random_actions(0))
        G.reset(G.step(act)[2])
    torch.cuda.current_stream().wait_stream(side)
    E.reset(E.step(act)[2])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, _, done, _ = G.step(act)
        G.reset(done)
    finished = 0
    for t in range(1, 80):
        act.copy_(E.random_actions(t))
        graph.replay()
        oe, re, de, _ = E.step(act)
        E.reset(de)
        torch.cuda.synchronize()
        assert torch.equal(G._obs, oe) and torch.equal(G._rew, re) and torch.equal(G._done, E._done) and torch.equal(G._info, E._info), t
        finished += int(de.sum())
    assert torch.equal(G.get_state(), E.get_state())
    assert finished >= 100, finished


def test_argument_checks_through_ctypes():
    from steppingstone_amd import _lib
    E = make(ENV_IDS[0], n=64)
    lib, h = _lib.load(), E.backend.h
    p = lambda t: C.c_void_p(t.data_ptr())
    mask = torch.ones(64, dtype=torch.uint8, device="cuda:0")
    ids = torch.arange(4, dtype=torch.int32, device="cuda:0")
    packed = torch.zeros((4, 186), device="cuda:0")
    term = torch.zeros((64, 60), device="cuda:0")
    before = E.get_state().clone()
    assert lib.ss_reset_masked(h, None, p(E._obs), 60, None, None) == -1             # null mask
    assert lib.ss_reset_masked(h, p(mask), p(E._obs), 61, None, None) == -1          # stride neither 60 nor 62
    assert lib.ss_reset_masked(h, p(mask), None, 60, p(term), None) == -1            # terminal rows without obs to copy from
    assert lib.ss_reset_masked(None, p(mask), p(E._obs), 60, None, None) == -1
    assert lib.ss_get_state_envs(h, p(ids), -1, p(packed), None) == -1               # m < 0
    assert lib.ss_set_state_envs(h, p(ids), -1, p(packed), None) == -1
    assert lib.ss_get_state_envs(h, p(ids), 4, None, None) == -1                     # null packed with m > 0
    assert lib.ss_set_state_envs(h, p(ids), 4, None, None) == -1
    assert lib.ss_get_state_envs(h, None, 0, None, None) == 0                        # m == 0: nothing to do
    torch.cuda.synchronize()
    assert torch.equal(E.get_state(), before)
