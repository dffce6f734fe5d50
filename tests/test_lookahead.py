"""The look-ahead on the CPU: steppingstone_amd/csrc/ss_lookahead.hpp compiled for the host (tests/host/lookahead_host.cpp, lane threads,
the pair exchange and the wavefront barrier of the host harness) against the host build of step_env from the same library, stepped 24
times with auto-reset off, on the case set of tests/lookahead_cases.py.  Everything is compared bit for bit: no tolerance enters.
  * the case set reaches every branch of the env logic (conditions on the inputs, judged by step_env alone);
  * obs / rew / done up to each row's first done, final_state against the packed state; the frozen rows behind a first done;
  * the first H' steps of a longer call are the call with horizon H' (1, 7, 24);
  * the instance is left as it was; rows do not depend on m, their position, repeated ids or the outputs asked for."""
import numpy as np
import pytest

import lookahead_cases as lc
import lookahead_host_lib as lh
import native_build

pytestmark = pytest.mark.skipif(not native_build.hipcc(), reason="needs hipcc")
FILL = np.float32(-777.25)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def expected(ref, h):
    """what ss_lookahead must return for horizon h, from the real steps `ref` (lookahead_cases.step_reference over >= h steps)"""
    done = ref["done"][:, :h]
    n = done.shape[0]
    first = np.where(done.any(1), done.argmax(1), h)
    last = np.minimum(first, h - 1)                                  # the step whose results a later step repeats
    src = np.minimum(np.arange(h)[None, :], last[:, None])
    rows = np.arange(n)[:, None]
    frozen = np.arange(h)[None, :] > first[:, None]
    return dict(obs=ref["obs"][rows, src], rew=np.where(frozen, np.float32(0), ref["rew"][rows, src]).astype(np.float32),
                done=(done[rows, src] | frozen).astype(np.uint8), final_state=ref["state"][last, np.arange(n)], first=first, frozen=frozen)


@pytest.fixture(scope="module", params=lc.KINDS)
def scene(request):
    kind = request.param
    c = lc.cases(kind)
    ref = lc.step_reference(kind, c["st"], c["act"])
    out = lh.lookahead(lc.KINDS.index(kind), c["st"], c["act"], seed=lc.SEED, curriculum=lc.CURRICULUM, state_after=True)
    return kind, c, ref, out


def test_case_set_reaches_every_branch_of_the_env_logic(scene):
    kind, c, ref, out = scene
    ev = lc.events(kind, c["st"], c["act"])
    print(kind, {k: v for k, v in ev.items() if k != "first"})
    assert ev["draws"] >= 8 and ev["last_stone"] >= 1 and ev["touches"] >= 8 and ev["falls"] >= 8
    assert ev["time_limit"] >= 1 and ev["nan"] >= 1 and ev["alive"] >= 8


def test_rows_are_the_steps_bit_for_bit(scene):
    kind, c, ref, out = scene
    want = expected(ref, lc.H)
    live = ~want["frozen"]
    assert live.sum() > 1000 and want["frozen"].sum() > 100
    for k in ("obs", "rew", "done"):
        assert (bits(out[k])[live] == bits(want[k])[live]).all(), k
    bad = bits(out["final_state"]) != bits(want["final_state"])
    assert not bad.any(), "final_state differs from the packed state in words %s" % np.unique(np.nonzero(bad)[1])
    assert not (bits(want["final_state"]) == bits(c["st"])).all(1).any()


def test_rows_behind_the_first_done_are_frozen(scene):
    kind, c, ref, out = scene
    want = expected(ref, lc.H)
    fr = want["frozen"]
    assert (out["done"][fr] == 1).all() and (bits(out["rew"])[fr] == 0).all(), "a finished branch is done and earns exactly +0.0"
    assert (bits(out["obs"])[fr] == bits(want["obs"])[fr]).all(), "a finished branch repeats its terminal observation"
    assert (out["done"] <= 1).all()


@pytest.mark.parametrize("h", [1, 7, 24])
def test_a_shorter_horizon_is_a_prefix(scene, h):
    kind, c, ref, out = scene
    got = lh.lookahead(lc.KINDS.index(kind), c["st"], c["act"][:, :h], seed=lc.SEED, curriculum=lc.CURRICULUM)
    for k in ("obs", "rew", "done"):
        assert (bits(got[k]) == bits(out[k][:, :h])).all(), k
    want = expected(ref, h)
    for k in ("obs", "rew", "done", "final_state"):
        assert (bits(got[k]) == bits(want[k])).all(), k


def test_the_instance_is_left_as_it_was(scene):
    kind, c, ref, out = scene
    assert (bits(out["state"]) == bits(c["st"])).all()


def test_rows_do_not_depend_on_position_repeats_or_requested_outputs(scene):
    kind, c, ref, out = scene
    k = lc.KINDS.index(kind)
    ids = np.array([5, 40, 5, -1, 63, 2, 64, 40, 3], np.int32)              # 9 rows: part of a wavefront; two ids out of range
    good = (ids >= 0) & (ids < lc.N_CASES)
    act = c["act"][np.where(good, ids, 0)].copy()
    act[2] = c["act"][41]                                                    # the second branch of env 5 under other actions
    full = lh.lookahead(k, c["st"], act, env_ids=ids, seed=lc.SEED, curriculum=lc.CURRICULUM, state_after=True, fill=FILL)
    assert (bits(full["state"]) == bits(c["st"])).all()
    for name in ("obs", "rew", "done", "final_state"):
        rows = bits(full[name])
        for r, i in enumerate(ids):
            if not good[r]:
                assert (full[name][r] == (FILL if name != "done" else lh.DONE_FILL)).all(), "row %d of %s (id %d) was written" % (r, name, i)
            elif r != 2:
                assert (rows[r] == bits(out[name])[i]).all(), "%s row %d (id %d)" % (name, r, i)
    assert not (bits(full["rew"][2]) == bits(full["rew"][0])).all()
    for obs, fs in ((False, False), (True, False), (False, True)):
        part = lh.lookahead(k, c["st"], act, env_ids=ids, seed=lc.SEED, curriculum=lc.CURRICULUM, obs=obs, final_state=fs, fill=FILL)
        for name in part:
            assert (bits(part[name]) == bits(full[name])).all(), (name, obs, fs)
    assert lh.lookahead(k, c["st"], np.zeros((0, 3, 21), np.float32), env_ids=np.zeros(0, np.int32))["rew"].shape == (0, 3)
