"""The look-ahead from caller-supplied state rows on the CPU (docs/PHYSICS.md 13, "Branches from caller-supplied states"):
look_row<Model, true> and obs_from_row of steppingstone_amd/csrc/ss_lookahead.hpp compiled for the host (tests/host/
lookahead_states_host.cpp) against the host build of ss_lookahead from the same library, on the case set of tests/lookahead_cases.py.
Everything is compared bit for bit: no tolerance enters.
  (a) transplant: an instance that does not hold the case states, called with states = st, gives the rows of ss_lookahead on an
      instance that holds st, and is left as it was;
  (b) chain: lookahead(H = 8, final_state) then lookahead_states(final_state, act[:, 8:]) is steps 8..23 of one 24-step look-ahead;
  (c) the id is part of the branch: one state row under two ids draws different stones, each as its transplant does;
  (d) observe(states) is get_obs after set_state;
  (e) containment: rows that no ss_step state looks like write nothing outside their rows -- here with canary tails, and as a
      stand-alone program under AddressSanitizer and UBSan."""
import subprocess

import numpy as np
import pytest

import lookahead_cases as lc
import lookahead_states_host_lib as lhs
import native_build

pytestmark = pytest.mark.skipif(not native_build.hipcc(), reason="needs hipcc")
CUT = 8
OUTS = ("obs", "rew", "done", "final_state")
# witnesses of the chain test: rows unfinished after CUT steps, of those the rows that advance a target / finish in steps CUT..23.  The
# CPU build of step_env counts 59 / 34 / 14 (Walker3D) and 62 / 39 / 26 (Mike); the floors keep a test that compares nothing from passing
FLOORS = (56, 30, 10)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(got, want, rows=None, what=""):
    for k in OUTS:
        a, b = bits(got[k]), bits(want[k])
        if rows is not None:
            a, b = a[rows], b[rows]
        bad = np.nonzero((a != b).reshape(a.shape[0], -1).any(1))[0]
        assert bad.size == 0, "%s: %s differs in rows %s" % (what, k, bad[:12].tolist())


@pytest.fixture(scope="module", params=lc.KINDS)
def scene(request):
    """kind, its index, the cases, ss_lookahead over 24 steps on an instance that holds the case states"""
    kind = request.param
    k = lc.KINDS.index(kind)
    c = lc.cases(kind)
    full = lhs.lookahead(k, c["st"], c["act"], seed=lc.SEED, curriculum=lc.CURRICULUM)
    assert full["tails_ok"]
    return kind, k, c, full


def test_transplant(scene):
    kind, k, c, full = scene
    other = np.roll(c["st"], 17, 0)                                   # env i holds case i - 17: not the state its row starts from
    assert not (bits(other) == bits(c["st"])).all(1).any()
    got = lhs.lookahead(k, other, c["act"], states=c["st"], seed=lc.SEED, curriculum=lc.CURRICULUM, fill=-777.25)
    assert got["tails_ok"]
    same(got, full, what="%s, states = st on an instance that holds other states" % kind)
    assert (bits(got["state"]) == bits(other)).all(), "the instance changed"
    assert not (bits(full["final_state"]) == bits(c["st"])).all(1).any()


def test_chain(scene):
    kind, k, c, full = scene
    act = c["act"]
    head = lhs.lookahead(k, c["st"], act[:, :CUT], seed=lc.SEED, curriculum=lc.CURRICULUM)
    other = np.roll(c["st"], 17, 0)
    tail = lhs.lookahead(k, other, act[:, CUT:], states=head["final_state"], seed=lc.SEED, curriculum=lc.CURRICULUM)
    assert head["tails_ok"] and tail["tails_ok"]
    open_ = ~head["done"].astype(bool).any(1)
    advance = open_ & (full["final_state"][:, lc.S_N] > head["final_state"][:, lc.S_N])
    finish = open_ & full["done"][:, CUT:].astype(bool).any(1)
    print("%s: %d rows unfinished after %d steps, %d of them advance, %d finish in steps %d..%d" %
          (kind, open_.sum(), CUT, advance.sum(), finish.sum(), CUT, lc.H - 1))
    assert all(int(x.sum()) >= f for x, f in zip((open_, advance, finish), FLOORS)), "the chain test lost its witnesses"
    want = dict(obs=full["obs"][:, CUT:], rew=full["rew"][:, CUT:], done=full["done"][:, CUT:], final_state=full["final_state"])
    same(tail, want, rows=open_, what="%s, steps %d..%d from final_state" % (kind, CUT, lc.H - 1))
    for name in ("obs", "rew", "done"):
        assert (bits(head[name]) == bits(full[name][:, :CUT])).all()


def test_the_id_is_part_of_the_branch(scene):
    kind, k, c, full = scene
    n = lc.N_CASES
    ids = (np.arange(n, dtype=np.int32) + 1) % n                       # row r: the state and actions of case r under id r + 1
    got = lhs.lookahead(k, c["st"], c["act"], env_ids=ids, states=c["st"], seed=lc.SEED, curriculum=lc.CURRICULUM)
    # its transplant: ss_lookahead on an instance whose env r + 1 holds case r
    want = lhs.lookahead(k, np.roll(c["st"], 1, 0), c["act"], env_ids=ids, seed=lc.SEED, curriculum=lc.CURRICULUM)
    same(got, want, what="%s, ids shifted by one" % kind)
    own = lhs.lookahead(k, np.roll(c["st"], 1, 0), c["act"], states=c["st"], seed=lc.SEED, curriculum=lc.CURRICULUM)
    same(own, full, what="%s, own ids" % kind)
    n0, n1 = c["st"][:, lc.S_N], full["final_state"][:, lc.S_N]
    drew = (n1 > n0) & (n0 <= 17)                                      # the first advance drew stone n0 + 2
    assert (got["final_state"][:, lc.S_N] == n1)[drew].all()
    terr = lambda o: bits(o["final_state"])[:, 65:185]
    differ = (terr(got) != terr(full)).any(1)
    print("%s: %d rows drew a stone, %d differ between the two ids" % (kind, drew.sum(), differ.sum()))
    assert drew.sum() >= 8 and differ[drew].all(), "a stone drawn under another id is the same stone"


def test_observe_is_get_obs_after_set_state(scene):
    kind, k, c, full = scene
    head = lhs.lookahead(k, c["st"], c["act"][:, :CUT], seed=lc.SEED, curriculum=lc.CURRICULUM)
    for name, st in (("the case states", c["st"]), ("the final_state rows of the first %d steps" % CUT, head["final_state"])):
        got, want = lhs.observe(k, st), lhs.get_obs(k, st)
        assert (bits(got) == bits(want)).all(), name
        assert np.unique(bits(got), axis=0).shape[0] >= 60
    # ... and what a branch from the row would see next is a step away from it, not the row's own observation
    assert not (bits(lhs.observe(k, c["st"])) == bits(full["obs"][:, 0])).all(1).any()


def spoilt_rows(st):
    """the case states with every odd row spoilt: word 59 = 1e9, -5, NaN; dynamic words all NaN, all +-Inf -> rows, non-finite mask"""
    rows = st.copy()
    nonfinite = np.zeros(rows.shape[0], bool)
    for r in range(1, rows.shape[0], 2):
        what = (r // 2) % 5
        if what < 3:
            rows[r, 59] = (1e9, -5.0, np.nan)[what]
        else:
            rows[r, :55] = np.nan if what == 3 else np.where(np.arange(55) % 2, np.inf, -np.inf)
            nonfinite[r] = True
    return rows, nonfinite


def test_containment_with_canary_tails(scene):
    kind, k, c, full = scene
    rows, nonfinite = spoilt_rows(c["st"])
    got = lhs.lookahead(k, np.roll(c["st"], 17, 0), c["act"], states=rows, seed=lc.SEED, curriculum=lc.CURRICULUM, fill=-777.25)
    assert got["tails_ok"], "a word behind a buffer was written"
    assert (bits(got["state"]) == bits(np.roll(c["st"], 17, 0))).all(), "the instance changed"
    assert nonfinite.sum() >= 12 and (got["done"][nonfinite, 0] == 1).all(), "a non-finite row is done in its first step"
    assert (got["done"] <= 1).all()
    good = np.arange(rows.shape[0]) % 2 == 0
    same(got, full, rows=good, what="%s, the rows between the spoilt ones" % kind)
    lhs.observe(k, rows)


def test_containment_under_the_sanitizers(scene, tmp_path):
    """the same rows through the stand-alone program built with AddressSanitizer and UBSan (host code only): a child process, exit status 0"""
    kind, k, c, full = scene
    data = tmp_path / "cases.f32"
    with open(data, "wb") as f:
        f.write(np.ascontiguousarray(c["st"], np.float32).tobytes())
        f.write(np.ascontiguousarray(c["act"], np.float32).tobytes())
    run = subprocess.run([lhs.build_asan(), str(data), str(k)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-4000:]
    assert run.stdout.strip().endswith("ok")
