"""The closed-loop look-ahead on the CPU (docs/PHYSICS.md 14, "Branches under a policy"): look_row with the action source of
steppingstone_amd/csrc/ss_policy.hpp compiled for the host (tests/host/lookahead_policy_host.cpp), on the start states of
tests/lookahead_cases.py under the three networks of tests/policy_nets.py.
  1  closed loop equals open loop, bit for bit: obs / rew / done / final_state are lookahead_host_lib.lookahead's (and, from state rows,
     lookahead_states_host_lib.lookahead's) under the reported actions
  2  every reported action is the policy's: act - offset against an fp64 evaluation of the net on the observation before the step, within
     8 E, E the error of a plain float32 evaluation (policy_nets.judge_actions)
  3  frozen rows: behind the first done act = 0, rew = 0, done = 1, obs repeats; row 0 ends at its time limit, a NaN bias ends every branch
  4  a row's bits do not depend on m, its position, repeated ids, the outputs asked for or the horizon
  5  ss_policy_words on valid and invalid descriptions, the refusals of the C functions that can be had without a GPU
  6  the stand-alone AddressSanitizer / UBSan program on the 64 cases with the ragged net
  7  the nets of policy_nets.SHAPES (the shapes tests/test_policy_ops.py pins on their own) through the whole call: N = 70, H = 2, so that
     the second MLP phase runs over the blocks the first one left; closed loop equals open loop, every action within its own fp64
     bound (tests/np_policy.py), and for the identity / relu nets bit for bit the exact fma chain and policy_eval
The shipped actors keep most walking rows alive (39 of 40 Walker3D, 36 of 40 Mike in the host build; all 24 fall rows): LIVE_FLOOR keeps
the per-step comparisons from passing on frozen rows."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import lookahead_cases as lc
import lookahead_host_lib as lh
import lookahead_policy_host_lib as lhp
import lookahead_states_host_lib as lhs
import native_build
import np_policy as npp
import policy_nets as pn

pytestmark = pytest.mark.skipif(not native_build.hipcc(), reason="needs hipcc")
H = lc.H
LIVE_FLOOR = 30
OUTS = ("obs", "rew", "done", "final_state")
KW = dict(seed=lc.SEED, curriculum=lc.CURRICULUM)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(got, want, keys=OUTS, rows=None, what=""):
    for k in keys:
        a, b = bits(got[k]), bits(want[k])
        if rows is not None:
            a, b = a[rows], b[rows]
        bad = np.nonzero((a != b).reshape(a.shape[0], -1).any(1))[0]
        assert bad.size == 0, "%s: %s differs in rows %s" % (what, k, bad[:12].tolist())


def offsets():
    return (np.random.default_rng(3).standard_normal((lc.N_CASES, H, 21)) * 0.05).astype(np.float32)


def other(st):
    return np.roll(st, 17, 0)


@functools.lru_cache(maxsize=None)
def closed(kind, name, with_offsets, from_rows):
    """the closed loop of net `name` over H steps from the case states: from the envs of an instance that holds them, or from state rows
    on an instance that holds other states"""
    k, st = lc.KINDS.index(kind), lc.cases(kind)["st"]
    off = offsets() if with_offsets else None
    out = lhp.lookahead_policy(k, other(st) if from_rows else st, pn.net(kind, name), H, states=st if from_rows else None, offsets=off,
                               fill=-777.25, **KW)
    assert out["tails_ok"], "a word behind a buffer was written"
    assert (bits(out["state"]) == bits(other(st) if from_rows else st)).all(), "the instance changed"
    return out


def live_steps(done):
    """[m,H] bool: no done before step s"""
    d = done.astype(bool)
    return ~np.concatenate([np.zeros((d.shape[0], 1), bool), np.logical_or.accumulate(d, 1)[:, :-1]], 1)


CASES = [(kind, name, off) for kind in lc.KINDS for name in pn.NAMES for off in (False, True)]


@pytest.mark.parametrize("kind,name,with_offsets", CASES)
def test_closed_loop_equals_open_loop(kind, name, with_offsets):
    k, st = lc.KINDS.index(kind), lc.cases(kind)["st"]
    got = closed(kind, name, with_offsets, False)
    assert np.isfinite(got["act"]).all()
    want = lh.lookahead(k, st, got["act"], **KW)
    same(got, want, what="%s %s from the envs" % (kind, name))
    rows = closed(kind, name, with_offsets, True)
    same(rows, lhs.lookahead(k, other(st), rows["act"], states=st, **KW), what="%s %s from state rows" % (kind, name))
    # the two starts are the same branches: same ids, same states
    same(rows, got, keys=OUTS + ("act",), what="%s %s: state rows against envs" % (kind, name))
    if name == "shipped":
        alive = ~got["done"].astype(bool).any(1)
        print("%s: %d of 40 walk rows and %d of 24 fall rows live through %d steps" % (kind, alive[:40].sum(), alive[40:].sum(), H))
        assert alive[:40].sum() >= LIVE_FLOOR, "the closed loop lost its live rows"


@pytest.mark.parametrize("kind,name,with_offsets", CASES)
def test_every_reported_action_is_the_policys(kind, name, with_offsets):
    k, st = lc.KINDS.index(kind), lc.cases(kind)["st"]
    off = offsets() if with_offsets else None
    for from_rows, root in ((False, lhs.get_obs(k, st)), (True, lhs.observe(k, st))):
        got = closed(kind, name, with_offsets, from_rows)
        inputs = np.concatenate([root[:, None], got["obs"][:, :-1]], 1)
        live = live_steps(got["done"])
        assert live.sum() >= (LIVE_FLOOR * H if name == "shipped" else 64)
        pn.judge_actions(pn.net(kind, name), got["act"], off, inputs, live, what="%s %s%s" % (kind, name, " + offsets" if with_offsets else ""))
    # the host form of f on its own: the same chain on the same packed words
    y = lhp.policy_eval(pn.net(kind, name), root)
    assert (bits(y) == bits(closed(kind, name, False, True)["act"][:, 0])).all()


@pytest.mark.parametrize("kind", lc.KINDS)
def test_frozen_rows(kind):
    k, st = lc.KINDS.index(kind), lc.cases(kind)["st"]
    got = closed(kind, "shipped", True, False)
    done = got["done"].astype(bool)
    assert done[0].argmax() == 2 and got["final_state"][0, lc.S_ELAPSED] == 1000, "row 0 ends at its time limit in its third step"
    ended = np.nonzero(done.any(1))[0]
    assert ended.size >= 1
    for r in ended:
        f = int(done[r].argmax())
        assert done[r, f:].all() and (bits(got["rew"][r, f + 1:]) == 0).all() and (bits(got["act"][r, f + 1:]) == 0).all(), r
        assert (bits(got["obs"][r, f + 1:]) == bits(got["obs"][r, f])).all(), r
        assert (got["act"][r, :f + 1] != 0).any(1).all(), "the steps up to the first done report their actions"
    # a NaN in the last bias: every action is NaN, every branch ends in step 0
    layers = [(w, b.copy(), a) for w, b, a in pn.net(kind, "ragged")]
    layers[-1][1][4] = np.nan
    bad = lhp.lookahead_policy(k, st, layers, 6, **KW)
    assert bad["tails_ok"] and (bad["done"] == 1).all() and (bits(bad["rew"][:, 1:]) == 0).all()
    assert np.isnan(bad["act"][:, 0, 4]).all() and np.isfinite(bad["act"][:, 0, :4]).all() and (bits(bad["act"][:, 1:]) == 0).all()
    assert (bits(bad["obs"][:, 1:]) == bits(bad["obs"][:, :1])).all()
    same(bad, lhs.lookahead(k, st, bad["act"], **KW), what="%s: NaN actions, open loop" % kind)


@pytest.mark.parametrize("kind", lc.KINDS)
def test_a_rows_bits_are_its_own(kind):
    k, st = lc.KINDS.index(kind), lc.cases(kind)["st"]
    net, off = pn.net(kind, "ragged"), offsets()
    full = closed(kind, "ragged", True, False)
    keys = OUTS + ("act",)
    # fewer rows, another order, an id twice, a bad id in between
    ids = np.array([40, 3, 63, 3, 99, 0, 17], np.int32)
    good = ids < lc.N_CASES
    sub = lhp.lookahead_policy(k, st, net, H, env_ids=ids, offsets=off[np.minimum(ids, 63)], fill=-777.25, **KW)
    assert sub["tails_ok"]
    same({n: sub[n][good] for n in keys}, {n: full[n][ids[good]] for n in keys}, keys=keys, what="%s: rows by id" % kind)
    for n in keys:
        assert (sub[n][~good] == (lhp.DONE_FILL if n == "done" else np.float32(-777.25))).all(), "a bad id's row of %s was written" % n
    # ... from state rows, each row its own state under one id: the id is part of the branch, so only the rows of that id compare
    rows = lhp.lookahead_policy(k, other(st), net, H, env_ids=ids, states=st[np.minimum(ids, 63)], offsets=off[np.minimum(ids, 63)], **KW)
    same({n: rows[n][good] for n in keys}, {n: full[n][ids[good]] for n in keys}, keys=keys, what="%s: state rows by id" % kind)
    # outputs not asked for
    bare = lhp.lookahead_policy(k, st, net, H, offsets=off, want=(), **KW)
    same(bare, full, keys=("rew", "done"), what="%s: without act, obs, final_state" % kind)
    only = lhp.lookahead_policy(k, st, net, H, offsets=off, want=("act",), **KW)
    same(only, full, keys=("rew", "done", "act"), what="%s: act alone" % kind)
    # a shorter horizon is a prefix
    cut = 8
    head = lhp.lookahead_policy(k, st, net, cut, offsets=np.ascontiguousarray(off[:, :cut]), **KW)
    same(head, {n: full[n][:, :cut] for n in ("obs", "rew", "done", "act")}, keys=("obs", "rew", "done", "act"), what="%s: prefix" % kind)


@pytest.mark.parametrize("name", pn.SHAPE_NAMES)
@pytest.mark.parametrize("kind", lc.KINDS)
def test_two_steps_under_the_shape_nets(kind, name):
    k, st = lc.KINDS.index(kind), lc.tile(kind, 70)[0]
    layers = pn.net(kind, name)
    got = lhp.lookahead_policy(k, st, layers, 2, fill=-777.25, **KW)
    assert got["tails_ok"] and np.isfinite(got["act"]).all()
    same(got, lh.lookahead(k, st, got["act"], **KW), what="%s %s, H = 2" % (kind, name))
    inputs = np.concatenate([lhs.get_obs(k, st)[:, None], got["obs"][:, :-1]], 1)
    live = live_steps(got["done"])
    assert live[:, 0].all() and live[:, 1].sum() >= 35, "the second step needs live rows"
    for s in range(2):
        x, act = inputs[live[:, s], s], got["act"][live[:, s], s]
        y, err = npp.eval64(layers, x, npp.TANH_ULPS["host"])[-1]
        d = np.abs(act.astype(np.float64) - y)
        print("%s %s step %d: worst err / bound %.3f over %d rows" % (kind, name, s, (d / err).max(), x.shape[0]))
        assert (d <= err).all(), "%s %s: step %d, rows %s outside their bounds" % (kind, name, s, np.nonzero(~(d <= err).all(1))[0][:8].tolist())
        if npp.is_chain_net(layers):
            assert npp.same_bits(act, npp.chain(layers, x)[-1]).all() and npp.same_bits(act, lhp.policy_eval(layers, x)).all()


def desc(widths, acts=None):
    d = lhp.Desc()
    d.layers = len(widths) - 1
    for i, w in enumerate(widths[:9]):
        d.width[i] = w
    for i in range(min(d.layers, 8)):
        d.activation[i] = 1 if acts is None else acts[i]
    return d


def test_policy_words_and_refusals():
    from steppingstone_amd import _lib
    lib = _lib.load()
    assert {"ss_policy_words", "ss_policy_pack", "ss_lookahead_policy"} <= set(_lib.SYMBOLS)
    assert C.sizeof(_lib.PolicyDesc) == C.sizeof(lhp.Desc) == 4 * (1 + 9 + 8)
    for fn in (lambda d: int(lib.ss_policy_words(None if d is None else C.byref(d))), lhp.words):
        shipped = fn(desc([60, 256, 256, 256, 256, 256, 21]))
        assert shipped >= 60 * 256 + 4 * 256 * 256 + 256 * 21 + 5 * 256 + 21 and shipped % 4 == 0
        assert fn(desc([60, 21])) > 0 and fn(desc([60, 37, 50, 21])) > 0 and fn(desc([60] + [8] * 7 + [21])) > 0
        assert fn(desc([60, 1, 21])) > 0 and fn(desc([60, 256, 21], [0, 3])) > 0
        for bad in (None, desc([60]), desc([60] + [8] * 8 + [21]), desc([59, 21]), desc([60, 22]), desc([60, 257, 21]), desc([60, 0, 21]),
                    desc([60, -4, 21]), desc([60, 32, 21], [1, 4]), desc([60, 32, 21], [-1, 1])):
            assert fn(bad) == -1
    # the packed words of both builds of the layout agree on the count; a null handle is refused before anything else
    lib.ss_last_error.restype = C.c_char_p
    d = desc([60, 21])
    assert lib.ss_policy_pack(None, C.byref(d), None, None, None, None) == -1 and b"null handle" in lib.ss_last_error()
    assert lib.ss_lookahead_policy(None, None, 0, None, 1, C.byref(d), None, None, None, None, None, None, None, None, None) == -1
    assert b"null handle" in lib.ss_last_error()


def test_packed_form_holds_every_weight_once():
    layers = pn.net("walker3d", "ragged")
    d, blob = lhp.pack(layers)
    assert np.isfinite(blob).all(), "a packed word was not written"
    want = np.sort(np.concatenate([np.concatenate([w.reshape(-1), b]) for w, b, _ in layers]))
    nz = np.sort(blob[blob != 0])
    assert (nz == want[want != 0]).all()


@pytest.mark.parametrize("kind", lc.KINDS)
def test_under_the_sanitizers(kind, tmp_path):
    """the stand-alone program built with AddressSanitizer and UBSan (host code only): a child process, exit status 0"""
    data = tmp_path / "cases.f32"
    with open(data, "wb") as f:
        f.write(np.ascontiguousarray(lc.cases(kind)["st"], np.float32).tobytes())
    run = subprocess.run([lhp.build_asan(), str(data), str(lc.KINDS.index(kind))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         timeout=600)
    assert run.returncode == 0, run.stdout[-4000:]
    assert run.stdout.strip().endswith("ok")
