"""ss_lookahead_policy and ss_policy_pack on the GPU (docs/PHYSICS.md 14, "Branches under a policy"): both robots, the start states of
tests/lookahead_cases.py on N = 70 envs (three workgroups of 32 rows, the last with 6), H = 24, the three networks of tests/policy_nets.py.
  1  closed loop equals open loop, bit for bit: obs / rew / done / final_state are lookahead()'s / lookahead(states=)'s under the
     reported actions; the root observation is get_obs() / observe()
  2  every reported action is the policy's: act - offset against an fp64 evaluation of the net on the observation before the step, within
     8 E, E the error of a plain float32 evaluation on the same inputs (policy_nets.judge_actions)
  3  frozen rows: behind the first done act = 0, rew = 0, done = 1, obs repeats; row 0 ends at its time limit; a NaN bias ends every branch
  4  a row's bits depend on its id, state, policy and offsets alone: not on N, m, the row's position, repeated ids, the outputs asked for
     or the horizon; the env is untouched (its 186 words, its next real step); the row of a bad id and the words behind every buffer
     are never written
  5  one graph capture of pack + call, replayed after the weights changed in place, gives the uncaptured result
  6  the Python surface: pack_policy from each kind of source, the [N,B] forms, numpy mode, the single-env wrapper; the C API's refusals
  7  the nets of policy_nets.SHAPES (the shapes tests/test_policy_ops.py pins on their own) through the whole call, H = 2, so that the
     second MLP phase runs over the blocks the first one left: closed loop equals open loop, every action within its own fp64 bound
     (tests/np_policy.py), and for the identity / relu nets bit for bit the exact fma chain (which tests/test_lookahead_policy.py
     holds equal to the host build's policy_eval)"""
import ctypes as C

import numpy as np
import pytest
import torch

import lookahead_cases as lc
import np_policy as npp
import policy_nets as pn

pytestmark = pytest.mark.gpu
N, H = 70, lc.H
LIVE_FLOOR = 30
FILL = 0x5A5A5A5A
TAIL = 64
WIDTH = lambda h: {"act": h * 21, "obs": h * 60, "rew": h, "done": h, "final_state": 186, "work": 160}
OUTS = ("obs", "rew", "done", "final_state")
DEV = "cuda:0"


def _env(kind, n, numpy_mode=False):
    from steppingstone_amd.envs import SteppingStoneVecEnv
    e = SteppingStoneVecEnv(lc.ENV_IDS[kind], n, seed=lc.SEED, device=DEV, return_numpy=numpy_mode)
    e.update_curriculum(lc.CURRICULUM)
    e.set_auto_reset(False)
    e.reset()
    return e


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _assert_same(got, want, what, keys=OUTS, rows=None):
    for k in keys:
        a, b = bits(got[k]), bits(want[k])
        if rows is not None:
            a, b = a[rows], b[rows]
        if not torch.equal(a, b):
            bad = (a != b).reshape(a.shape[0], -1).any(1).nonzero().flatten().tolist()
            raise AssertionError("%s: %s differs in rows %s" % (what, k, bad[:12]))


def _states(kind, n=N):
    return torch.from_numpy(lc.tile(kind, n)[0]).to(DEV)


def _offsets(n=N, h=H):
    return torch.from_numpy((np.random.default_rng(3).standard_normal((n, h, 21)) * 0.05).astype(np.float32)).to(DEV)


def _live_steps(done):
    d = done.cpu().numpy().astype(bool)
    return ~np.concatenate([np.zeros((d.shape[0], 1), bool), np.logical_or.accumulate(d, 1)[:, :-1]], 1)


@pytest.mark.parametrize("name", pn.NAMES)
@pytest.mark.parametrize("kind", lc.KINDS)
def test_closed_loop_is_the_open_loop_under_the_policys_actions(kind, name):
    from steppingstone_amd.envs import pack_policy
    st = _states(kind)
    a, b = _env(kind, N), _env(kind, N)
    a.set_state(st)
    layers = pn.net(kind, name)
    pp = pack_policy(layers, a)
    for off in (None, _offsets()):
        tag = "%s %s%s" % (kind, name, "" if off is None else " + offsets")
        got = a.lookahead_policy(pp, H, offsets=off, final_state=True)
        assert set(got) == {"rew", "done", "ret", "obs", "act", "final_state"} and torch.isfinite(got["act"]).all()
        _assert_same(got, a.lookahead(got["act"], final_state=True), tag + ", from the envs")
        rows = b.lookahead_policy(pp, H, states=st, offsets=off, final_state=True)
        _assert_same(rows, b.lookahead(rows["act"], final_state=True, states=st), tag + ", from state rows")
        _assert_same(rows, got, tag + ", state rows against envs", keys=OUTS + ("act",))
        live = _live_steps(got["done"])
        for root, out in ((a.get_obs(), got), (b.observe(st), rows)):
            inputs = torch.cat([root[:, None], out["obs"][:, :-1]], 1).cpu().numpy()
            pn.judge_actions(layers, out["act"].cpu().numpy(), None if off is None else off.cpu().numpy(), inputs, live, what="GPU " + tag)
        if name == "shipped":
            alive = ~got["done"][:40].any(1)
            print("%s: %d of 40 walk rows live through %d steps" % (tag, int(alive.sum()), H))
            assert int(alive.sum()) >= LIVE_FLOOR, "the closed loop lost its live rows"
    a.close()
    b.close()


@pytest.mark.parametrize("name", pn.SHAPE_NAMES)
@pytest.mark.parametrize("kind", lc.KINDS)
def test_two_steps_under_the_shape_nets(kind, name):
    """For the identity / relu nets the actions are compared, bit for bit, with np_policy.chain instead of the host build's
    lhp.policy_eval, so that no host code is compiled on the GPU machine: the chain is numpy's emulation of fmaf, held to the C
    library's on 1.4 million triples, and tests/test_lookahead_policy.py and tests/test_policy_ops.py hold policy_eval / eval_row
    equal to it."""
    from steppingstone_amd.envs import pack_policy
    e = _env(kind, N)
    e.set_state(_states(kind))
    layers = pn.net(kind, name)
    got = e.lookahead_policy(pack_policy(layers, e), 2, final_state=True)
    assert torch.isfinite(got["act"]).all()
    _assert_same(got, e.lookahead(got["act"], final_state=True), "%s %s, H = 2" % (kind, name))
    inputs = torch.cat([e.get_obs()[:, None], got["obs"][:, :-1]], 1).cpu().numpy()
    acts, live = got["act"].cpu().numpy(), _live_steps(got["done"])
    assert live[:, 0].all() and live[:, 1].sum() >= 35, "the second step needs live rows"
    for s in range(2):
        x, act = inputs[live[:, s], s], acts[live[:, s], s]
        y, err = npp.eval64(layers, x, npp.TANH_ULPS["device"])[-1]
        d = np.abs(act.astype(np.float64) - y)
        print("GPU %s %s step %d: worst err / bound %.3f over %d rows" % (kind, name, s, (d / err).max(), x.shape[0]))
        assert (d <= err).all(), "%s %s: step %d, rows %s outside their bounds" % (kind, name, s, np.nonzero(~(d <= err).all(1))[0][:8].tolist())
        if npp.is_chain_net(layers):
            assert npp.same_bits(act, npp.chain(layers, x)[-1]).all(), "%s %s: step %d is not the exact chain" % (kind, name, s)
    e.close()


@pytest.mark.parametrize("kind", lc.KINDS)
def test_frozen_rows(kind):
    from steppingstone_amd.envs import pack_policy
    e = _env(kind, N)
    e.set_state(_states(kind))
    got = e.lookahead_policy(pack_policy(pn.net(kind, "shipped"), e), H, offsets=_offsets(), final_state=True)
    done = got["done"].cpu().numpy()
    g = {k: v.cpu().numpy().view(np.int32) if v.dtype == torch.float32 else v.cpu().numpy() for k, v in got.items()}
    assert done[0].argmax() == 2 and got["final_state"][0, lc.S_ELAPSED] == 1000, "row 0 ends at its time limit in its third step"
    ended = np.nonzero(done.any(1))[0]
    for r in ended:
        f = int(done[r].argmax())
        assert done[r, f:].all() and (g["rew"][r, f + 1:] == 0).all() and (g["act"][r, f + 1:] == 0).all(), r
        assert (g["obs"][r, f + 1:] == g["obs"][r, f]).all() and (g["act"][r, :f + 1] != 0).any(1).all(), r
    layers = [(w, b.copy(), a) for w, b, a in pn.net(kind, "ragged")]
    layers[-1][1][4] = np.nan
    bad = e.lookahead_policy(layers, 6, final_state=True)
    assert bad["done"].all() and (bits(bad["rew"][:, 1:]) == 0).all() and (bits(bad["act"][:, 1:]) == 0).all()
    assert torch.isnan(bad["act"][:, 0, 4]).all() and torch.isfinite(bad["act"][:, 0, :4]).all()
    assert torch.equal(bits(bad["obs"][:, 1:]), bits(bad["obs"][:, :1].expand(-1, 5, -1)))
    _assert_same(bad, e.lookahead(bad["act"], final_state=True), "%s: NaN actions, open loop" % kind)
    e.close()


def _call(e, pp, ids, h, states=None, offsets=None, which=("act", "obs", "final_state")):
    """ss_lookahead_policy on pre-filled buffers with a canary tail -> {name: bit patterns [m, width]}; the tails are checked"""
    from steppingstone_amd.envs import _ptr, _stream
    m = len(ids)
    w = WIDTH(h)
    names = ("rew", "work") + tuple(which)
    bufs = {k: torch.full((m * w[k] + TAIL,), FILL, dtype=torch.int32, device=DEV) for k in names}
    bufs["done"] = torch.full((m * h + 4 * TAIL,), FILL & 0xFF, dtype=torch.uint8, device=DEV)
    dev_ids = torch.as_tensor(ids, dtype=torch.int32).to(DEV)
    ptr = lambda k: _ptr(bufs[k]) if k in bufs else None
    opt = lambda t: None if t is None else _ptr(t)
    rc = e.backend.lib.ss_lookahead_policy(e.backend.h, _ptr(dev_ids), m, opt(states), h, C.byref(pp.desc), _ptr(pp.blob), opt(offsets),
                                           ptr("act"), ptr("obs"), ptr("rew"), ptr("done"), ptr("final_state"), ptr("work"),
                                           _stream(e.device))
    assert rc == 0
    torch.cuda.synchronize()
    out = {}
    for k, v in bufs.items():
        v = v.cpu().numpy()
        fill = FILL if k != "done" else FILL & 0xFF
        assert (v[m * w[k]:] == fill).all(), "the words behind %s were written" % k
        out[k] = v[:m * w[k]].reshape(m, w[k])
    return out


@pytest.mark.parametrize("kind", lc.KINDS)
def test_a_rows_bits_are_its_own_and_the_env_is_untouched(kind):
    """Branch (i, r): id i from the state of case (i + 11 r) % 64 with the offsets of row (i + 11 r) % 70.  The base: three passes over one
    env of 70 after set_state of pass r's states.  Every call under test -- 130 rows of shuffled, repeated ids, each with its own state row
    and offsets, one id out of range, on freshly reset instances of 1, 70 and 130 envs; the outputs singly and together; horizons 1, 7,
    24 -- must give those rows."""
    from steppingstone_amd.envs import pack_policy
    rng = np.random.default_rng(9)
    c = lc.cases(kind)
    off_all = _offsets()
    case = lambda i, r: (i + 11 * r) % lc.N_CASES
    orow = lambda i, r: (i + 11 * r) % N
    keys = ("act",) + OUTS
    a = _env(kind, N)
    pp = pack_policy(pn.net(kind, "ragged"), a)
    base = {h: {} for h in (24, 7, 1)}
    for r in range(3):
        a.set_state(torch.from_numpy(c["st"][[case(i, r) for i in range(N)]].copy()).to(DEV))
        off = off_all[[orow(i, r) for i in range(N)]].contiguous()
        for h in (24, 7, 1):
            out = _call(a, pp, list(range(N)), h, offsets=off[:, :h].contiguous())
            for i in range(N):
                base[h][(i, r)] = {k: out[k][i] for k in keys}
                if h < 24:
                    for k in ("act", "obs", "rew", "done"):
                        assert (base[h][(i, r)][k] == base[24][(i, r)][k][:WIDTH(h)[k]]).all(), "horizon %d is no prefix" % h
    a.close()
    assert any((base[24][(i, 1)]["rew"] != base[24][(i, 0)]["rew"]).any() for i in range(N))
    envs = {n2: _env(kind, n2) for n2 in (N, 1, 130)}
    packed = {n2: pack_policy(pn.net(kind, "ragged"), e) for n2, e in envs.items()}

    def check(n2, h, which):
        e, keep, m = envs[n2], min(n2, N), 130
        ids = [int(i) for i in rng.permutation(keep)] + [int(i) for i in rng.integers(0, keep, m - keep - 1)]
        seen, pairs = {}, []
        for i in ids:
            seen[i] = seen.get(i, -1) + 1
            pairs.append((i, seen[i] % 3))
        spot = int(rng.integers(0, m))
        pairs.insert(spot, (n2 + 3 if h != 7 else -1, 0))          # one id out of range
        clamp = lambda i: max(min(i, N - 1), 0)
        st = torch.from_numpy(c["st"][[case(clamp(i), r) for i, r in pairs]].copy()).to(DEV)
        off = off_all[[orow(clamp(i), r) for i, r in pairs], :h].contiguous()
        before = e.get_state().clone()
        out = _call(e, packed[n2], [i for i, _ in pairs], h, states=st, offsets=off, which=which)
        assert torch.equal(bits(e.get_state()), bits(before)), "the call changed the env"
        for j, p in enumerate(pairs):
            for k in ("rew", "done") + tuple(which):
                if j == spot:
                    fill = FILL if k != "done" else FILL & 0xFF
                    assert (out[k][j] == fill).all(), "row %d (id %d) of %s was written" % (j, p[0], k)
                else:
                    assert (out[k][j] == base[h][p][k]).all(), "%s of branch %s at row %d: %d envs, H = %d, outputs %s" % (k, p, j, n2, h, which)

    for which in (("act", "obs", "final_state"), ("act",), ("obs",), ("final_state",), ()):
        check(N, 24, which)
    for n2 in (1, 130):
        check(n2, 24, ("act", "obs", "final_state"))
        check(n2, 7, ())
    check(N, 1, ("act", "obs", "final_state"))
    check(130, 7, ("act", "final_state"))
    for e in envs.values():
        e.close()
    # the env's own state as the root: its 186 words and its next real step are as without the call
    st, act = _states(kind), torch.from_numpy(lc.tile(kind, N)[1][:, 0].copy()).to(DEV)
    outs = []
    for dry in (True, False):
        e = _env(kind, N)
        e.set_state(st)
        if dry:
            e.lookahead_policy(pack_policy(pn.net(kind, "shipped"), e), H, offsets=off_all)
            assert torch.equal(bits(e.get_state()), bits(st)), "lookahead_policy changed the state"
        obs, rew, done, _ = e.step(act)
        outs.append((obs.clone(), rew.clone(), done.clone(), e._info.clone(), e.get_state().clone()))
        e.close()
    for x, y, name in zip(outs[0], outs[1], ("obs", "rew", "done", "info", "state")):
        assert torch.equal(bits(x), bits(y)), "the next real step's %s" % name


def test_capture_pack_and_call_into_a_graph():
    """one capture of refresh() + the look-ahead; after the weights changed in place a replay gives what an uncaptured refresh + call gives"""
    from steppingstone_amd import _lib
    from steppingstone_amd.envs import pack_policy
    kind, h = "walker3d", 7
    nn = torch.nn
    torch.manual_seed(5)
    net = nn.Sequential(nn.Linear(60, 37), nn.Softsign(), nn.Linear(37, 50), nn.ReLU(), nn.Linear(50, 21), nn.Tanh()).to(DEV)
    e = _env(kind, N)
    e.set_state(_states(kind))
    pp = pack_policy(net, e)
    off = _offsets(N, h)
    act, obs = torch.zeros((N, h, 21), device=DEV), torch.zeros((N, h, 60), device=DEV)
    rew, done = torch.zeros((N, h), device=DEV), torch.zeros((N, h), dtype=torch.uint8, device=DEV)
    fs, work = torch.zeros((N, 186), device=DEV), torch.zeros((N, _lib.LOOK_WORK), device=DEV)

    def run():
        pp.refresh()
        e.backend.lookahead_policy(None, N, None, h, pp.desc, pp.blob, off, act, obs, rew, done, fs, work)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first = act.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(0.7).add_(0.01)
    g.replay()
    torch.cuda.synchronize()
    pp.refresh()
    want = e.lookahead_policy(pp, h, offsets=off, final_state=True)
    _assert_same(dict(act=act, obs=obs, rew=rew, done=done.bool(), final_state=fs), want, "replayed graph", keys=OUTS + ("act",))
    assert not torch.equal(bits(first), bits(act))
    e.close()


def test_python_surface():
    from steppingstone_amd import ppo
    from steppingstone_amd.envs import PackedPolicy, SteppingStoneEnv, pack_policy
    kind, h, nn = "walker3d", 5, torch.nn
    e = _env(kind, N)
    e.set_state(_states(kind))
    torch.manual_seed(2)
    ac = ppo.ActorCritic().to(DEV)
    s = ac.actor
    seq = nn.Sequential(s.fc1, nn.Softsign(), s.fc2, nn.Softsign(), s.fc3, nn.Softsign(), s.fc4, nn.ReLU(), s.fc5, nn.ReLU(), s.out, nn.Tanh())
    triples = [(getattr(s, n).weight.detach().cpu().numpy(), getattr(s, n).bias.detach().cpu().numpy(), a)
               for n, a in zip(("fc1", "fc2", "fc3", "fc4", "fc5", "out"), ("softsign",) * 3 + ("relu",) * 2 + ("tanh",))]
    outs = [e.lookahead_policy(pack_policy(src, dev), h) for src, dev in ((ac, e), (s, DEV), (seq, e.device), (triples, e))]
    outs.append(e.lookahead_policy(s, h))                                    # packed on the call
    for o in outs[1:]:
        _assert_same(o, outs[0], "pack_policy from another kind of source", keys=("act", "obs", "rew", "done"))
    with torch.no_grad():
        want = s(e.get_obs())
    assert (outs[0]["act"][:, 0] - want).abs().max() < 1e-5
    for bad in (nn.Linear(60, 21), nn.Sequential(nn.Linear(60, 21), nn.Sigmoid()), [(np.zeros((21, 60), np.float32), np.zeros(21, np.float32), "gelu")],
                [(np.zeros((21, 59), np.float32), np.zeros(21, np.float32), "tanh")], "actor"):
        with pytest.raises(ValueError, match="supported"):
            pack_policy(bad, DEV)
    # B branches per env through offsets [N,B,H,21] and states [N,B,186]
    pp = pack_policy(s, e)
    assert isinstance(pp, PackedPolicy)
    off = _offsets(2 * N, h).reshape(N, 2, h, 21)
    st2 = torch.stack([_states(kind), _states(kind).roll(1, 0)], 1).contiguous()
    nb = e.lookahead_policy(pp, h, offsets=off, states=st2, final_state=True)
    assert nb["act"].shape == (N, 2, h, 21) and nb["obs"].shape == (N, 2, h, 60) and nb["final_state"].shape == (N, 2, 186) and nb["ret"].shape == (N, 2)
    flat = e.lookahead_policy(pp, h, env_ids=np.repeat(np.arange(N), 2), offsets=off.reshape(2 * N, h, 21), states=st2.reshape(2 * N, 186),
                              final_state=True)
    _assert_same({k: v.reshape((2 * N,) + tuple(v.shape[2:])) for k, v in nb.items()}, flat, "[N,B] against rows", keys=OUTS + ("act",))
    _assert_same({k: v[:, 0] for k, v in e.lookahead_policy(pp, h, offsets=off[:, :1].contiguous()).items()},
                 e.lookahead_policy(pp, h, offsets=off[:, 0].contiguous()), "[N,1] against [N]", keys=("act", "obs", "rew", "done"))
    for bad in (dict(horizon=0), dict(horizon=h, offsets=off[:, :, :4]), dict(horizon=h, offsets=off.double()), dict(horizon=h, env_ids=[0, N]),
                dict(horizon=h, states=st2[:3]), dict(horizon=h, env_ids=[1, 2], offsets=off)):
        with pytest.raises(ValueError):
            e.lookahead_policy(pp, **bad)
    assert e.lookahead_policy(pp, h, env_ids=[], actions=False, obs=False)["rew"].shape == (0, h)
    # numpy mode, the single-env wrapper
    en = _env(kind, N, numpy_mode=True)
    en.set_state(_states(kind).cpu().numpy())
    got = en.lookahead_policy(pack_policy(s, en), h, offsets=off[:, 0].cpu().numpy())
    assert all(isinstance(v, np.ndarray) for v in got.values()) and got["done"].dtype == np.bool_
    ref = e.lookahead_policy(pp, h, offsets=off[:, 0].contiguous())
    assert (got["act"].view(np.int32) == ref["act"].cpu().numpy().view(np.int32)).all()
    en.close()
    one = SteppingStoneEnv(lc.ENV_IDS[kind])
    one.reset()
    o1 = one.lookahead_policy(s, h, branches=3)
    assert o1["act"].shape == (3, h, 21) and (np.asarray(o1["act"][0]) == np.asarray(o1["act"][2])).all()
    assert one.lookahead_policy(s, h, offsets=np.zeros((h, 21), np.float32))["rew"].shape == (1, h)
    one.close()
    e.close()


def test_bad_arguments_are_refused_and_launch_nothing():
    from steppingstone_amd.envs import _ptr, _stream, pack_policy
    from steppingstone_amd import _lib
    kind, h = "walker3d", 3
    e = _env(kind, N)
    st = _states(kind)
    pp = pack_policy(pn.net(kind, "ragged"), e)
    torch.cuda.synchronize()
    lib, hd, s = e.backend.lib, e.backend.h, _stream(e.device)
    new = lambda words, dt=torch.int32: torch.full((words,), FILL if dt == torch.int32 else FILL & 0xFF, dtype=dt, device=DEV)
    act, obs, rew, done = new(N * h * 21 + 4), new(N * h * 60 + 4), new(N * h + 4), new(N * h, torch.uint8)
    fs, work, offs = new(N * 186 + 4), new(N * 160 + 4), torch.zeros(N * h * 21 + 4, device=DEV)
    ids = torch.arange(4, dtype=torch.int32, device=DEV)
    P = _ptr
    shift = lambda t, by=4: C.c_void_p(t.data_ptr() + by)
    d, blob = C.byref(pp.desc), P(pp.blob)
    bad_desc = _lib.PolicyDesc()
    bad_desc.layers, bad_desc.width[0], bad_desc.width[1] = 1, 60, 22
    call = lambda ids_, m, st_, hh, d_, b_, of, a, o, r, dn, f, w: lib.ss_lookahead_policy(hd, ids_, m, st_, hh, d_, b_, of, a, o, r, dn, f, w, s)
    ok = [P(ids), 4, P(st), h, d, blob, P(offs), P(act), P(obs), P(rew), P(done), P(fs), P(work)]

    def with_(**kw):
        names = ("ids", "m", "st", "h", "d", "blob", "off", "act", "obs", "rew", "done", "fs", "work")
        return [kw.get(n, v) for n, v in zip(names, ok)]
    assert lib.ss_lookahead_policy(None, *ok, s) == -1
    for kw in (dict(h=0), dict(h=1001), dict(m=-1), dict(d=None), dict(d=C.byref(bad_desc)), dict(blob=None), dict(rew=None), dict(done=None),
               dict(work=None), dict(ids=None), dict(ids=None, m=N + 1), dict(blob=shift(pp.blob)), dict(obs=shift(obs)), dict(rew=shift(rew)),
               dict(fs=shift(fs)), dict(work=shift(work)), dict(st=shift(st, 2)), dict(off=shift(offs, 2)), dict(act=shift(act, 2))):
        assert call(*with_(**kw)) == -1, kw
        assert b"ss_lookahead_policy" in lib.ss_last_error()
    assert call(*with_(m=0)) == 0 and call(None, 0, None, h, d, None, None, None, None, None, None, None, None) == 0
    # ss_policy_pack
    ws = [torch.zeros(n * k, device=DEV) for n, k in ((37, 60), (50, 37), (21, 50))]
    bs = [torch.zeros(n, device=DEV) for n in (37, 50, 21)]
    wp, bp = (C.c_void_p * 3)(*[P(w) for w in ws]), (C.c_void_p * 3)(*[P(b) for b in bs])
    target = new(pp.blob.numel())
    pack = lambda d_, w_, b_, t_: lib.ss_policy_pack(hd, d_, w_, b_, t_, s)
    assert lib.ss_policy_pack(None, d, wp, bp, P(target), s) == -1
    wnull = (C.c_void_p * 3)(P(ws[0]), None, P(ws[2]))
    for args in ((None, wp, bp, P(target)), (C.byref(bad_desc), wp, bp, P(target)), (d, None, bp, P(target)), (d, wp, None, P(target)),
                 (d, wp, bp, None), (d, wp, bp, shift(target)), (d, wnull, bp, P(target))):
        assert pack(*args) == -1
        assert b"ss_policy_pack" in lib.ss_last_error()
    torch.cuda.synchronize()
    for t in (act, obs, rew, fs, work, target):
        assert (t.cpu().numpy() == FILL).all()                    # nothing was launched
    assert (done.cpu().numpy() == FILL & 0xFF).all()
    # float alignment is enough for states, offsets and act; obs, act, final_state and offsets may be NULL
    held = torch.cat([torch.full((1, 186), float("nan"), device=DEV), st]).contiguous()
    assert call(None, N, C.c_void_p(held.data_ptr() + 744), h, d, blob, shift(offs), shift(act), None, P(rew), P(done), None, P(work)) == 0
    torch.cuda.synchronize()
    want = e.lookahead_policy(pp, h, states=st, offsets=offs[1:1 + N * h * 21].reshape(N, h, 21).contiguous())
    assert torch.equal(act[1:1 + N * h * 21].reshape(N, h, 21), bits(want["act"]))
    assert torch.equal(rew[:N * h].reshape(N, h), bits(want["rew"])) and (obs.cpu().numpy() == FILL).all()
    e.close()
