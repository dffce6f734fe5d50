"""The env logic of a control step behind its substeps (docs/PHYSICS.md 4.3 - 4.10; ss_kernels.hpp: step_logic on the lane pair of a robot,
step_score and ep_return_add by value), one op of tests/device/ss_probe.hip per call, against the fp64 reference of tests/np_step_logic.py.
Between the per-formula ops of tests/test_contact_ops.py and the step-level parity tests nothing else holds this layer on its own: those
compare whole steps within a tolerance sized for the dynamics and let a step near a threshold take either branch; the bit tests show that two
codings agree, not that either is right.

Flavours and judgement as in test_contact_ops.py: `host` is the probe compiled for the CPU at test time (the two lanes of a robot are two
threads that meet at every exchange), `device` the gfx950 build (@pytest.mark.gpu).  A float passes when |got - ref| <= k * 2^-24 * B, B the
reference's running bound, k the counted roundings (np_step_logic derives each), exact where B = 0.  An output that is a decision (d, bad,
advanced, n, count, elapsed, flags, the draw's record) is judged exactly wherever the reference's margin to the threshold exceeds the compared
quantity's own bound and left out otherwise; the presence of the two bonuses and the limit count are no outputs of step_logic and reach the
test through the reward, which is judged only where those decisions are the reference's.  The worst err / (2^-24 B) per output is printed
(pytest -s) and kept in docs/HISTORY.md."""
import numpy as np
import pytest

import np_contact as nc
import np_contact_ops as no
import np_env
import np_step_logic as sl
import probe_lib as pl

HAVE_HIPCC = bool(pl.hipcc())
FLAVOURS = [pytest.param("host", marks=pytest.mark.skipif(not HAVE_HIPCC, reason="needs hipcc")),
            pytest.param("device", marks=pytest.mark.gpu)]
KINDS = sl.KINDS


def _worst_per_output(got, ref, B, exact, k, names):
    """{name: worst err / (2^-24 B)} over the judged components of each named column"""
    out = {}
    for c, name in names.items():
        m = np.isfinite(B[..., c]) & (B[..., c] > 0) & ~exact[..., c]
        with np.errstate(invalid="ignore"):
            out["%s/%d" % (name, k[c])] = float((np.abs(got[..., c] - ref[..., c])[m] / (sl.U * B[..., c][m])).max()) if m.any() else 0.0
    return ", ".join("%s %.2f" % (n, w) for n, w in out.items())


# ---------------------------------------------------------------- step_score
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_step_score(flavour, kind):
    """every word of StepScore on 2048 random cases and the edges of every threshold; a single case alone gives the same words"""
    d = sl.score_prepared(kind)
    raw = pl.run(flavour, "step_score", KINDS.index(kind), d["inp"])
    with np.errstate(invalid="ignore"):
        got = raw.astype(np.float64)
    got[:, 1:3] = sl.from_bits(raw[:, 1:3])
    (worst, fails), left = sl.judge(got, d["ref"], d["B"], d["exact"], sl.SCORE_K)
    print("step-logic %s step_score %s: n=%d, %d components left out; worst err/(2^-24 B): %s" % (
        flavour, kind, got.shape[0], left, _worst_per_output(got, d["ref"], d["B"], d["exact"], sl.SCORE_K,
                                                             {0: "pot_prev", 3: "r", 4: "roll", 5: "pitch", 6: "cyaw", 7: "syaw"})))
    assert not fails, "%d failures; (case, column, got, ref, ratio): %s" % (len(fails), fails[:8])
    for name, (e, expect) in d["edges"].items():
        for key, want in expect.items():
            if key in ("d", "bad", "r"):
                assert got[e, sl.SCORE_NAMES.index(key)] == want, "%s: %s is %r, must be %r" % (name, key, got[e, sl.SCORE_NAMES.index(key)], want)
    one = pl.run(flavour, "step_score", KINDS.index(kind), d["inp"][:1])
    assert sl.same_words(one, raw[:1]).all(), "a run of one case differs from the same case among many"


# ---------------------------------------------------------------- ep_return
def _run_episodes(flavour, r):
    """rewards [n, 1000] -> pairs [n, 1000, 2] float32: rows of EP_R rewards chained through the pair, from (0, 0)"""
    n, T = r.shape
    pairs = np.zeros((n, T, 2), np.float32)
    start = np.zeros((n, 2), np.float32)
    for t0 in range(0, T, sl.EP_R):
        got = pl.run(flavour, "ep_return", 0, np.concatenate([start, r[:, t0:t0 + sl.EP_R]], 1))
        pairs[:, t0:t0 + sl.EP_R] = got.reshape(n, sl.EP_R, 2)
        start = pairs[:, t0 + sl.EP_R - 1]
    return pairs


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_ep_return(flavour):
    """After every one of 1000 rewards the pair is within its derived bound of the exact sum of the fp32 rewards, and normalised:
    hi == float32(hi + lo), |lo| <= ulp(hi) / 2.  Sequences: 2048 random ones of the env's sizes, zeros, alternating +-50, and one on which
    an fp32 running sum loses more than 1e-4 relative."""
    d = sl.ep_prepared()
    pairs = _run_episodes(flavour, d["r"])
    hi, lo = pairs[..., 0].astype(np.float64), pairs[..., 1].astype(np.float64)
    err = np.abs(hi + lo - d["T"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(d["B"] > 0, err / (sl.U * d["B"]), np.where(err == 0, 0.0, np.inf))
    print("step-logic %s ep_return: %d sequences of %d rewards: worst |hi + lo - sum| / (2^-24 B) = %.3f (k = %d); worst |hi + lo - sum| %.2e" % (
        flavour, d["r"].shape[0], d["r"].shape[1], ratio.max(), sl.K_EP, err.max()))
    bad = np.argwhere(~(ratio <= sl.K_EP))
    assert bad.size == 0, "pair beyond its bound at (sequence, step) %s: %r + %r against %r" % (bad[0], hi[tuple(bad[0])], lo[tuple(bad[0])], d["T"][tuple(bad[0])])
    assert (pairs[..., 0] == (hi + lo).astype(np.float32)).all(), "hi is not float32(hi + lo)"
    assert (np.abs(lo) <= 0.5 * np.spacing(np.abs(pairs[..., 0])).astype(np.float64)).all(), "|lo| exceeds half an ulp of hi"
    e = d["edges"]
    assert (pairs[e["zeros"]] == 0).all()
    assert (pairs[e["alternating"], :, 1] == 0).all() and (pairs[e["alternating"], 0::2, 0] == 50).all() and (pairs[e["alternating"], 1::2, 0] == 0).all()
    want = d["T"][e["lossy"], -1]
    # (the bound above is the judgement; this states the contrast: the fp32 running sum of this sequence is off by more than 1e-4 relative)
    assert want > 9e-4 and abs(hi[e["lossy"], -1] + lo[e["lossy"], -1] - want) <= 1e-4 * want, "the pair keeps what an fp32 running sum loses"
    # a single case alone
    one = pl.run(flavour, "ep_return", 0, np.concatenate([np.zeros((1, 2), np.float32), d["r"][:1, :sl.EP_R]], 1))
    assert (one.reshape(sl.EP_R, 2) == pairs[0, :sl.EP_R]).all()


def test_ep_return_reference():
    """the reference's running sums are math.fsum's, the lossy sequence loses what it is there to lose, and the sequences have the env's sizes"""
    d = sl.ep_prepared()
    assert sl.fsum_check(d["r"], d["T"]) == 0.0
    n = d["edges"]["zeros"]
    assert ((d["r"][:n] > 40).sum(1) == 1).all() and (np.abs(d["r"][:n]) <= 52.0).all()
    near = np.abs(d["r"][:n:2] + 1) <= 0.02
    assert (near.sum(1) >= 200).all(), "every other random sequence has a run of 200 rewards near -1"
    naive = np.float32(0)
    for v in d["r"][d["edges"]["lossy"]]:
        naive = np.float32(naive + v)
    assert abs(float(naive) - d["T"][d["edges"]["lossy"], -1]) > 1e-4 * abs(d["T"][d["edges"]["lossy"], -1])


# ---------------------------------------------------------------- step_logic
GOT_COLUMNS = dict(d=sl.O_D, bad=sl.O_BAD, advanced=sl.O_ADV, n=sl.O_N, count=sl.O_COUNT, elapsed=sl.O_ELAPSED, flags=sl.O_FLAGS, calls=sl.O_DRAW,
                   k=sl.O_DRAW + 1, draw_ctr=sl.O_DRAW + 2, ctr=sl.O_CTR, r=sl.O_R)
DECISIONS = ("tall", "low", "target", "pitch_out", "roll_out", "first", "at_limit")


def _check_edges(d, view, raw):
    """every stated outcome of every edge case, in both lanes"""
    inp = d["inp"]
    g = raw.reshape(-1, 2, sl.LOGIC_OWL)
    for name, (e, expect) in d["edges"].items():
        for key, want in expect.items():
            if key in GOT_COLUMNS:
                for lane in (0, 1):
                    assert view[e, lane, GOT_COLUMNS[key]] == want, "%s: lane %d: %s is %r, must be %r" % (name, lane, key, view[e, lane, GOT_COLUMNS[key]], want)
            elif key == "stores":
                assert tuple(int(view[e, lane, sl.O_STORE]) for lane in (0, 1)) == want, "%s: store is true in exactly one lane of the pair" % name
            elif key == "pair_unchanged":
                for lane in (0, 1):
                    assert (g[e, lane, sl.O_EPRET:sl.O_EPRET + 2].view(np.uint32) == inp[e, sl.I_WORDS + 2:sl.I_WORDS + 4].view(np.uint32)).all(), \
                        "%s: lane %d: the return pair changed" % (name, lane)
            elif key == "keeps_slot2":          # n = 18 -> 19: slots 0, 1 are the old 1, 2; slot 2 keeps the last stone and its heading; nn_dr stays
                old = inp[e, sl.I_CACHE:sl.I_CACHE + 24]
                for lane, mm in ((0, 1.0), (1, -1.0)):
                    c = g[e, lane, sl.O_CACHE:sl.O_CACHE + 24]
                    for off, w in ((0, 3), (9, 3), (18, 2)):
                        assert (c[off:off + w] == old[off + w:off + 2 * w]).all() and (c[off + w:off + 3 * w] == np.tile(old[off + 2 * w:off + 3 * w], 2)).all(), name
                    h = inp[e, sl.I_HEAD:sl.I_HEAD + 6]
                    assert (g[e, lane, sl.O_HD:sl.O_HD + 6] == np.concatenate([h[2:4], h[4:6], h[4:6]])).all(), name
                    assert (g[e, lane, sl.O_LDSHEAD:sl.O_LDSHEAD + 6] == np.concatenate([h[2:4], h[4:6], h[4:6]]) * np.float32([1, mm] * 3)).all(), name
                    assert g[e, lane, sl.O_NNDR] == inp[e, sl.I_WORDS + 1], name
            elif key == "drawn":                # slot 2, its heading and nn_dr are the stub's; the headings shifted; the left lane's LDS copy y-mirrored
                stub, h = inp[e, sl.I_STUB:sl.I_STUB + 11], inp[e, sl.I_HEAD:sl.I_HEAD + 6]
                for lane, mm in ((0, 1.0), (1, -1.0)):
                    c = g[e, lane, sl.O_CACHE:sl.O_CACHE + 24]
                    assert (c[6:9] == stub[0:3]).all() and (c[15:18] == stub[3:6]).all() and (c[22:24] == stub[6:8]).all(), name
                    want_h = np.concatenate([h[2:4], h[4:6], stub[8:10]])
                    assert (g[e, lane, sl.O_HD:sl.O_HD + 6] == want_h).all(), name
                    assert (g[e, lane, sl.O_LDSHEAD:sl.O_LDSHEAD + 6] == want_h * np.float32([1, mm] * 3)).all(), name
                    assert g[e, lane, sl.O_NNDR] == stub[10], name
                assert stub[9] != 0 and h[5] != 0, "the mirror shows"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_step_logic(flavour, kind):
    """all of StepEnd, the env words, the cache, the LDS headings and the draw's record, per lane, on 2048 random robots and the edges; the two
    lanes of a pair agree bit for bit in everything but the mirrored LDS headings and `store`; the return pair moves by the lane's own reward
    within ep_return_add's bound"""
    d = sl.logic_prepared(kind)
    inp = d["inp"]
    assert inp.shape[0] % 32 != 0, "the device's last wavefront is partial"
    raw = pl.run(flavour, "step_logic", KINDS.index(kind), inp)
    g = raw.reshape(-1, 2, sl.LOGIC_OWL)
    # pair invariant: env-level outputs identical in both lanes
    env_cols = [c for c in range(sl.LOGIC_OWL) if not (sl.O_LDSHEAD <= c < sl.O_LDSHEAD + 6) and c != sl.O_STORE]
    diff = np.argwhere(g[:, 0][:, env_cols].view(np.uint32) != g[:, 1][:, env_cols].view(np.uint32))
    assert diff.size == 0, "the lanes of robot %d differ in word %d: %r / %r" % (
        diff[0][0], env_cols[diff[0][1]], g[diff[0][0], 0, env_cols[diff[0][1]]], g[diff[0][0], 1, env_cols[diff[0][1]]])
    view = sl.logic_view(raw)
    ref, B, exact = d["ref"], d["B"], d["exact"]
    # the base words come back as they went in (non-finite ones included)
    assert sl.same_words(g[:, :, sl.O_BASE:sl.O_BASE + 13], inp[:, None, :13]).all(), "StepEnd's base is not the state's"
    # integer words: exactly (float32 would merge neighbouring counters)
    for c in sl.LOGIC_INT:
        m = exact[:, :, c]
        bad = np.argwhere(m & (view[:, :, c] != ref[:, :, c]))
        assert bad.size == 0, "robot %d lane %d: integer word %d is %r, must be %r" % (bad[0][0], bad[0][1], c, view[tuple(bad[0]) + (c,)], ref[tuple(bad[0]) + (c,)])
    n = inp.shape[0]
    (worst, fails), left = sl.judge(view.reshape(2 * n, -1), ref.reshape(2 * n, -1), B.reshape(2 * n, -1), exact.reshape(2 * n, -1), sl.LOGIC_K)
    print("step-logic %s step_logic %s: n=%d robots, %d components left out; worst err/(2^-24 B): %s" % (
        flavour, kind, n, left - 2 * n * 13, _worst_per_output(view, ref, B, exact, sl.LOGIC_K, sl.LOGIC_NAMES)))
    assert not fails, "%d failures; (lane row, column, got, ref, ratio): %s" % (len(fails), fails[:8])
    # the pair moved by this lane's own reward: hi' + lo' = hi + lo + r within two roundings of 2^-24 (2 |hi + lo| + |r|) (np_step_logic, ep_return_add)
    r_got = view[:, 0, sl.O_R]
    ok = np.isfinite(r_got)
    pair_in = inp[:, sl.I_WORDS + 2].astype(np.float64) + inp[:, sl.I_WORDS + 3].astype(np.float64)
    moved = np.abs(view[:, 0, sl.O_EPSUM] - (pair_in + r_got))
    assert ok.all() and (moved <= sl.K_EP * sl.U * sl.U * (2 * np.abs(pair_in) + np.abs(r_got)) * (1 + 2.0 ** -20)).all(), "the return pair lost part of the reward"
    hi, lo = g[:, 0, sl.O_EPRET], g[:, 0, sl.O_EPRET + 1]
    assert (hi == (hi.astype(np.float64) + lo.astype(np.float64)).astype(np.float32)).all() and (np.abs(lo) <= 0.5 * np.spacing(np.abs(hi))).all()
    _check_edges(d, view, raw)
    one = pl.run(flavour, "step_logic", KINDS.index(kind), inp[:1])
    assert sl.same_words(one, raw[:1]).all(), "a run of one robot differs from the same robot among many"


@pytest.mark.parametrize("kind", KINDS)
def test_step_logic_reference(kind):
    """The reference alone: it leaves at most 1 % of the random cases out of each decision and none of the edges, states every edge's outcome,
    and the random cases take every branch at least 2 % of the time."""
    for d, is_logic in ((sl.logic_prepared(kind), True), (sl.score_prepared(kind), False)):
        dec = d["dec"] if is_logic else d["s"]
        nr = d["n_random"]
        safes = dict(height=dec["tall_safe"], low=dec["low_safe"], target=dec["target_safe"], pitch=dec["pitch_safe"], roll=dec["roll_safe"], d=dec["d_safe"])
        if is_logic:
            safes["at_limit"] = dec["limit_safe"]
        for name, s in safes.items():
            assert (~s[:nr]).mean() <= 0.01, "%s: %d of %d random cases left out" % (name, (~s[:nr]).sum(), nr)
            assert s[nr:].all(), "%s: edge cases %s are left out" % (name, (nr + np.nonzero(~s[nr:])[0]).tolist())
        print("step-logic reference %s %s: random cases left out per decision: %s" % (
            "step_logic" if is_logic else "step_score", kind, ", ".join("%s %d" % (k, (~s[:nr]).sum()) for k, s in safes.items())))
        fin = dec["finite"][:nr] if is_logic else (sl.from_bits(d["inp"][:nr, 29]) != 0)
        branches = {"height <= 0.7": ~dec["tall"][:nr] & fin, "height > 0.7": dec["tall"][:nr], "below zlow + 0.3": dec["low"][:nr] & fin,
                    "target bonus": dec["target"][:nr] & fin, "pitch <= -0.2 or >= 0.4": dec["pitch_out"][:nr] & fin, "roll out of +-0.4": dec["roll_out"][:nr] & fin,
                    "time limit": dec["timeout"][:nr], "non-finite state": ~fin, "non-finite reward": dec["r_zero"][:nr] & fin, "done": dec["d"][:nr],
                    "not done": ~dec["d"][:nr]}
        if is_logic:
            pitch = dec["euler"][0][:nr, 1]
            with np.errstate(invalid="ignore"):
                branches.update({"pitch <= -0.2": fin & (pitch <= sl.T_PITCH_LO), "pitch >= 0.4": fin & (pitch >= sl.T_PITCH_HI)})
            cnt_in = sl.from_bits(d["inp"][:nr, sl.I_WORDS + 5])
            n_in = sl.from_bits(d["inp"][:nr, sl.I_WORDS + 4])
            touch = sl.from_bits(d["inp"][:nr][:, [sl.I_FOOT + 1, sl.I_FOOT + 6]])
            branches.update({"first touch": dec["first"][:nr], "advance with a draw": dec["drawn"][:nr], "advance to stone 19, no draw": dec["adv"][:nr] & ~dec["drawn"][:nr],
                             "on stone 19, count grows": dec["reached"][:nr] & (n_in == 19), "contact lost, count kept": ~dec["reached"][:nr] & (cnt_in > 0),
                             "right foot only": (touch[:, 0] == 1) & (touch[:, 1] == 0), "left foot only": (touch[:, 0] == 0) & (touch[:, 1] == 1),
                             "both feet": touch.all(1), "a joint at its limit": dec["at_limit"][:nr] > 0, "no joint at its limit": dec["at_limit"][:nr] == 0,
                             "a spine joint at its limit": _spine_limited(kind, d["inp"][:nr])})
        for name, b in branches.items():
            assert b.mean() >= 0.02, "branch '%s' is taken by %d of %d random cases" % (name, b.sum(), nr)
        for name, (e, expect) in d["edges"].items():
            for key, want in expect.items():
                if key in DECISIONS:
                    assert dec[key][e] == want, "%s: the reference's %s is %r, stated %r" % (name, key, dec[key][e], want)
                elif key == "a2":
                    assert abs(dec["a2"][e] - want) < 1e-6, name          # each actuated joint once
                elif key == "rho":      # the nearer sole's distance
                    assert abs(dec["step_bonus"][e] - 50.0 * np.exp(-want / 0.25)) < 1e-9, name
                elif is_logic and key in GOT_COLUMNS:
                    assert (d["ref"][e, :, GOT_COLUMNS[key]] == want).all() and d["exact"][e, :, GOT_COLUMNS[key]].all(), (name, key, d["ref"][e, :, GOT_COLUMNS[key]], want)
                elif not is_logic and key in ("d", "bad", "r"):
                    c = sl.SCORE_NAMES.index(key)
                    assert d["ref"][e, c] == want and d["exact"][e, c], (name, key, d["ref"][e, c], want)
        if is_logic:
            lim = [dec["at_limit"][e] for name, (e, _) in d["edges"].items() if name.startswith("joint counts: at_limit")]
            assert lim == list(range(22))


def _spine_limited(kind, inp):
    m = no.model(kind)
    lo, hi = m["range"][:3, 0], m["range"][:3, 1]
    with np.errstate(invalid="ignore"):
        return (np.abs(2 * (inp[:, sl.I_Q:sl.I_Q + 3].astype(np.float64) - 0.5 * (lo + hi)) / (hi - lo)) > 0.99).any(1)


# ---------------------------------------------------------------- the reference against np_env
@pytest.mark.parametrize("kind", KINDS)
def test_reference_is_np_env_on_steps_without_advance(kind):
    """On the cases of tests/test_oracle_env_numpy.py that do not advance, the reference's reward, done, bad, count and flags are those of
    np_env.control_step (fp64, unrounded inputs: 1e-12)."""
    import oracle_lib as ol
    from test_oracle_contact import contact_states
    m = nc.rounded_model(kind)
    rng = np.random.default_rng(23)
    states = np.array(contact_states(kind, rng)[:72], np.float64)
    states[:, ol.S_ELAPSED] = rng.integers(0, 990, states.shape[0])
    states[::9, ol.S_ELAPSED] = 999
    states[:, ol.S_COUNT] = 0
    for e in range(0, states.shape[0], 3):
        terrain = states[e, ol.S_TERRAIN].reshape(20, 6)
        k = int(states[e, ol.S_N])
        states[e, 0:3] += terrain[k][:3] - terrain[0][:3]
    acts = rng.uniform(-1.3, 1.3, (states.shape[0], 21))
    cases, wants = [], []
    for e in range(states.shape[0]):
        want = np_env.control_step(m, states[e], acts[e].astype(np.float32))
        if want["advance"]:
            continue
        st, n = want["state55"], want["n"]
        terrain = states[e, ol.S_TERRAIN].reshape(20, 6)
        idx = [max(n - 1, 0), n, min(n + 1, 19)]
        right_touch = int(want["on_target"])
        cases.append(dict(pos=st[None, 0:3], quat=st[None, 3:7], w=st[None, 7:10], v=st[None, 10:13], q=st[None, 13:34], qd=st[None, 34:55],
                          act=np.clip(acts[e].astype(np.float32).astype(np.float64), -1, 1)[None], contact=np.array([[want["flags"] & 1, want["flags"] >> 1]]),
                          touch=np.array([[right_touch, 0]]), sole=np.array([want["soles"]]), cp=terrain[idx, :3][None], cn=np.zeros((1, 3, 3)),
                          ct=np.zeros((1, 3, 2)), head=np.zeros((1, 3, 2)), pot_prev=states[e, [np_env.POT]], nn_dr=np.zeros(1), ep_ret=np.zeros(1),
                          ep_lo=np.zeros(1), n=np.array([n]), count=np.array([int(states[e, ol.S_COUNT])]), elapsed=np.array([int(states[e, ol.S_ELAPSED])]),
                          ctr=np.zeros(1, np.int64), stub=np.zeros((1, 11))))
        wants.append(want)
    c = sl._stack(cases)
    ref, B, exact, dec = sl.logic_ref(kind, sl.logic_rows(c), x64=sl.logic_rows(c, np.float64))
    assert len(wants) >= 60 and sum(w["done"] for w in wants) >= 5 and sum(w["count"] == 1 for w in wants) >= 3
    for i, want in enumerate(wants):
        assert abs(ref[i, 0, sl.O_R] - want["rew"]) <= 1e-12 * max(1.0, abs(want["rew"])), (i, ref[i, 0, sl.O_R], want["rew"])
        assert bool(ref[i, 0, sl.O_D]) == want["done"] and bool(ref[i, 0, sl.O_BAD]) == want["bad"]
        assert int(ref[i, 0, sl.O_COUNT]) == want["count"] and int(ref[i, 0, sl.O_FLAGS]) == want["flags"] and not dec["adv"][i]
