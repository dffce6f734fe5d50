"""The contact stage of ss_dynamics.hpp (fk_detect, jacobian_rows / row_moment, operator_T / operator_up / operator_pair_b) and the env
formulas of ss_kernels.hpp (sampler, observation terms, reset noise), one op per call, against the fp64 references of
tests/np_contact_ops.py.  Between tests/test_spatial_ops.py (one operator of the spatial algebra per call) and the step-level parity
tests nothing else holds these on their own; they carry the integer decisions a step tolerance only sees when a sample sits on them.

Flavours and judgement as in test_spatial_ops.py: `host` is tests/device/ss_probe.hip compiled for the CPU at test time, `device` the
gfx950 build (@pytest.mark.gpu); a component passes when |got - ref| <= k * 2^-24 * B, B the reference's running error bound, k the counted
roundings (np_contact_ops states and derives each), exact where B = 0.  The worst err / (2^-24 B) per op and k is printed (pytest -s) and
kept in docs/HISTORY.md.  Integer outputs of the detection are judged exactly wherever the reference's own margins decide them."""
import numpy as np
import pytest

import np_contact as nc
import np_contact_ops as no
import np_dynamics as nd
import np_spatial as ns
import probe_lib as pl
from steppingstone_amd import model as M

HAVE_HIPCC = bool(pl.hipcc())
FLAVOURS = [pytest.param("host", marks=pytest.mark.skipif(not HAVE_HIPCC, reason="needs hipcc")),
            pytest.param("device", marks=pytest.mark.gpu)]
KINDS = no.KINDS


def _report(op, flavour, kind, n, worst, k):
    print("contact-op %s %s %s: n=%d worst err/(2^-24 B) per k = %s (k: %s)" % (flavour, op, kind, n, no.show(worst), k))


# ---------------------------------------------------------------- detection
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_fk_detect(flavour, kind):
    """Rf, pen and the sole within their counted bounds; active / slot / contact / on_target exactly wherever every predicate's fp64
    margin exceeds its own tolerance; the two codings of the touch predicate bit-equal; every edge case's stated integers."""
    d = no.detect_prepared(kind)
    got = pl.run(flavour, "fk_detect", KINDS.index(kind), d["inp"])
    assert (got[:, :20].view(np.uint32) == got[:, 20:].view(np.uint32)).all(), "the two codings of fk_detect differ"
    worst, fails = no.detect_judge(got[:, :20], d)
    _report("fk_detect", flavour, kind, got.shape[0], worst, "Rf %d, pen %d, sole %d" % (no.K_RF, no.K_D, no.K_SOLE))
    assert not fails, "%d failures; (case, column, got, ref, ratio): %s" % (len(fails), fails[:8])
    for name, e, expect in d["edges"]:
        for key, want in expect.items():
            have = no.edge_value(got[e], key)
            assert have == want, "%s: %s is %d, must be %d (row %s)" % (name, key, have, want, got[e, :20].tolist())


@pytest.mark.parametrize("kind", KINDS)
def test_fk_detect_reference(kind):
    """The reference alone: it leaves at most 1 % of the random corners out of the integer judgement, decides every integer an edge case
    states, meets every slot and the empty outcome, and agrees with np_contact.detect on poses given as angles."""
    d = no.detect_prepared(kind)
    nr = d["n_random"]
    left_out = (~d["safe"][:nr]).mean()
    print("contact-op reference fk_detect %s: %d of %d random corners left out of the integer judgement (%.3f %%); slots %s" % (
        kind, (~d["safe"][:nr]).sum(), 4 * nr, 100 * left_out, np.bincount(d["slot"][:nr].ravel() + 1, minlength=4).tolist()))
    assert left_out <= 0.01
    assert (np.bincount(d["slot"][:nr].ravel() + 1, minlength=4) > 4 * nr // 50).all(), "no contact and each slot: at least 2 % of the corners each"
    for name, e, expect in d["edges"]:
        for key, want in expect.items():
            if isinstance(key, tuple):
                assert d["safe"][e, key[1]], "%s: the reference does not decide corner %d" % (name, key[1])
            else:
                assert d["safe"][e].all(), "%s: the reference does not decide all four corners" % name
            assert no.edge_value(d["ref"][e], key) == want, (name, key, want, d["ref"][e].tolist())
    # np_contact.detect from angles, quaternion and terrain rows (its own FK, its own normals)
    rng, m = np.random.default_rng(5), no.model(kind)
    lo, hi = m["range"][:, 0], m["range"][:, 1]
    checked = 0
    for _ in range(48):
        q = rng.uniform(lo, hi)
        quat = rng.normal(size=4) * np.array([1.0, 0.1, 0.1, 0.3]) + np.array([2.0, 0, 0, 0])
        quat /= np.linalg.norm(quat)
        pos = rng.uniform(-2, 2, 3)
        R, p = M.fk(m, q, pos, nd.quat_rot(quat))
        sole = p[M.RIGHT_FOOT_BODY] + R[M.RIGHT_FOOT_BODY] @ m["corners"].mean(0)
        terrain = np.zeros((20, 6))
        terrain[:, :3] = no.FAR
        for si in (4, 5, 6):
            terrain[si] = np.concatenate([sole + rng.uniform([-0.4, -0.4, -0.01], [0.4, 0.4, 0.09]), [rng.uniform(-3, 3)], rng.uniform(-no.TILT, no.TILT, 2)])
        want = nc.detect(m, pos, quat, q, terrain, 5)[:4]
        row = np.concatenate([np.cos(q[:8]), np.sin(q[:8]), nd.quat_rot(quat).reshape(9), pos] +
                             [np.concatenate([terrain[si, :3], nc.stone_normal(terrain[si]), [np.cos(terrain[si, 3]), np.sin(terrain[si, 3])]]) for si in (4, 5, 6)])
        r = no.detect_ref(kind, row[None])          # fp64 rows: the same numbers np_contact.detect works with
        for k in range(4):
            if not r["safe"][0, k]:
                continue
            checked += 1
            assert (want[k] is None) == (r["slot"][0, k] < 0)
            if want[k] is not None:
                assert want[k]["stone"] == 4 + r["slot"][0, k]
                assert abs(want[k]["pen"] - r["ref"][0, 9 + k]) < 1e-12
                assert np.abs(want[k]["Rf"].reshape(9) - r["ref"][0, :9]).max() < 1e-12
    assert checked > 150


# ---------------------------------------------------------------- rows
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_jacobian_rows(flavour, kind):
    """rWp (row_moment included) and rB; inactive corners give the finite +z rows and rB = 0; pen at, below, above kSlop and at the clamp"""
    d = no.rows_prepared(kind)
    got = pl.run(flavour, "jacobian_rows", KINDS.index(kind), d["inp"])
    worst, fails = no.judge_cols(got, d["ref"], d["B"], np.zeros(got.shape, bool), no.ROWS_K)
    _report("jacobian_rows", flavour, kind, got.shape[0], worst, "3 .. 20 per column")
    assert not fails, "%d failures; (case, column, got, ref, ratio): %s" % (len(fails), fails[:8])
    e = d["edges"]["inactive"]
    assert np.isfinite(got[e]).all() and (got[e, 72:] == 0).all()
    for k in range(4):
        rows = got[e, 18 * k:18 * k + 18].reshape(3, 6)
        for dn, axis in enumerate((2, 0, 1)):          # n = +z, t1 = +x, t2 = +y, seen from the foot
            assert (rows[dn, 3:] == d["inp"][e, 3 * axis:3 * axis + 3]).all(), "inactive corner %d: direction %d is not the foot's view of a world axis" % (k, dn)
    e = d["edges"]["pen"]
    assert got[e, 72] == 0 and got[e, 73] == 0 and got[e, 75] == no.VMAX
    assert 0 < got[e, 74] < no.VMAX                                       # pen = 2 kSlop (the value is judged above)


@pytest.mark.parametrize("kind", KINDS)
def test_jacobian_rows_reference_is_np_contact(kind):
    d = no.rows_prepared(kind)
    rows, bn = no.rows_vs_np_contact(kind, d["inp"], d["ref"])
    assert rows < 1e-12 and bn <= 3          # kErp, kSlop, 1 / kH as fp32 constants: one rounding each


# ---------------------------------------------------------------- operators
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_contact_operators(flavour, kind):
    """T, C and Lambda_own from fp32 records of fp64 articulated-body passes, stage by stage: each stage's reference starts from the kernel's
    own output of the stage before (p, x, G are handed out by the probe), the base solve by its residual as chol_judge does.  Device: lanes 2i / 2i + 1 are the right and the (mirrored) left
    half of one robot in an asymmetric pose and C takes the partner's G; host: the lane is its own partner."""
    d = no.ops_prepared(kind)
    inp = d["inp"]
    assert (inp[0::2] != inp[1::2]).any(1).mean() > 0.99, "the lane pairs hold two different lanes (all but the symmetric poses)"
    idx = np.arange(inp.shape[0])
    got = pl.run(flavour, "contact_ops", KINDS.index(kind), inp)
    worst, fails = no.ops_judge(kind, inp, got, idx if flavour == "host" else idx ^ 1)
    print("contact-op %s contact_ops %s: n=%d worst err/(2^-24 B): T %.2f/%d, p %.2f/%d, solve residual %.2f/%d, G %.2f/%d, Lambda %.2f/%d, C %.2f/%d" % (
        flavour, kind, got.shape[0], worst["T"], no.K_T, worst["p"], no.K_P, worst["solve"], ns.CHOL_K_SOLVE, worst["G"], no.K_G,
        worst["Lambda"], no.K_LAM, worst["C"], no.K_C))
    assert not fails, "%d failures; (case, column, got, ref, ratio): %s" % (len(fails), fails[:8])
    if flavour == "device":          # the partner matters: judged with the lane's own G, C is outside its bound for nearly every pair
        _, own = no.ops_judge(kind, inp, got, idx)
        assert len(set(e for e, c, *_ in own if isinstance(c, int) and 36 <= c < 72)) > 0.9 * inp.shape[0]


@pytest.mark.parametrize("kind", KINDS)
def test_operator_reference_is_j_hinv_jt(kind):
    """fp64 only: on unrounded records the reference recursion gives the blocks of np_contact.substep's Li = J H^-1 J^T (Lambda_own, and C
    mirrored into the lane's world) and T is the dense product of the leg's joint transforms with the joint freedoms projected out"""
    d = no.ops_prepared(kind)
    picks = [0, 1, 2, 3] + sorted(set(v for v in d["edges"].values())) + [d["edges"]["range ends"] + i for i in (1, 6, 11, 15)]
    for i in picks:
        eT, eL, eC = no.ops_anchor(kind, d["poses"][i])
        assert max(eT, eL, eC) < 1e-9, (i, eT, eL, eC)


# ---------------------------------------------------------------- sampler
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_sampler(flavour):
    """sample_cell on a shared and on a per-env grid: exactly the sequential fp32 cumulative sum with the kernel's pick rule, and the picked
    cell has p > 0; yaw_sample / pitch_sample, place_stone, stone_normal within their counts"""
    d = no.sampler_prepared()
    inp = d["inp"]
    assert (inp[:-1:2, :121] != inp[1::2, :121]).any(1).mean() > 0.95, "neighbouring lanes hold different grids"
    got = pl.run(flavour, "sampler", 0, inp)
    for c, name in ((0, "shared"), (1, "per-env")):
        bad = np.nonzero(got[:, c] != d["cell"])[0]
        assert bad.size == 0, "%s grid: case %d picked %s, the fp32 cumulative sum picks %d (u = %r)" % (name, bad[0], got[bad[0], c], d["cell"][bad[0]], inp[bad[0], 121])
        assert (inp[np.arange(inp.shape[0]), got[:, c].astype(int)] > 0).all(), "a cell with p = 0 was picked"
    worst, fails = no.judge_cols(got, d["ref"], d["B"], d["exact"], no.SAMPLER_K)
    _report("sampler", flavour, "-", got.shape[0], worst, "angles %d, place_stone %d, stone_normal %d" % (no.K_ANGLE_SAMPLE, no.K_PLACE, no.K_NORMAL))
    assert not fails, "%d failures; (case, column, got, ref, ratio): %s" % (len(fails), fails[:8])
    ed = d["edges"]
    for cell in (0, 60, 120):
        assert (got[ed["one-hot %d" % cell], :2] == cell).all()
    for e in ed["fp32 sum below 1"]:
        last = int(np.nonzero(inp[e, :121] > 0)[0][-1])
        assert (got[e, :2] == last).all() and last < 120
    assert (got[ed["u = 0"], :2] == 0).all()
    assert got[ed["leading and trailing zeros"][0], 0] == 7 and (got[ed["leading and trailing zeros"], :2] <= 99).all()


@pytest.mark.skipif(not HAVE_HIPCC, reason="needs hipcc")
def test_window_prob():
    """host code of the product: levels 0..5, window and ring; each entry within one rounding of the fp64 construction, zeros exact, the
    sum within 121 roundings of 1"""
    cases = np.array([[lv, ring] for lv in range(6) for ring in (0, 1)], np.float32)
    got = pl.run("host", "window_prob", 0, cases)
    for (lv, ring), g in zip(cases, got):
        want = no.window_prob_np(int(lv), bool(ring))
        assert ((g == 0) == (want == 0)).all()
        assert (np.abs(g.astype(np.float64) - want) <= ns.U * want).all()
        assert abs(g.astype(np.float64).sum() - 1.0) <= 121 * ns.U
    assert got[0].argmax() == 60 and got[0, 60] == 1.0 and got[1, 60] == 1.0


@pytest.mark.gpu
def test_window_prob_is_host_code():
    assert pl.run("device", "window_prob", 0, np.zeros((1, 2), np.float32)) is None


# ---------------------------------------------------------------- observation terms
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_obs_terms(flavour, kind):
    """quat_roll_pitch_cs, target_features, planar_dist, clip5, obs_angle / obs_rate of every joint, reset_angle of every joint of the robot
    and of the probe's ClampModel (whose draws reach the clamps: the shipped robots' cannot)"""
    d = no.obs_prepared(kind)
    got = pl.run(flavour, "obs_terms", KINDS.index(kind), d["inp"])
    worst, fails = no.judge_cols(got, d["ref"], d["B"], d["exact"], no.OBS_K)
    _report("obs_terms", flavour, kind, got.shape[0], worst, "roll %d, pitch %d, yaw %d, planar_dist %d, obs_angle %d, reset_angle %d" % (
        no.K_ROLL, no.K_PITCH, no.K_YAW, no.K_PD, no.K_OA, no.K_RA))
    assert not fails, "%d failures; (case, column, got, ref, ratio): %s" % (len(fails), fails[:8])
    ed = d["edges"]
    for e, sign in zip(ed["pitch clamp"], (1.0, -1.0)):          # 2 (w y - z x) = +-1.002: finite only through the clamp (the value is judged above)
        assert np.isfinite(got[e, 1]) and np.sign(got[e, 1]) == sign
    cm = d["clamped_cm"]
    assert cm[:, 0::2].mean() > 0.2 and cm[:, 1::2].mean() > 0.2, "the ClampModel's draws reach lo + 0.02 (even joints) and hi - 0.02 (odd joints)"
    assert got[ed["A = B = 0"], 2] == 1.0 and got[ed["A = B = 0"], 3] == 0.0
    e = ed["clip"]
    assert got[e, 10] == 5.0 and (got[e, 11:32] == 5.0 * np.array(M.POLICY_SIGN)).all()
    assert (np.abs(got[e, 32:53]) == 5.0).all()
    nr = no.N_RANDOM
    assert (np.abs(got[:nr, 11:32]) == 5.0).mean() > 0.05 and (np.abs(got[:nr, 11:32]) < 5.0).mean() > 0.5


@pytest.mark.parametrize("kind", KINDS)
def test_reset_angle_clamp_reach(kind):
    """What the shipped models allow: the reset draw is q0 +- 0.05 and the clamp sits 0.02 inside the range, so a draw reaches a clamp only
    where q0 is within 0.07 of a limit.  The extreme draws (u = 0, u = 1 - 2^-24) of every joint are in the cases either way; this records
    which joints, if any, they clamp."""
    d = no.obs_prepared(kind)
    lo_e, hi_e = d["edges"]["reset extremes"]
    hit = sorted(set(np.nonzero(d["clamped"][[lo_e, hi_e]].any(0))[0].tolist()))
    m = no.model(kind)
    near = [j for j in range(21) if m["q0"][j] - 0.05 < m["range"][j, 0] + 0.02 or m["q0"][j] + 0.05 > m["range"][j, 1] - 0.02]
    print("contact-op reference reset_angle %s: joints whose extreme draws clamp: %s" % (kind, hit))
    assert hit == near
