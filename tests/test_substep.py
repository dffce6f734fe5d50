"""One whole substep of the step kernels (ss_dynamics.hpp: substep<Model, 0>, the ~700 lines between the operators that
tests/test_spatial_ops.py / tests/test_contact_ops.py hold one at a time and the whole control step of the parity rule), stage by stage
against fp64: free dynamics (A), detection (B), impulses (C), response of the tree (D), integration (E), exact invariants (F).  Each stage is
judged from the KERNEL's own output of the stage before, |got - ref| <= K 2^-24 B with B the reference's running absolute-value bound;
tests/substep_cases.py holds the cases, the reference (np_contact, np_dynamics on model.build rounded to fp32), the formulas and the K.

Flavours as in test_contact_ops.py: `host` is tests/device/ss_probe.hip compiled for the CPU (the two lanes of a robot run as two threads
that meet at every lane exchange), `device` the gfx950 build with the product's flags (@pytest.mark.gpu).  The probe's launches of a
flavour and robot are made once and shared by the stages.  Worst ratios are printed (pytest -s) and kept in docs/HISTORY.md."""
import functools

import numpy as np
import pytest

import probe_lib as pl
import substep_cases as sc

HAVE_HIPCC = bool(pl.hipcc())
FLAVOURS = [pytest.param("host", marks=pytest.mark.skipif(not HAVE_HIPCC, reason="needs hipcc")),
            pytest.param("device", marks=pytest.mark.gpu)]
KINDS = sc.KINDS
U = sc.U
N_FEEDBACK = 40
LEFT_OUT_CAP = 0.02


def _cls(P, e):
    return "/".join(sorted(P["cls"][e])) if e < len(P["cls"]) else "derived"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def runs(flavour, kind):
    """every launch the stages need, once: the cases, the same with the stones 10 m down, mirrored, the second substep (the first call's
    output fed back), the same as two calls in one launch, and second substeps whose contact set differs from their warm key"""
    P = sc.prepared(kind)
    k = KINDS.index(kind)
    inp = P["inp"]
    go = lambda rows: pl.run(flavour, "substep", k, rows)
    R = dict(main=go(inp), down=go(sc.moved_down(inp)), mirror=go(sc.mirror_rows(inp)))
    fb = [e for e in range(inp.shape[0]) if P["contact"][e] and P["refs"][e]["safe"]][:N_FEEDBACK]
    R["fb"] = np.array(fb)
    R["second_in"] = sc.feedback_rows(inp[fb], R["main"][fb])
    R["second"] = go(R["second_in"])
    two = np.array(inp[fb])
    two[:, sc.I_CALLS] = 2
    R["two"] = go(two)
    R["changed_in"] = sc.warm_changed_rows(kind, R["second_in"])
    R["changed"] = go(R["changed_in"]) if R["changed_in"].shape[0] else np.zeros((0, 2 * sc.OWL), np.float32)
    R["second_refs"], _ = sc.references(kind, R["second_in"])
    R["changed_refs"], _ = sc.references(kind, R["changed_in"]) if R["changed_in"].shape[0] else ([], None)
    return R


def _sets(flavour, kind):
    """(name, rows, refs, output, class of case e) of the launches whose contact stage is judged"""
    P, R = sc.prepared(kind), runs(flavour, kind)
    return [("cases", P["inp"], P["refs"], R["main"], lambda e: _cls(P, e)),
            ("second substep", R["second_in"], R["second_refs"], R["second"], lambda e: "warm second substep of " + _cls(P, int(R["fb"][e]))),
            ("changed contact set", R["changed_in"], R["changed_refs"], R["changed"], lambda e: "warm start, contact set changed")]


def _kernel_active(a, e):
    return ((a["key"][e][:, None] >> np.arange(4)) & 1).astype(bool)


def _agrees(a, e, r):
    """the kernel's contact set is the reference's (stage B asserts that wherever the reference decides it)"""
    return np.array_equal(_kernel_active(a, e), r["active"])


# ---------------------------------------------------------------- the reference alone
@pytest.mark.parametrize("kind", KINDS)
def test_case_coverage(kind):
    """CPU, reference only: at most MAX_CASES cases, every class the issue names at least 8 times, and at most 2 % of the contact cases
    left out of stages C and D because the reference's own margins do not decide their contact set"""
    P = sc.prepared(kind)
    refs, inp = P["refs"], P["inp"].astype(np.float64)
    n = len(refs)
    assert n <= sc.MAX_CASES
    feet = np.array([r["active"].any(1) for r in refs])
    corners = np.array([r["active"].sum(1) for r in refs])
    slots = [set(c["stone"] for c in r["contacts"] if c is not None) for r in refs]
    st = inp[:, sc.I_STONES:sc.I_STONES + 24].reshape(n, 3, 8)
    tilted = [any(c is not None and abs(st[e, c["stone"], 5]) < 0.9999 and abs(st[e, c["stone"], 7]) > 0.03 for c in r["contacts"]) for e, r in enumerate(refs)]
    viol = np.array([r["viol"] for r in refs])
    act, power = inp[:, sc.I_ACT:sc.I_ACT + 21], inp[:, sc.I_POWER]
    extreme = np.array([set(np.unique(a)) == {-1.0, 0.0, 1.0} for a in act])
    qdm = np.abs(inp[:, sc.I_QD:sc.I_QD + 21]).max(1)
    contact = [e for e in range(n) if P["contact"][e]]
    fb = sc.reference_feedback(kind, P["inp"][contact], [refs[e] for e in contact])
    fb_refs, _ = sc.references(kind, fb[:N_FEEDBACK])
    changed = sc.warm_changed_rows(kind, fb[:N_FEEDBACK])
    count = {
        "free flight": int((~feet.any(1)).sum()),
        "one foot down": int((feet.sum(1) == 1).sum()),
        "both feet down": int(feet.all(1).sum()),
        "1 or 2 corners of a foot": int(((corners == 1) | (corners == 2)).any(1).sum()),
        "carried by slot 0": sum(0 in s for s in slots),
        "carried by slot 2": sum(2 in s for s in slots),
        "tilted and turned stone": int(np.sum(tilted)),
        "sliding": sum(bool(r.get("sliding")) for r in refs),
        "sticking": sum(r["active"].any() and not r["sliding"] for r in refs),
        "warm second substep": sum(bool(r["active"].any() and r["warm_kept"].any()) for r in fb_refs),
        "warm start, contact set changed": int(changed.shape[0]),
        "joint rates beyond 1.5 x the rollouts'": int((qdm > 1.5 * P["qdmax"]).sum()),
        "power 1.0 with actions -1, 0, +1": int((extreme & (power == 1.0)).sum()),
        "power 0.6 with actions -1, 0, +1": int((extreme & (np.abs(power - 0.6) < 1e-6)).sum()),
    }
    for name, grp in (("spine", sc.SPINE), ("leg", sc.LEG), ("arm", sc.ARM)):
        count["%s joint below lo" % name] = int((viol[:, grp] < 0).any(1).sum())
        count["%s joint above hi" % name] = int((viol[:, grp] > 0).any(1).sum())
    print("substep cases %s: %d cases; %s" % (kind, n, count))
    short = {k: v for k, v in count.items() if v < 8}
    assert not short, "classes with fewer than 8 cases: %s" % short
    assert qdm.max() >= 3.9 * P["qdmax"], "the fastest joint rate is below 4 x the rollouts' largest"
    left_out = [e for e in contact if not refs[e]["safe"]]
    print("substep cases %s: %d of %d contact cases left out of stages C and D" % (kind, len(left_out), len(contact)))
    assert len(left_out) <= LEFT_OUT_CAP * len(contact)


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_yardstick(kind):
    """K_A, K_C, K_D are 4 x the fp32 oracle's worst ratio, rounded up to a power of two (substep_cases.py).  Re-measured here: above K / 2
    the yardstick has drifted"""
    worst, used = sc.oracle_measure(kind)
    print("substep oracle yardstick %s: worst ratios A %.3g, C %.3g, D %.3g over %s cases; K_A %d, K_C %d, K_D %d" % (
        kind, worst["A"], worst["C"], worst["D"], used, sc.K_A, sc.K_C, sc.K_D))
    assert used["A"] >= 150 and used["C"] >= 100
    assert worst["A"] <= sc.K_A / 2 and worst["C"] <= sc.K_C / 2 and worst["D"] <= sc.K_D / 2, worst


# ---------------------------------------------------------------- the stages
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_stage_a_free_dynamics(flavour, kind):
    """no contact (the free-flight cases, and every other case with its stones 10 m down): the returned qd and base twist are the free
    velocities, and x = (v_f - v) / h must satisfy the equation of motion H~ x + c = tau within K_A 2^-24 of the terms' absolute values"""
    P, R = sc.prepared(kind), runs(flavour, kind)
    worst, fails, n = 0.0, [], 0
    for name, out in (("cases", R["main"]), ("stones 10 m down", R["down"])):
        a = sc.assemble(out)
        for e, r in enumerate(P["refs"]):
            if name == "cases" and P["contact"][e]:
                continue
            assert (a["key"][e] == 0).all(), "%s, case %d (%s): no stone in reach, but key = %s" % (name, e, _cls(P, e), a["key"][e])
            ratio = sc.ratio_A(r, a["v0"][e], a["qd"][e])
            n += 1
            worst = max(worst, float(ratio.max()))
            if not (ratio <= sc.K_A).all():
                i = int(np.nanargmax(np.where(np.isnan(ratio), np.inf, ratio)))
                fails.append((name, e, _cls(P, e), sc.joint_name(i), float(ratio[i] / sc.K_A)))
    print("substep %s %s stage A: n=%d worst residual / (2^-24 B) %.3f (K_A %d)" % (flavour, kind, n, worst, sc.K_A))
    assert not fails, "%d failures; (launch, case, class, component, ratio to the bound): %s" % (len(fails), fails[:8])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_stage_b_detection(flavour, kind):
    """active (from the Warm key), contact, on_target exactly wherever the fp64 margins decide them; the sole within its counted bound"""
    worst, fails, n = 0.0, [], 0
    for name, rows, refs, out, cls in _sets(flavour, kind):
        if not len(refs):
            continue
        det = sc.detect(kind, rows)
        a = sc.assemble(out)
        for e, r in enumerate(refs):
            act = _kernel_active(a, e)
            pair = r["active"].any()
            for f in (0, 1):
                safe = det["safe"][e, f]
                for k in range(4):
                    if safe[k] and pair and act[f, k] != r["active"][f, k]:
                        fails.append((name, e, cls(e), "foot %d corner %d active" % (f, k), int(act[f, k])))
                if safe.all():
                    n += 1
                    want_c, want_t = int(r["active"][f].any()), int((det["slot"][e, f] == 1).any())
                    if a["contact"][e, f] != want_c or a["on_target"][e, f] != want_t or (not pair and a["key"][e, f] != 0):
                        fails.append((name, e, cls(e), "foot %d contact / on_target / key" % f,
                                      (int(a["contact"][e, f]), int(a["on_target"][e, f]), int(a["key"][e, f]))))
                ratio = np.abs(a["sole"][e, f] - det["sole"][e, f]) / (U * det["Bsole"][e, f])
                worst = max(worst, float(ratio.max()))
                if not (ratio <= sc.K_SOLE).all():
                    fails.append((name, e, cls(e), "foot %d sole" % f, float(ratio.max() / sc.K_SOLE)))
    print("substep %s %s stage B: %d feet judged on integers; sole worst %.2f/%d" % (flavour, kind, n, worst, sc.K_SOLE))
    assert not fails, "%d failures; (launch, case, class, what, got or ratio): %s" % (len(fails), fails[:8])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_stage_c_impulses(flavour, kind):
    """Warm.lam against np_contact.pgs (five sweeps, the partner foot one sweep late, lam0 from the case's warm words) on the same fp32
    inputs; no case is excused for being near a clamp"""
    worst, fails, n, warm = 0.0, [], 0, 0
    for name, rows, refs, out, cls in _sets(flavour, kind):
        a = sc.assemble(out) if len(refs) else None
        for e, r in enumerate(refs):
            if not (r["active"].any() and r["safe"]):
                continue
            assert _agrees(a, e, r), "%s, case %d (%s): contact set %s, reference %s" % (name, e, cls(e), _kernel_active(a, e), r["active"])
            ratio = sc.ratio_C(r, sc.lam_true(a, e))
            n += 1
            warm += bool(r["warm_kept"].any())
            worst = max(worst, float(ratio.max()))
            if not (ratio <= sc.K_C).all():
                f = int(np.argmax(ratio))
                k = int(np.abs(sc.lam_true(a, e) - r["lam"]).reshape(2, 4, 3)[f].max(1).argmax())
                fails.append((name, e, cls(e), "foot %d corner %d" % (f, k), float(ratio[f] / sc.K_C)))
    print("substep %s %s stage C: n=%d (%d warm) worst |lam - lam64| / (2^-24 max|lam64|) %.1f (K_C %d)" % (flavour, kind, n, warm, worst, sc.K_C))
    assert n >= 100 and warm >= 16
    assert not fails, "%d failures; (launch, case, class, corner, ratio to the bound): %s" % (len(fails), fails[:8])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_stage_d_response(flavour, kind):
    """the kernel's velocity change (the contact run minus the run with the stones 10 m down, both its own) is H~^-1 J^T W^T lambda of
    its OWN impulses: imp_up, the pair sum, the base solve, both down-sweeps and the arms, independent of any error in the impulses"""
    P, R = sc.prepared(kind), runs(flavour, kind)
    a, b = sc.assemble(R["main"]), sc.assemble(R["down"])
    worst, fails, n = 0.0, [], 0
    for e, r in enumerate(P["refs"]):
        if not (r["active"].any() and r["safe"] and _agrees(a, e, r)):
            continue
        va, vb = np.concatenate([a["v0"][e], a["qd"][e]]), np.concatenate([b["v0"][e], b["qd"][e]])
        ref, B = sc.response(r, sc.lam_true(a, e))
        err = np.abs((va - vb) - ref)
        tol = U * (sc.K_D * B + np.abs(va) + np.abs(vb))          # the subtraction of two fp32 results adds 2^-24 (|a| + |b|)
        ratio = err / tol
        n += 1
        worst = max(worst, float(ratio.max()))
        if not (ratio <= 1).all():
            i = int(np.argmax(ratio))
            fails.append((e, _cls(P, e), sc.joint_name(i), float(ratio[i])))
    print("substep %s %s stage D: n=%d worst err / bound %.3f (K_D %d)" % (flavour, kind, n, worst, sc.K_D))
    assert n >= 100
    assert not fails, "%d failures; (case, class, component, ratio to the bound): %s" % (len(fails), fails[:8])


def _quat_rot_abs(q):
    w, x, y, z = np.abs(q)
    return np.array([[1 + 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 + 2 * (x * x + z * z), 2 * (y * z + w * x)],
                     [2 * (x * z + w * y), 2 * (y * z + w * x), 1 + 2 * (x * x + y * y)]])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_stage_e_integration(flavour, kind):
    """from the kernel's own new qd and base twist, per lane in the lane's world: q' = q + h qd', pos through Rb, the quaternion update and
    its normalisation, each within its counted roundings"""
    import np_dynamics as nd
    h, hh = sc.H32, float(np.float32(0.5) * np.float32(sc.H32))
    worst = {"q": 0.0, "pos": 0.0, "quat": 0.0}
    fails = []
    for name, rows, refs, out, cls in _sets(flavour, kind):
        x = rows.astype(np.float64)
        o = np.asarray(out, np.float64).reshape(-1, 2, sc.OWL)
        for e in range(x.shape[0]):
            for side in (0, 1):
                l = o[e, side]
                q0 = x[e, sc.I_Q + sc.LANE_JOINT[side]] * sc.LANE_SIGN[side]
                pos0 = x[e, sc.I_POS:sc.I_POS + 3] * (sc.M_POS if side else 1.0)
                qt0 = x[e, sc.I_QUAT:sc.I_QUAT + 4] * (sc.M_QUAT if side else 1.0)
                qd1, w1, v1 = l[sc.O_QD:sc.O_QD + 12], l[sc.O_W:sc.O_W + 3], l[sc.O_V:sc.O_V + 3]
                checks = [("q", l[sc.O_Q:sc.O_Q + 12], q0 + h * qd1, np.abs(q0) + h * np.abs(qd1), sc.K_Q)]
                checks.append(("pos", l[sc.O_POS:sc.O_POS + 3], pos0 + h * (nd.quat_rot(qt0) @ v1),
                               np.abs(pos0) + h * (_quat_rot_abs(qt0) @ np.abs(v1)), sc.K_POS))
                qw, qx, qy, qz = qt0
                ox, oy, oz = w1
                nq = np.array([qw + hh * (-qx * ox - qy * oy - qz * oz), qx + hh * (qw * ox + qy * oz - qz * oy),
                               qy + hh * (qw * oy - qx * oz + qz * ox), qz + hh * (qw * oz + qx * oy - qy * ox)])
                Bn = np.abs(qt0) + hh * np.array([
                    abs(qx * ox) + abs(qy * oy) + abs(qz * oz), abs(qw * ox) + abs(qy * oz) + abs(qz * oy),
                    abs(qw * oy) + abs(qx * oz) + abs(qz * ox), abs(qw * oz) + abs(qx * oy) + abs(qy * ox)])
                s, Bs = (nq * nq).sum(), (Bn * Bn).sum()
                Binv = max(0.5 * s ** -1.5 * Bs, s ** -0.5)
                checks.append(("quat", l[sc.O_QUAT:sc.O_QUAT + 4], nq / np.sqrt(s), Bn * Binv, sc.K_QUAT))
                for what, got, ref, B, K in checks:
                    ratio = np.abs(got - ref) / (U * B)
                    worst[what] = max(worst[what], float(ratio.max()))
                    if not (ratio <= K).all():
                        fails.append((name, e, cls(e), "lane %d %s[%d]" % (side, what, int(np.argmax(ratio))), float(ratio.max() / K)))
    print("substep %s %s stage E: worst err/(2^-24 B): q %.2f/%d, pos %.2f/%d, quat %.2f/%d" % (
        flavour, kind, worst["q"], sc.K_Q, worst["pos"], sc.K_POS, worst["quat"], sc.K_QUAT))
    assert not fails, "%d failures; (launch, case, class, component, ratio to the bound): %s" % (len(fails), fails[:8])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_stage_f_invariants(flavour, kind):
    """exact: the two lanes' base copies and spine joints equal up to the mirror signs; the mirrored robot among mirrored stones returns the
    mirrored output (the lanes swapped) bit for bit; a pair without an active corner returns key 0 and the very bits of the run with the
    stones 10 m down; the second substep gives the same bits as two calls in one launch or with the first call's output taken through the
    host.  (Signs are applied as factors and compared as values: the kernels are built with -fno-signed-zeros.)"""
    P, R = sc.prepared(kind), runs(flavour, kind)
    base_sign = np.concatenate([sc.M_POS, sc.M_QUAT, sc.M_ANG, sc.M_POS])
    for name in ("main", "down", "mirror", "second", "two", "changed"):
        o = np.asarray(R[name], np.float32).reshape(-1, 2, sc.OWL)
        assert np.isfinite(o).all(), "%s: a non-finite output" % name
        bad = np.nonzero((o[:, 0, sc.O_POS:sc.O_POS + 13] != o[:, 1, sc.O_POS:sc.O_POS + 13] * base_sign.astype(np.float32)).any(1))[0]
        assert bad.size == 0, "%s: the lanes' base copies differ in cases %s (first: %s)" % (name, bad[:8].tolist(), _cls(P, int(bad[0])) if name in ("main", "down", "mirror") else name)
        for off in (sc.O_Q, sc.O_QD):
            bad = np.nonzero((o[:, 0, off:off + 3] != o[:, 1, off:off + 3] * sc.LANE_SIGN[1][:3].astype(np.float32)).any(1))[0]
            assert bad.size == 0, "%s: the lanes' spine joints differ in cases %s" % (name, bad[:8].tolist())
    main = np.asarray(R["main"], np.float32).reshape(-1, 2, sc.OWL)
    mir = np.asarray(R["mirror"], np.float32).reshape(-1, 2, sc.OWL)
    bad = np.nonzero((main[:, ::-1] != mir).any((1, 2)))[0]
    assert bad.size == 0, "the mirrored robot does not return the mirrored output: cases %s (first: %s, words %s)" % (
        bad[:8].tolist(), _cls(P, int(bad[0])), np.nonzero((main[bad[0], ::-1] != mir[bad[0]]).ravel())[0][:8].tolist())
    a = sc.assemble(R["main"])
    down = np.asarray(R["down"], np.float32).reshape(-1, 2, sc.OWL)
    idle = np.nonzero((a["key"] == 0).all(1) & ~P["contact"])[0]
    assert idle.size >= 8
    words = list(range(sc.O_QD, sc.O_QD + 12)) + list(range(sc.O_W, sc.O_W + 6))
    assert (_bits(main[idle][:, :, words]) == _bits(down[idle][:, :, words])).all(), "a pair without contact: a velocity change that is not 0"
    for e in np.nonzero(~P["contact"])[0]:
        assert (a["key"][e] == 0).all(), "case %d (%s): no active corner but key %s" % (e, _cls(P, e), a["key"][e])
    two, second = _bits(R["two"]), _bits(R["second"])
    bad = np.nonzero((two != second).any(1))[0]
    assert bad.size == 0, "two calls and a round trip through the host differ: feedback cases %s" % bad[:8].tolist()
