"""fp64 references, running error bounds and test cases for the contact stage of ss_dynamics.hpp (fk_detect, jacobian_rows / row_moment,
operator_T / operator_up / operator_pair_b) and the env formulas of ss_kernels.hpp, as tests/device/ss_probe.hip exposes them.  Used by
tests/test_contact_ops.py; the judgement is np_spatial.judge: |got - ref| <= k * 2^-24 * B, exact where B = 0.

Counting.  An input of the probe carries no rounding (the reference starts from the same fp32 numbers).  A table constant counts one.
k(x + y) = max(k(x), k(y)) + 1 with B(x + y) = B(x) + B(y);  k(x * y) = k(x) + k(y) + 1 with B(x * y) = B(x) B(y) (both operands' errors
reach the product);  k(f(x)) = k(x) + k_f with B = max(|f'(x)| B(x), |f(x)|) for a library call f.  Every k below is derived that way
in the docstring of its op, from the source alone.  Library calls: no accuracy statement of the ROCm device library is installed beside
the compiler, so the OpenCL full-profile limits are used for both flavours (glibc's documented errors are inside them); one ulp is at
most two roundings.  SS_RSQRT counts two, as np_spatial.chol_judge counts it (the doubled textbook bound).

The model is np_contact.rounded_model(kind): the fp32 values the generated tables hold, NOT read from those tables."""
import functools

import numpy as np

import np_contact as nc
import np_dynamics as nd
import np_spatial as ns
from steppingstone_amd import model as M

U = ns.U
KINDS = ns.KINDS
N_RANDOM = 2048
# external constants: OpenCL 3.0 full profile, single precision, in ulp
OPENCL_ULP = {"sincos": 4, "asin": 4, "atan2": 6, "sqrt": 3, "exp": 3}
K_SINCOS, K_ASIN, K_ATAN2, K_SQRT = (2 * OPENCL_ULP[f] for f in ("sincos", "asin", "atan2", "sqrt"))
K_RSQRT = 2
F32 = np.float32
REACH = float(F32(0.10))
PLANK_A, PLANK_B = float(F32(nc.PLANK_A)), float(F32(nc.PLANK_B))          # the kernel's fp32 kPlankA / kPlankB
SLOP, ERP, VMAX = float(F32(nc.SLOP)), float(F32(nc.ERP)), nc.VCORR_MAX
INV_H = float(F32(1.0) / (F32(1.0) / F32(240.0)))
MIRROR = ns.MIRROR


@functools.lru_cache(maxsize=None)
def model(kind):
    return nc.rounded_model(kind)


def _rng(name, kind):
    return np.random.default_rng([sum(name.encode()), KINDS.index(kind), 77031])


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def _pad(rows, again):
    """float32 rows, never a multiple of 64 (the device build must meet a partial wavefront)"""
    rows = list(rows)
    if len(rows) % 64 == 0:
        rows.append(again)
    return np.asarray(rows, np.float64).astype(np.float32)


def judge_cols(got, ref, B, exact, k):
    """np_spatial.judge with a k per column -> ({k: worst err / (2^-24 B) over the columns with that k}, failures)"""
    k = np.asarray(k, np.float64)
    worst, fails = {}, []
    for kv in np.unique(k):
        c = np.nonzero(k == kv)[0]
        w, f = ns.judge(got[:, c], ref[:, c], B[:, c], exact[:, c], kv)
        worst[int(kv)] = w
        fails += [(e, int(c[col]), g, r, ratio) for e, col, g, r, ratio in f]
    return worst, fails


def show(worst):
    """'ratio/k' per group of columns, and the largest share of a bound that is used"""
    txt = ", ".join("%.2f/%d" % (w, k) for k, w in sorted(worst.items()) if k > 0)
    return "%s; largest share of a bound %.3f" % (txt, max([w / k for k, w in worst.items() if k > 0] + [0.0]))


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---------------------------------------------------------------- batched pieces
def rot_b(ax, c, s):
    """[n,3,3] active rotation about axis ax from given cos / sin (np_spatial.rot_cs, batched)"""
    i, j = (ax + 1) % 3, (ax + 2) % 3
    R = np.zeros(c.shape + (3, 3))
    R[..., ax, ax] = 1.0
    R[..., i, i] = c
    R[..., i, j] = -s
    R[..., j, i] = s
    R[..., j, j] = c
    return R


def xform_b(ax, c, s, r):
    """(X, |X|) [n,6,6] of a joint: X = xform(R^T, r), every factor's absolute value in |X| (np_spatial.joint_xform, batched)"""
    E = np.swapaxes(rot_b(ax, c, s), -1, -2)
    S = nd.skew(r)
    X = np.zeros(c.shape + (6, 6))
    aX = np.zeros_like(X)
    X[..., :3, :3] = X[..., 3:, 3:] = E
    X[..., 3:, :3] = -E @ S
    aX[..., :3, :3] = aX[..., 3:, 3:] = np.abs(E)
    aX[..., 3:, :3] = np.abs(E) @ np.abs(S)
    return X, aX


def quat_rot_b(q):
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)
    return R.reshape(q.shape[:-1] + (3, 3))


def stone_normal_b(phi, xt, yt):
    a = np.stack([np.cos(xt) * np.sin(yt), -np.sin(xt), np.cos(xt) * np.cos(yt)], -1)
    c, s = np.cos(phi), np.sin(phi)
    return np.stack([c * a[..., 0] - s * a[..., 1], s * a[..., 0] + c * a[..., 1], a[..., 2]], -1)


# ================================================================ fk_detect
# k, counted on fk_detect's source (c, s, Rb, pos, stones are inputs; Model::r, Model::corners are table constants):
#   Rw[b] = c Rw[p] +- s Rw[p]'                      k(R_b) = k(R_p) + 2               -> Rf (8 joints)          16
#   pw[b] = pw[p] + r . Rw[p] (3 accumulations)      k = max(k(pw_p), 1 + k(R_p) + 1) + 3 = 5, 8, .. -> pf      26
#   P = pf + Rf . corner                             max(26, 1 + 16 + 1) + 3                                     29
#   sole = sum of 0.25 P (0.25 is exact)             29 + 4                                                      33
#   d = (P - sp) . n                                 (29 + 1) + 0 + 1, + 2 additions        -> pen = -d          33
#   l = (P - sp) - d n                               max(30, 33 + 1) + 1 = 35;   u, v = l . heading: 35 + 1 + 1  37
K_RF, K_SOLE, K_D, K_UV = 16, 33, 33, 37
FK_K = np.array([K_RF] * 9 + [K_D] * 4 + [0] * 4 + [K_SOLE] * 3, np.float64)
VISIT = (1, 0, 2)


def fk_foot(m, cs, sn, Rb, pos):
    """Right foot from cos / sin of joints 0..7: (Rf, |.| bound, pf, bound), batched; Rw[b] = Rw[p] rot, pw[b] = pw[p] + Rw[p] r"""
    R, BR, p, Bp = Rb, np.abs(Rb), pos, np.abs(pos)
    for j in range(8):
        assert M.PARENT[j] == j
        r = m["r"][j]
        p, Bp = p + R @ r, Bp + BR @ np.abs(r)
        Rj = rot_b(M.AXIS[j], cs[:, j], sn[:, j])
        R, BR = R @ Rj, BR @ np.abs(Rj)
    return R, BR, p, Bp


def detect_ref(kind, inp):
    """fp64 detection of the right foot from the probe's input rows -> dict: ref / B [n,20] of one coding's output row, per corner the
    safe mask, the integer decisions and the candidates of pen"""
    m = model(kind)
    x = inp.astype(np.float64)
    n = x.shape[0]
    cs, sn, Rb, pos = x[:, 0:8], x[:, 8:16], x[:, 16:25].reshape(n, 3, 3), x[:, 25:28]
    st = x[:, 28:52].reshape(n, 3, 8)
    Rf, BRf, pf, Bpf = fk_foot(m, cs, sn, Rb, pos)
    ref, B = np.zeros((n, 20)), np.zeros((n, 20))
    ref[:, :9], B[:, :9] = Rf.reshape(n, 9), BRf.reshape(n, 9)
    safe = np.ones((n, 4), bool)
    slot = np.full((n, 4), -1)
    pen_cand = np.zeros((n, 4, 4))          # 0, and -d of the three stones
    pen_B = np.zeros((n, 4, 4))
    margins = np.zeros((n, 4, 3, 5))        # margin / tolerance of every predicate (information, and the edge cases' placement)
    tols = np.zeros((n, 4, 3, 5))
    P_all = np.zeros((n, 4, 3))
    for k in range(4):
        c = m["corners"][k]
        P, BP = pf + Rf @ c, Bpf + BRf @ np.abs(c)
        P_all[:, k] = P
        ref[:, 17:20] += 0.25 * P
        B[:, 17:20] += 0.25 * BP
        best, Bbest, best_sl = np.zeros(n), np.zeros(n), np.full(n, -1)
        for sl in VISIT:
            sp, nr, hc, hs = st[:, sl, 0:3], st[:, sl, 3:6], st[:, sl, 6], st[:, sl, 7]
            dx, Bdx = P - sp, BP + np.abs(sp)
            d, Bd = (dx * nr).sum(1), (Bdx * np.abs(nr)).sum(1)
            l, Bl = dx - d[:, None] * nr, Bdx + Bd[:, None] * np.abs(nr)
            u, Bu = l[:, 0] * hc + l[:, 1] * hs, Bl[:, 0] * np.abs(hc) + Bl[:, 1] * np.abs(hs)
            v, Bv = l[:, 1] * hc - l[:, 0] * hs, Bl[:, 1] * np.abs(hc) + Bl[:, 0] * np.abs(hs)
            # margins (> 0: the predicate holds) and their tolerances
            mg = np.stack([-d, d + REACH, PLANK_A - np.abs(u), PLANK_B - np.abs(v), best - d], 1)
            tl = U * np.stack([K_D * Bd, K_D * Bd, K_UV * Bu, K_UV * Bv, K_D * (Bd + Bbest)], 1)
            # d < best against a stone with the very same data compares two identical computations: false, and exactly so
            same = np.zeros(n, bool)
            for other in range(3):
                same |= (best_sl == other) & (st[:, sl] == st[:, other]).all(1) & (other != sl)
            tie = same & (mg[:, 4] == 0)
            true_safe = (mg > tl).all(1)
            false_safe = (mg < -tl).any(1) | tie
            touch = (mg > 0).all(1)
            safe[:, k] &= true_safe | false_safe
            margins[:, k, sl], tols[:, k, sl] = mg, tl
            best, Bbest = np.where(touch, d, best), np.where(touch, Bd, Bbest)
            best_sl = np.where(touch, sl, best_sl)
            pen_cand[:, k, 1 + sl], pen_B[:, k, 1 + sl] = -d, Bd
        slot[:, k] = best_sl
        ref[:, 9 + k], B[:, 9 + k] = -best, Bbest
    active = (slot >= 0).astype(np.int64)
    ref[:, 13] = (active << np.arange(4)).sum(1)
    ref[:, 14] = (np.where(slot >= 0, slot, 0) << (2 * np.arange(4))).sum(1)
    ref[:, 15] = active.any(1)
    ref[:, 16] = (slot == 1).any(1)
    return dict(ref=ref, B=B, safe=safe, slot=slot, pen_cand=pen_cand, pen_B=pen_B, margins=margins, tols=tols, P=P_all)


def _stone_row(centre, phi=0.0, xt=0.0, yt=0.0):
    """centre 3, unit normal 3, cos / sin of the heading: what the step kernel keeps of a stone"""
    return np.concatenate([centre, stone_normal_b(np.float64(phi), np.float64(xt), np.float64(yt)), [np.cos(phi), np.sin(phi)]])


def _pose_row(m, q8, quat, pos):
    return np.concatenate([np.cos(q8), np.sin(q8), nd.quat_rot(quat).reshape(9), pos])


def _corners_of(kind, pose):
    """fp64 world positions [4,3] of the sole corners as the reference sees them from the fp32 pose row"""
    row = np.concatenate([f32(pose), np.zeros(24, np.float32)])[None]
    return detect_ref(kind, row)["P"][0]


FAR = np.array([50.0, 50.0, -20.0])


def _flat_pose(m):
    """identity base, bent leg, the ankle cancelling hip and knee: the foot is axis aligned and level to rounding (what the constructions
    below assume)"""
    q8 = np.zeros(8)
    q8[5], q8[6] = m["q0"][5], m["q0"][6]
    q8[7] = -(q8[5] + q8[6])
    return _pose_row(m, q8, np.array([1.0, 0, 0, 0]), np.array([0.0, 0.0, 1.0]))


def detect_edges(kind):
    """[(name, row, expect)]: expect maps 'active' / 'cslot' / 'contact' / 'on_target' or ('slot', corner) / ('on', corner) to the stated
    integer.  Stones are flat with heading 0 unless said otherwise, so that d, u, v of a corner are coordinate differences."""
    m = model(kind)
    pose = _flat_pose(m)
    P = _corners_of(kind, pose)
    far = _stone_row(FAR)
    out = []

    def row(s0, s1, s2):
        return np.concatenate([pose, s0, s1, s2])

    def under(k, d, du=0.0, dv=0.0, centred=False, **kw):
        """a stone that sees corner k at signed distance d (d < 0: below its surface) and at the in-plane offset (du, dv) from its centre;
        centred: the centre under the middle of the sole instead"""
        xy = P.mean(0)[:2] if centred else P[k, :2] - np.array([du, dv])
        return _stone_row(np.array([xy[0], xy[1], P[k, 2] - d]), **kw)
    # ---- ties
    s = under(0, -0.02)
    out.append(("tie: three identical stones", row(s, s, s), {("slot", 0): 1, ("on", 0): 1, "on_target": 1}))
    out.append(("tie: n and n+1 identical, n-1 out of reach", row(far, s, s), {("slot", 0): 1, ("on", 0): 1, "on_target": 1}))
    out.append(("tie: n-1 and n+1 identical, n out of reach", row(s, far, s), {("slot", 0): 0, ("on", 0): 1, "on_target": 0}))
    # ---- predicate boundaries: corner 0 at +-16 x the predicate's own tolerance from its threshold
    def boundary(name, pred, make, inside_expect, outside_expect):
        for side, expect in ((+1.0, inside_expect), (-1.0, outside_expect)):
            # the tolerance depends (weakly) on the placement: place, read the reference's tolerance, place again
            tol = 1e-5
            for _ in range(3):
                r = row(*make(side * 16.0 * tol))
                ref = detect_ref(kind, f32(r)[None])
                sl = 0 if pred == 4 else 1
                tol = ref["tols"][0, 0, sl, pred]
            mg = ref["margins"][0, 0, sl, pred]
            assert 8 * tol < side * mg < 32 * tol, (name, side, mg, tol)
            out.append(("boundary %s, %s" % (name, "holds" if side > 0 else "fails"), r, expect))
    on1, off = {("on", 0): 1, ("slot", 0): 1}, {("on", 0): 0}
    boundary("d < 0", 0, lambda e: (far, under(0, -e), far), on1, off)
    boundary("d > -0.10", 1, lambda e: (far, under(0, -REACH + e), far), on1, off)
    boundary("|u| < kPlankA", 2, lambda e: (far, under(0, -0.02, du=PLANK_A - e), far), on1, off)
    boundary("|v| < kPlankB", 3, lambda e: (far, under(0, -0.02, dv=-(PLANK_B - e)), far), on1, off)
    boundary("d < best", 4, lambda e: (under(0, -0.02 - e), under(0, -0.02), far), {("on", 0): 1, ("slot", 0): 0}, {("on", 0): 1, ("slot", 0): 1})
    # ---- footprint orientation: 0.4 m lies between kPlankA and kPlankB
    assert PLANK_A < 0.4 < PLANK_B
    out.append(("heading 0, 0.4 m along x: the front corners are outside", row(far, under(0, -0.02, du=0.4), far), {("on", 0): 0, ("on", 1): 0}))
    out.append(("heading 90 deg, 0.4 m along x: inside", row(far, under(0, -0.02, du=0.4, phi=np.pi / 2), far), {"active": 15, "cslot": 0x55}))
    for name, ang, expect in (("along", 0.0, {("on", 0): 0}), ("across", np.pi / 2, {("on", 0): 1, ("slot", 0): 1, "on_target": 1})):
        h = np.radians(30.0) + ang
        out.append(("heading 30 deg, 0.4 m %s the heading" % name,
                    row(far, under(0, -0.02, du=0.4 * np.cos(h), dv=0.4 * np.sin(h), phi=np.radians(30.0)), far), expect))
    # ---- the deeper stone is not the target
    out.append(("deepest stone is n+1", row(far, under(0, -0.01, centred=True), under(0, -0.03, centred=True)), {"active": 15, "cslot": 0xAA, "on_target": 0, "contact": 1}))
    out.append(("deepest stone is n-1", row(under(0, -0.03, centred=True), under(0, -0.01, centred=True), far), {"active": 15, "cslot": 0x00, "on_target": 0, "contact": 1}))
    # ---- all corners inactive; all four active on three different slots (corners: 0 front -y, 1 front +y, 2 rear -y, 3 rear +y)
    out.append(("nothing in reach", row(far, far, far), {"active": 0, "cslot": 0, "contact": 0, "on_target": 0}))
    xm, ym = 0.5 * (P[0, 0] + P[2, 0]), 0.5 * (P[0, 1] + P[1, 1])
    zt = P[:, 2].max()
    rear = _stone_row(np.array([xm - PLANK_A, ym, zt + 0.03]))                       # front edge between rear and front corners, deepest there
    mid = _stone_row(np.array([xm, ym, zt + 0.02]))
    front_left = _stone_row(np.array([xm + PLANK_A, ym + PLANK_B, zt + 0.04]))     # covers corner 1 only
    out.append(("four corners on three slots", row(rear, mid, front_left),
                {"active": 15, "cslot": 1 | (2 << 2) | (0 << 4) | (0 << 6), "contact": 1, "on_target": 1}))
    return out


def _random_detect_rows(kind, n):
    rng, m = _rng("fk_detect", kind), model(kind)
    lo, hi = m["range"][:8, 0], m["range"][:8, 1]
    rows = []
    for _ in range(n):
        q8 = rng.uniform(lo, hi)
        yaw, roll, pitch = rng.uniform(-np.pi, np.pi), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)
        qz = np.array([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)])
        qy = np.array([np.cos(pitch / 2), 0, np.sin(pitch / 2), 0])
        qx = np.array([np.cos(roll / 2), np.sin(roll / 2), 0, 0])
        quat = _qmul(_qmul(qz, qy), qx)
        pose = _pose_row(m, q8, quat, rng.uniform(-3, 3, 3) + np.array([5.0, 0, 1.0]))
        P = _corners_of(kind, pose)
        c = P.mean(0)
        phi = rng.uniform(-np.pi, np.pi)
        tilt = np.radians(15.0)
        stones = []
        for sl in range(3):
            # around the sole: sideways up to past the plank's edge, vertically from clear of it to out of reach
            off = np.array([rng.uniform(-0.7, 0.7), rng.uniform(-0.7, 0.7), rng.uniform(-0.02, 0.13)])
            stones.append(_stone_row(c + off, phi + rng.uniform(-0.4, 0.4), rng.uniform(-tilt, tilt), rng.uniform(-tilt, tilt)))
        rows.append(np.concatenate([pose] + stones))
    return rows


def _qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


@functools.lru_cache(maxsize=None)
def detect_prepared(kind):
    edges = detect_edges(kind)
    rows = _random_detect_rows(kind, N_RANDOM) + [e[1] for e in edges]
    inp = _pad(rows, rows[0])
    d = detect_ref(kind, inp)
    d.update(inp=inp, n_random=N_RANDOM, edges=[(name, N_RANDOM + i, exp) for i, (name, _, exp) in enumerate(edges)])
    return _frozen(d)


def detect_judge(got, d):
    """one coding's 20 columns against the reference -> ({k: worst ratio}, failures)"""
    ref, B, safe = d["ref"], d["B"], d["safe"]
    fl = [c for c in range(20) if c not in (9, 10, 11, 12, 13, 14, 15, 16)]
    worst, fails = judge_cols(got[:, fl], ref[:, fl], B[:, fl], np.zeros((got.shape[0], len(fl)), bool), FK_K[fl])
    g = got.astype(np.float64)
    # pen: a safe corner against the reference's stone; any other against the nearest admissible outcome (no touch, or one of the stones)
    for k in range(4):
        err = np.abs(g[:, 9 + k, None] - d["pen_cand"][:, k])
        ok = err <= K_D * U * d["pen_B"][:, k]
        ok[:, 0] = g[:, 9 + k] == 0
        idx = np.where(d["slot"][:, k] >= 0, 1 + d["slot"][:, k], 0)
        ok_safe = ok[np.arange(g.shape[0]), idx]
        bad = np.where(safe[:, k], ~ok_safe, ~ok.any(1))
        fails += [(int(e), 9 + k, float(g[e, 9 + k]), float(ref[e, 9 + k]), float("nan")) for e in np.nonzero(bad)[0]]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(d["pen_B"][:, k, 1:] > 0, err[:, 1:] / (U * d["pen_B"][:, k, 1:]), 0.0)
        sel = safe[:, k] & (d["slot"][:, k] >= 0)
        if sel.any():
            worst[K_D] = max(worst.get(K_D, 0.0), float(r[sel, d["slot"][sel, k]].max()))
    # integers: per corner where the reference's margins decide; the whole words where all four do
    act, cs_ = g[:, 13].astype(np.int64), g[:, 14].astype(np.int64)
    for k in range(4):
        on = (act >> k) & 1
        sl = (cs_ >> (2 * k)) & 3
        want_on = (d["slot"][:, k] >= 0).astype(np.int64)
        bad = safe[:, k] & ((on != want_on) | ((want_on == 1) & (sl != d["slot"][:, k])) | ((want_on == 0) & (sl != 0)))
        fails += [(int(e), "corner %d" % k, (int(on[e]), int(sl[e])), int(d["slot"][e, k]), float("nan")) for e in np.nonzero(bad)[0]]
    allsafe = safe.all(1)
    for c in (13, 14, 15, 16):
        bad = allsafe & (g[:, c] != ref[:, c])
        fails += [(int(e), c, float(g[e, c]), float(ref[e, c]), float("nan")) for e in np.nonzero(bad)[0]]
    return worst, fails


def edge_value(got_row, key):
    """the integer an edge case states, read from one coding's output row"""
    act, cs_ = int(got_row[13]), int(got_row[14])
    if key == "active":
        return act
    if key == "cslot":
        return cs_
    if key == "contact":
        return int(got_row[15])
    if key == "on_target":
        return int(got_row[16])
    what, k = key
    return (act >> k) & 1 if what == "on" else (cs_ >> (2 * k)) & 3


# ================================================================ jacobian_rows
# k, counted on jacobian_rows / row_moment (Rf, pen, the normals are inputs; corners, kSlop, kErp, 1 / kH are constants):
#   t1 = (1 - n0 n0, -n0 n1, -n0 n2)   k 2, 1, 1        ss = t1 . t1: (2 + 2 + 1), + 2 additions = 7      inv = rsqrt(ss): 7 + 2 = 9
#   t1 *= inv: 2 + 9 + 1 = 12           t2 = n x t1: 0 + 12 + 1, - : 14
#   direction part  w[3 + c] = Rf[.][c] . dir: k(dir) + 0 + 1, + 2 additions         n: 3     t1: 15     t2: 17
#   moment part     corner x w: 1 + k(w) + 1, - : + 1                                   n: 6     t1: 18     t2: 20
#   rB = min(kErp * max(pen - kSlop, 0) * (1 / kH), kVcorrMax): (1 + 1 = 2), * kErp: 1 + 2 + 1 = 4, * (1 / kH): 4 + 1 + 1 = 6
ROWS_K = np.array(([6] * 3 + [3] * 3 + [18] * 3 + [15] * 3 + [20] * 3 + [17] * 3) * 4 + [6] * 4, np.float64)
TILT = np.radians(15.0)


def rows_ref(kind, inp):
    m = model(kind)
    x = inp.astype(np.float64)
    n = x.shape[0]
    Rf, pen = x[:, :9].reshape(n, 3, 3), x[:, 9:13]
    active, cslot = x[:, 13].astype(np.int64), x[:, 14].astype(np.int64)
    nrm = x[:, 15:24].reshape(n, 3, 3)
    ref, B = np.zeros((n, 76)), np.zeros((n, 76))
    ez = np.array([0.0, 0.0, 1.0])
    for k in range(4):
        on = ((active >> k) & 1).astype(bool)
        sl = (cslot >> (2 * k)) & 3
        nv = np.where(on[:, None], nrm[np.arange(n), np.minimum(sl, 2)], ez)
        t1 = np.stack([1 - nv[:, 0] * nv[:, 0], -nv[:, 0] * nv[:, 1], -nv[:, 0] * nv[:, 2]], 1)
        Bt1 = np.stack([1 + nv[:, 0] ** 2, np.abs(nv[:, 0] * nv[:, 1]), np.abs(nv[:, 0] * nv[:, 2])], 1)
        ss, Bss = (t1 * t1).sum(1), (Bt1 * Bt1).sum(1)
        inv = 1.0 / np.sqrt(ss)
        Binv = inv * np.maximum(0.5 * Bss / ss, 1.0)
        t1n, Bt1n = t1 * inv[:, None], Bt1 * Binv[:, None]
        t2 = np.cross(nv, t1n)
        an = np.abs(nv)
        Bt2 = np.stack([an[:, 1] * Bt1n[:, 2] + an[:, 2] * Bt1n[:, 1], an[:, 2] * Bt1n[:, 0] + an[:, 0] * Bt1n[:, 2],
                        an[:, 0] * Bt1n[:, 1] + an[:, 1] * Bt1n[:, 0]], 1)
        c = m["corners"][k]
        for d_, (dv, Bdv) in enumerate(((nv, an), (t1n, Bt1n), (t2, Bt2))):
            w = np.einsum("nrc,nr->nc", Rf, dv)
            Bw = np.einsum("nrc,nr->nc", np.abs(Rf), Bdv)
            mo = np.cross(c, w)
            ac = np.abs(c)
            Bmo = np.stack([ac[1] * Bw[:, 2] + ac[2] * Bw[:, 1], ac[2] * Bw[:, 0] + ac[0] * Bw[:, 2], ac[0] * Bw[:, 1] + ac[1] * Bw[:, 0]], 1)
            o = (3 * k + d_) * 6
            ref[:, o:o + 3], ref[:, o + 3:o + 6], B[:, o:o + 3], B[:, o + 3:o + 6] = mo, w, Bmo, Bw
        bn = np.minimum(ERP * np.maximum(pen[:, k] - SLOP, 0.0) * INV_H, VMAX)
        ref[:, 72 + k] = np.where(on, bn, 0.0)
        B[:, 72 + k] = np.where(on, ERP * (np.abs(pen[:, k]) + SLOP) * INV_H, 0.0)
    return ref, B


def rows_vs_np_contact(kind, inp, ref, every=16):
    """largest difference between rows_ref and np_contact.rows, and the largest one to pgs's bn in units of 2^-24 kErp (pen + kSlop) / h
    (pgs has kErp, kSlop and h in fp64, the reference the kernel's fp32 constants: one rounding each), on the active corners of every
    `every`-th case"""
    m = nc.rounded_model(kind)
    worst, worst_bn = 0.0, 0.0
    for e in range(0, inp.shape[0], every):
        x = inp[e].astype(np.float64)
        for k in range(4):
            if not (int(x[13]) >> k) & 1:
                continue
            sl = (int(x[14]) >> (2 * k)) & 3
            c = dict(n=x[15 + 3 * sl:18 + 3 * sl], Rf=x[:9].reshape(3, 3), r=m["corners"][k], pen=x[9 + k])
            W = nc.rows(c)
            bn = min(nc.ERP * max(c["pen"] - nc.SLOP, 0.0) / nc.H, nc.VCORR_MAX)
            worst = max(worst, np.abs(W.reshape(18) - ref[e, 18 * k:18 * k + 18]).max())
            worst_bn = max(worst_bn, abs(bn - ref[e, 72 + k]) / (U * ERP * (c["pen"] + SLOP) * INV_H))
    return worst, worst_bn


def _unit_normal(rng, xt=None, yt=None, phi=None):
    return stone_normal_b(np.float64(rng.uniform(-np.pi, np.pi) if phi is None else phi),
                          np.float64(rng.uniform(-TILT, TILT) if xt is None else xt), np.float64(rng.uniform(-TILT, TILT) if yt is None else yt))


def _random_rot(rng):
    q = rng.normal(size=4)
    return nd.quat_rot(q / np.linalg.norm(q))


@functools.lru_cache(maxsize=None)
def rows_prepared(kind):
    rng = _rng("jacobian_rows", kind)
    rows = []

    def one(pen, active, cslot, normals=None, Rf=None):
        nr = np.concatenate([_unit_normal(rng) for _ in range(3)]) if normals is None else np.concatenate(normals)
        return np.concatenate([(_random_rot(rng) if Rf is None else Rf).reshape(9), pen, [active, cslot], nr])
    for _ in range(N_RANDOM):
        cslot = sum(int(rng.integers(0, 3)) << (2 * k) for k in range(4))
        rows.append(one(10.0 ** rng.uniform(-4.5, -0.9, 4), int(rng.integers(0, 16)), cslot))
    edges = {}
    edges["inactive"] = len(rows)          # finite +z rows, rB = 0
    rows.append(one(np.array([0.02] * 4), 0, 0x24))
    edges["pen"] = len(rows)               # at, below, above kSlop; large enough to clamp at kVcorrMax
    rows.append(one(np.array([SLOP, 0.5 * SLOP, 2.0 * SLOP, 0.09]), 15, 0x55))
    edges["tilt"] = len(rows)              # 15 degrees on both axes, all four sign pairs, any heading
    for sx in (-1, 1):
        for sy in (-1, 1):
            nr = [_unit_normal(rng, sx * TILT, sy * TILT) for _ in range(3)]
            rows.append(one(np.array([0.01] * 4), 15, 0x18, normals=nr))
    edges["flat"] = len(rows)              # flat stones under a level foot: t1 = x, t2 = y exactly
    rows.append(one(np.array([0.01] * 4), 15, 0x66, normals=[np.array([0.0, 0, 1])] * 3, Rf=np.eye(3)))
    inp = _pad(rows, rows[0])
    ref, B = rows_ref(kind, inp)
    return _frozen(dict(inp=inp, ref=ref, B=B, edges=edges))


# ================================================================ contact-space operators
# Judged stage by stage, each stage from the KERNEL's own output of the stage before (the probe hands out the intermediates p, x, G of
# operator_pair_b), so that no bound has to carry the base solve's conditioning through the stages after it: an end-to-end bound on C
# (k = 288, through |M^-1| and eleven absolute-value stages) allowed a few per cent of |C| at the median and passed a C that was
# subtly wrong.
# k.  One step of a packed column recursion adds at most K_STAGE = 16 to the count of the column it is given (np_spatial.OPS holds
# imp_down_pair, imp_up_pair and imp_down_pair_loaded to that k one step at a time; counted on the source: down 14, loaded 15, up 9), the
# records being inputs.
#   T        a unit column down the leg, joints 3..7                                                              5 * 16 =  80
#   p        -unit impulse up the leg and the spine (8 steps); the u of every joint on the way carries at most this   8 * 16 = 128
#   x        the base solve from the kernel's p, as np_spatial.chol_judge judges it: |p + L L^T x| <= 26 u |L||L^T||x|
#   G        the kernel's x down the spine (3 loaded steps; the u they add carry up to 128)                 128 + 3 * 16 = 176
#   Lambda   the kernel's G down the leg (5 loaded steps; their u carry up to 4 * 16, the column up to 5 * 16) 80 + 5 * 16 = 160
#   C        sum over l of T[:, l] * mirror(G_partner)[l], G the kernel's (an input here): k(T) + 0 + 1, + 5 additions   =  86
K_STAGE = max(ns.OPS[o].k for o in ("imp_down_pair", "imp_up_pair", "imp_down_pair_loaded"))
K_T, K_P, K_G = 5 * K_STAGE, 8 * K_STAGE, 8 * K_STAGE + 3 * K_STAGE
K_LAM, K_C = 5 * K_STAGE + 5 * K_STAGE, 5 * K_STAGE + 1 + 5
OPS_K = np.array([K_T] * 36 + [K_C] * 36 + [K_LAM] * 36 + [K_P] * 36 + [K_G] * 36, np.float64)
LEG, SPINE = (3, 4, 5, 6, 7), (0, 1, 2)


def mirror_pose(q):
    """joint angles of the y-mirrored robot: sides swapped, rotations about x and z negated"""
    q = np.asarray(q, np.float64)
    o = q.copy()
    for r_, l_ in zip(M.MIRROR_RIGHT_JOINTS, M.MIRROR_LEFT_JOINTS):
        o[..., r_], o[..., l_] = q[..., l_], q[..., r_]
    for j in range(M.NJ):
        if M.AXIS[j] != 1:
            o[..., j] = -o[..., j]
    return o


def dadd(m, h=nd.H_SUB):
    """PHYSICS.md 3.1's implicit diagonal for angles inside their ranges"""
    return m["armature"] + h * m["damping"] + h * h * m["stiffness"]


def aba_records(m, q):
    """fp64 articulated-body inertia pass over the whole tree, batched over poses q [n,21] -> records of joints 0..7 [n,8,10] (cs, sn,
    Uw 3, Uv 3, Dinv, u = 0) and the base factor [n,21] (l15 row-major strictly lower, di6 = 1 / L_ii)"""
    n = q.shape[0]
    da = dadd(m)
    IA = [np.broadcast_to(nd.spatial_inertia(m, b), (n, 6, 6)).copy() for b in range(M.NB)]
    rec = np.zeros((n, 8, 10))
    for j in reversed(range(M.NJ)):
        ax = M.AXIS[j]
        c, s = np.cos(q[:, j]), np.sin(q[:, j])
        X, _ = xform_b(ax, c, s, m["r"][j])
        Uc = IA[j + 1][:, :, ax]
        D = Uc[:, ax] + da[j]
        Ia = IA[j + 1] - Uc[:, :, None] * Uc[:, None, :] / D[:, None, None]
        IA[M.PARENT[j]] += np.swapaxes(X, 1, 2) @ Ia @ X
        if j < 8:
            rec[:, j, 0], rec[:, j, 1], rec[:, j, 2:8], rec[:, j, 8] = c, s, Uc, 1.0 / D
    L = np.linalg.cholesky(IA[0])
    fac = np.zeros((n, 21))
    for i in range(6):
        fac[:, 15 + i] = 1.0 / L[:, i, i]
        for j2 in range(i):
            fac[:, i * (i - 1) // 2 + j2] = L[:, i, j2]
    return rec, fac


def _down(m, j, rec, d, Bd, ul=None, Bul=None):
    """imp_down_pair(_loaded) on all columns at once: d, Bd [n,6(component),ncol]"""
    ax = M.AXIS[j]
    X, aX = xform_b(ax, rec[:, j, 0], rec[:, j, 1], m["r"][j])
    Uv, Di = rec[:, j, 2:8], rec[:, j, 8]
    d, Bd = X @ d, aX @ Bd
    dot, Bdot = np.einsum("nk,nkc->nc", Uv, d), np.einsum("nk,nkc->nc", np.abs(Uv), Bd)
    dq, Bdq = -Di[:, None] * dot, np.abs(Di)[:, None] * Bdot
    if ul is not None:
        dq, Bdq = dq + Di[:, None] * ul, Bdq + np.abs(Di)[:, None] * Bul
    d, Bd = d.copy(), Bd.copy()
    d[:, ax] += dq
    Bd[:, ax] += Bdq
    return d, Bd


def _up(m, j, rec, p, Bp):
    """imp_up_pair on all columns: returns the parent's impulse, its bound, and the joint's u, |u| bound"""
    ax = M.AXIS[j]
    X, aX = xform_b(ax, rec[:, j, 0], rec[:, j, 1], m["r"][j])
    Uv, Di = rec[:, j, 2:8], rec[:, j, 8]
    u, Bu = -p[:, ax], Bp[:, ax]
    du, Bdu = Di[:, None] * u, np.abs(Di)[:, None] * Bu
    pa, Bpa = p + Uv[:, :, None] * du[:, None, :], Bp + np.abs(Uv)[:, :, None] * Bdu[:, None, :]
    return np.swapaxes(X, 1, 2) @ pa, np.swapaxes(aX, 1, 2) @ Bpa, u, Bu


def factor_dense(fac):
    n = fac.shape[0]
    L = np.zeros((n, 6, 6))
    for i in range(6):
        L[:, i, i] = 1.0 / fac[:, 15 + i]
        for j in range(i):
            L[:, i, j] = fac[:, i * (i - 1) // 2 + j]
    return L


def ops_lane(m, rec, fac):
    """The operators of one lane from its records, in fp64: T, G (own-foot impulse -> pelvis twist, before the exchange), Lambda_own and
    their bounds, each [n,6(component),6(column)].  The same recursion as the kernels', every column at once.
    Used in fp64 only (ops_anchor ties it to J H^-1 J^T); ops_judge runs the same steps (_up, _down) from the kernel's intermediates."""
    n = rec.shape[0]
    eye = np.broadcast_to(np.eye(6), (n, 6, 6))
    T, BT = eye.copy(), eye.copy()
    for j in LEG:
        T, BT = _down(m, j, rec, T, BT)
    p, Bp = -eye, eye.copy()
    ul, Bul = {}, {}
    for j in reversed(LEG):
        p, Bp, ul[j], Bul[j] = _up(m, j, rec, p, Bp)
    for j in reversed(SPINE):
        p, Bp, ul[j], Bul[j] = _up(m, j, rec, p, Bp)
    L = factor_dense(fac)
    Mx = L @ np.swapaxes(L, 1, 2)
    aM = np.abs(L) @ np.abs(np.swapaxes(L, 1, 2))
    Mi = np.linalg.inv(Mx)
    d = -Mi @ p
    Bd = np.abs(Mi) @ (aM @ np.abs(d) + Bp)          # (not used for a judgement)
    for j in SPINE:
        d, Bd = _down(m, j, rec, d, Bd, ul[j], Bul[j])
    G, BG = d, Bd
    for j in LEG:
        d, Bd = _down(m, j, rec, d, Bd, ul[j], Bul[j])
    return T, BT, G, BG, d, Bd


def ops_judge(kind, inp, got, partner):
    """probe rows and outputs [n,216] -> ({k: worst ratio}, with the solve's residual ratio under "solve", failures); partner[e] is the
    case whose G lane e receives (itself on the host, e ^ 1 on the device)"""
    m = model(kind)
    x = inp.astype(np.float64)
    g = np.asarray(got, np.float64)
    n = x.shape[0]
    rec, fac = x[:, :80].reshape(n, 8, 10), x[:, 80:101]

    def mat(a):
        return np.swapaxes(a.reshape(n, 6, 6), 1, 2)      # column-major row -> [n, component, column]

    def cols(A):
        return np.swapaxes(A, 1, 2).reshape(n, 36)
    pg, xg, Gg = mat(g[:, 108:144]), mat(g[:, 144:180]), mat(g[:, 180:216])
    eye = np.broadcast_to(np.eye(6), (n, 6, 6))
    T, BT = eye.copy(), eye.copy()
    for j in LEG:
        T, BT = _down(m, j, rec, T, BT)
    p, Bp = -eye, eye.copy()
    ul, Bul = {}, {}
    for j in list(reversed(LEG)) + list(reversed(SPINE)):
        p, Bp, ul[j], Bul[j] = _up(m, j, rec, p, Bp)
    L = factor_dense(fac)
    Mx, aM = L @ np.swapaxes(L, 1, 2), np.abs(L) @ np.abs(np.swapaxes(L, 1, 2))
    res, den = np.abs(pg + Mx @ xg), U * (aM @ np.abs(xg))
    with np.errstate(divide="ignore", invalid="ignore"):
        rs = np.where(den > 0, res / np.where(den > 0, den, 1.0), np.where(res == 0, 0.0, np.inf))
    G, BG = xg, np.abs(xg)
    for j in SPINE:
        G, BG = _down(m, j, rec, G, BG, ul[j], Bul[j])
    Lam, BLam = Gg, np.abs(Gg)
    for j in LEG:
        Lam, BLam = _down(m, j, rec, Lam, BLam, ul[j], Bul[j])
    go = MIRROR[None, :, None] * Gg[partner]
    C, BC = T @ go, BT @ np.abs(go)
    ref = np.concatenate([cols(T), cols(C), cols(Lam), cols(p), cols(G)], 1)
    B = np.concatenate([cols(BT), cols(BC), cols(BLam), cols(Bp), cols(BG)], 1)
    gsel = np.concatenate([got[:, :144], got[:, 180:216]], 1)
    worst, fails = judge_cols(gsel, ref, B, np.zeros(ref.shape, bool), OPS_K)
    worst = {"T": worst[K_T], "C": worst[K_C], "Lambda": worst[K_LAM], "p": worst[K_P], "G": worst[K_G], "solve": float(rs.max())}
    bad = ~(rs <= ns.CHOL_K_SOLVE) | ~np.isfinite(xg)
    fails += [(int(e), "solve column %d" % c, float(rs[e, r, c]), 0.0, float(rs[e, r, c])) for e, r, c in zip(*np.nonzero(bad))]
    return worst, fails


def ops_poses(kind):
    """[n_pairs,21] full poses, joints inside their ranges: random, then q0, both ends of every spine and leg joint's range (of the right
    side, the left leg random: asymmetric), the straightest knee"""
    rng, m = _rng("contact_ops", kind), model(kind)
    lo, hi = m["range"][:, 0], m["range"][:, 1]
    qs = [rng.uniform(lo, hi) for _ in range(N_RANDOM // 2)]
    edges = {"q0": len(qs)}
    qs.append(m["q0"].copy())
    edges["range ends"] = len(qs)
    for j in range(8):
        for end in (lo, hi):
            q = rng.uniform(lo, hi)
            q[j] = end[j]
            qs.append(q)
    edges["straight knee"] = len(qs)
    q = m["q0"].copy()
    q[6] = lo[6]
    q[11] = lo[11]
    qs.append(q)
    return np.array(qs), edges


def ops_rows(kind, q):
    """lane rows of every pose: even rows the right half, odd rows the left half in its mirrored world -> [2 n_pairs, 101]"""
    m = model(kind)
    recr, facr = aba_records(m, q)
    recl, facl = aba_records(m, mirror_pose(q))
    n = q.shape[0]
    rows = np.zeros((2 * n, 101))
    rows[0::2] = np.concatenate([recr.reshape(n, 80), facr], 1)
    rows[1::2] = np.concatenate([recl.reshape(n, 80), facl], 1)
    return rows


@functools.lru_cache(maxsize=None)
def ops_prepared(kind):
    q, edges = ops_poses(kind)
    rows = ops_rows(kind, q)
    if rows.shape[0] % 64 == 0:
        rows = np.concatenate([rows, rows[:2]])
    inp = rows.astype(np.float32)
    assert inp.shape[0] % 2 == 0 and inp.shape[0] % 64 != 0
    return _frozen(dict(inp=inp, poses=q, edges=edges))


def ops_anchor(kind, q):
    """fp64, unrounded records of ONE pose q [21] against the dense construction -> relative differences (T, Lambda_own, C) of the right
    lane: T against the product of the leg's joint transforms with the joint freedom projected out, Lambda_own and C against the blocks
    of np_contact.substep's J H^-1 J^T"""
    m = model(kind)
    rows = ops_rows(kind, q[None])
    T, _, G, _, Lam, _ = ops_lane(m, rows[:, :80].reshape(2, 8, 10), rows[:, 80:101])
    C = T[0] @ (MIRROR[:, None] * G[1])
    # dense T: (1 - S Dinv U^T) X per joint, multiplied out
    Td = np.eye(6)
    rec = rows[0, :80].reshape(8, 10)
    for j in LEG:
        S = np.zeros(6)
        S[M.AXIS[j]] = 1.0
        X = nd.xform(M._rot(M.AXIS[j], q[j]).T, m["r"][j])
        Td = (np.eye(6) - np.outer(S, rec[j, 2:8]) * rec[j, 8]) @ X @ Td
    st = np.zeros(185)
    st[3] = 1.0
    st[2] = 1.0
    st[13:34] = q
    st[59] = 1
    st[65:185] = np.tile(np.array([40.0, 40.0, -30.0, 0, 0, 0]), 20)
    Li = nc.substep(m, st, np.zeros(M.NJ))["Li"]
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    return rel(T[0], Td), rel(Lam[0], Li[0:6, 0:6]), rel(C, Li[0:6, 6:12] * MIRROR[None, :])


# ================================================================ sampler
# sample_cell: additions only, in the kernel's order: the reference is the same sequence in np.float32 and the match is exact.
# yaw_sample / pitch_sample: (-20 + 4 i) is exact, * kDeg (a constant, 1): k = 2.
# place_stone: planar = dr * cp (1); p + planar * cph: 1 + 0 + 1 = 2, + : 3.
# stone_normal: three sincosf (K_SINCOS each); x1 = sy * cx: 2 K_SINCOS + 1; cp * x1: 3 K_SINCOS + 2; - : 3 K_SINCOS + 3.
K_ANGLE_SAMPLE, K_PLACE, K_NORMAL = 2, 3, 3 * K_SINCOS + 3
SAMPLER_K = np.array([0, 0] + [K_ANGLE_SAMPLE] * 22 + [K_PLACE] * 3 + [K_NORMAL] * 3, np.float64)
NCELL = 121


def sample_cell_np(p, u):
    """the kernel's rule on float32 [n,121], u [n] float32: sequential cdf; the first cell with u < cdf, else the last cell with p > 0"""
    n = p.shape[0]
    cdf = np.zeros(n, np.float32)
    last = np.zeros(n, np.int64)
    pick = np.full(n, -1, np.int64)
    for k in range(NCELL):
        pk = p[:, k]
        last = np.where(pk > 0, k, last)
        cdf = (cdf + pk).astype(np.float32)
        pick = np.where((pick < 0) & (u < cdf), k, pick)
    return np.where(pick < 0, last, pick)


@functools.lru_cache(maxsize=None)
def sampler_prepared():
    rng = _rng("sampler", "walker3d")
    one_minus = float(F32(1.0) - F32(2.0 ** -24))
    grids, us = [], []
    for i in range(N_RANDOM):
        g = rng.uniform(0, 1, NCELL) ** rng.integers(1, 6)
        g[rng.uniform(size=NCELL) < rng.uniform(0, 0.9)] = 0.0
        if not g.any():
            g[int(rng.integers(NCELL))] = 1.0
        grids.append(g / g.sum())
        us.append(int(rng.integers(0, 2 ** 24)) * 2.0 ** -24)
    edges = {}

    def add(name, g, u):
        edges.setdefault(name, []).append(len(grids))
        grids.append(np.asarray(g, np.float64))
        us.append(u)
    for cell in (0, 60, 120):
        for u in (0.0, 0.5, one_minus):
            add("one-hot %d" % cell, np.eye(NCELL)[cell], u)
    g = np.zeros(NCELL)
    g[7:100] = 1.0 / 93
    for u in (0.0, 0.25, one_minus):
        add("leading and trailing zeros", g, u)
    # uniform grids whose fp32 running sum ends at or below 1 - 2^-24: u = 1 - 2^-24 is never below it and the last cell with p > 0 is returned
    for cnt in range(2, 118):
        g = np.zeros(NCELL)
        g[3:3 + cnt] = np.float32(1.0 / cnt)
        tot = np.float32(0)
        for v in g.astype(np.float32):
            tot = np.float32(tot + v)
        if float(tot) <= one_minus:
            add("fp32 sum below 1", g, one_minus)
    assert len(edges["fp32 sum below 1"]) >= 1
    add("u = 0", np.full(NCELL, 1.0 / NCELL), 0.0)
    n = len(grids)
    x = np.zeros((n, 133))
    x[:, :NCELL], x[:, NCELL] = np.array(grids), np.array(us)
    x[:, 122:125] = rng.uniform(-20, 20, (n, 3))                       # px, py, pz
    x[:, 125] = rng.uniform(0.65, 1.25, n)                             # dr
    pitch, phi = rng.uniform(-0.6, 0.6, n), rng.uniform(-8, 8, n)
    x[:, 126], x[:, 127], x[:, 128], x[:, 129] = np.cos(pitch), np.sin(pitch), np.cos(phi), np.sin(phi)
    x[:, 130], x[:, 131], x[:, 132] = rng.uniform(-8, 8, n), rng.uniform(-TILT, TILT, n), rng.uniform(-TILT, TILT, n)
    x[-1, 130:133] = [0.0, TILT, -TILT]
    inp = _pad(list(x), x[0])
    y = inp.astype(np.float64)
    n = y.shape[0]
    ref, B = np.zeros((n, 30)), np.zeros((n, 30))
    cell = sample_cell_np(inp[:, :NCELL], inp[:, NCELL])
    ref[:, 0] = ref[:, 1] = cell
    i = np.arange(11)
    ref[:, 2:13], ref[:, 13:24] = np.radians(-20.0 + 4.0 * i), np.radians(-30.0 + 6.0 * i)
    B[:, 2:24] = np.abs(ref[:, 2:24])
    px, dr, cp, sp, cph, sph = y[:, 122:125], y[:, 125], y[:, 126], y[:, 127], y[:, 128], y[:, 129]
    ref[:, 24:27] = px + np.stack([dr * cp * cph, dr * cp * sph, dr * sp], 1)
    B[:, 24:27] = np.abs(px) + np.abs(np.stack([dr * cp * cph, dr * cp * sph, dr * sp], 1))
    ph, xt, yt = y[:, 130], y[:, 131], y[:, 132]
    ref[:, 27:30] = stone_normal_b(ph, xt, yt)
    ac, as_ = np.abs(np.cos(ph)), np.abs(np.sin(ph))
    x1, y1 = np.abs(np.sin(yt) * np.cos(xt)), np.abs(np.sin(xt))
    B[:, 27:30] = np.stack([ac * x1 + as_ * y1, as_ * x1 + ac * y1, np.abs(np.cos(yt) * np.cos(xt))], 1)
    exact = np.zeros((n, 30), bool)
    exact[:, :2] = True
    return _frozen(dict(inp=inp, ref=ref, B=B, exact=exact, cell=cell, edges=edges))


def window_prob_np(level, ring):
    """fp64 construction of PHYSICS.md 8's sampling grid: uniform over the cells within (ring: exactly at) Chebyshev distance level"""
    i, j = np.meshgrid(np.arange(11), np.arange(11), indexing="ij")
    mdist = np.maximum(np.abs(i - 5), np.abs(j - 5))
    inside = (mdist == level) if ring else (mdist <= level)
    return (inside / inside.sum()).reshape(NCELL)


# ================================================================ observation terms
# k (the quaternion, positions, angles and rates are inputs):
#   roll = atan2(Y, X): Y = 2 (w x + y z) k 2; X = 1 - 2 (x x + y y) k 3; + K_ATAN2                          3 + 12 = 15
#   pitch = asin(clamp(S)): S = 2 (w y - z x) k 2; + K_ASIN                                                    2 +  8 = 10
#   cy = A * inv: A k 3, B k 2; n2 = A A + B B: (3 + 3 + 1) + 1 = 8; inv = rsqrt: 8 + 2 = 10; A * inv: 3 + 10 + 1     14
#   target_features: (sp - pos) k 1; dy cy - dx sy: 1 + 0 + 1, - : 3;  dz: 1;  tilts: copies (exact)
#   planar_dist: dx k 1; dx dx: 3; + : 4; sqrtf: 4 + K_SQRT                                                             10
#   obs_angle: mid, span are constants (1); ps * q - ps * mid: 2; / span: 2 + 1 + 1 = 4; * 2 exact; clip5 never widens   4
#   obs_rate: 0.1f (1) * (ps * qd) : 2
#   reset_angle: 2 u01 - 1 exact; * 0.05f: 2; q0 (1) + : 3; the clamp bounds lo + 0.02f, hi - 0.02f: 1, 1, + : 2 (< 3)    3
K_ROLL, K_PITCH_S, K_PITCH, K_YAW, K_TF, K_PD, K_OA, K_OR, K_RA = 3 + K_ATAN2, 2, 2 + K_ASIN, 14, 3, 4 + K_SQRT, 4, 2, 3
OBS_K = np.array([K_ROLL, K_PITCH, K_YAW, K_YAW, K_TF, K_TF, 1, 0, 0, K_PD, 0] + [K_OA] * 21 + [K_OR] * 21 + [K_RA] * 42, np.float64)


def obs_ref(kind, inp):
    m = model(kind)
    with np.errstate(invalid="ignore"):          # the Philox words are NaN patterns as floats; they are read as bits below
        x = inp.astype(np.float64)
    n = x.shape[0]
    ref, B = np.zeros((n, 95)), np.zeros((n, 95))
    exact = np.zeros((n, 95), bool)
    w, qx, qy, qz = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
    inf = np.inf
    # roll: the error box of (X, Y) must stay clear of the origin, else the angle is undetermined (B = inf: not judged)
    Y, BY = 2 * (w * qx + qy * qz), 2 * (np.abs(w * qx) + np.abs(qy * qz))
    X, BX = 1 - 2 * (qx * qx + qy * qy), 1 + 2 * (qx * qx + qy * qy)
    dX, dY = 3 * U * BX, 2 * U * BY
    r2 = np.maximum(np.abs(X) - dX, 0) ** 2 + np.maximum(np.abs(Y) - dY, 0) ** 2
    ref[:, 0] = np.arctan2(Y, X)
    with np.errstate(divide="ignore", invalid="ignore"):
        B[:, 0] = np.where(r2 > 0, ((np.abs(X) + dX) * BY + (np.abs(Y) + dY) * BX) / r2 + np.abs(ref[:, 0]), inf)
    # pitch: asin is monotonic, so the effect of S's error is read at the ends of its interval (the derivative is unbounded at +-1)
    S, BS = 2 * (w * qy - qz * qx), 2 * (np.abs(w * qy) + np.abs(qz * qx))
    asn = lambda v: np.arcsin(np.clip(v, -1.0, 1.0))
    dS = K_PITCH_S * U * BS
    ref[:, 1] = asn(S)
    spread = np.maximum(np.abs(asn(S + dS) - ref[:, 1]), np.abs(asn(S - dS) - ref[:, 1]))
    B[:, 1] = np.maximum(spread / (K_PITCH_S * U), np.abs(ref[:, 1]))
    # cos / sin of the yaw
    A, BA = 1 - 2 * (qy * qy + qz * qz), 1 + 2 * (qy * qy + qz * qz)
    Bq, BB = 2 * (w * qz + qx * qy), 2 * (np.abs(w * qz) + np.abs(qx * qy))
    n2, Bn2 = A * A + Bq * Bq, BA * BA + BB * BB
    deg = n2 == 0                                        # A = B = 0: yaw (1, 0), exactly
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(deg, 1.0, 1.0 / np.sqrt(n2))
        Binv = np.where(deg, 1.0, inv * np.maximum(0.5 * Bn2 / n2, 1.0))
    undecided = ~deg & (n2 - 1e-30 <= 8 * U * Bn2)       # n2 > 1e-30 not decided by the reference
    ref[:, 2], ref[:, 3] = np.where(deg, 1.0, A * inv), np.where(deg, 0.0, Bq * inv)
    B[:, 2], B[:, 3] = np.where(undecided, inf, BA * Binv), np.where(undecided, inf, BB * Binv)
    exact[:, 2] = exact[:, 3] = deg
    # target_features from the given (cy, sy)
    cy, sy, pos, sp, tilt = x[:, 4], x[:, 5], x[:, 6:9], x[:, 9:12], x[:, 12:14]
    dlt, Bdl = sp - pos, np.abs(sp) + np.abs(pos)
    ref[:, 4], B[:, 4] = dlt[:, 1] * cy - dlt[:, 0] * sy, Bdl[:, 1] * np.abs(cy) + Bdl[:, 0] * np.abs(sy)
    ref[:, 5], B[:, 5] = dlt[:, 0] * cy + dlt[:, 1] * sy, Bdl[:, 0] * np.abs(cy) + Bdl[:, 1] * np.abs(sy)
    ref[:, 6], B[:, 6] = dlt[:, 2], Bdl[:, 2]
    ref[:, 7:9], B[:, 7:9] = tilt, np.abs(tilt)
    exact[:, 7:9] = True
    # planar_dist
    s2, Bs2 = (dlt[:, :2] ** 2).sum(1), (Bdl[:, :2] ** 2).sum(1)
    ref[:, 9] = np.sqrt(s2)
    with np.errstate(divide="ignore", invalid="ignore"):
        B[:, 9] = np.where(s2 > 0, np.maximum(0.5 * Bs2 / np.sqrt(s2), np.sqrt(s2)), np.where(Bs2 > 0, inf, 0.0))
    ref[:, 10] = np.clip(x[:, 14], -5, 5)
    B[:, 10] = np.abs(ref[:, 10])
    exact[:, 10] = True
    # joint entries, from model.py's signs and the rounded ranges
    lo, hi = m["range"][:, 0], m["range"][:, 1]
    ps = np.array(M.POLICY_SIGN, np.float64)
    mid, span = 0.5 * (lo + hi), hi - lo
    q, qd = x[:, 15:36], x[:, 36:57]
    ref[:, 11:32] = np.clip(2 * (ps * q - ps * mid) / span, -5, 5)
    B[:, 11:32] = 2 * (np.abs(q) + np.abs(mid)) / span
    ref[:, 32:53] = np.clip(0.1 * ps * qd, -5, 5)
    B[:, 32:53] = 0.1 * np.abs(qd)
    # reset noise: global joint j reads word j of the 24
    words = inp[:, 57:81].copy().view(np.uint32)[:, :21]
    u = (words >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    ref[:, 53:74], B[:, 53:74], clamped = _reset_ref(u, m["q0"], lo, hi)
    # the same function over the probe's ClampModel, whose draws reach both clamps
    ref[:, 74:95], B[:, 74:95], clamped_cm = _reset_ref(u, CLAMP_Q0, CLAMP_LO, CLAMP_HI)
    return ref, B, exact, clamped, clamped_cm


# tests/device/ss_probe.hip's ClampModel (the fp32 values of its literals): q0 0.03 inside lo (even joints) or hi (odd joints)
CLAMP_LO = f32([-1.0, -0.5, -0.25, 0.1, -2.0, -0.3, 0.7, -1.5, -0.6, 0.2, -0.9, -1.1, -0.4, 0.3, -2.5, -0.7, 0.5, -1.3, -0.8, 0.4, -0.2]).astype(np.float64)
CLAMP_HI = f32([1.0, 0.75, 0.5, 1.1, -0.5, 0.3, 2.9, 0.6, 0.6, 1.2, 0.9, 1.3, 0.4, 2.3, -1.5, 0.7, 1.5, -0.3, 0.8, 0.9, 0.2]).astype(np.float64)
CLAMP_Q0 = f32([-0.97, 0.72, -0.22, 1.07, -1.97, 0.27, 0.73, 0.57, -0.57, 1.17, -0.87, 1.27, -0.37, 2.27, -2.47, 0.67, 0.53, -0.33, -0.77, 0.87,
                -0.17]).astype(np.float64)


def _reset_ref(u, q0, lo, hi):
    """reset_angle from the draws u [n,21] -> (ref, B, clamped): min(max(q0 + 0.05 (2 u - 1), lo + 0.02), hi - 0.02).  B is the draw's
    bound inside the clamps by more than the tolerance, the clamp bound's own (|lo| + 0.02) beyond them, the larger of the two between"""
    raw, Braw = q0 + 0.05 * (2 * u - 1), np.abs(q0) + 0.05 * np.abs(2 * u - 1)
    lo2, hi2 = lo + 0.02, hi - 0.02
    Blo, Bhi = np.abs(lo) + 0.02, np.abs(hi) + 0.02
    tol = K_RA * U * (Braw + Blo + Bhi)
    B = np.where(raw < lo2 - tol, Blo, np.where(raw > hi2 + tol, Bhi, np.where((raw > lo2 + tol) & (raw < hi2 - tol), Braw,
                                                                               np.maximum(Braw, np.maximum(Blo, Bhi)))))
    return np.clip(raw, lo2, hi2), B + np.zeros_like(raw), (raw < lo2) | (raw > hi2)


def _word(u24):
    """a Philox word whose u01 is u24 * 2^-24"""
    return np.uint32(int(u24) << 8)


@functools.lru_cache(maxsize=None)
def obs_prepared(kind):
    rng, m = _rng("obs_terms", kind), model(kind)
    lo, hi = m["range"][:, 0], m["range"][:, 1]
    n_edge = 16
    n = N_RANDOM + n_edge
    x = np.zeros((n, 81), np.float32)
    qt = rng.normal(size=(n, 4))
    qt /= np.linalg.norm(qt, axis=1)[:, None]
    yaw = rng.uniform(-np.pi, np.pi, n)
    x[:, 0:4] = qt
    x[:, 4], x[:, 5] = np.cos(yaw), np.sin(yaw)
    x[:, 6:9] = rng.uniform(-30, 30, (n, 3))
    x[:, 9:12] = x[:, 6:9] + rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    x[:, 12:14] = rng.uniform(-TILT, TILT, (n, 2))
    x[:, 14] = rng.uniform(-8, 8, n)
    # angles past the range by up to 2.5 spans (the clip at +-5 starts 2 spans past it), rates up to 80 rad/s (clip at 50)
    x[:, 15:36] = rng.uniform(lo - 2.5 * (hi - lo), hi + 2.5 * (hi - lo), (n, 21))
    x[:, 36:57] = rng.uniform(-80, 80, (n, 21))
    words = rng.integers(0, 2 ** 32, (n, 24), dtype=np.uint64).astype(np.uint32)
    e0 = N_RANDOM
    h = np.sqrt(0.5)
    edges = {"pitch +90": e0, "pitch -90": e0 + 1, "A = B = 0": e0 + 2, "norm 1 + 1e-3": e0 + 3, "norm 1 - 1e-3": e0 + 4,
             "clip": e0 + 5, "reset extremes": (e0 + 6, e0 + 7), "pitch clamp": (e0 + 8, e0 + 9)}
    x[e0, 0:4] = [h, 0, h, 0]
    x[e0 + 1, 0:4] = [h, 0, -h, 0]
    x[e0 + 2, 0:4] = [0.5, -0.5, 0.5, 0.5]
    x[e0 + 3, 0:4] = x[0, 0:4] * np.float32(1.001)
    x[e0 + 4, 0:4] = x[1, 0:4] * np.float32(0.999)
    x[e0 + 8, 0:4] = np.array([h, 0, h, 0], np.float32) * np.float32(1.001)          # 2 (w y - z x) = 1.002: only the clamp keeps asin defined
    x[e0 + 9, 0:4] = np.array([h, 0, -h, 0], np.float32) * np.float32(1.001)
    x[e0 + 5, 14] = 5.0
    x[e0 + 5, 15:36] = hi + 3.0 * (hi - lo)
    x[e0 + 5, 36:57] = np.where(np.arange(21) % 2 == 0, 50.0, -70.0)
    words[e0 + 6] = _word(0)                         # u = 0: q0 - 0.05
    words[e0 + 7] = _word(2 ** 24 - 1)               # u = 1 - 2^-24: q0 + 0.05 (1 - 2^-23)
    x[:, 57:81] = words.view(np.float32)
    if x.shape[0] % 64 == 0:
        x = np.concatenate([x, x[:1]])
    ref, B, exact, clamped, clamped_cm = obs_ref(kind, x)
    for e in edges["pitch clamp"]:
        assert abs(2 * (float(x[e, 0]) * float(x[e, 2]) - float(x[e, 3]) * float(x[e, 1]))) > 1.0
    return _frozen(dict(inp=x, ref=ref, B=B, exact=exact, clamped=clamped, clamped_cm=clamped_cm, edges=edges))
