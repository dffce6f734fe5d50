"""Cases, fp64 reference and judgement for ONE substep of the step kernels (ss_dynamics.hpp: substep<Model, 0>), as the `substep` op of
tests/device/ss_probe.hip runs it on the two lanes of a robot.  Used by tests/test_substep.py.  Nothing here is a fixture: the cases are
drawn at test time from the CPU oracle (deterministic), the reference is np_contact / np_dynamics on model.build(kind) rounded to fp32.

A case is one row of the probe (IW words, the robot in the TRUE world); the probe's answer is two lane rows of OWL raw LDS words, lane 1
in its y-mirrored world.  Every judgement has the form |got - ref| <= K * 2^-24 * B, B the reference's running absolute-value bound.

The constants K_A, K_C, K_D cannot be counted on the source (an articulated-body pass has no componentwise bound; five clamped sweeps
amplify).  They are 4 x the worst ratio of the fp32 ORACLE (oracle/ss_oracle.c, OracleEnv(prec="f32").debug_contact) on these cases, judged
by these formulas against this reference, rounded up to a power of two -- never taken from the kernels.  Measured (oracle_measure, both
robots; docs/HISTORY.md has the table):
    stage A residual    walker3d 1.13,  mike 1.17   -> 4 x 1.17  = 4.7    -> K_A = 8
    stage C impulses    walker3d 13780, mike 1337   -> 4 x 13780 = 55120  -> K_C = 65536
    stage D response    walker3d 3.90,  mike 2.66   -> 4 x 3.90  = 15.6   -> K_D = 16
(C: one random-action case of walker3d, a light foot pivoting on two corners, carries the 13780; the next is below 800.  The oracle's
debug_aba is the same pass that debug_contact taps as qdf / v0f, so A is measured on the tap.)
tests/test_substep.py::test_oracle_yardstick re-measures and fails above K / 2."""
import functools

import numpy as np

import np_contact as nc
import np_contact_ops as no
import np_dynamics as nd
import np_spatial as ns
import oracle_lib as ol
from steppingstone_amd import model as M

U = ns.U
KINDS = no.KINDS
F32 = np.float32
H32 = float(F32(1.0) / F32(240.0))          # kH
G32 = float(F32(9.8))                        # kGrav
MAX_CASES = 256

K_A, K_C, K_D = 8, 65536, 16                  # measured on the fp32 oracle: see the module docstring
# counted on substep()'s integrator (ss_dynamics.hpp, "integrate"); the kernel's own new qd / twist are inputs, h and 0.5 h constants:
#   q' = q + h qd':  the reference takes h as the kernel's fp32 value, so it carries no rounding here: the product 1, the sum 2
K_Q = 2
#   pos += h (Rb[r] . v):  Rb = quat_rot(quat): 1 - 2 (yy + zz): products 1, sum 2, 1 - : 3; Rb v: 3 + 0 + 1 = 4, two additions: 6;
#   h * : 6 + 1 + 1 = 8; pos + : 9
K_POS = 9
#   quaternion: q o products 1, three-term sum 3, hh * : 3 + 1 + 1 = 5, q + : 6 (n); n n: 6 + 6 + 1 = 13, four-term sum: 16;
#   SS_RSQRT: 16 + 2 = 18; n * inv: 6 + 18 + 1 = 25
K_QUAT = 25
# detection: np_contact_ops counts fk_detect with cos / sin / Rb as INPUTS (K_D = 33, K_UV = 37, K_SOLE = 33).  Here they come from ss_sincos
# (4 roundings, absolute) and quat_rot (3): a joint level costs k(R_p) + 4 + 1, + 1 = 6 instead of 2: Rf 3 + 8 * 6 = 51, pf 50, P 56,
# d 60, u / v 64, sole 60 -- all within twice the counts there, so its tolerances are doubled.
DETECT_SCALE = 2.0
K_SOLE = 2 * no.K_SOLE

# ---------------------------------------------------------------- layout of the probe's rows
I_POS, I_QUAT, I_W, I_V, I_Q, I_QD, I_ACT, I_POWER, I_STONES, I_WARM, I_CALLS, IW = 0, 3, 7, 10, 13, 34, 55, 76, 77, 101, 127, 128
O_Q, O_QD, O_POS, O_QUAT, O_W, O_V, O_KEY, O_LAM, O_CONTACT, O_TARGET, O_SOLE, OWL = 0, 12, 24, 27, 31, 34, 37, 38, 50, 51, 52, 55
KHALF = [0, 1, 2, 3, 4, 5, 6, 7, 13, 14, 15, 16]


def left_twin(j):
    return j if j < 3 else (j + 5 if j < 8 else j + 4)


LANE_JOINT = np.array([KHALF, [left_twin(j) for j in KHALF]])
LANE_SIGN = np.array([[1.0] * 12, [-1.0 if M.AXIS[j] != 1 else 1.0 for j in KHALF]])
POLICY = np.array(M.POLICY_SIGN, np.float64)
SPINE, LEG, ARM = (0, 1, 2), tuple(range(3, 13)), tuple(range(13, 21))
# a lane's world against the true one: pos / linear (+,-,+), quaternion (w, -x, y, -z), angular (-,+,-); the left lane's t2 = n x t1 is minus
# the mirror image of the true t2 (a cross product of two mirrored vectors), so its impulses are (l_n, l_t1, -l_t2) of the true ones
M_POS, M_QUAT, M_ANG, M_LAM = np.array([1.0, -1, 1]), np.array([1.0, -1, 1, -1]), np.array([-1.0, 1, -1]), np.array([1.0, 1, -1])
FAR = np.array([50.0, 50.0, -20.0, 0.0, 0.0, 0.0])


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def stone_words(t):
    """terrain row (x, y, z, phi, x_tilt, y_tilt) -> centre 3, unit normal 3, cos / sin of the heading: what the step kernel keeps"""
    t = f32(t).astype(np.float64)
    return np.concatenate([t[:3], nc.stone_normal(t), [np.cos(t[3]), np.sin(t[3])]])


def make_row(st55, act, power, terr3, warm=None, calls=1):
    row = np.zeros(IW)
    row[:55] = st55
    row[I_ACT:I_ACT + 21] = np.clip(act, -1.0, 1.0)
    row[I_POWER] = power
    row[I_STONES:I_STONES + 24] = np.concatenate([stone_words(t) for t in terr3])
    if warm is not None:
        row[I_WARM:I_WARM + 26] = warm
    row[I_CALLS] = calls
    return f32(row)


def mirror_rows(inp):
    """the rows of the y-mirrored robots (sides swapped) among mirrored stones, with mirrored actions: every change is a swap or a sign"""
    o = np.array(inp, np.float32)
    o[:, I_POS:I_POS + 3] *= F32(M_POS)
    o[:, I_QUAT:I_QUAT + 4] *= F32(M_QUAT)
    o[:, I_W:I_W + 3] *= F32(M_ANG)
    o[:, I_V:I_V + 3] *= F32(M_POS)
    for base in (I_Q, I_QD):
        o[:, base:base + 21] = no.mirror_pose(inp[:, base:base + 21].astype(np.float64)).astype(np.float32)
    a = inp[:, I_ACT:I_ACT + 21].copy()
    for r_, l_ in zip(M.MIRROR_RIGHT_JOINTS, M.MIRROR_LEFT_JOINTS):
        a[:, [r_, l_]] = a[:, [l_, r_]]
    for j in SPINE:
        if M.AXIS[j] != 1:
            a[:, j] = -a[:, j]
    o[:, I_ACT:I_ACT + 21] = a
    for sl in range(3):
        for c in (1, 4, 7):
            o[:, I_STONES + 8 * sl + c] = -o[:, I_STONES + 8 * sl + c]
    o[:, I_WARM:I_WARM + 13], o[:, I_WARM + 13:I_WARM + 26] = inp[:, I_WARM + 13:I_WARM + 26], inp[:, I_WARM:I_WARM + 13]
    return o


def moved_down(inp, dz=10.0):
    o = np.array(inp, np.float32)
    for sl in range(3):
        o[:, I_STONES + 8 * sl + 2] -= F32(dz)
    return o


def assemble(out):
    """probe output [n, 2 OWL] -> the robot in the true world: q, qd [n,21], pos, quat, v0 (w, v) of lane 0; per lane raw key, lam, report"""
    o = np.asarray(out, np.float64).reshape(-1, 2, OWL)
    n = o.shape[0]
    q, qd = np.zeros((n, 21)), np.zeros((n, 21))
    for side in (1, 0):          # the spine from lane 0
        q[:, LANE_JOINT[side]] = o[:, side, O_Q:O_Q + 12] * LANE_SIGN[side]
        qd[:, LANE_JOINT[side]] = o[:, side, O_QD:O_QD + 12] * LANE_SIGN[side]
    return dict(q=q, qd=qd, pos=o[:, 0, O_POS:O_POS + 3], quat=o[:, 0, O_QUAT:O_QUAT + 4], v0=o[:, 0, O_W:O_W + 6],
                key=o[:, :, O_KEY].astype(np.int64), lam=o[:, :, O_LAM:O_LAM + 12].reshape(n, 2, 4, 3),
                contact=o[:, :, O_CONTACT].astype(np.int64), on_target=o[:, :, O_TARGET].astype(np.int64), sole=o[:, :, O_SOLE:O_SOLE + 3],
                lanes=o)


def state55(a):
    """assembled output -> [n,55] packed (pos, quat, v0, q, qd), float64 values of the fp32 words"""
    return np.concatenate([a["pos"], a["quat"], a["v0"], a["q"], a["qd"]], 1)


def feedback_rows(inp, out, calls=1):
    """the second substep of the same control step: the first call's state and Warm, word for word (signs and swaps only)"""
    a = assemble(out)
    o = np.array(inp, np.float32)
    o[:, :55] = state55(a).astype(np.float32)
    raw = np.asarray(out, np.float32).reshape(-1, 2, OWL)
    o[:, I_WARM:I_WARM + 13] = raw[:, 0, O_KEY:O_KEY + 13]
    o[:, I_WARM + 13:I_WARM + 26] = raw[:, 1, O_KEY:O_KEY + 13]
    o[:, I_CALLS] = calls
    return o


# ---------------------------------------------------------------- detection (fp64, per lane, np_contact_ops.detect_ref)
def _lane_detect_rows(x, side):
    n = x.shape[0]
    q = x[:, I_Q:I_Q + 21] if side == 0 else no.mirror_pose(x[:, I_Q:I_Q + 21])
    quat = x[:, I_QUAT:I_QUAT + 4] * (M_QUAT if side else 1.0)
    pos = x[:, I_POS:I_POS + 3] * (M_POS if side else 1.0)
    st = x[:, I_STONES:I_STONES + 24].reshape(n, 3, 8).copy()
    if side:
        st[:, :, [1, 4, 7]] *= -1.0
    Rb = no.quat_rot_b(quat).reshape(n, 9)
    return np.concatenate([np.cos(q[:, :8]), np.sin(q[:, :8]), Rb, pos, st.reshape(n, 24)], 1)


def detect(kind, inp):
    """-> slot [n,2,4] (-1: no contact), pen, safe [n,2,4], sole / its bound [n,2,3] (lane world)"""
    x = np.asarray(inp, np.float64)
    n = x.shape[0]
    slot, pen, safe = np.zeros((n, 2, 4), np.int64), np.zeros((n, 2, 4)), np.zeros((n, 2, 4), bool)
    sole, Bsole = np.zeros((n, 2, 3)), np.zeros((n, 2, 3))
    for side in (0, 1):
        d = no.detect_ref(kind, _lane_detect_rows(x, side))
        # np_contact_ops.detect_ref's rule with the doubled tolerances: a stone's touch is decided when every predicate holds by more than
        # its tolerance or one fails by more; a corner when all three stones are
        mg, tl = d["margins"], DETECT_SCALE * d["tols"]
        ok = ((mg > tl).all(3) | (mg < -tl).any(3)).all(2)
        slot[:, side], pen[:, side], safe[:, side] = d["slot"], d["ref"][:, 9:13], ok
        sole[:, side], Bsole[:, side] = d["ref"][:, 17:20], d["B"][:, 17:20]
    return dict(slot=slot, pen=pen, safe=safe, sole=sole, Bsole=Bsole)


# ---------------------------------------------------------------- the reference of one case
@functools.lru_cache(maxsize=None)
def model(kind):
    return nc.rounded_model(kind)


def rnea_abs(m, q, v0, qd):
    """np_dynamics.rnea(m, q, v0, qd, 0, 0) with every factor's absolute value: the running bound of the bias forces"""
    v, a, f, aX = [None] * M.NB, [None] * M.NB, [None] * M.NB, [None] * M.NB
    aI = [np.abs(nd.spatial_inertia(m, b)) for b in range(M.NB)]
    v[0], a[0] = np.abs(v0), np.zeros(6)
    f[0] = np.abs(nd.crf(v[0])) @ aI[0] @ v[0]
    for j in range(M.NJ):
        b, p = j + 1, M.PARENT[j]
        aX[b] = np.abs(nd.xform(M._rot(M.AXIS[j], q[j]).T, m["r"][j]))
        vj = np.zeros(6)
        vj[M.AXIS[j]] = abs(qd[j])
        v[b] = aX[b] @ v[p] + vj
        a[b] = aX[b] @ a[p] + np.abs(nd.crm(v[b])) @ vj
        f[b] = aI[b] @ a[b] + np.abs(nd.crf(v[b])) @ aI[b] @ v[b]
    tau = np.zeros(M.NJ)
    for j in reversed(range(M.NJ)):
        b, p = j + 1, M.PARENT[j]
        tau[j] = f[b][M.AXIS[j]]
        f[p] = f[p] + aX[b].T @ f[b]
    return np.concatenate([f[0], tau])


def reference(kind, row, det, e):
    """fp64 substep of one probe row (its fp32 words are the inputs): free dynamics with their bounds, contacts from `det` (detect() of
    the rows, case e), np_contact.pgs from the row's warm words, response, integration"""
    m = model(kind)
    x = np.asarray(row, np.float64)
    pos, quat, v0, q, qd = x[0:3], x[3:7], x[7:13], x[13:34], x[34:55]
    act, power = x[I_ACT:I_ACT + 21], x[I_POWER]
    tau_m = power * m["torque"] * POLICY * act
    lo, hi = m["range"][:, 0], m["range"][:, 1]
    viol = np.where(q > hi, q - hi, np.where(q < lo, q - lo, 0.0))
    kl, dl = np.where(viol != 0, m["k_lim"], 0.0), np.where(viol != 0, m["d_lim"], 0.0)
    qdd, a0, Hm = nd.forward_dynamics(m, quat, v0, q, qd, tau_m, h=H32)
    tau = tau_m - m["damping"] * qd - m["stiffness"] * (q + H32 * qd) - kl * (viol + H32 * qd) - dl * qd
    B_tau = np.abs(tau_m) + m["damping"] * np.abs(qd) + m["stiffness"] * (np.abs(q) + H32 * np.abs(qd)) + \
        kl * (np.abs(viol) + H32 * np.abs(qd)) + dl * np.abs(qd)
    f0, tj = nd.rnea(m, q, v0, qd, np.zeros(6), np.zeros(M.NJ))
    Rb = nd.quat_rot(quat)
    gvec = np.concatenate([np.zeros(3), Rb.T @ np.array([0.0, 0.0, -G32]), np.zeros(M.NJ)])
    r = dict(q=q, qd=qd, v0=v0, pos=pos, quat=quat, Hm=Hm, Cb=np.concatenate([f0, tj]), tau=np.concatenate([np.zeros(6), tau]),
             B_tau=np.concatenate([np.zeros(6), B_tau]), B_c=rnea_abs(m, q, v0, qd), gvec=gvec, viol=viol)
    a0g = a0.copy()
    a0g[3:] += Rb.T @ np.array([0.0, 0.0, -G32 + 9.8])          # forward_dynamics has 9.8 in fp64; the kernel's constant is fp32
    qdf, v0f = qd + H32 * qdd, v0 + H32 * a0g
    r.update(qdf=qdf, v0f=v0f)
    # contacts
    slot, pen = det["slot"][e], det["pen"][e]
    R, p = M.fk(m, q, pos, Rb)
    st = x[I_STONES:I_STONES + 24].reshape(3, 8)
    contacts = []
    for f, b in enumerate(nc.FEET):
        for k in range(4):
            if slot[f, k] < 0:
                contacts.append(None)
                continue
            c = m["corners"][k].copy()
            if f == 1:
                c[1] = -c[1]
            contacts.append(dict(r=c, stone=int(slot[f, k]), n=st[slot[f, k], 3:6], pen=float(pen[f, k]), foot=f, Rf=R[b]))
    active = np.array([c is not None for c in contacts])
    r.update(contacts=contacts, active=active.reshape(2, 4), safe=bool(det["safe"][e].all()), dv=np.zeros(27), lam=np.zeros((8, 3)))
    if active.any():
        Jb = nc.body_jacobians(m, q)
        J = np.vstack([Jb[nc.FEET[0]], Jb[nc.FEET[1]]])
        Hinv = np.linalg.inv(Hm)
        Hinv_Jt = Hinv @ J.T
        Li = J @ Hinv_Jt
        vf = np.concatenate([v0f, qdf])
        Vfree = J @ vf
        key = x[[I_WARM, I_WARM + 13]].astype(np.int64)
        wl = x[I_WARM:I_WARM + 26].reshape(2, 13)[:, 1:].reshape(2, 4, 3)
        lam0 = np.zeros((8, 3))
        for f in (0, 1):
            for k in range(4):
                if (key[f] >> k) & 1:
                    lam0[4 * f + k] = wl[f, k] * (M_LAM if f else 1.0)
        warm_kept = np.array([active[i] and bool(np.abs(lam0[i]).max() > 0) for i in range(8)])
        lam, wrench, Wr, bn = nc.pgs(Li, Vfree, contacts, m["friction"], nc.SWEEPS, lam0)
        # B_lambda: the first update of a row with every factor's absolute value, (|b| + |w| . |V|) / A, the largest over the active rows
        aV = np.abs(J) @ np.abs(vf)
        B_lam = 0.0
        for i, c in enumerate(contacts):
            if c is None:
                continue
            f = c["foot"]
            for d in range(3):
                w = Wr[i][d]
                A = w @ Li[6 * f:6 * f + 6, 6 * f:6 * f + 6] @ w
                B_lam = max(B_lam, ((bn[i] if d == 0 else 0.0) + np.abs(w) @ aV[6 * f:6 * f + 6]) / A + np.abs(lam0[i]).max())
        mu = m["friction"]
        on = lam[active]
        sliding = bool(((on[:, 0] > 0)[:, None] & (np.abs(on[:, 1:]) >= mu * on[:, :1] * (1 - 1e-12))).any())
        r.update(J=J, Hinv=Hinv, Hinv_Jt=Hinv_Jt, Li=Li, Vfree=Vfree, lam0=lam0, lam=lam, Wr=Wr, bn=bn, B_lam=B_lam, sliding=sliding,
                 warm_kept=warm_kept, key_in=key, dv=Hinv_Jt @ wrench.reshape(12))
    return r


def references(kind, inp):
    det = detect(kind, inp)
    return [reference(kind, inp[e], det, e) for e in range(inp.shape[0])], det


def response(r, lam_true):
    """(H^-1 J^T W^T lam, its absolute-value bound) [27] for impulses [8,3] on the reference's contacts"""
    wrench, awrench = np.zeros((2, 6)), np.zeros((2, 6))
    for i, c in enumerate(r["contacts"]):
        if c is not None:
            wrench[c["foot"]] += r["Wr"][i].T @ lam_true[i]
            awrench[c["foot"]] += np.abs(r["Wr"][i]).T @ np.abs(lam_true[i])
    return r["Hinv_Jt"] @ wrench.reshape(12), np.abs(r["Hinv"]) @ (np.abs(r["J"]).T @ awrench.reshape(12))


def lam_true(a, e):
    """a lane pair's impulses in the true world, [8,3]"""
    l = a["lam"][e].copy()
    l[1] = l[1] * M_LAM
    return l.reshape(8, 3)


# ---------------------------------------------------------------- judgement, shared by the kernels' flavours and the oracle
def ratio_A(r, v0f, qdf):
    """stage A: the residual of the equation of motion per component, in units of 2^-24 x its bound"""
    v, vf = np.concatenate([r["v0"], r["qd"]]), np.concatenate([v0f, qdf])
    x = (vf - v) / H32
    aH = np.abs(r["Hm"])
    res = r["Hm"] @ (x - r["gvec"]) + r["Cb"] - r["tau"]
    B = aH @ np.abs(x) + aH @ np.abs(r["gvec"]) + aH @ ((np.abs(v) + np.abs(vf)) / H32) + r["B_c"] + r["B_tau"]
    return np.abs(res) / (U * B)


def ratio_C(r, lam):
    """stage C: |lam - lam64|_inf per foot over max(|lam64|_inf of the robot, 2^-24 B_lambda), in units of 2^-24"""
    den = max(np.abs(r["lam"]).max(), U * r["B_lam"])
    err = np.abs(lam - r["lam"]).reshape(2, 12).max(1)
    return err / den / U


def ratio_D(r, lam, delta):
    """stage D: |delta - H^-1 J^T W^T lam| per component in units of 2^-24 x its absolute-value bound"""
    ref, B = response(r, lam)
    err = np.abs(delta - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(B > 0, err / (U * np.where(B > 0, B, 1.0)), np.where(err == 0, 0.0, np.inf))


def joint_name(i):
    return "base %s%d" % ("w" if i < 3 else "v", i % 3) if i < 6 else "joint %d (%s)" % (i - 6, M.JOINT_NAMES[i - 6])


# ---------------------------------------------------------------- cases
def _detect_one(kind, row):
    d = detect(kind, row[None])
    return d["slot"][0], bool(d["safe"][0].all())


def _harvest(kind):
    """(state55, action, terrain rows of the stones n-1, n, n+1, source) from oracle rollouts: the shipped actor at curriculum 0 and 3, random
    actions from reset"""
    import torch
    import shipped_actor as sa
    actor = sa.load_actor(kind)
    out = []
    qdmax = 0.0

    def take(o, a, envs, src):
        nonlocal qdmax
        st = o.get_state()
        qdmax = max(qdmax, float(np.abs(st[:, ol.S_QD]).max()))
        for e in envs:
            n = int(st[e, ol.S_N])
            terr = st[e, ol.S_TERRAIN].reshape(20, 6)
            out.append((st[e, :55].astype(np.float64), a[e].astype(np.float64), terr[[max(n - 1, 0), n, min(n + 1, 19)]].astype(np.float64), src))
    for cur, steps, when, envs in ((0, 40, (9, 18, 27, 36), range(0, 12, 2)), (3, 124, (100, 104, 108, 112, 116, 120, 123), range(0, 12, 2))):
        o = ol.OracleEnv(kind, 12, seed=21 + cur)
        o.set_curriculum(cur)
        obs = o.reset()
        for t in range(steps):
            with torch.no_grad():
                a = actor(torch.from_numpy(obs)).numpy().astype(np.float32)
            if t in when:
                take(o, a, envs, "actor c%d" % cur)
            obs = o.step(a)[0]
    o = ol.OracleEnv(kind, 12, seed=5)
    o.set_curriculum(5)
    o.reset()
    for t in range(12):
        a = np.clip(o.random_actions(t), -1, 1)
        if t in (1, 4, 7, 10):
            take(o, a, range(1, 12, 2), "random")
        o.step(a)
    return out, qdmax


@functools.lru_cache(maxsize=None)
def cases(kind):
    """-> dict: inp [n, IW] float32, cls: list of sets of class names per case, src: list, qdmax.  Deterministic."""
    rng = np.random.default_rng([KINDS.index(kind), 4711])
    m = model(kind)
    pool, qdmax = _harvest(kind)
    rows, cls = [], []

    def add(st, act, power, terr, *names):
        rows.append(make_row(st, act, power, terr))
        cls.append(set(names))
        return rows[-1]
    for st, act, terr, src in pool:
        add(st, act, 1.0, terr, src)
    base = np.array(rows)
    d0 = detect(kind, base)
    feet = (d0["slot"] >= 0).any(2)
    both = [i for i in range(len(pool)) if feet[i].all() and d0["safe"][i].all()]
    some = [i for i in range(len(pool)) if feet[i].any() and d0["safe"][i].all()]
    assert len(both) >= 8 and len(some) >= 24, (len(both), len(some))
    # free flight: lifted one metre
    for i in some[:8]:
        st = pool[i][0].copy()
        st[2] += 1.0
        add(st, pool[i][1], 1.0, pool[i][2], "edge: lifted")
    # plank edge: the carrying stone shifted along its heading until a foot keeps 1 or 2 corners
    got = 0
    for i in both + [i for i in some if i not in both]:
        st, act, terr, _ = pool[i]
        carrier = int(np.bincount(d0["slot"][i][d0["slot"][i] >= 0]).argmax())
        found = None
        for s in np.concatenate([[a, -a] for a in np.linspace(0.04, 0.7, 67)]):
            t = terr.copy()
            t[carrier, 0] += s * np.cos(t[carrier, 3])
            t[carrier, 1] += s * np.sin(t[carrier, 3])
            slot, safe = _detect_one(kind, make_row(st, act, 1.0, t))
            cnt = (slot >= 0).sum(1)
            if safe and ((cnt == 1) | (cnt == 2)).any():
                found = t
                break
        if found is not None:
            add(st, act, 1.0, found, "edge: plank edge")
            got += 1
        if got >= 10:
            break
    # a corner carried by slot 0 / slot 2: the carrying stone changes places with the stone of that slot
    for i in some[:14]:
        st, act, terr, _ = pool[i]
        carrier = int(np.bincount(d0["slot"][i][d0["slot"][i] >= 0]).argmax())
        for to in (0, 2):
            order = [0, 1, 2]
            order[carrier], order[to] = order[to], order[carrier]
            add(st, act, 1.0, terr[order], "edge: carried by slot %d" % to)
    # tilted and turned about the stone's own centre, under a standing robot
    for i in (both + some)[:16]:
        st, act, terr, _ = pool[i]
        t = terr.copy()
        t[:, 3] += rng.uniform(-0.35, 0.35)
        t[:, 4:6] += np.radians(rng.uniform(-6, 6, (3, 2)))
        add(st, act, 1.0, t, "edge: tilted")
    # sliding: the whole robot moves sideways over the stone
    for n_, i in enumerate(some[:16]):
        st = pool[i][0].copy()
        ang = 2 * np.pi * n_ / 16
        st[10:12] += 1.5 * np.array([np.cos(ang), np.sin(ang)])
        add(st, pool[i][1], 1.0, pool[i][2], "edge: pushed sideways")
    # joints beyond their limits: one spine, one leg and one arm joint per case, below lo (even cases) / above hi (odd cases)
    for n_ in range(20):
        i = (some + both)[n_ % len(some)]
        st = pool[i][0].copy()
        for grp in (SPINE, LEG, ARM):
            j = grp[(n_ // 2) % len(grp)]
            st[13 + j] = m["range"][j, n_ % 2] + (0.03 + 0.01 * n_) * (1 if n_ % 2 else -1)
        add(st, pool[i][1], 1.0, pool[i][2], "edge: limits %s" % ("hi" if n_ % 2 else "lo"))
    # joint rates up to four times the largest of the rollouts
    for n_, i in enumerate(some[10:20]):
        st = pool[i][0].copy()
        st[34:55] *= (1.0 + 3.0 * (n_ + 1) / 10) * qdmax / np.abs(st[34:55]).max()
        add(st, pool[i][1], 1.0, pool[i][2], "edge: rates")
    # actions at -1, 0, +1 with power 1.0 and 0.6
    for n_ in range(20):
        i = some[n_ % len(some)] if n_ % 4 else n_
        act = rng.integers(-1, 2, 21).astype(np.float64)
        act[:3] = (-1.0, 0.0, 1.0)
        rng.shuffle(act)
        add(pool[i][0], act, 0.6 if n_ % 2 else 1.0, pool[i][2], "edge: actions")
    if len(rows) % 32 == 0:          # never whole wavefronts only: the device build must meet a partial one
        add(pool[0][0], pool[0][1], 1.0, pool[0][2], pool[0][3])
    inp = np.array(rows, np.float32)
    assert inp.shape[0] <= MAX_CASES, inp.shape
    inp.setflags(write=False)
    return dict(inp=inp, cls=cls, qdmax=qdmax)


@functools.lru_cache(maxsize=None)
def prepared(kind):
    """cases + their references + class membership decided by the reference"""
    c = cases(kind)
    refs, det = references(kind, c["inp"])
    return dict(c, refs=refs, det=det, contact=np.array([r["active"].any() for r in refs]))


def warm_changed_rows(kind, second):
    """from second-substep rows (feedback_rows): the carrying stone shifted along its heading so that the set of active corners differs from the
    warm key while some warm corner stays -- a warm start that must mask.  -> rows (possibly fewer than asked), deterministic"""
    out = []
    for row in second:
        x = row.astype(np.float64)
        key = x[[I_WARM, I_WARM + 13]].astype(np.int64)
        if not key.any():
            continue
        slot0, _ = _detect_one(kind, row)
        if not (slot0 >= 0).any():
            continue
        carrier = int(np.bincount(slot0[slot0 >= 0]).argmax())
        c, s = x[I_STONES + 8 * carrier + 6], x[I_STONES + 8 * carrier + 7]
        for sh in np.concatenate([[a, -a] for a in np.linspace(0.04, 0.7, 34)]):
            r2 = row.copy()
            r2[I_STONES + 8 * carrier] = F32(x[I_STONES + 8 * carrier] + sh * c)
            r2[I_STONES + 8 * carrier + 1] = F32(x[I_STONES + 8 * carrier + 1] + sh * s)
            slot, safe = _detect_one(kind, r2)
            act = ((slot >= 0) << np.arange(4)).sum(1)
            if safe and (act != key).any() and (act & key).any():
                out.append(r2)
                break
    return np.array(out, np.float32).reshape(-1, IW)


def reference_feedback(kind, inp, refs):
    """what feedback_rows makes of a kernel's output, made of the REFERENCE's own substep (fp64 rounded to fp32): for the class counts"""
    rows = []
    for row, r in zip(inp, refs):
        v1 = np.concatenate([r["v0f"], r["qdf"]]) + r["dv"]
        q1 = r["q"] + H32 * v1[6:]
        Rb = nd.quat_rot(r["quat"])
        pos1 = r["pos"] + H32 * (Rb @ v1[3:6])
        w, x, y, z = r["quat"]
        ox, oy, oz = v1[:3]
        qn = np.array([w + 0.5 * H32 * (-x * ox - y * oy - z * oz), x + 0.5 * H32 * (w * ox + y * oz - z * oy),
                       y + 0.5 * H32 * (w * oy - x * oz + z * ox), z + 0.5 * H32 * (w * oz + x * oy - y * ox)])
        o = np.array(row, np.float32)
        o[:55] = f32(np.concatenate([pos1, qn / np.linalg.norm(qn), v1[:6], q1, v1[6:]]))
        for f in (0, 1):
            act = r["active"][f]
            o[I_WARM + 13 * f] = (act << np.arange(4)).sum() if r["active"].any() else 0
            o[I_WARM + 13 * f + 1:I_WARM + 13 * f + 13] = f32((r["lam"][4 * f:4 * f + 4] * (M_LAM if f else 1.0)).reshape(12))
        rows.append(o)
    return np.array(rows, np.float32)


# ---------------------------------------------------------------- the fp32 oracle on the same cases
def _oracle_state(template, row, terr_words):
    st = template.copy()
    st[:55] = row[:55]
    st[ol.S_N] = 1
    terr = np.tile(FAR, (20, 1))
    terr[:3] = terr_words
    st[ol.S_TERRAIN] = terr.reshape(120)
    return st


def _terrain_of(row):
    """terrain rows (x, y, z, phi, x_tilt, y_tilt) that give the row's stones: phi from the heading, the tilts from the normal"""
    x = row.astype(np.float64)
    out = []
    for sl in range(3):
        w = x[I_STONES + 8 * sl:I_STONES + 8 * sl + 8]
        phi = np.arctan2(w[7], w[6])
        c, s = np.cos(phi), np.sin(phi)
        a = np.array([c * w[3] + s * w[4], -s * w[3] + c * w[4], w[5]])          # Rz(-phi) n = (cos xt sin yt, -sin xt, cos xt cos yt)
        xt = -np.arcsin(np.clip(a[1], -1, 1))
        yt = np.arctan2(a[0], a[2])
        out.append([w[0], w[1], w[2], phi, xt, yt])
    return np.array(out)


def oracle_measure(kind):
    """The fp32 oracle's worst ratios on the cases of prepared(kind) by the formulas the kernels are judged with: {"A", "C", "D"}.  Cold
    cases by debug_contact(prior=0); the warm second substep by debug_contact(prior=1) against the reference fed the oracle's own first
    substep (state and impulses).  Cases the reference does not decide, or where the oracle's own fp32 normals decide another contact set, are
    left out of C and D, as the kernels' are."""
    P = prepared(kind)
    m = model(kind)
    o = ol.OracleEnv(kind, 1, seed=0, prec="f32")
    o.reset()
    template = o.get_state()[0]
    worst = {"A": 0.0, "C": 0.0, "D": 0.0}
    used = {"A": 0, "C": 0, "D": 0}

    def judge(r, tap, contact_too):
        worst["A"] = max(worst["A"], float(ratio_A(r, tap["v0f"].astype(np.float64), tap["qdf"].astype(np.float64)).max()))
        used["A"] += 1
        if not (contact_too and r["safe"] and r["active"].any()) or not np.array_equal(tap["active"].astype(bool), r["active"].reshape(8)):
            return
        lam = tap["lam"].astype(np.float64)
        worst["C"] = max(worst["C"], float(ratio_C(r, lam).max()))
        rd = ratio_D(r, lam, np.concatenate([tap["dv0"], tap["dqd"]]).astype(np.float64))
        worst["D"] = max(worst["D"], float(rd.max()))
        used["C"] += 1
        used["D"] += 1
    second = []
    for e, (row, r) in enumerate(zip(P["inp"], P["refs"])):
        x = row.astype(np.float64)
        tau = f32(x[I_POWER] * m["torque"] * POLICY * x[I_ACT:I_ACT + 21])
        st0 = _oracle_state(template, row, _terrain_of(row))
        o.set_state(st0[None])
        tap0 = o.debug_contact(0, tau, 0)
        judge(r, tap0, True)
        if r["active"].any() and r["safe"] and len(second) < 48:
            st1 = o.get_state()[0]
            row2 = np.array(row, np.float32)
            row2[:55] = st1[:55]
            act = tap0["active"].astype(np.int64).reshape(2, 4)
            for f in (0, 1):
                row2[I_WARM + 13 * f] = (act[f] << np.arange(4)).sum()
                row2[I_WARM + 13 * f + 1:I_WARM + 13 * f + 13] = (tap0["lam"][4 * f:4 * f + 4].astype(np.float64) * (M_LAM if f else 1.0)).reshape(12)
            o.set_state(st0[None])
            second.append((row2, o.debug_contact(0, tau, 1)))
    rows2 = np.array([s[0] for s in second], np.float32)
    refs2, _ = references(kind, rows2)
    for (row2, tap1), r2 in zip(second, refs2):
        judge(r2, tap1, True)
    return worst, used


def power_of_two_above(x):
    return 2 ** int(np.ceil(np.log2(x)))
