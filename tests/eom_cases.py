"""The rows tests/test_eom.py and tests/test_gpu_eom.py judge the equation-of-motion readout on, the asserted error factors, and the
judgements both share.  TEST INFRASTRUCTURE ONLY.

Rows: kinematics_cases.sample(kind) (about 200 per robot: reset states, states 30 random steps in at curricula 0 and 5, joints at both
range ends, large rates, tilted torso); shifted(rows): the same rows with the torso position and every terrain centre moved by SHIFT.

K[group]: |code - fp64| <= K * 2^-24 * B is asserted (np_eom.readout gives value and B).  Each K is 4 x the worst ratio the CPU build of
steppingstone_amd/csrc/ss_eom.hpp reached on sample() of both robots (WORST below; docs/HISTORY.md has them per robot): the margin covers
the gfx950 build contracting the same source expressions differently, and the GPU test's states being another draw.  B is a worst-case
bound without cancellation whose rotation entries carry 1 + depth (np_kinematics), so a word that passes through several rotations and
products of rates -- `bias` -- has a B some 10^4 above its size and a ratio far below 1.

closing(...): the substep identity of PHYSICS.md 11 on forces_cases.cases(kind), see its docstring."""
import functools

import numpy as np

import forces_cases as fc
import kinematics_cases as kc
import np_eom as ne
import np_kinematics as nk
import np_dynamics as npd

KINDS = kc.KINDS
U = ne.U
SHIFT = np.array([15.0, -3.0, 2.0])

# worst |code - fp64| / (2^-24 B) of the host build over sample() of both robots, rounded up in the third digit, and the asserted
# factor: 4 x that.  Measured (walker3d / mike): mass 1.580 / 1.092, bias 9.376e-5 / 7.907e-5, gravity 1.307 / 1.337, passive
# 2.171 / 2.191, corner_jac 1.274 / 1.973.
WORST = {"mass": 1.59, "bias": 9.38e-5, "gravity": 1.34, "passive": 2.20, "corner_jac": 1.98}
K = {g: 4.0 * w for g, w in WORST.items()}
MARGIN = fc.ORACLE_MARGIN       # the closing test: readout against the measured yardstick


def model(kind):
    return kc.model(kind)


def sample(kind):
    return kc.sample(kind)


def shifted(rows):
    """rows [n,186] with the torso position and the 20 terrain centres moved by SHIFT (fp32 again)"""
    st = np.array(rows, np.float64)
    st[:, 0:3] += SHIFT
    terr = st[:, 65:185].reshape(-1, 20, 6)
    terr[:, :, :3] += SHIFT
    return st.astype(np.float32)


@functools.lru_cache(maxsize=None)
def references(kind):
    """np_eom.readout of every row of sample(kind): computed once, shared by the tests, never changed"""
    m = model(kind)
    return tuple(ne.readout(m, s) for s in sample(kind))


@functools.lru_cache(maxsize=None)
def closing_references(kind):
    """np_eom.readout of the 64 rows of forces_cases.cases(kind)"""
    m = model(kind)
    return tuple(ne.readout(m, s) for s in fc.cases(kind)["st"])


def stack(refs, group, which):
    return np.stack([r[group][which] for r in refs])


def beyond_limit(kind, q):
    lo, hi = ne.stored_range(model(kind))
    return (q > hi) | (q < lo)


def outside(got, refs, groups=ne.GROUPS):
    """{group: (worst ratio, K)} of the groups of got (np_eom.split_outputs) outside their K; also returns all worst ratios"""
    worst = ne.worst_ratios(got, refs)
    return {g: (w, K[g]) for g, w in worst.items() if g in groups and not w <= K[g]}, worst


def residual_ratio(kind, st, step, mass, bias, gravity, jac):
    """max over (env, joint) of |r| / B for the joint rows of PHYSICS.md 11's substep identity on substep 0 of a control step:
        (M + diag(0_6, Dadd - armature)) a = [0_6; tau] - c + g + sum_c J_c^T f_c,   a = (nu+ - nu) / h.
    st [n,186]: the states; step: ss_step_forces' contacts [n,4,8,8] and joints [n,4,4,21] on them; mass, bias, gravity, jac: the terms
    [n,...] under judgement (fp64).  a_j = (qd_1 - qd_0) / h from the joints rows; the base acceleration a_0, which ss_step_forces does
    not report per substep, solves the identity's six base rows (a 6 x 6 composite-inertia solve); r is what is left in the joint rows,
    B the sum of the absolute values of every product and term r is made of."""
    m = model(kind)
    h = fc.H32
    j = np.asarray(step["joints"], np.float64)
    c = np.asarray(step["contacts"], np.float64)
    q0, qd0, qd1, tau = j[:, 0, 0], j[:, 0, 1], j[:, 1, 1], j[:, 0, 2]
    f = c[:, 0, :, 5:8]                                            # [n,8,3] world force on each corner over substep 0
    out = beyond_limit(kind, q0)
    kl, dl = np.where(out, m["k_lim"], 0.0), np.where(out, m["d_lim"], 0.0)
    D = h * (m["damping"] + dl) + h * h * (m["stiffness"] + kl)    # Dadd - armature
    aj = (qd1 - qd0) / h
    Jf = np.einsum("ncik,nci->nk", jac, f)
    Jf_abs = np.einsum("ncik,nci->nk", np.abs(jac), np.abs(f))
    rhs = -bias + gravity + Jf
    rhs[:, 6:] += tau
    worst = 0.0
    for e in range(st.shape[0]):
        Me = mass[e]
        a0 = np.linalg.solve(Me[:6, :6], rhs[e, :6] - Me[:6, 6:] @ aj[e])
        a = np.concatenate([a0, aj[e]])
        r = Me[6:] @ a + D[e] * aj[e] - rhs[e, 6:]
        B = np.abs(Me[6:]) @ np.abs(a) + D[e] * np.abs(aj[e]) + np.abs(tau[e]) + np.abs(bias[e, 6:]) + np.abs(gravity[e, 6:]) + Jf_abs[e, 6:]
        worst = max(worst, float(np.max(np.abs(r) / B)))
    return worst


def judge_closing(kind, st, step, got, label):
    """test 5: rho of the readout `got` (np_eom.split_outputs) against rho of np_eom's own fp64 terms -- the substep's own fp32 error, the
    yardstick, measured here -- on the same ss_step_forces output.  Returns (rho_readout, rho_ref) in units of 2^-24."""
    refs = closing_references(kind)
    j = np.asarray(step["joints"], np.float64)
    carried = int((np.asarray(step["contacts"])[:, 0, :, 0] >= 0).sum())
    beyond = int(beyond_limit(kind, j[:, 0, 0]).sum())
    f64 = lambda g: np.asarray(got[g], np.float64)
    rho_got = residual_ratio(kind, st, step, f64("mass"), f64("bias"), f64("gravity"), f64("corner_jac")) / U
    rho_ref = residual_ratio(kind, st, step, *(stack(refs, g, 0) for g in ("mass", "bias", "gravity", "corner_jac"))) / U
    print("%s %s: substep identity, worst |r| / B: readout %.3f x 2^-24, fp64 terms %.3f x 2^-24 (bound %.3f); %d corners carried at "
          "substep 0, %d joints beyond a limit" % (label, kind, rho_got, rho_ref, MARGIN * rho_ref, carried, beyond))
    assert carried >= 32 and beyond >= 32, "the case set must exercise contacts and limits"
    assert rho_got <= MARGIN * rho_ref, "%s: %.3f over %.3f x 2^-24 B" % (kind, rho_got, MARGIN * rho_ref)
    return rho_got, rho_ref


def judge_against_kinematics(kind, st, got, kin, eom_refs, kin_refs):
    """test 4: from the readout `got` (np_eom.split_outputs), in fp64, against the kinematic readout `kin` (np_kinematics.split_outputs)
    of the same rows: J_c nu against corner_vel, nu^T (mass - diag(0, armature)) nu / 2 against kinetic, R (mass[3:6, :] nu) / M_total
    against com_vel.  Tolerance: the sum of both readouts' K 2^-24 B, the equation-of-motion side's carried through the product."""
    m = model(kind)
    st64 = np.asarray(st, np.float64)
    nu = np.concatenate([st64[:, 7:13], st64[:, 34:55]], axis=1)
    anu = np.abs(nu)
    Mm, J = np.asarray(got["mass"], np.float64), np.asarray(got["corner_jac"], np.float64)
    BM, BJ = stack(eom_refs, "mass", 1), stack(eom_refs, "corner_jac", 1)
    arm = np.diag(np.concatenate([np.zeros(6), m["armature"]]))
    tot = float(m["mass"].sum())
    R = np.stack([npd.quat_rot(s[3:7]) for s in st64])
    kK = kc.K
    cv = np.einsum("ncik,nk->nci", J, nu)
    tol = K["corner_jac"] * U * np.einsum("ncik,nk->nci", BJ, anu) + kK["corner_vel"] * U * stack(kin_refs, "corner_vel", 1)
    assert (np.abs(cv - kin["corner_vel"]) <= tol).all(), "J_c nu against corner_vel"
    T = 0.5 * np.einsum("ni,nik,nk->n", nu, Mm - arm, nu)
    tol = 0.5 * K["mass"] * U * np.einsum("ni,nik,nk->n", anu, BM, anu) + kK["kinetic"] * U * stack(kin_refs, "kinetic", 1)
    assert (np.abs(T - kin["kinetic"]) <= tol).all(), "kinetic energy"
    pl = np.einsum("nik,nk->ni", Mm[:, 3:6], nu)
    v = np.einsum("nai,ni->na", R, pl) / tot
    tol = K["mass"] * U * np.einsum("nai,ni->na", np.abs(R), np.einsum("nik,nk->ni", BM[:, 3:6], anu)) / tot + \
        kK["com_vel"] * U * stack(kin_refs, "com_vel", 1)
    assert (np.abs(v - kin["com_vel"]) <= tol).all(), "centre-of-mass velocity"
    return float(np.abs(T - kin["kinetic"]).max())
