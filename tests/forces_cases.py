"""Cases, references and judgement for the force readout (ss_step_forces, docs/PHYSICS.md 10), shared by tests/test_step_forces.py (the
CPU build of ss_forces.hpp) and tests/test_gpu_step_forces.py (the kernel).  Nothing here is a fixture: the cases are drawn at test time
from the CPU oracle (deterministic).

Case set per robot: 64 envs of the fp64 oracle, seed 5, curriculum 5, reset, three control steps of random actions; the state after them,
rounded to fp32 (what the readout is given), and the actions random_actions(1000).  Reference per (env, substep s): the oracle put back
into that state, debug_contact(e, motor torques, prior=s): the impulses, normals, penetrations, active corners and stones of substep s.

Bounds.  Every tolerance is counted on the source or taken from the fp32 oracle's own distance to the fp64 oracle; none comes from the code
under test.
  K_TAU = 8      joint row 2 against PHYSICS.md 3.1 in fp64 from rows 0 / 1, in units of 2^-24 B_tau (B_tau: the sum of the absolute
                 values of the terms, tests/substep_cases.py).  joint_tau: power tq act 2 roundings, kd qd 1, ks (q + h qd) 3,
                 kl (viol + h qd) 3 with viol = q - bound 1, dl qd 1: at most 3 per term; four additions of partial sums below B_tau: 7.
                 One more for the terms of second order.
  K_APPLIED = 10 row 3 = t - c (240 qd+), t = tau + c (240 qd), c = h (kd + dl) + h^2 (ks + kl), in units of 2^-24 (B_tau +
                 c (|qd+| + |qd|) / h): c carries 4 roundings (h^2 is a rounded constant), 240 x none but 240 kH = 1 to half a
                 rounding only, the product 6, t's sum K_TAU + 1 and 7, the last difference K_TAU + 2 = 10 and 8.
  WORLD          words 5:8 against f_n n + f_t1 t1 + f_t2 t2 in fp64 from the row's words 2:5 and the fp64 normal of the stone's fp32
                 terrain words: 2^-24 (14 sum|f| + 9 (|f_n| + 2 |f_t1| + 4.3 |f_t2|)), at most 53 sum|f|.  14 is the arithmetic on the
                 stored normal (all components of n, t1, t2 are below 1: t1 before scaling 2, its squared norm 7, rsqrt 7 / 2 + 2, t1 9,
                 t2 = n x t1 11, the products 1 / 10 / 12, two additions 14).  More than 32 because the STORED normal is itself fp32
                 arithmetic on sincosf (stone_normal: 2 roundings per sincosf value, products 5, the rotation by phi 9 per component) and
                 the test has only the terrain words; that distance enters n once, t1 = normalize(e_x - n_x n) twice, t2 = n x t1 4.3
                 times (1.42 + 2 x 1.42)."""
import functools

import numpy as np

import oracle_lib as ol
import substep_cases as sc

U = sc.U
KINDS = sc.KINDS
F32 = np.float32
H32 = sc.H32
N_ENVS, SUBSTEPS = 64, 4
K_TAU, K_APPLIED = 8, 10
K_WORLD_SUM, K_WORLD_NORMAL = 14, 9
WORLD_WEIGHT = np.array([1.0, 2.0, 4.3])
MAX_LEFT_OUT = 0.02                       # of the 256 (env, substep) pairs
ORACLE_MARGIN = 4.0
EX = np.array([1.0, 0.0, 0.0])


@functools.lru_cache(maxsize=None)
def cases(kind):
    """-> dict: st [64,186] float32 (the state), act [64,21] float32, tau [64,21] float64 (the oracle's motor torques), n [64] int"""
    o = ol.OracleEnv(kind, N_ENVS, seed=5, prec="f64")
    o.set_curriculum(5)
    o.reset()
    for t in range(3):
        o.step(o.random_actions(t))
    st = o.get_state().astype(np.float32)
    act = o.random_actions(1000)
    o.close()
    m = sc.model(kind)
    tau = np.clip(act.astype(np.float64), -1.0, 1.0) * m["torque"] * sc.POLICY
    for a in (st, act, tau):
        a.setflags(write=False)
    return dict(st=st, act=act, tau=tau, n=st[:, ol.S_N].astype(np.int64))


@functools.lru_cache(maxsize=None)
def tilted_cases(kind):
    """The case set on turned and tilted stones: three steps after a reset every stone is still the flat provisional one, whose world
    vector is the local one permuted.  The first three stones of every env are turned by up to 0.35 rad and tilted by up to 6 degrees
    about their own centres, under the standing robot (the `tilted` edge of tests/substep_cases.py)."""
    c = dict(cases(kind))
    rng = np.random.default_rng([KINDS.index(kind), 77])
    st = c["st"].copy()
    terr = st[:, ol.S_TERRAIN].reshape(N_ENVS, 20, 6).astype(np.float64)
    terr[:, :3, 3] += rng.uniform(-0.35, 0.35, (N_ENVS, 3))
    terr[:, :3, 4:6] += np.radians(rng.uniform(-6, 6, (N_ENVS, 3, 2)))
    st[:, ol.S_TERRAIN] = terr.reshape(N_ENVS, 120).astype(np.float32)
    st.setflags(write=False)
    c["st"] = st
    return c


@functools.lru_cache(maxsize=None)
def oracle_taps(kind, prec):
    """The oracle of precision prec on the case set: per (env, s) lam [8,3], nrm [8,3], pen [8], active [8], stone [8], stacked
    [64, 4, ...], float64"""
    c = cases(kind)
    o = ol.OracleEnv(kind, N_ENVS, seed=5, prec=prec)
    o.set_curriculum(5)
    o.reset()
    out = {k: [] for k in ("lam", "nrm", "pen", "active", "stone")}
    for e in range(N_ENVS):
        rows = {k: [] for k in out}
        for s in range(SUBSTEPS):
            o.set_state(c["st"])
            tap = o.debug_contact(e, c["tau"][e], prior=s)
            for k in out:
                rows[k].append(np.asarray(tap[k], np.float64))
        for k in out:
            out[k].append(np.stack(rows[k]))
    o.close()
    return {k: np.stack(v) for k, v in out.items()}


def tangents(n):
    """t1, t2 of PHYSICS.md 3.4 for unit normals n [..., 3]"""
    t1 = EX - n[..., :1] * n
    t1 = t1 / np.linalg.norm(t1, axis=-1, keepdims=True)
    return t1, np.cross(n, t1)


def world_force(f, n):
    t1, t2 = tangents(n)
    return f[..., 0:1] * n + f[..., 1:2] * t1 + f[..., 2:3] * t2


def reference_rows(kind, taps):
    """taps (oracle_taps) -> what the readout should say: slot [64,4,8] (-1: not carried; -2: carried, slot not comparable), pen
    [64,4,8], force [64,4,8,3] = lam / h, world [64,4,8,3]"""
    c = cases(kind)
    on = taps["active"] != 0
    n = c["n"][:, None, None]
    slot = np.where(on, np.where((n >= 1) & (n <= 18), taps["stone"] - (n - 1), -2), -1).astype(np.int64)
    force = np.where(on[..., None], taps["lam"] * 240.0, 0.0)
    nrm = np.where(on[..., None], taps["nrm"], np.array([0.0, 0.0, 1.0]))
    return dict(on=on, slot=slot, pen=np.where(on, taps["pen"], 0.0), force=force, world=np.where(on[..., None], world_force(force, nrm), 0.0))


def split(contacts):
    c = np.asarray(contacts, np.float64).reshape(-1, SUBSTEPS, 8, 8)
    return dict(on=c[..., 0] >= 0, slot=c[..., 0].astype(np.int64), pen=c[..., 1], force=c[..., 2:5], world=c[..., 5:8])


def distances(got, ref):
    """-> (used [64,4] bool: the pairs whose carried set equals the reference's in this and every earlier substep of the env,
    force distance [64,4], pen distance [64,4]): |d f| / max(1 N, max |f| of that substep) over words 2:8, |d pen| / max(1 m, max pen)"""
    same = (got["on"] == ref["on"]).all(2)
    used = np.logical_and.accumulate(same, axis=1)
    fmax = np.maximum(1.0, np.abs(ref["force"]).max((2, 3)))
    df = np.maximum(np.abs(got["force"] - ref["force"]).max((2, 3)), np.abs(got["world"] - ref["world"]).max((2, 3))) / fmax
    dp = np.abs(got["pen"] - ref["pen"]).max(2) / np.maximum(1.0, np.abs(ref["pen"]).max(2))
    return used, df, dp


@functools.lru_cache(maxsize=None)
def yardstick(kind):
    """The fp32 oracle against the fp64 oracle on the case set -> dict: ref (reference_rows of the fp64 oracle), left_out (pairs of the
    fp32 oracle outside `used`), force / pen: its largest distances on the used pairs"""
    ref = reference_rows(kind, oracle_taps(kind, "f64"))
    o32 = reference_rows(kind, oracle_taps(kind, "f32"))
    used, df, dp = distances(o32, ref)
    return dict(ref=ref, left_out=int((~used).sum()), force=float(df[used].max()), pen=float(dp[used].max()),
                force_abs=float((np.abs(o32["force"] - ref["force"]).max((2, 3))[used]).max()), fmax=float(np.abs(ref["force"]).max()))


def judge_against_oracle(kind, contacts, label):
    """test 6: contacts [64,4,8,8] of the case set against the fp64 oracle, tolerance 4 x the fp32 oracle's own distance"""
    y = yardstick(kind)
    ref, got = y["ref"], split(contacts)
    used, df, dp = distances(got, ref)
    left = int((~used).sum())
    print("%s %s: left out %d of %d pairs; force distance %.3g (fp32 oracle %.3g, bound %.3g), pen distance %.3g (fp32 oracle %.3g, bound "
          "%.3g); largest force %.4g N, largest |d f| %.3g N" %
          (label, kind, left, used.size, df[used].max(), y["force"], ORACLE_MARGIN * y["force"], dp[used].max(), y["pen"],
           ORACLE_MARGIN * y["pen"], y["fmax"], (np.abs(got["force"] - ref["force"]).max((2, 3))[used]).max()))
    assert left <= MAX_LEFT_OUT * used.size, "%d (env, substep) pairs differ from the oracle's carried set" % left
    assert df[used].max() <= ORACLE_MARGIN * y["force"], "forces: %g over %g" % (df[used].max(), ORACLE_MARGIN * y["force"])
    assert dp[used].max() <= ORACLE_MARGIN * y["pen"], "pen: %g over %g" % (dp[used].max(), ORACLE_MARGIN * y["pen"])
    cmp = used[:, :, None] & ref["on"] & (ref["slot"] >= 0)
    assert cmp.any() and (got["slot"][cmp] == ref["slot"][cmp]).all(), "a corner is carried by another stone than the oracle's"
    return dict(left_out=left, force=float(df[used].max()), pen=float(dp[used].max()))


def stone_normals(st):
    """fp64 normals of the active stones n-1, n, n+1 from the fp32 terrain words of packed states [N,186] -> [N,3,3]"""
    st = np.asarray(st, np.float64)
    out = np.zeros((st.shape[0], 3, 3))
    for e in range(st.shape[0]):
        n = int(st[e, ol.S_N])
        terr = st[e, ol.S_TERRAIN].reshape(20, 6)
        for sl, k in enumerate((max(n - 1, 0), n, min(n + 1, 19))):
            out[e, sl] = sc.nc.stone_normal(terr[k])
    return out


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def judge_cone_and_zeros(kind, contacts, st, label):
    """test 5 on contacts [N,4,8,8] of the states st [N,186]"""
    c = np.asarray(contacts, np.float32).reshape(-1, SUBSTEPS, 8, 8)
    g = split(c)
    on = g["on"]
    assert np.isin(c[..., 0], (-1.0, 0.0, 1.0, 2.0)).all()
    assert (c[~on][:, 1:] == 0).all(), "a corner that is not carried has a non-zero word"
    assert on.any() and (g["force"][..., 0] >= 0).all()
    assert ((g["pen"][on] > 0) & (g["pen"][on] < 0.10)).all()
    mu = sc.model(kind)["friction"]
    lim = (F32(mu) * c[..., 2]).astype(np.float32)                        # mu f_n as fp32 forms it
    room = lim.astype(np.float64) + 4 * ulp32(lim)                       # three roundings separate the clamp on lambda from this product
    assert (np.abs(g["force"][..., 1]) <= room).all() and (np.abs(g["force"][..., 2]) <= room).all(), "outside the friction pyramid"
    nrm = stone_normals(st)
    slot = np.where(on, g["slot"], 1)
    n = np.take_along_axis(nrm[:, None, :, :].repeat(SUBSTEPS, 1), slot[..., None].repeat(3, -1), axis=2)      # [N,4,8,3]
    want = world_force(g["force"], n)
    af = np.abs(g["force"])
    bound = U * (K_WORLD_SUM * af.sum(-1) + K_WORLD_NORMAL * (af * WORLD_WEIGHT).sum(-1))
    err = np.abs(g["world"] - want).max(-1)
    worst = (err[on] / np.maximum(bound[on], 1e-300)).max()
    print("%s %s: world vector, worst err / bound %.3f over %d carried corner rows; sliding rows %d" %
          (label, kind, worst, int(on.sum()), int((np.abs(g["force"][..., 1:]).max(-1)[on] >= lim[on] * (1 - 1e-6)).sum())))
    assert (err[on] <= bound[on]).all(), "world vector outside its bound: worst ratio %.3f" % worst


def judge_flags(contacts, next_state):
    """next_state word 55 against the last substep's detection in the same call: bit 0 / 1 a foot has a carried corner, bit 2 / 3 one
    carried by the target stone (slot 1)"""
    slot = np.asarray(contacts, np.float32).reshape(-1, SUBSTEPS, 2, 4, 8)[:, SUBSTEPS - 1, :, :, 0]
    flags = np.asarray(next_state, np.float32)[:, 55].astype(np.int64)
    assert (flags >= 0).all() and (flags < 16).all()
    for foot in (0, 1):
        assert (((flags >> foot) & 1) == (slot[:, foot] >= 0).any(1)).all(), "contact flag of foot %d" % foot
        assert (((flags >> (2 + foot)) & 1) == (slot[:, foot] == 1).any(1)).all(), "target flag of foot %d" % foot
    return flags


def joint_reference(kind, joints, next_state, act, power=1.0):
    """fp64 PHYSICS.md 3.1 from the readout's own rows 0 / 1 -> dict: tau, B_tau, applied, B_applied [N,4,21], viol [N,4,21]"""
    m = sc.model(kind)
    j = np.asarray(joints, np.float64).reshape(-1, SUBSTEPS, 4, 21)
    q, qd = j[:, :, 0], j[:, :, 1]
    qd_next = np.concatenate([qd[:, 1:], np.asarray(next_state, np.float64)[:, None, 34:55]], 1)
    a = np.clip(np.asarray(act, np.float64), -1.0, 1.0)[:, None, :]
    tau_m = float(F32(power)) * m["torque"] * sc.POLICY * a
    lo, hi = m["range"][:, 0], m["range"][:, 1]
    viol = np.where(q > hi, q - hi, np.where(q < lo, q - lo, 0.0))
    kl, dl = np.where(viol != 0, m["k_lim"], 0.0), np.where(viol != 0, m["d_lim"], 0.0)
    tau = tau_m - m["damping"] * qd - m["stiffness"] * (q + H32 * qd) - kl * (viol + H32 * qd) - dl * qd
    B_tau = np.abs(tau_m) + m["damping"] * np.abs(qd) + m["stiffness"] * (np.abs(q) + H32 * np.abs(qd)) + \
        kl * (np.abs(viol) + H32 * np.abs(qd)) + dl * np.abs(qd)
    c = H32 * (m["damping"] + dl) + H32 * H32 * (m["stiffness"] + kl)          # Dadd - armature
    applied = tau - c * (qd_next - qd) / H32
    B_applied = B_tau + c * (np.abs(qd_next) + np.abs(qd)) / H32
    return dict(tau=tau, B_tau=B_tau, applied=applied, B_applied=B_applied, viol=viol)


def judge_joint_torques(kind, joints, next_state, act, label, power=1.0):
    """test 7"""
    j = np.asarray(joints, np.float64).reshape(-1, SUBSTEPS, 4, 21)
    r = joint_reference(kind, joints, next_state, act, power)
    assert (r["viol"] != 0).any(), "no joint beyond a limit in the set"
    r2 = np.abs(j[:, :, 2] - r["tau"]) / (U * r["B_tau"])
    r3 = np.abs(j[:, :, 3] - r["applied"]) / (U * r["B_applied"])
    out = r["viol"] != 0
    print("%s %s: tau worst %.3f of K = %d (beyond a limit: %.3f over %d joint rows), applied worst %.3f of K = %d" %
          (label, kind, r2.max(), K_TAU, r2[out].max(), int(out.sum()), r3.max(), K_APPLIED))
    assert r2.max() <= K_TAU, "row 2: %.3f x 2^-24 B_tau at %s" % (r2.max(), np.unravel_index(r2.argmax(), r2.shape))
    assert r3.max() <= K_APPLIED, "row 3: %.3f x 2^-24 B at %s" % (r3.max(), np.unravel_index(r3.argmax(), r3.shape))
