"""fp64 reference, running error bounds and test cases for the env logic of a control step behind its substeps (docs/PHYSICS.md 4.3 - 4.10;
ss_kernels.hpp: step_logic, step_score, ep_return_add), as the ops `step_logic`, `step_score` and `ep_return` of tests/device/ss_probe.hip
expose them.  Used by tests/test_step_logic.py.  Written from the specification's text with formulas of its own: roll, pitch and yaw from
the rotation MATRIX (the kernels use quaternion algebra), sums over all 21 joints of the robot (the kernels sum per lane and exchange).

Judgement and counting are those of np_contact_ops: |got - ref| <= k * 2^-24 * B, exact where B = 0; an input carries no rounding, a
constant counts one, k(x + y) = max(k(x), k(y)) + 1, k(x * y) = k(x) + k(y) + 1, k(f(x)) = k(x) + k_f with the OpenCL full-profile ulp of
f (one ulp is at most two roundings).  B = inf marks a component the reference does not decide: it is left out.

Counts (the model's ranges are its fp32 table values and carry no rounding):
  planar distance   dx: 1; dx dx: 3; the sum: 4; sqrtf: 4 + 2 * 3                                                      K_PD   = 10
  potential         -dist / dt: the constant dt 1, the division 10 + 1 + 1                                             K_POT  = 12
  first-touch bonus min of two distances 10; / 0.25 and the negation are exact; expf: 10 + 2 * 3 = 16; 50 * : 17       K_SB   = 17
  e_sum             0.1f (1) * qd: 2; a * : 3; a lane's first term is added to 0 (exact), eleven more: 14; the pair: 15  K_ESUM = 15
  a2                a a: 1; eleven more additions: 12; the pair: 13                                                    K_A2   = 13
  energy            e_sum / 21: 16; the constant 4.5 / 21: 1; their product: 18; likewise a2: 14, 1, 16; the sum        K_EN   = 19
                    (step_score alone: e_sum and a2 are inputs: 1, 1, 3; the sum 4)
  posture           |pitch| (K_PITCH = 10) + |roll| (K_ROLL = 15)                                                      K_POST = 16
  joint penalty     0.1f (1) * count                                                                                    K_LIM  = 2
  reward            progress = pot - pot_prev: 13; + step_bonus: max(13, 17) + 1 = 18; + target_bonus: 19; + tall_bonus: 20;
                    - energy: max(20, 19) + 1 = 21; - posture: 22; - penalty                                           K_R    = 23
                    (step_score alone, step_bonus / e_sum / a2 given: 13, 14, 15, 16, - energy (4): 17, 18, 19         K_R_SCORE = 19)
  normalised angle  as obs_angle (np_contact_ops.K_OA): mid 1, q - mid 2, / span 2 + 1 + 1                                     4
  ep_ret            the pair's head after the step is RN(head + tail + r): K_R + 1; so is the pair's sum

Decisions.  A threshold is a constant the kernel compares with and is taken at its fp32 value (0.7f, 0.3f, 0.15f, -0.2f, 0.4f, 0.99f), so it
has no error of its own; the compared quantity has its counted bound, and the reference decides wherever its margin exceeds that bound.
pos z - sole z and zlow + 0.3f are one correctly rounded operation on inputs: where the fp64 result is an fp32 number the operation is
exact, the bound 0 and the decision the comparison's own, equality included.  d, the presence of both bonuses and the limit count reach
the reward, so a reward is judged only where every decision under it is the reference's to make.  Integer logic (flags, count, n,
advanced, elapsed, bad, the draw's record) involves no rounding and is always exact.

ep_return_add.  Let T be the exact sum, (hi, lo) the pair.  s = RN(hi + r) with err = hi + r - s formed error-free (two-sum); lo' = RN(lo +
err) is the first rounding, of a quantity |lo + err| <= 2^-24 (|hi| + |s|) (|lo| <= ulp(hi) / 2 <= 2^-24 |hi|; |err| <= 2^-24 |s|); the
renormalisation hi' = RN(s + lo'), lo'' = RN(lo' - (hi' - s)) is error-free when |s| >= |lo'| and otherwise rounds once more a quantity no
larger.  With |hi| <= |T_prev|, |s| <= |T_prev| + |r| up to second order: a step adds at most 2 * 2^-24 * 2^-24 (2 |T_prev| + |r|), so
after t steps |hi + lo - T_t| <= K_EP * 2^-24 * B_t with K_EP = 2 and B_t = 2^-24 * sum_i (2 |T_(i-1)| + |r_i|) (1 + 2^-20)."""
import functools
import math

import numpy as np

import np_contact_ops as no

U = no.U
KINDS = no.KINDS
N_RANDOM = 2048
F32 = np.float32
OPENCL_ULP = no.OPENCL_ULP                      # OpenCL 3.0 full profile, single precision: sqrt 3 ulp, exp 3 ulp
K_EXP = 2 * OPENCL_ULP["exp"]
K_PD = 4 + 2 * OPENCL_ULP["sqrt"]
assert K_PD == no.K_PD
K_POT, K_SB, K_ESUM, K_A2, K_EN, K_POST, K_LIM = K_PD + 2, K_PD + K_EXP + 1, 15, 13, 19, max(no.K_PITCH, no.K_ROLL) + 1, 2
K_R = max(max(max(K_POT + 1, K_SB) + 3, K_EN) + 1, K_POST) + 2
K_R_SCORE = max(K_POT + 1 + 3, 4) + 1 + 2
assert (K_POT, K_SB, K_POST, K_R, K_R_SCORE) == (12, 17, 16, 23, 19)
K_QN = no.K_OA
K_EP = 2
DT = 1.0 / 60.0
NUM_STONES, MAX_STEPS = 20, 1000
T_HEIGHT, T_LOW, T_TARGET, T_PITCH_LO, T_PITCH_HI, T_ROLL, T_QN = (float(F32(x)) for x in (0.7, 0.3, 0.15, -0.2, 0.4, 0.4, 0.99))
INF = np.inf


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def as_bits(i):
    """integers -> the float32 words that carry them as raw bits"""
    return np.asarray(i, np.int64).astype(np.uint32).view(np.float32)


def from_bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)


def _rng(name, kind):
    return np.random.default_rng([sum(name.encode()), KINDS.index(kind), 41017])


# ================================================================ pieces
def planar(a, b):
    """planar distance of points given as inputs -> (ref, B)"""
    d, Bd = a[..., :2] - b[..., :2], np.abs(a[..., :2]) + np.abs(b[..., :2])
    s2, Bs2 = (d * d).sum(-1), (Bd * Bd).sum(-1)
    ref = np.sqrt(s2)
    with np.errstate(divide="ignore", invalid="ignore"):
        B = np.where(s2 > 0, np.maximum(0.5 * Bs2 / ref, ref), np.where(Bs2 > 0, INF, 0.0))
    return ref, B


def rotation(quat):
    """rows 2 and the first column of R = Rz(yaw) Ry(pitch) Rx(roll) of a unit quaternion (w, x, y, z)"""
    w, x, y, z = (quat[..., i] for i in range(4))
    return dict(r00=1 - 2 * (y * y + z * z), r10=2 * (x * y + w * z), r20=2 * (x * z - w * y), r21=2 * (y * z + w * x), r22=1 - 2 * (x * x + y * y))


def euler(kind, quat):
    """roll, pitch, cos yaw, sin yaw from the rotation matrix -> ref [n, 4], B [n, 4], exact [n, 4].  The bounds are those
    np_contact_ops.obs_ref derives for the same four quantities (error box of atan2's arguments, asin read at the ends of its interval)."""
    n = quat.shape[0]
    R = rotation(quat)
    ref = np.zeros((n, 4))
    ref[:, 0] = np.arctan2(R["r21"], R["r22"])
    ref[:, 1] = -np.arcsin(np.clip(R["r20"], -1.0, 1.0))
    yaw = np.arctan2(R["r10"], R["r00"])
    ref[:, 2], ref[:, 3] = np.cos(yaw), np.sin(yaw)
    x = np.zeros((n, 81))
    x[:, :4] = quat
    oref, oB, oexact = no.obs_ref(kind, x)[:3]
    ok = np.isfinite(quat).all(1)
    assert np.allclose(ref[ok], oref[ok, :4], rtol=0, atol=1e-9)
    return ref, oB[:, :4].copy(), oexact[:, :4].copy()


def decide(value, B, k, thresh, exact_op=False):
    """-> margin of `value` to `thresh` exceeds its bound k U B.  exact_op: `value` is one correctly rounded operation on inputs, exact (bound
    0, every comparison decided) where the fp64 result is an fp32 number"""
    bound = k * U * B
    if exact_op:
        with np.errstate(invalid="ignore", over="ignore"):
            bound = np.where(value.astype(np.float32).astype(np.float64) == value, 0.0, bound)
    with np.errstate(invalid="ignore"):
        return (np.abs(value - thresh) > bound) | (bound == 0)


def score(kind, pos, quat, cp, target_old, sole, pot_prev, advanced, n, elapsed, finite, step_bonus, B_sb, e_sum, B_e, a2, B_a2, at_limit,
          limit_safe):
    """PHYSICS.md 4.6 - 4.9 for arrays of cases (fp64; cp: centres of the stones n-1, n, n+1 AFTER step 5; elapsed AFTER step 3) -> dict of
    (ref, B) pairs, decisions and their `safe` masks"""
    o = {}
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dist_old, B_old = planar(target_old, pos)
        dist_new, B_new = planar(cp[:, 1], pos)
        pot, B_pot = -dist_old / DT, B_old / DT
        o["pot_prev"] = (np.where(advanced != 0, -dist_new / DT, pot), np.where(advanced != 0, B_new / DT, B_pot))
        progress, B_prog = pot - pot_prev, B_pot + np.abs(pot_prev)
        last = n == NUM_STONES - 1
        o["target"] = last & (dist_new < T_TARGET)
        o["target_safe"] = ~last | decide(dist_new, B_new, K_PD, T_TARGET)
        zs = np.minimum(sole[:, 0, 2], sole[:, 1, 2])
        height = pos[:, 2] - zs
        o["tall"] = height > T_HEIGHT
        o["tall_safe"] = decide(height, np.abs(pos[:, 2]) + np.abs(zs), 1, T_HEIGHT, exact_op=True)
        zlow = cp[:, :, 2].min(1)
        o["low"] = pos[:, 2] < zlow + T_LOW
        o["low_safe"] = decide(zlow + T_LOW, np.abs(zlow) + T_LOW, 1, pos[:, 2], exact_op=True)
        o["timeout"] = elapsed >= MAX_STEPS
        causes = [(~o["tall"], o["tall_safe"]), (o["low"], o["low_safe"]), (~finite, np.ones_like(finite)), (o["timeout"], np.ones_like(finite))]
        o["d"] = np.any([c for c, _ in causes], axis=0)
        o["d_safe"] = np.all([s for _, s in causes], axis=0) | np.any([c & s for c, s in causes], axis=0)
        eu, B_eu, ex_eu = euler(kind, quat)
        o["euler"] = (eu, B_eu, ex_eu)
        roll, pitch = eu[:, 0], eu[:, 1]
        o["pitch_out"] = ~((pitch > T_PITCH_LO) & (pitch < T_PITCH_HI))
        o["pitch_safe"] = decide(pitch, B_eu[:, 1], no.K_PITCH, T_PITCH_LO) & decide(pitch, B_eu[:, 1], no.K_PITCH, T_PITCH_HI)
        o["roll_out"] = ~((roll > -T_ROLL) & (roll < T_ROLL))
        o["roll_safe"] = decide(roll, B_eu[:, 0], no.K_ROLL, -T_ROLL) & decide(roll, B_eu[:, 0], no.K_ROLL, T_ROLL)
        posture = np.where(o["pitch_out"], np.abs(pitch), 0.0) + np.where(o["roll_out"], np.abs(roll), 0.0)
        B_post = np.where(o["pitch_out"], B_eu[:, 1], 0.0) + np.where(o["roll_out"], B_eu[:, 0], 0.0)
        energy = (4.5 / 21) * (e_sum / 21) + (0.225 / 21) * (a2 / 21)
        B_en = (4.5 / 21) * (B_e / 21) + (0.225 / 21) * (B_a2 / 21)
        target_bonus, tall_bonus = np.where(o["target"], 2.0, 0.0), np.where(o["tall"], 2.0, -1.0)
        r = progress + step_bonus + target_bonus + tall_bonus - energy - posture - 0.1 * at_limit
        B_r = B_prog + B_sb + target_bonus + np.abs(tall_bonus) + B_en + B_post + 0.1 * at_limit
        r_safe = o["target_safe"] & o["tall_safe"] & o["pitch_safe"] & o["roll_safe"] & limit_safe
        zero = ~finite | ~np.isfinite(r)                 # (0 if non-finite): exact
        # a reward beyond fp32's range in fp32 alone, or no bound at all: not the reference's to state
        r_safe = np.where(zero, True, r_safe & np.isfinite(B_r) & (B_r < 1e30))
        for key in ("target_safe", "tall_safe", "low_safe", "pitch_safe", "roll_safe"):      # moot in a non-finite state: d = 1, r = 0 whatever they say
            o[key] = o[key] | ~finite
        o["r_zero"] = zero
        o["r"] = (np.where(zero, 0.0, r), np.where(zero, 0.0, np.where(r_safe, B_r, INF)))
    return o


# ================================================================ step_score
SCORE_IW, SCORE_OW = 34, 8
SCORE_K = np.array([K_POT, 0, 0, K_R_SCORE, no.K_ROLL, no.K_PITCH, no.K_YAW, no.K_YAW], np.float64)
SCORE_NAMES = ["pot_prev", "d", "bad", "r", "roll", "pitch", "cyaw", "syaw"]


def _assemble_score(s, finite):
    """columns pot_prev, d, bad, r, roll, pitch, cyaw, syaw of a score() result -> ref, B, exact [n, 8]"""
    n = finite.shape[0]
    ref, B, exact = np.zeros((n, 8)), np.zeros((n, 8)), np.zeros((n, 8), bool)
    ref[:, 0], B[:, 0] = s["pot_prev"]
    ref[:, 1], B[:, 1] = s["d"], np.where(s["d_safe"], 0.0, INF)
    ref[:, 2] = s["timeout"]
    ref[:, 3], B[:, 3] = s["r"]
    eu, B_eu, ex_eu = s["euler"]
    ref[:, 4:8], B[:, 4:8], exact[:, 4:8] = eu, B_eu, ex_eu
    exact[:, 1] = s["d_safe"]
    exact[:, 2] = True
    exact[:, 3] = s["r_zero"]
    # what a non-finite input reaches is not stated by the specification beyond d and r
    bad = ~np.isfinite(ref) | np.isnan(B)
    ref[bad], B[bad] = 0.0, INF
    exact &= ~bad
    return ref, B, exact


def score_ref(kind, inp):
    with np.errstate(invalid="ignore"):
        x = inp.astype(np.float64)
    ib = from_bits(inp[:, 26:30]), from_bits(inp[:, 33])
    advanced, n, elapsed, finite, at_limit = ib[0][:, 0], ib[0][:, 1], ib[0][:, 2], ib[0][:, 3] != 0, ib[1]
    s = score(kind, x[:, 0:3], x[:, 3:7], x[:, 7:16].reshape(-1, 3, 3), x[:, 16:19], x[:, 19:25].reshape(-1, 2, 3), x[:, 25], advanced, n, elapsed,
              finite, x[:, 30], np.abs(x[:, 30]), x[:, 31], np.abs(x[:, 31]), x[:, 32], np.abs(x[:, 32]), at_limit.astype(np.float64),
              np.ones(x.shape[0], bool))
    return _assemble_score(s, finite) + (s,)


def quat_of(roll, pitch, yaw):
    """unit quaternion (w, x, y, z) of Rz(yaw) Ry(pitch) Rx(roll)"""
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], -1)


def _scene(rng, n):
    """what step_score and step_logic share of a random case: base pose, three stones, soles, with every branch of 4.6 - 4.9 in reach"""
    c = {}
    c["pos"] = np.concatenate([rng.uniform(-3, 3, (n, 2)), rng.uniform(0.9, 1.6, (n, 1))], 1)
    c["quat"] = quat_of(rng.uniform(-0.7, 0.7, n), rng.uniform(-0.5, 0.7, n), rng.uniform(-np.pi, np.pi, n))
    cp = np.zeros((n, 3, 3))
    cp[:, 1, :2] = c["pos"][:, :2] + rng.uniform(-1.2, 1.2, (n, 2))
    near = rng.random(n) < 0.5                                   # half of the targets within reach of the 0.15 m bonus
    cp[near, 1, :2] = c["pos"][near, :2] + rng.uniform(-0.2, 0.2, (int(near.sum()), 2))
    cp[:, 0, :2] = cp[:, 1, :2] + rng.uniform(-0.9, 0.9, (n, 2))
    cp[:, 2, :2] = cp[:, 1, :2] + rng.uniform(-0.9, 0.9, (n, 2))
    cp[:, :, 2] = rng.uniform(-0.3, 0.3, (n, 3))
    c["cp"] = cp
    sole = cp[:, 1][:, None, :] + rng.uniform(-0.4, 0.4, (n, 2, 3)) * np.array([1.0, 1.0, 0.1])
    short = rng.random(n) < 0.1                                  # a fallen robot: height below 0.7
    sole[short, :, 2] = c["pos"][short, 2][:, None] - rng.uniform(0.2, 0.69, (int(short.sum()), 2))
    c["sole"] = sole
    low = rng.random(n) < 0.1                                    # the torso less than 0.3 above the lowest stone, which is in any slot
    lo_i = np.nonzero(low)[0]
    zl = c["pos"][lo_i, 2] - rng.uniform(-0.2, 0.29, lo_i.size)
    cp[lo_i, :, 2] = zl[:, None] + rng.uniform(0.01, 0.3, (lo_i.size, 3))
    cp[lo_i, rng.integers(0, 3, lo_i.size), 2] = zl
    c["pot_prev"] = -np.hypot(*(cp[:, 1, :2] - c["pos"][:, :2]).T) / DT + rng.uniform(-3, 3, n)
    inf = rng.random(n) < 0.03
    c["pot_prev"][inf] = np.where(rng.random(int(inf.sum())) < 0.5, INF, -INF)
    c["n"] = rng.choice(np.arange(1, 20), n, p=np.array([1.0] * 17 + [4.0, 4.0]) / 25.0)
    c["elapsed"] = np.where(rng.random(n) < 0.06, rng.integers(998, 1001, n), rng.integers(0, 998, n))
    return c


@functools.lru_cache(maxsize=None)
def score_prepared(kind):
    rng = _rng("step_score", kind)
    n = N_RANDOM
    c = _scene(rng, n)
    x = np.zeros((n, SCORE_IW), np.float32)
    x[:, 0:3], x[:, 3:7], x[:, 7:16] = c["pos"], c["quat"], c["cp"].reshape(n, 9)
    adv = rng.random(n) < 0.3
    x[:, 16:19] = np.where(adv[:, None], c["cp"][:, 0], c["cp"][:, 1])         # after an advance the old target is stone n-1
    x[:, 19:25] = c["sole"].reshape(n, 6)
    x[:, 25] = c["pot_prev"]
    x[:, 26], x[:, 27], x[:, 28] = as_bits(adv), as_bits(c["n"]), as_bits(c["elapsed"] + 1)
    x[:, 29] = as_bits(rng.random(n) >= 0.04)
    x[:, 30] = np.where(rng.random(n) < 0.3, 50 * np.exp(-rng.uniform(0, 0.5, n) / 0.25), 0.0)
    x[:, 31], x[:, 32] = rng.uniform(0, 40, n), rng.uniform(0, 21, n)
    x[:, 33] = as_bits(rng.integers(0, 22, n))
    rows, edges = [x], {}
    e0 = n

    def add(name, **kw):
        nonlocal e0
        r = np.zeros(SCORE_IW, np.float32)
        r[0:3], r[3:7] = kw.get("pos", (0.0, 0.0, 1.3)), kw.get("quat", (1.0, 0.0, 0.0, 0.0))
        r[7:16] = np.asarray(kw.get("cp", [[-0.75, 0, 0], [0.5, 0, 0], [1.25, 0, 0]]), np.float64).reshape(9)
        r[16:19] = kw.get("target_old", r[10:13])
        r[19:25] = np.asarray(kw.get("sole", [[0.0, -0.1, 0.0], [0.0, 0.1, 0.0]]), np.float64).reshape(6)
        r[25] = kw.get("pot_prev", -30.0)
        r[26:30] = as_bits([kw.get("advanced", 0), kw.get("n", 5), kw.get("elapsed", 10), kw.get("finite", 1)])
        r[30], r[31], r[32], r[33] = kw.get("step_bonus", 0.0), kw.get("e_sum", 1.0), kw.get("a2", 1.0), as_bits(kw.get("at_limit", 0))
        rows.append(r[None])
        edges[name] = (e0, kw["expect"])
        e0 += 1

    h = F32(T_HEIGHT)
    for name, z, tall in (("height 0.7 - ulp", np.nextafter(h, F32(0)), 0), ("height 0.7", h, 0), ("height 0.7 + ulp", np.nextafter(h, F32(1)), 1)):
        # the stones lie 5 m below, so that only the height decides
        add(name, pos=(0.0, 0.0, z), cp=[[-0.75, 0, -5], [0.5, 0, -5], [1.25, 0, -5]], expect=dict(d=1 - tall, tall=tall))
    t = F32(T_LOW)
    for slot in range(3):
        for name, z, low in (("below", np.nextafter(t, F32(0)), 1), ("at", t, 0), ("above", np.nextafter(t, F32(1)), 0)):
            cp = np.array([[-0.75, 0, 0.2], [0.5, 0, 0.2], [1.25, 0, 0.2]])
            cp[slot, 2] = 0.0
            add("low stone in slot %d: %s zlow + 0.3" % (slot, name), pos=(0.0, 0.0, z), cp=cp, sole=[[0, -0.1, -0.9], [0, 0.1, -0.9]],
                expect=dict(d=low, low=low))
    for nn, bonus in ((19, 1), (18, 0)):
        for dx, inside in ((0.1499, 1), (0.1501, 0)):
            add("target bonus: n = %d, distance %.4f" % (nn, dx), pos=(dx, 0.0, 1.3), cp=[[-0.75, 0, 0], [0.0, 0, 0], [0.75, 0, 0]], n=nn,
                expect=dict(target=bonus * inside))
    for name, roll, pitch, po, ro in (("pitch below -0.2", 0, -0.2001, 1, 0), ("pitch above -0.2", 0, -0.1999, 0, 0), ("pitch below 0.4", 0, 0.3999, 0, 0),
                                      ("pitch above 0.4", 0, 0.4001, 1, 0), ("roll below -0.4", -0.4001, 0.1, 0, 1), ("roll above -0.4", -0.3999, 0.1, 0, 0),
                                      ("roll below 0.4", 0.3999, 0.1, 0, 0), ("roll above 0.4", 0.4001, 0.1, 0, 1)):
        add("posture: " + name, quat=quat_of(np.float64(roll), np.float64(pitch), np.float64(0.3)), expect=dict(pitch_out=po, roll_out=ro))
    fallen = dict(sole=[[0, -0.1, 0.9], [0, 0.1, 0.9]])
    for el in (998, 999, 1000):          # as it comes in: step_score gets elapsed + 1
        add("time limit: elapsed %d, standing" % el, elapsed=el + 1, expect=dict(d=int(el + 1 >= 1000), bad=int(el + 1 >= 1000)))
        add("time limit: elapsed %d, fallen" % el, elapsed=el + 1, expect=dict(d=1, bad=int(el + 1 >= 1000)), **fallen)
    add("not finite", finite=0, expect=dict(d=1, r=0.0))
    for v in (INF, -INF):
        add("pot_prev %r" % v, pot_prev=v, expect=dict(r=0.0, d=0))
    for al in range(22):
        add("at_limit %d" % al, at_limit=al, expect=dict())
    x = np.concatenate(rows)
    if x.shape[0] % 64 == 0:
        x = np.concatenate([x, x[:1]])
    ref, B, exact, s = score_ref(kind, x)
    return no._frozen(dict(inp=x, ref=ref, B=B, exact=exact, s=s, edges=edges, n_random=n))


# ================================================================ ep_return
EP_R = 100                     # rewards per row of the probe
EP_STEPS = 1000


def ep_bound(rewards, start=0.0):
    """rewards [n, T] (fp32 values) -> (T_t [n, T] the exact running sums as fp64 pairs' heads, B_t [n, T]).  The sums are carried as an
    unevaluated fp64 pair (error-free two-sum), which holds 1000 fp32 rewards exactly; test_step_logic checks them against math.fsum."""
    r = np.asarray(rewards, np.float64)
    hi, lo = np.zeros(r.shape[0]) + start, np.zeros(r.shape[0])
    T, B = np.zeros(r.shape), np.zeros(r.shape)
    acc = np.zeros(r.shape[0])
    for t in range(r.shape[1]):
        acc = acc + (2 * np.abs(hi) + np.abs(r[:, t]))
        s = hi + r[:, t]
        bb = s - hi
        err = (hi - (s - bb)) + (r[:, t] - bb)
        lo = lo + err
        hi = s + lo
        lo = lo - (hi - s)
        T[:, t], B[:, t] = hi, U * acc * (1 + 2.0 ** -20)
    return T, B


@functools.lru_cache(maxsize=None)
def ep_prepared():
    rng = _rng("ep_return", "walker3d")
    n, T = N_RANDOM, EP_STEPS
    r = rng.uniform(-2, 2, (n, T))
    run = rng.integers(0, T - 200, n)
    for e in range(0, n, 2):                                     # long runs near -1: a fallen robot's tall_bonus, step after step
        r[e, run[e]:run[e] + 200] = -1 + rng.uniform(-0.02, 0.02, 200)
    r[np.arange(n), rng.integers(0, T, n)] += 50.0               # a first-touch bonus
    edges = {"zeros": n, "alternating": n + 1, "lossy": n + 2}
    zeros = np.zeros(T)
    alt = np.where(np.arange(T) % 2 == 0, 50.0, -50.0)
    lossy = np.full(T, 1e-6)                                     # below half an ulp of 50: an fp32 running sum drops every one of them
    lossy[0], lossy[-1] = 50.0, -50.0
    r = np.concatenate([r, zeros[None], alt[None], lossy[None]]).astype(np.float32)
    naive = np.float32(0)
    for v in r[edges["lossy"]]:
        naive = np.float32(naive + v)
    Tt, B = ep_bound(r)
    assert abs(float(naive) - Tt[edges["lossy"], -1]) > 1e-4 * abs(Tt[edges["lossy"], -1])
    return no._frozen(dict(r=r, T=Tt, B=B, edges=edges))


# ================================================================ step_logic
I_POS, I_QUAT, I_W, I_V, I_Q, I_QD, I_ACT, I_FOOT, I_CACHE, I_HEAD, I_WORDS, I_STUB, LOGIC_IW = 0, 3, 7, 10, 13, 34, 55, 76, 86, 110, 116, 124, 135
(O_BASE, O_FLAGS, O_ADV, O_HD, O_D, O_BAD, O_R, O_EULER, O_POT, O_NNDR, O_EPRET, O_EPSUM, O_N, O_COUNT, O_ELAPSED, O_CTR, O_CACHE, O_LDSHEAD,
 O_DRAW, LOGIC_OWL) = 0, 13, 14, 15, 21, 22, 23, 24, 28, 29, 30, 31, 32, 33, 34, 35, 36, 60, 66, 70
O_STORE = O_DRAW + 3
LOGIC_INT = [O_FLAGS, O_ADV, O_D, O_BAD, O_N, O_COUNT, O_ELAPSED, O_CTR, O_DRAW, O_DRAW + 1, O_DRAW + 2, O_DRAW + 3]
LOGIC_K = np.zeros(LOGIC_OWL)
LOGIC_K[O_R], LOGIC_K[O_EULER:O_EULER + 4], LOGIC_K[O_POT] = K_R, [no.K_ROLL, no.K_PITCH, no.K_YAW, no.K_YAW], K_POT
LOGIC_K[O_EPRET] = LOGIC_K[O_EPSUM] = K_R + 1
LOGIC_NAMES = {O_R: "r", O_EULER: "roll", O_EULER + 1: "pitch", O_EULER + 2: "cyaw", O_EULER + 3: "syaw", O_POT: "pot_prev", O_EPRET: "ep_ret",
               O_EPSUM: "ep_ret + ep_lo"}
DYNAMIC = 55                   # the words of the state a step may leave non-finite: base 13, angles 21, rates 21


def logic_view(got):
    """the probe's answer [n, 140] -> float64 [n, 2, 70]: integer words as numbers, and ep_lo's column as the PAIR'S SUM (the tail alone has no
    reference: it is what the head's rounding left)"""
    g = np.ascontiguousarray(got, np.float32).reshape(-1, 2, LOGIC_OWL)
    with np.errstate(invalid="ignore"):
        v = g.astype(np.float64)
    v[:, :, LOGIC_INT] = from_bits(g[:, :, LOGIC_INT])
    v[:, :, O_EPSUM] = v[:, :, O_EPRET] + v[:, :, O_EPSUM]
    return v


def logic_ref(kind, inp, x64=None):
    """-> ref, B, exact [n, 2, 70] (per lane) and the dict of decisions.  B = inf: not judged.  x64: the same rows with their floats
    unrounded (the integer words are read from inp either way)"""
    m = no.model(kind)
    with np.errstate(invalid="ignore"):
        x = inp.astype(np.float64) if x64 is None else np.asarray(x64, np.float64)
    N = x.shape[0]
    pos, quat = x[:, I_POS:I_POS + 3], x[:, I_QUAT:I_QUAT + 4]
    q, qd, act = x[:, I_Q:I_Q + 21], x[:, I_QD:I_QD + 21], x[:, I_ACT:I_ACT + 21]
    foot_i = from_bits(inp[:, [I_FOOT, I_FOOT + 1, I_FOOT + 5, I_FOOT + 6]])
    contact, touch = foot_i[:, [0, 2]], foot_i[:, [1, 3]]
    sole = np.stack([x[:, I_FOOT + 2:I_FOOT + 5], x[:, I_FOOT + 7:I_FOOT + 10] * np.array([1.0, -1.0, 1.0])], 1)      # the left lane's is y-mirrored
    cache = x[:, I_CACHE:I_CACHE + 24].copy()                    # p 9, nrm 9, tilt 6
    head = x[:, I_HEAD:I_HEAD + 6].copy()
    pot_prev, nn_dr, ep_ret, ep_lo = (x[:, I_WORDS + i].copy() for i in range(4))
    wi = from_bits(inp[:, I_WORDS + 4:I_WORDS + 8])
    n, count, elapsed, ctr = (wi[:, i].copy() for i in range(4))
    stub = x[:, I_STUB:I_STUB + 11]
    # 4.3 / 4.4
    elapsed = elapsed + 1
    flags = contact[:, 0] | (contact[:, 1] << 1)
    finite = np.isfinite(x[:, :DYNAMIC]).all(1)
    # joint sums over the robot's 21 joints
    lo, hi = m["range"][:, 0], m["range"][:, 1]
    with np.errstate(invalid="ignore"):
        e_terms = np.abs(act * 0.1 * qd)
        e_sum, a2 = e_terms.sum(1), (act * act).sum(1)
        qn = 2 * (q - 0.5 * (lo + hi)) / (hi - lo)
        B_qn = 2 * (np.abs(q) + np.abs(0.5 * (lo + hi))) / (hi - lo)
        limited = np.abs(qn) > T_QN
        limit_safe = decide(np.abs(qn), B_qn, K_QN, T_QN).all(1) | ~finite
    at_limit = limited.sum(1)
    # 4.5 target logic
    reached = (touch != 0).any(1)
    target_old = cache[:, 3:6].copy()
    count = np.where(reached, count + 1, count)
    first = reached & (count == 1)
    d_sole, B_sole = planar(sole, target_old[:, None, :])
    rho, B_rho = d_sole.min(1), B_sole.max(1)
    with np.errstate(invalid="ignore"):
        step_bonus = np.where(first, 50.0 * np.exp(-rho / 0.25), 0.0)
        B_sb = np.where(first, 50.0 * np.exp(-rho / 0.25) * np.maximum(B_rho / 0.25, 1.0), 0.0)
    adv = reached & (count >= 2) & (n < NUM_STONES - 1)
    n = np.where(adv, n + 1, n)
    count = np.where(adv, 0, count)
    drawn = adv & (n + 1 <= NUM_STONES - 1)
    a_ = adv[:, None]
    shifted = cache.copy()
    for off, w in ((0, 3), (9, 3), (18, 2)):                     # p, nrm, tilt: slots 1, 2 move down, slot 2 keeps the last stone's ...
        shifted[:, off:off + w] = cache[:, off + w:off + 2 * w]
        shifted[:, off + w:off + 2 * w] = cache[:, off + 2 * w:off + 3 * w]
    new_head = np.concatenate([head[:, 2:4], head[:, 4:6], head[:, 4:6]], 1)
    d_ = drawn[:, None]
    for off, w, so in ((0, 3, 0), (9, 3, 3), (18, 2, 6)):        # ... or takes the drawn one
        shifted[:, off + 2 * w:off + 3 * w] = np.where(d_, stub[:, so:so + w], shifted[:, off + 2 * w:off + 3 * w])
    new_head[:, 4:6] = np.where(d_, stub[:, 8:10], new_head[:, 4:6])
    cache = np.where(a_, shifted, cache)
    head_after = np.where(a_, new_head, head)
    nn_dr = np.where(drawn, stub[:, 10], nn_dr)
    ctr_in = ctr.copy()
    ctr = np.where(drawn, (ctr + 1) & 0xffffffff, ctr)
    # 4.6 - 4.9
    s = score(kind, pos, quat, cache[:, :9].reshape(N, 3, 3), target_old, sole, pot_prev, adv.astype(np.int64), n, elapsed, finite, step_bonus,
              B_sb, e_sum, e_terms.sum(1), a2, a2, at_limit.astype(np.float64), limit_safe)
    sref, sB, sexact = _assemble_score(s, finite)
    ref, B, exact = np.zeros((N, 2, LOGIC_OWL)), np.zeros((N, 2, LOGIC_OWL)), np.ones((N, 2, LOGIC_OWL), bool)
    for lane, mm in ((0, 1.0), (1, -1.0)):
        r_, B_, e_ = ref[:, lane], B[:, lane], exact[:, lane]
        r_[:, O_BASE:O_BASE + 13] = x[:, :13]                    # compared word by word in the test (they may be non-finite)
        r_[:, O_FLAGS], r_[:, O_ADV] = flags, adv
        r_[:, O_HD:O_HD + 6] = head_after
        B_[:, O_HD:O_HD + 6] = np.where(a_, 0.0, INF)            # meaningful after an advance only
        r_[:, O_D], B_[:, O_D] = sref[:, 1], sB[:, 1]
        r_[:, O_BAD] = sref[:, 2]
        r_[:, O_R], B_[:, O_R], e_[:, O_R] = sref[:, 3], sB[:, 3], sexact[:, 3]
        r_[:, O_EULER:O_EULER + 4], B_[:, O_EULER:O_EULER + 4], e_[:, O_EULER:O_EULER + 4] = sref[:, 4:8], sB[:, 4:8], sexact[:, 4:8]
        r_[:, O_POT], B_[:, O_POT], e_[:, O_POT] = sref[:, 0], sB[:, 0], False
        r_[:, O_NNDR] = nn_dr
        pair = ep_ret + ep_lo
        with np.errstate(invalid="ignore"):
            B_pair = np.where(s["r_zero"], 0.0, sB[:, 3] + U * (np.abs(ep_ret) + np.abs(ep_lo) + np.abs(sref[:, 3])))
        r_[:, O_EPRET], B_[:, O_EPRET], e_[:, O_EPRET] = np.where(s["r_zero"], ep_ret, pair + sref[:, 3]), B_pair + np.where(s["r_zero"], 0, np.abs(pair)), s["r_zero"]
        r_[:, O_EPSUM], B_[:, O_EPSUM], e_[:, O_EPSUM] = pair + sref[:, 3], B_pair, s["r_zero"]
        r_[:, O_N], r_[:, O_COUNT], r_[:, O_ELAPSED], r_[:, O_CTR] = n, count, elapsed, ctr
        r_[:, O_CACHE:O_CACHE + 24] = cache
        r_[:, O_LDSHEAD:O_LDSHEAD + 6] = head_after * np.array([1.0, mm] * 3)
        r_[:, O_DRAW], r_[:, O_DRAW + 1], r_[:, O_DRAW + 2] = drawn, np.where(drawn, n + 1, 0), np.where(drawn, ctr_in, 0)
        r_[:, O_STORE] = drawn & (lane == 0)
        e_[:, O_D] = s["d_safe"]
        e_[:, O_HD:O_HD + 6] = a_
    exact &= ~np.isinf(B)
    exact[:, :, O_BASE:O_BASE + 13] = False
    B[:, :, O_BASE:O_BASE + 13] = INF
    dec = dict(s, reached=reached, first=first, adv=adv, drawn=drawn, at_limit=at_limit, limit_safe=limit_safe, finite=finite, flags=flags,
               count=count, n=n, step_bonus=step_bonus, e_sum=e_sum, a2=a2, elapsed=elapsed)
    return ref, B, exact, dec


def logic_rows(c, dtype=np.float32):
    """dict of true-world arrays (leading dimension n) -> rows [n, 135] float32 (float64: the floats unrounded, the integer words lost)"""
    n = c["pos"].shape[0]
    x = np.zeros((n, LOGIC_IW), dtype)
    x[:, I_POS:I_POS + 3], x[:, I_QUAT:I_QUAT + 4], x[:, I_W:I_W + 3], x[:, I_V:I_V + 3] = c["pos"], c["quat"], c["w"], c["v"]
    x[:, I_Q:I_Q + 21], x[:, I_QD:I_QD + 21], x[:, I_ACT:I_ACT + 21] = c["q"], c["qd"], c["act"]
    for f in range(2):
        o = I_FOOT + 5 * f
        x[:, o], x[:, o + 1] = as_bits(c["contact"][:, f]), as_bits(c["touch"][:, f])
        x[:, o + 2:o + 5] = c["sole"][:, f] * (np.array([1.0, -1.0, 1.0]) if f else 1.0)
    x[:, I_CACHE:I_CACHE + 9], x[:, I_CACHE + 9:I_CACHE + 18], x[:, I_CACHE + 18:I_CACHE + 24] = c["cp"].reshape(n, 9), c["cn"].reshape(n, 9), c["ct"].reshape(n, 6)
    x[:, I_HEAD:I_HEAD + 6] = c["head"].reshape(n, 6)
    x[:, I_WORDS], x[:, I_WORDS + 1], x[:, I_WORDS + 2], x[:, I_WORDS + 3] = c["pot_prev"], c["nn_dr"], c["ep_ret"], c["ep_lo"]
    for i, key in enumerate(("n", "count", "elapsed", "ctr")):
        x[:, I_WORDS + 4 + i] = as_bits(c[key])
    x[:, I_STUB:I_STUB + 11] = c["stub"]
    return x


def _heading(phi):
    return np.stack([np.cos(phi), np.sin(phi)], -1)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _logic_random(kind, rng, n):
    m = no.model(kind)
    lo, hi = m["range"][:, 0], m["range"][:, 1]
    c = _scene(rng, n)
    c["w"], c["v"] = rng.uniform(-3, 3, (n, 3)), rng.uniform(-2, 2, (n, 3))
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    c["q"] = mid + half * rng.uniform(-0.97, 0.97, (n, 21))
    lim = rng.random((n, 21)) < 0.08                             # beyond 0.99 of the half range, inside or past the end stop
    c["q"] = np.where(lim, mid + half * rng.choice([-1.0, 1.0], (n, 21)) * rng.uniform(1.0, 1.1, (n, 21)), c["q"])
    c["qd"] = rng.uniform(-12, 12, (n, 21))
    c["act"] = np.clip(rng.uniform(-1.4, 1.4, (n, 21)), -1, 1)
    pattern = rng.integers(0, 4, n)                              # on the target: neither, right, left, both
    c["touch"] = np.stack([(pattern == 1) | (pattern == 3), (pattern == 2) | (pattern == 3)], 1).astype(np.int64)
    c["contact"] = c["touch"] | (rng.random((n, 2)) < 0.5)
    c["cn"] = _unit(np.concatenate([rng.uniform(-0.25, 0.25, (n, 3, 2)), np.ones((n, 3, 1))], 2))
    c["ct"] = rng.uniform(-no.TILT, no.TILT, (n, 3, 2))
    c["head"] = _heading(rng.uniform(-np.pi, np.pi, (n, 3)))
    c["nn_dr"] = rng.uniform(0.65, 1.25, n)
    hi_ = f32(rng.uniform(-300, 900, n))
    c["ep_ret"], c["ep_lo"] = hi_, f32(rng.uniform(-0.49, 0.49, n) * np.spacing(np.abs(hi_)))
    c["count"] = rng.choice([0, 1, 2, 5], n)
    c["ctr"] = rng.integers(0, 2 ** 32, n)
    bad = rng.random(n) < 0.04                                   # a state the substeps left non-finite
    word = rng.integers(0, DYNAMIC, n)
    val = rng.choice([np.nan, INF, -INF], n)
    state = np.concatenate([c["pos"], c["quat"], c["w"], c["v"], c["q"], c["qd"]], 1)
    state[bad, word[bad]] = val[bad]
    c["pos"], c["quat"], c["w"], c["v"], c["q"], c["qd"] = np.split(state, [3, 7, 10, 13, 34], 1)
    c["stub"] = np.concatenate([rng.uniform(-3, 3, (n, 2)), rng.uniform(-0.3, 0.3, (n, 1)), _unit(np.concatenate([rng.uniform(-0.25, 0.25, (n, 2)), np.ones((n, 1))], 1)),
                                rng.uniform(-no.TILT, no.TILT, (n, 2)), _heading(rng.uniform(-np.pi, np.pi, n)), rng.uniform(0.65, 1.25, (n, 1))], 1)
    return c


def _base_case(kind):
    """one quiet robot: standing, no contact with the target, nothing near a threshold"""
    m = no.model(kind)
    lo, hi = m["range"][:, 0], m["range"][:, 1]
    rng = _rng("base case", kind)
    c = dict(pos=np.array([[0.1, 0.05, 1.3]]), quat=quat_of(np.float64(0.05), np.float64(0.1), np.float64(0.3))[None], w=np.array([[0.1, -0.2, 0.3]]),
             v=np.array([[0.5, 0.1, -0.1]]), q=(0.5 * (lo + hi) + 0.2 * (hi - lo) * rng.uniform(-1, 1, 21))[None], qd=rng.uniform(-3, 3, (1, 21)),
             act=rng.uniform(-0.9, 0.9, (1, 21)), contact=np.array([[1, 1]]), touch=np.array([[0, 0]]),
             sole=np.array([[[0.6, -0.1, 0.02], [0.45, 0.12, 0.01]]]), cp=np.array([[[-0.25, 0.0, 0.0], [0.5, 0.05, 0.02], [1.25, -0.1, -0.05]]]),
             cn=_unit(np.array([[[0.05, 0.02, 1.0], [-0.1, 0.04, 1.0], [0.02, -0.07, 1.0]]])), ct=np.array([[[0.01, 0.02], [-0.03, 0.04], [0.05, -0.06]]]),
             head=_heading(np.array([[0.1, -0.4, 0.7]])), pot_prev=np.array([-25.0]), nn_dr=np.array([0.8]), ep_ret=f32([37.25]).astype(np.float64),
             ep_lo=f32([1.0e-6]).astype(np.float64), n=np.array([5]), count=np.array([0]), elapsed=np.array([10]), ctr=np.array([4000000000]),
             stub=np.array([[2.0, 0.3, 0.1, 0.06, -0.08, 0.995, 0.11, -0.12, np.cos(1.1), np.sin(1.1), 0.9]]))
    c["stub"][0, 3:6] = _unit(c["stub"][0, 3:6])
    return c


def _with(c, **kw):
    o = {k: np.array(v, copy=True) for k, v in c.items()}
    for k, v in kw.items():
        o[k] = np.asarray(v).reshape(o[k].shape) if np.ndim(v) else np.full(o[k].shape, v, o[k].dtype if o[k].dtype.kind == "i" else np.float64)
    return o


def _stack(cases):
    return {k: np.concatenate([c[k] for c in cases]) for k in cases[0]}


@functools.lru_cache(maxsize=None)
def logic_prepared(kind):
    """rows, reference and edges of the `step_logic` op.  edges: name -> (row, dict of stated outcomes)"""
    m = no.model(kind)
    lo, hi = m["range"][:, 0], m["range"][:, 1]
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    rng = _rng("step_logic", kind)
    cases, edges = [_logic_random(kind, rng, N_RANDOM)], {}
    e0 = N_RANDOM
    base = _base_case(kind)

    def add(name, expect, **kw):
        nonlocal e0
        cases.append(_with(base, **kw))
        edges[name] = (e0, expect)
        e0 += 1

    add("quiet", dict(d=0, bad=0, advanced=0, calls=0, count=0, n=5, flags=3, elapsed=11))
    h = F32(T_HEIGHT)
    zs = float(min(base["sole"][0, 0, 2], base["sole"][0, 1, 2]))
    for name, hh, tall in (("- ulp", np.nextafter(h, F32(0)), 0), ("", h, 0), (" + ulp", np.nextafter(h, F32(1)), 1)):
        # soles at z = 0 exactly: the height is pos z, one exact subtraction; the stones 5 m below
        add("height 0.7" + name, dict(d=1 - tall, tall=tall), pos=[0.1, 0.05, float(hh)], sole=[[[0.6, -0.1, 0.0], [0.45, 0.12, 0.25]]],
            cp=base["cp"] - np.array([0, 0, 5.0]))
    t = F32(T_LOW)
    for slot in range(3):
        for name, z, low in (("below", np.nextafter(t, F32(0)), 1), ("at", t, 0), ("above", np.nextafter(t, F32(1)), 0)):
            cp = base["cp"].copy()
            cp[0, :, 2] = 0.25
            cp[0, slot, 2] = 0.0
            add("low stone in slot %d: %s zlow + 0.3" % (slot, name), dict(d=low, low=low), pos=[0.1, 0.05, float(z)], cp=cp,
                sole=[[[0.6, -0.1, -0.9], [0.45, 0.12, -0.8]]])
    for nn, bonus in ((19, 1), (18, 0)):
        for dx, inside in ((0.1499, 1), (0.1501, 0)):
            cp = np.array([[[-0.75, 0, 0], [0.0, 0, 0], [0.75, 0, 0]]], np.float64)
            add("target bonus: n = %d, distance %.4f" % (nn, dx), dict(target=bonus * inside, advanced=0), pos=[dx, 0.0, 1.3], cp=cp, n=nn)
    for name, roll, pitch, po, ro in (("pitch below -0.2", 0, -0.2001, 1, 0), ("pitch above -0.2", 0, -0.1999, 0, 0), ("pitch below 0.4", 0, 0.3999, 0, 0),
                                      ("pitch above 0.4", 0, 0.4001, 1, 0), ("roll below -0.4", -0.4001, 0.1, 0, 1), ("roll above -0.4", -0.3999, 0.1, 0, 0),
                                      ("roll below 0.4", 0.3999, 0.1, 0, 0), ("roll above 0.4", 0.4001, 0.1, 0, 1)):
        add("posture: " + name, dict(pitch_out=po, roll_out=ro), quat=quat_of(np.float64(roll), np.float64(pitch), np.float64(0.3)))
    fallen = [[[0.6, -0.1, 0.9], [0.45, 0.12, 0.8]]]
    for el in (998, 999, 1000):
        add("time limit: elapsed %d, standing" % el, dict(d=int(el >= 999), bad=int(el >= 999), elapsed=el + 1), elapsed=el)
        add("time limit: elapsed %d, fallen" % el, dict(d=1, bad=int(el >= 999), elapsed=el + 1), elapsed=el, sole=fallen)
    state0 = np.concatenate([base[k] for k in ("pos", "quat", "w", "v", "q", "qd")], 1)
    for wd in range(DYNAMIC):
        for val in (np.nan, INF, -INF):
            st = state0.copy()
            st[0, wd] = val
            parts = np.split(st, [3, 7, 10, 13, 34], 1)
            add("non-finite state: word %d = %r" % (wd, val), dict(d=1, r=0.0, pair_unchanged=1), **dict(zip(("pos", "quat", "w", "v", "q", "qd"), parts)))
    for val in (INF, -INF):
        add("non-finite reward: pot_prev %r" % val, dict(r=0.0, d=0, pair_unchanged=1), pot_prev=val)
    # contact count: the soles at different distances from the target, the left one nearer
    near = np.array([[[0.9, -0.1, 0.02], [0.55, 0.1, 0.01]]])
    for cnt in (0, 1, 5):
        for pname, touch in (("right", [1, 0]), ("left", [0, 1]), ("both", [1, 1]), ("neither", [0, 0])):
            reached = int(any(touch))
            exp = dict(first=int(reached and cnt == 0), advanced=int(reached and cnt >= 1), count=(cnt + 1 if cnt == 0 else 0) if reached else cnt,
                       n=5 + int(reached and cnt >= 1), calls=int(reached and cnt >= 1))
            if exp["first"]:
                exp["rho"] = float(np.hypot(*(f32(near[0, 1, :2]).astype(np.float64) - f32(base["cp"][0, 1, :2]).astype(np.float64))))
            add("contact count %d, on target: %s" % (cnt, pname), exp, count=cnt, touch=[touch], contact=[touch], sole=near)
    add("last stones: n = 18 advances to 19", dict(advanced=1, n=19, count=0, calls=0, keeps_slot2=1), n=18, count=1, touch=[[1, 0]])
    add("last stones: n = 19", dict(advanced=0, n=19, count=4, calls=0), n=19, count=3, touch=[[0, 1]])
    add("advance with a draw", dict(advanced=1, n=6, count=0, calls=1, k=7, draw_ctr=4000000000, ctr=4000000001, stores=(1, 0), drawn=1),
        n=5, count=1, touch=[[1, 1]])
    add("advance with a draw: the counter wraps", dict(advanced=1, calls=1, k=3, draw_ctr=2 ** 32 - 1, ctr=0), n=1, count=2, touch=[[0, 1]], ctr=2 ** 32 - 1)
    # joint counts: one group alone at its limit / alone actuated; every other joint at its mid-range, unactuated
    quiet_q, zero = mid[None].copy(), np.zeros((1, 21))
    for gname, joints in (("spine", [0, 1, 2]), ("right-only joint", [5]), ("left-only joint", [10])):
        qq = quiet_q.copy()
        qq[0, joints] = mid[joints] + 0.995 * half[joints]
        add("joint counts: %s at its limit" % gname, dict(at_limit=len(joints)), q=qq, act=zero)
        aa = zero.copy()
        aa[0, joints] = 0.75
        add("joint counts: %s actuated" % gname, dict(at_limit=0, a2=0.5625 * len(joints)), q=quiet_q, act=aa)
    order = _rng("limit order", kind).permutation(21)
    for k in range(22):
        qq = quiet_q.copy()
        j = order[:k]
        qq[0, j] = mid[j] + half[j] * np.where(np.arange(k) % 2 == 0, 0.995, -1.02)
        add("joint counts: at_limit %d" % k, dict(at_limit=k), q=qq)
    c = _stack(cases)
    x = logic_rows(c)
    if x.shape[0] % 32 == 0:
        x = np.concatenate([x, x[:1]])
    assert x.shape[0] % 32 != 0          # robots: the device's last wavefront is partial
    ref, B, exact, dec = logic_ref(kind, x)
    return no._frozen(dict(inp=x, ref=ref, B=B, exact=exact, dec=no._frozen(dict(dec)), edges=edges, n_random=N_RANDOM))


def judge(got, ref, B, exact, k):
    """np_contact_ops.judge_cols, with the components the reference leaves out (B = inf) taken out first: the kernel may hold anything
    there, a NaN included"""
    out = np.isinf(B)
    got = np.where(out, 0.0, got)
    ref = np.where(out, 0.0, ref)
    return no.judge_cols(got, ref, np.where(out, 1.0, B), exact & ~out, k), int(out.sum())


def same_words(got, want):
    """float32 arrays agree word by word: equal, or both NaN"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return (got == want) | (np.isnan(got) & np.isnan(want))


def fsum_check(r, T, every=97):
    """the carried sums against math.fsum on a sample of (sequence, step) -> worst |T - fsum|"""
    worst = 0.0
    for e in range(0, r.shape[0], every):
        for t in (0, 1, 99, 100, 499, r.shape[1] - 1):
            worst = max(worst, abs(T[e, t] - math.fsum(float(v) for v in r[e, :t + 1])))
    return worst
