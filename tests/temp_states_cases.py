"""Cases, fp64 reference and tolerances for create_temp_states and get_obs (docs/PHYSICS.md 5 and 8; temp_states_kernel in
steppingstone_amd/csrc/ss_api.hip, obs_kernel / write_obs / target_features / place_stone in ss_kernels.hpp).  Used by
tests/test_temp_states_cases.py (CPU: the reference alone), tests/test_gpu_temp_states.py (the kernels) and
tests/test_oracle_env_numpy.py.  TEST INFRASTRUCTURE ONLY; no test in it.

reference(kind, row): fp64 [121, 60] from the packed row as the GPU holds it (its fp32 words): the observation of np_env.observation, and
per grid cell (i, j), row i * 11 + j, the second target block of stone n + 1 re-placed from stone n at heading phi_n + yaw_samples[i],
pitch_samples[j], the step length nn_dr and its own tilts; at n == 19 nothing is re-placed and all 121 rows are the observation.  The
target blocks are written as PHYSICS.md 5 states them (atan2 / sin / cos of the bearing); the kernels rotate the planar offset.

cases(kind): 76 synthetic packed rows, four per n in 1..19, built without any physics: see cases().

Tolerance per word: |got - ref| <= K * 2^-24 * B, B the reference's running absolute-value bound of that word, K counted on the kernel's
source by the rules of tests/np_contact_ops.py (an input carries no rounding, a table constant one; k(x + y) = max + 1, k(x * y) = sum + 1,
k(f(x)) = k(x) + k_f with B = max(|f'| B(x), |f|); library calls by the OpenCL full-profile limits np_contact_ops takes for the sampler and
the observation terms: K_SINCOS, K_ASIN, K_ATAN2; SS_RSQRT two).  Nothing is fitted to a kernel's output.  The counts:

  write_obs (k of the pieces as np_contact_ops.OBS_K counts them: roll 15, pitch 10, cos / sin of the yaw 14, joint angle 4, joint rate 2)
    obs[0]     z - z_init                                                                                               1
    R = quat_rot(quat): 1 - 2 (yy + zz): products 1, sum 2, 1 - : 3;  vw[r] = R[r] . v: products 3 + 0 + 1 = 4, two additions    6
    obs[1, 2]  cy vw0 + sy vw1: products 14 + 6 + 1 = 21, the sum                                                      22
    obs[3]     vw[2]                                                                                                    6
    obs[4, 5]  roll, pitch                                                                                         15, 10
    obs[6:27], obs[27:48]  obs_angle, obs_rate                                                                       4, 2
    obs[48:50] contact flags: exact
    obs[50:55] target_features of stone n (its centre a copy of the terrain row): dx = sp - pos: 1; dy cy: 1 + 14 + 1 = 16, the
               difference 17;  dz: 1;  tilts: copies, exact                                                     17, 17, 1, 0, 0
  temp_states_kernel, n <= 18
    yaw_sample, pitch_sample: 2;  phi = phi_n + yaw_sample: 3, B = |phi_n| + |yaw_sample|
    sincosf(pitch): 2 + K_SINCOS = 10;  sincosf(phi): 3 + K_SINCOS = 11
    place_stone: planar = dr cp: 0 + 10 + 1 = 11;  planar cph: 11 + 11 + 1 = 23;  px + : 24;  dr sp: 11;  pz + : 12
    target_features: dx = p2 - pos: 25;  dy cy: 25 + 14 + 1 = 40, the difference 41;  dz: 13;  tilts: copies  41, 41, 13, 0, 0
  temp_states_kernel, n == 19: target_features of the cached stone 19                                         17, 17, 1, 0, 0
A clipped word (clip5) is 1-Lipschitz in its argument, so it keeps the argument's tolerance."""
import functools

import numpy as np

import np_contact as npc
import np_contact_ops as no
import np_dynamics as npd
import np_env
import np_terrain as npt
import oracle_lib as ol

KINDS = ["walker3d", "mike"]
U = no.U
NCELL, GRID, OBS = 121, 11, 60
PER_N = 4
N_CASES = 19 * PER_N                     # 76: more than one wavefront, not a multiple of 64

K_YAW, K_ROLL, K_PITCH, K_OA, K_OR = no.K_YAW, no.K_ROLL, no.K_PITCH, no.K_OA, no.K_OR
K_Z, K_VW = 1, 6
K_VXY = K_YAW + K_VW + 1 + 1             # 22
K_TF_XY, K_TF_Z = 1 + K_YAW + 1 + 1, 1   # 17, 1
K_CP, K_CPH = no.K_ANGLE_SAMPLE + no.K_SINCOS, no.K_ANGLE_SAMPLE + 1 + no.K_SINCOS    # 10, 11
K_P2_XY, K_P2_Z = (K_CP + 1) + K_CPH + 1 + 1, (K_CP + 1) + 1                          # 24, 12
K_TEMP_XY, K_TEMP_Z = (K_P2_XY + 1) + K_YAW + 1 + 1, K_P2_Z + 1                       # 41, 13
K_OBS = np.array([K_Z, K_VXY, K_VXY, K_VW, K_ROLL, K_PITCH] + [K_OA] * 21 + [K_OR] * 21 + [0, 0] +
                 [K_TF_XY, K_TF_XY, K_TF_Z, 0, 0] * 2, np.float64)
K_TEMP = np.array([K_TEMP_XY, K_TEMP_XY, K_TEMP_Z, 0, 0], np.float64)
assert (K_VXY, K_TF_XY, K_CP, K_CPH, K_P2_XY, K_P2_Z, K_TEMP_XY, K_TEMP_Z) == (22, 17, 10, 11, 24, 12, 41, 13)

GROUPS = {"height": slice(0, 1), "velocity": slice(1, 4), "roll, pitch": slice(4, 6), "joint angles": slice(6, 27),
          "joint rates": slice(27, 48), "flags": slice(48, 50), "target n": slice(50, 55), "look-ahead": slice(55, 60)}
MUTATIONS = ("phi_n := 0", "tilts of stone n", "grid indices swapped", "dr := 0.75", "p1 := stone n-1", "yaw negated")


@functools.lru_cache(maxsize=None)
def model(kind):
    return npc.rounded_model(kind)


def _parts(row):
    st = np.asarray(row, np.float64)
    return st, int(st[ol.S_N]), int(st[ol.S_FLAGS]), st[ol.S_TERRAIN].reshape(20, 6)


def _target_block(pos, yaw, centre, tilts):
    """PHYSICS.md 5's target block for stone centres [..., 3]: [sin(dtheta) d, cos(dtheta) d, dz, x_tilt, y_tilt]"""
    d = centre - pos
    dist = np.hypot(d[..., 0], d[..., 1])
    dth = np.arctan2(d[..., 1], d[..., 0]) - yaw
    tl = np.broadcast_to(tilts, d.shape[:-1] + (2,))
    return np.stack([np.sin(dth) * dist, np.cos(dth) * dist, d[..., 2], tl[..., 0], tl[..., 1]], -1)


def replaced_stones(row, mutate=None):
    """centres [121, 3] of stone n + 1 re-placed at every grid cell (row i * 11 + j), and the tilts [2] it keeps (n <= 18)"""
    st, n, _, terrain = _parts(row)
    i, j = np.divmod(np.arange(NCELL), GRID)
    if mutate == "grid indices swapped":
        i, j = j, i
    phi = (0.0 if mutate == "phi_n := 0" else terrain[n][3]) + npt.YAW[i]
    pitch = npt.PITCH[j]
    dr = 0.75 if mutate == "dr := 0.75" else st[ol.S_NNDR]
    p1 = terrain[n - 1 if mutate == "p1 := stone n-1" else n][:3]
    step = np.stack([np.cos(pitch) * np.cos(phi), np.cos(pitch) * np.sin(phi), np.sin(pitch)], -1)
    return p1 + dr * step, terrain[n if mutate == "tilts of stone n" else n + 1][4:6]


def observation(kind, row):
    """fp64 [60]: get_obs of the row (np_env.observation)"""
    st, n, flags, _ = _parts(row)
    return np_env.observation(model(kind), st, flags, n)


def reference(kind, row, mutate=None):
    """fp64 [121, 60].  mutate: None, or one of MUTATIONS -- a wrong kernel restated, for the power test only."""
    assert mutate is None or mutate in MUTATIONS
    st, n, flags, _ = _parts(row)
    out = np.tile(observation(kind, row), (NCELL, 1))
    if n >= 19:
        return out
    _, _, yaw = np_env.euler_from_matrix(npd.quat_rot(st[ol.S_QUAT]))
    centres, tilts = replaced_stones(row, mutate)
    out[:, 55:60] = _target_block(st[ol.S_POS], -yaw if mutate == "yaw negated" else yaw, centres, tilts)
    return out


def bounds(kind, rows):
    """(B [n, 60] of observation(), B [n, 121, 60] of reference()) for packed rows [n, 186]: the running absolute-value bound of every word"""
    x = np.asarray(rows, np.float64)
    nr = x.shape[0]
    n = x[:, ol.S_N].astype(np.int64)
    terr = x[:, ol.S_TERRAIN].reshape(nr, 20, 6)
    e = np.arange(nr)
    pos, quat, v = x[:, ol.S_POS], x[:, ol.S_QUAT], x[:, 10:13]
    # roll, pitch, cos / sin of the yaw and the joint entries: the bounds the observation-term op is judged with
    inp = np.zeros((nr, 81))
    inp[:, 0:4], inp[:, 15:36], inp[:, 36:57] = quat, x[:, ol.S_Q], x[:, ol.S_QD]
    _, Bo, _, _, _ = no.obs_ref(kind, inp.astype(np.float32))
    Bcy, Bsy = Bo[:, 2], Bo[:, 3]
    w, qx, qy, qz = np.abs(quat).T
    BR = np.stack([np.stack([1 + 2 * (qy * qy + qz * qz), 2 * (qx * qy + w * qz), 2 * (qx * qz + w * qy)], -1),
                   np.stack([2 * (qx * qy + w * qz), 1 + 2 * (qx * qx + qz * qz), 2 * (qy * qz + w * qx)], -1),
                   np.stack([2 * (qx * qz + w * qy), 2 * (qy * qz + w * qx), 1 + 2 * (qx * qx + qy * qy)], -1)], 1)
    Bvw = np.einsum("nrc,nc->nr", BR, np.abs(v))
    B = np.zeros((nr, OBS))
    B[:, 0] = np.abs(pos[:, 2]) + np.abs(x[:, ol.S_ZINIT])
    B[:, 1], B[:, 2], B[:, 3] = Bcy * Bvw[:, 0] + Bsy * Bvw[:, 1], Bsy * Bvw[:, 0] + Bcy * Bvw[:, 1], Bvw[:, 2]
    B[:, 4], B[:, 5] = Bo[:, 0], Bo[:, 1]
    B[:, 6:27], B[:, 27:48] = Bo[:, 11:32], Bo[:, 32:53]
    B[:, 48:50] = 1.0

    def block(Bc, tilts):
        """bound of target_features for stone-centre bounds Bc [..., 3]"""
        d = Bc + np.abs(pos).reshape((nr,) + (1,) * (Bc.ndim - 2) + (3,))
        cy, sy = Bcy.reshape((nr,) + (1,) * (Bc.ndim - 2)), Bsy.reshape((nr,) + (1,) * (Bc.ndim - 2))
        tl = np.broadcast_to(np.abs(tilts).reshape((nr,) + (1,) * (Bc.ndim - 2) + (2,)), Bc.shape[:-1] + (2,))
        return np.stack([d[..., 1] * cy + d[..., 0] * sy, d[..., 0] * cy + d[..., 1] * sy, d[..., 2], tl[..., 0], tl[..., 1]], -1)
    nxt = np.minimum(n + 1, 19)
    B[:, 50:55] = block(np.abs(terr[e, n, :3]), terr[e, n, 4:6])
    B[:, 55:60] = block(np.abs(terr[e, nxt, :3]), terr[e, nxt, 4:6])
    out = np.repeat(B[:, None, :], NCELL, 1)
    i, j = np.divmod(np.arange(NCELL), GRID)
    phi_n, dr = terr[e, n, 3], x[:, ol.S_NNDR]
    phi, Bphi = phi_n[:, None] + npt.YAW[i], np.abs(phi_n)[:, None] + np.abs(npt.YAW[i])
    pitch = np.broadcast_to(npt.PITCH[j], phi.shape)
    Bcp, Bsp = np.maximum(np.abs(np.sin(pitch) * pitch), np.abs(np.cos(pitch))), np.maximum(np.abs(np.cos(pitch) * pitch), np.abs(np.sin(pitch)))
    Bcph, Bsph = np.maximum(np.abs(np.sin(phi)) * Bphi, np.abs(np.cos(phi))), np.maximum(np.abs(np.cos(phi)) * Bphi, np.abs(np.sin(phi)))
    p1 = np.abs(terr[e, n, :3])[:, None, :]
    Bp2 = p1 + dr[:, None, None] * np.stack([Bcp * Bcph, Bcp * Bsph, Bsp], -1)
    moved = n <= 18
    out[moved, :, 55:60] = block(Bp2, terr[e, nxt, 4:6])[moved]
    return B, out


def tolerance(kind, rows):
    """K 2^-24 B: ([n, 60] for observation(), [n, 121, 60] for reference())"""
    x = np.asarray(rows, np.float64)
    K = np.tile(K_OBS, (x.shape[0], NCELL, 1))
    K[x[:, ol.S_N] <= 18, :, 55:60] = K_TEMP
    B_obs, B_temp = bounds(kind, rows)
    return K_OBS * U * B_obs, K * U * B_temp


def judged(kind, rows):
    """dict(obs, obs_tol [n, 60], temp, temp_tol [n, 121, 60]): references and tolerances of packed rows [n, 186]"""
    obs_tol, temp_tol = tolerance(kind, rows)
    out = dict(obs=np.stack([observation(kind, r) for r in rows]), obs_tol=obs_tol, temp=np.stack([reference(kind, r) for r in rows]),
               temp_tol=temp_tol)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def references(kind):
    """judged() of cases(kind): computed once, shared by the tests, never changed"""
    return judged(kind, cases(kind))


def ratios(got, ref, tol):
    """|got - ref| / tol, 0 where both vanish and inf where only the tolerance does (an exact word that differs)"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))


def worst_by_group(got, ref, tol):
    r = ratios(got, ref, tol)
    return {g: float(r[..., s].max()) for g, s in GROUPS.items()}


def judge(got, ref, tol, label):
    """prints the worst got / bound ratio per word group, then asserts every word within its tolerance"""
    worst = worst_by_group(got, ref, tol)
    print("%s: worst |got - ref| / (K 2^-24 B) per group: %s" % (label, {g: float("%.3g" % w) for g, w in worst.items()}))
    r = ratios(got, ref, tol)
    assert (r <= 1.0).all(), "%s: words outside their tolerance, first at %s; per group %s" % (label, np.argwhere(~(r <= 1.0))[:5].tolist(), worst)
    return worst


def heading(row):
    """(n, phi_n, yaw of the torso) of a packed row"""
    st, n, _, terrain = _parts(row)
    return n, float(terrain[n][3]), float(np_env.euler_from_matrix(npd.quat_rot(st[ol.S_QUAT]))[2])


def _quat(yaw, pitch, roll):
    """unit quaternion (w, x, y, z) of Rz(yaw) Ry(pitch) Rx(roll)"""
    cy, sy, cp, sp, cr, sr = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(roll / 2), np.sin(roll / 2)
    return np.array([cy * cp * cr + sy * sp * sr, cy * cp * sr - sy * sp * cr, cy * sp * cr + sy * cp * sr, sy * cp * cr - cy * sp * sr])


@functools.lru_cache(maxsize=None)
def cases(kind):
    """76 packed rows [76, 186] float32, four per n in 1..19 (row 4 (n - 1) + c), built directly:
      terrain  a walk of 20 stones from the origin: heading steps of a per-case drift (0.1 to 0.3 rad, either sign) plus up to 0.15 rad, so
               that the accumulated heading passes +-pi/2; pitch within +-0.35; step lengths in [0.65, 1.25]; tilts within +-0.26
      torso    within 0.4 m (planar) of stone n - 1 and 0.9 to 1.3 m above it; yaw over (-pi, pi] with |sin yaw| >= 0.05 (a mirrored
               yaw must show), roll and pitch within +-0.5; twist within +-2
      nn_dr    in [0.65, 1.25], at least 0.03 from 0.75 (a step length taken from the wrong place must show)
      joints   angles inside their ranges, rates up to +-60 (obs[27:48] reaches the +-5 clip from 50 on)
      flags    c: all four values at every n;  count, elapsed and the Philox counter words arbitrary but valid."""
    rng = np.random.default_rng([KINDS.index(kind), 8121])
    m = model(kind)
    lo, hi = m["range"][:, 0], m["range"][:, 1]
    rows = np.zeros((N_CASES, ol.STATE_DIM))
    for n in range(1, 20):
        for c in range(PER_N):
            st = rows[PER_N * (n - 1) + c]
            terr = np.zeros((20, 6))
            drift = rng.uniform(0.1, 0.3) * (1 if rng.uniform() < 0.5 else -1)
            for k in range(1, 20):
                phi = terr[k - 1, 3] + drift + rng.uniform(-0.15, 0.15)
                pitch, dr = rng.uniform(-0.35, 0.35), rng.uniform(0.65, 1.25)
                terr[k, :3] = terr[k - 1, :3] + dr * np.array([np.cos(pitch) * np.cos(phi), np.cos(pitch) * np.sin(phi), np.sin(pitch)])
                terr[k, 3] = phi
            terr[:, 4:6] = rng.uniform(-0.26, 0.26, (20, 2))
            rad, ang = 0.4 * np.sqrt(rng.uniform()), rng.uniform(-np.pi, np.pi)
            st[ol.S_POS] = terr[n - 1, :3] + [rad * np.cos(ang), rad * np.sin(ang), rng.uniform(0.9, 1.3)]
            yaw = rng.uniform(0.05, np.pi - 0.05) * (1 if rng.uniform() < 0.5 else -1)
            st[ol.S_QUAT] = _quat(yaw, rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5))
            st[ol.S_VEL] = rng.uniform(-2, 2, 6)
            st[ol.S_Q] = lo + rng.uniform(0.02, 0.98, 21) * (hi - lo)
            st[ol.S_QD] = rng.uniform(-60, 60, 21)
            st[ol.S_POT] = -np.hypot(*(terr[n, :2] - st[0:2])) * 60.0
            st[ol.S_ZINIT] = rng.uniform(1.0, 1.3)
            st[ol.S_EPRET] = rng.uniform(-5, 40)
            dr = rng.uniform(0.65, 1.19)
            st[ol.S_NNDR] = dr if dr < 0.72 else dr + 0.06
            st[ol.S_N], st[ol.S_COUNT], st[ol.S_ELAPSED] = n, rng.integers(0, 2), rng.integers(0, 990)
            st[ol.S_CTRLO], st[ol.S_CTRHI] = rng.integers(0, 65536), rng.integers(0, 16)
            st[ol.S_FLAGS] = c
            st[ol.S_TERRAIN] = terr.reshape(120)
    out = rows.astype(np.float32)
    out.setflags(write=False)
    return out
