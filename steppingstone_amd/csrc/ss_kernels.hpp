// ss_kernels.hpp -- environment logic around the physics substep: control step, reward, termination,
// auto-reset, terrain sampler, observation assembly (docs/PHYSICS.md sections 4-8).
//
// HBM layout (structure of arrays, env index fastest so every field access of a wavefront is one coalesced
// 256-byte transaction):
//   fstate [NF][Npad] float : pos3 quat4 twist6 q21 qd21 pot z_init ep_ret nn_dr | 3 active stones x 8 | 3 x (cos, sin) of their headings | ep_ret_lo
//   istate [NI][Npad] int   : next_step_index, target_reached_count, elapsed, rng_ctr, flags, prov_from
//   terrain [20*6][Npad] float : terrain_info rows of the stones k < prov_from; the stones from prov_from on are the provisional
//                                straight flat path (x = 0.75 k, everything else 0; PHYSICS.md 6) BY DEFINITION and their rows are
//                                not written: a reset sets prov_from = 0 instead of storing 120 words that are scattered over 120
//                                rows -- at the benchmark's reset rate that was 1.0 MB of sector writes plus 1.2 MB of fill reads
//                                per 4096-env step, a third of the launch's HBM traffic (round 3).  Touched on stone advance,
//                                get_state / set_state and by create_temp_states only.
//   prob   [121] float shared grid, or [121][Npad] per-env grids
#pragma once
#include <cstdlib>

#include "ss_dynamics.hpp"
#include "../../include/steppingstone.h"

namespace ss {

enum { F_POS = 0, F_QUAT = 3, F_VEL = 7, F_Q = 13, F_QD = 34, F_POT = 55, F_ZINIT = 56, F_EPRET = 57, F_NNDR = 58,
       F_STONE = 59, F_HEAD = 59 + 24, F_EPRET_LO = 59 + 30, NF = 59 + 30 + 1 };
enum { I_N = 0, I_COUNT = 1, I_ELAPSED = 2, I_RNG = 3, I_FLAGS = 4, I_PROV = 5, NI = 6 };
constexpr int kNumStones = 20;
constexpr int kNumSubsteps = 4;        // per control step (PHYSICS.md 1: 1/60 s = 4 x 1/240 s)
constexpr float kDeg = 0.017453292519943295f;

// What the hooks (update_curriculum / update_specialist / update_sample_prob / set_robot_params / auto-reset switch)
// change between steps.  It lives in HBM and the kernels read it through Params::knobs, so a hipGraph that captured
// step launches sees every later update (a by-value kernel argument would be frozen at capture time).
struct Knobs {
  const float* prob;     // shared [121] or per-env [121][Npad]
  int per_env_prob;
  int curriculum;
  float power;
  int auto_reset;
};

struct Params {
  float* fstate;
  int* istate;
  float* terrain;
  const Knobs* knobs;    // device-resident (host harness: host memory)
  int n;                 // number of envs
  int npad;              // padded to a multiple of 64
  uint32_t seed_lo, seed_hi;
  uint32_t env_offset;
  uint32_t id_mask;      // global env id = env_offset + (e & id_mask): all ones, except under ss_debug_set_id_mask (duplicate-env self-check)
  unsigned long long* prof;   // 16 phase counters, tuning builds (-DSS_PROFILE_PHASES) only
};

using Cache = Stones;    // active stones n-1, n, n+1: centre, normal, tilts (ss_dynamics.hpp)

struct Dyn {             // full-robot dynamic state, true world (reset / obs / temp-state kernels)
  float pos[3];
  float quat[4];
  SV v0;                 // base twist, body coordinates
  float q[NJ];
  float qd[NJ];
};

// Sampling grid of a curriculum level c (ring = false: the cells within c of the centre cell, Chebyshev distance) or of a
// specialist level (ring = true: the cells at exactly c), uniform over those cells (PHYSICS.md 8).  Host side.
inline void window_prob(float* p, int c, bool ring) {
  int cnt = 0;
  for (int i = 0; i < SS_GRID; ++i)
    for (int j = 0; j < SS_GRID; ++j) {
      int di = std::abs(i - 5), dj = std::abs(j - 5), m = di > dj ? di : dj;
      bool in = ring ? (m == c) : (m <= c);
      p[i * SS_GRID + j] = in ? 1.f : 0.f;
      cnt += in;
    }
  for (int k = 0; k < SS_NCELL; ++k) p[k] = p[k] / (float)cnt;
}

SSD float yaw_sample(int i) { return (-20.0f + 4.0f * (float)i) * kDeg; }
SSD float pitch_sample(int j) { return (-30.0f + 6.0f * (float)j) * kDeg; }

SSD void stone_normal(float phi, float xt, float yt, float n[3]) {
  float sx, cx, sy, cy, sp, cp;
  sincosf(xt, &sx, &cx);
  sincosf(yt, &sy, &cy);
  sincosf(phi, &sp, &cp);
  float x1 = sy * cx, y1 = -sx, z1 = cy * cx;
  n[0] = cp * x1 - sp * y1;
  n[1] = sp * x1 + cp * y1;
  n[2] = z1;
}

SSD void env_block(const Params& P, int e, uint32_t& ctr, uint32_t out[4]) {
  philox4x32_10(ctr, 0u, P.env_offset + ((uint32_t)e & P.id_mask), 0u, P.seed_lo, P.seed_hi, out);
  ctr += 1u;
}

SSD int sample_cell(const Params& P, const Knobs& K, int e, float u) {
  float cdf = 0.f;
  int last = 0, pick = -1;
  const float* pr = K.per_env_prob ? K.prob + e : K.prob;
  const int stride = K.per_env_prob ? P.npad : 1;
#pragma unroll 1
  for (int k = 0; k < SS_NCELL; ++k) {
    float pk = pr[(size_t)k * stride];
    if (pk > 0.f) last = k;
    cdf += pk;
    if (pick < 0 && u < cdf) pick = k;
  }
  return pick < 0 ? last : pick;
}

// centre of a stone dr away from its predecessor at p, in the direction (phi, pitch) given by their cos / sin (PHYSICS.md 6)
SSD void place_stone(float px, float py, float pz, float dr, float cp, float sp, float cph, float sph, float out_p[3]) {
  float planar = dr * cp;
  out_p[0] = px + planar * cph;
  out_p[1] = py + planar * sph;
  out_p[2] = pz + dr * sp;
}
// A stone draw (PHYSICS.md 6) is sample_stone, the read of the predecessor's row of a terrain table, stone_after and the write of the
// new row.  The two functions are what every table shares; the read and the write stay with the table's owner: draw_stone below for the
// env's strided table with its provisional stones, look_row (ss_lookahead.hpp) for a branch's contiguous one.
// One Philox block of env e -> the new stone's distance dr (returned), tilts, and the yaw step and elevation of its sampled cell
SSD float sample_stone(const Params& P, const Knobs& K, int e, uint32_t& ctr, float& xt, float& yt, float& yaw, float& pitch) {
  uint32_t r[4];
  env_block(P, e, ctr, r);
  int cell = sample_cell(P, K, e, u01(r[0]));
  float ratio = (float)K.curriculum / 5.0f;
  float dr = 0.65f + u01(r[1]) * (0.6f * ratio);
  float tilt = 15.0f * kDeg * ratio;
  xt = (2.f * u01(r[2]) - 1.f) * tilt;
  yt = (2.f * u01(r[3]) - 1.f) * tilt;
  yaw = yaw_sample(cell / SS_GRID);
  pitch = pitch_sample(cell % SS_GRID);
  return dr;
}
// ... and the stone itself from its predecessor's centre and heading angle phi: centre, normal, tilts, cos / sin of its heading
SSD void stone_after(float px, float py, float pz, float phi, float dr, float pitch, float xt, float yt, float out_p[3], float out_n[3],
                     float out_t[2], float out_h[2]) {
  float sp, cp, sph, cph;
  sincosf(pitch, &sp, &cp);
  sincosf(phi, &sph, &cph);
  place_stone(px, py, pz, dr, cp, sp, cph, sph, out_p);
  out_t[0] = xt; out_t[1] = yt;
  out_h[0] = cph; out_h[1] = sph;
  stone_normal(phi, xt, yt, out_n);
}
// draw stone k from stone k-1 (terrain table), write it to the table; returns dr and the new stone's data
SSD float draw_stone(const Params& P, const Knobs& K, int e, uint32_t& ctr, int k, float out_p[3], float out_n[3],
                     float out_t[2], float out_h[2], bool store = true) {
  float xt, yt, yaw, pitch;
  float dr = sample_stone(P, K, e, ctr, xt, yt, yaw, pitch);
  const size_t np = (size_t)P.npad;
  float* T = P.terrain + e;
  // stones from prov_from on are provisional (not stored): the first draw of an episode (k = 3) starts from the provisional
  // stone 2 and puts the provisional stones 0..2 into the table
  int prov = P.istate[e + I_PROV * np];
  const bool prev_stored = k - 1 < prov;
  float px = prev_stored ? T[((k - 1) * 6 + 0) * np] : 0.75f * (float)(k - 1);
  float py = prev_stored ? T[((k - 1) * 6 + 1) * np] : 0.f, pz = prev_stored ? T[((k - 1) * 6 + 2) * np] : 0.f;
  float phi = (prev_stored ? T[((k - 1) * 6 + 3) * np] : 0.f) + yaw;
  stone_after(px, py, pz, phi, dr, pitch, xt, yt, out_p, out_n, out_t, out_h);
  if (store) {
#pragma unroll 1
    for (int j = prov; j < k; ++j) {            // (rare: once per episode that gets past its second stone)
      T[(j * 6 + 0) * np] = 0.75f * (float)j;
#pragma unroll
      for (int i = 1; i < 6; ++i) T[(j * 6 + i) * np] = 0.f;
    }
    T[(k * 6 + 0) * np] = out_p[0]; T[(k * 6 + 1) * np] = out_p[1]; T[(k * 6 + 2) * np] = out_p[2];
    T[(k * 6 + 3) * np] = phi; T[(k * 6 + 4) * np] = xt; T[(k * 6 + 5) * np] = yt;
    if (prov < k + 1) P.istate[e + I_PROV * np] = k + 1;
  }
  return dr;
}

SSD float planar_dist(const float a[3], const float b[3]) {
  float dx = a[0] - b[0], dy = a[1] - b[1];
  return sqrtf(dx * dx + dy * dy);
}

// roll and pitch of the base (PHYSICS.md 5), and cos / sin of its yaw WITHOUT the angle: yaw = atan2(B, A) with
// A = 1 - 2(y^2 + z^2), B = 2(wz + xy), so (cos yaw, sin yaw) = (A, B) / |(A, B)| (degenerate |(A,B)| = 0: yaw = 0).
SSD void quat_roll_pitch_cs(const float q[4], float& roll, float& pitch, float& cy, float& sy) {
  float w = q[0], x = q[1], y = q[2], z = q[3];
  roll = atan2f(2.f * (w * x + y * z), 1.f - 2.f * (x * x + y * y));
  pitch = asinf(fminf(fmaxf(2.f * (w * y - z * x), -1.f), 1.f));
  float A = 1.f - 2.f * (y * y + z * z), B = 2.f * (w * z + x * y);
  float n2 = A * A + B * B;
  float inv = SS_RSQRT(fmaxf(n2, 1e-30f));
  cy = n2 > 1e-30f ? A * inv : 1.f;
  sy = n2 > 1e-30f ? B * inv : 0.f;
}

// target block of the observation (PHYSICS.md 5): [sin(dtheta) d, cos(dtheta) d, dz, x_tilt, y_tilt] with dtheta the
// bearing of the stone relative to the body yaw and d the planar distance -- i.e. the planar offset rotated by -yaw:
// sin(a - yaw) d = dy cos(yaw) - dx sin(yaw), cos(a - yaw) d = dx cos(yaw) + dy sin(yaw).  No atan2 / sincos needed.
SSD void target_features(const float pos[3], float cy, float sy, const float sp[3], const float tilt[2], float o[5]) {
  float dx = sp[0] - pos[0], dy = sp[1] - pos[1], dz = sp[2] - pos[2];
  o[0] = dy * cy - dx * sy; o[1] = dx * cy + dy * sy; o[2] = dz; o[3] = tilt[0]; o[4] = tilt[1];
}

SSD float clip5(float x) { return fminf(fmaxf(x, -5.f), 5.f); }
// joint entries of the observation (PHYSICS.md 5), in POLICY coordinates (PHYSICS.md 2): ps = +-1 is the joint's kPolicySign, applied
// to the true-world angle and to the middle of its true range (the negations are exact)
SSD float obs_angle(float ps, float q, float mid, float span) { return clip5(2.f * (ps * q - ps * mid) / span); }
SSD float obs_rate(float ps, float qd) { return clip5(0.1f * (ps * qd)); }

// "Joint J is at its limit" (PHYSICS.md 4: the normalised angle beyond 0.99), one definition for step_env and step_logic.  The division
// stays: a compare of fabsf(q - mid) with the smallest float at which this form is true gives the same answer for every q (the division
// is correctly rounded, hence monotone) and takes 146 VALU instructions off the control step's epilogue, but the three-helper K-step
// kernel measured slower with it (docs/HISTORY.md "Spine torques on helper 1").
template <class Model, int J>
SSD bool at_joint_limit(float q) {
  constexpr float mid = 0.5f * (Model::lo[J] + Model::hi[J]);
  constexpr float span = Model::hi[J] - Model::lo[J];
  return fabsf(2.f * (q - mid) / span) > 0.99f;
}

// observation (PHYSICS.md section 5) written row-major to obs[60].  The base / contact / target entries (obs 0-5, 48-59) are
// written a second time in emit_outputs, on the lane-pair layout of the step kernels (merging the two moves the instructions of the
// benchmarked kernel); tests/test_gpu_env_control.py::test_reset_of_finished_envs_equals_auto_reset and
// tests/test_gpu_parity.py::test_reset_matches_oracle hold the two to the same bits.
template <class Model>
SSD void write_obs(const Dyn& s, float z_init, int flags, const Cache& c, float* obs) {
  float roll, pitch, sy, cy;
  quat_roll_pitch_cs(s.quat, roll, pitch, cy, sy);
  float R[3][3];
  quat_rot(s.quat, R);
  float vw[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) vw[r] = R[r][0] * s.v0.v[0] + R[r][1] * s.v0.v[1] + R[r][2] * s.v0.v[2];
  obs[0] = clip5(s.pos[2] - z_init);
  obs[1] = clip5(cy * vw[0] + sy * vw[1]);
  obs[2] = clip5(-sy * vw[0] + cy * vw[1]);
  obs[3] = clip5(vw[2]);
  obs[4] = clip5(roll);
  obs[5] = clip5(pitch);
  static_for<0, NJ>([&](auto Jc) {
    constexpr int j = decltype(Jc)::value;
    constexpr float mid = 0.5f * (Model::lo[j] + Model::hi[j]);
    constexpr float span = Model::hi[j] - Model::lo[j];
    constexpr float ps = (float)kPolicySign[j];
    obs[6 + j] = obs_angle(ps, s.q[j], mid, span);
    obs[27 + j] = obs_rate(ps, s.qd[j]);
  });
  obs[48] = (flags & 1) ? 1.f : 0.f;
  obs[49] = (flags & 2) ? 1.f : 0.f;
  float t[5];
  target_features(s.pos, cy, sy, c.p[1], c.tilt[1], t);
#pragma unroll
  for (int i = 0; i < 5; ++i) obs[50 + i] = t[i];
  target_features(s.pos, cy, sy, c.p[2], c.tilt[2], t);
#pragma unroll
  for (int i = 0; i < 5; ++i) obs[55 + i] = t[i];
}

// ---------------------------------------------------------------------------------------------------------------
SSD void load_dyn(const Params& P, int e, Dyn& s) {
  const float* F = P.fstate + e;
  const size_t np = (size_t)P.npad;
#pragma unroll
  for (int i = 0; i < 3; ++i) s.pos[i] = F[(F_POS + i) * np];
#pragma unroll
  for (int i = 0; i < 4; ++i) s.quat[i] = F[(F_QUAT + i) * np];
#pragma unroll
  for (int i = 0; i < 3; ++i) { s.v0.w[i] = F[(F_VEL + i) * np]; s.v0.v[i] = F[(F_VEL + 3 + i) * np]; }
#pragma unroll
  for (int j = 0; j < NJ; ++j) { s.q[j] = F[(F_Q + j) * np]; s.qd[j] = F[(F_QD + j) * np]; }
}
SSD void store_dyn(const Params& P, int e, const Dyn& s) {
  float* F = P.fstate + e;
  const size_t np = (size_t)P.npad;
#pragma unroll
  for (int i = 0; i < 3; ++i) F[(F_POS + i) * np] = s.pos[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) F[(F_QUAT + i) * np] = s.quat[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) { F[(F_VEL + i) * np] = s.v0.w[i]; F[(F_VEL + 3 + i) * np] = s.v0.v[i]; }
#pragma unroll
  for (int j = 0; j < NJ; ++j) { F[(F_Q + j) * np] = s.q[j]; F[(F_QD + j) * np] = s.qd[j]; }
}
SSD void load_cache(const Params& P, int e, Cache& c) {
  const float* F = P.fstate + e;
  const size_t np = (size_t)P.npad;
#pragma unroll
  for (int sl = 0; sl < 3; ++sl) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { c.p[sl][i] = F[(F_STONE + sl * 8 + i) * np]; c.nrm[sl][i] = F[(F_STONE + sl * 8 + 3 + i) * np]; }
    c.tilt[sl][0] = F[(F_STONE + sl * 8 + 6) * np];
    c.tilt[sl][1] = F[(F_STONE + sl * 8 + 7) * np];
  }
}
SSD void store_cache(const Params& P, int e, const Cache& c) {
  float* F = P.fstate + e;
  const size_t np = (size_t)P.npad;
#pragma unroll
  for (int sl = 0; sl < 3; ++sl) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { F[(F_STONE + sl * 8 + i) * np] = c.p[sl][i]; F[(F_STONE + sl * 8 + 3 + i) * np] = c.nrm[sl][i]; }
    F[(F_STONE + sl * 8 + 6) * np] = c.tilt[sl][0];
    F[(F_STONE + sl * 8 + 7) * np] = c.tilt[sl][1];
  }
}
// the active stones' headings (cos, sin of phi): what the plank footprint is aligned with (PHYSICS.md 3.3).  Their own 6 rows of fstate,
// written on reset / advance / set_state only; inside a step they live in the lane's LDS (kLdsHead), never in the Cache registers
SSD void store_headings(const Params& P, int e, const float (&h)[3][2]) {
  float* F = P.fstate + e;
  const size_t np = (size_t)P.npad;
#pragma unroll
  for (int sl = 0; sl < 3; ++sl) { F[(F_HEAD + sl * 2) * np] = h[sl][0]; F[(F_HEAD + sl * 2 + 1) * np] = h[sl][1]; }
}
// rebuild the active-stone cache of env e from the terrain table (after set_state)
SSD void cache_from_terrain(const Params& P, int e, int n, Cache& c, float (&hd)[3][2]) {
  const size_t np = (size_t)P.npad;
  const float* T = P.terrain + e;
  int idx[3] = {n - 1 < 0 ? 0 : n - 1, n, n + 1 > kNumStones - 1 ? kNumStones - 1 : n + 1};
#pragma unroll
  for (int sl = 0; sl < 3; ++sl) {
    int k = idx[sl];
#pragma unroll
    for (int i = 0; i < 3; ++i) c.p[sl][i] = T[(k * 6 + i) * np];
    float phi = T[(k * 6 + 3) * np], xt = T[(k * 6 + 4) * np], yt = T[(k * 6 + 5) * np];
    c.tilt[sl][0] = xt; c.tilt[sl][1] = yt;
    stone_normal(phi, xt, yt, c.nrm[sl]);
    sincosf(phi, &hd[sl][1], &hd[sl][0]);
  }
}

// the provisional path of a fresh episode (PHYSICS.md 6): stones along +x, 0.75 m apart, flat
SSD void flat_path(Stones& c) {
#pragma unroll
  for (int sl = 0; sl < 3; ++sl) {
    c.p[sl][0] = 0.75f * (float)sl; c.p[sl][1] = 0.f; c.p[sl][2] = 0.f;
    c.nrm[sl][0] = 0.f; c.nrm[sl][1] = 0.f; c.nrm[sl][2] = 1.f;
    c.tilt[sl][0] = 0.f; c.tilt[sl][1] = 0.f;
  }
}
// draw of the reset joint noise for global joint gj (PHYSICS.md section 7); r = the 6 Philox blocks of the reset
template <class Model, int GJ>
SSD float reset_angle(const uint32_t (&r)[6][4]) {
  constexpr float q0 = Model::q0[GJ], lo = Model::lo[GJ] + 0.02f, hi = Model::hi[GJ] - 0.02f;
  float q = q0 + 0.05f * (2.f * u01(r[GJ / 4][GJ % 4]) - 1.f);
  return fminf(fmaxf(q, lo), hi);
}

// PHYSICS.md section 7
template <class Model>
SSD void env_reset(const Params& P, int e, Dyn& s, Cache& c, uint32_t& ctr, float& pot, float& z_init, float& nn_dr) {
  const size_t np = (size_t)P.npad;
  P.istate[e + I_PROV * np] = 0;                // the whole path is provisional again: nothing is written to the terrain table
  flat_path(c);
  s.pos[0] = 0.f; s.pos[1] = 0.f; s.pos[2] = Model::stand_height + 0.01f;
  s.quat[0] = 1.f; s.quat[1] = s.quat[2] = s.quat[3] = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i) { s.v0.w[i] = 0.f; s.v0.v[i] = 0.f; }
  uint32_t r[6][4];
#pragma unroll
  for (int b = 0; b < 6; ++b) env_block(P, e, ctr, r[b]);
  static_for<0, NJ>([&](auto Jc) {
    constexpr int j = decltype(Jc)::value;
    s.q[j] = reset_angle<Model, j>(r);
    s.qd[j] = 0.f;
  });
  z_init = s.pos[2];
  nn_dr = 0.75f;
  pot = -planar_dist(c.p[1], s.pos) / kDt;
}
// The reset pose of this lane's half of env e at Philox counter ctr, in the lane's OWN world: write(k, angle) gets what put_joints
// stores to S_Q + k after a reset (reset_pose_offload() in ss_dynamics.hpp).  The six blocks of the reset noise are drawn three per lane
// of the pair and exchanged, as in step_env's reset branch: every lane of a pair calls this together.
template <class Model, class Write>
SSD void reset_pose_half(const Params& P, int e, int side, float m, uint32_t ctr, Write&& write) {
  uint32_t rr[6][4], c3 = ctr + (side ? 3u : 0u), mine[3][4];
#pragma unroll
  for (int b = 0; b < 3; ++b) env_block(P, e, c3, mine[b]);
#pragma unroll
  for (int b = 0; b < 3; ++b)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t other = xchg_u32(mine[b][i]);
      rr[b][i] = side ? other : mine[b][i];
      rr[3 + b][i] = side ? mine[b][i] : other;
    }
  static_for<0, NH>([&](auto Kc) {
    constexpr int k = decltype(Kc)::value, jr = kHalf[k];
    constexpr int jl = left_twin(jr);
    const float qt = side ? reset_angle<Model, jl>(rr) : reset_angle<Model, jr>(rr);      // true world, as step_env's
    write(k, mirror_sign(jr, m) * qt);
  });
}

// Peer-to-peer all-gather fused into the step kernel (multi-GPU, ss_step_packed_peers): every workgroup stores its rows of
// the packed block straight into each peer's gather buffer (xGMI stores into fine-grained memory) instead of a local
// buffer that a collective then ships.  Completion: every workgroup fences (system scope) and counts itself; the last
// one of a launch publishes flag_value in each peer's flag word of this rank.
constexpr int kMaxPeers = 8;
struct PeerTable {
  float* dst[kMaxPeers];        // peer p's gather buffer [G * n_local, 62] (p == my rank: my own)
  uint32_t* flag[kMaxPeers];    // peer p's flag array [G]
  uint32_t* done_counter;       // local, device scope: workgroups finished (monotonic)
  int count;                    // G
  int rank;                     // my rank: rows [rank * n_local, (rank+1) * n_local) and flag[p][rank] are mine
  int n_local;
};

struct StepIO {
  const float* act;   // [N,21] or null when actions are generated on device
  float* obs;         // [N,60]
  float* rew;         // [N]
  uint8_t* done;      // [N]
  ss_info* info;      // [N] or null
  uint64_t t;         // action-stream index for RANDOM_ACT
  float* packed;      // optional [N,62] = obs | rew | done(0/1): the block the multi-GPU all-gather ships; when set,
                      // obs / rew / done above may be null
  int nsteps;         // control steps per launch (rollout kernels; 1 otherwise)
  const PeerTable* peers;   // optional (device memory): also store the packed block into every peer's gather buffer
  uint32_t flag_value;      // what the last workgroup publishes in the peers' flag words (the step number)
  long long packed_step_stride;   // rollout kernels: step k of the launch writes its packed block at packed + k * stride
                                  // (0: every step overwrites the same block)
};

// The base state between the TRUE world and a lane's own world in LDS (m = +1: the right lane's is the true world; m = -1: the left
// lane's is its y-mirror, which negates y, the quaternion's x / z and the angular velocity's x / z)
SSD void put_base(const Lds& L, float m, const float pos[3], const float quat[4], const float w[3], const float v[3]) {
  L.s(S_POS + 0) = pos[0]; L.s(S_POS + 1) = m * pos[1]; L.s(S_POS + 2) = pos[2];
  L.s(S_QUAT + 0) = quat[0]; L.s(S_QUAT + 1) = m * quat[1]; L.s(S_QUAT + 2) = quat[2]; L.s(S_QUAT + 3) = m * quat[3];
  L.s(S_VW + 0) = m * w[0]; L.s(S_VW + 1) = w[1]; L.s(S_VW + 2) = m * w[2];
  L.s(S_VV + 0) = v[0]; L.s(S_VV + 1) = m * v[1]; L.s(S_VV + 2) = v[2];
}
SSD void get_base(const Lds& L, float m, float pos[3], float quat[4], SV& v0) {
  pos[0] = L.s(S_POS); pos[1] = m * L.s(S_POS + 1); pos[2] = L.s(S_POS + 2);
  quat[0] = L.s(S_QUAT); quat[1] = m * L.s(S_QUAT + 1); quat[2] = L.s(S_QUAT + 2); quat[3] = m * L.s(S_QUAT + 3);
  v0 = SV{{m * L.s(S_VW), L.s(S_VW + 1), m * L.s(S_VW + 2)}, {L.s(S_VV), m * L.s(S_VV + 1), L.s(S_VV + 2)}};
}
// ... and this lane's joints (mirror_sign)
SSD void put_joints(const Lds& L, float m, const float (&q)[NH], const float (&qd)[NH]) {
  static_for<0, NH>([&](auto Kc) {
    constexpr int k = decltype(Kc)::value, jr = kHalf[k];
    const float sg = mirror_sign(jr, m);
    L.s(S_Q + k) = sg * q[k];
    L.s(S_QD + k) = sg * qd[k];
  });
}
SSD void get_joints(const Lds& L, float m, float (&q)[NH], float (&qd)[NH]) {
  static_for<0, NH>([&](auto Kc) {
    constexpr int k = decltype(Kc)::value, jr = kHalf[k];
    const float sg = mirror_sign(jr, m);
    q[k] = sg * L.s(S_Q + k);
    qd[k] = sg * L.s(S_QD + k);
  });
}
// ... the active stones (true world) and, where they travel with them (h not null), the cos / sin of their headings
SSD void put_stones(const Lds& L, float m, const Cache& c, const float (*h)[2] = nullptr) {
#pragma unroll
  for (int sl = 0; sl < 3; ++sl) {
    L.s(S_STP + sl * 3 + 0) = c.p[sl][0]; L.s(S_STP + sl * 3 + 1) = m * c.p[sl][1]; L.s(S_STP + sl * 3 + 2) = c.p[sl][2];
    L.s(S_STN + sl * 3 + 0) = c.nrm[sl][0]; L.s(S_STN + sl * 3 + 1) = m * c.nrm[sl][1]; L.s(S_STN + sl * 3 + 2) = c.nrm[sl][2];
    if (h) L.q2(kLdsHead + sl) = make_float2(h[sl][0], m * h[sl][1]);       // the heading in this lane's (y-mirrored) world
  }
}
// this lane's half of an action row [21] ...
SSD void load_actions(const float* act_row, int side, float (&ain)[NH]) {
  static_for<0, NH>([&](auto Kc) {
    constexpr int k = decltype(Kc)::value, jr = kHalf[k];
    constexpr int jl = left_twin(jr);
    ain[k] = act_row[side ? jl : jr];
  });
}
// ... and its way into LDS: clipped to [-1, 1], signed for the lane's world
SSD void put_actions(const Lds& L, float m, const float (&ain)[NH]) {
  static_for<0, NH>([&](auto Kc) {
    constexpr int k = decltype(Kc)::value, jr = kHalf[k];
    const float sg = action_lane_sign(jr, m);
    const float x = ain[k];
    float a = fminf(fmaxf(x, -1.f), 1.f);
    a = (x != x) ? x : a;      // a NaN action is not clipped away (fmaxf would): it ends the episode, PHYSICS.md 4.8
    L.s(S_ACT + k) = sg * a;
  });
}

// What a control step has in a lane's LDS columns before its first substep, except the actions: the stones and headings of env e and the
// lane's half of its dynamic state, mirrored for the left lane.  ACT: this lane's half of act_row is loaded along (ain; put_actions
// stores it).  Only what the substeps need is loaded here: see step_env.
template <bool ACT>
SSD void load_in(const Params& P, int e, const float* act_row, int side, float m, const Lds& L, float (&ain)[NH]) {
  const size_t np = (size_t)P.npad;
  const float* F = P.fstate + e;
  {   // measured: merging these loads with the state loads below is slower (0.0867 vs 0.0857 ms/step)
    Cache c0;
    load_cache(P, e, c0);
    float h0[3][2];
#pragma unroll
    for (int sl = 0; sl < 3; ++sl) { h0[sl][0] = F[(F_HEAD + sl * 2) * np]; h0[sl][1] = F[(F_HEAD + sl * 2 + 1) * np]; }
    put_stones(L, m, c0, h0);
  }
  // this lane's half of the state.  All global loads are issued before the first LDS store: written load-store-load-store the
  // compiler waited for every load in turn (~25 exposed L2 round trips per step).
  float gin[13], qin[NH], qdin[NH];
#pragma unroll
  for (int i = 0; i < 3; ++i) gin[i] = F[(F_POS + i) * np];
#pragma unroll
  for (int i = 0; i < 4; ++i) gin[3 + i] = F[(F_QUAT + i) * np];
#pragma unroll
  for (int i = 0; i < 6; ++i) gin[7 + i] = F[(F_VEL + i) * np];
  static_for<0, NH>([&](auto Kc) {
    constexpr int k = decltype(Kc)::value, jr = kHalf[k];
    constexpr int jl = left_twin(jr);
    const int gj = side ? jl : jr;
    qin[k] = F[(F_Q + gj) * np];
    qdin[k] = F[(F_QD + gj) * np];
  });
  if constexpr (ACT) load_actions(act_row, side, ain);
  put_base(L, m, gin, gin + 3, gin + 7, gin + 10);
  put_joints(L, m, qin, qdin);
}

// Item 39 of LDS region A, the one item of the block that neither the contact operators (0..35) nor the headings (36..38) use: two words
// that a dry-run kernel keeps across its substep calls (ss_forces.hpp, ss_lookahead.hpp; the step kernels leave it alone)
constexpr int kLdsNote = kLdsHead + 3;
static_assert(kLdsNote < kSlotsA * 2, "the note is inside region A");

// ---- output stage of a control step: observation / reward / done / info rows and the bulk of the state write-back ----
struct StepOut {        // what it needs, true world, after the optional reset
  float pos[3], quat[4];
  SV v0;
  float qt[NH], qdt[NH];                      // this lane's joints
  float r, z_init, roll, pitch, cyaw, syaw;   // roll .. syaw: of the orientation the step ended in (not used after a reset)
  int d, flags, do_reset;
  float tgt[2][5];                            // stones n and n+1: centre (3), tilts (2)
  ss_info inf;
};
// Observation / info rows are staged in LDS (region A is free at that point) and written out by the whole wavefront as
// contiguous 256-byte stores: a lane writing its own [60]-float row directly would touch 32 partial cache lines
// per store instruction (measured 3.1x the algorithmic HBM traffic before this).  One body for the device and for the
// host pre-flight (tests/host/host_harness.cpp runs the 64 lanes of a wavefront as threads around the same LDS block).
// The global stores are plain: non-temporal ones in the one-launch-per-step kernels measured 1.2 % (0.0648 -> 0.0640 ms/step at 4096
// envs) on that secondary figure only, not adopted (docs/HISTORY.md).
//
// copy_out: one word (or float4) of the staged block to global memory.  By-value arguments on purpose: the address is formed before
// the LDS load and a float4 moves as four floats -- the schedule of the copy loops that the kernels were measured with (`dst[g] =
// lds[g]` evaluates the load first and the loops schedule differently).
template <class T>
SSD void copy_out(T* dst, T v) { *dst = v; }
// The observation row of one env on the lane-pair layout, into its staged row `stage`: every lane the joint entries of its own limbs,
// the right lane the spine's (stage_obs_joint, for the joints with jr >= 3 || side == 0) and the base / contact / target entries
// (stage_obs_base).  All values true world.  Two functions: the step kernels store the joint's state between the entries.
// Joint K of this lane's half: the observation carries POLICY coordinates (PHYSICS.md 2): ps = kPolicySign of THIS joint (left x / z
// joints: about the mirrored axis; knees: negative in flexion), applied to the true-world angle and to the middle of its true range (a
// left x / z joint's true range is (-hi, -lo) of its right twin's).  The state arrays keep angles about the +axis.
template <class Model, int K>
SSD void stage_obs_joint(float* stage, int side, float q, float qd) {
  constexpr int jr = kHalf[K];
  constexpr int jl = left_twin(jr);
  const int gj = side ? jl : jr;
  constexpr float midr = 0.5f * (Model::lo[jr] + Model::hi[jr]);
  constexpr float span = Model::hi[jr] - Model::lo[jr];
  const float ps = policy_true_sign(jr, side);
  const float mid = (side && mirror_flips(jr)) ? -midr : midr;
  stage[6 + gj] = obs_angle(ps, q, mid, span);
  stage[27 + gj] = obs_rate(ps, qd);
}
// obs 0-5 and 48-59: the same entries as in write_obs (see there for the tests that pin the two copies together).  roll .. sy:
// quat_roll_pitch_cs of the orientation; p1, t1, p2, t2: centre and tilts of the stones n and n+1
SSD void stage_obs_base(float* stage, const float pos[3], const float quat[4], const SV& v0, float z_init, float roll, float pitch,
                        float cy, float sy, int flags, const float* p1, const float* t1, const float* p2, const float* t2) {
  float R[3][3];
  quat_rot(quat, R);
  float vw[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) vw[i] = R[i][0] * v0.v[0] + R[i][1] * v0.v[1] + R[i][2] * v0.v[2];
  stage[0] = clip5(pos[2] - z_init);
  stage[1] = clip5(cy * vw[0] + sy * vw[1]);
  stage[2] = clip5(-sy * vw[0] + cy * vw[1]);
  stage[3] = clip5(vw[2]);
  stage[4] = clip5(roll);
  stage[5] = clip5(pitch);
  stage[48] = (flags & 1) ? 1.f : 0.f;
  stage[49] = (flags & 2) ? 1.f : 0.f;
  float t[5];
  target_features(pos, cy, sy, p1, t1, t);
#pragma unroll
  for (int i = 0; i < 5; ++i) stage[50 + i] = t[i];
  target_features(pos, cy, sy, p2, t2, t);
#pragma unroll
  for (int i = 0; i < 5; ++i) stage[55 + i] = t[i];
}
template <class Model, bool ROLLOUT>
SSD void emit_outputs(const Params& P, const StepIO& io, const StepOut& o, int e, int side, bool valid, int lane, int lane_global,
                      int kstep, float* lds) {
  const size_t np = (size_t)P.npad;
  // Rows are staged back to back in the layout of the output block -- [32][60] for obs, [32][62] = obs | rew | done for the
  // packed block -- so that the wavefront copies the block with float4 loads / stores (8 iterations instead of 31 scalar
  // ones with an index division each; the 4-way bank conflicts of the stride-60 staging writes are fire-and-forget).
  constexpr int kPackW = SS_OBS_DIM + 2;
  const bool packed_layout = io.packed != nullptr || io.peers != nullptr;   // wavefront-uniform
  const int stride = packed_layout ? kPackW : SS_OBS_DIM;
  constexpr int kInfoBase = kEnvsPerWave * 64;         // behind the largest staged block
  float* stage = lds + (lane >> 1) * stride;
  uint32_t* istage = reinterpret_cast<uint32_t*>(lds) + kInfoBase + (lane >> 1) * SS_INFO_WORDS;
  SS_WAVE_SYNC();          // the staging area is region A: every lane must be through with its contact operators
  if (valid) {
    float* Fo = P.fstate + e;
    // per-joint state + observation entries: own limbs by each lane, spine by the right lane
    static_for<0, NH>([&](auto Kc) {
      constexpr int k = decltype(Kc)::value, jr = kHalf[k];
      constexpr int jl = left_twin(jr);
      const int gj = side ? jl : jr;
      if (jr >= 3 || side == 0) {
        Fo[(F_Q + gj) * np] = o.qt[k];
        Fo[(F_QD + gj) * np] = o.qdt[k];
        stage_obs_joint<Model, k>(stage, side, o.qt[k], o.qdt[k]);
      }
    });
    if (side == 0) {
      // a reset leaves the identity orientation: roll = pitch = yaw = 0 exactly; otherwise the values of the final orientation
      const float r2 = o.do_reset ? 0.f : o.roll, p2 = o.do_reset ? 0.f : o.pitch;
      const float cy = o.do_reset ? 1.f : o.cyaw, sy = o.do_reset ? 0.f : o.syaw;
      stage_obs_base(stage, o.pos, o.quat, o.v0, o.z_init, r2, p2, cy, sy, o.flags, &o.tgt[0][0], &o.tgt[0][3], &o.tgt[1][0], &o.tgt[1][3]);
      if (io.rew) io.rew[e] = o.r;
      if (io.done) io.done[e] = o.d ? 1 : 0;
      if (packed_layout) {
        stage[SS_OBS_DIM] = o.r;
        stage[SS_OBS_DIM + 1] = o.d ? 1.f : 0.f;
      }
      istage[0] = SS_F2U(o.inf.ep_ret); istage[1] = SS_F2U(o.inf.ep_len);
      istage[2] = (uint32_t)o.inf.bad_transition; istage[3] = (uint32_t)o.inf.steps_reached; istage[4] = (uint32_t)o.inf.update_terrain;
      istage[5] = SS_F2U(o.inf.ep_ret_lo);
#pragma unroll
      for (int i = 0; i < 3; ++i) Fo[(F_POS + i) * np] = o.pos[i];
#pragma unroll
      for (int i = 0; i < 4; ++i) Fo[(F_QUAT + i) * np] = o.quat[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) { Fo[(F_VEL + i) * np] = o.v0.w[i]; Fo[(F_VEL + 3 + i) * np] = o.v0.v[i]; }
    }
  }
  {
    SS_WAVE_SYNC();
    const int env0 = (lane_global - lane) >> 1;                                   // first env of this wavefront
    // (never negative: a wavefront without a valid env -- not launched since round 4, ss_api.hip: grid = ceil(n / 32) -- would
    // otherwise reach copy_block with nfl < 0, where `n4 << 2` rounds below nfl and lanes 0 and 1 stored two out-of-range LDS words
    // into the reward / done slots of env n - 1's PACKED row: the schedule-dependent step of DESIGN.md 5.1b)
    const int nleft = P.n - env0;
    const int nvalid = nleft <= 0 ? 0 : (kEnvsPerWave < nleft ? kEnvsPerWave : nleft);
    // copy the staged block (nfl floats from the start of the LDS staging area) to dst: float4 when dst is 16-byte aligned
    auto copy_block = [&](float* dst, int nfl) {
      if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        const int n4 = nfl >> 2;
        float4* d4 = reinterpret_cast<float4*>(dst);
        const float4* s4 = reinterpret_cast<const float4*>(lds);
#pragma unroll 1
        for (int g = lane; g < n4; g += kWave) copy_out(&d4[g], s4[g]);
        for (int g = (n4 << 2) + lane; g < nfl; g += kWave) copy_out(&dst[g], lds[g]);
      } else {
#pragma unroll 1
        for (int g = lane; g < nfl; g += kWave) copy_out(&dst[g], lds[g]);
      }
    };
    if (io.obs) {
      float* og = io.obs + (size_t)env0 * SS_OBS_DIM;
      if (!packed_layout) {
        copy_block(og, nvalid * SS_OBS_DIM);
      } else {                                   // both outputs requested: the staging has the packed layout
#pragma unroll 1
        for (int g = lane; g < nvalid * SS_OBS_DIM; g += kWave) {
          const int el = g / SS_OBS_DIM, idx = g - el * SS_OBS_DIM;
          copy_out(&og[g], lds[el * kPackW + idx]);
        }
      }
    }
    if (io.packed) {
      float* pk = io.packed + (size_t)env0 * kPackW;
      if constexpr (ROLLOUT) pk += (long long)kstep * io.packed_step_stride;
      copy_block(pk, nvalid * kPackW);
    }
    if (io.info) {
      uint32_t* ig = reinterpret_cast<uint32_t*>(io.info + env0);
      const uint32_t* is = reinterpret_cast<const uint32_t*>(lds) + kInfoBase;
      for (int g = lane; g < nvalid * SS_INFO_WORDS; g += kWave) copy_out(&ig[g], is[g]);
    }
#if defined(__HIP_DEVICE_COMPILE__)                   // the peer-store exchange exists on the device only (xGMI stores, system-scope atomics)
    if constexpr (!ROLLOUT) {
      if (io.peers) {
        constexpr int kPack = SS_OBS_DIM + 2;
        const PeerTable* T = io.peers;
        const int G = T->count;
        const size_t row0 = (size_t)T->rank * (size_t)T->n_local + (size_t)env0;
#pragma unroll 1
        for (int p = 0; p < G; ++p) copy_block(T->dst[p] + row0 * kPack, nvalid * kPack);
        __threadfence_system();                                   // my rows are visible to every agent ...
        if (lane == 0) {
          const uint32_t prev = atomicAdd(T->done_counter, 1u);   // ... before I count myself
          if ((prev + 1u) % gridDim.x == 0u) {                    // last workgroup of this launch (launches are stream-ordered)
            __threadfence_system();
            for (int p = 0; p < G; ++p)
              __hip_atomic_store(T->flag[p] + T->rank, io.flag_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
          }
        }
      }
    }
#endif
  }
}

// The three-helper rollout kernel hands the output stage to a helper wavefront: the main wavefront leaves 14 words in the hand-off
// region (the place of the detection's Rf / pen, which that variant does not use, and the two spare words), everything else is the
// state in LDS region B (refreshed after a reset).  The helper works while the main wavefront is already in the next
// control step (between barriers #0b and #1 of its first substep; the state in LDS changes at that substep's end only).
// The one-launch-per-step kernel keeps its output stage inline: on a helper it measured 0.0697 against 0.0687 ms/step (round 3), and
// no gain again in round 6.
constexpr bool out_offload(int helpers, bool rollout) { return rollout && helpers >= 3; }
constexpr int kHandOut = kHandDet, kHandOut2 = kHandFloats;     // 13 + 2 words
static_assert(kHandOut2 + 2 <= kHandSlots * 4, "hand-off region");
// kHandOut2 + 1, the second spare word: the env's Philox counter as the control step leaves it, for the helper that draws the reset pose
// ahead of time (reset_pose_offload() in ss_dynamics.hpp; the three-helper K-step kernel, the only one that writes or reads the word)
constexpr int kHandCtr = kHandOut2 + 1;
static_assert(kHandCtr < kHandRows3, "below the rows' own words");
#if !defined(SS_HOST_HARNESS)
template <class Model, bool ROLLOUT>
__device__ __forceinline__ void emit_from_handoff(const Params& P, const StepIO& io, const Lds& L, int lane, int lane_global, int kstep,
                                                  float* lds) {
  const int e_raw = lane_global >> 1, side = lane_global & 1;
  const bool valid = e_raw < P.n;
  const int e = valid ? e_raw : P.n - 1;
  const float m = side ? -1.f : 1.f;
  StepOut o;
  get_base(L, m, o.pos, o.quat, o.v0);
  get_joints(L, m, o.qt, o.qdt);
  o.r = L.hs(kHandOut + 0);
  o.z_init = L.hs(kHandOut + 1);
  {   // the lane pair shares the word: the right lane left the leading part of the episode return, the left lane the trailing part
    const float w = L.hs(kHandOut + 2), w2 = xchg(w);
    o.inf.ep_ret = side ? w2 : w;
    o.inf.ep_ret_lo = side ? w : w2;
  }
  const int bits = __builtin_bit_cast(int, L.hs(kHandOut2 + 0));
  o.d = bits & 1;
  o.inf.bad_transition = (bits >> 1) & 1;
  o.inf.update_terrain = (bits >> 2) & 1;
  o.do_reset = (bits >> 3) & 1;
  o.flags = (bits >> 4) & 3;
  o.inf.steps_reached = (bits >> 8) & 31;
  o.inf.ep_len = (float)((bits >> 16) & 0xffff);
#pragma unroll
  for (int i = 0; i < 5; ++i) { o.tgt[0][i] = L.hs(kHandOut + 3 + i); o.tgt[1][i] = L.hs(kHandOut + 8 + i); }
  quat_roll_pitch_cs(o.quat, o.roll, o.pitch, o.cyaw, o.syaw);      // same function, same bits as the main wavefront's
  emit_outputs<Model, ROLLOUT>(P, io, o, e, side, valid, lane, lane_global, kstep, lds);
}
#endif

// Benchmark actions of control step tt for this lane's half of env e (PHYSICS.md 5: six Philox blocks per env and step, 21 of the
// 24 words -> U(-1,1)), in the lane's own (mirrored) world.  Both lanes of the pair draw all six blocks: three per lane, exchanged (as
// for the reset noise), measured -0.4 % / -0.6 % at 4096 envs and +0.9 % in the plain K-step kernel (round 6), not adopted.
template <class Write>
SSD void random_actions_half(const Params& P, int e, int side, float m, uint32_t tt, Write&& write) {
  uint32_t ra[6][4];
#pragma unroll
  for (int b = 0; b < 6; ++b) philox4x32_10(6u * tt + b, 1u, P.env_offset + ((uint32_t)e & P.id_mask), 0u, P.seed_lo, P.seed_hi, ra[b]);
  static_for<0, NH>([&](auto Kc) {
    constexpr int k = decltype(Kc)::value, jr = kHalf[k];
    constexpr int jl = left_twin(jr);
    const float sg = action_lane_sign(jr, m);
    const uint32_t bits = side ? ra[jl / 4][jl % 4] : ra[jr / 4][jr % 4];
    write(k, sg * (2.f * u01(bits) - 1.f));
  });
}

// Sections 6-9 of a control step by value: progress towards the target, termination, reward (PHYSICS.md 4.6-4.9)
struct StepScore {
  float pot_prev;                        // the potential the next step starts from
  bool d;                                // the episode ends
  int bad;                               // ... at the step limit
  float r, roll, pitch, cyaw, syaw;      // reward; quat_roll_pitch_cs of quat
};
SSD StepScore step_score(SS_PROF_DECL const float (&pos)[3], const float (&quat)[4], const Cache& c, const float (&target_old)[3],
                         const float (&sole)[2][3], float pot_prev, int advanced, int n, int elapsed, bool finite, float step_bonus,
                         float e_sum, float a2, int at_limit) {
  StepScore o;
  // 6. progress
  float pot = -planar_dist(target_old, pos) / kDt;
  SS_PROFE(4);       // first use of the loaded scalars (wait for L2) + target logic (+ draw on advance)
  float progress = pot - pot_prev;
  o.pot_prev = advanced ? -planar_dist(c.p[1], pos) / kDt : pot;
  // 7-8
  float target_bonus = (n == kNumStones - 1 && planar_dist(c.p[1], pos) < 0.15f) ? 2.f : 0.f;
  float zs = fminf(sole[0][2], sole[1][2]);
  float tall_bonus = (pos[2] - zs > 0.7f) ? 2.f : -1.f;
  float zlow = fminf(fminf(c.p[0][2], c.p[1][2]), c.p[2][2]);
  bool d = (tall_bonus < 0.f) || (pos[2] < zlow + 0.3f) || !finite;
  bool timeout = elapsed >= SS_MAX_EPISODE_STEPS;
  o.bad = timeout ? 1 : 0;                       // TimeLimitMask (common/envs_utils.py:59-65): done at the step limit, whatever else ended it
  o.d = d || timeout;
  // 9. reward
  quat_roll_pitch_cs(quat, o.roll, o.pitch, o.cyaw, o.syaw);      // of the state the step ended in (before a possible reset)
  float posture = 0.f;
  if (!(o.pitch > -0.2f && o.pitch < 0.4f)) posture += fabsf(o.pitch);
  if (!(o.roll > -0.4f && o.roll < 0.4f)) posture += fabsf(o.roll);
  float energy = (4.5f / NJ) * (e_sum / NJ) + (0.225f / NJ) * (a2 / NJ);
  float r = progress + step_bonus + target_bonus + tall_bonus - energy - posture - 0.1f * (float)at_limit;
  if (!finite || !finite_bits(r)) r = 0.f;
  o.r = r;
  SS_PROFE(5);       // progress, termination, roll / pitch, reward
  return o;
}
// episode return as an unevaluated float pair (ep_ret, ep_lo): error-free two-sum of the step reward, then renormalised, so that the
// pair carries the fp64 sum of the fp32 step rewards (Monitor.update sums Python floats, common/envs_utils.py:134)
SSD void ep_return_add(float& ep_ret, float& ep_lo, float r) {
  const float s = ep_ret + r, bb = s - ep_ret;
  const float err = (ep_ret - (s - bb)) + (r - bb);
  const float lo = ep_lo + err;
  ep_ret = s + lo;
  ep_lo = lo - (ep_ret - s);
}

// What the env logic of a control step (step_logic) gives back besides the env-level words it updates in place
struct StepEnd {
  float pos[3], quat[4];                 // the base the substeps ended in, true world
  SV v0;
  int flags, advanced;                   // feet in contact (bit 0: right, bit 1: left); the target moved on
  float hd[3][2];                        // headings of the active stones, true world: meaningful after an advance only
  bool d;                                // the episode ends
  int bad;                               // ... at the step limit
  float r, roll, pitch, cyaw, syaw;      // reward; quat_roll_pitch_cs of quat
};
// The env logic of a control step behind its substeps (PHYSICS.md 4; sections 3-9 of step_env): pair exchange of the foot reports,
// joint sums, target logic, progress, termination, reward and the episode return, for this lane of the pair.  Env-level logic runs
// redundantly (and identically) in both lanes in the true world.  c and the env-level words come in as loaded and go out updated.  The
// stone of an advance comes from draw(ctr, k, p, nrm, tilt, heading, store) -> dr, the one point where a user's terrain table shows;
// `store` marks the lane that writes the table.  LDS: the state, the actions and the headings are read, the headings rewritten on an advance.
// The look-ahead (ss_lookahead.hpp) calls it.  step_env has sections 3-5 restated inline and calls step_score / ep_return_add itself:
// with this function in their place the benchmarked kernel measured 1.2 of the parent's spreads slower (docs/HISTORY.md, "One
// definition of the control step"; kept, gate failed).  tests/test_lookahead.py (host builds) and tests/test_gpu_lookahead.py hold the
// two to the same bits on cases that reach every branch: a change of sections 3-5 is made here AND there.
template <class Model, class Draw>
SSD void step_logic(SS_PROF_DECL const Lds& L, int side, float m, const FootReport& fr, Cache& c, float& pot_prev, float& nn_dr,
                    float& ep_ret, float& ep_lo, int& n, int& count, int& elapsed, uint32_t& ctr, bool store, Draw&& draw, StepEnd& o) {
  float (&pos)[3] = o.pos, (&quat)[4] = o.quat, (&hd)[3][2] = o.hd;
  SV& v0 = o.v0;
  // 3-4. back to the true world; the pair shares its feet
  get_base(L, m, pos, quat, v0);
  elapsed += 1;
  const float my_sole[3] = {fr.sole[0], m * fr.sole[1], fr.sole[2]};
  float ot_sole[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) ot_sole[i] = xchg(my_sole[i]);
  const int ot_contact = xchg_i(fr.contact), ot_target = xchg_i(fr.on_target);
  float sole[2][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) { sole[0][i] = side ? ot_sole[i] : my_sole[i]; sole[1][i] = side ? my_sole[i] : ot_sole[i]; }
  o.flags = side ? (ot_contact | (fr.contact << 1)) : (fr.contact | (ot_contact << 1));
  const int on_target = fr.on_target | ot_target;
  SS_PROFE(2);       // LDS state read-back, pair exchange of the foot reports
  // partial sums over this lane's joints (the spine is counted by the right lane only)
  float accv = 0.f, e_sum = 0.f, a2 = 0.f;
  int at_limit = 0;
  static_for<0, NH>([&](auto Kc) {
    constexpr int k = decltype(Kc)::value, jr = kHalf[k];
    const float q = L.s(S_Q + k), qd = L.s(S_QD + k), a = L.s(S_ACT + k);
    const bool mine = (jr >= 3) || (side == 0);
    accv += q + qd;
    if (mine) {
      e_sum += fabsf(a * (0.1f * qd));
      a2 += a * a;
      if (at_joint_limit<Model, jr>(q)) at_limit += 1;
    }
  });
  accv += pos[0] + pos[1] + pos[2] + quat[0] + quat[1] + quat[2] + quat[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) accv += v0.w[i] + v0.v[i];
  e_sum += xchg(e_sum);
  a2 += xchg(a2);
  at_limit += xchg_i(at_limit);
  const bool finite = finite_bits(accv) && (xchg_i(finite_bits(accv) ? 1 : 0) != 0);
  SS_PROFE(3);       // joint sums (energy, limits, finiteness)

  // 5. target logic
  float target_old[3] = {c.p[1][0], c.p[1][1], c.p[1][2]};
  float step_bonus = 0.f;
  int advanced = 0;
#pragma unroll
  for (int sl = 0; sl < 3; ++sl) { hd[sl][0] = 1.f; hd[sl][1] = 0.f; }
  if (on_target != 0) {
    count += 1;
    if (count == 1) {
      float d0 = planar_dist(sole[0], target_old), d1 = planar_dist(sole[1], target_old);
      step_bonus = 50.f * expf(-fminf(d0, d1) / 0.25f);
    }
    if (count >= 2 && n < kNumStones - 1) {
      n += 1;
      count = 0;
      advanced = 1;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        c.p[0][i] = c.p[1][i]; c.nrm[0][i] = c.nrm[1][i];
        c.p[1][i] = c.p[2][i]; c.nrm[1][i] = c.nrm[2][i];
      }
      c.tilt[0][0] = c.tilt[1][0]; c.tilt[0][1] = c.tilt[1][1];
      c.tilt[1][0] = c.tilt[2][0]; c.tilt[1][1] = c.tilt[2][1];
      // the headings move with the stones: slot 2 from the draw (at n = 19 it keeps the last stone's).  hd[] is the TRUE-world copy that
      // the step kernels' write-back stores; the lane's LDS holds its own (y-mirrored) world.  LDS is read here only: a target advance
      // is rare, a reset is not, and the write-back path must not wait for LDS
      const float2 h1 = L.q2(kLdsHead + 1), h2 = L.q2(kLdsHead + 2);
      hd[0][0] = h1.x; hd[0][1] = m * h1.y;
      hd[1][0] = h2.x; hd[1][1] = m * h2.y;
      hd[2][0] = h2.x; hd[2][1] = m * h2.y;
      if (n + 1 <= kNumStones - 1) nn_dr = draw(ctr, n + 1, c.p[2], c.nrm[2], c.tilt[2], hd[2], store);
      L.q2(kLdsHead + 0) = h1;
      L.q2(kLdsHead + 1) = h2;
      L.q2(kLdsHead + 2) = make_float2(hd[2][0], m * hd[2][1]);
    }
  }
  o.advanced = advanced;
  // 6-9. progress, termination, reward, episode return
  const StepScore sc = step_score(SS_PROF_ARG pos, quat, c, target_old, sole, pot_prev, advanced, n, elapsed, finite, step_bonus, e_sum, a2, at_limit);
  pot_prev = sc.pot_prev;
  o.d = sc.d; o.bad = sc.bad; o.r = sc.r; o.roll = sc.roll; o.pitch = sc.pitch; o.cyaw = sc.cyaw; o.syaw = sc.syaw;
  ep_return_add(ep_ret, ep_lo, sc.r);
}

// One control step, lane `lane_global` = 2*env + side (side 0: right half, true world; side 1: left half, mirrored
// world).  PHYSICS.md section 4.  Env-level logic runs redundantly (and identically) in both lanes in the true world.
// ROLLOUT: io.nsteps control steps in ONE launch (actions from the benchmark Philox stream at io.t, io.t+1, ...): the
// state is loaded into LDS once and stays there between steps (the epilogue refreshes the LDS copy when an env is reset
// or its target advances); every step still writes its outputs and the HBM copy of the state, so the result after K
// steps is bit-identical to K single-step launches (tested).
template <class Model, bool RANDOM_ACT, int HELPERS = 0, bool ROLLOUT = false>
SSD void step_env(const Params& P, const StepIO& io, int lane_global, int lane, float* lds) {
  static_assert(!ROLLOUT || RANDOM_ACT, "a multi-step launch draws its actions on the device");
  constexpr bool kOffload =            // output stage on a helper wavefront
#if defined(__HIP_DEVICE_COMPILE__)
      out_offload(HELPERS, ROLLOUT);
#else
      false;
#endif
  constexpr bool kPose =               // reset pose drawn ahead of time by a helper wavefront (reset_pose_offload() in ss_dynamics.hpp)
#if defined(__HIP_DEVICE_COMPILE__)
      reset_pose_offload(HELPERS, ROLLOUT);
#else
      false;
#endif
  static_assert(!kPose || kOffload, "the pose's helper and the counter's hand-off word are the output stage's kernel's");
  const int e_raw = lane_global >> 1, side = lane_global & 1;
  const bool valid = e_raw < P.n;
  int e = valid ? e_raw : P.n - 1;
  const size_t np = (size_t)P.npad;
  const float m = side ? -1.f : 1.f;            // y-mirror factor of this lane's world
  const Lds L{lds, lane};
  // Only what the substeps need is loaded before them; everything the step's epilogue needs (stone tilts,
  // counters, episode statistics) is (re)loaded afterwards from the L2-hot arrays, so that nothing sits in scratch
  // across the four substeps (those parked values were 2.2 MB of scratch write-back per launch).
  // 1. stones, headings and this lane's half of the state, mirrored for the left lane, into LDS
  float ain[NH];
  load_in<!RANDOM_ACT>(P, e, RANDOM_ACT ? nullptr : io.act + (size_t)e * NJ, side, m, L, ain);

  const int nsteps = ROLLOUT ? io.nsteps : 1;
#pragma unroll 1
  for (int kstep = 0; kstep < nsteps; ++kstep) {
  SS_FUZZ(0x60u);
  // clipped actions of this lane's joints (its own world) into LDS
  if constexpr (RANDOM_ACT) {
    bool drawn = false;
    if constexpr (ROLLOUT && HELPERS > 1) {   // (a single helper is the critical path already: 0.0612 vs 0.0638 ms/step at 16384 envs)
      if (kstep > 0) {               // the last helper wavefront drew them during the previous step (rollout_kernel_helped)
        float a[NH];
#pragma unroll
        for (int k = 0; k < NH; ++k) a[k] = L.hs(kHandAct + k);
#pragma unroll
        for (int k = 0; k < NH; ++k) L.s(S_ACT + k) = a[k];
        drawn = true;
      }
    }
    if (!drawn) random_actions_half(P, e, side, m, (uint32_t)io.t + (uint32_t)kstep, [&](int k, float a) { L.s(S_ACT + k) = a; });
  } else {
    put_actions(L, m, ain);
  }

  // 2. four substeps on the LDS-resident state
  const float power = P.knobs->power;
  FootReport fr;
#if defined(SS_PROFILE_PHASES) && defined(__HIP_DEVICE_COMPILE__)
  Prof prof;
#pragma unroll
  for (int i = 0; i < 16; ++i) prof.t[i] = 0;
  prof.last = (uint32_t)__builtin_amdgcn_s_memtime();
#endif
  Warm wm;                                     // contact impulses carried from substep to substep; every control step starts cold
  warm_clear(wm);
  if constexpr (warm_in_lds(HELPERS)) L.s(S_WKEY) = 0.f;
#pragma unroll 1
  for (int k = 0; k < kNumSubsteps; ++k) substep<Model, HELPERS, ROLLOUT>(SS_PROF_ARG power, fr, L, wm);
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (limb_tail_offload(HELPERS, ROLLOUT)) {   // helpers 1 and 2 integrate the arm joints and the base of the last substep
    SS_PROF(11);
    __syncthreads();                 // their stores are in LDS: the epilogue reads S_Q, S_QD and the base
    SS_FUZZ(0xCFu);
  }
#endif
  SS_FUZZ(0x61u);
  SS_PROF(12);
  SS_MEMBAR();
  SS_OPAQUE(e);                                 // recompute every global address below instead of spilling 27 pointers
  const float* F = P.fstate + e;
  const Knobs K = *P.knobs;                     // wavefront-uniform scalar loads
  Cache c;                                      // true world
  load_cache(P, e, c);                          // (keeping these 32 words resident in LDS between the steps of the rollout kernel was
  // measured slower, 0.0556 vs 0.0539 ms/step: the loads' latency is covered by the arithmetic below already)
  float pot_prev = F[F_POT * np], z_init = F[F_ZINIT * np];
  float ep_ret = F[F_EPRET * np], ep_lo = F[F_EPRET_LO * np], nn_dr = F[F_NNDR * np];
  int n = P.istate[e + I_N * np], count = P.istate[e + I_COUNT * np], elapsed = P.istate[e + I_ELAPSED * np];
  uint32_t ctr = (uint32_t)P.istate[e + I_RNG * np];
  const uint32_t ctr_in = ctr;                  // (kPose: the counter the helper drew the reset pose at)
  SS_PROFE(1);       // address arithmetic + issue of the epilogue's global loads

  // Sections 3-5 are step_logic's, restated (see there: its call here failed the speed gate)
  // 3-4. back to the true world; the pair shares its feet
  float pos[3], quat[4];
  SV v0;
  get_base(L, m, pos, quat, v0);
  elapsed += 1;
  const float my_sole[3] = {fr.sole[0], m * fr.sole[1], fr.sole[2]};
  float ot_sole[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) ot_sole[i] = xchg(my_sole[i]);
  const int ot_contact = xchg_i(fr.contact), ot_target = xchg_i(fr.on_target);
  float sole[2][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) { sole[0][i] = side ? ot_sole[i] : my_sole[i]; sole[1][i] = side ? my_sole[i] : ot_sole[i]; }
  int flags = side ? (ot_contact | (fr.contact << 1)) : (fr.contact | (ot_contact << 1));
  const int on_target = fr.on_target | ot_target;
  SS_PROFE(2);       // LDS state read-back, pair exchange of the foot reports
  // partial sums over this lane's joints (the spine is counted by the right lane only)
  float accv = 0.f, e_sum = 0.f, a2 = 0.f;
  int at_limit = 0;
  static_for<0, NH>([&](auto Kc) {
    constexpr int k = decltype(Kc)::value, jr = kHalf[k];
    const float q = L.s(S_Q + k), qd = L.s(S_QD + k), a = L.s(S_ACT + k);
    const bool mine = (jr >= 3) || (side == 0);
    accv += q + qd;
    if (mine) {
      e_sum += fabsf(a * (0.1f * qd));
      a2 += a * a;
      if (at_joint_limit<Model, jr>(q)) at_limit += 1;
    }
  });
  accv += pos[0] + pos[1] + pos[2] + quat[0] + quat[1] + quat[2] + quat[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) accv += v0.w[i] + v0.v[i];
  e_sum += xchg(e_sum);
  a2 += xchg(a2);
  at_limit += xchg_i(at_limit);
  const bool finite = finite_bits(accv) && (xchg_i(finite_bits(accv) ? 1 : 0) != 0);
  SS_PROFE(3);       // joint sums (energy, limits, finiteness)

  // 5. target logic
  float target_old[3] = {c.p[1][0], c.p[1][1], c.p[1][2]};
  float step_bonus = 0.f;
  int advanced = 0;
  float hd[3][2] = {{1.f, 0.f}, {1.f, 0.f}, {1.f, 0.f}};      // headings of the active stones, true world: meaningful after an advance / a reset only
  if (on_target != 0) {
    count += 1;
    if (count == 1) {
      float d0 = planar_dist(sole[0], target_old), d1 = planar_dist(sole[1], target_old);
      step_bonus = 50.f * expf(-fminf(d0, d1) / 0.25f);
    }
    if (count >= 2 && n < kNumStones - 1) {
      n += 1;
      count = 0;
      advanced = 1;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        c.p[0][i] = c.p[1][i]; c.nrm[0][i] = c.nrm[1][i];
        c.p[1][i] = c.p[2][i]; c.nrm[1][i] = c.nrm[2][i];
      }
      c.tilt[0][0] = c.tilt[1][0]; c.tilt[0][1] = c.tilt[1][1];
      c.tilt[1][0] = c.tilt[2][0]; c.tilt[1][1] = c.tilt[2][1];
      // the headings move with the stones: slot 2 from the draw (at n = 19 it keeps the last stone's).  hd[] is the TRUE-world copy that
      // the write-back below stores; the lane's LDS holds its own (y-mirrored) world.  LDS is read here only: a target advance is rare,
      // a reset is not, and the write-back path must not wait for LDS
      const float2 h1 = L.q2(kLdsHead + 1), h2 = L.q2(kLdsHead + 2);
      hd[0][0] = h1.x; hd[0][1] = m * h1.y;
      hd[1][0] = h2.x; hd[1][1] = m * h2.y;
      hd[2][0] = h2.x; hd[2][1] = m * h2.y;
      if (n + 1 <= kNumStones - 1) nn_dr = draw_stone(P, K, e, ctr, n + 1, c.p[2], c.nrm[2], c.tilt[2], hd[2], valid && side == 0);
      L.q2(kLdsHead + 0) = h1;
      L.q2(kLdsHead + 1) = h2;
      L.q2(kLdsHead + 2) = make_float2(hd[2][0], m * hd[2][1]);
    }
  }
  // 6-9. progress, termination, reward, episode return
  const StepScore sc = step_score(SS_PROF_ARG pos, quat, c, target_old, sole, pot_prev, advanced, n, elapsed, finite, step_bonus, e_sum, a2, at_limit);
  pot_prev = sc.pot_prev;
  const bool d = sc.d;
  const int bad = sc.bad;
  const float r = sc.r, roll = sc.roll, pitch = sc.pitch, cyaw = sc.cyaw, syaw = sc.syaw;
  ep_return_add(ep_ret, ep_lo, r);
  // 10. outputs, auto-reset
  ss_info inf;
  inf.ep_ret = ep_ret;
  inf.ep_ret_lo = ep_lo;
  inf.ep_len = (float)elapsed;
  inf.bad_transition = bad;
  inf.steps_reached = n;
  inf.update_terrain = advanced;
  const bool do_reset = d && K.auto_reset;
  SS_PROFE(6);
  uint32_t rr[6][4];
  // kPose: the pose in S_POSE was drawn at ctr_in; a lane that drew a stone in this very step has moved on and draws inline (below)
  const bool pose_stale = kPose && do_reset && ctr != ctr_in;
  if (do_reset) {
    // PHYSICS.md section 7: provisional terrain (prov_from = 0: no table writes), standing pose, joint noise from 6 Philox blocks
    if (valid && side == 0) P.istate[e + I_PROV * np] = 0;
    flat_path(c);
#pragma unroll
    for (int sl = 0; sl < 3; ++sl) {
      hd[sl][0] = 1.f; hd[sl][1] = 0.f;
      L.q2(kLdsHead + sl) = make_float2(1.f, 0.f);
    }
    pos[0] = 0.f; pos[1] = 0.f; pos[2] = Model::stand_height + 0.01f;
    quat[0] = 1.f; quat[1] = quat[2] = quat[3] = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) { v0.w[i] = 0.f; v0.v[i] = 0.f; }
    // the six Philox blocks of the reset noise: three per lane of the pair, exchanged (round 6: both lanes used to draw all six --
    // 300 more instructions on every control step in which ANY of the wavefront's 32 envs resets, i.e. on 3 steps of 4 under random
    // actions).  Integer-exact: the words are the ones env_block() would have produced.
    if constexpr (kPose) {             // a helper wavefront drew them (reset_pose_half): no Philox here
      ctr += 6u;
    } else {
      uint32_t c3 = ctr + (side ? 3u : 0u), mine[3][4];
#pragma unroll
      for (int b = 0; b < 3; ++b) env_block(P, e, c3, mine[b]);
#pragma unroll
      for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint32_t other = xchg_u32(mine[b][i]);
          rr[b][i] = side ? other : mine[b][i];
          rr[3 + b][i] = side ? mine[b][i] : other;
        }
      ctr += 6u;
    }
    z_init = pos[2];
    nn_dr = 0.75f;
    pot_prev = -planar_dist(c.p[1], pos) / kDt;
    n = 1; count = 0; elapsed = 0; flags = 0; ep_ret = 0.f; ep_lo = 0.f;
  }
  SS_PROFE(7);       // reset branch (Philox blocks)
  // joint values of this lane in the TRUE world (after the optional reset).  Read per joint on purpose: get_joints() in the else
  // branch of one `if (do_reset)` is the same values and about 2 900 moved instructions in every step / rollout kernel
  float qt[NH], qdt[NH];
  if constexpr (!kPose) {
    static_for<0, NH>([&](auto Kc) {
      constexpr int k = decltype(Kc)::value, jr = kHalf[k];
      constexpr int jl = left_twin(jr);
      const float sg = mirror_sign(jr, m);
      if (do_reset) {
        qt[k] = side ? reset_angle<Model, jl>(rr) : reset_angle<Model, jr>(rr);
        qdt[k] = 0.f;
      } else {
        qt[k] = sg * L.s(S_Q + k);
        qdt[k] = sg * L.s(S_QD + k);
      }
    });
  }
  // 11. output stage (emit_outputs): inline, or on a helper wavefront in the three-helper rollout kernel
  SS_PROFE(8);       // joint values of the next state
  SS_FUZZ(0x62u);
  if constexpr (ROLLOUT) {
    // the LDS copy of the state is what comes next (the next step, a helper's output stage): refresh what the env logic changed
    if (do_reset) {
      put_base(L, m, pos, quat, v0.w, v0.v);
      if constexpr (kPose) {
        // The joints: the helper's twelve words as they are, and the zero rates as put_joints stores them, mirror_sign x 0 -- the left
        // lane's mirrored joints hold -0, which the output stage's get_joints turns back into the +0 of the true world.  Written as
        // bits: -fno-signed-zeros must not choose the sign
        float qp[NH];
#pragma unroll
        for (int k = 0; k < NH; ++k) qp[k] = L.s(S_POSE + k);
        const float zm = __builtin_bit_cast(float, side ? 0x80000000u : 0u);
        static_for<0, NH>([&](auto Kc) {
          constexpr int k = decltype(Kc)::value;
          L.s(S_Q + k) = qp[k];
          L.s(S_QD + k) = mirror_flips(kHalf[k]) ? zm : 0.f;
        });
      } else {
        put_joints(L, m, qt, qdt);
      }
    }
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (kPose) {
      // the inline draw, for the lanes whose counter moved behind the helper's back: target advance with a stone drawn AND reset in one
      // step.  Wavefront-level branch: the common path never executes it.  Both lanes of a pair take it together (the env logic is theirs
      // in common), so the exchange inside has its partner
      if (__any(pose_stale)) {
        if (pose_stale) reset_pose_half<Model>(P, e, side, m, ctr - 6u, [&](int k, float q) { L.s(S_Q + k) = q; });
      }
    }
#endif
    if (advanced || do_reset) put_stones(L, m, c);
  }
  if constexpr (kOffload) {
    L.hs(kHandOut + 0) = r;
    L.hs(kHandOut + 1) = z_init;
    L.hs(kHandOut + 2) = side ? inf.ep_ret_lo : inf.ep_ret;
    const int bits = (d ? 1 : 0) | (inf.bad_transition << 1) | (inf.update_terrain << 2) | ((do_reset ? 1 : 0) << 3) | (flags << 4) |
                     (inf.steps_reached << 8) | ((int)inf.ep_len << 16);
    L.hs(kHandOut2 + 0) = __builtin_bit_cast(float, bits);
    if constexpr (kPose) L.hs(kHandCtr) = __builtin_bit_cast(float, ctr);
#pragma unroll
    for (int i = 0; i < 3; ++i) { L.hs(kHandOut + 3 + i) = c.p[1][i]; L.hs(kHandOut + 8 + i) = c.p[2][i]; }
#pragma unroll
    for (int i = 0; i < 2; ++i) { L.hs(kHandOut + 6 + i) = c.tilt[1][i]; L.hs(kHandOut + 11 + i) = c.tilt[2][i]; }
  } else {
    StepOut o;
#pragma unroll
    for (int i = 0; i < 3; ++i) o.pos[i] = pos[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) o.quat[i] = quat[i];
    o.v0 = v0;
#pragma unroll
    for (int k = 0; k < NH; ++k) { o.qt[k] = qt[k]; o.qdt[k] = qdt[k]; }
    o.r = r; o.z_init = z_init; o.roll = roll; o.pitch = pitch; o.cyaw = cyaw; o.syaw = syaw;
    o.d = d ? 1 : 0; o.flags = flags; o.do_reset = do_reset ? 1 : 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) { o.tgt[0][i] = c.p[1][i]; o.tgt[1][i] = c.p[2][i]; }
#pragma unroll
    for (int i = 0; i < 2; ++i) { o.tgt[0][3 + i] = c.tilt[1][i]; o.tgt[1][3 + i] = c.tilt[2][i]; }
    o.inf = inf;
    emit_outputs<Model, ROLLOUT>(P, io, o, e, side, valid, lane, lane_global, kstep, lds);
  }
  if (valid && side == 0) {            // the env-level scalars
  SS_PROFE(9);       // LDS refresh + hand-off to the emitting helper (or the inline output stage)
    float* Fo = P.fstate + e;
    if (advanced || do_reset) {
      store_cache(P, e, c);
      store_headings(P, e, hd);
    }
    Fo[F_POT * np] = pot_prev;
    Fo[F_ZINIT * np] = z_init;
    Fo[F_EPRET * np] = ep_ret;
    Fo[F_EPRET_LO * np] = ep_lo;
    Fo[F_NNDR * np] = nn_dr;
    P.istate[e + I_N * np] = n;
    P.istate[e + I_COUNT * np] = count;
    P.istate[e + I_ELAPSED * np] = elapsed;
    P.istate[e + I_RNG * np] = (int)ctr;
    P.istate[e + I_FLAGS * np] = flags;
  }
  SS_MEMBAR();
#if defined(SS_PROFILE_PHASES) && defined(__HIP_DEVICE_COMPILE__)
  SS_PROFE(10);      // env-level stores
  SS_PROF(13);
  if (lane == 0 && P.prof)
    for (int i = 0; i < 16; ++i) atomicAdd(P.prof + i, (unsigned long long)prof.t[i]);
#endif
  }   // control steps of this launch
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (out_offload(HELPERS, ROLLOUT)) __syncthreads();   // a helper emits the last step's outputs
#endif
}

#ifndef SS_HOST_HARNESS
template <class Model, bool RANDOM_ACT>
__global__ __launch_bounds__(kWave, 1) void step_kernel(Params P, StepIO io) {
  __shared__ float4 lds4[kLdsSlots * kWave];
  step_env<Model, RANDOM_ACT>(P, io, blockIdx.x * kWave + threadIdx.x, threadIdx.x, reinterpret_cast<float*>(lds4));   // lane = 2*env + side
}
// Small-batch variant: 1 + HELPERS wavefronts per 32 envs.  Wavefront 0 runs the step as above; the helper wavefront(s)
// compute the contact-space operators of every substep concurrently on the CU's other SIMDs (ss_dynamics.hpp:
// helper_substep).  Worth it only while the batch leaves SIMDs idle (4096 envs occupy 128 of 1024).
template <class Model, bool RANDOM_ACT, int HELPERS>
__global__ __launch_bounds__(kWave * (1 + HELPERS), 1) void step_kernel_helped(Params P, StepIO io) {
  __shared__ float4 lds4[(kLdsSlots + hand_slots(HELPERS)) * kWave];      // (three helpers: + the rows' own 40 words per lane)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
  float* lds = reinterpret_cast<float*>(lds4);
  SS_FUZZ(0x70u + wave);
  if (wave == 0) {
    step_env<Model, RANDOM_ACT, HELPERS>(P, io, blockIdx.x * kWave + lane, lane, lds);
  } else {
    const Lds L{lds, lane};
#pragma unroll 1
    for (int k = 0; k < kNumSubsteps; ++k) helper_substep<Model, HELPERS, 6>(wave - 1, L, [](int) {});
  }
}
// K control steps per launch (ss_rollout_random): same code, state resident in LDS between the steps
template <class Model>
__global__ __launch_bounds__(kWave, 1) void rollout_kernel(Params P, StepIO io) {
  __shared__ float4 lds4[kLdsSlots * kWave];
  step_env<Model, true, 0, true>(P, io, blockIdx.x * kWave + threadIdx.x, threadIdx.x, reinterpret_cast<float*>(lds4));
}
template <class Model, int HELPERS>
__global__ __launch_bounds__(kWave * (1 + HELPERS), 1) void rollout_kernel_helped(Params P, StepIO io) {
  __shared__ float4 lds4[(kLdsSlots + hand_slots(HELPERS)) * kWave];      // (three helpers: + the rows' own 40 words per lane)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
  float* lds = reinterpret_cast<float*>(lds4);
  SS_FUZZ(0x70u + wave);
  if (wave == 0) {
    step_env<Model, true, HELPERS, true>(P, io, blockIdx.x * kWave + lane, lane, lds);
  } else {
    const Lds L{lds, lane};
    const int lane_global = blockIdx.x * kWave + lane, side = lane_global & 1;
    const int e = min(lane_global >> 1, P.n - 1);
    const float m = side ? -1.f : 1.f;
    // The reset pose (reset_pose_offload() in ss_dynamics.hpp) is this helper's, behind barrier #3 of a control step's first substep, where
    // every helper idles until the main wavefront is through its PGS.  The counter it draws at: in the launch's first step the one in
    // HBM -- the state is resident before the launch and the main wavefront stores a counter only in its epilogue, behind barrier #0 of
    // the second substep, which this wavefront reaches with the load consumed --, afterwards the word the previous step's epilogue left
    // in the hand-off region (barriers #0 .. #3 of this step lie between that store and this read; the next store follows barrier #0 of
    // the next substep).  It draws again only when some lane's counter has moved (a reset, a stone drawn): ctr_pose is what S_POSE holds.
    constexpr int kPoseHelper = 0;
    const float power = spine_tau_offload(HELPERS, true) ? P.knobs->power : 0.f;     // as step_env reads it, for helper 1's joint_tau
    uint32_t ctr_pose = 0u;
    if constexpr (reset_pose_offload(HELPERS, true))
      if (wave - 1 == kPoseHelper) ctr_pose = (uint32_t)P.istate[e + I_RNG * (size_t)P.npad];
#pragma unroll 1
    for (int kstep = 0; kstep < io.nsteps; ++kstep)
#pragma unroll 1
      for (int k = 0; k < kNumSubsteps; ++k) {
        helper_substep<Model, HELPERS, 4, spine_tau_offload(HELPERS, true)>(wave - 1, L, [&](int helper) {
          if (k != 0) return;
          SS_FUZZ(0x80u + helper);
          // the next control step's actions, while the main wavefront is in pass 1 / 2 of this step's first substep
          // (three helpers: helper 1 -- which also has the spine's bias forces in this window -- draws the actions, helper 2 has the
          // longer job, the previous step's outputs, to itself; rounds 3-5 had them the other way round)
          constexpr int kActHelper = 1, kEmitHelper = HELPERS - 1;
          if (HELPERS > 1 && helper == kActHelper && kstep + 1 < io.nsteps)
            random_actions_half(P, e, side, m, (uint32_t)io.t + (uint32_t)kstep + 1u, [&](int j, float a) { L.hs(kHandAct + j) = a; });
          // the previous control step's outputs
          if (out_offload(HELPERS, true) && helper == kEmitHelper && kstep > 0) emit_from_handoff<Model, true>(P, io, L, lane, lane_global, kstep - 1, lds);
        }, power);
        if constexpr (reset_pose_offload(HELPERS, true)) {
          if (k == 0 && wave - 1 == kPoseHelper) {
            SS_FUZZ(0xA0u);
            const uint32_t ctr_now = kstep == 0 ? ctr_pose : __builtin_bit_cast(uint32_t, L.hs(kHandCtr));
            if (kstep == 0 || __any(ctr_now != ctr_pose)) {      // wavefront-uniform: every lane of a pair is in the exchange
              ctr_pose = ctr_now;
              reset_pose_half<Model>(P, e, side, m, ctr_now, [&](int j, float q) { L.s(S_POSE + j) = q; });
            }
          }
        }
        // The substep's tail behind dv0 (limb_tail_offload() in ss_dynamics.hpp): every helper meets #3r, helper 1 takes the arms and
        // helper 2 the base while the main wavefront sweeps down its spine and leg.  The next substep's #0 orders their stores; behind a
        // control step's last substep the main wavefront's epilogue reads them, behind one more barrier
        if constexpr (limb_tail_offload(HELPERS, true)) {
          __syncthreads();             // #3r: dv0 is in the hand-off region
          SS_FUZZ(0xB0u + (wave - 1));
          if constexpr (arm_tail_offload(HELPERS, true))
            if (wave - 1 == kArmHelper) helper_arm_tail<Model>(L);
          if constexpr (base_tail_offload(HELPERS, true))
            if (wave - 1 == kBaseHelper) helper_base_tail(L);
          if (k == kNumSubsteps - 1) {
            __syncthreads();           // the state the control step's epilogue reads is in LDS
            SS_FUZZ(0xC0u + (wave - 1));
          }
        }
      }
    if constexpr (out_offload(HELPERS, true)) {
      __syncthreads();                 // the last step's results are in the hand-off region
      SS_FUZZ(0x90u + wave);
      if (wave == 2) emit_from_handoff<Model, true>(P, io, L, lane, lane_global, io.nsteps - 1, lds);
    }
  }
}

// Reset of env e and its stores (reset_kernel, and reset_masked_kernel in ss_api.hip): the state the step kernel's in-place reset
// leaves, from the same Philox counter; the fresh observation goes to obs_row[0..59] unless obs_row is null.
template <class Model>
SSD void reset_env(const Params& P, int e, float* obs_row) {
  const size_t np = (size_t)P.npad;
  Dyn s;
  Cache c;
  uint32_t ctr = (uint32_t)P.istate[e + I_RNG * np];
  float pot, z_init, nn_dr;
  env_reset<Model>(P, e, s, c, ctr, pot, z_init, nn_dr);
  store_dyn(P, e, s);
  store_cache(P, e, c);
  const float straight[3][2] = {{1.f, 0.f}, {1.f, 0.f}, {1.f, 0.f}};      // the provisional path runs along +x
  store_headings(P, e, straight);
  P.fstate[e + F_POT * np] = pot;
  P.fstate[e + F_ZINIT * np] = z_init;
  P.fstate[e + F_EPRET * np] = 0.f;
  P.fstate[e + F_EPRET_LO * np] = 0.f;
  P.fstate[e + F_NNDR * np] = nn_dr;
  P.istate[e + I_N * np] = 1;
  P.istate[e + I_COUNT * np] = 0;
  P.istate[e + I_ELAPSED * np] = 0;
  P.istate[e + I_RNG * np] = (int)ctr;
  P.istate[e + I_FLAGS * np] = 0;
  if (obs_row) {
    float o[SS_OBS_DIM];
    write_obs<Model>(s, z_init, 0, c, o);
#pragma unroll
    for (int i = 0; i < SS_OBS_DIM; ++i) obs_row[i] = o[i];
  }
}

template <class Model>
__global__ __launch_bounds__(kWave) void reset_kernel(Params P, float* obs) {
  const int e = blockIdx.x * kWave + threadIdx.x;
  if (e >= P.n) return;
  reset_env<Model>(P, e, obs ? obs + (size_t)e * SS_OBS_DIM : nullptr);
}

template <class Model>
__global__ __launch_bounds__(kWave) void obs_kernel(Params P, float* obs) {
  const int e = blockIdx.x * kWave + threadIdx.x;
  if (e >= P.n) return;
  const size_t np = (size_t)P.npad;
  Dyn s;
  Cache c;
  load_dyn(P, e, s);
  load_cache(P, e, c);
  float o[SS_OBS_DIM];
  write_obs<Model>(s, P.fstate[e + F_ZINIT * np], P.istate[e + I_FLAGS * np], c, o);
#pragma unroll
  for (int i = 0; i < SS_OBS_DIM; ++i) obs[(size_t)e * SS_OBS_DIM + i] = o[i];
}
#endif  // SS_HOST_HARNESS

// packed [N,186] <-> structure of arrays (PHYSICS / include/steppingstone.h layout): env e <-> row `row` of packed (the whole-batch
// forms: row e; ss_get_state_envs / ss_set_state_envs: row k <-> env ids[k])
SSD void pack_env(const Params& P, int e, float* packed, size_t row) {
  const size_t np = (size_t)P.npad;
  float* o = packed + row * SS_STATE_DIM;
  for (int i = 0; i < 59; ++i) o[i] = P.fstate[e + (size_t)i * np];
  o[59] = (float)P.istate[e + I_N * np];
  o[60] = (float)P.istate[e + I_COUNT * np];
  o[61] = (float)P.istate[e + I_ELAPSED * np];
  uint32_t ctr = (uint32_t)P.istate[e + I_RNG * np];
  o[62] = (float)(ctr & 0xFFFFu);
  o[63] = (float)(ctr >> 16);
  o[64] = (float)P.istate[e + I_FLAGS * np];
  const int prov = P.istate[e + I_PROV * np];
  for (int i = 0; i < 120; ++i) {
    const int k = i / 6;
    o[65 + i] = k < prov ? P.terrain[e + (size_t)i * np] : (i % 6 == 0 ? 0.75f * (float)k : 0.f);
  }
  o[185] = P.fstate[e + (size_t)F_EPRET_LO * np];
}
SSD void pack_env(const Params& P, int e, float* packed) { pack_env(P, e, packed, (size_t)e); }
SSD void unpack_env(const Params& P, int e, const float* packed, size_t row) {
  const size_t np = (size_t)P.npad;
  const float* o = packed + row * SS_STATE_DIM;
  for (int i = 0; i < 59; ++i) P.fstate[e + (size_t)i * np] = o[i];
  int n = (int)o[59];
  P.istate[e + I_N * np] = n;
  P.istate[e + I_COUNT * np] = (int)o[60];
  P.istate[e + I_ELAPSED * np] = (int)o[61];
  P.istate[e + I_RNG * np] = (int)((uint32_t)o[62] | ((uint32_t)o[63] << 16));
  P.istate[e + I_FLAGS * np] = (int)o[64];
  for (int i = 0; i < 120; ++i) P.terrain[e + (size_t)i * np] = o[65 + i];
  P.istate[e + I_PROV * np] = kNumStones;        // an injected terrain is stored in full
  P.fstate[e + (size_t)F_EPRET_LO * np] = o[185];
  Cache c;
  float hd[3][2];
  cache_from_terrain(P, e, n, c, hd);
  store_cache(P, e, c);
  store_headings(P, e, hd);
}
SSD void unpack_env(const Params& P, int e, const float* packed) { unpack_env(P, e, packed, (size_t)e); }

}  // namespace ss
