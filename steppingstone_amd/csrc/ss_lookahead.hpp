// ss_lookahead.hpp -- look-ahead (docs/PHYSICS.md "Look-ahead" is the specification): H control steps of ss_step, with auto-reset off, on a
// PRIVATE copy of an env, under a caller-supplied action sequence -- one row ("branch") per (env id, action sequence), any number of rows
// per env.  Every step's observation, reward and done flag and the state the branch ends in come back; nothing of the env is written.
//
// The per-lane code re-composes the step kernels' device functions on the plain step kernel's shape, as ss_forces.hpp does: two lanes per
// row, one wavefront per workgroup, one Lds block, the dynamic state resident in LDS across the H steps (the ROLLOUT path of step_env).
// What a control step reads or writes besides the dynamic state -- the active stones, the terrain row, the target counters, the episode
// statistics, the RNG counter -- lives in the row's `work` words (W_* below), where the step kernel has the env's own arrays: loaded
// after the substeps, stored by the right lane, so that nothing is held in registers across substep().  The epilogue of step_env
// (ss_kernels.hpp sections 3-10) is inline there and is RESTATED in look_row, with the reset branch left out, and so are draw_stone's
// lines around the terrain table (draw_stone_row: the table is the row's private one); tests/test_gpu_lookahead.py holds every output
// bit for bit to ss_step's, which pins the restatement.
//
// Every function is SSD (host and device): tests/host/lookahead_host.cpp runs the same code on the CPU, the 64 lanes as threads.  The
// kernel and its launcher are in ss_lookahead.hip.
#pragma once
#include "ss_forces.hpp"

namespace ss {
namespace look {

// DEVICE rows of the m branches: obs [m, H, 60] (may be null), rew [m, H], done [m, H], final_state [m, 186] (may be null),
// work [m, SS_LOOK_WORK]
struct Out {
  float* obs;
  float* rew;
  uint8_t* done;
  float* final_state;
  float* work;
};

// A row of `work`: the terrain table of the branch with the provisional stones written out (words 65..184 of the packed state, what
// pack_env gives), the active stones in the layout of fstate's F_STONE rows, and the env-level scalars (the integers as their bits).
enum { W_TERR = 0, W_STONE = 120, W_POT = 144, W_ZINIT, W_EPRET, W_EPLO, W_NNDR, W_N, W_COUNT, W_ELAPSED, W_RNG, W_FLAGS, W_END };
static_assert(W_END <= SS_LOOK_WORK && SS_LOOK_WORK % 4 == 0, "a work row holds the branch's words, rows stay 16-byte aligned");
static_assert(SS_LOOK_MAX_STEPS == SS_MAX_EPISODE_STEPS, "no branch outlives an episode");

// Two words that a lane keeps across the substeps, in item 39 of LDS region A (free: ss_forces.hpp, kLdsNote): 1 + the step the branch
// finished in (0: it has not), and which of the float4 this lane copies out per step belong to rows that may be written (copy_obs).
// The Lds block has no room for the observation row a finished branch repeats, and a second block would cost the fourth workgroup of a
// CU: the row is read back from obs[k, f, :], which this wavefront wrote in step f.
constexpr int kLdsNote = kLdsHead + 3;
static_assert(kLdsNote < kSlotsA * 2, "the note is inside region A");
constexpr int kRow4 = SS_OBS_DIM / 4;                          // float4 per observation row
constexpr int kCopyIters = (kEnvsPerWave * kRow4 + kWave - 1) / kWave;
static_assert(kEnvsPerWave * SS_OBS_DIM <= kEnvsPerWave * 64, "the staged rows stay in front of region A's headings, as in emit_outputs");

SSD float i2f(int x) { return __builtin_bit_cast(float, x); }
SSD int f2i(float x) { return __builtin_bit_cast(int, x); }

// "every lane of the wavefront": the device votes; the host build, whose lanes are threads, never takes the short cut (the stores of a
// finished row are gated either way, so the results are the same)
#if defined(__HIP_DEVICE_COMPILE__)
#define SS_LOOK_ALL(pred) (__builtin_amdgcn_ballot_w64(!(pred)) == 0ull)
#else
#define SS_LOOK_ALL(pred) (false && (pred))
#endif

// draw_stone (ss_kernels.hpp) on the branch's own terrain table Tw [120]: the same draws from the env's counter, global id, curriculum
// and probability grid, the predecessor read from Tw (whose provisional stones are written out: 0.75 (k - 1), 0, 0, 0 are the words
// draw_stone takes for a stone that is not stored), the new stone written to Tw by the lane that stores
SSD float draw_stone_row(const Params& P, const Knobs& K, int e, uint32_t& ctr, int k, float* Tw, float out_p[3], float out_n[3],
                         float out_t[2], float out_h[2], bool store) {
  uint32_t r[4];
  env_block(P, e, ctr, r);
  int cell = sample_cell(P, K, e, u01(r[0]));
  float ratio = (float)K.curriculum / 5.0f;
  float dr = 0.65f + u01(r[1]) * (0.6f * ratio);
  float tilt = 15.0f * kDeg * ratio;
  float xt = (2.f * u01(r[2]) - 1.f) * tilt, yt = (2.f * u01(r[3]) - 1.f) * tilt;
  float yaw = yaw_sample(cell / SS_GRID), pitch = pitch_sample(cell % SS_GRID);
  const int kk = k < 1 ? 1 : (k > kNumStones - 1 ? kNumStones - 1 : k);      // (1 <= k <= 19 for every state ss_step accepts)
  const float* prev = Tw + (kk - 1) * 6;
  float px = prev[0], py = prev[1], pz = prev[2];
  float phi = prev[3] + yaw;
  float sp, cp, sph, cph;
  sincosf(pitch, &sp, &cp);
  sincosf(phi, &sph, &cph);
  place_stone(px, py, pz, dr, cp, sp, cph, sph, out_p);
  out_t[0] = xt; out_t[1] = yt;
  out_h[0] = cph; out_h[1] = sph;
  stone_normal(phi, xt, yt, out_n);
  if (store) {
    float* o = Tw + kk * 6;
    o[0] = out_p[0]; o[1] = out_p[1]; o[2] = out_p[2];
    o[3] = phi; o[4] = xt; o[5] = yt;
  }
  return dr;
}

// the clipped, lane-signed actions of one step into the lane's LDS column (the action clip of step_env)
SSD void put_actions(const float* act_row, int side, float m, const Lds& L) {
  float ain[NH];
  static_for<0, NH>([&](auto Kc) {
    constexpr int k = decltype(Kc)::value, jr = kHalf[k];
    constexpr int jl = left_twin(jr);
    ain[k] = act_row[side ? jl : jr];
  });
  static_for<0, NH>([&](auto Kc) {
    constexpr int k = decltype(Kc)::value, jr = kHalf[k];
    const float sg = action_lane_sign(jr, m);
    const float x = ain[k];
    float a = fminf(fmaxf(x, -1.f), 1.f);
    a = (x != x) ? x : a;      // a NaN action stays a NaN: it ends the episode (PHYSICS.md 4.8)
    L.s(S_ACT + k) = sg * a;
  });
}

// The private copy of env e in the row's work words.  The two lanes of the row share the terrain table.
SSD void init_work(const Params& P, int e, int side, float* W) {
  const size_t np = (size_t)P.npad;
  const float* F = P.fstate + e;
  const float* T = P.terrain + e;
  const int prov = P.istate[e + I_PROV * np];
#pragma unroll 1
  for (int i = side * 60; i < side * 60 + 60; ++i) {
    const int k = i / 6;
    W[W_TERR + i] = k < prov ? T[(size_t)i * np] : (i % 6 == 0 ? 0.75f * (float)k : 0.f);      // pack_env's words
  }
  if (side == 0) {
#pragma unroll
    for (int i = 0; i < 24; ++i) W[W_STONE + i] = F[(F_STONE + i) * np];
    W[W_POT] = F[F_POT * np];
    W[W_ZINIT] = F[F_ZINIT * np];
    W[W_EPRET] = F[F_EPRET * np];
    W[W_EPLO] = F[F_EPRET_LO * np];
    W[W_NNDR] = F[F_NNDR * np];
    W[W_N] = i2f(P.istate[e + I_N * np]);
    W[W_COUNT] = i2f(P.istate[e + I_COUNT * np]);
    W[W_ELAPSED] = i2f(P.istate[e + I_ELAPSED * np]);
    W[W_RNG] = i2f(P.istate[e + I_RNG * np]);
    W[W_FLAGS] = i2f(P.istate[e + I_FLAGS * np]);
  }
}

// The wavefront copies the staged observation rows of step s (LDS [32][60], rows back to back) to obs[row0 + r, s, :]: every row is 15
// contiguous float4; `okmask` bit i: the i-th float4 of this lane belongs to a row that may be written.
SSD void copy_obs(float* obs, int row0, int H, int s, int lane, uint32_t okmask, const float* lds) {
  const float4* s4 = reinterpret_cast<const float4*>(lds);
#pragma unroll
  for (int i = 0; i < kCopyIters; ++i) {
    const int g = lane + kWave * i;
    if ((okmask >> i) & 1u) {
      const int rl = g / kRow4, c4 = g - rl * kRow4;
      float4* dst = reinterpret_cast<float4*>(obs + ((size_t)(row0 + rl) * (size_t)H + (size_t)s) * SS_OBS_DIM) + c4;
      copy_out(dst, s4[g]);
    }
  }
}

// One branch: lane `lane_global` = 2 * row + side.  A row >= m or an env id outside [0, N) runs the whole body on a valid env (the
// lane-pair exchanges need both lanes, the wavefront runs in lockstep) and stores nothing outside `work`; a row >= m stores nothing at all.
// A finished branch keeps running too, with every store gated to the frozen values.
template <class Model>
SSD void look_row(const Params& P, const int32_t* env_ids, int m, int H, const float* act, const Out& out, int lane_global, int lane,
                  float* lds) {
  const int row_raw = lane_global >> 1, side = lane_global & 1;
  int row = row_raw < m ? row_raw : m - 1;                  // m >= 1
  const int e_raw = env_ids ? env_ids[row] : row;
  const bool own = row_raw < m;                              // the work row is this lane pair's
  const bool valid = own && e_raw >= 0 && e_raw < P.n;
  const int e = valid ? e_raw : P.n - 1;
  const float m_ = side ? -1.f : 1.f;                        // y-mirror factor of this lane's world
  const int row0 = (lane_global - lane) >> 1;                // first row of this wavefront
  const Lds L{lds, lane};
  frc::load_row(P, e, act + (size_t)row * (size_t)H * NJ, side, m_, L);
  if (own) init_work(P, e, side, out.work + (size_t)row * SS_LOOK_WORK);
  {
    uint32_t okmask = 0;
#pragma unroll
    for (int i = 0; i < kCopyIters; ++i) {
      const int g = lane + kWave * i, rr = row0 + g / kRow4;
      if (g < kEnvsPerWave * kRow4 && rr < m) {
        const int id = env_ids ? env_ids[rr] : rr;
        if (id >= 0 && id < P.n) okmask |= 1u << i;
      }
    }
    L.q2(kLdsNote) = make_float2(i2f(0), i2f((int)okmask));
  }
  SS_MEMBAR();

#pragma unroll 1
  for (int s = 0; s < H; ++s) {
    const int fin = f2i(L.q2(kLdsNote).x);                   // finished in an earlier step: 1 + that step
    float r_out = 0.f;
    int d_out = 1;
    // wavefront-uniform: nothing of this wavefront is left to compute, the frozen rows below are all that remains
    if (!SS_LOOK_ALL(fin != 0 || !valid)) {
      put_actions(act + ((size_t)row * (size_t)H + (size_t)s) * NJ, side, m_, L);
      const float power = P.knobs->power;
      FootReport fr;
#if defined(SS_PROFILE_PHASES) && defined(__HIP_DEVICE_COMPILE__)
      Prof prof;
#pragma unroll
      for (int i = 0; i < 16; ++i) prof.t[i] = 0;
      prof.last = (uint32_t)__builtin_amdgcn_s_memtime();
#endif
      Warm wm;                                               // every control step starts cold
      warm_clear(wm);
      if constexpr (warm_in_lds(0)) L.s(S_WKEY) = 0.f;
#pragma unroll 1
      for (int k = 0; k < kNumSubsteps; ++k) substep<Model, 0, false>(SS_PROF_ARG power, fr, L, wm);
      SS_MEMBAR();
      SS_OPAQUE(row);                                        // form the row addresses again instead of keeping them across the substeps
      float* W = out.work + (size_t)row * SS_LOOK_WORK;
      const bool live = fin == 0;
      const bool store = own && side == 0 && live;           // the lane that writes the branch's words
      const Knobs K = *P.knobs;
      Cache c;                                               // true world
#pragma unroll
      for (int sl = 0; sl < 3; ++sl) {
#pragma unroll
        for (int i = 0; i < 3; ++i) { c.p[sl][i] = W[W_STONE + sl * 8 + i]; c.nrm[sl][i] = W[W_STONE + sl * 8 + 3 + i]; }
        c.tilt[sl][0] = W[W_STONE + sl * 8 + 6];
        c.tilt[sl][1] = W[W_STONE + sl * 8 + 7];
      }
      float pot_prev = W[W_POT], z_init = W[W_ZINIT];
      float ep_ret = W[W_EPRET], ep_lo = W[W_EPLO], nn_dr = W[W_NNDR];
      int n = f2i(W[W_N]), count = f2i(W[W_COUNT]), elapsed = f2i(W[W_ELAPSED]);
      uint32_t ctr = (uint32_t)f2i(W[W_RNG]);

      // ---- step_env sections 3-10, restated (ss_kernels.hpp); no reset branch: a branch never resets ----
      // 3-4. back to the true world; the pair shares its feet
      float pos[3], quat[4];
      SV v0;
      get_base(L, m_, pos, quat, v0);
      elapsed += 1;
      const float my_sole[3] = {fr.sole[0], m_ * fr.sole[1], fr.sole[2]};
      float ot_sole[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) ot_sole[i] = xchg(my_sole[i]);
      const int ot_contact = xchg_i(fr.contact), ot_target = xchg_i(fr.on_target);
      float sole[2][3];
#pragma unroll
      for (int i = 0; i < 3; ++i) { sole[0][i] = side ? ot_sole[i] : my_sole[i]; sole[1][i] = side ? my_sole[i] : ot_sole[i]; }
      const int flags = side ? (ot_contact | (fr.contact << 1)) : (fr.contact | (ot_contact << 1));
      const int on_target = fr.on_target | ot_target;
      // partial sums over this lane's joints (the spine is counted by the right lane only)
      float accv = 0.f, e_sum = 0.f, a2 = 0.f;
      int at_limit = 0;
      static_for<0, NH>([&](auto Kc) {
        constexpr int k = decltype(Kc)::value, jr = kHalf[k];
        constexpr float mid = 0.5f * (Model::lo[jr] + Model::hi[jr]);
        constexpr float span = Model::hi[jr] - Model::lo[jr];
        const float q = L.s(S_Q + k), qd = L.s(S_QD + k), a = L.s(S_ACT + k);
        const bool mine = (jr >= 3) || (side == 0);
        accv += q + qd;
        if (mine) {
          e_sum += fabsf(a * (0.1f * qd));
          a2 += a * a;
          if (fabsf(2.f * (q - mid) / span) > 0.99f) at_limit += 1;
        }
      });
      accv += pos[0] + pos[1] + pos[2] + quat[0] + quat[1] + quat[2] + quat[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) accv += v0.w[i] + v0.v[i];
      e_sum += xchg(e_sum);
      a2 += xchg(a2);
      at_limit += xchg_i(at_limit);
      const bool finite = finite_bits(accv) && (xchg_i(finite_bits(accv) ? 1 : 0) != 0);

      // 5. target logic
      float target_old[3] = {c.p[1][0], c.p[1][1], c.p[1][2]};
      float step_bonus = 0.f;
      int advanced = 0;
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
          // the headings move with the stones: slot 2 from the draw (at n = 19 it keeps the last stone's); they live in LDS only
          const float2 h1 = L.q2(kLdsHead + 1), h2 = L.q2(kLdsHead + 2);
          float h_new[2] = {h2.x, m_ * h2.y};
          if (n + 1 <= kNumStones - 1)
            nn_dr = draw_stone_row(P, K, e, ctr, n + 1, W + W_TERR, c.p[2], c.nrm[2], c.tilt[2], h_new, store);
          L.q2(kLdsHead + 0) = h1;
          L.q2(kLdsHead + 1) = h2;
          L.q2(kLdsHead + 2) = make_float2(h_new[0], m_ * h_new[1]);
        }
      }
      // 6. progress
      float pot = -planar_dist(target_old, pos) / kDt;
      float progress = pot - pot_prev;
      pot_prev = advanced ? -planar_dist(c.p[1], pos) / kDt : pot;
      // 7-8
      float target_bonus = (n == kNumStones - 1 && planar_dist(c.p[1], pos) < 0.15f) ? 2.f : 0.f;
      float zs = fminf(sole[0][2], sole[1][2]);
      float tall_bonus = (pos[2] - zs > 0.7f) ? 2.f : -1.f;
      float zlow = fminf(fminf(c.p[0][2], c.p[1][2]), c.p[2][2]);
      bool d = (tall_bonus < 0.f) || (pos[2] < zlow + 0.3f) || !finite;
      bool timeout = elapsed >= SS_MAX_EPISODE_STEPS;
      d = d || timeout;
      // 9. reward
      float roll, pitch, cyaw, syaw;
      quat_roll_pitch_cs(quat, roll, pitch, cyaw, syaw);
      float posture = 0.f;
      if (!(pitch > -0.2f && pitch < 0.4f)) posture += fabsf(pitch);
      if (!(roll > -0.4f && roll < 0.4f)) posture += fabsf(roll);
      float energy = (4.5f / NJ) * (e_sum / NJ) + (0.225f / NJ) * (a2 / NJ);
      float r = progress + step_bonus + target_bonus + tall_bonus - energy - posture - 0.1f * (float)at_limit;
      if (!finite || !finite_bits(r)) r = 0.f;
      {   // episode return as an unevaluated float pair: error-free two-sum of the step reward, then renormalised
        const float sm = ep_ret + r, bb = sm - ep_ret;
        const float err = (ep_ret - (sm - bb)) + (r - bb);
        const float lo = ep_lo + err;
        ep_ret = sm + lo;
        ep_lo = lo - (ep_ret - sm);
      }
      // joint values of this lane in the true world
      float qt[NH], qdt[NH];
      get_joints(L, m_, qt, qdt);
      // the LDS copy of the stones is what the next step's substeps read (the ROLLOUT path of step_env)
      if (advanced) {
#pragma unroll
        for (int sl = 0; sl < 3; ++sl) {
          L.s(S_STP + sl * 3 + 0) = c.p[sl][0]; L.s(S_STP + sl * 3 + 1) = m_ * c.p[sl][1]; L.s(S_STP + sl * 3 + 2) = c.p[sl][2];
          L.s(S_STN + sl * 3 + 0) = c.nrm[sl][0]; L.s(S_STN + sl * 3 + 1) = m_ * c.nrm[sl][1]; L.s(S_STN + sl * 3 + 2) = c.nrm[sl][2];
        }
      }
      // ---- end of the restated lines ----

      if (live) {
        r_out = r;
        d_out = d ? 1 : 0;
      }
      // 10. the observation row of a live branch: staged in LDS region A as emit_outputs does
      if (out.obs) {
        SS_WAVE_SYNC();          // the staging area is region A: every lane must be through with its contact operators
        if (live) {
          float* stage = lds + (lane >> 1) * SS_OBS_DIM;
#define SS_OBS(i, v) stage[i] = (v)
          static_for<0, NH>([&](auto Kc) {
            constexpr int k = decltype(Kc)::value, jr = kHalf[k];
            constexpr int jl = left_twin(jr);
            const int gj = side ? jl : jr;
            if (jr >= 3 || side == 0) {
              constexpr float midr = 0.5f * (Model::lo[jr] + Model::hi[jr]);
              constexpr float span = Model::hi[jr] - Model::lo[jr];
              const float ps = policy_true_sign(jr, side);
              const float mid = (side && mirror_flips(jr)) ? -midr : midr;
              SS_OBS(6 + gj, obs_angle(ps, qt[k], mid, span));
              SS_OBS(27 + gj, obs_rate(ps, qdt[k]));
            }
          });
          if (side == 0) {
            float R[3][3];
            quat_rot(quat, R);
            float vw[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) vw[i] = R[i][0] * v0.v[0] + R[i][1] * v0.v[1] + R[i][2] * v0.v[2];
            SS_OBS(0, clip5(pos[2] - z_init));
            SS_OBS(1, clip5(cyaw * vw[0] + syaw * vw[1]));
            SS_OBS(2, clip5(-syaw * vw[0] + cyaw * vw[1]));
            SS_OBS(3, clip5(vw[2]));
            SS_OBS(4, clip5(roll));
            SS_OBS(5, clip5(pitch));
            SS_OBS(48, (flags & 1) ? 1.f : 0.f);
            SS_OBS(49, (flags & 2) ? 1.f : 0.f);
            float t[5];
            target_features(pos, cyaw, syaw, c.p[1], c.tilt[1], t);
#pragma unroll
            for (int i = 0; i < 5; ++i) SS_OBS(50 + i, t[i]);
            target_features(pos, cyaw, syaw, c.p[2], c.tilt[2], t);
#pragma unroll
            for (int i = 0; i < 5; ++i) SS_OBS(55 + i, t[i]);
          }
#undef SS_OBS
        }
      }
      // the dynamic state the branch ends in: the finishing step's, or the last step's
      if (valid && live && out.final_state && (d || s == H - 1)) {
        float* o = out.final_state + (size_t)row * SS_STATE_DIM;
        static_for<0, NH>([&](auto Kc) {
          constexpr int k = decltype(Kc)::value, jr = kHalf[k];
          constexpr int jl = left_twin(jr);
          if (jr >= 3 || side == 0) {
            o[F_Q + (side ? jl : jr)] = qt[k];
            o[F_QD + (side ? jl : jr)] = qdt[k];
          }
        });
        if (side == 0) {
#pragma unroll
          for (int i = 0; i < 3; ++i) o[F_POS + i] = pos[i];
#pragma unroll
          for (int i = 0; i < 4; ++i) o[F_QUAT + i] = quat[i];
#pragma unroll
          for (int i = 0; i < 3; ++i) { o[F_VEL + i] = v0.w[i]; o[F_VEL + 3 + i] = v0.v[i]; }
        }
      }
      // the env-level words of the branch
      if (store) {
        if (advanced) {
#pragma unroll
          for (int sl = 0; sl < 3; ++sl) {
#pragma unroll
            for (int i = 0; i < 3; ++i) { W[W_STONE + sl * 8 + i] = c.p[sl][i]; W[W_STONE + sl * 8 + 3 + i] = c.nrm[sl][i]; }
            W[W_STONE + sl * 8 + 6] = c.tilt[sl][0];
            W[W_STONE + sl * 8 + 7] = c.tilt[sl][1];
          }
        }
        W[W_POT] = pot_prev;
        W[W_EPRET] = ep_ret;
        W[W_EPLO] = ep_lo;
        W[W_NNDR] = nn_dr;
        W[W_N] = i2f(n);
        W[W_COUNT] = i2f(count);
        W[W_ELAPSED] = i2f(elapsed);
        W[W_RNG] = i2f((int)ctr);
        W[W_FLAGS] = i2f(flags);
      }
      if (live && d) L.q2(kLdsNote).x = i2f(s + 1);
      SS_MEMBAR();
    }

    // the step's rows: a finished branch repeats its last observation, earns nothing and stays done
    if (out.obs) {
      if (fin != 0) {          // the terminal row again: 15 float4, eight by the right lane, seven by the left
        float4* stage = reinterpret_cast<float4*>(lds + (lane >> 1) * SS_OBS_DIM);
        const float4* term = reinterpret_cast<const float4*>(out.obs + ((size_t)row * (size_t)H + (size_t)(fin - 1)) * SS_OBS_DIM);
#pragma unroll 1
        for (int i = side * 8; i < (side ? kRow4 : 8); ++i) stage[i] = term[i];
      }
      SS_WAVE_SYNC();
      copy_obs(out.obs, row0, H, s, lane, (uint32_t)f2i(L.q2(kLdsNote).y), lds);
      SS_WAVE_SYNC();            // region A belongs to the substeps again
    }
    if (valid && side == 0) {
      out.rew[(size_t)row * (size_t)H + (size_t)s] = r_out;
      out.done[(size_t)row * (size_t)H + (size_t)s] = d_out ? 1 : 0;
    }
  }
  SS_MEMBAR();

  // the rest of the state the branch ends in: the words of its private copy, in the ss_get_state layout
  if (valid && out.final_state) {
    const float* W = out.work + (size_t)row * SS_LOOK_WORK;
    float* o = out.final_state + (size_t)row * SS_STATE_DIM;
#pragma unroll 1
    for (int i = side * 60; i < side * 60 + 60; ++i) o[65 + i] = W[W_TERR + i];
    if (side == 0) {
      o[F_POT] = W[W_POT];
      o[F_ZINIT] = W[W_ZINIT];
      o[F_EPRET] = W[W_EPRET];
      o[F_NNDR] = W[W_NNDR];
      o[59] = (float)f2i(W[W_N]);
      o[60] = (float)f2i(W[W_COUNT]);
      o[61] = (float)f2i(W[W_ELAPSED]);
      const uint32_t ctr = (uint32_t)f2i(W[W_RNG]);
      o[62] = (float)(ctr & 0xFFFFu);
      o[63] = (float)(ctr >> 16);
      o[64] = (float)f2i(W[W_FLAGS]);
      o[185] = W[W_EPLO];
    }
  }
}

}  // namespace look
}  // namespace ss
