// ss_lookahead.hpp -- look-ahead (docs/PHYSICS.md "Look-ahead" is the specification): H control steps of ss_step, with auto-reset off, on a
// PRIVATE copy of an env, under a caller-supplied action sequence -- one row ("branch") per (env id, action sequence), any number of rows
// per env.  Every step's observation, reward and done flag and the state the branch ends in come back; nothing of the env is written.
//
// The per-lane code re-composes the step kernels' device functions on the plain step kernel's shape, as ss_forces.hpp does: two lanes per
// row, one wavefront per workgroup, one Lds block, the dynamic state resident in LDS across the H steps (the ROLLOUT path of step_env).
// What a control step reads or writes besides the dynamic state -- the active stones, the terrain row, the target counters, the episode
// statistics, the RNG counter -- lives in the row's `work` words (W_* below), where the step kernel has the env's own arrays: loaded
// after the substeps, stored by the right lane, so that nothing is held in registers across substep().  The env logic of a control step
// is one definition with step_env's (ss_kernels.hpp): load_in, put_actions, step_logic (sections 3-9; step_env keeps sections 3-5 inline
// and the reset branch, and calls step_score / ep_return_add of sections 6-9 as step_logic does), put_stones and stage_obs_joint /
// stage_obs_base.  What look_row adds is where the words live: the draw of an advance reads and writes the row's private terrain table
// (sample_stone and stone_after around it are draw_stone's).  tests/test_gpu_lookahead.py holds every output bit for bit to ss_step's.
//
// Every function is SSD (host and device): tests/host/lookahead_host.cpp runs the same code on the CPU, the 64 lanes as threads.  The
// kernel and its launcher are in ss_lookahead.hip.
//
// Branches from caller-supplied states (ss_lookahead_states; PHYSICS.md 13 "Branches from caller-supplied states"): look_row<Model, true>
// is the same function with another prologue -- the lane's half of the dynamic state, the stones and headings and the work row come from
// row k of a packed [m,186] array (the ss_get_state layout) through unpack_env's conversions, where look_row<Model, false> reads env
// env_ids[k]'s arrays.  The env still gives the global id (the Philox key), its row of a per-env probability grid and the knobs.  The
// H-step loop and the epilogue are one text for both.  obs_from_row is the observation of such a row (ss_get_obs_states).
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

// Two words that a lane keeps across the substeps, in kLdsNote (ss_kernels.hpp): 1 + the step the branch finished in (0: it has not),
// and which of the float4 this lane copies out per step belong to rows that may be written (copy_obs).
// The Lds block has no room for the observation row a finished branch repeats, and a second block would cost the fourth workgroup of a
// CU: the row is read back from obs[k, f, :], which this wavefront wrote in step f.
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

// ---- a packed state row (the ss_get_state layout) as the source ----
// The integer words of a row, as unpack_env reads them: (int) / (uint32_t) of the float.  Written out so that every float has a defined
// result on the host as well: what v_cvt_i32_f32 / v_cvt_u32_f32 give (saturation; NaN: 0).
SSD int row_int(float x) {
  return x != x ? 0 : (x >= 2147483648.f ? 2147483647 : (x < -2147483648.f ? -2147483647 - 1 : (int)x));
}
SSD uint32_t row_u32(float x) { return !(x > 0.f) ? 0u : (x >= 4294967296.f ? 0xFFFFFFFFu : (uint32_t)x); }
SSD uint32_t row_rng(const float* S) { return row_u32(S[62]) | (row_u32(S[63]) << 16); }

// cache_from_terrain on the row's own terrain words (S[65 + 6 k ..]): the active stones n-1, n, n+1 of n = word 59 and the cos / sin of
// their headings.  n is clamped into [0, 19] first, so that no row, whatever it holds, reads outside its 120 terrain words; for every state
// ss_step accepts (1 <= n <= 19) the three indices are cache_from_terrain's.
SSD void cache_from_row(const float* S, Cache& c, float (&hd)[3][2]) {
  const int n_raw = row_int(S[59]);
  const int n = n_raw < 0 ? 0 : (n_raw > kNumStones - 1 ? kNumStones - 1 : n_raw);
  const int idx[3] = {n - 1 < 0 ? 0 : n - 1, n, n + 1 > kNumStones - 1 ? kNumStones - 1 : n + 1};
#pragma unroll
  for (int sl = 0; sl < 3; ++sl) {
    const float* T = S + 65 + idx[sl] * 6;
#pragma unroll
    for (int i = 0; i < 3; ++i) c.p[sl][i] = T[i];
    const float phi = T[3], xt = T[4], yt = T[5];
    c.tilt[sl][0] = xt; c.tilt[sl][1] = yt;
    stone_normal(phi, xt, yt, c.nrm[sl]);
    sincosf(phi, &hd[sl][1], &hd[sl][0]);
  }
}

// load_in from a row: the stones and headings and the lane's half of the dynamic state into the lane's LDS columns (words 0..54 of a row
// are fstate's F_POS .. F_QD).  c: the active stones, for init_work_row.
SSD void load_in_row(const float* S, int side, float m, const Lds& L, Cache& c) {
  float hd[3][2];
  cache_from_row(S, c, hd);
  put_stones(L, m, c, hd);
  float gin[13], qin[NH], qdin[NH];
#pragma unroll
  for (int i = 0; i < 13; ++i) gin[i] = S[F_POS + i];
  static_for<0, NH>([&](auto Kc) {
    constexpr int k = decltype(Kc)::value, jr = kHalf[k];
    constexpr int jl = left_twin(jr);
    const int gj = side ? jl : jr;
    qin[k] = S[F_Q + gj];
    qdin[k] = S[F_QD + gj];
  });
  put_base(L, m, gin, gin + 3, gin + 7, gin + 10);
  put_joints(L, m, qin, qdin);
}

// init_work from a row: all 20 terrain rows as stored (unpack_env sets prov = 20), the active stones as load_in_row made them, the
// env-level scalars through unpack_env's conversions
SSD void init_work_row(const float* S, const Cache& c, int side, float* W) {
#pragma unroll 1
  for (int i = side * 60; i < side * 60 + 60; ++i) W[W_TERR + i] = S[65 + i];
  if (side == 0) {
#pragma unroll
    for (int sl = 0; sl < 3; ++sl) {
#pragma unroll
      for (int i = 0; i < 3; ++i) { W[W_STONE + sl * 8 + i] = c.p[sl][i]; W[W_STONE + sl * 8 + 3 + i] = c.nrm[sl][i]; }
      W[W_STONE + sl * 8 + 6] = c.tilt[sl][0];
      W[W_STONE + sl * 8 + 7] = c.tilt[sl][1];
    }
    W[W_POT] = S[F_POT];
    W[W_ZINIT] = S[F_ZINIT];
    W[W_EPRET] = S[F_EPRET];
    W[W_EPLO] = S[185];
    W[W_NNDR] = S[F_NNDR];
    W[W_N] = i2f(row_int(S[59]));
    W[W_COUNT] = i2f(row_int(S[60]));
    W[W_ELAPSED] = i2f(row_int(S[61]));
    W[W_RNG] = i2f((int)row_rng(S));
    W[W_FLAGS] = i2f(row_int(S[64]));
  }
}

// The observation of a state row (ss_get_obs_states): write_obs over the row's dynamic state and active stones -- what obs_kernel writes
// for an env that unpack_env has put the row into.  It depends on no id and no knob.
template <class Model>
SSD void obs_from_row(const float* S, float* o) {
  Dyn s;
#pragma unroll
  for (int i = 0; i < 3; ++i) s.pos[i] = S[F_POS + i];
#pragma unroll
  for (int i = 0; i < 4; ++i) s.quat[i] = S[F_QUAT + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) { s.v0.w[i] = S[F_VEL + i]; s.v0.v[i] = S[F_VEL + 3 + i]; }
#pragma unroll
  for (int j = 0; j < NJ; ++j) { s.q[j] = S[F_Q + j]; s.qd[j] = S[F_QD + j]; }
  Cache c;
  float hd[3][2];
  cache_from_row(S, c, hd);
  write_obs<Model>(s, S[F_ZINIT], row_int(S[64]), c, o);
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

// Where a branch's actions come from, a compile-time choice of look_row.  ActGiven: row s of the caller's sequence act[k, s, :]
// (load_actions), the look-ahead as it was.  A source with kPolicy (ss_policy.hpp) computes them between the control steps from the
// observation rows staged in LDS region A, which look_row then stages whether or not the caller asked for obs:
//   root_obs<Model, ROWS>(P, e, states, row, lane, lds)   the observation at the branch's root into the lane pair's staged row
//   phase(lds, lane)                            every wavefront of the workgroup: staged rows -> the wavefront's 32 action rows
//   emit(row, H, s, lane, valid, live)          adds the row's offset, reports the action (zeros for a finished branch)
//   load(lane, side, ain)                       load_actions from those rows
struct ActGiven { static constexpr bool kPolicy = false; };

// One branch: lane `lane_global` = 2 * row + side.  A row >= m or an env id outside [0, N) runs the whole body on a valid env (the
// lane-pair exchanges need both lanes, the wavefront runs in lockstep) and stores nothing outside `work`; a row >= m stores nothing at all.
// A finished branch keeps running too, with every store gated to the frozen values.
// ROWS: the branch starts from states[row, :] instead of env e's state (a row >= m or a bad id runs on the row the lane pair was clamped
// to, which is inside `states` either way); e stays the env whose id, probability grid and knobs the draws use.
template <class Model, bool ROWS = false, class Src = ActGiven>
SSD void look_row(const Params& P, const int32_t* env_ids, int m, int H, const float* act, const Out& out, int lane_global, int lane,
                  float* lds, const float* states = nullptr, const Src& src = Src()) {
  const int row_raw = lane_global >> 1, side = lane_global & 1;
  int row = row_raw < m ? row_raw : m - 1;                  // m >= 1
  const int e_raw = env_ids ? env_ids[row] : row;
  const bool own = row_raw < m;                              // the work row is this lane pair's
  const bool valid = own && e_raw >= 0 && e_raw < P.n;
  const int e = valid ? e_raw : P.n - 1;
  const float m_ = side ? -1.f : 1.f;                        // y-mirror factor of this lane's world
  const int row0 = (lane_global - lane) >> 1;                // first row of this wavefront
  const Lds L{lds, lane};
  float ain[NH];
  if constexpr (ROWS) {
    const float* S = states + (size_t)row * SS_STATE_DIM;
    Cache c0;
    load_in_row(S, side, m_, L, c0);
    if (own) init_work_row(S, c0, side, out.work + (size_t)row * SS_LOOK_WORK);
  } else {
    load_in<false>(P, e, nullptr, side, m_, L, ain);          // (every step loads its own actions)
    if (own) init_work(P, e, side, out.work + (size_t)row * SS_LOOK_WORK);
  }
  if constexpr (Src::kPolicy) src.template root_obs<Model, ROWS>(P, e, states, row, lane, lds);
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
    if constexpr (Src::kPolicy) {
      src.phase(lds, lane);
      src.emit(row, H, s, lane, valid, fin == 0);
    }
    // wavefront-uniform: nothing of this wavefront is left to compute, the frozen rows below are all that remains
    if (!SS_LOOK_ALL(fin != 0 || !valid)) {
      if constexpr (Src::kPolicy) src.load(lane, side, ain);
      else load_actions(act + ((size_t)row * (size_t)H + (size_t)s) * NJ, side, ain);
      put_actions(L, m_, ain);
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

      // step_env sections 3-9 (step_logic); no reset branch: a branch never resets.  The stone of an advance is read from and written
      // to the branch's own terrain table, whose provisional stones are written out (0.75 (k - 1), 0, 0, 0 are the words draw_stone
      // takes for a stone that is not stored)
      StepEnd se;
      step_logic<Model>(SS_PROF_ARG L, side, m_, fr, c, pot_prev, nn_dr, ep_ret, ep_lo, n, count, elapsed, ctr, store,
                        [&](uint32_t& ct, int k, float* p, float* nrm, float* tilt, float* h, bool st) {
                          float xt, yt, yaw, pitch;
                          const float dr = sample_stone(P, K, e, ct, xt, yt, yaw, pitch);
                          const int kk = k < 1 ? 1 : (k > kNumStones - 1 ? kNumStones - 1 : k);      // (1 <= k <= 19 for every state ss_step accepts)
                          const float* prev = W + W_TERR + (kk - 1) * 6;
                          const float phi = prev[3] + yaw;
                          stone_after(prev[0], prev[1], prev[2], phi, dr, pitch, xt, yt, p, nrm, tilt, h);
                          if (st) {
                            float* o = W + W_TERR + kk * 6;
                            o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
                            o[3] = phi; o[4] = xt; o[5] = yt;
                          }
                          return dr;
                        }, se);
      const float (&pos)[3] = se.pos, (&quat)[4] = se.quat;
      const SV& v0 = se.v0;
      const int flags = se.flags, advanced = se.advanced;
      const bool d = se.d;
      const float r = se.r;
      // joint values of this lane in the true world
      float qt[NH], qdt[NH];
      get_joints(L, m_, qt, qdt);
      // the LDS copy of the stones is what the next step's substeps read (the ROLLOUT path of step_env)
      if (advanced) put_stones(L, m_, c);

      if (live) {
        r_out = r;
        d_out = d ? 1 : 0;
      }
      // 10. the observation row of a live branch: staged in LDS region A as emit_outputs does
      if (out.obs || Src::kPolicy) {
        SS_WAVE_SYNC();          // the staging area is region A: every lane must be through with its contact operators
        if (live) {
          float* stage = lds + (lane >> 1) * SS_OBS_DIM;
          static_for<0, NH>([&](auto Kc) {
            constexpr int k = decltype(Kc)::value;
            if (kHalf[k] >= 3 || side == 0) stage_obs_joint<Model, k>(stage, side, qt[k], qdt[k]);
          });
          if (side == 0)
            stage_obs_base(stage, pos, quat, v0, z_init, se.roll, se.pitch, se.cyaw, se.syaw, flags, c.p[1], c.tilt[1], c.p[2], c.tilt[2]);
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
