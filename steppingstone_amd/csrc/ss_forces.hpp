// ss_forces.hpp -- force readout of one control step (docs/PHYSICS.md "Force readout" is the specification): what the four substeps of
// ss_step WOULD do to an env under a given action -- the contact impulse of every sole corner per substep, as forces, the explicit and the
// applied torque of every joint, and the state the step would end in -- without touching the env.  A dry run: nothing is written to the
// env state, no reward, termination, target logic or reset is evaluated.
//
// The per-lane code re-composes the step kernels' own device functions (substep<Model, 0>, fk_detect, joint_limit, joint_tau) on the
// plain step kernel's shape: two lanes per env (lane 2r: right half of row r, lane 2r + 1: left half in its y-mirrored world), one
// wavefront per workgroup, one Lds block.  The load-in and the action clip are step_env's own (load_in, put_actions);
// tests/test_gpu_step_forces.py holds next_state to ss_step's own result bit for bit.
//
// Every function is SSD (host and device): tests/host/forces_host.cpp runs the same code on the CPU, the 64 lanes as threads.  The
// kernel and its launcher are in ss_forces.hip.
#pragma once
#include "ss_kernels.hpp"

namespace ss {
namespace frc {

// DEVICE rows of the m requested envs; any may be null (the stores are gated, nothing else):
//   contacts [m, 4, 8, 8], joints [m, 4, 4, 21], next_state [m, 56]
struct Out {
  float* contacts;
  float* joints;
  float* next_state;
};

// What a lane remembers across a substep call besides the state in LDS.  The note (two words: the detection of the substep's start and
// the limit switches of the lane's joints) lives in kLdsNote (ss_kernels.hpp).  The twelve words of Carry are the only values held in
// registers across the call: as many as the Warm record, which the plain variant of substep leaves unused (its impulses live in
// S_WLAM / S_WKEY).
struct Carry {
  float t[NH];      // tau_j + c_j qd_j / h, this lane's world (c_j: implicit_gain)
};

constexpr float kInvH = 240.0f;      // 1 / kH, exact
static_assert(kInvH * kH == 1.0f, "h = 1 / 240 s");

// Dadd_j - armature_j of PHYSICS.md 3.1 from the joint's limit gains (0 inside the range): h (kd + dl) + h^2 (ks + kl).  Formed without
// the armature, which dominates Dadd_j and would leave the difference few bits.
template <class Model, int J>
SSD float implicit_gain(float kl, float dl) {
  constexpr float h = kH;
  constexpr float kd = Model::damping[J], ks = Model::stiffness[J];
  return h * (kd + dl) + (h * h) * (ks + kl);
}

// Before substep s: joint rows 0..2 (q, qd, tau of the substep's start), the detection of the substep's start (contacts words 0 and 1),
// the note and the carry.
template <class Model>
SSD void before_substep(float power, const Lds& L, int side, float m, bool store, float* crow, float* jrow, Carry& cy) {
  float q[NH], qd[NH], a[NH];
#pragma unroll
  for (int k = 0; k < NH; ++k) { q[k] = L.s(S_Q + k); qd[k] = L.s(S_QD + k); a[k] = L.s(S_ACT + k); }
  SS_MEMBAR();
  uint32_t limits = 0;
  static_for<0, NH>([&](auto Kc) {
    constexpr int k = decltype(Kc)::value, jr = kHalf[k];
    constexpr int jl = left_twin(jr);
    float tau, Dadd, viol, kl, dl;
    joint_tau<Model, jr>(power, q[k], qd[k], a[k], tau, Dadd);
    joint_limit<Model, jr>(q[k], viol, kl, dl);          // the same switches joint_tau has just taken
    limits |= (viol != 0.f ? 1u : 0u) << k;
    cy.t[k] = tau + implicit_gain<Model, jr>(kl, dl) * (kInvH * qd[k]);
    if (store && jrow && (jr >= 3 || side == 0)) {       // own limbs by each lane, the spine by the right lane
      const float sg = mirror_sign(jr, m);
      const int gj = side ? jl : jr;
      jrow[0 * NJ + gj] = sg * q[k];
      jrow[1 * NJ + gj] = sg * qd[k];
      jrow[2 * NJ + gj] = sg * tau;
    }
  });
  // the detection substep<Model, 0> runs on this state: same function, same inputs
  float cs8[8], sn8[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) ss_sincos(q[k], sn8[k], cs8[k]);
  const float quat[4] = {L.s(S_QUAT), L.s(S_QUAT + 1), L.s(S_QUAT + 2), L.s(S_QUAT + 3)};
  float Rb[3][3];
  quat_rot(quat, Rb);
  DetectOut det;
  FootReport fr;
  fk_detect<Model>(cs8, sn8, Rb, L, det, fr);
  L.q2(kLdsNote) = make_float2(__builtin_bit_cast(float, det.active | (det.cslot << 4)), __builtin_bit_cast(float, limits));
  if (store && crow) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool on = (det.active >> k) & 1;
      const int sl = (det.cslot >> (2 * k)) & 3;
      float2* dst = reinterpret_cast<float2*>(crow + (4 * side + k) * SS_FRC_CONTACT);
      dst[0] = make_float2(on ? (float)sl : -1.f, on ? det.pen[k] : 0.f);
    }
  }
}

// After substep s: the impulses it left as forces (contacts words 2..7) and the applied torque (joint row 3)
template <class Model>
SSD void after_substep(const Lds& L, int side, float m, bool store, float* crow, float* jrow, const Carry& cy) {
  const float2 note = L.q2(kLdsNote);
  const int det = __builtin_bit_cast(int, note.x);
  const uint32_t limits = __builtin_bit_cast(uint32_t, note.y);
  const int key = __builtin_bit_cast(int, L.s(S_WKEY));      // the corners the solver ran on: the detection's, 0 without a contact
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool on = (key >> k) & 1;
    const int sl = (det >> (4 + 2 * k)) & 3;
    float f[3], n[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) f[d] = on ? L.s(S_WLAM + 3 * k + d) * kInvH : 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) n[i] = on ? L.s(S_STN + sl * 3 + i) : (i == 2 ? 1.f : 0.f);
    // n, t1, t2 of the row set-up (jacobian_rows), this lane's world
    float t1[3] = {1.f - n[0] * n[0], -n[0] * n[1], -n[0] * n[2]};
    const float inv = SS_RSQRT(t1[0] * t1[0] + t1[1] * t1[1] + t1[2] * t1[2]);
    t1[0] *= inv; t1[1] *= inv; t1[2] *= inv;
    float t2[3];
    cross(n, t1, t2);
    float w[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = f[0] * n[i] + f[1] * t1[i] + f[2] * t2[i];
    if (store && crow) {
      // true world: the left lane's t2 is minus the mirror image of the true one, a vector mirrors in y
      float* dst = crow + (4 * side + k) * SS_FRC_CONTACT;
      *reinterpret_cast<float2*>(dst + 2) = make_float2(f[0], f[1]);
      *reinterpret_cast<float4*>(dst + 4) = make_float4(m * f[2], w[0], m * w[1], w[2]);
    }
  }
  static_for<0, NH>([&](auto Kc) {
    constexpr int k = decltype(Kc)::value, jr = kHalf[k];
    constexpr int jl = left_twin(jr);
    const bool out = (limits >> k) & 1;
    const float kl = out ? Model::klim[jr] : 0.f, dl = out ? Model::dlim[jr] : 0.f;
    const float applied = cy.t[k] - implicit_gain<Model, jr>(kl, dl) * (kInvH * L.s(S_QD + k));
    if (store && jrow && (jr >= 3 || side == 0)) jrow[3 * NJ + (side ? jl : jr)] = mirror_sign(jr, m) * applied;
  });
}

// substep s of requested row `row` in the outputs (null when the output is not asked for)
SSD float* contact_rows(const Out& out, int row, int s) {
  return out.contacts ? out.contacts + ((size_t)row * SS_FRC_SUBSTEPS + s) * (8 * SS_FRC_CONTACT) : nullptr;
}
SSD float* joint_rows(const Out& out, int row, int s) {
  return out.joints ? out.joints + ((size_t)row * SS_FRC_SUBSTEPS + s) * (SS_FRC_JOINT * NJ) : nullptr;
}

// One requested row: lane `lane_global` = 2 * row + side.  A row >= m or an env id outside [0, N) runs the whole body on a valid env
// (the lane-pair exchanges need both lanes, the wavefront runs in lockstep) and stores nothing.
template <class Model>
SSD void forces_row(const Params& P, const int32_t* env_ids, int m, const float* act, const Out& out, int lane_global, int lane, float* lds) {
  const int row_raw = lane_global >> 1, side = lane_global & 1;
  int row = row_raw < m ? row_raw : m - 1;                  // m >= 1
  const int e_raw = env_ids ? env_ids[row] : row;
  const bool valid = row_raw < m && e_raw >= 0 && e_raw < P.n;
  const int e = valid ? e_raw : P.n - 1;
  const float m_ = side ? -1.f : 1.f;                        // y-mirror factor of this lane's world
  const Lds L{lds, lane};
  float ain[NH];
  load_in<true>(P, e, act + (size_t)row * NJ, side, m_, L, ain);      // what step_env has in LDS before its first substep
  put_actions(L, m_, ain);

  const float power = P.knobs->power;
  FootReport fr;
  Warm wm;                                                   // every control step starts cold
  warm_clear(wm);
  if constexpr (warm_in_lds(0)) L.s(S_WKEY) = 0.f;
#if defined(SS_PROFILE_PHASES) && defined(__HIP_DEVICE_COMPILE__)
  Prof prof;
#pragma unroll
  for (int i = 0; i < 16; ++i) prof.t[i] = 0;
  prof.last = (uint32_t)__builtin_amdgcn_s_memtime();
#endif
#pragma unroll 1
  for (int s = 0; s < kNumSubsteps; ++s) {
    Carry cy;
    before_substep<Model>(power, L, side, m_, valid, contact_rows(out, row, s), joint_rows(out, row, s), cy);
    SS_MEMBAR();
    substep<Model, 0, false>(SS_PROF_ARG power, fr, L, wm);
    SS_MEMBAR();
    SS_OPAQUE(row);                                          // form the row addresses again instead of keeping them across the substep
    after_substep<Model>(L, side, m_, valid, contact_rows(out, row, s), joint_rows(out, row, s), cy);
  }
  SS_MEMBAR();

  // the state the step would end in, true world, and the last detector's foot flags
  float pos[3], quat[4], qt[NH], qdt[NH];
  SV v0;
  get_base(L, m_, pos, quat, v0);
  get_joints(L, m_, qt, qdt);
  const int ot_contact = xchg_i(fr.contact), ot_target = xchg_i(fr.on_target);
  const int flags = side ? (ot_contact | (fr.contact << 1) | (ot_target << 2) | (fr.on_target << 3))
                         : (fr.contact | (ot_contact << 1) | (fr.on_target << 2) | (ot_target << 3));
  if (valid && out.next_state) {
    float* o = out.next_state + (size_t)row * SS_FRC_STATE;
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
      o[SS_FRC_STATE - 1] = (float)flags;
    }
  }
}

}  // namespace frc
}  // namespace ss
