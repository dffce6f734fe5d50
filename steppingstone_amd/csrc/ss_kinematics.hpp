// ss_kinematics.hpp -- whole-body kinematic readout of the packed state (docs/PHYSICS.md "Kinematic readout" is the specification;
// tests/np_kinematics.py restates it in fp64): world twist of every body, centre of mass / momentum / energy of the robot, and the eight
// sole corners with their height over the target stone and the stone that carries them.
//
// Every function is SSD (host and device): tests/host/kinematics_host.cpp runs the same code on the CPU.  The kernel (ss_kinematics.hip)
// only READS the environment state.  Lane layout there: the 22 bodies of an env are lanes 0..21 of one 32-lane half of a wavefront, lanes
// 22 / 23 run the step kernels' contact detection for the right / left foot, and the sums over the bodies are taken in the fixed order of
// half_sum below -- so a row's bits depend on nothing but the env's state.
#pragma once
#include "ss_render.hpp"

namespace ss {
namespace kin {

constexpr int kBodies = render::kBodies;
constexpr int kHalfLanes = 32;                  // lanes per env
constexpr int kDetectLane = kBodies;            // lanes 22, 23: detection of the right, left foot
static_assert(kDetectLane + 2 <= kHalfLanes, "bodies and the two detection lanes fit one half");
constexpr int kCornerNone = 0xff;               // foot_carriers: byte of a corner that no stone carries

struct BodyKin {       // body b in the world frame: pose of its link frame as body_pose writes it (position | R row-major), twist (v:
  float T[12], w[3], v[3];   // velocity of the frame's origin)
  SSD const float* p() const { return T; }
  SSD const float* R() const { return T + 3; }
};

template <class Model>
constexpr float total_mass() {
  double s = 0.0;
  for (int b = 0; b < kBodies; ++b) s += (double)Model::mass[b];
  return (float)s;
}

// Pose and twist of body b of env e.  The base twist of the state is in body coordinates (PHYSICS.md 3); along the chain
// v_child = v_parent + w_parent x (R_parent r_j),  w_child = w_parent + (R_parent e_axis) qd_j  (the axis is fixed under its own rotation).
template <class Model>
SSD void body_kin(const Params& P, int e, int b, BodyKin& o) {
  const float* F = P.fstate + e;
  const size_t np = (size_t)P.npad;
  float quat[4], wb[3], vb[3], R0[3][3];
  for (int i = 0; i < 4; ++i) quat[i] = F[(F_QUAT + i) * np];
  for (int i = 0; i < 3; ++i) { wb[i] = F[(F_VEL + i) * np]; vb[i] = F[(F_VEL + 3 + i) * np]; }
  quat_rot(quat, R0);
  float w[3], v[3];
  for (int i = 0; i < 3; ++i) {
    w[i] = R0[i][0] * wb[0] + R0[i][1] * wb[1] + R0[i][2] * wb[2];
    v[i] = R0[i][0] * vb[0] + R0[i][1] * vb[1] + R0[i][2] * vb[2];
  }
  render::walk_chain<Model>(P, e, b, o.T, [&](int j, const float (&R)[3][3]) {
    const float rj[3] = {Model::r[j][0], Model::r[j][1], Model::r[j][2]};
    float d[3], wxd[3];
    for (int i = 0; i < 3; ++i) d[i] = R[i][0] * rj[0] + R[i][1] * rj[1] + R[i][2] * rj[2];
    cross(w, d, wxd);
    const float qd = F[(F_QD + j) * np];
    const int ax = kAxis[j];
    for (int i = 0; i < 3; ++i) {
      v[i] += wxd[i];
      w[i] += R[i][ax] * qd;
    }
  });
  for (int i = 0; i < 3; ++i) { o.w[i] = w[i]; o.v[i] = v[i]; }
}

// o = R x (body -> world), o = R^T x (world -> body); R row-major
SSD void to_world(const float* R, const float x[3], float o[3]) {
  for (int i = 0; i < 3; ++i) o[i] = R[3 * i] * x[0] + R[3 * i + 1] * x[1] + R[3 * i + 2] * x[2];
}
SSD void to_body(const float* R, const float x[3], float o[3]) {
  for (int i = 0; i < 3; ++i) o[i] = R[i] * x[0] + R[3 + i] * x[1] + R[6 + i] * x[2];
}

// What body b adds to the first sums: m c (c: world position of its centre of mass) and m v_c
template <class Model>
SSD void body_moments(int b, const BodyKin& k, float mc[3], float mv[3]) {
  const float m = Model::mass[b];
  const float cl[3] = {Model::com[b][0], Model::com[b][1], Model::com[b][2]};
  float d[3], wxd[3];
  to_world(k.R(), cl, d);
  cross(k.w, d, wxd);
  for (int i = 0; i < 3; ++i) {
    mc[i] = m * (k.p()[i] + d[i]);
    mv[i] = m * (k.v[i] + wxd[i]);
  }
}

// ... and to the second ones, once the centre of mass `com` is known: angular momentum about it, L = (c - com) x m v_c + R I_c w_l, and
// kinetic energy T = (m |v_c|^2 + w_l . I_c w_l) / 2, with w_l = R^T w and the tables' inertia about the link origin:
// I_c w_l = I_O w_l - m c_l x (w_l x c_l),  w_l . I_c w_l = w_l . I_O w_l - m |w_l x c_l|^2.  Rotor armature is not part of either.
template <class Model>
SSD void body_momentum(int b, const BodyKin& k, const float com[3], float L[3], float& T) {
  const float m = Model::mass[b];
  const float cl[3] = {Model::com[b][0], Model::com[b][1], Model::com[b][2]};
  const float ixx = Model::inertia[b][0], iyy = Model::inertia[b][1], izz = Model::inertia[b][2];
  const float ixy = Model::inertia[b][3], ixz = Model::inertia[b][4], iyz = Model::inertia[b][5];
  float d[3], wxd[3], vc[3], rc[3], orb[3];
  to_world(k.R(), cl, d);
  cross(k.w, d, wxd);
  for (int i = 0; i < 3; ++i) {
    vc[i] = k.v[i] + wxd[i];
    rc[i] = (k.p()[i] + d[i]) - com[i];
  }
  const float mvc[3] = {m * vc[0], m * vc[1], m * vc[2]};
  cross(rc, mvc, orb);
  float wl[3], wxc[3], cxwxc[3], spin[3], spinw[3];
  to_body(k.R(), k.w, wl);
  cross(wl, cl, wxc);
  cross(cl, wxc, cxwxc);
  spin[0] = ixx * wl[0] + ixy * wl[1] + ixz * wl[2] - m * cxwxc[0];
  spin[1] = ixy * wl[0] + iyy * wl[1] + iyz * wl[2] - m * cxwxc[1];
  spin[2] = ixz * wl[0] + iyz * wl[1] + izz * wl[2] - m * cxwxc[2];
  to_world(k.R(), spin, spinw);
  for (int i = 0; i < 3; ++i) L[i] = orb[i] + spinw[i];
  T = 0.5f * (m * dot3(vc, vc) + dot3(wl, spin));
}

// The fixed order of the sums over an env's 32 lanes: x[i] += x[i ^ 16], then ^ 8, 4, 2, 1 (every lane ends with the same bits: the
// partners add the same two numbers).  The kernel takes these steps with lane exchanges; lanes without a body hold 0.
SSD float half_sum(float x[kHalfLanes]) {
  for (int off = kHalfLanes / 2; off > 0; off >>= 1)
    for (int i = 0; i < kHalfLanes; ++i)
      if ((i & off) == 0) { const float s = x[i] + x[i ^ off]; x[i] = s; x[i ^ off] = s; }
  return x[0];
}

// summary row (include/steppingstone.h) from the finished sums
template <class Model>
SSD void summary_row(const float mc[3], const float mv[3], const float L[3], float T, float out[12]) {
  constexpr float M = total_mass<Model>();
  for (int i = 0; i < 3; ++i) { out[i] = mc[i] / M; out[3 + i] = mv[i] / M; out[6 + i] = L[i]; }
  out[9] = T;
  out[10] = M * kGrav * out[2];
  out[11] = M;
}
template <class Model>
SSD void com_of(const float mc[3], float com[3]) {
  constexpr float M = total_mass<Model>();
  for (int i = 0; i < 3; ++i) com[i] = mc[i] / M;
}

// Sole corner c (0..3, Model::corners order; the left foot's list is its y-mirror) of foot `foot` (0 right, 1 left) whose body has the
// kinematics k: out = position (3) | velocity (3) | h = (x - s_n) . n_n over the surface plane of the target stone n (slot 1 of the
// env's active stones; negative below the surface)
template <class Model>
SSD void corner_row(const Params& P, int e, int foot, int c, const BodyKin& k, float out[7]) {
  const float* F = P.fstate + e;
  const size_t np = (size_t)P.npad;
  const float cl[3] = {Model::corners[c][0], foot ? -Model::corners[c][1] : Model::corners[c][1], Model::corners[c][2]};
  float d[3], wxd[3], s[3], n[3];
  to_world(k.R(), cl, d);
  cross(k.w, d, wxd);
  for (int i = 0; i < 3; ++i) {
    out[i] = k.p()[i] + d[i];
    out[3 + i] = k.v[i] + wxd[i];
    s[i] = F[(F_STONE + 8 + i) * np];
    n[i] = F[(F_STONE + 8 + 3 + i) * np];
  }
  const float x[3] = {out[0] - s[0], out[1] - s[1], out[2] - s[2]};
  out[6] = dot3(x, n);
}

// Which stone carries each corner of foot `foot`: the step kernels' own detection (fk_detect, PHYSICS.md 3.3), fed the way step_env and
// substep feed it -- the foot's half of the state in ITS world (the left foot's is the y-mirror) in the lane-private LDS view L, cos / sin
// of the spine and leg joints from ss_sincos.  Returns one byte per corner: the stone slot 0 / 1 / 2 (n-1 / n / n+1) or kCornerNone.
template <class Model>
SSD uint32_t foot_carriers(const Params& P, int e, int foot, const Lds& L) {
  const float* F = P.fstate + e;
  const size_t np = (size_t)P.npad;
  const float m = foot ? -1.f : 1.f;
  float pos[3], quat[4], zero[3] = {0.f, 0.f, 0.f};
  for (int i = 0; i < 3; ++i) pos[i] = F[(F_POS + i) * np];
  for (int i = 0; i < 4; ++i) quat[i] = F[(F_QUAT + i) * np];
  put_base(L, m, pos, quat, zero, zero);
  for (int sl = 0; sl < 3; ++sl) {
    for (int i = 0; i < 3; ++i) {
      const float mi = i == 1 ? m : 1.f;
      L.s(S_STP + sl * 3 + i) = mi * F[(F_STONE + sl * 8 + i) * np];
      L.s(S_STN + sl * 3 + i) = mi * F[(F_STONE + sl * 8 + 3 + i) * np];
    }
    L.q2(kLdsHead + sl) = make_float2(F[(F_HEAD + sl * 2) * np], m * F[(F_HEAD + sl * 2 + 1) * np]);
  }
  float cs8[8], sn8[8];
  static_for<0, 8>([&](auto Jc) {
    constexpr int jr = decltype(Jc)::value, jl = left_twin(jr);
    ss_sincos(mirror_sign(jr, m) * F[(F_Q + (foot ? jl : jr)) * np], sn8[jr], cs8[jr]);
  });
  const float ql[4] = {L.s(S_QUAT), L.s(S_QUAT + 1), L.s(S_QUAT + 2), L.s(S_QUAT + 3)};
  float Rb[3][3];
  quat_rot(ql, Rb);
  DetectOut det;
  FootReport fr;
  fk_detect<Model>(cs8, sn8, Rb, L, det, fr);
  uint32_t code = 0;
  for (int k = 0; k < 4; ++k)
    code |= (uint32_t)(((det.active >> k) & 1) ? ((det.cslot >> (2 * k)) & 3) : kCornerNone) << (8 * k);
  return code;
}
SSD float carrier_value(uint32_t code, int c) {
  const int v = (int)((code >> (8 * c)) & 0xffu);
  return v == kCornerNone ? -1.f : (float)v;
}

}  // namespace kin
}  // namespace ss
