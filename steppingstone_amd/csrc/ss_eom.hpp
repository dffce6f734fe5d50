// ss_eom.hpp -- the terms of the equation of motion read from the packed state (docs/PHYSICS.md 11 "Equation of motion readout" is the
// specification; tests/np_eom.py restates it in fp64): joint-space inertia M(q) with the rotor armature, velocity-product force c(q, nu),
// generalised force of gravity g(q), passive joint torques, and the Jacobians of the eight sole corners.
//
// Every function is SSD (host and device): tests/host/eom_host.cpp runs the same code on the CPU.  The kernel (ss_eom.hip) only READS the
// environment state.  Lane layout there: the 22 bodies of an env are lanes 0..21 of one 32-lane half of a wavefront; lane b walks the
// ancestor chain of body b, the sums over a body's subtree are taken in the fixed order of subtree_sum and joint_composite below, and
// lane b = j + 1 owns DoF 6 + j (lane 0: the six base DoFs).
//
// Every spatial quantity is taken in WORLD AXES about a point of the robot, never about the world origin: the torso's world position
// enters nowhere, so the readout is translation invariant.  The velocity-product and gravity wrenches and the base block are taken about
// the TORSO ORIGIN O: a motion screw is (omega, v_O: velocity of the body-fixed point at O), a wrench is (n_O: moment about O, f), their
// product omega . n_O + v_O . f.  The joint rows of the mass matrix are taken about the JOINT's own origin, with every offset a sum of link
// vectors down the chain: about O, a foot's m |p|^2 ~ 2 kg m^2 would leave an ankle's 0.02 kg m^2 two digits short.
#pragma once
#include "ss_kinematics.hpp"

namespace ss {
namespace eom {

constexpr int kBodies = kin::kBodies;
constexpr int kHalfLanes = kin::kHalfLanes;     // lanes per env
constexpr int kDof = SS_EOM_DOF;
constexpr int kParts = 16;                      // per-body terms summed over subtrees: m | h (3) | I_O (xx yy zz xy xz yz) | n_O (3) | f (3)
static_assert(kDof == 6 + NJ, "6 base DoFs and the joints");

// The bodies of the subtree of body b are the index range [b, subtree_end(b)] (spine 1..3 carries both legs 4..8 and 9..13; the arms
// 14..17 and 18..21 hang on the torso): checked against kParent below.
SSD constexpr int subtree_end(int b) { return b == 0 ? 21 : (b <= 3 ? 13 : (b <= 8 ? 8 : (b <= 13 ? 13 : (b <= 17 ? 17 : 21)))); }
constexpr bool subtree_ranges_match_parents() {
  for (int b = 0; b < kBodies; ++b)
    for (int c = 0; c < kBodies; ++c) {
      bool anc = false;
      for (int a = c;; a = kParent[a - 1]) {
        if (a == b) { anc = true; break; }
        if (a == 0) break;
      }
      if (anc != (c >= b && c <= subtree_end(b))) return false;
    }
  return true;
}
static_assert(subtree_ranges_match_parents(), "subtree_end describes the tree of kParent");
// body `a` is body b or one of its ancestors
SSD bool carries(int a, int b) { return b >= a && b <= subtree_end(a); }

// What lane b leaves for the other lanes of its env, one record per body (LDS in the kernel): per level l of its chain (root first; joint
// level_body(b, l) - 1 moves body level_body(b, l)) the joint's world axis and the vector from the joint's origin to the body's own origin -- a
// sum of link vectors, no difference of positions --, then its centre of mass relative to its origin, its mass and its inertia about
// the centre of mass (xx yy zz xy xz yz), all in world axes.
constexpr int kMaxChain = render::kMaxChain;
constexpr int kRecAxis = 0, kRecOff = 3 * kMaxChain, kRecCom = 6 * kMaxChain, kRecMass = kRecCom + 3, kRecInertia = kRecMass + 1;
constexpr int kBodyRecWords = kRecInertia + 6 + 1;      // 59: odd, so that the bodies' records start on different LDS banks
struct Levels {
  int body[kBodies][kMaxChain] = {};
  int depth[kBodies] = {};
};
constexpr Levels make_levels() {
  Levels t;
  for (int b = 0; b < kBodies; ++b) {
    int d = 0;
    for (int c = b; c != 0; c = kParent[c - 1]) ++d;
    t.depth[b] = d;
    int l = d;
    for (int c = b; c != 0; c = kParent[c - 1]) t.body[b][--l] = c;
  }
  return t;
}
constexpr Levels kLevels = make_levels();
static_assert(kLevels.depth[RFOOT] == kMaxChain && kLevels.depth[LFOOT] == kMaxChain, "the longest chains fill kMaxChain levels");
SSD int depth_of(int b) {
  constexpr Levels t = make_levels();
  return t.depth[b];
}
SSD int level_body(int b, int l) {
  constexpr Levels t = make_levels();
  return t.body[b][l];
}

struct BodyEom {       // body b about the torso origin, world axes
  float R0[9];         // torso orientation (row-major): column k is base axis k in the world
  float R[9], p[3];    // orientation, origin of the link frame relative to the torso origin
  float w[3], al[3];   // angular velocity; angular acceleration at nu-dot = 0
  float a[3];          // acceleration of the link origin at nu-dot = 0 (the torso's: w x v, its twist components being held)
  float ax[3], vo[3];  // b >= 1: screw of its joint b - 1 at unit rate: the axis, and p x axis
};

// Pose, rate and velocity-product acceleration of body b of env e along its ancestor chain (PHYSICS.md 11).  Across joint j, with d = R_par
// r_j and the axis s = R_par e_axis:  a_child = a + al x d + w x (w x d),  al_child = al + (w x s) qd_j,  w_child = w + s qd_j.
// It also fills the per-level part of the body's record `rec`.
template <class Model>
SSD void body_eom(const Params& P, int e, int b, BodyEom& o, float* rec) {
  const float* F = P.fstate + e;
  const size_t np = (size_t)P.npad;
  float quat[4], wb[3], vb[3], R[3][3];
  for (int i = 0; i < 4; ++i) quat[i] = F[(F_QUAT + i) * np];
  for (int i = 0; i < 3; ++i) { wb[i] = F[(F_VEL + i) * np]; vb[i] = F[(F_VEL + 3 + i) * np]; }
  quat_rot(quat, R);
  float p[3] = {0.f, 0.f, 0.f}, w[3], v[3], al[3] = {0.f, 0.f, 0.f}, a[3], ax[3] = {0.f, 0.f, 0.f};
  for (int i = 0; i < 3; ++i) {
    w[i] = R[i][0] * wb[0] + R[i][1] * wb[1] + R[i][2] * wb[2];
    v[i] = R[i][0] * vb[0] + R[i][1] * vb[1] + R[i][2] * vb[2];
    for (int k = 0; k < 3; ++k) o.R0[3 * i + k] = R[i][k];
  }
  cross(w, v, a);
  const int depth = depth_of(b);
#pragma unroll 1
  for (int l = 0; l < depth; ++l) {
    const int j = level_body(b, l) - 1;
    const float rj[3] = {Model::r[j][0], Model::r[j][1], Model::r[j][2]};
    const float qd = F[(F_QD + j) * np];
    const int axi = kAxis[j], i1 = axi == 0 ? 1 : (axi == 1 ? 2 : 0), i2 = axi == 0 ? 2 : (axi == 1 ? 0 : 1);
    float d[3], wxd[3], wxwxd[3], alxd[3], wxs[3];
    for (int i = 0; i < 3; ++i) {
      d[i] = R[i][0] * rj[0] + R[i][1] * rj[1] + R[i][2] * rj[2];
      ax[i] = R[i][axi];
    }
    cross(w, d, wxd);
    cross(w, wxd, wxwxd);
    cross(al, d, alxd);
    cross(w, ax, wxs);
    for (int i = 0; i < 3; ++i) {
      rec[kRecAxis + 3 * l + i] = ax[i];
      rec[kRecOff + 3 * l + i] = d[i];
      p[i] += d[i];
      a[i] = a[i] + alxd[i] + wxwxd[i];
      al[i] += wxs[i] * qd;
      w[i] += ax[i] * qd;
    }
    float s, c;
    sincosf(F[(F_Q + j) * np], &s, &c);
    for (int i = 0; i < 3; ++i) {          // R <- R Rot(axis, q): columns i1, i2 turn
      const float c1 = R[i][i1], c2 = R[i][i2];
      R[i][i1] = c * c1 + s * c2;
      R[i][i2] = c * c2 - s * c1;
    }
  }
  for (int i = 0; i < 3; ++i) {
    o.p[i] = p[i]; o.w[i] = w[i]; o.al[i] = al[i]; o.a[i] = a[i]; o.ax[i] = ax[i];
    for (int k = 0; k < 3; ++k) o.R[3 * i + k] = R[i][k];
  }
  cross(p, ax, o.vo);
  float off[3] = {0.f, 0.f, 0.f};          // the link vectors become offsets: level l holds the sum of the link vectors below it
#pragma unroll 1
  for (int l = depth - 1; l >= 0; --l)
    for (int i = 0; i < 3; ++i) {
      const float d = rec[kRecOff + 3 * l + i];
      rec[kRecOff + 3 * l + i] = off[i];
      off[i] += d;
    }
}

// the rest of body b's record: centre of mass relative to the link origin, mass, inertia about the centre of mass R (I - m (|c_l|^2 1 -
// c_l c_l^T)) R^T from the tables' inertia I about the link origin
template <class Model>
SSD void body_record(int b, const BodyEom& k, float* rec) {
  const float m = Model::mass[b];
  const float cl[3] = {Model::com[b][0], Model::com[b][1], Model::com[b][2]};
  const float cc = dot3(cl, cl);
  float Ic[3][3], T[3][3], c[3];
  constexpr int ia[6] = {0, 1, 2, 0, 0, 1}, ib[6] = {0, 1, 2, 1, 2, 2};
  for (int n = 0; n < 6; ++n) {
    const int i = ia[n], j = ib[n];
    const float v = Model::inertia[b][n] - m * ((i == j ? cc : 0.f) - cl[i] * cl[j]);
    Ic[i][j] = v;
    Ic[j][i] = v;
  }
  const float* R = k.R;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) T[i][j] = R[3 * i] * Ic[0][j] + R[3 * i + 1] * Ic[1][j] + R[3 * i + 2] * Ic[2][j];
  kin::to_world(R, cl, c);
  for (int i = 0; i < 3; ++i) rec[kRecCom + i] = c[i];
  rec[kRecMass] = m;
  for (int n = 0; n < 6; ++n) {
    const int i = ia[n], j = ib[n];
    rec[kRecInertia + n] = T[i][0] * R[3 * j] + T[i][1] * R[3 * j + 1] + T[i][2] * R[3 * j + 2];
  }
}

// Inertia of the subtree of body b >= 1 about the origin of its joint: m | h = sum m_t d_t | I = sum I_c,t + m_t (|d_t|^2 1 - d_t d_t^T),
// d_t the vector from that origin to body t's centre of mass, taken from t's record at b's level.  recs: the env's records, body t at
// recs + t * kBodyRecWords; the sum runs from body subtree_end(b) down to b.
SSD void joint_composite(int b, const float* recs, float C[10]) {
  for (int i = 0; i < 10; ++i) C[i] = 0.f;
  const int l = depth_of(b) - 1, end = subtree_end(b);
  for (int t = end; t >= b; --t) {
    const float* r = recs + t * kBodyRecWords;
    const float m = r[kRecMass];
    const float d[3] = {r[kRecOff + 3 * l] + r[kRecCom], r[kRecOff + 3 * l + 1] + r[kRecCom + 1], r[kRecOff + 3 * l + 2] + r[kRecCom + 2]};
    const float dd = dot3(d, d);
    C[0] = C[0] + m;
    for (int i = 0; i < 3; ++i) C[1 + i] = C[1 + i] + m * d[i];
    C[4] = C[4] + (r[kRecInertia] + m * (dd - d[0] * d[0]));
    C[5] = C[5] + (r[kRecInertia + 1] + m * (dd - d[1] * d[1]));
    C[6] = C[6] + (r[kRecInertia + 2] + m * (dd - d[2] * d[2]));
    C[7] = C[7] + (r[kRecInertia + 3] - m * (d[0] * d[1]));
    C[8] = C[8] + (r[kRecInertia + 4] - m * (d[0] * d[2]));
    C[9] = C[9] + (r[kRecInertia + 5] - m * (d[1] * d[2]));
  }
}

// What body b adds to the sums over the subtrees that hold it (x[kParts]):
//   its inertia about O:  m,  h = m c_O  (c_O = p + c, c = R c_l),  I_O = R I R^T + m [(p.p + 2 p.c) 1 - p p^T - p c^T - c p^T]  with the
//   tables' inertia I about the link origin (the shift from the link origin to O, written without the difference of two squares);
//   the wrench that moves it at nu-dot = 0 (Newton-Euler about the link origin, in link axes, then turned and shifted to O):
//   n_l = I al_l + w_l x I w_l + m c_l x a_l,  f_l = m (a_l + al_l x c_l + w_l x (w_l x c_l)),  n_O = R n_l + p x R f_l.
template <class Model>
SSD void body_parts(int b, const BodyEom& k, float x[kParts]) {
  const float m = Model::mass[b];
  const float cl[3] = {Model::com[b][0], Model::com[b][1], Model::com[b][2]};
  const float ixx = Model::inertia[b][0], iyy = Model::inertia[b][1], izz = Model::inertia[b][2];
  const float ixy = Model::inertia[b][3], ixz = Model::inertia[b][4], iyz = Model::inertia[b][5];
  const float* R = k.R;
  const float* p = k.p;
  float c[3];
  kin::to_world(R, cl, c);
  x[0] = m;
  for (int i = 0; i < 3; ++i) x[1 + i] = m * (p[i] + c[i]);
  float T[3][3];                             // R I
  for (int i = 0; i < 3; ++i) {
    T[i][0] = R[3 * i] * ixx + R[3 * i + 1] * ixy + R[3 * i + 2] * ixz;
    T[i][1] = R[3 * i] * ixy + R[3 * i + 1] * iyy + R[3 * i + 2] * iyz;
    T[i][2] = R[3 * i] * ixz + R[3 * i + 1] * iyz + R[3 * i + 2] * izz;
  }
  const float s = dot3(p, p) + 2.f * dot3(p, c);
  constexpr int ia[6] = {0, 1, 2, 0, 0, 1}, ib[6] = {0, 1, 2, 1, 2, 2};
  for (int n = 0; n < 6; ++n) {
    const int i = ia[n], j = ib[n];
    const float rot = T[i][0] * R[3 * j] + T[i][1] * R[3 * j + 1] + T[i][2] * R[3 * j + 2];
    const float shift = (i == j ? s : 0.f) - p[i] * p[j] - p[i] * c[j] - c[i] * p[j];
    x[4 + n] = rot + m * shift;
  }
  float wl[3], all[3], aol[3], Iw[3], Ial[3], wxIw[3], cxa[3], alxc[3], wxc[3], wxwxc[3], nl[3], fl[3], n[3], f[3], pxf[3];
  kin::to_body(R, k.w, wl);
  kin::to_body(R, k.al, all);
  kin::to_body(R, k.a, aol);
  Iw[0] = ixx * wl[0] + ixy * wl[1] + ixz * wl[2];
  Iw[1] = ixy * wl[0] + iyy * wl[1] + iyz * wl[2];
  Iw[2] = ixz * wl[0] + iyz * wl[1] + izz * wl[2];
  Ial[0] = ixx * all[0] + ixy * all[1] + ixz * all[2];
  Ial[1] = ixy * all[0] + iyy * all[1] + iyz * all[2];
  Ial[2] = ixz * all[0] + iyz * all[1] + izz * all[2];
  cross(wl, Iw, wxIw);
  cross(cl, aol, cxa);
  cross(all, cl, alxc);
  cross(wl, cl, wxc);
  cross(wl, wxc, wxwxc);
  for (int i = 0; i < 3; ++i) {
    nl[i] = Ial[i] + wxIw[i] + m * cxa[i];
    fl[i] = m * (aol[i] + alxc[i] + wxwxc[i]);
  }
  kin::to_world(R, nl, n);
  kin::to_world(R, fl, f);
  cross(p, f, pxf);
  for (int i = 0; i < 3; ++i) { x[10 + i] = n[i] + pxf[i]; x[13 + i] = f[i]; }
}

// The fixed order of the sum over the subtree of body b: from body subtree_end(b) down to b.  x holds one term per lane; the kernel reads
// the lanes one after the other with lane exchanges and adds in this order.
SSD float subtree_sum(const float x[kHalfLanes], int b) {
  float s = 0.f;
  const int end = subtree_end(b);
  for (int t = kBodies - 1; t >= 0; --t)
    if (t >= b && t <= end) s = s + x[t];
  return s;
}

// omega . n_O + v_O . f: what the wrench (n, f) does on the screw (w, vo)
SSD float on_screw(const float w[3], const float vo[3], const float n[3], const float f[3]) {
  return w[0] * n[0] + w[1] * n[1] + w[2] * n[2] + vo[0] * f[0] + vo[1] * f[1] + vo[2] * f[2];
}
// momentum (n_O, f) of the composite body C (m | h | I_O of a subtree) moving on the screw (w, vo): f = m v_O + w x h, n_O = I_O w + h x v_O
SSD void composite_on(const float* C, const float w[3], const float vo[3], float n[3], float f[3]) {
  const float* h = C + 1;
  const float* I = C + 4;
  float wxh[3], hxv[3];
  cross(w, h, wxh);
  cross(h, vo, hxv);
  n[0] = I[0] * w[0] + I[3] * w[1] + I[4] * w[2] + hxv[0];
  n[1] = I[3] * w[0] + I[1] * w[1] + I[5] * w[2] + hxv[1];
  n[2] = I[4] * w[0] + I[5] * w[1] + I[2] * w[2] + hxv[2];
  for (int i = 0; i < 3; ++i) f[i] = C[0] * vo[i] + wxh[i];
}
// weight of the composite body as a wrench about O: f = m g, n_O = h x g, g = (0, 0, -kGrav)
SSD void composite_weight(const float C[kParts], float n[3], float f[3]) {
  const float g[3] = {0.f, 0.f, -kGrav};
  cross(C + 1, g, n);
  for (int i = 0; i < 3; ++i) f[i] = C[0] * g[i];
}

// base DoF k (0..2: turning about torso axis k; 3..5: moving along torso axis k - 3) as a screw about O
SSD void base_screw(const float R0[9], int k, float w[3], float vo[3]) {
  for (int i = 0; i < 3; ++i) {
    const float c = R0[3 * i + (k < 3 ? k : k - 3)];
    w[i] = k < 3 ? c : 0.f;
    vo[i] = k < 3 ? 0.f : c;
  }
}
// the wrench (n, f) on base DoF k: one column of R0 against n or against f (the screw's other half is 0 and adds nothing)
SSD float on_base(const float R0[9], int k, const float n[3], const float f[3]) {
  const float* x = k < 3 ? n : f;
  const int c = k < 3 ? k : k - 3;
  return R0[c] * x[0] + R0[3 + c] * x[1] + R0[6 + c] * x[2];
}

// passive torque of joint j (PHYSICS.md 11; 3.1's tau_j at h = 0 and tau_m = 0): -damping qd - stiffness q - kl viol - dl qd
template <class Model>
SSD float passive_torque(int j, float q, float qd) {
  const float lo = Model::lo[j], hi = Model::hi[j];
  const float viol = fminf(q - lo, 0.f) + fmaxf(q - hi, 0.f);
  const float kl = viol != 0.f ? Model::klim[j] : 0.f, dl = viol != 0.f ? Model::dlim[j] : 0.f;
  return -Model::damping[j] * qd - Model::stiffness[j] * q - kl * viol - dl * qd;
}

// What lane b holds once the sums are taken: the sums C about O over its subtree (bias, gravity; lane 0: the base block) and, for a joint
// lane, the momentum of its subtree turning about its own joint at unit rate -- moment Fn about the joint's origin, the same moment Fo
// shifted to O, force Ff -- and its three words of `forces`.  recs: the env's records.
struct LaneEom {
  float C[kParts], Fn[3], Fo[3], Ff[3];
  float bias, grav, passive;
};
template <class Model>
SSD void lane_finish(const Params& P, int e, int b, const BodyEom& k, const float* recs, LaneEom& L) {
  float Cj[10], gn[3], gf[3], pxf[3];
  const float still[3] = {0.f, 0.f, 0.f};
  joint_composite(b, recs, Cj);
  composite_on(Cj, k.ax, still, L.Fn, L.Ff);
  cross(k.p, L.Ff, pxf);
  for (int i = 0; i < 3; ++i) L.Fo[i] = L.Fn[i] + pxf[i];
  composite_weight(L.C, gn, gf);
  L.bias = on_screw(k.ax, k.vo, L.C + 10, L.C + 13);
  L.grav = on_screw(k.ax, k.vo, gn, gf);
  const int j = b - 1;
  const size_t np = (size_t)P.npad;
  L.passive = passive_torque<Model>(j, P.fstate[e + (F_Q + j) * np], P.fstate[e + (F_QD + j) * np]);
}

// mass[6 + j][6 + j'] for the joint lane b = j + 1 and the joint j' at level l of its chain (its own joint: the last level): the axis of
// j' against the moment of the lane's momentum about the origin of j', Fn + off_l x Ff; the diagonal adds the armature.  rec: b's record.
template <class Model>
SSD float mass_at_level(int b, int l, const float* rec, const LaneEom& L) {
  const float* ax = rec + kRecAxis + 3 * l;
  float oxf[3];
  cross(rec + kRecOff + 3 * l, L.Ff, oxf);
  const float v = ax[0] * (L.Fn[0] + oxf[0]) + ax[1] * (L.Fn[1] + oxf[1]) + ax[2] * (L.Fn[2] + oxf[2]);
  return l == depth_of(b) - 1 ? v + Model::armature[b - 1] : v;
}

// lane 0: the 6 x 6 base block, lower triangle [a][k], k <= a (the caller mirrors it), and the base words of bias and gravity
SSD void base_block(const BodyEom& k0, const float C[kParts], float blk[6][6], float bias[6], float grav[6]) {
  float gn[3], gf[3];
  composite_weight(C, gn, gf);
  for (int a = 0; a < 6; ++a) {
    float w[3], vo[3], n[3], f[3];
    base_screw(k0.R0, a, w, vo);
    composite_on(C, w, vo, n, f);
    for (int k = 0; k < 6; ++k) blk[a][k] = k <= a ? on_base(k0.R0, k, n, f) : 0.f;
    bias[a] = on_base(k0.R0, a, C + 10, C + 13);
    grav[a] = on_base(k0.R0, a, gn, gf);
  }
}

// Jacobian of sole corner c of foot `foot`, whose body has the kinematics k and the record rec.  x: the corner relative to the foot's
// link origin, world axes.  Base column `col`: R0 e_col x (p + x) or R0 e_(col - 3); the joint at level l: axis_l x (off_l + x).
template <class Model>
SSD void corner_offset(int foot, int c, const BodyEom& k, float x[3]) {
  const float cl[3] = {Model::corners[c][0], foot ? -Model::corners[c][1] : Model::corners[c][1], Model::corners[c][2]};
  kin::to_world(k.R, cl, x);
}
SSD void corner_jac_base(const BodyEom& k, const float x[3], int col, float o[3]) {
  float w[3], vo[3], wxx[3];
  const float xo[3] = {k.p[0] + x[0], k.p[1] + x[1], k.p[2] + x[2]};
  base_screw(k.R0, col, w, vo);
  cross(w, xo, wxx);
  for (int i = 0; i < 3; ++i) o[i] = col < 3 ? wxx[i] : vo[i];
}
SSD void corner_jac_level(const float* rec, int l, const float x[3], float o[3]) {
  const float* off = rec + kRecOff + 3 * l;
  const float xj[3] = {off[0] + x[0], off[1] + x[1], off[2] + x[2]};
  cross(rec + kRecAxis + 3 * l, xj, o);
}

}  // namespace eom
}  // namespace ss
