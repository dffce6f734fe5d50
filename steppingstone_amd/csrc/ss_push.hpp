// ss_push.hpp -- an impulse on a body (docs/PHYSICS.md 12 "Impulse" is the specification; tests/np_push.py restates it in fp64): the
// change of the generalised velocity  delta_nu = M(q)^-1 J_{b,x}^T w  for a world wrench impulse w = (p, L) at the body-fixed point x of
// body b, M exactly the matrix of the equation-of-motion readout (ss_eom.hpp, rotor armature included).
//
// Every function is SSD (host and device): tests/host/push_host.cpp runs the same code on the CPU.  The kernel (ss_push.hip) keeps, per
// requested row, the 22 body records of ss_eom.hpp, the LOWER TRIANGLE of M (kTri words, never written to HBM), the right-hand side and
// the pushed point in LDS.  Two lane layouts: body lane b assembles row 5 + b of M from ss_eom.hpp's own functions (lane 0: the base
// block), so M is the readout's matrix word for word; DoF lane i < 27 owns word i of the right-hand side and row i in the solve.
//
// The solve is the sparse factorisation M = L^T D L of Featherstone (RBDA 6.5), taken from the last DoF to the first: with every subtree
// an index range (eom::subtree_ranges_match_parents) that order has no fill-in, so L keeps M's pattern -- the six base columns dense, a
// joint row coupled to the joints of its own chain only -- and the structural zeros are skipped, never computed.  Every word has one
// fixed summation order (the steps k = 26 .. 1 of eliminate, then the columns j = 0 .. 25 of substitute) on the host and in the kernel.
#pragma once
#include "ss_eom.hpp"

namespace ss {
namespace push {

constexpr int kBodies = eom::kBodies;
constexpr int kHalfLanes = eom::kHalfLanes;
constexpr int kDof = eom::kDof;
constexpr int kComposite = 10;                            // of eom::kParts: m | h | I_O, what the base block is made of
constexpr int kTri = kDof * (kDof + 1) / 2;               // 378: the lower triangle of M
static_assert(kDof <= kHalfLanes, "one DoF lane per generalised coordinate");

SSD constexpr int tri(int a, int c) { return a * (a + 1) / 2 + c; }   // M[a][c], c <= a
// M[k][i], i < k, is not a structural zero: i is a base DoF, or joint i - 6 carries the body of joint k - 6
SSD bool coupled(int k, int i) { return i < 6 || eom::carries(i - 5, k - 5); }

// the row's LDS block in the kernel, one plain array on the host
constexpr int kRecs = 0, kMass = kBodies * eom::kBodyRecWords, kRhs = kMass + kTri, kPoint = kRhs + kDof, kRowWords = kPoint + 6;
static_assert((kRowWords & 1) == 1, "odd: the rows' blocks start on different LDS banks");

// lane 0: the base block from the composite C of all bodies about the torso origin (C[kComposite:] is not read by what is kept)
SSD void base_rows(const eom::BodyEom& k0, const float C[eom::kParts], float* Ml) {
  float blk[6][6], bias[6], grav[6];
  eom::base_block(k0, C, blk, bias, grav);
  for (int a = 0; a < 6; ++a)
    for (int c = 0; c <= a; ++c) Ml[tri(a, c)] = blk[a][c];
}

// body lane b >= 1: row 5 + b of M, columns 0 .. 5 + b, the expressions of eom::lane_finish and of the eom kernel's stores
template <class Model>
SSD void joint_row(int b, const eom::BodyEom& k, const float* recs, float* Ml) {
  eom::LaneEom L;
  float Cj[10], pxf[3];
  const float still[3] = {0.f, 0.f, 0.f};
  eom::joint_composite(b, recs, Cj);
  eom::composite_on(Cj, k.ax, still, L.Fn, L.Ff);
  cross(k.p, L.Ff, pxf);
  for (int i = 0; i < 3; ++i) L.Fo[i] = L.Fn[i] + pxf[i];
  const int row = 5 + b;
  const float* rec = recs + b * eom::kBodyRecWords;
  for (int c = 0; c < 6; ++c) Ml[tri(row, c)] = eom::on_base(k.R0, c, L.Fo, L.Ff);
  const int depth = eom::depth_of(b);
#pragma unroll 1
  for (int l = 0; l < depth; ++l) Ml[tri(row, 5 + eom::level_body(b, l))] = eom::mass_at_level<Model>(b, l, rec, L);
#pragma unroll 1
  for (int a = 1; a < b; ++a)
    if (!eom::carries(a, b)) Ml[tri(row, 5 + a)] = 0.f;
}

// the lane of the pushed body bt: the point relative to its link origin (world axes; its centre of mass when point is null -- the link
// origin for a massless link, whose table entry is 0) and relative to the torso origin
SSD void pushed_point(const eom::BodyEom& k, const float* rec, const float* point, float* pt) {
  float xw[3];
  if (point) {
    const float xl[3] = {point[0], point[1], point[2]};
    kin::to_world(k.R, xl, xw);
  } else {
    for (int i = 0; i < 3; ++i) xw[i] = rec[eom::kRecCom + i];
  }
  for (int i = 0; i < 3; ++i) { pt[i] = xw[i]; pt[3 + i] = k.p[i] + xw[i]; }
}

// word i of J^T w.  Base DoF i < 6 (R0: the torso orientation): R0^T of the wrench about the torso origin, (L + xo x p, p).  Joint DoF
// i = 5 + a: s_a . (L + (x - o_a) x p) when body a carries the pushed body bt, x - o_a the offset of bt's record at a's level plus the
// point (sums of link vectors, no difference of positions); 0 otherwise.  w = p | L.
SSD float rhs_word(int i, int bt, const float* R0, const float* rec_t, const float* pt, const float w[6]) {
  const float p[3] = {w[0], w[1], w[2]};
  float xp[3], n[3];
  if (i < 6) {
    const float xo[3] = {pt[3], pt[4], pt[5]};
    cross(xo, p, xp);
    for (int c = 0; c < 3; ++c) n[c] = w[3 + c] + xp[c];
    return eom::on_base(R0, i, n, p);
  }
  const int a = i - 5;
  if (!eom::carries(a, bt)) return 0.f;
  const int l = eom::depth_of(a) - 1;
  const float* off = rec_t + eom::kRecOff + 3 * l;
  const float* ax = rec_t + eom::kRecAxis + 3 * l;
  const float xj[3] = {off[0] + pt[0], off[1] + pt[1], off[2] + pt[2]};
  cross(xj, p, xp);
  for (int c = 0; c < 3; ++c) n[c] = w[3 + c] + xp[c];
  return ax[0] * n[0] + ax[1] * n[1] + ax[2] * n[2];
}

// Step k (26 .. 1) of the factorisation for DoF lane i < k with coupled(k, i): l = M[k][i] / M[k][k]; row i (its columns j <= i that row k
// holds) loses l times row k, the right-hand side word i loses l times word k -- the back substitution L^T y = r rides along.  Returns l,
// which the caller stores in M[k][i] once EVERY lane has read row k (the kernel: after a barrier).  It writes row i and r[i] alone.
SSD float eliminate(float* Ml, float* r, int k, int i) {
  const float l = Ml[tri(k, i)] / Ml[tri(k, k)];
  for (int j = 0; j <= i; ++j)
    if (coupled(k, j)) Ml[tri(i, j)] = Ml[tri(i, j)] - l * Ml[tri(k, j)];
  r[i] = r[i] - l * r[k];
  return l;
}
// z = D^-1 y, DoF lane i
SSD void scale(const float* Ml, float* r, int i) { r[i] = r[i] / Ml[tri(i, i)]; }
// column j (0 .. 25) of the forward substitution L x = z for DoF lane i > j with coupled(i, j)
SSD void substitute(const float* Ml, float* r, int j, int i) { r[i] = r[i] - Ml[tri(i, j)] * r[j]; }

}  // namespace push
}  // namespace ss
