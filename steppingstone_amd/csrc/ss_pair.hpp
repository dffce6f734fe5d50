// ss_pair.hpp -- what the packed-f32 ("pair") chains need on top of the spatial algebra of ss_math.hpp.
//
// The leg joints 3..6 (hip x, z, y, knee) and the arm joints 13..16 (shoulder x, z, y, elbow) of a half body have the
// same axes and the same massless/massive link pattern (tools/gen_model_tables.py asserts it), so the three ABA sweeps
// apply the SAME operator sequence to both chains with different constants.  Here every quantity is a float pair
// {leg, arm} and every operation one v_pk_*_f32 instruction: half the VALU instructions for those eight joints.
// Constants become literal pairs; a term is dropped only when it is zero for BOTH chains.
//
// The types (SV2, Sym3P, ABIP) and the transforms (cross, rot, rotT, rot_sym, rot_gen, xmotion, xforce, xinertia) are the templates of
// ss_math.hpp at T = ssf2.  What is here: pack / unpack helpers, the pair's joint constants (PairJoint) and the three functions whose
// sums run in another order than their scalar namesakes (cross_rP, abi_add_bodyP, body_biasP).
#pragma once
#include "ss_math.hpp"

namespace ss {

SSD ssf2 pk(float a, float b) { return ssf2{a, b}; }          // constants
// run-time scalars: made opaque first, otherwise instcombine turns "insert (load float from an SV still in memory)"
// into overlapping <2 x float> loads, which keeps that SV in scratch (seen as 88 B/lane and +25 % wait cycles)
#if defined(__HIP_DEVICE_COMPILE__)
#define SS_REG(x) asm("" : "+v"(x))
#else
#define SS_REG(x) asm("" : "+x"(x))
#endif
SSD ssf2 pkv(float a, float b) { SS_REG(a); SS_REG(b); return ssf2{a, b}; }
// a * {s[H], s[H]} + c and a * {s[H], s[H]}: the factor is one half of a pair that is in registers already.  For the HIGH half the
// compiler copies it out first (v_mov_b32 tmp, s.hi, then op_sel_hi:[1,0,1] on tmp); the instruction can pick the high dword for
// both of its halves itself (op_sel:[0,1,0] op_sel_hi:[1,1,1]), which is what the inline assembly says.  The LOW half needs no help.
// Hazards of the statement: one VALU instruction, registers only.  The compiler treats its result like that of a packed instruction
// with the src0 op_sel_hi bit set (one wait state before a reader in the next instruction: it pads after the statement) and its
// operands like any packed instruction's (it pads in front where the producer is of that form); docs/HISTORY.md "Wait states".
// Values: two fused multiply-adds (two products) of the same operands either way -- tests/test_pair_broadcast.py holds both
// halves, on the device and in the host build, bitwise against fmaf / the plain product.
template <int H>
SSD ssf2 pk_fma_half(ssf2 a, ssf2 s, ssf2 c) {
  static_assert(H == 0 || H == 1, "low or high half");
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (H == 1) {
    ssf2 d;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(d) : "v"(a), "v"(s), "v"(c));
    return d;
  } else {
    return a * ssf2{s.x, s.x} + c;
  }
#else
  const float f = H ? s.y : s.x;
  return ssf2{__builtin_fmaf(a.x, f, c.x), __builtin_fmaf(a.y, f, c.y)};
#endif
}
template <int H>
SSD ssf2 pk_mul_half(ssf2 a, ssf2 s) {
  static_assert(H == 0 || H == 1, "low or high half");
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (H == 1) {
    ssf2 d;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(d) : "v"(a), "v"(s));
    return d;
  } else {
    return a * ssf2{s.x, s.x};
  }
#else
  const float f = H ? s.y : s.x;
  return ssf2{a.x * f, a.y * f};
#endif
}
SSD SV sv_half(const SV2& a, int h) {
  SV o;
#pragma unroll
  for (int i = 0; i < 3; ++i) { o.w[i] = h ? a.w[i].y : a.w[i].x; o.v[i] = h ? a.v[i].y : a.v[i].x; }
  return o;
}
SSD SV2 sv_pack(const SV& l, const SV& a) {
  SV2 o;
#pragma unroll
  for (int i = 0; i < 3; ++i) { o.w[i] = pkv(l.w[i], a.w[i]); o.v[i] = pkv(l.v[i], a.v[i]); }
  return o;
}
SSD ABI abi_half(const ABIP& a, int h) {
  ABI o;
#pragma unroll
  for (int i = 0; i < 6; ++i) { o.A.m[i] = h ? a.A.m[i].y : a.A.m[i].x; o.C.m[i] = h ? a.C.m[i].y : a.C.m[i].x; }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o.B[i][j] = h ? a.B[i][j].y : a.B[i][j].x;
  return o;
}

// The A and C blocks of ONE articulated inertia as a pair {A, C}: the joint's rank-one update and the rotation into the parent's
// orientation apply the same operator to both blocks (ss_dynamics.hpp uses it for the spine joints, whose chain has no twin to pair
// with).  A packed instruction is two scalar ones of the same operands: every entry keeps its bits.
SSD Sym3P sym_pack(const Sym3& A, const Sym3& C) {
  Sym3P o;
#pragma unroll
  for (int i = 0; i < 6; ++i) o.m[i] = pkv(A.m[i], C.m[i]);
  return o;
}
// xinertia of ss_math.hpp for a scalar joint, the blocks A and C given as the pair AC
template <class JT>
SSD ABI xinertia_ac(float c, float s, const Sym3P& AC, const float (&B)[3][3]) {
  const Sym3P R = rot_sym<JT::AX>(ssf2{c, c}, ssf2{s, s}, AC);
  ABI o;
#pragma unroll
  for (int i = 0; i < 6; ++i) { o.A.m[i] = R.m[i].x; o.C.m[i] = R.m[i].y; }
  xinertia_shift<JT>(c, s, B, o);
  return o;
}

template <class Model, int JL, int JA>
constexpr bool has_offsetP() { return has_offset<Model, JL>() || has_offset<Model, JA>(); }
// o = r x f with the constexpr offsets of joints JL (leg half) and JA (arm half)
// (not cross_r at T = ssf2: o2 takes ry then rx here, rx then ry there, which rounds differently)
template <class Model, int JL, int JA>
SSD void cross_rP(const ssf2 f[3], ssf2 o[3]) {
  constexpr float rxl = Model::r[JL][0], ryl = Model::r[JL][1], rzl = Model::r[JL][2];
  constexpr float rxa = Model::r[JA][0], rya = Model::r[JA][1], rza = Model::r[JA][2];
  ssf2 o0 = {0.f, 0.f}, o1 = {0.f, 0.f}, o2 = {0.f, 0.f};
  if constexpr (ryl != 0.f || rya != 0.f) { o0 += pk(ryl, rya) * f[2]; o2 -= pk(ryl, rya) * f[0]; }
  if constexpr (rzl != 0.f || rza != 0.f) { o0 -= pk(rzl, rza) * f[1]; o1 += pk(rzl, rza) * f[0]; }
  if constexpr (rxl != 0.f || rxa != 0.f) { o1 -= pk(rxl, rxa) * f[2]; o2 += pk(rxl, rxa) * f[1]; }
  o[0] = o0; o[1] = o1; o[2] = o2;
}
// the joint constants of the transforms of ss_math.hpp for the pair of joints JL (leg half) and JA (arm half)
template <class Model, int JL, int JA>
struct PairJoint {
  static_assert(kAxis[JL] == kAxis[JA], "paired joints must share their axis");
  static constexpr int AX = kAxis[JL];
  static constexpr bool offset = has_offsetP<Model, JL, JA>();
  static SSD void cross_r(const ssf2 f[3], ssf2 o[3]) { cross_rP<Model, JL, JA>(f, o); }
};
template <class Model, int BL, int BA>
constexpr bool massiveP() { return Model::mass[BL] != 0.f || Model::mass[BA] != 0.f; }
// add the constexpr rigid-body inertias of bodies BL (leg half) and BA (arm half)
// (not abi_add_body at T = ssf2: its constants are literal pairs, kept where either half is non-zero: another function of the model, not of T)
template <class Model, int BL, int BA>
SSD void abi_add_bodyP(ABIP& I) {
  constexpr float ml = Model::mass[BL], ma = Model::mass[BA];
  if constexpr (ml != 0.f || ma != 0.f) {
    constexpr float cxl = Model::com[BL][0], cyl = Model::com[BL][1], czl = Model::com[BL][2];
    constexpr float cxa = Model::com[BA][0], cya = Model::com[BA][1], cza = Model::com[BA][2];
    static_for<0, 6>([&](auto Ic) {
      constexpr int i = decltype(Ic)::value;
      constexpr float kl = Model::inertia[BL][i], ka = Model::inertia[BA][i];
      if constexpr (kl != 0.f || ka != 0.f) I.A.m[i] += pk(kl, ka);
    });
    I.C.m[0] += pk(ml, ma); I.C.m[1] += pk(ml, ma); I.C.m[2] += pk(ml, ma);
    if constexpr (czl != 0.f || cza != 0.f) { I.B[0][1] += pk(-ml * czl, -ma * cza); I.B[1][0] += pk(ml * czl, ma * cza); }
    if constexpr (cyl != 0.f || cya != 0.f) { I.B[0][2] += pk(ml * cyl, ma * cya); I.B[2][0] += pk(-ml * cyl, -ma * cya); }
    if constexpr (cxl != 0.f || cxa != 0.f) { I.B[1][2] += pk(-ml * cxl, -ma * cxa); I.B[2][1] += pk(ml * cxl, ma * cxa); }
  }
}
SSD ABIP abi_zeroP() {
  ABIP I;
  const ssf2 z = {0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 6; ++i) { I.A.m[i] = z; I.C.m[i] = z; }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) I.B[i][j] = z;
  return I;
}
// velocity-product bias forces of bodies BL / BA:  p = v x* (I_b v)
// (not body_bias at T = ssf2: n and f take their terms in another order here -- n[2], for one -- which rounds differently)
template <class Model, int BL, int BA>
SSD SV2 body_biasP(const SV2& v) {
  constexpr float ml = Model::mass[BL], ma = Model::mass[BA];
  constexpr float hxl = ml * Model::com[BL][0], hyl = ml * Model::com[BL][1], hzl = ml * Model::com[BL][2];
  constexpr float hxa = ma * Model::com[BA][0], hya = ma * Model::com[BA][1], hza = ma * Model::com[BA][2];
  const ssf2 z = {0.f, 0.f};
  ssf2 n[3] = {z, z, z}, f[3];
  static_for<0, 3>([&](auto Rc) {
    constexpr int r = decltype(Rc)::value;
    static_for<0, 3>([&](auto Cc) {
      constexpr int c = decltype(Cc)::value;
      constexpr int idx = r == c ? r : (r + c == 1 ? 3 : (r + c == 2 ? 4 : 5));
      constexpr float kl = Model::inertia[BL][idx], ka = Model::inertia[BA][idx];
      if constexpr (kl != 0.f || ka != 0.f) n[r] += pk(kl, ka) * v.w[c];
    });
  });
  if constexpr (hyl != 0.f || hya != 0.f) { n[0] += pk(hyl, hya) * v.v[2]; n[2] -= pk(hyl, hya) * v.v[0]; }
  if constexpr (hzl != 0.f || hza != 0.f) { n[0] -= pk(hzl, hza) * v.v[1]; n[1] += pk(hzl, hza) * v.v[0]; }
  if constexpr (hxl != 0.f || hxa != 0.f) { n[1] -= pk(hxl, hxa) * v.v[2]; n[2] += pk(hxl, hxa) * v.v[1]; }
  f[0] = pk(ml, ma) * v.v[0]; f[1] = pk(ml, ma) * v.v[1]; f[2] = pk(ml, ma) * v.v[2];
  if constexpr (hyl != 0.f || hya != 0.f) { f[0] -= pk(hyl, hya) * v.w[2]; f[2] += pk(hyl, hya) * v.w[0]; }
  if constexpr (hzl != 0.f || hza != 0.f) { f[0] += pk(hzl, hza) * v.w[1]; f[1] -= pk(hzl, hza) * v.w[0]; }
  if constexpr (hxl != 0.f || hxa != 0.f) { f[1] += pk(hxl, hxa) * v.w[2]; f[2] -= pk(hxl, hxa) * v.w[1]; }
  SV2 p;
  ssf2 a[3], b[3];
  cross(v.w, n, a);
  cross(v.v, f, b);
  p.w[0] = a[0] + b[0]; p.w[1] = a[1] + b[1]; p.w[2] = a[2] + b[2];
  cross(v.w, f, p.v);
  return p;
}

}  // namespace ss
