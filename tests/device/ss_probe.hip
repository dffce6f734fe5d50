// ss_probe.hip -- calls the step kernels' spatial algebra (ss_math.hpp, ss_pair.hpp, the per-joint helpers of ss_dynamics.hpp) one
// operator at a time, one case per lane, so that tests/test_spatial_ops.py can hold each operator against the fp64 reference of
// tests/np_spatial.py; and, the same way, the contact stage of ss_dynamics.hpp (detection, Jacobian rows, contact-space operators) and
// the env formulas of ss_kernels.hpp (sampler, observation terms, reset noise) for tests/test_contact_ops.py / tests/np_contact_ops.py;
// and one whole substep<Model, 0> on the lane pair of a robot for tests/test_substep.py / tests/substep_cases.py; and the forms the
// step kernels use in place of older ones, each beside its reference, for the tests that require the two sides to agree BITWISE: the
// half-broadcast packed multiply(-add) of ss_pair.hpp (tests/test_pair_broadcast.py), the joint-limit and joint-torque forms of
// ss_dynamics.hpp (tests/test_limit_forms.py) and joint_tau's {leg, arm} pair overload (tests/test_pair_response.py); and the env logic
// of a control step behind its substeps (ss_kernels.hpp: step_logic on the lane pair, step_score and ep_return_add by value) for
// tests/test_step_logic.py / tests/np_step_logic.py.  A second entry, ssp_mlp (at the end of the file), runs one MLP phase of the
// closed-loop look-ahead (ss_policy.hpp) and dumps its activation blocks for tests/test_policy_ops.py / tests/np_policy.py.
// TEST INFRASTRUCTURE ONLY: never part of libsteppingstone.so, nothing in the package loads it.
//
// The same source is compiled two ways:
//   * for gfx950 by steppingstone_amd/build.py: build_probe() -> steppingstone_amd/lib/libss_probe.so (the product's flags); ssp_run
//     takes DEVICE pointers and a stream, launches whole wavefronts of 64 (the lane exchange needs every lane active) and guards
//     only its stores by n;
//   * for the CPU by tests/probe_lib.py (-DSS_PROBE_HOST, the host recipe of tests/native_build.py); ssp_run loops over the cases with host pointers.
//     The lane exchange has no meaning there: that op answers SSP_UNSUPPORTED, and every other op sees the identity -- but `substep`
//     and `step_logic`, whose two lanes run as two threads that meet at every exchange.
//
//   int ssp_run(int op, int kind, int n, const float* in, float* out, void* stream)
//     in [n][IN_W(op)], out [n][OUT_W(op)], row-major; kind 0 = ModelWalker3D, 1 = ModelMike.  Joint / body / pair numbers are
//     columns of the input (as floats) and select the compile-time instantiation; words that are integers to the operator
//     (Philox, xchg_u32, xchg_i) travel as raw bits.  n == 0 reads and writes nothing and returns IN_W * 1000 + OUT_W, so that the
//     caller sizes its buffers from the library itself.  Returns 0, or a negative SSP_* / the HIP error of the launch.
//     An op given a joint number it is not instantiated for (see the lists below) leaves zeros.
//   The ops from fk_detect to substep, and step_logic, work on a lane-private Lds view as the step kernels do: on the device one __shared__ block of
//   kLdsSlots * kWave float4 per wavefront and Lds{base, lane}; on the host one such block per case (filled with NaN first) and lane 0.
#include <hip/hip_runtime.h>

#include <cstdint>

#include <limits>
#include <vector>

#include "../../steppingstone_amd/csrc/ss_kernels.hpp"
#include "../../steppingstone_amd/csrc/ss_policy.hpp"

#if !defined(__HIP_DEVICE_COMPILE__)
#include <atomic>
#include <thread>
// The lane exchange on the host.  Every op but `substep` runs one lane per case on the calling thread, which has no partner: the
// exchange is the identity (contact_ops forms C with the lane as its own partner; the exchange op itself is refused).  `substep` and
// `step_logic` run the two lanes of a robot as two threads that meet at every exchange, as tests/host/host_harness.cpp's lanes do.
namespace {
// A lane that leaves its case while its partner waits in an exchange did not take part in it: step_logic forms `finite` as
// finite_bits(own) && (xchg_i(...) != 0), so a lane whose own sum is not finite skips that exchange (the last one of the function).  On
// the device the partner's DPP move then reads a disabled lane, which gives 0 (bound_ctrl), "not finite"; here the waiting lane gets the
// same 0 once the partner is gone.
struct PairSync {
  std::atomic<int> arrived{0}, generation{0}, gone{0};
  float slot[2];
  bool wait() {       // false: the partner has left
    const int g = generation.load(std::memory_order_acquire);
    if (arrived.fetch_add(1, std::memory_order_acq_rel) == 1) {
      arrived.store(0, std::memory_order_relaxed);
      generation.store(g + 1, std::memory_order_release);
    } else {
      while (generation.load(std::memory_order_acquire) == g) {
        if (gone.load(std::memory_order_acquire) != 0) {
          arrived.fetch_sub(1, std::memory_order_acq_rel);
          return false;
        }
        std::this_thread::yield();
      }
    }
    return true;
  }
};
thread_local PairSync* t_sync = nullptr;      // null: no partner
thread_local int t_side = 0;
}  // namespace
float ss_host_xchg(float x) {
  PairSync* s = t_sync;
  if (!s) return x;
  s->slot[t_side] = x;
  if (!s->wait()) return __builtin_bit_cast(float, 0u);
  const float r = s->slot[1 - t_side];
  s->wait();
  return r;
}
void ss_host_wave_sync() {}
#endif

namespace ssp {
using namespace ss;

enum {
  OP_ROT = 0,          // [ax, c, s, v3]                           -> rot<ax> 3, rotT<ax> 3                      (float)
  OP_ROT2,             // [ax, (c, s, v3) x 2]                     -> per half: rot 3, rotT 3                    (ssf2)
  OP_CROSS_R,          // [J, f3]                                  -> r_J x f
  OP_CROSS_RP,         // [i, f3 leg, f3 arm]                      -> per half 3                    joints (3+i, 13+i)
  OP_XMOTION,          // [J, c, s, p6]                            -> 6
  OP_XFORCE,           // [J, c, s, f6]                            -> 6
  OP_XMOTION_P,        // [i, (c, s, p6) x 2]                      -> per half 6
  OP_XFORCE_P,         // [i, (c, s, f6) x 2]                      -> per half 6
  OP_XINERTIA,         // [J, c, s, abi21]                         -> abi21         abi21 = A.m[6], B[3][3] row-major, C.m[6]
  OP_XINERTIA_P,       // [i, (c, s, abi21) x 2]                   -> per half abi21
  OP_ABI_BODY,         // [b, abi21]                               -> abi_body<b> 21, abi_add_body<b>(input) 21
  OP_ABI_ADD_BODYP,    // [i, abi21 x 2]                           -> per half abi21                bodies (4+i, 14+i)
  OP_BODY_BIAS,        // [b, v6]                                  -> 6
  OP_BODY_BIASP,       // [i, v6 x 2]                              -> per half 6                    bodies (4+i, 14+i)
  OP_IMP_UP,           // [J, rec10, p6]                           -> 6, ul[k]      rec10 = cs, sn, Uw3, Uv3, Dinv, u
  OP_IMP_DOWN,         // [J, loaded, rec10, ul, d6]               -> 6, dq
  OP_IMP_DOWN_PAIR,    // [J, rec10, p6 x 2]                       -> per column 6
  OP_IMP_UP_PAIR,      // [J, rec10, p6 x 2]                       -> per column 6, then ul2[k] (2)
  OP_IMP_DOWN_PAIR_LD, // [J, rec10, ul2 (2), p6 x 2]              -> per column 6
  OP_ABA_ACC,          // [J, rec10, qd, aprev6, vb6]              -> 6, qdd
  OP_ABA_ACC_P,        // [i, (rec10, qd, aprev6, vb6) x 2]        -> per half 6, qdd
  OP_QUAT_ROT,         // [q4]                                     -> 9
  OP_MIRROR_SV,        // [a6]                                     -> 6
  OP_ABI_DENSE,        // [abi21]                                  -> 36
  OP_PACK,             // [l6, a6, abi21 l, abi21 a]               -> sv_half(sv_pack(l, a), 0 / 1), abi_half(pack, 0 / 1)
  OP_SINCOS,           // [x]                                      -> s, c
  OP_CHOL,             // [M 36, b0 6, b1 6]                       -> l15, di6, x(b0) 6, x(b1) 6 (float), pair solve: half 0 6, half 1 6
  OP_XCHG,             // [f, u32, i, sv6, abi21]                  -> xchg, xchg_u32, xchg_i, xchg_sv 6, xchg_abi 21   (device only)
  OP_PHILOX,           // [c0..c3, k0, k1, x] (raw bits)           -> out[4] (raw bits), u01(x)
  // ---- the contact stage and the env formulas.  Integers travel as float VALUES here (all are small).  A 6x6 operator is six columns of
  // six (column-major; a column is w0 w1 w2 v0 v1 v2).
  OP_FK_DETECT,        // [cs8, sn8, Rb 9 (row-major), pos 3, (centre 3, normal 3, cos, sin of the heading) x stones n-1, n, n+1]
                       //                                          -> per coding (BRANCHFREE, then &&): Rf 9, pen 4, active, cslot, contact, on_target, sole 3
  OP_JACOBIAN_ROWS,    // [Rf 9, pen 4, active, cslot, normal 3 x 3 stones] -> rWp: 12 rows (corner * 3 + direction) of (c x dir 3, dir 3), rB 4
  OP_CONTACT_OPS,      // [rec10 x 8 (joints 0..7), l15, di6]      -> T 36, C 36, Lambda_own 36 (T, C read back from kLdsT / kLdsC), then the
                       //                                             intermediates of operator_pair_b, formed a second time from the same calls:
                       //                                             p 36 (the impulses at the base), x 36 (the base solve), G 36 (pelvis twist);
                       //                                             device: lanes 2i, 2i + 1 are the two feet of a robot; host: the lane is its own partner
  OP_SAMPLER,          // [prob 121, u, (px, py, pz, dr, cp, sp, cph, sph), (phi, xt, yt)]
                       //                                          -> sample_cell: shared grid, per-env grid [121][kWave]; yaw_sample(0..10), pitch_sample(0..10),
                       //                                             place_stone 3, stone_normal 3
  OP_WINDOW_PROB,      // [level, ring]                            -> 121                                       (host only)
  OP_OBS_TERMS,        // [quat 4, (cy, sy), pos 3, stone 3, tilt 2, x, q 21, qd 21, 6 Philox blocks (24 words, raw bits)]
                       //                                          -> roll, pitch, cy, sy (quat); target_features 5 (given cy, sy); planar_dist(stone, pos);
                       //                                             clip5(x); obs_angle 21; obs_rate 21; reset_angle 21; reset_angle 21 over
                       //                                             ClampModel (below), whose draws reach the clamps
  // ---- one whole substep.  One case is one ROBOT = two lanes (2i: the right half, 2i + 1: the left half in its y-mirrored world); the row
  // is the robot's, in the true world, and each lane takes its half of it the way step_env does.
  OP_SUBSTEP,          // [pos 3, quat 4, w 3, v 3, q 21, qd 21, act 21 (clipped, policy coordinates), power, (centre 3, normal 3, cos, sin of the
                       //  heading) x stones n-1, n, n+1, (warm key, lam 12) x right foot, left foot (each in its lane's world), calls (1 or 2)]
                       //                                          -> per lane, the raw LDS words after `calls` x substep<Model, 0>: q 12, qd 12, pos 3,
                       //                                             quat 4, w 3, v 3; Warm: key, lam 12; FootReport: contact, on_target, sole 3
  // ---- forms beside their references: the test compares the two sides bitwise.  Every word travels as raw bits (NaN payloads survive).
  OP_PK_HALF,          // [a.x, a.y, s.x, s.y, c.x, c.y] (kind ignored) -> the form under test, then its scalar reference, 2 floats each:
                       //                                             fma<0>(a,s,c) fma<1>(a,s,c) fma<0>(a,a,c) fma<1>(a,a,c) mul<0>(a,s) mul<1>(a,s)
                       //                                             mul<0>(a,a) mul<1>(a,a) | the same eight by fmaf(a.x, f, c.x), fmaf(a.y, f, c.y) /
                       //                                             a.x * f, a.y * f with f the chosen half.  (a, a): one register as pair and as factor
  OP_LIMIT_FORMS,      // [power, act, (q, qd) x joints 0..20]      -> per joint 10: viol kl dl tau Dadd of the kernels' forms (joint_limit, joint_tau),
                       //                                             then of the replaced ones (joint_tau_old below)
  OP_TAU_PAIR,         // [power, act (leg halves), act (arm halves), (q, qd) x joints 0..20]
                       //                                          -> per pair (3,13) (4,14) (5,15) (6,16) 8: tau leg, tau arm, Dadd leg, Dadd arm of
                       //                                             joint_tau's pair overload, then of joint_tau per joint
  // ---- the env logic of a control step behind its substeps (PHYSICS.md 4.3-4.10).  Words that are integers to the kernels travel as raw
  // bits, in and out.
  OP_STEP_SCORE,       // [pos 3, quat 4, centres of the stones n-1, n, n+1 (9), target_old 3, sole 3 x right, left, pot_prev, advanced, n,
                       //  elapsed, finite, step_bonus, e_sum, a2, at_limit]
                       //                                          -> StepScore: pot_prev, d, bad, r, roll, pitch, cyaw, syaw
  OP_EP_RETURN,        // [ep_ret, ep_lo, r x kEpR]                 -> (ep_ret, ep_lo) after each ep_return_add
  // One case is one ROBOT = two lanes, as for substep; the row is the robot's, in the true world, but the foot reports, each in its lane's.
  OP_STEP_LOGIC,       // [pos 3, quat 4, w 3, v 3, q 21, qd 21, act 21 (clipped, policy coordinates), FootReport (contact, on_target, sole 3)
                       //  x right, left lane, cache (p 9, nrm 9, tilt 6), headings (cos, sin) x 3, pot_prev, nn_dr, ep_ret, ep_lo, n, count,
                       //  elapsed, ctr, stub stone (p 3, nrm 3, tilt 2, heading 2, dr)]
                       //                                          -> per lane: StepEnd (pos 3, quat 4, w 3, v 3, flags, advanced, hd 6, d, bad,
                       //                                             r, roll, pitch, cyaw, syaw), pot_prev, nn_dr, ep_ret, ep_lo, n, count,
                       //                                             elapsed, ctr, cache 24, the heading items of LDS 6, the draw's record:
                       //                                             calls, k, ctr, store (of the last call)
  OP_COUNT
};
enum { SSP_BAD_OP = -1, SSP_UNSUPPORTED = -2, SSP_BAD_KIND = -3 };

constexpr int kAbi = 21, kRec = 10;
constexpr int kEpR = 100;                        // rewards per ep_return row: the test chains rows through the pair to longer episodes
constexpr int kLogicIn = 13 + 3 * NJ + 10 + 24 + 6 + 8 + 11, kLogicOut = 28 + 8 + 24 + 6 + 4;
__host__ __device__ constexpr int in_w(int op) {
  switch (op) {
    case OP_ROT: return 6;
    case OP_ROT2: return 11;
    case OP_CROSS_R: return 4;
    case OP_CROSS_RP: return 7;
    case OP_XMOTION: case OP_XFORCE: return 9;
    case OP_XMOTION_P: case OP_XFORCE_P: return 17;
    case OP_XINERTIA: return 3 + kAbi;
    case OP_XINERTIA_P: return 1 + 2 * (2 + kAbi);
    case OP_ABI_BODY: return 1 + kAbi;
    case OP_ABI_ADD_BODYP: return 1 + 2 * kAbi;
    case OP_BODY_BIAS: return 7;
    case OP_BODY_BIASP: return 13;
    case OP_IMP_UP: return 1 + kRec + 6;
    case OP_IMP_DOWN: return 2 + kRec + 1 + 6;
    case OP_IMP_DOWN_PAIR: case OP_IMP_UP_PAIR: return 1 + kRec + 12;
    case OP_IMP_DOWN_PAIR_LD: return 1 + kRec + 2 + 12;
    case OP_ABA_ACC: return 1 + kRec + 13;
    case OP_ABA_ACC_P: return 1 + 2 * (kRec + 13);
    case OP_QUAT_ROT: return 4;
    case OP_MIRROR_SV: return 6;
    case OP_ABI_DENSE: return kAbi;
    case OP_PACK: return 12 + 2 * kAbi;
    case OP_SINCOS: return 1;
    case OP_CHOL: return 48;
    case OP_XCHG: return 9 + kAbi;
    case OP_PHILOX: return 7;
    case OP_FK_DETECT: return 16 + 9 + 3 + 24;
    case OP_JACOBIAN_ROWS: return 9 + 4 + 2 + 9;
    case OP_CONTACT_OPS: return 8 * kRec + 21;
    case OP_SAMPLER: return SS_NCELL + 1 + 8 + 3;
    case OP_WINDOW_PROB: return 2;
    case OP_OBS_TERMS: return 15 + 2 * NJ + 24;
    case OP_SUBSTEP: return 13 + 3 * NJ + 1 + 24 + 2 * 13 + 1;
    case OP_PK_HALF: return 6;
    case OP_LIMIT_FORMS: return 2 + 2 * NJ;
    case OP_TAU_PAIR: return 3 + 2 * NJ;
    case OP_STEP_SCORE: return 3 + 4 + 9 + 3 + 6 + 1 + 8;
    case OP_EP_RETURN: return 2 + kEpR;
    case OP_STEP_LOGIC: return kLogicIn;
    default: return 0;
  }
}
__host__ __device__ constexpr bool needs_lds(int op) { return (op >= OP_FK_DETECT && op <= OP_SUBSTEP) || op == OP_STEP_LOGIC; }
__host__ __device__ constexpr int lanes_per_case(int op) { return (op == OP_SUBSTEP || op == OP_STEP_LOGIC) ? 2 : 1; }      // out_w is per case: lanes x words
constexpr int kSubOut = 2 * NH + 13 + 13 + 5;
__host__ __device__ constexpr int out_w(int op) {
  switch (op) {
    case OP_ROT: return 6;
    case OP_ROT2: return 12;
    case OP_CROSS_R: return 3;
    case OP_CROSS_RP: return 6;
    case OP_XMOTION: case OP_XFORCE: return 6;
    case OP_XMOTION_P: case OP_XFORCE_P: return 12;
    case OP_XINERTIA: return kAbi;
    case OP_XINERTIA_P: return 2 * kAbi;
    case OP_ABI_BODY: return 2 * kAbi;
    case OP_ABI_ADD_BODYP: return 2 * kAbi;
    case OP_BODY_BIAS: return 6;
    case OP_BODY_BIASP: return 12;
    case OP_IMP_UP: return 7;
    case OP_IMP_DOWN: return 7;
    case OP_IMP_DOWN_PAIR: return 12;
    case OP_IMP_UP_PAIR: return 14;
    case OP_IMP_DOWN_PAIR_LD: return 12;
    case OP_ABA_ACC: return 7;
    case OP_ABA_ACC_P: return 14;
    case OP_QUAT_ROT: return 9;
    case OP_MIRROR_SV: return 6;
    case OP_ABI_DENSE: return 36;
    case OP_PACK: return 12 + 2 * kAbi;
    case OP_SINCOS: return 2;
    case OP_CHOL: return 45;
    case OP_XCHG: return 9 + kAbi;
    case OP_PHILOX: return 5;
    case OP_FK_DETECT: return 2 * 20;
    case OP_JACOBIAN_ROWS: return 72 + 4;
    case OP_CONTACT_OPS: return 216;
    case OP_SAMPLER: return 2 + 22 + 3 + 3;
    case OP_WINDOW_PROB: return SS_NCELL;
    case OP_OBS_TERMS: return 11 + 4 * NJ;
    case OP_SUBSTEP: return 2 * kSubOut;
    case OP_PK_HALF: return 32;
    case OP_LIMIT_FORMS: return 10 * NJ;
    case OP_TAU_PAIR: return 32;
    case OP_STEP_SCORE: return 8;
    case OP_EP_RETURN: return 2 * kEpR;
    case OP_STEP_LOGIC: return 2 * kLogicOut;
    default: return 0;
  }
}

// ---- rows <-> the kernels' types
SSD SV rd_sv(const float*& p) {
  SV a = {{p[0], p[1], p[2]}, {p[3], p[4], p[5]}};
  p += 6;
  return a;
}
SSD void wr_sv(float*& o, const SV& a) {
#pragma unroll
  for (int i = 0; i < 3; ++i) { o[i] = a.w[i]; o[3 + i] = a.v[i]; }
  o += 6;
}
SSD ABI rd_abi(const float*& p) {
  ABI I;
#pragma unroll
  for (int i = 0; i < 6; ++i) { I.A.m[i] = p[i]; I.C.m[i] = p[15 + i]; }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) I.B[i][j] = p[6 + 3 * i + j];
  p += kAbi;
  return I;
}
SSD void wr_abi(float*& o, const ABI& I) {
#pragma unroll
  for (int i = 0; i < 6; ++i) { o[i] = I.A.m[i]; o[15 + i] = I.C.m[i]; }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o[6 + 3 * i + j] = I.B[i][j];
  o += kAbi;
}
SSD JRec rd_rec(const float*& p) {
  JRec r;
  r.cs = p[0]; r.sn = p[1];
#pragma unroll
  for (int i = 0; i < 3; ++i) { r.Uw[i] = p[2 + i]; r.Uv[i] = p[5 + i]; }
  r.Dinv = p[8]; r.u = p[9];
  p += kRec;
  return r;
}
SSD ABIP abi_pack(const ABI& l, const ABI& a) {
  ABIP o;
#pragma unroll
  for (int i = 0; i < 6; ++i) { o.A.m[i] = ssf2{l.A.m[i], a.A.m[i]}; o.C.m[i] = ssf2{l.C.m[i], a.C.m[i]}; }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o.B[i][j] = ssf2{l.B[i][j], a.B[i][j]};
  return o;
}
SSD JRec2 rec_pack(const JRec& l, const JRec& a) {
  JRec2 r;
  r.cs = ssf2{l.cs, a.cs}; r.sn = ssf2{l.sn, a.sn}; r.Dinv = ssf2{l.Dinv, a.Dinv}; r.u = ssf2{l.u, a.u};
#pragma unroll
  for (int i = 0; i < 3; ++i) { r.Uw[i] = ssf2{l.Uw[i], a.Uw[i]}; r.Uv[i] = ssf2{l.Uv[i], a.Uv[i]}; }
  return r;
}
SSD uint32_t bits(float x) { return __builtin_bit_cast(uint32_t, x); }
SSD float unbits(uint32_t x) { return __builtin_bit_cast(float, x); }

// run f(integral_constant<J>) for the J in [LO, HI) that equals the run-time j
template <int LO, int HI, class F>
SSD void pick(int j, F&& f) {
  static_for<LO, HI>([&](auto Jc) {
    if (j == decltype(Jc)::value) f(Jc);
  });
}

// every lane of the wavefront has finished with the shared block (the sampler stages two layouts in it, one after the other)
#if defined(__HIP_DEVICE_COMPILE__)
#define SSP_WAVE_SYNC() __syncthreads()
#else
#define SSP_WAVE_SYNC() ((void)0)
#endif
SSD void wr_col(float* o, int col, const ssf2& a, const ssf2& b, const ssf2& c) {
  o[6 * col + 0] = a.x; o[6 * col + 1] = a.y; o[6 * col + 2] = b.x; o[6 * col + 3] = b.y; o[6 * col + 4] = c.x; o[6 * col + 5] = c.y;
}

// the two columns a packed recursion carries, as columns 2c and 2c + 1 of a column-major 6x6
SSD void wr_pair(float* dst, const SV2& a) {
#pragma unroll
  for (int i = 0; i < 3; ++i) { dst[i] = a.w[i].x; dst[3 + i] = a.v[i].x; dst[6 + i] = a.w[i].y; dst[9 + i] = a.v[i].y; }
}
// reset_angle's clamps cannot be reached with the shipped robots (no q0 within 0.07 of a limit).  This model exists for that one
// function: q0 sits 0.03 inside lo (even joints) or hi (odd joints) of ranges of different sizes, so the draws q0 +- 0.05 meet
// lo + 0.02 / hi - 0.02 from both sides.
struct ClampModel {
  static constexpr float lo[21] = {-1.0f, -0.5f, -0.25f, 0.1f, -2.0f, -0.3f, 0.7f, -1.5f, -0.6f, 0.2f, -0.9f,
                                   -1.1f, -0.4f, 0.3f, -2.5f, -0.7f, 0.5f, -1.3f, -0.8f, 0.4f, -0.2f};
  static constexpr float hi[21] = {1.0f, 0.75f, 0.5f, 1.1f, -0.5f, 0.3f, 2.9f, 0.6f, 0.6f, 1.2f, 0.9f,
                                   1.3f, 0.4f, 2.3f, -1.5f, 0.7f, 1.5f, -0.3f, 0.8f, 0.9f, 0.2f};
  static constexpr float q0[21] = {-0.97f, 0.72f, -0.22f, 1.07f, -1.97f, 0.27f, 0.73f, 0.57f, -0.57f, 1.17f, -0.87f,
                                   1.27f, -0.37f, 2.27f, -2.47f, 0.67f, 0.53f, -0.33f, -0.77f, 0.87f, -0.17f};
};

// ---- the forms beside their references
// the scalar reference of the half-broadcast forms: the factor and the operands made opaque one by one, so that each product is
// an instruction of its own
SSD float opaque(float x) { SS_REG(x); return x; }
SSD void ref_fma(ssf2 a, float f, ssf2 c, float* o) {
  o[0] = __builtin_fmaf(opaque(a.x), opaque(f), opaque(c.x));
  o[1] = __builtin_fmaf(opaque(a.y), opaque(f), opaque(c.y));
}
SSD void ref_mul(ssf2 a, float f, float* o) {
  o[0] = opaque(a.x) * opaque(f);
  o[1] = opaque(a.y) * opaque(f);
}
SSD void put2(float* o, ssf2 v) { o[0] = v.x; o[1] = v.y; }

SSD void run_pk(const float* in, float* out) {
  const ssf2 a = pkv(in[0], in[1]), s = pkv(in[2], in[3]), c = pkv(in[4], in[5]);
  put2(out + 0, pk_fma_half<0>(a, s, c));
  put2(out + 2, pk_fma_half<1>(a, s, c));
  put2(out + 4, pk_fma_half<0>(a, a, c));
  put2(out + 6, pk_fma_half<1>(a, a, c));
  put2(out + 8, pk_mul_half<0>(a, s));
  put2(out + 10, pk_mul_half<1>(a, s));
  put2(out + 12, pk_mul_half<0>(a, a));
  put2(out + 14, pk_mul_half<1>(a, a));
  ref_fma(a, s.x, c, out + 16);
  ref_fma(a, s.y, c, out + 18);
  ref_fma(a, a.x, c, out + 20);
  ref_fma(a, a.y, c, out + 22);
  ref_mul(a, s.x, out + 24);
  ref_mul(a, s.y, out + 26);
  ref_mul(a, a.x, out + 28);
  ref_mul(a, a.y, out + 30);
}

// the joint-limit and joint-torque forms as the step kernels had them before joint_limit (ss_dynamics.hpp): the reference of
// tests/test_limit_forms.py, kept VERBATIM
template <class Model, int j>
SSD void joint_tau_old(float power, float q, float qd, float act, float& viol_o, float& kl_o, float& dl_o, float& tau, float& Dadd) {
  constexpr float h = kH;
  constexpr float lo = Model::lo[j], hi = Model::hi[j], kd = Model::damping[j], ks = Model::stiffness[j];
  constexpr float klim = Model::klim[j], dlim = Model::dlim[j], arm = Model::armature[j], tq = Model::torque[j];
  float viol = q > hi ? q - hi : (q < lo ? q - lo : 0.f);
  bool lim = viol != 0.f;
  float kl = lim ? klim : 0.f, dl = lim ? dlim : 0.f;
  tau = power * tq * act - kd * qd - ks * (q + h * qd) - kl * (viol + h * qd) - dl * qd;
  Dadd = arm + h * (kd + dl) + (h * h) * (ks + kl);
  viol_o = viol; kl_o = kl; dl_o = dl;
}

template <class Model>
SSD void run_limit(const float* in, float* out) {
  const float power = in[0], act = in[1];
  static_for<0, NJ>([&](auto Jc) {
    constexpr int j = decltype(Jc)::value;
    const float q = in[2 + 2 * j], qd = in[3 + 2 * j];
    float* o = out + 10 * j;
    joint_limit<Model, j>(q, o[0], o[1], o[2]);
    joint_tau<Model, j>(power, q, qd, act, o[3], o[4]);
    joint_tau_old<Model, j>(power, q, qd, act, o[5], o[6], o[7], o[8], o[9]);
  });
}

template <class Model>
SSD void run_tau(const float* in, float* out) {
  const float power = in[0], actl = in[1], acta = in[2];
  static_for<0, 4>([&](auto Ic) {
    constexpr int i = decltype(Ic)::value, jl = 3 + i, ja = 13 + i;
    const float ql = in[3 + 2 * jl], qdl = in[4 + 2 * jl], qa = in[3 + 2 * ja], qda = in[4 + 2 * ja];
    float* o = out + 8 * i;
    ssf2 tau2, dadd2;
    joint_tau<Model, jl, ja>(power, pkv(ql, qa), pkv(qdl, qda), pkv(actl, acta), tau2, dadd2);
    o[0] = tau2.x; o[1] = tau2.y; o[2] = dadd2.x; o[3] = dadd2.y;
    joint_tau<Model, jl>(power, ql, qdl, actl, o[4], o[6]);
    joint_tau<Model, ja>(power, qa, qda, acta, o[5], o[7]);
  });
}

template <class Model, int OP>
SSD void run_case(const float* p, float* o, const Lds& L) {
  (void)L;
  if constexpr (OP == OP_ROT) {
    const int ax = (int)p[0];
    const float c = p[1], s = p[2], v[3] = {p[3], p[4], p[5]};
    pick<0, 3>(ax, [&](auto Ac) {
      constexpr int AX = decltype(Ac)::value;
      rot<AX>(c, s, v, o);
      rotT<AX>(c, s, v, o + 3);
    });
  } else if constexpr (OP == OP_ROT2) {
    const int ax = (int)p[0];
    const ssf2 c = {p[1], p[6]}, s = {p[2], p[7]}, v[3] = {{p[3], p[8]}, {p[4], p[9]}, {p[5], p[10]}};
    pick<0, 3>(ax, [&](auto Ac) {
      constexpr int AX = decltype(Ac)::value;
      ssf2 a[3], b[3];
      rot<AX>(c, s, v, a);
      rotT<AX>(c, s, v, b);
#pragma unroll
      for (int i = 0; i < 3; ++i) { o[i] = a[i].x; o[3 + i] = b[i].x; o[6 + i] = a[i].y; o[9 + i] = b[i].y; }
    });
  } else if constexpr (OP == OP_CROSS_R) {
    const float f[3] = {p[1], p[2], p[3]};
    pick<0, NJ>((int)p[0], [&](auto Jc) { cross_r<Model, decltype(Jc)::value>(f, o); });
  } else if constexpr (OP == OP_CROSS_RP) {
    const ssf2 f[3] = {{p[1], p[4]}, {p[2], p[5]}, {p[3], p[6]}};
    pick<0, 4>((int)p[0], [&](auto Ic) {
      constexpr int i = decltype(Ic)::value;
      ssf2 t[3];
      cross_rP<Model, 3 + i, 13 + i>(f, t);
#pragma unroll
      for (int m = 0; m < 3; ++m) { o[m] = t[m].x; o[3 + m] = t[m].y; }
    });
  } else if constexpr (OP == OP_XMOTION || OP == OP_XFORCE) {
    const int j = (int)p[0];
    const float c = p[1], s = p[2];
    p += 3;
    const SV a = rd_sv(p);
    pick<0, NJ>(j, [&](auto Jc) {
      constexpr int J = decltype(Jc)::value;
      if constexpr (OP == OP_XMOTION) wr_sv(o, xmotion<Model, J>(c, s, a));
      else wr_sv(o, xforce<Model, J>(c, s, a));
    });
  } else if constexpr (OP == OP_XMOTION_P || OP == OP_XFORCE_P) {
    const int i_ = (int)p[0];
    const ssf2 c = {p[1], p[9]}, s = {p[2], p[10]};
    const float *pl = p + 3, *pa = p + 11;
    const SV2 a = sv_pack(rd_sv(pl), rd_sv(pa));
    pick<0, 4>(i_, [&](auto Ic) {
      constexpr int i = decltype(Ic)::value;
      using JT = PairJoint<Model, 3 + i, 13 + i>;
      SV2 r;
      if constexpr (OP == OP_XMOTION_P) r = xmotion<JT>(c, s, a);
      else r = xforce<JT>(c, s, a);
      wr_sv(o, sv_half(r, 0));
      wr_sv(o, sv_half(r, 1));
    });
  } else if constexpr (OP == OP_XINERTIA) {
    const int j = (int)p[0];
    const float c = p[1], s = p[2];
    p += 3;
    const ABI I = rd_abi(p);
    pick<0, NJ>(j, [&](auto Jc) { wr_abi(o, xinertia<Model, decltype(Jc)::value>(c, s, I)); });
  } else if constexpr (OP == OP_XINERTIA_P) {
    const int i_ = (int)p[0];
    const ssf2 c = {p[1], p[3 + kAbi]}, s = {p[2], p[4 + kAbi]};
    const float *pl = p + 3, *pa = p + 5 + kAbi;
    const ABIP I = abi_pack(rd_abi(pl), rd_abi(pa));
    pick<0, 4>(i_, [&](auto Ic) {
      constexpr int i = decltype(Ic)::value;
      const ABIP r = xinertia<PairJoint<Model, 3 + i, 13 + i>>(c, s, I);
      wr_abi(o, abi_half(r, 0));
      wr_abi(o, abi_half(r, 1));
    });
  } else if constexpr (OP == OP_ABI_BODY) {
    const int b = (int)p[0];
    p += 1;
    ABI I = rd_abi(p);
    pick<0, NB>(b, [&](auto Bc) {
      constexpr int Bd = decltype(Bc)::value;
      wr_abi(o, abi_body<Model, Bd>());
      abi_add_body<Model, Bd>(I);
      wr_abi(o, I);
    });
  } else if constexpr (OP == OP_ABI_ADD_BODYP) {
    const int i_ = (int)p[0];
    p += 1;
    const ABI Il = rd_abi(p), Ia = rd_abi(p);
    ABIP I = abi_pack(Il, Ia);
    pick<0, 4>(i_, [&](auto Ic) {
      constexpr int i = decltype(Ic)::value;
      abi_add_bodyP<Model, 4 + i, 14 + i>(I);
      wr_abi(o, abi_half(I, 0));
      wr_abi(o, abi_half(I, 1));
    });
  } else if constexpr (OP == OP_BODY_BIAS) {
    const int b = (int)p[0];
    p += 1;
    const SV v = rd_sv(p);
    pick<0, NB>(b, [&](auto Bc) { wr_sv(o, body_bias<Model, decltype(Bc)::value>(v)); });
  } else if constexpr (OP == OP_BODY_BIASP) {
    const int i_ = (int)p[0];
    p += 1;
    const SV vl = rd_sv(p), va = rd_sv(p);
    const SV2 v = sv_pack(vl, va);
    pick<0, 4>(i_, [&](auto Ic) {
      constexpr int i = decltype(Ic)::value;
      const SV2 r = body_biasP<Model, 4 + i, 14 + i>(v);
      wr_sv(o, sv_half(r, 0));
      wr_sv(o, sv_half(r, 1));
    });
  } else if constexpr (OP == OP_IMP_UP) {
    // ss_dynamics.hpp, solve(): "accumulated foot wrenches -> whole tree": imp_up<Model, 7..3> then <2..0>
    const int j = (int)p[0];
    p += 1;
    const JRec r = rd_rec(p);
    const SV a = rd_sv(p);
    pick<0, 8>(j, [&](auto Jc) {
      constexpr int J = decltype(Jc)::value;
      JointCache jc;
      jc.r[half_pos(J)] = r;
      float ul[NH];
      wr_sv(o, imp_up<Model, J>(jc, ul, a));
      o[0] = ul[half_pos(J)];
    });
  } else if constexpr (OP == OP_IMP_DOWN) {
    // same place: imp_down<Model, 0..7, true> down spine and leg, imp_down<Model, 13..16, false> down the arm
    const int j = (int)p[0];
    const bool loaded = p[1] != 0.f;
    p += 2;
    const JRec r = rd_rec(p);
    const float ulk = p[0];
    p += 1;
    const SV a = rd_sv(p);
    pick<0, 17>(j, [&](auto Jc) {
      constexpr int J = decltype(Jc)::value;
      if constexpr (J <= 7 || J >= 13) {
        JointCache jc;
        jc.r[half_pos(J)] = r;
        float ul[NH];
        ul[half_pos(J)] = ulk;
        float dq = 0.f;
        if constexpr (J <= 7) {
          if (loaded) wr_sv(o, imp_down<Model, J, true>(jc, ul, a, &dq));
        } else {
          if (!loaded) wr_sv(o, imp_down<Model, J, false>(jc, ul, a, &dq));
        }
        if ((J <= 7) == loaded) o[0] = dq;
      }
    });
  } else if constexpr (OP == OP_IMP_DOWN_PAIR || OP == OP_IMP_UP_PAIR || OP == OP_IMP_DOWN_PAIR_LD) {
    // imp_down_pair<Model, 3..7>: operator_T; <0..7> through imp_down_pair_loaded.  imp_up_pair<Model, 7..3>: operator_up, <2..0>:
    // operator_pair_b.  imp_down_pair_loaded<Model, 0..2> and <3..7>: operator_pair_b.  The pair is two COLUMNS through one joint.
    const int j = (int)p[0];
    p += 1;
    const JRec r = rd_rec(p);
    ssf2 ulk = {0.f, 0.f};
    if constexpr (OP == OP_IMP_DOWN_PAIR_LD) { ulk = ssf2{p[0], p[1]}; p += 2; }
    const SV a0 = rd_sv(p), a1 = rd_sv(p);
    const SV2 a = sv_pack(a0, a1);
    pick<0, 8>(j, [&](auto Jc) {
      constexpr int J = decltype(Jc)::value;
      JointCache jc;
      jc.r[half_pos(J)] = r;
      ssf2 ul2[NH];
      ul2[half_pos(J)] = ulk;
      SV2 d;
      if constexpr (OP == OP_IMP_DOWN_PAIR) d = imp_down_pair<Model, J>(jc, a);
      else if constexpr (OP == OP_IMP_UP_PAIR) d = imp_up_pair<Model, J>(jc, ul2, a);
      else d = imp_down_pair_loaded<Model, J>(jc, ul2, a);
      wr_sv(o, sv_half(d, 0));
      wr_sv(o, sv_half(d, 1));
      if constexpr (OP == OP_IMP_UP_PAIR) { o[0] = ul2[half_pos(J)].x; o[1] = ul2[half_pos(J)].y; }
    });
  } else if constexpr (OP == OP_ABA_ACC) {
    // substep(), pass 3, acc_scalar: aba_acc<Joint<Model, j>> for the spine 0, 1, 2 and the ankle 7
    const int j = (int)p[0];
    p += 1;
    const JRec r = rd_rec(p);
    const float qd = p[0];
    p += 1;
    const SV ap = rd_sv(p), vb = rd_sv(p);
    pick<0, 8>(j, [&](auto Jc) {
      constexpr int J = decltype(Jc)::value;
      if constexpr (J <= 2 || J == 7) {
        float qdd;
        wr_sv(o, aba_acc<Joint<Model, J>>(r, qd, ap, vb, qdd));
        o[0] = qdd;
      }
    });
  } else if constexpr (OP == OP_ABA_ACC_P) {
    // substep(), pass 3: aba_acc<PairJoint<Model, 3 + i, 13 + i>> for i = 0..3
    const int i_ = (int)p[0];
    p += 1;
    const JRec rl = rd_rec(p);
    const float qdl = p[0];
    p += 1;
    const SV apl = rd_sv(p), vbl = rd_sv(p);
    const JRec ra = rd_rec(p);
    const float qda = p[0];
    p += 1;
    const SV apa = rd_sv(p), vba = rd_sv(p);
    const JRec2 r = rec_pack(rl, ra);
    const ssf2 qd = {qdl, qda};
    const SV2 ap = sv_pack(apl, apa), vb = sv_pack(vbl, vba);
    pick<0, 4>(i_, [&](auto Ic) {
      constexpr int i = decltype(Ic)::value;
      ssf2 qdd;
      const SV2 a = aba_acc<PairJoint<Model, 3 + i, 13 + i>>(r, qd, ap, vb, qdd);
      wr_sv(o, sv_half(a, 0));
      o[0] = qdd.x;
      o += 1;
      wr_sv(o, sv_half(a, 1));
      o[0] = qdd.y;
    });
  } else if constexpr (OP == OP_QUAT_ROT) {
    const float q[4] = {p[0], p[1], p[2], p[3]};
    float R[3][3];
    quat_rot(q, R);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) o[3 * i + j] = R[i][j];
  } else if constexpr (OP == OP_MIRROR_SV) {
    wr_sv(o, mirror_sv(rd_sv(p)));
  } else if constexpr (OP == OP_ABI_DENSE) {
    const ABI I = rd_abi(p);
    float M[6][6];
    abi_dense(I, M);
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) o[6 * i + j] = M[i][j];
  } else if constexpr (OP == OP_PACK) {
    const SV l = rd_sv(p), a = rd_sv(p);
    const ABI Il = rd_abi(p), Ia = rd_abi(p);
    const SV2 s2 = sv_pack(l, a);
    const ABIP I2 = abi_pack(Il, Ia);
    wr_sv(o, sv_half(s2, 0));
    wr_sv(o, sv_half(s2, 1));
    wr_abi(o, abi_half(I2, 0));
    wr_abi(o, abi_half(I2, 1));
  } else if constexpr (OP == OP_SINCOS) {
    ss_sincos(p[0], o[0], o[1]);
  } else if constexpr (OP == OP_CHOL) {
    float M[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) M[i][j] = p[6 * i + j];
    p += 36;
    const SV b0 = rd_sv(p), b1 = rd_sv(p);
    const Chol6 L = chol6(M);
#pragma unroll
    for (int i = 0; i < 15; ++i) o[i] = L.l[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) o[15 + i] = L.di[i];
    o += 21;
    wr_sv(o, chol6_solve_neg(L, b0));
    wr_sv(o, chol6_solve_neg(L, b1));
    const SV2 x2 = chol6_solve_neg(L, sv_pack(b0, b1));
    wr_sv(o, sv_half(x2, 0));
    wr_sv(o, sv_half(x2, 1));
  } else if constexpr (OP == OP_XCHG) {
    o[0] = xchg(p[0]);
    o[1] = unbits(xchg_u32(bits(p[1])));
    o[2] = unbits((uint32_t)xchg_i((int)bits(p[2])));
    p += 3;
    o += 3;
    const SV a = rd_sv(p);
    const ABI I = rd_abi(p);
    wr_sv(o, xchg_sv(a));
    wr_abi(o, xchg_abi(I));
  } else if constexpr (OP == OP_PHILOX) {
    uint32_t r[4];
    philox4x32_10(bits(p[0]), bits(p[1]), bits(p[2]), bits(p[3]), bits(p[4]), bits(p[5]), r);
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = unbits(r[i]);
    o[4] = u01(bits(p[6]));
  } else if constexpr (OP == OP_FK_DETECT) {
    // the stones as the step kernel places them: S_POS, S_STP, S_STN (scalars) and the headings as float2 items at kLdsHead
    float Rb[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Rb[i][j] = p[16 + 3 * i + j];
#pragma unroll
    for (int a = 0; a < 3; ++a) L.s(S_POS + a) = p[25 + a];
#pragma unroll
    for (int sl = 0; sl < 3; ++sl) {
#pragma unroll
      for (int i = 0; i < 3; ++i) { L.s(S_STP + sl * 3 + i) = p[28 + sl * 8 + i]; L.s(S_STN + sl * 3 + i) = p[28 + sl * 8 + 3 + i]; }
      L.q2(kLdsHead + sl) = make_float2(p[28 + sl * 8 + 6], p[28 + sl * 8 + 7]);
    }
    static_for<0, 2>([&](auto Bc) {
      constexpr bool BRANCHFREE = decltype(Bc)::value == 0;
      DetectOut det;
      FootReport fr;
      fk_detect<Model, BRANCHFREE>(p, p + 8, Rb, L, det, fr);
      float* q = o + 20 * decltype(Bc)::value;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) q[3 * i + j] = det.Rf[i][j];
#pragma unroll
      for (int k = 0; k < 4; ++k) q[9 + k] = det.pen[k];
      q[13] = (float)det.active; q[14] = (float)det.cslot; q[15] = (float)fr.contact; q[16] = (float)fr.on_target;
#pragma unroll
      for (int i = 0; i < 3; ++i) q[17 + i] = fr.sole[i];
    });
  } else if constexpr (OP == OP_JACOBIAN_ROWS) {
    DetectOut det;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) det.Rf[i][j] = p[3 * i + j];
#pragma unroll
    for (int k = 0; k < 4; ++k) det.pen[k] = p[9 + k];
    det.active = (int)p[13];
    det.cslot = (int)p[14];
#pragma unroll
    for (int i = 0; i < 9; ++i) L.s(S_STN + i) = p[15 + i];
    ssf2 rWp[12][3];
    float rB[4];
    jacobian_rows<Model>(det, L, rWp, rB);
#pragma unroll
    for (int row = 0; row < 12; ++row) wr_col(o, row, rWp[row][0], rWp[row][1], rWp[row][2]);
#pragma unroll
    for (int k = 0; k < 4; ++k) o[72 + k] = rB[k];
  } else if constexpr (OP == OP_CONTACT_OPS) {
    // substep(), the HELPERS == 0 branch: opaque copies of the records, all six T columns, then per column pair up the leg and part B
    JointCache jin, jo;
#pragma unroll
    for (int k = 0; k < 8; ++k) jin.r[k] = rd_rec(p);
#pragma unroll
    for (int i = 0; i < 15; ++i) jin.L0.l[i] = p[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) jin.L0.di[i] = p[15 + i];
    operator_records_leg(jin, jo);
    operator_records_spine(jin, jo);
    static_for<0, 3>([&](auto Cc) { operator_T<Model, decltype(Cc)::value>(jo, L); });
    static_for<0, 3>([&](auto Cc) {
      constexpr int c = decltype(Cc)::value;
      OpCarry oc;
      operator_up<Model, c>(jo, oc);
      const LamPair lp = operator_pair_b<Model, c>(L, jo, oc);
      wr_col(o + 72, 2 * c, lp.a[0], lp.a[1], lp.a[2]);
      wr_col(o + 72, 2 * c + 1, lp.b[0], lp.b[1], lp.b[2]);
      // the first half of operator_pair_b once more, for its intermediates (the same calls on the same data: the same bits)
      OpCarry o2;
      operator_up<Model, c>(jo, o2);
      SV2 pp = o2.p;
      static_rfor<2, 0>([&](auto Jc) { pp = imp_up_pair<Model, decltype(Jc)::value>(jo, o2.ul2, pp); });
      SV2 dd = chol6_solve_neg(jo.L0, pp);
      const SV2 xx = dd;
      static_for<0, 3>([&](auto Jc) { dd = imp_down_pair_loaded<Model, decltype(Jc)::value>(jo, o2.ul2, dd); });
      wr_pair(o + 108 + 12 * c, pp);
      wr_pair(o + 144 + 12 * c, xx);
      wr_pair(o + 180 + 12 * c, dd);
    });
#pragma unroll
    for (int l = 0; l < 6; ++l)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float2 t = L.q2(kLdsT + l * 3 + i), c = L.q2(kLdsC + l * 3 + i);
        o[6 * l + 2 * i] = t.x; o[6 * l + 2 * i + 1] = t.y;
        o[36 + 6 * l + 2 * i] = c.x; o[36 + 6 * l + 2 * i + 1] = c.y;
      }
  } else if constexpr (OP == OP_SAMPLER) {
    Params P = {};
    Knobs K = {};
    P.npad = kWave;
    const float u = p[SS_NCELL];
    float* shared_grid = L.base + L.lane * SS_NCELL;        // a [121] grid of this lane's own
    for (int k = 0; k < SS_NCELL; ++k) shared_grid[k] = p[k];
    K.prob = shared_grid; K.per_env_prob = 0;
    o[0] = (float)sample_cell(P, K, L.lane, u);
    SSP_WAVE_SYNC();
    for (int k = 0; k < SS_NCELL; ++k) L.base[k * kWave + L.lane] = p[k];      // [121][npad], npad = kWave: env = lane
    K.prob = L.base; K.per_env_prob = 1;
    o[1] = (float)sample_cell(P, K, L.lane, u);
#pragma unroll
    for (int i = 0; i < SS_GRID; ++i) { o[2 + i] = yaw_sample(i); o[2 + SS_GRID + i] = pitch_sample(i); }
    const float* s = p + SS_NCELL + 1;
    place_stone(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], o + 24);
    stone_normal(s[8], s[9], s[10], o + 27);
  } else if constexpr (OP == OP_WINDOW_PROB) {
#if !defined(__HIP_DEVICE_COMPILE__)
    window_prob(o, (int)p[0], p[1] != 0.f);
#endif
  } else if constexpr (OP == OP_OBS_TERMS) {
    quat_roll_pitch_cs(p, o[0], o[1], o[2], o[3]);
    target_features(p + 6, p[4], p[5], p + 9, p + 12, o + 4);
    o[9] = planar_dist(p + 9, p + 6);
    o[10] = clip5(p[14]);
    uint32_t r[6][4];
#pragma unroll
    for (int b = 0; b < 6; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i) r[b][i] = bits(p[15 + 2 * NJ + 4 * b + i]);
    static_for<0, NJ>([&](auto Jc) {      // instantiated as write_obs / env_reset do
      constexpr int j = decltype(Jc)::value;
      constexpr float mid = 0.5f * (Model::lo[j] + Model::hi[j]);
      constexpr float span = Model::hi[j] - Model::lo[j];
      constexpr float ps = (float)kPolicySign[j];
      o[11 + j] = obs_angle(ps, p[15 + j], mid, span);
      o[11 + NJ + j] = obs_rate(ps, p[15 + NJ + j]);
      o[11 + 2 * NJ + j] = reset_angle<Model, j>(r);
      o[11 + 3 * NJ + j] = reset_angle<ClampModel, j>(r);
    });
  } else if constexpr (OP == OP_SUBSTEP) {
    // the lane's state as step_env leaves it in LDS before its substeps (ss_kernels.hpp, steps 1 and 2 of step_env)
    const int side = L.lane & 1;
    const float m = side ? -1.f : 1.f;
    put_base(L, m, p, p + 3, p + 7, p + 10);
    float qin[NH], qdin[NH];
    static_for<0, NH>([&](auto Kc) {
      constexpr int k = decltype(Kc)::value, jr = kHalf[k], jl = left_twin(jr);
      const int gj = side ? jl : jr;
      qin[k] = p[13 + gj];
      qdin[k] = p[13 + NJ + gj];
      L.s(S_ACT + k) = action_lane_sign(jr, m) * p[13 + 2 * NJ + gj];
    });
    put_joints(L, m, qin, qdin);
    const float power = p[13 + 3 * NJ];
    const float* st = p + 14 + 3 * NJ;
#pragma unroll
    for (int sl = 0; sl < 3; ++sl) {
      L.s(S_STP + sl * 3 + 0) = st[sl * 8 + 0]; L.s(S_STP + sl * 3 + 1) = m * st[sl * 8 + 1]; L.s(S_STP + sl * 3 + 2) = st[sl * 8 + 2];
      L.s(S_STN + sl * 3 + 0) = st[sl * 8 + 3]; L.s(S_STN + sl * 3 + 1) = m * st[sl * 8 + 4]; L.s(S_STN + sl * 3 + 2) = st[sl * 8 + 5];
      L.q2(kLdsHead + sl) = make_float2(st[sl * 8 + 6], m * st[sl * 8 + 7]);
    }
    const float* wp = st + 24 + 13 * side;
    Warm wm;
    wm.key = (int)wp[0];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int d = 0; d < 3; ++d) wm.lam[k][d] = wp[1 + 3 * k + d];
    if constexpr (warm_in_lds(0)) {      // where the plain variant keeps it between the substeps
      L.s(S_WKEY) = __builtin_bit_cast(float, wm.key);
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int d = 0; d < 3; ++d) L.s(S_WLAM + 3 * k + d) = wm.lam[k][d];
    }
    const int calls = (int)st[24 + 26];
    FootReport fr = {};
#pragma unroll 1
    for (int c = 0; c < calls; ++c) substep<Model, 0>(power, fr, L, wm);
    if constexpr (warm_in_lds(0)) {
      wm.key = __builtin_bit_cast(int, L.s(S_WKEY));
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int d = 0; d < 3; ++d) wm.lam[k][d] = L.s(S_WLAM + 3 * k + d);
    }
#pragma unroll
    for (int k = 0; k < NH; ++k) { o[k] = L.s(S_Q + k); o[NH + k] = L.s(S_QD + k); }
    o += 2 * NH;
#pragma unroll
    for (int i = 0; i < 13; ++i) o[i] = L.s(S_POS + i);      // S_POS 3, S_QUAT 4, S_VW 3, S_VV 3 are consecutive
    static_assert(S_QUAT == S_POS + 3 && S_VW == S_QUAT + 4 && S_VV == S_VW + 3 && S_STP == S_VV + 3, "the base words are consecutive");
    o += 13;
    o[0] = (float)wm.key;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int d = 0; d < 3; ++d) o[1 + 3 * k + d] = wm.lam[k][d];
    o += 13;
    o[0] = (float)fr.contact; o[1] = (float)fr.on_target;
#pragma unroll
    for (int i = 0; i < 3; ++i) o[2 + i] = fr.sole[i];
  } else if constexpr (OP == OP_PK_HALF) {
    run_pk(p, o);
  } else if constexpr (OP == OP_LIMIT_FORMS) {
    run_limit<Model>(p, o);
  } else if constexpr (OP == OP_TAU_PAIR) {
    run_tau<Model>(p, o);
  } else if constexpr (OP == OP_STEP_SCORE) {
    const float pos[3] = {p[0], p[1], p[2]}, quat[4] = {p[3], p[4], p[5], p[6]};
    Cache c = {};
#pragma unroll
    for (int sl = 0; sl < 3; ++sl)
#pragma unroll
      for (int i = 0; i < 3; ++i) c.p[sl][i] = p[7 + 3 * sl + i];
    const float target_old[3] = {p[16], p[17], p[18]};
    const float sole[2][3] = {{p[19], p[20], p[21]}, {p[22], p[23], p[24]}};
    const StepScore sc = step_score(pos, quat, c, target_old, sole, p[25], (int)bits(p[26]), (int)bits(p[27]), (int)bits(p[28]),
                                    bits(p[29]) != 0u, p[30], p[31], p[32], (int)bits(p[33]));
    o[0] = sc.pot_prev; o[1] = unbits(sc.d ? 1u : 0u); o[2] = unbits((uint32_t)sc.bad);
    o[3] = sc.r; o[4] = sc.roll; o[5] = sc.pitch; o[6] = sc.cyaw; o[7] = sc.syaw;
  } else if constexpr (OP == OP_EP_RETURN) {
    float ep_ret = p[0], ep_lo = p[1];
#pragma unroll
    for (int i = 0; i < kEpR; ++i) {
      ep_return_add(ep_ret, ep_lo, p[2 + i]);
      o[2 * i] = ep_ret; o[2 * i + 1] = ep_lo;
    }
  } else if constexpr (OP == OP_STEP_LOGIC) {
    // the lane's LDS as step_env has it behind its substeps: base, joints, actions and heading items in the lane's own world
    const int side = L.lane & 1;
    const float m = side ? -1.f : 1.f;
    put_base(L, m, p, p + 3, p + 7, p + 10);
    float qin[NH], qdin[NH], ain[NH];
    static_for<0, NH>([&](auto Kc) {
      constexpr int k = decltype(Kc)::value, jr = kHalf[k], jl = left_twin(jr);
      const int gj = side ? jl : jr;
      qin[k] = p[13 + gj];
      qdin[k] = p[13 + NJ + gj];
    });
    load_actions(p + 13 + 2 * NJ, side, ain);
    put_joints(L, m, qin, qdin);
    put_actions(L, m, ain);
    const float* f = p + 13 + 3 * NJ + 5 * side;
    FootReport fr;
    fr.contact = (int)bits(f[0]); fr.on_target = (int)bits(f[1]);
#pragma unroll
    for (int i = 0; i < 3; ++i) fr.sole[i] = f[2 + i];
    const float* cp = p + 13 + 3 * NJ + 10;
    Cache c;
#pragma unroll
    for (int sl = 0; sl < 3; ++sl) {
#pragma unroll
      for (int i = 0; i < 3; ++i) { c.p[sl][i] = cp[3 * sl + i]; c.nrm[sl][i] = cp[9 + 3 * sl + i]; }
      c.tilt[sl][0] = cp[18 + 2 * sl]; c.tilt[sl][1] = cp[19 + 2 * sl];
      L.q2(kLdsHead + sl) = make_float2(cp[24 + 2 * sl], m * cp[25 + 2 * sl]);      // as put_stones places a heading
    }
    const float* w = cp + 30;
    float pot_prev = w[0], nn_dr = w[1], ep_ret = w[2], ep_lo = w[3];
    int n = (int)bits(w[4]), count = (int)bits(w[5]), elapsed = (int)bits(w[6]);
    uint32_t ctr = bits(w[7]);
    const float* stub = w + 8;
    const bool store = side == 0;                // the lane that writes the table, as in step_env
    uint32_t calls = 0u, rec_k = 0u, rec_ctr = 0u, rec_store = 0u;
    StepEnd se;
    step_logic<Model>(L, side, m, fr, c, pot_prev, nn_dr, ep_ret, ep_lo, n, count, elapsed, ctr, store,
                      [&](uint32_t& ct, int k, float* sp, float* nrm, float* tilt, float* h, bool st) {
                        calls += 1u; rec_k = (uint32_t)k; rec_ctr = ct; rec_store = st ? 1u : 0u;
                        ct += 1u;                // a draw uses one Philox block
#pragma unroll
                        for (int i = 0; i < 3; ++i) { sp[i] = stub[i]; nrm[i] = stub[3 + i]; }
                        tilt[0] = stub[6]; tilt[1] = stub[7];
                        h[0] = stub[8]; h[1] = stub[9];
                        return stub[10];
                      }, se);
#pragma unroll
    for (int i = 0; i < 3; ++i) { o[i] = se.pos[i]; o[7 + i] = se.v0.w[i]; o[10 + i] = se.v0.v[i]; }
#pragma unroll
    for (int i = 0; i < 4; ++i) o[3 + i] = se.quat[i];
    o[13] = unbits((uint32_t)se.flags); o[14] = unbits((uint32_t)se.advanced);
#pragma unroll
    for (int sl = 0; sl < 3; ++sl) { o[15 + 2 * sl] = se.hd[sl][0]; o[16 + 2 * sl] = se.hd[sl][1]; }
    o[21] = unbits(se.d ? 1u : 0u); o[22] = unbits((uint32_t)se.bad);
    o[23] = se.r; o[24] = se.roll; o[25] = se.pitch; o[26] = se.cyaw; o[27] = se.syaw;
    o += 28;
    o[0] = pot_prev; o[1] = nn_dr; o[2] = ep_ret; o[3] = ep_lo;
    o[4] = unbits((uint32_t)n); o[5] = unbits((uint32_t)count); o[6] = unbits((uint32_t)elapsed); o[7] = unbits(ctr);
    o += 8;
#pragma unroll
    for (int sl = 0; sl < 3; ++sl) {
#pragma unroll
      for (int i = 0; i < 3; ++i) { o[3 * sl + i] = c.p[sl][i]; o[9 + 3 * sl + i] = c.nrm[sl][i]; }
      o[18 + 2 * sl] = c.tilt[sl][0]; o[19 + 2 * sl] = c.tilt[sl][1];
      const float2 hl = L.q2(kLdsHead + sl);
      o[24 + 2 * sl] = hl.x; o[25 + 2 * sl] = hl.y;
    }
    o += 30;
    o[0] = unbits(calls); o[1] = unbits(rec_k); o[2] = unbits(rec_ctr); o[3] = unbits(rec_store);
  }
}

#if !defined(SS_PROBE_HOST)
// one wavefront per workgroup, one case per lane (`substep`, `step_logic`: per lane pair; a lane's share of the output row is OW words).  Lanes past
// the last case redo case n - 1 (every lane stays active and reads inside the buffer; a lane keeps its side, so a pair stays a pair); only
// lanes of a case below n store.
template <class Model, int OP>
__global__ __launch_bounds__(kWave) void probe_kernel(int n, const float* __restrict__ in, float* __restrict__ out) {
  constexpr int LPC = lanes_per_case(OP), IW = in_w(OP), OW = out_w(OP) / LPC;
  const int idx = blockIdx.x * kWave + threadIdx.x;
  const int cas = idx / LPC;
  const int src = cas < n ? cas : n - 1;
  float o[OW];
  // a lane pair's op reads its row where it lies: 128 words held in registers across the call would only spill
  float rowbuf[LPC == 1 ? IW : 1];
  const float* row = in + (size_t)src * IW;
  if constexpr (LPC == 1) {
#pragma unroll
    for (int i = 0; i < IW; ++i) rowbuf[i] = in[(size_t)src * IW + i];
    row = rowbuf;
  }
#pragma unroll
  for (int i = 0; i < OW; ++i) o[i] = 0.f;
  Lds L = {nullptr, (int)threadIdx.x};
  if constexpr (needs_lds(OP)) {
    __shared__ float4 lds[kLdsSlots * kWave];
    L.base = reinterpret_cast<float*>(lds);
  }
  run_case<Model, OP>(row, o, L);
  if (cas < n) {
#pragma unroll
    for (int i = 0; i < OW; ++i) out[(size_t)idx * OW + i] = o[i];
  }
}
#endif

template <class Model>
int run(int op, int n, const float* in, float* out, void* stream) {
  int rc = SSP_BAD_OP;
  static_for<0, OP_COUNT>([&](auto Oc) {
    constexpr int OP = decltype(Oc)::value;
    if (op != OP) return;
    if (n == 0) { rc = in_w(OP) * 1000 + out_w(OP); return; }
#if defined(SS_PROBE_HOST)
    (void)stream;
    if (OP == OP_XCHG) { rc = SSP_UNSUPPORTED; return; }
    std::vector<float> lds(needs_lds(OP) ? (size_t)kLdsSlots * kWave * 4 : 0);
    const Lds L = {lds.data(), 0};
    for (int e = 0; e < n; ++e) {
      float o[out_w(OP)];
      for (int i = 0; i < out_w(OP); ++i) o[i] = 0.f;
      for (float& x : lds) x = std::numeric_limits<float>::quiet_NaN();
      if constexpr (lanes_per_case(OP) == 2) {      // lanes 0 and 1 of the block, two threads that meet at every exchange
        PairSync sync;
        auto lane = [&](int side) {
          t_sync = &sync;
          t_side = side;
          run_case<Model, OP>(in + (size_t)e * in_w(OP), o + side * (out_w(OP) / 2), Lds{lds.data(), side});
          t_sync = nullptr;
          sync.gone.store(1, std::memory_order_release);
        };
        std::thread partner(lane, 1);
        lane(0);
        partner.join();
      } else {
        run_case<Model, OP>(in + (size_t)e * in_w(OP), o, L);
      }
      for (int i = 0; i < out_w(OP); ++i) out[(size_t)e * out_w(OP) + i] = o[i];
    }
    rc = 0;
#else
    if constexpr (OP == OP_WINDOW_PROB) {      // host code of the product: there is nothing to launch
      rc = SSP_UNSUPPORTED;
    } else {
      (void)hipGetLastError();      // what this call returns speaks of this launch alone
      probe_kernel<Model, OP><<<dim3((n * lanes_per_case(OP) + kWave - 1) / kWave), dim3(kWave), 0, (hipStream_t)stream>>>(n, in, out);
      rc = -(int)hipGetLastError();
    }
#endif
  });
  return rc;
}
}  // namespace ssp

// ---- the policy MLP of the closed-loop look-ahead (ss_policy.hpp), on its own
//   int ssp_mlp(const ss_policy_desc* desc, const float* packed, int n, const float* x, float* out, uint32_t prefill_bits, void* stream)
//     packed: the packed form of desc (ss_policy_words words); x [n][60]; out [(n + 31) / 32][2][256][32]: per group of 32 rows both
//     activation blocks whole, k-major, as they stand behind one MLP phase.  Every word of the blocks (and, on the device, of the staged
//     rows) holds prefill_bits before the phase; rows past n are staged as the prefill.  What a dump shows: the last layer's tile (32
//     columns, 21 of them the action) in block (layers - 1) & 1, the layer before it in the other block, what earlier layers left
//     behind those, and the prefill wherever the net wrote nothing.
//     device: one workgroup of kWaves wavefronts per 32 rows over policy::kLdsWords of LDS, as lookahead_policy_kernel has them; every
//     wavefront calls mlp_phase once.  host: eval_row per row on the same words; its y, t0, t1 laid out the same way (rows past n keep
//     the prefill).  Returns 0, SSP_BAD_OP for a description that is not valid, or the negative HIP error of the launch.
#if !defined(SS_PROBE_HOST)
__global__ __launch_bounds__(ss::kWave * ss::policy::kWaves, 1) void ssp_mlp_kernel(ss::policy::Net net, const float* __restrict__ packed, int n,
                                                                                    const float* __restrict__ x, float* __restrict__ out,
                                                                                    uint32_t prefill_bits) {
  using namespace ss;
  constexpr int kThreads = kWave * policy::kWaves, kStaged = kEnvsPerWave * SS_OBS_DIM;
  __shared__ float4 lds4[policy::kLdsWords / 4];
  float* lds = reinterpret_cast<float*>(lds4);
  float* xb = lds + kLdsSlots * kWave * 4;
  const int tid = (int)threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & (kWave - 1);
  const float fill = ssp::unbits(prefill_bits);
  const int row0 = (int)blockIdx.x * kEnvsPerWave;
  // the staged rows where look_row puts them: row r of the group at lds + r * 60
  for (int i = tid; i < kStaged; i += kThreads) {
    const int row = row0 + i / SS_OBS_DIM;
    lds[i] = row < n ? x[(size_t)row0 * SS_OBS_DIM + i] : fill;
  }
  for (int i = tid; i < policy::kXWords; i += kThreads) xb[i] = fill;
#if defined(__HIP_DEVICE_COMPILE__)      // (mlp_phase exists in the device pass only)
  policy::mlp_phase(net, packed, lds, xb, wave, lane);      // its first barrier stands behind the fills, its last before the dump
#else
  (void)wave; (void)lane;
#endif
  float* o = out + (size_t)blockIdx.x * policy::kXWords;
  for (int i = tid; i < policy::kXWords; i += kThreads) o[i] = xb[i];
}
#endif

extern "C" int ssp_mlp(const ss_policy_desc* desc, const float* packed, int n, const float* x, float* out, uint32_t prefill_bits,
                       void* stream) {
  using namespace ss;
  policy::Net net;
  if (!policy::make_net(desc, net) || n < 0 || (n > 0 && (!packed || !x || !out))) return ssp::SSP_BAD_OP;
  if (n == 0) return 0;
  const int groups = (n + kEnvsPerWave - 1) / kEnvsPerWave;
#if defined(SS_PROBE_HOST)
  (void)stream;
  const float fill = ssp::unbits(prefill_bits);
  for (size_t i = 0; i < (size_t)groups * policy::kXWords; ++i) out[i] = fill;
  for (int row = 0; row < n; ++row) {
    float y[32], t[2][SS_POLICY_MAX_WIDTH];
    for (int i = 0; i < 32; ++i) y[i] = fill;
    for (int b = 0; b < 2; ++b)
      for (int i = 0; i < SS_POLICY_MAX_WIDTH; ++i) t[b][i] = fill;
    policy::eval_row(net, packed, x + (size_t)row * SS_OBS_DIM, y, t[0], t[1]);
    float* o = out + (size_t)(row / kEnvsPerWave) * policy::kXWords + row % kEnvsPerWave;
    for (int b = 0; b < 2; ++b)
      for (int i = 0; i < SS_POLICY_MAX_WIDTH; ++i) o[b * policy::kBufWords + i * kEnvsPerWave] = t[b][i];
    for (int i = 0; i < 32; ++i) o[((net.layers - 1) & 1) * policy::kBufWords + i * kEnvsPerWave] = y[i];      // the tile stands over its block
  }
  return 0;
#else
  (void)hipGetLastError();
  ssp_mlp_kernel<<<dim3(groups), dim3(kWave * policy::kWaves), 0, (hipStream_t)stream>>>(net, packed, n, x, out, prefill_bits);
  return -(int)hipGetLastError();
#endif
}

#if defined(SS_PROBE_HOST)
// the C library's fmaf on n triples (the yardstick of tests/np_policy.py's emulation)
extern "C" void ssp_fmaf(int n, const float* a, const float* b, const float* c, float* out) {
  for (int i = 0; i < n; ++i) out[i] = fmaf(a[i], b[i], c[i]);
}
#endif

extern "C" int ssp_run(int op, int kind, int n, const float* in, float* out, void* stream) {
  if (n < 0 || (n > 0 && (!in || !out))) return ssp::SSP_BAD_OP;
  if (kind == 0) return ssp::run<ss::ModelWalker3D>(op, n, in, out, stream);
  if (kind == 1) return ssp::run<ss::ModelMike>(op, n, in, out, stream);
  return ssp::SSP_BAD_KIND;
}
