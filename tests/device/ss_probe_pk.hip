// ss_probe_pk.hip -- two small probes of forms the step kernels use in place of older ones, one case per lane:
//   * the half-broadcast packed multiply-add / multiply of ss_pair.hpp (pk_fma_half, pk_mul_half) beside two scalar fmaf / products;
//   * the joint-limit and joint-torque forms of ss_dynamics.hpp (joint_limit, joint_tau) beside the forms they replaced, which are
//     kept here VERBATIM as the reference.
// tests/test_pair_broadcast.py and tests/test_limit_forms.py require the two sides to agree bitwise.
// TEST INFRASTRUCTURE ONLY: never part of libsteppingstone.so, nothing in the package loads it.
//
// Compiled two ways, like ss_probe.hip: for gfx950 by steppingstone_amd/build.py: build_probe_pk() with the product's flags
// (steppingstone_amd/lib/libss_probe_pk.so; device pointers and a stream), and for the CPU by tests/probe_pk_lib.py
// (-DSS_PROBE_HOST, hipcc --cuda-host-only; host pointers, a loop over the cases).
//
//   int sspk_run(int op, int kind, int n, const float* in, float* out, void* stream)
//     in [n][IN_W(op)], out [n][OUT_W(op)], row-major; kind 0 = ModelWalker3D, 1 = ModelMike.  n == 0 reads and writes nothing and
//     returns IN_W * 1000 + OUT_W.  Returns 0, a negative SSPK_*, or the HIP error of the launch.
//   OP_PK (kind ignored): in a.x a.y s.x s.y c.x c.y -> out 32 floats, the form under test then its scalar reference, 2 floats each:
//     fma<0>(a,s,c) fma<1>(a,s,c) fma<0>(a,a,c) fma<1>(a,a,c) mul<0>(a,s) mul<1>(a,s) mul<0>(a,a) mul<1>(a,a) | the same eight by
//     fmaf(a.x, f, c.x), fmaf(a.y, f, c.y) / a.x * f, a.y * f with f the chosen half.  (a, a): one register as pair and as factor.
//   OP_LIMIT: in power, act, then (q, qd) per joint 0..20 -> out per joint 10 floats: viol kl dl tau Dadd of the kernels' forms, then
//     of the replaced ones.
#include <hip/hip_runtime.h>

#include <cstdint>

#include <vector>

#include "../../steppingstone_amd/csrc/ss_kernels.hpp"

#if !defined(__HIP_DEVICE_COMPILE__)
float ss_host_xchg(float x) { return x; }
void ss_host_wave_sync() {}
#endif

namespace sspk {
using namespace ss;

enum { OP_PK = 0, OP_LIMIT = 1, OP_COUNT };
enum { SSPK_BAD_OP = -1, SSPK_BAD_KIND = -3 };
constexpr int kInW[OP_COUNT] = {6, 2 + 2 * NJ};
constexpr int kOutW[OP_COUNT] = {32, 10 * NJ};

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

// the joint-limit and joint-torque forms as the step kernels had them before joint_limit (ss_dynamics.hpp): the reference
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

template <class Model, int OP>
SSD void run_case(const float* in, float* out) {
  if constexpr (OP == OP_PK) run_pk(in, out);
  else run_limit<Model>(in, out);
}

#if !defined(SS_PROBE_HOST)
template <class Model, int OP>
__global__ __launch_bounds__(kWave) void probe_pk_kernel(int n, const float* __restrict__ in, float* __restrict__ out) {
  const int i = blockIdx.x * kWave + threadIdx.x;
  if (i >= n) return;                  // no lane exchange in these ops: an idle lane may leave
  float a[kInW[OP]], o[kOutW[OP]];
#pragma unroll
  for (int k = 0; k < kInW[OP]; ++k) a[k] = in[(size_t)i * kInW[OP] + k];
  run_case<Model, OP>(a, o);
#pragma unroll
  for (int k = 0; k < kOutW[OP]; ++k) out[(size_t)i * kOutW[OP] + k] = o[k];
}
#endif

template <class Model, int OP>
int run_op(int n, const float* in, float* out, void* stream) {
#if defined(SS_PROBE_HOST)
  (void)stream;
  for (int i = 0; i < n; ++i) run_case<Model, OP>(in + (size_t)i * kInW[OP], out + (size_t)i * kOutW[OP]);
  return 0;
#else
  probe_pk_kernel<Model, OP><<<dim3((n + kWave - 1) / kWave), dim3(kWave), 0, (hipStream_t)stream>>>(n, in, out);
  return -(int)hipGetLastError();
#endif
}

template <class Model>
int run_model(int op, int n, const float* in, float* out, void* stream) {
  if (op == OP_PK) return run_op<Model, OP_PK>(n, in, out, stream);
  return run_op<Model, OP_LIMIT>(n, in, out, stream);
}

}  // namespace sspk

extern "C" int sspk_run(int op, int kind, int n, const float* in, float* out, void* stream) {
  using namespace sspk;
  if (op < 0 || op >= OP_COUNT) return SSPK_BAD_OP;
  if (n == 0) return kInW[op] * 1000 + kOutW[op];
  if (kind == 0) return run_model<ss::ModelWalker3D>(op, n, in, out, stream);
  if (kind == 1) return run_model<ss::ModelMike>(op, n, in, out, stream);
  return SSPK_BAD_KIND;
}
