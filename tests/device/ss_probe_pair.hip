// ss_probe_pair.hip -- the {leg, arm} pair form of the three-helper step kernels beside the scalar code it replaces, one case per lane:
// the joint torque / implicit diagonal of a pair of joints (joint_tau's pair overload of ss_dynamics.hpp) beside joint_tau per joint.
// tests/test_pair_response.py requires the two sides to agree bitwise.
// TEST INFRASTRUCTURE ONLY: never part of libsteppingstone.so, nothing in the package loads it.
//
// Compiled two ways, like ss_probe_pk.hip: for gfx950 by steppingstone_amd/build.py: build_probe_pair() with the product's flags
// (steppingstone_amd/lib/libss_probe_pair.so; device pointers and a stream), and for the CPU by tests/probe_pair_lib.py
// (-DSS_PROBE_HOST, hipcc --cuda-host-only; host pointers, a loop over the cases).
//
//   int sspr_run(int op, int kind, int n, const float* in, float* out, void* stream)
//     in [n][IN_W(op)], out [n][OUT_W(op)], row-major; kind 0 = ModelWalker3D, 1 = ModelMike.  n == 0 reads and writes nothing and
//     returns IN_W * 1000 + OUT_W.  Returns 0, a negative SSPR_*, or the HIP error of the launch.
//   OP_TAU: in power, act (leg halves), act (arm halves), then (q, qd) per joint 0..20 -> out per pair (3,13) (4,14) (5,15) (6,16) 8 floats:
//     tau leg, tau arm, Dadd leg, Dadd arm of the pair overload, then of joint_tau per joint.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../steppingstone_amd/csrc/ss_kernels.hpp"

#if !defined(__HIP_DEVICE_COMPILE__)
float ss_host_xchg(float x) { return x; }
void ss_host_wave_sync() {}
#endif

namespace sspr {
using namespace ss;

enum { OP_TAU = 0, OP_COUNT };
enum { SSPR_BAD_OP = -1, SSPR_BAD_KIND = -3 };
constexpr int kInW[OP_COUNT] = {3 + 2 * NJ};
constexpr int kOutW[OP_COUNT] = {32};

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
SSD void run_case(const float* in, float* out) {
  static_assert(OP == OP_TAU, "one op");
  run_tau<Model>(in, out);
}

#if !defined(SS_PROBE_HOST)
template <class Model, int OP>
__global__ __launch_bounds__(kWave) void probe_pair_kernel(int n, const float* __restrict__ in, float* __restrict__ out) {
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
  probe_pair_kernel<Model, OP><<<dim3((n + kWave - 1) / kWave), dim3(kWave), 0, (hipStream_t)stream>>>(n, in, out);
  return -(int)hipGetLastError();
#endif
}

template <class Model>
int run_model(int op, int n, const float* in, float* out, void* stream) {
  (void)op;
  return run_op<Model, OP_TAU>(n, in, out, stream);
}

}  // namespace sspr

extern "C" int sspr_run(int op, int kind, int n, const float* in, float* out, void* stream) {
  using namespace sspr;
  if (op < 0 || op >= OP_COUNT) return SSPR_BAD_OP;
  if (n == 0) return kInW[op] * 1000 + kOutW[op];
  if (kind == 0) return run_model<ss::ModelWalker3D>(op, n, in, out, stream);
  if (kind == 1) return run_model<ss::ModelMike>(op, n, in, out, stream);
  return SSPR_BAD_KIND;
}
