// ss_kinematics.hip -- the kinematic readout kernel (docs/PHYSICS.md "Kinematic readout"): world twist of every body,
// centre of mass / momentum / energy, and the sole corners with their height over the target stone and their carrier, for selected envs.
// It only READS the environment state; ss_api.hip validates the arguments and calls the launcher below.
#include <hip/hip_runtime.h>

#include "ss_kinematics.hpp"

namespace ss {
namespace kin {

constexpr int kEnvsPerBlock = 8;
constexpr int kThreads = kEnvsPerBlock * kHalfLanes;
static_assert(2 * kEnvsPerBlock <= kWave, "one lane-private LDS column per (env, foot)");

// half_sum of ss_kinematics.hpp, one term per lane of the env's 32-lane half
__device__ __forceinline__ float lane_sum(float x) {
#pragma unroll
  for (int off = kHalfLanes / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, kHalfLanes);
  return x;
}

// One 32-lane half of a wavefront = one requested row k (env env_ids[k]).  Lanes 0..21: pose and twist of body b along its own ancestor
// chain (no lane waits for another), then the two rounds of sums; lanes 22 / 23: the contact detection of the right / left foot on a
// lane-private column of the LDS block (the layout of the step kernels' Lds view, which fk_detect reads); the foot lanes 8 / 13 fetch
// the result and write their four corner rows.  A row outside [0, m) or an env id outside [0, N) reads and writes nothing.  What is
// computed does not depend on which outputs are requested: only the stores do.
template <class Model>
__global__ __launch_bounds__(kThreads) void kinematics_kernel(Params P, const int32_t* env_ids, int m, float* body_twist, float* summary,
                                                               float* corners) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsSlots * kWave * 4];
  const int half = threadIdx.x / kHalfLanes, b = threadIdx.x % kHalfLanes;
  const int k = blockIdx.x * kEnvsPerBlock + half;
  int e = -1;
  if (k < m) e = env_ids ? env_ids[k] : k;
  const bool valid = e >= 0 && e < P.n;
  const bool body = valid && b < kBodies;

  BodyKin kb;
  float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  uint32_t code = 0;
  if (body) {
    body_kin<Model>(P, e, b, kb);
    body_moments<Model>(b, kb, s, s + 3);
  } else if (valid && b < kDetectLane + 2) {
    const int foot = b - kDetectLane;
    code = foot_carriers<Model>(P, e, foot, Lds{lds, 2 * half + foot});
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) s[i] = lane_sum(s[i]);
  float com[3];
  com_of<Model>(s, com);
  float L[3] = {0.f, 0.f, 0.f}, T = 0.f;
  if (body) body_momentum<Model>(b, kb, com, L, T);
#pragma unroll
  for (int i = 0; i < 3; ++i) L[i] = lane_sum(L[i]);
  T = lane_sum(T);
  const int foot = b == LFOOT ? 1 : 0;
  const uint32_t carried = __shfl(code, kDetectLane + foot, kHalfLanes);

  if (!body) return;
  if (body_twist) {
    float2* dst = reinterpret_cast<float2*>(body_twist + ((size_t)k * kBodies + b) * 6);
    dst[0] = make_float2(kb.w[0], kb.w[1]);
    dst[1] = make_float2(kb.w[2], kb.v[0]);
    dst[2] = make_float2(kb.v[1], kb.v[2]);
  }
  if (summary && b == 0) {
    float o[SS_KIN_SUMMARY];
    summary_row<Model>(s, s + 3, L, T, o);
    float4* dst = reinterpret_cast<float4*>(summary + (size_t)k * SS_KIN_SUMMARY);
    dst[0] = make_float4(o[0], o[1], o[2], o[3]);
    dst[1] = make_float4(o[4], o[5], o[6], o[7]);
    dst[2] = make_float4(o[8], o[9], o[10], o[11]);
  }
  if (corners && (b == RFOOT || b == LFOOT)) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float o[7];
      corner_row<Model>(P, e, foot, c, kb, o);
      float4* dst = reinterpret_cast<float4*>(corners + ((size_t)k * SS_KIN_CORNER + 4 * foot + c) * 8);
      dst[0] = make_float4(o[0], o[1], o[2], o[3]);
      dst[1] = make_float4(o[4], o[5], o[6], carrier_value(carried, c));
    }
  }
}

}  // namespace kin

// launcher called by ss_api.hip (arguments validated there; m >= 1)
hipError_t launch_kinematics(const Params& P, int kind, const int32_t* env_ids, int m, float* body_twist, float* summary, float* corners,
                             hipStream_t st) {
  using namespace kin;
  const dim3 grid((m + kEnvsPerBlock - 1) / kEnvsPerBlock);
  if (kind == SS_WALKER3D)
    hipLaunchKernelGGL((kinematics_kernel<ModelWalker3D>), grid, dim3(kThreads), 0, st, P, env_ids, m, body_twist, summary, corners);
  else
    hipLaunchKernelGGL((kinematics_kernel<ModelMike>), grid, dim3(kThreads), 0, st, P, env_ids, m, body_twist, summary, corners);
  return hipGetLastError();
}

}  // namespace ss
