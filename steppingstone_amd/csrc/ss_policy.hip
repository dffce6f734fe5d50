// ss_policy.hip -- the closed-loop look-ahead kernel and the repack of a policy's weights (docs/PHYSICS.md 14).  Both only
// READ the environment state; ss_api.hip validates the arguments and calls the launchers below.  The per-lane code is look_row
// (ss_lookahead.hpp) with the action source of ss_policy.hpp.
#include <hip/hip_runtime.h>

#include "ss_policy.hpp"

namespace ss {
namespace policy {

// A workgroup of kWaves wavefronts around the look-ahead's 32 rows: wavefront 0 is the look-ahead kernel's one wavefront (two lanes per
// row, the Lds block), the others join it in the MLP phase between the control steps and wait at its first barrier meanwhile.  Behind the
// Lds block stand the two activation blocks: 106,496 B, one workgroup per CU.
template <class Model, bool ROWS>
__global__ __launch_bounds__(kWave * kWaves, 1) void lookahead_policy_kernel(Params P, const int32_t* env_ids, int m, const float* states,
                                                                              int horizon, Net net, const float* packed,
                                                                              const float* offset, float* act, look::Out out) {
  __shared__ float4 lds4[kLdsWords / 4];
  float* lds = reinterpret_cast<float*>(lds4);
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & (kWave - 1);
  const ActPolicy src{net, packed, offset, act, lds + kLdsSlots * kWave * 4, wave};
  if (wave == 0) {
    look::look_row<Model, ROWS, ActPolicy>(P, env_ids, m, horizon, nullptr, out, blockIdx.x * kWave + lane, lane, lds, states, src);
  } else {
#pragma unroll 1
    for (int s = 0; s < horizon; ++s) src.phase(lds, lane);
  }
}

__global__ __launch_bounds__(256) void pack_kernel(Net net, Arrays A, float* packed) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < net.words) packed[i] = packed_word(net, A, i);
}

}  // namespace policy

// launchers called by ss_api.hip (arguments validated there)
hipError_t launch_policy_pack(const ss_policy_desc* d, const float* const* weight, const float* const* bias, float* packed, hipStream_t st) {
  policy::Net net;
  if (!policy::make_net(d, net)) return hipErrorInvalidValue;
  policy::Arrays A;
  for (int l = 0; l < SS_POLICY_MAX_LAYERS; ++l) {
    A.weight[l] = l < net.layers ? weight[l] : nullptr;
    A.bias[l] = l < net.layers ? bias[l] : nullptr;
  }
  hipLaunchKernelGGL(policy::pack_kernel, dim3((net.words + 255) / 256), dim3(256), 0, st, net, A, packed);
  return hipGetLastError();
}

template <class Model>
static void launch_policy_model(const Params& P, const int32_t* env_ids, int m, const float* states, int horizon, const policy::Net& net,
                                const float* packed, const float* offset, float* act, const look::Out& out, hipStream_t st) {
  using namespace policy;
  const dim3 grid((m + kEnvsPerWave - 1) / kEnvsPerWave), block(kWave * kWaves);
  if (states)
    hipLaunchKernelGGL((lookahead_policy_kernel<Model, true>), grid, block, 0, st, P, env_ids, m, states, horizon, net, packed, offset, act, out);
  else
    hipLaunchKernelGGL((lookahead_policy_kernel<Model, false>), grid, block, 0, st, P, env_ids, m, states, horizon, net, packed, offset, act, out);
}

hipError_t launch_lookahead_policy(const Params& P, int kind, const int32_t* env_ids, int m, const float* states, int horizon,
                                   const ss_policy_desc* d, const float* packed, const float* offset, float* act, float* obs, float* rew,
                                   uint8_t* done, float* final_state, float* work, hipStream_t st) {
  policy::Net net;
  if (!policy::make_net(d, net)) return hipErrorInvalidValue;
  const look::Out out{obs, rew, done, final_state, work};
  if (kind == SS_WALKER3D) launch_policy_model<ModelWalker3D>(P, env_ids, m, states, horizon, net, packed, offset, act, out, st);
  else launch_policy_model<ModelMike>(P, env_ids, m, states, horizon, net, packed, offset, act, out, st);
  return hipGetLastError();
}

}  // namespace ss

extern "C" int64_t ss_policy_words(const ss_policy_desc* d) {
  ss::policy::Net net;
  return ss::policy::make_net(d, net) ? (int64_t)net.words : -1;
}
