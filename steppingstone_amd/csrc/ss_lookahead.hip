// ss_lookahead.hip -- the look-ahead kernel (docs/PHYSICS.md "Look-ahead"): H control steps of ss_step on private copies
// of selected envs under given action sequences, one branch per row.  It only READS the environment state; ss_api.hip validates the
// arguments and calls the launcher below.  The per-lane code is ss_lookahead.hpp.
#include <hip/hip_runtime.h>

#include "ss_lookahead.hpp"

namespace ss {
namespace look {

// The plain step kernel's shape: one wavefront per workgroup, 32 rows, two lanes per row, one Lds block (40,960 B: four workgroups per CU).
template <class Model>
__global__ __launch_bounds__(kWave, 1) void lookahead_kernel(Params P, const int32_t* env_ids, int m, int horizon, const float* act, Out out) {
  __shared__ float4 lds4[kLdsSlots * kWave];
  look_row<Model>(P, env_ids, m, horizon, act, out, blockIdx.x * kWave + threadIdx.x, threadIdx.x, reinterpret_cast<float*>(lds4));
}

// The same kernel with the prologue sourced from states[k, :] (ss_lookahead_states): a second instantiation of look_row, same shape
template <class Model>
__global__ __launch_bounds__(kWave, 1) void lookahead_states_kernel(Params P, const int32_t* env_ids, int m, const float* states, int horizon,
                                                                    const float* act, Out out) {
  __shared__ float4 lds4[kLdsSlots * kWave];
  look_row<Model, true>(P, env_ids, m, horizon, act, out, blockIdx.x * kWave + threadIdx.x, threadIdx.x, reinterpret_cast<float*>(lds4),
                        states);
}

// The observation of state rows (ss_get_obs_states): obs_kernel's shape, one lane per row
template <class Model>
__global__ __launch_bounds__(kWave) void obs_states_kernel(int m, const float* states, float* obs) {
  const int k = blockIdx.x * kWave + threadIdx.x;
  if (k >= m) return;
  float o[SS_OBS_DIM];
  obs_from_row<Model>(states + (size_t)k * SS_STATE_DIM, o);
#pragma unroll
  for (int i = 0; i < SS_OBS_DIM; ++i) obs[(size_t)k * SS_OBS_DIM + i] = o[i];
}

}  // namespace look

// launcher called by ss_api.hip (arguments validated there; m >= 1, 1 <= horizon <= SS_LOOK_MAX_STEPS)
hipError_t launch_lookahead(const Params& P, int kind, const int32_t* env_ids, int m, int horizon, const float* act, float* obs, float* rew,
                            uint8_t* done, float* final_state, float* work, hipStream_t st) {
  using namespace look;
  const dim3 grid((m + kEnvsPerWave - 1) / kEnvsPerWave);
  const Out out{obs, rew, done, final_state, work};
  if (kind == SS_WALKER3D)
    hipLaunchKernelGGL((lookahead_kernel<ModelWalker3D>), grid, dim3(kWave), 0, st, P, env_ids, m, horizon, act, out);
  else
    hipLaunchKernelGGL((lookahead_kernel<ModelMike>), grid, dim3(kWave), 0, st, P, env_ids, m, horizon, act, out);
  return hipGetLastError();
}

// launchers of ss_lookahead_states and ss_get_obs_states (arguments validated in ss_api.hip; m >= 1)
hipError_t launch_lookahead_states(const Params& P, int kind, const int32_t* env_ids, int m, const float* states, int horizon,
                                   const float* act, float* obs, float* rew, uint8_t* done, float* final_state, float* work, hipStream_t st) {
  using namespace look;
  const dim3 grid((m + kEnvsPerWave - 1) / kEnvsPerWave);
  const Out out{obs, rew, done, final_state, work};
  if (kind == SS_WALKER3D)
    hipLaunchKernelGGL((lookahead_states_kernel<ModelWalker3D>), grid, dim3(kWave), 0, st, P, env_ids, m, states, horizon, act, out);
  else
    hipLaunchKernelGGL((lookahead_states_kernel<ModelMike>), grid, dim3(kWave), 0, st, P, env_ids, m, states, horizon, act, out);
  return hipGetLastError();
}

hipError_t launch_obs_states(int kind, int m, const float* states, float* obs, hipStream_t st) {
  using namespace look;
  const dim3 grid((m + kWave - 1) / kWave);
  if (kind == SS_WALKER3D)
    hipLaunchKernelGGL((obs_states_kernel<ModelWalker3D>), grid, dim3(kWave), 0, st, m, states, obs);
  else
    hipLaunchKernelGGL((obs_states_kernel<ModelMike>), grid, dim3(kWave), 0, st, m, states, obs);
  return hipGetLastError();
}

}  // namespace ss
