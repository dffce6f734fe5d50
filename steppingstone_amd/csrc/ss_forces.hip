// ss_forces.hip -- the force readout kernel (docs/PHYSICS.md "Force readout"): contact forces per sole corner and
// substep, joint torques, and the state a control step would end in, for selected envs under given actions.  It only READS the
// environment state; ss_api.hip validates the arguments and calls the launcher below.  The per-lane code is ss_forces.hpp.
#include <hip/hip_runtime.h>

#include "ss_forces.hpp"

namespace ss {
namespace frc {

// The plain step kernel's shape: one wavefront per workgroup, 32 requested rows, two lanes per row, one Lds block.
template <class Model>
__global__ __launch_bounds__(kWave, 1) void step_forces_kernel(Params P, const int32_t* env_ids, int m, const float* act, Out out) {
  __shared__ float4 lds4[kLdsSlots * kWave];
  forces_row<Model>(P, env_ids, m, act, out, blockIdx.x * kWave + threadIdx.x, threadIdx.x, reinterpret_cast<float*>(lds4));
}

}  // namespace frc

// launcher called by ss_api.hip (arguments validated there; m >= 1)
hipError_t launch_step_forces(const Params& P, int kind, const int32_t* env_ids, int m, const float* act, float* contacts, float* joints,
                              float* next_state, hipStream_t st) {
  using namespace frc;
  const dim3 grid((m + kEnvsPerWave - 1) / kEnvsPerWave);
  const Out out{contacts, joints, next_state};
  if (kind == SS_WALKER3D)
    hipLaunchKernelGGL((step_forces_kernel<ModelWalker3D>), grid, dim3(kWave), 0, st, P, env_ids, m, act, out);
  else
    hipLaunchKernelGGL((step_forces_kernel<ModelMike>), grid, dim3(kWave), 0, st, P, env_ids, m, act, out);
  return hipGetLastError();
}

}  // namespace ss
