// ss_push.hip -- the impulse kernel (docs/PHYSICS.md 12): delta_nu = M^-1 J^T w for a wrench impulse on any body of
// selected envs, optionally added to the envs' velocities.  The only state words it writes are 7:13 and 34:55 of the listed envs, and
// only with `apply`; ss_api.hip validates the arguments and calls the launcher below.
#include <hip/hip_runtime.h>

#include "ss_push.hpp"

namespace ss {
namespace push {

// 8 rows per workgroup as in the eom kernel: 8 x 1709 words = 54 688 B of static LDS.  The kernel's registers hold a CU to 8 wavefronts,
// which is two such workgroups, so 4 rows per workgroup (27 KB each) raise no occupancy; built that way it times the same.
#ifndef SS_PUSH_ROWS
#define SS_PUSH_ROWS 8                                     // (a tuning build may set 4: tools/push_rate.py under STEPPINGSTONE_LIB)
#endif
constexpr int kRowsPerBlock = SS_PUSH_ROWS;
constexpr int kThreads = kRowsPerBlock * kHalfLanes;
static_assert(kThreads % kWave == 0 && kWave % kHalfLanes == 0, "whole wavefronts, whole halves");
static_assert(kRowsPerBlock * kRowWords * sizeof(float) <= 64 * 1024, "static LDS");

// eom::subtree_sum for body 0 (every body, from 21 down to 0), one term per lane of the row's half.  Every lane takes every exchange.
__device__ __forceinline__ float lane_total(float x) {
  float s = 0.f;
#pragma unroll
  for (int t = kBodies - 1; t >= 0; --t) s = s + __shfl(x, t, kHalfLanes);
  return s;
}

// One 32-lane half of a wavefront = one requested row k (env env_ids[k], body body[k]).  Body lane b walks its chain and leaves its
// record; the lane of the pushed body leaves the point.  After the first barrier body lane b writes row 5 + b of M's lower triangle
// (lane 0: the base block) and DoF lane i word i of J^T w; after the second the DoF lanes factor and substitute in LDS, a barrier per
// step.  A row outside [0, m), an env id outside [0, N) or a body outside [0, 22) reads and writes nothing in global memory; its lanes
// still reach every barrier and exchange (on whatever its LDS block holds).  What is computed does not depend on `apply` or on
// delta_nu being asked for: only the stores do.  HBM stores per row: 27 words of delta_nu, 27 words of state.
template <class Model>
__global__ __launch_bounds__(kThreads) void push_kernel(Params P, const int32_t* env_ids, int m, const int32_t* body,
                                                         const float* point, const float* impulse, float* delta_nu, int apply) {
  __shared__ float lds[kRowsPerBlock * kRowWords];
  const int half = threadIdx.x / kHalfLanes, b = threadIdx.x % kHalfLanes;
  const int k = blockIdx.x * kRowsPerBlock + half;
  int e = -1, bt = 0;
  if (k < m) {
    e = env_ids ? env_ids[k] : k;
    bt = body ? body[k] : 0;
  }
  const bool valid = e >= 0 && e < P.n && bt >= 0 && bt < kBodies;
  if (!valid) bt = 0;
  const bool is_body = valid && b < kBodies;
  const bool dof = valid && b < kDof;
  float* row = lds + half * kRowWords;
  float* recs = row + kRecs;
  float* Ml = row + kMass;
  float* r = row + kRhs;
  float* pt = row + kPoint;
  float* rec = recs + (is_body ? b : 0) * eom::kBodyRecWords;

  eom::BodyEom kb;
  float x[eom::kParts];
#pragma unroll
  for (int i = 0; i < eom::kParts; ++i) x[i] = 0.f;
  if (is_body) {
    eom::body_eom<Model>(P, e, b, kb, rec);
    eom::body_record<Model>(b, kb, rec);
    eom::body_parts<Model>(b, kb, x);
    if (b == bt) pushed_point(kb, rec, point ? point + (size_t)k * 3 : nullptr, pt);
  }
  float C[eom::kParts];
#pragma unroll
  for (int i = 0; i < eom::kParts; ++i) C[i] = i < kComposite ? lane_total(x[i]) : 0.f;
  __syncthreads();

  if (is_body && b == 0) base_rows(kb, C, Ml);
  if (is_body && b >= 1) joint_row<Model>(b, kb, recs, Ml);
  if (dof) {
    float w[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) w[i] = impulse[(size_t)k * 6 + i];
    r[b] = rhs_word(b, bt, kb.R0, recs + bt * eom::kBodyRecWords, pt, w);     // kb.R0 is read by the base DoFs b < 6 alone: body lanes
  }
  __syncthreads();

#pragma unroll 1
  for (int s = kDof - 1; s >= 1; --s) {
    const bool on = dof && b < s && coupled(s, b);
    float l = 0.f;
    if (on) l = eliminate(Ml, r, s, b);
    __syncthreads();
    if (on) Ml[tri(s, b)] = l;
  }
  __syncthreads();
  if (dof) scale(Ml, r, b);
  __syncthreads();
#pragma unroll 1
  for (int j = 0; j < kDof - 1; ++j) {
    if (dof && b > j && coupled(b, j)) substitute(Ml, r, j, b);
    __syncthreads();
  }

  if (dof) {
    const float d = r[b];
    if (delta_nu) delta_nu[(size_t)k * kDof + b] = d;
    if (apply) {
      float* F = P.fstate + e + (size_t)(b < 6 ? F_VEL + b : F_QD + (b - 6)) * (size_t)P.npad;
      *F = *F + d;
    }
  }
}

}  // namespace push

// launcher called by ss_api.hip (arguments validated there; m >= 1)
hipError_t launch_push(const Params& P, int kind, const int32_t* env_ids, int m, const int32_t* body, const float* point,
                       const float* impulse, float* delta_nu, int apply, hipStream_t st) {
  using namespace push;
  const dim3 grid((m + kRowsPerBlock - 1) / kRowsPerBlock);
  if (kind == SS_WALKER3D)
    hipLaunchKernelGGL((push_kernel<ModelWalker3D>), grid, dim3(kThreads), 0, st, P, env_ids, m, body, point, impulse, delta_nu, apply);
  else
    hipLaunchKernelGGL((push_kernel<ModelMike>), grid, dim3(kThreads), 0, st, P, env_ids, m, body, point, impulse, delta_nu, apply);
  return hipGetLastError();
}

}  // namespace ss
