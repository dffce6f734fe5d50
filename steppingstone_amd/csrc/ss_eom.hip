// ss_eom.hip -- the equation-of-motion readout kernel (docs/PHYSICS.md 11): joint-space inertia, velocity-product force,
// gravity and passive torques, and the sole-corner Jacobians of selected envs.  It only READS the environment state; ss_api.hip
// validates the arguments and calls the launcher below.
#include <hip/hip_runtime.h>

#include "ss_eom.hpp"

namespace ss {
namespace eom {

constexpr int kEnvsPerBlock = 8;
constexpr int kThreads = kEnvsPerBlock * kHalfLanes;
static_assert(kThreads % kWave == 0 && kWave % kHalfLanes == 0, "whole wavefronts, whole halves");

// subtree_sum of ss_eom.hpp, one term per lane of the env's 32-lane half.  Every lane of the wavefront takes every exchange.
__device__ __forceinline__ float lane_subtree_sum(float x, int b) {
  float s = 0.f;
  const int end = subtree_end(b);
#pragma unroll
  for (int t = kBodies - 1; t >= 0; --t) {
    const float xt = __shfl(x, t, kHalfLanes);
    if (t >= b && t <= end) s = s + xt;
  }
  return s;
}

// One 32-lane half of a wavefront = one requested row k (env env_ids[k]); lane b = body b walks its own ancestor chain (no lane waits for
// another) and leaves its record in LDS; after the one barrier lane b = j + 1 owns DoF 6 + j: it sums its subtree's inertia about its own
// joint from the records, takes the 16 sums about the torso origin with lane exchanges, and writes its word of each `forces` row and, of
// `mass`, the pairs (6 + j, DoF of an ancestor or itself) -- on both sides of the diagonal from one value -- and the zeros of its row.
// Lane 0 owns the base block.  The foot lanes 8 / 13 write their four corners' Jacobians.  A row outside [0, m) or an env id outside
// [0, N) reads and writes nothing in global memory; its lanes still reach the barrier and take the exchanges.  What is computed does not
// depend on which outputs are requested: only the stores do.  All stores are single words: rows of 729 and 81 words keep no wider alignment.
template <class Model>
__global__ __launch_bounds__(kThreads) void eom_kernel(Params P, const int32_t* env_ids, int m, float* mass, float* forces,
                                                        float* corner_jac) {
  __shared__ float lds[kEnvsPerBlock * kBodies * kBodyRecWords];
  const int half = threadIdx.x / kHalfLanes, b = threadIdx.x % kHalfLanes;
  const int k = blockIdx.x * kEnvsPerBlock + half;
  int e = -1;
  if (k < m) e = env_ids ? env_ids[k] : k;
  const bool valid = e >= 0 && e < P.n;
  const bool body = valid && b < kBodies;
  const bool joint = body && b >= 1;
  const bool foot = body && (b == RFOOT || b == LFOOT);
  float* recs = lds + half * (kBodies * kBodyRecWords);
  float* rec = recs + (body ? b : 0) * kBodyRecWords;

  BodyEom kb;
  LaneEom L;
  float x[kParts];
#pragma unroll
  for (int i = 0; i < kParts; ++i) x[i] = 0.f;
  if (body) {
    body_eom<Model>(P, e, b, kb, rec);
    body_record<Model>(b, kb, rec);
    body_parts<Model>(b, kb, x);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kParts; ++i) L.C[i] = lane_subtree_sum(x[i], b);
  if (joint) lane_finish<Model>(P, e, b, kb, recs, L);

  float* M = mass ? mass + (size_t)k * (kDof * kDof) : nullptr;
  float* Fo = forces ? forces + (size_t)k * (SS_EOM_FORCES * kDof) : nullptr;
  float* J = corner_jac ? corner_jac + (size_t)k * (SS_KIN_CORNER * 3 * kDof) : nullptr;
  const int row = 5 + b;                   // joint lanes: DoF 6 + (b - 1)
  const int f01 = b == LFOOT ? 1 : 0;
  const int depth = body ? depth_of(b) : 0;

  if (body && b == 0) {                    // the base block, the base words of bias and gravity, the zeros of passive
    float blk[6][6], bias[6], grav[6];
    base_block(kb, L.C, blk, bias, grav);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      if (M) {
#pragma unroll
        for (int c = 0; c <= a; ++c) {
          M[a * kDof + c] = blk[a][c];
          if (c != a) M[c * kDof + a] = blk[a][c];
        }
      }
      if (Fo) { Fo[a] = bias[a]; Fo[kDof + a] = grav[a]; Fo[2 * kDof + a] = 0.f; }
    }
  }
  if (joint && Fo) { Fo[row] = L.bias; Fo[kDof + row] = L.grav; Fo[2 * kDof + row] = L.passive; }
  if (joint && M) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {          // base columns: the lane's momentum about O against the six base screws
      const float v = on_base(kb.R0, c, L.Fo, L.Ff);
      M[row * kDof + c] = v;
      M[c * kDof + row] = v;
    }
#pragma unroll 1
    for (int l = 0; l < depth; ++l) {      // the joints of its chain, its own last
      const int col = 5 + level_body(b, l);
      const float v = mass_at_level<Model>(b, l, rec, L);
      M[row * kDof + col] = v;
      if (col != row) M[col * kDof + row] = v;
    }
#pragma unroll 1
    for (int a = 1; a < kBodies; ++a)      // the joints that neither carry the lane's body nor are carried by it
      if (!carries(a, b) && !carries(b, a)) M[row * kDof + 5 + a] = 0.f;
  }
  if (foot && J) {
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
      float xc[3], o[3];
      float* Jq = J + (4 * f01 + q) * 3 * kDof;
      corner_offset<Model>(f01, q, kb, xc);
#pragma unroll 1
      for (int c = 0; c < 6; ++c) {
        corner_jac_base(kb, xc, c, o);
        for (int i = 0; i < 3; ++i) Jq[i * kDof + c] = o[i];
      }
#pragma unroll 1
      for (int l = 0; l < depth; ++l) {
        corner_jac_level(rec, l, xc, o);
        for (int i = 0; i < 3; ++i) Jq[i * kDof + 5 + level_body(b, l)] = o[i];
      }
#pragma unroll 1
      for (int a = 1; a < kBodies; ++a)
        if (!carries(a, b))
          for (int i = 0; i < 3; ++i) Jq[i * kDof + 5 + a] = 0.f;
    }
  }
}

}  // namespace eom

// launcher called by ss_api.hip (arguments validated there; m >= 1)
hipError_t launch_eom(const Params& P, int kind, const int32_t* env_ids, int m, float* mass, float* forces, float* corner_jac,
                      hipStream_t st) {
  using namespace eom;
  const dim3 grid((m + kEnvsPerBlock - 1) / kEnvsPerBlock);
  if (kind == SS_WALKER3D)
    hipLaunchKernelGGL((eom_kernel<ModelWalker3D>), grid, dim3(kThreads), 0, st, P, env_ids, m, mass, forces, corner_jac);
  else
    hipLaunchKernelGGL((eom_kernel<ModelMike>), grid, dim3(kThreads), 0, st, P, env_ids, m, mass, forces, corner_jac);
  return hipGetLastError();
}

}  // namespace ss
