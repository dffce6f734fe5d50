// ss_api.hip -- C ABI of libsteppingstone.so (include/steppingstone.h).  Host side only: owns the HBM-resident
// structure-of-arrays state and launches the gfx950 kernels on the caller's stream.  There is no CPU path.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ss_kernels.hpp"

// compiled in ss_rollout3.hip (its own scheduling strategy, see there)
extern template __global__ void ss::rollout_kernel_helped<ss::ModelWalker3D, 3>(ss::Params, ss::StepIO);
extern template __global__ void ss::rollout_kernel_helped<ss::ModelMike, 3>(ss::Params, ss::StepIO);
// compiled in ss_render.hip (the render kernels, docs/RENDER.md)
namespace ss {
hipError_t launch_render(const Params& P, int kind, const int32_t* env_ids, int m, int W, int H, const ss_camera& cam,
                         unsigned char* rgb, float* depth, unsigned char* seg, hipStream_t st);
hipError_t launch_body_poses(const Params& P, int kind, float* out, hipStream_t st);
// compiled in ss_kinematics.hip (the kinematic readout, docs/PHYSICS.md)
hipError_t launch_kinematics(const Params& P, int kind, const int32_t* env_ids, int m, float* body_twist, float* summary, float* corners,
                             hipStream_t st);
// compiled in ss_forces.hip (the force readout, docs/PHYSICS.md)
hipError_t launch_step_forces(const Params& P, int kind, const int32_t* env_ids, int m, const float* act, float* contacts, float* joints,
                              float* next_state, hipStream_t st);
// compiled in ss_eom.hip (the equation-of-motion readout, docs/PHYSICS.md)
hipError_t launch_eom(const Params& P, int kind, const int32_t* env_ids, int m, float* mass, float* forces, float* corner_jac,
                      hipStream_t st);
// compiled in ss_push.hip (the impulse, docs/PHYSICS.md)
hipError_t launch_push(const Params& P, int kind, const int32_t* env_ids, int m, const int32_t* body, const float* point,
                       const float* impulse, float* delta_nu, int apply, hipStream_t st);
// compiled in ss_lookahead.hip (the look-ahead, docs/PHYSICS.md)
hipError_t launch_lookahead(const Params& P, int kind, const int32_t* env_ids, int m, int horizon, const float* act, float* obs, float* rew,
                            uint8_t* done, float* final_state, float* work, hipStream_t st);
hipError_t launch_lookahead_states(const Params& P, int kind, const int32_t* env_ids, int m, const float* states, int horizon,
                                   const float* act, float* obs, float* rew, uint8_t* done, float* final_state, float* work, hipStream_t st);
hipError_t launch_obs_states(int kind, int m, const float* states, float* obs, hipStream_t st);
// compiled in ss_policy.hip (the closed-loop look-ahead, docs/PHYSICS.md 14), which defines ss_policy_words as well
hipError_t launch_policy_pack(const ss_policy_desc* d, const float* const* weight, const float* const* bias, float* packed, hipStream_t st);
hipError_t launch_lookahead_policy(const Params& P, int kind, const int32_t* env_ids, int m, const float* states, int horizon,
                                   const ss_policy_desc* d, const float* packed, const float* offset, float* act, float* obs, float* rew,
                                   uint8_t* done, float* final_state, float* work, hipStream_t st);
}  // namespace ss

// The kernels of the C ABI besides the step, reset and observation kernels.  Only this unit launches them: `static`, so that they
// exist in its code object alone.
namespace ss {

// Consumer side of the peer-store all-gather: lane r waits until peer r has published `value` (or a later step) in this
// rank's flag array.  Bounded spin: on time-out it raises *error instead of hanging the GPU.
static __global__ void peer_wait_kernel(const uint32_t* flags, int count, uint32_t value, uint32_t* error) {
  const int r = threadIdx.x;
  if (r >= count) return;
  for (long long it = 0; it < (1ll << 23); ++it) {     // ~1 s
    const uint32_t v = __hip_atomic_load(flags + r, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
    if ((int32_t)(v - value) >= 0) return;
    __builtin_amdgcn_s_sleep(8);
  }
  *error = 1u + (uint32_t)r;
}

// hook updates, stream-ordered
static __global__ void set_knobs_kernel(Knobs* dst, Knobs v) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *dst = v;
}
// per-env sampling grids: [N][121] row-major (the caller's layout, playground/train.py:267-271) -> [121][Npad]
static __global__ void transpose_prob_kernel(const float* __restrict__ src, float* __restrict__ dst, int n, int npad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * SS_NCELL) return;
  const int e = i / SS_NCELL, k = i - e * SS_NCELL;
  dst[(size_t)k * npad + e] = src[i];
}
static __global__ void copy_prob_kernel(const float* __restrict__ src, float* __restrict__ dst) {
  if (threadIdx.x < SS_NCELL) dst[threadIdx.x] = src[threadIdx.x];
}

// one thread per (env, grid cell): PHYSICS.md section 8
// create_temp_states (common/envs_utils.py:573-578, playground/train.py:247-257): per env the 121 variants of the
// current observation with the look-ahead stone moved to each (yaw, pitch) grid cell.  Only obs[55..59] differ:
// obs_kernel first writes the current observation rows (lane per env, coalesced state loads) to a scratch [N,60];
// then one 256-thread workgroup per env computes the 121 x 5 target features (one lane per cell) and streams the
// [121,60] block out as 1815 coalesced float4 -- the one HBM-bound kernel of the path (29 KB written per env).
constexpr int kTempThreads = 240;      // a multiple of 15: every thread keeps ONE float4 column of the row
static __global__ __launch_bounds__(kTempThreads) void temp_states_kernel(Params P, const float* __restrict__ obs_rows, float* out) {
  __shared__ __attribute__((aligned(16))) float base[SS_OBS_DIM];
  __shared__ float feat[SS_NCELL * 5];
  const int e = blockIdx.x, t = threadIdx.x;
  const size_t np = (size_t)P.npad;
  if (t < SS_OBS_DIM) base[t] = obs_rows[(size_t)e * SS_OBS_DIM + t];
  if (t < SS_NCELL) {
    const int cell = t;
    float pos[3], quat[4], p1[3], p2[3], tilt2[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) pos[i] = P.fstate[e + (F_POS + i) * np];
#pragma unroll
    for (int i = 0; i < 4; ++i) quat[i] = P.fstate[e + (F_QUAT + i) * np];
#pragma unroll
    for (int i = 0; i < 3; ++i) { p1[i] = P.fstate[e + (F_STONE + 8 + i) * np]; p2[i] = P.fstate[e + (F_STONE + 16 + i) * np]; }
    tilt2[0] = P.fstate[e + (F_STONE + 16 + 6) * np];
    tilt2[1] = P.fstate[e + (F_STONE + 16 + 7) * np];
    const int n = P.istate[e + I_N * np];
    if (n + 1 <= kNumStones - 1) {
      const float* T = P.terrain + e;
      const float phi_n = n < P.istate[e + I_PROV * np] ? T[(n * 6 + 3) * np] : 0.f;      // a provisional stone is not stored
      float phi = phi_n + yaw_sample(cell / SS_GRID), pitch = pitch_sample(cell % SS_GRID);
      float dr = P.fstate[e + F_NNDR * np];
      float sp, cp, sph, cph;
      sincosf(pitch, &sp, &cp);
      sincosf(phi, &sph, &cph);
      place_stone(p1[0], p1[1], p1[2], dr, cp, sp, cph, sph, p2);
    }
    float roll, pitch, cyaw, syaw;         // the yaw only: roll and pitch are dead code here
    quat_roll_pitch_cs(quat, roll, pitch, cyaw, syaw);
    float f[5];
    target_features(pos, cyaw, syaw, p2, tilt2, f);
#pragma unroll
    for (int i = 0; i < 5; ++i) feat[cell * 5 + i] = f[i];
  }
  __syncthreads();
  // Measured in round 2 (profiles/r02_*_temp_states.txt): this one-workgroup-per-env shape writes 5.0-5.3 TB/s at 32768
  // envs (a torch fill of the same buffer: 6.9 TB/s) -- and it stays there with the feature computation removed, with 60-
  // or 120-thread workgroups, with persistent workgroups (4.1-5.0 TB/s) and with one workgroup per 16 rows (1.8 TB/s,
  // latency-bound): the limit is the write pattern of 29,040-byte blocks, not the prologue.
  constexpr int kRow4 = SS_OBS_DIM / 4;                      // 15 float4 per row
  static_assert(kTempThreads % kRow4 == 0, "a thread must stay in its column");
  constexpr int kRowsPerPass = kTempThreads / kRow4;
  float4* o4 = reinterpret_cast<float4*>(out) + (size_t)e * (SS_NCELL * kRow4);
  const float4* b4 = reinterpret_cast<const float4*>(base);
  const int c4 = t % kRow4;
  const float4 bv = b4[c4 < kRow4 - 1 ? c4 : kRow4 - 2];     // this thread's column of the common part, in registers
#pragma unroll 1
  for (int row = t / kRow4; row < SS_NCELL; row += kRowsPerPass) {
    float4 v = bv;
    const float* f = feat + row * 5;
    if (c4 == kRow4 - 2) v.w = f[0];                         // obs[52..54], obs[55]
    if (c4 == kRow4 - 1) v = make_float4(f[1], f[2], f[3], f[4]);
    o4[row * kRow4 + c4] = v;          // plain stores: nontemporal ones measured 20 % slower here
  }
}

static __global__ void random_actions_kernel(Params P, uint64_t t, float* act) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= P.n) return;
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    uint32_t r[4];
    philox4x32_10((uint32_t)(6u * (uint32_t)t + b), 1u, P.env_offset + ((uint32_t)e & P.id_mask), 0u, P.seed_lo, P.seed_hi, r);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int j = b * 4 + i;
      if (j < NJ) act[(size_t)e * NJ + j] = 2.f * u01(r[i]) - 1.f;
    }
  }
}

// PMC calibration: a dword-per-lane coalesced copy with the step kernel's access shape (tools/hbm_traffic.py)
static __global__ void calib_copy_kernel(const float* __restrict__ in, float* __restrict__ out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[i] + 1.0f;
}

// packed [m,186] <-> structure of arrays (pack_env / unpack_env): row k <-> env ids[k]; ids == null: row k <-> env k.  The ids live on
// the device and are not checked by the host: an id outside [0, N) is skipped -- its row is neither read nor written (the rule of
// ss_render)
static __global__ void pack_state_kernel(Params P, const int32_t* ids, int m, float* packed) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const int e = ids ? ids[k] : k;
  if (e >= 0 && e < P.n) pack_env(P, e, packed, (size_t)k);
}
static __global__ void unpack_state_kernel(Params P, const int32_t* ids, int m, const float* packed) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const int e = ids ? ids[k] : k;
  if (e >= 0 && e < P.n) unpack_env(P, e, packed, (size_t)k);
}

// Reset of the envs whose mask byte is set (ss_reset_masked), one lane per env like reset_kernel.  With auto-reset off, a step
// followed by this kernel with the step's done as the mask leaves the state and outputs of a step with auto-reset on: both resets
// draw from the env's own Philox counter as it stands after the step.  An env whose byte is 0 is not touched at all (no state
// word, obs row or terminal row read or written), and a wavefront without a masked env ends after its 64 mask bytes.
template <class Model>
static __global__ __launch_bounds__(kWave) void reset_masked_kernel(Params P, const uint8_t* mask, float* obs, int obs_stride,
                                                                    float* terminal_obs) {
  const int e = blockIdx.x * kWave + threadIdx.x;
  if (e >= P.n || mask[e] == 0) return;
  float* row = obs ? obs + (size_t)e * obs_stride : nullptr;
  if (terminal_obs) {                  // the observation the finished step left, before the fresh one replaces it
    float t[SS_OBS_DIM];
#pragma unroll
    for (int i = 0; i < SS_OBS_DIM; ++i) t[i] = row[i];
#pragma unroll
    for (int i = 0; i < SS_OBS_DIM; ++i) terminal_obs[(size_t)e * SS_OBS_DIM + i] = t[i];
  }
  reset_env<Model>(P, e, row);
}

}  // namespace ss


namespace {

thread_local std::string g_err;
constexpr int kMaxPeerSlots = 4;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define SS_HIP(call)                                                                                   \
  do {                                                                                                 \
    hipError_t _e = (call);                                                                            \
    if (_e != hipSuccess)                                                                              \
      return fail(SS_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_e));                      \
  } while (0)

}  // namespace

struct ss_env {
  ss::Params P;
  ss::Knobs hk;         // host mirror of the device-resident hook state (P.knobs)
  ss::Knobs* dk;
  int kind;
  int device;
  float* prob_shared;   // [121]
  float* prob_env;      // [121][npad] or null
  float* obs_rows;      // [n][60] scratch: current observation rows for create_temp_states
  int helpers;          // -1 auto, else 0 / 1 / 3 helper wavefronts (env SS_HELPERS)
  int helper_max_groups;  // auto: use the helper wavefront up to this many 32-env groups
  ss::PeerTable* peer_table;   // device copy of the peer-store table (ss_peer_connect), or null
  uint32_t* peer_counter;
  uint32_t* peer_error;
  uint32_t* my_flags[4];       // this rank's flag array [G] of every ring slot (fine-grained)
  int peer_count;
  int peer_slots;
};

namespace {

// Host-synchronous hook update: a <= 500-byte hipMemcpy on the null stream.  When it returns the device copy is
// current, so every step enqueued afterwards (on any stream, or replayed from a hipGraph) sees it.
int push_knobs(ss_env* env) {
  SS_HIP(hipMemcpy(env->dk, &env->hk, sizeof(ss::Knobs), hipMemcpyHostToDevice));
  return SS_OK;
}

// the stone sampler reads the shared grid or the per-env grids (host mirror; the caller pushes it to the device)
void use_grid(ss_env* env, bool per_env) {
  env->hk.prob = per_env ? env->prob_env : env->prob_shared;
  env->hk.per_env_prob = per_env ? 1 : 0;
}

int set_window(ss_env* env, int level, bool ring) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  if (level < 0 || level > 5) return fail(SS_ERR_INVALID, "curriculum level must be in 0..5");
  float p[SS_NCELL];
  ss::window_prob(p, level, ring);
  SS_HIP(hipSetDevice(env->device));
  SS_HIP(hipMemcpy(env->prob_shared, p, sizeof p, hipMemcpyHostToDevice));
  env->hk.curriculum = level;
  use_grid(env, false);
  return push_knobs(env);
}

int zero_state(ss_env* env) {
  const ss::Params& P = env->P;
  const size_t np = (size_t)P.npad;
  SS_HIP(hipMemset(P.fstate, 0, sizeof(float) * ss::NF * np));
  SS_HIP(hipMemset(P.istate, 0, sizeof(int) * ss::NI * np));
  SS_HIP(hipMemset(P.terrain, 0, sizeof(float) * 120 * np));
  return SS_OK;
}

int helpers_for(const ss_env* env, int groups) {
  // helper wavefronts (contact operators on the CU's other SIMDs) while the batch leaves SIMDs idle: three while every
  // 4-wavefront workgroup gets a CU to itself, one while two 2-wavefront workgroups fit a CU
  return env->helpers >= 0 ? env->helpers
                           : (groups <= env->helper_max_groups / 2 ? 3 : (groups <= env->helper_max_groups ? 1 : 0));
}

inline dim3 grid64(const ss_env* env) { return dim3(env->P.npad / ss::kWave); }

// The one place that turns env->kind into the robot's model type: f(Model{}) with Model = ss::ModelWalker3D or ss::ModelMike
template <class F>
auto with_model(const ss_env* env, F&& f) {
  return env->kind == SS_WALKER3D ? f(ss::ModelWalker3D{}) : f(ss::ModelMike{});
}

// A step or rollout launch: kernel_of(helpers) is the robot's kernel with that many helper wavefronts, launched with 1 + helpers
// wavefronts per workgroup.  helpers_for() gives 0, 1 or 3; a forced SS_HELPERS of 2 or more than 3 runs the one-helper kernel.
using StepKernel = void (*)(ss::Params, ss::StepIO);
template <class KernelOf>
int launch_env_kernel(ss_env* env, const ss::StepIO& io, hipStream_t st, KernelOf&& kernel_of) {
  // two lanes per env: 32 envs per 64-lane wavefront.  ceil(n / 32) workgroups, NOT npad / 32: the arrays are padded to 64 envs, and
  // for n mod 64 in 1..32 the padding used to launch one workgroup without a single valid env (see emit_outputs: nvalid).
  const dim3 grid((env->P.n + ss::kEnvsPerWave - 1) / ss::kEnvsPerWave);
  SS_HIP(hipSetDevice(env->device));                   // the stream belongs to this device
  const int h = helpers_for(env, (int)grid.x);
  const int helpers = h == 3 ? 3 : (h > 0 ? 1 : 0);
  hipLaunchKernelGGL(kernel_of(helpers), grid, dim3(ss::kWave * (1 + helpers)), 0, st, env->P, io);
  SS_HIP(hipGetLastError());
  return SS_OK;
}

template <bool RANDOM>
int launch_step(ss_env* env, const ss::StepIO& io, hipStream_t st) {
  return with_model(env, [&](auto model) {
    using Model = decltype(model);
    return launch_env_kernel(env, io, st, [](int helpers) -> StepKernel {
      if (helpers == 3) return ss::step_kernel_helped<Model, RANDOM, 3>;
      if (helpers == 1) return ss::step_kernel_helped<Model, RANDOM, 1>;
      return ss::step_kernel<Model, RANDOM>;
    });
  });
}

// io.nsteps control steps in one launch, actions from the benchmark Philox stream
int launch_rollout(ss_env* env, const ss::StepIO& io, hipStream_t st) {
  return with_model(env, [&](auto model) {
    using Model = decltype(model);
    return launch_env_kernel(env, io, st, [](int helpers) -> StepKernel {
      if (helpers == 3) return ss::rollout_kernel_helped<Model, 3>;
      if (helpers == 1) return ss::rollout_kernel_helped<Model, 1>;
      return ss::rollout_kernel<Model>;
    });
  });
}

// a one-lane-per-env kernel of the robot (reset, observation, masked reset): kernel_of(Model{}) is its instantiation
template <class KernelOf, class... Args>
int launch_per_env(ss_env* env, hipStream_t st, KernelOf&& kernel_of, Args... args) {
  SS_HIP(hipSetDevice(env->device));
  hipLaunchKernelGGL(with_model(env, kernel_of), grid64(env), dim3(ss::kWave), 0, st, env->P, args...);
  SS_HIP(hipGetLastError());
  return SS_OK;
}

// pack_state_kernel / unpack_state_kernel over m packed rows (ids == null: the whole batch, row k <-> env k)
template <class Packed>
int launch_state_rows(ss_env* env, void (*kernel)(ss::Params, const int32_t*, int, Packed*), const int32_t* ids, int m, Packed* packed,
                      void* stream) {
  SS_HIP(hipSetDevice(env->device));
  hipLaunchKernelGGL(kernel, dim3((m + 63) / 64), dim3(64), 0, (hipStream_t)stream, env->P, ids, m, packed);
  SS_HIP(hipGetLastError());
  return SS_OK;
}

}  // namespace

extern "C" {

const char* ss_last_error(void) { return g_err.c_str(); }
int ss_version(void) { return SS_ABI_VERSION; }
int32_t ss_num_envs(const ss_env* env) { return env ? env->P.n : 0; }

int ss_create(ss_env** out, int kind, int32_t num_envs, int device, uint64_t seed, int64_t env_id_offset) {
  if (!out) return fail(SS_ERR_INVALID, "out is null");
  *out = nullptr;
  if (kind != SS_WALKER3D && kind != SS_MIKE) return fail(SS_ERR_INVALID, "unknown robot kind");
  if (num_envs <= 0) return fail(SS_ERR_INVALID, "num_envs must be positive");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(SS_ERR_NO_DEVICE, "no HIP device visible: libsteppingstone has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(SS_ERR_INVALID, "device index out of range");
  SS_HIP(hipSetDevice(device));
  ss_env* env = new ss_env();
  std::memset(env, 0, sizeof *env);
  env->kind = kind;
  env->device = device;
  {   // SS_HELPERS=0|1|3 forces the number of helper wavefronts; default: as many as cannot cost throughput
    const char* h = std::getenv("SS_HELPERS");
    env->helpers = h ? std::atoi(h) : -1;
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    env->helper_max_groups = 2 * cus;     // two 2-wavefront workgroups per CU = its four SIMDs
  }
  ss::Params& P = env->P;
  P.n = num_envs;
  P.npad = (num_envs + ss::kWave - 1) / ss::kWave * ss::kWave;
  P.seed_lo = (uint32_t)seed;
  P.seed_hi = (uint32_t)(seed >> 32);
  P.env_offset = (uint32_t)env_id_offset;
  P.id_mask = 0xFFFFFFFFu;
  env->hk.curriculum = 0;
  env->hk.power = 1.0f;
  env->hk.auto_reset = 1;
  const size_t np = (size_t)P.npad;
  hipError_t e1 = hipMalloc(&P.fstate, sizeof(float) * ss::NF * np);
  hipError_t e2 = hipMalloc(&P.istate, sizeof(int) * ss::NI * np);
  hipError_t e3 = hipMalloc(&P.terrain, sizeof(float) * 120 * np);
  hipError_t e4 = hipMalloc(&env->prob_shared, sizeof(float) * SS_NCELL);
  hipError_t e5 = hipMalloc(&env->dk, sizeof(ss::Knobs));
  P.knobs = env->dk;
  int rc = SS_OK;
  if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess || e5 != hipSuccess)
    rc = fail(SS_ERR_ALLOC, "hipMalloc failed for the environment state");
  if (rc == SS_OK) rc = zero_state(env);
  if (rc == SS_OK) rc = set_window(env, 0, false);
  if (rc != SS_OK) {      // every failure after `new`: nothing of the handle survives
    ss_destroy(env);
    return rc;
  }
  *out = env;
  return SS_OK;
}

void ss_destroy(ss_env* env) {
  if (!env) return;
  (void)hipSetDevice(env->device);
  if (env->P.fstate) (void)hipFree(env->P.fstate);
  if (env->P.istate) (void)hipFree(env->P.istate);
  if (env->P.terrain) (void)hipFree(env->P.terrain);
  if (env->prob_shared) (void)hipFree(env->prob_shared);
  if (env->dk) (void)hipFree(env->dk);
  if (env->peer_table) (void)hipFree(env->peer_table);
  if (env->peer_counter) (void)hipFree(env->peer_counter);
  if (env->peer_error) (void)hipFree(env->peer_error);
  if (env->prob_env) (void)hipFree(env->prob_env);
  if (env->obs_rows) (void)hipFree(env->obs_rows);
  if (env->P.prof) (void)hipFree(env->P.prof);
  delete env;
}

int ss_reset(ss_env* env, float* obs, void* stream) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  return launch_per_env(env, (hipStream_t)stream, [](auto model) { return ss::reset_kernel<decltype(model)>; }, obs);
}

int ss_step(ss_env* env, const float* act, float* obs, float* rew, uint8_t* done, ss_info* info, void* stream) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  if (!act || !obs || !rew || !done) return fail(SS_ERR_INVALID, "act/obs/rew/done must be device pointers");
  ss::StepIO io{act, obs, rew, done, info, 0, nullptr, 1, nullptr, 0, 0};
  return launch_step<false>(env, io, (hipStream_t)stream);
}

int ss_rollout_random(ss_env* env, int32_t num_steps, int32_t steps_per_launch, uint64_t t0, float* obs, float* rew,
                      uint8_t* done, ss_info* info, void* stream) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  if (!obs || !rew || !done) return fail(SS_ERR_INVALID, "obs/rew/done must be device pointers");
  if (num_steps < 0 || steps_per_launch < 0) return fail(SS_ERR_INVALID, "num_steps / steps_per_launch must be >= 0");
  const int32_t chunk = steps_per_launch > 0 ? steps_per_launch : 1000;     // K = 1000 steps per launch
  for (int32_t k = 0; k < num_steps; k += chunk) {
    const int32_t ns = num_steps - k < chunk ? num_steps - k : chunk;
    ss::StepIO io{nullptr, obs, rew, done, info, t0 + (uint64_t)k, nullptr, ns, nullptr, 0, 0};
    int rc = ns == 1 ? launch_step<true>(env, io, (hipStream_t)stream) : launch_rollout(env, io, (hipStream_t)stream);
    if (rc != SS_OK) return rc;
  }
  return SS_OK;
}

int ss_rollout_random_packed(ss_env* env, int32_t num_steps, uint64_t t0, float* packed, ss_info* info, void* stream) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  if (!packed) return fail(SS_ERR_INVALID, "packed must be a device pointer to [num_steps, N, 62] floats");
  if (num_steps < 1) return fail(SS_ERR_INVALID, "num_steps must be >= 1");
  ss::StepIO io{nullptr, nullptr, nullptr, nullptr, info, t0, packed, num_steps, nullptr, 0, (long long)env->P.n * (SS_OBS_DIM + 2)};
  return launch_rollout(env, io, (hipStream_t)stream);
}

int ss_step_packed(ss_env* env, const float* act, int use_random_actions, uint64_t t, float* packed, ss_info* info,
                   void* stream) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  if (!packed || (!act && !use_random_actions)) return fail(SS_ERR_INVALID, "packed (and act, unless random) must be set");
  ss::StepIO io{act, nullptr, nullptr, nullptr, info, t, packed, 1, nullptr, 0, 0};
  return use_random_actions ? launch_step<true>(env, io, (hipStream_t)stream) : launch_step<false>(env, io, (hipStream_t)stream);
}

// ---- peer-store all-gather (multi-GPU without a collective library in the data path)
int ss_peer_alloc(void** out, uint64_t bytes) {
  if (!out || bytes == 0) return fail(SS_ERR_INVALID, "bad argument");
  SS_HIP(hipExtMallocWithFlags(out, (size_t)bytes, hipDeviceMallocFinegrained));
  SS_HIP(hipMemset(*out, 0, (size_t)bytes));
  SS_HIP(hipDeviceSynchronize());
  return SS_OK;
}
int ss_peer_free(void* ptr) {
  if (ptr) SS_HIP(hipFree(ptr));
  return SS_OK;
}
int ss_peer_ipc_handle(void* ptr, void* handle64) {
  if (!ptr || !handle64) return fail(SS_ERR_INVALID, "null argument");
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "ipc handle size");
  SS_HIP(hipIpcGetMemHandle(reinterpret_cast<hipIpcMemHandle_t*>(handle64), ptr));
  return SS_OK;
}
int ss_peer_ipc_open(const void* handle64, void** out) {
  if (!handle64 || !out) return fail(SS_ERR_INVALID, "null argument");
  hipIpcMemHandle_t h;
  std::memcpy(&h, handle64, sizeof h);
  SS_HIP(hipIpcOpenMemHandle(out, h, hipIpcMemLazyEnablePeerAccess));
  return SS_OK;
}
int ss_peer_ipc_close(void* ptr) {
  if (ptr) SS_HIP(hipIpcCloseMemHandle(ptr));
  return SS_OK;
}

int ss_peer_connect(ss_env* env, int32_t count, int32_t rank, int32_t slots, float* const* gather_bufs, uint32_t* const* flag_bufs) {
  if (!env || !gather_bufs || !flag_bufs) return fail(SS_ERR_INVALID, "null argument");
  if (count < 1 || count > ss::kMaxPeers || rank < 0 || rank >= count) return fail(SS_ERR_INVALID, "need 1 <= count <= 8, 0 <= rank < count");
  if (slots < 1 || slots > kMaxPeerSlots) return fail(SS_ERR_INVALID, "need 1 <= slots <= 4");
  SS_HIP(hipSetDevice(env->device));
  if (!env->peer_counter) {
    SS_HIP(hipMalloc(&env->peer_counter, sizeof(uint32_t)));
    SS_HIP(hipMalloc(&env->peer_error, sizeof(uint32_t)));
    SS_HIP(hipMalloc(&env->peer_table, sizeof(ss::PeerTable) * kMaxPeerSlots));
  }
  SS_HIP(hipDeviceSynchronize());
  SS_HIP(hipMemset(env->peer_counter, 0, sizeof(uint32_t)));
  SS_HIP(hipMemset(env->peer_error, 0, sizeof(uint32_t)));
  ss::PeerTable t[kMaxPeerSlots];
  std::memset(t, 0, sizeof t);
  for (int s = 0; s < slots; ++s) {
    for (int p = 0; p < count; ++p) {
      if (!gather_bufs[s * count + p] || !flag_bufs[s * count + p]) return fail(SS_ERR_INVALID, "null peer buffer");
      t[s].dst[p] = gather_bufs[s * count + p];
      t[s].flag[p] = flag_bufs[s * count + p];
    }
    t[s].done_counter = env->peer_counter;
    t[s].count = count;
    t[s].rank = rank;
    t[s].n_local = env->P.n;
    env->my_flags[s] = flag_bufs[s * count + rank];
  }
  SS_HIP(hipMemcpy(env->peer_table, t, sizeof t, hipMemcpyHostToDevice));
  env->peer_count = count;
  env->peer_slots = slots;
  return SS_OK;
}

int ss_step_packed_peers(ss_env* env, const float* act, int use_random_actions, uint64_t t, int32_t slot, uint32_t step_id,
                         float* packed, ss_info* info, void* stream) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  if (!env->peer_table) return fail(SS_ERR_INVALID, "ss_peer_connect has not been called");
  if (slot < 0 || slot >= env->peer_slots) return fail(SS_ERR_INVALID, "slot out of range");
  if (!act && !use_random_actions) return fail(SS_ERR_INVALID, "act must be set unless random");
  ss::StepIO io{act, nullptr, nullptr, nullptr, info, t, packed, 1, env->peer_table + slot, step_id, 0};
  return use_random_actions ? launch_step<true>(env, io, (hipStream_t)stream) : launch_step<false>(env, io, (hipStream_t)stream);
}

int ss_peer_wait(ss_env* env, int32_t slot, uint32_t step_id, void* stream) {
  if (!env || !env->peer_table) return fail(SS_ERR_INVALID, "ss_peer_connect has not been called");
  if (slot < 0 || slot >= env->peer_slots) return fail(SS_ERR_INVALID, "slot out of range");
  SS_HIP(hipSetDevice(env->device));
  hipLaunchKernelGGL(ss::peer_wait_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const uint32_t*)env->my_flags[slot],
                     env->peer_count, step_id, env->peer_error);
  SS_HIP(hipGetLastError());
  return SS_OK;
}

int ss_peer_error(ss_env* env, uint32_t* out) {
  if (!env || !out || !env->peer_error) return fail(SS_ERR_INVALID, "bad argument");
  SS_HIP(hipSetDevice(env->device));
  SS_HIP(hipMemcpy(out, env->peer_error, sizeof(uint32_t), hipMemcpyDeviceToHost));
  return SS_OK;
}

int ss_random_actions(ss_env* env, uint64_t t, float* act, void* stream) {
  if (!env || !act) return fail(SS_ERR_INVALID, "null argument");
  SS_HIP(hipSetDevice(env->device));
  hipLaunchKernelGGL(ss::random_actions_kernel, dim3((env->P.n + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     env->P, t, act);
  SS_HIP(hipGetLastError());
  return SS_OK;
}

int ss_set_curriculum(ss_env* env, int32_t level) { return set_window(env, level, false); }
int ss_set_specialist(ss_env* env, int32_t level) { return set_window(env, level, true); }

int ss_set_sample_prob(ss_env* env, const double* prob, int per_env) {
  if (!env || !prob) return fail(SS_ERR_INVALID, "null argument");
  SS_HIP(hipSetDevice(env->device));
  if (!per_env) {
    float p[SS_NCELL];
    for (int k = 0; k < SS_NCELL; ++k) p[k] = (float)prob[k];
    SS_HIP(hipMemcpy(env->prob_shared, p, sizeof p, hipMemcpyHostToDevice));
    use_grid(env, false);
    return push_knobs(env);
  }
  const size_t np = (size_t)env->P.npad;
  if (!env->prob_env) SS_HIP(hipMalloc(&env->prob_env, sizeof(float) * SS_NCELL * np));
  std::vector<float> t(SS_NCELL * np, 0.f);
  for (int e = 0; e < env->P.n; ++e)
    for (int k = 0; k < SS_NCELL; ++k) t[(size_t)k * np + e] = (float)prob[(size_t)e * SS_NCELL + k];
  SS_HIP(hipMemcpy(env->prob_env, t.data(), sizeof(float) * t.size(), hipMemcpyHostToDevice));
  use_grid(env, true);
  return push_knobs(env);
}

int ss_set_sample_prob_device(ss_env* env, const float* prob, int per_env, void* stream) {
  if (!env || !prob) return fail(SS_ERR_INVALID, "null argument");
  SS_HIP(hipSetDevice(env->device));
  hipStream_t st = (hipStream_t)stream;
  if (!per_env) {
    hipLaunchKernelGGL(ss::copy_prob_kernel, dim3(1), dim3(128), 0, st, prob, env->prob_shared);
  } else {
    const size_t np = (size_t)env->P.npad;
    if (!env->prob_env) {
      SS_HIP(hipMalloc(&env->prob_env, sizeof(float) * SS_NCELL * np));      // first use only (allocation synchronises)
      SS_HIP(hipMemset(env->prob_env, 0, sizeof(float) * SS_NCELL * np));
    }
    const int total = env->P.n * SS_NCELL;
    hipLaunchKernelGGL(ss::transpose_prob_kernel, dim3((total + 255) / 256), dim3(256), 0, st, prob, env->prob_env, env->P.n,
                       env->P.npad);
  }
  use_grid(env, per_env != 0);
  // the pointer / flag switch travels on the same stream, behind the grid it refers to
  hipLaunchKernelGGL(ss::set_knobs_kernel, dim3(1), dim3(64), 0, st, env->dk, env->hk);
  SS_HIP(hipGetLastError());
  return SS_OK;
}

int ss_set_mirror(ss_env* env, int32_t on) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  // ACCEPTED FOR PROTOCOL COMPATIBILITY ONLY: no state, no effect.  The reference forwards set_mirror to every env
  // (common/envs_utils.py:588-590; playground/train.py:109-111 under use_phase_mirror).  What an env does with it is in the
  // absent mocca_envs; the only consumer visible in the reference is the gait-phase-clocked Cassie stepper of train.py:37, whose
  // observation carries a phase variable.  The 60-float Walker3D / Mike observation (docs/PHYSICS.md 5) has no phase term, so there
  // is nothing for the flag to shift; the mirror symmetry itself is carried by ss_get_mirror_indices.
  (void)on;
  return SS_OK;
}

int ss_set_power(ss_env* env, float power) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  SS_HIP(hipSetDevice(env->device));
  env->hk.power = power;
  return push_knobs(env);
}

int ss_set_auto_reset(ss_env* env, int32_t on) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  SS_HIP(hipSetDevice(env->device));
  env->hk.auto_reset = on ? 1 : 0;
  return push_knobs(env);
}

int ss_create_temp_states(ss_env* env, float* out, void* stream) {
  if (!env || !out) return fail(SS_ERR_INVALID, "null argument");
  SS_HIP(hipSetDevice(env->device));
  if ((reinterpret_cast<uintptr_t>(out) & 15u) != 0) return fail(SS_ERR_INVALID, "out must be 16-byte aligned");
  if (!env->obs_rows) SS_HIP(hipMalloc(&env->obs_rows, sizeof(float) * SS_OBS_DIM * (size_t)env->P.npad));
  int rc = launch_per_env(env, (hipStream_t)stream, [](auto model) { return ss::obs_kernel<decltype(model)>; }, env->obs_rows);
  if (rc != SS_OK) return rc;
  hipLaunchKernelGGL(ss::temp_states_kernel, dim3(env->P.n), dim3(ss::kTempThreads), 0, (hipStream_t)stream, env->P,
                     (const float*)env->obs_rows, out);      // one workgroup per env
  SS_HIP(hipGetLastError());
  return SS_OK;
}

int ss_get_mirror_indices(int kind, int32_t* buf, int32_t* lens) {
  if (!buf || !lens) return fail(SS_ERR_INVALID, "null argument");
  (void)kind;   // both robots share the topology
  // In POLICY coordinates (docs/PHYSICS.md 2, ss::kPolicySign): the left limbs' x / z joints are measured about the mirrored
  // axis, so a mirror swaps the limbs without negating them and only the spine's z / x joints negate in place -- the lists
  // the reference's shipped actors are equivariant under (tools/checkpoint_layout_probe.py).  Generated from model.py.
  const auto& neg_j = ss::kMirrorNegate;
  const auto& right_j = ss::kMirrorRight;
  const auto& left_j = ss::kMirrorLeft;
  std::vector<int32_t> neg_obs = {2, 4}, right_obs, left_obs, neg_act, right_act, left_act;
  for (int j : neg_j) neg_obs.push_back(6 + j);
  for (int j : neg_j) neg_obs.push_back(27 + j);
  for (int i : {50, 53, 55, 58}) neg_obs.push_back(i);
  for (int j : right_j) right_obs.push_back(6 + j);
  for (int j : right_j) right_obs.push_back(27 + j);
  right_obs.push_back(48);
  for (int j : left_j) left_obs.push_back(6 + j);
  for (int j : left_j) left_obs.push_back(27 + j);
  left_obs.push_back(49);
  for (int j : neg_j) neg_act.push_back(j);
  for (int j : right_j) right_act.push_back(j);
  for (int j : left_j) left_act.push_back(j);
  const std::vector<int32_t>* lists[6] = {&neg_obs, &right_obs, &left_obs, &neg_act, &right_act, &left_act};
  int32_t* o = buf;
  for (int i = 0; i < 6; ++i) {
    lens[i] = (int32_t)lists[i]->size();
    for (int32_t v : *lists[i]) *o++ = v;
  }
  return SS_OK;
}

// PMC calibration helper: copies n floats in -> out (dword per lane, coalesced), device pointers
int ss_debug_calib_copy(const float* in, float* out, uint64_t n, void* stream) {
  if (!in || !out) return fail(SS_ERR_INVALID, "null argument");
  hipLaunchKernelGGL(ss::calib_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, out,
                     (size_t)n);
  SS_HIP(hipGetLastError());
  return SS_OK;
}

// Self-check aid (tests/test_gpu_first_launch.py): envs e and e' with (e & mask) == (e' & mask) share their global id, i.e. their
// Philox streams (reset noise, stone draws, benchmark actions); given the same state they must produce the same bits in one launch.
int ss_debug_set_id_mask(ss_env* env, uint32_t mask) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  env->P.id_mask = mask;
  return SS_OK;
}

// tuning aid: per-phase shader-clock totals (all zeros unless the library was built with -DSS_PROFILE_PHASES)
int ss_debug_phase_cycles(ss_env* env, unsigned long long* out16, int reset) {
  if (!env || !out16) return fail(SS_ERR_INVALID, "null argument");
  SS_HIP(hipSetDevice(env->device));
  if (!env->P.prof) {
    SS_HIP(hipMalloc(&env->P.prof, 16 * sizeof(unsigned long long)));
    SS_HIP(hipMemset(env->P.prof, 0, 16 * sizeof(unsigned long long)));
  }
  SS_HIP(hipDeviceSynchronize());
  SS_HIP(hipMemcpy(out16, env->P.prof, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  if (reset) SS_HIP(hipMemset(env->P.prof, 0, 16 * sizeof(unsigned long long)));
  return SS_OK;
}

int ss_get_state(ss_env* env, float* packed, void* stream) {
  if (!env || !packed) return fail(SS_ERR_INVALID, "null argument");
  return launch_state_rows(env, ss::pack_state_kernel, nullptr, env->P.n, packed, stream);
}

int ss_set_state(ss_env* env, const float* packed, void* stream) {
  if (!env || !packed) return fail(SS_ERR_INVALID, "null argument");
  return launch_state_rows(env, ss::unpack_state_kernel, nullptr, env->P.n, packed, stream);
}

int ss_reset_masked(ss_env* env, const uint8_t* mask, float* obs, int32_t obs_stride, float* terminal_obs, void* stream) {
  if (!env || !mask) return fail(SS_ERR_INVALID, "null handle or mask");
  if (obs_stride != SS_OBS_DIM && obs_stride != SS_OBS_DIM + 2)
    return fail(SS_ERR_INVALID, "ss_reset_masked: obs_stride must be 60 (ss_step's obs) or 62 (ss_step_packed's block)");
  if (terminal_obs && !obs) return fail(SS_ERR_INVALID, "ss_reset_masked: terminal_obs needs obs to copy the rows from");
  return launch_per_env(env, (hipStream_t)stream, [](auto model) { return ss::reset_masked_kernel<decltype(model)>; }, mask, obs,
                        (int)obs_stride, terminal_obs);
}

int ss_get_state_envs(ss_env* env, const int32_t* env_ids, int32_t m, float* packed, void* stream) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  if (m < 0) return fail(SS_ERR_INVALID, "ss_get_state_envs: m must be >= 0");
  if (m > 0 && (!env_ids || !packed)) return fail(SS_ERR_INVALID, "ss_get_state_envs: env_ids and packed must be device pointers");
  if (m == 0) return SS_OK;
  return launch_state_rows(env, ss::pack_state_kernel, env_ids, m, packed, stream);
}

int ss_set_state_envs(ss_env* env, const int32_t* env_ids, int32_t m, const float* packed, void* stream) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  if (m < 0) return fail(SS_ERR_INVALID, "ss_set_state_envs: m must be >= 0");
  if (m > 0 && (!env_ids || !packed)) return fail(SS_ERR_INVALID, "ss_set_state_envs: env_ids and packed must be device pointers");
  if (m == 0) return SS_OK;
  return launch_state_rows(env, ss::unpack_state_kernel, env_ids, m, packed, stream);
}

int ss_get_obs(ss_env* env, float* obs, void* stream) {
  if (!env || !obs) return fail(SS_ERR_INVALID, "null argument");
  return launch_per_env(env, (hipStream_t)stream, [](auto model) { return ss::obs_kernel<decltype(model)>; }, obs);
}

int ss_camera_default(ss_camera* cam) {
  if (!cam) return fail(SS_ERR_INVALID, "null argument");
  // docs/RENDER.md 1: a three-quarter view from the robot's right, aimed ahead of the torso and below it, so that a reset robot
  // (torso 1.0-1.2 m up) and its next stone 0.75 m ahead both fill the frame
  *cam = ss_camera{SS_CAM_TRACK, {-0.9f, -2.3f, 0.45f}, {0.4f, 0.f, -0.5f}, 45.f, 20.f, SS_CAM_SHADOWS};
  return SS_OK;
}

int ss_body_poses(ss_env* env, float* out, void* stream) {
  if (!env || !out) return fail(SS_ERR_INVALID, "null argument");
  if ((uintptr_t)out & 15) return fail(SS_ERR_INVALID, "ss_body_poses: out must be 16-byte aligned");
  SS_HIP(hipSetDevice(env->device));
  SS_HIP(ss::launch_body_poses(env->P, env->kind, out, (hipStream_t)stream));
  return SS_OK;
}

int ss_render(ss_env* env, const int32_t* env_ids, int32_t m, int32_t width, int32_t height, const ss_camera* cam, uint8_t* rgb,
              float* depth, uint8_t* seg, void* stream) {
  if (!env || !env_ids || !cam) return fail(SS_ERR_INVALID, "null argument");
  if (m < 1) return fail(SS_ERR_INVALID, "ss_render: m must be >= 1");
  if (width < 4 || height < 4 || width > 2048 || height > 2048 || width % 4 || height % 4)
    return fail(SS_ERR_INVALID, "ss_render: width and height must be multiples of 4 in 4..2048");
  if (!rgb && !depth && !seg) return fail(SS_ERR_INVALID, "ss_render: rgb, depth and seg are all NULL");
  if (cam->mode != SS_CAM_TRACK && cam->mode != SS_CAM_CHASE && cam->mode != SS_CAM_FIXED)
    return fail(SS_ERR_INVALID, "ss_render: camera mode must be SS_CAM_TRACK, SS_CAM_CHASE or SS_CAM_FIXED");
  if (!(cam->fov_y_deg > 0.f && cam->fov_y_deg < 180.f) || !(cam->far_m > 0.f && cam->far_m < 3.0e38f))
    return fail(SS_ERR_INVALID, "ss_render: fov_y_deg must lie in (0, 180) and far_m be positive and finite");
  {
    // the view vector (docs/RENDER.md 1): the eye offset for TRACK / CHASE, target - eye for FIXED.  camera_setup normalises it.
    float v2 = 0.f;
    bool finite = true;
    for (int i = 0; i < 3; ++i) {
      const float ei = cam->eye[i], ti = cam->target[i];
      finite = finite && std::isfinite(ei) && std::isfinite(ti);
      const float v = cam->mode == SS_CAM_FIXED ? ti - ei : ei;
      v2 += v * v;
    }
    if (!finite || !(v2 >= 1e-12f))
      return fail(SS_ERR_INVALID, "ss_render: eye and target must be finite and the view vector at least 1e-6 m long");
  }
  if (((uintptr_t)rgb & 3) || ((uintptr_t)seg & 3) || ((uintptr_t)depth & 3))
    return fail(SS_ERR_INVALID, "ss_render: rgb, depth and seg must be 4-byte aligned");
  SS_HIP(hipSetDevice(env->device));
  SS_HIP(ss::launch_render(env->P, env->kind, env_ids, m, width, height, *cam, rgb, depth, seg, (hipStream_t)stream));
  return SS_OK;
}

int ss_kinematics(ss_env* env, const int32_t* env_ids, int32_t m, float* body_twist, float* summary, float* corners, void* stream) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  if (m < 0) return fail(SS_ERR_INVALID, "ss_kinematics: m must be >= 0");
  if (m == 0) return SS_OK;
  if (!env_ids && m != env->P.n) return fail(SS_ERR_INVALID, "ss_kinematics: env_ids == NULL (envs 0..m-1) needs m == num_envs");
  if (!body_twist && !summary && !corners) return fail(SS_ERR_INVALID, "ss_kinematics: body_twist, summary and corners are all NULL");
  if (((uintptr_t)body_twist | (uintptr_t)summary | (uintptr_t)corners) & 15)
    return fail(SS_ERR_INVALID, "ss_kinematics: body_twist, summary and corners must be 16-byte aligned");
  SS_HIP(hipSetDevice(env->device));
  SS_HIP(ss::launch_kinematics(env->P, env->kind, env_ids, m, body_twist, summary, corners, (hipStream_t)stream));
  return SS_OK;
}

int ss_step_forces(ss_env* env, const int32_t* env_ids, int32_t m, const float* act, float* contacts, float* joints, float* next_state,
                   void* stream) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  if (m < 0) return fail(SS_ERR_INVALID, "ss_step_forces: m must be >= 0");
  if (m == 0) return SS_OK;
  if (!env_ids && m != env->P.n) return fail(SS_ERR_INVALID, "ss_step_forces: env_ids == NULL (envs 0..m-1) needs m == num_envs");
  if (!act) return fail(SS_ERR_INVALID, "ss_step_forces: act is NULL");
  if (!contacts && !joints && !next_state) return fail(SS_ERR_INVALID, "ss_step_forces: contacts, joints and next_state are all NULL");
  if (((uintptr_t)contacts | (uintptr_t)joints | (uintptr_t)next_state) & 15)
    return fail(SS_ERR_INVALID, "ss_step_forces: contacts, joints and next_state must be 16-byte aligned");
  SS_HIP(hipSetDevice(env->device));
  SS_HIP(ss::launch_step_forces(env->P, env->kind, env_ids, m, act, contacts, joints, next_state, (hipStream_t)stream));
  return SS_OK;
}

int ss_eom(ss_env* env, const int32_t* env_ids, int32_t m, float* mass, float* forces, float* corner_jac, void* stream) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  if (m < 0) return fail(SS_ERR_INVALID, "ss_eom: m must be >= 0");
  if (m == 0) return SS_OK;
  if (!env_ids && m != env->P.n) return fail(SS_ERR_INVALID, "ss_eom: env_ids == NULL (envs 0..m-1) needs m == num_envs");
  if (!mass && !forces && !corner_jac) return fail(SS_ERR_INVALID, "ss_eom: mass, forces and corner_jac are all NULL");
  if (((uintptr_t)mass | (uintptr_t)forces | (uintptr_t)corner_jac) & 15)
    return fail(SS_ERR_INVALID, "ss_eom: mass, forces and corner_jac must be 16-byte aligned");
  SS_HIP(hipSetDevice(env->device));
  SS_HIP(ss::launch_eom(env->P, env->kind, env_ids, m, mass, forces, corner_jac, (hipStream_t)stream));
  return SS_OK;
}

int ss_push(ss_env* env, const int32_t* env_ids, int32_t m, const int32_t* body, const float* point, const float* impulse,
            float* delta_nu, int32_t apply, void* stream) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  if (m < 0) return fail(SS_ERR_INVALID, "ss_push: m must be >= 0");
  if (m == 0) return SS_OK;
  if (!env_ids && m != env->P.n) return fail(SS_ERR_INVALID, "ss_push: env_ids == NULL (envs 0..m-1) needs m == num_envs");
  if (!impulse) return fail(SS_ERR_INVALID, "ss_push: impulse is NULL");
  if (!apply && !delta_nu) return fail(SS_ERR_INVALID, "ss_push: a dry run (apply == 0) needs delta_nu");
  if ((uintptr_t)delta_nu & 15) return fail(SS_ERR_INVALID, "ss_push: delta_nu must be 16-byte aligned");
  SS_HIP(hipSetDevice(env->device));
  SS_HIP(ss::launch_push(env->P, env->kind, env_ids, m, body, point, impulse, delta_nu, apply ? 1 : 0, (hipStream_t)stream));
  return SS_OK;
}

int ss_lookahead(ss_env* env, const int32_t* env_ids, int32_t m, int32_t horizon, const float* act, float* obs, float* rew, uint8_t* done,
                 float* final_state, float* work, void* stream) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  if (m < 0) return fail(SS_ERR_INVALID, "ss_lookahead: m must be >= 0");
  if (horizon < 1 || horizon > SS_LOOK_MAX_STEPS) return fail(SS_ERR_INVALID, "ss_lookahead: horizon must be in [1, SS_LOOK_MAX_STEPS]");
  if (m == 0) return SS_OK;
  if (!env_ids && m != env->P.n) return fail(SS_ERR_INVALID, "ss_lookahead: env_ids == NULL (envs 0..m-1) needs m == num_envs");
  if (((uintptr_t)obs | (uintptr_t)rew | (uintptr_t)final_state | (uintptr_t)work) & 15)
    return fail(SS_ERR_INVALID, "ss_lookahead: obs, rew, final_state and work must be 16-byte aligned");
  if (!act || !rew || !done || !work) return fail(SS_ERR_INVALID, "ss_lookahead: act, rew, done and work are required when m > 0");
  SS_HIP(hipSetDevice(env->device));
  SS_HIP(ss::launch_lookahead(env->P, env->kind, env_ids, m, horizon, act, obs, rew, done, final_state, work, (hipStream_t)stream));
  return SS_OK;
}

int ss_lookahead_states(ss_env* env, const int32_t* env_ids, int32_t m, const float* states, int32_t horizon, const float* act, float* obs,
                        float* rew, uint8_t* done, float* final_state, float* work, void* stream) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  if (m < 0) return fail(SS_ERR_INVALID, "ss_lookahead_states: m must be >= 0");
  if (horizon < 1 || horizon > SS_LOOK_MAX_STEPS)
    return fail(SS_ERR_INVALID, "ss_lookahead_states: horizon must be in [1, SS_LOOK_MAX_STEPS]");
  if (m == 0) return SS_OK;
  if (!env_ids && m != env->P.n) return fail(SS_ERR_INVALID, "ss_lookahead_states: env_ids == NULL (envs 0..m-1) needs m == num_envs");
  if (((uintptr_t)obs | (uintptr_t)rew | (uintptr_t)final_state | (uintptr_t)work) & 15)
    return fail(SS_ERR_INVALID, "ss_lookahead_states: obs, rew, final_state and work must be 16-byte aligned");
  if ((uintptr_t)states & 3) return fail(SS_ERR_INVALID, "ss_lookahead_states: states must be 4-byte aligned");
  if (!states || !act || !rew || !done || !work)
    return fail(SS_ERR_INVALID, "ss_lookahead_states: states, act, rew, done and work are required when m > 0");
  SS_HIP(hipSetDevice(env->device));
  SS_HIP(ss::launch_lookahead_states(env->P, env->kind, env_ids, m, states, horizon, act, obs, rew, done, final_state, work,
                                     (hipStream_t)stream));
  return SS_OK;
}

int ss_get_obs_states(ss_env* env, int32_t m, const float* states, float* obs, void* stream) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  if (m < 0) return fail(SS_ERR_INVALID, "ss_get_obs_states: m must be >= 0");
  if (m == 0) return SS_OK;
  if (!states || !obs) return fail(SS_ERR_INVALID, "ss_get_obs_states: states and obs are required when m > 0");
  if (((uintptr_t)states | (uintptr_t)obs) & 3) return fail(SS_ERR_INVALID, "ss_get_obs_states: states and obs must be 4-byte aligned");
  SS_HIP(hipSetDevice(env->device));
  SS_HIP(ss::launch_obs_states(env->kind, m, states, obs, (hipStream_t)stream));
  return SS_OK;
}

int ss_policy_pack(ss_env* env, const ss_policy_desc* d, const float* const* weight, const float* const* bias, float* packed, void* stream) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  if (ss_policy_words(d) < 0) return fail(SS_ERR_INVALID, "ss_policy_pack: not a valid policy description");
  if (!weight || !bias || !packed) return fail(SS_ERR_INVALID, "ss_policy_pack: weight, bias and packed are required");
  for (int l = 0; l < d->layers; ++l) {
    if (!weight[l] || !bias[l]) return fail(SS_ERR_INVALID, "ss_policy_pack: a layer's weight or bias is NULL");
    if (((uintptr_t)weight[l] | (uintptr_t)bias[l]) & 3) return fail(SS_ERR_INVALID, "ss_policy_pack: weight and bias must be 4-byte aligned");
  }
  if ((uintptr_t)packed & 15) return fail(SS_ERR_INVALID, "ss_policy_pack: packed must be 16-byte aligned");
  SS_HIP(hipSetDevice(env->device));
  SS_HIP(ss::launch_policy_pack(d, weight, bias, packed, (hipStream_t)stream));
  return SS_OK;
}

int ss_lookahead_policy(ss_env* env, const int32_t* env_ids, int32_t m, const float* states, int32_t horizon, const ss_policy_desc* d,
                        const float* packed, const float* act_offset, float* act, float* obs, float* rew, uint8_t* done,
                        float* final_state, float* work, void* stream) {
  if (!env) return fail(SS_ERR_INVALID, "null handle");
  if (m < 0) return fail(SS_ERR_INVALID, "ss_lookahead_policy: m must be >= 0");
  if (horizon < 1 || horizon > SS_LOOK_MAX_STEPS)
    return fail(SS_ERR_INVALID, "ss_lookahead_policy: horizon must be in [1, SS_LOOK_MAX_STEPS]");
  if (ss_policy_words(d) < 0) return fail(SS_ERR_INVALID, "ss_lookahead_policy: not a valid policy description");
  if (m == 0) return SS_OK;
  if (!env_ids && m != env->P.n) return fail(SS_ERR_INVALID, "ss_lookahead_policy: env_ids == NULL (envs 0..m-1) needs m == num_envs");
  if (((uintptr_t)obs | (uintptr_t)rew | (uintptr_t)final_state | (uintptr_t)work | (uintptr_t)packed) & 15)
    return fail(SS_ERR_INVALID, "ss_lookahead_policy: packed, obs, rew, final_state and work must be 16-byte aligned");
  if (((uintptr_t)states | (uintptr_t)act_offset | (uintptr_t)act) & 3)
    return fail(SS_ERR_INVALID, "ss_lookahead_policy: states, act_offset and act must be 4-byte aligned");
  if (!packed || !rew || !done || !work) return fail(SS_ERR_INVALID, "ss_lookahead_policy: packed, rew, done and work are required when m > 0");
  SS_HIP(hipSetDevice(env->device));
  SS_HIP(ss::launch_lookahead_policy(env->P, env->kind, env_ids, m, states, horizon, d, packed, act_offset, act, obs, rew, done, final_state,
                                     work, (hipStream_t)stream));
  return SS_OK;
}

}  // extern "C"
