// forces_host.cpp -- compiles the force readout's per-lane code (steppingstone_amd/csrc/ss_forces.hpp) for the CPU, so that
// tests/test_step_forces.py can hold it against the fp64 oracle and the host harness' control step in the GPU-less build container.
// TEST INFRASTRUCTURE ONLY: built by tests/forces_host_lib.py into tests/host/, never shipped.  A wavefront runs as in
// tests/host/host_harness.cpp: its 64 lanes are 64 threads around one LDS block, the two lanes of a row meet at every lane-pair exchange.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#include "../../steppingstone_amd/csrc/ss_forces.hpp"

namespace {
struct Barrier {
  const int parties;
  std::atomic<int> arrived{0};
  std::atomic<int> generation{0};
  explicit Barrier(int n) : parties(n) {}
  void wait() {
    int g = generation.load(std::memory_order_acquire);
    if (arrived.fetch_add(1, std::memory_order_acq_rel) == parties - 1) {
      arrived.store(0, std::memory_order_relaxed);
      generation.store(g + 1, std::memory_order_release);
    } else {
      while (generation.load(std::memory_order_acquire) == g) std::this_thread::yield();
    }
  }
};
struct PairSync {
  Barrier b{2};
  float slot[2];
};
thread_local PairSync* t_sync = nullptr;
thread_local int t_side = 0;
}  // namespace

float ss_host_xchg(float x) {
  PairSync* s = t_sync;
  s->slot[t_side] = x;
  s->b.wait();
  float r = s->slot[1 - t_side];
  s->b.wait();
  return r;
}
void ss_host_wave_sync() {}      // the readout has no wavefront-wide hand-over

extern "C" {

// ss_step_forces over an instance of n envs given as packed states [n,186]: env_ids [m] (null: 0..m-1), act [m,21], power;
// contacts [m,4,8,8], joints [m,4,4,21], next_state [m,56] (any may be null).  packed_out [n,186] (may be null): the instance's state
// after the call, which must be the state before it.
int fh_step_forces(int kind, int n, const float* packed, const int* env_ids, int m, const float* act, float power, float* contacts,
                   float* joints, float* next_state, float* packed_out) {
  ss::Params P;
  ss::Knobs K;
  std::memset(&P, 0, sizeof P);
  std::memset(&K, 0, sizeof K);
  P.n = n;
  P.npad = (n + 63) / 64 * 64;
  std::vector<float> f((size_t)ss::NF * P.npad, 0.f), terr((size_t)120 * P.npad, 0.f);
  std::vector<int> is((size_t)ss::NI * P.npad, 0);
  K.power = power;
  P.fstate = f.data(); P.istate = is.data(); P.terrain = terr.data(); P.knobs = &K;
  P.id_mask = 0xFFFFFFFFu;
  for (int e = 0; e < n; ++e) ss::unpack_env(P, e, packed);
  const ss::frc::Out out{contacts, joints, next_state};
  const int waves = (m + ss::kEnvsPerWave - 1) / ss::kEnvsPerWave;
  for (int w = 0; w < waves; ++w) {
    std::vector<float4> lds((size_t)ss::kLdsSlots * ss::kWave);
    std::memset(lds.data(), 0xFF, lds.size() * sizeof(float4));      // NaN first: nothing may rely on a cleared block
    std::vector<PairSync> pairs(ss::kEnvsPerWave);
    auto run = [&](int lane) {
      t_sync = &pairs[lane >> 1];
      t_side = lane & 1;
      const int lg = ss::kWave * w + lane;
      if (kind == 0) ss::frc::forces_row<ss::ModelWalker3D>(P, env_ids, m, act, out, lg, lane, reinterpret_cast<float*>(lds.data()));
      else ss::frc::forces_row<ss::ModelMike>(P, env_ids, m, act, out, lg, lane, reinterpret_cast<float*>(lds.data()));
    };
    std::vector<std::thread> th;
    for (int lane = 1; lane < ss::kWave; ++lane) th.emplace_back(run, lane);
    run(0);
    for (auto& t : th) t.join();
  }
  if (packed_out)
    for (int e = 0; e < n; ++e) ss::pack_env(P, e, packed_out);
  return 0;
}

}  // extern "C"
