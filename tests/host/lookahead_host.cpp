// lookahead_host.cpp -- compiles the look-ahead's per-lane code (steppingstone_amd/csrc/ss_lookahead.hpp) for the CPU, next to the
// control step it restates (step_env, with the auto-reset switch as an argument), so that tests/test_lookahead.py can hold the one to
// the other bit for bit in the GPU-less build container.
// TEST INFRASTRUCTURE ONLY: built by tests/lookahead_host_lib.py into tests/host/, never shipped.  A wavefront runs as in
// tests/host/host_harness.cpp: its 64 lanes are 64 threads around one LDS block, the two lanes of a row meet at every lane-pair
// exchange, all 64 where the device code relies on the wavefront's lockstep (SS_WAVE_SYNC).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <thread>
#include <vector>

#include "../../steppingstone_amd/csrc/ss_lookahead.hpp"

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
thread_local Barrier* t_wave = nullptr;
thread_local int t_side = 0;

// an instance of n envs from packed states [n,186]
struct Instance {
  ss::Params P;
  ss::Knobs K;
  std::vector<float> f, terr, pr;
  std::vector<int> is;
  Instance(int n, unsigned long long seed, int curriculum, const double* prob, float power, int auto_reset, const float* packed) {
    std::memset(&P, 0, sizeof P);
    std::memset(&K, 0, sizeof K);
    P.n = n;
    P.npad = (n + 63) / 64 * 64;
    f.assign((size_t)ss::NF * P.npad, 0.f);
    terr.assign((size_t)120 * P.npad, 0.f);
    is.assign((size_t)ss::NI * P.npad, 0);
    pr.resize(121);
    ss::window_prob(pr.data(), curriculum, false);
    if (prob) for (int k = 0; k < 121; ++k) pr[k] = (float)prob[k];
    K.prob = pr.data(); K.per_env_prob = 0; K.curriculum = curriculum; K.power = power; K.auto_reset = auto_reset;
    P.fstate = f.data(); P.istate = is.data(); P.terrain = terr.data(); P.knobs = &K;
    P.seed_lo = (uint32_t)seed; P.seed_hi = (uint32_t)(seed >> 32); P.env_offset = 0; P.id_mask = 0xFFFFFFFFu;
    for (int e = 0; e < n; ++e) ss::unpack_env(P, e, packed);
  }
};

template <class Body>
void run_waves(int waves, Body&& body) {
  for (int w = 0; w < waves; ++w) {
    std::vector<float4> lds((size_t)ss::kLdsSlots * ss::kWave);
    std::memset(lds.data(), 0xFF, lds.size() * sizeof(float4));      // NaN first: nothing may rely on a cleared block
    Barrier wave(ss::kWave);
    std::vector<PairSync> pairs(ss::kEnvsPerWave);
    auto run = [&](int lane) {
      t_sync = &pairs[lane >> 1];
      t_wave = &wave;
      t_side = lane & 1;
      body(ss::kWave * w + lane, lane, reinterpret_cast<float*>(lds.data()));
    };
    std::vector<std::thread> th;
    for (int lane = 1; lane < ss::kWave; ++lane) th.emplace_back(run, lane);
    run(0);
    for (auto& t : th) t.join();
  }
}
}  // namespace

float ss_host_xchg(float x) {
  PairSync* s = t_sync;
  s->slot[t_side] = x;
  s->b.wait();
  float r = s->slot[1 - t_side];
  s->b.wait();
  return r;
}
void ss_host_wave_sync() { t_wave->wait(); }

extern "C" {

int lh_work_words() { return SS_LOOK_WORK; }

// one control step of n envs (ss_step): packed state in / out [n,186], act [n,21]; outputs obs [n,60], rew, done, info
int lh_step(int kind, int n, unsigned long long seed, int curriculum, const double* prob, float power, int auto_reset,
            const float* packed_in, const float* act, float* packed_out, float* obs, float* rew, unsigned char* done, ss_info* info) {
  Instance I(n, seed, curriculum, prob, power, auto_reset, packed_in);
  ss::StepIO io{act, obs, rew, done, info, 0, nullptr, 1, nullptr, 0, 0};
  run_waves((2 * n + 63) / 64, [&](int lg, int lane, float* lds) {
    if (kind == 0) ss::step_env<ss::ModelWalker3D, false>(I.P, io, lg, lane, lds);
    else ss::step_env<ss::ModelMike, false>(I.P, io, lg, lane, lds);
  });
  for (int e = 0; e < n; ++e) ss::pack_env(I.P, e, packed_out);
  return 0;
}

// ss_lookahead over an instance of n envs given as packed states [n,186]: env_ids [m] (null: 0..m-1), act [m,H,21]; obs [m,H,60] (may be
// null), rew [m,H], done [m,H], final_state [m,186] (may be null), work [m, SS_LOOK_WORK].  packed_out [n,186] (may be null): the
// instance's state after the call, which must be the state before it.
int lh_lookahead(int kind, int n, unsigned long long seed, int curriculum, const double* prob, float power, const float* packed,
                 const int* env_ids, int m, int horizon, const float* act, float* obs, float* rew, unsigned char* done,
                 float* final_state, float* work, float* packed_out) {
  Instance I(n, seed, curriculum, prob, power, 1, packed);       // the switch is on: a branch must ignore it
  const ss::look::Out out{obs, rew, done, final_state, work};
  run_waves((m + ss::kEnvsPerWave - 1) / ss::kEnvsPerWave, [&](int lg, int lane, float* lds) {
    if (kind == 0) ss::look::look_row<ss::ModelWalker3D>(I.P, env_ids, m, horizon, act, out, lg, lane, lds);
    else ss::look::look_row<ss::ModelMike>(I.P, env_ids, m, horizon, act, out, lg, lane, lds);
  });
  if (packed_out)
    for (int e = 0; e < n; ++e) ss::pack_env(I.P, e, packed_out);
  return 0;
}

}  // extern "C"
