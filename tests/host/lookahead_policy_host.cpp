// lookahead_policy_host.cpp -- the closed-loop look-ahead (look_row with the action source of steppingstone_amd/csrc/ss_policy.hpp)
// compiled for the CPU, on the host harness of lookahead_host.cpp through lookahead_states_host.cpp: those files are included, so this
// library holds lh_lookahead, lhs_lookahead_states and lhs_observe next to the new entries, built with one set of flags, and
// tests/test_lookahead_policy.py can hold the closed loop to the open loop bit for bit in the GPU-less build container.  The MLP is the
// host form of ss_policy.hpp (eval_row over the packed words that packed_word lays out: the repack is under test as well).
// TEST INFRASTRUCTURE ONLY: built by tests/lookahead_policy_host_lib.py into tests/host/, never shipped.
#include "lookahead_states_host.cpp"

#include "../../steppingstone_amd/csrc/ss_policy.hpp"

extern "C" {

long long lhp_policy_words(const ss_policy_desc* d) {
  ss::policy::Net net;
  return ss::policy::make_net(d, net) ? (long long)net.words : -1;
}

// ss_policy_pack: weight / bias are arrays of d->layers host pointers; packed: lhp_policy_words(d) words
int lhp_policy_pack(const ss_policy_desc* d, const float* const* weight, const float* const* bias, float* packed) {
  ss::policy::Net net;
  if (!ss::policy::make_net(d, net)) return 1;
  ss::policy::Arrays A{};
  for (int l = 0; l < net.layers; ++l) { A.weight[l] = weight[l]; A.bias[l] = bias[l]; }
  for (int i = 0; i < net.words; ++i) packed[i] = ss::policy::packed_word(net, A, i);
  return 0;
}

// f of x [rows,60] -> y [rows,21], the chain the host build of the look-ahead evaluates
int lhp_policy_eval(const ss_policy_desc* d, const float* packed, int rows, const float* x, float* y) {
  ss::policy::Net net;
  if (!ss::policy::make_net(d, net)) return 1;
  float o[32], t0[SS_POLICY_MAX_WIDTH], t1[SS_POLICY_MAX_WIDTH];
  for (int r = 0; r < rows; ++r) {
    ss::policy::eval_row(net, packed, x + (size_t)r * SS_OBS_DIM, o, t0, t1);
    for (int i = 0; i < SS_ACT_DIM; ++i) y[(size_t)r * SS_ACT_DIM + i] = o[i];
  }
  return 0;
}

// ss_lookahead_policy over an instance of n envs given as packed states [n,186]; states, offset, act, obs, final_state, packed_out may
// be null; everything else as in lh_lookahead
int lhp_lookahead_policy(int kind, int n, unsigned long long seed, int curriculum, const double* prob, float power, const float* packed_state,
                         const int* env_ids, int m, const float* states, int horizon, const ss_policy_desc* d, const float* packed,
                         const float* offset, float* act, float* obs, float* rew, unsigned char* done, float* final_state, float* work,
                         float* packed_out) {
  ss::policy::Net net;
  if (!ss::policy::make_net(d, net)) return 1;
  Instance I(n, seed, curriculum, prob, power, 1, packed_state);
  const ss::look::Out out{obs, rew, done, final_state, work};
  const int waves = (m + ss::kEnvsPerWave - 1) / ss::kEnvsPerWave;
  std::vector<float> xb((size_t)waves * ss::policy::kXWords);
  std::memset(xb.data(), 0xFF, xb.size() * sizeof(float));           // NaN first
  run_waves(waves, [&](int lg, int lane, float* lds) {
    const ss::policy::ActPolicy src{net, packed, offset, act, xb.data() + (size_t)(lg / ss::kWave) * ss::policy::kXWords, 0};
    if (kind == 0) {
      if (states) ss::look::look_row<ss::ModelWalker3D, true>(I.P, env_ids, m, horizon, nullptr, out, lg, lane, lds, states, src);
      else ss::look::look_row<ss::ModelWalker3D, false>(I.P, env_ids, m, horizon, nullptr, out, lg, lane, lds, states, src);
    } else {
      if (states) ss::look::look_row<ss::ModelMike, true>(I.P, env_ids, m, horizon, nullptr, out, lg, lane, lds, states, src);
      else ss::look::look_row<ss::ModelMike, false>(I.P, env_ids, m, horizon, nullptr, out, lg, lane, lds, states, src);
    }
  });
  if (packed_out)
    for (int e = 0; e < n; ++e) ss::pack_env(I.P, e, packed_out);
  return 0;
}

}  // extern "C"
