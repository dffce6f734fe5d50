// lookahead_states_host.cpp -- the look-ahead from caller-supplied state rows (look_row<Model, true>, steppingstone_amd/csrc/
// ss_lookahead.hpp) and the observation of a state row (obs_from_row) compiled for the CPU, on the host harness of lookahead_host.cpp:
// that file is included, so this library holds lh_step and lh_lookahead next to the new entries, built with one set of flags, and
// tests/test_lookahead_states.py can hold the one to the other bit for bit in the GPU-less build container.
// TEST INFRASTRUCTURE ONLY: built by tests/lookahead_states_host_lib.py into tests/host/, never shipped.
#include "lookahead_host.cpp"

extern "C" {

// ss_lookahead_states over an instance of n envs given as packed states [n,186]: row k is a branch of env env_ids[k] (null: env k) from
// states[k, :]; the outputs and packed_out as in lh_lookahead.
int lhs_lookahead_states(int kind, int n, unsigned long long seed, int curriculum, const double* prob, float power, const float* packed,
                         const int* env_ids, int m, const float* states, int horizon, const float* act, float* obs, float* rew,
                         unsigned char* done, float* final_state, float* work, float* packed_out) {
  Instance I(n, seed, curriculum, prob, power, 1, packed);
  const ss::look::Out out{obs, rew, done, final_state, work};
  run_waves((m + ss::kEnvsPerWave - 1) / ss::kEnvsPerWave, [&](int lg, int lane, float* lds) {
    if (kind == 0) ss::look::look_row<ss::ModelWalker3D, true>(I.P, env_ids, m, horizon, act, out, lg, lane, lds, states);
    else ss::look::look_row<ss::ModelMike, true>(I.P, env_ids, m, horizon, act, out, lg, lane, lds, states);
  });
  if (packed_out)
    for (int e = 0; e < n; ++e) ss::pack_env(I.P, e, packed_out);
  return 0;
}

// ss_get_obs_states: obs [m,60] of states [m,186]
int lhs_observe(int kind, int m, const float* states, float* obs) {
  for (int k = 0; k < m; ++k) {
    if (kind == 0) ss::look::obs_from_row<ss::ModelWalker3D>(states + (size_t)k * SS_STATE_DIM, obs + (size_t)k * SS_OBS_DIM);
    else ss::look::obs_from_row<ss::ModelMike>(states + (size_t)k * SS_STATE_DIM, obs + (size_t)k * SS_OBS_DIM);
  }
  return 0;
}

// ss_set_state + ss_get_obs: obs_kernel's body over an instance that unpack_env has put packed [n,186] into
int lhs_get_obs(int kind, int n, const float* packed, float* obs) {
  Instance I(n, 0, 0, nullptr, 1.f, 0, packed);
  const size_t np = (size_t)I.P.npad;
  for (int e = 0; e < n; ++e) {
    ss::Dyn s;
    ss::Cache c;
    ss::load_dyn(I.P, e, s);
    ss::load_cache(I.P, e, c);
    float* o = obs + (size_t)e * SS_OBS_DIM;
    if (kind == 0) ss::write_obs<ss::ModelWalker3D>(s, I.P.fstate[e + ss::F_ZINIT * np], I.P.istate[e + ss::I_FLAGS * np], c, o);
    else ss::write_obs<ss::ModelMike>(s, I.P.fstate[e + ss::F_ZINIT * np], I.P.istate[e + ss::I_FLAGS * np], c, o);
  }
  return 0;
}

}  // extern "C"
