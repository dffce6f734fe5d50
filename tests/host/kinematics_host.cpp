// kinematics_host.cpp -- compiles the kinematic readout's per-body and per-corner code (steppingstone_amd/csrc/ss_kinematics.hpp) for the
// CPU, so that tests/test_kinematics.py can hold it against the fp64 restatement of tests/np_kinematics.py in the GPU-less build container.
// TEST INFRASTRUCTURE ONLY: built by tests/kinematics_host_lib.py into tests/host/, never shipped.  It does per env what one 32-lane half
// of ss_kinematics.hip's kinematics_kernel does: 22 body lanes, the two detection lanes, the sums in half_sum's order.
#include <hip/hip_runtime.h>

#include <cstring>
#include <limits>
#include <vector>

#include "../../steppingstone_amd/csrc/ss_kinematics.hpp"

float ss_host_xchg(float x) { return x; }      // not used by the readout; ss_math.hpp declares them for the step harness
void ss_host_wave_sync() {}

namespace {
struct HostEnvs {
  ss::Params P;
  ss::Knobs K;
  std::vector<float> f, terr;
  std::vector<int> is;
  HostEnvs(int n, const float* packed) {
    std::memset(&P, 0, sizeof P);
    std::memset(&K, 0, sizeof K);
    P.n = n;
    P.npad = (n + 63) / 64 * 64;
    f.assign((size_t)ss::NF * P.npad, 0.f);
    terr.assign((size_t)120 * P.npad, 0.f);
    is.assign((size_t)ss::NI * P.npad, 0);
    P.fstate = f.data(); P.istate = is.data(); P.terrain = terr.data(); P.knobs = &K;
    P.id_mask = 0xFFFFFFFFu;
    for (int e = 0; e < n; ++e) ss::unpack_env(P, e, packed);
  }
};

template <class Model>
void kinematics_one(const ss::Params& P, int e, float* lds, float* body_twist, float* summary, float* corners) {
  using namespace ss;
  using namespace ss::kin;
  BodyKin kb[kBodies];
  float s[6][kHalfLanes] = {}, t[4][kHalfLanes] = {};
  for (int b = 0; b < kBodies; ++b) {
    body_kin<Model>(P, e, b, kb[b]);
    float mc[3], mv[3];
    body_moments<Model>(b, kb[b], mc, mv);
    for (int i = 0; i < 3; ++i) { s[i][b] = mc[i]; s[3 + i][b] = mv[i]; }
  }
  uint32_t code[2];
  for (int foot = 0; foot < 2; ++foot) code[foot] = foot_carriers<Model>(P, e, foot, Lds{lds, foot});
  float sum[6], com[3];
  for (int i = 0; i < 6; ++i) sum[i] = half_sum(s[i]);
  com_of<Model>(sum, com);
  for (int b = 0; b < kBodies; ++b) {
    float L[3], T;
    body_momentum<Model>(b, kb[b], com, L, T);
    for (int i = 0; i < 3; ++i) t[i][b] = L[i];
    t[3][b] = T;
  }
  float L[3];
  for (int i = 0; i < 3; ++i) L[i] = half_sum(t[i]);
  const float T = half_sum(t[3]);
  if (body_twist)
    for (int b = 0; b < kBodies; ++b)
      for (int i = 0; i < 3; ++i) { body_twist[b * 6 + i] = kb[b].w[i]; body_twist[b * 6 + 3 + i] = kb[b].v[i]; }
  if (summary) summary_row<Model>(sum, sum + 3, L, T, summary);
  if (corners)
    for (int foot = 0; foot < 2; ++foot)
      for (int c = 0; c < 4; ++c) {
        float* o = corners + (4 * foot + c) * 8;
        corner_row<Model>(P, e, foot, c, kb[foot ? LFOOT : RFOOT], o);
        o[7] = carrier_value(code[foot], c);
      }
}
}  // namespace

extern "C" {

// ss_kinematics over n envs given as packed states [n,186]: body_twist [n,22,6], summary [n,12], corners [n,8,8] (any may be null)
int kh_kinematics(int kind, int n, const float* packed, float* body_twist, float* summary, float* corners) {
  HostEnvs h(n, packed);
  // the lane-private LDS view of the detection, as tests/device/ss_probe.hip's host build has it: one block, NaN first
  std::vector<float> lds((size_t)ss::kLdsSlots * ss::kWave * 4);
  for (int e = 0; e < n; ++e) {
    std::fill(lds.begin(), lds.end(), std::numeric_limits<float>::quiet_NaN());
    float* bt = body_twist ? body_twist + (size_t)e * ss::kin::kBodies * 6 : nullptr;
    float* sm = summary ? summary + (size_t)e * SS_KIN_SUMMARY : nullptr;
    float* co = corners ? corners + (size_t)e * SS_KIN_CORNER * 8 : nullptr;
    if (kind == 0) kinematics_one<ss::ModelWalker3D>(h.P, e, lds.data(), bt, sm, co);
    else kinematics_one<ss::ModelMike>(h.P, e, lds.data(), bt, sm, co);
  }
  return 0;
}

}  // extern "C"
