// eom_host.cpp -- compiles the equation-of-motion readout's per-lane code (steppingstone_amd/csrc/ss_eom.hpp) for the CPU, so that
// tests/test_eom.py can hold it against the fp64 restatement of tests/np_eom.py in the GPU-less build container.  TEST INFRASTRUCTURE
// ONLY: built by tests/eom_host_lib.py into tests/host/, never shipped.  It does per env what one 32-lane half of ss_eom.hip's eom_kernel
// does: 22 body lanes, the subtree sums in subtree_sum's order, every pair of the mass matrix from one value.
#include <hip/hip_runtime.h>

#include <cstring>
#include <limits>
#include <vector>

#include "../../steppingstone_amd/csrc/ss_eom.hpp"

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
void eom_one(const ss::Params& P, int e, float* M, float* Fo, float* J) {
  using namespace ss;
  using namespace ss::eom;
  BodyEom kb[kBodies];
  LaneEom L[kBodies];
  std::vector<float> recs((size_t)kBodies * kBodyRecWords, std::numeric_limits<float>::quiet_NaN());
  float x[kParts][kHalfLanes] = {};
  for (int b = 0; b < kBodies; ++b) {
    float* rec = recs.data() + b * kBodyRecWords;
    body_eom<Model>(P, e, b, kb[b], rec);
    body_record<Model>(b, kb[b], rec);
    float xb[kParts];
    body_parts<Model>(b, kb[b], xb);
    for (int i = 0; i < kParts; ++i) x[i][b] = xb[i];
  }
  for (int b = 0; b < kBodies; ++b) {
    for (int i = 0; i < kParts; ++i) L[b].C[i] = subtree_sum(x[i], b);
    if (b >= 1) lane_finish<Model>(P, e, b, kb[b], recs.data(), L[b]);
  }
  float blk[6][6], bias[6], grav[6];
  base_block(kb[0], L[0].C, blk, bias, grav);
  for (int a = 0; a < 6; ++a) {
    if (M)
      for (int c = 0; c <= a; ++c) { M[a * kDof + c] = blk[a][c]; M[c * kDof + a] = blk[a][c]; }
    if (Fo) { Fo[a] = bias[a]; Fo[kDof + a] = grav[a]; Fo[2 * kDof + a] = 0.f; }
  }
  for (int b = 1; b < kBodies; ++b) {
    const int row = 5 + b;
    const float* rec = recs.data() + b * kBodyRecWords;
    if (Fo) { Fo[row] = L[b].bias; Fo[kDof + row] = L[b].grav; Fo[2 * kDof + row] = L[b].passive; }
    if (!M) continue;
    for (int c = 0; c < 6; ++c) {
      const float v = on_base(kb[b].R0, c, L[b].Fo, L[b].Ff);
      M[row * kDof + c] = v;
      M[c * kDof + row] = v;
    }
    for (int l = 0; l < depth_of(b); ++l) {
      const int col = 5 + level_body(b, l);
      const float v = mass_at_level<Model>(b, l, rec, L[b]);
      M[row * kDof + col] = v;
      M[col * kDof + row] = v;
    }
    for (int a = 1; a < kBodies; ++a)
      if (!carries(a, b) && !carries(b, a)) M[row * kDof + 5 + a] = 0.f;
  }
  if (J)
    for (int foot = 0; foot < 2; ++foot) {
      const int fb = foot ? LFOOT : RFOOT;
      const float* rec = recs.data() + fb * kBodyRecWords;
      for (int q = 0; q < 4; ++q) {
        float xc[3], o[3];
        float* Jq = J + (4 * foot + q) * 3 * kDof;
        corner_offset<Model>(foot, q, kb[fb], xc);
        for (int c = 0; c < 6; ++c) {
          corner_jac_base(kb[fb], xc, c, o);
          for (int i = 0; i < 3; ++i) Jq[i * kDof + c] = o[i];
        }
        for (int l = 0; l < depth_of(fb); ++l) {
          corner_jac_level(rec, l, xc, o);
          for (int i = 0; i < 3; ++i) Jq[i * kDof + 5 + level_body(fb, l)] = o[i];
        }
        for (int a = 1; a < kBodies; ++a)
          if (!carries(a, fb))
            for (int i = 0; i < 3; ++i) Jq[i * kDof + 5 + a] = 0.f;
      }
    }
}
}  // namespace

extern "C" {

// ss_eom over n envs given as packed states [n,186]: mass [n,27,27], forces [n,3,27], corner_jac [n,8,3,27] (any may be null)
int eh_eom(int kind, int n, const float* packed, float* mass, float* forces, float* corner_jac) {
  HostEnvs h(n, packed);
  const int D = ss::eom::kDof;
  for (int e = 0; e < n; ++e) {
    float* M = mass ? mass + (size_t)e * D * D : nullptr;
    float* Fo = forces ? forces + (size_t)e * SS_EOM_FORCES * D : nullptr;
    float* J = corner_jac ? corner_jac + (size_t)e * SS_KIN_CORNER * 3 * D : nullptr;
    if (kind == 0) eom_one<ss::ModelWalker3D>(h.P, e, M, Fo, J);
    else eom_one<ss::ModelMike>(h.P, e, M, Fo, J);
  }
  return 0;
}

}  // extern "C"
