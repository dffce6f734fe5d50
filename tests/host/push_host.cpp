// push_host.cpp -- compiles the impulse's per-lane code (steppingstone_amd/csrc/ss_push.hpp) for the CPU, so that tests/test_push.py can
// hold it against the fp64 restatement of tests/np_push.py in the GPU-less build container.  TEST INFRASTRUCTURE ONLY: built by
// tests/push_host_lib.py into tests/host/, never shipped.  It does per row what one 32-lane half of ss_push.hip's push_kernel does: 22
// body lanes, the composite of all bodies in subtree_sum's order, 27 DoF lanes that run eliminate / scale / substitute in the kernel's
// steps -- within a step every lane first, then the stores the kernel makes behind its barrier.
// With -DPUSH_HOST_MAIN it is a stand-alone program that pushes a few rows of a standing robot (for a sanitised build).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../steppingstone_amd/csrc/ss_push.hpp"

float ss_host_xchg(float x) { return x; }      // not used by the push; ss_math.hpp declares them for the step harness
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

// one row: env e, body bt, point (or null), wrench w -> delta_nu[27]; mass (or null) receives the assembled lower triangle
template <class Model>
void push_one(const ss::Params& P, int e, int bt, const float* point, const float* w, float* delta_nu, float* mass) {
  using namespace ss;
  using namespace ss::push;
  std::vector<float> row((size_t)kRowWords, std::numeric_limits<float>::quiet_NaN());
  float* recs = row.data() + kRecs;
  float* Ml = row.data() + kMass;
  float* r = row.data() + kRhs;
  float* pt = row.data() + kPoint;
  eom::BodyEom kb[kBodies];
  float x[eom::kParts][kHalfLanes] = {};
  for (int b = 0; b < kBodies; ++b) {
    float* rec = recs + b * eom::kBodyRecWords;
    eom::body_eom<Model>(P, e, b, kb[b], rec);
    eom::body_record<Model>(b, kb[b], rec);
    float xb[eom::kParts];
    eom::body_parts<Model>(b, kb[b], xb);
    for (int i = 0; i < eom::kParts; ++i) x[i][b] = xb[i];
    if (b == bt) pushed_point(kb[b], rec, point, pt);
  }
  float C[eom::kParts];
  for (int i = 0; i < eom::kParts; ++i) C[i] = i < kComposite ? eom::subtree_sum(x[i], 0) : 0.f;
  base_rows(kb[0], C, Ml);
  for (int b = 1; b < kBodies; ++b) joint_row<Model>(b, kb[b], recs, Ml);
  for (int i = 0; i < kDof; ++i) r[i] = rhs_word(i, bt, kb[0].R0, recs + bt * eom::kBodyRecWords, pt, w);
  if (mass) std::memcpy(mass, Ml, sizeof(float) * kTri);
  for (int s = kDof - 1; s >= 1; --s) {
    float l[kDof];
    for (int i = 0; i < s; ++i)
      if (coupled(s, i)) l[i] = eliminate(Ml, r, s, i);
    for (int i = 0; i < s; ++i)
      if (coupled(s, i)) Ml[tri(s, i)] = l[i];
  }
  for (int i = 0; i < kDof; ++i) scale(Ml, r, i);
  for (int j = 0; j < kDof - 1; ++j)
    for (int i = j + 1; i < kDof; ++i)
      if (coupled(i, j)) substitute(Ml, r, j, i);
  for (int i = 0; i < kDof; ++i) delta_nu[i] = r[i];
}
}  // namespace

extern "C" {

// ss_push's dry run over n rows, row k on env k given as packed states [n,186]: body [n] (null: the torso), point [n,3] (null: the
// centre of mass), impulse [n,6] -> delta_nu [n,27]; mass [n,378] (may be null): the lower triangle the solve started from
int ph_push(int kind, int n, const float* packed, const int* body, const float* point, const float* impulse, float* delta_nu,
            float* mass) {
  HostEnvs h(n, packed);
  const int D = ss::push::kDof, T = ss::push::kTri;
  for (int e = 0; e < n; ++e) {
    const int bt = body ? body[e] : 0;
    if (bt < 0 || bt >= ss::push::kBodies) continue;
    const float* pt = point ? point + (size_t)e * 3 : nullptr;
    float* M = mass ? mass + (size_t)e * T : nullptr;
    if (kind == 0) push_one<ss::ModelWalker3D>(h.P, e, bt, pt, impulse + (size_t)e * 6, delta_nu + (size_t)e * D, M);
    else push_one<ss::ModelMike>(h.P, e, bt, pt, impulse + (size_t)e * 6, delta_nu + (size_t)e * D, M);
  }
  return 0;
}

}  // extern "C"

#ifdef PUSH_HOST_MAIN
int main() {
  const int n = 22;
  std::vector<float> packed((size_t)n * SS_STATE_DIM, 0.f), imp((size_t)n * 6), pt((size_t)n * 3, 0.1f), dn((size_t)n * 27), M((size_t)n * 378);
  std::vector<int> body(n);
  for (int e = 0; e < n; ++e) {
    float* s = packed.data() + (size_t)e * SS_STATE_DIM;
    s[2] = 1.3f; s[3] = 1.f;                                 // upright, all joints at 0 except a little bend
    for (int j = 0; j < 21; ++j) { s[13 + j] = 0.05f * (float)(j % 5); s[34 + j] = 0.1f; }
    body[e] = e;
    for (int i = 0; i < 6; ++i) imp[(size_t)e * 6 + i] = (float)(i + 1);
  }
  float worst = 0.f;
  for (int kind = 0; kind < 2; ++kind) {
    ph_push(kind, n, packed.data(), body.data(), pt.data(), imp.data(), dn.data(), M.data());
    ph_push(kind, n, packed.data(), nullptr, nullptr, imp.data(), dn.data(), nullptr);
    for (float v : dn) worst = v != v ? std::numeric_limits<float>::infinity() : (v > worst ? v : (-v > worst ? -v : worst));
  }
  std::printf("push_host: largest |delta_nu| %g\n", worst);
  return worst < 1e6f ? 0 : 1;
}
#endif
