// render_host.cpp -- compiles the render kernels' per-body, per-primitive and per-pixel code (steppingstone_amd/csrc/ss_render.hpp) for
// the CPU, so that tests/test_render_host.py can compare its frames with tests/np_render.py in the GPU-less build container.
// TEST INFRASTRUCTURE ONLY: built by tests/test_render_host.py into tests/host/, never shipped.  It does per env and per tile what one
// workgroup of ss_render.hip's render_kernel does: poses, primitives, stones, camera, the tile's cull mask, then every pixel.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../steppingstone_amd/csrc/ss_render.hpp"

float ss_host_xchg(float x) { return x; }      // not used by the render code; ss_math.hpp declares them for the step harness
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

template <class Model, class Vis>
void render_one(const ss::Params& P, int e, int m, int W, int H, const ss_camera& cam, unsigned char* rgb, float* depth,
                unsigned char* seg) {
  using namespace ss::render;
  const bool valid = e >= 0 && e < P.n;
  float poses[kBodies * 12];
  Prim prims[kPrims];
  Cam c;
  if (valid) {
    for (int b = 0; b < kBodies; ++b) body_pose<Model>(P, e, b, &poses[12 * b]);
    for (int k = 0; k < kRobotPrims; ++k) robot_prim<Vis>(k, poses, prims[k]);
    for (int s = 0; s < kStones; ++s) stone_prim(P, e, s, prims[kRobotPrims + s]);
  }
  camera_setup(cam, P, e, valid, W, H, c);
  for (int i0 = 0; i0 < H; i0 += kTile)
    for (int j0 = 0; j0 < W; j0 += kTile) {
      const int i1 = i0 + kTile < H ? i0 + kTile : H, j1 = j0 + kTile < W ? j0 + kTile : W;
      uint32_t mask = 0;
      for (int k = 0; k < kPrims; ++k)
        if (valid && (k >= kRobotPrims || prim_in_tile(prims[k], c, i0, i1, j0, j1))) mask |= 1u << k;
      for (int i = i0; i < i1; ++i)
        for (int j = j0; j < j1; ++j) {
          float col[3], dep;
          int sg;
          shade_pixel(prims, valid ? kPrims : 0, mask, c, i, j, (cam.flags & 1) != 0, col, dep, sg);
          const size_t px = ((size_t)m * H + i) * W + j;
          if (rgb)
            for (int k = 0; k < 3; ++k) rgb[px * 3 + k] = to_u8(col[k]);
          if (depth) depth[px] = dep;
          if (seg) seg[px] = (unsigned char)sg;
        }
    }
}
}  // namespace

extern "C" {

// body poses of n envs given as packed states [n,186]: out [n,22,12]
int rh_body_poses(int kind, int n, const float* packed, float* out) {
  HostEnvs h(n, packed);
  for (int e = 0; e < n; ++e)
    for (int b = 0; b < ss::render::kBodies; ++b) {
      if (kind == 0) ss::render::body_pose<ss::ModelWalker3D>(h.P, e, b, out + ((size_t)e * ss::render::kBodies + b) * 12);
      else ss::render::body_pose<ss::ModelMike>(h.P, e, b, out + ((size_t)e * ss::render::kBodies + b) * 12);
    }
  return 0;
}

// frames of the m envs env_ids[] of n envs given as packed states [n,186] (ss_render's outputs; any may be null)
int rh_render(int kind, int n, const float* packed, const int* env_ids, int m, int W, int H, const ss_camera* cam,
              unsigned char* rgb, float* depth, unsigned char* seg) {
  HostEnvs h(n, packed);
  for (int k = 0; k < m; ++k) {
    if (kind == 0) render_one<ss::ModelWalker3D, ss::VisualWalker3D>(h.P, env_ids[k], k, W, H, *cam, rgb, depth, seg);
    else render_one<ss::ModelMike, ss::VisualMike>(h.P, env_ids[k], k, W, H, *cam, rgb, depth, seg);
  }
  return 0;
}

}  // extern "C"
