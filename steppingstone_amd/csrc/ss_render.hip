// ss_render.hip -- the render kernels (docs/RENDER.md; DESIGN.md "Rendering"): world poses of all bodies, and RGB / depth / segmentation
// frames of selected envs.  Both only READ the environment state; ss_api.hip validates the arguments and calls the launchers below.
#include <hip/hip_runtime.h>

#include "ss_render.hpp"

namespace ss {
namespace render {

static_assert(VisualWalker3D::count == kRobotPrims && VisualMike::count == kRobotPrims, "kRobotPrims");
static_assert(kPrims <= 32, "one cull bit per primitive");
constexpr int kThreads = kTile * kTile;
constexpr int kRgbWords = kTile * kTile * 3 / 4;      // a tile's RGB bytes as dwords: 16 rows x 12
constexpr int kSegWords = kTile * kTile / 4;          // ... and its segmentation bytes: 16 rows x 4

// One workgroup = one (env, 16 x 16 tile).  Wave 0 places the env's bodies, primitives and stones in LDS and culls the primitives
// against the tile; then every lane casts its pixel's primary (and shadow) ray; the tile's bytes are staged in LDS and leave as
// dwords (a pixel row of RGB is 48 bytes = 12 dwords, W % 4 == 0 keeps every row start 4-byte aligned).
template <class Model, class Vis>
__global__ __launch_bounds__(kThreads) void render_kernel(Params P, const int32_t* env_ids, int W, int H, ss_camera cam,
                                                          unsigned char* rgb, float* depth, unsigned char* seg) {
  __shared__ float s_pose[kBodies * 12];
  __shared__ Prim s_prim[kPrims];
  __shared__ Cam s_cam;
  __shared__ int s_keep[kPrims];
  __shared__ uint32_t s_rgb[kRgbWords];
  __shared__ uint32_t s_seg[kSegWords];

  const int t = threadIdx.x;
  const int m = blockIdx.x;
  const int tiles_x = (W + kTile - 1) / kTile;
  const int i0 = (int)(blockIdx.y / tiles_x) * kTile, j0 = (int)(blockIdx.y % tiles_x) * kTile;
  const int i1 = min(i0 + kTile, H), j1 = min(j0 + kTile, W);
  const int e = env_ids[m];
  const bool valid = e >= 0 && e < P.n;          // an id outside [0, N) is drawn as background and reads no state

  if (valid && t < kBodies) body_pose<Model>(P, e, t, &s_pose[12 * t]);
  if (valid && t >= 32 && t < 32 + kStones) stone_prim(P, e, t - 32, s_prim[kRobotPrims + t - 32]);
  if (t == 64) camera_setup(cam, P, e, valid, W, H, s_cam);
  __syncthreads();
  if (t < kRobotPrims) {
    bool keep = false;
    if (valid) {
      robot_prim<Vis>(t, s_pose, s_prim[t]);
      keep = prim_in_tile(s_prim[t], s_cam, i0, i1, j0, j1);
    }
    s_keep[t] = keep ? 1 : 0;
  } else if (t < kPrims) {
    s_keep[t] = valid ? 1 : 0;
  }
  __syncthreads();
  uint32_t mask = 0;
#pragma unroll
  for (int k = 0; k < kPrims; ++k) mask |= (uint32_t)s_keep[k] << k;

  const int li = t / kTile, lj = t % kTile;
  const int i = i0 + li, j = j0 + lj;
  if (i < H && j < W) {
    float c[3], dep;
    int sg;
    shade_pixel(s_prim, valid ? kPrims : 0, mask, s_cam, i, j, (cam.flags & 1) != 0, c, dep, sg);
    if (depth) depth[((size_t)m * H + i) * W + j] = dep;
    unsigned char* rb = reinterpret_cast<unsigned char*>(s_rgb) + li * kTile * 3 + lj * 3;
    rb[0] = to_u8(c[0]);
    rb[1] = to_u8(c[1]);
    rb[2] = to_u8(c[2]);
    reinterpret_cast<unsigned char*>(s_seg)[li * kTile + lj] = (unsigned char)sg;
  }
  __syncthreads();
  const int vw = j1 - j0;                       // valid columns of the tile: a multiple of 4
  if (rgb && t < kRgbWords) {
    const int row = t / (kTile * 3 / 4), w = t % (kTile * 3 / 4);
    if (i0 + row < H && w < vw * 3 / 4)
      reinterpret_cast<uint32_t*>(rgb + (((size_t)m * H + i0 + row) * W + j0) * 3)[w] = s_rgb[t];
  }
  if (seg && t < kSegWords) {
    const int row = t / (kTile / 4), w = t % (kTile / 4);
    if (i0 + row < H && w < vw / 4) reinterpret_cast<uint32_t*>(seg + ((size_t)m * H + i0 + row) * W + j0)[w] = s_seg[t];
  }
}

// out [N, 22, 12]: one lane per (env, body)
template <class Model>
__global__ __launch_bounds__(256) void body_poses_kernel(Params P, float* out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= P.n * kBodies) return;
  float o[12];
  body_pose<Model>(P, g / kBodies, g % kBodies, o);
  float4* dst = reinterpret_cast<float4*>(out + (size_t)g * 12);
  dst[0] = make_float4(o[0], o[1], o[2], o[3]);
  dst[1] = make_float4(o[4], o[5], o[6], o[7]);
  dst[2] = make_float4(o[8], o[9], o[10], o[11]);
}

}  // namespace render

// launchers called by ss_api.hip (arguments validated there)
hipError_t launch_render(const Params& P, int kind, const int32_t* env_ids, int m, int W, int H, const ss_camera& cam,
                         unsigned char* rgb, float* depth, unsigned char* seg, hipStream_t st) {
  using namespace render;
  const int tiles = ((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile);
  const dim3 grid(m, tiles);
  if (kind == SS_WALKER3D)
    hipLaunchKernelGGL((render_kernel<ModelWalker3D, VisualWalker3D>), grid, dim3(kThreads), 0, st, P, env_ids, W, H, cam, rgb, depth, seg);
  else
    hipLaunchKernelGGL((render_kernel<ModelMike, VisualMike>), grid, dim3(kThreads), 0, st, P, env_ids, W, H, cam, rgb, depth, seg);
  return hipGetLastError();
}

hipError_t launch_body_poses(const Params& P, int kind, float* out, hipStream_t st) {
  using namespace render;
  const dim3 grid((P.n * kBodies + 255) / 256);
  if (kind == SS_WALKER3D)
    hipLaunchKernelGGL((body_poses_kernel<ModelWalker3D>), grid, dim3(256), 0, st, P, out);
  else
    hipLaunchKernelGGL((body_poses_kernel<ModelMike>), grid, dim3(256), 0, st, P, out);
  return hipGetLastError();
}

}  // namespace ss
