// ss_render.hpp -- ray-cast renderer of the stepping-stone scene: the robot's primitives placed by forward kinematics of the packed state,
// the three active stones as their exact contact sets (docs/RENDER.md is the specification; tests/np_render.py restates it in numpy).
//
// Every per-body, per-primitive and per-pixel function is SSD (host and device): tests/host/render_host.cpp runs the same code on the CPU.
// The kernels (ss_render.hip) only READ the environment state (Params::fstate); they never write to it.
#pragma once
#include "ss_kernels.hpp"
#include "ss_visual_tables.hpp"

namespace ss {
namespace render {

constexpr int kBodies = NJ + 1;
constexpr int kRobotPrims = 17;                 // VisualWalker3D::count == VisualMike::count (static_assert in ss_render.hip)
constexpr int kStones = 3;
constexpr int kPrims = kRobotPrims + kStones;   // <= 32: one bit each in a tile's cull mask
constexpr int kTile = 16;                       // a workgroup draws a 16 x 16 pixel tile of one env
constexpr int kMaxChain = 8;                    // longest body -> root chain (hand: 0 -> 13 ... -> 21 is 5; leg: 0..8 is 8)
constexpr int kSegStone = 23;                   // segmentation id of stone slot 0 (n - 1); 24 = target n, 25 = n + 1
constexpr float kStoneThickness = 0.10f;        // PHYSICS.md 3.3: -0.10 < d < 0
constexpr float kShadowBias = 1e-3f;            // the shadow ray starts this far out along the surface normal
enum { kPrimCapsule = kVisCapsule, kPrimSphere = kVisSphere, kPrimSlabs = 2 };   // boxes and stones are both three-slab solids
enum { kModeTrack = 0, kModeChase = 1, kModeFixed = 2 };

// docs/RENDER.md section 3: albedo per mass group (model.MASS_GROUPS order) and per stone role; light, ambient, sky
SSD float group_albedo(int g, int c) {
  constexpr float tab[8][3] = {{0.80f, 0.45f, 0.25f}, {0.75f, 0.50f, 0.30f}, {0.70f, 0.42f, 0.28f}, {0.25f, 0.45f, 0.75f},
                               {0.30f, 0.58f, 0.82f}, {0.20f, 0.24f, 0.32f}, {0.85f, 0.66f, 0.35f}, {0.92f, 0.78f, 0.48f}};
  return tab[g][c];
}
SSD float stone_albedo(int slot, int c) {
  constexpr float other[3] = {0.58f, 0.57f, 0.53f}, target[3] = {0.86f, 0.32f, 0.28f};
  return slot == 1 ? target[c] : other[c];
}
constexpr float kLight[3] = {-0.32444284f, -0.48666426f, 0.81110711f};   // normalize(-0.4, -0.6, 1)
constexpr float kAmbient = 0.30f, kDiffuse = 0.70f;
constexpr float kHorizon[3] = {0.86f, 0.89f, 0.93f}, kZenith[3] = {0.32f, 0.52f, 0.82f};

// A primitive in world coordinates.  capsule: a = p0, b = p1, r; sphere: a = centre, r; slabs (box or stone): the points x with
// lo[k] < (x - a) . w[k] < hi[k] for k = 0, 1, 2 (w need not be unit).  bc / br: bounding sphere (culling; robot primitives only).
struct Prim {
  float a[3], b[3], r;
  float w[3][3], lo[3], hi[3];
  float bc[3], br;
  int type, seg, albedo;       // albedo: mass group 0..7, or 8 + stone slot
};

struct Cam {
  float eye[3], f[3], r[3], u[3];
  float kx, ky;                // tan(fov_y / 2) * W / H, tan(fov_y / 2)
  float far_m;
  int W, H;
};

SSD float dot3(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
SSD void cross3(const float a[3], const float b[3], float o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
SSD void normalize3(float v[3]) {
  float inv = 1.0f / sqrtf(dot3(v, v));
  v[0] *= inv; v[1] *= inv; v[2] *= inv;
}

// World pose of body b of env e (docs/RENDER.md 2; the frame convention of model.fk): out = position (3) | R row-major (9).  The lane walks
// its body's ancestor chain from the root, so the 22 bodies of an env are 22 independent lanes.  through(j, R) is called once per joint j
// of the chain, root first, with the world orientation R of the joint's PARENT body, before the joint moves the pose on to its child
// (ss_kinematics.hpp carries the twist along the chain with it; body_pose below passes nothing).
template <class Model, class Through>
SSD void walk_chain(const Params& P, int e, int b, float out[12], Through&& through) {
  const float* F = P.fstate + e;
  const size_t np = (size_t)P.npad;
  float quat[4], p[3], R[3][3];
  for (int i = 0; i < 3; ++i) p[i] = F[(F_POS + i) * np];
  for (int i = 0; i < 4; ++i) quat[i] = F[(F_QUAT + i) * np];
  quat_rot(quat, R);
  int chain[kMaxChain], depth = 0;
#pragma unroll 1
  for (int c = b; c != 0 && depth < kMaxChain; c = kParent[c - 1]) chain[depth++] = c;
#pragma unroll 1
  for (int k = depth - 1; k >= 0; --k) {
    const int j = chain[k] - 1;
    through(j, R);
    const float rj[3] = {Model::r[j][0], Model::r[j][1], Model::r[j][2]};
    for (int i = 0; i < 3; ++i) p[i] += R[i][0] * rj[0] + R[i][1] * rj[1] + R[i][2] * rj[2];
    float s, c;
    sincosf(F[(F_Q + j) * np], &s, &c);
    const int ax = kAxis[j], i1 = ax == 0 ? 1 : (ax == 1 ? 2 : 0), i2 = ax == 0 ? 2 : (ax == 1 ? 0 : 1);
    for (int i = 0; i < 3; ++i) {          // R <- R Rot(axis, q): columns i1, i2 turn
      const float c1 = R[i][i1], c2 = R[i][i2];
      R[i][i1] = c * c1 + s * c2;
      R[i][i2] = c * c2 - s * c1;
    }
  }
  for (int i = 0; i < 3; ++i) out[i] = p[i];
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) out[3 + 3 * i + k] = R[i][k];
}
template <class Model>
SSD void body_pose(const Params& P, int e, int b, float out[12]) {
  walk_chain<Model>(P, e, b, out, [](int, const float (&)[3][3]) {});
}

// robot primitive k, placed by the pose of its body (poses: [22][12] as body_pose writes them)
template <class Vis>
SSD void robot_prim(int k, const float* poses, Prim& o) {
  const float* T = poses + 12 * Vis::body[k];
  const float* R = T + 3;
  const float la[3] = {Vis::a[k][0], Vis::a[k][1], Vis::a[k][2]}, lb[3] = {Vis::b[k][0], Vis::b[k][1], Vis::b[k][2]};
  for (int i = 0; i < 3; ++i) o.a[i] = T[i] + R[3 * i] * la[0] + R[3 * i + 1] * la[1] + R[3 * i + 2] * la[2];
  o.r = Vis::r[k];
  o.seg = 1 + Vis::body[k];
  o.albedo = Vis::group[k];
  const int t = Vis::type[k];
  if (t == kVisCapsule) {
    o.type = kPrimCapsule;
    for (int i = 0; i < 3; ++i) o.b[i] = T[i] + R[3 * i] * lb[0] + R[3 * i + 1] * lb[1] + R[3 * i + 2] * lb[2];
    float d[3] = {o.b[0] - o.a[0], o.b[1] - o.a[1], o.b[2] - o.a[2]};
    for (int i = 0; i < 3; ++i) o.bc[i] = 0.5f * (o.a[i] + o.b[i]);
    o.br = 0.5f * sqrtf(dot3(d, d)) + o.r;
  } else if (t == kVisSphere) {
    o.type = kPrimSphere;
    for (int i = 0; i < 3; ++i) { o.b[i] = o.a[i]; o.bc[i] = o.a[i]; }
    o.br = o.r;
  } else {                                  // box: the slabs |(x - c) . e_k| < half_k along the box's world axes e_k = R[:, k]
    o.type = kPrimSlabs;
    for (int kk = 0; kk < 3; ++kk) {
      for (int i = 0; i < 3; ++i) o.w[kk][i] = R[3 * i + kk];
      o.lo[kk] = -lb[kk];
      o.hi[kk] = lb[kk];
    }
    for (int i = 0; i < 3; ++i) { o.b[i] = 0.f; o.bc[i] = o.a[i]; }
    o.br = sqrtf(dot3(lb, lb));
  }
}

// active stone slot sl (0: n-1, 1: n, 2: n+1) of env e: the contact set of PHYSICS.md 3.3, -0.10 < d < 0, |u| < a, |v| < b, with
// d = (x - s) . n, u = (x - s) . (h_u - (n . h_u) n), v = (x - s) . (h_v - (n . h_v) n), h_u = (cos phi, sin phi, 0), h_v = (-sin phi, cos phi, 0)
SSD void stone_prim(const Params& P, int e, int sl, Prim& o) {
  const float* F = P.fstate + e;
  const size_t np = (size_t)P.npad;
  float n[3];
  for (int i = 0; i < 3; ++i) { o.a[i] = F[(F_STONE + sl * 8 + i) * np]; n[i] = F[(F_STONE + sl * 8 + 3 + i) * np]; }
  const float ch = F[(F_HEAD + sl * 2) * np], sh = F[(F_HEAD + sl * 2 + 1) * np];
  const float hu[3] = {ch, sh, 0.f}, hv[3] = {-sh, ch, 0.f};
  const float nu = dot3(n, hu), nv = dot3(n, hv);
  for (int i = 0; i < 3; ++i) {
    o.w[0][i] = n[i];
    o.w[1][i] = hu[i] - nu * n[i];
    o.w[2][i] = hv[i] - nv * n[i];
    o.b[i] = 0.f;
    o.bc[i] = o.a[i];
  }
  o.lo[0] = -kStoneThickness; o.hi[0] = 0.f;
  o.lo[1] = -kStonePlankHalfLength; o.hi[1] = kStonePlankHalfLength;
  o.lo[2] = -kStonePlankHalfWidth; o.hi[2] = kStonePlankHalfWidth;
  o.r = 0.f;
  o.br = 0.f;                               // stones are never culled
  o.type = kPrimSlabs;
  o.seg = kSegStone + sl;
  o.albedo = 8 + sl;
}

// docs/RENDER.md 1: TRACK / CHASE follow the torso (offsets in eye / target; CHASE turns them by the torso's yaw), FIXED is in world
// coordinates.  An env id outside [0, N) is drawn as background: its camera is placed as if the torso were at the origin with yaw 0.
SSD void camera_setup(const ss_camera& c, const Params& P, int e, bool valid, int W, int H, Cam& o) {
  float tgt[3], eye[3];
  if (c.mode == kModeFixed) {
    for (int i = 0; i < 3; ++i) { tgt[i] = c.target[i]; eye[i] = c.eye[i]; }
  } else {
    float pos[3] = {0.f, 0.f, 0.f}, cy = 1.f, sy = 0.f;
    if (valid) {
      const float* F = P.fstate + e;
      const size_t np = (size_t)P.npad;
      for (int i = 0; i < 3; ++i) pos[i] = F[(F_POS + i) * np];
      if (c.mode == kModeChase) {
        const float w = F[F_QUAT * np], x = F[(F_QUAT + 1) * np], y = F[(F_QUAT + 2) * np], z = F[(F_QUAT + 3) * np];
        const float A = 1.f - 2.f * (y * y + z * z), B = 2.f * (w * z + x * y), n2 = A * A + B * B;
        if (n2 > 1e-30f) {
          const float inv = 1.0f / sqrtf(n2);
          cy = A * inv;
          sy = B * inv;
        }
      }
    }
    const float to[3] = {cy * c.target[0] - sy * c.target[1], sy * c.target[0] + cy * c.target[1], c.target[2]};
    const float eo[3] = {cy * c.eye[0] - sy * c.eye[1], sy * c.eye[0] + cy * c.eye[1], c.eye[2]};
    for (int i = 0; i < 3; ++i) { tgt[i] = pos[i] + to[i]; eye[i] = tgt[i] + eo[i]; }
  }
  for (int i = 0; i < 3; ++i) { o.eye[i] = eye[i]; o.f[i] = tgt[i] - eye[i]; }
  normalize3(o.f);
  const float up[3] = {0.f, 0.f, 1.f}, upx[3] = {1.f, 0.f, 0.f};
  cross3(o.f, up, o.r);
  if (dot3(o.r, o.r) < 1e-12f) cross3(o.f, upx, o.r);     // looking straight up or down
  normalize3(o.r);
  cross3(o.r, o.f, o.u);
  o.ky = tanf(0.5f * c.fov_y_deg * kDeg);
  o.kx = o.ky * (float)W / (float)H;
  o.far_m = c.far_m;
  o.W = W;
  o.H = H;
}

// conservative tile test: false only if the primitive's bounding sphere lies wholly outside the view wedge of pixel columns [j0, j1)
// and rows [i0, i1) (the wedge's four planes pass through the eye and the tile's outer pixel edges)
SSD bool prim_in_tile(const Prim& p, const Cam& c, int i0, int i1, int j0, int j1) {
  const float v[3] = {p.bc[0] - c.eye[0], p.bc[1] - c.eye[1], p.bc[2] - c.eye[2]};
  const float vf = dot3(v, c.f), vr = dot3(v, c.r), vu = dot3(v, c.u);
  const float rad = 1.001f * p.br + 1e-4f;
  const float sl = c.kx * (2.f * (float)j0 / (float)c.W - 1.f), sr = c.kx * (2.f * (float)j1 / (float)c.W - 1.f);
  const float st = c.ky * (1.f - 2.f * (float)i0 / (float)c.H), sb = c.ky * (1.f - 2.f * (float)i1 / (float)c.H);
  // plane normals N (not unit) in (f, r, u) coordinates; |N| = sqrt(1 + s^2)
  if (vr - sl * vf < -rad * sqrtf(1.f + sl * sl)) return false;
  if (sr * vf - vr < -rad * sqrtf(1.f + sr * sr)) return false;
  if (st * vf - vu < -rad * sqrtf(1.f + st * st)) return false;
  if (vu - sb * vf < -rad * sqrtf(1.f + sb * sb)) return false;
  return true;
}

// primary ray through the centre of pixel (i, j), row 0 at the top
SSD void pixel_ray(const Cam& c, int i, int j, float d[3]) {
  const float sx = 2.f * ((float)j + 0.5f) / (float)c.W - 1.f, sy = 1.f - 2.f * ((float)i + 0.5f) / (float)c.H;
  for (int k = 0; k < 3; ++k) d[k] = c.f[k] + sx * c.kx * c.r[k] + sy * c.ky * c.u[k];
  normalize3(d);
}

// Nearest entering intersection t > 0 of the ray o + t d (|d| = 1) with primitive p, or -1.  n (if not null): unit outward normal there.
// Spheres and capsules are intersected from the ray's point nearest to their bounding centre, o + t0 d with t0 = (bc - o) . d: the
// quadratics then see offsets of the primitive's own size instead of the camera distance (fp32 keeps depth to ~1e-6 relative).
SSD float intersect(const Prim& p, const float o[3], const float d[3], float* n) {
  if (p.type != kPrimSlabs) {
    const float t0 = (p.bc[0] - o[0]) * d[0] + (p.bc[1] - o[1]) * d[1] + (p.bc[2] - o[2]) * d[2];
    const float q[3] = {o[0] + t0 * d[0], o[1] + t0 * d[1], o[2] + t0 * d[2]};
    float t, cen[3];
    if (p.type == kPrimSphere) {
      const float oc[3] = {q[0] - p.a[0], q[1] - p.a[1], q[2] - p.a[2]};
      const float b = dot3(oc, d), c = dot3(oc, oc) - p.r * p.r, h = b * b - c;
      if (h < 0.f) return -1.f;
      t = t0 + (-b - sqrtf(h));
      if (!(t > 0.f)) return -1.f;
      for (int k = 0; k < 3; ++k) cen[k] = p.a[k];
    } else {
      const float ba[3] = {p.b[0] - p.a[0], p.b[1] - p.a[1], p.b[2] - p.a[2]};
      const float oa[3] = {q[0] - p.a[0], q[1] - p.a[1], q[2] - p.a[2]};
      const float baba = dot3(ba, ba), bard = dot3(ba, d), baoa = dot3(ba, oa), rdoa = dot3(d, oa), oaoa = dot3(oa, oa);
      const float A = baba - bard * bard, B = baba * rdoa - baoa * bard, C = baba * oaoa - baoa * baoa - p.r * p.r * baba;
      const float h = B * B - A * C;
      if (h < 0.f) return -1.f;
      const float ts = (-B - sqrtf(h)) / A;
      const float y = baoa + ts * bard;
      if (y > 0.f && y < baba) {                          // the cylinder's side
        t = t0 + ts;
        if (!(t > 0.f)) return -1.f;
        const float s = y / baba;
        for (int k = 0; k < 3; ++k) cen[k] = p.a[k] + s * ba[k];
      } else {                                            // a cap: the sphere at the end the side hit lies beyond
        const float* e = y <= 0.f ? p.a : p.b;
        const float oc[3] = {q[0] - e[0], q[1] - e[1], q[2] - e[2]};
        const float b2 = dot3(d, oc), c2 = dot3(oc, oc) - p.r * p.r, h2 = b2 * b2 - c2;
        if (!(h2 > 0.f)) return -1.f;
        t = t0 + (-b2 - sqrtf(h2));
        if (!(t > 0.f)) return -1.f;
        for (int k = 0; k < 3; ++k) cen[k] = e[k];
      }
    }
    if (n) {
      const float inv = 1.0f / p.r;
      for (int k = 0; k < 3; ++k) n[k] = (o[k] + t * d[k] - cen[k]) * inv;
    }
    return t;
  }
  // three slabs: the entering t is the largest of the per-slab entries, the leaving one the smallest exit
  const float oa[3] = {o[0] - p.a[0], o[1] - p.a[1], o[2] - p.a[2]};
  float tn = -3.0e38f, tf = 3.0e38f;
  int kn = 0;
  float sn = 1.f;
  for (int k = 0; k < 3; ++k) {
    const float den = dot3(d, p.w[k]);
    const float num = dot3(oa, p.w[k]);
    const float t1 = (p.lo[k] - num) / den, t2 = (p.hi[k] - num) / den;
    const float te = fminf(t1, t2), tx = fmaxf(t1, t2);
    if (te > tn) { tn = te; kn = k; sn = den > 0.f ? -1.f : 1.f; }
    tf = fminf(tf, tx);
  }
  if (!(tn <= tf) || !(tn > 0.f)) return -1.f;
  if (n) {
    const float inv = sn / sqrtf(dot3(p.w[kn], p.w[kn]));
    for (int k = 0; k < 3; ++k) n[k] = p.w[kn][k] * inv;
  }
  return tn;
}

SSD float albedo_of(int a, int c) { return a < 8 ? group_albedo(a, c) : stone_albedo(a - 8, c); }

// One pixel (docs/RENDER.md 3, 4): closest hit among the primitives whose bit is set in `mask` (robot first, then stones; the first of
// equal t wins), Lambert + ambient, the optional any-hit shadow ray against ALL primitives, sky otherwise.  rgb in [0, 1] before the u8
// conversion; depth = z-depth (t d . f) or far; seg = 0 (background), 1 + body, 23 + stone slot.
SSD void shade_pixel(const Prim* prims, int count, uint32_t mask, const Cam& c, int i, int j, bool shadows, float rgb[3], float& depth,
                     int& seg) {
  float d[3];
  pixel_ray(c, i, j, d);
  const float df = dot3(d, c.f);
  float best = 3.0e38f;
  int hit = -1;
#pragma unroll 1
  for (int k = 0; k < count; ++k) {
    if (!((mask >> k) & 1u)) continue;
    const float t = intersect(prims[k], c.eye, d, nullptr);
    if (t > 0.f && t < best && t * df < c.far_m) { best = t; hit = k; }
  }
  if (hit < 0) {
    const float s = fminf(fmaxf(0.5f + 0.5f * d[2], 0.f), 1.f);
    for (int k = 0; k < 3; ++k) rgb[k] = (1.f - s) * kHorizon[k] + s * kZenith[k];
    depth = c.far_m;
    seg = 0;
    return;
  }
  float n[3];
  const float t = intersect(prims[hit], c.eye, d, n);
  float x[3];
  for (int k = 0; k < 3; ++k) x[k] = c.eye[k] + t * d[k];
  const float nl = dot3(n, kLight);
  float lit = nl > 0.f ? nl : 0.f;
  if (shadows && lit > 0.f) {
    float so[3];
    for (int k = 0; k < 3; ++k) so[k] = x[k] + kShadowBias * n[k];
#pragma unroll 1
    for (int k = 0; k < count; ++k)
      if (intersect(prims[k], so, kLight, nullptr) > 0.f) { lit = 0.f; break; }
  }
  const int a = prims[hit].albedo;
  for (int k = 0; k < 3; ++k) rgb[k] = albedo_of(a, k) * (kAmbient + kDiffuse * lit);
  depth = t * df;
  seg = prims[hit].seg;
}

SSD unsigned char to_u8(float x) { return (unsigned char)floorf(fminf(fmaxf(x, 0.f), 1.f) * 255.f + 0.5f); }

}  // namespace render
}  // namespace ss
