// ss_policy.hpp -- the closed-loop look-ahead (docs/PHYSICS.md 14 "Branches under a policy"): look_row (ss_lookahead.hpp)
// with its actions computed between the control steps by a small frozen MLP, a[k,s] = f(o[k,s-1]) + offset[k,s], instead of read from a
// caller's sequence.  This file is the action source ActPolicy that look_row is instantiated with, the network's packed form, and f.
//
// Between two control steps the dynamic state is in LDS, nothing of a row is live in registers, and the wavefront's 32 observation rows
// stand back to back in LDS region A (look_row stages them for a policy whether or not obs was asked for): f is a chain of M = 32
// products.  On the device the workgroup has kWaves wavefronts: wavefront 0 runs look_row, the others only the MLP phases, and in a
// phase every wavefront takes the 32-column tiles t = wave, wave + kWaves, .. of each layer (v_mfma_f32_32x32x2_f32: exact f32, a fma
// chain over k in index order that starts from the bias, so a row's bits depend on its own observation alone -- not on the row's place
// in the wavefront, not on which wavefront computed a tile).  Activations ping-pong between two [width][32] blocks behind the Lds block,
// k-major (what the next layer's A operand reads without bank conflicts); a workgroup barrier stands between layers.  The host build
// (tests/host/lookahead_policy_host.cpp), whose lanes are threads, lets the right lane of each row evaluate the same chain in plain
// loops over the same packed words.
//
// The packed form (OPAQUE to callers; ss_policy_pack writes it): per layer the weights as the B operands of its MFMAs, then the biases.
// With Kp / Np the layer's input / output width rounded up (Kp: 64 for the first layer, the previous Np otherwise; Np: to 32), word
//     woff + (((n / 32) * (Kp / 8) + kk / 4) * 64 + (k & 1) * 32 + n % 32) * 4 + kk % 4,   kk = k / 2
// is W[n][k], zero where n or k is beyond the layer's own widths: one float4 per lane holds the lane's B values of four consecutive
// MFMAs, and a wavefront reads 1 KiB in one piece.  The padding needs no special case: a padded output is activation(0) = 0 for all
// four activations and meets zero weights in the next layer.
#pragma once
#include "ss_lookahead.hpp"

namespace ss {
namespace policy {

constexpr int kWaves = 4;                                              // wavefronts per workgroup: one per SIMD
constexpr int kBufWords = kEnvsPerWave * SS_POLICY_MAX_WIDTH;          // one activation block [256][32]
constexpr int kXWords = 2 * kBufWords;                                 // ping and pong
constexpr int kLdsWords = kLdsSlots * kWave * 4 + kXWords;             // the Lds block, then the activation blocks
static_assert(kLdsWords * 4 <= 160 * 1024, "one workgroup fits a CU's LDS");
static_assert(SS_OBS_DIM == 60 && NJ == 21 && SS_POLICY_MAX_WIDTH % 32 == 0, "the widths the packed form is laid out for");

struct Net {        // a valid ss_policy_desc with the padded widths and the offsets of the packed form
  int layers;
  int kin[SS_POLICY_MAX_LAYERS], nout[SS_POLICY_MAX_LAYERS];      // the layer's own widths
  int kp[SS_POLICY_MAX_LAYERS], np[SS_POLICY_MAX_LAYERS];         // padded
  int act[SS_POLICY_MAX_LAYERS];
  int woff[SS_POLICY_MAX_LAYERS], boff[SS_POLICY_MAX_LAYERS];
  int words;
};

// false: the description is not valid
SSD bool make_net(const ss_policy_desc* d, Net& net) {
  if (!d || d->layers < 1 || d->layers > SS_POLICY_MAX_LAYERS) return false;
  if (d->width[0] != SS_OBS_DIM || d->width[d->layers] != NJ) return false;
  int off = 0;
  net.layers = d->layers;
  for (int l = 0; l < SS_POLICY_MAX_LAYERS; ++l) {
    if (l >= d->layers) {
      net.kin[l] = net.nout[l] = net.kp[l] = net.np[l] = net.act[l] = net.woff[l] = net.boff[l] = 0;
      continue;
    }
    const int k = d->width[l], n = d->width[l + 1], a = d->activation[l];
    if (k < 1 || k > SS_POLICY_MAX_WIDTH || n < 1 || n > SS_POLICY_MAX_WIDTH) return false;
    if (a != SS_POLICY_IDENTITY && a != SS_POLICY_RELU && a != SS_POLICY_SOFTSIGN && a != SS_POLICY_TANH) return false;
    net.kin[l] = k;
    net.nout[l] = n;
    net.kp[l] = l == 0 ? 64 : net.np[l - 1];
    net.np[l] = (n + 31) / 32 * 32;
    net.act[l] = a;
    net.woff[l] = off;
    off += net.np[l] * net.kp[l];
    net.boff[l] = off;
    off += net.np[l];
  }
  net.words = off;
  return true;
}

SSD int w_index(const Net& net, int l, int n, int k) {
  const int kk = k >> 1;
  return net.woff[l] + ((((n >> 5) * (net.kp[l] >> 3) + (kk >> 2)) * 64 + (k & 1) * 32 + (n & 31)) << 2) + (kk & 3);
}

// word i of the packed form, from the layers' own arrays (weight[l]: [nout, kin] row-major)
struct Arrays { const float* weight[SS_POLICY_MAX_LAYERS]; const float* bias[SS_POLICY_MAX_LAYERS]; };
SSD float packed_word(const Net& net, const Arrays& A, int i) {
  int l = 0;
  while (l + 1 < net.layers && i >= net.woff[l + 1]) ++l;
  if (i >= net.boff[l]) {
    const int n = i - net.boff[l];
    return n < net.nout[l] ? A.bias[l][n] : 0.f;
  }
  const int w = i - net.woff[l];
  const int j = w & 3, ln = (w >> 2) & 63, g = w >> 8, kp8 = net.kp[l] >> 3;
  const int n = (g / kp8) * 32 + (ln & 31), k = 2 * (4 * (g % kp8) + j) + (ln >> 5);
  return (n < net.nout[l] && k < net.kin[l]) ? A.weight[l][(size_t)n * net.kin[l] + k] : 0.f;
}

SSD float activate(int a, float x) {
  if (a == SS_POLICY_RELU) return x < 0.f ? 0.f : x;          // (a NaN stays a NaN)
  if (a == SS_POLICY_SOFTSIGN) return x / (1.f + fabsf(x));
  if (a == SS_POLICY_TANH) return tanhf(x);
  return x;
}

// f of one row in plain loops: x [60] -> y [32] (the first 21 are the action); t0, t1: SS_POLICY_MAX_WIDTH words each.  The sums are
// the fma chains of the matrix instruction: from the bias, over k in index order.
SSD void eval_row(const Net& net, const float* packed, const float* x, float* y, float* t0, float* t1) {
  const float* in = x;
  for (int l = 0; l < net.layers; ++l) {
    float* o = l == net.layers - 1 ? y : ((l & 1) ? t1 : t0);
    const int kn = l == 0 ? SS_OBS_DIM : net.kp[l];
    for (int n = 0; n < net.np[l]; ++n) {
      float s = packed[net.boff[l] + n];
      for (int k = 0; k < kn; ++k) s = fmaf(in[k], packed[w_index(net, l, n, k)], s);
      o[n] = activate(net.act[l], s);
    }
    in = o;
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
typedef float f32x16 __attribute__((ext_vector_type(16)));

// One MLP phase of this wavefront: the staged rows lds[32][60] -> the action tile.  Every wavefront of the workgroup calls it, and
// every call passes 1 + layers workgroup barriers.
__device__ __forceinline__ void mlp_phase(const Net& net, const float* __restrict__ packed, const float* lds, float* xb, int wave, int lane) {
  const int r = lane & 31, h = lane >> 5;
  __syncthreads();                                   // the staged rows are written, the last phase's tile is read
#pragma unroll 1
  for (int l = 0; l < net.layers; ++l) {
    const float* in = xb + ((l - 1) & 1) * kBufWords + h * 32 + r;                     // (l >= 1) A[row r][k]: word k * 32 + r
    float* ob = xb + (l & 1) * kBufWords;
    const int kp8 = net.kp[l] >> 3, tiles = net.np[l] >> 5, a = net.act[l];
#pragma unroll 1
    for (int t = wave; t < tiles; t += kWaves) {
      const float b = packed[net.boff[l] + t * 32 + r];
      f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = b;
      const float4* w4 = reinterpret_cast<const float4*>(packed + net.woff[l]) + (size_t)t * kp8 * 64 + lane;
      // Every load stands a group of 16 MFMAs (1024 cycles) ahead of its use: a wavefront has one accumulator chain and nothing else
      // to do, so a load waited for where it is issued costs its whole L2 latency (measured: 84 us per step that way, 2.8 x the MFMAs).
      if (l == 0) {                                  // the observation rows: row major, 60 wide; k = 60 .. 63 are zeros against zero weights
        const float* o = lds + r * SS_OBS_DIM + h;
        float4 w[8];
        float av[32];
#pragma unroll
        for (int k4 = 0; k4 < 8; ++k4) w[k4] = w4[k4 * 64];
#pragma unroll
        for (int kk = 0; kk < 32; ++kk) av[kk] = 2 * kk < SS_OBS_DIM ? o[2 * kk] : 0.f;
        __builtin_amdgcn_sched_barrier(0);           // (left alone, the scheduler moves every load down to its use)
#pragma unroll
        for (int k4 = 0; k4 < 8; ++k4) {
          const float wv[4] = {w[k4].x, w[k4].y, w[k4].z, w[k4].w};
#pragma unroll
          for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[4 * k4 + j], wv[j], acc, 0, 0, 0);
        }
      } else {
        float4 w[4], wn[4];
        float av[16], an[16];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = w4[i * 64];
#pragma unroll
        for (int i = 0; i < 16; ++i) av[i] = in[i * 64];
        const int groups = kp8 >> 2;                 // (kp8 is a multiple of 4: Kp is a multiple of 32 behind the first layer)
#pragma unroll 1
        for (int g = 0; g < groups; ++g) {
          const int gn = g + 1 < groups ? g + 1 : g; // (the last group once more instead of a branch: inside the layer's words)
#pragma unroll
          for (int i = 0; i < 4; ++i) wn[i] = w4[(4 * gn + i) * 64];
#pragma unroll
          for (int i = 0; i < 16; ++i) an[i] = in[(16 * gn + i) * 64];
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float wv[4] = {w[i].x, w[i].y, w[i].z, w[i].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[4 * i + j], wv[j], acc, 0, 0, 0);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < 4; ++i) w[i] = wn[i];
#pragma unroll
          for (int i = 0; i < 16; ++i) av[i] = an[i];
        }
      }
      // acc[4 g + i] is row 8 g + 4 h + i of column r of the tile: four float4 of the k-major block
      float4* o4 = reinterpret_cast<float4*>(ob + (t * 32 + r) * 32 + 4 * h);
#pragma unroll
      for (int g = 0; g < 4; ++g)
        o4[2 * g] = make_float4(activate(a, acc[4 * g]), activate(a, acc[4 * g + 1]), activate(a, acc[4 * g + 2]), activate(a, acc[4 * g + 3]));
    }
    __syncthreads();
  }
}
#endif

// The action source of look_row.  xb: the two activation blocks (device: behind the Lds block; host: the wavefront's own memory).
struct ActPolicy {
  static constexpr bool kPolicy = true;
  const Net& net;
  const float* packed;
  const float* offset;       // [m, H, 21] or null
  float* act;                // [m, H, 21] or null
  float* xb;
  int wave;                  // this wavefront in its workgroup

  SSD float* tile() const { return xb + ((net.layers - 1) & 1) * kBufWords; }      // [21 (of 32)][32 rows]: the last layer's block

  // the observation at the root: obs_kernel's / obs_states_kernel's body, by the row's right lane, into the row's staged place
  template <class Model, bool ROWS>
  SSD void root_obs(const Params& P, int e, const float* states, int row, int lane, float* lds) const {
    if (lane & 1) return;
    float o[SS_OBS_DIM];
    if constexpr (ROWS) {
      look::obs_from_row<Model>(states + (size_t)row * SS_STATE_DIM, o);
    } else {
      const size_t np = (size_t)P.npad;
      Dyn s;
      Cache c;
      load_dyn(P, e, s);
      load_cache(P, e, c);
      write_obs<Model>(s, P.fstate[e + F_ZINIT * np], P.istate[e + I_FLAGS * np], c, o);
    }
    float* stage = lds + (lane >> 1) * SS_OBS_DIM;
#pragma unroll
    for (int i = 0; i < SS_OBS_DIM; ++i) stage[i] = o[i];
  }

  SSD void phase(float* lds, int lane) const {
#if defined(__HIP_DEVICE_COMPILE__)
    mlp_phase(net, packed, lds, xb, wave, lane);
#else
    SS_WAVE_SYNC();
    if (!(lane & 1)) {
      float y[32], t0[SS_POLICY_MAX_WIDTH], t1[SS_POLICY_MAX_WIDTH];
      eval_row(net, packed, lds + (lane >> 1) * SS_OBS_DIM, y, t0, t1);
      for (int i = 0; i < NJ; ++i) tile()[i * 32 + (lane >> 1)] = y[i];
    }
    SS_WAVE_SYNC();
#endif
  }

  // a = f(o) + offset, by the row's right lane: back into the tile for load(), and reported (a finished branch reports zeros)
  SSD void emit(int row, int H, int s, int lane, bool valid, bool live) const {
    if (!(lane & 1)) {
      float* t = tile() + (lane >> 1);
      const size_t at = ((size_t)row * (size_t)H + (size_t)s) * NJ;
#pragma unroll 1
      for (int i = 0; i < NJ; ++i) {
        float v = t[i * 32];
        if (offset) v += offset[at + i];
        t[i * 32] = v;
        if (valid && act) act[at + i] = live ? v : 0.f;
      }
    }
    SS_WAVE_SYNC();
  }

  // load_actions from the tile
  SSD void load(int lane, int side, float (&ain)[NH]) const {
    const float* t = tile() + (lane >> 1);
    static_for<0, NH>([&](auto Kc) {
      constexpr int k = decltype(Kc)::value, jr = kHalf[k];
      constexpr int jl = left_twin(jr);
      ain[k] = t[(side ? jl : jr) * 32];
    });
  }
};

}  // namespace policy
}  // namespace ss
