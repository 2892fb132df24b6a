// s2d_actor_net.h -- the 10-H1-H2-A network of the reach-ball engine's fused actors, shared by s2d_actor.hip (the Q-network and
// the tanh actor) and s2d_policy.hip (the stochastic policy heads): its dimensions, the repacking of the caller's parameters
// into fragment order, the forward pass on the wave's observation tile and the LDS plan.  (Moved out of s2d_actor.hip unchanged.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "s2d_kernels.h"
#include "s2d_net.h"

struct QNetDims {
  int h1, h2, na;        // hidden widths (multiples of 16, 16 .. 128), actions (1 .. 64)
  int na16;              // actions rounded up to 16 (rows of layer 3's tiles; the padding rows have zero weights and bias)
  int pitch;             // LDS row pitch of the hidden-activation images (words): max width rounded up to 64, + 4
  int qpitch;            // LDS row pitch of the Q-value image: na16 + 4
};
// LDS layout, in floats: [W1 frags | W2 frags | W3 frags | b1 | b2 | b3 (na16)] shared by the block, then per wave
// [hA 16 x pitch | hB 16 x pitch | q 64 x qpitch | obs tile 640 | PrepTile]
S2D_DEV int w1_frags(const QNetDims& d) { return (d.h1 / 16) * 3; }
S2D_DEV int w2_frags(const QNetDims& d) { return (d.h2 / 16) * (d.h1 / 4); }
S2D_DEV int w3_frags(const QNetDims& d) { return (d.na16 / 16) * (d.h2 / 4); }

// the network on the observation tile of the wave (lane = env): qv[env][j] (pitch d.qpitch) = the output layer's
// pre-activations y_j; ARGMAX: then the spec's argmax scan, whose result is returned (the Q-actor's greedy action)
template <bool ARGMAX>
S2D_DEV int net_forward(const QNetDims& d, const float* __restrict__ wl, float* __restrict__ ha, float* __restrict__ hb,
                        float* __restrict__ qv, const float* __restrict__ obs_tile, int lane) {
  const int g = lane >> 4, c = lane & 15;
  const float* w1 = wl;
  const float* w2 = w1 + w1_frags(d) * kWave;
  const float* w3 = w2 + w2_frags(d) * kWave;
  const float* b1 = w3 + w3_frags(d) * kWave;
  const float* b2 = b1 + d.h1;
  const float* b3 = b2 + d.h2;
  for (int nt = 0; nt < 4; ++nt) {
    const float* x = obs_tile + (16 * nt + c) * S2D_OBS_DIM;
    layer_tile<true, 3>(w1, b1, d.h1 / 16, 3, [&](int s) { const int k = 4 * s + g; return k < S2D_OBS_DIM ? x[k] : 0.0f; },
                     ha, d.pitch, lane);
    wave_lds_fence();
    layer_tile<true, 4>(w2, b2, d.h2 / 16, d.h1 / 4, [&](int s) { return ha[c * d.pitch + 4 * s + g]; }, hb, d.pitch, lane);
    wave_lds_fence();
    layer_tile<false, 4>(w3, b3, d.na16 / 16, d.h2 / 4, [&](int s) { return hb[c * d.pitch + 4 * s + g]; },
                      qv + 16 * nt * d.qpitch, d.qpitch, lane);
    wave_lds_fence();
  }
  if constexpr (!ARGMAX) return 0;
  // best = 0; for a = 1 .. A-1: if (q[a] > q[best]) best = a   (ties: lowest index; a NaN never replaces the best)
  const float* q = qv + lane * d.qpitch;
  int best = 0;
  float bv = q[0];
  for (int a = 1; a < d.na; ++a) {
    const float v = q[a];
    if (v > bv) { bv = v; best = a; }
  }
  wave_lds_fence();
  return best;
}

// the caller's parameters (nn.Sequential order: W1 [h1][10], b1, W2 [h2][h1], b2, W3 [na][h2], b3) into the block's LDS in
// fragment order, then b1 | b2 | b3 padded with zeros to na16 (block-wide: every thread of the block takes part)
S2D_DEV void net_pack(const QNetDims& d, const float* __restrict__ params, float* __restrict__ smem) {
  const int f1 = w1_frags(d), f2 = w2_frags(d), f3 = w3_frags(d);
  const int nfrag = f1 + f2 + f3;
  const int o_b1 = 10 * d.h1, o_w2 = o_b1 + d.h1, o_b2 = o_w2 + d.h2 * d.h1, o_w3 = o_b2 + d.h2, o_b3 = o_w3 + d.na * d.h2;
  for (int idx = threadIdx.x; idx < nfrag * kWave; idx += blockDim.x) {
    const int f = idx / kWave, l = idx & (kWave - 1);
    const int row = l & 15, kk = l >> 4;
    float v = 0.0f;
    if (f < f1) {
      const int jt = f / 3, s = f - 3 * jt, k = 4 * s + kk;
      if (k < S2D_OBS_DIM) v = params[(16 * jt + row) * S2D_OBS_DIM + k];
    } else if (f < f1 + f2) {
      const int g2 = f - f1, ks = d.h1 / 4, jt = g2 / ks, s = g2 - jt * ks;
      v = params[o_w2 + (16 * jt + row) * d.h1 + 4 * s + kk];
    } else {
      const int g3 = f - f1 - f2, ks = d.h2 / 4, jt = g3 / ks, s = g3 - jt * ks, j = 16 * jt + row;
      if (j < d.na) v = params[o_w3 + j * d.h2 + 4 * s + kk];
    }
    smem[idx] = v;
  }
  float* const bias = smem + nfrag * kWave;
  for (int j = threadIdx.x; j < d.h1 + d.h2 + d.na16; j += blockDim.x) {
    float v;
    if (j < d.h1) v = params[o_b1 + j];
    else if (j < d.h1 + d.h2) v = params[o_b2 + j - d.h1];
    else v = (j - d.h1 - d.h2 < d.na) ? params[o_b3 + j - d.h1 - d.h2] : 0.0f;
    bias[j] = v;
  }
}
// words of the block-shared part of the LDS (fragments and biases, rounded up to 16 bytes); the waves' parts follow
S2D_DEV int net_shared_words(const QNetDims& d) {
  return ((w1_frags(d) + w2_frags(d) + w3_frags(d)) * kWave + d.h1 + d.h2 + d.na16 + 3) & ~3;
}

// host side
static constexpr size_t kLdsMax = 160 * 1024;   // gfx950: LDS of a CU, all of it available to one workgroup
static constexpr int kMaxDevices = 64;

// the LDS plan of a 10-h1-h2-na network: dims, per-wave words and the wave count per workgroup (as many as the LDS holds, 4 for
// 10-64-64-16); false if one wave does not fit
static inline bool plan_lds(int h1, int h2, int na, QNetDims& d, int& wave_words, int& waves, size_t& lds) {
  d.h1 = h1; d.h2 = h2; d.na = na; d.na16 = (na + 15) / 16 * 16;
  const int wmax = h1 > h2 ? h1 : h2;
  d.pitch = (wmax + 63) / 64 * 64 + 4;
  d.qpitch = d.na16 + 4;
  const int nfrag = (h1 / 16) * 3 + (h2 / 16) * (h1 / 4) + (d.na16 / 16) * (h2 / 4);
  const size_t shared_words = ((size_t)nfrag * kWave + h1 + h2 + d.na16 + 3) & ~(size_t)3;
  wave_words = 2 * 16 * d.pitch + kWave * d.qpitch + kObsTile + (int)(sizeof(PrepTile) / sizeof(float));
  waves = kWavesPerBlock;
  while (waves > 1 && (shared_words + (size_t)waves * wave_words) * sizeof(float) > kLdsMax) waves /= 2;
  lds = (shared_words + (size_t)waves * wave_words) * sizeof(float);
  return lds <= kLdsMax;
}
