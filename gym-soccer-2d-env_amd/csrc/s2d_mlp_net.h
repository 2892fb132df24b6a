// s2d_mlp_net.h -- the general MLP of the reach-ball engine's fused actors (s2d_mlp_actor.hip; include/s2d.h S2DMlpNet, DESIGN.md
// section 4): 10 -> h_1 -> ... -> h_L -> A with one to four hidden layers, every hidden width a multiple of 8 in [8, 128], one
// hidden activation for the whole network (relu or tanh_spec) and a linear output layer.  Its dimensions, the LDS plan, the
// repacking of the caller's parameters into fragment order and the forward pass on the wave's observation tile, built on
// layer_group of s2d_net.h (one layer on v_mfma_f32_16x16x4_f32, bit for bit a k-ordered fmaf chain).
//
// Every unit is acc = b[j]; for k ascending: acc = fmaf(W[j][k], in[k], acc).  Layer 1 runs over k = 0 .. 11 with x_10 = x_11 = 0
// against zero weights (two fmaf(0, 0, acc): an accumulator of -0 becomes +0, visible through tanh_spec).  Layers 2 .. L and
// the output layer run over exactly k = 0 .. h_(l-1) - 1: a width that is a multiple of 8 but not of 16 pads the OUTPUT ROWS of
// its last tile with zero weights and bias, and the next layer's k-steps stop at h / 4, so no padded unit is ever read and no
// extra fmaf enters a chain.
//
// LDS, in floats: [layer 1 frags | ... | layer L frags | output frags | b_1 | ... | b_L | b_out, each padded to its tiles' 16 rows]
// shared by the block, then per wave [hA 16 x pitch | hB 16 x pitch | q 64 x qpitch | obs tile 640 | PrepTile], as the
// two-layer actors'.  Layer l's fragments are tile-major: fragment (jt, s) = 64 words, lane l holds W[16 jt + (l & 15)][4 s + (l >> 4)].
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "s2d_actor_net.h"

static constexpr int kMlpMaxHidden = 4;

struct MlpDims {
  int n_hidden;              // L, 1 .. 4
  int act;                   // hidden activation: 0 relu, 1 tanh_spec
  uint32_t widths;           // the hidden widths (multiples of 8, 8 .. 128), h_l in byte l - 1; 0 past L
  int na;                    // outputs (1 .. 64)
  int na16;                  // outputs rounded up to 16 (rows of the output layer's tiles)
  int nfrag;                 // fragments in all (layers 1 .. L, then the output layer); the bias block follows them
  int nbias;                 // words of the bias block: every layer's width rounded up to 16
  int pitch;                 // LDS row pitch of the hidden images (words): the widest layer's tiles, rounded up to 64, + 4
  int qpitch;                // LDS row pitch of the output image: na16 + 4
};
// The widths are bytes of one word, and a layer's first fragment is summed up on the way through the layers, rather than
// arrays: the struct is a kernel argument, and an array in it indexed by the layer would be copied to scratch.
// hidden width h_(l + 1), l = 0 .. 3
S2D_DEV int mlp_width(const MlpDims& d, int l) { return (int)((d.widths >> (8 * l)) & 255u); }
S2D_DEV int net_shared_words(const MlpDims& d) { return (d.nfrag * kWave + d.nbias + 3) & ~3; }

// J output tiles of one layer whose k-step count is only known to be even (a width that is a multiple of 8): layer_group's
// chain with its k-steps in groups of four and, where ksteps is not a multiple of four, one last group of two.  The order of
// the k-steps, and so every bit, is layer_group's.
template <int ACT, int J, typename InFrag>
S2D_DEV void layer_group_even(const float* __restrict__ wf, const float* __restrict__ bias, int jt0, int ksteps, InFrag in_frag,
                              float* __restrict__ out, int op, int lane) {
  const int g = lane >> 4, c = lane & 15;
  v4f_t acc[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const float4 b4 = *reinterpret_cast<const float4*>(bias + 16 * (jt0 + j) + 4 * g);
    acc[j] = v4f_t{b4.x, b4.y, b4.z, b4.w};
  }
  int s0 = 0;
  for (; s0 + 4 <= ksteps; s0 += 4) {
    float b[4], w[J][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      b[u] = in_frag(s0 + u);
#pragma unroll
      for (int j = 0; j < J; ++j) w[j][u] = wf[((jt0 + j) * ksteps + s0 + u) * kWave + lane];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int j = 0; j < J; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j][u], b[u], acc[j], 0, 0, 0);
    }
  }
  if (s0 < ksteps) {                                       // ksteps = 4 m + 2
    float b[2], w[J][2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      b[u] = in_frag(s0 + u);
#pragma unroll
      for (int j = 0; j < J; ++j) w[j][u] = wf[((jt0 + j) * ksteps + s0 + u) * kWave + lane];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int j = 0; j < J; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j][u], b[u], acc[j], 0, 0, 0);
    }
  }
#pragma unroll
  for (int j = 0; j < J; ++j) {
    if (ACT == S2D_ACT_FN_RELU) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[j][r] = acc[j][r] > 0.0f ? acc[j][r] : 0.0f;   // relu: NaN and -0 -> +0
    } else if (ACT == S2D_ACT_FN_TANH) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[j][r] = tanh_spec(acc[j][r]);
    }
    *reinterpret_cast<float4*>(out + c * op + 16 * (jt0 + j) + 4 * g) = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
  }
}
// all m16 output tiles of such a layer, four (then two, then one) at a time
template <int ACT, typename InFrag>
S2D_DEV void layer_tile_even(const float* __restrict__ wf, const float* __restrict__ bias, int m16, int ksteps, InFrag in_frag,
                             float* __restrict__ out, int op, int lane) {
  int jt = 0;
  for (; jt + 4 <= m16; jt += 4) layer_group_even<ACT, 4>(wf, bias, jt, ksteps, in_frag, out, op, lane);
  if (jt + 2 <= m16) { layer_group_even<ACT, 2>(wf, bias, jt, ksteps, in_frag, out, op, lane); jt += 2; }
  if (jt < m16) layer_group_even<ACT, 1>(wf, bias, jt, ksteps, in_frag, out, op, lane);
}

// the layers on the wave's observation tile with hidden activation ACT, ping-ponging between the wave's two hidden images:
// layer 1 reads the observation tile, the output layer writes into the output image qv[env][j] (pitch d.qpitch)
template <int ACT>
S2D_DEV void mlp_layers(const MlpDims& d, const float* __restrict__ wl, float* __restrict__ ha, float* __restrict__ hb,
                        float* __restrict__ qv, const float* __restrict__ obs_tile, int lane) {
  const int g = lane >> 4, c = lane & 15;
  const float* const bias0 = wl + d.nfrag * kWave;
  for (int nt = 0; nt < 4; ++nt) {
    const float* x = obs_tile + (16 * nt + c) * S2D_OBS_DIM;
    const float* bias = bias0;
    int hin = mlp_width(d, 0), m16 = (hin + 15) >> 4, frag = 3 * m16;
    layer_tile<ACT, 3>(wl, bias, m16, 3, [&](int s) { const int k = 4 * s + g; return k < S2D_OBS_DIM ? x[k] : 0.0f; }, ha, d.pitch,
                       lane);
    wave_lds_fence();
    bias += 16 * m16;
    float* in = ha;
    float* out = hb;
    for (int l = 1; l < d.n_hidden; ++l) {
      const float* const src = in;
      m16 = (mlp_width(d, l) + 15) >> 4;
      layer_tile_even<ACT>(wl + frag * kWave, bias, m16, hin >> 2, [&](int s) { return src[c * d.pitch + 4 * s + g]; }, out, d.pitch,
                           lane);
      wave_lds_fence();
      bias += 16 * m16;
      frag += m16 * (hin >> 2);
      hin = mlp_width(d, l);
      float* const swap = in; in = out; out = swap;
    }
    const float* const src = in;
    layer_tile_even<S2D_ACT_FN_NONE>(wl + frag * kWave, bias, d.na16 >> 4, hin >> 2,
                                     [&](int s) { return src[c * d.pitch + 4 * s + g]; }, qv + 16 * nt * d.qpitch, d.qpitch, lane);
    wave_lds_fence();
  }
}

// the network on the observation tile of the wave (lane = env): qv[env][j] = the output layer's pre-activations y_j; d.act is
// wave-uniform and both forms are compiled into every kernel, so the activation does not multiply the instantiations; ARGMAX:
// then the argmax scan of the two-layer net_forward, whose result is returned (the Q-actor's greedy action).  (net_forward,
// net_pack and net_shared_words are overloads of s2d_actor_net.h's on MlpDims: what the rollout kernel of
// s2d_actor_rollout.h asks of its network.)
template <bool ARGMAX>
S2D_DEV int net_forward(const MlpDims& d, const float* __restrict__ wl, float* __restrict__ ha, float* __restrict__ hb,
                        float* __restrict__ qv, const float* __restrict__ obs_tile, int lane) {
  if (d.act) mlp_layers<S2D_ACT_FN_TANH>(d, wl, ha, hb, qv, obs_tile, lane);
  else mlp_layers<S2D_ACT_FN_RELU>(d, wl, ha, hb, qv, obs_tile, lane);
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

// the caller's parameters (nn.Sequential order: W_1 [h_1][10], b_1, ..., W_L [h_L][h_(L-1)], b_L, W_out [A][h_L], b_out) into the
// block's LDS in fragment order, then the biases, every layer's padded with zeros to its tiles' 16 rows (block-wide: every
// thread of the block takes part).  Rows past a layer's width and layer 1's k = 10, 11 are zero.
S2D_DEV void net_pack(const MlpDims& d, const float* __restrict__ params, float* __restrict__ smem) {
  const int L = d.n_hidden;
  for (int idx = threadIdx.x; idx < d.nfrag * kWave; idx += blockDim.x) {
    const int f = idx / kWave, lw = idx & (kWave - 1);
    const int row = lw & 15, kk = lw >> 4;
    // the layer of fragment f: its first fragment, widths in and out, k-steps and the offset of its W in params
    int f0 = 0, win = S2D_OBS_DIM, wout = mlp_width(d, 0), ks = 3, ow = 0;
#pragma unroll
    for (int l = 1; l <= kMlpMaxHidden; ++l) {
      const int next = f0 + ((wout + 15) >> 4) * ks;       // the first fragment of the layer after this one
      if (l <= L && f >= next) {
        ow += wout * win + wout;
        f0 = next;
        win = wout;
        wout = l < L ? mlp_width(d, l) : d.na;
        ks = win >> 2;
      }
    }
    const int r = f - f0, jt = r / ks, s = r - jt * ks, j = 16 * jt + row, k = 4 * s + kk;
    smem[idx] = (j < wout && k < win) ? params[ow + j * win + k] : 0.0f;
  }
  float* const bias = smem + d.nfrag * kWave;
  for (int idx = threadIdx.x; idx < d.nbias; idx += blockDim.x) {
    int b0 = 0, win = S2D_OBS_DIM, wout = mlp_width(d, 0), ob = wout * win;     // ob: the offset of the layer's bias in params
#pragma unroll
    for (int l = 1; l <= kMlpMaxHidden; ++l) {
      const int pad = (wout + 15) & ~15;
      if (l <= L && idx >= b0 + pad) {
        b0 += pad;
        win = wout;
        wout = l < L ? mlp_width(d, l) : d.na;
        ob += win + wout * win;
      }
    }
    const int j = idx - b0;
    bias[idx] = j < wout ? params[ob + j] : 0.0f;
  }
}

// host side
// is (n_hidden, hidden[]) on the grid: 1 .. 4 layers, every width a multiple of 8 in [8, 128], zeros past n_hidden
static inline bool mlp_shape_ok(int n_hidden, const int32_t* hidden) {
  if (n_hidden < 1 || n_hidden > kMlpMaxHidden) return false;
  for (int l = 0; l < kMlpMaxHidden; ++l) {
    const int w = hidden[l];
    if (l < n_hidden ? (w < 8 || w > 128 || w % 8 != 0) : w != 0) return false;
  }
  return true;
}

// the LDS plan of a valid shape: dims, per-wave words, the wave count per workgroup (as many of 4 / 2 / 1 as the LDS holds)
// and the bytes that count needs (one wave's if even that does not fit); false if one wave does not fit
static inline bool mlp_plan_lds(int n_hidden, const int32_t* hidden, int na, int act, MlpDims& d, int& wave_words, int& waves, size_t& lds) {
  d = MlpDims{};
  d.n_hidden = n_hidden; d.act = act; d.na = na; d.na16 = (na + 15) / 16 * 16;
  int nfrag = 0, nbias = 0, wmax = 0, ksteps = 3;
  for (int l = 0; l < n_hidden; ++l) {
    const int w = hidden[l], m16 = (w + 15) / 16;
    d.widths |= (uint32_t)w << (8 * l);
    nfrag += m16 * ksteps;
    nbias += 16 * m16;
    if (16 * m16 > wmax) wmax = 16 * m16;
    ksteps = w / 4;
  }
  nfrag += (d.na16 / 16) * ksteps;
  nbias += d.na16;
  d.nfrag = nfrag; d.nbias = nbias;
  d.pitch = (wmax + 63) / 64 * 64 + 4;
  d.qpitch = d.na16 + 4;
  const size_t shared_words = ((size_t)nfrag * kWave + nbias + 3) & ~(size_t)3;
  wave_words = 2 * 16 * d.pitch + kWave * d.qpitch + kObsTile + (int)(sizeof(PrepTile) / sizeof(float));
  waves = kWavesPerBlock;
  while (waves > 1 && (shared_words + (size_t)waves * wave_words) * sizeof(float) > kLdsMax) waves /= 2;
  lds = (shared_words + (size_t)waves * wave_words) * sizeof(float);
  return lds <= kLdsMax;
}
