// s2d_wide_net.h -- the streamed-weight MLP of the reach-ball engine's fused actors (s2d_wide_actor.hip; include/s2d.h S2DWideNet,
// DESIGN.md section 4): 10 -> h_1 -> ... -> h_L -> A with one to five hidden layers, every hidden width a multiple of 4 in
// [8, 400], one hidden activation for the whole network (relu, tanh_spec or sigmoid_spec) and a linear output layer.  The second
// network back end of the rollout template (s2d_actor_rollout.h): the spec is s2d_mlp_net.h's, the place of the weights is not.
//
// The weight fragments stay in GLOBAL memory (the caller's workspace, written by s2d_wide_pack.hip's pack kernel ahead of every
// launch that reads it; the shape's checks, the fragment count, the workspace and the (waves, tiles) search are s2d_wide_host.h's,
// shared with the TD targets of s2d_td.hip), in the resident path's MFMA fragment order: fragment (jt, s) = 64 words, lane l
// holds W[16 jt + (l & 15)][4 s + (l >> 4)], so a fragment load is one coalesced 256-byte wave access that the L2 serves ([400] * 5
// is 2.6 MB).  A wave loads a fragment once per pass and feeds it to the MFMAs of T = 4, 2 or 1 of its four 16-env tiles (one
// accumulator per (output tile, env tile)), with the next k-group's fragments requested ahead of the current group's MFMAs.  LDS
// holds only the biases (block-shared) and per wave
// [image A: T x 16 x rpitch | image B: T x 16 x rpitch | q 64 x qpitch | obs tile 640 | PrepTile].
//
// Every unit is acc = b[j]; for k ascending: acc = fmaf(W[j][k], in[k], acc): layer 1 over k = 0 .. 11 (x_10 = x_11 = 0 against zero
// weights), later layers over exactly h_(l-1) terms; a width that is no multiple of 16 pads the OUTPUT ROWS of its last tile and
// the next layer's k-steps stop at h / 4.  h / 4 may be odd: the k-steps go in groups of four, then one group of two, then one
// single step, in ascending order.  Neither T nor the waves per workgroup enters a chain: the bits do not depend on the plan.
//
// The input width is a compile-time parameter IN of the layers (S2D_OBS_DIM unless said): it is the observation tile's row
// stride and gives layer 1 its ceil(IN / 4) k-steps; the host side and the pack kernel take it as a run-time n_in, the pack
// kernel's first `win`.  The GoToCenter actors (s2d_gtc_actor.hip) use IN = 4: layer 1 is then ONE k-step over exactly
// k = 0 .. 3 with no zero pad, so an accumulator of -0 stays -0 there (the padded layer 1 of IN = 10 turns it into +0); a wave's
// LDS part ends with the observation tile of 64 x IN words and no PrepTile.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "s2d_actor_net.h"
#include "s2d_wide_host.h"

enum { S2D_WIDE_RELU = 0, S2D_WIDE_TANH = 1, S2D_WIDE_SIGMOID = 2, S2D_WIDE_LINEAR = 3 };

struct WideDims {
  int n_hidden;              // L, 1 .. 5
  int act;                   // hidden activation: 0 relu, 1 tanh_spec, 2 sigmoid_spec
  uint64_t widths;           // h_l / 4 (2 .. 100) in bits 7 (l - 1) .. 7 l - 1; 0 past L
  int na;                    // outputs (1 .. 64)
  int na16;                  // outputs rounded up to 16
  int nfrag;                 // fragments in all (layers 1 .. L, then the output layer); the bias block follows them in the workspace
  int nbias;                 // words of the bias block: every layer's width rounded up to 16
  int pitch;                 // what the rollout template steps its two images by: tiles * rpitch (hb = image B, qv behind it)
  int qpitch;                // LDS row pitch of the output image: na16 + 4
  int rpitch;                // LDS row pitch of a hidden image (words): the widest layer's tiles, rounded up to 64, + 4
  int tiles;                 // T: env tiles per pass, 4 | 2 | 1
  const float* wf;           // the workspace: nfrag fragments, then the bias block
};
// As MlpDims: no array indexed by the layer in a kernel argument (it would be copied to scratch); a layer's first fragment is
// summed up on the way through the layers.
S2D_DEV int wide_width(const WideDims& d, int l) { return 4 * (int)((d.widths >> (7 * l)) & 127u); }
S2D_DEV int net_shared_words(const WideDims& d) { return (d.nbias + 3) & ~3; }

// the activation of four units of one env (one float4 of an image)
S2D_DEV float4 wide_act4(int act, float4 v) {
  if (act == S2D_WIDE_TANH) return make_float4(tanh_spec(v.x), tanh_spec(v.y), tanh_spec(v.z), tanh_spec(v.w));
  return make_float4(sigmoid_spec(v.x), sigmoid_spec(v.y), sigmoid_spec(v.z), sigmoid_spec(v.w));
}

// J output tiles (jt0 .. jt0 + J - 1) of one layer for T env tiles at once: out[t][c][j] (image of T x 16 rows, pitch `op`, tile t at
// t * tstride) = act(b[j] + sum_k W[j][k] in[t][c][k]) for the 16 envs c of every tile.  wf = the layer's fragments in global
// memory; `in` = the input image (same tiling, pitch ip).  The chain of every accumulator is layer_group's: the k-steps in
// ascending order, in groups of four, then two, then one.  The fragments of the next group of four (or of the tail) are
// requested before the current group's MFMAs; a fragment is loaded once and used by all T env tiles.
// relu is applied on the accumulators; tanh_spec / sigmoid_spec by a rolled loop over the float4s this lane has just stored
// (the same lane, the same addresses: program order), so that their code exists once per instantiation and not J * T times.
template <int J, int T>
S2D_DEV void wide_group(const float* __restrict__ wf, const float* __restrict__ bias, int jt0, int ksteps, const float* __restrict__ in,
                        int ip, int itile, float* __restrict__ out, int op, int otile, int act, int lane) {
  const int g = lane >> 4, c = lane & 15;
  v4f_t acc[J][T];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const float4 b4 = *reinterpret_cast<const float4*>(bias + 16 * (jt0 + j) + 4 * g);
#pragma unroll
    for (int t = 0; t < T; ++t) acc[j][t] = v4f_t{b4.x, b4.y, b4.z, b4.w};
  }
  const float* const src = in + c * ip + g;
  const int last = ksteps - 1;
  float w[J][4], wn[J][4];
  // k-steps s0 .. s0 + 3 of the J tiles, the step clamped to the layer's last (a tail shorter than four reads its own steps first)
#define S2D_WIDE_LOAD(dst, s0)                                                                            \
  _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                                         \
    const int s_ = (s0) + u < last ? (s0) + u : last;                                                     \
    _Pragma("unroll") for (int j = 0; j < J; ++j) dst[j][u] = wf[((jt0 + j) * ksteps + s_) * kWave + lane]; \
  }
  S2D_WIDE_LOAD(w, 0)
  int s0 = 0;
  for (; s0 + 4 <= ksteps; s0 += 4) {
    float b[T][4];
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
      for (int u = 0; u < 4; ++u) b[t][u] = src[t * itile + 4 * (s0 + u)];
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
      for (int u = 0; u < 4; ++u) wn[j][u] = w[j][u];
    }
    if (s0 + 4 < ksteps) { S2D_WIDE_LOAD(wn, s0 + 4) }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int t = 0; t < T; ++t) acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j][u], b[t][u], acc[j][t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
      for (int u = 0; u < 4; ++u) w[j][u] = wn[j][u];
    }
  }
#undef S2D_WIDE_LOAD
  // w now holds steps s0, s0 + 1, s0 + 2 (those that exist)
  bool two = false;
  if (ksteps - s0 >= 2) {                                  // the group of two
    float b[T][2];
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
      for (int u = 0; u < 2; ++u) b[t][u] = src[t * itile + 4 * (s0 + u)];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int t = 0; t < T; ++t) acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j][u], b[t][u], acc[j][t], 0, 0, 0);
      }
    }
    s0 += 2;
    two = true;
  }
  if (s0 < ksteps) {                                       // the single step
    float b[T];
#pragma unroll
    for (int t = 0; t < T; ++t) b[t] = src[t * itile + 4 * s0];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const float wl = two ? w[j][2] : w[j][0];
#pragma unroll
      for (int t = 0; t < T; ++t) acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wl, b[t], acc[j][t], 0, 0, 0);
    }
  }
  float* const dst = out + c * op + 16 * jt0 + 4 * g;
  if (act == S2D_WIDE_RELU) {
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[j][t][r] = acc[j][t][r] > 0.0f ? acc[j][t][r] : 0.0f;   // relu: NaN and -0 -> +0
      }
    }
  }
#pragma unroll
  for (int j = 0; j < J; ++j) {
#pragma unroll
    for (int t = 0; t < T; ++t)
      *reinterpret_cast<float4*>(dst + t * otile + 16 * j) = make_float4(acc[j][t][0], acc[j][t][1], acc[j][t][2], acc[j][t][3]);
  }
  if (act == S2D_WIDE_TANH || act == S2D_WIDE_SIGMOID) {
#pragma unroll 1
    for (int q = 0; q < J * T; ++q) {
      float4* const p4 = reinterpret_cast<float4*>(dst + (q % T) * otile + 16 * (q / T));
      *p4 = wide_act4(act, *p4);
    }
  }
}
// all m16 output tiles of such a layer, four (then two, then one) at a time
template <int T>
S2D_DEV void wide_layer(const float* __restrict__ wf, const float* __restrict__ bias, int m16, int ksteps, const float* __restrict__ in,
                        int ip, int itile, float* __restrict__ out, int op, int otile, int act, int lane) {
  int jt = 0;
  for (; jt + 4 <= m16; jt += 4) wide_group<4, T>(wf, bias, jt, ksteps, in, ip, itile, out, op, otile, act, lane);
  if (jt + 2 <= m16) { wide_group<2, T>(wf, bias, jt, ksteps, in, ip, itile, out, op, otile, act, lane); jt += 2; }
  if (jt < m16) wide_group<1, T>(wf, bias, jt, ksteps, in, ip, itile, out, op, otile, act, lane);
}

// the layers on the wave's observation tile, T env tiles per pass, ping-ponging between the wave's two images: the pass's
// observations go into image B as 4 ceil(IN / 4) words a row (IN = 10: 12 words, x_10 = x_11 = 0), layer 1 reads them and writes
// image A, the output layer writes into the output image qv[env][j] (pitch d.qpitch)
template <int T, int IN = S2D_OBS_DIM>
S2D_DEV void wide_layers(const WideDims& d, const float* __restrict__ bias0, float* __restrict__ ia, float* __restrict__ ib,
                         float* __restrict__ qv, const float* __restrict__ obs_tile, int lane) {
  const int g = lane >> 4, c = lane & 15;
  constexpr int KS1 = (IN + 3) / 4;                         // layer 1's k-steps
  const int rp = d.rpitch, tstride = 16 * rp;
  for (int nt = 0; nt < 4; nt += T) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const float* x = obs_tile + (16 * (nt + t) + c) * IN;
#pragma unroll
      for (int s = 0; s < KS1; ++s) {
        const int k = 4 * s + g;
        ib[t * tstride + c * rp + k] = k < IN ? x[k] : 0.0f;
      }
    }
    wave_lds_fence();
    const float* wf = d.wf;
    const float* bias = bias0;
    int hin = wide_width(d, 0), m16 = (hin + 15) >> 4;
    wide_layer<T>(wf, bias, m16, KS1, ib, rp, tstride, ia, rp, tstride, d.act, lane);
    wave_lds_fence();
    wf += KS1 * m16 * kWave;
    bias += 16 * m16;
    float* in = ia;
    float* out = ib;
    for (int l = 1; l < d.n_hidden; ++l) {
      m16 = (wide_width(d, l) + 15) >> 4;
      wide_layer<T>(wf, bias, m16, hin >> 2, in, rp, tstride, out, rp, tstride, d.act, lane);
      wave_lds_fence();
      wf += m16 * (hin >> 2) * kWave;
      bias += 16 * m16;
      hin = wide_width(d, l);
      float* const swap = in; in = out; out = swap;
    }
    wide_layer<T>(wf, bias, d.na16 >> 4, hin >> 2, in, rp, tstride, qv + 16 * nt * d.qpitch, d.qpitch, 16 * d.qpitch, S2D_WIDE_LINEAR,
                  lane);
    wave_lds_fence();
  }
}

// the network on the observation tile of the wave (lane = env): qv[env][j] = the output layer's pre-activations y_j; ARGMAX: then
// the argmax scan of the two-layer net_forward.  `bias` = the block's LDS (net_pack); ha = the wave's images (A, then B at hb =
// ha + 16 d.pitch).  d.tiles and d.act are wave-uniform; every form is compiled into every kernel.
template <bool ARGMAX, int IN = S2D_OBS_DIM>
S2D_DEV int net_forward(const WideDims& d, const float* __restrict__ bias, float* __restrict__ ha, float* __restrict__ hb,
                        float* __restrict__ qv, const float* __restrict__ obs_tile, int lane) {
  if (d.tiles == 4) wide_layers<4, IN>(d, bias, ha, hb, qv, obs_tile, lane);
  else if (d.tiles == 2) wide_layers<2, IN>(d, bias, ha, hb, qv, obs_tile, lane);
  else wide_layers<1, IN>(d, bias, ha, hb, qv, obs_tile, lane);
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

// what the rollout template calls before its barrier: the bias block of the workspace into the block's LDS (the fragments stay
// where they are).  The template's `params` argument is not used: the pack kernel has read it.
S2D_DEV void net_pack(const WideDims& d, const float* __restrict__, float* __restrict__ smem) {
  const float* const bias = d.wf + (size_t)d.nfrag * kWave;
  for (int idx = threadIdx.x; idx < d.nbias; idx += blockDim.x) smem[idx] = bias[idx];
}

// diagnostic (s2d_debug_wide_forward: IN = 10; s2d_gtc_debug_forward: IN = 4; every unit instantiates its own): the rollouts'
// network on caller observations obs [n][IN] -> y [n][na] and the first maximum, with the rollouts' LDS layout: the wave's
// observation tile sits behind its output image
template <int IN>
__global__ __launch_bounds__(kBlock) void s2d_wide_debug_forward_kernel(WideDims d, const float* __restrict__ obs, int64_t n,
                                                                        float* __restrict__ y, int32_t* __restrict__ greedy,
                                                                        int wave_words) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t wave_first = i - lane;
  net_pack(d, nullptr, smem);
  float* const ha = smem + net_shared_words(d) + wv * wave_words;
  float* const hb = ha + 16 * d.pitch;
  float* const qv = hb + 16 * d.pitch;
  float* const tile = qv + kWave * d.qpitch;
  __syncthreads();
  if (wave_first >= n) return;
  const bool active = i < n;
#pragma unroll
  for (int k = 0; k < IN; ++k) tile[lane * IN + k] = active ? obs[i * IN + k] : 0.0f;
  wave_lds_fence();
  const int best = net_forward<true, IN>(d, smem, ha, hb, qv, tile, lane);
  if (active) {
    for (int a = 0; a < d.na; ++a) y[i * d.na + a] = qv[lane * d.qpitch + a];
    greedy[i] = best;
  }
}

// host side (the shape's grid, the fragment count, the workspace and the plan search are s2d_wide_host.h's)
// words of a wave's LDS part behind its output image, in the rollout template: the observation tile and the PrepTile
static constexpr int kWideTail = kObsTile + (int)(sizeof(PrepTile) / sizeof(float));

// The plan of a valid shape with input width n_in (layer 1 has ceil(n_in / 4) k-steps): the dims (wf left NULL), per-wave words,
// waves per workgroup, env tiles per pass and the LDS bytes: the first of (4, 4) (4, 2) (4, 1) (2, 4) ... (1, 1) that 160 KiB hold
// (wide_plan_search); (1, 1) always fits (width 400: 2 x 16 x 452 words of images).  `force`: the testing override; false if the
// forced pair does not fit or is not in {4, 2, 1}.  tail: the words of a wave behind its output image.
static inline bool wide_plan_lds(int n_in, int n_hidden, const int32_t* hidden, int na, int act, const WidePlanOverride& force, WideDims& d,
                                 int& wave_words, int& waves, size_t& lds, int tail = kWideTail) {
  const WideCounts c = s2d_internal_wide_counts(n_in, n_hidden, hidden, na);
  d = WideDims{};
  d.n_hidden = n_hidden; d.act = act; d.na = na; d.na16 = c.na16;
  d.widths = c.widths; d.nfrag = c.nfrag; d.nbias = c.nbias;
  d.rpitch = (c.wmax + 63) / 64 * 64 + 4;
  d.qpitch = d.na16 + 4;
  const auto words = [&](int t) { return 2 * t * 16 * d.rpitch + kWave * d.qpitch + tail; };
  if (!wide_plan_search(force, kWavesPerBlock, (size_t)((d.nbias + 3) & ~3), words, waves, d.tiles, wave_words, lds)) return false;
  d.pitch = d.tiles * d.rpitch;
  return true;
}

// The plan of `net`'s shape (everything but the engine's side of n_out and the pointers) for an actor with input width n_in: S2D_OK,
// or S2D_EINVAL with the error text set (`who` = the entry point's name).  S2D_WIDE_PLAN=waves,tiles in the environment, read at
// every launch, overrides the plan's choice (testing: the results do not depend on it); a pair that is not of {4, 2, 1} or does
// not fit the LDS is refused.
static inline int wide_net_plan(const std::string& who, const S2DWideNet* net, int n_in, int tail, WideDims& d, int& wave_words, int& waves,
                                size_t& lds) {
  if (s2d_internal_wide_shape(who, nullptr, net->n_hidden, net->hidden, net->activation, net->n_out) != S2D_OK) return S2D_EINVAL;
  const WidePlanOverride force = s2d_internal_plan_override("S2D_WIDE_PLAN");
  if (!wide_plan_lds(n_in, net->n_hidden, net->hidden, net->n_out, net->activation, force, d, wave_words, waves, lds, tail))
    return fail(who, wide_plan_refusal(force) + " for " + s2d_internal_wide_text(n_in, net->n_hidden, net->hidden, net->n_out));
  return S2D_OK;
}
