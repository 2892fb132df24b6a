// s2d_net.h -- the building blocks of the fused networks, shared by the reach-ball actors (s2d_actor.hip) and the 11v11
// engine's network slots (s2d_match_slots.h): one layer on v_mfma_f32_16x16x4_f32 in the k-ordered fmaf spec, and the exploration
// threshold of a device epsilon.  (Moved out of s2d_actor.hip unchanged.)
//
// v_mfma_f32_16x16x4_f32 is bit for bit the k-ordered fmaf chain acc = fma(a_k3, b_k3, fma(a_k2, b_k2, fma(a_k1, b_k1,
// fma(a_k0, b_k0, C)))), so a chain of them that starts from C = bias and is fed its k-steps in ascending order is exactly
// acc = b[j]; for k ascending: acc = fmaf(W[j][k], in[k], acc).  A = the weights in fragment order (fragment f = 64 consecutive
// words, lane l holds W[16 jt + (l & 15)][4 s + (l >> 4)] of k-step s), B = the activations (lane l holds in[row (l & 15)][4 s +
// (l >> 4)]), D: lane l, register r = unit 16 jt + 4 (l >> 4) + r of row (l & 15).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "s2d_device.h"

static constexpr int kWave = 64;
typedef float v4f_t __attribute__((ext_vector_type(4)));

// J output tiles (jt0 .. jt0 + J - 1) of one layer for one 16-env tile: out[c][j] (LDS, pitch `op`) = (act)(b[j] + sum_k W[j][k]
// in[k]) for the tile's 16 envs c.  in_frag(s) = this lane's B word of k-step s.  J independent accumulators keep the matrix pipe
// issuing (dependent latency 40 cycles against a 32-cycle issue); the k-steps go in groups of KU whose LDS reads are issued together.
// All 64 lanes take part (MFMA).  ACT: the activation on the accumulators, S2D_ACT_FN_* (the callers that say true / false get
// relu / none, as before; tanh_spec is the stochastic policy's, s2d_policy.hip).
enum { S2D_ACT_FN_NONE = 0, S2D_ACT_FN_RELU = 1, S2D_ACT_FN_TANH = 2 };
template <int ACT, int J, int KU, typename InFrag>
S2D_DEV void layer_group(const float* __restrict__ wf, const float* __restrict__ bias, int jt0, int ksteps, InFrag in_frag,
                         float* __restrict__ out, int op, int lane) {
  const int g = lane >> 4, c = lane & 15;
  v4f_t acc[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const float4 b4 = *reinterpret_cast<const float4*>(bias + 16 * (jt0 + j) + 4 * g);
    acc[j] = v4f_t{b4.x, b4.y, b4.z, b4.w};
  }
  for (int s0 = 0; s0 < ksteps; s0 += KU) {
    float b[KU], w[J][KU];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      b[u] = in_frag(s0 + u);
#pragma unroll
      for (int j = 0; j < J; ++j) w[j][u] = wf[((jt0 + j) * ksteps + s0 + u) * kWave + lane];
    }
#pragma unroll
    for (int u = 0; u < KU; ++u) {
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
// all m16 output tiles of one layer, four (then two, then one) at a time
template <int ACT, int KU, typename InFrag>
S2D_DEV void layer_tile(const float* __restrict__ wf, const float* __restrict__ bias, int m16, int ksteps, InFrag in_frag,
                        float* __restrict__ out, int op, int lane) {
  int jt = 0;
  for (; jt + 4 <= m16; jt += 4) layer_group<ACT, 4, KU>(wf, bias, jt, ksteps, in_frag, out, op, lane);
  if (jt + 2 <= m16) { layer_group<ACT, 2, KU>(wf, bias, jt, ksteps, in_frag, out, op, lane); jt += 2; }
  if (jt < m16) layer_group<ACT, 1, KU>(wf, bias, jt, ksteps, in_frag, out, op, lane);
}

// exploration threshold of a device epsilon: eps >= 1 -> 2^32, eps > 0 -> (uint64)(eps 2^32), else (0, -x, NaN) 0
S2D_DEV uint64_t explore_threshold(float eps) {
  return eps >= 1.0f ? (1ull << 32) : eps > 0.0f ? (uint64_t)(eps * 4294967296.0f) : 0ull;
}
