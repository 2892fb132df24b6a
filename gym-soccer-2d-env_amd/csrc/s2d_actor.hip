// s2d_actor.hip -- the fused actors: the epsilon-greedy Q-network (s2d_rollout_qnet) and the deterministic tanh policy with
// Gaussian action noise (s2d_rollout_actor); include/s2d.h, DESIGN.md sections 4, 5.
//
// The plain rollout kernel (one env per lane, the whole cycle in one wave, T cycles per launch) with the action of every cycle
// chosen in-kernel from the caller's network  y = W3 relu(W2 relu(W1 x + b1) + b2) + b3  on the env's current observation, and
// per-env epsilon exploration.  Head by mode: discrete engines take the argmax of y (DQN("MlpPolicy").predict inside SB3's
// collect_rollouts, dqn_stable_baselines3.py:36-49); continuous (A = 1) and turning (A = 4) engines take a_j = tanh_spec(y_j),
// optionally plus clipped Gaussian noise (SB3's DDPG / TD3 actor.mu with NormalActionNoise, ddpg_stable_baselines3.py).
//
// The network runs on the f32-input matrix cores: v_mfma_f32_16x16x4_f32 is bit for bit the k-ordered fmaf chain
// acc = fma(a_k3, b_k3, fma(a_k2, b_k2, fma(a_k1, b_k1, fma(a_k0, b_k0, C)))), so a chain of them that starts from C = bias
// and is fed its k-steps in ascending order is exactly the spec's  acc = b[j]; for k ascending: acc = fmaf(W[j][k], in[k], acc).
// Orientation: A = the weights (rows = output units j, lane l holds W[16 jt + (l & 15)][4 s + (l >> 4)] for k-step s), B = the
// activations (lane l holds in[env 16 nt + (l & 15)][4 s + (l >> 4)]), D: lane l, register r = unit 16 jt + 4 (l >> 4) + r of env
// 16 nt + (l & 15).  D is not the next layer's B fragment (that would permute k), so every layer's output goes through LDS:
// each lane writes its four units as one 16-byte store into [env][unit] rows and the next layer reads single words in k order.
// A wave works through its 64 envs as four tiles of 16.  Layer 1 reads the observation tile ([64][10], k = 10, 11 read as
// zero against zero weights: fmaf(0, 0, acc) can only turn -0 into +0, which relu maps to +0 anyway).
// The weights are repacked once per launch into fragment order in LDS (each fragment = 64 consecutive words, conflict-free
// reads); the parameter buffer and epsilon are read when the kernel runs, so a captured graph acts with what they hold at replay.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "s2d_actor_net.h"
#include "s2d_actor_rollout.h"

// The fused rollout of both actors is s2d_reach_actor_rollout_kernel<MODE, NK, GAUSS, Dims, Noise...> of s2d_actor_rollout.h, here
// with Dims = QNetDims (net_pack, net_shared_words and net_forward of s2d_actor_net.h).

// diagnostic (s2d_debug_net_forward): the rollout's network on caller observations.  The same packing, LDS layout and
// net_forward as s2d_reach_actor_rollout_kernel; the observation tile holds obs[i] for the wave's envs i < n and zero rows past
// n; y[i][0 .. na-1] = the output layer's pre-activations, greedy[i] = their argmax.
__global__ __launch_bounds__(kBlock) void s2d_debug_net_forward_kernel(QNetDims d, const float* __restrict__ params,
                                                                       const float* __restrict__ obs, int64_t n, float* __restrict__ y,
                                                                       int32_t* __restrict__ greedy, int wave_words) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t wave_first = i - lane;
  net_pack(d, params, smem);
  float* const ha = smem + net_shared_words(d) + wv * wave_words;
  float* const hb = ha + 16 * d.pitch;
  float* const qv = hb + 16 * d.pitch;
  float* const tile = qv + kWave * d.qpitch;
  __syncthreads();
  if (wave_first >= n) return;
  const bool active = i < n;
#pragma unroll
  for (int k = 0; k < S2D_OBS_DIM; ++k) tile[lane * S2D_OBS_DIM + k] = active ? obs[i * S2D_OBS_DIM + k] : 0.0f;
  wave_lds_fence();
  const int best = net_forward<true>(d, smem, ha, hb, qv, tile, lane);
  if (active) {
    for (int a = 0; a < d.na; ++a) y[i * d.na + a] = qv[lane * d.qpitch + a];
    greedy[i] = best;
  }
}

// host side (same library, hidden symbol; the rollouts' C entry points and their argument checks are in s2d_engine.hip, the
// tables and the launch in s2d_actor_rollout.h, s2d_debug_net_forward is at the end of this file; the LDS plan is in
// s2d_actor_net.h)
bool s2d_internal_net_plan(int h1, int h2, int na, ActorPlanBuf* buf) {
  ActorPlan<QNetDims>& pl = plan_in<QNetDims>(buf);
  return plan_lds(h1, h2, na, pl.d, pl.wave_words, pl.waves, pl.lds);
}

int s2d_internal_rollout_net(const ActorRollout& a, const ActorPlanBuf& buf, const float* params, const float* eps, const float* noise) {
  const ActorPlan<QNetDims>& pl = plan_of<QNetDims>(buf);
  const int h1 = pl.d.h1, h2 = pl.d.h2, na = pl.d.na;
  if (!launch_actor_rollout(a, pl, params, eps, noise, [] {})) return -2;
  if (a.mode == S2D_MODE_DISCRETE)
    std::snprintf(a.name, a.name_bytes, "s2d_reach_qnet_rollout_kernel<noise=%d,h1=%d,h2=%d,a=%d,waves=%d>", a.nk, h1, h2, na, pl.waves);
  else
    std::snprintf(a.name, a.name_bytes, "s2d_reach_actor_rollout_kernel<mode=%s,noise=%d,gauss=%d,h1=%d,h2=%d,a=%d,waves=%d>",
                  a.mode == S2D_MODE_TURN4 ? "turn4" : "cont1", a.nk, noise ? 1 : 0, h1, h2, na, pl.waves);
  return 0;
}

S2D_API int s2d_debug_net_forward(int h1, int h2, int na, const void* params_dev, const void* obs_dev, int64_t n, void* y_dev,
                                  void* greedy_dev, char* name, void* stream) {
  static const char who[] = "s2d_debug_net_forward";
  const auto width_ok = [](int w) { return w >= 16 && w <= 128 && w % 16 == 0; };
  const char* err = nullptr;
  if (!width_ok(h1) || !width_ok(h2)) err = "s2d_debug_net_forward: hidden widths must be multiples of 16 in [16, 128]";
  else if (na < 1 || na > 64) err = "s2d_debug_net_forward: na must be in [1, 64]";
  if (err) { s2d_internal_set_error(err); return S2D_EINVAL; }
  int rc = debug_forward_args(who, params_dev, obs_dev, n, y_dev, greedy_dev);
  if (rc != S2D_OK) return rc;
  ActorPlanBuf buf;
  if (!s2d_internal_net_plan(h1, h2, na, &buf)) {
    s2d_internal_set_error("s2d_debug_net_forward: the network does not fit the LDS of a workgroup");
    return S2D_EINVAL;
  }
  const ActorPlan<QNetDims>& pl = plan_of<QNetDims>(buf);
  rc = debug_forward_launch(who, reinterpret_cast<const void*>(s2d_debug_net_forward_kernel), pl, n, [&](unsigned blocks, int threads) {
    hipLaunchKernelGGL(s2d_debug_net_forward_kernel, dim3(blocks), dim3(threads), pl.lds, static_cast<hipStream_t>(stream), pl.d,
                       static_cast<const float*>(params_dev), static_cast<const float*>(obs_dev), n, static_cast<float*>(y_dev),
                       static_cast<int32_t*>(greedy_dev), pl.wave_words);
  });
  if (rc == S2D_OK && name) std::snprintf(name, 96, "s2d_debug_net_forward_kernel<h1=%d,h2=%d,a=%d,waves=%d>", h1, h2, na, pl.waves);
  return rc;
}
