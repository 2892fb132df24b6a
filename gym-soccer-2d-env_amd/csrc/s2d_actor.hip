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
#include <mutex>
#include <string>

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

// host side (same library, hidden symbol; the rollouts' C entry points and their argument checks are in s2d_engine.hip,
// s2d_debug_net_forward is at the end of this file; the LDS plan is in s2d_actor_net.h)
using QNetKernel = void (*)(S2DHot, const S2DRare*, float*, int64_t, int64_t, int, QNetDims, const float*, const float*, RolloutOut,
                            float*, StepOut, int);
using TanhKernel = void (*)(S2DHot, const S2DRare*, float*, int64_t, int64_t, int, QNetDims, const float*, const float*, RolloutOut,
                            float*, StepOut, int, const float*);

// slots of allow_lds_slot (s2d_actor_net.h): the Q-actor's 3, the tanh actor's 2 x 3 x 2, then s2d_debug_net_forward's
static constexpr int kActorSlots = 3 + 2 * 3 * 2 + 1;
static bool allow_lds(const void* fn, int slot) { return allow_lds_slot<kActorSlots>(fn, slot); }

extern "C" int s2d_internal_rollout_qnet(int nk, const S2DHot* hot, const S2DRare* rare_dev, float* S, int64_t stride, int64_t n,
                                         int n_steps, int h1, int h2, int na, const float* params, const float* eps,
                                         const RolloutOut* ro, float* term_rec, const StepOut* o, void* stream, char* name) {
  QNetDims d;
  int wave_words, waves;
  size_t lds;
  if (!plan_lds(h1, h2, na, d, wave_words, waves, lds)) return -1;
  static const QNetKernel table[3] = {s2d_reach_actor_rollout_kernel<S2D_MODE_DISCRETE, S2D_NK_OFF, false, QNetDims>,
                                       s2d_reach_actor_rollout_kernel<S2D_MODE_DISCRETE, S2D_NK_LATTICE, false, QNetDims>,
                                       s2d_reach_actor_rollout_kernel<S2D_MODE_DISCRETE, S2D_NK_SQUARE, false, QNetDims>};
  if (!allow_lds(reinterpret_cast<const void*>(table[nk]), nk)) return -2;
  const int threads = waves * kWave;
  const unsigned blocks = (unsigned)((n + threads - 1) / threads);
  hipLaunchKernelGGL(table[nk], dim3(blocks), dim3(threads), lds, static_cast<hipStream_t>(stream), *hot, rare_dev, S, stride, n,
                     n_steps, d, params, eps, *ro, term_rec, *o, wave_words);
  if (name) std::snprintf(name, 96, "s2d_reach_qnet_rollout_kernel<noise=%d,h1=%d,h2=%d,a=%d,waves=%d>", nk, h1, h2, na, waves);
  return 0;
}

// mode = S2D_MODE_CONT1 | S2D_MODE_TURN4 (na = 1 | 4), gauss = 0 | 1
extern "C" int s2d_internal_rollout_actor(int mode, int nk, int gauss, const S2DHot* hot, const S2DRare* rare_dev, float* S,
                                          int64_t stride, int64_t n, int n_steps, int h1, int h2, int na, const float* params,
                                          const float* eps, const float* noise, const RolloutOut* ro, float* term_rec,
                                          const StepOut* o, void* stream, char* name) {
  QNetDims d;
  int wave_words, waves;
  size_t lds;
  if (!plan_lds(h1, h2, na, d, wave_words, waves, lds)) return -1;
#define S2D_DDPG_ROW(M)                                                                                                          \
  {s2d_reach_actor_rollout_kernel<M, S2D_NK_OFF, false, QNetDims, const float*>, s2d_reach_actor_rollout_kernel<M, S2D_NK_LATTICE, false, QNetDims, const float*>,                 \
   s2d_reach_actor_rollout_kernel<M, S2D_NK_SQUARE, false, QNetDims, const float*>, s2d_reach_actor_rollout_kernel<M, S2D_NK_OFF, true, QNetDims, const float*>,                   \
   s2d_reach_actor_rollout_kernel<M, S2D_NK_LATTICE, true, QNetDims, const float*>, s2d_reach_actor_rollout_kernel<M, S2D_NK_SQUARE, true, QNetDims, const float*>}
  static const TanhKernel table[2][6] = {S2D_DDPG_ROW(S2D_MODE_CONT1), S2D_DDPG_ROW(S2D_MODE_TURN4)};
#undef S2D_DDPG_ROW
  const int m = mode == S2D_MODE_TURN4 ? 1 : 0, v = 3 * gauss + nk;
  const TanhKernel k = table[m][v];
  if (!allow_lds(reinterpret_cast<const void*>(k), 3 + 6 * m + v)) return -2;
  const int threads = waves * kWave;
  const unsigned blocks = (unsigned)((n + threads - 1) / threads);
  hipLaunchKernelGGL(k, dim3(blocks), dim3(threads), lds, static_cast<hipStream_t>(stream), *hot, rare_dev, S, stride, n, n_steps, d,
                     params, eps, *ro, term_rec, *o, wave_words, noise);
  if (name)
    std::snprintf(name, 96, "s2d_reach_actor_rollout_kernel<mode=%s,noise=%d,gauss=%d,h1=%d,h2=%d,a=%d,waves=%d>",
                  m ? "turn4" : "cont1", nk, gauss, h1, h2, na, waves);
  return 0;
}

// errors share the thread-local text of s2d_last_error() (defined in s2d_engine.hip)
extern "C" void s2d_internal_set_error(const char* msg);

S2D_API int s2d_debug_net_forward(int h1, int h2, int na, const void* params_dev, const void* obs_dev, int64_t n, void* y_dev,
                                  void* greedy_dev, char* name, void* stream) {
  const auto width_ok = [](int w) { return w >= 16 && w <= 128 && w % 16 == 0; };
  const char* err = nullptr;
  if (!width_ok(h1) || !width_ok(h2)) err = "s2d_debug_net_forward: hidden widths must be multiples of 16 in [16, 128]";
  else if (na < 1 || na > 64) err = "s2d_debug_net_forward: na must be in [1, 64]";
  else if (n < 1 || n > INT32_MAX) err = "s2d_debug_net_forward: n must be in [1, 2^31 - 1]";
  else if (!params_dev || (reinterpret_cast<uintptr_t>(params_dev) & 15u))
    err = "s2d_debug_net_forward: params must be a non-NULL, 16-byte aligned device pointer";
  else if (!obs_dev || !y_dev || !greedy_dev ||
           ((reinterpret_cast<uintptr_t>(obs_dev) | reinterpret_cast<uintptr_t>(y_dev) | reinterpret_cast<uintptr_t>(greedy_dev)) & 3u))
    err = "s2d_debug_net_forward: obs, y and greedy must be non-NULL, 4-byte aligned device pointers";
  if (err) { s2d_internal_set_error(err); return S2D_EINVAL; }
  QNetDims d;
  int wave_words, waves;
  size_t lds;
  if (!plan_lds(h1, h2, na, d, wave_words, waves, lds)) {
    s2d_internal_set_error("s2d_debug_net_forward: the network does not fit the LDS of a workgroup");
    return S2D_EINVAL;
  }
  if (!allow_lds(reinterpret_cast<const void*>(s2d_debug_net_forward_kernel), kActorSlots - 1)) {
    s2d_internal_set_error("s2d_debug_net_forward: hipGetDevice or hipFuncSetAttribute failed");
    return S2D_EHIP;
  }
  const int threads = waves * kWave;
  const unsigned blocks = (unsigned)((n + threads - 1) / threads);
  hipLaunchKernelGGL(s2d_debug_net_forward_kernel, dim3(blocks), dim3(threads), lds, static_cast<hipStream_t>(stream), d,
                     static_cast<const float*>(params_dev), static_cast<const float*>(obs_dev), n, static_cast<float*>(y_dev),
                     static_cast<int32_t*>(greedy_dev), wave_words);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    s2d_internal_set_error((std::string("s2d_debug_net_forward: launch: ") + hipGetErrorString(e)).c_str());
    return S2D_EHIP;
  }
  if (name) std::snprintf(name, 96, "s2d_debug_net_forward_kernel<h1=%d,h2=%d,a=%d,waves=%d>", h1, h2, na, waves);
  return S2D_OK;
}
