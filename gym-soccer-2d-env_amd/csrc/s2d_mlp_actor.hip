// s2d_mlp_actor.hip -- the fused actors on a general MLP: the epsilon-greedy Q-network (s2d_rollout_qnet_mlp) and the
// deterministic tanh policy with Gaussian action noise (s2d_rollout_actor_mlp) with one to four hidden layers, widths that are
// multiples of 8 and relu or tanh_spec between them; include/s2d.h S2DMlpNet, DESIGN.md sections 4, 5.
//
// The rollout kernel is s2d_reach_actor_rollout_kernel (s2d_actor_rollout.h), the template of s2d_rollout_qnet / s2d_rollout_actor
// over the network's descriptor: the heads, the draws, the simulation, the records and the statistics are theirs.  Only the
// network differs (MlpDims, s2d_mlp_net.h): a loop over the layers on the f32 matrix cores in the k-ordered fmaf spec.  The
// hidden activation is a field of that kernel argument (wave-uniform) with both forms compiled in, so the instantiations are
// those of the two-layer actors: 3 for the Q-actor, 12 for the tanh actor, and the diagnostic kernel.  With two hidden layers,
// widths that are multiples of 16 and relu the result is the two-layer actors' bit for bit.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>

#include "s2d_actor_rollout.h"
#include "s2d_mlp_net.h"

// The rollout kernels are s2d_reach_actor_rollout_kernel<MODE, NK, GAUSS, MlpDims, Noise...> (s2d_actor_rollout.h): MODE =
// S2D_MODE_DISCRETE is s2d_rollout_qnet_mlp, CONT1 / TURN4 s2d_rollout_actor_mlp (GAUSS: with Gaussian action noise).

// diagnostic (s2d_debug_mlp_forward): the rollout's network on caller observations.  The same packing, LDS layout and
// net_forward as the rollout kernels; the observation tile holds obs[i] for the wave's envs i < n and zero rows past n;
// y[i][0 .. na-1] = the output layer's pre-activations, greedy[i] = their argmax.
__global__ __launch_bounds__(kBlock) void s2d_debug_mlp_forward_kernel(MlpDims d, const float* __restrict__ params,
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

// host side (same library, hidden symbols; the rollouts' C entry points are in s2d_engine.hip, s2d_debug_mlp_forward is at the
// end of this file; the LDS plan is in s2d_mlp_net.h)
using MlpQNetKernel = void (*)(S2DHot, const S2DRare*, float*, int64_t, int64_t, int, MlpDims, const float*, const float*,
                               RolloutOut, float*, StepOut, int);
using MlpTanhKernel = void (*)(S2DHot, const S2DRare*, float*, int64_t, int64_t, int, MlpDims, const float*, const float*,
                               RolloutOut, float*, StepOut, int, const float*);

// slots of allow_lds_slot (s2d_actor_net.h): the Q-actor's 3, the tanh actor's 2 x 3 x 2, then s2d_debug_mlp_forward's
static constexpr int kMlpSlots = 3 + 2 * 3 * 2 + 1;
static bool allow_lds(const void* fn, int slot) { return allow_lds_slot<kMlpSlots>(fn, slot); }

// errors share the thread-local text of s2d_last_error() (defined in s2d_engine.hip)
extern "C" void s2d_internal_set_error(const char* msg);

// "128-64-32-16"
static std::string widths_text(const S2DMlpNet* net) {
  std::string s;
  for (int l = 0; l < net->n_hidden; ++l) s += (l ? "-" : "") + std::to_string(net->hidden[l]);
  return s;
}

// The shape of `net` (everything but the engine's side of n_out and the pointers): 0 and the plan, or S2D_EINVAL with the
// error text set (`who` = the entry point's name).  The text of a shape that does not fit says how many bytes it needs.
static int mlp_plan(const char* who, const S2DMlpNet* net, MlpDims* d, int* wave_words, int* waves, size_t* lds) {
  const std::string w(who);
  if (net->n_hidden < 1 || net->n_hidden > kMlpMaxHidden) {
    s2d_internal_set_error((w + ": n_hidden must be in [1, 4]").c_str());
    return S2D_EINVAL;
  }
  if (!mlp_shape_ok(net->n_hidden, net->hidden)) {
    s2d_internal_set_error((w + ": hidden widths must be multiples of 8 in [8, 128] (the weights live in LDS), and 0 past n_hidden").c_str());
    return S2D_EINVAL;
  }
  if (net->activation != 0 && net->activation != 1) {
    s2d_internal_set_error((w + ": activation must be 0 (ReLU) or 1 (Tanh)").c_str());
    return S2D_EINVAL;
  }
  if (net->n_out < 1 || net->n_out > 64) {
    s2d_internal_set_error((w + ": n_out must be in [1, 64]").c_str());
    return S2D_EINVAL;
  }
  if (!mlp_plan_lds(net->n_hidden, net->hidden, net->n_out, net->activation, *d, *wave_words, *waves, *lds)) {
    s2d_internal_set_error((w + ": the network 10-" + widths_text(net) + "-" + std::to_string(net->n_out) + " needs " +
                            std::to_string(*lds) + " bytes of LDS for its fragments and one wave's images; a workgroup has " +
                            std::to_string(kLdsMax)).c_str());
    return S2D_EINVAL;
  }
  return S2D_OK;
}

// the shape check alone, for the entry points of s2d_engine.hip (they check their engine's side and the pointers themselves)
extern "C" int s2d_internal_mlp_check(const char* who, const S2DMlpNet* net) {
  MlpDims d;
  int wave_words, waves;
  size_t lds;
  return mlp_plan(who, net, &d, &wave_words, &waves, &lds);
}

// launches the Q-network actor rollout of a checked network: 0, S2D_EINVAL (the error text set), or -2 on a HIP failure
extern "C" int s2d_internal_rollout_qnet_mlp(int nk, const S2DHot* hot, const S2DRare* rare_dev, float* S, int64_t stride, int64_t n,
                                             int n_steps, const S2DMlpNet* net, const RolloutOut* ro, float* term_rec,
                                             const StepOut* o, void* stream, char* name, size_t name_bytes) {
  MlpDims d;
  int wave_words, waves;
  size_t lds;
  if (mlp_plan("s2d_rollout_qnet_mlp", net, &d, &wave_words, &waves, &lds) != S2D_OK) return S2D_EINVAL;
  static const MlpQNetKernel table[3] = {s2d_reach_actor_rollout_kernel<S2D_MODE_DISCRETE, S2D_NK_OFF, false, MlpDims>,
                                          s2d_reach_actor_rollout_kernel<S2D_MODE_DISCRETE, S2D_NK_LATTICE, false, MlpDims>,
                                          s2d_reach_actor_rollout_kernel<S2D_MODE_DISCRETE, S2D_NK_SQUARE, false, MlpDims>};
  if (!allow_lds(reinterpret_cast<const void*>(table[nk]), nk)) return -2;
  const int threads = waves * kWave;
  const unsigned blocks = (unsigned)((n + threads - 1) / threads);
  hipLaunchKernelGGL(table[nk], dim3(blocks), dim3(threads), lds, static_cast<hipStream_t>(stream), *hot, rare_dev, S, stride, n,
                     n_steps, d, net->params, net->epsilon, *ro, term_rec, *o, wave_words);
  if (name)
    std::snprintf(name, name_bytes, "s2d_mlp_qnet_rollout_kernel<noise=%d,act=%s,h=%s,a=%d,waves=%d>", nk,
                  net->activation ? "tanh" : "relu", widths_text(net).c_str(), net->n_out, waves);
  return 0;
}

// mode = S2D_MODE_CONT1 | S2D_MODE_TURN4 (n_out = 1 | 4), the noise kind is net's
extern "C" int s2d_internal_rollout_actor_mlp(int mode, int nk, const S2DHot* hot, const S2DRare* rare_dev, float* S, int64_t stride,
                                              int64_t n, int n_steps, const S2DMlpNet* net, const RolloutOut* ro, float* term_rec,
                                              const StepOut* o, void* stream, char* name, size_t name_bytes) {
  MlpDims d;
  int wave_words, waves;
  size_t lds;
  if (mlp_plan("s2d_rollout_actor_mlp", net, &d, &wave_words, &waves, &lds) != S2D_OK) return S2D_EINVAL;
#define S2D_MLP_ROW(M)                                                                                                       \
  {s2d_reach_actor_rollout_kernel<M, S2D_NK_OFF, false, MlpDims, const float*>, s2d_reach_actor_rollout_kernel<M, S2D_NK_LATTICE, false, MlpDims, const float*>, \
   s2d_reach_actor_rollout_kernel<M, S2D_NK_SQUARE, false, MlpDims, const float*>, s2d_reach_actor_rollout_kernel<M, S2D_NK_OFF, true, MlpDims, const float*>,   \
   s2d_reach_actor_rollout_kernel<M, S2D_NK_LATTICE, true, MlpDims, const float*>, s2d_reach_actor_rollout_kernel<M, S2D_NK_SQUARE, true, MlpDims, const float*>}
  static const MlpTanhKernel table[2][6] = {S2D_MLP_ROW(S2D_MODE_CONT1), S2D_MLP_ROW(S2D_MODE_TURN4)};
#undef S2D_MLP_ROW
  const int gauss = net->noise_kind ? 1 : 0;
  const int m = mode == S2D_MODE_TURN4 ? 1 : 0, v = 3 * gauss + nk;
  const MlpTanhKernel k = table[m][v];
  if (!allow_lds(reinterpret_cast<const void*>(k), 3 + 6 * m + v)) return -2;
  const int threads = waves * kWave;
  const unsigned blocks = (unsigned)((n + threads - 1) / threads);
  hipLaunchKernelGGL(k, dim3(blocks), dim3(threads), lds, static_cast<hipStream_t>(stream), *hot, rare_dev, S, stride, n, n_steps, d,
                     net->params, net->epsilon, *ro, term_rec, *o, wave_words, gauss ? net->noise : nullptr);
  if (name)
    std::snprintf(name, name_bytes, "s2d_mlp_actor_rollout_kernel<mode=%s,noise=%d,gauss=%d,act=%s,h=%s,a=%d,waves=%d>",
                  m ? "turn4" : "cont1", nk, gauss, net->activation ? "tanh" : "relu", widths_text(net).c_str(), net->n_out, waves);
  return 0;
}

S2D_API int s2d_debug_mlp_forward(const S2DMlpNet* shape, const void* obs_dev, int64_t n, void* y_dev, void* greedy_dev, char* name,
                                  void* stream) {
  if (!shape) { s2d_internal_set_error("s2d_debug_mlp_forward: shape is NULL"); return S2D_EINVAL; }
  MlpDims d;
  int wave_words, waves;
  size_t lds;
  const int rc = mlp_plan("s2d_debug_mlp_forward", shape, &d, &wave_words, &waves, &lds);
  if (rc != S2D_OK) return rc;
  const char* err = nullptr;
  if (n < 1 || n > INT32_MAX) err = "s2d_debug_mlp_forward: n must be in [1, 2^31 - 1]";
  else if (!shape->params || (reinterpret_cast<uintptr_t>(shape->params) & 15u))
    err = "s2d_debug_mlp_forward: params must be a non-NULL, 16-byte aligned device pointer";
  else if (!obs_dev || !y_dev || !greedy_dev ||
           ((reinterpret_cast<uintptr_t>(obs_dev) | reinterpret_cast<uintptr_t>(y_dev) | reinterpret_cast<uintptr_t>(greedy_dev)) & 3u))
    err = "s2d_debug_mlp_forward: obs, y and greedy must be non-NULL, 4-byte aligned device pointers";
  if (err) { s2d_internal_set_error(err); return S2D_EINVAL; }
  if (!allow_lds(reinterpret_cast<const void*>(s2d_debug_mlp_forward_kernel), kMlpSlots - 1)) {
    s2d_internal_set_error("s2d_debug_mlp_forward: hipGetDevice or hipFuncSetAttribute failed");
    return S2D_EHIP;
  }
  const int threads = waves * kWave;
  const unsigned blocks = (unsigned)((n + threads - 1) / threads);
  hipLaunchKernelGGL(s2d_debug_mlp_forward_kernel, dim3(blocks), dim3(threads), lds, static_cast<hipStream_t>(stream), d,
                     shape->params, static_cast<const float*>(obs_dev), n, static_cast<float*>(y_dev),
                     static_cast<int32_t*>(greedy_dev), wave_words);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    s2d_internal_set_error((std::string("s2d_debug_mlp_forward: launch: ") + hipGetErrorString(e)).c_str());
    return S2D_EHIP;
  }
  if (name)
    std::snprintf(name, 96, "s2d_debug_mlp_forward_kernel<act=%s,h=%s,a=%d,waves=%d>", shape->activation ? "tanh" : "relu",
                  widths_text(shape).c_str(), shape->n_out, waves);
  return S2D_OK;
}
