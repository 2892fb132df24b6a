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

// host side (same library, hidden symbols; the rollouts' C entry points are in s2d_engine.hip, the tables and the launch in
// s2d_actor_rollout.h, s2d_debug_mlp_forward is at the end of this file; the LDS plan is in s2d_mlp_net.h)

// The shape of `net` (everything but the engine's side of n_out and the pointers): 0 and the plan, or S2D_EINVAL with the
// error text set (`who` = the entry point's name).  The text of a shape that does not fit says how many bytes it needs.
int s2d_internal_mlp_plan(const char* who, const S2DMlpNet* net, ActorPlanBuf* buf) {
  ActorPlan<MlpDims>* const pl = &plan_in<MlpDims>(buf);
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
  if (!mlp_plan_lds(net->n_hidden, net->hidden, net->n_out, net->activation, pl->d, pl->wave_words, pl->waves, pl->lds)) {
    s2d_internal_set_error((w + ": the network 10-" + widths_text(net) + "-" + std::to_string(net->n_out) + " needs " +
                            std::to_string(pl->lds) + " bytes of LDS for its fragments and one wave's images; a workgroup has " +
                            std::to_string(kLdsMax)).c_str());
    return S2D_EINVAL;
  }
  return S2D_OK;
}

int s2d_internal_rollout_mlp(const ActorRollout& a, const char*, const S2DMlpNet* net, const ActorPlanBuf& buf) {
  const ActorPlan<MlpDims>& pl = plan_of<MlpDims>(buf);
  const float* const noise = net->noise_kind ? net->noise : nullptr;
  if (!launch_actor_rollout(a, pl, net->params, net->epsilon, noise, [] {})) return -2;
  const char* const act = net->activation ? "tanh" : "relu";
  if (a.mode == S2D_MODE_DISCRETE)
    std::snprintf(a.name, a.name_bytes, "s2d_mlp_qnet_rollout_kernel<noise=%d,act=%s,h=%s,a=%d,waves=%d>", a.nk, act,
                  widths_text(net).c_str(), net->n_out, pl.waves);
  else
    std::snprintf(a.name, a.name_bytes, "s2d_mlp_actor_rollout_kernel<mode=%s,noise=%d,gauss=%d,act=%s,h=%s,a=%d,waves=%d>",
                  a.mode == S2D_MODE_TURN4 ? "turn4" : "cont1", a.nk, noise ? 1 : 0, act, widths_text(net).c_str(), net->n_out, pl.waves);
  return 0;
}

S2D_API int s2d_debug_mlp_forward(const S2DMlpNet* shape, const void* obs_dev, int64_t n, void* y_dev, void* greedy_dev, char* name,
                                  void* stream) {
  static const char who[] = "s2d_debug_mlp_forward";
  if (!shape) { s2d_internal_set_error("s2d_debug_mlp_forward: shape is NULL"); return S2D_EINVAL; }
  ActorPlanBuf buf;
  int rc = s2d_internal_mlp_plan(who, shape, &buf);
  if (rc == S2D_OK) rc = debug_forward_args(who, shape->params, obs_dev, n, y_dev, greedy_dev);
  if (rc != S2D_OK) return rc;
  const ActorPlan<MlpDims>& pl = plan_of<MlpDims>(buf);
  rc = debug_forward_launch(who, reinterpret_cast<const void*>(s2d_debug_mlp_forward_kernel), pl, n, [&](unsigned blocks, int threads) {
    hipLaunchKernelGGL(s2d_debug_mlp_forward_kernel, dim3(blocks), dim3(threads), pl.lds, static_cast<hipStream_t>(stream), pl.d,
                       shape->params, static_cast<const float*>(obs_dev), n, static_cast<float*>(y_dev),
                       static_cast<int32_t*>(greedy_dev), pl.wave_words);
  });
  if (rc == S2D_OK && name)
    std::snprintf(name, 96, "s2d_debug_mlp_forward_kernel<act=%s,h=%s,a=%d,waves=%d>", shape->activation ? "tanh" : "relu",
                  widths_text(shape).c_str(), shape->n_out, pl.waves);
  return rc;
}
