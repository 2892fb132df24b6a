// s2d_wide_actor.hip -- the fused actors on the streamed-weight MLP: the epsilon-greedy Q-network (s2d_rollout_qnet_wide) and the
// deterministic tanh policy with Gaussian action noise (s2d_rollout_actor_wide) with one to five hidden layers, widths that are
// multiples of 4 up to 400 and relu, tanh_spec or sigmoid_spec between them; include/s2d.h S2DWideNet, DESIGN.md sections 4, 5, 7.
//
// The rollout kernel is s2d_reach_actor_rollout_kernel (s2d_actor_rollout.h) over a second network back end (WideDims,
// s2d_wide_net.h): the heads, the draws, the simulation, the records and the statistics are the template's.  The weights do not
// live in LDS: a pack kernel writes them in fragment order into the caller's workspace, on the same stream ahead of the
// rollout, and the rollout's waves stream them from there (L2) into registers layer by layer.  The activation and the env tiles
// per pass are fields of the kernel argument (wave-uniform), so the instantiations are those of the resident actors: 3 for the
// Q-actor, 12 for the tanh actor, and the diagnostic kernel.  On a shape the resident path takes the result is its, bit for bit.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "s2d_actor_rollout.h"
#include "s2d_wide_net.h"

// diagnostic (s2d_debug_wide_forward): the rollout's network on caller observations, as s2d_debug_mlp_forward_kernel
__global__ __launch_bounds__(kBlock) void s2d_debug_wide_forward_kernel(WideDims d, const float* __restrict__ obs, int64_t n,
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
  for (int k = 0; k < S2D_OBS_DIM; ++k) tile[lane * S2D_OBS_DIM + k] = active ? obs[i * S2D_OBS_DIM + k] : 0.0f;
  wave_lds_fence();
  const int best = net_forward<true>(d, smem, ha, hb, qv, tile, lane);
  if (active) {
    for (int a = 0; a < d.na; ++a) y[i * d.na + a] = qv[lane * d.qpitch + a];
    greedy[i] = best;
  }
}

// host side (same library, hidden symbols; the rollouts' C entry points are in s2d_engine.hip, the tables and the launch in
// s2d_actor_rollout.h, s2d_wide_workspace_bytes and s2d_debug_wide_forward at the end of this file; the plan is in s2d_wide_net.h)
static const char* const kActName[3] = {"relu", "tanh", "sigmoid"};

static size_t workspace_bytes(const WideDims& d) { return ((size_t)d.nfrag * kWave + d.nbias) * sizeof(float); }

// The shape of `net` (everything but the engine's side of n_out and the pointers): 0 and the plan, or S2D_EINVAL with the
// error text set (`who` = the entry point's name).  S2D_WIDE_PLAN=waves,tiles in the environment, read at every launch, overrides
// the plan's choice of waves per workgroup and env tiles per pass (testing: the results do not depend on them); a pair that is
// not of {4, 2, 1} or does not fit the LDS is refused.
int s2d_internal_wide_plan(const char* who, const S2DWideNet* net, ActorPlanBuf* buf) {
  ActorPlan<WideDims>* const pl = &plan_in<WideDims>(buf);
  const std::string w(who);
  if (net->n_hidden < 1 || net->n_hidden > kWideMaxHidden) {
    s2d_internal_set_error((w + ": n_hidden must be in [1, 5]").c_str());
    return S2D_EINVAL;
  }
  if (!wide_shape_ok(net->n_hidden, net->hidden)) {
    s2d_internal_set_error((w + ": hidden widths must be multiples of 4 in [8, 400], and 0 past n_hidden").c_str());
    return S2D_EINVAL;
  }
  if (net->activation < 0 || net->activation > 2) {
    s2d_internal_set_error((w + ": activation must be 0 (ReLU), 1 (Tanh) or 2 (Sigmoid)").c_str());
    return S2D_EINVAL;
  }
  if (net->n_out < 1 || net->n_out > 64) {
    s2d_internal_set_error((w + ": n_out must be in [1, 64]").c_str());
    return S2D_EINVAL;
  }
  int fw = 0, ft = 0;
  const char* const env = std::getenv("S2D_WIDE_PLAN");
  if (env && *env && std::sscanf(env, "%d,%d", &fw, &ft) != 2) fw = ft = -1;
  if (!wide_plan_lds(net->n_hidden, net->hidden, net->n_out, net->activation, fw, ft, pl->d, pl->wave_words, pl->waves, pl->lds)) {
    s2d_internal_set_error((w + ": S2D_WIDE_PLAN=" + (env ? env : "") + " is not waves,tiles of {4, 2, 1} that fit the LDS for 10-" +
                            widths_text(net) + "-" + std::to_string(net->n_out)).c_str());
    return S2D_EINVAL;
  }
  return S2D_OK;
}

// the workspace of a planned shape: S2D_EINVAL with the text set if it is NULL, misaligned or too small
static int wide_workspace(const char* who, const S2DWideNet* net, const WideDims& d) {
  const std::string w(who);
  if (!net->workspace || (reinterpret_cast<uintptr_t>(net->workspace) & 255u)) {
    s2d_internal_set_error((w + ": workspace must be a non-NULL, 256-byte aligned device pointer").c_str());
    return S2D_EINVAL;
  }
  if (net->workspace_bytes < workspace_bytes(d)) {
    s2d_internal_set_error((w + ": workspace_bytes is " + std::to_string(net->workspace_bytes) + ", the network 10-" + widths_text(net) +
                            "-" + std::to_string(net->n_out) + " needs " + std::to_string(workspace_bytes(d)) +
                            " (s2d_wide_workspace_bytes)").c_str());
    return S2D_EINVAL;
  }
  return S2D_OK;
}

// params -> workspace in fragment order, on `stream`
static void launch_pack(const WideDims& d, const S2DWideNet* net, hipStream_t stream) {
  const int words = d.nfrag * kWave + d.nbias;
  hipLaunchKernelGGL(s2d_wide_pack_kernel<S2D_OBS_DIM>, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, d, net->params,
                     static_cast<float*>(net->workspace));
}

// the workspace check, then the pack kernel and the rollout
int s2d_internal_rollout_wide(const ActorRollout& a, const char* who, const S2DWideNet* net, const ActorPlanBuf& buf) {
  ActorPlan<WideDims> pl = plan_of<WideDims>(buf);
  if (wide_workspace(who, net, pl.d) != S2D_OK) return S2D_EINVAL;
  pl.d.wf = static_cast<const float*>(net->workspace);
  const float* const noise = net->noise_kind ? net->noise : nullptr;
  if (!launch_actor_rollout(a, pl, net->params, net->epsilon, noise, [&] { launch_pack(pl.d, net, static_cast<hipStream_t>(a.stream)); }))
    return -2;
  if (a.mode == S2D_MODE_DISCRETE)
    std::snprintf(a.name, a.name_bytes, "s2d_wide_qnet_rollout_kernel<noise=%d,act=%s,h=%s,a=%d,waves=%d,tiles=%d>", a.nk,
                  kActName[net->activation], widths_text(net).c_str(), net->n_out, pl.waves, pl.d.tiles);
  else
    std::snprintf(a.name, a.name_bytes, "s2d_wide_actor_rollout_kernel<mode=%s,noise=%d,gauss=%d,act=%s,h=%s,a=%d,waves=%d,tiles=%d>",
                  a.mode == S2D_MODE_TURN4 ? "turn4" : "cont1", a.nk, noise ? 1 : 0, kActName[net->activation], widths_text(net).c_str(),
                  net->n_out, pl.waves, pl.d.tiles);
  return 0;
}

S2D_API size_t s2d_wide_workspace_bytes(const S2DWideNet* shape) {
  if (!shape || !wide_shape_ok(shape->n_hidden, shape->hidden) || shape->n_out < 1 || shape->n_out > 64) return 0;
  WideDims d;
  int wave_words, waves;
  size_t lds;
  if (!wide_plan_lds(shape->n_hidden, shape->hidden, shape->n_out, 0, 0, 0, d, wave_words, waves, lds)) return 0;
  return workspace_bytes(d);
}

S2D_API int s2d_debug_wide_forward(const S2DWideNet* shape, const void* obs_dev, int64_t n, void* y_dev, void* greedy_dev, char* name,
                                   void* stream) {
  static const char who[] = "s2d_debug_wide_forward";
  if (!shape) { s2d_internal_set_error("s2d_debug_wide_forward: shape is NULL"); return S2D_EINVAL; }
  ActorPlanBuf buf;
  int rc = s2d_internal_wide_plan(who, shape, &buf);
  if (rc == S2D_OK) rc = debug_forward_args(who, shape->params, obs_dev, n, y_dev, greedy_dev);
  if (rc == S2D_OK) rc = wide_workspace(who, shape, plan_of<WideDims>(buf).d);
  if (rc != S2D_OK) return rc;
  ActorPlan<WideDims> pl = plan_of<WideDims>(buf);
  pl.d.wf = static_cast<const float*>(shape->workspace);
  rc = debug_forward_launch(who, reinterpret_cast<const void*>(s2d_debug_wide_forward_kernel), pl, n, [&](unsigned blocks, int threads) {
    launch_pack(pl.d, shape, static_cast<hipStream_t>(stream));
    hipLaunchKernelGGL(s2d_debug_wide_forward_kernel, dim3(blocks), dim3(threads), pl.lds, static_cast<hipStream_t>(stream), pl.d,
                       static_cast<const float*>(obs_dev), n, static_cast<float*>(y_dev), static_cast<int32_t*>(greedy_dev), pl.wave_words);
  });
  if (rc == S2D_OK && name)
    std::snprintf(name, 96, "s2d_debug_wide_forward_kernel<act=%s,h=%s,a=%d,waves=%d,tiles=%d>", kActName[shape->activation],
                  widths_text(shape).c_str(), shape->n_out, pl.waves, pl.d.tiles);
  return rc;
}
