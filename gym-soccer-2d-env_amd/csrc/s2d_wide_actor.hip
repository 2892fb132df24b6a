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

// host side (same library, hidden symbols; the rollouts' C entry points are in s2d_engine.hip, s2d_wide_workspace_bytes and
// s2d_debug_wide_forward at the end of this file; the plan is in s2d_wide_net.h)
using WideQNetKernel = void (*)(S2DHot, const S2DRare*, float*, int64_t, int64_t, int, WideDims, const float*, const float*,
                                RolloutOut, float*, StepOut, int);
using WideTanhKernel = void (*)(S2DHot, const S2DRare*, float*, int64_t, int64_t, int, WideDims, const float*, const float*,
                                RolloutOut, float*, StepOut, int, const float*);

// slots of allow_lds_slot (s2d_actor_net.h): the Q-actor's 3, the tanh actor's 2 x 3 x 2, then s2d_debug_wide_forward's
static constexpr int kWideSlots = 3 + 2 * 3 * 2 + 1;
static bool allow_lds(const void* fn, int slot) { return allow_lds_slot<kWideSlots>(fn, slot); }

extern "C" void s2d_internal_set_error(const char* msg);

static const char* const kActName[3] = {"relu", "tanh", "sigmoid"};

// "400-300"
static std::string widths_text(const S2DWideNet* net) {
  std::string s;
  for (int l = 0; l < net->n_hidden; ++l) s += (l ? "-" : "") + std::to_string(net->hidden[l]);
  return s;
}

static size_t workspace_bytes(const WideDims& d) { return ((size_t)d.nfrag * kWave + d.nbias) * sizeof(float); }

// The shape of `net` (everything but the engine's side of n_out and the pointers): 0 and the plan, or S2D_EINVAL with the
// error text set (`who` = the entry point's name).  S2D_WIDE_PLAN=waves,tiles in the environment, read at every launch, overrides
// the plan's choice of waves per workgroup and env tiles per pass (testing: the results do not depend on them); a pair that is
// not of {4, 2, 1} or does not fit the LDS is refused.
static int wide_plan(const char* who, const S2DWideNet* net, WideDims* d, int* wave_words, int* waves, size_t* lds) {
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
  if (!wide_plan_lds(net->n_hidden, net->hidden, net->n_out, net->activation, fw, ft, *d, *wave_words, *waves, *lds)) {
    s2d_internal_set_error((w + ": S2D_WIDE_PLAN=" + (env ? env : "") + " is not waves,tiles of {4, 2, 1} that fit the LDS for 10-" +
                            widths_text(net) + "-" + std::to_string(net->n_out)).c_str());
    return S2D_EINVAL;
  }
  return S2D_OK;
}

// the workspace of a checked shape: S2D_EINVAL with the text set if it is NULL, misaligned or too small
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

// the shape check alone, for the entry points of s2d_engine.hip (they check their engine's side and the other pointers
// themselves; the workspace is checked by the launch functions below, before anything is enqueued)
extern "C" int s2d_internal_wide_check(const char* who, const S2DWideNet* net) {
  WideDims d;
  int wave_words, waves;
  size_t lds;
  return wide_plan(who, net, &d, &wave_words, &waves, &lds);
}

// params -> workspace in fragment order, on `stream`
static void launch_pack(WideDims& d, const S2DWideNet* net, hipStream_t stream) {
  d.wf = static_cast<const float*>(net->workspace);
  const int words = d.nfrag * kWave + d.nbias;
  hipLaunchKernelGGL(s2d_wide_pack_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, d, net->params,
                     static_cast<float*>(net->workspace));
}

// launches the pack kernel and the Q-network actor rollout of a checked network: 0, S2D_EINVAL (the error text set), or -2 on a
// HIP failure
extern "C" int s2d_internal_rollout_qnet_wide(int nk, const S2DHot* hot, const S2DRare* rare_dev, float* S, int64_t stride, int64_t n,
                                              int n_steps, const S2DWideNet* net, const RolloutOut* ro, float* term_rec,
                                              const StepOut* o, void* stream, char* name, size_t name_bytes) {
  WideDims d;
  int wave_words, waves;
  size_t lds;
  if (wide_plan("s2d_rollout_qnet_wide", net, &d, &wave_words, &waves, &lds) != S2D_OK) return S2D_EINVAL;
  if (wide_workspace("s2d_rollout_qnet_wide", net, d) != S2D_OK) return S2D_EINVAL;
  static const WideQNetKernel table[3] = {s2d_reach_actor_rollout_kernel<S2D_MODE_DISCRETE, S2D_NK_OFF, false, WideDims>,
                                           s2d_reach_actor_rollout_kernel<S2D_MODE_DISCRETE, S2D_NK_LATTICE, false, WideDims>,
                                           s2d_reach_actor_rollout_kernel<S2D_MODE_DISCRETE, S2D_NK_SQUARE, false, WideDims>};
  if (!allow_lds(reinterpret_cast<const void*>(table[nk]), nk)) return -2;
  launch_pack(d, net, static_cast<hipStream_t>(stream));
  const int threads = waves * kWave;
  const unsigned blocks = (unsigned)((n + threads - 1) / threads);
  hipLaunchKernelGGL(table[nk], dim3(blocks), dim3(threads), lds, static_cast<hipStream_t>(stream), *hot, rare_dev, S, stride, n,
                     n_steps, d, net->params, net->epsilon, *ro, term_rec, *o, wave_words);
  if (name)
    std::snprintf(name, name_bytes, "s2d_wide_qnet_rollout_kernel<noise=%d,act=%s,h=%s,a=%d,waves=%d,tiles=%d>", nk,
                  kActName[net->activation], widths_text(net).c_str(), net->n_out, waves, d.tiles);
  return 0;
}

// mode = S2D_MODE_CONT1 | S2D_MODE_TURN4 (n_out = 1 | 4), the noise kind is net's
extern "C" int s2d_internal_rollout_actor_wide(int mode, int nk, const S2DHot* hot, const S2DRare* rare_dev, float* S, int64_t stride,
                                               int64_t n, int n_steps, const S2DWideNet* net, const RolloutOut* ro, float* term_rec,
                                               const StepOut* o, void* stream, char* name, size_t name_bytes) {
  WideDims d;
  int wave_words, waves;
  size_t lds;
  if (wide_plan("s2d_rollout_actor_wide", net, &d, &wave_words, &waves, &lds) != S2D_OK) return S2D_EINVAL;
  if (wide_workspace("s2d_rollout_actor_wide", net, d) != S2D_OK) return S2D_EINVAL;
#define S2D_WIDE_ROW(M)                                                                                                       \
  {s2d_reach_actor_rollout_kernel<M, S2D_NK_OFF, false, WideDims, const float*>, s2d_reach_actor_rollout_kernel<M, S2D_NK_LATTICE, false, WideDims, const float*>, \
   s2d_reach_actor_rollout_kernel<M, S2D_NK_SQUARE, false, WideDims, const float*>, s2d_reach_actor_rollout_kernel<M, S2D_NK_OFF, true, WideDims, const float*>,   \
   s2d_reach_actor_rollout_kernel<M, S2D_NK_LATTICE, true, WideDims, const float*>, s2d_reach_actor_rollout_kernel<M, S2D_NK_SQUARE, true, WideDims, const float*>}
  static const WideTanhKernel table[2][6] = {S2D_WIDE_ROW(S2D_MODE_CONT1), S2D_WIDE_ROW(S2D_MODE_TURN4)};
#undef S2D_WIDE_ROW
  const int gauss = net->noise_kind ? 1 : 0;
  const int m = mode == S2D_MODE_TURN4 ? 1 : 0, v = 3 * gauss + nk;
  const WideTanhKernel k = table[m][v];
  if (!allow_lds(reinterpret_cast<const void*>(k), 3 + 6 * m + v)) return -2;
  launch_pack(d, net, static_cast<hipStream_t>(stream));
  const int threads = waves * kWave;
  const unsigned blocks = (unsigned)((n + threads - 1) / threads);
  hipLaunchKernelGGL(k, dim3(blocks), dim3(threads), lds, static_cast<hipStream_t>(stream), *hot, rare_dev, S, stride, n, n_steps, d,
                     net->params, net->epsilon, *ro, term_rec, *o, wave_words, gauss ? net->noise : nullptr);
  if (name)
    std::snprintf(name, name_bytes, "s2d_wide_actor_rollout_kernel<mode=%s,noise=%d,gauss=%d,act=%s,h=%s,a=%d,waves=%d,tiles=%d>",
                  m ? "turn4" : "cont1", nk, gauss, kActName[net->activation], widths_text(net).c_str(), net->n_out, waves, d.tiles);
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
  if (!shape) { s2d_internal_set_error("s2d_debug_wide_forward: shape is NULL"); return S2D_EINVAL; }
  WideDims d;
  int wave_words, waves;
  size_t lds;
  int rc = wide_plan("s2d_debug_wide_forward", shape, &d, &wave_words, &waves, &lds);
  if (rc != S2D_OK) return rc;
  const char* err = nullptr;
  if (n < 1 || n > INT32_MAX) err = "s2d_debug_wide_forward: n must be in [1, 2^31 - 1]";
  else if (!shape->params || (reinterpret_cast<uintptr_t>(shape->params) & 15u))
    err = "s2d_debug_wide_forward: params must be a non-NULL, 16-byte aligned device pointer";
  else if (!obs_dev || !y_dev || !greedy_dev ||
           ((reinterpret_cast<uintptr_t>(obs_dev) | reinterpret_cast<uintptr_t>(y_dev) | reinterpret_cast<uintptr_t>(greedy_dev)) & 3u))
    err = "s2d_debug_wide_forward: obs, y and greedy must be non-NULL, 4-byte aligned device pointers";
  if (err) { s2d_internal_set_error(err); return S2D_EINVAL; }
  rc = wide_workspace("s2d_debug_wide_forward", shape, d);
  if (rc != S2D_OK) return rc;
  if (!allow_lds(reinterpret_cast<const void*>(s2d_debug_wide_forward_kernel), kWideSlots - 1)) {
    s2d_internal_set_error("s2d_debug_wide_forward: hipGetDevice or hipFuncSetAttribute failed");
    return S2D_EHIP;
  }
  launch_pack(d, shape, static_cast<hipStream_t>(stream));
  const int threads = waves * kWave;
  const unsigned blocks = (unsigned)((n + threads - 1) / threads);
  hipLaunchKernelGGL(s2d_debug_wide_forward_kernel, dim3(blocks), dim3(threads), lds, static_cast<hipStream_t>(stream), d,
                     static_cast<const float*>(obs_dev), n, static_cast<float*>(y_dev), static_cast<int32_t*>(greedy_dev), wave_words);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    s2d_internal_set_error((std::string("s2d_debug_wide_forward: launch: ") + hipGetErrorString(e)).c_str());
    return S2D_EHIP;
  }
  if (name)
    std::snprintf(name, 96, "s2d_debug_wide_forward_kernel<act=%s,h=%s,a=%d,waves=%d,tiles=%d>", kActName[shape->activation],
                  widths_text(shape).c_str(), shape->n_out, waves, d.tiles);
  return S2D_OK;
}
