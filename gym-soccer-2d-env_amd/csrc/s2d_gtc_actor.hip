// s2d_gtc_actor.hip -- the fused actors of the GoToCenter task (include/s2d_gtc.h; DESIGN.md sections 4, 5): the epsilon-greedy
// Q-network (s2d_gtc_rollout_qnet, discrete engines) and the deterministic tanh policy with optional Gaussian action noise
// (s2d_gtc_rollout_actor, continuous and turn-mode engines), evaluated inside the rollout kernel on each env's own 4-word
// observation.  One network back end: the streamed-weight MLP of s2d_wide_net.h with input width 4 (4 -> h_1 -> ... -> h_L -> A,
// L = 1 .. 5, widths multiples of 4 up to 400, relu / tanh_spec / sigmoid_spec), its fragments written into the caller's workspace
// by the pack kernel (s2d_wide_pack.hip) on the same stream ahead of every rollout; the shape's checks, the workspace's, the plan
// and the diagnostic's host half are shared with the network's other users (s2d_wide_host.h, s2d_wide_net.h,
// s2d_actor_rollout.h).  The environment half is s2d_gtc_device.h's, word for word what s2d_gtc_rollout runs.
//
// lane = env, 64 envs a wave, four 16-env tiles; waves per workgroup and env tiles per pass come from the plan.  LDS: the
// biases (block-shared, net_pack before the one barrier), then per wave [image A | image B | q 64 x qpitch | obs tile 64 x 4].
// Every draw of env g in episode j at step s is philox(g, j, (stream << 16) | s, seed), the keying of s2d_gtc_rollout's random
// policy: stream 9 = explore or not, POLICY = the random action, 10 = the Gaussian noise, SELECT = the turn / dash uniform.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>

#include "s2d_actor_rollout.h"
#include "s2d_gtc_device.h"
#include "s2d_wide_net.h"

static constexpr int kGtcIn = S2D_GTC_OBS_DIM;
static constexpr int kGtcTail = kWave * kGtcIn;          // a wave's LDS part ends with its observation tile; no PrepTile
enum { S2D_GTC_ST_EXPLORE = 9, S2D_GTC_ST_GAUSS = 10 };  // Philox streams no engine uses

// the wave's parts of the LDS behind the block's biases
struct GtcWaveLds { float *ha, *hb, *qv, *tile; };
S2D_DEV GtcWaveLds gtc_wave_lds(const WideDims& d, float* smem, int wv, int wave_words) {
  GtcWaveLds w;
  w.ha = smem + net_shared_words(d) + wv * wave_words;
  w.hb = w.ha + 16 * d.pitch;
  w.qv = w.hb + 16 * d.pitch;
  w.tile = w.qv + kWave * d.qpitch;
  return w;
}

// QHEAD: the Q-network's epsilon-greedy argmax on a discrete engine; else the tanh policy with epsilon-random exploration on a
// continuous or turn-mode engine (p.adim outputs), GAUSS: plus clip(. + mu_j + sigma_j z_j), noise = [2][p.adim] (mu, sigma).
template <bool QHEAD, bool GAUSS>
__global__ __launch_bounds__(kBlock) void s2d_gtc_actor_rollout_kernel(GParams p, GPtrs q, int64_t n, int n_steps, WideDims d,
                                                                       const float* __restrict__ eps_dev,
                                                                       const float* __restrict__ noise, GRoll ro,
                                                                       float* __restrict__ term_rec, int wave_words) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t wave_first = i - lane;
  net_pack(d, nullptr, smem);
  const GtcWaveLds L = gtc_wave_lds(d, smem, wv, wave_words);
  __syncthreads();
  if (wave_first >= n) return;

  const bool active = i < n;
  const uint64_t thr = explore_threshold(*eps_dev);
  GEnv e{0, 0, 0, 0, 0, 0, 0};
  uint32_t gl = 0, gh = 0;
  float4 ob = make_float4(0, 0, 0, 0);
  if (active) {
    g_load(q, i, e);
    const uint64_t gid = (((uint64_t)p.gid_hi << 32) | p.gid_lo) + (uint64_t)i;
    gl = (uint32_t)gid; gh = (uint32_t)(gid >> 32);
    ob = g_obs(e);                                         // what the last step / reset returned for this state
  }
  float reward = 0.0f; int done = 0, res = 0;
  unsigned int c1 = 0, c2 = 0, c3 = 0;
  for (int t = 0; t < n_steps; ++t) {
    // the action of step t from the observation returned by step t - 1 (the launch's start state at t = 0)
    wave_lds_fence();
    reinterpret_cast<float4*>(L.tile)[lane] = ob;          // zeros in the lanes past n
    wave_lds_fence();
    int greedy = 0;
    float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (QHEAD) {
      greedy = net_forward<true, kGtcIn>(d, smem, L.ha, L.hb, L.qv, L.tile, lane);
    } else {
      net_forward<false, kGtcIn>(d, smem, L.ha, L.hb, L.qv, L.tile, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = L.qv[lane * d.qpitch + j];   // A <= 4 of the 16 rows of the one output tile
      wave_lds_fence();
    }
    if (active) {
      const uint32_t ep = (uint32_t)e.episode, sc = (uint32_t)e.step_count;
      const int64_t row = (int64_t)t * n + i;
      const bool explore = (uint64_t)philox4x32_10(gl, gh, ep, (S2D_GTC_ST_EXPLORE << 16) | sc, p.seed_lo, p.seed_hi).x < thr;
      Action4 a{0.0f, 0.0f, 0.0f, 0.0f};
      float u = 0.0f;
      if (explore) {                                       // the random policy's own draw for the mode
        const U4 w = philox4x32_10(gl, gh, ep, (S2D_ST_POLICY << 16) | sc, p.seed_lo, p.seed_hi);
        if (QHEAD) a.a0 = (float)rnd_below(w.x, 16);
        else {
          a.a0 = rnd_u01(w.x) * 2.0f - 1.0f;
          if (p.adim > 1) a.a1 = rnd_u01(w.y) * 2.0f - 1.0f;
          if (p.adim > 2) a.a2 = rnd_u01(w.z) * 2.0f - 1.0f;
          if (p.adim > 3) a.a3 = rnd_u01(w.w) * 2.0f - 1.0f;
        }
      } else if (QHEAD) {
        a.a0 = (float)greedy;
      } else {
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f}, z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (GAUSS) {
          const U4 w = philox4x32_10(gl, gh, ep, (S2D_GTC_ST_GAUSS << 16) | sc, p.seed_lo, p.seed_hi);
          box_muller(w.x, w.y, z[0], z[1]);
          box_muller(w.z, w.w, z[2], z[3]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j < p.adim) {
            v[j] = tanh_spec(y[j]);
            if constexpr (GAUSS) {
              const float s = v[j] + fmaf(noise[p.adim + j], z[j], noise[j]);
              v[j] = s < -1.0f ? -1.0f : s > 1.0f ? 1.0f : s;
            }
          }
        }
        a = Action4{v[0], v[1], v[2], v[3]};
      }
      if (p.turn && p.continuous && p.use_turn)            // the uniform of :151: the SELECT stream, as s2d_gtc_rollout
        u = rnd_u01(philox4x32_10(gl, gh, ep, (S2D_ST_SELECT << 16) | sc, p.seed_lo, p.seed_hi).x);
      if (ro.action) {
        if (QHEAD) static_cast<int32_t*>(ro.action)[row] = (int32_t)a.a0;
        else {
          float* ar = static_cast<float*>(ro.action) + row * p.adim;
          ar[0] = a.a0;
          if (p.adim > 1) ar[1] = a.a1;
          if (p.adim > 2) ar[2] = a.a2;
          if (p.adim > 3) ar[3] = a.a3;
        }
      }
      g_step(p, e, a, u, reward, done, res);
      ob = g_obs(e);
      c1 += res == 1; c2 += res == 2; c3 += res == 3;
      if (term_rec && done) reinterpret_cast<float4*>(term_rec)[row] = ob;   // the observation the episode ended on
      if (done && p.auto_reset) {
        reinterpret_cast<float4*>(q.terminal_obs)[i] = ob;
        g_reset(p, e, gl, gh);
        ob = g_obs(e);
      }
      if (ro.obs) reinterpret_cast<float4*>(ro.obs)[row] = ob;
      if (ro.reward) ro.reward[row] = reward;
      if (ro.done) ro.done[row] = (uint8_t)done;
      if (ro.result) ro.result[row] = (uint8_t)res;
    }
  }
  if (active) {
    g_store(q, i, e);
    reinterpret_cast<float4*>(q.obs)[i] = ob; q.reward[i] = reward; q.done[i] = (uint8_t)done; q.result[i] = (uint8_t)res;
  }
  // the striped counters as s2d_gtc_rollout leaves them: the stripe of the 256 envs this wave belongs to
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { c1 += __shfl_down(c1, off); c2 += __shfl_down(c2, off); c3 += __shfl_down(c3, off); }
  unsigned long long* st = q.stats + ((wave_first / 256) % S2D_STATS_STRIPES) * 8;
  if (lane == 0) {
    if (c1) atomicAdd(&st[1], (unsigned long long)c1);
    if (c2) atomicAdd(&st[2], (unsigned long long)c2);
    if (c3) atomicAdd(&st[3], (unsigned long long)c3);
    if (wave_first == 0) atomicAdd(&st[0], (unsigned long long)n * (unsigned long long)n_steps);
  }
}

// ------------------------------------------------------------------------------------------ host side
static const char kBytesFn[] = "s2d_gtc_actor_workspace_bytes";

// The plan of `net`'s shape: wide_net_plan with the 4-word observation and its tile as the tail.  S2D_WIDE_PLAN overrides the
// plan's choice, as for the reach-ball actors.
static int gtc_plan(const char* who, const S2DWideNet* net, ActorPlan<WideDims>& pl) {
  return wide_net_plan(who, net, kGtcIn, kGtcTail, pl.d, pl.wave_words, pl.waves, pl.lds);
}

S2D_API size_t s2d_gtc_actor_workspace_bytes(const S2DWideNet* shape) { return wide_net_workspace_bytes(shape, kGtcIn); }

// both entry points: every check, then the pack kernel and the rollout
static int gtc_rollout(const char* who, bool qhead, S2DGtcHandle h, int n_steps, const S2DWideNet* net, const S2DGtcRollout* out,
                       float* terminal_obs, void* stream) {
  using Kernel = void (*)(GParams, GPtrs, int64_t, int, WideDims, const float*, const float*, GRoll, float*, int);
  static const Kernel table[3] = {s2d_gtc_actor_rollout_kernel<true, false>, s2d_gtc_actor_rollout_kernel<false, false>,
                                  s2d_gtc_actor_rollout_kernel<false, true>};
  const std::string w(who);
  if (!h) return fail(w, "NULL handle");
  if (!net) return fail(w, "net is NULL");
  if (n_steps < 0) return fail(w, "n_steps must be >= 0");
  const GParams& gp = h->gp;
  if (qhead && gp.continuous) return fail(w, "the Q head needs a discrete engine (this one is continuous): use s2d_gtc_rollout_actor");
  if (!qhead && !gp.continuous) return fail(w, "the tanh head needs a continuous engine (this one is discrete): use s2d_gtc_rollout_qnet");
  ActorPlan<WideDims> pl;
  if (gtc_plan(who, net, pl) != S2D_OK) return S2D_EINVAL;
  const int want = qhead ? 16 : gp.adim;
  if (net->n_out != want)
    return fail(w, "n_out is " + std::to_string(net->n_out) + ", the engine's " + (qhead ? "action count" : "action width") + " is " +
                       std::to_string(want));
  if (qhead ? net->noise_kind != 0 : (net->noise_kind != 0 && net->noise_kind != 1))
    return fail(w, qhead ? "noise_kind must be 0 for the Q head" : "noise_kind must be 0 or 1");
  if (net->noise_kind == 1 && (!net->noise || (reinterpret_cast<uintptr_t>(net->noise) & 3u)))
    return fail(w, "noise_kind = 1 needs noise, a 4-byte aligned device buffer [2][n_out]");
  if (!net->params || (reinterpret_cast<uintptr_t>(net->params) & 15u))
    return fail(w, "params must be a non-NULL, 16-byte aligned device pointer");
  if (!net->epsilon || (reinterpret_cast<uintptr_t>(net->epsilon) & 3u))
    return fail(w, "epsilon must be a non-NULL, 4-byte aligned device pointer");
  const WidePackArgs pack = wide_pack_args(pl.d, kGtcIn);
  if (wide_net_workspace(w, net, pack, kBytesFn) != S2D_OK) return S2D_EINVAL;
  if ((reinterpret_cast<uintptr_t>(terminal_obs) & 15u) || (out && (reinterpret_cast<uintptr_t>(out->obs) & 15u)))
    return fail(w, "the obs and terminal_obs records must be 16-byte aligned");
  if (n_steps == 0) return S2D_OK;
  if (hipSetDevice(h->device) != hipSuccess) { s2d_internal_set_error((w + ": hipSetDevice failed").c_str()); return S2D_EHIP; }
  const int slot = qhead ? 0 : 1 + (net->noise_kind ? 1 : 0);
  const Kernel k = table[slot];
  if (!allow_lds_slot<WideDims>(reinterpret_cast<const void*>(k), slot)) {
    s2d_internal_set_error((w + ": hipGetDevice or hipFuncSetAttribute failed").c_str());
    return S2D_EHIP;
  }
  pl.d.wf = static_cast<const float*>(net->workspace);
  GRoll ro{nullptr, nullptr, nullptr, nullptr, nullptr};
  if (out) ro = GRoll{out->obs, out->action, out->reward, out->done, out->result};
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int threads = pl.waves * kWave;
  s2d_internal_wide_pack(pack, net->params, net->workspace, s);
  hipLaunchKernelGGL(k, dim3((unsigned)((h->n + threads - 1) / threads)), dim3(threads), pl.lds, s, gp, h->q, h->n, n_steps, pl.d,
                     net->epsilon, net->noise_kind ? net->noise : nullptr, ro, terminal_obs, pl.wave_words);
  if (launched(w) != S2D_OK) return S2D_EHIP;
  const char* const mode = !gp.continuous ? "discrete" : !gp.turn ? "continuous" : gp.use_turn ? "useturn" : "turn";
  std::snprintf(h->name, sizeof h->name, "s2d_gtc_actor_rollout_kernel<head=%s,mode=%s,gauss=%d,act=%s,h=%s,a=%d,waves=%d,tiles=%d>",
                qhead ? "q" : "tanh", mode, net->noise_kind ? 1 : 0, kActName[net->activation], widths_text(net).c_str(), net->n_out,
                pl.waves, pl.d.tiles);
  return S2D_OK;
}

S2D_API int s2d_gtc_rollout_qnet(S2DGtcHandle h, int n_steps, const S2DWideNet* net, const S2DGtcRollout* out, float* terminal_obs,
                                 void* stream) {
  return gtc_rollout("s2d_gtc_rollout_qnet", true, h, n_steps, net, out, terminal_obs, stream);
}
S2D_API int s2d_gtc_rollout_actor(S2DGtcHandle h, int n_steps, const S2DWideNet* net, const S2DGtcRollout* out, float* terminal_obs,
                                  void* stream) {
  return gtc_rollout("s2d_gtc_rollout_actor", false, h, n_steps, net, out, terminal_obs, stream);
}
S2D_API const char* s2d_gtc_kernel_name(S2DGtcHandle h) { return h ? h->name : ""; }

S2D_API int s2d_gtc_debug_forward(const S2DWideNet* shape, const void* obs_dev, int64_t n, void* y_dev, void* greedy_dev, char* name,
                                  void* stream) {
  return debug_forward_streamed("s2d_gtc_debug_forward", "s2d_gtc_debug_forward_kernel", kGtcIn, kBytesFn, gtc_plan,
                                s2d_wide_debug_forward_kernel<kGtcIn>, shape, obs_dev, n, y_dev, greedy_dev, name, stream);
}
