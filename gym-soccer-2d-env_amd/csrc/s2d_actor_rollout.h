// s2d_actor_rollout.h -- the rollout kernel of the reach-ball engine's fused actors, as one template over the network it acts
// with, shared by s2d_actor.hip (Dims = QNetDims, the 10-H1-H2-A network of s2d_actor_net.h), s2d_mlp_actor.hip (Dims =
// MlpDims, the general MLP of s2d_mlp_net.h) and s2d_wide_actor.hip (Dims = WideDims, the streamed-weight MLP of s2d_wide_net.h):
// the prologue, the heads (epsilon-greedy argmax; tanh with optional Gaussian action noise), the simulation, the records and the
// statistics.  (Moved out of s2d_actor.hip; the text of the kernel is unchanged but for the type of `d`, so that the QNetDims
// instantiations keep their instructions: profiles/r05/mlp_actor_isa.txt.)  At the end of the file, the kernel's host side as
// one template over the same Dims: the launch tables, the dynamic-LDS attribute and the launch.
//
// Dims: the kernel argument that describes the network.  Beside its fields pitch and qpitch (the row pitches of the wave's two
// hidden images [16] and of its output image [64]) the kernel asks for three overloads on it:
//   net_pack(d, params, smem)            the caller's parameters into the block's LDS (block-wide, before a barrier)
//   net_shared_words(d)                  words of that block-shared part; the waves' parts follow
//   net_forward<ARGMAX>(d, smem, ha, hb, qv, tile, lane)   the network on the wave's observation tile -> qv (and the argmax)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <new>
#include <string>

#include "s2d_actor_launch.h"
#include "s2d_actor_net.h"
#include "s2d_wide_host.h"

// experiment build (-DS2D_QNET_STAMPS, profiles/experiments/qnet_actor_clocks.py): per wave, the shader clocks (s_memtime) of the
// network (observation tile + three layers + argmax), of the rest of the cycle (action draw, simulation, record stores) and of the
// prologue, summed over the launch; lane 0 writes them as floats into terminal_obs row wave_first of the arena
#ifdef S2D_QNET_STAMPS
#define QS_DECL uint64_t qs_net = 0, qs_rest = 0, qs_t = __builtin_amdgcn_s_memtime(); const uint64_t qs_begin = qs_t; uint64_t qs_pro = 0
#define QS_MARK(acc) do { const uint64_t qs_now = __builtin_amdgcn_s_memtime(); acc += qs_now - qs_t; qs_t = qs_now; } while (0)
#define QS_STORE() do { if (lane == 0) { float* q_ = o.terminal_obs + wave_first * S2D_OBS_DIM; q_[0] = (float)qs_net; \
    q_[1] = (float)qs_rest; q_[2] = (float)qs_pro; q_[3] = (float)(__builtin_amdgcn_s_memtime() - qs_begin); } } while (0)
#else
#define QS_DECL do {} while (0)
#define QS_MARK(acc) do {} while (0)
#define QS_STORE() do {} while (0)
#endif

// the deterministic policy's action of one env (lane = env), not exploring: a_j = tanh_spec(y_j), with GAUSS + clip(mu_j +
// sigma_j z_j), z from Box-Muller on POLICY block 3 (TURN4: z0..z3 of the block at counter k; CONT1: z_{k & 3} of the block at
// counter k >> 2, cached in gquad).  noise = [2][A] (mu, sigma) in device memory.
template <int MODE, bool GAUSS>
S2D_DEV Action4 tanh_action(const S2DHot& p, const float* __restrict__ y, const float* __restrict__ noise, uint32_t gl, uint32_t gh,
                            uint32_t k, const U4& gquad) {
  constexpr int A = MODE == S2D_MODE_TURN4 ? 4 : 1;
  float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int j = 0; j < A; ++j) a[j] = tanh_spec(y[j]);
  if constexpr (GAUSS) {
    float z[4];
    if constexpr (MODE == S2D_MODE_TURN4) {
      const U4 w = s2d_draw(p, gl, gh, k, S2D_ST_POLICY, 3);
      box_muller(w.x, w.y, z[0], z[1]);
      box_muller(w.z, w.w, z[2], z[3]);
    } else {
      const bool hi = (k & 2u) != 0u;
      float zc, zs;
      box_muller(hi ? gquad.z : gquad.x, hi ? gquad.w : gquad.y, zc, zs);
      z[0] = (k & 1u) ? zs : zc;
    }
#pragma unroll
    for (int j = 0; j < A; ++j) {
      const float v = a[j] + fmaf(noise[A + j], z[j], noise[j]);
      a[j] = v < -1.0f ? -1.0f : v > 1.0f ? 1.0f : v;
    }
  }
  return Action4{a[0], a[1], a[2], a[3]};
}

// the noise buffer of the tanh-head instantiations (Noise = const float*); the Q-actor's have no such argument
S2D_DEV const float* actor_noise() { return nullptr; }
S2D_DEV const float* actor_noise(const float* p) { return p; }

// The fused rollout of both actors.  MODE = S2D_MODE_DISCRETE: the Q-network's epsilon-greedy argmax (s2d_rollout_qnet);
// CONT1 / TURN4: the deterministic tanh policy with epsilon-random exploration and optional Gaussian action noise (GAUSS,
// s2d_rollout_actor).  One body, so that both share the prologue, the simulation, the records and the epilogue.  The noise
// buffer is a trailing argument pack, empty for the Q-actor, so that its kernel arguments, and its code, stay as they were.
template <int MODE, int NK, bool GAUSS, typename Dims, typename... Noise>
__global__ __launch_bounds__(kBlock) void s2d_reach_actor_rollout_kernel(S2DHot p_sgpr, const S2DRare* __restrict__ rp,
                                                                         float* __restrict__ S, int64_t stride, int64_t n,
                                                                         int n_steps, Dims d, const float* __restrict__ params,
                                                                         const float* __restrict__ eps_dev, RolloutOut ro,
                                                                         float* __restrict__ term_rec, StepOut o, int wave_words,
                                                                         Noise... noise_arg) {
  const float* __restrict__ noise = actor_noise(noise_arg...);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  QS_DECL;
  const S2DHot p = hot_in_vgprs(p_sgpr);
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t wave_first = i - lane;

  // ---- the network in fragment order (block-wide, once per launch)
  net_pack(d, params, smem);
  float* const wbase = smem + net_shared_words(d) + wv * wave_words;
  float* const ha = wbase;
  float* const hb = ha + 16 * d.pitch;
  float* const qv = hb + 16 * d.pitch;
  float* const tile = qv + kWave * d.qpitch;
  PrepTile* const prep = reinterpret_cast<PrepTile*>(tile + kObsTile);
  __syncthreads();
  if (wave_first >= n) return;

  const bool active = i < n;
  int64_t rows = n - wave_first; if (rows > kWave) rows = kWave;
  const int valid = (int)rows * S2D_OBS_DIM;
  const uint64_t thr = explore_threshold(*eps_dev);
  uint32_t* const kplane = reinterpret_cast<uint32_t*>(S + F_POLICY * stride);
  Env e;
  uint32_t gl = 0, gh = 0, k0 = 0;
  ObsOut ob;
#pragma unroll
  for (int k = 0; k < S2D_OBS_DIM; ++k) ob.o[k] = 0.0f;
  if (active) {
    env_load(e, S, stride, i);
    k0 = kplane[i];
    uint64_t gid = (((uint64_t)p.gid_hi << 32) | p.gid_lo) + (uint64_t)i;
    gl = (uint32_t)gid; gh = (uint32_t)(gid >> 32);
    observe(p, e.px, e.py, e.body, e.bx, e.by, e.bvx, e.bvy, ob);   // what the last step / reset returned for this state
  }
  float reward = 0.0f, dir = 0.0f; int done = 0, res = 0, cmd = 0;
  unsigned int cnt1 = 0, cnt2 = 0, cnt3 = 0;
  float* const term_row = o.terminal_obs + i * S2D_OBS_DIM;
  U4 quad{0, 0, 0, 0}, equad{0, 0, 0, 0}, squad{0, 0, 0, 0}, gquad{0, 0, 0, 0};
  bool have_prep = false;
  uint32_t* const coop_scratch = reinterpret_cast<uint32_t*>(tile);
  if (p.auto_reset) {
    prep_fill_coop<NK>(p, rp, *prep, lane, active ? reset_key(e) : 0u, gl, gh, active, coop_scratch);
    have_prep = active;
  }
  int n_missing = 0;
  int64_t row = 0;
  QS_MARK(qs_pro);
  for (int t = 0; t < n_steps; ++t, row += n) {
    res = 0;
    if (n_missing >= kRefillMin) {
      if (active && !have_prep) { prep_fill<NK>(p, rp, *prep, lane, e, gl, gh); have_prep = true; }
      n_missing = 0;
    }
    // the action of step t from the observation returned by step t - 1 (the launch's start state at t = 0)
    wave_lds_fence();
    tile_write(tile, ob, lane, active);
    wave_lds_fence();
    int greedy = 0;
    float y[4];
    if constexpr (MODE == S2D_MODE_DISCRETE) {
      greedy = net_forward<true>(d, smem, ha, hb, qv, tile, lane);
    } else {
      net_forward<false>(d, smem, ha, hb, qv, tile, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = qv[lane * d.qpitch + j];   // A <= 4 of the 16 rows of the one output tile
      wave_lds_fence();
    }
    QS_MARK(qs_net);
    if (active) {
      const uint32_t k = k0 + (uint32_t)t;
      CmdPrep c;
      if constexpr (MODE == S2D_MODE_DISCRETE) {
        if (t == 0 || (k & 3u) == 0u) {
          quad = policy_quad(p, gl, gh, k, S2D_ST_POLICY);                      // block 0: S2D_ACT_RANDOM's draw
          equad = s2d_draw(p, gl, gh, k >> 2, S2D_ST_POLICY, 2);                // block 2: explore or not
        }
        const bool explore = (uint64_t)quad_word(equad, k) < thr;
        const int a = explore ? rnd_below(quad_word(quad, k), (uint32_t)p.n_actions) : greedy;
        if (ro.action) static_cast<int32_t*>(ro.action)[row + i] = a;
        c = decode_action<S2D_MODE_DISCRETE>(p, Action4{(float)a, 0.0f, 0.0f, 0.0f}, gl, gh, k, false, squad, cmd, dir);
      } else {
        const bool refresh = t == 0 || (k & 3u) == 0u;
        if (refresh) {
          equad = s2d_draw(p, gl, gh, k >> 2, S2D_ST_POLICY, 2);                // block 2: explore or not
          if (MODE == S2D_MODE_CONT1) quad = policy_quad(p, gl, gh, k, S2D_ST_POLICY);              // block 0: the random action
          if (GAUSS && MODE == S2D_MODE_CONT1) gquad = s2d_draw(p, gl, gh, k >> 2, S2D_ST_POLICY, 3);   // block 3: noise
        }
        const bool explore = (uint64_t)quad_word(equad, k) < thr;
        const Action4 a = explore ? random_action<MODE>(p, gl, gh, k, quad, false) : tanh_action<MODE, GAUSS>(p, y, noise, gl, gh, k, gquad);
        if (ro.action) store_rollout_action<MODE>(ro.action, row + i, a);
        c = decode_action<MODE>(p, a, gl, gh, k, refresh, squad, cmd, dir);
      }
      step_env<NK, false>(p, rp, e, gl, gh, k, cmd, c, ob, reward, done, res, term_row, prep, lane, have_prep);
      if (ro.reward) ro.reward[row + i] = reward;
      if (ro.done) ro.done[row + i] = (uint8_t)done;
      if (ro.result) ro.result[row + i] = (uint8_t)res;
      if (term_rec && done) {                              // the observation the finished episode ended on
        float* const dst = term_rec + (row + i) * S2D_OBS_DIM;
#pragma unroll
        for (int k2 = 0; k2 < S2D_OBS_DIM; ++k2) dst[k2] = p.auto_reset ? term_row[k2] : ob.o[k2];
      }
      cnt1 += res == S2D_RESULT_GOAL; cnt2 += res == S2D_RESULT_OUT; cnt3 += res == S2D_RESULT_TIMEOUT;
    }
    if (p.auto_reset) n_missing += __popcll(__ballot(active && done != 0));
    if (ro.obs) store_obs_tile(tile, ob, lane, active, ro.obs + (row + wave_first) * S2D_OBS_DIM, valid);
    QS_MARK(qs_rest);
  }
  if (active) {
    env_store(e, S, stride, i);
    kplane[i] = k0 + (uint32_t)n_steps;
    o.reward[i] = reward; o.done[i] = (uint8_t)done; o.result[i] = (uint8_t)res;
    o.action_dir[i] = dir; o.action_cmd[i] = (uint8_t)cmd;
  }
  store_obs_tile(tile, ob, lane, active, o.obs + wave_first * S2D_OBS_DIM, valid);
  if (!active) { cnt1 = cnt2 = cnt3 = 0; }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    cnt1 += __shfl_xor(cnt1, off); cnt2 += __shfl_xor(cnt2, off); cnt3 += __shfl_xor(cnt3, off);
  }
  unsigned long long* const srow = stats_row(o.stats, wave_first);
  stats_store(srow, lane, stats_load(srow, lane), wave_first == 0 ? (unsigned long long)n * (unsigned long long)n_steps : 0ull, cnt1, cnt2, cnt3);
  QS_STORE();
}

// ------------------------------------------------------------------------------------------ host side
// (allow_lds_slot<Owner>, the dynamic-LDS limit of an instantiation, is s2d_wide_host.h's)
// a back end's plan for one network: its kernel argument, the LDS words of a wave, the waves of a workgroup, the LDS bytes; and
// its place in the buffer the entry points carry
template <typename Dims>
struct ActorPlan {
  Dims d;
  int wave_words, waves;
  size_t lds;
};
template <typename Dims>
static ActorPlan<Dims>& plan_in(ActorPlanBuf* buf) {
  static_assert(sizeof(ActorPlan<Dims>) <= sizeof buf->bytes && alignof(ActorPlan<Dims>) <= alignof(ActorPlanBuf), "ActorPlanBuf");
  return *new (buf->bytes) ActorPlan<Dims>;
}
template <typename Dims>
static const ActorPlan<Dims>& plan_of(const ActorPlanBuf& buf) { return *reinterpret_cast<const ActorPlan<Dims>*>(buf.bytes); }

// "128-64-32-16" (Net = S2DMlpNet | S2DWideNet)
template <typename Net>
static std::string widths_text(const Net* net) {
  std::string s;
  for (int l = 0; l < net->n_hidden; ++l) s += (l ? "-" : "") + std::to_string(net->hidden[l]);
  return s;
}

// The rollout of a planned network with the head of the engine's mode: the Q head on a discrete engine, the tanh head on a
// continuous or turning one (`noise` non-NULL: with Gaussian action noise).  `before()` enqueues what has to run ahead of the
// rollout on the same stream (the wide back end's pack kernel); it is called once nothing can fail any more.  false, with
// nothing enqueued, if hipGetDevice or hipFuncSetAttribute failed.
template <typename Dims, typename Before>
static bool launch_actor_rollout(const ActorRollout& a, const ActorPlan<Dims>& pl, const float* params, const float* eps,
                                 const float* noise, Before before) {
  using QKernel = void (*)(S2DHot, const S2DRare*, float*, int64_t, int64_t, int, Dims, const float*, const float*, RolloutOut, float*,
                           StepOut, int);
  using TanhKernel = void (*)(S2DHot, const S2DRare*, float*, int64_t, int64_t, int, Dims, const float*, const float*, RolloutOut,
                              float*, StepOut, int, const float*);
  static const QKernel qtable[3] = {s2d_reach_actor_rollout_kernel<S2D_MODE_DISCRETE, S2D_NK_OFF, false, Dims>,
                                    s2d_reach_actor_rollout_kernel<S2D_MODE_DISCRETE, S2D_NK_LATTICE, false, Dims>,
                                    s2d_reach_actor_rollout_kernel<S2D_MODE_DISCRETE, S2D_NK_SQUARE, false, Dims>};
#define S2D_TANH_ROW(M)                                                                                                                            \
  {s2d_reach_actor_rollout_kernel<M, S2D_NK_OFF, false, Dims, const float*>, s2d_reach_actor_rollout_kernel<M, S2D_NK_LATTICE, false, Dims, const float*>, \
   s2d_reach_actor_rollout_kernel<M, S2D_NK_SQUARE, false, Dims, const float*>, s2d_reach_actor_rollout_kernel<M, S2D_NK_OFF, true, Dims, const float*>,   \
   s2d_reach_actor_rollout_kernel<M, S2D_NK_LATTICE, true, Dims, const float*>, s2d_reach_actor_rollout_kernel<M, S2D_NK_SQUARE, true, Dims, const float*>}
  static const TanhKernel ttable[2][6] = {S2D_TANH_ROW(S2D_MODE_CONT1), S2D_TANH_ROW(S2D_MODE_TURN4)};
#undef S2D_TANH_ROW
  const hipStream_t stream = static_cast<hipStream_t>(a.stream);
  const int threads = pl.waves * kWave;
  const unsigned blocks = (unsigned)((a.n + threads - 1) / threads);
  if (a.mode == S2D_MODE_DISCRETE) {
    const QKernel k = qtable[a.nk];
    if (!allow_lds_slot<Dims>(reinterpret_cast<const void*>(k), a.nk)) return false;
    before();
    hipLaunchKernelGGL(k, dim3(blocks), dim3(threads), pl.lds, stream, *a.hot, a.rare_dev, a.S, a.stride, a.n, a.n_steps, pl.d, params,
                       eps, *a.ro, a.term_rec, *a.o, pl.wave_words);
    return true;
  }
  const int m = a.mode == S2D_MODE_TURN4 ? 1 : 0, v = 3 * (noise ? 1 : 0) + a.nk;
  const TanhKernel k = ttable[m][v];
  if (!allow_lds_slot<Dims>(reinterpret_cast<const void*>(k), 3 + 6 * m + v)) return false;
  before();
  hipLaunchKernelGGL(k, dim3(blocks), dim3(threads), pl.lds, stream, *a.hot, a.rare_dev, a.S, a.stride, a.n, a.n_steps, pl.d, params, eps,
                     *a.ro, a.term_rec, *a.o, pl.wave_words, noise);
  return true;
}

// The host half of s2d_debug_{net,mlp,wide}_forward (`who`).  Its arguments beside the shape: S2D_OK, or S2D_EINVAL with the text set
static inline int debug_forward_args(const std::string& who, const void* params, const void* obs, int64_t n, const void* y, const void* greedy) {
  std::string err;
  if (n < 1 || n > INT32_MAX) err = ": n must be in [1, 2^31 - 1]";
  else if (!params || (reinterpret_cast<uintptr_t>(params) & 15u)) err = ": params must be a non-NULL, 16-byte aligned device pointer";
  else if (!obs || !y || !greedy ||
           ((reinterpret_cast<uintptr_t>(obs) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(greedy)) & 3u))
    err = ": obs, y and greedy must be non-NULL, 4-byte aligned device pointers";
  if (err.empty()) return S2D_OK;
  s2d_internal_set_error((who + err).c_str());
  return S2D_EINVAL;
}

// and its launch: the dynamic-LDS limit of `kernel` (the last slot of Dims' table), then enqueue(blocks, threads), which launches
// the kernel (and whatever goes ahead of it), then the launch's error
template <typename Dims, typename Enqueue>
static int debug_forward_launch(const std::string& who, const void* kernel, const ActorPlan<Dims>& pl, int64_t n, Enqueue enqueue) {
  if (!allow_lds_slot<Dims>(kernel, kLdsSlots - 1)) {
    s2d_internal_set_error((who + ": hipGetDevice or hipFuncSetAttribute failed").c_str());
    return S2D_EHIP;
  }
  const int threads = pl.waves * kWave;
  enqueue((unsigned)((n + threads - 1) / threads), threads);
  return launched(who);
}

// The whole of s2d_debug_wide_forward and s2d_gtc_debug_forward (`who`): the streamed-weight network (Dims = WideDims) with input
// width n_in.  plan(who, shape, pl) is the unit's plan, `kernel` its instantiation of s2d_wide_debug_forward_kernel, kname what
// the kernel is called in `name` (96 bytes or NULL), bytes_fn the entry point that tells the workspace's size.
template <typename Dims, typename Plan>
static int debug_forward_streamed(const char* who, const char* kname, int n_in, const char* bytes_fn, Plan plan,
                                  void (*kernel)(Dims, const float*, int64_t, float*, int32_t*, int), const S2DWideNet* shape,
                                  const void* obs_dev, int64_t n, void* y_dev, void* greedy_dev, char* name, void* stream) {
  if (!shape) return fail(who, "shape is NULL");
  ActorPlan<Dims> pl;
  int rc = plan(who, shape, pl);
  if (rc == S2D_OK) rc = debug_forward_args(who, shape->params, obs_dev, n, y_dev, greedy_dev);
  if (rc == S2D_OK) rc = wide_net_workspace(who, shape, wide_pack_args(pl.d, n_in), bytes_fn);
  if (rc != S2D_OK) return rc;
  pl.d.wf = static_cast<const float*>(shape->workspace);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  rc = debug_forward_launch(who, reinterpret_cast<const void*>(kernel), pl, n, [&](unsigned blocks, int threads) {
    s2d_internal_wide_pack(wide_pack_args(pl.d, n_in), shape->params, shape->workspace, s);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), pl.lds, s, pl.d, static_cast<const float*>(obs_dev), n, static_cast<float*>(y_dev),
                       static_cast<int32_t*>(greedy_dev), pl.wave_words);
  });
  if (rc == S2D_OK && name)
    std::snprintf(name, 96, "%s<act=%s,h=%s,a=%d,waves=%d,tiles=%d>", kname, kActName[shape->activation], widths_text(shape).c_str(),
                  shape->n_out, pl.waves, pl.d.tiles);
  return rc;
}
