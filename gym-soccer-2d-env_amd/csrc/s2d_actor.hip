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
template <int MODE, int NK, bool GAUSS, typename... Noise>
__global__ __launch_bounds__(kBlock) void s2d_reach_actor_rollout_kernel(S2DHot p_sgpr, const S2DRare* __restrict__ rp,
                                                                         float* __restrict__ S, int64_t stride, int64_t n,
                                                                         int n_steps, QNetDims d, const float* __restrict__ params,
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
  static const QNetKernel table[3] = {s2d_reach_actor_rollout_kernel<S2D_MODE_DISCRETE, S2D_NK_OFF, false>,
                                       s2d_reach_actor_rollout_kernel<S2D_MODE_DISCRETE, S2D_NK_LATTICE, false>,
                                       s2d_reach_actor_rollout_kernel<S2D_MODE_DISCRETE, S2D_NK_SQUARE, false>};
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
  {s2d_reach_actor_rollout_kernel<M, S2D_NK_OFF, false, const float*>, s2d_reach_actor_rollout_kernel<M, S2D_NK_LATTICE, false, const float*>,                 \
   s2d_reach_actor_rollout_kernel<M, S2D_NK_SQUARE, false, const float*>, s2d_reach_actor_rollout_kernel<M, S2D_NK_OFF, true, const float*>,                   \
   s2d_reach_actor_rollout_kernel<M, S2D_NK_LATTICE, true, const float*>, s2d_reach_actor_rollout_kernel<M, S2D_NK_SQUARE, true, const float*>}
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
