// s2d_policy.hip -- on-policy collection (PPO / A2C): the fused stochastic policy (s2d_rollout_policy), its head evaluated alone
// (s2d_debug_policy_head) and the advantage scan (s2d_gae); include/s2d.h, DESIGN.md sections 4, 5.
//
// The rollout is the body of s2d_reach_actor_rollout_kernel (s2d_actor.hip): one env per lane, the whole cycle in one wave, T
// cycles per launch, the action of step t chosen from the observation step t - 1 returned.  The network (s2d_actor_net.h) is the
// actors' 10-H1-H2-A MLP on the f32 matrix cores in the k-ordered fmaf spec, with relu or tanh_spec on the hidden accumulators
// (`act`, a wave-uniform kernel argument: both forms are compiled into every kernel, so the activation does not multiply the
// instantiations) and a linear output layer: logits or means.  The head samples from the policy's own distribution and records
// the log-probability of what it took:
//   discrete    categorical over softmax(y): exp_spec / log_spec in a fixed order, u from POLICY block 4;
//   continuous  diagonal Gaussian N(y, exp(log_std)^2) with the state-independent log_std[A] of SB3, z from POLICY block 3
//               (the Gaussian block of the tanh actor); recorded unclipped, the env receives clip(a, -1, 1).
// One device word switches to greedy actions (read when the kernel runs: evaluation is the same captured graph).  There is no
// epsilon in this path.
//
// s2d_gae is engine-independent: raw [T][N] device arrays (the reach-ball and the 11v11 records share that layout), one lane
// per env, a backward scan over T whose loads run a chunk ahead of the recurrence.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#include "s2d_actor_rollout.h"
#include "s2d_head.h"

// ------------------------------------------------------------------------------------------ network
// the three layers on the wave's observation tile with hidden activation ACT (1 relu, 2 tanh_spec): net_forward<false> of
// s2d_actor_net.h with the activation as a parameter
template <int ACT>
S2D_DEV void policy_layers(const QNetDims& d, const float* __restrict__ wl, float* __restrict__ ha, float* __restrict__ hb,
                           float* __restrict__ qv, const float* __restrict__ obs_tile, int lane) {
  const int g = lane >> 4, c = lane & 15;
  const float* w1 = wl;
  const float* w2 = w1 + w1_frags(d) * kWave;
  const float* w3 = w2 + w2_frags(d) * kWave;
  const float* b1 = w3 + w3_frags(d) * kWave;
  const float* b2 = b1 + d.h1;
  const float* b3 = b2 + d.h2;
  for (int nt = 0; nt < 4; ++nt) {
    const float* x = obs_tile + (16 * nt + c) * S2D_OBS_DIM;
    layer_tile<ACT, 3>(w1, b1, d.h1 / 16, 3, [&](int s) { const int k = 4 * s + g; return k < S2D_OBS_DIM ? x[k] : 0.0f; },
                       ha, d.pitch, lane);
    wave_lds_fence();
    layer_tile<ACT, 4>(w2, b2, d.h2 / 16, d.h1 / 4, [&](int s) { return ha[c * d.pitch + 4 * s + g]; }, hb, d.pitch, lane);
    wave_lds_fence();
    layer_tile<S2D_ACT_FN_NONE, 4>(w3, b3, d.na16 / 16, d.h2 / 4, [&](int s) { return hb[c * d.pitch + 4 * s + g]; },
                                   qv + 16 * nt * d.qpitch, d.qpitch, lane);
    wave_lds_fence();
  }
}
// act: 0 relu, 1 tanh (S2DPolicyNet.activation; wave-uniform)
S2D_DEV void policy_forward(const QNetDims& d, int act, const float* __restrict__ wl, float* __restrict__ ha, float* __restrict__ hb,
                            float* __restrict__ qv, const float* __restrict__ obs_tile, int lane) {
  if (act) policy_layers<S2D_ACT_FN_TANH>(d, wl, ha, hb, qv, obs_tile, lane);
  else policy_layers<S2D_ACT_FN_RELU>(d, wl, ha, hb, qv, obs_tile, lane);
}

// ------------------------------------------------------------------------------------------ heads (include/s2d.h: the spec)
// (the categorical head: s2d_head.h, shared with the 11v11 policy slots)

// z0 .. z(A-1) of the Gaussian block (POLICY block 3) at policy step k: the tanh actor's layout (turning: the four of the block
// at counter k; continuous: z_{k & 3} of the block at counter k >> 2, cached in gquad)
template <int MODE>
S2D_DEV void policy_gauss(const S2DHot& p, uint32_t gl, uint32_t gh, uint32_t k, const U4& gquad, float* z) {
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
}
S2D_DEV float clip1(float v) { return v < -1.0f ? -1.0f : v > 1.0f ? 1.0f : v; }

// diagonal-Gaussian head on the means y[0 .. A-1]: a = the recorded action (sampling: unclipped; greedy: clip(y), z = 0 in logp)
template <int A>
S2D_DEV void gaussian_head(const float* y, const float* log_std, const float* sigma, bool det, const float* z, float* a, float& logp) {
  float lp = 0.0f;
#pragma unroll
  for (int j = 0; j < A; ++j) {
    const float zj = det ? 0.0f : z[j];
    a[j] = det ? clip1(y[j]) : fmaf(sigma[j], zj, y[j]);
    const float term = fmaf(-0.5f * zj, zj, -log_std[j]) - 0.91893853f;
    lp = j == 0 ? term : lp + term;
  }
  logp = lp;
}

// ------------------------------------------------------------------------------------------ rollout
template <int MODE, int NK>
__global__ __launch_bounds__(kBlock) void s2d_reach_policy_rollout_kernel(S2DHot p_sgpr, const S2DRare* __restrict__ rp,
                                                                          float* __restrict__ S, int64_t stride, int64_t n,
                                                                          int n_steps, QNetDims d, int act_fn,
                                                                          const float* __restrict__ params,
                                                                          const float* __restrict__ log_std_dev,
                                                                          const uint32_t* __restrict__ det_dev, RolloutOut ro,
                                                                          float* __restrict__ term_rec, float* __restrict__ logp_rec,
                                                                          StepOut o, int wave_words) {
  constexpr int A = MODE == S2D_MODE_TURN4 ? 4 : 1;   // outputs of the continuous heads
  extern __shared__ __attribute__((aligned(16))) float smem[];
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
  const bool det = *det_dev != 0u;
  float log_std[A], sigma[A];
#pragma unroll
  for (int j = 0; j < A; ++j) { log_std[j] = 0.0f; sigma[j] = 1.0f; }
  if constexpr (MODE != S2D_MODE_DISCRETE) {
#pragma unroll
    for (int j = 0; j < A; ++j) { log_std[j] = log_std_dev[j]; sigma[j] = exp_spec(log_std[j]); }
  }
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
  U4 uquad{0, 0, 0, 0}, squad{0, 0, 0, 0}, gquad{0, 0, 0, 0};
  bool have_prep = false;
  uint32_t* const coop_scratch = reinterpret_cast<uint32_t*>(tile);
  if (p.auto_reset) {
    prep_fill_coop<NK>(p, rp, *prep, lane, active ? reset_key(e) : 0u, gl, gh, active, coop_scratch);
    have_prep = active;
  }
  int n_missing = 0;
  int64_t row = 0;
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
    policy_forward(d, act_fn, smem, ha, hb, qv, tile, lane);
    if (active) {
      const uint32_t k = k0 + (uint32_t)t;
      const bool refresh = t == 0 || (k & 3u) == 0u;
      float lp;
      CmdPrep c;
      if constexpr (MODE == S2D_MODE_DISCRETE) {
        if (refresh && !det) uquad = s2d_draw(p, gl, gh, k >> 2, S2D_ST_POLICY, 4);   // block 4: the categorical draw
        const int a = categorical_head(qv + lane * d.qpitch, d.na, det, quad_word(uquad, k), lp);
        if (ro.action) static_cast<int32_t*>(ro.action)[row + i] = a;
        c = decode_action<S2D_MODE_DISCRETE>(p, Action4{(float)a, 0.0f, 0.0f, 0.0f}, gl, gh, k, false, squad, cmd, dir);
      } else {
        float y[4], z[4] = {0.0f, 0.0f, 0.0f, 0.0f}, a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = qv[lane * d.qpitch + j];   // A <= 4 of the 16 rows of the one output tile
        if (!det) {
          if (MODE == S2D_MODE_CONT1 && refresh) gquad = s2d_draw(p, gl, gh, k >> 2, S2D_ST_POLICY, 3);   // block 3: z
          policy_gauss<MODE>(p, gl, gh, k, gquad, z);
        }
        gaussian_head<A>(y, log_std, sigma, det, z, a, lp);
        if (ro.action) store_rollout_action<MODE>(ro.action, row + i, Action4{a[0], a[1], a[2], a[3]});
        c = decode_action<MODE>(p, Action4{clip1(a[0]), clip1(a[1]), clip1(a[2]), clip1(a[3])}, gl, gh, k, refresh, squad, cmd, dir);
      }
      if (logp_rec) logp_rec[row + i] = lp;
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
    wave_lds_fence();                                      // the head has read its logits before the next forward overwrites them
    if (p.auto_reset) n_missing += __popcll(__ballot(active && done != 0));
    if (ro.obs) store_obs_tile(tile, ob, lane, active, ro.obs + (row + wave_first) * S2D_OBS_DIM, valid);
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
}

using PolicyKernel = void (*)(S2DHot, const S2DRare*, float*, int64_t, int64_t, int, QNetDims, int, const float*, const float*,
                              const uint32_t*, RolloutOut, float*, float*, StepOut, int);
struct PolicySlots {};   // the table of allow_lds_slot (s2d_actor_rollout.h) of this unit: 3 x 3 instantiations

// act_fn = 0 relu | 1 tanh; 0, or -2 on a HIP failure
int s2d_internal_rollout_policy(const ActorRollout& a, const ActorPlanBuf& buf, int act_fn, const float* params, const float* log_std,
                                const uint32_t* det, float* logp) {
  const ActorPlan<QNetDims>& pl = plan_of<QNetDims>(buf);
#define S2D_POLICY_ROW(M)                                                                                                \
  {s2d_reach_policy_rollout_kernel<M, S2D_NK_OFF>, s2d_reach_policy_rollout_kernel<M, S2D_NK_LATTICE>,                   \
   s2d_reach_policy_rollout_kernel<M, S2D_NK_SQUARE>}
  static const PolicyKernel table[3][3] = {S2D_POLICY_ROW(S2D_MODE_DISCRETE), S2D_POLICY_ROW(S2D_MODE_CONT1),
                                           S2D_POLICY_ROW(S2D_MODE_TURN4)};
#undef S2D_POLICY_ROW
  const PolicyKernel k = table[a.mode][a.nk];
  if (!allow_lds_slot<PolicySlots>(reinterpret_cast<const void*>(k), 3 * a.mode + a.nk)) return -2;
  const int threads = pl.waves * kWave;
  const unsigned blocks = (unsigned)((a.n + threads - 1) / threads);
  hipLaunchKernelGGL(k, dim3(blocks), dim3(threads), pl.lds, static_cast<hipStream_t>(a.stream), *a.hot, a.rare_dev, a.S, a.stride, a.n,
                     a.n_steps, pl.d, act_fn, params, log_std, det, *a.ro, a.term_rec, logp, *a.o, pl.wave_words);
  static const char* const mode_names[3] = {"discrete", "cont1", "turn4"};
  std::snprintf(a.name, a.name_bytes, "s2d_reach_policy_rollout_kernel<mode=%s,noise=%d,act=%s,h1=%d,h2=%d,a=%d,waves=%d>",
                mode_names[a.mode], a.nk, act_fn ? "tanh" : "relu", pl.d.h1, pl.d.h2, pl.d.na, pl.waves);
  return 0;
}

// ------------------------------------------------------------------------------------------ the head alone
__global__ void s2d_debug_policy_head_kernel(int mode, int A, const float* __restrict__ y, const float* __restrict__ log_std_dev,
                                             const uint64_t* __restrict__ gid, const uint32_t* __restrict__ kk, uint32_t seed_lo,
                                             uint32_t seed_hi, int det_i, int64_t n, void* __restrict__ action,
                                             float* __restrict__ logp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  S2DHot p{}; p.seed_lo = seed_lo; p.seed_hi = seed_hi;
  const uint32_t gl = (uint32_t)gid[i], gh = (uint32_t)(gid[i] >> 32), k = kk[i];
  const bool det = det_i != 0;
  float lp;
  if (mode == S2D_MODE_DISCRETE) {
    const U4 uquad = s2d_draw(p, gl, gh, k >> 2, S2D_ST_POLICY, 4);
    static_cast<int32_t*>(action)[i] = categorical_head(y + i * A, A, det, quad_word(uquad, k), lp);
  } else if (mode == S2D_MODE_CONT1) {
    const float ls[1] = {log_std_dev[0]}, sg[1] = {exp_spec(log_std_dev[0])};
    float z[1] = {0.0f}, a[1];
    if (!det) policy_gauss<S2D_MODE_CONT1>(p, gl, gh, k, s2d_draw(p, gl, gh, k >> 2, S2D_ST_POLICY, 3), z);
    gaussian_head<1>(y + i, ls, sg, det, z, a, lp);
    static_cast<float*>(action)[i] = a[0];
  } else {
    float ls[4], sg[4], z[4] = {0.0f, 0.0f, 0.0f, 0.0f}, a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { ls[j] = log_std_dev[j]; sg[j] = exp_spec(ls[j]); }
    if (!det) policy_gauss<S2D_MODE_TURN4>(p, gl, gh, k, U4{0, 0, 0, 0}, z);
    gaussian_head<4>(y + 4 * i, ls, sg, det, z, a, lp);
#pragma unroll
    for (int j = 0; j < 4; ++j) static_cast<float*>(action)[4 * i + j] = a[j];
  }
  logp[i] = lp;
}

S2D_API int s2d_debug_policy_head(int mode, int n_out, const void* y_dev, const void* log_std_dev, const void* gid_dev,
                                  const void* k_dev, uint64_t seed, int deterministic, int64_t n, void* action_dev, void* logp_dev,
                                  void* stream) {
  const auto misaligned = [](const void* q, unsigned m) { return (reinterpret_cast<uintptr_t>(q) & m) != 0; };
  const char* err = nullptr;
  if (mode != S2D_MODE_DISCRETE && mode != S2D_MODE_CONT1 && mode != S2D_MODE_TURN4)
    err = "s2d_debug_policy_head: mode must be 0 (discrete), 1 (continuous) or 2 (turning)";
  else if (mode == S2D_MODE_DISCRETE ? (n_out < 1 || n_out > 64) : n_out != (mode == S2D_MODE_TURN4 ? 4 : 1))
    err = "s2d_debug_policy_head: n_out must be in [1, 64] (discrete), 1 (continuous) or 4 (turning)";
  else if (n < 1 || n > INT32_MAX) err = "s2d_debug_policy_head: n must be in [1, 2^31 - 1]";
  else if (!y_dev || !k_dev || !action_dev || !logp_dev || misaligned(y_dev, 3u) || misaligned(k_dev, 3u) ||
           misaligned(action_dev, 3u) || misaligned(logp_dev, 3u))
    err = "s2d_debug_policy_head: y, k, action and logp must be non-NULL, 4-byte aligned device pointers";
  else if (!gid_dev || misaligned(gid_dev, 7u)) err = "s2d_debug_policy_head: gid must be a non-NULL, 8-byte aligned device pointer";
  else if (mode != S2D_MODE_DISCRETE && (!log_std_dev || misaligned(log_std_dev, 3u)))
    err = "s2d_debug_policy_head: a continuous head needs a non-NULL, 4-byte aligned log_std buffer [n_out]";
  if (err) { s2d_internal_set_error(err); return S2D_EINVAL; }
  hipLaunchKernelGGL(s2d_debug_policy_head_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     mode, n_out, static_cast<const float*>(y_dev), static_cast<const float*>(log_std_dev),
                     static_cast<const uint64_t*>(gid_dev), static_cast<const uint32_t*>(k_dev), (uint32_t)seed,
                     (uint32_t)(seed >> 32), deterministic, n, action_dev, static_cast<float*>(logp_dev));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    s2d_internal_set_error((std::string("s2d_debug_policy_head: launch: ") + hipGetErrorString(e)).c_str());
    return S2D_EHIP;
  }
  return S2D_OK;
}

// ------------------------------------------------------------------------------------------ GAE
// One lane per env, t = T-1 .. 0.  The recurrence is two dependent fmaf per step; the loads do not depend on it, so they are
// issued one chunk of kGaeChunk steps ahead: while chunk c is scanned and stored, the loads of chunk c + 1 are in flight.  At
// 65 536 envs there is one wave per SIMD and nothing else to hide a memory latency per step.  One wave per workgroup, so that
// small batches still spread over the CUs.
static constexpr int kGaeChunk = 8;
struct GaeChunk { float r[kGaeChunk], v[kGaeChunk], tv[kGaeChunk]; uint8_t d[kGaeChunk], res[kGaeChunk]; };

template <bool TV>
S2D_DEV void gae_load(GaeChunk& c, int t_hi, int64_t N, int64_t i, const float* __restrict__ reward, const uint8_t* __restrict__ done,
                      const float* __restrict__ value, const uint8_t* __restrict__ result, const float* __restrict__ tval) {
#pragma unroll
  for (int u = 0; u < kGaeChunk; ++u) {
    const int t = t_hi - u;
    c.r[u] = 0.0f; c.v[u] = 0.0f; c.tv[u] = 0.0f; c.d[u] = 0; c.res[u] = 0;
    if (t >= 0) {
      const int64_t idx = (int64_t)t * N + i;
      c.r[u] = reward[idx]; c.v[u] = value[idx]; c.d[u] = done[idx];
      if constexpr (TV) { c.res[u] = result[idx]; c.tv[u] = tval[idx]; }
    }
  }
}

template <bool TV>
__global__ __launch_bounds__(kWave) void s2d_gae_kernel(const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                        const float* __restrict__ value, const float* __restrict__ last_value,
                                                        const uint8_t* __restrict__ result, const float* __restrict__ tval,
                                                        float gamma, float lam, int T, int64_t N, float* __restrict__ adv,
                                                        float* __restrict__ ret) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const float gl = gamma * lam;
  float next_v = last_value[i], gae = 0.0f;
  GaeChunk cur, nxt;
  gae_load<TV>(cur, T - 1, N, i, reward, done, value, result, tval);
  for (int t_hi = T - 1; t_hi >= 0; t_hi -= kGaeChunk) {
    gae_load<TV>(nxt, t_hi - kGaeChunk, N, i, reward, done, value, result, tval);   // nothing to load past t = 0
#pragma unroll
    for (int u = 0; u < kGaeChunk; ++u) {
      const int t = t_hi - u;
      if (t >= 0) {
        float r = cur.r[u];
        if constexpr (TV) r = cur.res[u] == S2D_RESULT_TIMEOUT ? fmaf(gamma, cur.tv[u], r) : r;
        const float nt = cur.d[u] ? 0.0f : 1.0f;
        const float v = cur.v[u];
        const float delta = fmaf(gamma * nt, next_v, r) - v;
        gae = fmaf(gl * nt, gae, delta);
        const int64_t idx = (int64_t)t * N + i;
        adv[idx] = gae;
        ret[idx] = gae + v;
        next_v = v;
      }
    }
    cur = nxt;
  }
}

S2D_API int s2d_gae(int n_steps, int64_t n_envs, const float* reward, const uint8_t* done, const float* value,
                    const float* last_value, const uint8_t* result, const float* terminal_value, float gamma, float lam,
                    float* advantage, float* ret, void* stream) {
  const auto misaligned = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3u) != 0; };
  const char* err = nullptr;
  if (n_steps < 1) err = "s2d_gae: n_steps must be >= 1";
  else if (n_envs < 1 || n_envs > INT32_MAX) err = "s2d_gae: n_envs must be in [1, 2^31 - 1]";
  else if (!std::isfinite(gamma) || !std::isfinite(lam)) err = "s2d_gae: gamma and lam must be finite";
  else if ((result == nullptr) != (terminal_value == nullptr)) err = "s2d_gae: result and terminal_value go together (both or neither)";
  else if (!reward || !done || !value || !last_value || !advantage || !ret)
    err = "s2d_gae: reward, done, value, last_value, advantage and ret must be non-NULL device pointers";
  else if (misaligned(reward) || misaligned(value) || misaligned(last_value) || misaligned(terminal_value) || misaligned(advantage) ||
           misaligned(ret))
    err = "s2d_gae: the float arrays must be 4-byte aligned";
  if (err) { s2d_internal_set_error(err); return S2D_EINVAL; }
  const unsigned blocks = (unsigned)((n_envs + kWave - 1) / kWave);
  if (result)
    hipLaunchKernelGGL(s2d_gae_kernel<true>, dim3(blocks), dim3(kWave), 0, static_cast<hipStream_t>(stream), reward, done, value,
                       last_value, result, terminal_value, gamma, lam, n_steps, n_envs, advantage, ret);
  else
    hipLaunchKernelGGL(s2d_gae_kernel<false>, dim3(blocks), dim3(kWave), 0, static_cast<hipStream_t>(stream), reward, done, value,
                       last_value, result, terminal_value, gamma, lam, n_steps, n_envs, advantage, ret);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    s2d_internal_set_error((std::string("s2d_gae: launch: ") + hipGetErrorString(e)).c_str());
    return S2D_EHIP;
  }
  return S2D_OK;
}
