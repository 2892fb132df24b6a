// s2d_wide_actor.hip -- the fused actors on the streamed-weight MLP: the epsilon-greedy Q-network (s2d_rollout_qnet_wide) and the
// deterministic tanh policy with Gaussian action noise (s2d_rollout_actor_wide) with one to five hidden layers, widths that are
// multiples of 4 up to 400 and relu, tanh_spec or sigmoid_spec between them; include/s2d.h S2DWideNet, DESIGN.md sections 4, 5, 7.
//
// The rollout kernel is s2d_reach_actor_rollout_kernel (s2d_actor_rollout.h) over a second network back end (WideDims,
// s2d_wide_net.h): the heads, the draws, the simulation, the records and the statistics are the template's.  The weights do not
// live in LDS: the pack kernel (s2d_wide_pack.hip) writes them in fragment order into the caller's workspace, on the same stream
// ahead of the rollout, and the rollout's waves stream them from there (L2) into registers layer by layer.  The shape's checks,
// the workspace's, the plan and the diagnostic's host half are shared with the other users of the network (s2d_wide_host.h,
// s2d_wide_net.h, s2d_actor_rollout.h).  The activation and the env tiles
// per pass are fields of the kernel argument (wave-uniform), so the instantiations are those of the resident actors: 3 for the
// Q-actor, 12 for the tanh actor, and the diagnostic kernel.  On a shape the resident path takes the result is its, bit for bit.
//
// The third actor on the same network is Soft Actor-Critic's squashed Gaussian (s2d_rollout_sac): a kernel of its own below,
// s2d_reach_sac_rollout_kernel, with the template's body and the head of s2d_sac_head.h; the template keeps its instantiations.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>

#include "s2d_actor_rollout.h"
#include "s2d_sac_head.h"
#include "s2d_wide_net.h"

// ------------------------------------------------------------------------------------------ the SAC rollout
// s2d_rollout_sac: the body of s2d_reach_actor_rollout_kernel (s2d_actor_rollout.h) on the streamed-weight network with 2A outputs
// (rows 0 .. A-1 the means, A .. 2A-1 the raw log-std) and the squashed-Gaussian head of s2d_sac_head.h in place of the tanh
// head: no epsilon, one device word that switches to the greedy action, logp recorded.  z is POLICY block 3, laid out as the
// tanh actor's Gaussian noise (turning: z0..z3 of the block at counter k; continuous: z_{k & 3} of the block at counter k >> 2,
// cached in gquad).  The activation and the env tiles per pass are fields of `d`: 2 modes x 3 noise models = 6 instantiations.
template <int MODE, int NK>
__global__ __launch_bounds__(kBlock) void s2d_reach_sac_rollout_kernel(S2DHot p_sgpr, const S2DRare* __restrict__ rp,
                                                                       float* __restrict__ S, int64_t stride, int64_t n, int n_steps,
                                                                       WideDims d, const uint32_t* __restrict__ det_dev, RolloutOut ro,
                                                                       float* __restrict__ term_rec, float* __restrict__ logp_rec,
                                                                       StepOut o, int wave_words) {
  constexpr int A = MODE == S2D_MODE_TURN4 ? 4 : 1;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const S2DHot p = hot_in_vgprs(p_sgpr);
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t wave_first = i - lane;

  // ---- the biases into LDS (block-wide, once per launch); the fragments stay in the workspace
  net_pack(d, nullptr, smem);
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
  U4 squad{0, 0, 0, 0}, gquad{0, 0, 0, 0};
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
    net_forward<false>(d, smem, ha, hb, qv, tile, lane);
    float y[2 * A];
#pragma unroll
    for (int j = 0; j < 2 * A; ++j) y[j] = qv[lane * d.qpitch + j];   // 2A <= 8 of the 16 rows of the one output tile
    wave_lds_fence();
    if (active) {
      const uint32_t k = k0 + (uint32_t)t;
      const bool refresh = t == 0 || (k & 3u) == 0u;
      float z[4] = {0.0f, 0.0f, 0.0f, 0.0f}, a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (!det) {
        if constexpr (MODE == S2D_MODE_TURN4) {
          const U4 w = s2d_draw(p, gl, gh, k, S2D_ST_POLICY, 3);
          box_muller(w.x, w.y, z[0], z[1]);
          box_muller(w.z, w.w, z[2], z[3]);
        } else {
          if (refresh) gquad = s2d_draw(p, gl, gh, k >> 2, S2D_ST_POLICY, 3);
          const bool hi = (k & 2u) != 0u;
          float zc, zs;
          box_muller(hi ? gquad.z : gquad.x, hi ? gquad.w : gquad.y, zc, zs);
          z[0] = (k & 1u) ? zs : zc;
        }
      }
      float lp = 0.0f;
#pragma unroll
      for (int j = 0; j < A; ++j) {
        const float term = sac_head_term(y[j], y[A + j], z[j], det, a[j]);
        lp = j == 0 ? term : lp + term;
      }
      const Action4 act{a[0], a[1], a[2], a[3]};
      if (ro.action) store_rollout_action<MODE>(ro.action, row + i, act);
      if (logp_rec) logp_rec[row + i] = lp;
      const CmdPrep c = decode_action<MODE>(p, act, gl, gh, k, refresh, squad, cmd, dir);
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

// host side (same library, hidden symbols; the rollouts' C entry points are in s2d_engine.hip, the tables and the launch in
// s2d_actor_rollout.h, s2d_wide_workspace_bytes and s2d_debug_wide_forward at the end of this file)
static const char kBytesFn[] = "s2d_wide_workspace_bytes";

// the plan of `net`'s shape: wide_net_plan with the observation's width and the rollout template's tail
static int wide_plan(const char* who, const S2DWideNet* net, ActorPlan<WideDims>& pl) {
  return wide_net_plan(who, net, S2D_OBS_DIM, kWideTail, pl.d, pl.wave_words, pl.waves, pl.lds);
}
int s2d_internal_wide_plan(const char* who, const S2DWideNet* net, ActorPlanBuf* buf) { return wide_plan(who, net, plan_in<WideDims>(buf)); }

// the workspace check, then the pack kernel and the rollout
int s2d_internal_rollout_wide(const ActorRollout& a, const char* who, const S2DWideNet* net, const ActorPlanBuf& buf) {
  ActorPlan<WideDims> pl = plan_of<WideDims>(buf);
  const WidePackArgs pack = wide_pack_args(pl.d, S2D_OBS_DIM);
  if (wide_net_workspace(who, net, pack, kBytesFn) != S2D_OK) return S2D_EINVAL;
  pl.d.wf = static_cast<const float*>(net->workspace);
  const float* const noise = net->noise_kind ? net->noise : nullptr;
  if (!launch_actor_rollout(a, pl, net->params, net->epsilon, noise,
                            [&] { s2d_internal_wide_pack(pack, net->params, net->workspace, static_cast<hipStream_t>(a.stream)); }))
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

// s2d_rollout_sac's launch: the workspace check, then the pack kernel and the SAC rollout
namespace {
struct SacSlots {};   // the owner of the SAC kernels' dynamic-LDS slots (allow_lds_slot): 2 modes x 3 noise models
}
int s2d_internal_rollout_sac(const ActorRollout& a, const char* who, const S2DWideNet* net, const ActorPlanBuf& buf, const uint32_t* det,
                             float* logp) {
  using Kernel = void (*)(S2DHot, const S2DRare*, float*, int64_t, int64_t, int, WideDims, const uint32_t*, RolloutOut, float*, float*,
                          StepOut, int);
#define S2D_SAC_ROW(M) \
  {s2d_reach_sac_rollout_kernel<M, S2D_NK_OFF>, s2d_reach_sac_rollout_kernel<M, S2D_NK_LATTICE>, s2d_reach_sac_rollout_kernel<M, S2D_NK_SQUARE>}
  static const Kernel table[2][3] = {S2D_SAC_ROW(S2D_MODE_CONT1), S2D_SAC_ROW(S2D_MODE_TURN4)};
#undef S2D_SAC_ROW
  ActorPlan<WideDims> pl = plan_of<WideDims>(buf);
  const WidePackArgs pack = wide_pack_args(pl.d, S2D_OBS_DIM);
  if (wide_net_workspace(who, net, pack, kBytesFn) != S2D_OK) return S2D_EINVAL;
  pl.d.wf = static_cast<const float*>(net->workspace);
  const int m = a.mode == S2D_MODE_TURN4 ? 1 : 0;
  const Kernel k = table[m][a.nk];
  if (!allow_lds_slot<SacSlots>(reinterpret_cast<const void*>(k), 3 * m + a.nk)) return -2;
  const hipStream_t stream = static_cast<hipStream_t>(a.stream);
  const int threads = pl.waves * kWave;
  const unsigned blocks = (unsigned)((a.n + threads - 1) / threads);
  s2d_internal_wide_pack(pack, net->params, net->workspace, stream);
  hipLaunchKernelGGL(k, dim3(blocks), dim3(threads), pl.lds, stream, *a.hot, a.rare_dev, a.S, a.stride, a.n, a.n_steps, pl.d, det, *a.ro,
                     a.term_rec, logp, *a.o, pl.wave_words);
  std::snprintf(a.name, a.name_bytes, "s2d_wide_sac_rollout_kernel<mode=%s,noise=%d,act=%s,h=%s,a=%d,waves=%d,tiles=%d>",
                m ? "turn4" : "cont1", a.nk, kActName[net->activation], widths_text(net).c_str(), net->n_out, pl.waves, pl.d.tiles);
  return 0;
}

S2D_API size_t s2d_wide_workspace_bytes(const S2DWideNet* shape) { return wide_net_workspace_bytes(shape, S2D_OBS_DIM); }

S2D_API int s2d_debug_wide_forward(const S2DWideNet* shape, const void* obs_dev, int64_t n, void* y_dev, void* greedy_dev, char* name,
                                   void* stream) {
  return debug_forward_streamed("s2d_debug_wide_forward", "s2d_debug_wide_forward_kernel", S2D_OBS_DIM, kBytesFn, wide_plan,
                                s2d_wide_debug_forward_kernel<S2D_OBS_DIM>, shape, obs_dev, n, y_dev, greedy_dev, name, stream);
}
