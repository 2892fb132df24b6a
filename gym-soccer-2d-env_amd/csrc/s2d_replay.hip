// s2d_replay.hip -- the device replay buffer of the off-policy learners (DQN, DDPG): s2d_replay_push turns a whole [T][N]
// rollout record into n-step transitions in a caller-owned ring, s2d_replay_sample draws a batch from it; include/s2d.h (the
// spec), DESIGN.md section 4.  Engine-independent like s2d_gae: raw device arrays, no engine handle.
//
// Both kernels are row movers around a short scan.  A wave owns 64 consecutive slots (push) or batch elements (sample):
//   1. each lane works out its own transition -- the n-step scan over done / reward (coalesced across lanes, strided by N in
//      time), or the Philox index -- and keeps a ROW DESCRIPTOR per row array: which source array and which row of it;
//   2. the wave then copies the 64 x D words of each row array together: flat unit f = 64 * iteration + lane belongs to row
//      f / D, column f % D, whose descriptor comes from that row's lane by __shfl.  Consecutive lanes therefore store
//      consecutive words (one 256-byte wave store per iteration, whatever D is), instead of 64 rows strided by D.
// With D % 4 == 0 the unit is 16 bytes (rows are then 16-byte aligned on both sides).  Rows are addressed by slot, so a wave
// that straddles the ring's wrap needs nothing special.  Row indices fit 31 bits (T * N <= capacity < 2^31); element offsets
// are 64-bit (capacity * D words exceeds 2^32 in practice).  No atomics, no LDS.  The cursor is read by every wave when it
// runs and advanced by a one-thread kernel queued behind the copy on the same stream, so no wave can see the new position.
#include "s2d_replay_common.h"

struct ReplayPushArgs {
  const uint32_t* first_obs; const uint32_t* obs; const uint32_t* terminal_obs; const uint32_t* action;
  const float* reward; const uint8_t* done; const uint8_t* result;
  const uint64_t* cursor;
  uint32_t T, N, D, AW, n_step, total;
  float gamma;
};

template <bool VEC>
__global__ __launch_bounds__(kReplayBlock) void s2d_replay_push_kernel(ReplayPushArgs a, ReplayRingDev ring) {
  using U = std::conditional_t<VEC, uint4, uint32_t>;
  const int lane = threadIdx.x & (kWave - 1);
  const uint64_t first = ((uint64_t)blockIdx.x * kReplayWaves + (threadIdx.x >> 6)) * kWave;
  if (first >= a.total) return;                                    // wave-uniform
  const uint32_t k0 = (uint32_t)first, rows = min((uint32_t)kWave, a.total - k0);
  const uint32_t C = ring.cap, pos = (uint32_t)(a.cursor[0] % C);
  uint32_t slot0 = pos + k0;                                       // pos < C, k0 < T * N <= C < 2^31
  if (slot0 >= C) slot0 -= C;
  const auto slot_of = [&](uint32_t r) { const uint32_t s = slot0 + r; return s >= C ? s - C : s; };   // r < rows <= C

  const uint32_t k = k0 + lane;
  uint32_t d_obs = 0, d_next = 0;
  if ((uint32_t)lane < rows) {
    const uint32_t t = k / a.N, i = k - t * a.N;
    uint32_t s = t, ks = k;
    float R = a.reward[k], g = a.gamma;
    bool dn = a.done[k] != 0;
    while (!dn && s + 1 < a.T && s + 1 - t < a.n_step) {
      s += 1; ks += a.N;
      R = fmaf(g, a.reward[ks], R);
      g = g * a.gamma;
      dn = a.done[ks] != 0;
    }
    float discount = g;
    if (dn) discount = (a.result && a.result[ks] == S2D_RESULT_TIMEOUT) ? g : 0.0f;
    d_obs = t == 0 ? (i | kRowAlt) : k - a.N;                      // first_obs[i] | obs[t - 1][i]
    d_next = dn ? (ks | kRowAlt) : ks;                             // terminal_obs[s][i] | obs[s][i]
    const uint32_t slot = slot_of(lane);
    ring.reward[slot] = R;
    ring.discount[slot] = discount;
  }

  const uint32_t w = VEC ? a.D / 4 : a.D;
  const U* obs = reinterpret_cast<const U*>(a.obs);
  const U* alt_obs = reinterpret_cast<const U*>(a.first_obs);
  const U* alt_next = reinterpret_cast<const U*>(a.terminal_obs);
  U* r_obs = reinterpret_cast<U*>(ring.obs);
  U* r_next = reinterpret_cast<U*>(ring.next);
  wave_copy_rows<U>(lane, rows, w, d_obs,
                    [&](uint32_t d, uint32_t c) { return ((d & kRowAlt) ? alt_obs : obs)[(uint64_t)(d & kRowMask) * w + c]; },
                    [&](uint32_t r, uint32_t c) { return r_obs + (uint64_t)slot_of(r) * w + c; });
  wave_copy_rows<U>(lane, rows, w, d_next,
                    [&](uint32_t d, uint32_t c) { return ((d & kRowAlt) ? alt_next : obs)[(uint64_t)(d & kRowMask) * w + c]; },
                    [&](uint32_t r, uint32_t c) { return r_next + (uint64_t)slot_of(r) * w + c; });
  wave_copy_rows<uint32_t>(lane, rows, a.AW, k,
                           [&](uint32_t d, uint32_t c) { return a.action[(uint64_t)d * a.AW + c]; },
                           [&](uint32_t r, uint32_t c) { return ring.action + (uint64_t)slot_of(r) * a.AW + c; });
}

__global__ void s2d_replay_push_cursor_kernel(uint64_t* cursor, uint64_t n, uint64_t cap) {
  const uint64_t pos = cursor[0] % cap, size = cursor[1] + n;
  cursor[0] = (pos + n) % cap;
  cursor[1] = size < cap ? size : cap;
  cursor[2] += 1;
}

struct ReplaySampleArgs {
  const uint64_t* cursor;
  uint32_t* obs; uint32_t* next; uint32_t* action;
  float* reward; float* discount; int32_t* index;
  uint32_t B, D, AW, seed_lo, seed_hi;
};

template <bool VEC>
__global__ __launch_bounds__(kReplayBlock) void s2d_replay_sample_kernel(ReplaySampleArgs a, ReplayRingDev ring) {
  using U = std::conditional_t<VEC, uint4, uint32_t>;
  const int lane = threadIdx.x & (kWave - 1);
  const uint64_t first = ((uint64_t)blockIdx.x * kReplayWaves + (threadIdx.x >> 6)) * kWave;
  if (first >= a.B) return;                                        // wave-uniform
  const uint32_t b0 = (uint32_t)first, rows = min((uint32_t)kWave, a.B - b0);
  const uint64_t have = a.cursor[1], samples = a.cursor[3];
  const uint32_t size = (uint32_t)(have < ring.cap ? have : ring.cap);

  const uint32_t b = b0 + lane;
  uint32_t desc = kRowAlt;                                         // the alternate source of a sample is the zero row
  if ((uint32_t)lane < rows) {
    float R = 0.0f, discount = 0.0f;
    int32_t index = -1;
    if (size) {
      const U4 q = philox4x32_10(b >> 2, (uint32_t)samples, (uint32_t)(samples >> 32), (uint32_t)S2D_REPLAY_STREAM << 16, a.seed_lo,
                                 a.seed_hi);
      desc = (uint32_t)rnd_below(quad_word(q, b), size);
      index = (int32_t)desc;
      R = ring.reward[desc];
      discount = ring.discount[desc];
    }
    a.reward[b] = R;
    a.discount[b] = discount;
    a.index[b] = index;
  }

  const uint32_t w = VEC ? a.D / 4 : a.D;
  const U* r_obs = reinterpret_cast<const U*>(ring.obs);
  const U* r_next = reinterpret_cast<const U*>(ring.next);
  U* o_obs = reinterpret_cast<U*>(a.obs);
  U* o_next = reinterpret_cast<U*>(a.next);
  wave_copy_rows<U>(lane, rows, w, desc,
                    [&](uint32_t d, uint32_t c) { return (d & kRowAlt) ? U{} : r_obs[(uint64_t)d * w + c]; },
                    [&](uint32_t r, uint32_t c) { return o_obs + (uint64_t)(b0 + r) * w + c; });
  wave_copy_rows<U>(lane, rows, w, desc,
                    [&](uint32_t d, uint32_t c) { return (d & kRowAlt) ? U{} : r_next[(uint64_t)d * w + c]; },
                    [&](uint32_t r, uint32_t c) { return o_next + (uint64_t)(b0 + r) * w + c; });
  wave_copy_rows<uint32_t>(lane, rows, a.AW, desc,
                           [&](uint32_t d, uint32_t c) { return (d & kRowAlt) ? 0u : ring.action[(uint64_t)d * a.AW + c]; },
                           [&](uint32_t r, uint32_t c) { return a.action + (uint64_t)(b0 + r) * a.AW + c; });
}

__global__ void s2d_replay_sample_cursor_kernel(uint64_t* cursor) { cursor[3] += 1; }

// ------------------------------------------------------------------------------------------ host (checks: s2d_replay_common.h)
S2D_API int s2d_replay_push(int n_steps, int64_t n_envs, int obs_dim, int action_words, int n_step, float gamma, const void* first_obs,
                            const void* obs, const void* terminal_obs, const void* action, const float* reward, const uint8_t* done,
                            const uint8_t* result, const S2DReplayRing* ring, uint64_t* cursor, void* stream) {
  static const char* fn = "s2d_replay_push";
  if (n_steps < 1) return fail(fn, "n_steps must be >= 1");
  if (n_envs < 1) return fail(fn, "n_envs must be >= 1");
  if (n_step < 1) return fail(fn, "n_step must be >= 1");
  if (!std::isfinite(gamma)) return fail(fn, "gamma must be finite");
  if (const char* e = ring_error(obs_dim, action_words, ring, cursor)) return fail(fn, e);
  const int64_t C = ring->capacity;
  if (n_envs > C || (int64_t)n_steps * n_envs > C) return fail(fn, "n_steps * n_envs must not exceed the ring's capacity");
  if (!first_obs || !obs || !terminal_obs || !action || !reward || !done)
    return fail(fn, "first_obs, obs, terminal_obs, action, reward and done must be non-NULL device pointers");
  const uintptr_t row = obs_dim % 4 == 0 ? 16 : 4;
  if (misaligned(first_obs, row) || misaligned(obs, row) || misaligned(terminal_obs, row))
    return fail(fn, "first_obs, obs and terminal_obs must be 4-byte aligned (16-byte when obs_dim % 4 == 0)");
  if (misaligned(action, 4) || misaligned(reward, 4)) return fail(fn, "action and reward must be 4-byte aligned");
  const uint64_t TN = (uint64_t)n_steps * (uint64_t)n_envs, D = (uint64_t)obs_dim, AW = (uint64_t)action_words, Cu = (uint64_t)C;
  const Span outs[] = {{ring->obs, Cu * D * 4}, {ring->next_obs, Cu * D * 4}, {ring->action, Cu * AW * 4}, {ring->reward, Cu * 4},
                       {ring->discount, Cu * 4}, {cursor, 32}};
  const Span ins[] = {{first_obs, (uint64_t)n_envs * D * 4}, {obs, TN * D * 4}, {terminal_obs, TN * D * 4}, {action, TN * AW * 4},
                      {reward, TN * 4}, {done, TN}, {result, TN}};
  if (any_overlap(outs, 6, ins, 7)) return fail(fn, "the ring arrays and the cursor must not overlap the record or each other");

  ReplayPushArgs a{static_cast<const uint32_t*>(first_obs), static_cast<const uint32_t*>(obs), static_cast<const uint32_t*>(terminal_obs),
                   static_cast<const uint32_t*>(action), reward, done, result, cursor, (uint32_t)n_steps, (uint32_t)n_envs,
                   (uint32_t)obs_dim, (uint32_t)action_words, (uint32_t)n_step, (uint32_t)TN, gamma};
  const dim3 grid((unsigned)((TN + kReplayBlock - 1) / kReplayBlock)), block(kReplayBlock);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (obs_dim % 4 == 0) hipLaunchKernelGGL(s2d_replay_push_kernel<true>, grid, block, 0, st, a, ring_dev(ring));
  else hipLaunchKernelGGL(s2d_replay_push_kernel<false>, grid, block, 0, st, a, ring_dev(ring));
  hipLaunchKernelGGL(s2d_replay_push_cursor_kernel, dim3(1), dim3(1), 0, st, cursor, TN, Cu);
  return launched(fn);
}

S2D_API int s2d_replay_sample(int64_t batch, int obs_dim, int action_words, const S2DReplayRing* ring, uint64_t* cursor, uint64_t seed,
                              void* b_obs, void* b_next, void* b_action, float* b_reward, float* b_discount, int32_t* b_index,
                              void* stream) {
  static const char* fn = "s2d_replay_sample";
  if (batch < 1 || batch > INT32_MAX) return fail(fn, "batch must be in [1, 2^31 - 1]");
  if (const char* e = ring_error(obs_dim, action_words, ring, cursor)) return fail(fn, e);
  if (!b_obs || !b_next || !b_action || !b_reward || !b_discount || !b_index)
    return fail(fn, "the batch arrays must be non-NULL device pointers");
  const uintptr_t row = obs_dim % 4 == 0 ? 16 : 4;
  if (misaligned(b_obs, row) || misaligned(b_next, row))
    return fail(fn, "the batch's obs and next_obs must be 4-byte aligned (16-byte when obs_dim % 4 == 0)");
  if (misaligned(b_action, 4) || misaligned(b_reward, 4) || misaligned(b_discount, 4) || misaligned(b_index, 4))
    return fail(fn, "the batch's action, reward, discount and index must be 4-byte aligned");
  const uint64_t B = (uint64_t)batch, D = (uint64_t)obs_dim, AW = (uint64_t)action_words, Cu = (uint64_t)ring->capacity;
  const Span outs[] = {{b_obs, B * D * 4}, {b_next, B * D * 4}, {b_action, B * AW * 4}, {b_reward, B * 4}, {b_discount, B * 4},
                       {b_index, B * 4}};
  const Span ins[] = {{ring->obs, Cu * D * 4}, {ring->next_obs, Cu * D * 4}, {ring->action, Cu * AW * 4}, {ring->reward, Cu * 4},
                      {ring->discount, Cu * 4}, {cursor, 32}};
  if (any_overlap(outs, 6, ins, 6)) return fail(fn, "the batch arrays must not overlap the ring, the cursor or each other");

  ReplaySampleArgs a{cursor, static_cast<uint32_t*>(b_obs), static_cast<uint32_t*>(b_next), static_cast<uint32_t*>(b_action), b_reward,
                     b_discount, b_index, (uint32_t)batch, (uint32_t)obs_dim, (uint32_t)action_words, (uint32_t)seed,
                     (uint32_t)(seed >> 32)};
  const dim3 grid((unsigned)((B + kReplayBlock - 1) / kReplayBlock)), block(kReplayBlock);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (obs_dim % 4 == 0) hipLaunchKernelGGL(s2d_replay_sample_kernel<true>, grid, block, 0, st, a, ring_dev(ring));
  else hipLaunchKernelGGL(s2d_replay_sample_kernel<false>, grid, block, 0, st, a, ring_dev(ring));
  hipLaunchKernelGGL(s2d_replay_sample_cursor_kernel, dim3(1), dim3(1), 0, st, cursor);
  return launched(fn);
}
