// s2d_episodes.hip -- episode statistics of a [T][N] rollout record on the device: s2d_episode_stats carries every env's running
// return and length from record to record, writes the finished episodes to a caller-owned ring in the order a per-step loop
// over the envs would have met them, and keeps exact integer totals; include/s2d.h (the spec), DESIGN.md section 4.
// Engine-independent like s2d_gae and s2d_replay_push: raw device arrays, no engine handle.
//
// The order needs every episode's rank among the record's set `done` bytes in row-major order.  A wave owns 64 consecutive
// envs (a tile); the record is a table of T x W (row, tile) cells, W = ceil(N / 64).  Five launches, one behind the other:
//   1. count   reads `done` only: cell (t, w) <- popcount of the wave's ballot.  No carry, so rows are split over waves too.
//   2. chunk   an exclusive scan inside each chunk of 1024 cells, in place (32 bits: a chunk holds at most 65536 episodes),
//              and the chunk's total.
//   3. top     one workgroup scans the chunk totals (64 bits: n may pass 2^32), stores n and zeroes the integer accumulators.
//   4. scatter each lane walks its env's column with the carry in registers; rank = chunk base + cell base + popcount of the
//              ballot below the lane.  Nothing is shared between the waves of a workgroup: no LDS, no barrier.  Each wave
//              adds its result histogram and length sum to the accumulators with five integer atomics.
//   5. totals  one thread, queued behind the others as s2d_replay_push_cursor_kernel is, advances `totals`: no wave of the
//              same call can see the new cursor.
// No workgroup waits on another, there is no float atomic, and the only floating-point operation is the one add of the spec.
// Element offsets are 64-bit (T * N < 2^40); a written episode's distance from the first kept rank is below capacity < 2^31.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "s2d_kernels.h"

extern "C" void s2d_internal_set_error(const char* msg);

namespace {
constexpr int kEpBlock = 256;                        // 4 waves; the waves of a block share nothing
constexpr int kEpWaves = kEpBlock / kWave;
constexpr int kEpChunk = 1024;                       // cells per scan chunk: 256 threads x 4
constexpr int kEpCountRows = 16;                     // rows per wave in the count pass (at least; more when T is huge)
constexpr int kEpBatch = 8;                          // rows whose loads the count pass issues together
constexpr int kEpScatterBatch = 8;                   // ... and the scatter pass, which keeps two such batches in flight
constexpr int kEpAcc = 5;                            // accumulators: results 0..3, sum of lengths

// the workspace, carved from its 16-byte aligned start
struct EpLayout {
  uint64_t W, cells, chunks;
  size_t off_parts, off_acc, bytes;
};
bool ep_shape_ok(int T, int64_t N) {
  return T >= 1 && N >= 1 && N <= INT32_MAX && (uint64_t)T * (uint64_t)N < (1ull << 40);
}
EpLayout ep_layout(int T, int64_t N) {
  EpLayout l;
  l.W = ((uint64_t)N + kWave - 1) / kWave;
  l.cells = (uint64_t)T * l.W;
  l.chunks = (l.cells + kEpChunk - 1) / kEpChunk;
  l.off_parts = (size_t)((l.cells * 4 + 15) & ~15ull);
  l.off_acc = l.off_parts + (size_t)(l.chunks + 1) * 8;      // parts[chunks] holds n
  l.bytes = l.off_acc + kEpAcc * 8 + 16;                     // + the slack of the alignment
  return l;
}

struct EpDev {
  uint32_t* cell;              // [T][W]: counts, then exclusive bases inside their chunk
  uint64_t* parts;             // [chunks]: chunk totals, then exclusive bases; [chunks] = n
  unsigned long long* acc;     // [5]
  uint64_t cells, chunks;
  uint32_t T, N, W;
};

// Loads of the record are never predicated: a lane past N reads its tile's last env and a row past the end reads the last row
// (always inside the arrays), and the value is masked afterwards, so a batch's loads are all in flight together.
S2D_DEV uint8_t stream_u8(const uint8_t* p) { return __builtin_nontemporal_load(p); }
S2D_DEV float stream_f32(const float* p) { return __builtin_nontemporal_load(p); }

template <typename V>
S2D_DEV V wave_inclusive(V v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const V u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  return v;
}
}  // namespace

// ---- 1. count: cell (t, w) <- the number of set done[t][64 w .. 64 w + 63]
__global__ __launch_bounds__(kEpBlock) void s2d_episode_count_kernel(const uint8_t* __restrict__ done, EpDev d, uint32_t rows_per_wave) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * kEpWaves + (threadIdx.x >> 6));
  if (w >= d.W) return;                                            // wave-uniform
  const uint32_t i = w * kWave + lane, ic = min(i, d.N - 1);
  const bool live = i < d.N;
  const uint32_t t0 = blockIdx.y * rows_per_wave, t1 = min(d.T, t0 + rows_per_wave);
  for (uint32_t tb = t0; tb < t1; tb += kEpBatch) {
    uint8_t dn[kEpBatch];
#pragma unroll
    for (int u = 0; u < kEpBatch; ++u) dn[u] = stream_u8(done + ((uint64_t)min(tb + u, t1 - 1) * d.N + ic));
#pragma unroll
    for (int u = 0; u < kEpBatch; ++u) {
      const uint32_t c = (uint32_t)__popcll(__ballot(live && dn[u] != 0));
      if (lane == 0 && tb + u < t1) d.cell[(uint64_t)(tb + u) * d.W + w] = c;
    }
  }
}

// ---- 2. chunk: exclusive scan of the chunk's 1024 cells in place, the chunk's total to parts
__global__ __launch_bounds__(kEpBlock) void s2d_episode_chunk_kernel(EpDev d) {
  __shared__ uint32_t wave_sum[kEpWaves];
  const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
  const uint64_t c0 = (uint64_t)blockIdx.x * kEpChunk + tid * 4;
  uint32_t v[4];
  if (c0 + 4 <= d.cells) {
    const uint4 q = *reinterpret_cast<const uint4*>(d.cell + c0);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = c0 + j < d.cells ? d.cell[c0 + j] : 0u;
  }
  const uint32_t s = v[0] + v[1] + v[2] + v[3];
  const uint32_t incl = wave_inclusive(s, (int)lane);
  if (lane == kWave - 1) wave_sum[wv] = incl;
  __syncthreads();
  uint32_t before = 0, total = 0;
#pragma unroll
  for (int k = 0; k < kEpWaves; ++k) {
    const uint32_t ws = wave_sum[k];
    if ((uint32_t)k < wv) before += ws;
    total += ws;
  }
  const uint32_t e0 = before + incl - s, e1 = e0 + v[0], e2 = e1 + v[1], e3 = e2 + v[2];
  if (c0 + 4 <= d.cells) {
    *reinterpret_cast<uint4*>(d.cell + c0) = make_uint4(e0, e1, e2, e3);
  } else {
    const uint32_t e[4] = {e0, e1, e2, e3};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c0 + j < d.cells) d.cell[c0 + j] = e[j];
  }
  if (tid == 0) d.parts[blockIdx.x] = total;
}

// ---- 3. top: exclusive scan of the chunk totals by one workgroup, n behind them, the accumulators zeroed
__global__ __launch_bounds__(kEpBlock) void s2d_episode_top_kernel(EpDev d) {
  __shared__ unsigned long long wave_sum[kEpWaves];
  const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
  unsigned long long carry = 0;
  for (uint64_t b0 = 0; b0 < d.chunks; b0 += kEpBlock) {             // block-uniform trip count
    const uint64_t b = b0 + tid;
    const unsigned long long s = b < d.chunks ? (unsigned long long)d.parts[b] : 0ull;
    const unsigned long long incl = wave_inclusive(s, (int)lane);
    if (lane == kWave - 1) wave_sum[wv] = incl;
    __syncthreads();
    unsigned long long before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kEpWaves; ++k) {
      const unsigned long long ws = wave_sum[k];
      if ((uint32_t)k < wv) before += ws;
      total += ws;
    }
    if (b < d.chunks) d.parts[b] = carry + before + incl - s;
    carry += total;
    __syncthreads();                                                // wave_sum is rewritten by the next round
  }
  if (tid == 0) d.parts[d.chunks] = carry;
  if (tid < kEpAcc) d.acc[tid] = 0ull;
}

// ---- 4. scatter
struct EpScatterArgs {
  const float* reward; const uint8_t* done; const uint8_t* result;
  float* acc_return; int32_t* acc_length;
  float* ring_ret; int32_t* ring_len; uint8_t* ring_res; int32_t* ring_env; int64_t* ring_step;
  const uint64_t* totals;
  uint32_t cap;
};

template <bool REWARD, bool RESULT>
__global__ __launch_bounds__(kEpBlock) void s2d_episode_scatter_kernel(EpScatterArgs a, EpDev d) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * kEpWaves + (threadIdx.x >> 6));
  if (w >= d.W) return;                                            // wave-uniform
  const uint32_t i = w * kWave + lane, ic = min(i, d.N - 1);
  const bool live = i < d.N;
  const uint64_t below = lane ? (~0ull >> (kWave - lane)) : 0ull;  // the lanes before this one

  const uint64_t e0 = a.totals[0], s0 = a.totals[1], n = d.parts[d.chunks];
  const uint64_t first_kept = n > a.cap ? n - a.cap : 0;           // ranks below it are not written
  const uint32_t slot_first = (uint32_t)((e0 % a.cap + first_kept % a.cap) % a.cap);

  float R = a.acc_return[ic];
  int32_t L = a.acc_length[ic];
  uint32_t hist[4] = {0, 0, 0, 0};
  unsigned long long len_sum = 0;

  // Two batches in flight: the loads of the next 8 rows are issued before the current 8 are worked through (at N = 65 536
  // a wave is alone on its SIMD, so nothing else overlaps its loads).
  struct Batch {
    uint8_t dn[kEpScatterBatch], rs[kEpScatterBatch];
    float rw[kEpScatterBatch];
    uint64_t part[kEpScatterBatch];                                // the chunk's base and the cell's base inside it: added
    uint32_t cell[kEpScatterBatch];                                // where they are used, so that no load waits on another
  };
  const uint64_t* __restrict__ parts = d.parts;
  const uint32_t* __restrict__ cell = d.cell;
  const auto load = [&](uint32_t tb) {
    Batch b;
#pragma unroll
    for (int u = 0; u < kEpScatterBatch; ++u) {
      // the row's base and the cell are wave-uniform: scalar arithmetic and scalar loads
      const uint32_t t = __builtin_amdgcn_readfirstlane(min(tb + u, d.T - 1));
      const uint64_t row = (uint64_t)t * d.N;
      b.dn[u] = stream_u8(a.done + row + ic);
      b.rw[u] = REWARD ? stream_f32(a.reward + row + ic) : 0.0f;
      b.rs[u] = RESULT ? stream_u8(a.result + row + ic) : (uint8_t)0;
      const uint64_t c = (uint64_t)t * d.W + w;                    // wave-uniform
      b.part[u] = parts[c / kEpChunk];
      b.cell[u] = cell[c];
    }
    return b;
  };
  Batch cur = load(0);
  for (uint32_t tb = 0; tb < d.T; tb += kEpScatterBatch) {
    Batch nxt = cur;
    if (tb + kEpScatterBatch < d.T) nxt = load(tb + kEpScatterBatch);     // wave-uniform
#pragma unroll
    for (int u = 0; u < kEpScatterBatch; ++u) {
      const bool on = tb + u < d.T;                                 // wave-uniform; a row past the end changes nothing
      const bool fin = on && live && cur.dn[u] != 0;
      R = on ? R + cur.rw[u] : R;
      L = on ? L + 1 : L;
      if (fin) {                                                     // the active lanes are exactly the row's set done bytes
        const uint64_t k = cur.part[u] + cur.cell[u] + (uint32_t)__popcll(__ballot(true) & below);
        const uint32_t r = cur.rs[u];
        hist[r <= 3 ? r : 0] += 1;
        len_sum += (unsigned long long)(uint32_t)L;
        if (k >= first_kept) {
          uint32_t slot = slot_first + (uint32_t)(k - first_kept);  // both below cap < 2^31
          if (slot >= a.cap) slot -= a.cap;
          a.ring_ret[slot] = R;
          a.ring_len[slot] = L;
          a.ring_res[slot] = (uint8_t)r;
          a.ring_env[slot] = (int32_t)i;
          a.ring_step[slot] = (int64_t)(s0 + tb + u);
        }
        R = 0.0f;
        L = 0;
      }
    }
    cur = nxt;
  }
  if (live) {
    a.acc_return[i] = R;
    a.acc_length[i] = L;
  }
  // the wave's integer sums, then one atomic each (exact in any order)
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) {
#pragma unroll
    for (int j = 0; j < 4; ++j) hist[j] += __shfl_xor(hist[j], m);
    len_sum += __shfl_xor(len_sum, m);
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (hist[j]) atomicAdd(d.acc + j, (unsigned long long)hist[j]);
    if (len_sum) atomicAdd(d.acc + 4, len_sum);
  }
}

// ---- 5. totals: queued behind the scatter pass, so no wave of this call sees the new cursor
__global__ void s2d_episode_totals_kernel(uint64_t* totals, EpDev d, uint64_t cap) {
  const uint64_t n = d.parts[d.chunks];
  totals[0] += n;
  totals[1] += d.T;
  for (int j = 0; j < 4; ++j) totals[2 + j] += d.acc[j];
  totals[6] += d.acc[4];
  totals[7] += n > cap ? n - cap : 0;
}

// ------------------------------------------------------------------------------------------ host
namespace {
bool misaligned(const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; }
int fail(const char* fn, const char* msg) {
  s2d_internal_set_error((std::string(fn) + ": " + msg).c_str());
  return S2D_EINVAL;
}
int launched(const char* fn) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return S2D_OK;
  s2d_internal_set_error((std::string(fn) + ": launch: " + hipGetErrorString(e)).c_str());
  return S2D_EHIP;
}
}  // namespace

S2D_API size_t s2d_episode_stats_workspace(int n_steps, int64_t n_envs) {
  return ep_shape_ok(n_steps, n_envs) ? ep_layout(n_steps, n_envs).bytes : 0;
}

S2D_API int s2d_episode_stats(int n_steps, int64_t n_envs, const float* reward, const uint8_t* done, const uint8_t* result,
                              float* acc_return, int32_t* acc_length, const S2DEpisodeRing* ring, uint64_t* totals, void* workspace,
                              size_t workspace_bytes, void* stream) {
  static const char* fn = "s2d_episode_stats";
  if (n_steps < 1) return fail(fn, "n_steps must be >= 1");
  if (n_envs < 1 || n_envs > INT32_MAX) return fail(fn, "n_envs must be in [1, 2^31 - 1]");
  if (!ep_shape_ok(n_steps, n_envs)) return fail(fn, "n_steps * n_envs must be below 2^40");
  if (!ring) return fail(fn, "ring must be non-NULL");
  if (ring->capacity < 1 || ring->capacity > INT32_MAX) return fail(fn, "ring capacity must be in [1, 2^31 - 1]");
  if (!done || !acc_return || !acc_length || !totals || !workspace || !ring->ret || !ring->length || !ring->result || !ring->env ||
      !ring->step)
    return fail(fn, "done, acc_return, acc_length, the ring arrays, totals and workspace must be non-NULL device pointers");
  if (misaligned(totals, 8) || misaligned(ring->step, 8)) return fail(fn, "totals and the ring's step must be 8-byte aligned");
  if (misaligned(reward, 4) || misaligned(acc_return, 4) || misaligned(acc_length, 4) || misaligned(ring->ret, 4) ||
      misaligned(ring->length, 4) || misaligned(ring->env, 4))
    return fail(fn, "the 4-byte arrays must be 4-byte aligned");
  const EpLayout l = ep_layout(n_steps, n_envs);
  if (workspace_bytes < l.bytes) return fail(fn, "workspace_bytes is below s2d_episode_stats_workspace(n_steps, n_envs)");

  char* ws = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15);
  EpDev d{reinterpret_cast<uint32_t*>(ws), reinterpret_cast<uint64_t*>(ws + l.off_parts),
          reinterpret_cast<unsigned long long*>(ws + l.off_acc), l.cells, l.chunks, (uint32_t)n_steps, (uint32_t)n_envs, (uint32_t)l.W};
  EpScatterArgs a{reward, done, result, acc_return, acc_length, ring->ret, ring->length, ring->result, ring->env, ring->step, totals,
                  (uint32_t)ring->capacity};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned tile_blocks = (unsigned)((l.W + kEpWaves - 1) / kEpWaves);
  const uint32_t T = (uint32_t)n_steps;
  const uint32_t rows = T <= 65535u * kEpCountRows ? (uint32_t)kEpCountRows : (T + 65534u) / 65535u;   // grid.y <= 65535
  hipLaunchKernelGGL(s2d_episode_count_kernel, dim3(tile_blocks, (T + rows - 1) / rows), dim3(kEpBlock), 0, st, done, d, rows);
  hipLaunchKernelGGL(s2d_episode_chunk_kernel, dim3((unsigned)l.chunks), dim3(kEpBlock), 0, st, d);
  hipLaunchKernelGGL(s2d_episode_top_kernel, dim3(1), dim3(kEpBlock), 0, st, d);
  if (reward && result) hipLaunchKernelGGL((s2d_episode_scatter_kernel<true, true>), dim3(tile_blocks), dim3(kEpBlock), 0, st, a, d);
  else if (reward) hipLaunchKernelGGL((s2d_episode_scatter_kernel<true, false>), dim3(tile_blocks), dim3(kEpBlock), 0, st, a, d);
  else if (result) hipLaunchKernelGGL((s2d_episode_scatter_kernel<false, true>), dim3(tile_blocks), dim3(kEpBlock), 0, st, a, d);
  else hipLaunchKernelGGL((s2d_episode_scatter_kernel<false, false>), dim3(tile_blocks), dim3(kEpBlock), 0, st, a, d);
  hipLaunchKernelGGL(s2d_episode_totals_kernel, dim3(1), dim3(1), 0, st, totals, d, (uint64_t)ring->capacity);
  return launched(fn);
}
