// s2d_replay_prio.hip -- proportional prioritized replay on a device sum tree over the ring of s2d_replay.hip:
// s2d_replay_prio_push marks the slots a push is about to write, s2d_replay_sample_prio draws a stratified batch by descending
// the tree, s2d_replay_prio_update stores new priorities; include/s2d.h (the spec), DESIGN.md section 4.
//
// The tree is float[2P]: leaves at P + slot, node i = tree[2i] + tree[2i+1] (one fp32 add, left + right), tree[1] the total,
// tree[0] the running maximum.  Every node is ONE add of its two children, so its value does not depend on who computes it or
// how the work is cut; that is the whole determinism argument, and the kernels keep to it:
//   * no float atomics and no sum by arrival order.  The only atomic is an integer max on the bit pattern of clamped (normal,
//     positive) floats, which order like unsigned ints; a max is order-independent.
//   * no grid-wide sync: every phase is a launch of its own on the caller's stream.
// Repair goes up the tree in TIERS of up to 6 levels, one launch per tier (ceil(log2 P / 6) <= 5 launches; the top tier is the
// partial one).  A lane owns the subtree of height H under one ancestor: it loads the 2^H consecutive nodes of the tier's
// bottom level (finished by the previous launch), forms the 2^H - 1 sums in registers and stores them.  Lanes that share an
// ancestor (duplicate indices, neighbouring leaves) store identical words.  Node indices fit 31 bits (2P <= 2^31).
#include "s2d_replay_common.h"

static constexpr int kTier = 6;   // levels per repair launch: 64 nodes in registers per lane

S2D_DEV float prio_clamp(float p) { return p >= S2D_PRIO_MIN ? (p <= S2D_PRIO_MAX ? p : S2D_PRIO_MAX) : S2D_PRIO_MIN; }
S2D_DEV float prio_max_seen(const float* tree) { const float t = tree[0]; return t >= S2D_PRIO_MIN ? t : 1.0f; }

// The subtree of height H whose root is node `a` of level `bottom - H`: tree[a << H .. +2^H) are its bottom nodes.
template <int H>
S2D_DEV void repair_subtree(float* tree, uint32_t a) {
  float v[1 << H];
  const float* src = tree + ((uint64_t)a << H);
#pragma unroll
  for (int j = 0; j < (1 << H) / 2; ++j) {
    const float2 q = reinterpret_cast<const float2*>(src)[j];          // a << H is even and the tree 8-byte aligned
    v[2 * j] = q.x; v[2 * j + 1] = q.y;
  }
#pragma unroll
  for (int k = 1; k <= H; ++k) {
    float* dst = tree + ((uint64_t)a << (H - k));
#pragma unroll
    for (int j = 0; j < (1 << (H - k)); ++j) {
      v[j] = v[2 * j] + v[2 * j + 1];
      dst[j] = v[j];
    }
  }
}

// ------------------------------------------------------------------------------------------ prio_push
struct PrioPushArgs {
  float* tree; const uint64_t* cursor;
  uint32_t n, cap, P;
};

__global__ __launch_bounds__(kReplayBlock) void s2d_prio_mark_kernel(PrioPushArgs a) {
  const uint64_t j = (uint64_t)blockIdx.x * kReplayBlock + threadIdx.x;
  if (j >= a.n) return;
  uint32_t slot = (uint32_t)(a.cursor[0] % a.cap) + (uint32_t)j;       // pos < cap, j < n <= cap <= 2^30
  if (slot >= a.cap) slot -= a.cap;
  a.tree[(uint64_t)a.P + slot] = prio_max_seen(a.tree);
}

// The marked slots are the run [pos, pos + n) wrapped at the capacity: at most two runs of leaves, hence two runs of subtrees
// `shift` levels up.  One lane per subtree; the host sizes the grid for the worst case ((n >> shift) + 4 lanes) because pos is
// known only here.  A subtree both runs touch is repaired twice, to the same words.
template <int H>
__global__ __launch_bounds__(kReplayBlock) void s2d_prio_push_tier_kernel(PrioPushArgs a, uint32_t shift) {
  const uint32_t t = blockIdx.x * kReplayBlock + threadIdx.x;
  const uint32_t pos = (uint32_t)(a.cursor[0] % a.cap);
  const uint32_t end1 = min(pos + a.n, a.cap), n2 = pos + a.n - end1;  // [pos, end1) and [0, n2)
  const uint32_t g0 = pos >> shift, c1 = ((end1 - 1) >> shift) - g0 + 1, c2 = n2 ? ((n2 - 1) >> shift) + 1 : 0;
  uint32_t g;
  if (t < c1) g = g0 + t;
  else if (t - c1 < c2) g = t - c1;
  else return;
  repair_subtree<H>(a.tree, (a.P >> shift) + g);
}

// ------------------------------------------------------------------------------------------ prio_update
struct PrioUpdateArgs {
  float* tree; const uint64_t* cursor; const int32_t* index; const float* priority;
  uint32_t B, cap, P;
};

S2D_DEV bool update_slot(const PrioUpdateArgs& a, uint32_t b, uint32_t& slot) {
  if (b >= a.B) return false;
  const uint64_t have = a.cursor[1];
  const uint32_t size = (uint32_t)(have < a.cap ? have : a.cap);
  const int32_t i = a.index[b];
  slot = (uint32_t)i;
  return i >= 0 && slot < size;
}

// phase 1: the named leaves to +0 (so that the max of phase 2 forgets the old priority), tree[0] to its as-read value
__global__ __launch_bounds__(kReplayBlock) void s2d_prio_clear_kernel(PrioUpdateArgs a) {
  const uint32_t b = blockIdx.x * kReplayBlock + threadIdx.x;
  uint32_t slot;
  if (update_slot(a, b, slot)) a.tree[(uint64_t)a.P + slot] = 0.0f;
  if (b == 0) a.tree[0] = prio_max_seen(a.tree);                      // the only thread that touches tree[0] in this launch
}

// phase 2: integer max of the clamped bits into the leaf; one max per wave into the hot word tree[0]
__global__ __launch_bounds__(kReplayBlock) void s2d_prio_max_kernel(PrioUpdateArgs a) {
  const uint32_t b = blockIdx.x * kReplayBlock + threadIdx.x;
  uint32_t slot, bits = 0;
  uint32_t* words = reinterpret_cast<uint32_t*>(a.tree);
  if (update_slot(a, b, slot)) {
    bits = __float_as_uint(prio_clamp(a.priority[b]));
    atomicMax(words + (uint64_t)a.P + slot, bits);
  }
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) bits = max(bits, (uint32_t)__shfl_xor((int)bits, d));
  if ((threadIdx.x & (kWave - 1)) == 0 && bits) atomicMax(words, bits);
}

template <int H>
__global__ __launch_bounds__(kReplayBlock) void s2d_prio_update_tier_kernel(PrioUpdateArgs a, uint32_t shift) {
  const uint32_t b = blockIdx.x * kReplayBlock + threadIdx.x;
  uint32_t slot;
  if (update_slot(a, b, slot)) repair_subtree<H>(a.tree, (a.P + slot) >> shift);
}

// ------------------------------------------------------------------------------------------ sample_prio
struct PrioSampleArgs {
  const float* tree; const uint64_t* cursor;
  uint32_t* obs; uint32_t* next; uint32_t* action;
  float* reward; float* discount; int32_t* index; float* priority; float* total;
  uint32_t B, D, AW, P, seed_lo, seed_hi;
};

template <bool VEC>
__global__ __launch_bounds__(kReplayBlock) void s2d_replay_sample_prio_kernel(PrioSampleArgs a, ReplayRingDev ring) {
  using U = std::conditional_t<VEC, uint4, uint32_t>;
  const int lane = threadIdx.x & (kWave - 1);
  const uint64_t first = ((uint64_t)blockIdx.x * kReplayWaves + (threadIdx.x >> 6)) * kWave;
  if (first >= a.B) return;                                        // wave-uniform
  const uint32_t b0 = (uint32_t)first, rows = min((uint32_t)kWave, a.B - b0);
  const uint64_t have = a.cursor[1], samples = a.cursor[3];
  const uint32_t size = (uint32_t)(have < ring.cap ? have : ring.cap);
  const float total = a.tree[1];
  const bool empty = size == 0 || !(total > 0.0f);

  const uint32_t b = b0 + lane;
  uint32_t desc = kRowAlt;                                         // the alternate source of a sample is the zero row
  if ((uint32_t)lane < rows) {
    float R = 0.0f, discount = 0.0f, priority = 0.0f;
    int32_t index = -1;
    if (!empty) {
      const U4 q = philox4x32_10(b >> 2, (uint32_t)samples, (uint32_t)(samples >> 32), (uint32_t)S2D_REPLAY_PRIO_STREAM << 16,
                                 a.seed_lo, a.seed_hi);
      const float seg = total / (float)a.B;
      const float u = (float)(quad_word(q, b) >> 8) * 0x1p-24f;
      float m = fmaf(u, seg, (float)b * seg);
      uint32_t i = 1;
      while (i < a.P) {                                            // the two children are adjacent: one 8-byte load per level
        const float2 lr = *reinterpret_cast<const float2*>(a.tree + 2 * (uint64_t)i);
        if (m >= lr.x && lr.y > 0.0f) { m = m - lr.x; i = 2 * i + 1; }
        else i = 2 * i;
      }
      desc = i - a.P;
      if (desc >= size) desc = size - 1;                           // never with a tree these calls maintained; a corrupted one
      index = (int32_t)desc;                                       // must not send the row copy outside the ring
      priority = a.tree[(uint64_t)a.P + desc];
      R = ring.reward[desc];
      discount = ring.discount[desc];
    }
    a.reward[b] = R;
    a.discount[b] = discount;
    a.index[b] = index;
    a.priority[b] = priority;
    if (b == 0) a.total[0] = empty ? 0.0f : total;
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

__global__ void s2d_replay_sample_prio_cursor_kernel(uint64_t* cursor) { cursor[3] += 1; }

// ------------------------------------------------------------------------------------------ host
namespace {
constexpr int64_t kPrioCapMax = (int64_t)1 << 30, kPrioBatchMax = (int64_t)1 << 24;

int log2_leaves(int64_t capacity) {          // L with P = 2^L the smallest power of two >= capacity
  int L = 0;
  while (((int64_t)1 << L) < capacity) ++L;
  return L;
}

// the checks the three entry points share; nullptr if acceptable
const char* tree_error(int64_t capacity, const float* tree, const uint64_t* cursor) {
  if (capacity < 1 || capacity > kPrioCapMax) return "capacity must be in [1, 2^30]";
  if (!tree || !cursor) return "tree and cursor must be non-NULL device pointers";
  if (misaligned(tree, 8)) return "the tree must be 8-byte aligned";
  if (misaligned(cursor, 8)) return "the cursor must be 8-byte aligned";
  return nullptr;
}

dim3 blocks_for(uint64_t lanes) { return dim3((unsigned)((lanes + kReplayBlock - 1) / kReplayBlock)); }

// One launch per tier, from the leaves up; launch(H, shift) repairs the subtrees whose roots are `shift` levels above the leaves.
template <typename Launch>
void for_each_tier(int L, Launch launch) {
  for (int bottom = L; bottom > 0;) {
    const int H = bottom < kTier ? bottom : kTier;
    bottom -= H;
    launch(H, (uint32_t)(L - bottom));
  }
}

#define S2D_PRIO_TIER_SWITCH(KERNEL, H, ...)                                            \
  switch (H) {                                                                          \
    case 1: hipLaunchKernelGGL(KERNEL<1>, __VA_ARGS__); break;                          \
    case 2: hipLaunchKernelGGL(KERNEL<2>, __VA_ARGS__); break;                          \
    case 3: hipLaunchKernelGGL(KERNEL<3>, __VA_ARGS__); break;                          \
    case 4: hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__); break;                          \
    case 5: hipLaunchKernelGGL(KERNEL<5>, __VA_ARGS__); break;                          \
    default: hipLaunchKernelGGL(KERNEL<6>, __VA_ARGS__); break;                         \
  }
}  // namespace

S2D_API int64_t s2d_replay_tree_words(int64_t capacity) {
  if (capacity < 1 || capacity > kPrioCapMax) return 0;
  return (int64_t)2 << log2_leaves(capacity);
}

S2D_API int s2d_replay_prio_push(int64_t n, int64_t capacity, float* tree, const uint64_t* cursor, void* stream) {
  static const char* fn = "s2d_replay_prio_push";
  if (const char* e = tree_error(capacity, tree, cursor)) return fail(fn, e);
  if (n < 1 || n > capacity) return fail(fn, "n must be in [1, capacity]");
  const int L = log2_leaves(capacity);
  const uint64_t P = (uint64_t)1 << L;
  if (overlaps(Span{tree, 2 * P * 4}, Span{cursor, 32})) return fail(fn, "the tree must not overlap the cursor");

  const PrioPushArgs a{tree, cursor, (uint32_t)n, (uint32_t)capacity, (uint32_t)P};
  const dim3 block(kReplayBlock);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(s2d_prio_mark_kernel, blocks_for((uint64_t)n), block, 0, st, a);
  for_each_tier(L, [&](int H, uint32_t shift) {
    const dim3 grid = blocks_for(((uint64_t)n >> shift) + 4);
    S2D_PRIO_TIER_SWITCH(s2d_prio_push_tier_kernel, H, grid, block, 0, st, a, shift)
  });
  return launched(fn);
}

S2D_API int s2d_replay_prio_update(int64_t batch, int64_t capacity, float* tree, const uint64_t* cursor, const int32_t* index,
                                   const float* priority, void* stream) {
  static const char* fn = "s2d_replay_prio_update";
  if (batch < 1 || batch > kPrioBatchMax) return fail(fn, "batch must be in [1, 2^24]");
  if (const char* e = tree_error(capacity, tree, cursor)) return fail(fn, e);
  if (!index || !priority) return fail(fn, "index and priority must be non-NULL device pointers");
  if (misaligned(index, 4) || misaligned(priority, 4)) return fail(fn, "index and priority must be 4-byte aligned");
  const int L = log2_leaves(capacity);
  const uint64_t P = (uint64_t)1 << L, B = (uint64_t)batch;
  const Span outs[] = {{tree, 2 * P * 4}};
  const Span ins[] = {{cursor, 32}, {index, B * 4}, {priority, B * 4}};
  if (any_overlap(outs, 1, ins, 3)) return fail(fn, "the tree must not overlap the cursor, index or priority");

  const PrioUpdateArgs a{tree, cursor, index, priority, (uint32_t)batch, (uint32_t)capacity, (uint32_t)P};
  const dim3 grid = blocks_for(B), block(kReplayBlock);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(s2d_prio_clear_kernel, grid, block, 0, st, a);
  hipLaunchKernelGGL(s2d_prio_max_kernel, grid, block, 0, st, a);
  for_each_tier(L, [&](int H, uint32_t shift) {
    S2D_PRIO_TIER_SWITCH(s2d_prio_update_tier_kernel, H, grid, block, 0, st, a, shift)
  });
  return launched(fn);
}

S2D_API int s2d_replay_sample_prio(int64_t batch, int obs_dim, int action_words, const S2DReplayRing* ring, const float* tree,
                                   uint64_t* cursor, uint64_t seed, void* b_obs, void* b_next, void* b_action, float* b_reward,
                                   float* b_discount, int32_t* b_index, float* b_priority, float* b_total, void* stream) {
  static const char* fn = "s2d_replay_sample_prio";
  if (batch < 1 || batch > kPrioBatchMax) return fail(fn, "batch must be in [1, 2^24]");
  if (const char* e = ring_error(obs_dim, action_words, ring, cursor)) return fail(fn, e);
  if (const char* e = tree_error(ring->capacity, tree, cursor)) return fail(fn, e);
  if (!b_obs || !b_next || !b_action || !b_reward || !b_discount || !b_index || !b_priority || !b_total)
    return fail(fn, "the batch arrays must be non-NULL device pointers");
  const uintptr_t row = obs_dim % 4 == 0 ? 16 : 4;
  if (misaligned(b_obs, row) || misaligned(b_next, row))
    return fail(fn, "the batch's obs and next_obs must be 4-byte aligned (16-byte when obs_dim % 4 == 0)");
  if (misaligned(b_action, 4) || misaligned(b_reward, 4) || misaligned(b_discount, 4) || misaligned(b_index, 4) ||
      misaligned(b_priority, 4) || misaligned(b_total, 4))
    return fail(fn, "the batch's action, reward, discount, index, priority and total must be 4-byte aligned");
  const uint64_t B = (uint64_t)batch, D = (uint64_t)obs_dim, AW = (uint64_t)action_words, Cu = (uint64_t)ring->capacity;
  const uint64_t P = (uint64_t)1 << log2_leaves(ring->capacity);
  const Span outs[] = {{b_obs, B * D * 4}, {b_next, B * D * 4}, {b_action, B * AW * 4}, {b_reward, B * 4}, {b_discount, B * 4},
                       {b_index, B * 4}, {b_priority, B * 4}, {b_total, 4}};
  const Span ins[] = {{ring->obs, Cu * D * 4}, {ring->next_obs, Cu * D * 4}, {ring->action, Cu * AW * 4}, {ring->reward, Cu * 4},
                      {ring->discount, Cu * 4}, {cursor, 32}, {tree, 2 * P * 4}};
  if (any_overlap(outs, 8, ins, 7)) return fail(fn, "the batch arrays must not overlap the ring, the tree, the cursor or each other");
  if (any_overlap(ins + 6, 1, ins, 6)) return fail(fn, "the tree must not overlap the ring or the cursor");

  const PrioSampleArgs a{tree, cursor, static_cast<uint32_t*>(b_obs), static_cast<uint32_t*>(b_next), static_cast<uint32_t*>(b_action),
                         b_reward, b_discount, b_index, b_priority, b_total, (uint32_t)batch, (uint32_t)obs_dim,
                         (uint32_t)action_words, (uint32_t)P, (uint32_t)seed, (uint32_t)(seed >> 32)};
  const dim3 grid = blocks_for(B), block(kReplayBlock);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (obs_dim % 4 == 0) hipLaunchKernelGGL(s2d_replay_sample_prio_kernel<true>, grid, block, 0, st, a, ring_dev(ring));
  else hipLaunchKernelGGL(s2d_replay_sample_prio_kernel<false>, grid, block, 0, st, a, ring_dev(ring));
  hipLaunchKernelGGL(s2d_replay_sample_prio_cursor_kernel, dim3(1), dim3(1), 0, st, cursor);
  return launched(fn);
}
