// s2d_replay_common.h -- what the replay translation units share (s2d_replay.hip, s2d_replay_prio.hip): the ring as the kernels
// see it, the wave row mover and the host-side argument checks.  Everything here has internal linkage: no device code crosses a unit.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "s2d_kernels.h"

extern "C" void s2d_internal_set_error(const char* msg);

static constexpr int kReplayBlock = 256;
static constexpr int kReplayWaves = kReplayBlock / kWave;
static constexpr uint32_t kRowAlt = 0x80000000u;   // descriptor: bit 31 = the alternate source, bits 0..30 = the row
static constexpr uint32_t kRowMask = 0x7fffffffu;

struct ReplayRingDev {
  uint32_t* obs; uint32_t* next; uint32_t* action;
  float* reward; float* discount;
  uint32_t cap;
};

// The wave copies `rows` (<= 64) rows of `w` units U.  The loop count is wave-uniform and every lane takes part in the shuffle
// (a lane past the end still owns a descriptor others read); only the load and the store are predicated.  Row and column are
// carried from one iteration to the next, so there is one division per call.
template <typename U, typename Src, typename Dst>
S2D_DEV void wave_copy_rows(int lane, uint32_t rows, uint32_t w, uint32_t desc, Src src, Dst dst) {
  const uint32_t total = rows * w, q = kWave / w, m = kWave % w;
  uint32_t r = (uint32_t)lane / w, c = (uint32_t)lane % w;
  for (uint32_t f0 = 0; f0 < total; f0 += kWave) {
    const uint32_t d = __shfl(desc, (int)(r & (kWave - 1)));
    if (f0 + lane < total) *dst(r, c) = src(d, c);
    r += q; c += m;
    if (c >= w) { c -= w; r += 1; }
  }
}

// ------------------------------------------------------------------------------------------ host
namespace {
struct Span { const void* p; uint64_t bytes; };
bool overlaps(const Span& x, const Span& y) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(x.p), b = reinterpret_cast<uintptr_t>(y.p);
  return x.p && y.p && a < b + y.bytes && b < a + x.bytes;
}
// any of outs[] against any of ins[] or another of outs[]
bool any_overlap(const Span* outs, int n_out, const Span* ins, int n_in) {
  for (int i = 0; i < n_out; ++i) {
    for (int j = 0; j < n_in; ++j)
      if (overlaps(outs[i], ins[j])) return true;
    for (int j = i + 1; j < n_out; ++j)
      if (overlaps(outs[i], outs[j])) return true;
  }
  return false;
}
bool misaligned(const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; }

// the shape and ring checks both entry points share; nullptr if acceptable
const char* ring_error(int D, int AW, const S2DReplayRing* ring, const uint64_t* cursor) {
  if (D < 1 || D > 1024) return "obs_dim must be in [1, 1024]";
  if (AW < 1 || AW > 8) return "action_words must be in [1, 8]";
  if (!ring) return "ring must be non-NULL";
  if (ring->capacity < 1 || ring->capacity > INT32_MAX) return "ring capacity must be in [1, 2^31 - 1]";
  if (!ring->obs || !ring->next_obs || !ring->action || !ring->reward || !ring->discount || !cursor)
    return "the ring arrays and the cursor must be non-NULL device pointers";
  const uintptr_t row = D % 4 == 0 ? 16 : 4;
  if (misaligned(ring->obs, row) || misaligned(ring->next_obs, row))
    return "the ring's obs and next_obs must be 4-byte aligned (16-byte when obs_dim % 4 == 0)";
  if (misaligned(ring->action, 4) || misaligned(ring->reward, 4) || misaligned(ring->discount, 4))
    return "the ring's action, reward and discount must be 4-byte aligned";
  if (misaligned(cursor, 8)) return "the cursor must be 8-byte aligned";
  return nullptr;
}
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
ReplayRingDev ring_dev(const S2DReplayRing* r) {
  return ReplayRingDev{static_cast<uint32_t*>(r->obs), static_cast<uint32_t*>(r->next_obs), static_cast<uint32_t*>(r->action), r->reward,
                       r->discount, (uint32_t)r->capacity};
}
}  // namespace
