// s2d_hear.hip -- the audio layer of the 11v11 match engine for MI355X (gfx950): say, hear capacities, attention and the hear row
// (include/s2d_match.h, "Hearing").  Restated from the published behaviour of rcssserver (EXT: parity to rcssserver unpinned);
// tests/hear_ref.c is an independent CPU restatement this file matches bit for bit.
//
// A unit of its own, as s2d_see.hip: it reads an engine through the public s2d_match_buffers() and the library-internal accessor
// for the Philox keys; the engine holds no hear state and none of its kernels knows of this file.
//
// Mapping of the step kernel, as the see kernel's: ONE MATCH PER HALF-WAVE, lane = listener (0..21).  The positions and the
// quantised payloads of the match are in LDS, who said is a ballot; the loop over the 22 possible speakers is uniform (broadcast
// LDS reads), Philox runs only for pairs that are candidates of a listener with more than one on that side and none attended.
// The 22 rows of a match (2 816 B) are assembled in LDS and leave as whole 64-byte lines, one float4 per lane and instruction.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "s2d_device.h"
#include "s2d_see_row.h"
#include "../../include/s2d_match.h"

#define S2D_API extern "C" __attribute__((visibility("default")))

extern "C" void s2d_internal_set_error(const char* msg);
extern "C" int s2d_match_internal_keys(S2DMatchHandle h, uint32_t keys[4], int* device);

namespace {

using s2d_see::see_fence;
using s2d_see::see_hballot;
using s2d_see::own_body;

constexpr int kBlock = 256;
constexpr int kHalf = s2d_see::kSeeHalf;
constexpr int kEnvsPerBlock = kBlock / kHalf;
constexpr int NP = S2D_MATCH_PLAYERS;
constexpr int SLOTS = S2D_MATCH_SLOTS;
constexpr int kRowVec = S2D_HEAR_DIM / 4;                // 8 float4 per row
constexpr int kMatchVec = NP * kRowVec;                  // 176 float4 = 44 lines of 64 B per match
constexpr uint32_t kAll = 0x3FFFFFu, kLeft = 0x7FFu;
static_assert(S2D_HEAR_DIM == 2 * S2D_HEAR_RECORD && S2D_HEAR_RECORD == 6 + S2D_SAY_WORDS && S2D_SAY_ROW == 2 + S2D_SAY_WORDS, "row layout");
static_assert(S2D_SAY_ROW % 4 == 0, "a say row is whole float4");
static_assert((kMatchVec * 16) % 64 == 0, "a match's rows are whole 64-byte lines");

// S2DHearParams rounded once
struct HearParams {
  float cut, half, inv_half;
  int hear_max, hear_inc, hear_decay, msg_size;
  uint32_t seed_lo, seed_hi, gid_lo, gid_hi;
};

HearParams hear_params(const S2DHearParams& v, const uint32_t keys[4]) {
  HearParams p;
  p.cut = (float)v.audio_cut_dist;
  const double half = (v.say_levels - 1.0) / 2.0;
  p.half = (float)half; p.inv_half = (float)(1.0 / half);
  p.hear_max = (int)v.hear_max; p.hear_inc = (int)v.hear_inc; p.hear_decay = (int)v.hear_decay; p.msg_size = (int)v.say_msg_size;
  p.seed_lo = keys[0]; p.seed_hi = keys[1]; p.gid_lo = keys[2]; p.gid_hi = keys[3];
  return p;
}

// the planes ([N][24]) and the word ([N]) of S2DMatchBuffers the layer reads
struct HearState {
  const float *x, *y, *body;
  const int32_t *card, *tick;
};

struct HearShared {                                      // one match (half-wave)
  float x[kHalf], y[kHalf];
  float pay[NP * S2D_SAY_WORDS + 4];                     // the speakers' payloads, quantised
  float4 row[kMatchVec];                                 // the 22 rows; float4 q of row r sits at r * 8 + (q ^ (r & 7))
};

S2D_DEV int row_at(int r, int q) { return r * kRowVec + (q ^ (r & (kRowVec - 1))); }
S2D_DEV float say_quant(const HearParams& p, float v, int i) {
  if (i >= p.msg_size || v != v) return 0.0f;
  return rintf(clampf(v, -1.0f, 1.0f) * p.half) * p.inv_half;
}
// the raw slot of own-frame slot a for a listener of the right team, and back
S2D_DEV int swap_side(int s) { return s < 11 ? s + 11 : s - 11; }

// One record of the row: what the listener (lane l, raw slot) hears of one side.  cand = the side's candidates (raw slots), att_raw =
// the attended raw slot or -1, cap = the side's capacity (refilled; decremented here when a message is delivered).
struct Record { float heard, sender, dir, missed; float pay[S2D_SAY_WORDS]; };

S2D_DEV Record hear_side(const HearParams& p, const HearShared& sh, int l, bool right, uint32_t cand, int att_raw, int& cap, bool ours,
                         float ax, float ay, float face, float sg, uint64_t gid, uint32_t tick) {
  Record r{};
  const int count = __builtin_popcount(cand);
  r.missed = (float)count;
  if (count == 0 || cap < p.hear_decay) return r;
  int win;
  if (att_raw >= 0 && ((cand >> att_raw) & 1u)) {
    win = att_raw;
  } else if (count == 1) {
    win = __builtin_ctz(cand);
  } else {
    // the smallest (u, own-frame slot): a 22-iteration loop, Philox for this lane's candidates only.  The own-frame order of a
    // side's raw slots is the raw order (both teams keep their order under the swap), so "first smallest" is the tie rule.
    uint32_t best = 0xFFFFFFFFu;
    win = 0;
    for (int j = 0; j < NP; ++j) {
      if ((cand >> j) & 1u) {
        const U4 w = philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), tick, ((uint32_t)S2D_MATCH_ST_HEAR << 16) | (uint32_t)(l * SLOTS + j),
                                   p.seed_lo, p.seed_hi);
        const uint32_t u = w.x >> 8;
        if (u < best) { best = u; win = j; }
      }
    }
  }
  cap -= p.hear_decay;
  r.heard = 1.0f;
  r.sender = ours ? (float)(win % 11 + 1) : 0.0f;
  r.missed = (float)(count - 1);
  const float dx = sg * sh.x[win] - ax, dy = sg * sh.y[win] - ay;
  const float d = hypot2(dx, dy);
  r.dir = d == 0.0f ? 0.0f : rintf(norm_deg_any(atan2_deg(dy, dx) - face));
#pragma unroll
  for (int i = 0; i < S2D_SAY_WORDS; ++i) r.pay[i] = sh.pay[win * S2D_SAY_WORDS + i];
  return r;
}

S2D_DEV void record_store(HearShared& sh, int l, int base, const Record& r, float cap, float att) {
  sh.row[row_at(l, base + 0)] = make_float4(r.heard, r.sender, r.dir, r.missed);
  sh.row[row_at(l, base + 1)] = make_float4(cap, att, r.pay[0], r.pay[1]);
  sh.row[row_at(l, base + 2)] = make_float4(r.pay[2], r.pay[3], r.pay[4], r.pay[5]);
  sh.row[row_at(l, base + 3)] = make_float4(r.pay[6], r.pay[7], r.pay[8], r.pay[9]);
}

__global__ __launch_bounds__(kBlock) void s2d_match_hear_step_kernel(HearParams p, HearState s, S2DMatchHear hs, const float* __restrict__ neck_dev,
                                                                     const float* __restrict__ say, const uint8_t* __restrict__ done, int64_t n) {
  __shared__ HearShared sh_all[kEnvsPerBlock];
  HearShared& sh = sh_all[threadIdx.x / kHalf];
  const int l = threadIdx.x & (kHalf - 1);
  const int half = (threadIdx.x >> 5) & 1;
  const int64_t e = (int64_t)blockIdx.x * kEnvsPerBlock + threadIdx.x / kHalf;
  const bool valid = e < n;
  const int64_t ec = valid ? e : n - 1;
  const bool is_player = l < NP;
  const int64_t k = ec * SLOTS + l;
  float x = 0.0f, y = 0.0f, body = 0.0f, neck = 0.0f, cmd = 0.0f;
  int card = S2D_CARD_RED, cap_our = 0, cap_opp = 0, att = -1;
  bool said = false;
  if (is_player) {
    x = s.x[k]; y = s.y[k]; body = s.body[k]; card = s.card[k];
    if (neck_dev) neck = neck_dev[k];
    cap_our = hs.cap_our[k]; cap_opp = hs.cap_opp[k]; att = hs.attention[k];
    if (say) {
      const float4* row = reinterpret_cast<const float4*>(say + (ec * NP + l) * S2D_SAY_ROW);
      const float4 a = row[0], b = row[1], c = row[2];
      said = a.x != 0.0f && a.x == a.x;
      cmd = a.y;
      float* pay = sh.pay + l * S2D_SAY_WORDS;
      pay[0] = say_quant(p, a.z, 0); pay[1] = say_quant(p, a.w, 1);
      pay[2] = say_quant(p, b.x, 2); pay[3] = say_quant(p, b.y, 3); pay[4] = say_quant(p, b.z, 4); pay[5] = say_quant(p, b.w, 5);
      pay[6] = say_quant(p, c.x, 6); pay[7] = say_quant(p, c.y, 7); pay[8] = say_quant(p, c.z, 8); pay[9] = say_quant(p, c.w, 9);
    }
  }
  sh.x[l] = x; sh.y[l] = y;
  const bool is_done = done && done[ec];
  const uint32_t tick = (uint32_t)s.tick[ec];
  const uint64_t gid = (((uint64_t)p.gid_hi << 32) | p.gid_lo) + (uint64_t)ec;
  const uint32_t speakers = see_hballot(is_player && said && card < S2D_CARD_RED, half) & kAll;
  see_fence();

  const bool right = l >= 11;
  const bool listens = is_player && !is_done && card < S2D_CARD_RED;
  Record ours{}, theirs{};
  float cap_our_w = 0.0f, cap_opp_w = 0.0f, att_w = 0.0f;
  if (is_player && is_done) {
    cap_our = cap_opp = p.hear_max; att = -1;
    cap_our_w = cap_opp_w = (float)p.hear_max;
  }
  if (listens) {
    // 3. the attention command, on own-frame slots
    if (att < -1 || att >= NP) att = -1;
    const int own_l = l % 11;
    if (cmd == -1.0f) {
      att = -1;
    } else if (cmd >= 1.0f && cmd <= 22.0f && cmd == rintf(cmd)) {
      const int a = (int)cmd - 1;
      if (a != own_l) att = a;
    }
    // 4. the capacities
    if (cap_our < 0 || cap_our > p.hear_max) cap_our = p.hear_max;
    if (cap_opp < 0 || cap_opp > p.hear_max) cap_opp = p.hear_max;
    cap_our = min(cap_our + p.hear_inc, p.hear_max);
    cap_opp = min(cap_opp + p.hear_inc, p.hear_max);
    // 5. the candidates: speakers within the cut distance, on own-frame values
    const float sg = right ? -1.0f : 1.0f;
    const float ax = sg * x, ay = sg * y;
    const float face = norm_deg_any(own_body(body, right) + neck);
    uint32_t cand = 0u;
    const uint32_t others = speakers & ~(1u << l);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      if ((others >> j) & 1u) {
        const float dx = sg * sh.x[j] - ax, dy = sg * sh.y[j] - ay;
        if (hypot2(dx, dy) <= p.cut) cand |= 1u << j;
      }
    }
    const uint32_t mine = right ? (kAll & ~kLeft) : kLeft;
    const int att_raw = att < 0 ? -1 : (right ? swap_side(att) : att);
    // 6. one message per side
    ours = hear_side(p, sh, l, right, cand & mine, att_raw, cap_our, true, ax, ay, face, sg, gid, tick);
    theirs = hear_side(p, sh, l, right, cand & ~mine, att_raw, cap_opp, false, ax, ay, face, sg, gid, tick);
    cap_our_w = (float)cap_our; cap_opp_w = (float)cap_opp; att_w = (float)(att + 1);
  }
  if (is_player) {
    record_store(sh, l, 0, ours, cap_our_w, att_w);
    record_store(sh, l, 4, theirs, cap_opp_w, 0.0f);
    if (valid && (listens || is_done)) { hs.cap_our[k] = cap_our; hs.cap_opp[k] = cap_opp; hs.attention[k] = att; }
  }
  see_fence();
  if (valid) {
    float4* out = reinterpret_cast<float4*>(hs.hear + e * (int64_t)(NP * S2D_HEAR_DIM));
#pragma unroll
    for (int i = l; i < kMatchVec; i += kHalf) out[i] = sh.row[row_at(i / kRowVec, i % kRowVec)];
  }
}

// one thread per slot of the [N][24] planes; the threads of the 22 players write their rows as well
__global__ __launch_bounds__(kBlock) void s2d_match_hear_reset_kernel(int hear_max, S2DMatchHear hs, const uint8_t* __restrict__ mask, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n * SLOTS) return;
  const int64_t e = i / SLOTS;
  const int l = (int)(i - e * SLOTS);
  if (mask && !mask[e]) return;
  hs.cap_our[i] = hear_max; hs.cap_opp[i] = hear_max; hs.attention[i] = -1;
  if (l >= NP) return;
  float4* row = reinterpret_cast<float4*>(hs.hear + (e * NP + l) * (int64_t)S2D_HEAR_DIM);
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f), capq = make_float4((float)hear_max, 0.0f, 0.0f, 0.0f);
#pragma unroll
  for (int q = 0; q < kRowVec; ++q) row[q] = (q == 1 || q == 5) ? capq : zero;
}

int hfail(int code, const std::string& msg) { s2d_internal_set_error(msg.c_str()); return code; }

struct DeviceGuard {
  int prev = -1; bool ok = false;
  explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) == hipSuccess) ok = (prev == dev) || (hipSetDevice(dev) == hipSuccess); }
  ~DeviceGuard() { if (ok && prev >= 0) (void)hipSetDevice(prev); }
};

bool whole_in(double v, double lo, double hi) { return std::isfinite(v) && v >= lo && v <= hi && v == std::floor(v); }

const char* hear_params_error(const S2DHearParams* v) {
  if (!v) return "NULL hear parameters";
  if (!std::isfinite(v->audio_cut_dist) || v->audio_cut_dist < 0.0) return "audio_cut_dist must be finite and >= 0";
  if (!whole_in(v->hear_max, 1.0, 1.0e6)) return "hear_max must be a whole number in [1, 1e6]";
  if (!whole_in(v->hear_inc, 0.0, 1.0e6)) return "hear_inc must be a whole number in [0, 1e6]";
  if (!whole_in(v->hear_decay, 1.0, 1.0e6)) return "hear_decay must be a whole number in [1, 1e6]";
  if (!whole_in(v->say_msg_size, 1.0, (double)S2D_SAY_WORDS)) return "say_msg_size must be a whole number in [1, S2D_SAY_WORDS]";
  if (!whole_in(v->say_levels, 3.0, 4097.0) || std::fmod(v->say_levels, 2.0) != 1.0) return "say_levels must be an odd whole number in [3, 4097]";
  return nullptr;
}

struct Span { uintptr_t lo, hi; };
Span span_of(const void* p, int64_t bytes) { return Span{reinterpret_cast<uintptr_t>(p), reinterpret_cast<uintptr_t>(p) + (uintptr_t)bytes}; }
bool overlap(const Span& a, const Span& b) { return a.lo && b.lo && a.lo < b.hi && b.lo < a.hi; }

// the four planes of `hs`, then (when given) neck, say and done: NULL, alignment and overlap of every written plane with the rest
const char* hear_planes_error(const S2DMatchHear* hs, int64_t n, const float* neck, const float* say, const uint8_t* done) {
  if (!hs || !hs->cap_our || !hs->cap_opp || !hs->attention || !hs->hear) return "NULL hear plane";
  if ((reinterpret_cast<uintptr_t>(hs->cap_our) | reinterpret_cast<uintptr_t>(hs->cap_opp) | reinterpret_cast<uintptr_t>(hs->attention)) & 3u)
    return "the hear capacity and attention planes must be 4-byte aligned";
  if (reinterpret_cast<uintptr_t>(hs->hear) & 15u) return "the hear rows must be 16-byte aligned";
  if (reinterpret_cast<uintptr_t>(neck) & 3u) return "neck must be 4-byte aligned (float)";
  if (reinterpret_cast<uintptr_t>(say) & 15u) return "say must be 16-byte aligned";
  const int64_t plane = n * SLOTS * 4;
  const Span sp[7] = {span_of(hs->hear, n * NP * S2D_HEAR_DIM * 4), span_of(hs->cap_our, plane), span_of(hs->cap_opp, plane),
                      span_of(hs->attention, plane), span_of(neck, plane), span_of(say, n * NP * S2D_SAY_ROW * 4), span_of(done, n)};
  for (int a = 0; a < 4; ++a)
    for (int b = a + 1; b < 7; ++b)
      if (overlap(sp[a], sp[b])) return "a hear plane overlaps another plane";
  return nullptr;
}

struct EngineView { S2DMatchBuffers buf; uint32_t keys[4]; int device; };
int engine_view(S2DMatchHandle h, EngineView& v) {
  if (!h) return hfail(S2D_EINVAL, "NULL handle");
  int rc = s2d_match_buffers(h, &v.buf);
  if (rc != S2D_OK) return rc;
  return s2d_match_internal_keys(h, v.keys, &v.device);
}

}  // namespace

S2D_API void s2d_match_hear_default_params(S2DHearParams* v) {
  if (!v) return;
  v->audio_cut_dist = 50.0; v->hear_max = 1.0; v->hear_inc = 1.0; v->hear_decay = 1.0;
  v->say_msg_size = (double)S2D_SAY_WORDS; v->say_levels = 73.0;
}

S2D_API int s2d_match_hear_validate(const S2DHearParams* v) {
  const char* err = hear_params_error(v);
  return err ? hfail(S2D_EINVAL, err) : S2D_OK;
}

S2D_API int s2d_match_hear_reset(S2DMatchHandle h, const S2DHearParams* prm, const S2DMatchHear* hear, const uint8_t* mask_dev, void* stream) {
  EngineView ev;
  int rc = engine_view(h, ev);
  if (rc != S2D_OK) return rc;
  if (const char* err = hear_params_error(prm)) return hfail(S2D_EINVAL, err);
  if (const char* err = hear_planes_error(hear, ev.buf.n_envs, nullptr, nullptr, mask_dev)) return hfail(S2D_EINVAL, err);
  DeviceGuard guard(ev.device);
  const unsigned grid = (unsigned)((ev.buf.n_envs * SLOTS + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(s2d_match_hear_reset_kernel, dim3(grid), dim3(kBlock), 0, static_cast<hipStream_t>(stream), (int)prm->hear_max, *hear,
                     mask_dev, ev.buf.n_envs);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return hfail(S2D_EHIP, std::string("hear reset launch: ") + hipGetErrorString(e));
  return S2D_OK;
}

S2D_API int s2d_match_hear_step(S2DMatchHandle h, const S2DHearParams* prm, const S2DMatchHear* hear, const float* neck_dev,
                                const float* say_dev, const uint8_t* done_dev, void* stream) {
  EngineView ev;
  int rc = engine_view(h, ev);
  if (rc != S2D_OK) return rc;
  if (const char* err = hear_params_error(prm)) return hfail(S2D_EINVAL, err);
  if (const char* err = hear_planes_error(hear, ev.buf.n_envs, neck_dev, say_dev, done_dev)) return hfail(S2D_EINVAL, err);
  const S2DMatchBuffers& b = ev.buf;
  const HearState st{b.x, b.y, b.body, b.card, b.tick};
  DeviceGuard guard(ev.device);
  const unsigned grid = (unsigned)((b.n_envs + kEnvsPerBlock - 1) / kEnvsPerBlock);
  hipLaunchKernelGGL(s2d_match_hear_step_kernel, dim3(grid), dim3(kBlock), 0, static_cast<hipStream_t>(stream), hear_params(*prm, ev.keys), st,
                     *hear, neck_dev, say_dev, done_dev, b.n_envs);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return hfail(S2D_EHIP, std::string("hear step launch: ") + hipGetErrorString(e));
  return S2D_OK;
}
