// s2d_belief.hip -- the belief layer of the 11v11 match engine for MI355X (gfx950): each agent's memory of what it has seen
// (include/s2d_match.h, "Belief").  The project's own filter over see rows (no parity claim to librcsc's world model);
// tests/belief_ref.c is an independent CPU restatement this file matches bit for bit.
//
// A unit of its own and engine-free, as s2d_gae: raw device pointers, the current device, any of its streams.  It reads see rows
// and nothing else -- no engine handle, no state plane -- so it cannot leak ground truth, and no kernel of another unit knows of it.
//
// Mapping of the scan kernel: ONE AGENT PER HALF-WAVE, lane = entry (0 the ball, 1..21 the player rows; lanes 22..31 help with
// the copies).  The belief row lives in LDS for the whole launch; the loop over the T rows runs inside the kernel.  Per row:
//   - the see row comes in as two float4 per lane (the next one is already in flight) and is staged in LDS;
//   - every lane ages its own entry (steps 1, 2);
//   - lane = SIGHTING: the 21 player rows and the ball are located in parallel (one sincos each) into an LDS tile;
//   - first pass: every entry looks for the last level-4 row that names it (22 broadcast reads);
//   - second pass: sequential over the level 1-3 rows (a ballot names them), a half-wave minimum over the candidates' distances
//     (four DPP rounds and one row swap) and a ballot for the lowest row at that distance;
//   - ghosts per entry; the row leaves as whole 64-byte lines, one float4 per lane and store instruction.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "s2d_device.h"
#include "../../include/s2d_match.h"

#define S2D_API extern "C" __attribute__((visibility("default")))

extern "C" void s2d_internal_set_error(const char* msg);

namespace {

constexpr int kBlock = 256;
constexpr int kHalf = 32;
constexpr int kAgentsPerBlock = kBlock / kHalf;
constexpr int kVec = S2D_BELIEF_DIM / 4;                 // 48 float4 per row
constexpr int NP = S2D_MATCH_PLAYERS;
constexpr int kEntries = 22;                             // the ball and 21 player rows
constexpr int kSightings = 22;                           // 21 player rows of the see row, then its ball
static_assert(S2D_BELIEF_DIM == S2D_SEE_DIM && S2D_BELIEF_BALL == S2D_SEE_BALL && S2D_BELIEF_PLAYERS == S2D_SEE_PLAYERS &&
              S2D_BELIEF_ROW_WORDS == 8 && S2D_SEE_ROW_WORDS == 8, "a belief row is laid out over a see row");
static_assert(kVec > kHalf && kVec <= 2 * kHalf, "a half-wave moves a row as two float4 per lane");

// S2DBeliefParams rounded once (double -> float)
struct BeliefParams { float ball_decay, player_decay, view_angle[3], match_dist, match_rate, ghost_margin, count_max; };

BeliefParams belief_params(const S2DBeliefParams& v) {
  BeliefParams p;
  p.ball_decay = (float)v.ball_decay; p.player_decay = (float)v.player_decay;
  for (int i = 0; i < 3; ++i) p.view_angle[i] = (float)v.view_angle[i];
  p.match_dist = (float)v.match_dist; p.match_rate = (float)v.match_rate; p.ghost_margin = (float)v.ghost_margin;
  p.count_max = (float)v.count_max;
  return p;
}

struct BeliefShared {                                    // one agent (half-wave)
  float4 row[kVec];                                      // the belief row: the state between see rows
  float4 see[kVec];                                      // the see row being taken in
  float4 fix[kHalf];                                     // per sighting: X, Y, VX, VY
  float body[kHalf];                                     // per sighting: the absolute body direction (level 4)
  int target[kHalf];                                     // per sighting: the entry a level-4 row (or the ball) names, -1 none
};

S2D_DEV void half_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
S2D_DEV uint32_t half_ballot(bool pred, int half) { return (uint32_t)(__ballot(pred) >> (half * kHalf)); }
// The minimum over the 32 lanes of a half-wave, in every lane: quad permutes and row mirrors in the VALU's data path, then one
// swap of the two rows of 16 through the LDS crossbar (bit mode: lane ^ 16).  The values are never NaN.
S2D_DEV float half_min(float v) {
  constexpr int kQuadXor1 = 0xB1, kQuadXor2 = 0x4E, kRowHalfMirror = 0x141, kRowMirror = 0x140, kSwapRows = 0x401F;
  int x = __float_as_int(v);
  v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(x, x, kQuadXor1, 0xf, 0xf, true)));
  x = __float_as_int(v);
  v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(x, x, kQuadXor2, 0xf, 0xf, true)));
  x = __float_as_int(v);
  v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(x, x, kRowHalfMirror, 0xf, 0xf, true)));
  x = __float_as_int(v);
  v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(x, x, kRowMirror, 0xf, 0xf, true)));
  return fminf(v, __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), kSwapRows)));
}
S2D_DEV float older(float c, float count_max) { return c + 1.0f < count_max ? c + 1.0f : count_max; }

struct Entry { float x, y, vx, vy, body, pos_count, vel_count, body_count; };
S2D_DEV void forget(Entry& e, float count_max) {
  e.x = e.y = e.vx = e.vy = e.body = 0.0f;
  e.pos_count = e.vel_count = e.body_count = count_max;
}

template <bool RECORD>
__global__ __launch_bounds__(kBlock) void s2d_match_belief_scan_kernel(BeliefParams p, const float* __restrict__ see,
                                                                       const uint8_t* __restrict__ reset, float* belief,
                                                                       float* __restrict__ out, int n_steps, int64_t n_matches,
                                                                       int k, uint32_t mask) {
  __shared__ BeliefShared sh_all[kAgentsPerBlock];
  BeliefShared& sh = sh_all[threadIdx.x / kHalf];
  const int l = threadIdx.x & (kHalf - 1);
  const int half = (threadIdx.x >> 5) & 1;
  const int64_t n_agents = n_matches * k;
  const int64_t a = (int64_t)blockIdx.x * kAgentsPerBlock + threadIdx.x / kHalf;
  const bool valid = a < n_agents;
  const int64_t ac = valid ? a : n_agents - 1;
  const int64_t e = ac / k;
  const int r = (int)(ac - e * k);
  uint32_t rest = mask;
  for (int i = 0; i < r; ++i) rest &= rest - 1u;
  const int u = __builtin_ctz(rest) % 11;                // the agent's own index
  const bool has2 = l + kHalf < kVec;
  const int64_t step_vecs = n_agents * kVec;             // float4 per time step of a record

  float4* brow = reinterpret_cast<float4*>(belief) + ac * kVec;
  const float4* srow = reinterpret_cast<const float4*>(see) + ac * kVec;
  float4* orow = RECORD ? reinterpret_cast<float4*>(out) + ac * kVec : nullptr;
  sh.row[l] = brow[l];
  if (has2) sh.row[l + kHalf] = brow[l + kHalf];
  float4 s0 = srow[l], s1 = has2 ? srow[l + kHalf] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  int flag = reset ? (int)reset[e] : 0;

  const bool is_entry = l < kEntries;
  const bool is_ball = l == 0;
  const int rv = is_ball ? S2D_BELIEF_BALL / 4 : S2D_BELIEF_PLAYERS / 4 + 2 * (l - 1);   // this entry's two float4 of the row
  const int sv = l < 21 ? S2D_SEE_PLAYERS / 4 + 2 * l : S2D_SEE_BALL / 4;                // this sighting's two float4 of the see row
  const float cm = p.count_max;

  for (int t = 0; t < n_steps; ++t) {
    sh.see[l] = s0;
    if (has2) sh.see[l + kHalf] = s1;
    const bool do_reset = flag != 0;
    if (t + 1 < n_steps) {                               // the next row and flag are in flight while this one is taken in
      const float4* nx = srow + (int64_t)(t + 1) * step_vecs;
      s0 = nx[l];
      if (has2) s1 = nx[l + kHalf];
      if (reset) flag = (int)reset[(int64_t)(t + 1) * n_matches + e];
    }
    half_fence();

    // this lane's entry, steps 1 and 2
    Entry en{};
    bool updated = false;
    if (is_entry) {
      const float4 w0 = sh.row[rv], w1 = sh.row[rv + 1];
      en.x = w0.x; en.y = w0.y; en.vx = w0.z; en.vy = w0.w;
      if (is_ball) { en.pos_count = w1.x; en.vel_count = cm; en.body_count = cm; }
      else { en.body = w1.x; en.pos_count = w1.y; en.vel_count = w1.z; en.body_count = w1.w; }
      if (do_reset) forget(en, cm);
      if (en.pos_count < cm) {
        const float decay = is_ball ? p.ball_decay : p.player_decay;
        en.x = en.x + en.vx; en.y = en.y + en.vy;
        en.vx = en.vx * decay; en.vy = en.vy * decay;
      }
      en.pos_count = older(en.pos_count, cm); en.vel_count = older(en.vel_count, cm); en.body_count = older(en.body_count, cm);
      if (en.pos_count == cm) forget(en, cm);
    }

    const float4 self0 = sh.see[0], self1 = sh.see[1];
    const float sx = self0.x, sy = self0.y, svx = self0.z, svy = self0.w, face = self1.z, code = self1.w;
    const bool can = sh.see[2].x == 1.0f && sh.see[3].w < (float)S2D_CARD_RED;   // uniform within the half-wave
    if (can) {
      uint32_t pending;                                  // the level 1-3 rows of the see row, one bit each
      // lane = sighting: locate it
      {
        float level = 0.0f, team = 0.0f, unum = 0.0f, dist = 0.0f, dir = 0.0f, dchg = 0.0f, rchg = 0.0f, brel = 0.0f;
        if (l < kSightings) {
          const float4 a0 = sh.see[sv], a1 = sh.see[sv + 1];
          if (l < 21) { level = a0.x; team = a0.y; unum = a0.z; dist = a0.w; dir = a1.x; dchg = a1.y; rchg = a1.z; brel = a1.w; }
          else { level = a0.x; dist = a0.y; dir = a0.z; dchg = a0.w; rchg = a1.x; }
        }
        float s, c;
        sincos_deg(norm_deg_any(face + dir), s, c);
        const float X = fmaf(dist, c, sx), Y = fmaf(dist, s, sy);
        float VX = svx, VY = svy;
        if (dist != 0.0f) {
          const float vr = dchg, vt = (rchg * 0.017453292519943295f) * dist;
          VX = fmaf(vr, c, -(vt * s)) + svx;
          VY = fmaf(vr, s, vt * c) + svy;
        }
        int target = -1;
        if (l < 21) {
          if (level == 4.0f && unum >= 1.0f && unum <= 11.0f && unum == rintf(unum)) {
            const int n = (int)unum;
            if (team > 0.0f) { if (n - 1 != u) target = 1 + (n - 1 < u ? n - 1 : n - 2); }
            else if (team < 0.0f) target = 1 + n + 9;
          }
        } else if (l == 21) {
          target = level >= 1.0f ? 0 : -1;
        }
        sh.fix[l] = make_float4(X, Y, VX, VY);
        sh.body[l] = norm_deg_any(brel + face);
        sh.target[l] = target;
        pending = half_ballot(l < 21 && (level == 1.0f || level == 2.0f || level == 3.0f), half);
      }
      half_fence();
      // first pass: lane = entry again; the last sighting that names it
      if (is_entry) {
        int hit = -1;
#pragma unroll
        for (int q = 0; q < kSightings; ++q) hit = sh.target[q] == l ? q : hit;
        if (hit >= 0) {
          const float4 f = sh.fix[hit];
          en.x = f.x; en.y = f.y; en.pos_count = 0.0f;
          updated = true;
          if (!is_ball) {
            en.vx = f.z; en.vy = f.w; en.body = sh.body[hit]; en.vel_count = 0.0f; en.body_count = 0.0f;
          } else if (sh.see[S2D_SEE_BALL / 4].x == 4.0f) {
            en.vx = f.z; en.vy = f.w;
          }
        }
      }
      // second pass: the level 1-3 rows, one after the other
#pragma unroll 1
      while (pending != 0u) {                            // (uniform within the half-wave)
        const int q = __builtin_ctz(pending);
        pending &= pending - 1u;
        const float4 a0 = sh.see[S2D_SEE_PLAYERS / 4 + 2 * q];
        const float team = a0.y, dist = a0.w;
        const float4 f = sh.fix[q];
        const float tol = fmaf(p.match_rate, dist, p.match_dist), tol2 = tol * tol;
        const int j = l - 1;                             // this lane's player row
        bool cand = is_entry && !is_ball && !updated && en.pos_count < cm;
        cand = cand && (team > 0.0f ? j < 10 : (team < 0.0f ? j >= 10 : true));
        float best = __builtin_inff();
        if (cand) {
          best = sq2(f.x - en.x, f.y - en.y);
          cand = best <= tol2;
          best = cand ? best : __builtin_inff();
        }
        const float least = half_min(best);              // (every lane of the half-wave takes part: no short circuit around it)
        const uint32_t nearest = half_ballot(cand && best == least, half);   // the candidates at the smallest distance
        if (nearest != 0u && l == __builtin_ctz(nearest)) { en.x = f.x; en.y = f.y; en.pos_count = 0.0f; updated = true; }   // ties: the lowest row
      }
      // ghosts
      if (is_entry && !updated && en.pos_count < cm) {
        const int wi = code == 1.0f ? 0 : (code == 3.0f ? 2 : 1);
        const float va = wi == 0 ? p.view_angle[0] : (wi == 2 ? p.view_angle[2] : p.view_angle[1]);
        const float cone = 0.5f * va - p.ghost_margin;
        const float dx = en.x - sx, dy = en.y - sy;
        const float d = hypot2(dx, dy);
        if (d > 0.0f && fabsf(norm_deg_any(atan2_deg(dy, dx) - face)) <= cone) forget(en, cm);
      }
    }

    // the row: this lane's entry, the self words and the game words (steps 3 to 5 are done)
    if (is_entry) {
      sh.row[rv] = make_float4(en.x, en.y, en.vx, en.vy);
      if (is_ball) {
        const float4 g = sh.see[S2D_SEE_BALL / 4 + 1];
        sh.row[rv + 1] = make_float4(en.pos_count, g.y, g.z, g.w);
      } else {
        sh.row[rv + 1] = make_float4(en.body, en.pos_count, en.vel_count, en.body_count);
      }
    } else if (l < kEntries + 4) {
      sh.row[l - kEntries] = sh.see[l - kEntries];       // lanes 22..25: the four float4 of the self words
    }
    half_fence();
    if (RECORD && valid) {
      float4* o = orow + (int64_t)t * step_vecs;
      o[l] = sh.row[l];
      if (has2) o[l + kHalf] = sh.row[l + kHalf];
    }
  }
  if (valid) {
    brow[l] = sh.row[l];
    if (has2) brow[l + kHalf] = sh.row[l + kHalf];
  }
}

// one thread per float4 of the rows
__global__ __launch_bounds__(kBlock) void s2d_match_belief_reset_kernel(float4* __restrict__ belief, const uint8_t* __restrict__ mask,
                                                                        int64_t n_matches, int k) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_matches * k * kVec) return;
  const int64_t a = i / kVec;
  const int v = (int)(i - a * kVec);
  if (mask && !mask[a / k]) return;
  const float L = S2D_BELIEF_COUNT_LIMIT;
  float4 w = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (v == S2D_BELIEF_BALL / 4 + 1) w.x = L;                                  // the ball's pos_count
  else if (v >= S2D_BELIEF_PLAYERS / 4 && (v & 1)) { w.y = L; w.z = L; w.w = L; }   // body | pos_count, vel_count, body_count
  belief[i] = w;
}

int bfail(const std::string& msg) { s2d_internal_set_error(msg.c_str()); return S2D_EINVAL; }

const char* belief_params_error(const S2DBeliefParams* v) {
  if (!v) return "NULL belief parameters";
  const double all[] = {v->ball_decay, v->player_decay, v->view_angle[0], v->view_angle[1], v->view_angle[2], v->match_dist,
                        v->match_rate, v->ghost_margin, v->count_max};
  for (double d : all) if (!std::isfinite(d)) return "belief parameters must be finite";
  if (!(v->ball_decay > 0.0 && v->ball_decay <= 1.0 && v->player_decay > 0.0 && v->player_decay <= 1.0))
    return "ball_decay and player_decay must lie in (0, 1]";
  for (int i = 0; i < 3; ++i)
    if (!(v->view_angle[i] > 0.0 && v->view_angle[i] <= 360.0)) return "view_angle must lie in (0, 360]";
  if (v->match_dist < 0.0 || v->match_rate < 0.0 || v->ghost_margin < 0.0) return "match_dist, match_rate and ghost_margin must be >= 0";
  if (!(v->count_max >= 1.0 && v->count_max <= (double)S2D_BELIEF_COUNT_LIMIT) || v->count_max != std::floor(v->count_max))
    return "count_max must be a whole number in [1, 16777216]";
  return nullptr;
}

const char* rows_error(int64_t n_matches, uint32_t slot_mask) {
  if (n_matches < 1 || n_matches > (int64_t)1 << 24) return "n_matches must be in [1, 2^24]";
  if (slot_mask == 0u || (slot_mask >> NP) != 0u) return "slot_mask must be a non-empty set of bits 0..21 (0x3FFFFF = all agents)";
  return nullptr;
}

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace

S2D_API void s2d_match_belief_default_params(S2DBeliefParams* v) {
  if (!v) return;
  v->ball_decay = 0.94; v->player_decay = 0.4;
  v->view_angle[0] = 60.0; v->view_angle[1] = 120.0; v->view_angle[2] = 180.0;
  v->match_dist = 3.0; v->match_rate = 0.1; v->ghost_margin = 5.0;
  v->count_max = 1000.0;
}

S2D_API int s2d_match_belief_validate(const S2DBeliefParams* v) {
  const char* err = belief_params_error(v);
  return err ? bfail(err) : S2D_OK;
}

S2D_API int s2d_match_belief_reset(float* belief_dev, int64_t n_matches, uint32_t slot_mask, const uint8_t* mask_dev, void* stream) {
  if (!belief_dev) return bfail("s2d_match_belief_reset: NULL belief buffer");
  if (const char* err = rows_error(n_matches, slot_mask)) return bfail(std::string("s2d_match_belief_reset: ") + err);
  if (reinterpret_cast<uintptr_t>(belief_dev) & 15u) return bfail("s2d_match_belief_reset: the belief buffer must be 16-byte aligned");
  const int k = __builtin_popcount(slot_mask);
  const int64_t vecs = n_matches * k * kVec;
  hipLaunchKernelGGL(s2d_match_belief_reset_kernel, dim3((unsigned)((vecs + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), reinterpret_cast<float4*>(belief_dev), mask_dev, n_matches, k);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) {
    s2d_internal_set_error((std::string("s2d_match_belief_reset: launch: ") + hipGetErrorString(e)).c_str());
    return S2D_EHIP;
  }
  return S2D_OK;
}

S2D_API int s2d_match_belief_scan(const S2DBeliefParams* prm, const float* see_dev, const uint8_t* reset_dev, float* belief_dev,
                                  float* out_dev, int n_steps, int64_t n_matches, uint32_t slot_mask, void* stream) {
  if (!prm || !see_dev || !belief_dev) return bfail("s2d_match_belief_scan: prm, see_dev and belief_dev must be non-NULL");
  if (const char* err = rows_error(n_matches, slot_mask)) return bfail(std::string("s2d_match_belief_scan: ") + err);
  if (n_steps < 1) return bfail("s2d_match_belief_scan: n_steps must be >= 1");
  if ((reinterpret_cast<uintptr_t>(see_dev) | reinterpret_cast<uintptr_t>(belief_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 15u)
    return bfail("s2d_match_belief_scan: see_dev, belief_dev and out_dev must be 16-byte aligned");
  if (const char* err = belief_params_error(prm)) return bfail(std::string("s2d_match_belief_scan: ") + err);
  const int k = __builtin_popcount(slot_mask);
  const size_t state_bytes = (size_t)n_matches * k * S2D_BELIEF_DIM * sizeof(float), record_bytes = state_bytes * (size_t)n_steps;
  if (overlap(belief_dev, state_bytes, see_dev, record_bytes)) return bfail("s2d_match_belief_scan: belief_dev overlaps see_dev");
  if (out_dev && (overlap(out_dev, record_bytes, belief_dev, state_bytes) || overlap(out_dev, record_bytes, see_dev, record_bytes)))
    return bfail("s2d_match_belief_scan: out_dev overlaps belief_dev or see_dev");
  const int64_t agents = n_matches * k;
  const unsigned grid = (unsigned)((agents + kAgentsPerBlock - 1) / kAgentsPerBlock);
  const BeliefParams p = belief_params(*prm);
  if (out_dev)
    hipLaunchKernelGGL(s2d_match_belief_scan_kernel<true>, dim3(grid), dim3(kBlock), 0, static_cast<hipStream_t>(stream), p, see_dev,
                       reset_dev, belief_dev, out_dev, n_steps, n_matches, k, slot_mask);
  else
    hipLaunchKernelGGL(s2d_match_belief_scan_kernel<false>, dim3(grid), dim3(kBlock), 0, static_cast<hipStream_t>(stream), p, see_dev,
                       reset_dev, belief_dev, out_dev, n_steps, n_matches, k, slot_mask);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) {
    s2d_internal_set_error((std::string("s2d_match_belief_scan: launch: ") + hipGetErrorString(e)).c_str());
    return S2D_EHIP;
  }
  return S2D_OK;
}
