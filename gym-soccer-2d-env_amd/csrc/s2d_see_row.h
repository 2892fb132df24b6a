// s2d_see_row.h -- the see row and the vision step of the 11v11 vision layer (include/s2d_match.h, "Vision") as device functions.
// Two kernels execute this source: s2d_match_see_kernel / s2d_match_vision_step_kernel (s2d_see.hip: state from memory, one launch
// per call) and the SEE instantiations of the cycle kernel (s2d_match_cycle.h: state from registers, every cycle of a launch).  A see
// row recorded by the cycle kernel is therefore bitwise the row s2d_match_see returns at that moment.
//
// Mapping (both callers): ONE MATCH PER HALF-WAVE, lane = object (0..21 players, 22 the ball).  Per agent every lane derives the
// eight words of its object; the place of a player's row (left to right across the view) is a COUNT over the half-wave's keys (22
// broadcast reads of an LDS tile, no sort loop and no divergence over agents); the row is assembled in LDS.
#ifndef S2D_SEE_ROW_H_
#define S2D_SEE_ROW_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "s2d_device.h"
#include "../../include/s2d_match.h"

namespace s2d_see {

constexpr int kSeeHalf = 32;
constexpr int kSeeVec = S2D_SEE_DIM / 4;                 // 48 float4 per row
constexpr int kSeeOthers = S2D_MATCH_PLAYERS - 1;        // 21 player rows
static_assert(S2D_SEE_DIM == S2D_SEE_PLAYERS + kSeeOthers * S2D_SEE_ROW_WORDS, "row layout");
static_assert(S2D_SEE_SELF == 0 && S2D_SEE_BALL == 16 && S2D_SEE_PLAYERS == 24 && S2D_SEE_ROW_WORDS == 8, "row layout");
static_assert(kSeeVec > kSeeHalf && kSeeVec <= 2 * kSeeHalf, "a half-wave stores a row as two float4 per lane");
enum { SEE_SIDE_NONE = 0, SEE_SIDE_LEFT = 1, SEE_SIDE_RIGHT = 2 };

// S2DVisionParams rounded once (double -> float); the reciprocals are the floats of the double quotients
struct SeeParams {
  float view_angle[3]; int interval[3];
  float visible, dist_q, inv_dist_q, dist_r, inv_dist_r, dchg_q, inv_dchg_q, rchg_q, inv_rchg_q;
  float unum_far, unum_too_far, inv_unum_band, team_far, team_too_far, inv_team_band;
  float min_moment, max_moment, min_neck, max_neck;
  uint32_t seed_lo, seed_hi, gid_lo, gid_hi;
};

inline SeeParams see_params(const S2DVisionParams& v, const uint32_t keys[4]) {
  SeeParams p;
  for (int i = 0; i < 3; ++i) { p.view_angle[i] = (float)v.view_angle[i]; p.interval[i] = (int)v.see_interval[i]; }
  p.visible = (float)v.visible_distance;
  p.dist_q = (float)v.dist_quantize_step; p.inv_dist_q = (float)(1.0 / v.dist_quantize_step);
  p.dist_r = (float)v.dist_round; p.inv_dist_r = (float)(1.0 / v.dist_round);
  p.dchg_q = (float)v.dist_chg_quantize; p.inv_dchg_q = (float)(1.0 / v.dist_chg_quantize);
  p.rchg_q = (float)v.dir_chg_quantize; p.inv_rchg_q = (float)(1.0 / v.dir_chg_quantize);
  p.unum_far = (float)v.unum_far_length; p.unum_too_far = (float)v.unum_too_far_length;
  p.team_far = (float)v.team_far_length; p.team_too_far = (float)v.team_too_far_length;
  const double ub = v.unum_too_far_length - v.unum_far_length, tb = v.team_too_far_length - v.team_far_length;
  p.inv_unum_band = ub > 0.0 ? (float)(1.0 / ub) : 0.0f;
  p.inv_team_band = tb > 0.0 ? (float)(1.0 / tb) : 0.0f;
  p.min_moment = (float)v.min_neck_moment; p.max_moment = (float)v.max_neck_moment;
  p.min_neck = (float)v.min_neck_angle; p.max_neck = (float)v.max_neck_angle;
  p.seed_lo = keys[0]; p.seed_hi = keys[1]; p.gid_lo = keys[2]; p.gid_hi = keys[3];
  return p;
}

S2D_DEV void see_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
S2D_DEV uint32_t see_hballot(bool pred, int half) { return (uint32_t)(__ballot(pred) >> (half * kSeeHalf)); }
S2D_DEV float own_body(float b, bool right) { return right ? (b > 0.0f ? b - 180.0f : b + 180.0f) : b; }
S2D_DEV float side_word(int side, int ours) { return side == ours ? 1.0f : (side == SEE_SIDE_NONE ? 0.0f : -1.0f); }
S2D_DEV int width_index(int code) { return code == 1 ? 0 : (code == 3 ? 2 : 1); }   // anything but narrow / wide reads as normal
// (constant indices and selects: a lane-varying index into a kernel argument would go through scratch memory.  The three values
// are passed by value: with the array handed on by reference the compiler turned the selects back into an indexed load from a
// scratch copy of it, 16 bytes of scratch per lane in every kernel that builds a row)
S2D_DEV float pick3(float a0, float a1, float a2, int i) { return i == 0 ? a0 : (i == 2 ? a2 : a1); }
S2D_DEV int pick3(int a0, int a1, int a2, int i) { return i == 0 ? a0 : (i == 2 ? a2 : a1); }
S2D_DEV float view_angle_of(const SeeParams& p, int wi) { return pick3(p.view_angle[0], p.view_angle[1], p.view_angle[2], wi); }
S2D_DEV int interval_of(const SeeParams& p, int wi) { return pick3(p.interval[0], p.interval[1], p.interval[2], wi); }
S2D_DEV float quant(float v, float q, float inv_q) { return rintf(v * inv_q) * q; }

// What a row reads of one lane's object (zero where the lane has no such word: x .. vy up to the ball, the rest for players only)
// and of its match.  The see kernel loads them from memory, the cycle kernel takes them from its registers at the start of a cycle.
struct SeeIn {
  float x, y, vx, vy, body, neck, stamina, effort, recovery, capacity;
  int card, width, wait;
  int mode, mode_side, cycle;
  uint32_t tick;
};
struct SeeFacts {                                        // one match (half-wave): the lanes' state and the order keys
  float x[kSeeHalf], y[kSeeHalf], vx[kSeeHalf], vy[kSeeHalf], body[kSeeHalf], neck[kSeeHalf];
  int width[kSeeHalf], wait[kSeeHalf], card[kSeeHalf];
  float2 key[kSeeHalf];
};

// every lane's words into the half-wave's facts; ends with a wave fence
S2D_DEV void see_facts(SeeFacts& sh, const SeeIn& in, int l) {
  sh.x[l] = in.x; sh.y[l] = in.y; sh.vx[l] = in.vx; sh.vy[l] = in.vy; sh.body[l] = in.body; sh.neck[l] = in.neck;
  sh.width[l] = in.width; sh.wait[l] = in.wait; sh.card[l] = in.card;
  see_fence();
}

// The see row of agent pa (uniform within the half-wave) into `row` (LDS, 48 float4), from the facts and this lane's words; gid =
// the match's Philox id.  Called by all 64 lanes; after the closing wave fence all 48 float4 hold the row.  THE definition of a row.
S2D_DEV void see_row(const SeeParams& p, SeeFacts& sh, const SeeIn& in, int l, int half, int pa, uint64_t gid, float4* row) {
  constexpr int NP = S2D_MATCH_PLAYERS, BALL = S2D_MATCH_BALL, SLOTS = S2D_MATCH_SLOTS;
  const float x = in.x, y = in.y, vx = in.vx, vy = in.vy, body = in.body;
  const int card = in.card;
  const bool is_player = l < NP;
  const bool active = l == BALL || (is_player && card < S2D_CARD_RED);
  const bool right = pa >= 11;
  const int ours = right ? SEE_SIDE_RIGHT : SEE_SIDE_LEFT;
  const float sg = right ? -1.0f : 1.0f;
  // the agent, in its team's frame
  const float ax = sg * sh.x[pa], ay = sg * sh.y[pa], avx = sg * sh.vx[pa], avy = sg * sh.vy[pa];
  const float abody = own_body(sh.body[pa], right), aneck = sh.neck[pa];
  const float face = norm_deg_any(abody + aneck);
  const int wi = width_index(sh.width[pa]);
  const bool fresh = sh.wait[pa] == interval_of(p, wi);
  const bool can_see = fresh && sh.card[pa] < S2D_CARD_RED;
  // this lane's object in that frame
  const float ox = sg * x, oy = sg * y, ovx = sg * vx, ovy = sg * vy, obody = own_body(body, right);
  const bool object = can_see && active && l != pa;    // something this agent could see in this cycle
  int level = 0;
  float dist = 0.0f, dir = 0.0f, dist_chg = 0.0f, dir_chg = 0.0f, body_rel = 0.0f;
  if (object) {                                        // (an agent who does not see costs none of the arithmetic below)
    const float dx = ox - ax, dy = oy - ay;
    const float d = hypot2(dx, dy);
    const bool here = d == 0.0f;
    const float rel = here ? 0.0f : norm_deg_any(atan2_deg(dy, dx) - face);
    const bool in_cone = fabsf(rel) <= 0.5f * view_angle_of(p, wi);
    const bool felt = d <= p.visible;
    if (in_cone) {
      level = 4;
      if (is_player) {
        const bool band = (d > p.unum_far && d < p.unum_too_far) || (d > p.team_far && d < p.team_too_far);
        float u1 = 0.0f, u2 = 0.0f;
        if (band) {
          const U4 w = philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), in.tick,
                                     ((uint32_t)S2D_MATCH_ST_SEE << 16) | (uint32_t)(pa * SLOTS + l), p.seed_lo, p.seed_hi);
          u1 = rnd_u01(w.x); u2 = rnd_u01(w.y);
        }
        if (d <= p.unum_far) level = 4;
        else if (d < p.unum_too_far && u1 >= (d - p.unum_far) * p.inv_unum_band) level = 4;
        else if (d <= p.team_far) level = 3;
        else if (d < p.team_too_far && u2 >= (d - p.team_far) * p.inv_team_band) level = 3;
        else level = 2;
      }
    } else if (felt) {
      level = 1;
    }
    if (level >= 1 && !here) {
      dist = quant(exp_spec(quant(log_spec(d), p.dist_q, p.inv_dist_q)), p.dist_r, p.inv_dist_r);
      dir = rintf(rel);
    }
    if (level == 4) {
      if (!here) {
        const float ex = dx / d, ey = dy / d, rvx = ovx - avx, rvy = ovy - avy;
        dist_chg = dist * quant(fmaf(rvx, ex, rvy * ey) / d, p.dchg_q, p.inv_dchg_q);
        dir_chg = quant((fmaf(rvy, ex, -(rvx * ey)) / d) * 57.29577951308232f, p.rchg_q, p.inv_rchg_q);
      }
      body_rel = rintf(norm_deg_any(obody - face));
    }
  }
  // the place of a player's row: seen ones ascending by (dir, dist, own-frame slot), then the unseen ones
  const bool seen = is_player && level >= 1;
  sh.key[l] = make_float2(dir, dist);
  const uint32_t seen_mask = see_hballot(seen, half) & 0x3FFFFFu;
  see_fence();
  int rank = 0;
  const int own_l = right ? (l < 11 ? l + 11 : l - 11) : l;   // the slot in the agent's frame: his team first
  if (seen) {
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const float2 kj = sh.key[j];
      const int own_j = right ? (j + 11) % NP : j;       // (a constant per side after unrolling)
      const bool before = kj.x < dir || (kj.x == dir && (kj.y < dist || (kj.y == dist && own_j < own_l)));
      rank += (((seen_mask >> j) & 1u) != 0u && before) ? 1 : 0;
    }
  } else {
    const uint32_t unseen = 0x3FFFFFu & ~seen_mask & ~(1u << pa);
    rank = __builtin_popcount(seen_mask) + __builtin_popcount(unseen & ((1u << l) - 1u));
  }
  if (is_player && l != pa) {
    const float team = level >= 3 ? ((l < 11) == !right ? 1.0f : -1.0f) : 0.0f;
    const float unum = level == 4 ? (float)(l % 11 + 1) : 0.0f;
    row[S2D_SEE_PLAYERS / 4 + 2 * rank] = make_float4((float)level, team, unum, dist);
    row[S2D_SEE_PLAYERS / 4 + 2 * rank + 1] = make_float4(dir, dist_chg, dir_chg, body_rel);
  } else if (l == pa) {
    row[0] = make_float4(ox, oy, ovx, ovy);
    row[1] = make_float4(obody, aneck, face, (float)(wi + 1));
    row[2] = make_float4(fresh ? 1.0f : 0.0f, (float)in.wait, in.stamina, in.effort);
    row[3] = make_float4(in.recovery, in.capacity, (l == S2D_MATCH_GOALIE_LEFT || l == S2D_MATCH_GOALIE_RIGHT) ? 1.0f : 0.0f, (float)card);
  } else if (l == BALL) {
    row[S2D_SEE_BALL / 4] = make_float4((float)level, dist, dir, dist_chg);
    row[S2D_SEE_BALL / 4 + 1] = make_float4(dir_chg, (float)in.mode, side_word(in.mode_side, ours), (float)in.cycle);
  }
  see_fence();
}

// The half-wave stores a row assembled in LDS (512 + 256 B): every 64-byte line written whole by one instruction.
S2D_DEV void see_row_store(float* __restrict__ dst, const float4* row, int l) {
  float4* d = reinterpret_cast<float4*>(dst);
  d[l] = row[l];
  if (l + kSeeHalf < kSeeVec) d[l + kSeeHalf] = row[l + kSeeHalf];
}

// One cycle of one player's vision state (s2d_match_vision_step, steps 1 to 4): done, sent off, the action (has_act: a moment and
// a ChangeView code were given), the timer.
S2D_DEV void vision_advance(const SeeParams& p, float& neck, int& width, int& wait, bool done, bool sent_off, bool has_act, float m_in,
                            float c) {
  if (done) {
    neck = 0.0f; width = 2; wait = 0;
  } else if (sent_off) {
    return;                                              // sent off: the state stands
  } else if (has_act) {
    const float m = m_in != m_in ? 0.0f : clampf(m_in, p.min_moment, p.max_moment);
    neck = clampf(norm_deg_any(neck + m), p.min_neck, p.max_neck);
    const int code = c == 1.0f ? 1 : (c == 2.0f ? 2 : (c == 3.0f ? 3 : 0));
    if (code != 0) {
      width = code;
      const int lim = interval_of(p, code - 1);
      wait = wait > lim ? lim : wait;                    // a pending wait never exceeds the new width's interval
    }
  }
  wait = wait > 1 ? wait - 1 : 0;
  if (wait == 0) wait = interval_of(p, width_index(width));
}

}  // namespace s2d_see
#endif  // S2D_SEE_ROW_H_
