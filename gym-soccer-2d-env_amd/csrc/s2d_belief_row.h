// s2d_belief_row.h -- one update of one agent's belief row (include/s2d_match.h, "Belief") as a device function.
// The BELIEF instantiations of the cycle kernel execute it (s2d_match_slots.h: the see row built in the cycle, the row loaded into
// the network's tile and stored back).  s2d_match_belief_scan_kernel (s2d_belief.hip) holds the same update, statement for
// statement, inside its own loop and does not call this function: called from there the function compiled to another order of the
// same instructions and four more VGPRs, and measured 0.6 to 2 % slower than that kernel may become ("Belief network").
// WHOEVER CHANGES ONE CHANGES THE OTHER: a belief row recorded by the cycle kernel must be bitwise the row the scan kernel writes
// for the same see rows and flags, and tests/test_gpu_match_belief_net.py compares them so.
//
// Mapping (the scan kernel's): ONE AGENT PER HALF-WAVE, lane = entry (0 the ball, 1..21 the player rows; lanes 22..25 copy the self
// words).  Per update:
//   - every lane ages its own entry (steps 1, 2);
//   - lane = SIGHTING: the 21 player rows and the ball are located in parallel (one sincos each) into an LDS tile;
//   - first pass: every entry looks for the last level-4 row that names it (22 broadcast reads);
//   - second pass: sequential over the level 1-3 rows (a ballot names them), a half-wave minimum over the candidates' distances
//     (four DPP rounds and one row swap) and a ballot for the lowest row at that distance;
//   - ghosts per entry; the row is written in place.
// Both halves of a wave may run different agents: every cross-lane step stays inside the half (DPP rows of 16, one swap of lane ^ 16,
// ballots shifted by the half), and the branches that are uniform within a half-wave may differ between the halves.
#ifndef S2D_BELIEF_ROW_H_
#define S2D_BELIEF_ROW_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "s2d_device.h"
#include "../../include/s2d_match.h"

namespace s2d_belief {

constexpr int kHalf = 32;
constexpr int kVec = S2D_BELIEF_DIM / 4;                 // 48 float4 per row
constexpr int kEntries = 22;                             // the ball and 21 player rows
constexpr int kSightings = 22;                           // 21 player rows of the see row, then its ball
static_assert(S2D_BELIEF_DIM == S2D_SEE_DIM && S2D_BELIEF_BALL == S2D_SEE_BALL && S2D_BELIEF_PLAYERS == S2D_SEE_PLAYERS &&
              S2D_BELIEF_ROW_WORDS == 8 && S2D_SEE_ROW_WORDS == 8, "a belief row is laid out over a see row");
static_assert(kVec > kHalf && kVec <= 2 * kHalf, "a half-wave moves a row as two float4 per lane");

// S2DBeliefParams rounded once (double -> float)
struct BeliefParams { float ball_decay, player_decay, view_angle[3], match_dist, match_rate, ghost_margin, count_max; };

inline BeliefParams belief_params(const S2DBeliefParams& v) {
  BeliefParams p;
  p.ball_decay = (float)v.ball_decay; p.player_decay = (float)v.player_decay;
  for (int i = 0; i < 3; ++i) p.view_angle[i] = (float)v.view_angle[i];
  p.match_dist = (float)v.match_dist; p.match_rate = (float)v.match_rate; p.ghost_margin = (float)v.ghost_margin;
  p.count_max = (float)v.count_max;
  return p;
}

struct BeliefScratch {                                   // one agent (half-wave), live inside one update only
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

// One update of the belief row `row` (LDS, 48 float4, updated in place) with the see row `see` (LDS, 48 float4): steps 1 to 5 of
// "Belief".  l = the lane within the half-wave, u = the agent's own index (raw slot % 11), do_reset = the reset flag of its match
// (uniform within the half-wave).  Called by every lane of the half-wave, after a fence that made `row` and `see` whole; ends
// with a fence: the row is whole.
// (The parameters are passed by value: through a reference to a kernel argument the selects below -- a decay by the lane's entry,
// a view angle by the row's code -- become per-lane loads from a selected address, two vector loads from memory per update.)
S2D_DEV void belief_update(const BeliefParams p, float4* row, const float4* see, BeliefScratch& sc, int l, int half, int u,
                           bool do_reset) {
  const bool is_entry = l < kEntries;
  const bool is_ball = l == 0;
  const int rv = is_ball ? S2D_BELIEF_BALL / 4 : S2D_BELIEF_PLAYERS / 4 + 2 * (l - 1);   // this entry's two float4 of the row
  const int sv = l < 21 ? S2D_SEE_PLAYERS / 4 + 2 * l : S2D_SEE_BALL / 4;                // this sighting's two float4 of the see row
  const float cm = p.count_max;

  // this lane's entry, steps 1 and 2
  Entry en{};
  bool updated = false;
  if (is_entry) {
    const float4 w0 = row[rv], w1 = row[rv + 1];
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

  const float4 self0 = see[0], self1 = see[1];
  const float sx = self0.x, sy = self0.y, svx = self0.z, svy = self0.w, face = self1.z, code = self1.w;
  const bool can = see[2].x == 1.0f && see[3].w < (float)S2D_CARD_RED;   // uniform within the half-wave
  if (can) {
    uint32_t pending;                                  // the level 1-3 rows of the see row, one bit each
    // lane = sighting: locate it
    {
      float level = 0.0f, team = 0.0f, unum = 0.0f, dist = 0.0f, dir = 0.0f, dchg = 0.0f, rchg = 0.0f, brel = 0.0f;
      if (l < kSightings) {
        const float4 a0 = see[sv], a1 = see[sv + 1];
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
      sc.fix[l] = make_float4(X, Y, VX, VY);
      sc.body[l] = norm_deg_any(brel + face);
      sc.target[l] = target;
      pending = half_ballot(l < 21 && (level == 1.0f || level == 2.0f || level == 3.0f), half);
    }
    half_fence();
    // first pass: lane = entry again; the last sighting that names it
    if (is_entry) {
      int hit = -1;
#pragma unroll
      for (int q = 0; q < kSightings; ++q) hit = sc.target[q] == l ? q : hit;
      if (hit >= 0) {
        const float4 f = sc.fix[hit];
        en.x = f.x; en.y = f.y; en.pos_count = 0.0f;
        updated = true;
        if (!is_ball) {
          en.vx = f.z; en.vy = f.w; en.body = sc.body[hit]; en.vel_count = 0.0f; en.body_count = 0.0f;
        } else if (see[S2D_SEE_BALL / 4].x == 4.0f) {
          en.vx = f.z; en.vy = f.w;
        }
      }
    }
    // second pass: the level 1-3 rows, one after the other
#pragma unroll 1
    while (pending != 0u) {                            // (uniform within the half-wave)
      const int q = __builtin_ctz(pending);
      pending &= pending - 1u;
      const float4 a0 = see[S2D_SEE_PLAYERS / 4 + 2 * q];
      const float team = a0.y, dist = a0.w;
      const float4 f = sc.fix[q];
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
    row[rv] = make_float4(en.x, en.y, en.vx, en.vy);
    if (is_ball) {
      const float4 g = see[S2D_SEE_BALL / 4 + 1];
      row[rv + 1] = make_float4(en.pos_count, g.y, g.z, g.w);
    } else {
      row[rv + 1] = make_float4(en.body, en.pos_count, en.vel_count, en.body_count);
    }
  } else if (l < kEntries + 4) {
    row[l - kEntries] = see[l - kEntries];             // lanes 22..25: the four float4 of the self words
  }
  half_fence();
}

}  // namespace s2d_belief
#endif  // S2D_BELIEF_ROW_H_
