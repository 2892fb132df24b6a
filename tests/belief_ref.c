/* Host restatement of the belief layer (include/s2d_match.h, "Belief"; device: csrc/s2d_belief.hip).  TEST INFRASTRUCTURE: compiled
 * by the tests with -ffp-contract=off and bound with ctypes.  sincos_deg / atan2_deg / norm_deg / hypot2 / sq2 are those of
 * oracle/s2d_oracle_common.h, so the result is comparable with the device bit for bit.  Written from the header's words: one agent
 * at a time, its row unpacked into a list of entries, the five steps one after the other, the row packed again.
 *
 * What is independent of csrc/s2d_belief.hip: the structure (a serial loop over agents, entries and sightings against one agent
 * per half-wave with a lane per entry); the association (a plain scan for the minimum against the device's cross-lane reduction);
 * the first pass (sightings in row order writing their entry, against the device's entries looking for their last sighting); the
 * elementary functions (the oracle's C against s2d_device.h).  Shared on purpose: the BeliefParams layout, the form in which the
 * header states the parameters (each rounded to fp32 once; tests/belief.py derives them here, belief_params() there). */
#include "../oracle/s2d_oracle_common.h"
#include "../include/s2d_match.h"

#define N_ENT 22   /* entry 0 = the ball, entry 1 + j = player row j */

typedef struct {
  float ball_decay, player_decay, view_angle[3], match_dist, match_rate, ghost_margin, count_max;
} BeliefParams;

typedef struct {
  float x, y, vx, vy, body, pos_count, vel_count, body_count;   /* the ball uses x .. vy and pos_count only */
  int updated;
} Entry;

static void forget(Entry *e, float count_max) {
  e->x = e->y = e->vx = e->vy = e->body = 0.0f;
  e->pos_count = e->vel_count = e->body_count = count_max;
}
static float older(float c, float count_max) { return c + 1.0f < count_max ? c + 1.0f : count_max; }

typedef struct { float X, Y, VX, VY; } Fix;
static Fix locate(const float *S, float level, float dist, float dir, float dist_chg, float dir_chg) {
  const float face = S[S2D_SEE_SELF + 6];
  Fix f;
  float s, c;
  sincos_deg(norm_deg(face + dir), &s, &c);
  f.X = fmaf(dist, c, S[0]);
  f.Y = fmaf(dist, s, S[1]);
  f.VX = f.VY = 0.0f;
  if (level == 4.0f) {
    if (dist != 0.0f) {
      const float vr = dist_chg, vt = (dir_chg * 0.017453292519943295f) * dist;
      f.VX = fmaf(vr, c, -(vt * s)) + S[2];
      f.VY = fmaf(vr, s, vt * c) + S[3];
    } else {
      f.VX = S[2]; f.VY = S[3];
    }
  }
  return f;
}

/* one update of one row: B in place, S the see row, u the agent's own index, reset the match's flag */
static void update(const BeliefParams *P, float *B, const float *S, int u, int reset) {
  Entry en[N_ENT];
  const float cm = P->count_max;
  /* unpack */
  memset(en, 0, sizeof en);
  en[0].x = B[16]; en[0].y = B[17]; en[0].vx = B[18]; en[0].vy = B[19]; en[0].pos_count = B[20];
  en[0].vel_count = en[0].body_count = cm;                  /* (words the ball does not have) */
  for (int j = 0; j < 21; ++j) {
    const float *w = B + S2D_BELIEF_PLAYERS + S2D_BELIEF_ROW_WORDS * j;
    Entry *e = &en[1 + j];
    e->x = w[0]; e->y = w[1]; e->vx = w[2]; e->vy = w[3]; e->body = w[4]; e->pos_count = w[5]; e->vel_count = w[6]; e->body_count = w[7];
  }
  /* 1. reset */
  if (reset) for (int i = 0; i < N_ENT; ++i) forget(&en[i], cm);
  /* 2. predict */
  for (int i = 0; i < N_ENT; ++i) {
    Entry *e = &en[i];
    if (e->pos_count < cm) {
      const float decay = i == 0 ? P->ball_decay : P->player_decay;
      e->x = e->x + e->vx; e->y = e->y + e->vy;
      e->vx = e->vx * decay; e->vy = e->vy * decay;
    }
    e->pos_count = older(e->pos_count, cm); e->vel_count = older(e->vel_count, cm); e->body_count = older(e->body_count, cm);
    if (e->pos_count == cm) forget(e, cm);
  }
  /* 3. copy */
  memcpy(B, S, sizeof(float) * 16);
  memcpy(B + 21, S + 21, sizeof(float) * 3);
  /* 4. correct, 5. ghosts */
  if (S[8] == 1.0f && S[15] < (float)S2D_CARD_RED) {
    const float face = S[6];
    const float *sb = S + S2D_SEE_BALL;
    if (sb[0] >= 1.0f) {
      const Fix f = locate(S, sb[0], sb[1], sb[2], sb[3], sb[4]);
      en[0].x = f.X; en[0].y = f.Y; en[0].pos_count = 0.0f; en[0].updated = 1;
      if (sb[0] == 4.0f) { en[0].vx = f.VX; en[0].vy = f.VY; }
    }
    for (int r = 0; r < 21; ++r) {                           /* first pass: the identified players */
      const float *w = S + S2D_SEE_PLAYERS + S2D_SEE_ROW_WORDS * r;
      if (w[0] != 4.0f) continue;
      const float team = w[1], unum = w[2];
      if (!(unum >= 1.0f && unum <= 11.0f) || unum != rintf(unum)) continue;
      const int n = (int)unum;
      int j;
      if (team > 0.0f) {
        if (n - 1 == u) continue;
        j = n - 1 < u ? n - 1 : n - 2;
      } else if (team < 0.0f) {
        j = n + 9;
      } else {
        continue;
      }
      const Fix f = locate(S, 4.0f, w[3], w[4], w[5], w[6]);
      Entry *e = &en[1 + j];
      e->x = f.X; e->y = f.Y; e->vx = f.VX; e->vy = f.VY; e->body = norm_deg(w[7] + face);
      e->pos_count = e->vel_count = e->body_count = 0.0f;
      e->updated = 1;
    }
    for (int r = 0; r < 21; ++r) {                           /* second pass: the others, by nearest neighbour */
      const float *w = S + S2D_SEE_PLAYERS + S2D_SEE_ROW_WORDS * r;
      if (!(w[0] == 1.0f || w[0] == 2.0f || w[0] == 3.0f)) continue;
      const Fix f = locate(S, w[0], w[3], w[4], 0.0f, 0.0f);
      const float tol = fmaf(P->match_rate, w[3], P->match_dist), tol2 = tol * tol;
      const int lo = w[1] < 0.0f ? 10 : 0, hi = w[1] > 0.0f ? 10 : 21;
      int best = -1;
      float best_q = 0.0f;
      for (int j = lo; j < hi; ++j) {
        const Entry *e = &en[1 + j];
        if (e->updated || !(e->pos_count < cm)) continue;
        const float q = sq2(f.X - e->x, f.Y - e->y);
        if (!(q <= tol2)) continue;
        if (best < 0 || q < best_q) { best = j; best_q = q; }
      }
      if (best >= 0) {
        Entry *e = &en[1 + best];
        e->x = f.X; e->y = f.Y; e->pos_count = 0.0f; e->updated = 1;
      }
    }
    const float code = S[7];
    const int wi = code == 1.0f ? 0 : code == 3.0f ? 2 : 1;
    const float cone = 0.5f * P->view_angle[wi] - P->ghost_margin;
    for (int i = 0; i < N_ENT; ++i) {
      Entry *e = &en[i];
      if (e->updated || !(e->pos_count < cm)) continue;
      const float dx = e->x - S[0], dy = e->y - S[1];
      const float d = hypot2(dx, dy);
      if (d > 0.0f && fabsf(norm_deg(atan2_deg(dy, dx) - face)) <= cone) forget(e, cm);
    }
  }
  /* pack */
  B[16] = en[0].x; B[17] = en[0].y; B[18] = en[0].vx; B[19] = en[0].vy; B[20] = en[0].pos_count;
  for (int j = 0; j < 21; ++j) {
    float *w = B + S2D_BELIEF_PLAYERS + S2D_BELIEF_ROW_WORDS * j;
    const Entry *e = &en[1 + j];
    w[0] = e->x; w[1] = e->y; w[2] = e->vx; w[3] = e->vy; w[4] = e->body; w[5] = e->pos_count; w[6] = e->vel_count; w[7] = e->body_count;
  }
}

/* see [T][n][k][192], reset [T][n] or NULL, belief [n][k][192] in place, out [T][n][k][192] or NULL; mask = the k slots */
API void s2dbel_scan(const BeliefParams *P, const float *see, const uint8_t *reset, float *belief, float *out, int T, int64_t n,
                     uint32_t mask) {
  int slots[S2D_MATCH_PLAYERS], k = 0;
  for (int p = 0; p < S2D_MATCH_PLAYERS; ++p) if ((mask >> p) & 1u) slots[k++] = p;
  for (int t = 0; t < T; ++t)
    for (int64_t e = 0; e < n; ++e)
      for (int r = 0; r < k; ++r) {
        const int64_t row = (e * k + r) * S2D_BELIEF_DIM, at = ((int64_t)t * n * k) * S2D_BELIEF_DIM + row;
        update(P, belief + row, see + at, slots[r] % 11, reset ? reset[(int64_t)t * n + e] : 0);
        if (out) memcpy(out + at, belief + row, sizeof(float) * S2D_BELIEF_DIM);
      }
}

/* the rows s2d_match_belief_reset leaves in the masked matches */
API void s2dbel_reset(float *belief, int64_t n, int k, const uint8_t *mask) {
  for (int64_t e = 0; e < n; ++e) {
    if (mask && !mask[e]) continue;
    for (int r = 0; r < k; ++r) {
      float *B = belief + (e * k + r) * S2D_BELIEF_DIM;
      memset(B, 0, sizeof(float) * S2D_BELIEF_DIM);
      B[20] = S2D_BELIEF_COUNT_LIMIT;
      for (int j = 0; j < 21; ++j) B[24 + 8 * j + 5] = B[24 + 8 * j + 6] = B[24 + 8 * j + 7] = S2D_BELIEF_COUNT_LIMIT;
    }
  }
}
