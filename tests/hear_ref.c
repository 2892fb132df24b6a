/* Host restatement of the audio layer (include/s2d_match.h, "Hearing"; device: csrc/s2d_hear.hip).  TEST INFRASTRUCTURE: compiled by
 * the tests with -ffp-contract=off and bound with ctypes.  atan2_deg / norm_deg / hypot2 and the Philox block are those of
 * oracle/s2d_oracle_common.h, so the result is comparable with the device bit for bit.  Written from the header's words: one listener
 * at a time, a list of the candidates of each side in own-frame order, a draw for every one of them, an explicit search for the
 * smallest key.
 *
 * What is independent of csrc/s2d_hear.hip and what is not:
 *   independent   the structure (a serial loop over listeners and a list per side against one match per half-wave and bit masks);
 *                 the own-frame slots (every speaker is mapped into the listener's frame and compared there; the device stays on
 *                 raw slots and argues that the order is the same); the draw (made for every candidate, also for a lone one or beside
 *                 an attended one, where the device makes none); the payload (quantised per listener from the say row, per speaker
 *                 on the device); the math functions and the Philox block (the oracle's C against s2d_device.h).
 *   shared shape  HearParams with half / inv_half pre-derived (tests/match_hear.py: params) is the form in which the header states
 *                 them; non-default say_levels in the GPU tests check the derivation. */
#include "../oracle/s2d_oracle_common.h"
#include "../include/s2d_match.h"

#define NP S2D_MATCH_PLAYERS
#define REC S2D_HEAR_RECORD

typedef struct {
  float cut, half, inv_half;
  int32_t hear_max, hear_inc, hear_decay, msg_size;
  uint64_t seed, env_id_offset;
} HearParams;

/* what the layer reads of the engine ([n][24] planes, tick [n]), the neck plane or NULL, then the four hear planes */
typedef struct {
  const float *x, *y, *body;
  const int32_t *card, *tick;
  const float *neck;
  int32_t *cap_our, *cap_opp, *attention;
  float *hear;
} HearState;

static float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
static float turned(float b) { return b > 0.0f ? b - 180.0f : b + 180.0f; }
/* own-frame slot <-> raw slot for a listener of the given team */
static int own_of(int raw, int right) { return right ? (raw + 11) % NP : raw; }
static int raw_of(int own, int right) { return right ? (own + 11) % NP : own; }

static void reset_row(float *row, int hear_max) {
  for (int i = 0; i < S2D_HEAR_DIM; ++i) row[i] = 0.0f;
  row[4] = (float)hear_max;
  row[REC + 4] = (float)hear_max;
}

typedef struct { int own, raw; uint32_t u; float dx, dy, d; } Cand;

static void listener(const HearParams *P, const HearState *s, const float *say, int64_t e, int p) {
  const int64_t k = e * S2D_MATCH_SLOTS;
  float *row = s->hear + (e * NP + p) * S2D_HEAR_DIM;
  for (int i = 0; i < S2D_HEAR_DIM; ++i) row[i] = 0.0f;
  if (s->card[k + p] >= S2D_CARD_RED) return;                       /* 2. sent off: planes kept, the row +0 */
  const int right = p >= 11;
  const float sg = right ? -1.0f : 1.0f;
  /* 3. attention */
  int att = s->attention[k + p];
  if (att < -1 || att > 21) att = -1;
  if (say) {
    const float c = say[(e * NP + p) * S2D_SAY_ROW + 1];
    if (c == -1.0f) att = -1;
    else if (c >= 1.0f && c <= 22.0f && c == floorf(c) && (int)c - 1 != own_of(p, right)) att = (int)c - 1;
  }
  /* 4. capacities: [0] ours, [1] theirs */
  int cap[2] = {s->cap_our[k + p], s->cap_opp[k + p]};
  for (int side = 0; side < 2; ++side) {
    if (cap[side] < 0 || cap[side] > P->hear_max) cap[side] = P->hear_max;
    cap[side] += P->hear_inc;
    if (cap[side] > P->hear_max) cap[side] = P->hear_max;
  }
  const float xp = sg * s->x[k + p], yp = sg * s->y[k + p];
  const float bp = right ? turned(s->body[k + p]) : s->body[k + p];
  const float face = norm_deg(bp + (s->neck ? s->neck[k + p] : 0.0f));
  for (int side = 0; side < 2; ++side) {
    /* 5. the side's candidates, in own-frame order */
    Cand list[11];
    int count = 0;
    for (int own = side * 11; say && own < side * 11 + 11; ++own) {
      const int j = raw_of(own, right);
      if (j == p || s->card[k + j] >= S2D_CARD_RED) continue;
      const float said = say[(e * NP + j) * S2D_SAY_ROW];
      if (said == 0.0f || isnan(said)) continue;
      Cand c;
      c.own = own; c.raw = j;
      c.dx = sg * s->x[k + j] - xp; c.dy = sg * s->y[k + j] - yp;
      c.d = hypot2(c.dx, c.dy);
      if (!(c.d <= P->cut)) continue;
      uint32_t w[4];
      draw(P->seed, P->env_id_offset + (uint64_t)e, (uint32_t)s->tick[e], S2D_MATCH_ST_HEAR, (uint32_t)(p * S2D_MATCH_SLOTS + j), w);
      c.u = w[0] >> 8;
      list[count++] = c;
    }
    float *r = row + side * REC;
    /* 6. */
    if (cap[side] >= P->hear_decay && count > 0) {
      int win = -1;
      for (int a = 0; a < count; ++a) if (list[a].own == att) win = a;
      if (win < 0) {
        win = 0;
        for (int a = 1; a < count; ++a)
          if (list[a].u < list[win].u || (list[a].u == list[win].u && list[a].own < list[win].own)) win = a;
      }
      const Cand *c = &list[win];
      cap[side] -= P->hear_decay;
      r[0] = 1.0f;
      r[1] = side == 0 ? (float)(c->own + 1) : 0.0f;
      r[2] = c->d == 0.0f ? 0.0f : rintf(norm_deg(atan2_deg(c->dy, c->dx) - face));
      r[3] = (float)(count - 1);
      const float *v = say + (e * NP + c->raw) * S2D_SAY_ROW + 2;
      for (int i = 0; i < P->msg_size; ++i) r[6 + i] = isnan(v[i]) ? 0.0f : rintf(clampf(v[i], -1.0f, 1.0f) * P->half) * P->inv_half;
    } else {
      r[3] = (float)count;
    }
    /* 7. */
    r[4] = (float)cap[side];
  }
  row[5] = (float)(att + 1);
  s->cap_our[k + p] = cap[0]; s->cap_opp[k + p] = cap[1]; s->attention[k + p] = att;
}

/* one cycle, in place; say [n][22][12] or NULL, done [n] or NULL */
API void s2dhear_step(int64_t n, const HearState *s, const HearParams *P, const float *say, const uint8_t *done) {
  for (int64_t e = 0; e < n; ++e)
    for (int p = 0; p < NP; ++p) {
      if (done && done[e]) {                                         /* 1. the reset state */
        const int64_t i = e * S2D_MATCH_SLOTS + p;
        s->cap_our[i] = P->hear_max; s->cap_opp[i] = P->hear_max; s->attention[i] = -1;
        reset_row(s->hear + (e * NP + p) * S2D_HEAR_DIM, P->hear_max);
      } else {
        listener(P, s, say, e, p);
      }
    }
}

/* the masked matches (mask NULL = all): all 24 slots of the three planes, the 22 rows */
API void s2dhear_reset(int64_t n, const HearState *s, const HearParams *P, const uint8_t *mask) {
  for (int64_t e = 0; e < n; ++e) {
    if (mask && !mask[e]) continue;
    for (int l = 0; l < S2D_MATCH_SLOTS; ++l) {
      const int64_t i = e * S2D_MATCH_SLOTS + l;
      s->cap_our[i] = P->hear_max; s->cap_opp[i] = P->hear_max; s->attention[i] = -1;
    }
    for (int p = 0; p < NP; ++p) reset_row(s->hear + (e * NP + p) * S2D_HEAR_DIM, P->hear_max);
  }
}

/* the draw alone: u of (tick, p, j) for match id gid */
API uint32_t s2dhear_draw(const HearParams *P, uint64_t e, uint32_t tick, int p, int j) {
  uint32_t w[4];
  draw(P->seed, P->env_id_offset + e, tick, S2D_MATCH_ST_HEAR, (uint32_t)(p * S2D_MATCH_SLOTS + j), w);
  return w[0] >> 8;
}
