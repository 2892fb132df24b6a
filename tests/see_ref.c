/* Host restatement of the vision layer (include/s2d_match.h, "Vision"; device: csrc/s2d_see.hip).  TEST INFRASTRUCTURE: compiled by
 * the tests with -ffp-contract=off and bound with ctypes.  atan2_deg / norm_deg / hypot2 / exp_r and the Philox block are those of
 * oracle/s2d_oracle_common.h, log_spec is restated here, so the result is comparable with the device bit for
 * bit.  Written from the header's words: one agent at a time, a list of what he sees, an explicit sort.
 *
 * What is independent of csrc/s2d_see.hip and what is not, for whoever maintains the pair:
 *   independent   the structure (a serial loop over agents and objects against one match per half-wave); the order of the player
 *                 rows (an insertion sort of a list against the device's counting of keys across lanes, and its treatment of the
 *                 unseen rows: never listed here, ranked behind the seen ones there); norm_deg, atan2_deg, hypot2, exp_r and the
 *                 Philox block (the oracle's C against s2d_device.h); log_spec (restated below from DESIGN.md section 4); the
 *                 vision_step timer (written as "decrement, floor at 0, reload" on the stored words).
 *   shared shape  the SeeParams layout with its pre-derived reciprocals mirrors the device struct on purpose (it is the form in
 *                 which the header states the parameters: "each rounded to fp32 once; inv(v) is the float of the double 1 / v",
 *                 a zero inv for an empty band), and the level cascade follows the header's sentence clause by clause, as the
 *                 device does: a misreading of the header there would be shared.  This file's band decisions are themselves held
 *                 against the header's linear probability by the statistics in test_match_see_host.py.
 *   derivation    S2DVisionParams -> SeeParams happens in Python here (tests/match_see.py: params), in see_params() on the device
 *                 side; the two meet only through the rows.  Non-default parameters (test_other_parameters on the GPU) are what
 *                 checks that derivation; with the defaults alone a wrong reciprocal could hide in both. */
#include "../oracle/s2d_oracle_common.h"
#include "../include/s2d_match.h"

#define NP S2D_MATCH_PLAYERS
#define BALL S2D_MATCH_BALL
enum { SIDE_NONE = 0, SIDE_LEFT = 1, SIDE_RIGHT = 2 };

/* S2DVisionParams as the layer rounds them (tests/match_see.py: params) and the engine's Philox words */
typedef struct {
  float view_angle[3]; int32_t interval[3];
  float visible, dist_q, inv_dist_q, dist_r, inv_dist_r, dchg_q, inv_dchg_q, rchg_q, inv_rchg_q;
  float unum_far, unum_too_far, inv_unum_band, team_far, team_too_far, inv_team_band;
  float min_moment, max_moment, min_neck, max_neck;
  uint64_t seed, env_id_offset;
} SeeParams;

/* what the layer reads: engine planes ([n][24]) and words ([n]), then the three vision planes */
typedef struct {
  const float *x, *y, *vx, *vy, *body, *stamina, *effort, *recovery, *stamina_capacity;
  const int32_t *card, *cycle, *mode, *mode_side, *tick;
  float *neck; int32_t *view_width, *see_wait;
} SeeState;

static float log_spec(float v) {
  int e;
  float m = frexpf(v, &e), x;
  if (m < 0.70710678118654752f) { e -= 1; x = (m + m) - 1.0f; } else { x = m - 1.0f; }
  const float z = x * x;
  float p = 7.0376836292e-2f;
  p = fmaf(p, x, -1.1514610310e-1f);
  p = fmaf(p, x, 1.1676998740e-1f);
  p = fmaf(p, x, -1.2420140846e-1f);
  p = fmaf(p, x, 1.4249322787e-1f);
  p = fmaf(p, x, -1.6668057665e-1f);
  p = fmaf(p, x, 2.0000714765e-1f);
  p = fmaf(p, x, -2.4999993993e-1f);
  p = fmaf(p, x, 3.3333331174e-1f);
  const float fe = (float)e;
  float y = (p * x) * z;
  y = fmaf(fe, -2.12194440e-4f, y);
  y = fmaf(-0.5f, z, y);
  return fmaf(fe, 0.693359375f, x + y);
}
static float quant(float v, float q, float inv_q) { return rintf(v * inv_q) * q; }
static int width_index(int code) { return code == S2D_VIEW_NARROW ? 0 : code == S2D_VIEW_WIDE ? 2 : 1; }
static float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
static float turned(float b) { return b > 0.0f ? b - 180.0f : b + 180.0f; }
static float see_dist(const SeeParams *P, float d) {
  return quant(exp_r(quant(log_spec(d), P->dist_q, P->inv_dist_q)), P->dist_r, P->inv_dist_r);
}

typedef struct { float w[8]; int slot; } Seen;   /* a seen player: his row and the last word of his order key */
static int before(const Seen *a, const Seen *b) {   /* (dir, dist, own-frame slot) ascending */
  if (a->w[4] != b->w[4]) return a->w[4] < b->w[4];
  if (a->w[3] != b->w[3]) return a->w[3] < b->w[3];
  return a->slot < b->slot;
}

static void see_row(const SeeParams *P, const SeeState *s, int64_t e, int p, float *o) {
  const int64_t k = e * S2D_MATCH_SLOTS;
  const int right = p >= 11, ours = right ? SIDE_RIGHT : SIDE_LEFT;
  const float sg = right ? -1.0f : 1.0f;
  memset(o, 0, sizeof(float) * S2D_SEE_DIM);
  const float xp = sg * s->x[k + p], yp = sg * s->y[k + p], vxp = sg * s->vx[k + p], vyp = sg * s->vy[k + p];
  const float bp = right ? turned(s->body[k + p]) : s->body[k + p];
  const float neck = s->neck[k + p];
  const float face = norm_deg(bp + neck);
  const int wi = width_index(s->view_width[k + p]);
  const int fresh = s->see_wait[k + p] == P->interval[wi];
  float *w = o + S2D_SEE_SELF;
  w[0] = xp; w[1] = yp; w[2] = vxp; w[3] = vyp; w[4] = bp; w[5] = neck; w[6] = face; w[7] = (float)(wi + 1);
  w[8] = fresh ? 1.0f : 0.0f; w[9] = (float)s->see_wait[k + p];
  w[10] = s->stamina[k + p]; w[11] = s->effort[k + p]; w[12] = s->recovery[k + p]; w[13] = s->stamina_capacity[k + p];
  w[14] = (p == S2D_MATCH_GOALIE_LEFT || p == S2D_MATCH_GOALIE_RIGHT) ? 1.0f : 0.0f; w[15] = (float)s->card[k + p];
  w = o + S2D_SEE_BALL;
  const int ms = s->mode_side[e];
  w[5] = (float)s->mode[e]; w[6] = ms == ours ? 1.0f : (ms == SIDE_NONE ? 0.0f : -1.0f); w[7] = (float)s->cycle[e];
  if (!fresh || s->card[k + p] >= S2D_CARD_RED) return;
  const float half_angle = 0.5f * P->view_angle[wi];
  Seen list[NP];
  int n_seen = 0;
  for (int j = 0; j <= BALL; ++j) {
    if (j == p) continue;
    if (j < NP && s->card[k + j] >= S2D_CARD_RED) continue;
    const float dx = sg * s->x[k + j] - xp, dy = sg * s->y[k + j] - yp;
    const float d = hypot2(dx, dy);
    const float rel = d == 0.0f ? 0.0f : norm_deg(atan2_deg(dy, dx) - face);
    int level;
    if (fabsf(rel) <= half_angle) {
      if (j == BALL || d <= P->unum_far) {
        level = 4;
      } else {
        uint32_t r[4] = {0, 0, 0, 0};
        if ((d > P->unum_far && d < P->unum_too_far) || (d > P->team_far && d < P->team_too_far))
          draw(P->seed, P->env_id_offset + (uint64_t)e, (uint32_t)s->tick[e], S2D_MATCH_ST_SEE, (uint32_t)(p * S2D_MATCH_SLOTS + j), r);
        const float u1 = rnd_u01(r[0]), u2 = rnd_u01(r[1]);
        if (d < P->unum_too_far && u1 >= (d - P->unum_far) * P->inv_unum_band) level = 4;
        else if (d <= P->team_far) level = 3;
        else if (d < P->team_too_far && u2 >= (d - P->team_far) * P->inv_team_band) level = 3;
        else level = 2;
      }
    } else if (d <= P->visible) {
      level = 1;
    } else {
      continue;                                              /* unseen */
    }
    const float dist = d == 0.0f ? 0.0f : see_dist(P, d), dir = d == 0.0f ? 0.0f : rintf(rel);
    float dist_chg = 0.0f, dir_chg = 0.0f;
    if (level == 4 && d != 0.0f) {
      const float ex = dx / d, ey = dy / d;
      const float rvx = sg * s->vx[k + j] - vxp, rvy = sg * s->vy[k + j] - vyp;
      dist_chg = dist * quant(fmaf(rvx, ex, rvy * ey) / d, P->dchg_q, P->inv_dchg_q);
      dir_chg = quant((fmaf(rvy, ex, -(rvx * ey)) / d) * 57.29577951308232f, P->rchg_q, P->inv_rchg_q);
    }
    if (j == BALL) {
      w[0] = (float)level; w[1] = dist; w[2] = dir; w[3] = dist_chg; w[4] = dir_chg;
      continue;
    }
    Seen *q = &list[n_seen++];
    memset(q, 0, sizeof *q);
    q->slot = right ? (j + 11) % NP : j;                     /* the slot in the agent's frame: his team first */
    q->w[0] = (float)level; q->w[3] = dist; q->w[4] = dir;
    if (level >= 3) q->w[1] = ((j >= 11) == right) ? 1.0f : -1.0f;
    if (level == 4) {
      const float bj = right ? turned(s->body[k + j]) : s->body[k + j];
      q->w[2] = (float)(j % 11 + 1); q->w[5] = dist_chg; q->w[6] = dir_chg; q->w[7] = rintf(norm_deg(bj - face));
    }
  }
  for (int a = 1; a < n_seen; ++a) {                         /* insertion sort, left to right across the view */
    const Seen t = list[a];
    int b = a;
    while (b > 0 && before(&t, &list[b - 1])) { list[b] = list[b - 1]; --b; }
    list[b] = t;
  }
  for (int a = 0; a < n_seen; ++a) memcpy(o + S2D_SEE_PLAYERS + S2D_SEE_ROW_WORDS * a, list[a].w, sizeof list[a].w);
}

/* n matches; mask = agents (bits 0..21); out [n][popcount(mask)][S2D_SEE_DIM] */
API void s2dsee_see(int64_t n, const SeeState *s, const SeeParams *P, uint32_t mask, float *out) {
  float *o = out;
  for (int64_t e = 0; e < n; ++e)
    for (int p = 0; p < NP; ++p)
      if ((mask >> p) & 1u) { see_row(P, s, e, p, o); o += S2D_SEE_DIM; }
}

/* one cycle of the vision state, in place; act [n][22][2] or NULL, done [n] or NULL */
API void s2dsee_vision_step(int64_t n, const SeeState *s, const SeeParams *P, const float *act, const uint8_t *done) {
  for (int64_t e = 0; e < n; ++e)
    for (int l = 0; l < NP; ++l) {
      const int64_t i = e * S2D_MATCH_SLOTS + l;
      if (done && done[e]) {
        s->neck[i] = 0.0f; s->view_width[i] = S2D_VIEW_NORMAL; s->see_wait[i] = 0;
      } else {
        if (s->card[i] >= S2D_CARD_RED) continue;
        if (act) {
          float m = act[(e * NP + l) * 2];
          const float c = act[(e * NP + l) * 2 + 1];
          m = isnan(m) ? 0.0f : clampf(m, P->min_moment, P->max_moment);
          s->neck[i] = clampf(norm_deg(s->neck[i] + m), P->min_neck, P->max_neck);
          if (c == 1.0f || c == 2.0f || c == 3.0f) {
            s->view_width[i] = (int32_t)c;
            if (s->see_wait[i] > P->interval[(int)c - 1]) s->see_wait[i] = P->interval[(int)c - 1];
          }
        }
      }
      int wait = s->see_wait[i] - 1;
      if (wait < 0) wait = 0;
      if (wait == 0) wait = P->interval[width_index(s->view_width[i])];
      s->see_wait[i] = wait;
    }
}

/* the distance grid alone (tests of the quantisation) */
API void s2dsee_dist(int64_t n, const SeeParams *P, const float *d, float *out) {
  for (int64_t i = 0; i < n; ++i) out[i] = see_dist(P, d[i]);
}
