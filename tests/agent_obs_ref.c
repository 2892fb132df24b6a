/* Host restatement of the per-agent observations (include/s2d_match.h, "Per-agent observations"; device:
 * s2d_match_agent_obs_kernel in s2d_match.hip).  TEST INFRASTRUCTURE: compiled by the tests with -ffp-contract=off and bound with
 * ctypes.  atan2_deg / norm_deg / sq2 / hypot2 are the fp32 spec functions of oracle/s2d_oracle_common.h, so the result is
 * comparable with the device bit for bit.  Written from the header's words, one agent at a time, without the kernel's sharing. */
#include "../oracle/s2d_oracle_common.h"
#include "../include/s2d_match.h"

#define NP S2D_MATCH_PLAYERS
#define BALL S2D_MATCH_BALL
enum { SIDE_NONE = 0, SIDE_LEFT = 1, SIDE_RIGHT = 2 };

/* per-slot words, as the engine derives them from its configuration */
typedef struct {
  float ka[NP], ka2[NP], speed_max[NP], kick_rate[NP], inv_margin[NP], size[NP], type_id[NP];
  float ball_size, ball_decay;
  int32_t half_time_cycles, nr_extra_halfs, extra_half_cycles, total_cycles;
} AgentParams;

/* the state planes ([n][24]) and words ([n]) of S2DMatchBuffers the observation reads */
typedef struct {
  const float *x, *y, *vx, *vy, *body, *stamina, *effort, *recovery, *stamina_capacity;
  const int32_t *tackle_cycles, *catch_ban, *card;
  const int32_t *cycle, *mode, *mode_side, *score_left, *score_right, *last_touch_side, *ball_holder, *stopped_cycle;
} AgentState;

static int cycles_to_half(int cycle, int h) { const int rem = cycle % h; return rem < 0 ? -rem : h - rem; }
static int cycles_to_period_end(const AgentParams *P, int cycle) {
  if (P->nr_extra_halfs > 0 && cycle >= P->total_cycles) return cycles_to_half(cycle - P->total_cycles, P->extra_half_cycles);
  return cycles_to_half(cycle, P->half_time_cycles);
}
static int side_of(int i) { return i < 11 ? SIDE_LEFT : SIDE_RIGHT; }
static float side_word(int side, int ours) { return side == ours ? 1.0f : (side == SIDE_NONE ? 0.0f : -1.0f); }
static int in_set(int mode, const int *set, int n) { for (int i = 0; i < n; ++i) if (mode == set[i]) return 1; return 0; }
static const int kPenalty[] = {S2D_GM_PENALTY_SETUP, S2D_GM_PENALTY_READY, S2D_GM_PENALTY_TAKEN, S2D_GM_PENALTY_MISS,
                               S2D_GM_PENALTY_SCORE, S2D_GM_PENALTY_ONFIELD, S2D_GM_PENALTY_FOUL};
static const int kSetPlay[] = {S2D_GM_KICK_OFF, S2D_GM_KICK_IN, S2D_GM_FREE_KICK, S2D_GM_CORNER_KICK, S2D_GM_GOAL_KICK,
                               S2D_GM_IND_FREE_KICK, S2D_GM_GOALIE_CATCH, S2D_GM_PENALTY_KICK};

/* one match (pointers at its first slot / word), agent p -> 224 words */
static void agent_row(const AgentParams *P, const AgentState *s, int64_t e, int p, float *o) {
  const int64_t k = e * S2D_MATCH_SLOTS;
  const int right = p >= 11, ours = right ? SIDE_RIGHT : SIDE_LEFT;
  const float sg = right ? -1.0f : 1.0f;
  float X[BALL + 1], Y[BALL + 1], VX[BALL + 1], VY[BALL + 1], B[NP];
  int active[NP], reach[NP], kick[NP];
  for (int j = 0; j <= BALL; ++j) {                         /* the own frame */
    X[j] = sg * s->x[k + j]; Y[j] = sg * s->y[k + j]; VX[j] = sg * s->vx[k + j]; VY[j] = sg * s->vy[k + j];
    if (j < NP) { const float b = s->body[k + j]; B[j] = right ? (b > 0.0f ? b - 180.0f : b + 180.0f) : b; }
  }
  const float bx = X[BALL], by = Y[BALL];
  for (int j = 0; j < NP; ++j) {
    active[j] = s->card[k + j] < S2D_CARD_RED;
    const float d2 = sq2(bx - X[j], by - Y[j]);
    kick[j] = active[j] && d2 <= P->ka2[j];
    reach[j] = S2D_AGENT_REACH_NONE;
    if (!active[j]) continue;
    if (d2 <= P->ka2[j]) { reach[j] = 0; continue; }
    float cx = bx, cy = by, cvx = VX[BALL], cvy = VY[BALL];
    for (int t = 1; t <= S2D_AGENT_REACH_MAX; ++t) {
      cx = cx + cvx; cy = cy + cvy; cvx = cvx * P->ball_decay; cvy = cvy * P->ball_decay;
      const float r = P->ka[j] + (float)t * P->speed_max[j];
      if (sq2(cx - X[j], cy - Y[j]) <= r * r) { reach[j] = t; break; }
    }
  }
  memset(o, 0, sizeof(float) * S2D_AGENT_OBS_DIM);
  /* self */
  float *w = o + S2D_AGENT_OBS_SELF;
  const float bdx = bx - X[p], bdy = by - Y[p];
  const float bdist = hypot2(bdx, bdy), bbear = norm_deg(atan2_deg(bdy, bdx) - B[p]);
  w[0] = X[p]; w[1] = Y[p]; w[2] = VX[p]; w[3] = VY[p]; w[4] = B[p];
  w[5] = s->stamina[k + p]; w[6] = s->effort[k + p]; w[7] = s->recovery[k + p]; w[8] = s->stamina_capacity[k + p];
  w[9] = (p == S2D_MATCH_GOALIE_LEFT || p == S2D_MATCH_GOALIE_RIGHT) ? 1.0f : 0.0f;
  w[10] = (float)s->tackle_cycles[k + p]; w[11] = (float)s->card[k + p];
  w[12] = kick[p] ? 1.0f : 0.0f;
  if (kick[p]) {
    const float dir_diff = fabsf(bbear), dist_ball = sqrtf(sq2(bdx, bdy)) - P->size[p] - P->ball_size;
    w[13] = P->kick_rate[p] * (1.0f - 0.25f * (dir_diff * 0.005555555555555556f) - 0.25f * (dist_ball * P->inv_margin[p]));
  }
  w[14] = (float)s->catch_ban[k + p]; w[15] = P->type_id[p];
  /* ball */
  w = o + S2D_AGENT_OBS_BALL;
  w[0] = bx; w[1] = by; w[2] = VX[BALL]; w[3] = VY[BALL]; w[4] = bdist; w[5] = bbear;
  w[6] = side_word(s->last_touch_side[e], ours);
  w[7] = side_word(s->ball_holder[e] > 0 ? side_of(s->ball_holder[e] - 1) : SIDE_NONE, ours);
  /* game */
  w = o + S2D_AGENT_OBS_GAME;
  const int mode = s->mode[e], us = right ? 11 : 0, them = right ? 0 : 11;
  w[0] = (float)mode; w[1] = side_word(s->mode_side[e], ours);
  w[2] = (float)(right ? s->score_right[e] : s->score_left[e]); w[3] = (float)(right ? s->score_left[e] : s->score_right[e]);
  w[4] = (float)s->cycle[e]; w[5] = (float)s->stopped_cycle[e]; w[6] = (float)cycles_to_period_end(P, s->cycle[e]);
  w[7] = in_set(mode, kPenalty, 7) ? 1.0f : 0.0f;
  float first = -1.0e9f, second = -1.0e9f;                   /* the offside rule's scan: all 11 opponents */
  for (int j = them; j < them + 11; ++j) {
    const float v = X[j];
    if (v > first) { second = first; first = v; } else if (v > second) second = v;
  }
  float line = 0.0f;
  if (second > line) line = second;
  if (bx > line) line = bx;
  float mn = bx, mx = bx;
  for (int j = 1; j < 11; ++j) {
    if (active[us + j] && X[us + j] < mn) mn = X[us + j];
    if (active[them + j] && X[them + j] > mx) mx = X[them + j];
  }
  w[8] = line; w[9] = mn; w[10] = mx;
  for (int j = us; j < us + 11; ++j) if (j != p && kick[j]) { w[11] = (float)(j - us + 1); break; }
  for (int j = them; j < them + 11; ++j) if (kick[j]) { w[12] = (float)(j - them + 1); break; }
  w[13] = (float)reach[p];
  for (int team = 0; team < 2; ++team) {                    /* two smallest (reach, slot) keys, scanned in slot order */
    const int t0 = team == 0 ? us : them;
    int b1 = -1, b2 = -1;
    for (int j = t0; j < t0 + 11; ++j) {
      if (!active[j] || (team == 0 && j == p)) continue;
      if (b1 < 0 || reach[j] < reach[b1]) { b2 = b1; b1 = j; } else if (b2 < 0 || reach[j] < reach[b2]) b2 = j;
    }
    float *q = w + (team == 0 ? 14 : 18);
    q[0] = b1 >= 0 ? (float)reach[b1] : (float)S2D_AGENT_REACH_NONE; q[1] = b1 >= 0 ? (float)(b1 - t0 + 1) : 0.0f;
    q[2] = b2 >= 0 ? (float)reach[b2] : (float)S2D_AGENT_REACH_NONE; q[3] = b2 >= 0 ? (float)(b2 - t0 + 1) : 0.0f;
  }
  const int sp = in_set(mode, kSetPlay, 8);
  w[22] = (sp && s->mode_side[e] == ours) ? 1.0f : 0.0f;
  w[23] = (sp && s->mode_side[e] != ours && s->mode_side[e] != SIDE_NONE) ? 1.0f : 0.0f;
  /* teammates, opponents */
  for (int j = 0; j < NP; ++j) {
    float *r = o + (side_of(j) == ours ? S2D_AGENT_OBS_TEAMMATES : S2D_AGENT_OBS_OPPONENTS) + S2D_AGENT_OBS_ROW_WORDS * (j % 11);
    r[7] = (float)reach[j];
    if (!active[j]) continue;
    const float dx = X[j] - X[p], dy = Y[j] - Y[p];
    r[0] = X[j]; r[1] = Y[j]; r[2] = VX[j]; r[3] = VY[j]; r[4] = B[j];
    r[5] = j == p ? 0.0f : hypot2(dx, dy);
    r[6] = j == p ? 0.0f : norm_deg(atan2_deg(dy, dx) - B[p]);
  }
}

/* n matches; mask = agents (bits 0..21); out [n][popcount(mask)][S2D_AGENT_OBS_DIM] */
API void s2dao_agent_obs(int64_t n, const AgentState *s, const AgentParams *P, uint32_t mask, float *out) {
  float *o = out;
  for (int64_t e = 0; e < n; ++e)
    for (int p = 0; p < NP; ++p)
      if ((mask >> p) & 1u) { agent_row(P, s, e, p, o); o += S2D_AGENT_OBS_DIM; }
}
