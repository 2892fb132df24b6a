/* Host restatement of the agent reward (include/s2d_match.h, "Agent reward"; device: m_agent_reward in s2d_match_slots.h).
 * TEST INFRASTRUCTURE: compiled by the tests with -ffp-contract=off and bound with ctypes.  Written from the header's table: the
 * row words come from the rows of tests/agent_obs_ref.c (row(S), row(S')), everything else from the two states' planes. */
#include "../oracle/s2d_oracle_common.h"
#include "../include/s2d_match.h"

#define NP S2D_MATCH_PLAYERS
#define BALL S2D_MATCH_BALL
#define DIM S2D_AGENT_OBS_DIM
enum { W_BALL_X = S2D_AGENT_OBS_BALL + 0, W_BALL_DIST = S2D_AGENT_OBS_BALL + 4, W_BALL_BEARING = S2D_AGENT_OBS_BALL + 5,
       W_LAST_TOUCH = S2D_AGENT_OBS_BALL + 6, W_KICKABLE = S2D_AGENT_OBS_SELF + 12 };

/* what the reward reads of a state beside its rows: planes [n][24], words [n] */
typedef struct { const float *x, *y; const int32_t *card, *mode; } RewardState;

/* the scripted team's rule-5 chaser of the team whose first slot is t0: nearest non-goalie to the ball by sq2, ties to the lower
 * index, sent-off players excluded; -1: the team has none */
static int chaser(const RewardState *s, int64_t e, int t0) {
  const int64_t k = e * S2D_MATCH_SLOTS;
  const float bx = s->x[k + BALL], by = s->y[k + BALL];
  int best = -1; float bd = 0.0f;
  for (int j = t0 + 1; j < t0 + 11; ++j) {                  /* (slot t0 is the goalie) */
    if (s->card[k + j] >= S2D_CARD_RED) continue;
    const float d2 = sq2(bx - s->x[k + j], by - s->y[k + j]);
    if (best < 0 || d2 < bd) { best = j; bd = d2; }
  }
  return best;
}

/* rows0 / rows1: [n][22][224] of S / S'; reward_left1: [n] of S'; w: the six weights.
 * out [n][22]; terms (or NULL) [n][22][6]: the six terms before weighting. */
API void s2dar_agent_reward(int64_t n, const float *rows0, const float *rows1, const RewardState *s0, const RewardState *s1,
                            const float *reward_left1, const float *w, int chaser_only, float *out, float *terms) {
  for (int64_t e = 0; e < n; ++e) {
    const int live = s0->mode[e] == S2D_GM_PLAY_ON && s1->mode[e] == S2D_GM_PLAY_ON, play1 = s1->mode[e] == S2D_GM_PLAY_ON;
    const int ch[2] = {chaser(s0, e, 0), chaser(s0, e, 11)};
    for (int l = 0; l < NP; ++l) {
      const float *r0 = rows0 + (e * NP + l) * DIM, *r1 = rows1 + (e * NP + l) * DIM;
      const float sgn = l < 11 ? 1.0f : -1.0f;
      const int64_t k = e * S2D_MATCH_SLOTS + l;
      const int active = s0->card[k] < S2D_CARD_RED && s1->card[k] < S2D_CARD_RED;
      const int gate = active && (chaser_only ? ch[l >= 11] == l : 1);
      float t[S2D_MATCH_REWARD_TERMS];
      t[0] = sgn * reward_left1[e];
      t[1] = live ? r1[W_BALL_X] - r0[W_BALL_X] : 0.0f;
      t[2] = (live && gate) ? r0[W_BALL_DIST] - r1[W_BALL_DIST] : 0.0f;
      t[3] = (live && gate) ? (fabsf(r0[W_BALL_BEARING]) - fabsf(r1[W_BALL_BEARING])) * (float)(1.0 / 180.0) : 0.0f;
      t[4] = (play1 && active) ? r1[W_KICKABLE] : 0.0f;
      t[5] = play1 ? r1[W_LAST_TOUCH] : 0.0f;
      float acc = 0.0f;
      for (int i = 0; i < S2D_MATCH_REWARD_TERMS; ++i) acc = fmaf(w[i], t[i], acc);
      out[e * NP + l] = acc;
      if (terms) memcpy(terms + (e * NP + l) * S2D_MATCH_REWARD_TERMS, t, sizeof t);
    }
  }
}
