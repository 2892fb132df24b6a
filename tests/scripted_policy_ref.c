/* Host restatement of the scripted team (include/s2d_match.h, rules 1-8; device: m_scripted_action in s2d_match_rules.h).
 * TEST INFRASTRUCTURE: compiled by the tests with -ffp-contract=off and bound with ctypes.  atan2_deg / norm_deg / sq2 are the
 * fp32 spec functions of oracle/s2d_oracle_common.h, so the result is comparable with the device bit for bit. */
#include "../oracle/s2d_oracle_common.h"
#include "../include/s2d_match.h"

/* the kick-off formation of the engine (left team; the right team mirrors x) */
static const float kFormX[11] = {-50.0f, -35.0f, -35.0f, -35.0f, -35.0f, -20.0f, -20.0f, -20.0f, -20.0f, -10.5f, -10.5f};
static const float kFormY[11] = {0.0f, -20.0f, -7.0f, 7.0f, 20.0f, -22.0f, -8.0f, 8.0f, 22.0f, -6.0f, 6.0f};

enum { SIDE_LEFT = 1, SIDE_RIGHT = 2 };
#define BIT(m) (1u << (m))
static const uint32_t kHalted = BIT(S2D_GM_TIME_OVER) | BIT(S2D_GM_PAUSE) | BIT(S2D_GM_HUMAN);
static const uint32_t kPenalty = BIT(S2D_GM_PENALTY_SETUP) | BIT(S2D_GM_PENALTY_READY) | BIT(S2D_GM_PENALTY_TAKEN) |
                                 BIT(S2D_GM_PENALTY_MISS) | BIT(S2D_GM_PENALTY_SCORE) | BIT(S2D_GM_PENALTY_ONFIELD) | BIT(S2D_GM_PENALTY_FOUL);
static const uint32_t kDead = BIT(S2D_GM_OFF_SIDE) | BIT(S2D_GM_BACK_PASS) | BIT(S2D_GM_FREE_KICK_FAULT) | BIT(S2D_GM_CATCH_FAULT) |
                              BIT(S2D_GM_FOUL_CHARGE) | BIT(S2D_GM_ILLEGAL_DEFENSE) | BIT(S2D_GM_FOUL_PUSH) |
                              BIT(S2D_GM_FOUL_MULTIPLE_ATTACKER) | BIT(S2D_GM_FOUL_BALL_OUT) | BIT(S2D_GM_AFTER_GOAL) |
                              BIT(S2D_GM_BEFORE_KICK_OFF) | BIT(S2D_GM_FIRST_HALF_OVER) | BIT(S2D_GM_EXTEND_HALF) |
                              BIT(S2D_GM_GOALIE_CATCH) | (kPenalty & ~(BIT(S2D_GM_PENALTY_READY) | BIT(S2D_GM_PENALTY_TAKEN)));
static int in_modes(int mode, uint32_t mask) { return (mask >> (mode & 31)) & 1u; }
static float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

static void turn_or_dash(float ang, float *o) {
  if (fabsf(ang) > S2D_SCRIPT_TURN_TOL) { o[0] = S2D_MCMD_TURN; o[1] = ang; }
  else { o[0] = S2D_MCMD_DASH; o[1] = S2D_SCRIPT_DASH_POWER; }
  o[2] = 0.0f;
}

/* fp = {half_l, half_w, max_power, pen_x, pen_half_w, max_catch_angle, min_catch_angle}: the engine's fp32 parameters */
static void one_match(const float *x, const float *y, const float *body, const int32_t *tackle, const int32_t *catch_ban,
                      const int32_t *card, int mode, int mside, int last_touch, int holder, int taker_word,
                      const float *ka2, const float *catch_len, const float *fp, float *out) {
  const float half_l = fp[0], half_w = fp[1], max_power = fp[2], pen_x = fp[3], pen_half_w = fp[4];
  const float max_catch = fp[5], min_catch = fp[6];
  const float bx = x[S2D_MATCH_BALL], by = y[S2D_MATCH_BALL];
  float d2[S2D_MATCH_PLAYERS];
  int chaser[2] = {-1, -1};
  for (int l = 0; l < S2D_MATCH_PLAYERS; ++l) d2[l] = sq2(bx - x[l], by - y[l]);
  for (int l = 0; l < S2D_MATCH_PLAYERS; ++l) {          /* index order: ties go to the lower index */
    if (l == S2D_MATCH_GOALIE_LEFT || l == S2D_MATCH_GOALIE_RIGHT || card[l] >= S2D_CARD_RED) continue;
    const int t = l < 11 ? 0 : 1;
    if (chaser[t] < 0 || d2[l] < d2[chaser[t]]) chaser[t] = l;
  }
  for (int l = 0; l < S2D_MATCH_PLAYERS; ++l) {
    float *o = out + 3 * l;
    o[0] = S2D_MCMD_NONE; o[1] = 0.0f; o[2] = 0.0f;
    const int side = l < 11 ? SIDE_LEFT : SIDE_RIGHT, other = l < 11 ? SIDE_RIGHT : SIDE_LEFT;
    if (in_modes(mode, kHalted) || in_modes(mode, kDead) || tackle[l] > 0 || card[l] >= S2D_CARD_RED) continue;   /* 1 */
    const int pen = in_modes(mode, kPenalty);
    const int goalie = l == S2D_MATCH_GOALIE_LEFT || l == S2D_MATCH_GOALIE_RIGHT;
    const int taker = pen && l == (taker_word & 0xff) - 1;
    const int keeper = mode == S2D_GM_PENALTY_TAKEN && l == (mside == SIDE_LEFT ? S2D_MATCH_GOALIE_RIGHT : S2D_MATCH_GOALIE_LEFT);
    if (pen && !taker && !keeper) continue;                                                                       /* 8 */
    const float att = pen ? 1.0f : (side == SIDE_LEFT ? 1.0f : -1.0f);
    const float def = pen ? 1.0f : -att;
    const float ang_ball = norm_deg(atan2_deg(by - y[l], bx - x[l]) - body[l]);
    const float shot = norm_deg(atan2_deg(0.0f - y[l], att * half_l - x[l]) - body[l]);
    if (mode == S2D_GM_FREE_KICK && holder == l + 1) { o[0] = S2D_MCMD_KICK; o[1] = max_power; o[2] = shot; continue; }   /* 2 */
    if (goalie && (mode == S2D_GM_PLAY_ON || keeper) && catch_ban[l] == 0 && last_touch == other) {                        /* 3 */
      const float cl = catch_len[l];
      if (d2[l] <= cl * cl && ang_ball <= max_catch && ang_ball >= min_catch && fabsf(by) <= pen_half_w && def * bx >= pen_x) {
        o[0] = S2D_MCMD_CATCH; o[1] = ang_ball; continue;
      }
    }
    const int may_play = pen ? taker : (mode == S2D_GM_PLAY_ON || mside == side);
    if (may_play && d2[l] <= ka2[l]) { o[0] = S2D_MCMD_KICK; o[1] = max_power; o[2] = shot; continue; }             /* 4 */
    if (may_play && (taker || chaser[side == SIDE_LEFT ? 0 : 1] == l)) { turn_or_dash(ang_ball, o); continue; }     /* 5 */
    float tx, ty;
    if (goalie) { tx = def * S2D_SCRIPT_GOALIE_X; ty = clampf(by * S2D_SCRIPT_GOALIE_Y_GAIN, -S2D_SCRIPT_GOALIE_Y_MAX, S2D_SCRIPT_GOALIE_Y_MAX); }
    else {
      const int k = l % 11;
      tx = clampf(att * kFormX[k] + S2D_SCRIPT_HOME_GAIN_X * bx, -half_l, half_l);
      ty = clampf(kFormY[k] + S2D_SCRIPT_HOME_GAIN_Y * by, -half_w, half_w);
    }
    const float dx = tx - x[l], dy = ty - y[l];
    if (sq2(dx, dy) <= S2D_SCRIPT_ARRIVE * S2D_SCRIPT_ARRIVE) {                                                      /* 6, 7 */
      if (fabsf(ang_ball) > S2D_SCRIPT_TURN_TOL) { o[0] = S2D_MCMD_TURN; o[1] = ang_ball; }
      continue;
    }
    turn_or_dash(norm_deg(atan2_deg(dy, dx) - body[l]), o);
  }
}

/* n matches in the engine's layout: x / y / body / tackle / catch_ban / card [n][24] (slot 22 = the ball), mode / mode_side /
 * last_touch_side / ball_holder / set_play_taker [n]; ka2 / catch_len [22] per slot; out [n][22][3] */
API void s2dsp_actions(int64_t n, const float *x, const float *y, const float *body, const int32_t *tackle, const int32_t *catch_ban,
                       const int32_t *card, const int32_t *mode, const int32_t *mode_side, const int32_t *last_touch,
                       const int32_t *holder, const int32_t *taker, const float *ka2, const float *catch_len, const float *fp,
                       float *out) {
  for (int64_t e = 0; e < n; ++e) {
    const int64_t k = e * S2D_MATCH_SLOTS;
    one_match(x + k, y + k, body + k, tackle + k, catch_ban + k, card + k, mode[e], mode_side[e], last_touch[e], holder[e], taker[e],
              ka2, catch_len, fp, out + e * S2D_MATCH_PLAYERS * 3);
  }
}
