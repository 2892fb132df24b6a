/*
 * s2d_match.h -- C ABI of the 11v11 full-match engine (BASELINE.json
 * configs[3]: 22 players, kick / tackle / catch / offside / stamina, heterogeneous player
 * types, thousands of lockstep matches).
 * Same library (libs2d_hip.so), same conventions as s2d.h: plain C, device pointers,
 * hipStream_t as void*, stream-ordered asynchronous launches, 0 / negative error codes.
 *
 * What it replaces in the reference: the rcssserver match itself behind Soccer2DEnv
 * (soccer_2d_env.py:356-383 starts it; every State read at server.py:49-103 comes from it).
 * The reference holds NO Python for an 11v11 task; the boundary mirrored here is therefore the
 * protobuf schema: commands = PlayerAction {Dash, Turn, Kick, Tackle} (idl/service.proto:380-402),
 * observations = WorldModel {ball, teammates[11], opponents[11], game_mode_type, scores, cycle}
 * (idl/service.proto:144-175, 306-349), play modes = GameModeType (267-301).
 * All match rules are rcssserver's (EXT): parity-unpinned.
 */
#ifndef S2D_MATCH_H_
#define S2D_MATCH_H_

#include "s2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define S2D_MATCH_PLAYERS 22      /* 0..10 left team (attacks +x), 11..21 right team */
#define S2D_MATCH_SLOTS 24        /* per-env object slots in memory: 22 players, slot 22 = ball, 23 = pad */
#define S2D_MATCH_BALL 22
#define S2D_MATCH_OBJ_WORDS 5     /* observation row of one object: x, y, vx, vy, body */

#define S2D_MATCH_PLAYER_TYPES 18 /* PlayerParam.player_types, idl/service.proto:1666 */
#define S2D_MATCH_GOALIE_LEFT 0   /* the goalie is the first player of each team */
#define S2D_MATCH_GOALIE_RIGHT 11

/* body commands = the PlayerAction oneof members 1..6 (idl/service.proto:380-411, 1291-1298).  TurnNeck and
 * ChangeView (:413-419) are no body commands: they steer the opt-in vision layer below ("Vision": s2d_match_vision_step
 * takes them as a row of their own); in an action row of the body step send S2D_MCMD_NONE. */
enum { S2D_MCMD_NONE = 0, S2D_MCMD_DASH = 1, S2D_MCMD_TURN = 2, S2D_MCMD_KICK = 3, S2D_MCMD_TACKLE = 4,
       S2D_MCMD_CATCH = 5, S2D_MCMD_MOVE = 6 };
/* GameModeType values used (idl/service.proto:267-301).  mode_side: for the restarts (KickOff_, KickIn_, FreeKick_, CornerKick_,
 * GoalKick_, IndFreeKick_, GoalieCatch_, PenaltyKick_ -- a FoulCharge_ called inside the offender's own penalty area, restarted from
 * that half's penalty spot) the side that takes it; for the ANNOUNCEMENTS (AfterGoal_, OffSide_, BackPass_,
 * FreeKickFault_, CatchFault_, FoulCharge_: rcssserver's goal_l, offside_l, back_pass_l, ...) the side the call is named after --
 * the scorer, the offender.  An announcement is a dead ball with the clock stopped; after announce_wait (after_goal_wait) cycles
 * the referee turns it into the restart for the other side.  FirstHalfOver / ExtendHalf: one stopped cycle at the end of a half /
 * of a drawn normal time (side = who kicks off next).  The shoot-out's modes: side = the team of the current taker
 * (PenaltyOnfield_: the half the kicks are taken in). */
enum {
  S2D_GM_BEFORE_KICK_OFF = 0, S2D_GM_TIME_OVER = 1, S2D_GM_PLAY_ON = 2, S2D_GM_KICK_OFF = 3, S2D_GM_KICK_IN = 4,
  S2D_GM_FREE_KICK = 5, S2D_GM_CORNER_KICK = 6, S2D_GM_GOAL_KICK = 7, S2D_GM_AFTER_GOAL = 8, S2D_GM_OFF_SIDE = 9,
  S2D_GM_PENALTY_KICK = 10, S2D_GM_FIRST_HALF_OVER = 11, S2D_GM_FOUL_CHARGE = 14, S2D_GM_BACK_PASS = 18, S2D_GM_FREE_KICK_FAULT = 19,
  S2D_GM_CATCH_FAULT = 20, S2D_GM_IND_FREE_KICK = 21, S2D_GM_GOALIE_CATCH = 30, S2D_GM_EXTEND_HALF = 31,
  /* the penalty shoot-out after a drawn extra time (idl/service.proto:290-297).  PenaltyFoul_: the kicker played the ball a second
   * time although pen_allow_mult_kicks is off -- the kick counts as missed (the defending goalie cannot infringe: he stands still
   * until the kick) */
  S2D_GM_PENALTY_SETUP = 22, S2D_GM_PENALTY_READY = 23, S2D_GM_PENALTY_TAKEN = 24, S2D_GM_PENALTY_MISS = 25,
  S2D_GM_PENALTY_SCORE = 26, S2D_GM_PENALTY_ONFIELD = 28, S2D_GM_PENALTY_FOUL = 29,
  S2D_GM_FOUL_PUSH = 15, S2D_GM_FOUL_MULTIPLE_ATTACKER = 16, S2D_GM_FOUL_BALL_OUT = 17,   /* announcements the engine's own referee never
                                             makes (rcssserver defines them and calls only FoulCharge_): written into the mode plane with the
                                             offending side they are played like one -- dead ball, then a FreeKick_ for the other side */
  S2D_GM_PAUSE = 12, S2D_GM_HUMAN = 13,   /* never entered by the engine: an operator writes them into the mode plane to HOLD a match
                                             (nobody acts, nothing is decided, the clock stands) and another mode to let it go on */
  S2D_GM_ILLEGAL_DEFENSE = 27   /* an announcement like OffSide_: named after the offending side (see illegal_defense_number) */
};
/* During the shoot-out the set-play word (S2DMatchBuffers.set_play_taker) carries its state -- PenaltyKickState of the proto
 * (idl/service.proto:130-138): bits 0-7 = 1 + index of the current taker, 12-15 / 16-19 = kicks taken by the left / right team,
 * 20-23 / 24-27 = their shoot-out goals; the mode side is the current taker's team. */
#define S2D_PEN_TAKER(w) (((w) & 0xff) - 1)
#define S2D_PEN_KICKS_LEFT(w) (((w) >> 12) & 15)
#define S2D_PEN_KICKS_RIGHT(w) (((w) >> 16) & 15)
#define S2D_PEN_SCORE_LEFT(w) (((w) >> 20) & 15)
#define S2D_PEN_SCORE_RIGHT(w) (((w) >> 24) & 15)
/* cards (rcssserver's yellow_card / red_card referee messages; no field of the proto's Player carries them) */
enum { S2D_CARD_NONE = 0, S2D_CARD_YELLOW = 1, S2D_CARD_RED = 2 /* sent off: parked beside the pitch, commands ignored */ };

/* ServerParam fields the match needs beyond S2DServerParams (same names as idl/service.proto:
 * 1435-1662); defaults = rcssserver stock values. */
typedef struct S2DMatchParams {
  double kick_power_rate, kickable_margin, kick_rand, max_power, min_power;        /* .027 .7 .1 100 -100 */
  double tackle_dist, tackle_back_dist, tackle_width, tackle_power_rate;           /* 2 0 1.25 .027 */
  double max_tackle_power, max_back_tackle_power;                                  /* 100 0 */
  double goal_width, offside_active_area_size, free_kick_distance;                 /* 14.02 2.5 9.15 */
  int32_t tackle_cycles, half_time_cycles, nr_normal_halfs, drop_ball_time;        /* 10 3000 2 100 */
  int32_t use_offside, catch_ban_cycle;                                            /* 1 5 */
  /* goalie catch (idl/service.proto:1488-1490, 1643-1644); the catch rectangle is catchable_area_l *
   * PlayerType.catchable_area_l_stretch long, catch_area_w wide, rooted at the goalie */
  double catchable_area_l, catch_area_w, catch_probability, max_catch_angle, min_catch_angle;  /* 1.2 1 1 90 -90 */
  double penalty_area_length, penalty_area_half_width;                             /* 16.5 20.16 */
  int32_t goalie_max_moves;               /* 2: Move commands a goalie may issue while he holds a caught ball */
  int32_t after_goal_wait;                /* 50: cycles of AfterGoal_ (mode side = the scorer) between a goal and the
                                             kick-off formation; 0 = kick-off at once */
  int32_t kick_off_wait;                  /* 0: cycles of BeforeKickOff (idl/service.proto:268) before the kick-off of each
                                             half -- nobody may play the ball, players may Move inside their own half
                                             (rcssserver's auto_mode waits kick_off_wait = 100); 0 = KickOff_ at once */
  int32_t back_passes;                    /* 1: a goalie catching a ball a team-mate kicked concedes an indirect free kick
                                             (BackPass_, idl/service.proto:286; ServerParam.back_passes :1579) */
  int32_t free_kick_faults;               /* 1: the taker of a set play may not play the ball twice in a row
                                             (FreeKickFault_, :287; ServerParam.free_kick_faults :1578) */
  int32_t stopped_clock;                  /* 1: the clock (WorldModel.cycle) stands still in BeforeKickOff, AfterGoal_, the
                                             announcements, FirstHalfOver and TimeOver; WorldModel.stoped_cycle (:333) counts those
                                             cycles.  0 = the round-1/2 behaviour: time runs in every mode */
  int32_t announce_wait;                  /* 30: cycles an announcement (OffSide_, BackPass_, FreeKickFault_, CatchFault_,
                                             FoulCharge_) lasts before the restart it awards (rcssserver's AFTER_*_WAIT) */
  int32_t foul_cycles;                    /* 5: cycles a fouled player stays down (ServerParam.foul_cycles, :1633) */
  int32_t nr_extra_halfs;                 /* 2: extra halves played when the normal time ends in a draw (ServerParam.nr_extra_halfs,
                                             idl/service.proto:1601): one stopped cycle of ExtendHalf (:299, rcssserver's
                                             "time_extended"), then a kick-off; 0 = the match ends with the normal time */
  double foul_detect_probability;         /* .5: chance that the referee sees an intentional foul (:1632) */
  int32_t extra_half_cycles;              /* 1000: length of an extra half (ServerParam.extra_half_time :1622, 100 s of 10 cycles);
                                             FirstHalfOver between extra halves; after the last one a draw goes to the shoot-out below */
  int32_t golden_goal;                    /* 0: a goal in extra time ends the match at once (ServerParam.golden_goal :1635) */
  /* The penalty shoot-out (ServerParam.penalty_shoot_outs, pen_*: idl/service.proto:1602-1613) after a draw that the last period
   * leaves: PenaltyOnfield_ (side = the half the kicks are taken in: the right one) for pen_before_setup_wait cycles; then per
   * kick PenaltySetup_ (one cycle: the ball on the spot pen_dist_x from the right goal line, the taker behind it, the other team's
   * goalie on the line, everybody else inside the centre circle, all placed by the referee = pen_coach_moves_players), PenaltyReady_
   * (the taker has pen_ready_wait cycles to play the ball), PenaltyTaken_ (taker against goalie, at most pen_taken_wait cycles:
   * ball in the goal = PenaltyScore_; out, caught or out of time = PenaltyMiss_; a second touch with pen_allow_mult_kicks off =
   * PenaltyFoul_), the verdict for pen_before_setup_wait cycles.
   * The left team kicks first, takers from index 10 downwards; pen_nr_kicks each (decided early when one side cannot catch up),
   * then pairs of kicks until one pair decides or pen_max_extra_kicks more are used up (then the draw stands, unless pen_random_winner
   * below tosses a coin).  The clock stands throughout. */
  int32_t penalty_shoot_outs;             /* 1 */
  int32_t pen_before_setup_wait, pen_ready_wait, pen_taken_wait;   /* 10 10 150 */
  int32_t pen_nr_kicks, pen_max_extra_kicks;                       /* 5 5 (their sum <= 15) */
  double pen_dist_x;                      /* 42.5 */
  /* IllegalDefense_ (idl/service.proto:295; ServerParam.illegal_defense_number / _duration / _dist_x / _width :1637-1640; OFF in the
   * stock server: number = 0).  While the ball is in play and the OTHER team was the last to play it, a team that keeps at least
   * `number` players inside the strip of dist_x in front of its own goal line, width wide, for `duration` cycles on end is called:
   * IllegalDefense_ named after it, the ball on that half's penalty spot, after announce_wait a FreeKick_ for the other team.
   * (In PlayOn the two counters live in setplay_timer, bits 0-7 left / 8-15 right: the word is otherwise unused there.) */
  int32_t illegal_defense_number, illegal_defense_duration;   /* 0 20 (duration <= 255) */
  double illegal_defense_dist_x, illegal_defense_width;       /* 16.5 40.32 */
  int32_t pen_allow_mult_kicks;           /* 1 (ServerParam.pen_allow_mult_kicks, idl/service.proto:1611): the taker may play the ball
                                             again during PenaltyTaken_; 0 = a second touch of his is PenaltyFoul_, the kick is missed */
  int32_t pen_random_winner;              /* 0 (ServerParam.pen_random_winner, idl/service.proto:1610): a shoot-out that ends level is decided
                                             by a coin (one Philox draw in the cycle the match ends): bits 28-29 of the set-play word =
                                             1 left / 2 right won the toss; the score is not touched.  (The field took the place of
                                             reserved_mp2: the struct's size and every other offset are unchanged.) */
} S2DMatchParams;

/* PlayerType (idl/service.proto:1697-1732): the members that enter the dynamics.  Type 0 is the
 * default type (= the ServerParam / S2DMatchParams values). */
typedef struct S2DPlayerType {
  double player_speed_max, stamina_inc_max, player_decay, inertia_moment, dash_power_rate, player_size;
  double kickable_margin, kick_rand, extra_stamina, effort_max, effort_min, kick_power_rate;
  double catchable_area_l_stretch;
} S2DPlayerType;

/* PlayerParam (idl/service.proto:1664-1695): the ranges rcssserver draws its heterogeneous types
 * from (stock values in s2d_match_default_player_params). */
typedef struct S2DPlayerParams {
  double player_speed_max_delta_min, player_speed_max_delta_max, stamina_inc_max_delta_factor;
  double player_decay_delta_min, player_decay_delta_max, inertia_moment_delta_factor;
  double dash_power_rate_delta_min, dash_power_rate_delta_max, player_size_delta_factor;
  double kickable_margin_delta_min, kickable_margin_delta_max, kick_rand_delta_factor;
  double extra_stamina_delta_min, extra_stamina_delta_max, effort_max_delta_factor, effort_min_delta_factor;
  double new_dash_power_rate_delta_min, new_dash_power_rate_delta_max, new_stamina_inc_max_delta_factor;
  double kick_power_rate_delta_min, kick_power_rate_delta_max;
  double catchable_area_l_stretch_min, catchable_area_l_stretch_max;
} S2DPlayerParams;

typedef struct S2DMatchConfig {
  uint32_t abi_version;   /* S2D_ABI_VERSION */
  uint32_t struct_bytes;  /* sizeof(S2DMatchConfig) */
  S2DServerParams sp;
  S2DMatchParams mp;
  uint64_t seed;
  int64_t env_id_offset;
  int32_t auto_reset;     /* 1: a finished match (TimeOver) restarts inside the same step */
  int32_t noise;          /* 0: player_rand/ball_rand/kick_rand off; tackle success is always drawn */
  int32_t reserved[4];
  /* heterogeneous players: the type table and the type of every player slot (DoChangePlayerType,
   * idl/service.proto:1393-1433).  s2d_match_default_config: 18 copies of the default type, all ids 0. */
  S2DPlayerType player_types[S2D_MATCH_PLAYER_TYPES];
  int32_t player_type_id[S2D_MATCH_SLOTS];   /* [0..21]; the goalies (0, 11) keep type 0 in rcssserver */
} S2DMatchConfig;

/* Device buffers.  Per-object planes are [N][24] (slot = lane of the env's half-wave);
 * per-env arrays are [N]. */
typedef struct S2DMatchBuffers {
  int64_t n_envs;
  float *x, *y, *vx, *vy, *body;                      /* players + ball (ball: body unused) */
  float *stamina, *effort, *recovery, *stamina_capacity;
  int32_t *tackle_cycles;                             /* >0: player frozen after a tackle */
  int32_t *catch_ban;                                 /* >0: goalie may not catch (catch_ban_cycle after every attempt) */
  int32_t *cycle, *mode, *mode_side, *score_left, *score_right;
  int32_t *last_touch_side, *setplay_timer, *offside_mask;     /* bit i = player i flagged */
  int32_t *ball_holder, *goalie_moves;  /* 1 + index of the goalie holding a caught ball (0 = nobody), his remaining moves */
  int32_t *set_play_taker, *last_kicker;   /* 1 + index (0 = nobody): who put the ball into play from the last set play and has
                                            not been followed by another touch; who last moved it with a Kick command */
  int32_t *stopped_cycle;  /* [N] WorldModel.stoped_cycle (idl/service.proto:333): cycles the clock has been standing still */
  int32_t *tick;           /* [N] simulator cycles since s2d_match_reset, stopped ones included: the Philox counter of every draw */
  int32_t *card;           /* [N][24] S2D_CARD_* per player */
  float *reward_left;      /* [N] +1 left goal, -1 right goal this cycle */
  uint8_t *done;           /* [N] 1 when the match reached TimeOver this cycle */
  int32_t *nearest_left, *nearest_right;              /* [N] index of the player closest to the ball, per team */
  unsigned long long *stats;  /* [S2D_STATS_STRIPES][8], sum over stripes: [0] env-steps [1] goals left
                                 [2] goals right [3] matches finished [4] kicks + catches [5] tackles
                                 [6] offsides [7] ball-outs */
} S2DMatchBuffers;

typedef struct S2DMatchRollout {
  float *obs;        /* [T][N][24][5] x,y,vx,vy,body after each cycle (slot 22 = ball) or NULL; 16-byte aligned */
  float *reward;     /* [T][N] or NULL */
  int32_t *mode;     /* [T][N] or NULL */
  uint8_t *done;     /* [T][N] or NULL */
} S2DMatchRollout;

typedef struct S2DMatchEngine *S2DMatchHandle;

void s2d_match_default_config(S2DMatchConfig *cfg);
void s2d_match_default_player_params(S2DPlayerParams *pp);
/* Fill cfg->player_types[1..17] the way rcssserver's HeteroPlayer does (trade-off pairs drawn from
 * the PlayerParam ranges; EXT), deterministically from `seed` (Philox).
 * pp == NULL: stock ranges.  Type 0 stays the default type; player_type_id is not touched. */
int s2d_match_generate_player_types(S2DMatchConfig *cfg, const S2DPlayerParams *pp, uint64_t seed);
int s2d_match_validate_config(const S2DMatchConfig *cfg);
size_t s2d_match_arena_bytes(const S2DMatchConfig *cfg, int64_t n_envs);
int s2d_match_create(const S2DMatchConfig *cfg, int64_t n_envs, int device, void *arena_dev, size_t arena_bytes,
                     void *stream, S2DMatchHandle *out);
void s2d_match_destroy(S2DMatchHandle h);
int s2d_match_buffers(S2DMatchHandle h, S2DMatchBuffers *out);
/* byte offsets of every S2DMatchBuffers pointer from the arena base (slot 0 = arena size) */
int s2d_match_buffer_offsets(S2DMatchHandle h, int64_t *offsets, int n_offsets);
/* kick-off formation, full stamina, score 0-0, cycle 0, KickOff for the left side */
int s2d_match_reset(S2DMatchHandle h, const uint8_t *mask_dev, void *stream);
/* actions_dev: float[N][22][3] = {command, a, b}: Dash(power=a, dir=b) Turn(moment=a)
 * Kick(power=a, dir=b) Tackle(power_or_dir=a, foul = b != 0; idl/service.proto:399-402) Catch(dir=a, goalies only) Move(x=a, y=b in the team's own frame: the
 * right team's coordinates are mirrored; legal before a kick-off into the own half, and for a goalie
 * holding a caught ball inside his penalty area); NULL = uniform random policy drawn in-kernel */
int s2d_match_step(S2DMatchHandle h, const float *actions_dev, void *stream);
int s2d_match_rollout(S2DMatchHandle h, int n_steps, const float *actions_dev /* [T][N][22][3] or NULL */,
                      const S2DMatchRollout *out, void *stream);

/* Per-slot controllers.  Without a table (the default, and after s2d_match_set_controllers(h, NULL)) every slot takes the caller's
 * row, or the random policy when actions_dev is NULL: the behaviour above.  With a table, each of the 22 slots has its own code:
 *   S2D_CTL_EXTERNAL  the caller's row of actions_dev (rows of the other slots are never read: they may hold anything),
 *   S2D_CTL_RANDOM    the random policy's draw (the same Philox stream and counters as with actions_dev == NULL),
 *   S2D_CTL_SCRIPTED  the scripted team below, evaluated in the cycle kernel from the start-of-cycle state of the match.
 * s2d_match_step / s2d_match_rollout use the table when one is set.
 *
 * The scripted team is this project's own rule-based baseline, written to give a learner an opponent that plays and to label
 * expert actions.  It is not the behaviour of any published team (helios or other) and claims no parity with a reference.  For
 * player l of side s, the first rule that applies wins (ball = the ball at the start of the cycle; "goal" = the centre of a goal
 * line; every direction is relative to the body, norm(atan2_deg(dy, dx) - body), every distance is compared squared):
 *   1. NONE in the halted modes (TimeOver, Pause, Human), the dead-ball modes (announcements, AfterGoal_, BeforeKickOff,
 *      FirstHalfOver, ExtendHalf, GoalieCatch_, the shoot-out modes other than PenaltyReady_ / PenaltyTaken_), and for a player
 *      who is tackling or sent off.
 *   2. A goalie holding a caught ball (FreeKick_, ball_holder == l + 1): KICK(max_power, toward the opponents' goal).
 *   3. Goalie catch: the goalie in PlayOn (or defending in PenaltyTaken_) with catch_ban == 0, the ball within his catch length
 *      (catchable_area_l * stretch) and catch angle, inside his own penalty area, last touched by the other side (no back pass):
 *      CATCH(direction of the ball).
 *   4. The ball kickable (his PlayerType's kickable area) and his team may play it (PlayOn or its own restart):
 *      KICK(max_power, toward the opponents' goal).
 *   5. Chaser: his team's nearest non-goalie to the ball (ties to the lower index, sent-off players excluded), in PlayOn and his
 *      team's own restarts: with ang = direction of the ball, TURN(ang) if |ang| > S2D_SCRIPT_TURN_TOL, else
 *      DASH(S2D_SCRIPT_DASH_POWER, 0).
 *   6. The goalie otherwise: goes to (-+S2D_SCRIPT_GOALIE_X, clamp(ball_y * S2D_SCRIPT_GOALIE_Y_GAIN, +-S2D_SCRIPT_GOALIE_Y_MAX)) on
 *      his own goal's side with the same turn / dash rule; within S2D_SCRIPT_ARRIVE of it he turns toward the ball instead (TURN if
 *      |ang| > S2D_SCRIPT_TURN_TOL, else NONE).
 *   7. Everybody else: the same toward his home position -- the kick-off formation's place (x mirrored for the right team) plus
 *      S2D_SCRIPT_HOME_GAIN_X * ball_x, S2D_SCRIPT_HOME_GAIN_Y * ball_y, clamped to the pitch.  This also covers the other team's
 *      restarts: nobody chases a ball the other side is to play.
 *   8. The shoot-out: in PenaltyReady_ / PenaltyTaken_ the current taker uses rules 4 and 5 (he is his team's chaser), the
 *      defending goalie in PenaltyTaken_ rules 3 and 6; both aim at / guard the goal the kicks are taken at (the right one).
 *      Everybody else: NONE.
 * The constants: */
enum { S2D_CTL_EXTERNAL = 0, S2D_CTL_RANDOM = 1, S2D_CTL_SCRIPTED = 2 };
#define S2D_SCRIPT_TURN_TOL 10.0f       /* degrees: a target further off the body axis is turned to, not dashed to */
#define S2D_SCRIPT_ARRIVE 1.0f          /* m: a goalie / home position this close is reached */
#define S2D_SCRIPT_DASH_POWER 100.0f    /* power of every scripted dash */
#define S2D_SCRIPT_GOALIE_X 50.0f       /* |x| of the goalie's guard point (2.5 m in front of his goal line) */
#define S2D_SCRIPT_GOALIE_Y_GAIN 0.25f  /* guard point y = this * ball y ... */
#define S2D_SCRIPT_GOALIE_Y_MAX 5.0f    /* ... clamped to +- this (inside the goal mouth, half width 7.01) */
#define S2D_SCRIPT_HOME_GAIN_X 0.5f     /* home position = formation place + these gains * ball position */
#define S2D_SCRIPT_HOME_GAIN_Y 0.25f
/* ctl: host array of 22 codes, or NULL = no table (the behaviour without one).  Error: a code outside 0..2. */
int s2d_match_set_controllers(S2DMatchHandle h, const uint8_t *ctl);
/* s2d_match_rollout plus the action record: actions_out_dev = float[T][N][22][3] (4-byte aligned) or NULL receives the (command, a, b)
 * each slot's controller produced in each cycle, before the engine's own gating (halted modes, tackling, red cards); caller slots
 * hold the caller's row.  Without a table the record shows the behaviour without one.  Errors: an unaligned actions_out_dev; a table
 * with an S2D_CTL_EXTERNAL slot while actions_dev is NULL (that error also applies to s2d_match_step / s2d_match_rollout). */
int s2d_match_rollout_ex(S2DMatchHandle h, int n_steps, const float *actions_dev, const S2DMatchRollout *out,
                         float *actions_out_dev, void *stream);

/* Per-agent relative tables of the WorldModel every player receives: for agent p (0..21) and object
 * j (0..21 players, 22 = ball) dist[N][22][23] = Player.dist_from_self / Ball.dist_from_self and
 * angle[N][22][23] = Player.angle_from_self / Ball.angle_from_self (absolute direction of j seen from
 * p, degrees; idl/service.proto:84-85, 155-156).  The diagonal (j = p) is 0. */
int s2d_match_relative(S2DMatchHandle h, float *dist_dev, float *angle_dev, void *stream);

/* Per-agent observations in each team's own frame (the WorldModel / Self / InterceptTable / Player messages every agent reads,
 * idl/service.proto:144-265, 306-349), from the current state.  A full-state observation: the view cone, the see-message
 * quantisation and the see timing are the vision layer's ("Vision" below, s2d_match_see), not this row's.  One row of
 * S2D_AGENT_OBS_DIM float32 words per agent; integers and flags are stored as their float values.
 *
 * Own frame.  For agent p of side s (left = slots 0..10, right = 11..21), sgn = +1 left, -1 right:
 *   every position and velocity is multiplied by sgn (exact); every body direction b becomes
 *   s == left ? b : (b > 0 ? b - 180 : b + 180); all further arithmetic uses only these own-frame values, so for a mirrored state
 *   (teams swapped, positions and velocities negated, bodies turned by 180) the rows are bitwise those of the original.
 *   Distances are hypot2(dx, dy), bearings norm_deg_any(atan2_deg(dy, dx) - body) with the fp32 spec functions (DESIGN.md
 *   section 4); sq2(x, y) = fmaf(x, x, y * y).  Unum = slot index within the team + 1.  "Active" = card < S2D_CARD_RED.
 *   "Ours" / "theirs": sides as seen from s; a side word is +1 ours, -1 theirs, 0 none.
 *
 * Words (offsets below):
 *   self [0, 16)       x, y, vx, vy, body, stamina, effort, recovery, stamina_capacity, is_goalie (slot 0 / 11), tackle_cycles,
 *                      card, is_kickable, kick_rate, catch_ban, PlayerType id
 *   ball [16, 24)      x, y, vx, vy, dist_from_self, bearing, last_touch (side word), holder (+1 our goalie holds a caught ball,
 *                      -1 theirs, 0 nobody: S2DMatchBuffers.ball_holder)
 *   game [24, 48)      game_mode_type, mode side (side word), our_score, their_score, cycle, stopped_cycle,
 *                      cycles_to_period_end (cycles until the clock reaches the end of the current half or extra half, the
 *                      engine's countdown), is_penalty_kick_mode, offside_line_x, our_defense_line_x, their_defense_line_x,
 *                      kickable teammate unum, kickable opponent unum, self reach steps, first teammate reach / unum, second
 *                      teammate reach / unum, first opponent reach / unum, second opponent reach / unum, is_our_set_play,
 *                      is_their_set_play
 *   teammates [48, 136)  11 rows of 8 words in slot order, self included: x, y, vx, vy, body, dist, bearing, reach_steps
 *   opponents [136, 224) 11 rows of 8 words in slot order, the same words
 * Definitions:
 *   is_kickable   sq2(ball - self) <= the slot's kickable bound (the largest float whose root does not exceed its PlayerType's
 *                 kickable area: the engine's own test); 0 for an inactive agent.
 *   kick_rate     when kickable: kick_power_rate * (1 - 0.25 * (dir_diff * (1/180)) - 0.25 * (dist_ball / kickable_margin)), in the
 *                 operation order of the engine's kick (dir_diff = |ball bearing|, dist_ball = sqrtf(sq2) - player_size -
 *                 ball_size, the division a multiplication by the float of 1/kickable_margin); otherwise 0.
 *   reach_steps   this project's own estimate, not librcsc's InterceptSimulator (no parity claimed).  The ball runs noise-free,
 *                 pos += vel; vel *= ball_decay; the player stands still at t = 0 and gains his type's player_speed_max per
 *                 cycle.  t = 0 hits if sq2(ball - pos) <= the kickable bound; t >= 1 if sq2(ball_t - pos) <= r * r with
 *                 r = ka + (float)t * speed_max, ka = (float)((float)player_size + (float)ball_size) + (float)kickable_margin.
 *                 The first t in 0..S2D_AGENT_REACH_MAX, else S2D_AGENT_REACH_NONE; inactive players: NONE.
 *   first / second teammate / opponent   the two smallest (reach, slot) keys among the active players of that team, self
 *                 excluded from the teammates; missing ones: reach NONE, unum 0.
 *   kickable teammate / opponent   unum of the lowest-slot active kickable player of that team other than self; 0 if none.
 *   offside_line_x  max(0, ball x, second-largest x among the 11 opponents), own frame: the line of the engine's offside rule.
 *                 As there, the scan covers all 11 opponents, sent-off ones included at their parked place (x = 0 beside the
 *                 halfway line), and "second-largest" counts equal values twice.
 *   our_defense_line_x    min(ball x, x of our active non-goalies); their_defense_line_x = max(ball x, x of their active
 *                 non-goalies); own frame.  (The proto's comment says "minimum" for both; the maximum for theirs is a deliberate
 *                 choice: in the own frame their last defender is the one with the largest x.)
 *   is_penalty_kick_mode  the mode is a shoot-out mode: 22, 23, 24, 25, 26, 28 or 29 (IllegalDefense_, 27, is not one).
 *   is_our_set_play       the mode is KickOff_, KickIn_, FreeKick_, CornerKick_, GoalKick_, IndFreeKick_, GoalieCatch_ or
 *                 PenaltyKick_ and its side is ours; is_their_set_play: the same with theirs.
 *   rows of inactive teammates / opponents: 0 except reach = NONE (this includes the agent's own row when he is sent off).
 *   the agent's own row: dist = 0 and bearing = 0. */
#define S2D_AGENT_OBS_DIM 224          /* float32 words per agent: 896 B, 14 lines of 64 B */
#define S2D_AGENT_OBS_SELF 0
#define S2D_AGENT_OBS_BALL 16
#define S2D_AGENT_OBS_GAME 24
#define S2D_AGENT_OBS_TEAMMATES 48
#define S2D_AGENT_OBS_OPPONENTS 136
#define S2D_AGENT_OBS_ROW_WORDS 8     /* words of one teammate / opponent row */
#define S2D_AGENT_REACH_MAX 50
#define S2D_AGENT_REACH_NONE 51
/* obs_dev: float[N][popcount(slot_mask)][S2D_AGENT_OBS_DIM], rows in ascending slot order, 16-byte aligned.
 * slot_mask: bits 0..21 (0x3FFFFF all, 0x7FF the left team).  Reads the current state; writes nothing else.
 * Errors: a mask with bits above 21, an empty mask, a NULL or unaligned obs_dev. */
int s2d_match_agent_obs(S2DMatchHandle h, uint32_t slot_mask, float *obs_dev, void *stream);

/* Network slots: the caller's epsilon-greedy Q-network chooses the action of every slot in slot_mask inside the cycle kernel, on
 * that slot's own-frame agent row.  One network serves all its slots (both teams: self-play); the other slots keep their
 * controllers (the table of s2d_match_set_controllers, or the caller's rows / the random policy without one).  For network slot l
 * of match e in a cycle:
 *   1. x = the slot's S2D_AGENT_OBS_DIM-word row of the START-of-cycle state: bitwise what s2d_match_agent_obs returns for it (the
 *      two share one device function).
 *   2. y = W3 relu(W2 relu(W1 x + b1) + b2) + b3, each unit acc = b[j]; for k ascending: acc = fmaf(W[j][k], in[k], acc); relu maps
 *      NaN and -0 to +0.  params (device, 16-byte aligned, torch nn.Sequential(...).parameters() order):
 *      W1[h1][224], b1[h1], W2[h2][h1], b2[h2], W3[K][h2], b3[K]; h1, h2 in {16, 32, 48, 64}, 1 <= K <= 64.
 *   3. greedy = the first index of the maximum of y (best = 0; for a = 1 .. K-1: if (y[a] > y[best]) best = a: a NaN never
 *      replaces the best).
 *   4. exploration: w = Philox block (counter = the match's tick, stream S2D_MATCH_ST_NET, block = l), the random policy's keys;
 *      thr = *epsilon >= 1 ? 2^32 : *epsilon > 0 ? (uint64)(*epsilon * 2^32) : 0 (epsilon read when the kernel runs);
 *      index = w.x < thr ? (w.y * K) >> 32 : greedy.
 *   5. (cmd, a, b) = table[index] (device float[K][3], read at run time; cmd = (int)table[index][0]), then the engine's usual
 *      gating, exactly as for a scripted slot.  Bodies are relative and Move is in own-frame coordinates: no per-side conversion.
 * The engine keeps the pointers, not copies: a launch (or a captured graph's replay) acts with what params, epsilon and table
 * hold when it runs; every launch first repacks params into an engine-owned copy in the kernel's fragment order. */
#define S2D_MATCH_ST_NET 7   /* Philox stream id of the network slots' exploration (no other match draw uses it) */
typedef struct S2DMatchNet {
  int32_t h1, h2, n_actions;   /* hidden widths, K */
  uint32_t slot_mask;          /* bits 0..21 */
  const float *params;         /* device, 16-byte aligned, layout above */
  const float *epsilon;        /* device float */
  const float *table;          /* device float[K][3] */
} S2DMatchNet;
/* net == NULL: no network (the behaviour above).  Errors (S2D_EINVAL, the engine unchanged): h1 / h2 not in {16, 32, 48, 64},
 * n_actions outside [1, 64], an empty slot_mask or bits above 21, NULL or unaligned pointers.  s2d_match_step, s2d_match_rollout and
 * s2d_match_rollout_ex use the network when one is set; a caller row of a network slot is never read. */
int s2d_match_set_network(S2DMatchHandle h, const S2DMatchNet *net);
/* Opponent network: a second, independent network of the same kind, so that a learner plays a frozen snapshot of itself (or another
 * league member) inside one launch.  It takes the same S2DMatchNet -- its own h1, h2, n_actions, slot_mask, params, epsilon and
 * table -- and the engine keeps its pointers and repacks its params before every launch, as for the first network.
 *   - Steps 1 to 5 of "Network slots" hold for each slot with the network that slot belongs to: the same start-of-cycle row, the
 *     same k-ascending fmaf order, relu and first-maximum argmax, the same Philox stream S2D_MATCH_ST_NET with block = the slot; the
 *     threshold from that network's own *epsilon, the random index below that network's own K, the action from its own table.
 *   - The two slot masks must be disjoint: a slot's index is a function of its own network only.
 *   - The two are symmetric and either may be set without the other: (network A on mask a, opponent B on mask b) and (network B on
 *     b, opponent A on a) are bitwise the same launch; with one of them set the launch is the single-network one.
 *   - s2d_match_step, s2d_match_rollout, s2d_match_rollout_ex and s2d_match_rollout_net use both.  net_index_out holds the index of
 *     the slots of either network, -1 elsewhere (the masks tell which network a slot belongs to); agent_obs_out is unchanged.
 *   - s2d_match_kernel_name ends in "two networks>" when both are set.
 * net == NULL clears the opponent only, and s2d_match_set_network(h, NULL) the first network only.  Errors (S2D_EINVAL, the engine
 * unchanged): everything s2d_match_set_network rejects; a slot_mask that overlaps the other network's (s2d_match_set_network
 * rejects the same against a set opponent); a see network is set -- the see network stays single, and s2d_match_set_see_network
 * clears both agent-row networks. */
int s2d_match_set_opponent_network(S2DMatchHandle h, const S2DMatchNet *net);
/* s2d_match_rollout_ex plus two records (either may be NULL):
 *   net_index_out_dev  int32[T][N][22]: the index each network slot chose, -1 for the other slots (4-byte aligned);
 *   agent_obs_out_dev  float[T][N][popcount(obs_mask)][S2D_AGENT_OBS_DIM]: the start-of-cycle rows of the slots in obs_mask, in
 *                      ascending slot order (the learner's obs_t; 16-byte aligned; written as whole 64-byte lines).
 * Errors: as s2d_match_rollout_ex; unaligned records; agent_obs_out_dev with an empty obs_mask or bits above 21. */
int s2d_match_rollout_net(S2DMatchHandle h, int n_steps, const float *actions_dev, const S2DMatchRollout *out,
                          float *actions_out_dev, int32_t *net_index_out_dev, uint32_t obs_mask, float *agent_obs_out_dev,
                          void *stream);

/* Policy slots: a stochastic policy (PPO / A2C with shared parameters) in the place of the epsilon-greedy Q-network of "Network
 * slots" -- the slot's action is sampled from the policy's own categorical distribution and its log-probability is recorded.
 * Either role (the one s2d_match_set_network fills, the one s2d_match_set_opponent_network fills) may hold one.  For a policy slot
 * l of match e in a cycle:
 *   1. x = the row of step 1 of "Network slots", unchanged (the device function of s2d_match_agent_obs).
 *   2. logits y = W3 f(W2 f(W1 x + b1) + b2) + b3 in the same k-ascending fmaf order, params in the S2DMatchNet layout;
 *      f = relu (NaN and -0 -> +0) or tanh_spec (include/s2d.h), the same on both hidden layers; the output layer is linear.
 *   3. The head is the categorical head of s2d_rollout_policy (include/s2d.h; tests/policy_ref.c::categorical restates it): m = the
 *      first maximum of y, at index g; S = sum over a ascending of exp_spec(y[a] - m).  Not deterministic: target = rnd_u01(w) * S,
 *      index = the first a whose running sum c (c = 0; c += exp_spec(y[a] - m), a ascending) exceeds target, g if none does.
 *      Deterministic (*deterministic != 0, read when the kernel runs): index = g.  Both: logp = (y[index] - m) - log_spec(S).
 *   4. w = word z of the Philox block of step 4 of "Network slots" (counter = the match's tick, stream S2D_MATCH_ST_NET, block = l).
 *      The epsilon-greedy head uses words x and y of that block: its draws and the keys are what they were.
 *   5. (cmd, a, b) = table[index], then the engine's usual gating, as in step 5.
 * Roles: each role holds at most one network, of either kind -- setting a policy network replaces a Q-network there and the
 * reverse; s2d_match_set_network(h, NULL) and s2d_match_set_opponent_network(h, NULL) clear their role whatever it holds, and so
 * does net == NULL here.  All four combinations of kinds are legal; the two masks must be disjoint whatever the kinds; the symmetry
 * of the opponent network holds: (A in role 0 on mask a, B in role 1 on b) is bitwise the launch (B in role 0 on b, A in role 1 on
 * a).  Setting role 0 clears a see network (as s2d_match_set_network does), setting role 1 while a see network is set is
 * S2D_EINVAL, and s2d_match_set_see_network clears policy networks too.  Not offered: a Gaussian head (11v11 actions go
 * through the table), a value head (the critic runs on the recorded rows), action masking.  A policy on see rows is the see
 * network's counterpart of this one ("See policy slots" below, s2d_match_set_see_policy_network), not a role here.
 * The engine keeps the pointers, not copies, as for S2DMatchNet.
 * Errors (S2D_EINVAL, the engine unchanged): a role other than 0 or 1; an activation other than 0 or 1; h1 / h2 not in {16, 32, 48,
 * 64}; n_actions outside [1, 64]; an empty slot_mask or bits above 21; NULL or unaligned pointers (params 16 bytes, deterministic
 * and table 4); a slot_mask that overlaps the other role's.
 * s2d_match_kernel_name ends in "policy network>" when one role is set and holds a policy network, in "two networks, policy>" when
 * both roles are set and at least one holds a policy network. */
#define S2D_MATCH_ROLE_NETWORK  0   /* the role s2d_match_set_network fills */
#define S2D_MATCH_ROLE_OPPONENT 1   /* the role s2d_match_set_opponent_network fills */
typedef struct S2DMatchPolicyNet {
  int32_t h1, h2, n_actions;      /* {16,32,48,64}, {16,32,48,64}, 1..64 */
  uint32_t slot_mask;             /* bits 0..21, not empty */
  int32_t activation;             /* 0 relu, 1 tanh (tanh_spec) on both hidden layers */
  const float *params;            /* device, 16-byte aligned, the S2DMatchNet layout */
  const uint32_t *deterministic;  /* device word, read when the kernel runs: != 0 -> greedy */
  const float *table;             /* device float[K][3] */
} S2DMatchPolicyNet;
int s2d_match_set_policy_network(S2DMatchHandle h, int role, const S2DMatchPolicyNet *net);
/* s2d_match_step, s2d_match_rollout, s2d_match_rollout_ex and s2d_match_rollout_net use a policy network when one is set
 * (s2d_match_rollout_net then records the index alone).  This is s2d_match_rollout_net plus
 *   logp_out_dev  float[T][N][22] (4-byte aligned, or NULL): a policy slot receives the log-probability of the index it took (in
 *                 deterministic mode: of the greedy index); every other slot, Q-network slots included, receives 0.0f.
 * With no policy network set it behaves as s2d_match_rollout_net and logp_out_dev is all zeros.
 * Errors: as s2d_match_rollout_net; an unaligned logp_out_dev. */
int s2d_match_rollout_policy(S2DMatchHandle h, int n_steps, const float *actions_dev, const S2DMatchRollout *out,
                             float *actions_out_dev, int32_t *net_index_out_dev, float *logp_out_dev,
                             uint32_t obs_mask, float *agent_obs_out_dev, void *stream);

/* Agent reward: an opt-in per-agent shaped reward, computed inside the cycle kernel where it writes its records.  The engine's own
 * reward stays reward_left (+1 / -1 on a goal); this record is what a learner of sparse-goal self-play can learn from.  With no
 * agent reward set an engine launches what it launched before, under the same names, and every record is bitwise what it was.
 * For a cycle, S is the match's start-of-cycle state and S' the state the cycle leaves -- after the auto-reset, if the cycle
 * ended the match: what s2d_match_buffers shows.  For agent l: sgn = +1 for slots 0..10, -1 for 11..21; row(S) is the agent's
 * S2D_AGENT_OBS_DIM-word row of S as s2d_match_agent_obs defines it (the same device functions: the words below are bitwise the
 * row's words).
 *   live    mode(S) == PlayOn && mode(S') == PlayOn: a cycle that starts or ends in a restart, a halted mode, or a finished
 *           (and reset) match is never live.
 *   active  card(S) < S2D_CARD_RED && card(S') < S2D_CARD_RED.
 *   chaser(S)  the scripted team's rule-5 chaser of the agent's team in S ("Controllers" above): its nearest non-goalie to the
 *           ball by sq2, ties to the lower index, sent-off players excluded.
 *   gate    active && (chaser_only ? chaser(S) == l : true).
 * Terms, in this order (team terms are the same for the 11 agents of a side; individual ones are the agent's own):
 *   0 goal          team        sgn * reward_left(S')
 *   1 ball_advance  team        live ? row(S')[ball.x] - row(S)[ball.x] : 0     own frame: positive toward the opponents' goal
 *   2 approach      individual  live && gate ? row(S)[ball.dist_from_self] - row(S')[ball.dist_from_self] : 0
 *   3 facing        individual  live && gate ? (|row(S)[ball.bearing]| - |row(S')[ball.bearing]|) * (float)(1.0 / 180.0) : 0
 *   4 kickable      individual  mode(S') == PlayOn && active ? row(S')[self.is_kickable] : 0
 *   5 possession    team        mode(S') == PlayOn ? row(S')[ball.last_touch] : 0     the side word: +1 ours, -1 theirs, 0 none
 * reward = acc after: acc = +0; for k ascending: acc = fmaf(w[k], term[k], acc).  Every "0" above is +0.0f.  Terms 2 + 3 with unit
 * weights are the reference's ReachBall reward (reach_ball_env.py:130-134), per agent.
 * w = weights: a device float[S2D_MATCH_REWARD_TERMS], read when the kernel runs (once, at its start), like epsilon: a captured
 * graph replays with what the buffer holds, and a curriculum anneals it in place.  The engine keeps the pointer, not a copy.
 * Mirror property: for a mirrored pair of (S, S') (teams swapped, positions and velocities negated, bodies turned by 180, sides
 * swapped, reward_left negated) the mirrored agents' rewards are bitwise equal; between the two sides of one match the team terms
 * 0, 1 and 5 are exact negations of each other.
 * Lanes past the 22 agents and matches past N store nothing.
 * Not offered: an agent reward with the see network (its cycle kernel is out of scope: setting either while the other is set is
 * S2D_EINVAL); per-agent weights; terms that need more of the row than the words above.
 * s2d_match_kernel_name gains the suffix ", agent reward>" in place of ">" while an agent reward is set (the instantiation a
 * launch takes has the record only when s2d_match_rollout_reward is given one).
 * rw == NULL clears.  Errors (S2D_EINVAL, the engine unchanged): NULL or unaligned weights; chaser_only outside {0, 1}; a see
 * network is set (and s2d_match_set_see_network refuses while an agent reward is set). */
#define S2D_MATCH_REWARD_TERMS 6
typedef struct S2DMatchAgentReward {
  const float *weights;   /* device float[S2D_MATCH_REWARD_TERMS], 4-byte aligned */
  int32_t chaser_only;    /* 0 | 1 */
} S2DMatchAgentReward;
int s2d_match_set_agent_reward(S2DMatchHandle h, const S2DMatchAgentReward *rw);
/* s2d_match_rollout_policy plus
 *   agent_reward_out_dev  float[T][N][22] (4-byte aligned, or NULL): the agent reward of every agent for every cycle.
 * With agent_reward_out_dev == NULL it is s2d_match_rollout_policy.  With a record the launch takes the ", agent reward"
 * instantiation of the kernel it would have taken: the controller one (without a table: every slot the caller's row, or random,
 * as for the action record), the network one or the policy one; every other record and the final state are bitwise those of the
 * launch without it.
 * Errors: as s2d_match_rollout_policy; a record while no agent reward is set; an unaligned record. */
int s2d_match_rollout_reward(S2DMatchHandle h, int n_steps, const float *actions_dev, const S2DMatchRollout *out,
                             float *actions_out_dev, int32_t *net_index_out_dev, float *logp_out_dev,
                             uint32_t obs_mask, float *agent_obs_out_dev, float *agent_reward_out_dev, void *stream);

/* Vision: an opt-in layer beside the engine -- view cone, neck, see-message quantisation, see timing.  Restated from the published
 * behaviour of rcssserver's synchronous see mode; like every 11v11 rule it is this project's own restatement: PARITY TO RCSSSERVER
 * UNPINNED.  The fp32 words below are the contract (the device equals tests/see_ref.c bit for bit).  The engine handle stores
 * nothing of it: the three state planes are the caller's, an engine that never calls these functions is byte for byte the engine
 * without them.  Deviations: the self words are exact (self-localisation from flags and lines is not modelled: they are what
 * sense_body plus a perfect localiser would give); no landmark flags or lines; no gaussian_see; nothing is heard but the referee
 * (the game words; what players say is the opt-in "Hearing" layer below, a row of its own); synchronous timing only.
 *
 * Parameters (ServerParam names; doubles, each rounded to fp32 once; a reciprocal inv(v) is the float of the double 1 / v):
 *   view_angle[3]       60, 120, 180 degrees for narrow, normal, wide (rcssserver: visible_angle 90 scaled by 2/3, 4/3 and 2 in
 *                       synchronous mode; the comment at idl/service.proto:12-14 names 60 / 90 / 180)
 *   see_interval[3]     1, 2, 3 cycles between two see messages (whole numbers)
 *   visible_distance    3: closer objects outside the cone are felt
 *   dist_quantize_step 0.1, dist_round 0.1, dist_chg_quantize 0.02, dir_chg_quantize 0.1
 *   unum_far_length 20, unum_too_far_length 40, team_far_length 40, team_too_far_length 60 (idl/service.proto:1713-1716)
 *   min / max_neck_moment -+180, min / max_neck_angle -+90 (:1477-1480) */
typedef struct S2DVisionParams {
  double view_angle[3], see_interval[3];
  double visible_distance;
  double dist_quantize_step, dist_round, dist_chg_quantize, dir_chg_quantize;
  double unum_far_length, unum_too_far_length, team_far_length, team_too_far_length;
  double min_neck_moment, max_neck_moment, min_neck_angle, max_neck_angle;
} S2DVisionParams;
void s2d_match_vision_default_params(S2DVisionParams *prm);
/* Errors: non-finite values; view angles outside (0, 360]; intervals < 1 (or not whole, or > 1e6); quantisation steps <= 0; negative
 * distances; a far length above its too_far length; a minimum above its maximum. */
int s2d_match_vision_validate(const S2DVisionParams *prm);

/* The vision state: caller-owned device planes [N][24] (slot = player; slots 22, 23 are padding), 4-byte aligned. */
typedef struct S2DMatchVision {
  float *neck;          /* neck angle relative to the body, degrees */
  int32_t *view_width;  /* S2D_VIEW_NARROW / NORMAL / WIDE; any other value reads as normal */
  int32_t *see_wait;    /* cycles until the next see message; right after a step, see_wait == see_interval[width] says "fresh" */
} S2DMatchVision;
enum { S2D_VIEW_KEEP = 0, S2D_VIEW_NARROW = 1, S2D_VIEW_NORMAL = 2, S2D_VIEW_WIDE = 3 };
/* neck = +0, width = normal, wait = 0 in every slot of the masked matches (mask_dev NULL = all).  A reset state is not fresh: the
 * first s2d_match_vision_step makes every player see. */
int s2d_match_vision_reset(S2DMatchHandle h, const S2DMatchVision *vis, const uint8_t *mask_dev, void *stream);
/* One cycle of the vision state; call it once after each body step.  view_actions_dev: float[N][22][2] = (TurnNeck moment,
 * ChangeView code) per player, or NULL = nobody turns or changes.  Codes: S2D_VIEW_*; any other value (NaN included) keeps the width.
 * done_dev: uint8[N] or NULL.  For player l of match e:
 *   1. done_dev[e] != 0: neck = +0, width = normal, wait = 0 (the match has just restarted; the actions are not read).
 *   2. otherwise a sent-off player (card == S2D_CARD_RED) keeps all three words and nothing below happens to him.
 *   3. otherwise, with actions: m = moment is NaN ? 0 : clamp(moment, min_neck_moment, max_neck_moment);
 *      neck = clamp(norm_deg_any(neck + m), min_neck_angle, max_neck_angle)   (clamp(v, lo, hi) = v < lo ? lo : v > hi ? hi : v);
 *      with a code 1..3: width = code and wait = min(wait, see_interval[code]) -- a pending wait never exceeds the new width's
 *      interval, so switching to a narrower view shortens the wait and "fresh" below stays unambiguous.
 *   4. the timer (cases 1 and 3): wait = max(wait - 1, 0); fresh = (wait == 0); if fresh: wait = see_interval[width].
 * fresh is not stored: after the step it is see_wait == see_interval[width].  What a ChangeView does, with the default intervals:
 *   - to a width whose interval is not below the pending wait (any change to a wider view, for one): the running timer goes on;
 *     the new cone is first used at its next expiry, the new interval from then on.
 *   - to a narrower width with a longer wait pending: the wait is cut in the same step, so the next see message comes EARLIER than
 *     the running timer would have sent it.  To narrow (interval 1) that is this very cycle: wait = min(wait, 1) = 1, the timer
 *     takes it to 0, the player is fresh in the step of the ChangeView and in every cycle after it.  Wide (wait 3) -> normal gives
 *     wait 2 -> 1: fresh in the next cycle, one cycle before the wide timer would have expired.  Without the cut that step would
 *     leave wait == 2 == see_interval[normal], which reads as fresh although no see message is due.
 * Reads the card plane of the engine; writes the three planes only.  While a see network is set ("See network" below) the cycle
 * kernel runs this step itself, once per cycle: do not call it for those cycles as well. */
int s2d_match_vision_step(S2DMatchHandle h, const S2DVisionParams *prm, const S2DMatchVision *vis, const float *view_actions_dev,
                          const uint8_t *done_dev, void *stream);

/* The see row of agent p: S2D_SEE_DIM float32 words in p's team's own frame, exactly as in the agent rows above (positions and
 * velocities times sgn, bodies turned by 180 degrees for the right team, all arithmetic on own-frame values: a mirrored state gives
 * the mirrored agent bitwise the same row when no distance lies inside a probabilistic band).  Integers and flags are stored as
 * their float values.
 *   self [0, 16)     x, y, vx, vy, body, neck, face, view width code (1..3), fresh (0 / 1), see_wait, stamina, effort, recovery,
 *                    stamina_capacity, is_goalie, card.                   face = norm_deg_any(body + neck)
 *   ball [16, 24)    level, dist, dir, dist_chg, dir_chg | game_mode_type, mode side (side word), cycle (the referee is heard)
 *   players [24, 192)  21 rows of 8 words: level, team (+1 ours, -1 theirs, 0 unknown), unum (0 unknown), dist, dir, dist_chg,
 *                    dir_chg, body_rel
 * The self words and the three game words are always delivered.  When the cycle is not fresh for p, or p is sent off, the five ball
 * words and all player rows are +0.  Otherwise, for every other ACTIVE object j (card < S2D_CARD_RED; the ball is always active), in
 * this order of fp32 operations (quant(v, q) = rintf(v * inv(q)) * q):
 *   dx = x_j - x_p, dy = y_j - y_p;  d = hypot2(dx, dy)
 *   rel = d == 0 ? 0 : norm_deg_any(atan2_deg(dy, dx) - face)
 *   in_cone = fabsf(rel) <= 0.5f * view_angle[width];   felt = d <= visible_distance
 *   level = in_cone ? (ball: 4; player: by distance, below) : felt ? 1 : 0
 *   level >= 1:  dist = d == 0 ? 0 : quant(exp_spec(quant(log_spec(d), dist_quantize_step)), dist_round);  dir = rintf(rel)
 *   level == 4, d != 0:  ex = dx / d, ey = dy / d, rvx = vx_j - vx_p, rvy = vy_j - vy_p
 *                dist_chg = dist * quant(fmaf(rvx, ex, rvy * ey) / d, dist_chg_quantize)
 *                dir_chg = quant((fmaf(rvy, ex, -(rvx * ey)) / d) * 57.29577951308232f, dir_chg_quantize)
 *   level == 4, players:  body_rel = rintf(norm_deg_any(body_j - face))
 *   every word a level does not carry is +0: level 1 (felt, outside the cone) and level 2 carry dist and dir only, level 3 adds the
 *   team word, level 4 the unum, the two changes and body_rel.  (A quantised word may be -0.)
 * A player in the cone:  d <= unum_far_length: 4;  else if d < unum_too_far_length and u1 >= (d - unum_far_length) *
 * inv(unum_too_far_length - unum_far_length): 4;  else if d <= team_far_length: 3;  else if d < team_too_far_length and
 * u2 >= (d - team_far_length) * inv(team_too_far_length - team_far_length): 3;  else 2.   u1, u2 = (w.x >> 8) * 2^-24,
 * (w.y >> 8) * 2^-24 of the Philox block with counter = the match's tick, stream S2D_MATCH_ST_SEE, block = p * 24 + j, the random
 * policy's keys: the row is a pure function of state, vision state and tick.
 * Order of the player rows: the seen ones (level >= 1) first, ascending by (dir, dist, slot) -- left to right across the view --
 * then the others, all +0.  The slot is the own-frame one (p's team 0..10, the other team 11..21: the raw slot for the left
 * team, (slot + 11) % 22 for the right team), so that mirrored states order alike; as the last tie-break it is a named, negligible
 * identity leak. */
#define S2D_SEE_DIM 192            /* float32 words per agent: 768 B, 12 lines of 64 B */
#define S2D_SEE_SELF 0
#define S2D_SEE_BALL 16
#define S2D_SEE_PLAYERS 24
#define S2D_SEE_ROW_WORDS 8        /* words of one player row */
#define S2D_MATCH_ST_SEE 8         /* Philox stream id of the identity draws (streams 0..7 belong to the engine) */
/* see_dev: float[N][popcount(slot_mask)][S2D_SEE_DIM], rows in ascending slot order, 16-byte aligned; slot_mask as for
 * s2d_match_agent_obs.  Reads the current state and the vision planes; writes nothing else.
 * Errors: a mask with bits above 21, an empty mask, a NULL or unaligned see_dev, invalid parameters, NULL or unaligned planes. */
int s2d_match_see(S2DMatchHandle h, const S2DVisionParams *prm, const S2DMatchVision *vis, uint32_t slot_mask, float *see_dev,
                  void *stream);

/* See network: the network slots of "Network slots" above under partial observability.  The Q-network acts on each slot's SEE row
 * (S2D_SEE_DIM words) instead of its full-state agent row, it also chooses the slot's view action (TurnNeck, ChangeView), and the
 * vision state of all 22 players is stepped inside the cycle kernel: T cycles of self-play under the vision model are one launch.
 * One see network per engine, and no agent-row network beside it: setting a see network clears the s2d_match_set_network and
 * s2d_match_set_opponent_network ones, s2d_match_set_network clears the see network.  For every cycle of a launch
 * and every match:
 *   1. For every slot in slot_mask | obs_mask: x = the slot's see row, built from the START-of-cycle engine state, the current
 *      vision state and the match's tick: bitwise what s2d_match_see returns at that moment (the two share one device function).
 *      Slots of obs_mask are recorded (s2d_match_rollout_see), as whole 64-byte lines.
 *   2. For every slot of slot_mask: steps 2 to 4 of "Network slots" on the 192 words -- params = W1[h1][192], b1[h1], W2[h2][h1],
 *      b2[h2], W3[K][h2], b3[K]; the same k-ascending fmaf order, the same relu and first-maximum argmax, the same Philox stream
 *      S2D_MATCH_ST_NET with block = slot, epsilon read when the kernel runs.
 *   3. (cmd, a, b) = table[index][0..2] (device float[K][5]), then the engine's usual gating and the body cycle.
 *   4. One vision step per player, exactly as s2d_match_vision_step specifies (the order done / sent-off / action / timer): done =
 *      this cycle's done of the match; the card is the one after the body cycle; the view action (TurnNeck moment, ChangeView
 *      code) is table[index][3..4] for a network slot, for any other slot its row of view_actions_dev, or "nobody turns or
 *      changes" when view_actions_dev is NULL.
 * One launch of T cycles therefore equals T rounds of s2d_match_see, the host-side choice, s2d_match_rollout_ex for one step and
 * s2d_match_vision_step with the engine's done.
 * The vision planes are read once at the start of a launch and written once at its end, for valid matches and slots 0..21 only.
 * While a see network is set the cycle kernel OWNS the vision step: the caller must not also call s2d_match_vision_step for those
 * cycles (s2d_match_see and s2d_match_vision_reset between launches are fine).  The engine keeps the pointers (params, epsilon,
 * table, the three planes), not copies; prm is copied at the call.
 * slot_mask == 0 is the record-only see network: no forward pass (params, epsilon and table are not read and may be NULL), the
 * vision state is stepped in the kernel and see rows can be recorded. */
typedef struct S2DMatchSeeNet {
  int32_t h1, h2, n_actions;   /* h1, h2 in {16, 32, 48, 64}; 1 <= K <= 64 */
  uint32_t slot_mask;          /* bits 0..21; 0 = no network: vision stepped and recorded in-kernel only */
  const float *params;         /* W1[h1][192], b1, W2[h2][h1], b2, W3[K][h2], b3; device, 16-byte aligned */
  const float *epsilon;        /* device float */
  const float *table;          /* device float[K][5]: command, a, b, TurnNeck moment, ChangeView code */
  S2DVisionParams prm;         /* copied at the call */
  S2DMatchVision vis;          /* the caller's three planes; the engine keeps the pointers */
} S2DMatchSeeNet;
/* net == NULL: clears the see network.  Errors (S2D_EINVAL, the engine unchanged): h1 / h2 not in {16, 32, 48, 64}, n_actions outside
 * [1, 64], bits above 21 in slot_mask; with slot_mask != 0, NULL or unaligned params (16 bytes), epsilon or table (4 bytes); NULL or
 * unaligned vision planes; parameters s2d_match_vision_validate rejects.  s2d_match_step, s2d_match_rollout and s2d_match_rollout_ex
 * use the see network when one is set, with no view actions for the other slots; s2d_match_rollout_net then returns S2D_EINVAL (the
 * agent rows are not built). */
int s2d_match_set_see_network(S2DMatchHandle h, const S2DMatchSeeNet *net);
/* s2d_match_rollout_ex with the see network, plus:
 *   view_actions_dev   float[T][N][22][2] or NULL: (TurnNeck moment, ChangeView code) of the slots outside slot_mask; rows of
 *                      network slots are never read (nor are their rows of actions_dev);
 *   net_index_out_dev  int32[T][N][22] or NULL: the index each network slot chose, -1 for the other slots;
 *   see_out_dev        float[T][N][popcount(obs_mask)][S2D_SEE_DIM] or NULL: the start-of-cycle see rows of the slots in obs_mask,
 *                      in ascending slot order (the learner's obs_t; 16-byte aligned).
 * Errors: no see network set; as s2d_match_rollout_ex; unaligned records or view actions; see_out_dev with an empty obs_mask or
 * bits above 21. */
int s2d_match_rollout_see(S2DMatchHandle h, int n_steps, const float *actions_dev, const float *view_actions_dev,
                          const S2DMatchRollout *out, float *actions_out_dev, int32_t *net_index_out_dev, uint32_t obs_mask,
                          float *see_out_dev, void *stream);

/* See policy slots: "Policy slots" under partial observability -- a stochastic policy (PPO / A2C with shared parameters) in the
 * place of the epsilon-greedy Q-network of "See network".  It occupies the see network's place: one per engine, no agent-row
 * network beside it (it clears both roles and is cleared by s2d_match_set_network and s2d_match_set_policy_network(h, 0, ..),
 * exactly as the see network is; role 1 refuses beside it; refused while an agent reward is set).  For every cycle of a launch
 * and every match:
 *   1. The see rows are step 1 of "See network", unchanged, and are recorded for obs_mask as there.
 *   2. For every slot l of slot_mask: logits y = W3 f(W2 f(W1 x + b1) + b2) + b3 on the 192 words, params in the S2DMatchSeeNet
 *      layout, the k-ascending fmaf order of step 2 of "Policy slots"; f = relu (NaN and -0 -> +0) or tanh_spec (include/s2d.h),
 *      the same on both hidden layers; the output layer is linear.
 *   3. The head is step 3 of "Policy slots" (the categorical head; *deterministic != 0, read once when the kernel runs: the first
 *      maximum) on word z of the block of its step 4: counter = the match's tick, stream S2D_MATCH_ST_NET, block = l.  There is no
 *      epsilon.  logp = (y[index] - m) - log_spec(S).
 *   4. (cmd, a, b) = table[index][0..2] (device float[K][5]), the engine's usual gating and the body cycle; then the vision step of
 *      step 4 of "See network", the slot's view action being table[index][3..4].  Slots outside slot_mask take the caller's rows,
 *      the controllers and view_actions_dev, exactly as there.
 * A finished match's or a sent-off player's row is built and acted on as "Policy slots" and "See network" treat theirs (the
 * engine's gating discards the command).  The engine keeps the pointers, not copies; prm is copied at the call.
 * Not offered: a second see role (no frozen see opponent in the same launch), the agent reward in the see families, a value head
 * or a Gaussian head (the critic runs on the recorded see rows), agent rows recorded beside see rows (an asymmetric critic),
 * action masking.
 * s2d_match_kernel_name ends in "see policy network>" while one is set. */
typedef struct S2DMatchSeePolicyNet {
  int32_t h1, h2, n_actions;      /* h1, h2 in {16, 32, 48, 64}; 1 <= K <= 64 */
  uint32_t slot_mask;             /* bits 0..21, not empty (a policy with no slots is not the record-only network) */
  const float *params;            /* W1[h1][192], b1, W2[h2][h1], b2, W3[K][h2], b3; device, 16-byte aligned */
  const uint32_t *deterministic;  /* device word, read when the kernel runs: != 0 -> greedy */
  const float *table;             /* device float[K][5]: command, a, b, TurnNeck moment, ChangeView code */
  S2DVisionParams prm;            /* copied at the call */
  S2DMatchVision vis;             /* the caller's three planes; the engine keeps the pointers */
  int32_t activation;             /* 0 relu, 1 tanh (tanh_spec) on both hidden layers */
} S2DMatchSeePolicyNet;
/* net == NULL: clears the see network, whichever kind is set.  Errors (S2D_EINVAL, the engine unchanged): everything
 * s2d_match_set_see_network rejects; an activation other than 0 or 1; a NULL or unaligned deterministic word (4 bytes); an empty
 * slot_mask; an agent reward is set.  s2d_match_step, s2d_match_rollout, s2d_match_rollout_ex and s2d_match_rollout_see use the
 * see policy when one is set (no log-probability is recorded there); s2d_match_rollout_net, s2d_match_rollout_policy and
 * s2d_match_rollout_reward return S2D_EINVAL as beside the see network. */
int s2d_match_set_see_policy_network(S2DMatchHandle h, const S2DMatchSeePolicyNet *net);
/* s2d_match_rollout_see plus
 *   logp_out_dev  float[T][N][22] (4-byte aligned, or NULL): a policy slot receives the log-probability of the index it took (in
 *                 deterministic mode: of the greedy index); every other slot receives 0.0f.
 * With a see Q-network or the record-only see network set it behaves as s2d_match_rollout_see and logp_out_dev is all zeros.
 * Errors: as s2d_match_rollout_see; an unaligned logp_out_dev. */
int s2d_match_rollout_see_policy(S2DMatchHandle h, int n_steps, const float *actions_dev, const float *view_actions_dev,
                                 const S2DMatchRollout *out, float *actions_out_dev, int32_t *net_index_out_dev,
                                 float *logp_out_dev, uint32_t obs_mask, float *see_out_dev, void *stream);

/* Belief: each agent's memory of what it has seen -- an opt-in layer beside the vision layer, the counterpart of the world model
 * every real client keeps over its see messages (idl/service.proto:71-83, 146-168: seen_position, pos_count, vel_count,
 * body_direction_count, ghost_count).  It reads NOTHING but see rows: no engine handle, no state plane -- it cannot leak ground
 * truth.  The fp32 words below are the contract (the device, csrc/s2d_belief.hip, equals tests/belief_ref.c bit for bit).
 * Deviations: this is the project's own filter and claims NO PARITY TO LIBRCSC (its WorldModel localises, matches and forgets by
 * other rules); players beyond identification range enter the belief only once they have been identified (a level 1-3 sighting
 * can move a known entry, it never creates one); the ball has no vel_count word (its eight words are full: its velocity is as old
 * as the last level-4 ball sighting, which the row does not say); self-localisation is the see row's (exact).
 *
 * A belief row is S2D_BELIEF_DIM float32 words per agent, in the agent's own-team frame (the see row's frame).  The row is both the
 * memory and the observation: belief' = f(belief, see row, parameters), there is no hidden state.  It is as wide as a see row, so
 * every 192-input network, learner and target of the see path takes it unchanged.
 *   self [0, 16)      the see row's self words, copied
 *   ball [16, 24)     x, y, vx, vy, pos_count | game_mode_type, mode side, cycle (the see row's three game words, copied)
 *   players [24, 192) 21 rows of 8 words in FIXED IDENTITY ORDER: with u = the agent's own index (raw slot % 11), row j < 10 is the
 *                     teammate with own index (j < u ? j : j + 1), row j >= 10 the opponent with unum j - 9.
 *                     Words: x, y, vx, vy, body, pos_count, vel_count, body_count.
 * The 22 ENTRIES are the ball and the 21 player rows.  Positions and velocities are absolute, in the own frame.  A count is the
 * number of updates since the word group was last seen: a whole number stored as a float, saturating at count_max.  An UNKNOWN
 * entry is all +0 with every count equal to count_max; an entry is KNOWN while pos_count < count_max.
 *
 * Parameters (doubles, each rounded to fp32 once, as S2DVisionParams):
 *   ball_decay 0.94, player_decay 0.4   ServerParam's; one player_decay for everybody (PlayerTypes are not visible)
 *   view_angle[3] 60 / 120 / 180        the vision parameters' (narrow, normal, wide)
 *   match_dist 3.0, match_rate 0.1      a level 1-3 sighting matches an entry within tol = match_dist + match_rate * dist
 *   ghost_margin 5.0                    degrees kept clear of the cone's edge when an unseen entry is forgotten
 *   count_max 1000                      a whole number in [1, 16777216]
 * match_dist, match_rate and ghost_margin are this project's own choice and are measured against nothing.
 *
 * One update of agent p's row B with its see row S (S2D_SEE_* words), in this order; "entry := unknown" writes the +0 words and
 * count_max into every count:
 *   1. Reset.  If the reset flag of p's match is set: every entry := unknown.
 *   2. Predict.  For every entry with pos_count < count_max:  x = x + vx; y = y + vy;  then vx = vx * decay; vy = vy * decay
 *      (ball_decay for the ball, player_decay for a player).  Then for EVERY entry each count c becomes
 *      (c + 1 < count_max ? c + 1 : count_max) -- a count above count_max, or NaN, becomes count_max -- and an entry whose pos_count
 *      is now count_max := unknown (a belief too old to keep is forgotten, so that every unknown entry is the canonical one).
 *   3. Copy.  B[0, 16) = S[0, 16); B[21, 24) = S[21, 24).
 *   4. Correct, only if S[self.fresh] == 1 and S[self.card] < S2D_CARD_RED.  With face, (sx, sy), (svx, svy) the self words of S, a
 *      SIGHTING (level, dist, dir, dist_chg, dir_chg) with level >= 1 gives
 *        th = norm_deg_any(face + dir);  (s, c) = sincos_deg(th);  X = fmaf(dist, c, sx);  Y = fmaf(dist, s, sy)
 *        level 4, dist != 0:  vr = dist_chg;  vt = (dir_chg * 0.017453292519943295f) * dist;
 *                             VX = fmaf(vr, c, -(vt * s)) + svx;  VY = fmaf(vr, s, vt * c) + svy
 *        level 4, dist == 0:  VX = svx;  VY = svy
 *      Ball (its five see words): level >= 1 sets x = X, y = Y, pos_count = 0 and marks it updated; level 4 also vx = VX, vy = VY.
 *      Players, first pass: the see rows of level 4, in row order.  The identity names the entry: team > 0 and unum n in 1..11,
 *        n - 1 != u: row j = (n - 1 < u ? n - 1 : n - 2);  team < 0 and n in 1..11: row j = n + 9;  any other identity (team 0, a
 *        unum outside 1..11 or not whole, the agent itself) is dropped.  Set x, y, vx, vy = X, Y, VX, VY and body =
 *        norm_deg_any(body_rel + face); all three counts = 0; mark the entry updated.  (Two rows naming one entry: the later wins.)
 *      Players, second pass: the see rows of level 1, 2 or 3, in row order, one after the other.  Candidates are the player rows
 *        compatible with the team word (> 0: rows 0..9; < 0: rows 10..20; otherwise all 21) that are not marked updated and have
 *        pos_count < count_max.  tol = fmaf(match_rate, dist, match_dist); of the candidates with q = sq2(X - x, Y - y) <= tol * tol
 *        the one with the smallest q is taken, ties to the lowest row: x = X, y = Y, pos_count = 0, marked updated; velocity, body
 *        and their counts stay.  Without such a candidate the sighting is dropped.
 *   5. Ghosts, under the condition of step 4.  wi = the view width of S (code 1 -> 0, 3 -> 2, anything else 1);
 *      cone = 0.5f * view_angle[wi] - ghost_margin.  An entry (the ball included) that is not marked updated and has pos_count <
 *      count_max := unknown when, with dx = x - sx, dy = y - sy, d = hypot2(dx, dy):
 *        d > 0  and  fabsf(norm_deg_any(atan2_deg(dy, dx) - face)) <= cone.
 *      The see model reports everything inside the cone, so the object is not where the belief put it.
 * The marks live for one update only. */
#define S2D_BELIEF_DIM 192         /* float32 words per agent: a see row's width */
#define S2D_BELIEF_SELF 0
#define S2D_BELIEF_BALL 16
#define S2D_BELIEF_PLAYERS 24
#define S2D_BELIEF_ROW_WORDS 8     /* words of one player row */
#define S2D_BELIEF_COUNT_LIMIT 16777216.0f   /* 2^24: the largest count_max (every smaller whole number is an exact float) */
typedef struct S2DBeliefParams {
  double ball_decay, player_decay;
  double view_angle[3];
  double match_dist, match_rate, ghost_margin;
  double count_max;
} S2DBeliefParams;
void s2d_match_belief_default_params(S2DBeliefParams *prm);
/* Errors: non-finite values; a decay outside (0, 1]; view angles outside (0, 360]; match_dist, match_rate or ghost_margin < 0;
 * count_max < 1, above S2D_BELIEF_COUNT_LIMIT or not whole. */
int s2d_match_belief_validate(const S2DBeliefParams *prm);
/* Engine-free, on the current device, as s2d_gae: raw device pointers, any stream of that device; no atomics, no host reads,
 * capturable.  k = popcount(slot_mask); the rows of a match are those of the mask's slots in ascending order, as s2d_match_see
 * writes them (the slot gives u).  All row buffers 16-byte aligned.
 *
 * s2d_match_belief_reset: every row of the masked matches (mask_dev uint8[N], NULL = all) becomes +0 in every word but the
 * counts, which become S2D_BELIEF_COUNT_LIMIT: the call takes no parameters, so it writes the one value that is not below any
 * count_max.  Such a row is unknown in every entry for any parameters (pos_count >= count_max), and step 2 of the first update
 * stores count_max in its place.
 * Errors: a NULL or unaligned belief_dev; n_matches < 1 (or above 2^24); a mask that is empty or has bits above 21. */
int s2d_match_belief_reset(float *belief_dev, int64_t n_matches, uint32_t slot_mask, const uint8_t *mask_dev, void *stream);
/* s2d_match_belief_scan: T = n_steps updates in one launch.
 *   see_dev     float[T][N][k][S2D_SEE_DIM]
 *   reset_dev   uint8[T][N] or NULL: a set flag = step 1 of that match's agents before row t is taken in
 *   belief_dev  float[N][k][S2D_BELIEF_DIM], updated in place to the state after row T - 1
 *   out_dev     float[T][N][k][S2D_BELIEF_DIM] or NULL: the belief after each row
 * n_steps = 1 is the per-cycle step.  Errors (S2D_EINVAL, before any HIP call): NULL prm, see_dev or belief_dev; a mask that is
 * empty or has bits above 21; see_dev, belief_dev or out_dev not 16-byte aligned; parameters s2d_match_belief_validate rejects;
 * n_steps < 1 or n_matches < 1 (or above 2^24); out_dev overlapping belief_dev or see_dev (or belief_dev overlapping see_dev). */
int s2d_match_belief_scan(const S2DBeliefParams *prm, const float *see_dev, const uint8_t *reset_dev, float *belief_dev,
                          float *out_dev, int n_steps, int64_t n_matches, uint32_t slot_mask, void *stream);

/* Belief network: the network slots of "See network" / "See policy slots" on each slot's BELIEF row -- the see row is built, taken
 * into the slot's belief row, and the network acts on that row, all inside the cycle kernel: T cycles of collection under partial
 * observability with a memory are one launch.  It occupies the see network's place: one per engine, no agent-row network beside it
 * (it clears both roles and is cleared by the calls that clear a see network; role 1 refuses beside it; refused while an agent
 * reward is set).  For every cycle of a launch, every match and slot:
 *   1. See row.  For every slot of row_mask = slot_mask | obs_mask: its see row from the start-of-cycle state, the vision state and
 *      the tick, as step 1 of "See network".  row_mask must lie inside belief_mask, the layout of the state buffer
 *      belief[N][popcount(belief_mask)][S2D_BELIEF_DIM] (what s2d_match_belief_reset / _scan take with slot_mask = belief_mask): a
 *      slot's row index in a match is its rank in belief_mask, and its own index u is slot % 11.
 *   2. Belief update.  One update of that slot's row with that see row, exactly as "Belief" specifies for one row (bitwise the row
 *      s2d_match_belief_scan writes for the same see row and flag).  The reset flag is the match's done of the previous cycle; for the first
 *      cycle of a launch it is the engine's done plane (S2DMatchBuffers.done) as the launch finds it.  Slots of belief_mask outside
 *      row_mask are not touched.  After a launch the state buffer holds every row_mask slot's belief after the start-of-cycle see
 *      row of the launch's last cycle; it is read and written in every cycle, for valid matches only.
 *   3. Network.  For every slot of slot_mask, on the slot's belief row (192 words): the logits of step 2 of "See policy slots"
 *      (same layout of params, same k-ascending fmaf order, f = relu or tanh_spec).  head 1: step 3 of "See policy slots" (the
 *      categorical head, *deterministic, logp) on the same Philox words.  head 0: the first-maximum argmax and the epsilon
 *      exploration of "See network" (stream S2D_MATCH_ST_NET, block = slot, *epsilon read when the kernel runs); activation 0 only;
 *      its logp is 0.
 *   4. Act.  (cmd, a, b) = table[index][0..2] into the body cycle, table[index][3..4] into the vision step of step 4 of "See
 *      network"; every other slot as there.
 * The kernel OWNS the belief update of its row_mask slots as it owns the vision step: the caller must not also call
 * s2d_match_belief_scan on those rows for cycles it runs.  Note the order: the kernel updates the belief BEFORE the body cycle (with
 * the start-of-cycle row, the row the network acts on); a per-step loop that calls s2d_match_belief_scan after each step holds the
 * same rows one call later.  The engine keeps the pointers (params, the head's word, table, planes, belief), not copies; prm and
 * belief_prm are copied at the call.
 * Not offered: a belief network as the in-kernel opponent of an environment that updates the same buffer after the cycle (two
 * conventions on one buffer); a record-only belief network (slot_mask == 0: a see record and s2d_match_belief_scan give that); a
 * second belief role; the agent reward.
 * s2d_match_kernel_name ends in "belief network>" while one is set. */
typedef struct S2DMatchBeliefNet {
  int32_t h1, h2, n_actions;      /* h1, h2 in {16, 32, 48, 64}; 1 <= K <= 64 */
  uint32_t slot_mask;             /* bits 0..21, not empty, inside belief_mask */
  const float *params;            /* W1[h1][192], b1, W2[h2][h1], b2, W3[K][h2], b3; device, 16-byte aligned */
  const float *table;             /* device float[K][5]: command, a, b, TurnNeck moment, ChangeView code */
  S2DVisionParams prm;            /* copied at the call */
  S2DMatchVision vis;             /* the caller's three planes; the engine keeps the pointers */
  int32_t head;                   /* 0 epsilon-greedy Q-network, 1 categorical policy */
  int32_t activation;             /* 0 relu, 1 tanh (tanh_spec) on both hidden layers; head 0: 0 */
  const float *epsilon;           /* head 0: device float, read when the kernel runs (head 1: not read) */
  const uint32_t *deterministic;  /* head 1: device word, read when the kernel runs: != 0 -> greedy (head 0: not read) */
  S2DBeliefParams belief_prm;     /* copied at the call */
  float *belief;                  /* device float[N][popcount(belief_mask)][S2D_BELIEF_DIM], 16-byte aligned; the engine keeps the pointer */
  uint32_t belief_mask;           /* bits 0..21, not empty: the buffer's slots */
} S2DMatchBeliefNet;
/* net == NULL: clears the see network, whichever kind is set.  Errors (S2D_EINVAL, the engine unchanged): everything
 * s2d_match_set_see_policy_network rejects (the device word being the head's: epsilon or deterministic); head outside {0, 1}; head 0
 * with activation 1; a NULL or not 16-byte aligned belief; an empty belief_mask or bits above 21 in it; slot_mask not inside
 * belief_mask; parameters s2d_match_belief_validate rejects; an agent reward is set.  s2d_match_step, s2d_match_rollout,
 * s2d_match_rollout_ex, s2d_match_rollout_see and s2d_match_rollout_see_policy use the belief network when one is set (no belief
 * record; an obs_mask outside belief_mask, or a record overlapping the state buffer, is refused); s2d_match_rollout_net, s2d_match_rollout_policy and s2d_match_rollout_reward
 * return S2D_EINVAL as beside the see network. */
int s2d_match_set_belief_network(S2DMatchHandle h, const S2DMatchBeliefNet *net);
/* s2d_match_rollout_see_policy plus
 *   belief_out_dev  float[T][N][popcount(obs_mask)][S2D_BELIEF_DIM] or NULL (16-byte aligned), written as whole 64-byte lines: the
 *                   row the network acted on at cycle t, i.e. the belief after see row t.  see_out_dev and belief_out_dev share
 *                   obs_mask; either may be NULL.
 * Errors: as s2d_match_rollout_see_policy; no belief network set; obs_mask not inside belief_mask; an unaligned belief_out_dev; a
 * record overlapping the state buffer. */
int s2d_match_rollout_belief(S2DMatchHandle h, int n_steps, const float *actions_dev, const float *view_actions_dev,
                             const S2DMatchRollout *out, float *actions_out_dev, int32_t *net_index_out_dev, float *logp_out_dev,
                             uint32_t obs_mask, float *see_out_dev, float *belief_out_dev, void *stream);

/* Hearing: say and hear, an opt-in audio layer beside the vision and belief layers -- Say (idl/service.proto:549-574), AttentionTo /
 * AttentionToOf (:585-592), ServerParam player_say_msg_size, player_hear_max, player_hear_inc, player_hear_decay (:1511-1514) and
 * audio_cut_dist (:1520).  Restated from the published behaviour of rcssserver; like every 11v11 rule it is this project's own
 * restatement: PARITY TO RCSSSERVER UNPINNED.  The fp32 words below are the contract (the device equals tests/hear_ref.c bit for
 * bit).  The engine handle stores nothing of it: all state is in caller-owned planes, an engine that never calls these functions is
 * byte for byte the engine without them.  Deviations: at most ONE message per side and cycle is delivered, even where hear_max /
 * hear_decay would allow more (the capacity still tallies); the draw among several speakers is per listener, not one shuffle per
 * cycle; a player does not hear itself; no coach; a message reaches the listener one step after it was said (the step that follows
 * the body step it was given with) and is never kept longer.  A message is say_msg_size symbols, each one of say_levels levels on
 * [-1, 1]: rcssserver's 10 characters of a 73-character alphabet kept as numbers -- the same channel capacity, no string codec.
 *
 * Parameters (doubles, each rounded to fp32 or to int once):
 *   audio_cut_dist  50   finite, >= 0: a speaker further away is not heard
 *   hear_max        1    whole, 1 .. 1e6: the largest hear capacity
 *   hear_inc        1    whole, 0 .. 1e6: what a capacity gains per cycle
 *   hear_decay      1    whole, 1 .. 1e6: what a delivered message costs
 *   say_msg_size    10   whole, 1 .. S2D_SAY_WORDS: payload words delivered; the others arrive as +0
 *   say_levels      73   odd whole, 3 .. 4097: half = the float of (say_levels - 1) / 2, inv_half = the float of the double 1 / half */
#define S2D_HEAR_DIM 32            /* float32 words per listener: 128 B, two lines of 64 B; see row + hear row = 224 words */
#define S2D_HEAR_RECORD 16         /* words of one record: ours at [0, 16), theirs at [16, 32) */
#define S2D_SAY_WORDS 10           /* payload words of a message */
#define S2D_SAY_ROW 12             /* words of a say row: said, attention command, payload */
#define S2D_MATCH_ST_HEAR 9        /* Philox stream id of the hear draws */
typedef struct S2DHearParams {
  double audio_cut_dist, hear_max, hear_inc, hear_decay, say_msg_size, say_levels;
} S2DHearParams;
void s2d_match_hear_default_params(S2DHearParams *prm);
/* Errors: NULL; a value outside the rule above (non-finite values included). */
int s2d_match_hear_validate(const S2DHearParams *prm);

/* The hear state: caller-owned device planes.  The three int32 planes are [N][24] (slot = player; slots 22, 23 are padding), 4-byte
 * aligned.  Own-frame slots are the see rows': the listener's team is 0..10, the other team 11..21 (the raw slot for the left
 * team, (slot + 11) % 22 for the right team).
 * A hear row is two records of S2D_HEAR_RECORD words, ours (the listener's team) then theirs; integers and flags as float values:
 *   0       heard (0 / 1)
 *   1       sender: own index + 1 (1..11) for a teammate; +0 in the theirs record -- opponents' numbers are not heard
 *   2       dir: the direction the message came from, relative to the face, whole degrees
 *   3       missed: the count of candidates not delivered
 *   4       the side's capacity after the step
 *   5       attention, ours record only: 0 for none, else own-frame slot + 1; +0 in the theirs record
 *   6..15   payload */
typedef struct S2DMatchHear {
  int32_t *cap_our, *cap_opp;   /* hear capacities for the listener's team and for the other team */
  int32_t *attention;           /* -1 for none, otherwise an own-frame slot 0..21; any other value reads as -1 */
  float *hear;                  /* float[N][22][S2D_HEAR_DIM], 16-byte aligned */
} S2DMatchHear;
/* For the masked matches (mask_dev uint8[N], NULL = all): caps = hear_max and attention = -1 in every slot of the three planes; every
 * word of the 22 hear rows +0, then word 4 of both records = hear_max (the reset row).
 * Errors (S2D_EINVAL, nothing written): invalid parameters, NULL or unaligned planes, a hear plane overlapping another plane. */
int s2d_match_hear_reset(S2DMatchHandle h, const S2DHearParams *prm, const S2DMatchHear *hear, const uint8_t *mask_dev, void *stream);
/* One cycle of hearing; call it once after each body step, beside s2d_match_vision_step.
 *   say_dev   float[N][22][S2D_SAY_ROW] (raw slots), 16-byte aligned, or NULL = nobody speaks or changes attention.  It holds what
 *             the players said with the body step just taken.
 *               word 0       said: nonzero and not NaN means said (-0 is zero)
 *               word 1       attention command: -1 switches attention off; a whole k in 1..22 attends own-frame slot k - 1, except
 *                            that the listener's own slot keeps; 0, NaN and every other value keep
 *               words 2..11  payload
 *   neck_dev  the vision layer's neck plane float[N][24], 4-byte aligned, or NULL = every neck +0
 *   done_dev  uint8[N] or NULL
 * Listener p of match e, on the current (post-step) engine state, in this order:
 *   1. done_dev[e] != 0: p's three plane words and row become the reset state and nothing below happens (a message does not cross
 *      a restart).
 *   2. otherwise, p sent off (card == S2D_CARD_RED): the three plane words are kept as they are, the row is all +0, and nothing
 *      below happens.
 *   3. p's attention command is applied (a stored attention outside -1..21 first reads as -1).
 *   4. for both sides: a cap outside [0, hear_max] reads as hear_max; cap = min(cap + hear_inc, hear_max).
 *   5. candidates of side s (ours: p's team; theirs: the other): every j != p of that side with card < S2D_CARD_RED who said, with
 *      d = hypot2(dx, dy) <= audio_cut_dist; dx = x_j - x_p, dy = y_j - y_p on the own-frame values (positions times sgn), so that
 *      mirrored states give the mirrored listener bitwise the same row whenever no draw decides.
 *   6. if cap_s >= hear_decay and side s has a candidate, the listener hears one:
 *        the winner is the attended slot if it is a candidate of this side; otherwise the candidate with the smallest
 *        (u_j, own-frame slot), u_j = w.x >> 8 of the Philox block with counter = the match's tick as the state holds it, stream
 *        S2D_MATCH_ST_HEAR, block = p * 24 + j (raw slots), the random policy's keys;
 *        cap_s -= hear_decay; heard = 1; sender as above; missed = candidates - 1;
 *        dir = d == 0 ? 0 : rintf(norm_deg_any(atan2_deg(dy, dx) - face)), face = norm_deg_any(body + neck) with the own-frame body;
 *        payload word i < say_msg_size: v NaN: +0; otherwise rintf(clamp(v, -1, 1) * half) * inv_half (clamp as in
 *        s2d_match_vision_step; a quantised word may be -0); payload word i >= say_msg_size: +0.
 *      otherwise (no capacity or no candidate): heard = 0, missed = the candidate count, sender, dir and payload +0.
 *   7. words 4 and 5 of both records are written and the three plane words stored.
 * The row is a pure function of state, planes, say rows and tick.  Reads x, y, body, card and tick of the engine; writes the four
 * planes of `hear` only.
 * Errors (S2D_EINVAL, nothing written): invalid parameters; NULL or unaligned planes; an unaligned say_dev or neck_dev; a plane of
 * `hear` overlapping another plane of it, say_dev, neck_dev or done_dev. */
int s2d_match_hear_step(S2DMatchHandle h, const S2DHearParams *prm, const S2DMatchHear *hear, const float *neck_dev,
                        const float *say_dev, const uint8_t *done_dev, void *stream);

/* Which instantiation of the cycle kernel this engine launches: "...<stock>" when its configuration equals
 * s2d_match_default_config() in every rule / physics word (those are compile-time constants there), "...<general>" otherwise
 * (same arithmetic, parameters read at run time; S2D_MATCH_GENERAL_KERNEL=1 in the environment selects it regardless).  Seed,
 * env_id_offset, auto_reset, noise and the PlayerTypes do not matter for the choice.  With a controller table, a network, a see
 * network, a see policy or a belief network set the name ends in "controllers>", "network>", "see network>", "see policy network>"
 * or "belief network>". */
const char *s2d_match_kernel_name(S2DMatchHandle h);

#ifdef __cplusplus
}
#endif
#endif /* S2D_MATCH_H_ */
