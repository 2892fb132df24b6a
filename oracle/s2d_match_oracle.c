/*
 * s2d_match_oracle.c -- CPU ORACLE of the 11v11 match engine.  TEST INFRASTRUCTURE ONLY
 * (same rules as s2d_oracle.c: only tests/, smoke() and bench.py's cpu_baseline may load it).
 *
 * The reference holds no Python for an 11v11 task: everything here restates rcssserver's
 * published match model (EXT) -- dash / turn / kick / tackle, stamina,
 * movement, player-player and player-ball collisions, goals, ball-out restarts (kick-in,
 * corner, goal kick), a basic offside rule, kick-off, half time, time over -- in the
 * simplified form documented in DESIGN.md section 10.  PARITY UNPINNED against a real
 * rcssserver; pinned by the hand-derived scenarios of tests/test_match_oracle.py.
 *
 * One source of truth for the HIP kernels: gym-soccer-2d-env_amd/csrc/s2d_match.hip must
 * reproduce every fp32 word and integer of this file bit for bit (same deterministic math
 * spec as the reach_ball path).
 */
#include "s2d_oracle_common.h"
#include "../include/s2d_match.h"

#define API __attribute__((visibility("default")))
#define NP S2D_MATCH_PLAYERS
#define NOBJ (NP + 1)
#define BALL S2D_MATCH_BALL

enum { ST_TACKLE = 4, ST_CATCH = 5, ST_TYPES = 6 };
enum { SIDE_NONE = 0, SIDE_LEFT = 1, SIDE_RIGHT = 2 };

typedef struct MP {
  REAL half_l, half_w, player_size, ball_size, player_decay, ball_decay, player_rand, ball_rand;
  REAL player_speed_max, player_speed_max2, player_accel_max, player_accel_max2, ball_speed_max, ball_speed_max2;
  REAL ball_accel_max, ball_accel_max2, inertia_moment;
  REAL stamina_max, stamina_inc_max, stamina_capacity, extra_stamina;
  REAL recover_init, recover_dec_thr_value, recover_min, recover_dec;
  REAL effort_init, effort_dec_thr_value, effort_min, effort_dec, effort_inc_thr_value, effort_inc;
  REAL dash_power_rate, max_dash_power, min_dash_power, max_dash_angle, min_dash_angle;
  REAL dash_angle_step, inv_dash_angle_step, side_dash_rate, back_dash_rate, max_moment, min_moment;
  REAL collision_vel_rate;
  REAL kick_power_rate, kickable_area, kickable_margin, inv_kickable_margin, kick_rand, max_power, min_power, inv_max_power;
  REAL tackle_dist, tackle_back_dist, tackle_width, tackle_power_rate, max_tackle_power, max_back_tackle_power;
  REAL goal_half_width, offside_area2, free_kick_distance, inv_speed_decay;
  int tackle_cycles, half_time_cycles, nr_normal_halfs, drop_ball_time, use_offside, catch_ban_cycle, goalie_max_moves;
  int after_goal_wait;
  int kick_off_wait, back_passes, free_kick_faults;
  int stopped_clock, announce_wait, foul_cycles; REAL foul_detect_probability;
  int nr_extra_halfs, extra_half_cycles, golden_goal;
  int penalty_shoot_outs, pen_before_setup_wait, pen_ready_wait, pen_taken_wait, pen_nr_kicks, pen_max_extra_kicks; REAL pen_spot_x;
  int pen_allow_mult_kicks, pen_random_winner;
  int illegal_defense_number, illegal_defense_duration; REAL ill_x, ill_half_w;   /* the strip: |x| > ill_x on the own side, |y| < ill_half_w */
  REAL catch_half_w, catch_probability, max_catch_angle, min_catch_angle, pen_x, pen_half_w;
  uint64_t seed; int64_t env_id_offset; int auto_reset, noise;
  /* heterogeneous players: the parameters of every player slot's PlayerType (idl/service.proto:1697-1732) */
  struct PT {
    REAL player_speed_max, player_speed_max2, stamina_inc_max, player_decay, inertia_moment, dash_power_rate, player_size;
    REAL kickable_margin, inv_kickable_margin, kickable_area, kick_rand, extra_stamina, effort_max, effort_min;
    REAL kick_power_rate, catch_len;
  } pt[S2D_MATCH_PLAYERS];
} MP;
typedef struct PT PT;

static void mp_from_config(const S2DMatchConfig *c, MP *p) {
  const S2DServerParams *s = &c->sp; const S2DMatchParams *m = &c->mp;
  p->half_l = (REAL)s->pitch_half_length; p->half_w = (REAL)s->pitch_half_width;
  p->player_size = (REAL)s->player_size; p->ball_size = (REAL)s->ball_size;
  p->player_decay = (REAL)s->player_decay; p->ball_decay = (REAL)s->ball_decay;
  p->player_rand = (REAL)s->player_rand; p->ball_rand = (REAL)s->ball_rand;
  p->player_speed_max = (REAL)s->player_speed_max; p->player_speed_max2 = p->player_speed_max * p->player_speed_max;
  p->player_accel_max = (REAL)s->player_accel_max; p->player_accel_max2 = p->player_accel_max * p->player_accel_max;
  p->ball_speed_max = (REAL)s->ball_speed_max; p->ball_speed_max2 = p->ball_speed_max * p->ball_speed_max;
  p->ball_accel_max = (REAL)s->ball_accel_max; p->ball_accel_max2 = p->ball_accel_max * p->ball_accel_max;
  p->inertia_moment = (REAL)s->inertia_moment;
  p->stamina_max = (REAL)s->stamina_max; p->stamina_inc_max = (REAL)s->stamina_inc_max;
  p->stamina_capacity = (REAL)s->stamina_capacity; p->extra_stamina = (REAL)s->extra_stamina;
  p->recover_init = (REAL)s->recover_init; p->recover_dec_thr_value = (REAL)(s->recover_dec_thr * s->stamina_max);
  p->recover_min = (REAL)s->recover_min; p->recover_dec = (REAL)s->recover_dec;
  p->effort_init = (REAL)s->effort_init; p->effort_dec_thr_value = (REAL)(s->effort_dec_thr * s->stamina_max);
  p->effort_min = (REAL)s->effort_min; p->effort_dec = (REAL)s->effort_dec;
  p->effort_inc_thr_value = (REAL)(s->effort_inc_thr * s->stamina_max); p->effort_inc = (REAL)s->effort_inc;
  p->dash_power_rate = (REAL)s->dash_power_rate; p->max_dash_power = (REAL)s->max_dash_power;
  p->min_dash_power = (REAL)s->min_dash_power; p->max_dash_angle = (REAL)s->max_dash_angle;
  p->min_dash_angle = (REAL)s->min_dash_angle; p->dash_angle_step = (REAL)s->dash_angle_step;
  p->inv_dash_angle_step = s->dash_angle_step > 0 ? (REAL)(1.0 / s->dash_angle_step) : R(0.0);
  p->side_dash_rate = (REAL)s->side_dash_rate; p->back_dash_rate = (REAL)s->back_dash_rate;
  p->max_moment = (REAL)s->max_moment; p->min_moment = (REAL)s->min_moment;
  p->collision_vel_rate = (REAL)s->collision_vel_rate;
  p->kick_power_rate = (REAL)m->kick_power_rate; p->kickable_margin = (REAL)m->kickable_margin;
  p->inv_kickable_margin = (REAL)(1.0 / m->kickable_margin);
  p->kickable_area = p->player_size + p->ball_size + p->kickable_margin;
  p->kick_rand = (REAL)m->kick_rand; p->max_power = (REAL)m->max_power; p->min_power = (REAL)m->min_power;
  p->inv_max_power = (REAL)(1.0 / m->max_power);
  p->tackle_dist = (REAL)m->tackle_dist; p->tackle_back_dist = (REAL)m->tackle_back_dist;
  p->tackle_width = (REAL)m->tackle_width; p->tackle_power_rate = (REAL)m->tackle_power_rate;
  p->max_tackle_power = (REAL)m->max_tackle_power; p->max_back_tackle_power = (REAL)m->max_back_tackle_power;
  p->goal_half_width = (REAL)(m->goal_width * 0.5);
  p->offside_area2 = (REAL)(m->offside_active_area_size * m->offside_active_area_size);
  p->free_kick_distance = (REAL)m->free_kick_distance;
  p->inv_speed_decay = (REAL)(1.0 / (s->ball_speed_max * s->ball_decay));
  p->tackle_cycles = m->tackle_cycles; p->half_time_cycles = m->half_time_cycles;
  p->nr_normal_halfs = m->nr_normal_halfs; p->drop_ball_time = m->drop_ball_time; p->use_offside = m->use_offside;
  p->catch_ban_cycle = m->catch_ban_cycle; p->goalie_max_moves = m->goalie_max_moves;
  p->after_goal_wait = m->after_goal_wait;
  p->kick_off_wait = m->kick_off_wait; p->back_passes = m->back_passes; p->free_kick_faults = m->free_kick_faults;
  p->stopped_clock = m->stopped_clock; p->announce_wait = m->announce_wait; p->foul_cycles = m->foul_cycles;
  p->foul_detect_probability = (REAL)m->foul_detect_probability;
  p->nr_extra_halfs = m->nr_extra_halfs; p->extra_half_cycles = m->extra_half_cycles; p->golden_goal = m->golden_goal;
  p->penalty_shoot_outs = m->penalty_shoot_outs; p->pen_before_setup_wait = m->pen_before_setup_wait; p->pen_ready_wait = m->pen_ready_wait;
  p->pen_taken_wait = m->pen_taken_wait; p->pen_nr_kicks = m->pen_nr_kicks; p->pen_max_extra_kicks = m->pen_max_extra_kicks;
  p->pen_spot_x = (REAL)(s->pitch_half_length - m->pen_dist_x);
  p->pen_allow_mult_kicks = m->pen_allow_mult_kicks; p->pen_random_winner = m->pen_random_winner != 0;
  p->illegal_defense_number = m->illegal_defense_number; p->illegal_defense_duration = m->illegal_defense_duration;
  p->ill_x = (REAL)(s->pitch_half_length - m->illegal_defense_dist_x); p->ill_half_w = (REAL)(m->illegal_defense_width * 0.5);
  p->catch_half_w = (REAL)(m->catch_area_w * 0.5); p->catch_probability = (REAL)m->catch_probability;
  p->max_catch_angle = (REAL)m->max_catch_angle; p->min_catch_angle = (REAL)m->min_catch_angle;
  p->pen_x = (REAL)(s->pitch_half_length - m->penalty_area_length); p->pen_half_w = (REAL)m->penalty_area_half_width;
  p->seed = c->seed; p->env_id_offset = c->env_id_offset; p->auto_reset = c->auto_reset; p->noise = c->noise;
  for (int i = 0; i < S2D_MATCH_PLAYERS; ++i) {
    int id = c->player_type_id[i];
    if (id < 0 || id >= S2D_MATCH_PLAYER_TYPES) id = 0;
    const S2DPlayerType *t = &c->player_types[id];
    PT *q = &p->pt[i];
    q->player_speed_max = (REAL)t->player_speed_max; q->player_speed_max2 = q->player_speed_max * q->player_speed_max;
    q->stamina_inc_max = (REAL)t->stamina_inc_max; q->player_decay = (REAL)t->player_decay;
    q->inertia_moment = (REAL)t->inertia_moment; q->dash_power_rate = (REAL)t->dash_power_rate;
    q->player_size = (REAL)t->player_size; q->kickable_margin = (REAL)t->kickable_margin;
    q->inv_kickable_margin = (REAL)(1.0 / t->kickable_margin);
    q->kickable_area = q->player_size + p->ball_size + q->kickable_margin;
    q->kick_rand = (REAL)t->kick_rand; q->extra_stamina = (REAL)t->extra_stamina;
    q->effort_max = (REAL)t->effort_max; q->effort_min = (REAL)t->effort_min;
    q->kick_power_rate = (REAL)t->kick_power_rate;
    q->catch_len = (REAL)(m->catchable_area_l * t->catchable_area_l_stretch);
  }
}

typedef struct Obj { REAL x, y, vx, vy, body, stamina, effort, recovery, capacity; int32_t tackle, catch_ban, card; } Obj;
typedef struct Match {
  Obj o[NOBJ];
  int32_t cycle, mode, mode_side, score_left, score_right, last_touch_side, setplay_timer, offside_mask;
  int32_t ball_holder, goalie_moves;    /* 1 + index of the goalie holding a caught ball (0 = nobody), remaining moves */
  int32_t set_play_taker;               /* 1 + index of the player who put the ball into play from the last set play and whom
                                           nobody else has touched the ball after (0 = nobody): a second touch is a free-kick fault */
  int32_t last_kicker;                  /* 1 + index of the last player who moved the ball with a Kick command and whom no other
                                           touch (tackle, collision) followed (0 = nobody): the back-pass rule */
  int32_t stopped_cycle;                /* WorldModel.stoped_cycle (idl/service.proto:333): cycles the clock has been standing still */
  int32_t tick;                         /* cycles since the reset, stopped ones included: the Philox counter of every draw */
  REAL reward_left; uint8_t done; int32_t nearest_left, nearest_right;
} Match;

static int side_of(int i) { return i < 11 ? SIDE_LEFT : SIDE_RIGHT; }
static int other_side(int s) { return s == SIDE_LEFT ? SIDE_RIGHT : SIDE_LEFT; }
/* TimeOver, and the two modes only an operator sets (Pause, Human: idl/service.proto:280-281): nobody acts, nothing is decided, the clock stands */
static int is_halted(int mode) { return mode == S2D_GM_TIME_OVER || mode == S2D_GM_PAUSE || mode == S2D_GM_HUMAN; }
static int is_setplay(int mode) { return mode != S2D_GM_PLAY_ON && !is_halted(mode); }
/* announcements: a dead ball named after the offending side; after announce_wait cycles the referee awards the restart */
static int is_announcement(int mode) {
  return mode == S2D_GM_OFF_SIDE || mode == S2D_GM_BACK_PASS || mode == S2D_GM_FREE_KICK_FAULT || mode == S2D_GM_CATCH_FAULT ||
         mode == S2D_GM_FOUL_CHARGE || mode == S2D_GM_ILLEGAL_DEFENSE ||
         mode == S2D_GM_FOUL_PUSH || mode == S2D_GM_FOUL_MULTIPLE_ATTACKER || mode == S2D_GM_FOUL_BALL_OUT;   /* (an operator's calls) */
}
/* modes in which nobody may play the ball */
/* the shoot-out's modes (idl/service.proto:290-297) */
static int is_penalty(int mode) {
  return mode == S2D_GM_PENALTY_SETUP || mode == S2D_GM_PENALTY_READY || mode == S2D_GM_PENALTY_TAKEN || mode == S2D_GM_PENALTY_MISS ||
         mode == S2D_GM_PENALTY_SCORE || mode == S2D_GM_PENALTY_ONFIELD || mode == S2D_GM_PENALTY_FOUL;
}
static int is_period_end(int mode) { return mode == S2D_GM_FIRST_HALF_OVER || mode == S2D_GM_EXTEND_HALF; }   /* "half_time", "time_extended" */
static int ball_dead(int mode) {
  return mode == S2D_GM_AFTER_GOAL || mode == S2D_GM_BEFORE_KICK_OFF || is_period_end(mode) || mode == S2D_GM_GOALIE_CATCH ||
         is_announcement(mode) || (is_penalty(mode) && mode != S2D_GM_PENALTY_READY && mode != S2D_GM_PENALTY_TAKEN);
}
/* modes in which the clock stands still (with stopped_clock): WorldModel.cycle keeps its value, stoped_cycle counts */
static int clock_stands(int mode) {
  return mode == S2D_GM_BEFORE_KICK_OFF || mode == S2D_GM_AFTER_GOAL || is_period_end(mode) || is_halted(mode) ||
         is_announcement(mode) || is_penalty(mode);
}
/* where a sent-off player waits: beside the halfway line, outside the pitch, one spot per uniform number */
static void park_sent_off(const MP *p, Obj *o, int i) {
  o->x = R(0.0); o->y = (side_of(i) == SIDE_LEFT ? R(-1.0) : R(1.0)) * (p->half_w + R(6.0) + R(1.5) * (REAL)(i % 11));
  o->vx = R(0.0); o->vy = R(0.0);
}

/* kick-off formation of the left team (right team mirrored); DESIGN.md section 10 */
static const REAL FORM_X[11] = {R(-50.0), R(-35.0), R(-35.0), R(-35.0), R(-35.0), R(-20.0), R(-20.0), R(-20.0), R(-20.0), R(-10.5), R(-10.5)};
static const REAL FORM_Y[11] = {R(0.0), R(-20.0), R(-7.0), R(7.0), R(20.0), R(-22.0), R(-8.0), R(8.0), R(22.0), R(-6.0), R(6.0)};

static void place_formation(Match *m, int kickoff_side) {
  for (int i = 0; i < NP; ++i) {
    int k = i % 11; int left = i < 11;
    Obj *o = &m->o[i];
    if (o->card >= S2D_CARD_RED) continue;               /* sent off: stays where he was parked */
    o->x = left ? FORM_X[k] : -FORM_X[k]; o->y = FORM_Y[k];
    o->vx = R(0.0); o->vy = R(0.0); o->body = left ? R(0.0) : R(180.0); o->tackle = 0; o->catch_ban = 0;
  }
  /* the taker stands at the ball */
  if (kickoff_side == SIDE_LEFT) { if (m->o[10].card < S2D_CARD_RED) { m->o[10].x = R(-0.4); m->o[10].y = R(0.0); } }
  else { if (m->o[21].card < S2D_CARD_RED) { m->o[21].x = R(0.4); m->o[21].y = R(0.0); } }
  Obj *b = &m->o[BALL]; b->x = R(0.0); b->y = R(0.0); b->vx = R(0.0); b->vy = R(0.0);
}
static void recover_all(const MP *p, Match *m, int with_capacity) {
  for (int i = 0; i < NP; ++i) {
    Obj *o = &m->o[i];
    o->stamina = p->stamina_max; o->effort = p->pt[i].effort_max; o->recovery = p->recover_init;
    if (with_capacity) o->capacity = p->stamina_capacity;
  }
}
static void match_reset(const MP *p, Match *m) {
  memset(m, 0, sizeof *m);
  recover_all(p, m, 1);
  place_formation(m, SIDE_LEFT);
  m->mode = p->kick_off_wait > 0 ? S2D_GM_BEFORE_KICK_OFF : S2D_GM_KICK_OFF; m->mode_side = SIDE_LEFT;
  m->nearest_left = 10; m->nearest_right = 20;
}

static REAL clampr(REAL v, REAL lo, REAL hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* Player::dash / Player::turn -- identical arithmetic to s2d_oracle.c (appendix A) */
static void m_dash(const MP *p, const PT *t, Obj *o, REAL power, REAL dir, REAL *ax, REAL *ay) {
  power = clampr(power, p->min_dash_power, p->max_dash_power);
  dir = clampr(dir, p->min_dash_angle, p->max_dash_angle);
  if (p->dash_angle_step > R(0.0)) dir = p->dash_angle_step * R(rint)(DIVC(dir, p->dash_angle_step, p->inv_dash_angle_step));
  int back = power < R(0.0);
  REAL need = back ? power * R(-2.0) : power;
  REAL avail = o->stamina + t->extra_stamina;
  if (need > avail) need = avail;
  REAL st = o->stamina - need;
  o->stamina = st > R(0.0) ? st : R(0.0);
  power = back ? need / R(-2.0) : need;
  REAL ad = R(fabs)(dir);
  REAL dir_rate = ad > R(90.0)
      ? p->back_dash_rate - ((p->back_dash_rate - p->side_dash_rate) * (R(1.0) - DIVC(ad - R(90.0), R(90.0), 0.011111111111111112f)))
      : p->side_dash_rate + ((R(1.0) - p->side_dash_rate) * (R(1.0) - DIVC(ad, R(90.0), 0.011111111111111112f)));
  dir_rate = clampr(dir_rate, R(0.0), R(1.0));
  REAL acc = R(fabs)(o->effort * power * dir_rate * t->dash_power_rate);
  if (back) dir += R(180.0);
  REAL sn, cs;
  sincos_deg(norm_deg(o->body + dir), &sn, &cs);
  *ax = acc * cs; *ay = acc * sn;
}
static void m_turn(const MP *p, const PT *t, Obj *o, REAL moment, REAL noise_u) {
  moment = clampr(moment, p->min_moment, p->max_moment);
  REAL speed = hypot2(o->vx, o->vy);
  REAL f = R(1.0);
  if (p->noise) f = R(1.0) + (noise_u * R(2.0) - R(1.0)) * p->player_rand;
  o->body = norm_deg(o->body + f * moment / (R(1.0) + t->inertia_moment * speed));
}
/* Player::kick -- appendix A "Kick(power, dir)".  Returns 1 if the ball was kickable. */
static int m_kick(const MP *p, const PT *t, const Obj *o, const Obj *b, REAL power, REAL dir, REAL u_mag, REAL u_ang, REAL *kx, REAL *ky) {
  REAL dx = b->x - o->x, dy = b->y - o->y;
  REAL dist = hypot2(dx, dy);
  if (!(dist <= t->kickable_area)) return 0;
  power = clampr(power, p->min_power, p->max_power);
  dir = clampr(dir, R(-180.0), R(180.0));
  REAL dir_diff = R(fabs)(norm_deg(atan2_deg(dy, dx) - o->body));
  REAL dist_ball = dist - t->player_size - p->ball_size;
  REAL eff = power * t->kick_power_rate * (R(1.0) - R(0.25) * DIVC(dir_diff, R(180.0), 0.005555555555555556f)
                                            - R(0.25) * DIVC(dist_ball, t->kickable_margin, t->inv_kickable_margin));
  REAL sn, cs;
  sincos_deg(norm_deg(o->body + dir), &sn, &cs);
  REAL ax = eff * cs, ay = eff * sn;
  if (p->noise) {
    REAL pos_rate = R(0.5) + R(0.25) * (DIVC(dir_diff, R(180.0), 0.005555555555555556f) + DIVC(dist_ball, t->kickable_margin, t->inv_kickable_margin));
    REAL speed_rate = R(0.5) + R(0.5) * (hypot2(b->vx, b->vy) * p->inv_speed_decay);
    REAL max_rand = t->kick_rand * (power * p->inv_max_power) * (pos_rate + speed_rate);
    REAL mag = u_mag * max_rand;
    REAL s2, c2;
    sincos_deg(u_ang * R(360.0) - R(180.0), &s2, &c2);
    ax += mag * c2; ay += mag * s2;
  }
  *kx = ax; *ky = ay;
  return 1;
}
/* Player::tackle -- appendix A.  `u` = uniform draw; foul = Tackle.foul (idl/service.proto:401): exponent foul_exponent = 10
 * instead of tackle_exponent = 6.  Returns 1 on success. */
static int m_tackle(const MP *p, const Obj *o, const Obj *b, REAL dir, REAL u, int foul, REAL *kx, REAL *ky) {
  REAL dx = b->x - o->x, dy = b->y - o->y;
  REAL sn, cs;
  sincos_deg(o->body, &sn, &cs);
  REAL rx = dx * cs + dy * sn;                /* ball in the body frame */
  REAL ry = dy * cs - dx * sn;
  REAL d = rx > R(0.0) ? p->tackle_dist : p->tackle_back_dist;
  REAL tx = d > R(0.0) ? R(fabs)(rx) / d : (rx == R(0.0) ? R(0.0) : R(1.0e9));
  REAL ty = R(fabs)(ry) / p->tackle_width;
  REAL tx2 = tx * tx, ty2 = ty * ty;
  REAL fail = tx2 * tx2 * tx2 + ty2 * ty2 * ty2;    /* exponent 6 */
  if (foul) { REAL tx4 = tx2 * tx2, ty4 = ty2 * ty2; fail = tx4 * tx4 * tx2 + ty4 * ty4 * ty2; }   /* exponent 10 */
  if (!(u >= fail)) return 0;
  dir = clampr(dir, R(-180.0), R(180.0));
  REAL ang_ball = R(fabs)(norm_deg(atan2_deg(dy, dx) - o->body));
  REAL eff = (p->max_back_tackle_power + (p->max_tackle_power - p->max_back_tackle_power) * (R(1.0) - DIVC(R(fabs)(dir), R(180.0), 0.005555555555555556f)))
             * p->tackle_power_rate * (R(1.0) - R(0.5) * DIVC(ang_ball, R(180.0), 0.005555555555555556f));
  REAL s2, c2;
  sincos_deg(norm_deg(o->body + dir), &s2, &c2);
  *kx = eff * c2; *ky = eff * s2;
  return 1;
}
/* Player::goalieCatch -- the ball must lie in the catch rectangle (catchable_area_l * stretch long,
 * catch_area_w wide) rooted at the goalie and turned to body + dir; `u` = uniform draw (used when
 * catch_probability < 1).  Returns 1 if the goalie holds the ball. */
static int m_catch(const MP *p, const PT *t, const Obj *o, const Obj *b, REAL dir, REAL u) {
  dir = clampr(dir, p->min_catch_angle, p->max_catch_angle);
  REAL sn, cs;
  sincos_deg(norm_deg(o->body + dir), &sn, &cs);
  REAL dx = b->x - o->x, dy = b->y - o->y;
  REAL rx = dx * cs + dy * sn, ry = dy * cs - dx * sn;
  if (!(rx >= R(0.0) && rx <= t->catch_len && R(fabs)(ry) <= p->catch_half_w)) return 0;
  return u < p->catch_probability;
}
static void m_update_stamina(const MP *p, const PT *t, Obj *e) {
  if (e->stamina <= p->recover_dec_thr_value) {
    if (e->recovery > p->recover_min) { REAL r = e->recovery - p->recover_dec; e->recovery = r > p->recover_min ? r : p->recover_min; }
  }
  if (e->stamina <= p->effort_dec_thr_value) {
    if (e->effort > t->effort_min) { REAL f = e->effort - p->effort_dec; e->effort = f > t->effort_min ? f : t->effort_min; }
  }
  if (e->stamina >= p->effort_inc_thr_value) {
    if (e->effort < t->effort_max) { REAL f = e->effort + p->effort_inc; e->effort = f < t->effort_max ? f : t->effort_max; }
  }
  REAL inc = e->recovery * t->stamina_inc_max;
  REAL room = p->stamina_max - e->stamina;
  if (inc > room) inc = room;
  if (p->stamina_capacity >= R(0.0)) { if (inc > e->capacity) inc = e->capacity; }
  e->stamina += inc;
  if (e->stamina > p->stamina_max) e->stamina = p->stamina_max;
  if (p->stamina_capacity >= R(0.0)) { REAL c = e->capacity - inc; e->capacity = c > R(0.0) ? c : R(0.0); }
}
static void add_noise(REAL *vx, REAL *vy, REAL rnd, REAL u_mag, REAL u_ang) {
  REAL s = hypot2(*vx, *vy);
  REAL mag = u_mag * (rnd * s);
  REAL sn, cs;
  sincos_deg(u_ang * R(360.0) - R(180.0), &sn, &cs);
  *vx += mag * cs; *vy += mag * sn;
}

static void restart(Match *m, int mode, int side, REAL bx, REAL by) {
  Obj *b = &m->o[BALL];
  b->x = bx; b->y = by; b->vx = R(0.0); b->vy = R(0.0);
  m->mode = mode; m->mode_side = side; m->setplay_timer = 0; m->offside_mask = 0;
  m->set_play_taker = 0; m->last_kicker = 0;
}

/* ---- the penalty shoot-out (rcssserver's PenaltyRef restated; ServerParam.pen_*: idl/service.proto:1602-1613).  Its state lives in
 * the set-play word: bits 0-7 = 1 + taker, 12-15 / 16-19 kicks taken left / right, 20-23 / 24-27 goals left / right (include/s2d_match.h). */
static int pen_kicks(int w, int side) { return (w >> (side == SIDE_LEFT ? 12 : 16)) & 15; }
static int pen_goals(int w, int side) { return (w >> (side == SIDE_LEFT ? 20 : 24)) & 15; }
/* PenaltySetup_ for `side`: the referee places everybody (pen_coach_moves_players): the ball on the spot, the taker (index 10 downwards,
 * by the kicks his team has taken) 0.7 m behind it, the other team's goalie on the right goal line, the rest inside the centre circle */
static void pen_setup(const MP *p, Match *m, int side) {
  const int w = m->set_play_taker;
  const int taker = (side == SIDE_LEFT ? 0 : 11) + 10 - pen_kicks(w, side) % 11;
  const int goalie = side == SIDE_LEFT ? S2D_MATCH_GOALIE_RIGHT : S2D_MATCH_GOALIE_LEFT;
  for (int i = 0; i < NP; ++i) {
    Obj *o = &m->o[i];
    if (o->card >= S2D_CARD_RED) continue;               /* sent off: stays parked (a kick that falls to him is missed) */
    if (i == taker) { o->x = p->pen_spot_x - R(0.7); o->y = R(0.0); o->body = R(0.0); }
    else if (i == goalie) { o->x = p->half_l - R(1.0); o->y = R(0.0); o->body = R(180.0); }
    else { o->x = i < 11 ? R(-3.0) : R(3.0); o->y = R(-7.5) + R(1.5) * (REAL)(i % 11); }
    o->vx = R(0.0); o->vy = R(0.0);
  }
  Obj *b = &m->o[BALL]; b->x = p->pen_spot_x; b->y = R(0.0); b->vx = R(0.0); b->vy = R(0.0);
  m->mode = S2D_GM_PENALTY_SETUP; m->mode_side = side; m->setplay_timer = 0; m->offside_mask = 0; m->last_kicker = 0;
  m->set_play_taker = (w & ~0xff) | (taker + 1);
}
/* the kick of `side` is over: counted, announced (PenaltyScore_ / PenaltyMiss_), the ball is dead */
static void pen_result(Match *m, int side, int scored) {
  int w = m->set_play_taker;
  w += 1 << (side == SIDE_LEFT ? 12 : 16);
  if (scored) { w += 1 << (side == SIDE_LEFT ? 20 : 24); m->reward_left = side == SIDE_LEFT ? R(1.0) : R(-1.0); }
  m->set_play_taker = w;
  m->mode = scored ? S2D_GM_PENALTY_SCORE : S2D_GM_PENALTY_MISS; m->setplay_timer = 0;
  m->o[BALL].vx = R(0.0); m->o[BALL].vy = R(0.0);
}
/* is the shoot-out decided (or used up) after the kicks counted in w? */
static int pen_over(const MP *p, int w) {
  const int kl = pen_kicks(w, SIDE_LEFT), kr = pen_kicks(w, SIDE_RIGHT), gl = pen_goals(w, SIDE_LEFT), gr = pen_goals(w, SIDE_RIGHT);
  const int nr = p->pen_nr_kicks;
  if (kl <= nr && kr <= nr) {                            /* the regular kicks: over as soon as one side cannot catch up */
    if (gl > gr + (nr - kr) || gr > gl + (nr - kl)) return 1;
    if (kl == nr && kr == nr) return p->pen_max_extra_kicks <= 0;   /* (level: a lead was decided by the line above) */
    return 0;
  }
  if (kl == kr) return gl != gr || kl >= nr + p->pen_max_extra_kicks;   /* pairs of extra kicks */
  return 0;
}

typedef struct MatchStats { unsigned long long v[8]; } MatchStats;

/* what happened in a cycle (s2dmo_events; test coverage only, nothing of the match depends on it) */
enum { EV_KICK = 1, EV_TACKLE = 2, EV_CATCH = 4, EV_COLLIDE = 8, EV_BALL_COLLIDE = 16, EV_GOAL = 32 };

/* one cycle of one match; act = [22][3] {cmd, a, b} */
static void match_step(const MP *p, Match *m, uint64_t gid, const float *act, MatchStats *st, uint32_t *ev) {
  const uint32_t cyc = (uint32_t)m->tick;                /* Philox counter: cycles since the reset, stopped ones included */
  const int mode0 = m->mode, side0 = m->mode_side;
  Obj *b = &m->o[BALL];
  REAL x0[NOBJ], y0[NOBJ];
  for (int i = 0; i < NOBJ; ++i) { x0[i] = m->o[i].x; y0[i] = m->o[i].y; }
  m->reward_left = R(0.0); m->done = 0;
  int foul_by = -1, foul_victim = -1, foul_seen = 0;      /* an intentional foul of this cycle: tackler, victim, seen by the referee */
  const int pen = is_penalty(mode0);
  const int pen_taker = pen ? (m->set_play_taker & 0xff) - 1 : -1;
  const int pen_goalie = !pen ? -1 : side0 == SIDE_LEFT ? S2D_MATCH_GOALIE_RIGHT : S2D_MATCH_GOALIE_LEFT;

  /* 1. commands */
  REAL ax[NP], ay[NP], kx[NP], ky[NP];
  int kicked[NP], by_kick[NP];           /* by_kick: the impulse came from a Kick command (not a tackle) */
  int caught_by = -1, hold_move = -1;
  uint32_t nzb[4] = {0, 0, 0, 0};
  if (p->noise) draw(p->seed, gid, cyc, ST_NOISE, BALL, nzb);
  for (int i = 0; i < NP; ++i) {
    Obj *o = &m->o[i];
    const PT *t = &p->pt[i];
    ax[i] = ay[i] = kx[i] = ky[i] = R(0.0); kicked[i] = 0; by_kick[i] = 0;
    int cmd = (int)act[i * 3 + 0];
    REAL a = (REAL)act[i * 3 + 1], bb = (REAL)act[i * 3 + 2];
    if (o->tackle > 0 || is_halted(mode0) || o->card >= S2D_CARD_RED) cmd = S2D_MCMD_NONE;
    /* the shoot-out: the taker acts once the kick is ready, the defending goalie once it is taken, nobody else at all */
    if (pen && !((i == pen_taker && (mode0 == S2D_GM_PENALTY_READY || mode0 == S2D_GM_PENALTY_TAKEN)) ||
                 (i == pen_goalie && mode0 == S2D_GM_PENALTY_TAKEN))) cmd = S2D_MCMD_NONE;
    uint32_t nz[4] = {0, 0, 0, 0};                       /* x, y: movement noise; z, w: the command's noise (Turn: z; Kick: z, w) */
    if (p->noise) draw(p->seed, gid, cyc, ST_NOISE, (uint32_t)i, nz);
    /* set play: only the taking side plays the ball; after a goal nobody does */
    int may_touch = !is_setplay(mode0) || (side_of(i) == side0 && !ball_dead(mode0)) || (mode0 == S2D_GM_PENALTY_TAKEN && i == pen_goalie);
    if (cmd == S2D_MCMD_DASH) m_dash(p, t, o, a, bb, &ax[i], &ay[i]);
    else if (cmd == S2D_MCMD_TURN) m_turn(p, t, o, a, rnd_u01(nz[2]));
    else if (cmd == S2D_MCMD_CATCH) {
      /* goalies only, play_on only, not while banned; every attempt starts the ban */
      if ((i == S2D_MATCH_GOALIE_LEFT || i == S2D_MATCH_GOALIE_RIGHT) && (mode0 == S2D_GM_PLAY_ON || mode0 == S2D_GM_PENALTY_TAKEN) && o->catch_ban == 0) {
        REAL u = R(0.0);
        if (p->catch_probability < R(1.0)) { uint32_t w[4]; draw(p->seed, gid, cyc, ST_CATCH, (uint32_t)i, w); u = rnd_u01(w[0]); }
        o->catch_ban = p->catch_ban_cycle + 1;
        if (m_catch(p, t, o, b, a, u) && caught_by < 0) caught_by = i;
      }
    } else if (cmd == S2D_MCMD_MOVE) {
      /* Move(x, y) in the team's own frame (right team mirrored): before a kick-off anywhere in the own
       * half; while holding a caught ball, goalie_max_moves times inside the own penalty area */
      REAL sgn = side_of(i) == SIDE_LEFT ? R(1.0) : R(-1.0);
      int holds = mode0 == S2D_GM_FREE_KICK && m->ball_holder == i + 1 && m->goalie_moves > 0;
      if (mode0 == S2D_GM_KICK_OFF || mode0 == S2D_GM_AFTER_GOAL || mode0 == S2D_GM_BEFORE_KICK_OFF || holds) {
        REAL tx = clampr(a, -p->half_l, holds ? -p->pen_x : R(0.0));
        REAL ty = holds ? clampr(bb, -p->pen_half_w, p->pen_half_w) : clampr(bb, -p->half_w, p->half_w);
        o->x = sgn * tx; o->y = sgn * ty; o->vx = R(0.0); o->vy = R(0.0);
        if (holds) hold_move = i;
      }
    } else if (cmd == S2D_MCMD_KICK) {
      int ok = m_kick(p, t, o, b, a, bb, rnd_u01(nz[2]), rnd_u01(nz[3]), &kx[i], &ky[i]);
      if (ok && may_touch) { kicked[i] = 1; by_kick[i] = 1; st->v[4]++; } else { kx[i] = ky[i] = R(0.0); }
    } else if (cmd == S2D_MCMD_TACKLE) {
      uint32_t w[4];
      const int foul = bb != R(0.0);                      /* Tackle.foul */
      draw(p->seed, gid, cyc, ST_TACKLE, (uint32_t)i, w);
      int ok = m_tackle(p, o, b, a, rnd_u01(w[0]), foul, &kx[i], &ky[i]);
      o->tackle = p->tackle_cycles + 1;
      st->v[5]++;
      if (ok && may_touch) kicked[i] = 1; else { kx[i] = ky[i] = R(0.0); }
      /* FoulCharge_ (idl/service.proto:282): a successful INTENTIONAL tackle that goes through an opponent who has the ball
       * (kickable) inside the tackler's tackle area brings him down for foul_cycles; the referee sees it with
       * foul_detect_probability (second word of the tackle block).  Positions of the start of the cycle; the first such
       * tackler (lowest index) counts. */
      if (ok && foul && mode0 == S2D_GM_PLAY_ON && foul_by < 0) {
        REAL sn, cs;
        sincos_deg(m->o[i].body, &sn, &cs);
        const int o0 = side_of(i) == SIDE_LEFT ? 11 : 0;
        for (int j = o0; j < o0 + 11 && foul_victim < 0; ++j) {
          if (m->o[j].card >= S2D_CARD_RED) continue;
          if (!(hypot2(x0[BALL] - x0[j], y0[BALL] - y0[j]) <= p->pt[j].kickable_area)) continue;
          REAL dx = x0[j] - x0[i], dy = y0[j] - y0[i];
          REAL rx = dx * cs + dy * sn, ry = dy * cs - dx * sn;
          if (rx >= R(0.0) && rx <= p->tackle_dist && R(fabs)(ry) <= p->tackle_width) foul_victim = j;
        }
        if (foul_victim >= 0) { foul_by = i; foul_seen = rnd_u01(w[1]) < p->foul_detect_probability; }
      }
    }
    /* _inc of player i */
    if (cmd == S2D_MCMD_DASH) {
      REAL a2 = sq2(ax[i], ay[i]);
      if (a2 > p->player_accel_max2) { REAL k = p->player_accel_max / R(sqrt)(a2); ax[i] *= k; ay[i] *= k; }
      o->vx += ax[i]; o->vy += ay[i];
    }
    REAL s2 = sq2(o->vx, o->vy);
    if (s2 > t->player_speed_max2) { REAL k = t->player_speed_max / R(sqrt)(s2); o->vx *= k; o->vy *= k; }
    if (p->noise) add_noise(&o->vx, &o->vy, p->player_rand, rnd_u01(nz[0]), rnd_u01(nz[1]));
    o->x += o->vx; o->y += o->vy;
  }
  if (caught_by >= 0) { st->v[4]++; *ev |= EV_CATCH; }
  if (caught_by >= 0 || hold_move >= 0)                    /* a catch / a move with the ball wins the cycle: kicks are dropped */
    for (int i = 0; i < NP; ++i) { kicked[i] = 0; by_kick[i] = 0; kx[i] = ky[i] = R(0.0); }
  if (foul_by >= 0) {                                      /* the victim goes down; a foul the referee saw is a card */
    Obj *v = &m->o[foul_victim];
    if (v->tackle < p->foul_cycles + 1) v->tackle = p->foul_cycles + 1;
    if (foul_seen) m->o[foul_by].card += 1;                /* (he tackled in this cycle: he had not been sent off) */
  }
  /* 2. ball: accelerations summed in player order */
  REAL bax = R(0.0), bay = R(0.0);
  int any_kick = 0, last_kicker = -1, last_kick_cmd = -1, other_touch = 0;
  const int taker0 = m->set_play_taker & 0xff;            /* who may not touch the ball twice in a row (bit 8: his set play was an INDIRECT free kick) */
  for (int i = 0; i < NP; ++i) if (kicked[i]) {
    *ev |= by_kick[i] ? EV_KICK : EV_TACKLE;
    bax += kx[i]; bay += ky[i]; any_kick = 1; last_kicker = i;
    if (by_kick[i]) last_kick_cmd = i;
    if (i + 1 != taker0) other_touch = 1;
  }
  if (any_kick) m->last_touch_side = side_of(last_kicker);
  /* free-kick fault (FreeKickFault_, idl/service.proto:287): the taker of a set play plays the ball again before anybody else */
  const int fk_fault = p->free_kick_faults && mode0 == S2D_GM_PLAY_ON && taker0 != 0 && any_kick && !other_touch;
  if (any_kick) {
    if (pen) { /* the word carries the shoot-out's state */ }
    else if (is_setplay(mode0)) m->set_play_taker = (last_kicker + 1) | (mode0 == S2D_GM_IND_FREE_KICK ? 0x100 : 0);   /* this kick puts the ball into play */
    else if (other_touch) m->set_play_taker = 0;
    /* back-pass bookkeeping: the last Kick command counts; a tackle touch ends it */
    m->last_kicker = (last_kick_cmd == last_kicker) ? last_kick_cmd + 1 : 0;
  }
  const int ball_live = !is_setplay(mode0) || any_kick || mode0 == S2D_GM_PENALTY_TAKEN;
  if (caught_by >= 0) {                                   /* held: the ball rests where it was caught */
    b->vx = R(0.0); b->vy = R(0.0); m->last_touch_side = side_of(caught_by);
  } else if (hold_move >= 0) {                            /* the holding goalie moved: the ball goes with him, in front of his body */
    const Obj *g = &m->o[hold_move];
    REAL sn, cs, r = p->pt[hold_move].player_size + p->ball_size + R(0.1);   /* clear of the collision radius, well inside the kickable area */
    sincos_deg(g->body, &sn, &cs);
    b->x = g->x + r * cs; b->y = g->y + r * sn; b->vx = R(0.0); b->vy = R(0.0);
    m->goalie_moves -= 1;
  } else if (ball_live) {
    if (any_kick) {
      REAL a2 = sq2(bax, bay);
      if (a2 > p->ball_accel_max2) { REAL k = p->ball_accel_max / R(sqrt)(a2); bax *= k; bay *= k; }
      b->vx += bax; b->vy += bay;
    }
    REAL s2 = sq2(b->vx, b->vy);
    if (s2 > p->ball_speed_max2) { REAL k = p->ball_speed_max / R(sqrt)(s2); b->vx *= k; b->vy *= k; }
    if (p->noise) add_noise(&b->vx, &b->vy, p->ball_rand, rnd_u01(nzb[0]), rnd_u01(nzb[1]));
    b->x += b->vx; b->y += b->vy;
  }
  /* 3. collisions: Jacobi passes, every overlapping pair proposes symmetric contact positions */
  int collided[NOBJ]; memset(collided, 0, sizeof collided);
  int touch_player = -1;
  for (int pass = 0; pass < 10; ++pass) {
    REAL sx[NOBJ], sy[NOBJ]; int cnt[NOBJ]; int any = 0;
    for (int i = 0; i < NOBJ; ++i) {
      sx[i] = sy[i] = R(0.0); cnt[i] = 0;
      REAL ri = i == BALL ? p->ball_size : p->pt[i].player_size;
      for (int j = 0; j < NOBJ; ++j) {
        if (j == i) continue;
        REAL rj = j == BALL ? p->ball_size : p->pt[j].player_size;
        REAL dx = m->o[i].x - m->o[j].x, dy = m->o[i].y - m->o[j].y;
        REAL d2 = sq2(dx, dy), r = ri + rj;
        if (d2 < r * r) {
          REAL d = R(sqrt)(d2), ux, uy;
          if (d > R(0.0)) { ux = dx / d; uy = dy / d; } else { ux = i < j ? R(-1.0) : R(1.0); uy = R(0.0); }
          REAL mx = (m->o[i].x + m->o[j].x) * R(0.5), my = (m->o[i].y + m->o[j].y) * R(0.5), h = r * R(0.5);
          sx[i] += mx + ux * h; sy[i] += my + uy * h; cnt[i]++;
          if (i == BALL) touch_player = j;       /* last (highest index) player overlapping the ball */
        }
      }
      if (cnt[i]) any = 1;
    }
    if (!any) break;
    for (int i = 0; i < NOBJ; ++i) if (cnt[i]) {
      m->o[i].x = sx[i] / (REAL)cnt[i]; m->o[i].y = sy[i] / (REAL)cnt[i]; collided[i] = 1;
    }
  }
  for (int i = 0; i < NP; ++i) if (collided[i]) *ev |= EV_COLLIDE;
  if (collided[BALL]) *ev |= EV_BALL_COLLIDE;
  for (int i = 0; i < NOBJ; ++i) if (collided[i]) { m->o[i].vx *= p->collision_vel_rate; m->o[i].vy *= p->collision_vel_rate; }
  int coll_touch_side = SIDE_NONE;
  if (touch_player >= 0 && (!is_setplay(mode0) || side_of(touch_player) == side0)) {
    coll_touch_side = side_of(touch_player);
    m->last_touch_side = coll_touch_side;
    if (!pen && touch_player + 1 != (m->set_play_taker & 0xff)) m->set_play_taker = 0;
    if (touch_player + 1 != m->last_kicker) m->last_kicker = 0;
  }
  /* 4. set play: the side that does not take it keeps free_kick_distance from the ball; during an announcement that is the
   * offending side, the one the mode is named after (the restart will be the other side's) */
  if (is_setplay(mode0) && mode0 != S2D_GM_AFTER_GOAL && !is_period_end(mode0) && !pen) {
    const int kept_away = is_announcement(mode0) ? side0 : other_side(side0);
    for (int i = 0; i < NP; ++i) if (side_of(i) == kept_away && m->o[i].card < S2D_CARD_RED) {
      Obj *o = &m->o[i];
      REAL dx = o->x - b->x, dy = o->y - b->y, d = hypot2(dx, dy);
      if (d < p->free_kick_distance) {
        REAL ux, uy;
        if (d > R(0.0)) { ux = dx / d; uy = dy / d; } else { ux = side_of(i) == SIDE_LEFT ? R(-1.0) : R(1.0); uy = R(0.0); }
        o->x = b->x + ux * p->free_kick_distance; o->y = b->y + uy * p->free_kick_distance;
      }
    }
  }
  /* 5. referee.  The clock: WorldModel.cycle advances unless the mode of this cycle is one in which it stands still */
  m->tick = (int32_t)((uint32_t)m->tick + 1u);
  const int advanced = !(p->stopped_clock && clock_stands(mode0));
  if (advanced) { m->cycle = (int32_t)((uint32_t)m->cycle + 1u); m->stopped_cycle = 0; }
  else m->stopped_cycle += 1;
  if (!is_halted(mode0)) {
    if (mode0 == S2D_GM_AFTER_GOAL) {                   /* the ball is dead until the wait is over, then the conceding side kicks off */
      m->setplay_timer += 1;
      if (m->setplay_timer >= p->after_goal_wait) {
        int ks = other_side(side0);
        place_formation(m, ks);
        restart(m, S2D_GM_KICK_OFF, ks, R(0.0), R(0.0)); m->last_touch_side = SIDE_NONE;
      }
    } else if (mode0 == S2D_GM_BEFORE_KICK_OFF) {        /* BeforeKickOff (idl/service.proto:268): nobody plays the ball, players may Move */
      m->setplay_timer += 1;
      if (m->setplay_timer >= p->kick_off_wait) { m->mode = S2D_GM_KICK_OFF; m->setplay_timer = 0; }
    } else if (is_period_end(mode0)) {                   /* one cycle of "half time" / "time extended" (idl/service.proto:279, 299), then the next kick-off */
      m->mode = p->kick_off_wait > 0 ? S2D_GM_BEFORE_KICK_OFF : S2D_GM_KICK_OFF; m->setplay_timer = 0;
    } else if (mode0 == S2D_GM_GOALIE_CATCH) {           /* one cycle of "goalie_catch_ball" (:298), then his free kick */
      m->mode = S2D_GM_FREE_KICK; m->setplay_timer = 0;
    } else if (is_announcement(mode0)) {                 /* offside_l, back_pass_l, ...: after the wait, the restart for the other side */
      m->setplay_timer += 1;
      if (m->setplay_timer >= p->announce_wait) {
        m->mode = (mode0 == S2D_GM_BACK_PASS || mode0 == S2D_GM_FREE_KICK_FAULT) ? S2D_GM_IND_FREE_KICK : S2D_GM_FREE_KICK;
        m->mode_side = other_side(side0); m->setplay_timer = 0;
        /* PenaltyKick_ (idl/service.proto:278): a foul called inside the offender's own penalty area is restarted from the penalty
         * spot of that half, 11 m from the goal line (a constant of the pitch in rcssserver too), by the other side */
        const int own_area = R(fabs)(b->y) <= p->pen_half_w && (side0 == SIDE_LEFT ? b->x <= -p->pen_x : b->x >= p->pen_x);
        if (mode0 == S2D_GM_FOUL_CHARGE && own_area)
          restart(m, S2D_GM_PENALTY_KICK, other_side(side0), (side0 == SIDE_LEFT ? R(-1.0) : R(1.0)) * (p->half_l - R(11.0)), R(0.0));
      }
    } else if (pen) {                                    /* the shoot-out's own sequence */
      if (mode0 == S2D_GM_PENALTY_ONFIELD) {
        m->setplay_timer += 1;
        if (m->setplay_timer >= p->pen_before_setup_wait) pen_setup(p, m, SIDE_LEFT);          /* the left team kicks first */
      } else if (mode0 == S2D_GM_PENALTY_SETUP) {          /* one cycle: everybody was placed on entering it */
        m->mode = S2D_GM_PENALTY_READY; m->setplay_timer = 0;
      } else if (mode0 == S2D_GM_PENALTY_READY) {
        if (any_kick) { m->mode = S2D_GM_PENALTY_TAKEN; m->setplay_timer = 0; }
        else { m->setplay_timer += 1; if (m->setplay_timer >= p->pen_ready_wait) pen_result(m, side0, 0); }
      } else if (mode0 == S2D_GM_PENALTY_TAKEN) {
        const REAL bx = b->x, by = b->y;
        if (caught_by >= 0) pen_result(m, side0, 0);
        else if (!p->pen_allow_mult_kicks && kicked[pen_taker]) {   /* PenaltyFoul_ (:297): the kicker played the ball a second time */
          pen_result(m, side0, 0); m->mode = S2D_GM_PENALTY_FOUL;
        }
        else if (bx > p->half_l && R(fabs)(by) < p->goal_half_width) pen_result(m, side0, 1);
        else if (R(fabs)(bx) > p->half_l || R(fabs)(by) > p->half_w) pen_result(m, side0, 0);
        else { m->setplay_timer += 1; if (m->setplay_timer > p->pen_taken_wait) pen_result(m, side0, 0); }
      } else {                                             /* PenaltyScore_ / PenaltyMiss_ / PenaltyFoul_: the verdict stands for a while */
        m->setplay_timer += 1;
        if (m->setplay_timer >= p->pen_before_setup_wait) {
          if (pen_over(p, m->set_play_taker)) {
            /* ServerParam.pen_random_winner (idl/service.proto:1610): a shoot-out that ends level is decided by the toss of a coin --
             * one draw (TACKLE stream, the ball's block: no tackle uses it), below one half = the left team; the winner is written
             * into bits 28-29 of the set-play word (1 left, 2 right), the score stays as it is */
            if (p->pen_random_winner && pen_goals(m->set_play_taker, SIDE_LEFT) == pen_goals(m->set_play_taker, SIDE_RIGHT)) {
              uint32_t w[4]; draw(p->seed, gid, cyc, ST_TACKLE, BALL, w);
              m->set_play_taker |= (rnd_u01(w[0]) < R(0.5) ? 1 : 2) << 28;
            }
            m->mode = S2D_GM_TIME_OVER; m->mode_side = SIDE_NONE; m->done = 1; st->v[3]++;
          } else pen_setup(p, m, other_side(side0));
        }
      }
    } else if (is_setplay(mode0)) {
      if (any_kick) { m->mode = S2D_GM_PLAY_ON; m->setplay_timer = 0; }
      else { m->setplay_timer += 1; if (m->setplay_timer > p->drop_ball_time) { m->mode = S2D_GM_PLAY_ON; m->setplay_timer = 0; } }
    }
    if (m->mode == S2D_GM_PLAY_ON) {
      /* offside bookkeeping at the moment of a pass (positions before this cycle's movement) */
      if (any_kick) {
        int mask = 0;
        int exempt = mode0 == S2D_GM_KICK_IN || mode0 == S2D_GM_GOAL_KICK || mode0 == S2D_GM_CORNER_KICK;
        if (p->use_offside && !exempt) {
          int S = side_of(last_kicker);
          REAL dirS = S == SIDE_LEFT ? R(1.0) : R(-1.0);
          int o0 = S == SIDE_LEFT ? 11 : 0;
          REAL first = R(-1.0e9), second = R(-1.0e9);       /* two largest dirS*x among opponents */
          for (int j = o0; j < o0 + 11; ++j) {
            REAL v = dirS * x0[j];
            if (v > first) { second = first; first = v; } else if (v > second) second = v;
          }
          REAL line = R(0.0);
          if (second > line) line = second;
          REAL bl = dirS * x0[BALL];
          if (bl > line) line = bl;
          int t0 = S == SIDE_LEFT ? 0 : 11;
          for (int t = t0; t < t0 + 11; ++t) if (t != last_kicker && dirS * x0[t] > line) mask |= 1 << t;
        }
        m->offside_mask = mask;
      } else if (coll_touch_side != SIDE_NONE && m->offside_mask) {
        int flagged_side = (m->offside_mask & 0x7FF) ? SIDE_LEFT : SIDE_RIGHT;
        if (coll_touch_side != flagged_side) m->offside_mask = 0;
      }
      REAL bx = b->x, by = b->y;
      if (caught_by >= 0) {                                                  /* goalie holds the ball */
        int gs = side_of(caught_by);
        int in_area = R(fabs)(by) <= p->pen_half_w && (gs == SIDE_LEFT ? bx <= -p->pen_x : bx >= p->pen_x);
        /* back pass (BackPass_, idl/service.proto:286): the goalie catches a ball a team-mate kicked to him -- indirect free
         * kick for the other side from the nearer front corner of the penalty area */
        const int lk = m->last_kicker - 1;
        const int back_pass = p->back_passes && in_area && lk >= 0 && lk != caught_by && side_of(lk) == gs;
        /* otherwise, inside the own penalty area: GoalieCatch_, then a free kick for the goalie's side; outside: CatchFault_ */
        if (back_pass) restart(m, S2D_GM_BACK_PASS, gs, gs == SIDE_LEFT ? -p->pen_x : p->pen_x, by > R(0.0) ? p->pen_half_w : -p->pen_half_w);
        else restart(m, in_area ? S2D_GM_GOALIE_CATCH : S2D_GM_CATCH_FAULT, gs, bx, by);
        if (in_area && !back_pass) { m->ball_holder = caught_by + 1; m->goalie_moves = p->goalie_max_moves; }
      } else if (foul_by >= 0 && foul_seen) {                                /* the referee saw the foul: FoulCharge_ where the ball is */
        restart(m, S2D_GM_FOUL_CHARGE, side_of(foul_by), clampr(bx, -p->half_l, p->half_l), clampr(by, -p->half_w, p->half_w));
      } else if (fk_fault) {                                                 /* the taker touched the ball twice */
        restart(m, S2D_GM_FREE_KICK_FAULT, side_of(taker0 - 1), clampr(bx, -p->half_l, p->half_l), clampr(by, -p->half_w, p->half_w));
      /* no goal directly from an indirect free kick (IndFreeKick_, idl/service.proto:289): while nobody but its taker has touched the
       * ball, a ball in the net is a ball over the goal line -- a goal kick for the defenders, by the branch below */
      } else if (!(m->set_play_taker & 0x100) && bx > p->half_l && R(fabs)(by) < p->goal_half_width) {       /* goal for the left team */
        m->score_left += 1; m->reward_left = R(1.0); st->v[1]++; *ev |= EV_GOAL;
        if (p->after_goal_wait > 0) restart(m, S2D_GM_AFTER_GOAL, SIDE_LEFT, bx, by);   /* the ball rests in the net */
        else { place_formation(m, SIDE_RIGHT); restart(m, S2D_GM_KICK_OFF, SIDE_RIGHT, R(0.0), R(0.0)); }
        m->last_touch_side = SIDE_NONE;
      } else if (!(m->set_play_taker & 0x100) && bx < -p->half_l && R(fabs)(by) < p->goal_half_width) {      /* goal for the right team */
        m->score_right += 1; m->reward_left = R(-1.0); st->v[2]++; *ev |= EV_GOAL;
        if (p->after_goal_wait > 0) restart(m, S2D_GM_AFTER_GOAL, SIDE_RIGHT, bx, by);
        else { place_formation(m, SIDE_LEFT); restart(m, S2D_GM_KICK_OFF, SIDE_LEFT, R(0.0), R(0.0)); }
        m->last_touch_side = SIDE_NONE;
      } else if (R(fabs)(bx) > p->half_l || R(fabs)(by) > p->half_w) {       /* ball out */
        st->v[7]++;
        int toucher = m->last_touch_side == SIDE_NONE ? SIDE_LEFT : m->last_touch_side;
        REAL sy = by < R(0.0) ? R(-1.0) : R(1.0), sxn = bx < R(0.0) ? R(-1.0) : R(1.0);
        if (R(fabs)(bx) <= p->half_l) {                                      /* over a side line: kick-in */
          restart(m, S2D_GM_KICK_IN, other_side(toucher), clampr(bx, -p->half_l, p->half_l), sy * p->half_w);
        } else {
          int defender = bx > R(0.0) ? SIDE_RIGHT : SIDE_LEFT;               /* right team defends the +x goal */
          if (toucher == defender) restart(m, S2D_GM_CORNER_KICK, other_side(defender), sxn * (p->half_l - R(1.0)), sy * (p->half_w - R(1.0)));
          else restart(m, S2D_GM_GOAL_KICK, defender, sxn * (p->half_l - R(5.5)), sy * R(9.16));
        }
      } else if (m->offside_mask) {                                          /* flagged player plays the ball */
        for (int t = 0; t < NP; ++t) if (m->offside_mask & (1 << t)) {
          REAL dx = m->o[t].x - bx, dy = m->o[t].y - by;
          if (sq2(dx, dy) < p->offside_area2) {
            st->v[6]++;
            restart(m, S2D_GM_OFF_SIDE, side_of(t), m->o[t].x, m->o[t].y);
            break;
          }
        }
      }
    }
    /* IllegalDefense_ (idl/service.proto:295; ServerParam.illegal_defense_*: 1637-1640; rcssserver's IllegalDefenseRef restated; off when
     * number = 0, as in the stock server).  Counted in the cycles played in PlayOn that leave the game in PlayOn: a team with at
     * least `number` players (not sent off) inside the strip in front of its own goal while the other team was the last to play
     * the ball adds a cycle, anything else starts again; `duration` cycles on end are called.  The two counters live in
     * setplay_timer (bits 0-7 left, 8-15 right), which PlayOn does not use and every restart clears. */
    if (p->illegal_defense_number > 0 && mode0 == S2D_GM_PLAY_ON && m->mode == S2D_GM_PLAY_ON) {
      int nl = 0, nr = 0;
      for (int i = 0; i < NP; ++i) {
        const Obj *o = &m->o[i];
        if (o->card >= S2D_CARD_RED || !(R(fabs)(o->y) < p->ill_half_w)) continue;
        if (i < 11) { if (o->x < -p->ill_x) nl++; } else { if (o->x > p->ill_x) nr++; }
      }
      int cl = m->setplay_timer & 0xff, cr = (m->setplay_timer >> 8) & 0xff;
      cl = (m->last_touch_side == SIDE_RIGHT && nl >= p->illegal_defense_number) ? (cl < 255 ? cl + 1 : 255) : 0;
      cr = (m->last_touch_side == SIDE_LEFT && nr >= p->illegal_defense_number) ? (cr < 255 ? cr + 1 : 255) : 0;
      m->setplay_timer = cl | (cr << 8);
      if (cl >= p->illegal_defense_duration) restart(m, S2D_GM_ILLEGAL_DEFENSE, SIDE_LEFT, -(p->half_l - R(11.0)), R(0.0));
      else if (cr >= p->illegal_defense_duration) restart(m, S2D_GM_ILLEGAL_DEFENSE, SIDE_RIGHT, p->half_l - R(11.0), R(0.0));
    }
    /* half time / extra time / time over (rcssserver's TimeReferee; ServerParam.nr_extra_halfs, extra_half_time, golden_goal:
     * idl/service.proto:1601, 1622, 1635): decided only when the clock has just moved.  Normal time = nr_normal_halfs halves; a
     * draw at its end is extended by nr_extra_halfs halves of extra_half_cycles, played in full unless golden_goal; the periods
     * alternate the kick-off side; a draw after the last period goes to the penalty shoot-out (penalty_shoot_outs, :1602). */
    const int total = p->half_time_cycles * p->nr_normal_halfs;
    const int ext_total = total + p->extra_half_cycles * p->nr_extra_halfs;
    const int tied = m->score_left == m->score_right;
    int over = 0, period = -1;                           /* period = index of the period that starts now (kick-off side by parity) */
    if (p->nr_extra_halfs <= 0) over = advanced && m->cycle >= total;
    else if (advanced && m->cycle == total) over = !tied;
    else if (advanced && m->cycle >= ext_total) over = 1;
    if (p->golden_goal && p->nr_extra_halfs > 0 && m->cycle > total && m->reward_left != R(0.0)) over = 1;   /* a goal (this cycle) in extra time */
    if (pen) over = 0;                                   /* (the shoot-out ends by its own count; its clock stands) */
    const int last_end = advanced && m->cycle == ext_total;       /* (= total without extra halves) */
    if (over && last_end && tied && p->penalty_shoot_outs) {
      /* a draw after the last period: PenaltyOnfield_, named after the half the kicks are taken in (the right one) */
      restart(m, S2D_GM_PENALTY_ONFIELD, SIDE_RIGHT, b->x, b->y); m->last_touch_side = SIDE_NONE;
    } else if (over) {
      m->mode = S2D_GM_TIME_OVER; m->mode_side = SIDE_NONE; m->done = 1; m->offside_mask = 0; st->v[3]++;
    } else if (pen) {
    } else if (advanced && m->cycle < total) {
      if (p->half_time_cycles > 0 && m->cycle % p->half_time_cycles == 0) period = m->cycle / p->half_time_cycles;
    } else if (advanced) {                               /* cycle >= total and not over: extra halves are being played */
      if ((m->cycle - total) % p->extra_half_cycles == 0) period = p->nr_normal_halfs + (m->cycle - total) / p->extra_half_cycles;
    }
    if (period >= 0) {
      int ks = (period & 1) ? SIDE_RIGHT : SIDE_LEFT;
      recover_all(p, m, 0);
      place_formation(m, ks);
      restart(m, m->cycle == total ? S2D_GM_EXTEND_HALF : S2D_GM_FIRST_HALF_OVER, ks, R(0.0), R(0.0)); m->last_touch_side = SIDE_NONE;
    }
    if (m->mode != S2D_GM_FREE_KICK && m->mode != S2D_GM_GOALIE_CATCH) { m->ball_holder = 0; m->goalie_moves = 0; }   /* nobody holds the ball any more */
  }
  /* a second card is a red one: the player leaves the pitch (checked every cycle; a parked player does not move) */
  for (int i = 0; i < NP; ++i) if (m->o[i].card >= S2D_CARD_RED) park_sent_off(p, &m->o[i], i);
  /* 6. decay, tackle timers, stamina */
  for (int i = 0; i < NP; ++i) {
    Obj *o = &m->o[i];
    o->vx *= p->pt[i].player_decay; o->vy *= p->pt[i].player_decay;
    if (o->tackle > 0) o->tackle -= 1;
    if (o->catch_ban > 0) o->catch_ban -= 1;
    m_update_stamina(p, &p->pt[i], o);
  }
  b->vx *= p->ball_decay; b->vy *= p->ball_decay;
  /* 7. nearest player to the ball per team (ties: lowest index) */
  {
    REAL best_l = R(3.0e38), best_r = R(3.0e38); int il = 0, ir = 11;
    for (int i = 0; i < NP; ++i) {
      REAL d2 = sq2(m->o[i].x - b->x, m->o[i].y - b->y);
      if (i < 11) { if (d2 < best_l) { best_l = d2; il = i; } } else { if (d2 < best_r) { best_r = d2; ir = i; } }
    }
    m->nearest_left = il; m->nearest_right = ir;
  }
  st->v[0]++;
  if (m->done && p->auto_reset) {
    uint8_t d = m->done; REAL rw = m->reward_left; int32_t tk = m->tick;
    match_reset(p, m);
    m->done = d; m->reward_left = rw; m->tick = tk;      /* the draws of the next match continue the sequence */
  }
}

/* uniform random policy of the benchmark: Philox POLICY stream, block = player, counter = cycle / 4 (one word per cycle):
 * command = the two top bits of the word, magnitude = the 15 bits below them, direction = the low 15 bits */
static void random_actions(const MP *p, uint64_t gid, uint32_t cyc, float *act) {
  for (int i = 0; i < NP; ++i) {
    uint32_t w[4];
    draw(p->seed, gid, cyc >> 2, ST_POLICY, (uint32_t)i, w);
    const uint32_t wd = w[cyc & 3u];
    int cmd = 1 + (int)(wd >> 30);
    REAL u = (REAL)((wd >> 15) & 0x7FFFu) * R(3.0517578125e-05), s = (REAL)(wd & 0x7FFFu) * R(6.103515625e-05) - R(1.0);
    REAL a, b = R(0.0);
    if (cmd == S2D_MCMD_DASH || cmd == S2D_MCMD_KICK) { a = u * R(100.0); b = s * R(180.0); }
    else { a = s * R(180.0); }
    act[i * 3 + 0] = (float)cmd; act[i * 3 + 1] = (float)a; act[i * 3 + 2] = (float)b;
  }
}

/* ------------------------------------------------------------------ vectorised engine */
/* env_id: each env's Philox id (NULL: env_id_offset + e) -- a batch of states taken from different matches keeps their draws;
 * ev: what happened in each env in the last cycle (EV_* bits) */
typedef struct S2DMOEngine { MP p; int64_t n; Match *m; MatchStats st; int64_t *env_id; uint32_t *ev; } S2DMOEngine;
static uint64_t env_gid(const S2DMOEngine *h, int64_t e) { return (uint64_t)(h->env_id ? h->env_id[e] : h->p.env_id_offset + e); }

API S2DMOEngine *s2dmo_create(const S2DMatchConfig *cfg, int64_t n) {
  if (!cfg || n <= 0) return NULL;
  S2DMOEngine *h = (S2DMOEngine *)calloc(1, sizeof *h);
  mp_from_config(cfg, &h->p); h->n = n;
  h->m = (Match *)calloc((size_t)n, sizeof(Match));
  h->ev = (uint32_t *)calloc((size_t)n, sizeof(uint32_t));
  for (int64_t e = 0; e < n; ++e) match_reset(&h->p, &h->m[e]);
  return h;
}
API void s2dmo_destroy(S2DMOEngine *h) { if (h) { free(h->m); free(h->env_id); free(h->ev); free(h); } }
API void s2dmo_reset(S2DMOEngine *h, const uint8_t *mask) {
  for (int64_t e = 0; e < h->n; ++e) if (!mask || mask[e]) match_reset(&h->p, &h->m[e]);
}
API void s2dmo_step(S2DMOEngine *h, const float *actions) {
  MatchStats tot; memset(&tot, 0, sizeof tot);
#pragma omp parallel
  {
    MatchStats loc; memset(&loc, 0, sizeof loc);
#pragma omp for schedule(static)
    for (int64_t e = 0; e < h->n; ++e) {
      float buf[NP * 3];
      const float *a = actions ? actions + (size_t)e * NP * 3 : buf;
      if (!actions) random_actions(&h->p, env_gid(h, e), (uint32_t)h->m[e].tick, buf);
      h->ev[e] = 0;
      match_step(&h->p, &h->m[e], env_gid(h, e), a, &loc, &h->ev[e]);
    }
#pragma omp critical
    for (int k = 0; k < 8; ++k) tot.v[k] += loc.v[k];
  }
  for (int k = 0; k < 8; ++k) h->st.v[k] += tot.v[k];
}
/* field: 0..8 object planes x,y,vx,vy,body,stamina,effort,recovery,capacity -> out[n][24] (float as double);
 * 9 tackle -> out[n][24]; 10.. per-env ints: cycle, mode, mode_side, score_left, score_right, last_touch_side,
 * setplay_timer, offside_mask, 18 reward_left, 19 done, 20 nearest_left, 21 nearest_right -> out[n] */
API int s2dmo_get(const S2DMOEngine *h, int field, double *out) {
  for (int64_t e = 0; e < h->n; ++e) {
    const Match *m = &h->m[e];
    if (field <= 9 || field == 22 || field == 29) {      /* 22 = catch_ban, 29 = card (object planes) */
      for (int s = 0; s < S2D_MATCH_SLOTS; ++s) {
        double v = 0;
        if (s < NOBJ) {
          const Obj *o = &m->o[s];
          switch (field) {
            case 22: v = o->catch_ban; break; case 29: v = o->card; break;
            case 0: v = o->x; break; case 1: v = o->y; break; case 2: v = o->vx; break; case 3: v = o->vy; break;
            case 4: v = o->body; break; case 5: v = o->stamina; break; case 6: v = o->effort; break;
            case 7: v = o->recovery; break; case 8: v = o->capacity; break; default: v = o->tackle; break;
          }
        }
        out[e * S2D_MATCH_SLOTS + s] = v;
      }
    } else {
      double v;
      switch (field) {
        case 10: v = m->cycle; break; case 11: v = m->mode; break; case 12: v = m->mode_side; break;
        case 13: v = m->score_left; break; case 14: v = m->score_right; break; case 15: v = m->last_touch_side; break;
        case 16: v = m->setplay_timer; break; case 17: v = m->offside_mask; break; case 18: v = m->reward_left; break;
        case 19: v = m->done; break; case 20: v = m->nearest_left; break; case 21: v = m->nearest_right; break;
        case 23: v = m->ball_holder; break; case 24: v = m->goalie_moves; break;
        case 25: v = m->set_play_taker; break; case 26: v = m->last_kicker; break;
        case 27: v = m->stopped_cycle; break; case 28: v = m->tick; break;
        default: return -1;
      }
      out[e] = v;
    }
  }
  return 0;
}
/* place one object / set per-env ints (tests: hand-built scenarios).  slot 0..22; vals = 10 numbers in plane order */
API int s2dmo_set_obj(S2DMOEngine *h, int64_t e, int slot, const double *v10) {
  if (e < 0 || e >= h->n || slot < 0 || slot >= NOBJ) return -1;
  Obj *o = &h->m[e].o[slot];
  o->x = (REAL)v10[0]; o->y = (REAL)v10[1]; o->vx = (REAL)v10[2]; o->vy = (REAL)v10[3]; o->body = (REAL)v10[4];
  o->stamina = (REAL)v10[5]; o->effort = (REAL)v10[6]; o->recovery = (REAL)v10[7]; o->capacity = (REAL)v10[8];
  o->tackle = (int32_t)v10[9]; o->catch_ban = 0;
  return 0;
}
API int s2dmo_set_card(S2DMOEngine *h, int64_t e, int slot, int card) {
  if (e < 0 || e >= h->n || slot < 0 || slot >= NP) return -1;
  h->m[e].o[slot].card = card;
  return 0;
}
API int s2dmo_set_touch(S2DMOEngine *h, int64_t e, int set_play_taker, int last_kicker) {
  if (e < 0 || e >= h->n) return -1;
  h->m[e].set_play_taker = set_play_taker; h->m[e].last_kicker = last_kicker;
  return 0;
}
API int s2dmo_set_game(S2DMOEngine *h, int64_t e, const int32_t *v8) {
  if (e < 0 || e >= h->n) return -1;
  Match *m = &h->m[e];
  m->cycle = v8[0]; m->mode = v8[1]; m->mode_side = v8[2]; m->score_left = v8[3]; m->score_right = v8[4];
  m->last_touch_side = v8[5]; m->setplay_timer = v8[6]; m->offside_mask = v8[7];
  return 0;
}
API const unsigned long long *s2dmo_stats(const S2DMOEngine *h) { return h->st.v; }
/* Player.dist_from_self / angle_from_self tables (idl/service.proto:84-85, 155-156): out[n][22][23] as float */
API void s2dmo_relative(const S2DMOEngine *h, float *dist, float *angle) {
  for (int64_t e = 0; e < h->n; ++e) for (int p = 0; p < NP; ++p) for (int j = 0; j < NOBJ; ++j) {
    const Match *m = &h->m[e];
    REAL dx = m->o[j].x - m->o[p].x, dy = m->o[j].y - m->o[p].y;
    size_t k = ((size_t)e * NP + p) * NOBJ + j;
    dist[k] = j == p ? 0.0f : (float)hypot2(dx, dy);
    angle[k] = j == p ? 0.0f : (float)atan2_deg(dy, dx);
  }
}
API void s2dmo_random_actions(const S2DMOEngine *h, float *out) {
  for (int64_t e = 0; e < h->n; ++e)
    random_actions(&h->p, env_gid(h, e), (uint32_t)h->m[e].tick, out + (size_t)e * NP * 3);
}
/* Load every Match word of envs e0 .. e0 + count - 1 from planes laid out like the device buffers (MATCH_BUFFER_FIELDS of
 * soccer2d_amd/_capi_match.py, stats left out), so that a device snapshot goes straight in:
 *   0-8   x y vx vy body stamina effort recovery stamina_capacity   float [count][24]
 *   9-10  tackle_cycles catch_ban                                    int32 [count][24]
 *   11-24 cycle mode mode_side score_left score_right last_touch_side setplay_timer offside_mask ball_holder goalie_moves
 *         set_play_taker last_kicker stopped_cycle tick               int32 [count]
 *   25    card int32 [count][24];  26 reward_left float [count];  27 done uint8 [count];  28-29 nearest_left nearest_right int32 [count]
 * Slot 23 of the object planes is padding and is not read. */
enum { LOAD_PLANES = 30 };
API int s2dmo_load(S2DMOEngine *h, int64_t e0, int64_t count, const void *const *planes) {
  if (e0 < 0 || count < 0 || e0 + count > h->n) return -1;
  for (int k = 0; k < LOAD_PLANES; ++k) if (!planes[k]) return -2;
  for (int64_t j = 0; j < count; ++j) {
    Match *m = &h->m[e0 + j];
    for (int s = 0; s < NOBJ; ++s) {
      const size_t q = (size_t)j * S2D_MATCH_SLOTS + (size_t)s;
      Obj *o = &m->o[s];
      o->x = (REAL)((const float *)planes[0])[q]; o->y = (REAL)((const float *)planes[1])[q];
      o->vx = (REAL)((const float *)planes[2])[q]; o->vy = (REAL)((const float *)planes[3])[q];
      o->body = (REAL)((const float *)planes[4])[q]; o->stamina = (REAL)((const float *)planes[5])[q];
      o->effort = (REAL)((const float *)planes[6])[q]; o->recovery = (REAL)((const float *)planes[7])[q];
      o->capacity = (REAL)((const float *)planes[8])[q];
      o->tackle = ((const int32_t *)planes[9])[q]; o->catch_ban = ((const int32_t *)planes[10])[q];
      o->card = ((const int32_t *)planes[25])[q];
    }
    int32_t w[14];
    for (int k = 0; k < 14; ++k) w[k] = ((const int32_t *)planes[11 + k])[j];
    m->cycle = w[0]; m->mode = w[1]; m->mode_side = w[2]; m->score_left = w[3]; m->score_right = w[4]; m->last_touch_side = w[5];
    m->setplay_timer = w[6]; m->offside_mask = w[7]; m->ball_holder = w[8]; m->goalie_moves = w[9]; m->set_play_taker = w[10];
    m->last_kicker = w[11]; m->stopped_cycle = w[12]; m->tick = w[13];
    m->reward_left = (REAL)((const float *)planes[26])[j]; m->done = ((const uint8_t *)planes[27])[j];
    m->nearest_left = ((const int32_t *)planes[28])[j]; m->nearest_right = ((const int32_t *)planes[29])[j];
  }
  return 0;
}
/* the Philox id of every env (n of them; NULL: env_id_offset + e again) */
API void s2dmo_set_env_ids(S2DMOEngine *h, const int64_t *ids) {
  free(h->env_id); h->env_id = NULL;
  if (ids) { h->env_id = (int64_t *)malloc((size_t)h->n * sizeof(int64_t)); memcpy(h->env_id, ids, (size_t)h->n * sizeof(int64_t)); }
}
API const uint32_t *s2dmo_events(const S2DMOEngine *h) { return h->ev; }
