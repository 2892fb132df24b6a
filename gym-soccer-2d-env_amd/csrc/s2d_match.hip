// s2d_match.hip -- 11v11 full-match engine for MI355X (gfx950): kernels + C ABI of
// include/s2d_match.h.  Rules = rcssserver's, restated (EXT); the tests
// hold an independent CPU restatement of the same rules which this file matches bit for bit.
//
// Mapping: ONE MATCH PER HALF-WAVE.  Lanes 0..21 of a 32-lane half are the players
// (0..10 left team, 11..21 right team), lane 22 is the ball, lanes 23..31 idle; a wave runs
// two matches, a 256-thread workgroup eight.  All per-object work (commands, movement,
// stamina) is lane-local; the cross-object steps use half-wave shuffles (ds_bpermute, width
// 32) and 64-bit ballots split per half:
//   * kick / tackle impulses are summed into the ball in player order (fixed order = fixed
//     fp32 result),
//   * collisions are Jacobi passes: every lane scans the 23 objects of its match, proposes
//     the symmetric contact position for each overlap and takes the mean (no ordering, no
//     atomics), up to 10 passes,
//   * referee decisions (goal, ball out, restarts, offside, half time) are evaluated
//     redundantly by every lane of the half from broadcast values, so there is no divergence
//     inside a match and no serial "referee lane",
//   * nearest-player-to-ball per team is a 22-step scan in index order.
// Every lane stays active for the whole kernel (shuffles need their source lanes), matches
// beyond N only skip their loads and stores.
#include "s2d_match_host.h"

__global__ __launch_bounds__(kMBlock) void s2d_match_reset_kernel(MParams p, MPtrs q, int64_t n, const uint8_t* __restrict__ mask) {
  const int l = threadIdx.x & (kHalf - 1);
  const int64_t e = (int64_t)blockIdx.x * kEnvsPerBlock + threadIdx.x / kHalf;
  if (e >= n) return;
  if (mask && !mask[e]) return;
  MObj o; MGame g; MRare r;
  m_reset(p, q.ptab[PT_EFFORT_MAX * kHalf + l], o, g, r, l);
  m_store(q, e, l, o, g, r);
}

// Relative tables (Player.dist_from_self / angle_from_self of every agent's WorldModel): lane p scans the
// 23 objects of its match through a broadcast-read LDS tile and writes one row of 23 values.
__global__ __launch_bounds__(kMBlock) void s2d_match_relative_kernel(MPtrs q, int64_t n, float* __restrict__ dist,
                                                                      float* __restrict__ angle) {
  __shared__ float2 pos_tile[kEnvsPerBlock][kHalf];
  const int l = threadIdx.x & (kHalf - 1);
  const int64_t e = (int64_t)blockIdx.x * kEnvsPerBlock + threadIdx.x / kHalf;
  const bool valid = e < n;
  const int64_t ec = valid ? e : n - 1;
  float x = 0.0f, y = 0.0f;
  if (l <= BALL) { x = q.obj[MF_X * q.obj_stride + ec * SLOTS + l]; y = q.obj[MF_Y * q.obj_stride + ec * SLOTS + l]; }
  float2* pos = pos_tile[threadIdx.x / kHalf];
  pos[l] = make_float2(x, y);
  wave_fence();
  if (valid && l < NP) {
    float* drow = dist + ((e * NP + l) * (int64_t)(BALL + 1));
    float* arow = angle + ((e * NP + l) * (int64_t)(BALL + 1));
    for (int j = 0; j <= BALL; ++j) {
      const float2 pj = pos[j];
      float dx = pj.x - x, dy = pj.y - y;
      drow[j] = j == l ? 0.0f : hypot2(dx, dy);
      arow[j] = j == l ? 0.0f : atan2_deg(dy, dx);
    }
  }
}

// One match per half-wave: the facts, then for each agent of the mask in slot order its row into LDS and out to memory.
__global__ __launch_bounds__(kMBlock) void s2d_match_agent_obs_kernel(MParams p, MAgentTab tab, MPtrs q, int64_t n, uint32_t mask,
                                                                       float* __restrict__ obs) {
  __shared__ MAObsShared sh_all[kEnvsPerBlock];
  MAObsShared& sh = sh_all[threadIdx.x / kHalf];
  const int l = threadIdx.x & (kHalf - 1);
  const int half = (threadIdx.x >> 5) & 1;
  const int64_t e = (int64_t)blockIdx.x * kEnvsPerBlock + threadIdx.x / kHalf;
  const bool valid = e < n;
  const int64_t ec = valid ? e : n - 1;
  MAgentIn in{};
  if (l <= BALL) {
    const int64_t k = ec * SLOTS + l;
    in.x = q.obj[MF_X * q.obj_stride + k]; in.y = q.obj[MF_Y * q.obj_stride + k];
    in.vx = q.obj[MF_VX * q.obj_stride + k]; in.vy = q.obj[MF_VY * q.obj_stride + k];
  }
  if (l < NP) {
    const int64_t k = ec * SLOTS + l;
    in.body = q.obj[MF_BODY * q.obj_stride + k];
    in.stamina = q.obj[MF_STAMINA * q.obj_stride + k]; in.effort = q.obj[MF_EFFORT * q.obj_stride + k];
    in.recovery = q.obj[MF_RECOVERY * q.obj_stride + k]; in.capacity = q.obj[MF_CAPACITY * q.obj_stride + k];
    in.tackle = __float_as_int(q.obj[MF_TACKLE * q.obj_stride + k]); in.card = __float_as_int(q.obj[MF_CARD * q.obj_stride + k]);
    in.catch_ban = __float_as_int(q.obj[MF_CATCH_BAN * q.obj_stride + k]);
  }
  in.cycle = q.env[ME_CYCLE * q.env_stride + ec]; in.mode = q.env[ME_MODE * q.env_stride + ec];
  in.mode_side = q.env[ME_MODE_SIDE * q.env_stride + ec]; in.last_touch = q.env[ME_LAST_TOUCH * q.env_stride + ec];
  in.score_l = q.env[ME_SCORE_L * q.env_stride + ec]; in.score_r = q.env[ME_SCORE_R * q.env_stride + ec];
  in.holder = q.env[ME_HOLDER * q.env_stride + ec]; in.stopped = q.env[ME_STOPPED * q.env_stride + ec];
  const MAgentDerived f = m_agent_facts(tab, sh, in, l, half);
  const int nrows = __builtin_popcount(mask);
  float* out = obs + (e * (int64_t)nrows) * S2D_AGENT_OBS_DIM;
  uint32_t rest = mask;
  for (int r = 0; r < nrows; ++r) {
    const int pa = __builtin_ctz(rest);                // the agent (uniform: the mask is a kernel argument)
    rest &= rest - 1u;
    m_agent_row(p, tab, sh, in, f, l, pa, sh.row);
    wave_fence();
    if (valid) m_agent_row_store(out + (int64_t)r * S2D_AGENT_OBS_DIM, sh.row, l);
    wave_fence();
  }
}

static size_t m_align(size_t v, size_t a) { return (v + a - 1) / a * a; }
struct MLayout { size_t obj, env, reward, done, stats, ptab, total; int64_t stride; };
static MLayout m_layout(int64_t n) {
  MLayout L; L.stride = (int64_t)m_align((size_t)n, 64);
  size_t off = 0;
  L.obj = off; off += m_align((size_t)MF_OBJ_PLANES * (size_t)L.stride * SLOTS * 4, 256);
  L.env = off; off += m_align((size_t)ME_ENV_PLANES * (size_t)L.stride * 4, 256);
  L.reward = off; off += m_align((size_t)L.stride * 4, 256);
  L.done = off; off += m_align((size_t)L.stride, 256);
  L.stats = off; off += (size_t)S2D_STATS_STRIPES * 8 * sizeof(unsigned long long);
  L.ptab = off; off += m_align((size_t)PT_WORDS * kHalf * 4, 256);
  L.total = off;
  return L;
}

// PlayerType 0 = the ServerParam values
static S2DPlayerType m_default_type(const S2DServerParams& s, const S2DMatchParams& m) {
  S2DPlayerType t;
  t.player_speed_max = s.player_speed_max; t.stamina_inc_max = s.stamina_inc_max; t.player_decay = s.player_decay;
  t.inertia_moment = s.inertia_moment; t.dash_power_rate = s.dash_power_rate; t.player_size = s.player_size;
  t.kickable_margin = m.kickable_margin; t.kick_rand = m.kick_rand; t.extra_stamina = s.extra_stamina;
  t.effort_max = s.effort_init; t.effort_min = s.effort_min; t.kick_power_rate = m.kick_power_rate;
  t.catchable_area_l_stretch = 1.0;
  return t;
}

S2D_API void s2d_match_default_player_params(S2DPlayerParams* q) {   // rcssserver stock player.conf (EXT)
  if (!q) return;
  std::memset(q, 0, sizeof *q);
  q->player_speed_max_delta_min = 0.0; q->player_speed_max_delta_max = 0.0; q->stamina_inc_max_delta_factor = 0.0;
  q->player_decay_delta_min = -0.1; q->player_decay_delta_max = 0.1; q->inertia_moment_delta_factor = 25.0;
  q->dash_power_rate_delta_min = 0.0; q->dash_power_rate_delta_max = 0.0; q->player_size_delta_factor = -100.0;
  q->kickable_margin_delta_min = -0.1; q->kickable_margin_delta_max = 0.1; q->kick_rand_delta_factor = 1.0;
  q->extra_stamina_delta_min = 0.0; q->extra_stamina_delta_max = 50.0;
  q->effort_max_delta_factor = -0.004; q->effort_min_delta_factor = -0.004;
  q->new_dash_power_rate_delta_min = -0.0012; q->new_dash_power_rate_delta_max = 0.0008;
  q->new_stamina_inc_max_delta_factor = -6000.0;
  q->kick_power_rate_delta_min = 0.0; q->kick_power_rate_delta_max = 0.0;
  q->catchable_area_l_stretch_min = 1.0; q->catchable_area_l_stretch_max = 1.3;
}

// host-side Philox (same function as the device's) for the type generator
static void h_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
  for (int r = 0; r < 10; ++r) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// rcssserver's HeteroPlayer recipe (EXT, as published): each non-default type draws one delta per
// trade-off pair from the PlayerParam ranges -- faster decay <-> more inertia, stronger dash <-> less
// stamina income, wider kickable margin <-> noisier kicks, more extra stamina <-> lower effort range --
// and is re-drawn until its top speed (effort_max * dash_power_rate * max_dash_power / (1 - decay))
// lies in (0.75, player_speed_max].  Uniforms: Philox stream S2D_ST_TYPES at counter (type id, try).
S2D_API int s2d_match_generate_player_types(S2DMatchConfig* c, const S2DPlayerParams* pp, uint64_t seed) {
  if (!c) return mfail(S2D_EINVAL, "config is NULL");
  S2DPlayerParams stock;
  if (!pp) { s2d_match_default_player_params(&stock); pp = &stock; }
  const S2DServerParams& s = c->sp; const S2DMatchParams& m = c->mp;
  const S2DPlayerType base = m_default_type(s, m);
  c->player_types[0] = base;
  for (int id = 1; id < S2D_MATCH_PLAYER_TYPES; ++id) {
    S2DPlayerType t = base;
    for (int attempt = 0; attempt < 1000; ++attempt) {
      double u[12];
      for (int b = 0; b < 3; ++b) {
        uint32_t w[4];
        h_philox((uint32_t)id, (uint32_t)attempt, 0u, (S2D_ST_TYPES << 16) | (uint32_t)b, (uint32_t)seed, (uint32_t)(seed >> 32), w);
        for (int k = 0; k < 4; ++k) u[b * 4 + k] = (double)(w[k] >> 8) * 5.9604644775390625e-8;
      }
      auto U = [&](int k, double lo, double hi) { return lo + u[k] * (hi - lo); };
      t = base;
      double d = U(0, pp->player_speed_max_delta_min, pp->player_speed_max_delta_max);
      t.player_speed_max += d; t.stamina_inc_max += d * pp->stamina_inc_max_delta_factor;
      d = U(1, pp->player_decay_delta_min, pp->player_decay_delta_max);
      t.player_decay += d; t.inertia_moment += d * pp->inertia_moment_delta_factor;
      d = U(2, pp->dash_power_rate_delta_min, pp->dash_power_rate_delta_max);
      t.dash_power_rate += d; t.player_size += d * pp->player_size_delta_factor;
      d = U(3, pp->new_dash_power_rate_delta_min, pp->new_dash_power_rate_delta_max);
      t.dash_power_rate += d; t.stamina_inc_max += d * pp->new_stamina_inc_max_delta_factor;
      d = U(4, pp->kickable_margin_delta_min, pp->kickable_margin_delta_max);
      t.kickable_margin += d; t.kick_rand += d * pp->kick_rand_delta_factor;
      d = U(5, pp->extra_stamina_delta_min, pp->extra_stamina_delta_max);
      t.extra_stamina += d; t.effort_max += d * pp->effort_max_delta_factor; t.effort_min += d * pp->effort_min_delta_factor;
      d = U(6, pp->kick_power_rate_delta_min, pp->kick_power_rate_delta_max);
      t.kick_power_rate += d;
      t.catchable_area_l_stretch = U(7, pp->catchable_area_l_stretch_min, pp->catchable_area_l_stretch_max);
      if (!(t.player_decay > 0.0 && t.player_decay < 1.0) || !(t.kickable_margin > 0.0) || !(t.player_size > 0.0)) continue;
      const double real_speed_max = t.effort_max * t.dash_power_rate * s.max_dash_power / (1.0 - t.player_decay);
      if (real_speed_max > 0.75 && real_speed_max <= t.player_speed_max) break;
      t = base;                                           // exhausted tries fall back to the default type
    }
    c->player_types[id] = t;
  }
  return S2D_OK;
}

S2D_API void s2d_match_default_config(S2DMatchConfig* c) {
  if (!c) return;
  S2DConfig base; s2d_default_config(&base);
  std::memset(c, 0, sizeof *c);
  c->abi_version = S2D_ABI_VERSION; c->struct_bytes = (uint32_t)sizeof(S2DMatchConfig);
  c->sp = base.sp;
  S2DMatchParams& m = c->mp;   // rcssserver stock values (EXT)
  m.kick_power_rate = 0.027; m.kickable_margin = 0.7; m.kick_rand = 0.1; m.max_power = 100.0; m.min_power = -100.0;
  m.tackle_dist = 2.0; m.tackle_back_dist = 0.0; m.tackle_width = 1.25; m.tackle_power_rate = 0.027;
  m.max_tackle_power = 100.0; m.max_back_tackle_power = 0.0;
  m.goal_width = 14.02; m.offside_active_area_size = 2.5; m.free_kick_distance = 9.15;
  m.tackle_cycles = 10; m.half_time_cycles = 3000; m.nr_normal_halfs = 2; m.drop_ball_time = 100; m.use_offside = 1;
  m.catch_ban_cycle = 5; m.catchable_area_l = 1.2; m.catch_area_w = 1.0; m.catch_probability = 1.0;
  m.max_catch_angle = 90.0; m.min_catch_angle = -90.0; m.penalty_area_length = 16.5; m.penalty_area_half_width = 20.16;
  m.goalie_max_moves = 2; m.after_goal_wait = 50;
  m.kick_off_wait = 0; m.back_passes = 1; m.free_kick_faults = 1;
  m.stopped_clock = 1; m.announce_wait = 30; m.foul_cycles = 5; m.foul_detect_probability = 0.5;
  m.nr_extra_halfs = S2D_STOCK_EXTRA_HALFS; m.extra_half_cycles = 1000; m.golden_goal = 0;
  m.penalty_shoot_outs = S2D_STOCK_SHOOT_OUTS; m.pen_before_setup_wait = 10; m.pen_ready_wait = 10; m.pen_taken_wait = 150; m.pen_nr_kicks = 5;
  m.pen_max_extra_kicks = 5; m.pen_dist_x = 42.5;
  m.pen_allow_mult_kicks = 1; m.pen_random_winner = 0;
  m.illegal_defense_number = 0; m.illegal_defense_duration = 20; m.illegal_defense_dist_x = 16.5; m.illegal_defense_width = 40.32;
  c->seed = 0x5EEDull; c->env_id_offset = 0; c->auto_reset = 1; c->noise = 0;
  for (int t = 0; t < S2D_MATCH_PLAYER_TYPES; ++t) c->player_types[t] = m_default_type(c->sp, m);   // homogeneous
}

S2D_API int s2d_match_validate_config(const S2DMatchConfig* c) {
  if (!c) return mfail(S2D_EINVAL, "config is NULL");
  if (c->abi_version != S2D_ABI_VERSION) return mfail(S2D_EINVAL, "config.abi_version mismatch");
  if (c->struct_bytes != sizeof(S2DMatchConfig)) return mfail(S2D_EINVAL, "config.struct_bytes != sizeof(S2DMatchConfig)");
  if (!(c->sp.pitch_half_length > 0) || !(c->sp.pitch_half_width > 0)) return mfail(S2D_EINVAL, "pitch extents must be > 0");
  if (!(c->mp.kickable_margin > 0) || !(c->mp.max_power > 0) || !(c->mp.tackle_width > 0))
    return mfail(S2D_EINVAL, "kickable_margin, max_power and tackle_width must be > 0");
  if (c->mp.half_time_cycles < 1 || c->mp.nr_normal_halfs < 1) return mfail(S2D_EINVAL, "half_time_cycles and nr_normal_halfs must be >= 1");
  if (c->mp.tackle_cycles < 0 || c->mp.drop_ball_time < 0) return mfail(S2D_EINVAL, "tackle_cycles / drop_ball_time must be >= 0");
  if (c->env_id_offset < 0) return mfail(S2D_EINVAL, "env_id_offset must be >= 0");
  if (c->mp.goalie_max_moves < 0 || c->mp.after_goal_wait < 0 || c->mp.kick_off_wait < 0)
    return mfail(S2D_EINVAL, "goalie_max_moves / after_goal_wait / kick_off_wait must be >= 0");
  if (c->mp.catch_ban_cycle < 0 || !(c->mp.catch_area_w > 0) || !(c->mp.catchable_area_l > 0))
    return mfail(S2D_EINVAL, "catch_ban_cycle must be >= 0, catch_area_w and catchable_area_l > 0");
  if (c->mp.announce_wait < 0 || c->mp.foul_cycles < 0 || !(c->mp.foul_detect_probability >= 0 && c->mp.foul_detect_probability <= 1))
    return mfail(S2D_EINVAL, "announce_wait / foul_cycles must be >= 0, foul_detect_probability in [0, 1]");
  if (c->mp.nr_extra_halfs < 0 || (c->mp.nr_extra_halfs > 0 && c->mp.extra_half_cycles < 1))
    return mfail(S2D_EINVAL, "nr_extra_halfs must be >= 0 and extra_half_cycles >= 1 when extra halves are played");
  if (c->mp.pen_before_setup_wait < 0 || c->mp.pen_ready_wait < 0 || c->mp.pen_taken_wait < 0 || c->mp.pen_nr_kicks < 1 ||
      c->mp.pen_max_extra_kicks < 0 || c->mp.pen_nr_kicks + c->mp.pen_max_extra_kicks > 15)
    return mfail(S2D_EINVAL, "pen_*_wait must be >= 0, pen_nr_kicks >= 1, pen_max_extra_kicks >= 0 and their sum <= 15");
  if (c->mp.illegal_defense_number < 0 || c->mp.illegal_defense_duration < 1 || c->mp.illegal_defense_duration > 255)
    return mfail(S2D_EINVAL, "illegal_defense_number must be >= 0 and illegal_defense_duration in [1, 255]");
  for (int i = 0; i < S2D_MATCH_PLAYERS; ++i)
    if (c->player_type_id[i] < 0 || c->player_type_id[i] >= S2D_MATCH_PLAYER_TYPES)
      return mfail(S2D_EINVAL, "player_type_id entries must be in [0, 18)");
  for (int t = 0; t < S2D_MATCH_PLAYER_TYPES; ++t) {
    const S2DPlayerType& y = c->player_types[t];
    if (!(y.player_decay >= 0 && y.player_decay <= 1) || !(y.kickable_margin > 0) || !(y.player_size > 0) ||
        !(y.player_speed_max > 0))
      return mfail(S2D_EINVAL, "player_types: decay must be in [0,1], kickable_margin / player_size / player_speed_max > 0");
  }
  return S2D_OK;
}

static void mparams_from_config(const S2DMatchConfig& c, MParams& p, float (*ptab)[kHalf]) {
  const S2DServerParams& s = c.sp; const S2DMatchParams& m = c.mp;
  std::memset(&p, 0, sizeof p);
  p.half_l = (float)s.pitch_half_length; p.half_w = (float)s.pitch_half_width;
  p.ball_size = (float)s.ball_size;
  p.player_rand = (float)s.player_rand; p.ball_rand = (float)s.ball_rand;
  p.player_accel_max = (float)s.player_accel_max; p.player_accel_max2 = p.player_accel_max * p.player_accel_max;
  p.ball_speed_max = (float)s.ball_speed_max; p.ball_speed_max2 = p.ball_speed_max * p.ball_speed_max;
  p.ball_accel_max = (float)s.ball_accel_max; p.ball_accel_max2 = p.ball_accel_max * p.ball_accel_max;
  p.stamina_max = (float)s.stamina_max; p.stamina_capacity = (float)s.stamina_capacity;
  p.recover_init = (float)s.recover_init; p.recover_dec_thr_value = (float)(s.recover_dec_thr * s.stamina_max);
  p.recover_min = (float)s.recover_min; p.recover_dec = (float)s.recover_dec;
  p.effort_dec_thr_value = (float)(s.effort_dec_thr * s.stamina_max); p.effort_dec = (float)s.effort_dec;
  p.effort_inc_thr_value = (float)(s.effort_inc_thr * s.stamina_max); p.effort_inc = (float)s.effort_inc;
  p.max_dash_power = (float)s.max_dash_power;
  p.min_dash_power = (float)s.min_dash_power; p.max_dash_angle = (float)s.max_dash_angle;
  p.min_dash_angle = (float)s.min_dash_angle; p.dash_angle_step = (float)s.dash_angle_step;
  p.inv_dash_angle_step = s.dash_angle_step > 0 ? (float)(1.0 / s.dash_angle_step) : 0.0f;
  p.side_dash_rate = (float)s.side_dash_rate; p.back_dash_rate = (float)s.back_dash_rate;
  p.max_moment = (float)s.max_moment; p.min_moment = (float)s.min_moment;
  p.collision_vel_rate = (float)s.collision_vel_rate;
  p.max_power = (float)m.max_power; p.min_power = (float)m.min_power;
  p.inv_max_power = (float)(1.0 / m.max_power);
  p.tackle_dist = (float)m.tackle_dist; p.tackle_back_dist = (float)m.tackle_back_dist;
  p.tackle_width = (float)m.tackle_width; p.tackle_power_rate = (float)m.tackle_power_rate;
  p.max_tackle_power = (float)m.max_tackle_power; p.max_back_tackle_power = (float)m.max_back_tackle_power;
  {
    const double td = m.tackle_dist > m.tackle_back_dist ? m.tackle_dist : m.tackle_back_dist;
    p.tackle_reach2 = (float)(1.01 * (td * td + m.tackle_width * m.tackle_width));
  }
  p.goal_half_width = (float)(m.goal_width * 0.5);
  p.offside_area2 = (float)(m.offside_active_area_size * m.offside_active_area_size);
  p.free_kick_distance = (float)m.free_kick_distance;
  p.inv_speed_decay = (float)(1.0 / (s.ball_speed_max * s.ball_decay));
  p.catch_half_w = (float)(m.catch_area_w * 0.5); p.catch_probability = (float)m.catch_probability;
  p.max_catch_angle = (float)m.max_catch_angle; p.min_catch_angle = (float)m.min_catch_angle;
  p.pen_x = (float)(s.pitch_half_length - m.penalty_area_length); p.pen_half_w = (float)m.penalty_area_half_width;
  p.tackle_cycles = m.tackle_cycles; p.half_time_cycles = m.half_time_cycles;
  p.nr_normal_halfs = m.nr_normal_halfs; p.drop_ball_time = m.drop_ball_time; p.use_offside = m.use_offside;
  p.catch_ban_cycle = m.catch_ban_cycle; p.goalie_max_moves = m.goalie_max_moves; p.after_goal_wait = m.after_goal_wait;
  p.kick_off_wait = m.kick_off_wait; p.back_passes = m.back_passes; p.free_kick_faults = m.free_kick_faults;
  p.stopped_clock = m.stopped_clock; p.announce_wait = m.announce_wait; p.foul_cycles = m.foul_cycles;
  p.foul_detect_probability = (float)m.foul_detect_probability;
  p.nr_extra_halfs = m.nr_extra_halfs; p.extra_half_cycles = m.extra_half_cycles; p.golden_goal = m.golden_goal != 0;
  p.penalty_shoot_outs = m.penalty_shoot_outs != 0; p.pen_before_setup_wait = m.pen_before_setup_wait; p.pen_ready_wait = m.pen_ready_wait;
  p.pen_taken_wait = m.pen_taken_wait; p.pen_nr_kicks = m.pen_nr_kicks; p.pen_max_extra_kicks = m.pen_max_extra_kicks;
  p.pen_spot_x = (float)(s.pitch_half_length - m.pen_dist_x);
  p.illegal_defense_number = m.illegal_defense_number; p.illegal_defense_duration = m.illegal_defense_duration;
  p.pen_allow_mult_kicks = m.pen_allow_mult_kicks != 0; p.pen_random_winner = m.pen_random_winner != 0;
  p.ill_x = (float)(s.pitch_half_length - m.illegal_defense_dist_x); p.ill_half_w = (float)(m.illegal_defense_width * 0.5);
  p.total_cycles = m.half_time_cycles * m.nr_normal_halfs;
  p.end_cycles = p.total_cycles + (m.nr_extra_halfs > 0 ? m.extra_half_cycles * m.nr_extra_halfs : 0);
  p.auto_reset = c.auto_reset; p.noise = c.noise;
  p.seed_lo = (uint32_t)c.seed; p.seed_hi = (uint32_t)(c.seed >> 32);
  p.gid_lo = (uint32_t)(uint64_t)c.env_id_offset; p.gid_hi = (uint32_t)((uint64_t)c.env_id_offset >> 32);
  // per-slot table: column i = the PlayerType of player i, column 22 = the ball (size / decay rows)
  std::memset(ptab, 0, sizeof(float) * PT_WORDS * kHalf);
  for (int i = 0; i < NP; ++i) {
    const S2DPlayerType& t = c.player_types[c.player_type_id[i]];
    const float size = (float)t.player_size, margin = (float)t.kickable_margin;
    ptab[PT_SPEED_MAX][i] = (float)t.player_speed_max; ptab[PT_SPEED_MAX2][i] = ptab[PT_SPEED_MAX][i] * ptab[PT_SPEED_MAX][i];
    ptab[PT_STAMINA_INC][i] = (float)t.stamina_inc_max; ptab[PT_DECAY][i] = (float)t.player_decay;
    ptab[PT_INERTIA][i] = (float)t.inertia_moment; ptab[PT_DASH_RATE][i] = (float)t.dash_power_rate;
    ptab[PT_SIZE][i] = size; ptab[PT_INV_KICK_MARGIN][i] = (float)(1.0 / t.kickable_margin);
    {  // largest float T with sqrtf(T) <= kickable_area  (dist <= ka  <=>  dist^2 <= T)
      const float ka = size + p.ball_size + margin;
      float T = ka * ka;
      while (std::sqrt(T) > ka) T = std::nextafter(T, 0.0f);
      while (std::sqrt(std::nextafter(T, INFINITY)) <= ka) T = std::nextafter(T, INFINITY);
      ptab[PT_KICKABLE_AREA2][i] = T;
    }
    ptab[PT_KICK_RAND][i] = (float)t.kick_rand; ptab[PT_EXTRA_STAMINA][i] = (float)t.extra_stamina;
    ptab[PT_EFFORT_MAX][i] = (float)t.effort_max; ptab[PT_EFFORT_MIN][i] = (float)t.effort_min;
    ptab[PT_KICK_RATE][i] = (float)t.kick_power_rate;
    ptab[PT_CATCH_LEN][i] = (float)(m.catchable_area_l * t.catchable_area_l_stretch);
  }
  ptab[PT_SIZE][BALL] = p.ball_size; ptab[PT_DECAY][BALL] = (float)s.ball_decay;
}

// the configuration words of p, bit for bit, against MStock's constants
static bool m_is_stock(const MParams& p) {
  auto same = [](float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; };
  bool ok = true;
#define X(name) ok = ok && same(p.name, (float)MStock::name);
  M_CONFIG_FLOATS(X)
#undef X
#define X(name) ok = ok && p.name == (int)MStock::name;
  M_CONFIG_INTS(X)
#undef X
  return ok;
}

// ... all of them but the schedule words (MStockSched keeps those as variables)
static bool m_rules_are_stock(const MParams& p) {
  auto same = [](float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; };
  bool ok = true;
#define X(name) ok = ok && same(p.name, (float)MStockSched::name);
  M_CONFIG_FLOATS(X)
#undef X
  return ok && p.tackle_cycles == MStockSched::tackle_cycles && p.use_offside == MStockSched::use_offside &&
         p.catch_ban_cycle == MStockSched::catch_ban_cycle && p.goalie_max_moves == MStockSched::goalie_max_moves &&
         p.back_passes == MStockSched::back_passes && p.free_kick_faults == MStockSched::free_kick_faults &&
         p.stopped_clock == MStockSched::stopped_clock && p.foul_cycles == MStockSched::foul_cycles &&
         p.illegal_defense_number == MStockSched::illegal_defense_number && p.illegal_defense_duration == MStockSched::illegal_defense_duration &&
         p.pen_allow_mult_kicks == MStockSched::pen_allow_mult_kicks && p.pen_random_winner == MStockSched::pen_random_winner;
}

static bool m_types_are_stock(const float (*t)[kHalf]) {
  auto same = [](float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; };
  bool ok = same(t[PT_SIZE][BALL], MStock::ball_size) && same(t[PT_DECAY][BALL], MStockTypes::ball_decay);
  for (int i = 0; i < NP && ok; ++i) {
    ok = same(t[PT_SPEED_MAX][i], MStockTypes::speed_max) && same(t[PT_SPEED_MAX2][i], MStockTypes::speed_max2) &&
         same(t[PT_STAMINA_INC][i], MStockTypes::stamina_inc) && same(t[PT_DECAY][i], MStockTypes::decay) &&
         same(t[PT_INERTIA][i], MStockTypes::inertia) && same(t[PT_DASH_RATE][i], MStockTypes::dash_rate) &&
         same(t[PT_SIZE][i], MStockTypes::size) && same(t[PT_INV_KICK_MARGIN][i], MStockTypes::inv_kick_margin) &&
         same(t[PT_KICKABLE_AREA2][i], t[PT_KICKABLE_AREA2][0]) && same(t[PT_KICK_RAND][i], MStockTypes::kick_rand) &&
         same(t[PT_EXTRA_STAMINA][i], MStockTypes::extra_stamina) && same(t[PT_EFFORT_MAX][i], MStockTypes::effort_max) &&
         same(t[PT_EFFORT_MIN][i], MStockTypes::effort_min) && same(t[PT_KICK_RATE][i], MStockTypes::kick_rate) &&
         same(t[PT_CATCH_LEN][i], MStockTypes::catch_len);
  }
  return ok;
}

S2D_API size_t s2d_match_arena_bytes(const S2DMatchConfig* cfg, int64_t n_envs) {
  if (!cfg || n_envs <= 0) return 0;
  return m_layout(n_envs).total;
}

S2D_API int s2d_match_reset(S2DMatchHandle h, const uint8_t* mask_dev, void* stream) {
  if (!h) return mfail(S2D_EINVAL, "NULL handle");
  MDeviceGuard guard(h->device);
  hipLaunchKernelGGL(s2d_match_reset_kernel, dim3(m_grid(h->n)), dim3(kMBlock), 0, static_cast<hipStream_t>(stream), h->mp,
                     h->ptrs, h->n, mask_dev);
  MHIP_TRY(hipGetLastError());
  return S2D_OK;
}

S2D_API int s2d_match_create(const S2DMatchConfig* cfg, int64_t n_envs, int device, void* arena_dev, size_t arena_bytes,
                             void* stream, S2DMatchHandle* out) {
  if (!out) return mfail(S2D_EINVAL, "out handle is NULL");
  *out = nullptr;
  int rc = s2d_match_validate_config(cfg);
  if (rc != S2D_OK) return rc;
  if (n_envs <= 0 || n_envs > (int64_t)1 << 28) return mfail(S2D_EINVAL, "n_envs must be in [1, 2^28]");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return mfail(S2D_ENODEV, "no HIP device visible");
  if (device < 0 || device >= ndev) return mfail(S2D_EINVAL, "device index out of range");
  MDeviceGuard guard(device);
  if (!guard.ok) return mfail(S2D_EHIP, "hipSetDevice failed");
  MLayout L = m_layout(n_envs);
  S2DMatchEngine* h = new (std::nothrow) S2DMatchEngine();
  if (!h) return mfail(S2D_ENOMEM, "host allocation failed");
  h->cfg = *cfg; h->n = n_envs; h->stride = L.stride; h->device = device;
  mparams_from_config(*cfg, h->mp, h->ptab);
  std::memset(&h->atab, 0, sizeof h->atab);
  for (int i = 0; i < NP; ++i) {
    const S2DPlayerType& t = cfg->player_types[cfg->player_type_id[i]];
    h->atab.ka[i] = (float)t.player_size + h->mp.ball_size + (float)t.kickable_margin;   // as the kickable bound is derived
    h->atab.ka2[i] = h->ptab[PT_KICKABLE_AREA2][i]; h->atab.speed_max[i] = h->ptab[PT_SPEED_MAX][i];
    h->atab.kick_rate[i] = h->ptab[PT_KICK_RATE][i]; h->atab.inv_margin[i] = h->ptab[PT_INV_KICK_MARGIN][i];
    h->atab.size[i] = h->ptab[PT_SIZE][i]; h->atab.type_id[i] = (float)cfg->player_type_id[i];
  }
  h->atab.ball_size = h->mp.ball_size; h->atab.ball_decay = h->ptab[PT_DECAY][BALL];
  {                                                     // S2D_MATCH_GENERAL_KERNEL=1: the general instantiation whatever the configuration (tests, A/B)
    const char* general = std::getenv("S2D_MATCH_GENERAL_KERNEL");
    h->stock = m_is_stock(h->mp) && !(general && general[0] == '1');
    h->stock_types = h->stock && m_types_are_stock(h->ptab);
    h->stock_sched = !h->stock && m_rules_are_stock(h->mp) && m_types_are_stock(h->ptab) && !(general && general[0] == '1');
  }
  if (arena_dev) {
    if (arena_bytes < L.total) { delete h; return mfail(S2D_ENOMEM, "arena smaller than s2d_match_arena_bytes()"); }
    if (reinterpret_cast<uintptr_t>(arena_dev) & 255u) { delete h; return mfail(S2D_EINVAL, "arena must be 256-byte aligned"); }
    h->arena = static_cast<char*>(arena_dev); h->owns_arena = false;
  } else {
    void* pmem = nullptr;
    if (hipMalloc(&pmem, L.total) != hipSuccess) { delete h; return mfail(S2D_ENOMEM, "hipMalloc of the arena failed"); }
    h->arena = static_cast<char*>(pmem); h->owns_arena = true;
  }
  h->arena_bytes = L.total;
  float* obj = reinterpret_cast<float*>(h->arena + L.obj);
  int32_t* env = reinterpret_cast<int32_t*>(h->arena + L.env);
  const size_t os = (size_t)L.stride * SLOTS, es = (size_t)L.stride;
  S2DMatchBuffers& b = h->buf;
  b.n_envs = n_envs;
  b.x = obj + MF_X * os; b.y = obj + MF_Y * os; b.vx = obj + MF_VX * os; b.vy = obj + MF_VY * os; b.body = obj + MF_BODY * os;
  b.stamina = obj + MF_STAMINA * os; b.effort = obj + MF_EFFORT * os; b.recovery = obj + MF_RECOVERY * os;
  b.stamina_capacity = obj + MF_CAPACITY * os; b.tackle_cycles = reinterpret_cast<int32_t*>(obj + MF_TACKLE * os);
  b.catch_ban = reinterpret_cast<int32_t*>(obj + MF_CATCH_BAN * os);
  b.cycle = env + ME_CYCLE * es; b.mode = env + ME_MODE * es; b.mode_side = env + ME_MODE_SIDE * es;
  b.score_left = env + ME_SCORE_L * es; b.score_right = env + ME_SCORE_R * es; b.last_touch_side = env + ME_LAST_TOUCH * es;
  b.setplay_timer = env + ME_TIMER * es; b.offside_mask = env + ME_OFFSIDE * es;
  b.ball_holder = env + ME_HOLDER * es; b.goalie_moves = env + ME_MOVES * es;
  b.set_play_taker = env + ME_TAKER * es; b.last_kicker = env + ME_LAST_KICKER * es;
  b.stopped_cycle = env + ME_STOPPED * es; b.tick = env + ME_TICK * es;
  b.card = reinterpret_cast<int32_t*>(obj + MF_CARD * os);
  b.reward_left = reinterpret_cast<float*>(h->arena + L.reward);
  b.done = reinterpret_cast<uint8_t*>(h->arena + L.done);
  b.nearest_left = env + ME_NEAREST_L * es; b.nearest_right = env + ME_NEAREST_R * es;
  b.stats = reinterpret_cast<unsigned long long*>(h->arena + L.stats);
  h->ptrs = MPtrs{obj, env, b.reward_left, b.done, b.stats, (int64_t)os, (int64_t)es,
                  reinterpret_cast<const float*>(h->arena + L.ptab)};
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(h->arena, 0, L.total, st);
  // h->ptab lives as long as the handle, so the (possibly staged) copy may complete later
  if (e == hipSuccess) e = hipMemcpyAsync(h->arena + L.ptab, h->ptab, sizeof h->ptab, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(s2d_match_reset_kernel, dim3(m_grid(n_envs)), dim3(kMBlock), 0, st, h->mp, h->ptrs, h->n,
                       (const uint8_t*)nullptr);
    e = hipGetLastError();
  }
  if (e != hipSuccess) {
    std::string msg = std::string("arena initialisation: ") + hipGetErrorString(e);
    if (h->owns_arena) (void)hipFree(h->arena);
    delete h;
    return mfail(S2D_EHIP, msg);
  }
  *out = h;
  return S2D_OK;
}

S2D_API void s2d_match_destroy(S2DMatchHandle h) {
  if (!h) return;
  if (h->owns_arena && h->arena) { MDeviceGuard guard(h->device); (void)hipFree(h->arena); }
  if (h->net_frags) { MDeviceGuard guard(h->device); (void)hipFree(h->net_frags); }
  delete h;
}
S2D_API int s2d_match_buffers(S2DMatchHandle h, S2DMatchBuffers* out) {
  if (!h || !out) return mfail(S2D_EINVAL, "NULL argument");
  *out = h->buf;
  return S2D_OK;
}
S2D_API int s2d_match_buffer_offsets(S2DMatchHandle h, int64_t* offsets, int n_offsets) {
  if (!h || !offsets) return mfail(S2D_EINVAL, "NULL argument");
  const S2DMatchBuffers& b = h->buf;
  const void* ptrs[] = {b.x, b.y, b.vx, b.vy, b.body, b.stamina, b.effort, b.recovery, b.stamina_capacity, b.tackle_cycles,
                        b.catch_ban, b.cycle, b.mode, b.mode_side, b.score_left, b.score_right, b.last_touch_side, b.setplay_timer,
                        b.offside_mask, b.ball_holder, b.goalie_moves, b.set_play_taker, b.last_kicker, b.stopped_cycle, b.tick, b.card,
                        b.reward_left, b.done, b.nearest_left, b.nearest_right, b.stats};
  const int count = 1 + (int)(sizeof ptrs / sizeof ptrs[0]);
  if (n_offsets < count) return mfail(S2D_EINVAL, "offsets array too small (need 32)");
  offsets[0] = (int64_t)h->arena_bytes;
  for (int k = 1; k < count; ++k) offsets[k] = (int64_t)(static_cast<const char*>(ptrs[k - 1]) - h->arena);
  return S2D_OK;
}

// The caller's parameters (torch order: W1 [h1][in_dim], b1, W2 [h2][h1], b2, W3 [na][h2], b3; in_dim = 224 for the agent-row
// network, 192 for the see network) into the engine's fragment-order copy:
// W1's fragments [h1/16][in_dim/4][64], W2's [h2/16][h1/4][64], W3's [na16/16][h2/4][64] (rows past na zero), b1 | b2 | b3 (zero past na).
// Enqueued by every network launch, so that a captured graph repacks what the parameter buffer holds at replay.
__global__ __launch_bounds__(256) void s2d_match_net_pack_kernel(const float* __restrict__ params, int in_dim, int h1, int h2, int na,
                                                                 int na16, float* __restrict__ frags, int total) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int k1 = in_dim / 4;
  const int f1 = h1 / 16 * k1, f2 = h2 / 16 * (h1 / 4), f3 = na16 / 16 * (h2 / 4);
  const int o_b1 = in_dim * h1, o_w2 = o_b1 + h1, o_b2 = o_w2 + h2 * h1, o_w3 = o_b2 + h2, o_b3 = o_w3 + na * h2;
  float v = 0.0f;
  if (idx < (f1 + f2 + f3) * 64) {
    const int f = idx / 64, l = idx & 63, row = l & 15, kk = l >> 4;
    if (f < f1) {
      const int jt = f / k1, s = f - k1 * jt;
      v = params[(16 * jt + row) * in_dim + 4 * s + kk];
    } else if (f < f1 + f2) {
      const int g2 = f - f1, ks = h1 / 4, jt = g2 / ks, s = g2 - jt * ks;
      v = params[o_w2 + (16 * jt + row) * h1 + 4 * s + kk];
    } else {
      const int g3 = f - f1 - f2, ks = h2 / 4, jt = g3 / ks, s = g3 - jt * ks, j = 16 * jt + row;
      if (j < na) v = params[o_w3 + j * h2 + 4 * s + kk];
    }
  } else {
    const int j = idx - (f1 + f2 + f3) * 64;
    if (j < h1) v = params[o_b1 + j];
    else if (j < h1 + h2) v = params[o_b2 + j - h1];
    else if (j - h1 - h2 < na) v = params[o_b3 + j - h1 - h2];
  }
  frags[idx] = v;
}
static constexpr int kNetFragsMax = (64 / 16 * kNetK1 + 64 / 16 * (64 / 4) + 64 / 16 * (64 / 4)) * 64 + 64 + 64 + 64;
static_assert(kSeeK1 <= kNetK1, "the see network's copy fits the agent-row network's");

// words of W2 .. b3 in fragment order: what a pass stages into LDS
static int m_net_shared_words(int h1, int h2, int na16) { return (h2 / 16 * (h1 / 4) + na16 / 16 * (h2 / 4)) * 64 + h1 + h2 + na16; }
// One pass's network words (D = MNet, MNetOpp or MSee) from the caller's network, and the pack kernel that fills its copy `frags`.
template <class D> static void m_net_pass(D& d, const S2DMatchNet& net, int in_dim, float* frags, hipStream_t st) {
  d.h1 = net.h1; d.h2 = net.h2; d.na = net.n_actions; d.na16 = (d.na + 15) / 16 * 16;
  d.frags = frags; d.epsilon = net.epsilon; d.table = net.table;
  d.shared_words = m_net_shared_words(d.h1, d.h2, d.na16);
  const int total = (d.h1 / 16 * (in_dim / 4)) * 64 + d.shared_words;
  hipLaunchKernelGGL(s2d_match_net_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, st, net.params, in_dim, d.h1, d.h2, d.na, d.na16,
                     frags, total);
}
// the fields the see network shares with the agent-row ones
static S2DMatchNet m_see_as_net(const S2DMatchSeeNet& s) { return S2DMatchNet{s.h1, s.h2, s.n_actions, s.slot_mask, s.params, s.epsilon, s.table}; }

static bool m_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a && b && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
// actions_out != NULL without a table records today's controllers: every slot the caller's row, or every slot random (actions NULL).
// With a network set, or a row record asked for (obs_mask), the NET instantiation runs (after the pack kernel, when there is a network).
// With a see network set the SEE instantiation runs (agent_obs_out is then the see record, view_actions the other slots' view actions).
// agent_reward_out != NULL (an agent reward is set: the entry point has checked): the RW instantiation of the same launch, which
// lives in s2d_match_reward.hip -- the controller one (without a table: every slot the caller's row, or random) unless the launch
// is a network or policy one.
// With a see policy set the SEEPOL instantiation runs, which lives in s2d_match_see_policy.hip (logp_out: its record, or NULL).
// With a belief network set the BEL instantiation runs, which lives in s2d_match_belief_net.hip (belief_out: its row record, or
// NULL; obs_mask names the slots of both row records).
static int m_launch(S2DMatchHandle h, int n_steps, const float* actions, const S2DMatchRollout* out, void* stream,
                    float* actions_out = nullptr, int32_t* net_index_out = nullptr, uint32_t obs_mask = 0u,
                    float* agent_obs_out = nullptr, const float* view_actions = nullptr, float* logp_out = nullptr,
                    float* agent_reward_out = nullptr, float* belief_out = nullptr) {
  MRoll ro{nullptr, nullptr, nullptr, nullptr};
  if (out) ro = MRoll{out->obs, out->reward, out->mode, out->done};
  const hipStream_t st = static_cast<hipStream_t>(stream);
  constexpr uint32_t kAll = (1u << NP) - 1u;
  const MRole* const role = h->role;
  const uint32_t net_mask = h->has_see ? h->see.slot_mask : role[0].net.slot_mask | role[1].net.slot_mask;
  if (!agent_obs_out && !belief_out) obs_mask = 0u;
  if (h->has_ctl && !actions && ((h->ctl_random | h->ctl_script | net_mask) & kAll) != kAll)
    return mfail(S2D_EINVAL, "the controller table has external slots (S2D_CTL_EXTERNAL) but actions_dev is NULL");
  const MCtl ctl = h->has_ctl ? MCtl{h->ctl_random, h->ctl_script, actions_out} : MCtl{actions ? 0u : kAll, 0u, actions_out};
  const MCtlRw crw{ctl, MRw{h->rw.w, agent_reward_out, h->rw.chaser_only}};
  if (h->has_see) {
    if (h->has_bel) {                                      // refused before anything is launched, whichever entry point came here
      if ((net_mask | obs_mask) & ~h->bel_mask)            // (the kernel addresses a slot's row by its rank in belief_mask)
        return mfail(S2D_EINVAL, "a belief network is set: obs_mask must lie inside its belief_mask");
      // no record may lie over the state the kernel updates every cycle
      const size_t N = (size_t)h->n, T = (size_t)n_steps, k = (size_t)__builtin_popcount(obs_mask);
      const size_t state = N * (size_t)__builtin_popcount(h->bel_mask) * S2D_BELIEF_DIM * sizeof(float);
      const size_t rows = T * N * k * S2D_BELIEF_DIM * sizeof(float), slots = T * N * NP * sizeof(float);
      if (m_overlap(h->bel_rows, state, agent_obs_out, rows) || m_overlap(h->bel_rows, state, belief_out, rows) ||
          m_overlap(agent_obs_out, rows, belief_out, rows) || m_overlap(h->bel_rows, state, actions_out, 3 * slots) ||
          m_overlap(h->bel_rows, state, net_index_out, slots) || m_overlap(h->bel_rows, state, logp_out, slots))
        return mfail(S2D_EINVAL, "a record overlaps the belief state buffer (or see_out overlaps belief_out)");
    }
    MSeeArg sa;
    std::memset(&sa, 0, sizeof sa);
    MSee& nt = sa.net;
    nt.net_mask = net_mask; nt.obs_mask = obs_mask; nt.row_mask = net_mask | obs_mask;
    nt.net_index = net_index_out; nt.see_out = agent_obs_out; nt.view_actions = view_actions;
    const uint32_t keys[4] = {h->mp.seed_lo, h->mp.seed_hi, h->mp.gid_lo, h->mp.gid_hi};
    sa.sp = s2d_see::see_params(h->see.prm, keys);
    sa.vis = h->see.vis;
    if (net_mask) {
      MDeviceGuard guard(h->device);
      m_net_pass(nt, m_see_as_net(h->see), S2D_SEE_DIM, h->net_frags, st);
      MHIP_TRY(hipGetLastError());
    }
    if (h->has_bel) {                                      // the BEL instantiation: the same MSeeArg, the policy words, the belief words
      MBelArg ba;
      std::memset(&ba, 0, sizeof ba);
      ba.net = sa.net; ba.sp = sa.sp; ba.vis = sa.vis;
      ba.act = h->see_act; ba.det = h->see_det; ba.logp = logp_out;
      ba.head = h->bel_head; ba.bp = s2d_belief::belief_params(h->bel_prm);
      ba.belief = h->bel_rows; ba.belief_mask = h->bel_mask; ba.belief_out = belief_out; ba.done0 = h->buf.done;
      return s2d_match_internal_belief_net_launch(h, n_steps, actions, ro, st, ctl, ba);
    }
    if (h->see_pol) {                                      // the SEEPOL instantiation: the same MSeeArg plus the policy words
      MSeePolArg pa;
      std::memset(&pa, 0, sizeof pa);
      pa.net = sa.net; pa.sp = sa.sp; pa.vis = sa.vis;
      pa.act = h->see_act; pa.det = h->see_det; pa.logp = logp_out;
      return s2d_match_internal_see_policy_launch(h, n_steps, actions, ro, st, ctl, pa);
    }
    if (logp_out) {                                        // no see policy: the record is all zero
      MDeviceGuard guard(h->device);
      MHIP_TRY(hipMemsetAsync(logp_out, 0, (size_t)n_steps * (size_t)h->n * NP * sizeof(float), st));
    }
    return m_dispatch<true, true>(h, n_steps, actions, ro, st, ctl, sa);
  }
  if (logp_out && !(role[0].pol || role[1].pol)) {       // no policy network: the record is all zero
    MDeviceGuard guard(h->device);
    MHIP_TRY(hipMemsetAsync(logp_out, 0, (size_t)n_steps * (size_t)h->n * NP * sizeof(float), st));
  }
  if (net_mask || obs_mask || net_index_out) {
    MNetArg na;
    std::memset(&na, 0, sizeof na);
    MNet& nt = na.net;
    nt.obs_mask = obs_mask; nt.row_mask = net_mask | obs_mask;
    nt.net_index = net_index_out; nt.agent_obs = agent_obs_out;
    na.tab = h->atab;
    MPol pol;                                              // a role on a stochastic policy: each pass's kind, activation and word
    std::memset(&pol, 0, sizeof pol);
    pol.logp = logp_out;
    // The kernel's first pass is the network when one is set, else the opponent; its second pass the opponent beside a network.
    // Each role keeps its own half of the fragment copy, so which pass a network runs in changes no word it reads.
    const int first = role[S2D_MATCH_ROLE_NETWORK].set ? S2D_MATCH_ROLE_NETWORK : S2D_MATCH_ROLE_OPPONENT;
    const int passes = role[0].set + role[1].set;
    MDeviceGuard guard(h->device);
    for (int k = 0; k < passes; ++k) {
      const MRole& r = role[first + k];
      float* const frags = h->net_frags + (first + k) * kNetFragsMax;
      if (k == 0) { nt.net_mask = r.net.slot_mask; m_net_pass(nt, r.net, S2D_AGENT_OBS_DIM, frags, st); }
      else { nt.opp.mask = r.net.slot_mask; m_net_pass(nt.opp, r.net, S2D_AGENT_OBS_DIM, frags, st); }
      MHIP_TRY(hipGetLastError());
      if (r.pol) { pol.kind[k] = 1; pol.act[k] = r.act; pol.det[k] = r.det; }
    }
    if (pol.kind[0] || pol.kind[1]) {                      // the POL instantiation: the same MNetArg plus the policy words
      MPolArg pa;
      std::memset(&pa, 0, sizeof pa);
      pa.net = na.net; pa.tab = na.tab; pa.pol = pol;
      if (agent_reward_out) return s2d_match_internal_reward_launch(h, n_steps, actions, ro, st, crw, nullptr, &pa);
      return m_dispatch<true, true>(h, n_steps, actions, ro, st, ctl, pa);
    }
    if (agent_reward_out) return s2d_match_internal_reward_launch(h, n_steps, actions, ro, st, crw, &na, nullptr);
    return m_dispatch<true, true>(h, n_steps, actions, ro, st, ctl, na);
  }
  if (agent_reward_out) return s2d_match_internal_reward_launch(h, n_steps, actions, ro, st, crw, nullptr, nullptr);
  if (h->has_ctl || actions_out) return m_dispatch<true>(h, n_steps, actions, ro, st, ctl);
  return m_dispatch<false>(h, n_steps, actions, ro, st);
}
// "s2d_match_rollout_kernel<" variant [", " slot kind] [", agent reward"] ">"
S2D_API const char* s2d_match_kernel_name(S2DMatchHandle h) {
  if (!h) return "";
  constexpr int kKinds = 9;
  static const char* const kind_text[kKinds] = {"", ", controllers", ", network", ", two networks", ", policy network",
                                                ", two networks, policy", ", see network", ", see policy network", ", belief network"};
  static const std::array<std::string, 2 * 5 * kKinds> names = [] {
    std::array<std::string, 2 * 5 * kKinds> t;
    for (int v = 0; v < 5; ++v)
      for (int k = 0; k < kKinds; ++k) {
        const std::string stem = std::string("s2d_match_rollout_kernel<") + kVariant[v].text + kind_text[k];
        t[v * kKinds + k] = stem + ">";
        t[(5 + v) * kKinds + k] = stem + ", agent reward>";
      }
    return t;
  }();
  const int nets = h->role[0].set + h->role[1].set;
  const bool pol = h->role[0].pol || h->role[1].pol;
  const int kind = h->has_see ? (h->has_bel ? 8 : h->see_pol ? 7 : 6) : nets == 2 ? (pol ? 5 : 3) : nets == 1 ? (pol ? 4 : 2) : h->has_ctl ? 1 : 0;
  return names[((h->has_rw ? 5 : 0) + m_variant(h)) * kKinds + kind].c_str();
}
S2D_API int s2d_match_relative(S2DMatchHandle h, float* dist_dev, float* angle_dev, void* stream) {
  if (!h || !dist_dev || !angle_dev) return mfail(S2D_EINVAL, "NULL argument");
  MDeviceGuard guard(h->device);
  hipLaunchKernelGGL(s2d_match_relative_kernel, dim3(m_grid(h->n)), dim3(kMBlock), 0, static_cast<hipStream_t>(stream), h->ptrs,
                     h->n, dist_dev, angle_dev);
  MHIP_TRY(hipGetLastError());
  return S2D_OK;
}
S2D_API int s2d_match_agent_obs(S2DMatchHandle h, uint32_t slot_mask, float* obs_dev, void* stream) {
  if (!h || !obs_dev) return mfail(S2D_EINVAL, "NULL argument");
  if (slot_mask == 0u || (slot_mask >> NP) != 0u)
    return mfail(S2D_EINVAL, "slot_mask must be a non-empty set of bits 0..21 (0x3FFFFF = all agents)");
  if (reinterpret_cast<uintptr_t>(obs_dev) & 15u) return mfail(S2D_EINVAL, "agent observation buffer must be 16-byte aligned");
  MDeviceGuard guard(h->device);
  hipLaunchKernelGGL(s2d_match_agent_obs_kernel, dim3(m_grid(h->n)), dim3(kMBlock), 0, static_cast<hipStream_t>(stream), h->mp,
                     h->atab, h->ptrs, h->n, slot_mask, obs_dev);
  MHIP_TRY(hipGetLastError());
  return S2D_OK;
}
S2D_API int s2d_match_step(S2DMatchHandle h, const float* actions_dev, void* stream) {
  if (!h) return mfail(S2D_EINVAL, "NULL handle");
  return m_launch(h, 1, actions_dev, nullptr, stream);
}
// What the rollout entry points check alike, in the order they report it: the handle, n_steps, the obs buffer, the optional records
// `recs` (4-byte aligned), then the row record `rows` (agent_obs_out or see_out: 16-byte aligned, with a proper obs_mask).
// true: launch.  false: return *rc (an error, or S2D_OK for n_steps == 0).
struct MRecord { const void* ptr; const char* name; const char* type; };
static bool m_rollout_args(int* rc, S2DMatchHandle h, int n_steps, const S2DMatchRollout* out, std::initializer_list<MRecord> recs = {},
                           const void* rows = nullptr, const char* rows_name = "", uint32_t obs_mask = 0u) {
  const auto fail = [rc](const std::string& msg) { *rc = mfail(S2D_EINVAL, msg); return false; };
  if (!h) return fail("NULL handle");
  if (n_steps < 0) return fail("n_steps must be >= 0");
  if (out && out->obs && (reinterpret_cast<uintptr_t>(out->obs) & 15u)) return fail("rollout obs buffer must be 16-byte aligned");
  for (const MRecord& r : recs)
    if (reinterpret_cast<uintptr_t>(r.ptr) & 3u) return fail(std::string(r.name) + " must be 4-byte aligned (" + r.type + ")");
  if (rows) {
    if (obs_mask == 0u || (obs_mask >> NP) != 0u)
      return fail(std::string("obs_mask must be a non-empty set of bits 0..21 when ") + rows_name + " is given");
    if (reinterpret_cast<uintptr_t>(rows) & 15u) return fail(std::string(rows_name) + " must be 16-byte aligned");
  }
  *rc = S2D_OK;
  return n_steps != 0;
}
S2D_API int s2d_match_rollout(S2DMatchHandle h, int n_steps, const float* actions_dev, const S2DMatchRollout* out, void* stream) {
  int rc;
  if (!m_rollout_args(&rc, h, n_steps, out)) return rc;
  return m_launch(h, n_steps, actions_dev, out, stream);
}
S2D_API int s2d_match_set_controllers(S2DMatchHandle h, const uint8_t* ctl) {
  if (!h) return mfail(S2D_EINVAL, "NULL handle");
  if (!ctl) { h->has_ctl = false; h->ctl_random = 0u; h->ctl_script = 0u; return S2D_OK; }
  uint32_t rnd = 0u, scr = 0u;
  for (int i = 0; i < NP; ++i) {
    if (ctl[i] > S2D_CTL_SCRIPTED)
      return mfail(S2D_EINVAL, "controller code of slot " + std::to_string(i) + " is " + std::to_string((int)ctl[i]) +
                               " (S2D_CTL_EXTERNAL / RANDOM / SCRIPTED = 0 / 1 / 2)");
    if (ctl[i] == S2D_CTL_RANDOM) rnd |= 1u << i;
    if (ctl[i] == S2D_CTL_SCRIPTED) scr |= 1u << i;
  }
  h->has_ctl = true; h->ctl_random = rnd; h->ctl_script = scr;
  return S2D_OK;
}
S2D_API int s2d_match_rollout_ex(S2DMatchHandle h, int n_steps, const float* actions_dev, const S2DMatchRollout* out,
                                 float* actions_out_dev, void* stream) {
  int rc;
  if (!m_rollout_args(&rc, h, n_steps, out, {{actions_out_dev, "actions_out", "float"}})) return rc;
  return m_launch(h, n_steps, actions_dev, out, stream, actions_out_dev);
}

static int m_net_frags_alloc(S2DMatchHandle h) {
  if (h->net_frags) return S2D_OK;
  MDeviceGuard guard(h->device);
  void* pmem = nullptr;
  if (hipMalloc(&pmem, 2 * (size_t)kNetFragsMax * sizeof(float)) != hipSuccess) return mfail(S2D_ENOMEM, "hipMalloc of the network copy failed");
  h->net_frags = static_cast<float*>(pmem);
  return S2D_OK;
}
// What every network setter rejects.  what: "network", "policy network" or "see network"; word / word_name: the network's device
// word beside the table (epsilon or deterministic); other_mask: the slots of the engine's other agent-row network (0: none set).
// empty_ok (the see network): an empty slot_mask is a record-only network, whose pointers are not read.
static int m_net_validate(const std::string& what, const S2DMatchNet& net, const void* word, const char* word_name, bool empty_ok,
                          uint32_t other_mask) {
  const auto width_ok = [](int w) { return w == 16 || w == 32 || w == 48 || w == 64; };
  if (!width_ok(net.h1) || !width_ok(net.h2)) return mfail(S2D_EINVAL, what + " hidden widths must be 16, 32, 48 or 64");
  if (net.n_actions < 1 || net.n_actions > 64) return mfail(S2D_EINVAL, what + " n_actions must be in [1, 64]");
  if ((net.slot_mask == 0u && !empty_ok) || (net.slot_mask >> NP) != 0u)
    return mfail(S2D_EINVAL, what + " slot_mask must be a " + (empty_ok ? "" : "non-empty ") + "set of bits 0..21");
  if (net.slot_mask & other_mask)
    return mfail(S2D_EINVAL, what + " slot_mask overlaps the network of the engine's other role (a slot belongs to one network)");
  if (net.slot_mask == 0u) return S2D_OK;
  if (!net.params || (reinterpret_cast<uintptr_t>(net.params) & 15u))
    return mfail(S2D_EINVAL, what + " params must be a non-NULL, 16-byte aligned device pointer");
  if (!word || !net.table || ((reinterpret_cast<uintptr_t>(word) | reinterpret_cast<uintptr_t>(net.table)) & 3u))
    return mfail(S2D_EINVAL, what + " " + word_name + " and table must be non-NULL, 4-byte aligned device pointers");
  return S2D_OK;
}
// Who excludes whom, for all five setters.  `slot`: a role, or kSlotSee (a see network of either kind).  The see network is the engine's only one: the opponent role
// refuses beside it, the network role replaces it, and setting it clears both roles (policy networks too).
static constexpr int kSlotSee = 2;
static int m_slot_admit(S2DMatchHandle h, int slot) {
  if (slot == S2D_MATCH_ROLE_OPPONENT && h->has_see)
    return mfail(S2D_EINVAL, "a see network is set: the see network stays single (clear it first)");
  return S2D_OK;
}
static void m_slot_clear(S2DMatchHandle h, int slot) {   // a slot without a network, whatever kind it held
  if (slot == kSlotSee) {
    h->has_see = false; h->see = S2DMatchSeeNet{}; h->see_pol = false; h->see_act = 0; h->see_det = nullptr;
    h->has_bel = false; h->bel_head = 0; h->bel_prm = S2DBeliefParams{}; h->bel_rows = nullptr; h->bel_mask = 0u;
  }
  else h->role[slot] = MRole{};
}
static void m_slot_displace(S2DMatchHandle h, int slot) {
  if (slot == kSlotSee) { m_slot_clear(h, S2D_MATCH_ROLE_NETWORK); m_slot_clear(h, S2D_MATCH_ROLE_OPPONENT); }
  if (slot == S2D_MATCH_ROLE_NETWORK) m_slot_clear(h, kSlotSee);
}
// an agent-row network into a role: r = the role's new state (set, with the caller's pointers)
static int m_role_set(S2DMatchHandle h, int role, const MRole& r) {
  if (int rc = m_slot_admit(h, role); rc != S2D_OK) return rc;
  if (r.pol && r.act != 0 && r.act != 1) return mfail(S2D_EINVAL, "policy network activation must be 0 (relu) or 1 (tanh)");
  const void* const word = r.pol ? static_cast<const void*>(r.det) : r.net.epsilon;
  const uint32_t other_mask = h->role[role ^ 1].net.slot_mask;
  if (int rc = m_net_validate(r.pol ? "policy network" : "network", r.net, word, r.pol ? "deterministic" : "epsilon", false, other_mask);
      rc != S2D_OK)
    return rc;
  if (int rc = m_net_frags_alloc(h); rc != S2D_OK) return rc;
  h->role[role] = r;                                   // (whatever kind the role held goes)
  m_slot_displace(h, role);
  return S2D_OK;
}
S2D_API int s2d_match_set_network(S2DMatchHandle h, const S2DMatchNet* net) {
  if (!h) return mfail(S2D_EINVAL, "NULL handle");
  if (!net) { m_slot_clear(h, S2D_MATCH_ROLE_NETWORK); return S2D_OK; }
  return m_role_set(h, S2D_MATCH_ROLE_NETWORK, MRole{true, *net});
}
S2D_API int s2d_match_set_opponent_network(S2DMatchHandle h, const S2DMatchNet* net) {
  if (!h) return mfail(S2D_EINVAL, "NULL handle");
  if (!net) { m_slot_clear(h, S2D_MATCH_ROLE_OPPONENT); return S2D_OK; }
  return m_role_set(h, S2D_MATCH_ROLE_OPPONENT, MRole{true, *net});
}
S2D_API int s2d_match_set_policy_network(S2DMatchHandle h, int role, const S2DMatchPolicyNet* net) {
  if (!h) return mfail(S2D_EINVAL, "NULL handle");
  if (role != S2D_MATCH_ROLE_NETWORK && role != S2D_MATCH_ROLE_OPPONENT)
    return mfail(S2D_EINVAL, "policy network role must be S2D_MATCH_ROLE_NETWORK (0) or S2D_MATCH_ROLE_OPPONENT (1)");
  if (!net) { m_slot_clear(h, role); return S2D_OK; }
  // a policy keeps its words in the same S2DMatchNet, epsilon NULL
  const S2DMatchNet as_net{net->h1, net->h2, net->n_actions, net->slot_mask, net->params, nullptr, net->table};
  return m_role_set(h, role, MRole{true, as_net, true, net->activation, net->deterministic});
}
// a see network of either kind into the see slot: word / word_name as for m_net_validate; pol: a policy (act, det: its words)
static int m_see_set(S2DMatchHandle h, const S2DMatchSeeNet* net, const std::string& what, const void* word, const char* word_name,
                     bool pol, int act, const uint32_t* det) {
  if (h->has_rw) return mfail(S2D_EINVAL, "an agent reward is set: the see network's cycle kernel has none (clear it first)");
  if (pol && act != 0 && act != 1) return mfail(S2D_EINVAL, what + " activation must be 0 (relu) or 1 (tanh)");
  if (int rc = m_net_validate(what, m_see_as_net(*net), word, word_name, !pol, 0u); rc != S2D_OK) return rc;
  if (!net->vis.neck || !net->vis.view_width || !net->vis.see_wait) return mfail(S2D_EINVAL, "NULL vision plane");
  if ((reinterpret_cast<uintptr_t>(net->vis.neck) | reinterpret_cast<uintptr_t>(net->vis.view_width) |
       reinterpret_cast<uintptr_t>(net->vis.see_wait)) & 3u)
    return mfail(S2D_EINVAL, "the vision planes must be 4-byte aligned");
  if (int rc = s2d_match_vision_validate(&net->prm); rc != S2D_OK) return rc;
  if (net->slot_mask != 0u)
    if (int rc = m_net_frags_alloc(h); rc != S2D_OK) return rc;
  m_slot_clear(h, kSlotSee);                            // (a belief network's words go with whatever the slot held)
  h->see = *net; h->has_see = true;
  h->see_pol = pol; h->see_act = pol ? act : 0; h->see_det = pol ? det : nullptr;
  m_slot_displace(h, kSlotSee);
  return S2D_OK;
}
S2D_API int s2d_match_set_see_network(S2DMatchHandle h, const S2DMatchSeeNet* net) {
  if (!h) return mfail(S2D_EINVAL, "NULL handle");
  if (!net) { m_slot_clear(h, kSlotSee); return S2D_OK; }
  return m_see_set(h, net, "see network", net->epsilon, "epsilon", false, 0, nullptr);
}
S2D_API int s2d_match_set_see_policy_network(S2DMatchHandle h, const S2DMatchSeePolicyNet* net) {
  if (!h) return mfail(S2D_EINVAL, "NULL handle");
  if (!net) { m_slot_clear(h, kSlotSee); return S2D_OK; }
  // a see policy keeps its words in the same S2DMatchSeeNet, epsilon NULL
  const S2DMatchSeeNet as_see{net->h1, net->h2, net->n_actions, net->slot_mask, net->params, nullptr, net->table, net->prm, net->vis};
  return m_see_set(h, &as_see, "see policy network", net->deterministic, "deterministic", true, net->activation, net->deterministic);
}
// The belief network: the see slot's words through m_see_set (every check of the see policy's setter, with the head's own device
// word), then the belief words.  All checks come first: a refusal leaves the engine as it was.
S2D_API int s2d_match_set_belief_network(S2DMatchHandle h, const S2DMatchBeliefNet* net) {
  if (!h) return mfail(S2D_EINVAL, "NULL handle");
  if (!net) { m_slot_clear(h, kSlotSee); return S2D_OK; }
  const std::string what = "belief network";
  if (net->head != 0 && net->head != 1) return mfail(S2D_EINVAL, what + " head must be 0 (epsilon-greedy Q-network) or 1 (categorical policy)");
  if (net->head == 0 && net->activation != 0) return mfail(S2D_EINVAL, what + " head 0 (the Q-network) takes activation 0 (relu) only");
  if (!net->belief || (reinterpret_cast<uintptr_t>(net->belief) & 15u))
    return mfail(S2D_EINVAL, what + " belief must be a non-NULL, 16-byte aligned device pointer");
  if (net->belief_mask == 0u || (net->belief_mask >> NP) != 0u)
    return mfail(S2D_EINVAL, what + " belief_mask must be a non-empty set of bits 0..21");
  if ((net->slot_mask >> NP) == 0u && (net->slot_mask & ~net->belief_mask))
    return mfail(S2D_EINVAL, what + " slot_mask must lie inside belief_mask (a slot's row is its rank in belief_mask)");
  if (int rc = s2d_match_belief_validate(&net->belief_prm); rc != S2D_OK) return rc;
  const void* const word = net->head ? static_cast<const void*>(net->deterministic) : static_cast<const void*>(net->epsilon);
  const S2DMatchSeeNet as_see{net->h1, net->h2, net->n_actions, net->slot_mask, net->params, net->head ? nullptr : net->epsilon,
                              net->table, net->prm, net->vis};
  if (int rc = m_see_set(h, &as_see, what, word, net->head ? "deterministic" : "epsilon", true, net->activation,
                         net->head ? net->deterministic : nullptr);
      rc != S2D_OK)
    return rc;
  h->see_pol = false;                                    // (the see slot holds a belief network: its launches are the BEL kernels')
  h->has_bel = true; h->bel_head = net->head; h->bel_prm = net->belief_prm; h->bel_rows = net->belief; h->bel_mask = net->belief_mask;
  return S2D_OK;
}
S2D_API int s2d_match_rollout_belief(S2DMatchHandle h, int n_steps, const float* actions_dev, const float* view_actions_dev,
                                     const S2DMatchRollout* out, float* actions_out_dev, int32_t* net_index_out_dev,
                                     float* logp_out_dev, uint32_t obs_mask, float* see_out_dev, float* belief_out_dev, void* stream) {
  if (h && !h->has_bel) return mfail(S2D_EINVAL, "s2d_match_rollout_belief needs a belief network (s2d_match_set_belief_network)");
  if (reinterpret_cast<uintptr_t>(belief_out_dev) & 15u) return mfail(S2D_EINVAL, "belief_out must be 16-byte aligned");
  int rc;
  const bool go = m_rollout_args(&rc, h, n_steps, out, {{actions_out_dev, "actions_out", "float"}, {view_actions_dev, "view_actions", "float"},
                                                        {net_index_out_dev, "net_index_out", "int32"}, {logp_out_dev, "logp_out", "float"}},
                                 see_out_dev ? see_out_dev : belief_out_dev, see_out_dev ? "see_out" : "belief_out", obs_mask);
  if (rc != S2D_OK) return rc;
  if ((see_out_dev || belief_out_dev) && (obs_mask & ~h->bel_mask))
    return mfail(S2D_EINVAL, "obs_mask must lie inside the belief network's belief_mask");
  if (!go) return rc;
  return m_launch(h, n_steps, actions_dev, out, stream, actions_out_dev, net_index_out_dev, obs_mask, see_out_dev, view_actions_dev,
                  logp_out_dev, nullptr, belief_out_dev);
}
S2D_API int s2d_match_rollout_see(S2DMatchHandle h, int n_steps, const float* actions_dev, const float* view_actions_dev,
                                  const S2DMatchRollout* out, float* actions_out_dev, int32_t* net_index_out_dev, uint32_t obs_mask,
                                  float* see_out_dev, void* stream) {
  if (h && !h->has_see) return mfail(S2D_EINVAL, "s2d_match_rollout_see needs a see network (s2d_match_set_see_network)");
  int rc;
  if (!m_rollout_args(&rc, h, n_steps, out, {{actions_out_dev, "actions_out", "float"}, {view_actions_dev, "view_actions", "float"},
                                             {net_index_out_dev, "net_index_out", "int32"}}, see_out_dev, "see_out", obs_mask))
    return rc;
  return m_launch(h, n_steps, actions_dev, out, stream, actions_out_dev, net_index_out_dev, obs_mask, see_out_dev, view_actions_dev);
}
S2D_API int s2d_match_rollout_see_policy(S2DMatchHandle h, int n_steps, const float* actions_dev, const float* view_actions_dev,
                                         const S2DMatchRollout* out, float* actions_out_dev, int32_t* net_index_out_dev,
                                         float* logp_out_dev, uint32_t obs_mask, float* see_out_dev, void* stream) {
  if (h && !h->has_see)
    return mfail(S2D_EINVAL, "s2d_match_rollout_see_policy needs a see network (s2d_match_set_see_policy_network, s2d_match_set_see_network)");
  int rc;
  if (!m_rollout_args(&rc, h, n_steps, out, {{actions_out_dev, "actions_out", "float"}, {view_actions_dev, "view_actions", "float"},
                                             {net_index_out_dev, "net_index_out", "int32"}, {logp_out_dev, "logp_out", "float"}},
                      see_out_dev, "see_out", obs_mask))
    return rc;
  return m_launch(h, n_steps, actions_dev, out, stream, actions_out_dev, net_index_out_dev, obs_mask, see_out_dev, view_actions_dev,
                  logp_out_dev);
}
S2D_API int s2d_match_rollout_net(S2DMatchHandle h, int n_steps, const float* actions_dev, const S2DMatchRollout* out,
                                  float* actions_out_dev, int32_t* net_index_out_dev, uint32_t obs_mask, float* agent_obs_out_dev,
                                  void* stream) {
  if (h && h->has_see) return mfail(S2D_EINVAL, "a see network is set: use s2d_match_rollout_see (the agent-row record is not built)");
  int rc;
  if (!m_rollout_args(&rc, h, n_steps, out, {{actions_out_dev, "actions_out", "float"}, {net_index_out_dev, "net_index_out", "int32"}},
                      agent_obs_out_dev, "agent_obs_out", obs_mask))
    return rc;
  return m_launch(h, n_steps, actions_dev, out, stream, actions_out_dev, net_index_out_dev, obs_mask, agent_obs_out_dev);
}
S2D_API int s2d_match_rollout_policy(S2DMatchHandle h, int n_steps, const float* actions_dev, const S2DMatchRollout* out,
                                     float* actions_out_dev, int32_t* net_index_out_dev, float* logp_out_dev, uint32_t obs_mask,
                                     float* agent_obs_out_dev, void* stream) {
  if (h && h->has_see) return mfail(S2D_EINVAL, "a see network is set: use s2d_match_rollout_see, or s2d_match_rollout_see_policy for a see policy's log-probabilities");
  int rc;
  if (!m_rollout_args(&rc, h, n_steps, out, {{actions_out_dev, "actions_out", "float"}, {net_index_out_dev, "net_index_out", "int32"},
                                             {logp_out_dev, "logp_out", "float"}}, agent_obs_out_dev, "agent_obs_out", obs_mask))
    return rc;
  return m_launch(h, n_steps, actions_dev, out, stream, actions_out_dev, net_index_out_dev, obs_mask, agent_obs_out_dev, nullptr,
                  logp_out_dev);
}
S2D_API int s2d_match_set_agent_reward(S2DMatchHandle h, const S2DMatchAgentReward* rw) {
  if (!h) return mfail(S2D_EINVAL, "NULL handle");
  if (!rw) { h->has_rw = false; h->rw = MRw{nullptr, nullptr, 0}; return S2D_OK; }
  if (!rw->weights || (reinterpret_cast<uintptr_t>(rw->weights) & 3u))
    return mfail(S2D_EINVAL, "agent reward weights must be a non-NULL, 4-byte aligned device pointer (float[S2D_MATCH_REWARD_TERMS])");
  if (rw->chaser_only != 0 && rw->chaser_only != 1) return mfail(S2D_EINVAL, "agent reward chaser_only must be 0 or 1");
  if (h->has_see) return mfail(S2D_EINVAL, "a see network is set: the see network's cycle kernel has no agent reward (clear it first)");
  h->has_rw = true; h->rw = MRw{rw->weights, nullptr, rw->chaser_only};
  return S2D_OK;
}
S2D_API int s2d_match_rollout_reward(S2DMatchHandle h, int n_steps, const float* actions_dev, const S2DMatchRollout* out,
                                     float* actions_out_dev, int32_t* net_index_out_dev, float* logp_out_dev, uint32_t obs_mask,
                                     float* agent_obs_out_dev, float* agent_reward_out_dev, void* stream) {
  if (h && h->has_see) return mfail(S2D_EINVAL, "a see network is set: use s2d_match_rollout_see (the see network has no agent reward)");
  if (h && agent_reward_out_dev && !h->has_rw)
    return mfail(S2D_EINVAL, "agent_reward_out needs an agent reward (s2d_match_set_agent_reward)");
  int rc;
  if (!m_rollout_args(&rc, h, n_steps, out, {{actions_out_dev, "actions_out", "float"}, {net_index_out_dev, "net_index_out", "int32"},
                                             {logp_out_dev, "logp_out", "float"}, {agent_reward_out_dev, "agent_reward_out", "float"}},
                      agent_obs_out_dev, "agent_obs_out", obs_mask))
    return rc;
  return m_launch(h, n_steps, actions_dev, out, stream, actions_out_dev, net_index_out_dev, obs_mask, agent_obs_out_dev, nullptr,
                  logp_out_dev, agent_reward_out_dev);
}

// What the vision layer (s2d_see.hip, a translation unit of its own) needs of an engine beyond s2d_match_buffers(): the Philox key
// and id words of its draws and its device.  Library-internal (hidden visibility): not part of the C ABI.
extern "C" int s2d_match_internal_keys(S2DMatchHandle h, uint32_t keys[4], int* device) {
  if (!h) return S2D_EINVAL;
  keys[0] = h->mp.seed_lo; keys[1] = h->mp.seed_hi; keys[2] = h->mp.gid_lo; keys[3] = h->mp.gid_hi;
  *device = h->device;
  return S2D_OK;
}
