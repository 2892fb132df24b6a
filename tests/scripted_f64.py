"""The scripted team of the 11v11 match (include/s2d_match.h, "Per-slot controllers", rules 1-8) in plain float64, the rule by which
an fp32 result (the host restatement tests/scripted_policy_ref.c or the device) is held against it, and the corpus of states both
are tried on.  TEST INFRASTRUCTURE (tests/test_scripted_f64_host.py, tests/test_match_scripted_scenes_host.py,
tests/test_gpu_match_scripted_*.py), in the style of tests/obs_f64.py.

The reference is written from the header's prose, not from the kernel or its restatement: whole-array NumPy in float64, libm arctan2,
no fp32 intermediate.  Parameters are data, each rounded to fp32 once as the engine holds them (scripted_policy.params: the per-slot
kickable bound and catch length, the pitch, the penalty area, the catch cone, max_power); the S2D_SCRIPT_* constants are the
header's.  The kick-off formation is data too (FORM_X / FORM_Y; the host test holds it to the oracle's kick-off).

Every body is kept in (-180, 180] and every position on the pitch or beside it, so |atan2_deg - body| < 360: for such an argument
the restatement's norm_deg and the kernel's norm_deg_any are the SAME function (both take fmod only outside +-360, then fold once by
360); the controller can feed them nothing else.

The rule (the unit is one row: match, slot):
  * float64 runs from the state as given, from K_PROBES copies whose float words (x, y, body of players and ball) are moved by
    1..PROBE_ULPS fp32 ulps in a random direction (fixed seed), and from two copies moved by 3 ulps towards and away from zero;
  * a row is ILL-CONDITIONED if any run changes its command, its rule number or its team's chaser;
  * a well-conditioned row must reproduce the float64 command exactly, and its constant arguments (max_power, S2D_SCRIPT_DASH_POWER,
    the zeros) exactly;
  * its angle argument must satisfy |f32 - f64| <= T + 2 * spread (spread = the largest deviation of the probe runs), T in fp32 ulps
    at 180 degrees by the kind of angle; -180 equals +180 and +0 equals -0;
  * the share of ill-conditioned rows is reported; callers cap it (ILL_CAP for random and played states, EDGE_ILL_CAP for the
    constructed scenes).
"""
import numpy as np

import match_f64 as MF
import match_oracle as MO
import obs_f64 as OF
import scripted_policy as SP
from soccer2d_amd import _capi_match as M

K_PROBES, PROBE_ULPS = MF.K_PROBES, MF.PROBE_ULPS
ILL_CAP, EDGE_ILL_CAP = OF.ILL_CAP, OF.EDGE_ILL_CAP
UNIT = float(np.spacing(np.float32(180.0)))           # one fp32 ulp at 180 degrees
BALL_ANG, SHOT_ANG, HOME_ANG = 1, 2, 3                # kinds of angle argument (0: the row has none)
KIND_NAME = {BALL_ANG: 'ball', SHOT_ANG: 'shot', HOME_ANG: 'home'}
# T by kind, in UNITs.  Measured on the CPU by tests/test_scripted_f64_host.py over its whole corpus (the fp32 restatement against
# this reference: max over well-conditioned rows of (|f32 - f64| - 2 spread) / UNIT; the six strata at 3000 matches, the GPU batch and
# its swap_x, default and heterogeneous types); each T is at most 4x the measured maximum, and the host test re-measures both bounds.
# The largest values are swap_x's: a bearing near 0 becomes one near 180, whose fp32 rounding the unswapped state's probes do not show.
T_ULPS = {'ball': 2.0,                                # measured 0.854 (rules 3, 5, and 6 / 7 arrived; the strata alone 0.318)
          'shot': 1.2,                                # measured 0.306 (rules 2, 4; states reached by play 0.569)
          'home': 2.3}                                # measured 1.169 (rules 6, 7 on the way; the strata alone 0.411)

# the header's constants (S2D_SCRIPT_*), as the numbers it states
TURN_TOL, ARRIVE, DASH_POWER = 10.0, 1.0, 100.0
GOALIE_X, GOALIE_Y_GAIN, GOALIE_Y_MAX = 50.0, 0.25, 5.0
HOME_GAIN_X, HOME_GAIN_Y = 0.5, 0.25
# the kick-off formation (left team; the right team mirrors x)
FORM_X = np.array([-50.0, -35.0, -35.0, -35.0, -35.0, -20.0, -20.0, -20.0, -20.0, -10.5, -10.5])
FORM_Y = np.array([0.0, -20.0, -7.0, 7.0, 20.0, -22.0, -8.0, 8.0, 22.0, -6.0, 6.0])

LEFT, RIGHT = 1, 2
HALTED = (M.GM_TIME_OVER, M.GM_PAUSE, M.GM_HUMAN)
ANNOUNCEMENTS = (M.GM_OFF_SIDE, M.GM_BACK_PASS, M.GM_FREE_KICK_FAULT, M.GM_CATCH_FAULT, M.GM_FOUL_CHARGE, M.GM_ILLEGAL_DEFENSE,
                 M.GM_FOUL_PUSH, M.GM_FOUL_MULTIPLE_ATTACKER, M.GM_FOUL_BALL_OUT)
SHOOT_OUT = (M.GM_PENALTY_SETUP, M.GM_PENALTY_READY, M.GM_PENALTY_TAKEN, M.GM_PENALTY_MISS, M.GM_PENALTY_SCORE,
             M.GM_PENALTY_ONFIELD, M.GM_PENALTY_FOUL)
SHOOT_OUT_LIVE = (M.GM_PENALTY_READY, M.GM_PENALTY_TAKEN)
DEAD = ANNOUNCEMENTS + (M.GM_AFTER_GOAL, M.GM_BEFORE_KICK_OFF, M.GM_FIRST_HALF_OVER, M.GM_EXTEND_HALF, M.GM_GOALIE_CATCH) + \
    tuple(m for m in SHOOT_OUT if m not in SHOOT_OUT_LIVE)
RESTARTS = (M.GM_KICK_OFF, M.GM_KICK_IN, M.GM_FREE_KICK, M.GM_CORNER_KICK, M.GM_GOAL_KICK, M.GM_PENALTY_KICK, M.GM_IND_FREE_KICK)
SLOT = np.arange(22)
SIDE = np.where(SLOT < 11, LEFT, RIGHT)
GOALIE = (SLOT == 0) | (SLOT == 11)
KEYS = SP.OBJ_PLANES + SP.ENV_WORDS

# one heterogeneous configuration: kickable area, size and catch stretch differ by type; both goalies typed (their stretches differ)
HETERO_TYPES = {t: dict(kickable_margin=0.6 + 0.02 * t, player_size=0.3 + 0.005 * (t % 4), catchable_area_l_stretch=1.0 + 0.02 * t)
                for t in range(1, 18)}
HETERO_IDS = [16] + list(range(1, 11)) + [9] + [17 - i for i in range(10)]


def hetero_config(**kw):
    return MO.make_match_config(**dict(dict(player_types=HETERO_TYPES, player_type_id=HETERO_IDS), **kw))


def _norm(d):
    d = np.where(d <= -180.0, d + 360.0, d)
    return np.where(d > 180.0, d - 360.0, d)


def _bearing(dy, dx, body):
    """norm(atan2_deg(dy, dx) - body); atan2_deg of the zero vector is 0"""
    a = np.where((dx == 0.0) & (dy == 0.0), 0.0, np.degrees(np.arctan2(dy, dx)))
    return _norm(a - body)


def decide(state, prm):
    """the rule table on n matches -> dict of [n, 22] arrays: cmd, a, b (float64), rule (1..8: the rule that fired), search (the
    team search of the row's team: a slot, or -1 when it has no field player left), chaser (his team's chaser where the rules name
    one: the search in PlayOn and the team's own restarts, the taker in the shoot-out, else -1), ang (the angle argument, 0 where none) and kind
    (0 / BALL_ANG / SHOT_ANG / HOME_ANG)"""
    ka2, cl, fp = (np.asarray(v, dtype=np.float64) for v in prm)
    half_l, half_w, max_power, pen_x, pen_half_w, max_catch, min_catch = fp
    x, y, body = (np.asarray(state[k], dtype=np.float64) for k in ('x', 'y', 'body'))
    bx, by = x[:, 22:23], y[:, 22:23]
    x, y, body = x[:, :22], y[:, :22], body[:, :22]
    tackle, ban, card = (np.asarray(state[k])[:, :22] for k in ('tackle_cycles', 'catch_ban', 'card'))
    mode, mside, touch, holder, word = (np.asarray(state[k]).astype(np.int64)[:, None] for k in SP.ENV_WORDS)
    n = x.shape[0]
    d2 = (bx - x) ** 2 + (by - y) ** 2
    # the team search: nearest non-goalie on the pitch, ties to the lower index
    key = np.where(~GOALIE[None, :] & (card < M.CARD_RED), d2, np.inf)
    chaser = np.empty((n, 22), dtype=np.int64)
    for lo in (0, 11):
        k = key[:, lo:lo + 11]
        chaser[:, lo:lo + 11] = np.where(np.isfinite(k.min(axis=1)), lo + k.argmin(axis=1), -1)[:, None]
    shoot_out = np.isin(mode, SHOOT_OUT_LIVE)
    rule1 = np.isin(mode, HALTED + DEAD) | (tackle > 0) | (card >= M.CARD_RED)
    taker = shoot_out & (SLOT[None, :] == (word & 0xff) - 1)
    keeper = (mode == M.GM_PENALTY_TAKEN) & (SLOT[None, :] == np.where(mside == LEFT, 11, 0))
    rule8 = shoot_out & ~taker & ~keeper
    # the goal he attacks and the one he defends: by side, in the shoot-out the right one for both
    att = np.where(shoot_out, 1.0, np.where(SIDE == LEFT, 1.0, -1.0)[None, :])
    dfn = np.where(shoot_out, 1.0, -att)
    to_ball = _bearing(by - y, bx - x, body)
    shot = _bearing(0.0 - y, att * half_l - x, body)
    rule2 = (mode == M.GM_FREE_KICK) & (holder == SLOT[None, :] + 1)
    other = np.where(SIDE == LEFT, RIGHT, LEFT)[None, :]
    rule3 = GOALIE[None, :] & ((mode == M.GM_PLAY_ON) | keeper) & (ban == 0) & (touch == other) & (d2 <= (cl * cl)[None, :]) & \
        (to_ball <= max_catch) & (to_ball >= min_catch) & (np.abs(by) <= pen_half_w) & (dfn * bx >= pen_x)
    may_play = np.where(shoot_out, taker, (mode == M.GM_PLAY_ON) | (mside == SIDE[None, :]))
    rule4 = may_play & (d2 <= ka2[None, :])
    rule5 = may_play & (taker | (chaser == SLOT[None, :]))
    # "his team's chaser" exists where rule 5 names one: in PlayOn and the team's own restarts the team search, in the shoot-out
    # the taker for his team (rule 8); elsewhere nobody chases and the search decides nothing (-1)
    plays = np.where(shoot_out, (SIDE[None, :] == np.where((word & 0xff) <= 11, LEFT, RIGHT)) & ((word & 0xff) >= 1) & ((word & 0xff) <= 22),
                     ~np.isin(mode, HALTED + DEAD) & ((mode == M.GM_PLAY_ON) | (mside == SIDE[None, :])))
    named = np.where(plays, np.where(shoot_out, (word & 0xff) - 1, chaser), -1)
    k11 = SLOT % 11
    tx = np.where(GOALIE[None, :], dfn * GOALIE_X, np.clip(att * FORM_X[k11][None, :] + HOME_GAIN_X * bx, -half_l, half_l))
    ty = np.where(GOALIE[None, :], np.clip(by * GOALIE_Y_GAIN, -GOALIE_Y_MAX, GOALIE_Y_MAX),
                  np.clip(FORM_Y[k11][None, :] + HOME_GAIN_Y * by, -half_w, half_w))
    arrived = (tx - x) ** 2 + (ty - y) ** 2 <= ARRIVE * ARRIVE
    to_home = _bearing(ty - y, tx - x, body)
    rule = np.select([rule1, rule8, rule2, rule3, rule4, rule5], [1, 8, 2, 3, 4, 5], np.where(GOALIE[None, :], 6, 7))
    rule = np.broadcast_to(rule, (n, 22))
    kick, catch, chase, place = (rule == 2) | (rule == 4), rule == 3, rule == 5, rule >= 6
    place = place & (rule <= 7)
    target = np.where(chase | (place & arrived), to_ball, to_home)          # what a chaser or a placed player turns to
    turn = (chase | place) & (np.abs(target) > TURN_TOL)
    dash = (chase | (place & ~arrived)) & ~turn
    cmd = np.select([kick, catch, turn, dash], [M.MCMD_KICK, M.MCMD_CATCH, M.MCMD_TURN, M.MCMD_DASH], M.MCMD_NONE)
    ang = np.select([kick, catch, turn], [shot, to_ball, target], 0.0)
    kind = np.select([kick, catch | (turn & (chase | arrived)), turn], [SHOT_ANG, BALL_ANG, HOME_ANG], 0)
    a = np.select([kick, catch | turn, dash], [np.broadcast_to(max_power, ang.shape), ang, DASH_POWER], 0.0)
    b = np.where(kick, ang, 0.0)
    return dict(cmd=cmd, a=a, b=b, rule=rule.copy(), chaser=named, search=chaser, ang=ang, kind=kind)


def _circ(a, b):
    d = np.abs(a - b)
    return np.minimum(d, np.abs(360.0 - d))


def angle_of(actions):
    """the angle word of fp32 actions [n, 22, 3] by command: Kick's direction, Turn's moment, Catch's direction"""
    act = np.asarray(actions, dtype=np.float64)
    return np.where(act[..., 0] == M.MCMD_KICK, act[..., 2], act[..., 1])


def compare(state, prm, got, T=T_ULPS, seed=0x5C1, probes=K_PROBES):
    """(report, failures) of fp32 actions `got` [n, 22, 3] against float64 by the rule above.  report: n, ill, share, well [n, 22],
    f64 (decide's dict), spread [n, 22], worst {kind name: max over well-conditioned rows of (|f32 - f64| - 2 spread) / UNIT}"""
    base = decide(state, prm)
    ill = np.zeros(base['cmd'].shape, dtype=bool)
    spread = np.zeros(base['cmd'].shape)
    rs = np.random.RandomState(seed)
    for k in range(probes + 2):
        scale = 0 if k < probes else (-1 if k == probes else 1)
        p = decide(OF.perturb(state, rs, scale=scale), prm)
        ill |= (p['cmd'] != base['cmd']) | (p['rule'] != base['rule']) | (p['chaser'] != base['chaser'])
        spread = np.maximum(spread, _circ(p['ang'], base['ang']))
    well = ~ill
    g = np.asarray(got, dtype=np.float64)
    assert g.shape == base['cmd'].shape + (3,), g.shape
    fails = []

    def report(bad, what, f32, f64):
        idx = np.argwhere(bad & well)
        if len(idx):
            e, l = idx[0]
            fails.append(f'{what}: {len(idx)} well-conditioned rows differ; match {e} slot {l} (rule {base["rule"][e, l]}): '
                         f'f32={f32[e, l]!r} f64={f64[e, l]!r}')
    report(g[..., 0] != base['cmd'], 'command', g[..., 0], base['cmd'])
    same = g[..., 0] == base['cmd']
    is_ang_a, is_ang_b = np.isin(base['cmd'], (M.MCMD_TURN, M.MCMD_CATCH)), base['cmd'] == M.MCMD_KICK
    report(same & ~is_ang_a & (g[..., 1] != base['a']), 'constant argument a', g[..., 1], base['a'])
    report(same & ~is_ang_b & (g[..., 2] != base['b']), 'constant argument b', g[..., 2], base['b'])
    err = _circ(angle_of(g), base['ang'])
    worst = {}
    for kind, name in KIND_NAME.items():
        sel = well & same & (base['kind'] == kind)
        excess = np.where(sel, (err - 2.0 * spread) / UNIT, -np.inf)
        worst[name] = float(excess.max()) if excess.size else -np.inf
        if T is not None and worst[name] > T[name]:
            e, l = np.unravel_index(np.argmax(excess), excess.shape)
            fails.append(f'{name} angle: |f32 - f64| - 2 spread = {worst[name]:.2f} ulps > {T[name]} at match {e} slot {l} '
                         f'(rule {base["rule"][e, l]}): f32={float(angle_of(g)[e, l])!r} f64={float(base["ang"][e, l])!r} '
                         f'spread={float(spread[e, l])!r}')
    n_rows = int(well.size)
    return dict(n=n_rows, ill=int(ill.sum()), share=float(ill.sum()) / max(n_rows, 1), well=well, f64=base, spread=spread,
                worst=worst), fails


# ------------------------------------------------------------------------------------------------ the corpus
GPU_N, GPU_SEED, GPU_SIZES = 521, 77, (1, 7, 9, 521)       # the batches the GPU tests run; the host test runs them first
STRATA = ('scattered', 'ball at a player', 'ball at a goalie', 'set play', 'shoot-out', 'near home')
GRID = 65536.0                                        # bodies on the 2^-16-degree grid, without 0 and +-180 (match_symmetry.snap_bodies)


def home_points(bx, by, prm, shoot_out=None):
    """float64 [n, 22] x, y: every slot's guard point (goalies) or home position for the ball at bx, by [n]"""
    half_l, half_w = float(prm[2][0]), float(prm[2][1])
    bx, by = np.asarray(bx, np.float64)[:, None], np.asarray(by, np.float64)[:, None]
    att = np.where(SIDE == LEFT, 1.0, -1.0)[None, :]
    k = SLOT % 11
    tx = np.where(GOALIE[None, :], -att * GOALIE_X, np.clip(att * FORM_X[k][None, :] + HOME_GAIN_X * bx, -half_l, half_l))
    ty = np.where(GOALIE[None, :], np.clip(by * GOALIE_Y_GAIN, -GOALIE_Y_MAX, GOALIE_Y_MAX),
                  np.clip(FORM_Y[k][None, :] + HOME_GAIN_Y * by, -half_w, half_w))
    return tx, ty


def corpus(cfg, n, seed, strata=None):
    """(state, stratum [n]): n matches, every word of MATCH_BUFFER_FIELDS in the device dtypes (the words the controller does not read
    are those of a kick-off), match e drawn from stratum strata[e % len(strata)] of STRATA (default: all six in turn):
      0 scattered players and ball, PlayOn or any mode;
      1 the ball within 0..2 kickable radii of a random player, PlayOn or a restart;
      2 the ball within 0..2 catch lengths of a goalie inside or near his area, random last touch and catch ban;
      3 a random set-play mode and side, the ball at somebody's feet half of the time, a held ball in FreeKick_;
      4 PenaltyReady_ / PenaltyTaken_ with a random taker word;
      5 everybody within 0..2 m of his home or guard point.
    Random cards and tackle counters are sprinkled over all of them."""
    rs = np.random.RandomState(seed)
    prm = SP.params(cfg)
    ka, cl = np.sqrt(prm[0].astype(np.float64)), prm[1].astype(np.float64)
    f = np.float32
    s = MO.MatchOracle(cfg, n).snapshot()
    strata = tuple(range(len(STRATA))) if strata is None else tuple(strata)
    st = np.array([strata[e % len(strata)] for e in range(n)])
    x, y = rs.uniform(-52.0, 52.0, (n, 23)), rs.uniform(-33.5, 33.5, (n, 23))
    for g, sgn in ((0, -1.0), (11, 1.0)):                                    # the goalies in or near their areas
        x[:, g], y[:, g] = sgn * rs.uniform(34.0, 52.4, n), rs.uniform(-22.0, 22.0, n)
    body = rs.randint(1, 180 * 65536, (n, 22)) * rs.choice([-1, 1], (n, 22)) / GRID
    mode = np.where(rs.random_sample(n) < 0.7, M.GM_PLAY_ON, rs.randint(0, 32, n))
    mside = rs.randint(1, 3, n)
    touch = rs.randint(0, 3, n)
    holder = np.zeros(n, np.int64)
    word = np.zeros(n, np.int64)
    ban = np.zeros((n, 24), np.int32)
    ban[:, [0, 11]] = np.where(rs.random_sample((n, 2)) < 0.1, rs.randint(1, 6, (n, 2)), 0)
    e = np.arange(n)
    ang, u = rs.uniform(-np.pi, np.pi, n), rs.uniform(0.0, 2.0, n)
    # 1: the ball at a random player's feet
    who = rs.randint(0, 22, n)
    m = st == 1
    restart = rs.random_sample(n) < 0.4
    mode = np.where(m, np.where(restart, np.array(RESTARTS)[rs.randint(0, len(RESTARTS), n)], M.GM_PLAY_ON), mode)
    # 3: a set play
    m3 = st == 3
    mode = np.where(m3, np.where(rs.random_sample(n) < 0.4, M.GM_FREE_KICK, np.array(RESTARTS)[rs.randint(0, len(RESTARTS), n)]), mode)
    at_feet = m | (m3 & (rs.random_sample(n) < 0.5))
    held = m3 & (mode == M.GM_FREE_KICK) & (rs.random_sample(n) < 0.5)
    gk = np.where(rs.randint(0, 2, n) == 0, 0, 11)
    who = np.where(held, gk, who)
    holder = np.where(held, np.where(rs.random_sample(n) < 0.8, gk + 1, rs.randint(0, 23, n)), holder)
    at_feet |= held
    x[:, 22] = np.where(at_feet, x[e, who] + u * ka[who] * np.cos(ang), x[:, 22])
    y[:, 22] = np.where(at_feet, y[e, who] + u * ka[who] * np.sin(ang), y[:, 22])
    # 2: the ball in front of a goalie
    m2 = st == 2
    taken = m2 & (rs.random_sample(n) < 0.2)
    g2 = np.where(taken, np.where(mside == LEFT, 11, 0), gk)
    mode = np.where(m2, np.where(taken, M.GM_PENALTY_TAKEN, M.GM_PLAY_ON), mode)
    x[:, 0] = np.where(taken & (g2 == 0), -x[:, 0], x[:, 0])                 # the shoot-out is played at the right goal
    rel = rs.uniform(-120.0, 120.0, n)
    direction = np.radians(body[e, g2] + rel)
    x[:, 22] = np.where(m2, x[e, g2] + u * cl[g2] * np.cos(direction), x[:, 22])
    y[:, 22] = np.where(m2, y[e, g2] + u * cl[g2] * np.sin(direction), y[:, 22])
    touch = np.where(m2 & (rs.random_sample(n) < 0.6), np.where(g2 == 0, RIGHT, LEFT), touch)
    ban[e, g2] = np.where(m2, np.where(rs.random_sample(n) < 0.2, rs.randint(1, 6, n), 0), ban[e, g2])
    # 4: the shoot-out
    m4 = st == 4
    tk = np.where(rs.random_sample(n) < 0.1, 0, rs.randint(1, 23, n))
    mode = np.where(m4, np.where(rs.random_sample(n) < 0.5, M.GM_PENALTY_READY, M.GM_PENALTY_TAKEN), mode)
    word = np.where(m4 | taken, tk | (rs.randint(0, 1 << 16, n) << 12), word)
    mside = np.where((m4 | taken) & (tk > 0) & (rs.random_sample(n) < 0.9), np.where(tk <= 11, LEFT, RIGHT), mside)
    spot = m4 & (rs.random_sample(n) < 0.8)
    x[:, 22] = np.where(spot, 42.5 + rs.uniform(-3.0, 3.0, n), x[:, 22])
    y[:, 22] = np.where(spot, rs.uniform(-3.0, 3.0, n), y[:, 22])
    t = np.maximum(tk - 1, 0)
    close = m4 & (tk > 0) & (rs.random_sample(n) < 0.6)
    a4, u4 = rs.uniform(-np.pi, np.pi, n), rs.uniform(0.0, 2.0, n)
    x[e, t] = np.where(close, x[:, 22] + u4 * ka[t] * np.cos(a4), x[e, t])
    y[e, t] = np.where(close, y[:, 22] + u4 * ka[t] * np.sin(a4), y[e, t])
    kp = np.where(mside == LEFT, 11, 0)
    x[e, kp] = np.where(m4, rs.uniform(46.0, 52.4, n), x[e, kp])
    y[e, kp] = np.where(m4, rs.uniform(-6.0, 6.0, n), y[e, kp])
    # 5: everybody near his place
    m5 = st == 5
    mode = np.where(m5, np.where(rs.random_sample(n) < 0.6, M.GM_PLAY_ON, np.array(RESTARTS)[rs.randint(0, len(RESTARTS), n)]), mode)
    hx, hy = home_points(f(x[:, 22]), f(y[:, 22]), prm)
    r5, a5 = rs.uniform(0.0, 2.0, (n, 22)), rs.uniform(-np.pi, np.pi, (n, 22))
    x[:, :22] = np.where(m5[:, None], hx + r5 * np.cos(a5), x[:, :22])
    y[:, :22] = np.where(m5[:, None], hy + r5 * np.sin(a5), y[:, :22])
    facing = m5[:, None] & (rs.random_sample((n, 22)) < 0.5)                 # half of them look at the ball, more or less
    to_ball = np.degrees(np.arctan2(y[:, 22:23] - y[:, :22], x[:, 22:23] - x[:, :22])) + rs.uniform(-20.0, 20.0, (n, 22))
    to_ball = np.clip(_norm(np.round(to_ball * GRID) / GRID), -179.9, 179.9)
    body = np.where(facing & (to_ball != 0.0), to_ball, body)
    s['x'][:, :23], s['y'][:, :23] = x.astype(f), y.astype(f)
    s['body'][:, :22] = body.astype(f)
    s['vx'][:], s['vy'][:] = 0, 0
    s['mode'][:], s['mode_side'][:], s['last_touch_side'][:] = mode, mside, touch
    s['ball_holder'][:], s['set_play_taker'][:] = holder, word
    s['catch_ban'][:] = ban
    card = rs.random_sample((n, 22))
    s['card'][:, :22] = np.where(card < 0.03, M.CARD_RED, np.where(card < 0.08, M.CARD_YELLOW, M.CARD_NONE))
    s['tackle_cycles'][:, :22] = np.where(rs.random_sample((n, 22)) < 0.03, rs.randint(1, 11, (n, 22)), 0)
    return s, st


# ------------------------------------------------------------------------------------------------ reflections
FLIP_PERM = np.array([0, 4, 3, 2, 1, 8, 7, 6, 5, 10, 9])       # the formation under y -> -y: (1 4)(2 3)(5 8)(6 7)(9 10)
FLIP_SLOTS = np.r_[FLIP_PERM, 11 + FLIP_PERM, 22, 23]
SWAP_EXEMPT_MODES = SHOOT_OUT                                   # SWAP_X: the shoot-out always uses the right goal


def flip_y_state(s):
    """FLIP_Y of a state with the slot permutation under which the formation is symmetric; every plane moves with its slot"""
    import match_symmetry as SY
    out = SY.flip_y(s, 'state')
    for k in SY.SLOT_PLANES:
        out[k] = out[k][:, FLIP_SLOTS]
    for k in ('ball_holder', 'set_play_taker', 'last_kicker'):
        w = np.asarray(out[k]).astype(np.int64)
        idx = w & 0xff
        ok = (idx >= 1) & (idx <= 22)
        out[k] = ((w & ~0xff) | np.where(ok, FLIP_SLOTS[np.where(ok, idx - 1, 0)] + 1, idx)).astype(np.asarray(s[k]).dtype)
    return out


def flip_y_actions(a):
    import match_symmetry as SY
    return SY.flip_y_actions(np.asarray(a))[..., FLIP_SLOTS[:22], :]


def flip_y_dropped(state, prm, actions):
    """bool [n]: the matches FLIP_Y may not be held on bit for bit: an exact tie for chaser (the lower index wins, and the permutation
    changes who that is), or an angle argument of exactly +-180 (its sign is the rounding's)"""
    x, y = (np.asarray(state[k], np.float32) for k in ('x', 'y'))
    dx, dy = (x[:, 22:23] - x[:, :22]).astype(np.float64), y[:, 22:23] - y[:, :22]
    d2 = (dx * dx + (dy * dy).astype(np.float64)).astype(np.float32)      # the tie is the engine's: fmaf(dx, dx, dy * dy) in fp32
    key = np.where(~GOALIE[None, :] & (np.asarray(state['card'])[:, :22] < M.CARD_RED), d2, np.inf)
    tie = np.zeros(len(x), bool)
    for lo in (0, 11):
        k = np.sort(key[:, lo:lo + 11], axis=1)
        tie |= np.isfinite(k[:, 0]) & (k[:, 0] == k[:, 1])
    act = np.asarray(actions)
    has = np.isin(act[..., 0], (M.MCMD_TURN, M.MCMD_CATCH, M.MCMD_KICK))
    return tie | (has & (np.abs(angle_of(act)) == 180.0)).any(axis=1)
