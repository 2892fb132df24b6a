"""One cycle of the reach-ball engine from a shared state: an fp32 result (the fp32 oracle or the device) against the fp64 libm build
of the oracle, with a conditioning probe.  TEST INFRASTRUCTURE (tests/test_reach_oracle_f64.py, tests/test_gpu_reach_f64.py).

The rule (per env, after one cycle from the same 19 state words and the same action):
  * the fp64 build runs from the state as given, from K_PROBES copies whose 15 float words (and, where the action has float words,
    those too) are moved by 1..PROBE_ULPS fp32 ulps in a random direction (fixed seed), and from two copies moved PROBE_ULPS ulps
    towards and away from zero;
  * an env is ILL-CONDITIONED if any of these runs changes done, result, action_cmd, step_number, cycle, policy_step or episode
    (with auto-reset a changed `episode` is a changed reset), or the grid point the dash direction snaps to (dash_angle_step: the
    one discrete choice of the cycle that no output word holds; it is recomputed here from action_dir in float64);
  * a well-conditioned env must reproduce every fp64 discrete word, and every float word must satisfy
    |f32 - f64| <= (T_field + REF_ULPS) * unit_field + 2 * spread, spread = the largest deviation of the probe runs from the unperturbed one;
    angle words are compared on the circle;
  * an env that ends with auto-reset on is compared in reward, done, result and terminal_obs; its state and obs are a reset's, a
    function of (env id, episode) alone, and follow the reset rule (compare_reset);
  * a frozen env (S2D_CMD_FREEZE) must keep its 19 state words; its outputs are not part of the cycle;
  * the fraction of ill-conditioned envs is returned so that callers can cap it.
"""
import ctypes as C

import numpy as np

import oracle as O

F = O.STATE_FIELDS
NF = 15                                   # float words of a state row; the other four are counters
IDX = {f: i for i, f in enumerate(F)}
DISCRETE = ('done', 'result', 'action_cmd', 'step_number', 'cycle', 'policy_step', 'episode')
ANGLE_STATE = ('player_body', 'prev_angle')
K_PROBES, PROBE_ULPS = 4, 3
ILL_CAP = 0.01                            # the largest ill-conditioned share of one case
TRIES_CAP = 0.001                         # resets whose number of ball-velocity candidates may differ between the builds
GOAL, OUT, TIMEOUT = 1, 2, 3
CMD_FREEZE, CMD_NONE, CMD_DASH, CMD_TURN = -1, 0, 1, 2
f32 = np.float32


def ulp(m):
    return float(np.spacing(f32(abs(m))))


def units(cfg):
    """one fp32 ulp at each word's natural magnitude"""
    sp = cfg.sp
    cap = abs(sp.stamina_capacity) if sp.stamina_capacity != 0 else 1.0
    u = dict(player_x=52.5, player_y=34.0, player_vx=sp.player_speed_max, player_vy=sp.player_speed_max, player_body=180.0,
             stamina=sp.stamina_max, effort=1.0, recovery=1.0, stamina_capacity=cap, ball_x=52.5, ball_y=34.0,
             ball_vx=sp.ball_speed_max, ball_vy=sp.ball_speed_max, prev_dist=128.0, prev_angle=180.0, reward=128.0,
             action_dir=180.0, obs=1.0, terminal_obs=1.0)
    return {k: ulp(v) for k, v in u.items()}


# T_field in those units, one cycle from a shared state.  MEASURED_ULPS: the host corpus of tests/test_reach_oracle_f64.py (fp32 oracle
# against the fp64 build; the maximum over well-conditioned envs and all cases of (|f32 - f64| - 2 spread) / unit, rounded up in the
# third decimal).  Each T is at most 4x that maximum, and 0 where it is not above 0 (the fp32 error lies inside the probes' spread).
# No T is above 8 ulps.  The positions' own rounding (half an ulp at 52.5) is inside the spread of a 1-3 ulp probe, so their T is
# nearly 0; velocities, angles and observations carry the sincos / atan2 polynomials and the x * fl(1/c) products.
MEASURED_ULPS = dict(player_x=0.018, player_y=0.013, player_vx=1.187, player_vy=1.347, player_body=1.081, stamina=0.034, effort=0.2,
                     recovery=0.03, stamina_capacity=0.0, ball_x=0.06, ball_y=0.052, ball_vx=1.569, ball_vy=1.755, prev_dist=0.247,
                     prev_angle=1.569, obs=1.52, reward=0.145, action_dir=1.143, terminal_obs=1.52)
T_ULPS = dict(player_x=0.07, player_y=0.05,        # measured 0.018, 0.013 (a dash from a position near 0, where 3 ulps are small)
              player_vx=4.7, player_vy=5.3,        # measured 1.187, 1.347
              player_body=4.3,                     # measured 1.081 (turns)
              stamina=0.13, effort=0.8,            # measured 0.034, 0.2 (effort_dec, effort_inc are not fp32 numbers)
              recovery=0.12, stamina_capacity=0.0, # measured 0.03, 0
              ball_x=0.24, ball_y=0.2,             # measured 0.06, 0.052
              ball_vx=6.2, ball_vy=7.0,            # measured 1.569, 1.755
              prev_dist=0.98, prev_angle=6.2,      # measured 0.247, 1.569
              obs=6.0, terminal_obs=6.0,           # measured 1.52, 1.52
              reward=0.58,                         # measured 0.145
              action_dir=4.5)                      # measured 1.143 (a * fl(360 / n) for a * 360 / n)
# the same for the words a reset leaves (no input to perturb, so no spread: the whole fp32 error of the sample, the sincos of the ball
# velocity and the command-less cycle); maxima over test_resets_match_f64 and the resets inside the one-cycle cases.  prev_angle
# (and obs[0]) get the propagated bound of compare_reset_words on top: measured below it, T = 0.
RESET_MEASURED_ULPS = dict(player_x=1.094, player_y=0.615, player_vx=0.0, player_vy=0.0, player_body=0.0, stamina=0.471, effort=0.0,
                           recovery=0.0, stamina_capacity=0.0, ball_x=1.566, ball_y=0.626, ball_vx=1.954, ball_vy=1.916,
                           prev_dist=0.733, prev_angle=0.0, obs=1.636)
RESET_T_ULPS = dict(player_x=4.3, player_y=2.4,    # measured 1.094, 0.615 (a collision in the command-less cycle moves the player)
                    player_vx=0.0, player_vy=0.0, player_body=0.0,   # measured 0: +-0 and whole degrees
                    stamina=1.8,                   # measured 0.471 (recovery * stamina_inc_max)
                    effort=0.0, recovery=0.0, stamina_capacity=0.0,  # measured 0
                    ball_x=6.2, ball_y=2.5,        # measured 1.566, 0.626
                    ball_vx=7.8, ball_vy=7.6,      # measured 1.954, 1.916 (speed * sincos, then the decay)
                    prev_dist=2.9, prev_angle=0.0, # measured 0.733, below its propagated bound
                    obs=6.5)                       # measured 1.636
REF_ULPS = 1e-6                           # the float64 reference's own rounding (libm's cos(90 deg) is 6e-17, not 0): about a
                                          # thousand float64 roundings at the word's natural magnitude, added to every T
ATAN2_ERR_DEG = 3e-5                      # the stated maximum error of the atan2_deg polynomial


def make_cfg(kw, env_id_offset=0):
    """S2DConfig from a keyword set of test_gpu_parity.CONFIGS (noise off unless named, as test_gpu_parity._oracle)"""
    kw = dict(kw)
    return O.make_config(seed=kw.pop('seed', 0x5EED), env_id_offset=env_id_offset, auto_reset=int(kw.pop('auto_reset', True)),
                         noise=int(kw.pop('noise', False)), server=kw.pop('server', None), **kw)


def random_server_kw(seed):
    """the random ServerParam / task draw of test_gpu_rollout2.test_ws2_random_server_parameters (same generator, same seed)"""
    rs = np.random.RandomState(700 + seed)
    server = dict(
        player_decay=float(rs.uniform(0.2, 0.7)), ball_decay=float(rs.uniform(0.85, 0.99)),
        player_speed_max=float(rs.uniform(0.3, 1.2)), player_accel_max=float(rs.uniform(0.2, 1.0)),
        ball_speed_max=float(rs.uniform(1.0, 3.0)), player_size=float(rs.uniform(0.2, 2.5)), ball_size=float(rs.uniform(0.05, 0.5)),
        dash_power_rate=float(rs.uniform(0.003, 0.012)), side_dash_rate=float(rs.uniform(0.2, 0.6)),
        back_dash_rate=float(rs.uniform(0.4, 0.8)), dash_angle_step=float(rs.choice([0.0, 1.0, 22.5, 45.0])),
        min_dash_power=float(rs.choice([0.0, -100.0])), max_dash_power=float(rs.choice([100.0, 60.0])),
        stamina_max=float(rs.uniform(2000, 8000)), stamina_inc_max=float(rs.uniform(10, 60)),
        stamina_capacity=float(rs.choice([-1.0, 5000.0, 130600.0])), extra_stamina=float(rs.uniform(0, 100)),
        effort_min=float(rs.uniform(0.3, 0.8)), recover_min=float(rs.uniform(0.3, 0.7)),
        collision_vel_rate=float(rs.uniform(-0.5, -0.05)), player_rand=float(rs.uniform(0, 0.2)), ball_rand=float(rs.uniform(0, 0.1)))
    mode = seed % 3
    return dict(server=server, max_steps=int(rs.randint(5, 40)), min_distance_to_ball=float(rs.uniform(0.5, 8.0)),
                change_ball_velocity=bool(rs.randint(2)), change_ball_position=bool(rs.randint(2)),
                ball_position_x=float(rs.uniform(-20, 20)), ball_position_y=float(rs.uniform(-10, 10)),
                ball_speed=float(rs.uniform(0, 2.5)), ball_direction=float(rs.uniform(-180, 180)),
                use_continuous_action=mode != 0, use_turning=mode == 2, action_space_size=int(rs.choice([3, 8, 16, 36])),
                noise=bool(seed & 1), seed=int(rs.randint(1, 2 ** 31)))


def action_kind(cfg, actions, command=False):
    if command:
        return 'command'
    if not cfg.task.use_continuous_action:
        return 'discrete'
    return 'turning' if cfg.task.use_turning else 'continuous'


# ------------------------------------------------------------------------------------------------------------------ oracle plumbing
def read_rows(orc):
    """[n, 19] float64: the state words of an oracle engine (fp32 words as their values, counters as int32 values)"""
    return np.stack([orc.state(f).astype(np.float64) for f in F], axis=1)


def load_rows(orc, rows):
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    assert rows.shape == (orc.n, len(F))
    set_env, h = orc.L.s2do_set_env, orc.h
    for i in range(orc.n):
        a = orc._row(rows[i])
        assert set_env(h, i, a.ctypes.data_as(C.POINTER(C.c_double))) == 0


def last_tries(orc):
    out = np.zeros(orc.n, dtype=np.int32)
    orc.L.s2do_last_tries.argtypes = [C.c_void_p, C.c_void_p]
    orc.L.s2do_last_tries(orc.h, out.ctypes.data)
    return out


def outputs(orc):
    """what one cycle leaves, as float64 / integer arrays"""
    return dict(state=read_rows(orc), obs=orc.obs().astype(np.float64), reward=orc.reward().astype(np.float64),
                done=orc.done().astype(np.int64), result=orc.result().astype(np.int64), action_cmd=orc.action_cmd().astype(np.int64),
                action_dir=orc.action_dir().astype(np.float64), terminal_obs=orc.terminal_obs().astype(np.float64),
                tries=last_tries(orc))


def step_from(cfg, rows, actions, prec, command=False):
    """one cycle of the `prec` build from `rows` (env ids cfg.env_id_offset + 0..n-1)"""
    orc = O.OracleEngine(cfg, len(rows), prec)
    load_rows(orc, rows)
    if command:
        orc.step_commands(actions)
    else:
        orc.step(actions)
    out = outputs(orc)
    orc.close()
    return out


def f32_step(cfg, rows, actions, command=False):
    return step_from(cfg, rows, actions, 'f32', command)


def _move(v, steps, ulps):
    v = v.astype(f32)
    for k in range(ulps):
        go = np.abs(steps) > k
        v = np.where(go, np.nextafter(v, np.where(steps > 0, f32(np.inf), f32(-np.inf))), v)
    return v


def perturb(a, rs, ulps=PROBE_ULPS, scale=0):
    """a copy of the float array `a` (fp32 values) with every word moved by 1..ulps fp32 ulps in a random direction; scale = -1 /
    +1: every word moved by `ulps` ulps towards / away from zero (match_f64.perturb)"""
    v = np.asarray(a).astype(f32)
    if scale:
        steps = np.where(np.signbit(v), -1, 1) * scale * ulps
    else:
        steps = rs.randint(1, ulps + 1, size=v.shape) * rs.choice([-1, 1], size=v.shape)
    return _move(v, steps, ulps)


def snapped_dash_dir(cfg, out):
    """the grid point Player::dash snaps the direction to (float64, a true division; NaN where the cycle did not dash or the angle
    is free)"""
    sp = cfg.sp
    d = np.clip(out['action_dir'], sp.min_dash_angle, sp.max_dash_angle)
    if sp.dash_angle_step > 0:
        step = float(f32(sp.dash_angle_step))
        d = step * np.rint(d / step)
        return np.where(out['action_cmd'] == CMD_DASH, d, np.nan)
    return np.full(len(d), np.nan)


def circ(d, period=360.0):
    d = np.abs(d) % period
    return np.minimum(d, period - d)


def _fdiff(name, a, b, col=None):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    if name in ANGLE_STATE or name == 'action_dir':
        return circ(d)
    if name in ('obs', 'terminal_obs'):
        d = d.copy()
        d[:, 0] = circ(d[:, 0], 2.0); d[:, 1] = circ(d[:, 1], 2.0); d[:, 7] = circ(d[:, 7], 1.0)
    return d


def _float_words(out):
    w = {f: out['state'][:, IDX[f]] for f in F[:NF]}
    w.update(obs=out['obs'], reward=out['reward'], action_dir=out['action_dir'], terminal_obs=out['terminal_obs'])
    return w


def _discrete_words(out):
    w = {k: out[k] for k in ('done', 'result', 'action_cmd')}
    w.update({f: out['state'][:, IDX[f]].astype(np.int64) for f in F[NF:]})
    return w


def probe(cfg, rows, actions, command=False, seed=0xF64, probes=K_PROBES):
    """(float64 outputs from `rows`, ill-conditioned mask, {word: envs it flagged first}, {float word: spread}) of the probe runs"""
    rows = np.asarray(rows, dtype=np.float64)
    n = len(rows)
    kind = action_kind(cfg, actions, command)
    base = step_from(cfg, rows, actions, 'f64', command)
    rs = np.random.RandomState(seed)
    bd, bf, bsnap = _discrete_words(base), _float_words(base), snapped_dash_dir(cfg, base)
    ill = np.zeros(n, bool)
    ill_words = {}
    spread = {k: np.zeros_like(v) for k, v in bf.items()}
    for k in range(probes + 2):
        scale = 0 if k < probes else (-1 if k == probes else 1)
        prow = rows.copy()
        prow[:, :NF] = perturb(rows[:, :NF], rs, scale=scale)
        pact = actions
        if kind in ('continuous', 'turning'):
            pact = perturb(np.asarray(actions, dtype=f32), rs, scale=scale)
        elif kind == 'command':
            pact = np.asarray(actions, dtype=f32).copy()
            pact[:, 1:3] = perturb(pact[:, 1:3], rs, scale=scale)
        p = step_from(cfg, prow, pact, 'f64', command)
        pd, pf, psnap = _discrete_words(p), _float_words(p), snapped_dash_dir(cfg, p)
        for w in DISCRETE:
            d = pd[w] != bd[w]
            ill_words[w] = ill_words.get(w, 0) + int((d & ~ill).sum())
            ill |= d
        d = ~((psnap == bsnap) | (np.isnan(psnap) & np.isnan(bsnap)))
        ill_words['dash_grid'] = ill_words.get('dash_grid', 0) + int((d & ~ill).sum())
        ill |= d
        for w in spread:
            spread[w] = np.maximum(spread[w], _fdiff(w, pf[w], bf[w]))
    return base, ill, ill_words, spread


def compare(cfg, rows, actions, f32_after, command=False, seed=0xF64, probes=K_PROBES, t_ulps=None, reset_t=None):
    """(report dict, list of failure strings).  rows [n, 19]; f32_after: the dict of outputs() from the fp32 oracle or the device."""
    rows = np.asarray(rows, dtype=np.float64)
    n = len(rows)
    t_ulps = T_ULPS if t_ulps is None else t_ulps
    base, ill, ill_words, spread = probe(cfg, rows, actions, command, seed, probes)
    bd, bf = _discrete_words(base), _float_words(base)
    frozen = np.zeros(n, bool)
    if command:
        c = np.asarray(actions, dtype=f32)[:, 0]
        frozen = (c >= -1.5) & (c <= -0.5)
    ill &= ~frozen
    well = ~ill & ~frozen
    ended = (base['done'] != 0) & bool(cfg.auto_reset)          # these envs hold a reset's state and obs
    fails = []
    gd, gf = _discrete_words(f32_after), _float_words(f32_after)
    for w in DISCRETE:
        bad = np.flatnonzero((gd[w] != bd[w]) & well)
        if len(bad):
            e = bad[0]
            fails.append(f'{w}: {len(bad)} well-conditioned envs differ; env {e}: f32={gd[w][e]!r} f64={bd[w][e]!r}')
    if frozen.any():
        same = (f32_after['state'][frozen].astype(f32).view(np.int32)[:, :NF] == rows[frozen].astype(f32).view(np.int32)[:, :NF]).all() \
            and (f32_after['state'][frozen][:, NF:] == rows[frozen][:, NF:]).all()
        if not same:
            fails.append('a frozen env changed its state')
    unit = units(cfg)
    worst = {}
    for w in spread:
        err = _fdiff(w, gf[w], bf[w])
        excess = (err - 2.0 * spread[w]) / unit[w] - REF_ULPS
        use = well.copy()
        if w == 'terminal_obs':
            use &= ended
        elif w not in ('reward', 'action_dir'):
            use &= ~ended
        excess = np.where(use[:, None] if excess.ndim == 2 else use, excess, -np.inf)
        worst[w] = float(excess.max()) if n else -np.inf
        if worst[w] > t_ulps[w]:
            i = np.unravel_index(np.argmax(excess), excess.shape)
            fails.append(f'{w}: |f32 - f64| - 2 spread = {worst[w]:.2f} ulps > {t_ulps[w]} at {i}: f32={gf[w][i]!r} f64={bf[w][i]!r} '
                         f'spread={spread[w][i]!r}')
    rep = dict(n=n, ill=int(ill.sum()), share=float(ill.sum()) / max(n, 1), ill_mask=ill, ill_words=ill_words, well=well, worst=worst,
               f64=base, ended=int((ended & well).sum()), reset=None)
    sel = ended & well
    if sel.any():
        rrep, rfails = compare_reset_words(cfg, {k: (v[sel] if isinstance(v, np.ndarray) and len(v) == n else v)
                                                 for k, v in f32_after.items()},
                                           {k: (v[sel] if isinstance(v, np.ndarray) and len(v) == n else v) for k, v in base.items()},
                                           reset_t)
        rep['reset'] = rrep
        fails += [f'auto-reset: {m}' for m in rfails]
    return rep, fails


# ------------------------------------------------------------------------------------------------------------------------ resets
RESET_WORDS = F[:NF] + ('obs',)


def compare_reset_words(cfg, g, b, reset_t=None):
    """the words a reset leaves, fp32 `g` against float64 `b` (dicts of outputs(), rows of the same (env id, episode)).  Envs whose
    resets drew another number of ball-velocity candidates are skipped and counted.  Every word: |f32 - f64| <= T * unit; the angle
    words prev_angle and obs[0] get, instead of a probe spread, the angle a vector of length d can turn by when its ends are each off
    by delta (the measured position error): asin(2 delta / d), plus the error of the atan2 polynomial."""
    reset_t = RESET_T_ULPS if reset_t is None else reset_t
    unit = units(cfg)
    n = len(g['done'])
    skip = g['tries'] != b['tries']
    use = ~skip
    fails, worst = [], {}
    for w in F[NF:]:
        d = g['state'][:, IDX[w]] != b['state'][:, IDX[w]]
        if (d & use).any():
            fails.append(f'{w}: {int((d & use).sum())} resets differ')
    gs, bs = g['state'], b['state']
    delta = np.maximum(np.hypot(gs[:, IDX['player_x']] - bs[:, IDX['player_x']], gs[:, IDX['player_y']] - bs[:, IDX['player_y']]),
                       np.hypot(gs[:, IDX['ball_x']] - bs[:, IDX['ball_x']], gs[:, IDX['ball_y']] - bs[:, IDX['ball_y']]))
    dist = bs[:, IDX['prev_dist']]
    with np.errstate(divide='ignore', invalid='ignore'):
        turn = np.degrees(np.arcsin(np.minimum(1.0, np.where(dist > 0, 2.0 * delta / dist, 1.0)))) + ATAN2_ERR_DEG
    turn = np.where(dist > 0, turn, 180.0)
    gf, bf = _float_words(g), _float_words(b)
    for w in RESET_WORDS:
        err = _fdiff(w, gf[w], bf[w])
        extra = np.zeros_like(err)
        if w == 'prev_angle':
            extra = turn
        elif w == 'obs':
            extra[:, 0] = turn / 180.0
        excess = (err - extra) / unit[w] - REF_ULPS
        excess = np.where(use[:, None] if excess.ndim == 2 else use, excess, -np.inf)
        worst[w] = float(excess.max()) if use.any() else -np.inf
        if worst[w] > reset_t[w]:
            i = np.unravel_index(np.argmax(excess), excess.shape)
            fails.append(f'{w}: |f32 - f64| = {worst[w]:.2f} ulps over its bound > {reset_t[w]} at {i}: f32={gf[w][i]!r} f64={bf[w][i]!r}')
    return dict(n=n, skipped=int(skip.sum()), worst=worst), fails


def reset_from(cfg, n, episode, prec, mask=None):
    """outputs() of the `prec` build after a reset that starts episode `episode` + 1 (the masked envs; the others stay as created)"""
    orc = O.OracleEngine(cfg, n, prec)
    rows = read_rows(orc)
    rows[:, IDX['episode']] = episode
    load_rows(orc, rows)
    orc.reset(mask)
    out = outputs(orc)
    orc.close()
    return out


def compare_reset(cfg, n, episode, f32_after, mask=None, reset_t=None):
    """a reset of envs cfg.env_id_offset + 0..n-1 from episode counters `episode` [n]: fp32 outputs against the float64 build"""
    b = reset_from(cfg, n, episode, 'f64', mask)
    sel = np.ones(n, bool) if mask is None else np.asarray(mask).astype(bool)
    pick = lambda d: {k: (v[sel] if isinstance(v, np.ndarray) and len(v) == n else v) for k, v in d.items()}
    return compare_reset_words(cfg, pick(f32_after), pick(b), reset_t)


# ------------------------------------------------------------------------------------------------------------------------ corpora
def random_actions(rs, cfg, n):
    t = cfg.task
    if not t.use_continuous_action:
        return rs.randint(0, t.action_space_size, n).astype(np.int64)
    return rs.uniform(-1.3, 1.3, (n, 4 if t.use_turning else 1)).astype(f32)


def played_states(cfg, n=512, steps=90, points=15, seed=42):
    """[(rows, actions)] at `points` cycles of a `steps`-cycle fp32 run with random caller actions (the first right after the reset)"""
    orc = O.OracleEngine(cfg, n, 'f32')
    orc.reset()
    rs = np.random.RandomState(seed)
    take = set(np.unique(np.linspace(0, steps - 1, points).astype(int)).tolist())
    out = []
    for t in range(steps):
        a = random_actions(rs, cfg, n)
        if t in take:
            out.append((read_rows(orc), a))
        orc.step(a)
    orc.close()
    return out


def written_states(cfg, n=512, seed=7):
    """rows no rollout reaches: positions over the pitch and 2 m beyond, velocities up to 1.5x the caps, any body angle, stamina around
    0, the three thresholds and stamina_max, effort and recovery over their ranges, capacity 0 / small / full, a ball inside the
    collision radius (10 %) and inside min_distance_to_ball (10 %), step_number around max_steps"""
    rs = np.random.RandomState(seed)
    sp, t = cfg.sp, cfg.task
    r = np.zeros((n, len(F)))
    col = lambda f, v: r.__setitem__((slice(None), IDX[f]), v)
    px, py = rs.uniform(-54.5, 54.5, n), rs.uniform(-36, 36, n)
    bx, by = rs.uniform(-54.5, 54.5, n), rs.uniform(-36, 36, n)
    u = rs.uniform(size=n)
    ang = rs.uniform(-np.pi, np.pi, n)
    near = np.where(u < 0.1, rs.uniform(0, sp.player_size + sp.ball_size, n), rs.uniform(0, max(t.min_distance_to_ball, 0.1), n))
    bx = np.where(u < 0.2, px + near * np.cos(ang), bx)
    by = np.where(u < 0.2, py + near * np.sin(ang), by)
    for f, v in (('player_x', px), ('player_y', py), ('ball_x', bx), ('ball_y', by)):
        col(f, v)
    for fx, fy, cap in (('player_vx', 'player_vy', sp.player_speed_max), ('ball_vx', 'ball_vy', sp.ball_speed_max)):
        m, a = rs.uniform(0, 1.5 * cap, n) * (rs.uniform(size=n) < 0.9), rs.uniform(-np.pi, np.pi, n)
        col(fx, m * np.cos(a)); col(fy, m * np.sin(a))
    col('player_body', np.where(rs.uniform(size=n) < 0.5, rs.randint(-180, 181, n), rs.uniform(-180, 180, n)))
    marks = np.array([0.0, sp.recover_dec_thr * sp.stamina_max, sp.effort_dec_thr * sp.stamina_max, sp.effort_inc_thr * sp.stamina_max,
                      sp.stamina_max])
    st = marks[rs.randint(0, 5, n)] + rs.uniform(-150, 150, n)
    st = np.where(rs.uniform(size=n) < 0.3, rs.uniform(0, sp.stamina_max, n), st)
    col('stamina', np.clip(st, 0, sp.stamina_max))
    col('effort', rs.uniform(sp.effort_min, sp.effort_init, n))
    col('recovery', rs.uniform(sp.recover_min, sp.recover_init, n))
    full = sp.stamina_capacity
    col('stamina_capacity', full if full < 0 else np.choose(rs.randint(0, 3, n), [np.zeros(n), rs.uniform(0, 100, n), np.full(n, full)]))
    rr = r.astype(f32).astype(np.float64)
    col('prev_dist', np.hypot(rr[:, IDX['ball_x']] - rr[:, IDX['player_x']], rr[:, IDX['ball_y']] - rr[:, IDX['player_y']])
        + rs.uniform(-1, 1, n) * (rs.uniform(size=n) < 0.5))
    col('prev_angle', rs.uniform(-180, 180, n))
    r[:, :NF] = r[:, :NF].astype(f32)
    sn = np.where(rs.uniform(size=n) < 0.25, rs.randint(t.max_steps - 3, t.max_steps + 3, n), rs.randint(0, max(t.max_steps, 1), n))
    col('step_number', np.maximum(sn, 0))
    col('cycle', rs.randint(1, 5000, n))
    col('policy_step', rs.randint(0, 5000, n))
    col('episode', rs.randint(1, 60, n))
    return r


def random_commands(n, seed=3):
    """[n, 4] S2D_ACT_COMMAND rows: Dash with powers in [-150, 150] (the back dash under min_dash_power = -100) and directions
    beyond +-180, Turn with moments beyond +-180, NONE and FREEZE"""
    rs = np.random.RandomState(seed)
    c = np.zeros((n, 4), dtype=f32)
    c[:, 0] = rs.choice([CMD_DASH, CMD_DASH, CMD_DASH, CMD_TURN, CMD_TURN, CMD_NONE, CMD_FREEZE], n)
    c[:, 1] = rs.uniform(-150, 150, n)
    c[:, 2] = rs.uniform(-270, 270, n)
    return c


COMMAND_KW = dict(use_continuous_action=False, change_ball_velocity=True, max_steps=40, server=dict(min_dash_power=-100.0))


WRITTEN = ('dqn-discrete16', 'continuous1', 'turning4', 'noise-on', 'no-autoreset-collide')


def case_names():
    from test_gpu_parity import CONFIGS
    return ([f'played {k}' for k in CONFIGS] + [f'played random-server-{s}' for s in range(6)] + [f'written {k}' for k in WRITTEN]
            + ['written random-server-1', 'written random-server-2', 'commands', 'fast-path', 'fast-path noise', 'scene states', 'scene states auto-reset'])


def capped(name):
    """the 1 % cap on ill-conditioned envs holds for every case but the constructed scenes' states, which sit on their thresholds"""
    return not name.startswith('scene states')


def build_case(name, points=15):
    """(config keywords, command?, [(rows, actions)]) of one case: a played configuration of test_gpu_parity.CONFIGS, a random
    ServerParam draw, written states under a configuration, or the S2D_ACT_COMMAND path on played and written states.  `points`
    time points of the played run; a quarter as many batches of written states."""
    from test_gpu_parity import CONFIGS
    kind, _, key = name.partition(' ')
    if name == 'commands':
        cfg = make_cfg(COMMAND_KW)
        played = played_states(cfg, points=max(points // 3, 2))
        return COMMAND_KW, True, ([(rows, random_commands(512, seed=20 + j)) for j, (rows, _) in enumerate(played)]
                                  + [(written_states(cfg, seed=200 + j), random_commands(512, seed=40 + j)) for j in range(2)])
    if name.startswith('scene states'):
        kw, _, rows, a = scene_state_case(name.endswith('auto-reset'))
        return kw, False, [(rows, a)]
    if name.startswith('fast-path'):
        kw, items = fast_path_case(noise=name.endswith('noise'))
        return kw, False, items
    kw = random_server_kw(int(key[-1])) if key.startswith('random-server-') else CONFIGS[key]
    cfg = make_cfg(kw)
    if kind == 'played':
        return kw, False, played_states(cfg, points=points)
    k = case_names().index(name)
    rs = np.random.RandomState(50 + k)
    return kw, False, [(written_states(cfg, seed=10 * k + j), random_actions(rs, cfg, 512)) for j in range(max(points // 4, 2))]


# ------------------------------------------------------------------------------------------------- constructed scenes, known answers
# Server and task values under which the scenes' arithmetic does not round: radii 0.5 + 0.5, powers of two for the rates and
# decays, thresholds 0.25 / 0.375 / 0.5 of stamina_max = 2000 / 3000 / 4000, no extra stamina, Dash(128) = acceleration 1.
_EXACT = dict(player_size=0.5, ball_size=0.5, extra_stamina=0.0, min_dash_power=-100.0, max_dash_power=128.0, dash_power_rate=2.0 ** -7,
              side_dash_rate=0.5, back_dash_rate=0.75, inertia_moment=4.0, recover_dec_thr=0.25, effort_dec_thr=0.375,
              effort_inc_thr=0.5, effort_min=0.5, recover_min=0.5, effort_dec=2.0 ** -7, effort_inc=2.0 ** -6, recover_dec=2.0 ** -9,
              player_decay=0.5, ball_decay=0.5, collision_vel_rate=-0.125)
_TASK = dict(use_continuous_action=False, auto_reset=False, max_steps=200, min_distance_to_ball=5.0, change_ball_velocity=True)
SCENE_CONFIGS = {
    'A': dict(_TASK, server=dict(_EXACT)),
    'unlimited': dict(_TASK, server=dict(_EXACT, stamina_capacity=-1.0)),
    'points': dict(_TASK, server=dict(_EXACT, player_size=0.0, ball_size=0.0)),          # no radius: the ball can stay on the player
    'step7.5': dict(_TASK, use_continuous_action=True, server=dict(_EXACT, dash_angle_step=7.5)),
    'step22.5': dict(_TASK, use_continuous_action=True, server=dict(_EXACT, dash_angle_step=22.5)),
    'step45': dict(_TASK, use_continuous_action=True, server=dict(_EXACT, dash_angle_step=45.0)),
}
_BASE_ROW = dict(player_x=0.0, player_y=0.0, player_vx=0.0, player_vy=0.0, player_body=0.0, stamina=8000.0, effort=1.0, recovery=1.0,
                 stamina_capacity=130600.0, ball_x=20.0, ball_y=0.0, ball_vx=0.0, ball_vy=0.0, prev_dist=20.0, prev_angle=0.0,
                 step_number=10, cycle=11, policy_step=5, episode=1)
FLOAT_TOL = 1e-9          # hand-written floats against float64 (libm's cos(90 deg) is 6e-17, not 0)


def up(x, k=1):
    """the fp32 value k ulps above x in magnitude (k < 0: below)"""
    v = f32(x)
    for _ in range(abs(k)):
        v = np.nextafter(v, f32(np.copysign(np.inf, v)) if k > 0 else f32(0.0))
    return float(v)


def scenes():
    """[dict(name, cfg, row, action, expect, ill)]: action = a command row (cmd, power, dir) or, in the continuous configurations,
    the action word; expect = {word: value}: done / result / reward / a state field / 'obs<k>' / '|obs0|'; '-0' / '+0' ask for
    the sign of a zero; 'grid' = the grid point the dash direction snaps to in float64 (fp32: that one or a neighbour)."""
    out = []
    NONE, DASH, TURN = (CMD_NONE, 0.0, 0.0), CMD_DASH, CMD_TURN

    def S(name, action=NONE, cfg='A', ill=False, expect=None, **row):
        e = dict(done=0, result=0)
        e.update(expect or {})
        out.append(dict(name=name, cfg=cfg, row=dict(_BASE_ROW, **row), action=action, expect=e, ill=ill))

    b5 = up(5.0, -1)
    # Goal: strict <
    S('goal: d = min_distance on x', ball_x=5.0, prev_dist=5.0, expect=dict(reward=0.0))
    S('goal: one ulp inside on x', ball_x=b5, prev_dist=5.0, expect=dict(done=1, result=GOAL, reward=10.0 + (5.0 - b5)))
    S('goal: d = min_distance on y', ball_x=0.0, ball_y=-5.0, player_body=-90.0, prev_dist=5.0, expect=dict(reward=0.0))
    S('goal: one ulp inside on y', ball_x=0.0, ball_y=-b5, player_body=-90.0, prev_dist=5.0,
      expect=dict(done=1, result=GOAL, reward=10.0 + (5.0 - b5)))
    S('goal: (3, 4) is 5', ball_x=3.0, ball_y=4.0, prev_dist=5.0)
    S('goal: (3, 4 - ulp) rounds to 5 in fp32', ball_x=3.0, ball_y=up(4.0, -1), prev_dist=5.0, ill=True, expect=dict(done=1, result=GOAL))
    # Out: strict >, the four lines; the ball 20 m inside, straight ahead
    for name, px, py, body in (('x+', 52.5, 0.0, 180.0), ('x-', -52.5, 0.0, 0.0), ('y+', 0.0, 34.0, -90.0), ('y-', 0.0, -34.0, 90.0)):
        bx, by = px - np.sign(px) * 20.0, py - np.sign(py) * 20.0
        S(f'out: on the line {name}', player_x=px, player_y=py, ball_x=bx, ball_y=by, player_body=body, expect=dict(reward=0.0))
        qx, qy = (up(px), py) if px else (px, up(py))
        S(f'out: one ulp beyond {name}', player_x=qx, player_y=qy, ball_x=bx, ball_y=by, player_body=body,
          expect=dict(done=1, result=OUT, reward=10.0 - (abs(qx - px) + abs(qy - py))))
    # Timeout: strict > after the increment
    S('timeout: step_number = max_steps after the increment', step_number=199, expect=dict(step_number=200, reward=0.0))
    S('timeout: one more', step_number=200, expect=dict(done=1, result=TIMEOUT, step_number=201, reward=-5.0))
    # label overwrite: Goal, then Out, then Timeout (the reward keeps every term)
    xo = up(52.5)
    S('labels: goal + out + timeout', player_x=xo, ball_x=50.0, player_body=180.0, prev_dist=2.5, step_number=200,
      expect=dict(done=1, result=TIMEOUT, reward=(2.5 - (xo - 50.0)) + 10.0 + 10.0 - 5.0))
    S('labels: goal + out', player_x=xo, ball_x=50.0, player_body=180.0, prev_dist=2.5,
      expect=dict(done=1, result=OUT, reward=(2.5 - (xo - 50.0)) + 20.0))
    S('labels: goal + timeout', ball_x=2.5, prev_dist=2.5, step_number=200, expect=dict(done=1, result=TIMEOUT, reward=5.0))
    S('labels: out + timeout', player_x=xo, ball_x=32.5, player_body=180.0, step_number=200,
      expect=dict(done=1, result=TIMEOUT, reward=(20.0 - (xo - 32.5)) + 10.0 - 5.0))
    # collision (radius sum 1, velocity rate -1/8): strict <; at d = 0 the axis is (1, 0); an object at rest is left with -0
    S('collision: centres coincide', player_x=1.0, player_y=1.0, ball_x=1.0, ball_y=1.0, prev_dist=0.0,
      expect=dict(done=1, result=GOAL, player_x=0.5, player_y=1.0, ball_x=1.5, ball_y=1.0, player_vx='-0', player_vy='-0', ball_vx='-0',
                  ball_vy='-0', reward=9.0))
    S('collision: d = radius sum', player_x=1.0, player_y=1.0, ball_x=2.0, ball_y=1.0, prev_dist=1.0,
      expect=dict(done=1, result=GOAL, player_x=1.0, ball_x=2.0, player_vx='+0', player_vy='+0', ball_vx='+0', ball_vy='+0', reward=10.0))
    bx = up(2.0, -1)
    S('collision: one ulp inside', player_x=1.0, player_y=1.0, ball_x=bx, ball_y=1.0, prev_dist=1.0,
      expect=dict(done=1, result=GOAL, player_x=(1.0 + bx) / 2 - 0.5, ball_x=(1.0 + bx) / 2 + 0.5, player_vx='-0', player_vy='-0',
                  ball_vx='-0', ball_vy='-0', reward=10.0))
    S('collision: a moving ball bounces', player_x=1.0, player_y=1.0, ball_x=1.5, ball_y=1.0, ball_vx=0.25, prev_dist=0.5,
      expect=dict(done=1, result=GOAL, player_x=0.875, ball_x=1.875, player_vx='-0', ball_vx=0.25 * -0.125 * 0.5, ball_vy='-0'))
    # speed clamps: |v| = cap is not clamped
    pc, bc = float(f32(1.05)), 3.0
    S('speed: player at the cap', player_vx=pc, expect=dict(player_x=pc, player_vx=pc * 0.5))
    S('speed: player one ulp above', player_vx=up(pc), expect=dict(player_x=1.05, player_vx=0.525))   # float64's cap is 1.05 itself
    S('speed: player at the cap, -y', player_vy=-pc, expect=dict(player_y=-pc, player_vy=-pc * 0.5))
    S('speed: ball at the cap', ball_vx=bc, expect=dict(ball_x=23.0, ball_vx=1.5, reward=-3.0))
    S('speed: ball one ulp above', ball_vx=up(bc), expect=dict(ball_x=23.0, ball_vx=1.5, reward=-3.0))
    # acceleration clamp: Dash(128) with effort 1 is |a| = 1 = player_accel_max
    S('accel: at the cap', (DASH, 128.0, 0.0), expect=dict(player_x=1.0, player_vx=0.5, stamina=7917.0, stamina_capacity=130555.0))
    S('accel: one ulp above', (DASH, 128.0, 0.0), effort=up(1.0), expect=dict(player_x=1.0, player_vx=0.5))
    # dash stamina (no extra stamina)
    S('stamina: need > stamina cuts the power', (DASH, 100.0, 0.0), stamina=30.0, effort=0.5, recovery=0.5,
      expect=dict(player_x=0.5 * 30.0 / 128.0, stamina=22.5, effort=0.5, recovery=0.5, stamina_capacity=130577.5))
    S('stamina: exactly 0 afterwards', (DASH, 100.0, 0.0), stamina=100.0, effort=0.5, recovery=0.5, stamina_capacity=0.0,
      expect=dict(player_x=0.5 * 100.0 / 128.0, stamina=0.0, stamina_capacity=0.0))
    S('stamina: stamina_max before recovery', stamina=8000.0, expect=dict(stamina=8000.0, stamina_capacity=130600.0))
    S('stamina: inc > capacity', stamina=1000.0, stamina_capacity=10.0,
      expect=dict(stamina=1010.0, stamina_capacity=0.0, recovery=1.0 - 2.0 ** -9, effort=1.0 - 2.0 ** -7))
    S('stamina: capacity 0, no recovery', stamina=1000.0, stamina_capacity=0.0, expect=dict(stamina=1000.0, stamina_capacity=0.0))
    S('stamina: capacity < 0 is unlimited', cfg='unlimited', stamina=5000.0, stamina_capacity=-1.0,
      expect=dict(stamina=5045.0, stamina_capacity=-1.0))
    # the three thresholds: recovery decays at stamina <= 2000, effort decays at <= 3000, grows at >= 4000
    for st, rec, eff0, eff in ((2000.0, 1.0 - 2.0 ** -9, 1.0, 1.0 - 2.0 ** -7), (up(2000.0), 1.0, 1.0, 1.0 - 2.0 ** -7),
                               (up(2000.0, -1), 1.0 - 2.0 ** -9, 1.0, 1.0 - 2.0 ** -7),
                               (3000.0, 1.0, 1.0, 1.0 - 2.0 ** -7), (up(3000.0), 1.0, 1.0, 1.0), (up(3000.0, -1), 1.0, 1.0, 1.0 - 2.0 ** -7),
                               (4000.0, 1.0, 0.75, 0.765625), (up(4000.0), 1.0, 0.75, 0.765625), (up(4000.0, -1), 1.0, 0.75, 0.75)):
        S(f'threshold: stamina {st!r}', stamina=st, effort=eff0, expect=dict(recovery=rec, effort=eff, stamina=st + rec * 45.0))
    S('threshold: effort and recovery at their minima', stamina=0.0, effort=0.5, recovery=0.5,
      expect=dict(effort=0.5, recovery=0.5, stamina=22.5))
    S('threshold: effort one increment below effort_init', effort=1.0 - 2.0 ** -6, expect=dict(effort=1.0))
    S('threshold: effort half an increment below effort_init', effort=1.0 - 2.0 ** -7, expect=dict(effort=1.0))
    # dash direction: side rate 0.5 at |dir| = 90, back rate 0.75 at 180, clamps, the back dash (power < 0: direction + 180)
    a0 = 100.0 / 128.0
    S('dash: dir 0', (DASH, 100.0, 0.0), expect=dict(player_x=a0, player_y=0.0, stamina=7945.0))
    S('dash: dir 90', (DASH, 100.0, 90.0), expect=dict(player_x=0.0, player_y=a0 * 0.5))
    S('dash: dir -90', (DASH, 100.0, -90.0), expect=dict(player_x=0.0, player_y=-a0 * 0.5))
    S('dash: dir 180', (DASH, 100.0, 180.0), expect=dict(player_x=-a0 * 0.75, player_y=0.0))
    S('dash: dir -180', (DASH, 100.0, -180.0), expect=dict(player_x=-a0 * 0.75, player_y=0.0))
    S('dash: dir 270 clamps to 180', (DASH, 100.0, 270.0), expect=dict(player_x=-a0 * 0.75, player_y=0.0))
    S('dash: back dash', (DASH, -50.0, 0.0), expect=dict(player_x=-50.0 / 128.0, player_y=0.0, stamina=7945.0))
    S('dash: back dash clamps at min_dash_power', (DASH, -150.0, 0.0), expect=dict(player_x=-a0, player_y=0.0, stamina=7845.0))
    S('dash: body + dir past 180', (DASH, 100.0, 90.0), player_body=170.0, ball_x=-20.0,
      expect=dict(player_x=a0 * 0.5 * np.cos(np.radians(-100.0)), player_y=a0 * 0.5 * np.sin(np.radians(-100.0))))
    # turn: moment clamps, the sign at +-180 (AngleDeg keeps +180 and -180 as they are; +-360 is +0), the inertia divisor
    S('turn: moment 270 clamps to 180', (TURN, 0.0, 270.0), expect=dict(player_body=180.0))
    S('turn: moment -270 clamps to -180', (TURN, 0.0, -270.0), expect=dict(player_body=-180.0))
    S('turn: body + turn = 180', (TURN, 0.0, 90.0), player_body=90.0, expect=dict(player_body=180.0))
    S('turn: body + turn = -180', (TURN, 0.0, -90.0), player_body=-90.0, expect=dict(player_body=-180.0))
    S('turn: body + turn = 360', (TURN, 0.0, 180.0), player_body=180.0, expect=dict(player_body='+0'))
    S('turn: body + turn = -360', (TURN, 0.0, -180.0), player_body=-180.0, expect=dict(player_body='+0'))
    S('turn: a moving player', (TURN, 0.0, 90.0), player_vx=0.25, expect=dict(player_body=45.0, player_x=0.25, player_vx=0.125))
    # observation angles
    S('obs: ball exactly behind', ball_x=-10.0, prev_dist=10.0, prev_angle=180.0, expect={'|obs0|': 1.0, 'obs1': 0.0})
    S('obs: ball at rest', expect=dict(obs6=0.0, obs7=0.0, obs8=0.0, obs9=0.0, obs0=0.0))
    S('obs: ball on the player', cfg='points', player_x=3.0, player_y=3.0, ball_x=3.0, ball_y=3.0, player_body=90.0, prev_dist=0.0,
      expect=dict(done=1, result=GOAL, obs0=-0.5, obs1=0.5, reward=10.0 - 0.5))
    S('obs: body 180', player_body=180.0, ball_x=-20.0, expect=dict(obs1=1.0, obs0=0.0))
    S('obs: body -180', player_body=-180.0, ball_x=-20.0, expect=dict(obs1=-1.0, obs0=0.0))
    # dash_angle_step ties: the action (k + 1/2) step / 180 is exact, dir / step is a tie; float64 takes the even grid point, fp32
    # multiplies by fl(1 / step) and may land on the other side
    for cfg, step, acts in (('step7.5', 7.5, (7 / 16, -7 / 16, 15 / 16, -15 / 16, 1 / 16)), ('step22.5', 22.5, (-15 / 16, 1 / 16, 3 / 16, 15 / 16)),
                            ('step45', 45.0, (-7 / 8, 1 / 8, 3 / 8, 7 / 8))):
        for a in acts:
            d = a * 180.0
            S(f'tie: step {step} dir {d}', a, cfg=cfg, ill=True, expect=dict(grid=step * float(np.rint(d / step)), step=step))
    return out


def scene_batch(cfg_name, items):
    """(cfg, rows [m, 19], actions, command?) of the scenes of one configuration"""
    cfg = make_cfg(SCENE_CONFIGS[cfg_name])
    rows = np.array([[s['row'][f] for f in F] for s in items], dtype=np.float64)
    rows[:, :NF] = rows[:, :NF].astype(f32)
    command = not cfg.task.use_continuous_action
    if command:
        a = np.array([list(s['action']) + [0.0] for s in items], dtype=f32)
    else:
        a = np.array([[s['action']] for s in items], dtype=f32)
    return cfg, rows, a, command


def _word(out, i, w):
    if w.startswith('obs') or w == '|obs0|':
        v = out['obs'][i, int(w.strip('|')[3:])]
        return abs(v) if w.startswith('|') else v
    return out['state'][i, IDX[w]] if w in IDX else out[w][i]


def dash_angle(out, i):
    return float(np.degrees(np.arctan2(out['state'][i, IDX['player_vy']], out['state'][i, IDX['player_vx']])))


def check_scene_f64(s, out, i):
    """failure strings: the hand-written answer against the float64 result `out`, row i"""
    fails = []
    for w, want in s['expect'].items():
        if w == 'step':
            continue
        if w == 'grid':
            if circ(dash_angle(out, i) - want) > 1e-6:
                fails.append(f"{s['name']}: float64 dashes towards {dash_angle(out, i)!r}, the half-even grid point is {want!r}")
            continue
        got = _word(out, i, w)
        if isinstance(want, str):
            ok = got == 0 and bool(np.signbit(got)) == (want == '-0')
        elif w in DISCRETE:
            ok = int(got) == int(want)
        else:
            ok = abs(got - want) <= FLOAT_TOL
        if not ok:
            fails.append(f"{s['name']}: {w} is {got!r} in float64, the hand-written answer is {want!r}")
    return fails


def check_scene_f32(s, g, b, i, unit):
    """failure strings: the fp32 result `g` against float64 `b` in scene s (row i): the same discrete words unless the scene is
    marked ill-conditioned; a tie scene dashes towards the float64 grid point or a neighbouring one; the signs of zeros and, within
    4 ulps of the word's unit (nothing in a scene rounds but the polynomials: 2.5e-7 relative for sincos), the exact floats."""
    fails = []
    if 'grid' in s['expect']:
        want, step = s['expect']['grid'], s['expect']['step']
        if min(circ(dash_angle(g, i) - (want + k * step)) for k in (-1, 0, 1)) > 1e-3:
            fails.append(f"{s['name']}: fp32 dashes towards {dash_angle(g, i)!r}, neither {want!r} nor a neighbouring grid point")
        return fails
    if s['ill']:
        return fails
    gd, bd = _discrete_words(g), _discrete_words(b)
    for w in DISCRETE:
        if gd[w][i] != bd[w][i]:
            fails.append(f"{s['name']}: {w} is {gd[w][i]!r} in fp32, {bd[w][i]!r} in float64")
    for w, want in s['expect'].items():
        got = _word(g, i, w)
        if isinstance(want, str):
            if not (got == 0 and bool(np.signbit(got)) == (want == '-0')):
                fails.append(f"{s['name']}: {w} is {got!r} in fp32, the hand-written answer is {want}")
        elif w not in DISCRETE:
            u = unit['obs'] if 'obs' in w else unit[w]
            if abs(got - want) > 4 * u:
                fails.append(f"{s['name']}: {w} is {got!r} in fp32, {abs(got - want) / u:.1f} ulps from the hand-written {want!r}")
    return fails


RESET_CONFIGS = {
    'max_steps 200': dict(use_continuous_action=False, change_ball_velocity=True),
    'max_steps 30': dict(use_continuous_action=False, change_ball_velocity=True, max_steps=30),
    'max_steps 200, noise': dict(use_continuous_action=False, change_ball_velocity=True, noise=True),
    'max_steps 30, noise': dict(use_continuous_action=False, change_ball_velocity=True, max_steps=30, noise=True),
    'fixed ball': dict(use_continuous_action=False, action_space_size=7, change_ball_position=False, ball_position_x=10,
                       ball_position_y=-5, ball_speed=1.5, ball_direction=30, max_steps=40),
    'random-server-1': random_server_kw(1),
}


def reset_episodes(n, seed=5):
    """episode counters before a masked reset, and the mask"""
    rs = np.random.RandomState(seed)
    return rs.randint(0, 2000, n), (rs.uniform(size=n) < 0.5).astype(np.uint8)


def stamina_table(cfg):
    """[max_steps + 1, 4]: stamina, effort, recovery, capacity before step s of an episode in which every command is Dash(100, .)
    (the discrete and 1-D continuous modes): the states on which the rollout kernels take the dash fast path.  Played by the fp32
    oracle from a reset."""
    orc = O.OracleEngine(cfg, 1, 'f32')
    orc.reset()
    rows = read_rows(orc)
    rows[0, IDX['player_x']], rows[0, IDX['player_y']], rows[0, IDX['ball_x']], rows[0, IDX['ball_y']] = 0.0, 0.0, 40.0, 0.0
    cols = [IDX[f] for f in ('stamina', 'effort', 'recovery', 'stamina_capacity')]
    out = []
    for s in range(cfg.task.max_steps + 1):
        out.append(rows[0, cols].copy())
        rows[0, IDX['player_x']], rows[0, IDX['player_y']] = 0.0, 0.0          # (stays inside, far from the ball: the episode goes on)
        rows[0, IDX['step_number']] = 0
        load_rows(orc, rows)
        orc.step(np.zeros(1, dtype=np.int64) if not cfg.task.use_continuous_action else np.zeros((1, 1), dtype=f32))
        rows = read_rows(orc)
    orc.close()
    return np.array(out)


def fast_path_rows(cfg, n, seed=9, foreign=None):
    """n rows that all qualify for the dash fast path (stamina words on the table of their step number, whole-degree bodies) and sit
    on what the table code must get right: speeds above the caps, a ball around min_distance_to_ball and inside the collision
    radius, a player around the touch and goal lines, step numbers up to max_steps.  foreign: the index of one env moved off the
    table (its group then runs the generic loop)."""
    rs = np.random.RandomState(seed)
    sp, t = cfg.sp, cfg.task
    r = written_states(cfg, n, seed)
    tab = stamina_table(cfg)
    sn = np.where(rs.uniform(size=n) < 0.3, t.max_steps - rs.randint(0, 2, n), rs.randint(0, t.max_steps + 1, n))
    r[:, IDX['step_number']] = sn
    for k, f in enumerate(('stamina', 'effort', 'recovery', 'stamina_capacity')):
        r[:, IDX[f]] = tab[sn, k]
    r[:, IDX['player_body']] = rs.randint(-180, 181, n)
    edge = rs.uniform(size=n)
    side = rs.choice([-1.0, 1.0], n)
    px, py = r[:, IDX['player_x']], r[:, IDX['player_y']]
    px[:] = np.where(edge < 0.15, side * (52.5 + rs.uniform(-1.0, 0.3, n)), px)
    py[:] = np.where((edge >= 0.15) & (edge < 0.3), side * (34.0 + rs.uniform(-1.0, 0.3, n)), py)
    ang = rs.uniform(-np.pi, np.pi, n)
    d = np.where(edge < 0.5, t.min_distance_to_ball + rs.uniform(-1.2, 1.2, n), rs.uniform(0, 2.0 * (sp.player_size + sp.ball_size), n))
    near = (edge >= 0.3) & (edge < 0.7)
    r[:, IDX['ball_x']] = np.where(near, px + d * np.cos(ang), r[:, IDX['ball_x']])
    r[:, IDX['ball_y']] = np.where(near, py + d * np.sin(ang), r[:, IDX['ball_y']])
    r[:, :NF] = r[:, :NF].astype(f32)
    r[:, IDX['prev_dist']] = np.hypot(r[:, IDX['ball_x']] - px, r[:, IDX['ball_y']] - py).astype(f32)
    if foreign is not None:
        r[foreign, IDX['stamina']] = float(f32(r[foreign, IDX['stamina']] - 123.25))
    return r


def fast_path_case(noise, n=512):
    """(config keywords, [(rows, actions)]) of the states that qualify for the dash fast path, under the headline configuration"""
    from test_gpu_parity import CONFIGS
    kw = dict(CONFIGS['dqn-discrete16'], noise=noise, max_steps=40)
    cfg = make_cfg(kw)
    rs = np.random.RandomState(31 + int(noise))
    return kw, [(fast_path_rows(cfg, n, seed=9 + j), random_actions(rs, cfg, n)) for j in range(2)]


def scene_state_case(auto_reset, n=512):
    """(config keywords, cfg, rows, actions): the state rows of the scenes of configuration A, repeated to n envs, each copy with
    another discrete action (what the rollout kernels can be given); with auto-reset on, the scenes that end an episode reset"""
    items = [s for s in scenes() if s['cfg'] == 'A']
    kw = dict(SCENE_CONFIGS['A'], auto_reset=auto_reset)
    _, rows, _, _ = scene_batch('A', items)
    m = len(items)
    rows = rows[np.arange(n) % m]
    rows[:, IDX['episode']] = 1 + np.arange(n) // m
    a = ((np.arange(n) // m) * 3 + np.arange(n) % 5).astype(np.int64) % 16
    return kw, make_cfg(kw), rows, a
