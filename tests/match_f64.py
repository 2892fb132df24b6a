"""One cycle of the 11v11 match from a shared state: an fp32 result (the fp32 oracle or the device) against the fp64 libm build of
the oracle, with a conditioning probe.  TEST INFRASTRUCTURE (tests/test_match_oracle_f64.py, tests/test_gpu_match_f64.py).

The rule (per env, after one cycle from the same state and actions):
  * the fp64 build runs from the state as given, from K copies whose float words are moved by a few fp32 ulps in a random
    direction (fixed seed), and from two copies scaled by a few ulps towards and away from the origin;
  * an env is ILL-CONDITIONED if any of these runs changes a discrete word (a threshold lies within a few ulps of the state);
  * a well-conditioned env must reproduce every fp64 discrete word exactly, and every float must satisfy
    |f32 - f64| <= T_field + 2 * spread, spread = the largest deviation of the perturbed fp64 runs from the unperturbed one;
  * the fraction of ill-conditioned envs is reported so that callers can cap it.
"""
import numpy as np

import match_oracle as MO
from soccer2d_amd import _capi_match as M

# the words a threshold decides (the conditioning probe watches these)
DISCRETE = ('mode', 'mode_side', 'score_left', 'score_right', 'last_touch_side', 'setplay_timer', 'offside_mask', 'ball_holder',
            'goalie_moves', 'set_play_taker', 'last_kicker', 'tackle_cycles', 'catch_ban', 'card', 'done')
# nearest_left / nearest_right are an argmin of distances that may tie to the last bit: the fp32 pick must be a nearest player of the
# fp64 state within NEAREST_SLACK_M plus four times the env's position spread, not the same index
# counters no threshold decides: always equal
CLOCKS = ('cycle', 'stopped_cycle', 'tick')
OBJ_FLOATS = ('x', 'y', 'vx', 'vy', 'body', 'stamina', 'effort', 'recovery', 'stamina_capacity')
# the unit of each tolerance: one fp32 ulp at the field's natural magnitude (pitch half length, ball_speed_max, 180 deg,
# stamina_max, 1, stamina_capacity, a goal)
UNIT = {f: float(np.spacing(np.float32(m))) for f, m in (('x', 52.5), ('y', 52.5), ('vx', 3.0), ('vy', 3.0), ('body', 180.0),
                                                         ('stamina', 8000.0), ('effort', 1.0), ('recovery', 1.0),
                                                         ('stamina_capacity', 130600.0), ('reward_left', 1.0))}
# T_field in those units.  Measured over the CPU corpus of tests/test_match_oracle_f64.py (max over well-conditioned envs of
# (|f32 - f64| - 2 spread) / unit, every source, noise off and on); each T is at most 4x the measured maximum (in the comment).
T_ULPS = {'x': 1.5, 'y': 1.5,            # measured 0.38, 0.41
          'vx': 6.0, 'vy': 3.5,          # measured 1.71, 0.95
          'body': 7.0, 'effort': 0.8,    # measured 1.82, 0.20
          'stamina': 0.0, 'recovery': 0.0, 'stamina_capacity': 0.0, 'reward_left': 0.0}   # measured 0 (equal within the spread)
K_PROBES, PROBE_ULPS = 4, 3
NEAREST_SLACK_M = 1e-3


def _discrete(s):
    return {k: s[k][:, :23] if s[k].ndim == 2 else s[k] for k in DISCRETE + CLOCKS}


def perturb(state, rs, ulps=PROBE_ULPS, scale=0):
    """a copy of `state` with every float word of the 23 objects moved by 1..ulps fp32 ulps in a random direction; scale = -1 / +1:
    every word moved by `ulps` ulps towards / away from zero instead (the whole scene scaled about the origin: every distance moves
    by a few ulps in the same direction, which flips a distance threshold that random directions can cancel)"""
    out = {k: v.copy() for k, v in state.items()}
    for f in OBJ_FLOATS:
        v = out[f][:, :23].astype(np.float32)
        if scale:
            steps = np.where(v < 0, -1, 1) * scale * ulps
        else:
            steps = rs.randint(1, ulps + 1, size=v.shape) * rs.choice([-1, 1], size=v.shape)
        for k in range(ulps):
            move = np.abs(steps) > k
            v = np.where(move, np.nextafter(v, np.where(steps > 0, np.float32(np.inf), np.float32(-np.inf))), v)
        out[f][:, :23] = v
    return out


def step_from(cfg, state, actions, ids, prec):
    o = MO.MatchOracle(cfg, len(ids), prec)
    o.set_env_ids(ids)
    o.load(state)
    o.step(actions)
    return o.snapshot(), o.events()


def f32_step(cfg, state, actions, ids):
    return step_from(cfg, state, actions, ids, 'f32')


def compare(cfg, state, actions, ids, f32_after, seed=0xF64, probes=K_PROBES):
    """(report dict, list of failure strings).  state / f32_after: {MATCH_BUFFER_FIELDS name: array}; ids: Philox env ids."""
    ids = np.asarray(ids, dtype=np.int64)
    n = len(ids)
    base, _ = step_from(cfg, state, actions, ids, 'f64')
    rs = np.random.RandomState(seed)
    bd = _discrete(base)
    ill = np.zeros(n, bool)
    ill_words = {}
    spread = {f: np.zeros((n, 23)) for f in OBJ_FLOATS}
    spread['reward_left'] = np.zeros(n)
    for k in range(probes + 2):
        scale = 0 if k < probes else (-1 if k == probes else 1)
        p, _ = step_from(cfg, perturb(state, rs, scale=scale), actions, ids, 'f64')
        pd = _discrete(p)
        for w in DISCRETE:
            d = pd[w] != bd[w]
            d = d.any(axis=1) if d.ndim == 2 else d
            ill_words[w] = ill_words.get(w, 0) + int((d & ~ill).sum())
            ill |= d
        for f in spread:
            dv = _fdiff(f, p[f][:, :23] if p[f].ndim == 2 else p[f], base[f][:, :23] if base[f].ndim == 2 else base[f])
            spread[f] = np.maximum(spread[f], dv)
    well = ~ill
    fails = []
    gd = _discrete(f32_after)
    for k in DISCRETE + CLOCKS:
        d = gd[k] != bd[k]
        d = d.any(axis=1) if d.ndim == 2 else d
        bad = np.flatnonzero(d & (well if k in DISCRETE else True))
        if len(bad):
            e = bad[0]
            fails.append(f'{k}: {len(bad)} well-conditioned envs differ; env {e} (id {ids[e]}): f32={gd[k][e]!r} f64={bd[k][e]!r}')
    bx, by = base['x'][:, 22], base['y'][:, 22]
    d = np.hypot(base['x'][:, :22] - bx[:, None], base['y'][:, :22] - by[:, None])
    for k, sl in (('nearest_left', slice(0, 11)), ('nearest_right', slice(11, 22))):
        pick = d[np.arange(n), f32_after[k].astype(np.int64)]
        slack = pick - d[:, sl].min(axis=1)
        allowed = NEAREST_SLACK_M + 4.0 * np.maximum(spread['x'], spread['y']).max(axis=1)    # (positions the probe moves)
        bad = np.flatnonzero((slack > allowed) | ~np.isin(f32_after[k], np.arange(22)[sl]))
        if len(bad):
            e = bad[0]
            fails.append(f'{k}: {len(bad)} envs pick a player {slack[e]:.3g} m farther than the nearest; env {e}: '
                         f'f32={f32_after[k][e]} f64={base[k][e]}')
    worst = {}
    for f in spread:
        g = f32_after[f][:, :23] if f32_after[f].ndim == 2 else f32_after[f]
        b = base[f][:, :23] if base[f].ndim == 2 else base[f]
        err = _fdiff(f, g.astype(np.float64), b)
        excess = (err - 2.0 * spread[f]) / UNIT[f]
        excess = np.where(well[:, None] if excess.ndim == 2 else well, excess, -np.inf)
        worst[f] = float(excess.max()) if n else -np.inf
        if worst[f] > T_ULPS[f]:
            i = np.unravel_index(np.argmax(excess), excess.shape)
            fails.append(f'{f}: |f32 - f64| - 2 spread = {worst[f]:.1f} ulps > {T_ULPS[f]} at {i} (env id {ids[i[0]]}): '
                         f'f32={g[i]!r} f64={b[i]!r} spread={spread[f][i]!r}')
    return dict(n=n, ill=int(ill.sum()), ill_words=ill_words, well=well, worst=worst, f64=base), fails


def _fdiff(f, a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    if f == 'body':
        d = np.minimum(d, 360.0 - d)
    return d


class Tally:
    """what the compared cycles covered, the worst excess per field and the ill-conditioned fraction per source"""

    def __init__(self):
        self.events = dict(kick=0, tackle=0, catch=0, collision=0, goal=0)
        self.modes = set()
        self.worst = {f: -np.inf for f in T_ULPS}
        self.ill = {}
        self.ill_max = {}              # the largest ill-conditioned fraction of one checkpoint (one compared batch) per source
        self.ill_words = {}
        self.fails = []

    def add(self, source, state, rep, fails, events, f32_after):
        for name, bit in (('kick', MO.EV_KICK), ('tackle', MO.EV_TACKLE), ('catch', MO.EV_CATCH), ('collision', MO.EV_COLLIDE),
                          ('goal', MO.EV_GOAL)):
            self.events[name] += int(((events & bit) != 0).sum())
        self.modes |= set(np.unique(state['mode']).tolist()) | set(np.unique(f32_after['mode']).tolist())
        for f, v in rep['worst'].items():
            self.worst[f] = max(self.worst[f], v)
        a, b = self.ill.get(source, (0, 0))
        self.ill[source] = (a + rep['ill'], b + rep['n'])
        self.ill_max[source] = max(self.ill_max.get(source, 0.0), rep['ill'] / max(rep['n'], 1))
        for k, v in rep['ill_words'].items():
            self.ill_words[k] = self.ill_words.get(k, 0) + v
        self.fails += [f'{source}: {m}' for m in fails]

    def ill_fraction(self, source):
        assert source in self.ill, f'no checkpoint of {source!r} was compared'
        a, b = self.ill[source]
        return a / max(b, 1)


def edge_states():
    """(state, actions) of constructed edge states for the default configuration: exact contacts, the kickable distance, the goal line, a post,
    the touch line, +-0 velocities, body +-180, speed at the cap, stamina at the effort / recovery thresholds, a goalie holding the
    ball at the edge of the penalty area, catches on the edges of the catch rectangle.  Every state is played with several commands (the same state in several envs)."""
    base = MO.MatchOracle(MO.make_match_config(), 1).snapshot()
    base['x'][0, 10], base['y'][0, 10] = -10.5, 6.0                  # (the kick-off taker back in the formation, clear of the scenes)
    f32 = np.float32
    ka = f32(f32(0.3) + f32(0.085)) + f32(0.7)                      # kickable area of the default type (fp32, as the engine)
    scenes = []

    def scene(mode=M.GM_PLAY_ON, side=0, **words):
        s = {k: v.copy() for k, v in base.items()}
        s['mode'][:] = mode; s['mode_side'][:] = side; s['set_play_taker'][:] = 0
        for k, v in words.items():
            s[k][:] = v
        s['tick'][:] = 77; s['cycle'][:] = 77
        scenes.append(s)
        return s

    def put(s, slot, **kv):
        for k, v in kv.items():
            s[k][0, slot] = v
    # two players exactly in contact (0.3 + 0.3), head on and at an angle; three in a chain
    for dx, dy in ((f32(0.3) + f32(0.3), 0.0), (0.0, f32(0.3) + f32(0.3)), (0.36, 0.48)):
        s = scene(); put(s, 5, x=10.0, y=10.0, vx=0.0, vy=0.0); put(s, 16, x=10.0 + dx, y=10.0 + dy, vx=0.0, vy=0.0)
    s = scene()
    for k, i in enumerate((5, 16, 6)):
        put(s, i, x=f32(10.0) + f32(k) * f32(0.6), y=10.0, vx=0.0, vy=0.0, body=0.0)
    s = scene()
    for k, i in enumerate((5, 16, 6)):
        put(s, i, x=f32(10.0) + f32(k) * f32(0.59), y=0.0, vx=0.01 * (1 - k), vy=0.0, body=0.0)
    # the ball exactly at the kickable distance of player 9 (in front, behind, diagonal); player and ball exactly in contact
    for ang in (0.0, 180.0, 45.0, -90.0):
        s = scene(); put(s, 9, x=0.0, y=0.0, body=0.0, vx=0.0, vy=0.0)
        c, sn = np.cos(np.radians(ang)), np.sin(np.radians(ang))
        put(s, 22, x=f32(ka * c), y=f32(ka * sn), vx=0.0, vy=0.0)
    s = scene(); put(s, 9, x=0.0, y=0.0, vx=0.0, vy=0.0); put(s, 22, x=f32(0.3) + f32(0.085), y=0.0, vx=0.0, vy=0.0)
    # ball on the goal line (in and beside the goal), on a post, on the touch line; moving out and standing
    for bx, by, vx, vy in ((52.5, 0.0, 0.0, 0.0), (52.5, 0.0, 0.5, 0.0), (-52.5, 3.0, -0.5, 0.0), (52.5, 7.01, 0.3, 0.0),
                           (52.5, -7.01, 0.3, 0.0), (-52.5, 7.01, -0.3, 0.1), (10.0, 34.0, 0.0, 0.2), (-20.0, -34.0, 0.1, -0.2),
                           (52.5, 34.0, 0.2, 0.2)):
        s = scene(last_touch_side=1); put(s, 22, x=bx, y=by, vx=vx, vy=vy)
        put(s, 10, x=bx - np.sign(bx or 1.0) * 0.8, y=by, body=0.0 if bx >= 0 else 180.0)
    # +-0 velocities of players and ball
    for z in (0.0, -0.0):
        s = scene(); put(s, 9, x=-5.0, y=0.0, vx=z, vy=-z); put(s, 22, x=-4.0, y=0.0, vx=-z, vy=z)
        put(s, 3, vx=-0.0, vy=-0.0)
    # body at +-180 (dash, turn, kick, tackle from it)
    for b in (180.0, -180.0, 179.99998, -179.99998):
        s = scene(); put(s, 9, x=0.0, y=0.0, body=b, vx=0.0, vy=0.0); put(s, 22, x=-0.8, y=0.0, vx=0.0, vy=0.0)
    # speed exactly at the cap: player 1.05 (x, diagonal), ball 3.0
    s = scene(); put(s, 5, vx=1.05, vy=0.0, body=0.0); put(s, 22, x=0.0, y=20.0, vx=3.0, vy=0.0)
    s = scene(); put(s, 5, vx=f32(1.05) * f32(0.6), vy=f32(1.05) * f32(0.8), body=53.130102); put(s, 22, x=0.0, y=20.0, vx=0.0, vy=-3.0)
    # stamina exactly at the thresholds (effort_dec / recover_dec = 0.3 * 8000, effort_inc = 0.6 * 8000), an effort at its bounds
    for st in (2400.0, 4800.0, 2399.9998, 4800.0005, 0.0, 8000.0):
        s = scene()
        for i in range(22):
            put(s, i, stamina=st, effort=0.6 if st < 2400.5 else 0.99, recovery=0.5 if st == 0.0 else 0.8)
    # a goalie holding the ball at the edge of his penalty area (x = -(52.5 - 16.5), |y| = 20.16): free kick with moves left
    for gx, gy in ((-36.0, 20.16), (-36.0, -20.16), (-52.5, 0.0), (-36.0, 0.0)):
        s = scene(M.GM_FREE_KICK, 1, ball_holder=1, goalie_moves=2)
        put(s, 0, x=gx, y=gy, body=0.0, vx=0.0, vy=0.0); put(s, 22, x=gx + 0.485, y=gy, vx=0.0, vy=0.0)
    # a goalie catching the ball exactly on the edge of the area and of his catch rectangle
    for gx, gy in ((-36.0, 0.0), (-36.0 - 1.2, 20.16)):
        s = scene(last_touch_side=2); put(s, 0, x=gx, y=gy, body=0.0, vx=0.0, vy=0.0); put(s, 22, x=gx + 1.2, y=gy, vx=0.0, vy=0.0)
    # a goalie with the ball in his catch rectangle (1.2 long, 1 wide, turned to body + dir): on its edges, inside and outside his
    # penalty area (GoalieCatch_ / CatchFault_), the right goalie as well
    for g, sgn in ((0, 1.0), (11, -1.0)):
        for gx, bx, by in ((-45.0, 0.6, 0.0), (-45.0, 1.2, 0.0), (-45.0, 0.6, 0.5), (-45.0, 0.0, 0.0), (-36.5, 1.0, 0.2),
                           (-30.0, 0.6, 0.0), (-36.0, 0.6, 0.0), (-45.0, 1.0, -0.5)):
            s = scene(last_touch_side=2 if g == 0 else 1)
            put(s, g, x=sgn * gx, y=3.0, body=0.0 if g == 0 else 180.0, vx=0.0, vy=0.0, catch_ban=0)
            put(s, 22, x=sgn * (gx + bx), y=3.0 + sgn * by, vx=sgn * -0.3, vy=0.0)
    # the commands every scene is played with (slots 0, 5, 9, 10 act; everybody else dashes towards the ball)
    cmds = [(M.MCMD_DASH, 100.0, 0.0), (M.MCMD_DASH, 100.0, 180.0), (M.MCMD_DASH, 37.5, -90.0), (M.MCMD_TURN, 180.0, 0.0),
            (M.MCMD_TURN, -180.0, 0.0), (M.MCMD_KICK, 100.0, 0.0), (M.MCMD_KICK, 100.0, 180.0), (M.MCMD_KICK, 55.0, -45.0),
            (M.MCMD_TACKLE, 100.0, 0.0), (M.MCMD_TACKLE, -90.0, 1.0), (M.MCMD_CATCH, 0.0, 0.0), (M.MCMD_CATCH, 90.0, 0.0),
            (M.MCMD_MOVE, -36.0, 20.16), (M.MCMD_MOVE, -52.5, -20.16), (M.MCMD_NONE, 0.0, 0.0)]
    state = {k: np.concatenate([np.repeat(s[k], len(cmds), axis=0) for s in scenes]) for k in base}
    a = np.zeros((len(state['mode']), 22, 3), dtype=np.float32)
    for j in range(len(scenes)):
        for k, c in enumerate(cmds):
            row = a[j * len(cmds) + k]
            row[:] = (M.MCMD_DASH, 60.0, 0.0)
            for i in (0, 5, 9, 10, 11, 16):
                row[i] = c
    return state, a
