"""The rule-scene table of the 11v11 match engine.  TEST INFRASTRUCTURE.

A scene is plain data: a name, the keyword arguments of match_oracle.make_match_config, `n` matches, edits to the state after the
reset (the shared setters: ('obj', envs, slot, fields) / ('game', envs, fields) / ('card', envs, slot, card)), an action source
(None: the in-engine random policy of the configuration's seed; else a list of (cycles, envs, slot, (command, a, b)) rows that are
expanded to one [T, n, 22, 3] array), resets by mask before given cycles, `T` cycles, and a witness: a predicate on the oracle's
trajectory that says the scene reached the rule it is named after.  One match per variant of the rule: left and right, both signs,
the value on either side of a comparison.  tests/test_match_scenes_host.py runs the table on the oracle and measures, with gcov,
that it reaches every line and branch direction of the oracle's step and reset path but those of ALLOW (below);
tests/test_gpu_match_scenes.py runs it on the kernel, every word of every cycle against the oracle.
"""
from collections import namedtuple

import numpy as np

import match_oracle as MO
from soccer2d_amd import _capi_match as M

LEFT, RIGHT = 1, 2
NONE, DASH, TURN, KICK, TACKLE, CATCH, MOVE = (M.MCMD_NONE, M.MCMD_DASH, M.MCMD_TURN, M.MCMD_KICK, M.MCMD_TACKLE, M.MCMD_CATCH,
                                               M.MCMD_MOVE)
BALL = 22

Scene = namedtuple('Scene', 'name cfg n T edits actions witness resets')

# configuration words the kernel's stock instantiations take as per-engine words: a scene that changes only these (or nothing)
# runs the stock kernel (or the stock rules with the engine's own schedule), and is run through the general one as well
SCHEDULE_WORDS = frozenset((
    'seed', 'env_id_offset', 'auto_reset', 'noise', 'half_time_cycles', 'nr_normal_halfs', 'drop_ball_time', 'after_goal_wait',
    'kick_off_wait', 'announce_wait', 'nr_extra_halfs', 'extra_half_cycles', 'golden_goal', 'penalty_shoot_outs',
    'pen_before_setup_wait', 'pen_ready_wait', 'pen_taken_wait', 'pen_nr_kicks', 'pen_max_extra_kicks'))


def stock_accepts(scene):
    return set(scene.cfg) <= SCHEDULE_WORDS


# ------------------------------------------------------------------ running a scene
def _envs(envs, n):
    if envs is None:
        return range(n)
    return (envs,) if isinstance(envs, int) else envs


def apply_edits(orc, edits):
    for ed in edits:
        if ed[0] == 'obj':
            for e in _envs(ed[1], orc.n):
                orc.set_obj(e, ed[2], **ed[3])
        elif ed[0] == 'game':
            for e in _envs(ed[1], orc.n):
                orc.set_game(e, **ed[2])
        elif ed[0] == 'card':
            for e in _envs(ed[1], orc.n):
                assert orc.L.s2dmo_set_card(orc.h, e, ed[2], ed[3]) == 0
        else:
            raise ValueError(ed[0])


def make_oracle(scene, prec='f32'):
    """the oracle of a scene in its initial state"""
    orc = MO.MatchOracle(MO.make_match_config(**scene.cfg), scene.n, prec)
    apply_edits(orc, scene.edits)
    return orc


def scene_actions(scene):
    """float32 [T, n, 22, 3], or None for the random policy"""
    if scene.actions is None:
        return None
    a = np.zeros((scene.T, scene.n, 22, 3), dtype=np.float32)
    for ts, envs, slot, cmd in scene.actions:
        ts = range(scene.T) if ts is None else ((ts,) if isinstance(ts, int) else ts)
        for t in ts:
            for e in _envs(envs, scene.n):
                a[t, e, slot] = cmd
    return a


def reset_mask(scene, t):
    """uint8 [n] mask of the reset before cycle t, or None"""
    for rt, mask in scene.resets:
        if rt == t:
            return np.ones(scene.n, dtype=np.uint8) if mask is None else np.asarray(mask, dtype=np.uint8)
    return None


class Trajectory:
    """what the oracle did: f[name] = [T, n(, 24)] of every state word after each cycle, events [T, n], stats [T, 8], actions"""

    def __init__(self, scene):
        self.scene, self.f, self.events, self.stats, self.actions = scene, {}, [], [], []

    def add(self, orc, act):
        for k, v in orc.snapshot().items():
            self.f.setdefault(k, []).append(v)
        self.events.append(orc.events()); self.stats.append(orc.stats()); self.actions.append(act)

    def close(self):
        self.f = {k: np.stack(v) for k, v in self.f.items()}
        self.events, self.stats, self.actions = np.stack(self.events), np.stack(self.stats), np.stack(self.actions)
        return self

    def __getitem__(self, name):
        return {'stats': self.stats, 'events': self.events}.get(name, self.f.get(name))

    def saw(self, mode, e=None, side=None):
        hit = self.f['mode'] == mode
        if side is not None:
            hit &= self.f['mode_side'] == side
        return bool(hit.any() if e is None else hit[:, e].any())

    def event(self, bit, e=None):
        hit = (self.events & bit) != 0
        return bool(hit.any() if e is None else hit[:, e].any())


def run_on_oracle(scene, prec='f32', each=None):
    """the scene's trajectory; each(t, orc, actions of the cycle, reset mask or None) after every cycle (the GPU test's hook)"""
    orc = make_oracle(scene, prec)
    acts = scene_actions(scene)
    tr = Trajectory(scene)
    for t in range(scene.T):
        mask = reset_mask(scene, t)
        if mask is not None:
            orc.reset(None if mask.all() else mask)
        a = orc.random_actions() if acts is None else acts[t]
        orc.step(None if acts is None else a)
        tr.add(orc, a)
        if each is not None:
            each(t, orc, a, mask)
    return tr.close()


# ------------------------------------------------------------------ builders
def obj(envs, slot, **kw):
    return ('obj', envs, slot, kw)


def game(envs, **kw):
    return ('game', envs, kw)


def card(envs, slot, c):
    return ('card', envs, slot, c)


PLAY_ON = game(None, mode=M.GM_PLAY_ON, mode_side=0)


def ball(envs, x, y, vx=0.0, vy=0.0):
    return obj(envs, BALL, x=x, y=y, vx=vx, vy=vy)


def pen_word(taker=0, kicks=(0, 0), goals=(0, 0)):
    """the shoot-out's state in the set-play word (include/s2d_match.h)"""
    return (taker + 1 if taker is not None else 0) | kicks[0] << 12 | kicks[1] << 16 | goals[0] << 20 | goals[1] << 24


def mirrored(edits):
    """the same edits for the other team: slots swapped, x and body mirrored (y kept)"""
    out = []
    for ed in edits:
        if ed[0] == 'obj':
            kw = dict(ed[3])
            for k in ('x', 'vx'):
                if k in kw:
                    kw[k] = -kw[k]
            if 'body' in kw:
                kw['body'] = 180.0 - kw['body'] if kw['body'] >= 0 else -180.0 - kw['body']
            slot = ed[2] if ed[2] == BALL else (ed[2] + 11) % 22
            out.append(('obj', ed[1], slot, kw))
        elif ed[0] == 'card':
            out.append(('card', ed[1], (ed[2] + 11) % 22, ed[3]))
        else:
            raise ValueError(ed[0])
    return out


def at_env(e, edits):
    return [(ed[0], e) + tuple(ed[2:]) for ed in edits]


SCENES = []


def scene(name, cfg, n, T, edits, actions, witness, resets=()):
    assert n <= 64 and T <= 400 and all(s.name != name for s in SCENES)
    SCENES.append(Scene(name, dict(cfg), n, T, list(edits), actions if actions is None else list(actions), witness, tuple(resets)))


def by_name(name):
    (s,) = [s for s in SCENES if s.name == name]
    return s


# ================================================================== the table
# ---- reset, kick-off, masked reset
scene('kick_off_and_masked_reset', {}, 4, 5, [],
      [(0, 0, 10, (KICK, 100, 0)),                       # the taker puts the ball into play
       (0, 1, 21, (KICK, 100, 0)),                       # the other side may not
       (0, 2, 5, (KICK, 100, 0)),                        # too far
       (0, 3, 3, (MOVE, -12, 5)), (0, 3, 14, (MOVE, -30, -4)), (0, 3, 5, (MOVE, 20, 50)),     # Move before the kick-off, clamped
       (4, None, 3, (DASH, 60, 0))],
      lambda tr: tr['mode'][0, 0] == M.GM_PLAY_ON and tr['mode'][0, 1] == M.GM_KICK_OFF and tr['x'][0, 3, 5] == 0.0
      and tr['mode'][2, 0] == M.GM_PLAY_ON and list(tr['tick'][2]) == [3, 3, 1, 1] and (tr['tick'][3] == 1).all() and (tr['mode'][3] == M.GM_KICK_OFF).all(),
      resets=[(2, [0, 0, 1, 1]), (3, None)])

# ---- BeforeKickOff, the drop ball, half time, time over with and without the automatic reset
for _auto in (1, 0):
    scene('before_kick_off_half_time_time_over' + ('' if _auto else '_no_auto_reset'),
          dict(kick_off_wait=3, half_time_cycles=5, nr_extra_halfs=0, penalty_shoot_outs=0, drop_ball_time=2, auto_reset=_auto), 2, 26, [],
          [(0, None, 10, (KICK, 100, 0)), (0, None, 3, (MOVE, -20, 5)), (1, None, 14, (MOVE, -12, -3)),
           (range(4, 26), 0, 10, (KICK, 30, 0)), (range(20, 26), None, 4, (DASH, 50, 0))],
          lambda tr: tr.saw(M.GM_BEFORE_KICK_OFF) and tr.saw(M.GM_FIRST_HALF_OVER) and tr['done'].any() and tr.saw(M.GM_PLAY_ON, 1)
          and tr.saw(M.GM_TIME_OVER) != bool(tr.scene.cfg['auto_reset']))

# ---- Dash: direction rates, the power and angle clamps, stamina that runs out, speed limit; Turn with and without speed
_DASH = [(100, 0), (100, 90), (100, 135), (100, -135), (100, 180), (150, 200), (-50, -200), (100, 45.4), (100, 0), (100, 0), (30, 0), (100, 0)]
scene('dash_directions_and_empty_stamina', {}, len(_DASH), 4,
      [PLAY_ON, obj(8, 5, stamina=30.0), obj(9, 5, stamina=0.0), obj(10, 5, stamina=60.0), obj(11, 5, vx=0.9), obj(None, 6, vx=0.8, vy=0.3)],
      [(None, e, 5, (DASH, p, d)) for e, (p, d) in enumerate(_DASH)] +
      [(None, None, 6, (TURN, 90, 0)), (None, None, 7, (TURN, -300, 0)), (None, 0, 8, (TURN, 300, 0))],
      lambda tr: tr['stamina'][0, 8, 5] == tr['stamina'][0, 9, 5] and tr['stamina'][0, 10, 5] > 0 and tr['y'][0, 1, 5] > -22.0
      and tr['x'][0, 4, 5] < -20.0 and tr['vx'][0, 11, 5] == np.float32(1.05) * np.float32(0.4) and tr['body'][0, 0, 7] == -180.0 and 0 < tr['body'][0, 0, 6] < 90)

# ---- the back dash (min_dash_power < 0), no angle quantisation, the acceleration limit
_BACK = [(-80, 0), (-80, 120), (100, 33.3), (-100, 0), (-100, 0), (100, 0)]
scene('back_dash', dict(server=dict(min_dash_power=-100.0, dash_angle_step=0.0, player_accel_max=0.3)), len(_BACK), 3,
      [PLAY_ON, obj(3, 5, stamina=100.0), obj(4, 5, stamina=400.0)],
      [(None, e, 5, (DASH, p, d)) for e, (p, d) in enumerate(_BACK)],
      lambda tr: tr['x'][0, 0, 5] == np.float32(-20.3) and tr['stamina'][0, 0, 5] == 8000 - 160 + 45 and tr['x'][0, 5, 5] == np.float32(-19.7)
      and 0 < tr['stamina'][0, 3, 5] < 45 and tr['stamina'][0, 4, 5] == tr['stamina'][0, 3, 5] + 200 and tr['vy'][0, 2, 5] > 0
      and tr['vy'][0, 1, 5] < 0)

# ---- the stamina model: recovery and effort floors, effort ceiling, the room and capacity clamps (one player per variant)
_STAMINA = {1: dict(stamina=2000.0, recovery=0.501, effort=0.602), 2: dict(stamina=2000.0, recovery=0.5, effort=0.6),
            3: dict(stamina=2000.0, recovery=0.9, effort=0.9), 4: dict(stamina=5000.0, effort=0.995), 5: dict(stamina=5000.0, effort=0.9),
            6: dict(stamina=7990.0), 7: dict(stamina=3000.0, stamina_capacity=10.0), 8: dict(stamina=3000.0, stamina_capacity=0.0),
            9: dict(stamina=3000.0, stamina_capacity=-5.0), 12: dict(stamina=8100.0), 13: dict(stamina=2400.0, recovery=0.8, effort=0.8),
            14: dict(stamina=4800.0, effort=0.8), 15: dict(stamina=2400.5, recovery=0.8, effort=0.8), 16: dict(stamina=4799.5, effort=0.8)}
scene('stamina_floors_and_clamps', {}, 1, 3, [PLAY_ON] + [obj(0, s, **kw) for s, kw in _STAMINA.items()], [],
      lambda tr: tr['recovery'][0, 0, 1] == np.float32(0.5) and tr['effort'][0, 0, 1] == np.float32(0.6) and tr['effort'][0, 0, 4] == 1.0
      and tr['stamina'][0, 0, 6] == 8000.0 and tr['stamina'][0, 0, 7] == 3010.0 and tr['stamina_capacity'][0, 0, 7] == 0.0
      and tr['stamina'][0, 0, 8] == 3000.0 and tr['stamina'][0, 0, 12] == 8000.0)

# ---- no stamina capacity (< 0), and a player type whose increment overshoots stamina_max by a rounding: the last clamp
scene('stamina_without_capacity_and_overshoot',
      dict(server=dict(stamina_capacity=-1.0, stamina_max=100.1), player_types={3: dict(stamina_inc_max=9000.0, player_size=0.4, kickable_margin=0.9)},
           player_type_id=[3 if i in (5, 16) else 0 for i in range(22)]), 1, 3,
      [PLAY_ON] + [obj(0, 5, stamina=2.477855682373047), obj(0, 16, stamina=3.3535118103027344), obj(0, 6, stamina=100.0)], [(None, 0, 6, (DASH, 100, 0))],
      lambda tr: tr['stamina'][0, 0, 5] == np.float32(100.1) and tr['stamina'][0, 0, 16] == np.float32(100.1) and tr['stamina_capacity'][0, 0, 5] == -1.0
      and np.float32(2.477855682373047) + (np.float32(100.1) - np.float32(2.477855682373047)) > np.float32(100.1))

# ---- Kick: two kickers (acceleration limit), a fast ball (speed limit), clamps, out of reach
scene('kick_limits', {}, 5, 3,
      [PLAY_ON, ball(None, 5.0, 0.0), obj(None, 9, x=4.4, y=0.0, body=0.0), obj(0, 20, x=5.0, y=0.6, body=0.0),
       ball(1, 5.0, 0.0, vx=2.5), obj(4, 9, x=3.0, y=0.0)],
      [(0, 0, 9, (KICK, 100, 0)), (0, 0, 20, (KICK, 100, 0)), (0, 1, 9, (KICK, 100, 0)), (0, 2, 9, (KICK, 150, 200)),
       (0, 3, 9, (KICK, -150, -200)), (0, 4, 9, (KICK, 100, 0))],
      lambda tr: tr.event(MO.EV_KICK, 0) and tr['vx'][0, 0, BALL] == np.float32(2.7) * np.float32(0.94) and tr['vx'][0, 4, BALL] == 0
      and abs(float(tr['vx'][0, 1, BALL]) - 3.0 * 0.94) < 1e-5 and tr['stats'][0, 4] == 5)

# ---- the noise model: movement, turn, kick and ball noise under the random policy (kick-off crowd)
scene('noise_random_policy', dict(noise=1, half_time_cycles=60, drop_ball_time=5), 24, 150, [], None,
      lambda tr: tr['stats'][-1, 4] > 0 and tr['stats'][-1, 5] > 0 and tr.event(MO.EV_COLLIDE))
scene('random_policy_short_match', dict(half_time_cycles=40, extra_half_cycles=10, drop_ball_time=4, after_goal_wait=3, announce_wait=3,
                                        pen_before_setup_wait=1, pen_ready_wait=2, pen_taken_wait=6, pen_nr_kicks=2, pen_max_extra_kicks=1),
      32, 300, [], None,
      lambda tr: tr['done'].any() and tr.saw(M.GM_EXTEND_HALF) and tr.saw(M.GM_PENALTY_SETUP))

# ---- Tackle: in front, behind (tackle_back_dist = 0), exactly beside, out of reach, with the foul flag, in a set play of the others
_TB = [(-19.0, -22.0), (-21.0, -22.0), (-20.0, -21.0), (-17.9, -22.0), (-19.0, -22.0), (-19.0, -22.0), (-19.0, -22.0)]
scene('tackle_geometry', {}, len(_TB), 3,
      [PLAY_ON, game(6, mode=M.GM_KICK_IN, mode_side=RIGHT)] + [ball(e, x, y) for e, (x, y) in enumerate(_TB)],
      [(0, None, 5, (TACKLE, 0, 0)), (0, 4, 5, (TACKLE, 0, 1)), (0, 5, 5, (TACKLE, 200, 0)), (1, None, 5, (DASH, 100, 0))],
      lambda tr: (tr['tackle_cycles'][0, :, 5] == 10).all() and tr['vx'][0, 0, BALL] > 0 and tr['vx'][0, 2, BALL] > 0
      and (tr['vx'][0, [1, 3, 5, 6], BALL] == 0).all() and (tr['vx'][1, :, 5] == 0).all() and tr['stats'][0, 5] == 7)

# ---- Catch: the goalie's rectangle on every side, the ban, field players, both goalies at once, faults outside the area,
#      the held ball carried by Move (goalie_max_moves), then played
_CATCH_EDITS = [PLAY_ON, ball(0, -49.2, 0.3, vx=-1.0), ball(1, -33.8, -20.0), ball(2, -48.5, 0.0), ball(3, -50.0, 0.9), ball(4, -50.0, 0.9),
                ball(5, -50.6, 0.0), game(6, mode=M.GM_KICK_OFF, mode_side=LEFT), ball(6, -49.2, 0.3),
                obj(7, 11, x=-48.6, y=0.3, body=180.0), obj(7, 0, x=-50.0, y=0.3), ball(7, -49.3, 0.3),
                ball(8, 49.2, 0.3), obj(9, 0, x=-30.0, y=0.0), ball(9, -29.2, 0.0), obj(10, 11, x=30.0, y=0.0), ball(10, 29.2, 0.0),
                obj(11, 0, x=-45.0, y=25.0), ball(11, -44.2, 25.0), obj(12, 11, x=45.0, y=-25.0), ball(12, 44.2, -25.0),
                ball(13, -49.2, 0.3)]
_CATCH_ACTS = [(0, (0, 2, 3, 5, 6, 7, 9, 11, 13), 0, (CATCH, 0, 0)), (0, 1, 1, (CATCH, 0, 0)), (0, 4, 0, (CATCH, 120, 0)),
               (0, (7, 8, 10, 12), 11, (CATCH, 0, 0)), (1, 2, 0, (CATCH, 0, 0)),
               (1, 0, 0, (MOVE, -40, 10)), (2, 0, 0, (MOVE, -40, 10)), (2, 0, 1, (MOVE, -40, 10)), (3, 0, 0, (MOVE, -20, 30)),
               (4, 0, 0, (MOVE, -45, 0)), (5, 0, 0, (KICK, 60, 0)), (2, 8, 11, (MOVE, -40, -10)), (3, 8, 11, (KICK, 60, 0)),
               (1, 13, 21, (KICK, 100, 0)), (2, 13, 0, (KICK, 100, 0))]


def _catch_witness(tr):
    md = tr['mode']
    return (md[0, [0, 4, 7, 8, 13]] == M.GM_GOALIE_CATCH).all() and (md[0, [1, 2, 3, 5]] == M.GM_PLAY_ON).all() and md[0, 6] == M.GM_KICK_OFF \
        and (md[0, [9, 10, 11, 12]] == M.GM_CATCH_FAULT).all() and tr['catch_ban'][0, 2, 0] == 5 and tr['catch_ban'][1, 2, 0] == 4 \
        and tr['goalie_moves'][3, 0] == 0 and tr['x'][4, 0, 0] == -36.0 and md[5, 0] == M.GM_PLAY_ON and tr['x'][2, 8, 11] == 40.0 \
        and md[3, 8] == M.GM_PLAY_ON and tr['catch_ban'][0, 7, 11] == 5 and tr['last_touch_side'][0, 7] == LEFT


scene('catch_rectangle_ban_and_held_ball', {}, 14, 7, _CATCH_EDITS, _CATCH_ACTS, _catch_witness)
scene('catch_probability_back_pass_and_offside_switched_off',
      dict(catch_probability=0.5, back_passes=0, use_offside=0, free_kick_faults=0, stopped_clock=0, half_time_cycles=4, after_goal_wait=2,
           nr_extra_halfs=0, penalty_shoot_outs=0, auto_reset=0), 16, 12,
      [PLAY_ON, ball(range(12), -49.2, 0.3, vx=-1.0), game(range(12), last_kicker=3),
       ball((12, 13), 5.5, 0.0), obj((12, 13), 9, x=5.0, y=0.0, body=0.0), obj((12, 13), 10, x=35.0, y=0.0),
       ball(14, 52.0, 1.0, vx=1.5), game((14, 15), mode=M.GM_KICK_OFF, mode_side=LEFT)],
      [(0, range(12), 0, (CATCH, 0, 0)), (0, (12, 13), 9, (KICK, 20, 0)), (1, 12, 9, (DASH, 100, 0)), (2, 12, 9, (KICK, 50, 0)),
       (0, 15, 10, (KICK, 20, 0)), (1, 15, 10, (DASH, 100, 0)), (2, 15, 10, (KICK, 50, 0))],
      lambda tr: 0 < (tr['mode'][0, :12] == M.GM_GOALIE_CATCH).sum() < 12 and not tr.saw(M.GM_BACK_PASS) and (tr['offside_mask'] == 0).all()
      and not tr.saw(M.GM_FREE_KICK_FAULT) and tr['stats'][2, 4] > tr['stats'][1, 4] and (tr['stopped_cycle'] == 0)[:4].all()
      and tr.saw(M.GM_TIME_OVER))

# ---- the back pass: a team-mate's kick caught inside the area (both corners, both goalies); not an opponent's, not his own,
#      not outside the area; then the announcement and the indirect free kick
scene('back_pass', dict(announce_wait=3), 7, 6,
      [PLAY_ON, ball((0, 2, 3), -49.2, 0.3, vx=-1.0), ball(1, -49.2, -0.3, vx=-1.0), ball(4, 49.2, 0.3), ball(5, 49.2, -0.3),
       game((0, 1), last_kicker=3), game(2, last_kicker=14), game(3, last_kicker=1), game((4, 5), last_kicker=13),
       obj(6, 0, x=-30.0, y=0.0), ball(6, -29.2, 0.0), game(6, last_kicker=3)],
      [(0, (0, 1, 2, 3, 6), 0, (CATCH, 0, 0)), (0, (4, 5), 11, (CATCH, 0, 0)), (range(1, 6), None, 15, (DASH, 30, 0))],
      lambda tr: (tr['mode'][0, [0, 1, 4, 5]] == M.GM_BACK_PASS).all() and (tr['mode'][0, [2, 3]] == M.GM_GOALIE_CATCH).all()
      and tr['mode'][0, 6] == M.GM_CATCH_FAULT and tr['y'][0, 0, BALL] == np.float32(20.16) and tr['y'][0, 1, BALL] == np.float32(-20.16)
      and tr['x'][0, 4, BALL] == 36.0 and tr['mode'][3, 0] == M.GM_IND_FREE_KICK and tr['mode_side'][3, 4] == LEFT)

# ---- every announcement, for both sides: the dead ball, the offenders kept away, then the restart; FoulCharge_ inside the
#      offender's own penalty area -> PenaltyKick_ (each side; just outside in x and in y; the other area; another call there)
_ANN = (M.GM_OFF_SIDE, M.GM_BACK_PASS, M.GM_FREE_KICK_FAULT, M.GM_CATCH_FAULT, M.GM_FOUL_CHARGE, M.GM_ILLEGAL_DEFENSE, M.GM_FOUL_PUSH,
        M.GM_FOUL_MULTIPLE_ATTACKER, M.GM_FOUL_BALL_OUT)
_ANN_EDITS = [ball(None, 10.0, 5.0), obj(None, 14, x=10.5, y=5.0), obj(None, 9, x=9.0, y=5.0)]
for _k, _md in enumerate(_ANN):
    _ANN_EDITS += [game(2 * _k, mode=_md, mode_side=LEFT), game(2 * _k + 1, mode=_md, mode_side=RIGHT)]
_PK = [(LEFT, -45.0, 3.0), (RIGHT, 45.0, 3.0), (LEFT, -45.0, 25.0), (LEFT, 45.0, 3.0), (RIGHT, -45.0, 3.0), (LEFT, -36.0, 20.16),
       (RIGHT, 36.0, -20.16), (LEFT, -35.9, 3.0), (RIGHT, 35.9, 3.0)]
for _k, (_sd, _x, _y) in enumerate(_PK):
    _ANN_EDITS += [game(18 + _k, mode=M.GM_FOUL_CHARGE, mode_side=_sd), ball(18 + _k, _x, _y)]
_ANN_EDITS += [game(27, mode=M.GM_CATCH_FAULT, mode_side=LEFT), ball(27, -45.0, 3.0), obj(18, 2, x=-40.0, y=1.0), obj(19, 13, x=40.0, y=1.0)]
scene('announcements_and_penalty_kick', dict(announce_wait=2), 28, 5, _ANN_EDITS,
      [((0, 1), None, 14, (KICK, 100, 0)), ((0, 1), None, 9, (KICK, 100, 180)), (4, 19, 2, (DASH, 50, 0))],
      lambda tr: all(tr.saw(md, 2 * k, LEFT) and tr.saw(md, 2 * k + 1, RIGHT) for k, md in enumerate(_ANN))
      and (tr['mode'][1, [2, 3, 4, 5]] == M.GM_IND_FREE_KICK).all() and (tr['mode'][1, [0, 1, 6, 7, 8, 9]] == M.GM_FREE_KICK).all()
      and (tr['mode'][1, [18, 19, 23, 24]] == M.GM_PENALTY_KICK).all() and (tr['mode'][1, [20, 21, 22, 25, 26, 27]] == M.GM_FREE_KICK).all()
      and tr['x'][1, 18, BALL] == -41.5 and tr['x'][1, 19, BALL] == 41.5 and (tr['vx'][:, :, BALL] == 0).all())

# ---- the intentional foul: the victim's geometry on every side, two foulers, a victim already down, cards, sent-off players
_FOUL = [obj(None, 5, x=0.0, y=0.0, body=0.0), obj(None, 15, x=1.0, y=0.2, body=180.0), ball(None, 0.7, 0.1)]
FOUL_SCENE = [PLAY_ON] + _FOUL          # (tests/test_match_oracle.py builds its foul scenarios from it)
_FOUL_VAR = [card(1, 5, M.CARD_YELLOW), card(2, 15, M.CARD_RED), obj(3, 15, x=-0.5, y=0.5), ball(3, 0.3, 0.1),
             obj(4, 15, x=2.1, y=0.0), ball(4, 1.2, 0.0), obj(5, 15, x=0.5, y=1.4), ball(5, 0.6, 0.4), obj(6, 15, x=20.0, y=20.0),
             obj(7, 6, x=0.0, y=0.9, body=0.0), obj(8, 15, x=1.0, y=0.2, body=180.0, tackle_cycles=10),
             ball(9, 0.4, 0.1), game(11, mode=M.GM_KICK_IN, mode_side=LEFT),
             obj(12, 15, x=2.0, y=0.0), ball(12, 1.1, 0.0), obj(13, 15, x=0.5, y=1.25), ball(13, 0.6, 0.4), obj(14, 15, x=0.0, y=0.7), ball(14, 0.5, 0.0)]
scene('intentional_foul_geometry_and_cards', dict(foul_detect_probability=1.0, announce_wait=2, half_time_cycles=8, nr_extra_halfs=0,
                                                  penalty_shoot_outs=0, auto_reset=0), 15, 14,
      [PLAY_ON] + _FOUL + _FOUL_VAR,
      [(0, (0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 13, 14), 5, (TACKLE, 0, 1)), (0, 7, 6, (TACKLE, 0, 1)), (0, 9, 15, (TACKLE, 0, 1)),
       (0, 10, 5, (TACKLE, 0, 0)), (range(1, 14), 1, 5, (DASH, 100, 0)), (range(1, 14), 2, 15, (DASH, 100, 0))],
      lambda tr: tr['mode'][0, 0] == M.GM_FOUL_CHARGE and tr['card'][0, 0, 5] == M.CARD_YELLOW and tr['card'][0, 1, 5] == M.CARD_RED
      and tr['tackle_cycles'][0, 0, 15] == 5 and tr['y'][0, 1, 5] == np.float32(-47.5) and tr['y'][-1, 1, 5] == np.float32(-47.5)
      and (tr['mode'][0, [2, 3, 4, 5, 6, 10]] == M.GM_PLAY_ON).all() and tr['card'][0, 7, 5] == 1 and tr['card'][0, 7, 6] == 0
      and tr['tackle_cycles'][0, 8, 15] == 9 and tr.saw(M.GM_FOUL_CHARGE, 9, RIGHT) and tr['mode'][0, 11] == M.GM_PLAY_ON and tr['card'][0, 11, 5] == 0
      and (tr['mode'][0, [12, 13, 14]] == M.GM_FOUL_CHARGE).all() and tr.saw(M.GM_FIRST_HALF_OVER, 1))
scene('intentional_foul_seen_or_not', {}, 12, 2, [PLAY_ON] + _FOUL, [(0, None, 5, (TACKLE, 0, 1))],
      lambda tr: 0 < (tr['mode'][0] == M.GM_FOUL_CHARGE).sum() < 12 and ((tr['card'][0, :, 5] == 1) == (tr['mode'][0] == M.GM_FOUL_CHARGE)).all()
      and (tr['tackle_cycles'][0, :, 15] == 5).sum() > (tr['mode'][0] == M.GM_FOUL_CHARGE).sum())

# ---- goals on both sides, the kick-off that follows at once (after_goal_wait = 0), a sent-off kick-off taker, no goal directly
#      from an indirect free kick, the posts and the goal line themselves
_GOAL = [PLAY_ON, ball((0, 2), 52.0, 1.0, vx=1.5), ball((1, 3), -52.0, -6.9, vx=-1.5), card(2, 21, M.CARD_RED), card(3, 10, M.CARD_RED),
         ball(4, 52.0, 1.0, vx=1.5), game(4, set_play_taker=10 | 0x100), ball(5, -52.0, 1.0, vx=-1.5), game(5, set_play_taker=12 | 0x100, last_touch_side=RIGHT), game((4, 8), last_touch_side=LEFT),
         game(9, last_touch_side=RIGHT),
         ball(6, 51.5, 1.0, vx=1.0), ball(7, -51.5, 1.0, vx=-1.0), ball(8, 52.0, 7.01, vx=1.5), ball(9, -52.0, -7.01, vx=-1.5)]
scene('goals_and_kick_off_at_once', dict(after_goal_wait=0), 10, 3, _GOAL, [(None, 2, 21, (DASH, 100, 0)), (None, 3, 10, (KICK, 100, 0))],
      lambda tr: (tr['score_left'][0, [0, 2]] == 1).all() and (tr['score_right'][0, [1, 3]] == 1).all() and tr['mode'][0, 0] == M.GM_KICK_OFF
      and tr['mode_side'][0, 0] == RIGHT and tr['x'][0, 0, 21] == np.float32(0.4) and tr['x'][0, 2, 21] == 0.0 and tr['x'][0, 3, 10] == 0.0
      and tr['x'][0, 1, 10] == np.float32(-0.4) and (tr['mode'][0, [4, 5, 8, 9]] == M.GM_GOAL_KICK).all() and (tr['score_left'][0, 4:] == 0).all()
      and (tr['mode'][0, [6, 7]] == M.GM_PLAY_ON).all() and tr.event(MO.EV_GOAL, 0) and not tr.event(MO.EV_GOAL, 4))
scene('after_goal_wait', dict(after_goal_wait=3), 2, 6,
      [PLAY_ON, ball(0, 52.0, 1.0, vx=1.5), ball(1, -52.0, 1.0, vx=-1.5), obj(0, 9, x=52.9, y=1.0, body=0.0)],
      [(range(1, 4), 0, 9, (KICK, 100, 0)), (range(1, 4), None, 15, (MOVE, -20, 5)), (range(1, 4), None, 3, (MOVE, -20, 5))],
      lambda tr: (tr['mode'][:3] == M.GM_AFTER_GOAL).all() and (tr['mode'][3] == M.GM_KICK_OFF).all() and tr['mode_side'][3, 0] == RIGHT
      and tr['x'][1, 0, 15] == 20.0 and tr['x'][1, 0, BALL] == np.float32(53.5) and tr['stats'][-1, 4] == 0)

# ---- ball out: both side lines and both goal lines, by the last touch (left, right, nobody), both signs of y; the lines themselves
_OUT = [(10.0, 33.5, 0.0, 1.0, LEFT), (10.0, -33.5, 0.0, -1.0, RIGHT), (-10.0, 33.5, 0.0, 1.0, 0), (52.0, 20.0, 1.0, 0.0, RIGHT),
        (52.0, -20.0, 1.0, 0.0, LEFT), (-52.0, 20.0, -1.0, 0.0, LEFT), (-52.0, -20.0, -1.0, 0.0, RIGHT), (52.0, 20.0, 1.0, 0.0, 0),
        (10.0, 33.0, 0.0, 1.0, LEFT), (51.5, 20.0, 1.0, 0.0, LEFT), (52.0, 33.5, 1.0, 1.0, RIGHT), (-52.0, 0.0, -1.0, 0.0, 0)]
scene('ball_out_restarts', {}, len(_OUT), 3,
      [PLAY_ON] + [ball(e, x, y, vx, vy) for e, (x, y, vx, vy, _s) in enumerate(_OUT)] +
      [game(e, last_touch_side=s) for e, (_x, _y, _vx, _vy, s) in enumerate(_OUT)] + [obj(0, 3, x=10.0, y=30.0), obj(0, 15, x=12.0, y=30.0)], [],
      lambda tr: list(tr['mode'][0]) == [M.GM_KICK_IN] * 3 + [M.GM_CORNER_KICK, M.GM_GOAL_KICK, M.GM_CORNER_KICK, M.GM_GOAL_KICK, M.GM_GOAL_KICK,
                                         M.GM_PLAY_ON, M.GM_PLAY_ON, M.GM_CORNER_KICK, M.GM_AFTER_GOAL]
      and list(tr['mode_side'][0, :8]) == [RIGHT, LEFT, RIGHT, LEFT, RIGHT, RIGHT, LEFT, RIGHT] and tr['stats'][0, 7] == 9
      and abs(float(np.hypot(tr['x'][1, 0, 3] - 10.0, tr['y'][1, 0, 3] - 34.0)) - 9.15) < 1e-4 and tr['y'][1, 0, 15] == 30.0)

# ---- the kick that puts a set play into play: which set plays are exempt from offside, the indirect mark, the drop ball
_SETPLAYS = (M.GM_KICK_IN, M.GM_GOAL_KICK, M.GM_CORNER_KICK, M.GM_FREE_KICK, M.GM_IND_FREE_KICK, M.GM_KICK_OFF, M.GM_PENALTY_KICK)
scene('set_play_kicks_and_offside_exemptions', dict(drop_ball_time=3), 2 * len(_SETPLAYS), 6,
      [ball(None, 5.5, 0.0), obj(None, 9, x=5.0, y=0.0, body=0.0), obj(None, 10, x=40.0, y=0.0), obj(None, 20, x=6.0, y=0.0, body=180.0)] +
      [game((k, k + len(_SETPLAYS)), mode=md, mode_side=LEFT) for k, md in enumerate(_SETPLAYS)],
      [(0, range(len(_SETPLAYS)), 9, (KICK, 40, 90)), (0, None, 20, (KICK, 100, 0))],
      lambda tr: (tr['mode'][0, :7] == M.GM_PLAY_ON).all() and list(tr['offside_mask'][0, :7]) == [0, 0, 0, 1 << 10, 1 << 10, 1 << 10, 1 << 10]
      and tr['set_play_taker'][0, 4] == (10 | 0x100) and tr['set_play_taker'][0, 3] == 10 and (tr['mode'][2, 7:] != M.GM_PLAY_ON).all()
      and (tr['mode'][3, 7:] == M.GM_PLAY_ON).all() and (tr['vx'][:, 7:, BALL] == 0).all())

# ---- offside: the line (second-last defender, the ball, the halfway line), both teams, the flag cleared by the other side's
#      collision touch and kept by the own side's, the flagged player near the ball
_DEF = [obj(None, i, x=30.0 - (i - 11), y=-30.0 + 2 * (i - 11)) for i in range(11, 22)]


def _offside_edits():
    left = [obj(0, 9, x=5.0, y=0.0, body=0.0), ball(0, 5.5, 0.0), obj(0, 10, x=35.0, y=0.0), obj(0, 8, x=3.0, y=12.0)]
    back = [obj(0, 9, x=5.0, y=0.0, body=0.0), ball(0, 4.5, 0.0), obj(0, 10, x=35.0, y=0.0), obj(0, 8, x=3.0, y=0.0)]
    near = [obj(0, i, x=-5.0 - (i - 11), y=-30.0 + 2 * (i - 11)) for i in range(12, 22)] + \
           [obj(0, 9, x=5.0, y=0.0, body=0.0), ball(0, 5.5, 0.0), obj(0, 10, x=30.0, y=20.0), obj(0, 8, x=7.5, y=0.5), obj(0, 7, x=5.2, y=-20.0)]
    asc = [obj(0, i, x=20.0 + (i - 11), y=-30.0 + 2 * (i - 11)) for i in range(11, 22)]
    e = []
    e += at_env(0, left) + [obj(0, 20, x=7.0, y=0.0)]                       # the other side's collision touch clears the flag
    e += at_env(1, back)                                                  # a team-mate's does not
    e += at_env(2, mirrored(_DEF + left)) + [obj(2, 9, x=-7.0, y=0.0)]
    e += at_env(3, mirrored(_DEF + back))
    e += at_env(4, near)                                                  # the line is the ball; a flagged player near it is called
    e += at_env(5, mirrored(_DEF + near))
    e += at_env(6, asc + left)                                            # defenders in ascending order of x
    e += at_env(7, left) + [obj(7, 10, x=29.0, y=0.0)]                     # level with the second-last defender: onside
    return e


scene('offside_line_flag_and_call', {}, 8, 5, [PLAY_ON] + _DEF + _offside_edits(),
      [(0, (0, 4, 6, 7), 9, (KICK, 30, 0)), (0, 1, 9, (KICK, 30, 180)), (0, (2, 5), 20, (KICK, 30, 0)), (0, 3, 20, (KICK, 30, 180))],
      lambda tr: tr['offside_mask'][0, 0] == 1 << 10 and tr['offside_mask'][-1, 0] == 0 and (tr['mode'][:, 0] == M.GM_PLAY_ON).all()
      and (tr['offside_mask'][:, 1] == 1 << 10).all() and tr.event(MO.EV_BALL_COLLIDE, 1) and tr['offside_mask'][0, 2] == 1 << 21
      and tr['offside_mask'][-1, 2] == 0 and (tr['offside_mask'][:, 3] == 1 << 21).all() and tr.event(MO.EV_BALL_COLLIDE, 3)
      and tr['mode'][0, 4] == M.GM_OFF_SIDE and tr['mode_side'][0, 4] == LEFT and tr['x'][0, 4, BALL] == 7.5
      and tr['mode'][0, 5] == M.GM_OFF_SIDE and tr['mode_side'][0, 5] == RIGHT and tr['offside_mask'][0, 6] == 1 << 10
      and tr['offside_mask'][0, 7] == 0 and tr['stats'][-1, 6] == 2)

# ---- the free-kick fault: the taker's second touch; not after a team-mate's kick, a kick in the same cycle or a collision touch
scene('free_kick_fault', {}, 5, 4,
      [obj(1, 9, x=1.2, y=0.3, body=0.0), obj(2, 9, x=0.2, y=0.5, body=0.0), obj(3, 8, x=1.3, y=0.0)],
      [(0, None, 10, (KICK, 20, 0)), (1, None, 10, (DASH, 100, 0)), (2, None, 10, (KICK, 50, 0)), (1, 1, 9, (KICK, 10, 0)),
       (0, 2, 9, (KICK, 10, 0)), (1, 4, 10, (DASH, 0, 0)), (1, 4, 10, (KICK, 50, 0))],
      lambda tr: tr['mode'][2, 0] == M.GM_FREE_KICK_FAULT and tr['mode_side'][2, 0] == LEFT and tr['set_play_taker'][0, 0] == 11
      and tr['set_play_taker'][1, 1] == 0 and tr['mode'][2, 1] == M.GM_PLAY_ON and tr['mode'][2, 2] == M.GM_PLAY_ON
      and tr['set_play_taker'][0, 2] == 11 and tr.event(MO.EV_BALL_COLLIDE, 3) and tr['mode'][2, 3] == M.GM_PLAY_ON)

# ---- collisions: two players, two on one spot, the ball on a player, a crowd that ten passes do not untangle, the ball touched
#      in a set play by either side, the last kicker's own touch
scene('collisions', {}, 7, 3,
      [PLAY_ON, obj(0, 1, x=0.0, y=20.0), obj(0, 12, x=0.4, y=20.0), obj(1, 1, x=0.0, y=20.0), obj(1, 12, x=0.0, y=20.0),
       ball(2, 5.0, 5.0, vx=0.5), obj(2, 15, x=5.5, y=5.0)] +
      [obj(3, i, x=10.0 + 0.1 * (i % 5), y=10.0 + 0.1 * (i // 5)) for i in range(22)] + [ball(3, 10.2, 10.2)] +
      [game((4, 5), mode=M.GM_KICK_IN, mode_side=LEFT), ball((4, 5), 10.0, 34.0), obj(4, 15, x=10.2, y=33.9), obj(5, 3, x=10.2, y=33.9),
       game(4, last_touch_side=0, set_play_taker=4), game(5, last_touch_side=0), ball(6, 5.0, 5.0), obj(6, 9, x=5.2, y=5.0),
       game(6, last_kicker=10, set_play_taker=10)],
      [],
      lambda tr: abs(float(tr['x'][0, 0, 12] - tr['x'][0, 0, 1]) - 0.6) < 1e-5 and tr['x'][0, 1, 1] < 0 < tr['x'][0, 1, 12]
      and tr['last_touch_side'][0, 2] == RIGHT and tr.event(MO.EV_COLLIDE, 3) and tr.event(MO.EV_BALL_COLLIDE, 3)
      and tr['last_touch_side'][0, 4] == 0 and tr['last_touch_side'][0, 5] == LEFT and tr['last_kicker'][0, 6] == 10
      and tr['set_play_taker'][0, 6] == 10 and tr['set_play_taker'][0, 4] == 4)

# ---- the modes that hold a match
scene('pause_human_time_over_hold', dict(auto_reset=0), 3, 3,
      [game(0, mode=M.GM_PAUSE), game(1, mode=M.GM_HUMAN), game(2, mode=M.GM_TIME_OVER, mode_side=0)],
      [(None, None, 3, (DASH, 100, 0)), (None, None, 10, (KICK, 100, 0))],
      lambda tr: (tr['cycle'] == 0).all() and (tr['stopped_cycle'][-1] == 3).all() and (tr['x'][-1, :, 3] == -35.0).all()
      and (tr['setplay_timer'] == 0).all() and list(tr['mode'][-1]) == [M.GM_PAUSE, M.GM_HUMAN, M.GM_TIME_OVER])

# ---- the shoot-out's sequence from PenaltyOnfield_: setup, ready, taken, the verdict, the other side's kick; a kick not taken, a
#      sent-off taker, a second touch (allowed), nobody else acts
_PEN = dict(half_time_cycles=3, nr_normal_halfs=1, nr_extra_halfs=0, auto_reset=0, pen_before_setup_wait=2, pen_ready_wait=3,
            pen_taken_wait=5, pen_nr_kicks=1, pen_max_extra_kicks=1)
_PEN_START = [game(None, mode=M.GM_PENALTY_ONFIELD, mode_side=RIGHT, cycle=3)]
scene('penalty_setup_ready_taken', _PEN, 4, 24, _PEN_START + [card(2, 10, M.CARD_RED)],
      [(3, 0, 10, (KICK, 30, 0)), (3, 3, 10, (KICK, 10, 0)), (4, 3, 10, (KICK, 30, 0)), (None, None, 3, (DASH, 100, 0)),
       (range(0, 4), None, 11, (DASH, 100, 0)), (range(0, 3), None, 10, (DASH, 100, 0)), (range(12, 24), None, 21, (KICK, 30, 0))],
      lambda tr: list(tr['mode'][1]) == [M.GM_PENALTY_SETUP] * 4 and list(tr['mode'][2]) == [M.GM_PENALTY_READY] * 4
      and list(tr['mode'][3]) == [M.GM_PENALTY_TAKEN, M.GM_PENALTY_READY, M.GM_PENALTY_READY, M.GM_PENALTY_TAKEN]
      and tr['mode'][5, 1] == M.GM_PENALTY_MISS and tr['mode'][5, 2] == M.GM_PENALTY_MISS and tr['mode'][9, 0] == M.GM_PENALTY_MISS
      and tr['stats'][4, 4] == 3 and (tr['vx'][:, :, 3] == 0).all() and (tr['vx'][:4, :, 11] == 0).all() and tr.saw(M.GM_PENALTY_SETUP, 0, RIGHT)
      and tr.saw(M.GM_PENALTY_TAKEN, 0, RIGHT) and tr['y'][-1, 2, 10] == np.float32(-55.0) and (tr['cycle'] == 3).all())

# ---- the verdicts of a kick that is under way: scored by either team, beside the goal, over the side line, behind the other goal line,
#      caught, out of time, played by the goalie, played again by the taker
_TAKEN = [game(None, mode=M.GM_PENALTY_TAKEN, mode_side=LEFT, cycle=3, set_play_taker=pen_word(10)), obj(None, 10, x=9.3, y=0.0, body=0.0),
          obj(None, 11, x=51.5, y=0.0, body=180.0), ball(0, 52.0, 1.0, vx=1.5), ball(1, 52.0, 20.0, vx=1.5), ball(2, 30.0, 33.9, vy=1.0),
          game(3, mode_side=RIGHT, set_play_taker=pen_word(21, (1, 0))), obj(3, 0, x=51.5, y=0.0, body=180.0), obj(3, 11, x=3.0, y=0.0),
          obj(3, 21, x=9.3, y=0.0, body=0.0), ball(3, 52.0, -1.0, vx=1.5), ball((4, 6), 50.9, 0.0), ball(5, 20.0, 0.0), game(5, setplay_timer=5),
          ball(7, 10.0, 0.0), ball(8, -52.0, 0.0, vx=-1.5), ball(9, 20.0, 0.0), game(9, setplay_timer=4)]
scene('penalty_taken_verdicts', _PEN, 10, 2, _TAKEN,
      [(0, 4, 11, (CATCH, 0, 0)), (0, 6, 11, (KICK, 100, 0)), (0, 7, 10, (KICK, 50, 0)), (0, None, 3, (DASH, 100, 0)), (0, 0, 5, (KICK, 100, 0)),
       (0, 3, 11, (CATCH, 0, 0))],
      lambda tr: list(tr['mode'][0]) == [M.GM_PENALTY_SCORE, M.GM_PENALTY_MISS, M.GM_PENALTY_MISS, M.GM_PENALTY_SCORE, M.GM_PENALTY_MISS,
                                         M.GM_PENALTY_MISS, M.GM_PENALTY_TAKEN, M.GM_PENALTY_TAKEN, M.GM_PENALTY_MISS, M.GM_PENALTY_TAKEN]
      and tr['reward_left'][0, 0] == 1.0 and tr['reward_left'][0, 3] == -1.0 and tr['set_play_taker'][0, 3] == pen_word(21, (1, 1), (0, 1))
      and tr['set_play_taker'][0, 0] == pen_word(10, (1, 0), (1, 0)) and tr.event(MO.EV_CATCH, 4) and not tr.event(MO.EV_CATCH, 3)
      and tr['vx'][0, 6, BALL] < 0 and tr['vx'][0, 7, BALL] > 0 and (tr['score_left'] == 0).all() and (tr['vx'][0, :, 3] == 0).all())

# ---- PenaltyFoul_ (pen_allow_mult_kicks = 0) and the coin of pen_random_winner (tossed only for a level shoot-out)
scene('penalty_foul_and_random_winner', dict(_PEN, pen_allow_mult_kicks=0, pen_random_winner=1, pen_max_extra_kicks=0, pen_taken_wait=4,
                                             pen_before_setup_wait=1, pen_ready_wait=2), 11, 16,
      _PEN_START + [game(10, mode=M.GM_PENALTY_SCORE, mode_side=RIGHT, set_play_taker=pen_word(21, (1, 1), (1, 0)))],
      [(2, 0, 10, (KICK, 10, 0)), (3, 0, 10, (KICK, 100, 0)), (2, 1, 10, (KICK, 10, 0))],
      lambda tr: tr.saw(M.GM_PENALTY_FOUL, 0, LEFT) and not tr.saw(M.GM_PENALTY_FOUL, 1) and (tr['mode'][-1] == M.GM_TIME_OVER).all()
      and {1, 2} == set(int(w) >> 28 for w in tr['set_play_taker'][-1, :10]) and int(tr['set_play_taker'][-1, 10]) >> 28 == 0)

# ---- when the shoot-out is over: every count of kicks and goals around each comparison, written into the verdict's word
_OVER = [((1, 0), (1, 0), LEFT, 0), ((2, 1), (2, 0), LEFT, 1), ((1, 1), (0, 1), RIGHT, 0), ((2, 1), (0, 1), LEFT, 1), ((2, 2), (1, 1), RIGHT, 0),
         ((2, 2), (2, 1), RIGHT, 1), ((3, 2), (1, 1), LEFT, 0), ((3, 3), (1, 1), RIGHT, 0), ((3, 3), (2, 1), RIGHT, 1), ((4, 4), (1, 1), RIGHT, 1),
         ((2, 3), (1, 1), RIGHT, 0), ((1, 0), (0, 0), LEFT, 0), ((2, 2), (1, 2), RIGHT, 1), ((12, 11), (0, 0), LEFT, 0), ((4, 4), (1, 2), RIGHT, 1)]
scene('penalty_shoot_out_is_over', dict(_PEN, pen_nr_kicks=2, pen_max_extra_kicks=2, pen_before_setup_wait=1, auto_reset=1), len(_OVER), 3,
      [game(e, mode=M.GM_PENALTY_MISS if e % 2 else M.GM_PENALTY_SCORE, mode_side=sd, cycle=3,
            set_play_taker=pen_word(10 if sd == LEFT else 21, k, g)) for e, (k, g, sd, _o) in enumerate(_OVER)], [],
      lambda tr: [int(d) for d in tr['done'][0]] == [o for _k, _g, _s, o in _OVER]
      and all(tr['mode'][0, e] == (M.GM_KICK_OFF if o else M.GM_PENALTY_SETUP) for e, (_k, _g, _s, o) in enumerate(_OVER))
      and tr['mode_side'][0, 0] == RIGHT and (tr['set_play_taker'][0, 0] & 0xff) == 22 and (tr['set_play_taker'][0, 2] & 0xff) == 10
      and (tr['set_play_taker'][0, 13] & 0xff) == 22)
scene('penalty_shoot_out_without_extra_kicks', dict(_PEN, pen_nr_kicks=2, pen_max_extra_kicks=0, pen_before_setup_wait=1), 2, 2,
      [game(0, mode=M.GM_PENALTY_MISS, mode_side=RIGHT, cycle=3, set_play_taker=pen_word(21, (2, 2), (1, 1))),
       game(1, mode=M.GM_PENALTY_MISS, mode_side=RIGHT, cycle=3, set_play_taker=pen_word(21, (1, 1), (1, 1)))], [],
      lambda tr: list(tr['mode'][0]) == [M.GM_TIME_OVER, M.GM_PENALTY_SETUP])

# ---- IllegalDefense_: both teams, one defender too few, the own side's touch, beside and in front of the strip, a sent-off
#      defender, counters at their ceiling
def _illegal_edits():
    base = [obj(0, i, x=(-20.0 if i < 11 else 20.0) - (i % 11), y=-25.0 + 2.0 * (i % 11), vx=0.0, vy=0.0) for i in range(22)]
    pack = [obj(0, i, x=-45.0 - k, y=-6.0 + 4.0 * k) for k, i in enumerate((1, 2, 3, 4))]
    e = []
    for env in range(11):
        e += at_env(env, base + [ball(0, 0.0, 30.0)])
    e += at_env(0, pack) + [game(0, last_touch_side=RIGHT)]
    e += at_env(1, mirrored(pack)) + [game(1, last_touch_side=LEFT)]
    e += at_env(2, pack[:3]) + [game(2, last_touch_side=RIGHT)]
    e += at_env(3, pack) + [game(3, last_touch_side=LEFT)]
    e += at_env(4, pack[:3]) + [obj(4, 4, x=-45.0, y=20.16), game(4, last_touch_side=RIGHT)]
    e += at_env(5, pack[:3]) + [obj(5, 4, x=-36.0, y=0.0), game(5, last_touch_side=RIGHT)]
    e += at_env(6, pack) + [card(6, 4, M.CARD_RED), game(6, last_touch_side=RIGHT)]
    e += at_env(7, pack) + [game(7, last_touch_side=RIGHT, setplay_timer=255)]
    e += at_env(8, mirrored(pack)) + [game(8, last_touch_side=LEFT, setplay_timer=255 << 8)]
    e += at_env(9, mirrored(pack[:3])) + [obj(9, 15, x=36.0, y=0.0), game(9, last_touch_side=LEFT)]
    e += at_env(10, pack) + [game(10, last_touch_side=RIGHT), ball(10, 0.0, 33.5, vy=1.0)]
    return e


ILLEGAL_DEFENSE_SCENE = [PLAY_ON] + [ed for ed in _illegal_edits() if ed[1] == 0]     # (tests/test_match_oracle.py starts from it)
scene('illegal_defense', dict(illegal_defense_number=4, illegal_defense_duration=255, announce_wait=2, auto_reset=0), 11, 4,
      [PLAY_ON] + _illegal_edits(), [],
      lambda tr: list(tr['setplay_timer'][1, :7]) == [2, 2 << 8, 0, 0, 0, 0, 0] and tr['mode'][0, 7] == M.GM_ILLEGAL_DEFENSE
      and tr['mode_side'][0, 7] == LEFT and tr['x'][0, 7, BALL] == -41.5 and tr['mode'][0, 8] == M.GM_ILLEGAL_DEFENSE
      and tr['mode_side'][0, 8] == RIGHT and tr['x'][0, 8, BALL] == 41.5 and tr['mode'][2, 7] == M.GM_FREE_KICK and tr['setplay_timer'][1, 9] == 0
      and tr['mode'][0, 10] == M.GM_KICK_IN and tr['setplay_timer'][0, 10] == 0)
scene('illegal_defense_called_after_duration', dict(illegal_defense_number=4, illegal_defense_duration=3, auto_reset=0), 2, 4,
      [PLAY_ON] + [ed for ed in _illegal_edits() if ed[1] in (0, 1)], [],
      lambda tr: list(tr['setplay_timer'][1]) == [2, 2 << 8] and list(tr['mode'][2]) == [M.GM_ILLEGAL_DEFENSE] * 2
      and list(tr['mode_side'][2]) == [LEFT, RIGHT])

# ---- the clock: the end of the normal time decided or drawn, the extra halves and their half time, a goal in extra time with and
#      without golden_goal, the last period ending decided / drawn / with and without the shoot-out, clocks beyond the end
_CLOCK = dict(half_time_cycles=4, extra_half_cycles=3, auto_reset=0, after_goal_wait=2, pen_before_setup_wait=1)
_CLOCK_EDITS = [PLAY_ON, game(0, cycle=7), game(1, cycle=7, score_left=1), game(2, cycle=10), game(3, cycle=13), game(4, cycle=13, score_right=2),
                game(5, cycle=9), ball(5, 52.0, 0.0, vx=2.0), game(6, cycle=5), ball(6, 52.0, 0.0, vx=2.0), game(7, cycle=40), game(8, cycle=3),
                game(9, cycle=11)]
for _gg in (0, 1):
    scene('clock_periods' + ('_golden_goal' if _gg else ''), dict(_CLOCK, golden_goal=_gg), 10, 4, _CLOCK_EDITS, [],
          lambda tr: list(tr['mode'][0, :5]) == [M.GM_EXTEND_HALF, M.GM_TIME_OVER, M.GM_FIRST_HALF_OVER, M.GM_PENALTY_ONFIELD, M.GM_TIME_OVER]
          and tr['mode_side'][0, 0] == LEFT and tr['mode_side'][0, 2] == RIGHT and tr['mode'][0, 5] == (M.GM_TIME_OVER if tr.scene.cfg['golden_goal'] else M.GM_AFTER_GOAL)
          and tr['mode'][0, 6] == M.GM_AFTER_GOAL and tr['mode'][0, 7] == M.GM_TIME_OVER and tr['mode'][0, 8] == M.GM_FIRST_HALF_OVER
          and tr['mode_side'][0, 8] == RIGHT and tr['mode'][0, 9] == M.GM_PLAY_ON and tr['mode'][1, 0] == M.GM_KICK_OFF)
scene('clock_last_period_without_shoot_out', dict(_CLOCK, penalty_shoot_outs=0, nr_extra_halfs=0, golden_goal=1, auto_reset=1), 3, 2,
      [PLAY_ON, game(0, cycle=7), game(1, cycle=7, score_right=1), game(2, cycle=30)], [],
      lambda tr: tr['done'][0].all() and (tr['mode'][0] == M.GM_KICK_OFF).all() and (tr['cycle'][0] == 0).all() and (tr['tick'][0] == 1).all())
scene('clock_shoot_out_after_the_normal_time', dict(_CLOCK, nr_extra_halfs=0), 2, 3, [PLAY_ON, game(0, cycle=7), game(1, cycle=7, score_right=1)], [],
      lambda tr: list(tr['mode'][0]) == [M.GM_PENALTY_ONFIELD, M.GM_TIME_OVER] and tr['mode'][1, 0] == M.GM_PENALTY_SETUP)


# ================================================================== the allow-list of the coverage test
# (a line of oracle/s2d_match_oracle.c by its source text, why no state of a validated configuration takes the directions of that line
#  that the table misses).  The text is matched, not a line number, so that an edit elsewhere in the file does not move an entry.
#  A condition, not a measurement: at most 3 % of the path's branch directions, no whole rule, and no entry for dead code (that is
#  deleted from the oracle instead).
ALLOW = [
    ('if (id < 0 || id >= S2D_MATCH_PLAYER_TYPES) id = 0;',
     's2d_match_validate_config refuses a player_type_id outside [0, 18): the clamp only guards the table read of a configuration nobody validated.'),
    ('static uint64_t env_gid(const S2DMOEngine *h, int64_t e)',
     'per-env Philox ids exist only behind the accessor s2dmo_set_env_ids (the engine has none): no scene sets them.'),
    ('API void s2dmo_destroy(S2DMOEngine *h)', 'the NULL guard of the destructor: an argument guard like that of s2dmo_create.'),
    ('if (d > R(0.0)) { ux = dx / d; uy = dy / d; } else { ux = side_of(i) == SIDE_LEFT ? R(-1.0) : R(1.0); uy = R(0.0); }',
     'a kept-away player exactly on the ball: the collision passes that run before have pushed every player off the ball, so d = 0 needs '
     'an exact rounding coincidence; the arm only keeps the division defined.'),
    ('if (p->half_time_cycles > 0 && m->cycle % p->half_time_cycles == 0)',
     's2d_match_validate_config refuses half_time_cycles < 1: the first operand only keeps the modulo defined.'),
]
