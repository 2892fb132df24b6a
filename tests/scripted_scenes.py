"""Constructed one-match states for the scripted team (include/s2d_match.h, rules 1-8), each with the (command, rule) every slot must
get, written by hand.  TEST INFRASTRUCTURE (tests/test_match_scripted_scenes_host.py, tests/test_gpu_match_scripted_scenes.py), in
the style of tests/belief_scenes.py and the edge scenes of tests/obs_f64.py.

A scene starts from a quiet base: everybody stands on his guard point (goalies) or home position for the scene's ball and looks at
the ball, PlayOn, nobody touched the ball.  In that base a goalie gets (NONE, rule 6), a field player (NONE, rule 7), each team's
chaser (DASH, rule 5); a scene then moves somebody or changes a word, and says what that changes.  Distances that are computed are
kept probe-safe (a factor 0.999 / 1.001 or 0.99 / 1.01 around the bound); quantities the rule copies (ball x, ball y) use fp32
neighbours, and those rows may be ill-conditioned under the float64 rule's probes.

Every scene is built for the left team and, through match_symmetry.swap_x, for the right team (the expected rows move with their
slots).  The shoot-out scenes are the exception: they play on the right goal by design, so they name their slots themselves.
scene_config(hetero=True) types the two teams alike (slot i and i + 11 share a type), so that swap_x of the configuration is the
configuration.
"""
import numpy as np

import match_oracle as MO
import match_symmetry as SY
import scripted_f64 as F
import scripted_policy as SP
from soccer2d_amd import _capi_match as M

NONE, DASH, TURN, KICK, CATCH = M.MCMD_NONE, M.MCMD_DASH, M.MCMD_TURN, M.MCMD_KICK, M.MCMD_CATCH
LEFT, RIGHT = 1, 2
SCENE_IDS = [16] + list(range(1, 11)) + [16] + list(range(1, 11))
# the header's list for rule 1: halted (TimeOver, Pause, Human), announcements, AfterGoal_, BeforeKickOff, FirstHalfOver, ExtendHalf,
# GoalieCatch_, and the shoot-out's modes other than PenaltyReady_ (23) / PenaltyTaken_ (24), by GameModeType number
QUIET_MODES = (1, 12, 13, 9, 18, 19, 20, 14, 27, 15, 16, 17, 8, 0, 11, 31, 30, 22, 25, 26, 28, 29)
SET_PLAYS = (3, 4, 5, 6, 7, 10, 21)      # KickOff_, KickIn_, FreeKick_, CornerKick_, GoalKick_, PenaltyKick_, IndFreeKick_


def scene_config(hetero=False, **kw):
    if not hetero:
        return MO.make_match_config(**kw)
    return MO.make_match_config(**dict(dict(player_types=F.HETERO_TYPES, player_type_id=SCENE_IDS), **kw))


def _zero_state():
    s = {}
    for name, _ct, dt, trail in M.MATCH_BUFFER_FIELDS:
        if trail is not None:
            s[name] = np.zeros((1,) + tuple(trail), dtype=dt)
    return s


def on_the_bound(T):
    """(dx, dx_out, dy) fp32: a point whose squared distance, in fp32 as the engine computes it (fmaf(dx, dx, dy * dy)) and exactly, is
    on the bound T (fp32 == T, exact <= T), and its fp32 neighbour outside in both"""
    f32, T64 = np.float32, float(T)
    for dy in (0.0, 0.25, 0.5, 0.75, 0.125, 0.375, 0.625, 0.875):
        x = f32(np.sqrt(max(T64 - dy * dy, 0.0)))
        for _ in range(8):
            x = np.nextafter(x, f32(0))
        for _ in range(17):
            xo, y = np.nextafter(x, f32(np.inf)), f32(dy)
            sq32 = lambda a: f32(np.float64(a) * np.float64(a) + np.float64(f32(y * y)))       # noqa: E731
            sq64 = lambda a: float(a) ** 2 + float(y) ** 2                                     # noqa: E731
            if sq32(x) == T and sq64(x) <= T64 and sq32(xo) > T and sq64(xo) > T64:
                return float(x), float(xo), float(dy)
            x = xo
    raise AssertionError('no point exactly on the bound on which fp32 and float64 agree')


class Scene:
    def __init__(self, name, prm, ball=(0.0, -3.0), mode=M.GM_PLAY_ON, swap=True, **words):
        self.name, self.prm, self.swap = name, prm, swap
        self.s = _zero_state()
        self.s['mode'][:] = mode
        for k, v in words.items():
            self.s[k][:] = v
        self.s['x'][0, 22], self.s['y'][0, 22] = ball
        self.want, self.ang = {}, {}
        hx, hy = F.home_points(self.s['x'][:, 22], self.s['y'][:, 22], prm)
        for l in range(22):
            self.put(l, hx[0, l], hy[0, l])

    @property
    def ball(self):
        return float(self.s['x'][0, 22]), float(self.s['y'][0, 22])

    def home(self, l):
        hx, hy = F.home_points(self.s['x'][:, 22], self.s['y'][:, 22], self.prm)
        return float(hx[0, l]), float(hy[0, l])

    def put(self, l, x, y, body=None, off=0.0, **words):
        """slot l at (x, y); body: given, or the direction of the ball plus `off` degrees"""
        self.s['x'][0, l], self.s['y'][0, l] = x, y
        if body is None:
            bx, by = self.ball
            dx, dy = bx - float(self.s['x'][0, l]), by - float(self.s['y'][0, l])
            body = (np.degrees(np.arctan2(dy, dx)) if (dx or dy) else 0.0) + off
            body = body - 360.0 if body > 180.0 else (body + 360.0 if body <= -180.0 else body)
        self.s['body'][0, l] = body
        for k, v in words.items():
            self.s[k][0, l] = v
        return self

    def base(self, chaser_left, chaser_right):
        """the quiet base's answers in a mode both teams play in"""
        for l in range(22):
            self.want[l] = (NONE, 6) if l in (0, 11) else (NONE, 7)
        for c in (chaser_left, chaser_right):
            if c is not None:
                self.want[c] = (DASH, 5)
        return self

    def all(self, cmd, rule):
        for l in range(22):
            self.want[l] = (cmd, rule)
        return self

    def expect(self, l, cmd, rule, ang=None):
        self.want[l] = (cmd, rule)
        if ang is not None:
            self.ang[l] = ang
        return self


def _swapped(sc):
    out = Scene.__new__(Scene)
    out.name, out.prm, out.swap = sc.name + ' (right)', sc.prm, False
    out.s = SY.swap_x(sc.s, 'state')
    out.want = {(l + 11) % 22: v for l, v in sc.want.items()}
    out.ang = {(l + 11) % 22: -v for l, v in sc.ang.items()}      # a relative angle mirrors with the pitch
    return out


def scenes(cfg):
    """the table for one configuration: a list of Scene, the left version of each followed by its swap_x"""
    prm = SP.params(cfg)
    ka = np.sqrt(prm[0].astype(np.float64))
    cl = prm[1].astype(np.float64)
    pen_x, pen_half_w = np.float32(prm[2][3]), np.float32(prm[2][4])
    hetero = len(set(cfg.player_type_id[i] for i in range(22))) > 1
    f32 = np.float32
    out = []

    def new(name, **kw):
        sc = Scene(name, prm, **kw)
        out.append(sc)
        return sc

    # ------------------------------------------------------------------ rule 1
    for mode in range(32):
        if mode in (M.GM_PENALTY_READY, M.GM_PENALTY_TAKEN):
            continue                                          # the shoot-out's own scenes, below
        sc = new(f'mode {mode}, left side', mode=mode, mode_side=LEFT)
        if mode in QUIET_MODES:
            sc.all(NONE, 1)
        elif mode == M.GM_PLAY_ON:
            sc.base(9, 20)
        else:
            assert mode in SET_PLAYS, mode
            sc.base(9, None)                                  # the left's restart: nobody of the right team chases
    sc = new('the nearest player is tackling: he does nothing and stays his team\'s nearest, so nobody chases').base(9, 20)
    sc.put(9, *sc.home(9), tackle_cycles=3).expect(9, NONE, 1)
    sc = new('a tackling player with the ball at his feet does not kick').base(9, 20)
    sc.put(9, -0.5, -3.0, tackle_cycles=1).expect(9, NONE, 1)
    sc = new('a sent-off player with the ball at his feet does not kick; the next nearest chases').base(10, 20)
    sc.put(9, -0.5, -3.0, card=M.CARD_RED).expect(9, NONE, 1)
    sc = new('a booked player plays on').base(9, 20)
    sc.put(9, *sc.home(9), card=M.CARD_YELLOW)
    # ------------------------------------------------------------------ rule 2
    for holder, what in ((1, 'the holder clears the ball, however far it lies'), (0, 'nobody holds the ball'),
                         (12, 'the other goalie holds the ball')):
        sc = new(f'FreeKick_: {what}', ball=(-48.0, -2.0), mode=M.GM_FREE_KICK, mode_side=LEFT, ball_holder=holder).base(2, None)
        if holder == 1:
            sc.expect(0, KICK, 2)
        if holder == 12:
            sc.expect(11, KICK, 2)                            # rule 2 asks for the mode and the holder, not for the side
    # ------------------------------------------------------------------ rule 3
    G = (-45.0, -2.0)

    def catch_scene(name, dist=None, body=0.0, chasers=(6, 20), **kw):
        d = 0.8 * cl[0] if dist is None else dist
        sc = new(name, ball=(G[0] + d, G[1]), last_touch_side=kw.pop('touch', RIGHT), **kw).base(*chasers)
        sc.put(0, G[0], G[1], body=body)
        return sc
    catch_scene('catch: the ball in reach, in the cone, in the area, played by the others').expect(0, CATCH, 3, ang=0.0)
    catch_scene('catch length: just inside', dist=0.999 * cl[0]).expect(0, CATCH, 3)
    catch_scene('catch length: just outside (and not kickable): back to the guard point', dist=1.001 * cl[0]).expect(0, TURN, 6)
    for sgn, name in ((1.0, 'max'), (-1.0, 'min')):
        catch_scene(f'{name} catch angle: inside', body=-sgn * 89.9).expect(0, CATCH, 3, ang=sgn * 89.9)
        catch_scene(f'{name} catch angle: outside, the kickable ball is kicked', body=-sgn * 90.1).expect(0, KICK, 4)
    for sgn, ch in ((-1.0, (5, 20)), (1.0, (8, 21))):
        for y, inside in ((pen_half_w, True), (np.nextafter(pen_half_w, f32(np.inf)), False)):
            sc = new(f'ball y = {sgn * y!r}: {"on" if inside else "one ulp outside"} the penalty area\'s side line',
                     ball=(-45.0, sgn * y), last_touch_side=RIGHT).base(*ch)
            sc.put(0, -45.0, sgn * (float(y) - 0.5))
            sc.expect(0, *((CATCH, 3) if inside else (KICK, 4)))
    for x, inside in ((-pen_x, True), (np.nextafter(-pen_x, f32(0)), False)):
        sc = new(f'ball x = {x!r}: {"on" if inside else "one ulp outside"} the penalty area\'s front line', ball=(x, -2.0),
                 last_touch_side=RIGHT).base(6, 20)
        sc.put(0, float(x) - 0.5, -2.0)
        sc.expect(0, *((CATCH, 3) if inside else (KICK, 4)))
    sc = catch_scene('catch ban 1: no catch, the kickable ball is kicked').expect(0, KICK, 4)
    sc.put(0, *G, body=0.0, catch_ban=1)
    catch_scene('last touch by the own side: a back pass is not caught', touch=LEFT).expect(0, KICK, 4)
    catch_scene('last touch by nobody: not caught', touch=0).expect(0, KICK, 4)
    catch_scene('a goalie in the other mode: KickIn_ of his side, he kicks', mode=M.GM_KICK_IN, mode_side=LEFT,
                chasers=(6, None)).expect(0, KICK, 4)
    # 1.5 m: beyond the default catch length 1.2 and kickable area 1.085; within this table's typed goalie's 1.2 * 1.32 = 1.584
    catch_scene('1.5 m: only a stretched goalie reaches', dist=1.5).expect(0, *((CATCH, 3) if hetero else (TURN, 6)))
    # ------------------------------------------------------------------ rules 4 and 5
    B = (0.0, -3.0)
    new('kickable bound of slot 9: just inside').base(9, 20).put(9, B[0] - 0.999 * ka[9], B[1]).expect(9, KICK, 4)
    new('kickable bound of slot 9: just outside, he is the chaser').base(9, 20).put(9, B[0] - 1.001 * ka[9], B[1]).expect(9, DASH, 5)
    # exactly on the two bounds that the rules compare with <= and >: the squared distance an fp32 word equal to the bound, the
    # bearing exactly S2D_SCRIPT_TURN_TOL (ball straight ahead of a body of +-10).  The rows are ill-conditioned under the probes;
    # the restatement, the device and unprobed float64 must agree on them
    dx, dx_out, dy = on_the_bound(prm[0][9])
    new('slot 9 exactly on his kickable bound: he kicks').base(9, 20).put(9, B[0] - dx, B[1] - dy).expect(9, KICK, 4)
    new('slot 9 one ulp outside his kickable bound: he chases').base(9, 20).put(9, B[0] - dx_out, B[1] - dy).expect(9, DASH, 5)
    for body in (10.0, -10.0):
        sc = new(f'the chaser\'s body {body}, the ball straight along +x: exactly the turn tolerance, he dashes').base(9, 20)
        sc.put(9, B[0] - 5.0, B[1], body=body).expect(9, DASH, 5)
    if hetero:                                                # kickable areas 1.17 (slot 9) and 1.195 (slot 10)
        sc = new('two types at 1.18 m and 1.185 m: slot 9 cannot kick and chases, slot 10 kicks').base(9, 20)
        sc.put(9, B[0] - 1.18, B[1]).put(10, B[0] + 1.185, B[1]).expect(10, KICK, 4)
    for mode in SET_PLAYS:
        sc = new(f'mode {mode}: the taking side kicks the kickable ball, the other side keeps its places', mode=mode,
                 mode_side=LEFT).base(9, None)
        sc.put(9, B[0] - 0.5, B[1]).expect(9, KICK, 4)
        sc.put(20, B[0] + 0.5, B[1], body=180.0).expect(20, TURN, 7)         # on the ball, and sent home: 10 m behind his back
    sc = new('a tie of two (slots 6, 8; swapped 17, 19: not the first lane of a quarter-wave)', ball=(0.0, 0.0)).base(6, 20)
    sc.put(6, 3.0, 4.0).put(8, -4.0, 3.0).expect(8, TURN, 7)
    sc = new('a tie of two across the quarter-waves (slots 2, 7; swapped 13, 18)', ball=(0.0, 0.0)).base(2, 20)
    sc.put(2, 0.0, 5.0).put(7, -3.0, -4.0).expect(7, TURN, 7)
    sc = new('a tie of three (slots 6, 9, 10)', ball=(0.0, 0.0)).base(6, 20)
    sc.put(6, 0.0, 5.0).put(9, 3.0, 4.0).put(10, -4.0, 3.0).expect(9, TURN, 7).expect(10, TURN, 7)
    sc = new('a tie of two at home (slots 9, 10 and 20, 21 stand mirrored about the ball)', ball=(0.0, 0.0)).base(9, 20)
    sc = new('the goalie is the nearest: a field player chases', ball=(-43.5, -2.0), last_touch_side=LEFT).base(6, 20)
    sc.put(0, *G, body=0.0).expect(0, TURN, 6)
    sc = new('the nearest field player is sent off: the next one chases').base(10, 20)
    sc.put(9, *sc.home(9), card=M.CARD_RED).expect(9, NONE, 1)
    sc = new('all ten field players sent off: nobody chases').base(None, 20)
    for l in range(1, 11):
        sc.put(l, *sc.home(l), card=M.CARD_RED).expect(l, NONE, 1)
    for off, cmd in ((9.9, DASH), (-9.9, DASH), (10.1, TURN), (-10.1, TURN)):
        sc = new(f'the chaser {off} degrees off the ball').base(9, 20)
        sc.put(9, *sc.home(9), off=off).expect(9, cmd, 5, ang=-off if cmd == TURN else None)
    # ------------------------------------------------------------------ rules 6 and 7
    for sgn, ch_in, ch_out in ((1.0, (7, 21), (8, 21)), (-1.0, (6, 20), (5, 20))):
        sc = new(f'guard point y inside the clamp: ball y = {sgn * 19.6}', ball=(-30.0, sgn * 19.6)).base(*ch_in)
        sc.put(0, -50.0, sgn * 5.85)                          # 0.95 m from (-50, 4.9)
        sc = new(f'guard point y clamped: ball y = {sgn * 24.0}', ball=(-30.0, sgn * 24.0)).base(*ch_out)
        sc.put(0, -50.0, sgn * 6.05).expect(0, TURN, 6)       # 1.05 m from (-50, 5); 0.05 m from an unclamped (-50, 6)
    new('home positions clamped to the goal line: ball x = -50', ball=(-50.0, 3.0)).base(3, 21)
    new('home positions clamped to the touch line: ball y = 52', ball=(0.0, 52.0)).base(8, 19)
    new('home positions clamped to the touch line: ball y = -52', ball=(0.0, -52.0)).base(5, 16)
    for l, rule in ((5, 7), (0, 6)):
        sc = new(f'slot {l} 0.99 m from his place: arrived').base(9, 20)
        hx, hy = sc.home(l)
        sc.put(l, hx + 0.99, hy)
        sc = new(f'slot {l} 1.01 m from his place: not arrived, it lies behind him').base(9, 20)
        sc.put(l, hx + 1.01, hy).expect(l, TURN, rule)
        sc = new(f'slot {l} 5 m from his place and facing it: he dashes').base(9, 20)
        sc.put(l, hx + 5.0, hy, body=180.0).expect(l, DASH, rule)
        sc = new(f'slot {l} arrived, the ball 90 degrees off: he turns to it').base(9, 20)
        sc.put(l, hx, hy, off=90.0).expect(l, TURN, rule, ang=-90.0)
    # ------------------------------------------------------------------ rule 8 (played at the right goal: not swapped)
    SPOT = (42.5, -0.75)                                      # (off the axis: the waiting players' places do not tie)
    UPPER = (3 << 12) | (2 << 16) | (1 << 20) | (1 << 24)
    for mode in (M.GM_PENALTY_READY, M.GM_PENALTY_TAKEN):
        for side, taker, keeper in ((LEFT, 10, 11), (RIGHT, 21, 0)):
            for word, what in ((taker + 1, ''), (taker + 1 + UPPER, ', the word\'s upper bits set')):
                sc = new(f'mode {mode}, taker {taker}{what}: he shoots at the right goal', ball=SPOT, mode=mode, mode_side=side,
                         set_play_taker=word, swap=False).all(NONE, 8)
                sc.put(taker, 42.0, 0.0, body=0.0).expect(taker, KICK, 4, ang=0.0)    # 0.9 m from the ball, on the goal's axis
                sc.put(keeper, 50.0, 0.0)
                if mode == M.GM_PENALTY_TAKEN:
                    sc.expect(keeper, NONE, 6)                # on the guard point (50, 0) of the right goal, facing the ball
            sc = new(f'mode {mode}, side {side}: taker byte 0, nobody takes', ball=SPOT, mode=mode, mode_side=side,
                     set_play_taker=UPPER, swap=False).all(NONE, 8)
            sc.put(keeper, 50.0, 0.0)
            if mode == M.GM_PENALTY_TAKEN:
                sc.expect(keeper, NONE, 6)
            sc = new(f'mode {mode}, taker {taker} 8 m away: he dashes as his team\'s chaser although slot {taker - 1} is nearer',
                     ball=SPOT, mode=mode, mode_side=side, set_play_taker=taker + 1, swap=False).all(NONE, 8)
            sc.put(taker, SPOT[0] - 8.0, SPOT[1]).put(taker - 1, SPOT[0] - 2.0, SPOT[1]).expect(taker, DASH, 5)
            sc.put(keeper, 47.0, 0.0, body=180.0)
            if mode == M.GM_PENALTY_TAKEN:
                sc.expect(keeper, TURN, 6)                    # the guard point (50, 0) lies behind him
            # the keeper with the ball in his hands' reach: caught in PenaltyTaken_ only, and only after the taker's touch
            for touch in (side, 0):
                sc = new(f'mode {mode}, side {side}, last touch {touch}: the ball in the keeper\'s reach', ball=(49.0, 0.5), mode=mode,
                         mode_side=side, set_play_taker=taker + 1, last_touch_side=touch, swap=False).all(NONE, 8)
                sc.put(taker, 44.0, 0.5).expect(taker, DASH, 5)
                sc.put(keeper, 49.0 + 0.8 * cl[keeper], 0.5)
                if mode == M.GM_PENALTY_TAKEN:
                    sc.expect(keeper, *((CATCH, 3) if touch == side else (NONE, 6)))     # (within 1 m of the guard point)
    table = []
    for sc in out:
        table.append(sc)
        if sc.swap:
            table.append(_swapped(sc))
    return table


def batch(table):
    """(state [n] of every MATCH_BUFFER_FIELDS word, cmd [n, 22], rule [n, 22], [(match, slot, angle)]) of a table"""
    state = {k: np.concatenate([sc.s[k] for sc in table]) for k in table[0].s}
    cmd = np.array([[sc.want[l][0] for l in range(22)] for sc in table])
    rule = np.array([[sc.want[l][1] for l in range(22)] for sc in table])
    angles = [(e, l, a) for e, sc in enumerate(table) for l, a in sc.ang.items()]
    return state, cmd, rule, angles


def check(table, cmd, rule, angles, got_cmd, got_rule=None, got_ang=None, rows=None):
    """failure strings: the hand-written answers against commands [n, 22] (and rules, and angle words); rows: bool [n, 22] to hold"""
    fails = []
    for e, sc in enumerate(table):
        for l in range(22):
            if rows is not None and not rows[e, l]:
                continue
            if got_cmd[e, l] != cmd[e, l] or (got_rule is not None and got_rule[e, l] != rule[e, l]):
                fails.append(f'{sc.name}: slot {l} got command {got_cmd[e, l]}' + (f' by rule {got_rule[e, l]}' if got_rule is not None else '')
                             + f', expected {cmd[e, l]} by rule {rule[e, l]}')
    if got_ang is not None:
        for e, l, a in angles:
            d = abs(float(got_ang[e, l]) - a)
            if min(d, abs(360.0 - d)) > 1e-3 and (rows is None or rows[e, l]):
                fails.append(f'{table[e].name}: slot {l} angle {float(got_ang[e, l])!r}, expected {a!r}')
    return fails
