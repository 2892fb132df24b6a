"""Constructed ENGINE STATES whose belief update has a known answer (include/s2d_match.h, "Belief"): the table that takes the
edges of tests/belief_scenes.py to the SECOND copy of the rule, belief_update() of csrc/s2d_belief_row.h, which the cycle kernel
calls on a see row it builds itself from the engine state.  Shared by tests/test_belief_state_scenes_host.py (see_ref -> belief_ref
and float64) and tests/test_gpu_match_belief_net_edges.py (the cycle kernel).  TEST INFRASTRUCTURE.

A state scene is one update of one agent: the engine planes of one match (x, y, vx, vy, body of the 22 players and the ball, cards,
mode words, the done byte), the three vision planes, the agent's slot, a parameter set (belief_scenes.PARAMS; the vision parameters
are VISION for every scene), the prior belief row, what the see row of that state MUST contain (level, team, unum, dist, dir of
every player row, in order, and the ball's level: `check_see`), and the hand-written answer in belief_scenes.Scene's form: every
entry known afterwards word for word, every other entry the canonical unknown one, the self and game words the see row's.

How a state makes the see row it wants.  Everything is written in the AGENT'S OWN FRAME (own-frame slot k: 0..10 its team, 11..21
the other one; `state()` turns it into the engine's frame for an agent of the right team).  The agent stands at the origin, body
and neck 0, view width wide.  VISION gives the wide view a half angle of 100 degrees, so a player ON THE Y AXIS is seen at
direction +-90, and the identity bands are narrow and far apart: a player in view at d <= 10 m is level 4, at 10.5 <= d <= 20
level 3, at d >= 20.5 level 2, with no draw.  A player BEHIND the agent (direction 180) within visible_distance = 3 m is felt:
level 1.  dist_round = 0.5 and a fine dist_quantize_step make the see row's dist word the true distance at every multiple of 0.5 m;
face + dir is a multiple of 90 degrees, so the fix is exactly (sx + dist c, sy + dist s) = where the player stands.  Players a scene
does not use are parked behind the agent at 30 m and more, the ball at 25 m: unseen.  The prior is free and carries the edges: exact
floats at a chosen offset from the fix.  The belief's cone for the wide view is 90 - 5 = 85 degrees (82 under `other`): entries on
the y axis or behind are outside it, so no ghost rule reaches them unless a scene is about ghosts.

A scene tagged `near` stands on an edge or one float beside it; under the probes of tests/belief_f64.py it is ill-conditioned on
purpose and every other scene is not; the share of such scenes stays below belief_f64.EDGE_ILL_CAP / 2.

What the cycle kernel CANNOT be driven to, and therefore stays pinned on the scan kernel alone (tests/belief_scenes.py through
tests/test_gpu_match_belief_edges.py), which is why the bitwise fused-against-scan comparison stays as it is:
  * non-finite see words (dist = inf or NaN, a NaN team word): the see row is built from finite planes by finite arithmetic;
  * malformed identities (unum 0, 12 or 2.5, team 0 on a level-4 row) and two level-4 rows naming one entry: one player gives one
    row, with its own team and unum.  `first pass` is therefore a level-4 row naming an entry that a level 1-3 row would also match;
  * a sighting of the agent itself (a level-4 row with the agent's own unum): the see row leaves the agent out;
  * level words other than 0..4, team words other than -1, 0, +1, view codes other than 1, 2, 3, a fresh word other than 0 or 1;
  * non-finite or negative or fractional counts in the prior are reachable (the prior is free) but are the scan kernel's scenes
    already and bring nothing the see row's origin changes; they are left there."""
import numpy as np

import belief_scenes as SC

f32 = np.float32
PARAMS = SC.PARAMS
USED = ('default', 'other', 'cm1', 'cm2', 'md0', 'mr0', 'cone45', 'negcone')
BULLETS = ('min', 'tie', 'competing', 'first pass', 'team word', 'tolerance', 'gate', 'levels', 'ghosts', 'counts', 'reset flag')
# the vision parameters of every scene (over match_see.DEFAULTS / s2d_match_vision_default_params)
VISION = dict(view_angle=(60.0, 120.0, 200.0), visible_distance=3.0, dist_quantize_step=0.001, dist_round=0.5,
              dist_chg_quantize=0.015625, dir_chg_quantize=0.125, unum_far_length=10.0, unum_too_far_length=10.5,
              team_far_length=20.0, team_too_far_length=20.5)
INTERVAL = (1, 2, 3)                                      # see_interval by width code - 1 (the defaults)
BELIEF_VIEW = (60.0, 120.0, 180.0)                        # belief.DEFAULTS' (the engine would default to the vision's)
PLAY_ON = 2                                               # S2D GM_PLAY_ON
PARK_X, PARK_BALL = -30.0, -25.0
P4 = float(f32(0.4))                                      # player_decay, ball_decay as fp32
B94 = float(f32(0.94))
up = lambda v: float(np.nextafter(f32(v), f32(np.inf)))   # noqa: E731
down = lambda v: float(np.nextafter(f32(v), f32(-np.inf)))  # noqa: E731


def belief_over(prm):
    """the S2DBeliefParams fields an engine gets for parameter set `prm` (the view angles explicitly: enable_belief would take the
    vision's); belief.params(**PARAMS[prm]) are the same values on the host"""
    return dict({'view_angle': BELIEF_VIEW}, **PARAMS[prm])


def row_of(u, k):
    """the player row of own-frame slot k (belief.row_of in the own frame)"""
    assert k != u
    return (k if k < u else k - 1) if k < 11 else k - 1


def identity(k):
    """(team, unum) of own-frame slot k on a level-4 row"""
    return (1, k + 1) if k < 11 else (-1, k - 10)


def turned(b):
    return b - 180.0 if b > 0.0 else b + 180.0


class StateScene(SC.Scene):
    def __init__(self, table, name, bullet, prm='default', slot=0, done=0, near=False, at=(0.0, 0.0), body=0.0, width=3, wait=None, card=0):
        assert bullet in BULLETS and prm in USED
        super().__init__([], name, bullet, prm, slot, done, near)
        self.see = None                                   # (the see row is the state's: answer(see))
        self.u = slot % 11
        self.done, self.width, self.card = done, width, card
        self.wait = INTERVAL[width - 1] if wait is None else wait
        self.fresh = self.wait == INTERVAL[width - 1]
        self.can = self.fresh and card < 2
        self.objects = {self.u: (at[0], at[1], 0.0, 0.0, body)}
        self.ball = (PARK_BALL, 0.0, 0.0, 0.0)
        self.rows, self.ball_sees = [], (0, 0.0, 0.0)
        self.ties = []
        table.append(self)

    # ---- the state
    def put(self, k, x, y, vx=0.0, vy=0.0, body=0.0):
        """the player of own-frame slot k"""
        assert 0 <= k < 22 and k != self.u and k not in self.objects
        self.objects[k] = (x, y, vx, vy, body)
        return self

    def put_ball(self, x, y, vx=0.0, vy=0.0):
        self.ball = (x, y, vx, vy)
        return self

    def state(self):
        """the planes of one match in the engine's frame: float32 / int32 [24] each, and the words"""
        right = self.slot >= 11
        sg = -1.0 if right else 1.0
        st = {k: np.zeros(24, dtype=f32) for k in ('x', 'y', 'vx', 'vy', 'body', 'neck')}
        st['card'] = np.zeros(24, dtype=np.int32)
        st['view_width'] = np.full(24, 2, dtype=np.int32)
        st['see_wait'] = np.full(24, 2, dtype=np.int32)
        for k in range(22):
            x, y, vx, vy, body = self.objects.get(k, (PARK_X - 0.5 * k, 0.0, 0.0, 0.0, 0.0))
            w = (k + 11) % 22 if right else k
            st['x'][w], st['y'][w], st['vx'][w], st['vy'][w] = sg * x, sg * y, sg * vx, sg * vy
            st['body'][w] = turned(body) if right else body
        bx, by, bvx, bvy = self.ball
        st['x'][22], st['y'][22], st['vx'][22], st['vy'][22] = sg * bx, sg * by, sg * bvx, sg * bvy
        st['view_width'][self.slot], st['see_wait'][self.slot], st['card'][self.slot] = self.width, self.wait, self.card
        st.update(mode=PLAY_ON, mode_side=0, cycle=7)
        return st

    # ---- what the see row must contain
    def sees(self, *rows, ball=(0, 0.0, 0.0)):
        """rows: (level, team, unum, dist, dir) of every player row, in the see row's order; ball: (level, dist, dir)"""
        self.rows, self.ball_sees = list(rows), ball
        return self

    def pending(self):
        return self.can and any(r[0] in (1, 2, 3) for r in self.rows)

    def check_see(self, row):
        """the words of `row` that are not what the scene states, as text"""
        at = self.objects[self.u]
        bad = []
        for w, want, what in ((0, at[0], 'x'), (1, at[1], 'y'), (4, at[4], 'body'), (5, 0.0, 'neck'), (7, self.width, 'width'),
                              (8, float(self.fresh), 'fresh'), (15, self.card, 'card'), (21, PLAY_ON, 'mode'), (23, 7, 'cycle')):
            if float(row[w]) != float(f32(want)):
                bad.append(f'{what}: {row[w]!r}, stated {want!r}')
        rows = self.rows if self.can else []
        for r in range(21):
            got = tuple(float(v) for v in row[24 + 8 * r:29 + 8 * r])
            want = tuple(float(v) for v in rows[r]) if r < len(rows) else (0.0,) * 5
            if got != want:
                bad.append(f'player row {r}: {got}, stated {want}')
        got = tuple(float(v) for v in row[16:19])
        want = tuple(float(v) for v in self.ball_sees) if self.can else (0.0,) * 3
        if got != want:
            bad.append(f'ball: {got}, stated {want}')
        return bad

    def tie(self, *rows):
        """prior rows that the scene claims stand at a bit-equal squared distance from the first level 1-3 fix"""
        self.ties = list(rows)
        return self

    def look(self, **kw):
        raise TypeError('a state scene has no free see row')

    def answer(self, see):
        self.see = np.asarray(see, dtype=f32)
        return super().answer()


AXIS = {3: ((0.0, 1.0), 15.0, 90.0), 2: ((0.0, 1.0), 25.0, 90.0), 1: ((-1.0, 0.0), 2.0, 180.0)}   # level -> (axis, distance, dir)


def _on(axis, d):
    return (axis[0] * d + 0.0, axis[1] * d + 0.0)         # (+ 0.0: no negative zero)


def table():
    """every scene, in a fixed order"""
    T = []
    # ---- minimum: the nearest known entry in each of the 21 rows in turn, for a level 3, 2 and 1 row.  Farther candidates in every
    # third row; for level 3 a NEARER entry of the other team, which the team word keeps out
    for lv in (3, 2, 1):
        axis, d0, direc = AXIS[lv]
        for r in range(21):
            slot = (r * 5 + lv) % 22
            u = slot % 11
            mate = r < 10
            k = ((u + 1) % 11) if mate else 11 + r % 11   # the player who is seen
            sc = StateScene(T, f'level {lv}: nearest in row {r}', 'min', slot=slot)
            sc.put(k, *_on(axis, d0))
            team = (1 if mate else -1) if lv == 3 else 0
            sc.sees((lv, team, 0, d0, direc))
            for j in range(21):
                if j == r:
                    sc.know(j, *_on(axis, d0 + 0.5)).then(j, *_on(axis, d0), counts=(0, 3, 3))
                elif j % 3 == 0:
                    p = _on(axis, d0 + 1.5 + 0.125 * j)
                    sc.know(j, *p).then(j, *p)
                elif lv == 3 and j % 3 == 1 and (j < 10) != mate:
                    p = _on(axis, d0 + 0.25)
                    sc.know(j, *p).then(j, *p)
    # ---- ties: bit-equal squared distances, the lowest row takes the fix (entry lane = row + 1)
    sc = StateScene(T, 'tie of two, rows 3 and 4', 'tie', near=True).put(5, 0.0, 15.0).sees((3, 1, 0, 15.0, 90.0))
    sc.know(3, 0.0, 16.0).know(4, 0.0, 14.0).know(7, 0.0, 17.0).tie(3, 4)
    sc.then(3, 0.0, 15.0, counts=(0, 3, 3)).then(4, 0.0, 14.0).then(7, 0.0, 17.0)
    sc = StateScene(T, 'tie of two, rows 14 and 15 (across the rows of 16 lanes)', 'tie', near=True, slot=13).put(12, 0.0, 15.0)
    sc.sees((3, -1, 0, 15.0, 90.0)).know(14, 0.0, 14.0).know(15, 0.0, 16.0).know(20, 0.0, 17.5).tie(14, 15)
    sc.then(14, 0.0, 15.0, counts=(0, 3, 3)).then(15, 0.0, 16.0).then(20, 0.0, 17.5)
    sc = StateScene(T, 'tie of three, rows 2, 6 and 9', 'tie', near=True, slot=4).put(20, 0.0, 25.0).sees((2, 0, 0, 25.0, 90.0))
    sc.know(2, 0.0, 26.0).know(6, 0.0, 24.0).know(9, -1.0, 25.0).know(10, 0.0, 27.0).tie(2, 6, 9)
    sc.then(2, 0.0, 25.0, counts=(0, 3, 3)).then(6, 0.0, 24.0).then(9, -1.0, 25.0).then(10, 0.0, 27.0)
    sc = StateScene(T, 'tie of two, rows 9 and 10 (no team word)', 'tie', slot=18).put(3, 0.0, 25.0).sees((2, 0, 0, 25.0, 90.0))
    sc.know(9, 0.0, 26.5).know(10, 0.0, 23.5).know(4, 0.0, 28.0).tie(9, 10)
    sc.then(9, 0.0, 25.0, counts=(0, 3, 3)).then(10, 0.0, 23.5).then(4, 0.0, 28.0)
    sc.near = True
    # ---- competing rows: in the see row's order; an updated entry is no longer a candidate
    sc = StateScene(T, 'two rows and one entry: the first takes it, the second is dropped', 'competing', slot=3)
    sc.put(2, 0.0, 15.0).put(4, 0.0, 16.0).sees((3, 1, 0, 15.0, 90.0), (3, 1, 0, 16.0, 90.0))
    sc.know(1, 0.0, 15.75).know(12, 0.0, 16.0)            # (row 1 is nearer to the second row; row 12 is the other team's)
    sc.then(1, 0.0, 15.0, counts=(0, 3, 3)).then(12, 0.0, 16.0)
    sc = StateScene(T, 'two rows and two entries: the second takes the next candidate', 'competing', slot=14)
    sc.put(2, 0.0, 15.0).put(4, 0.0, 16.0).sees((3, 1, 0, 15.0, 90.0), (3, 1, 0, 16.0, 90.0))
    sc.know(0, 0.0, 14.0).know(1, 0.0, 15.75)
    sc.then(1, 0.0, 15.0, counts=(0, 3, 3)).then(0, 0.0, 16.0, counts=(0, 3, 3))
    # ---- first pass: the entry a level-4 row names is taken before the level 1-3 rows, wherever its row stands
    sc = StateScene(T, 'a level-4 row names the entry an earlier level-3 row is nearest to', 'first pass')
    sc.put(6, 0.0, -11.0).put(3, 0.0, 8.0, body=45.0).sees((3, 1, 0, 11.0, -90.0), (4, 1, 4, 8.0, 90.0))
    sc.know(2, 0.0, -10.75).know(5, 0.0, -12.5)
    sc.then(2, 0.0, 8.0, body=45.0, counts=(0, 0, 0)).then(5, 0.0, -11.0, counts=(0, 3, 3))
    for prm, slot in [('default', s) for s in range(22)] + [('other', s) for s in range(22)]:
        u = slot % 11
        sc = StateScene(T, f'all 21 identities seen from slot {slot} ({prm})', 'first pass', prm=prm, slot=slot)
        rows = []
        for k in range(22):
            if k == u:
                continue
            n = k % 11 + 1
            y, body = (0.5 * n + 0.5, 10.0 * n) if k < 11 else (-(0.5 * n + 0.5), -10.0 * n)
            sc.put(k, 0.0, y, body=body)
            rows.append((4,) + identity(k) + (abs(y), 90.0 if y > 0 else -90.0))
            sc.then(row_of(u, k), 0.0, y, body=body, counts=(0, 0, 0))
        sc.sees(*sorted(rows, key=lambda r: (r[4], r[3])))
    # ---- the team word: a level-3 row of either team against entries in rows 9 and 10, the other team's entry the nearer one
    for slot in range(22):
        u = slot % 11
        sc = StateScene(T, f'level 3, team word > 0, from slot {slot}: row 10 nearer, row 9 taken', 'team word', slot=slot)
        sc.put((u + 1) % 11, 0.0, 15.0).sees((3, 1, 0, 15.0, 90.0)).know(9, 0.0, 15.5).know(10, 0.0, 15.25)
        sc.then(9, 0.0, 15.0, counts=(0, 3, 3)).then(10, 0.0, 15.25)
        sc = StateScene(T, f'level 3, team word < 0, from slot {slot}: row 9 nearer, row 10 taken', 'team word', slot=slot)
        sc.put(11 + (u + 3) % 11, 0.0, 15.0).sees((3, -1, 0, 15.0, 90.0)).know(9, 0.0, 15.25).know(10, 0.0, 15.5)
        sc.then(10, 0.0, 15.0, counts=(0, 3, 3)).then(9, 0.0, 15.25)
    # ---- tolerance: md0: tol = 0.125 * 16 = 2; mr0: tol = 3 at any distance
    for prm, d, tag in (('md0', 16.0, 'match_dist = 0'), ('mr0', 15.0, 'match_rate = 0')):
        for y, what, hit in ((18.0, 'exactly at tol', True), (down(18.0), 'one float inside tol', True), (up(18.0), 'one float outside tol', False)):
            sc = StateScene(T, f'{tag}: an entry {what}', 'tolerance', prm=prm, near=True, slot=7 if hit else 19)
            sc.put(2, 0.0, d).sees((3, 1, 0, d, 90.0)).know(2, 0.0, y)
            sc.then(2, 0.0, d if hit else y, counts=(0, 3, 3) if hit else (3, 3, 3))
    # ---- the gate: not fresh, or sent off: the entries age only, the self words are copied
    for tag, kw in (('see_wait 2 of 3: not fresh', dict(wait=2)), ('see_wait 1 of 3: not fresh', dict(wait=1)), ('the agent is sent off', dict(card=2))):
        sc = StateScene(T, f'{tag}, with players and the ball in view', 'gate', slot=15, at=(3.0, 4.0), **kw)
        sc.put(2, 3.0, 10.0).put(13, 3.0, 19.0).put_ball(8.0, 4.0)
        sc.know(1, 3.0, 14.0, 1.0, -1.0, 30.0, (2, 5, 7)).know(4, 8.0, 4.0).know_ball(8.0, 4.0, 0.5, 0.25)   # (8, 4): straight ahead
        sc.then(1, 4.0, 13.0, P4, -P4, 30.0, (3, 6, 8)).then(4, 8.0, 4.0).then_ball(8.5, 4.25, 0.5 * B94, 0.25 * B94)
    # ---- levels: a felt ball (level 1) moves the position and keeps the remembered velocity, a seen one (level 4) brings its own
    sc = StateScene(T, 'ball level 1 keeps the remembered velocity', 'levels', slot=17).put_ball(-2.0, 0.0, 0.25, 0.5)
    sc.sees(ball=(1, 2.0, 180.0)).know_ball(5.0, 5.0, 1.0, 0.0).then_ball(-2.0, 0.0, B94, 0.0, 0)
    sc = StateScene(T, 'ball level 4 takes the new velocity', 'levels', slot=6).put_ball(0.0, 4.0, 0.0, 0.5)
    sc.sees(ball=(4, 4.0, 90.0)).know_ball(5.0, 5.0, 1.0, 0.0).then_ball(0.0, 4.0, 0.0, 0.5, 0)
    # ---- ghosts
    sc = StateScene(T, 'an unseen known entry inside the cone is forgotten, one outside is kept', 'ghosts', slot=12)
    sc.know(0, 5.0, 0.0).know(1, 0.0, 5.0).then(1, 0.0, 5.0)
    sc = StateScene(T, 'an entry exactly on the cone is forgotten', 'ghosts', prm='cone45', near=True, slot=21, width=2)
    sc.know(0, 5.0, 5.0).know(1, 5.0, -5.0).know(2, 0.0, 5.0).then(2, 0.0, 5.0)
    sc = StateScene(T, 'the next float outside the cone is kept', 'ghosts', prm='cone45', near=True, slot=1, width=2, body=-2.0 ** -17)
    sc.know(0, 5.0, 5.0).know(1, 5.0, -5.0).then(0, 5.0, 5.0)                   # 45 + 2^-17 > 45 > 45 - 2^-17
    # (not tagged near: the probes move x = 0 and face = 0 by subnormal steps only, which float64's 90 degrees does not feel)
    sc = StateScene(T, 'exactly on a cone of 90 degrees', 'ghosts', prm='cone45', slot=2)
    sc.know(0, 0.0, 5.0).know(1, 0.0, -5.0).know(2, -1.0, 5.0).then(2, -1.0, 5.0)
    sc = StateScene(T, 'an entry exactly at the agent (d = 0) is kept; straight ahead it is forgotten', 'ghosts', near=True, slot=20, at=(1.0, 2.0))
    sc.know(2, 1.0, 2.0).know(3, 2.0, 2.0).then(2, 1.0, 2.0)
    for code, gone in ((1, ()), (2, (0,)), (3, (0, 1))):
        sc = StateScene(T, f'view code {code}', 'ghosts', slot=5, width=code)    # cones 25 / 55 / 85: bearings 45, 59.04 and 90
        sc.know(0, 5.0, 5.0).know(1, 3.0, 5.0).know(2, 0.0, 5.0)
        for j, (x, y) in enumerate(((5.0, 5.0), (3.0, 5.0), (0.0, 5.0))):
            if j not in gone:
                sc.then(j, x, y)
    sc = StateScene(T, 'view_angle < 2 ghost_margin: a negative cone forgets nobody', 'ghosts', prm='negcone', slot=6, width=2)
    sc.know(0, 5.0, 0.0).know_ball(4.0, 0.0).then(0, 5.0, 0.0).then_ball(4.0, 0.0)
    sc = StateScene(T, 'the ball as a ghost', 'ghosts', slot=7).know_ball(5.0, 0.0, 1.0, 0.5).know(0, 0.0, 5.0).then(0, 0.0, 5.0)
    # ---- counts: pos_count at count_max - 3 .. count_max, vel_count and body_count older than pos_count; a fresh agent who sees
    # nobody (the whole update runs) and one who is not fresh (the gate is closed)
    for prm in ('cm1', 'cm2', 'other'):
        cm = SC.count_max(prm)
        old = lambda c: c + 1.0 if c + 1.0 < cm else cm                         # noqa: E731  (the header's words for a count)
        pd = 0.25 if prm == 'other' else P4
        given = [(c, 0, 0) for c in sorted({0.0, cm - 3, cm - 2, cm - 1, cm}) if c >= 0]
        given += [(0, cm - 1, cm)] + ([(0, cm - 2, cm - 1)] if cm >= 2 else []) + ([(1, cm - 1, cm - 2), (cm - 3, cm - 2, cm - 1)] if cm >= 3 else [])
        for tag, kw in (('fresh, nobody in view', {}), ('not fresh', dict(wait=1))):
            sc = StateScene(T, f'count_max {cm:g}, {tag}: pos_count up to count_max, older vel_count and body_count', 'counts', prm=prm, slot=8, **kw)
            for j, c in enumerate(given):
                sc.know(j, -1.0, 10.0 + j, -0.5, 0.0, 20.0, c)
                if c[0] + 1.0 < cm:
                    sc.then(j, -1.5, 10.0 + j, -0.5 * pd, 0.0, 20.0, tuple(old(c1) for c1 in c))
            if cm >= 2:
                sc.know_ball(-1.0, 10.0, 0.0, 0.0, cm - 2).then_ball(-1.0, 10.0, 0.0, 0.0, cm - 1)
    sc = StateScene(T, 'count_max 1: only what this very update saw is known', 'counts', prm='cm1', slot=9)
    sc.put(1, 0.0, 6.0).put(15, 0.0, 25.0).put_ball(-2.0, 0.0).sees((4, 1, 2, 6.0, 90.0), (2, 0, 0, 25.0, 90.0), ball=(1, 2.0, 180.0))
    sc.know(3, 0.0, 25.0, counts=(0, 0, 0)).then(1, 0.0, 6.0, counts=(0, 0, 0)).then_ball(-2.0, 0.0, 0.0, 0.0, 0)   # (u = 9: slot 1 is row 1)
    # ---- the reset flag: the done byte the launch finds; everything is forgotten before the sightings are taken
    for byte in (0, 1, 255):
        sc = StateScene(T, f'done byte {byte} before the launch', 'reset flag', done=byte, slot=10)
        sc.put(17, 0.0, 8.0).put(2, 0.0, 15.0).sees((4, -1, 7, 8.0, 90.0), (3, 1, 0, 15.0, 90.0))
        sc.know(0, 0.0, 15.5).know(16, 0.0, 9.0).know_ball(-4.0, 0.0)
        sc.then(16, 0.0, 8.0, counts=(0, 0, 0))            # the reset comes first: this row is still taken in
        if byte == 0:
            sc.then(0, 0.0, 15.0, counts=(0, 3, 3)).then_ball(-4.0, 0.0)
    return T


# ------------------------------------------------------------------------------------------------ the order of a launch
def kind(s):
    """what the half-wave of this scene does in belief_update(): 'gate' the gate is closed, 'reset' its reset flag is set,
    'none' no level 1-3 row, 'pending' some"""
    return 'gate' if not s.can else 'reset' if s.done else 'pending' if s.pending() else 'none'


def launch_order(scenes):
    """the scenes of one parameter set in the order of their matches: the four kinds in turn, so that neighbours -- the two halves
    of one wave -- take different branches for as long as the kinds last"""
    buckets = {k: [s for s in scenes if kind(s) == k] for k in ('gate', 'reset', 'none', 'pending')}
    out = []
    while any(buckets.values()):
        for k in ('gate', 'pending', 'reset', 'none'):
            if buckets[k]:
                out.append(buckets[k].pop(0))
    return out


def divergences(kinds):
    """kinds: the kind of every match of one launch, None = no scene (a filler match, or none at all).  The set of divergences
    inside the waves (matches 2m and 2m + 1): 'can', 'pending', 'reset'"""
    seen = set()
    for a, b in zip(kinds[0::2], kinds[1::2]):
        if a is None or b is None:
            continue
        if (a == 'gate') != (b == 'gate'):
            seen.add('can')
        if 'gate' not in (a, b) and (a == 'pending') != (b == 'pending'):
            seen.add('pending')
        if 'gate' not in (a, b) and (a == 'reset') != (b == 'reset'):
            seen.add('reset')
    return seen


def write_state(state, m, s):
    """scene s into match m of `state`: a dict of numpy arrays named as match_see.ENGINE_KEYS + VISION_PLANES ([N, 24] planes,
    [N] words), changed in place; returns the done byte"""
    for k, v in s.state().items():
        state[k][m] = v
    return s.done
