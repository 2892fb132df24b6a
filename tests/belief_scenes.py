"""Constructed updates of the belief layer with known answers (include/s2d_match.h, "Belief"): a shared table for
tests/test_belief_f64_host.py (the host restatement and float64) and tests/test_gpu_match_belief_edges.py (the device).  TEST
INFRASTRUCTURE.

A scene is one update of one agent row: a prior belief row, a see row, the agent's slot, the match's reset byte, a parameter set
(PARAMS) and the HAND-WRITTEN answer.  The answer names every entry that is known afterwards, word for word; every entry it does
not name must be the canonical unknown one; the self and game words are the see row's.  All numbers are exactly representable and
every face + dir is a multiple of 90 degrees (sincos_deg is exact there), so every fp32 operation that reaches an answer word is
exact: the restatement, the device and float64 without probes must give the answer in every word -- NaN where the answer is NaN,
bit for bit otherwise, the sign of zero included.  A scene tagged `near` stands one float beside an edge (or exactly on one): its
answer is as exact as the others', and under the probes of tests/belief_f64.py it is ill-conditioned on purpose; the share of such
rows in the table stays below belief_f64.EDGE_ILL_CAP / 2.

The common geometry: the agent at the origin, face 0, narrow view (cone = 60 / 2 - 5 = 25 degrees); sightings at direction 90, which
land on the y axis ((s, c) = (1, -0)), where no ghost rule reaches them."""
import numpy as np

import belief as B

f32 = np.float32
NAN, INF = float('nan'), float('inf')
LIMIT = 16777216.0
PARAMS = {
    'default': {},
    'other': dict(ball_decay=0.5, player_decay=0.25, view_angle=(50.0, 100.0, 170.0), match_dist=2.0, match_rate=0.05, ghost_margin=3.0,
                  count_max=6.0),
    'cm1': dict(count_max=1.0), 'cm2': dict(count_max=2.0), 'cm24': dict(count_max=LIMIT),
    'md0': dict(match_dist=0.0, match_rate=0.125), 'mr0': dict(match_rate=0.0),
    'cone45': dict(view_angle=(100.0, 100.0, 190.0)),      # cones of exactly 45, 45 and 90 degrees
    'full': dict(view_angle=(360.0, 360.0, 360.0), ghost_margin=0.0),          # a cone of exactly 180 degrees
    'negcone': dict(view_angle=(8.0, 8.0, 8.0)),           # view_angle < 2 ghost_margin: cone = -1
}
BULLETS = ('min', 'tie', 'competing', 'first pass', 'team word', 'tolerance', 'gate', 'levels', 'ghosts', 'counts', 'non-finite',
           'reset flag')
up = lambda v: float(np.nextafter(f32(v), f32(np.inf)))                          # noqa: E731


def count_max(prm):
    return float(PARAMS[prm].get('count_max', 1000.0))


def see_row(x=0.0, y=0.0, vx=0.0, vy=0.0, body=0.0, neck=0.0, face=None, width=1, fresh=1, card=0, ball=None, players=(), game=(2, 1, 7)):
    """tests/test_belief_host.see_row's layout, narrow by default: ball = (level, dist, dir, dist_chg, dir_chg); players = rows
    (level, team, unum, dist, dir, dist_chg, dir_chg, body_rel)"""
    s = np.zeros(192, dtype=f32)
    s[0:8] = (x, y, vx, vy, body, neck, body + neck if face is None else face, width)
    s[8], s[9], s[10:14], s[14], s[15] = fresh, 2, (8000, 1, 1, 130600), 0, card
    if ball is not None:
        s[16:21] = ball
    s[21:24] = game
    for r, p in enumerate(players):
        s[24 + 8 * r:32 + 8 * r] = p
    return s


class Scene:
    def __init__(self, table, name, bullet, prm='default', slot=0, flag=0, near=False):
        assert bullet in BULLETS and prm in PARAMS and 0 <= slot < 22
        self.name, self.bullet, self.prm, self.slot, self.flag, self.near = name, bullet, prm, slot, flag, near
        self.cm = count_max(prm)
        self.prior = B.unknown(1, 1, f32(self.cm))[0, 0]
        self.see = see_row()
        self.want = {}                                    # entry (0 = the ball, 1 + j = player row j) -> its words afterwards
        table.append(self)

    def know(self, row, x, y, vx=0.0, vy=0.0, body=0.0, counts=(2, 2, 2)):
        """the prior knows player row `row`"""
        self.prior[24 + 8 * row:32 + 8 * row] = (x, y, vx, vy, body) + tuple(counts)
        return self

    def know_ball(self, x, y, vx=0.0, vy=0.0, count=2):
        self.prior[16:21] = (x, y, vx, vy, count)
        return self

    def look(self, **kw):
        self.see = see_row(**kw)
        return self

    def then(self, row, x, y, vx=0.0, vy=0.0, body=0.0, counts=(3, 3, 3)):
        """the answer: player row `row` afterwards"""
        self.want[1 + row] = (x, y, vx, vy, body) + tuple(counts)
        return self

    def then_ball(self, x, y, vx=0.0, vy=0.0, count=3):
        self.want[0] = (x, y, vx, vy, count)
        return self

    def answer(self):
        """the expected row, fp32 [192]"""
        o = B.unknown(1, 1, f32(self.cm))[0, 0]
        o[:16], o[21:24] = self.see[:16], self.see[21:24]
        for e, w in self.want.items():
            if e == 0:
                o[16:21] = w
            else:
                o[24 + 8 * (e - 1):32 + 8 * (e - 1)] = w
        return o


def identity(u, j):
    """(team, unum) that names player row j for an agent of own index u"""
    return (1, (j if j < u else j + 1) + 1) if j < 10 else (-1, j - 9)


def table():
    """every scene, in a fixed order"""
    T = []
    # ---- minimum: the nearest known entry in each of the 21 player rows in turn; the others farther, unknown or already updated
    for r, lv in ((r, lv) for lv in (2, 1, 3) for r in range(21)):
        sc = Scene(T, f'level {lv}: nearest in row {r}', 'min')
        rows = [(lv, 0, 0, 10.0, 90, 0, 0, 0)]
        for j in range(21):
            if j == r:
                sc.know(j, 0.0, 10.5).then(j, 0.0, 10.0, counts=(0, 3, 3))
            elif j % 3 == 0:                                                    # farther, inside tol = 4
                sc.know(j, 0.0, 11.5 + 0.125 * j).then(j, 0.0, 11.5 + 0.125 * j)
            elif j % 3 == 2 and len(rows) < 8:                                  # on the very spot, but placed by level 4 in this update
                t, n = identity(0, j)
                rows.append((4, t, n, 10.0, 90, 0, 0, 30))
                sc.know(j, 0.0, 10.0).then(j, 0.0, 10.0, body=30.0, counts=(0, 0, 0))
        sc.look(players=rows)
    # ---- ties: the lowest row, across the quad, 16-lane and team boundaries (entry lane = row + 1)
    for a, b, lv, team in ((0, 1, 3, 1), (3, 4, 3, 1), (14, 15, 3, -1), (15, 16, 3, -1), (9, 10, 2, 0)):
        for flip in ((0, 1) if a >= 9 and b != 15 else (0,)):                   # the lower row on either side of the sighting
            sc = Scene(T, f'tie between rows {a} and {b}' + (' (mirrored)' if flip else ''), 'tie', near=True)
            ya, yb = (11.0, 9.0) if flip else (9.0, 11.0)
            c = 20 if team <= 0 else 7                                          # a farther candidate of the same team
            sc.know(a, 0.0, ya).know(b, 0.0, yb).know(c, 0.0, 13.0)
            sc.look(players=[(lv, team, 0, 10.0, 90, 0, 0, 0)])
            sc.then(a, 0.0, 10.0, counts=(0, 3, 3)).then(b, 0.0, yb).then(c, 0.0, 13.0)
    # ---- competing sightings
    sc = Scene(T, 'two sightings nearest to one entry: the first takes it, the second the next candidate', 'competing', slot=3)
    sc.know(0, 0.0, 10.0).know(1, 0.0, 12.0)
    sc.look(players=[(3, 1, 0, 11.75, 90, 0, 0, 0), (3, 1, 0, 12.25, 90, 0, 0, 0)])
    sc.then(1, 0.0, 11.75, counts=(0, 3, 3)).then(0, 0.0, 12.25, counts=(0, 3, 3))
    sc = Scene(T, 'two sightings nearest to one entry: the second is dropped', 'competing', slot=4)
    sc.know(1, 0.0, 12.0).know(12, 0.0, 12.0)
    sc.look(players=[(3, 1, 0, 11.75, 90, 0, 0, 0), (3, 1, 0, 12.25, 90, 0, 0, 0)])
    sc.then(1, 0.0, 11.75, counts=(0, 3, 3)).then(12, 0.0, 12.0)
    sc = Scene(T, 'an entry placed by level 4 is no candidate', 'competing')
    sc.know(0, 0.0, 10.0).know(1, 0.0, 12.0)
    sc.look(players=[(3, 1, 0, 12.25, 90, 0, 0, 0), (4, 1, 3, 12.0, 90, 0, 0, 0)])
    sc.then(1, 0.0, 12.0, counts=(0, 0, 0)).then(0, 0.0, 12.25, counts=(0, 3, 3))
    # ---- first pass
    sc = Scene(T, 'two level-4 rows name one entry: the later wins', 'first pass')
    sc.look(players=[(4, 1, 3, 8.0, 90, 0, 0, 10), (4, -1, 4, 7.0, 90, 0, 0, 0), (4, 1, 3, 9.0, 90, 0, 0, 45)])
    sc.then(1, 0.0, 9.0, body=45.0, counts=(0, 0, 0)).then(13, 0.0, 7.0, counts=(0, 0, 0))
    for slot, prm in ((slot, prm) for prm in ('default', 'other') for slot in range(22)):
        u = slot % 11
        rows = [(4, 1, n, float(n), 90, 0, 0, 10 * n) for n in range(1, 12) if n - 1 != u]
        rows += [(4, -1, n, 20.0 + n, 90, 0, 0, -10 * n) for n in range(1, 12)]
        sc = Scene(T, f'all 21 identities seen from slot {slot} ({prm})', 'first pass', prm=prm, slot=slot)
        sc.look(players=rows[::-1])
        for _lv, team, n, dist, *_rest, brel in rows:
            sc.then((n - 1 if n - 1 < u else n - 2) if team > 0 else n + 9, 0.0, dist, body=float(brel), counts=(0, 0, 0))
        sc = Scene(T, f'junk identities seen from slot {slot} ({prm})', 'first pass', prm=prm, slot=slot)
        sc.look(players=[(4, 1, u + 1, 5.0, 90, 0, 0, 0), (4, 0, 3, 5.0, 90, 0, 0, 0), (4, -1, 12, 5.0, 90, 0, 0, 0), (4, -1, 0, 5.0, 90, 0, 0, 0),
                         (4, 1, 2.5, 5.0, 90, 0, 0, 0)])
    # ---- the team word of a level 1-3 sighting, candidates on both sides of rows 9 | 10
    for word, tag in ((1.0, '> 0'), (-1.0, '< 0'), (0.0, '+0'), (-0.0, '-0'), (NAN, 'NaN')):
        for near9, lv in ((n9, lv) for lv in (2, 1, 3) for n9 in (False, True)):
            sc = Scene(T, f'level {lv}, team word {tag}, row {9 if near9 else 10} nearer', 'team word', slot=5 + near9)
            y9, y10 = (10.25, 9.5) if near9 else (9.5, 10.25)
            sc.know(9, 0.0, y9).know(10, 0.0, y10)
            sc.look(players=[(lv, word, 0, 10.0, 90, 0, 0, 0)])
            take = 9 if word > 0 else 10 if word < 0 else (9 if near9 else 10)
            sc.then(9, 0.0, y9).then(10, 0.0, y10).then(take, 0.0, 10.0, counts=(0, 3, 3))
    # ---- tolerance
    sc = Scene(T, 'q == tol^2 exactly matches (dist 0, 3 m off)', 'tolerance', near=True, slot=7)
    sc.know(2, 0.0, 3.0).look(players=[(2, 0, 0, 0.0, 0, 0, 0, 0)]).then(2, 0.0, 0.0, counts=(0, 3, 3))
    sc = Scene(T, 'the next float above tol does not match', 'tolerance', near=True, slot=8)
    sc.know(2, 0.0, up(3.0)).look(players=[(2, 0, 0, 0.0, 0, 0, 0, 0)]).then(2, 0.0, up(3.0))
    sc = Scene(T, 'match_dist = 0: tol = match_rate * dist', 'tolerance', prm='md0', slot=9)
    sc.know(2, 0.0, 15.0).know(3, 0.0, 18.0).look(players=[(2, 0, 0, 16.0, 90, 0, 0, 0)])           # tol = 2: 1 m off beats 2 m off
    sc.then(2, 0.0, 16.0, counts=(0, 3, 3)).then(3, 0.0, 18.0)
    sc = Scene(T, 'match_dist = 0 and dist = 0: only the very spot matches', 'tolerance', prm='md0', near=True, slot=10)
    sc.know(2, 0.0, 0.0).know(3, 0.0, 0.5).look(players=[(1, 0, 0, 0.0, 0, 0, 0, 0), (1, 0, 0, 0.0, 0, 0, 0, 0)])
    sc.then(2, 0.0, 0.0, counts=(0, 3, 3)).then(3, 0.0, 0.5)
    sc = Scene(T, 'match_rate = 0: tol = match_dist at any distance', 'tolerance', prm='mr0', near=True, slot=11)
    sc.know(4, 0.0, 27.0).know(5, 0.0, 34.5)
    sc.look(players=[(2, 0, 0, 30.0, 90, 0, 0, 0), (2, 0, 0, 31.0, 90, 0, 0, 0)])                   # q = 9 == tol^2; 3.5 m off is dropped
    sc.then(4, 0.0, 30.0, counts=(0, 3, 3)).then(5, 0.0, 34.5)
    sc = Scene(T, 'dist = +inf at direction 45: q = tol^2 = inf, the lowest candidate takes it', 'tolerance', slot=12)
    sc.know(6, 0.0, 10.0).know(8, 0.0, 12.0).look(body=45.0, players=[(2, 0, 0, INF, 0, 0, 0, 0)])
    sc.then(6, INF, INF, counts=(0, 3, 3)).then(8, 0.0, 12.0)
    sc = Scene(T, 'dist = +inf at direction 90: X = inf * 0 = NaN, nothing matches', 'tolerance', near=True, slot=13)
    sc.know(6, 0.0, 10.0).look(players=[(2, 0, 0, INF, 90, 0, 0, 0)]).then(6, 0.0, 10.0)
    sc = Scene(T, 'dist = NaN: nothing matches', 'tolerance', slot=14)
    sc.know(6, 0.0, 10.0).look(players=[(2, 0, 0, NAN, 90, 0, 0, 0)]).then(6, 0.0, 10.0)
    # ---- the gate: the copies still happen, nothing is corrected or forgotten
    full = dict(ball=(4, 5.0, 0, 0, 0), players=[(4, 1, 2, 6.0, 0, 0, 0, 0), (3, 1, 0, 10.0, 90, 0, 0, 0)], x=3.0, y=4.0, game=(4, -1, 99))
    for tag, kw in (('fresh = 0', dict(fresh=0)), ('fresh = 2', dict(fresh=2)), ('card = red, fresh = 1', dict(card=2))):
        sc = Scene(T, f'{tag} with sightings present', 'gate', slot=15)
        sc.know(1, 3.0, 14.0, 1.0, -1.0, 30.0, (2, 5, 7)).know(4, 8.0, 4.0).know_ball(8.0, 4.0, 0.5, 0.25)       # (8, 4): straight ahead
        sc.look(**dict(full, **kw))
        sc.then(1, 4.0, 13.0, float(f32(0.4)), -float(f32(0.4)), 30.0, (3, 6, 8)).then(4, 8.0, 4.0)
        sc.then_ball(8.5, 4.25, 0.5 * float(f32(0.94)), 0.25 * float(f32(0.94)))
    # ---- levels
    for lv, tag in ((0.0, '0'), (0.5, '0.5'), (5.0, '5'), (-1.0, '-1'), (NAN, 'NaN')):
        sc = Scene(T, f'level {tag} for a player and for the ball', 'levels', slot=16)
        sc.know(12, 0.0, 10.5).know_ball(0.0, 7.0, 0.0, 0.5)
        sc.look(players=[(lv, -1, 3, 10.0, 90, 0.5, 0, 0)], ball=(lv, 9.0, 90, 0.25, 0))
        sc.then(12, 0.0, 10.5)
        if lv == 5.0:                                                           # level >= 1 places the ball; only level 4 sets its velocity
            sc.then_ball(0.0, 9.0, 0.0, 0.5 * float(f32(0.94)), 0)
        else:
            sc.then_ball(0.0, 7.5, 0.0, 0.5 * float(f32(0.94)))
    for lv in (1, 2, 3):
        sc = Scene(T, f'ball level {lv} moves the position and keeps the velocity', 'levels', slot=17)
        sc.know_ball(5.0, 5.0, 1.0, 0.0).look(ball=(lv, 2.0, 90, 0.75, 3.0)).then_ball(0.0, 2.0, float(f32(0.94)), 0.0, 0)
    sc = Scene(T, 'ball level 4 sets the velocity', 'levels', slot=18)
    sc.know_ball(5.0, 5.0, 1.0, 0.0).look(x=1.0, y=2.0, vx=0.125, vy=0.25, ball=(4, 4.0, 90, -0.25, 0)).then_ball(1.0, 6.0, 0.125, 0.0, 0)
    sc = Scene(T, 'level 4 with dist = 0: where the agent is, moving as the agent does', 'levels', slot=19)
    sc.look(x=1.0, y=2.0, vx=0.125, vy=0.25, ball=(4, 0.0, 0, 0.5, 3.0), players=[(4, 1, 4, 0.0, 0, 0.75, 9.0, 15)])
    sc.then_ball(1.0, 2.0, 0.125, 0.25, 0).then(3, 1.0, 2.0, 0.125, 0.25, 15.0, (0, 0, 0))
    # ---- ghosts
    sc = Scene(T, 'an entry exactly at the agent (d = 0) is kept; straight ahead it is forgotten', 'ghosts', near=True, slot=20)
    sc.know(2, 1.0, 2.0).know(3, 2.0, 2.0).look(x=1.0, y=2.0, width=3).then(2, 1.0, 2.0)
    sc = Scene(T, 'an entry exactly on the cone is forgotten', 'ghosts', prm='cone45', near=True, slot=21)
    sc.know(0, 5.0, 5.0).know(1, 5.0, -5.0).know(2, 0.0, 5.0).look(width=2).then(2, 0.0, 5.0)
    sc = Scene(T, 'the next float outside the cone is kept', 'ghosts', prm='cone45', near=True, slot=1)
    sc.know(0, 5.0, 5.0).know(1, 5.0, -5.0).look(width=2, face=-2.0 ** -17).then(0, 5.0, 5.0)       # 45 + 2^-17 > 45 > 45 - 2^-17
    sc = Scene(T, 'exactly on a cone of 90 degrees', 'ghosts', prm='cone45', near=True, slot=2)
    sc.know(0, 0.0, 5.0).know(1, 0.0, -5.0).know(2, -1.0, 5.0).look(width=3).then(2, -1.0, 5.0)
    for zero, tag in ((0.0, '+180'), (-0.0, '-180')):
        sc = Scene(T, f'directly behind at {tag}: outside any cone below 180', 'ghosts', slot=3)
        sc.know(5, -5.0, zero, vy=zero).look(width=3).then(5, -5.0, zero, vy=zero)                   # (-0 + -0 = -0: atan2_deg = -180)
        sc = Scene(T, f'directly behind at {tag}: on a cone of exactly 180', 'ghosts', prm='full', near=True, slot=4)
        sc.know(5, -5.0, zero, vy=zero).look(width=3)
    for code, tag, gone in ((1, '1', ()), (2, '2', (0,)), (3, '3', (0, 1)), (0, '0', (0,)), (7, '7', (0,)), (NAN, 'NaN', (0,))):
        sc = Scene(T, f'view code {tag}', 'ghosts', slot=5)                      # cones 25 / 55 / 85: bearings 45, 59.04 and 90
        sc.know(0, 5.0, 5.0).know(1, 3.0, 5.0).know(2, 0.0, 5.0).look(width=code)
        for j, (x, y) in enumerate(((5.0, 5.0), (3.0, 5.0), (0.0, 5.0))):
            if j not in gone:
                sc.then(j, x, y)
    sc = Scene(T, 'view_angle < 2 ghost_margin: a negative cone forgets nobody', 'ghosts', prm='negcone', slot=6)
    sc.know(0, 5.0, 0.0).know_ball(4.0, 0.0).look(width=2).then(0, 5.0, 0.0).then_ball(4.0, 0.0)
    sc = Scene(T, 'the ball as a ghost', 'ghosts', slot=7)
    sc.know_ball(5.0, 0.0, 1.0, 0.5).know(0, 0.0, 5.0).look().then(0, 0.0, 5.0)
    # ---- counts
    for prm in ('cm1', 'cm2', 'other', 'cm24'):
        cm = count_max(prm)
        old = lambda c: c + 1.0 if c + 1.0 < cm else cm                         # noqa: E731  (the header's words for a count)
        pd = 0.25 if prm == 'other' else float(f32(0.4))
        sc = Scene(T, f'count_max {cm:g}: NaN, negative, 2.5, above count_max, 2^24 and count_max - 1', 'counts', prm=prm, slot=8)
        given = [(0, 0, 0), (NAN, 0, 0), (0, NAN, NAN), (-3, -1, 0), (2.5, 0.5, 1.5), (0, 3.0e7, cm + 2), (LIMIT, LIMIT, LIMIT),
                 (cm - 1, 0, 0), (cm, 0, 0), (0, cm - 1, cm)]
        for j, c in enumerate(given):
            sc.know(j, 1.0, 10.0 + j, 0.5, 0.0, 20.0, c)
            if not (c[0] + 1.0 < cm):                                           # too old to keep (NaN too): the canonical unknown entry
                continue
            sc.then(j, 1.5, 10.0 + j, 0.5 * pd, 0.0, 20.0, tuple(cm if c1 != c1 else old(c1) for c1 in c))
        sc.know_ball(1.0, 10.0, 0.0, 0.0, cm - 2).look(fresh=0).then_ball(1.0, 10.0, 0.0, 0.0, cm - 1)
    sc = Scene(T, 'count_max 1: only what this very update saw is known', 'counts', prm='cm1', slot=9)
    sc.know(3, 0.0, 10.0, counts=(0, 0, 0)).look(players=[(4, 1, 2, 6.0, 90, 0, 0, 0), (2, 0, 0, 10.0, 90, 0, 0, 0)], ball=(1, 2.0, 90, 0, 0))
    sc.then(1, 0.0, 6.0, counts=(0, 0, 0)).then_ball(0.0, 2.0, 0.0, 0.0, 0)                       # (u = 9: unum 2 is row 1)
    sc = Scene(T, 'count_max 2^24: a count of 2^24 - 2 still ages', 'counts', prm='cm24', slot=10)
    sc.know(3, 0.0, 10.0, counts=(LIMIT - 2, LIMIT - 3, 5)).look(fresh=0).then(3, 0.0, 10.0, counts=(LIMIT - 1, LIMIT - 2, 6))
    sc = Scene(T, 'the rows s2d_match_belief_reset leaves: the limit becomes count_max', 'counts', prm='other', slot=11)
    sc.prior = B.unknown(1, 1)[0, 0]
    sc.look(fresh=0)
    # ---- non-finite memory: predicted as the header says, never a match candidate when q is NaN
    sc = Scene(T, 'NaN, -inf, inf - inf and -0 in a known entry', 'non-finite', slot=12)
    sc.know(0, NAN, 10.0, 1.0, 0.0).know(1, -INF, 10.0, 1.0, 0.0).know(2, INF, 10.0, -INF, 0.0).know(3, -0.0, 12.0, -0.0, -0.0)
    sc.know(4, 0.0, 10.5, NAN, 0.5)
    sc.look(players=[(2, 0, 0, 10.0, 90, 0, 0, 0)])
    p4 = float(f32(0.4))
    sc.then(0, NAN, 10.0, p4, 0.0).then(1, -INF, 10.0, p4, 0.0).then(2, NAN, 10.0, -INF, 0.0).then(3, -0.0, 12.0, -0.0, -0.0)
    sc.then(4, NAN, 11.0, NAN, 0.5 * p4)                                        # x + NaN = NaN: no candidate either; row 3 is (q = 4 < 16)
    sc.want[1 + 3] = (0.0, 10.0, -0.0, -0.0, 0.0, 0, 3, 3)
    sc = Scene(T, 'only NaN candidates: the sighting is dropped', 'non-finite', slot=13)
    sc.know(0, NAN, 10.0).know(1, 0.0, NAN).look(players=[(2, 0, 0, 10.0, 90, 0, 0, 0)]).then(0, NAN, 10.0).then(1, 0.0, NAN)
    # ---- the reset byte
    for byte in (0, 1, 2, 255):
        sc = Scene(T, f'reset byte {byte}', 'reset flag', flag=byte, slot=14)
        sc.know(0, 0.0, 10.0).know(16, 0.0, 9.0).know_ball(0.0, 4.0)
        sc.look(players=[(4, -1, 7, 8.0, 90, 0, 0, 0), (3, 1, 0, 10.5, 90, 0, 0, 0)])
        sc.then(16, 0.0, 8.0, counts=(0, 0, 0))                                 # the reset comes first: this row is still taken in
        if byte == 0:
            sc.then(0, 0.0, 10.5, counts=(0, 3, 3)).then_ball(0.0, 4.0)
    return T


def pack(scenes):
    """the scenes of ONE parameter set as matches of 22 rows: a scene for slot s sits in row s, scenes of one match share the reset
    byte, free rows are blank (an all-zero see row over an unknown belief).  Returns (belief [n, 22, 192], see [n, 22, 192],
    reset uint8 [n], where: (match, row) per scene)"""
    assert len({s.prm for s in scenes}) == 1
    cm = f32(scenes[0].cm)
    matches, where = [], []                               # matches: [flag, {slot: scene}]
    for s in scenes:
        for m, (flag, rows) in enumerate(matches):
            if flag == s.flag and s.slot not in rows:
                rows[s.slot] = s
                where.append((m, s.slot))
                break
        else:
            matches.append((s.flag, {s.slot: s}))
            where.append((len(matches) - 1, s.slot))
    n = len(matches)
    bel, see = B.unknown(n, 22, cm), np.zeros((n, 22, 192), dtype=f32)
    for m, (_flag, rows) in enumerate(matches):
        for slot, s in rows.items():
            bel[m, slot], see[m, slot] = s.prior, s.see
    return bel, see, np.array([flag for flag, _ in matches], dtype=np.uint8), where


def same_row(got, want):
    """NaN matches NaN, otherwise bit for bit (tests/test_gpu_learn.same's rule): the indices of the words that differ"""
    got, want = np.asarray(got, dtype=f32), np.asarray(want, dtype=f32)
    gn, wn = np.isnan(got), np.isnan(want)
    return np.flatnonzero((gn != wn) | (~gn & ~wn & (got.view(np.int32) != want.view(np.int32))))
