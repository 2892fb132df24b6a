"""CPU checks of the belief layer (include/s2d_match.h, "Belief"): hand-built see rows through the host restatement
(tests/belief_ref.c), one test per clause of the update; the refusals of both entry points through the library (they return
before any HIP call); and one closed loop -- match oracle, see restatement, belief restatement -- that holds every level-4 update
against the true position within the bound the see quantisation allows."""
import ctypes as C
import math

import numpy as np
import pytest

import belief as B

f32 = np.float32
CM = f32(1000.0)


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return B.build(tmp_path_factory.mktemp('belief_ref'))


# ---- hand-built rows -------------------------------------------------------------------------------------------------------------
def see_row(x=0.0, y=0.0, vx=0.0, vy=0.0, body=0.0, neck=0.0, width=2, fresh=1, card=0, ball=None, players=(), game=(2, 1, 7)):
    """a see row: ball = (level, dist, dir, dist_chg, dir_chg); players = rows (level, team, unum, dist, dir, dist_chg, dir_chg,
    body_rel) in the given order; face = body + neck (choose them without a wrap)"""
    s = np.zeros(192, dtype=f32)
    s[0:8] = (x, y, vx, vy, body, neck, body + neck, width)
    s[8], s[9], s[10:14], s[14], s[15] = fresh, 2, (8000, 1, 1, 130600), 0, card
    if ball is not None:
        s[16:21] = ball
    s[21:24] = game
    for r, p in enumerate(players):
        s[24 + 8 * r:32 + 8 * r] = p
    return s


def known(b, row, x, y, vx=0.0, vy=0.0, body=0.0, counts=(0, 0, 0)):
    b[24 + 8 * row:32 + 8 * row] = (x, y, vx, vy, body) + tuple(counts)


def prow(b, row):
    return b[24 + 8 * row:32 + 8 * row]


def one(ref, see, belief, slot=0, reset=None, **prm):
    """one update of one agent's row"""
    out = B.step(ref, B.params(**prm), see[None, None], belief[None, None], None if reset is None else [reset], mask=1 << slot)
    return out[0, 0]


def blank():
    return B.unknown(1, 1, CM)[0, 0]


def is_unknown(words, count=CM):
    return not words[:5].any() and (words[5:] == count).all() and not np.signbit(words[:5]).any()


# ---- the clauses -----------------------------------------------------------------------------------------------------------------
def test_prediction_decay_and_counts_while_not_fresh(ref):
    b = blank()
    b[16:21] = (1.0, 2.0, 0.5, 0.25, 3)
    known(b, 4, 10.0, -5.0, 1.0, -1.0, 30.0, (2, 5, 7))
    s = see_row(x=3.0, y=4.0, body=10.0, neck=5.0, fresh=0, game=(4, -1, 99),
                ball=(4, 5.0, 0.0, 0, 0), players=[(4, 1, 2, 6.0, 0, 0, 0, 0)])   # (a stale row's sightings must not be read)
    o = one(ref, s, b)
    assert np.array_equal(o[0:16], s[0:16]) and np.array_equal(o[21:24], s[21:24])
    assert tuple(o[16:21]) == (1.5, 2.25, f32(0.5) * f32(0.94), f32(0.25) * f32(0.94), 4)
    assert tuple(prow(o, 4)) == (11.0, -6.0, f32(0.4), -f32(0.4), 30.0, 3, 6, 8)
    for j in range(21):
        if j != 4:
            assert is_unknown(prow(o, j)), j
    # the position moves by the velocity before the decay: a second step moves by the decayed one
    o2 = one(ref, s, o)
    assert o2[16] == f32(1.5) + f32(0.5) * f32(0.94) and o2[20] == 5
    assert prow(o2, 4)[0] == f32(11.0) + f32(0.4) and prow(o2, 4)[2] == f32(0.4) * f32(0.4)


@pytest.mark.parametrize('slot', range(22))
def test_level4_identity_placement(ref, slot):
    """every identity seen at level 4 by the agent in `slot` lands in the row the header names: teammates by own index with the
    agent itself left out (the shift around self), then the opponents by unum"""
    from soccer2d_amd import _capi_match as M
    u = slot % 11
    rows = [(4, 1, n, float(n), 90, 0, 0, 10 * n) for n in range(1, 12) if n - 1 != u]
    rows += [(4, -1, n, 20.0 + n, 90, 0, 0, -10 * n) for n in range(1, 12)]
    rows = rows[::-1][:21]                                   # (any order; 21 rows is all a see row holds)
    s = see_row(width=1, players=rows)
    o = one(ref, s, blank(), slot=slot)
    side = 0 if slot < 11 else 11
    seen = set()
    for lv, team, n, dist, *_rest, brel in rows:
        other = (side if team > 0 else 11 - side) + n - 1    # the raw slot of that player
        j = B.row_of(slot, other)
        assert j == M.belief_row_of(slot, other)
        assert j == ((n - 1 if n - 1 < u else n - 2) if team > 0 else n + 9)
        w = prow(o, j)
        assert tuple(w) == (0.0, dist, 0.0, 0.0, brel, 0, 0, 0), (slot, team, n, w)
        seen.add(j)
    assert len(seen) == 21
    # a row that names the agent itself, team 0 or a unum outside 1..11 names nobody
    junk = [(4, 1, u + 1, 5.0, 90, 0, 0, 0), (4, 0, 3, 5.0, 90, 0, 0, 0), (4, -1, 12, 5.0, 90, 0, 0, 0), (4, -1, 0, 5.0, 90, 0, 0, 0),
            (4, 1, 2.5, 5.0, 90, 0, 0, 0)]
    o = one(ref, see_row(width=1, players=junk), blank(), slot=slot)
    assert all(is_unknown(prow(o, j)) for j in range(21))


def test_velocity_reconstruction(ref):
    # axis-aligned: face 0, dir 90 -> (s, c) = (1, -0) exactly
    s = see_row(x=1.0, y=2.0, vx=0.1, vy=0.2, width=1, players=[(4, -1, 3, 10.0, 90, 0.5, 2.0, 45)], ball=(4, 4.0, 90, -0.25, -1.0))
    o = one(ref, s, blank())
    vt = (f32(2.0) * f32(0.017453292519943295)) * f32(10.0)
    w = prow(o, 12)
    assert tuple(w[:2]) == (1.0, 12.0)
    assert w[2] == f32(-vt) + f32(0.1) and w[3] == f32(0.5) + f32(0.2) and w[4] == 45.0
    bvt = (f32(-1.0) * f32(0.017453292519943295)) * f32(4.0)
    assert tuple(o[16:18]) == (1.0, 6.0) and o[18] == f32(-bvt) + f32(0.1) and o[19] == f32(-0.25) + f32(0.2) and o[20] == 0
    # a general direction against float64: position and velocity of an object moving with (rvx, rvy) relative to the agent
    face, dirn, dist, vr, dchg = 20.0, 33.0, 15.0, 0.3, 1.5
    th = math.radians(face + dirn)
    s = see_row(x=-4.0, y=7.0, vx=0.05, vy=-0.1, body=30.0, neck=-10.0, width=3, players=[(4, 1, 5, dist, dirn, vr, dchg, -170)])
    w = prow(one(ref, s, blank()), 3)                       # own index 4, u = 0 -> row 3
    vt64 = math.radians(dchg) * dist
    want = (-4.0 + dist * math.cos(th), 7.0 + dist * math.sin(th), vr * math.cos(th) - vt64 * math.sin(th) + 0.05,
            vr * math.sin(th) + vt64 * math.cos(th) - 0.1)
    assert np.allclose(w[:4], want, rtol=0, atol=2e-5)
    assert w[4] == -150.0                                    # body = norm(body_rel + face)
    # dist == 0: the object is where the agent is and moves as the agent does, whatever the change words say
    s = see_row(x=1.0, y=2.0, vx=0.1, vy=0.2, width=1, players=[(4, 1, 4, 0.0, 0, 0.7, 9.0, 0)], ball=(4, 0.0, 0, 0.3, 3.0))
    o = one(ref, s, blank())
    assert tuple(prow(o, 2)[:4]) == (1.0, 2.0, f32(0.1), f32(0.2)) and tuple(o[16:20]) == (1.0, 2.0, f32(0.1), f32(0.2))
    # a felt ball (level 1) sets the position only: the velocity is the predicted one
    b = blank()
    b[16:21] = (5.0, 5.0, 1.0, 0.0, 2)
    o = one(ref, see_row(width=1, ball=(1, 2.0, 90, 0, 0)), b)
    assert tuple(o[16:21]) == (0.0, 2.0, f32(0.94), 0.0, 0)


def _two_mates():
    """teammates with own index 1 and 2 (rows 0, 1 for u = 0) known at (0, 10) and (0, 12), an opponent (row 10) at (0, 11.25);
    everything at bearing 90 of a narrow cone, so that no ghost rule touches them"""
    b = blank()
    known(b, 0, 0.0, 10.0, counts=(2, 2, 2))
    known(b, 1, 0.0, 12.0, counts=(2, 2, 2))
    known(b, 10, 0.0, 11.25, counts=(2, 2, 2))
    return b


def test_association_nearest_tie_team_updated_dropped(ref):
    # nearest within tol among the teammates (the opponent is nearer but the team word excludes it)
    o = one(ref, see_row(width=1, players=[(3, 1, 0, 11.5, 90, 0, 0, 0)]), _two_mates())
    assert tuple(prow(o, 1)) == (0.0, 11.5, 0, 0, 0, 0, 3, 3) and tuple(prow(o, 0)) == (0.0, 10.0, 0, 0, 0, 3, 3, 3)
    assert prow(o, 10)[1] == 11.25 and prow(o, 10)[5] == 3
    # without a team word (level 2, and level 1) all 21 rows are candidates
    for lv in (2, 1):
        o = one(ref, see_row(width=1, players=[(lv, 0, 0, 11.5, 90, 0, 0, 0)]), _two_mates())
        assert tuple(prow(o, 10)) == (0.0, 11.5, 0, 0, 0, 0, 3, 3) and prow(o, 1)[5] == 3 and prow(o, 0)[5] == 3
    o = one(ref, see_row(width=1, players=[(3, -1, 0, 10.0, 90, 0, 0, 0)]), _two_mates())
    assert prow(o, 10)[1] == 10.0 and prow(o, 0)[5] == 3      # theirs: only rows 10..20
    # a tie goes to the lowest row
    o = one(ref, see_row(width=1, players=[(3, 1, 0, 11.0, 90, 0, 0, 0)]), _two_mates())
    assert prow(o, 0)[1] == 11.0 and prow(o, 0)[5] == 0 and prow(o, 1)[1] == 12.0 and prow(o, 1)[5] == 3
    # an entry updated in this cycle is no candidate: by the first pass ...
    o = one(ref, see_row(width=1, players=[(3, 1, 0, 11.9, 90, 0, 0, 0), (4, 1, 3, 12.0, 90, 0, 0, 0)]), _two_mates())
    assert tuple(prow(o, 1)[[1, 5, 6]]) == (12.0, 0, 0) and tuple(prow(o, 0)[[1, 5, 6]]) == (f32(11.9), 0, 3)
    # ... or by an earlier sighting of the second pass (sequential, in row order)
    o = one(ref, see_row(width=1, players=[(3, 1, 0, 11.9, 90, 0, 0, 0), (3, 1, 0, 12.1, 90, 0, 0, 0)]), _two_mates())
    assert prow(o, 1)[1] == f32(11.9) and prow(o, 0)[1] == f32(12.1)
    # outside tol = match_dist + match_rate * dist the sighting is dropped, and it never creates an entry
    b = _two_mates()
    o = one(ref, see_row(width=1, players=[(3, 1, 0, 30.0, 90, 0, 0, 0), (2, 0, 0, 20.0, 0, 0, 0, 0)]), b)
    want = one(ref, see_row(width=1), b)
    assert np.array_equal(o, want) and sum(prow(o, j)[5] < CM for j in range(21)) == 3
    # tol grows with the distance: 5.2 m off at 30 m is inside 3 + 0.1 * 30 (and outside with match_rate = 0)
    b = blank()
    known(b, 5, 0.0, 24.8)
    s = see_row(width=1, players=[(2, 0, 0, 30.0, 90, 0, 0, 0)])
    assert prow(one(ref, s, b), 5)[1] == 30.0 and prow(one(ref, s, b, match_rate=0.0), 5)[1] == f32(24.8)
    # an unknown entry is no candidate even at distance 0 of its +0 words
    o = one(ref, see_row(width=1, players=[(2, 0, 0, 0.0, 0, 0, 0, 0)]), blank())
    assert all(is_unknown(prow(o, j)) for j in range(21))


def _at(bearing, dist=10.0):
    return f32(dist * math.cos(math.radians(bearing))), f32(dist * math.sin(math.radians(bearing)))


def test_ghosts_inside_the_cone_none_inside_the_margin(ref):
    b = blank()
    for row, bearing in enumerate((0.0, 54.0, -54.0, 57.0, -57.0, 70.0, 180.0)):   # normal view: 120 / 2 - 5 = 55
        known(b, row, *_at(bearing), counts=(1, 1, 1))
    b[16:21] = (5.0, 0.0, 0.0, 0.0, 1)
    o = one(ref, see_row(width=2), b)
    assert [bool(prow(o, j)[5] < CM) for j in range(7)] == [False, False, False, True, True, True, True]
    assert all(is_unknown(prow(o, j)) for j in range(3)) and tuple(o[16:21]) == (0, 0, 0, 0, CM)
    # the face is what counts (body + neck), the width is the see row's, and the margin is a parameter
    o = one(ref, see_row(body=40.0, neck=30.0, width=1), b)              # cone 25 around 70
    assert [bool(prow(o, j)[5] < CM) for j in range(7)] == [True, False, True, False, True, False, True] and o[20] == 2
    o = one(ref, see_row(width=3), b, ghost_margin=0.0)                  # 90
    assert [bool(prow(o, j)[5] < CM) for j in range(7)] == [False] * 6 + [True]
    # an entry seen in this cycle is kept; one at the agent's own place (d == 0) is kept; nothing is forgotten while not fresh
    o = one(ref, see_row(width=2, players=[(3, 1, 0, 10.0, 0, 0, 0, 0)], ball=(4, 5.0, 0, 0, 0)), b)
    assert prow(o, 0)[5] == 0 and o[20] == 0 and is_unknown(prow(o, 1))
    b0 = blank()
    known(b0, 2, 0.0, 0.0)
    assert prow(one(ref, see_row(width=3), b0), 2)[5] == 1
    o = one(ref, see_row(width=2, fresh=0), b)
    assert all(prow(o, j)[5] == 2 for j in range(7)) and o[20] == 2


def test_reset_flag(ref):
    b = _two_mates()
    b[16:21] = (1.0, 1.0, 0.5, 0.5, 0)
    s = see_row(width=1, players=[(4, -1, 7, 8.0, 90, 0, 0, 0), (3, 1, 0, 10.0, 90, 0, 0, 0)])
    o = one(ref, s, b, reset=1)
    assert prow(o, 16)[1] == 8.0 and prow(o, 16)[5] == 0       # the reset comes first: this cycle's row is taken in
    assert all(is_unknown(prow(o, j)) for j in range(21) if j != 16) and tuple(o[16:21]) == (0, 0, 0, 0, CM)
    assert np.array_equal(o[:16], s[:16])
    assert prow(one(ref, s, b, reset=0), 0)[5] == 0           # (without the flag the level-3 sighting finds its entry)
    # the rows s2d_match_belief_reset leaves hold the limit; one update stores count_max in its place, whatever count_max is
    r = B.reset(ref, np.full((3, 2, 192), 7.0, dtype=f32), mask=[1, 0, 1])
    assert np.array_equal(r[[0, 2]], B.unknown(2, 2)) and (r[1] == 7.0).all()
    for cm in (1000.0, 5.0):
        o = one(ref, see_row(fresh=0), r[0, 0], count_max=cm)
        assert all(is_unknown(prow(o, j), f32(cm)) for j in range(21)) and o[20] == cm


def test_sent_off_self_takes_nothing_in(ref):
    b = _two_mates()
    rows = [(4, 1, 2, 3.0, 0, 0, 0, 0), (3, 1, 0, 12.0, 90, 0, 0, 0)]
    o = one(ref, see_row(width=3, card=2, players=rows, ball=(4, 1.0, 0, 0, 0)), b)
    want = one(ref, see_row(width=3, card=2, fresh=0), b)
    want[8] = 1
    assert np.array_equal(o, want) and o[15] == 2
    assert one(ref, see_row(width=3, card=1, players=rows), b)[24 + 5] == 0   # a yellow card sees


def test_count_saturation(ref):
    b = blank()
    known(b, 0, 1.0, 1.0, 0.5, 0.0, 20.0, (0, 1, 2))
    b[16:21] = (1.0, 1.0, 0.0, 0.0, 1)
    s = see_row(fresh=0)
    o = one(ref, s, b, count_max=3.0)
    assert tuple(prow(o, 0)[5:]) == (1, 2, 3) and o[20] == 2
    assert all(is_unknown(prow(o, j), f32(3)) for j in range(1, 21))       # 1000 is above count_max 3: stored as 3
    o = one(ref, s, o, count_max=3.0)
    assert tuple(prow(o, 0)[5:]) == (2, 3, 3) and prow(o, 0)[0] != 0       # the counts saturate one by one
    assert tuple(o[16:21]) == (0, 0, 0, 0, 3)                              # the ball's pos_count reached count_max: forgotten
    o = one(ref, s, o, count_max=3.0)
    assert is_unknown(prow(o, 0), f32(3))                                  # and so is the player, canonically
    o2 = one(ref, s, o, count_max=3.0)
    assert np.array_equal(o2, o)
    # NaN counts read as unknown
    b = blank()
    known(b, 0, 1.0, 1.0, counts=(np.nan, 0, 0))
    assert is_unknown(prow(one(ref, s, b), 0))


def test_scan_is_steps(ref):
    rng = np.random.default_rng(3)
    T, n, mask = 5, 3, 0x801
    see = np.stack([np.stack([np.stack([see_row(width=1, fresh=int(rng.integers(0, 2)),
                                               players=[(4, 1, int(rng.integers(2, 12)), float(rng.integers(1, 30)), 90, 0.25, 1.0, 0)])
                                        for _ in range(2)]) for _ in range(n)]) for _ in range(T)])
    rs = (rng.random((T, n)) < 0.3).astype(np.uint8)
    b0 = B.reset(ref, np.zeros((n, 2, 192), dtype=f32))
    fin, rec = B.scan(ref, B.params(), see, b0, rs, mask)
    b = b0
    for t in range(T):
        b = B.step(ref, B.params(), see[t], b, rs[t], mask)
        assert np.array_equal(b, rec[t])
    assert np.array_equal(fin, rec[-1])


# ---- the library's refusals (before any HIP call: no GPU needed) --------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi, _capi_match as M
    return M.bind(_capi.load_library())


def test_default_parameters_and_validation(lib):
    from soccer2d_amd import _capi, _capi_match as M
    prm = M.S2DBeliefParams()
    lib.s2d_match_belief_default_params(C.byref(prm))
    got = {k: getattr(prm, k) for k in M.BELIEF_PARAM_FIELDS}
    got['view_angle'] = tuple(prm.view_angle)
    assert got == B.DEFAULTS
    assert lib.s2d_match_belief_validate(C.byref(prm)) == 0
    assert lib.s2d_match_belief_validate(None) == _capi.S2D_EINVAL
    bad = [('ball_decay', 0.0), ('ball_decay', 1.5), ('player_decay', -0.1), ('player_decay', float('nan')), ('match_dist', -1.0),
           ('match_rate', -0.5), ('match_rate', float('inf')), ('ghost_margin', -1.0), ('count_max', 0.0), ('count_max', 2.5),
           ('count_max', 2.0 ** 25), ('view_angle', (0.0, 120.0, 180.0)), ('view_angle', (60.0, 120.0, 400.0))]
    for k, v in bad:
        with pytest.raises((RuntimeError, ValueError)):
            M.belief_params(lib, **{k: v})
    for k, v in (('ball_decay', 1.0), ('player_decay', 1.0), ('match_dist', 0.0), ('ghost_margin', 0.0), ('count_max', 1.0),
                 ('count_max', 2.0 ** 24), ('view_angle', (45.0, 90.0, 360.0))):
        M.belief_params(lib, **{k: v})
    with pytest.raises(ValueError):
        M.belief_params(lib, nonsense=1.0)
    assert M.BELIEF_DIM == M.SEE_DIM == B.DIM
    words = np.zeros(192, dtype=int)
    for v in M.BELIEF_FIELDS.values():
        words[v] += 1
    assert (words == 1).all()
    assert M.BELIEF_FIELDS['players.pos_count'] == slice(29, 192, 8) and M.BELIEF_FIELDS['ball.pos_count'] == 20


def test_refusals_before_any_hip_call(lib):
    from soccer2d_amd import _capi, _capi_match as M
    prm = M.S2DBeliefParams()
    lib.s2d_match_belief_default_params(C.byref(prm))
    P = C.byref(prm)
    ALL, n, T = 0x3FFFFF, 4, 3
    state = n * 22 * 768
    SEE, BEL, OUT = 1 << 30, 2 << 30, 3 << 30              # addresses no call below dereferences: each is refused first

    def scan(prm=P, see=SEE, reset=None, belief=BEL, out=OUT, T=T, n=n, mask=ALL, word=None):
        assert lib.s2d_match_belief_scan(prm, see, reset, belief, out, T, n, mask, None) == _capi.S2D_EINVAL
        assert word is None or word in lib.s2d_last_error().decode(), lib.s2d_last_error()

    scan(prm=None, word='non-NULL'); scan(see=None, word='non-NULL'); scan(belief=None, word='non-NULL')
    scan(mask=0, word='slot_mask'); scan(mask=1 << 22, word='slot_mask'); scan(mask=0xFFFFFFFF, word='slot_mask')
    scan(see=SEE + 4, word='aligned'); scan(belief=BEL + 8, word='aligned'); scan(out=OUT + 12, word='aligned')
    scan(T=0, word='n_steps'); scan(T=-1, word='n_steps'); scan(n=0, word='n_matches'); scan(n=-5, word='n_matches')
    scan(out=BEL, word='overlaps'); scan(out=SEE, word='overlaps'); scan(out=BEL + state - 16, word='overlaps')
    scan(out=SEE + T * state - 16, word='overlaps'); scan(out=BEL - T * state + 16, word='overlaps')
    scan(belief=SEE + 16, out=None, word='overlaps')
    for k, v in (('ball_decay', 0.0), ('player_decay', 2.0), ('count_max', 0.5), ('match_dist', float('nan'))):
        q = M.S2DBeliefParams.from_buffer_copy(prm)
        setattr(q, k, v)
        scan(prm=C.byref(q))
    q = M.S2DBeliefParams.from_buffer_copy(prm)
    q.view_angle[1] = -1.0
    scan(prm=C.byref(q), word='view_angle')

    def reset(belief=BEL, n=n, mask=ALL, word=None):
        assert lib.s2d_match_belief_reset(belief, n, mask, None, None) == _capi.S2D_EINVAL
        assert word is None or word in lib.s2d_last_error().decode(), lib.s2d_last_error()

    reset(belief=None, word='NULL'); reset(belief=BEL + 4, word='aligned'); reset(n=0, word='n_matches')
    reset(mask=0, word='slot_mask'); reset(mask=1 << 22, word='slot_mask')


def test_engine_surface_needs_no_gpu_to_refuse():
    from soccer2d_amd.match import Soccer2DMatchVecEnv as Env
    osp, asp = Env.spaces(None, 'belief')
    assert osp.shape == (22, 192) and asp.shape == (22, 5)
    osp, asp = Env.spaces('scripted', 'belief')
    assert osp.shape == (11, 192) and asp.shape == (11, 5)
    with pytest.raises(ValueError, match="belief parameters need obs='belief'"):
        Env(4, obs='see', belief={'count_max': 10})


# ---- the closed loop -------------------------------------------------------------------------------------------------------------
def test_closed_loop_level4_updates_lie_within_the_quantisation_bound(ref, tmp_path_factory):
    """4 matches, 60 cycles, scripted teams, random view actions, noise on: match oracle -> see restatement -> belief restatement.
    Every entry given a level-4 update this cycle lies within

        d * (exp(0.05) - 1) + 0.05 + 0.0088 * 1.052 * d + (2e-6 * d + 1e-4)

    of the object's true position, d = the true distance.  The first three terms follow from dist_quantize_step 0.1 (the
    logarithm is rounded to 0.1: a factor of at most exp(0.05)), dist_round 0.1 (+-0.05) and whole-degree directions (half a
    degree = 0.0088 rad at the reported distance <= 1.052 d).  The last is the fp32 slack: log_spec, exp_spec, atan2_deg and
    sincos_deg are each good to a few 1e-7 relative (or radians), so a value can be rounded as if it lay that far across a grid
    point, and the result carries that error too -- below 2e-6 * d in sum; about ten roundings of coordinates below 128 m add
    at most 10 * 2^-18 < 1e-4.  A derivation, not a measurement."""
    import match_oracle as MO
    import match_see as S
    import scripted_policy as SP
    n, T = 4, 60
    cfg = MO.make_match_config(seed=21, noise=1, half_time_cycles=25, nr_extra_halfs=0, penalty_shoot_outs=0)
    orc = MO.MatchOracle(cfg, n)
    orc.reset()
    see_lib = S.build(tmp_path_factory.mktemp('see_ref'))
    sp_lib = SP.build(tmp_path_factory.mktemp('scripted'))
    sprm, vprm, bprm = SP.params(cfg), S.params(seed=cfg.seed, env_id_offset=cfg.env_id_offset), B.params()
    rng = np.random.default_rng(8)
    planes = {'neck': np.zeros((n, 24), dtype=f32), 'view_width': np.full((n, 24), 2, dtype=np.int32),
              'see_wait': np.zeros((n, 24), dtype=np.int32)}
    bel = B.reset(ref, np.zeros((n, 22, 192), dtype=f32))
    checked = checked_ball = restarts = matched = forgotten = 0
    worst = 0.0
    for t in range(T):
        orc.step(SP.actions(sp_lib, orc.snapshot(), sprm))
        st = orc.snapshot()
        done = st['done']
        restarts += int(done.sum())
        v = np.zeros((n, 22, 2), dtype=f32)
        v[..., 0] = rng.uniform(-90, 90, (n, 22))
        v[..., 1] = rng.integers(0, 4, (n, 22)) * (rng.random((n, 22)) < 0.3)
        planes = S.vision_step(see_lib, dict(st, **planes), vprm, v, done)
        see = S.see(see_lib, dict(st, **planes), vprm)
        before = bel
        bel = B.step(ref, bprm, see, bel, done)
        pc, vc = bel[:, :, 29::8], bel[:, :, 30::8]
        matched += int(((pc == 0) & (vc > 0)).sum())          # placed by a level 1-3 sighting: the second pass
        forgotten += int(((before[:, :, 29::8] < 999) & (pc == 1000) & (done[:, None, None] == 0)).sum())   # ghosts
        for e in range(n):
            for p in range(22):
                sg = 1.0 if p < 11 else -1.0
                b, s = bel[e, p], see[e, p]
                assert np.array_equal(b[:16], s[:16]) and np.array_equal(b[21:24], s[21:24])
                me = np.array([sg * float(st['x'][e, p]), sg * float(st['y'][e, p])])
                objs = [(o, 24 + 8 * B.row_of(p, o), 30 + 8 * B.row_of(p, o)) for o in range(22) if o != p]
                for o, at, vel_count in objs:
                    if b[vel_count] != 0:                    # vel_count == 0: identified (level 4) in this very cycle
                        continue
                    true = np.array([sg * float(st['x'][e, o]), sg * float(st['y'][e, o])])
                    d = float(np.hypot(*(true - me)))
                    err = float(np.hypot(*(b[at:at + 2].astype(np.float64) - true)))
                    bound = d * (math.exp(0.05) - 1) + 0.05 + 0.0088 * 1.052 * d + (2e-6 * d + 1e-4)
                    assert err <= bound, (t, e, p, o, err, bound)
                    worst = max(worst, err / bound)
                    checked += 1
                if s[16] == 4:
                    true = np.array([sg * float(st['x'][e, 22]), sg * float(st['y'][e, 22])])
                    d = float(np.hypot(*(true - me)))
                    err = float(np.hypot(*(b[16:18].astype(np.float64) - true)))
                    bound = d * (math.exp(0.05) - 1) + 0.05 + 0.0088 * 1.052 * d + (2e-6 * d + 1e-4)
                    assert err <= bound and b[20] == 0, (t, e, p, 'ball', err, bound)
                    checked_ball += 1
    assert checked > 5000 and checked_ball > 500 and restarts > 0, (checked, checked_ball, restarts)
    assert matched > 100 and forgotten > 100, (matched, forgotten)       # every step of the update took part
    known_share = (bel[:, :, 29::8] < 1000).mean()
    assert 0.2 < known_share <= 1.0, known_share
    print(f'closed loop: {checked} player and {checked_ball} ball level-4 updates, {matched} matched, {forgotten} forgotten, '
          f'worst error / bound = {worst:.3f}, '
          f'known entries at the end {known_share:.2f}')
