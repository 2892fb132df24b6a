"""The vision layer on the host: the words of include/s2d_match.h ("Vision") checked on tests/see_ref.c, the independent CPU
restatement the device is compared with bit for bit (tests/test_gpu_match_see.py) -- cone, felt objects, the distance grid, the
identity levels, the order of the rows, freshness, the timers and the neck -- plus the library's parameter validation, the
ctypes mirror and the VecEnv spaces.  No GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import match_see as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_BANDS = dict(unum_far_length=20.0, unum_too_far_length=20.0, team_far_length=40.0, team_too_far_length=40.0)


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return S.build(tmp_path_factory.mktemp('see_ref'))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi, _capi_match as M
    return M.bind(_capi.load_library())


def _fields():
    from soccer2d_amd import _capi_match as M
    return M.SEE_FIELDS


def _scene(n=1, others_off=True):
    """agent 0 at the origin facing +x; with others_off everybody else is sent off (unseen) until a test places him"""
    s = S.blank_state(n)
    if others_off:
        s['card'][:, 1:22] = 2
    s['x'][:, 22], s['y'][:, 22] = -50.0, 30.0            # the ball far behind the agent
    return s


def _place(s, j, dist, ang_deg, e=0):
    s['card'][e, j] = 0
    s['x'][e, j] = np.float32(dist * math.cos(math.radians(ang_deg)))
    s['y'][e, j] = np.float32(dist * math.sin(math.radians(ang_deg)))


def _rows(o):
    """the 21 player rows of one see row"""
    return o[24:].reshape(21, 8)


@pytest.mark.parametrize('width', [1, 2, 3])
@pytest.mark.parametrize('neck', [0.0, 90.0, -90.0])
def test_cone(ref, width, neck):
    prm = S.params()
    half = prm.view_angle[width - 1] / 2
    for side in (1, -1):
        for off, seen in ((-1.0, True), (1.0, False)):
            s = _scene()
            s['neck'][0, 0], s['view_width'][0, 0], s['see_wait'][0, 0] = neck, width, prm.interval[width - 1]
            _place(s, 1, 10.0, neck + side * (half + off))
            o = S.see(ref, s, prm, 1)[0, 0]
            r = _rows(o)
            assert o[_fields()['self.fresh']] == 1 and o[_fields()['self.face']] == neck
            if seen:
                assert r[0, 0] == 4 and r[0, 1] == 1 and r[0, 2] == 2 and abs(r[0, 3] - 10.0) < 0.06
                assert r[0, 4] == round(side * (half + off))
            else:
                assert not r.any()
            assert not r[1:].any()


def test_felt_behind(ref):
    prm = S.params()
    s = _scene()
    _place(s, 12, 2.0, 180.0)
    s['vx'][0, 12] = 1.0
    s['body'][0, 12] = 45.0
    s['x'][0, 22], s['y'][0, 22] = -1.0, -1.0             # the ball too: felt, outside the 120-degree cone
    o = S.see(ref, s, prm, 1)[0, 0]
    r = _rows(o)
    assert r[0, 0] == 1 and r[0, 1] == 0 and r[0, 2] == 0            # level 1: no team, no unum
    assert abs(r[0, 3] - 2.0) < 0.05 and abs(r[0, 4]) == 180
    assert not r[0, 5:].any() and not r[1:].any()                    # no changes, no body
    assert o[16] == 1 and abs(o[17] - 1.3) < 0.01      # sqrt(2) on the grid: exp(0.3) = 1.35 -> 1.3
    assert o[18] == -135 and o[19] == 0 and o[20] == 0
    _place(s, 12, 3.5, 180.0)                                        # beyond visible_distance: gone
    assert not _rows(S.see(ref, s, prm, 1)[0, 0]).any()


def test_distance_grid(ref):
    prm = S.params()
    rng = np.random.default_rng(20)
    d = np.exp(rng.uniform(math.log(0.5), math.log(120.0), 400)).astype(np.float32)
    d64 = d.astype(np.float64)
    a = np.log(d64) / 0.1
    b = np.exp(np.round(a) * 0.1) / 0.1
    want = np.round(b) * 0.1
    near = lambda v: np.abs(v - np.floor(v) - 0.5) <= 1e-4
    keep = ~(near(a) | near(b))
    assert (~keep).mean() <= 0.02
    got = S.dist_grid(ref, prm, d).astype(np.float64)
    # fp32 rounding of the product k * 0.1: the float of 0.1 is off by 1.5e-8 relative (a quarter of an ulp), the product rounds
    # once (half an ulp)
    ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
    bad = np.abs(got - want)[keep] > ulp[keep]
    assert not bad.any(), (d[keep][bad][:5], got[keep][bad][:5], want[keep][bad][:5])
    # and the same words arrive in a row
    s = _scene(len(d))
    for e in range(len(d)):
        _place(s, 1, 1.0, 0.0, e)
    s['x'][:, 1] = d
    o = S.see(ref, s, prm, 1)
    assert np.array_equal(o[:, 0, 24 + 3], S.dist_grid(ref, prm, d))


def _arc(n, dist, ticks):
    """n matches: agent 0 with the wide view, the other 21 on an arc at `dist` in front of him"""
    s = _scene(n)
    s['view_width'][:, 0], s['see_wait'][:, 0] = 3, 3
    for j in range(1, 22):
        for_all = math.radians(-80.0 + 8.0 * (j - 1))
        s['card'][:, j] = 0
        s['x'][:, j], s['y'][:, j] = np.float32(dist * math.cos(for_all)), np.float32(dist * math.sin(for_all))
    s['tick'][:] = ticks
    return s


def test_levels_outside_the_bands(ref):
    prm = S.params()
    for dist, level in ((10.0, 4), (19.9, 4), (40.0, 3), (60.5, 2), (90.0, 2)):
        s = _arc(50, dist, np.arange(50))
        if dist == 40.0:                                  # exactly on the edge: on the x axis (the arc's roots are not exact)
            s['x'][:, 1:22], s['y'][:, 1:22] = 40.0, 0.0
        r = S.see(ref, s, prm, 1)[:, 0, 24:].reshape(50, 21, 8)
        assert (r[..., 0] == level).all(), dist
        assert ((r[..., 1] != 0) == (level >= 3)).all() and ((r[..., 2] != 0) == (level == 4)).all()
    # without bands (far == too_far) every level is a function of the distance alone
    prm = S.params(**NO_BANDS)
    for dist, level in ((15.0, 4), (30.0, 3), (50.0, 2)):
        assert (S.see(ref, _arc(8, dist, np.arange(8)), prm, 1)[:, 0, 24::8] == level).all()


@pytest.mark.parametrize('dist,kept,lost,p', [(30.0, 4, 3, 0.5), (25.0, 4, 3, 0.75), (50.0, 3, 2, 0.5), (55.0, 3, 2, 0.25)])
def test_levels_inside_the_bands(ref, dist, kept, lost, p):
    """the header's linear probability: keep with 1 - (d - far) / (too_far - far)"""
    prm = S.params(seed=77)
    n = 1000
    lv = S.see(ref, _arc(n, dist, 3 + 7 * np.arange(n)), prm, 1)[:, 0, 24::8]
    draws = lv.size
    assert draws >= 20000 and set(np.unique(lv)) == {kept, lost}
    k = int((lv == kept).sum())
    assert abs(k - draws * p) <= 5.0 * math.sqrt(draws * p * (1.0 - p)), (k, draws * p)
    # a pure function of the tick: the same ticks give the same identities, other ticks other ones
    again = S.see(ref, _arc(n, dist, 3 + 7 * np.arange(n)), prm, 1)[:, 0, 24::8]
    other = S.see(ref, _arc(n, dist, 4 + 7 * np.arange(n)), prm, 1)[:, 0, 24::8]
    assert np.array_equal(lv, again) and not np.array_equal(lv, other)


def test_order_and_zero_rows(ref):
    prm = S.params(view_angle=(60.0, 120.0, 180.0))
    s = _scene()
    s['view_width'][0, 0], s['see_wait'][0, 0] = 3, 3
    place = {5: (10.0, 40.0), 14: (10.0, -40.0), 3: (5.0, 0.0), 16: (12.0, 0.0), 9: (12.0, 0.0), 2: (12.0, 0.0), 20: (2.0, 170.0)}
    for j, (dist, ang) in place.items():
        _place(s, j, dist, ang)
    r = _rows(S.see(ref, s, prm, 1)[0, 0])
    # left to right: -40 (slot 14), then dir 0: the nearer first, the three at one place by slot; +40; the felt one at 170
    want = [(14, -40), (3, 0), (2, 0), (9, 0), (16, 0), (5, 40), (20, 170)]
    assert [int(v) for v in r[:7, 4]] == [d for _, d in want]
    assert [int(v) for v in r[:6, 2]] == [j % 11 + 1 for j, _ in want[:6]]
    assert [int(v) for v in r[:7, 1]] == [-1, 1, 1, 1, -1, 1, 0] and r[6, 0] == 1
    assert (r[:7, 0] >= 1).all() and not r[7:].any()
    key = [(r[i, 4], r[i, 3]) for i in range(7)]
    assert key == sorted(key)
    # the right team's agent: its own team first among equals
    m = S.mirror(s)
    rm = _rows(S.see(ref, m, prm, 1 << 11)[0, 0])
    assert np.array_equal(rm.view(np.int32), r.view(np.int32))


def test_not_fresh_and_sent_off(ref):
    prm = S.params()
    rng = np.random.default_rng(3)
    s = S.random_state(rng, 40, prm)
    s['card'][:] = 0
    fresh = S.see(ref, s, prm)
    assert (fresh[:, :, 24] > 0).any()
    t = dict(s)
    t['see_wait'] = np.where(s['see_wait'] > 1, s['see_wait'] - 1, 0).astype(np.int32)      # nobody fresh
    o = S.see(ref, t, prm)
    assert not o[:, :, 16:21].any() and not o[:, :, 24:].any()
    keepw = [i for i in range(24) if i not in (8, 9, 16, 17, 18, 19, 20)]
    was = np.array([prm.interval[w - 1] for w in s['view_width'][:, :22].ravel()]).reshape(-1, 22) == s['see_wait'][:, :22]
    assert np.array_equal(o[:, :, keepw][was].view(np.int32), fresh[:, :, keepw][was].view(np.int32))
    assert (o[:, :, 8] == 0).all() and np.array_equal(o[:, :, 9], t['see_wait'][:, :22].astype(np.float32))
    assert np.array_equal(o[:, :, 21], np.broadcast_to(s['mode'][:, None], (40, 22)).astype(np.float32))
    # a sent-off agent: self and game words only; a sent-off player is seen by nobody
    u = dict(s)
    u['card'] = s['card'].copy()
    u['card'][:, 4] = 2
    o = S.see(ref, u, prm)
    assert not o[:, 4, 16:21].any() and not o[:, 4, 24:].any() and (o[:, 4, 15] == 2).all() and (o[:, 4, 0] == s['x'][:, 4]).all()
    seen = (o[:, :, 24::8] > 0).sum(axis=2)
    assert (seen <= 20).all()
    unums = o[:, :11, 24:].reshape(40, 11, 21, 8)
    assert not ((unums[..., 1] == 1) & (unums[..., 2] == 5)).any()     # nobody on the left sees his team-mate number 5


def _run(ref, prm, s, acts, done=None):
    """apply vision_step per entry of acts ([22][2] rows or None); returns the list of (neck, width, wait, fresh) of match 0"""
    out = []
    for i, a in enumerate(acts):
        act = None if a is None else np.broadcast_to(np.asarray(a, dtype=np.float32), (s['x'].shape[0], 22, 2))
        s = dict(s, **S.vision_step(ref, s, prm, act, None if done is None else done[i]))
        iv = np.array([prm.interval[0], prm.interval[1], prm.interval[2]])[np.clip(s['view_width'], 1, 3) - 1]
        out.append((s['neck'][0].copy(), s['view_width'][0].copy(), s['see_wait'][0].copy(), (s['see_wait'] == iv)[0]))
    return s, out


def _reset_state(n=1):
    s = S.blank_state(n)
    s['view_width'][:], s['see_wait'][:] = 2, 0
    return s


def test_timers(ref):
    prm = S.params()
    for code, every in ((1, 1), (2, 2), (3, 3)):
        first = [[0.0, code]] * 22
        _, out = _run(ref, prm, _reset_state(), [first] + [None] * 11)
        fresh = [bool(o[3][0]) for o in out]
        assert fresh == [t % every == 0 for t in range(12)], (code, fresh)
        assert all((o[1][:22] == code).all() for o in out)
    # the state after a reset is not fresh; the first step is, for everybody
    s = _reset_state()
    o = S.see(ref, dict(s, card=np.zeros((1, 24), np.int32)), prm)
    assert (o[:, :, 8] == 0).all() and not o[:, :, 24:].any()
    # a change of width: the new interval is loaded at the next expiry; a pending wait is cut to the new width's interval
    wide, narrow, keep = [[0.0, 3]] * 22, [[0.0, 1]] * 22, [[0.0, 0]] * 22
    _, out = _run(ref, prm, _reset_state(), [wide, narrow, keep, keep])
    assert [int(o[2][0]) for o in out] == [3, 1, 1, 1] and [bool(o[3][0]) for o in out] == [True, True, True, True]
    _, out = _run(ref, prm, _reset_state(), [None, wide, None, None, None, None])      # normal, asked for wide while waiting
    assert [int(o[2][0]) for o in out] == [2, 1, 3, 2, 1, 3]
    assert [bool(o[3][0]) for o in out] == [True, False, True, False, False, True]
    assert [int(o[1][0]) for o in out] == [2, 3, 3, 3, 3, 3]
    # unknown codes keep the width
    _, out = _run(ref, prm, _reset_state(), [[[0.0, c]] * 22 for c in (7.0, -1.0, 2.5, float('nan'))])
    assert all((o[1][:22] == 2).all() for o in out)
    # fresh is never ambiguous: over random actions see_wait == see_interval[width] exactly when the timer has just expired
    rng = np.random.default_rng(8)
    s = _reset_state(64)
    for _ in range(60):
        act = np.stack([rng.uniform(-200, 200, (64, 22)), rng.integers(0, 5, (64, 22))], axis=2).astype(np.float32)
        before = s['see_wait'][:, :22].copy()
        s = dict(s, **S.vision_step(ref, s, prm, act))
        iv = np.array([1, 2, 3])[s['view_width'][:, :22] - 1]
        code = act[..., 1].astype(int)
        cut = np.where((code >= 1) & (code <= 3), np.minimum(before, np.array([0, 1, 2, 3, 0])[code]), before)
        expired = np.maximum(cut - 1, 0) == 0
        assert np.array_equal(s['see_wait'][:, :22] == iv, expired)
        assert (np.abs(s['neck'][:, :22]) <= 90).all()


def test_neck_and_done(ref):
    prm = S.params()
    turn = lambda m: [[m, 0.0]] * 22
    _, out = _run(ref, prm, _reset_state(), [turn(50.0), turn(50.0), turn(-200.0), turn(float('nan')), turn(-30.0), turn(float('inf'))])
    assert [float(o[0][0]) for o in out] == [50.0, 90.0, -90.0, -90.0, -90.0, 90.0]       # -200 counts as -180; NaN as 0
    # a narrower range of moments and angles
    small = S.params(min_neck_moment=-10.0, max_neck_moment=20.0, min_neck_angle=-15.0, max_neck_angle=25.0)
    _, out = _run(ref, small, _reset_state(), [turn(90.0), turn(90.0), turn(-90.0), turn(-90.0), turn(-90.0), turn(-90.0)])
    assert [float(o[0][0]) for o in out] == [20.0, 25.0, 15.0, 5.0, -5.0, -15.0]
    # sent off: the state stands; done: reset values, then the timer runs
    s = _reset_state(2)
    s['card'][:, 3] = 2
    s['neck'][:, 3], s['view_width'][:, 3], s['see_wait'][:, 3] = 33.0, 3, 2
    done = [np.array([0, 0], np.uint8), np.array([0, 1], np.uint8)]
    acts = [[[40.0, 3.0]] * 22] * 2
    s2, out = _run(ref, prm, s, acts, done)
    assert s2['neck'][0, 3] == 33.0 and s2['view_width'][0, 3] == 3 and s2['see_wait'][0, 3] == 2
    assert s2['neck'][0, 0] == 80.0 and s2['view_width'][0, 0] == 3
    assert (s2['neck'][1, :22] == 0).all() and (s2['view_width'][1, :22] == 2).all() and (s2['see_wait'][1, :22] == 2).all()
    assert (s2['neck'][:, 22:] == 0).all() and (s2['see_wait'][:, 22:] == 0).all()        # the pad slots are left alone


def test_mirror(ref):
    prm = S.params(**NO_BANDS)
    s = S.random_state(np.random.default_rng(12), 300, prm)
    m = S.mirror(s)
    a, b = S.see(ref, s, prm), S.see(ref, m, prm)
    assert np.array_equal(a[:, :11].view(np.int32), b[:, 11:].view(np.int32))
    assert np.array_equal(a[:, 11:].view(np.int32), b[:, :11].view(np.int32))
    lv = a[:, :, 24::8]
    assert all((lv == k).any() for k in (0, 1, 2, 3, 4)) and (a[:, :, 16] == 4).any()
    # masks select rows
    for mask in (0x7FF, 0x3FF800, 0x2A5A5, 1 << 21):
        rows = [i for i in range(22) if (mask >> i) & 1]
        assert np.array_equal(S.see(ref, s, prm, mask).view(np.int32), a[:, rows].view(np.int32))


def test_validate(lib):
    from soccer2d_amd import _capi_match as M
    prm = M.S2DVisionParams()
    lib.s2d_match_vision_default_params(C.byref(prm))
    for k, v in S.DEFAULTS.items():
        got = getattr(prm, k)
        assert (tuple(got) if k in ('view_angle', 'see_interval') else got) == v, k
    assert lib.s2d_match_vision_validate(C.byref(prm)) == 0
    assert lib.s2d_match_vision_validate(None) != 0
    bad = [dict(view_angle=(0.0, 120.0, 180.0)), dict(view_angle=(60.0, 361.0, 180.0)), dict(view_angle=(60.0, 120.0, float('nan'))),
           dict(see_interval=(0.0, 2.0, 3.0)), dict(see_interval=(1.0, 2.0, -3.0)), dict(see_interval=(1.0, 2.5, 3.0)),
           dict(dist_quantize_step=0.0), dict(dist_round=-0.1), dict(dist_chg_quantize=0.0), dict(dir_chg_quantize=float('inf')),
           dict(visible_distance=float('nan')), dict(visible_distance=-1.0),
           dict(unum_far_length=41.0), dict(team_far_length=61.0), dict(team_too_far_length=float('inf')),
           dict(min_neck_moment=181.0), dict(min_neck_angle=91.0), dict(max_neck_angle=float('nan'))]
    for over in bad:
        with pytest.raises(ValueError):
            M.vision_params(lib, **over)
        assert b'' != lib.s2d_last_error()
    ok = [dict(view_angle=(45.0, 90.0, 360.0)), dict(see_interval=(2.0, 2.0, 5.0)), dict(unum_far_length=40.0), NO_BANDS,
          dict(min_neck_angle=0.0, max_neck_angle=0.0)]
    for over in ok:
        M.vision_params(lib, **over)
    with pytest.raises(ValueError):
        M.vision_params(lib, view_angle=(60.0, 120.0))
    with pytest.raises(ValueError):
        M.vision_params(lib, visible=3.0)


def test_see_fields_and_spaces():
    from soccer2d_amd import _capi_match as M
    from soccer2d_amd.match import Soccer2DMatchVecEnv
    hit = np.zeros(M.SEE_DIM, dtype=int)
    for name, ix in M.SEE_FIELDS.items():
        hit[ix] += 1
    assert (hit == 1).all()
    assert M.SEE_FIELDS['self.fresh'] == 8 and M.SEE_FIELDS['ball.level'] == 16 and M.SEE_FIELDS['players.level'] == slice(24, 192, 8)
    assert len(range(192)[M.SEE_FIELDS['players.body_rel']]) == 21
    assert sorted(M.SEE_BLOCKS.values(), key=lambda s: s.start) == [slice(0, 16), slice(16, 24), slice(24, 192)]
    assert (M.SEE_DIM, M.MATCH_ST_SEE) == (192, 8)
    for opp, agents in ((None, 22), ('scripted', 11), ('random', 11)):
        o, a = Soccer2DMatchVecEnv.spaces(opp, 'see')
        assert o.shape == (agents, 192) and a.shape == (agents, 5)
    assert Soccer2DMatchVecEnv.spaces(None, 'agent')[0].shape == (22, 224)
    assert Soccer2DMatchVecEnv.spaces(None, 'state')[1].shape == (22, 3)
    with pytest.raises(ValueError):
        Soccer2DMatchVecEnv.spaces(None, 'sight')


def test_header_constants_and_struct_sizes(tmp_path):
    from soccer2d_amd import _capi_match as M
    prog = tmp_path / 'szv.c'
    prog.write_text('#include <stdio.h>\n#include "s2d_match.h"\nint main(){printf("%zu %zu %d %d %d %d %d %d\\n",'
                    'sizeof(S2DVisionParams),sizeof(S2DMatchVision),S2D_SEE_DIM,S2D_MATCH_ST_SEE,S2D_SEE_SELF,S2D_SEE_BALL,'
                    'S2D_SEE_PLAYERS,S2D_SEE_ROW_WORDS);return 0;}\n')
    exe = tmp_path / 'szv'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(prog), '-o', str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [C.sizeof(M.S2DVisionParams), C.sizeof(M.S2DMatchVision), M.SEE_DIM, M.MATCH_ST_SEE, 0, 16, 24, 8]
    # streams 0..7 belong to the engine
    src = open(os.path.join(ROOT, 'gym-soccer-2d-env_amd', 'csrc', 's2d_match_rules.h')).read()
    assert 'S2D_ST_NET = S2D_MATCH_ST_NET' in src and M.MATCH_ST_NET == 7


def test_library_entry_points_refuse_bad_arguments(lib):
    """without a GPU: the argument checks that come before any device work"""
    from soccer2d_amd import _capi_match as M
    prm = M.vision_params(lib)
    vis = M.S2DMatchVision(16, 16, 16)
    assert lib.s2d_match_see(None, C.byref(prm), C.byref(vis), 1, 16, None) != 0
    assert lib.s2d_match_vision_step(None, C.byref(prm), C.byref(vis), None, None, None) != 0
    assert lib.s2d_match_vision_reset(None, C.byref(vis), None, None) != 0
