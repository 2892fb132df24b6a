"""The two reflections of tests/match_symmetry.py on the CPU oracles of the 11v11 match.  No reference is needed: the run from the
reflected state with the reflected commands must be the reflection of the run.

* FLIP_Y (y, vy, body negated), fp32 and fp64 build, BITWISE: every non-noise scene of tests/match_scenes.py through all its cycles and
  256 scattered matches x 200 cycles of driven play with all six commands.  The pair of runs is re-paired only where PLACEMENTS says the
  engine writes an absolute y per slot (and at a reset by mask), decided from the first run alone; there it may differ in x, y, body of
  the placed slots and in nothing else.
  The fp64 build of the match oracle takes the quadrant out of sincos_deg first (S2DO_SINCOS_QUADRANT, oracle/s2d_oracle_common.h):
  with libm alone sin(180 deg) is 1.22e-16 with one sign, and a back dash straight behind (back_dash) missed the reflection by
  2.9e-17 in vy.
* SWAP_X (teams exchanged, x mirrored), fp64 build, one cycle from shared states: every cycle of every non-noise scene's fp32
  trajectory and of the driven play; discrete words equal, continuous words within 1e-9 * max(1, |value|).  A match-cycle leaves the
  comparison only through a row of ORDER_RULES, as ill-conditioned (the fp64 step does not reproduce the fp32 trajectory's discrete
  words) or as a nearest_* tie; the last two are capped.
* Every row of PLACEMENTS and of ORDER_RULES is needed: without it the comparison fails in the scene the row names.
* The counts of profiles/r19/match_symmetry.md are the ones measured here."""
import os

import numpy as np
import pytest

import match_oracle as MO
import match_scenes as MS
import match_symmetry as SY
from soccer2d_amd import _capi_match as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, 'profiles', 'r19', 'match_symmetry.md')
SCENES = [s for s in MS.SCENES if not s.cfg.get('noise')]          # noise draws are polar and keyed by slot: out of scope
DRIVEN_N, DRIVEN_T = 256, 200
EXCUSED_CAP = 0.02            # ill-conditioned states plus ties (nearest_*, contact chains), of the compared match-cycles of a transform


# ------------------------------------------------------------------ transforms
def _random_full_state(rng, n):
    s = MO.MatchOracle(MO.make_match_config(), n).snapshot()
    for k, v in s.items():
        if v.dtype == np.float32:
            v[...] = rng.uniform(-50, 50, v.shape).astype(np.float32)
            v[rng.random(v.shape) < 0.1] = 0.0
        elif k == 'done':
            v[...] = rng.integers(0, 2, v.shape)
        else:
            v[...] = rng.integers(0, 6, v.shape)
    s['body'][:, :22] = (rng.integers(1, 179 * 65536, (n, 22)) * rng.choice([-1, 1], (n, 22)) / SY.GRID).astype(np.float32)
    s['body'][0, :4] = (0.0, 180.0, 90.0, -90.0)
    s['mode'][:] = rng.integers(0, 32, n)
    for k in ('mode_side', 'last_touch_side'):
        s[k][:] = rng.integers(0, 3, n)
    s['offside_mask'][:] = rng.integers(0, 1 << 22, n)
    s['setplay_timer'][:] = rng.integers(0, 1 << 16, n)
    for k in ('ball_holder', 'last_kicker'):
        s[k][:] = rng.integers(0, 23, n) | (rng.integers(0, 2, n) << 8)
    s['set_play_taker'][:] = rng.integers(0, 23, n) | (rng.integers(0, 2, n) << 8) | (rng.integers(0, 1 << 18, n) << 12)
    s['nearest_left'][:] = rng.integers(0, 11, n); s['nearest_right'][:] = rng.integers(11, 22, n)
    return s


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(SY.bits(a), SY.bits(b))


@pytest.mark.parametrize('t', [SY.flip_y, SY.swap_x], ids=['flip_y', 'swap_x'])
def test_transform_twice_is_the_identity(t):
    rng = np.random.default_rng(19)
    s = SY.snap_bodies(_random_full_state(rng, 64))
    once = t(s)
    assert any(not _bits_equal(once[k], s[k]) for k in s)
    twice = t(once)
    assert sorted(twice) == sorted(s) == sorted(MO.STATE_FIELDS)
    for k in s:
        assert _bits_equal(twice[k], s[k]), k
    a = np.zeros((5, 64, 22, 3), np.float32)
    a[..., 0] = rng.integers(0, 7, a.shape[:-1]); a[..., 1:] = rng.uniform(-180, 180, a.shape[:-1] + (2,))
    assert _bits_equal(t(t(a)), a) and not _bits_equal(t(a), a)
    foul = a[..., 0] == M.MCMD_TACKLE
    assert _bits_equal(SY.flip_y(a)[..., 2][foul], a[..., 2][foul])             # Tackle's foul flag is not an angle
    cfg = SY.driven_config(max_catch_angle=70.0, min_catch_angle=-40.0)
    assert bytes(memoryview(t(t(cfg)))) == bytes(memoryview(cfg)) and bytes(memoryview(t(cfg))) != bytes(memoryview(cfg))
    rec = dict(obs=rng.uniform(-50, 50, (3, 4, 24, 5)).astype(np.float32), mode=rng.integers(0, 32, (3, 4)).astype(np.int32),
               reward=rng.choice([-1.0, 0.0, 1.0], (3, 4)).astype(np.float32), done=rng.integers(0, 2, (3, 4)).astype(np.uint8), actions=a[:3, :4])
    rec['obs'][..., :22, 4] = SY.snap_bodies(dict(body=rec['obs'][..., :22, 4]))['body']
    back = t(t(rec))
    for k in rec:
        assert _bits_equal(back[k], rec[k]), k
    st = rng.integers(0, 1000, (8,))
    assert np.array_equal(t(t(st, 'stats'), 'stats'), st)


def test_swap_x_moves_every_side_word():
    s = MO.MatchOracle(MO.make_match_config(), 1).snapshot()
    s['mode'][:] = M.GM_PENALTY_READY; s['mode_side'][:] = 1; s['score_left'][:] = 3; s['last_touch_side'][:] = 2
    s['set_play_taker'][:] = MS.pen_word(10, (2, 1), (1, 0)) | (1 << 28); s['ball_holder'][:] = 1; s['last_kicker'][:] = 14 | 0x100
    s['offside_mask'][:] = 1 << 10; s['nearest_left'][:] = 4; s['nearest_right'][:] = 20; s['reward_left'][:] = 1.0
    s['setplay_timer'][:] = 3 | (7 << 8)
    w = SY.swap_x(s)
    assert w['mode_side'][0] == 2 and w['score_right'][0] == 3 and w['score_left'][0] == 0 and w['last_touch_side'][0] == 1
    assert w['set_play_taker'][0] == MS.pen_word(21, (1, 2), (0, 1)) | (2 << 28)
    assert w['ball_holder'][0] == 12 and w['last_kicker'][0] == (3 | 0x100) and w['offside_mask'][0] == 1 << 21
    assert w['nearest_right'][0] == 15 and w['nearest_left'][0] == 9 and w['reward_left'][0] == -1.0
    assert w['setplay_timer'][0] == (3 | (7 << 8))                              # a timer outside PlayOn
    s['mode'][:] = M.GM_PLAY_ON
    assert SY.swap_x(s)['setplay_timer'][0] == (7 | (3 << 8))                   # the two illegal-defense counters in PlayOn
    assert w['x'][0, 21] == np.float32(0.4) and w['body'][0, 11] == 180.0 and w['body'][0, 0] == 0.0 and w['y'][0, 12] == s['y'][0, 1]


# ------------------------------------------------------------------ FLIP_Y: pairs of runs
class Pair:
    """an oracle and a second one that runs its reflection; counts what was compared and re-paired"""

    def __init__(self, o1, prec, rows=None):
        self.o1, self.prec, self.rows = o1, prec, rows
        self.o2 = MO.MatchOracle(SY.flip_y(o1.cfg), o1.n, prec)
        self.fails, self.compared, self.repaired = [], 0, 0
        self.repair()

    def repair(self):
        s = self.o1.snapshot()
        if self.prec == 'f64':                       # (a state goes in as fp32: both runs continue from the rounded one)
            self.o1.load(s)
            s = self.o1.snapshot()
        self.o2.load(SY.flip_y(s))

    def reset(self, mask):
        self.o1.reset(mask); self.o2.reset(mask)
        self.repair()                                # a reset by mask is a placement

    def step(self, a, tag):
        before = self.o1.snapshot()
        self.o1.step(a); self.o2.step(SY.flip_y(a))
        after = self.o1.snapshot()
        f, rp = SY.flip_y_cycle(before, after, self.o2.snapshot(), self.o1.cfg, self.rows)
        assert list(self.o1.stats()) == list(self.o2.stats()), tag
        self.fails += [f'{tag} {m}' for m in f]
        self.compared += self.o1.n
        if rp.any():
            self.repaired += int(rp.sum())
            self.repair()


def run_scene_pair(sc, prec, rows=None, stop_at=20):
    p = Pair(MS.make_oracle(sc, prec), prec, rows)
    acts = MS.scene_actions(sc)
    for t in range(sc.T):
        mask = MS.reset_mask(sc, t)
        if mask is not None:
            p.reset(None if mask.all() else mask)
        p.step(p.o1.random_actions() if acts is None else acts[t], f'{sc.name} [{prec}] cycle {t}')
        if len(p.fails) >= stop_at:
            break
    return p


def run_driven_pair(prec, cfg=None, n=DRIVEN_N, T=DRIVEN_T, mirror_cfg=True):
    cfg = SY.driven_config() if cfg is None else cfg
    o = MO.MatchOracle(cfg, n, prec)
    o.load(SY.scattered_state(cfg, n, 1905))
    p = Pair(o, prec)
    if not mirror_cfg:                               # (the second run on the first's configuration: see the limits test)
        p.o2 = MO.MatchOracle(cfg, n, prec)
        p.repair()
    rs = np.random.RandomState(7)
    seen = set()
    for t in range(T):
        a = SY.driven_commands(rs, o.snapshot(), n)
        seen |= set(np.unique(a[:, :, 0]).astype(int).tolist())
        p.step(a, f'driven [{prec}] cycle {t}')
        if len(p.fails) >= 20:
            break
    assert seen == set(range(7))
    return p


FLIP_CASES = [(sc, prec) for prec in ('f32', 'f64') for sc in SCENES]


@pytest.fixture(scope='module')
def flip():
    """every pair of runs, once: {(scene name or 'driven', precision): Pair}"""
    out = {(sc.name, prec): run_scene_pair(sc, prec) for sc, prec in FLIP_CASES}
    out.update({('driven', prec): run_driven_pair(prec) for prec in ('f32', 'f64')})
    return out


def flip_counts_line(flip, prec):
    c = sum(p.compared for (_n, q), p in flip.items() if q == prec)
    r = sum(p.repaired for (_n, q), p in flip.items() if q == prec)
    bad = sum(bool(p.fails) for (_n, q), p in flip.items() if q == prec)
    return f'FLIP_Y [{prec}]: {c} match-cycles compared bit for bit, {r} re-paired at a placement, {bad} runs different'


@pytest.mark.parametrize('sc,prec', FLIP_CASES, ids=[f'{sc.name}-{prec}' for sc, prec in FLIP_CASES])
def test_flip_y_scene_is_bitwise(flip, sc, prec):
    """every word of every cycle, re-paired only at PLACEMENTS"""
    p = flip[(sc.name, prec)]
    assert not p.fails, '\n'.join(p.fails[:10])
    assert p.compared == sc.n * sc.T                       # every match through its last cycle


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_flip_y_driven_play_is_bitwise(flip, prec):
    p = flip[('driven', prec)]
    assert not p.fails, '\n'.join(p.fails[:10])
    st = p.o1.stats()
    print(f'driven [{prec}]: compared {p.compared}, re-paired {p.repaired}, stats {list(st)}')
    assert p.compared == DRIVEN_N * DRIVEN_T and st[4] > 1000 and st[5] > 300 and st[1] + st[2] + st[7] > 20, list(st)


def test_flip_y_mirrors_asymmetric_angle_limits():
    """limits that are not symmetric about 0 (catch angle, dash angle, turn moment) are part of the reflection: with the mirrored
    configuration the runs agree bit for bit, with the first run's own they do not"""
    cfg = SY.driven_config(min_catch_angle=-40.0, max_catch_angle=70.0,
                           server=dict(min_moment=-120.0, max_moment=150.0, min_dash_angle=-90.0, max_dash_angle=135.0))
    p = run_driven_pair('f32', cfg, n=64, T=60)
    assert not p.fails, '\n'.join(p.fails[:10])
    assert run_driven_pair('f32', cfg, n=64, T=60, mirror_cfg=False).fails


# a scene in which each row of PLACEMENTS is the only excuse of a difference
PLACEMENT_SCENES = {'kick-off formation': 'goals_and_kick_off_at_once', 'shoot-out line-up': 'penalty_setup_ready_taken',
                    'sent-off parking': 'intentional_foul_geometry_and_cards'}


@pytest.mark.parametrize('row', SY.PLACEMENTS, ids=[r.name for r in SY.PLACEMENTS])
def test_every_placement_row_is_needed(row):
    assert row.reason.strip().endswith('.') and 's2d_match_oracle.c:' in row.reason
    p = run_scene_pair(MS.by_name(PLACEMENT_SCENES[row.name]), 'f32', rows=[r for r in SY.PLACEMENTS if r is not row])
    # what the engine writes there: an absolute y, the body 180 whose reflection is -180; a parked player's y decides nearest_*
    assert p.fails and all((' y: ' in m or ' body: ' in m or ' nearest_' in m) for m in p.fails), p.fails[:5]


# ------------------------------------------------------------------ SWAP_X: one cycle from shared states
def _cat(states):
    return {k: np.concatenate([s[k] for s in states]) for k in states[0]}


def scene_cycles(sc):
    """every cycle of the scene's fp32 trajectory, stacked [T * n]: (cfg, start states, commands, next states, Philox ids)"""
    o = MS.make_oracle(sc)
    acts = MS.scene_actions(sc)
    B, A, N = [], [], []
    for t in range(sc.T):
        mask = MS.reset_mask(sc, t)
        if mask is not None:
            o.reset(None if mask.all() else mask)
        a = o.random_actions() if acts is None else acts[t]
        B.append(o.snapshot()); A.append(a)
        o.step(a)
        N.append(o.snapshot())
    return o.cfg, _cat(B), np.concatenate(A), _cat(N), np.tile(o.cfg.env_id_offset + np.arange(sc.n), sc.T)


def driven_cycles(t0, t1, _cache={}):
    """cycles t0 .. t1 - 1 of the fp32 driven play, stacked like scene_cycles"""
    if not _cache:
        cfg = SY.driven_config()
        o = MO.MatchOracle(cfg, DRIVEN_N)
        o.load(SY.scattered_state(cfg, DRIVEN_N, 1905))
        rs = np.random.RandomState(7)
        B, A, N = [], [], []
        for t in range(DRIVEN_T):
            a = SY.driven_commands(rs, o.snapshot(), DRIVEN_N)
            B.append(o.snapshot()); A.append(a)
            o.step(a)
            N.append(o.snapshot())
        _cache.update(cfg=cfg, B=B, A=A, N=N)
    c = _cache
    return c['cfg'], _cat(c['B'][t0:t1]), np.concatenate(c['A'][t0:t1]), _cat(c['N'][t0:t1]), np.tile(np.arange(DRIVEN_N), t1 - t0)


class SwapTally:
    def __init__(self):
        self.n = dict(cycles=0, compared=0, ill=0, tie=0, contact=0, rule=0, bad=0)
        self.by_rule = {r.name: 0 for r in SY.ORDER_RULES}
        self.fails, self.scenes, self.through = [], {}, [0, 0]

    def add(self, name, r, T, n):
        for k in ('compared', 'ill', 'tie', 'contact', 'rule', 'bad'):
            self.n[k] += int(r[k].sum())
        self.n['cycles'] += T * n
        for k, v in r['by_rule'].items():
            self.by_rule[k] += int((v & ~r['ill']).sum())
        self.fails += [f'{name}: {m}' for m in r['fails']]
        full = (r['compared'] | r['tie'] | r['contact']).reshape(T, n).all(axis=0)
        self.scenes[name] = (int(r['compared'].sum()), T * n, int(full.sum()), n)
        return full


@pytest.fixture(scope='module')
def swap():
    t = SwapTally()
    for sc in SCENES:
        cfg, b, a, nx, ids = scene_cycles(sc)
        full = t.add(sc.name, SY.swap_x_cycle(cfg, b, a, ids, nx), sc.T, sc.n)
        t.through[0] += int(full.sum()); t.through[1] += sc.n
    for t0 in range(0, DRIVEN_T, 25):
        cfg, b, a, nx, ids = driven_cycles(t0, t0 + 25)
        t.add(f'driven {t0}..{t0 + 24}', SY.swap_x_cycle(cfg, b, a, ids, nx), 25, DRIVEN_N)
    return t


def swap_counts_lines(t):
    """(what the rules and the corpus alone decide, what the rounding of the fp64 build has a say in)"""
    return ('SWAP_X: %d match-cycles, %d excluded by rule; scene matches compared through their last cycle: %d of %d'
            % (t.n['cycles'], t.n['rule'], t.through[0], t.through[1]),
            'SWAP_X: %(compared)d compared, %(ill)d ill-conditioned, %(tie)d nearest ties, %(contact)d contact chains, %(bad)d different' % t.n)


def test_swap_x_one_cycle_from_shared_states(swap):
    print('\n'.join(swap_counts_lines(swap)))
    print({k: v for k, v in swap.by_rule.items() if v})
    assert not swap.fails, '\n'.join(swap.fails[:20])
    assert swap.n['bad'] == 0


def test_swap_x_conditions(swap):
    n = swap.n
    assert n['compared'] + n['rule'] + n['ill'] + n['tie'] + n['contact'] + n['bad'] == n['cycles']
    assert n['ill'] + n['tie'] + n['contact'] <= EXCUSED_CAP * n['compared'], n
    whole = [name for name, (c, _tot, _f, _n) in swap.scenes.items() if c == 0]
    assert not whole, f'excluded whole: {whole}'
    assert 2 * swap.through[0] >= swap.through[1], swap.through
    assert len(swap.scenes) == len(SCENES) + DRIVEN_T // 25


@pytest.mark.parametrize('row', SY.ORDER_RULES, ids=[r.name for r in SY.ORDER_RULES])
def test_every_order_rule_shows_and_is_needed(row):
    """the (scene, match) of the row breaks the symmetry in a cycle that only this row takes out: without the row the comparison fails"""
    assert row.reason.strip().endswith('.') and 's2d_match_oracle.c:' in row.reason
    if callable(row.shows):
        assert row.shows()
        return
    name, match = row.shows
    sc = MS.by_name(name)
    cfg, b, a, nx, ids = scene_cycles(sc)
    r = SY.swap_x_cycle(cfg, b, a, ids, nx, rules=[q for q in SY.ORDER_RULES if q is not row])
    bad = r['bad'].reshape(sc.T, sc.n) & r['by_rule_all'][row.name].reshape(sc.T, sc.n)
    assert (bad.any() if match is None else bad[:, match].any()), (name, match, r['fails'][:3])
    with_row = SY.swap_x_cycle(cfg, b, a, ids, nx)
    assert not with_row['bad'].any()


def test_report_holds_the_measured_counts(swap, flip):
    """profiles/r19/match_symmetry.md states the counts this file measures: those that the rules and the corpus alone decide are
    asserted (the split between compared, ties and contact chains, and the fp64 FLIP_Y line, hang on libm's last bit and are printed)"""
    text = open(REPORT).read()
    fixed, rounding = swap_counts_lines(swap)
    lines = [flip_counts_line(flip, 'f32'), fixed] + [f'| {k} | {v} |' for k, v in swap.by_rule.items()]
    print('\n'.join(lines + [flip_counts_line(flip, 'f64'), rounding]))
    for ln in lines:
        assert ln in text, ln
    for r in SY.ORDER_RULES + SY.PLACEMENTS:
        assert r.name in text, r.name
