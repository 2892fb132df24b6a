"""The 11v11 match oracle's fp32 spec build against its fp64 libm build (CPU; the kernel reproduces the fp32 build bit for bit, so a
numeric mistake the two share is caught here, not by the parity tests).

* whole trajectories of the random policy (few touches of the ball: the builds stay together);
* one cycle from shared states (real play is chaotic: a corpus of checkpoints of fp32 runs, the rule scenarios of
  tests/test_match_oracle.py played forward, and constructed edge states), compared by the rule of tests/match_f64.py;
* coverage of that corpus (events and GameModeTypes), the full-state load round trip, the fp32 spec's reciprocals."""
import inspect
import os
import re

import numpy as np
import pytest

import match_f64 as F
import match_oracle as MO
import scripted_policy as SP
from soccer2d_amd import _capi_match as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the largest fraction of ill-conditioned envs accepted in one checkpoint (one compared batch) per part of the corpus.  Measured,
# largest checkpoint / whole part: play 0 / 0 of 59 552, scenarios 0.047 / 0.0088 of 200 372, edges 0.076 / 0.062 of 1 650.
# play: at most one match of a 32-match checkpoint.
ILL_CAP = {'play': 0.035, 'scenarios': 0.10, 'edges': 0.15}


def _pt_cfg(**kw):
    """oracle config; hetero_seed draws the generated player types (the table is input data)"""
    hetero = kw.pop('hetero_seed', None)
    cfg = MO.make_match_config(**kw)
    if hetero is not None:
        from soccer2d_amd.match import make_match_config
        dev = make_match_config(hetero_seed=hetero, player_type_id=kw.get('player_type_id'),
                                server_params=kw.get('server'), **{k: v for k, v in kw.items()
                                                                   if k not in ('player_type_id', 'server', 'noise', 'seed')})
        for t in range(M.MATCH_PLAYER_TYPES):
            cfg.player_types[t] = dev.player_types[t]
    return cfg


def _random_params(seed):
    """seeded like tests/test_gpu_match.py::test_match_random_parameters_parity: kick_power_rate != tackle_power_rate etc."""
    rs = np.random.RandomState(300 + seed)
    server = dict(player_decay=float(rs.uniform(0.3, 0.6)), ball_decay=float(rs.uniform(0.9, 0.97)),
                  player_speed_max=float(rs.uniform(0.6, 1.2)), player_accel_max=float(rs.uniform(0.3, 1.0)),
                  ball_speed_max=float(rs.uniform(1.5, 3.0)), ball_accel_max=float(rs.uniform(1.0, 2.7)),
                  player_size=float(rs.uniform(0.25, 0.8)), ball_size=float(rs.uniform(0.05, 0.3)),
                  dash_angle_step=float(rs.choice([0.0, 1.0, 45.0])), min_dash_power=float(rs.choice([0.0, -100.0])),
                  stamina_capacity=float(rs.choice([-1.0, 20000.0, 130600.0])), collision_vel_rate=float(rs.uniform(-0.4, -0.05)))
    return dict(server=server, half_time_cycles=int(rs.randint(40, 90)), drop_ball_time=int(rs.randint(2, 30)),
                tackle_cycles=int(rs.randint(1, 6)), tackle_dist=float(rs.uniform(1.0, 3.0)),
                tackle_back_dist=float(rs.choice([0.0, 0.5])), kickable_margin=float(rs.uniform(0.5, 1.5)),
                kick_power_rate=float(rs.uniform(0.02, 0.04)), tackle_power_rate=float(rs.uniform(0.02, 0.04)),
                free_kick_distance=float(rs.uniform(3.0, 9.15)), offside_active_area_size=float(rs.uniform(1.0, 5.0)),
                use_offside=int(rs.randint(2)), catch_probability=float(rs.choice([1.0, 0.6])), catch_ban_cycle=int(rs.randint(0, 6)),
                seed=int(rs.randint(1, 2 ** 31)), hetero_seed=int(rs.randint(1, 1000)),
                player_type_id=[0] + [int(v) for v in rs.randint(0, 18, 10)] + [0] + [int(v) for v in rs.randint(0, 18, 10)])


SHORT = dict(half_time_cycles=60, nr_extra_halfs=1, extra_half_cycles=20, kick_off_wait=2, after_goal_wait=5, pen_before_setup_wait=2,
             pen_ready_wait=3, pen_taken_wait=12, pen_nr_kicks=2, pen_max_extra_kicks=2)
# (name, config, left policy, right policy, matches, cycles)
PLAY = [('scripted-scripted', dict(SHORT), 'scripted', 'scripted', 64, 300),
        ('scripted-random', dict(SHORT, half_time_cycles=40), 'scripted', 'random', 64, 240),
        ('random-random', dict(SHORT, half_time_cycles=30, nr_extra_halfs=0), 'random', 'random', 64, 160),
        ('hetero', dict(SHORT, hetero_seed=17, player_type_id=[0] + [(i % 17) + 1 for i in range(10)] + [0] + [(i * 5) % 18 for i in range(10)]),
         'scripted', 'scripted', 48, 240),
        ('illegal-defense', dict(SHORT, illegal_defense_number=2, illegal_defense_duration=3, illegal_defense_dist_x=25.0, announce_wait=3),
         'scripted', 'random', 48, 200)] + [
        (f'random-params-{s}', dict(_random_params(s), kick_off_wait=1), 'scripted', 'random' if s & 1 else 'scripted', 32, 160)
        for s in range(4)]


def _policy_actions(spl, prm, o, left, right):
    s = o.snapshot()
    a = o.random_actions()
    if 'scripted' in (left, right):
        sa = SP.actions(spl, s, prm)
        if left == 'scripted':
            a[:, :11] = sa[:, :11]
        if right == 'scripted':
            a[:, 11:] = sa[:, 11:]
    return s, a


def _check_batch(tally, source, cfg, state, actions, ids):
    ids = np.asarray(ids, dtype=np.int64)
    after, ev = F.f32_step(cfg, state, actions, ids)
    rep, fails = F.compare(cfg, state, actions, ids, after, probes=8 if source == 'edges' else F.K_PROBES)
    tally.add(source, state, rep, fails, ev, after)


def _play_corpus(tally, spl, sources=PLAY, every=3):
    for name, kw, left, right, n, T in sources:
        for noise in (0, 1):
            kw = dict(kw)
            cfg = _pt_cfg(noise=noise, **kw)
            prm = SP.params(cfg)
            o = MO.MatchOracle(cfg, n)
            ids = np.arange(n)
            for t in range(T):
                s, a = _policy_actions(spl, prm, o, left, right)
                if t % every == 0 or t < 4:
                    _check_batch(tally, 'play', cfg, s, a, ids)
                o.step(a)


# the rule scenarios of tests/test_match_oracle.py the corpus must hold (each one records at least one cycle)
RULE_SCENARIOS = ('test_penalty_shoot_out', 'test_pen_random_winner_tosses_a_coin', 'test_illegal_defense',
                  'test_intentional_foul_brings_the_victim_down_and_may_be_carded', 'test_foul_inside_the_own_penalty_area_is_a_penalty_kick',
                  'test_goalie_catch_gives_free_kick_and_bans_catching', 'test_catch_outside_the_penalty_area_is_a_fault',
                  'test_back_pass_to_the_goalie_is_an_indirect_free_kick', 'test_offside_is_called', 'test_extra_time_after_a_draw',
                  'test_half_time_and_time_over', 'test_free_kick_fault_on_a_second_touch_by_the_taker', 'test_after_goal_pause',
                  'test_before_kick_off_mode_waits_and_lets_players_move', 'test_no_goal_directly_from_an_indirect_free_kick')


def _scenario_corpus(tally):
    """every step of the scenarios of tests/test_match_oracle.py (the rules' hand-built states and cycles), recorded as the tests
    play them forward, then compared per configuration"""
    import test_match_oracle as TMO
    rec = {}
    recorded = set()
    current = [None]
    orig = MO.MatchOracle.step

    def recording(self, actions=None):
        if self.prec == 'f32':
            a = self.random_actions() if actions is None else np.ascontiguousarray(actions, dtype=np.float32)
            key = bytes(memoryview(self.cfg))
            rec.setdefault(key, (self.cfg, []))[1].append((self.snapshot(), a.copy(), self.cfg.env_id_offset + np.arange(self.n)))
            recorded.add(current[0])
            return orig(self, a)
        return orig(self, actions)
    MO.MatchOracle.step = recording
    try:
        for name, fn in sorted(vars(TMO).items()):
            if name.startswith('test_') and callable(fn):
                assert not inspect.signature(fn).parameters, f'{name} takes arguments now: replay it here explicitly'
                current[0] = name
                fn()
    finally:
        MO.MatchOracle.step = orig
    missing = set(RULE_SCENARIOS) - recorded
    assert not missing, f'rule scenarios that recorded no cycle: {sorted(missing)}'
    for cfg, items in rec.values():
        for k in range(0, len(items), 256):
            chunk = items[k:k + 256]
            state = {f: np.concatenate([c[0][f] for c in chunk]) for f in chunk[0][0]}
            _check_batch(tally, 'scenarios', cfg, state, np.concatenate([c[1] for c in chunk]), np.concatenate([c[2] for c in chunk]))


def _edge_corpus(tally):
    state, a = F.edge_states()
    for noise in (0, 1):
        cfg = MO.make_match_config(noise=noise)
        _check_batch(tally, 'edges', cfg, state, a, np.arange(len(a)))


@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    spl = SP.build(tmp_path_factory.mktemp('sp'))
    tally = F.Tally()
    _play_corpus(tally, spl)
    _scenario_corpus(tally)
    _edge_corpus(tally)
    return tally


def test_random_policy_trajectories_f32_track_f64():
    """512 matches x 400 cycles of the random policy from the reset, noise off and on: positions within 1e-3 m (as the reach-ball
    engine's test), every discrete word identical.  Measured: 2.4e-4 m (noise off), 1.5e-4 m (noise on)."""
    n, T = 512, 400
    for noise in (0, 1):
        cfg = MO.make_match_config(noise=noise, half_time_cycles=150)
        a, b = MO.MatchOracle(cfg, n, 'f32'), MO.MatchOracle(cfg, n, 'f64')
        worst = 0.0
        for t in range(T):
            a.step(None); b.step(None)
            if t % 20 == 19 or t == T - 1:
                sa, sb = a.snapshot(), b.snapshot()
                for k in F.DISCRETE + F.CLOCKS:
                    if k not in ('nearest_left', 'nearest_right'):     # (an argmin: near-ties of two distances flip it)
                        assert np.array_equal(sa[k], sb[k]), (noise, t, k)
                for f in ('x', 'y'):
                    worst = max(worst, float(np.abs(sa[f][:, :23].astype(np.float64) - sb[f][:, :23]).max()))
        assert worst <= 1e-3, (noise, worst)
        assert a.stats()[4] > 100, list(a.stats())


def test_one_cycle_from_shared_states_f32_matches_f64(corpus):
    """every compared cycle: well-conditioned envs reproduce the fp64 discrete words and stay within T_field + 2 spread"""
    assert not corpus.fails, '\n'.join(corpus.fails[:20])
    print('worst excess (ulps):', {f: round(v, 2) for f, v in corpus.worst.items()})
    print('ill-conditioned:', {k: (a, b, round(a / max(b, 1), 4)) for k, (a, b) in corpus.ill.items()}, corpus.ill_words)


def test_ill_conditioned_fraction_is_capped(corpus):
    """a systematic error must not hide as ill-conditioning: the excused envs stay a small fraction of every checkpoint (one compared
    batch: the matches of a run at one cycle, up to 256 recorded scenario cycles of one configuration, the edge states)"""
    print('largest fraction of one checkpoint:', corpus.ill_max)
    for source, cap in ILL_CAP.items():
        corpus.ill_fraction(source)                     # (asserts the source was compared)
        assert corpus.ill_max[source] <= cap, (source, corpus.ill_max[source], cap)


# the rule-reachable GameModeTypes: all but the operator's (Pause, Human, FoulPush_, FoulMultipleAttacker_, FoulBallOut_)
REACHABLE_MODES = set(range(32)) - {M.GM_PAUSE, M.GM_HUMAN, M.GM_FOUL_PUSH, M.GM_FOUL_MULTIPLE_ATTACKER, M.GM_FOUL_BALL_OUT}
MIN_EVENTS = dict(kick=2000, tackle=500, catch=30, collision=1000, goal=40)    # measured: 4147, 1233, 42, 2441, 90


def test_corpus_covers_events_and_modes(corpus):
    """the corpus cannot pass empty: enough successful kicks, tackles, catches, collisions and goals in the compared cycles, and
    every GameModeType the rules reach"""
    print('events:', corpus.events, 'modes:', sorted(corpus.modes))
    missing = REACHABLE_MODES - corpus.modes
    assert not missing, sorted(M.GM_NAMES[m] for m in missing)
    for k, v in MIN_EVENTS.items():
        assert corpus.events[k] >= v, (k, corpus.events)


def test_full_state_round_trip(tmp_path):
    """snapshot an fp32 oracle mid-match (scripted play, noise on, set plays in progress), load it into a fresh one, step both: every
    word equal for several cycles -- no field (tick included) is left out of the loader"""
    spl = SP.build(tmp_path)
    cfg = MO.make_match_config(noise=1, **dict(SHORT, half_time_cycles=50))
    prm = SP.params(cfg)
    n = 64
    a = MO.MatchOracle(cfg, n)
    for t in range(137):
        _, act = _policy_actions(spl, prm, a, 'scripted', 'scripted')
        a.step(act)
    s = a.snapshot()
    assert (s['mode'] != M.GM_PLAY_ON).sum() >= 4 and (s['tick'] != s['cycle']).any(), s['mode']
    b = MO.MatchOracle(cfg, n)
    b.load(s)
    for t in range(12):
        sa = a.snapshot()
        for k, v in b.snapshot().items():
            assert np.array_equal(v.view(np.uint8), sa[k].view(np.uint8)), (t, k)
        _, act = _policy_actions(spl, prm, a, 'scripted', 'random')
        a.step(act); b.step(act)
        assert np.array_equal(a.events(), b.events()), t


def test_divc_reciprocals_are_correctly_rounded():
    """every DIVC(x, c, ic) of the fp32 spec: ic == float32(1 / c) for a literal c; for a parameter c, the reciprocal is derived as
    (REAL)(1.0 / c) from the same parameter in mp_from_config"""
    src = open(os.path.join(ROOT, 'oracle', 's2d_match_oracle.c')).read()
    sites = re.findall(r'DIVC\(((?:[^()]|\([^()]*\))*?),\s*((?:[^,()]|\([^()]*\))+?),\s*([^,()]+?)\)', src)
    assert len(sites) == src.count('DIVC(') and sites, sites          # (every site parsed)
    for x, c, ic in sites:
        c, ic = c.strip(), ic.strip()
        lit = re.fullmatch(r'R\(([-0-9.eE+]+)\)', c)
        if lit:
            want = np.float32(1.0 / float(lit.group(1)))
            got = np.float32(float(ic.rstrip('fF')))
            assert got == want and float(ic.rstrip('fF')) == pytest.approx(1.0 / float(lit.group(1)), rel=1e-12), (c, ic)
        else:
            pc, pic = re.fullmatch(r'(?:p|t)->(\w+)', c), re.fullmatch(r'(?:p|t)->(\w+)', ic)
            assert pc and pic, (c, ic)
            derived = re.search(r'->\s*' + pic.group(1) + r'\s*=\s*(?:[^;]*\?\s*)?\(REAL\)\(1\.0\s*/\s*\w+->' + pc.group(1) + r'\)', src)
            assert derived, (c, ic)
