"""The fp32 spec of the reach-ball cycle (the fp32 build of oracle/s2d_oracle.c, which the device equals bit for
bit) against the fp64 libm build of the same oracle, one cycle from shared states, by the rule of tests/reach_f64.py.  Runs without
a GPU.  This corpus is where the T values of reach_f64.T_ULPS / RESET_T_ULPS were measured; tests/test_gpu_reach_f64.py holds the
device to the same values."""
import numpy as np
import pytest

import reach_f64 as R


@pytest.fixture(scope='module')
def corpus():
    """{case: dict(fails, ill, n, worst, reset_worst, skipped, ended)}: every case compared once, with the T values of reach_f64"""
    out = {}
    for name in R.case_names():
        kw, command, items = R.build_case(name)
        cfg = R.make_cfg(kw)
        c = dict(fails=[], ill=0, n=0, worst={}, reset_worst={}, skipped=0, ended=0, ill_words={})
        for k, (rows, a) in enumerate(items):
            g = R.f32_step(cfg, rows, a, command)
            rep, fails = R.compare(cfg, rows, a, g, command)
            c['fails'] += [f'batch {k}: {m}' for m in fails]
            c['ill'] += rep['ill']; c['n'] += rep['n']; c['ended'] += rep['ended']
            for w, v in rep['worst'].items():
                c['worst'][w] = max(c['worst'].get(w, -np.inf), v)
            for w, v in rep['ill_words'].items():
                c['ill_words'][w] = c['ill_words'].get(w, 0) + v
            if rep['reset']:
                c['skipped'] += rep['reset']['skipped']
                for w, v in rep['reset']['worst'].items():
                    c['reset_worst'][w] = max(c['reset_worst'].get(w, -np.inf), v)
        out[name] = c
    return out


@pytest.mark.parametrize('name', R.case_names())
def test_one_cycle_matches_f64(corpus, name):
    c = corpus[name]
    print(f"{name}: ill-conditioned {c['ill']} of {c['n']} ({100.0 * c['ill'] / c['n']:.3f} %) {c['ill_words']}; {c['ended']} envs ended "
          f"into a reset, {c['skipped']} of them skipped; worst excess in ulps "
          f"{ {w: round(v, 2) for w, v in c['worst'].items() if v > 0} }")
    assert not c['fails'], '\n'.join(c['fails'][:10])
    assert c['n'] >= 512 and (c['ill'] <= R.ILL_CAP * c['n'] or not R.capped(name)), (c['ill'], c['n'], c['ill_words'])
    assert c['skipped'] <= max(R.TRIES_CAP * c['ended'], 0), (c['skipped'], c['ended'])


def test_the_corpus_reaches_what_it_is_for(corpus):
    """collisions, every result label, resets inside a step, the back dash, turns and frozen envs all occur in the compared cycles"""
    assert sum(c['ended'] for c in corpus.values()) > 5000
    kw, command, items = R.build_case('commands')
    cfg = R.make_cfg(kw)
    cmds = np.concatenate([a for _, a in items])
    assert command and ((cmds[:, 0] == R.CMD_DASH) & (cmds[:, 1] < 0)).sum() > 200 and (cmds[:, 0] == R.CMD_TURN).sum() > 200
    assert (np.abs(cmds[cmds[:, 0] == R.CMD_TURN, 2]) > 180).any() and (cmds[:, 0] == R.CMD_FREEZE).sum() > 100
    seen = set()
    for name in ('written dqn-discrete16', 'written no-autoreset-collide'):
        kw, command, items = R.build_case(name)
        cfg = R.make_cfg(kw)
        for rows, a in items:
            b = R.step_from(cfg, rows, a, 'f64')
            seen |= set(np.unique(b['result']).tolist())
            vx = b['state'][:, R.IDX['player_vx']]
            if ((vx == 0) & np.signbit(vx)).any():
                seen.add('-0')
    assert seen >= {0, R.GOAL, R.OUT, R.TIMEOUT, '-0'}, seen


def test_t_values_carry_their_measurement(corpus):
    """every T is at most 4x the maximum measured on this corpus (recorded beside it), 0 where that maximum is not above 0; and the
    recorded maxima are this corpus's: no case exceeds them"""
    for T, M in ((R.T_ULPS, R.MEASURED_ULPS), (R.RESET_T_ULPS, R.RESET_MEASURED_ULPS)):
        assert set(T) == set(M)
        for w in T:
            assert T[w] <= 4.0 * max(M[w], 0.0) and (T[w] > 0 or M[w] <= 0), (w, T[w], M[w])
            assert T[w] >= M[w], (w, T[w], M[w])
    worst, rworst = {}, {}
    for c in corpus.values():
        for w, v in c['worst'].items():
            worst[w] = max(worst.get(w, -np.inf), v)
        for w, v in c['reset_worst'].items():
            rworst[w] = max(rworst.get(w, -np.inf), v)
    print('one cycle:', {w: round(v, 3) for w, v in worst.items()})
    print('resets inside a step:', {w: round(v, 3) for w, v in rworst.items()})
    for w, v in worst.items():
        assert v <= max(R.MEASURED_ULPS[w], 0.0) + 1e-3, (w, v)
    for w, v in rworst.items():
        assert v <= max(R.RESET_MEASURED_ULPS[w], 0.0) + 1e-3, (w, v)


@pytest.mark.parametrize('name', list(R.SCENE_CONFIGS))
def test_scenes_have_their_known_answers(name):
    """every constructed scene: (1) the hand-written answer is float64's, (2) the fp32 oracle gives the same discrete words (a scene
    marked ill-conditioned must be flagged by the probe instead; a dash_angle_step tie lands on the float64 grid point or a
    neighbouring one)"""
    items = [s for s in R.scenes() if s['cfg'] == name]
    assert items
    cfg, rows, a, command = R.scene_batch(name, items)
    g = R.f32_step(cfg, rows, a, command)
    rep, rule_fails = R.compare(cfg, rows, a, g, command)
    unit = R.units(cfg)
    fails = []
    for i, s in enumerate(items):
        fails += R.check_scene_f64(s, rep['f64'], i)
        if s['ill'] and not rep['ill_mask'][i]:
            fails.append(f"{s['name']}: the probe does not flag it ill-conditioned")
    assert not fails, '\n'.join(fails)
    for i, s in enumerate(items):
        fails += R.check_scene_f32(s, g, rep['f64'], i, unit)
    assert not fails, '\n'.join(fails)
    assert not rule_fails, '\n'.join(rule_fails)            # the scenes the probe leaves well-conditioned also obey the rule


def test_the_scene_table_covers_the_list():
    names = [s['name'] for s in R.scenes()]
    assert len(set(names)) == len(names)
    for group in ('goal', 'out', 'timeout', 'labels', 'collision', 'speed', 'accel', 'stamina', 'threshold', 'dash', 'turn', 'obs', 'tie'):
        assert sum(n.startswith(group + ':') for n in names) >= 2, group
    ties = [s for s in R.scenes() if 'grid' in s['expect']]
    assert {s['expect']['step'] for s in ties} == {7.5, 22.5, 45.0} and all(s['ill'] for s in ties)


@pytest.mark.parametrize('name', list(R.RESET_CONFIGS))
def test_resets_match_f64(name):
    """a reset is a function of (env id, episode): the fp32 oracle's first reset and a masked reset at scattered episode counters
    against the fp64 build's (resets inside a step are part of the one-cycle cases)"""
    cfg = R.make_cfg(R.RESET_CONFIGS[name])
    n = 8192
    for ep, mask in ((np.zeros(n, dtype=np.int64), None), R.reset_episodes(n)):
        g = R.reset_from(cfg, n, ep, 'f32', mask)
        rep, fails = R.compare_reset(cfg, n, ep, g, mask)
        print(f"{name} {'first' if mask is None else 'masked'}: {rep['n']} resets, {rep['skipped']} skipped; worst "
              f"{ {w: round(v, 2) for w, v in rep['worst'].items() if v > 0} }")
        assert not fails, '\n'.join(fails)
        assert rep['n'] > 4000 and rep['skipped'] <= R.TRIES_CAP * rep['n']
        for w, v in rep['worst'].items():
            assert v <= max(R.RESET_MEASURED_ULPS[w], 0.0) + 1e-3, (w, v)
        if mask is not None:                                # an unmasked env keeps the state it was created with
            keep = ~mask.astype(bool)
            assert (g['state'][keep, R.IDX['episode']] == ep[keep]).all() and (g['state'][keep, R.IDX['cycle']] == 0).all()
