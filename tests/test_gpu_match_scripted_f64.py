"""The in-kernel scripted team (m_scripted_action) against the float64 rule table of tests/scripted_f64.py, on written states and on
states reached by play; bit for bit against the host restatement throughout.  Controller tables with only some slots scripted, fused
launches against one-cycle launches, and the two reflections of the controller.  (The host twins of the batches used here run in
tests/test_scripted_f64_host.py: the same states, the restatement in the device's place.)"""
import numpy as np
import pytest

import match_oracle as MO
import match_symmetry as SY
import scripted_f64 as F
import scripted_policy as SP
from soccer2d_amd import _capi_match as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

CONFIGS = {'default': MO.make_match_config, 'hetero': F.hetero_config}
# states reached by play: halves short enough for extra time and the shoot-out to arrive within 150 cycles, long enough for a goalie
# to get the ball into his hands (tests/test_gpu_match_obs_f64.py's SCHED, the halves longer)
PLAYED = dict(half_time_cycles=46, nr_extra_halfs=1, extra_half_cycles=8, kick_off_wait=2, after_goal_wait=3, drop_ball_time=20,
              announce_wait=4, pen_before_setup_wait=2, pen_ready_wait=3, pen_taken_wait=12, pen_nr_kicks=2, pen_max_extra_kicks=2)


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return SP.build(tmp_path_factory.mktemp('scripted_f64_gpu'))


def _held(ref, cfg, state, rec, cap, tag):
    import scripted_device as D
    prm = SP.params(cfg)
    D.assert_same_words(rec, SP.actions(ref, state, prm), tag)
    rep, fails = F.compare(state, prm, rec)
    assert not fails, (tag, fails)
    assert cap is None or rep['share'] <= cap, (tag, rep['share'])
    return rep


@pytest.mark.parametrize('name', list(CONFIGS))
@pytest.mark.parametrize('n', F.GPU_SIZES)
def test_corpus_on_the_device(ref, name, n):
    import scripted_device as D
    cfg = CONFIGS[name]()
    state, _ = F.corpus(cfg, n, F.GPU_SEED)
    eng = D.engine(cfg, n)
    D.load(eng, state)
    rec = D.cycle(eng)[0][0]
    rep = _held(ref, cfg, state, rec, F.ILL_CAP if n >= 100 else None, f'{name}, N = {n}')
    if n >= 100:
        fired = [int((rep['f64']['rule'] == r).sum()) for r in range(1, 9)]
        assert min(fired) >= 5, fired
    eng.close()


def test_states_reached_by_play(ref):
    """both teams scripted, noise on, 150 cycles of 521 matches through kick-off, play, extra time and the shoot-out: every recorded
    cycle against float64 from the state read before it"""
    import scripted_device as D
    cfg = MO.make_match_config(noise=1, seed=13, **PLAYED)
    n, T = F.GPU_N, 150
    eng = D.engine(cfg, n)
    modes, cmds, ill, rows = set(), set(), 0, 0
    for t in range(T):
        state = D.read(eng)
        rec = D.cycle(eng)[0][0]
        rep = _held(ref, cfg, state, rec, None, f'cycle {t}')
        ill, rows = ill + rep['ill'], rows + rep['n']
        modes.update(np.unique(state['mode']).tolist())
        cmds.update(np.unique(rec[..., 0]).tolist())
    print(f'played: modes {sorted(modes)}, commands {sorted(cmds)}, ill-conditioned {ill} / {rows}')
    assert ill <= F.ILL_CAP * rows
    assert {M.GM_PENALTY_READY, M.GM_PENALTY_TAKEN, M.GM_PLAY_ON, M.GM_KICK_OFF} <= modes, modes
    assert float(M.MCMD_CATCH) in cmds and {0.0, 1.0, 2.0, 3.0} <= cmds, cmds
    eng.close()


def _tables():
    rs = np.random.RandomState(17)
    out = [[2 if j == i else 1 for j in range(22)] for i in range(22)]                  # slot i scripted, the others random
    out += [[2] * 11 + [1] * 11, [1] * 11 + [2] * 11]
    out += [rs.randint(1, 3, 22).tolist() for _ in range(3)]
    return out


def test_partly_scripted_tables(ref):
    """a scripted slot's row is the all-scripted run's row bit for bit (the team search does not depend on who is scripted), and
    the random slots draw what the table-less engine draws"""
    import scripted_device as D
    cfg = F.hetero_config()
    n = 132
    state, _ = F.corpus(cfg, n, 31)
    eng = D.engine(cfg, n)

    def run(table):
        eng.set_controllers(table)
        D.load(eng, state)
        return D.cycle(eng)[0][0]
    scripted = run(D.ALL_SCRIPTED)
    D.assert_same_words(scripted, SP.actions(ref, state, SP.params(cfg)), 'all scripted')
    drawn = run(None)
    assert len(np.unique(drawn[..., 1])) > n                                             # (draws, not a constant)
    for table in _tables():
        rec = run(table)
        s = np.array(table) == 2
        D.assert_same_words(rec[:, s], scripted[:, s], f'scripted slots of {table}')
        D.assert_same_words(rec[:, ~s], drawn[:, ~s], f'random slots of {table}')
    eng.close()


@pytest.mark.parametrize('general', [False, True])
@pytest.mark.parametrize('T', [2, 33])
def test_fused_launch_is_the_one_cycle_launches(T, general, monkeypatch):
    import scripted_device as D
    if general:
        monkeypatch.setenv('S2D_MATCH_GENERAL_KERNEL', '1')
    cfg = MO.make_match_config()
    n = 9
    state, _ = F.corpus(cfg, n, 41)
    fused, single = D.engine(cfg, n), D.engine(cfg, n)
    assert ('general' in fused.kernel_name()) == general
    D.load(fused, state); D.load(single, state)
    rec = D.cycle(fused, T)[0]
    for t in range(T):
        D.assert_same_words(D.cycle(single)[0][0], rec[t], f'cycle {t} of {T}')
    a, b = D.read(fused, D.FIELDS), D.read(single, D.FIELDS)
    for k in D.FIELDS:
        if k not in ('nearest_left', 'nearest_right'):              # outputs of a launch's last cycle: the same here, but no state
            assert np.array_equal(D.bits(a[k]), D.bits(b[k])), k
    assert len(np.unique(rec[..., 0])) >= 4
    fused.close(); single.close()


# ------------------------------------------------------------------------------------------------ reflections
@pytest.mark.parametrize('name', list(CONFIGS))
def test_swap_x_on_the_device(name):
    """swap_x of every corpus state (bodies snapped) through one device cycle; the actions mapped back are judged by the float64
    rule against the unswapped state's float64 answer.  Exempt, as data: F.SWAP_EXEMPT_MODES (the shoot-out uses the right goal)"""
    import scripted_device as D
    cfg = CONFIGS[name]()
    state = SY.snap_bodies(F.corpus(cfg, F.GPU_N, F.GPU_SEED)[0])
    keep = ~np.isin(state['mode'], F.SWAP_EXEMPT_MODES)
    state = {k: v[keep] for k, v in state.items()}
    n = int(keep.sum())
    assert n > 0.7 * F.GPU_N
    eng = D.engine(SY.swap_x(cfg, 'config'), n)
    D.load(eng, SY.swap_x(state, 'state'))
    rec = SY.swap_x_actions(D.cycle(eng)[0][0])
    rep, fails = F.compare(state, SP.params(cfg), rec)
    assert not fails, fails
    assert rep['share'] <= F.ILL_CAP
    eng.close()


def test_flip_y_on_the_device():
    """flip_y with the slot permutation (1 4)(2 3)(5 8)(6 7)(9 10) under which the formation is symmetric, homogeneous types: the
    flipped run's record is the flipped record bit for bit.  Dropped: exact chaser ties and angles of exactly +-180, <= 1 %."""
    import scripted_device as D
    cfg = MO.make_match_config()
    prm = SP.params(cfg)
    state = SY.snap_bodies(F.corpus(cfg, F.GPU_N, F.GPU_SEED)[0])
    n = F.GPU_N
    eng = D.engine(cfg, n)
    D.load(eng, state)
    a = D.cycle(eng)[0][0]
    D.load(eng, F.flip_y_state(state))
    b = D.cycle(eng)[0][0]
    drop = F.flip_y_dropped(state, prm, a) | F.flip_y_dropped(state, prm, F.flip_y_actions(b))
    assert drop.mean() <= 0.01
    want = F.flip_y_actions(a)
    bad = (D.bits(b) != D.bits(want)) & ~((b == 0) & (want == 0))
    bad[drop] = False
    assert not bad.any(), np.argwhere(bad)[:4]
    eng.close()
