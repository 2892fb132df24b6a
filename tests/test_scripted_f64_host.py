"""The scripted team's host restatement (tests/scripted_policy_ref.c) against the float64 rule table of tests/scripted_f64.py, on
the CPU: the stratified corpus by the float64 rule, the ill-conditioned share per stratum, every rule fired on either side, the
committed T values re-measured, and the two reflections of the controller on the restatement.

Measured (default types / the heterogeneous configuration, 3000 matches = 66 000 rows per stratum; share of ill-conditioned rows):
    scattered 0.000 % / 0.000 %, ball at a player 0.002 % / 0.002 %, ball at a goalie 0.000 % / 0.000 %, set play 0.000 % / 0.000 %,
    shoot-out 0.000 % / 0.000 %, near home 0.002 % / 0.002 %; the GPU batch and its swap_x 0.000 %.  The cap is ILL_CAP = 1 %.
"""
import numpy as np
import pytest

import match_oracle as MO
import match_symmetry as SY
import scripted_f64 as F
import scripted_policy as SP

N_PER = 3000                      # matches per stratum and configuration
MIN_FIRED = 200                   # every rule number fires at least this often on each side, over a configuration's corpus
CONFIGS = {'default': MO.make_match_config, 'hetero': F.hetero_config}


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return SP.build(tmp_path_factory.mktemp('scripted_f64'))


_ENTRIES = {}
STRATUM_KEYS = tuple(range(len(F.STRATA)))
ALL_KEYS = STRATUM_KEYS + ('gpu batch', 'swap_x')


def _entry(ref, name, key):
    """(report, failures, state) of one corpus entry of one configuration, computed once per session: a stratum at N_PER matches,
    the GPU batch (tests/test_gpu_match_scripted_f64.py runs the same states), or its swap_x mapped back"""
    if (name, key) not in _ENTRIES:
        cfg = CONFIGS[name]()
        prm = SP.params(cfg)
        if key == 'swap_x':
            state = _snapped(cfg)
            keep = ~np.isin(state['mode'], F.SWAP_EXEMPT_MODES)
            state = {k: v[keep] for k, v in state.items()}
            got = SY.swap_x_actions(SP.actions(ref, SY.swap_x(state, 'state'), SP.params(SY.swap_x(cfg, 'config'))))
        else:
            state = F.corpus(cfg, F.GPU_N, F.GPU_SEED)[0] if key == 'gpu batch' else F.corpus(cfg, N_PER, 100 + key, strata=(key,))[0]
            got = SP.actions(ref, state, prm)
        _ENTRIES[(name, key)] = F.compare(state, prm, got) + (state,)
    return _ENTRIES[(name, key)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize('name', list(CONFIGS))
@pytest.mark.parametrize('stratum', range(len(F.STRATA)))
def test_restatement_against_float64(ref, name, stratum):
    rep, fails, _ = _entry(ref, name, stratum)
    print(f'{name}, {F.STRATA[stratum]}: ill-conditioned {rep["ill"]} / {rep["n"]} = {100 * rep["share"]:.3f} %, worst {rep["worst"]}')
    assert not fails, fails
    assert rep['share'] <= F.ILL_CAP


def test_formation_is_the_kick_off():
    s = MO.MatchOracle(MO.make_match_config(), 1).snapshot()
    # the side that kicks off stands differently around the centre spot; the defenders and the goalie stand on the formation
    assert np.array_equal(s['x'][0, 11:22], -F.FORM_X.astype(np.float32)) and np.array_equal(s['y'][0, 11:22], F.FORM_Y.astype(np.float32))


def test_bodies_and_angles_stay_in_range(ref):
    cfg = MO.make_match_config()
    state, _ = F.corpus(cfg, 600, seed=3)
    assert (np.abs(state['body'][:, :22]) <= 180.0).all() and (state['body'][:, :22] > -180.0).all()
    got = SP.actions(ref, state, SP.params(cfg))
    ang = F.angle_of(got)
    assert (ang <= 180.0).all() and (ang >= -180.0).all()


# ------------------------------------------------------------------------------------------------ reflections (host twins)
def _snapped(cfg):
    """the batch the GPU tests run (tests/test_gpu_match_scripted_f64.py), bodies snapped: what passes here passes there, the
    device being the restatement bit for bit"""
    return SY.snap_bodies(F.corpus(cfg, F.GPU_N, F.GPU_SEED)[0])


@pytest.mark.parametrize('name', list(CONFIGS))
def test_the_gpu_batch_on_the_restatement(ref, name):
    cfg = CONFIGS[name]()
    prm = SP.params(cfg)
    for n in F.GPU_SIZES[:-1]:
        state, _ = F.corpus(cfg, n, F.GPU_SEED)
        rep, fails = F.compare(state, prm, SP.actions(ref, state, prm))
        assert not fails, fails
    rep, fails, _ = _entry(ref, name, 'gpu batch')
    assert not fails, fails
    assert rep['share'] <= F.ILL_CAP


@pytest.mark.parametrize('name', list(CONFIGS))
def test_swap_x_of_the_restatement(ref, name):
    """swap_x of every corpus state through the restatement; the actions mapped back are judged by the float64 rule against the
    unswapped state's float64 answer.  The shoot-out's modes are exempt (F.SWAP_EXEMPT_MODES): they always use the right goal."""
    rep, fails, state = _entry(ref, name, 'swap_x')
    assert len(state['mode']) > 0.7 * F.GPU_N
    print(f'swap_x, {name}: ill-conditioned {100 * rep["share"]:.3f} %, worst {rep["worst"]}')
    assert not fails, fails
    assert rep['share'] <= F.ILL_CAP


def test_flip_y_of_the_restatement(ref):
    """flip_y with the slot permutation (1 4)(2 3)(5 8)(6 7)(9 10): the flipped run's record is the flipped record bit for bit
    (homogeneous types); dropped: exact chaser ties and angles of exactly +-180, at most 1 % of the batch"""
    cfg = MO.make_match_config()
    prm = SP.params(cfg)
    state = _snapped(cfg)
    a = SP.actions(ref, state, prm)
    b = SP.actions(ref, F.flip_y_state(state), prm)
    drop = F.flip_y_dropped(state, prm, a) | F.flip_y_dropped(state, prm, F.flip_y_actions(b))
    print(f'flip_y: dropped {int(drop.sum())} of {len(drop)} matches')
    assert drop.mean() <= 0.01
    want = F.flip_y_actions(a)
    bad = (_bits(b) != _bits(want)) & ~((b == 0) & (want == 0))
    bad[drop] = False
    assert not bad.any(), (np.argwhere(bad)[0], b[tuple(np.argwhere(bad)[0][:2])], want[tuple(np.argwhere(bad)[0][:2])])


def test_flip_permutation_is_the_formation_s_symmetry():
    assert np.array_equal(F.FORM_X[F.FLIP_PERM], F.FORM_X) and np.array_equal(F.FORM_Y[F.FLIP_PERM], -F.FORM_Y + 0.0)


@pytest.mark.parametrize('name', list(CONFIGS))
def test_every_rule_fired(ref, name):
    """over the six strata of one configuration: each rule number at least MIN_FIRED times on each side"""
    rules = [_entry(ref, name, s)[0]['f64']['rule'] for s in STRATUM_KEYS]
    fired = np.sum([[(int((r[:, :11] == k).sum()), int((r[:, 11:] == k).sum())) for k in range(1, 9)] for r in rules], axis=0)
    print(f'{name}: rules 1..8 fired (left, right): {fired.tolist()}')
    assert (fired >= MIN_FIRED).all(), fired.tolist()


def test_the_committed_t_is_the_measurement(ref):
    """re-measured over every entry of this module (the strata, the GPU batch, its swap_x; both configurations): the maximum of each
    kind of angle is within its committed T, and T is at most 4x that maximum"""
    worsts = [_entry(ref, name, key)[0]['worst'] for name in CONFIGS for key in ALL_KEYS]
    for kind in F.T_ULPS:
        worst = max(w[kind] for w in worsts)
        print(f'{kind}: measured {worst:.3f} ulps, T = {F.T_ULPS[kind]}')
        assert worst <= F.T_ULPS[kind] <= 4.0 * worst, (kind, worst)
