"""Host checks of the episode statistics (no GPU): the C restatement of s2d_episode_stats (tests/episodes_ref.c, what the GPU
tests compare the device with) against an independent per-env Monitor loop; the overflow rule; InfoCollectorCallback's
on_episode_stats against on_result_codes; new_result_codes after a drop; header, binding and build list."""
import os
import re

import numpy as np
import pytest

import episodes as EP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def L(tmp_path_factory):
    return EP.build(tmp_path_factory.mktemp('episodes_ref'))


def chained(rng, T, N, rate, n_records=3, **kw):
    return [EP.synthetic_record(rng, T, N, done_rate=rate, **kw) for _ in range(n_records)]


@pytest.mark.parametrize('T', [1, 5])
@pytest.mark.parametrize('N', [1, 7])
@pytest.mark.parametrize('rate', [0.0, 0.15, 0.6, 1.0])
@pytest.mark.parametrize('with_reward,with_result', [(True, True), (False, True), (True, False), (False, False)])
def test_restatement_equals_monitor_loop(L, T, N, rate, with_reward, with_result):
    rng = np.random.default_rng([T, N, int(rate * 100), with_reward, with_result])
    recs = chained(rng, T, N, rate, with_reward=with_reward, with_result=with_result)
    eps, acc_ret, acc_len = EP.monitor(recs, N)
    hs = EP.HostStats(L, N, capacity=max(1, 3 * T * N))          # keeps every episode
    for k, rec in enumerate(recs):
        hs.update(*rec)
        assert int(hs.totals[6]) + int(hs.acc_length.sum()) == int(hs.totals[1]) * N, k
    got = hs.episodes()
    assert len(got['return']) == len(eps) == int(hs.totals[0])
    assert int(hs.totals[1]) == 3 * T and int(hs.totals[7]) == 0
    want = {k: np.array([e[j] for e in eps], dt) for j, (k, dt) in enumerate(zip(EP.RING_FIELDS, EP.RING_DTYPES))}
    for k in EP.RING_FIELDS:
        assert np.array_equal(EP.bits(got[k]), EP.bits(want[k])), k           # returns bitwise
    hist = np.bincount(np.where(want['result'] <= 3, want['result'], 0), minlength=4)
    assert hs.totals[2:6].tolist() == hist.tolist()
    assert int(hs.totals[6]) == int(want['length'].sum())
    assert np.array_equal(EP.bits(hs.acc_return), EP.bits(acc_ret)) and np.array_equal(hs.acc_length, acc_len)


def test_minus_zero_carry_becomes_plus_zero_without_reward(L):
    hs = EP.HostStats(L, 2, capacity=4)
    hs.acc_return[:] = np.float32(-0.0)
    hs.update(None, np.array([[0, 1]], np.uint8))
    assert EP.bits(hs.acc_return).tolist() == [0, 0] and EP.bits(hs.episodes()['return']).tolist() == [0]


@pytest.mark.parametrize('C', [1, 3, 5])
def test_overflow_keeps_the_last_C_of_the_call(L, C):
    rng = np.random.default_rng(C)
    T, N, e0 = 4, 6, 7
    rec = EP.synthetic_record(rng, T, N, done_rate=0.7)
    n = int((rec[1] != 0).sum())
    assert n > 5
    full = EP.HostStats(L, N, capacity=T * N)
    full.update(*rec)
    all_eps = full.episodes()
    hs = EP.HostStats(L, N, capacity=C, fill=0xA5)
    hs.totals[0] = e0
    hs.update(*rec)
    assert hs.totals[0] == e0 + n and hs.totals[7] == n - C
    for k in EP.RING_FIELDS:
        for rank in range(n - C, n):
            assert EP.bits(hs.ring[k])[(e0 + rank) % C] == EP.bits(all_eps[k])[rank], (k, rank)
    # fewer than C in a call: the slots it does not own keep what they held
    few = EP.HostStats(L, 3, capacity=8, fill=0xA5)
    few.update(None, np.array([[0, 3, 0]], np.uint8))
    assert few.ring['length'].tolist() == [1] + [int(EP.sentinel((1,), np.int32, 0xA5)[0])] * 7 and few.totals[7] == 0


def test_callback_on_episode_stats_equals_on_result_codes(L):
    from utils.info_collector_callback import InfoCollectorCallback
    rng = np.random.default_rng(11)
    N = 37
    hs = EP.HostStats(L, N, capacity=400)
    a, b = InfoCollectorCallback(), InfoCollectorCallback()
    for T in (9, 1, 12):
        reward, done, result = EP.synthetic_record(rng, T, N, done_rate=0.3, junk=False)
        hs.update(reward, done, result)
        a.on_episode_stats(hs)
        b.on_result_codes(result)
    assert len(a.infos) > 200                                     # more than two blocks of 100
    assert a.infos == b.infos
    assert a.update_results_dict() == b.update_results_dict()
    a.on_episode_stats(hs)                                         # nothing new: nothing appended
    assert a.infos == b.infos


def test_new_result_codes_raises_after_a_drop(L):
    rng = np.random.default_rng(5)
    hs = EP.HostStats(L, 8, capacity=5)
    hs.update(None, np.eye(8, dtype=np.uint8)[:3], np.full((3, 8), 2, np.uint8))
    assert hs.new_result_codes().tolist() == [2, 2, 2]
    hs.update(*EP.synthetic_record(rng, 2, 8, done_rate=1.0))      # 16 episodes into a ring of 5
    assert hs.totals[7] == 11
    with pytest.raises(RuntimeError, match='larger capacity'):
        hs.new_result_codes()
    hs.update(None, np.eye(8, dtype=np.uint8)[:2], np.full((2, 8), 3, np.uint8))
    assert hs.new_result_codes().tolist() == [3, 3]               # and it recovers
    # overwritten between two calls without any single call dropping
    hs2 = EP.HostStats(L, 8, capacity=5)
    for _ in range(2):
        hs2.update(None, np.eye(8, dtype=np.uint8)[:3])
    assert hs2.totals[7] == 0
    with pytest.raises(RuntimeError, match='larger capacity'):
        hs2.new_result_codes()


def test_declared_bound_and_built():
    from soccer2d_amd import _capi
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 's2d.h')).read(), flags=re.S)
    bound = {p[0]: p for p in _capi.PROTOTYPES}
    for name in ('s2d_episode_stats', 's2d_episode_stats_workspace'):
        assert re.search(r'\b%s\s*\(' % name, hdr) and name in bound, name
    assert len(bound['s2d_episode_stats'][2]) == 12 and len(bound['s2d_episode_stats_workspace'][2]) == 2
    assert [f[0] for f in _capi.S2DEpisodeRing._fields_] == ['ret', 'length', 'result', 'env', 'step', 'capacity']
    mk = open(os.path.join(ROOT, 'gym-soccer-2d-env_amd', 'csrc', 'Makefile')).read()
    assert 's2d_episodes.hip' in mk
