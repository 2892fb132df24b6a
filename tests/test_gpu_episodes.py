"""Episode statistics on the GPU (s2d_episode_stats through soccer2d_amd.episodes.EpisodeStats and through ctypes): every ring
slot, carry and total against the host restatement (tests/episodes_ref.c) over the wave and workgroup edges, every done rate,
with and without reward / result and at every kind of capacity; sentinels and guard words; chained records with the ring's
wrap inside a call; update in a captured graph; closed loops with the reach-ball and 11v11 engines; the reference's callback;
rejections.  Every comparison is bitwise."""
import ctypes as C
import itertools

import numpy as np
import pytest

import episodes as EP

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

DEV = 'cuda:0'
FILL, GUARD, GUARD_BYTES = 0xA5, 0x5C, 64
NS, TS = (1, 63, 64, 65, 255, 256, 257, 1000), (1, 2, 7, 33)
RATES = (0.0, 0.02, 0.5, 1.0)
MODES = ((True, True), (True, False), (False, False))          # (reward, result): both, result=None, reward=None and result=None
CAPS = (1, 5, 100, None)                                        # None: 2 * T * N


@pytest.fixture(scope='module')
def L(tmp_path_factory):
    return EP.build(tmp_path_factory.mktemp('episodes_ref'))


@pytest.fixture(scope='module')
def lib():
    from soccer2d_amd import _capi
    return _capi.load_library()


def grid_record(N, T, rate, mode):
    rng = np.random.default_rng([N, T, int(rate * 100), mode[0], mode[1]])
    return EP.synthetic_record(rng, T, N, done_rate=rate, with_reward=mode[0], with_result=mode[1]), rng


class Guarded:
    """a host array on the device with GUARD bytes behind it"""

    def __init__(self, host):
        self.host = np.ascontiguousarray(host)
        raw = np.concatenate([self.host.view(np.uint8).ravel(), np.full(GUARD_BYTES, GUARD, np.uint8)])
        self.t = torch.from_numpy(raw).to(DEV)
        self.ptr = self.t.data_ptr()

    def get(self):
        raw = self.t.cpu().numpy()
        assert (raw[self.host.nbytes:] == GUARD).all(), 'guard bytes overwritten'
        return raw[:self.host.nbytes].view(self.host.dtype).reshape(self.host.shape)


def start_state(L, rng, N, cap):
    """a host twin with sentinel ring, non-zero carries and totals (the episode cursor somewhere inside the ring)"""
    hs = EP.HostStats(L, N, cap, fill=FILL)
    hs.acc_return[:] = rng.standard_normal(N).astype(np.float32)
    hs.acc_return[::3] = np.float32(-0.0)
    hs.acc_length[:] = rng.integers(0, 50, N)
    hs.totals[:] = rng.integers(1, 1000, 8).astype(np.uint64)
    return hs


def raw_call(lib, T, N, dev, inputs, space, ws_bytes=None, cap=None, **ptr):
    """s2d_episode_stats through ctypes on the state `dev`, the record `inputs` ('done', and 'reward' / 'res' or NULL) and the
    workspace; ptr overrides single pointers"""
    from soccer2d_amd import _capi
    p = dict(reward=None, res=None, ws=space.ptr)
    p.update({k: v.ptr for k, v in list(dev.items()) + list(inputs.items())})
    p.update(ptr)
    ring = _capi.S2DEpisodeRing(p['return'], p['length'], p['result'], p['env'], p['step'], dev['return'].host.size if cap is None else cap)
    return lib.s2d_episode_stats(T, N, p['reward'], p['done'], p['res'], p['acc_return'], p['acc_length'], C.byref(ring), p['totals'],
                                 p['ws'], space.host.nbytes if ws_bytes is None else ws_bytes,
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))


def to_device(hs):
    dev = {k: Guarded(hs.ring[k]) for k in EP.RING_FIELDS}
    dev.update(acc_return=Guarded(hs.acc_return), acc_length=Guarded(hs.acc_length), totals=Guarded(hs.totals))
    return dev


def record_to_device(rec):
    return {k: Guarded(v) for k, v in zip(('reward', 'done', 'res'), rec) if v is not None}


def same_state(dev, hs, what):
    torch.cuda.synchronize()
    for k in EP.RING_FIELDS:
        got, want = EP.bits(dev[k].get()), EP.bits(hs.ring[k])
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f'{what}: ring {k} differs in {bad.size} slots, first {bad[:5]}: {got[bad[:5]]} != {want[bad[:5]]}'
    assert np.array_equal(EP.bits(dev['acc_return'].get()), EP.bits(hs.acc_return)), f'{what}: acc_return'
    assert np.array_equal(dev['acc_length'].get(), hs.acc_length), f'{what}: acc_length'
    assert dev['totals'].get().tolist() == hs.totals.tolist(), f'{what}: totals'


def test_grid_holds_every_kind_of_case():
    """on the host-side counts, so the grid cannot silently lose a branch: no episode, all kept, some dropped -- and the ring's
    wrap inside a call happens too (start_state puts the cursor inside the ring)"""
    kinds = dict(none=0, kept=0, dropped=0)
    for N, T, rate, mode, cap in itertools.product(NS, TS, RATES, MODES, CAPS):
        (_, done, _), _ = grid_record(N, T, rate, mode)
        n, c = int((done != 0).sum()), 2 * T * N if cap is None else cap
        kinds['none' if n == 0 else 'kept' if n <= c else 'dropped'] += 1
    print('grid cases:', kinds)
    assert min(kinds.values()) >= 32, kinds
    assert set(NS) >= {63, 64, 65, 255, 256, 257} and max(NS) > 256 * 3 and min(TS) == 1


@pytest.mark.parametrize('T', TS)
@pytest.mark.parametrize('N', NS)
def test_grid_equals_restatement_sentinels_and_guards(L, lib, N, T):
    for rate, mode in itertools.product(RATES, MODES):
        rec, rng = grid_record(N, T, rate, mode)
        inputs = record_to_device(rec)
        ws = Guarded(np.full(lib.s2d_episode_stats_workspace(T, N), FILL, np.uint8))
        for cap in CAPS:
            cap = 2 * T * N if cap is None else cap
            hs = start_state(L, rng, N, cap)
            dev = to_device(hs)
            hs.update(*rec)
            assert raw_call(lib, T, N, dev, inputs, ws) == 0, lib.s2d_last_error()
            same_state(dev, hs, f'N={N} T={T} rate={rate} mode={mode} C={cap}')
        ws.get()                                                    # the workspace's guard
        for k, v in inputs.items():                                 # the inputs are untouched
            assert np.array_equal(v.get(), v.host), k


def dev_stats(hs):
    """an EpisodeStats in the host twin's state"""
    from soccer2d_amd.episodes import EpisodeStats
    st = EpisodeStats(hs.num_envs, hs.capacity, DEV)
    for k in EP.RING_FIELDS:
        st.ring[k].copy_(torch.from_numpy(hs.ring[k]))
    st.acc_return.copy_(torch.from_numpy(hs.acc_return))
    st.acc_length.copy_(torch.from_numpy(hs.acc_length))
    st.totals.copy_(torch.from_numpy(hs.totals.astype(np.int64)))
    return st


def same_stats(st, hs, what):
    torch.cuda.synchronize()
    for k in EP.RING_FIELDS:
        assert np.array_equal(EP.bits(st.ring[k].cpu().numpy()), EP.bits(hs.ring[k])), f'{what}: ring {k}'
    assert np.array_equal(EP.bits(st.acc_return.cpu().numpy()), EP.bits(hs.acc_return)), f'{what}: acc_return'
    assert np.array_equal(st.acc_length.cpu().numpy(), hs.acc_length), f'{what}: acc_length'
    assert st.totals.cpu().tolist() == hs.totals.astype(np.int64).tolist(), f'{what}: totals'


def dev_rec(rec):
    return tuple(None if v is None else torch.from_numpy(v).to(DEV) for v in rec)


@pytest.mark.parametrize('N, T, cap, e0, rate', [(257, 7, 100, 93, 0.02), (65, 33, 5, 4, 0.1), (1000, 2, 300, 299, 0.05),
                                                 (1, 33, 7, 6, 0.3)])
def test_three_chained_records_wrap_inside_a_call(L, N, T, cap, e0, rate):
    rng = np.random.default_rng([N, T, cap])
    hs = EP.HostStats(L, N, cap, fill=FILL)
    hs.totals[0] = e0                                               # (e0 + k) mod C wraps inside the first call
    st = dev_stats(hs)
    wrapped = False
    for k in range(3):
        rec = EP.synthetic_record(rng, T, N, done_rate=rate)
        n, before = int((rec[1] != 0).sum()), int(hs.totals[0])
        wrapped |= (before + max(0, n - cap)) % cap + min(n, cap) > cap      # the written slots pass the ring's end
        hs.update(*rec)
        assert st.update(*dev_rec(rec)) is st
        same_stats(st, hs, f'record {k}')
        t = st.totals.cpu().tolist()
        assert t[6] + int(st.acc_length.sum()) == t[1] * N           # every step is in a finished episode or in a carry
    assert wrapped and hs.totals[0] > e0
    got, want = st.episodes(), hs.episodes()
    for k in EP.RING_FIELDS:
        assert np.array_equal(EP.bits(got[k].cpu().numpy()), EP.bits(want[k])), k
    s = st.summary()
    assert s['episodes'] == int(hs.totals[0]) and s['steps'] == 3 * T and s['dropped'] == int(hs.totals[7])
    assert s['ep_len_mean'] == pytest.approx(float(want['length'].mean()), rel=1e-6)
    # a float32 mean of m values: every partial sum is within m * max|x| and rounds once, so the mean is within m * 2^-24 * max|x|
    m = len(want['return'])
    assert abs(s['ep_rew_mean'] - float(want['return'].astype(np.float64).mean())) <= m * 2.0 ** -24 * float(np.abs(want['return']).max())
    st.reset()
    assert not st.totals.any() and not st.acc_length.any() and not st.acc_return.any() and st.summary()['episodes'] == 0


def test_update_in_a_captured_graph(L):
    from soccer2d_amd.episodes import EpisodeStats
    rng = np.random.default_rng(21)
    T, N, cap = 7, 321, 150
    recs = [EP.synthetic_record(rng, T, N, done_rate=0.08) for _ in range(3)]
    st = EpisodeStats(N, cap, DEV)
    st.workspace(T, N)                                              # allocated outside the capture
    buf = dev_rec(recs[2])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # a warm-up outside the capture, on an object of its own
        EpisodeStats(N, cap, DEV).update(*buf)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st.update(*buf)
    torch.cuda.synchronize()
    assert not st.totals.any()                                      # capturing ran nothing
    hs = EP.HostStats(L, N, cap)
    for k, rec in enumerate(recs):
        for b, v in zip(buf, rec):
            b.copy_(torch.from_numpy(v))
        graph.replay()
        hs.update(*rec)
        same_stats(st, hs, f'replay {k}')
    assert hs.totals[0] > cap                                        # the ring went round


def check_record(L, rec, N, cap, what):
    """EpisodeStats.update_record against the restatement on the downloaded record; returns (stats, host twin)"""
    from soccer2d_amd.episodes import EpisodeStats
    st, hs = EpisodeStats(N, cap, DEV), EP.HostStats(L, N, cap)
    for k, r in enumerate(rec):
        st.update_record(r)
        torch.cuda.synchronize()
        h = {k2: v.cpu().numpy() for k2, v in r.items() if torch.is_tensor(v)}
        hs.update(h.get('reward'), h['done'], h.get('result'))
        same_stats(st, hs, f'{what}, launch {k}')
    return st, hs


def copy_rec(rec):
    return {k: v.clone() for k, v in rec.items() if torch.is_tensor(v)}


@pytest.fixture(scope='module')
def reach_records():
    """two launches of T = 16 at N = 256, max_steps = 8: random actions and the in-kernel stochastic policy"""
    import oracle as O
    from soccer2d_amd.actor import StochasticActor
    from soccer2d_amd.engine import Engine, make_config
    N, T = 256, 16
    out = {}
    for kind in ('random', 'policy'):
        eng = Engine(N, DEV, cfg=make_config(**dict(O.DQN_KWARGS, max_steps=8)))
        eng.reset()
        if kind == 'policy':
            net = torch.nn.Sequential(torch.nn.Linear(10, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
                                      torch.nn.Linear(64, 16))
            g = torch.Generator().manual_seed(3)
            with torch.no_grad():
                for p in net.parameters():
                    p.copy_(torch.rand(p.shape, generator=g) * 2 - 1)
            actor = StochasticActor.from_module(net.to(DEV), device=DEV)
            out[kind] = [copy_rec(eng.rollout_policy(T, actor)) for _ in range(2)]
        else:
            out[kind] = [copy_rec(eng.rollout(T)) for _ in range(2)]
        torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('kind', ['random', 'policy'])
def test_closed_loop_reach_ball(L, reach_records, kind):
    recs = reach_records[kind]
    st, hs = check_record(L, recs, 256, 2 * 2 * 16 * 256, f'reach-ball {kind}')
    res = torch.cat([r['result'][r['done'] != 0] for r in recs])
    counts = torch.bincount(res.long(), minlength=4).cpu().tolist()
    t = st.totals.cpu().tolist()
    print(f'reach-ball {kind}: results none/goal/out/timeout {counts}, totals {t}')
    assert t[2:6] == counts and t[0] == sum(counts) >= 256          # max_steps = 8: every env finished at least once in 32 steps
    assert t[7] == 0 and t[6] + int(st.acc_length.sum()) == t[1] * 256
    assert int(st.episodes()['length'].min()) >= 1
    s = st.summary()
    assert s['Goal'] == counts[1] / t[0] and s['Timeout'] == counts[3] / t[0] and s['unlabelled'] == 0


def test_closed_loop_match_record_without_result(L):
    from soccer2d_amd.match import MatchEngine
    N, T = 48, 24
    eng = MatchEngine(N, DEV, noise=True, seed=11, half_time_cycles=8, nr_extra_halfs=0, penalty_shoot_outs=0)
    eng.reset()
    recs = []
    for _ in range(2):
        r = eng.rollout(T, with_obs=False)
        recs.append({k: r[k].clone() for k in ('reward', 'done') if r.get(k) is not None})
    assert 'result' not in recs[0]
    st, hs = check_record(L, recs, N, 4 * N, '11v11')
    t = st.totals.cpu().tolist()
    print('11v11 totals:', t)
    assert t[0] > 0 and t[2] == t[0] and t[3:6] == [0, 0, 0]         # every episode is unlabelled
    eng.close()


def test_callback_on_a_closed_loop_record(reach_records):
    from soccer2d_amd.episodes import EpisodeStats
    from utils.info_collector_callback import InfoCollectorCallback
    a, b = InfoCollectorCallback(), InfoCollectorCallback()
    st = EpisodeStats(256, 2 * 16 * 256, DEV)
    for rec in reach_records['random']:
        a.on_episode_stats(st.update_record(rec))
        b.on_result_codes(rec['result'])
    assert len(a.infos) >= 256 and a.infos == b.infos
    assert a.update_results_dict() == b.update_results_dict()
    small = EpisodeStats(256, 100, DEV).update_record(reach_records['random'][0])
    with pytest.raises(RuntimeError, match='larger capacity'):
        small.new_result_codes()


def test_rejections_return_einval_and_touch_nothing(L, lib):
    from soccer2d_amd import _capi
    rng = np.random.default_rng(13)
    T, N, cap = 3, 70, 9
    rec = EP.synthetic_record(rng, T, N, done_rate=0.3)
    hs = start_state(L, rng, N, cap)
    dev, inputs = to_device(hs), record_to_device(rec)
    need = lib.s2d_episode_stats_workspace(T, N)
    ws = Guarded(np.full(need, FILL, np.uint8))
    assert need > 0
    for shape in ((0, 4), (-1, 4), (4, 0), (4, -3), (4, 2 ** 31), (2 ** 20, 2 ** 20), (2 ** 30, 2 ** 10)):
        assert lib.s2d_episode_stats_workspace(*shape) == 0, shape
    assert lib.s2d_episode_stats_workspace(2 ** 20, 2 ** 20 - 1) > 0   # just below 2^40: a size, computed on the host

    def call(T=T, N=N, ws_bytes=None, cap=None, **kw):
        return raw_call(lib, T, N, dev, inputs, ws, ws_bytes=ws_bytes, cap=cap, **kw)

    cases = [dict(T=0), dict(T=-2), dict(N=0), dict(N=-1), dict(N=2 ** 31), dict(T=2 ** 20, N=2 ** 20), dict(cap=0), dict(cap=-4),
             dict(cap=2 ** 31), dict(done=None), dict(acc_return=None), dict(acc_length=None), dict(totals=None), dict(ws=None),
             dict(length=None), dict(env=None), dict(step=None), dict(result=None), dict(totals=dev['totals'].ptr + 4),
             dict(step=dev['step'].ptr + 4), dict(ws_bytes=need - 1), dict(ws_bytes=0)]
    cases.append({'return': None})
    for kw in cases:
        assert call(**kw) == _capi.S2D_EINVAL, kw
        assert b's2d_episode_stats' in lib.s2d_last_error(), (kw, lib.s2d_last_error())
    assert lib.s2d_episode_stats(T, N, inputs['reward'].ptr, inputs['done'].ptr, inputs['res'].ptr, dev['acc_return'].ptr,
                                 dev['acc_length'].ptr, None, dev['totals'].ptr, ws.ptr, need, None) == _capi.S2D_EINVAL   # no ring
    same_state(dev, hs, 'after the refused calls')                  # hs was never advanced
    assert (ws.get() == FILL).all()
    for k, v in inputs.items():
        assert np.array_equal(v.get(), v.host), k
    assert call() == 0                                               # and the same arguments, unchanged, are accepted
    hs.update(*rec)
    same_state(dev, hs, 'the accepted call')


def test_python_side_validation():
    from soccer2d_amd.episodes import EpisodeStats
    T, N = 4, 10
    st = EpisodeStats(N, 5, DEV)
    good = dict(reward=torch.zeros(T, N, device=DEV), done=torch.ones(T, N, dtype=torch.uint8, device=DEV),
                result=torch.ones(T, N, dtype=torch.uint8, device=DEV))
    bad = [dict(done=good['done'].bool()), dict(done=good['done'][:, :9]), dict(done=good['done'].cpu()),
           dict(done=torch.ones(N, T, dtype=torch.uint8, device=DEV).t()), dict(done=good['done'][0]), dict(done=None),
           dict(reward=good['reward'].double()), dict(reward=good['reward'][:3]), dict(reward=good['reward'].cpu()),
           dict(reward=torch.zeros(T, 2 * N, device=DEV)[:, ::2]),
           dict(result=good['result'].int()), dict(result=good['result'][1:]), dict(result=good['result'].cpu())]
    for kw in bad:
        with pytest.raises(ValueError):
            st.update(**dict(good, **kw))
    torch.cuda.synchronize()
    assert not st.totals.any() and not st.acc_length.any()           # nothing ran
    st.update(**good)
    assert st.summary()['episodes'] == T * N and st.summary()['dropped'] == T * N - 5
    for kw in (dict(num_envs=0), dict(num_envs=4, capacity=0), dict(num_envs=4, capacity=2 ** 31), dict(num_envs=4, device='cpu')):
        with pytest.raises(ValueError):
            EpisodeStats(**kw)
