"""The fused stochastic policy (s2d_rollout_policy / Engine.rollout_policy) and the advantage scan (s2d_gae / gae()): closed-loop
bit parity against the CPU oracle (the per-step API for the rcssserver noise model) driven by the host restatement of the
policy (tests/policy_ref.c) with every record word, logp included; the head alone bit for bit on the edge rows; other shapes;
the device draw's distribution; graph replay with weights, log_std and the deterministic word updated in place; chaining; the
greedy switch against the Q-actor; gae() bit for bit; rejections; and a short run of the example."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
import policy_ref as P
from actor_refusals import refused
from test_policy_host import EDGE_WORDS, chi2_sf_odd, chi2_stat, edge_rows, fixed_logits, gae_case, softmax64

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE = {'off': dict(noise=False), 'lattice': dict(noise=True), 'square': dict(noise=True, noise_model='rcssserver')}
MODES = {'discrete': dict(use_continuous_action=False), 'cont1': dict(use_continuous_action=True, use_turning=False),
         'turn4': dict(use_continuous_action=True, use_turning=True)}
NA = {'discrete': 16, 'cont1': 1, 'turn4': 4}
LOG_STD = {'discrete': None, 'cont1': [-0.7], 'turn4': [-0.5, -1.0, -0.3, 0.2]}
ACT = {'relu': torch.nn.ReLU, 'tanh': torch.nn.Tanh}


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp('policy_ref'))


def _kw(mode, **over):
    kw = dict(O.DQN_KWARGS)
    kw.update(MODES[mode])
    kw.update(over)
    return kw


def _engine(n, mode, noise='off', **kw):
    from soccer2d_amd.engine import Engine, make_config
    return Engine(n, 'cuda:0', cfg=make_config(**NOISE[noise], **_kw(mode, **kw)))


class _StepEngine:
    """The GPU per-step API with caller actions behind the oracle's interface (reference for the rcssserver noise model)."""

    def __init__(self, n, mode, noise, **kw):
        self.e = _engine(n, mode, noise, **kw)
        self.discrete = mode == 'discrete'

    def _np(self, t):
        torch.cuda.synchronize()
        return t.detach().cpu().numpy().copy()

    def reset(self):
        self.e.reset()

    def rollout(self, T):
        self.e.rollout(T)

    def step(self, a):
        a = np.ascontiguousarray(a, dtype=np.int32 if self.discrete else np.float32)
        o, r, d, res = self.e.step(torch.from_numpy(a).to('cuda:0'))
        return self._np(o), self._np(r), self._np(d), self._np(res)

    def obs(self):
        return self._np(self.e.obs)

    def terminal_obs(self):
        return self._np(self.e.terminal_obs)

    def done(self):
        return self._np(self.e.done)

    def result(self):
        return self._np(self.e.result)

    def stats(self):
        return self._np(self.e.stats).astype(np.uint64)

    def state(self, f):
        return self._np(getattr(self.e, f))


def _oracle(n, mode, noise='off', seed=0x5EED, **kw):
    nz = NOISE[noise]
    if nz.get('noise_model') == 'rcssserver':
        return _StepEngine(n, mode, noise, seed=seed, **kw)
    return O.OracleEngine(O.make_config(seed=seed, auto_reset=1, noise=int(nz['noise']), **_kw(mode, **kw)), n, 'f32')


def _net(h1=64, h2=64, a=16, act='tanh', seed=0, scale=0.5):
    g = torch.Generator().manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(10, h1), ACT[act](), torch.nn.Linear(h1, h2), ACT[act](), torch.nn.Linear(h2, a))
    with torch.no_grad():
        for p in net.parameters():
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * scale)
    return net


def _actor(net, log_std=None, det=False):
    from soccer2d_amd.actor import StochasticActor
    actor = StochasticActor.from_module(net.to('cuda:0'), device='cuda:0', deterministic=det)
    if log_std is not None:
        actor.log_std = log_std
    return actor


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(g, c, what):
    g = g.detach().cpu().numpy() if torch.is_tensor(g) else np.asarray(g)
    c = np.asarray(c)
    assert g.shape == c.shape, (what, g.shape, c.shape)
    if not np.array_equal(bits(g), bits(c)):
        bad = np.argwhere(bits(g) != bits(c))
        i = tuple(bad[0])
        raise AssertionError(f'{what}: {len(bad)} of {g.size} words differ; first at {i}: gpu={g[i]!r} cpu={c[i]!r}')


def int32_view(k):
    return (np.asarray(k, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


RECORD = ('obs', 'action', 'reward', 'done', 'result', 'logp')


def _closed_loop_parity(ref, n, T, mode, noise, act, det, warm=5, seed=0x5EED, h1=64, h2=64, k_set=None, scale=0.5, **kw):
    na = NA[mode]
    eng = _engine(n, mode, noise, seed=seed, **kw)
    orc = _oracle(n, mode, noise, seed=seed, **kw)
    eng.reset(); orc.reset()
    if warm:
        eng.rollout(warm); orc.rollout(warm)
    if k_set is not None:
        eng.policy_step.copy_(torch.from_numpy(int32_view(k_set)).to('cuda:0'))
        if isinstance(orc, _StepEngine):
            orc.e.policy_step.copy_(torch.from_numpy(int32_view(k_set)).to('cuda:0'))
        else:
            orc.set_state('policy_step', k_set)
    actor = _actor(_net(h1, h2, na, act, seed=n + T + na, scale=scale), LOG_STD[mode], det)
    params = actor.params.cpu().numpy()
    k0 = eng.policy_step.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    out = eng.alloc_rollout(T, terminal_obs=True, logp=True)
    out['terminal_obs'].fill_(float('nan'))
    out = eng.rollout_policy(T, actor, out=out)
    torch.cuda.synchronize()
    obs = orc.obs()
    rec = {k: [] for k in RECORD}
    term = np.full((T, n, 10), np.nan, dtype=np.float32)
    for t in range(T):
        a, lp = P.actions(ref, obs, params, h1, h2, na, act == 'tanh', mode, LOG_STD[mode], det, eng.cfg.seed, k0 + t)
        obs, rew, done, res = orc.step(a if mode == 'discrete' else np.clip(a, -1, 1))   # recorded unclipped, stepped clipped
        for k, v in (('obs', obs), ('action', a), ('reward', rew), ('done', done), ('result', res), ('logp', lp)):
            rec[k].append(v)
        d = done != 0
        term[t][d] = orc.terminal_obs()[d]
    for k in rec:
        same(out[k], np.stack(rec[k]), f'record.{k}')
    same(out['terminal_obs'], term, 'record.terminal_obs')
    for f in O.STATE_FIELDS:
        if f != 'policy_step':
            same(getattr(eng, f), orc.state(f), f'state.{f}')
    same(eng.policy_step, int32_view(k0 + T), 'policy_step = k0 + T (mod 2^32)')
    same(eng.obs, orc.obs(), 'obs'); same(eng.done, orc.done(), 'done'); same(eng.result, orc.result(), 'result')
    same(eng.reward, rec['reward'][-1], 'reward')
    same(eng.stats[:4], orc.stats()[:4].astype(np.int64), 'stats')
    return out


@pytest.mark.parametrize('det', [0, 1])
@pytest.mark.parametrize('act', ['relu', 'tanh'])
@pytest.mark.parametrize('noise', ['off', 'lattice'])
@pytest.mark.parametrize('mode', ['discrete', 'cont1', 'turn4'])
def test_closed_loop_parity(ref, mode, noise, act, det):
    out = _closed_loop_parity(ref, 1000, 64, mode, noise, act, det)
    assert int(out['done'].sum()) >= 1
    a = out['action'].cpu().numpy()
    if mode == 'discrete':
        assert a.min() >= 0 and a.max() <= 15 and (det or len(np.unique(a)) == 16)
    elif not det:
        assert (np.abs(a) > 1).any()                       # recorded unclipped
    else:
        assert (np.abs(a) <= 1).all()
    lp = out['logp'].cpu().numpy()
    assert np.isfinite(lp).all() and (mode != 'discrete' or (lp <= 0).all())


@pytest.mark.parametrize('mode', ['discrete', 'turn4'])
def test_closed_loop_parity_short_episodes_timeout_and_goal(ref, mode):
    """max_steps = 20: every env runs into Timeouts inside the launch, some reach the ball; terminal_obs on both"""
    out = _closed_loop_parity(ref, 1000, 64, mode, 'lattice', 'tanh', 0, scale=0.05, max_steps=20)
    res = out['result'].cpu().numpy()
    assert (res == 3).sum() >= 1 and (res == 1).sum() >= 1
    term = out['terminal_obs'].cpu().numpy()
    done = out['done'].cpu().numpy() != 0
    assert np.isfinite(term[done]).all() and np.isnan(term[~done]).all()


@pytest.mark.parametrize('mode', ['discrete', 'cont1', 'turn4'])
def test_closed_loop_parity_rcssserver_noise(ref, mode):
    _closed_loop_parity(ref, 1000, 32, mode, 'square', 'tanh', 0)


@pytest.mark.parametrize('mode', ['discrete', 'cont1', 'turn4'])
def test_policy_counter_wraps_past_2_31_and_2_32(ref, mode):
    n = 600
    k = np.array([2 ** 32 - 1 - (i % 7) if i % 3 == 0 else 2 ** 31 - 2 for i in range(n)], dtype=np.int64)
    _closed_loop_parity(ref, n, 12, mode, 'lattice', 'tanh', 0, warm=3, k_set=k)


# ------------------------------------------------------------------------------------------ the head alone
def _head(mode, y, log_std, gid, k, seed, det=0):
    from soccer2d_amd import _capi
    lib = _capi.load_library()
    y = np.ascontiguousarray(y, dtype=np.float32)
    n, na = y.shape
    dev = 'cuda:0'
    yt = torch.from_numpy(y).to(dev)
    lst = None if log_std is None else torch.tensor(log_std, dtype=torch.float32, device=dev)
    gt = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.asarray(gid, dtype=np.uint64), (n,))).view(np.int64)).to(dev)
    kt = torch.from_numpy(int32_view(np.broadcast_to(np.asarray(k, dtype=np.int64), (n,)))).to(dev)
    act = torch.zeros(n, dtype=torch.int32, device=dev) if mode == 'discrete' else torch.zeros((n, na), dtype=torch.float32, device=dev)
    lp = torch.zeros(n, dtype=torch.float32, device=dev)
    rc = lib.s2d_debug_policy_head(P.MODES[mode], na, yt.data_ptr(), None if lst is None else lst.data_ptr(), gt.data_ptr(),
                                   kt.data_ptr(), int(seed), int(det), n, act.data_ptr(), lp.data_ptr(), None)
    _capi.check(lib, rc, 's2d_debug_policy_head')
    torch.cuda.synchronize()
    return act.cpu().numpy(), lp.cpu().numpy()


COUNTERS = np.concatenate([np.arange(2 ** 31 - 6, 2 ** 31 + 6), np.arange(2 ** 32 - 6, 2 ** 32 + 6), np.arange(0, 64)])


def same_logp(g, c, what):
    """bit for bit; where both are NaN (non-finite logits: out of contract beyond the index) the payload is not compared"""
    both_nan = np.isnan(g) & np.isnan(c)
    same(np.where(both_nan, np.float32(0), g), np.where(both_nan, np.float32(0), c), what)


@pytest.mark.parametrize('det', [0, 1])
def test_head_alone_edge_rows(ref, det):
    seed = 0xABCDEF0123
    for name, row in edge_rows():
        y = np.broadcast_to(row, (COUNTERS.size, row.size))
        gid = np.arange(COUNTERS.size, dtype=np.uint64) * 977 + (1 << 33)
        a, lp = _head('discrete', y, None, gid, COUNTERS, seed, det)
        ca, clp = P.head(ref, 'discrete', y, None, gid, COUNTERS, seed, det)
        same(a, ca, f'{name}: action')
        same_logp(lp, clp, f'{name}: logp')
        assert a.min() >= 0 and a.max() < row.size, name


@pytest.mark.parametrize('A', [1, 2, 15, 16, 17, 64])
def test_head_alone_categorical_sizes(ref, A):
    rs = np.random.RandomState(A)
    n = 4099
    y = (rs.uniform(-1, 1, (n, A)) * rs.uniform(0, 20, (n, 1))).astype(np.float32)
    gid = rs.randint(0, 2 ** 40, n, dtype=np.int64).astype(np.uint64)
    k = COUNTERS[rs.randint(0, COUNTERS.size, n)]
    for det in (0, 1):
        a, lp = _head('discrete', y, None, gid, k, 0x5EED, det)
        ca, clp = P.head(ref, 'discrete', y, None, gid, k, 0x5EED, det)
        same(a, ca, f'A={A} det={det}: action'); same(lp, clp, f'A={A} det={det}: logp')


@pytest.mark.parametrize('mode', ['cont1', 'turn4'])
def test_head_alone_gaussian(ref, mode):
    rs = np.random.RandomState(9)
    n, A = 4099, NA[mode]
    y = (rs.uniform(-1, 1, (n, A)) * rs.uniform(0, 20, (n, 1))).astype(np.float32)
    y[:8] = np.array([0.0, -0.0, 1.0, -1.0, 1.0000001, np.inf, -np.inf, 3e38], np.float32)[:, None]
    gid = rs.randint(0, 2 ** 40, n, dtype=np.int64).astype(np.uint64)
    k = COUNTERS[rs.randint(0, COUNTERS.size, n)]
    for ls in (LOG_STD[mode], [0.0] * A, [-20.0] * A, [2.0] * A):
        for det in (0, 1):
            a, lp = _head(mode, y, ls, gid, k, 0x77, det)
            ca, clp = P.head(ref, mode, y, ls, gid, k, 0x77, det)
            same_logp(a, ca, f'{mode} ls={ls} det={det}: action'); same(lp, clp, f'{mode} ls={ls} det={det}: logp')


# ------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize('n', [1, 63, 1000, 4097])
def test_ragged_sizes(ref, n):
    _closed_loop_parity(ref, n, 9, 'turn4', 'lattice', 'tanh', 0, warm=3)
    _closed_loop_parity(ref, n, 9, 'discrete', 'lattice', 'relu', 0, warm=3)


@pytest.mark.parametrize('act', ['relu', 'tanh'])
@pytest.mark.parametrize('h1,h2', [(16, 16), (128, 128), (48, 80)])
def test_other_shapes(ref, h1, h2, act):
    _closed_loop_parity(ref, 1000, 6, 'discrete', 'lattice', act, 0, warm=2, h1=h1, h2=h2)
    _closed_loop_parity(ref, 1000, 6, 'cont1', 'lattice', act, 0, warm=2, h1=h1, h2=h2)


def test_device_draws_follow_the_softmax():
    """fixed logits (zero output weights, the logits as the bias): 65 536 envs x 4 steps pass the host test's chi-square"""
    y = fixed_logits()
    net = _net(seed=1)
    with torch.no_grad():
        net[4].weight.zero_(); net[4].bias.copy_(torch.from_numpy(y))
    eng = _engine(65536, 'discrete', 'off')
    eng.reset()
    r = eng.rollout_policy(4, _actor(net), with_obs=False)
    torch.cuda.synchronize()
    a = r['action'].cpu().numpy().reshape(-1)
    prob = softmax64(y)
    stat = chi2_stat(np.bincount(a, minlength=16).astype(np.float64), prob)
    assert chi2_sf_odd(stat, 15) > 1e-6, stat
    assert np.abs(r['logp'].cpu().numpy().reshape(-1).astype(np.float64) - np.log(prob)[a]).max() < 1e-6


# ------------------------------------------------------------------------------------------ graph replay, chaining, greedy
def test_graph_replay_reads_weights_log_std_and_the_deterministic_word_at_replay():
    n, T = 4096, 16
    eng = _engine(n, 'turn4', 'lattice')
    eng.reset()
    net1, net2 = _net(a=4, seed=7).to('cuda:0'), _net(a=4, seed=8).to('cuda:0')
    actor = _actor(net1, LOG_STD['turn4'])
    out = eng.alloc_rollout(T, terminal_obs=True, logp=True)
    eng.rollout_policy(T, actor, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.rollout_policy(T, actor, out=out)
    torch.cuda.synchronize()
    new_ls = [0.1, -0.2, -1.5, 0.0]
    for det in (False, True):
        actor.load_from(net2)
        actor.log_std = new_ls
        actor.deterministic = det
        sd = eng.state_dict()
        g.replay()
        torch.cuda.synchronize()
        got = {k: out[k].clone() for k in RECORD}
        state = {f: getattr(eng, f).clone() for f in O.STATE_FIELDS}
        eng.load_state_dict(sd)
        r = eng.rollout_policy(T, _actor(net2, new_ls, det))
        torch.cuda.synchronize()
        for k in got:
            same(got[k], r[k].cpu().numpy(), f'det={det} {k}')
        for f in state:
            same(state[f], getattr(eng, f).cpu().numpy(), f'det={det} {f}')
    assert (got['action'].abs() <= 1).all()                # the last replay was the greedy one: clip(y)


@pytest.mark.parametrize('mode', ['discrete', 'turn4'])
def test_chaining(mode):
    n, T = 2048, 64
    a, b = _engine(n, mode, 'lattice'), _engine(n, mode, 'lattice')
    a.reset(); b.reset()
    actor = _actor(_net(a=NA[mode], seed=3), LOG_STD[mode])
    r1 = a.rollout_policy(T // 2, actor, terminal_obs=True)
    r2 = a.rollout_policy(T // 2, actor, terminal_obs=True)
    r = b.rollout_policy(T, actor, terminal_obs=True)
    torch.cuda.synchronize()
    for k in RECORD:
        same(torch.cat([r1[k], r2[k]]), r[k].cpu().numpy(), k)
    d = torch.cat([r1['done'], r2['done']]).bool()
    same(torch.cat([r1['terminal_obs'], r2['terminal_obs']])[d], r['terminal_obs'][d].cpu().numpy(), 'terminal_obs')
    for f in O.STATE_FIELDS:
        same(getattr(a, f), getattr(b, f).cpu().numpy(), f)
    same(a.stats, b.stats.cpu().numpy(), 'stats')


@pytest.mark.parametrize('noise', ['off', 'lattice'])
def test_deterministic_discrete_is_the_q_actor_with_epsilon_zero(noise):
    from soccer2d_amd.actor import QNetActor
    n, T = 3000, 40
    a, b = _engine(n, 'discrete', noise), _engine(n, 'discrete', noise)
    a.reset(); b.reset()
    net = _net(act='relu', seed=12)
    ra = a.rollout_policy(T, _actor(net, det=True))
    rb = b.rollout_qnet(T, QNetActor.from_module(net.to('cuda:0'), device='cuda:0', epsilon=0.0))
    torch.cuda.synchronize()
    for k in ('obs', 'action', 'reward', 'done', 'result'):
        same(ra[k], rb[k].cpu().numpy(), k)
    for f in O.STATE_FIELDS:
        same(getattr(a, f), getattr(b, f).cpu().numpy(), f)
    same(a.stats, b.stats.cpu().numpy(), 'stats')


# ------------------------------------------------------------------------------------------ gae
@pytest.fixture(scope='module')
def gae_record():
    """one record [256, 4097] shared by the gae cases (slices of it)"""
    return gae_case(0.99, 0.95, T=256, N=4097, seed=3)


@pytest.mark.parametrize('T', [1, 2, 33, 256])
def test_gae_equals_the_restatement(ref, gae_record, T):
    from soccer2d_amd.gae import gae
    out = None
    for N in (1, 63, 1000, 4097):
        reward, done, value, last, result, tval = (np.ascontiguousarray(x[-T:, :N] if x.ndim == 2 else x[:N]) for x in gae_record)
        dev = [torch.from_numpy(x).to('cuda:0') for x in (reward, done, value, last, result, tval)]
        for timeouts in (True, False):
            for gamma, lam in ((0.99, 0.95), (1.0, 1.0), (0.9, 0.0)):
                kw = dict(result=dev[4], terminal_value=dev[5]) if timeouts else {}
                ckw = dict(result=result, terminal_value=tval) if timeouts else {}
                if out is None or out[0].shape != (T, N):
                    out = (torch.empty((T, N), device='cuda:0'), torch.empty((T, N), device='cuda:0'))
                adv, ret = gae(dev[0], dev[1], dev[2], dev[3], gamma, lam, out=out, **kw)      # `out` reused across the cases
                assert adv is out[0] and ret is out[1]
                torch.cuda.synchronize()
                cadv, cret = P.gae(ref, reward, done, value, last, gamma, lam, **ckw)
                same(adv, cadv, f'T={T} N={N} timeouts={timeouts} gamma={gamma}: advantage')
                same(ret, cret, f'T={T} N={N} timeouts={timeouts} gamma={gamma}: ret')
        adv, ret = gae(*dev[:4], 0.99, 0.95)                                                   # fresh outputs
        torch.cuda.synchronize()
        same(adv, P.gae(ref, reward, done, value, last, 0.99, 0.95)[0], 'fresh advantage')


def test_gae_rejections_raise_without_a_launch():
    from soccer2d_amd import _capi
    from soccer2d_amd.gae import gae
    T, N = 4, 100
    f = lambda *s: torch.zeros(s, device='cuda:0')
    r, d, v, lv = f(T, N), torch.zeros((T, N), dtype=torch.uint8, device='cuda:0'), f(T, N), f(N)
    adv, ret = torch.full((T, N), 7.0, device='cuda:0'), torch.full((T, N), 7.0, device='cuda:0')
    bad = [dict(gamma=float('nan')), dict(lam=float('inf')), dict(result=d), dict(terminal_value=v), dict(last_value=f(N + 1)),
           dict(done=d.float()), dict(value=f(T + 1, N)), dict(reward=f(T, N).t().contiguous().t()), dict(reward=f(0, N))]
    for over in bad:
        kw = dict(reward=r, done=d, value=v, last_value=lv, gamma=0.99, lam=0.95, out=(adv, ret))
        kw.update(over)
        with pytest.raises(ValueError):
            gae(**kw)
    lib = _capi.load_library()
    p = [x.data_ptr() for x in (r, d, v, lv)]
    for args in ((0, N, *p, None, None, 0.99, 0.95), (T, 0, *p, None, None, 0.99, 0.95), (T, N, *p, d.data_ptr(), None, 0.99, 0.95),
                 (T, N, *p, None, v.data_ptr(), 0.99, 0.95), (T, N, *p, None, None, float('nan'), 0.95),
                 (T, N, *p, None, None, 0.99, float('-inf')), (T, N, None, *p[1:], None, None, 0.99, 0.95)):
        assert lib.s2d_gae(*args, adv.data_ptr(), ret.data_ptr(), None) == _capi.S2D_EINVAL, args
    torch.cuda.synchronize()
    assert bool((adv == 7).all()) and bool((ret == 7).all())


# ------------------------------------------------------------------------------------------ rejections, surface, example
def test_rejections_leave_the_state_unchanged():
    from soccer2d_amd import _capi
    from soccer2d_amd.actor import StochasticActor
    ro = _capi.S2DRollout()
    for mode in ('discrete', 'cont1', 'turn4'):
        na = NA[mode]
        actor = _actor(_net(a=na), LOG_STD[mode])
        eng = _engine(256, mode, 'off')
        eng.reset()
        before = {f: getattr(eng, f).clone() for f in O.STATE_FIELDS}
        arena = eng.arena.clone()

        def rc(net, T=4):
            return eng.lib.s2d_rollout_policy(eng._h, T, C.byref(net), C.byref(ro), None, None, eng._stream())
        for h1, h2, a, fn in ((40, 64, na, 1), (256, 64, na, 1), (64, 0, na, 1), (64, 64, na + 1, 1), (64, 64, 65, 1), (64, 64, 0, 1),
                              (64, 64, na, 2), (64, 64, na, -1)):
            net = actor.c_struct()
            net.hidden1, net.hidden2, net.n_out, net.activation = h1, h2, a, fn
            refused(eng.lib, f's2d_rollout_policy/struct/{mode}/{h1}-{h2}-{a} activation {fn}', rc(net))
        fields = [('params', actor.params.data_ptr() + 4), ('params', None), ('deterministic', None),
                  ('deterministic', actor.deterministic_tensor.data_ptr() + 2)]
        if mode != 'discrete':
            fields += [('log_std', None), ('log_std', actor.log_std.data_ptr() + 1)]
        for field, val in fields:
            net = actor.c_struct()
            setattr(net, field, val)
            text = refused(eng.lib, f's2d_rollout_policy/struct/{mode}/{field} {"NULL" if val is None else "misaligned"}', rc(net))
            assert 's2d_rollout_policy' in text
        refused(eng.lib, f's2d_rollout_policy/struct/{mode}/n_steps 0', rc(actor.c_struct(), T=0))
        with pytest.raises(ValueError):
            eng.rollout_policy(4, StochasticActor(64, 64, na + 1))
        with pytest.raises(ValueError):
            eng.rollout_policy(0, actor)
        torch.cuda.synchronize()
        for f in before:
            assert torch.equal(before[f], getattr(eng, f)), (mode, f)
        assert torch.equal(arena, eng.arena)
        if mode == 'discrete':                               # log_std may be NULL on a discrete engine
            net = actor.c_struct()
            net.log_std = None
            assert rc(net) == _capi.S2D_OK
            torch.cuda.synchronize()


def test_record_forms_and_vec_env_dispatch():
    from soccer2d_amd.vec_env import Soccer2DVecEnv
    venv = Soccer2DVecEnv(256, **_kw('turn4'))
    venv.reset()
    actor = _actor(_net(a=4), LOG_STD['turn4'])
    r = venv.rollout(8, policy=actor, terminal_obs=True)
    torch.cuda.synchronize()
    assert r['action'].shape == (8, 256, 4) and r['terminal_obs'].shape == (8, 256, 10) and r['logp'].shape == (8, 256)
    eng = venv.engine
    r = eng.rollout_policy(8, actor, logp=False, with_obs=False)
    assert 'logp' not in r and r['obs'] is None
    out = eng.alloc_rollout(8, logp=True)
    out['logp'] = out['logp'].double()
    with pytest.raises(ValueError):
        eng.rollout_policy(8, actor, out=out)
    assert 'tanh' in eng.kernel_name() and 'policy' in eng.kernel_name()


def test_example_runs(tmp_path):
    ex = os.path.join(ROOT, 'gym-soccer-2d-env_amd', 'examples', 'ppo_reach_ball.py')
    r = subprocess.run([sys.executable, ex, '--envs', '1024', '--iters', '2', '--fused-actor', '32'], cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    losses = [float(line.split('loss')[1].split()[0]) for line in r.stdout.splitlines() if ' loss ' in line]
    assert len(losses) == 2 and all(np.isfinite(losses)), r.stdout[-3000:]
