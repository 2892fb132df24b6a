"""The fused tanh actor (s2d_rollout_actor / Engine.rollout_actor) of continuous and turning engines: closed-loop bit parity
against the CPU oracle (the per-step API for the rcssserver noise model, which the oracle does not have) driven by the host
restatement of the policy (tests/actor_ref.c), the math-spec primitives bit for bit, equivalences with the existing rollout,
the device noise's distribution, graph replay with weights, epsilon and sigma updated in place, a float64 forward, other
shapes, rejections, and a short run of the example."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
import actor_ref as R
from actor_refusals import refused
from test_actor_host import chi2_phi

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE = {'off': dict(noise=False), 'lattice': dict(noise=True), 'square': dict(noise=True, noise_model='rcssserver')}
MODES = {'cont1': dict(use_continuous_action=True, use_turning=False), 'turn4': dict(use_continuous_action=True, use_turning=True)}
NA = {'cont1': 1, 'turn4': 4}


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return R.build(tmp_path_factory.mktemp('actor_ref'))


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

    def _np(self, t):
        torch.cuda.synchronize()
        return t.detach().cpu().numpy().copy()

    def reset(self):
        self.e.reset()

    def rollout(self, T):
        self.e.rollout(T)

    def step(self, a):
        o, r, d, res = self.e.step(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to('cuda:0'))
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


def _oracle(n, mode, noise='off', seed=0x5EED, env_id_offset=0, **kw):
    nz = NOISE[noise]
    if nz.get('noise_model') == 'rcssserver':
        return _StepEngine(n, mode, noise, seed=seed, env_id_offset=env_id_offset, **kw)
    cfg = O.make_config(seed=seed, env_id_offset=env_id_offset, auto_reset=1, noise=int(nz['noise']), **_kw(mode, **kw))
    return O.OracleEngine(cfg, n, 'f32')


def _mu(h1=64, h2=64, a=1, seed=0, scale=0.5):
    g = torch.Generator().manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(10, h1), torch.nn.ReLU(), torch.nn.Linear(h1, h2), torch.nn.ReLU(),
                              torch.nn.Linear(h2, a), torch.nn.Tanh())
    with torch.no_grad():
        for p in net.parameters():
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * scale)
    return net


def _actor(net, eps, sigma=None, mean=None):
    from soccer2d_amd.actor import DeterministicActor
    return DeterministicActor.from_module(net.to('cuda:0'), device='cuda:0', epsilon=eps, noise_sigma=sigma, noise_mean=mean)


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


def _noise_of(actor):
    return None if actor.noise_kind == 0 else torch.stack([actor.noise_mean, actor.noise_sigma]).cpu().numpy()


def int32_view(k):
    """uint32 counters (taken modulo 2^32) as the engine's int32 plane holds them"""
    return (np.asarray(k, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def _closed_loop_parity(ref, n, T, mode, eps, noise, sigma, warm=5, seed=0x5EED, h1=64, h2=64, k_set=None):
    na = NA[mode]
    eng = _engine(n, mode, noise, seed=seed)
    orc = _oracle(n, mode, noise, seed=seed)
    eng.reset(); orc.reset()
    if warm:
        eng.rollout(warm); orc.rollout(warm)
    if k_set is not None:
        eng.policy_step.copy_(torch.from_numpy(int32_view(k_set)).to('cuda:0'))
        if isinstance(orc, _StepEngine):
            orc.e.policy_step.copy_(torch.from_numpy(int32_view(k_set)).to('cuda:0'))
        else:
            orc.set_state('policy_step', k_set)
        same(eng.policy_step, orc.state('policy_step'), 'policy_step set')
    actor = _actor(_mu(h1, h2, na, seed=n + T + na), eps, sigma)
    params = actor.params.cpu().numpy()
    k0 = eng.policy_step.cpu().numpy().astype(np.int64)
    out = eng.alloc_rollout(T, terminal_obs=True)
    out['terminal_obs'].fill_(float('nan'))
    out = eng.rollout_actor(T, actor, out=out)
    torch.cuda.synchronize()
    obs = orc.obs()
    rec = {k: [] for k in ('obs', 'action', 'reward', 'done', 'result')}
    term = np.full((T, n, 10), np.nan, dtype=np.float32)
    for t in range(T):
        a = R.actions(ref, obs, params, h1, h2, na, eps, actor.noise_kind, _noise_of(actor), eng.cfg.seed, k0 + t)
        obs, rew, done, res = orc.step(a)
        for k, v in (('obs', obs), ('action', a), ('reward', rew), ('done', done), ('result', res)):
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
    same(eng.stats[:4], orc.stats()[:4].astype(np.int64), 'stats')
    return out


@pytest.mark.parametrize('sigma', [None, 0.1, 0.3])
@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('noise', ['off', 'lattice'])
@pytest.mark.parametrize('mode', ['cont1', 'turn4'])
def test_closed_loop_parity(ref, mode, noise, eps, sigma):
    out = _closed_loop_parity(ref, 4096, 64, mode, eps, noise, sigma)
    assert int(out['done'].sum()) > 0
    a = out['action'].cpu().numpy()
    assert len(np.unique(a)) > 100 and (np.abs(a) <= 1).all()


@pytest.mark.parametrize('mode,noise', [('cont1', 'lattice'), ('cont1', 'off'), ('turn4', 'lattice')])
def test_policy_counter_wraps_past_2_31_and_2_32(ref, mode, noise):
    """policy_step keys the exploration, the random action and the Gaussian noise (cont1: the block at k >> 2, cached over
    four cycles): a launch that carries it across 2^31 (the int32 view turns negative) and 2^32 (the counter wraps, and with
    it the cached block's counter) acts exactly as R.actions"""
    n = 600
    k = np.array([2 ** 32 - 1 - (i % 7) if i % 3 == 0 else 2 ** 31 - 2 for i in range(n)], dtype=np.int64)
    _closed_loop_parity(ref, n, 40, mode, 0.1, noise, 0.3, warm=3, k_set=k)


@pytest.mark.parametrize('mode', ['cont1', 'turn4'])
def test_closed_loop_parity_rcssserver_noise(ref, mode):
    _closed_loop_parity(ref, 2048, 32, mode, 0.1, 'square', 0.3)


def _debug(op, x, n_out):
    from soccer2d_amd import _capi
    lib = _capi.load_library()
    xt = torch.from_numpy(np.ascontiguousarray(x)).to('cuda:0')
    y = torch.zeros(n_out, dtype=torch.float32, device='cuda:0')
    n = x.shape[0]
    _capi.check(lib, lib.s2d_debug_eval(op, xt.data_ptr(), y.data_ptr(), n, None), 's2d_debug_eval')
    torch.cuda.synchronize()
    return y.cpu().numpy()


def test_debug_eval_primitives_equal_the_restatement(ref):
    f = np.float32
    x = np.concatenate([np.linspace(-12, 12, 300001, dtype=np.float32),
                        np.array([0.0, -0.0, np.nextafter(f(0.625), f(0)), 0.625, np.nextafter(f(0.625), f(1)), 9.0, -9.0,
                                  np.nextafter(f(9), f(10)), np.inf, -np.inf, np.nan], dtype=np.float32)])
    same(_debug(13, x, x.size), R.tanh(ref, x), 'tanh_spec')
    u = np.concatenate([np.linspace(2.0 ** -24, 1.0, 1 << 20).astype(np.float32),
                        np.float32(2.0) ** -np.arange(0, 126, dtype=np.float32), np.array([0.0, -1.0, np.nan, np.inf, 3e38],
                                                                                         dtype=np.float32)])
    same(_debug(14, u, u.size), R.log(ref, u), 'log_spec')
    n = 1 << 18
    rs = np.random.RandomState(5)
    gid = rs.randint(0, 2 ** 40, n, dtype=np.int64).astype(np.uint64)
    ctr = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    seed = 0x1234ABCD
    inp = np.stack([(gid & 0xFFFFFFFF).astype(np.uint32), (gid >> 32).astype(np.uint32), ctr,
                    np.full(n, seed, np.uint32)], axis=1)
    same(_debug(15, inp, 4 * n).reshape(n, 4), R.gauss(ref, seed, gid, ctr), 'gaussian block')


@pytest.mark.parametrize('mode', ['cont1', 'turn4'])
@pytest.mark.parametrize('noise', ['off', 'lattice'])
def test_epsilon_one_is_the_random_policy_rollout(mode, noise):
    n, T = 3000, 40
    a, b = _engine(n, mode, noise), _engine(n, mode, noise)
    a.reset(); b.reset()
    ra = a.rollout_actor(T, _actor(_mu(a=NA[mode]), 1.0, 0.3))
    rb = b.rollout(T)
    torch.cuda.synchronize()
    for k in ('obs', 'action', 'reward', 'done', 'result'):
        same(ra[k], rb[k].cpu().numpy(), k)
    for f in O.STATE_FIELDS:
        same(getattr(a, f), getattr(b, f).cpu().numpy(), f)
    same(a.stats, b.stats.cpu().numpy(), 'stats')


@pytest.mark.parametrize('mode', ['cont1', 'turn4'])
def test_zero_gaussian_equals_no_noise(mode):
    n, T = 2048, 32
    a, b = _engine(n, mode, 'lattice'), _engine(n, mode, 'lattice')
    a.reset(); b.reset()
    net = _mu(a=NA[mode], seed=2)
    ra = a.rollout_actor(T, _actor(net, 0.1, 0.0, 0.0))
    rb = b.rollout_actor(T, _actor(net, 0.1))
    torch.cuda.synchronize()
    assert torch.equal(ra['action'], rb['action'])                     # -0 and +0 compare equal
    for k in ('obs', 'reward', 'done', 'result'):
        same(ra[k], rb[k].cpu().numpy(), k)


@pytest.mark.parametrize('mode', ['cont1', 'turn4'])
def test_device_noise_is_gaussian(mode):
    n, T, sigma = 65536, 16, 0.05
    eng = _engine(n, mode, 'off')
    eng.reset()
    net = _mu(a=NA[mode], seed=4, scale=0.05)                           # small outputs: tanh + 5.77 sigma stays in (-1, 1)
    actor = _actor(net, 0.0, sigma)
    obs0 = eng.obs.clone()
    r = eng.rollout_actor(T, actor)
    torch.cuda.synchronize()
    x = torch.cat([obs0[None], r['obs'][:-1]])
    with torch.no_grad():
        y = torch.cat([net[:5](x[t]) for t in range(T)]).reshape(T, n, -1)
    eng_tanh = torch.tanh(y.double())
    a = r['action'].double()
    assert float((a.abs() < 1).float().mean()) == 1.0
    z = ((a - eng_tanh) / sigma).reshape(-1).cpu().numpy()
    assert z.size >= 1 << 20
    assert abs(z.mean()) < 0.01 and abs(z.var() - 1) < 0.01
    stat, limit = chi2_phi(z)
    assert stat < limit, (stat, limit)


@pytest.mark.parametrize('mode', ['cont1', 'turn4'])
def test_greedy_agrees_with_a_float64_torch_forward(mode):
    n, T = 8192, 32
    eng = _engine(n, mode, 'lattice')
    eng.reset()
    net = _mu(a=NA[mode], seed=11)
    obs0 = eng.obs.clone()
    r = eng.rollout_actor(T, _actor(net, 0.0))
    torch.cuda.synchronize()
    x = torch.cat([obs0[None], r['obs'][:-1]]).double()
    with torch.no_grad():
        want = net.to('cuda:0').double()(x)
    assert float((want - r['action'].double()).abs().max()) <= 1e-5


def test_chaining():
    n = 2048
    a, b = _engine(n, 'turn4', 'lattice'), _engine(n, 'turn4', 'lattice')
    a.reset(); b.reset()
    actor = _actor(_mu(a=4, seed=3), 0.1, 0.2)
    r1 = a.rollout_actor(33, actor, terminal_obs=True)
    r2 = a.rollout_actor(31, actor, terminal_obs=True)
    r = b.rollout_actor(64, actor, terminal_obs=True)
    torch.cuda.synchronize()
    for k in ('obs', 'action', 'reward', 'done', 'result'):
        same(torch.cat([r1[k], r2[k]]), r[k].cpu().numpy(), k)
    d = torch.cat([r1['done'], r2['done']]).bool()
    same(torch.cat([r1['terminal_obs'], r2['terminal_obs']])[d], r['terminal_obs'][d].cpu().numpy(), 'terminal_obs')
    for f in O.STATE_FIELDS:
        same(getattr(a, f), getattr(b, f).cpu().numpy(), f)


def test_sharding():
    n, T = 4096, 32
    full = _engine(n, 'cont1', 'lattice')
    halves = [_engine(n // 2, 'cont1', 'lattice', env_id_offset=0), _engine(n // 2, 'cont1', 'lattice', env_id_offset=n // 2)]
    actor = _actor(_mu(seed=5), 0.1, 0.3)
    full.reset(); [h.reset() for h in halves]
    rf = full.rollout_actor(T, actor)
    rh = [h.rollout_actor(T, actor) for h in halves]
    torch.cuda.synchronize()
    for k in ('obs', 'action', 'reward', 'done', 'result'):
        same(torch.cat([rh[0][k], rh[1][k]], dim=1), rf[k].cpu().numpy(), k)


def test_graph_replay_reads_weights_epsilon_and_sigma_at_replay():
    n, T = 4096, 16
    eng = _engine(n, 'turn4', 'lattice')
    eng.reset()
    net1, net2 = _mu(a=4, seed=7).to('cuda:0'), _mu(a=4, seed=8).to('cuda:0')
    actor = _actor(net1, 0.05, 0.1)
    out = eng.alloc_rollout(T, terminal_obs=True)
    eng.rollout_actor(T, actor, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.rollout_actor(T, actor, out=out)
    torch.cuda.synchronize()
    actor.load_from(net2)
    actor.epsilon = 0.3
    actor.noise_sigma = [0.2, 0.3, 0.4, 0.5]
    sd = eng.state_dict()
    g.replay()
    torch.cuda.synchronize()
    got = {k: out[k].clone() for k in ('obs', 'action', 'reward', 'done', 'result')}
    state = {f: getattr(eng, f).clone() for f in O.STATE_FIELDS}
    eng.load_state_dict(sd)
    r = eng.rollout_actor(T, _actor(net2, 0.3, [0.2, 0.3, 0.4, 0.5]))
    torch.cuda.synchronize()
    for k in got:
        same(got[k], r[k].cpu().numpy(), k)
    for f in state:
        same(state[f], getattr(eng, f).cpu().numpy(), f)


@pytest.mark.parametrize('n', [1, 63, 1000, 4097])
def test_ragged_sizes(ref, n):
    _closed_loop_parity(ref, n, 9, 'turn4', 0.1, 'lattice', 0.3, warm=3)


@pytest.mark.parametrize('h1,h2', [(16, 16), (128, 128), (64, 32), (48, 80), (112, 96)])
@pytest.mark.parametrize('mode', ['cont1', 'turn4'])
def test_other_shapes(ref, mode, h1, h2):
    _closed_loop_parity(ref, 1000, 6, mode, 0.1, 'lattice', 0.3, warm=2, h1=h1, h2=h2)


def test_rejections_leave_the_state_unchanged():
    from soccer2d_amd import _capi
    from soccer2d_amd.actor import DeterministicActor
    actor = _actor(_mu(), 0.1, 0.2)
    eng = _engine(256, 'cont1', 'off')
    eng.reset()
    before = eng.arena.clone()
    ro = _capi.S2DRollout()

    def rc(net, T=4):
        return eng.lib.s2d_rollout_actor(eng._h, T, C.byref(net), C.byref(ro), None, eng._stream())
    for h1, h2, na, kind in ((40, 64, 1, 0), (256, 64, 1, 0), (400, 300, 1, 0), (64, 0, 1, 0), (64, 64, 4, 0), (64, 64, 2, 0),
                             (64, 64, 1, 2), (64, 64, 1, -1)):
        net = actor.c_struct()
        net.hidden1, net.hidden2, net.n_out, net.noise_kind = h1, h2, na, kind
        refused(eng.lib, f's2d_rollout_actor/struct/{h1}-{h2}-{na} noise_kind {kind}', rc(net))
    for field, val in (('params', actor.params.data_ptr() + 4), ('params', None), ('epsilon', None),
                       ('epsilon', actor.epsilon_tensor.data_ptr() + 2), ('noise', None)):
        net = actor.c_struct()
        setattr(net, field, val)
        refused(eng.lib, f's2d_rollout_actor/struct/{field} {"NULL" if val is None else "misaligned"}', rc(net))
    refused(eng.lib, 's2d_rollout_actor/struct/n_steps 0', rc(actor.c_struct(), T=0))
    with pytest.raises(ValueError):
        eng.rollout_actor(4, DeterministicActor(64, 64, 4))
    torch.cuda.synchronize()
    assert torch.equal(before, eng.arena)
    t4 = _engine(256, 'turn4', 'off')
    t4.reset()
    before4 = t4.arena.clone()
    with pytest.raises(ValueError):
        t4.rollout_actor(4, actor)
    assert torch.equal(before4, t4.arena)
    # discrete engines: rejected by s2d_rollout_actor; rollout_qnet still refuses continuous engines
    from soccer2d_amd.engine import Engine, make_config
    from soccer2d_amd.actor import QNetActor
    d = Engine(256, 'cuda:0', cfg=make_config(noise=False, **O.DQN_KWARGS))
    d.reset()
    dbefore = d.arena.clone()
    refused(d.lib, 's2d_rollout_actor/struct/discrete engine',
            d.lib.s2d_rollout_actor(d._h, 4, C.byref(actor.c_struct()), C.byref(ro), None, d._stream()))
    with pytest.raises(ValueError):
        d.rollout_actor(4, actor)
    q = torch.nn.Sequential(torch.nn.Linear(10, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(),
                            torch.nn.Linear(64, 16)).to('cuda:0')
    with pytest.raises(ValueError):
        eng.rollout_qnet(4, QNetActor.from_module(q, device='cuda:0'))
    torch.cuda.synchronize()
    assert torch.equal(dbefore, d.arena) and torch.equal(before, eng.arena)


def test_vec_env_dispatch():
    from soccer2d_amd.vec_env import Soccer2DVecEnv
    venv = Soccer2DVecEnv(256, **_kw('turn4'))
    venv.reset()
    r = venv.rollout(8, policy=_actor(_mu(a=4), 0.1, 0.1), terminal_obs=True)
    torch.cuda.synchronize()
    assert r['action'].shape == (8, 256, 4) and r['terminal_obs'].shape == (8, 256, 10)


def test_example_runs(tmp_path):
    ex = os.path.join(ROOT, 'gym-soccer-2d-env_amd', 'examples', 'ddpg_reach_ball.py')
    r = subprocess.run([sys.executable, ex, '--envs', '1024', '--iters', '2', '--fused-actor', '32'], cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert 'goal share' in r.stdout
