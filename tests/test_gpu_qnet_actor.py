"""The fused epsilon-greedy Q-network actor (s2d_rollout_qnet / Engine.rollout_qnet): closed-loop bit parity against the CPU
oracle (the per-step API for the rcssserver noise model, which the oracle does not have) driven by the host restatement of the
policy (tests/qnet_ref.c), equivalences with the existing rollout, graph replay
with weights updated in place, agreement with a float64 torch forward, other network shapes and rejections."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import qnet_ref as Q
from actor_refusals import refused

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

NOISE = {'off': dict(noise=False), 'lattice': dict(noise=True), 'square': dict(noise=True, noise_model='rcssserver')}


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return Q.build(tmp_path_factory.mktemp('qnet_ref'))


def _kw(**over):
    kw = dict(O.DQN_KWARGS)
    kw.update(over)
    return kw


def _engine(n, noise='off', **kw):
    from soccer2d_amd.engine import Engine, make_config
    return Engine(n, 'cuda:0', cfg=make_config(**NOISE[noise], **_kw(**kw)))


class _StepEngine:
    """The GPU per-step API (s2d_step with caller actions) behind the oracle's interface: the reference for the rcssserver noise
    model, which the CPU oracle does not implement (its step parity with that model is tests/test_gpu_noise_model.py's)."""

    def __init__(self, n, noise, **kw):
        self.e = _engine(n, noise, **kw)

    def _np(self, t):
        torch.cuda.synchronize()
        return t.detach().cpu().numpy().copy()

    def reset(self):
        self.e.reset()

    def rollout(self, T):
        self.e.rollout(T)

    def step(self, a):
        o, r, d, res = self.e.step(torch.from_numpy(np.asarray(a, dtype=np.int32)).to('cuda:0'))
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


def _oracle(n, noise='off', seed=0x5EED, env_id_offset=0, **kw):
    nz = NOISE[noise]
    if nz.get('noise_model') == 'rcssserver':
        return _StepEngine(n, noise, seed=seed, env_id_offset=env_id_offset, **kw)
    cfg = O.make_config(seed=seed, env_id_offset=env_id_offset, auto_reset=1, noise=int(nz['noise']), **_kw(**kw))
    return O.OracleEngine(cfg, n, 'f32')


def _net(h1=64, h2=64, na=16, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(10, h1), torch.nn.ReLU(), torch.nn.Linear(h1, h2), torch.nn.ReLU(),
                              torch.nn.Linear(h2, na))
    with torch.no_grad():
        for p in net.parameters():
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * scale)
    return net


def _actor(net, eps):
    from soccer2d_amd.actor import QNetActor
    return QNetActor.from_module(net.to('cuda:0'), device='cuda:0', epsilon=eps)


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


def _record(eng, T, terminal=True):
    out = eng.alloc_rollout(T, terminal_obs=terminal)
    if terminal:
        out['terminal_obs'].fill_(float('nan'))     # rows where no episode ended must stay untouched
    return out


def wrap_counters(n):
    """policy_step values that cross 2^32 (every third env) and 2^31 (the others) within a 40-cycle launch"""
    return np.array([2 ** 32 - 1 - (i % 7) if i % 3 == 0 else 2 ** 31 - 2 for i in range(n)], dtype=np.int64)


def int32_view(k):
    """uint32 counters (taken modulo 2^32) as the engine's int32 plane holds them"""
    return (np.asarray(k, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def _closed_loop_parity(ref, n, T, eps, noise, warm=5, seed=0x5EED, auto_reset=True, with_obs=True, k_set=None):
    kw = dict(seed=seed)
    eng = _engine(n, noise, auto_reset=auto_reset, **kw)
    orc = _oracle(n, noise, **kw) if auto_reset else O.OracleEngine(
        O.make_config(seed=seed, auto_reset=0, noise=int(NOISE[noise]['noise']), **_kw()), n, 'f32')
    eng.reset(); orc.reset()
    if warm:
        eng.rollout(warm); orc.rollout(warm)
    if k_set is not None:
        eng.policy_step.copy_(torch.from_numpy(int32_view(k_set)).to('cuda:0'))
        if isinstance(orc, _StepEngine):
            orc.e.policy_step.copy_(torch.from_numpy(int32_view(k_set)).to('cuda:0'))
        else:
            orc.set_state('policy_step', k_set)
    net = _net(seed=n + T)
    actor = _actor(net, eps)
    params = actor.params.cpu().numpy()
    k0 = eng.policy_step.cpu().numpy().astype(np.int64)
    same(eng.policy_step, orc.state('policy_step'), 'policy_step before')
    out = _record(eng, T)
    if not with_obs:
        out['obs'] = None
    out = eng.rollout_qnet(T, actor, out=out)
    torch.cuda.synchronize()
    gid = np.arange(n, dtype=np.int64)
    obs = orc.obs()
    rec = {k: [] for k in ('obs', 'action', 'reward', 'done', 'result')}
    term = np.full((T, n, 10), np.nan, dtype=np.float32)
    for t in range(T):
        a = Q.actions(ref, obs, params, 64, 64, 16, eps, eng.cfg.seed, gid, k0 + t)
        obs, rew, done, res = orc.step(a)
        for k, v in (('obs', obs), ('action', a), ('reward', rew), ('done', done), ('result', res)):
            rec[k].append(v)
        d = done != 0
        term[t][d] = (orc.terminal_obs() if auto_reset else obs)[d]   # without auto-reset the step returns the terminal one
    for k in rec:
        if out[k] is None:
            continue
        same(out[k], np.stack(rec[k]), f'record.{k}')
    same(out['terminal_obs'], term, 'record.terminal_obs')
    for f in O.STATE_FIELDS:
        if f == 'policy_step':
            continue
        same(getattr(eng, f), orc.state(f), f'state.{f}')
    same(eng.policy_step, int32_view(k0 + T), 'policy_step = k0 + T (mod 2^32)')
    same(eng.obs, orc.obs(), 'obs'); same(eng.done, orc.done(), 'done'); same(eng.result, orc.result(), 'result')
    same(eng.stats[:4], orc.stats()[:4].astype(np.int64), 'stats')
    return out


@pytest.mark.parametrize('noise', ['lattice', 'square'])
@pytest.mark.parametrize('eps', [0.1, 0.5])
def test_policy_counter_wraps_past_2_31_and_2_32(ref, noise, eps):
    """policy_step is a uint32 keying every POLICY and noise draw: an actor launch that carries it across 2^31 (the int32
    view turns negative) and 2^32 (the counter wraps) acts and moves exactly as the oracle driven by Q.actions"""
    n, T = 600, 40
    _closed_loop_parity(ref, n, T, eps, noise, warm=3, k_set=wrap_counters(n))


@pytest.mark.parametrize('noise', ['off', 'lattice', 'square'])
@pytest.mark.parametrize('eps', [0.0, 0.1])
def test_closed_loop_parity(ref, noise, eps):
    out = _closed_loop_parity(ref, 8192, 128, eps, noise)
    assert int(out['done'].sum()) > 0
    acts = out['action'].cpu().numpy()
    assert len(np.unique(acts)) > 4                  # the network and the exploration both pick various actions


def test_without_auto_reset_and_without_obs_record(ref):
    out = _closed_loop_parity(ref, 2048, 40, 0.1, 'lattice', auto_reset=False)
    assert int(out['done'].sum()) > 0
    _closed_loop_parity(ref, 2048, 40, 0.1, 'off', with_obs=False)


def test_record_buffers_are_checked():
    eng = _engine(256, 'off')
    eng.reset()
    actor = _actor(_net(), 0.1)
    for name, bad in (('terminal_obs', torch.zeros(4, 256, 10, dtype=torch.float16, device='cuda:0')),
                      ('terminal_obs', torch.zeros(4, 256, 4, device='cuda:0')),
                      ('obs', torch.zeros(4, 256, 4, device='cuda:0')),
                      ('action', torch.zeros(4, 256, dtype=torch.int64, device='cuda:0')),
                      ('reward', torch.zeros(4, 256, 2, device='cuda:0'))):
        out = eng.alloc_rollout(4, terminal_obs=True)
        out[name] = bad
        with pytest.raises(ValueError):
            eng.rollout_qnet(4, actor, out=out)
    from soccer2d_amd.vec_env import Soccer2DVecEnv
    venv = Soccer2DVecEnv(64, **_kw())
    venv.reset()
    with pytest.raises(ValueError):
        venv.rollout(4, terminal_obs=True)


@pytest.mark.parametrize('n', [1, 63, 1000, 4097])
def test_ragged_sizes(ref, n):
    _closed_loop_parity(ref, n, 9, 0.1, 'lattice', warm=3)


@pytest.mark.parametrize('noise', ['off', 'lattice', 'square'])
def test_epsilon_one_is_the_random_policy_rollout(noise):
    n, T = 3000, 40
    a, b = _engine(n, noise), _engine(n, noise)
    a.reset(); b.reset()
    actor = _actor(_net(), 1.0)
    ra = a.rollout_qnet(T, actor)
    rb = b.rollout(T)
    torch.cuda.synchronize()
    for k in ('obs', 'action', 'reward', 'done', 'result'):
        same(ra[k], rb[k].cpu().numpy(), k)
    for f in O.STATE_FIELDS:
        same(getattr(a, f), getattr(b, f).cpu().numpy(), f)
    same(a.stats, b.stats.cpu().numpy(), 'stats')


def test_chaining():
    n = 2048
    a, b = _engine(n, 'lattice'), _engine(n, 'lattice')
    a.reset(); b.reset()
    actor = _actor(_net(seed=3), 0.1)
    r1 = a.rollout_qnet(64, actor, terminal_obs=True)
    r2 = a.rollout_qnet(64, actor, terminal_obs=True)
    r = b.rollout_qnet(128, actor, terminal_obs=True)
    torch.cuda.synchronize()
    for k in ('obs', 'action', 'reward', 'done', 'result'):
        same(torch.cat([r1[k], r2[k]]), r[k].cpu().numpy(), k)
    d = torch.cat([r1['done'], r2['done']]).bool()
    same(torch.cat([r1['terminal_obs'], r2['terminal_obs']])[d], r['terminal_obs'][d].cpu().numpy(), 'terminal_obs')
    for f in O.STATE_FIELDS:
        same(getattr(a, f), getattr(b, f).cpu().numpy(), f)


def test_sharding():
    n, T = 4096, 32
    full = _engine(n, 'lattice')
    halves = [_engine(n // 2, 'lattice', env_id_offset=0), _engine(n // 2, 'lattice', env_id_offset=n // 2)]
    actor = _actor(_net(seed=5), 0.1)
    full.reset(); [h.reset() for h in halves]
    rf = full.rollout_qnet(T, actor)
    rh = [h.rollout_qnet(T, actor) for h in halves]
    torch.cuda.synchronize()
    for k in ('obs', 'action', 'reward', 'done', 'result'):
        same(torch.cat([rh[0][k], rh[1][k]], dim=1), rf[k].cpu().numpy(), k)


def test_graph_replay_reads_weights_and_epsilon_at_replay():
    n, T = 4096, 16
    eng = _engine(n, 'lattice')
    eng.reset()
    net1, net2 = _net(seed=7).to('cuda:0'), _net(seed=8).to('cuda:0')
    actor = _actor(net1, 0.05)
    out = _record(eng, T)
    eng.rollout_qnet(T, actor, out=out)              # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.rollout_qnet(T, actor, out=out)
    torch.cuda.synchronize()
    actor.load_from(net2)
    actor.epsilon = 0.3
    sd = eng.state_dict()
    g.replay()
    torch.cuda.synchronize()
    got = {k: out[k].clone() for k in ('obs', 'action', 'reward', 'done', 'result')}
    state = {f: getattr(eng, f).clone() for f in O.STATE_FIELDS}
    eng.load_state_dict(sd)
    ref_actor = _actor(net2, 0.3)
    r = eng.rollout_qnet(T, ref_actor)
    torch.cuda.synchronize()
    for k in got:
        same(got[k], r[k].cpu().numpy(), k)
    for f in state:
        same(state[f], getattr(eng, f).cpu().numpy(), f)


def test_greedy_agrees_with_a_float64_torch_forward():
    n, T = 8192, 32
    eng = _engine(n, 'lattice')
    eng.reset()
    net = _net(seed=11)
    actor = _actor(net, 0.0)
    obs0 = eng.obs.clone()
    r = eng.rollout_qnet(T, actor)
    torch.cuda.synchronize()
    x = torch.cat([obs0[None], r['obs'][:-1]]).double()          # the observation each action was chosen from
    net64 = net.to('cuda:0').double()
    with torch.no_grad():
        q = net64(x)
    top2 = torch.topk(q, 2, dim=-1).values
    clear = (top2[..., 0] - top2[..., 1]) > 1e-3 * q.abs().amax(dim=-1)
    agree = (q.argmax(dim=-1) == r['action'].long()) | ~clear
    assert bool(agree.all()), int((~agree).sum())
    assert float(clear.float().mean()) > 0.9


@pytest.mark.parametrize('h1,h2', [(16, 16), (128, 128), (64, 32), (48, 80), (112, 96), (80, 112)])
@pytest.mark.parametrize('na', [1, 2, 17, 33, 48, 64])
def test_other_shapes(ref, h1, h2, na):
    n, T = 1000, 6
    eng = _engine(n, 'lattice', action_space_size=na)
    eng.reset()
    net = _net(h1, h2, na, seed=h1 + h2 + na)
    actor = _actor(net, 0.1)
    params = actor.params.cpu().numpy()
    k0 = eng.policy_step.cpu().numpy().astype(np.int64)
    obs = eng.obs.cpu().numpy()
    r = eng.rollout_qnet(T, actor)
    torch.cuda.synchronize()
    gid = np.arange(n, dtype=np.int64)
    for t in range(T):
        want = Q.actions(ref, obs, params, h1, h2, na, 0.1, eng.cfg.seed, gid, k0 + t)
        same(r['action'][t], want, f'action[{t}]')
        obs = r['obs'][t].cpu().numpy()


def test_rejections_leave_the_state_unchanged():
    from soccer2d_amd import _capi
    from soccer2d_amd.actor import QNetActor
    actor = _actor(_net(), 0.1)
    for kw in (dict(use_continuous_action=True), dict(use_continuous_action=True, use_turning=True)):
        eng = _engine(256, 'off', **kw)
        eng.reset()
        before = eng.arena.clone()
        with pytest.raises(ValueError):
            eng.rollout_qnet(4, actor)
        torch.cuda.synchronize()
        assert torch.equal(before, eng.arena)
    eng = _engine(256, 'off')
    eng.reset()
    before = eng.arena.clone()
    ro = _capi.S2DRollout()
    for h1, h2, na, bad_ptr in ((40, 64, 16, False), (256, 64, 16, False), (64, 64, 8, False), (64, 0, 16, False),
                                (64, 64, 16, True)):
        net = actor.c_struct()
        net.hidden1, net.hidden2, net.n_actions = h1, h2, na
        if bad_ptr:
            net.params = actor.params.data_ptr() + 4
        rc = eng.lib.s2d_rollout_qnet(eng._h, 4, C.byref(net), C.byref(ro), None, eng._stream())
        refused(eng.lib, f's2d_rollout_qnet/struct/{h1}-{h2}-{na}' + '/params + 4' * bad_ptr, rc)
    net = actor.c_struct()
    refused(eng.lib, 's2d_rollout_qnet/struct/n_steps 0', eng.lib.s2d_rollout_qnet(eng._h, 0, C.byref(net), C.byref(ro), None, eng._stream()))
    net.epsilon = None
    refused(eng.lib, 's2d_rollout_qnet/struct/epsilon NULL', eng.lib.s2d_rollout_qnet(eng._h, 4, C.byref(net), C.byref(ro), None, eng._stream()))
    with pytest.raises(ValueError):
        eng.rollout_qnet(4, QNetActor(64, 64, 8))
    torch.cuda.synchronize()
    assert torch.equal(before, eng.arena)


@pytest.mark.parametrize('eps', [2.0 ** -33, 2.0 ** -32, 1 - 2.0 ** -24, 1.0, 1.5, -0.0, float('nan'), float('inf')],
                         ids=['2^-33', '2^-32', '1-2^-24', '1', '1.5', '-0', 'nan', 'inf'])
def test_epsilon_edges(ref, eps):
    """the device threshold of epsilons at the edges (rounding to 0 or 1 in 2^32 units, 1 - ulp, >= 1, -0, NaN, inf): the
    actions equal Q.actions bit for bit"""
    n, T = 4096, 6
    eng = _engine(n, 'lattice')
    eng.reset()
    actor = _actor(_net(seed=21), eps)
    params = actor.params.cpu().numpy()
    k0 = eng.policy_step.cpu().numpy().astype(np.int64)
    obs = eng.obs.cpu().numpy()
    r = eng.rollout_qnet(T, actor)
    torch.cuda.synchronize()
    gid = np.arange(n, dtype=np.int64)
    for t in range(T):
        want = Q.actions(ref, obs, params, 64, 64, 16, eps, eng.cfg.seed, gid, k0 + t)
        same(r['action'][t], want, f'action[{t}]')
        obs = r['obs'][t].cpu().numpy()
