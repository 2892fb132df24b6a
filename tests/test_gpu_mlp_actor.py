"""The fused actors on a general MLP (s2d_rollout_qnet_mlp / s2d_rollout_actor_mlp, s2d_debug_mlp_forward; MlpQNetActor /
MlpDeterministicActor): the network alone against the host restatement (tests/mlp_ref.c) bit for bit at every depth, at widths
that are not multiples of 16, at the tile / wave / workgroup edges and on edge values; equivalence with the two-layer path;
closed loops against the CPU oracle; graph replay with weights updated in place; agreement with a float64 forward; rejections."""
import ctypes as C
import itertools
import re

import numpy as np
import pytest

import actor_ref as R
import mlp_ref as M
import oracle as O
import qnet_ref as Q
from actor_refusals import refused

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
nn = torch.nn

F = np.float32
NOISE = {'off': dict(noise=False), 'lattice': dict(noise=True)}
MODES = {'discrete': dict(), 'cont1': dict(use_continuous_action=True, use_turning=False),
         'turn4': dict(use_continuous_action=True, use_turning=True)}
WIDTH_SETS = [(8,), (16, 8), (24, 40), (128, 64, 32, 16), (8, 128, 8), (64, 64, 64, 64)]
OUTPUTS = [1, 4, 16, 17, 64]
SIZES = [1, 63, 65, 257]


@pytest.fixture(scope='module')
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp('mlp_ref')
    return M.build(d), Q.build(d), R.build(d)


# ------------------------------------------------------------------------------------------------------------------ helpers
def views(p, hidden, na):
    """[W_1, b_1, ..., W_out, b_out]: writable views into the packed parameter vector p (nn.Sequential order)"""
    out, o, win = [], 0, 10
    for w in tuple(hidden) + (na,):
        for shape in ((w, win), (w,)):
            s = int(np.prod(shape))
            out.append(p[o:o + s].reshape(shape))
            o += s
        win = w
    return out


def random_net(rs, hidden, na):
    """weights and biases N(0, 1 / fan_in)"""
    p = np.zeros(M.param_count(hidden, na), dtype=F)
    fans = [f for w in (10,) + tuple(hidden) for f in (w, w)]
    for v, fan in zip(views(p, hidden, na), fans):
        v[...] = rs.normal(0, 1 / np.sqrt(fan), v.shape)
    return p


def random_obs(rs, n):
    x = rs.uniform(-1, 1, (n, 10))
    x[::4] *= 100                                     # a slice far outside the observation range
    return x.astype(F)


def shape_struct(hidden, na, act, params_ptr):
    from soccer2d_amd import _capi
    s = _capi.S2DMlpNet()
    s.n_hidden = len(hidden)
    for l, w in enumerate(hidden):
        s.hidden[l] = w
    s.n_out, s.activation, s.noise_kind, s.params = na, M.ACT[act], 0, params_ptr
    return s


def device_forward(params, x, hidden, na, act, pad=64):
    """(y [n][na], greedy [n], kernel name) of s2d_debug_mlp_forward; `pad` guard rows past n must stay untouched"""
    from soccer2d_amd import _capi
    lib = _capi.load_library()
    x = np.ascontiguousarray(x, dtype=F)
    n = x.shape[0]
    p = torch.from_numpy(np.ascontiguousarray(params, dtype=F)).to('cuda:0')
    xt = torch.from_numpy(x).to('cuda:0')
    y = torch.full((n + pad, na), -7777.0, dtype=torch.float32, device='cuda:0')
    g = torch.full((n + pad,), -5, dtype=torch.int32, device='cuda:0')
    name = C.create_string_buffer(96)
    s = shape_struct(hidden, na, act, p.data_ptr())
    torch.cuda.synchronize()
    _capi.check(lib, lib.s2d_debug_mlp_forward(C.byref(s), xt.data_ptr(), n, y.data_ptr(), g.data_ptr(), name, None),
                's2d_debug_mlp_forward')
    torch.cuda.synchronize()
    y, g = y.cpu().numpy(), g.cpu().numpy()
    assert (y[n:] == -7777.0).all() and (g[n:] == -5).all(), 'wrote past n'
    return y[:n], g[:n], name.value.decode()


def same(got, want, what):
    """bit for bit, the sign of zero included; where both are NaN only that they are NaN"""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype == F:
        gn, wn = np.isnan(got), np.isnan(want)
        bad = (gn != wn) | (~gn & ~wn & (got.view(np.int32) != want.view(np.int32)))
    else:
        bad = got != want
    if bad.any():
        idx = np.argwhere(bad)
        i = tuple(idx[0])
        raise AssertionError(f'{what}: {len(idx)} of {got.size} differ; first at {i}: gpu={got[i]!r} cpu={want[i]!r}')


def check(ml, params, x, hidden, na, act, what):
    """the device against mlp_ref's forward and argmax, and the kernel's name against the shape and the plan; returns y"""
    from soccer2d_amd.mlp_actor import lds_plan
    y, g, name = device_forward(params, x, hidden, na, act)
    want_name = (f's2d_debug_mlp_forward_kernel<act={act},h={"-".join(map(str, hidden))},a={na},'
                 f'waves={lds_plan(hidden, na)[0]}>')
    assert name == want_name, (name, want_name)
    want = M.forward(ml, x, params, hidden, na, act)
    same(y, want, f'{what} y')
    same(g, M.argmax(ml, want), f'{what} greedy')
    return y


# ---------------------------------------------------------------------------------------------------------- the network alone
# every width set with both activations; the outputs and the batch sizes go round, twice with another phase, so that every A
# and every n meets several depths: 24 cases
_COMBOS = list(itertools.product(WIDTH_SETS, ('relu', 'tanh')))
SWEEP = [(h, act, OUTPUTS[(i + r) % 5], SIZES[(i + 3 * r) % 4]) for r in (0, 2) for i, (h, act) in enumerate(_COMBOS)]


def test_sweep_covers_every_output_count_and_size():
    assert {c[2] for c in SWEEP} == set(OUTPUTS) and {c[3] for c in SWEEP} == set(SIZES)
    assert {len(c[0]) for c in SWEEP} == {1, 2, 3, 4}


@pytest.mark.parametrize('hidden,act,na,n', SWEEP, ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_network_alone(refs, hidden, act, na, n):
    rs = np.random.RandomState(sum(hidden) * 131 + na * 7 + n)
    y = check(refs[0], random_net(rs, hidden, na), random_obs(rs, n), hidden, na, act, f'{hidden} {act} a={na} n={n}')
    assert np.isfinite(y).all() and (n == 1 or len(np.unique(y)) > 1)


EDGE_SHAPES = [((8,), 4), ((24, 40), 17), ((16, 8, 24, 8), 1), ((128, 64, 32, 16), 16)]


def _identity_net(hidden, na, diag=1.0, bias=0.0):
    """every layer W[j][j mod fan_in] = diag, the rest zero; biases `bias`"""
    p = np.zeros(M.param_count(hidden, na), dtype=F)
    v = views(p, hidden, na)
    for W, b in zip(v[0::2], v[1::2]):
        for j in range(W.shape[0]):
            W[j, j % W.shape[1]] = diag
        b[...] = bias
    return p


@pytest.mark.parametrize('hidden,na', EDGE_SHAPES)
def test_minus_zero_through_a_tanh_network(refs, hidden, na):
    """layer 1's accumulator is exactly -0 (bias -0, products -0 * +0): its two padding terms make it +0, so +0 reaches the
    output through tanh_spec (odd: -0 would stay -0) and identity weights with -0 biases"""
    p = _identity_net(hidden, na, bias=-0.0)
    views(p, hidden, na)[0][...] = -0.0
    x = np.zeros((65, 10), dtype=F)
    y = check(refs[0], p, x, hidden, na, 'tanh', 'minus zero')
    assert (y == 0).all() and not np.signbit(y).any()
    # without the padding terms the sign would have come through: the restatement over k = 0 .. 9 shows -0 at the output
    y10 = M.forward(refs[0], x, p, hidden, na, 'tanh', first_k=10)
    assert np.signbit(y10[:, :min(na, hidden[-1])]).all()


@pytest.mark.parametrize('act', ['relu', 'tanh'])
@pytest.mark.parametrize('hidden,na', EDGE_SHAPES[:3])
def test_subnormals_are_kept(refs, hidden, na, act):
    x = np.full((63, 10), 1e-40, dtype=F)
    x[1::2] = 2.0 ** -149
    y = check(refs[0], _identity_net(hidden, na), x, hidden, na, act, 'subnormal')
    assert (y[:, 0] > 0).all() and (y[:, 0] < 2.0 ** -126).all()                # not flushed, not rounded away


@pytest.mark.parametrize('hidden,na', EDGE_SHAPES[:3])
def test_nan_and_overflow(refs, hidden, na):
    """relu(NaN) = +0, tanh_spec passes NaN on (a NaN input reaches every unit of layer 1: 0 * NaN = NaN); sums past 3.4e38
    overflow to +-inf"""
    ml = refs[0]
    x = np.ones((65, 10), dtype=F)
    x[::2, 0] = np.nan
    p = _identity_net(hidden, na)
    yr = check(ml, p, x, hidden, na, 'relu', 'nan relu')
    yt = check(ml, p, x, hidden, na, 'tanh', 'nan tanh')
    assert np.isfinite(yr).all() and (yr[::2, 0] == 0).all() and not np.signbit(yr[::2, 0]).any()
    assert np.isnan(yt[::2, 0]).all() and np.isfinite(yt[1::2]).all()
    # overflow in the output layer's chain: four terms of -+3e38 times hidden units of 10 (relu) or in (0.4, 1] (tanh_spec)
    big = _identity_net(hidden, na)
    Wo = views(big, hidden, na)[-2]
    Wo[...] = 0.0
    Wo[0, :4] = -3e38
    if na > 1:
        Wo[1, :4] = 3e38
    x = np.full((63, 10), 10.0, dtype=F)
    for act in ('relu', 'tanh'):
        y = check(ml, big, x, hidden, na, act, f'overflow {act}')
        assert np.isneginf(y[:, 0]).all() and (na == 1 or np.isposinf(y[:, 1]).all())


@pytest.mark.parametrize('act', ['relu', 'tanh'])
@pytest.mark.parametrize('hidden,na', [((24, 40, 8, 16), 17), ((8, 128, 8, 24), 4)])
def test_one_hot_routing_through_four_layers(refs, hidden, na, act):
    """every unit of every layer reads exactly one input, by a permutation of the layer below, with a weight of its own: a
    permuted k, a shifted fragment or a padded unit read by mistake changes the output"""
    rs = np.random.RandomState(5)
    p = np.zeros(M.param_count(hidden, na), dtype=F)
    v = views(p, hidden, na)
    for W, b in zip(v[0::2], v[1::2]):
        fan = W.shape[1]
        perm = rs.permutation(fan)
        for j in range(W.shape[0]):
            W[j, perm[(5 * j + 3) % fan]] = 0.5 + (j + 1) / 256.0
        b[...] = (np.arange(W.shape[0]) + 1) / 1024.0
    x = rs.uniform(0.25, 1.0, (65, 10)).astype(F)
    y = check(refs[0], p, x, hidden, na, act, 'one-hot')
    assert len(np.unique(y[0])) > min(na, 8) // 2


@pytest.mark.parametrize('hidden,at', [((8,), 5), ((24, 40), 17), ((24, 40), 33), ((128, 64, 32, 16), 12), ((16, 8, 24), 17)])
def test_cancellation_shows_ascending_k(refs, hidden, at):
    """the output layer over the last hidden layer's units, all exactly 1: 1 + 2^24 - 2^24 is 0 only if the terms enter in
    ascending k (2^24 - 2^24 + 1 = 1); `at` is the last of the three terms' k: they lie across two k-steps, across two groups of
    four k-steps (k = 15 | 16) and across the last group of four and the tail group of two (k = 31 | 32 of 40)"""
    na = 4
    for act, one in (('relu', 1.0), ('tanh', 20.0)):                            # tanh_spec(20) = 1 exactly
        p = np.zeros(M.param_count(hidden, na), dtype=F)
        v = views(p, hidden, na)
        v[2 * len(hidden) - 1][...] = one                                        # b_L: every unit of the last hidden layer = 1
        Wo = v[-2]
        Wo[0, at - 2:at + 1] = [1.0, 2.0 ** 24, -2.0 ** 24]                      # ascending: 0
        Wo[1, at - 2:at + 1] = [2.0 ** 24, -2.0 ** 24, 1.0]                      # this order: 1
        Wo[2, at - 2:at + 1] = [2.0 ** 24, 1.0, -2.0 ** 24]                      # 0 (2^24 + 1 rounds to 2^24)
        x = np.zeros((63, 10), dtype=F)
        y = check(refs[0], p, x, hidden, na, act, 'cancellation')
        assert (y[:, 0] == 0).all() and (y[:, 1] == 1).all() and (y[:, 2] == 0).all()


# ------------------------------------------------------------------------------------------ equivalence with the two-layer path
def _kw(mode, **over):
    kw = dict(O.DQN_KWARGS)
    kw.update(MODES[mode])
    kw.update(over)
    return kw


def _engine(n, mode='discrete', noise='off', **kw):
    from soccer2d_amd.engine import Engine, make_config
    return Engine(n, 'cuda:0', cfg=make_config(**NOISE[noise], **_kw(mode, **kw)))


def _oracle(n, mode='discrete', noise='off', seed=0x5EED, **kw):
    cfg = O.make_config(seed=seed, auto_reset=1, noise=int(NOISE[noise]['noise']), **_kw(mode, **kw))
    return O.OracleEngine(cfg, n, 'f32')


def _module(hidden, na, act, seed, tanh_head=False, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    layers, win = [], 10
    for w in hidden:
        layers += [nn.Linear(win, w), nn.Tanh() if act == 'tanh' else nn.ReLU()]
        win = w
    layers.append(nn.Linear(win, na))
    if tanh_head:
        layers.append(nn.Tanh())
    net = nn.Sequential(*layers)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * scale)
    return net


@pytest.mark.parametrize('h1,h2', [(64, 64), (48, 80), (128, 128)])
def test_debug_forward_equals_the_two_layer_kernel(h1, h2):
    from soccer2d_amd import _capi
    lib = _capi.load_library()
    rs = np.random.RandomState(h1 + h2)
    for na in (4, 16):
        p, x = random_net(rs, (h1, h2), na), random_obs(rs, 257)
        y, g, _ = device_forward(p, x, (h1, h2), na, 'relu')
        pt, xt = torch.from_numpy(p).to('cuda:0'), torch.from_numpy(x).to('cuda:0')
        y2 = torch.zeros((257, na), device='cuda:0')
        g2 = torch.zeros(257, dtype=torch.int32, device='cuda:0')
        _capi.check(lib, lib.s2d_debug_net_forward(h1, h2, na, pt.data_ptr(), xt.data_ptr(), 257, y2.data_ptr(), g2.data_ptr(),
                                                   None, None), 's2d_debug_net_forward')
        torch.cuda.synchronize()
        same(y, y2.cpu().numpy(), f'y {h1}-{h2}-{na}')
        same(g, g2.cpu().numpy(), f'greedy {h1}-{h2}-{na}')


RECORD = ('obs', 'action', 'reward', 'done', 'result', 'terminal_obs')


def _both_paths(mode, rollout, make_old, make_new):
    """the same launch through the two-layer and the general entry point on twin engines: every record word and the arena"""
    n, T = 150, 24
    engs = [_engine(n, mode, 'lattice'), _engine(n, mode, 'lattice')]
    outs = []
    for eng, make in zip(engs, (make_old, make_new)):
        eng.reset()
        eng.rollout(3)
        out = eng.alloc_rollout(T, terminal_obs=True)
        out['terminal_obs'].fill_(float('nan'))
        outs.append(getattr(eng, rollout)(T, make(), out=out))
    torch.cuda.synchronize()
    for k in RECORD:
        same(outs[1][k], outs[0][k].cpu().numpy(), f'record.{k}')
    assert torch.equal(engs[0].arena, engs[1].arena)
    return engs


def test_rollout_qnet_equals_the_two_layer_path():
    from soccer2d_amd.actor import QNetActor
    from soccer2d_amd.mlp_actor import MlpQNetActor
    net = _module((64, 64), 16, 'relu', 3).to('cuda:0')
    engs = _both_paths('discrete', 'rollout_qnet', lambda: QNetActor.from_module(net, epsilon=0.3),
                       lambda: MlpQNetActor.from_module(net, epsilon=0.3))
    assert engs[0].kernel_name().startswith('s2d_reach_qnet_rollout_kernel<')
    assert engs[1].kernel_name() == 's2d_mlp_qnet_rollout_kernel<noise=1,act=relu,h=64-64,a=16,waves=4>'


def test_rollout_actor_equals_the_two_layer_path():
    from soccer2d_amd.actor import DeterministicActor
    from soccer2d_amd.mlp_actor import MlpDeterministicActor
    net = _module((64, 64), 4, 'relu', 4, tanh_head=True, scale=0.5).to('cuda:0')
    kw = dict(epsilon=0.3, noise_sigma=0.2, noise_mean=0.05)
    engs = _both_paths('turn4', 'rollout_actor', lambda: DeterministicActor.from_module(net, **kw),
                       lambda: MlpDeterministicActor.from_module(net, **kw))
    assert engs[1].kernel_name() == 's2d_mlp_actor_rollout_kernel<mode=turn4,noise=1,gauss=1,act=relu,h=64-64,a=4,waves=4>'


# ---------------------------------------------------------------------------------------- closed loops against the CPU oracle
def _closed_loop(refs, mode, hidden, act, n, T, eps, noise, sigma=None, **task):
    from soccer2d_amd.mlp_actor import MlpDeterministicActor, MlpQNetActor
    ml, ql, _ = refs
    discrete = mode == 'discrete'
    na = 16 if discrete else 4 if mode == 'turn4' else 1
    eng, orc = _engine(n, mode, noise, **task), _oracle(n, mode, noise, **task)
    eng.reset(); orc.reset()
    eng.rollout(5); orc.rollout(5)
    net = _module(hidden, na, act, n + T + na, tanh_head=not discrete, scale=1.0 if discrete else 0.5).to('cuda:0')
    actor = (MlpQNetActor.from_module(net, epsilon=eps) if discrete
             else MlpDeterministicActor.from_module(net, epsilon=eps, noise_sigma=sigma))
    params = actor.params.cpu().numpy()
    noise_rows = None if discrete or actor.noise_kind == 0 else torch.stack([actor.noise_mean, actor.noise_sigma]).cpu().numpy()
    k0 = eng.policy_step.cpu().numpy().astype(np.int64)
    same(eng.policy_step, orc.state('policy_step'), 'policy_step before')
    out = eng.alloc_rollout(T, terminal_obs=True)
    out['terminal_obs'].fill_(float('nan'))                     # rows where no episode ended must stay untouched
    out = (eng.rollout_qnet if discrete else eng.rollout_actor)(T, actor, out=out)
    torch.cuda.synchronize()
    gid = np.arange(n, dtype=np.int64)
    obs = orc.obs()
    rec = {k: [] for k in ('obs', 'action', 'reward', 'done', 'result')}
    term = np.full((T, n, 10), np.nan, dtype=F)
    for t in range(T):
        if discrete:
            a = M.q_actions(ml, ql, obs, params, hidden, na, act, eps, eng.cfg.seed, gid, k0 + t)
        else:
            a = M.actor_actions(ml, obs, params, hidden, na, act, eps, actor.noise_kind, noise_rows, eng.cfg.seed, k0 + t)
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
    same(eng.policy_step, ((k0 + T) & 0xFFFFFFFF).astype(np.uint32).view(np.int32), 'policy_step = k0 + T')
    same(eng.obs, orc.obs(), 'obs'); same(eng.done, orc.done(), 'done'); same(eng.result, orc.result(), 'result')
    same(eng.stats[:4], orc.stats()[:4].astype(np.int64), 'stats')
    return eng, out


@pytest.mark.parametrize('noise', ['off', 'lattice'])
@pytest.mark.parametrize('eps', [0.0, 0.3, 1.0])
def test_qnet_closed_loop(refs, eps, noise):
    """[128, 64, 32, 16] Tanh, A = 16 (the reference's custom DQN model); max_steps = 12, so every env auto-resets at least
    twice in 40 cycles; eps = 1 is the random-policy rollout"""
    eng, out = _closed_loop(refs, 'discrete', (128, 64, 32, 16), 'tanh', 200, 40, eps, noise, max_steps=12)
    assert eng.kernel_name() == f's2d_mlp_qnet_rollout_kernel<noise={int(noise != "off")},act=tanh,h=128-64-32-16,a=16,waves=2>'
    assert int(out['done'].sum(dim=0).min()) >= 2
    if eps == 1.0:
        twin = _engine(200, 'discrete', noise, max_steps=12)
        twin.reset(); twin.rollout(5)
        r = twin.rollout(40)
        torch.cuda.synchronize()
        for k in ('obs', 'action', 'reward', 'done', 'result'):
            same(out[k], r[k].cpu().numpy(), f'random-policy rollout {k}')


@pytest.mark.parametrize('mode,hidden,act', [('cont1', (16, 8), 'relu'), ('turn4', (32, 32, 32), 'tanh')])
def test_tanh_actor_closed_loop(refs, mode, hidden, act):
    """pi [16, 8] ReLU on a continuous engine (the reference's DDPG script) and [32] * 3 Tanh on a turning one, Gaussian noise"""
    eng, out = _closed_loop(refs, mode, hidden, act, 130, 30, 0.1, 'lattice', sigma=0.2, max_steps=12)
    a = out['action'].cpu().numpy()
    assert len(np.unique(a)) > 100 and (np.abs(a) <= 1).all()
    assert eng.kernel_name() == (f's2d_mlp_actor_rollout_kernel<mode={mode},noise=1,gauss=1,act={act},'
                                 f'h={"-".join(map(str, hidden))},a={a.shape[-1]},waves=4>')


# ------------------------------------------------------------------------------------------------------------- graph capture
def test_graph_replay_reads_weights_and_epsilon_at_replay():
    from soccer2d_amd.mlp_actor import MlpQNetActor
    n, T, hidden = 300, 12, (24, 40, 8)
    eng = _engine(n, 'discrete', 'lattice')
    eng.reset()
    net1, net2 = _module(hidden, 16, 'tanh', 7).to('cuda:0'), _module(hidden, 16, 'tanh', 8).to('cuda:0')
    actor = MlpQNetActor.from_module(net1, epsilon=0.05)
    out = eng.alloc_rollout(T, terminal_obs=True)
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
    r = eng.rollout_qnet(T, MlpQNetActor.from_module(net2, epsilon=0.3))
    torch.cuda.synchronize()
    for k in got:
        same(got[k], r[k].cpu().numpy(), k)
    for f in state:
        same(state[f], getattr(eng, f).cpu().numpy(), f)
    eng.load_state_dict(sd)
    old = eng.rollout_qnet(T, MlpQNetActor.from_module(net1, epsilon=0.05))
    torch.cuda.synchronize()
    assert not torch.equal(old['action'], got['action'])       # the replay did not act with what the capture saw


# ------------------------------------------------------------------------------------------------------ agreement with float64
def gamma(k):
    u = 2.0 ** -24
    return k * u / (1 - k * u)


def f64_bound(params, x, hidden, na):
    """y64 (the tanh network in float64 on the same float32 inputs) and a rigorous bound on |y - y64| per output: the running
    bound of tests/test_gpu_actor_network.py per layer, e_pre = |W| e + gamma_K (|b| + |W| (|a| + e)) + K 2^-149 for a k-ordered
    fmaf chain of K terms (K = 12 in layer 1), and behind every hidden unit tanh_spec's stated 1e-6 against float64 tanh,
    carried on with tanh's Lipschitz constant 1: e = e_pre + 1e-6"""
    v = [t.astype(np.float64) for t in views(params.copy(), hidden, na)]
    a, e, K = x.astype(np.float64), np.zeros(x.shape), 12
    for l, (W, b) in enumerate(zip(v[0::2], v[1::2])):
        pre = a @ W.T + b
        e = e @ np.abs(W).T + gamma(K) * (np.abs(b) + (np.abs(a) + e) @ np.abs(W).T) + K * 2.0 ** -149
        if l < len(hidden):
            a, e = np.tanh(pre), e + 1e-6
        else:
            a = pre
        K = W.shape[0]
    return a, e


def test_greedy_agrees_with_a_float64_forward():
    """the greedy action of the 4-layer Tanh network is float64's argmax wherever float64's top-two gap exceeds twice the
    bound; rows inside it are only counted, and with these seeded weights float64 alone leaves at most 1 % of them there.
    The bound carries every hidden unit's 1e-6 through the absolute row sums of all the layers above it, about 0.8 sqrt(fan_in)
    each for dense Gaussian rows: 9 x 6.4 x 4.5 x 3.2 for this shape, which would put 3.5 % of the rows inside.  So every
    unit here reads 8 inputs of the layer below (row sums of 2.3), all 128-64-32-16 units and every k-step still in use."""
    hidden, na, n = (128, 64, 32, 16), 16, 4000
    rs = np.random.RandomState(11)
    params = np.zeros(M.param_count(hidden, na), dtype=F)
    for W, b in zip(views(params, hidden, na)[0::2], views(params, hidden, na)[1::2]):
        for j in range(W.shape[0]):                            # 8 inputs per unit, N(0, 1 / 8)
            W[j, rs.choice(W.shape[1], 8, replace=False)] = rs.normal(0, 1 / np.sqrt(8), 8)
        b[...] = rs.normal(0, 0.1, b.shape)
    net = _module(hidden, na, 'tanh', 0)
    with torch.no_grad():
        for p, v in zip(net.parameters(), views(params, hidden, na)):
            p.copy_(torch.from_numpy(v))
    x = rs.uniform(-1, 1, (n, 10)).astype(F)
    y64, e = f64_bound(params, x, hidden, na)
    with torch.no_grad():
        yt = net.double()(torch.from_numpy(x).double()).numpy()
    assert np.allclose(yt, y64, rtol=0, atol=1e-12)
    top = np.sort(y64, axis=1)
    clear = (top[:, -1] - top[:, -2]) > 2 * e.max(axis=1)
    inside = int((~clear).sum())
    print(f'rows inside the bound: {inside} of {n}; largest bound {e.max():.3g}')
    assert inside <= n // 100
    y, g, _ = device_forward(params, x, hidden, na, 'tanh')
    assert (np.abs(y - y64) <= e).all(), float((np.abs(y - y64) / e).max())
    assert np.array_equal(g[clear], y64.argmax(axis=1)[clear])


# ------------------------------------------------------------------------------------------------------------------ rejections
def test_rejections_leave_the_state_unchanged():
    from soccer2d_amd import _capi
    from soccer2d_amd.mlp_actor import MlpDeterministicActor, MlpQNetActor
    q = MlpQNetActor.from_module(_module((24, 40), 16, 'tanh', 1).to('cuda:0'), epsilon=0.1)
    mu1 = MlpDeterministicActor.from_module(_module((16, 8), 1, 'relu', 2, tanh_head=True).to('cuda:0'), noise_sigma=0.1)
    mu4 = MlpDeterministicActor.from_module(_module((16, 8), 4, 'relu', 2, tanh_head=True).to('cuda:0'), noise_sigma=0.1)
    ro = _capi.S2DRollout()

    def edits(net):
        """every struct the header refuses: (what, edit)"""
        def set_(**kw):
            def f(s):
                for k, v in kw.items():
                    setattr(s, k, v)
            return f

        def width(l, w):
            def f(s):
                s.hidden[l] = w
            return f
        return [('n_hidden 0', set_(n_hidden=0)), ('n_hidden 5', set_(n_hidden=5)), ('width 12', width(0, 12)),
                ('width 136', width(1, 136)), ('width 0', width(1, 0)), ('entry past n_hidden', width(3, 8)),
                ('activation 2', set_(activation=2)), ('activation -1', set_(activation=-1)),
                ('n_out', set_(n_out=net.n_out + 1)), ('params NULL', set_(params=None)),
                ('params misaligned', set_(params=net.params + 4)), ('epsilon NULL', set_(epsilon=None)),
                ('epsilon misaligned', set_(epsilon=net.epsilon + 2))]

    for mode, actor, entry in (('discrete', q, 's2d_rollout_qnet_mlp'), ('cont1', mu1, 's2d_rollout_actor_mlp'),
                               ('turn4', mu4, 's2d_rollout_actor_mlp')):
        eng = _engine(256, mode)
        eng.reset()
        before = eng.arena.clone()
        fn = getattr(eng.lib, entry)
        base = actor.c_struct()
        cases = edits(base)
        if mode == 'discrete':
            cases += [('noise_kind on the Q path', lambda s: setattr(s, 'noise_kind', 1))]
        else:
            cases += [('noise_kind 2', lambda s: setattr(s, 'noise_kind', 2)), ('noise NULL', lambda s: setattr(s, 'noise', None)),
                      ('noise misaligned', lambda s: setattr(s, 'noise', base.noise + 2))]
        for what, edit in cases:
            s = actor.c_struct()
            edit(s)
            refused(eng.lib, f'{entry}/struct/{mode}/{what}', fn(eng._h, 4, C.byref(s), C.byref(ro), None, eng._stream()))
        s = actor.c_struct()
        refused(eng.lib, f'{entry}/struct/{mode}/n_steps 0', fn(eng._h, 0, C.byref(s), C.byref(ro), None, eng._stream()))
        refused(eng.lib, f'{entry}/struct/{mode}/net NULL', fn(eng._h, 4, None, C.byref(ro), None, eng._stream()))
        # a shape that does not fit: the text says how many bytes it needs
        s = actor.c_struct()
        s.n_hidden = 3
        for l in range(3):
            s.hidden[l] = 128
        msg = refused(eng.lib, f'{entry}/struct/{mode}/10-128-128-128', fn(eng._h, 4, C.byref(s), C.byref(ro), None, eng._stream()))
        assert re.search(r'10-128-128-128-\d+ needs 1\d{5} bytes of LDS', msg), msg
        # the wrong engine mode, through both layers
        other = getattr(eng.lib, 's2d_rollout_actor_mlp' if mode == 'discrete' else 's2d_rollout_qnet_mlp')
        refused(eng.lib, f'{entry}/struct/{mode}/the other entry',
                other(eng._h, 4, C.byref(actor.c_struct()), C.byref(ro), None, eng._stream()))
        with pytest.raises(ValueError):
            if mode == 'discrete':
                eng.rollout_actor(4, mu1)
            else:
                eng.rollout_qnet(4, q)
        torch.cuda.synchronize()
        assert torch.equal(before, eng.arena), mode
    # the diagnostic refuses the same shapes, and bad pointers and counts
    lib = _capi.load_library()
    x = torch.zeros((4, 10), device='cuda:0')
    y = torch.zeros((4, 16), device='cuda:0')
    g = torch.zeros(4, dtype=torch.int32, device='cuda:0')
    for what, edit in edits(q.c_struct())[:8] + [('params NULL', lambda s: setattr(s, 'params', None))]:
        s = q.c_struct()
        edit(s)
        assert lib.s2d_debug_mlp_forward(C.byref(s), x.data_ptr(), 4, y.data_ptr(), g.data_ptr(), None, None) == _capi.S2D_EINVAL, what
    s = q.c_struct()
    assert lib.s2d_debug_mlp_forward(C.byref(s), x.data_ptr(), 0, y.data_ptr(), g.data_ptr(), None, None) == _capi.S2D_EINVAL
    assert lib.s2d_debug_mlp_forward(C.byref(s), None, 4, y.data_ptr(), g.data_ptr(), None, None) == _capi.S2D_EINVAL
    assert lib.s2d_debug_mlp_forward(C.byref(s), x.data_ptr() + 2, 4, y.data_ptr(), g.data_ptr(), None, None) == _capi.S2D_EINVAL
    assert lib.s2d_debug_mlp_forward(None, x.data_ptr(), 4, y.data_ptr(), g.data_ptr(), None, None) == _capi.S2D_EINVAL
