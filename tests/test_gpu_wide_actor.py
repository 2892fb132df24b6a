"""The fused actors on the streamed-weight MLP (s2d_rollout_qnet_wide / s2d_rollout_actor_wide, s2d_debug_wide_forward;
WideQNetActor / WideDeterministicActor): the network alone against the host restatement (tests/wide_ref.c) word for word at
every k-step tail, tile-group count, depth, output count and batch edge, on special values, under every admissible plan, and
against the resident kernels; closed loops against the CPU oracle; graph replay with weights updated in place; rejections;
agreement with a float64 forward."""
import ctypes as C

import numpy as np
import pytest

import mlp_ref as M
import oracle as O
import qnet_ref as Q
from actor_refusals import refused
import wide_f64 as W64
import wide_ref as W
from test_gpu_qnet_actor import _StepEngine
from wide_f64 import random_net, views

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
nn = torch.nn

F = np.float32
NOISE = {'off': dict(noise=False), 'lattice': dict(noise=True), 'square': dict(noise=True, noise_model='rcssserver')}
MODES = {'discrete': dict(), 'cont1': dict(use_continuous_action=True, use_turning=False),
         'turn4': dict(use_continuous_action=True, use_turning=True)}
ACT_NN = {'relu': nn.ReLU, 'tanh': nn.Tanh, 'sigmoid': nn.Sigmoid}


@pytest.fixture(scope='module')
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp('wide_ref')
    return W.build(d), M.build(d), Q.build(d)


# ------------------------------------------------------------------------------------------------------------------ helpers
def random_obs(rs, n):
    x = rs.uniform(-1, 1, (n, 10))
    x[::4] *= 100                                     # a slice far outside the observation range
    return x.astype(F)


def hname(hidden):
    return '-'.join(map(str, hidden))


def shape_struct(hidden, na, act, params, workspace):
    from soccer2d_amd import _capi
    s = _capi.S2DWideNet()
    s.n_hidden = len(hidden)
    for l, w in enumerate(hidden):
        s.hidden[l] = w
    s.n_out, s.activation, s.noise_kind, s.params = na, W.ACT[act], 0, params.data_ptr()
    s.workspace, s.workspace_bytes = workspace.data_ptr(), workspace.numel() * 4
    return s


def device_forward(params, x, hidden, na, act, pad=64):
    """(y [n][na], greedy [n], kernel name) of s2d_debug_wide_forward; `pad` guard rows past n and 64 guard words past the
    workspace must stay untouched"""
    from soccer2d_amd import _capi
    from soccer2d_amd.wide_actor import wide_plan
    lib = _capi.load_library()
    x = np.ascontiguousarray(x, dtype=F)
    n = x.shape[0]
    p = torch.from_numpy(np.ascontiguousarray(params, dtype=F)).to('cuda:0')
    xt = torch.from_numpy(x).to('cuda:0')
    y = torch.full((n + pad, na), -7777.0, dtype=torch.float32, device='cuda:0')
    g = torch.full((n + pad,), -5, dtype=torch.int32, device='cuda:0')
    words = wide_plan(hidden, na)[3] // 4
    ws = torch.full((words + 64,), -3333.0, dtype=torch.float32, device='cuda:0')
    name = C.create_string_buffer(96)
    s = shape_struct(hidden, na, act, p, ws)
    s.workspace_bytes = words * 4
    torch.cuda.synchronize()
    _capi.check(lib, lib.s2d_debug_wide_forward(C.byref(s), xt.data_ptr(), n, y.data_ptr(), g.data_ptr(), name, None),
                's2d_debug_wide_forward')
    torch.cuda.synchronize()
    y, g = y.cpu().numpy(), g.cpu().numpy()
    assert (y[n:] == -7777.0).all() and (g[n:] == -5).all(), 'wrote past n'
    assert bool((ws[words:] == -3333.0).all()), 'wrote past the workspace'
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


def check(refs, params, x, hidden, na, act, what):
    """the device against wide_ref's forward and the argmax scan, and the kernel's name against the shape and the plan; returns y"""
    from soccer2d_amd.wide_actor import wide_plan
    y, g, name = device_forward(params, x, hidden, na, act)
    waves, tiles = wide_plan(hidden, na)[:2]
    want_name = f's2d_debug_wide_forward_kernel<act={act},h={hname(hidden)},a={na},waves={waves},tiles={tiles}>'
    assert name == want_name, (name, want_name)
    want = W.forward(refs[0], x, params, hidden, na, act)
    same(y, want, f'{what} y')
    same(g, M.argmax(refs[1], want), f'{what} greedy')
    return y


# ---------------------------------------------------------------------------------------------------------- the network alone
# k-step tails of h / 4: 12 -> 3 = 2 + 1, 20 -> 4 + 1, 28 -> 4 + 2 + 1, 16 -> 4, 8 -> 2 (read by the layer above, so each is followed
# by another layer); tile groups: 300 -> 19 = 4 x 4 + 2 + 1, 400 -> 25 = 6 x 4 + 1, 256 -> 16 = 4 x 4; depth 1 and 5; every A, every
# activation, and n at the tile (16), wave (64) and workgroup edges.
NETWORKS = [((12, 20), 'relu', 16, 1), ((20, 28), 'tanh', 17, 15), ((28, 12), 'sigmoid', 4, 16), ((16, 8), 'relu', 1, 17),
            ((8, 16), 'sigmoid', 64, 63), ((300,), 'tanh', 16, 64), ((400,), 'sigmoid', 1, 65), ((256,), 'relu', 17, 129),
            ((400, 300), 'sigmoid', 16, 127), ((256, 256), 'tanh', 16, 128), ((12, 400, 28, 300, 20), 'relu', 4, 129),
            ((8, 16, 12, 28, 20), 'tanh', 16, 255), ((136, 64), 'sigmoid', 16, 257), ((400,) * 5, 'sigmoid', 16, 129)]


def test_networks_cover_the_edges():
    from soccer2d_amd.wide_actor import wide_plan
    assert {c[2] for c in NETWORKS} == {1, 4, 16, 17, 64} and {c[1] for c in NETWORKS} == set(W.ACT)
    assert {1, 15, 16, 17, 63, 64, 65} <= {c[3] for c in NETWORKS} and {1, 5} <= {len(c[0]) for c in NETWORKS}
    for hidden, _, na, n in NETWORKS[8:]:                                  # the planned workgroup size - 1, itself, + 1
        assert abs(n - 64 * wide_plan(hidden, na)[0]) <= 1, (hidden, n)
    assert {wide_plan(c[0], c[2])[:2] for c in NETWORKS} >= {(4, 2), (4, 1), (2, 2), (2, 1)}


@pytest.mark.parametrize('hidden,act,na,n', NETWORKS, ids=lambda v: hname(v) if isinstance(v, tuple) else str(v))
def test_network_alone(refs, hidden, act, na, n):
    rs = np.random.RandomState(sum(hidden) * 131 + na * 7 + n)
    y = check(refs, random_net(rs, hidden, na), random_obs(rs, n), hidden, na, act, f'{hidden} {act} a={na} n={n}')
    assert np.isfinite(y).all() and (n * na == 1 or len(np.unique(y)) > 1)


# ------------------------------------------------------------------------------------------------------------- special values
EDGE_SHAPES = [((12, 20), 4), ((300, 28), 17), ((136, 12, 260), 1)]     # above 128, and widths that are no multiple of 8


def _identity_net(hidden, na, diag=1.0, bias=0.0):
    """every layer W[j][j mod fan_in] = diag, the rest zero; biases `bias`"""
    p = np.zeros(M.param_count(hidden, na), dtype=F)
    v = views(p, hidden, na)
    for Wl, b in zip(v[0::2], v[1::2]):
        for j in range(Wl.shape[0]):
            Wl[j, j % Wl.shape[1]] = diag
        b[...] = bias
    return p


@pytest.mark.parametrize('hidden,na', EDGE_SHAPES)
def test_minus_zero_through_tanh_and_sigmoid_networks(refs, hidden, na):
    """layer 1's accumulator is exactly -0 (bias -0, products -0 * +0): its two padding terms make it +0, which tanh_spec (odd)
    would otherwise hand on as -0 to the output; a sigmoid network maps either zero to 0.5 and the word-for-word comparison holds"""
    p = _identity_net(hidden, na, bias=-0.0)
    views(p, hidden, na)[0][...] = -0.0
    x = np.zeros((65, 10), dtype=F)
    y = check(refs, p, x, hidden, na, 'tanh', 'minus zero tanh')
    assert (y == 0).all() and not np.signbit(y).any()
    ys = check(refs, p, x, hidden, na, 'sigmoid', 'minus zero sigmoid')
    assert (ys[:, 0] > 0).all()


@pytest.mark.parametrize('act', ['relu', 'tanh'])
@pytest.mark.parametrize('hidden,na', EDGE_SHAPES)
def test_subnormals_are_kept(refs, hidden, na, act):
    x = np.full((63, 10), 1e-40, dtype=F)
    x[1::2] = 2.0 ** -149
    y = check(refs, _identity_net(hidden, na), x, hidden, na, act, 'subnormal')
    assert (y[:, 0] > 0).all() and (y[:, 0] < 2.0 ** -126).all()                # not flushed, not rounded away


def test_subnormal_weights_and_sums(refs):
    """subnormal weights against inputs of 1 and sums of subnormals that stay subnormal, in a layer of 300 units"""
    hidden, na = (300, 20), 4
    p = _identity_net(hidden, na)
    v = views(p, hidden, na)
    v[0][...] = 2.0 ** -140                                                     # 10 products of 2^-140: 10 x 2^-140, subnormal
    x = np.ones((17, 10), dtype=F)
    y = check(refs, p, x, hidden, na, 'relu', 'subnormal weights')
    assert (y[:, 0] == F(10 * 2.0 ** -140)).all()


@pytest.mark.parametrize('hidden,na', EDGE_SHAPES)
def test_nan_and_overflow(refs, hidden, na):
    """relu(NaN) = +0, tanh_spec and sigmoid_spec pass NaN on (a NaN input reaches every unit of layer 1: 0 * NaN = NaN); sums past
    3.4e38 overflow to +-inf; inf * 0 and inf - inf give NaN"""
    x = np.ones((65, 10), dtype=F)
    x[::2, 0] = np.nan
    p = _identity_net(hidden, na)
    yr = check(refs, p, x, hidden, na, 'relu', 'nan relu')
    yt = check(refs, p, x, hidden, na, 'tanh', 'nan tanh')
    ys = check(refs, p, x, hidden, na, 'sigmoid', 'nan sigmoid')
    assert np.isfinite(yr).all() and (yr[::2, 0] == 0).all() and not np.signbit(yr[::2, 0]).any()
    assert np.isnan(yt[::2, 0]).all() and np.isfinite(yt[1::2]).all()
    assert np.isnan(ys[::2, 0]).all() and np.isfinite(ys[1::2]).all()
    # overflow in the output layer's chain: four terms of -+3e38 times hidden units of 10 (relu) or in (0.4, 1]
    big = _identity_net(hidden, na)
    Wo = views(big, hidden, na)[-2]
    Wo[...] = 0.0
    Wo[0, :4] = -3e38
    if na > 1:
        Wo[1, :4] = 3e38
    x = np.full((63, 10), 10.0, dtype=F)
    for act in ('relu', 'tanh', 'sigmoid'):
        y = check(refs, big, x, hidden, na, act, f'overflow {act}')
        assert np.isneginf(y[:, 0]).all() and (na == 1 or np.isposinf(y[:, 1]).all())
    # an infinite input: inf * 0 = NaN in every unit of layer 1 that does not read it; inf - inf = NaN in one that reads both
    x = np.ones((17, 10), dtype=F)
    x[:, 0], x[:, 1] = np.inf, -np.inf
    p = _identity_net(hidden, na)
    views(p, hidden, na)[0][0, :2] = 1.0                                        # unit 0: inf - inf
    y = check(refs, p, x, hidden, na, 'tanh', 'inf')
    assert np.isnan(y[:, 0]).all()


@pytest.mark.parametrize('act', ['relu', 'tanh', 'sigmoid'])
@pytest.mark.parametrize('hidden,na', [((28, 300, 12, 136, 20), 17), ((400, 8, 260, 16, 44), 4)])
def test_one_hot_routing_through_five_layers(refs, hidden, na, act):
    """every unit of every layer reads exactly one input, by a permutation of the layer below, with a weight of its own: a
    permuted k, a shifted fragment or a padded unit read by mistake changes the output"""
    rs = np.random.RandomState(5)
    p = np.zeros(M.param_count(hidden, na), dtype=F)
    v = views(p, hidden, na)
    for Wl, b in zip(v[0::2], v[1::2]):
        fan = Wl.shape[1]
        perm = rs.permutation(fan)
        for j in range(Wl.shape[0]):
            Wl[j, perm[(5 * j + 3) % fan]] = 0.5 + (j + 1) / 1024.0
        b[...] = (np.arange(Wl.shape[0]) + 1) / 4096.0
    x = rs.uniform(0.25, 1.0, (65, 10)).astype(F)
    y = check(refs, p, x, hidden, na, act, 'one-hot')
    assert len(np.unique(y[0])) > min(na, 8) // 2


# `at` = the k of the last of the three cancelling terms, which then lie: in one k-step; across two groups of four k-steps (k = 15 |
# 16); across the last group of four and the group of two (k = 15 | 16 of 28: steps 0-3 | 4, 5 | 6); across the group of two and
# the single step (k = 23 | 24 of 28); across the last group of four and the single step (k = 15 | 16 of 20); in the single step
# after the group of two (k = 8 .. 10 of 12); and far out in a row of 300
CANCEL = [((20,), 6), ((300,), 17), ((136, 28), 17), ((136, 28), 25), ((12, 20), 17), ((12,), 10), ((300,), 299), ((400, 260), 258)]


@pytest.mark.parametrize('hidden,at', CANCEL)
def test_cancellation_shows_ascending_k(refs, hidden, at):
    """the output layer over the last hidden layer's units, all exactly 1: 1 + 2^24 - 2^24 is 0 only if the terms enter in
    ascending k (2^24 - 2^24 + 1 = 1)"""
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
        y = check(refs, p, x, hidden, na, act, 'cancellation')
        assert (y[:, 0] == 0).all() and (y[:, 1] == 1).all() and (y[:, 2] == 0).all()


# ------------------------------------------------------------------------------------------------- independence of the plan
@pytest.mark.parametrize('hidden,act,na,pairs', [((28, 136), 'sigmoid', 17, 5), ((64, 64), 'tanh', 16, 8)])
def test_every_admissible_plan_gives_the_same_words(refs, hidden, act, na, pairs, monkeypatch):
    """S2D_WIDE_PLAN=waves,tiles (read at launch) runs one shape under every pair that fits the LDS: for [28, 136] with 17 outputs
    (pitch 196) those are (2, 2), (2, 1) and one wave with 4, 2 or 1 tiles; for [64, 64] with 16 all but (4, 4)"""
    rs = np.random.RandomState(3)
    p, x = random_net(rs, hidden, na), random_obs(rs, 300)
    want = W.forward(refs[0], x, p, hidden, na, act)
    seen = set()
    for waves in (4, 2, 1):
        for tiles in (4, 2, 1):
            monkeypatch.setenv('S2D_WIDE_PLAN', f'{waves},{tiles}')
            try:
                y, g, name = device_forward(p, x, hidden, na, act)
            except ValueError as e:                                          # the pair does not fit: refused, by name
                assert 'S2D_WIDE_PLAN' in str(e)
                continue
            assert name.endswith(f'waves={waves},tiles={tiles}>'), name
            same(y, want, name)
            seen.add((waves, tiles))
    monkeypatch.delenv('S2D_WIDE_PLAN')
    from soccer2d_amd.wide_actor import wide_plan
    assert len(seen) == pairs and {(1, 1), (1, 4), (2, 2), wide_plan(hidden, na)[:2]} <= seen, seen


# ------------------------------------------------------------------------------------------ equality with the resident kernels
def _kw(mode, **over):
    kw = dict(O.DQN_KWARGS)
    kw.update(MODES[mode])
    kw.update(over)
    return kw


def _engine(n, mode='discrete', noise='off', **kw):
    from soccer2d_amd.engine import Engine, make_config
    return Engine(n, 'cuda:0', cfg=make_config(**NOISE[noise], **_kw(mode, **kw)))


class _StepOracle(_StepEngine):
    """test_gpu_qnet_actor's reference for the rcssserver noise model (the per-step API with caller actions; the CPU oracle does
    not implement that model) on an engine of any action mode"""

    def __init__(self, n, mode, noise, **kw):
        self.e = _engine(n, mode, noise, **kw)
        self.dtype = np.int32 if mode == 'discrete' else np.float32

    def step(self, a):
        o, r, d, res = self.e.step(torch.from_numpy(np.ascontiguousarray(a, dtype=self.dtype)).to('cuda:0'))
        return self._np(o), self._np(r), self._np(d), self._np(res)


def _oracle(n, mode='discrete', noise='off', seed=0x5EED, **kw):
    if noise == 'square':
        return _StepOracle(n, mode, noise, seed=seed, **kw)
    cfg = O.make_config(seed=seed, auto_reset=1, noise=int(NOISE[noise]['noise']), **_kw(mode, **kw))
    return O.OracleEngine(cfg, n, 'f32')


def _module(hidden, na, act, seed, tanh_head=False, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    layers, win = [], 10
    for w in hidden:
        layers += [nn.Linear(win, w), ACT_NN[act]()]
        win = w
    layers.append(nn.Linear(win, na))
    if tanh_head:
        layers.append(nn.Tanh())
    net = nn.Sequential(*layers)
    with torch.no_grad():
        for p in net.parameters():
            fan = p.shape[-1] if p.dim() == 2 else 10
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * scale * min(1.0, (30.0 / fan) ** 0.5))
    return net


@pytest.mark.parametrize('hidden', [(24, 40, 8), (128, 64, 32, 16)])
def test_debug_forward_equals_the_resident_kernel(hidden):
    from soccer2d_amd import _capi
    lib = _capi.load_library()
    rs = np.random.RandomState(sum(hidden))
    na, n = 16, 257
    p, x = random_net(rs, hidden, na), random_obs(rs, n)
    y, g, _ = device_forward(p, x, hidden, na, 'tanh')
    pt, xt = torch.from_numpy(p).to('cuda:0'), torch.from_numpy(x).to('cuda:0')
    y2 = torch.zeros((n, na), device='cuda:0')
    g2 = torch.zeros(n, dtype=torch.int32, device='cuda:0')
    s = _capi.S2DMlpNet()
    s.n_hidden = len(hidden)
    for l, w in enumerate(hidden):
        s.hidden[l] = w
    s.n_out, s.activation, s.params = na, 1, pt.data_ptr()
    _capi.check(lib, lib.s2d_debug_mlp_forward(C.byref(s), xt.data_ptr(), n, y2.data_ptr(), g2.data_ptr(), None, None),
                's2d_debug_mlp_forward')
    torch.cuda.synchronize()
    same(y, y2.cpu().numpy(), f'y {hidden}')
    same(g, g2.cpu().numpy(), f'greedy {hidden}')


RECORD = ('obs', 'action', 'reward', 'done', 'result', 'terminal_obs')


def _both_paths(mode, rollout, make_old, make_new):
    """the same launch through the resident and the streamed entry point on twin engines: every record word and the arena"""
    n, T = 130, 8
    engs = [_engine(n, mode, 'lattice', max_steps=12), _engine(n, mode, 'lattice', max_steps=12)]
    outs = []
    for eng, make in zip(engs, (make_old, make_new)):
        eng.reset()
        eng.rollout(7)
        out = eng.alloc_rollout(T, terminal_obs=True)
        out['terminal_obs'].fill_(float('nan'))
        outs.append(getattr(eng, rollout)(T, make(), out=out))
    torch.cuda.synchronize()
    for k in RECORD:
        same(outs[1][k], outs[0][k].cpu().numpy(), f'record.{k}')
    assert torch.equal(engs[0].arena, engs[1].arena)
    return engs


def test_rollout_qnet_equals_the_resident_path():
    from soccer2d_amd.mlp_actor import MlpQNetActor
    from soccer2d_amd.wide_actor import WideQNetActor
    net = _module((24, 40, 8), 16, 'tanh', 3).to('cuda:0')
    engs = _both_paths('discrete', 'rollout_qnet', lambda: MlpQNetActor.from_module(net, epsilon=0.3),
                       lambda: WideQNetActor.from_module(net, epsilon=0.3))
    assert engs[0].kernel_name().startswith('s2d_mlp_qnet_rollout_kernel<')
    assert engs[1].kernel_name() == 's2d_wide_qnet_rollout_kernel<noise=1,act=tanh,h=24-40-8,a=16,waves=4,tiles=2>'


def test_rollout_actor_equals_the_resident_path():
    from soccer2d_amd.mlp_actor import MlpDeterministicActor
    from soccer2d_amd.wide_actor import WideDeterministicActor
    net = _module((64, 64), 4, 'relu', 4, tanh_head=True, scale=0.5).to('cuda:0')
    kw = dict(epsilon=0.3, noise_sigma=0.2, noise_mean=0.05)
    engs = _both_paths('turn4', 'rollout_actor', lambda: MlpDeterministicActor.from_module(net, **kw),
                       lambda: WideDeterministicActor.from_module(net, **kw))
    assert engs[1].kernel_name() == 's2d_wide_actor_rollout_kernel<mode=turn4,noise=1,gauss=1,act=relu,h=64-64,a=4,waves=4,tiles=2>'


# ---------------------------------------------------------------------------------------- closed loops against the CPU oracle
def _closed_loop(refs, mode, hidden, act, n, T, eps, noise, sigma=None, twins=(), **task):
    """the wide actor's launch against the oracle's closed loop; twins: make(net) -> an actor of another back end on the same
    module, launched on a twin engine: its record and arena are the wide launch's bit for bit (returns [eng, *twin engines])"""
    from soccer2d_amd.wide_actor import WideDeterministicActor, WideQNetActor
    wl, ml, ql = refs
    discrete = mode == 'discrete'
    na = 16 if discrete else 4 if mode == 'turn4' else 1
    eng, orc = _engine(n, mode, noise, **task), _oracle(n, mode, noise, **task)
    eng.reset(); orc.reset()
    eng.rollout(5); orc.rollout(5)
    net = _module(hidden, na, act, n + T + na, tanh_head=not discrete, scale=1.0 if discrete else 0.5).to('cuda:0')
    actor = (WideQNetActor.from_module(net, epsilon=eps) if discrete
             else WideDeterministicActor.from_module(net, epsilon=eps, noise_sigma=sigma))
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
            a = W.q_actions(wl, ml, ql, obs, params, hidden, na, act, eps, eng.cfg.seed, gid, k0 + t)
        else:
            a = W.actor_actions(wl, ml, obs, params, hidden, na, act, eps, actor.noise_kind, noise_rows, eng.cfg.seed, k0 + t)
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
    if not twins:
        return eng, out
    engs = [eng]
    for make in twins:
        twin = _engine(n, mode, noise, **task)
        twin.reset()
        twin.rollout(5)
        tout = twin.alloc_rollout(T, terminal_obs=True)
        tout['terminal_obs'].fill_(float('nan'))
        tout = (twin.rollout_qnet if discrete else twin.rollout_actor)(T, make(net), out=tout)
        torch.cuda.synchronize()
        for k in RECORD:
            same(tout[k], out[k].cpu().numpy(), f'{twin.kernel_name()} record.{k}')
        assert torch.equal(twin.arena, eng.arena), twin.kernel_name()
        engs.append(twin)
    return engs, out


INSTANTIATIONS = ([('discrete', nz, None) for nz in NOISE] +
                  [(m, nz, sigma) for m in ('cont1', 'turn4') for nz in NOISE for sigma in (None, 0.2)])


@pytest.mark.parametrize('mode,noise,sigma', INSTANTIATIONS)
def test_every_instantiation_of_the_three_back_ends(refs, mode, noise, sigma):
    """Each kernel of the launch tables the three back ends share -- the Q head's 3 (engine noise off / lattice / square) and the
    tanh head's 2 x 3 x 2 (mode x engine noise x Gaussian action noise) -- once per back end: 256 envs x 8 steps on a 10-16-16-A
    ReLU network, the wide launch against the oracle's closed loop and the MLP and two-layer launches equal to it bit for bit, so
    that a mixed-up table entry (off for square, a swapped gauss) shows in the record; and the full kernel name of each."""
    from soccer2d_amd.actor import DeterministicActor, QNetActor
    from soccer2d_amd.mlp_actor import MlpDeterministicActor, MlpQNetActor, lds_plan
    from soccer2d_amd.wide_actor import wide_plan
    discrete = mode == 'discrete'
    kw = dict(epsilon=0.2) if discrete else dict(epsilon=0.2, noise_sigma=sigma)
    mlp, two = (MlpQNetActor, QNetActor) if discrete else (MlpDeterministicActor, DeterministicActor)
    engs, out = _closed_loop(refs, mode, (16, 16), 'relu', 256, 8, 0.2, noise, sigma=sigma, max_steps=6,
                             twins=[lambda net: mlp.from_module(net, **kw), lambda net: two.from_module(net, **kw)])
    assert int(out['done'].sum()) >= 256
    a = 16 if discrete else out['action'].shape[-1]
    nk, gauss = list(NOISE).index(noise), int(sigma is not None)
    waves, tiles = wide_plan((16, 16), a)[:2]
    head = f'noise={nk}' if discrete else f'mode={mode},noise={nk},gauss={gauss}'
    kind = 'qnet' if discrete else 'actor'
    assert [e.kernel_name() for e in engs] == [
        f's2d_wide_{kind}_rollout_kernel<{head},act=relu,h=16-16,a={a},waves={waves},tiles={tiles}>',
        f's2d_mlp_{kind}_rollout_kernel<{head},act=relu,h=16-16,a={a},waves={lds_plan((16, 16), a)[0]}>',
        f's2d_reach_{kind}_rollout_kernel<{head},h1=16,h2=16,a={a},waves=4>']


@pytest.mark.parametrize('noise', ['off', 'lattice'])
@pytest.mark.parametrize('eps', [0.0, 0.3, 1.0])
def test_qnet_closed_loop(refs, eps, noise):
    """[400, 300] Sigmoid, A = 16; max_steps = 12, so every env auto-resets in 24 cycles; eps = 1 is the random-policy rollout"""
    eng, out = _closed_loop(refs, 'discrete', (400, 300), 'sigmoid', 200, 24, eps, noise, max_steps=12)
    assert eng.kernel_name() == (f's2d_wide_qnet_rollout_kernel<noise={int(noise != "off")},act=sigmoid,h=400-300,a=16,'
                                 f'waves=2,tiles=1>')
    assert int(out['done'].sum(dim=0).min()) >= 1
    if eps == 1.0:
        twin = _engine(200, 'discrete', noise, max_steps=12)
        twin.reset(); twin.rollout(5)
        r = twin.rollout(24)
        torch.cuda.synchronize()
        for k in ('obs', 'action', 'reward', 'done', 'result'):
            same(out[k], r[k].cpu().numpy(), f'random-policy rollout {k}')


@pytest.mark.parametrize('mode,hidden,act,plan', [('cont1', (400, 300), 'relu', 'waves=2,tiles=1'),
                                                  ('turn4', (256,) * 5, 'sigmoid', 'waves=2,tiles=1')])
def test_tanh_actor_closed_loop(refs, mode, hidden, act, plan):
    """SB3's default DDPG actor [400, 300] ReLU on a continuous engine and [256] * 5 Sigmoid on a turning one, Gaussian noise"""
    eng, out = _closed_loop(refs, mode, hidden, act, 130, 24, 0.1, 'lattice', sigma=0.2, max_steps=12)
    a = out['action'].cpu().numpy()
    assert len(np.unique(a)) > 100 and (np.abs(a) <= 1).all()
    assert eng.kernel_name() == (f's2d_wide_actor_rollout_kernel<mode={mode},noise=1,gauss=1,act={act},h={hname(hidden)},'
                                 f'a={a.shape[-1]},{plan}>')


# ------------------------------------------------------------------------------------------------------------- graph capture
def test_graph_replay_packs_and_reads_at_replay():
    """the captured graph holds the pack node: after load_from another module and a new epsilon the replay acts with them"""
    from soccer2d_amd.wide_actor import WideQNetActor
    n, T, hidden = 300, 12, (300, 28)
    eng = _engine(n, 'discrete', 'lattice')
    eng.reset()
    net1, net2 = _module(hidden, 16, 'sigmoid', 7).to('cuda:0'), _module(hidden, 16, 'sigmoid', 8).to('cuda:0')
    actor = WideQNetActor.from_module(net1, epsilon=0.05)
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
    r = eng.rollout_qnet(T, WideQNetActor.from_module(net2, epsilon=0.3))
    torch.cuda.synchronize()
    for k in got:
        same(got[k], r[k].cpu().numpy(), k)
    for f in state:
        same(state[f], getattr(eng, f).cpu().numpy(), f)
    eng.load_state_dict(sd)
    old = eng.rollout_qnet(T, WideQNetActor.from_module(net1, epsilon=0.05))
    torch.cuda.synchronize()
    assert not torch.equal(old['action'], got['action'])       # the replay did not act with what the capture saw


# ------------------------------------------------------------------------------------------------------ agreement with float64
@pytest.mark.parametrize('hidden,act', [((400, 300), 'relu'), ((400, 300), 'tanh'), ((256, 256), 'sigmoid')])
def test_outputs_and_greedy_agree_with_a_float64_forward(hidden, act):
    """every device output lies within the rigorous running bound (tests/wide_f64.py: the chains' rounding, the activation's
    Lipschitz constant -- 1/4 for the sigmoid -- and the spec function's own error) of the float64 network, and the greedy action
    is float64's wherever its top-two gap exceeds twice the bound; rows inside it are only counted, at most 1 % of them.  Every
    unit reads 8 inputs of the layer below (N(0, 1 / 8); biases N(0, 0.1); RandomState(11), per layer all rows of W, then b): dense
    rows of 400 would carry every unit's error through row sums of about 16.  Float64 alone left 3, 0 and 6 of the 4000 rows
    inside for the three networks, with bounds <= 1.8e-4.  The sigmoid network's argmax takes few values: there the output bound
    is the check."""
    na, n = 16, 4000
    rs = np.random.RandomState(11)
    params = W64.sparse_net(rs, hidden, na)
    x = rs.uniform(-1, 1, (n, 10)).astype(F)
    y64, e = W64.f64_bound(params, x, hidden, na, act)
    net = _module(hidden, na, act, 0)
    with torch.no_grad():
        for p, v in zip(net.parameters(), views(params, hidden, na)):
            p.copy_(torch.from_numpy(v))
        yt = net.double()(torch.from_numpy(x).double()).numpy()
    assert np.allclose(yt, y64, rtol=0, atol=1e-12)
    top = np.sort(y64, axis=1)
    clear = (top[:, -1] - top[:, -2]) > 2 * e.max(axis=1)
    inside = int((~clear).sum())
    y, g, _ = device_forward(params, x, hidden, na, act)
    print(f'{hidden} {act}: rows inside the bound: {inside} of {n}; largest bound {e.max():.3g}; '
          f'largest |y - y64| / bound {float((np.abs(y - y64) / e).max()):.3g}; greedy values {len(np.unique(g))}')
    assert inside <= n // 100
    assert (np.abs(y - y64) <= e).all(), float((np.abs(y - y64) / e).max())
    assert np.array_equal(g[clear], y64.argmax(axis=1)[clear])


# ------------------------------------------------------------------------------------------------------------------ rejections
def test_rejections_leave_the_state_unchanged():
    from soccer2d_amd import _capi
    from soccer2d_amd.mlp_actor import MlpQNetActor
    from soccer2d_amd.wide_actor import WideDeterministicActor, WideQNetActor
    q = WideQNetActor.from_module(_module((300, 28), 16, 'sigmoid', 1).to('cuda:0'), epsilon=0.1)
    mu1 = WideDeterministicActor.from_module(_module((400, 300), 1, 'relu', 2, tanh_head=True).to('cuda:0'), noise_sigma=0.1)
    mu4 = WideDeterministicActor.from_module(_module((20, 12), 4, 'tanh', 2, tanh_head=True).to('cuda:0'), noise_sigma=0.1)
    ro = _capi.S2DRollout()

    def edits(net):
        """every struct the header refuses: (what, edit, a word of the error text)"""
        def set_(**kw):
            def f(s):
                for k, v in kw.items():
                    setattr(s, k, v)
            return f

        def width(l, w):
            def f(s):
                s.hidden[l] = w
            return f
        return [('n_hidden 0', set_(n_hidden=0), 'n_hidden'), ('n_hidden 6', set_(n_hidden=6), 'n_hidden'),
                ('width 6', width(0, 6), 'hidden'), ('width 18', width(1, 18), 'hidden'), ('width 404', width(0, 404), 'hidden'),
                ('width 0', width(1, 0), 'hidden'), ('entry past n_hidden', width(4, 8), 'hidden'),
                ('activation 3', set_(activation=3), 'activation'), ('activation -1', set_(activation=-1), 'activation'),
                ('n_out', set_(n_out=net.n_out + 1), 'n_out'), ('params NULL', set_(params=None), 'params'),
                ('params misaligned', set_(params=net.params + 4), 'params'), ('epsilon NULL', set_(epsilon=None), 'epsilon'),
                ('epsilon misaligned', set_(epsilon=net.epsilon + 2), 'epsilon'),
                ('workspace NULL', set_(workspace=None), 'workspace'),
                ('workspace misaligned', set_(workspace=net.workspace + 128), 'workspace'),
                ('workspace_bytes', set_(workspace_bytes=net.workspace_bytes - 4), f'needs {net.workspace_bytes}')]

    for mode, actor, entry in (('discrete', q, 's2d_rollout_qnet_wide'), ('cont1', mu1, 's2d_rollout_actor_wide'),
                               ('turn4', mu4, 's2d_rollout_actor_wide')):
        eng = _engine(256, mode)
        eng.reset()
        before = eng.arena.clone()
        ws_before = actor.workspace.clone()
        fn = getattr(eng.lib, entry)
        base = actor.c_struct()
        assert base.workspace_bytes == eng.lib.s2d_wide_workspace_bytes(C.byref(base))
        cases = edits(base)
        if mode == 'discrete':
            cases += [('noise_kind on the Q path', lambda s: setattr(s, 'noise_kind', 1), 'noise_kind')]
        else:
            cases += [('noise_kind 2', lambda s: setattr(s, 'noise_kind', 2), 'noise_kind'),
                      ('noise NULL', lambda s: setattr(s, 'noise', None), 'noise'),
                      ('noise misaligned', lambda s: setattr(s, 'noise', base.noise + 2), 'noise')]
        for what, edit, word in cases:
            s = actor.c_struct()
            edit(s)
            msg = refused(eng.lib, f'{entry}/struct/{mode}/{what}', fn(eng._h, 4, C.byref(s), C.byref(ro), None, eng._stream()))
            assert word in msg and entry in msg, (mode, what, msg)
        s = actor.c_struct()
        assert 'n_steps' in refused(eng.lib, f'{entry}/struct/{mode}/n_steps 0',
                                    fn(eng._h, 0, C.byref(s), C.byref(ro), None, eng._stream()))
        refused(eng.lib, f'{entry}/struct/{mode}/net NULL', fn(eng._h, 4, None, C.byref(ro), None, eng._stream()))
        # the wrong engine mode, through both layers
        other = getattr(eng.lib, 's2d_rollout_actor_wide' if mode == 'discrete' else 's2d_rollout_qnet_wide')
        refused(eng.lib, f'{entry}/struct/{mode}/the other entry',
                other(eng._h, 4, C.byref(actor.c_struct()), C.byref(ro), None, eng._stream()))
        with pytest.raises(ValueError):
            if mode == 'discrete':
                eng.rollout_actor(4, mu1)
            else:
                eng.rollout_qnet(4, q)
        torch.cuda.synchronize()
        assert torch.equal(before, eng.arena), mode
        assert torch.equal(ws_before, actor.workspace), mode                   # no pack kernel ran either
    # the diagnostic refuses the same shapes and workspaces, and bad pointers and counts
    lib = _capi.load_library()
    x = torch.zeros((4, 10), device='cuda:0')
    y = torch.zeros((4, 16), device='cuda:0')
    g = torch.zeros(4, dtype=torch.int32, device='cuda:0')
    dbg = [c for c in edits(q.c_struct()) if c[0] not in ('n_out', 'epsilon NULL', 'epsilon misaligned')]
    for what, edit, word in dbg:
        s = q.c_struct()
        edit(s)
        assert lib.s2d_debug_wide_forward(C.byref(s), x.data_ptr(), 4, y.data_ptr(), g.data_ptr(), None, None) == _capi.S2D_EINVAL, what
        assert word in lib.s2d_last_error().decode(), what
    s = q.c_struct()
    assert lib.s2d_debug_wide_forward(C.byref(s), x.data_ptr(), 0, y.data_ptr(), g.data_ptr(), None, None) == _capi.S2D_EINVAL
    assert lib.s2d_debug_wide_forward(C.byref(s), None, 4, y.data_ptr(), g.data_ptr(), None, None) == _capi.S2D_EINVAL
    assert lib.s2d_debug_wide_forward(C.byref(s), x.data_ptr() + 2, 4, y.data_ptr(), g.data_ptr(), None, None) == _capi.S2D_EINVAL
    assert lib.s2d_debug_wide_forward(None, x.data_ptr(), 4, y.data_ptr(), g.data_ptr(), None, None) == _capi.S2D_EINVAL
    # the resident path keeps its own limit
    with pytest.raises(ValueError, match='bytes of LDS'):
        MlpQNetActor((128, 128, 128), 16, device='cuda:0')
