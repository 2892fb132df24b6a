"""CPU checks of the fused Q-learner's host side (s2d_learn_q / s2d_learn_q_grad, soccer2d_amd.learn): the ABI, the workspace
arithmetic, and the host restatement tests/learn_ref.c -- its forward against td_ref.c bitwise, its gradients against float64
torch autograd, its Adam against float64 torch.optim.Adam, the clip, hand-computed cases and a training sanity run -- and the
argument checks of QLearner that raise before any library call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import learn as LR
import td as TD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip('torch')
nn = torch.nn
F = np.float32


@pytest.fixture(scope='module')
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp('learn_ref')
    return LR.build(d), TD.build(d)


# ------------------------------------------------------------------------------------------------------------------------ ABI
NET_FIELDS = ('n_in', 'n_hidden', 'hidden', 'n_out', 'activation', 'params', 'workspace', 'workspace_bytes')
STATE_FIELDS = ('m', 'v', 'grad', 'hyper', 'stats', 'error', 'loss_kind')


def test_struct_layout_matches_c(tmp_path):
    from soccer2d_amd import _capi
    prog = tmp_path / 'learn_abi.c'
    offs = ','.join([f'offsetof(S2DLearnNet,{f})' for f in NET_FIELDS] + [f'offsetof(S2DLearnState,{f})' for f in STATE_FIELDS])
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s2d.h"\nint main(){size_t v[]={sizeof(S2DLearnNet),'
                    'sizeof(S2DLearnState),' + offs + ',S2D_ABI_VERSION,S2D_LEARN_BLOCK_ROWS,S2D_LEARN_NORM_CHUNK,S2D_LEARN_MSE,'
                    'S2D_LEARN_HUBER};for(unsigned i=0;i<sizeof v/sizeof*v;++i)printf("%zu ",v[i]);return 0;}\n')
    exe = tmp_path / 'learn_abi'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(prog), '-o', str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    from soccer2d_amd import learn
    want = ([C.sizeof(_capi.S2DLearnNet), C.sizeof(_capi.S2DLearnState)] + [getattr(_capi.S2DLearnNet, f).offset for f in NET_FIELDS] +
            [getattr(_capi.S2DLearnState, f).offset for f in STATE_FIELDS] + [4, learn.BLOCK_ROWS, learn.NORM_CHUNK, 0, 1])
    assert got == want
    assert (learn.BLOCK_ROWS, learn.NORM_CHUNK) == (LR.BLOCK_ROWS, LR.NORM_CHUNK)
    assert learn.LOSSES.index('mse') == 0 and learn.LOSSES.index('huber') == 1


def test_symbols_exported_and_workspace_arithmetic():
    """the built library exports the three symbols and binds them; s2d_learn_workspace_bytes (host only) agrees with the Python
    arithmetic on the grid, grows with max_batch, and is 0 off the grid"""
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi
    from soccer2d_amd.learn import learn_workspace_bytes, learn_param_count
    lib = _capi.load_library()
    protos = {p[0]: p for p in _capi.PROTOTYPES}
    for name, nargs in (('s2d_learn_workspace_bytes', 2), ('s2d_learn_q', 10), ('s2d_learn_q_grad', 10)):
        assert hasattr(lib, name) and len(protos[name][2]) == nargs, name
    assert _capi.S2D_ABI_VERSION == 4

    def shape(n_in, hidden, n_out, act=0):
        s = _capi.S2DLearnNet()
        s.n_in, s.n_hidden, s.n_out, s.activation = n_in, len(hidden), n_out, act
        for l, w in enumerate(hidden):
            s.hidden[l] = w
        return s
    for n_in, hidden, n_out, _act in LR.SHAPES + [(224, (64, 64), 16, 'relu'), (10, (256, 256), 16, 'relu'), (256, (256,) * 4, 64, 'relu')]:
        for B in (1, 63, 64, 65, 4096, 2 ** 31 - 1):
            got = lib.s2d_learn_workspace_bytes(C.byref(shape(n_in, hidden, n_out)), B)
            assert got == learn_workspace_bytes(n_in, hidden, n_out, B) and got >= 4 * learn_param_count(n_in, hidden, n_out), (hidden, B)
    # 64 rows of 256-256-256-64 do not fit the LDS: the workspace holds the activations too
    P = learn_param_count(256, (256, 256), 64)
    assert learn_workspace_bytes(256, (256, 256), 64, 64) > 4 * (P + 64 * (256 + 512 + 64))
    assert learn_workspace_bytes(10, (64, 64), 16, 64) < 4 * (learn_param_count(10, (64, 64), 16) + 64 * 3)
    for bad in (shape(0, (8,), 1), shape(257, (8,), 1), shape(10, (12,), 1), shape(10, (264,), 1), shape(10, (4,), 1), shape(10, (8,), 0),
                shape(10, (8,), 65), shape(10, (), 4), shape(10, (8,) * 5, 4), shape(10, (8,), 4, act=3)):
        assert lib.s2d_learn_workspace_bytes(C.byref(bad), 64) == 0
    trailing = shape(10, (8,), 4)
    trailing.hidden[3] = 8                                                  # a width past n_hidden
    assert lib.s2d_learn_workspace_bytes(C.byref(trailing), 64) == 0
    assert lib.s2d_learn_workspace_bytes(None, 64) == 0
    for B in (0, -1, 2 ** 31):
        assert lib.s2d_learn_workspace_bytes(C.byref(shape(10, (64, 64), 16)), B) == 0


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('shape', LR.SHAPES, ids=lambda s: '-'.join(map(str, (s[0],) + s[1] + (s[2],))) + s[3])
def test_forward_equals_td_ref(refs, shape):
    """the forward of learn_ref.c is td_ref.c's td_forward bit for bit at every test shape, edge rows included"""
    L, T = refs
    n_in, hidden, n_out, act = shape
    rs = np.random.RandomState(3)
    net = TD.random_net(rs, n_in, hidden, n_out, act)
    x = rs.uniform(-2, 2, (70, n_in)).astype(F)
    x[0] = 0.0
    x[1] = -0.0
    x[2] = 1e30
    x[3, 0] = np.nan
    assert np.array_equal(TD.bits(LR.forward(L, net, x)), TD.bits(TD.forward(T, net, x)))


@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize('loss', ['huber', 'mse'])
@pytest.mark.parametrize('shape', LR.SHAPES, ids=lambda s: '-'.join(map(str, (s[0],) + s[1] + (s[2],))) + s[3])
def test_gradient_against_float64_autograd(refs, shape, loss, weighted):
    """the restated gradient against float64 torch autograd of the same loss: at most 4 x the largest error of torch's own fp32
    autograd on the same inputs (test_td_host.py's convention), the bound computed here.  B = 150: three blocks, the last partial."""
    L, _ = refs
    n_in, hidden, n_out, act = shape
    rs = np.random.RandomState(11)
    net = TD.random_net(rs, n_in, hidden, n_out, act)
    obs, action, target, weight = LR.random_batch(rs, net, 150)
    if not weighted:
        weight = None
    g64, l64 = LR.torch_grad(net, loss, obs, action, target, weight, torch.float64)
    g32, l32 = LR.torch_grad(net, loss, obs, action, target, weight, torch.float32)
    got = LR.grad(L, net, loss, obs, action, target, weight, max_grad_norm=0.0)
    assert got['error'] == 0
    err_torch, err_ref = np.abs(g32 - g64).max(), np.abs(got['grad'].astype(np.float64) - g64).max()
    print(f'grad error vs float64: torch fp32 {err_torch:.3e}, learn_ref {err_ref:.3e}; |g|max {np.abs(g64).max():.3e}')
    assert err_torch > 0 and err_ref <= 4 * err_torch
    lerr_torch, lerr_ref = abs(l32 - l64), abs(float(got['stats'][0]) - l64)
    print(f'loss error vs float64: torch fp32 {lerr_torch:.3e}, learn_ref {lerr_ref:.3e}')
    assert lerr_ref <= 4 * max(lerr_torch, np.spacing(F(l64)) / 2)          # torch's may happen to round to the float64 value
    norm64 = np.sqrt((g64 ** 2).sum())
    assert abs(float(got['stats'][1]) - norm64) <= 4 * max(err_torch, np.spacing(F(norm64)))
    assert float(got['stats'][2]) == 1.0
    q64 = TD.forward64(net, obs)[np.arange(150), action]
    assert np.abs(got['td_abs'] - np.abs(q64 - target)).max() < 1e-4


def test_adam_against_float64_torch(refs):
    """the restated Adam fed 20 fixed gradient vectors against torch.optim.Adam in float64 fed the same vectors through .grad (and
    the same fp32-representable hyper-parameters): parameters, at most 4 x the error of torch's fp32 Adam on the same vectors.
    |g| >= 1e-3, so that g / (|g| + eps) is well-conditioned."""
    L, _ = refs
    rs = np.random.RandomState(5)
    P, steps = 2000, 20
    p0 = rs.uniform(-1, 1, P).astype(F)
    grads = [(rs.uniform(1e-3, 1.0, P) * rs.choice([-1.0, 1.0], P)).astype(F) for _ in range(steps)]
    lr, b1, b2, eps = (float(F(x)) for x in (1e-3, 0.9, 0.999, 1e-8))

    def run_torch(dtype):
        p = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(dtype))
        opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
        for g in grads:
            p.grad = torch.from_numpy(g.copy()).to(dtype)
            opt.step()
        st = opt.state[p]
        return [t.detach().double().numpy() for t in (p, st['exp_avg'], st['exp_avg_sq'])]
    want, t32 = run_torch(torch.float64), run_torch(torch.float32)
    p, state = p0.copy(), LR.State(P, lr=lr, betas=(b1, b2), eps=eps)
    for g in grads:
        LR.adam(L, p, state, g)
    for name, w, t, r in zip(('params', 'exp_avg', 'exp_avg_sq'), want, t32, (p, state.m, state.v)):
        err_torch, err_ref = np.abs(t - w).max(), np.abs(r.astype(np.float64) - w).max()
        print(f'{name}: torch fp32 {err_torch:.3e}, learn_ref {err_ref:.3e}')
        assert err_torch > 0 and err_ref <= 4 * err_torch, name
    # the running products: beta^20 from 20 fp32 multiplications
    assert abs(float(state.hyper[5]) - b1 ** steps) < 20 * 2.0 ** -24 and abs(float(state.hyper[6]) - b2 ** steps) < 20 * 2.0 ** -24


def test_clip(refs):
    """clip_grad_norm_'s scale: active (norm > max), inactive, and max_grad_norm <= 0; the step applies it, grad stays unclipped"""
    L, _ = refs
    rs = np.random.RandomState(7)
    net = TD.random_net(rs, 10, (16, 16), 4, 'relu')
    obs, action, target, weight = LR.random_batch(rs, net, 100)
    target = target + F(3.0)                                                # a gradient well above the small clip norm
    free = LR.grad(L, net, 'mse', obs, action, target, weight, max_grad_norm=0.0)
    norm = free['stats'][1]
    g64 = free['grad'].astype(np.float64)
    assert abs(float(norm) - np.sqrt((g64 ** 2).sum())) <= 4 * np.spacing(norm) and norm > 0.1
    for mx, want in ((F(0.05), F(0.05) / (norm + F(1e-6))), (F(1e3), F(1.0)), (F(0.0), F(1.0)), (F(-1.0), F(1.0))):
        got = LR.grad(L, net, 'mse', obs, action, target, weight, max_grad_norm=float(mx))
        assert TD.bits(got['stats'][2]) == TD.bits(F(want)) and np.array_equal(TD.bits(got['grad']), TD.bits(free['grad'])), mx
    assert F(0.05) / (norm + F(1e-6)) < 1
    # the step: Adam on grad * scale
    a, b = TD.Net(10, (16, 16), 4, 'relu', net.params.copy()), net.params.copy()
    sa, sb = LR.State(a.params.size, max_grad_norm=0.05), LR.State(a.params.size, max_grad_norm=0.05)
    out = LR.step(L, a, sa, 'mse', obs, action, target, weight)
    LR.adam(L, b, sb, out['grad'], scale=float(out['stats'][2]))
    assert np.array_equal(TD.bits(a.params), TD.bits(b)) and np.array_equal(TD.bits(sa.m), TD.bits(sb.m))
    assert np.array_equal(TD.bits(out['grad']), TD.bits(free['grad'])) and float(out['stats'][2]) < 1


def _hand_net():
    """1-8-1 ReLU: y = relu(W1 x + b1) with rows x = 1 -> (1, 0, 0 [pre-activation exactly 0], 0 ...), x = -1 -> (0, 1, 0 ...);
    q = (2, 3, 5, 0 ...) . y + 0.25: q(1) = 2.25, q(-1) = 3.25"""
    W1 = np.array([1, -1, 0.5, 0, 0, 0, 0, 0], F)
    b1 = np.array([0, 0, -0.5, 0, 0, 0, 0, 0], F)
    W2 = np.array([2, 3, 5, 0, 0, 0, 0, 0], F)
    return TD.Net(1, (8,), 1, 'relu', np.concatenate([W1, b1, W2, [0.25]]).astype(F))


@pytest.mark.parametrize('e0, loss, d0, l0', [(1.0, 'huber', 1.0, 0.5), (-1.0, 'huber', -1.0, 0.5), (1.0, 'mse', 1.0, 0.5),
                                              (2.0, 'huber', 1.0, 1.5), (2.0, 'mse', 2.0, 2.0), (-2.0, 'huber', -1.0, 1.5),
                                              (0.0, 'huber', 0.0, 0.0)])
def test_hand_computed(refs, e0, loss, d0, l0):
    """B = 2 on the 1-8-1 network: row 0 has a TD error of exactly e0, row 1 of exactly 0; every number below is exact in fp32.
    The unit whose pre-activation is exactly 0 gets no gradient (torch's relu'(0) = 0)."""
    L, _ = refs
    net = _hand_net()
    obs, action = np.array([[1.0], [-1.0]], F), np.zeros(2, np.int32)
    target = np.array([2.25 - e0, 3.25], F)
    got = LR.grad(L, net, loss, obs, action, target, None, max_grad_norm=0.0)
    assert np.array_equal(got['q'], np.array([[2.25], [3.25]], F)) and np.array_equal(got['td_abs'], np.array([abs(e0), 0.0], F))
    g = d0 / 2                                                              # the output delta of row 0; row 1's is 0
    dW1 = np.array([2 * g, 0, 0, 0, 0, 0, 0, 0], F)                         # W2[k] g relu'(y) x: only unit 0 is active in row 0
    dW2 = np.array([g, 0, 0, 0, 0, 0, 0, 0], F)                             # g y0[k]
    want = np.concatenate([dW1, dW1, dW2, [g]]).astype(F)
    assert np.array_equal(got['grad'], want), (got['grad'], want)
    assert float(got['stats'][0]) == l0 / 2
    assert float(got['stats'][1]) == float(np.sqrt(F((2 * g) ** 2 * 2 + g * g * 2)))
    # torch agrees, the relu'(0) = 0 convention included
    g64, l64 = LR.torch_grad(net, loss, obs, action, target, None, torch.float64)
    assert np.array_equal(g64, want.astype(np.float64)) and l64 == l0 / 2


def test_bad_action_and_nan(refs):
    """an action outside [0, A) is a zero row with the error word set; a NaN target reaches the loss and the gradient"""
    L, _ = refs
    rs = np.random.RandomState(2)
    net = TD.random_net(rs, 4, (8,), 3, 'tanh')
    obs, action, target, weight = LR.random_batch(rs, net, 9)
    good = LR.grad(L, net, 'huber', obs[:8], action[:8], target[:8], weight[:8])
    for bad in (3, -1, 2 ** 31 - 1):
        a = action.copy()
        a[8] = bad
        got = LR.grad(L, net, 'huber', obs, a, target, weight)
        assert got['error'] == 1 and got['td_abs'][8] == 0
        # the same rows with B = 9 in the divisor: compare against the good rows scaled by hand is inexact, so re-run with weight 0
        w0 = weight.copy()
        w0[8] = 0
        a0 = action.copy()
        same = LR.grad(L, net, 'huber', obs, a0, target, w0)
        assert np.array_equal(TD.bits(got['grad']), TD.bits(same['grad'])) and TD.bits(got['stats'][0]) == TD.bits(same['stats'][0])
    assert good['error'] == 0
    t = target.copy()
    t[4] = np.nan
    got = LR.grad(L, net, 'huber', obs, action, t, weight)
    assert np.isnan(got['stats'][0]) and np.isnan(got['stats'][1]) and np.isnan(got['td_abs'][4]) and np.isnan(got['grad']).any()
    assert not np.isnan(got['td_abs'][[0, 1, 2, 3, 5, 6, 7, 8]]).any()


def test_training_sanity(refs):
    """200 updates of the restatement on a fixed teacher-network regression (B = 256, 10-16-16-4) bring the loss under a tenth of
    its start; torch's fp32 learner on the same batches must meet the same condition first, so the inputs are known learnable."""
    L, _ = refs
    rs = np.random.RandomState(1)
    teacher = TD.random_net(rs, 10, (16, 16), 4, 'tanh', gain=2.0)
    student = TD.random_net(rs, 10, (16, 16), 4, 'tanh')
    batches = []
    for _ in range(200):
        obs = rs.uniform(-1, 1, (256, 10)).astype(F)
        action = rs.randint(0, 4, 256).astype(np.int32)
        batches.append((obs, action, TD.forward64(teacher, obs)[np.arange(256), action].astype(F)))
    lr = 1e-2
    mod = LR.torch_module(student, torch.float32)
    opt = torch.optim.Adam(mod.parameters(), lr=lr)
    tl = []
    for obs, action, target in batches:
        q = mod(torch.from_numpy(obs)).gather(1, torch.from_numpy(action).long().unsqueeze(1)).squeeze(1)
        loss = nn.functional.smooth_l1_loss(q, torch.from_numpy(target))
        opt.zero_grad()
        loss.backward()
        nn.utils.clip_grad_norm_(mod.parameters(), 10.0)
        opt.step()
        tl.append(float(loss))
    assert np.mean(tl[-10:]) < 0.1 * tl[0], (tl[0], np.mean(tl[-10:]))
    net, state, rl = TD.Net(10, (16, 16), 4, 'tanh', student.params.copy()), LR.State(student.params.size, lr=lr), []
    for obs, action, target in batches:
        rl.append(float(LR.step(L, net, state, 'huber', obs, action, target)['stats'][0]))
    print(f'loss: torch {tl[0]:.4f} -> {np.mean(tl[-10:]):.4f}, learn_ref {rl[0]:.4f} -> {np.mean(rl[-10:]):.4f}')
    assert abs(rl[0] - tl[0]) < 1e-5 and np.mean(rl[-10:]) < 0.1 * rl[0]
    assert abs(np.mean(rl[-10:]) - np.mean(tl[-10:])) < 0.25 * np.mean(tl[-10:])    # the two learners follow the same path


# ---------------------------------------------------------------------------------------------------------------- QLearner
def seq(n_in, hidden, n_out, act=nn.ReLU, bias=True):
    layers, win = [], n_in
    for w in hidden:
        layers += [nn.Linear(win, w, bias=bias), act()]
        win = w
    return nn.Sequential(*layers, nn.Linear(win, n_out, bias=bias))


def test_module_parameters_become_views():
    from soccer2d_amd.learn import QLearner, learn_param_count
    mod = seq(10, (64, 64), 16)
    before = [p.detach().clone() for p in mod.parameters()]
    lrn = QLearner.from_module(mod, device='cpu')
    assert lrn.params.numel() == learn_param_count(10, (64, 64), 16) == 5904
    lo, hi = lrn.params.data_ptr(), lrn.params.data_ptr() + 4 * lrn.params.numel()
    off = lo
    for p, b in zip(mod.parameters(), before):
        assert p.data_ptr() == off and lo <= p.data_ptr() < hi and torch.equal(p.detach(), b)    # nn.Sequential order, values kept
        off += 4 * p.numel()
    with torch.no_grad():
        lrn.params.fill_(0.5)
    assert all(bool((p == 0.5).all()) for p in mod.parameters())
    assert set(mod.state_dict()) == {'0.weight', '0.bias', '2.weight', '2.bias', '4.weight', '4.bias'}
    assert lrn.hyper.tolist() == [float(F(x)) for x in (1e-3, 0.9, 0.999, 1e-8, 10.0, 1.0, 1.0)]


def test_qlearner_refusals_on_the_host():
    """every refusal of the Python layer raises ValueError before a library call (there is no GPU here to call)"""
    from soccer2d_amd.learn import QLearner
    for mod, text in ((seq(10, (12,), 4), 'multiple of 8'), (seq(10, (264,), 4), 'multiple of 8'), (seq(10, (8,) * 5, 4), '1 to 4 hidden'),
                      (seq(257, (8,), 4), 'input width'), (seq(10, (8,), 65), 'output width'), (seq(10, (8,), 4, bias=False), 'bias'),
                      (seq(10, (8,), 4, act=nn.ELU), 'activation'), (nn.Linear(10, 4), 'Q-network'),
                      (seq(10, (8,), 4).double(), 'float32')):
        with pytest.raises(ValueError, match=text):
            QLearner.from_module(mod, device='cpu')
    for kw, text in ((dict(loss='l1'), 'loss'), (dict(max_batch=0), 'max_batch'), (dict(betas=(0.9, 1.0)), 'betas'), (dict(lr=-1.0), 'lr')):
        with pytest.raises(ValueError, match=text):
            QLearner.from_module(seq(10, (8,), 4), device='cpu', **kw)
    with pytest.raises(ValueError, match='torch.nn.Module'):
        QLearner.from_module('q')
    lrn = QLearner.from_module(seq(10, (8,), 4), max_batch=32, device='cpu')
    before = lrn.params.clone()
    B = 8
    good = dict(obs=torch.zeros(B, 10), action=torch.zeros(B, 1, dtype=torch.int32))
    tgt = torch.zeros(B)
    for batch, target, kw, text in (
            ({'obs': good['obs']}, tgt, {}, "'obs' and 'action'"),
            (dict(good, obs=torch.zeros(B, 9)), tgt, {}, r"batch\['obs'\]"),
            (dict(good, obs=torch.zeros(B, 10, dtype=torch.float64)), tgt, {}, r"batch\['obs'\]"),
            (dict(good, action=torch.zeros(B, dtype=torch.int64)), tgt, {}, r"batch\['action'\]"),
            (dict(good, action=torch.zeros(B + 1, dtype=torch.int32)), tgt, {}, r"batch\['action'\]"),
            (good, torch.zeros(B + 1), {}, 'target'),
            (good, tgt, dict(weight=torch.zeros(B, 1)), 'weight'),
            (good, tgt, dict(td_abs_out=torch.zeros(B, dtype=torch.float64)), 'td_abs_out'),
            (dict(obs=torch.zeros(33, 10), action=torch.zeros(33, dtype=torch.int32)), torch.zeros(33), {}, 'max_batch=32'),
            (good, tgt, {}, 'no CPU path')):
        with pytest.raises(ValueError, match=text):
            lrn.step(batch, target, **kw)
    with pytest.raises(ValueError, match='no CPU path'):
        lrn.grad(good, tgt)
    with pytest.raises(ValueError, match='td.QTarget'):
        lrn.update_target(seq(10, (8,), 4))
    assert torch.equal(lrn.params, before)
