"""The fused Q-learner step (s2d_learn_q / s2d_learn_q_grad; soccer2d_amd.learn.QLearner) on the GPU, every comparison bit for bit
against the host restatement tests/learn_ref.c: the flat gradient, norm, scale and loss, td_abs and out_q, and after a step the
parameters, m, v and the beta products -- at every shape and batch edge, on the data edges, against QTarget's forward, eagerly and
from one captured graph of sample -> target -> step, through the class, and every rejection, which launches nothing.  Every
output and the workspace are allocated with sentinel guard words past their end, and the guards are checked.  (The kernels have
no plan override: there is one plan per shape, so the issue's two-plans case has nothing to run.)"""
import ctypes as C

import numpy as np
import pytest

import learn as LR
import replay as RR
import td as TD

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
nn = torch.nn

F = np.float32
DEV = 'cuda:0'
PAD = 64
S_F = -7777.0
R = LR.BLOCK_ROWS
ACT_NN = {'relu': nn.ReLU, 'tanh': nn.Tanh, 'sigmoid': nn.Sigmoid}
BATCHES = (1, R - 1, R, R + 1, 2 * R + 5, 4096)
# every shape at B = 2R + 5; SB3's default shape at every batch edge
CASES = [(s, 2 * R + 5) for s in LR.SHAPES] + [(LR.SHAPES[3], B) for B in BATCHES if B != 2 * R + 5] + [(LR.SHAPES[1], 1), (LR.SHAPES[4], R + 1)]


@pytest.fixture(scope='module')
def L(tmp_path_factory):
    return LR.build(tmp_path_factory.mktemp('learn_ref'))


@pytest.fixture(scope='module')
def T(tmp_path_factory):
    return TD.build(tmp_path_factory.mktemp('td_ref'))


@pytest.fixture(scope='module')
def lib():
    from soccer2d_amd import _capi
    return _capi.load_library()


def same(got, want, what):
    """bit for bit, the sign of zero included; where both are NaN only that they are NaN (the payload is the hardware's)"""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~gn & ~wn & (got.view(np.int32) != want.view(np.int32)))
    if bad.any():
        idx = np.argwhere(bad)
        i = tuple(idx[0])
        raise AssertionError(f'{what}: {len(idx)} of {got.size} differ; first at {i}: gpu={got[i]!r} cpu={want[i]!r}')


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(n, fill=S_F):
    return torch.full((n + PAD,), fill, dtype=torch.float32, device=DEV)


class DevLearner:
    """a tests/td.py Net and a tests/learn.py State on the device behind the raw C ABI: every array with guard words behind it, the
    workspace of exactly the bytes the library asks for"""

    def __init__(self, lib, net, state, loss, max_batch):
        from soccer2d_amd import _capi
        self.lib, self.net, self.P = lib, net, net.params.size
        s, st = _capi.S2DLearnNet(), _capi.S2DLearnState()
        s.n_in, s.n_hidden, s.n_out, s.activation = net.n_in, len(net.hidden), net.n_out, TD.ACT[net.act]
        for l, w in enumerate(net.hidden):
            s.hidden[l] = w
        self.words = lib.s2d_learn_workspace_bytes(C.byref(s), max_batch) // 4
        assert self.words > 0
        self.ws = guarded(self.words, -3333.0)
        self.params, self.m, self.v, self.grad = (guarded(self.P) for _ in range(4))
        self.params[:self.P] = to_dev(net.params)
        self.m[:self.P], self.v[:self.P] = to_dev(state.m), to_dev(state.v)
        self.hyper, self.stats = guarded(7), guarded(3)
        self.hyper[:7] = to_dev(state.hyper)
        self.error = torch.zeros(1 + PAD, dtype=torch.int32, device=DEV)
        s.params, s.workspace, s.workspace_bytes = self.params.data_ptr(), self.ws.data_ptr(), self.words * 4
        st.m, st.v, st.grad, st.hyper, st.stats, st.error = (t.data_ptr() for t in (self.m, self.v, self.grad, self.hyper, self.stats, self.error))
        st.loss_kind = LR.LOSS[loss]
        self.s, self.st = s, st

    def call(self, fn, obs, action, target, weight, with_outs=True):
        """one s2d_learn_q / s2d_learn_q_grad on device copies; returns (rc, td_abs, q); guards checked"""
        B = obs.shape[0]
        o, a, t = to_dev(obs.astype(F)), to_dev(action.astype(np.int32)), to_dev(target.astype(F))
        w = to_dev(weight.astype(F)) if weight is not None else None
        td_abs, q = (guarded(B), guarded(B * self.net.n_out)) if with_outs else (None, None)
        torch.cuda.synchronize()
        rc = getattr(self.lib, fn)(B, C.byref(self.s), C.byref(self.st), o.data_ptr(), a.data_ptr(), t.data_ptr(),
                                   w.data_ptr() if w is not None else None, td_abs.data_ptr() if with_outs else None,
                                   q.data_ptr() if with_outs else None, None)
        torch.cuda.synchronize()
        self.check_guards()
        if not with_outs:
            return rc, None, None
        for x, n in ((td_abs, B), (q, B * self.net.n_out)):
            assert bool((x[n:] == S_F).all()), 'wrote past an output'
        return rc, td_abs[:B], q[:B * self.net.n_out].view(B, self.net.n_out)

    def check_guards(self):
        assert bool((self.ws[self.words:] == -3333.0).all()), 'wrote past the workspace'
        for x, n in ((self.params, self.P), (self.m, self.P), (self.v, self.P), (self.grad, self.P), (self.hyper, 7), (self.stats, 3)):
            assert bool((x[n:] == S_F).all()), 'wrote past a state array'
        assert bool((self.error[1:] == 0).all())

    def ok(self, rc, fn):
        from soccer2d_amd import _capi
        _capi.check(self.lib, rc, fn)


def check_grad(dev, got, want, what):
    rc, td_abs, q = got
    same(dev.grad[:dev.P], want['grad'], f'{what}: grad')
    same(dev.stats[:3], want['stats'], f'{what}: stats (loss, norm, scale)')
    same(td_abs, want['td_abs'], f'{what}: td_abs')
    same(q, want['q'], f'{what}: out_q')
    assert int(dev.error[0]) == want['error'], what


def check_state(dev, net, state, what):
    same(dev.params[:dev.P], net.params, f'{what}: params')
    same(dev.m[:dev.P], state.m, f'{what}: m')
    same(dev.v[:dev.P], state.v, f'{what}: v')
    same(dev.hyper[:7], state.hyper, f'{what}: hyper (the beta products)')


def copy_net(net):
    return TD.Net(net.n_in, net.hidden, net.n_out, net.act, net.params.copy())


def grad_then_steps(L, lib, net, loss, batches, max_grad_norm=10.0, lr=1e-2):
    """s2d_learn_q_grad on the first batch, then one s2d_learn_q per batch, each compared with the restatement"""
    state = LR.State(net.params.size, lr=lr, max_grad_norm=max_grad_norm)
    dev = DevLearner(lib, net, state, loss, max(b[0].shape[0] for b in batches))
    before = (net.params.copy(), state.hyper.copy())
    obs, action, target, weight = batches[0]
    got = dev.call('s2d_learn_q_grad', obs, action, target, weight)
    dev.ok(got[0], 's2d_learn_q_grad')
    check_grad(dev, got, LR.grad(L, net, loss, obs, action, target, weight, max_grad_norm), 'grad')
    same(dev.params[:dev.P], before[0], 'grad leaves params')
    same(dev.hyper[:7], before[1], 'grad leaves the beta products')
    assert bool((dev.m[:dev.P] == 0).all()) and bool((dev.v[:dev.P] == 0).all())
    for n, (obs, action, target, weight) in enumerate(batches):
        dev.error.zero_()
        got = dev.call('s2d_learn_q', obs, action, target, weight)
        dev.ok(got[0], 's2d_learn_q')
        check_grad(dev, got, LR.step(L, net, state, loss, obs, action, target, weight), f'step {n}')
        check_state(dev, net, state, f'step {n}')
    return dev


def test_cases_cover_every_axis_value():
    shapes = [c[0] for c in CASES]
    assert {s[0] for s in shapes} >= {1, 4, 10, 13, 256} and {s[2] for s in shapes} >= {1, 3, 16, 17, 64}
    assert {s[1] for s in shapes} >= {(8,), (8, 16), (24, 40), (64, 64), (128, 64, 32, 16), (256, 256)}
    assert {s[3] for s in shapes} == {'relu', 'tanh', 'sigmoid'} and {B for s, B in CASES if s == LR.SHAPES[3]} == set(BATCHES)


@pytest.mark.parametrize('shape, B', CASES, ids=lambda v: str(v) if isinstance(v, int) else '-'.join(map(str, (v[0],) + v[1] + (v[2],))) + v[3])
def test_grad_and_step_equal_the_restatement(L, lib, shape, B):
    """Huber with weights: the gradient call, then two steps (the second on moved parameters and a non-trivial Adam state)"""
    n_in, hidden, n_out, act = shape
    rs = np.random.RandomState(B + n_in)
    net = TD.random_net(rs, n_in, hidden, n_out, act)
    grad_then_steps(L, lib, net, 'huber', [LR.random_batch(rs, net, B) for _ in range(2)], max_grad_norm=0.05)


@pytest.mark.parametrize('loss, weighted, mx', [('mse', False, 10.0), ('mse', True, 0.0), ('huber', False, -1.0)])
def test_loss_kinds_weights_and_clip(L, lib, loss, weighted, mx):
    rs = np.random.RandomState(21)
    net = TD.random_net(rs, 13, (24, 40), 17, 'sigmoid')
    batches = [LR.random_batch(rs, net, R + 7) for _ in range(2)]
    if not weighted:
        batches = [(o, a, t, None) for o, a, t, _ in batches]
    dev = grad_then_steps(L, lib, net, loss, batches, max_grad_norm=mx)
    assert float(dev.stats[2]) == 1.0


def test_data_edges(L, lib):
    """all actions in one column; a column never chosen (its gradient is exactly +0); all weights zero; a NaN target; an action
    out of range (a zero row and the error word)"""
    rs = np.random.RandomState(31)
    net = TD.random_net(rs, 10, (64, 64), 16, 'relu')
    B, P = 2 * R + 5, net.params.size
    obs, action, target, weight = LR.random_batch(rs, net, B)
    out_w, out_b = slice(P - 16 - 16 * 64, P - 16), slice(P - 16, P)

    def run(action, target, weight, what):
        state = LR.State(P)
        dev = DevLearner(lib, net, state, 'huber', B)
        got = dev.call('s2d_learn_q_grad', obs, action, target, weight)
        dev.ok(got[0], 's2d_learn_q_grad')
        want = LR.grad(L, net, 'huber', obs, action, target, weight)
        check_grad(dev, got, want, what)
        return dev.grad[:P].cpu().numpy(), want

    g, _ = run(np.full(B, 5, np.int32), target, weight, 'one column')
    rows = g[out_w].reshape(16, 64)
    assert (TD.bits(np.delete(rows, 5, 0)) == 0).all() and (TD.bits(np.delete(g[out_b], 5)) == 0).all() and g[out_b][5] != 0
    a = np.where(action == 7, 8, action).astype(np.int32)
    g, _ = run(a, target, weight, 'column 7 never chosen')
    assert (TD.bits(g[out_w].reshape(16, 64)[7]) == 0).all() and TD.bits(g[out_b])[7] == 0 and (g[out_b][[6, 8]] != 0).all()
    g, want = run(action, target, np.zeros(B, F), 'weights all zero')
    assert (g == 0).all() and want['stats'][0] == 0 and want['stats'][1] == 0 and (want['td_abs'] > 0).any()
    t = target.copy()
    t[70] = np.nan
    g, want = run(action, t, weight, 'NaN target')
    assert np.isnan(want['stats'][:2]).all() and np.isnan(g).any() and np.isnan(want['td_abs'][70]) and np.isnan(want['td_abs']).sum() == 1
    for bad in (16, -1, 2 ** 31 - 1, -2 ** 31):
        a = action.copy()
        a[R] = bad
        g, want = run(a, target, weight, f'action {bad}')
        assert want['error'] == 1 and want['td_abs'][R] == 0
    # the step with a bad action still updates from the other rows, as the restatement does
    a = action.copy()
    a[3] = 99
    state = LR.State(P)
    dev = DevLearner(lib, net, state, 'huber', B)
    got = dev.call('s2d_learn_q', obs, a, target, weight)
    check_grad(dev, got, LR.step(L, net, state, 'huber', obs, a, target, weight), 'step with a bad action')
    check_state(dev, net, state, 'step with a bad action')


def test_td_error_of_exactly_one_and_zero(L, lib):
    """the 1-8-1 hand network of test_learn_host.py: TD errors of exactly +1, -1, 0 and 2, a ReLU pre-activation of exactly 0"""
    W1, b1 = np.array([1, -1, 0.5, 0, 0, 0, 0, 0], F), np.array([0, 0, -0.5, 0, 0, 0, 0, 0], F)
    net = TD.Net(1, (8,), 1, 'relu', np.concatenate([W1, b1, np.array([2, 3, 5, 0, 0, 0, 0, 0], F), [0.25]]).astype(F))
    obs, action = np.array([[1.0], [1.0], [-1.0], [1.0]], F), np.zeros(4, np.int32)
    target = np.array([1.25, 3.25, 3.25, 0.25], F)
    for loss in ('huber', 'mse'):
        dev = DevLearner(lib, net, LR.State(25), loss, 4)
        got = dev.call('s2d_learn_q_grad', obs, action, target, None)
        want = LR.grad(L, net, loss, obs, action, target, None)
        check_grad(dev, got, want, loss)
        assert got[1].tolist() == [1.0, 1.0, 0.0, 2.0] and got[2].view(-1).tolist() == [2.25, 2.25, 3.25, 2.25]
        d = [1, -1, 0, 1 if loss == 'huber' else 2]
        assert dev.grad[24].item() == sum(d) / 4 and dev.grad[2].item() == 0.0          # db_out; the unit at exactly 0 gets nothing


def seq(n_in, hidden, n_out, act='relu'):
    layers, win = [], n_in
    for w in hidden:
        layers += [nn.Linear(win, w), ACT_NN[act]()]
        win = w
    return nn.Sequential(*layers, nn.Linear(win, n_out)).to(DEV)


def net_of(module, act):
    lin = [m for m in module if isinstance(m, nn.Linear)]
    p = np.concatenate([np.concatenate([l.weight.detach().cpu().numpy().ravel(), l.bias.detach().cpu().numpy().ravel()]) for l in lin])
    return TD.Net(lin[0].in_features, [l.out_features for l in lin[:-1]], lin[-1].out_features, act, p)


@pytest.mark.parametrize('n_in, hidden, n_out, act', [(10, (64, 64), 16, 'relu'), (13, (24, 40), 17, 'sigmoid'), (4, (128, 64, 32, 16), 3, 'tanh')])
def test_forward_is_the_target_kernels(T, n_in, hidden, n_out, act):
    """the forward identity: out_q[b][index[b]] has the bits of the q that QTarget (s2d_td_target_q) returns for the same
    parameters and rows, and the whole of out_q those of td_ref.c"""
    from soccer2d_amd.learn import QLearner
    from soccer2d_amd.td import QTarget
    torch.manual_seed(n_in)
    mod = seq(n_in, hidden, n_out, act)
    lrn = QLearner.from_module(mod, max_batch=200)
    B = 2 * R + 5
    x = torch.randn(B, n_in, device=DEV)
    batch = {'obs': x, 'action': torch.zeros(B, dtype=torch.int32, device=DEV), 'next_obs': x,
             'reward': torch.zeros(B, device=DEV), 'discount': torch.ones(B, device=DEV)}
    _, q, index = QTarget.from_module(mod).target(batch, return_q=True)
    out_q = torch.full((B, n_out), S_F, device=DEV)
    lrn.grad(batch, torch.zeros(B, device=DEV), q_out=out_q)
    torch.cuda.synchronize()
    assert torch.equal(out_q.gather(1, index.long().unsqueeze(1)).squeeze(1).view(torch.int32), q.view(torch.int32))
    same(out_q, TD.forward(T, net_of(mod, act), x.cpu().numpy()), 'out_q against td_ref.c')


def dev_rec(rec):
    return {k: torch.from_numpy(v).to(DEV) for k, v in rec.items() if v is not None}


def test_five_steps_eagerly_and_from_one_captured_graph(L, T):
    """sample -> target -> step five times eagerly == five replays of one captured graph of the three == the restatement on the
    batches the graph drew, bit for bit; set_lr between replays takes effect"""
    from soccer2d_amd.learn import QLearner
    from soccer2d_amd.replay import DeviceReplay
    from soccer2d_amd.td import QTarget
    torch.manual_seed(6)
    rng = np.random.default_rng(6)
    B, D = 2 * R + 5, 10
    rec, first = RR.synthetic_record(rng, 4, 60, D, 1)
    online0, qt = seq(D, (64, 64), 16), seq(D, (32,), 16, 'tanh')

    def make():
        mod = seq(D, (64, 64), 16)
        mod.load_state_dict(online0.state_dict())
        rb = DeviceReplay(512, D, device=DEV, seed=9)
        rb.push(dev_rec(rec), torch.from_numpy(first).to(DEV))
        lrn = QLearner.from_module(mod, lr=1e-2, max_grad_norm=0.5, max_batch=B)
        return mod, rb, lrn, QTarget.from_module(qt), rb.alloc_batch(B), torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    lrs = [1e-2, 1e-2, 3e-3, 3e-3, 1e-3]
    # eagerly
    mod_e, rb_e, lrn_e, td_e, batch_e, tgt_e, abs_e = make()
    for lr in lrs:
        lrn_e.set_lr(lr)
        lrn_e.step(rb_e.sample(B, out=batch_e), td_e.target(batch_e, out=tgt_e), td_abs_out=abs_e)
    # captured once, replayed five times
    mod_g, rb_g, lrn_g, td_g, batch_g, tgt_g, abs_g = make()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                            # a warm-up outside the capture, on objects of its own
        w = make()
        w[2].step(w[1].sample(B, out=w[4]), w[3].target(w[4], out=w[5]), td_abs_out=w[6])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lrn_g.step(rb_g.sample(B, out=batch_g), td_g.target(batch_g, out=tgt_g), td_abs_out=abs_g)
    torch.cuda.synchronize()
    same(lrn_g.params, net_of(online0, 'relu').params, 'capturing ran nothing')
    net, state = net_of(online0, 'relu'), LR.State(lrn_g.params.numel(), lr=1e-2, max_grad_norm=0.5)
    tnet = net_of(qt, 'tanh')
    for n, lr in enumerate(lrs):
        lrn_g.set_lr(lr)
        graph.replay()
        torch.cuda.synchronize()
        h = {k: v.cpu().numpy() for k, v in batch_g.items()}
        target = TD.target_q(T, tnet, None, h['next_obs'], h['reward'], h['discount'])[0]
        same(tgt_g, target, f'replay {n}: target')
        state.hyper[0] = F(lr)
        want = LR.step(L, net, state, 'huber', h['obs'], h['action'].reshape(-1), target)
        same(abs_g, want['td_abs'], f'replay {n}: td_abs')
        same(lrn_g._grad, want['grad'], f'replay {n}: grad')
        same(lrn_g.stats, want['stats'], f'replay {n}: stats')
        same(lrn_g.params, net.params, f'replay {n}: params')
        same(lrn_g.hyper, state.hyper, f'replay {n}: hyper')
        assert lrn_g.loss == float(want['stats'][0]) and lrn_g.grad_norm == float(want['stats'][1]) and lrn_g.clip_scale == float(want['stats'][2])
    for name, a, b in (('params', lrn_e.params, lrn_g.params), ('m', lrn_e.m, lrn_g.m), ('v', lrn_e.v, lrn_g.v), ('hyper', lrn_e.hyper, lrn_g.hyper),
                       ('td_abs', abs_e, abs_g)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'eager against graph: {name}'
    same(lrn_g.m, state.m, 'm'), same(lrn_g.v, state.v, 'v')
    for p_e, p_g in zip(mod_e.parameters(), mod_g.parameters()):             # the modules hold the learners' weights
        assert torch.equal(p_e, p_g)
    assert not torch.equal(lrn_g.params, to_dev(net_of(online0, 'relu').params))


def test_qlearner_views_actor_sync_and_update_target():
    from soccer2d_amd.learn import QLearner
    from soccer2d_amd.td import QTarget
    from soccer2d_amd.wide_actor import WideQNetActor
    torch.manual_seed(8)
    mod, tmod = seq(10, (64, 64), 16), seq(10, (64, 64), 16)
    lrn = QLearner.from_module(mod, lr=1e-2, max_batch=256)
    lo, hi = lrn.params.data_ptr(), lrn.params.data_ptr() + 4 * lrn.params.numel()
    assert all(lo <= p.data_ptr() < hi for p in mod.parameters()) and all(p.device == lrn.device for p in mod.parameters())
    actor = WideQNetActor.from_module(mod)
    td = QTarget.from_module(tmod, online=mod)
    B = 200
    batch = {'obs': torch.randn(B, 10, device=DEV), 'action': torch.randint(0, 16, (B, 1), dtype=torch.int32, device=DEV)}
    before = lrn.params.clone()
    lrn.step(batch, torch.randn(B, device=DEV), weight=torch.rand(B, device=DEV))
    assert not torch.equal(lrn.params, before) and lrn.loss > 0 and lrn.grad_norm > 0 and 0 < lrn.clip_scale <= 1
    flat = torch.cat([p.detach().reshape(-1) for p in mod.parameters()])
    assert torch.equal(flat, lrn.params)                                     # the module IS the flat buffer
    actor.sync(), td.online.sync()
    want = actor.params.clone()
    fresh = WideQNetActor.from_module(mod)
    assert torch.equal(fresh.params, want) and torch.equal(td.online.params, lrn.params)
    assert set(mod.state_dict()) == {'0.weight', '0.bias', '2.weight', '2.bias', '4.weight', '4.bias'}
    # update_target: lerp_ / copy_ on the flat buffers, bit for bit, and the target module follows
    old = td.q_target.params.clone()
    lrn.update_target(td, tau=0.005)
    assert torch.equal(td.q_target.params, old.lerp(lrn.params, 0.005)) and not torch.equal(td.q_target.params, old)
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in tmod.parameters()]), td.q_target.params)
    td.q_target.sync()                                                       # the module round trip still works
    assert torch.equal(td.q_target.params, old.lerp(lrn.params, 0.005))
    lrn.update_target(td)
    assert torch.equal(td.q_target.params, lrn.params)
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in tmod.parameters()]), lrn.params)
    # reset_optimizer, set_lr, and the lazily surfaced error word
    lrn.reset_optimizer(), lrn.set_lr(0.25)
    assert lrn.hyper.tolist() == [0.25, float(F(0.9)), float(F(0.999)), float(F(1e-8)), 10.0, 1.0, 1.0] and not lrn.m.any() and not lrn.v.any()
    bad = dict(batch, action=torch.full((B,), 16, dtype=torch.int32, device=DEV))
    lrn.grad(bad, torch.randn(B, device=DEV))
    with pytest.raises(ValueError, match='action outside'):
        lrn.loss
    assert lrn.loss == 0.0                                                   # the word was cleared
    with pytest.raises(ValueError, match='target network is'):
        lrn.update_target(QTarget.from_module(seq(10, (32,), 16)))


def test_rejections_return_einval_with_text_and_launch_nothing(L, lib):
    from soccer2d_amd import _capi
    from soccer2d_amd.learn import QLearner
    rs = np.random.RandomState(9)
    net = TD.random_net(rs, 10, (16, 8), 4, 'relu')
    B = 70
    obs, action, target, weight = LR.random_batch(rs, net, B)
    dev = DevLearner(lib, net, LR.State(net.params.size), 'huber', B)
    o, a, t, w = to_dev(obs), to_dev(action), to_dev(target), to_dev(weight)
    out = guarded(B)
    snap = [x.clone() for x in (dev.params, dev.m, dev.v, dev.grad, dev.hyper, dev.stats, dev.ws, out)]

    def refused(rc, text):
        torch.cuda.synchronize()
        assert rc == _capi.S2D_EINVAL and text in lib.s2d_last_error().decode(), (text, lib.s2d_last_error())
        for x, y in zip((dev.params, dev.m, dev.v, dev.grad, dev.hyper, dev.stats, dev.ws, out), snap):
            assert torch.equal(x, y), f'{text}: something was written'

    def call(fn='s2d_learn_q', batch=B, net_=None, st_=None, o_=o.data_ptr(), a_=a.data_ptr(), t_=t.data_ptr(), w_=w.data_ptr(),
             abs_=out.data_ptr(), q_=None):
        return getattr(lib, fn)(batch, C.byref(net_ or dev.s), C.byref(st_ or dev.st), o_, a_, t_, w_, abs_, q_, None)

    def copy_of(s, **changes):
        c = type(s)()
        C.memmove(C.byref(c), C.byref(s), C.sizeof(s))
        for k, v in changes.items():
            setattr(c, k, v)
        return c

    def hidden(*ws):
        return (C.c_int32 * 5)(*ws)
    for fn in ('s2d_learn_q', 's2d_learn_q_grad'):
        for changes, text in ((dict(n_in=0), 'n_in'), (dict(n_in=257), 'n_in'), (dict(n_hidden=0), 'n_hidden'), (dict(n_hidden=5), 'n_hidden'),
                              (dict(hidden=hidden(16, 12)), 'hidden widths'), (dict(hidden=hidden(264, 8)), 'hidden widths'),
                              (dict(hidden=hidden(16, 8, 8)), 'hidden widths'), (dict(n_out=0), 'n_out'), (dict(n_out=65), 'n_out'),
                              (dict(activation=3), 'activation'), (dict(params=None), 'params'), (dict(params=dev.params.data_ptr() + 4), 'params'),
                              (dict(workspace=None), 'workspace'), (dict(workspace=dev.ws.data_ptr() + 16), 'workspace'),
                              (dict(workspace_bytes=dev.words * 4 - 4), 'workspace_bytes'),
                              (dict(workspace=dev.params.data_ptr()), 'overlap'), (dict(params=dev.grad.data_ptr()), 'overlap')):
            refused(call(fn, net_=copy_of(dev.s, **changes)), text)
        for changes, text in ((dict(loss_kind=2), 'loss_kind'), (dict(loss_kind=-1), 'loss_kind'), (dict(grad=None), 'grad'),
                              (dict(grad=dev.grad.data_ptr() + 4), 'grad'), (dict(hyper=None), 'hyper'), (dict(stats=dev.stats.data_ptr() + 2), 'stats'),
                              (dict(error=None), 'error'), (dict(grad=dev.ws.data_ptr() + 256), 'overlap')):
            refused(call(fn, st_=copy_of(dev.st, **changes)), text)
        for kw, text in ((dict(batch=0), 'batch'), (dict(batch=-3), 'batch'), (dict(batch=2 ** 31), 'batch'), (dict(batch=B + 64), 'max_batch'),
                         (dict(o_=None), 'obs'), (dict(a_=a.data_ptr() + 2), 'action'), (dict(t_=None), 'target'),
                         (dict(w_=w.data_ptr() + 1), 'weight'), (dict(abs_=out.data_ptr() + 3), 'out_td_abs'), (dict(q_=out.data_ptr() + 2), 'out_q')):
            refused(call(fn, **kw), text)
    for changes, text in ((dict(m=None), 'm and v'), (dict(v=dev.v.data_ptr() + 8), 'm and v'), (dict(m=dev.v.data_ptr()), 'overlap'),
                          (dict(v=dev.params.data_ptr() + 16), 'overlap')):
        refused(call('s2d_learn_q', st_=copy_of(dev.st, **changes)), text)
    assert lib.s2d_learn_q(B, None, C.byref(dev.st), o.data_ptr(), a.data_ptr(), t.data_ptr(), None, None, None, None) == _capi.S2D_EINVAL
    # s2d_learn_q_grad does not read m and v
    assert call('s2d_learn_q_grad', st_=copy_of(dev.st, m=None, v=None)) == _capi.S2D_OK
    torch.cuda.synchronize()
    same(dev.grad[:dev.P], LR.grad(L, net, 'huber', obs, action, target, weight)['grad'], 'grad without m and v')
    dev.check_guards()
    # through the class: a ValueError, and the parameters stay
    lrn = QLearner.from_module(seq(10, (16, 8), 4), max_batch=64)
    before = lrn.params.clone()
    batch = {'obs': o[:64], 'action': a[:64]}
    for b_, t_, kw, text in ((dict(batch, obs=o[:64].cpu()), t[:64], {}, r"batch\['obs'\]"), (batch, t[:63], {}, 'target'),
                             (dict(batch, action=a[:64].long()), t[:64], {}, r"batch\['action'\]"), (batch, t[:64], dict(weight=w[:64].double()), 'weight'),
                             ({'obs': o, 'action': a}, t, {}, 'max_batch=64'), (batch, t[:64], dict(td_abs_out=out[:128][::2]), 'td_abs_out')):
        with pytest.raises(ValueError, match=text):
            lrn.step(b_, t_, **kw)
    torch.cuda.synchronize()
    assert torch.equal(lrn.params, before)
