"""The fused DDPG / TD3 update (s2d_learn_critic / s2d_learn_actor and their _grad twins; soccer2d_amd.learn.ActorCriticLearner) on
the GPU, every comparison bit for bit against the host restatement tests/learn_ac_ref.c: the flat gradients, the three stats,
td_abs, out_q and out_action, and after a step the parameters, m, v and the beta products -- at every shape and batch edge, for
every loss, weight and clip regime, on the data edges, against ActorCriticTarget's forward, eagerly and from one captured graph of
sample -> target -> step_critic -> step_actor -> update_targets, through the class, and every rejection, which launches nothing.
Every output and workspace is allocated with sentinel guard words past its end, and the guards are checked."""
import ctypes as C

import numpy as np
import pytest

import learn as LR
import learn_ac as AC
import replay as RR
import td as TD

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
nn = torch.nn

F = np.float32
DEV = 'cuda:0'
PAD = 64
S_F = -7777.0
S_W = -3333.0
R = AC.BLOCK_ROWS
ACT_NN = {'relu': nn.ReLU, 'tanh': nn.Tanh, 'sigmoid': nn.Sigmoid}
MIXED = (10, 1, (64, 64), (64, 64), ('tanh', 'relu'))                       # actor tanh with critic relu
CASES = [(s, 133) for s in AC.SHAPES] + [(AC.REACH_BALL, B) for B in (1, 63, 64, 65, 4096)] + [(MIXED, 133)]


@pytest.fixture(scope='module')
def L(tmp_path_factory):
    return AC.build(tmp_path_factory.mktemp('learn_ac_ref'))


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


def pair_of(rs, shape):
    D, A, ha, hc, act = shape
    act_a, act_c = act if isinstance(act, tuple) else (act, act)
    return AC.random_pair(rs, D, A, ha, hc, act_a, act_c)


def c_shape(net):
    from soccer2d_amd import _capi
    s = _capi.S2DLearnNet()
    s.n_in, s.n_hidden, s.n_out, s.activation = net.n_in, len(net.hidden), net.n_out, TD.ACT[net.act]
    for l, w in enumerate(net.hidden):
        s.hidden[l] = w
    return s


class DevNet:
    """a tests/td.py Net and a tests/learn.py State on the device behind the raw C ABI: every array with guard words behind it, the
    workspace of exactly `words` words"""

    def __init__(self, net, state, loss, words):
        from soccer2d_amd import _capi
        self.net, self.P, self.words = net, net.params.size, words
        s, st = c_shape(net), _capi.S2DLearnState()
        self.ws = guarded(words, S_W)
        self.params, self.m, self.v, self.grad = (guarded(self.P) for _ in range(4))
        self.params[:self.P] = to_dev(net.params)
        self.m[:self.P], self.v[:self.P] = to_dev(state.m), to_dev(state.v)
        self.hyper, self.stats = guarded(7), guarded(3)
        self.hyper[:7] = to_dev(state.hyper)
        self.error = torch.zeros(1 + PAD, dtype=torch.int32, device=DEV)
        s.params, s.workspace, s.workspace_bytes = self.params.data_ptr(), self.ws.data_ptr(), words * 4
        st.m, st.v, st.grad, st.hyper, st.stats, st.error = (t.data_ptr() for t in (self.m, self.v, self.grad, self.hyper, self.stats, self.error))
        st.loss_kind = AC.LOSS[loss]
        self.s, self.st = s, st

    def arrays(self):
        return (self.params, self.m, self.v, self.grad, self.hyper, self.stats, self.ws)

    def check_guards(self):
        assert bool((self.ws[self.words:] == S_W).all()), 'wrote past the workspace'
        for x, n in ((self.params, self.P), (self.m, self.P), (self.v, self.P), (self.grad, self.P), (self.hyper, 7), (self.stats, 3)):
            assert bool((x[n:] == S_F).all()), 'wrote past a state array'
        assert bool((self.error == 0).all()), 'the error word was written'

    def check_state(self, net, state, what):
        same(self.params[:self.P], net.params, f'{what}: params')
        same(self.m[:self.P], state.m, f'{what}: m')
        same(self.v[:self.P], state.v, f'{what}: v')
        same(self.hyper[:7], state.hyper, f'{what}: hyper (the beta products)')

    def snapshot(self):
        return [x.clone() for x in (self.params, self.m, self.v, self.hyper)]

    def unchanged(self, snap, what):
        for x, y in zip((self.params, self.m, self.v, self.hyper), snap):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), what


def dev_critic(lib, critic, state, loss, max_batch):
    words = lib.s2d_learn_workspace_bytes(C.byref(c_shape(critic)), max_batch) // 4
    assert words > 0
    return DevNet(critic, state, loss, words)


def dev_actor(lib, actor, critic, state, max_batch):
    words = lib.s2d_learn_actor_workspace_bytes(C.byref(c_shape(actor)), C.byref(c_shape(critic)), max_batch) // 4
    assert words > 0
    return DevNet(actor, state, 'mse', words)


def outputs(*sizes):
    return [guarded(n) for n in sizes]


def check_outputs(outs, sizes):
    for x, n in zip(outs, sizes):
        assert bool((x[n:] == S_F).all()), 'wrote past an output'


def critic_call(lib, fn, dev, A, obs, action, target, weight):
    """one s2d_learn_critic / _grad on device copies; returns (td_abs, q); guards checked"""
    from soccer2d_amd import _capi
    B = obs.shape[0]
    o, a, t = to_dev(obs.astype(F)), to_dev(action.astype(F)), to_dev(target.astype(F))
    w = to_dev(weight.astype(F)) if weight is not None else None
    td_abs, q = outputs(B, B)
    torch.cuda.synchronize()
    rc = getattr(lib, fn)(B, C.byref(dev.s), C.byref(dev.st), o.data_ptr(), A, a.data_ptr(), t.data_ptr(), w.data_ptr() if w is not None else None,
                          td_abs.data_ptr(), q.data_ptr(), None)
    torch.cuda.synchronize()
    _capi.check(lib, rc, fn)
    dev.check_guards()
    check_outputs((td_abs, q), (B, B))
    return td_abs[:B], q[:B]


def actor_call(lib, fn, dev, devc, obs):
    """one s2d_learn_actor / _grad; returns (action [B][A], q [B]); guards of both networks checked"""
    from soccer2d_amd import _capi
    B, A = obs.shape[0], dev.net.n_out
    o = to_dev(obs.astype(F))
    act, q = outputs(B * A, B)
    torch.cuda.synchronize()
    rc = getattr(lib, fn)(B, C.byref(dev.s), C.byref(dev.st), C.byref(devc.s), o.data_ptr(), act.data_ptr(), q.data_ptr(), None)
    torch.cuda.synchronize()
    _capi.check(lib, rc, fn)
    dev.check_guards(), devc.check_guards()
    check_outputs((act, q), (B * A, B))
    return act[:B * A].view(B, A), q[:B]


def check_critic(dev, got, want, what):
    same(dev.grad[:dev.P], want['grad'], f'{what}: grad')
    same(dev.stats[:3], want['stats'], f'{what}: stats (loss, norm, scale)')
    same(got[0], want['td_abs'], f'{what}: td_abs')
    same(got[1], want['q'], f'{what}: out_q')


def check_actor(dev, got, want, what):
    same(dev.grad[:dev.P], want['grad'], f'{what}: grad')
    same(dev.stats[:3], want['stats'], f'{what}: stats (-mean q, norm, scale)')
    same(got[0], want['action'], f'{what}: out_action')
    same(got[1], want['q'], f'{what}: out_q')


def run_pair(L, lib, actor, critic, loss, batches, max_grad_norm, lr=1e-2):
    """the gradient calls on the first batch, then per batch one critic step and one actor step (through the updated critic), each
    compared with the restatement; each network bitwise untouched by the other's calls.  Returns the two DevNets and the last
    restated results."""
    A = actor.n_out
    sc, sa = LR.State(critic.params.size, lr=lr, max_grad_norm=max_grad_norm), LR.State(actor.params.size, lr=lr, max_grad_norm=max_grad_norm)
    Bmax = max(b[0].shape[0] for b in batches)
    dc, da = dev_critic(lib, critic, sc, loss, Bmax), dev_actor(lib, actor, critic, sa, Bmax)
    obs, action, target, weight = batches[0]
    snap_c, snap_a = dc.snapshot(), da.snapshot()
    got = critic_call(lib, 's2d_learn_critic_grad', dc, A, obs, action, target, weight)
    check_critic(dc, got, AC.critic_grad(L, critic, loss, obs, action, target, weight, max_grad_norm), 'critic grad')
    got = actor_call(lib, 's2d_learn_actor_grad', da, dc, obs)
    check_actor(da, got, AC.actor_grad(L, actor, critic, obs, max_grad_norm), 'actor grad')
    dc.unchanged(snap_c, 'the gradient calls leave the critic'), da.unchanged(snap_a, 'the gradient calls leave the actor')
    want_c = want_a = None
    for n, (obs, action, target, weight) in enumerate(batches):
        snap_a = da.snapshot()
        got = critic_call(lib, 's2d_learn_critic', dc, A, obs, action, target, weight)
        want_c = AC.critic_step(L, critic, sc, loss, obs, action, target, weight)
        check_critic(dc, got, want_c, f'critic step {n}')
        dc.check_state(critic, sc, f'critic step {n}')
        da.unchanged(snap_a, 'the critic step leaves the actor')
        snap_c, grad_c = dc.snapshot(), dc.grad.clone()
        got = actor_call(lib, 's2d_learn_actor', da, dc, obs)
        want_a = AC.actor_step(L, actor, critic, sa, obs)
        check_actor(da, got, want_a, f'actor step {n}')
        da.check_state(actor, sa, f'actor step {n}')
        dc.unchanged(snap_c, 'the actor step leaves the critic\'s params, m, v and beta products')
        assert torch.equal(dc.grad.view(torch.int32), grad_c.view(torch.int32)), 'the actor step touched the critic\'s gradient'
    return dc, da, want_c, want_a


def test_cases_cover_the_issues_list():
    shapes = [c[0] for c in CASES]
    assert {(s[0], s[1]) for s in shapes} >= {(1, 1), (10, 1), (10, 4), (4, 4), (13, 8), (248, 8)}
    assert {B for s, B in CASES if s == AC.REACH_BALL} == {1, 63, 64, 65, 133, 4096} and MIXED in shapes
    assert {s[4] for s in AC.SHAPES} == {'relu', 'tanh', 'sigmoid'}


@pytest.mark.parametrize('shape, B', CASES, ids=lambda v: str(v) if isinstance(v, int) else AC.shape_id(v[:4] + (''.join(v[4]),)))
def test_grad_and_step_equal_the_restatement(L, lib, shape, B):
    """the square loss with weights and an active clip: both gradient calls, then two rounds of critic step and actor step (the
    second on moved parameters and a non-trivial Adam state)"""
    rs = np.random.RandomState(B + shape[0])
    actor, critic = pair_of(rs, shape)
    _, da, want_c, _ = run_pair(L, lib, actor, critic, 'square', [AC.random_batch(rs, critic, shape[1], B) for _ in range(2)], max_grad_norm=0.05)
    assert float(want_c['stats'][2]) < 1.0


@pytest.mark.parametrize('clip', ['active', 'inactive', 'off'])
@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize('loss', ['square', 'mse', 'huber'])
def test_loss_kinds_weights_and_clip(L, lib, loss, weighted, clip):
    """every loss with and without weights under a clip that scales, one that does not and none; the inputs reach each regime: TD
    errors on both sides of Huber's 1, both gradient norms between 1e-3 and 1e3"""
    rs = np.random.RandomState(21)
    actor, critic = pair_of(rs, (13, 8, (24, 40), (40, 24), 'sigmoid'))
    batches = [AC.random_batch(rs, critic, 8, R + 7) for _ in range(2)]
    if not weighted:
        batches = [(o, a, t, None) for o, a, t, _ in batches]
    mx = {'active': 1e-3, 'inactive': 1e3, 'off': 0.0}[clip]
    dc, da, want_c, want_a = run_pair(L, lib, actor, critic, loss, batches, max_grad_norm=mx)
    for want in (want_c, want_a):
        assert 1e-3 < want['stats'][1] < 1e3 and (want['stats'][2] < 1.0) == (clip == 'active')
    assert (want_c['td_abs'] > 1).any() and (want_c['td_abs'] < 1).any()


def test_data_edges(L, lib):
    """a NaN and an inf observation row; a saturated action (|a| == 1, dz == 0: that row adds exactly nothing); a dead-ReLU critic
    (no hidden unit fires: the actor's gradient is exactly +0); a zero weight"""
    rs = np.random.RandomState(31)
    shape = AC.REACH_BALL
    B = 2 * R + 5
    actor, critic = pair_of(rs, shape)
    obs, action, target, weight = AC.random_batch(rs, critic, 1, B)

    def run(actor, critic, obs, weight, what):
        dc = dev_critic(lib, critic, LR.State(critic.params.size), 'huber', B)
        da = dev_actor(lib, actor, critic, LR.State(actor.params.size), B)
        got = critic_call(lib, 's2d_learn_critic_grad', dc, 1, obs, action, target, weight)
        want_c = AC.critic_grad(L, critic, 'huber', obs, action, target, weight)
        check_critic(dc, got, want_c, f'{what}: critic')
        got = actor_call(lib, 's2d_learn_actor_grad', da, dc, obs)
        want_a = AC.actor_grad(L, actor, critic, obs)
        check_actor(da, got, want_a, f'{what}: actor')
        return want_c, want_a
    o = obs.copy()
    o[70, 3] = np.nan
    o[5] = np.inf
    want_c, want_a = run(actor, critic, o, weight, 'NaN and inf rows')
    # the spec's relu (v > 0 ? v : +0) sends a NaN pre-activation to +0, so the values stay finite; the first layer's gradients do not
    assert np.isnan(want_c['stats'][1]) and np.isnan(want_a['stats'][1]) and np.isnan(want_c['grad']).any() and np.isnan(want_a['grad']).any()
    # a saturated head: the output bias of the actor at +40 in every row
    sat = TD.Net(actor.n_in, actor.hidden, 1, actor.act, actor.params.copy())
    sat.params[-1] = 40.0
    _, want_a = run(sat, critic, obs, weight, 'saturated action')
    assert (want_a['action'] == 1.0).all() and (TD.bits(want_a['grad']) == 0).all() and want_a['stats'][1] == 0
    # a dead-ReLU critic: every first-layer bias at -100
    dead = TD.Net(critic.n_in, critic.hidden, 1, critic.act, critic.params.copy())
    dead.params[64 * 11:64 * 11 + 64] = -100.0
    want_c, want_a = run(actor, dead, obs, weight, 'dead critic')
    assert (TD.bits(want_a['grad']) == 0).all() and (want_a['q'] == want_a['q'][0]).all() and (want_c['grad'][:64 * 11] == 0).all()
    # zero weights: one row, then all
    w = weight.copy()
    w[R] = 0.0
    run(actor, critic, obs, w, 'one zero weight')
    want_c, _ = run(actor, critic, obs, np.zeros(B, F), 'weights all zero')
    assert (want_c['grad'] == 0).all() and want_c['stats'][0] == 0 and (want_c['td_abs'] > 0).any()


def seq(n_in, hidden, n_out, act='relu', head=False):
    layers, win = [], n_in
    for w in hidden:
        layers += [nn.Linear(win, w), ACT_NN[act]()]
        win = w
    return nn.Sequential(*layers, nn.Linear(win, n_out), *([nn.Tanh()] if head else [])).to(DEV)


def net_of(module, act):
    lin = [m for m in module if isinstance(m, nn.Linear)]
    p = np.concatenate([np.concatenate([l.weight.detach().cpu().numpy().ravel(), l.bias.detach().cpu().numpy().ravel()]) for l in lin])
    return TD.Net(lin[0].in_features, [l.out_features for l in lin[:-1]], lin[-1].out_features, act, p)


@pytest.mark.parametrize('shape', [AC.SHAPES[1], AC.SHAPES[2], AC.SHAPES[4]], ids=AC.shape_id)
def test_forward_is_the_target_kernels(shape):
    """out_action and out_q of s2d_learn_actor_grad have the bits s2d_td_target_ac (ActorCriticTarget) writes for the same
    parameters with next_obs = obs"""
    from soccer2d_amd.learn import ActorCriticLearner
    from soccer2d_amd.td import ActorCriticTarget
    D, A, ha, hc, act = shape
    torch.manual_seed(D)
    mu, q = seq(D, ha, A, act, head=True), seq(D + A, hc, 1, act)
    lrn = ActorCriticLearner.from_modules(mu, q, max_batch=200)
    B = 2 * R + 5
    x = torch.randn(B, D, device=DEV)
    batch = {'obs': x, 'next_obs': x, 'reward': torch.zeros(B, device=DEV), 'discount': torch.ones(B, device=DEV)}
    _, q_t, a_t = ActorCriticTarget.from_modules(mu, q).target(batch, return_q=True)
    out_a, out_q = torch.full((B, A), S_F, device=DEV), torch.full((B,), S_F, device=DEV)
    lrn.grad_actor(batch, action_out=out_a, q_out=out_q)
    torch.cuda.synchronize()
    assert torch.equal(out_a.view(torch.int32), a_t.view(torch.int32)) and torch.equal(out_q.view(torch.int32), q_t.view(torch.int32))


def dev_rec(rec):
    return {k: torch.from_numpy(v).to(DEV) for k, v in rec.items() if v is not None}


def test_five_updates_eagerly_and_from_one_captured_graph(L, T):
    """sample -> ActorCriticTarget.target -> step_critic -> step_actor -> update_targets(tau = 1) five times eagerly == five replays
    of one captured graph of the five == the restatement on the batches the graph drew, bit for bit (TD3: two critics); set_lr
    between replays takes effect"""
    from soccer2d_amd.learn import ActorCriticLearner
    from soccer2d_amd.replay import DeviceReplay
    from soccer2d_amd.td import ActorCriticTarget
    torch.manual_seed(6)
    rng = np.random.default_rng(6)
    B, D, A = 2 * R + 5, 10, 2
    rec, first = RR.synthetic_record(rng, 4, 60, D, A, float_action=True)
    mods0 = (seq(D, (64, 64), A, head=True), seq(D + A, (64, 64), 1), seq(D + A, (32, 16), 1, 'tanh'))

    def make():
        mods = (seq(D, (64, 64), A, head=True), seq(D + A, (64, 64), 1), seq(D + A, (32, 16), 1, 'tanh'))
        tmods = (seq(D, (64, 64), A, head=True), seq(D + A, (64, 64), 1), seq(D + A, (32, 16), 1, 'tanh'))
        for m, t, m0 in zip(mods, tmods, mods0):
            m.load_state_dict(m0.state_dict()), t.load_state_dict(m0.state_dict())
        rb = DeviceReplay(512, D, action_words=A, action_dtype=torch.float32, device=DEV, seed=9)
        rb.push(dev_rec(rec), torch.from_numpy(first).to(DEV))
        lrn = ActorCriticLearner.from_modules(*mods, actor_lr=1e-2, critic_lr=1e-2, max_grad_norm=0.5, max_batch=B)
        return dict(mods=mods, tmods=tmods, rb=rb, lrn=lrn, td=ActorCriticTarget.from_modules(*tmods), batch=rb.alloc_batch(B),
                    tgt=torch.empty(B, device=DEV), abs=torch.empty(B, device=DEV))

    def update(s):
        s['rb'].sample(B, out=s['batch'])
        s['td'].target(s['batch'], out=s['tgt'])
        s['lrn'].step_critic(s['batch'], s['tgt'], td_abs_out=s['abs'])
        s['lrn'].step_actor(s['batch'])
        s['lrn'].update_targets(s['td'], tau=1.0)
    lrs = [(1e-2, 1e-2), (1e-2, 3e-3), (3e-3, 3e-3), (3e-3, 1e-3), (1e-3, 1e-3)]
    e = make()
    for la, lc in lrs:
        e['lrn'].set_lr(actor=la, critic=lc)
        update(e)
    g = make()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                            # a warm-up outside the capture, on objects of its own
        update(make())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g['lrn'].update_targets(g['td'], tau=1.0)                                # the mirrors exist before the capture; a copy of equals
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        update(g)
    torch.cuda.synchronize()
    same(g['lrn'].actor.params, net_of(mods0[0], 'relu').params, 'capturing ran nothing')
    nets = [net_of(mods0[0], 'relu'), net_of(mods0[1], 'relu'), net_of(mods0[2], 'tanh')]
    tnets = [TD.Net(n.n_in, n.hidden, n.n_out, n.act, n.params.copy()) for n in nets]
    states = [LR.State(n.params.size, lr=1e-2, max_grad_norm=0.5) for n in nets]
    lrn = g['lrn']
    for n, (la, lc) in enumerate(lrs):
        lrn.set_lr(actor=la, critic=lc)
        graph.replay()
        torch.cuda.synchronize()
        h = {k: v.cpu().numpy() for k, v in g['batch'].items()}
        target = TD.target_ac(T, tnets[0], tnets[1], tnets[2], h['next_obs'], h['reward'], h['discount'])[0]
        same(g['tgt'], target, f'replay {n}: target')
        states[0].hyper[0], states[1].hyper[0], states[2].hyper[0] = F(la), F(lc), F(lc)
        want1 = AC.critic_step(L, nets[1], states[1], 'square', h['obs'], h['action'], target)
        want2 = AC.critic_step(L, nets[2], states[2], 'square', h['obs'], h['action'], target)
        want_a = AC.actor_step(L, nets[0], nets[1], states[0], h['obs'])
        same(g['abs'], want1['td_abs'], f'replay {n}: td_abs')
        for dev_net, net, st, want, name in zip((lrn.actor,) + lrn.critics, nets, states, (want_a, want1, want2), ('actor', 'critic 1', 'critic 2')):
            same(dev_net.grad, want['grad'], f'replay {n}: {name} grad')
            same(dev_net.stats, want['stats'], f'replay {n}: {name} stats')
            same(dev_net.params, net.params, f'replay {n}: {name} params')
            same(dev_net.m, st.m, f'replay {n}: {name} m'), same(dev_net.v, st.v, f'replay {n}: {name} v')
            same(dev_net.hyper, st.hyper, f'replay {n}: {name} hyper')
        assert (lrn.critic_loss, lrn.critic_grad_norm, lrn.critic_clip_scale) == tuple(float(x) for x in want1['stats'])
        assert (lrn.actor_loss, lrn.actor_grad_norm, lrn.actor_clip_scale) == tuple(float(x) for x in want_a['stats'])
        for t, net in zip(tnets, nets):                                      # update_targets(tau = 1)
            t.params[:] = net.params
        for t_dev, t in zip((g['td'].mu_target,) + g['td'].critics, tnets):
            same(t_dev.params, t.params, f'replay {n}: target params')
    for a, b in zip((e['lrn'].actor,) + e['lrn'].critics, (lrn.actor,) + lrn.critics):
        for name in ('params', 'm', 'v', 'hyper', 'grad', 'stats'):
            assert torch.equal(getattr(a, name).view(torch.int32), getattr(b, name).view(torch.int32)), f'eager against graph: {a.what} {name}'
    assert torch.equal(e['abs'].view(torch.int32), g['abs'].view(torch.int32))
    for me, mg in zip(e['mods'] + e['tmods'], g['mods'] + g['tmods']):       # the modules, targets included, hold the learners' weights
        for p_e, p_g in zip(me.parameters(), mg.parameters()):
            assert torch.equal(p_e, p_g)
    assert not torch.equal(lrn.actor.params, to_dev(net_of(mods0[0], 'relu').params))


def test_views_actor_sync_and_update_targets():
    from soccer2d_amd.learn import ActorCriticLearner
    from soccer2d_amd.td import ActorCriticTarget
    from soccer2d_amd.wide_actor import WideDeterministicActor
    torch.manual_seed(8)
    mk = lambda: (seq(10, (64, 64), 1, head=True), seq(11, (64, 64), 1), seq(11, (64, 32), 1))
    mods, tmods = mk(), mk()
    lrn = ActorCriticLearner.from_modules(*mods, actor_lr=1e-2, critic_lr=1e-2, max_batch=256)
    for net, mod in zip((lrn.actor,) + lrn.critics, mods):
        lo, hi = net.params.data_ptr(), net.params.data_ptr() + 4 * net.params.numel()
        assert all(lo <= p.data_ptr() < hi for p in mod.parameters()) and all(p.device == lrn.device for p in mod.parameters())
    fused = WideDeterministicActor.from_module(mods[0])
    td = ActorCriticTarget.from_modules(*tmods)
    B = 200
    batch = {'obs': torch.randn(B, 10, device=DEV), 'action': torch.rand(B, 1, device=DEV) * 2 - 1}
    before = [n.params.clone() for n in (lrn.actor,) + lrn.critics]
    lrn.step(batch, torch.randn(B, device=DEV), weight=torch.rand(B, device=DEV))
    assert all(not torch.equal(n.params, b) for n, b in zip((lrn.actor,) + lrn.critics, before))
    assert lrn.critic_loss > 0 and lrn.critic_grad_norm > 0 and lrn.critic_clip_scale == 1 and lrn.actor_grad_norm > 0
    held = lrn.actor.params.clone()
    lrn.step(batch, torch.randn(B, device=DEV), actor=False)                 # TD3's delayed policy update: the actor waits
    assert torch.equal(lrn.actor.params, held)
    for net, mod in zip((lrn.actor,) + lrn.critics, mods):
        assert torch.equal(torch.cat([p.detach().reshape(-1) for p in mod.parameters()]), net.params)    # the module IS the flat buffer
    fused.sync()
    assert torch.equal(fused.params, WideDeterministicActor.from_module(mods[0]).params)
    assert set(mods[0].state_dict()) == {'0.weight', '0.bias', '2.weight', '2.bias', '4.weight', '4.bias'}
    g1, g2 = lrn.grad_critic(batch, torch.randn(B, device=DEV))
    assert g1.numel() == lrn.critics[0].params.numel() and g2.numel() == lrn.critics[1].params.numel() and lrn.grad_actor(batch) is lrn.actor.grad
    # update_targets: lerp_ / copy_ on the flat buffers, bit for bit, and the target modules follow
    nets, tnets = (lrn.actor,) + lrn.critics, (td.mu_target,) + td.critics
    old = [t.params.clone() for t in tnets]
    lrn.update_targets(td, tau=0.005)
    for n, t, o, m in zip(nets, tnets, old, tmods):
        assert torch.equal(t.params, o.lerp(n.params, 0.005)) and not torch.equal(t.params, o)
        assert torch.equal(torch.cat([p.detach().reshape(-1) for p in m.parameters()]), t.params)
    td.sync()
    assert all(torch.equal(t.params, o.lerp(n.params, 0.005)) for n, t, o in zip(nets, tnets, old))
    lrn.update_targets(td)
    assert all(torch.equal(t.params, n.params) for n, t in zip(nets, tnets))
    lrn.reset_optimizer(), lrn.set_lr(actor=0.25)
    assert lrn.actor.hyper.tolist() == [0.25, float(F(0.9)), float(F(0.999)), float(F(1e-8)), 0.0, 1.0, 1.0] and not lrn.actor.m.any()


def copy_of(s, **changes):
    c = type(s)()
    C.memmove(C.byref(c), C.byref(s), C.sizeof(s))
    for k, v in changes.items():
        setattr(c, k, v)
    return c


def hidden(*ws):
    return (C.c_int32 * 5)(*ws)


def test_rejections_return_einval_with_text_and_launch_nothing(L, lib):
    from soccer2d_amd import _capi
    from soccer2d_amd.learn import ActorCriticLearner
    rs = np.random.RandomState(9)
    D, A, B = 10, 2, 70
    actor, critic = AC.random_pair(rs, D, A, (16, 8), (16, 8), 'relu')
    obs, action, target, weight = AC.random_batch(rs, critic, A, B)
    dc = dev_critic(lib, critic, LR.State(critic.params.size), 'square', B)
    da = dev_actor(lib, actor, critic, LR.State(actor.params.size), B)
    o, a, t, w = to_dev(obs), to_dev(action), to_dev(target), to_dev(weight)
    out = guarded(B * A)
    watched = dc.arrays() + da.arrays() + (out,)
    snap = [x.clone() for x in watched]

    def refused(rc, text):
        torch.cuda.synchronize()
        assert rc == _capi.S2D_EINVAL and text in lib.s2d_last_error().decode(), (text, rc, lib.s2d_last_error())
        for x, y in zip(watched, snap):
            assert torch.equal(x, y), f'{text}: something was written'

    def critic_(fn='s2d_learn_critic', batch=B, net_=None, st_=None, o_=o.data_ptr(), A_=A, a_=a.data_ptr(), t_=t.data_ptr(), w_=w.data_ptr(),
               abs_=out.data_ptr(), q_=None):
        return getattr(lib, fn)(batch, C.byref(net_ or dc.s), C.byref(st_ or dc.st), o_, A_, a_, t_, w_, abs_, q_, None)

    def actor_(fn='s2d_learn_actor', batch=B, net_=None, st_=None, c_=None, o_=o.data_ptr(), act_=out.data_ptr(), q_=None):
        return getattr(lib, fn)(batch, C.byref(net_ or da.s), C.byref(st_ or da.st), C.byref(c_ or dc.s), o_, act_, q_, None)
    shapes = ((dict(n_in=0), 'n_in'), (dict(n_in=257), 'n_in'), (dict(n_hidden=0), 'n_hidden'), (dict(n_hidden=5), 'n_hidden'),
              (dict(hidden=hidden(16, 12)), 'hidden widths'), (dict(hidden=hidden(264, 8)), 'hidden widths'), (dict(hidden=hidden(16, 8, 8)), 'hidden widths'),
              (dict(activation=3), 'activation'))
    for fn in ('s2d_learn_critic', 's2d_learn_critic_grad'):
        for changes, text in shapes + ((dict(n_out=0), 'n_out'), (dict(n_out=2), 'n_out'), (dict(n_in=2), 'obs_dim'), (dict(params=None), 'params'),
                                       (dict(params=dc.params.data_ptr() + 4), 'params'), (dict(workspace=None), 'workspace'),
                                       (dict(workspace=dc.ws.data_ptr() + 16), 'workspace'), (dict(workspace_bytes=dc.words * 4 - 4), 'workspace_bytes'),
                                       (dict(workspace=dc.params.data_ptr()), 'overlap'), (dict(params=dc.grad.data_ptr()), 'overlap')):
            refused(critic_(fn, net_=copy_of(dc.s, **changes)), text)
        for changes, text in ((dict(loss_kind=3), 'loss_kind'), (dict(loss_kind=-1), 'loss_kind'), (dict(grad=None), 'grad'),
                              (dict(grad=dc.grad.data_ptr() + 4), 'grad'), (dict(hyper=None), 'hyper'), (dict(stats=dc.stats.data_ptr() + 2), 'stats'),
                              (dict(error=None), 'error'), (dict(grad=dc.ws.data_ptr() + 256), 'overlap')):
            refused(critic_(fn, st_=copy_of(dc.st, **changes)), text)
        for kw, text in ((dict(batch=0), 'batch'), (dict(batch=2 ** 31), 'batch'), (dict(batch=B + 64), 'max_batch'), (dict(A_=0), 'action_dim'),
                         (dict(A_=9), 'action_dim'), (dict(o_=None), 'obs'), (dict(a_=a.data_ptr() + 2), 'action'), (dict(a_=None), 'action'),
                         (dict(t_=None), 'target'), (dict(w_=w.data_ptr() + 1), 'weight'), (dict(abs_=out.data_ptr() + 3), 'out_td_abs'),
                         (dict(q_=out.data_ptr() + 2), 'out_q')):
            refused(critic_(fn, **kw), text)
    for changes, text in ((dict(m=None), 'm and v'), (dict(v=dc.v.data_ptr() + 8), 'm and v'), (dict(m=dc.v.data_ptr()), 'overlap')):
        refused(critic_('s2d_learn_critic', st_=copy_of(dc.st, **changes)), text)
    # the Q-learner's entry points keep rejecting the square loss
    ai = torch.zeros(B, dtype=torch.int32, device=DEV)
    for fn in ('s2d_learn_q', 's2d_learn_q_grad'):
        refused(getattr(lib, fn)(B, C.byref(copy_of(dc.s)), C.byref(copy_of(dc.st, loss_kind=2)), o.data_ptr(), ai.data_ptr(), t.data_ptr(), None,
                                 None, None, None), 'loss_kind')
    for fn in ('s2d_learn_actor', 's2d_learn_actor_grad'):
        for changes, text in shapes + ((dict(n_out=0), 'n_out'), (dict(n_out=9), 'n_out'), (dict(n_out=1), "actor's n_in + n_out"), (dict(n_in=249), 'n_in'),
                                       (dict(params=None), 'actor: params'), (dict(params=da.params.data_ptr() + 4), 'actor: params'),
                                       (dict(workspace=None), 'workspace'), (dict(workspace=da.ws.data_ptr() + 16), 'workspace'),
                                       (dict(workspace_bytes=da.words * 4 - 4), 'workspace_bytes'), (dict(workspace=da.params.data_ptr()), 'overlap'),
                                       (dict(params=dc.params.data_ptr()), 'overlap'), (dict(workspace=dc.params.data_ptr()), 'overlap')):
            refused(actor_(fn, net_=copy_of(da.s, **changes)), 'actor: ' + text if text in ('n_in', 'n_hidden', 'hidden widths', 'activation') else text)
        for changes, text in shapes[2:] + ((dict(n_in=D + A + 1), "actor's n_in + n_out"), (dict(n_out=2), "actor's n_in + n_out"),
                                           (dict(params=None), 'critic: params'), (dict(params=dc.params.data_ptr() + 8), 'critic: params')):
            refused(actor_(fn, c_=copy_of(dc.s, **changes)), 'critic: ' + text if text in ('n_hidden', 'hidden widths', 'activation') else text)
        for changes, text in ((dict(grad=None), 'grad'), (dict(hyper=None), 'hyper'), (dict(stats=da.stats.data_ptr() + 2), 'stats'),
                              (dict(grad=dc.params.data_ptr()), 'overlap'), (dict(grad=da.ws.data_ptr() + 256), 'overlap')):
            refused(actor_(fn, st_=copy_of(da.st, **changes)), text)
        for kw, text in ((dict(batch=0), 'batch'), (dict(batch=2 ** 31), 'batch'), (dict(batch=B + 64), 'max_batch'), (dict(o_=None), 'obs'),
                         (dict(act_=out.data_ptr() + 2), 'out_action'), (dict(q_=out.data_ptr() + 1), 'out_q')):
            refused(actor_(fn, **kw), text)
    for changes, text in ((dict(m=None), 'm and v'), (dict(v=dc.params.data_ptr()), 'overlap')):
        refused(actor_('s2d_learn_actor', st_=copy_of(da.st, **changes)), text)
    assert lib.s2d_learn_actor(B, C.byref(da.s), C.byref(da.st), None, o.data_ptr(), None, None, None) == _capi.S2D_EINVAL
    assert lib.s2d_learn_critic(B, None, C.byref(dc.st), o.data_ptr(), A, a.data_ptr(), t.data_ptr(), None, None, None, None) == _capi.S2D_EINVAL
    # the _grad twins do not read m and v; the actor's calls neither need nor write the error word; optional outputs may be NULL
    assert critic_('s2d_learn_critic_grad', st_=copy_of(dc.st, m=None, v=None), abs_=None) == _capi.S2D_OK
    assert actor_('s2d_learn_actor_grad', st_=copy_of(da.st, m=None, v=None, error=None), act_=None) == _capi.S2D_OK
    torch.cuda.synchronize()
    same(dc.grad[:dc.P], AC.critic_grad(L, dc.net, 'square', obs, action, target, weight)['grad'], 'critic grad without m and v')
    same(da.grad[:da.P], AC.actor_grad(L, da.net, dc.net, obs)['grad'], 'actor grad without m, v and error')
    dc.check_guards(), da.check_guards()
    assert torch.equal(out, snap[-1])
    # through the class: a ValueError, and the parameters stay
    lrn = ActorCriticLearner.from_modules(seq(D, (16, 8), A, head=True), seq(D + A, (16, 8), 1), max_batch=64)
    before = [n.params.clone() for n in (lrn.actor,) + lrn.critics]
    batch = {'obs': o[:64], 'action': a[:64]}
    for b_, t_, kw, text in ((dict(batch, obs=o[:64].cpu()), t[:64], {}, r"batch\['obs'\]"), (batch, t[:63], {}, 'target'),
                             (dict(batch, action=a[:64].long()), t[:64], {}, r"batch\['action'\]"), (batch, t[:64], dict(weight=w[:64].double()), 'weight'),
                             ({'obs': o, 'action': a}, t, {}, 'max_batch=64'), (batch, t[:64], dict(td_abs_out=out[:128][::2]), 'td_abs_out')):
        with pytest.raises(ValueError, match=text):
            lrn.step(b_, t_, **kw)
    with pytest.raises(ValueError, match='action_out'):
        lrn.step_actor(batch, action_out=out[:64])
    torch.cuda.synchronize()
    assert all(torch.equal(n.params, b) for n, b in zip((lrn.actor,) + lrn.critics, before))


EXAMPLES = [('ddpg_reach_ball.py', ['--fused-learner', '--fused-target'], 'goal share'),
            ('ddpg_reach_ball.py', ['--fused-learner', '--per-alpha', '0.6', '--n-step', '3', '--turning'], 'goal share'),
            ('go_to_center.py', ['--continuous', '--turn', '--useturn', '--fused-learner', '--fused-target'], 'iter 0'),
            ('ddpg_reach_ball.py', ['--fused-learner', '--net-arch', '400,300'], 'multiple of 8 in [8, 256]')]


@pytest.mark.parametrize('script, flags, text', EXAMPLES, ids=['fused_target', 'per_nstep_turning', 'go_to_center', 'off_grid'])
def test_examples_run_with_the_fused_learner(tmp_path, script, flags, text):
    """--fused-learner in the examples: with --fused-target, with PER weights and n-step returns, on GoToCenter's DDPG arm; an actor
    off the learner's grid ends the run with an error naming the grid"""
    import os
    import subprocess
    import sys
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gym-soccer-2d-env_amd', 'examples', script)
    r = subprocess.run([sys.executable, ex, '--envs', '512', '--iters', '1', '--train-steps', '64', '--test-steps', '20', '--fused-actor', '32'] + flags,
                       cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    off_grid = '400,300' in flags
    assert (r.returncode != 0) == off_grid, r.stdout[-3000:]
    assert text in r.stdout, r.stdout[-3000:]
