"""The fused Soft Actor-Critic update (s2d_learn_sac_actor / s2d_learn_sac_actor_grad, with s2d_learn_critic for the critics;
soccer2d_amd.learn.SACLearner) on the GPU, every comparison bit for bit against the host restatement tests/learn_sac_ref.c: the
actor's flat gradient and three stats, the temperature's stats, out_action / out_logp / out_q, and after a step the parameters, m,
v, both sets of beta products, log_alpha, alpha and draws -- at every shape and batch edge, with and without a clip, a learned and a
fixed temperature, one and two critics, on the data edges, against the critics' own forward, eagerly and from one captured graph of
sample -> SacTarget.target -> step_critic -> step_actor -> update_targets, through the class and the example, and every rejection,
which launches nothing.  Every output, state array and workspace has sentinel guard words past its end, and the guards are checked."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import learn as LR
import learn_ac as AC
import learn_sac as LS
import replay as RR
import sac_ref as SR
import td as TD
from test_gpu_learn_ac import (DevNet, c_shape, check_outputs, copy_of, critic_call, dev_critic, dev_rec, guarded, hidden, net_of, outputs, same,
                               seq, to_dev)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

F = np.float32
DEV = 'cuda:0'
PAD = 64
S_F = -7777.0
R = LS.BLOCK_ROWS
SEED = 0x1234567890ABCDEF
DRAWS0 = 2 ** 32 + 5                       # both halves of the counter's middle words are in use
CASES = [(s, 133) for s in LS.SHAPES] + [(LS.REACH_BALL, B) for B in (1, 63, 64, 65, 4096)]


@pytest.fixture(scope='module')
def L(tmp_path_factory):
    return LS.build(tmp_path_factory.mktemp('learn_sac_ref'))


@pytest.fixture(scope='module')
def S(tmp_path_factory):
    return SR.build(tmp_path_factory.mktemp('sac_ref'))


@pytest.fixture(scope='module')
def lib():
    from soccer2d_amd import _capi
    return _capi.load_library()


class DevSac:
    """the three networks and the temperature on the device behind the raw C ABI, every array with guard words behind it, the actor's
    workspace of exactly s2d_learn_sac_workspace_bytes; the host copies (nets, states, alpha, draws, AlphaState) beside them"""

    def __init__(self, lib, actor, c1, c2, max_batch, max_grad_norm=0.0, alpha=0.6, learned=True, lr=1e-2, target_entropy=None):
        from soccer2d_amd import _capi
        A = actor.n_out // 2
        self.actor, self.c1, self.c2, self.A = actor, c1, c2, A
        self.sa = LR.State(actor.params.size, lr=lr, max_grad_norm=max_grad_norm)
        self.sc = [LR.State(c.params.size, lr=lr, max_grad_norm=max_grad_norm) for c in (c1, c2) if c is not None]
        words = lib.s2d_learn_sac_workspace_bytes(C.byref(c_shape(actor)), C.byref(c_shape(c1)), C.byref(c_shape(c2)) if c2 is not None else None,
                                                  max_batch) // 4
        assert words > 0
        self.da = DevNet(actor, self.sa, 'mse', words)
        self.dc = [dev_critic(lib, c, s, 'mse', max_batch) for c, s in zip((c1, c2), self.sc)]
        self.alpha_h, self.draws_h = np.array([alpha], F), np.array([DRAWS0], np.uint64)
        self.ast = LS.AlphaState(-A if target_entropy is None else target_entropy, log_alpha=float(np.log(alpha)) if alpha > 0 else 0.0,
                                 lr=lr) if learned else None
        self.alpha, self.log_alpha, self.m_v, self.ahyper, self.astats = guarded(1), guarded(1), guarded(2), guarded(7), guarded(3)
        self.alpha[:1] = to_dev(self.alpha_h)
        self.draws = torch.full((1 + PAD,), -77, dtype=torch.int64, device=DEV)
        self.draws[0] = DRAWS0
        self.t = None
        if learned:
            self.log_alpha[:1], self.ahyper[:7] = to_dev(self.ast.log_alpha), to_dev(self.ast.hyper)
            self.m_v[:2] = 0.0
            t = _capi.S2DLearnSacAlpha()
            t.log_alpha, t.m_v, t.hyper, t.stats = (x.data_ptr() for x in (self.log_alpha, self.m_v, self.ahyper, self.astats))
            t.target_entropy = self.ast.target_entropy
            self.t = t

    def temperature(self):
        return (self.alpha, self.log_alpha, self.m_v, self.ahyper, self.astats, self.draws)

    def check_guards(self):
        self.da.check_guards()
        for d in self.dc:
            d.check_guards()
        for x, n in zip(self.temperature()[:5], (1, 1, 2, 7, 3)):
            assert bool((x[n:] == S_F).all()), 'wrote past a temperature array'
        assert bool((self.draws[1:] == -77).all()), 'wrote past draws'

    def call(self, lib, fn, obs, t='own', outs=True):
        """one s2d_learn_sac_actor / _grad; returns (action [B][A], logp [B], q [B]); every guard checked"""
        from soccer2d_amd import _capi
        B, A = obs.shape[0], self.A
        o = to_dev(np.ascontiguousarray(obs, F))
        act, lp, q = outputs(B * A, B, B)
        t = self.t if t == 'own' else t
        torch.cuda.synchronize()
        rc = getattr(lib, fn)(B, C.byref(self.da.s), C.byref(self.da.st), C.byref(self.dc[0].s), C.byref(self.dc[1].s) if len(self.dc) > 1 else None,
                              o.data_ptr(), self.alpha.data_ptr(), C.byref(t) if t is not None else None, self.draws.data_ptr(), SEED,
                              act.data_ptr() if outs else None, lp.data_ptr() if outs else None, q.data_ptr() if outs else None, None)
        torch.cuda.synchronize()
        _capi.check(lib, rc, fn)
        self.check_guards()
        check_outputs((act, lp, q), (B * A, B, B))
        return act[:B * A].view(B, A), lp[:B], q[:B]

    def check(self, got, want, what):
        same(self.da.grad[:self.da.P], want['grad'], f'{what}: grad')
        same(self.da.stats[:3], want['stats'], f'{what}: stats (loss, norm, scale)')
        same(got[0], want['action'], f'{what}: out_action')
        same(got[1], want['logp'], f'{what}: out_logp')
        same(got[2], want['q'], f'{what}: out_q')

    def check_temperature(self, what):
        """the device's temperature, alpha and draws against the host copies"""
        same(self.alpha[:1], self.alpha_h, f'{what}: alpha')
        assert int(self.draws[0]) == int(self.draws_h[0]), f'{what}: draws {int(self.draws[0])} != {int(self.draws_h[0])}'
        if self.ast is not None:
            same(self.log_alpha[:1], self.ast.log_alpha, f'{what}: log_alpha')
            same(self.m_v[:2], self.ast.m_v, f'{what}: the temperature\'s m, v')
            same(self.ahyper[:7], self.ast.hyper, f'{what}: the temperature\'s hyper (beta products)')

    def snapshot(self, critics_only=False):
        xs = [x for d in self.dc for x in d.arrays()]
        if not critics_only:
            xs += [self.da.params, self.da.m, self.da.v, self.da.hyper] + list(self.temperature())
        return xs, [x.clone() for x in xs]

    @staticmethod
    def unchanged(snap, what, skip=()):
        for n, (x, y) in enumerate(zip(*snap)):
            if n not in skip:
                assert torch.equal(x, y) or torch.equal(x.view(torch.int32), y.view(torch.int32)), f'{what} (array {n})'


def run_sac(L, lib, nets, batches, max_grad_norm=0.0, alpha=0.6, learned=True, lr=1e-2):
    """_grad twice on the first batch (the same noise, nothing else touched), then per batch a step of each critic and one actor step
    through the updated critics, each compared with the restatement; the critics bitwise untouched by the actor's calls"""
    actor, c1, c2 = nets
    Bmax = max(b[0].shape[0] for b in batches)
    d = DevSac(lib, actor, c1, c2, Bmax, max_grad_norm, alpha, learned, lr)
    A = d.A
    obs = batches[0][0]
    snap = d.snapshot()
    want = LS.actor_grad(L, actor, c1, c2, obs, d.alpha_h[0], seed=SEED, draws=DRAWS0, max_grad_norm=max_grad_norm)
    for rep in range(2):
        got = d.call(lib, 's2d_learn_sac_actor_grad', obs)
        d.check(got, want, f'grad call {rep}')
        if learned:
            same(d.astats[:2], LS.alpha_stats(L, want['mean_logp'], d.ast), 'grad: the temperature\'s stats[0..1]')
            assert float(d.astats[2]) == S_F, '_grad wrote alpha_state->stats[2]'
        else:
            assert bool((d.astats == S_F).all())
        # everything but the actor's grad, stats, workspace and the temperature's stats (array 4 of the temperature's six)
        nc = len(d.dc) * 7
        d.unchanged(snap, 'the gradient call touched something', skip=(nc + 4 + 4,))
    want_a = None
    for n, (obs, action, target, weight) in enumerate(batches):
        for dc, c, s, name in zip(d.dc, (c1, c2), d.sc, ('critic 1', 'critic 2')):
            got = critic_call(lib, 's2d_learn_critic', dc, A, obs, action, target, weight)
            wc = LS.critic_step(L, c, s, obs, action, target, weight)
            same(dc.grad[:dc.P], wc['grad'], f'{name} step {n}: grad'), same(dc.stats[:3], wc['stats'], f'{name} step {n}: stats')
            same(got[0], wc['td_abs'], f'{name} step {n}: td_abs'), same(got[1], wc['q'], f'{name} step {n}: q')
            dc.check_state(c, s, f'{name} step {n}')
        snap_c = d.snapshot(critics_only=True)
        got = d.call(lib, 's2d_learn_sac_actor', obs)
        want_a = LS.actor_step(L, actor, c1, c2, d.sa, obs, d.alpha_h, d.ast, d.draws_h, SEED)
        d.check(got, want_a, f'actor step {n}')
        d.da.check_state(actor, d.sa, f'actor step {n}')
        d.check_temperature(f'actor step {n}')
        if learned:
            same(d.astats[:3], d.ast.stats, f'actor step {n}: the temperature\'s stats')
        d.unchanged(snap_c, 'the actor step touched a critic\'s params, m, v, grad, hyper, stats or workspace')
    assert int(d.draws_h[0]) == DRAWS0 + len(batches)
    return d, want_a


def batches_of(rs, nets, B, n=2):
    return [AC.random_batch(rs, nets[1], nets[0].n_out // 2, B) for _ in range(n)]


def test_cases_cover_the_issues_list():
    assert [s[:2] for s in LS.SHAPES] == [(1, 1), (10, 1), (10, 4), (13, 8), (10, 1), (10, 1), (248, 8)]
    assert {B for s, B in CASES if s == LS.REACH_BALL} == {1, 63, 64, 65, 133, 4096}
    assert any(s[4] is None for s in LS.SHAPES) and {a for s in LS.SHAPES for a in s[5]} == {'relu', 'tanh', 'sigmoid'}


def test_both_image_paths_are_exercised(lib):
    """the 64-64 triple's image is in LDS (no image words in the workspace), the 256-256 triple's in the workspace"""
    from soccer2d_amd.learn import learn_param_count
    for s, in_ws in ((LS.SHAPES[1], False), (LS.SHAPES[5], True), (LS.SHAPES[6], True)):
        rs = np.random.RandomState(0)
        a, c1, c2 = LS.random_nets(rs, s)
        got = lib.s2d_learn_sac_workspace_bytes(C.byref(c_shape(a)), C.byref(c_shape(c1)), C.byref(c_shape(c2)), 64) // 4
        P = learn_param_count(s[0], s[2], 2 * s[1])
        base = (P + 63) // 64 * 64 + 64 + 64 + 64
        assert (got > base) == in_ws, (s, got, base)


@pytest.mark.parametrize('shape, B', CASES, ids=lambda v: str(v) if isinstance(v, int) else LS.shape_id(v))
def test_grad_and_step_equal_the_restatement(L, lib, shape, B):
    """a learned temperature and an active clip: the gradient call twice, then two rounds of critic 1 step, critic 2 step and actor
    step (the second on moved parameters, a non-trivial Adam state, a moved alpha and fresh noise)"""
    rs = np.random.RandomState(B + shape[0])
    nets = LS.random_nets(rs, shape)
    _, want = run_sac(L, lib, nets, batches_of(rs, nets, B), max_grad_norm=0.05)
    assert float(want['stats'][2]) < 1.0


@pytest.mark.parametrize('clip', ['active', 'inactive', 'off'])
@pytest.mark.parametrize('learned', [True, False], ids=['learned', 'fixed'])
@pytest.mark.parametrize('twin', [True, False], ids=['two_critics', 'one_critic'])
def test_regimes(L, lib, twin, learned, clip):
    rs = np.random.RandomState(21)
    D, A, ha, h1, h2, acts = LS.SHAPES[2]
    nets = LS.random_nets(rs, (D, A, ha, h1, h2 if twin else None, acts))
    mx = {'active': 1e-3, 'inactive': 1e3, 'off': 0.0}[clip]
    d, want = run_sac(L, lib, nets, batches_of(rs, nets, R + 7), max_grad_norm=mx, learned=learned, alpha=0.3)
    assert 1e-3 < want['stats'][1] < 1e3 and (want['stats'][2] < 1.0) == (clip == 'active')
    if not learned:
        assert float(d.alpha[0]) == float(F(0.3)) and bool((d.astats == S_F).all()) and bool((d.log_alpha == S_F).all())


def _with_head(actor, A, mean_bias=None, v_bias=None):
    """a copy of the actor whose mean (and / or raw log-std) outputs are constants: zero weights, the given biases"""
    p = actor.params.copy()
    h = actor.hidden[-1]
    W = p[-(2 * A * h + 2 * A):-2 * A].reshape(2 * A, h)
    b = p[-2 * A:]
    if mean_bias is not None:
        W[:A], b[:A] = 0.0, np.asarray(mean_bias, F)
    if v_bias is not None:
        W[A:], b[A:] = 0.0, np.asarray(v_bias, F)
    return TD.Net(actor.n_in, actor.hidden, actor.n_out, actor.act, p)


def test_data_edges(L, lib):
    """v exactly at and just outside the clamp's bounds and NaN; a saturated action; equal critics (a tie keeps critic 1); a NaN q2;
    alpha = 0; a NaN and an inf observation row -- the device equals the restatement on each, and the restatement shows the edge"""
    rs = np.random.RandomState(31)
    shape = (10, 4, (64, 64), (64, 32), (32, 16), ('relu', 'relu', 'relu'))
    actor, c1, c2 = LS.random_nets(rs, shape)
    A, B = 4, 2 * R + 5
    batch = AC.random_batch(rs, c1, A, B)
    lo, hi = F(-20.0), F(2.0)

    def run(nets, what, alpha=0.6, obs=None):
        b = batch if obs is None else (obs,) + batch[1:]
        nets = tuple(TD.Net(n.n_in, n.hidden, n.n_out, n.act, n.params.copy()) if n is not None else None for n in nets)   # the steps move them
        return run_sac(L, lib, nets, [b], alpha=alpha)[1]
    want = run((_with_head(actor, A, v_bias=[lo, hi, np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))]), c1, c2), 'v at the bounds')
    db = want['grad'][-2 * A:]
    assert db[A] != 0 and db[A + 1] != 0 and (TD.bits(db[A + 2:]) == 0).all(), 'the clamp passes at both bounds and stops just outside'
    want = run((_with_head(actor, A, v_bias=[np.nan, 0.0, 0.0, 0.0]), c1, c2), 'NaN v')
    assert TD.bits(want['grad'][-2 * A:][A]) == 0 and np.isfinite(want['grad']).all()
    want = run((_with_head(actor, A, mean_bias=[40.0, -40.0, 0.0, 0.0], v_bias=[-20.0] * 4), c1, c2), 'saturated actions')
    assert (want['action'][:, 0] == 1).all() and (want['action'][:, 1] == -1).all()
    assert (TD.bits(want['grad'][-2 * A:][:2]) == 0).all(), 'du = 0 for a saturated action'
    twin = TD.Net(c1.n_in, c1.hidden, 1, c1.act, c1.params.copy())
    want = run((actor, c1, twin), 'q1 == q2')
    same(want['grad'], run((actor, c1, None), 'critic 1 alone')['grad'], 'a tie takes critic 1\'s path')
    nanq = TD.Net(c2.n_in, c2.hidden, 1, c2.act, c2.params.copy())
    nanq.params[-1] = np.nan
    want = run((actor, c1, nanq), 'NaN q2')
    same(want['grad'], run((actor, c1, None), 'critic 1 alone')['grad'], 'a NaN q2 keeps critic 1')
    run((actor, c1, c2), 'alpha = 0', alpha=0.0)
    o = batch[0].copy()
    o[70, 3] = np.nan
    o[5] = np.inf
    want = run((actor, c1, c2), 'NaN and inf rows', obs=o)
    assert np.isnan(want['grad']).any()


def test_forward_equals_the_critics_own_and_alpha_feeds_the_target():
    """out_q of grad_actor on the actions it returns == the smaller of the two critics' q_out (s2d_learn_critic_grad) on [obs | a];
    SacTarget.target takes lrn.alpha"""
    from soccer2d_amd.learn import SACLearner
    from soccer2d_amd.td import SacTarget
    D, A, B = 10, 4, 2 * R + 5
    torch.manual_seed(3)
    mods = (seq(D, (64, 64), 2 * A), seq(D + A, (64, 32), 1), seq(D + A, (32, 16), 1, 'tanh'))
    swapped = tuple(seq(m[0].in_features, [x.out_features for x in m if isinstance(x, torch.nn.Linear)][:-1], m[-1].out_features, act)
                    for m, act in ((mods[0], 'relu'), (mods[2], 'tanh'), (mods[1], 'relu')))
    for m, s in zip((mods[0], mods[2], mods[1]), swapped):
        s.load_state_dict(m.state_dict())
    lrn, swp = SACLearner.from_modules(*mods, max_batch=B, seed=5), SACLearner.from_modules(*swapped, max_batch=B, seed=5)
    x = torch.randn(B, D, device=DEV)
    act, lp, q = torch.full((B, A), S_F, device=DEV), torch.full((B,), S_F, device=DEV), torch.full((B,), S_F, device=DEV)
    lrn.grad_actor({'obs': x}, action_out=act, logp_out=lp, q_out=q)
    q1, q2, tgt = torch.empty(B, device=DEV), torch.empty(B, device=DEV), torch.zeros(B, device=DEV)
    lrn.grad_critic({'obs': x, 'action': act}, tgt, q_out=q1)
    swp.grad_critic({'obs': x, 'action': act}, tgt, q_out=q2)
    torch.cuda.synchronize()
    assert torch.equal(q.view(torch.int32), torch.where(q2 < q1, q2, q1).view(torch.int32)) and bool((q2 < q1).any()) and bool((q1 < q2).any())
    assert float(lrn.entropy) == -float(lrn.alpha_stats[0]) and lrn.ent_coef == 1.0 and int(lrn.draws) == 0
    td = SacTarget.from_modules(mods[0], mods[1], mods[2], seed=7)
    batch = {'next_obs': x, 'reward': torch.zeros(B, device=DEV), 'discount': torch.ones(B, device=DEV)}
    t, qt, at, lpt = td.target(batch, lrn.alpha, return_q=True)
    torch.cuda.synchronize()
    assert torch.equal(t.view(torch.int32), (qt - lrn.alpha * lpt).view(torch.int32))


def test_five_updates_eagerly_and_from_one_captured_graph(L, S):
    """sample -> SacTarget.target -> step_critic -> step_actor -> update_targets(tau = 0.005) five times eagerly == five replays of
    one captured graph == the restatement on the batches the graph drew, bit for bit; set_lr between replays takes effect; both
    draw counters end at 5; the target modules and a fused actor's sync() see the learner's weights"""
    from soccer2d_amd.learn import SACLearner
    from soccer2d_amd.replay import DeviceReplay
    from soccer2d_amd.td import SacTarget
    from soccer2d_amd.wide_actor import SquashedGaussianActor
    torch.manual_seed(6)
    rng = np.random.default_rng(6)
    B, D, A, TAU = 2 * R + 5, 10, 1, 0.005
    rec, first = RR.synthetic_record(rng, 4, 60, D, A, float_action=True)
    mk = lambda: (seq(D, (64, 64), 2 * A), seq(D + A, (64, 64), 1), seq(D + A, (32, 16), 1, 'tanh'))
    mods0 = mk()

    def make():
        mods, tmods = mk(), mk()[1:]
        for m, m0 in zip(mods, mods0):
            m.load_state_dict(m0.state_dict())
        for t, m0 in zip(tmods, mods0[1:]):
            t.load_state_dict(m0.state_dict())
        rb = DeviceReplay(512, D, action_words=A, action_dtype=torch.float32, device=DEV, seed=9)
        rb.push(dev_rec(rec), torch.from_numpy(first).to(DEV))
        lrn = SACLearner.from_modules(*mods, actor_lr=1e-2, critic_lr=1e-2, alpha_lr=1e-2, max_grad_norm=0.5, max_batch=B, seed=13)
        return dict(mods=mods, tmods=tmods, rb=rb, lrn=lrn, td=SacTarget.from_modules(mods[0], *tmods, seed=11), batch=rb.alloc_batch(B),
                    tgt=torch.empty(B, device=DEV), abs=torch.empty(B, device=DEV))

    def update(s):
        s['rb'].sample(B, out=s['batch'])
        s['td'].target(s['batch'], s['lrn'].alpha, out=s['tgt'])
        s['lrn'].step_critic(s['batch'], s['tgt'], td_abs_out=s['abs'])
        s['lrn'].step_actor(s['batch'])
        s['lrn'].update_targets(s['td'], tau=TAU)
    lrs = [(1e-2, 1e-2, 1e-2), (1e-2, 3e-3, 1e-2), (3e-3, 3e-3, 3e-3), (3e-3, 1e-3, 1e-3), (1e-3, 1e-3, 3e-2)]
    e = make()
    for la, lc, lt in lrs:
        e['lrn'].set_lr(actor=la, critic=lc, alpha=lt)
        update(e)
    g = make()
    fused = SquashedGaussianActor.from_module(g['mods'][0], device=DEV)
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
    nets = [net_of(mods0[0], 'relu'), net_of(mods0[1], 'relu'), net_of(mods0[2], 'tanh')]
    same(g['lrn'].actor.params, nets[0].params, 'capturing ran nothing')
    tnets = [TD.Net(n.n_in, n.hidden, n.n_out, n.act, n.params.copy()) for n in nets[1:]]
    states = [LR.State(n.params.size, lr=1e-2, max_grad_norm=0.5) for n in nets]
    ast, alpha_h, draws_h = LS.AlphaState(-A, lr=1e-2), np.ones(1, F), np.zeros(1, np.uint64)
    lrn = g['lrn']
    for n, (la, lc, lt) in enumerate(lrs):
        lrn.set_lr(actor=la, critic=lc, alpha=lt)
        told = [t.params.clone() for t in g['td'].critics]
        graph.replay()
        torch.cuda.synchronize()
        h = {k: v.cpu().numpy() for k, v in g['batch'].items()}
        target = SR.target(S, nets[0], tnets[0], tnets[1], h['next_obs'], h['reward'], h['discount'], alpha_h[0], n, 11)[0]
        same(g['tgt'], target, f'replay {n}: target')
        states[0].hyper[0], states[1].hyper[0], states[2].hyper[0], ast.hyper[0] = F(la), F(lc), F(lc), F(lt)
        want1 = LS.critic_step(L, nets[1], states[1], h['obs'], h['action'], target)
        want2 = LS.critic_step(L, nets[2], states[2], h['obs'], h['action'], target)
        want_a = LS.actor_step(L, nets[0], nets[1], nets[2], states[0], h['obs'], alpha_h, ast, draws_h, 13)
        same(g['abs'], want1['td_abs'], f'replay {n}: td_abs')
        for dev_net, net, st, want, name in zip((lrn.actor,) + lrn.critics, nets, states, (want_a, want1, want2), ('actor', 'critic 1', 'critic 2')):
            same(dev_net.grad, want['grad'], f'replay {n}: {name} grad')
            same(dev_net.stats, want['stats'], f'replay {n}: {name} stats')
            same(dev_net.params, net.params, f'replay {n}: {name} params')
            same(dev_net.m, st.m, f'replay {n}: {name} m'), same(dev_net.v, st.v, f'replay {n}: {name} v')
            same(dev_net.hyper, st.hyper, f'replay {n}: {name} hyper')
        same(lrn.alpha, alpha_h, f'replay {n}: alpha'), same(lrn.log_alpha, ast.log_alpha, f'replay {n}: log_alpha')
        same(lrn.alpha_stats, ast.stats, f'replay {n}: the temperature\'s stats'), same(lrn.alpha_hyper, ast.hyper, f'replay {n}: its hyper')
        assert (lrn.critic_loss, lrn.actor_loss, lrn.entropy, lrn.alpha_loss, lrn.ent_coef) == (
            float(want1['stats'][0]), float(want_a['stats'][0]), -float(ast.stats[0]), float(ast.stats[1]), float(alpha_h[0]))
        # update_targets(tau): torch's lerp_ on the flat buffers, the online actor copied into the target's
        for t_dev, o, c, t in zip(g['td'].critics, told, lrn.critics, tnets):
            assert torch.equal(t_dev.params, o.lerp(c.params, TAU)) and not torch.equal(t_dev.params, o)
            t.params[:] = t_dev.params.cpu().numpy()
        same(g['td'].actor.params, nets[0].params, f'replay {n}: the target\'s online actor')
    assert int(lrn.draws) == 5 and int(g['td'].draws) == 5 and int(e['lrn'].draws) == 5 and int(e['td'].draws) == 5
    for a, b in zip((e['lrn'].actor,) + e['lrn'].critics, (lrn.actor,) + lrn.critics):
        for name in ('params', 'm', 'v', 'hyper', 'grad', 'stats'):
            assert torch.equal(getattr(a, name).view(torch.int32), getattr(b, name).view(torch.int32)), f'eager against graph: {a.what} {name}'
    for name in ('alpha', 'log_alpha', 'alpha_m_v', 'alpha_hyper', 'alpha_stats'):
        assert torch.equal(getattr(e['lrn'], name).view(torch.int32), getattr(lrn, name).view(torch.int32)), f'eager against graph: {name}'
    assert torch.equal(e['abs'].view(torch.int32), g['abs'].view(torch.int32))
    for me, mg in zip(e['mods'] + e['tmods'], g['mods'] + g['tmods']):       # the modules, targets included, hold the learners' weights
        for p_e, p_g in zip(me.parameters(), mg.parameters()):
            assert torch.equal(p_e, p_g)
    for t_dev, m in zip(g['td'].critics, g['tmods']):
        assert torch.equal(torch.cat([p.detach().reshape(-1) for p in m.parameters()]), t_dev.params)
    stale = fused.params.clone()
    fused.sync()                                                             # the rollout's actor, made before the updates, follows the learner
    assert torch.equal(fused.params, SquashedGaussianActor.from_module(g['mods'][0], device=DEV).params) and not torch.equal(fused.params, stale)
    assert not torch.equal(lrn.actor.params, to_dev(net_of(mods0[0], 'relu').params))


def test_rejections_return_einval_with_text_and_launch_nothing(L, lib):
    from soccer2d_amd import _capi
    from soccer2d_amd.learn import SACLearner
    rs = np.random.RandomState(9)
    D, A, B = 10, 2, 70
    shape = (D, A, (16, 8), (16, 8), (8, 8), ('relu',) * 3)
    nets = LS.random_nets(rs, shape)
    obs = AC.random_batch(rs, nets[1], A, B)[0]
    d = DevSac(lib, *nets, B)
    o, out = to_dev(obs), guarded(B * A)
    watched = tuple(d.da.arrays()) + tuple(x for c in d.dc for x in c.arrays()) + d.temperature() + (out,)
    snap = [x.clone() for x in watched]

    def refused(rc, text):
        torch.cuda.synchronize()
        assert rc == _capi.S2D_EINVAL and text in lib.s2d_last_error().decode(), (text, rc, lib.s2d_last_error())
        for x, y in zip(watched, snap):
            assert torch.equal(x, y), f'{text}: something was written'

    def call(fn, batch=B, a_=None, st_=None, c1_=None, c2_='own', o_=o.data_ptr(), alpha_=d.alpha.data_ptr(), t_='own', draws_=d.draws.data_ptr(),
             act_=out.data_ptr(), lp_=None, q_=None):
        c2 = d.dc[1].s if c2_ == 'own' else c2_
        t = d.t if t_ == 'own' else t_
        return getattr(lib, fn)(batch, C.byref(a_ or d.da.s), C.byref(st_ or d.da.st), C.byref(c1_ or d.dc[0].s), C.byref(c2) if c2 is not None else None,
                                o_, alpha_, C.byref(t) if t is not None else None, draws_, SEED, act_, lp_, q_, None)
    shapes = ((dict(n_in=0), 'n_in'), (dict(n_hidden=0), 'n_hidden'), (dict(n_hidden=5), 'n_hidden'), (dict(hidden=hidden(16, 12)), 'hidden widths'),
              (dict(hidden=hidden(264, 8)), 'hidden widths'), (dict(activation=3), 'activation'))
    da, dc1, dc2 = d.da, d.dc[0], d.dc[1]
    for fn in ('s2d_learn_sac_actor', 's2d_learn_sac_actor_grad'):
        for changes, text in shapes + ((dict(n_out=3), 'even and in [2, 16]'), (dict(n_out=0), 'n_out'), (dict(n_out=18), 'even and in [2, 16]'),
                                       (dict(n_out=2), "actor's n_in + n_out / 2"), (dict(n_in=249), 'n_in'), (dict(params=None), 'actor: params'),
                                       (dict(params=da.params.data_ptr() + 4), 'actor: params'), (dict(workspace=None), 'workspace'),
                                       (dict(workspace=da.ws.data_ptr() + 16), 'workspace'), (dict(workspace_bytes=da.words * 4 - 4), 'workspace_bytes'),
                                       (dict(workspace=da.params.data_ptr()), 'overlap'), (dict(params=dc1.params.data_ptr()), 'overlap'),
                                       (dict(params=dc2.params.data_ptr()), 'overlap'), (dict(workspace=dc2.params.data_ptr()), 'overlap')):
            refused(call(fn, a_=copy_of(da.s, **changes)), text)
        for which, dcx in (('c1_', dc1), ('c2_', dc2)):
            name = 'critic1' if which == 'c1_' else 'critic2'
            for changes, text in shapes[1:] + ((dict(n_in=D + A + 1), "actor's n_in + n_out / 2"), (dict(n_out=2), "actor's n_in + n_out / 2"),
                                               (dict(params=None), f'{name}: params'), (dict(params=dcx.params.data_ptr() + 8), f'{name}: params')):
                refused(call(fn, **{which: copy_of(dcx.s, **changes)}), text)
        for changes, text in ((dict(grad=None), 'grad'), (dict(hyper=None), 'hyper'), (dict(stats=da.stats.data_ptr() + 2), 'stats'),
                              (dict(grad=dc1.params.data_ptr()), 'overlap'), (dict(grad=dc2.params.data_ptr()), 'overlap'),
                              (dict(grad=da.ws.data_ptr() + 256), 'overlap')):
            refused(call(fn, st_=copy_of(da.st, **changes)), text)
        for kw, text in ((dict(batch=0), 'batch'), (dict(batch=2 ** 31), 'batch'), (dict(batch=B + 64), 'max_batch'), (dict(o_=None), 'obs'),
                         (dict(alpha_=None), 'alpha'), (dict(alpha_=d.alpha.data_ptr() + 2), 'alpha'), (dict(draws_=None), 'draws'),
                         (dict(draws_=d.draws.data_ptr() + 4), 'draws'), (dict(act_=out.data_ptr() + 2), 'out_action'),
                         (dict(lp_=out.data_ptr() + 1), 'out_logp'), (dict(q_=out.data_ptr() + 3), 'out_q'),
                         # the new arrays against the actor's buffers, a critic's params and the outputs
                         (dict(alpha_=da.params.data_ptr() + 8), 'must not overlap'), (dict(alpha_=da.grad.data_ptr()), 'must not overlap'),
                         (dict(alpha_=da.ws.data_ptr() + 64), 'must not overlap'), (dict(draws_=dc1.params.data_ptr()), 'must not overlap'),
                         (dict(draws_=dc2.params.data_ptr() + 8), 'must not overlap'), (dict(alpha_=out.data_ptr() + 4), 'must not overlap'),
                         (dict(draws_=out.data_ptr() + 8, lp_=out.data_ptr()), 'must not overlap'),
                         (dict(alpha_=d.draws.data_ptr() + 4), 'must not overlap')):
            refused(call(fn, **kw), text)
        for changes, text in ((dict(log_alpha=None), 'alpha_state'), (dict(m_v=None), 'alpha_state'), (dict(hyper=None), 'alpha_state'),
                              (dict(stats=None), 'alpha_state'), (dict(m_v=d.m_v.data_ptr() + 2), 'alpha_state'),
                              (dict(log_alpha=d.alpha.data_ptr()), 'must not overlap'), (dict(stats=d.ahyper.data_ptr() + 8), 'must not overlap'),
                              (dict(hyper=da.params.data_ptr()), 'must not overlap'), (dict(m_v=dc2.params.data_ptr()), 'must not overlap'),
                              (dict(stats=out.data_ptr()), 'must not overlap')):
            refused(call(fn, t_=copy_of(d.t, **changes)), text)
    for changes, text in ((dict(m=None), 'm and v'), (dict(v=dc1.params.data_ptr()), 'overlap'), (dict(v=dc2.params.data_ptr()), 'overlap')):
        refused(call('s2d_learn_sac_actor', st_=copy_of(da.st, **changes)), text)
    refused(call('s2d_learn_sac_actor', alpha_=da.m.data_ptr()), 'must not overlap')
    assert lib.s2d_learn_sac_actor(B, C.byref(da.s), C.byref(da.st), None, None, o.data_ptr(), d.alpha.data_ptr(), None, d.draws.data_ptr(), SEED,
                                   None, None, None, None) == _capi.S2D_EINVAL
    # the _grad twin does not read m and v; the error word is neither needed nor written; critic2, alpha_state and the outputs may be NULL
    assert call('s2d_learn_sac_actor_grad', st_=copy_of(da.st, m=None, v=None, error=None), c2_=None, t_=None, act_=None) == _capi.S2D_OK
    torch.cuda.synchronize()
    same(da.grad[:da.P], LS.actor_grad(L, nets[0], nets[1], None, obs, d.alpha_h[0], seed=SEED, draws=DRAWS0)['grad'], 'grad with the optional parts NULL')
    d.check_guards()
    assert torch.equal(out, snap[-1]) and int(d.draws[0]) == DRAWS0
    # through the class: a ValueError, and the parameters stay
    lrn = SACLearner.from_modules(seq(D, (16, 8), 2 * A), seq(D + A, (16, 8), 1), seq(D + A, (8, 8), 1), max_batch=64)
    before = [n.params.clone() for n in (lrn.actor,) + lrn.critics]
    a = torch.rand(B, A, device=DEV)
    t = torch.zeros(B, device=DEV)
    batch = {'obs': o[:64], 'action': a[:64]}
    for b_, t_, kw, text in ((dict(batch, obs=o[:64].cpu()), t[:64], {}, r"batch\['obs'\]"), (batch, t[:63], {}, 'target'),
                             (dict(batch, action=a[:64].long()), t[:64], {}, r"batch\['action'\]"), (batch, t[:64], dict(weight=t[:64].double()), 'weight'),
                             ({'obs': o, 'action': a}, t, {}, 'max_batch=64'), (batch, t[:64], dict(td_abs_out=out[:128][::2]), 'td_abs_out')):
        with pytest.raises(ValueError, match=text):
            lrn.step(b_, t_, **kw)
    for kw, text in ((dict(action_out=out[:64]), 'action_out'), (dict(logp_out=out[:63]), 'logp_out'), (dict(q_out=out[:64].double()), 'q_out')):
        with pytest.raises(ValueError, match=text):
            lrn.step_actor(batch, **kw)
    torch.cuda.synchronize()
    assert all(torch.equal(n.params, b) for n, b in zip((lrn.actor,) + lrn.critics, before)) and int(lrn.draws) == 0


EXAMPLES = [(['--fused-learner', '--fused-actor', '16', '--fused-target'], 'goal share'),
            (['--fused-learner', '--fused-actor', '16', '--fused-target', '--turning'], 'goal share'),
            (['--fused-learner', '--net-arch', '400,300'], 'multiple of 8 in [8, 256]')]


@pytest.mark.parametrize('flags, text', EXAMPLES, ids=['plain', 'turning', 'off_grid'])
def test_example_runs_with_the_fused_learner(tmp_path, flags, text):
    """examples/sac_reach_ball.py --fused-learner: finite losses and the goal-share line; an actor off the learner's grid ends the
    run with an error naming the grid"""
    import re
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gym-soccer-2d-env_amd', 'examples', 'sac_reach_ball.py')
    r = subprocess.run([sys.executable, ex, '--envs', '256', '--batch', '256', '--iters', '2', '--train-steps', '32', '--test-steps', '10'] + flags,
                       cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    off_grid = '400,300' in flags
    assert (r.returncode != 0) == off_grid, r.stdout[-3000:]
    assert text in r.stdout, r.stdout[-3000:]
    if not off_grid:
        losses = re.findall(r'loss_q (\S+) loss_pi (\S+) loss_alpha (\S+) ent_coef (\S+)', r.stdout)
        assert len(losses) == 2 and all(np.isfinite(float(v)) for row in losses for v in row), r.stdout[-3000:]
