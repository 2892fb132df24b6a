"""TD3's target with target-policy smoothing (s2d_td_target_td3; soccer2d_amd.td.Td3Target) on the GPU, bit for bit against the
host restatement (tests/td3_ref.c): every batch edge at one to eight action dimensions (the second Philox block partial and whole),
4, 10, 16 and 224 inputs, with and without the second critic and the optional outputs; sigma = 0 against s2d_td_target_ac on the
same buffers; the clamps' edges, NaN rows and the NaN rule of the twin minimum; the accounting of the `draws` word in eager calls,
in refused calls and in a captured sample -> target graph with the noise words rewritten between replays; independence of the
plan; the target networks that ActorCriticLearner.update_targets steps; and the rejections, which launch nothing."""
import copy
import ctypes as C

import numpy as np
import pytest

import replay as RR
import td as TD
import td3 as T3
from test_gpu_td import DEV, PAD, S_F, DevNet, _out, _take, batch_of, dev_rec, host, run_ac, same, to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
nn = torch.nn
F = np.float32
SEED = 0x7D3A5EED1234
BIG = (7 << 32) + 5          # a preset of the draws word above 2^32: the counter's high word matters
NAMES = ('target', 'q', 'action')


@pytest.fixture(scope='module')
def L(tmp_path_factory):
    return T3.build(tmp_path_factory.mktemp('td3_ref'))


@pytest.fixture(scope='module')
def lib():
    from soccer2d_amd import _capi
    return _capi.load_library()


def word(v=0):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


def run_td3(lib, actor, c1, c2, x, r, d, sigma, clip, draws, seed=SEED, with_q=True, with_action=True):
    """s2d_td_target_td3 on device copies; `draws`: a device int64 word, advanced by the call.  (target, q, action), None where
    not asked for; guards checked"""
    from soccer2d_amd import _capi
    B, A = x.shape[0], actor.net.n_out
    xt, rt, dt = to_dev(x.astype(F)), to_dev(r.astype(F)), to_dev(d.astype(F))
    noise = torch.tensor([sigma, clip], dtype=torch.float32, device=DEV)
    t, q, a = _out(B), (_out(B) if with_q else None), (_out(B, (A,)) if with_action else None)
    ptr = lambda v: None if v is None else v.data_ptr()
    torch.cuda.synchronize()
    rc = lib.s2d_td_target_td3(B, actor.ref(), c1.ref(), c2.ref() if c2 is not None else None, xt.data_ptr(), rt.data_ptr(), dt.data_ptr(),
                               noise.data_ptr(), draws.data_ptr(), seed, t.data_ptr(), ptr(q), ptr(a), None)
    _capi.check(lib, rc, 's2d_td_target_td3')
    torch.cuda.synchronize()
    for n in (actor, c1, c2):
        if n is not None:
            n.check_guard()
    assert noise.tolist() == [float(F(sigma)), float(F(clip))]
    return _take(t, B, 'target'), (_take(q, B, 'q') if with_q else None), (_take(a, B, 'action') if with_action else None)


def nets_of(rs, D, A, pi, qf, act, twin):
    actor = TD.random_net(rs, D, pi, A, act, gain=2.0)
    c1 = TD.random_net(rs, D + A, qf, 1, act)
    c2 = TD.random_net(rs, D + A, qf, 1, act) if twin else None
    return actor, c1, c2


# (D, A, actor hidden, critic hidden, activation, twin): block 1 not drawn, partial (A = 5) and whole (A = 8)
CASES = [(10, 1, (64, 64), (64, 64), 'relu', True), (10, 4, (20, 12), (16,), 'tanh', False), (16, 5, (16, 8), (12, 20), 'sigmoid', True),
         (224, 8, (64, 64), (64, 64), 'relu', True), (4, 2, (16, 8), (64, 32, 16, 8), 'tanh', True)]


@pytest.mark.parametrize('B', [1, 63, 64, 65, 200])
@pytest.mark.parametrize('D,A,pi,qf,act,twin', CASES, ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_target_equals_the_restatement(L, lib, D, A, pi, qf, act, twin, B):
    rs = np.random.RandomState(D + A + B)
    actor, c1, c2 = nets_of(rs, D, A, pi, qf, act, twin)
    x, r, d = batch_of(rs, B, D)
    draws = word(BIG)
    got = run_td3(lib, DevNet(lib, actor), DevNet(lib, c1), DevNet(lib, c2) if twin else None, x, r, d, 0.2, 0.5, draws)
    want = T3.target(L, actor, c1, c2, x, r, d, 0.2, 0.5, BIG, SEED)
    for g, w, name in zip(got, want, NAMES):
        same(g, w, name)
    assert int(draws[0]) == BIG + 1
    a, m = got[2], want[3]
    assert (np.abs(a) <= 1).all() and (B < 60 or len(np.unique(a)) > B // 2)
    assert B < 60 or not np.array_equal(a, m)                                 # the noise is there
    if B >= 60:                                                               # and the low word alone is another draw
        assert not np.array_equal(a, T3.target(L, actor, c1, c2, x, r, d, 0.2, 0.5, BIG & 0xFFFFFFFF, SEED)[2])


@pytest.mark.parametrize('D,A,pi,qf,act,twin', CASES[:3], ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_sigma_zero_equals_the_unsmoothed_launch(lib, D, A, pi, qf, act, twin):
    """sigma = 0 on the buffers s2d_td_target_ac ran on: target and q bit for bit, the actions equal as numbers (-0 + +0 = +0)"""
    rs = np.random.RandomState(31 * D + A)
    B = 200
    actor, c1, c2 = nets_of(rs, D, A, pi, qf, act, twin)
    x, r, d = batch_of(rs, B, D)
    nets = DevNet(lib, actor), DevNet(lib, c1), (DevNet(lib, c2) if twin else None)
    plain = run_ac(lib, *nets, x, r, d)
    if np.any((plain[2] == 0) & np.signbit(plain[2])):
        pytest.fail('the case has a -0 action: choose another seed')
    for clip in (0.5, 0.0):
        got = run_td3(lib, *nets, x, r, d, 0.0, clip, word(BIG))
        same(got[0], plain[0], 'target')
        same(got[1], plain[1], 'q')
        assert np.array_equal(got[2], plain[2])


def _const_critic(n_in, v):
    p = np.zeros(TD.param_count(n_in, (8,), 1), F)
    p[-1] = v
    return TD.Net(n_in, (8,), 1, 'relu', p)


def test_clamp_edges_nan_rows_and_null_outputs(L, lib):
    rs = np.random.RandomState(4)
    D, A, B = 10, 5, 130
    actor, c1, c2 = nets_of(rs, D, A, (20, 12), (16,), 'tanh', True)           # tanh: a NaN input reaches the output
    actor.params[-A:] += np.array([40.0, -40.0, 0.0, 40.0, -40.0], F)         # tanh_spec saturates: m = +1, -1, inside, +1, -1
    x, r, d = batch_of(rs, B, D)
    x[::5] /= 30                                                              # rows in range: the saturation is the bias's
    nets = DevNet(lib, actor), DevNet(lib, c1), DevNet(lib, c2)
    for sigma, clip in ((1e30, 0.125), (0.7, np.inf), (1e30, np.inf), (0.2, 0.0), (3.0, 0.5)):
        got = run_td3(lib, *nets, x, r, d, sigma, clip, word(3))
        want = T3.target(L, actor, c1, c2, x, r, d, sigma, clip, 3, SEED)
        for g, w, name in zip(got, want, NAMES):
            same(g, w, f'sigma={sigma} clip={clip} {name}')
        a = got[2]
        assert (a[:, 0] == 1).any() and (a[:, 1] == -1).any() and (np.abs(a) <= 1).all()
        if sigma == 1e30 and np.isfinite(clip):                              # the noise clamp binds in every word
            assert np.all((a[:, 0] == 1) | (a[:, 0] == F(1) - F(clip))) and np.all(np.abs(a[:, 2] - want[3][:, 2]) <= F(clip) + 2e-7)
        if sigma == 1e30 and not np.isfinite(clip):
            assert np.all(np.abs(a) == 1)
    # a NaN observation row: its target is NaN, every other row keeps its bits
    clean = run_td3(lib, *nets, x, r, d, 0.2, 0.5, word(3))
    xn = x.copy()
    xn[7, 3], xn[64] = np.nan, np.nan
    got = run_td3(lib, *nets, xn, r, d, 0.2, 0.5, word(3))
    want = T3.target(L, actor, c1, c2, xn, r, d, 0.2, 0.5, 3, SEED)
    for g, w, name in zip(got, want, NAMES):
        same(g, w, f'NaN rows {name}')
    others = np.ones(B, bool)
    others[[7, 64]] = False
    assert np.isnan(got[0][[7, 64]]).all() and np.isnan(got[1][[7, 64]]).all()
    for g, c, name in zip(got, clean, NAMES):
        same(g[others], c[others], f'rows beside the NaN rows: {name}')
    # a NaN in q2 never replaces q1
    da = nets[0]
    for q1, q2, want_q in ((1.5, np.nan, 1.5), (np.nan, 1.0, np.nan), (2.0, 1.0, 1.0), (1.0, 2.0, 1.0)):
        k1, k2 = _const_critic(D + A, q1), _const_critic(D + A, q2)
        got = run_td3(lib, da, DevNet(lib, k1), DevNet(lib, k2), x, r, d, 0.2, 0.5, word())
        for g, w, name in zip(got, T3.target(L, actor, k1, k2, x, r, d, 0.2, 0.5, 0, SEED), NAMES):
            same(g, w, f'q1={q1} q2={q2} {name}')
        same(got[1], np.full(B, want_q, F), f'q1={q1} q2={q2}')
    # the optional outputs
    full = T3.target(L, actor, c1, None, x, r, d, 0.2, 0.5, 0, SEED)
    for wq, wa in ((False, False), (True, False), (False, True)):
        got = run_td3(lib, da, nets[1], None, x, r, d, 0.2, 0.5, word(), with_q=wq, with_action=wa)
        for g, w, name, asked in zip(got, full, NAMES, (True, wq, wa)):
            assert (g is not None) == asked
            if asked:
                same(g, w, f'outputs {wq, wa}: {name}')


def test_draws_accounting(L, lib):
    """every eager call advances the word by exactly one and equals the restatement at the count it found; another seed draws
    other noise; a refused call leaves the word as it is"""
    from soccer2d_amd import _capi
    rs = np.random.RandomState(6)
    actor, c1, c2 = nets_of(rs, 10, 1, (64, 64), (64, 64), 'relu', True)
    x, r, d = batch_of(rs, 130, 10)
    nets = DevNet(lib, actor), DevNet(lib, c1), DevNet(lib, c2)
    draws = word(2 ** 32 - 1)                                                 # the carry into the high word
    seen = []
    for n in range(3):
        got = run_td3(lib, *nets, x, r, d, 0.2, 0.5, draws)
        assert int(draws[0]) == 2 ** 32 + n
        for g, w, name in zip(got, T3.target(L, actor, c1, c2, x, r, d, 0.2, 0.5, 2 ** 32 - 1 + n, SEED), NAMES):
            same(g, w, f'call {n} {name}')
        seen.append(got[2])
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    other = run_td3(lib, *nets, x, r, d, 0.2, 0.5, word(2 ** 32 - 1), seed=SEED + 1)
    assert not np.array_equal(seen[0], other[2])
    t = _out(130)
    xt, rt, dt = to_dev(x), to_dev(r), to_dev(d)
    noise = torch.tensor([0.2, 0.5], device=DEV)
    rc = lib.s2d_td_target_td3(0, nets[0].ref(), nets[1].ref(), nets[2].ref(), xt.data_ptr(), rt.data_ptr(), dt.data_ptr(), noise.data_ptr(),
                               draws.data_ptr(), SEED, t.data_ptr(), None, None, None)
    torch.cuda.synchronize()
    assert rc == _capi.S2D_EINVAL and b'batch' in lib.s2d_last_error()
    assert int(draws[0]) == 2 ** 32 + 2 and bool((t == S_F).all())


def _modules(D, A, pi, qf, twin):
    def seq(n_in, hidden, n_out, head=False):
        layers = [m for w_in, w in zip((n_in,) + hidden, hidden) for m in (nn.Linear(w_in, w), nn.ReLU())] + [nn.Linear(hidden[-1], n_out)]
        return nn.Sequential(*layers, *([nn.Tanh()] if head else [])).to(DEV)
    return seq(D, pi, A, head=True), seq(D + A, qf, 1), (seq(D + A, qf, 1) if twin else None)


def _net_of(module):
    lin = [m for m in module if isinstance(m, nn.Linear)]
    p = np.concatenate([np.concatenate([l.weight.detach().cpu().numpy().ravel(), l.bias.detach().cpu().numpy().ravel()]) for l in lin])
    return TD.Net(lin[0].in_features, [l.out_features for l in lin[:-1]], lin[-1].out_features, 'relu', p)


def test_sample_then_target_in_one_captured_graph(L):
    """sample(out=) -> Td3Target.target(out=) captured once and replayed three times, the noise words rewritten between the
    replays: each replay equals the restatement at draws = k, k + 1, k + 2 on the batch it sampled.  A linear chain."""
    from soccer2d_amd.replay import DeviceReplay
    from soccer2d_amd.td import Td3Target
    torch.manual_seed(4)
    rng = np.random.default_rng(4)
    B, D, A, k = 96, 10, 4, BIG
    rec, first = RR.synthetic_record(rng, 3, 50, D, A, float_action=True)
    mu, q1, q2 = _modules(D, A, (20, 12), (16,), True)
    rb = DeviceReplay(512, D, action_words=A, action_dtype=torch.float32, device=DEV, seed=9)
    rb.push(dev_rec(rec), torch.from_numpy(first).to(DEV))
    t = Td3Target(mu, q1, q2, seed=SEED)
    assert t.noise.tolist() == [float(F(0.2)), 0.5] and int(t.draws[0]) == 0
    t.draws.fill_(k)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                            # a warm-up outside the capture, on objects of its own
        warm = DeviceReplay(512, D, action_words=A, action_dtype=torch.float32, device=DEV, seed=9)
        warm.push(dev_rec(rec), torch.from_numpy(first).to(DEV))
        Td3Target(mu, q1, q2, seed=SEED).target(warm.sample(B), return_q=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    batch = rb.alloc_batch(B)
    out = tuple(torch.full(s, S_F, device=DEV) for s in ((B,), (B,), (B, A)))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rb.sample(B, out=batch)
        t.target(batch, out=out, return_q=True)
    torch.cuda.synchronize()
    assert bool((out[0] == S_F).all()) and int(t.draws[0]) == k              # capturing ran nothing
    nets = _net_of(mu), _net_of(q1), _net_of(q2)
    seen = []
    for n, (sigma, clip) in enumerate(((0.2, 0.5), (0.2, 0.5), (1.5, 0.25))):
        t.set_noise(sigma, clip)
        graph.replay()
        torch.cuda.synchronize()
        assert int(t.draws[0]) == k + n + 1 and rb.cursor.cpu().tolist()[3] == n + 1
        want = T3.target(L, *nets, *host(batch), sigma, clip, k + n, SEED)
        for g, w, name in zip(out, want, NAMES):
            same(g, w, f'replay {n} {name}')
        seen.append((out[2].cpu().numpy() - want[3]).copy())                  # the noise that was added
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    assert np.abs(seen[1]).max() > 0.25 and np.abs(seen[2]).max() <= 0.25 + 2e-7 and (np.abs(seen[2]) > 0.2).mean() > 0.5
    # the class eagerly: sync() after an in-place change of the modules
    b = rb.sample(B)
    same(t.target(b), T3.target(L, *nets, *host(b), 1.5, 0.25, k + 3, SEED)[0], 'eager')
    with torch.no_grad():
        mu[0].weight.mul_(1.5); q1[0].bias.add_(0.25)
    same(t.target(b), T3.target(L, *nets, *host(b), 1.5, 0.25, k + 4, SEED)[0], 'without sync() nothing changes')
    t.sync()
    got = t.target(b, return_q=True)
    for g, w, name in zip(got, T3.target(L, _net_of(mu), _net_of(q1), _net_of(q2), *host(b), 1.5, 0.25, k + 5, SEED), NAMES):
        same(g, w, f'after sync() {name}')


def plan_fits(wmax16, n_in, na, waves, tiles):
    rp, xp, qp = (wmax16 + 63) // 64 * 64 + 4, ((n_in + 3) // 4 * 4 + 63) // 64 * 64 + 4, (na + 15) // 16 * 16 + 4
    return waves * (tiles * 16 * (xp + 2 * rp) + 64 * qp) * 4 <= 160 * 1024


def test_results_do_not_depend_on_the_plan(L, lib, monkeypatch):
    """S2D_TD_PLAN=waves,tiles (read at every launch): every pair that fits gives the same bits, the others are refused by name"""
    rs = np.random.RandomState(3)
    B, D, A = 300, 16, 5
    actor, c1, c2 = nets_of(rs, D, A, (28, 136), (64, 64), 'sigmoid', True)
    x, r, d = batch_of(rs, B, D)
    nets = DevNet(lib, actor), DevNet(lib, c1), DevNet(lib, c2)
    want = T3.target(L, actor, c1, c2, x, r, d, 0.2, 0.5, BIG, SEED)
    ran = 0
    for waves in (4, 2, 1):
        for tiles in (4, 2, 1):
            monkeypatch.setenv('S2D_TD_PLAN', f'{waves},{tiles}')
            fits = plan_fits(144, D + A, A, waves, tiles)
            try:
                got = run_td3(lib, *nets, x, r, d, 0.2, 0.5, word(BIG))
                assert fits
                ran += 1
                for g, w, name in zip(got, want, NAMES):
                    same(g, w, f'plan {waves},{tiles} {name}')
            except ValueError as e:
                assert not fits and 'S2D_TD_PLAN' in str(e) and 's2d_td_target_td3' in str(e), (waves, tiles, str(e))
    monkeypatch.delenv('S2D_TD_PLAN')
    assert ran >= 6
    for g, w, name in zip(run_td3(lib, *nets, x, r, d, 0.2, 0.5, word(BIG)), want, NAMES):
        same(g, w, f'the plan\'s own choice: {name}')


def test_with_the_learner(L):
    """ActorCriticLearner with q2: a critic-only step and a full step, each followed by update_targets(td3, tau).  The next
    Td3Target.target equals the restatement on the Polyak-stepped parameters, with no sync()."""
    from soccer2d_amd.learn import ActorCriticLearner
    from soccer2d_amd.td import Td3Target
    torch.manual_seed(11)
    rs = np.random.RandomState(11)
    B, D, A, tau = 64, 10, 1, 0.005
    mods = _modules(D, A, (16, 16), (16, 16), True)
    tmods = copy.deepcopy(mods)
    lrn = ActorCriticLearner.from_modules(*mods, max_batch=B)
    td3 = Td3Target.from_modules(*tmods, seed=SEED)
    x, r, d = batch_of(rs, B, D)
    batch = {'obs': to_dev(rs.uniform(-1, 1, (B, D)).astype(F)), 'action': to_dev(rs.uniform(-1, 1, (B, A)).astype(F)),
             'next_obs': to_dev(x), 'reward': to_dev(r), 'discount': to_dev(d)}
    tnets, nets = (td3.mu_target,) + td3.critics, (lrn.actor,) + lrn.critics
    mine = [n.params.clone() for n in tnets]                                 # the same lerp on copies: the expected parameters
    first = [m.clone() for m in mine]

    def check(n):
        got = td3.target(batch, return_q=True)
        host_nets = [TD.Net(t.n_in, t.hidden, t.n_out, 'relu', m.cpu().numpy()) for t, m in zip(tnets, mine)]
        for g, w, name in zip(got, T3.target(L, *host_nets, x, r, d, 0.2, 0.5, n, SEED), NAMES):
            same(g, w, f'after {n} updates: {name}')
        return got[0]
    target = check(0)
    for n, with_actor in enumerate((False, True)):
        lrn.step(batch, target, actor=with_actor)
        lrn.update_targets(td3, tau)
        mine = [m.lerp(p.params, tau) for m, p in zip(mine, nets)]
        assert torch.equal(mine[0], first[0]) == (not with_actor)             # the critic-only step leaves the actor where it was
        assert not torch.equal(mine[1], first[1]) and not torch.equal(mine[2], first[2])
        target = check(n + 1)
    assert int(td3.draws[0]) == 3
    for t, m in zip(tnets, mine):
        assert torch.equal(t.params, m)


def test_rejections_return_einval_with_text_and_launch_nothing(lib, monkeypatch):
    from soccer2d_amd import _capi
    rs = np.random.RandomState(8)
    B, D, A = 70, 10, 4
    actor, c1, c2 = (DevNet(lib, n) for n in nets_of(rs, D, A, (20, 12), (16,), 'relu', True))
    x, r, d = (to_dev(v) for v in batch_of(rs, B, D))
    noise, draws = torch.tensor([0.2, 0.5], device=DEV), word(11)
    t, q, a = _out(B), _out(B), _out(B, (A,))
    base = dict(actor=actor.ref(), c1=c1.ref(), c2=c2.ref(), B=B, x=x.data_ptr(), r=r.data_ptr(), d=d.data_ptr(), noise=noise.data_ptr(),
                draws=draws.data_ptr(), t=t.data_ptr(), q=q.data_ptr(), a=a.data_ptr())

    def refused(what, needle, **over):
        p = dict(base, **over)
        rc = lib.s2d_td_target_td3(p['B'], p['actor'], p['c1'], p['c2'], p['x'], p['r'], p['d'], p['noise'], p['draws'], SEED, p['t'], p['q'],
                                   p['a'], None)
        text = lib.s2d_last_error().decode()
        assert rc == _capi.S2D_EINVAL and 's2d_td_target_td3' in text and needle in text, (what, rc, text)

    def copy_of(s, **over):
        c = _capi.S2DTdNet()
        C.memmove(C.byref(c), C.byref(s), C.sizeof(c))
        for k, v in over.items():
            setattr(c, k, v)
        return C.byref(c)
    refused('actor NULL', 'actor', actor=None)
    refused('critic1 NULL', 'critic1', c1=None)
    refused('n_out 9', 'n_out', actor=copy_of(actor.s, n_out=9))
    refused('n_out 0', 'n_out', actor=copy_of(actor.s, n_out=0))
    refused('critic n_in', 'critic1', c1=copy_of(c1.s, n_in=D + A + 1))
    refused('critic2 n_out', 'critic2', c2=copy_of(c2.s, n_out=2))
    refused('hidden off the grid', 'hidden', actor=copy_of(actor.s, n_hidden=6))
    refused('params NULL', 'params', actor=copy_of(actor.s, params=None))
    refused('params misaligned', 'params', actor=copy_of(actor.s, params=actor.params.data_ptr() + 4))
    refused('workspace NULL', 'workspace', c2=copy_of(c2.s, workspace=None))
    refused('workspace small', 'workspace', c1=copy_of(c1.s, workspace_bytes=c1.words * 4 - 4))
    refused('shared workspace', 'share', c2=copy_of(c2.s, workspace=c1.s.workspace))
    refused('batch 0', 'batch', B=0)
    refused('batch 2^31', 'batch', B=2 ** 31)
    refused('next_obs NULL', 'next_obs', x=None)
    refused('reward misaligned', 'reward', r=r.data_ptr() + 2)
    refused('out_target NULL', 'out_target', t=None)
    refused('out_target misaligned', 'out_target', t=t.data_ptr() + 2)
    refused('out_q misaligned', 'optional', q=q.data_ptr() + 2)
    refused('out_action misaligned', 'optional', a=a.data_ptr() + 1)
    refused('noise NULL', 'noise', noise=None)
    refused('noise misaligned', 'noise', noise=noise.data_ptr() + 2)
    refused('draws NULL', 'draws', draws=None)
    refused('draws misaligned', 'draws', draws=draws.data_ptr() + 4)
    refused('draws inside out_action', 'draws must not overlap', draws=a.data_ptr() + 8)
    refused('draws inside out_target', 'draws must not overlap', draws=t.data_ptr())
    refused('draws inside out_q', 'draws must not overlap', draws=q.data_ptr() + 8 * (B // 2 - 1))
    refused('noise inside out_target', 'noise must not overlap', noise=t.data_ptr() + 4 * (B - 1))
    refused('noise inside out_q', 'noise must not overlap', noise=q.data_ptr())
    refused('noise inside out_action', 'noise must not overlap', noise=a.data_ptr() + 4 * (B * A - 1))
    monkeypatch.setenv('S2D_TD_PLAN', '3,1')
    refused('plan', 'S2D_TD_PLAN')
    monkeypatch.delenv('S2D_TD_PLAN')
    torch.cuda.synchronize()
    # nothing ran: every output and every workspace still holds its sentinel, and the words what they held
    assert all(bool((v == S_F).all()) for v in (t, q, a)) and int(draws[0]) == 11 and noise.tolist() == [float(F(0.2)), 0.5]
    for n in (actor, c1, c2):
        assert bool((n.ws == -3333.0).all())
    assert PAD > 0
