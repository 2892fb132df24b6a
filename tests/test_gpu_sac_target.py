"""The SAC target (s2d_td_target_sac; soccer2d_amd.td.SacTarget) on the GPU, bit for bit against the host restatement
(tests/sac_ref.c): every batch edge at one to eight action dimensions (the second Philox block whole and partial), 10, 16 and 224
inputs, with and without the second critic and the optional outputs; the NaN rule of the twin minimum; the accounting of the
`draws` word in eager calls and in a captured sample -> target graph with alpha rewritten between replays; independence of the
plan; the head's consistency with the rollout's greedy action through the diagnostic entry point (s2d_debug_td_target_sac, the
target with a deterministic switch); and the rejections, which launch nothing."""
import ctypes as C

import numpy as np
import pytest

import replay as RR
import sac_ref as S
import td as TD
from test_gpu_td import DEV, PAD, S_F, DevNet, _out, _take, batch_of, dev_rec, host, same, to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
nn = torch.nn
F = np.float32
SEED = 0x1234ABCD5EED


@pytest.fixture(scope='module')
def L(tmp_path_factory):
    return S.build(tmp_path_factory.mktemp('sac_ref'))


@pytest.fixture(scope='module')
def lib():
    from soccer2d_amd import _capi
    return _capi.load_library()


def run_sac(lib, actor, c1, c2, x, r, d, alpha, draws, seed=SEED, det=None, with_q=True, with_action=True, with_logp=True):
    """s2d_td_target_sac (det given: its diagnostic form) on device copies; `draws`: a device int64 word, advanced by the call.
    (target, q, action, logp), None where not asked for; guards checked"""
    from soccer2d_amd import _capi
    B, A = x.shape[0], actor.net.n_out // 2
    xt, rt, dt = to_dev(x.astype(F)), to_dev(r.astype(F)), to_dev(d.astype(F))
    al = torch.tensor([alpha], dtype=torch.float32, device=DEV)
    t, q, a, lp = _out(B), (_out(B) if with_q else None), (_out(B, (A,)) if with_action else None), (_out(B) if with_logp else None)
    ptr = lambda v: None if v is None else v.data_ptr()
    torch.cuda.synchronize()
    head = (B, actor.ref(), c1.ref(), c2.ref() if c2 is not None else None, xt.data_ptr(), rt.data_ptr(), dt.data_ptr(), al.data_ptr(),
            draws.data_ptr(), seed)
    if det is None:
        rc = lib.s2d_td_target_sac(*head, t.data_ptr(), ptr(q), ptr(a), ptr(lp), None)
    else:
        rc = lib.s2d_debug_td_target_sac(*head, int(det), t.data_ptr(), ptr(q), ptr(a), ptr(lp), None)
    _capi.check(lib, rc, 's2d_td_target_sac')
    torch.cuda.synchronize()
    for n in (actor, c1, c2):
        if n is not None:
            n.check_guard()
    return (_take(t, B, 'target'), _take(q, B, 'q') if with_q else None, _take(a, B, 'action') if with_action else None,
            _take(lp, B, 'logp') if with_logp else None)


def word(v=0):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


def nets_of(rs, D, A, pi, qf, act, twin, ls_bias=-1.0):
    actor = TD.random_net(rs, D, pi, 2 * A, act)
    actor.params[-A:] += F(ls_bias)                                          # the raw log-std rows around ls_bias
    c1 = TD.random_net(rs, D + A, qf, 1, act)
    c2 = TD.random_net(rs, D + A, qf, 1, act) if twin else None
    return actor, c1, c2


# (D, A, actor hidden, critic hidden, activation, twin)
CASES = [(10, 1, (64, 64), (64, 64), 'relu', True), (10, 4, (20, 12), (16,), 'tanh', False), (16, 5, (16, 8), (12, 20), 'sigmoid', True),
         (16, 8, (64,), (64, 64), 'relu', False), (224, 4, (64, 64), (64, 64), 'tanh', True)]
NAMES = ('target', 'q', 'action', 'logp')


@pytest.mark.parametrize('B', [1, 63, 64, 65, 200])
@pytest.mark.parametrize('D,A,pi,qf,act,twin', CASES, ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_target_equals_the_restatement(L, lib, D, A, pi, qf, act, twin, B):
    rs = np.random.RandomState(D + A + B)
    actor, c1, c2 = nets_of(rs, D, A, pi, qf, act, twin)
    x, r, d = batch_of(rs, B, D)
    draws = word(5)
    got = run_sac(lib, DevNet(lib, actor), DevNet(lib, c1), DevNet(lib, c2) if twin else None, x, r, d, 0.2, draws)
    want = S.target(L, actor, c1, c2, x, r, d, 0.2, 5, SEED)
    for g, w, name in zip(got, want, NAMES):
        same(g, w, name)
    assert int(draws[0]) == 6
    a = got[2]
    assert (np.abs(a) <= 1).all() and np.isfinite(got[3]).all() and (B < 60 or len(np.unique(a)) > B // 2)


def test_nan_in_q2_never_replaces_q1_and_null_outputs(L, lib):
    rs = np.random.RandomState(4)
    D, A, B = 10, 4, 70
    actor = nets_of(rs, D, A, (20, 12), (8,), 'relu', False)[0]

    def const(v):
        p = np.zeros(TD.param_count(D + A, (8,), 1), F)
        p[-1] = v
        return TD.Net(D + A, (8,), 1, 'relu', p)
    x, r, d = batch_of(rs, B, D)
    da = DevNet(lib, actor)
    for q1, q2, want_q in ((1.5, np.nan, 1.5), (np.nan, 1.0, np.nan), (2.0, 1.0, 1.0), (1.0, 2.0, 1.0)):
        got = run_sac(lib, da, DevNet(lib, const(q1)), DevNet(lib, const(q2)), x, r, d, 0.5, word())
        want = S.target(L, actor, const(q1), const(q2), x, r, d, 0.5, 0, SEED)
        for g, w, name in zip(got, want, NAMES):
            same(g, w, f'q1={q1} q2={q2} {name}')
        same(got[1], np.full(B, want_q, F), f'q1={q1} q2={q2}')
    c1 = TD.random_net(rs, D + A, (16,), 1, 'relu')
    full = S.target(L, actor, c1, None, x, r, d, 0.3, 0, SEED)
    d1 = DevNet(lib, c1)
    for wq, wa, wl in ((False, False, False), (True, False, False), (False, True, False), (False, False, True), (True, True, False)):
        got = run_sac(lib, da, d1, None, x, r, d, 0.3, word(), with_q=wq, with_action=wa, with_logp=wl)
        for g, w, name, asked in zip(got, full, NAMES, (True, wq, wa, wl)):
            assert (g is not None) == asked
            if asked:
                same(g, w, f'outputs {wq, wa, wl}: {name}')


def test_draws_accounting_in_eager_calls(L, lib):
    """two calls on one word equal the restatement at draws = 0 and 1, and differ; another seed draws other noise"""
    rs = np.random.RandomState(6)
    actor, c1, c2 = nets_of(rs, 10, 1, (64, 64), (64, 64), 'relu', True)
    x, r, d = batch_of(rs, 130, 10)
    nets = DevNet(lib, actor), DevNet(lib, c1), DevNet(lib, c2)
    draws = word()
    first, second = run_sac(lib, *nets, x, r, d, 0.1, draws), run_sac(lib, *nets, x, r, d, 0.1, draws)
    assert int(draws[0]) == 2
    for n, got in enumerate((first, second)):
        for g, w, name in zip(got, S.target(L, actor, c1, c2, x, r, d, 0.1, n, SEED), NAMES):
            same(g, w, f'draws={n} {name}')
    assert not np.array_equal(first[2], second[2])
    other = run_sac(lib, *nets, x, r, d, 0.1, word(), seed=SEED + 1)
    assert not np.array_equal(first[2], other[2])
    big = run_sac(lib, *nets, x, r, d, 0.1, word(2 ** 32 + 3))                # the counter's high word
    same(big[2], S.target(L, actor, c1, c2, x, r, d, 0.1, 2 ** 32 + 3, SEED)[2], 'draws = 2^32 + 3')


def _modules(D, A, pi, qf, twin):
    seq = lambda n_in, hidden, n_out: nn.Sequential(*[m for w_in, w in zip((n_in,) + hidden, hidden) for m in (nn.Linear(w_in, w), nn.ReLU())],
                                                    nn.Linear(hidden[-1], n_out)).to(DEV)
    actor = seq(D, pi, 2 * A)
    with torch.no_grad():
        actor[-1].bias[A:].sub_(1.0)
    return actor, seq(D + A, qf, 1), (seq(D + A, qf, 1) if twin else None)


def _net_of(module):
    lin = [m for m in module if isinstance(m, nn.Linear)]
    p = np.concatenate([np.concatenate([l.weight.detach().cpu().numpy().ravel(), l.bias.detach().cpu().numpy().ravel()]) for l in lin])
    return TD.Net(lin[0].in_features, [l.out_features for l in lin[:-1]], lin[-1].out_features, 'relu', p)


def test_sample_then_target_in_one_captured_graph(L):
    """sample(out=) -> SacTarget.target(out=) captured once and replayed three times, alpha (a device word) rewritten between
    the replays: each replay equals the restatement at draws = 0, 1, 2 on the batch it sampled.  A linear chain."""
    from soccer2d_amd.replay import DeviceReplay
    from soccer2d_amd.td import SacTarget
    torch.manual_seed(4)
    rng = np.random.default_rng(4)
    B, D, A = 96, 10, 4
    rec, first = RR.synthetic_record(rng, 3, 50, D, A, float_action=True)
    actor, q1, q2 = _modules(D, A, (20, 12), (16,), True)
    rb = DeviceReplay(512, D, action_words=A, action_dtype=torch.float32, device=DEV, seed=9)
    rb.push(dev_rec(rec), torch.from_numpy(first).to(DEV))
    t = SacTarget(actor, q1, q2, seed=SEED)
    alpha = torch.tensor([0.2], device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                            # a warm-up outside the capture, on objects of its own
        warm = DeviceReplay(512, D, action_words=A, action_dtype=torch.float32, device=DEV, seed=9)
        warm.push(dev_rec(rec), torch.from_numpy(first).to(DEV))
        SacTarget(actor, q1, q2, seed=SEED).target(warm.sample(B), alpha, return_q=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    batch = rb.alloc_batch(B)
    out = tuple(torch.full(s, S_F, device=DEV) for s in ((B,), (B,), (B, A), (B,)))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rb.sample(B, out=batch)
        t.target(batch, alpha, out=out, return_q=True)
    torch.cuda.synchronize()
    assert bool((out[0] == S_F).all()) and int(t.draws[0]) == 0              # capturing ran nothing
    nets = _net_of(actor), _net_of(q1), _net_of(q2)
    seen = []
    for n, al in enumerate((0.2, 0.05, 1.0)):
        alpha.fill_(al)
        graph.replay()
        torch.cuda.synchronize()
        assert int(t.draws[0]) == n + 1 and rb.cursor.cpu().tolist()[3] == n + 1
        want = S.target(L, *nets, *host(batch), float(F(al)), n, SEED)
        for g, w, name in zip(out, want, NAMES):
            same(g, w, f'replay {n} {name}')
        seen.append(out[2].cpu().numpy().copy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    # the class eagerly: a float alpha, sync() after an in-place change of the modules
    b = rb.sample(B)
    same(t.target(b, 0.3), S.target(L, *nets, *host(b), 0.3, 3, SEED)[0], 'eager, float alpha')
    with torch.no_grad():
        actor[0].weight.mul_(1.5); q1[0].bias.add_(0.25)
    same(t.target(b, 0.3), S.target(L, *nets, *host(b), 0.3, 4, SEED)[0], 'without sync() nothing changes')
    t.sync()
    got = t.target(b, 0.3, return_q=True)
    for g, w, name in zip(got, S.target(L, _net_of(actor), _net_of(q1), _net_of(q2), *host(b), 0.3, 5, SEED), NAMES):
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
    want = S.target(L, actor, c1, c2, x, r, d, 0.2, 1, SEED)
    ran = 0
    for waves in (4, 2, 1):
        for tiles in (4, 2, 1):
            monkeypatch.setenv('S2D_TD_PLAN', f'{waves},{tiles}')
            fits = plan_fits(144, D + A, 2 * A, waves, tiles)
            try:
                got = run_sac(lib, *nets, x, r, d, 0.2, word(1))
                assert fits
                ran += 1
                for g, w, name in zip(got, want, NAMES):
                    same(g, w, f'plan {waves},{tiles} {name}')
            except ValueError as e:
                assert not fits and 'S2D_TD_PLAN' in str(e) and 's2d_td_target_sac' in str(e), (waves, tiles, str(e))
    monkeypatch.delenv('S2D_TD_PLAN')
    assert ran >= 6
    for g, w, name in zip(run_sac(lib, *nets, x, r, d, 0.2, word(1)), want, NAMES):
        same(g, w, f'the plan\'s own choice: {name}')


@pytest.mark.parametrize('mode', ['cont1', 'turn4'])
def test_head_is_the_rollouts(L, lib, mode):
    """the same parameters, z = 0 on both sides: out_action of the diagnostic call (deterministic = 1) on the engine's
    observations equals the greedy action the rollout takes from them; deterministic = 0 is s2d_td_target_sac itself"""
    from soccer2d_amd.wide_actor import SquashedGaussianActor
    from test_gpu_ppo_actor import _engine
    A, n = S.NA[mode], 200
    rs = np.random.RandomState(A)
    actor, c1, _ = nets_of(rs, 10, A, (20, 12), (16,), 'tanh', False)
    eng = _engine(n, mode, 'lattice')
    eng.reset()
    eng.rollout(3)
    x = eng.obs.cpu().numpy().copy()
    sac = SquashedGaussianActor((20, 12), A, activation='tanh', device=DEV, deterministic=True)
    sac.params.copy_(to_dev(actor.params))
    rec = eng.rollout_sac(1, sac)
    torch.cuda.synchronize()
    r, d = np.zeros(n, F), np.ones(n, F)
    nets = DevNet(lib, actor), DevNet(lib, c1), None
    got = run_sac(lib, *nets, x, r, d, 0.2, word(), det=1)
    same(got[2], rec['action'][0].cpu().numpy(), 'action')
    same(got[3], rec['logp'][0].cpu().numpy(), 'logp')
    for g, w, name in zip(got, S.target(L, actor, c1, None, x, r, d, 0.2, 0, SEED, det=1), NAMES):
        same(g, w, f'deterministic {name}')
    for g, w, name in zip(run_sac(lib, *nets, x, r, d, 0.2, word(7), det=0), run_sac(lib, *nets, x, r, d, 0.2, word(7)), NAMES):
        same(g, w, f'deterministic = 0 {name}')


def test_rejections_return_einval_with_text_and_launch_nothing(lib, monkeypatch):
    from soccer2d_amd import _capi
    rs = np.random.RandomState(8)
    B, D, A = 70, 10, 4
    actor, c1, c2 = (DevNet(lib, n) for n in nets_of(rs, D, A, (20, 12), (16,), 'relu', True))
    x, r, d = (to_dev(v) for v in batch_of(rs, B, D))
    alpha, draws = torch.tensor([0.2], device=DEV), word(11)
    t, q, a, lp = _out(B), _out(B), _out(B, (A,)), _out(B)
    base = dict(actor=actor.ref(), c1=c1.ref(), c2=c2.ref(), B=B, x=x.data_ptr(), r=r.data_ptr(), d=d.data_ptr(), alpha=alpha.data_ptr(),
                draws=draws.data_ptr(), t=t.data_ptr(), q=q.data_ptr(), a=a.data_ptr(), lp=lp.data_ptr())

    def refused(what, needle, **over):
        p = dict(base, **over)
        rc = lib.s2d_td_target_sac(p['B'], p['actor'], p['c1'], p['c2'], p['x'], p['r'], p['d'], p['alpha'], p['draws'], SEED, p['t'], p['q'],
                                   p['a'], p['lp'], None)
        text = lib.s2d_last_error().decode()
        assert rc == _capi.S2D_EINVAL and 's2d_td_target_sac' in text and needle in text, (what, rc, text)

    def copy_of(s, **over):
        c = _capi.S2DTdNet()
        C.memmove(C.byref(c), C.byref(s), C.sizeof(c))
        for k, v in over.items():
            setattr(c, k, v)
        return C.byref(c)
    refused('actor NULL', 'actor', actor=None)
    refused('critic1 NULL', 'critic1', c1=None)
    refused('odd n_out', 'n_out', actor=copy_of(actor.s, n_out=2 * A - 1))
    refused('n_out 0', 'n_out', actor=copy_of(actor.s, n_out=0))
    refused('critic n_in', 'critic1', c1=copy_of(c1.s, n_in=D + 2 * A))
    refused('critic2 n_out', 'critic2', c2=copy_of(c2.s, n_out=2))
    refused('params misaligned', 'params', actor=copy_of(actor.s, params=actor.params.data_ptr() + 4))
    refused('workspace small', 'workspace', c1=copy_of(c1.s, workspace_bytes=c1.words * 4 - 4))
    refused('shared workspace', 'share', c2=copy_of(c2.s, workspace=c1.s.workspace))
    refused('batch 0', 'batch', B=0)
    refused('next_obs NULL', 'next_obs', x=None)
    refused('out_target misaligned', 'out_target', t=t.data_ptr() + 2)
    refused('out_logp misaligned', 'optional', lp=lp.data_ptr() + 2)
    refused('alpha NULL', 'alpha', alpha=None)
    refused('alpha misaligned', 'alpha', alpha=alpha.data_ptr() + 1)
    refused('draws NULL', 'draws', draws=None)
    refused('draws misaligned', 'draws', draws=draws.data_ptr() + 4)
    refused('draws inside out_action', 'draws', draws=a.data_ptr() + 8)
    refused('draws inside out_target', 'draws', draws=t.data_ptr())
    monkeypatch.setenv('S2D_TD_PLAN', '3,1')
    refused('plan', 'S2D_TD_PLAN')
    monkeypatch.delenv('S2D_TD_PLAN')
    torch.cuda.synchronize()
    # nothing ran: every output and every workspace still holds its sentinel, and the word its count
    assert all(bool((v == S_F).all()) for v in (t, q, a, lp)) and int(draws[0]) == 11
    for n in (actor, c1, c2):
        assert bool((n.ws == -3333.0).all())
    assert PAD > 0
