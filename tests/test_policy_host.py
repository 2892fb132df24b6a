"""CPU checks of the stochastic policy's host restatement (tests/policy_ref.c, the bit-level statement of s2d_rollout_policy's
heads and of s2d_gae that the GPU tests compare the device with): the categorical draw's frequencies, logp against float64, the
edge rows by value, gae against a float64 statement of SB3's compute_returns_and_advantage, and the module forms
StochasticActor.from_module accepts and refuses."""
import math

import numpy as np
import pytest

import policy_ref as P

SEED = 0x5EED


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp('policy_ref'))


@pytest.fixture(scope='module')
def gauss_ref(tmp_path_factory):
    import actor_ref as R
    L = R.build(tmp_path_factory.mktemp('actor_ref'))
    return lambda gid, ctr: R.gauss(L, SEED, gid, ctr)


def chi2_sf_odd(x, dof):
    """P(chi2_dof > x) for odd dof: Q(1/2, h) = erfc(sqrt(h)), Q(s + 1, h) = Q(s, h) + h^s e^-h / Gamma(s + 1), h = x / 2"""
    assert dof % 2 == 1
    h, s = x / 2.0, 0.5
    q = math.erfc(math.sqrt(h))
    while s < dof / 2.0:
        q += math.exp(s * math.log(h) - h - math.lgamma(s + 1.0))
        s += 1.0
    return q


def chi2_stat(counts, prob):
    n = counts.sum()
    return float((((counts - n * prob) ** 2) / (n * prob)).sum())


def fixed_logits():
    """the one logit row of the frequency tests: A = 16, uniform in [-1, 1], so every probability is >= 1 / (16 e^2)"""
    return np.random.RandomState(20240607).uniform(-1, 1, 16).astype(np.float32)


def softmax64(y):
    y = np.asarray(y, dtype=np.float64)
    e = np.exp(y - y.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def test_chi2_sf_known_values():
    assert abs(chi2_sf_odd(24.99579, 15) - 0.05) < 1e-6 and abs(chi2_sf_odd(37.69730, 15) - 0.001) < 1e-7


def test_categorical_frequencies(ref):
    """2^18 draws at consecutive policy steps of one env against the float64 softmax: chi-square with 15 degrees of freedom,
    accepted below the 1 - 1e-6 quantile"""
    y = fixed_logits()
    prob = softmax64(y)
    assert prob.min() >= 1 / (16 * math.e ** 2)
    n = 1 << 18
    a, lp = P.head(ref, 'discrete', np.broadcast_to(y, (n, 16)), None, 7, np.arange(n), SEED)
    assert a.min() >= 0 and a.max() <= 15
    stat = chi2_stat(np.bincount(a, minlength=16).astype(np.float64), prob)
    assert chi2_sf_odd(stat, 15) > 1e-6, stat
    assert np.abs(lp.astype(np.float64) - np.log(prob)[a]).max() < 1e-6


LOGP_TOL_DISCRETE = 4 * 7.2e-7
LOGP_TOL_GAUSS = 4 * 1.4e-6


@pytest.mark.parametrize('A', [1, 2, 16, 64])
def test_categorical_logp_against_float64(ref, A):
    """logp of the sampled action against a float64 log-softmax over 4 096 rows with logits up to +-20.  Measured maximum
    absolute difference: 0 (A = 1), 3.5e-7 (A = 2), 4.3e-7 (A = 16), 7.2e-7 (A = 64) -- the rounding of the sequential sum
    grows with A; allowed: 4 x 7.2e-7."""
    rs = np.random.RandomState(100 + A)
    y = (rs.uniform(-1, 1, (4096, A)) * rs.uniform(0, 20, (4096, 1))).astype(np.float32)
    a, lp = P.head(ref, 'discrete', y, None, np.arange(4096), rs.randint(0, 2 ** 32, 4096, dtype=np.uint64), SEED)
    want = np.log(softmax64(y))[np.arange(4096), a]
    err = np.abs(lp.astype(np.float64) - want).max()
    print(f'A={A}: max |logp - float64| = {err:.3e}')
    assert err <= LOGP_TOL_DISCRETE
    ag, lpg = P.head(ref, 'discrete', y, None, np.arange(4096), 0, SEED, det=1)
    assert np.array_equal(ag, y.argmax(axis=1))
    assert np.abs(lpg.astype(np.float64) - np.log(softmax64(y)).max(axis=1)).max() <= LOGP_TOL_DISCRETE


@pytest.mark.parametrize('mode,A', [('cont1', 1), ('turn4', 4)])
def test_gaussian_logp_against_float64(ref, gauss_ref, mode, A):
    """logp of the recorded (unclipped) action against the float64 diagonal-Gaussian log-density evaluated at the restatement's
    own z (actor_ref.gauss, the block of s2d_debug_eval op 15), 4 096 rows, means up to +-20, log_std in [-2, 0.5].  Measured
    maximum absolute difference: 2.5e-7 (A = 1), 1.4e-6 (A = 4); allowed: 4 x 1.4e-6."""
    rs = np.random.RandomState(200 + A)
    n = 4096
    y = (rs.uniform(-1, 1, (n, A)) * rs.uniform(0, 20, (n, 1))).astype(np.float32)
    ls = rs.uniform(-2, 0.5, A).astype(np.float32)
    gid = np.arange(n, dtype=np.uint64) + 5
    k = rs.randint(0, 2 ** 32, n, dtype=np.uint64)
    a, lp = P.head(ref, mode, y, ls, gid, k, SEED)
    k32 = (k & 0xFFFFFFFF).astype(np.uint32)
    if mode == 'turn4':
        z = gauss_ref(gid, k32)
    else:
        z = gauss_ref(gid, k32 >> 2)[np.arange(n), k32 & 3][:, None]
    z64, ls64 = z.astype(np.float64), ls.astype(np.float64)
    # the action is mean + sigma z (one fmaf: error below an ulp of the result); the density of that action
    assert np.abs(a.astype(np.float64) - (y + np.exp(ls64) * z64)).max() < 4e-6
    want = (-0.5 * z64 ** 2 - ls64 - 0.5 * math.log(2 * math.pi)).sum(axis=1)
    err = np.abs(lp.astype(np.float64) - want).max()
    print(f'{mode}: max |logp - float64| = {err:.3e}')
    assert err <= LOGP_TOL_GAUSS
    ad, lpd = P.head(ref, mode, y, ls, gid, k, SEED, det=1)
    assert np.array_equal(ad, np.clip(y, -1, 1))
    assert np.abs(lpd.astype(np.float64) - (-ls64 - 0.5 * math.log(2 * math.pi)).sum()).max() <= LOGP_TOL_GAUSS


def edge_rows():
    """(name, logits [A]) of the edge cases shared with the GPU head test"""
    f = np.float32
    peak = np.full(16, -3.0, f); peak[11] = 197.0
    tie = np.array([0.25, 1.5, -1.0, 1.5, 0.0], f)
    nan = np.array([0.3, np.nan, -0.2, 0.9, 0.1, np.nan], f)
    return [('single', np.array([0.7], f)), ('equal', np.full(16, 0.37, f)), ('peak', peak), ('tie', tie), ('nan', nan),
            ('nan_first', np.array([np.nan, 1.0, 2.0], f)), ('inf', np.array([0.0, np.inf, 1.0], f))]


EDGE_WORDS = np.array([0, 1 << 8, 0x7FFFFFFF, 0x80000000, 0x12345678, 0xDEADBEEF, 0x40000000, 0xB0000000,
                       0xFFFFFEFF, 0xFFFFFFFF], dtype=np.uint32)


def test_edge_rows_by_value(ref):
    rows = dict(edge_rows())
    W = EDGE_WORDS
    u = (W >> 8).astype(np.float64) * 2.0 ** -24
    assert u[-1] == 1 - 2.0 ** -24

    def run(name, det=0):
        return P.categorical(ref, np.broadcast_to(rows[name], (len(W), rows[name].size)), W, det)
    a, lp = run('single')                                   # A = 1
    assert (a == 0).all() and (lp == 0).all()
    a, lp = run('equal')                                    # the action follows u alone: floor(16 u)
    assert np.array_equal(a, np.floor(16 * u).astype(np.int32)) and a[-1] == 15
    assert np.abs(lp + math.log(16)).max() < 1e-6 and len(set(lp.tolist())) == 1
    a, lp = run('peak')                                     # one logit 200 above the rest: always it, logp = 0
    assert (a == 11).all() and (lp == 0).all()
    a, lp = run('tie')                                      # a tie for the maximum: greedy takes the lowest index
    ad, lpd = run('tie', det=1)
    assert (ad == 1).all() and len(set(lpd.tolist())) == 1
    p = softmax64(rows['tie'])
    cum = np.cumsum(p)
    want = np.searchsorted(cum, u, side='right')
    assert np.array_equal(a, want) and {1, 3} <= set(a.tolist())
    assert np.array_equal(lp[a == 1], lp[a == 1][:1].repeat((a == 1).sum())) and lp[a == 1][0] == lp[a == 3][0]
    # u = 1 - 2^-24, the largest: u S < S = the final c (the same sequential sum), so a finite row still finds its index --
    # the last with a non-zero e_a; the fallback (the greedy index) is reached by non-finite logits alone
    for name in ('equal', 'tie'):
        a, _ = run(name)
        last = int(np.flatnonzero(np.exp(rows[name].astype(np.float64) - rows[name].max()) > 0).max())
        assert a[-1] == last, name
    for name, g in (('nan', 3), ('nan_first', 0), ('inf', 1)):   # non-finite logits: the index stays in range (the greedy one)
        a, lp = run(name)
        assert (a == g).all(), name
        a, lp = run(name, det=1)
        assert (a == g).all(), name


def gae_case(gamma, lam, T=33, N=257, seed=0):
    """a record with dones at t = 0 and t = T - 1, a Timeout at each, and other ends in between"""
    rs = np.random.RandomState(seed)
    reward = rs.uniform(-1, 1, (T, N)).astype(np.float32)
    value = rs.normal(0, 1, (T, N)).astype(np.float32)
    last = rs.normal(0, 1, N).astype(np.float32)
    tval = rs.normal(0, 1, (T, N)).astype(np.float32)
    done = (rs.uniform(size=(T, N)) < 0.08).astype(np.uint8)
    result = np.where(done != 0, rs.randint(1, 4, (T, N)), 0).astype(np.uint8)
    for t, i, r in ((0, 0, 3), (0, 1, 1), (T - 1, 2, 3), (T - 1, 3, 2), (0, 4, 3), (T - 1, 4, 3)):
        done[t, i], result[t, i] = 1, r
    assert (result[0] == 3).any() and (result[T - 1] == 3).any()
    return reward, done, value, last, result, tval


def gae_float64(reward, done, value, last, gamma, lam, result=None, tval=None):
    """SB3's RolloutBuffer.compute_returns_and_advantage (with collect_rollouts' time-limit bootstrap of the reward) in float64"""
    r = reward.astype(np.float64).copy()
    v = value.astype(np.float64)
    if result is not None:
        r += np.where(result == 3, gamma * tval.astype(np.float64), 0.0)
    T = r.shape[0]
    adv = np.zeros_like(r)
    last_gae = 0.0
    for t in reversed(range(T)):
        next_values = last.astype(np.float64) if t == T - 1 else v[t + 1]
        nnt = 1.0 - (done[t] != 0)
        delta = r[t] + gamma * next_values * nnt - v[t]
        last_gae = delta + gamma * lam * nnt * last_gae
        adv[t] = last_gae
    return adv, adv + v


GAE_TOL = 4 * 1.7e-6


@pytest.mark.parametrize('gamma,lam', [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0)])
@pytest.mark.parametrize('timeouts', [True, False])
def test_gae_against_float64_sb3(ref, gamma, lam, timeouts):
    """T = 33, N = 257, rewards in [-1, 1], values N(0, 1).  Measured maximum absolute difference of advantage and return over
    the three (gamma, lam) and both forms: 1.4e-6 (0.99, 0.95), 1.7e-6 (1, 1: 33 steps accumulate), 4.2e-7 (0.9, 0); allowed:
    4 x 1.7e-6."""
    reward, done, value, last, result, tval = gae_case(gamma, lam)
    kw = dict(result=result, terminal_value=tval) if timeouts else {}
    adv, ret = P.gae(ref, reward, done, value, last, gamma, lam, **kw)
    a64, r64 = gae_float64(reward, done, value, last, gamma, lam, *((result, tval) if timeouts else ()))
    err = max(np.abs(adv - a64).max(), np.abs(ret - r64).max())
    print(f'gamma={gamma} lam={lam} timeouts={timeouts}: max |gae - float64| = {err:.3e}')
    assert err <= GAE_TOL
    if timeouts:
        plain, _ = P.gae(ref, reward, done, value, last, gamma, lam)
        assert (plain != adv)[result == 3].all()          # the bootstrap reaches every Timeout


def _mlp(act, h1=32, h2=48, a=16, extra=None):
    torch = pytest.importorskip('torch')
    nn = torch.nn
    layers = [nn.Linear(10, h1), act(), nn.Linear(h1, h2), act(), nn.Linear(h2, a)]
    return nn.Sequential(*(layers + ([extra] if extra else [])))


def test_from_module_accepted_and_refused_forms():
    torch = pytest.importorskip('torch')
    nn = torch.nn
    from soccer2d_amd.actor import StochasticActor
    for act, name in ((nn.ReLU, 'relu'), (nn.Tanh, 'tanh')):
        net = _mlp(act)
        actor = StochasticActor.from_module(net, device='cpu')
        assert (actor.hidden1, actor.hidden2, actor.n_out, actor.activation) == (32, 48, 16, name)
        assert torch.equal(actor.params, torch.cat([p.detach().reshape(-1) for p in net.parameters()]))
        assert actor.c_struct().activation == (name == 'tanh')
    # a leading Flatten / Identity is skipped
    StochasticActor.from_module(nn.Sequential(nn.Flatten(), nn.Identity(), _mlp(nn.Tanh)), device='cpu')
    # SB3's pair: mlp_extractor.policy_net (Linear-Tanh-Linear-Tanh) + action_net (Linear), with policy.log_std
    trunk = nn.Sequential(nn.Linear(10, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh())
    action_net, log_std = nn.Linear(64, 4), nn.Parameter(torch.full((4,), -0.5))
    actor = StochasticActor.from_module([trunk, action_net], log_std=log_std, device='cpu')
    assert (actor.hidden1, actor.hidden2, actor.n_out, actor.activation) == (64, 64, 4, 'tanh')
    assert torch.equal(actor.log_std, torch.full((4,), -0.5))
    with torch.no_grad():
        log_std.fill_(0.25); action_net.bias.fill_(3.0)
    actor.sync()                                             # reads the module and the log_std parameter again
    assert torch.equal(actor.log_std, torch.full((4,), 0.25)) and torch.equal(actor.params[-4:], torch.full((4,), 3.0))
    snap = actor.snapshot(deterministic=True)
    with torch.no_grad():
        action_net.bias.fill_(-1.0)
    actor.sync()
    assert torch.equal(snap.params[-4:], torch.full((4,), 3.0)) and snap.deterministic and not actor.deterministic
    actor.log_std = [0.1, 0.2, 0.3, 0.4]
    assert torch.allclose(actor.log_std, torch.tensor([0.1, 0.2, 0.3, 0.4]))
    actor.deterministic = True
    assert int(actor.deterministic_tensor[0]) == 1
    refused = [nn.Sequential(nn.Linear(10, 32), nn.ReLU(), nn.Linear(32, 32), nn.Tanh(), nn.Linear(32, 4)),       # mixed
               _mlp(nn.ELU), _mlp(nn.Sigmoid),                                                                   # another activation
               _mlp(nn.Tanh, extra=nn.Tanh()),                                                                   # a squashed output
               nn.Sequential(nn.Linear(10, 32), nn.Linear(32, 32), nn.Linear(32, 4)),                            # no activation
               nn.Sequential(nn.Linear(10, 32), nn.Tanh(), nn.Linear(32, 4)),                                    # one hidden layer
               [trunk], _mlp(nn.Tanh, h1=40), _mlp(nn.Tanh, a=65),
               nn.Sequential(nn.Linear(12, 32), nn.Tanh(), nn.Linear(32, 32), nn.Tanh(), nn.Linear(32, 4))]      # not 10 inputs
    for bad in refused:
        with pytest.raises(ValueError):
            StochasticActor.from_module(bad, device='cpu')
    with pytest.raises(ValueError):
        StochasticActor.from_module([trunk, action_net], log_std=torch.zeros(3), device='cpu')
    with pytest.raises(ValueError):
        StochasticActor(64, 64, 4, activation='gelu', device='cpu')
    with pytest.raises(ValueError):
        StochasticActor(64, 64, 4, activation='relu', device='cpu').load_from([trunk, action_net])
