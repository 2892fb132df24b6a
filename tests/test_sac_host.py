"""CPU checks of Soft Actor-Critic's collection and target (s2d_rollout_sac / s2d_td_target_sac, soccer2d_amd.wide_actor.
SquashedGaussianActor, soccer2d_amd.td.SacTarget): the host restatement of the squashed-Gaussian head (tests/sac_ref.c) bit for bit
on hand-written edge rows, the accuracy of its logp against float64 with torch's own fp32 error as the yardstick, the moments of
the target's z stream, the Python layer without a GPU, and the C ABI's refusals that need no device."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import sac_ref as S
import td as TD

torch = pytest.importorskip('torch')
nn = torch.nn
F = np.float32
_ACT = {'relu': nn.ReLU, 'tanh': nn.Tanh, 'sigmoid': nn.Sigmoid}


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return S.build(tmp_path_factory.mktemp('sac_ref'))


# ------------------------------------------------------------------------------------------------------------------ the head
def _round_f32(fr):
    """the float32 nearest to the non-negative Fraction fr (ties to even; normal range)"""
    if fr == 0:
        return F(0.0)
    e = math.floor(math.log2(fr)) - 23
    while fr / Fraction(2) ** e >= 2 ** 24:
        e += 1
    while fr / Fraction(2) ** e < 2 ** 23:
        e -= 1
    q = fr / Fraction(2) ** e
    n = math.floor(q)
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    return F(float(Fraction(n) * Fraction(2) ** e))


def _expected(ref, a, gauss):
    """logp of one dimension from its squashed action a and its Gaussian part: gauss - log_spec(fmaf(-a, a, 1) + 1e-6f), with
    the fmaf rounded once from the exact value"""
    one_minus = _round_f32(Fraction(1) - Fraction(float(a)) ** 2)
    return F(gauss - S.log_spec(ref, [F(one_minus + F(1e-6))])[0])


HALF_LOG_2PI = F(0.91893853)


def test_head_edge_rows_bitwise(ref):
    """the clamp of the raw log-std (-25, -20, 2, 3, NaN), a = +-1 exactly (the log's argument is exactly 1e-6f), z = 0 sampled
    and deterministic, and -0 means, against expectations written out by hand from tanh_spec / log_spec alone"""
    nan = F(np.nan)
    # (mean, raw log-std, z, det) -> (a, the Gaussian part of logp); z = 0 keeps sigma out of u, so exp_spec is not needed here
    rows = []
    for v, ls in ((-25.0, -20.0), (-20.0, -20.0), (2.0, 2.0), (3.0, 2.0), (nan, -20.0), (-19.999, F(-19.999)), (1.5, 1.5)):
        mean = F(0.3)
        a = S.tanh_spec(ref, [mean])[0]
        rows.append((mean, F(v), F(0.0), 0, a, F(F(-F(ls)) - HALF_LOG_2PI)))
    # sigma = exp_spec(0) = 1 exactly: u = 0.25 + 0.5 = 0.75; the Gaussian part is (-(0.5 * 0.5) * 0.5 - 0) - 0.91893853
    rows.append((F(0.25), F(0.0), F(0.5), 0, S.tanh_spec(ref, [F(0.75)])[0], F(F(-0.125) - HALF_LOG_2PI)))
    # the same row deterministic: z is ignored, u = the mean
    rows.append((F(0.25), F(0.0), F(0.5), 1, S.tanh_spec(ref, [F(0.25)])[0], F(F(-0.0) - HALF_LOG_2PI)))
    # |u| > 9: a = +-1 exactly, the log's argument exactly 1e-6f
    for mean, z, det in ((10.0, 0.0, 0), (-10.0, 0.0, 1), (1.0, 9.5, 0), (-1.0, -9.5, 0)):
        g = F(fma32(F(-0.5) * F(z), F(z), F(-0.0)) - HALF_LOG_2PI) if not det else F(F(-0.0) - HALF_LOG_2PI)
        rows.append((F(mean), F(0.0), F(z), det, F(math.copysign(1.0, mean)), g))
    # -0 means: deterministic keeps the sign (u = the mean itself), sampling with z = 0 gives fmaf(sigma, +0, -0) = +0
    rows.append((F(-0.0), F(-1.0), F(0.0), 1, F(-0.0), F(F(1.0) - HALF_LOG_2PI)))
    rows.append((F(-0.0), F(-1.0), F(0.0), 0, F(0.0), F(F(1.0) - HALF_LOG_2PI)))
    rows.append((F(0.0), F(-1.0), F(-0.0), 0, F(0.0), F(F(1.0) - HALF_LOG_2PI)))
    for mean, v, z, det, a_want, gauss in rows:
        a = C.c_float()
        lp = F(ref.sac_term(mean, v, z, det, C.byref(a)))
        what = (mean, v, z, det)
        assert S.bits(a.value) == S.bits(a_want), (what, a.value, a_want)
        want = _expected(ref, a_want, gauss)
        assert S.bits(lp) == S.bits(want), (what, lp, want)
        if abs(float(a_want)) == 1.0:
            assert S.bits(lp) == S.bits(F(gauss - S.log_spec(ref, [F(1e-6)])[0]))
    # the sum over dimensions: t_0 + t_1 + t_2 + t_3 in ascending order
    y = np.array([[0.3, -0.7, 1.1, -0.0, -25.0, 3.0, np.nan, 0.0]], F)
    z = np.array([[0.0, 0.0, 0.0, 0.0]], F)
    a, lp = S.head(ref, y, z, 0)
    t = [F(ref.sac_term(y[0, j], y[0, 4 + j], F(0.0), 0, C.byref(C.c_float()))) for j in range(4)]
    assert S.bits(lp[0]) == S.bits(F(F(F(t[0] + t[1]) + t[2]) + t[3]))
    assert np.array_equal(S.bits(a[0]), S.bits(S.tanh_spec(ref, [0.3, -0.7, 1.1, 0.0])))


def fma32(a, b, c):
    """fmaf on float32 values through exact rationals (one rounding)"""
    fr = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    return -_round_f32(-fr) if fr < 0 else (_round_f32(fr) if fr > 0 else F(float(a) * float(b) + float(c)))


def _logp_grid():
    """the stated grid: mean = -2 + 0.1 i (i = 0 .. 40), raw log-std in {-5, -3, -1.5, -0.5, 0, 0.5}, z = -3 + 0.25 i (i = 0 .. 24),
    kept where |mean + exp(log_std) z| <= 3 in float64"""
    mean, ls, z = np.meshgrid(-2 + 0.1 * np.arange(41), [-5.0, -3.0, -1.5, -0.5, 0.0, 0.5], -3 + 0.25 * np.arange(25), indexing='ij')
    mean, ls, z = (v.reshape(-1).astype(F) for v in (mean, ls, z))
    keep = np.abs(mean.astype(np.float64) + np.exp(ls.astype(np.float64)) * z.astype(np.float64)) <= 3.0
    return mean[keep], ls[keep], z[keep]


def _sb3_logp(mean, log_std, z):
    """SB3's SquashedDiagGaussianDistribution.log_prob of the action sampled with noise z, in the tensors' dtype"""
    std = log_std.exp()
    u = mean + std * z
    return torch.distributions.Normal(mean, std).log_prob(u) - torch.log(1 - torch.tanh(u) ** 2 + 1e-6)


def test_logp_accuracy_against_float64(ref):
    """On the grid of _logp_grid() (5 478 points, |u| <= 3) the restated head's logp against a float64 evaluation of SB3's formula
    from the same (y, z).  Yardstick: torch's own fp32 evaluation of that formula against the same float64; the restatement's
    largest error may be at most twice torch's.  Measured: restatement 5.98e-06, torch fp32 4.46e-05 (its (u - mean) / std
    cancels at the small standard deviations)."""
    mean, ls, z = _logp_grid()
    assert mean.size > 4000
    y = np.stack([mean, ls], axis=1)
    _, lp = S.head(ref, y, z[:, None], 0)
    t = [torch.from_numpy(v) for v in (mean, ls, z)]
    want64 = _sb3_logp(*(v.double() for v in t)).numpy()
    torch32 = _sb3_logp(*t).numpy()
    err = np.abs(lp.astype(np.float64) - want64).max()
    torch_err = np.abs(torch32.astype(np.float64) - want64).max()
    print(f'logp on {mean.size} points: restatement {err:.3g}, torch fp32 {torch_err:.3g}')
    assert err <= 2.0 * torch_err, (err, torch_err)


def test_td_stream_z_moments(ref):
    """the target's z over 2^16 rows x 8: |mean| <= 5 / sqrt(n), |var - 1| <= 5 sqrt(2 / n)"""
    z = S.td_z(ref, 1 << 16, 8, 0x5EED, 3).astype(np.float64)
    n = z.size
    assert n == 1 << 19 and np.isfinite(z).all()
    assert abs(z.mean()) <= 5 / math.sqrt(n), z.mean()
    assert abs(z.var() - 1) <= 5 * math.sqrt(2 / n), z.var()
    # another call draws other noise; A <= 4 reads the first block only
    assert not np.array_equal(z[:, :4], S.td_z(ref, 1 << 16, 4, 0x5EED, 4))
    assert np.array_equal(z[:, :4].astype(F), S.td_z(ref, 1 << 16, 4, 0x5EED, 3))


def test_rollout_z_is_the_policy_rollouts_gaussian_block(ref):
    """continuous: z_{k & 3} of the block at counter k >> 2; turning: the four of the block at counter k (actor_ref.c's block)"""
    n, seed = 50, 0xABCDEF0123
    k = np.arange(n) + 2 ** 32 - 20
    gid = np.arange(n, dtype=np.uint64) + 7
    zt = S.rollout_z(ref, 'turn4', n, seed, k, gid0=7)
    zc = S.rollout_z(ref, 'cont1', n, seed, k, gid0=7)
    want = np.zeros((n, 4), F)
    ctr = np.ascontiguousarray(k & 0xFFFFFFFF, dtype=np.uint32)
    ref.actor_gauss.restype, ref.actor_gauss.argtypes = None, [C.c_int64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    ref.actor_gauss(n, seed, gid.ctypes.data, ctr.ctypes.data, want.ctypes.data)
    assert np.array_equal(S.bits(zt), S.bits(want))
    c4 = np.ascontiguousarray(ctr >> 2)
    ref.actor_gauss(n, seed, gid.ctypes.data, c4.ctypes.data, want.ctypes.data)
    assert np.array_equal(S.bits(zc[:, 0]), S.bits(want[np.arange(n), ctr & 3]))


# ------------------------------------------------------------------------------------------------------------ the Python layer
def _latent(n_in, hidden, act='relu'):
    layers, win = [], n_in
    for w in hidden:
        layers += [nn.Linear(win, w), _ACT[act]()]
        win = w
    return nn.Sequential(*layers)


def _stacked(latent, mu, log_std):
    head = nn.Linear(mu.in_features, 2 * mu.out_features)
    with torch.no_grad():
        head.weight.copy_(torch.cat([mu.weight, log_std.weight]))
        head.bias.copy_(torch.cat([mu.bias, log_std.bias]))
    return nn.Sequential(*latent, head)


@pytest.mark.parametrize('A', [1, 4])
def test_module_readers_give_the_same_flat_buffer(A):
    from soccer2d_amd.td import SacTarget
    from soccer2d_amd.wide_actor import SquashedGaussianActor, param_count, wide_plan
    torch.manual_seed(A)
    latent, mu, ls = _latent(10, (20, 12), 'tanh'), nn.Linear(12, A), nn.Linear(12, A)
    full = _stacked(latent, mu, ls)
    a = SquashedGaussianActor.from_modules(latent, mu, ls, device='cpu')
    b = SquashedGaussianActor.from_module(full, device='cpu', deterministic=True)
    assert (a.hidden, a.action_dim, a.n_out, a.activation) == ((20, 12), A, 2 * A, 'tanh')
    assert a.params.numel() == param_count((20, 12), 2 * A) and torch.equal(a.params, b.params)
    lin = [m for m in full if isinstance(m, nn.Linear)]
    flat = torch.cat([torch.cat([l.weight.detach().reshape(-1), l.bias.detach()]) for l in lin])
    assert torch.equal(a.params, flat)                                       # nn.Sequential order of the stacked network
    assert (a.deterministic, b.deterministic) == (False, True) and int(b.deterministic_tensor[0]) == 1
    b.deterministic = False
    assert int(b.deterministic_tensor[0]) == 0
    assert a.workspace.numel() * 4 == wide_plan((20, 12), 2 * A)[3]
    net = a.c_struct()
    assert (net.n_hidden, list(net.hidden), net.n_out, net.activation, net.noise_kind) == (2, [20, 12, 0, 0, 0], 2 * A, 1, 0)
    assert net.epsilon is None and net.noise is None and net.params == a.params.data_ptr() and net.workspace == a.workspace.data_ptr()
    # sync() rereads in place; a snapshot does not follow
    snap, ptr = a.snapshot(deterministic=True), a.params.data_ptr()
    with torch.no_grad():
        ls.bias.add_(1.0)
    assert a.sync() is a and a.params.data_ptr() == ptr
    assert torch.equal(a.params[-A:], ls.bias.detach()) and not torch.equal(a.params, snap.params) and snap.deterministic
    # the target's actor reads both forms too, at any input width
    q = nn.Sequential(nn.Linear(10 + A, 16), nn.ReLU(), nn.Linear(16, 1))
    t1, t2 = SacTarget((latent, mu, ls), q, q, device='cpu'), SacTarget.from_modules(_stacked(latent, mu, ls), q, device='cpu')
    assert torch.equal(t1.actor.params, t2.actor.params) and torch.equal(t1.actor.params, a.params)
    assert (t1.action_dim, t1.obs_dim, len(t1.critics), len(t2.critics)) == (A, 10, 2, 1)
    assert t1.draws.dtype == torch.int64 and int(t1.draws[0]) == 0
    wide = SacTarget((_latent(224, (64, 64)), nn.Linear(64, 8), nn.Linear(64, 8)),
                     nn.Sequential(nn.Linear(232, 8), nn.ReLU(), nn.Linear(8, 1)), device='cpu')
    assert (wide.obs_dim, wide.action_dim) == (224, 8)


def test_refusals_of_the_python_layer(monkeypatch):
    from soccer2d_amd import _capi
    from soccer2d_amd.td import SacTarget
    from soccer2d_amd.wide_actor import SquashedGaussianActor

    def boom(*a, **k):
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_capi, 'load_library', boom)
    lat = _latent(10, (16, 8))
    with pytest.raises(ValueError, match='2 A outputs'):                     # an odd output width
        SquashedGaussianActor.from_module(nn.Sequential(*lat, nn.Linear(8, 3)), device='cpu')
    with pytest.raises(ValueError, match='2 A outputs'):                     # A = 2 is no engine's
        SquashedGaussianActor.from_module(nn.Sequential(*lat, nn.Linear(8, 4)), device='cpu')
    with pytest.raises(ValueError, match='one activation'):                  # a mix
        SquashedGaussianActor.from_module(nn.Sequential(nn.Linear(10, 8), nn.ReLU(), nn.Linear(8, 8), nn.Tanh(), nn.Linear(8, 2)),
                                          device='cpu')
    with pytest.raises(ValueError, match='multiple of 4'):                   # the wide reader's texts
        SquashedGaussianActor.from_modules(_latent(10, (16, 10)), nn.Linear(10, 1), nn.Linear(10, 1), device='cpu')
    with pytest.raises(ValueError, match='multiple of 4'):
        SquashedGaussianActor((404,), 1, device='cpu')
    with pytest.raises(ValueError, match='hidden layers'):
        SquashedGaussianActor.from_module(nn.Sequential(*_latent(10, (8,) * 6), nn.Linear(8, 2)), device='cpu')
    with pytest.raises(ValueError, match='log_std must be a Linear'):
        SquashedGaussianActor.from_modules(lat, nn.Linear(8, 4), nn.Linear(8, 1), device='cpu')
    with pytest.raises(ValueError, match='action_dim'):
        SquashedGaussianActor((16,), 2, device='cpu')
    with pytest.raises(ValueError, match='observation'):
        SquashedGaussianActor.from_module(nn.Sequential(*_latent(11, (8,)), nn.Linear(8, 2)), device='cpu')
    actor = nn.Sequential(*lat, nn.Linear(8, 8))
    critic = lambda n_in, n_out=1: nn.Sequential(nn.Linear(n_in, 8), nn.ReLU(), nn.Linear(8, n_out))
    with pytest.raises(ValueError, match='obs_dim \\+ A'):                   # a critic's n_in is D + A, not D + 2A
        SacTarget(actor, critic(18), device='cpu')
    with pytest.raises(ValueError, match='critic 2'):
        SacTarget(actor, critic(14), critic(13), device='cpu')
    with pytest.raises(ValueError, match='obs_dim \\+ A'):
        SacTarget(actor, critic(14, 2), device='cpu')
    with pytest.raises(ValueError, match='2 A'):
        SacTarget(nn.Sequential(*lat, nn.Linear(8, 5)), critic(12), device='cpu')
    with pytest.raises(ValueError, match='2 A'):
        SacTarget(nn.Sequential(*lat, nn.Linear(8, 18)), critic(19), device='cpu')
    with pytest.raises(ValueError, match='torch.nn.Module'):
        SacTarget((lat, nn.Linear(8, 1)), critic(11), device='cpu')
    t = SacTarget(actor, critic(14), critic(14), seed=5, device='cpu')
    B = 3
    good = {'next_obs': torch.zeros(B, 10), 'reward': torch.zeros(B), 'discount': torch.zeros(B)}
    with pytest.raises(ValueError, match='no CPU path'):
        t.target(good, 0.2)
    with pytest.raises(ValueError, match='no CPU path'):
        t.target(good, torch.tensor([0.2]), return_q=True)
    with pytest.raises(ValueError, match='four'):
        t.target(good, 0.2, out=(torch.zeros(B), torch.zeros(B), torch.zeros(B, 4)), return_q=True)
    with pytest.raises(ValueError, match=r'out\[2\]'):
        t.target(good, 0.2, out=(torch.zeros(B), torch.zeros(B), torch.zeros(B, 8), torch.zeros(B)), return_q=True)
    with pytest.raises(ValueError, match='next_obs'):
        t.target(dict(good, next_obs=torch.zeros(B, 14)), 0.2)


# -------------------------------------------------------------------------------------------------------------------- the C ABI
def test_prototypes_are_bound_and_exported():
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi
    protos = {p[0]: p for p in _capi.PROTOTYPES}
    assert protos['s2d_rollout_sac'][1] is C.c_int and len(protos['s2d_rollout_sac'][2]) == 8
    assert protos['s2d_td_target_sac'][1] is C.c_int and len(protos['s2d_td_target_sac'][2]) == 15
    assert len(protos['s2d_debug_td_target_sac'][2]) == 16
    lib = _capi.load_library()
    for name in ('s2d_rollout_sac', 's2d_td_target_sac', 's2d_debug_td_target_sac'):
        assert hasattr(lib, name), name


def test_c_abi_refusals_that_need_no_device():
    """s2d_td_target_sac checks everything before its first HIP call: every refusal is S2D_EINVAL with the field named (the
    pointers are never read: made-up addresses do).  s2d_rollout_sac needs an engine for all but the NULL handle."""
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi
    from soccer2d_amd.td import td_workspace_bytes
    lib = _capi.load_library()
    net = _capi.S2DWideNet()
    assert lib.s2d_rollout_sac(None, 4, C.byref(net), None, None, None, None, None) == _capi.S2D_EINVAL
    assert b'NULL handle' in lib.s2d_last_error()

    def tdnet(n_in, hidden, n_out, base):
        s = _capi.S2DTdNet()
        s.n_in, s.n_hidden, s.n_out = n_in, len(hidden), n_out
        for l, w in enumerate(hidden):
            s.hidden[l] = w
        s.params, s.workspace = base, base + 0x100000
        s.workspace_bytes = td_workspace_bytes(n_in, hidden, n_out)
        return s
    D, A, B = 10, 4, 100
    arr = {k: 0x40000000 + 0x10000 * i for i, k in enumerate(('next_obs', 'reward', 'discount', 'alpha', 'draws', 'out_target', 'out_q',
                                                               'out_action', 'out_logp'))}

    def call(actor=None, c1=None, c2=None, batch=B, null_c2=False, **over):
        actor = actor or tdnet(D, (16, 8), 2 * A, 0x10000000)
        c1 = c1 or tdnet(D + A, (8,), 1, 0x20000000)
        c2 = c2 or tdnet(D + A, (8,), 1, 0x30000000)
        p = dict(arr, **over)
        rc = lib.s2d_td_target_sac(batch, C.byref(actor) if actor != 'null' else None, C.byref(c1), None if null_c2 else C.byref(c2),
                                   p['next_obs'], p['reward'], p['discount'], p['alpha'], p['draws'], 7, p['out_target'], p['out_q'],
                                   p['out_action'], p['out_logp'], None)
        return rc, lib.s2d_last_error().decode()

    def refused(what, needle, **kw):
        rc, text = call(**kw)
        assert rc == _capi.S2D_EINVAL, (what, rc)
        assert 's2d_td_target_sac' in text and needle in text, (what, text)
    refused('actor NULL', 'actor', actor='null')
    refused('odd n_out', 'n_out', actor=tdnet(D, (16, 8), 7, 0x10000000), c1=tdnet(D + 3, (8,), 1, 0x20000000))
    refused('n_out 18', 'n_out', actor=tdnet(D, (16, 8), 18, 0x10000000))
    refused('critic n_in = D + 2A', 'critic1', c1=tdnet(D + 2 * A, (8,), 1, 0x20000000))
    refused('critic2 n_in', 'critic2', c2=tdnet(D + A + 1, (8,), 1, 0x30000000))
    refused('critic n_out', 'critic1', c1=tdnet(D + A, (8,), 2, 0x20000000))
    refused('width off the grid', 'hidden', actor=tdnet(D, (16, 10), 2 * A, 0x10000000))
    refused('n_in', 'n_in', actor=tdnet(257, (16,), 2 * A, 0x10000000))
    bad = tdnet(D, (16, 8), 2 * A, 0x10000000); bad.activation = 3
    refused('activation', 'activation', actor=bad)
    bad = tdnet(D, (16, 8), 2 * A, 0x10000000); bad.params = None
    refused('params NULL', 'params', actor=bad)
    bad = tdnet(D, (16, 8), 2 * A, 0x10000000); bad.params += 4
    refused('params misaligned', 'params', actor=bad)
    bad = tdnet(D, (16, 8), 2 * A, 0x10000000); bad.workspace = None
    refused('workspace NULL', 'workspace', actor=bad)
    bad = tdnet(D + A, (8,), 1, 0x20000000); bad.workspace_bytes -= 4
    refused('workspace small', 'workspace', c1=bad)
    shared = tdnet(D + A, (8,), 1, 0x20000000)
    refused('shared workspace', 'share', c2=shared)
    refused('batch 0', 'batch', batch=0)
    refused('batch 2^31', 'batch', batch=2 ** 31)
    for name in ('next_obs', 'reward', 'discount', 'out_target'):
        refused(name + ' NULL', name, **{name: None})
        refused(name + ' misaligned', name, **{name: arr[name] + 2})
    for name in ('out_q', 'out_action', 'out_logp'):
        refused(name + ' misaligned', 'optional', **{name: arr[name] + 1})
    refused('alpha NULL', 'alpha', alpha=None)
    refused('alpha misaligned', 'alpha', alpha=arr['alpha'] + 2)
    refused('draws NULL', 'draws', draws=None)
    refused('draws misaligned', 'draws', draws=arr['draws'] + 4)
    refused('draws in out_target', 'draws', draws=arr['out_target'] + 8)
    refused('draws in out_action', 'draws', draws=arr['out_action'] + 4 * (B * A - 2))
    refused('draws in out_logp', 'draws', draws=arr['out_logp'] + 4 * (B - 2))
    refused('draws in out_q', 'draws', draws=arr['out_q'])
