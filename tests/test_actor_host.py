"""CPU checks of the fused tanh actor's host side (s2d_rollout_actor): the restatement of its math spec (tests/actor_ref.c) --
tanh_spec, log_spec and the Box-Muller draw -- against float64, its forward pass, DeterministicActor packing and module
validation, and the S2DActorNet / export ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
import actor_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip('torch')
P_TAIL = 1e-6


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return R.build(tmp_path_factory.mktemp('actor_ref'))


def f32(v):
    return np.float32(v)


def test_tanh_spec(ref):
    x = np.concatenate([np.linspace(-12, 12, 400001, dtype=np.float32),
                        np.float32(2.0) ** -np.arange(1, 140, dtype=np.float32)])
    t = R.tanh(ref, x)
    assert np.abs(t.astype(np.float64) - np.tanh(x.astype(np.float64))).max() <= 1e-6
    assert np.array_equal(R.tanh(ref, -x).view(np.int32), (-t).view(np.int32))          # odd, bit for bit
    s = np.sort(x)
    assert (np.diff(R.tanh(ref, s)) >= 0).all()                                          # monotone
    edge = np.array([0.0, -0.0, np.nextafter(f32(0.625), f32(0)), f32(0.625), np.nextafter(f32(0.625), f32(1)), 9.0, -9.0,
                     np.nextafter(f32(9), f32(10)), 20.0, -1e30, np.inf, -np.inf, np.nan], dtype=np.float32)
    e = R.tanh(ref, edge)
    assert e[0] == 0 and not np.signbit(e[0]) and e[1] == 0 and np.signbit(e[1])
    assert np.abs(e[2:5].astype(np.float64) - np.tanh(edge[2:5].astype(np.float64))).max() <= 1e-6
    assert e[2] <= e[3] <= e[4]
    assert abs(e[5] - np.tanh(9.0)) <= 1e-6 and e[6] == -e[5]
    assert e[7:].tolist()[:5] == [1.0, 1.0, -1.0, 1.0, -1.0] and np.isnan(e[12])          # |y| > 9: +-1 exactly


def test_log_spec(ref):
    # (0, 1]: every float of [2^-24, 1] on a dense grid plus powers of two down to the smallest normal; error within 2 ulp of
    # the result, and 1e-7 absolute near ln 1 = 0
    u = np.unique(np.concatenate([np.linspace(2.0 ** -24, 1.0, 1 << 20).astype(np.float32),
                                  (np.arange(1, 1 << 16) * 2.0 ** -24).astype(np.float32),
                                  np.float32(2.0) ** -np.arange(0, 126, dtype=np.float32)]))
    got = R.log(ref, u).astype(np.float64)
    want = np.log(u.astype(np.float64))
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert (np.abs(got - want) <= np.maximum(2 * ulp, 1e-7)).all()
    assert R.log(ref, [1.0])[0] == 0.0
    sp = R.log(ref, [0.0, -1.0, np.nan, np.inf])
    assert sp[0] == -np.inf and np.isnan(sp[1]) and np.isnan(sp[2]) and sp[3] == np.inf


def chi2_phi(z, bins=64):
    """chi-square of Phi(z) in `bins` equal-probability bins and its 1 - P_TAIL limit"""
    from scipy.special import ndtr
    from scipy.stats import chi2
    h = np.bincount(np.minimum((ndtr(z.astype(np.float64)) * bins).astype(np.int64), bins - 1), minlength=bins)
    e = z.size / bins
    return float(((h - e) ** 2 / e).sum()), float(chi2.ppf(1.0 - P_TAIL, bins - 1))


def test_box_muller_distribution(ref):
    n = 1 << 18
    z = R.gauss(ref, 0x5EED, np.arange(n, dtype=np.uint64) + (7 << 32), 3).reshape(-1)     # 2^20 draws
    assert abs(z.mean()) < 5 * (1 / np.sqrt(z.size))
    assert abs(z.var() - 1) < 5 * np.sqrt(2 / z.size)
    assert np.abs(z).max() <= 5.77
    stat, limit = chi2_phi(z)
    assert stat < limit, (stat, limit)
    # the four words are independent normals: no correlation between z0 and z1 of one block
    zz = z.reshape(n, 4)
    assert abs(np.corrcoef(zz[:, 0], zz[:, 1])[0, 1]) < 5 / np.sqrt(n)


def test_box_muller_uses_block_three_of_the_policy_stream(ref):
    seed, gid, ctr = 0x5EED, 12345, 77
    w = O.philox([gid, 0, ctr, (1 << 16) | 3], [seed, 0])
    u1 = np.float32((w[0] >> 8) + 1) * np.float32(2.0 ** -24)
    r = np.sqrt(-2.0 * np.log(np.float64(u1)))
    deg = np.float64(np.float32(w[1] >> 8) * np.float32(45 * 2.0 ** -21))
    z = R.gauss(ref, seed, [gid], ctr)[0]
    assert abs(z[0] - r * np.cos(np.radians(deg))) < 1e-5 and abs(z[1] - r * np.sin(np.radians(deg))) < 1e-5


def _split(p, h1, h2, na):
    sizes = [10 * h1, h1, h1 * h2, h2, na * h2, na]
    out, o = [], 0
    for s in sizes:
        out.append(p[o:o + s].astype(np.float64)); o += s
    W1, b1, W2, b2, W3, b3 = out
    return W1.reshape(h1, 10), b1, W2.reshape(h2, h1), b2, W3.reshape(na, h2), b3


def test_restatement_matches_a_float64_forward(ref):
    rs = np.random.RandomState(0)
    for h1, h2, na in ((64, 64, 1), (16, 128, 4), (128, 32, 4)):
        n = 10 * h1 + h1 + h1 * h2 + h2 + na * h2 + na
        p = (rs.uniform(-1, 1, n) * 0.3).astype(np.float32)
        x = rs.uniform(-1.5, 1.5, (4000, 10)).astype(np.float32)
        W1, b1, W2, b2, W3, b3 = _split(p, h1, h2, na)
        a64 = np.tanh(np.maximum(np.maximum(x.astype(np.float64) @ W1.T + b1, 0) @ W2.T + b2, 0) @ W3.T + b3)
        a = R.actions(ref, x, p, h1, h2, na, 0.0, 0, None, 1, np.zeros(4000, np.int64))
        assert np.abs(a - a64).max() < 1e-5
        assert np.array_equal(R.tanh(ref, R.forward(ref, x, p, h1, h2, na)), a.reshape(-1))


def test_actions_noise_clip_and_exploration(ref):
    rs = np.random.RandomState(3)
    h1 = h2 = 16
    p = (rs.uniform(-1, 1, 10 * 16 + 16 + 256 + 16 + 4 * 16 + 4) * 0.5).astype(np.float32)
    x = rs.uniform(-1, 1, (5000, 10)).astype(np.float32)
    k = rs.randint(0, 1 << 20, 5000)
    base = R.actions(ref, x, p, h1, h2, 4, 0.0, 0, None, 9, k)
    zero = R.actions(ref, x, p, h1, h2, 4, 0.0, 1, np.zeros((2, 4)), 9, k)
    assert np.array_equal(base, zero)                                       # mu = sigma = 0: kind 0 (values; -0 may turn +0)
    big = R.actions(ref, x, p, h1, h2, 4, 0.0, 1, np.array([[0, 0, 0, 0], [3, 3, 3, 3]]), 9, k)
    assert big.min() == -1.0 and big.max() == 1.0 and (np.abs(big) <= 1).all()
    ex = R.actions(ref, x, p, h1, h2, 4, 1.0, 1, np.array([[0, 0, 0, 0], [3, 3, 3, 3]]), 9, k)
    assert (np.abs(ex) < 1).all() and abs(ex.mean()) < 0.05                 # eps = 1: the uniform random action, no noise


def _mu(h1=64, h2=64, a=1, tanh=True, extra=None, lead=None):
    mods = ([lead] if lead is not None else []) + [torch.nn.Linear(10, h1), torch.nn.ReLU(), torch.nn.Linear(h1, h2),
                                                   torch.nn.ReLU(), torch.nn.Linear(h2, a)]
    if tanh:
        mods.append(torch.nn.Tanh())
    if extra is not None:
        mods += extra
    return torch.nn.Sequential(*mods)


def test_deterministic_actor_packing():
    from soccer2d_amd.actor import DeterministicActor
    torch.manual_seed(0)
    for lead in (None, torch.nn.Flatten(), torch.nn.Identity()):
        mu = _mu(64, 32, 4, lead=lead)
        a = DeterministicActor.from_module(mu, device='cpu', epsilon=0.1, noise_sigma=0.2)
        want = torch.cat([t.detach().reshape(-1) for t in mu.parameters()])
        assert torch.equal(a.params, want)
        assert (a.hidden1, a.hidden2, a.n_out, a.noise_kind) == (64, 32, 4, 1)
        assert torch.equal(a.noise_sigma, torch.full((4,), 0.2)) and torch.equal(a.noise_mean, torch.zeros(4))
    with torch.no_grad():
        mu[1].weight.add_(1.0)
    a.sync()
    assert torch.equal(a.params, torch.cat([t.detach().reshape(-1) for t in mu.parameters()]))
    a.noise_sigma = None
    assert a.noise_kind == 0 and a.c_struct().noise_kind == 0
    a.noise_sigma = [0.1, 0.2, 0.3, 0.4]
    a.noise_mean = 0.5
    assert a.c_struct().noise_kind == 1 and torch.allclose(a.noise_sigma, torch.tensor([0.1, 0.2, 0.3, 0.4]))
    with pytest.raises(ValueError):
        a.noise_sigma = [0.1, 0.2]


def test_deterministic_actor_module_validation():
    from soccer2d_amd.actor import DeterministicActor
    with pytest.raises(ValueError, match='Tanh'):
        DeterministicActor.from_module(_mu(tanh=False), device='cpu')                     # a missing trailing Tanh
    with pytest.raises(ValueError):
        DeterministicActor.from_module(_mu(extra=[torch.nn.Linear(1, 1)]), device='cpu')   # a fourth layer
    bad = _mu()
    bad[1] = torch.nn.Tanh()
    with pytest.raises(ValueError):
        DeterministicActor.from_module(bad, device='cpu')                                   # another activation
    with pytest.raises(ValueError, match='n_out'):
        DeterministicActor.from_module(_mu(a=2), device='cpu')                              # no mode has A = 2
    with pytest.raises(ValueError, match=r'net_arch=\[64, 64\]'):
        DeterministicActor.from_module(_mu(400, 300), device='cpu')                         # SB3's default DDPG net_arch
    a = DeterministicActor(64, 64, 1, device='cpu')
    with pytest.raises(ValueError):
        a.load_from(_mu(64, 64, 4))


def test_struct_and_export_abi():
    from soccer2d_amd import _capi
    assert C.sizeof(_capi.S2DActorNet) == 40
    assert [f[0] for f in _capi.S2DActorNet._fields_] == ['hidden1', 'hidden2', 'n_out', 'noise_kind', 'params', 'epsilon', 'noise']
    hdr = open(os.path.join(ROOT, 'include', 's2d.h')).read()
    assert re.search(r'typedef struct S2DActorNet \{\s*int32_t hidden1, hidden2, n_out, noise_kind;\s*const float \*params;\s*'
                     r'const float \*epsilon;\s*const float \*noise;\s*\} S2DActorNet;', hdr)
    assert re.search(r'int s2d_rollout_actor\(S2DHandle h, int n_steps, const S2DActorNet \*net, const S2DRollout \*out, '
                     r'float \*terminal_obs, void \*stream\);', hdr)
    protos = {p[0]: p for p in _capi.PROTOTYPES}
    assert 's2d_rollout_actor' in protos and len(protos['s2d_rollout_actor'][2]) == 6
    lib = os.path.join(ROOT, 'gym-soccer-2d-env_amd', 'lib', 'libs2d_hip.so')
    if os.path.exists(lib):
        syms = subprocess.run(['nm', '-D', '--defined-only', lib], stdout=subprocess.PIPE, text=True).stdout
        assert re.search(r'\bs2d_rollout_actor\b', syms)


# ------------------------------------------------------------------------------- the contract every packed-parameter actor keeps
def _layers(widths, act=torch.nn.ReLU, tanh=False, bias=True):
    mods = []
    for win, w in zip(widths[:-2], widths[1:-1]):
        mods += [torch.nn.Linear(win, w, bias=bias), act()]
    mods.append(torch.nn.Linear(widths[-2], widths[-1], bias=bias))
    return torch.nn.Sequential(*mods, *([torch.nn.Tanh()] if tanh else []))


_TABLE3 = [[0.0, 0.0, 0.0]] * 3
# class: (module widths, Tanh head, arguments of from_module after the module, does the class's own host test refuse a bias-less Linear)
ACTOR_CLASSES = {
    'actor.QNetActor': ((10, 16, 32, 5), False, {}, False),
    'actor.DeterministicActor': ((10, 16, 32, 4), True, {}, False),
    'actor.StochasticActor': ((10, 16, 32, 5), False, {}, False),
    'actor.MatchQNetActor': ((224, 16, 32, 3), False, dict(table=_TABLE3), False),
    'actor.MatchPolicyActor': ((224, 16, 32, 3), False, dict(table=_TABLE3), True),
    'mlp_actor.MlpQNetActor': ((10, 24, 8, 40, 5), False, {}, True),
    'mlp_actor.MlpDeterministicActor': ((10, 8, 1), True, {}, False),
    'wide_actor.WideQNetActor': ((10, 300, 28, 5), False, {}, True),
    'wide_actor.WideDeterministicActor': ((10, 12, 20, 400, 4), True, {}, False),
}


@pytest.mark.parametrize('name', list(ACTOR_CLASSES))
def test_common_contract_of_the_packed_actors(name):
    """What the nine actor classes share through their base (soccer2d_amd.actor), on device='cpu', where the class's own host
    test does not already check it: sync() without a module raises; a bias-less nn.Linear is refused (MatchPolicyActor,
    MlpQNetActor and WideQNetActor have that in test_match_policy_host.py, test_mlp_actor_host.py and test_wide_actor_host.py;
    the other six, the Tanh-head readers among them, here); sync() after an in-place
    change of the module changes `params` to the module's parameters and keeps the buffer the kernel reads (data_ptr()).
    That from_module packs torch.cat of the parameters, and that snapshot() does not follow later sync() calls, is checked
    for every class that has them in test_{qnet,mlp,wide}_actor_host.py, test_policy_host.py, test_match_{net,policy,two_nets}
    _host.py and test_deterministic_actor_packing above."""
    import importlib
    mod, cls_name = name.split('.')
    cls = getattr(importlib.import_module('soccer2d_amd.' + mod), cls_name)
    widths, tanh, kw, bias_checked = ACTOR_CLASSES[name]
    torch.manual_seed(len(name))
    net = _layers(widths, tanh=tanh)
    a = cls.from_module(net, device='cpu', **kw)
    assert a.device == torch.device('cpu') and a._module is net
    assert a.params.numel() == sum(p.numel() for p in net.parameters()) == sum(int(np.prod(s)) for s in a.shapes())
    # a fresh actor of the same shape has no module
    ctor = dict(device='cpu', **({} if getattr(a, 'activation', None) is None else dict(activation=a.activation)))
    if hasattr(a, 'hidden'):
        fresh = cls(a.hidden, widths[-1], **ctor)
    else:
        fresh = cls(a.hidden1, a.hidden2, widths[-1], **ctor)
    with pytest.raises(ValueError, match='no module loaded'):
        fresh.sync()
    if not bias_checked:
        with pytest.raises(ValueError, match='needs a bias'):
            cls.from_module(_layers(widths, tanh=tanh, bias=False), device='cpu', **kw)
        with pytest.raises(ValueError, match='needs a bias'):
            fresh.load_from(_layers(widths, tanh=tanh, bias=False))
    ptr, before = a.params.data_ptr(), a.params.clone()
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(-0.5).add_(0.25)
    assert torch.equal(a.params, before)                       # nothing moves before sync()
    assert a.sync() is a
    assert not torch.equal(a.params, before)
    assert torch.equal(a.params, torch.cat([p.detach().reshape(-1) for p in net.parameters()]))
    assert a.params.data_ptr() == ptr
