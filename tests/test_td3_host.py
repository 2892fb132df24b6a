"""CPU checks of TD3's target with target-policy smoothing (s2d_td_target_td3, soccer2d_amd.td.Td3Target): the header and the
binding, the host restatement (tests/td3_ref.c) against td_ref.c at sigma = 0 and against float64, the properties of the noise,
and the refusals of the Python class and of the C entry point, none of which needs a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import td as TD
import td3 as T3
from test_td_host import _check_against_f64, _torch_forward, seq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, 'include', 's2d.h')
torch = pytest.importorskip('torch')
nn = torch.nn
F = np.float32
ULP1 = float(np.spacing(F(1.0)))


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return T3.build(tmp_path_factory.mktemp('td3_ref'))


def _case(rs, D, A, pi, qf, act, B):
    actor = TD.random_net(rs, D, pi, A, act)
    c1, c2 = TD.random_net(rs, D + A, qf, 1, act), TD.random_net(rs, D + A, qf, 1, act)
    x = rs.uniform(-1, 1, (B, D)).astype(F)
    r, d = rs.uniform(-1, 1, B).astype(F), np.where(rs.rand(B) < 0.2, 0.0, 0.99).astype(F)
    return actor, c1, c2, x, r, d


# ------------------------------------------------------------------------------------------------------- header and binding
def test_header_and_binding(tmp_path):
    from soccer2d_amd import _capi
    src = re.sub(r'/\*.*?\*/', '', open(HDR).read(), flags=re.S)
    assert re.search(r'^#define\s+S2D_TD3_STREAM\s+15\s*$', src, flags=re.M)
    assert re.search(r'\bint\s+s2d_td_target_td3\s*\(', src)
    # the prototype as the issue states it: assigning the function to a pointer of that type compiles without a diagnostic
    prog = tmp_path / 'td3_abi.c'
    prog.write_text('#include <stdio.h>\n#include "s2d.h"\n'
                    'int (*const f)(int64_t, const S2DTdNet *, const S2DTdNet *, const S2DTdNet *, const float *, const float *,'
                    ' const float *, const float *, uint64_t *, uint64_t, float *, float *, float *, void *) = s2d_td_target_td3;\n'
                    'int main(){printf("%d %d %d\\n", S2D_TD3_STREAM, S2D_TD_STREAM, S2D_ABI_VERSION);return f == 0;}\n')
    obj = tmp_path / 'td3_abi.o'
    subprocess.run(['gcc', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'), '-c', str(prog), '-o', str(obj)], check=True)
    pre = subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), '-E', '-P', str(prog)], check=True, capture_output=True, text=True).stdout
    assert re.search(r'printf\("%d %d %d\\n", 15, 13, 4\)', pre)
    protos = {p[0]: p for p in _capi.PROTOTYPES}
    ret, args = protos['s2d_td_target_td3'][1:]
    N, V = C.POINTER(_capi.S2DTdNet), C.c_void_p
    assert ret is C.c_int and tuple(args) == (C.c_int64, N, N, N, V, V, V, V, V, C.c_uint64, V, V, V, V)
    assert _capi.S2D_ABI_VERSION == 4


def test_symbol_exported():
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi
    lib = _capi.load_library()
    assert hasattr(lib, 's2d_td_target_td3')
    assert lib.s2d_td_target_td3.argtypes[9] is C.c_uint64


# --------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('D', [4, 10])
@pytest.mark.parametrize('A', [1, 4])
def test_sigma_zero_is_the_unsmoothed_target(ref, D, A):
    """sigma = 0: n = +-0, so target, q and (with no -0 action) the action have td_ref.c's bits, single and twin"""
    rs = np.random.RandomState(100 * D + A)
    actor, c1, c2, x, r, d = _case(rs, D, A, (16, 8), (12, 20), 'tanh', 97)
    for twin in (None, c2):
        want = TD.target_ac(ref, actor, c1, twin, x, r, d)
        assert not np.any((want[2] == 0) & np.signbit(want[2]))              # no -0 action: the case the header sets apart
        for clip in (0.5, 0.0, np.inf):
            got = T3.target(ref, actor, c1, twin, x, r, d, 0.0, clip, 5, 0xC0FFEE)
            for g, w in zip(got[:3], want):
                assert np.array_equal(T3.bits(g), T3.bits(w))
            assert np.array_equal(T3.bits(got[3]), T3.bits(want[2]))         # the mean is the unsmoothed action
    assert len(np.unique(want[0])) > 48


F64_CASES = [(10, 1, (64, 64), (64, 64), 'relu', True), (4, 4, (16, 8), (64, 32, 16, 8), 'tanh', False),
             (16, 5, (16, 8), (12, 20), 'sigmoid', True)]


@pytest.mark.parametrize('D,A,pi,qf,act,twin', F64_CASES, ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_target_against_float64(ref, D, A, pi, qf, act, twin):
    """The restatement against the float64 formula clamp(tanh(mu(x)) + clamp(sigma z, -c, c), -1, 1) -> min Q -> r + d q fed the same
    z, by test_td_host's rule (at most 4 x torch-fp32's own error on the same inputs, floored at one ulp).  Rows within 1e-6 of a
    clamp's corner (|sigma z| of clip, |m + n| of 1) may take the other branch in another precision and are left out: at most 1 %."""
    B, sigma, clip, seed, draws = 192, F(0.2), F(0.5), 0xBADC0DE + D, (3 << 32) + 17
    rs = np.random.RandomState(D + A)
    actor, c1, c2, x, r, d = _case(rs, D, A, pi, qf, act, B)
    z = T3.z(ref, B, A, seed, draws)
    t, q, a, m = T3.target(ref, actor, c1, c2 if twin else None, x, r, d, sigma, clip, draws, seed)
    # float64
    pre64, pre32 = TD.forward64(actor, x), _torch_forward(actor, x)
    m64 = np.tanh(pre64)
    p64 = float(sigma) * z.astype(np.float64)
    s64 = m64 + np.clip(p64, -float(clip), float(clip))
    a64 = np.clip(s64, -1.0, 1.0)
    near = (np.abs(np.abs(p64) - float(clip)) < 1e-6) | (np.abs(np.abs(s64) - 1.0) < 1e-6)
    keep = ~near.any(axis=1)
    left_out = B - int(keep.sum())
    print(f'td3 {D}+{A}: {left_out} of {B} rows left out at a clamp corner')
    assert left_out <= B // 100
    # torch fp32 on the same inputs
    a32 = np.clip(np.tanh(pre32) + np.clip(sigma * z, -clip, clip), F(-1), F(1)).astype(F)
    nets = (c1, c2) if twin else (c1,)
    q64 = np.min([TD.forward64(c, np.concatenate([x.astype(np.float64), a64], axis=1))[:, 0] for c in nets], axis=0)
    q32 = np.min([_torch_forward(c, np.concatenate([x, a32], axis=1))[:, 0] for c in nets], axis=0)
    want = r.astype(np.float64) + d.astype(np.float64) * q64
    tt = r + d * q32
    _check_against_f64(f'td3 smoothed {D}+{A} pi{pi} qf{qf} {act}', t[keep], want[keep], tt[keep])
    # the action: tanh_spec's stated error (1e-6) on top of the pre-activation's, one rounding each for the product and the sum
    a_allowed = 1e-6 + 2 * ULP1 + max(4.0 * np.abs(pre32.astype(np.float64) - pre64).max(), float(np.spacing(F(np.abs(pre64).max()))))
    a_err = np.abs(a.astype(np.float64) - a64)[keep].max()
    print(f'action error {a_err:.3g}, allowed {a_allowed:.3g}')
    assert a_err <= a_allowed
    assert np.any(np.abs(p64) > float(clip)) or A == 1                        # the noise clamp is exercised


def test_noise_properties(ref):
    rs = np.random.RandomState(7)
    B, D, A, seed, k = 300, 10, 5, 0x5EED5EED5EED, (9 << 32) + 4
    actor, c1, c2, x, r, d = _case(rs, D, A, (16, 8), (12, 20), 'relu', B)
    actor.params[-A:] += np.array([3.0, -3.0, 0.0, 9.0, -9.0], F)             # means near and at +-1 as well as inside
    # |a' - clamp(m, -1, 1)| <= clip up to one ulp, for small and large sigma
    for sigma, clip in ((0.2, 0.5), (50.0, 0.125), (1e30, 0.3), (0.7, np.inf)):
        t, q, a, m = T3.target(ref, actor, c1, c2, x, r, d, sigma, clip, k, seed)
        dist = np.abs(a.astype(np.float64) - np.clip(m, -1, 1).astype(np.float64))
        assert np.all(np.abs(a) <= 1.0) and np.all(np.abs(m) <= 1.0)
        if np.isfinite(clip):
            assert dist.max() <= float(F(clip)) + ULP1, (sigma, clip, dist.max())
        if sigma >= 50.0:
            assert dist.max() >= float(F(clip)) - ULP1 or np.all(np.abs(a) == 1.0)   # the noise clamp binds
        want = T3.smooth(ref, m, sigma, clip, T3.z(ref, B, A, seed, k))
        assert np.array_equal(T3.bits(a), T3.bits(want))
    # clip = 0: the unsmoothed action (as numbers: -0 + +0 is +0)
    t0, q0, a0, m0 = T3.target(ref, actor, c1, c2, x, r, d, 0.2, 0.0, k, seed)
    assert np.array_equal(a0, m0)
    tu = TD.target_ac(ref, actor, c1, c2, x, r, d)
    assert np.array_equal(a0, tu[2])
    # draws = k and k + 1 (and k + 2^32: the high word) give different noise, the same draws the same
    z = T3.z(ref, B, A, seed, k)
    assert np.array_equal(T3.bits(z), T3.bits(T3.z(ref, B, A, seed, k)))
    for other in (k + 1, k + (1 << 32), k - 1):
        assert not np.any(np.all(z == T3.z(ref, B, A, seed, other), axis=1))
    assert not np.any(np.all(z == T3.z(ref, B, A, seed + 1, k), axis=1))
    assert not np.any(np.all(z == T3.z(ref, B, A, seed + (1 << 32), k), axis=1))
    # row b's noise does not depend on B: the counter is the global row
    assert np.array_equal(T3.bits(T3.z(ref, 50, A, seed, k)), T3.bits(z[:50]))
    assert np.array_equal(T3.bits(T3.z(ref, 10, A, seed, k, row0=140)), T3.bits(z[140:150]))
    ta = T3.target(ref, actor, c1, c2, x[:33], r[:33], d[:33], 0.2, 0.5, k, seed)
    tb = T3.target(ref, actor, c1, c2, x, r, d, 0.2, 0.5, k, seed)
    assert all(np.array_equal(T3.bits(p), T3.bits(q_[:33])) for p, q_ in zip(ta, tb))
    # A <= 4 never draws block 1; block 0 is the same whatever A is
    z8 = T3.z(ref, B, 8, seed, k)
    for n_act in range(1, 9):
        before = T3.blocks(ref)
        zz = T3.z(ref, B, n_act, seed, k)
        assert T3.blocks(ref) - before == B * (2 if n_act > 4 else 1)
        assert np.array_equal(T3.bits(zz), T3.bits(z8[:, :n_act]))
    before = T3.blocks(ref)
    T3.target(ref, TD.random_net(rs, D, (8,), 4, 'relu'), TD.random_net(rs, D + 4, (8,), 1, 'relu'), None, x, r, d, 0.2, 0.5, k, seed)
    assert T3.blocks(ref) - before == B
    # N(0, 1): |mean| <= 5 / sqrt(n), |var - 1| <= 5 sqrt(2 / n)
    zl = T3.z(ref, 1 << 14, 8, seed, k).astype(np.float64)
    assert abs(zl.mean()) <= 5 / np.sqrt(zl.size) and abs(zl.var() - 1.0) <= 5 * np.sqrt(2.0 / zl.size)


def test_smooth_special_values(ref):
    """a NaN passes through both clamps (torch.clamp), the bounds are reached exactly, -0 + +0 = +0"""
    nan, inf = F(np.nan), F(np.inf)

    def one(m, sigma, clip, z):
        return F(ref.td3_smooth(float(F(m)), float(F(sigma)), float(F(clip)), float(F(z))))
    assert np.isnan(one(nan, 0.2, 0.5, 1.0)) and np.isnan(one(0.3, 0.2, 0.5, nan)) and np.isnan(one(0.3, nan, 0.5, 1.0))
    assert np.isnan(one(0.3, inf, 0.5, 0.0))                                  # inf * 0, as torch
    assert one(1.0, 0.2, 0.5, 3.0) == 1.0 and one(-1.0, 0.2, 0.5, -3.0) == -1.0
    assert one(0.75, 1e30, 0.5, 1.0) == 1.0 and one(-0.75, 1e30, 0.5, -1.0) == -1.0
    assert one(0.25, 1e30, 0.5, 1.0) == 0.75 and one(0.25, 1e30, 0.5, -1.0) == -0.25
    assert one(0.25, inf, inf, 1.0) == 1.0 and one(0.25, inf, inf, -1.0) == -1.0
    assert one(0.25, 2.0, inf, 0.125) == 0.5
    for m, z, want in ((-0.0, 1.0, 0.0), (-0.0, -1.0, -0.0), (0.0, -1.0, 0.0)):
        got = one(m, 0.0, 0.5, z)
        assert got == 0.0 and np.signbit(got) == np.signbit(F(want))
    t = torch.tensor([0.3, -0.9, 0.99], dtype=torch.float32)
    zt = torch.tensor([1.7, -4.0, 0.2], dtype=torch.float32)
    want = (t + (0.2 * zt).clamp(-0.5, 0.5)).clamp(-1, 1).numpy()
    assert np.array_equal(T3.bits(T3.smooth(ref, t.numpy(), 0.2, 0.5, zt.numpy())), T3.bits(want))


# -------------------------------------------------------------------------------------------------------------------- the class
def test_td3target_refusals_need_no_gpu(monkeypatch):
    from soccer2d_amd import _capi
    from soccer2d_amd.td import Td3Target

    def boom(*a, **k):
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_capi, 'load_library', boom)
    mu = seq(10, (16, 8), 2, tanh_head=True)
    with pytest.raises(ValueError, match='1 to 8'):
        Td3Target.from_modules(seq(10, (16, 8), 9, tanh_head=True), seq(19, (8,), 1))
    with pytest.raises(ValueError, match='end in a Tanh'):
        Td3Target.from_modules(seq(10, (16, 8), 2), seq(12, (8,), 1))
    with pytest.raises(ValueError, match='obs_dim \\+ A'):
        Td3Target.from_modules(mu, seq(11, (8,), 1))
    with pytest.raises(ValueError, match='obs_dim \\+ A'):
        Td3Target.from_modules(mu, seq(12, (8,), 2))
    with pytest.raises(ValueError, match='critic 2'):
        Td3Target(mu, seq(12, (8,), 1), seq(10, (8,), 1))
    with pytest.raises(ValueError, match='torch.nn.Module'):
        Td3Target(mu, None)
    for kw in (dict(target_policy_noise=-0.1), dict(target_noise_clip=-1.0), dict(target_policy_noise=float('nan')),
               dict(target_noise_clip=float('nan')), dict(target_policy_noise='0.2')):
        with pytest.raises(ValueError, match='set_noise'):
            Td3Target(mu, seq(12, (8,), 1), **kw)
    t = Td3Target.from_modules(mu, seq(12, (8,), 1), seq(12, (64, 64), 1), seed=2 ** 64 + 5)
    assert (t.obs_dim, t.action_dim, len(t.critics), t.seed) == (10, 2, 2, 5)
    assert t.draws.dtype == torch.int64 and tuple(t.draws.shape) == (1,) and int(t.draws[0]) == 0
    assert t.noise.dtype == torch.float32 and t.noise.tolist() == [float(F(0.2)), 0.5]
    ptr = t.noise.data_ptr()
    assert t.set_noise(0.1, float('inf')) is t and t.noise.data_ptr() == ptr and t.noise.tolist() == [float(F(0.1)), float('inf')]
    for bad in ((-0.0001, 0.5), (0.2, -0.5), (float('nan'), 0.5), (0.2, float('nan')), (None, 0.5), (True, 0.5)):
        with pytest.raises(ValueError, match='set_noise'):
            t.set_noise(*bad)
    assert t.noise.tolist() == [float(F(0.1)), float('inf')]                 # a refused call writes nothing
    assert t.sync() is t
    B = 3
    good = {'next_obs': torch.zeros(B, 10), 'reward': torch.zeros(B), 'discount': torch.zeros(B)}
    with pytest.raises(ValueError, match='need a GPU'):
        t.target(good)
    with pytest.raises(ValueError, match='next_obs'):
        t.target(dict(good, next_obs=torch.zeros(B, 12)))
    with pytest.raises(ValueError, match=r'out\[2\]'):
        t.target(good, out=(torch.zeros(B), torch.zeros(B), torch.zeros(B, 3)), return_q=True)   # the action is [B, 2]
    with pytest.raises(ValueError, match='Td3Target.target'):
        t.target(good, out=torch.zeros(B + 1))


def test_learner_updates_a_td3target_on_the_host():
    """ActorCriticLearner.update_targets is torch on the flat buffers, so it runs here: it takes a Td3Target as it takes an
    ActorCriticTarget (lerp_ / copy_ bit for bit, the target modules follow), and leaves its noise words and counter alone"""
    from soccer2d_amd.learn import ActorCriticLearner
    from soccer2d_amd.td import Td3Target
    torch.manual_seed(4)
    mk = lambda: (seq(10, (16, 8), 2, tanh_head=True), seq(12, (16,), 1), seq(12, (8, 8), 1, 'tanh'))
    mods, tmods = mk(), mk()
    lrn = ActorCriticLearner.from_modules(*mods, device='cpu')
    tgt = Td3Target.from_modules(*tmods, device='cpu')
    nets, tnets = (lrn.actor,) + lrn.critics, (tgt.mu_target,) + tgt.critics
    old = [t.params.clone() for t in tnets]
    lrn.update_targets(tgt, tau=0.005)
    for n, t, o, m in zip(nets, tnets, old, tmods):
        assert torch.equal(t.params, o.lerp(n.params, 0.005)) and not torch.equal(t.params, o)
        assert torch.equal(torch.cat([p.detach().reshape(-1) for p in m.parameters()]), t.params)
    lrn.update_targets(tgt)
    assert all(torch.equal(t.params, n.params) for n, t in zip(nets, tnets))
    assert int(tgt.draws[0]) == 0 and tgt.noise.tolist() == [float(F(0.2)), 0.5]
    with pytest.raises(ValueError, match='critic'):
        lrn.update_targets(Td3Target.from_modules(tmods[0], tmods[1], device='cpu'))


# -------------------------------------------------------------------------------------------------------------------- the C ABI
def test_c_abi_refusals_that_need_no_device():
    """s2d_td_target_td3 checks everything before its first HIP call: every refusal is S2D_EINVAL with the field named (the
    pointers are never read: made-up addresses do)"""
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi
    from soccer2d_amd.td import td_workspace_bytes
    lib = _capi.load_library()

    def tdnet(n_in, hidden, n_out, base):
        s = _capi.S2DTdNet()
        s.n_in, s.n_hidden, s.n_out = n_in, len(hidden), n_out
        for l, w in enumerate(hidden):
            s.hidden[l] = w
        s.params, s.workspace = base, base + 0x100000
        s.workspace_bytes = td_workspace_bytes(n_in, hidden, n_out)
        return s
    D, A, B = 10, 4, 100
    arr = {k: 0x40000000 + 0x10000 * i for i, k in enumerate(('next_obs', 'reward', 'discount', 'noise', 'draws', 'out_target', 'out_q',
                                                               'out_action'))}

    def call(actor=None, c1=None, c2=None, batch=B, **over):
        actor = actor or tdnet(D, (16, 8), A, 0x10000000)
        c1 = c1 or tdnet(D + A, (8,), 1, 0x20000000)
        c2 = c2 or tdnet(D + A, (8,), 1, 0x30000000)
        p = dict(arr, **over)
        rc = lib.s2d_td_target_td3(batch, C.byref(actor) if actor != 'null' else None, C.byref(c1) if c1 != 'null' else None, C.byref(c2),
                                   p['next_obs'], p['reward'], p['discount'], p['noise'], p['draws'], 7, p['out_target'], p['out_q'],
                                   p['out_action'], None)
        return rc, lib.s2d_last_error().decode()

    def refused(what, needle, **kw):
        rc, text = call(**kw)
        assert rc == _capi.S2D_EINVAL, (what, rc)
        assert 's2d_td_target_td3' in text and needle in text, (what, text)
    refused('actor NULL', 'actor', actor='null')
    refused('critic1 NULL', 'critic1', c1='null')
    refused('n_out 9', 'n_out', actor=tdnet(D, (16, 8), 9, 0x10000000), c1=tdnet(D + 9, (8,), 1, 0x20000000))
    refused('critic n_in', 'critic1', c1=tdnet(D + A + 1, (8,), 1, 0x20000000))
    refused('critic2 n_in', 'critic2', c2=tdnet(D + A - 1, (8,), 1, 0x30000000))
    refused('critic n_out', 'critic1', c1=tdnet(D + A, (8,), 2, 0x20000000))
    refused('width off the grid', 'hidden', actor=tdnet(D, (16, 10), A, 0x10000000))
    refused('n_in', 'n_in', actor=tdnet(257, (16,), A, 0x10000000))
    bad = tdnet(D, (16, 8), A, 0x10000000); bad.activation = 3
    refused('activation', 'activation', actor=bad)
    bad = tdnet(D, (16, 8), A, 0x10000000); bad.params = None
    refused('params NULL', 'params', actor=bad)
    bad = tdnet(D, (16, 8), A, 0x10000000); bad.params += 4
    refused('params misaligned', 'params', actor=bad)
    bad = tdnet(D, (16, 8), A, 0x10000000); bad.workspace = None
    refused('workspace NULL', 'workspace', actor=bad)
    bad = tdnet(D + A, (8,), 1, 0x20000000); bad.workspace_bytes -= 4
    refused('workspace small', 'workspace', c1=bad)
    refused('shared workspace', 'share', c2=tdnet(D + A, (8,), 1, 0x20000000))
    refused('batch 0', 'batch', batch=0)
    refused('batch 2^31', 'batch', batch=2 ** 31)
    for name in ('next_obs', 'reward', 'discount', 'out_target'):
        refused(name + ' NULL', name, **{name: None})
        refused(name + ' misaligned', name, **{name: arr[name] + 2})
    for name in ('out_q', 'out_action'):
        refused(name + ' misaligned', 'optional', **{name: arr[name] + 1})
    refused('noise NULL', 'noise', noise=None)
    refused('noise misaligned', 'noise', noise=arr['noise'] + 2)
    refused('draws NULL', 'draws', draws=None)
    refused('draws misaligned', 'draws', draws=arr['draws'] + 4)
    refused('draws in out_target', 'draws must not overlap', draws=arr['out_target'] + 8)
    refused('draws in out_action', 'draws must not overlap', draws=arr['out_action'] + 4 * (B * A - 2))
    refused('draws in out_q', 'draws must not overlap', draws=arr['out_q'])
    refused('noise in out_target', 'noise must not overlap', noise=arr['out_target'] + 4 * (B - 1))
    refused('noise in out_q', 'noise must not overlap', noise=arr['out_q'] + 4)
    refused('noise in out_action', 'noise must not overlap', noise=arr['out_action'])
