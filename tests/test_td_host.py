"""CPU checks of the TD-target kernels' host side (s2d_td_target_q / s2d_td_target_ac, soccer2d_amd.td): the S2DTdNet ABI, the
host restatement (tests/td_ref.c) against wide_ref.c at n_in = 10 and against float64 NumPy, the workspace arithmetic, and the
argument checks of QTarget / ActorCriticTarget, every one of which raises before any library call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import td as TD
import wide_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip('torch')
nn = torch.nn
F = np.float32
_ACT = {'relu': nn.ReLU, 'tanh': nn.Tanh, 'sigmoid': nn.Sigmoid}


@pytest.fixture(scope='module')
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp('td_ref')
    return TD.build(d), W.build(d)


def seq(n_in, hidden, n_out, act='relu', tanh_head=False, bias=True):
    layers, win = [], n_in
    for w in hidden:
        layers += [nn.Linear(win, w, bias=bias), _ACT[act]()]
        win = w
    layers.append(nn.Linear(win, n_out, bias=bias))
    if tanh_head:
        layers.append(nn.Tanh())
    return nn.Sequential(*layers)


def net_of(module, act):
    """tests/td.py's Net of an nn.Sequential"""
    lin = [m for m in module if isinstance(m, nn.Linear)]
    p = np.concatenate([np.concatenate([l.weight.detach().numpy().ravel(), l.bias.detach().numpy().ravel()]) for l in lin])
    return TD.Net(lin[0].in_features, [l.out_features for l in lin[:-1]], lin[-1].out_features, act, p)


# ------------------------------------------------------------------------------------------------------------------------ ABI
TD_FIELDS = ('n_in', 'n_hidden', 'hidden', 'n_out', 'activation', 'params', 'workspace', 'workspace_bytes')


def test_struct_layout_matches_c(tmp_path):
    from soccer2d_amd import _capi
    prog = tmp_path / 'td_abi.c'
    offs = ','.join(f'offsetof(S2DTdNet,{f})' for f in TD_FIELDS)
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s2d.h"\nint main(){size_t v[]={sizeof(S2DTdNet),' + offs +
                    ',S2D_ABI_VERSION};for(unsigned i=0;i<sizeof v/sizeof*v;++i)printf("%zu ",v[i]);return 0;}\n')
    exe = tmp_path / 'td_abi'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(prog), '-o', str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    want = [C.sizeof(_capi.S2DTdNet)] + [getattr(_capi.S2DTdNet, f).offset for f in TD_FIELDS] + [4]
    assert got == want
    assert [f[0] for f in _capi.S2DTdNet._fields_] == list(TD_FIELDS)


def test_prototypes_are_bound():
    from soccer2d_amd import _capi
    protos = {p[0]: p for p in _capi.PROTOTYPES}
    assert protos['s2d_td_workspace_bytes'][1] is C.c_size_t and len(protos['s2d_td_workspace_bytes'][2]) == 1
    assert protos['s2d_td_target_q'][1] is C.c_int and len(protos['s2d_td_target_q'][2]) == 10
    assert protos['s2d_td_target_ac'][1] is C.c_int and len(protos['s2d_td_target_ac'][2]) == 11
    assert _capi.S2D_ABI_VERSION == 4


def test_symbols_exported_and_workspace_arithmetic():
    """the built library exports the three symbols; s2d_td_workspace_bytes (host only) agrees with the Python arithmetic on the
    grid and is 0 off it"""
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi
    from soccer2d_amd.td import td_workspace_bytes
    lib = _capi.load_library()
    for name in ('s2d_td_workspace_bytes', 's2d_td_target_q', 's2d_td_target_ac'):
        assert hasattr(lib, name), name

    def shape(n_in, hidden, n_out):
        s = _capi.S2DTdNet()
        s.n_in, s.n_hidden, s.n_out = n_in, len(hidden), n_out
        for l, w in enumerate(hidden):
            s.hidden[l] = w
        return s
    for n_in, hidden, n_out in ((1, (8,), 1), (10, (64, 64), 16), (4, (16, 8), 1), (256, (8,), 64), (14, (400, 300), 1),
                                (224, (12, 20, 400, 8, 28), 17)):
        got = lib.s2d_td_workspace_bytes(C.byref(shape(n_in, hidden, n_out)))
        assert got == td_workspace_bytes(n_in, hidden, n_out) and got > 0
    # n_in = 10: the wide actors' workspace
    s10 = _capi.S2DWideNet()
    s10.n_hidden, s10.n_out = 2, 16
    s10.hidden[0], s10.hidden[1] = 400, 300
    assert lib.s2d_wide_workspace_bytes(C.byref(s10)) == td_workspace_bytes(10, (400, 300), 16)
    for bad in (shape(0, (8,), 1), shape(257, (8,), 1), shape(10, (6,), 1), shape(10, (404,), 1), shape(10, (8,), 0), shape(10, (8,), 65),
                shape(10, (), 4), shape(10, (8, 10), 4)):
        assert lib.s2d_td_workspace_bytes(C.byref(bad)) == 0
    trailing = shape(10, (8,), 4)
    trailing.hidden[3] = 8                                                  # a width past n_hidden
    assert lib.s2d_td_workspace_bytes(C.byref(trailing)) == 0
    assert lib.s2d_td_workspace_bytes(None) == 0


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('act', ['relu', 'tanh', 'sigmoid'])
def test_restatement_equals_wide_ref_at_ten_inputs(refs, act):
    """at n_in = 10 the forward is wide_ref.c's wide_forward bit for bit (the padded 12-term layer 1), edge values included"""
    tl, wl = refs
    rs = np.random.RandomState(ACT_SEED[act])
    for hidden, na in (((8,), 1), ((12, 20), 17), ((64, 64), 16), ((128, 64, 32, 16), 4), ((400, 300), 1), ((8, 400, 12, 300, 16), 64)):
        net = TD.random_net(rs, 10, hidden, na, act, gain=2.0)
        x = rs.uniform(-1.5, 1.5, (96, 10)).astype(F)
        x[0], x[1], x[2] = 0.0, -0.0, 1e-40
        x[3] = [np.inf, -np.inf, np.nan, 3e38, -3e38, 1.0, -1.0, 1e-45, 0.5, -0.5]
        net.params[10 * hidden[0]:10 * hidden[0] + 4] = -0.0               # -0 biases: the padded layer 1 turns them into +0
        got, want = TD.forward(tl, net, x), W.forward(wl, x, net.params, hidden, na, act)
        assert np.array_equal(TD.bits(got), TD.bits(want))
        assert len(np.unique(got[4:])) > 8


ACT_SEED = {'relu': 11, 'tanh': 12, 'sigmoid': 13}


def _torch_forward(net, x):
    """torch's own CPU fp32 forward of the same parameters (a blocked GEMM sum)"""
    m = seq(net.n_in, net.hidden, net.n_out, net.act)
    lin = [l for l in m if isinstance(l, nn.Linear)]
    with torch.no_grad():
        for l, (Wt, b) in zip(lin, net.layers()):
            l.weight.copy_(torch.from_numpy(Wt.copy()))
            l.bias.copy_(torch.from_numpy(b.copy()))
        return m(torch.from_numpy(x)).numpy()


def _check_against_f64(what, got, want64, torch32):
    """every error against float64; allowed: 4 x torch's own largest fp32 error on the same inputs (a serial fmaf chain against
    a blocked GEMM sum), floored at one fp32 ulp of the largest |target|"""
    err = np.abs(got.astype(np.float64) - want64).max()
    torch_err = np.abs(torch32.astype(np.float64) - want64).max()
    ulp = float(np.spacing(F(np.abs(want64).max())))
    allowed = max(4.0 * torch_err, ulp)
    print(f'{what}: restatement error {err:.3g}, torch fp32 error {torch_err:.3g}, ulp {ulp:.3g}, ratio {err / allowed:.3g}')
    assert err <= allowed, f'{what}: error {err:.3g} is {err / allowed:.3g} x the allowed {allowed:.3g} (torch {torch_err:.3g}, ulp {ulp:.3g})'


Q_CASES = [(10, (64, 64), 16, 'relu'), (4, (16, 8), 16, 'tanh'), (224, (64, 64), 16, 'relu'), (256, (8,), 64, 'sigmoid'),
           (21, (128, 64, 32, 16), 17, 'tanh'), (36, (400, 300), 4, 'relu')]


@pytest.mark.parametrize('n_in,hidden,na,act', Q_CASES, ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_q_targets_against_float64(refs, n_in, hidden, na, act):
    tl = refs[0]
    rs = np.random.RandomState(n_in + na)
    B = 192
    tgt, onl = TD.random_net(rs, n_in, hidden, na, act), TD.random_net(rs, n_in, hidden, na, act)
    x = rs.uniform(-1, 1, (B, n_in)).astype(F)
    r, d = rs.uniform(-1, 1, B).astype(F), np.where(rs.rand(B) < 0.2, 0.0, 0.99).astype(F)
    y64, t32 = TD.forward64(tgt, x), _torch_forward(tgt, x)
    for online in (None, onl):
        t, q, idx = TD.target_q(tl, tgt, online, x, r, d)
        # the reference takes the value at the restatement's index: near-ties may order differently in another precision, and
        # what is checked here is the value's accuracy (the argmax itself is checked bitwise elsewhere)
        rows = np.arange(B)
        want = r.astype(np.float64) + d.astype(np.float64) * y64[rows, idx]
        tt = r + d * t32[rows, idx]
        _check_against_f64(f'{"double " if online else ""}dqn {n_in}-{hidden}-{na} {act}', t, want, tt)
        if online is None:                                                   # the argmax is the float64 one wherever it is clear-cut
            top2 = np.sort(y64, axis=1)[:, -2:] if na > 1 else None
            clear = (top2[:, 1] - top2[:, 0] > 1e-4) if na > 1 else np.ones(B, bool)
            assert clear.sum() > B // 2 and np.array_equal(idx[clear], y64.argmax(axis=1)[clear])


AC_CASES = [(10, 1, (400, 300), (64, 64), 'relu'), (4, 1, (16, 8), (64, 32, 16, 8), 'relu'), (224, 8, (64, 64), (64, 64), 'tanh'),
            (10, 4, (12, 20), (128, 64), 'sigmoid')]


@pytest.mark.parametrize('D,A,pi,qf,act', AC_CASES, ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_actor_critic_targets_against_float64(refs, D, A, pi, qf, act):
    tl = refs[0]
    rs = np.random.RandomState(D + A)
    B = 192
    actor = TD.random_net(rs, D, pi, A, act)
    c1, c2 = TD.random_net(rs, D + A, qf, 1, act), TD.random_net(rs, D + A, qf, 1, act)
    x = rs.uniform(-1, 1, (B, D)).astype(F)
    r, d = rs.uniform(-1, 1, B).astype(F), np.where(rs.rand(B) < 0.2, 0.0, 0.99).astype(F)
    pre64, pre32 = TD.forward64(actor, x), _torch_forward(actor, x)
    a64 = np.tanh(pre64)
    # the action: tanh_spec's stated error (1e-6, s2d_device.h) on top of the pre-activation's, which tanh (slope <= 1) does not grow
    a_allowed = 1e-6 + max(4.0 * np.abs(pre32.astype(np.float64) - pre64).max(), float(np.spacing(F(np.abs(pre64).max()))))
    row64 = np.concatenate([x.astype(np.float64), a64], axis=1)
    a32 = np.tanh(pre32)
    row32 = np.concatenate([x, a32], axis=1)
    q64 = [TD.forward64(c, row64)[:, 0] for c in (c1, c2)]
    q32 = [_torch_forward(c, row32)[:, 0] for c in (c1, c2)]
    for twin in (False, True):
        t, q, a = TD.target_ac(tl, actor, c1, c2 if twin else None, x, r, d)
        want = r.astype(np.float64) + d.astype(np.float64) * (np.minimum(q64[0], q64[1]) if twin else q64[0])
        tt = r + d * (np.minimum(q32[0], q32[1]) if twin else q32[0])
        _check_against_f64(f'{"td3" if twin else "ddpg"} {D}+{A} pi{pi} qf{qf} {act}', t, want, tt)
        assert np.abs(a.astype(np.float64) - a64).max() <= a_allowed


def _same(got, want):
    """one float32 against the expected one: both NaN, or the same bits"""
    got, want = F(got), F(want)
    return (np.isnan(got) and np.isnan(want)) or got.view(np.int32) == want.view(np.int32)


def test_restatement_special_values(refs):
    """the argmax's ties and NaNs, infinities through the two-rounding target, -0 rewards, the twin minimum's NaN rule"""
    tl = refs[0]
    # a network whose outputs are its biases: zero weights, so y = b for every row
    na = 5
    def const_net(n_in, b_out, n_out):
        p = np.zeros(TD.param_count(n_in, (8,), n_out), F)
        p[-n_out:] = b_out
        return TD.Net(n_in, (8,), n_out, 'relu', p)
    x = np.zeros((1, 3), F)
    one, zero = np.ones(1, F), np.zeros(1, F)
    for b, want_i in (([1, 3, 3, 2, 3], 1), ([np.nan, 1, 2, np.nan, 0], 0), ([1, np.nan, 2, 2, np.nan], 2), ([np.nan] * 5, 0),
                      ([-np.inf, np.inf, np.inf, 0, 1], 1), ([-np.inf] * 5, 0), ([0.0, -0.0, 0.0, -0.0, 0.0], 0)):
        t, q, i = TD.target_q(tl, const_net(3, np.array(b, F), na), None, x, one, one)
        assert i[0] == want_i and _same(q[0], b[want_i]), (b, i, q)
    inf_net = const_net(3, np.array([np.inf, 0, 0, 0, 0], F), na)
    t, _, _ = TD.target_q(tl, inf_net, None, x, one, zero)
    assert np.isnan(t[0])                                                     # 0 * inf: no special case, as torch
    t, _, _ = TD.target_q(tl, const_net(3, np.array([2, 0, 0, 0, 0], F), na), None, x, -zero, zero)
    assert _same(t[0], 0.0)                                # -0 + (0 * 2) = +0
    t, _, _ = TD.target_q(tl, const_net(3, np.array([-2, -3, -3, -3, -3], F), na), None, x, -zero, zero)
    assert _same(t[0], -0.0)                               # -0 + (0 * -2) = -0
    actor = const_net(3, np.array([0.5], F), 1)
    for b1, b2, want in ((1.0, 2.0, 1.0), (2.0, 1.0, 1.0), (1.0, np.nan, 1.0), (np.nan, 1.0, np.nan), (-np.inf, 0.0, -np.inf)):
        t, q, a = TD.target_ac(tl, actor, const_net(4, F(b1), 1), const_net(4, F(b2), 1), x, zero, one)
        assert _same(q[0], want), (b1, b2, q)


# -------------------------------------------------------------------------------------------------------------------- classes
def test_classes_pack_and_sync_on_cpu():
    """from_module reads the wide actors' module forms, holds the parameters flat in nn.Sequential order and reloads them on sync()"""
    from soccer2d_amd.td import ActorCriticTarget, QTarget, td_workspace_bytes
    torch.manual_seed(0)
    qt, qo = seq(10, (64, 64), 16), seq(10, (32,), 16, 'tanh')
    t = QTarget.from_module(qt, online=qo)
    assert (t.obs_dim, t.n_actions, t.q_target.hidden, t.online.hidden, t.online.activation) == (10, 16, (64, 64), (32,), 'tanh')
    assert np.array_equal(t.q_target.params.numpy(), net_of(qt, 'relu').params)
    assert t.q_target.workspace.numel() * 4 == td_workspace_bytes(10, (64, 64), 16)
    ptr = t.q_target.params.data_ptr()
    with torch.no_grad():
        qt[0].weight.mul_(2.0)
    assert not np.array_equal(t.q_target.params.numpy(), net_of(qt, 'relu').params)
    assert t.sync() is t and t.q_target.params.data_ptr() == ptr
    assert np.array_equal(t.q_target.params.numpy(), net_of(qt, 'relu').params)
    mu, q1, q2 = seq(224, (16, 8), 8, tanh_head=True), seq(232, (64, 32, 16, 8), 1), seq(232, (64, 64), 1, 'sigmoid')
    ac = ActorCriticTarget.from_modules(mu, q1, q2)
    assert (ac.obs_dim, ac.action_dim, len(ac.critics), ac.critics[1].activation) == (224, 8, 2, 'sigmoid')
    assert np.array_equal(ac.mu_target.params.numpy(), net_of(mu, 'relu').params)


def _forbid_library(monkeypatch):
    from soccer2d_amd import _capi

    def boom(*a, **k):
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_capi, 'load_library', boom)


def test_qtarget_argument_errors_raise_before_any_library_call(monkeypatch):
    from soccer2d_amd.td import QTarget
    _forbid_library(monkeypatch)
    with pytest.raises(ValueError, match='torch.nn.Module'):
        QTarget.from_module('q')
    with pytest.raises(ValueError, match='Linear'):
        QTarget.from_module(nn.Sequential(nn.Linear(10, 8), nn.ELU(), nn.Linear(8, 4)))
    with pytest.raises(ValueError, match='one activation'):
        QTarget.from_module(nn.Sequential(nn.Linear(10, 8), nn.ReLU(), nn.Linear(8, 8), nn.Tanh(), nn.Linear(8, 4)))
    with pytest.raises(ValueError, match='hidden layers'):
        QTarget.from_module(seq(10, (8,) * 6, 4))
    with pytest.raises(ValueError, match='multiple of 4'):
        QTarget.from_module(seq(10, (10,), 4))
    with pytest.raises(ValueError, match='multiple of 4'):
        QTarget.from_module(seq(10, (404,), 4))
    with pytest.raises(ValueError, match='bias'):
        QTarget.from_module(seq(10, (8,), 4, bias=False))
    with pytest.raises(ValueError, match='input width'):
        QTarget.from_module(seq(257, (8,), 4))
    with pytest.raises(ValueError, match='output width'):
        QTarget.from_module(seq(10, (8,), 65))
    with pytest.raises(ValueError, match='input and output widths'):
        QTarget.from_module(seq(10, (8,), 16), online=seq(11, (8,), 16))
    with pytest.raises(ValueError, match='input and output widths'):
        QTarget.from_module(seq(10, (8,), 16), online=seq(10, (8,), 15))
    t = QTarget.from_module(seq(10, (8,), 16), online=seq(10, (12, 8), 16, 'sigmoid'))
    B = 5
    good = {'next_obs': torch.zeros(B, 10), 'reward': torch.zeros(B), 'discount': torch.zeros(B)}
    with pytest.raises(ValueError, match='need a GPU'):                      # a CPU device: DeviceReplay's error
        t.target(good)
    with pytest.raises(ValueError, match='dict'):
        t.target(torch.zeros(B, 10))
    with pytest.raises(ValueError, match='dict'):
        t.target({'next_obs': torch.zeros(B, 10), 'reward': torch.zeros(B)})
    for key, bad in (('next_obs', torch.zeros(B, 11)), ('next_obs', torch.zeros(B, 10, dtype=torch.float64)), ('next_obs', torch.zeros(0, 10)),
                     ('next_obs', torch.zeros(B, 20)[:, ::2]), ('next_obs', torch.zeros(B)), ('reward', torch.zeros(B + 1)),
                     ('reward', torch.zeros(B, 1)), ('discount', torch.zeros(B, dtype=torch.int32)), ('discount', np.zeros(B, F))):
        with pytest.raises(ValueError, match=key):
            t.target(dict(good, **{key: bad}))
    with pytest.raises(ValueError, match='out'):
        t.target(good, out=torch.zeros(B + 1))
    with pytest.raises(ValueError, match='out'):
        t.target(good, out=torch.zeros(B, dtype=torch.float64))
    with pytest.raises(ValueError, match='three'):
        t.target(good, out=torch.zeros(B), return_q=True)
    with pytest.raises(ValueError, match=r'out\[2\]'):
        t.target(good, out=(torch.zeros(B), torch.zeros(B), torch.zeros(B)), return_q=True)       # the index is int32
    with pytest.raises(ValueError, match='one tensor'):
        t.target(good, out=(torch.zeros(B), torch.zeros(B)))


def test_actor_critic_argument_errors_raise_before_any_library_call(monkeypatch):
    from soccer2d_amd.td import ActorCriticTarget
    _forbid_library(monkeypatch)
    mu = seq(10, (16, 8), 2, tanh_head=True)
    with pytest.raises(ValueError, match='end in a Tanh'):
        ActorCriticTarget.from_modules(seq(10, (16, 8), 2), seq(12, (8,), 1))
    with pytest.raises(ValueError, match='obs_dim \\+ A'):
        ActorCriticTarget.from_modules(mu, seq(11, (8,), 1))
    with pytest.raises(ValueError, match='obs_dim \\+ A'):
        ActorCriticTarget.from_modules(mu, seq(12, (8,), 2))
    with pytest.raises(ValueError, match='critic 2'):
        ActorCriticTarget.from_modules(mu, seq(12, (8,), 1), seq(10, (8,), 1))
    with pytest.raises(ValueError, match='1 to 8'):
        ActorCriticTarget.from_modules(seq(10, (16, 8), 9, tanh_head=True), seq(19, (8,), 1))
    with pytest.raises(ValueError, match='torch.nn.Module'):
        ActorCriticTarget.from_modules(mu, None)
    ac = ActorCriticTarget.from_modules(mu, seq(12, (8,), 1), seq(12, (64, 64), 1))
    B = 3
    good = {'next_obs': torch.zeros(B, 10), 'reward': torch.zeros(B), 'discount': torch.zeros(B)}
    with pytest.raises(ValueError, match='need a GPU'):
        ac.target(good)
    with pytest.raises(ValueError, match='next_obs'):
        ac.target(dict(good, next_obs=torch.zeros(B, 12)))                   # the critic's width is not the batch's
    with pytest.raises(ValueError, match=r'out\[2\]'):
        ac.target(good, out=(torch.zeros(B), torch.zeros(B), torch.zeros(B, 3)), return_q=True)   # the action is [B, 2]
    with pytest.raises(ValueError, match='reward'):
        ac.target(dict(good, reward=torch.zeros(B, dtype=torch.float16)))
