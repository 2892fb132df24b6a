"""CPU checks of the streamed-weight fused actors' host side: the restatement of the network (tests/wide_ref.c) against numpy
float64 and against the resident path's restatement (tests/mlp_ref.c), sigmoid_spec (error, edge values, monotonicity),
WideQNetActor / WideDeterministicActor shapes, packing and refusals, the plan's arithmetic and the S2DWideNet ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mlp_ref as M
import wide_f64 as W64
import wide_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip('torch')
nn = torch.nn
F = np.float32


@pytest.fixture(scope='module')
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp('wide_ref')
    return W.build(d), M.build(d)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


# ------------------------------------------------------------------------------------------------------------ the restatement
F64_SHAPES = [(12,), (20,), (28,), (300,), (400, 300), (256, 256), (8, 400, 12, 300, 16)]


@pytest.mark.parametrize('hidden', F64_SHAPES, ids=lambda h: '-'.join(map(str, h)))
def test_restatement_against_float64(refs, hidden):
    """every output of wide_ref lies within the rigorous running bound (tests/wide_f64.py) of the float64 network, for all three
    activations; the bound is what the number formats and the activations' stated errors give, nothing is fitted"""
    wl = refs[0]
    rs = np.random.RandomState(sum(hidden))
    for act, na in (('relu', 16), ('tanh', 4), ('sigmoid', 17)):
        p = W64.random_net(rs, hidden, na)
        x = rs.uniform(-1, 1, (64, 10)).astype(F)
        y = W.forward(wl, x, p, hidden, na, act)
        y64, e = W64.f64_bound(p, x, hidden, na, act)
        assert (np.abs(y - y64) <= e).all(), (act, float((np.abs(y - y64) / e).max()))
        assert len(np.unique(y)) > 32


def test_old_grid_shapes_equal_the_resident_restatement(refs):
    """L <= 4, widths multiples of 8 up to 128, relu / tanh: wide_ref is mlp_ref bit for bit, edge values included"""
    wl, ml = refs
    rs = np.random.RandomState(1)
    for hidden, na in (((8,), 1), ((24, 40), 17), ((128, 64, 32, 16), 16), ((64, 64), 4), ((8, 128, 8, 24), 64)):
        x = rs.uniform(-1.5, 1.5, (200, 10)).astype(F)
        x[0], x[1], x[2] = 0.0, -0.0, 1e-40
        x[3] = [np.inf, -np.inf, np.nan, 3e38, -3e38, 1.0, -1.0, 1e-45, 0.5, -0.5]
        for scale in (1.0, 1e19):
            p = (rs.uniform(-1, 1, M.param_count(hidden, na)) * scale).astype(F)
            p[10 * hidden[0]:10 * hidden[0] + 4] = -0.0
            for act in ('relu', 'tanh'):
                assert np.array_equal(bits(W.forward(wl, x, p, hidden, na, act)), bits(M.forward(ml, x, p, hidden, na, act)))


# --------------------------------------------------------------------------------------------------------------- sigmoid_spec
def _sig64(v):
    return 1.0 / (1.0 + np.exp(-np.asarray(v, dtype=np.float64)))


def test_sigmoid_spec_error_against_float64(refs):
    """the absolute error on [-100, 100] stays within the figure written next to the definition (W.SIGMOID_ERR = 1.0e-7;
    measured 8.93e-8), which is what the float64 bound of the networks then uses"""
    wl = refs[0]
    rs = np.random.RandomState(0)
    v = np.concatenate([np.linspace(-100, 100, 2000001), rs.uniform(-20, 20, 1000000), rs.uniform(-1, 1, 500000)]).astype(F)
    err = np.abs(W.sigmoid(wl, v).astype(np.float64) - _sig64(v))
    print(f'sigmoid_spec: largest error {err.max():.3g} at v = {v[err.argmax()]!r}')
    assert err.max() <= W.SIGMOID_ERR


def test_sigmoid_spec_edge_values(refs):
    wl = refs[0]
    tiny = F(W.sigmoid(wl, [-87.0])[0])                                          # exp_spec(-87) / 1: the named deviation from 0
    assert 1.6e-38 < tiny < 1.7e-38 and tiny >= 2.0 ** -126                      # normal
    v = np.array([0.0, -0.0, 87.0, 88.0, 1e30, np.inf, -87.0, -88.0, -1e30, -np.inf, 1e-40, -1e-40, 2.0 ** -149], dtype=F)
    want = np.array([0.5, 0.5, 1.0, 1.0, 1.0, 1.0, tiny, tiny, tiny, tiny, 0.5, 0.5, 0.5], dtype=F)
    assert np.array_equal(bits(W.sigmoid(wl, v)), bits(want))
    n = W.sigmoid(wl, np.array([np.nan, -np.nan], dtype=F))
    assert np.isnan(n).all()
    # symmetric where both branches are exact enough to say so: s(v) + s(-v) = 1 to an ulp of 1
    g = np.linspace(-20, 20, 4001).astype(F)
    assert np.abs(W.sigmoid(wl, g).astype(np.float64) + W.sigmoid(wl, -g) - 1.0).max() <= 2.0 ** -23


@pytest.mark.parametrize('centre,half', [(0.0, 1e-3), (0.0, 20.0), (87.0, 0.2), (-87.0, 0.2)])
def test_sigmoid_spec_is_monotone(refs, centre, half):
    """never decreasing on dense grids around 0 (the two branches meet), over the working range, and around +-87 (the clamp; the
    last change of exp_spec's exponent is at 86.99)"""
    g = np.unique(np.linspace(centre - half, centre + half, 400001).astype(F))
    s = W.sigmoid(refs[0], g)
    assert (np.diff(s.astype(np.float64)) >= 0).all()
    if centre == 0.0 and half < 1:
        u = (np.arange(-2000, 2001) * 2.0 ** -30).astype(F)                       # and float by float around 0
        assert (np.diff(W.sigmoid(refs[0], u).astype(np.float64)) >= 0).all()


# -------------------------------------------------------------------------------------------------------------------- classes
_ACT = {'relu': nn.ReLU, 'tanh': nn.Tanh, 'sigmoid': nn.Sigmoid}


def _seq(hidden, na, act=nn.ReLU, tanh_head=False, bias=True, flatten=False):
    layers, win = ([nn.Flatten()] if flatten else []), 10
    for w in hidden:
        layers += [nn.Linear(win, w, bias=bias), act()]
        win = w
    layers.append(nn.Linear(win, na, bias=bias))
    if tanh_head:
        layers.append(nn.Tanh())
    return nn.Sequential(*layers)


def test_from_module_on_the_reference_shapes():
    from soccer2d_amd.wide_actor import WideDeterministicActor, WideQNetActor, param_count, wide_plan
    torch.manual_seed(0)
    cases = ((WideDeterministicActor, (400, 300), 'relu', 1, True),        # ddpg_stable_baselines3.py: SB3's default actor
             (WideQNetActor, (256, 256), 'sigmoid', 16, False),            # the optuna samples: Sigmoid
             (WideQNetActor, (32, 400, 8, 128, 64), 'tanh', 16, False))    # ... and five layers
    for cls, hidden, act, na, head in cases:
        net = _seq(hidden, na, _ACT[act], tanh_head=head, flatten=cls is WideQNetActor)
        a = cls.from_module(net, device='cpu')
        want_shapes, win = [], 10
        for w in hidden + (na,):
            want_shapes += [(w, win), (w,)]
            win = w
        assert a.shapes() == tuple(want_shapes)
        assert a.hidden == hidden and a.activation == act
        flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
        assert a.params.shape == (param_count(hidden, na),) == flat.shape
        assert param_count(hidden, na) == sum(p.numel() for p in net.parameters())
        assert torch.equal(a.params, flat)                                  # parameters() order
        before = a.params.clone()
        with torch.no_grad():
            for p in net.parameters():
                p.add_(0.5)
        assert torch.equal(a.params, before)
        a.sync()
        assert torch.equal(a.params, torch.cat([p.detach().reshape(-1) for p in net.parameters()]))
        s = a.c_struct()
        assert s.n_hidden == len(hidden) and list(s.hidden) == list(hidden) + [0] * (5 - len(hidden))
        assert s.n_out == na and s.activation == ('relu', 'tanh', 'sigmoid').index(act) and s.noise_kind == 0
        assert s.workspace_bytes == wide_plan(hidden, na)[3] == a.workspace.numel() * 4 and a.plan == wide_plan(hidden, na)
        a.epsilon = 0.25
        assert a.epsilon == 0.25 and float(a.epsilon_tensor) == 0.25
    d = WideDeterministicActor.from_module(_seq((400, 300), 1, tanh_head=True), device='cpu', noise_sigma=0.2, noise_mean=0.1)
    assert d.noise_kind == 1 and d.c_struct().noise_kind == 1
    assert d.noise_sigma.tolist() == pytest.approx([0.2]) and d.noise_mean.tolist() == pytest.approx([0.1])
    # the resident classes still refuse these networks
    from soccer2d_amd.mlp_actor import MlpDeterministicActor, MlpQNetActor
    with pytest.raises(ValueError, match='multiple of 8'):
        MlpDeterministicActor.from_module(_seq((400, 300), 1, tanh_head=True), device='cpu')
    with pytest.raises(ValueError, match='bytes of LDS'):
        MlpQNetActor((128, 128, 128), 16, device='cpu')


def test_refusals_name_the_limit():
    from soccer2d_amd.wide_actor import WideDeterministicActor, WideQNetActor
    mixed = nn.Sequential(nn.Linear(10, 32), nn.ReLU(), nn.Linear(32, 32), nn.Sigmoid(), nn.Linear(32, 16))
    cases = ((mixed, 'one activation'),
             (_seq((32, 32), 16, nn.GELU), 'ReLU, Tanh or Sigmoid'),
             (_seq((404,), 16), 'multiple of 4'),
             (_seq((6,), 16), 'multiple of 4'),
             (_seq((64, 18), 16), 'multiple of 4'),
             (_seq((), 16), 'hidden layers'),
             (_seq((32,) * 6, 16), 'hidden layers'),
             (_seq((32, 32), 16, bias=False), 'bias'),
             (nn.Sequential(nn.Linear(10, 32), nn.Linear(32, 16)), 'Linear-(F-Linear)'))
    for net, word in cases:
        with pytest.raises(ValueError, match=re.escape(word)):
            WideQNetActor.from_module(net, device='cpu')
    with pytest.raises(ValueError, match='Tanh'):
        WideDeterministicActor.from_module(_seq((400, 300), 1), device='cpu')         # no tanh head
    with pytest.raises(ValueError, match='n_out'):
        WideDeterministicActor.from_module(_seq((400, 300), 2, tanh_head=True), device='cpu')
    with pytest.raises(ValueError, match='n_actions'):
        WideQNetActor((64, 64), 65, device='cpu')
    with pytest.raises(ValueError, match='activation'):
        WideQNetActor((64, 64), 16, activation='gelu', device='cpu')
    with pytest.raises(ValueError, match='activation'):
        WideQNetActor((64, 64), 16, activation='sigmoid', device='cpu').load_from(_seq((64, 64), 16, nn.Tanh))
    with pytest.raises(ValueError, match='shapes'):
        WideQNetActor((400, 300), 16, device='cpu').load_from(_seq((400, 296), 16))
    for hidden in ((404,), (6,), (18,), (32,) * 6):
        with pytest.raises(ValueError):
            WideQNetActor(hidden, 16, device='cpu')


# ----------------------------------------------------------------------------------------------------------------------- plan
# (hidden, outputs) -> (waves, env tiles, LDS bytes, workspace bytes), worked by hand.  Per wave W(T) = 32 T pitch + 64 (A16 + 4) +
# 640 + 1600 words, pitch = the widest padded layer rounded up to 64, + 4; LDS = 4 (B + waves W(T)) <= 163840 with B = the widths
# and A each rounded up to 16; the first of (4, 4) (4, 2) (4, 1) (2, 4) (2, 2) (2, 1) (1, 4) ... that fits.  Workspace = 4 (64 F + B),
# F = sum over the layers of ceil(h_l / 16) * ksteps_l (3, then h_(l-1) / 4), the output layer's ceil(A / 16) * h_L / 4 included.
PLAN_TABLE = (
    # pitch 68, B = 144, fixed 1280 + 2240 = 3520: W(4) = 8704 + 3520 = 12224 -> 4 (144 + 48896) = 196160 too much; W(2) = 4352 +
    # 3520 = 7872 -> 4 (144 + 31488) = 126528.  F = 12 + 64 + 16 = 92: 4 (5888 + 144) = 24128
    (((64, 64), 16), (4, 2, 126528, 24128)),
    # pitch 452 (400 -> 448 + 4), B = 400 + 304 + 16 = 720, fixed 3520: W(1) = 14464 + 3520 = 17984; 4 waves 4 (720 + 71936) =
    # 290624 too much; 2 waves: W(4) = 61376 and W(2) = 32448 too much (4 (720 + 64896) = 262464), W(1): 4 (720 + 35968) = 146752.
    # F = 25 * 3 + 19 * 100 + 1 * 75 = 2050: 4 (131200 + 720) = 527680
    (((400, 300), 1), (2, 1, 146752, 527680)),
    # pitch 260, B = 528, fixed 3520: 4 waves W(1) = 11840 -> 4 (528 + 47360) = 191552 too much; 2 waves W(4) = 36800 too much,
    # W(2) = 16640 + 3520 = 20160 -> 4 (528 + 40320) = 163392, 448 bytes to spare.  F = 48 + 16 * 64 + 64 = 1136: 4 (72704 + 528)
    (((256, 256), 16), (2, 2, 163392, 292928)),
    # pitch 452, B = 2000 + 16 = 2016: 2 waves W(1): 4 (2016 + 35968) = 151936.  F = 75 + 4 * 25 * 100 + 100 = 10175: 4 (651200 + 2016)
    (((400,) * 5, 16), (2, 1, 151936, 2612864)),
)


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi
    return _capi.load_library()


def test_plan_arithmetic(lib):
    from soccer2d_amd import _capi
    from soccer2d_amd.wide_actor import LDS_BYTES, WIDE_WIDTHS, wide_plan
    for (hidden, na), want in PLAN_TABLE:
        assert wide_plan(hidden, na) == want, (hidden, na, wide_plan(hidden, na))
        s = _capi.S2DWideNet()
        s.n_hidden = len(hidden)
        for l, w in enumerate(hidden):
            s.hidden[l] = w
        s.n_out = na
        assert lib.s2d_wide_workspace_bytes(C.byref(s)) == want[3]           # the C plan's own figure
    # every plan fits, the worst ones included
    for hidden, na in (((400,) * 5, 64), ((400,), 64), ((8,), 1), ((396, 400), 64), ((128,) * 5, 16)):
        waves, tiles, nbytes, _ = wide_plan(hidden, na)
        assert nbytes <= LDS_BYTES and waves in (1, 2, 4) and tiles in (1, 2, 4)
    assert all(wide_plan((w,), 64)[2] <= LDS_BYTES for w in WIDE_WIDTHS)
    bad = _capi.S2DWideNet()
    bad.n_hidden, bad.n_out = 1, 16
    for w in (404, 6, 18, 0):
        bad.hidden[0] = w
        assert lib.s2d_wide_workspace_bytes(C.byref(bad)) == 0
    bad.hidden[0], bad.hidden[1] = 64, 8                                       # an entry past n_hidden
    assert lib.s2d_wide_workspace_bytes(C.byref(bad)) == 0
    bad.hidden[1], bad.n_hidden = 0, 6
    assert lib.s2d_wide_workspace_bytes(C.byref(bad)) == 0
    assert lib.s2d_wide_workspace_bytes(None) == 0


def test_struct_and_exports_match_the_header(tmp_path):
    from soccer2d_amd import _capi
    prog = tmp_path / 'sz.c'
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s2d.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %d\\n",'
                    'sizeof(S2DWideNet),offsetof(S2DWideNet,hidden),offsetof(S2DWideNet,n_out),offsetof(S2DWideNet,params),'
                    'offsetof(S2DWideNet,noise),offsetof(S2DWideNet,workspace),offsetof(S2DWideNet,workspace_bytes),'
                    'S2D_ABI_VERSION);return 0;}\n')
    exe = tmp_path / 'sz'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(prog), '-o', str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    S = _capi.S2DWideNet
    assert got == [C.sizeof(S), S.hidden.offset, S.n_out.offset, S.params.offset, S.noise.offset, S.workspace.offset,
                   S.workspace_bytes.offset, 4]
    assert _capi.S2D_ABI_VERSION == 4
    protos = {p[0]: p for p in _capi.PROTOTYPES}
    for name, nargs in (('s2d_rollout_qnet_wide', 6), ('s2d_rollout_actor_wide', 6), ('s2d_debug_wide_forward', 7),
                        ('s2d_wide_workspace_bytes', 1)):
        assert name in protos and len(protos[name][2]) == nargs
    lib = os.path.join(ROOT, 'gym-soccer-2d-env_amd', 'lib', 'libs2d_hip.so')
    if os.path.exists(lib):
        syms = subprocess.run(['nm', '-D', '--defined-only', lib], stdout=subprocess.PIPE, text=True).stdout
        for name in protos:
            if 'wide' in name:
                assert re.search(r'\b%s\b' % name, syms)
