"""CPU checks of the general-MLP fused actors' host side: the restatement of the network (tests/mlp_ref.c) against the two-layer
restatements and on the -0 edge, MlpQNetActor / MlpDeterministicActor shapes, packing and refusals, the LDS fit arithmetic and
the S2DMlpNet ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import actor_ref as A
import mlp_ref as M
import qnet_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip('torch')
nn = torch.nn


@pytest.fixture(scope='module')
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp('mlp_ref')
    return M.build(d), Q.build(d), A.build(d)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _edge_inputs(rs, n):
    x = rs.uniform(-1.5, 1.5, (n, 10)).astype(np.float32)
    x[0] = 0.0
    x[1] = -0.0
    x[2] = 1e-40                      # subnormals
    x[3] = [np.inf, -np.inf, np.nan, 3e38, -3e38, 1.0, -1.0, 1e-45, 0.5, -0.5]
    x[4] = 3e38
    return x


def test_two_layer_relu_equals_the_two_layer_restatements(refs):
    """L = 2, relu, widths that are multiples of 16: mlp_ref (layer 1 over k = 0 .. 11) equals qnet_ref.forward (k = 0 .. 9) and
    actor_ref.forward bit for bit -- behind relu the two padding terms cannot show"""
    ml, ql, al = refs
    rs = np.random.RandomState(0)
    for h1, h2, na in ((64, 64, 16), (16, 128, 3), (48, 80, 64), (128, 32, 1), (32, 16, 4)):
        x = _edge_inputs(rs, 300)
        for scale in (1.0, 1e19):     # 1e19: overflow to +-inf and NaN in the hidden layers
            p = (rs.uniform(-1, 1, M.param_count((h1, h2), na)) * scale).astype(np.float32)
            p[10 * h1:10 * h1 + 4] = -0.0
            y = M.forward(ml, x, p, (h1, h2), na, 'relu')
            assert np.array_equal(bits(y), bits(Q.forward(ql, x, p, h1, h2, na)))
            assert np.array_equal(bits(y), bits(A.forward(al, x, p, h1, h2, na)))
            assert np.array_equal(M.argmax(ml, y), Q.argmax(ql, y))
    # the tanh head on those outputs is actor_ref's
    p = rs.uniform(-1, 1, M.param_count((32, 16), 4)).astype(np.float32)
    x = _edge_inputs(rs, 64)
    k = np.arange(64) + 2 ** 32 - 30
    noise = np.array([[0.1, -0.1, 0.0, 0.2], [0.3, 0.2, 0.1, 0.5]], np.float32)
    for eps, kind in ((0.0, 0), (0.3, 1), (1.0, 1)):
        got = M.actor_actions(ml, x, p, (32, 16), 4, 'relu', eps, kind, noise, 0x5EED, k, gid0=7)
        want = A.actions(al, x, p, 32, 16, 4, eps, kind, noise, 0x5EED, k, gid0=7)
        assert np.array_equal(bits(got), bits(want))


def test_first_layer_padding_terms_turn_minus_zero_into_plus_zero(refs):
    """a tanh network whose first-layer accumulator is exactly -0 (bias -0, zero weights): without the two fmaf(0, 0, acc) of
    k = 10, 11 the unit is tanh_spec(-0) = -0, with them +0.  The spec, and so the restatement's default, is +0; the sign
    reaches the output through a weight of 1 and a bias of -0."""
    ml = refs[0]
    hidden, na = (8,), 1
    p = np.zeros(M.param_count(hidden, na), np.float32)
    p[:80] = -0.0                     # W_1 = -0 against x = +0: every product is -0, so the chain of ten stays at its bias
    p[80:88] = -0.0                   # b_1
    p[88] = 1.0                       # W_out[0][0]
    p[96] = -0.0                      # b_out
    x = np.zeros((2, 10), np.float32)
    y10 = M.forward(ml, x, p, hidden, na, 'tanh', first_k=10)
    y12 = M.forward(ml, x, p, hidden, na, 'tanh')
    assert (y10 == 0).all() and np.signbit(y10).all()            # -0 all the way: tanh_spec(-0) = -0, fmaf(1, -0, -0) = -0
    assert (y12 == 0).all() and not np.signbit(y12).any()        # the padding terms: fmaf(+0, +0, -0) = +0
    yr = M.forward(ml, x, p, hidden, na, 'relu', first_k=10)     # relu hides it: -0 -> +0 either way
    assert not np.signbit(yr).any()


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
    from soccer2d_amd.mlp_actor import MlpDeterministicActor, MlpQNetActor, param_count
    torch.manual_seed(0)
    cases = ((MlpQNetActor, (128, 64, 32, 16), nn.Tanh, 16, False),       # dqn_stable_baselines3_custom_model.py
             (MlpDeterministicActor, (16, 8), nn.ReLU, 1, True),          # dqn_ddpg_stable_baselines3.py: pi [16, 8]
             (MlpDeterministicActor, (32, 32, 32), nn.Tanh, 4, True))     # the optuna sweep: pi [32] * 3, Tanh
    for cls, hidden, act, na, head in cases:
        net = _seq(hidden, na, act, tanh_head=head, flatten=cls is MlpQNetActor)
        a = cls.from_module(net, device='cpu')
        want_shapes, win = [], 10
        for w in hidden + (na,):
            want_shapes += [(w, win), (w,)]
            win = w
        assert a.shapes() == tuple(want_shapes)
        assert a.hidden == hidden and a.activation == ('tanh' if act is nn.Tanh else 'relu')
        flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
        assert a.params.shape == (param_count(hidden, na),) == flat.shape
        assert torch.equal(a.params, flat)                                  # parameters() order
        before = a.params.clone()
        with torch.no_grad():
            for p in net.parameters():
                p.add_(0.5)
        assert torch.equal(a.params, before)
        a.sync()
        assert not torch.equal(a.params, before)
        assert torch.equal(a.params, torch.cat([p.detach().reshape(-1) for p in net.parameters()]))
        s = a.c_struct()
        assert s.n_hidden == len(hidden) and list(s.hidden) == list(hidden) + [0] * (4 - len(hidden))
        assert s.n_out == na and s.activation == (1 if act is nn.Tanh else 0) and s.noise_kind == 0
        a.epsilon = 0.25
        assert a.epsilon == 0.25 and float(a.epsilon_tensor) == 0.25
    d = MlpDeterministicActor.from_module(_seq((16, 8), 1, tanh_head=True), device='cpu', noise_sigma=0.2, noise_mean=0.1)
    assert d.noise_kind == 1 and d.c_struct().noise_kind == 1
    assert d.noise_sigma.tolist() == pytest.approx([0.2]) and d.noise_mean.tolist() == pytest.approx([0.1])
    # the existing classes still refuse these networks
    from soccer2d_amd.actor import QNetActor
    with pytest.raises(ValueError):
        QNetActor.from_module(_seq((128, 64, 32, 16), 16, nn.Tanh), device='cpu')


def test_refusals_name_the_limit():
    from soccer2d_amd.mlp_actor import MlpDeterministicActor, MlpQNetActor
    mixed = nn.Sequential(nn.Linear(10, 32), nn.ReLU(), nn.Linear(32, 32), nn.Tanh(), nn.Linear(32, 16))
    cases = ((mixed, 'one activation'),
             (_seq((32, 32), 16, nn.Sigmoid), 'ReLU or Tanh'),
             (_seq((12,), 16), 'multiple of 8'),
             (_seq((64, 136), 16), 'multiple of 8'),
             (_seq((), 16), 'hidden layers'),
             (_seq((32,) * 5, 16), 'hidden layers'),
             (_seq((32, 32), 16, bias=False), 'bias'),
             (_seq((128, 128, 128), 16), 'bytes of LDS'),
             (nn.Sequential(nn.Linear(10, 32), nn.Linear(32, 16)), 'Linear-(F-Linear)'))
    for net, word in cases:
        with pytest.raises(ValueError, match=re.escape(word)):
            MlpQNetActor.from_module(net, device='cpu')
    with pytest.raises(ValueError, match='Tanh'):
        MlpDeterministicActor.from_module(_seq((16, 8), 1), device='cpu')           # no tanh head
    with pytest.raises(ValueError, match='n_out'):
        MlpDeterministicActor.from_module(_seq((16, 8), 2, tanh_head=True), device='cpu')
    with pytest.raises(ValueError, match='n_actions'):
        MlpQNetActor((64, 64), 65, device='cpu')
    with pytest.raises(ValueError, match='activation'):
        MlpQNetActor((64, 64), 16, activation='sigmoid', device='cpu')
    with pytest.raises(ValueError, match='activation'):
        MlpQNetActor((64, 64), 16, activation='relu', device='cpu').load_from(_seq((64, 64), 16, nn.Tanh))
    with pytest.raises(ValueError, match='shapes'):
        MlpQNetActor((64, 64), 16, device='cpu').load_from(_seq((64, 32), 16))


# (hidden, outputs) -> waves per workgroup, or None: does not fit.  Worked by hand from the plan: LDS bytes = 4 * (64 F + B + waves *
# W) <= 163840 with F = sum over the layers of ceil(h_l / 16) * ksteps_l (ksteps = 3, then h_(l-1) / 4), the output layer's
# ceil(A / 16) * h_L / 4 included; B = the widths and A, each rounded up to 16; W = 32 * pitch + 64 * (A16 + 4) + 640 + 1600,
# pitch = the widest padded layer rounded up to 64, + 4.
FIT_TABLE = (
    # F = 12 + 64 + 16 = 92, B = 144, W = 2176 + 1280 + 2240 = 5696: 4 * (5888 + 144 + 4 * 5696) = 115264
    (((64, 64), 16), 4),
    # F = 24 + 128 + 32 + 8 + 4 = 196, B = 256, W = 4224 + 1280 + 2240 = 7744: 4 waves 175104 > 163840; 2 waves 113152
    (((128, 64, 32, 16), 16), 2),
    # F = 24 + 256 + 256 + 32 = 568, B = 400: 4 * (36352 + 400) = 147008, + one wave 30976 = 177984 > 163840
    (((128, 128, 128), 16), None),
    # F = 24 + 256 + 32 = 312, B = 272: 80960 + 4 * 30976 = 204864; 2 waves 142912
    (((128, 128), 16), 2),
    # F = 24 + 256 + 128 = 408 (A = 64: 4 tiles x 32), B = 320, W = 4224 + 4352 + 2240 = 10816: 105728 + 2 * 43264 = 192256; 1 wave 148992
    (((128, 128), 64), 1),
    # F = 3 + 2 = 5 (h = 8: one tile; the output layer 2 k-steps), B = 32, W = 2176 + 1280 + 2240 = 5696: 4 * 352 + 91136 = 92544
    (((8,), 1), 4),
    # F = 3 + 4 + 2 = 9 ([16, 8]), B = 48: 4 * (576 + 48) + 91136 = 93632
    (((16, 8), 1), 4),
    # F = 24 + 8 * 32 + 4 * 32 + 4 * 16 + 16 = 488, B = 128 + 128 + 64 + 64 + 16 = 400: 126528 + 30976 = 157504 with 1 wave (2: 188480)
    (((128, 128, 64, 64), 16), 1),
    # F = 6 + 3 * 10 = 36 ([24, 40]: 2 and 3 tiles; 40 over 24 inputs is 6 k-steps), + 10 = 46; B = 32 + 48 + 16 = 96; 4 waves 103296
    (((24, 40), 16), 4),
)


def test_fit_arithmetic_equals_the_plan():
    from soccer2d_amd.mlp_actor import LDS_BYTES, lds_plan
    want_bytes = {((64, 64), 16): 115264, ((128, 64, 32, 16), 16): 113152, ((128, 128, 128), 16): 177984,
                  ((128, 128), 16): 142912, ((128, 128), 64): 148992, ((8,), 1): 92544, ((16, 8), 1): 93632,
                  ((128, 128, 64, 64), 16): 157504}
    for (hidden, na), waves in FIT_TABLE:
        got_waves, nbytes = lds_plan(hidden, na)
        assert got_waves == waves, (hidden, na, got_waves, nbytes)
        assert (nbytes <= LDS_BYTES) == (waves is not None)
        if (hidden, na) in want_bytes:
            assert nbytes == want_bytes[(hidden, na)], (hidden, na, nbytes)


def test_struct_and_exports_match_the_header(tmp_path):
    from soccer2d_amd import _capi
    prog = tmp_path / 'sz.c'
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s2d.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n",'
                    'sizeof(S2DMlpNet),offsetof(S2DMlpNet,hidden),offsetof(S2DMlpNet,n_out),offsetof(S2DMlpNet,params),'
                    'offsetof(S2DMlpNet,noise));return 0;}\n')
    exe = tmp_path / 'sz'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(prog), '-o', str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    S = _capi.S2DMlpNet
    assert got == [C.sizeof(S), S.hidden.offset, S.n_out.offset, S.params.offset, S.noise.offset]
    protos = {p[0]: p for p in _capi.PROTOTYPES}
    for name, nargs in (('s2d_rollout_qnet_mlp', 6), ('s2d_rollout_actor_mlp', 6), ('s2d_debug_mlp_forward', 7)):
        assert name in protos and len(protos[name][2]) == nargs
    lib = os.path.join(ROOT, 'gym-soccer-2d-env_amd', 'lib', 'libs2d_hip.so')
    if os.path.exists(lib):
        syms = subprocess.run(['nm', '-D', '--defined-only', lib], stdout=subprocess.PIPE, text=True).stdout
        for name in ('s2d_rollout_qnet_mlp', 's2d_rollout_actor_mlp', 's2d_debug_mlp_forward'):
            assert re.search(r'\b%s\b' % name, syms)
