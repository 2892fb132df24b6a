"""CPU checks of the fused Q-network actor's host side: the restatement of its policy (tests/qnet_ref.c) against a float64
forward and on edge networks, the epsilon threshold, QNetActor packing and validation, and the S2DQNet / export ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as O
import qnet_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return Q.build(tmp_path_factory.mktemp('qnet_ref'))


def _params(rs, h1, h2, na, scale=1.0):
    return (rs.uniform(-1, 1, Q_count(h1, h2, na)) * scale).astype(np.float32)


def Q_count(h1, h2, na):
    return 10 * h1 + h1 + h1 * h2 + h2 + na * h2 + na


def _split(p, h1, h2, na):
    sizes = [10 * h1, h1, h1 * h2, h2, na * h2, na]
    out, o = [], 0
    for s in sizes:
        out.append(p[o:o + s].astype(np.float64)); o += s
    W1, b1, W2, b2, W3, b3 = out
    return W1.reshape(h1, 10), b1, W2.reshape(h2, h1), b2, W3.reshape(na, h2), b3


def test_restatement_matches_a_float64_forward(ref):
    rs = np.random.RandomState(0)
    for h1, h2, na in ((64, 64, 16), (16, 128, 3), (128, 32, 64)):
        p = _params(rs, h1, h2, na)
        x = rs.uniform(-1.5, 1.5, (4000, 10)).astype(np.float32)
        W1, b1, W2, b2, W3, b3 = _split(p, h1, h2, na)
        a1 = np.maximum(x.astype(np.float64) @ W1.T + b1, 0)
        a2 = np.maximum(a1 @ W2.T + b2, 0)
        q64 = a2 @ W3.T + b3
        q = Q.forward(ref, x, p, h1, h2, na)
        assert np.allclose(q, q64, rtol=1e-4, atol=1e-4 * np.abs(q64).max())
        g = Q.argmax(ref, q)
        if na > 1:
            s = np.sort(q64, axis=1)
            clear = (s[:, -1] - s[:, -2]) > 1e-3 * np.abs(q64).max(axis=1)
            assert clear.mean() > 0.8
            assert np.array_equal(g[clear], q64.argmax(axis=1)[clear])
        else:
            assert (g == 0).all()


def test_edge_networks(ref):
    h1 = h2 = 16
    na = 4
    # zero weights, -0 biases: every hidden unit is relu(-0) = +0, so q = b3 exactly
    p = np.zeros(Q_count(h1, h2, na), dtype=np.float32)
    p[10 * h1:10 * h1 + h1] = -0.0
    o_b3 = Q_count(h1, h2, na) - na
    p[o_b3:] = [1.0, 3.0, 3.0, 2.0]
    x = np.ones((3, 10), dtype=np.float32)
    q = Q.forward(ref, x, p, h1, h2, na)
    assert np.array_equal(q, np.tile([1.0, 3.0, 3.0, 2.0], (3, 1)).astype(np.float32))
    assert (Q.greedy(ref, x, p, h1, h2, na) == 1).all()        # tie: lowest index
    # the -0 bias case through one hidden unit: relu maps -0 to +0 (sign bit clear), visible through 1 / h
    p2 = np.zeros_like(p)
    p2[10 * h1:10 * h1 + h1] = -0.0
    p2[o_b3 - na * h2:o_b3] = 1.0                               # W3 = 1: q = sum of hidden units (+0) + b3 (-0)
    p2[o_b3:] = -0.0
    q2 = Q.forward(ref, x, p2, h1, h2, na)
    assert (np.signbit(q2) == False).all()                      # noqa: E712  (+0 + -0 = +0)
    # NaN never wins; a NaN first entry keeps action 0
    qn = np.array([[0.0, np.nan, 1.0, np.nan], [np.nan, 5.0, 6.0, 7.0], [2.0, 2.0, np.nan, 2.0], [np.nan] * 4],
                  dtype=np.float32)
    assert Q.argmax(ref, qn).tolist() == [2, 0, 0, 0]
    assert Q.argmax(ref, np.zeros((2, 7), np.float32)).tolist() == [0, 0]
    assert Q.argmax(ref, np.array([[-np.inf, -1.0, -np.inf]], np.float32)).tolist() == [1]


def test_epsilon_threshold(ref):
    assert Q.threshold(ref, 0.0) == 0
    assert Q.threshold(ref, -0.5) == 0
    assert Q.threshold(ref, float('nan')) == 0
    assert Q.threshold(ref, 1.0) == 1 << 32
    assert Q.threshold(ref, 2.0) == 1 << 32
    assert Q.threshold(ref, float('inf')) == 1 << 32
    assert Q.threshold(ref, 0.5) == 1 << 31
    assert Q.threshold(ref, 2.0 ** -32) == 1
    assert Q.threshold(ref, 0.05) == int(np.float32(0.05) * np.float32(2.0 ** 32))
    assert Q.threshold(ref, np.nextafter(np.float32(1), np.float32(0))) == (1 << 32) - 256


def test_vectorised_philox_matches_the_oracle():
    rs = np.random.RandomState(1)
    for _ in range(20):
        ctr = [int(v) for v in rs.randint(0, 2 ** 32, 4, dtype=np.uint64)]
        key = [int(v) for v in rs.randint(0, 2 ** 32, 2, dtype=np.uint64)]
        got = [int(w[()]) for w in Q.philox(*[np.uint64(c) for c in ctr], key[0], key[1])]
        assert got == O.philox(ctr, key)
    seed, gid, k = 0x5EED, np.array([0, 7, 2 ** 33 + 5]), np.array([0, 5, 11])
    for block in (0, 2):
        w = Q.policy_word(seed, gid, k, block)
        for i in range(3):
            g = int(gid[i])
            ref = O.philox([g & 0xFFFFFFFF, g >> 32, int(k[i]) >> 2, (1 << 16) | block], [seed & 0xFFFFFFFF, seed >> 32])
            assert int(w[i]) == ref[int(k[i]) & 3]


def _seq(h1=64, h2=64, na=16):
    return torch.nn.Sequential(torch.nn.Linear(10, h1), torch.nn.ReLU(), torch.nn.Linear(h1, h2), torch.nn.ReLU(),
                               torch.nn.Linear(h2, na))


def test_actor_packing_and_validation():
    from soccer2d_amd.actor import QNetActor, param_count
    torch.manual_seed(0)
    net = _seq()
    a = QNetActor.from_module(net, device='cpu')
    want = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    assert a.params.shape == (5904,) and param_count(64, 64, 16) == 5904
    assert torch.equal(a.params, want)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(1.0)
    a.sync()
    assert torch.equal(a.params, torch.cat([p.detach().reshape(-1) for p in net.parameters()]))
    a.epsilon = 0.25
    assert a.epsilon == 0.25 and float(a.epsilon_tensor) == 0.25
    for h1, h2 in ((40, 64), (64, 256)):
        with pytest.raises(ValueError):
            QNetActor.from_module(_seq(h1, h2), device='cpu')
    four = torch.nn.Sequential(torch.nn.Linear(10, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(),
                               torch.nn.Linear(64, 64), torch.nn.ReLU(), torch.nn.Linear(64, 16))
    with pytest.raises(ValueError):
        QNetActor.from_module(four, device='cpu')
    with pytest.raises(ValueError):
        QNetActor(64, 64, 16, device='cpu').load_from(_seq(64, 64, 8))
    with pytest.raises(ValueError):
        QNetActor(64, 64, 65, device='cpu')
    # the kernel evaluates ReLU between the layers: other activations, or none, are refused
    tanh = torch.nn.Sequential(torch.nn.Linear(10, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
                               torch.nn.Linear(64, 16))
    bare = torch.nn.Sequential(torch.nn.Linear(10, 64), torch.nn.Linear(64, 64), torch.nn.Linear(64, 16))
    for m in (tanh, bare):
        with pytest.raises(ValueError):
            QNetActor.from_module(m, device='cpu')
        with pytest.raises(ValueError):
            QNetActor(64, 64, 16, device='cpu').load_from(m)
    # SB3's QNetwork form: a Flatten features extractor in front of the Sequential
    sb3_like = torch.nn.Sequential(torch.nn.Flatten(), _seq())
    assert QNetActor.from_module(sb3_like, device='cpu').params.shape == (5904,)


def test_qnet_struct_and_export_match_the_header():
    from soccer2d_amd import _capi
    hdr = open(os.path.join(ROOT, 'include', 's2d.h')).read()
    m = re.search(r'typedef struct S2DQNet \{(.*?)\} S2DQNet;', hdr, re.S)
    assert m and 'hidden1, hidden2, n_actions, reserved' in m.group(1)
    assert C.sizeof(_capi.S2DQNet) == 32
    assert [f[0] for f in _capi.S2DQNet._fields_] == ['hidden1', 'hidden2', 'n_actions', 'reserved', 'params', 'epsilon']
    assert _capi.S2DQNet.params.offset == 16 and _capi.S2DQNet.epsilon.offset == 24
    assert re.search(r'int s2d_rollout_qnet\(S2DHandle h, int n_steps, const S2DQNet \*net, const S2DRollout \*out, '
                     r'float \*terminal_obs, void \*stream\);', hdr)
    protos = {p[0]: p for p in _capi.PROTOTYPES}
    assert 's2d_rollout_qnet' in protos and len(protos['s2d_rollout_qnet'][2]) == 6
    lib = os.path.join(ROOT, 'gym-soccer-2d-env_amd', 'lib', 'libs2d_hip.so')
    if os.path.exists(lib):
        import subprocess
        syms = subprocess.run(['nm', '-D', '--defined-only', lib], stdout=subprocess.PIPE, text=True).stdout
        assert re.search(r'\bs2d_rollout_qnet\b', syms)


def test_policy_counter_helpers_wrap_modulo_2_32(ref):
    """policy_step is a uint32 on the device, seen through an int32 plane: the helpers take every counter modulo 2^32, so
    the int32 view (negative past 2^31), the uint32 value and k0 + t past 2^32 all name the same Philox words"""
    seed, gid = 0x5EED, np.arange(6, dtype=np.int64)
    k = np.array([2 ** 31 - 2, 2 ** 31, 2 ** 32 - 4, 2 ** 32 - 1, 0, 3], dtype=np.int64)
    view = k.astype(np.uint32).view(np.int32).astype(np.int64)
    assert (view[1:4] < 0).all()
    for block in (0, 2):
        w = Q.policy_word(seed, gid, k, block)
        assert np.array_equal(w, Q.policy_word(seed, gid, view, block))
        assert np.array_equal(w, Q.policy_word(seed, gid, k + 2 ** 32, block))
        for i in range(k.size):
            kk = int(k[i])
            want = O.philox([int(gid[i]), 0, kk >> 2, (1 << 16) | block], [seed & 0xFFFFFFFF, seed >> 32])
            assert int(w[i]) == want[kk & 3]
    rs = np.random.RandomState(3)
    p = _params(rs, 16, 16, 5)
    x = rs.uniform(-1, 1, (6, 10)).astype(np.float32)
    a = Q.actions(ref, x, p, 16, 16, 5, 0.5, seed, gid, k)
    assert np.array_equal(a, Q.actions(ref, x, p, 16, 16, 5, 0.5, seed, gid, view))
    assert np.array_equal(a, Q.actions(ref, x, p, 16, 16, 5, 0.5, seed, gid, k + 2 ** 32))


def test_oracle_uint32_counters_are_exact_past_2_31():
    """OracleEngine.state returns the uint32 counters exactly in the engine's int32 view, set_env / set_state pass them
    to the oracle as non-negative values, and a rollout across 2^32 wraps policy_step modulo 2^32"""
    n, T = 12, 9
    orc = O.OracleEngine(O.make_config(**O.DQN_KWARGS), n, 'f32')
    orc.reset()
    k = np.array([2 ** 32 - 1 - (i % 7) if i % 3 == 0 else 2 ** 31 - 2 for i in range(n)], dtype=np.int64)
    orc.set_state('policy_step', k)
    want = k.astype(np.uint32).view(np.int32)
    assert np.array_equal(orc.state('policy_step'), want)
    orc.set_env(1, episode=int(want[0]))                                 # an int32 view round-trips too
    orc.set_env(2, episode=2 ** 32 - 2)
    ep = orc.state('episode')
    assert ep[1] == want[0] and ep[2] == -2
    orc.set_env(4, cycle=5)                                              # rewrites every field from state(): unchanged
    assert np.array_equal(orc.state('policy_step'), want)
    orc.rollout(T)
    assert np.array_equal(orc.state('policy_step'), (k + T).astype(np.uint32).view(np.int32))
    assert orc.state('episode')[2] in (-2, -1)


def test_debug_net_forward_is_declared_and_bound():
    from soccer2d_amd import _capi
    hdr = open(os.path.join(ROOT, 'include', 's2d.h')).read()
    assert re.search(r'int s2d_debug_net_forward\(int h1, int h2, int na, const void \*params_dev, const void \*obs_dev, '
                     r'int64_t n, void \*y_dev,\s+void \*greedy_dev, char \*name, void \*stream\);', hdr)
    protos = {p[0]: p for p in _capi.PROTOTYPES}
    assert len(protos['s2d_debug_net_forward'][2]) == 10
