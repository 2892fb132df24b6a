"""The fused actors' network on the matrix cores, bit for bit.  s2d_debug_net_forward runs the rollout kernels' weight packing,
LDS plan and net_forward on caller observations; its output y and argmax are compared with the host restatements
(tests/qnet_ref.c, tests/actor_ref.c: fmaf chains from the bias in ascending k) at every supported shape, on edge values
(signed zeros, subnormals, overflow, inf * 0, NaN), with the k order made observable, against a rigorous float64 error bound,
and tied back to the actions the rollouts record."""
import ctypes as C
import re

import numpy as np
import pytest

import oracle as O
import actor_ref as R
import qnet_ref as Q

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

F = np.float32
WIDTHS = list(range(16, 129, 16))
NS = [1, 63, 64, 65, 257, 1000]
SWEEP = [(h1, h2, 16) for h1 in WIDTHS for h2 in WIDTHS] + \
        [(h1, h2, na) for (h1, h2) in ((48, 80), (80, 48), (112, 16), (16, 112), (96, 96), (128, 128))
         for na in (1, 2, 4, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)]
TINY = F(2.0 ** -149)


@pytest.fixture(scope='module')
def qref(tmp_path_factory):
    return Q.build(tmp_path_factory.mktemp('qnet_ref'))


@pytest.fixture(scope='module')
def aref(tmp_path_factory):
    return R.build(tmp_path_factory.mktemp('actor_ref'))


def count(h1, h2, na):
    return 10 * h1 + h1 + h1 * h2 + h2 + na * h2 + na


def views(p, h1, h2, na):
    """W1, b1, W2, b2, W3, b3: writable views into the packed parameter vector p (nn.Sequential order)"""
    out, o = [], 0
    for shape in ((h1, 10), (h1,), (h2, h1), (h2,), (na, h2), (na,)):
        s = int(np.prod(shape))
        out.append(p[o:o + s].reshape(shape))
        o += s
    return out


def plan_waves(h1, h2, na):
    """waves per workgroup of the LDS plan (plan_lds in s2d_actor.hip): as many of 4, 2, 1 as 160 KiB hold"""
    na16 = (na + 15) // 16 * 16
    pitch = (max(h1, h2) + 63) // 64 * 64 + 4
    nfrag = h1 // 16 * 3 + h2 // 16 * (h1 // 4) + na16 // 16 * (h2 // 4)
    shared = (nfrag * 64 + h1 + h2 + na16 + 3) & ~3
    wave = 2 * 16 * pitch + 64 * (na16 + 4) + 640 + 25 * 64
    w = 4
    while w > 1 and (shared + w * wave) * 4 > 160 * 1024:
        w //= 2
    return w


def device_forward(params, x, h1, h2, na, pad=64):
    """(y [n][na], greedy [n], kernel name) of s2d_debug_net_forward; `pad` rows past n must stay untouched"""
    from soccer2d_amd import _capi
    lib = _capi.load_library()
    x = np.ascontiguousarray(x, dtype=F)
    n = x.shape[0]
    p = torch.from_numpy(np.ascontiguousarray(params, dtype=F)).to('cuda:0')
    xt = torch.from_numpy(x).to('cuda:0')
    y = torch.full((n + pad, na), -7777.0, dtype=torch.float32, device='cuda:0')
    g = torch.full((n + pad,), -5, dtype=torch.int32, device='cuda:0')
    name = C.create_string_buffer(96)
    torch.cuda.synchronize()
    _capi.check(lib, lib.s2d_debug_net_forward(h1, h2, na, p.data_ptr(), xt.data_ptr(), n, y.data_ptr(), g.data_ptr(), name,
                                               None), 's2d_debug_net_forward')
    torch.cuda.synchronize()
    y, g = y.cpu().numpy(), g.cpu().numpy()
    assert (y[n:] == -7777.0).all() and (g[n:] == -5).all(), 'wrote past n'
    return y[:n], g[:n], name.value.decode()


def same(got, want, what):
    """bit for bit, the sign of zero included; where both are NaN only that they are NaN"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype == F:
        gn, wn = np.isnan(got), np.isnan(want)
        bad = (gn != wn) | (~gn & ~wn & (got.view(np.int32) != want.view(np.int32)))
    else:
        bad = got != want
    if bad.any():
        idx = np.argwhere(bad)
        i = tuple(idx[0])
        raise AssertionError(f'{what}: {len(idx)} of {got.size} differ; first at {i}: gpu={got[i]!r} cpu={want[i]!r}')


def check(qref, aref, params, x, h1, h2, na, what):
    """the device against Q.forward / Q.argmax (and R.forward for the tanh heads' widths); returns y"""
    y, g, name = device_forward(params, x, h1, h2, na)
    m = re.fullmatch(r's2d_debug_net_forward_kernel<h1=(\d+),h2=(\d+),a=(\d+),waves=(\d)>', name)
    assert m and tuple(map(int, m.groups())) == (h1, h2, na, plan_waves(h1, h2, na)), name
    want = Q.forward(qref, x, params, h1, h2, na)
    same(y, want, f'{what} y')
    same(g, Q.argmax(qref, want), f'{what} greedy')
    if na in (1, 4):
        same(y, R.forward(aref, x, params, h1, h2, na), f'{what} y (actor restatement)')
    return y


def random_net(rs, h1, h2, na):
    """weights and biases N(0, 1 / fan_in)"""
    p = np.zeros(count(h1, h2, na), dtype=F)
    for v, fan in zip(views(p, h1, h2, na), (10, 10, h1, h1, h2, h2)):
        v[...] = rs.normal(0, 1 / np.sqrt(fan), v.shape)
    return p


def random_obs(rs, n):
    x = rs.uniform(-1, 1, (n, 10))
    x[::4] *= 100                                     # a slice far outside the observation range
    return x.astype(F)


def gamma(k):
    u = 2.0 ** -24
    return k * u / (1 - k * u)


def error_bound(params, x, h1, h2, na):
    """y64 (the network in float64 on the same float32 inputs) and a rigorous bound on |y - y64| for any k-ordered fmaf chain:
    e_l = |W_l| e_{l-1} + gamma_K (|b_l| + |W_l| (|a_{l-1}| + e_{l-1})) + K 2^-149 (relu is 1-Lipschitz)"""
    W1, b1, W2, b2, W3, b3 = [v.astype(np.float64) for v in views(params.copy(), h1, h2, na)]
    x = x.astype(np.float64)
    a1 = np.maximum(x @ W1.T + b1, 0)
    a2 = np.maximum(a1 @ W2.T + b2, 0)
    y64 = a2 @ W3.T + b3
    e1 = gamma(10) * (np.abs(b1) + np.abs(x) @ np.abs(W1).T) + 10 * 2.0 ** -149
    e2 = e1 @ np.abs(W2).T + gamma(h1) * (np.abs(b2) + (a1 + e1) @ np.abs(W2).T) + h1 * 2.0 ** -149
    e3 = e2 @ np.abs(W3).T + gamma(h2) * (np.abs(b3) + (a2 + e2) @ np.abs(W3).T) + h2 * 2.0 ** -149
    return y64, e3


# ---------------------------------------------------------------------------------------------------------------- shape sweep
def test_sweep_covers_every_plan_and_remainder():
    assert {plan_waves(*s) for s in SWEEP} == {1, 2, 4}
    assert {h // 16 for s in SWEEP for h in s[:2]} == set(range(1, 9))                  # 1 .. 8 output tiles per layer
    assert {(na + 15) // 16 for *_, na in SWEEP} == {1, 2, 3, 4}


@pytest.mark.parametrize('case', range(len(SWEEP)), ids=lambda c: '%d-%d-%d' % SWEEP[c])
def test_shape_sweep(qref, aref, case):
    h1, h2, na = SWEEP[case]
    n = NS[case % len(NS)]
    rs = np.random.RandomState(1000 + case)
    params, x = random_net(rs, h1, h2, na), random_obs(rs, n)
    y = check(qref, aref, params, x, h1, h2, na, f'{h1}-{h2}-{na} n={n}')
    y64, bound = error_bound(params, x, h1, h2, na)
    err = np.abs(y.astype(np.float64) - y64)
    assert np.isfinite(y).all() and (err <= bound).all(), float((err / bound).max())


# -------------------------------------------------------------------------------------------------------------- edge networks
EDGE_SHAPES = [(16, 16, 4), (48, 80, 33)]


def _edge(name, h1, h2, na, rs):
    """params, obs of one edge network (the network in float32, so the restatement sees exactly what the device sees)"""
    p = np.zeros(count(h1, h2, na), dtype=F)
    W1, b1, W2, b2, W3, b3 = views(p, h1, h2, na)
    n = 65
    x = rs.uniform(-1, 1, (n, 10)).astype(F)
    sub = lambda shape: (rs.randint(1, 1 << 22, shape) * rs.choice([-1, 1], shape)).astype(F) * TINY   # subnormals
    if name == 'zero_weights_signed_zero_biases':
        b1[:] = -0.0; b2[:] = -0.0
        b3[:] = rs.choice(np.array([-0.0, 0.0, 1.0, -2.5], F), na)
        x[0] = -0.0
    elif name == 'negative_zero_through_layer3':
        W1[:] = rs.normal(0, 0.3, W1.shape); W2[:] = rs.normal(0, 0.3, W2.shape)
        W3[:] = -0.0; b3[:] = -0.0                                  # fma(-0, a >= +0, -0) = -0 at every step
    elif name == 'subnormal_weights_observations_biases':
        W1[:] = sub(W1.shape); b1[:] = sub(b1.shape)                # subnormal A operands and C
        x[:, :5] = sub((n, 5))                                      # subnormal B operands
        W2[:] = rs.normal(0, 2.0 ** 100, W2.shape)                  # lifts the subnormal hidden units into the normals
        b2[:] = sub(b2.shape)
        W3[:] = sub(W3.shape) * F(2.0 ** 20); b3[:] = sub(b3.shape)
    elif name == 'products_underflow':
        W1[:] = rs.normal(0, 2.0 ** -70, W1.shape); x *= F(2.0 ** -70)     # products around 2^-140
        W2[:] = rs.normal(0, 2.0 ** 110, W2.shape)
        W3[:] = rs.normal(0, 2.0 ** -110, W3.shape)                         # y subnormal again
    elif name == 'sums_end_subnormal':
        x[:, 0] = 1.0
        W1[:, 0] = -(2.0 ** -126)
        b1[:] = rs.choice(np.array([1.5, 1.25, 1.0, 0.75], F), h1) * F(2.0 ** -126)   # 2^-127, 2^-128, 0, -2^-128
        W2[:] = rs.uniform(0.5, 1.0, W2.shape).astype(F) * F(2.0 ** 100)
        W3[:] = rs.uniform(-1, 1, W3.shape).astype(F) * F(2.0 ** -100 / (h1 * h2))
        b3[:] = F(2.0 ** -126) * rs.uniform(-1, 1, na).astype(F)           # ends near the normal/subnormal edge
    elif name == 'overflow_inf_times_zero_inf_minus_inf':
        # layer 1: units 1 mod 3 overflow to -inf -> relu +0; the rest are finite, about 2^100 (in an fma chain a finite
        # product is exact, so inf - inf needs an infinite operand: it comes from the layer before)
        x[:, 2] = 4.0
        x[:, 3] = rs.uniform(1, 2, n)
        j = np.arange(h1)
        W1[j[j % 3 == 1], 2] = -(2.0 ** 127)
        W1[j[j % 3 != 1], 3] = 2.0 ** 100
        W1[j[j % 3 != 1], 4] = rs.choice(np.array([0.0, 1.0, -1.0], F), int((j % 3 != 1).sum()))
        # layer 2: rows 0, 1 overflow to +inf (sums of 2^127 terms); the other rows stay finite
        W2[:2] = 2.0 ** 27
        W2[2:] = rs.choice(np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -10], F), (h2 - 2, h1))
        # layer 3: +-1 * inf -> +-inf, 0 * inf -> NaN, and inf - inf -> NaN on rows 3 mod 4
        W3[:, 0] = np.resize(np.array([1.0, -1.0, 0.0, 1.0, -1.0], F), na)
        W3[:, 1] = np.where(np.arange(na) % 4 == 3, -W3[:, 0], W3[:, 0])
        W3[:, 2:] = rs.choice(np.array([0.0, 1.0, -1.0, 2.0 ** -100], F), (na, h2 - 2))
        b3[:] = rs.normal(0, 1, na)
    elif name == 'nan_hidden_units_relu_to_plus_zero':
        # layer 1: units 0, 1 overflow to +inf; layer 2: every row takes 0 * inf or inf - inf, so every unit is NaN and relu
        # makes it +0; y = b3 + sum W3 * (+0), whose sign of zero follows W3 where b3 = -0
        x[:, 0] = 4.0
        W1[:2, 0] = 2.0 ** 127
        W1[2:] = rs.normal(0, 1, (h1 - 2, 10))
        W2[:] = rs.normal(0, 1, W2.shape)
        W2[0::2, 0] = 0.0
        W2[1::2, 0], W2[1::2, 1] = 1.0, -1.0
        W3[:] = rs.choice(np.array([1.0, -1.0, 0.0, -0.0], F), W3.shape)
        b3[:] = np.resize(np.array([-0.0, 0.0, 1.0, -0.0, -3.0], F), na)
    elif name == 'nan_and_inf_observations':
        W1[:] = rs.choice(np.array([0.0, -0.0, 0.5, -0.5, 1.0], F), W1.shape)
        W2[:] = rs.normal(0, 0.3, W2.shape); W3[:] = rs.normal(0, 0.3, W3.shape)
        b1[:] = rs.normal(0, 0.1, h1); b3[:] = rs.normal(0, 0.1, na)
        x[rs.rand(n, 10) < 0.1] = np.nan
        x[rs.rand(n, 10) < 0.1] = np.inf
        x[rs.rand(n, 10) < 0.1] = -np.inf
    else:
        raise KeyError(name)
    return p, x


def _is_sub(v):
    return np.isfinite(v) & (v != 0) & (np.abs(v) < 2.0 ** -126)


@pytest.mark.parametrize('h1,h2,na', EDGE_SHAPES)
@pytest.mark.parametrize('name', ['zero_weights_signed_zero_biases', 'negative_zero_through_layer3',
                                  'subnormal_weights_observations_biases', 'products_underflow', 'sums_end_subnormal',
                                  'overflow_inf_times_zero_inf_minus_inf', 'nan_hidden_units_relu_to_plus_zero',
                                  'nan_and_inf_observations'])
def test_edge_networks(qref, aref, name, h1, h2, na):
    rs = np.random.RandomState(7 + h1 + na + len(name))
    p, x = _edge(name, h1, h2, na, rs)
    y = check(qref, aref, p, x, h1, h2, na, name)
    # what each network exercises, seen in the restatement's (= the device's) output
    if name == 'zero_weights_signed_zero_biases':
        assert (y == views(p, h1, h2, na)[5]).all()
    elif name == 'negative_zero_through_layer3':
        assert (y == 0).all() and np.signbit(y).all()
    elif name == 'subnormal_weights_observations_biases':
        ftz = lambda v: np.where(_is_sub(v), F(0), v).astype(F)
        flushed = Q.forward(qref, ftz(x), ftz(p), h1, h2, na)          # what a build that flushes its inputs would give
        assert np.isfinite(y).all() and (y.view(np.int32) != flushed.view(np.int32)).mean() > 0.9
    elif name == 'products_underflow':
        assert np.isfinite(y).all() and (y != 0).mean() > 0.9 and _is_sub(y).any()   # flushed products would give y = 0
    elif name == 'sums_end_subnormal':
        W1, b1, _, _, _, b3 = views(p, h1, h2, na)
        assert _is_sub(b1 + W1[:, 0]).any()                          # exact: the first layer's sums end subnormal
        assert (y != b3).mean() > 0.9 and _is_sub(y).any()           # and are lifted into y; flushed they would leave y = b3
    elif name == 'overflow_inf_times_zero_inf_minus_inf':
        assert np.isposinf(y).any() and np.isneginf(y).any() and np.isnan(y).any()
    elif name == 'nan_hidden_units_relu_to_plus_zero':
        assert (y == views(p, h1, h2, na)[5]).all() and (np.signbit(y) != np.signbit(views(p, h1, h2, na)[5])).any()
    elif name == 'nan_and_inf_observations':
        assert np.isnan(y).any() and np.isfinite(y).any()


# ------------------------------------------------------------------------------------------------------- the k order is observable
@pytest.mark.parametrize('h1,h2,na', [(16, 16, 16), (48, 80, 33), (128, 112, 64), (112, 128, 10)])
def test_one_hot_weights_route_every_input(qref, aref, h1, h2, na):
    """unit j of each layer reads only input pi(j): y_j = x_{pi1(pi2(pi3(j)))} exactly (a packing that puts a weight at a
    wrong k or row routes a different input)"""
    rs = np.random.RandomState(h1 * h2 + na)
    p = np.zeros(count(h1, h2, na), dtype=F)
    W1, b1, W2, b2, W3, b3 = views(p, h1, h2, na)
    pi1 = np.concatenate([rs.permutation(10) for _ in range(h1 // 10 + 1)])[:h1]
    pi2 = np.concatenate([rs.permutation(h1) for _ in range(h2 // h1 + 1)])[:h2]
    pi3 = np.concatenate([rs.permutation(h2) for _ in range(na // h2 + 1)])[:na]
    W1[np.arange(h1), pi1] = 1.0
    W2[np.arange(h2), pi2] = 1.0
    W3[np.arange(na), pi3] = 1.0
    x = rs.uniform(0.5, 2.0, (257, 10)).astype(F)
    y = check(qref, aref, p, x, h1, h2, na, 'one-hot')
    same(y, x[:, pi1[pi2[pi3]]], 'one-hot routing')


@pytest.mark.parametrize('h1,h2,na', [(16, 16, 4), (48, 80, 33), (128, 128, 64)])
def test_cancellation_shows_ascending_k(qref, aref, h1, h2, na):
    """b = 1, then +2^24 at k = a and -2^24 at k = b > a: 1 + 2^24 rounds to 2^24 (tie to even), so ascending k gives 0 and
    the other order gives 1; with the signs swapped ascending gives 1.  Pairs within one k-step, across k-steps and across
    the 16-row groups of the fragment, in every layer; the other layers pass the result through one-hot weights of 1."""
    p = np.zeros(count(h1, h2, na), dtype=F)
    W1, b1, W2, b2, W3, b3 = views(p, h1, h2, na)
    big = F(2.0 ** 24)
    x = np.ones((64, 10), dtype=F)
    pairs1 = [(0, 1), (2, 3), (3, 4), (0, 9), (5, 8), (4, 7), (1, 6), (7, 9)]
    # layer 1: unit j cancels inputs pairs1[j % 8]; layer 2 / 3 pass unit j through (y_j = a1_j for j < 8)
    for j in range(min(h1, 16)):
        a, b = pairs1[j % 8]
        W1[j, a], W1[j, b] = (big, -big) if j < 8 else (-big, big)
        b1[j] = 1.0
    W2[np.arange(min(h1, h2)), np.arange(min(h1, h2))] = 1.0
    W3[np.arange(min(na, h2)), np.arange(min(na, h2))] = 1.0
    y = check(qref, aref, p, x, h1, h2, na, 'layer-1 cancellation')
    m = min(na, 16, h1, h2)
    assert (y[:, :min(m, 8)] == 0).all() and (y[:, 8:m] == 1).all()
    # layer 2 / layer 3: every hidden unit of the previous layer is 1 (bias 1, zero weights); rows cancel k pairs
    for layer in (2, 3):
        p = np.zeros(count(h1, h2, na), dtype=F)
        W1, b1, W2, b2, W3, b3 = views(p, h1, h2, na)
        b1[:] = 1.0
        K, rows = (h1, h2) if layer == 2 else (h2, na)
        W = W2 if layer == 2 else W3
        bb = b2 if layer == 2 else b3
        rs = np.random.RandomState(layer * 100 + K)
        want = np.zeros(rows, F)
        for j in range(rows):
            a, b = sorted(rs.choice(K, 2, replace=False))
            up = j % 2 == 0
            W[j, a], W[j, b] = (big, -big) if up else (-big, big)
            bb[j] = 1.0
            want[j] = 0.0 if up else 1.0
        if layer == 2:                                                 # y_j = a2_j for j < min(na, h2), else 0
            W3[np.arange(min(na, h2)), np.arange(min(na, h2))] = 1.0
            want = np.concatenate([want[:min(na, h2)], np.zeros(max(na - h2, 0), F)])
        else:
            b2[:] = 1.0
        y = check(qref, aref, p, x, h1, h2, na, f'layer-{layer} cancellation')
        same(y, np.tile(want, (x.shape[0], 1)), f'layer-{layer} ascending k')


# ---------------------------------------------------------------------------------------------------- argmax edges on the device
def _const_net(h1, h2, na, q):
    """y = q for every env: zero W3 (fma(0, a >= +0 finite, q) = q) and b3 = q"""
    p = np.zeros(count(h1, h2, na), dtype=F)
    views(p, h1, h2, na)[5][:] = q
    return p


@pytest.mark.parametrize('na,q,best', [
    (17, {15: 3.0, 16: 3.0}, 15),                                   # tie across the tile boundary: the lower row
    (17, {16: 3.0}, 16),                                            # the best action in the second tile's first row
    (33, {16: 2.0, 32: 2.5}, 32),
    (17, {0: np.nan, 16: 9.0}, 0),                                  # a NaN q[0] is never replaced
    (17, {5: np.nan, 9: 4.0}, 9),                                   # a NaN elsewhere never wins
    (16, {3: np.nan, 4: np.nan}, 0),
    (33, {'all': -np.inf, 21: -1e30}, 21),                          # all -inf but one
    (33, {'all': -np.inf}, 0),
    (64, {'all': 1.0}, 0),
])
def test_argmax_edges(qref, aref, na, q, best):
    qv = np.zeros(na, F)
    if 'all' in q:
        qv[:] = q['all']
    for k, v in q.items():
        if k != 'all':
            qv[k] = v
    for h1, h2 in ((16, 16), (48, 80)):
        rs = np.random.RandomState(na)
        x = random_obs(rs, 65)
        p = _const_net(h1, h2, na, qv)
        check(qref, aref, p, x, h1, h2, na, 'argmax')
        _, g, _ = device_forward(p, x, h1, h2, na)
        assert (g == best).all(), (g[:4], best)


def test_argmax_ties_between_computed_rows(qref, aref):
    """rows 15 and 16 read the same hidden unit: per env a computed tie across the tile boundary, resolved to row 15"""
    h1, h2, na = 48, 80, 17
    rs = np.random.RandomState(3)
    p = random_net(rs, h1, h2, na)
    W3, b3 = views(p, h1, h2, na)[4:]
    W3[:] = 0.0
    b3[:] = 0.0
    W3[np.arange(na), rs.permutation(h2)[:na]] = 1.0
    W3[16] = W3[15]
    x = random_obs(rs, 1000)
    y = check(qref, aref, p, x, h1, h2, na, 'computed ties')
    _, g, _ = device_forward(p, x, h1, h2, na)
    assert (y[:, 15] == y[:, 16]).all() and (g == 15).sum() > 10 and not (g == 16).any()


# ------------------------------------------------------------------------------------------------------------------ rejections
def test_rejections():
    from soccer2d_amd import _capi
    lib = _capi.load_library()
    big = torch.zeros(count(128, 128, 64) + 64, dtype=torch.float32, device='cuda:0')
    obs = torch.zeros(64, 10, device='cuda:0')
    y = torch.zeros(64, 64, device='cuda:0')
    g = torch.zeros(64, dtype=torch.int32, device='cuda:0')
    ok = dict(h1=64, h2=64, na=16, p=big.data_ptr(), x=obs.data_ptr(), n=64, y=y.data_ptr(), g=g.data_ptr())
    bad = [dict(h1=40), dict(h1=0), dict(h2=144), dict(h2=8), dict(na=0), dict(na=65), dict(n=0), dict(n=-1),
           dict(p=None), dict(p=big.data_ptr() + 4), dict(x=None), dict(y=None), dict(g=None), dict(x=obs.data_ptr() + 2)]
    for b in bad:
        a = dict(ok, **b)
        rc = lib.s2d_debug_net_forward(a['h1'], a['h2'], a['na'], a['p'], a['x'], a['n'], a['y'], a['g'], None, None)
        assert rc == _capi.S2D_EINVAL, b
    torch.cuda.synchronize()
    assert not y.any() and not g.any()


# ---------------------------------------------------------------------------------------------------- the debug path = the rollout
def _q_engine(n, na):
    from soccer2d_amd.engine import Engine, make_config
    kw = dict(O.DQN_KWARGS)
    kw['action_space_size'] = na
    return Engine(n, 'cuda:0', cfg=make_config(noise=True, **kw))


@pytest.mark.parametrize('h1,h2,na', [(48, 80, 33), (112, 96, 17)])
def test_qnet_rollout_acts_with_the_debug_network(qref, aref, h1, h2, na):
    from soccer2d_amd.actor import QNetActor
    n, T = 1000, 12
    eng = _q_engine(n, na)
    eng.reset()
    rs = np.random.RandomState(h1 + h2)
    actor = QNetActor(h1, h2, na, device='cuda:0', epsilon=0.0)
    actor.params.copy_(torch.from_numpy(random_net(rs, h1, h2, na)))
    params = actor.params.cpu().numpy()
    obs0 = eng.obs.cpu().numpy()
    r = eng.rollout_qnet(T, actor)
    torch.cuda.synchronize()
    xs = np.concatenate([obs0[None], r['obs'][:-1].cpu().numpy()])
    acts = r['action'].cpu().numpy()
    for t in range(T):
        _, g, _ = device_forward(params, xs[t], h1, h2, na)
        same(g, acts[t], f'action[{t}]')
    assert len(np.unique(acts)) > 3


@pytest.mark.parametrize('mode,h1,h2', [('cont1', 48, 80), ('turn4', 112, 96), ('cont1', 80, 112)])
def test_tanh_rollout_acts_with_the_debug_network(qref, aref, mode, h1, h2):
    from soccer2d_amd.actor import DeterministicActor
    from soccer2d_amd.engine import Engine, make_config
    na = 4 if mode == 'turn4' else 1
    n, T = 1000, 12
    kw = dict(O.DQN_KWARGS)
    kw.update(use_continuous_action=True, use_turning=mode == 'turn4')
    eng = Engine(n, 'cuda:0', cfg=make_config(noise=True, **kw))
    eng.reset()
    rs = np.random.RandomState(h1 + h2 + na)
    actor = DeterministicActor(h1, h2, na, device='cuda:0', epsilon=0.0)
    actor.params.copy_(torch.from_numpy(random_net(rs, h1, h2, na)))
    params = actor.params.cpu().numpy()
    obs0 = eng.obs.cpu().numpy()
    r = eng.rollout_actor(T, actor)
    torch.cuda.synchronize()
    xs = np.concatenate([obs0[None], r['obs'][:-1].cpu().numpy()])
    acts = r['action'].cpu().numpy().reshape(T, n, na)
    for t in range(T):
        y, _, _ = device_forward(params, xs[t], h1, h2, na)
        same(y, R.forward(aref, xs[t], params, h1, h2, na), f'y[{t}]')
        same(R.tanh(aref, y).reshape(n, na), acts[t], f'action[{t}]')
    assert len(np.unique(acts)) > 100
