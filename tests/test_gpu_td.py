"""The TD-target kernels (s2d_td_target_q / s2d_td_target_ac; soccer2d_amd.td QTarget / ActorCriticTarget) on the GPU, every
comparison bit for bit: against the host restatement (tests/td_ref.c) at every k-step pattern, hidden shape, activation, output
count and batch edge, with and without the online network and the optional outputs; against the fused actors' own forward kernels
at n_in = 10 and n_in = 4; on special values; Double DQN; DDPG / TD3; under every plan that fits; through the classes on a
DeviceReplay batch; in one captured graph with the sample; and every rejection, which launches nothing.  Every output and every
workspace is allocated with sentinel guard words past its end, and the guards are checked."""
import ctypes as C

import numpy as np
import pytest

import replay as RR
import td as TD

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
nn = torch.nn

F = np.float32
DEV = 'cuda:0'
PAD = 64                     # guard words past every output and workspace
S_F, S_I = -7777.0, -5       # their sentinels
ACT_NN = {'relu': nn.ReLU, 'tanh': nn.Tanh, 'sigmoid': nn.Sigmoid}
ACTS = ('relu', 'tanh', 'sigmoid')


@pytest.fixture(scope='module')
def L(tmp_path_factory):
    return TD.build(tmp_path_factory.mktemp('td_ref'))


@pytest.fixture(scope='module')
def lib():
    from soccer2d_amd import _capi
    return _capi.load_library()


# ------------------------------------------------------------------------------------------------------------------ helpers
def same(got, want, what):
    """bit for bit, the sign of zero included; where both are NaN only that they are NaN"""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = want.detach().cpu().numpy() if torch.is_tensor(want) else np.asarray(want)
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


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class DevNet:
    """a tests/td.py Net on the device: its parameters, a workspace of exactly the bytes the library asks for with guard words
    behind it, and the S2DTdNet of both"""

    def __init__(self, lib, net):
        from soccer2d_amd import _capi
        self.net = net
        self.params = to_dev(net.params)
        s = _capi.S2DTdNet()
        s.n_in, s.n_hidden, s.n_out, s.activation = net.n_in, len(net.hidden), net.n_out, TD.ACT[net.act]
        for l, w in enumerate(net.hidden):
            s.hidden[l] = w
        self.words = lib.s2d_td_workspace_bytes(C.byref(s)) // 4
        assert self.words > 0
        self.ws = torch.full((self.words + PAD,), -3333.0, dtype=torch.float32, device=DEV)
        s.params, s.workspace, s.workspace_bytes = self.params.data_ptr(), self.ws.data_ptr(), self.words * 4
        self.s = s

    def ref(self):
        return C.byref(self.s)

    def check_guard(self):
        assert bool((self.ws[self.words:] == -3333.0).all()), 'wrote past the workspace'


def _out(B, tail=(), dtype=torch.float32):
    return torch.full((B + PAD,) + tail, S_I if dtype == torch.int32 else S_F, dtype=dtype, device=DEV)


def _take(t, B, what):
    h = t.cpu().numpy()
    assert (h[B:] == (S_I if h.dtype == np.int32 else F(S_F))).all(), f'{what}: wrote past the batch'
    return h[:B]


def run_q(lib, tgt, onl, x, r, d, with_q=True, with_index=True):
    """s2d_td_target_q on device copies: (target, q or None, index or None), guards checked"""
    from soccer2d_amd import _capi
    B = x.shape[0]
    xt, rt, dt = to_dev(x.astype(F)), to_dev(r.astype(F)), to_dev(d.astype(F))
    t, q, i = _out(B), (_out(B) if with_q else None), (_out(B, dtype=torch.int32) if with_index else None)
    torch.cuda.synchronize()
    rc = lib.s2d_td_target_q(B, tgt.ref(), onl.ref() if onl is not None else None, xt.data_ptr(), rt.data_ptr(), dt.data_ptr(), t.data_ptr(),
                             q.data_ptr() if with_q else None, i.data_ptr() if with_index else None, None)
    _capi.check(lib, rc, 's2d_td_target_q')
    torch.cuda.synchronize()
    for n in (tgt, onl):
        if n is not None:
            n.check_guard()
    return _take(t, B, 'target'), (_take(q, B, 'q') if with_q else None), (_take(i, B, 'index') if with_index else None)


def run_ac(lib, actor, c1, c2, x, r, d, with_q=True, with_action=True):
    """s2d_td_target_ac on device copies: (target, q or None, action or None), guards checked"""
    from soccer2d_amd import _capi
    B, A = x.shape[0], actor.net.n_out
    xt, rt, dt = to_dev(x.astype(F)), to_dev(r.astype(F)), to_dev(d.astype(F))
    t, q, a = _out(B), (_out(B) if with_q else None), (_out(B, (A,)) if with_action else None)
    torch.cuda.synchronize()
    rc = lib.s2d_td_target_ac(B, actor.ref(), c1.ref(), c2.ref() if c2 is not None else None, xt.data_ptr(), rt.data_ptr(), dt.data_ptr(),
                              t.data_ptr(), q.data_ptr() if with_q else None, a.data_ptr() if with_action else None, None)
    _capi.check(lib, rc, 's2d_td_target_ac')
    torch.cuda.synchronize()
    for n in (actor, c1, c2):
        if n is not None:
            n.check_guard()
    return _take(t, B, 'target'), (_take(q, B, 'q') if with_q else None), (_take(a, B, 'action') if with_action else None)


def batch_of(rs, B, D):
    """rows in and a little outside the observation range, rewards, and discounts of which a fifth are 0 (terminations)"""
    x = rs.uniform(-1, 1, (B, D))
    x[::5] *= 30
    return x.astype(F), rs.uniform(-2, 2, B).astype(F), np.where(rs.rand(B) < 0.2, 0.0, 0.970299).astype(F)


# ------------------------------------------------------------------------------------------------- against the restatement
# every n_in of {1, 3, 4, 10, 11, 14, 21, 25, 36, 224, 256} (k-steps 1, 1, 1, 3, 3, 4, 6, 7, 9, 56, 64: every group pattern), every
# hidden shape with every activation, every n_out of {1, 16, 17, 64}, every B of {1, 63, 64, 65, 257}; the edges together:
# n_in = 256 with [8] (the input row wider than the hidden image), [400, 300] with B = 65
Q_CASES = [
    (256, (8,), 64, 'relu', 257), (1, (8,), 1, 'tanh', 1), (3, (8,), 17, 'sigmoid', 63),
    (11, (12, 20), 17, 'relu', 65), (14, (12, 20), 16, 'tanh', 64), (21, (12, 20), 1, 'sigmoid', 257),
    (10, (64, 64), 16, 'relu', 257), (224, (64, 64), 16, 'tanh', 65), (25, (64, 64), 64, 'sigmoid', 63),
    (36, (128, 64, 32, 16), 17, 'relu', 64), (4, (128, 64, 32, 16), 16, 'tanh', 1), (256, (128, 64, 32, 16), 1, 'sigmoid', 65),
    (10, (400, 300), 16, 'relu', 65), (21, (400, 300), 64, 'tanh', 65), (224, (400, 300), 17, 'sigmoid', 63),
]


def test_cases_cover_every_axis_value():
    assert {c[0] for c in Q_CASES} == {1, 3, 4, 10, 11, 14, 21, 25, 36, 224, 256}
    assert {(c[1], c[3]) for c in Q_CASES} == {(h, a) for h in ((8,), (12, 20), (64, 64), (128, 64, 32, 16), (400, 300)) for a in ACTS}
    assert {c[2] for c in Q_CASES} == {1, 16, 17, 64} and {c[4] for c in Q_CASES} == {1, 63, 64, 65, 257}
    assert (256, (8,)) in {(c[0], c[1]) for c in Q_CASES} and ((400, 300), 65) in {(c[1], c[4]) for c in Q_CASES}


@pytest.mark.parametrize('n_in,hidden,na,act,B', Q_CASES, ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_q_target_equals_the_restatement(L, lib, n_in, hidden, na, act, B):
    rs = np.random.RandomState(n_in * 1000 + na + B)
    tgt = TD.random_net(rs, n_in, hidden, na, act, gain=2.0)
    # the online network has another hidden shape and another activation
    onl = TD.random_net(rs, n_in, (20, 12), na, ACTS[(ACTS.index(act) + 1) % 3], gain=2.0)
    x, r, d = batch_of(rs, B, n_in)
    dt, do = DevNet(lib, tgt), DevNet(lib, onl)
    for online, dev_onl in ((None, None), (onl, do)):
        want = TD.target_q(L, tgt, online, x, r, d)
        what = f'{"double " if online else ""}dqn {n_in}-{hidden}-{na} {act} B={B}'
        got = run_q(lib, dt, dev_onl, x, r, d)
        for g, w, name in zip(got, want, ('target', 'q', 'index')):
            same(g, w, f'{what} {name}')
        # the optional outputs: both NULL, and one of each
        for wq, wi in ((False, False), (True, False), (False, True)):
            g = run_q(lib, dt, dev_onl, x, r, d, with_q=wq, with_index=wi)
            same(g[0], want[0], f'{what} target (q={wq}, index={wi})')
            if wq:
                same(g[1], want[1], f'{what} q alone')
            if wi:
                same(g[2], want[2], f'{what} index alone')
    assert len(np.unique(want[0])) > B // 2


# ----------------------------------------------------------------------------------------------- same function as the actors
@pytest.mark.parametrize('hidden,act', [((64, 64), 'relu'), ((400, 300), 'tanh'), ((12, 20, 28), 'sigmoid')])
def test_same_function_as_the_reach_ball_actor(L, lib, hidden, act):
    """n_in = 10: out_q / out_index are y[greedy] / greedy of s2d_debug_wide_forward on the same parameters and rows"""
    from test_gpu_wide_actor import device_forward
    rs = np.random.RandomState(len(hidden))
    net = TD.random_net(rs, 10, hidden, 16, act, gain=2.0)
    x, r, d = batch_of(rs, 130, 10)
    y, greedy, _ = device_forward(net.params, x, hidden, 16, act)
    _, q, idx = run_q(lib, DevNet(lib, net), None, x, r, d)
    same(idx, greedy, 'index against the actor\'s greedy')
    same(q, y[np.arange(130), greedy], 'q against the actor\'s y[greedy]')


@pytest.mark.parametrize('hidden,act', [((16, 8), 'relu'), ((64, 64), 'tanh')])
def test_same_function_as_the_go_to_center_actor(L, lib, hidden, act):
    """n_in = 4: the same against s2d_gtc_debug_forward (GtcQNetActor's network: one k-step, no zero pad)"""
    from test_gpu_gtc_actor import device_forward
    rs = np.random.RandomState(4 + len(hidden))
    net = TD.random_net(rs, 4, hidden, 16, act, gain=2.0)
    x, r, d = batch_of(rs, 130, 4)
    net.params[4 * hidden[0]:4 * hidden[0] + 4] = -0.0                       # -0 biases stay -0 without the pad
    x[1] = 0.0
    y, greedy, _ = device_forward(net.params, x, hidden, 16, act)
    _, q, idx = run_q(lib, DevNet(lib, net), None, x, r, d)
    same(idx, greedy, 'index against the actor\'s greedy')
    same(q, y[np.arange(130), greedy], 'q against the actor\'s y[greedy]')


# ------------------------------------------------------------------------------------------------------------ special values
def const_net(n_in, b_out, act='relu'):
    """zero weights, zero hidden biases: every row's outputs are the output layer's biases"""
    b_out = np.atleast_1d(np.asarray(b_out, F))
    p = np.zeros(TD.param_count(n_in, (8,), b_out.size), F)
    p[-b_out.size:] = b_out
    return TD.Net(n_in, (8,), b_out.size, act, p)


def test_special_values_equal_the_restatement(L, lib):
    nan, inf = np.nan, np.inf
    x = np.zeros((6, 3), F)
    r = np.array([1.0, -0.0, 0.0, -0.0, inf, 2.5], F)
    d = np.array([1.0, 0.0, -0.0, 0.99, 0.0, 0.0], F)
    outs = ([1, 3, 3, 2, 3], [nan, 1, 2, nan, 0], [1, nan, 2, 2, nan], [nan] * 5, [-inf, inf, inf, 0, 1], [-inf] * 5, [inf] * 5,
            [0.0, -0.0, 0.0, -0.0, 0.0], [-0.0, 0.0, 0.0, 0.0, 0.0], [-2, -3, -3, -3, -3], [3e38, 3e38, -3e38, 1e-45, -1e-45])
    want_index = (1, 0, 2, 0, 1, 0, 0, 0, 0, 0, 0)
    for b, wi in zip(outs, want_index):
        net = const_net(3, b)
        want = TD.target_q(L, net, None, x, r, d)
        assert (want[2] == wi).all(), (b, want[2])                          # ties: the lowest index; a NaN never becomes the best
        got = run_q(lib, DevNet(lib, net), None, x, r, d)
        for g, w, name in zip(got, want, ('target', 'q', 'index')):
            same(g, w, f'outputs {b}: {name}')
    # discount = 0 with an infinite q is NaN, with a finite q the reward (and -0 + +0 = +0)
    t, _, _ = run_q(lib, DevNet(lib, const_net(3, [inf, 0, 0])), None, x, r, d)
    assert np.isnan(t[1]) and np.isnan(t[5]) and np.isinf(t[0])
    t, _, _ = run_q(lib, DevNet(lib, const_net(3, [2.0, 0, 0])), None, x, r, d)
    same(t, TD.target_q(L, const_net(3, [2.0, 0, 0]), None, x, r, d)[0], 'finite q')
    assert t[1].view(np.int32) == 0 and t[5] == 2.5 and t[4] == inf         # -0 + (0 * 2) = +0; the reward alone; inf + 0
    # special rows through a real network, both kernels
    rs = np.random.RandomState(5)
    xs = rs.uniform(-1, 1, (70, 10)).astype(F)
    xs[0], xs[1], xs[2] = 0.0, -0.0, 1e-40
    xs[3] = [inf, -inf, nan, 3e38, -3e38, 1.0, -1.0, 1e-45, 0.5, -0.5]
    xs[4, 2], xs[5, 9], xs[66, 0] = nan, inf, -inf
    rr, dd = rs.uniform(-1, 1, 70).astype(F), np.full(70, 0.99, F)
    rr[7], rr[8], dd[9], dd[10], dd[5] = inf, nan, inf, nan, 0.0
    for act in ACTS:
        for scale in (1.0, 1e19):
            tgt, onl = TD.random_net(rs, 10, (12, 20), 17, act, gain=scale), TD.random_net(rs, 10, (64,), 17, act, gain=scale)
            for g, w, name in zip(run_q(lib, DevNet(lib, tgt), DevNet(lib, onl), xs, rr, dd), TD.target_q(L, tgt, onl, xs, rr, dd),
                                  ('target', 'q', 'index')):
                same(g, w, f'special rows {act} x{scale}: {name}')
            actor = TD.random_net(rs, 10, (16, 8), 2, act, gain=scale)
            c1, c2 = TD.random_net(rs, 12, (12, 20), 1, act, gain=scale), TD.random_net(rs, 12, (64,), 1, act, gain=scale)
            for g, w, name in zip(run_ac(lib, DevNet(lib, actor), DevNet(lib, c1), DevNet(lib, c2), xs, rr, dd),
                                  TD.target_ac(L, actor, c1, c2, xs, rr, dd), ('target', 'q', 'action')):
                same(g, w, f'special rows actor-critic {act} x{scale}: {name}')
    # the twin minimum: a NaN in q2 never replaces q1, a NaN in q1 stays
    actor = const_net(3, [0.5])
    for b1, b2 in ((1.0, 2.0), (2.0, 1.0), (1.0, nan), (nan, 1.0), (-inf, 0.0), (0.0, -0.0), (-0.0, 0.0)):
        c1, c2 = const_net(4, [b1]), const_net(4, [b2])
        want = TD.target_ac(L, actor, c1, c2, x, r, d)
        for g, w, name in zip(run_ac(lib, DevNet(lib, actor), DevNet(lib, c1), DevNet(lib, c2), x, r, d), want, ('target', 'q', 'action')):
            same(g, w, f'twin {b1} {b2}: {name}')


# ---------------------------------------------------------------------------------------------------------------- Double DQN
def test_double_dqn_takes_the_target_value_at_the_online_index(L, lib):
    rs = np.random.RandomState(21)
    B = 200
    tgt, onl = TD.random_net(rs, 10, (64, 64), 16, 'relu', gain=2.0), TD.random_net(rs, 10, (64, 64), 16, 'relu', gain=2.0)
    x, r, d = batch_of(rs, B, 10)
    y_t, y_o = TD.forward(L, tgt, x), TD.forward(L, onl, x)
    plain = TD.target_q(L, tgt, None, x, r, d)
    want = TD.target_q(L, tgt, onl, x, r, d)
    assert (plain[2] != want[2]).sum() >= B // 2                            # the two argmax differ on at least half of the rows
    assert np.array_equal(want[2], y_o.argmax(axis=1)) and np.array_equal(TD.bits(want[1]), TD.bits(y_t[np.arange(B), want[2]]))
    got = run_q(lib, DevNet(lib, tgt), DevNet(lib, onl), x, r, d)
    for g, w, name in zip(got, want, ('target', 'q', 'index')):
        same(g, w, f'double dqn {name}')
    same(got[1], y_t[np.arange(B), got[2]], 'q is the target network\'s value at the online index')


# -------------------------------------------------------------------------------------------------------------- actor-critic
AC_CASES = [(4, 1, (16, 8), (64, 32, 16, 8), 'relu', 257), (10, 2, (64, 64), (64, 64), 'tanh', 65), (224, 4, (12, 20), (128, 64), 'sigmoid', 63),
            (10, 8, (400, 300), (64, 64), 'relu', 65), (4, 8, (8,), (8,), 'tanh', 1), (224, 1, (64, 64), (400, 300), 'relu', 64),
            (10, 1, (400, 300), (64, 64), 'sigmoid', 130), (10, 4, (16, 8), (12, 20), 'tanh', 64)]


@pytest.mark.parametrize('D,A,pi,qf,act,B', AC_CASES, ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_actor_critic_target_equals_the_restatement(L, lib, D, A, pi, qf, act, B):
    rs = np.random.RandomState(D * 100 + A + B)
    actor = TD.random_net(rs, D, pi, A, act, gain=2.0)
    c1, c2 = TD.random_net(rs, D + A, qf, 1, act, gain=2.0), TD.random_net(rs, D + A, qf[::-1], 1, ACTS[(ACTS.index(act) + 1) % 3], gain=2.0)
    x, r, d = batch_of(rs, B, D)
    # the second critic's output bias is moved by the median difference, so that each critic is the smaller on about half the rows
    gap = TD.target_ac(L, actor, c1, None, x, r, d)[1] - TD.target_ac(L, actor, c2, None, x, r, d)[1]
    c2.params[-1] += F(np.median(gap))
    da, d1, d2 = DevNet(lib, actor), DevNet(lib, c1), DevNet(lib, c2)
    y = TD.forward(L, actor, x)
    for twin, dev2 in ((None, None), (c2, d2)):
        want = TD.target_ac(L, actor, c1, twin, x, r, d)
        what = f'{"td3" if twin else "ddpg"} {D}+{A} pi{pi} qf{qf} {act} B={B}'
        if twin is not None and B >= 63:                                     # each critic is the smaller on at least a quarter of the rows
            q1 = TD.target_ac(L, actor, c1, None, x, r, d)[1]
            q2 = TD.target_ac(L, actor, c2, None, x, r, d)[1]
            assert (q1 < q2).sum() >= B // 4 and (q2 < q1).sum() >= B // 4, ((q1 < q2).sum(), (q2 < q1).sum())
            same(want[1], np.minimum(q1, q2), f'{what}: the restatement\'s minimum')
        got = run_ac(lib, da, d1, dev2, x, r, d)
        for g, w, name in zip(got, want, ('target', 'q', 'action')):
            same(g, w, f'{what} {name}')
        same(got[2], tanh_spec(L, y), f'{what}: the action is tanh_spec of the actor\'s output')
        for wq, wa in ((False, False), (True, False), (False, True)):
            g = run_ac(lib, da, d1, dev2, x, r, d, with_q=wq, with_action=wa)
            same(g[0], want[0], f'{what} target (q={wq}, action={wa})')
            if wa:
                same(g[2], want[2], f'{what} action alone')


def tanh_spec(L, v):
    """tanh_spec of every element (actor_ref.c's actor_tanh, inside the restatement's library)"""
    v = np.ascontiguousarray(v, dtype=F)
    out = np.zeros_like(v)
    L.actor_tanh.restype, L.actor_tanh.argtypes = None, [C.c_int64, C.c_void_p, C.c_void_p]
    L.actor_tanh(v.size, v.ctypes.data, out.ctypes.data)
    return out


def test_ac_cases_cover_the_axes():
    assert {c[1] for c in AC_CASES} == {1, 2, 4, 8} and {c[0] for c in AC_CASES} == {4, 10, 224}


# --------------------------------------------------------------------------------------------------------- plan independence
def plan_fits(wmax, n_in, na, waves, tiles):
    """the layout of s2d_td.hip's head: per wave T x 16 rows of the input image and of two hidden images, and the output image"""
    rp, xp, qp = (wmax + 63) // 64 * 64 + 4, ((n_in + 3) // 4 * 4 + 63) // 64 * 64 + 4, (na + 15) // 16 * 16 + 4
    return waves * (tiles * 16 * (xp + 2 * rp) + 64 * qp) * 4 <= 160 * 1024


def test_results_do_not_depend_on_the_plan(L, lib, monkeypatch):
    """S2D_TD_PLAN=waves,tiles (read at every launch): one shape per kernel under every pair; those that fit give the same
    bits, the others are refused by name"""
    from soccer2d_amd import _capi
    rs = np.random.RandomState(3)
    B = 300
    tgt, onl = TD.random_net(rs, 21, (28, 136), 17, 'tanh', gain=2.0), TD.random_net(rs, 21, (12,), 17, 'relu', gain=2.0)
    actor = TD.random_net(rs, 10, (28, 136), 4, 'relu', gain=2.0)
    c1, c2 = TD.random_net(rs, 14, (64, 64), 1, 'relu', gain=2.0), TD.random_net(rs, 14, (20,), 1, 'sigmoid', gain=2.0)
    x, r, d = batch_of(rs, B, 21)
    xa = x[:, :10].copy()
    want_q, want_ac = TD.target_q(L, tgt, onl, x, r, d), TD.target_ac(L, actor, c1, c2, xa, r, d)
    dq, da = (DevNet(lib, tgt), DevNet(lib, onl)), (DevNet(lib, actor), DevNet(lib, c1), DevNet(lib, c2))
    ran = 0
    for waves in (4, 2, 1):
        for tiles in (4, 2, 1):
            monkeypatch.setenv('S2D_TD_PLAN', f'{waves},{tiles}')
            fits = plan_fits(144, 21, 17, waves, tiles)                     # 136 padded to its tiles' 144
            try:
                got = run_q(lib, dq[0], dq[1], x, r, d)
                assert fits
                ran += 1
                for g, w, name in zip(got, want_q, ('target', 'q', 'index')):
                    same(g, w, f'plan {waves},{tiles} q {name}')
            except ValueError as e:
                assert not fits and 'S2D_TD_PLAN' in str(e) and 's2d_td_target_q' in str(e), (waves, tiles, str(e))
            try:
                got = run_ac(lib, *da, xa, r, d)
                assert plan_fits(144, 14, 4, waves, tiles)
                for g, w, name in zip(got, want_ac, ('target', 'q', 'action')):
                    same(g, w, f'plan {waves},{tiles} ac {name}')
            except ValueError as e:
                assert not plan_fits(144, 14, 4, waves, tiles) and 'S2D_TD_PLAN' in str(e), (waves, tiles, str(e))
    assert ran >= 6
    for bad in ('3,1', '4', 'x', '0,8'):
        monkeypatch.setenv('S2D_TD_PLAN', bad)
        with pytest.raises(ValueError, match='S2D_TD_PLAN'):
            run_q(lib, dq[0], None, x, r, d)
    monkeypatch.delenv('S2D_TD_PLAN')
    for g, w, name in zip(run_q(lib, dq[0], dq[1], x, r, d), want_q, ('target', 'q', 'index')):
        same(g, w, f'the plan\'s own choice: {name}')
    assert _capi.S2D_ABI_VERSION == 4


# ------------------------------------------------------------------------------------------------------- through the classes
def seq(n_in, hidden, n_out, act='relu', tanh_head=False):
    layers, win = [], n_in
    for w in hidden:
        layers += [nn.Linear(win, w), ACT_NN[act]()]
        win = w
    layers.append(nn.Linear(win, n_out))
    if tanh_head:
        layers.append(nn.Tanh())
    return nn.Sequential(*layers).to(DEV)


def net_of(module, act):
    lin = [m for m in module if isinstance(m, nn.Linear)]
    p = np.concatenate([np.concatenate([l.weight.detach().cpu().numpy().ravel(), l.bias.detach().cpu().numpy().ravel()]) for l in lin])
    return TD.Net(lin[0].in_features, [l.out_features for l in lin[:-1]], lin[-1].out_features, act, p)


def dev_rec(rec):
    return {k: torch.from_numpy(v).to(DEV) for k, v in rec.items() if v is not None}


def host(batch):
    return [batch[k].cpu().numpy() for k in ('next_obs', 'reward', 'discount')]


def test_qtarget_on_a_replay_batch(L):
    from soccer2d_amd.replay import DeviceReplay
    from soccer2d_amd.td import QTarget
    torch.manual_seed(1)
    rng = np.random.default_rng(1)
    rb = DeviceReplay(512, 10, device=DEV, n_step=3, seed=5)
    rec, first = RR.synthetic_record(rng, 4, 60, 10, 1)
    rb.push(dev_rec(rec), torch.from_numpy(first).to(DEV))
    batch = rb.sample(96)
    qt, qo = seq(10, (64, 64), 16), seq(10, (32,), 16, 'tanh')
    for online in (None, qo):
        t = QTarget.from_module(qt, online=online)
        assert t.device == torch.device(DEV)
        h_online = net_of(qo, 'tanh') if online is not None else None
        want = TD.target_q(L, net_of(qt, 'relu'), h_online, *host(batch))
        same(t.target(batch), want[0], 'target')
        got = t.target(batch, return_q=True)
        assert got[0].dtype == torch.float32 and got[2].dtype == torch.int32 and tuple(got[1].shape) == (96,)
        for g, w, name in zip(got, want, ('target', 'q', 'index')):
            same(g, w, f'return_q {name}')
        out = torch.full((96,), S_F, device=DEV)
        assert t.target(batch, out=out) is out
        same(out, want[0], 'out=')
        with torch.no_grad():                                                # an in-place change of the target module
            qt[2].weight.add_(0.05)
            qt[4].bias.mul_(-1.0)
        same(t.target(batch), want[0], 'without sync() nothing changes')
        t.sync()
        changed = TD.target_q(L, net_of(qt, 'relu'), h_online, *host(batch))
        assert not np.array_equal(TD.bits(changed[0]), TD.bits(want[0]))
        same(t.target(batch), changed[0], 'after sync()')


def test_actor_critic_target_on_a_replay_batch(L):
    from soccer2d_amd.replay import DeviceReplay
    from soccer2d_amd.td import ActorCriticTarget
    torch.manual_seed(2)
    rng = np.random.default_rng(2)
    rb = DeviceReplay(512, 10, action_words=2, action_dtype=torch.float32, device=DEV, seed=6)
    rec, first = RR.synthetic_record(rng, 4, 60, 10, 2, float_action=True)
    rb.push(dev_rec(rec), torch.from_numpy(first).to(DEV))
    batch = rb.sample(96)
    mu, q1, q2 = seq(10, (16, 8), 2, tanh_head=True), seq(12, (64, 32, 16, 8), 1), seq(12, (64, 64), 1, 'sigmoid')
    for twin in (None, q2):
        t = ActorCriticTarget.from_modules(mu, q1, twin)
        h2 = net_of(q2, 'sigmoid') if twin is not None else None
        want = TD.target_ac(L, net_of(mu, 'relu'), net_of(q1, 'relu'), h2, *host(batch))
        same(t.target(batch), want[0], 'target')
        for g, w, name in zip(t.target(batch, return_q=True), want, ('target', 'q', 'action')):
            same(g, w, f'return_q {name}')
        with torch.no_grad():
            mu[0].weight.mul_(1.5)
            q1[0].bias.add_(0.25)
        same(t.target(batch), want[0], 'without sync() nothing changes')
        t.sync()
        changed = TD.target_ac(L, net_of(mu, 'relu'), net_of(q1, 'relu'), h2, *host(batch))
        assert not np.array_equal(TD.bits(changed[0]), TD.bits(want[0]))
        same(t.target(batch), changed[0], 'after sync()')


def test_wide_rows_of_the_match_through_the_class(L):
    """the 11v11 rows of 224 and 192 words, flattened as the replay buffer takes them"""
    from soccer2d_amd.td import QTarget
    torch.manual_seed(3)
    rs = np.random.RandomState(3)
    for D in (224, 192):
        qt = seq(D, (64, 64), 16)
        x, r, d = batch_of(rs, 70, D)
        batch = {'next_obs': to_dev(x), 'reward': to_dev(r), 'discount': to_dev(d)}
        same(QTarget.from_module(qt).target(batch), TD.target_q(L, net_of(qt, 'relu'), None, x, r, d)[0], f'D={D}')


# ------------------------------------------------------------------------------------------------------------ captured graph
def test_sample_then_target_in_one_captured_graph(L):
    """sample(out=) -> target(out=) captured once and replayed three times; between replays the parameter buffers change in
    place and a push happens; each replay equals the eager result for the same cursor and parameters.  A linear chain."""
    from soccer2d_amd.replay import DeviceReplay
    from soccer2d_amd.td import QTarget
    torch.manual_seed(4)
    rng = np.random.default_rng(4)
    B, D = 96, 10
    recs = [RR.synthetic_record(rng, 3, 50, D, 1) for _ in range(4)]

    def pushed(rb, n):
        rb.push(dev_rec(recs[n][0]), torch.from_numpy(recs[n][1]).to(DEV))
    qt, qo = seq(D, (64, 64), 16), seq(D, (12, 20), 16, 'sigmoid')
    rb, eager = DeviceReplay(512, D, device=DEV, seed=9), DeviceReplay(512, D, device=DEV, seed=9)
    t, t_eager = QTarget.from_module(qt, online=qo), QTarget.from_module(qt, online=qo)
    pushed(rb, 0), pushed(eager, 0)
    batch, out = rb.alloc_batch(B), torch.full((B,), S_F, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                            # a warm-up outside the capture, on objects of its own
        warm = DeviceReplay(512, D, device=DEV, seed=9)
        pushed(warm, 0)
        QTarget.from_module(qt, online=qo).target(warm.sample(B))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rb.sample(B, out=batch)
        t.target(batch, out=out)
    torch.cuda.synchronize()
    assert bool((out == S_F).all()) and rb.cursor.cpu().tolist()[3] == 0     # capturing ran nothing
    seen = []
    for n in range(3):
        if n:
            pushed(rb, n), pushed(eager, n)                                  # a push in between
            with torch.no_grad():                                            # and the parameter buffers change in place
                t.q_target.params.mul_(1.0 + 0.1 * n)
                t.online.params.add_(0.01 * n)
            t_eager.q_target.params.copy_(t.q_target.params)
            t_eager.online.params.copy_(t.online.params)
        graph.replay()
        torch.cuda.synchronize()
        want_batch = eager.sample(B)
        want = t_eager.target(want_batch)
        torch.cuda.synchronize()
        assert rb.cursor.cpu().tolist() == eager.cursor.cpu().tolist()
        for k in ('next_obs', 'reward', 'discount', 'index'):
            assert torch.equal(batch[k], want_batch[k]), (n, k)
        same(out, want, f'replay {n}')
        tgt = TD.Net(D, (64, 64), 16, 'relu', t.q_target.params.cpu().numpy())
        onl = TD.Net(D, (12, 20), 16, 'sigmoid', t.online.params.cpu().numpy())
        same(out, TD.target_q(L, tgt, onl, *host(batch))[0], f'replay {n} against the restatement')
        seen.append(out.cpu().numpy().copy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


# ---------------------------------------------------------------------------------------------------------------- rejections
def test_rejections_return_einval_with_text_and_launch_nothing(L, lib, monkeypatch):
    from soccer2d_amd import _capi
    rs = np.random.RandomState(8)
    B = 70
    tgt, onl = DevNet(lib, TD.random_net(rs, 10, (64, 64), 16, 'relu')), DevNet(lib, TD.random_net(rs, 10, (12, 20), 16, 'tanh'))
    actor = DevNet(lib, TD.random_net(rs, 10, (16, 8), 2, 'relu'))
    c1, c2 = DevNet(lib, TD.random_net(rs, 12, (64, 64), 1, 'relu')), DevNet(lib, TD.random_net(rs, 12, (8,), 1, 'relu'))
    x, r, d = (to_dev(a) for a in batch_of(rs, B, 10))
    t, q, i, a = _out(B), _out(B), _out(B, dtype=torch.int32), _out(B, (2,))
    torch.cuda.synchronize()

    def copy_of(s, **changes):
        c = _capi.S2DTdNet()
        C.memmove(C.byref(c), C.byref(s), C.sizeof(c))
        for k, v in changes.items():
            if k == 'hidden':
                for l in range(5):
                    c.hidden[l] = v[l] if l < len(v) else 0
            else:
                setattr(c, k, v)
        return C.byref(c)

    def refused(entry, rc, what):
        assert rc == _capi.S2D_EINVAL, (what, rc)
        text = lib.s2d_last_error().decode()
        assert entry in text, (what, text)

    def q_call(target=tgt.ref(), online=onl.ref(), batch=B, x_=x.data_ptr(), r_=r.data_ptr(), d_=d.data_ptr(), t_=t.data_ptr(), q_=q.data_ptr(),
               i_=i.data_ptr()):
        return lib.s2d_td_target_q(batch, target, online, x_, r_, d_, t_, q_, i_, None)

    def ac_call(actor_=actor.ref(), c1_=c1.ref(), c2_=c2.ref(), batch=B, x_=x.data_ptr(), r_=r.data_ptr(), d_=d.data_ptr(), t_=t.data_ptr(),
                q_=q.data_ptr(), a_=a.data_ptr()):
        return lib.s2d_td_target_ac(batch, actor_, c1_, c2_, x_, r_, d_, t_, q_, a_, None)

    s = tgt.s

    def bad_nets(n):
        return {
        'workspace NULL': dict(workspace=None), 'workspace misaligned': dict(workspace=n.workspace + 128),
        'workspace too small': dict(workspace_bytes=n.workspace_bytes - 4), 'workspace_bytes 0': dict(workspace_bytes=0),
        'n_in 0': dict(n_in=0), 'n_in 257': dict(n_in=257), 'n_hidden 0': dict(n_hidden=0), 'n_hidden 6': dict(n_hidden=6),
        'width 6': dict(hidden=(6, 64)), 'width 404': dict(hidden=(64, 404)), 'width 4': dict(hidden=(4, 64)),
        'a width past n_hidden': dict(hidden=(64, 64, 8)), 'n_out 0': dict(n_out=0), 'n_out 65': dict(n_out=65),
        'activation 3': dict(activation=3), 'activation -1': dict(activation=-1), 'params NULL': dict(params=None),
        'params misaligned': dict(params=n.params + 4)}
    for what in bad_nets(s):
        refused('s2d_td_target_q', q_call(target=copy_of(s, **bad_nets(s)[what])), f'target: {what}')
        refused('s2d_td_target_q', q_call(online=copy_of(onl.s, **bad_nets(onl.s)[what])), f'online: {what}')
        refused('s2d_td_target_ac', ac_call(actor_=copy_of(actor.s, **bad_nets(actor.s)[what])), f'actor: {what}')
        refused('s2d_td_target_ac', ac_call(c1_=copy_of(c1.s, **bad_nets(c1.s)[what])), f'critic1: {what}')
        refused('s2d_td_target_ac', ac_call(c2_=copy_of(c2.s, **bad_nets(c2.s)[what])), f'critic2: {what}')
    refused('s2d_td_target_q', q_call(target=None), 'target NULL')
    refused('s2d_td_target_q', q_call(online=copy_of(onl.s, n_in=11)), 'online n_in')
    refused('s2d_td_target_q', q_call(online=copy_of(onl.s, n_out=15)), 'online n_out')
    refused('s2d_td_target_q', q_call(online=copy_of(onl.s, workspace=s.workspace, workspace_bytes=s.workspace_bytes)), 'a shared workspace')
    refused('s2d_td_target_q', q_call(online=copy_of(onl.s, workspace=s.workspace + 256, workspace_bytes=s.workspace_bytes - 256)),
            'overlapping workspaces')
    for b in (0, -1, 2 ** 31, 2 ** 40):
        refused('s2d_td_target_q', q_call(batch=b), f'batch {b}')
        refused('s2d_td_target_ac', ac_call(batch=b), f'batch {b}')
    for name in ('x_', 'r_', 'd_', 't_'):
        refused('s2d_td_target_q', q_call(**{name: None}), f'{name} NULL')
        refused('s2d_td_target_ac', ac_call(**{name: None}), f'{name} NULL')
    for name, ptr in (('x_', x), ('r_', r), ('d_', d), ('t_', t), ('q_', q), ('i_', i)):
        refused('s2d_td_target_q', q_call(**{name: ptr.data_ptr() + 2}), f'{name} misaligned')
    for name, ptr in (('x_', x), ('r_', r), ('d_', d), ('t_', t), ('q_', q), ('a_', a)):
        refused('s2d_td_target_ac', ac_call(**{name: ptr.data_ptr() + 2}), f'{name} misaligned')
    refused('s2d_td_target_ac', ac_call(actor_=None), 'actor NULL')
    refused('s2d_td_target_ac', ac_call(c1_=None), 'critic1 NULL')
    refused('s2d_td_target_ac', ac_call(actor_=copy_of(actor.s, n_out=9), c1_=copy_of(c1.s, n_in=19), c2_=None), 'nine actions')
    refused('s2d_td_target_ac', ac_call(c1_=copy_of(c1.s, n_in=11)), 'critic1 n_in')
    refused('s2d_td_target_ac', ac_call(c1_=copy_of(c1.s, n_in=10)), 'critic1 without the action')
    refused('s2d_td_target_ac', ac_call(c1_=copy_of(c1.s, n_out=2)), 'critic1 n_out')
    refused('s2d_td_target_ac', ac_call(c2_=copy_of(c2.s, n_in=13)), 'critic2 n_in')
    refused('s2d_td_target_ac', ac_call(c1_=copy_of(c1.s, workspace=actor.s.workspace, workspace_bytes=c1.s.workspace_bytes)),
            'actor and critic1 share')
    refused('s2d_td_target_ac', ac_call(c2_=copy_of(c2.s, workspace=c1.s.workspace, workspace_bytes=c1.s.workspace_bytes)),
            'critic1 and critic2 share')
    refused('s2d_td_target_ac', ac_call(c2_=copy_of(c2.s, workspace=actor.s.workspace, workspace_bytes=c2.s.workspace_bytes)),
            'actor and critic2 share')
    for plan in ('3,1', '1', 'waves'):
        monkeypatch.setenv('S2D_TD_PLAN', plan)
        refused('s2d_td_target_q', q_call(), f'plan {plan}')
        refused('s2d_td_target_ac', ac_call(), f'plan {plan}')
        assert 'S2D_TD_PLAN' in lib.s2d_last_error().decode()
    monkeypatch.delenv('S2D_TD_PLAN')
    torch.cuda.synchronize()
    # nothing ran: every output and every workspace still holds its sentinel
    assert bool((t == S_F).all()) and bool((q == S_F).all()) and bool((i == S_I).all()) and bool((a == S_F).all())
    for n in (tgt, onl, actor, c1, c2):
        assert bool((n.ws == -3333.0).all())
    # and the same arguments, unchanged, are accepted
    assert q_call() == 0 and ac_call() == 0
    torch.cuda.synchronize()
    assert not bool((t[:B] == S_F).any()) and bool((t[B:] == S_F).all())
