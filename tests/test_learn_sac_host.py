"""CPU checks of the fused Soft Actor-Critic update's host side (s2d_learn_sac_actor, soccer2d_amd.learn.SACLearner): the ABI
additions, the workspace arithmetic, and the host restatement tests/learn_sac_ref.c -- its forward against sac_ref.c's head and
td_ref.c's networks bitwise, its gradients against float64 torch autograd of the example's loss_pi and loss_alpha, a hand-computed
case for the head's derivative and the min-Q selection, the data edges, a training sanity run -- and the argument checks of the
class that raise before any library call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import learn as LR
import learn_sac as LS
import sac_ref as SR
import td as TD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip('torch')
nn = torch.nn
F = np.float32


@pytest.fixture(scope='module')
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp('learn_sac_ref')
    return LS.build(d), SR.build(d), TD.build(d)


def clone(net):
    return TD.Net(net.n_in, net.hidden, net.n_out, net.act, net.params.copy()) if net is not None else None


def same_bits(a, b):
    """bit for bit; where both are NaN only that they are NaN"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(TD.bits(a)[~na], TD.bits(b)[~nb])


# ------------------------------------------------------------------------------------------------------------------------ ABI
def test_abi_additions(tmp_path):
    """the ABI version stays 4, the learner's structs are unchanged, S2D_LEARN_SAC_STREAM is 14 and no other stream's id, the new
    struct has the ctypes size and the header declares the three functions"""
    from soccer2d_amd import _capi
    prog = tmp_path / 'learn_sac_abi.c'
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s2d.h"\nint main(){printf("%d %d %d %d %d %zu %zu %zu %zu %zu", S2D_ABI_VERSION, '
                    'S2D_LEARN_SAC_STREAM, S2D_TD_STREAM, S2D_REPLAY_STREAM, S2D_REPLAY_PRIO_STREAM, sizeof(S2DLearnNet), sizeof(S2DLearnState), '
                    'sizeof(S2DLearnSacAlpha), offsetof(S2DLearnSacAlpha, target_entropy), sizeof &s2d_learn_sac_actor + '
                    'sizeof &s2d_learn_sac_actor_grad + sizeof &s2d_learn_sac_workspace_bytes);return 0;}\n')
    exe = tmp_path / 'learn_sac_abi'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(prog), '-o', str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [4, 14, 13, 11, 12, C.sizeof(_capi.S2DLearnNet), C.sizeof(_capi.S2DLearnState), C.sizeof(_capi.S2DLearnSacAlpha),
                   _capi.S2DLearnSacAlpha.target_entropy.offset, 3 * C.sizeof(C.c_void_p)]
    assert LS.STREAM == 14 and _capi.S2D_ABI_VERSION == 4


def _shape(n_in, hidden, n_out, act=0):
    from soccer2d_amd import _capi
    s = _capi.S2DLearnNet()
    s.n_in, s.n_hidden, s.n_out, s.activation = n_in, len(hidden), n_out, act
    for l, w in enumerate(hidden):
        s.hidden[l] = w
    return s


def test_symbols_exported_and_workspace_arithmetic():
    """the built library exports and binds the three symbols; s2d_learn_sac_workspace_bytes (host only) agrees with the Python
    arithmetic on the grid and is 0 off it; the 64-64 triple needs no image words, the 256-256 triple does"""
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi
    from soccer2d_amd.learn import learn_param_count, learn_sac_workspace_bytes, learn_workspace_bytes
    lib = _capi.load_library()
    protos = {p[0]: p for p in _capi.PROTOTYPES}
    for name, nargs in (('s2d_learn_sac_actor', 14), ('s2d_learn_sac_actor_grad', 14), ('s2d_learn_sac_workspace_bytes', 4)):
        assert hasattr(lib, name) and len(protos[name][2]) == nargs, name
    assert protos['s2d_learn_sac_workspace_bytes'][1] is C.c_size_t

    def ws(D, A, ha, h1, h2, B):
        return lib.s2d_learn_sac_workspace_bytes(C.byref(_shape(D, ha, 2 * A)), C.byref(_shape(D + A, h1, 1)),
                                                 C.byref(_shape(D + A, h2, 1)) if h2 is not None else None, B)
    for D, A, ha, h1, h2, _ in LS.SHAPES + [(248, 8, (256,) * 4, (256,) * 4, (256,) * 4, None), (10, 1, (256, 256), (64,), None, None)]:
        for B in (1, 63, 64, 65, 4096, 2 ** 31 - 1):
            got = ws(D, A, ha, h1, h2, B)
            assert got == learn_sac_workspace_bytes(D, ha, A, h1, h2, B) and got >= 4 * learn_param_count(D, ha, 2 * A), (D, A, ha, h1, h2, B)
            assert got >= learn_workspace_bytes(D, ha, 2 * A, B)             # never less than the actor alone would need
    r64 = lambda w: (w + 63) // 64 * 64
    P = learn_param_count(10, (64, 64), 2)
    assert ws(10, 1, (64, 64), (64, 64), (64, 64), 64) == 4 * (r64(P) + r64((P + 255) // 256) + 64 + 64)   # partials, chunks, loss, logp: no image
    P = learn_param_count(10, (256, 256), 2)
    pitch = (12 + 512 + 2 + 2 * 513 + 1) | 1
    assert ws(10, 1, (256, 256), (256, 256), (256, 256), 64) == 4 * (r64(P) + r64((P + 255) // 256) + 64 + 64 + r64(64 * pitch))
    # a second critic can push the image out of the LDS
    assert ws(10, 1, (128, 64), (128, 128), None, 64) < ws(10, 1, (128, 64), (128, 128), (256, 256), 64)
    for a, c1, c2 in ((_shape(10, (64,), 3), _shape(11, (64,), 1), None), (_shape(10, (64,), 18), _shape(19, (64,), 1), None),
                      (_shape(10, (64,), 0), _shape(10, (64,), 1), None), (_shape(249, (64,), 2), _shape(250, (64,), 1), None),
                      (_shape(10, (64,), 2), _shape(12, (64,), 1), None), (_shape(10, (64,), 2), _shape(11, (64,), 2), None),
                      (_shape(10, (64,), 2), _shape(11, (64,), 1), _shape(12, (64,), 1)), (_shape(10, (64,), 2), _shape(11, (64,), 1), _shape(11, (12,), 1)),
                      (_shape(10, (12,), 2), _shape(11, (64,), 1), None), (_shape(10, (64,), 2), _shape(11, (64,) * 5, 1), None),
                      (_shape(10, (64,), 2, act=3), _shape(11, (64,), 1), None)):
        assert lib.s2d_learn_sac_workspace_bytes(C.byref(a), C.byref(c1), C.byref(c2) if c2 is not None else None, 64) == 0
    good = (_shape(10, (64,), 2), _shape(11, (64,), 1))
    assert lib.s2d_learn_sac_workspace_bytes(None, C.byref(good[1]), None, 64) == 0 == lib.s2d_learn_sac_workspace_bytes(C.byref(good[0]), None, None, 64)
    for B in (0, -1, 2 ** 31):
        assert lib.s2d_learn_sac_workspace_bytes(C.byref(good[0]), C.byref(good[1]), None, B) == 0
    assert lib.s2d_learn_sac_workspace_bytes(C.byref(good[0]), C.byref(good[1]), None, 1) > 0


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('shape', LS.SHAPES, ids=LS.shape_id)
def test_forward_equals_sac_ref_and_td_ref(refs, shape):
    """action and logp are sac_ref.c's head on td_ref.c's forward of the actor with the step's z; q is the smaller of td_ref.c's
    forwards of [obs | a]; z changes with draws and differs from the target's z at the same (seed, draws): another stream"""
    L, S, T = refs
    D, A = shape[:2]
    rs = np.random.RandomState(3)
    actor, c1, c2 = LS.random_nets(rs, shape)
    B = 70
    obs = rs.uniform(-1, 1, (B, D)).astype(F)
    obs[0], obs[1], obs[2], obs[3, 0] = 0.0, -0.0, 1e30, np.nan
    z = LS.z(L, B, A, 99, 2 ** 33 + 1)
    got = LS.actor_grad(L, actor, c1, c2, obs, 0.5, seed=99, draws=2 ** 33 + 1)
    a, lp = SR.head(S, TD.forward(T, actor, obs), z)
    assert same_bits(got['action'], a) and same_bits(got['logp'], lp)
    x = np.concatenate([obs, a], 1)
    q1 = TD.forward(T, c1, x)[:, 0]
    q = q1 if c2 is None else np.where(TD.forward(T, c2, x)[:, 0] < q1, TD.forward(T, c2, x)[:, 0], q1)
    assert same_bits(got['q'], q)
    assert same_bits(LS.actor_grad(L, actor, c1, c2, obs, 0.5, z=z)['grad'], got['grad'])      # z given == z drawn
    assert not np.array_equal(z, LS.z(L, B, A, 99, 2 ** 33 + 2)) and not np.array_equal(z, LS.z(L, B, A, 99, 1))   # both halves of draws count
    assert not np.array_equal(z, LS.z(L, B, A, 98, 2 ** 33 + 1)) and not np.array_equal(z, SR.td_z(S, B, A, 99, 2 ** 33 + 1))
    assert abs(float(z.mean())) < 0.5 and 0.5 < float(z.std()) < 1.5


def comparison_inputs(L, shape, B=150, alpha=0.7):
    """nets, obs and z on which the comparison with float64 autograd is meaningful: critic 2's output bias moved by the median of
    q1 - q2 so that both critics are chosen, rows whose q1 and q2 are within 1e-3 drawn again, the draw counter advanced (and, failing that, the log-std biases lowered) until every
    |u_j| < 4 -- all decided on the float64 values alone"""
    D, A = shape[:2]
    rs = np.random.RandomState(11)
    actor, c1, c2 = LS.random_nets(rs, shape)
    obs = rs.uniform(-1, 1, (B, D)).astype(F)
    for draws in range(64):
        z = LS.z(L, B, A, 7, draws % 8)
        t = LS.torch_losses(actor, c1, c2, obs, z, alpha, 1.0, -A, torch.float64)
        if np.abs(t['u']).max() < 3.9:
            break
        if draws % 8 == 7:
            actor.params[-A:] -= F(0.5)                                      # a smaller sigma: the log-std rows' biases go down
    for _ in range(20):
        if c2 is None:
            break
        c2.params[-1] += F(np.median(t['q1'] - t['q2']))
        t = LS.torch_losses(actor, c1, c2, obs, z, alpha, 1.0, -A, torch.float64)
        close = np.abs(t['q1'] - t['q2']) < 2e-3
        if not close.any() and np.abs(t['u']).max() < 4 and 0.3 < (t['q2'] < t['q1']).mean() < 0.7:
            break
        obs[close] = rs.uniform(-1, 1, (int(close.sum()), D)).astype(F)
    return (actor, c1, c2), obs, z


@pytest.mark.parametrize('shape', LS.SHAPES, ids=LS.shape_id)
def test_gradient_against_float64_autograd(refs, shape):
    """the restated actor gradient, loss_pi, mean logp and the temperature's gradient against float64 torch autograd of the example's
    losses on the same z: at most 4 x the error of torch's own fp32 autograd on the same inputs, the bound computed here, with the
    sequential-sum allowance for the means.  B = 150: three blocks, the last partial."""
    L = refs[0]
    D, A = shape[:2]
    alpha, B = F(0.7), 150
    (actor, c1, c2), obs, z = comparison_inputs(L, shape, B, alpha)
    t64 = LS.torch_losses(actor, c1, c2, obs, z, alpha, 1.0, -A, torch.float64)
    t32 = LS.torch_losses(actor, c1, c2, obs, z, alpha, 1.0, -A, torch.float32)
    # the comparison is meaningful: the selection cannot differ, both critics are used, the clamp and tanh are away from their edges
    if c2 is not None:
        sel = t64['q2'] < t64['q1']
        assert np.abs(t64['q1'] - t64['q2']).min() >= 1e-3 and 0.25 <= sel.mean() <= 0.75, (np.abs(t64['q1'] - t64['q2']).min(), sel.mean())
    assert t64['v'].min() >= -20 + 1e-3 and t64['v'].max() <= 2 - 1e-3 and np.abs(t64['u']).max() < 4
    before = [c.params.copy() for c in (c1, c2) if c is not None]
    got = LS.actor_grad(L, actor, c1, c2, obs, alpha, z=z)
    if c2 is not None:
        x = np.concatenate([obs, got['action']], 1)
        assert np.array_equal(LS.forward(L, c2, x)[:, 0] < LS.forward(L, c1, x)[:, 0], sel)
    err_torch, err_ref = np.abs(t32['grad'] - t64['grad']).max(), np.abs(got['grad'].astype(np.float64) - t64['grad']).max()
    print(f'grad error vs float64: torch fp32 {err_torch:.3e}, learn_sac_ref {err_ref:.3e}; |g|max {np.abs(t64["grad"]).max():.3e}')
    assert err_torch > 0 and err_ref <= 4 * err_torch
    u = 2.0 ** -24
    rows = np.abs(alpha * got['logp'].astype(np.float64) - got['q'])
    for name, ref, key, terms in (('loss_pi', got['stats'][0], 'loss_pi', rows), ('mean logp', got['mean_logp'], 'mean_logp', np.abs(got['logp']))):
        e_torch, e_ref = abs(t32[key] - t64[key]), abs(float(ref) - t64[key])
        print(f'{name} error vs float64: torch fp32 {e_torch:.3e}, learn_sac_ref {e_ref:.3e}')
        # a sequential fp32 sum of B terms: to torch's error (its sum is pairwise) the worst case of that order is added,
        # (B - 1) u sum|t| / B with u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2)
        assert e_ref <= 4 * max(e_torch, np.spacing(F(abs(t64[key]))) / 2) + (B - 1) * u * terms.mean()
    ast = LS.AlphaState(-A, log_alpha=1.0)
    g_ref = float(LS.alpha_stats(L, got['mean_logp'], ast)[1])               # log_alpha = 1: the loss is the gradient
    e_torch, e_ref = abs(t32['dalpha'] - t64['dalpha']), abs(g_ref - t64['dalpha'])
    assert e_ref <= 4 * max(e_torch, np.spacing(F(abs(t64['dalpha']))) / 2) + (B - 1) * u * np.abs(got['logp']).mean()
    assert abs(float(LS.alpha_stats(L, got['mean_logp'], LS.AlphaState(-A, log_alpha=0.37))[1]) - F(0.37) * g_ref) <= 1e-6 * abs(g_ref)
    norm64 = np.sqrt((t64['grad'] ** 2).sum())
    assert abs(float(got['stats'][1]) - norm64) <= 4 * max(err_torch, np.spacing(F(norm64))) and float(got['stats'][2]) == 1.0
    assert all(np.array_equal(c.params, b) for c, b in zip((c1, c2), before))


def _hand_nets():
    """actor 1-8-2 ReLU: mean = 0.5 relu(x), v = 0 (sigma = 1); critic 1 2-8-1 ReLU: q1 = 3 relu(2 a) + 0.25; critic 2: q2 = 2 relu(a) + 1
    (both read the action column alone)"""
    e0 = np.eye(8, dtype=F)[0]
    actor = TD.Net(1, (8,), 2, 'relu', np.concatenate([e0, np.zeros(8), 0.5 * e0, np.zeros(8), [0.0, 0.0]]).astype(F))
    W1, W2 = np.zeros((8, 2), F), np.zeros((8, 2), F)
    W1[0, 1], W2[0, 1] = 2.0, 1.0
    c1 = TD.Net(2, (8,), 1, 'relu', np.concatenate([W1.ravel(), np.zeros(8), 3 * e0, [0.25]]).astype(F))
    c2 = TD.Net(2, (8,), 1, 'relu', np.concatenate([W2.ravel(), np.zeros(8), 2 * e0, [1.0]]).astype(F))
    return actor, c1, c2


def test_hand_computed_head_derivative_and_selection(refs):
    """B = 2, A = 1, obs 1 and -1, z 0.5 and -1, alpha 0.5 (w = 1/4).  Row 0: u = 1, a = tanh(1), q1 = 6 a + 0.25 > q2 = 2 a + 1: critic 2;
    its output delta -1/2, its unit's delta -1, s = -1.  Row 1: u = -1, a < 0, q1 = 0.25 < q2 = 1: critic 1, whose unit sits at exactly 0,
    so s = 0.  Every operation below is the spec's, in fp32, given a."""
    L = refs[0]
    actor, c1, c2 = _hand_nets()
    obs, z = np.array([[1.0], [-1.0]], F), np.array([[0.5], [-1.0]], F)
    got = LS.actor_grad(L, actor, c1, c2, obs, 0.5, z=z)
    a0, a1 = got['action'][:, 0]
    assert abs(float(a0) - np.tanh(1.0)) < 1e-6 and a1 == -a0
    assert np.array_equal(got['q'], np.array([F(2) * a0 + F(1), 0.25], F))   # row 0 took critic 2, row 1 critic 1
    w, one = F(0.25), F(1.0)

    def head(a, s, sz):
        om = F(np.float64(-a) * np.float64(a) + 1.0)                         # fmaf: one rounding
        r = om / (om + F(1e-6))
        du = ((w * (F(2) * a)) * r) + (s * om)
        return du, (du * sz) - w
    du0, dls0 = head(a0, F(-1.0), one * F(0.5))
    du1, dls1 = head(a1, F(0.0), one * F(-1.0))
    assert np.array_equal(got['du'][:, 0], np.array([du0, du1], F)) and np.array_equal(got['dls'][:, 0], np.array([dls0, dls1], F))
    e0 = np.eye(8, dtype=F)[0]
    dh = F(0.5) * du0                                                        # the hidden unit's delta in row 0; row 1's unit is dead
    want = np.concatenate([dh * e0, dh * e0, du0 * e0, dls0 * e0, [du0 + du1, dls0 + dls1]]).astype(F)
    assert np.array_equal(got['grad'], want), (got['grad'], want)
    lp = got['logp']
    l0, l1 = F(0.5) * lp[0] - got['q'][0], F(0.5) * lp[1] - got['q'][1]
    assert got['stats'][0] == (l0 + l1) / F(2) and got['mean_logp'] == (lp[0] + lp[1]) / F(2)
    t64 = LS.torch_losses(actor, c1, c2, obs, z, 0.5, 0.0, -1, torch.float64)
    assert np.abs(t64['grad'] - want).max() < 1e-6 and abs(t64['loss_pi'] - float(got['stats'][0])) < 1e-6
    assert abs(t64['mean_logp'] - float(got['mean_logp'])) < 1e-6


def _head_actor(actor, A, mean_bias=None, v_bias=None):
    p = actor.params.copy()
    h = actor.hidden[-1]
    W, b = p[-(2 * A * h + 2 * A):-2 * A].reshape(2 * A, h), p[-2 * A:]
    if mean_bias is not None:
        W[:A], b[:A] = 0.0, np.asarray(mean_bias, F)
    if v_bias is not None:
        W[A:], b[A:] = 0.0, np.asarray(v_bias, F)
    return TD.Net(actor.n_in, actor.hidden, actor.n_out, actor.act, p)


def test_edges_on_the_restatement(refs):
    L = refs[0]
    rs = np.random.RandomState(31)
    shape = (10, 4, (16, 8), (16, 8), (8, 8), ('relu',) * 3)
    actor, c1, c2 = LS.random_nets(rs, shape)
    A, B = 4, 70
    obs = rs.uniform(-1, 1, (B, 10)).astype(F)
    z = LS.z(L, B, A, 5, 0)
    w = F(0.6) / F(B)
    lo, hi = F(-20.0), F(2.0)
    # v exactly at the bounds: the gradient passes; one ulp outside, and NaN: dv = +0 (the bias gradient of that output is its sum)
    got = LS.actor_grad(L, _head_actor(actor, A, v_bias=[lo, hi, np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))]), c1, c2, obs, 0.6, z=z)
    db = got['grad'][-A:]
    assert db[0] != 0 and db[1] != 0 and (TD.bits(db[2:]) == 0).all()
    assert abs(db[0] - got['dls'][:, 0].astype(np.float64).sum()) < 1e-5 and (got['dls'][:, 2:] != 0).all()
    got = LS.actor_grad(L, _head_actor(actor, A, v_bias=[np.nan, 0.0, 0.0, 0.0]), c1, c2, obs, 0.6, z=z)
    assert TD.bits(got['grad'][-A]) == 0 and np.isfinite(got['grad']).all() and np.isfinite(got['logp']).all()
    # saturated actions: du = 0, dls = -w
    got = LS.actor_grad(L, _head_actor(actor, A, mean_bias=[40.0, -40.0, 0.0, 0.0], v_bias=[-20.0] * 4), c1, c2, obs, 0.6, z=z)
    assert (got['action'][:, 0] == 1).all() and (got['action'][:, 1] == -1).all()
    assert (got['du'][:, :2] == 0).all() and (got['dls'][:, :2] == -w).all() and (got['du'][:, 2:] != 0).any()
    # q1 == q2 and a NaN q2: critic 1's path, bit for bit
    alone = LS.actor_grad(L, actor, c1, None, obs, 0.6, z=z)
    nanq = clone(c2)
    nanq.params[-1] = np.nan
    for second in (clone(c1), nanq):
        got = LS.actor_grad(L, actor, c1, second, obs, 0.6, z=z)
        assert all(np.array_equal(TD.bits(got[k]), TD.bits(alone[k])) for k in ('grad', 'stats', 'q', 'logp', 'action', 'du'))
    both = LS.actor_grad(L, actor, c1, c2, obs, 0.6, z=z)
    assert not np.array_equal(both['q'], alone['q']) and not np.array_equal(both['grad'], alone['grad'])
    # alpha = 0: the entropy term is gone, the loss is -mean q, dls = du sigma z
    got = LS.actor_grad(L, actor, c1, c2, obs, 0.0, z=z)
    assert abs(float(got['stats'][0]) + got['q'].astype(np.float64).mean()) < 1e-6 and np.isfinite(got['grad']).all()
    # a fixed temperature: the step writes nothing of it and leaves alpha; a learned one moves log_alpha and alpha = exp(log_alpha)
    alpha, draws = np.array([0.6], F), np.array([3], np.uint64)
    a1 = clone(actor)
    LS.actor_step(L, a1, c1, c2, LR.State(a1.params.size, lr=1e-2, max_grad_norm=0.0), obs, alpha, None, draws, 5)
    assert alpha[0] == F(0.6) and draws[0] == 4 and not np.array_equal(a1.params, actor.params)
    ast, a2 = LS.AlphaState(-A, log_alpha=float(np.log(0.6)), lr=1e-2), clone(actor)
    alpha, draws = np.array([0.6], F), np.array([3], np.uint64)
    LS.actor_step(L, a2, c1, c2, LR.State(a2.params.size, lr=1e-2, max_grad_norm=0.0), obs, alpha, ast, draws, 5)
    assert np.array_equal(a1.params, a2.params)                              # the rows read alpha before the temperature moves
    assert abs(float(alpha[0]) - np.exp(float(ast.log_alpha[0]))) < 1e-6 and alpha[0] != F(0.6) and ast.stats[2] == alpha[0]
    assert np.array_equal(ast.hyper[5:7], np.array([0.9, 0.999], F)) and ast.m_v[0] != 0


def test_training_sanity(refs):
    """with fixed critics (trained on a teacher), 200 restated actor steps raise mean(min Q - alpha logp) on a fixed batch; with a fixed
    policy, the temperature's steps move alpha to the side the sign of mean logp + target_entropy dictates; torch's fp32 chain on the
    same inputs meets both conditions first"""
    L = refs[0]
    rs = np.random.RandomState(1)
    D, A, B, lr, alpha = 10, 2, 256, 1e-2, F(0.2)
    shape = (D, A, (16, 16), (16, 16), (16, 16), ('tanh',) * 3)
    actor, c1, c2 = LS.random_nets(rs, shape, gain=2.0)
    obs = rs.uniform(-1, 1, (B, D)).astype(F)
    zs = [LS.z(L, B, A, 3, n) for n in range(200)]
    mods = [LR.torch_module(n, torch.float32) for n in (actor, c1, c2)]
    opt = torch.optim.Adam(mods[0].parameters(), lr=lr)
    o = torch.from_numpy(obs)

    def torch_objective(z):
        import math
        mean, v = mods[0](o).chunk(2, dim=1)
        ls = v.clamp(-20.0, 2.0)
        a = torch.tanh(mean + ls.exp() * torch.from_numpy(z))
        logp = (-0.5 * torch.from_numpy(z) ** 2 - ls - 0.5 * math.log(2 * math.pi) - torch.log(1 - a * a + 1e-6)).sum(dim=1)
        x = torch.cat([o, a], 1)
        return (float(alpha) * logp - torch.min(mods[1](x), mods[2](x)).squeeze(1)).mean(), logp
    tq = []
    for z in zs:
        loss, _ = torch_objective(z)
        opt.zero_grad()
        loss.backward()
        opt.step()
        tq.append(-float(loss.detach()))
    assert np.mean(tq[-10:]) > np.mean(tq[:10]) + 0.1, (tq[0], tq[-1])
    st, rq = LR.State(actor.params.size, lr=lr, max_grad_norm=0.0), []
    a_h, draws = np.array([alpha], F), np.zeros(1, np.uint64)
    policy0 = clone(actor)
    for n in range(200):
        rq.append(-float(LS.actor_step(L, actor, c1, c2, st, obs, a_h, None, draws, 3)['stats'][0]))
    print(f'mean(min q - alpha logp): torch {np.mean(tq[:10]):.4f} -> {np.mean(tq[-10:]):.4f}, learn_sac_ref {np.mean(rq[:10]):.4f} -> {np.mean(rq[-10:]):.4f}')
    assert abs(rq[0] - tq[0]) < 1e-5 and np.mean(rq[-10:]) > np.mean(rq[:10]) + 0.1 and draws[0] == 200
    assert abs(np.mean(rq[-10:]) - np.mean(tq[-10:])) < 0.25 * (np.mean(tq[-10:]) - np.mean(tq[:10]))
    # the temperature with a fixed policy: mean logp + target_entropy > 0 (too little entropy) raises alpha, < 0 lowers it
    for te, up in ((4.0, True), (-8.0, False)):
        la = torch.zeros(1, requires_grad=True)
        opt_a = torch.optim.Adam([la], lr=lr)
        ast, a_h = LS.AlphaState(te, lr=lr), np.ones(1, F)
        signs = []
        for n in range(50):
            got = LS.actor_grad(L, policy0, c1, c2, obs, a_h[0], seed=3, draws=n)
            signs.append(got['mean_logp'] + F(te) > 0)
            loss = -(la * float(got['mean_logp'] + F(te)))
            opt_a.zero_grad()
            loss.backward()
            opt_a.step()
            L.learn_sac_alpha(float(got['mean_logp']), float(F(te)), 1, ast.log_alpha.ctypes.data, ast.m_v.ctypes.data, ast.hyper.ctypes.data,
                              ast.stats.ctypes.data, a_h.ctypes.data)
        assert all(s == up for s in signs) and (float(la.detach().exp()) > 1.0) == up and (a_h[0] > 1.0) == up
        assert abs(float(la.detach()) - float(ast.log_alpha[0])) < 1e-4 and abs(float(ast.log_alpha[0])) > 0.2


# ---------------------------------------------------------------------------------------------------------------- SACLearner
def seq(n_in, hidden, n_out, act=nn.ReLU, bias=True):
    layers, win = [], n_in
    for w in hidden:
        layers += [nn.Linear(win, w, bias=bias), act()]
        win = w
    return nn.Sequential(*layers, nn.Linear(win, n_out, bias=bias))


def test_module_parameters_become_views_and_hyper_words():
    from soccer2d_amd.learn import SACLearner, learn_param_count
    actor, q1, q2 = seq(10, (64, 64), 2), seq(11, (64, 64), 1), seq(11, (32,), 1, act=nn.Tanh)
    before = [[p.detach().clone() for p in m.parameters()] for m in (actor, q1, q2)]
    lrn = SACLearner.from_modules(actor, q1, q2, actor_lr=1e-4, alpha_lr=2e-4, device='cpu', seed=2 ** 64 + 5)
    for net, mod, old, P in zip((lrn.actor,) + lrn.critics, (actor, q1, q2), before, (learn_param_count(10, (64, 64), 2),
                                                                                      learn_param_count(11, (64, 64), 1), learn_param_count(11, (32,), 1))):
        assert net.params.numel() == P
        off = net.params.data_ptr()
        for p, b in zip(mod.parameters(), old):
            assert p.data_ptr() == off and torch.equal(p.detach(), b)        # nn.Sequential order, values kept
            off += 4 * p.numel()
    with torch.no_grad():
        lrn.actor.params.fill_(0.5)
    assert all(bool((p == 0.5).all()) for p in actor.parameters())
    assert lrn.actor.hyper.tolist() == [float(F(x)) for x in (1e-4, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0)]
    assert lrn.critics[1].hyper.tolist() == [float(F(x)) for x in (3e-4, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0)]
    assert lrn.alpha_hyper.tolist() == [float(F(x)) for x in (2e-4, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0)]
    assert (lrn.obs_dim, lrn.action_dim, lrn.loss_kind, lrn.target_entropy, lrn.seed, lrn.auto) == (10, 1, 0, -1.0, 5, True)
    assert lrn.alpha.tolist() == [1.0] and lrn.log_alpha.tolist() == [0.0] and lrn.draws.tolist() == [0] and lrn.draws.dtype == torch.int64
    assert lrn.ent_coef == 1.0 and lrn.alpha_struct().target_entropy == -1.0 and lrn.alpha_struct().log_alpha == lrn.log_alpha.data_ptr()
    lrn.set_lr(actor=0.5)
    lrn.set_lr(critic=0.25, alpha=0.125)
    assert lrn.actor.hyper[0] == 0.5 and all(c.hyper[0] == 0.25 for c in lrn.critics) and lrn.alpha_hyper[0] == 0.125
    lrn.critics[0].m.fill_(1.0), lrn.alpha_m_v.fill_(1.0), lrn.alpha_hyper[5:7].fill_(0.5)
    lrn.reset_optimizer()
    assert not lrn.critics[0].m.any() and not lrn.alpha_m_v.any() and lrn.alpha_hyper[5:7].tolist() == [1.0, 1.0]
    fixed = SACLearner.from_modules(seq(10, (8,), 8), seq(14, (8,), 1), ent_coef=0.2, target_entropy=-2.5, device='cpu')
    assert fixed.alpha.tolist() == [float(F(0.2))] and fixed.alpha_struct() is None and fixed.log_alpha is None and fixed.action_dim == 4
    assert fixed.target_entropy == -2.5 and len(fixed.critics) == 1 and fixed.ent_coef == float(F(0.2))
    with pytest.raises(ValueError, match='fixed'):
        fixed.entropy


def test_refusals_on_the_host():
    """every refusal of the Python layer raises ValueError before a library call (there is no GPU here to call), and a refused
    construction leaves the modules' parameters where they were"""
    from soccer2d_amd.learn import SACLearner
    good_q = lambda: seq(11, (8,), 1)
    for actor, q, text in ((seq(10, (12,), 2), good_q(), 'multiple of 8'), (seq(10, (264,), 2), good_q(), 'multiple of 8'),
                           (seq(10, (400, 300), 2), good_q(), r'multiple of 8 in \[8, 256\]'), (seq(10, (8,) * 5, 2), good_q(), '1 to 4 hidden'),
                           (seq(10, (8,), 2), seq(11, (400, 300), 1), 'multiple of 8'), (seq(10, (8,), 3), good_q(), '2 A'),
                           (seq(10, (8,), 18), seq(19, (8,), 1), '2 A'), (seq(249, (8,), 2), seq(250, (8,), 1), 'input width'),
                           (seq(10, (8,), 2), seq(12, (8,), 1), 'obs_dim [+] A'), (seq(10, (8,), 2), seq(11, (8,), 2), 'one output'),
                           (seq(10, (8,), 2, bias=False), good_q(), 'bias'), (seq(10, (8,), 2), seq(11, (8,), 1, act=nn.ELU), 'activation'),
                           (seq(10, (8,), 2).double(), good_q(), 'float32'), ('actor', good_q(), 'torch.nn.Module'),
                           ((seq(10, (8,), 8), nn.Linear(8, 1), nn.Linear(8, 1)), good_q(), 'triple')):
        mods = [m for m in (actor, q) if isinstance(m, nn.Module)]
        olds = [p.data_ptr() for m in mods for p in m.parameters()]
        with pytest.raises(ValueError, match=text):
            SACLearner.from_modules(actor, q, device='cpu')
        assert olds == [p.data_ptr() for m in mods for p in m.parameters()]
    with pytest.raises(ValueError, match='critic 2'):
        SACLearner.from_modules(seq(10, (8,), 2), good_q(), seq(12, (8,), 1), device='cpu')
    for kw, text in ((dict(ent_coef='fixed'), 'ent_coef'), (dict(ent_coef=-0.1), 'ent_coef'), (dict(ent_coef=float('nan')), 'ent_coef'),
                     (dict(ent_coef=None), 'ent_coef'), (dict(target_entropy='auto'), 'target_entropy'), (dict(max_batch=0), 'max_batch'),
                     (dict(max_batch=2 ** 31), 'max_batch'), (dict(betas=(0.9, 1.0)), 'betas'), (dict(actor_lr=-1.0), 'lr'), (dict(alpha_lr=-1.0), 'alpha_lr')):
        actor, q = seq(10, (8,), 2), good_q()
        olds = [p.data_ptr() for m in (actor, q) for p in m.parameters()]
        with pytest.raises(ValueError, match=text):
            SACLearner.from_modules(actor, q, device='cpu', **kw)
        assert olds == [p.data_ptr() for m in (actor, q) for p in m.parameters()]
    lrn = SACLearner.from_modules(seq(10, (8,), 4), seq(12, (8,), 1), seq(12, (8,), 1), max_batch=32, device='cpu')
    before = [n.params.clone() for n in (lrn.actor,) + lrn.critics]
    B = 8
    good = dict(obs=torch.zeros(B, 10), action=torch.zeros(B, 2))
    tgt = torch.zeros(B)
    for batch, target, kw, text in (
            ({'obs': good['obs']}, tgt, {}, "'obs' and 'action'"),
            (dict(good, obs=torch.zeros(B, 9)), tgt, {}, r"batch\['obs'\]"),
            (dict(good, obs=torch.zeros(B, 10, dtype=torch.float64)), tgt, {}, r"batch\['obs'\]"),
            (dict(good, action=torch.zeros(B, 2, dtype=torch.int32)), tgt, {}, r"batch\['action'\]"),
            (dict(good, action=torch.zeros(B, 1)), tgt, {}, r"batch\['action'\]"),
            (good, torch.zeros(B + 1), {}, 'target'),
            (good, tgt, dict(weight=torch.zeros(B, 1)), 'weight'),
            (good, tgt, dict(td_abs_out=torch.zeros(B, dtype=torch.float64)), 'td_abs_out'),
            (good, tgt, dict(q_out=torch.zeros(B, 1)), 'q_out'),
            (dict(obs=torch.zeros(33, 10), action=torch.zeros(33, 2)), torch.zeros(33), {}, 'max_batch=32'),
            (good, tgt, {}, 'SACLearner.step_critic: .*no CPU path')):
        with pytest.raises(ValueError, match=text):
            lrn.step_critic(batch, target, **kw)
    for batch, kw, text in (({}, {}, "'obs'"), (good, dict(action_out=torch.zeros(B, 1)), 'action_out'), (good, dict(logp_out=torch.zeros(B, 1)), 'logp_out'),
                            (good, dict(q_out=torch.zeros(B + 1)), 'q_out'), (good, {}, 'SACLearner.step_actor: .*no CPU path')):
        with pytest.raises(ValueError, match=text):
            lrn.step_actor(batch, **kw)
    for call in (lambda: lrn.grad_critic(good, tgt), lambda: lrn.grad_actor(good), lambda: lrn.step(good, tgt)):
        with pytest.raises(ValueError, match='no CPU path'):
            call()
    with pytest.raises(ValueError, match='td.SacTarget'):
        lrn.update_targets(seq(10, (8,), 4))
    assert all(torch.equal(n.params, b) for n, b in zip((lrn.actor,) + lrn.critics, before)) and lrn.draws.tolist() == [0]


def test_update_targets_on_the_host():
    """update_targets is torch on the flat buffers, so it runs here: lerp_ / copy_ of the critics bit for bit with the target modules
    following, the learner's actor copied into the buffer the target reads its ONLINE actor from; shapes and the critic count checked"""
    from soccer2d_amd.learn import SACLearner
    from soccer2d_amd.td import SacTarget
    torch.manual_seed(4)
    mk = lambda: (seq(10, (16, 8), 4), seq(12, (16,), 1), seq(12, (8, 8), 1, act=nn.Tanh))
    mods, other = mk(), mk()
    tmods = mk()[1:]
    lrn = SACLearner.from_modules(*mods, device='cpu')
    tgt = SacTarget.from_modules(other[0], *tmods, device='cpu')             # a target made from ANOTHER actor: update_targets replaces it
    assert not torch.equal(tgt.actor.params, lrn.actor.params)
    old = [t.params.clone() for t in tgt.critics]
    lrn.update_targets(tgt, tau=0.005)
    for n, t, o, m in zip(lrn.critics, tgt.critics, old, tmods):
        assert torch.equal(t.params, o.lerp(n.params, 0.005)) and not torch.equal(t.params, o)
        assert torch.equal(torch.cat([p.detach().reshape(-1) for p in m.parameters()]), t.params)
    assert torch.equal(tgt.actor.params, lrn.actor.params) and tgt.actor.params.data_ptr() != lrn.actor.params.data_ptr()
    for n in tgt.critics:
        n.sync()                                                             # the module round trip still works
    assert all(torch.equal(t.params, o.lerp(n.params, 0.005)) for n, t, o in zip(lrn.critics, tgt.critics, old))
    lrn.update_targets(tgt)
    for n, t, m in zip(lrn.critics, tgt.critics, tmods):
        assert torch.equal(t.params, n.params) and torch.equal(torch.cat([p.detach().reshape(-1) for p in m.parameters()]), n.params)
    same_actor = SacTarget.from_modules(mods[0], *mk()[1:], device='cpu')    # the usual case: the target was made from the learner's actor
    with torch.no_grad():
        lrn.actor.params.add_(1.0)
    lrn.update_targets(same_actor, tau=0.5)
    assert torch.equal(same_actor.actor.params, lrn.actor.params)
    with pytest.raises(ValueError, match='critic'):
        lrn.update_targets(SacTarget.from_modules(*mk()[:2], device='cpu'))
    with pytest.raises(ValueError, match='target critic 1 is'):
        lrn.update_targets(SacTarget.from_modules(mk()[0], seq(12, (32,), 1), mk()[2], device='cpu'))
    with pytest.raises(ValueError, match='the actor is'):
        lrn.update_targets(SacTarget.from_modules(seq(10, (16, 16), 4), *mk()[1:], device='cpu'))
    with pytest.raises(ValueError, match='tau'):
        lrn.update_targets(tgt, tau=1.5)
