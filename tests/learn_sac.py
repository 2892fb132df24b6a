"""ctypes binding of tests/learn_sac_ref.c (the host restatement of s2d_learn_sac_actor / s2d_learn_sac_actor_grad: the squashed-Gaussian
actor's step through min(Q1, Q2) and the temperature's step) and what the tests of the fused SAC update share: the shape list,
networks and batches, and a float64 / float32 torch autograd of the example's loss_pi and loss_alpha on given z.  Networks are
tests/td.py's Net, the optimiser's state tests/learn.py's State; SAC's critic step is learn_ac.critic_step with loss 'mse'.
TEST INFRASTRUCTURE: compiled on demand with -ffp-contract=off."""
import ctypes as C
import os
import subprocess

import numpy as np

import learn as LR
import td as TD

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'learn_sac_ref.c')
F = np.float32
BLOCK_ROWS = LR.BLOCK_ROWS
STREAM = 14   # S2D_LEARN_SAC_STREAM

# (D, A, actor hidden, critic 1 hidden, critic 2 hidden or None, (actor, critic 1, critic 2) activations)
SHAPES = [
    (1, 1, (8,), (8,), (8,), ('relu',) * 3),                             # the critics' row is padded 2 -> 4
    (10, 1, (64, 64), (64, 64), (64, 64), ('relu',) * 3),                # reach-ball: the image is in LDS
    (10, 4, (64, 64), (64, 32), (32, 16), ('tanh', 'relu', 'tanh')),     # the turning action, unequal critics, mixed activations
    (13, 8, (24, 40), (40, 24), (24,), ('sigmoid',) * 3),                # A = 8: the second Philox block
    (10, 1, (64, 64), (64, 64), None, ('relu',) * 3),                    # one critic
    (10, 1, (256, 256), (256, 256), (256, 256), ('relu',) * 3),          # SB3's default: the image lives in the workspace
    (248, 8, (256, 256), (256, 256), (256, 256), ('relu',) * 3),         # the widest rows
]
REACH_BALL = SHAPES[1]


def shape_id(s):
    x = lambda h: 'x'.join(map(str, h)) if h is not None else 'none'
    return f'{s[0]}+{s[1]}-{x(s[2])}-{x(s[3])}-{x(s[4])}-' + '.'.join(a[0] for a in s[5])


def build(outdir):
    so = os.path.join(str(outdir), 'liblearn_sac_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-I', HERE, '-I', os.path.join(ROOT, 'include'), '-o', so, SRC,
                    '-lm'], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    V, N, f, B, U = C.c_void_p, C.POINTER(LR.LearnNet), C.c_float, C.c_int64, C.c_uint64
    L.learn_sac_z.restype, L.learn_sac_z.argtypes = None, [B, C.c_int, U, U, V]
    L.learn_sac_actor_grad.restype = None
    L.learn_sac_actor_grad.argtypes = [B, N, N, N, V, f, V, U, U, f, V, V, V, V, V, V, V, V]
    L.learn_sac_alpha.restype, L.learn_sac_alpha.argtypes = None, [f, f, C.c_int, V, V, V, V, V]
    L.learn_sac_actor_step.restype = None
    L.learn_sac_actor_step.argtypes = [B, N, N, N, V, V, V, V, V, V, f, V, U, V, V, V, V, V, V, V, V]
    # what learn_ac_ref.c and learn_ref.c export from the same library
    I = C.c_int
    L.learn_ac_critic_grad.restype, L.learn_ac_critic_grad.argtypes = None, [B, N, I, I, V, V, V, V, f, V, V, V, V]
    L.learn_ac_critic_step.restype, L.learn_ac_critic_step.argtypes = None, [B, N, I, I, V, V, V, V, V, V, V, V, V, V, V]
    L.learn_forward.restype, L.learn_forward.argtypes = None, [B, N, V, V]
    return L


_p = LR._p


def random_nets(rs, shape, gain=1.0):
    """(actor D-ha-2A, critic 1, critic 2 or None) of a SHAPES entry with torch's Linear initialisation"""
    D, A, ha, h1, h2, acts = shape
    actor = TD.random_net(rs, D, ha, 2 * A, acts[0], gain)
    c1 = TD.random_net(rs, D + A, h1, 1, acts[1], gain)
    c2 = TD.random_net(rs, D + A, h2, 1, acts[2], gain) if h2 is not None else None
    return actor, c1, c2


def z(L, n, A, seed, draws):
    """the step's z [n][A] of rows 0 .. n-1 at call `draws`"""
    out = np.zeros((n, A), F)
    L.learn_sac_z(n, A, int(seed), int(draws), out.ctypes.data)
    return out


class AlphaState:
    """the temperature's state of the spec: log_alpha, (m, v), hyper, stats, and the alpha word the rows read"""

    def __init__(self, target_entropy, log_alpha=0.0, lr=3e-4, betas=(0.9, 0.999), eps=1e-8):
        self.log_alpha, self.m_v = np.array([log_alpha], F), np.zeros(2, F)
        self.hyper = np.array([lr, betas[0], betas[1], eps, 0.0, 1.0, 1.0], F)
        self.stats = np.zeros(3, F)
        self.target_entropy = float(target_entropy)


def _nets(actor, c1, c2):
    return LR.c_net(actor), LR.c_net(c1), (LR.c_net(c2) if c2 is not None else None)


def actor_grad(L, actor, c1, c2, obs, alpha, z=None, seed=0, draws=0, max_grad_norm=0.0):
    """dict(grad [P of the actor], stats (mean of alpha logp - q, norm, scale), mean_logp, action [B][A], logp [B], q [B], du [B][A],
    dls [B][A]); z [B][A] given, or drawn at (seed, draws); the critics are only read"""
    obs = np.ascontiguousarray(obs, F)
    B, A = obs.shape[0], actor.n_out // 2
    assert obs.shape == (B, actor.n_in) and c1.n_in == actor.n_in + A and c1.n_out == 1 and (c2 is None or c2.n_in == c1.n_in)
    zz = np.ascontiguousarray(z, F) if z is not None else None
    assert zz is None or zz.shape == (B, A)
    g, stats, ml = np.zeros(actor.params.size, F), np.zeros(3, F), np.zeros(1, F)
    act, lp, q, du, dls = np.zeros((B, A), F), np.zeros(B, F), np.zeros(B, F), np.zeros((B, A), F), np.zeros((B, A), F)
    a, k1, k2 = _nets(actor, c1, c2)
    L.learn_sac_actor_grad(B, C.byref(a), C.byref(k1), C.byref(k2) if k2 is not None else None, _p(obs), float(F(alpha)), _p(zz), int(seed),
                           int(draws), max_grad_norm, _p(g), _p(stats), _p(ml), _p(act), _p(lp), _p(q), _p(du), _p(dls))
    return dict(grad=g, stats=stats, mean_logp=ml[0], action=act, logp=lp, q=q, du=du, dls=dls)


def alpha_stats(L, mean_logp, ast):
    """the temperature's stats[0..1] of a _grad call: nothing of `ast` is touched"""
    out = np.zeros(3, F)
    la = ast.log_alpha.copy()
    L.learn_sac_alpha(float(F(mean_logp)), float(F(ast.target_entropy)), 0, _p(la), None, None, _p(out), None)
    return out[:2]


def actor_step(L, actor, c1, c2, state, obs, alpha, ast, draws, seed):
    """one s2d_learn_sac_actor on actor.params, state, alpha [1] and draws [1] (uint64) and (ast an AlphaState, or None: a fixed
    coefficient) the temperature, all in place; returns dict(grad, stats, action, logp, q)"""
    obs = np.ascontiguousarray(obs, F)
    B, A = obs.shape[0], actor.n_out // 2
    assert alpha.dtype == F and alpha.shape == (1,) and draws.dtype == np.uint64 and draws.shape == (1,)
    g, stats = np.zeros(actor.params.size, F), np.zeros(3, F)
    act, lp, q = np.zeros((B, A), F), np.zeros(B, F), np.zeros(B, F)
    a, k1, k2 = _nets(actor, c1, c2)
    L.learn_sac_actor_step(B, C.byref(a), C.byref(k1), C.byref(k2) if k2 is not None else None, _p(obs), _p(alpha),
                           _p(ast.log_alpha) if ast else None, _p(ast.m_v) if ast else None, _p(ast.hyper) if ast else None,
                           _p(ast.stats) if ast else None, float(F(ast.target_entropy)) if ast else 0.0, _p(draws), int(seed),
                           _p(state.m), _p(state.v), _p(g), _p(state.hyper), _p(stats), _p(act), _p(lp), _p(q))
    return dict(grad=g, stats=stats, action=act, logp=lp, q=q)


def critic_step(L, critic, state, obs, action, target, weight=None):
    """SAC's critic step: learn_ac_ref.c's with S2D_LEARN_MSE; dict(grad, stats, td_abs, q)"""
    obs, action, target = (np.ascontiguousarray(a, F) for a in (obs, action, target))
    B, A = action.shape
    g, stats, td_abs, q = np.zeros(critic.params.size, F), np.zeros(3, F), np.zeros(B, F), np.zeros(B, F)
    c = LR.c_net(critic)
    L.learn_ac_critic_step(B, C.byref(c), A, 0, _p(obs), _p(action), _p(target), _p(weight), _p(state.m), _p(state.v), _p(g),
                           _p(state.hyper), _p(stats), _p(td_abs), _p(q))
    return dict(grad=g, stats=stats, td_abs=td_abs, q=q)


def forward(L, net, x):
    return LR.forward(L, net, x)


def torch_losses(actor, c1, c2, obs, z, alpha, log_alpha, target_entropy, dtype):
    """the example's loss_pi and loss_alpha on given z by torch autograd in `dtype`: dict(grad (the actor's flat gradient, float64
    NumPy), loss_pi, mean_logp, dalpha (d loss_alpha / d log_alpha), loss_alpha, q1, q2, v, u (NumPy, for the tests' conditions))"""
    import math

    import torch
    mod = LR.torch_module(actor, dtype)
    q1m, q2m = LR.torch_module(c1, dtype), (LR.torch_module(c2, dtype) if c2 is not None else None)
    o, zz = torch.from_numpy(np.asarray(obs)).to(dtype), torch.from_numpy(np.asarray(z)).to(dtype)
    mean, v = mod(o).chunk(2, dim=1)
    ls = v.clamp(-20.0, 2.0)
    u = mean + ls.exp() * zz
    a = torch.tanh(u)
    logp = (-0.5 * zz * zz - ls - 0.5 * math.log(2 * math.pi) - torch.log(1 - a * a + 1e-6)).sum(dim=1)
    x = torch.cat([o, a], 1)
    q1 = q1m(x).squeeze(1)
    q2 = q2m(x).squeeze(1) if q2m is not None else None
    q = torch.min(q1, q2) if q2 is not None else q1
    loss_pi = (float(alpha) * logp - q).mean()
    loss_pi.backward()
    la = torch.tensor([float(log_alpha)], dtype=dtype, requires_grad=True)
    loss_alpha = -(la * (logp.detach() + float(target_entropy)).mean())
    loss_alpha.backward()
    flat = np.concatenate([p.grad.detach().double().numpy().reshape(-1) for p in mod.parameters()])
    n = lambda t: t.detach().double().numpy() if t is not None else None
    return dict(grad=flat, loss_pi=float(loss_pi.detach()), mean_logp=float(logp.detach().mean()), dalpha=float(la.grad[0]),
                loss_alpha=float(loss_alpha.detach()), q1=n(q1), q2=n(q2), v=n(v), u=n(u))


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)
