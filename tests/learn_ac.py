"""ctypes binding of tests/learn_ac_ref.c (the host restatement of s2d_learn_critic / s2d_learn_actor and their _grad twins: the
critic's step on [obs | action] and the actor's step through a read-only critic) and what the tests of the fused DDPG / TD3 update
share: the shape list, batches and a float64 / float32 torch autograd of the example's losses.  Networks are tests/td.py's Net, the
optimiser's state tests/learn.py's State.  TEST INFRASTRUCTURE: compiled on demand with -ffp-contract=off."""
import ctypes as C
import os
import subprocess

import numpy as np

import learn as LR
import td as TD

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'learn_ac_ref.c')
F = np.float32
BLOCK_ROWS = LR.BLOCK_ROWS
LOSS = {'mse': 0, 'huber': 1, 'square': 2}

# (D, A, actor hidden, critic hidden, activation of both)
SHAPES = [
    (1, 1, (8,), (8,), 'relu'),                      # the critic's row is padded 2 -> 4
    (10, 1, (64, 64), (64, 64), 'relu'),             # reach-ball's default: 11 -> 12
    (10, 4, (16, 8), (64, 32, 16, 8), 'tanh'),       # the reference's pi / qf: 14 -> 16
    (4, 4, (64, 64), (64, 64), 'relu'),              # GoToCenter: no pad
    (13, 8, (24, 40), (40, 24), 'sigmoid'),          # 21 -> 24, the largest A
    (248, 8, (256, 256), (256, 256), 'relu'),        # the image lives in the workspace
]
REACH_BALL = SHAPES[1]


def shape_id(s):
    return f'{s[0]}+{s[1]}-' + 'x'.join(map(str, s[2])) + '-' + 'x'.join(map(str, s[3])) + '-' + s[4]


def build(outdir):
    so = os.path.join(str(outdir), 'liblearn_ac_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC, '-lm'], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    V, N, I, f, B = C.c_void_p, C.POINTER(LR.LearnNet), C.c_int, C.c_float, C.c_int64
    L.learn_ac_critic_grad.restype, L.learn_ac_critic_grad.argtypes = None, [B, N, I, I, V, V, V, V, f, V, V, V, V]
    L.learn_ac_critic_step.restype, L.learn_ac_critic_step.argtypes = None, [B, N, I, I, V, V, V, V, V, V, V, V, V, V, V]
    L.learn_ac_actor_grad.restype, L.learn_ac_actor_grad.argtypes = None, [B, N, N, V, f, V, V, V, V]
    L.learn_ac_actor_step.restype, L.learn_ac_actor_step.argtypes = None, [B, N, N, V, V, V, V, V, V, V, V]
    return L


_p = LR._p


def random_pair(rs, D, A, ha, hc, act, act_c=None, gain=1.0):
    """(actor D-ha-A, critic (D + A)-hc-1) with torch's Linear initialisation"""
    return TD.random_net(rs, D, ha, A, act, gain), TD.random_net(rs, D + A, hc, 1, act_c or act, gain)


def random_batch(rs, critic, A, B):
    """obs U(-1, 1), actions U(-1, 1), targets = the critic's value + N(0.5, 0.7), weights U(0.2, 1).  The TD errors fall on both
    sides of 0 and of Huber's +-1, but do not average to zero: with ONE output column every row's delta lands in the same output
    bias, and a sum of zero-mean terms has a condition number sum|t| / |sum t| of about sqrt(B), at which the rounding error of
    any fixed summation order is a matter of luck relative to another order's.  With the mean at 0.5 it is about 1.4, so a
    comparison with torch's error on the same inputs says something about the gradient and not about the order of a sum."""
    D = critic.n_in - A
    obs, action = rs.uniform(-1, 1, (B, D)).astype(F), rs.uniform(-1, 1, (B, A)).astype(F)
    q = TD.forward64(critic, np.concatenate([obs, action], 1))[:, 0]
    return obs, action, (q + rs.normal(0.5, 0.7, B)).astype(F), rs.uniform(0.2, 1.0, B).astype(F)


def _critic_args(critic, obs, action, target, weight):
    obs, action, target = (np.ascontiguousarray(a, F) for a in (obs, action, target))
    weight = np.ascontiguousarray(weight, F) if weight is not None else None
    B, A = action.shape
    assert obs.shape == (B, critic.n_in - A) and target.shape == (B,) and (weight is None or weight.shape == (B,)) and critic.n_out == 1
    return B, A, obs, action, target, weight


def critic_grad(L, critic, loss, obs, action, target, weight=None, max_grad_norm=0.0):
    """dict(grad [P], stats (loss, norm, scale), td_abs [B], q [B])"""
    B, A, obs, action, target, weight = _critic_args(critic, obs, action, target, weight)
    g, stats, td_abs, q = np.zeros(critic.params.size, F), np.zeros(3, F), np.zeros(B, F), np.zeros(B, F)
    c = LR.c_net(critic)
    L.learn_ac_critic_grad(B, C.byref(c), A, LOSS[loss], _p(obs), _p(action), _p(target), _p(weight), max_grad_norm, _p(g), _p(stats),
                           _p(td_abs), _p(q))
    return dict(grad=g, stats=stats, td_abs=td_abs, q=q)


def critic_step(L, critic, state, loss, obs, action, target, weight=None):
    """one s2d_learn_critic on critic.params and state (both in place); returns critic_grad()'s dict"""
    B, A, obs, action, target, weight = _critic_args(critic, obs, action, target, weight)
    g, stats, td_abs, q = np.zeros(critic.params.size, F), np.zeros(3, F), np.zeros(B, F), np.zeros(B, F)
    c = LR.c_net(critic)
    L.learn_ac_critic_step(B, C.byref(c), A, LOSS[loss], _p(obs), _p(action), _p(target), _p(weight), _p(state.m), _p(state.v), _p(g),
                           _p(state.hyper), _p(stats), _p(td_abs), _p(q))
    return dict(grad=g, stats=stats, td_abs=td_abs, q=q)


def _actor_args(actor, critic, obs):
    obs = np.ascontiguousarray(obs, F)
    assert obs.ndim == 2 and obs.shape[1] == actor.n_in and critic.n_in == actor.n_in + actor.n_out and critic.n_out == 1
    return obs.shape[0], obs


def actor_grad(L, actor, critic, obs, max_grad_norm=0.0):
    """dict(grad [P of the actor], stats (-mean q, norm, scale), action [B][A], q [B]); the critic is only read"""
    B, obs = _actor_args(actor, critic, obs)
    g, stats, act, q = np.zeros(actor.params.size, F), np.zeros(3, F), np.zeros((B, actor.n_out), F), np.zeros(B, F)
    a, c = LR.c_net(actor), LR.c_net(critic)
    L.learn_ac_actor_grad(B, C.byref(a), C.byref(c), _p(obs), max_grad_norm, _p(g), _p(stats), _p(act), _p(q))
    return dict(grad=g, stats=stats, action=act, q=q)


def actor_step(L, actor, critic, state, obs):
    """one s2d_learn_actor on actor.params and state (both in place); returns actor_grad()'s dict"""
    B, obs = _actor_args(actor, critic, obs)
    g, stats, act, q = np.zeros(actor.params.size, F), np.zeros(3, F), np.zeros((B, actor.n_out), F), np.zeros(B, F)
    a, c = LR.c_net(actor), LR.c_net(critic)
    L.learn_ac_actor_step(B, C.byref(a), C.byref(c), _p(obs), _p(state.m), _p(state.v), _p(g), _p(state.hyper), _p(stats), _p(act), _p(q))
    return dict(grad=g, stats=stats, action=act, q=q)


def _flat(mod):
    return np.concatenate([p.grad.detach().double().numpy().reshape(-1) for p in mod.parameters()])


def torch_critic_grad(critic, loss, obs, action, target, weight, dtype):
    """(flat gradient as float64 NumPy, loss) of the example's critic loss by torch autograd: F.mse_loss ('square'), e^2 / 2 ('mse')
    or smooth_l1_loss ('huber') of q(cat(obs, action)) against target, weighted per row where given, mean over the batch"""
    import torch
    mod = LR.torch_module(critic, dtype)
    o, a, t = (torch.from_numpy(np.asarray(x)).to(dtype) for x in (obs, action, target))
    q = mod(torch.cat([o, a], 1)).squeeze(1)
    fn = torch.nn.functional
    per = fn.mse_loss(q, t, reduction='none') if loss == 'square' else fn.smooth_l1_loss(q, t, reduction='none') if loss == 'huber' else 0.5 * (q - t) ** 2
    if weight is not None:
        per = torch.from_numpy(np.asarray(weight)).to(dtype) * per
    total = per.mean()
    total.backward()
    return _flat(mod), float(total.detach())


def torch_actor_grad(actor, critic, obs, dtype):
    """(the actor's flat gradient, the critic's flat gradient, loss) of -q(cat(o, tanh(mu(o)))).mean() by torch autograd"""
    import torch
    mu, q = LR.torch_module(actor, dtype), LR.torch_module(critic, dtype)
    o = torch.from_numpy(np.asarray(obs)).to(dtype)
    total = -q(torch.cat([o, torch.tanh(mu(o))], 1)).mean()
    total.backward()
    return _flat(mu), _flat(q), float(total.detach())
