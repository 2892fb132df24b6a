"""ctypes binding of tests/learn_ref.c (the host restatement of s2d_learn_q / s2d_learn_q_grad: forward, TD error, MSE / Huber
derivative, backward, block and chunk reductions, clip, Adam) and what the learner's tests share: the shape list, batches and a
float64 / float32 torch autograd of the same loss.  Networks are tests/td.py's Net (NumPy parameter vectors in nn.Sequential order).
TEST INFRASTRUCTURE: compiled on demand with -ffp-contract=off (the fp32 contract)."""
import ctypes as C
import os
import subprocess

import numpy as np

import td as TD

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'learn_ref.c')
F = np.float32
BLOCK_ROWS = 64
NORM_CHUNK = 256
LOSS = {'mse': 0, 'huber': 1}

# (n_in, hidden, n_out, activation): every value of the issue's lists appears at least once
SHAPES = [
    (1, (8,), 1, 'relu'),
    (4, (8, 16), 3, 'tanh'),
    (13, (24, 40), 17, 'sigmoid'),            # tiles that are no multiples of 16
    (10, (64, 64), 16, 'relu'),               # SB3's default
    (10, (128, 64, 32, 16), 16, 'tanh'),      # the reference's; 64 rows of it need more than 64 KiB of LDS
    (256, (256, 256), 64, 'relu'),            # the widest: its activations live in the workspace
]


class LearnNet(C.Structure):
    _fields_ = [('n_in', C.c_int32), ('n_hidden', C.c_int32), ('hidden', C.c_int32 * 5), ('n_out', C.c_int32),
                ('activation', C.c_int32), ('params', C.c_void_p)]


def build(outdir):
    so = os.path.join(str(outdir), 'liblearn_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC, '-lm'], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    V, N, I, f = C.c_void_p, C.POINTER(LearnNet), C.c_int, C.c_float
    L.learn_param_count.restype, L.learn_param_count.argtypes = C.c_int64, [N]
    L.learn_forward.restype, L.learn_forward.argtypes = None, [C.c_int64, N, V, V]
    L.learn_grad.restype, L.learn_grad.argtypes = None, [C.c_int64, N, I, V, V, V, V, f, V, V, V, V, V]
    L.learn_adam.restype, L.learn_adam.argtypes = None, [C.c_int64, V, V, V, V, V, f]
    L.learn_step.restype, L.learn_step.argtypes = None, [C.c_int64, N, I, V, V, V, V, V, V, V, V, V, V, V, V]
    return L


def c_net(net):
    return LearnNet(net.n_in, len(net.hidden), (C.c_int32 * 5)(*net.hidden), net.n_out, TD.ACT[net.act], net.params.ctypes.data)


def _p(a):
    return a.ctypes.data if a is not None else None


def forward(L, net, x):
    x = np.ascontiguousarray(x, F)
    q = np.zeros((x.shape[0], net.n_out), F)
    c = c_net(net)
    L.learn_forward(x.shape[0], C.byref(c), x.ctypes.data, q.ctypes.data)
    return q


def _batch(net, obs, action, target, weight):
    obs, action, target = np.ascontiguousarray(obs, F), np.ascontiguousarray(action, np.int32), np.ascontiguousarray(target, F)
    weight = np.ascontiguousarray(weight, F) if weight is not None else None
    B = obs.shape[0]
    assert obs.shape == (B, net.n_in) and action.shape == (B,) and target.shape == (B,) and (weight is None or weight.shape == (B,))
    return B, obs, action, target, weight


def grad(L, net, loss, obs, action, target, weight=None, max_grad_norm=10.0):
    """dict(grad [P], stats (loss, norm, scale), td_abs [B], q [B][A], error)"""
    B, obs, action, target, weight = _batch(net, obs, action, target, weight)
    g, stats, td_abs, q = np.zeros(net.params.size, F), np.zeros(3, F), np.zeros(B, F), np.zeros((B, net.n_out), F)
    err = np.zeros(1, np.int32)
    c = c_net(net)
    L.learn_grad(B, C.byref(c), LOSS[loss], _p(obs), _p(action), _p(target), _p(weight), max_grad_norm, _p(g), _p(stats), _p(td_abs),
                 _p(q), _p(err))
    return dict(grad=g, stats=stats, td_abs=td_abs, q=q, error=int(err[0]))


class State:
    """the optimiser's state of the spec: m, v, hyper = (lr, beta1, beta2, eps, max_grad_norm, beta1^t, beta2^t)"""

    def __init__(self, P, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=10.0):
        self.m, self.v = np.zeros(P, F), np.zeros(P, F)
        self.hyper = np.array([lr, betas[0], betas[1], eps, max_grad_norm, 1.0, 1.0], F)


def adam(L, params, state, g, scale=1.0):
    """one Adam update of params (in place) with the gradient g * scale"""
    g = np.ascontiguousarray(g, F)
    L.learn_adam(params.size, _p(params), _p(state.m), _p(state.v), _p(g), _p(state.hyper), scale)


def step(L, net, state, loss, obs, action, target, weight=None):
    """one s2d_learn_q on net.params and state (both in place); returns grad()'s dict"""
    B, obs, action, target, weight = _batch(net, obs, action, target, weight)
    g, stats, td_abs, q = np.zeros(net.params.size, F), np.zeros(3, F), np.zeros(B, F), np.zeros((B, net.n_out), F)
    err = np.zeros(1, np.int32)
    c = c_net(net)
    L.learn_step(B, C.byref(c), LOSS[loss], _p(obs), _p(action), _p(target), _p(weight), _p(state.m), _p(state.v), _p(g), _p(state.hyper),
                 _p(stats), _p(td_abs), _p(q), _p(err))
    return dict(grad=g, stats=stats, td_abs=td_abs, q=q, error=int(err[0]))


def random_batch(rs, net, B):
    """obs U(-1, 1), actions uniform, targets = the net's value at the action + N(0, 0.7): TD errors on both sides of Huber's 1"""
    obs = rs.uniform(-1, 1, (B, net.n_in)).astype(F)
    action = rs.randint(0, net.n_out, B).astype(np.int32)
    qv = TD.forward64(net, obs)
    target = (qv[np.arange(B), action] + rs.normal(0, 0.7, B)).astype(F)
    weight = rs.uniform(0.2, 1.0, B).astype(F)
    return obs, action, target, weight


def torch_module(net, dtype):
    """the net as a torch nn.Sequential of `dtype` with the same parameters"""
    import torch
    acts = {'relu': torch.nn.ReLU, 'tanh': torch.nn.Tanh, 'sigmoid': torch.nn.Sigmoid}
    mods, layers = [], net.layers()
    for l, (W, b) in enumerate(layers):
        lin = torch.nn.Linear(W.shape[1], W.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(W.copy()))
            lin.bias.copy_(torch.from_numpy(b.copy()))
        mods.append(lin)
        if l < len(layers) - 1:
            mods.append(acts[net.act]())
    return torch.nn.Sequential(*mods).to(dtype)


def torch_grad(net, loss, obs, action, target, weight, dtype):
    """(flat gradient in nn.Sequential order as float64 NumPy, loss) of mean(weight * loss(q[action] - target)) by torch autograd"""
    import torch
    mod = torch_module(net, dtype)
    o, t = torch.from_numpy(np.asarray(obs)).to(dtype), torch.from_numpy(np.asarray(target)).to(dtype)
    a = torch.from_numpy(np.asarray(action)).long()
    q = mod(o).gather(1, a.unsqueeze(1)).squeeze(1)
    per = torch.nn.functional.smooth_l1_loss(q, t, reduction='none') if loss == 'huber' else 0.5 * (q - t) ** 2
    if weight is not None:
        per = torch.from_numpy(np.asarray(weight)).to(dtype) * per
    total = per.mean()
    total.backward()
    flat = np.concatenate([p.grad.detach().double().numpy().reshape(-1) for p in mod.parameters()])
    return flat, float(total.detach())


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)
