"""float64 forward of the fused actors' MLP with a rigorous running bound on the fp32 spec's distance from it, for relu, tanh and
sigmoid networks: tests/test_gpu_mlp_actor.py's f64_bound, extended by the activation.  TEST INFRASTRUCTURE, shared by
tests/test_wide_actor_host.py and tests/test_gpu_wide_actor.py."""
import numpy as np

import wide_ref as W

F = np.float32


def views(p, hidden, na):
    """[W_1, b_1, ..., W_out, b_out]: writable views into the packed parameter vector p (nn.Sequential order)"""
    out, o, win = [], 0, 10
    for w in tuple(hidden) + (na,):
        for shape in ((w, win), (w,)):
            s = int(np.prod(shape))
            out.append(p[o:o + s].reshape(shape))
            o += s
        win = w
    return out


def gamma(k):
    u = 2.0 ** -24
    return k * u / (1 - k * u)


# activation -> (float64 function, Lipschitz constant, the spec function's absolute error against it)
ACTS = {'relu': (lambda v: np.maximum(v, 0.0), 1.0, 0.0),
        'tanh': (np.tanh, 1.0, 1e-6),
        'sigmoid': (lambda v: 1.0 / (1.0 + np.exp(-v)), 0.25, W.SIGMOID_ERR)}


def f64_bound(params, x, hidden, na, act):
    """y64 (the network in float64 on the same float32 inputs) and a rigorous bound on |y - y64| per output.  Per layer a
    k-ordered fmaf chain of K terms (K = 12 in layer 1) gives e_pre = |W| e + gamma_K (|b| + |W| (|a| + e)) + K 2^-149; behind
    every hidden unit the activation carries it on with its Lipschitz constant (relu, tanh: 1; sigmoid: 1/4) and adds the spec
    function's own error against float64 (relu: none; tanh_spec: its stated 1e-6; sigmoid_spec: the measured SIGMOID_ERR)."""
    fn, lip, err = ACTS[act]
    v = [t.astype(np.float64) for t in views(np.array(params, dtype=F), hidden, na)]
    a, e, K = x.astype(np.float64), np.zeros(x.shape), 12
    for l, (Wl, b) in enumerate(zip(v[0::2], v[1::2])):
        pre = a @ Wl.T + b
        e = e @ np.abs(Wl).T + gamma(K) * (np.abs(b) + (np.abs(a) + e) @ np.abs(Wl).T) + K * 2.0 ** -149
        if l < len(hidden):
            a, e = fn(pre), lip * e + err
        else:
            a = pre
        K = Wl.shape[0]
    return a, e


def random_net(rs, hidden, na):
    """weights and biases N(0, 1 / fan_in)"""
    p = np.zeros(W.param_count(hidden, na), dtype=F)
    fans = [f for w in (10,) + tuple(hidden) for f in (w, w)]
    for v, fan in zip(views(p, hidden, na), fans):
        v[...] = rs.normal(0, 1 / np.sqrt(fan), v.shape)
    return p


def sparse_net(rs, hidden, na):
    """every unit reads 8 inputs of the layer below, N(0, 1 / 8); biases N(0, 0.1).  Drawn per layer: all rows of W, then b"""
    p = np.zeros(W.param_count(hidden, na), dtype=F)
    v = views(p, hidden, na)
    for Wl, b in zip(v[0::2], v[1::2]):
        for j in range(Wl.shape[0]):
            Wl[j, rs.choice(Wl.shape[1], 8, replace=False)] = rs.normal(0, 1 / np.sqrt(8), 8)
        b[...] = rs.normal(0, 0.1, b.shape)
    return p
