"""ctypes binding of tests/td_ref.c (the host restatement of s2d_td_target_q / s2d_td_target_ac: S2DWideNet's MLP with a general
input width, the argmax, the two-rounding target, the tanh head, the critics' input row and the twin minimum) and what the TD
tests share: networks as NumPy parameter vectors and a float64 forward.  TEST INFRASTRUCTURE: compiled on demand with
-ffp-contract=off (the fp32 contract)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'td_ref.c')
ACT = {'relu': 0, 'tanh': 1, 'sigmoid': 2}
F = np.float32


class TdNet(C.Structure):
    _fields_ = [('n_in', C.c_int32), ('n_hidden', C.c_int32), ('hidden', C.c_int32 * 5), ('n_out', C.c_int32),
                ('activation', C.c_int32), ('params', C.c_void_p)]


def build(outdir):
    so = os.path.join(str(outdir), 'libtd_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC, '-lm'], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    V, N = C.c_void_p, C.POINTER(TdNet)
    L.td_forward.restype, L.td_forward.argtypes = None, [C.c_int64, N, V, V]
    L.td_target_q.restype, L.td_target_q.argtypes = None, [C.c_int64, N, N, V, V, V, V, V, V]
    L.td_target_ac.restype, L.td_target_ac.argtypes = None, [C.c_int64, N, N, N, V, V, V, V, V, V]
    return L


def param_count(n_in, hidden, n_out):
    n, win = 0, n_in
    for w in tuple(hidden) + (n_out,):
        n += w * win + w
        win = w
    return n


class Net:
    """a network of the spec: shape, activation name and the parameters in nn.Sequential order (float32)"""

    def __init__(self, n_in, hidden, n_out, act, params):
        self.n_in, self.hidden, self.n_out, self.act = int(n_in), tuple(int(w) for w in hidden), int(n_out), act
        self.params = np.ascontiguousarray(params, dtype=F)
        assert self.params.size == param_count(n_in, hidden, n_out), (self.params.size, param_count(n_in, hidden, n_out))

    def c(self):
        s = TdNet(self.n_in, len(self.hidden), (C.c_int32 * 5)(*self.hidden), self.n_out, ACT[self.act], self.params.ctypes.data)
        return s

    def layers(self):
        """[(W [out][in], b [out])] as views of params"""
        out, off, win = [], 0, self.n_in
        for w in self.hidden + (self.n_out,):
            out.append((self.params[off:off + w * win].reshape(w, win), self.params[off + w * win:off + w * win + w]))
            off += w * win + w
            win = w
        return out


def random_net(rs, n_in, hidden, n_out, act, gain=1.0):
    """weights and biases U(-1, 1) / sqrt(fan_in) * gain, as torch initialises a Linear: activations stay O(1) at every width"""
    parts, win = [], n_in
    for w in tuple(hidden) + (n_out,):
        s = gain / np.sqrt(win)
        parts += [rs.uniform(-s, s, w * win), rs.uniform(-s, s, w)]
        win = w
    return Net(n_in, hidden, n_out, act, np.concatenate(parts).astype(F))


def _f32(a):
    return np.ascontiguousarray(a, dtype=F)


def _ref(net):
    return C.byref(net) if net is not None else None


def forward(L, net, x):
    x = _f32(x)
    assert x.ndim == 2 and x.shape[1] == net.n_in
    y = np.zeros((x.shape[0], net.n_out), F)
    c = net.c()
    L.td_forward(x.shape[0], C.byref(c), x.ctypes.data, y.ctypes.data)
    return y


def target_q(L, target, online, next_obs, reward, discount):
    """(target [B], q [B], index [B] int32)"""
    x, r, d = _f32(next_obs), _f32(reward), _f32(discount)
    B = x.shape[0]
    assert x.shape == (B, target.n_in) and r.shape == (B,) and d.shape == (B,)
    t, q, i = np.zeros(B, F), np.zeros(B, F), np.zeros(B, np.int32)
    ct, co = target.c(), (online.c() if online is not None else None)
    L.td_target_q(B, C.byref(ct), _ref(co), x.ctypes.data, r.ctypes.data, d.ctypes.data, t.ctypes.data, q.ctypes.data, i.ctypes.data)
    return t, q, i


def target_ac(L, actor, critic1, critic2, next_obs, reward, discount):
    """(target [B], q [B], action [B][A])"""
    x, r, d = _f32(next_obs), _f32(reward), _f32(discount)
    B = x.shape[0]
    assert x.shape == (B, actor.n_in) and critic1.n_in == actor.n_in + actor.n_out and critic1.n_out == 1
    t, q, a = np.zeros(B, F), np.zeros(B, F), np.zeros((B, actor.n_out), F)
    ca, c1, c2 = actor.c(), critic1.c(), (critic2.c() if critic2 is not None else None)
    L.td_target_ac(B, C.byref(ca), C.byref(c1), _ref(c2), x.ctypes.data, r.ctypes.data, d.ctypes.data, t.ctypes.data, q.ctypes.data,
                   a.ctypes.data)
    return t, q, a


def forward64(net, x):
    """the network in float64 NumPy on the same float32 parameters and rows"""
    h = np.asarray(x, np.float64)
    layers = net.layers()
    for l, (W, b) in enumerate(layers):
        h = h @ W.astype(np.float64).T + b.astype(np.float64)
        if l < len(layers) - 1:
            h = np.maximum(h, 0.0) if net.act == 'relu' else np.tanh(h) if net.act == 'tanh' else 1.0 / (1.0 + np.exp(-h))
    return h


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)
