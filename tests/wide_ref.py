"""ctypes binding of tests/wide_ref.c (the host restatement of the fused actors' streamed-weight MLP: up to five layers of up to 400
units, relu / tanh_spec / sigmoid_spec) and the heads built on tests/mlp_ref.py's (the argmax, the epsilon-greedy choice, the tanh
actor's action: they work on the network's outputs and do not depend on its shape).  TEST INFRASTRUCTURE: compiled on demand
with -ffp-contract=off (the fp32 contract)."""
import ctypes as C
import os
import subprocess

import numpy as np

import mlp_ref as M
import qnet_ref as Q

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'wide_ref.c')
ACT = {'relu': 0, 'tanh': 1, 'sigmoid': 2}
param_count = M.param_count
argmax = M.argmax

# |sigmoid_spec(v) - 1 / (1 + exp(-v))| in float64 over [-100, 100]: the figure written next to the definition (s2d_device.h,
# DESIGN.md section 4), measured by tests/test_wide_actor_host.py
SIGMOID_ERR = 1.0e-7          # measured 8.93e-8 (at v = 8.66)


def build(outdir):
    so = os.path.join(str(outdir), 'libwide_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC, '-lm'], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    L.wide_forward.restype = None
    L.wide_forward.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.wide_sigmoid.restype = None
    L.wide_sigmoid.argtypes = [C.c_int64, C.c_void_p, C.c_void_p]
    return L


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def forward(L, x, params, hidden, na, act):
    """y[n][na] of observations x[n][10]; act 'relu' | 'tanh' | 'sigmoid'"""
    x, params = _f32(x), _f32(params)
    assert params.size == param_count(hidden, na), (params.size, param_count(hidden, na))
    h = np.ascontiguousarray(hidden, dtype=np.int32)
    y = np.zeros((x.shape[0], na), dtype=np.float32)
    L.wide_forward(x.shape[0], x.ctypes.data, params.ctypes.data, len(h), h.ctypes.data, na, ACT[act], y.ctypes.data)
    return y


def sigmoid(L, v):
    v = _f32(v)
    out = np.zeros_like(v)
    L.wide_sigmoid(v.size, v.ctypes.data, out.ctypes.data)
    return out


def q_actions(L, Lm, Lq, obs, params, hidden, na, act, eps, seed, gid, k):
    """the Q actor's action per env (Lm = mlp_ref's library: the argmax; Lq = qnet_ref's: the threshold), as mlp_ref.q_actions"""
    g = M.argmax(Lm, forward(L, obs, params, hidden, na, act))
    thr = Q.threshold(Lq, eps)
    explore = Q.policy_word(seed, gid, k, 2).astype(np.uint64) < np.uint64(thr)
    rnd = ((Q.policy_word(seed, gid, k, 0).astype(np.uint64) * np.uint64(na)) >> np.uint64(32)).astype(np.int32)
    return np.where(explore, rnd, g).astype(np.int32)


def actor_actions(L, Lm, obs, params, hidden, na, act, eps, kind, noise, seed, k, gid0=0):
    """the tanh actor's action [n][na] per env at policy steps k: mlp_ref's head on this network's outputs"""
    y = forward(L, obs, params, hidden, na, act)
    noise = _f32(np.zeros((2, na)) if noise is None else noise)
    k = np.ascontiguousarray(np.asarray(k) & 0xFFFFFFFF, dtype=np.uint32)
    out = np.zeros((y.shape[0], na), dtype=np.float32)
    Lm.mlp_actor_actions(y.shape[0], y.ctypes.data, na, float(eps), int(kind), noise.ctypes.data, int(seed), int(gid0),
                         k.ctypes.data, out.ctypes.data)
    return out
