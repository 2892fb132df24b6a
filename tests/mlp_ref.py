"""ctypes binding of tests/mlp_ref.c (the host restatement of the fused actors' general MLP: generic depth, the k = 0 .. 11 first
layer, relu / tanh_spec, argmax, and the tanh actor's head on its outputs) and the epsilon-greedy choice built on
tests/qnet_ref.py's draws.  TEST INFRASTRUCTURE: compiled on demand with -ffp-contract=off (the fp32 contract, DESIGN.md
section 4)."""
import ctypes as C
import os
import subprocess

import numpy as np

import qnet_ref as Q

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'mlp_ref.c')
ACT = {'relu': 0, 'tanh': 1}


def build(outdir):
    so = os.path.join(str(outdir), 'libmlp_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC, '-lm'], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    L.mlp_forward.restype = None
    L.mlp_forward.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.mlp_argmax.restype = None
    L.mlp_argmax.argtypes = [C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
    L.mlp_actor_actions.restype = None
    L.mlp_actor_actions.argtypes = [C.c_int64, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_uint64, C.c_uint64,
                                    C.c_void_p, C.c_void_p]
    return L


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def param_count(hidden, na):
    n, win = 0, 10
    for w in tuple(hidden) + (na,):
        n += w * win + w
        win = w
    return n


def forward(L, x, params, hidden, na, act, first_k=12):
    """y[n][na] of observations x[n][10]; act 'relu' | 'tanh'; first_k = 12 is the spec (10: without layer 1's padding terms)"""
    x, params = _f32(x), _f32(params)
    assert params.size == param_count(hidden, na), (params.size, param_count(hidden, na))
    h = np.ascontiguousarray(hidden, dtype=np.int32)
    y = np.zeros((x.shape[0], na), dtype=np.float32)
    L.mlp_forward(x.shape[0], x.ctypes.data, params.ctypes.data, len(h), h.ctypes.data, na, ACT[act], first_k, y.ctypes.data)
    return y


def argmax(L, y):
    y = _f32(y)
    out = np.zeros(y.shape[0], dtype=np.int32)
    L.mlp_argmax(y.shape[0], y.ctypes.data, y.shape[1], out.ctypes.data)
    return out


def q_actions(L, Lq, obs, params, hidden, na, act, eps, seed, gid, k):
    """the Q actor's action per env: explore (block 2 word < thr) -> S2D_ACT_RANDOM's draw (block 0), else the greedy action
    (Lq = qnet_ref's library: the threshold; the draws are qnet_ref.policy_word's)"""
    g = argmax(L, forward(L, obs, params, hidden, na, act))
    thr = Q.threshold(Lq, eps)
    explore = Q.policy_word(seed, gid, k, 2).astype(np.uint64) < np.uint64(thr)
    rnd = ((Q.policy_word(seed, gid, k, 0).astype(np.uint64) * np.uint64(na)) >> np.uint64(32)).astype(np.int32)
    return np.where(explore, rnd, g).astype(np.int32)


def actor_actions(L, obs, params, hidden, na, act, eps, kind, noise, seed, k, gid0=0):
    """the tanh actor's action [n][na] per env at policy steps k (int array)"""
    y = forward(L, obs, params, hidden, na, act)
    noise = _f32(np.zeros((2, na)) if noise is None else noise)
    k = np.ascontiguousarray(np.asarray(k) & 0xFFFFFFFF, dtype=np.uint32)
    out = np.zeros((y.shape[0], na), dtype=np.float32)
    L.mlp_actor_actions(y.shape[0], y.ctypes.data, na, float(eps), int(kind), noise.ctypes.data, int(seed), int(gid0),
                        k.ctypes.data, out.ctypes.data)
    return out
