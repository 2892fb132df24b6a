"""ctypes binding of tests/match_net_ref.c (the host restatement of the 11v11 network slots' forward pass, argmax and
epsilon threshold) and a numpy restatement of their exploration draws.  TEST INFRASTRUCTURE: compiled on demand with
-ffp-contract=off (the fp32 contract)."""
import ctypes as C
import os
import subprocess

import numpy as np

import qnet_ref as Q

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'match_net_ref.c')
DIM = 224
ST_NET = 7


def build(outdir):
    so = os.path.join(str(outdir), 'libmatch_net_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC, '-lm'], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    L.mnet_forward.restype = None
    L.mnet_forward.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.mnet_argmax.restype = None
    L.mnet_argmax.argtypes = [C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
    L.mnet_threshold.restype = C.c_uint64
    L.mnet_threshold.argtypes = [C.c_float]
    return L


def param_count(h1, h2, k):
    return h1 * DIM + h1 + h2 * h1 + h2 + k * h2 + k


def forward(L, x, params, h1, h2, k):
    """q float32 [..., K] of rows x [..., 224]"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    params = np.ascontiguousarray(params, dtype=np.float32)
    lead = x.shape[:-1]
    x = x.reshape(-1, DIM)
    q = np.zeros((x.shape[0], k), dtype=np.float32)
    L.mnet_forward(x.shape[0], x.ctypes.data, params.ctypes.data, h1, h2, k, q.ctypes.data)
    return q.reshape(lead + (k,))


def argmax(L, q):
    q = np.ascontiguousarray(q, dtype=np.float32)
    lead, k = q.shape[:-1], q.shape[-1]
    q2 = q.reshape(-1, k)
    out = np.zeros(q2.shape[0], dtype=np.int32)
    L.mnet_argmax(q2.shape[0], q2.ctypes.data, k, out.ctypes.data)
    return out.reshape(lead)


def threshold(L, eps):
    return int(L.mnet_threshold(float(eps)))


def draws(seed, gid, tick, slots):
    """(x, y) words of the exploration block per (match, slot): counter = the match's tick, stream ST_NET, block = slot"""
    gid = np.asarray(gid, dtype=np.uint64)[:, None]
    tick = (np.asarray(tick).astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)[:, None]
    slots = np.asarray(slots, dtype=np.uint64)[None, :]
    shape = np.broadcast_shapes(gid.shape, slots.shape)
    w = Q.philox(np.broadcast_to(gid & np.uint64(0xFFFFFFFF), shape), np.broadcast_to(gid >> np.uint64(32), shape),
                 np.broadcast_to(tick, shape), np.broadcast_to((np.uint64(ST_NET) << np.uint64(16)) | slots, shape),
                 seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return w[0], w[1]


def indices(L, rows, params, h1, h2, k, eps, seed, gid, tick, slots):
    """the index each slot in `slots` chooses: rows [N, len(slots), 224] -> int32 [N, len(slots)]"""
    greedy = argmax(L, forward(L, rows, params, h1, h2, k))
    wx, wy = draws(seed, gid, tick, slots)
    explore = wx.astype(np.uint64) < np.uint64(threshold(L, eps))
    rnd = ((wy.astype(np.uint64) * np.uint64(k)) >> np.uint64(32)).astype(np.int32)
    return np.where(explore, rnd, greedy).astype(np.int32)
