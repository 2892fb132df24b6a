"""ctypes binding of tests/see_net_ref.c (the host restatement of the see network's forward pass, input width as an argument) and
the index each see-network slot chooses: argmax, threshold and exploration draws are tests/match_net.py's, rows and vision state
tests/match_see.py's.  TEST INFRASTRUCTURE: compiled on demand with -ffp-contract=off (the fp32 contract)."""
import ctypes as C
import os
import subprocess

import numpy as np

import match_net as MN

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'see_net_ref.c')
DIM = 192


def build(outdir):
    so = os.path.join(str(outdir), 'libsee_net_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC, '-lm'], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    L.snet_forward.restype = None
    L.snet_forward.argtypes = [C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return L


def param_count(h1, h2, k, dim=DIM):
    return h1 * dim + h1 + h2 * h1 + h2 + k * h2 + k


def forward(L, x, params, h1, h2, k, dim=DIM):
    """q float32 [..., K] of rows x [..., dim]"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    params = np.ascontiguousarray(params, dtype=np.float32)
    assert x.shape[-1] == dim and params.size == param_count(h1, h2, k, dim)
    lead = x.shape[:-1]
    x = x.reshape(-1, dim)
    q = np.zeros((x.shape[0], k), dtype=np.float32)
    L.snet_forward(x.shape[0], dim, x.ctypes.data, params.ctypes.data, h1, h2, k, q.ctypes.data)
    return q.reshape(lead + (k,))


def indices(L, ML, rows, params, h1, h2, k, eps, seed, gid, tick, slots):
    """the index each slot in `slots` chooses: see rows [N, len(slots), 192] -> int32 [N, len(slots)]  (L: this module's
    library, ML: match_net's)"""
    greedy = MN.argmax(ML, forward(L, rows, params, h1, h2, k))
    wx, wy = MN.draws(seed, gid, tick, slots)
    explore = wx.astype(np.uint64) < np.uint64(MN.threshold(ML, eps))
    rnd = ((wy.astype(np.uint64) * np.uint64(k)) >> np.uint64(32)).astype(np.int32)
    return np.where(explore, rnd, greedy).astype(np.int32)
