"""ctypes binding of tests/match_policy_ref.c: the host restatement of the 11v11 policy slots (forward pass with relu or
tanh_spec, the categorical head on word z of the slot's ST_NET block, logp, the deterministic switch).  TEST INFRASTRUCTURE:
compiled on demand with -ffp-contract=off (the fp32 contract)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'match_policy_ref.c')
DIM = 224


def build(outdir):
    so = os.path.join(str(outdir), 'libmatch_policy_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC, '-lm'], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    vp, i64, ci = C.c_void_p, C.c_int64, C.c_int
    L.mpol_forward.restype = None
    L.mpol_forward.argtypes = [i64, vp, vp, ci, ci, ci, ci, vp]
    L.mnet_forward.restype = None
    L.mnet_forward.argtypes = [i64, vp, vp, ci, ci, ci, vp]
    L.mpol_block.restype = None
    L.mpol_block.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, vp]
    L.mpol_head_words.restype = None
    L.mpol_head_words.argtypes = [i64, ci, vp, vp, ci, vp, vp]
    L.mpol_head.restype = None
    L.mpol_head.argtypes = [i64, ci, vp, C.c_uint64, vp, vp, vp, ci, vp, vp]
    L.mpol_tanh.restype = None
    L.mpol_tanh.argtypes = [i64, vp, vp]
    return L


def param_count(h1, h2, k):
    return h1 * DIM + h1 + h2 * h1 + h2 + k * h2 + k


def forward(L, x, params, h1, h2, k, act):
    """logits float32 [..., K] of rows x [..., 224]; act 0 relu, 1 tanh"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    params = np.ascontiguousarray(params, dtype=np.float32)
    assert params.size == param_count(h1, h2, k)
    lead = x.shape[:-1]
    x = x.reshape(-1, DIM)
    y = np.zeros((x.shape[0], k), dtype=np.float32)
    L.mpol_forward(x.shape[0], x.ctypes.data, params.ctypes.data, h1, h2, k, int(act), y.ctypes.data)
    return y.reshape(lead + (k,))


def block(L, seed, gid, tick, slot):
    w = np.zeros(4, dtype=np.uint32)
    L.mpol_block(int(seed) & (2**64 - 1), int(gid), int(tick) & 0xFFFFFFFF, int(slot), w.ctypes.data)
    return w


def head_words(L, y, w, det):
    """(index int32 [n], logp float32 [n]) of logits y [n, K] with the blocks w uint32 [n, 4] (word z is used)"""
    y = np.ascontiguousarray(y, dtype=np.float32)
    w = np.ascontiguousarray(w, dtype=np.uint32)
    n, k = y.shape
    assert w.shape == (n, 4)
    idx, lp = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float32)
    L.mpol_head_words(n, k, y.ctypes.data, w.ctypes.data, int(bool(det)), idx.ctypes.data, lp.ctypes.data)
    return idx, lp


def head(L, y, seed, gid, tick, slot, det):
    """(index, logp) of logits y [..., K]; gid, tick, slot broadcast to y's leading shape"""
    y = np.ascontiguousarray(y, dtype=np.float32)
    lead, k = y.shape[:-1], y.shape[-1]
    y2 = y.reshape(-1, k)
    n = y2.shape[0]
    g = np.ascontiguousarray(np.broadcast_to(np.asarray(gid, dtype=np.uint64), lead)).reshape(-1)
    t = np.ascontiguousarray(np.broadcast_to((np.asarray(tick).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32), lead)).reshape(-1)
    s = np.ascontiguousarray(np.broadcast_to(np.asarray(slot, dtype=np.uint32), lead)).reshape(-1)
    idx, lp = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float32)
    L.mpol_head(n, k, y2.ctypes.data, int(seed) & (2**64 - 1), g.ctypes.data, t.ctypes.data, s.ctypes.data, int(bool(det)),
                idx.ctypes.data, lp.ctypes.data)
    return idx.reshape(lead), lp.reshape(lead)


def actions(L, rows, params, h1, h2, k, act, det, seed, gid, tick, slots):
    """what each policy slot in `slots` does: rows [N, len(slots), 224] -> (index int32, logp float32) [N, len(slots)]"""
    y = forward(L, rows, params, h1, h2, k, act)
    gid = np.asarray(gid, dtype=np.uint64)[:, None]
    tick = np.asarray(tick)[:, None]
    return head(L, y, seed, gid, tick, np.asarray(slots, dtype=np.uint32)[None, :], det)


def tanh_spec(L, v):
    v = np.ascontiguousarray(v, dtype=np.float32)
    out = np.zeros_like(v)
    L.mpol_tanh(v.size, v.ctypes.data, out.ctypes.data)
    return out
