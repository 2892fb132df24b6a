"""ctypes binding of tests/see_policy_ref.c (the host restatement of the see policy's forward pass: input width as an argument,
relu or tanh_spec) and what each see-policy slot does: the categorical head and the slot's ST_NET block are tests/match_policy.py's
library, rows and vision state tests/match_see.py's.  TEST INFRASTRUCTURE: compiled on demand with -ffp-contract=off (the fp32
contract)."""
import ctypes as C
import os
import subprocess

import numpy as np

import match_policy as MP

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'see_policy_ref.c')
DIM = 192


def build(outdir):
    """(this module's library, match_policy's)"""
    so = os.path.join(str(outdir), 'libsee_policy_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC, '-lm'], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    L.spol_forward.restype = None
    L.spol_forward.argtypes = [C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return L, MP.build(outdir)


def param_count(h1, h2, k, dim=DIM):
    return h1 * dim + h1 + h2 * h1 + h2 + k * h2 + k


def forward(L, x, params, h1, h2, k, act, dim=DIM):
    """logits float32 [..., K] of rows x [..., dim]; act 0 relu, 1 tanh"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    params = np.ascontiguousarray(params, dtype=np.float32)
    assert x.shape[-1] == dim and params.size == param_count(h1, h2, k, dim)
    lead = x.shape[:-1]
    x = x.reshape(-1, dim)
    y = np.zeros((x.shape[0], k), dtype=np.float32)
    L.spol_forward(x.shape[0], dim, x.ctypes.data, params.ctypes.data, h1, h2, k, int(act), y.ctypes.data)
    return y.reshape(lead + (k,))


def actions(libs, rows, params, h1, h2, k, act, det, seed, gid, tick, slots):
    """what each see-policy slot in `slots` does: see rows [N, len(slots), 192] -> (index int32, logp float32, logits float32
    [.., K]), the first two [N, len(slots)]  (libs: what build() returned)"""
    L, PL = libs
    y = forward(L, rows, params, h1, h2, k, act)
    gid = np.asarray(gid, dtype=np.uint64)[:, None]
    tick = np.asarray(tick)[:, None]
    idx, lp = MP.head(PL, y, seed, gid, tick, np.asarray(slots, dtype=np.uint32)[None, :], det)
    return idx, lp, y
