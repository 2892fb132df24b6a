"""ctypes binding of tests/qnet_ref.c (the host restatement of the fused actor's forward pass, argmax and epsilon threshold)
and a numpy restatement of its exploration draws.  TEST INFRASTRUCTURE: compiled on demand with -ffp-contract=off (the fp32
contract)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'qnet_ref.c')
ST_POLICY = 1


def build(outdir):
    so = os.path.join(str(outdir), 'libqnet_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC, '-lm'], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    L.qnet_forward.restype = None
    L.qnet_forward.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.qnet_argmax.restype = None
    L.qnet_argmax.argtypes = [C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
    L.qnet_greedy.restype = None
    L.qnet_greedy.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.qnet_threshold.restype = C.c_uint64
    L.qnet_threshold.argtypes = [C.c_float]
    return L


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def forward(L, x, params, h1, h2, na):
    x, params = _f32(x), _f32(params)
    n = x.shape[0]
    q = np.zeros((n, na), dtype=np.float32)
    L.qnet_forward(n, x.ctypes.data, params.ctypes.data, h1, h2, na, q.ctypes.data)
    return q


def argmax(L, q):
    q = _f32(q)
    out = np.zeros(q.shape[0], dtype=np.int32)
    L.qnet_argmax(q.shape[0], q.ctypes.data, q.shape[1], out.ctypes.data)
    return out


def greedy(L, x, params, h1, h2, na):
    return argmax(L, forward(L, x, params, h1, h2, na))


def threshold(L, eps):
    return int(L.qnet_threshold(float(eps)))


# ---- Philox4x32-10, vectorised over envs (checked against the oracle's exported philox in test_qnet_actor_host.py)
def philox(c0, c1, c2, c3, k0, k1):
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for v in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = M0 * c[0]
        p1 = M1 * c[2]
        n0 = (p1 >> np.uint64(32)) ^ c[1] ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c[3] ^ k1
        c = [n0 & mask, p1 & mask, n2 & mask, p0 & mask]
        k0 = (k0 + np.uint64(0x9E3779B9)) & mask
        k1 = (k1 + np.uint64(0xBB67AE85)) & mask
    return [v.astype(np.uint32) for v in c]


def policy_word(seed, gid, k, block):
    """word k & 3 of Philox block `block` of stream POLICY at counter k >> 2, per env (gid, k: int arrays; k is the uint32
    policy counter, taken modulo 2^32, so the engine's int32 view and k0 + t past 2^32 both give the device's counter)"""
    gid = np.asarray(gid, dtype=np.uint64)
    k = (np.asarray(k).astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)
    ctr = np.broadcast_to(k >> np.uint64(2), gid.shape)
    w = philox(gid & np.uint64(0xFFFFFFFF), gid >> np.uint64(32), ctr, np.full(gid.shape, (ST_POLICY << 16) | block, np.uint64),
               seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    j = np.broadcast_to(k & np.uint64(3), gid.shape).astype(np.int64)
    return np.choose(j, w)


def actions(L, obs, params, h1, h2, na, eps, seed, gid, k):
    """the actor's action per env: explore (block 2 word < thr) -> S2D_ACT_RANDOM's draw (block 0), else the greedy action"""
    g = greedy(L, obs, params, h1, h2, na)
    thr = threshold(L, eps)
    explore = policy_word(seed, gid, k, 2).astype(np.uint64) < np.uint64(thr)
    rnd = ((policy_word(seed, gid, k, 0).astype(np.uint64) * np.uint64(na)) >> np.uint64(32)).astype(np.int32)
    return np.where(explore, rnd, g).astype(np.int32)
