"""ctypes binding of tests/replay_prio_ref.c (the host restatement of s2d_replay_prio_push / s2d_replay_prio_update /
s2d_replay_sample_prio) and the helpers the prioritized-replay tests share: a NumPy twin of the sum tree and the priority lists
of the spec.  TEST INFRASTRUCTURE: compiled on demand with -ffp-contract=off (the fp32 contract)."""
import ctypes as C
import os
import subprocess

import numpy as np

import replay as RR

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'replay_prio_ref.c')
PRIO_MIN, PRIO_MAX = np.float32(2.0 ** -40), np.float32(2.0 ** 40)
PRIO_STREAM = 12
BATCH_FIELDS = RR.BATCH_FIELDS + ('priority', 'total')
# what clamp() has to deal with: NaN, a negative, both zeros, a denormal, below MIN, above MAX, +inf, and ordinary values
ODD_PRIORITIES = np.array([np.nan, -1.0, 0.0, -0.0, 1e-42, 2.0 ** -50, 2.0 ** 50, np.inf, 2.0 ** -40, 2.0 ** 40, 1.0, 0.3, 7.5],
                          np.float32)


def build(outdir):
    so = os.path.join(str(outdir), 'libreplay_prio_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC, '-lm'], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    V = C.c_void_p
    L.prio_leaves.restype, L.prio_leaves.argtypes = C.c_int64, [C.c_int64]
    L.prio_clamp.restype, L.prio_clamp.argtypes = C.c_float, [C.c_float]
    L.prio_rebuild.restype, L.prio_rebuild.argtypes = None, [C.c_int64, V]
    L.prio_push.restype, L.prio_push.argtypes = None, [C.c_int64, C.c_int64, V, V]
    L.prio_update.restype, L.prio_update.argtypes = None, [C.c_int64, C.c_int64, V, V, V, V]
    L.prio_mass.restype, L.prio_mass.argtypes = C.c_float, [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_float]
    L.prio_descend.restype, L.prio_descend.argtypes = C.c_int32, [C.c_int64, V, C.c_float]
    L.prio_sample.restype = None
    L.prio_sample.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_int64, V, V, V, V, V, V, V, C.c_uint64, V, V, V, V, V, V, V, V]
    return L


def leaves(capacity):
    P = 1
    while P < capacity:
        P *= 2
    return P


def rebuilt(tree):
    """the NumPy twin: a copy of tree whose internal nodes are summed level by level from its leaves, one fp32 add per node"""
    t = np.array(tree, np.float32)
    P = t.size // 2
    w = P
    while w > 1:
        w //= 2
        t[w:2 * w] = t[2 * w:4 * w:2] + t[2 * w + 1:4 * w:2]
    return t


def random_tree(rng, capacity, size, lo=-40, hi=40, top=None):
    """a consistent tree: `size` leaves 2^U(lo, hi), the rest +0, tree[0] = top (default: the largest leaf)"""
    P = leaves(capacity)
    t = np.zeros(2 * P, np.float32)
    t[P:P + size] = np.exp2(rng.uniform(lo, hi, size)).astype(np.float32).clip(PRIO_MIN, PRIO_MAX)
    t = rebuilt(t)
    t[0] = t[P:].max() if top is None else top
    return t


def push(L, tree, cursor, n, capacity):
    assert tree.dtype == np.float32 and tree.size == 2 * leaves(capacity) and cursor.dtype == np.uint64
    L.prio_push(n, capacity, tree.ctypes.data, cursor.ctypes.data)


def update(L, tree, cursor, index, priority, capacity):
    index, priority = np.ascontiguousarray(index, np.int32), np.ascontiguousarray(priority, np.float32)
    assert tree.dtype == np.float32 and tree.size == 2 * leaves(capacity) and index.shape == priority.shape
    L.prio_update(index.size, capacity, tree.ctypes.data, cursor.ctypes.data, index.ctypes.data, priority.ctypes.data)


def sample(L, ring, tree, B, seed):
    """prio_sample on a replay.Ring: the batch as a dict of word arrays (reward / discount / priority / total float32, index int32)"""
    out = {'obs': np.full((B, ring.D), 0xDEADBEEF, np.uint32), 'next_obs': np.full((B, ring.D), 0xDEADBEEF, np.uint32),
           'action': np.full((B, ring.AW), 0xDEADBEEF, np.uint32), 'reward': np.full(B, np.nan, np.float32),
           'discount': np.full(B, np.nan, np.float32), 'index': np.full(B, -7, np.int32), 'priority': np.full(B, np.nan, np.float32),
           'total': np.full(1, np.nan, np.float32)}
    L.prio_sample(B, ring.D, ring.AW, ring.capacity, ring.obs.ctypes.data, ring.next_obs.ctypes.data, ring.action.ctypes.data,
                  ring.reward.ctypes.data, ring.discount.ctypes.data, tree.ctypes.data, ring.cursor.ctypes.data, int(seed),
                  *(out[k].ctypes.data for k in BATCH_FIELDS))
    return out


def indices(L, tree, capacity, B, seed, samples):
    """the slots one sample call draws, without a ring"""
    total = float(tree[1])
    return np.array([L.prio_descend(capacity, tree.ctypes.data, L.prio_mass(seed, samples, b, B, total)) for b in range(B)], np.int32)
