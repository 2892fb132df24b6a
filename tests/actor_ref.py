"""ctypes binding of tests/actor_ref.c (the host restatement of the fused tanh actor: forward pass, tanh_spec, log_spec,
Box-Muller, clip, exploration).  TEST INFRASTRUCTURE: compiled on demand with -ffp-contract=off (the fp32 contract, DESIGN.md
section 4)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'actor_ref.c')


def build(outdir):
    so = os.path.join(str(outdir), 'libactor_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC, '-lm'], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    L.actor_forward.restype = None
    L.actor_forward.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    for f in ('actor_tanh', 'actor_log'):
        getattr(L, f).restype = None
        getattr(L, f).argtypes = [C.c_int64, C.c_void_p, C.c_void_p]
    L.actor_gauss.restype = None
    L.actor_gauss.argtypes = [C.c_int64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.actor_actions.restype = None
    L.actor_actions.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p,
                                C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def forward(L, x, params, h1, h2, na):
    x, params = _f32(x), _f32(params)
    y = np.zeros((x.shape[0], na), dtype=np.float32)
    L.actor_forward(x.shape[0], x.ctypes.data, params.ctypes.data, h1, h2, na, y.ctypes.data)
    return y


def tanh(L, v):
    v = _f32(v).reshape(-1)
    out = np.empty_like(v)
    L.actor_tanh(v.size, v.ctypes.data, out.ctypes.data)
    return out


def log(L, v):
    v = _f32(v).reshape(-1)
    out = np.empty_like(v)
    L.actor_log(v.size, v.ctypes.data, out.ctypes.data)
    return out


def gauss(L, seed, gid, ctr):
    """z0..z3 [n][4] of the Gaussian block (POLICY block 3) at counters ctr of envs gid"""
    gid = np.ascontiguousarray(gid, dtype=np.uint64)
    ctr = np.ascontiguousarray(np.broadcast_to(ctr, gid.shape), dtype=np.uint32)
    z = np.zeros((gid.size, 4), dtype=np.float32)
    L.actor_gauss(gid.size, int(seed), gid.ctypes.data, ctr.ctypes.data, z.ctypes.data)
    return z


def actions(L, obs, params, h1, h2, na, eps, kind, noise, seed, k, gid0=0):
    """the actor's action [n][na] per env at policy steps k (int array)"""
    obs, params = _f32(obs), _f32(params)
    n = obs.shape[0]
    noise = _f32(np.zeros((2, na)) if noise is None else noise)
    k = np.ascontiguousarray(np.asarray(k) & 0xFFFFFFFF, dtype=np.uint32)
    y = np.zeros((n, na), dtype=np.float32)
    out = np.zeros((n, na), dtype=np.float32)
    L.actor_actions(n, obs.ctypes.data, params.ctypes.data, h1, h2, na, float(eps), int(kind), noise.ctypes.data, int(seed),
                    int(gid0), k.ctypes.data, y.ctypes.data, out.ctypes.data)
    return out
