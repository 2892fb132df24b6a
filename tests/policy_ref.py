"""ctypes binding of tests/policy_ref.c (the host restatement of the fused stochastic policy: forward pass with either
activation, categorical and Gaussian heads, logp, the deterministic switch, gae).  TEST INFRASTRUCTURE: compiled on demand with
-ffp-contract=off (the fp32 contract)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'policy_ref.c')
MODES = {'discrete': 0, 'cont1': 1, 'turn4': 2}


def build(outdir):
    so = os.path.join(str(outdir), 'libpolicy_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-I', HERE, '-o', so, SRC, '-lm'], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    V = C.c_void_p
    L.policy_forward.restype = None
    L.policy_forward.argtypes = [C.c_int64, V, V, C.c_int, C.c_int, C.c_int, C.c_int, V]
    L.policy_categorical.restype = None
    L.policy_categorical.argtypes = [C.c_int64, C.c_int, V, V, C.c_int, V, V]
    L.policy_head.restype = None
    L.policy_head.argtypes = [C.c_int, C.c_int, C.c_int64, V, V, V, V, C.c_uint64, C.c_int, V, V]
    L.policy_actions.restype = None
    L.policy_actions.argtypes = [C.c_int64, V, V, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, V, C.c_int, C.c_uint64, C.c_uint64,
                                 V, V, V, V, V]
    L.policy_gae.restype = None
    L.policy_gae.argtypes = [C.c_int, C.c_int64, V, V, V, V, V, V, C.c_float, C.c_float, V, V]
    return L


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _u32(k):
    return np.ascontiguousarray(np.asarray(k, dtype=np.int64) & 0xFFFFFFFF, dtype=np.uint32)


def forward(L, x, params, h1, h2, na, act):
    """y [n][na]; act 0 relu / 1 tanh"""
    x, params = _f32(x), _f32(params)
    y = np.zeros((x.shape[0], na), dtype=np.float32)
    L.policy_forward(x.shape[0], x.ctypes.data, params.ctypes.data, h1, h2, na, int(act), y.ctypes.data)
    return y


def categorical(L, y, w, det=0):
    """(action int32 [n], logp [n]) of logit rows y [n][A] with the uniform words w (uint32 [n])"""
    y = _f32(y)
    n, A = y.shape
    w = np.ascontiguousarray(np.broadcast_to(np.asarray(w, dtype=np.uint32), (n,)))
    a, lp = np.zeros(n, np.int32), np.zeros(n, np.float32)
    L.policy_categorical(n, A, y.ctypes.data, w.ctypes.data, int(det), a.ctypes.data, lp.ctypes.data)
    return a, lp


def head(L, mode, y, log_std, gid, k, seed, det=0):
    """the head alone: (action, logp); action int32 [n] (discrete) or float32 [n][A]"""
    y = _f32(y)
    n, na = y.shape
    m = MODES[mode]
    ls = _f32(np.zeros(na) if log_std is None else log_std)
    gid = np.ascontiguousarray(np.broadcast_to(np.asarray(gid, dtype=np.uint64), (n,)))
    k = np.ascontiguousarray(np.broadcast_to(_u32(k), (n,)))
    a = np.zeros(n, np.int32) if m == 0 else np.zeros((n, na), np.float32)
    lp = np.zeros(n, np.float32)
    L.policy_head(m, na, n, y.ctypes.data, ls.ctypes.data, gid.ctypes.data, k.ctypes.data, int(seed), int(det), a.ctypes.data,
                  lp.ctypes.data)
    return a, lp


def actions(L, obs, params, h1, h2, na, act, mode, log_std, det, seed, k, gid0=0):
    """(action, logp) per env at policy steps k"""
    obs, params = _f32(obs), _f32(params)
    n, m = obs.shape[0], MODES[mode]
    ls = _f32(np.zeros(na) if log_std is None else log_std)
    k = np.ascontiguousarray(np.broadcast_to(_u32(k), (n,)))
    y = np.zeros((n, na), np.float32)
    gid = np.zeros(n, np.uint64)
    a = np.zeros(n, np.int32) if m == 0 else np.zeros((n, na), np.float32)
    lp = np.zeros(n, np.float32)
    L.policy_actions(n, obs.ctypes.data, params.ctypes.data, h1, h2, na, int(act), m, ls.ctypes.data, int(det), int(seed), int(gid0),
                     k.ctypes.data, y.ctypes.data, gid.ctypes.data, a.ctypes.data, lp.ctypes.data)
    return a, lp


def gae(L, reward, done, value, last_value, gamma, lam, result=None, terminal_value=None):
    reward, value, last_value = _f32(reward), _f32(value), _f32(last_value)
    done = np.ascontiguousarray(done, dtype=np.uint8)
    T, N = reward.shape
    res = None if result is None else np.ascontiguousarray(result, dtype=np.uint8)
    tv = None if terminal_value is None else _f32(terminal_value)
    adv, ret = np.zeros((T, N), np.float32), np.zeros((T, N), np.float32)
    L.policy_gae(T, N, reward.ctypes.data, done.ctypes.data, value.ctypes.data, last_value.ctypes.data,
                 None if res is None else res.ctypes.data, None if tv is None else tv.ctypes.data, float(gamma), float(lam),
                 adv.ctypes.data, ret.ctypes.data)
    return adv, ret
