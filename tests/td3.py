"""ctypes binding of tests/td3_ref.c (the host restatement of s2d_td_target_td3: the DDPG / twin target with target-policy
smoothing, its z stream, the clipped noise and the clamped action) and what the TD3 tests share.  The networks are tests/td.py's
Net objects (NumPy parameter vectors in nn.Sequential order).  TEST INFRASTRUCTURE: compiled on demand with -ffp-contract=off (the
fp32 contract)."""
import ctypes as C
import os
import subprocess

import numpy as np

import td as TD

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'td3_ref.c')
F = np.float32


def build(outdir):
    so = os.path.join(str(outdir), 'libtd3_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-I', HERE, '-I', os.path.join(ROOT, 'include'), '-o', so, SRC,
                    '-lm'], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    V, N = C.c_void_p, C.POINTER(TD.TdNet)
    L.td3_z.restype, L.td3_z.argtypes = None, [C.c_int64, C.c_int64, C.c_int, C.c_uint64, C.c_uint64, V]
    L.td3_smooth.restype, L.td3_smooth.argtypes = C.c_float, [C.c_float, C.c_float, C.c_float, C.c_float]
    L.td3_smooth_n.restype, L.td3_smooth_n.argtypes = None, [C.c_int64, V, C.c_float, C.c_float, V, V]
    L.td3_target.restype = None
    L.td3_target.argtypes = [C.c_int64, N, N, N, V, V, V, C.c_float, C.c_float, C.c_uint64, C.c_uint64, V, V, V, V]
    L.td_target_ac.restype, L.td_target_ac.argtypes = None, [C.c_int64, N, N, N, V, V, V, V, V, V]
    L.td_forward.restype, L.td_forward.argtypes = None, [C.c_int64, N, V, V]
    return L


def _f32(a):
    return np.ascontiguousarray(a, dtype=F)


def blocks(L):
    """Philox blocks the restatement has drawn so far"""
    return C.c_uint64.in_dll(L, 'td3_blocks').value


def z(L, n, A, seed, draws, row0=0):
    """z [n][A] of global rows row0 .. row0 + n - 1 at call `draws`"""
    out = np.zeros((n, A), F)
    L.td3_z(n, int(row0), A, int(seed), int(draws), out.ctypes.data)
    return out


def smooth(L, m, sigma, clip, zz):
    """clamp(m + clamp(sigma z, -clip, clip), -1, 1) word by word, in the kernel's operation order"""
    m, zz = _f32(m), _f32(zz)
    assert m.shape == zz.shape
    out = np.zeros_like(m)
    L.td3_smooth_n(m.size, m.ctypes.data, float(F(sigma)), float(F(clip)), zz.ctypes.data, out.ctypes.data)
    return out


def target(L, actor, critic1, critic2, next_obs, reward, discount, sigma, clip, draws, seed):
    """(target [B], q [B], action [B][A], mean [B][A]) of s2d_td_target_td3 at call `draws`; mean: the unsmoothed action"""
    x, r, d = _f32(next_obs), _f32(reward), _f32(discount)
    B, A = x.shape[0], actor.n_out
    assert x.shape == (B, actor.n_in) and critic1.n_in == actor.n_in + A and critic1.n_out == 1
    t, q, a, m = np.zeros(B, F), np.zeros(B, F), np.zeros((B, A), F), np.zeros((B, A), F)
    ca, c1, c2 = actor.c(), critic1.c(), (critic2.c() if critic2 is not None else None)
    L.td3_target(B, C.byref(ca), C.byref(c1), C.byref(c2) if c2 is not None else None, x.ctypes.data, r.ctypes.data, d.ctypes.data,
                 float(F(sigma)), float(F(clip)), int(draws), int(seed), t.ctypes.data, q.ctypes.data, a.ctypes.data, m.ctypes.data)
    return t, q, a, m


bits = TD.bits
