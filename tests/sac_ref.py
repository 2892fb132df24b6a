"""ctypes binding of tests/sac_ref.c (the host restatement of Soft Actor-Critic's collection and target: the squashed-Gaussian
head, the rollout policy on the streamed-weight MLP with its z layout, the target's z stream, s2d_td_target_sac) and what the SAC
tests share.  The networks are tests/td.py's Net objects (NumPy parameter vectors in nn.Sequential order).  TEST INFRASTRUCTURE:
compiled on demand with -ffp-contract=off (the fp32 contract)."""
import ctypes as C
import os
import subprocess

import numpy as np

import td as TD

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'sac_ref.c')
MODES = {'cont1': 1, 'turn4': 2}
NA = {'cont1': 1, 'turn4': 4}
F = np.float32


def build(outdir):
    so = os.path.join(str(outdir), 'libsac_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-I', HERE, '-I', os.path.join(ROOT, 'include'), '-o', so, SRC,
                    '-lm'], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    V, N = C.c_void_p, C.POINTER(TD.TdNet)
    L.sac_term.restype, L.sac_term.argtypes = C.c_float, [C.c_float, C.c_float, C.c_float, C.c_int, C.POINTER(C.c_float)]
    L.sac_head.restype, L.sac_head.argtypes = None, [C.c_int64, C.c_int, V, V, C.c_int, V, V]
    L.sac_rollout_z.restype, L.sac_rollout_z.argtypes = None, [C.c_int64, C.c_int, C.c_uint64, C.c_uint64, V, V]
    L.sac_actions.restype = None
    L.sac_actions.argtypes = [C.c_int64, V, V, C.c_int, V, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, V, V, V, V, V]
    L.sac_td_z.restype, L.sac_td_z.argtypes = None, [C.c_int64, C.c_int, C.c_uint64, C.c_uint64, V]
    L.sac_target.restype = None
    L.sac_target.argtypes = [C.c_int64, N, N, N, V, V, V, C.c_float, C.c_uint64, C.c_uint64, C.c_int, V, V, V, V]
    L.actor_tanh.restype, L.actor_tanh.argtypes = None, [C.c_int64, V, V]
    L.actor_log.restype, L.actor_log.argtypes = None, [C.c_int64, V, V]
    return L


def _f32(a):
    return np.ascontiguousarray(a, dtype=F)


def _u32(k):
    return np.ascontiguousarray(np.asarray(k, dtype=np.int64) & 0xFFFFFFFF, dtype=np.uint32)


def head(L, y, z, det=0):
    """(action [n][A], logp [n]) of rows y [n][2A] with z [n][A]"""
    y = _f32(y)
    n, A = y.shape[0], y.shape[1] // 2
    z = _f32(np.broadcast_to(np.zeros(1, F) if z is None else z, (n, A)))
    a, lp = np.zeros((n, A), F), np.zeros(n, F)
    L.sac_head(n, A, y.ctypes.data, z.ctypes.data, int(det), a.ctypes.data, lp.ctypes.data)
    return a, lp


def rollout_z(L, mode, n, seed, k, gid0=0):
    """z [n][A] of envs gid0 .. gid0 + n - 1 at policy steps k"""
    k = np.ascontiguousarray(np.broadcast_to(_u32(k), (n,)))
    z = np.zeros((n, NA[mode]), F)
    L.sac_rollout_z(n, MODES[mode], int(seed), int(gid0), k.ctypes.data, z.ctypes.data)
    return z


def actions(L, obs, params, hidden, act, mode, det, seed, k, gid0=0):
    """the rollout policy's (action [n][A], logp [n]) per env at policy steps k; act 'relu' | 'tanh' | 'sigmoid'"""
    obs, params = _f32(obs), _f32(params)
    n, A = obs.shape[0], NA[mode]
    assert params.size == TD.param_count(10, hidden, 2 * A), (params.size, hidden, A)
    h = np.ascontiguousarray(hidden, dtype=np.int32)
    k = np.ascontiguousarray(np.broadcast_to(_u32(k), (n,)))
    y, z, a, lp = np.zeros((n, 2 * A), F), np.zeros((n, A), F), np.zeros((n, A), F), np.zeros(n, F)
    L.sac_actions(n, obs.ctypes.data, params.ctypes.data, len(h), h.ctypes.data, TD.ACT[act], MODES[mode], int(det), int(seed), int(gid0),
                  k.ctypes.data, y.ctypes.data, z.ctypes.data, a.ctypes.data, lp.ctypes.data)
    return a, lp


def td_z(L, n, A, seed, draws):
    z = np.zeros((n, A), F)
    L.sac_td_z(n, A, int(seed), int(draws), z.ctypes.data)
    return z


def target(L, actor, critic1, critic2, next_obs, reward, discount, alpha, draws, seed, det=0):
    """(target [B], q [B], action [B][A], logp [B]) of s2d_td_target_sac at call `draws`"""
    x, r, d = _f32(next_obs), _f32(reward), _f32(discount)
    B, A = x.shape[0], actor.n_out // 2
    assert x.shape == (B, actor.n_in) and critic1.n_in == actor.n_in + A and critic1.n_out == 1
    t, q, a, lp = np.zeros(B, F), np.zeros(B, F), np.zeros((B, A), F), np.zeros(B, F)
    ca, c1, c2 = actor.c(), critic1.c(), (critic2.c() if critic2 is not None else None)
    L.sac_target(B, C.byref(ca), C.byref(c1), C.byref(c2) if c2 is not None else None, x.ctypes.data, r.ctypes.data, d.ctypes.data,
                 float(F(alpha)), int(draws), int(seed), int(det), t.ctypes.data, q.ctypes.data, a.ctypes.data, lp.ctypes.data)
    return t, q, a, lp


def tanh_spec(L, v):
    v = _f32(v)
    out = np.zeros_like(v)
    L.actor_tanh(v.size, v.ctypes.data, out.ctypes.data)
    return out


def log_spec(L, v):
    v = _f32(v)
    out = np.zeros_like(v)
    L.actor_log(v.size, v.ctypes.data, out.ctypes.data)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)
