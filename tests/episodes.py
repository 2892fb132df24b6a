"""ctypes binding of tests/episodes_ref.c (the host restatement of s2d_episode_stats) and what the episode tests share: a NumPy
twin of EpisodeStats' state, an independent per-env "Monitor" loop and a synthetic-record generator.  TEST INFRASTRUCTURE:
compiled on demand with -ffp-contract=off (the fp32 contract)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'episodes_ref.c')
RING_FIELDS = ('return', 'length', 'result', 'env', 'step')
RING_DTYPES = (np.float32, np.int32, np.uint8, np.int32, np.int64)


def build(outdir):
    so = os.path.join(str(outdir), 'libepisodes_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    V = C.c_void_p
    L.episode_stats.restype = None
    L.episode_stats.argtypes = [C.c_int, C.c_int64, V, V, V, V, V, C.c_int64, V, V, V, V, V, V]
    return L


def sentinel(shape, dtype, byte=0xA5):
    """an array whose every byte is `byte`"""
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, byte, np.uint8).view(dtype).reshape(shape)


class HostStats:
    """NumPy twin of EpisodeStats, advanced by the C restatement; `fill`: the byte every ring array starts from"""

    def __init__(self, L, num_envs, capacity, fill=0):
        self.L, self.num_envs, self.capacity = L, num_envs, capacity
        self.acc_return = np.zeros(num_envs, np.float32)
        self.acc_length = np.zeros(num_envs, np.int32)
        self.ring = {k: sentinel((capacity,), dt, fill) for k, dt in zip(RING_FIELDS, RING_DTYPES)}
        self.totals = np.zeros(8, np.uint64)
        self._seen = 0

    def update(self, reward, done, result=None):
        done = np.ascontiguousarray(done, np.uint8)
        T, N = done.shape
        assert N == self.num_envs
        reward = None if reward is None else np.ascontiguousarray(reward, np.float32)
        result = None if result is None else np.ascontiguousarray(result, np.uint8)
        p = lambda a: None if a is None else a.ctypes.data
        self.L.episode_stats(T, N, p(reward), p(done), p(result), p(self.acc_return), p(self.acc_length), self.capacity,
                             *(p(self.ring[k]) for k in RING_FIELDS), p(self.totals))
        return self

    def episodes(self):
        e = int(self.totals[0])
        m = min(e, self.capacity)
        idx = (e - m + np.arange(m)) % self.capacity
        return {k: self.ring[k][idx] for k in RING_FIELDS}

    def new_result_codes(self):
        """EpisodeStats.new_result_codes on the twin: the product's own window arithmetic (and its RuntimeError)"""
        from soccer2d_amd.episodes import new_window
        e = int(self.totals[0])
        seen, self._seen = self._seen, e
        first, new = new_window(seen, e, self.capacity)
        return self.ring['result'][(first + np.arange(new)) % self.capacity].astype(np.uint8)


def monitor(records, num_envs, acc_return=None, acc_length=None, s0=0):
    """Independent restatement: every env accumulates on its own, as a gym Monitor wrapper would (a float32 running return,
    a length), over the chained records; the finished episodes are then merged by (step, env).  Returns (list of
    (return, length, result, env, step), acc_return, acc_length)."""
    ret = np.zeros(num_envs, np.float32) if acc_return is None else acc_return.copy()
    length = np.zeros(num_envs, np.int64) if acc_length is None else acc_length.astype(np.int64)
    eps = []
    for i in range(num_envs):
        step = s0
        for reward, done, result in records:
            for t in range(done.shape[0]):
                ret[i] = np.float32(ret[i] + (np.float32(0) if reward is None else reward[t, i]))
                length[i] += 1
                if done[t, i]:
                    eps.append((ret[i].copy(), int(length[i]), 0 if result is None else int(result[t, i]), i, step))
                    ret[i], length[i] = np.float32(0), 0
                step += 1
    eps.sort(key=lambda e: (e[4], e[3]))
    return eps, ret, length


def synthetic_record(rng, T, N, done_rate=0.2, with_result=True, with_reward=True, junk=True):
    """(reward, done, result): rewards with awkward bits (mixed magnitudes and signs, so the add's order and rounding show),
    dones at done_rate (every non-zero byte counts as set), results 1..3 where done and, with junk, RANDOM BYTES elsewhere (the
    contract uses result only where done is set; junk=False: zero elsewhere, as an engine writes it)"""
    done = (rng.random((T, N)) < done_rate)
    done = np.where(done, rng.integers(1, 256, (T, N)), 0).astype(np.uint8)
    reward = result = None
    if with_reward:
        reward = (rng.standard_normal((T, N)) * 10.0 ** rng.integers(-3, 4, (T, N))).astype(np.float32)
    if with_result:
        label = rng.integers(1, 4, (T, N))
        if junk:                                             # one episode in ten carries 0 or a code past Timeout
            label = np.where(rng.random((T, N)) < 0.1, rng.choice([0, 4, 9, 255], (T, N)), label)
        result = np.where(done != 0, label, rng.integers(0, 256, (T, N)) if junk else 0).astype(np.uint8)
    return reward, done, result


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a
