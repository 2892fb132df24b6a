"""ctypes binding of tests/replay_ref.c (the host restatement of s2d_replay_push / s2d_replay_sample) and the helpers the
replay tests share: a NumPy ring, synthetic records and the examples' torch formulation of a 1-step push.  TEST INFRASTRUCTURE:
compiled on demand with -ffp-contract=off (the fp32 contract)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'replay_ref.c')
RING_FIELDS = ('obs', 'next_obs', 'action', 'reward', 'discount')
BATCH_FIELDS = RING_FIELDS + ('index',)


def build(outdir):
    so = os.path.join(str(outdir), 'libreplay_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC, '-lm'], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    V = C.c_void_p
    L.replay_push.restype = None
    L.replay_push.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_float, V, V, V, V, V, V, V, C.c_int64, V, V, V, V, V, V]
    L.replay_index.restype = C.c_int32
    L.replay_index.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
    L.replay_sample.restype = None
    L.replay_sample.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_int64, V, V, V, V, V, V, C.c_uint64, V, V, V, V, V, V]
    return L


def words(a):
    """a 4-byte array as contiguous uint32 words (a view where possible)"""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4, a.dtype
    return a.view(np.uint32)


class Ring:
    """the caller-owned ring as NumPy words; fill: the sentinel word every array starts with"""

    def __init__(self, capacity, D, AW, fill=0):
        self.capacity, self.D, self.AW = capacity, D, AW
        self.obs = np.full((capacity, D), fill, np.uint32)
        self.next_obs = np.full((capacity, D), fill, np.uint32)
        self.action = np.full((capacity, AW), fill, np.uint32)
        self.reward = np.full((capacity,), fill, np.uint32).view(np.float32)
        self.discount = np.full((capacity,), fill, np.uint32).view(np.float32)
        self.cursor = np.zeros(4, np.uint64)

    def arrays(self):
        return {k: getattr(self, k) for k in RING_FIELDS}


def push(L, ring, rec, first_obs, n_step, gamma):
    """replay_push of a record of NumPy arrays ('obs', 'terminal_obs' [T,N,D]; 'action' [T,N] or [T,N,AW]; 'reward', 'done' and
    optionally 'result' [T,N]) into ring"""
    T, N = rec['reward'].shape
    obs, term, first, act = words(rec['obs']), words(rec['terminal_obs']), words(first_obs), words(rec['action'])
    assert obs.shape == (T, N, ring.D) and term.shape == obs.shape and first.shape == (N, ring.D) and act.size == T * N * ring.AW
    rew = np.ascontiguousarray(rec['reward'], np.float32)
    done = np.ascontiguousarray(rec['done'], np.uint8)
    res = None if rec.get('result') is None else np.ascontiguousarray(rec['result'], np.uint8)
    L.replay_push(T, N, ring.D, ring.AW, int(n_step), float(gamma), first.ctypes.data, obs.ctypes.data, term.ctypes.data,
                  act.ctypes.data, rew.ctypes.data, done.ctypes.data, None if res is None else res.ctypes.data, ring.capacity,
                  ring.obs.ctypes.data, ring.next_obs.ctypes.data, ring.action.ctypes.data, ring.reward.ctypes.data,
                  ring.discount.ctypes.data, ring.cursor.ctypes.data)


def sample(L, ring, B, seed):
    """replay_sample: the batch as a dict of word arrays (reward / discount float32, index int32)"""
    out = {'obs': np.full((B, ring.D), 0xDEADBEEF, np.uint32), 'next_obs': np.full((B, ring.D), 0xDEADBEEF, np.uint32),
           'action': np.full((B, ring.AW), 0xDEADBEEF, np.uint32), 'reward': np.full(B, np.nan, np.float32),
           'discount': np.full(B, np.nan, np.float32), 'index': np.full(B, -7, np.int32)}
    L.replay_sample(B, ring.D, ring.AW, ring.capacity, ring.obs.ctypes.data, ring.next_obs.ctypes.data, ring.action.ctypes.data,
                    ring.reward.ctypes.data, ring.discount.ctypes.data, ring.cursor.ctypes.data, int(seed), out['obs'].ctypes.data,
                    out['next_obs'].ctypes.data, out['action'].ctypes.data, out['reward'].ctypes.data, out['discount'].ctypes.data,
                    out['index'].ctypes.data)
    return out


def synthetic_record(rng, T, N, D, AW, float_action=False, done_rate=0.2, with_result=True):
    """(rec, first_obs): random words everywhere a kernel may read, dones at done_rate carrying one of the three results (None
    elsewhere), terminal_obs distinct from obs"""
    rec = {'obs': rng.standard_normal((T, N, D)).astype(np.float32),
           'terminal_obs': rng.standard_normal((T, N, D)).astype(np.float32),
           'reward': rng.standard_normal((T, N)).astype(np.float32),
           'done': (rng.random((T, N)) < done_rate).astype(np.uint8)}
    if float_action:
        rec['action'] = rng.uniform(-1, 1, (T, N, AW)).astype(np.float32)
    else:
        rec['action'] = rng.integers(0, 16, (T, N) if AW == 1 else (T, N, AW)).astype(np.int32)
    if with_result:
        rec['result'] = (rec['done'] * rng.integers(1, 4, (T, N))).astype(np.uint8)
    first_obs = rng.standard_normal((N, D)).astype(np.float32)
    return rec, first_obs


def torch_formulation(rec, first_obs, gamma):
    """The 1-step transitions as the examples' learn_fused built them before DeviceReplay (cat / where / gamma * (1 - term)), on
    torch tensors of any device: (obs_t, action, reward, next_obs, discount), flattened to T * N rows."""
    import torch
    obs = rec['obs']
    obs_t = torch.cat([first_obs[None], obs[:-1]])             # action t was chosen from the observation of step t - 1
    done = rec['done'].bool()
    next_obs = torch.where(done.unsqueeze(-1), rec['terminal_obs'], obs)        # bootstrap through Timeouts
    term = ((rec['result'] == 1) | (rec['result'] == 2)).float()              # Goal / Out are true terminations
    d = obs.shape[-1]
    T, N = rec['reward'].shape
    return (obs_t.reshape(-1, d), rec['action'].reshape(T * N, -1), rec['reward'].reshape(-1), next_obs.reshape(-1, d),
            (gamma * (1 - term)).reshape(-1))
