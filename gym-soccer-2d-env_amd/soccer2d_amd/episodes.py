"""EpisodeStats: episode returns, lengths and results of [T, N] rollout records, kept on the device (s2d_episode_stats in
include/s2d.h): what SB3's Monitor / ep_info_buffer and the reference's InfoCollectorCallback report, without a per-step host
loop.  An episode usually spans several records, so the object owns every env's running return and length and carries them from
one ``update`` to the next; finished episodes land in a ring of ``capacity`` episodes in the order a per-step loop over the envs
would have met them, and exact integer totals count everything since ``reset()``.  Engine-independent: any time-major record
(reach-ball, GoToCenter, 11v11 with agents flattened into N) on one device."""
import ctypes as C

import numpy as np
import torch

from . import _capi

RESULT_NAMES = ('Goal', 'Out', 'Timeout')                  # S2D_RESULT_GOAL / OUT / TIMEOUT = 1 / 2 / 3
RING_FIELDS = ('return', 'length', 'result', 'env', 'step')


def _arr(name, t, dtype, shape, device):
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or t.device != device or not t.is_contiguous():
        raise ValueError(f'EpisodeStats: {name} must be a contiguous {dtype} tensor of shape {shape} on {device}')
    return C.c_void_p(t.data_ptr())


def new_window(seen, episodes, capacity):
    """(first, count) of the episodes numbered seen .. episodes - 1, which live in slots (first + j) mod capacity; RuntimeError
    if the ring of `capacity` no longer holds all of them (host arithmetic, shared with the tests' NumPy twin)"""
    new = episodes - seen
    if new > capacity:
        raise RuntimeError(f'EpisodeStats: {new} episodes finished since the last new_result_codes() but the ring keeps '
                           f'{capacity}, so {new - capacity} of them were dropped or overwritten: use a larger capacity (or '
                           f'call it after fewer updates)')
    return seen, new


class EpisodeStats:
    """``EpisodeStats(num_envs, capacity=100)``: the default capacity is the length of SB3's ``ep_info_buffer``, so
    ``summary()['ep_rew_mean']`` means what SB3 logs.  ``update`` only queues kernels; ``episodes``, ``summary`` and
    ``new_result_codes`` read the cursor, which synchronises, and are not for use inside a graph capture."""

    def __init__(self, num_envs, capacity=100, device='cuda:0'):
        if int(num_envs) < 1 or not 1 <= int(capacity) < 2 ** 31:
            raise ValueError('EpisodeStats: num_envs must be >= 1 and capacity in [1, 2^31 - 1]')
        self.num_envs, self.capacity, self.device = int(num_envs), int(capacity), torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError('EpisodeStats: device must be a GPU')
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=self.device)
        self.acc_return, self.acc_length = z(self.num_envs, torch.float32), z(self.num_envs, torch.int32)
        self.ring = {'return': z(self.capacity, torch.float32), 'length': z(self.capacity, torch.int32),
                     'result': z(self.capacity, torch.uint8), 'env': z(self.capacity, torch.int32),
                     'step': z(self.capacity, torch.int64)}
        self.totals = z(8, torch.int64)                      # the uint64[8] of the C contract
        self._workspaces = {}
        self._seen = 0                                       # totals[0] at the last new_result_codes()
        self._lib = _capi.load_library()
        self._ring = _capi.S2DEpisodeRing(*(self.ring[k].data_ptr() for k in RING_FIELDS), self.capacity)

    def workspace(self, T, N):
        """the scratch of a (T, N) call, allocated on first use (so: call update once before capturing it)"""
        ws = self._workspaces.get((T, N))
        if ws is None:
            nbytes = self._lib.s2d_episode_stats_workspace(T, N)
            if nbytes == 0:
                raise ValueError(f'EpisodeStats: no workspace for T = {T}, N = {N} (T, N >= 1, N < 2^31, T * N < 2^40)')
            ws = self._workspaces[(T, N)] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return ws

    def update(self, reward, done, result=None):
        """Fold one record in: done uint8 [T, N]; reward float32 [T, N] or None (every return is 0); result uint8 [T, N] or None
        (every episode counts as unlabelled).  Stream-ordered on torch's current stream, capturable; returns self."""
        if not torch.is_tensor(done) or done.dim() != 2:
            raise ValueError('EpisodeStats: done must be a [T, N] tensor')
        T, N = done.shape
        if T < 1 or N != self.num_envs:
            raise ValueError(f'EpisodeStats: done must be [T >= 1, {self.num_envs}], got {tuple(done.shape)}')
        dev, shape = self.device, (T, N)
        p_done = _arr('done', done, torch.uint8, shape, dev)
        p_reward = None if reward is None else _arr('reward', reward, torch.float32, shape, dev)
        p_result = None if result is None else _arr('result', result, torch.uint8, shape, dev)
        ws = self.workspace(T, N)
        with torch.cuda.device(dev):
            rc = self._lib.s2d_episode_stats(T, N, p_reward, p_done, p_result, C.c_void_p(self.acc_return.data_ptr()),
                                             C.c_void_p(self.acc_length.data_ptr()), C.byref(self._ring),
                                             C.c_void_p(self.totals.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                                             C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        _capi.check(self._lib, rc, 's2d_episode_stats')
        return self

    def update_record(self, rec):
        """update() from a rollout dict: 'done', and 'reward' / 'result' where the record has them"""
        return self.update(rec.get('reward'), rec['done'], rec.get('result'))

    def reset(self):
        """forget everything: carries and totals to zero (the ring's old entries become unreachable)"""
        self.acc_return.zero_()
        self.acc_length.zero_()
        self.totals.zero_()
        self._seen = 0

    def _window(self, first, count):
        idx = (torch.arange(count, dtype=torch.int64, device=self.device) + first) % self.capacity
        return {k: self.ring[k][idx] for k in RING_FIELDS}

    def episodes(self):
        """The last min(episodes, capacity) finished episodes, oldest first: a dict of device tensors 'return', 'length',
        'result', 'env', 'step' (the vector step, counted from reset(), at which the episode ended).  Reads the cursor once (a
        synchronisation): not for use inside a capture."""
        e = int(self.totals[0])
        m = min(e, self.capacity)
        return self._window(e - m, m)

    def summary(self):
        """{'episodes', 'steps', 'ep_rew_mean', 'ep_len_mean' (over the kept window, SB3's meaning; nan with no episode yet),
        'Goal', 'Out', 'Timeout' (shares of all episodes since reset()), 'unlabelled', 'dropped' (counts since reset()),
        'window' (episodes in the kept window) and 'window_goal' (the Goal share over it)}"""
        t = self.totals.cpu().tolist()
        e, m = t[0], min(t[0], self.capacity)
        win = self._window(e - m, m)
        n = max(1, e)
        out = {'episodes': e, 'steps': t[1],
               'ep_rew_mean': float(win['return'].mean()) if m else float('nan'),
               'ep_len_mean': float(win['length'].float().mean()) if m else float('nan')}
        out.update({name: t[3 + j] / n for j, name in enumerate(RESULT_NAMES)})
        out.update(unlabelled=t[2], dropped=t[7], window=m,
                   window_goal=float((win['result'] == 1).float().mean()) if m else float('nan'))
        return out

    def new_result_codes(self):
        """The results of the episodes finished since the previous call, oldest first, as a host uint8 array: one byte per
        episode crosses to the host.  RuntimeError if the ring no longer holds all of them."""
        e = int(self.totals[0])
        seen, self._seen = self._seen, e
        first, new = new_window(seen, e, self.capacity)
        if new == 0:
            return np.zeros(0, np.uint8)
        idx = (torch.arange(new, dtype=torch.int64, device=self.device) + first) % self.capacity
        return self.ring['result'][idx].cpu().numpy()
