"""DeviceReplay: the off-policy learners' replay buffer on the device (s2d_replay_push / s2d_replay_sample in include/s2d.h), the
counterpart of gae() for DQN and DDPG.  One launch turns a whole [T, N] rollout record into n-step transitions with SB3's
time-limit handling (``ReplayBuffer.add`` with ``handle_timeout_termination``), one launch samples a batch
(``ReplayBuffer.sample``), instead of a chain of cat / where / reshape / index-scatter ops and five gathers.  Both read the cursor
from device memory when the kernel runs, so collect -> push -> sample can sit in one captured graph.  Engine-independent: any
record with the [T, N] layout (reach-ball, GoToCenter, 11v11 with agents flattened into N) on one device."""
import ctypes as C
import math

import torch

from . import _capi

FIELDS = ('obs', 'next_obs', 'action', 'reward', 'discount', 'index')


def _is_int(x):
    return isinstance(x, int) and not isinstance(x, bool)


class DeviceReplay:
    """A ring of `capacity` transitions (obs, action, reward, next_obs, discount); the learner's target is
    ``reward + discount * bootstrap(next_obs)``: reward is the n-step return, discount is gamma^k, or 0 where the episode
    terminated within the horizon (a Timeout keeps gamma^k and bootstraps from the terminal observation).

    obs_dim in [1, 1024] float32 words per observation; action_words in [1, 8] words of action_dtype (torch.int32 or
    torch.float32) per action.  seed keys the sample indices (Philox stream S2D_REPLAY_STREAM, counter = the number of sample()
    calls so far): the same seed and the same calls give the same batches."""

    def __init__(self, capacity, obs_dim, action_words=1, action_dtype=torch.int32, device='cuda:0', n_step=1, gamma=0.99, seed=0):
        if not _is_int(capacity) or not 1 <= capacity < 2 ** 31:
            raise ValueError('DeviceReplay: capacity must be an int in [1, 2^31 - 1]')
        if not _is_int(obs_dim) or not 1 <= obs_dim <= 1024:
            raise ValueError('DeviceReplay: obs_dim must be an int in [1, 1024]')
        if not _is_int(action_words) or not 1 <= action_words <= 8:
            raise ValueError('DeviceReplay: action_words must be an int in [1, 8]')
        if action_dtype not in (torch.int32, torch.float32):
            raise ValueError('DeviceReplay: action_dtype must be torch.int32 or torch.float32')
        if not _is_int(n_step) or n_step < 1 or n_step >= 2 ** 31:
            raise ValueError('DeviceReplay: n_step must be an int in [1, 2^31 - 1]')
        if not isinstance(gamma, (int, float)) or not math.isfinite(gamma):
            raise ValueError('DeviceReplay: gamma must be a finite number')
        if not _is_int(seed) or not 0 <= seed < 2 ** 64:
            raise ValueError('DeviceReplay: seed must be an int in [0, 2^64 - 1]')
        self.capacity, self.obs_dim, self.action_words, self.action_dtype = capacity, obs_dim, action_words, action_dtype
        self.n_step, self.gamma, self.seed = n_step, float(gamma), seed
        dev, f32 = torch.device(device), torch.float32
        self.obs = torch.zeros((capacity, obs_dim), dtype=f32, device=dev)
        self.device = dev = self.obs.device                                  # with its index: 'cuda' -> cuda:0
        self.next_obs = torch.zeros((capacity, obs_dim), dtype=f32, device=dev)
        self.action = torch.zeros((capacity, action_words), dtype=action_dtype, device=dev)
        self.reward = torch.zeros((capacity,), dtype=f32, device=dev)
        self.discount = torch.zeros((capacity,), dtype=f32, device=dev)
        self.cursor = torch.zeros((4,), dtype=torch.int64, device=dev)      # {pos, size, pushes, samples}, read by the kernels
        self._ring = _capi.S2DReplayRing(capacity, self.obs.data_ptr(), self.next_obs.data_ptr(), self.action.data_ptr(),
                                         self.reward.data_ptr(), self.discount.data_ptr())

    # ---- checks -----------------------------------------------------------------------------------------------------------
    def _arr(self, what, name, t, dtype, shape):
        if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or t.device != self.device or not t.is_contiguous():
            raise ValueError(f'DeviceReplay.{what}: {name} must be a contiguous {dtype} tensor of shape {shape} on {self.device}')
        return C.c_void_p(t.data_ptr())

    def _library(self, what):
        if self.device.type != 'cuda':
            raise ValueError(f'DeviceReplay.{what}: the buffer is on {self.device}; the kernels need a GPU (there is no CPU path)')
        return _capi.load_library()

    # ---- the two launches ---------------------------------------------------------------------------------------------------
    def push(self, rec, first_obs):
        """Append the T x N transitions of a rollout record (the dict Engine.rollout_qnet / rollout_actor /
        GoToCenterVecEnv.rollout_* return with terminal_obs=True: 'obs' [T,N,D], 'terminal_obs' [T,N,D], 'action' [T,N] or
        [T,N,A], 'reward', 'done' and optionally 'result' [T,N]); first_obs [N,D] is the observation action 0 was chosen from
        (a copy taken before the rollout).  Without 'result' every done is a termination.  T * N must not exceed the capacity.
        Stream-ordered on torch's current stream, capturable."""
        T, N, ptrs = self._record(rec, first_obs)
        self._push(T, N, ptrs)

    def _record(self, rec, first_obs):
        """push()'s argument checks: (T, N, the seven record pointers)"""
        if not isinstance(rec, dict):
            raise ValueError('DeviceReplay.push: rec must be a rollout record dict')
        for k in ('obs', 'terminal_obs', 'action', 'reward', 'done'):
            if k not in rec:
                raise ValueError(f"DeviceReplay.push: the record has no '{k}'" +
                                 (' (collect with terminal_obs=True)' if k == 'terminal_obs' else ''))
        reward = rec['reward']
        if not torch.is_tensor(reward) or reward.dim() != 2:
            raise ValueError("DeviceReplay.push: rec['reward'] must be a [T, N] tensor")
        T, N = reward.shape
        if T < 1 or N < 1:
            raise ValueError('DeviceReplay.push: T and N must be >= 1')
        if T * N > self.capacity:
            raise ValueError(f'DeviceReplay.push: the record holds {T} x {N} transitions, more than the capacity {self.capacity}')
        D, A = self.obs_dim, self.action_words
        act = rec['action']
        a_shape = (T, N) if A == 1 and torch.is_tensor(act) and act.dim() == 2 else (T, N, A)
        ptrs = [self._arr('push', 'first_obs', first_obs, torch.float32, (N, D)),
                self._arr('push', "rec['obs']", rec['obs'], torch.float32, (T, N, D)),
                self._arr('push', "rec['terminal_obs']", rec['terminal_obs'], torch.float32, (T, N, D)),
                self._arr('push', "rec['action']", act, self.action_dtype, a_shape),
                self._arr('push', "rec['reward']", reward, torch.float32, (T, N)),
                self._arr('push', "rec['done']", rec['done'], torch.uint8, (T, N)),
                None if rec.get('result') is None else self._arr('push', "rec['result']", rec['result'], torch.uint8, (T, N))]
        return T, N, ptrs

    def _push(self, T, N, ptrs):
        lib = self._library('push')
        with torch.cuda.device(self.device):
            rc = lib.s2d_replay_push(T, N, self.obs_dim, self.action_words, self.n_step, self.gamma, *ptrs, C.byref(self._ring),
                                     C.c_void_p(self.cursor.data_ptr()),
                                     C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        _capi.check(lib, rc, 's2d_replay_push')

    def alloc_batch(self, batch):
        """the dict sample() fills: 'obs' / 'next_obs' [B,D], 'action' [B,A], 'reward' / 'discount' [B], 'index' int32 [B]"""
        if not _is_int(batch) or not 1 <= batch < 2 ** 31:
            raise ValueError('DeviceReplay.sample: batch must be an int in [1, 2^31 - 1]')
        f32, dev = torch.float32, self.device
        return {'obs': torch.empty((batch, self.obs_dim), dtype=f32, device=dev),
                'next_obs': torch.empty((batch, self.obs_dim), dtype=f32, device=dev),
                'action': torch.empty((batch, self.action_words), dtype=self.action_dtype, device=dev),
                'reward': torch.empty((batch,), dtype=f32, device=dev), 'discount': torch.empty((batch,), dtype=f32, device=dev),
                'index': torch.empty((batch,), dtype=torch.int32, device=dev)}

    def sample(self, batch, out=None):
        """A uniform batch with replacement: the dict of alloc_batch() ('index' = the slots drawn; -1 and zero rows while the
        buffer is empty).  out: a dict from an earlier call, written again (a captured graph replays into it).  Stream-ordered
        on torch's current stream, capturable; each call advances the sample counter on the device."""
        if out is None:
            out = self.alloc_batch(batch)
        elif not _is_int(batch) or not 1 <= batch < 2 ** 31:
            raise ValueError('DeviceReplay.sample: batch must be an int in [1, 2^31 - 1]')
        elif not isinstance(out, dict) or any(k not in out for k in FIELDS):
            raise ValueError(f'DeviceReplay.sample: out must be a dict with {FIELDS}')
        B, D, A, f32 = batch, self.obs_dim, self.action_words, torch.float32
        ptrs = [self._arr('sample', "out['obs']", out['obs'], f32, (B, D)), self._arr('sample', "out['next_obs']", out['next_obs'], f32, (B, D)),
                self._arr('sample', "out['action']", out['action'], self.action_dtype, (B, A)),
                self._arr('sample', "out['reward']", out['reward'], f32, (B,)), self._arr('sample', "out['discount']", out['discount'], f32, (B,)),
                self._arr('sample', "out['index']", out['index'], torch.int32, (B,))]
        lib = self._library('sample')
        with torch.cuda.device(self.device):
            rc = lib.s2d_replay_sample(B, D, A, C.byref(self._ring), C.c_void_p(self.cursor.data_ptr()), self.seed, *ptrs,
                                       C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        _capi.check(lib, rc, 's2d_replay_sample')
        return out

    # ---- the cursor -------------------------------------------------------------------------------------------------------
    @property
    def pos(self):
        """the slot the next push starts at (synchronises: reads the device cursor)"""
        return int(self.cursor[0].item())

    @property
    def size(self):
        """transitions held, at most the capacity (synchronises: reads the device cursor)"""
        return int(self.cursor[1].item())

    def clear(self):
        """empty the buffer and restart the push and sample counters (stream-ordered; the ring's contents stay as they are)"""
        self.cursor.zero_()


PRIO_FIELDS = FIELDS + ('priority', 'total')


class PrioritizedReplay(DeviceReplay):
    """DeviceReplay with proportional prioritized sampling (Schaul et al., 2016) on a device sum tree
    (s2d_replay_prio_push / s2d_replay_sample_prio / s2d_replay_prio_update in include/s2d.h).  Same constructor; capacity at most
    2^30.  The tree stores priorities exactly as handed over: apply alpha before update_priorities() and beta in weights().  New
    transitions enter with the largest priority stored so far (1.0 on a fresh buffer).  seed keys the stratified draws (Philox
    stream S2D_REPLAY_PRIO_STREAM, counter = the number of sample() calls so far).  Sampling resolves 2^-24 of the total mass."""

    def __init__(self, capacity, *args, **kw):
        if not _is_int(capacity) or not 1 <= capacity <= 2 ** 30:
            raise ValueError('PrioritizedReplay: capacity must be an int in [1, 2^30]')
        super().__init__(capacity, *args, **kw)
        self.leaves = 1 << (capacity - 1).bit_length()                   # P; s2d_replay_tree_words(capacity) = 2 * P
        self.tree = torch.zeros((2 * self.leaves,), dtype=torch.float32, device=self.device)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def push(self, rec, first_obs):
        """DeviceReplay.push, behind a launch that gives the T * N slots it is about to write the largest priority stored so far"""
        T, N, ptrs = self._record(rec, first_obs)
        lib = self._library('push')
        with torch.cuda.device(self.device):
            rc = lib.s2d_replay_prio_push(T * N, self.capacity, C.c_void_p(self.tree.data_ptr()), C.c_void_p(self.cursor.data_ptr()),
                                          self._stream())
        _capi.check(lib, rc, 's2d_replay_prio_push')
        self._push(T, N, ptrs)

    def alloc_batch(self, batch):
        """DeviceReplay.alloc_batch plus 'priority' float32 [B] (the leaf each element was drawn from) and 'total' float32 [1]"""
        if not _is_int(batch) or not 1 <= batch <= 2 ** 24:
            raise ValueError('PrioritizedReplay.sample: batch must be an int in [1, 2^24]')
        out = super().alloc_batch(batch)
        out['priority'] = torch.empty((batch,), dtype=torch.float32, device=self.device)
        out['total'] = torch.empty((1,), dtype=torch.float32, device=self.device)
        return out

    def sample(self, batch, out=None):
        """A batch drawn in proportion to priority, one stratified draw per B-th of the total mass: the dict of alloc_batch()
        (index -1, zero rows, priority and total 0 while the buffer is empty).  out, stream order and capture as for
        DeviceReplay.sample."""
        if out is None:
            out = self.alloc_batch(batch)
        elif not _is_int(batch) or not 1 <= batch <= 2 ** 24:
            raise ValueError('PrioritizedReplay.sample: batch must be an int in [1, 2^24]')
        elif not isinstance(out, dict) or any(k not in out for k in PRIO_FIELDS):
            raise ValueError(f'PrioritizedReplay.sample: out must be a dict with {PRIO_FIELDS}')
        B, D, A, f32 = batch, self.obs_dim, self.action_words, torch.float32
        ptrs = [self._arr('sample', "out['obs']", out['obs'], f32, (B, D)), self._arr('sample', "out['next_obs']", out['next_obs'], f32, (B, D)),
                self._arr('sample', "out['action']", out['action'], self.action_dtype, (B, A)),
                self._arr('sample', "out['reward']", out['reward'], f32, (B,)), self._arr('sample', "out['discount']", out['discount'], f32, (B,)),
                self._arr('sample', "out['index']", out['index'], torch.int32, (B,)),
                self._arr('sample', "out['priority']", out['priority'], f32, (B,)), self._arr('sample', "out['total']", out['total'], f32, (1,))]
        lib = self._library('sample')
        with torch.cuda.device(self.device):
            rc = lib.s2d_replay_sample_prio(B, D, A, C.byref(self._ring), C.c_void_p(self.tree.data_ptr()),
                                            C.c_void_p(self.cursor.data_ptr()), self.seed, *ptrs, self._stream())
        _capi.check(lib, rc, 's2d_replay_sample_prio')
        return out

    def update_priorities(self, index, priority):
        """Store priority[b] (float32 [B], alpha already applied) as the new priority of slot index[b] (int32 [B], a batch's
        'index'); entries outside [0, size) are ignored, of duplicates the largest wins, values are clamped to [2^-40, 2^40] (NaN
        and anything <= 0 become 2^-40).  Stream-ordered on torch's current stream, capturable."""
        if not torch.is_tensor(index) or index.dim() != 1 or not 1 <= index.numel() <= 2 ** 24:
            raise ValueError('PrioritizedReplay.update_priorities: index must be an int32 tensor of shape [B], B in [1, 2^24]')
        B = index.numel()
        ptrs = [self._arr('update_priorities', 'index', index, torch.int32, (B,)),
                self._arr('update_priorities', 'priority', priority, torch.float32, (B,))]
        lib = self._library('update_priorities')
        with torch.cuda.device(self.device):
            rc = lib.s2d_replay_prio_update(B, self.capacity, C.c_void_p(self.tree.data_ptr()), C.c_void_p(self.cursor.data_ptr()), *ptrs,
                                            self._stream())
        _capi.check(lib, rc, 's2d_replay_prio_update')

    def weights(self, batch, beta):
        """The importance weights of a sampled batch, float32 [B]: (size * priority / total) ** -beta divided by the batch's
        largest weight; 0 where index is -1.  Pure torch on the buffer's device, no synchronisation."""
        if not isinstance(beta, (int, float)) or isinstance(beta, bool) or not math.isfinite(beta) or beta < 0:
            raise ValueError('PrioritizedReplay.weights: beta must be a finite number >= 0')
        if not isinstance(batch, dict) or any(k not in batch for k in ('index', 'priority', 'total')):
            raise ValueError("PrioritizedReplay.weights: batch must be a dict with 'index', 'priority' and 'total'")
        size = self.cursor[1].clamp(max=self.capacity).to(torch.float32)
        valid = batch['index'] >= 0
        w = torch.where(valid, (size * batch['priority'] / batch['total']) ** -float(beta), torch.zeros_like(batch['priority']))
        return w / w.max().clamp_min(torch.finfo(torch.float32).tiny)

    @property
    def total(self):
        """the sum of all priorities, tree[1] (synchronises)"""
        return float(self.tree[1].item())

    @property
    def max_priority(self):
        """the priority the next push hands out: the largest ever stored, 1.0 before the first update (synchronises)"""
        top = float(self.tree[0].item())
        return top if top >= 2.0 ** -40 else 1.0

    def clear(self):
        """DeviceReplay.clear, and the tree back to its empty state (all zero)"""
        super().clear()
        self.tree.zero_()
