"""QLearner: one gradient step of the online Q-network in HIP (s2d_learn_q / s2d_learn_q_grad in include/s2d.h), the step that
follows QTarget.target in DQN, Double DQN, n-step and prioritized replay:

    q = q_net(obs)[action];  e = q - target;  loss = mean(weight * huber(e))      (or e^2 / 2)
    backward;  clip_grad_norm_(max_grad_norm);  Adam.step()

instead of torch's chain of forward, gather, smooth_l1_loss, backward, clip_grad_norm_ and Adam.step.  The network is the MLP of
the wide actors and of td.QTarget on a narrower grid (input width 1 .. 256, 1 .. 4 hidden layers of multiples of 8 in [8, 256],
1 .. 64 outputs, ReLU, Tanh or Sigmoid) on the project's fp32 spec: the forward value is, bit for bit, what the fused actor acts
on and the target launch bootstraps from, and the gradient is a function of the batch alone (fixed blocks of rows, fixed order, no
float atomics), equal to tests/learn_ref.c.

The learner owns ONE flat fp32 parameter buffer and REBINDS THE MODULE'S PARAMETERS AS VIEWS OF IT: the module always holds the
learner's weights, so ``actor.sync()``, ``QTarget.sync()`` and ``state_dict()`` keep working unchanged.  Learning rate, betas,
epsilon, the clip norm and Adam's running beta products are device words read when the kernels run: a step is a linear chain on
torch's current stream, capturable, and ``set_lr`` between replays takes effect.  Out of scope: the DDPG / TD3 update (the
actor's gradient through the critic)."""
import ctypes as C

import torch

from . import _capi
from .actor import _read_layers
from .mlp_actor import param_count
from .td import _arr, _fill_shape, _net_text
from .wide_actor import _WideShape

MAX_IN = 256
MAX_OUT = 64
MAX_HIDDEN = 4
MAX_WIDTH = 256
BLOCK_ROWS = 64      # S2D_LEARN_BLOCK_ROWS
NORM_CHUNK = 256     # S2D_LEARN_NORM_CHUNK
LDS_BYTES = 160 * 1024
LOSSES = ('mse', 'huber')


def _round64(w):
    return (w + 63) // 64 * 64


def learn_param_count(n_in, hidden, n_out):
    return param_count(hidden, n_out, n_in)


def learn_workspace_bytes(n_in, hidden, n_out, max_batch):
    """bytes of the learner's workspace, by the arithmetic of the C layout (s2d_learn_workspace_bytes): the blocks' partial
    gradients, the chunk sums of the norm, the blocks' loss partials and, where 64 rows of activations do not fit the LDS, the
    blocks' activations; every part rounded up to 64 words"""
    P = learn_param_count(n_in, hidden, n_out)
    blocks, chunks = (max_batch + BLOCK_ROWS - 1) // BLOCK_ROWS, (P + NORM_CHUNK - 1) // NORM_CHUNK
    pitch = ((n_in + 3) // 4 * 4 + sum(hidden) + n_out) | 1
    words = _round64(blocks * P) + _round64(chunks) + _round64(blocks)
    if BLOCK_ROWS * (pitch + 1) * 4 > LDS_BYTES:
        words += _round64(blocks * BLOCK_ROWS * pitch)
    return words * 4


class QLearner:
    """The online Q-network's optimiser step in one call.  ``q_net`` is Linear-(F-Linear) x L (SB3's ``q_net.q_net``)."""

    def __init__(self, q_net, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=10.0, loss='huber', max_batch=4096, device=None):
        who = 'QLearner'
        if not isinstance(q_net, torch.nn.Module):
            raise ValueError(f'{who}: the Q-network must be a torch.nn.Module')
        try:
            linears, act = _read_layers(q_net, **_WideShape._grid)
        except ValueError as e:
            raise ValueError(f'{who}: Q-network: {e}') from None
        if any(lin.bias is None for lin in linears):
            raise ValueError(f'{who}: every nn.Linear of the Q-network needs a bias')
        if any(p.dtype != torch.float32 for lin in linears for p in (lin.weight, lin.bias)):
            raise ValueError(f'{who}: the Q-network\'s parameters must be float32')
        self.hidden = tuple(lin.out_features for lin in linears[:-1])
        self.n_in, self.n_out, self.activation = linears[0].in_features, linears[-1].out_features, act
        if not 1 <= len(self.hidden) <= MAX_HIDDEN:
            raise ValueError(f'{who}: the learner takes 1 to {MAX_HIDDEN} hidden layers, got {len(self.hidden)}')
        for w in self.hidden:
            if w % 8 or not 8 <= w <= MAX_WIDTH:
                raise ValueError(f'{who}: every hidden width must be a multiple of 8 in [8, {MAX_WIDTH}], got {w} in {list(self.hidden)}')
        if not 1 <= self.n_in <= MAX_IN:
            raise ValueError(f'{who}: the Q-network\'s input width must be in [1, {MAX_IN}], got {self.n_in}')
        if not 1 <= self.n_out <= MAX_OUT:
            raise ValueError(f'{who}: the Q-network\'s output width must be in [1, {MAX_OUT}], got {self.n_out}')
        if loss not in LOSSES:
            raise ValueError(f"{who}: loss must be 'huber' or 'mse', got {loss!r}")
        if not isinstance(max_batch, int) or not 1 <= max_batch < 2 ** 31:
            raise ValueError(f'{who}: max_batch must be an int in [1, 2^31 - 1], got {max_batch!r}')
        b1, b2 = (float(b) for b in betas)
        if not (lr >= 0.0 and 0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and eps >= 0.0):
            raise ValueError(f'{who}: lr and eps must be >= 0 and the betas in [0, 1), got lr={lr}, betas={betas}, eps={eps}')
        self.module, self.loss_kind, self.max_batch = q_net, LOSSES.index(loss), max_batch
        dev = torch.device(device if device is not None else linears[0].weight.device)
        f32 = torch.float32
        P = learn_param_count(self.n_in, self.hidden, self.n_out)
        # torch's device allocations are 256-byte aligned (the ABI asks for 16 of the [P] arrays, 256 of the workspace)
        self.params = torch.zeros(P, dtype=f32, device=dev)
        self.device = self.params.device                                     # with its index: 'cuda' -> cuda:0
        self.m, self.v, self._grad = (torch.zeros(P, dtype=f32, device=self.device) for _ in range(3))
        self.hyper = torch.tensor([lr, b1, b2, eps, max_grad_norm, 1.0, 1.0], dtype=f32).to(self.device)
        self.stats = torch.zeros(3, dtype=f32, device=self.device)
        self.error = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.workspace = torch.zeros(learn_workspace_bytes(self.n_in, self.hidden, self.n_out, max_batch) // 4, dtype=f32, device=self.device)
        # the module's parameters become views of the flat buffer (nn.Sequential order): the module IS the learner's weights
        off = 0
        with torch.no_grad():
            for lin in linears:
                for p in (lin.weight, lin.bias):
                    n = p.numel()
                    self.params[off:off + n].copy_(p.detach().reshape(-1))
                    p.data = self.params[off:off + n].view_as(p)
                    off += n
        self._mirror = None

    @classmethod
    def from_module(cls, q_net, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=10.0, loss='huber', max_batch=4096, device=None):
        """A learner of `q_net` with torch.optim.Adam's and clip_grad_norm_'s arguments (max_grad_norm <= 0: no clip), the loss
        ('huber': smooth_l1_loss with beta 1; 'mse': e^2 / 2) and the largest batch a step will see (it sizes the workspace).
        device: where the buffers, and from then on the module's parameters, live (default: the module's)."""
        return cls(q_net, lr=lr, betas=betas, eps=eps, max_grad_norm=max_grad_norm, loss=loss, max_batch=max_batch, device=device)

    text = _net_text

    # ------------------------------------------------------------------ the step
    def _arr(self, who, name, t, dtype, shape):
        return _arr(who, self.device, name, t, dtype, shape)

    def _call(self, fn, batch, target, weight, td_abs_out, q_out):
        who = f'QLearner.{"step" if fn == "s2d_learn_q" else "grad"}'
        if not isinstance(batch, dict) or any(k not in batch for k in ('obs', 'action')):
            raise ValueError(f"{who}: batch must be a dict with 'obs' and 'action' (DeviceReplay.sample's)")
        obs, action = batch['obs'], batch['action']
        if not torch.is_tensor(obs) or obs.dim() != 2 or obs.shape[0] < 1:
            raise ValueError(f"{who}: batch['obs'] must be a [B, {self.n_in}] tensor, B >= 1")
        B, f32 = obs.shape[0], torch.float32
        if B > self.max_batch:
            raise ValueError(f'{who}: the batch has {B} rows, the learner was made with max_batch={self.max_batch}')
        if torch.is_tensor(action) and tuple(action.shape) == (B, 1):
            action = action.view(B) if action.is_contiguous() else action
        ptrs = [self._arr(who, "batch['obs']", obs, f32, (B, self.n_in)),
                self._arr(who, "batch['action'] ([B] or [B, 1])", action, torch.int32, (B,)),
                self._arr(who, 'target', target, f32, (B,)),
                self._arr(who, 'weight', weight, f32, (B,)) if weight is not None else None,
                self._arr(who, 'td_abs_out', td_abs_out, f32, (B,)) if td_abs_out is not None else None,
                self._arr(who, 'q_out', q_out, f32, (B, self.n_out)) if q_out is not None else None]
        if self.device.type != 'cuda':
            raise ValueError(f'{who}: the networks are on {self.device}; the kernels need a GPU (there is no CPU path)')
        lib = _capi.load_library()
        net, st = self.c_structs()
        with torch.cuda.device(self.device):
            rc = getattr(lib, fn)(B, C.byref(net), C.byref(st), *ptrs, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        _capi.check(lib, rc, fn)

    def c_structs(self):
        net, st = _fill_shape(_capi.S2DLearnNet(), self), _capi.S2DLearnState()
        net.params, net.workspace, net.workspace_bytes = self.params.data_ptr(), self.workspace.data_ptr(), self.workspace.numel() * 4
        st.m, st.v, st.grad = self.m.data_ptr(), self.v.data_ptr(), self._grad.data_ptr()
        st.hyper, st.stats, st.error, st.loss_kind = self.hyper.data_ptr(), self.stats.data_ptr(), self.error.data_ptr(), self.loss_kind
        return net, st

    def step(self, batch, target, weight=None, td_abs_out=None, q_out=None):
        """One update on the dict DeviceReplay.sample / PrioritizedReplay.sample returns (its 'obs' [B, obs_dim] and 'action' int32
        [B] or [B, 1]) towards `target` float32 [B] (QTarget.target's), with the importance weights `weight` [B] where given.
        td_abs_out [B] <- |q - target| (the new priorities' base), q_out [B, A] <- the forward values.  Stream-ordered on torch's
        current stream, capturable; returns nothing: read ``loss`` / ``grad_norm`` / ``clip_scale`` when they are wanted."""
        self._call('s2d_learn_q', batch, target, weight, td_abs_out, q_out)

    def grad(self, batch, target, weight=None, td_abs_out=None, q_out=None):
        """The flat, unclipped gradient [P] (a view, written again by the next call) of the same loss, with ``loss`` /
        ``grad_norm`` / ``clip_scale`` set, without touching the parameters or the optimiser's state."""
        self._call('s2d_learn_q_grad', batch, target, weight, td_abs_out, q_out)
        return self._grad

    # ------------------------------------------------------------------ state
    def _stat(self, i):
        host = self.stats.tolist()                                           # synchronises
        if int(self.error.item()):
            self.error.zero_()
            raise ValueError(f'QLearner: a batch held an action outside [0, {self.n_out}): its rows were left out of the update')
        return host[i]

    @property
    def loss(self):
        """the last call's mean loss (synchronises; raises ValueError if a batch since the last look held a bad action)"""
        return self._stat(0)

    @property
    def grad_norm(self):
        """the last call's gradient norm before the clip (synchronises)"""
        return self._stat(1)

    @property
    def clip_scale(self):
        """the factor the last call's gradient was scaled by: min(1, max_grad_norm / (norm + 1e-6)) (synchronises)"""
        return self._stat(2)

    def set_lr(self, lr):
        """the learning rate of the steps enqueued from now on: a device write, also between the replays of a captured graph"""
        self.hyper[0:1].fill_(float(lr))

    def reset_optimizer(self):
        """Adam as new: m = v = 0, both beta products 1"""
        self.m.zero_()
        self.v.zero_()
        self.hyper[5:7].fill_(1.0)

    def update_target(self, q_target, tau=1.0):
        """The learner's weights into a td.QTarget's target network: a hard copy (tau = 1) or a Polyak step target += tau (online
        - target), one ``copy_`` or ``lerp_`` from the learner's flat buffer straight into the target's (the layouts are the
        same); one more flat copy keeps the target MODULE equal, whose parameters become views of a mirror buffer."""
        from .td import QTarget
        if not isinstance(q_target, QTarget):
            raise ValueError('QLearner.update_target: q_target must be a td.QTarget')
        net = q_target.q_target
        if (net.n_in, net.hidden, net.n_out) != (self.n_in, self.hidden, self.n_out) or net.device != self.device:
            raise ValueError(f'QLearner.update_target: the target network is {net.text()} on {net.device}, the learner\'s '
                             f'{self.text()} on {self.device}')
        if not 0.0 <= tau <= 1.0:
            raise ValueError(f'QLearner.update_target: tau must be in [0, 1], got {tau}')
        with torch.no_grad():
            if tau == 1.0:
                net.params.copy_(self.params)
            else:
                net.params.lerp_(self.params, float(tau))
            if self._mirror is None or self._mirror[0] is not net:
                linears, _ = _read_layers(net.module, **_WideShape._grid)
                mirror, off = torch.empty_like(net.params), 0
                for lin in linears:
                    for p in (lin.weight, lin.bias):
                        p.data = mirror[off:off + p.numel()].view_as(p)
                        off += p.numel()
                self._mirror = (net, mirror)
            self._mirror[1].copy_(net.params)


__all__ = ['QLearner', 'learn_workspace_bytes', 'learn_param_count']
