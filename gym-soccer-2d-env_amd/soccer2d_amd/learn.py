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
torch's current stream, capturable, and ``set_lr`` between replays takes effect.

ActorCriticLearner is the same for DDPG and TD3 (s2d_learn_critic / s2d_learn_actor): the critics' step on [obs | action] and the
actor's step on -mean Q(obs, tanh-mu(obs)), whose gradient goes through the critic inside one kernel; tests/learn_ac_ref.c.

SACLearner is Soft Actor-Critic's (s2d_learn_critic per critic, s2d_learn_sac_actor): the squashed-Gaussian actor's reparameterised
step on mean(alpha * logp - min(Q1, Q2)(obs, a)) through the critic that gave each row's minimum, and the temperature's scalar Adam
step; tests/learn_sac_ref.c.

PPOLearner is the PPO minibatch update (s2d_learn_ppo); tests/learn_ppo_ref.c.  The four share one host path: _Stepped owns the
flat buffers one optimiser steps, _StepNet is one stepped network, _workspace_bytes the one workspace formula and _launch the
one way into the library."""
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
AC_LOSSES = ('mse', 'huber', 'square')   # S2D_LEARN_SQUARE: the critics' steps only
MAX_ACTION = 8
MAX_OBS = 248
PPO_MAX_GROUPS = 256      # S2D_LEARN_PPO_MAX_GROUPS
PPO_HEADS = ('categorical', 'gaussian')


def _round64(w):
    return (w + 63) // 64 * 64


def learn_param_count(n_in, hidden, n_out):
    return param_count(hidden, n_out, n_in)


def _blocks(batch):
    return (batch + BLOCK_ROWS - 1) // BLOCK_ROWS


def _workspace_bytes(P, pitch, row_words, rows, loss_words=1, extras=()):
    """bytes of a learner's workspace, by the arithmetic of the C layout(): `rows` rows of partial gradients of P words, the chunk
    sums of the norm, `loss_words` loss partials per row, the learner's extra parts and, where 64 rows of an image of `pitch` words
    and of the `row_words` beside it do not fit the LDS, the rows' images; every part rounded up to 64 words"""
    words = _round64(rows * P) + _round64((P + NORM_CHUNK - 1) // NORM_CHUNK) + sum(map(_round64, (rows * loss_words, *extras)))
    if BLOCK_ROWS * (pitch + row_words) * 4 > LDS_BYTES:
        words += _round64(rows * BLOCK_ROWS * pitch)
    return words * 4


def learn_workspace_bytes(n_in, hidden, n_out, max_batch):
    """bytes of the learner's workspace, by the arithmetic of the C layout (s2d_learn_workspace_bytes): the blocks' partial
    gradients, the chunk sums of the norm, the blocks' loss partials and, where 64 rows of activations do not fit the LDS, the
    blocks' activations; every part rounded up to 64 words"""
    pitch = ((n_in + 3) // 4 * 4 + sum(hidden) + n_out) | 1
    return _workspace_bytes(learn_param_count(n_in, hidden, n_out), pitch, 1, _blocks(max_batch))


def learn_actor_workspace_bytes(obs_dim, actor_hidden, action_dim, critic_hidden, max_batch):
    """bytes of the ACTOR's workspace for the actor step through a critic (s2d_learn_actor_workspace_bytes): the parts above for the
    actor's parameters, and the blocks' images where 64 rows of BOTH networks ([obs | action] padded to a multiple of 4, every
    layer's outputs of the actor and of the critic) do not fit the LDS"""
    pitch = ((obs_dim + action_dim + 3) // 4 * 4 + sum(actor_hidden) + action_dim + sum(critic_hidden) + 1) | 1
    return _workspace_bytes(learn_param_count(obs_dim, actor_hidden, action_dim), pitch, 1, _blocks(max_batch))


def learn_sac_workspace_bytes(obs_dim, actor_hidden, action_dim, critic1_hidden, critic2_hidden, max_batch):
    """bytes of the ACTOR's workspace for the SAC actor step (s2d_learn_sac_workspace_bytes): learn_actor_workspace_bytes' parts for
    the actor's parameters (D -> ... -> 2A), a second row of block partials (the rows' logp), and the blocks' images where 64 rows of
    ALL the networks ([obs | action] padded to a multiple of 4, every layer's outputs of the actor and of each critic, the head's A
    noise words) and three words a row do not fit the LDS.  critic2_hidden: None for one critic."""
    pitch = ((obs_dim + action_dim + 3) // 4 * 4 + sum(actor_hidden) + 2 * action_dim + sum(critic1_hidden) + 1
             + (sum(critic2_hidden) + 1 if critic2_hidden is not None else 0) + action_dim) | 1
    blocks = _blocks(max_batch)
    return _workspace_bytes(learn_param_count(obs_dim, actor_hidden, 2 * action_dim), pitch, 3, blocks, 1, (blocks,))


def learn_ppo_workspace_bytes(obs_dim, pi_hidden, n_out, vf_hidden, head, max_batch):
    """bytes of the PPO learner's workspace, by the arithmetic of the C layout (s2d_learn_ppo_workspace_bytes): the partial gradients
    and statistics of at most 256 groups of blocks, the chunk sums of the norm, the advantage pre-pass's two words and block sums
    and, where 64 rows of BOTH networks do not fit the LDS, the groups' images; every part rounded up to 64 words.  head: 0 / 1."""
    P = learn_param_count(obs_dim, pi_hidden, n_out) + learn_param_count(obs_dim, vf_hidden, 1) + (n_out if head else 0)
    pitch = ((obs_dim + 3) // 4 * 4 + sum(pi_hidden) + n_out + sum(vf_hidden) + 1 + (n_out if head else 0)) | 1
    blocks = _blocks(max_batch)
    return _workspace_bytes(P, pitch, 6, min(blocks, PPO_MAX_GROUPS), 8, (2, blocks))


def _read_shape(who, what, module, tanh_head=False):
    """(linears, hidden, n_in, n_out, activation) of `module` = Linear-(F-Linear) x L [-Tanh] on the learner's grid"""
    if not isinstance(module, torch.nn.Module):
        raise ValueError(f'{who}: the {what} must be a torch.nn.Module')
    try:
        linears, act = _read_layers(module, **dict(_WideShape._grid, tanh_head=tanh_head))
    except ValueError as e:
        raise ValueError(f'{who}: {what}: {e}') from None
    if any(lin.bias is None for lin in linears):
        raise ValueError(f'{who}: every nn.Linear of the {what} needs a bias')
    if any(p.dtype != torch.float32 for lin in linears for p in (lin.weight, lin.bias)):
        raise ValueError(f'{who}: the {what}\'s parameters must be float32')
    hidden = tuple(lin.out_features for lin in linears[:-1])
    n_in = linears[0].in_features
    if not 1 <= len(hidden) <= MAX_HIDDEN:
        raise ValueError(f'{who}: the learner takes 1 to {MAX_HIDDEN} hidden layers, got {len(hidden)}')
    for w in hidden:
        if w % 8 or not 8 <= w <= MAX_WIDTH:
            raise ValueError(f'{who}: every hidden width must be a multiple of 8 in [8, {MAX_WIDTH}], got {w} in {list(hidden)}')
    if not 1 <= n_in <= MAX_IN:
        raise ValueError(f'{who}: the {what}\'s input width must be in [1, {MAX_IN}], got {n_in}')
    return linears, hidden, n_in, linears[-1].out_features, act


def _check_optimiser(who, max_batch, lr, betas, eps):
    """max_batch and Adam's arguments, checked; returns the betas as floats"""
    if not isinstance(max_batch, int) or not 1 <= max_batch < 2 ** 31:
        raise ValueError(f'{who}: max_batch must be an int in [1, 2^31 - 1], got {max_batch!r}')
    b1, b2 = (float(b) for b in betas)
    if not (lr >= 0.0 and 0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and eps >= 0.0):
        raise ValueError(f'{who}: lr and eps must be >= 0 and the betas in [0, 1), got lr={lr}, betas={betas}, eps={eps}')
    return b1, b2


def _rebind(params, linears):
    """the module's parameters become views of the flat buffer (nn.Sequential order), which takes their values: the module IS the
    learner's weights"""
    off = 0
    with torch.no_grad():
        for lin in linears:
            for p in (lin.weight, lin.bias):
                n = p.numel()
                params[off:off + n].copy_(p.detach().reshape(-1))
                p.data = params[off:off + n].view_as(p)
                off += n


def _into_target(params, net, tau, mirror):
    """`params` into the td._Net `net`'s flat buffer, hard (tau = 1) or as a Polyak step, and on into the mirror buffer that the
    target MODULE's parameters are views of; returns the (net, mirror) pair to keep"""
    with torch.no_grad():
        if tau == 1.0:
            net.params.copy_(params)
        else:
            net.params.lerp_(params, float(tau))
        if mirror is None or mirror[0] is not net:
            linears, _ = _read_layers(net.module, **dict(_WideShape._grid, tanh_head=net._tanh_head))
            buf, off = torch.empty_like(net.params), 0
            for lin in linears:
                for p in (lin.weight, lin.bias):
                    p.data = buf[off:off + p.numel()].view_as(p)
                    off += p.numel()
            mirror = (net, buf)
        mirror[1].copy_(net.params)
    return mirror


# ---------------------------------------------------------------------------------------------- what every learner's call does
def _batch_obs(who, lrn, batch, keys):
    """the checks of a sampled batch (`lrn` has ``device``, ``obs_dim`` and ``max_batch``); returns B and the pointer of batch['obs']"""
    if not isinstance(batch, dict) or any(k not in batch for k in keys):
        raise ValueError(f'{who}: batch must be a dict with ' + ' and '.join(repr(k) for k in keys) + " (DeviceReplay.sample's)")
    obs = batch['obs']
    if not torch.is_tensor(obs) or obs.dim() != 2 or obs.shape[0] < 1:
        raise ValueError(f"{who}: batch['obs'] must be a [B, {lrn.obs_dim}] tensor, B >= 1")
    B = obs.shape[0]
    if B > lrn.max_batch:
        raise ValueError(f'{who}: the batch has {B} rows, the learner was made with max_batch={lrn.max_batch}')
    return B, _arr(who, lrn.device, "batch['obs']", obs, torch.float32, (B, lrn.obs_dim))


def _opt(who, device, name, t, shape, dtype=torch.float32):
    """the pointer of an optional argument tensor, checked, or None"""
    return _arr(who, device, name, t, dtype, shape) if t is not None else None


def _launch(who, device, fn, calls):
    """the library's `fn` once per argument list of `calls`, each with torch's current stream of `device` behind it and its return
    code through _capi.check; ValueError where the learner is not on a GPU"""
    if device.type != 'cuda':
        raise ValueError(f'{who}: the networks are on {device}; the kernels need a GPU (there is no CPU path)')
    lib = _capi.load_library()
    with torch.cuda.device(device):
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        for args in calls:
            _capi.check(lib, getattr(lib, fn)(*args, stream), fn)


class _Stepped:
    """the flat fp32 device buffers that one optimiser steps: ``params``, Adam's ``m`` and ``v``, the gradient ``_grad``, the
    ``hyper`` words (lr, beta1, beta2, eps, max_grad_norm, beta1^t, beta2^t and the learner's own behind them), ``stats``, the
    ``error`` word and the ``workspace``"""

    def _alloc(self, P, device, lr, b1, b2, eps, max_grad_norm, more_hyper=(), n_stats=3):
        # torch's device allocations are 256-byte aligned (the ABI asks for 16 of the [P] arrays, 256 of the workspace)
        f32 = torch.float32
        self.params = torch.zeros(P, dtype=f32, device=torch.device(device))
        self.device = self.params.device                                     # with its index: 'cuda' -> cuda:0
        self.m, self.v, self._grad = (torch.zeros(P, dtype=f32, device=self.device) for _ in range(3))
        self.hyper = torch.tensor([lr, b1, b2, eps, max_grad_norm, 1.0, 1.0, *more_hyper], dtype=f32).to(self.device)
        self.stats = torch.zeros(n_stats, dtype=f32, device=self.device)
        self.error = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _alloc_workspace(self, workspace_bytes):
        self.workspace = torch.zeros(workspace_bytes // 4, dtype=torch.float32, device=self.device)

    def set_lr(self, lr):
        """the learning rate of the steps enqueued from now on: a device write, also between the replays of a captured graph"""
        self.hyper[0:1].fill_(float(lr))

    def reset_optimizer(self):
        """Adam as new: m = v = 0, both beta products 1"""
        self.m.zero_()
        self.v.zero_()
        self.hyper[5:7].fill_(1.0)


class _StepNet(_Stepped):
    """one network that a learner steps: its module (rebound to the flat buffer by ``bind``), shape, Adam state, device words and
    workspace.  PPOLearner reads its two networks' shapes with it and steps them in a buffer of its own."""
    loss_kind = 0             # S2DLearnState.loss_kind, where the call reads it
    grad = property(lambda self: self._grad)

    def __init__(self, who, what, module, tanh_head=False):
        self._linears, self.hidden, self.n_in, self.n_out, self.activation = _read_shape(who, what, module, tanh_head)
        self.what, self.module, self.mirror = what, module, None

    def alloc(self, device, lr, b1, b2, eps, max_grad_norm):
        """the buffers, on `device` (default: the module's); the workspace waits for ``bind``"""
        self._alloc(learn_param_count(self.n_in, self.hidden, self.n_out), device if device is not None else self._linears[0].weight.device,
                    lr, b1, b2, eps, max_grad_norm)
        return self

    def bind(self, workspace_bytes):
        """called once every network of the learner has passed its checks: the workspace, and the module's parameters as views"""
        self._alloc_workspace(workspace_bytes)
        _rebind(self.params, self._linears)

    text = _net_text

    def c_structs(self):
        net, st = _fill_shape(_capi.S2DLearnNet(), self), _capi.S2DLearnState()
        net.params, net.workspace, net.workspace_bytes = self.params.data_ptr(), self.workspace.data_ptr(), self.workspace.numel() * 4
        st.m, st.v, st.grad = self.m.data_ptr(), self.v.data_ptr(), self._grad.data_ptr()
        st.hyper, st.stats, st.error, st.loss_kind = self.hyper.data_ptr(), self.stats.data_ptr(), self.error.data_ptr(), self.loss_kind
        return net, st


class QLearner(_StepNet):
    """The online Q-network's optimiser step in one call.  ``q_net`` is Linear-(F-Linear) x L (SB3's ``q_net.q_net``)."""

    def __init__(self, q_net, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=10.0, loss='huber', max_batch=4096, device=None):
        who = 'QLearner'
        _StepNet.__init__(self, who, 'Q-network', q_net)
        if not 1 <= self.n_out <= MAX_OUT:
            raise ValueError(f'{who}: the Q-network\'s output width must be in [1, {MAX_OUT}], got {self.n_out}')
        if loss not in LOSSES:
            raise ValueError(f"{who}: loss must be 'huber' or 'mse', got {loss!r}")
        b1, b2 = _check_optimiser(who, max_batch, lr, betas, eps)
        self.loss_kind, self.max_batch, self.obs_dim = LOSSES.index(loss), max_batch, self.n_in
        self.alloc(device, lr, b1, b2, eps, max_grad_norm).bind(learn_workspace_bytes(self.n_in, self.hidden, self.n_out, max_batch))

    @classmethod
    def from_module(cls, q_net, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=10.0, loss='huber', max_batch=4096, device=None):
        """A learner of `q_net` with torch.optim.Adam's and clip_grad_norm_'s arguments (max_grad_norm <= 0: no clip), the loss
        ('huber': smooth_l1_loss with beta 1; 'mse': e^2 / 2) and the largest batch a step will see (it sizes the workspace).
        device: where the buffers, and from then on the module's parameters, live (default: the module's)."""
        return cls(q_net, lr=lr, betas=betas, eps=eps, max_grad_norm=max_grad_norm, loss=loss, max_batch=max_batch, device=device)

    # ------------------------------------------------------------------ the step
    def _call(self, fn, batch, target, weight, td_abs_out, q_out):
        who, dev = f'QLearner.{"step" if fn == "s2d_learn_q" else "grad"}', self.device
        B, obs = _batch_obs(who, self, batch, ('obs', 'action'))
        action = batch['action']
        if torch.is_tensor(action) and tuple(action.shape) == (B, 1):
            action = action.view(B) if action.is_contiguous() else action
        ptrs = [obs, _arr(who, dev, "batch['action'] ([B] or [B, 1])", action, torch.int32, (B,)),
                _arr(who, dev, 'target', target, torch.float32, (B,)), _opt(who, dev, 'weight', weight, (B,)),
                _opt(who, dev, 'td_abs_out', td_abs_out, (B,)), _opt(who, dev, 'q_out', q_out, (B, self.n_out))]
        _launch(who, dev, fn, [(B, *map(C.byref, self.c_structs()), *ptrs)])

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
        self.mirror = _into_target(self.params, net, tau, self.mirror)


class _ActorCritic:
    """what ActorCriticLearner and SACLearner share: an actor with A actions and one or two critics on [obs | action] as _StepNets,
    built and checked as a pair; the critics' call (s2d_learn_critic or its _grad twin, once per critic, the optional outputs from
    critic 1); learning rates, Adam's reset, the statistics and the pair check of ``update_targets``.  ``_sac``: the actor has 2 A
    outputs and no Tanh behind them, and a target's networks must agree in the activation too."""
    _sac = False

    def _networks(self, who, actor, q, q2, device, actor_lr, critic_lr, b1, b2, eps, max_grad_norm, max_batch):
        """the networks with their buffers, the pair's checks; nothing of a module is touched before ``_bind``"""
        a = self.actor = _StepNet(who, 'actor', actor, not self._sac).alloc(device, actor_lr, b1, b2, eps, max_grad_norm)
        dev = device if device is not None else a.device
        names = ('critic',) if q2 is None else ('critic 1', 'critic 2')
        self.critics = tuple(_StepNet(who, n, mod).alloc(dev, critic_lr, b1, b2, eps, max_grad_norm) for n, mod in zip(names, (q, q2)))
        A = a.n_out // 2 if self._sac else a.n_out
        if self._sac and (a.n_out % 2 or not 1 <= A <= MAX_ACTION):
            raise ValueError(f'{who}: the actor has {a.n_out} outputs; the kernel takes 2 A (A means, then A log-std rows) with A in '
                             f'1 .. {MAX_ACTION}')
        if not 1 <= A <= MAX_ACTION:
            raise ValueError(f'{who}: the actor has {a.n_out} outputs, the kernel takes 1 to {MAX_ACTION}')
        if a.n_in > MAX_OBS:
            raise ValueError(f'{who}: the actor\'s input width must be in [1, {MAX_OBS}], got {a.n_in}')
        for c in self.critics:
            if c.n_in != a.n_in + A or c.n_out != 1:
                raise ValueError(f'{who}: the {c.what} is {c.text()}; with the actor {a.text()} it must take obs_dim + A = '
                                 f'{a.n_in} + {A} inputs and give one output')
            if c.device != a.device:
                raise ValueError(f'{who}: the {c.what} is on {c.device}, the actor on {a.device}')
        self.device, self.obs_dim, self.action_dim, self.max_batch = a.device, a.n_in, A, max_batch

    def _bind(self, loss, actor_workspace_bytes):
        self.loss_kind = AC_LOSSES.index(loss)
        self.actor.bind(actor_workspace_bytes)
        for c in self.critics:
            c.loss_kind = self.loss_kind
            c.bind(learn_workspace_bytes(c.n_in, c.hidden, 1, self.max_batch))

    # ------------------------------------------------------------------ the critics' steps
    def _critic_call(self, fn, name, batch, target, weight, td_abs_out, q_out):
        who, dev, f32 = f'{type(self).__name__}.{name}', self.device, torch.float32
        B, obs = _batch_obs(who, self, batch, ('obs', 'action'))
        ptrs = [_arr(who, dev, "batch['action']", batch['action'], f32, (B, self.action_dim)), _arr(who, dev, 'target', target, f32, (B,)),
                _opt(who, dev, 'weight', weight, (B,))]
        outs = [_opt(who, dev, 'td_abs_out', td_abs_out, (B,)), _opt(who, dev, 'q_out', q_out, (B,))]
        _launch(who, dev, fn, ((B, *map(C.byref, c.c_structs()), obs, self.action_dim, *ptrs, *(outs if n == 0 else (None, None)))
                               for n, c in enumerate(self.critics)))

    def step_critic(self, batch, target, weight=None, td_abs_out=None, q_out=None):
        """One update of the critic (of both, where ``q2`` was given) on the dict DeviceReplay.sample returns (its 'obs' [B, obs_dim]
        and 'action' float32 [B, A]) towards `target` float32 [B] (ActorCriticTarget.target's; SACLearner: SacTarget.target's, with
        the loss e^2 / 2), with the importance weights `weight` [B] where given.  td_abs_out [B] <- |q1 - target| (the new
        priorities' base), q_out [B] <- critic 1's forward values.  Stream-ordered on torch's current stream, capturable; returns
        nothing."""
        self._critic_call('s2d_learn_critic', 'step_critic', batch, target, weight, td_abs_out, q_out)

    def grad_critic(self, batch, target, weight=None, td_abs_out=None, q_out=None):
        """The flat, unclipped gradient [P] of critic 1's loss (with ``q2`` the tuple of both critics'; views, written again by the
        next call), with the critic's statistics set, without touching parameters or optimiser state."""
        self._critic_call('s2d_learn_critic_grad', 'grad_critic', batch, target, weight, td_abs_out, q_out)
        return self.critics[0].grad if len(self.critics) == 1 else tuple(c.grad for c in self.critics)

    # ------------------------------------------------------------------ state
    critic_loss = property(lambda self: self.critics[0].stats.tolist()[0],
                           doc="critic 1's last mean loss (SACLearner: of e^2 / 2; synchronises)")
    critic_grad_norm = property(lambda self: self.critics[0].stats.tolist()[1], doc="critic 1's last gradient norm before the clip")
    critic_clip_scale = property(lambda self: self.critics[0].stats.tolist()[2], doc="the factor critic 1's last gradient was scaled by")
    actor_loss = property(lambda self: self.actor.stats.tolist()[0],
                          doc="the actor's last loss: -mean q (SACLearner: mean(alpha logp - min q)) (synchronises)")
    actor_grad_norm = property(lambda self: self.actor.stats.tolist()[1], doc="the actor's last gradient norm before the clip")
    actor_clip_scale = property(lambda self: self.actor.stats.tolist()[2], doc="the factor the actor's last gradient was scaled by")

    def set_lr(self, actor=None, critic=None):
        """the learning rates of the steps enqueued from now on: device writes, also between the replays of a captured graph"""
        if actor is not None:
            self.actor.set_lr(actor)
        if critic is not None:
            for c in self.critics:
                c.set_lr(critic)

    def reset_optimizer(self):
        """Adam as new for every network: m = v = 0, both beta products 1"""
        for n in (self.actor,) + self.critics:
            n.reset_optimizer()

    def _target_pairs(self, who, target, actor_net, tau):
        """update_targets' checks -- the critic count, every network's shape and device against the target's, tau -- and the
        (learner's, target's) pairs, the actor's first"""
        if len(target.critics) != len(self.critics):
            raise ValueError(f'{who}: the target has {len(target.critics)} critic(s), the learner {len(self.critics)}')
        pairs = list(zip((self.actor,) + self.critics, (actor_net,) + target.critics))

        def shape(n):
            return (n.n_in, n.hidden, n.n_out) + ((n.activation,) if self._sac else ())

        def text(n):
            return n.text() + (f' ({n.activation})' if self._sac else '')
        for mine, net in pairs:
            if shape(net) != shape(mine) or net.device != mine.device:
                raise ValueError(f'{who}: the {net.what} is {text(net)} on {net.device}, the learner\'s {mine.what} {text(mine)} on '
                                 f'{mine.device}')
        if not 0.0 <= tau <= 1.0:
            raise ValueError(f'{who}: tau must be in [0, 1], got {tau}')
        return pairs


class ActorCriticLearner(_ActorCritic):
    """The DDPG / TD3 update in HIP (s2d_learn_critic / s2d_learn_actor in include/s2d.h), the steps that follow
    ActorCriticTarget.target:

        critic:  e = q(cat(obs, action)) - target;  loss = mean(weight * e^2);  backward;  Adam.step()      (each critic)
        actor:   loss = -q(cat(obs, tanh-mu(obs))).mean();  backward through the critic;  Adam.step() on mu

    ``mu`` is Linear-(F-Linear) x L-Tanh with 1 .. 8 outputs, ``q`` (and TD3's ``q2``) Linear-(F-Linear) x L from obs_dim + A
    inputs to one output -- the forms td.ActorCriticTarget takes -- on the learner's grid (1 .. 4 hidden layers of multiples of 8
    in [8, 256], ReLU / Tanh / Sigmoid, obs_dim <= 248); actor and critics may differ in hidden shape and activation.  SB3's default
    [400, 300] is off this grid and stays with torch's optimisers.  Every network gets one flat fp32 buffer and its module's
    parameters are rebound as views of it, as QLearner does.  The actor's step goes through critic 1 (SB3's ``q1_forward``) and
    never forms or touches a critic's gradient.  Both steps are linear chains on torch's current stream, capturable; learning
    rates are device words (``set_lr``)."""

    def __init__(self, mu, q, q2=None, actor_lr=1e-3, critic_lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.0, loss='square',
                 max_batch=4096, device=None):
        who = 'ActorCriticLearner'
        if loss not in AC_LOSSES:
            raise ValueError(f"{who}: loss must be 'square' (F.mse_loss), 'mse' (e^2 / 2) or 'huber', got {loss!r}")
        b1, b2 = _check_optimiser(who, max_batch, min(actor_lr, critic_lr), betas, eps)
        self._networks(who, mu, q, q2, device, actor_lr, critic_lr, b1, b2, eps, max_grad_norm, max_batch)
        a = self.actor
        self._bind(loss, learn_actor_workspace_bytes(a.n_in, a.hidden, a.n_out, self.critics[0].hidden, max_batch))

    @classmethod
    def from_modules(cls, mu, q, q2=None, actor_lr=1e-3, critic_lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.0, loss='square',
                     max_batch=4096, device=None):
        """A learner of the modules with torch.optim.Adam's arguments (one optimiser per network, as SB3), clip_grad_norm_'s
        max_grad_norm per network (<= 0, the default: no clip, as SB3), the critic's loss ('square': F.mse_loss; 'mse': e^2 / 2;
        'huber') and the largest batch a step will see.  device: where the buffers, and from then on the modules' parameters, live
        (default: the actor's)."""
        return cls(mu, q, q2=q2, actor_lr=actor_lr, critic_lr=critic_lr, betas=betas, eps=eps, max_grad_norm=max_grad_norm, loss=loss,
                   max_batch=max_batch, device=device)

    # ------------------------------------------------------------------ the steps
    def _actor_call(self, fn, name, batch, action_out, q_out):
        who, dev = f'ActorCriticLearner.{name}', self.device
        B, obs = _batch_obs(who, self, batch, ('obs',))
        outs = [_opt(who, dev, 'action_out', action_out, (B, self.action_dim)), _opt(who, dev, 'q_out', q_out, (B,))]
        _launch(who, dev, fn, [(B, *map(C.byref, self.actor.c_structs()), C.byref(self.critics[0].c_structs()[0]), obs, *outs)])

    def step_actor(self, batch, action_out=None, q_out=None):
        """One update of the actor on -mean critic_1(obs, tanh-mu(obs)) over batch['obs'].  action_out [B, A] <- the actions the
        critic was evaluated at, q_out [B] <- its values (both before the update)."""
        self._actor_call('s2d_learn_actor', 'step_actor', batch, action_out, q_out)

    def step(self, batch, target, weight=None, td_abs_out=None, q_out=None, actor=True):
        """The critics' step, then (actor=True) the actor's through the UPDATED critic 1, as DDPG orders them.  TD3's
        ``policy_delay`` is the caller's: pass ``actor=(n_updates % policy_delay == 0)``; q_out is the critic step's."""
        self.step_critic(batch, target, weight=weight, td_abs_out=td_abs_out, q_out=q_out)
        if actor:
            self.step_actor(batch)

    def grad_actor(self, batch, action_out=None, q_out=None):
        """The flat, unclipped gradient [P] of the actor's loss, with the actor's statistics set, without touching anything else."""
        self._actor_call('s2d_learn_actor_grad', 'grad_actor', batch, action_out, q_out)
        return self.actor.grad

    def update_targets(self, ac_target, tau=1.0):
        """The learner's weights into a td.ActorCriticTarget's (or a td.Td3Target's) target networks: a hard copy (tau = 1) or a
        Polyak step, one ``copy_`` or ``lerp_`` per network from flat buffer to flat buffer, and one more flat copy each keeps the
        target MODULES equal (their parameters become views of mirror buffers), as QLearner.update_target."""
        from .td import ActorCriticTarget, Td3Target
        who = 'ActorCriticLearner.update_targets'
        if not isinstance(ac_target, (ActorCriticTarget, Td3Target)):
            raise ValueError(f'{who}: ac_target must be a td.ActorCriticTarget or a td.Td3Target')
        for mine, net in self._target_pairs(who, ac_target, ac_target.mu_target, tau):
            mine.mirror = _into_target(mine.params, net, tau, mine.mirror)


class SACLearner(_ActorCritic):
    """The Soft Actor-Critic update in HIP (s2d_learn_critic with the 'mse' loss per critic, s2d_learn_sac_actor in include/s2d.h),
    the steps that follow SacTarget.target:

        critics: loss = 0.5 * (mse(q1(cat(obs, action)), target) + mse(q2(...), target));  backward;  Adam.step()
        actor:   a, logp = squashed-Gaussian head of actor(obs), reparameterised, with the kernel's own noise
                 loss = (alpha * logp - min(q1, q2)(cat(obs, a))).mean();  backward through the critic that gave the minimum;  Adam.step()
        alpha:   loss = -(log_alpha * (logp + target_entropy).mean());  Adam.step();  alpha = exp(log_alpha)

    ``actor`` is ONE module Linear-(F-Linear) x L ending in Linear(h_L, 2A) (A means, then A raw log-std rows clamped to [-20, 2];
    A = 1 .. 8), ``q1`` (and ``q2``) Linear-(F-Linear) x L from obs_dim + A inputs to one output -- the forms td.SacTarget and
    wide_actor.SquashedGaussianActor take -- on the learner's grid (1 .. 4 hidden layers of multiples of 8 in [8, 256], ReLU / Tanh /
    Sigmoid, obs_dim <= 248); the three may differ in hidden shape and activation.  SB3's default [256, 256] is on this grid; its
    module triple (latent_pi, mu, log_std) is not taken.  Every network gets one flat fp32 buffer and its module's parameters are
    rebound as views of it, as QLearner does.  The actor's step never forms or touches a critic's gradient.  ``alpha`` is the [1]
    device tensor SacTarget.target takes; every step is a linear chain on torch's current stream, capturable; learning rates are
    device words (``set_lr``).  tests/learn_sac_ref.c."""
    _sac = True

    def __init__(self, actor, q1, q2=None, ent_coef='auto', target_entropy=None, actor_lr=3e-4, critic_lr=3e-4, alpha_lr=3e-4,
                 betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.0, max_batch=4096, seed=0, device=None):
        who = 'SACLearner'
        if isinstance(actor, (tuple, list)):
            raise ValueError(f'{who}: the actor must be ONE nn.Module ending in Linear(h_L, 2A); SB3\'s (latent_pi, mu, log_std) triple '
                             'is not taken by the learner (stack mu and log_std into one Linear)')
        if ent_coef != 'auto' and (isinstance(ent_coef, (str, bool)) or not isinstance(ent_coef, (int, float)) or not ent_coef >= 0.0
                                   or ent_coef == float('inf')):
            raise ValueError(f"{who}: ent_coef must be 'auto' or a finite float >= 0, got {ent_coef!r}")
        if not (alpha_lr >= 0.0):
            raise ValueError(f'{who}: alpha_lr must be >= 0, got {alpha_lr}')
        b1, b2 = _check_optimiser(who, max_batch, min(actor_lr, critic_lr), betas, eps)
        self._networks(who, actor, q1, q2, device, actor_lr, critic_lr, b1, b2, eps, max_grad_norm, max_batch)
        if target_entropy is not None and not isinstance(target_entropy, (int, float)):
            raise ValueError(f'{who}: target_entropy must be a float (or None: -A), got {target_entropy!r}')
        a, A = self.actor, self.action_dim
        self.seed = int(seed) & (2 ** 64 - 1)
        self.auto = ent_coef == 'auto'
        self.target_entropy = float(-A if target_entropy is None else target_entropy)
        f32 = torch.float32
        self.alpha = torch.full((1,), 1.0 if self.auto else float(ent_coef), dtype=f32, device=self.device)
        self.log_alpha = torch.zeros(1, dtype=f32, device=self.device) if self.auto else None
        self.alpha_m_v = torch.zeros(2, dtype=f32, device=self.device)
        self.alpha_hyper = torch.tensor([alpha_lr, b1, b2, eps, 0.0, 1.0, 1.0], dtype=f32).to(self.device)
        self.alpha_stats = torch.tensor([0.0, 0.0, float(self.alpha[0])], dtype=f32).to(self.device)
        self.draws = torch.zeros(1, dtype=torch.int64, device=self.device)       # steps so far: the Philox counter's middle words
        hc = [c.hidden for c in self.critics]
        self._bind('mse', learn_sac_workspace_bytes(a.n_in, a.hidden, A, hc[0], hc[1] if len(hc) > 1 else None, max_batch))

    @classmethod
    def from_modules(cls, actor, q1, q2=None, ent_coef='auto', target_entropy=None, actor_lr=3e-4, critic_lr=3e-4, alpha_lr=3e-4,
                     betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.0, max_batch=4096, seed=0, device=None):
        """A learner of the modules with SB3 SAC's arguments: ent_coef 'auto' (log_alpha = 0, learned towards target_entropy, default
        -A) or a float (fixed), torch.optim.Adam's arguments (one optimiser per network and one for log_alpha), clip_grad_norm_'s
        max_grad_norm per network (<= 0, the default: no clip, as SB3), the largest batch a step will see and the seed of the actor
        step's noise.  device: where the buffers, and from then on the modules' parameters, live (default: the actor's)."""
        return cls(actor, q1, q2=q2, ent_coef=ent_coef, target_entropy=target_entropy, actor_lr=actor_lr, critic_lr=critic_lr,
                   alpha_lr=alpha_lr, betas=betas, eps=eps, max_grad_norm=max_grad_norm, max_batch=max_batch, seed=seed, device=device)

    # ------------------------------------------------------------------ the steps
    def alpha_struct(self):
        """the S2DLearnSacAlpha of a learned temperature, or None"""
        if not self.auto:
            return None
        t = _capi.S2DLearnSacAlpha()
        t.log_alpha, t.m_v, t.hyper, t.stats = (x.data_ptr() for x in (self.log_alpha, self.alpha_m_v, self.alpha_hyper, self.alpha_stats))
        t.target_entropy = self.target_entropy
        return t

    def _actor_call(self, fn, name, batch, action_out, logp_out, q_out):
        who, dev = f'SACLearner.{name}', self.device
        B, obs = _batch_obs(who, self, batch, ('obs',))
        outs = [_opt(who, dev, 'action_out', action_out, (B, self.action_dim)), _opt(who, dev, 'logp_out', logp_out, (B,)),
                _opt(who, dev, 'q_out', q_out, (B,))]
        cs = [C.byref(c.c_structs()[0]) for c in self.critics]
        t = self.alpha_struct()
        _launch(who, dev, fn, [(B, *map(C.byref, self.actor.c_structs()), cs[0], cs[1] if len(cs) > 1 else None, obs,
                                C.c_void_p(self.alpha.data_ptr()), C.byref(t) if t is not None else None, C.c_void_p(self.draws.data_ptr()),
                                self.seed, *outs)])

    def step_actor(self, batch, action_out=None, logp_out=None, q_out=None):
        """One update of the actor on (alpha * logp - min Q(obs, a)).mean() over batch['obs'] and, with ent_coef='auto', of log_alpha;
        ``alpha`` then holds exp(log_alpha) and ``draws`` is one more.  action_out [B, A] <- the sampled actions, logp_out [B] <-
        their log-probabilities, q_out [B] <- the smaller critic's values (all before the update)."""
        self._actor_call('s2d_learn_sac_actor', 'step_actor', batch, action_out, logp_out, q_out)

    def step(self, batch, target, weight=None, td_abs_out=None, q_out=None):
        """The critics' step, then the actor's (and the temperature's) through the UPDATED critics, as SB3 orders them; q_out is the
        critic step's."""
        self.step_critic(batch, target, weight=weight, td_abs_out=td_abs_out, q_out=q_out)
        self.step_actor(batch)

    def grad_actor(self, batch, action_out=None, logp_out=None, q_out=None):
        """The flat, unclipped gradient [P] of the actor's loss at the noise the next step will draw, with the actor's statistics,
        ``entropy`` and ``alpha_loss`` set, without touching anything else (``draws`` included)."""
        self._actor_call('s2d_learn_sac_actor_grad', 'grad_actor', batch, action_out, logp_out, q_out)
        return self.actor.grad

    # ------------------------------------------------------------------ state
    def _alpha_stat(self, i):
        if not self.auto:
            raise ValueError('SACLearner: the entropy coefficient is fixed: the temperature has no statistics (ent_coef=\'auto\')')
        return self.alpha_stats.tolist()[i]

    entropy = property(lambda self: -self._alpha_stat(0), doc="minus the last actor call's mean logp (ent_coef='auto'; synchronises)")
    alpha_loss = property(lambda self: self._alpha_stat(1), doc="the last actor call's log_alpha * -(mean logp + target_entropy)")
    ent_coef = property(lambda self: float(self.alpha.item()), doc='the entropy coefficient now (synchronises)')

    def set_lr(self, actor=None, critic=None, alpha=None):
        """the learning rates of the steps enqueued from now on: device writes, also between the replays of a captured graph"""
        _ActorCritic.set_lr(self, actor, critic)
        if alpha is not None:
            self.alpha_hyper[0:1].fill_(float(alpha))

    def reset_optimizer(self):
        """Adam as new for every network and for log_alpha: m = v = 0, both beta products 1"""
        _ActorCritic.reset_optimizer(self)
        self.alpha_m_v.zero_()
        self.alpha_hyper[5:7].fill_(1.0)

    def update_targets(self, sac_target, tau=1.0):
        """The learner's weights into a td.SacTarget: the critics into its target critics, a hard copy (tau = 1) or a Polyak step,
        one ``copy_`` or ``lerp_`` per critic from flat buffer to flat buffer with one more flat copy each that keeps the target
        MODULES equal (as ActorCriticLearner.update_targets), and ONE flat ``copy_`` of the actor into the buffer the target reads its
        ONLINE actor from.  Capturable: a loop that calls this needs no ``sac_target.sync()``."""
        from .td import SacTarget
        who = 'SACLearner.update_targets'
        if not isinstance(sac_target, SacTarget):
            raise ValueError(f'{who}: sac_target must be a td.SacTarget')
        for mine, net in self._target_pairs(who, sac_target, sac_target.actor, tau)[1:]:
            mine.mirror = _into_target(mine.params, net, tau, mine.mirror)
        with torch.no_grad():
            sac_target.actor.params.copy_(self.actor.params)


class PPOLearner(_Stepped):
    """The PPO update in HIP (s2d_learn_ppo in include/s2d.h): what the examples' minibatch loop does in torch --

        logp, entropy = dist(pi(obs[i])).log_prob(action[i]), .entropy();  a = normalised advantage[i]
        ratio = exp(logp - logp_old[i]);  pg = -min(ratio a, clamp(ratio, 1 - c, 1 + c) a).mean()
        loss = pg + vf_coef mse_loss(vf(obs[i]), return[i]) - ent_coef entropy.mean()
        backward;  clip_grad_norm_(all parameters, max_grad_norm);  Adam.step()

    -- as one call, the gather by ``index`` included.  ``pi`` and ``vf`` are separate Linear-(F-Linear) x L modules on the learner's
    grid (1 .. 4 hidden layers of multiples of 8 in [8, 256], ReLU / Tanh / Sigmoid, at most 256 inputs) on the same observation;
    without ``log_std`` the head is categorical (1 .. 64 logits, int32 actions), with it diagonal Gaussian (1 .. 8 means, float
    actions as Engine.rollout_policy records them).  ONE flat buffer [pi | vf | log_std] holds every parameter, and the modules'
    parameters and the log_std nn.Parameter are rebound as views of it: ``StochasticActor.sync()``, ``MatchPolicyActor.sync()``,
    ``vf(obs)`` in torch for GAE and ``state_dict()`` keep working unchanged.  One Adam, one gradient norm and one clip run over
    all of it.  Every hyper-parameter is a device word read when the kernels run: a step is a linear chain on torch's current
    stream, capturable, and ``set_lr`` / ``set_clip_range`` / ``set_coefs`` between replays take effect.  tests/learn_ppo_ref.c."""

    def __init__(self, pi, vf, log_std=None, lr=3e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5, clip_range=0.2, vf_coef=0.5,
                 ent_coef=0.0, normalize_advantage=True, max_batch=65536, device=None):
        who = 'PPOLearner'
        self.pi, self.vf = _StepNet(who, 'policy network', pi), _StepNet(who, 'value network', vf)   # their shapes: the buffers are the learner's
        p, q = self.pi, self.vf
        self.head = 0 if log_std is None else 1
        if q.n_in != p.n_in or q.n_out != 1:
            raise ValueError(f'{who}: the value network is {q.text()}; with the policy network {p.text()} it must take {p.n_in} inputs '
                             f'and give one output')
        if self.head:
            if not isinstance(log_std, torch.nn.Parameter) or log_std.dtype != torch.float32 or log_std.numel() != p.n_out:
                raise ValueError(f'{who}: log_std must be a float32 nn.Parameter of {p.n_out} values (or None: a categorical policy)')
            if not 1 <= p.n_out <= MAX_ACTION:
                raise ValueError(f'{who}: the Gaussian head takes 1 to {MAX_ACTION} means, the policy network has {p.n_out} outputs')
        elif not 1 <= p.n_out <= MAX_OUT:
            raise ValueError(f'{who}: the categorical head takes 1 to {MAX_OUT} logits, the policy network has {p.n_out} outputs')
        b1, b2 = _check_optimiser(who, max_batch, lr, betas, eps)
        if not (clip_range >= 0.0 and vf_coef >= 0.0 and ent_coef >= 0.0):
            raise ValueError(f'{who}: clip_range, vf_coef and ent_coef must be >= 0, got {clip_range}, {vf_coef}, {ent_coef}')
        self.obs_dim, self.n_out, self.max_batch, self.normalize_advantage = p.n_in, p.n_out, max_batch, bool(normalize_advantage)
        self.P_pi, self.P_vf = learn_param_count(p.n_in, p.hidden, p.n_out), learn_param_count(q.n_in, q.hidden, 1)
        self._alloc(self.P_pi + self.P_vf + (p.n_out if self.head else 0), device if device is not None else p._linears[0].weight.device,
                    lr, b1, b2, eps, max_grad_norm, (clip_range, vf_coef, ent_coef), 8)
        self._alloc_workspace(learn_ppo_workspace_bytes(p.n_in, p.hidden, p.n_out, q.hidden, self.head, max_batch))
        _rebind(self.params[:self.P_pi], p._linears)
        _rebind(self.params[self.P_pi:self.P_pi + self.P_vf], q._linears)
        self.log_std = log_std
        if self.head:
            with torch.no_grad():
                view = self.params[self.P_pi + self.P_vf:]
                view.copy_(log_std.detach().reshape(-1))
                log_std.data = view.view_as(log_std)

    @classmethod
    def from_modules(cls, pi, vf, log_std=None, lr=3e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5, clip_range=0.2, vf_coef=0.5,
                     ent_coef=0.0, normalize_advantage=True, max_batch=65536, device=None):
        """A learner of the modules with SB3 PPO's arguments: torch.optim.Adam's (one optimiser over everything), clip_grad_norm_'s
        max_grad_norm over everything (<= 0: no clip), the clip range, the two coefficients, per-minibatch advantage normalisation,
        and the largest minibatch a step will see (it sizes the workspace).  device: where the buffers, and from then on the
        modules' parameters and log_std, live (default: the policy network's)."""
        return cls(pi, vf, log_std=log_std, lr=lr, betas=betas, eps=eps, max_grad_norm=max_grad_norm, clip_range=clip_range, vf_coef=vf_coef,
                   ent_coef=ent_coef, normalize_advantage=normalize_advantage, max_batch=max_batch, device=device)

    # ------------------------------------------------------------------ the step
    def c_structs(self):
        q = _capi.S2DLearnPPO()
        _fill_shape(q.pi, self.pi), _fill_shape(q.vf, self.vf)
        q.head, q.normalize_advantage = self.head, int(self.normalize_advantage)
        q.params, q.m, q.v, q.grad = self.params.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self._grad.data_ptr()
        q.hyper, q.stats, q.error = self.hyper.data_ptr(), self.stats.data_ptr(), self.error.data_ptr()
        q.workspace, q.workspace_bytes = self.workspace.data_ptr(), self.workspace.numel() * 4
        return q

    def _call(self, fn, rollout, index, logp_out, value_out):
        who, f32 = f'PPOLearner.{"step" if fn == "s2d_learn_ppo" else "grad"}', torch.float32
        keys = ('obs', 'action', 'logp', 'advantage', 'return')
        if not isinstance(rollout, dict) or any(k not in rollout for k in keys):
            raise ValueError(f'{who}: rollout must be a dict with ' + ', '.join(repr(k) for k in keys) + ', flattened to [R, ...]')
        obs = rollout['obs']
        if not torch.is_tensor(obs) or obs.dim() != 2 or not 1 <= obs.shape[0] < 2 ** 31:
            raise ValueError(f"{who}: rollout['obs'] must be a [R, {self.obs_dim}] tensor, 1 <= R < 2^31")
        R = obs.shape[0]
        if index is not None and (not torch.is_tensor(index) or index.dim() != 1 or index.shape[0] < 1):
            raise ValueError(f'{who}: index must be an int32 tensor [B], B >= 1 (or None: every row)')
        B = index.shape[0] if index is not None else R
        if B > self.max_batch:
            raise ValueError(f'{who}: the minibatch has {B} rows, the learner was made with max_batch={self.max_batch}')

        def arr(name, t, dtype, shape):
            return _arr(who, self.device, name, t, dtype, shape)
        action = (arr("rollout['action']", rollout['action'], f32, (R, self.n_out)) if self.head
                  else arr("rollout['action']", rollout['action'], torch.int32, (R,)))
        b = _capi.S2DLearnPPOBatch()
        b.rows, b.batch = R, B
        b.obs, b.action = arr("rollout['obs']", obs, f32, (R, self.obs_dim)), action
        b.logp_old, b.advantage = arr("rollout['logp']", rollout['logp'], f32, (R,)), arr("rollout['advantage']", rollout['advantage'], f32, (R,))
        b.ret = arr("rollout['return']", rollout['return'], f32, (R,))
        b.index = _opt(who, self.device, 'index', index, (B,), torch.int32)
        b.out_logp, b.out_value = _opt(who, self.device, 'logp_out', logp_out, (B,)), _opt(who, self.device, 'value_out', value_out, (B,))
        _launch(who, self.device, fn, [(C.byref(self.c_structs()), C.byref(b))])

    def step(self, rollout, index=None, logp_out=None, value_out=None):
        """One update on the minibatch that `index` (int32 [B]; None: every row, in order) names in the rollout: a dict with 'obs'
        [R, obs_dim], 'action' (int32 [R], or float32 [R, A] with log_std), 'logp', 'advantage' and 'return' [R] -- the flattened
        record of Engine.rollout_policy and gae().  The epochs pass ``perm[s:s + mb]``: the permuted minibatch never exists in
        memory.  logp_out / value_out [B] <- the rows' log-probabilities and values before the update.  Stream-ordered on torch's
        current stream, capturable; returns nothing: read ``loss`` and the other statistics when they are wanted."""
        self._call('s2d_learn_ppo', rollout, index, logp_out, value_out)

    def grad(self, rollout, index=None, logp_out=None, value_out=None):
        """The flat, unclipped gradient [P] over [pi | vf | log_std] (a view, written again by the next call) of the same loss, with
        the statistics set, without touching the parameters or the optimiser's state."""
        self._call('s2d_learn_ppo_grad', rollout, index, logp_out, value_out)
        return self._grad

    # ------------------------------------------------------------------ state
    def _stat(self, i):
        host = self.stats.tolist()                                           # synchronises
        err = int(self.error.item())
        if err:
            self.error.zero_()
            why = ([f'an action outside [0, {self.n_out})'] if err & 1 else []) + (['an index outside [0, R)'] if err & 2 else [])
            raise ValueError(f'PPOLearner: a minibatch held {" and ".join(why)}: its rows were left out of the update')
        return host[i]

    loss = property(lambda self: self._stat(0), doc='the last call\'s loss: pg + vf_coef v_loss - ent_coef entropy (synchronises; '
                    'raises ValueError if a minibatch since the last look held a bad action or index)')
    grad_norm = property(lambda self: self._stat(1), doc='the last call\'s gradient norm over all parameters, before the clip')
    clip_scale = property(lambda self: self._stat(2), doc='the factor the last call\'s gradient was scaled by')
    policy_loss = property(lambda self: self._stat(3), doc='the last call\'s mean clipped-surrogate loss')
    value_loss = property(lambda self: self._stat(4), doc='the last call\'s mean squared value error')
    entropy = property(lambda self: self._stat(5), doc='the last call\'s mean entropy')
    approx_kl = property(lambda self: self._stat(6), doc='mean((ratio - 1) - log ratio) of the last call (SB3\'s approx_kl)')
    clip_fraction = property(lambda self: self._stat(7), doc='the share of the last call\'s rows with |ratio - 1| > clip_range')

    def set_clip_range(self, clip_range):
        """the clip range of the steps enqueued from now on (a schedule writes it as it writes lr)"""
        self.hyper[7:8].fill_(float(clip_range))

    def set_coefs(self, vf_coef=None, ent_coef=None):
        """the value and entropy coefficients of the steps enqueued from now on"""
        if vf_coef is not None:
            self.hyper[8:9].fill_(float(vf_coef))
        if ent_coef is not None:
            self.hyper[9:10].fill_(float(ent_coef))


__all__ = ['QLearner', 'ActorCriticLearner', 'SACLearner', 'PPOLearner', 'learn_workspace_bytes', 'learn_actor_workspace_bytes',
           'learn_sac_workspace_bytes', 'learn_ppo_workspace_bytes', 'learn_param_count']
