"""QTarget / ActorCriticTarget / Td3Target: the off-policy learners' TD targets from their target networks in one launch
(s2d_td_target_q / s2d_td_target_ac in include/s2d.h), the step that follows DeviceReplay.sample in DQN, Double DQN, DDPG and TD3:

    target = reward + discount * max_a Q'(next_obs, a)                          QTarget
    target = reward + discount * Q'(next_obs, argmax_a Q(next_obs, a))          QTarget with online=
    target = reward + discount * min_i Q'_i(next_obs, tanh-actor'(next_obs))    ActorCriticTarget
    target = reward + discount * min_i Q'_i(next_obs, that action, smoothed)    Td3Target

instead of the 8 - 15 small torch ops of ``r + d * q_target(next_obs).max(dim=1).values``.  The networks are the streamed-weight
MLP of the wide actors (Linear-(F-Linear) x L, L = 1 .. 5, widths multiples of 4 in [8, 400], F = ReLU, Tanh or Sigmoid) with any
input width up to 256, evaluated on the project's fp32 spec: at obs_dim = 10 the value bootstrapped from is the same function of
the weights, bit for bit, that the fused actor acts on.  Engine-independent: any batch with the replay buffer's layout.

Each network keeps ONE flat fp32 parameter buffer and a workspace.  The kernels read the buffers when they run: ``sync()``
reloads them from the modules (after ``load_state_dict`` or a Polyak step for the target networks, after every optimiser step
for ``online``), and a captured graph computes with whatever they hold at replay.  The online Q-network's forward / backward pass and the
optimiser are soccer2d_amd.learn.QLearner's, the DDPG / TD3 update soccer2d_amd.learn.ActorCriticLearner's.  Out of scope: the target is not fused into the sample launch.
TD3's target-policy smoothing noise is Td3Target's (s2d_td_target_td3): ActorCriticTarget's launch with clipped Gaussian noise on
the target actor's action, from a Philox stream and a device counter of its own.

SacTarget is Soft Actor-Critic's: the ONLINE actor's squashed-Gaussian head draws the next action, and the target carries the
entropy term, reward + discount * (min_i Q'_i(next_obs, a') - alpha * logp(a')) (s2d_td_target_sac)."""
import ctypes as C

import torch

from . import _capi
from .actor import _read_layers
from .mlp_actor import _fragments
from .wide_actor import ACTIVATIONS, _WideShape

MAX_IN = 256
MAX_OUT = 64
MAX_ACTION = 8
_WAVE = 64


def td_workspace_bytes(n_in, hidden, n_out):
    """bytes of a network's workspace, by the arithmetic of the C plan (s2d_td_workspace_bytes): every layer's fragments
    (ceil(h / 16) tiles x its k-steps, ceil(n_in / 4) for layer 1, h_(l-1) / 4 after it, 64 words each) and the biases padded to
    their tiles"""
    nfrag, nbias = _fragments(hidden, n_out, n_in)[:2]
    return (nfrag * _WAVE + nbias) * 4


def _arr(who, device, name, t, dtype, shape):
    """the pointer of an argument tensor, checked"""
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or t.device != device or not t.is_contiguous():
        raise ValueError(f'{who}: {name} must be a contiguous {dtype} tensor of shape {shape} on {device}')
    return C.c_void_p(t.data_ptr())


def _fill_shape(net, shape):
    """n_in, n_hidden, hidden[], n_out and activation of a C struct from `shape` (a _Net or a learn.QLearner)"""
    net.n_in, net.n_hidden, net.n_out = shape.n_in, len(shape.hidden), shape.n_out
    for l in range(len(net.hidden)):
        net.hidden[l] = shape.hidden[l] if l < len(shape.hidden) else 0
    net.activation = ACTIVATIONS.index(shape.activation)
    return net


def _net_text(shape):
    return '-'.join(map(str, (shape.n_in,) + shape.hidden + (shape.n_out,)))


class _Net:
    """one network of a target: its module, shape, flat parameter buffer and workspace"""

    def __init__(self, who, what, module, device, tanh_head=False):
        self.what, self.module, self._tanh_head = what, module, tanh_head
        if not self._is_module():
            raise ValueError(f'{who}: the {what} must be a torch.nn.Module')
        try:
            tensors, n_in, widths, act = self._read()
        except ValueError as e:
            raise ValueError(f'{who}: {what}: {e}') from None
        if any(t is None for t in tensors):
            raise ValueError(f'{who}: every nn.Linear of the {what} needs a bias')
        self.hidden = _WideShape._check_shape(widths[:-1], widths[-1], act)
        self.n_in, self.n_out, self.activation = n_in, widths[-1], act
        if not 1 <= self.n_in <= MAX_IN:
            raise ValueError(f'{who}: the {what}\'s input width must be in [1, {MAX_IN}], got {self.n_in}')
        if not 1 <= self.n_out <= MAX_OUT:
            raise ValueError(f'{who}: the {what}\'s output width must be in [1, {MAX_OUT}], got {self.n_out}')
        dev = torch.device(device if device is not None else tensors[0].device)
        # torch's device allocations are 256-byte aligned (the ABI asks for 16 of params, 256 of the workspace)
        self.params = torch.zeros(sum(t.numel() for t in tensors), dtype=torch.float32, device=dev)
        self.device = self.params.device                                     # with its index: 'cuda' -> cuda:0
        self.workspace = torch.zeros(td_workspace_bytes(self.n_in, self.hidden, self.n_out) // 4, dtype=torch.float32, device=self.device)
        self.sync()

    def _is_module(self):
        return isinstance(self.module, torch.nn.Module)

    def _read(self):
        """(the flat buffer's tensors in order, n_in, the layers' widths, the activation) of the module as it is now"""
        # the wide actors' reader and grid: Linear-(F-Linear) x L [-Tanh], one F of ReLU / Tanh / Sigmoid throughout
        linears, act = _read_layers(self.module, **dict(_WideShape._grid, tanh_head=self._tanh_head))
        tensors = []
        for lin in linears:
            tensors += [lin.weight, lin.bias]
        return tensors, linears[0].in_features, [lin.out_features for lin in linears], act

    def sync(self):
        """the module's current parameters into the flat buffer: one device copy, no allocation of what the kernel reads"""
        tensors, n_in, widths, act = self._read()
        if act != self.activation or (n_in, widths) != (self.n_in, list(self.hidden) + [self.n_out]):
            raise ValueError(f'the {self.what} has changed its shape since from_module')
        with torch.no_grad():
            torch.cat([t.detach().reshape(-1).to(self.device, torch.float32) for t in tensors], out=self.params)

    text = _net_text

    def c_struct(self):
        net = _fill_shape(_capi.S2DTdNet(), self)
        net.params = self.params.data_ptr()
        net.workspace = self.workspace.data_ptr()
        net.workspace_bytes = self.workspace.numel() * 4
        return net


class _Target:
    """what the targets share: the networks on one device, sync() and the checks of target()'s arguments"""

    _name = '_Target'

    def _init_nets(self, nets):
        self._nets = nets
        self.device = nets[0].device
        for n in nets[1:]:
            if n.device != self.device:
                raise ValueError(f'{self._name}: the {n.what} is on {n.device}, the {nets[0].what} on {self.device}')
        self.obs_dim = nets[0].n_in

    def sync(self):
        """Reload every network's parameter buffer from its module, in place: after ``load_state_dict`` or a Polyak step for
        the target networks, after every optimiser step for ``online``.  Stream-ordered device copies, capturable."""
        for n in self._nets:
            n.sync()
        return self

    def _arr(self, name, t, dtype, shape):
        return _arr(f'{self._name}.target', self.device, name, t, dtype, shape)

    def _batch(self, batch, out, return_q, extra_dtype, extra_shape):
        """target()'s argument checks: (B, the pointers of next_obs / reward / discount, the three outputs)"""
        who = f'{self._name}.target'
        if not isinstance(batch, dict) or any(k not in batch for k in ('next_obs', 'reward', 'discount')):
            raise ValueError(f"{who}: batch must be a dict with 'next_obs', 'reward' and 'discount' (DeviceReplay.sample's)")
        nxt = batch['next_obs']
        if not torch.is_tensor(nxt) or nxt.dim() != 2 or nxt.shape[0] < 1 or nxt.shape[0] >= 2 ** 31:
            raise ValueError(f"{who}: batch['next_obs'] must be a [B, {self.obs_dim}] tensor, 1 <= B < 2^31")
        B, f32 = nxt.shape[0], torch.float32
        ins = [self._arr("batch['next_obs']", nxt, f32, (B, self.obs_dim)), self._arr("batch['reward']", batch['reward'], f32, (B,)),
               self._arr("batch['discount']", batch['discount'], f32, (B,))]
        if out is None:
            outs = [torch.empty((B,), dtype=f32, device=self.device)]
            if return_q:
                outs += [torch.empty((B,), dtype=f32, device=self.device), torch.empty((B,) + extra_shape, dtype=extra_dtype, device=self.device)]
        else:
            outs = list(out) if isinstance(out, (tuple, list)) else [out]
            if len(outs) != (3 if return_q else 1):
                raise ValueError(f'{who}: out must be ' + ('a tuple of three tensors (target, q, the index or action)' if return_q
                                                           else 'one tensor [B]'))
        shapes = [((B,), f32), ((B,), f32), ((B,) + extra_shape, extra_dtype)]
        ptrs = [self._arr(f'out[{j}]' if return_q else 'out', t, shapes[j][1], shapes[j][0]) for j, t in enumerate(outs)]
        ptrs += [None] * (3 - len(ptrs))
        if self.device.type != 'cuda':
            raise ValueError(f'{who}: the networks are on {self.device}; the kernels need a GPU (there is no CPU path)')
        return B, ins, ptrs, (tuple(outs) if return_q else outs[0])


class QTarget(_Target):
    """``reward + discount * max_a q_target(next_obs)[a]`` (DQN), or with ``online`` the target network's value at the online
    network's argmax (Double DQN), in one launch.  Both modules are Linear-(F-Linear) x L (SB3's ``q_net_target.q_net`` /
    ``q_net.q_net``) with the same input and output widths; hidden shapes and activations may differ."""

    _name = 'QTarget'

    def __init__(self, q_target, online=None, device=None):
        tgt = _Net('QTarget', 'target Q-network', q_target, device)
        nets = [tgt]
        if online is not None:
            onl = _Net('QTarget', 'online Q-network', online, device if device is not None else tgt.device)
            if (onl.n_in, onl.n_out) != (tgt.n_in, tgt.n_out):
                raise ValueError(f'QTarget: the online Q-network is {onl.text()}, the target {tgt.text()}: input and output widths must '
                                 'be the same')
            nets.append(onl)
        self.q_target, self.online = tgt, (nets[1] if online is not None else None)
        self.n_actions = tgt.n_out
        self._init_nets(nets)

    @classmethod
    def from_module(cls, q_target, online=None, device=None):
        """A target shaped like the modules, loaded from them.  device: where the buffers live (default: the modules')."""
        return cls(q_target, online=online, device=device)

    def target(self, batch, out=None, return_q=False):
        """float32 [B] targets of the dict DeviceReplay.sample / PrioritizedReplay.sample returns (its 'next_obs' [B, obs_dim],
        'reward' and 'discount' [B]).  return_q: (target, q [B], index int32 [B]): the bootstrapped value and the action it was
        read at.  out: the tensor (with return_q the tuple of three) of an earlier call, written again (a captured graph replays
        into it).  Stream-ordered on torch's current stream, capturable."""
        B, ins, outs, result = self._batch(batch, out, return_q, torch.int32, ())
        lib = _capi.load_library()
        net, onl = self.q_target.c_struct(), (self.online.c_struct() if self.online is not None else None)
        with torch.cuda.device(self.device):
            rc = lib.s2d_td_target_q(B, C.byref(net), C.byref(onl) if onl is not None else None, *ins, *outs,
                                     C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        _capi.check(lib, rc, 's2d_td_target_q')
        return result


class _ActorCriticTarget(_Target):
    """what ActorCriticTarget, Td3Target and SacTarget share: an actor and one or two critics on obs_dim + A inputs, and the
    launch of their entry point"""

    _entry = None                              # the C entry point
    _actor = (_Net, 'target actor', True)      # the actor's reader, what the errors call it, whether the module ends in a Tanh

    def __init__(self, actor, q_target, q_target2, device, seed=None):
        who = self._name
        net, what, tanh_head = self._actor
        act = net(who, what, actor, device, tanh_head=tanh_head)
        self.action_dim = A = self._actions(act)
        dev = device if device is not None else act.device
        critics = [_Net(who, 'target critic 1', q_target, dev)]
        if q_target2 is not None:
            critics.append(_Net(who, 'target critic 2', q_target2, dev))
        for c in critics:
            if c.n_in != act.n_in + A or c.n_out != 1:
                raise ValueError(f'{who}: the {c.what} is {c.text()}; with the actor {act.text()} it must take obs_dim + A = '
                                 f'{act.n_in} + {A} inputs and give one output')
        self.critics = tuple(critics)
        self._init_nets([act] + critics)
        if seed is not None:
            self.seed = int(seed) & (2 ** 64 - 1)
            self.draws = torch.zeros(1, dtype=torch.int64, device=self.device)  # calls so far: the Philox counter's middle words

    def _actions(self, act):
        """A of the actor's n_out: here n_out itself, 1 .. 8"""
        if not 1 <= act.n_out <= MAX_ACTION:
            raise ValueError(f'{self._name}: the target actor has {act.n_out} outputs, the kernel takes 1 to {MAX_ACTION}')
        return act.n_out

    def _launch(self, B, ins, words, outs):
        """the entry point on torch's current stream: the networks, the batch arrays, the target's own `words`, the outputs"""
        lib = _capi.load_library()
        nets = [n.c_struct() for n in self._nets]
        with torch.cuda.device(self.device):
            rc = getattr(lib, self._entry)(B, C.byref(nets[0]), C.byref(nets[1]), C.byref(nets[2]) if len(nets) > 2 else None, *ins, *words,
                                           *outs, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        _capi.check(lib, rc, self._entry)


class ActorCriticTarget(_ActorCriticTarget):
    """``reward + discount * q_target(cat(next_obs, mu_target(next_obs)))`` (DDPG), with ``q_target2`` the smaller of the two
    critics' values (TD3's clipped double-Q; with target-policy smoothing noise: Td3Target), in one launch.  mu_target is
    Linear-(F-Linear) x L-Tanh with 1 .. 8 outputs (SB3's ``actor_target.mu``); a critic is Linear-(F-Linear) x L from
    obs_dim + A inputs to one output (SB3's ``critic_target.qf0``)."""

    _name, _entry = 'ActorCriticTarget', 's2d_td_target_ac'

    def __init__(self, mu_target, q_target, q_target2=None, device=None):
        super().__init__(mu_target, q_target, q_target2, device)
        self.mu_target = self._nets[0]

    @classmethod
    def from_modules(cls, mu_target, q_target, q_target2=None, device=None):
        """A target shaped like the modules, loaded from them.  device: where the buffers live (default: the actor's)."""
        return cls(mu_target, q_target, q_target2=q_target2, device=device)

    def target(self, batch, out=None, return_q=False):
        """float32 [B] targets of a sampled batch, as QTarget.target.  return_q: (target, q [B], action [B, A]): the bootstrapped
        value and the target actor's action it was evaluated at."""
        B, ins, outs, result = self._batch(batch, out, return_q, torch.float32, (self.action_dim,))
        self._launch(B, ins, (), outs)
        return result


class Td3Target(_ActorCriticTarget):
    """TD3's target in one launch (s2d_td_target_td3): ActorCriticTarget's with target-policy smoothing,

        a'     = (mu_target(next_obs) + (sigma * z).clamp(-clip, clip)).clamp(-1, 1)     z ~ N(0, 1), fresh every call
        target = reward + discount * min_i Q'_i(next_obs, a')

    The networks are ActorCriticTarget's: mu_target Linear-(F-Linear) x L-Tanh with 1 .. 8 outputs, a critic Linear-(F-Linear) x L
    from obs_dim + A inputs to one output.  sigma (SB3's ``target_policy_noise``) and clip (``target_noise_clip``) are two device
    words the target owns (``noise``, written by ``set_noise``); z is Philox with key `seed` at a device counter the target owns
    (``draws``): every call, and every replay of a captured graph, advances it by one."""

    _name, _entry = 'Td3Target', 's2d_td_target_td3'

    def __init__(self, mu_target, q_target, q_target2=None, target_policy_noise=0.2, target_noise_clip=0.5, seed=0, device=None):
        super().__init__(mu_target, q_target, q_target2, device, seed=seed)
        self.mu_target = self._nets[0]
        self.noise = torch.zeros(2, dtype=torch.float32, device=self.device)    # sigma, clip: read when the kernel runs
        self.set_noise(target_policy_noise, target_noise_clip)

    @classmethod
    def from_modules(cls, mu_target, q_target, q_target2=None, target_policy_noise=0.2, target_noise_clip=0.5, seed=0, device=None):
        """A target shaped like the modules, loaded from them.  device: where the buffers live (default: the actor's)."""
        return cls(mu_target, q_target, q_target2=q_target2, target_policy_noise=target_policy_noise, target_noise_clip=target_noise_clip,
                   seed=seed, device=device)

    def set_noise(self, sigma, clip):
        """sigma (target_policy_noise) and clip (target_noise_clip) into the device words the kernel reads, in place: legal
        between the replays of a captured graph.  Both are floats >= 0 (clip may be inf: no clipping)."""
        for name, v in (('sigma', sigma), ('clip', clip)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not v >= 0.0:
                raise ValueError(f'Td3Target.set_noise: {name} must be a float >= 0, got {v!r}')
        self.noise[0].fill_(float(sigma))
        self.noise[1].fill_(float(clip))
        return self

    def target(self, batch, out=None, return_q=False):
        """float32 [B] targets of a sampled batch, as ActorCriticTarget.target.  return_q: (target, q [B], action [B, A]): the
        bootstrapped value and the smoothed, clamped action it was evaluated at."""
        B, ins, outs, result = self._batch(batch, out, return_q, torch.float32, (self.action_dim,))
        self._launch(B, ins, (C.c_void_p(self.noise.data_ptr()), C.c_void_p(self.draws.data_ptr()), self.seed), outs)
        return result


class _SacActorNet(_Net):
    """the online actor of SacTarget: one module ending in Linear(h_L, 2A) (A means, then A log-std rows), or SB3's triple
    (latent_pi, mu, log_std), read into the same flat buffer: ..., [mu.weight ; log_std.weight], [mu.bias | log_std.bias]"""

    def _is_module(self):
        m = self.module
        return isinstance(m, torch.nn.Module) or (isinstance(m, (tuple, list)) and len(m) == 3
                                                  and all(isinstance(x, torch.nn.Module) for x in m))

    def _read(self):
        if isinstance(self.module, torch.nn.Module):
            return super()._read()
        latent_pi, mu, log_std = self.module
        linears, act = _read_layers([latent_pi, mu], **dict(_WideShape._grid, many=True))
        mu = linears[-1]
        if not isinstance(log_std, torch.nn.Linear) or (log_std.in_features, log_std.out_features) != (mu.in_features, mu.out_features):
            raise ValueError(f'log_std must be a Linear({mu.in_features}, {mu.out_features}) like mu, got {log_std}')
        tensors = []
        for lin in linears[:-1]:
            tensors += [lin.weight, lin.bias]
        tensors += [mu.weight, log_std.weight, mu.bias, log_std.bias]
        return tensors, linears[0].in_features, [lin.out_features for lin in linears[:-1]] + [2 * mu.out_features], act


class SacTarget(_ActorCriticTarget):
    """Soft Actor-Critic's entropy-regularised target in one launch (s2d_td_target_sac):

        a', logp = squashed-Gaussian head of actor(next_obs)     the ONLINE actor, as in SB3, with fresh noise every call
        target   = reward + discount * (min_i Q'_i(next_obs, a') - alpha * logp)

    actor: Linear-(F-Linear) x L ending in Linear(h_L, 2A) (A means, then A raw log-std rows, clamped to [-20, 2]; A = 1 .. 8), or
    SB3's triple ``(actor.latent_pi, actor.mu, actor.log_std)``; a critic is Linear-(F-Linear) x L from obs_dim + A inputs to one
    output (SB3's ``critic_target.qf0``).  The noise is Philox with key `seed` at a device counter the target owns (``draws``):
    every call, and every replay of a captured graph, advances it by one."""

    _name, _entry = 'SacTarget', 's2d_td_target_sac'
    _actor = (_SacActorNet, 'actor', False)

    def __init__(self, actor, q_target, q_target2=None, seed=0, device=None):
        super().__init__(actor, q_target, q_target2, device, seed=seed)
        self.actor = self._nets[0]
        self._alpha = torch.zeros(1, dtype=torch.float32, device=self.device)   # where a Python float alpha is written

    def _actions(self, act):
        """A of the actor's n_out = 2 A"""
        if act.n_out % 2 or not 1 <= act.n_out // 2 <= MAX_ACTION:
            raise ValueError(f'{self._name}: the actor has {act.n_out} outputs; the kernel takes 2 A (A means, then A log-std rows) with A in '
                             f'1 .. {MAX_ACTION}')
        return act.n_out // 2

    @classmethod
    def from_modules(cls, actor, q_target, q_target2=None, seed=0, device=None):
        """A target shaped like the modules, loaded from them.  device: where the buffers live (default: the actor's)."""
        return cls(actor, q_target, q_target2=q_target2, seed=seed, device=device)

    def target(self, batch, alpha, out=None, return_q=False):
        """float32 [B] targets of a sampled batch, as QTarget.target.  alpha: the entropy coefficient, a float (written in place
        into a device word the target owns) or a one-element float32 device tensor the kernel reads when it runs (a captured
        graph computes with what it holds at replay).  return_q: (target, q [B], action [B, A], logp [B]): the smaller critic's
        value, the sampled action it was evaluated at and that action's log-probability; `out` is then the tuple of four."""
        who = 'SacTarget.target'
        logp = None
        if return_q and out is not None:
            if not isinstance(out, (tuple, list)) or len(out) != 4:
                raise ValueError(f'{who}: out must be a tuple of four tensors (target, q, action, logp)')
            out, logp = tuple(out[:3]), out[3]
        B, ins, outs, result = self._batch(batch, out, return_q, torch.float32, (self.action_dim,))
        if return_q:
            if logp is None:
                logp = torch.empty((B,), dtype=torch.float32, device=self.device)
            lp = self._arr('out[3]', logp, torch.float32, (B,))
            result = tuple(result) + (logp,)
        else:
            lp = None
        if torch.is_tensor(alpha):
            a = self._arr('alpha', alpha.reshape(-1) if alpha.dim() == 0 else alpha, torch.float32, (1,))
        else:
            self._alpha.fill_(float(alpha))
            a = C.c_void_p(self._alpha.data_ptr())
        self._launch(B, ins, (a, C.c_void_p(self.draws.data_ptr()), self.seed), outs + [lp])
        return result


__all__ = ['QTarget', 'ActorCriticTarget', 'Td3Target', 'SacTarget', 'td_workspace_bytes']
