"""QNetActor: the device-side state of the fused epsilon-greedy actor (Engine.rollout_qnet, s2d_rollout_qnet in include/s2d.h).
DeterministicActor: the same for the fused tanh actor of continuous and turning engines (Engine.rollout_actor,
s2d_rollout_actor), SB3's DDPG / TD3 ``actor.mu`` with optional Gaussian action noise.  StochasticActor: the sampled policy of
on-policy collection (Engine.rollout_policy, s2d_rollout_policy): a categorical or diagonal-Gaussian head with log-probabilities.

It owns ONE packed fp32 parameter buffer in torch's ``nn.Sequential(Linear, ReLU, Linear, ReLU, Linear).parameters()`` order
(W1[H1][10], b1[H1], W2[H2][H1], b2[H2], W3[A][H2], b3[A]) and a device epsilon scalar.  The kernel reads both when it runs, so a
learner updates them in place (``sync()`` after an optimiser phase, ``epsilon = ...``) and a captured graph acts with the new
values at its next replay.  SB3's ``DQN.q_net.q_net`` (an nn.Sequential of that shape) qualifies as the source module.
"""
import math

import torch

from . import _capi

OBS_DIM = _capi.S2D_OBS_DIM
WIDTHS = tuple(range(16, 129, 16))
MAX_ACTIONS = 64


_NO_OPS = (torch.nn.Identity, torch.nn.Flatten)   # SB3's features extractor of a flat Box observation is a Flatten
_ACT_KINDS = {torch.nn.ReLU: 'ReLU', torch.nn.Tanh: 'Tanh', torch.nn.Sigmoid: 'Sigmoid'}


def _read_layers(module, acts=('ReLU',), hidden=(2, 2), tanh_head=False, many=False):
    """(the nn.Linear layers in order, the hidden activation's name in lower case) of a module of the form the kernels evaluate:
    Linear-(F-Linear) x L with L in hidden = (fewest, most) hidden layers and one F of `acts` throughout; with tanh_head the module
    must end in one more Tanh (the deterministic actors' head); with many, `module` may be a list / tuple of modules read one
    after the other (SB3's ``[policy.mlp_extractor.policy_net, policy.action_net]``).  Leaf modules are read in registration
    order; Identity / Flatten are skipped; anything else (another activation, a mix, a missing one, a layer too many) is refused:
    the kernel would silently act with a different function."""
    mods = list(module) if many and isinstance(module, (list, tuple)) else [module]
    leaves = [m for mod in mods for m in mod.modules() if not any(True for _ in m.children()) and not isinstance(m, _NO_OPS)]
    kinds = ['Linear' if isinstance(m, torch.nn.Linear) else _ACT_KINDS.get(type(m), type(m).__name__) for m in leaves]
    what = 'actor' if tanh_head else 'Q-network'
    got = '-'.join(kinds) or 'nothing'
    fewest, most = hidden
    if fewest == most:                  # one depth: the module is one of len(acts) forms
        for name in acts:
            want = ['Linear'] + [name, 'Linear'] * most + (['Tanh'] if tanh_head else [])
            if kinds == want:
                return leaves[0:2 * most + 1:2], name.lower()
        if len(acts) == 1:
            raise ValueError(f'the {what} must be {"-".join(want)} (10 -> H1 -> H2 -> A), got {got}')
        raise ValueError('the policy must be Linear-F-Linear-F-Linear (10 -> H1 -> H2 -> A) with F = ReLU or Tanh, the same twice, '
                         f'got {got}')
    names = ', '.join(acts[:-1]) + ' or ' + acts[-1]
    form = 'Linear-(F-Linear) x L' + ('-Tanh' if tanh_head else '') + f', L = {fewest} .. {most} hidden layers, F = {names}'
    body = kinds
    if tanh_head:
        if not kinds or kinds[-1] != 'Tanh':
            raise ValueError(f'the actor must end in a Tanh ({form}), got {got}')
        body = kinds[:-1]
    if len(body) % 2 == 0 or any(k != 'Linear' for k in body[0::2]):
        raise ValueError(f'the {what} must be {form}, got {got}')
    used = set(body[1::2])
    n_hidden = len(body) // 2
    if not fewest <= n_hidden <= most:
        raise ValueError(f'the {what} must have {fewest} to {most} hidden layers ({form}), got {n_hidden}: {got}')
    if len(used) > 1 and used <= set(acts):
        raise ValueError(f'the {what} must use one activation throughout, {names}, not a mix ({form}), got {got}')
    if not used <= set(acts):
        raise ValueError(f'the hidden activation must be {names} ({form}), got {got}')
    return leaves[0:len(body):2], used.pop().lower()


class _PackedActor:
    """What every actor does alike: ONE packed fp32 parameter buffer on a resolved device, sized from shapes(), loaded from a
    module the class's reader accepts (load_from) and refreshed from it in place (sync).  A class says how its modules read
    (`_grid`, the arguments of _read_layers), what its texts call the network (`_what`), which C entry point of the reach-ball
    engine launches it (`_entry`; Engine.rollout_qnet / rollout_actor read it), and its layers' widths (`_widths`)."""

    _grid = {}
    _what = 'Q-network'
    _shape_error = '{what} shapes {got} do not match the actor {want}'
    _entry = None
    in_dim = OBS_DIM
    activation = None               # the hidden activation's name, where the class has a choice
    _buffers = ('params',)          # the device buffers a snapshot() copies
    _has_noise = False              # the Gaussian action-noise rows of the deterministic actors

    def _init_packed(self, device):
        self.device = torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        # torch's device allocations are 256-byte aligned (the ABI asks for 16)
        self.params = torch.zeros(sum(math.prod(shape) for shape in self.shapes()), dtype=torch.float32, device=self.device)
        self._module = None

    @classmethod
    def _read(cls, module):
        return _read_layers(module, **cls._grid)

    @property
    def _outputs(self):
        """the output layer's width: n_actions, or n_out in the classes that call it so"""
        return self.n_actions

    def _widths(self):
        return (self.hidden1, self.hidden2, self._outputs)

    def shapes(self):
        out, win = [], self.in_dim
        for w in self._widths():
            out += [(w, win), (w,)]
            win = w
        return tuple(out)

    def _validate(self, module):
        linears, act = self._read(module)
        got = []
        for lin in linears:
            if lin.bias is None:
                raise ValueError(f'every nn.Linear of the {self._what} needs a bias')
            got += [tuple(lin.weight.shape), tuple(lin.bias.shape)]
        if self.activation is not None and act != self.activation:
            raise ValueError(f'the {self._what}\'s activation is {act}, the actor\'s {self.activation}')
        if tuple(got) != self.shapes():
            raise ValueError(self._shape_error.format(what=self._what, got=got, want=list(self.shapes())))

    def load_from(self, module):
        """Validate `module` against this actor (shapes, and the activation where there is a choice), remember it, and pack its
        parameters (sync())."""
        self._validate(module)
        self._module = module
        return self.sync()

    def sync(self):
        """Copy the loaded module's current parameters into the packed buffer: one device copy, no allocation of the buffers the
        kernel reads (capturable)."""
        if self._module is None:
            raise ValueError('no module loaded (load_from)')
        srcs = []
        for lin in self._read(self._module)[0]:
            srcs += [lin.weight.detach().reshape(-1), lin.bias.detach().reshape(-1)]
        with torch.no_grad():
            torch.cat([s.to(self.device, torch.float32) for s in srcs], out=self.params)
        return self

    def _frozen(self, snap):
        """`snap`, a new actor of this shape, with copies of this one's buffers (snapshot())"""
        for name in self._buffers:
            getattr(snap, name).copy_(getattr(self, name))
        return snap


class _Epsilon:
    """the device epsilon scalar of the epsilon actors"""

    def _init_epsilon(self, epsilon):
        self._eps = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._eps_value = None
        self.epsilon = epsilon

    @property
    def epsilon(self):
        return self._eps_value

    @epsilon.setter
    def epsilon(self, value):
        """Written in place into the device scalar the kernel reads (stream-ordered on torch's current stream)."""
        self._eps_value = float(value)
        self._eps.fill_(self._eps_value)

    @property
    def epsilon_tensor(self):
        return self._eps


class _Deterministic:
    """the device `deterministic` word of the stochastic policies"""

    def _init_deterministic(self, deterministic):
        self._det = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._det_value = False
        self.deterministic = deterministic

    @property
    def deterministic(self):
        return self._det_value

    @deterministic.setter
    def deterministic(self, value):
        """Written in place into the device word the kernel reads (stream-ordered on torch's current stream)."""
        self._det_value = bool(value)
        self._det.fill_(int(self._det_value))

    @property
    def deterministic_tensor(self):
        return self._det


def param_count(hidden1, hidden2, n_actions):
    return OBS_DIM * hidden1 + hidden1 + hidden1 * hidden2 + hidden2 + n_actions * hidden2 + n_actions


class QNetActor(_Epsilon, _PackedActor):
    """Packed parameters + device epsilon of a 10-H1-H2-A ReLU MLP for Engine.rollout_qnet."""

    _entry = 's2d_rollout_qnet'

    def __init__(self, hidden1=64, hidden2=64, n_actions=16, device='cuda:0', epsilon=0.05):
        for name, w in (('hidden1', hidden1), ('hidden2', hidden2)):
            if int(w) not in WIDTHS:
                raise ValueError(f'{name} must be a multiple of 16 in [16, 128], got {w}')
        if not 1 <= int(n_actions) <= MAX_ACTIONS:
            raise ValueError(f'n_actions must be in [1, {MAX_ACTIONS}], got {n_actions}')
        self.hidden1, self.hidden2, self.n_actions = int(hidden1), int(hidden2), int(n_actions)
        self._init_packed(device)
        self._init_epsilon(epsilon)

    @classmethod
    def from_module(cls, module, device=None, epsilon=0.05):
        """An actor shaped like `module` (three nn.Linear layers 10 -> H1 -> H2 -> A), loaded from it."""
        (l1, l2, l3), _ = cls._read(module)
        dev = device if device is not None else l1.weight.device
        actor = cls(l1.out_features, l2.out_features, l3.out_features, device=dev, epsilon=epsilon)
        actor.load_from(module)
        return actor

    def c_struct(self):
        net = _capi.S2DQNet()
        net.hidden1, net.hidden2, net.n_actions, net.reserved = self.hidden1, self.hidden2, self.n_actions, 0
        net.params = self.params.data_ptr()
        net.epsilon = self._eps.data_ptr()
        return net


ACTOR_OUTPUTS = (1, 4)   # use_continuous_action without / with use_turning


class DeterministicActor(_Epsilon, _PackedActor):
    """Packed parameters, device epsilon and Gaussian action noise of a 10-H1-H2-A tanh actor for Engine.rollout_actor.

    a = tanh(W3 relu(W2 relu(W1 x + b1) + b2) + b3), SB3's DDPG / TD3 ``model.actor.mu``; A = 1 on a continuous engine, 4 on a
    turning one.  noise_sigma=None: no action noise (kind 0); otherwise the kernel adds mu + sigma z, z ~ N(0, 1) per output
    (truncated at |z| <= 5.77), and clips to [-1, 1], as SB3's NormalActionNoise does.  The parameter, epsilon and (mu, sigma)
    buffers are written in place and read when the kernel runs, so a captured graph acts with what they hold at replay; the
    noise kind (None or not) selects the kernel and is fixed at capture."""

    _grid = dict(tanh_head=True)
    _what = 'actor'
    _shape_error = '{what} shapes {got} do not match {want}'
    _entry = 's2d_rollout_actor'
    _has_noise = True
    _outputs = property(lambda self: self.n_out)

    def __init__(self, hidden1=64, hidden2=64, n_out=1, device='cuda:0', epsilon=0.0, noise_mean=None, noise_sigma=None):
        for name, w in (('hidden1', hidden1), ('hidden2', hidden2)):
            if int(w) not in WIDTHS:
                raise ValueError(f'{name} must be a multiple of 16 in [16, 128] (the weights live in LDS), got {w}; SB3\'s '
                                 f'default DDPG net_arch=[400, 300] does not fit: use policy_kwargs=dict(net_arch=[64, 64])')
        if int(n_out) not in ACTOR_OUTPUTS:
            raise ValueError(f'n_out must be 1 (continuous engine) or 4 (turning engine), got {n_out}')
        self.hidden1, self.hidden2, self.n_out = int(hidden1), int(hidden2), int(n_out)
        self._init_packed(device)
        self._init_epsilon(epsilon)
        self._init_noise(noise_mean, noise_sigma)

    def _init_noise(self, noise_mean, noise_sigma):
        self._noise = torch.zeros(2, self.n_out, dtype=torch.float32, device=self.device)   # [mu; sigma]
        self._sigma = None
        self.noise_mean = 0.0 if noise_mean is None else noise_mean
        self.noise_sigma = noise_sigma

    @classmethod
    def from_module(cls, module, device=None, epsilon=0.0, noise_mean=None, noise_sigma=None):
        """An actor shaped like `module` (SB3's actor.mu: Linear-ReLU-Linear-ReLU-Linear-Tanh, optionally behind a Flatten or
        Identity), loaded from it."""
        (l1, l2, l3), _ = cls._read(module)
        dev = device if device is not None else l1.weight.device
        actor = cls(l1.out_features, l2.out_features, l3.out_features, device=dev, epsilon=epsilon, noise_mean=noise_mean,
                    noise_sigma=noise_sigma)
        actor.load_from(module)
        return actor

    def _set_row(self, row, value):
        v = torch.as_tensor(value, dtype=torch.float32).reshape(-1)
        if v.numel() not in (1, self.n_out):
            raise ValueError(f'expected a scalar or {self.n_out} values, got {v.numel()}')
        self._noise[row].copy_(v.expand(self.n_out))

    @property
    def noise_mean(self):
        return self._noise[0]

    @noise_mean.setter
    def noise_mean(self, value):
        """mu of the Gaussian action noise (scalar or [A]), written in place."""
        self._set_row(0, value)

    @property
    def noise_sigma(self):
        """sigma of the Gaussian action noise ([A] device tensor), or None: no action noise."""
        return None if self._sigma is None else self._noise[1]

    @noise_sigma.setter
    def noise_sigma(self, value):
        if value is None:
            self._sigma = None
            return
        self._set_row(1, value)
        self._sigma = True

    @property
    def noise_kind(self):
        return 0 if self._sigma is None else 1

    def c_struct(self):
        net = _capi.S2DActorNet()
        net.hidden1, net.hidden2, net.n_out, net.noise_kind = self.hidden1, self.hidden2, self.n_out, self.noise_kind
        net.params = self.params.data_ptr()
        net.epsilon = self._eps.data_ptr()
        net.noise = self._noise.data_ptr()
        return net


_POLICY_GRID = dict(acts=('ReLU', 'Tanh'), many=True)


class StochasticActor(_Deterministic, _PackedActor):
    """Packed parameters, device log_std and the deterministic word of a 10-H1-H2-A stochastic policy for Engine.rollout_policy
    (s2d_rollout_policy): on-policy collection for PPO / A2C.

    y = W3 f(W2 f(W1 x + b1) + b2) + b3 with f = ReLU or Tanh (``activation`` 'relu' / 'tanh'; Tanh is SB3's default for PPO's
    MlpPolicy).  On a discrete engine y are the logits of a categorical policy (A = action_space_size <= 64); on a continuous
    (A = 1) or turning (A = 4) engine the means of a diagonal Gaussian with the state-independent ``log_std`` [A] (SB3's
    ``policy.log_std``).  The kernel samples, records the unclipped action and its log-probability, and hands the env the
    clipped action.  ``deterministic = True`` switches to greedy actions (argmax / clipped mean).  The parameter buffer,
    log_std and the deterministic word are device buffers written in place and read when the kernel runs, so a captured graph
    acts with what they hold at replay: an evaluation pass is the collection graph with ``deterministic = True``."""

    _grid = _POLICY_GRID
    _what = 'policy'
    _buffers = ('params', '_log_std')
    _outputs = property(lambda self: self.n_out)

    def __init__(self, hidden1=64, hidden2=64, n_out=16, activation='tanh', device='cuda:0', log_std=0.0, deterministic=False):
        for name, w in (('hidden1', hidden1), ('hidden2', hidden2)):
            if int(w) not in WIDTHS:
                raise ValueError(f'{name} must be a multiple of 16 in [16, 128] (the weights live in LDS), got {w}')
        if not 1 <= int(n_out) <= MAX_ACTIONS:
            raise ValueError(f'n_out must be in [1, {MAX_ACTIONS}], got {n_out}')
        if activation not in ('relu', 'tanh'):
            raise ValueError(f"activation must be 'relu' or 'tanh', got {activation!r}")
        self.hidden1, self.hidden2, self.n_out, self.activation = int(hidden1), int(hidden2), int(n_out), activation
        self._init_packed(device)
        self._init_deterministic(deterministic)
        self._log_std = torch.zeros(self.n_out, dtype=torch.float32, device=self.device)
        self.log_std = log_std
        self._log_std_src = None

    @classmethod
    def from_module(cls, policy_net, log_std=None, device=None, deterministic=False):
        """An actor shaped like `policy_net`, loaded from it.  Accepted: an nn.Module whose leaves are Linear-F-Linear-F-Linear
        with F = ReLU or Tanh (a leading Flatten / Identity is skipped), or a list / tuple of modules that read so one after the
        other: SB3's ``[model.policy.mlp_extractor.policy_net, model.policy.action_net]``.  log_std: None (zeros), a scalar,
        [A] values, or a tensor / nn.Parameter that sync() reads again (SB3's ``model.policy.log_std``)."""
        (l1, l2, l3), act = cls._read(policy_net)
        dev = device if device is not None else l1.weight.device
        actor = cls(l1.out_features, l2.out_features, l3.out_features, activation=act, device=dev, deterministic=deterministic)
        actor.load_from(policy_net, log_std=log_std)
        return actor

    def load_from(self, policy_net, log_std=None):
        """Validate `policy_net` against this actor (shapes and activation), remember it and `log_std` (if a tensor), and pack
        them (sync())."""
        self._validate(policy_net)
        if log_std is not None:
            if torch.is_tensor(log_std):
                if log_std.numel() != self.n_out:
                    raise ValueError(f'log_std must have {self.n_out} values, got {log_std.numel()}')
                self._log_std_src = log_std
            else:
                self.log_std = log_std
        self._module = policy_net
        return self.sync()

    def sync(self):
        """Copy the loaded module's current parameters (and the remembered log_std tensor) into the device buffers: device
        copies, no allocation of the buffers the kernel reads (capturable)."""
        super().sync()
        if self._log_std_src is not None:
            with torch.no_grad():
                self._log_std.copy_(self._log_std_src.detach().reshape(-1))
        return self

    @property
    def log_std(self):
        """the device log_std [A] the kernel reads"""
        return self._log_std

    @log_std.setter
    def log_std(self, value):
        """a scalar or [A] values, written in place"""
        v = torch.as_tensor(value, dtype=torch.float32).detach().reshape(-1)
        if v.numel() not in (1, self.n_out):
            raise ValueError(f'expected a scalar or {self.n_out} values, got {v.numel()}')
        self._log_std.copy_(v.expand(self.n_out))

    def snapshot(self, deterministic=None):
        """A frozen copy: a new actor of the same shape with its own parameters, log_std and deterministic word (the old policy
        of a PPO update, an evaluation copy).  It has no module: later sync() calls of the original do not touch it."""
        return self._frozen(type(self)(self.hidden1, self.hidden2, self.n_out, activation=self.activation, device=self.device,
                                       deterministic=self._det_value if deterministic is None else deterministic))

    def c_struct(self):
        net = _capi.S2DPolicyNet()
        net.hidden1, net.hidden2, net.n_out = self.hidden1, self.hidden2, self.n_out
        net.activation = 1 if self.activation == 'tanh' else 0
        net.params = self.params.data_ptr()
        net.log_std = self._log_std.data_ptr()
        net.deterministic = self._det.data_ptr()
        return net


def match_param_count(h1, h2, k):
    """words of a 224-H1-H2-K network in nn.Sequential order"""
    return h1 * MATCH_OBS_DIM + h1 + h2 * h1 + h2 + k * h2 + k


MATCH_OBS_DIM = 224                  # S2D_AGENT_OBS_DIM: the 11v11 engine's per-agent row
MATCH_SEE_DIM = 192                  # S2D_SEE_DIM: its see row (the vision layer)
MATCH_WIDTHS = (16, 32, 48, 64)
MATCH_MAX_ACTIONS = 64


class _ActionTable:
    """the device action table of the 11v11 actors: float32 [K, table_width]"""

    _buffers = ('params', 'table')

    def _init_table(self, table):
        self.table = torch.zeros((self.n_actions, self.table_width), dtype=torch.float32, device=self.device)
        if table is not None:
            self.set_table(table)

    def set_table(self, table):
        """Write the action table (float [K, 3] = command, a, b per index; obs='see': [K, 5], with the TurnNeck moment and the
        ChangeView code) in place."""
        t = torch.as_tensor(table, dtype=torch.float32)
        if tuple(t.shape) != (self.n_actions, self.table_width):
            raise ValueError(f'action table must have shape ({self.n_actions}, {self.table_width}), got {tuple(t.shape)}')
        self.table.copy_(t.to(self.device))
        return self


class MatchQNetActor(_ActionTable, _Epsilon, _PackedActor):
    """Packed parameters, device epsilon and action table of a 224-H1-H2-K ReLU Q-network for the 11v11 engine's network slots
    (MatchEngine.set_network, s2d_match_set_network in include/s2d_match.h).

    The network sees one agent's own-frame row (MatchEngine.agent_observations); its index chooses a row of `table`, float32
    [K, 3] = (command, a, b).  params, epsilon and table are device buffers written in place (``sync()``, ``epsilon = ...``,
    ``set_table()``) and read when the kernel runs, so a captured graph acts with what they hold at replay.

    obs='see': a 192-H1-H2-K network on the agent's see row (MatchEngine.see: partial observability) with a table float32
    [K, 5] = (command, a, b, TurnNeck moment, ChangeView code) -- the see network of include/s2d_match.h
    (s2d_match_set_see_network): the index chooses the body command and the view action.

    obs='belief': the same network and table on the agent's belief row (MatchEngine.belief: the memory over its see rows) -- head
    0 of the belief network of include/s2d_match.h (s2d_match_set_belief_network): the cycle kernel builds the see row, takes
    it into the belief row and acts on that."""

    def __init__(self, hidden1=64, hidden2=64, n_actions=16, device='cuda:0', epsilon=0.05, table=None, obs='agent'):
        if obs not in ('agent', 'see', 'belief'):
            raise ValueError(f"obs must be 'agent', 'see' or 'belief', got {obs!r}")
        self.obs = obs
        self.in_dim = MATCH_OBS_DIM if obs == 'agent' else MATCH_SEE_DIM
        self.table_width = 3 if obs == 'agent' else 5
        for name, w in (('hidden1', hidden1), ('hidden2', hidden2)):
            if int(w) not in MATCH_WIDTHS:
                raise ValueError(f'{name} must be one of {MATCH_WIDTHS}, got {w}')
        if not 1 <= int(n_actions) <= MATCH_MAX_ACTIONS:
            raise ValueError(f'n_actions must be in [1, {MATCH_MAX_ACTIONS}], got {n_actions}')
        self.hidden1, self.hidden2, self.n_actions = int(hidden1), int(hidden2), int(n_actions)
        self._init_packed(device)
        self._init_epsilon(epsilon)
        self._init_table(table)

    @classmethod
    def from_module(cls, module, table, device=None, epsilon=0.05, obs='agent'):
        """An actor shaped like `module` (three nn.Linear layers 224 -> H1 -> H2 -> K), loaded from it, with action table
        `table` [K, 3]; obs='see' or 'belief': 192 -> H1 -> H2 -> K and a table [K, 5]."""
        (l1, l2, l3), _ = cls._read(module)
        dev = device if device is not None else l1.weight.device
        actor = cls(l1.out_features, l2.out_features, l3.out_features, device=dev, epsilon=epsilon, obs=obs)
        actor.load_from(module)
        actor.set_table(table)
        return actor

    def snapshot(self, epsilon=0.0):
        """A frozen copy: a new actor of the same shape with its own copies of the packed parameters and the action table and
        its own epsilon -- the league member a learner plays against (MatchEngine.set_opponent_network).  It has no module:
        later sync() calls of the original do not touch it."""
        return self._frozen(type(self)(self.hidden1, self.hidden2, self.n_actions, device=self.device, epsilon=epsilon, obs=self.obs))

    def c_struct(self, slot_mask, vision_params=None, vision=None, belief_params=None, belief=None, belief_mask=0):
        """S2DMatchNet; obs='see': S2DMatchSeeNet, which needs the engine's vision parameters and planes; obs='belief':
        S2DMatchBeliefNet (head 0), which also needs the engine's belief parameters, buffer and mask."""
        from . import _capi_match as M
        if self.obs == 'belief':
            net = _belief_struct(self, slot_mask, vision_params, vision, belief_params, belief, belief_mask)
            net.head, net.activation, net.epsilon = 0, 0, self._eps.data_ptr()
            return net
        if self.obs == 'see':
            if vision_params is None or vision is None:
                raise ValueError("a see actor's struct needs the engine's vision parameters and planes (enable_vision)")
            net = M.S2DMatchSeeNet()
            net.prm, net.vis = vision_params, vision
        else:
            net = M.S2DMatchNet()
        net.h1, net.h2, net.n_actions, net.slot_mask = self.hidden1, self.hidden2, self.n_actions, int(slot_mask)
        net.params, net.epsilon, net.table = self.params.data_ptr(), self._eps.data_ptr(), self.table.data_ptr()
        return net


def _belief_struct(actor, slot_mask, vision_params, vision, belief_params, belief, belief_mask):
    """the words of S2DMatchBeliefNet both heads share: the network, the table, the engine's vision and belief layers"""
    from . import _capi_match as M
    if vision_params is None or vision is None:
        raise ValueError("a belief actor's struct needs the engine's vision parameters and planes (enable_vision)")
    if belief_params is None or belief is None:
        raise ValueError("a belief actor's struct needs the engine's belief parameters, buffer and mask (enable_belief)")
    net = M.S2DMatchBeliefNet()
    net.h1, net.h2, net.n_actions, net.slot_mask = actor.hidden1, actor.hidden2, actor.n_actions, int(slot_mask)
    net.params, net.table = actor.params.data_ptr(), actor.table.data_ptr()
    net.prm, net.vis = vision_params, vision
    net.belief_prm, net.belief, net.belief_mask = belief_params, belief.data_ptr(), int(belief_mask)
    return net


class _MatchPolicy(_ActionTable, _Deterministic, _PackedActor):
    """what the 11v11 engine's two stochastic policies share: the row width and table width are the class's (`in_dim`,
    `table_width`); widths, K, the activation, the deterministic word and the table are checked and built alike"""

    kind = 'policy'
    _grid = _POLICY_GRID
    _what = 'policy'

    def _init_policy(self, hidden1, hidden2, n_actions, activation, device, deterministic, table):
        for name, w in (('hidden1', hidden1), ('hidden2', hidden2)):
            if int(w) not in MATCH_WIDTHS:
                raise ValueError(f'{name} must be one of {MATCH_WIDTHS}, got {w}')
        if not 1 <= int(n_actions) <= MATCH_MAX_ACTIONS:
            raise ValueError(f'n_actions must be in [1, {MATCH_MAX_ACTIONS}], got {n_actions}')
        if activation not in ('relu', 'tanh'):
            raise ValueError(f"activation must be 'relu' or 'tanh', got {activation!r}")
        self.hidden1, self.hidden2, self.n_actions, self.activation = int(hidden1), int(hidden2), int(n_actions), activation
        self._init_packed(device)
        self._init_deterministic(deterministic)
        self._init_table(table)

    @classmethod
    def _from_module(cls, policy_net, table, device, deterministic, **kwargs):
        (l1, l2, l3), act = cls._read(policy_net)
        dev = device if device is not None else l1.weight.device
        actor = cls(l1.out_features, l2.out_features, l3.out_features, activation=act, device=dev, deterministic=deterministic,
                    **kwargs)
        actor.load_from(policy_net)
        actor.set_table(table)
        return actor

    def snapshot(self, deterministic=None):
        """A frozen copy: a new actor of the same shape with its own parameters, table and deterministic word -- the league
        member a learner plays against, or an evaluation copy.  It has no module: later sync() calls do not touch it."""
        return self._frozen(type(self)(self.hidden1, self.hidden2, self.n_actions, activation=self.activation, device=self.device,
                                       deterministic=self._det_value if deterministic is None else deterministic, obs=self.obs))

    def _fill(self, net, slot_mask):
        """the words S2DMatchPolicyNet and S2DMatchSeePolicyNet share"""
        net.h1, net.h2, net.n_actions, net.slot_mask = self.hidden1, self.hidden2, self.n_actions, int(slot_mask)
        net.activation = 1 if self.activation == 'tanh' else 0
        net.params, net.deterministic, net.table = self.params.data_ptr(), self._det.data_ptr(), self.table.data_ptr()
        return net


class MatchPolicyActor(_MatchPolicy):
    """Packed parameters, the device deterministic word and the action table of a 224-H1-H2-K stochastic policy for the 11v11
    engine's policy slots (MatchEngine.set_network / set_opponent_network, s2d_match_set_policy_network in include/s2d_match.h):
    on-policy self-play (PPO / A2C with shared parameters) collected inside the cycle kernel.

    y = W3 f(W2 f(W1 x + b1) + b2) + b3 with f = ReLU or Tanh (``activation``; Tanh is SB3's default for PPO's MlpPolicy) are the
    logits of a categorical policy over the K rows of `table`, float32 [K, 3] = (command, a, b).  The kernel samples the index,
    records it (``net_index``) and its log-probability (``MatchEngine.rollout(logp=True)``); ``deterministic = True`` switches to
    the first maximum.  params, the deterministic word and table are device buffers written in place and read when the kernel
    runs, so a captured graph acts with what they hold at replay.  obs='see' is refused: the policy on see rows is a class of
    its own, MatchSeePolicyActor."""

    obs, in_dim, table_width = 'agent', MATCH_OBS_DIM, 3

    def __init__(self, hidden1=64, hidden2=64, n_actions=16, activation='tanh', device='cuda:0', deterministic=False, table=None,
                 obs='agent'):
        if obs != 'agent':
            raise ValueError(f"a MatchPolicyActor acts on agent rows only (obs='agent'), got obs={obs!r}: the policy on see rows "
                             f"is MatchSeePolicyActor")
        self._init_policy(hidden1, hidden2, n_actions, activation, device, deterministic, table)

    @classmethod
    def from_module(cls, policy_net, table, device=None, deterministic=False, obs='agent'):
        """An actor shaped like `policy_net` (224 -> H1 -> H2 -> K; the module forms StochasticActor.from_module accepts, SB3's
        ``[policy.mlp_extractor.policy_net, policy.action_net]`` among them), loaded from it, with action table `table` [K, 3].
        The activation is the module's."""
        return cls._from_module(policy_net, table, device, deterministic, obs=obs)

    def c_struct(self, slot_mask):
        """S2DMatchPolicyNet for s2d_match_set_policy_network"""
        from . import _capi_match as M
        return self._fill(M.S2DMatchPolicyNet(), slot_mask)


class MatchSeePolicyActor(_MatchPolicy):
    """MatchPolicyActor under partial observability: a 192-H1-H2-K stochastic policy on each slot's see row (MatchEngine.see)
    for the 11v11 engine's see policy slots (MatchEngine.set_network, s2d_match_set_see_policy_network in include/s2d_match.h).

    The logits are MatchPolicyActor's with 192 inputs; the sampled index chooses a row of `table`, float32 [K, 5] = (command, a,
    b, TurnNeck moment, ChangeView code), so the policy also turns the neck and changes the view width, and the cycle kernel
    steps the vision state of all 22 players.  ``MatchEngine.rollout(logp=True, see_obs=..., net_index=True)`` records what a
    PPO / A2C learner needs.  It is the engine's only network (no opponent beside it) and needs enable_vision() first.

    obs='belief': the same policy and table on each slot's belief row (MatchEngine.belief) -- head 1 of the belief network of
    include/s2d_match.h (s2d_match_set_belief_network); ``rollout(logp=True, belief_obs=..., net_index=True)`` records the rows
    it acted on.  It needs enable_belief() too."""

    obs, in_dim, table_width = 'see', MATCH_SEE_DIM, 5

    def __init__(self, hidden1=64, hidden2=64, n_actions=16, activation='tanh', device='cuda:0', deterministic=False, table=None,
                 obs='see'):
        if obs not in ('see', 'belief'):
            raise ValueError(f"a MatchSeePolicyActor acts on see rows or belief rows (obs='see' or 'belief'), got obs={obs!r}: the "
                             f"policy on agent rows is MatchPolicyActor")
        self.obs = obs
        self._init_policy(hidden1, hidden2, n_actions, activation, device, deterministic, table)

    @classmethod
    def from_module(cls, policy_net, table, device=None, deterministic=False, obs='see'):
        """An actor shaped like `policy_net` (192 -> H1 -> H2 -> K, the module forms MatchPolicyActor.from_module accepts), loaded
        from it, with action table `table` [K, 5].  The activation is the module's."""
        return cls._from_module(policy_net, table, device, deterministic, obs=obs)

    def c_struct(self, slot_mask, vision_params=None, vision=None, belief_params=None, belief=None, belief_mask=0):
        """S2DMatchSeePolicyNet for s2d_match_set_see_policy_network; it needs the engine's vision parameters and planes.
        obs='belief': S2DMatchBeliefNet (head 1), which also needs the engine's belief parameters, buffer and mask."""
        from . import _capi_match as M
        if self.obs == 'belief':
            net = _belief_struct(self, slot_mask, vision_params, vision, belief_params, belief, belief_mask)
            net.head, net.activation, net.deterministic = 1, 1 if self.activation == 'tanh' else 0, self._det.data_ptr()
            return net
        if vision_params is None or vision is None:
            raise ValueError("a see actor's struct needs the engine's vision parameters and planes (enable_vision)")
        net = self._fill(M.S2DMatchSeePolicyNet(), slot_mask)
        net.prm, net.vis = vision_params, vision
        return net
