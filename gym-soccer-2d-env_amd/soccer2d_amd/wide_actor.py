"""WideQNetActor / WideDeterministicActor: the fused actors of Engine.rollout_qnet / Engine.rollout_actor on the streamed-weight
MLP (s2d_rollout_qnet_wide / s2d_rollout_actor_wide, S2DWideNet in include/s2d.h): 10 -> h_1 -> ... -> h_L -> A with one to five
hidden layers, every hidden width a multiple of 4 in [8, 400] and one hidden activation, ReLU, Tanh or Sigmoid.  These are the
networks the reference's scripts build by default or search over: SB3's ``DDPG("MlpPolicy", env)`` actor ``[400, 300]``, and
``layer_size in {8, ..., 400} x n_layers in 1..5 x {ReLU, Tanh, Sigmoid}`` of its Optuna samples.

They are MlpQNetActor / MlpDeterministicActor (soccer2d_amd.mlp_actor) on a wider grid.  The weights do not have to fit the
LDS: every launch first rewrites them in the matrix cores' fragment order into a workspace tensor the actor owns, and the rollout
kernel streams them from there.  The workspace belongs to one launch at a time: an actor is for one engine and one stream.  On
every shape the Mlp classes take both paths give the same bits.

SquashedGaussianActor is the third actor on the same network: Soft Actor-Critic's policy with a state-dependent log-std
(s2d_rollout_sac, Engine.rollout_sac), 10 -> h_1 -> ... -> h_L -> 2A: A means, then A raw log-std rows.
"""
import torch

from . import _capi
from .actor import ACTOR_OUTPUTS, MAX_ACTIONS, OBS_DIM, DeterministicActor, QNetActor, _Deterministic, _read_layers
from .mlp_actor import _fragments, _MlpShape, param_count  # noqa: F401  (param_count: part of this module's interface)

MAX_HIDDEN = 5
WIDE_WIDTHS = tuple(range(8, 401, 4))
ACTIVATIONS = ('relu', 'tanh', 'sigmoid')

# the plan of csrc/s2d_wide_net.h (wide_plan_lds over s2d_wide_host.h's counts and search), in 4-byte words
LDS_BYTES = 160 * 1024
_WAVE = 64
_OBS_TILE = _WAVE * OBS_DIM
_PREP_TILE = (13 + OBS_DIM + 2) * _WAVE


def wide_plan(hidden, n_out, n_in=OBS_DIM, tail_words=_OBS_TILE + _PREP_TILE):
    """(waves per workgroup, env tiles per pass, LDS bytes, workspace bytes) of an n_in-hidden...-n_out network, by the arithmetic
    of the C plan.  The workspace holds every layer's fragments (ceil(h / 16) tiles x its k-steps, ceil(n_in / 4) for layer 1 --
    3 for the 10-word observation -- and h_(l-1) / 4 after it, 64 words each) and the biases padded to their tiles.  The LDS holds
    the biases and per wave two images of `tiles` x 16 rows (pitch: the widest padded layer rounded up to 64, + 4), the output
    image and `tail_words` behind it (here the observation tile and the prepared-episode tile).  More waves go before more
    tiles: the first of (4, 4), (4, 2), (4, 1), (2, 4), ..., (1, 1) that 160 KiB hold."""
    nfrag, nbias, wmax, na16 = _fragments(hidden, n_out, n_in)
    rpitch = (wmax + 63) // 64 * 64 + 4
    shared = (nbias + 3) & ~3
    for waves in (4, 2, 1):
        for tiles in (4, 2, 1):
            wave_words = 2 * tiles * 16 * rpitch + _WAVE * (na16 + 4) + tail_words
            nbytes = (shared + waves * wave_words) * 4
            if nbytes <= LDS_BYTES:
                return waves, tiles, nbytes, (nfrag * _WAVE + nbias) * 4
    raise AssertionError('one wave with one tile fits for every shape on the grid')


def _check_shape(hidden, n_out, activation):
    hidden = tuple(int(w) for w in hidden)
    if not 1 <= len(hidden) <= MAX_HIDDEN:
        raise ValueError(f'the streamed MLP has 1 to {MAX_HIDDEN} hidden layers, got {len(hidden)}')
    for w in hidden:
        if w not in WIDE_WIDTHS:
            raise ValueError(f'every hidden width must be a multiple of 4 in [8, 400], got {w} in {list(hidden)}')
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation must be 'relu', 'tanh' or 'sigmoid', got {activation!r}")
    return hidden


class _WideShape(_MlpShape):
    """_MlpShape on the wide grid, and the workspace the pack kernel writes"""

    _grid = dict(acts=('ReLU', 'Tanh', 'Sigmoid'), hidden=(1, MAX_HIDDEN))
    _check_shape = staticmethod(_check_shape)
    _activations = ACTIVATIONS
    _struct = _capi.S2DWideNet

    def _init_shape(self, hidden, n_out, activation, device):
        super()._init_shape(hidden, n_out, activation, device)
        # torch's device allocations are 256-byte aligned (the ABI asks for 256 of the workspace)
        self.workspace = torch.zeros(self.plan[3] // 4, dtype=torch.float32, device=self.device)

    @property
    def plan(self):
        """(waves per workgroup, env tiles per pass, LDS bytes, workspace bytes) of the kernel's plan for this shape"""
        return wide_plan(self.hidden, self._outputs)

    @property
    def waves(self):
        return self.plan[0]

    def c_struct(self):
        net = super().c_struct()
        net.workspace = self.workspace.data_ptr()
        net.workspace_bytes = self.workspace.numel() * 4
        return net


class WideQNetActor(_WideShape, QNetActor):
    """Packed parameters, device epsilon and workspace of a 10-h_1-...-h_L-A Q-network (L = 1 .. 5, widths up to 400, ReLU, Tanh or
    Sigmoid) for Engine.rollout_qnet.  epsilon / epsilon_tensor are QNetActor's."""

    _entry = 's2d_rollout_qnet_wide'

    def __init__(self, hidden=(256, 256), n_actions=16, activation='relu', device='cuda:0', epsilon=0.05):
        if not 1 <= int(n_actions) <= MAX_ACTIONS:
            raise ValueError(f'n_actions must be in [1, {MAX_ACTIONS}], got {n_actions}')
        self.n_actions = int(n_actions)
        self._init_shape(hidden, self.n_actions, activation, device)
        self._init_epsilon(epsilon)

    @classmethod
    def from_module(cls, module, device=None, epsilon=0.05):
        """An actor shaped like `module` (Linear-(F-Linear) x L, F = ReLU, Tanh or Sigmoid throughout, optionally behind a
        Flatten or Identity: SB3's ``model.q_net.q_net``), loaded from it."""
        return cls._from(module, device, epsilon=epsilon)


class WideDeterministicActor(_WideShape, DeterministicActor):
    """Packed parameters, device epsilon, Gaussian action noise and workspace of a 10-h_1-...-h_L-A tanh actor (L = 1 .. 5, widths
    up to 400: SB3's default [400, 300]) for Engine.rollout_actor.  epsilon and the noise properties are DeterministicActor's."""

    _grid = dict(_WideShape._grid, tanh_head=True)
    _entry = 's2d_rollout_actor_wide'

    def __init__(self, hidden=(400, 300), n_out=1, activation='relu', device='cuda:0', epsilon=0.0, noise_mean=None,
                 noise_sigma=None):
        if int(n_out) not in ACTOR_OUTPUTS:
            raise ValueError(f'n_out must be 1 (continuous engine) or 4 (turning engine), got {n_out}')
        self.n_out = int(n_out)
        self._init_shape(hidden, self.n_out, activation, device)
        self._init_epsilon(epsilon)
        self._init_noise(noise_mean, noise_sigma)

    @classmethod
    def from_module(cls, module, device=None, epsilon=0.0, noise_mean=None, noise_sigma=None):
        """An actor shaped like `module` (SB3's ``model.actor.mu``: Linear-(F-Linear) x L-Tanh, F = ReLU, Tanh or Sigmoid
        throughout, optionally behind a Flatten or Identity), loaded from it."""
        return cls._from(module, device, epsilon=epsilon, noise_mean=noise_mean, noise_sigma=noise_sigma)


class SquashedGaussianActor(_Deterministic, _WideShape):
    """Packed parameters, the device deterministic word and the workspace of Soft Actor-Critic's squashed-Gaussian policy for
    Engine.rollout_sac (s2d_rollout_sac): 10-h_1-...-h_L-2A on the streamed-weight MLP (L = 1 .. 5, widths up to 400: SB3's
    default [256, 256]), A = 1 on a continuous engine, 4 on a turning one.  Output rows 0 .. A-1 are the means (SB3's
    ``actor.mu``), rows A .. 2A-1 the raw log-std (``actor.log_std``), clamped to [-20, 2] in the kernel.  The kernel samples
    u = mean + exp(log_std) z, records a = tanh(u) and its log-probability with SB3's tanh correction, and hands the env the
    same a.  ``deterministic = True`` switches to tanh(mean).  The parameter buffer and the deterministic word are device
    buffers written in place and read when the kernel runs, so a captured graph acts with what they hold at replay."""

    _what = 'actor'
    _entry = 's2d_rollout_sac'
    _outputs = property(lambda self: self.n_out)

    def __init__(self, hidden=(256, 256), action_dim=1, activation='relu', device='cuda:0', deterministic=False):
        if int(action_dim) not in ACTOR_OUTPUTS:
            raise ValueError(f'action_dim must be 1 (continuous engine) or 4 (turning engine), got {action_dim}')
        self.action_dim = int(action_dim)
        self.n_out = 2 * self.action_dim
        self._init_shape(hidden, self.n_out, activation, device)
        self._init_deterministic(deterministic)
        self._source = None

    # ---- how the two module forms read: (the flat buffer's tensors in order, hidden widths, output width, activation)
    @classmethod
    def _read_source(cls, source):
        if len(source) == 1:
            linears, act = _read_layers(source[0], **cls._grid)
            heads = [(linears[-1].weight,), (linears[-1].bias,)]
            n_out = linears[-1].out_features
        else:
            latent_pi, mu, log_std = source
            linears, act = _read_layers([latent_pi, mu], **dict(cls._grid, many=True))
            if not isinstance(log_std, torch.nn.Linear) or (log_std.in_features, log_std.out_features) != (mu.in_features, mu.out_features):
                raise ValueError(f'log_std must be a Linear({mu.in_features}, {mu.out_features}) like mu, got {log_std}')
            heads = [(mu.weight, log_std.weight), (mu.bias, log_std.bias)]
            n_out = 2 * mu.out_features
        if n_out % 2 or n_out // 2 not in ACTOR_OUTPUTS:
            raise ValueError(f'the actor\'s output layer must have 2 A outputs (A means, then A log-std rows) with A = 1 (continuous '
                             f'engine) or 4 (turning engine), got {n_out}')
        tensors = []
        for lin in linears[:-1]:
            tensors += [lin.weight, lin.bias]
        tensors += list(heads[0]) + list(heads[1])
        if any(t is None for t in tensors):
            raise ValueError('every nn.Linear of the actor needs a bias')
        return tensors, tuple(lin.out_features for lin in linears[:-1]), n_out, act, linears[0].in_features

    @classmethod
    def _from_source(cls, source, device, deterministic):
        tensors, hidden, n_out, act, n_in = cls._read_source(source)
        if n_in != OBS_DIM:
            raise ValueError(f'the actor must take the {OBS_DIM}-word observation, got an input width of {n_in}')
        actor = cls(hidden, n_out // 2, activation=act, device=device if device is not None else tensors[0].device,
                    deterministic=deterministic)
        actor._source = source
        return actor.sync()

    @classmethod
    def from_module(cls, net, device=None, deterministic=False):
        """An actor shaped like `net` (Linear-(F-Linear) x L ending in Linear(h_L, 2A): means, then log-std rows; F = ReLU, Tanh
        or Sigmoid throughout, optionally behind a Flatten or Identity), loaded from it."""
        return cls._from_source((net,), device, deterministic)

    @classmethod
    def from_modules(cls, latent_pi, mu, log_std, device=None, deterministic=False):
        """An actor shaped like SB3's SAC triple ``model.actor.latent_pi`` (Linear-F x L), ``model.actor.mu`` and
        ``model.actor.log_std`` (both Linear(h_L, A)), loaded from them: the same flat buffer as from_module on the stacked
        network."""
        return cls._from_source((latent_pi, mu, log_std), device, deterministic)

    def load_from(self, *source):
        """Validate a module (or the triple latent_pi, mu, log_std) against this actor, remember it and pack it (sync())."""
        self._source = tuple(source)
        return self.sync()

    def sync(self):
        """Copy the loaded modules' current parameters into the packed buffer: one device copy, no allocation of the buffers the
        kernel reads (capturable)."""
        if self._source is None:
            raise ValueError('no module loaded (from_module / from_modules)')
        tensors, hidden, n_out, act, _ = self._read_source(self._source)
        if act != self.activation:
            raise ValueError(f'the modules\' activation is {act}, this actor\'s {self.activation}')
        if (hidden, n_out) != (self.hidden, self.n_out):
            raise ValueError(self._shape_error.format(what=self._what, got=list(hidden) + [n_out], want=list(self.hidden) + [self.n_out]))
        with torch.no_grad():
            torch.cat([t.detach().reshape(-1).to(self.device, torch.float32) for t in tensors], out=self.params)
        return self

    def snapshot(self, deterministic=None):
        """A frozen copy: a new actor of the same shape with its own parameters, workspace and deterministic word (an evaluation
        copy).  It has no module: later sync() calls of the original do not touch it."""
        return self._frozen(type(self)(self.hidden, self.action_dim, activation=self.activation, device=self.device,
                                       deterministic=self._det_value if deterministic is None else deterministic))

    def c_struct(self):
        net = _capi.S2DWideNet()
        net.n_hidden = len(self.hidden)
        for l in range(len(net.hidden)):
            net.hidden[l] = self.hidden[l] if l < len(self.hidden) else 0
        net.n_out = self.n_out
        net.activation = ACTIVATIONS.index(self.activation)
        net.noise_kind = 0
        net.params = self.params.data_ptr()
        net.epsilon = None
        net.noise = None
        net.workspace = self.workspace.data_ptr()
        net.workspace_bytes = self.workspace.numel() * 4
        return net
