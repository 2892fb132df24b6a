"""MlpQNetActor / MlpDeterministicActor: the fused actors of Engine.rollout_qnet / Engine.rollout_actor on a general MLP
(s2d_rollout_qnet_mlp / s2d_rollout_actor_mlp, S2DMlpNet in include/s2d.h): 10 -> h_1 -> ... -> h_L -> A with one to four hidden
layers, every hidden width a multiple of 8 in [8, 128] and one hidden activation, ReLU or Tanh.  These are the networks SB3
builds from ``policy_kwargs=dict(net_arch=[128, 64, 32, 16], activation_fn=nn.Tanh)`` (``model.q_net.q_net``) or
``dict(net_arch=dict(pi=[16, 8], qf=[...]))`` (``model.actor.mu``).

They are QNetActor / DeterministicActor (soccer2d_amd.actor) with another shape: one packed fp32 parameter buffer in
``nn.Sequential(Linear, F, ..., Linear).parameters()`` order, a device epsilon and (the deterministic actor) the Gaussian noise
rows, all written in place and read when the kernel runs.  The two-layer classes stay what they are; for a 10-H1-H2-A ReLU
network with widths that are multiples of 16 both paths give the same bits.
"""
from . import _capi
from .actor import ACTOR_OUTPUTS, MAX_ACTIONS, OBS_DIM, DeterministicActor, QNetActor, _PackedActor

MAX_HIDDEN = 4
MLP_WIDTHS = tuple(range(8, 129, 8))
ACTIVATIONS = ('relu', 'tanh')

# the LDS plan of csrc/s2d_mlp_net.h (mlp_plan_lds), in 4-byte words
LDS_BYTES = 160 * 1024
_WAVE = 64
_WAVES_PER_BLOCK = 4
_OBS_TILE = _WAVE * OBS_DIM
_PREP_TILE = (13 + OBS_DIM + 2) * _WAVE


def _fragments(hidden, n_out, n_in=OBS_DIM):
    """(fragments, bias words, widest padded layer, n_out rounded up to 16) of an n_in-hidden...-n_out network, as the C plans
    count them (csrc/s2d_wide_pack.hip s2d_internal_wide_counts): ceil(h / 16) tiles of 16 rows x the layer's k-steps
    (ceil(n_in / 4) for layer 1: 3 for the 10-word observation; h_(l-1) / 4 after it), the biases padded to their tiles"""
    na16 = (n_out + 15) // 16 * 16
    nfrag = nbias = wmax = 0
    ksteps = (n_in + 3) // 4
    for w in hidden:
        m16 = (w + 15) // 16
        nfrag += m16 * ksteps
        nbias += 16 * m16
        wmax = max(wmax, 16 * m16)
        ksteps = w // 4
    return nfrag + (na16 // 16) * ksteps, nbias + na16, wmax, na16


def lds_plan(hidden, n_out):
    """(waves per workgroup, LDS bytes) of a 10-hidden...-n_out network, by the arithmetic of the C plan: the fragments of every
    layer (ceil(h / 16) tiles of 16 rows x its k-steps, 3 for layer 1, h_(l-1) / 4 after it), the biases padded to their tiles,
    and per wave two hidden images, the output image, the observation tile and the prepared-episode tile; as many waves of
    4 / 2 / 1 as 160 KiB hold.  waves = None: not even one wave fits (bytes = what one wave would need)."""
    nfrag, nbias, wmax, na16 = _fragments(hidden, n_out)
    pitch = (wmax + 63) // 64 * 64 + 4
    shared = (nfrag * _WAVE + nbias + 3) & ~3
    wave_words = 2 * 16 * pitch + _WAVE * (na16 + 4) + _OBS_TILE + _PREP_TILE
    waves = _WAVES_PER_BLOCK
    while waves > 1 and (shared + waves * wave_words) * 4 > LDS_BYTES:
        waves //= 2
    nbytes = (shared + waves * wave_words) * 4
    return (waves if nbytes <= LDS_BYTES else None), nbytes


def _check_shape(hidden, n_out, activation):
    hidden = tuple(int(w) for w in hidden)
    if not 1 <= len(hidden) <= MAX_HIDDEN:
        raise ValueError(f'the fused MLP has 1 to {MAX_HIDDEN} hidden layers, got {len(hidden)}')
    for w in hidden:
        if w not in MLP_WIDTHS:
            raise ValueError(f'every hidden width must be a multiple of 8 in [8, 128] (the weights live in LDS), got {w} in '
                             f'{list(hidden)}')
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation must be 'relu' or 'tanh', got {activation!r}")
    waves, nbytes = lds_plan(hidden, int(n_out))
    if waves is None:
        raise ValueError(f'the network 10-{"-".join(map(str, hidden))}-{n_out} needs {nbytes} bytes of LDS for its fragments and '
                         f'one wave\'s images; a workgroup has {LDS_BYTES}')
    return hidden


def param_count(hidden, n_out, n_in=OBS_DIM):
    """parameters of an n_in-hidden...-n_out network (nn.Sequential order: every layer's weights, then its biases)"""
    n, win = 0, n_in
    for w in tuple(hidden) + (n_out,):
        n += w * win + w
        win = w
    return n


class _MlpShape(_PackedActor):
    """What the two MLP actors share beyond their two-layer base classes: the shape, the packed buffer's layout, how a module
    is read and the C struct.  wide_actor has another grid (`_grid`, `_check_shape`, `_activations`, `_struct`)."""

    _grid = dict(acts=('ReLU', 'Tanh'), hidden=(1, MAX_HIDDEN))
    _shape_error = _PackedActor._shape_error
    _check_shape = staticmethod(_check_shape)
    _activations = ACTIVATIONS
    _struct = _capi.S2DMlpNet

    def _init_shape(self, hidden, n_out, activation, device):
        self.hidden = self._check_shape(hidden, n_out, activation)
        self.activation = activation
        self._init_packed(device)

    @classmethod
    def _from(cls, module, device, **kw):
        """an actor shaped like `module`, loaded from it (from_module)"""
        linears, act = cls._read(module)
        dev = device if device is not None else linears[0].weight.device
        actor = cls([lin.out_features for lin in linears[:-1]], linears[-1].out_features, activation=act, device=dev, **kw)
        return actor.load_from(module)

    def _widths(self):
        return self.hidden + (self._outputs,)

    @property
    def waves(self):
        """waves per workgroup of the kernel's LDS plan for this shape"""
        return lds_plan(self.hidden, self._outputs)[0]

    def c_struct(self):
        net = self._struct()
        net.n_hidden = len(self.hidden)
        for l in range(len(net.hidden)):
            net.hidden[l] = self.hidden[l] if l < len(self.hidden) else 0
        net.n_out = self._outputs
        net.activation = self._activations.index(self.activation)
        net.noise_kind = self.noise_kind if self._has_noise else 0
        net.params = self.params.data_ptr()
        net.epsilon = self._eps.data_ptr()
        net.noise = self._noise.data_ptr() if self._has_noise else None
        return net


class MlpQNetActor(_MlpShape, QNetActor):
    """Packed parameters + device epsilon of a 10-h_1-...-h_L-A Q-network (L = 1 .. 4, ReLU or Tanh) for Engine.rollout_qnet.
    epsilon / epsilon_tensor are QNetActor's."""

    _entry = 's2d_rollout_qnet_mlp'

    def __init__(self, hidden=(64, 64), n_actions=16, activation='relu', device='cuda:0', epsilon=0.05):
        if not 1 <= int(n_actions) <= MAX_ACTIONS:
            raise ValueError(f'n_actions must be in [1, {MAX_ACTIONS}], got {n_actions}')
        self.n_actions = int(n_actions)
        self._init_shape(hidden, self.n_actions, activation, device)
        self._init_epsilon(epsilon)

    @classmethod
    def from_module(cls, module, device=None, epsilon=0.05):
        """An actor shaped like `module` (Linear-(F-Linear) x L, F = ReLU or Tanh throughout, optionally behind a Flatten or
        Identity: SB3's ``model.q_net.q_net``), loaded from it."""
        return cls._from(module, device, epsilon=epsilon)


class MlpDeterministicActor(_MlpShape, DeterministicActor):
    """Packed parameters, device epsilon and Gaussian action noise of a 10-h_1-...-h_L-A tanh actor (L = 1 .. 4, ReLU or Tanh
    between the layers) for Engine.rollout_actor.  epsilon and the noise properties are DeterministicActor's."""

    _grid = dict(_MlpShape._grid, tanh_head=True)
    _entry = 's2d_rollout_actor_mlp'

    def __init__(self, hidden=(64, 64), n_out=1, activation='relu', device='cuda:0', epsilon=0.0, noise_mean=None,
                 noise_sigma=None):
        if int(n_out) not in ACTOR_OUTPUTS:
            raise ValueError(f'n_out must be 1 (continuous engine) or 4 (turning engine), got {n_out}')
        self.n_out = int(n_out)
        self._init_shape(hidden, self.n_out, activation, device)
        self._init_epsilon(epsilon)
        self._init_noise(noise_mean, noise_sigma)

    @classmethod
    def from_module(cls, module, device=None, epsilon=0.0, noise_mean=None, noise_sigma=None):
        """An actor shaped like `module` (SB3's ``model.actor.mu``: Linear-(F-Linear) x L-Tanh, F = ReLU or Tanh throughout,
        optionally behind a Flatten or Identity), loaded from it."""
        return cls._from(module, device, epsilon=epsilon, noise_mean=noise_mean, noise_sigma=noise_sigma)
