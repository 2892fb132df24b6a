"""WideQNetActor / WideDeterministicActor: the fused actors of Engine.rollout_qnet / Engine.rollout_actor on the streamed-weight
MLP (s2d_rollout_qnet_wide / s2d_rollout_actor_wide, S2DWideNet in include/s2d.h): 10 -> h_1 -> ... -> h_L -> A with one to five
hidden layers, every hidden width a multiple of 4 in [8, 400] and one hidden activation, ReLU, Tanh or Sigmoid.  These are the
networks the reference's scripts build by default or search over: SB3's ``DDPG("MlpPolicy", env)`` actor ``[400, 300]``, and
``layer_size in {8, ..., 400} x n_layers in 1..5 x {ReLU, Tanh, Sigmoid}`` of its Optuna samples.

They are MlpQNetActor / MlpDeterministicActor (soccer2d_amd.mlp_actor) on a wider grid.  The weights do not have to fit the
LDS: every launch first rewrites them in the matrix cores' fragment order into a workspace tensor the actor owns, and the rollout
kernel streams them from there.  The workspace belongs to one launch at a time: an actor is for one engine and one stream.  On
every shape the Mlp classes take both paths give the same bits.
"""
import torch

from . import _capi
from .actor import ACTOR_OUTPUTS, MAX_ACTIONS, OBS_DIM, DeterministicActor, QNetActor
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
