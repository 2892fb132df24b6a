"""GtcQNetActor / GtcDeterministicActor: the fused actors of GoToCenterVecEnv.rollout_qnet / rollout_actor (s2d_gtc_rollout_qnet /
s2d_gtc_rollout_actor, include/s2d_gtc.h): 4 -> h_1 -> ... -> h_L -> A on the env's own 4-word observation, with one to five hidden
layers, every hidden width a multiple of 4 in [8, 400] and one hidden activation, ReLU, Tanh or Sigmoid -- every network the
reference's GoToCenter scripts build: SB3's DQN default [64, 64], DDPG's ``pi: [16, 8]`` and the Optuna grids
``layer_size in {8, ..., 400} x n_layers in 1..5 x {ReLU, Tanh, Sigmoid}``.

They are WideQNetActor / WideDeterministicActor (soccer2d_amd.wide_actor) with ``in_dim = 4``: one packed fp32 parameter buffer in
``nn.Sequential(...).parameters()`` order, a device epsilon, the Gaussian noise rows of the deterministic actor and the workspace
the pack kernel writes, all read when the kernels run.  Layer 1 runs over exactly its four inputs (no zero pad).
"""
from .actor import DeterministicActor, QNetActor
from .gtc import GTC_OBS_DIM
from .mlp_actor import param_count as _param_count
from .wide_actor import ACTIVATIONS, LDS_BYTES, MAX_HIDDEN, WIDE_WIDTHS, _WideShape, wide_plan  # noqa: F401  (part of this module's interface)

N_ACTIONS = 16                   # GoToCenterEnv's Discrete(16)
ACTOR_OUTPUTS = (1, 2, 3, 4)     # continuous: 1; turn mode: actor_out_size
_WAVE = 64


def param_count(hidden, n_out):
    return _param_count(hidden, n_out, GTC_OBS_DIM)


def gtc_plan(hidden, n_out):
    """(waves per workgroup, env tiles per pass, LDS bytes, workspace bytes) of a 4-hidden...-n_out network: wide_plan with input
    width 4 (ONE k-step for layer 1) and, behind a wave's output image, only the observation tile of 64 x 4 words; there is no
    prepared-episode tile"""
    return wide_plan(hidden, n_out, n_in=GTC_OBS_DIM, tail_words=_WAVE * GTC_OBS_DIM)


class _GtcShape(_WideShape):
    """_WideShape on the 4-word observation: the packed buffer's first layer, the plan and how a module is read"""

    in_dim = GTC_OBS_DIM

    @property
    def plan(self):
        """(waves per workgroup, env tiles per pass, LDS bytes, workspace bytes) of the kernel's plan for this shape"""
        return gtc_plan(self.hidden, self._outputs)

    @classmethod
    def _from(cls, module, device, **kw):
        linears, _ = cls._read(module)
        if linears[0].in_features != GTC_OBS_DIM:
            raise ValueError(f'the first layer must have in_features = {GTC_OBS_DIM} (GoToCenter\'s observation), got '
                             f'{linears[0].in_features}')
        return super()._from(module, device, **kw)


class GtcQNetActor(_GtcShape, QNetActor):
    """Packed parameters, device epsilon and workspace of a 4-h_1-...-h_L-16 Q-network for GoToCenterVecEnv.rollout_qnet
    (a discrete env).  epsilon / epsilon_tensor are QNetActor's."""

    _entry = 's2d_gtc_rollout_qnet'

    def __init__(self, hidden=(64, 64), activation='relu', device='cuda:0', epsilon=0.05):
        self.n_actions = N_ACTIONS
        self._init_shape(hidden, self.n_actions, activation, device)
        self._init_epsilon(epsilon)

    @classmethod
    def _from(cls, module, device, **kw):
        linears, act = cls._read(module)
        if linears[-1].out_features != N_ACTIONS:
            raise ValueError(f'the Q-network must have {N_ACTIONS} outputs (GoToCenter\'s Discrete({N_ACTIONS})), got '
                             f'{linears[-1].out_features}')
        if linears[0].in_features != GTC_OBS_DIM:
            raise ValueError(f'the first layer must have in_features = {GTC_OBS_DIM} (GoToCenter\'s observation), got '
                             f'{linears[0].in_features}')
        dev = device if device is not None else linears[0].weight.device
        return cls([lin.out_features for lin in linears[:-1]], activation=act, device=dev, **kw).load_from(module)

    @classmethod
    def from_module(cls, module, device=None, epsilon=0.05):
        """An actor shaped like `module` (Linear-(F-Linear) x L with in_features = 4 and 16 outputs, F = ReLU, Tanh or Sigmoid
        throughout, optionally behind a Flatten or Identity: SB3's ``model.q_net.q_net``), loaded from it."""
        return cls._from(module, device, epsilon=epsilon)


class GtcDeterministicActor(_GtcShape, DeterministicActor):
    """Packed parameters, device epsilon, Gaussian action noise and workspace of a 4-h_1-...-h_L-A tanh actor for
    GoToCenterVecEnv.rollout_actor: A = 1 on a continuous env, actor_out_size (1 .. 4) on a turn-mode one.  epsilon and the noise
    properties are DeterministicActor's."""

    _grid = dict(_WideShape._grid, tanh_head=True)
    _entry = 's2d_gtc_rollout_actor'

    def __init__(self, hidden=(16, 8), n_out=1, activation='relu', device='cuda:0', epsilon=0.0, noise_mean=None, noise_sigma=None):
        if int(n_out) not in ACTOR_OUTPUTS:
            raise ValueError(f'n_out must be the env\'s action width, 1 .. 4, got {n_out}')
        self.n_out = int(n_out)
        self._init_shape(hidden, self.n_out, activation, device)
        self._init_epsilon(epsilon)
        self._init_noise(noise_mean, noise_sigma)

    @classmethod
    def from_module(cls, module, device=None, epsilon=0.0, noise_mean=None, noise_sigma=None):
        """An actor shaped like `module` (SB3's ``model.actor.mu``: Linear-(F-Linear) x L-Tanh with in_features = 4, F = ReLU,
        Tanh or Sigmoid throughout, optionally behind a Flatten or Identity), loaded from it."""
        return cls._from(module, device, epsilon=epsilon, noise_mean=noise_mean, noise_sigma=noise_sigma)
