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
import torch

from . import _capi
from .actor import _NO_OPS, ACTOR_OUTPUTS, MAX_ACTIONS, OBS_DIM, DeterministicActor, QNetActor

MAX_HIDDEN = 4
MLP_WIDTHS = tuple(range(8, 129, 8))
ACTIVATIONS = ('relu', 'tanh')

# the LDS plan of csrc/s2d_mlp_net.h (mlp_plan_lds), in 4-byte words
LDS_BYTES = 160 * 1024
_WAVE = 64
_WAVES_PER_BLOCK = 4
_OBS_TILE = _WAVE * OBS_DIM
_PREP_TILE = (13 + OBS_DIM + 2) * _WAVE


def lds_plan(hidden, n_out):
    """(waves per workgroup, LDS bytes) of a 10-hidden...-n_out network, by the arithmetic of the C plan: the fragments of every
    layer (ceil(h / 16) tiles of 16 rows x its k-steps, 3 for layer 1, h_(l-1) / 4 after it), the biases padded to their tiles,
    and per wave two hidden images, the output image, the observation tile and the prepared-episode tile; as many waves of
    4 / 2 / 1 as 160 KiB hold.  waves = None: not even one wave fits (bytes = what one wave would need)."""
    na16 = (n_out + 15) // 16 * 16
    nfrag = nbias = wmax = 0
    ksteps = 3
    for w in hidden:
        m16 = (w + 15) // 16
        nfrag += m16 * ksteps
        nbias += 16 * m16
        wmax = max(wmax, 16 * m16)
        ksteps = w // 4
    nfrag += (na16 // 16) * ksteps
    nbias += na16
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


def param_count(hidden, n_out):
    n, win = 0, OBS_DIM
    for w in tuple(hidden) + (n_out,):
        n += w * win + w
        win = w
    return n


def _mlp_layers(module, tanh_head=False):
    """(the nn.Linear layers in order, activation name) of a Linear-(F-Linear) x L module, F = ReLU or Tanh, the same throughout;
    with tanh_head=True the module must end in one more Tanh (the deterministic actor's head).  Leaf modules are read in
    registration order; Identity / Flatten are skipped; anything else is refused: the kernel would silently act with a
    different function."""
    leaves = [m for m in module.modules() if not any(True for _ in m.children()) and not isinstance(m, _NO_OPS)]
    kinds = ['Linear' if isinstance(m, torch.nn.Linear) else 'ReLU' if isinstance(m, torch.nn.ReLU)
             else 'Tanh' if isinstance(m, torch.nn.Tanh) else type(m).__name__ for m in leaves]
    what = 'actor' if tanh_head else 'Q-network'
    form = 'Linear-(F-Linear) x L' + ('-Tanh' if tanh_head else '') + f', L = 1 .. {MAX_HIDDEN} hidden layers, F = ReLU or Tanh'
    got = '-'.join(kinds) or 'nothing'
    body = kinds
    if tanh_head:
        if not kinds or kinds[-1] != 'Tanh':
            raise ValueError(f'the actor must end in a Tanh ({form}), got {got}')
        body = kinds[:-1]
    if len(body) % 2 == 0 or any(k != 'Linear' for k in body[0::2]):
        raise ValueError(f'the {what} must be {form}, got {got}')
    acts = set(body[1::2])
    n_hidden = len(body) // 2
    if not 1 <= n_hidden <= MAX_HIDDEN:
        raise ValueError(f'the {what} must have 1 to {MAX_HIDDEN} hidden layers ({form}), got {n_hidden}: {got}')
    if len(acts) > 1 and acts <= {'ReLU', 'Tanh'}:
        raise ValueError(f'the {what} must use one activation throughout, ReLU or Tanh, not a mix ({form}), got {got}')
    if not acts <= {'ReLU', 'Tanh'}:
        raise ValueError(f'the hidden activation must be ReLU or Tanh ({form}), got {got}')
    linears = leaves[0:len(body):2]
    for lin in linears:
        if lin.bias is None:
            raise ValueError(f'every nn.Linear of the {what} needs a bias')
    return linears, acts.pop().lower()


class _MlpShape:
    """What the two MLP actors share beyond their two-layer base classes: the shape, the packed buffer's layout, loading from
    a module and the C struct."""

    _tanh_head = False
    _what = 'Q-network'
    _layers = staticmethod(_mlp_layers)     # how a module is read: the grid of layers and activations (wide_actor has another)

    def _init_shape(self, hidden, n_out, activation, device):
        self.hidden = _check_shape(hidden, n_out, activation)
        self.activation = activation
        self.device = torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        # torch's device allocations are 256-byte aligned (the ABI asks for 16)
        self.params = torch.zeros(param_count(self.hidden, n_out), dtype=torch.float32, device=self.device)
        self._eps = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._eps_value = None
        self._module = None

    @property
    def _outputs(self):
        return self.n_out if self._tanh_head else self.n_actions

    @property
    def waves(self):
        """waves per workgroup of the kernel's LDS plan for this shape"""
        return lds_plan(self.hidden, self._outputs)[0]

    def shapes(self):
        out, win = [], OBS_DIM
        for w in self.hidden + (self._outputs,):
            out += [(w, win), (w,)]
            win = w
        return tuple(out)

    def load_from(self, module):
        """Validate `module`'s shapes and activation against this actor, remember it, and pack its parameters (sync())."""
        linears, act = self._layers(module, self._tanh_head)
        if act != self.activation:
            raise ValueError(f'the {self._what}\'s activation is {act}, the actor\'s {self.activation}')
        got = []
        for lin in linears:
            got += [tuple(lin.weight.shape), tuple(lin.bias.shape)]
        if tuple(got) != self.shapes():
            raise ValueError(f'{self._what} shapes {got} do not match the actor {list(self.shapes())}')
        self._module = module
        self.sync()
        return self

    def sync(self):
        """Copy the loaded module's current parameters into the packed buffer: one device copy, no allocation (capturable)."""
        if self._module is None:
            raise ValueError('no module loaded (load_from)')
        srcs = []
        for lin in self._layers(self._module, self._tanh_head)[0]:
            srcs += [lin.weight.detach().reshape(-1), lin.bias.detach().reshape(-1)]
        with torch.no_grad():
            torch.cat([s.to(self.device, torch.float32) for s in srcs], out=self.params)
        return self

    def c_struct(self):
        net = _capi.S2DMlpNet()
        net.n_hidden = len(self.hidden)
        for l in range(MAX_HIDDEN):
            net.hidden[l] = self.hidden[l] if l < len(self.hidden) else 0
        net.n_out = self._outputs
        net.activation = ACTIVATIONS.index(self.activation)
        net.noise_kind = self.noise_kind if self._tanh_head else 0
        net.params = self.params.data_ptr()
        net.epsilon = self._eps.data_ptr()
        net.noise = self._noise.data_ptr() if self._tanh_head else None
        return net


class MlpQNetActor(_MlpShape, QNetActor):
    """Packed parameters + device epsilon of a 10-h_1-...-h_L-A Q-network (L = 1 .. 4, ReLU or Tanh) for Engine.rollout_qnet.
    epsilon / epsilon_tensor are QNetActor's."""

    def __init__(self, hidden=(64, 64), n_actions=16, activation='relu', device='cuda:0', epsilon=0.05):
        if not 1 <= int(n_actions) <= MAX_ACTIONS:
            raise ValueError(f'n_actions must be in [1, {MAX_ACTIONS}], got {n_actions}')
        self.n_actions = int(n_actions)
        self._init_shape(hidden, self.n_actions, activation, device)
        self.epsilon = epsilon

    @classmethod
    def from_module(cls, module, device=None, epsilon=0.05):
        """An actor shaped like `module` (Linear-(F-Linear) x L, F = ReLU or Tanh throughout, optionally behind a Flatten or
        Identity: SB3's ``model.q_net.q_net``), loaded from it."""
        linears, act = _mlp_layers(module)
        dev = device if device is not None else linears[0].weight.device
        actor = cls([lin.out_features for lin in linears[:-1]], linears[-1].out_features, activation=act, device=dev,
                    epsilon=epsilon)
        actor.load_from(module)
        return actor


class MlpDeterministicActor(_MlpShape, DeterministicActor):
    """Packed parameters, device epsilon and Gaussian action noise of a 10-h_1-...-h_L-A tanh actor (L = 1 .. 4, ReLU or Tanh
    between the layers) for Engine.rollout_actor.  epsilon and the noise properties are DeterministicActor's."""

    _tanh_head = True
    _what = 'actor'

    def __init__(self, hidden=(64, 64), n_out=1, activation='relu', device='cuda:0', epsilon=0.0, noise_mean=None,
                 noise_sigma=None):
        if int(n_out) not in ACTOR_OUTPUTS:
            raise ValueError(f'n_out must be 1 (continuous engine) or 4 (turning engine), got {n_out}')
        self.n_out = int(n_out)
        self._init_shape(hidden, self.n_out, activation, device)
        self._noise = torch.zeros(2, self.n_out, dtype=torch.float32, device=self.device)   # [mu; sigma]
        self._sigma = None
        self.epsilon = epsilon
        self.noise_mean = 0.0 if noise_mean is None else noise_mean
        self.noise_sigma = noise_sigma

    @classmethod
    def from_module(cls, module, device=None, epsilon=0.0, noise_mean=None, noise_sigma=None):
        """An actor shaped like `module` (SB3's ``model.actor.mu``: Linear-(F-Linear) x L-Tanh, F = ReLU or Tanh throughout,
        optionally behind a Flatten or Identity), loaded from it."""
        linears, act = _mlp_layers(module, tanh_head=True)
        dev = device if device is not None else linears[0].weight.device
        actor = cls([lin.out_features for lin in linears[:-1]], linears[-1].out_features, activation=act, device=dev,
                    epsilon=epsilon, noise_mean=noise_mean, noise_sigma=noise_sigma)
        actor.load_from(module)
        return actor
