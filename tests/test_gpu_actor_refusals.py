"""What the seven fused-actor entry points of the reach-ball engine (s2d_rollout_qnet / _actor, their _mlp and _wide forms and
s2d_rollout_policy) refuse alike, one fault at a time: a NULL handle or net, n_steps = 0, a misaligned terminal_obs, record obs,
record action (2 bytes off; 4 bytes off on a turning engine, whose float4 rows want 16) or logp, and an engine of a mode the entry
does not take.  Each returns S2D_EINVAL with the text tests/golden/actor_refusals.json holds (actor_refusals.py) and enqueues
nothing: the arena, and a wide actor's workspace, stay bit for bit what they were."""
import ctypes as C

import pytest

import oracle as O
from actor_refusals import refused

torch = pytest.importorskip('torch')
nn = torch.nn

pytestmark = pytest.mark.gpu

MODES = {'discrete': dict(), 'cont1': dict(use_continuous_action=True, use_turning=False),
         'turn4': dict(use_continuous_action=True, use_turning=True)}
NA = {'discrete': 16, 'cont1': 1, 'turn4': 4}
T = 4


@pytest.fixture(scope='module')
def engines():
    """one 256-env engine per mode, with a record of T + 1 steps: nothing of a launch a refusal let through would leave its buffers"""
    from soccer2d_amd.engine import Engine, make_config
    out = {}
    for mode, kw in MODES.items():
        eng = Engine(256, 'cuda:0', cfg=make_config(noise=False, **dict(O.DQN_KWARGS, **kw)))
        eng.reset()
        out[mode] = (eng, eng.alloc_rollout(T + 1, terminal_obs=True, logp=True))
    return out


def _module(widths, tanh_head):
    layers = []
    for win, w in zip(widths[:-2], widths[1:-1]):
        layers += [nn.Linear(win, w), nn.ReLU()]
    layers.append(nn.Linear(widths[-2], widths[-1]))
    return nn.Sequential(*layers, *([nn.Tanh()] if tanh_head else [])).to('cuda:0')


def _actor(entry, mode):
    """the smallest network the entry's back end takes, for an engine of `mode`"""
    from soccer2d_amd.actor import DeterministicActor, QNetActor, StochasticActor
    from soccer2d_amd.mlp_actor import MlpDeterministicActor, MlpQNetActor
    from soccer2d_amd.wide_actor import WideDeterministicActor, WideQNetActor
    na = NA[mode]
    if entry == 's2d_rollout_policy':
        return StochasticActor.from_module(_module((10, 16, 16, na), False))
    cls, widths = {'s2d_rollout_qnet': (QNetActor, (10, 16, 16, na)), 's2d_rollout_actor': (DeterministicActor, (10, 16, 16, na)),
                   's2d_rollout_qnet_mlp': (MlpQNetActor, (10, 8, na)), 's2d_rollout_actor_mlp': (MlpDeterministicActor, (10, 8, na)),
                   's2d_rollout_qnet_wide': (WideQNetActor, (10, 8, na)),
                   's2d_rollout_actor_wide': (WideDeterministicActor, (10, 8, na))}[entry]
    return cls.from_module(_module(widths, 'actor' in entry))


ENTRIES = {'s2d_rollout_qnet': ('discrete',), 's2d_rollout_qnet_mlp': ('discrete',), 's2d_rollout_qnet_wide': ('discrete',),
           's2d_rollout_actor': ('cont1', 'turn4'), 's2d_rollout_actor_mlp': ('cont1', 'turn4'),
           's2d_rollout_actor_wide': ('cont1', 'turn4'), 's2d_rollout_policy': ('discrete', 'cont1', 'turn4')}


@pytest.mark.parametrize('entry', list(ENTRIES))
def test_refusals_of_the_shared_prologue(engines, entry):
    from soccer2d_amd import _capi
    policy = entry == 's2d_rollout_policy'
    for mode, (eng, out) in engines.items():
        takes = mode in ENTRIES[entry]
        # an engine of a mode the entry does not take is handed the actor of a mode it takes: the mode is the one fault
        actor = _actor(entry, mode if takes else ENTRIES[entry][0])
        net = actor.c_struct()
        fn = getattr(eng.lib, entry)
        arena = eng.arena.clone()
        workspace = actor.workspace.clone() if hasattr(actor, 'workspace') else None

        def call(h=eng._h, n_steps=T, net=C.byref(net), term=0, logp=0, **off):
            ro = _capi.S2DRollout()
            for name in ('obs', 'action', 'reward', 'done', 'result'):
                setattr(ro, name, out[name].data_ptr() + off.get(name, 0))
            args = [h, n_steps, net, C.byref(ro), C.c_void_p(out['terminal_obs'].data_ptr() + term)]
            if policy:
                args.append(C.c_void_p(out['logp'].data_ptr() + logp))
            return fn(*args, eng._stream())

        if not takes:
            refused(eng.lib, f'{entry}/{mode}/wrong engine mode', call())
        else:
            faults = [('NULL handle', dict(h=None)), ('NULL net', dict(net=None)), ('n_steps 0', dict(n_steps=0)),
                      ('terminal_obs + 2', dict(term=2)), ('record obs + 2', dict(obs=2)), ('record action + 2', dict(action=2))]
            if mode == 'turn4':
                faults.append(('record action + 4', dict(action=4)))
            if policy:
                faults.append(('logp + 2', dict(logp=2)))
            for what, kw in faults:
                refused(eng.lib, f'{entry}/{mode}/{what}', call(**kw))
        torch.cuda.synchronize()
        assert torch.equal(eng.arena, arena), (entry, mode)
        if workspace is not None:
            assert torch.equal(actor.workspace, workspace), (entry, mode)
