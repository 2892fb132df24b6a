"""CPU check of the learners' host path in csrc/s2d_learn.hip: a table of bad calls to every s2d_learn* step / grad entry point,
each of which must return S2D_EINVAL with the FULL text below in s2d_last_error().  The table holds every refusal of the host path
at least once and rows with two faults at once, which pin the order of the checks.  The pointers are aligned fake integers: the
host path never dereferences a device pointer, and a refused call launches nothing."""
import ctypes as C
import types

import pytest

A0, STEP = 0x10000000, 0x1000000            # fake device addresses: 256-byte aligned, 16 MiB apart


def addr(i):
    return A0 + i * STEP


def _net(_capi, n_in, hidden, n_out, params=0, workspace=0):
    s = _capi.S2DLearnNet()
    s.n_in, s.n_hidden, s.n_out, s.activation = n_in, len(hidden), n_out, 0
    for l, w in enumerate(hidden):
        s.hidden[l] = w
    s.params, s.workspace = params, workspace
    return s


def _state(_capi, loss_kind):
    st = _capi.S2DLearnState()
    st.m, st.v, st.grad, st.hyper, st.stats, st.error, st.loss_kind = addr(2), addr(3), addr(4), addr(5), addr(6), addr(7), loss_kind
    return st


def _ref(x):
    return C.byref(x) if x is not None else None


# one good call per family: the names a row's edits address, and the argument list made of them
def q_call(_capi, lib):
    c = types.SimpleNamespace(batch=64, net=_net(_capi, 10, (16,), 4, addr(0), addr(1)), st=_state(_capi, 1), obs=addr(8), action=addr(9),
                              target=addr(10), weight=0, out_td_abs=0, out_q=0)
    c.net.workspace_bytes = lib.s2d_learn_workspace_bytes(C.byref(c.net), 64)
    c.args = lambda: (c.batch, _ref(c.net), _ref(c.st), c.obs, c.action, c.target, c.weight, c.out_td_abs, c.out_q, None)
    return c


def critic_call(_capi, lib):
    c = q_call(_capi, lib)
    c.net, c.st, c.action_dim = _net(_capi, 12, (16,), 1, addr(0), addr(1)), _state(_capi, 2), 2
    c.net.workspace_bytes = lib.s2d_learn_workspace_bytes(C.byref(c.net), 64)
    c.args = lambda: (c.batch, _ref(c.net), _ref(c.st), c.obs, c.action_dim, c.action, c.target, c.weight, c.out_td_abs, c.out_q, None)
    return c


def actor_call(_capi, lib):
    c = types.SimpleNamespace(batch=64, actor=_net(_capi, 10, (16,), 2, addr(0), addr(1)), st=_state(_capi, 0),
                              critic=_net(_capi, 12, (16,), 1, addr(11)), obs=addr(8), out_action=0, out_q=0)
    c.actor.workspace_bytes = lib.s2d_learn_actor_workspace_bytes(C.byref(c.actor), C.byref(c.critic), 64)
    c.args = lambda: (c.batch, _ref(c.actor), _ref(c.st), _ref(c.critic), c.obs, c.out_action, c.out_q, None)
    return c


def sac_call(_capi, lib):
    c = types.SimpleNamespace(batch=64, actor=_net(_capi, 10, (16,), 4, addr(0), addr(1)), st=_state(_capi, 0),
                              critic1=_net(_capi, 12, (16,), 1, addr(11)), critic2=_net(_capi, 12, (8,), 1, addr(12)), obs=addr(8),
                              alpha=addr(13), alpha_state=_capi.S2DLearnSacAlpha(), draws=addr(14), out_action=0, out_logp=0, out_q=0)
    t = c.alpha_state
    t.log_alpha, t.m_v, t.hyper, t.stats, t.target_entropy = addr(15), addr(16), addr(17), addr(18), -2.0
    c.actor.workspace_bytes = lib.s2d_learn_sac_workspace_bytes(C.byref(c.actor), C.byref(c.critic1), C.byref(c.critic2), 64)
    c.args = lambda: (c.batch, _ref(c.actor), _ref(c.st), _ref(c.critic1), _ref(c.critic2), c.obs, c.alpha, _ref(c.alpha_state), c.draws, 7,
                      c.out_action, c.out_logp, c.out_q, None)
    return c


def ppo_call(_capi, lib):
    q, b = _capi.S2DLearnPPO(), _capi.S2DLearnPPOBatch()
    q.pi, q.vf, q.head, q.normalize_advantage = _net(_capi, 10, (16,), 4), _net(_capi, 10, (16,), 1), 0, 1
    q.params, q.workspace, q.m, q.v, q.grad, q.hyper, q.stats, q.error = (addr(i) for i in range(8))
    q.workspace_bytes = lib.s2d_learn_ppo_workspace_bytes(C.byref(q.pi), C.byref(q.vf), 0, 64)
    b.rows, b.batch, b.obs, b.action, b.logp_old, b.advantage, b.ret = 128, 64, addr(8), addr(9), addr(10), addr(11), addr(12)
    c = types.SimpleNamespace(q=q, b=b)
    c.args = lambda: (_ref(c.q), _ref(c.b), None)
    return c


FAMILIES = {'q': (q_call, ('s2d_learn_q', 's2d_learn_q_grad')), 'critic': (critic_call, ('s2d_learn_critic', 's2d_learn_critic_grad')),
            'actor': (actor_call, ('s2d_learn_actor', 's2d_learn_actor_grad')),
            'sac': (sac_call, ('s2d_learn_sac_actor', 's2d_learn_sac_actor_grad')), 'ppo': (ppo_call, ('s2d_learn_ppo', 's2d_learn_ppo_grad'))}

SHAPE = (({'n_in': 0}, 'n_in must be in [1, 256]'), ({'n_in': 257}, 'n_in must be in [1, 256]'),
         ({'n_hidden': 0}, 'n_hidden must be in [1, 4]'), ({'n_hidden': 5}, 'n_hidden must be in [1, 4]'),
         ({'hidden.0': 12}, 'hidden widths must be multiples of 8 in [8, 256], and 0 past n_hidden'),
         ({'hidden.0': 264}, 'hidden widths must be multiples of 8 in [8, 256], and 0 past n_hidden'),
         ({'hidden.1': 8}, 'hidden widths must be multiples of 8 in [8, 256], and 0 past n_hidden'),
         ({'n_out': 0}, 'n_out must be in [1, 64]'), ({'n_out': 65}, 'n_out must be in [1, 64]'),
         ({'activation': 3}, 'activation must be 0 (ReLU), 1 (Tanh) or 2 (Sigmoid)'),
         ({'activation': -1}, 'activation must be 0 (ReLU), 1 (Tanh) or 2 (Sigmoid)'))


def shape_rows(family, net, prefix):
    """every refusal of one network's shape, with the prefix the entry point gives that network"""
    return [(family, {f'{net}.{k}': v for k, v in edit.items()}, prefix + text, None) for edit, text in SHAPE]


BATCH = 'batch must be in [1, 2^31 - 1]'
NO_OVERLAP = 'params, m, v, grad and the workspace must not overlap one another'
ACTOR_NO_OVERLAP = "the actor's params, m, v, grad and workspace must not overlap one another or the critic's params"
STATE = 'state: grad (16 bytes), hyper, stats and error (4 bytes) must be non-NULL, aligned device pointers'
ACTOR_STATE = 'state: grad (16 bytes), hyper, stats (4 bytes) must be non-NULL, aligned device pointers'
M_V = 'state: m and v must be non-NULL, 16-byte aligned device pointers'
ARRAYS = 'obs, action and target must be non-NULL, 4-byte aligned device pointers'
OPTIONAL = 'weight, out_td_abs and out_q must be 4-byte aligned device pointers (or NULL)'
OBS = 'obs must be a non-NULL, 4-byte aligned device pointer'
SAC_MINE = "alpha, draws and alpha_state's log_alpha, m_v, hyper and stats must not overlap one another"
SAC_OTHER = ("alpha, draws and alpha_state's arrays must not overlap the actor's params, m, v, grad or workspace, a critic's params or an "
             'output')
SAC_ALPHA_STATE = 'alpha_state: log_alpha, m_v, hyper and stats must be non-NULL, 4-byte aligned device pointers'
SAC_OUTS = 'out_action, out_logp and out_q must be 4-byte aligned device pointers (or NULL)'
PPO_STATE = 'grad (16 bytes), hyper, stats and error (4 bytes) must be non-NULL, aligned device pointers'
PPO_ARRAYS = 'obs, action, logp_old, advantage and ret must be non-NULL, 4-byte aligned device pointers'
PPO_OPTIONAL = 'index, out_logp and out_value must be 4-byte aligned device pointers (or NULL)'


def params_text(name):
    return f'{name}params must be a non-NULL, 16-byte aligned device pointer'


def workspace_text(name):
    return f'{name}workspace must be a non-NULL, 256-byte aligned device pointer'


def bytes_text(name, have, need, fn):
    return f"{name}workspace_bytes is {have}, a batch of 64 needs {need} ({fn}: batch is above the workspace's max_batch)"


# (family, {dotted name: value}, the text behind '<entry point>: ', the one entry point the row is for or None: both)
ROWS = (
    # ---------------------------------------------------------------------------------------------------- s2d_learn_q[_grad]
    [('q', {'net': None}, 'net and state must be non-NULL', None), ('q', {'st': None}, 'net and state must be non-NULL', None)]
    + shape_rows('q', 'net', 'net: ')
    + [('q', {'st.loss_kind': 2}, 'state: loss_kind must be 0 (MSE) or 1 (Huber)', None),
       ('q', {'st.loss_kind': -1}, 'state: loss_kind must be 0 (MSE) or 1 (Huber)', None),
       ('q', {'batch': 0}, BATCH, None), ('q', {'batch': 2 ** 31}, BATCH, None),
       ('q', {'net.params': 0}, params_text('net: '), None), ('q', {'net.params': addr(0) + 8}, params_text('net: '), None),
       ('q', {'net.workspace': 0}, workspace_text('net: '), None), ('q', {'net.workspace': addr(1) + 128}, workspace_text('net: '), None),
       ('q', {'st.grad': 0}, STATE, None), ('q', {'st.grad': addr(4) + 4}, STATE, None), ('q', {'st.hyper': 0}, STATE, None),
       ('q', {'st.hyper': addr(5) + 2}, STATE, None), ('q', {'st.stats': 0}, STATE, None), ('q', {'st.stats': addr(6) + 1}, STATE, None),
       ('q', {'st.error': 0}, STATE, None), ('q', {'st.error': addr(7) + 2}, STATE, None),
       ('q', {'st.m': 0}, M_V, 's2d_learn_q'), ('q', {'st.v': 0}, M_V, 's2d_learn_q'), ('q', {'st.m': addr(2) + 4}, M_V, 's2d_learn_q'),
       ('q', {'st.v': addr(3) + 8}, M_V, 's2d_learn_q'),
       ('q', {'obs': 0}, ARRAYS, None), ('q', {'action': 0}, ARRAYS, None), ('q', {'target': 0}, ARRAYS, None),
       ('q', {'obs': addr(8) + 2}, ARRAYS, None), ('q', {'action': addr(9) + 1}, ARRAYS, None), ('q', {'target': addr(10) + 3}, ARRAYS, None),
       ('q', {'weight': addr(19) + 2}, OPTIONAL, None), ('q', {'out_td_abs': addr(19) + 1}, OPTIONAL, None),
       ('q', {'out_q': addr(19) + 3}, OPTIONAL, None),
       ('q', {'net.workspace_bytes': 1535}, bytes_text('net: ', 1535, 1536, 's2d_learn_workspace_bytes'), None),
       ('q', {'batch': 65}, 'net: workspace_bytes is 1536, a batch of 65 needs 2560 (s2d_learn_workspace_bytes: batch is above the '
        "workspace's max_batch)", None),
       ('q', {'st.grad': addr(0)}, NO_OVERLAP, None), ('q', {'st.grad': addr(1) + 1520}, NO_OVERLAP, None),
       ('q', {'net.workspace': addr(0) + 768}, NO_OVERLAP, None), ('q', {'st.m': addr(0)}, NO_OVERLAP, 's2d_learn_q'),
       ('q', {'st.v': addr(4) + 960}, NO_OVERLAP, 's2d_learn_q'), ('q', {'st.v': addr(2)}, NO_OVERLAP, 's2d_learn_q'),
       # two faults: the earlier check speaks
       ('q', {'net.n_in': 0, 'st.loss_kind': 2}, 'net: n_in must be in [1, 256]', None),
       ('q', {'net.n_out': 0, 'net.n_hidden': 0}, 'net: n_hidden must be in [1, 4]', None),
       ('q', {'st.loss_kind': 2, 'batch': 0}, 'state: loss_kind must be 0 (MSE) or 1 (Huber)', None),
       ('q', {'batch': 0, 'net.params': 0}, BATCH, None),
       ('q', {'net.params': 0, 'net.workspace': 0}, params_text('net: '), None),
       ('q', {'net.workspace': 0, 'st.grad': 0}, workspace_text('net: '), None),
       ('q', {'st.error': 0, 'st.m': 0}, STATE, None),
       ('q', {'st.m': 0, 'obs': 0}, M_V, 's2d_learn_q'), ('q', {'st.m': 0, 'obs': 0}, ARRAYS, 's2d_learn_q_grad'),
       ('q', {'st.m': addr(0), 'st.v': 4, 'target': 0}, ARRAYS, 's2d_learn_q_grad'),
       ('q', {'target': 0, 'weight': 2}, ARRAYS, None),
       ('q', {'out_q': 2, 'net.workspace_bytes': 0}, OPTIONAL, None),
       ('q', {'net.workspace_bytes': 0, 'st.grad': addr(0)}, bytes_text('net: ', 0, 1536, 's2d_learn_workspace_bytes'), None)]
    # ----------------------------------------------------------------------------------------------- s2d_learn_critic[_grad]
    + [('critic', {'net': None}, 'net and state must be non-NULL', None), ('critic', {'st': None}, 'net and state must be non-NULL', None)]
    + shape_rows('critic', 'net', 'net: ')
    + [('critic', {'action_dim': 0}, 'action_dim must be in [1, 8]', None), ('critic', {'action_dim': 9}, 'action_dim must be in [1, 8]', None),
       ('critic', {'net.n_out': 2}, 'net: n_out must be 1 (a critic)', None),
       ('critic', {'net.n_in': 2}, 'net: n_in must be obs_dim + action_dim with obs_dim in [1, 248]', None),
       ('critic', {'net.n_in': 251}, 'net: n_in must be obs_dim + action_dim with obs_dim in [1, 248]', None),
       ('critic', {'st.loss_kind': 3}, 'state: loss_kind must be 0 (MSE), 1 (Huber) or 2 (square)', None),
       ('critic', {'st.loss_kind': -1}, 'state: loss_kind must be 0 (MSE), 1 (Huber) or 2 (square)', None),
       ('critic', {'batch': 0}, BATCH, None), ('critic', {'net.params': 8}, params_text('net: '), None),
       ('critic', {'net.workspace': 0}, workspace_text('net: '), None), ('critic', {'st.error': 0}, STATE, None),
       ('critic', {'st.v': 0}, M_V, 's2d_learn_critic'), ('critic', {'action': 0}, ARRAYS, None),
       ('critic', {'weight': 1}, OPTIONAL, None),
       ('critic', {'net.workspace_bytes': 0}, bytes_text('net: ', 0, 1536, 's2d_learn_workspace_bytes'), None),
       ('critic', {'st.grad': addr(1)}, NO_OVERLAP, None),
       ('critic', {'action_dim': 0, 'net.n_out': 2}, 'action_dim must be in [1, 8]', None),
       ('critic', {'net.n_out': 2, 'net.n_in': 2}, 'net: n_out must be 1 (a critic)', None),
       ('critic', {'net.n_in': 2, 'st.loss_kind': 3}, 'net: n_in must be obs_dim + action_dim with obs_dim in [1, 248]', None),
       ('critic', {'net.n_in': 0, 'action_dim': 0}, 'net: n_in must be in [1, 256]', None),
       ('critic', {'st.loss_kind': 3, 'batch': 0}, 'state: loss_kind must be 0 (MSE), 1 (Huber) or 2 (square)', None),
       ('critic', {'st.v': 0, 'action': 0}, ARRAYS, 's2d_learn_critic_grad')]
    # ------------------------------------------------------------------------------------------------ s2d_learn_actor[_grad]
    + [('actor', {k: None}, 'actor, state and critic must be non-NULL', None) for k in ('actor', 'st', 'critic')]
    + shape_rows('actor', 'actor', 'actor: ') + shape_rows('actor', 'critic', 'critic: ')
    + [('actor', {'actor.n_out': 9, 'critic.n_in': 19}, 'actor: n_out (the action width) must be in [1, 8]', None),
       ('actor', {'actor.n_in': 249, 'critic.n_in': 251}, 'actor: n_in must be in [1, 248]', None),
       ('actor', {'critic.n_in': 13}, "critic: n_in must be the actor's n_in + n_out, its n_out 1", None),
       ('actor', {'critic.n_out': 2}, "critic: n_in must be the actor's n_in + n_out, its n_out 1", None),
       ('actor', {'batch': -1}, BATCH, None), ('actor', {'actor.params': 0}, params_text('actor: '), None),
       ('actor', {'actor.workspace': 64}, workspace_text('actor: '), None),
       ('actor', {'st.grad': 0}, ACTOR_STATE, None), ('actor', {'st.hyper': 2}, ACTOR_STATE, None), ('actor', {'st.stats': 0}, ACTOR_STATE, None),
       ('actor', {'st.error': 0, 'obs': 0}, OBS, None),                      # the actor steps have no error word
       ('actor', {'st.m': 0}, M_V, 's2d_learn_actor'), ('actor', {'st.v': 8}, M_V, 's2d_learn_actor'),
       ('actor', {'critic.params': 0}, params_text('critic: '), None), ('actor', {'critic.params': addr(11) + 4}, params_text('critic: '), None),
       ('actor', {'obs': 0}, OBS, None), ('actor', {'obs': 2}, OBS, None),
       ('actor', {'out_action': 2}, 'out_action and out_q must be 4-byte aligned device pointers (or NULL)', None),
       ('actor', {'out_q': 1}, 'out_action and out_q must be 4-byte aligned device pointers (or NULL)', None),
       ('actor', {'actor.workspace_bytes': 100}, bytes_text('actor: ', 100, 1536, 's2d_learn_actor_workspace_bytes'), None),
       ('actor', {'st.grad': addr(0)}, ACTOR_NO_OVERLAP, None), ('actor', {'critic.params': addr(0)}, ACTOR_NO_OVERLAP, None),
       ('actor', {'critic.params': addr(1) + 1024}, ACTOR_NO_OVERLAP, None), ('actor', {'critic.params': addr(4) - 16}, ACTOR_NO_OVERLAP, None),
       ('actor', {'critic.params': addr(2)}, ACTOR_NO_OVERLAP, 's2d_learn_actor'),
       ('actor', {'critic.params': addr(2), 'obs': 0}, OBS, 's2d_learn_actor_grad'),
       ('actor', {'actor.n_in': 0, 'critic.n_out': 0}, 'actor: n_in must be in [1, 256]', None),
       ('actor', {'critic.n_hidden': 0, 'actor.n_out': 9}, 'critic: n_hidden must be in [1, 4]', None),
       ('actor', {'actor.n_out': 9, 'actor.n_in': 249}, 'actor: n_out (the action width) must be in [1, 8]', None),
       ('actor', {'critic.n_out': 2, 'batch': 0}, "critic: n_in must be the actor's n_in + n_out, its n_out 1", None),
       ('actor', {'batch': 0, 'actor.params': 0}, BATCH, None),
       ('actor', {'st.m': 0, 'critic.params': 0}, M_V, 's2d_learn_actor'),
       ('actor', {'critic.params': 0, 'obs': 0}, params_text('critic: '), None),
       ('actor', {'obs': 0, 'out_q': 1}, OBS, None),
       ('actor', {'out_q': 1, 'actor.workspace_bytes': 0}, 'out_action and out_q must be 4-byte aligned device pointers (or NULL)', None),
       ('actor', {'actor.workspace_bytes': 0, 'critic.params': addr(0)}, bytes_text('actor: ', 0, 1536, 's2d_learn_actor_workspace_bytes'), None)]
    # -------------------------------------------------------------------------------------------- s2d_learn_sac_actor[_grad]
    + [('sac', {k: None}, 'actor, state and critic1 must be non-NULL', None) for k in ('actor', 'st', 'critic1')]
    + shape_rows('sac', 'actor', 'actor: ') + shape_rows('sac', 'critic1', 'critic1: ') + shape_rows('sac', 'critic2', 'critic2: ')
    + [('sac', {'actor.n_out': 3}, 'actor: n_out (means, then raw log-std) must be even and in [2, 16]', None),
       ('sac', {'actor.n_out': 18}, 'actor: n_out (means, then raw log-std) must be even and in [2, 16]', None),
       ('sac', {'actor.n_in': 249}, 'actor: n_in must be in [1, 248]', None),
       ('sac', {'critic1.n_in': 14}, "critic1: n_in must be the actor's n_in + n_out / 2, its n_out 1", None),
       ('sac', {'critic1.n_out': 2}, "critic1: n_in must be the actor's n_in + n_out / 2, its n_out 1", None),
       ('sac', {'critic2.n_in': 11}, "critic2: n_in must be the actor's n_in + n_out / 2, its n_out 1", None),
       ('sac', {'critic2.n_out': 2}, "critic2: n_in must be the actor's n_in + n_out / 2, its n_out 1", None),
       ('sac', {'batch': 0}, BATCH, None), ('sac', {'actor.params': 4}, params_text('actor: '), None),
       ('sac', {'actor.workspace': 0}, workspace_text('actor: '), None), ('sac', {'st.stats': 0}, ACTOR_STATE, None),
       ('sac', {'st.m': 0}, M_V, 's2d_learn_sac_actor'),
       ('sac', {'critic1.params': 0}, params_text('critic1: '), None), ('sac', {'critic1.params': 8}, params_text('critic1: '), None),
       ('sac', {'critic2.params': 0}, params_text('critic2: '), None), ('sac', {'critic2.params': 8}, params_text('critic2: '), None),
       ('sac', {'obs': 0}, OBS, None),
       ('sac', {'alpha': 0}, 'alpha must be a non-NULL, 4-byte aligned device pointer', None),
       ('sac', {'alpha': 2}, 'alpha must be a non-NULL, 4-byte aligned device pointer', None),
       ('sac', {'draws': 0}, 'draws must be a non-NULL, 8-byte aligned device pointer', None),
       ('sac', {'draws': addr(14) + 4}, 'draws must be a non-NULL, 8-byte aligned device pointer', None)]
    + [('sac', {f'alpha_state.{k}': v}, SAC_ALPHA_STATE, None) for k in ('log_alpha', 'm_v', 'hyper', 'stats') for v in (0, addr(20) + 2)]
    + [('sac', {k: addr(20) + 2}, SAC_OUTS, None) for k in ('out_action', 'out_logp', 'out_q')]
    + [('sac', {'actor.workspace_bytes': 1791}, bytes_text('actor: ', 1791, 1792, 's2d_learn_sac_workspace_bytes'), None),
       ('sac', {'st.grad': addr(1)}, ACTOR_NO_OVERLAP, None), ('sac', {'critic1.params': addr(4)}, ACTOR_NO_OVERLAP, None),
       ('sac', {'critic2.params': addr(4)}, ACTOR_NO_OVERLAP, None), ('sac', {'critic2.params': addr(0) - 16}, ACTOR_NO_OVERLAP, None),
       ('sac', {'critic2.params': addr(3)}, ACTOR_NO_OVERLAP, 's2d_learn_sac_actor'),
       ('sac', {'critic2.params': addr(3), 'alpha': addr(14) + 4}, SAC_MINE, 's2d_learn_sac_actor_grad'),
       ('sac', {'alpha': addr(14)}, SAC_MINE, None), ('sac', {'alpha': addr(14) + 4}, SAC_MINE, None),
       ('sac', {'alpha_state.m_v': addr(17) - 4}, SAC_MINE, None), ('sac', {'alpha_state.stats': addr(17) + 24}, SAC_MINE, None),
       ('sac', {'alpha_state.stats': addr(15) - 8}, SAC_MINE, None), ('sac', {'draws': addr(16)}, SAC_MINE, None),
       ('sac', {'alpha': addr(0)}, SAC_OTHER, None), ('sac', {'draws': addr(4) + 8}, SAC_OTHER, None),
       ('sac', {'alpha_state.log_alpha': addr(1) + 1788}, SAC_OTHER, None), ('sac', {'alpha_state.m_v': addr(11)}, SAC_OTHER, None),
       ('sac', {'alpha_state.hyper': addr(12) - 24}, SAC_OTHER, None), ('sac', {'alpha_state.stats': addr(3)}, SAC_OTHER, 's2d_learn_sac_actor'),
       ('sac', {'out_action': addr(13) - 508}, SAC_OTHER, None), ('sac', {'out_logp': addr(13) - 252}, SAC_OTHER, None),
       ('sac', {'out_q': addr(18) + 8}, SAC_OTHER, None),
       # a fixed temperature (alpha_state NULL) and one critic: the same checks of what is left
       ('sac', {'alpha_state': None, 'critic2': None, 'alpha': addr(14)}, SAC_MINE, None),
       ('sac', {'alpha_state': None, 'critic2': None, 'draws': addr(11)}, SAC_OTHER, None),
       ('sac', {'critic2': None, 'critic1.n_in': 13}, "critic1: n_in must be the actor's n_in + n_out / 2, its n_out 1", None),
       # two faults
       ('sac', {'actor.n_in': 0, 'critic1.n_hidden': 0}, 'actor: n_in must be in [1, 256]', None),
       ('sac', {'critic1.n_hidden': 0, 'critic2.n_in': 0}, 'critic1: n_hidden must be in [1, 4]', None),
       ('sac', {'critic2.n_in': 0, 'actor.n_out': 3}, 'critic2: n_in must be in [1, 256]', None),
       ('sac', {'actor.n_out': 18, 'actor.n_in': 249}, 'actor: n_out (means, then raw log-std) must be even and in [2, 16]', None),
       ('sac', {'actor.n_in': 249, 'critic1.n_out': 2}, 'actor: n_in must be in [1, 248]', None),
       ('sac', {'critic1.n_out': 2, 'critic2.n_out': 2}, "critic1: n_in must be the actor's n_in + n_out / 2, its n_out 1", None),
       ('sac', {'critic2.n_out': 2, 'batch': 0}, "critic2: n_in must be the actor's n_in + n_out / 2, its n_out 1", None),
       ('sac', {'batch': 0, 'actor.params': 0}, BATCH, None),
       ('sac', {'st.m': 0, 'critic1.params': 0}, M_V, 's2d_learn_sac_actor'),
       ('sac', {'st.m': 0, 'critic1.params': 0}, params_text('critic1: '), 's2d_learn_sac_actor_grad'),
       ('sac', {'critic1.params': 0, 'critic2.params': 0}, params_text('critic1: '), None),
       ('sac', {'critic2.params': 0, 'obs': 0}, params_text('critic2: '), None),
       ('sac', {'obs': 0, 'alpha': 0}, OBS, None),
       ('sac', {'alpha': 0, 'draws': 0}, 'alpha must be a non-NULL, 4-byte aligned device pointer', None),
       ('sac', {'draws': 0, 'alpha_state.hyper': 0}, 'draws must be a non-NULL, 8-byte aligned device pointer', None),
       ('sac', {'alpha_state.hyper': 0, 'out_q': 2}, SAC_ALPHA_STATE, None),
       ('sac', {'out_q': 2, 'actor.workspace_bytes': 0}, SAC_OUTS, None),
       ('sac', {'actor.workspace_bytes': 0, 'alpha': addr(14)}, bytes_text('actor: ', 0, 1792, 's2d_learn_sac_workspace_bytes'), None),
       ('sac', {'st.grad': addr(0), 'alpha': addr(14)}, ACTOR_NO_OVERLAP, None),
       ('sac', {'critic1.params': addr(1), 'alpha': addr(0)}, ACTOR_NO_OVERLAP, None),
       ('sac', {'alpha': addr(0), 'draws': addr(15)}, SAC_OTHER, None),       # alpha's turn comes before draws'
       ('sac', {'alpha': addr(14), 'alpha_state.log_alpha': addr(0)}, SAC_MINE, None),
       ('sac', {'alpha': addr(15), 'draws': addr(0)}, SAC_MINE, None),
       ('sac', {'alpha': addr(15), 'out_q': addr(15)}, SAC_MINE, None),       # an array's own kind first, then the others
       ('sac', {'critic2.params': addr(4), 'alpha_state.stats': addr(17)}, SAC_MINE, None),
       ('sac', {'critic2.params': addr(4), 'out_q': addr(13)}, SAC_OTHER, None)]
    # -------------------------------------------------------------------------------------------------- s2d_learn_ppo[_grad]
    + [('ppo', {k: None}, 'learner and batch must be non-NULL', None) for k in ('q', 'b')]
    + shape_rows('ppo', 'q.pi', 'pi: ') + shape_rows('ppo', 'q.vf', 'vf: ')
    + [('ppo', {'q.vf.n_out': 2}, "vf: n_in must be pi's n_in, its n_out 1", None),
       ('ppo', {'q.vf.n_in': 11}, "vf: n_in must be pi's n_in, its n_out 1", None),
       ('ppo', {'q.head': 2}, 'head must be 0 (categorical) or 1 (diagonal Gaussian)', None),
       ('ppo', {'q.head': -1}, 'head must be 0 (categorical) or 1 (diagonal Gaussian)', None),
       ('ppo', {'q.head': 1, 'q.pi.n_out': 9}, 'pi: n_out (the action width) must be in [1, 8] with the Gaussian head', None),
       ('ppo', {'b.rows': 0}, 'rows must be in [1, 2^31 - 1]', None), ('ppo', {'b.rows': 2 ** 31}, 'rows must be in [1, 2^31 - 1]', None),
       ('ppo', {'b.batch': 0}, BATCH, None), ('ppo', {'b.batch': 2 ** 31}, BATCH, None),
       ('ppo', {'b.rows': 63}, 'batch must be at most rows where index is NULL', None),
       ('ppo', {'q.params': 0}, params_text(''), None), ('ppo', {'q.params': 8}, params_text(''), None),
       ('ppo', {'q.workspace': 0}, workspace_text(''), None), ('ppo', {'q.workspace': addr(1) + 16}, workspace_text(''), None)]
    + [('ppo', {f'q.{k}': v}, PPO_STATE, None) for k, v in (('grad', 0), ('grad', 8), ('hyper', 0), ('hyper', 2), ('stats', 0), ('stats', 1),
                                                             ('error', 0), ('error', 3))]
    + [('ppo', {f'q.{k}': v}, 'm and v must be non-NULL, 16-byte aligned device pointers', 's2d_learn_ppo') for k in 'mv' for v in (0, 8)]
    + [('ppo', {f'b.{k}': v}, PPO_ARRAYS, None) for k in ('obs', 'action', 'logp_old', 'advantage', 'ret') for v in (0, addr(20) + 2)]
    + [('ppo', {f'b.{k}': addr(20) + 1}, PPO_OPTIONAL, None) for k in ('index', 'out_logp', 'out_value')]
    + [('ppo', {'q.workspace_bytes': 2815}, bytes_text('', 2815, 2816, 's2d_learn_ppo_workspace_bytes'), None),
       ('ppo', {'q.grad': addr(0)}, NO_OVERLAP, None), ('ppo', {'q.workspace': addr(0) + 1024}, NO_OVERLAP, None),
       ('ppo', {'q.grad': addr(1) + 2800}, NO_OVERLAP, None), ('ppo', {'q.m': addr(3)}, NO_OVERLAP, 's2d_learn_ppo'),
       ('ppo', {'q.v': addr(0) + 1024}, NO_OVERLAP, 's2d_learn_ppo'),
       ('ppo', {'q.pi.n_in': 0, 'q.vf.n_in': 0}, 'pi: n_in must be in [1, 256]', None),
       ('ppo', {'q.vf.n_hidden': 0, 'q.vf.n_out': 2}, 'vf: n_hidden must be in [1, 4]', None),
       ('ppo', {'q.vf.n_out': 2, 'q.head': 2}, "vf: n_in must be pi's n_in, its n_out 1", None),
       ('ppo', {'q.head': 2, 'b.rows': 0}, 'head must be 0 (categorical) or 1 (diagonal Gaussian)', None),
       ('ppo', {'b.rows': 0, 'b.batch': 0}, 'rows must be in [1, 2^31 - 1]', None),
       ('ppo', {'b.batch': 0, 'q.params': 0}, BATCH, None),
       ('ppo', {'b.rows': 63, 'q.params': 0}, 'batch must be at most rows where index is NULL', None),
       ('ppo', {'b.rows': 63, 'b.index': addr(13), 'q.params': 0}, params_text(''), None),
       ('ppo', {'q.params': 0, 'q.workspace': 0}, params_text(''), None),
       ('ppo', {'q.workspace': 0, 'q.error': 0}, workspace_text(''), None),
       ('ppo', {'q.error': 0, 'q.m': 0}, PPO_STATE, None),
       ('ppo', {'q.m': 0, 'b.obs': 0}, 'm and v must be non-NULL, 16-byte aligned device pointers', 's2d_learn_ppo'),
       ('ppo', {'q.m': 0, 'b.obs': 0}, PPO_ARRAYS, 's2d_learn_ppo_grad'),
       ('ppo', {'q.v': addr(0), 'b.ret': 0}, PPO_ARRAYS, 's2d_learn_ppo_grad'),
       ('ppo', {'b.ret': 0, 'b.index': 2}, PPO_ARRAYS, None),
       ('ppo', {'b.out_value': 2, 'q.workspace_bytes': 0}, PPO_OPTIONAL, None),
       ('ppo', {'q.workspace_bytes': 0, 'q.grad': addr(0)}, bytes_text('', 0, 2816, 's2d_learn_ppo_workspace_bytes'), None)])


def put(c, name, value):
    *path, last = name.split('.')
    for p in path:
        c = getattr(c, p)
    if last.isdigit():
        c[int(last)] = value
    else:
        setattr(c, last, value)


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi
    return _capi, _capi.load_library()


def test_the_table_covers_every_entry_point_and_every_row_is_written_out():
    from soccer2d_amd import _capi
    steps = {p[0] for p in _capi.PROTOTYPES if p[0].startswith('s2d_learn') and not p[0].endswith('workspace_bytes')}
    assert steps == {fn for _, fns in FAMILIES.values() for fn in fns}
    assert all(fam in FAMILIES and edits and text and (only is None or only in FAMILIES[fam][1]) for fam, edits, text, only in ROWS)
    assert len(set((fam, tuple(edits.items()), only) for fam, edits, _, only in ROWS)) == len(ROWS)


def test_the_good_calls_are_on_the_grid(lib):
    """the calls the rows edit are good in everything the host can see: their workspace sizes are the library's, so every refusal
    below is the edit's"""
    _capi, L = lib
    sizes = {fam: make(_capi, L) for fam, (make, _) in FAMILIES.items()}
    assert [sizes['q'].net.workspace_bytes, sizes['critic'].net.workspace_bytes, sizes['actor'].actor.workspace_bytes,
            sizes['sac'].actor.workspace_bytes, sizes['ppo'].q.workspace_bytes] == [1536, 1536, 1536, 1792, 2816]


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_every_refusal_in_full(lib, family):
    _capi, L = lib
    make, fns = FAMILIES[family]
    wrong = []
    for fam, edits, text, only in ROWS:
        if fam != family:
            continue
        for fn in fns if only is None else (only,):
            c = make(_capi, L)
            for name, value in edits.items():
                put(c, name, value)
            rc = getattr(L, fn)(*c.args())
            got = L.s2d_last_error().decode() if rc != _capi.S2D_OK else ''
            if rc != _capi.S2D_EINVAL or got != f'{fn}: {text}':
                wrong.append((fn, edits, rc, got, f'{fn}: {text}'))
    assert not wrong, '\n'.join(f'{fn} {edits}: rc {rc}\n  got  {got!r}\n  want {want!r}' for fn, edits, rc, got, want in wrong)
