"""CPU checks of the 11v11 see policy slots (s2d_match_set_see_policy_network, s2d_match_rollout_see_policy): the host restatement
of the forward pass (tests/see_policy_ref.c) against float64 torch at the see network's bound and against the two restatements it
joins; MatchSeePolicyActor's validation, snapshot and device word; what MatchEngine checks and calls, on the recording library of
tests/test_match_policy_host.py; the struct's ctypes layout against the compiler; the entry points declared, bound and exported."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import match_policy as MP
import see_net as SN
import see_policy as SP
from test_match_policy_host import _bare_engine

torch = pytest.importorskip('torch')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp('see_policy')
    return SP.build(d), SN.build(d)


def _module(h1, h2, k, seed, act=torch.nn.Tanh, dim=192):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(dim, h1), act(), torch.nn.Linear(h1, h2), act(), torch.nn.Linear(h2, k))


def _packed(m):
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()]).numpy()


# ------------------------------------------------------------------------------------------ the restated forward
@pytest.mark.parametrize('act', [torch.nn.ReLU, torch.nn.Tanh])
@pytest.mark.parametrize('h1,h2,k', [(16, 16, 1), (32, 48, 5), (64, 64, 16), (48, 32, 64)])
def test_host_forward_against_float64_torch(refs, h1, h2, k, act):
    """the bound of tests/test_match_see_net_host.py::test_host_forward_against_float64_torch, on the same rows"""
    (L, _), _ = refs
    m = _module(h1, h2, k, h1 + h2 + k, act)
    rng = np.random.default_rng(k)
    x = rng.normal(0, 20, (257, 192)).astype(np.float32)
    got = SP.forward(L, x, _packed(m), h1, h2, k, act is torch.nn.Tanh)
    want = m.double()(torch.from_numpy(x).double()).detach().numpy()
    assert got.shape == (257, k)
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4 * np.abs(want).max())


def test_host_forward_equals_the_restatements_it_joins(refs):
    """relu on 192 words is bitwise the see network's restatement; either activation on 224 words is bitwise the policy slots'"""
    (L, PL), SL = refs
    rng = np.random.default_rng(2)
    m = _module(32, 16, 7, 3, torch.nn.ReLU)
    x = rng.normal(0, 5, (64, 192)).astype(np.float32)
    x[0, :6] = [np.nan, -0.0, np.inf, -np.inf, 1e30, 1e-40]
    a = SP.forward(L, x, _packed(m), 32, 16, 7, 0)
    b = SN.forward(SL, x, _packed(m), 32, 16, 7)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    for act, cls in ((0, torch.nn.ReLU), (1, torch.nn.Tanh)):
        m = _module(48, 32, 9, 4, cls, dim=224)
        x = rng.normal(0, 5, (64, 224)).astype(np.float32)
        a = SP.forward(L, x, _packed(m), 48, 32, 9, act, dim=224)
        b = MP.forward(PL, x, _packed(m), 48, 32, 9, act)
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), act


# ------------------------------------------------------------------------------------------ MatchSeePolicyActor
def test_actor_packs_validates_and_snapshots():
    from soccer2d_amd import _capi_match as M
    from soccer2d_amd.actor import MatchPolicyActor, MatchSeePolicyActor
    m = _module(32, 16, 5, 1)
    table = np.arange(25, dtype=np.float32).reshape(5, 5)
    a = MatchSeePolicyActor.from_module(m, table, device='cpu')
    assert (a.hidden1, a.hidden2, a.n_actions, a.obs, a.kind, a.in_dim, a.activation) == (32, 16, 5, 'see', 'policy', 192, 'tanh')
    assert a.shapes()[0] == (32, 192) and a.table.shape == (5, 5)
    assert np.array_equal(a.params.numpy(), _packed(m)) and a.params.numel() == SP.param_count(32, 16, 5)
    assert MatchSeePolicyActor.from_module(_module(16, 16, 3, 1, torch.nn.ReLU), np.zeros((3, 5)), device='cpu').activation == 'relu'
    with torch.no_grad():
        m[0].weight.add_(1.0)
    a.sync()
    assert np.array_equal(a.params.numpy(), _packed(m))
    for kw in (dict(hidden1=24), dict(hidden2=80), dict(hidden1=128), dict(n_actions=0), dict(n_actions=65),
               dict(activation='sigmoid')):
        with pytest.raises(ValueError):
            MatchSeePolicyActor(device='cpu', **kw)
    for bad in (np.zeros((5, 3)), np.zeros((4, 5)), np.zeros((5, 6)), np.zeros(25)):
        with pytest.raises(ValueError, match='table'):
            a.set_table(bad)
        with pytest.raises(ValueError, match='table'):
            MatchSeePolicyActor.from_module(m, bad, device='cpu')
    with pytest.raises(ValueError, match='shapes'):
        MatchSeePolicyActor.from_module(_module(32, 16, 5, 1, dim=224), table, device='cpu')       # an agent-row module
    with pytest.raises(ValueError, match='activation'):
        MatchSeePolicyActor(32, 16, 5, activation='relu', device='cpu').load_from(m)
    with pytest.raises(ValueError):
        MatchSeePolicyActor.from_module(torch.nn.Sequential(torch.nn.Linear(192, 16), torch.nn.Tanh(), torch.nn.Linear(16, 16),
                                                            torch.nn.ReLU(), torch.nn.Linear(16, 5)), table, device='cpu')
    # the agent-row policy keeps refusing see rows, and says where they went
    with pytest.raises(ValueError, match='MatchSeePolicyActor'):
        MatchPolicyActor(16, 16, 5, device='cpu', obs='see')
    with pytest.raises(ValueError, match='shapes'):
        MatchPolicyActor.from_module(m, np.zeros((5, 3), dtype=np.float32), device='cpu')
    # the deterministic word: one device word, written in place
    assert a.deterministic is False and a.deterministic_tensor.dtype == torch.int32 and int(a.deterministic_tensor) == 0
    word = a.deterministic_tensor.data_ptr()
    a.deterministic = True
    assert a.deterministic is True and int(a.deterministic_tensor) == 1 and a.deterministic_tensor.data_ptr() == word
    # snapshot: its own buffers, no module
    s = a.snapshot()
    assert isinstance(s, MatchSeePolicyActor) and s.deterministic is True and a.snapshot(deterministic=False).deterministic is False
    assert torch.equal(s.params, a.params) and torch.equal(s.table, a.table)
    for x, y in ((s.params, a.params), (s.table, a.table), (s.deterministic_tensor, a.deterministic_tensor)):
        assert x.data_ptr() != y.data_ptr()
    old = a.params.clone()
    with torch.no_grad():
        m[2].bias.add_(1.0)
    a.sync()
    a.set_table(table + 1.0)
    a.deterministic = False
    assert not torch.equal(a.params, old) and torch.equal(s.params, old) and torch.equal(s.table, torch.from_numpy(table))
    assert int(s.deterministic_tensor) == 1
    with pytest.raises(ValueError):
        s.sync()
    # the struct
    with pytest.raises(ValueError, match='vision'):
        a.c_struct(0x7FF)
    prm, vis = M.S2DVisionParams(), M.S2DMatchVision(64, 128, 192)
    prm.visible_distance = 3.0
    cs = a.c_struct(0x3FF800, prm, vis)
    assert isinstance(cs, M.S2DMatchSeePolicyNet)
    assert (cs.h1, cs.h2, cs.n_actions, cs.slot_mask, cs.activation) == (32, 16, 5, 0x3FF800, 1)
    assert (cs.params, cs.deterministic, cs.table) == (a.params.data_ptr(), a.deterministic_tensor.data_ptr(), a.table.data_ptr())
    assert cs.prm.visible_distance == 3.0 and (cs.vis.neck, cs.vis.view_width, cs.vis.see_wait) == (64, 128, 192)


# ------------------------------------------------------------------------------------------ MatchEngine's dispatch
def _vision(eng):
    from soccer2d_amd import _capi_match as M
    eng.vision_params, eng.vision = M.S2DVisionParams(), M.S2DMatchVision(64, 128, 192)


def test_set_network_calls_the_new_setter():
    from soccer2d_amd.actor import MatchQNetActor, MatchSeePolicyActor
    from soccer2d_amd.match import Soccer2DMatchVecEnv, _is_match_actor
    eng = _bare_engine()
    p = MatchSeePolicyActor(16, 16, 4, device='cpu')
    assert _is_match_actor(p)
    assert Soccer2DMatchVecEnv.spaces(p, 'see')[0].shape == (11, 192) and Soccer2DMatchVecEnv.spaces(p, 'see')[1].shape == (11, 5)
    with pytest.raises(RuntimeError, match='enable_vision'):
        eng.set_network(p, 'all')
    assert eng.lib.calls == [] and eng.network is None
    _vision(eng)
    eng.opponent_network, eng.opponent_mask = MatchQNetActor(16, 16, 4, device='cpu'), 0x3FF800
    eng.set_network(p, 'left')
    assert eng.lib.calls == [('s2d_match_set_see_policy_network',)] and eng.network is p and eng.network_mask == 0x7FF
    assert eng.opponent_network is None and eng.opponent_mask == 0          # the see policy is the engine's only network
    n_calls = len(eng.lib.calls)
    with pytest.raises(ValueError, match='see'):
        eng.set_opponent_network(p.snapshot(), 'right')                      # a see actor is never the opponent
    with pytest.raises(ValueError, match='see network'):
        eng.set_opponent_network(MatchQNetActor(16, 16, 4, device='cpu'), 'right')   # nor anything beside a see policy
    assert len(eng.lib.calls) == n_calls
    q = MatchQNetActor(16, 16, 4, device='cpu', obs='see')
    eng.set_network(q, 'all')                                                # the see Q-network keeps its setter
    assert eng.lib.calls[-1] == ('s2d_match_set_see_network',)


def test_rollout_dispatch_and_buffer_validation():
    from soccer2d_amd.actor import MatchQNetActor, MatchSeePolicyActor
    eng = _bare_engine(4)
    _vision(eng)
    eng.agent_reward_weights = None
    eng.set_network(MatchSeePolicyActor(16, 16, 4, device='cpu'), 'all')
    T = 3
    base = dict(reward=torch.zeros((T, 4)), mode=torch.zeros((T, 4), dtype=torch.int32), done=torch.zeros((T, 4), dtype=torch.uint8))
    out = eng.rollout(T, out=dict(base), with_obs=False, logp=True, see_obs='left', net_index=True, record_actions=True,
                      view_actions=np.zeros((T, 4, 22, 2), dtype=np.float32))
    assert eng.lib.calls[-1][0] == 's2d_match_rollout_see_policy'
    assert out['logp'].dtype == torch.float32 and tuple(out['logp'].shape) == (T, 4, 22)
    assert tuple(out['see'].shape) == (T, 4, 11, 192) and tuple(out['net_index'].shape) == (T, 4, 22)
    assert tuple(out['actions'].shape) == (T, 4, 22, 3)
    out = eng.rollout(T, out=dict(base), with_obs=False, logp=True)          # logp alone: still the see policy's entry point
    assert eng.lib.calls[-1][0] == 's2d_match_rollout_see_policy' and set(out) == set(base) | {'logp'}
    eng.rollout(T, out=dict(base), with_obs=False, net_index=True, see_obs='all')
    assert eng.lib.calls[-1][0] == 's2d_match_rollout_see'                   # without logp: the entry point it was
    eng.rollout(T, out=dict(base), with_obs=False)
    assert eng.lib.calls[-1][0] == 's2d_match_rollout'
    n_calls = len(eng.lib.calls)
    for bad in (torch.zeros((T, 4, 22), dtype=torch.float64), torch.zeros((T - 1, 4, 22)), torch.zeros((T, 4, 21)),
                torch.zeros((T, 3, 22)), torch.zeros((T, 4, 44))[:, :, ::2]):
        with pytest.raises(ValueError, match='logp'):
            eng.rollout(T, out=dict(base, logp=bad), with_obs=False, logp=True, see_obs='all')
    with pytest.raises(ValueError, match='agent_obs'):
        eng.rollout(T, out=dict(base), with_obs=False, logp=True, agent_obs='left')
    with pytest.raises(ValueError, match='agent_obs'):
        eng.rollout(T, out=dict(base), with_obs=False, logp=True, see_obs='left', agent_obs='left')
    with pytest.raises(ValueError, match='agent_reward'):
        eng.rollout(T, out=dict(base), with_obs=False, logp=True, agent_reward=True)
    with pytest.raises(ValueError, match='view_actions'):
        eng.rollout(T, out=dict(base), with_obs=False, logp=True, view_actions=np.zeros((T, 4, 22, 3), dtype=np.float32))
    assert len(eng.lib.calls) == n_calls
    big = torch.zeros((T + 2, 4, 22))
    assert eng.rollout(T, out=dict(base, logp=big), with_obs=False, logp=True)['logp'] is big
    # a see Q-network has no log-probabilities, with or without a see record
    eng.network = MatchQNetActor(16, 16, 4, device='cpu', obs='see')
    n_calls = len(eng.lib.calls)
    for kw in (dict(), dict(see_obs='all'), dict(net_index=True)):
        with pytest.raises(ValueError, match='policy head'):
            eng.rollout(T, out=dict(base), with_obs=False, logp=True, **kw)
    assert len(eng.lib.calls) == n_calls


# ------------------------------------------------------------------------------------------ the ABI
def test_struct_and_entry_points_match_the_header(tmp_path):
    import __graft_entry__ as g
    from soccer2d_amd import _capi, _capi_match as M
    hdr = open(os.path.join(ROOT, 'include', 's2d_match.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint\s+s2d_match_set_see_policy_network\s*\(\s*S2DMatchHandle\s+h\s*,\s*const\s+S2DMatchSeePolicyNet\s*\*\s*net\s*\)\s*;', code)
    assert re.search(r'\bint\s+s2d_match_rollout_see_policy\s*\(\s*S2DMatchHandle\s+h\s*,\s*int\s+n_steps\s*,\s*const\s+float\s*\*\s*actions_dev\s*,'
                     r'\s*const\s+float\s*\*\s*view_actions_dev\s*,\s*const\s+S2DMatchRollout\s*\*\s*out\s*,\s*float\s*\*\s*actions_out_dev\s*,'
                     r'\s*int32_t\s*\*\s*net_index_out_dev\s*,\s*float\s*\*\s*logp_out_dev\s*,\s*uint32_t\s+obs_mask\s*,'
                     r'\s*float\s*\*\s*see_out_dev\s*,\s*void\s*\*\s*stream\s*\)\s*;', code)
    protos = {p[0]: p for p in M.MATCH_PROTOTYPES}
    assert protos['s2d_match_set_see_policy_network'][1:] == protos['s2d_match_set_see_network'][1:]
    see = protos['s2d_match_rollout_see'][2]
    assert protos['s2d_match_rollout_see_policy'][1:] == (C.c_int, see[:7] + (C.c_void_p,) + see[7:])
    fields = [f for f, _ in M.S2DMatchSeePolicyNet._fields_]
    assert fields == ['h1', 'h2', 'n_actions', 'slot_mask', 'params', 'deterministic', 'table', 'prm', 'vis', 'activation']
    probe = tmp_path / 'probe.c'
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s2d_match.h"\nint main(void) {\n'
                     '  printf("%zu", sizeof(S2DMatchSeePolicyNet));\n' +
                     ''.join(f'  printf(" %zu", offsetof(S2DMatchSeePolicyNet, {f}));\n' for f in fields) +
                     '  printf(" %zu", sizeof(S2DMatchSeeNet));\n  return 0;\n}\n')
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(probe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got[0] == C.sizeof(M.S2DMatchSeePolicyNet)
    assert got[1:-1] == [getattr(M.S2DMatchSeePolicyNet, f).offset for f in fields]
    assert got[-1] == C.sizeof(M.S2DMatchSeeNet)           # the see Q-network's struct keeps its layout
    g.build_hip()
    lib = M.bind(_capi.load_library())
    fn = lib.s2d_match_set_see_policy_network
    assert fn.restype is C.c_int and fn.argtypes == [C.c_void_p, C.c_void_p]
    assert fn(None, None) == _capi.S2D_EINVAL and b'NULL handle' in lib.s2d_last_error()
    ro = lib.s2d_match_rollout_see_policy
    assert ro.restype is C.c_int and len(ro.argtypes) == 11
    assert ro(None, 1, None, None, None, None, None, None, 0, None, None) == _capi.S2D_EINVAL and b'NULL handle' in lib.s2d_last_error()
