"""CPU checks of the 11v11 policy slots (s2d_match_set_policy_network, s2d_match_rollout_policy): the entry points are declared,
bound and exported and the struct's ctypes layout is the C one; MatchPolicyActor's accepted and refused module forms, its
snapshot and its device word; the argument checks MatchEngine makes before it reaches the library; and the host restatement
tests/match_policy_ref.c that the GPU tests compare the device with -- the sampler's frequencies and logp against float64, which
word of the slot's block it uses, the edge rows by value, and both activations of the forward pass."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import match_policy as MP
from test_policy_host import chi2_sf_odd, chi2_stat, fixed_logits, softmax64

torch = pytest.importorskip('torch')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return MP.build(tmp_path_factory.mktemp('match_policy_ref'))


# ------------------------------------------------------------------------------------------ exports
def test_entry_points_are_declared_bound_and_exported(tmp_path):
    import __graft_entry__ as g
    from soccer2d_amd import _capi, _capi_match as M
    hdr = open(os.path.join(ROOT, 'include', 's2d_match.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint\s+s2d_match_set_policy_network\s*\(\s*S2DMatchHandle\s+h\s*,\s*int\s+role\s*,\s*const\s+S2DMatchPolicyNet\s*\*\s*net\s*\)\s*;', code)
    assert re.search(r'\bint\s+s2d_match_rollout_policy\s*\(\s*S2DMatchHandle\s+h\s*,\s*int\s+n_steps\s*,\s*const\s+float\s*\*\s*actions_dev\s*,'
                     r'\s*const\s+S2DMatchRollout\s*\*\s*out\s*,\s*float\s*\*\s*actions_out_dev\s*,\s*int32_t\s*\*\s*net_index_out_dev\s*,'
                     r'\s*float\s*\*\s*logp_out_dev\s*,\s*uint32_t\s+obs_mask\s*,\s*float\s*\*\s*agent_obs_out_dev\s*,\s*void\s*\*\s*stream\s*\)\s*;', code)
    assert re.search(r'#define\s+S2D_MATCH_ROLE_NETWORK\s+0\b', code) and re.search(r'#define\s+S2D_MATCH_ROLE_OPPONENT\s+1\b', code)
    assert (M.MATCH_ROLE_NETWORK, M.MATCH_ROLE_OPPONENT) == (0, 1)
    protos = {p[0]: p for p in M.MATCH_PROTOTYPES}
    assert protos['s2d_match_set_policy_network'][1:] == (C.c_int, (C.c_void_p, C.c_int, C.c_void_p))
    net = protos['s2d_match_rollout_net'][2]
    assert protos['s2d_match_rollout_policy'][1:] == (C.c_int, net[:6] + (C.c_void_p,) + net[6:])
    # the struct: ctypes against the compiler
    probe = tmp_path / 'probe.c'
    fields = [f for f, _ in M.S2DMatchPolicyNet._fields_]
    assert fields == ['h1', 'h2', 'n_actions', 'slot_mask', 'activation', 'params', 'deterministic', 'table']
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s2d_match.h"\nint main(void) {\n'
                     '  printf("%zu", sizeof(S2DMatchPolicyNet));\n' +
                     ''.join(f'  printf(" %zu", offsetof(S2DMatchPolicyNet, {f}));\n' for f in fields) +
                     '  printf(" %zu", sizeof(S2DMatchNet));\n  return 0;\n}\n')
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(probe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got[0] == C.sizeof(M.S2DMatchPolicyNet)
    assert got[1:-1] == [getattr(M.S2DMatchPolicyNet, f).offset for f in fields]
    assert got[-1] == C.sizeof(M.S2DMatchNet)              # the Q-network's struct keeps its layout
    g.build_hip()
    lib = M.bind(_capi.load_library())
    fn = lib.s2d_match_set_policy_network
    assert fn.restype is C.c_int and fn.argtypes == [C.c_void_p, C.c_int, C.c_void_p]
    assert fn(None, 0, None) == _capi.S2D_EINVAL and b'NULL handle' in lib.s2d_last_error()
    ro = lib.s2d_match_rollout_policy
    assert ro.restype is C.c_int and len(ro.argtypes) == 10
    assert ro(None, 1, None, None, None, None, None, 0, None, None) == _capi.S2D_EINVAL and b'NULL handle' in lib.s2d_last_error()


# ------------------------------------------------------------------------------------------ MatchPolicyActor
def _module(h1, h2, k, seed, act=torch.nn.Tanh, act2=None, bias=True, in_dim=224):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(in_dim, h1), act(), torch.nn.Linear(h1, h2, bias=bias), (act2 or act)(),
                               torch.nn.Linear(h2, k))


def test_actor_module_forms():
    from soccer2d_amd.actor import MatchPolicyActor, match_param_count
    table = np.arange(15, dtype=np.float32).reshape(5, 3)
    for act, name in ((torch.nn.ReLU, 'relu'), (torch.nn.Tanh, 'tanh')):
        m = _module(32, 16, 5, 1, act)
        a = MatchPolicyActor.from_module(m, table, device='cpu')
        assert (a.hidden1, a.hidden2, a.n_actions, a.activation, a.obs, a.kind) == (32, 16, 5, name, 'agent', 'policy')
        assert a.shapes() == ((32, 224), (32,), (16, 32), (16,), (5, 16), (5,))
        want = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
        assert a.params.numel() == match_param_count(32, 16, 5) and torch.equal(a.params, want)
        assert torch.equal(a.table, torch.as_tensor(table))
        assert a.c_struct(0x7FF).activation == (1 if name == 'tanh' else 0)
    # SB3's pair [mlp_extractor.policy_net, action_net], behind a Flatten
    body = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(224, 16), torch.nn.Tanh(), torch.nn.Linear(16, 16), torch.nn.Tanh())
    a = MatchPolicyActor.from_module([body, torch.nn.Linear(16, 5)], table, device='cpu')
    assert (a.hidden1, a.hidden2, a.n_actions, a.activation) == (16, 16, 5, 'tanh')
    with pytest.raises(ValueError, match='ReLU or Tanh'):
        MatchPolicyActor.from_module(_module(16, 16, 5, 1, torch.nn.ReLU, torch.nn.Tanh), table, device='cpu')   # mixed
    with pytest.raises(ValueError, match='ReLU or Tanh'):
        MatchPolicyActor.from_module(_module(16, 16, 5, 1, torch.nn.Sigmoid), table, device='cpu')
    with pytest.raises(ValueError, match='must be one of'):
        MatchPolicyActor.from_module(_module(24, 16, 5, 1), table, device='cpu')                                  # wrong width
    with pytest.raises(ValueError, match='must be one of'):
        MatchPolicyActor.from_module(_module(16, 80, 5, 1), np.zeros((5, 3)), device='cpu')
    with pytest.raises(ValueError, match='bias'):
        MatchPolicyActor.from_module(_module(16, 16, 5, 1, bias=False), table, device='cpu')
    with pytest.raises(ValueError, match='shapes'):
        MatchPolicyActor.from_module(_module(16, 16, 5, 1, in_dim=192), table, device='cpu')                      # a see-row module
    with pytest.raises(ValueError, match='activation'):
        MatchPolicyActor(16, 16, 5, activation='relu', device='cpu').load_from(_module(16, 16, 5, 1))
    with pytest.raises(ValueError, match='activation'):
        MatchPolicyActor(16, 16, 5, activation='gelu', device='cpu')
    for k in (0, 65):
        with pytest.raises(ValueError, match='n_actions'):
            MatchPolicyActor(16, 16, k, device='cpu')
    with pytest.raises(ValueError, match='see'):
        MatchPolicyActor(16, 16, 5, device='cpu', obs='see')
    with pytest.raises(ValueError, match='see'):
        MatchPolicyActor.from_module(_module(16, 16, 5, 1), table, device='cpu', obs='see')
    with pytest.raises(ValueError, match='table'):
        MatchPolicyActor(16, 16, 5, device='cpu').set_table(np.zeros((5, 5)))
    assert MatchPolicyActor(64, 64, 1, device='cpu').n_actions == 1 and MatchPolicyActor(16, 16, 64, device='cpu').n_actions == 64


def test_actor_snapshot_and_deterministic_word():
    from soccer2d_amd.actor import MatchPolicyActor
    m = _module(32, 16, 5, 2)
    table = np.arange(15, dtype=np.float32).reshape(5, 3)
    a = MatchPolicyActor.from_module(m, table, device='cpu')
    assert a.deterministic is False and a.deterministic_tensor.dtype == torch.int32 and int(a.deterministic_tensor) == 0
    word = a.deterministic_tensor.data_ptr()
    a.deterministic = True
    assert a.deterministic is True and int(a.deterministic_tensor) == 1 and a.deterministic_tensor.data_ptr() == word
    s = a.snapshot()
    assert (s.hidden1, s.hidden2, s.n_actions, s.activation, s.device, s.deterministic) == (32, 16, 5, 'tanh', a.device, True)
    assert a.snapshot(deterministic=False).deterministic is False and int(a.snapshot(deterministic=False).deterministic_tensor) == 0
    assert torch.equal(s.params, a.params) and torch.equal(s.table, a.table)
    for x, y in ((s.params, a.params), (s.table, a.table), (s.deterministic_tensor, a.deterministic_tensor)):
        assert x.data_ptr() != y.data_ptr()
    old_params, old_table = a.params.clone(), a.table.clone()
    with torch.no_grad():
        m[0].weight.add_(1.0)
    a.sync()
    a.set_table(table + 1.0)
    a.deterministic = False
    assert not torch.equal(a.params, old_params)
    assert torch.equal(s.params, old_params) and torch.equal(s.table, old_table) and int(s.deterministic_tensor) == 1
    with pytest.raises(ValueError):
        s.sync()                                           # a snapshot has no module: nothing can move it
    cs = s.c_struct(0x3FF800)
    assert (cs.h1, cs.h2, cs.n_actions, cs.slot_mask, cs.activation) == (32, 16, 5, 0x3FF800, 1)
    assert (cs.params, cs.deterministic, cs.table) == (s.params.data_ptr(), s.deterministic_tensor.data_ptr(), s.table.data_ptr())


# ------------------------------------------------------------------------------------------ binding validation
class _Lib:
    """records the calls that reach the library; every call succeeds"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name,) + tuple(a for a in args[1:2] if isinstance(a, int)))
            return 0
        return fn


def _bare_engine(n=4):
    from soccer2d_amd.match import MatchEngine
    eng = MatchEngine.__new__(MatchEngine)                 # no GPU here: the argument checks run before the library call
    eng.lib, eng._h, eng.device, eng.num_envs = _Lib(), None, torch.device('cpu'), n
    eng.network, eng.network_mask = None, 0
    eng.opponent_network, eng.opponent_mask = None, 0
    eng.vision = None
    eng._stream = lambda: None
    return eng


def test_set_network_dispatches_on_the_actor_kind():
    from soccer2d_amd.actor import MatchPolicyActor, MatchQNetActor
    from soccer2d_amd.match import Soccer2DMatchVecEnv, _is_match_actor
    eng = _bare_engine()
    p = MatchPolicyActor(16, 16, 4, device='cpu')
    q = MatchQNetActor(32, 16, 7, device='cpu')
    assert _is_match_actor(p) and _is_match_actor(q) and not _is_match_actor('scripted')
    assert Soccer2DMatchVecEnv.spaces(p, 'agent')[0].shape == (11, 224)
    for slots in (0, 1 << 22, 'middle', True, 1.5):
        with pytest.raises(ValueError):
            eng.set_network(p, slots)
        with pytest.raises(ValueError):
            eng.set_opponent_network(p, slots)
    other = MatchPolicyActor(16, 16, 4, device='cpu')
    other.device = torch.device('meta')
    for setter in (eng.set_network, eng.set_opponent_network):
        with pytest.raises(ValueError, match='engine on'):
            setter(other, 'right')
    assert eng.lib.calls == [] and eng.network is None and eng.opponent_network is None
    eng.set_network(p, 'left')
    assert eng.lib.calls == [('s2d_match_set_policy_network', 0)] and eng.network is p and eng.network_mask == 0x7FF
    for bad in ('all', 1 << 10):
        with pytest.raises(ValueError, match='overlap'):
            eng.set_opponent_network(q, bad)
        with pytest.raises(ValueError, match='overlap'):
            eng.set_opponent_network(p.snapshot(), bad)
    assert eng.opponent_network is None and len(eng.lib.calls) == 1
    eng.set_opponent_network(q)                            # policy + Q-network
    assert eng.lib.calls[-1] == ('s2d_match_set_opponent_network',) and eng.opponent_mask == 0x3FF800
    snap = p.snapshot(deterministic=True)
    eng.set_opponent_network(snap, 'right')                # policy + policy: replaces the Q-network in that role
    assert eng.lib.calls[-1] == ('s2d_match_set_policy_network', 1) and eng.opponent_network is snap
    with pytest.raises(ValueError, match='overlap'):
        eng.set_network(q, 'all')                          # the first role against the set opponent, whatever the kinds
    eng.set_network(q, 'left')                             # Q-network in role 0 + policy in role 1
    assert eng.lib.calls[-1] == ('s2d_match_set_network',) and eng.network is q
    eng.set_opponent_network(None)
    assert eng.opponent_network is None and eng.opponent_mask == 0 and eng.network is q
    eng.set_network(None)                                  # clears everything
    assert (eng.network, eng.network_mask, eng.opponent_network, eng.opponent_mask) == (None, 0, None, 0)
    assert [c[0] for c in eng.lib.calls[-3:]] == ['s2d_match_set_network', 's2d_match_set_opponent_network', 's2d_match_set_see_network']
    # a see network is the engine's only one
    see = MatchQNetActor(16, 16, 4, device='cpu', obs='see')
    eng.network, eng.network_mask = see, 0x7FF
    n_calls = len(eng.lib.calls)
    with pytest.raises(ValueError, match='see network'):
        eng.set_opponent_network(p, 'right')
    assert len(eng.lib.calls) == n_calls


def test_rollout_logp_buffer_validation():
    from soccer2d_amd.actor import MatchPolicyActor, MatchQNetActor
    eng = _bare_engine(4)
    eng.set_network(MatchPolicyActor(16, 16, 4, device='cpu'), 'all')
    T = 3
    base = dict(reward=torch.zeros((T, 4)), mode=torch.zeros((T, 4), dtype=torch.int32), done=torch.zeros((T, 4), dtype=torch.uint8))
    out = eng.rollout(T, out=dict(base), with_obs=False, logp=True)
    assert eng.lib.calls[-1][0] == 's2d_match_rollout_policy'
    assert out['logp'].dtype == torch.float32 and tuple(out['logp'].shape) == (T, 4, 22)
    out = eng.rollout(T, out=dict(base), with_obs=False, logp=True, net_index=True, agent_obs='left')
    assert eng.lib.calls[-1][0] == 's2d_match_rollout_policy'
    assert tuple(out['net_index'].shape) == (T, 4, 22) and tuple(out['agent_obs'].shape) == (T, 4, 11, 224)
    eng.rollout(T, out=dict(base), with_obs=False, net_index=True)
    assert eng.lib.calls[-1][0] == 's2d_match_rollout_net'                  # without logp: the entry point it was
    n_calls = len(eng.lib.calls)
    for bad in (torch.zeros((T, 4, 22), dtype=torch.float64), torch.zeros((T - 1, 4, 22)), torch.zeros((T, 4, 21)),
                torch.zeros((T, 3, 22)), torch.zeros((T, 4, 44))[:, :, ::2]):
        with pytest.raises(ValueError, match='logp'):
            eng.rollout(T, out=dict(base, logp=bad), with_obs=False, logp=True)
    assert len(eng.lib.calls) == n_calls
    big = torch.zeros((T + 2, 4, 22))
    assert eng.rollout(T, out=dict(base, logp=big), with_obs=False, logp=True)['logp'] is big
    eng.network = MatchQNetActor(16, 16, 4, device='cpu', obs='see')
    with pytest.raises(ValueError, match='policy head'):
        eng.rollout(T, out=dict(base), with_obs=False, logp=True)


# ------------------------------------------------------------------------------------------ the sampler
def test_sampler_frequencies_and_logp(ref):
    """2^18 draws at consecutive ticks of one match and slot, K = 16, against the float64 softmax: chi-square with 15 degrees of
    freedom, accepted below the 1 - 1e-6 quantile (test_policy_host.py::test_categorical_frequencies' acceptance)"""
    y = fixed_logits()
    prob = softmax64(y)
    n = 1 << 18
    a, lp = MP.head(ref, np.broadcast_to(y, (n, 16)), SEED, 12345, np.arange(n), 7, det=0)
    assert a.min() >= 0 and a.max() <= 15
    stat = chi2_stat(np.bincount(a, minlength=16).astype(np.float64), prob)
    assert chi2_sf_odd(stat, 15) > 1e-6, stat
    assert np.abs(lp.astype(np.float64) - np.log(prob)[a]).max() < 1e-6


def test_logp_against_float64_log_softmax(ref):
    """logits in [-8, 8]: logp of the index taken within 1e-6 of float64 log_softmax (test_policy_host.py's bound), both modes"""
    rs = np.random.RandomState(77)
    y = rs.uniform(-8, 8, (4096, 16)).astype(np.float32)
    want = np.log(softmax64(y))
    for det in (0, 1):
        a, lp = MP.head(ref, y, SEED, np.arange(4096), rs.randint(0, 6000, 4096), rs.randint(0, 22, 4096), det=det)
        err = np.abs(lp.astype(np.float64) - want[np.arange(4096), a]).max()
        print(f'det={det}: max |logp - float64| = {err:.3e}')
        assert err < 1e-6
        if det:
            assert np.array_equal(a, y.argmax(axis=1))


def test_word_z_is_the_uniform_word(ref):
    """the head reads word z of the slot's block: changing x and y (the epsilon-greedy head's words) and w leaves the index,
    changing z alone moves it for some draw; and the block is counter = tick, stream 7, block = slot of the match's id"""
    import qnet_ref as Q
    rs = np.random.RandomState(5)
    n = 512
    y = np.broadcast_to(fixed_logits(), (n, 16))
    gid, tick, slot = rs.randint(0, 1 << 40, n).astype(np.uint64), rs.randint(0, 6000, n), rs.randint(0, 22, n)
    blocks = np.stack([MP.block(ref, SEED, g, t, s) for g, t, s in zip(gid, tick, slot)])
    w = Q.philox(gid & np.uint64(0xFFFFFFFF), gid >> np.uint64(32), tick.astype(np.uint64),
                 (np.uint64(7) << np.uint64(16)) | slot.astype(np.uint64), SEED & 0xFFFFFFFF, SEED >> 32)
    assert np.array_equal(blocks, np.stack([np.asarray(v, dtype=np.uint32) for v in w], axis=1))
    a0, lp0 = MP.head(ref, y, SEED, gid, tick, slot, det=0)
    a1, lp1 = MP.head_words(ref, y, blocks, det=0)
    assert np.array_equal(a0, a1) and np.array_equal(lp0.view(np.int32), lp1.view(np.int32))
    other = blocks.copy()
    other[:, [0, 1, 3]] = rs.randint(0, 2 ** 32, (n, 3), dtype=np.uint64).astype(np.uint32)
    a2, lp2 = MP.head_words(ref, y, other, det=0)
    assert np.array_equal(a2, a0) and np.array_equal(lp2.view(np.int32), lp0.view(np.int32))
    onlyz = blocks.copy()
    onlyz[:, 2] = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    assert (MP.head_words(ref, y, onlyz, det=0)[0] != a0).any()
    assert np.array_equal(MP.head_words(ref, y, onlyz, det=1)[0], np.full(n, y[0].argmax()))   # greedy: no word is read


def _words(z):
    w = np.zeros((len(z), 4), dtype=np.uint32)
    w[:, 2] = z
    return w


def test_edge_rows_by_value(ref):
    # K = 1: index 0, logp exactly 0, whatever the logit and the word
    y1 = np.array([[3.5], [-20.0], [0.0]], dtype=np.float32)
    for det in (0, 1):
        a, lp = MP.head_words(ref, y1, _words([0, 0xFFFFFFFF, 12345]), det)
        assert np.array_equal(a, [0, 0, 0]) and np.array_equal(lp.view(np.int32), np.zeros(3, dtype=np.int32))
    # all logits equal: every exp is 1, S = K, index = floor(u K) (u K is exact for K = 16), one logp value: -log_spec(16)
    n = 1 << 16
    z = np.random.RandomState(9).randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    a, lp = MP.head_words(ref, np.full((n, 16), 0.75, dtype=np.float32), _words(z), 0)
    assert np.array_equal(a, (z >> 8).astype(np.int64) * 16 >> 24)
    stat = chi2_stat(np.bincount(a, minlength=16).astype(np.float64), np.full(16, 1 / 16))
    assert chi2_sf_odd(stat, 15) > 1e-6, stat
    assert len(set(lp.view(np.int32).tolist())) == 1 and abs(float(lp[0]) + math.log(16.0)) < 1e-6
    # the ends of the draw: w = 0 -> u = 0 -> the first index with a positive term; w = 2^32 - 1 -> u = 1 - 2^-24: the last index
    # whose running sum still passes u S; if rounding lets none pass, the first maximum
    y = np.array([[0.0, 1.0, 2.0, 1.0], [2.0, 2.0, -1.0, 0.0]], dtype=np.float32)
    a, lp = MP.head_words(ref, y, _words([0, 0]), 0)
    assert np.array_equal(a, [0, 0])
    want = np.log(softmax64(y))
    assert np.abs(lp - want[[0, 1], a]).max() < 1e-6
    a, lp = MP.head_words(ref, y, _words([0xFFFFFFFF, 0xFFFFFFFF]), 0)
    assert np.array_equal(a, [3, 3]) and np.abs(lp - want[[0, 1], a]).max() < 1e-6
    # deterministic: the first maximum on ties
    a, lp = MP.head_words(ref, y, _words([0xFFFFFFFF, 0xFFFFFFFF]), 1)
    assert np.array_equal(a, [2, 0]) and np.abs(lp - want[[0, 1], a]).max() < 1e-6
    # a NaN logit: `v > m` is false for a NaN, so a NaN at index 0 stays the "maximum" (g = 0) and a NaN elsewhere never becomes
    # it; S is NaN either way, no running sum exceeds a NaN target, so the index is g in both modes and logp is NaN
    nan, inf = np.float32('nan'), np.float32('inf')
    rows = np.array([[nan, 1.0, 3.0, 2.0], [1.0, nan, 3.0, 2.0], [1.0, 3.0, 2.0, nan]], dtype=np.float32)
    for det in (0, 1):
        a, lp = MP.head_words(ref, rows, _words([1 << 31] * 3), det)
        assert np.array_equal(a, [0, 2, 1]) and np.isnan(lp).all()
    # a -inf logit: exp_spec(-inf) is NaN (its range reduction forms inf - inf), so S is NaN as above: the first maximum of the
    # finite logits, logp NaN -- masking an action with -inf is not offered (include/s2d_match.h)
    rows = np.array([[-inf, 1.0, 3.0, 2.0], [1.0, 3.0, -inf, 3.0]], dtype=np.float32)
    for det in (0, 1):
        a, lp = MP.head_words(ref, rows, _words([1 << 31] * 2), det)
        assert np.array_equal(a, [2, 1]) and np.isnan(lp).all()


@pytest.mark.parametrize('h1,h2,k', [(16, 16, 1), (32, 48, 17), (64, 64, 64)])
def test_forward_activations(ref, h1, h2, k):
    """relu: mnet_forward bitwise; tanh: a plain loop of fmaf chains with tanh_spec on the hidden units"""
    rs = np.random.RandomState(h1 + k)
    params = (rs.standard_normal(MP.param_count(h1, h2, k)) * 0.2).astype(np.float32)
    x = (rs.standard_normal((5, 224)) * 2).astype(np.float32)
    x[0, :8] = [np.nan, -0.0, 0.0, np.inf, -np.inf, 1e30, -1e30, 1e-40]
    q = np.zeros((5, k), dtype=np.float32)
    ref.mnet_forward(5, x.ctypes.data, params.ctypes.data, h1, h2, k, q.ctypes.data)
    assert np.array_equal(MP.forward(ref, x, params, h1, h2, k, 0).view(np.int32), q.view(np.int32))
    o = np.cumsum([0, 224 * h1, h1, h1 * h2, h2, h2 * k, k])
    W1, b1, W2, b2, W3, b3 = (params[o[i]:o[i + 1]] for i in range(6))
    W1, W2, W3 = W1.reshape(h1, 224), W2.reshape(h2, h1), W3.reshape(k, h2)

    def dense(W, b, v):
        out = np.zeros(len(b), dtype=np.float32)
        for j in range(len(b)):
            acc = np.float64(b[j])
            for i in range(W.shape[1]):                    # fmaf: the exact product and sum in float64 (24 + 24 + guard bits
                acc = np.float64(np.float32(np.float64(W[j, i]) * np.float64(v[i]) + acc))   # fit 53 only loosely: compare to ulps)
            out[j] = acc
        return out

    got = MP.forward(ref, x[1:], params, h1, h2, k, 1)
    with np.errstate(all='ignore'):
        for r in range(1, 5):
            a1 = MP.tanh_spec(ref, dense(W1, b1, x[r]))
            a2 = MP.tanh_spec(ref, dense(W2, b2, a1))
            want = dense(W3, b3, a2)
            assert np.abs(got[r - 1] - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
    assert np.abs(MP.tanh_spec(ref, np.linspace(-12, 12, 4801).astype(np.float32)) - np.tanh(np.linspace(-12, 12, 4801))).max() < 5e-7
    assert not np.array_equal(got, MP.forward(ref, x[1:], params, h1, h2, k, 0))
