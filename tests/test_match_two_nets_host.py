"""Host-side checks of the 11v11 opponent network (s2d_match_set_opponent_network): MatchQNetActor.snapshot() copies and does
not alias, MatchEngine.set_opponent_network validates its arguments before it reaches the library, league.play_networks
validates its own, and the new entry point is declared, bound and exported."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip('torch')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module(h1, h2, k, seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(224, h1), torch.nn.ReLU(), torch.nn.Linear(h1, h2), torch.nn.ReLU(),
                               torch.nn.Linear(h2, k))


def test_snapshot_copies_and_does_not_alias():
    from soccer2d_amd.actor import MatchQNetActor
    m = _module(32, 16, 5, 1)
    table = np.arange(15, dtype=np.float32).reshape(5, 3)
    a = MatchQNetActor.from_module(m, table, device='cpu', epsilon=0.2)
    s = a.snapshot()
    assert (s.hidden1, s.hidden2, s.n_actions, s.obs, s.device) == (32, 16, 5, 'agent', a.device)
    assert s.epsilon == 0.0 and float(s.epsilon_tensor) == 0.0 and a.epsilon == pytest.approx(0.2)
    assert a.snapshot(epsilon=0.05).epsilon == pytest.approx(0.05)
    assert torch.equal(s.params, a.params) and torch.equal(s.table, a.table)
    for x, y in ((s.params, a.params), (s.table, a.table), (s.epsilon_tensor, a.epsilon_tensor)):
        assert x.data_ptr() != y.data_ptr()
    old_params, old_table = a.params.clone(), a.table.clone()
    with torch.no_grad():
        m[0].weight.add_(1.0)
    a.sync()
    a.set_table(table + 1.0)
    a.epsilon = 0.9
    assert not torch.equal(a.params, old_params)
    assert torch.equal(s.params, old_params) and torch.equal(s.table, old_table) and s.epsilon == 0.0
    with pytest.raises(ValueError):
        s.sync()                                           # a snapshot has no module: nothing can move it
    cs = s.c_struct(0x3FF800)
    assert (cs.h1, cs.h2, cs.n_actions, cs.slot_mask) == (32, 16, 5, 0x3FF800)
    assert cs.params == s.params.data_ptr() and cs.table == s.table.data_ptr() and cs.epsilon == s.epsilon_tensor.data_ptr()
    see = MatchQNetActor(16, 16, 3, device='cpu', obs='see').snapshot()
    assert see.obs == 'see' and tuple(see.table.shape) == (3, 5)


class _Lib:
    """records the calls that reach the library; every call succeeds"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return 0
        return fn


def _bare_engine():
    from soccer2d_amd.match import MatchEngine
    eng = MatchEngine.__new__(MatchEngine)                 # no GPU here: the argument checks run before the library call
    eng.lib, eng._h, eng.device = _Lib(), None, torch.device('cpu')
    eng.network, eng.network_mask = None, 0
    eng.opponent_network, eng.opponent_mask = None, 0
    eng.vision = None
    return eng


def test_set_opponent_network_argument_validation():
    from soccer2d_amd.actor import MatchQNetActor
    eng = _bare_engine()
    a = MatchQNetActor(16, 16, 4, device='cpu')
    b = MatchQNetActor(32, 16, 7, device='cpu')
    for slots in (0, 1 << 22, 'middle', True, 1.5):
        with pytest.raises(ValueError):
            eng.set_opponent_network(b, slots)
    with pytest.raises(ValueError, match='see'):
        eng.set_opponent_network(MatchQNetActor(16, 16, 4, device='cpu', obs='see'), 'right')
    other = MatchQNetActor(16, 16, 4, device='cpu')
    other.device = torch.device('meta')
    with pytest.raises(ValueError, match='engine on'):
        eng.set_opponent_network(other, 'right')
    assert eng.lib.calls == [] and eng.opponent_network is None and eng.opponent_mask == 0
    eng.set_network(a, 'left')
    with pytest.raises(ValueError, match='overlap'):
        eng.set_opponent_network(b, 'all')
    with pytest.raises(ValueError, match='overlap'):
        eng.set_opponent_network(b, 1 << 10)
    assert eng.opponent_network is None
    eng.set_opponent_network(b)                            # the default: the right team
    assert eng.opponent_network is b and eng.opponent_mask == 0x3FF800 and eng.network is a and eng.network_mask == 0x7FF
    assert eng.lib.calls == ['s2d_match_set_network', 's2d_match_set_opponent_network']
    eng.set_opponent_network(None)                         # clears the opponent only
    assert eng.opponent_network is None and eng.opponent_mask == 0 and eng.network is a
    eng.set_opponent_network(b, 0x3FF800)
    eng.set_network(None)                                  # clears everything
    assert (eng.network, eng.network_mask, eng.opponent_network, eng.opponent_mask) == (None, 0, None, 0)
    assert eng.lib.calls[-3:] == ['s2d_match_set_network', 's2d_match_set_opponent_network', 's2d_match_set_see_network']


def test_play_networks_argument_validation():
    from soccer2d_amd import league
    eng = _bare_engine()
    for kw in (dict(n_cycles=-1), dict(n_cycles=4, chunk=0)):
        with pytest.raises(ValueError):
            league.play_networks(eng, None, None, **kw)
    assert eng.lib.calls == []


def test_entry_point_is_declared_bound_and_exported():
    import __graft_entry__ as g
    from soccer2d_amd import _capi, _capi_match as M
    hdr = open(os.path.join(ROOT, 'include', 's2d_match.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint\s+s2d_match_set_opponent_network\s*\(\s*S2DMatchHandle\s+h\s*,\s*const\s+S2DMatchNet\s*\*\s*net\s*\)\s*;', code)
    protos = {p[0]: p for p in M.MATCH_PROTOTYPES}
    assert protos['s2d_match_set_opponent_network'][1:] == protos['s2d_match_set_network'][1:] == (C.c_int, (C.c_void_p, C.c_void_p))
    g.build_hip()
    lib = M.bind(_capi.load_library())
    fn = lib.s2d_match_set_opponent_network
    assert fn.restype is C.c_int and fn.argtypes == [C.c_void_p, C.c_void_p]
    assert fn(None, None) == _capi.S2D_EINVAL and b'NULL handle' in lib.s2d_last_error()
