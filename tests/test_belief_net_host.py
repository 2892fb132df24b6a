"""The belief network's host side without a device (include/s2d_match.h, "Belief network"): the ctypes struct against the header's
layout, the two prototypes, the actor classes' `obs` words."""
import ctypes as C
import os
import re

import pytest

from soccer2d_amd import _capi_match as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 's2d_match.h')


def _header_struct(name):
    """[(type text, field name)] of `typedef struct NAME { ... } NAME;`, comments stripped"""
    text = open(HEADER).read()
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), text, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = ' '.join(decl.split())
        if not decl:
            continue
        m = re.match(r'(.*?[\s\*])([A-Za-z_0-9, ]+)$', decl)
        typ, names = m.group(1).strip(), m.group(2)
        for nm in names.split(','):
            fields.append((typ, nm.strip()))
    return fields


CTYPE = {'int32_t': C.c_int32, 'uint32_t': C.c_uint32, 'const float *': C.c_void_p, 'const uint32_t *': C.c_void_p,
         'float *': C.c_void_p, 'S2DVisionParams': M.S2DVisionParams, 'S2DMatchVision': M.S2DMatchVision,
         'S2DBeliefParams': M.S2DBeliefParams}


def test_struct_matches_the_header():
    """field names, order and types of S2DMatchBeliefNet; its size is what a C compiler lays out for the header's struct"""
    hdr = _header_struct('S2DMatchBeliefNet')
    got = M.S2DMatchBeliefNet._fields_
    assert [n for _, n in hdr] == [n for n, _ in got]
    for (typ, name), (_, ct) in zip(hdr, got):
        assert CTYPE[typ] is ct, (name, typ, ct)
    # natural alignment, as the C ABI: 4 x 4 | 2 pointers | 19 doubles | 3 pointers | 2 x 4 | 2 pointers | 9 doubles | pointer | 4 + pad
    want = 16 + 16 + C.sizeof(M.S2DVisionParams) + 24 + 8 + 16 + C.sizeof(M.S2DBeliefParams) + 8 + 8
    assert C.sizeof(M.S2DVisionParams) == 19 * 8 and C.sizeof(M.S2DBeliefParams) == 9 * 8
    assert C.sizeof(M.S2DMatchBeliefNet) == want == 320
    assert M.S2DMatchBeliefNet.belief_mask.offset == want - 8 and M.S2DMatchBeliefNet.head.offset == 32 + 19 * 8 + 24


def test_prototypes():
    protos = {name: (res, args) for name, res, args in M.MATCH_PROTOTYPES}
    res, args = protos['s2d_match_set_belief_network']
    assert res is C.c_int and len(args) == 2
    res, args = protos['s2d_match_rollout_belief']
    assert res is C.c_int and len(args) == 12 and args[8] is C.c_uint32
    text = open(HEADER).read()
    decl = re.search(r'int s2d_match_rollout_belief\((.*?)\);', text, re.S).group(1)
    assert len(decl.split(',')) == 12
    assert 'S2DMatchBeliefNet' in re.search(r'int s2d_match_set_belief_network\((.*?)\);', text, re.S).group(1)


def test_default_obs_of_every_class_is_unchanged():
    import inspect
    from soccer2d_amd.actor import MatchPolicyActor, MatchQNetActor, MatchSeePolicyActor
    assert inspect.signature(MatchQNetActor.__init__).parameters['obs'].default == 'agent'
    assert inspect.signature(MatchPolicyActor.__init__).parameters['obs'].default == 'agent'
    assert inspect.signature(MatchSeePolicyActor.__init__).parameters['obs'].default == 'see'
    assert inspect.signature(MatchQNetActor.from_module).parameters['obs'].default == 'agent'
    assert inspect.signature(MatchSeePolicyActor.from_module).parameters['obs'].default == 'see'
    assert MatchSeePolicyActor.obs == 'see' and MatchPolicyActor.obs == 'agent'
    assert MatchSeePolicyActor.in_dim == 192 and MatchSeePolicyActor.table_width == 5


def test_obs_validation():
    """a bad `obs` is refused before any buffer is allocated (no device needed)"""
    from soccer2d_amd.actor import MatchPolicyActor, MatchQNetActor, MatchSeePolicyActor
    with pytest.raises(ValueError, match="'agent', 'see' or 'belief'"):
        MatchQNetActor(16, 16, 4, obs='state')
    with pytest.raises(ValueError, match='agent rows only'):
        MatchPolicyActor(16, 16, 4, obs='belief')
    with pytest.raises(ValueError, match="'see' or 'belief'"):
        MatchSeePolicyActor(16, 16, 4, obs='agent')


def test_snapshot_keeps_obs():
    """snapshot() builds its copy with the original's obs (the frozen copy itself needs a device: the constructor call is observed)"""
    from soccer2d_amd.actor import MatchQNetActor, MatchSeePolicyActor
    for cls, kw in ((MatchQNetActor, {}), (MatchSeePolicyActor, dict(activation='relu'))):
        seen = {}

        class Probe(cls):
            def __init__(self, *a, **k):                  # (no buffers: only the words snapshot() passes on)
                seen.update(k)

            def _frozen(self, other):
                return other
        p = Probe()
        p.hidden1, p.hidden2, p.n_actions, p.device, p.obs = 16, 16, 4, 'cpu', 'belief'
        p.activation, p._det_value = kw.get('activation'), False
        p.snapshot()
        assert seen['obs'] == 'belief', cls.__name__


def test_belief_struct_needs_the_layers():
    """c_struct of a belief actor names what is missing (checked before any pointer is read)"""
    from soccer2d_amd import actor as A

    class Fake:
        hidden1 = hidden2 = 16
        n_actions = 4
    with pytest.raises(ValueError, match='enable_vision'):
        A._belief_struct(Fake(), 1, None, None, None, None, 0)
    with pytest.raises(ValueError, match='enable_belief'):
        A._belief_struct(Fake(), 1, M.S2DVisionParams(), M.S2DMatchVision(), None, None, 0)
