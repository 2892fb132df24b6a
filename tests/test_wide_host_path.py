"""CPU checks of the one host path of the streamed-weight MLP's three users (csrc/s2d_wide_host.h, s2d_wide_pack.hip): the reach-ball
actors (s2d_debug_wide_forward, input width 10), the GoToCenter actors (s2d_gtc_debug_forward, 4) and the TD targets
(s2d_td_target_q, any width).  A shape off the grid is refused by all three with the same text behind their own prefix, before
any HIP call, and the three workspace and plan arithmetics are one.  The texts are pinned here as literals: they are what the
library said when each user had a copy of the checks (the plans' own expected values are in the three users' host tests)."""
import ctypes as C

import pytest

GOOD = dict(n_hidden=2, hidden=(12, 20), activation=1, n_out=17)
# the four ways off the grid -> the text behind the prefix
BAD = (('n_hidden', dict(n_hidden=6), 'n_hidden must be in [1, 5]'),
       ('n_hidden', dict(n_hidden=0), 'n_hidden must be in [1, 5]'),
       ('hidden', dict(hidden=(12, 22)), 'hidden widths must be multiples of 4 in [8, 400], and 0 past n_hidden'),
       ('hidden', dict(hidden=(404, 20)), 'hidden widths must be multiples of 4 in [8, 400], and 0 past n_hidden'),
       ('hidden', dict(hidden=(12, 20, 8)), 'hidden widths must be multiples of 4 in [8, 400], and 0 past n_hidden'),
       ('activation', dict(activation=3), 'activation must be 0 (ReLU), 1 (Tanh) or 2 (Sigmoid)'),
       ('activation', dict(activation=-1), 'activation must be 0 (ReLU), 1 (Tanh) or 2 (Sigmoid)'),
       ('n_out', dict(n_out=0), 'n_out must be in [1, 64]'),
       ('n_out', dict(n_out=65), 'n_out must be in [1, 64]'))
SHAPES = ((8,), (12, 20), (400, 300), (128, 64, 32, 16, 8))
OUTPUTS = (1, 16, 17, 64)


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi, gtc
    lib = _capi.load_library()
    gtc.bind(lib)
    return lib


def _fill(s, n_hidden, hidden, activation, n_out):
    s.n_hidden, s.activation, s.n_out = n_hidden, activation, n_out
    for l, w in enumerate(hidden):
        s.hidden[l] = w
    return s


def _wide(**kw):
    from soccer2d_amd import _capi
    return _fill(_capi.S2DWideNet(), **dict(GOOD, **kw))


def _td(n_in=10, **kw):
    from soccer2d_amd import _capi
    s = _fill(_capi.S2DTdNet(), **dict(GOOD, **kw))
    s.n_in = n_in
    return s


def _refusal(lib, rc):
    assert rc != 0
    return lib.s2d_last_error().decode()


@pytest.mark.parametrize('field,change,text', BAD, ids=[f'{b[0]}-{i}' for i, b in enumerate(BAD)])
def test_three_entry_points_refuse_a_bad_shape_alike(lib, field, change, text):
    """every pointer is NULL: the shape is looked at first, and nothing touches the device"""
    wide, td = _wide(**change), _td(**change)
    got = (_refusal(lib, lib.s2d_debug_wide_forward(C.byref(wide), None, 1, None, None, None, None)),
           _refusal(lib, lib.s2d_gtc_debug_forward(C.byref(wide), None, 1, None, None, None, None)),
           _refusal(lib, lib.s2d_td_target_q(1, C.byref(td), None, None, None, None, None, None, None, None)))
    assert got == ('s2d_debug_wide_forward: ' + text, 's2d_gtc_debug_forward: ' + text, 's2d_td_target_q: target: ' + text)
    # the online network of the same call: its own infix, the same text (the target's workspace is checked before it: a host array)
    good = _td()
    params, ws = (C.c_float * 4096)(), (C.c_char * (lib.s2d_td_workspace_bytes(C.byref(good)) + 256))()
    good.params = C.addressof(params) + (-C.addressof(params)) % 16
    good.workspace = C.addressof(ws) + (-C.addressof(ws)) % 256
    good.workspace_bytes = lib.s2d_td_workspace_bytes(C.byref(good))
    rc = lib.s2d_td_target_q(1, C.byref(good), C.byref(td), None, None, None, None, None, None, None)
    assert _refusal(lib, rc) == 's2d_td_target_q: online: ' + text


@pytest.mark.parametrize('field,change,text', BAD, ids=[f'{b[0]}-{i}' for i, b in enumerate(BAD)])
def test_workspace_bytes_of_a_bad_shape(lib, field, change, text):
    """0 off the grid.  The workspace does not depend on the activation and the three functions do not read it (include/s2d.h:
    "n_hidden, hidden and n_out are read"): with a bad activation they give the good shape's bytes, as they always have."""
    from soccer2d_amd.td import td_workspace_bytes
    got = (lib.s2d_td_workspace_bytes(C.byref(_td(**change))), lib.s2d_wide_workspace_bytes(C.byref(_wide(**change))),
           lib.s2d_gtc_actor_workspace_bytes(C.byref(_wide(**change))))
    if field == 'activation':
        assert got == (td_workspace_bytes(10, (12, 20), 17), td_workspace_bytes(10, (12, 20), 17), td_workspace_bytes(4, (12, 20), 17))
    else:
        assert got == (0, 0, 0)


def test_good_shape_passes_the_shape_check(lib):
    """the refusals above are the shape's: the good shape gets past it, to the next check"""
    wide, td = _wide(), _td()
    assert _refusal(lib, lib.s2d_debug_wide_forward(C.byref(wide), None, 1, None, None, None, None)) == \
        's2d_debug_wide_forward: params must be a non-NULL, 16-byte aligned device pointer'
    assert _refusal(lib, lib.s2d_gtc_debug_forward(C.byref(wide), None, 1, None, None, None, None)) == \
        's2d_gtc_debug_forward: params must be a non-NULL, 16-byte aligned device pointer'
    assert _refusal(lib, lib.s2d_td_target_q(1, C.byref(td), None, None, None, None, None, None, None, None)) == \
        's2d_td_target_q: target: params must be a non-NULL, 16-byte aligned device pointer'
    assert _refusal(lib, lib.s2d_td_target_q(1, C.byref(_td(n_in=257)), None, None, None, None, None, None, None, None)) == \
        's2d_td_target_q: target: n_in must be in [1, 256]'


@pytest.mark.parametrize('hidden', SHAPES, ids=lambda h: '-'.join(map(str, h)))
def test_one_workspace_and_plan_arithmetic(lib, hidden):
    from soccer2d_amd.gtc_actor import gtc_plan
    from soccer2d_amd.td import td_workspace_bytes
    from soccer2d_amd.wide_actor import wide_plan
    for a in OUTPUTS:
        assert td_workspace_bytes(10, hidden, a) == wide_plan(hidden, a)[3]
        assert td_workspace_bytes(4, hidden, a) == gtc_plan(hidden, a)[3]
        assert wide_plan(hidden, a, n_in=4, tail_words=256) == gtc_plan(hidden, a)
        # and the library's three functions say the same
        kw = dict(n_hidden=len(hidden), hidden=hidden, activation=0, n_out=a)
        assert lib.s2d_wide_workspace_bytes(C.byref(_wide(**kw))) == lib.s2d_td_workspace_bytes(C.byref(_td(10, **kw))) == wide_plan(hidden, a)[3]
        assert lib.s2d_gtc_actor_workspace_bytes(C.byref(_wide(**kw))) == lib.s2d_td_workspace_bytes(C.byref(_td(4, **kw))) == gtc_plan(hidden, a)[3]
