"""ctypes binding of tests/hear_ref.c, the host restatement of the audio layer (include/s2d_match.h, "Hearing").
TEST INFRASTRUCTURE: compiled on demand with -ffp-contract=off (the fp32 contract)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hear_ref.c')
# what the layer reads of the engine (S2DMatchBuffers names), the optional neck plane, then the hear planes
FLOAT_PLANES = ('x', 'y', 'body')
ENGINE_KEYS = FLOAT_PLANES + ('card', 'tick')
HEAR_PLANES = ('cap_our', 'cap_opp', 'attention', 'hear')
DIM, REC, SAY_ROW, SAY_WORDS = 32, 16, 12, 10
# defaults of s2d_match_hear_default_params, restated (the host tests compare the library's with these)
DEFAULTS = dict(audio_cut_dist=50.0, hear_max=1.0, hear_inc=1.0, hear_decay=1.0, say_msg_size=10.0, say_levels=73.0)
# words of one record
HEARD, SENDER, DIR, MISSED, CAP, ATT, PAY = 0, 1, 2, 3, 4, 5, 6


class HearParams(C.Structure):
    _fields_ = [('cut', C.c_float), ('half', C.c_float), ('inv_half', C.c_float), ('hear_max', C.c_int32), ('hear_inc', C.c_int32),
                ('hear_decay', C.c_int32), ('msg_size', C.c_int32), ('seed', C.c_uint64), ('env_id_offset', C.c_uint64)]


class HearState(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ENGINE_KEYS + ('neck',) + HEAR_PLANES]


def build(outdir):
    so = os.path.join(str(outdir), 'libhear_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC, '-lm'], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    L.s2dhear_step.restype = None
    L.s2dhear_step.argtypes = [C.c_int64, C.POINTER(HearState), C.POINTER(HearParams), C.c_void_p, C.c_void_p]
    L.s2dhear_reset.restype = None
    L.s2dhear_reset.argtypes = [C.c_int64, C.POINTER(HearState), C.POINTER(HearParams), C.c_void_p]
    L.s2dhear_draw.restype = C.c_uint32
    L.s2dhear_draw.argtypes = [C.POINTER(HearParams), C.c_uint64, C.c_uint32, C.c_int, C.c_int]
    return L


def params(seed=0x5EED, env_id_offset=0, **over):
    """HearParams as the layer derives them from an S2DHearParams with `over` written over the defaults: each word rounded once,
    half = the float of (say_levels - 1) / 2, inv_half = the float of the double 1 / half"""
    v = dict(DEFAULTS)
    for k, x in over.items():
        assert k in v, k
        v[k] = x
    P = HearParams()
    P.cut = np.float32(v['audio_cut_dist'])
    half = (v['say_levels'] - 1.0) / 2.0
    P.half, P.inv_half = np.float32(half), np.float32(1.0 / half)
    P.hear_max, P.hear_inc, P.hear_decay = int(v['hear_max']), int(v['hear_inc']), int(v['hear_decay'])
    P.msg_size = int(v['say_msg_size'])
    P.seed, P.env_id_offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_id_offset)
    return P


def blank_state(n=1, prm=None):
    """zeroed engine words (everybody at the origin, body 0, no cards, tick 0), no neck plane, the hear planes as after a reset"""
    prm = params() if prm is None else prm
    s = {k: np.zeros((n, 24), dtype=np.float32) for k in FLOAT_PLANES}
    s['card'] = np.zeros((n, 24), dtype=np.int32)
    s['tick'] = np.zeros((n,), dtype=np.int32)
    s['neck'] = None
    s.update(reset_planes(n, prm))
    return s


def reset_planes(n, prm):
    hear = np.zeros((n, 22, DIM), dtype=np.float32)
    hear[:, :, CAP] = hear[:, :, REC + CAP] = prm.hear_max
    return {'cap_our': np.full((n, 24), prm.hear_max, dtype=np.int32), 'cap_opp': np.full((n, 24), prm.hear_max, dtype=np.int32),
            'attention': np.full((n, 24), -1, dtype=np.int32), 'hear': hear}


def blank_say(n=1):
    return np.zeros((n, 22, SAY_ROW), dtype=np.float32)


def _arrays(state):
    """contiguous copies of the right types in the order of HearState (the hear planes are the outputs); neck may be None"""
    out = []
    for k in ENGINE_KEYS + ('neck',) + HEAR_PLANES:
        if k == 'neck' and state.get('neck') is None:
            out.append(None)
            continue
        dt = np.float32 if k in FLOAT_PLANES + ('neck', 'hear') else np.int32
        out.append(np.array(state[k], dtype=dt, order='C'))
    n = out[0].shape[0]
    for k, a in zip(ENGINE_KEYS + ('neck',) + HEAR_PLANES, out):
        if a is not None:
            assert a.shape == {'tick': (n,), 'hear': (n, 22, DIM)}.get(k, (n, 24)), (k, a.shape)
    return n, out


def _planes(arrs):
    return dict(zip(HEAR_PLANES, arrs[-4:]))


def step(L, state, prm, say=None, done=None):
    """one cycle: returns the four new hear planes (the input is not modified).  say [N, 22, 12] or None, done [N] or None"""
    n, arrs = _arrays(state)
    st = HearState(*[None if a is None else a.ctypes.data for a in arrs])
    sy = None if say is None else np.ascontiguousarray(say, dtype=np.float32)
    assert sy is None or sy.shape == (n, 22, SAY_ROW)
    dn = None if done is None else np.ascontiguousarray(done, dtype=np.uint8)
    assert dn is None or dn.shape == (n,)
    L.s2dhear_step(n, C.byref(st), C.byref(prm), None if sy is None else sy.ctypes.data, None if dn is None else dn.ctypes.data)
    return _planes(arrs)


def reset(L, state, prm, mask=None):
    n, arrs = _arrays(state)
    st = HearState(*[None if a is None else a.ctypes.data for a in arrs])
    mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    L.s2dhear_reset(n, C.byref(st), C.byref(prm), None if mk is None else mk.ctypes.data)
    return _planes(arrs)


def draw(L, prm, e, tick, p, j):
    return int(L.s2dhear_draw(C.byref(prm), e, tick, p, j))


def mirror(state, say=None):
    """the mirrored state: teams swapped, positions negated, bodies turned by 180 degrees; necks, capacities, attention (own-frame)
    and hear rows move with their players.  Returns (state, say)"""
    perm = np.r_[11:22, 0:11, 22, 23]
    out = {}
    for k in ('x', 'y'):
        out[k] = (-np.asarray(state[k], dtype=np.float32))[:, perm]
    b = np.asarray(state['body'], dtype=np.float32)
    out['body'] = np.where(b > 0, b - np.float32(180.0), b + np.float32(180.0)).astype(np.float32)[:, perm]
    out['card'] = np.asarray(state['card'])[:, perm].copy()
    out['tick'] = np.asarray(state['tick']).copy()
    out['neck'] = None if state.get('neck') is None else np.asarray(state['neck'])[:, perm].copy()
    for k in ('cap_our', 'cap_opp', 'attention'):
        out[k] = np.asarray(state[k])[:, perm].copy()
    out['hear'] = np.asarray(state['hear'])[:, perm[:22]].copy()
    return out, (None if say is None else np.asarray(say)[:, perm[:22]].copy())
