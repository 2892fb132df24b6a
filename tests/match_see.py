"""ctypes binding of tests/see_ref.c, the host restatement of the vision layer (include/s2d_match.h, "Vision").
TEST INFRASTRUCTURE: compiled on demand with -ffp-contract=off (the fp32 contract)."""
import ctypes as C
import os
import subprocess

import numpy as np

import agent_obs as A

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'see_ref.c')
# what the layer reads (S2DMatchBuffers names): [N][24] planes, [N] words, then the vision planes
FLOAT_PLANES = ('x', 'y', 'vx', 'vy', 'body', 'stamina', 'effort', 'recovery', 'stamina_capacity')
INT_PLANES = ('card',)
ENV_WORDS = ('cycle', 'mode', 'mode_side', 'tick')
VISION_PLANES = ('neck', 'view_width', 'see_wait')
ENGINE_KEYS = FLOAT_PLANES + INT_PLANES + ENV_WORDS
DIM = 192
# defaults of s2d_match_vision_default_params, restated (the host tests compare the library's with these)
DEFAULTS = dict(view_angle=(60.0, 120.0, 180.0), see_interval=(1.0, 2.0, 3.0), visible_distance=3.0, dist_quantize_step=0.1,
                dist_round=0.1, dist_chg_quantize=0.02, dir_chg_quantize=0.1, unum_far_length=20.0, unum_too_far_length=40.0,
                team_far_length=40.0, team_too_far_length=60.0, min_neck_moment=-180.0, max_neck_moment=180.0,
                min_neck_angle=-90.0, max_neck_angle=90.0)


class SeeParams(C.Structure):
    _fields_ = [('view_angle', C.c_float * 3), ('interval', C.c_int32 * 3)] + [(n, C.c_float) for n in (
        'visible', 'dist_q', 'inv_dist_q', 'dist_r', 'inv_dist_r', 'dchg_q', 'inv_dchg_q', 'rchg_q', 'inv_rchg_q',
        'unum_far', 'unum_too_far', 'inv_unum_band', 'team_far', 'team_too_far', 'inv_team_band',
        'min_moment', 'max_moment', 'min_neck', 'max_neck')] + [('seed', C.c_uint64), ('env_id_offset', C.c_uint64)]


class SeeState(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ENGINE_KEYS + VISION_PLANES]


def build(outdir):
    so = os.path.join(str(outdir), 'libsee_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC, '-lm'], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    L.s2dsee_see.restype = None
    L.s2dsee_see.argtypes = [C.c_int64, C.POINTER(SeeState), C.POINTER(SeeParams), C.c_uint32, C.c_void_p]
    L.s2dsee_vision_step.restype = None
    L.s2dsee_vision_step.argtypes = [C.c_int64, C.POINTER(SeeState), C.POINTER(SeeParams), C.c_void_p, C.c_void_p]
    L.s2dsee_dist.restype = None
    L.s2dsee_dist.argtypes = [C.c_int64, C.POINTER(SeeParams), C.c_void_p, C.c_void_p]
    return L


def params(seed=0x5EED, env_id_offset=0, **over):
    """SeeParams as the layer derives them from an S2DVisionParams with `over` written over the defaults: every word rounded to
    fp32 once, reciprocals the floats of the double quotients"""
    v = dict(DEFAULTS)
    for k, x in over.items():
        assert k in v, k
        v[k] = x
    f = np.float32
    P = SeeParams()
    for i in range(3):
        P.view_angle[i] = f(v['view_angle'][i])
        P.interval[i] = int(v['see_interval'][i])
    for name, key in (('dist_q', 'dist_quantize_step'), ('dist_r', 'dist_round'), ('dchg_q', 'dist_chg_quantize'),
                      ('rchg_q', 'dir_chg_quantize')):
        setattr(P, name, f(v[key]))
        setattr(P, 'inv_' + name, f(1.0 / v[key]))
    P.visible = f(v['visible_distance'])
    for kind in ('unum', 'team'):
        far, too = v[kind + '_far_length'], v[kind + '_too_far_length']
        setattr(P, kind + '_far', f(far))
        setattr(P, kind + '_too_far', f(too))
        setattr(P, f'inv_{kind}_band', f(1.0 / (too - far)) if too > far else f(0.0))
    P.min_moment, P.max_moment = f(v['min_neck_moment']), f(v['max_neck_moment'])
    P.min_neck, P.max_neck = f(v['min_neck_angle']), f(v['max_neck_angle'])
    P.seed, P.env_id_offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_id_offset)
    return P


def _arrays(state):
    """contiguous arrays of the right types, in the order of SeeState (kept alive by the caller)"""
    out = []
    for k in ENGINE_KEYS + VISION_PLANES:
        dt = np.float32 if k in FLOAT_PLANES or k == 'neck' else np.int32
        a = np.ascontiguousarray(state[k], dtype=dt)
        out.append(a)
    n = out[0].shape[0]
    for k, a in zip(ENGINE_KEYS + VISION_PLANES, out):
        assert a.shape == ((n,) if k in ENV_WORDS else (n, 24)), (k, a.shape)
    return n, out


def see(L, state, prm, mask=0x3FFFFF):
    """state: dict of numpy arrays named as in ENGINE_KEYS and VISION_PLANES -> float32 [N, popcount(mask), 192]"""
    n, arrs = _arrays(state)
    out = np.zeros((n, bin(mask).count('1'), DIM), dtype=np.float32)
    st = SeeState(*[a.ctypes.data for a in arrs])
    L.s2dsee_see(n, C.byref(st), C.byref(prm), mask, out.ctypes.data)
    return out


def vision_step(L, state, prm, view_actions=None, done=None):
    """one cycle of the vision state: returns the three new planes (the input is not modified)"""
    n, arrs = _arrays(state)
    arrs = [a.copy() if k in VISION_PLANES else a for k, a in zip(ENGINE_KEYS + VISION_PLANES, arrs)]
    st = SeeState(*[a.ctypes.data for a in arrs])
    act = None if view_actions is None else np.ascontiguousarray(view_actions, dtype=np.float32)
    assert act is None or act.shape == (n, 22, 2)
    dn = None if done is None else np.ascontiguousarray(done, dtype=np.uint8)
    assert dn is None or dn.shape == (n,)
    L.s2dsee_vision_step(n, C.byref(st), C.byref(prm), None if act is None else act.ctypes.data, None if dn is None else dn.ctypes.data)
    return {k: a for k, a in zip(ENGINE_KEYS + VISION_PLANES, arrs) if k in VISION_PLANES}


def dist_grid(L, prm, d):
    d = np.ascontiguousarray(d, dtype=np.float32)
    out = np.zeros_like(d)
    L.s2dsee_dist(d.size, C.byref(prm), d.ctypes.data, out.ctypes.data)
    return out


def blank_state(n=1):
    """zeroed state (engine words and vision planes) for hand-built scenes: everybody at the origin, vision as after a reset and
    one step (normal width, fresh)"""
    s = {k: np.zeros((n, 24), dtype=np.float32) for k in FLOAT_PLANES}
    s['card'] = np.zeros((n, 24), dtype=np.int32)
    s.update({k: np.zeros((n,), dtype=np.int32) for k in ENV_WORDS})
    s['neck'] = np.zeros((n, 24), dtype=np.float32)
    s['view_width'] = np.full((n, 24), 2, dtype=np.int32)
    s['see_wait'] = np.full((n, 24), 2, dtype=np.int32)
    return s


def random_vision(rng, n, prm, fresh_share=0.7):
    """random vision planes: necks on a 2^-10-degree grid in [-90, 90], all widths, a share of the players fresh"""
    neck = (rng.integers(-90 * 1024, 90 * 1024 + 1, (n, 24)) / 1024.0).astype(np.float32)
    width = rng.integers(1, 4, (n, 24)).astype(np.int32)
    interval = np.array([prm.interval[0], prm.interval[1], prm.interval[2]], dtype=np.int32)[width - 1]
    wait = np.where(rng.random((n, 24)) < fresh_share, interval, np.maximum(interval - 1, 1) * (interval > 1)).astype(np.int32)
    return {'neck': neck, 'view_width': width, 'see_wait': wait}


def random_state(rng, n, prm):
    """agent_obs.random_state plus ticks and random vision planes"""
    s = A.random_state(rng, n)
    out = {k: s[k] for k in ENGINE_KEYS if k != 'tick'}
    out['tick'] = rng.integers(0, 20000, n).astype(np.int32)
    out.update(random_vision(rng, n, prm))
    return out


def mirror(state):
    """the mirrored state (agent_obs.mirror); necks are relative to the body: each player's neck mirrors as itself"""
    perm = np.r_[11:22, 0:11, 22, 23]
    full = A.blank_state(state['x'].shape[0])
    full.update({k: state[k] for k in ENGINE_KEYS if k in full})
    m = A.mirror(full)
    out = {k: m[k] for k in ENGINE_KEYS if k != 'tick'}
    out['tick'] = np.asarray(state['tick']).copy()
    for k in VISION_PLANES:
        out[k] = np.asarray(state[k])[:, perm].copy()
    return out
