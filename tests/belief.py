"""ctypes binding of tests/belief_ref.c, the host restatement of the belief layer (include/s2d_match.h, "Belief").
TEST INFRASTRUCTURE: compiled on demand with -ffp-contract=off (the fp32 contract)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'belief_ref.c')
DIM = 192
COUNT_LIMIT = np.float32(16777216.0)
# defaults of s2d_match_belief_default_params, restated (the host tests compare the library's with these)
DEFAULTS = dict(ball_decay=0.94, player_decay=0.4, view_angle=(60.0, 120.0, 180.0), match_dist=3.0, match_rate=0.1,
                ghost_margin=5.0, count_max=1000.0)
BALL = 16                                                 # x, y, vx, vy, pos_count | game_mode_type, mode side, cycle
PLAYERS = 24                                              # 21 rows of x, y, vx, vy, body, pos_count, vel_count, body_count


class BeliefParams(C.Structure):
    _fields_ = [('ball_decay', C.c_float), ('player_decay', C.c_float), ('view_angle', C.c_float * 3), ('match_dist', C.c_float),
                ('match_rate', C.c_float), ('ghost_margin', C.c_float), ('count_max', C.c_float)]


def build(outdir):
    so = os.path.join(str(outdir), 'libbelief_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC, '-lm'], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    L.s2dbel_scan.restype = None
    L.s2dbel_scan.argtypes = [C.POINTER(BeliefParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_uint32]
    L.s2dbel_reset.restype = None
    L.s2dbel_reset.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    return L


def params(**over):
    """BeliefParams as the layer derives them from an S2DBeliefParams with `over` written over the defaults: every word rounded
    to fp32 once"""
    v = dict(DEFAULTS)
    for k, x in over.items():
        assert k in v, k
        v[k] = x
    P = BeliefParams()
    for k in ('ball_decay', 'player_decay', 'match_dist', 'match_rate', 'ghost_margin', 'count_max'):
        setattr(P, k, np.float32(v[k]))
    for i in range(3):
        P.view_angle[i] = np.float32(v['view_angle'][i])
    return P


def popcount(mask):
    return bin(mask).count('1')


def unknown(n, k, count=COUNT_LIMIT):
    """[n, k, 192] rows as s2d_match_belief_reset leaves them (count = the limit) or as an update keeps unknown entries under
    all-zero self and game words (count = count_max)"""
    b = np.zeros((n, k, DIM), dtype=np.float32)
    b[..., BALL + 4] = count
    for w in (5, 6, 7):
        b[..., PLAYERS + w::8] = count
    return b


def reset(L, belief, mask=None):
    """the rows of the masked matches as s2d_match_belief_reset leaves them; returns a new array"""
    b = np.ascontiguousarray(belief, dtype=np.float32).copy()
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    L.s2dbel_reset(b.ctypes.data, b.shape[0], b.shape[1], None if m is None else m.ctypes.data)
    return b


def scan(L, prm, see, belief, reset=None, mask=0x3FFFFF, record=True):
    """see [T, N, k, 192], belief [N, k, 192], reset [T, N] or None -> (the belief after row T - 1, the record [T, N, k, 192] or
    None); the inputs are not modified"""
    s = np.ascontiguousarray(see, dtype=np.float32)
    T, n, k, d = s.shape
    assert d == DIM and k == popcount(mask), s.shape
    b = np.ascontiguousarray(belief, dtype=np.float32).copy()
    assert b.shape == (n, k, DIM), b.shape
    r = None if reset is None else np.ascontiguousarray(reset, dtype=np.uint8)
    assert r is None or r.shape == (T, n)
    out = np.zeros_like(s) if record else None
    L.s2dbel_scan(C.byref(prm), s.ctypes.data, None if r is None else r.ctypes.data, b.ctypes.data,
                  None if out is None else out.ctypes.data, T, n, mask)
    return b, out


def step(L, prm, see, belief, reset=None, mask=0x3FFFFF):
    """one update: see [N, k, 192], reset [N] or None -> the new belief"""
    r = None if reset is None else np.asarray(reset, dtype=np.uint8)[None]
    return scan(L, prm, np.asarray(see, dtype=np.float32)[None], belief, r, mask, record=False)[0]


def row_of(slot, other):
    """the player row of raw slot `other` in the belief of the agent in raw slot `slot` (the header's identity order)"""
    assert slot != other
    u, i = slot % 11, other % 11
    if (slot < 11) == (other < 11):
        return i if i < u else i - 1
    return 10 + i
