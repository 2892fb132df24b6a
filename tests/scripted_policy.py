"""ctypes binding of tests/scripted_policy_ref.c, the host restatement of the scripted team (include/s2d_match.h).
TEST INFRASTRUCTURE: compiled on demand with -ffp-contract=off (the fp32 contract)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'scripted_policy_ref.c')
# what the engine reads for the policy (S2DMatchBuffers names); [N][24] planes first, then [N] words
OBJ_PLANES = ('x', 'y', 'body', 'tackle_cycles', 'catch_ban', 'card')
ENV_WORDS = ('mode', 'mode_side', 'last_touch_side', 'ball_holder', 'set_play_taker')


def build(outdir):
    so = os.path.join(str(outdir), 'libscripted_policy_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    L.s2dsp_actions.restype = None
    L.s2dsp_actions.argtypes = [C.c_int64] + [C.c_void_p] * 15
    return L


def kickable_area2(cfg, slot):
    """the engine's per-slot kickable bound: the largest float T with sqrtf(T) <= kickable area (fp32)"""
    t = cfg.player_types[cfg.player_type_id[slot]]
    ka = np.float32(np.float32(t.player_size) + np.float32(cfg.sp.ball_size)) + np.float32(t.kickable_margin)
    T = np.float32(ka * ka)
    while np.sqrt(T) > ka:
        T = np.nextafter(T, np.float32(0))
    while np.sqrt(np.nextafter(T, np.float32(np.inf))) <= ka:
        T = np.nextafter(T, np.float32(np.inf))
    return T


def params(cfg):
    """(ka2[22], catch_len[22], fp[7]) float32 as the engine derives them from an S2DMatchConfig"""
    ka2 = np.array([kickable_area2(cfg, i) for i in range(22)], dtype=np.float32)
    cl = np.array([np.float32(cfg.mp.catchable_area_l * cfg.player_types[cfg.player_type_id[i]].catchable_area_l_stretch)
                   for i in range(22)], dtype=np.float32)
    mp, sp = cfg.mp, cfg.sp
    fp = np.array([sp.pitch_half_length, sp.pitch_half_width, mp.max_power, sp.pitch_half_length - mp.penalty_area_length,
                   mp.penalty_area_half_width, mp.max_catch_angle, mp.min_catch_angle], dtype=np.float32)
    return ka2, cl, fp


def actions(L, state, prm):
    """state: dict of numpy arrays named as in OBJ_PLANES ([N][24]) and ENV_WORDS ([N]) -> float32 [N, 22, 3]"""
    ka2, cl, fp = prm
    planes = [np.ascontiguousarray(state[k], dtype=np.float32 if k in ('x', 'y', 'body') else np.int32) for k in OBJ_PLANES]
    words = [np.ascontiguousarray(state[k], dtype=np.int32) for k in ENV_WORDS]
    n = planes[0].shape[0]
    assert all(p.shape == (n, 24) for p in planes) and all(w.shape == (n,) for w in words)
    out = np.zeros((n, 22, 3), dtype=np.float32)
    keep = planes + words + [ka2, cl, fp]
    L.s2dsp_actions(n, *[a.ctypes.data for a in keep], out.ctypes.data)
    return out
