"""ctypes binding of tests/agent_obs_ref.c, the host restatement of the per-agent observations (include/s2d_match.h).
TEST INFRASTRUCTURE: compiled on demand with -ffp-contract=off (the fp32 contract)."""
import ctypes as C
import os
import subprocess

import numpy as np

import scripted_policy as SP

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'agent_obs_ref.c')
# what the observation reads (S2DMatchBuffers names); [N][24] planes first, then [N] words
OBJ_PLANES = ('x', 'y', 'vx', 'vy', 'body', 'stamina', 'effort', 'recovery', 'stamina_capacity', 'tackle_cycles', 'catch_ban', 'card')
ENV_WORDS = ('cycle', 'mode', 'mode_side', 'score_left', 'score_right', 'last_touch_side', 'ball_holder', 'stopped_cycle')
FLOAT_PLANES = OBJ_PLANES[:9]
DIM = 224


class AgentParams(C.Structure):
    _fields_ = [(n, C.c_float * 22) for n in ('ka', 'ka2', 'speed_max', 'kick_rate', 'inv_margin', 'size', 'type_id')] + [
        ('ball_size', C.c_float), ('ball_decay', C.c_float)] + [
        (n, C.c_int32) for n in ('half_time_cycles', 'nr_extra_halfs', 'extra_half_cycles', 'total_cycles')]


class AgentState(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in OBJ_PLANES + ENV_WORDS]


def build(outdir):
    so = os.path.join(str(outdir), 'libagent_obs_ref.so')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(so)
    L.s2dao_agent_obs.restype = None
    L.s2dao_agent_obs.argtypes = [C.c_int64, C.POINTER(AgentState), C.POINTER(AgentParams), C.c_uint32, C.c_void_p]
    return L


def params(cfg):
    """AgentParams as the engine derives them from an S2DMatchConfig (fp32, rounded as the engine rounds them)"""
    P = AgentParams()
    f = np.float32
    bs = f(cfg.sp.ball_size)
    for i in range(22):
        t = cfg.player_types[cfg.player_type_id[i]]
        P.ka[i] = f(f(f(t.player_size) + bs) + f(t.kickable_margin))
        P.ka2[i] = SP.kickable_area2(cfg, i)
        P.speed_max[i] = f(t.player_speed_max)
        P.kick_rate[i] = f(t.kick_power_rate)
        P.inv_margin[i] = f(1.0 / t.kickable_margin)
        P.size[i] = f(t.player_size)
        P.type_id[i] = f(cfg.player_type_id[i])
    P.ball_size, P.ball_decay = bs, f(cfg.sp.ball_decay)
    mp = cfg.mp
    P.half_time_cycles, P.nr_extra_halfs, P.extra_half_cycles = mp.half_time_cycles, mp.nr_extra_halfs, mp.extra_half_cycles
    P.total_cycles = mp.half_time_cycles * mp.nr_normal_halfs
    return P


def observations(L, state, prm, mask=0x3FFFFF):
    """state: dict of numpy arrays named as in OBJ_PLANES ([N][24]) and ENV_WORDS ([N]) -> float32 [N, popcount(mask), 224]"""
    planes = [np.ascontiguousarray(state[k], dtype=np.float32 if k in FLOAT_PLANES else np.int32) for k in OBJ_PLANES]
    words = [np.ascontiguousarray(state[k], dtype=np.int32) for k in ENV_WORDS]
    n = planes[0].shape[0]
    assert all(p.shape == (n, 24) for p in planes) and all(w.shape == (n,) for w in words)
    out = np.zeros((n, bin(mask).count('1'), DIM), dtype=np.float32)
    st = AgentState(*[a.ctypes.data for a in planes + words])
    L.s2dao_agent_obs(n, C.byref(st), C.byref(prm), mask, out.ctypes.data)
    return out


def blank_state(n=1):
    """zeroed state dict (all planes and words) for hand-built scenes"""
    s = {k: np.zeros((n, 24), dtype=np.float32 if k in FLOAT_PLANES else np.int32) for k in OBJ_PLANES}
    s.update({k: np.zeros((n,), dtype=np.int32) for k in ENV_WORDS})
    return s


def mirror_body(b):
    b = np.asarray(b, dtype=np.float32)
    return np.where(b > 0, b - np.float32(180.0), b + np.float32(180.0)).astype(np.float32)


def mirror(state):
    """the mirrored state: teams swapped (slot i <-> i + 11), positions and velocities negated, bodies turned by 180 degrees,
    scores / mode side / last touch / holder swapped.  Exact for bodies on a coarse grid away from 0 and +-180."""
    perm = np.r_[11:22, 0:11, 22, 23]
    m = {}
    for k in OBJ_PLANES:
        v = np.asarray(state[k])[:, perm].copy()
        if k in ('x', 'y', 'vx', 'vy'):
            v = -v
        if k == 'body':
            v[:, :22] = mirror_body(v[:, :22])
        m[k] = v
    swap = {0: 0, 1: 2, 2: 1}
    for k in ENV_WORDS:
        m[k] = np.asarray(state[k]).copy()
    m['score_left'], m['score_right'] = np.asarray(state['score_right']).copy(), np.asarray(state['score_left']).copy()
    for k in ('mode_side', 'last_touch_side'):
        m[k] = np.vectorize(swap.get)(np.asarray(state[k])).astype(np.int32)
    h = np.asarray(state['ball_holder'])
    m['ball_holder'] = np.where(h > 0, (h - 1 + 11) % 22 + 1, 0).astype(np.int32)
    return m


def random_state(rng, n):
    """a random state with every word the observation reads; bodies on a 2^-16-degree grid in [-179, 179] without 0"""
    s = blank_state(n)
    s['x'][:, :23] = rng.uniform(-55, 55, (n, 23)).astype(np.float32)
    s['y'][:, :23] = rng.uniform(-36, 36, (n, 23)).astype(np.float32)
    s['vx'][:, :23] = rng.uniform(-1.5, 1.5, (n, 23)).astype(np.float32)
    s['vy'][:, :23] = rng.uniform(-1.5, 1.5, (n, 23)).astype(np.float32)
    near = rng.random(n) < 0.5                          # half the matches: the ball at someone's feet, slow
    who = rng.integers(0, 22, n)
    s['x'][near, 22] = s['x'][near, who[near]] + rng.uniform(-0.8, 0.8, near.sum()).astype(np.float32)
    s['y'][near, 22] = s['y'][near, who[near]] + rng.uniform(-0.8, 0.8, near.sum()).astype(np.float32)
    k = rng.integers(1, 179 * 65536, (n, 22)) * rng.choice([-1, 1], (n, 22))
    s['body'][:, :22] = (k / 65536.0).astype(np.float32)
    s['stamina'][:, :22] = rng.uniform(0, 8000, (n, 22)).astype(np.float32)
    s['effort'][:, :22] = rng.uniform(0.6, 1, (n, 22)).astype(np.float32)
    s['recovery'][:, :22] = rng.uniform(0.5, 1, (n, 22)).astype(np.float32)
    s['stamina_capacity'][:, :22] = rng.uniform(0, 130600, (n, 22)).astype(np.float32)
    s['tackle_cycles'][:, :22] = rng.integers(0, 3, (n, 22)) * (rng.random((n, 22)) < 0.1)
    s['catch_ban'][:, [0, 11]] = rng.integers(0, 6, (n, 2))
    s['card'][:, :22] = rng.choice([0, 1, 2], (n, 22), p=[0.85, 0.1, 0.05])
    s['cycle'][:] = rng.integers(0, 8000, n)
    s['mode'][:] = rng.integers(0, 32, n)
    s['mode_side'][:] = rng.integers(0, 3, n)
    s['score_left'][:] = rng.integers(0, 9, n)
    s['score_right'][:] = rng.integers(0, 9, n)
    s['last_touch_side'][:] = rng.integers(0, 3, n)
    s['ball_holder'][:] = rng.choice([0, 1, 12], n)
    s['stopped_cycle'][:] = rng.integers(0, 500, n)
    return s
