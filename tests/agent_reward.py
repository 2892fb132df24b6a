"""ctypes binding of tests/agent_reward_ref.c, the host restatement of the agent reward (include/s2d_match.h, "Agent reward").
TEST INFRASTRUCTURE: compiled on demand with -ffp-contract=off (the fp32 contract).  The row words come
from the agent-observation restatement (tests/agent_obs.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

import agent_obs as A

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'agent_reward_ref.c')
TERMS = 6
PLAY_ON = 2
# weights that are not all powers of two, so that the fmaf chain rounds
WEIGHTS = (1.0, 0.03, 0.7, 0.3, 0.11, 0.05)


class RewardState(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('x', 'y', 'card', 'mode')]


class Ref:
    def __init__(self, outdir):
        self.obs = A.build(outdir)
        so = os.path.join(str(outdir), 'libagent_reward_ref.so')
        subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-o', so, SRC], check=True,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        self.L = C.CDLL(so)
        self.L.s2dar_agent_reward.restype = None
        self.L.s2dar_agent_reward.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(RewardState), C.POINTER(RewardState),
                                              C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]

    def reward(self, prm, s0, s1, reward_left1, weights, chaser_only=False):
        """s0, s1: state dicts (agent_obs.OBJ_PLANES [N][24] and ENV_WORDS [N]) of S and S'; prm: agent_obs.params(cfg);
        reward_left1 float32 [N] of S' -> (reward float32 [N, 22], terms float32 [N, 22, 6])"""
        rows0, rows1 = A.observations(self.obs, s0, prm), A.observations(self.obs, s1, prm)
        n = rows0.shape[0]
        keep = []

        def st(s):
            a = [np.ascontiguousarray(s['x'], dtype=np.float32), np.ascontiguousarray(s['y'], dtype=np.float32),
                 np.ascontiguousarray(s['card'], dtype=np.int32), np.ascontiguousarray(s['mode'], dtype=np.int32)]
            keep.extend(a)
            return RewardState(*[v.ctypes.data for v in a])
        r0, r1 = st(s0), st(s1)
        rl = np.ascontiguousarray(reward_left1, dtype=np.float32)
        w = np.ascontiguousarray(weights, dtype=np.float32)
        assert rl.shape == (n,) and w.shape == (TERMS,)
        out = np.zeros((n, 22), dtype=np.float32)
        terms = np.zeros((n, 22, TERMS), dtype=np.float32)
        self.L.s2dar_agent_reward(n, rows0.ctypes.data, rows1.ctypes.data, C.byref(r0), C.byref(r1), rl.ctypes.data, w.ctypes.data,
                                  int(bool(chaser_only)), out.ctypes.data, terms.ctypes.data)
        return out, terms


SHORT = dict(half_time_cycles=8, nr_extra_halfs=0, penalty_shoot_outs=0)   # periods that end inside a 33-cycle run


def write_scene(s, seed=0):
    """Scenes written over a freshly reset state `s` (a dict with the agent_obs planes and words, [N][24] / [N]) so that every
    term of the reward contributes within a few cycles whatever the controllers do: every match in PlayOn with the players spread
    over the pitch; by match index, a ball about to cross a goal line (either one), a slow ball inside a player's kickable
    area with a last touch, red cards; and clocks at 0, 5 and 12 of the 16 cycles, so that a half-time, a TimeOver with its
    auto-reset and the kick-off after it fall inside the run."""
    rng = np.random.default_rng(seed)
    n = s['x'].shape[0]
    e = np.arange(n)
    s['x'][:, :22] = rng.uniform(-50, 50, (n, 22)).astype(np.float32)
    s['y'][:, :22] = rng.uniform(-32, 32, (n, 22)).astype(np.float32)
    s['body'][:, :22] = (rng.integers(-179 * 64, 179 * 64, (n, 22)) / 64.0).astype(np.float32)
    s['x'][:, 22] = rng.uniform(-40, 40, n).astype(np.float32)
    s['y'][:, 22] = rng.uniform(-25, 25, n).astype(np.float32)
    s['vx'][:, 22] = rng.uniform(-1, 1, n).astype(np.float32)
    s['vy'][:, 22] = rng.uniform(-1, 1, n).astype(np.float32)
    s['mode'][:] = PLAY_ON
    s['mode_side'][:] = 0
    s['last_touch_side'][:] = rng.integers(0, 3, n)
    s['cycle'][:] = np.array([0, 5, 12])[e % 3]
    goal = e % 4 == 0                                        # a goal in the first cycle: left scores, or right (every 8th match)
    sgn = np.where(e % 8 == 0, 1.0, -1.0).astype(np.float32)
    s['x'][goal, 22] = (sgn * 52.25)[goal]; s['y'][goal, 22] = 0.5
    s['vx'][goal, 22] = (sgn * 1.5)[goal]; s['vy'][goal, 22] = 0.0
    s['x'][goal, :22] = np.clip(s['x'][goal, :22], -30, 30)  # (nobody near enough to stop it)
    feet = e % 4 == 1                                        # the ball at the feet of a field player of either team
    who = np.where(e % 8 == 1, 3, 14)
    s['x'][feet, 22] = s['x'][e, who][feet] + 0.5; s['y'][feet, 22] = s['y'][e, who][feet]
    s['vx'][feet, 22] = 0.0; s['vy'][feet, 22] = 0.0
    s['last_touch_side'][feet] = np.where(e % 8 == 1, 1, 2)[feet]
    red = e % 4 == 2                                         # sent-off players, one of them the nearest to the ball
    s['card'][red, 5] = 2; s['card'][red, 16] = 2
    s['x'][red, 22] = s['x'][red, 5] + 2.0; s['y'][red, 22] = s['y'][red, 5]
    return s
