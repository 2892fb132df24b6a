"""CPU checks of the agent reward (include/s2d_match.h, "Agent reward"): the host restatement (tests/agent_reward_ref.c) gives the
header's answers in hand-built scenes with exactly representable numbers, one term at a time; mirrored (S, S') pairs give bitwise
equal rewards to mirrored agents; the ctypes struct and the term names equal the header's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import agent_obs as A
import agent_reward as R
import match_oracle as MO
from soccer2d_amd import _capi_match as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NONE, LEFT, RIGHT = 0, 1, 2
PLAY_ON, KICK_IN = M.GM_PLAY_ON, M.GM_KICK_IN
SIGN = np.array([1.0] * 11 + [-1.0] * 11, dtype=f32)


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return R.Ref(tmp_path_factory.mktemp('agent_reward'))


@pytest.fixture(scope='module')
def prm():
    return A.params(MO.make_match_config())


def scene():
    """one PlayOn match: the players far apart on a coarse grid, far from the ball at the centre, bodies at 0 (own frame: the
    right team's field bodies are 180)"""
    s = A.blank_state(1)
    for i in range(11):
        s['x'][0, i], s['y'][0, i] = -40.0 + 2.0 * i, -20.0 + 4.0 * i
        s['x'][0, 11 + i], s['y'][0, 11 + i] = 40.0 - 2.0 * i, 20.0 - 4.0 * i
        s['body'][0, 11 + i] = 180.0
    s['mode'][:] = PLAY_ON
    return s


def copy(s, **ball):
    t = {k: v.copy() for k, v in s.items()}
    for k, v in ball.items():
        t[k][0, 22] = v
    return t


def one(k, w):
    v = [0.0] * 6
    v[M.REWARD_TERMS.index(k)] = w
    return v


def run(ref, prm, s0, s1, weights, reward_left=0.0, chaser_only=False):
    out, terms = ref.reward(prm, s0, s1, np.array([reward_left], dtype=f32), weights, chaser_only)
    return out[0], terms[0]


def test_ball_advance_is_signed_by_side_and_needs_live_play(ref, prm):
    s0 = scene()
    s1 = copy(s0, x=1.0)
    out, _ = run(ref, prm, s0, s1, one('ball_advance', 0.03))
    assert np.array_equal(out, f32(0.03) * SIGN)
    s1['mode'][:] = KICK_IN                                  # the cycle ends in a restart: not live
    out, _ = run(ref, prm, s0, s1, one('ball_advance', 0.03))
    assert np.array_equal(out, np.zeros(22, dtype=f32))
    s0['mode'][:] = KICK_IN; s1['mode'][:] = PLAY_ON         # ... or starts in one
    out, _ = run(ref, prm, s0, s1, one('ball_advance', 0.03))
    assert np.array_equal(out, np.zeros(22, dtype=f32))


def test_approach_3_4_5(ref, prm):
    s0 = scene()
    for a, sg in ((1, 1.0), (12, -1.0)):                     # agent 1 at (-38, -16), agent 12 its mirror image
        ax, ay = s0['x'][0, a], s0['y'][0, a]
        b0 = copy(s0, x=ax + sg * 3.0, y=ay + sg * 4.0)      # 5 m away
        b1 = copy(s0, x=ax, y=ay + sg * 3.0)                 # 3 m away
        out, terms = run(ref, prm, b0, b1, one('approach', 1.0))
        assert out[a] == f32(2.0) and terms[a, 2] == f32(2.0)
        out, _ = run(ref, prm, b1, b0, one('approach', 0.5))
        assert out[a] == f32(-1.0)


def test_facing_90_to_45(ref, prm):
    s0 = scene()
    for a, sg in ((1, 1.0), (12, -1.0)):
        ax, ay = s0['x'][0, a], s0['y'][0, a]
        b0 = copy(s0, x=ax, y=ay + sg * 5.0)                 # bearing 90 (own frame, body 0)
        b1 = copy(s0, x=ax + sg * 5.0, y=ay + sg * 5.0)      # bearing 45
        out, terms = run(ref, prm, b0, b1, one('facing', 1.0))
        assert terms[a, 3] == f32(45.0) * f32(1.0 / 180.0) == f32(0.25)
        assert out[a] == f32(0.25)
        b2 = copy(s0, x=ax, y=ay - sg * 5.0)                 # bearing -90: the absolute value is what counts
        out, terms = run(ref, prm, b2, b1, one('facing', 1.0))
        assert out[a] == f32(0.25)


def test_kickable_inside_and_outside_the_bound(ref, prm):
    s0 = scene()
    ax, ay = s0['x'][0, 4], s0['y'][0, 4]
    inside, outside = copy(s0, x=ax + 1.0, y=ay), copy(s0, x=ax + 2.0, y=ay)
    out, _ = run(ref, prm, s0, inside, one('kickable', 0.11))
    want = np.zeros(22, dtype=f32); want[4] = f32(0.11)
    assert np.array_equal(out, want)
    out, _ = run(ref, prm, s0, outside, one('kickable', 0.11))
    assert np.array_equal(out, np.zeros(22, dtype=f32))
    inside['mode'][:] = KICK_IN                              # mode(S') is what counts, not mode(S)
    out, _ = run(ref, prm, s0, inside, one('kickable', 0.11))
    assert np.array_equal(out, np.zeros(22, dtype=f32))
    s0k = copy(s0); s0k['mode'][:] = KICK_IN; inside['mode'][:] = PLAY_ON
    out, _ = run(ref, prm, s0k, inside, one('kickable', 0.11))
    assert np.array_equal(out, want)


def test_possession_signs(ref, prm):
    s0 = scene()
    for side, sg in ((LEFT, 1.0), (RIGHT, -1.0), (NONE, 0.0)):
        s1 = copy(s0)
        s1['last_touch_side'][:] = side
        out, _ = run(ref, prm, s0, s1, one('possession', 0.05))
        assert np.array_equal(out, f32(0.05) * f32(sg) * SIGN)
    s1['last_touch_side'][:] = LEFT; s1['mode'][:] = KICK_IN
    out, _ = run(ref, prm, s0, s1, one('possession', 0.05))
    assert np.array_equal(out, np.zeros(22, dtype=f32))


@pytest.mark.parametrize('when', ['before', 'after', 'both'])
def test_a_sent_off_agent_keeps_team_terms_and_loses_individual_ones(ref, prm, when):
    s0 = scene()
    ax, ay = s0['x'][0, 4], s0['y'][0, 4]
    b0, b1 = copy(s0, x=ax + 5.0, y=ay), copy(s0, x=ax + 1.0, y=ay)
    if when in ('before', 'both'):
        b0['card'][0, 4] = M.CARD_RED
    if when in ('after', 'both'):
        b1['card'][0, 4] = M.CARD_RED
    b1['last_touch_side'][:] = LEFT
    _, terms = run(ref, prm, b0, b1, [1.0] * 6)
    assert terms[4, 1] == f32(-4.0) and terms[4, 5] == f32(1.0)          # team terms: as his team-mates'
    assert np.array_equal(terms[4, [1, 5]], terms[5, [1, 5]])
    assert np.array_equal(terms[4, [2, 3, 4]], np.zeros(3, dtype=f32))   # individual terms: none
    assert terms[5, 2] != 0.0


def test_chaser_only_tie_goes_to_the_lower_index_and_never_to_the_goalie(ref, prm):
    s0 = scene()
    b0 = copy(s0, x=0.0, y=0.0)
    for t0, sg in ((0, 1.0), (11, -1.0)):
        b0['x'][0, t0], b0['y'][0, t0] = sg * 1.0, 0.0                   # the goalie: nearest of all
        b0['x'][0, t0 + 3], b0['y'][0, t0 + 3] = sg * 3.0, sg * 4.0      # two field players exactly 5 m away
        b0['x'][0, t0 + 7], b0['y'][0, t0 + 7] = -sg * 4.0, sg * 3.0
    b1 = copy(b0, x=0.0, y=1.0)
    _, every = run(ref, prm, b0, b1, one('approach', 1.0))
    _, only = run(ref, prm, b0, b1, one('approach', 1.0), chaser_only=True)
    assert (every[:, 2] != 0).all()
    for t0 in (0, 11):
        want = np.zeros(11, dtype=f32); want[3] = every[t0 + 3, 2]
        assert np.array_equal(only[t0:t0 + 11, 2], want)
    b0['card'][0, 3] = M.CARD_RED                                        # the chaser sent off: the other one of the tie
    _, only = run(ref, prm, b0, b1, one('approach', 1.0), chaser_only=True)
    assert only[3, 2] == 0.0 and only[7, 2] == every[7, 2] and np.count_nonzero(only[:11, 2]) == 1
    # chaser_only gates approach and facing only
    b1['last_touch_side'][:] = LEFT
    _, t_all = run(ref, prm, b0, b1, [1.0] * 6, chaser_only=True)
    _, t_any = run(ref, prm, b0, b1, [1.0] * 6)
    assert np.array_equal(t_all[:, [0, 1, 4, 5]], t_any[:, [0, 1, 4, 5]])


def test_goal_cycle(ref, prm):
    s0 = scene()
    s0['x'][0, 22] = 52.0
    s1 = copy(s0, x=0.0)                                                 # a goal: the ball back on the centre spot, play stopped
    s1['mode'][:] = M.GM_AFTER_GOAL
    s1['mode_side'][:] = LEFT
    s1['score_left'][:] = 1
    s1['last_touch_side'][:] = LEFT
    out, terms = run(ref, prm, s0, s1, R.WEIGHTS, reward_left=1.0)
    assert np.array_equal(out, SIGN)                                     # the goal term alone: nothing else is live
    assert np.array_equal(terms[:, 1:], np.zeros((22, 5), dtype=f32))
    out, _ = run(ref, prm, s0, s1, R.WEIGHTS, reward_left=-1.0)
    assert np.array_equal(out, -SIGN)


def test_the_weighted_sum_is_the_fmaf_chain(ref, prm):
    rng = np.random.default_rng(3)
    s0, s1 = A.random_state(rng, 64), A.random_state(rng, 64)
    s0['mode'][:] = PLAY_ON; s1['mode'][:] = PLAY_ON
    w = np.array(R.WEIGHTS, dtype=f32)
    out, terms = ref.reward(prm, s0, s1, np.zeros(64, dtype=f32), w)
    acc = np.zeros((64, 22), dtype=np.float64)
    for k in range(6):                                                   # fmaf in float64: exact product, one rounding to fp32
        acc = (w[k].astype(np.float64) * terms[..., k].astype(np.float64) + acc).astype(f32).astype(np.float64)
    assert np.array_equal(out, acc.astype(f32))
    assert all(np.count_nonzero(terms[..., k]) for k in (1, 2, 3, 4, 5))


@pytest.mark.parametrize('chaser_only', [False, True])
def test_mirrored_pairs_give_bitwise_equal_rewards(ref, prm, chaser_only):
    rng = np.random.default_rng(11)
    n = 256
    s0, s1 = A.random_state(rng, n), A.random_state(rng, n)
    s0['mode'][:] = np.where(rng.random(n) < 0.8, PLAY_ON, s0['mode'])
    s1['mode'][:] = np.where(rng.random(n) < 0.8, PLAY_ON, s1['mode'])
    rl = rng.choice([-1.0, 0.0, 1.0], n).astype(f32)
    out, terms = ref.reward(prm, s0, s1, rl, R.WEIGHTS, chaser_only)
    mout, mterms = ref.reward(prm, A.mirror(s0), A.mirror(s1), -rl, R.WEIGHTS, chaser_only)
    perm = np.r_[11:22, 0:11]
    assert np.array_equal(out.view(np.int32), mout[:, perm].view(np.int32))
    assert np.array_equal(terms.view(np.int32), mterms[:, perm].view(np.int32))
    # team terms are exact negations between the sides of one match
    for k in (0, 1, 5):
        assert np.array_equal(terms[:, :11, k], -terms[:, 11:, k])
        assert (terms[:, :11, k] == terms[:, :1, k]).all()
    assert np.count_nonzero(out) > n


def test_struct_size_and_term_names_against_the_header(tmp_path):
    hdr = open(os.path.join(ROOT, 'include', 's2d_match.h')).read()
    names = re.findall(r'^ \*   (\d) (\w+)\s+(?:team|individual)\s', hdr, flags=re.M)
    assert tuple(n for _i, n in names) == M.REWARD_TERMS and [int(i) for i, _n in names] == list(range(6))
    prog = tmp_path / 'sz.c'
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s2d_match.h"\nint main(){printf("%zu %zu %d\\n",'
                    'sizeof(S2DMatchAgentReward),offsetof(S2DMatchAgentReward,chaser_only),S2D_MATCH_REWARD_TERMS);return 0;}\n')
    exe = tmp_path / 'sz'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(prog), '-o', str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [C.sizeof(M.S2DMatchAgentReward), M.S2DMatchAgentReward.chaser_only.offset, len(M.REWARD_TERMS)]
    assert R.TERMS == len(M.REWARD_TERMS)
    for name in ('s2d_match_set_agent_reward', 's2d_match_rollout_reward'):
        assert name in {p[0] for p in M.MATCH_PROTOTYPES}
    assert M.reward_weights({'goal': 1, 'facing': 0.5}) == [1.0, 0.0, 0.0, 0.5, 0.0, 0.0]
    assert M.reward_weights(R.WEIGHTS) == list(R.WEIGHTS)
    for bad in ({'goals': 1}, [1, 2, 3]):
        with pytest.raises(ValueError):
            M.reward_weights(bad)
