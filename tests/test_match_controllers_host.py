"""CPU checks of the 11v11 engine's per-slot controllers: the new C ABI is exported and declared, the Python layer rejects
bad controller specs and reports the right spaces, and the host restatement of the scripted team
(tests/scripted_policy_ref.c) chooses the commands that include/s2d_match.h's rule table describes in hand-built scenes."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import scripted_policy as SP
from soccer2d_amd import _capi_match as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEFT, RIGHT = 1, 2
FORM_X = [-50.0, -35.0, -35.0, -35.0, -35.0, -20.0, -20.0, -20.0, -20.0, -10.5, -10.5]
FORM_Y = [0.0, -20.0, -7.0, 7.0, 20.0, -22.0, -8.0, 8.0, 22.0, -6.0, 6.0]


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi
    return M.bind(_capi.load_library())


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return SP.build(tmp_path_factory.mktemp('scripted'))


@pytest.fixture(scope='module')
def prm():
    import match_oracle as MO
    return SP.params(MO.make_match_config())


def test_new_exports_in_library_and_header(lib):
    import test_capi_exports as T
    declared = T.declared_functions(os.path.join(ROOT, 'include', 's2d_match.h'))
    bound = {p[0] for p in M.MATCH_PROTOTYPES}
    for name in ('s2d_match_set_controllers', 's2d_match_rollout_ex'):
        assert name in declared and name in bound
        assert hasattr(lib, name)
    hdr = open(os.path.join(ROOT, 'include', 's2d_match.h')).read()
    for word in ('S2D_CTL_EXTERNAL = 0', 'S2D_CTL_RANDOM = 1', 'S2D_CTL_SCRIPTED = 2'):
        assert word in hdr
    # the C side rejects a NULL handle without touching a device
    assert lib.s2d_match_set_controllers(None, None) != 0
    assert lib.s2d_match_rollout_ex(None, 1, None, None, None, None) != 0


def test_controller_specs():
    assert M.controller_codes(None) is None
    assert M.controller_codes({'left': 'external', 'right': 'scripted'}) == bytes([0] * 11 + [2] * 11)
    assert M.controller_codes({'right': 'random'}) == bytes([0] * 11 + [1] * 11)
    assert M.controller_codes([2] * 22) == bytes([2] * 22)
    assert M.controller_codes(['random'] * 11 + [0] * 11) == bytes([1] * 11 + [0] * 11)
    for bad in ([0] * 21, [0] * 23, [3] + [0] * 21, [-1] + [0] * 21, [0.5] + [0] * 21, {'left': 'expert'},
                {'middle': 'random'}, ['scripted'] * 21 + ['nobody'], [True] + [0] * 21):
        with pytest.raises(ValueError):
            M.controller_codes(bad)


def test_vec_env_spaces():
    from soccer2d_amd.match import Soccer2DMatchVecEnv
    obs, act = Soccer2DMatchVecEnv.spaces(None)
    assert obs.shape == (23, 5) and act.shape == (22, 3)
    for opp in ('random', 'scripted'):
        obs, act = Soccer2DMatchVecEnv.spaces(opp)
        assert obs.shape == (23, 5) and act.shape == (11, 3)
    with pytest.raises(ValueError):
        Soccer2DMatchVecEnv.spaces('helios')


# ---------------------------------------------------------------------------------------------- scenes
def scene(mode=M.GM_PLAY_ON, side=LEFT, ball=(0.0, 0.0), last_touch=0, holder=0, taker=0):
    """one match: every player on his kick-off formation place facing the other goal, the ball at `ball`"""
    s = {k: np.zeros((1, 24), dtype=np.float32 if k in ('x', 'y', 'body') else np.int32) for k in SP.OBJ_PLANES}
    for i in range(22):
        k = i % 11
        s['x'][0, i] = FORM_X[k] if i < 11 else -FORM_X[k]
        s['y'][0, i] = FORM_Y[k]
        s['body'][0, i] = 0.0 if i < 11 else 180.0
    s['x'][0, 22], s['y'][0, 22] = ball
    for k, v in (('mode', mode), ('mode_side', side), ('last_touch_side', last_touch), ('ball_holder', holder),
                 ('set_play_taker', taker)):
        s[k] = np.array([v], dtype=np.int32)
    return s


def act(ref, prm, s):
    return SP.actions(ref, s, prm)[0]


def bearing(s, i, tx, ty):
    d = math.degrees(math.atan2(ty - s['y'][0, i], tx - s['x'][0, i])) - s['body'][0, i]
    d = (d + 180.0) % 360.0 - 180.0
    return 180.0 if d == -180.0 else d                     # the engine's range: (-180, 180]


def test_goalie_catch_and_back_pass(ref, prm):
    s = scene(ball=(-49.5, 0.2), last_touch=RIGHT)
    a = act(ref, prm, s)
    assert a[0][0] == M.MCMD_CATCH and a[0][1] == pytest.approx(bearing(s, 0, -49.5, 0.2), abs=1e-3)
    s['catch_ban'][0, 0] = 2                               # banned: the ball is kickable, so he clears it instead
    a = act(ref, prm, s)
    assert a[0][0] == M.MCMD_KICK and a[0][1] == 100.0 and a[0][2] == pytest.approx(bearing(s, 0, 52.5, 0.0), abs=1e-3)
    s = scene(ball=(-49.5, 0.2), last_touch=LEFT)          # back pass: no catch
    assert act(ref, prm, s)[0][0] == M.MCMD_KICK
    s = scene(ball=(-30.0, 0.0), last_touch=RIGHT)          # outside the penalty area: no catch (and out of reach)
    s['x'][0, 0] = -30.6
    assert act(ref, prm, s)[0][0] != M.MCMD_CATCH
    s = scene(ball=(49.5, 0.0), last_touch=LEFT)            # the right goalie catches a ball the left team played
    a = act(ref, prm, s)
    assert a[11][0] == M.MCMD_CATCH and a[11][1] == pytest.approx(bearing(s, 11, 49.5, 0.0), abs=1e-3)


def test_goalie_holding_clears(ref, prm):
    s = scene(mode=M.GM_FREE_KICK, side=LEFT, ball=(-49.5, 0.0), holder=1)
    a = act(ref, prm, s)
    assert a[0][0] == M.MCMD_KICK and a[0][1] == 100.0 and a[0][2] == pytest.approx(bearing(s, 0, 52.5, 0.0), abs=1e-3)


def test_kickable_player_shoots(ref, prm):
    s = scene(ball=(-19.5, -8.3))                          # within player 6's kickable area (-20, -8)
    a = act(ref, prm, s)
    assert a[6][0] == M.MCMD_KICK and a[6][1] == 100.0 and a[6][2] == pytest.approx(bearing(s, 6, 52.5, 0.0), abs=1e-3)


def test_chaser_tie_goes_to_lower_index(ref, prm):
    s = scene(ball=(-20.0, 0.0))                           # players 6 (-20, -8) and 7 (-20, 8): the same distance
    s['body'][0, 6] = 90.0                                 # 6 faces the ball: dashes
    a = act(ref, prm, s)
    assert a[6][0] == M.MCMD_DASH and a[6][1] == 100.0 and a[6][2] == 0.0
    assert a[7][0] != M.MCMD_DASH or a[7][2] == 0.0
    # 7 is not the chaser: he heads for his home place (formation + gains * ball), 10 m behind and 0 to the side
    hx, hy = -20.0 + 0.5 * -20.0, 8.0
    assert a[7][0] == M.MCMD_TURN and a[7][1] == pytest.approx(bearing(s, 7, hx, hy), abs=1e-3)
    s['body'][0, 6] = 0.0                                  # now facing away: turns
    a = act(ref, prm, s)
    assert a[6][0] == M.MCMD_TURN and a[6][1] == pytest.approx(90.0, abs=1e-3)


def test_opponent_restart_nobody_chases(ref, prm):
    s = scene(mode=M.GM_KICK_IN, side=RIGHT, ball=(-20.0, -34.0))
    a = act(ref, prm, s)
    # the left team's nearest (5 at (-20, -22)) does not chase: he goes toward his home place
    hx, hy = -20.0 + 0.5 * -20.0, -22.0 + 0.25 * -34.0
    assert a[5][0] == M.MCMD_TURN and a[5][1] == pytest.approx(bearing(s, 5, hx, hy), abs=1e-3)
    # the right team's nearest non-goalie takes it (16: (20, -22) -> the ball is behind him: he turns to it)
    d2 = [(s['x'][0, i] + 20.0) ** 2 + (s['y'][0, i] + 34.0) ** 2 for i in range(12, 22)]
    c = 12 + int(np.argmin(d2))
    assert a[c][0] == M.MCMD_TURN and a[c][1] == pytest.approx(bearing(s, c, -20.0, -34.0), abs=1e-3)
    s['mode_side'][0] = LEFT                               # the left team's own kick-in: 5 chases
    a = act(ref, prm, s)
    assert a[5][0] == M.MCMD_TURN and a[5][1] == pytest.approx(bearing(s, 5, -20.0, -34.0), abs=1e-3)


def test_dead_ball_halted_tackling_sent_off(ref, prm):
    for mode in (M.GM_AFTER_GOAL, M.GM_OFF_SIDE, M.GM_BEFORE_KICK_OFF, M.GM_TIME_OVER, M.GM_FIRST_HALF_OVER, M.GM_EXTEND_HALF,
                 M.GM_PAUSE, M.GM_HUMAN, M.GM_GOALIE_CATCH, M.GM_PENALTY_SETUP, M.GM_PENALTY_ONFIELD, M.GM_PENALTY_SCORE):
        assert (act(ref, prm, scene(mode=mode))[:, 0] == M.MCMD_NONE).all(), mode
    s = scene(ball=(-19.5, -8.3))
    s['tackle_cycles'][0, 6] = 3
    s['card'][0, 7] = M.CARD_RED
    a = act(ref, prm, s)
    assert a[6][0] == M.MCMD_NONE and a[7][0] == M.MCMD_NONE


def test_shoot_out(ref, prm):
    # PenaltyReady_: the right team's taker 21 stands behind the spot; he plays on the right goal, everybody else waits
    s = scene(mode=M.GM_PENALTY_READY, side=RIGHT, ball=(10.0, 0.0), taker=22)
    s['x'][0, 21], s['y'][0, 21], s['body'][0, 21] = 9.3, 0.0, 0.0
    a = act(ref, prm, s)
    assert a[21][0] == M.MCMD_KICK and a[21][2] == pytest.approx(bearing(s, 21, 52.5, 0.0), abs=1e-3)
    assert (a[np.arange(22) != 21, 0] == M.MCMD_NONE).all()
    s['x'][0, 21] = 7.0                                    # out of reach: he goes to the ball
    assert act(ref, prm, s)[21][0] == M.MCMD_DASH
    # PenaltyTaken_: the defending (left) goalie guards the right goal; he catches a ball in that penalty area
    s = scene(mode=M.GM_PENALTY_TAKEN, side=RIGHT, ball=(30.0, 0.0), taker=22, last_touch=RIGHT)
    s['x'][0, 0], s['y'][0, 0], s['body'][0, 0] = 51.5, 0.0, 180.0
    a = act(ref, prm, s)
    assert a[0][0] == M.MCMD_DASH                          # his guard point (50, 0) lies straight ahead
    s['x'][0, 22] = 50.8
    a = act(ref, prm, s)
    assert a[0][0] == M.MCMD_CATCH
    assert a[11][0] == M.MCMD_NONE                         # the kicking team's goalie does nothing
