"""CPU checks of the per-agent observations (include/s2d_match.h, s2d_match_agent_obs): the entry point is exported and declared,
the header's layout constants equal the Python layout, the VecEnv reports the right spaces for both observation kinds, and the
host restatement (tests/agent_obs_ref.c) gives the header's answers in hand-built scenes and is exactly symmetric between sides."""
import math
import os
import re

import numpy as np
import pytest

import agent_obs as A
import match_oracle as MO
from soccer2d_amd import _capi_match as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEFT, RIGHT = 1, 2
F = M.AGENT_OBS_FIELDS
NONE = M.REACH_NONE


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from soccer2d_amd import _capi
    return M.bind(_capi.load_library())


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return A.build(tmp_path_factory.mktemp('agent_obs'))


@pytest.fixture(scope='module')
def cfg():
    return MO.make_match_config()


@pytest.fixture(scope='module')
def prm(cfg):
    return A.params(cfg)


def test_export_in_library_and_header(lib):
    import test_capi_exports as T
    declared = T.declared_functions(os.path.join(ROOT, 'include', 's2d_match.h'))
    assert 's2d_match_agent_obs' in declared and 's2d_match_agent_obs' in {p[0] for p in M.MATCH_PROTOTYPES}
    assert hasattr(lib, 's2d_match_agent_obs')
    assert lib.s2d_match_agent_obs(None, 0x3FFFFF, None, None) != 0      # NULL handle: refused without touching a device


def test_header_layout_equals_python():
    hdr = open(os.path.join(ROOT, 'include', 's2d_match.h')).read()
    d = {k: int(v) for k, v in re.findall(r'#define S2D_AGENT_(\w+)\s+(\d+)', hdr)}
    assert d['OBS_DIM'] == M.AGENT_OBS_DIM == 224 and d['REACH_NONE'] == M.REACH_NONE and d['REACH_MAX'] == M.AGENT_REACH_MAX
    for name in ('self', 'ball', 'game', 'teammates', 'opponents'):
        assert d['OBS_' + name.upper()] == M.AGENT_OBS_BLOCKS[name].start
    starts = sorted(b.start for b in M.AGENT_OBS_BLOCKS.values())
    stops = sorted(b.stop for b in M.AGENT_OBS_BLOCKS.values())
    assert starts == [0] + stops[:-1] and stops[-1] == 224                  # the blocks tile the row
    assert (M.AGENT_OBS_BLOCKS['teammates'].stop - M.AGENT_OBS_BLOCKS['teammates'].start) == 11 * d['OBS_ROW_WORDS']
    scalars = sorted(v for v in F.values() if isinstance(v, int))
    assert scalars == list(range(48))                                        # every header word named once
    row = np.arange(224)
    assert list(row[F['opponents.reach_steps']]) == [136 + 8 * i + 7 for i in range(11)]
    assert M.agent_slot_mask('left') == 0x7FF and M.agent_slot_mask('right') == 0x3FF800 and M.agent_slot_mask(0x5) == 5
    for bad in (0, 1 << 22, -1, 'middle', 1.5, True):
        with pytest.raises(ValueError):
            M.agent_slot_mask(bad)


def test_vec_env_spaces():
    from soccer2d_amd.match import Soccer2DMatchVecEnv as V
    assert V.spaces(None)[0].shape == (23, 5) and V.spaces(None, 'state')[0].shape == (23, 5)
    o, a = V.spaces(None, 'agent')
    assert o.shape == (22, 224) and a.shape == (22, 3)
    for opp in ('random', 'scripted'):
        o, a = V.spaces(opp, 'agent')
        assert o.shape == (11, 224) and a.shape == (11, 3)
    with pytest.raises(ValueError):
        V.spaces(None, 'pixels')


# ---------------------------------------------------------------------------------------------- scenes
def scene():
    """everybody on a line, far from the ball at the centre, at rest, facing +x; PlayOn"""
    s = A.blank_state(1)
    for i in range(22):
        s['x'][0, i] = -30.0 if i < 11 else 30.0
        s['y'][0, i] = -30.0 + 3.0 * (i % 11)
        s['body'][0, i] = 0.0 if i < 11 else 180.0
    s['mode'][0] = M.GM_PLAY_ON
    return s


def obs(ref, prm, s, mask=0x3FFFFF):
    return A.observations(ref, s, prm, mask)[0]


def test_reach_of_a_ball_at_rest_and_of_one_rolling_away(ref, prm, cfg):
    s = scene()
    s['x'][0, 22], s['y'][0, 22] = 5.0, 0.0
    s['x'][0, 3], s['y'][0, 3] = 0.0, 0.0                # 5 m from the ball
    o = obs(ref, prm, s)
    ka = np.float32(np.float32(cfg.sp.player_size) + np.float32(cfg.sp.ball_size)) + np.float32(cfg.mp.kickable_margin)
    want = math.ceil((5.0 - ka) / cfg.sp.player_speed_max)
    assert o[3, F['game.self_reach_steps']] == want == 4
    assert o[0, F['teammates.reach_steps']][3] == want and o[11, F['opponents.reach_steps']][3] == want
    assert o[3, F['teammates.reach_steps']][3] == want and o[3, F['teammates.dist']][3] == 0 and o[3, F['teammates.bearing']][3] == 0
    assert o[3, F['ball.dist_from_self']] == 5.0 and o[3, F['ball.bearing']] == 0.0
    s['vx'][0, 22] = 3.0                                 # rolling away at full speed: nobody catches it within 50 cycles
    s['x'][0, :22] = -30.0                               # (at t = 50 the reach radius is 53.6 m; the ball is 83 m away)
    o = obs(ref, prm, s)
    assert (o[:, F['game.self_reach_steps']] == NONE).all()
    assert o[0, F['game.first_teammate_reach_steps']] == NONE and o[0, F['game.first_teammate_unum']] == 2   # slot order breaks ties


def test_offside_line(ref, prm):
    s = scene()
    s['x'][0, 11:22] = [52.0, 40.0, 30.0, 20.0, 10.0, 10.0, 5.0, 5.0, 5.0, 5.0, 5.0]   # right team's x (absolute)
    s['x'][0, 22] = 3.0
    o = obs(ref, prm, s)
    assert o[0, F['game.offside_line_x']] == 40.0        # the second-largest opponent x (left agent's frame)
    s['x'][0, 22] = 45.0                                  # ball behind the defenders
    assert obs(ref, prm, s)[0, F['game.offside_line_x']] == 45.0
    s['x'][0, 22] = -20.0
    s['x'][0, 11:22] = -np.abs(s['x'][0, 11:22])          # everybody in the left half: the line is the halfway line
    assert obs(ref, prm, s)[0, F['game.offside_line_x']] == 0.0
    # right agents: the left team's own-frame x = -x
    s = scene()
    s['x'][0, 0:11] = [-52.0, -45.0, -30.0, -20.0, -10.0, -10.0, -5.0, -5.0, -5.0, -5.0, -5.0]
    o = obs(ref, prm, s)
    assert o[11, F['game.offside_line_x']] == 45.0 and o[11, F['game.their_defense_line_x']] == 45.0
    assert o[11, F['game.our_defense_line_x']] == -30.0 and o[0, F['game.our_defense_line_x']] == -45.0


def test_kickable_opponent_and_teammate(ref, prm):
    s = scene()
    s['x'][0, 22], s['y'][0, 22] = 0.0, 0.0
    s['x'][0, 15], s['y'][0, 15] = 0.5, 0.0              # right slot 15 (unum 5) next to the ball
    s['x'][0, 13], s['y'][0, 13] = -0.4, 0.3             # right slot 13 (unum 3) too
    o = obs(ref, prm, s)
    assert o[0, F['game.kickable_opponent_unum']] == 3 and o[0, F['game.kickable_teammate_unum']] == 0
    assert o[15, F['game.kickable_teammate_unum']] == 3 and o[13, F['game.kickable_teammate_unum']] == 5
    assert o[15, F['self.is_kickable']] == 1 and o[0, F['self.is_kickable']] == 0
    assert 0 < o[15, F['self.kick_rate']] < 0.027 and o[0, F['self.kick_rate']] == 0
    assert o[15, F['game.self_reach_steps']] == 0
    assert o[15, F['game.first_teammate_reach_steps']] == 0 and o[15, F['game.first_teammate_unum']] == 3
    assert o[0, F['game.first_opponent_unum']] == 3 and o[0, F['game.second_opponent_unum']] == 5
    s['card'][0, 13] = M.CARD_RED                         # sent off: no longer kickable, not counted
    o = obs(ref, prm, s)
    assert o[15, F['game.kickable_teammate_unum']] == 0 and o[0, F['game.kickable_opponent_unum']] == 5


def test_red_carded_teammate_row(ref, prm):
    s = scene()
    s['card'][0, 4] = M.CARD_RED
    s['stamina'][0, 4] = 123.0
    o = obs(ref, prm, s)
    row = o[0, 48 + 8 * 4: 48 + 8 * 5]
    assert list(row[:7]) == [0.0] * 7 and row[7] == NONE
    row = o[11, 136 + 8 * 4: 136 + 8 * 5]
    assert list(row[:7]) == [0.0] * 7 and row[7] == NONE
    assert o[4, F['self.card']] == M.CARD_RED and o[4, F['self.stamina']] == 123.0 and o[4, F['game.self_reach_steps']] == NONE
    assert o[0, 48 + 8 * 5] == -30.0                      # the next row is a normal one


def test_penalty_modes_and_set_plays(ref, prm):
    s = scene()
    for mode in range(32):
        s['mode'][0] = mode
        assert obs(ref, prm, s)[0, F['game.is_penalty_kick_mode']] == (mode in (22, 23, 24, 25, 26, 28, 29)), mode
    s['mode'][0] = M.GM_ILLEGAL_DEFENSE
    assert obs(ref, prm, s)[0, F['game.is_penalty_kick_mode']] == 0
    s['mode'][0], s['mode_side'][0] = M.GM_CORNER_KICK, RIGHT
    o = obs(ref, prm, s)
    assert o[11, F['game.is_our_set_play']] == 1 and o[11, F['game.is_their_set_play']] == 0
    assert o[0, F['game.is_our_set_play']] == 0 and o[0, F['game.is_their_set_play']] == 1
    assert o[11, F['game.mode_side']] == 1 and o[0, F['game.mode_side']] == -1
    s['mode'][0] = M.GM_OFF_SIDE                           # an announcement is no set play
    o = obs(ref, prm, s)
    assert o[11, F['game.is_our_set_play']] == 0 and o[0, F['game.is_their_set_play']] == 0
    s['score_left'][0], s['score_right'][0], s['ball_holder'][0], s['last_touch_side'][0] = 2, 5, 12, LEFT
    o = obs(ref, prm, s)
    assert (o[11, F['game.our_score']], o[11, F['game.their_score']], o[0, F['game.our_score']]) == (5, 2, 2)
    assert o[11, F['ball.holder']] == 1 and o[0, F['ball.holder']] == -1
    assert o[11, F['ball.last_touch']] == -1 and o[0, F['ball.last_touch']] == 1


def test_own_frame_and_cycles_to_period_end(ref, prm, cfg):
    s = scene()
    s['x'][0, 14], s['y'][0, 14], s['vx'][0, 14], s['body'][0, 14] = 20.0, -3.0, -0.5, 170.0
    s['cycle'][0] = 2990
    o = obs(ref, prm, s)
    assert list(o[14, 0:5]) == [-20.0, 3.0, 0.5, -0.0, -10.0]
    assert o[14, F['self.is_goalie']] == 0 and o[11, F['self.is_goalie']] == 1 and o[0, F['self.is_goalie']] == 1
    assert o[0, F['game.cycles_to_period_end']] == 10 and o[0, F['game.cycle']] == 2990
    s['cycle'][0] = 6000 + 5                               # extra time
    assert obs(ref, prm, s)[0, F['game.cycles_to_period_end']] == cfg.mp.extra_half_cycles - 5


def test_mirror_is_exact_in_the_restatement(ref, cfg):
    rng = np.random.default_rng(3)
    s = A.random_state(rng, 512)
    types = {t: {'player_speed_max': 1.05 + 0.01 * t, 'kickable_margin': 0.7 + 0.01 * t, 'player_size': 0.3 + 0.005 * t,
                 'kick_power_rate': 0.027 + 0.0002 * t} for t in range(1, 17)}
    ids = [0] + list(range(1, 11)) + [0] + list(range(7, 17))
    cfg_h = MO.make_match_config(player_types=types, player_type_id=ids)
    cfg_m = MO.make_match_config(player_types=types, player_type_id=ids[11:] + ids[:11])
    a = A.observations(ref, s, A.params(cfg_h))
    b = A.observations(ref, A.mirror(s), A.params(cfg_m))
    assert np.array_equal(a[:, :11].view(np.int32), b[:, 11:].view(np.int32))
    assert np.array_equal(a[:, 11:].view(np.int32), b[:, :11].view(np.int32))
    assert not np.array_equal(a[:, :11], a[:, 11:])
