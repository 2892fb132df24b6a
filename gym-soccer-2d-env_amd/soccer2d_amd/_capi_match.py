"""ctypes mirror of include/s2d_match.h (11v11 match engine entry points of libs2d_hip.so)."""
import ctypes as C

from . import _capi

MATCH_PLAYERS, MATCH_SLOTS, MATCH_BALL, MATCH_OBJ_WORDS = 22, 24, 22, 5
MCMD_NONE, MCMD_DASH, MCMD_TURN, MCMD_KICK, MCMD_TACKLE, MCMD_CATCH, MCMD_MOVE = 0, 1, 2, 3, 4, 5, 6
MATCH_PLAYER_TYPES, GOALIE_LEFT, GOALIE_RIGHT = 18, 0, 11
GM_TIME_OVER, GM_PLAY_ON, GM_KICK_OFF, GM_KICK_IN, GM_FREE_KICK, GM_CORNER_KICK, GM_GOAL_KICK, GM_AFTER_GOAL, GM_OFF_SIDE = 1, 2, 3, 4, 5, 6, 7, 8, 9
GM_BEFORE_KICK_OFF, GM_BACK_PASS, GM_FREE_KICK_FAULT = 0, 18, 19          # idl/service.proto:268, 286-287
GM_FIRST_HALF_OVER, GM_FOUL_CHARGE, GM_CATCH_FAULT, GM_IND_FREE_KICK, GM_GOALIE_CATCH, GM_EXTEND_HALF = 11, 14, 20, 21, 30, 31   # :279, 282, 288-289, 298-299
GM_PENALTY_SETUP, GM_PENALTY_READY, GM_PENALTY_TAKEN, GM_PENALTY_MISS, GM_PENALTY_SCORE, GM_PENALTY_ONFIELD, GM_PENALTY_FOUL = 22, 23, 24, 25, 26, 28, 29   # :290-297
GM_FOUL_PUSH, GM_FOUL_MULTIPLE_ATTACKER, GM_FOUL_BALL_OUT = 15, 16, 17   # :283-285 (an operator's calls: played like FoulCharge_)
GM_PAUSE, GM_HUMAN = 12, 13                            # :280-281 (an operator's: written into eng.mode to hold a match)
PENALTY_MODES = (GM_PENALTY_SETUP, GM_PENALTY_READY, GM_PENALTY_TAKEN, GM_PENALTY_MISS, GM_PENALTY_SCORE, GM_PENALTY_ONFIELD,
                 GM_PENALTY_FOUL)                      # the shoot-out's modes (the kernel's set)
GM_ILLEGAL_DEFENSE = 27                                # :295 (off in the stock server)
GM_PENALTY_KICK = 10                                   # :278 (a foul inside the offender's own penalty area; the shoot-out modes are not built)
GM_NAMES = {0: 'BeforeKickOff', 1: 'TimeOver', 2: 'PlayOn', 3: 'KickOff_', 4: 'KickIn_', 5: 'FreeKick_', 6: 'CornerKick_', 7: 'GoalKick_',
            8: 'AfterGoal_', 9: 'OffSide_', 11: 'FirstHalfOver', 12: 'Pause', 13: 'Human', 14: 'FoulCharge_', 15: 'FoulPush_', 16: 'FoulMultipleAttacker_', 17: 'FoulBallOut_', 18: 'BackPass_', 19: 'FreeKickFault_',
            20: 'CatchFault_', 21: 'IndFreeKick_', 22: 'PenaltySetup_', 23: 'PenaltyReady_', 24: 'PenaltyTaken_',
            25: 'PenaltyMiss_', 26: 'PenaltyScore_', 27: 'IllegalDefense_', 28: 'PenaltyOnfield_', 29: 'PenaltyFoul_', 30: 'GoalieCatch_', 31: 'ExtendHalf'}
CARD_NONE, CARD_YELLOW, CARD_RED = 0, 1, 2
CTL_EXTERNAL, CTL_RANDOM, CTL_SCRIPTED = 0, 1, 2          # per-slot controllers (s2d_match_set_controllers)
CTL_CODES = {'external': CTL_EXTERNAL, 'random': CTL_RANDOM, 'scripted': CTL_SCRIPTED}
# per-agent observations in each team's own frame (s2d_match_agent_obs; the words are specified in include/s2d_match.h)
AGENT_OBS_DIM, AGENT_REACH_MAX, REACH_NONE = 224, 50, 51
AGENT_OBS_BLOCKS = {'self': slice(0, 16), 'ball': slice(16, 24), 'game': slice(24, 48), 'teammates': slice(48, 136),
                    'opponents': slice(136, 224)}
AGENT_ROW_FIELDS = ('x', 'y', 'vx', 'vy', 'body', 'dist', 'bearing', 'reach_steps')    # one teammate / opponent row
AGENT_OBS_FIELDS = dict(AGENT_OBS_BLOCKS)
for _i, _n in enumerate(('x', 'y', 'vx', 'vy', 'body', 'stamina', 'effort', 'recovery', 'stamina_capacity', 'is_goalie',
                         'tackle_cycles', 'card', 'is_kickable', 'kick_rate', 'catch_ban', 'type_id')):
    AGENT_OBS_FIELDS['self.' + _n] = 0 + _i
for _i, _n in enumerate(('x', 'y', 'vx', 'vy', 'dist_from_self', 'bearing', 'last_touch', 'holder')):
    AGENT_OBS_FIELDS['ball.' + _n] = 16 + _i
for _i, _n in enumerate(('game_mode_type', 'mode_side', 'our_score', 'their_score', 'cycle', 'stopped_cycle', 'cycles_to_period_end',
                         'is_penalty_kick_mode', 'offside_line_x', 'our_defense_line_x', 'their_defense_line_x',
                         'kickable_teammate_unum', 'kickable_opponent_unum', 'self_reach_steps',
                         'first_teammate_reach_steps', 'first_teammate_unum', 'second_teammate_reach_steps', 'second_teammate_unum',
                         'first_opponent_reach_steps', 'first_opponent_unum', 'second_opponent_reach_steps', 'second_opponent_unum',
                         'is_our_set_play', 'is_their_set_play')):
    AGENT_OBS_FIELDS['game.' + _n] = 24 + _i
for _t, _base in (('teammates', 48), ('opponents', 136)):       # [..., 11 rows] with a stride of 8 words
    for _i, _n in enumerate(AGENT_ROW_FIELDS):
        AGENT_OBS_FIELDS[f'{_t}.{_n}'] = slice(_base + _i, _base + 88, 8)
AGENT_SLOT_MASKS = {'all': 0x3FFFFF, 'left': 0x7FF, 'right': 0x3FF800}

# the vision layer (s2d_match_see; the words are specified in include/s2d_match.h, "Vision")
SEE_DIM, MATCH_ST_SEE = 192, 8
VIEW_KEEP, VIEW_NARROW, VIEW_NORMAL, VIEW_WIDE = 0, 1, 2, 3
VIEW_CODES = {'keep': VIEW_KEEP, 'narrow': VIEW_NARROW, 'normal': VIEW_NORMAL, 'wide': VIEW_WIDE}
SEE_LEVEL_UNSEEN, SEE_LEVEL_FELT, SEE_LEVEL_NO_TEAM, SEE_LEVEL_TEAM, SEE_LEVEL_FULL = 0, 1, 2, 3, 4
SEE_BLOCKS = {'self': slice(0, 16), 'ball': slice(16, 24), 'players': slice(24, 192)}
SEE_ROW_FIELDS = ('level', 'team', 'unum', 'dist', 'dir', 'dist_chg', 'dir_chg', 'body_rel')     # one player row
SEE_FIELDS = {}                                        # every word 0..191 exactly once: name -> index, or a slice over the 21 rows
for _i, _n in enumerate(('x', 'y', 'vx', 'vy', 'body', 'neck', 'face', 'view_width', 'fresh', 'see_wait', 'stamina', 'effort',
                         'recovery', 'stamina_capacity', 'is_goalie', 'card')):
    SEE_FIELDS['self.' + _n] = 0 + _i
for _i, _n in enumerate(('level', 'dist', 'dir', 'dist_chg', 'dir_chg', 'game_mode_type', 'mode_side', 'cycle')):
    SEE_FIELDS['ball.' + _n] = 16 + _i
for _i, _n in enumerate(SEE_ROW_FIELDS):
    SEE_FIELDS['players.' + _n] = slice(24 + _i, 192, 8)

# the belief layer (s2d_match_belief_scan; the words are specified in include/s2d_match.h, "Belief")
BELIEF_DIM, BELIEF_COUNT_LIMIT = 192, 16777216.0
BELIEF_BLOCKS = {'self': slice(0, 16), 'ball': slice(16, 24), 'players': slice(24, 192)}
BELIEF_ROW_FIELDS = ('x', 'y', 'vx', 'vy', 'body', 'pos_count', 'vel_count', 'body_count')     # one player row
BELIEF_FIELDS = {k: v for k, v in SEE_FIELDS.items() if k.startswith('self.')}   # every word 0..191 exactly once, as SEE_FIELDS
for _i, _n in enumerate(('x', 'y', 'vx', 'vy', 'pos_count', 'game_mode_type', 'mode_side', 'cycle')):
    BELIEF_FIELDS['ball.' + _n] = 16 + _i
for _i, _n in enumerate(BELIEF_ROW_FIELDS):
    BELIEF_FIELDS['players.' + _n] = slice(24 + _i, 192, 8)

# the audio layer (s2d_match_hear_step; the words are specified in include/s2d_match.h, "Hearing")
HEAR_DIM, HEAR_RECORD, SAY_WORDS, SAY_ROW, MATCH_ST_HEAR = 32, 16, 10, 12, 9
HEAR_BLOCKS = {'ours': slice(0, 16), 'theirs': slice(16, 32)}
HEAR_FIELDS = {}                                       # every word 0..31 exactly once: name -> index, or the payload's slice
for _r, _base in (('ours', 0), ('theirs', 16)):
    for _i, _n in enumerate(('heard', 'sender', 'dir', 'missed', 'capacity', 'attention')):
        HEAR_FIELDS[f'{_r}.{_n}'] = _base + _i
    HEAR_FIELDS[f'{_r}.payload'] = slice(_base + 6, _base + 16)
SAY_FIELDS = {'said': 0, 'attention': 1, 'payload': slice(2, 12)}   # one say row (MatchEngine.hear_step)


def belief_row_of(slot, other):
    """the player row (0..20) of raw slot `other` in the belief of the agent in raw slot `slot`: teammates first by own index
    with the agent itself left out, then the opponents by unum"""
    if slot == other or not (0 <= slot < MATCH_PLAYERS and 0 <= other < MATCH_PLAYERS):
        raise ValueError(f"no belief row of slot {other} for the agent in slot {slot}")
    u, i = slot % 11, other % 11
    if (slot < 11) == (other < 11):
        return i if i < u else i - 1
    return 10 + i


class S2DMatchParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        'kick_power_rate', 'kickable_margin', 'kick_rand', 'max_power', 'min_power',
        'tackle_dist', 'tackle_back_dist', 'tackle_width', 'tackle_power_rate',
        'max_tackle_power', 'max_back_tackle_power',
        'goal_width', 'offside_active_area_size', 'free_kick_distance')] + [(n, C.c_int32) for n in (
            'tackle_cycles', 'half_time_cycles', 'nr_normal_halfs', 'drop_ball_time', 'use_offside', 'catch_ban_cycle')] + [
                (n, C.c_double) for n in ('catchable_area_l', 'catch_area_w', 'catch_probability', 'max_catch_angle',
                                          'min_catch_angle', 'penalty_area_length', 'penalty_area_half_width')] + [
                    ('goalie_max_moves', C.c_int32), ('after_goal_wait', C.c_int32), ('kick_off_wait', C.c_int32),
                    ('back_passes', C.c_int32), ('free_kick_faults', C.c_int32), ('stopped_clock', C.c_int32),
                    ('announce_wait', C.c_int32), ('foul_cycles', C.c_int32), ('nr_extra_halfs', C.c_int32),
                    ('foul_detect_probability', C.c_double), ('extra_half_cycles', C.c_int32), ('golden_goal', C.c_int32),
                    ('penalty_shoot_outs', C.c_int32), ('pen_before_setup_wait', C.c_int32), ('pen_ready_wait', C.c_int32),
                    ('pen_taken_wait', C.c_int32), ('pen_nr_kicks', C.c_int32), ('pen_max_extra_kicks', C.c_int32),
                    ('pen_dist_x', C.c_double), ('illegal_defense_number', C.c_int32), ('illegal_defense_duration', C.c_int32),
                    ('illegal_defense_dist_x', C.c_double), ('illegal_defense_width', C.c_double),
                    ('pen_allow_mult_kicks', C.c_int32), ('pen_random_winner', C.c_int32)]


PLAYER_TYPE_FIELDS = ('player_speed_max', 'stamina_inc_max', 'player_decay', 'inertia_moment', 'dash_power_rate',
                      'player_size', 'kickable_margin', 'kick_rand', 'extra_stamina', 'effort_max', 'effort_min',
                      'kick_power_rate', 'catchable_area_l_stretch')


class S2DPlayerType(C.Structure):          # idl/service.proto:1697-1732 (members that enter the dynamics)
    _fields_ = [(n, C.c_double) for n in PLAYER_TYPE_FIELDS]


class S2DPlayerParams(C.Structure):        # idl/service.proto:1664-1695
    _fields_ = [(n, C.c_double) for n in (
        'player_speed_max_delta_min', 'player_speed_max_delta_max', 'stamina_inc_max_delta_factor',
        'player_decay_delta_min', 'player_decay_delta_max', 'inertia_moment_delta_factor',
        'dash_power_rate_delta_min', 'dash_power_rate_delta_max', 'player_size_delta_factor',
        'kickable_margin_delta_min', 'kickable_margin_delta_max', 'kick_rand_delta_factor',
        'extra_stamina_delta_min', 'extra_stamina_delta_max', 'effort_max_delta_factor', 'effort_min_delta_factor',
        'new_dash_power_rate_delta_min', 'new_dash_power_rate_delta_max', 'new_stamina_inc_max_delta_factor',
        'kick_power_rate_delta_min', 'kick_power_rate_delta_max',
        'catchable_area_l_stretch_min', 'catchable_area_l_stretch_max')]


class S2DMatchConfig(C.Structure):
    _fields_ = [('abi_version', C.c_uint32), ('struct_bytes', C.c_uint32),
                ('sp', _capi.S2DServerParams), ('mp', S2DMatchParams),
                ('seed', C.c_uint64), ('env_id_offset', C.c_int64),
                ('auto_reset', C.c_int32), ('noise', C.c_int32), ('reserved', C.c_int32 * 4),
                ('player_types', S2DPlayerType * MATCH_PLAYER_TYPES), ('player_type_id', C.c_int32 * MATCH_SLOTS)]


_F, _I, _U8 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
# (name, ctypes type, torch dtype, per-env trailing shape; None = stats[8])
MATCH_BUFFER_FIELDS = tuple(
    [(n, _F, 'float32', (MATCH_SLOTS,)) for n in ('x', 'y', 'vx', 'vy', 'body', 'stamina', 'effort', 'recovery', 'stamina_capacity')]
    + [('tackle_cycles', _I, 'int32', (MATCH_SLOTS,)), ('catch_ban', _I, 'int32', (MATCH_SLOTS,))]
    + [(n, _I, 'int32', ()) for n in ('cycle', 'mode', 'mode_side', 'score_left', 'score_right', 'last_touch_side',
                                      'setplay_timer', 'offside_mask', 'ball_holder', 'goalie_moves', 'set_play_taker',
                                      'last_kicker', 'stopped_cycle', 'tick')]
    + [('card', _I, 'int32', (MATCH_SLOTS,))]
    + [('reward_left', _F, 'float32', ()), ('done', _U8, 'uint8', ()),
       ('nearest_left', _I, 'int32', ()), ('nearest_right', _I, 'int32', ()),
       ('stats', C.POINTER(C.c_ulonglong), 'int64', None)])


class S2DMatchBuffers(C.Structure):
    _fields_ = [('n_envs', C.c_int64)] + [(n, t) for (n, t, _, _) in MATCH_BUFFER_FIELDS]


class S2DMatchRollout(C.Structure):
    _fields_ = [('obs', C.c_void_p), ('reward', C.c_void_p), ('mode', C.c_void_p), ('done', C.c_void_p)]


class S2DMatchNet(C.Structure):             # include/s2d_match.h: network slots
    _fields_ = [('h1', C.c_int32), ('h2', C.c_int32), ('n_actions', C.c_int32), ('slot_mask', C.c_uint32),
                ('params', C.c_void_p), ('epsilon', C.c_void_p), ('table', C.c_void_p)]


class S2DMatchPolicyNet(C.Structure):       # include/s2d_match.h: policy slots
    _fields_ = [('h1', C.c_int32), ('h2', C.c_int32), ('n_actions', C.c_int32), ('slot_mask', C.c_uint32),
                ('activation', C.c_int32), ('params', C.c_void_p), ('deterministic', C.c_void_p), ('table', C.c_void_p)]


MATCH_ROLE_NETWORK = 0                     # S2D_MATCH_ROLE_NETWORK: the role s2d_match_set_network fills
MATCH_ROLE_OPPONENT = 1                    # S2D_MATCH_ROLE_OPPONENT: the role s2d_match_set_opponent_network fills


VISION_PARAM_FIELDS = ('visible_distance', 'dist_quantize_step', 'dist_round', 'dist_chg_quantize', 'dir_chg_quantize',
                       'unum_far_length', 'unum_too_far_length', 'team_far_length', 'team_too_far_length',
                       'min_neck_moment', 'max_neck_moment', 'min_neck_angle', 'max_neck_angle')


class S2DVisionParams(C.Structure):         # include/s2d_match.h: Vision
    _fields_ = [('view_angle', C.c_double * 3), ('see_interval', C.c_double * 3)] + [(n, C.c_double) for n in VISION_PARAM_FIELDS]


class S2DMatchVision(C.Structure):          # the caller-owned vision planes, [N][24] each
    _fields_ = [('neck', C.c_void_p), ('view_width', C.c_void_p), ('see_wait', C.c_void_p)]


BELIEF_PARAM_FIELDS = ('ball_decay', 'player_decay', 'match_dist', 'match_rate', 'ghost_margin', 'count_max')


class S2DBeliefParams(C.Structure):         # include/s2d_match.h: Belief
    _fields_ = [('ball_decay', C.c_double), ('player_decay', C.c_double), ('view_angle', C.c_double * 3),
                ('match_dist', C.c_double), ('match_rate', C.c_double), ('ghost_margin', C.c_double), ('count_max', C.c_double)]


HEAR_PARAM_FIELDS = ('audio_cut_dist', 'hear_max', 'hear_inc', 'hear_decay', 'say_msg_size', 'say_levels')


class S2DHearParams(C.Structure):           # include/s2d_match.h: Hearing
    _fields_ = [(n, C.c_double) for n in HEAR_PARAM_FIELDS]


class S2DMatchHear(C.Structure):            # the caller-owned hear planes: three [N][24], the rows [N][22][32]
    _fields_ = [('cap_our', C.c_void_p), ('cap_opp', C.c_void_p), ('attention', C.c_void_p), ('hear', C.c_void_p)]


class S2DMatchSeeNet(C.Structure):          # include/s2d_match.h: see network
    _fields_ = [('h1', C.c_int32), ('h2', C.c_int32), ('n_actions', C.c_int32), ('slot_mask', C.c_uint32),
                ('params', C.c_void_p), ('epsilon', C.c_void_p), ('table', C.c_void_p),
                ('prm', S2DVisionParams), ('vis', S2DMatchVision)]


class S2DMatchSeePolicyNet(C.Structure):    # include/s2d_match.h: see policy slots
    _fields_ = [('h1', C.c_int32), ('h2', C.c_int32), ('n_actions', C.c_int32), ('slot_mask', C.c_uint32),
                ('params', C.c_void_p), ('deterministic', C.c_void_p), ('table', C.c_void_p),
                ('prm', S2DVisionParams), ('vis', S2DMatchVision), ('activation', C.c_int32)]


class S2DMatchBeliefNet(C.Structure):       # include/s2d_match.h: Belief network
    _fields_ = [('h1', C.c_int32), ('h2', C.c_int32), ('n_actions', C.c_int32), ('slot_mask', C.c_uint32),
                ('params', C.c_void_p), ('table', C.c_void_p), ('prm', S2DVisionParams), ('vis', S2DMatchVision),
                ('head', C.c_int32), ('activation', C.c_int32), ('epsilon', C.c_void_p), ('deterministic', C.c_void_p),
                ('belief_prm', S2DBeliefParams), ('belief', C.c_void_p), ('belief_mask', C.c_uint32)]


class S2DMatchAgentReward(C.Structure):     # include/s2d_match.h: Agent reward
    _fields_ = [('weights', C.c_void_p), ('chaser_only', C.c_int32)]


REWARD_TERMS = ('goal', 'ball_advance', 'approach', 'facing', 'kickable', 'possession')   # S2D_MATCH_REWARD_TERMS, in term order

MATCH_NET_WIDTHS = (16, 32, 48, 64)
MATCH_NET_MAX_ACTIONS = 64
MATCH_ST_NET = 7                           # S2D_MATCH_ST_NET: Philox stream of the network slots' exploration


MATCH_PROTOTYPES = (
    ('s2d_match_default_config', None, (C.POINTER(S2DMatchConfig),)),
    ('s2d_match_default_player_params', None, (C.POINTER(S2DPlayerParams),)),
    ('s2d_match_generate_player_types', C.c_int, (C.POINTER(S2DMatchConfig), C.POINTER(S2DPlayerParams), C.c_uint64)),
    ('s2d_match_validate_config', C.c_int, (C.POINTER(S2DMatchConfig),)),
    ('s2d_match_arena_bytes', C.c_size_t, (C.POINTER(S2DMatchConfig), C.c_int64)),
    ('s2d_match_create', C.c_int, (C.POINTER(S2DMatchConfig), C.c_int64, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                   C.POINTER(C.c_void_p))),
    ('s2d_match_destroy', None, (C.c_void_p,)),
    ('s2d_match_buffers', C.c_int, (C.c_void_p, C.POINTER(S2DMatchBuffers))),
    ('s2d_match_buffer_offsets', C.c_int, (C.c_void_p, C.POINTER(C.c_int64), C.c_int)),
    ('s2d_match_reset', C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_match_step', C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_match_rollout', C.c_int, (C.c_void_p, C.c_int, C.c_void_p, C.POINTER(S2DMatchRollout), C.c_void_p)),
    ('s2d_match_relative', C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_match_kernel_name', C.c_char_p, (C.c_void_p,)),
    ('s2d_match_set_controllers', C.c_int, (C.c_void_p, C.c_void_p)),
    ('s2d_match_rollout_ex', C.c_int, (C.c_void_p, C.c_int, C.c_void_p, C.POINTER(S2DMatchRollout), C.c_void_p, C.c_void_p)),
    ('s2d_match_agent_obs', C.c_int, (C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p)),
    ('s2d_match_set_network', C.c_int, (C.c_void_p, C.c_void_p)),
    ('s2d_match_set_opponent_network', C.c_int, (C.c_void_p, C.c_void_p)),
    ('s2d_match_rollout_net', C.c_int, (C.c_void_p, C.c_int, C.c_void_p, C.POINTER(S2DMatchRollout), C.c_void_p, C.c_void_p,
                                        C.c_uint32, C.c_void_p, C.c_void_p)),
    ('s2d_match_vision_default_params', None, (C.POINTER(S2DVisionParams),)),
    ('s2d_match_vision_validate', C.c_int, (C.POINTER(S2DVisionParams),)),
    ('s2d_match_vision_reset', C.c_int, (C.c_void_p, C.POINTER(S2DMatchVision), C.c_void_p, C.c_void_p)),
    ('s2d_match_vision_step', C.c_int, (C.c_void_p, C.POINTER(S2DVisionParams), C.POINTER(S2DMatchVision), C.c_void_p, C.c_void_p,
                                        C.c_void_p)),
    ('s2d_match_see', C.c_int, (C.c_void_p, C.POINTER(S2DVisionParams), C.POINTER(S2DMatchVision), C.c_uint32, C.c_void_p,
                                C.c_void_p)),
    ('s2d_match_belief_default_params', None, (C.POINTER(S2DBeliefParams),)),
    ('s2d_match_belief_validate', C.c_int, (C.POINTER(S2DBeliefParams),)),
    ('s2d_match_belief_reset', C.c_int, (C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p)),
    ('s2d_match_belief_scan', C.c_int, (C.POINTER(S2DBeliefParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_int64, C.c_uint32, C.c_void_p)),
    ('s2d_match_hear_default_params', None, (C.POINTER(S2DHearParams),)),
    ('s2d_match_hear_validate', C.c_int, (C.POINTER(S2DHearParams),)),
    ('s2d_match_hear_reset', C.c_int, (C.c_void_p, C.POINTER(S2DHearParams), C.POINTER(S2DMatchHear), C.c_void_p, C.c_void_p)),
    ('s2d_match_hear_step', C.c_int, (C.c_void_p, C.POINTER(S2DHearParams), C.POINTER(S2DMatchHear), C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p)),
    ('s2d_match_set_see_network', C.c_int, (C.c_void_p, C.c_void_p)),
    ('s2d_match_rollout_see', C.c_int, (C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(S2DMatchRollout), C.c_void_p,
                                        C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p)),
    ('s2d_match_set_see_policy_network', C.c_int, (C.c_void_p, C.c_void_p)),
    ('s2d_match_rollout_see_policy', C.c_int, (C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(S2DMatchRollout), C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p)),
    ('s2d_match_set_belief_network', C.c_int, (C.c_void_p, C.c_void_p)),
    ('s2d_match_rollout_belief', C.c_int, (C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(S2DMatchRollout), C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_match_set_policy_network', C.c_int, (C.c_void_p, C.c_int, C.c_void_p)),
    ('s2d_match_rollout_policy', C.c_int, (C.c_void_p, C.c_int, C.c_void_p, C.POINTER(S2DMatchRollout), C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p)),
    ('s2d_match_set_agent_reward', C.c_int, (C.c_void_p, C.c_void_p)),
    ('s2d_match_rollout_reward', C.c_int, (C.c_void_p, C.c_int, C.c_void_p, C.POINTER(S2DMatchRollout), C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)),
)


def bind(lib):
    """Attach restype/argtypes of the match entry points (idempotent)."""
    for name, res, args in MATCH_PROTOTYPES:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = list(args)
    return lib


def controller_codes(spec):
    """22 controller codes (bytes) from `spec`: 22 codes (ints or names), or {'left': c, 'right': c} with c a code or a name
    ('external' | 'random' | 'scripted'; a missing side is external).  None stays None (no table)."""
    if spec is None:
        return None

    def code(v):
        if isinstance(v, str):
            if v not in CTL_CODES:
                raise ValueError(f"unknown controller {v!r} (use one of {sorted(CTL_CODES)})")
            return CTL_CODES[v]
        if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= 2:
            raise ValueError(f"controller code {v!r} is not 0 (external), 1 (random) or 2 (scripted)")
        return int(v)
    if isinstance(spec, dict):
        extra = set(spec) - {'left', 'right'}
        if extra:
            raise ValueError(f"controller spec keys must be 'left' / 'right', got {sorted(extra)}")
        codes = [code(spec.get('left', CTL_EXTERNAL))] * 11 + [code(spec.get('right', CTL_EXTERNAL))] * 11
    else:
        codes = [code(v) for v in spec]
        if len(codes) != MATCH_PLAYERS:
            raise ValueError(f"controller spec needs {MATCH_PLAYERS} codes, got {len(codes)}")
    return bytes(codes)


def reward_weights(weights):
    """the six agent-reward weights (floats, in REWARD_TERMS order) from a dict by term name (missing terms are 0) or a sequence
    of six"""
    if isinstance(weights, dict):
        extra = set(weights) - set(REWARD_TERMS)
        if extra:
            raise ValueError(f"unknown reward terms {sorted(extra)} (the terms: {', '.join(REWARD_TERMS)})")
        return [float(weights.get(k, 0.0)) for k in REWARD_TERMS]
    vals = [float(v) for v in weights]
    if len(vals) != len(REWARD_TERMS):
        raise ValueError(f"reward weights need {len(REWARD_TERMS)} values ({', '.join(REWARD_TERMS)}), got {len(vals)}")
    return vals


def agent_slot_mask(slots):
    """slot mask of s2d_match_agent_obs from 'all' | 'left' | 'right' | an int mask of bits 0..21"""
    if isinstance(slots, str):
        if slots not in AGENT_SLOT_MASKS:
            raise ValueError(f"slots must be one of {sorted(AGENT_SLOT_MASKS)} or a mask, got {slots!r}")
        return AGENT_SLOT_MASKS[slots]
    if isinstance(slots, bool) or int(slots) != slots or not 0 < int(slots) <= 0x3FFFFF:
        raise ValueError(f"slot mask must be a non-empty set of bits 0..21, got {slots!r}")
    return int(slots)


def vision_params(lib, **params):
    """S2DVisionParams: the defaults of s2d_match_vision_default_params with `params` written over them (view_angle and
    see_interval: three values, narrow / normal / wide), validated by s2d_match_vision_validate."""
    from . import _capi
    prm = S2DVisionParams()
    lib.s2d_match_vision_default_params(C.byref(prm))
    for k, v in params.items():
        if k in ('view_angle', 'see_interval'):
            vals = [float(x) for x in v]
            if len(vals) != 3:
                raise ValueError(f"{k} needs three values (narrow, normal, wide)")
            for i, x in enumerate(vals):
                getattr(prm, k)[i] = x
        elif k in VISION_PARAM_FIELDS:
            setattr(prm, k, float(v))
        else:
            raise ValueError(f"unknown vision parameter {k!r}")
    _capi.check(lib, lib.s2d_match_vision_validate(C.byref(prm)), 's2d_match_vision_validate')
    return prm


def belief_params(lib, **params):
    """S2DBeliefParams: the defaults of s2d_match_belief_default_params with `params` written over them (view_angle: three
    values, narrow / normal / wide), validated by s2d_match_belief_validate."""
    prm = S2DBeliefParams()
    lib.s2d_match_belief_default_params(C.byref(prm))
    for k, v in params.items():
        if k == 'view_angle':
            vals = [float(x) for x in v]
            if len(vals) != 3:
                raise ValueError("view_angle needs three values (narrow, normal, wide)")
            for i, x in enumerate(vals):
                prm.view_angle[i] = x
        elif k in BELIEF_PARAM_FIELDS:
            setattr(prm, k, float(v))
        else:
            raise ValueError(f"unknown belief parameter {k!r}")
    _capi.check(lib, lib.s2d_match_belief_validate(C.byref(prm)), 's2d_match_belief_validate')
    return prm


def hear_params(lib, **params):
    """S2DHearParams: the defaults of s2d_match_hear_default_params with `params` written over them, validated by
    s2d_match_hear_validate."""
    prm = S2DHearParams()
    lib.s2d_match_hear_default_params(C.byref(prm))
    for k, v in params.items():
        if k not in HEAR_PARAM_FIELDS:
            raise ValueError(f"unknown hear parameter {k!r}")
        setattr(prm, k, float(v))
    _capi.check(lib, lib.s2d_match_hear_validate(C.byref(prm)), 's2d_match_hear_validate')
    return prm
