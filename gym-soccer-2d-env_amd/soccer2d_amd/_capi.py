"""ctypes mirror of include/s2d.h (the C ABI of libs2d_hip.so) and the loader.

No compute happens here: structs, prototypes and error translation only.  The library is
loaded AFTER ``import torch`` so that its ``libamdhip64.so.7`` dependency resolves to the
HIP runtime torch already mapped (one runtime per process: torch's streams and device
memory are then valid in the engine).

The product path has no CPU fallback: if the HIP library is missing or does not load,
``load_library()`` raises ``S2DLibraryError``.
"""
import ctypes as C
import os

S2D_ABI_VERSION = 4
S2D_OBS_DIM = 10

# error codes
S2D_OK, S2D_EINVAL, S2D_EHIP, S2D_ENOMEM, S2D_ENODEV = 0, -1, -2, -3, -4
# enums (include/s2d.h)
MODE_BEFORE_KICK_OFF, MODE_TIME_OVER, MODE_PLAY_ON = 0, 1, 2
SIDE_UNKNOWN, SIDE_LEFT, SIDE_RIGHT = 0, 1, 2
RESULT_NONE, RESULT_GOAL, RESULT_OUT, RESULT_TIMEOUT = 0, 1, 2, 3
RESULT_NAMES = (None, 'Goal', 'Out', 'Timeout')   # info['result'], reach_ball_env.py:126-150
CMD_NONE, CMD_DASH, CMD_TURN, CMD_FREEZE = 0, 1, 2, -1
ACT_DISCRETE_I32, ACT_DISCRETE_I64, ACT_CONTINUOUS, ACT_TURNING, ACT_RANDOM, ACT_COMMAND = 0, 1, 2, 3, 4, 5
NOISE_LATTICE, NOISE_RCSSSERVER = 0, 1
NOISE_MODELS = {'lattice': NOISE_LATTICE, 'rcssserver': NOISE_RCSSSERVER}   # S2DConfig.noise_model by name


class S2DLibraryError(RuntimeError):
    """libs2d_hip.so is missing / failed to load.  There is no fallback path."""


class S2DServerParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        'pitch_half_length', 'pitch_half_width',
        'player_size', 'player_decay', 'player_rand', 'player_speed_max', 'player_accel_max',
        'inertia_moment',
        'stamina_max', 'stamina_inc_max', 'stamina_capacity', 'extra_stamina',
        'recover_init', 'recover_dec_thr', 'recover_min', 'recover_dec',
        'effort_init', 'effort_dec_thr', 'effort_min', 'effort_dec', 'effort_inc_thr', 'effort_inc',
        'dash_power_rate', 'max_dash_power', 'min_dash_power',
        'max_dash_angle', 'min_dash_angle', 'dash_angle_step', 'side_dash_rate', 'back_dash_rate',
        'max_moment', 'min_moment',
        'ball_size', 'ball_decay', 'ball_rand', 'ball_speed_max', 'ball_accel_max',
        'collision_vel_rate')]


class S2DReachBallParams(C.Structure):
    _fields_ = [
        ('change_ball_position', C.c_int32), ('change_ball_velocity', C.c_int32),
        ('ball_position_x', C.c_double), ('ball_position_y', C.c_double),
        ('ball_speed', C.c_double), ('ball_direction', C.c_double),
        ('min_distance_to_ball', C.c_double),
        ('max_steps', C.c_int32), ('use_continuous_action', C.c_int32),
        ('action_space_size', C.c_int32), ('use_turning', C.c_int32),
        ('reset_ball_decay', C.c_double)]


class S2DConfig(C.Structure):
    _fields_ = [
        ('abi_version', C.c_uint32), ('struct_bytes', C.c_uint32),
        ('sp', S2DServerParams), ('task', S2DReachBallParams),
        ('seed', C.c_uint64), ('env_id_offset', C.c_int64),
        ('auto_reset', C.c_int32), ('noise', C.c_int32), ('noise_model', C.c_int32), ('reserved', C.c_int32 * 3)]


_F = C.POINTER(C.c_float)
_U8 = C.POINTER(C.c_uint8)
_I32 = C.POINTER(C.c_int32)

# (name, ctypes pointer type, torch dtype name, trailing dims) in S2DBuffers order
BUFFER_FIELDS = (
    ('player_x', _F, 'float32', ()), ('player_y', _F, 'float32', ()),
    ('player_vx', _F, 'float32', ()), ('player_vy', _F, 'float32', ()),
    ('player_body', _F, 'float32', ()),
    ('stamina', _F, 'float32', ()), ('effort', _F, 'float32', ()),
    ('recovery', _F, 'float32', ()), ('stamina_capacity', _F, 'float32', ()),
    ('ball_x', _F, 'float32', ()), ('ball_y', _F, 'float32', ()),
    ('ball_vx', _F, 'float32', ()), ('ball_vy', _F, 'float32', ()),
    ('prev_dist', _F, 'float32', ()), ('prev_angle', _F, 'float32', ()),
    ('step_number', _I32, 'int32', ()), ('cycle', _I32, 'int32', ()),
    ('policy_step', _I32, 'int32', ()), ('episode', _I32, 'int32', ()),
    ('obs', _F, 'float32', (S2D_OBS_DIM,)), ('reward', _F, 'float32', ()),
    ('done', _U8, 'uint8', ()), ('result', _U8, 'uint8', ()),
    ('terminal_obs', _F, 'float32', (S2D_OBS_DIM,)),
    ('action_dir', _F, 'float32', ()), ('action_cmd', _U8, 'uint8', ()),
    ('stats', C.POINTER(C.c_ulonglong), 'int64', None),   # [8], not per-env
)
STATE_FIELDS = tuple(f[0] for f in BUFFER_FIELDS[:19])


class S2DBuffers(C.Structure):
    _fields_ = [('n_envs', C.c_int64)] + [(n, t) for (n, t, _, _) in BUFFER_FIELDS]


class S2DRollout(C.Structure):
    _fields_ = [('obs', C.c_void_p), ('action', C.c_void_p), ('reward', C.c_void_p),
                ('done', C.c_void_p), ('result', C.c_void_p)]


class S2DQNet(C.Structure):
    """the caller's Q-network of s2d_rollout_qnet (widths, device pointers of the packed parameters and of epsilon)"""
    _fields_ = [('hidden1', C.c_int32), ('hidden2', C.c_int32), ('n_actions', C.c_int32), ('reserved', C.c_int32),
                ('params', C.c_void_p), ('epsilon', C.c_void_p)]


class S2DActorNet(C.Structure):
    """the caller's deterministic actor of s2d_rollout_actor (widths, outputs, noise kind; device pointers of the packed
    parameters, of epsilon and of the [2][n_out] (mu, sigma) noise buffer)"""
    _fields_ = [('hidden1', C.c_int32), ('hidden2', C.c_int32), ('n_out', C.c_int32), ('noise_kind', C.c_int32),
                ('params', C.c_void_p), ('epsilon', C.c_void_p), ('noise', C.c_void_p)]


class S2DPolicyNet(C.Structure):
    """the caller's stochastic policy of s2d_rollout_policy (widths, outputs, activation 0 ReLU / 1 Tanh; device pointers of the
    packed parameters, of log_std[n_out] (NULL on a discrete engine) and of the deterministic word)"""
    _fields_ = [('hidden1', C.c_int32), ('hidden2', C.c_int32), ('n_out', C.c_int32), ('activation', C.c_int32),
                ('params', C.c_void_p), ('log_std', C.c_void_p), ('deterministic', C.c_void_p)]


class S2DMlpNet(C.Structure):
    """the caller's general MLP of s2d_rollout_qnet_mlp / s2d_rollout_actor_mlp (1 .. 4 hidden widths, outputs, activation 0 ReLU
    / 1 Tanh, noise kind; device pointers as S2DQNet's / S2DActorNet's)"""
    _fields_ = [('n_hidden', C.c_int32), ('hidden', C.c_int32 * 4), ('n_out', C.c_int32), ('activation', C.c_int32),
                ('noise_kind', C.c_int32), ('params', C.c_void_p), ('epsilon', C.c_void_p), ('noise', C.c_void_p)]


class S2DWideNet(C.Structure):
    """the caller's streamed-weight MLP of s2d_rollout_qnet_wide / s2d_rollout_actor_wide (1 .. 5 hidden widths up to 400, outputs,
    activation 0 ReLU / 1 Tanh / 2 Sigmoid, noise kind; device pointers as S2DMlpNet's, and the workspace the pack kernel writes)"""
    _fields_ = [('n_hidden', C.c_int32), ('hidden', C.c_int32 * 5), ('n_out', C.c_int32), ('activation', C.c_int32),
                ('noise_kind', C.c_int32), ('params', C.c_void_p), ('epsilon', C.c_void_p), ('noise', C.c_void_p),
                ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t)]


class S2DReplayRing(C.Structure):
    """the caller-owned ring of s2d_replay_push / s2d_replay_sample (capacity in transitions; device pointers of the five arrays)"""
    _fields_ = [('capacity', C.c_int64), ('obs', C.c_void_p), ('next_obs', C.c_void_p), ('action', C.c_void_p),
                ('reward', C.c_void_p), ('discount', C.c_void_p)]


class S2DEpisodeRing(C.Structure):
    """the caller-owned ring of s2d_episode_stats (device pointers of the five arrays, capacity in episodes)"""
    _fields_ = [('ret', C.c_void_p), ('length', C.c_void_p), ('result', C.c_void_p), ('env', C.c_void_p), ('step', C.c_void_p),
                ('capacity', C.c_int64)]


class S2DLearnNet(C.Structure):
    """the network of s2d_learn_q / s2d_learn_q_grad: S2DTdNet's shape on the learner's grid, its READ-WRITE parameters and the
    workspace of the blocks' partial gradients"""
    _fields_ = [('n_in', C.c_int32), ('n_hidden', C.c_int32), ('hidden', C.c_int32 * 5), ('n_out', C.c_int32),
                ('activation', C.c_int32), ('params', C.c_void_p), ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t)]


class S2DLearnState(C.Structure):
    """the optimiser's device state: Adam's moments and the summed gradient [P], hyper = (lr, beta1, beta2, eps, max_grad_norm,
    beta1^t, beta2^t), stats = (loss, norm, scale), the error word and the loss (0 MSE, 1 Huber)"""
    _fields_ = [('m', C.c_void_p), ('v', C.c_void_p), ('grad', C.c_void_p), ('hyper', C.c_void_p), ('stats', C.c_void_p),
                ('error', C.c_void_p), ('loss_kind', C.c_int32)]


class S2DLearnPPO(C.Structure):
    """the learner of s2d_learn_ppo: the shapes of pi and vf, the head (0 categorical, 1 Gaussian), the flat [pi | vf | log_std]
    parameters with their Adam state and gradient, hyper[10], stats[8], the error word and the workspace"""
    _fields_ = [('pi', S2DLearnNet), ('vf', S2DLearnNet), ('head', C.c_int32), ('normalize_advantage', C.c_int32),
                ('params', C.c_void_p), ('m', C.c_void_p), ('v', C.c_void_p), ('grad', C.c_void_p), ('hyper', C.c_void_p),
                ('stats', C.c_void_p), ('error', C.c_void_p), ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t)]


class S2DLearnSacAlpha(C.Structure):
    """the temperature's state of s2d_learn_sac_actor: log_alpha [1], Adam's (m, v) [2], hyper [7] as S2DLearnState's, stats =
    (mean logp, alpha loss, alpha after the call) and the target entropy"""
    _fields_ = [('log_alpha', C.c_void_p), ('m_v', C.c_void_p), ('hyper', C.c_void_p), ('stats', C.c_void_p),
                ('target_entropy', C.c_float)]


class S2DLearnPPOBatch(C.Structure):
    """the rollout arrays of R rows and the minibatch of B rows that `index` (or NULL) names in them"""
    _fields_ = [('rows', C.c_int64), ('batch', C.c_int64), ('obs', C.c_void_p), ('action', C.c_void_p), ('logp_old', C.c_void_p),
                ('advantage', C.c_void_p), ('ret', C.c_void_p), ('index', C.c_void_p), ('out_logp', C.c_void_p),
                ('out_value', C.c_void_p)]


class S2DTdNet(C.Structure):
    """one network of s2d_td_target_q / s2d_td_target_ac: S2DWideNet's MLP with a run-time input width (1 .. 256), the device
    pointer of its packed parameters and the workspace the pack kernel writes"""
    _fields_ = [('n_in', C.c_int32), ('n_hidden', C.c_int32), ('hidden', C.c_int32 * 5), ('n_out', C.c_int32),
                ('activation', C.c_int32), ('params', C.c_void_p), ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t)]


WORLD_MODEL_FIELDS = (
    'ball_dist_from_self', 'ball_angle_from_self', 'ball_relative_x', 'ball_relative_y',
    'ball_pos_dist', 'ball_pos_angle', 'ball_vel_dist', 'ball_vel_angle',
    'self_pos_dist', 'self_pos_angle', 'self_vel_dist', 'self_vel_angle',
    'self_dist_from_ball', 'self_angle_from_ball')


class S2DWorldModel(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in WORLD_MODEL_FIELDS]


# every symbol include/s2d.h declares: (name, restype, argtypes)
PROTOTYPES = (
    ('s2d_version', C.c_char_p, ()),
    ('s2d_last_error', C.c_char_p, ()),
    ('s2d_default_config', None, (C.POINTER(S2DConfig),)),
    ('s2d_validate_config', C.c_int, (C.POINTER(S2DConfig),)),
    ('s2d_arena_bytes', C.c_size_t, (C.POINTER(S2DConfig), C.c_int64)),
    ('s2d_create', C.c_int, (C.POINTER(S2DConfig), C.c_int64, C.c_int, C.c_void_p, C.c_size_t,
                             C.c_void_p, C.POINTER(C.c_void_p))),
    ('s2d_destroy', None, (C.c_void_p,)),
    ('s2d_buffers', C.c_int, (C.c_void_p, C.POINTER(S2DBuffers))),
    ('s2d_buffer_offsets', C.c_int, (C.c_void_p, C.POINTER(C.c_int64), C.c_int)),
    ('s2d_reset', C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_step', C.c_int, (C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)),
    ('s2d_rollout', C.c_int, (C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(S2DRollout), C.c_void_p)),
    ('s2d_step_k', C.c_int, (C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(S2DRollout), C.c_void_p)),
    ('s2d_rollout_qnet', C.c_int, (C.c_void_p, C.c_int, C.POINTER(S2DQNet), C.POINTER(S2DRollout), C.c_void_p, C.c_void_p)),
    ('s2d_rollout_actor', C.c_int, (C.c_void_p, C.c_int, C.POINTER(S2DActorNet), C.POINTER(S2DRollout), C.c_void_p, C.c_void_p)),
    ('s2d_rollout_qnet_mlp', C.c_int, (C.c_void_p, C.c_int, C.POINTER(S2DMlpNet), C.POINTER(S2DRollout), C.c_void_p, C.c_void_p)),
    ('s2d_rollout_actor_mlp', C.c_int, (C.c_void_p, C.c_int, C.POINTER(S2DMlpNet), C.POINTER(S2DRollout), C.c_void_p, C.c_void_p)),
    ('s2d_wide_workspace_bytes', C.c_size_t, (C.POINTER(S2DWideNet),)),
    ('s2d_rollout_qnet_wide', C.c_int, (C.c_void_p, C.c_int, C.POINTER(S2DWideNet), C.POINTER(S2DRollout), C.c_void_p, C.c_void_p)),
    ('s2d_rollout_actor_wide', C.c_int, (C.c_void_p, C.c_int, C.POINTER(S2DWideNet), C.POINTER(S2DRollout), C.c_void_p, C.c_void_p)),
    ('s2d_rollout_policy', C.c_int, (C.c_void_p, C.c_int, C.POINTER(S2DPolicyNet), C.POINTER(S2DRollout), C.c_void_p, C.c_void_p,
                                     C.c_void_p)),
    ('s2d_rollout_sac', C.c_int, (C.c_void_p, C.c_int, C.POINTER(S2DWideNet), C.c_void_p, C.POINTER(S2DRollout), C.c_void_p, C.c_void_p,
                                  C.c_void_p)),
    ('s2d_gae', C.c_int, (C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                          C.c_float, C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_replay_push', C.c_int, (C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(S2DReplayRing), C.c_void_p, C.c_void_p)),
    ('s2d_replay_sample', C.c_int, (C.c_int64, C.c_int, C.c_int, C.POINTER(S2DReplayRing), C.c_void_p, C.c_uint64, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_replay_tree_words', C.c_int64, (C.c_int64,)),
    ('s2d_replay_prio_push', C.c_int, (C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_replay_prio_update', C.c_int, (C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_replay_sample_prio', C.c_int, (C.c_int64, C.c_int, C.c_int, C.POINTER(S2DReplayRing), C.c_void_p, C.c_void_p, C.c_uint64,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p)),
    ('s2d_episode_stats_workspace', C.c_size_t, (C.c_int, C.c_int64)),
    ('s2d_episode_stats', C.c_int, (C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.POINTER(S2DEpisodeRing), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)),
    ('s2d_td_workspace_bytes', C.c_size_t, (C.POINTER(S2DTdNet),)),
    ('s2d_td_target_q', C.c_int, (C.c_int64, C.POINTER(S2DTdNet), C.POINTER(S2DTdNet), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_td_target_ac', C.c_int, (C.c_int64, C.POINTER(S2DTdNet), C.POINTER(S2DTdNet), C.POINTER(S2DTdNet), C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_td_target_td3', C.c_int, (C.c_int64, C.POINTER(S2DTdNet), C.POINTER(S2DTdNet), C.POINTER(S2DTdNet), C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_td_target_sac', C.c_int, (C.c_int64, C.POINTER(S2DTdNet), C.POINTER(S2DTdNet), C.POINTER(S2DTdNet), C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p)),
    ('s2d_debug_td_target_sac', C.c_int, (C.c_int64, C.POINTER(S2DTdNet), C.POINTER(S2DTdNet), C.POINTER(S2DTdNet), C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p)),
    ('s2d_learn_workspace_bytes', C.c_size_t, (C.POINTER(S2DLearnNet), C.c_int64)),
    ('s2d_learn_q', C.c_int, (C.c_int64, C.POINTER(S2DLearnNet), C.POINTER(S2DLearnState), C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_learn_q_grad', C.c_int, (C.c_int64, C.POINTER(S2DLearnNet), C.POINTER(S2DLearnState), C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_learn_critic', C.c_int, (C.c_int64, C.POINTER(S2DLearnNet), C.POINTER(S2DLearnState), C.c_void_p, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_learn_critic_grad', C.c_int, (C.c_int64, C.POINTER(S2DLearnNet), C.POINTER(S2DLearnState), C.c_void_p, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_learn_actor', C.c_int, (C.c_int64, C.POINTER(S2DLearnNet), C.POINTER(S2DLearnState), C.POINTER(S2DLearnNet), C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_learn_actor_grad', C.c_int, (C.c_int64, C.POINTER(S2DLearnNet), C.POINTER(S2DLearnState), C.POINTER(S2DLearnNet), C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_learn_actor_workspace_bytes', C.c_size_t, (C.POINTER(S2DLearnNet), C.POINTER(S2DLearnNet), C.c_int64)),
    ('s2d_learn_ppo_workspace_bytes', C.c_size_t, (C.POINTER(S2DLearnNet), C.POINTER(S2DLearnNet), C.c_int32, C.c_int64)),
    ('s2d_learn_ppo', C.c_int, (C.POINTER(S2DLearnPPO), C.POINTER(S2DLearnPPOBatch), C.c_void_p)),
    ('s2d_learn_ppo_grad', C.c_int, (C.POINTER(S2DLearnPPO), C.POINTER(S2DLearnPPOBatch), C.c_void_p)),
    ('s2d_learn_sac_actor', C.c_int, (C.c_int64, C.POINTER(S2DLearnNet), C.POINTER(S2DLearnState), C.POINTER(S2DLearnNet),
                                      C.POINTER(S2DLearnNet), C.c_void_p, C.c_void_p, C.POINTER(S2DLearnSacAlpha), C.c_void_p, C.c_uint64,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_learn_sac_actor_grad', C.c_int, (C.c_int64, C.POINTER(S2DLearnNet), C.POINTER(S2DLearnState), C.POINTER(S2DLearnNet),
                                           C.POINTER(S2DLearnNet), C.c_void_p, C.c_void_p, C.POINTER(S2DLearnSacAlpha), C.c_void_p,
                                           C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_learn_sac_workspace_bytes', C.c_size_t, (C.POINTER(S2DLearnNet), C.POINTER(S2DLearnNet), C.POINTER(S2DLearnNet), C.c_int64)),
    ('s2d_world_model', C.c_int, (C.c_void_p, C.POINTER(S2DWorldModel), C.c_void_p)),
    ('s2d_stats_reset', C.c_int, (C.c_void_p, C.c_void_p)),
    ('s2d_kernel_name', C.c_char_p, (C.c_void_p,)),
    ('s2d_validate_state', C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p)),
    ('s2d_set_seed', C.c_int, (C.c_void_p, C.c_uint64, C.c_void_p)),
    ('s2d_debug_eval', C.c_int, (C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)),
    ('s2d_debug_net_forward', C.c_int, (C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                        C.c_char_p, C.c_void_p)),
    ('s2d_debug_mlp_forward', C.c_int, (C.POINTER(S2DMlpNet), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p)),
    ('s2d_debug_wide_forward', C.c_int, (C.POINTER(S2DWideNet), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p)),
    ('s2d_debug_policy_head', C.c_int, (C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int,
                                        C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)),
)

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(PKG_ROOT, 'lib', 'libs2d_hip.so')

_lib = None


def load_library(path=None):
    """Load libs2d_hip.so and bind every prototype.  Raises S2DLibraryError on failure."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    import torch  # noqa: F401  -- maps torch's libamdhip64.so.7 first (see module docstring)
    p = path or os.environ.get('S2D_LIB', LIB_PATH)
    if not os.path.exists(p):
        raise S2DLibraryError(
            f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(or `make -C gym-soccer-2d-env_amd/csrc`). There is no CPU fallback.")
    try:
        lib = C.CDLL(p, mode=C.RTLD_GLOBAL)
    except OSError as e:
        raise S2DLibraryError(f"cannot load {p}: {e}") from e
    for name, res, args in PROTOTYPES:
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise S2DLibraryError(f"{p} does not export {name}") from e
        fn.restype = res
        fn.argtypes = list(args)
    _lib = lib
    return lib


def check(lib, rc, what):
    """Translate a C return code into the Python exception the boundary promises
    (SURVEY.md 8b 'Errors': ValueError for bad arguments, RuntimeError for HIP errors)."""
    if rc == S2D_OK:
        return
    msg = lib.s2d_last_error()
    msg = msg.decode() if msg else ''
    text = f"{what} failed ({rc}): {msg}"
    if rc == S2D_EINVAL:
        raise ValueError(text)
    if rc == S2D_ENOMEM:
        raise MemoryError(text)
    raise RuntimeError(text)
