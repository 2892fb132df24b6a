/*
 * s2d.h -- C ABI of the MI355X-native batched 2D-soccer engine (libs2d_hip.so).
 *
 * This is the drop-in boundary for the `reach_ball` hot path of
 * CLSFramework/gym-soccer-2d-env.  The reference has no C ABI / FFI of its own (its
 * boundary is the Python gym.Env surface); each entry point below therefore cites the
 * reference *Python* interface it replaces (file:line under /root/reference):
 *
 *   s2d_create / s2d_destroy   Soccer2DEnv.__init__ / close      soccer_2d_env.py:30-95, 280-299
 *                              (spawn rcssserver + proxy + gRPC  -> one in-process engine)
 *   s2d_reset                  Soccer2DEnv.reset -> abs_reset -> env_reset
 *                              soccer_2d_env.py:179-224, reach_ball_env.py:163-218
 *   s2d_step                   Soccer2DEnv.step                  soccer_2d_env.py:226-269
 *                              + ReachBallEnv hooks              reach_ball_env.py:53-161
 *   s2d_rollout                SB3 collect_rollouts loop over step()  dqn_stable_baselines3.py:41-55
 *                              (T fused steps, random policy or caller actions)
 *   s2d_rollout_qnet           DQN("MlpPolicy").predict inside SB3's collect_rollouts  dqn_stable_baselines3.py:36-49
 *                              (T fused steps, epsilon-greedy actions of the caller's Q-network, in-kernel)
 *   s2d_rollout_actor          DDPG / TD3 actor.mu + NormalActionNoise inside SB3's collect_rollouts
 *                              ddpg_stable_baselines3.py (T fused steps, the caller's tanh policy, in-kernel)
 *   s2d_rollout_qnet_wide / s2d_rollout_actor_wide   the same with the networks the reference's scripts build by default or
 *                              search over: SB3's DDPG("MlpPolicy") actor [400, 300] (ddpg_stable_baselines3.py), the Optuna
 *                              grids of best_python_sample_soccer_env*.py (up to five layers of 400, Sigmoid)
 *   s2d_rollout_policy         PPO / A2C: sampling from the policy's distribution + log_prob inside collect_rollouts
 *   s2d_gae                    RolloutBuffer.compute_returns_and_advantage
 *   s2d_replay_push            ReplayBuffer.add with handle_timeout_termination, for a whole [T][N] record at once, in the place
 *                              of the per-step add of OffPolicyAlgorithm.collect_rollouts (n-step returns formed on the way in)
 *   s2d_replay_sample          ReplayBuffer.sample (uniform, with replacement)
 *   s2d_replay_prio_push / s2d_replay_sample_prio / s2d_replay_prio_update   proportional prioritized replay (Schaul et al.,
 *                              2016; SB3 has none) on a sum tree over the same ring
 *   s2d_episode_stats          Monitor's episode returns / lengths (ep_info_buffer: ep_rew_mean, ep_len_mean) and the results
 *                              InfoCollectorCallback tallies, for a whole [T][N] record at once
 *   s2d_world_model            protobuf State/WorldModel fields  idl/service.proto:22-27, 68-86,
 *                              144-223, 306-349 (returned as device arrays, not wire bytes)
 *   S2DConfig                  ReachBallEnv kwargs               reach_ball_env.py:26-36
 *                              + ServerParam / PlayerType names  idl/service.proto:1435-1732
 *
 * Plain C: pointers and sizes only, no torch / C++ types.  All `*_dev` pointers are HIP
 * device pointers; `stream` is a hipStream_t passed as void* (NULL = the null stream).
 * Every launch function is stream-ordered, asynchronous and hipGraph-capturable (no
 * allocation, no synchronisation inside).  One engine per (process, GPU); a handle is not
 * thread-safe, different handles are independent.
 */
#ifndef S2D_H_
#define S2D_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S2D_ABI_VERSION 4

/* ---- error codes (0 = ok, negative = failure; text via s2d_last_error()) ------------ */
enum {
  S2D_OK = 0,
  S2D_EINVAL = -1,   /* bad argument / config (Python raises ValueError)           */
  S2D_EHIP = -2,     /* a HIP runtime call failed (Python raises RuntimeError)      */
  S2D_ENOMEM = -3,   /* arena too small / allocation failed                         */
  S2D_ENODEV = -4    /* no usable gfx950 device                                     */
};

/* ---- enums mirroring the reference ---------------------------------------------------- */
/* GameModeType values, idl/service.proto:267-301 (only the ones the path can reach).    */
enum { S2D_MODE_BEFORE_KICK_OFF = 0, S2D_MODE_TIME_OVER = 1, S2D_MODE_PLAY_ON = 2 };
/* Side, idl/service.proto:88-92 */
enum { S2D_SIDE_UNKNOWN = 0, S2D_SIDE_LEFT = 1, S2D_SIDE_RIGHT = 2 };
/* info['result'] labels, reach_ball_env.py:126-150 (None / 'Goal' / 'Out' / 'Timeout') */
enum { S2D_RESULT_NONE = 0, S2D_RESULT_GOAL = 1, S2D_RESULT_OUT = 2, S2D_RESULT_TIMEOUT = 3 };
/* low-level body commands = PlayerAction oneof members, idl/service.proto:380-397 */
enum { S2D_CMD_NONE = 0, S2D_CMD_DASH = 1, S2D_CMD_TURN = 2,
       S2D_CMD_FREEZE = -1 /* S2D_ACT_COMMAND only: this env does not take part in the cycle (state and outputs stay as they are) --
                            * how a host mirror lets ONE env of a batch consume its reset cycle (soccer_2d_env.py:187-197) */ };

/* how `actions_dev` of s2d_step / s2d_rollout is laid out (reach_ball_env.py:39-47, 53-85) */
enum {
  S2D_ACT_DISCRETE_I32 = 0, /* int32[N]    Discrete(n)                                   */
  S2D_ACT_DISCRETE_I64 = 1, /* int64[N]    same, torch's default integer dtype           */
  S2D_ACT_CONTINUOUS = 2,   /* float[N][1] Box(-1,1,(1,))  rel_dir = a*180 (not clipped) */
  S2D_ACT_TURNING = 3,      /* float[N][4] Box(-1,1,(4,))  [turn_p, turn_a, dash_p, dash_a] */
  S2D_ACT_RANDOM = 4,       /* NULL: uniform random policy drawn in-kernel (Philox)      */
  /* float[N][4] = {S2D_CMD_*, power, relative direction, 0}: one decoded PlayerAction body command per env, executed as it is
   * (what the proxy does with `ignore_preprocess=True`, server.py:64) -- the boundary of the reference's task HOOK
   * `action_to_rpc_actions` (soccer_2d_env.py:317-325): a user-defined task env builds pb2.PlayerAction objects in Python and the
   * host mirror turns them into this array.  Accepted by s2d_step in every task mode (16-byte aligned); not by s2d_rollout.
   * (The env-step counter of the episode statistics counts every env of the launch, frozen ones included.) */
  S2D_ACT_COMMAND = 5   /* the command word is read as the nearest of -1 / 0 / 1 / 2 (S2D_CMD_*); any other number, NaN included, is
                         * S2D_CMD_NONE */
};

/* velocity noise of MPObject::_inc (S2DConfig.noise_model) */
enum {
  S2D_NOISE_LATTICE = 0,    /* default: polar(U(0, m) on a 2^-16 grid, a whole degree), m = rand |v|; E|dv|^2 = m^2 / 3 */
  S2D_NOISE_RCSSSERVER = 1  /* rcssserver's MPObject::noise(): (drand(-m, m), drand(-m, m)); E|dv|^2 = 2 m^2 / 3.  Needs
                             * noise = 1.  The two-envs-per-lane rollout (S2D_ROLLOUT_E=2) does not have it and falls back. */
};

/* ---- configuration -------------------------------------------------------------------- */
/* Physics parameters.  Field names follow ServerParam / PlayerType of idl/service.proto:
 * 1435-1732.  The reference never holds their VALUES (rcssserver sends them at run time,
 * server.py:105-118); the defaults of s2d_default_config() are rcssserver's stock values
 * (EXT / parity-unpinned).  Doubles here; each engine rounds to its
 * own arithmetic type (the HIP engine computes in float).                                 */
typedef struct S2DServerParams {
  double pitch_half_length;  /* 52.5  reach_ball_env.py:100,142 */
  double pitch_half_width;   /* 34.0  reach_ball_env.py:101,142 */
  double player_size, player_decay, player_rand, player_speed_max, player_accel_max;
  double inertia_moment;
  double stamina_max, stamina_inc_max, stamina_capacity, extra_stamina;
  double recover_init, recover_dec_thr, recover_min, recover_dec;
  double effort_init, effort_dec_thr, effort_min, effort_dec, effort_inc_thr, effort_inc;
  double dash_power_rate, max_dash_power, min_dash_power;
  double max_dash_angle, min_dash_angle, dash_angle_step, side_dash_rate, back_dash_rate;
  double max_moment, min_moment;
  double ball_size, ball_decay, ball_rand, ball_speed_max, ball_accel_max;
  double collision_vel_rate; /* -0.1: velocity factor applied to collided objects          */
} S2DServerParams;

/* Task parameters = ReachBallEnv kwargs, reach_ball_env.py:26-36, same names/defaults.   */
typedef struct S2DReachBallParams {
  int32_t change_ball_position;  /* True  */
  int32_t change_ball_velocity;  /* False */
  double ball_position_x, ball_position_y, ball_speed, ball_direction; /* 0 */
  double min_distance_to_ball;   /* 5.0 */
  int32_t max_steps;             /* 200 */
  int32_t use_continuous_action; /* True */
  int32_t action_space_size;     /* 16  */
  int32_t use_turning;           /* False */
  double reset_ball_decay;       /* 0.96: literal used by get_ball_velocity, reach_ball_env.py:207 */
} S2DReachBallParams;

typedef struct S2DConfig {
  uint32_t abi_version;   /* S2D_ABI_VERSION */
  uint32_t struct_bytes;  /* sizeof(S2DConfig), checked by s2d_create */
  S2DServerParams sp;
  S2DReachBallParams task;
  uint64_t seed;          /* Philox key; resets use stream 0, random policy stream 1, ... */
  int64_t env_id_offset;  /* global id of local env 0 (multi-GPU sharding: results are
                             invariant to how the global env range is cut into shards)   */
  int32_t auto_reset;     /* 1: a done env is reset inside the same step (SB3 VecEnv
                             convention); 0: caller resets (reference single-env flow)   */
  int32_t noise;          /* 0: player_rand/ball_rand ignored (parity mode); 1: Philox noise */
  int32_t noise_model;    /* S2D_NOISE_*: form of the velocity noise when noise = 1 (was reserved[0], which older
                             callers zero: they get the lattice) */
  int32_t reserved[3];
} S2DConfig;

/* ---- device buffers --------------------------------------------------------------------
 * All arrays are struct-of-arrays over the N local envs (one contiguous array per field,
 * 256-byte aligned), except obs / terminal_obs which are row-major [N][10] as PyTorch
 * consumers expect.  Valid for the life of the handle; contents change at every
 * s2d_step / s2d_reset / s2d_rollout.                                                     */
#define S2D_OBS_DIM 10
#define S2D_STATS_STRIPES 64
/* rows of S2DBuffers.stats of an engine of n envs: one per group of 64 envs (its wave owns it), at least S2D_STATS_STRIPES */
#define S2D_STATS_ROWS(n) ((((n) + 63) / 64) > S2D_STATS_STRIPES ? (((n) + 63) / 64) : S2D_STATS_STRIPES)
typedef struct S2DBuffers {
  int64_t n_envs;
  /* state, row S of SURVEY.md 8(a): 15 float + 2 int32 words per env (+ policy_step, which only
   * launches that draw in-engine policy randomness read or write) */
  float *player_x, *player_y, *player_vx, *player_vy, *player_body; /* body in degrees [-180,180] */
  float *stamina, *effort, *recovery, *stamina_capacity;
  float *ball_x, *ball_y, *ball_vx, *ball_vy;
  float *prev_dist, *prev_angle;  /* carry of check_trainer_observation, reach_ball_env.py:158-159 */
  int32_t *step_number;           /* reach_ball_env.py:55, 172 */
  int32_t *cycle;                 /* WorldModel.cycle, idl/service.proto:326 */
  int32_t *policy_step;           /* steps that consumed an in-engine policy / select draw (S2D_ACT_RANDOM,
                                   * or any step of a use_turning env): the Philox counter of those draws */
  int32_t *episode;               /* resets so far = index of the current episode (0 before the first reset): the
                                   * Philox counter of the reset sampler, so that episode j of env g is a function of
                                   * (g, j) alone and can be prepared ahead of the simulation */
  /* per-step outputs */
  float *obs;            /* [N][10]  reach_ball_env.py:98-107 */
  float *reward;         /* [N] */
  uint8_t *done;         /* [N] 0/1 */
  uint8_t *result;       /* [N] S2D_RESULT_* */
  float *terminal_obs;   /* [N][10] observation of the finished episode (valid where done) */
  float *action_dir;     /* [N] decoded relative direction in degrees of the last command  */
  uint8_t *action_cmd;   /* [N] S2D_CMD_* of the last command                              */
  /* episode statistics, one row per group of 64 envs (plain load / store by the wave that owns the group, no atomics):
   * stats[S2D_STATS_ROWS(n_envs)][8]; the value of counter k is the sum over rows of [r][k].
   * k: 0 = env-steps, 1 = Goal, 2 = Out, 3 = Timeout, 4..7 reserved                        */
  unsigned long long *stats;
} S2DBuffers;

/* Caller-owned rollout buffers for s2d_rollout, time-major (any pointer may be NULL to
 * skip that output).  T = n_steps, N = local envs.                                        */
typedef struct S2DRollout {
  float *obs;        /* [T][N][10] observation returned by step t (post auto-reset)        */
  void *action;      /* [T][N] int32 (discrete) | float[T][N][1] | float[T][N][4]          */
  float *reward;     /* [T][N] */
  uint8_t *done;     /* [T][N] */
  uint8_t *result;   /* [T][N] */
} S2DRollout;

/* The caller's Q-network for s2d_rollout_qnet (DESIGN.md sections 4, 5): q = W3 relu(W2 relu(W1 x + b1) + b2) + b3 on the
 * env's 10-word observation x.  hidden1 / hidden2 in {16, 32, ..., 128}; n_actions = task.action_space_size, 1 .. 64.
 * params: ONE contiguous fp32 device buffer, 16-byte aligned, in torch's nn.Sequential(Linear, ReLU, Linear, ReLU, Linear)
 * .parameters() order: W1[H1][10], b1[H1], W2[H2][H1], b2[H2], W3[A][H2], b3[A].  epsilon: one fp32 device word.  Both are
 * read when the kernel runs (a captured graph acts with what they hold at replay).  reserved: 0.                          */
typedef struct S2DQNet {
  int32_t hidden1, hidden2, n_actions, reserved;
  const float *params;
  const float *epsilon;
} S2DQNet;

/* The caller's deterministic actor for s2d_rollout_actor (DESIGN.md sections 4, 5): a = tanh(W3 relu(W2 relu(W1 x + b1) + b2)
 * + b3), SB3's DDPG / TD3 actor.mu.  hidden1 / hidden2 in {16, 32, ..., 128} (the weights live in LDS; SB3's default
 * net_arch=[400, 300] does not fit there: s2d_rollout_actor_wide streams it, S2DWideNet); n_out = 1 (use_continuous_action, not turning) or
 * 4 (use_turning).  params as S2DQNet's (W3[n_out][H2], b3[n_out]), 16-byte aligned; epsilon: one fp32 device word; noise:
 * fp32 device buffer [2][n_out] = (mu, sigma) of the Gaussian action noise, required when noise_kind = 1 (0: no action noise,
 * noise may be NULL).  params, epsilon and noise are read when the kernel runs; noise_kind selects the instantiation.  */
typedef struct S2DActorNet {
  int32_t hidden1, hidden2, n_out, noise_kind;
  const float *params;
  const float *epsilon;
  const float *noise;
} S2DActorNet;

/* The caller's stochastic policy for s2d_rollout_policy (DESIGN.md sections 4, 5): y = W3 f(W2 f(W1 x + b1) + b2) + b3, f =
 * relu (activation = 0) or tanh_spec (1, SB3's default for PPO's MlpPolicy); y = the logits of a categorical policy on a discrete
 * engine (n_out = action_space_size, 1 .. 64), the means of a diagonal Gaussian on a continuous (n_out = 1) or turning (4) one.
 * hidden1 / hidden2 in {16, 32, ..., 128}.  params as S2DQNet's (W3[n_out][H2], b3[n_out]), 16-byte aligned.  log_std: fp32
 * device buffer [n_out], SB3's state-independent log_std parameter (may be NULL on a discrete engine).  deterministic: one
 * uint32 device word, 0 = sample, non-zero = act greedily.  params, log_std and deterministic are read when the kernel runs (a
 * captured graph acts with what they hold at replay: an evaluation pass is the collection graph with the word set).  */
typedef struct S2DPolicyNet {
  int32_t hidden1, hidden2, n_out, activation;
  const float *params;
  const float *log_std;
  const uint32_t *deterministic;
} S2DPolicyNet;

/* The caller's network for s2d_rollout_qnet_mlp / s2d_rollout_actor_mlp: a general MLP 10 -> h_1 -> ... -> h_L -> n_out (DESIGN.md
 * section 4), for the networks SB3's policy_kwargs=dict(net_arch=[...], activation_fn=...) build.  One to four hidden layers;
 * every hidden width a multiple of 8 in [8, 128] (the weights live in LDS); one hidden activation for the whole network, relu or
 * tanh_spec; the output layer is linear.  The observation is x[0..9], h_0 = 10:
 *   params    torch's nn.Sequential(Linear, F, ..., Linear).parameters() order: W_1[h_1][10], b_1, ..., W_L[h_L][h_(L-1)], b_L,
 *             W_out[n_out][h_L], b_out, in one contiguous, 16-byte aligned fp32 device buffer;
 *   units     every unit is acc = b[j]; for k ascending: acc = fmaf(W[j][k], in[k], acc);
 *   layer 1   runs over k = 0 .. 11 with x_10 = x_11 = 0 against zero weights: two more fmaf(0, 0, acc), which turn an
 *             accumulator of -0 into +0 (invisible behind relu, visible behind tanh_spec; part of the spec);
 *   layers 2 .. L and the output layer run over exactly k = 0 .. h_(l-1) - 1 (a width that is a multiple of 8 but not of 16
 *             pads the output rows of its tile; no padded unit is ever read and no extra fmaf enters a chain);
 *   hidden    relu(v) = v > 0 ? v : +0, or tanh_spec(v);
 *   heads     s2d_rollout_qnet's (the argmax scan, epsilon-greedy at policy_step k, Philox blocks 0 and 2) and
 *             s2d_rollout_actor's (tanh_spec(y_j), optional Gaussian noise from block 3, clip, epsilon-random exploration),
 *             unchanged: no draw, key or counter differs.
 * With n_hidden = 2, both widths multiples of 16 and activation 0 the result is s2d_rollout_qnet's / s2d_rollout_actor's bit
 * for bit.  epsilon and noise as S2DQNet's / S2DActorNet's; params, epsilon and noise are read when the kernel runs.  A
 * network whose fragments and biases plus one wave's images exceed the 160 KiB LDS of a workgroup is refused
 * ([128, 64, 32, 16] with 16 outputs runs with 2 waves per workgroup; [128, 128, 128] does not fit). */
typedef struct S2DMlpNet {
  int32_t n_hidden;        /* 1 .. 4 */
  int32_t hidden[4];       /* multiples of 8 in [8, 128]; entries past n_hidden are 0 */
  int32_t n_out;           /* Q: action_space_size, 1 .. 64; tanh actor: 1 | 4 */
  int32_t activation;      /* 0 relu, 1 tanh_spec */
  int32_t noise_kind;      /* tanh actor only: 0 | 1; must be 0 for the Q actor */
  const float *params, *epsilon, *noise;   /* as S2DQNet / S2DActorNet */
} S2DMlpNet;

/* The caller's network for s2d_rollout_qnet_wide / s2d_rollout_actor_wide: S2DMlpNet's MLP on a wider grid, with the weights
 * streamed from memory instead of living in LDS (DESIGN.md sections 4, 7): every network the reference's scripts can build --
 * SB3's default DDPG actor [400, 300], the Optuna grids layer_size in {8, ..., 400} x n_layers in 1..5 x {ReLU, Tanh, Sigmoid}.
 *   shape     10 -> h_1 -> ... -> h_L -> n_out, L in 1..5; every hidden width a multiple of 4 (the MFMA's k-step) in [8, 400];
 *             one hidden activation for the whole network; the output layer is linear;
 *   params    as S2DMlpNet's: nn.Sequential(...).parameters() order in one contiguous, 16-byte aligned fp32 device buffer;
 *   units     acc = b[j]; for k ascending: acc = fmaf(W[j][k], in[k], acc); layer 1 over k = 0 .. 11 (x_10 = x_11 = 0 against zero
 *             weights: an accumulator of -0 becomes +0), later layers over exactly h_(l-1) terms (a width that is no multiple
 *             of 16 pads the output rows of its last tile; no padded unit is ever read);
 *   hidden    relu(v) = v > 0 ? v : +0, tanh_spec(v), or sigmoid_spec(v): a = min(|v|, 87) (NaN: 87), t = exp_spec(-a),
 *             d = 1 + t, v >= 0 ? 1 / d : t / d (correctly rounded), NaN passes; +-0 -> 0.5, +inf -> 1, v <= -87 ->
 *             exp_spec(-87) = 1.6458115e-38 rather than 0;
 *   heads     s2d_rollout_qnet's and s2d_rollout_actor's, unchanged: no draw, key or counter differs.
 * On every shape S2DMlpNet takes (L <= 4, widths multiples of 8 up to 128, relu or tanh, fitting the LDS) the result is the
 * _mlp entry points' bit for bit.
 *   workspace a 256-byte aligned device buffer of at least s2d_wide_workspace_bytes() bytes, where every call first writes
 *             the parameters in the matrix cores' fragment order (a pack kernel on the caller's stream) and the rollout kernel
 *             then reads them: params, epsilon and noise are still read when the kernels run, and a captured graph holds both
 *             nodes and acts with what the buffers hold at replay.  A workspace belongs to ONE launch at a time: two launches
 *             that may overlap (two streams, two engines) need a workspace each. */
typedef struct S2DWideNet {
  int32_t n_hidden;        /* 1 .. 5 */
  int32_t hidden[5];       /* multiples of 4 in [8, 400]; entries past n_hidden are 0 */
  int32_t n_out;           /* Q: action_space_size, 1 .. 64; tanh actor: 1 | 4 */
  int32_t activation;      /* 0 relu, 1 tanh_spec, 2 sigmoid_spec */
  int32_t noise_kind;      /* tanh actor only: 0 | 1; must be 0 for the Q actor */
  const float *params, *epsilon, *noise;   /* as S2DMlpNet */
  void *workspace;         /* 256-byte aligned device memory, written by every call */
  size_t workspace_bytes;  /* >= s2d_wide_workspace_bytes(this shape) */
} S2DWideNet;

/* Derived protobuf-mirroring fields that are not plain state words (row T1).  Each array
 * is [N]; NULL pointers are skipped.                                                       */
typedef struct S2DWorldModel {
  float *ball_dist_from_self;    /* Ball.dist_from_self   idl/service.proto:84 */
  float *ball_angle_from_self;   /* Ball.angle_from_self  idl/service.proto:85 */
  float *ball_relative_x, *ball_relative_y; /* Ball.relative_position idl/service.proto:70 */
  float *ball_pos_dist, *ball_pos_angle;    /* RpcVector2D.dist/.angle of Ball.position :25-26 */
  float *ball_vel_dist, *ball_vel_angle;    /* ... of Ball.velocity */
  float *self_pos_dist, *self_pos_angle;    /* ... of Self.position */
  float *self_vel_dist, *self_vel_angle;    /* ... of Self.velocity */
  float *self_dist_from_ball;    /* Self.dist_from_ball   idl/service.proto:204 */
  float *self_angle_from_ball;   /* Self.angle_from_ball  idl/service.proto:205 */
} S2DWorldModel;

typedef struct S2DEngine *S2DHandle;

/* ---- entry points ---------------------------------------------------------------------- */
const char *s2d_version(void);
/* last error text of the calling thread ("" if none) */
const char *s2d_last_error(void);
/* rcssserver stock ServerParam/PlayerType(0) values + ReachBallEnv kwargs defaults */
void s2d_default_config(S2DConfig *cfg);
/* 0 if cfg is acceptable, else S2D_EINVAL with s2d_last_error() set */
int s2d_validate_config(const S2DConfig *cfg);
/* bytes of device memory an engine of n_envs needs (0 on bad input) */
size_t s2d_arena_bytes(const S2DConfig *cfg, int64_t n_envs);
/* arena_dev == NULL: the engine hipMallocs (and owns) its arena; otherwise the caller owns
 * `arena_dev` (>= s2d_arena_bytes, 256-byte aligned) and keeps it alive until s2d_destroy.
 * The arena is zero-filled and the state initialised on `stream`. */
int s2d_create(const S2DConfig *cfg, int64_t n_envs, int device, void *arena_dev,
               size_t arena_bytes, void *stream, S2DHandle *out);
void s2d_destroy(S2DHandle h);
int s2d_buffers(S2DHandle h, S2DBuffers *out);
/* byte offset of every S2DBuffers pointer from the arena base, same field order
 * (n_envs slot = arena size); lets a host language build zero-copy views of an arena
 * it allocated itself. */
int s2d_buffer_offsets(S2DHandle h, int64_t *offsets, int n_offsets);
/* reset envs where mask_dev[i] != 0 (NULL = all): reach_ball_env.py:170-218 sampler, then
 * ONE simulator cycle (soccer_2d_env.py:187-197), obs + carry refreshed. */
int s2d_reset(S2DHandle h, const uint8_t *mask_dev, void *stream);
/* one cycle for every env: decode action, dash/turn, stamina, integrate, collide, decay,
 * obs, reward/done/result, auto-reset under cfg.auto_reset. */
int s2d_step(S2DHandle h, const void *actions_dev, int action_kind, void *stream);
/* k cycles (1 <= k <= 64) of the per-step API in ONE launch, for callers that hold their actions for k steps ahead (action repeat,
 * open-loop chunks): actions_dev is [k][N] in `action_kind` layout (or NULL with S2D_ACT_RANDOM); `out` (may be NULL, and any of its
 * arrays may be NULL) receives the per-step record [k][N]; the arena's per-step outputs hold the last step.  Same results as k calls
 * of s2d_step (soccer_2d_env.py:226-269 each); no prologue, the state makes one round trip. */
int s2d_step_k(S2DHandle h, int k, const void *actions_dev, int action_kind, const S2DRollout *out, void *stream);
/* n_steps cycles fused in ONE launch (state stays in registers).  actions_dev is
 * [T][N] in `action_kind` layout, or NULL with S2D_ACT_RANDOM. */
int s2d_rollout(S2DHandle h, int n_steps, const void *actions_dev, int action_kind,
                const S2DRollout *out, void *stream);
/* n_steps >= 1 cycles fused in ONE launch (discrete-action engines only) whose action at every cycle is the caller's
 * Q-network, epsilon-greedy per env:
 *   greedy  = the first index of the largest q (ties: lowest index; a NaN never replaces the current best), every output
 *             an fmaf chain from its bias in ascending k, relu(v) = v > 0 ? v : +0;
 *   explore = word k & 3 of Philox block 2 of stream POLICY at counter k >> 2 < thr, k = the env's policy_step (advanced by
 *             one every step), thr = eps >= 1 ? 2^32 : eps > 0 ? (uint64)(eps 2^32) : 0 (NaN: 0);
 *   the random action is S2D_ACT_RANDOM's draw, so eps = 1 is s2d_rollout(NULL, S2D_ACT_RANDOM) bit for bit.
 * The action of step t is chosen from the observation step t - 1 returned (t = 0: the observation of the launch's start
 * state).  `out` as for s2d_rollout (action = int32[T][N]); terminal_obs (may be NULL) = float[T][N][10], written only where
 * done[t][i] (the observation the episode ended on).  Rejected without a launch: continuous / turning engines, widths not in
 * {16, ..., 128} step 16, n_actions != action_space_size or > 64, NULL or misaligned params / epsilon, n_steps < 1. */
int s2d_rollout_qnet(S2DHandle h, int n_steps, const S2DQNet *net, const S2DRollout *out, float *terminal_obs, void *stream);
/* n_steps >= 1 cycles fused in ONE launch (continuous or turning engines) whose action at every cycle is the caller's tanh
 * policy on the env's observation, per env and step at its policy_step k (advanced by one every step):
 *   explore (as s2d_rollout_qnet's) -> S2D_ACT_RANDOM's draw for the mode, without action noise (eps = 1 is
 *             s2d_rollout(NULL, S2D_ACT_RANDOM) bit for bit);
 *   else      a_j = tanh_spec(y_j), with noise_kind = 1 clip(tanh_spec(y_j) + (mu_j + sigma_j z_j)) (one fmaf), clip to [-1, 1],
 *             z from Box-Muller on Philox block 3 of stream POLICY: turning z0..z3 of the block at counter k, continuous
 *             z_{k & 3} of the block at counter k >> 2.
 * The action then goes through the mode's action map (turning: the softmax and the SELECT draw).  `out` as for s2d_rollout
 * (action = float[T][N][1] | float[T][N][4]: the noisy, clipped action, what SB3's replay buffer stores); terminal_obs as for
 * s2d_rollout_qnet.  Rejected without a launch: discrete engines, n_out != the mode's A, widths not in {16, ..., 128} step
 * 16, noise_kind not in {0, 1}, NULL or misaligned params / epsilon / noise (noise only with kind 1), n_steps < 1, a network
 * that does not fit the LDS. */
int s2d_rollout_actor(S2DHandle h, int n_steps, const S2DActorNet *net, const S2DRollout *out, float *terminal_obs, void *stream);
/* s2d_rollout_qnet (discrete engines) and s2d_rollout_actor (continuous and turning engines) with the general MLP of S2DMlpNet.
 * Records, terminal_obs, graph capture, policy_step, statistics and the per-step outputs behave as their two-layer
 * counterparts'; s2d_kernel_name() names the instantiation with its shape and waves per workgroup
 * (...<noise=0,act=tanh,h=128-64-32-16,a=16,waves=2>).  Rejected with S2D_EINVAL, without a launch and with the state untouched:
 * n_hidden outside 1..4, a width that is not a multiple of 8 in [8, 128], a non-zero hidden[] entry past n_hidden, activation
 * outside {0, 1}, the wrong engine mode or an n_out that is not the engine's (action_space_size <= 64 | 1 | 4), noise_kind set
 * on the Q path or outside {0, 1}, NULL or misaligned params / epsilon / noise (noise only with kind 1), n_steps < 1, and a
 * network that does not fit the LDS (the error text says how many bytes it needs). */
int s2d_rollout_qnet_mlp(S2DHandle h, int n_steps, const S2DMlpNet *net, const S2DRollout *out, float *terminal_obs, void *stream);
int s2d_rollout_actor_mlp(S2DHandle h, int n_steps, const S2DMlpNet *net, const S2DRollout *out, float *terminal_obs, void *stream);
/* bytes of the workspace of S2DWideNet for `shape` (n_hidden, hidden and n_out are read): the fragment-order copy of the
 * parameters, every layer's weights in tile-major fragments of 64 words with zero padding, then the biases padded to their tiles.
 * 0 for a shape off the grid. */
size_t s2d_wide_workspace_bytes(const S2DWideNet *shape);
/* s2d_rollout_qnet_mlp / s2d_rollout_actor_mlp with the streamed-weight network of S2DWideNet.  A call enqueues two kernels on
 * `stream`: the pack kernel (params -> workspace) and the rollout.  Records, terminal_obs, policy_step, statistics and the
 * per-step outputs behave as the _mlp pair's; s2d_kernel_name() names the instantiation with its shape, its waves per workgroup
 * and its env tiles per pass (...<noise=0,act=sigmoid,h=400-300,a=16,waves=2,tiles=1>); neither enters the result.  Rejected with
 * S2D_EINVAL, without a launch and with the state untouched, the error text naming the field: n_hidden outside 1..5, a width
 * that is not a multiple of 4 in [8, 400], a non-zero hidden[] entry past n_hidden, activation outside {0, 1, 2}, the wrong
 * engine mode or an n_out that is not the engine's, noise_kind set on the Q path or outside {0, 1}, NULL or misaligned params /
 * epsilon / noise / workspace, workspace_bytes too small (the text says how many bytes are needed), n_steps < 1.  (The
 * environment variable S2D_WIDE_PLAN=waves,tiles, read at every launch, overrides the plan for testing.) */
int s2d_rollout_qnet_wide(S2DHandle h, int n_steps, const S2DWideNet *net, const S2DRollout *out, float *terminal_obs, void *stream);
int s2d_rollout_actor_wide(S2DHandle h, int n_steps, const S2DWideNet *net, const S2DRollout *out, float *terminal_obs, void *stream);
/* n_steps >= 1 cycles fused in ONE launch (every action mode) whose action at every cycle is SAMPLED from the caller's policy
 * on the env's observation, with the log-probability of the action taken recorded: on-policy collection (PPO / A2C).  Per env
 * and step at its policy_step k (advanced by one every step); every line one fixed fp32 operation:
 *   network   every unit an fmaf chain from its bias in ascending k; hidden units then relu(v) = v > 0 ? v : +0 or
 *             tanh_spec(v); layer 1 runs over k = 0 .. 11 with x_10 = x_11 = 0 against zero weights (two fmaf(0, 0, acc): an
 *             accumulator of -0 becomes +0, visible only through tanh_spec); the output layer is linear.
 *   discrete  m = max of y[0 .. A-1] by the argmax scan of s2d_rollout_qnet (ascending; a NaN never replaces the best), g = its
 *             index; e_a = exp_spec(y_a - m); S = e_0, S += e_a for ascending a; u = (w >> 8) 2^-24 with w = word k & 3 of
 *             Philox block 4 of stream POLICY at counter k >> 2; target = u * S; c = 0, the action is the first a with
 *             (c += e_a) > target, or g if there is none (u * S rounds up to S; non-finite logits);
 *             logp = (y_a - m) - log_spec(S).  The action is in [0, A) for every input; non-finite logits are otherwise out
 *             of contract.
 *   continuous / turning   sigma_j = exp_spec(log_std_j); z from Box-Muller on Philox block 3 of stream POLICY, laid out as
 *             s2d_rollout_actor's (turning: z0..z3 of the block at counter k; continuous: z_{k & 3} of the block at counter
 *             k >> 2; s2d_debug_eval op 15); a_j = fmaf(sigma_j, z_j, y_j), RECORDED UNCLIPPED (what SB3's rollout buffer
 *             stores); the env receives clip(a_j, -1, 1) = a < -1 ? -1 : a > 1 ? 1 : a through the mode's action map;
 *             logp = t_0 (+ t_1 + t_2 + t_3 in ascending j), t_j = fmaf(-0.5f * z_j, z_j, -log_std_j) - 0.91893853f.
 *   deterministic != 0   greedy: the action is g (discrete) or a_j = clip(y_j, -1, 1) (recorded so), logp as above with
 *             z_j = 0; no Philox draw.  There is no epsilon in this path.
 * `out` as for s2d_rollout (action = int32[T][N] | float[T][N][1] | float[T][N][4]); terminal_obs as for s2d_rollout_qnet;
 * logp (may be NULL) = float[T][N].  policy_step advances by n_steps; the state, the statistics and the per-step outputs
 * are left as s2d_rollout_actor leaves them.  A discrete engine with deterministic != 0 and activation 0 is
 * s2d_rollout_qnet with epsilon = 0 bit for bit.  Rejected without a launch, the state untouched: n_out that is not the
 * engine's (action_space_size | 1 | 4) or > 64, widths not in {16, ..., 128} step 16, activation not in {0, 1}, NULL or
 * misaligned params / deterministic, log_std NULL or misaligned on a continuous or turning engine, n_steps < 1, a network that
 * does not fit the LDS. */
int s2d_rollout_policy(S2DHandle h, int n_steps, const S2DPolicyNet *net, const S2DRollout *out, float *terminal_obs, float *logp,
                       void *stream);
/* Soft Actor-Critic's collection: n_steps >= 1 cycles fused in ONE launch (continuous or turning engines) whose action at every
 * cycle is SAMPLED from the caller's squashed-Gaussian policy with a state-dependent log-std, and its log-probability recorded.
 * The network is S2DWideNet's streamed-weight MLP 10 -> h_1 .. h_L -> n_out = 2A (A = 1 continuous, 4 turning; SB3's default
 * net_arch=[256, 256] runs), the same fmaf chains, pack kernel and workspace as s2d_rollout_actor_wide.  Output rows 0 .. A-1 are
 * the means (SB3's actor.mu), rows A .. 2A-1 the raw log-std (actor.log_std): the flat params are the hidden layers in
 * nn.Sequential order, then W_out[2A][h_L] = [mu.weight ; log_std.weight], b_out = [mu.bias | log_std.bias].  net->epsilon and
 * net->noise must be NULL and noise_kind 0: there is no epsilon in this path (warm-up with uniform actions is S2D_ACT_RANDOM of
 * the plain rollout).  Per env and step at its policy_step k (advanced by one every step), every line one fixed fp32 operation:
 *   ls_j    = v > 2 ? 2 : (v >= -20 ? v : -20), v = y[A + j]  (SB3's LOG_STD_MAX / LOG_STD_MIN; a NaN becomes -20, so exp_spec
 *             never sees a non-finite argument);
 *   sigma_j = exp_spec(ls_j);
 *   z_j     from Box-Muller on Philox block 3 of stream POLICY, laid out exactly as the Gaussian head of the policy rollout above
 *             (turning: z0..z3 of the block at counter k; continuous: z_{k & 3} of the block at counter k >> 2, cached and
 *             refreshed at t == 0 and when k & 3 == 0);
 *   u_j     = fmaf(sigma_j, z_j, y_j); a_j = tanh_spec(u_j).  The record and the env both get a_j (SB3's SAC replay stores the
 *             squashed action; it is already in [-1, 1]); it then goes through the mode's action map;
 *   logp    = t_0 (+ t_1 + t_2 + t_3 in ascending j),
 *             t_j = (fmaf(-0.5f * z_j, z_j, -ls_j) - 0.91893853f) - log_spec(fmaf(-a_j, a_j, 1.0f) + 1e-6f)
 *             (SB3's log(1 - tanh^2 + 1e-6) correction; at a_j = +-1 the argument is exactly 1e-6f);
 *   *deterministic != 0   z_j = 0, u_j = y_j itself (a mean of -0 gives -0), no Philox draw.  The word is read when the kernel
 *             runs: evaluation is the collection graph with the word set.
 * Non-finite means are out of contract, as non-finite logits are above.  Records, terminal_obs, logp (float[T][N] or NULL),
 * policy_step, statistics, per-step outputs and graph capture (two nodes: pack kernel and rollout) behave as the wide tanh
 * actor's and the policy rollout's; the kernel's name carries mode, noise model, activation, widths, waves and tiles (neither of
 * the last two enters the result).  Rejected with S2D_EINVAL, without a launch and with the state untouched, the error text
 * naming the field: a discrete engine, n_out != 2A, a shape off S2DWideNet's grid, non-NULL epsilon / noise or noise_kind != 0,
 * NULL or misaligned params / deterministic / workspace, a workspace too small, n_steps < 1. */
int s2d_rollout_sac(S2DHandle h, int n_steps, const S2DWideNet *net, const uint32_t *deterministic, const S2DRollout *out,
                    float *terminal_obs, float *logp /* [T][N] or NULL */, void *stream);
/* Generalised advantage estimation over a time-major record, one backward scan per env (no engine handle: raw device
 * pointers, any stream of the current device).  ENGINE-INDEPENDENT: it assumes nothing of reach-ball; the 11v11 records have
 * the same [T][N] layout (N = envs, or envs x agents flattened).  Inputs: reward[T][N], done[T][N] (uint8), value[T][N] = V of
 * the observation action t was chosen from, last_value[N] = V of the observation after step T - 1; optionally result[T][N]
 * (uint8) with terminal_value[T][N] = V of the terminal observation (both or neither).  Outputs advantage[T][N], ret[T][N]
 * (they must not overlap the inputs).  fp32, in this order, next_v = last_value, gae = 0, for t = T-1 .. 0:
 *   r = reward[t]; where result[t] == S2D_RESULT_TIMEOUT (and terminal values are given) r = fmaf(gamma, terminal_value[t], r)
 *   (SB3's time-limit bootstrap); nt = done[t] ? 0 : 1; delta = fmaf(gamma * nt, next_v, r) - value[t];
 *   gae = fmaf((gamma * lam) * nt, gae, delta); advantage[t] = gae; ret[t] = gae + value[t]; next_v = value[t].
 * S2D_EINVAL without a launch: n_steps < 1, n_envs < 1, result without terminal_value or the reverse, non-finite gamma / lam,
 * NULL or misaligned arrays. */
int s2d_gae(int n_steps, int64_t n_envs, const float *reward, const uint8_t *done, const float *value, const float *last_value,
            const uint8_t *result, const float *terminal_value, float gamma, float lam, float *advantage, float *ret, void *stream);
/* ---- device replay buffer (off-policy counterpart of s2d_gae) ------------------------------------------------------------
 * ENGINE-INDEPENDENT like s2d_gae: no engine handle, raw device pointers, any stream of the current device; it assumes nothing
 * of reach-ball beyond the S2D_RESULT_TIMEOUT label (GoToCenter and the 11v11 records, agents flattened into N, share it).
 * The ring is caller-owned: `capacity` transitions, 1 <= capacity < 2^31; obs / next_obs = 32-bit words [capacity][D] and
 * action = 32-bit words [capacity][AW] (int32 or float), all copied raw (NaN payloads survive); reward / discount = float
 * [capacity].  D in [1, 1024], AW in [1, 8].  The learner's target is reward + discount * bootstrap(next_obs).
 * `cursor` = device uint64[4] = {pos, size, pushes, samples}, 8-byte aligned, zero at start; both calls read it WHEN THE
 * KERNEL RUNS, so collect -> push -> sample can sit in one captured graph. */
typedef struct S2DReplayRing {
  int64_t capacity;
  void *obs, *next_obs; /* uint32[capacity][D] */
  void *action;         /* uint32[capacity][AW] */
  float *reward, *discount;
} S2DReplayRing;
#define S2D_REPLAY_STREAM 11 /* Philox stream id of the sample indices (no engine draw uses it) */
/* Push a time-major record as n-step transitions, one launch.  first_obs[N][D] = the observation action 0 was chosen from;
 * obs[T][N][D] = what step t returned (post-reset where done); terminal_obs[T][N][D] is read only where done; action[T][N][AW];
 * reward[T][N]; done[T][N] (uint8); result[T][N] (uint8, S2D_RESULT_*) or NULL = every done is a termination.  Requires
 * T * N <= capacity and n_step >= 1.  For every (t, i), fp32, in exactly this order:
 *   R = reward[t][i]; g = gamma; s = t;
 *   while (!done[s][i] && s + 1 < T && s + 1 - t < n_step) { s += 1; R = fmaf(g, reward[s][i], R); g = g * gamma; }
 *   done[s][i]:  next = terminal_obs[s][i];  discount = (result && result[s][i] == S2D_RESULT_TIMEOUT) ? g : +0
 *   else:        next = obs[s][i];           discount = g
 * and slot (pos + t * N + i) mod capacity, pos = cursor[0], receives obs_t = (t == 0 ? first_obs[i] : obs[t - 1][i]), next,
 * action[t][i], R, discount.  A horizon cut by the record's end is a shorter, still valid transition.  A one-thread kernel on
 * the same stream then sets pos = (pos + T * N) mod capacity, size = min(size + T * N, capacity), pushes += 1.
 * S2D_EINVAL without a launch: a range above violated or T * N > capacity, non-finite gamma, NULL (result excepted) or
 * misaligned pointers (4 bytes; 16 bytes for the [.][D] arrays when D % 4 == 0; 8 bytes for the cursor), ring arrays or the
 * cursor overlapping the record or each other. */
int s2d_replay_push(int n_steps, int64_t n_envs, int obs_dim, int action_words, int n_step, float gamma, const void *first_obs,
                    const void *obs, const void *terminal_obs, const void *action, const float *reward, const uint8_t *done,
                    const uint8_t *result, const S2DReplayRing *ring, uint64_t *cursor, void *stream);
/* Sample a batch, one launch.  size = cursor[1] and samples = cursor[3] are read when the kernel runs.  Element b takes word
 * b & 3 of Philox4x32-10 at counter {b >> 2, samples_lo, samples_hi, S2D_REPLAY_STREAM << 16} with key `seed`, and
 * index = ((uint64)w * size) >> 32 (uniform with replacement); the slot's five fields are copied to b_obs[B][D], b_next[B][D],
 * b_action[B][AW], b_reward[B], b_discount[B], and b_index[B] (int32) <- index.  With size == 0: index -1, zero rows, reward
 * and discount +0.  A one-thread kernel then sets samples += 1.  B in [1, 2^31 - 1].  S2D_EINVAL without a launch as above
 * (the batch arrays must not overlap the ring, the cursor or each other). */
int s2d_replay_sample(int64_t batch, int obs_dim, int action_words, const S2DReplayRing *ring, uint64_t *cursor, uint64_t seed,
                      void *b_obs, void *b_next, void *b_action, float *b_reward, float *b_discount, int32_t *b_index, void *stream);
/* ---- prioritized replay: proportional sampling (Schaul et al., 2016) on a sum tree over the same ring ---------------------
 * The library stores and sums priorities exactly as handed over; the exponents alpha and beta stay with the caller, so this
 * contract holds only +, -, /, fmaf and comparisons.  capacity in [1, 2^30]; P = the smallest power of two >= capacity.
 * `tree` = caller-owned device float[2 * P], 8-byte aligned:
 *   tree[P + s]            the leaf (priority) of slot s; leaves of slots >= size are +0
 *   tree[i], 1 <= i < P    tree[2i] + tree[2i+1]: ONE fp32 add, left + right; tree[1] is the total
 *   tree[0]                the largest priority any update has stored; a value below S2D_PRIO_MIN there reads as 1.0f
 * An all-zero array is the valid empty state.  Every priority is clamped on its way in,
 *   clamp(p) = p >= S2D_PRIO_MIN ? (p <= S2D_PRIO_MAX ? p : S2D_PRIO_MAX) : S2D_PRIO_MIN
 * (NaN, zero, negatives and denormals -> MIN, +inf -> MAX), so every stored leaf is a normal positive number, no sum can
 * overflow (2^30 * 2^40) or become denormal, and every node's value is the same whoever computes it and however the work is
 * cut: there is no float atomic and no sum by arrival order anywhere.  Sampling resolves 2^-24 of the total mass (fp32).
 * All calls are stream-ordered, read the cursor WHEN THE KERNEL RUNS and can be captured as a linear chain on one stream. */
#define S2D_REPLAY_PRIO_STREAM 12 /* Philox stream id of the stratified draws (no other draw uses it) */
#define S2D_PRIO_MIN 0x1p-40f
#define S2D_PRIO_MAX 0x1p+40f
/* 2 * P, the tree's length in floats; 0 if capacity is outside [1, 2^30].  Host only, needs no GPU. */
int64_t s2d_replay_tree_words(int64_t capacity);
/* Mark the n slots the next s2d_replay_push of n = T * N transitions will write: with pos = cursor[0] mod capacity and
 * p0 = tree[0] >= S2D_PRIO_MIN ? tree[0] : 1.0f, the leaves of slots (pos + j) mod capacity, j in [0, n), become p0 (new
 * transitions carry the largest priority seen) and every ancestor is made consistent again.  tree[0] and the cursor are
 * untouched.  Requires 1 <= n <= capacity; call it BEFORE s2d_replay_push on the same stream (that call advances pos).
 * S2D_EINVAL without a launch: a range violated, NULL or misaligned (8 bytes) tree / cursor, the tree overlapping the cursor. */
int s2d_replay_prio_push(int64_t n, int64_t capacity, float *tree, const uint64_t *cursor, void *stream);
/* Store new priorities.  size = min(cursor[1], capacity).  Element b is valid iff 0 <= index[b] < size, others are ignored (the
 * -1 of an empty sample is the usual case).  Every slot named by at least one valid element gets leaf = max over those
 * elements of clamp(priority[b]) (with duplicate indices the largest wins); tree[0] = max(tree[0] read as above, every valid
 * element's clamped priority); ancestors are made consistent.  Nothing else changes.  batch in [1, 2^24].  A slot a push has
 * overwritten between the sample and the update simply takes the stale priority.  S2D_EINVAL without a launch: a range
 * violated, NULL or misaligned pointers (4 bytes; 8 for tree and cursor), the tree overlapping cursor, index or priority. */
int s2d_replay_prio_update(int64_t batch, int64_t capacity, float *tree, const uint64_t *cursor, const int32_t *index,
                           const float *priority, void *stream);
/* Sample a batch in proportion to priority, stratified.  total = tree[1], size = min(cursor[1], capacity) and samples =
 * cursor[3] are read when the kernel runs.  If size == 0 or !(total > 0): the zero batch of s2d_replay_sample (index -1, zero
 * rows, reward and discount +0), b_priority +0 and b_total[0] = +0.  Otherwise, with seg = total / (float)B, element b does
 *   w = word (b & 3) of Philox4x32-10 at counter {b >> 2, samples_lo, samples_hi, S2D_REPLAY_PRIO_STREAM << 16}, key seed
 *   u = (float)(w >> 8) * 0x1p-24f
 *   m = fmaf(u, seg, (float)b * seg)                      one draw per segment of the mass
 *   i = 1
 *   while (i < P) { l = tree[2i]; r = tree[2i+1]; if (m >= l && r > 0) { m = m - l; i = 2i + 1; } else i = 2i; }
 *   index = i - P; priority = tree[i]
 * (the r > 0 guard makes rounding drift harmless: every visited node has a positive sum, so the walk ends on a leaf with a
 * positive priority, hence on a slot < size).  The slot's five fields are copied as s2d_replay_sample copies them,
 * b_priority[b] <- priority, b_total[0] <- total, and a one-thread kernel then sets samples += 1.  B in [1, 2^24] ((float)b is
 * exact); ring->capacity in [1, 2^30].  S2D_EINVAL without a launch as for s2d_replay_sample, plus: NULL or misaligned tree (8
 * bytes), b_priority, b_total (4 bytes); the tree overlapping the ring, the cursor or the batch arrays. */
int s2d_replay_sample_prio(int64_t batch, int obs_dim, int action_words, const S2DReplayRing *ring, const float *tree,
                           uint64_t *cursor, uint64_t seed, void *b_obs, void *b_next, void *b_action, float *b_reward,
                           float *b_discount, int32_t *b_index, float *b_priority, float *b_total, void *stream);

/* ---- episode statistics of a record (s2d_episodes.hip): what the person watching the run reads ----
 * The third consumer of a [T][N] record beside s2d_gae and s2d_replay_push, ENGINE-INDEPENDENT like them: no handle, raw device
 * pointers, any stream of the current device; everything is read WHEN THE KERNELS RUN, so it can be captured behind a rollout
 * launch as a linear chain on one stream.  An episode usually spans several records: the caller owns each env's running
 * return and length (acc_return / acc_length [N], zero at start) and hands them to every call.  Finished episodes go to a
 * caller-owned ring of `capacity` episodes, 1 <= capacity < 2^31 (the five arrays [capacity]; step 8-byte aligned), exact
 * counts to `totals` = device uint64[8], 8-byte aligned, zero at start:
 *   {episodes, vector steps, episodes by result 0 (unlabelled) / 1 / 2 / 3, sum of episode lengths, episodes not kept}.
 * With e0 = totals[0] and s0 = totals[1] before the call, for every env i, t ascending:
 *   R = acc_return[i] + (reward ? reward[t][i] : +0.0f);                one fp32 add, in this order
 *   L = acc_length[i] + 1;
 *   if (done[t][i]) { emit(R, L, r = result ? result[t][i] : 0, i, s0 + t); acc_return[i] = +0.0f; acc_length[i] = 0; }
 *   else            { acc_return[i] = R; acc_length[i] = L; }
 * (result is read only where done is set).  The emitted episode's rank k is the number of set done[t'][i'] with (t', i')
 * lexicographically before (t, i): row-major order, the order a per-step loop over the envs meets them.  With n = the number
 * of set done bytes of the record and C = capacity, the episode of rank k is written to slot (e0 + k) mod C of all five
 * arrays if and only if k >= n - C; earlier episodes of the call are not written at all, so a slot has at most one writer.
 * A one-thread kernel queued behind the others then sets totals[0] = e0 + n, totals[1] = s0 + T,
 * totals[2 + (r <= 3 ? r : 0)] += 1 per episode, totals[6] += the sum of L, totals[7] += max(0, n - C); no wave of the call sees
 * the new values.  Slots the call does not own and the inputs are untouched; the workspace belongs to one call at a time and
 * holds nothing between calls.  There is no float atomic and no sum by arrival order: every output is the same bits whatever
 * the launch geometry.  S2D_EINVAL without a launch: n_steps < 1, n_envs outside [1, 2^31 - 1], T * N >= 2^40, capacity outside
 * [1, 2^31 - 1], a NULL pointer other than reward / result, totals or step not 8-byte aligned (4 bytes for the 4-byte arrays),
 * workspace_bytes below s2d_episode_stats_workspace(n_steps, n_envs). */
typedef struct S2DEpisodeRing {
  float *ret;
  int32_t *length;
  uint8_t *result;
  int32_t *env;
  int64_t *step;
  int64_t capacity;
} S2DEpisodeRing;
/* bytes of workspace of a shape; 0 for a shape the call rejects.  Host only, needs no GPU. */
size_t s2d_episode_stats_workspace(int n_steps, int64_t n_envs);
int s2d_episode_stats(int n_steps, int64_t n_envs, const float *reward /* [T][N] or NULL */, const uint8_t *done /* [T][N] */,
                      const uint8_t *result /* [T][N] or NULL */, float *acc_return /* [N] */, int32_t *acc_length /* [N] */,
                      const S2DEpisodeRing *ring, uint64_t *totals /* [8] */, void *workspace, size_t workspace_bytes, void *stream);

/* ---- TD targets from the target networks (s2d_td.hip) ----
 * What follows a sampled batch in every off-policy learner and needs no gradient: reward + discount * bootstrap(next_obs), in
 * one launch.  Engine-independent like s2d_gae and s2d_replay_*: no handle, raw device pointers, any stream of the current
 * device; everything is read WHEN THE KERNELS RUN, so sample -> target can be captured as a linear chain on one stream.
 *
 * The network is S2DWideNet's MLP with a run-time input width: n_in -> h_1 -> ... -> h_L -> n_out, every unit
 *   acc = b[j]; for k ascending: acc = fmaf(W[j][k], in[k], acc)
 * layer 1 over k = 0 .. 4 ceil(n_in / 4) - 1 with x_k = 0 against zero weights past n_in (n_in = 10: the reach-ball actors' 12
 * terms; n_in = 4: the GoToCenter actors' single k-step), later layers over exactly h_(l-1) terms; relu (v > 0 ? v : +0), tanh_spec or
 * sigmoid_spec between the layers and a linear output layer: at n_in = 10 the same function of the parameters, bit for bit, that
 * s2d_rollout_qnet_wide / s2d_rollout_actor_wide act on.  A call first rewrites every network's params in fragment order into its
 * workspace (a pack kernel on the caller's stream), so a captured graph computes with whatever the parameter buffers hold at
 * replay.  A workspace belongs to one call at a time, and every network of a call needs its own.  The result does not depend on
 * the launch plan (S2D_TD_PLAN=waves,tiles in the environment, read at every launch, overrides it for testing). */
typedef struct S2DTdNet {
  int32_t n_in;            /* 1 .. 256 */
  int32_t n_hidden;        /* 1 .. 5 */
  int32_t hidden[5];       /* multiples of 4 in [8, 400]; 0 past n_hidden */
  int32_t n_out;           /* 1 .. 64 */
  int32_t activation;      /* 0 relu, 1 tanh_spec, 2 sigmoid_spec */
  const float *params;     /* nn.Sequential order, contiguous, 16-byte aligned */
  void *workspace;         /* 256-byte aligned, >= s2d_td_workspace_bytes() */
  size_t workspace_bytes;
} S2DTdNet;
/* bytes of workspace of a shape (the pointers are not read); 0 for a shape off the grid.  Host only, needs no GPU. */
size_t s2d_td_workspace_bytes(const S2DTdNet *shape);
/* DQN and Double DQN.  Per row b: y = target(next_obs[b]); a* = argmax(y) by the actors' scan (best = 0; for a = 1 .. A-1:
 * if (y[a] > y[best]) best = a -- lowest index on ties, a NaN never replaces the best, an all-NaN row gives 0); with online !=
 * NULL a* is that argmax of online(next_obs[b]) instead (same n_in and n_out; hidden shape and activation may differ).
 * q = y[a*]; out_target[b] = reward[b] + (discount[b] * q): one fp32 multiply, then one fp32 add, never contracted -- what eager
 * torch's r + d * q computes.  There are NO special cases: discount = 0 with q = +-inf gives NaN, as in torch.  out_q[b] <- q and
 * out_index[b] <- a* where given.  Enqueues the pack kernel(s) and one target kernel.  S2D_EINVAL without a launch: a NULL,
 * misaligned or too small workspace, a shape off the grid, NULL or misaligned params (16 bytes), online's n_in / n_out differing
 * from target's, batch outside [1, 2^31 - 1], NULL or misaligned (4 bytes) next_obs / reward / discount / out_target, misaligned
 * optional outputs, the two networks sharing a workspace. */
int s2d_td_target_q(int64_t batch, const S2DTdNet *target, const S2DTdNet *online /* NULL: plain DQN */,
                    const float *next_obs /* [B][n_in] */, const float *reward, const float *discount,
                    float *out_target /* [B] */, float *out_q /* [B] or NULL */, int32_t *out_index /* [B] or NULL */, void *stream);
/* DDPG, and TD3's clipped double-Q (with smoothing noise: s2d_td_target_td3).  Per row b, with D = actor->n_in and A = actor->n_out
 * in [1, 8]: a'[i] = tanh_spec(actor(next_obs[b])[i]) (the tanh actor's head without noise and without epsilon); the critics' input
 * row is [next_obs[b] (D words) | a' (A words)], so critic->n_in == D + A and critic->n_out == 1; q = critic1(row)[0], with critic2
 * q = q2 < q1 ? q2 : q1 (a NaN in q2 never replaces q1); out_target[b] as above; out_q[b] <- q, out_action[b][i] <- a'[i] where
 * given.  All networks run on one row tile in one kernel: the critics' input never passes through memory.  S2D_EINVAL without a
 * launch as above, plus: actor->n_out outside [1, 8], a critic whose n_in is not D + A or whose n_out is not 1. */
int s2d_td_target_ac(int64_t batch, const S2DTdNet *actor, const S2DTdNet *critic1, const S2DTdNet *critic2 /* or NULL */,
                     const float *next_obs /* [B][actor->n_in] */, const float *reward, const float *discount, float *out_target,
                     float *out_q /* or NULL */, float *out_action /* [B][A] or NULL */, void *stream);
#define S2D_TD3_STREAM 15 /* Philox stream id of the TD3 target's smoothing noise (no other draw uses it) */
/* TD3's target: the call above with target-policy smoothing, SB3's (actor_target(next_obs) + noise.clamp(-c, c)).clamp(-1, 1).  Per
 * row b, with D = actor->n_in and A = actor->n_out in [1, 8]: y = actor(next_obs[b]), m_i = tanh_spec(y_i) (s2d_td_target_ac's
 * action); z_0 .. z_7 from Philox4x32-10 with key `seed` at counter {b, draws_lo, draws_hi, (S2D_TD3_STREAM << 16) | blk}: blk = 0
 * gives z0..z3, blk = 1 (drawn only if A > 4) z4..z7, words x, y -> (z0, z1) and z, w -> (z2, z3) through the engine's Box-Muller, as
 * in the SAC target below.  With sigma = noise[0] (target_policy_noise) and clip = noise[1] (target_noise_clip):
 *   n_i  = sigma * z_i                                    one fp32 multiply
 *   n_i  = n_i < -clip ? -clip : (n_i > clip ? clip : n_i)
 *   s_i  = m_i + n_i                                      one fp32 add, never contracted with the multiply
 *   a'_i = s_i < -1 ? -1 : (s_i > 1 ? 1 : s_i)
 * so a NaN passes through both clamps, as in torch.clamp.  The critics' row is [next_obs[b] | a']; q = q1, with critic2
 * q2 < q1 ? q2 : q1; out_target[b] = reward[b] + (discount[b] * q) as above; out_q[b] <- q, out_action[b][i] <- a'_i (the smoothed,
 * clamped action) where given.  noise[0], noise[1] and *draws are device words read when the kernel runs; a one-thread kernel on
 * the same stream then sets *draws += 1, so every call and every replay of a captured graph draws fresh noise and sample -> target
 * stays one capturable linear chain.  The counter is keyed by the global row: the result does not depend on S2D_TD_PLAN.
 * sigma = 0: n_i = +-0, so out_target and out_q have s2d_td_target_ac's bits wherever no action word is -0; an action of -0 may come
 * out as +0 (-0 + +0 = +0).  S2D_EINVAL without a launch as for s2d_td_target_ac, plus: NULL or misaligned noise (4 bytes) or draws
 * (8 bytes), draws or noise overlapping an output. */
int s2d_td_target_td3(int64_t batch, const S2DTdNet *actor, const S2DTdNet *critic1, const S2DTdNet *critic2 /* or NULL */,
                      const float *next_obs, const float *reward, const float *discount,
                      const float *noise /* device float[2]: sigma (target_policy_noise), clip (target_noise_clip) */,
                      uint64_t *draws, uint64_t seed,
                      float *out_target, float *out_q /* or NULL */, float *out_action /* [B][A] or NULL */, void *stream);
#define S2D_TD_STREAM 13 /* Philox stream id of the SAC target's action noise (no other draw uses it) */
/* Soft Actor-Critic's entropy-regularised target.  Per row b, with D = actor->n_in and A = actor->n_out / 2 in [1, 8]:
 * y = actor(next_obs[b]) -- the ONLINE actor, as in SB3 --, rows 0 .. A-1 the means, A .. 2A-1 the raw log-std; the head of the SAC
 * rollout above (ls_j, sigma_j, u_j, a_j, t_j, logp: the same function) with z from Philox4x32-10 with key `seed` at counter
 * {b, draws_lo, draws_hi, (S2D_TD_STREAM << 16) | m}: m = 0 gives z0..z3, m = 1 (drawn only if A > 4) z4..z7, words x, y -> (z0, z1)
 * and z, w -> (z2, z3) through the engine's Box-Muller.  The critics' row is [next_obs[b] | a']; q = q1, or with critic2
 * q2 < q1 ? q2 : q1 as above; v = q - (alpha * logp): one multiply, then one subtract, never contracted; out_target[b] =
 * reward[b] + (discount[b] * v).  out_q[b] <- q, out_action[b][j] <- a'_j, out_logp[b] <- logp where given.  *alpha (ent_coef) and
 * *draws are device words read when the kernel runs; a one-thread kernel on the same stream then sets *draws += 1, so a replayed
 * graph draws fresh noise and sample -> target stays one capturable linear chain.  The result does not depend on S2D_TD_PLAN.
 * S2D_EINVAL without a launch as for the DDPG target, plus: actor->n_out odd or outside [2, 16], a critic whose n_in is not
 * D + A, NULL or misaligned alpha (4 bytes) or draws (8 bytes), draws overlapping an output. */
int s2d_td_target_sac(int64_t batch, const S2DTdNet *actor /* n_out = 2A */, const S2DTdNet *critic1, const S2DTdNet *critic2 /* or NULL */,
                      const float *next_obs, const float *reward, const float *discount, const float *alpha, uint64_t *draws,
                      uint64_t seed, float *out_target, float *out_q /* or NULL */, float *out_action /* [B][A] or NULL */,
                      float *out_logp /* [B] or NULL */, void *stream);
/* diagnostic: the SAC target with a `deterministic` switch, so that its head can be compared with the rollout's greedy action.
 * deterministic = 0: the call above, bit for bit.  Non-zero: z_j = 0 and u_j = y_j, no Philox draw (the rollout's deterministic
 * word); *draws is still advanced. */
int s2d_debug_td_target_sac(int64_t batch, const S2DTdNet *actor, const S2DTdNet *critic1, const S2DTdNet *critic2, const float *next_obs,
                            const float *reward, const float *discount, const float *alpha, uint64_t *draws, uint64_t seed,
                            int deterministic, float *out_target, float *out_q, float *out_action, float *out_logp, void *stream);
/* ---- the Q-learner's gradient step (s2d_learn.hip) ----
 * What follows the TD target in DQN, Double DQN, n-step and PER: ONE gradient step of the online Q-network on a sampled batch --
 * forward, TD error, MSE / Huber derivative, backward, gradient-norm clip and Adam -- as a linear chain of three launches on one
 * stream.  Engine-independent like s2d_td_*: no handle, raw device pointers, any stream of the current device; the parameters, the
 * hyper-parameters and the step state are all read WHEN THE KERNELS RUN (there is no host step counter), so sample -> target ->
 * step can be captured and replayed, and a scheduler writes hyper[0] (lr) between replays.
 *
 * The network is S2DTdNet's MLP on the learner's grid: n_in 1 .. 256, 1 .. 4 hidden layers of multiples of 8 in [8, 256], n_out
 * 1 .. 64.  The forward pass is the same fp32 chain (acc = b[j]; k ascending: acc = fmaf(W[j][k], in[k], acc); layer 1 over
 * 4 ceil(n_in / 4) terms), so q[b][a] has the bits s2d_td_target_q and the wide actors compute from the same parameters.
 * Per row b: a = action[b]; e = q[b][a] - target[b]; out_td_abs[b] = |e|; d = e (MSE, loss e^2 / 2) or e < -1 ? -1 : e > 1 ? 1 : e
 * (Huber with delta 1, loss |e| <= 1 ? e^2 / 2 : |e| - 1/2: torch's smooth_l1_loss); the output delta is (weight[b] * d) / (float)B
 * in column a and +0 elsewhere (weight NULL: 1).  An action outside [0, n_out) is never used as an index: its row has e = 0, a
 * zero delta and no loss, and *error |= 1.  A NaN target propagates (there are no special cases).
 * Backward: the delta of unit k of the layer below is s = +0; j ascending: s = fmaf(W[j][k], delta[j], s), times the activation's
 * derivative from its stored output y, separate operations: relu y > 0 ? s : +0; tanh s * (1 - y * y); sigmoid s * (y * (1 - y)).
 * Parameter gradients: rows are cut into blocks of S2D_LEARN_BLOCK_ROWS; within a block dW[j][k] = +0; rows ascending:
 * fmaf(delta[row][j], in[row][k], .), db[j] the same with in = 1; the blocks' partials are added in ascending block order (the first
 * block starts the sum).  No float atomics: the gradient is a function of the inputs alone, not of the grid or the device.
 * Norm: per chunk of S2D_LEARN_NORM_CHUNK words of the flat gradient s = +0; ascending: s = fmaf(g, g, s); chunks added ascending;
 * norm = sqrt (correctly rounded); scale = max_grad_norm > 0 ? min(1, max_grad_norm / (norm + 1e-6f)) : 1 (clip_grad_norm_).
 * stats <- {mean loss (block partials, rows ascending, blocks ascending, / (float)B), norm, scale}; grad <- the UNCLIPPED sum.
 * Adam (no amsgrad, no weight decay), every step one fp32 operation: beta1^t *= beta1, beta2^t *= beta2 (device words, once per
 * call); g' = g * scale; m += (g' - m) * (1 - beta1); v = v * beta2 + ((1 - beta2) * g') * g';
 * p -= (lr / (1 - beta1^t)) * (m / (sqrt(v) / sqrt(1 - beta2^t) + eps)).  A fresh state has m = v = 0 and both products 1. */
#define S2D_LEARN_BLOCK_ROWS 64
#define S2D_LEARN_NORM_CHUNK 256
enum { S2D_LEARN_MSE = 0, S2D_LEARN_HUBER = 1, S2D_LEARN_SQUARE = 2 /* s2d_learn_critic only */ };
typedef struct S2DLearnNet {
  int32_t n_in;            /* 1 .. 256 */
  int32_t n_hidden;        /* 1 .. 4 */
  int32_t hidden[5];       /* multiples of 8 in [8, 256]; 0 past n_hidden */
  int32_t n_out;           /* 1 .. 64 */
  int32_t activation;      /* 0 relu, 1 tanh_spec, 2 sigmoid_spec */
  float *params;           /* READ-WRITE, nn.Sequential order, contiguous, 16-byte aligned */
  void *workspace;         /* 256-byte aligned, >= s2d_learn_workspace_bytes(shape, batch) */
  size_t workspace_bytes;
} S2DLearnNet;
typedef struct S2DLearnState {
  float *m, *v, *grad;     /* [P] each, 16-byte aligned (m and v are not read by s2d_learn_q_grad) */
  float *hyper;            /* [7]: lr, beta1, beta2, eps, max_grad_norm, beta1^t, beta2^t */
  float *stats;            /* [3]: mean loss, gradient norm, clip scale */
  int32_t *error;          /* |= 1: an action outside [0, n_out) */
  int32_t loss_kind;       /* S2D_LEARN_MSE | S2D_LEARN_HUBER (| S2D_LEARN_SQUARE for s2d_learn_critic; s2d_learn_actor ignores it) */
} S2DLearnState;
/* bytes of workspace of a shape for batches up to max_batch (the pointers are not read): the blocks' partial gradients, the
 * chunk and loss partials and, where 64 rows of activations do not fit the LDS, the blocks' activations.  0 for a shape off the
 * grid or max_batch outside [1, 2^31 - 1].  Host only, needs no GPU. */
size_t s2d_learn_workspace_bytes(const S2DLearnNet *shape, int64_t max_batch);
/* One step.  out_td_abs [B] and out_q [B][n_out] (the forward values) may be NULL.  S2D_EINVAL without a launch and with nothing
 * written, the text naming the field: a shape off the grid, an unknown loss_kind, batch outside [1, 2^31 - 1] or above what the
 * workspace holds, NULL or misaligned params / workspace / m / v / grad / hyper / stats / error / obs / action / target, misaligned
 * optional arrays, params, m, v, grad or the workspace overlapping one another. */
int s2d_learn_q(int64_t batch, const S2DLearnNet *net, const S2DLearnState *state, const float *obs /* [B][n_in] */,
                const int32_t *action /* [B] */, const float *target /* [B] */, const float *weight /* [B] or NULL */,
                float *out_td_abs, float *out_q, void *stream);
/* The same up to and including grad, stats, out_td_abs and out_q, WITHOUT touching params, m, v or the beta products: for tests
 * and for callers with their own optimiser. */
int s2d_learn_q_grad(int64_t batch, const S2DLearnNet *net, const S2DLearnState *state, const float *obs, const int32_t *action,
                     const float *target, const float *weight, float *out_td_abs, float *out_q, void *stream);
/* ---- the DDPG / TD3 update (s2d_learn.hip): the critic's step and the actor's step through the critic ----
 * Engine-independent like s2d_learn_q: no handle, raw device pointers, any stream of the current device, everything read WHEN THE
 * KERNELS RUN, each call a linear chain of three launches on one stream (capturable), no float atomics, no result depends on the
 * grid.  All networks are on the learner's grid above; further D = obs width in 1 .. 248, A = action width in 1 .. 8 (D + A <= 256),
 * a critic has n_in == D + A and n_out == 1; actor and critic may differ in hidden shape and activation.
 *
 * s2d_learn_critic: one step of a critic.  The input row [obs[b] (D = net->n_in - action_dim words) | action[b] (action_dim float
 * words)], zero-padded to 4 ceil((D + A) / 4), is assembled in the kernel and never passes through memory.  Everything after that is
 * s2d_learn_q's spec with output column 0: e = q[b] - target[b]; out_td_abs[b] = |e|; the delta (weight[b] * d) / (float)B;
 * backward, block partials, norm, clip, Adam; out_q is [B].  One more loss kind: S2D_LEARN_SQUARE, loss e * e and d = 2.0f * e
 * (F.mse_loss); s2d_learn_q keeps rejecting it.  The error word is required as for s2d_learn_q and never set.  Workspace:
 * s2d_learn_workspace_bytes of the critic's shape.  TD3's second critic is a second call with a state of its own (Adam is
 * element-wise, so two states equal one optimiser over both critics as long as nothing clips across them).  S2D_EINVAL without a
 * launch and with nothing written: all that s2d_learn_q rejects, plus action_dim outside [1, 8], n_out != 1, n_in - action_dim
 * outside [1, 248], loss_kind outside 0 .. 2. */
int s2d_learn_critic(int64_t batch, const S2DLearnNet *net, const S2DLearnState *state, const float *obs /* [B][D] */,
                     int32_t action_dim, const float *action /* [B][action_dim] */, const float *target /* [B] */,
                     const float *weight /* [B] or NULL */, float *out_td_abs /* [B] or NULL */, float *out_q /* [B] or NULL */,
                     void *stream);
/* the same WITHOUT touching params, m, v or the beta products */
int s2d_learn_critic_grad(int64_t batch, const S2DLearnNet *net, const S2DLearnState *state, const float *obs, int32_t action_dim,
                          const float *action, const float *target, const float *weight, float *out_td_abs, float *out_q,
                          void *stream);
/* s2d_learn_actor: one step of the actor on loss = -mean_b Q(obs[b], tanh(mu(obs[b]))).  actor holds the linear layers of mu
 * (n_in = D, n_out = A in 1 .. 8); the tanh head is part of the call, as in s2d_td_target_ac.  Of critic only shape and params are
 * read (params READ-ONLY; workspace fields ignored).  actor_state->loss_kind is ignored and its error word is neither required nor
 * written (there is no index to be wrong).  Per row b:
 *   forward, actor   a[i] = tanh_spec(actor(obs[b])[i])
 *   forward, critic  q = critic([obs[b] | a])[0]; both by the chain acc = b[j]; k ascending: acc = fmaf(W[j][k], in[k], acc) (layer 1
 *                    over its padded terms), so out_action [B][A] and out_q [B] have the bits s2d_td_target_ac writes for the same
 *                    parameters with next_obs = obs
 *   critic's output delta   -1.0f / (float)B
 *   critic backward  the delta spec above (s = +0; j ascending: s = fmaf(W[j][k], delta[j], s), then the activation's derivative from
 *                    the stored output) down to the input layer, where only the A action columns k = D .. D + A - 1 are formed:
 *                    s[i] = +0; j ascending over h_1: s[i] = fmaf(W_1[j][D + i], delta_1[j], s[i]).  No critic dW or db is computed or
 *                    written.
 *   tanh head        dz[i] = s[i] * (1.0f - a[i] * a[i]), separate operations
 *   actor backward   s2d_learn_q's spec with output delta dz: block partials of S2D_LEARN_BLOCK_ROWS rows, rows ascending, blocks added
 *                    ascending; the same norm, clip and Adam on the actor's state
 * stats <- {-(sum of q: rows ascending per block, blocks ascending) / (float)B, norm, scale}; grad <- the UNCLIPPED sum.  The block's
 * image holds both networks' rows (in LDS where 64 rows fit 160 KiB, else in the actor's workspace).  S2D_EINVAL without a launch and
 * with nothing written, the text naming the field: a shape off the grid, A outside [1, 8], D above 248, a critic whose n_in != D + A
 * or n_out != 1, batch outside [1, 2^31 - 1] or above what the workspace holds, NULL or misaligned actor params / workspace / m / v /
 * grad / hyper / stats / obs or critic params, misaligned optional outputs, the actor's params, m, v, grad or workspace overlapping
 * one another or the critic's params. */
int s2d_learn_actor(int64_t batch, const S2DLearnNet *actor, const S2DLearnState *actor_state,
                    const S2DLearnNet *critic /* params only read */, const float *obs /* [B][D] */,
                    float *out_action /* [B][A] or NULL */, float *out_q /* [B] or NULL */, void *stream);
/* the same WITHOUT touching the actor's params, m, v or beta products */
int s2d_learn_actor_grad(int64_t batch, const S2DLearnNet *actor, const S2DLearnState *actor_state, const S2DLearnNet *critic,
                         const float *obs, float *out_action, float *out_q, void *stream);
/* bytes of the ACTOR's workspace for s2d_learn_actor with this pair of shapes (the pointers are not read) and batches up to
 * max_batch: s2d_learn_workspace_bytes' parts for the actor's parameters and, where 64 rows of both networks do not fit the LDS,
 * the blocks' images.  0 for a pair off the grid or max_batch outside [1, 2^31 - 1].  Host only, needs no GPU. */
size_t s2d_learn_actor_workspace_bytes(const S2DLearnNet *actor_shape, const S2DLearnNet *critic_shape, int64_t max_batch);
/* ---- the PPO update (s2d_learn.hip): clipped surrogate, value loss, entropy bonus, one clip and one Adam over both networks ----
 * Engine-independent like s2d_learn_q: no handle, raw device pointers, any stream of the current device, everything read WHEN THE
 * KERNELS RUN, a linear chain of launches on one stream (pre-pass if normalising, block kernel, reduce, finish; capturable), no float
 * atomics, no result depends on the grid or the device.  tests/learn_ppo_ref.c restates every operation below.
 *
 * Networks: pi D -> h... -> A and vf D -> h... -> 1, both on the learner's grid above (shapes and activations may differ, D is
 * shared).  head 0: categorical, A in 1 .. 64, action int32 [R].  head 1: diagonal Gaussian, A in 1 .. 8, action float [R][A] (the
 * unclipped action s2d_rollout_policy records) and a parameter log_std[A].  ONE flat buffer params = [pi | vf | log_std] (log_std
 * with head 1 only) of P words, with one m, v, grad, one norm and one clip over all of it.
 * Rows: the rollout arrays have R rows; row b of the minibatch (b < B) is row index[b], or row b where index is NULL (then B <= R);
 * the gather happens in the kernel.  An index outside [0, R) is never used: its row is DROPPED -- zero input, zero output deltas, no
 * loss, no share in any statistic, out_logp = out_value = +0 -- the divisor stays B, and *error |= 2.  A categorical action outside
 * [0, A) drops its row in the same way (but its advantage takes part in the normalisation) and *error |= 1.
 * hyper[10]: the seven words of S2DLearnState, then clip_range c, vf_coef, ent_coef.
 * Advantage normalisation (normalize_advantage != 0 and B > 1; a launch of its own), over the rows that are not dropped for their
 * index: per block of 64 rows s = +0, rows ascending s = s + adv; blocks added ascending (the first starts the sum); mean = S / (float)B;
 * the same with d = adv - mean, s = fmaf(d, d, s); std = sqrt(S2 / (float)(B - 1)); A^ = (adv - mean) / (std + 1e-8f).  Else A^ = adv.
 * (The order is serial: the pre-pass is ONE workgroup and one lane adds the B / 64 block sums, twice: O(B / 64) on a single lane, so a
 * normalised minibatch near the largest B is slow.)
 * Per row, every step one fp32 operation, y = pi's outputs and v = vf's by s2d_learn_q's forward chain (layer 1 over 4 ceil(D / 4)
 * terms: the bits s2d_rollout_policy acts on):
 *   categorical  m = the first maximum of y; S = exp_spec(y_0 - m), j ascending: S += exp_spec(y_j - m); logS = log_spec(S);
 *                logp = (y_a - m) - logS (categorical_head's); p_j = exp_spec(y_j - m) / S; lp_j = (y_j - m) - logS;
 *                h = +0, j ascending: h = fmaf(p_j, lp_j, h); H = -h
 *   Gaussian     z_j = (a_j - y_j) / exp_spec(log_std_j); term_j = fmaf(-0.5f * z_j, z_j, -log_std_j) - 0.91893853f; logp = term_0 + term_1
 *                + ... ascending; H = (log_std_0 + log_std_1 + ...) + (float)A * 1.4189385f
 *   surrogate    d = logp - logp_old; r = exp_spec(d); rc = r < 1 - c ? 1 - c : r > 1 + c ? 1 + c : r; s1 = r * A^; s2 = rc * A^;
 *                policy loss -min(s1, s2) (a NaN wins); g = +0 where (r > 1 + c and A^ > 0) or (r < 1 - c and A^ < 0), else -s1
 *   value        e = v - ret; loss e * e; delta (vf_coef * (2.0f * e)) / (float)B
 *   deltas       categorical: (g * (1[j = a] - p_j) + (ent_coef * p_j) * (lp_j + H)) / (float)B;  Gaussian means: ((g * z_j) / sigma_j) /
 *                (float)B, and the row's log_std term (g * (z_j * z_j - 1.0f)) / (float)B, summed over rows like a bias gradient;
 *                grad[log_std_j] = that sum - ent_coef
 *   statistics   policy loss, value loss, H, (r - 1.0f) - d, |r - 1.0f| > c ? 1 : 0
 * Backward and parameter gradients are s2d_learn_q's per network, except for the order of the row sums: consecutive blocks of 64 rows
 * are grouped G = ceil(blocks / S2D_LEARN_PPO_MAX_GROUPS) at a time; every dW / db / log_std chain and every statistic starts at +0 at
 * the group's first row and runs over the group's rows ascending; the groups' partials are added in ascending group order (the first
 * starts the sum).  G depends on B alone; for B <= 16 384 a group is a block.  Norm, clip scale and Adam are s2d_learn_q's over all
 * P words.  stats[8] <- {loss = (pg + vf_coef * vl) - ent_coef * ent, norm, scale, pg, vl, ent, approx_kl, clip_fraction}, the last five
 * the statistics' sums / (float)B.  NaN and inf propagate.  Not included: value clipping, a shared trunk, a target-KL stop. */
#define S2D_LEARN_PPO_MAX_GROUPS 256
enum { S2D_LEARN_PPO_CATEGORICAL = 0, S2D_LEARN_PPO_GAUSSIAN = 1 };
typedef struct S2DLearnPPO {
  S2DLearnNet pi, vf;      /* the shapes; their params / workspace fields are ignored */
  int32_t head;            /* S2D_LEARN_PPO_CATEGORICAL | S2D_LEARN_PPO_GAUSSIAN */
  int32_t normalize_advantage;
  float *params;           /* READ-WRITE [P] = [pi | vf | log_std], 16-byte aligned */
  float *m, *v, *grad;     /* [P] each, 16-byte aligned (m and v are not read by s2d_learn_ppo_grad) */
  float *hyper;            /* [10]: lr, beta1, beta2, eps, max_grad_norm, beta1^t, beta2^t, clip_range, vf_coef, ent_coef */
  float *stats;            /* [8] */
  int32_t *error;          /* |= 1: a categorical action outside [0, A); |= 2: an index outside [0, R) */
  void *workspace;         /* 256-byte aligned, >= s2d_learn_ppo_workspace_bytes(pi, vf, head, batch) */
  size_t workspace_bytes;
} S2DLearnPPO;
typedef struct S2DLearnPPOBatch {
  int64_t rows;            /* R: rows of the rollout arrays */
  int64_t batch;           /* B: rows of the minibatch */
  const float *obs;        /* [R][D] */
  const void *action;      /* int32 [R] or float [R][A] */
  const float *logp_old, *advantage, *ret;   /* [R] each */
  const int32_t *index;    /* [B] or NULL */
  float *out_logp, *out_value;               /* [B] each, or NULL */
} S2DLearnPPOBatch;
/* bytes of workspace for batches up to max_batch (only the shapes are read): at most 256 groups' partial gradients and statistics,
 * the chunk sums, the pre-pass's block sums and, where 64 rows of both networks do not fit the LDS, the groups' images.  0 for a
 * pair or head off the grid or max_batch outside [1, 2^31 - 1].  Host only, needs no GPU. */
size_t s2d_learn_ppo_workspace_bytes(const S2DLearnNet *pi_shape, const S2DLearnNet *vf_shape, int32_t head, int64_t max_batch);
/* One step.  S2D_EINVAL without a launch and with nothing written, the text naming the field: a shape or head off the grid, vf's n_in
 * != pi's or n_out != 1, rows or batch outside [1, 2^31 - 1], batch above rows without an index or above what the workspace holds,
 * NULL or misaligned params / workspace / m / v / grad / hyper / stats / error / obs / action / logp_old / advantage / ret, misaligned
 * optional arrays, params, m, v, grad or the workspace overlapping one another. */
int s2d_learn_ppo(const S2DLearnPPO *learner, const S2DLearnPPOBatch *batch, void *stream);
/* The same up to and including grad, stats, out_logp and out_value, WITHOUT touching params, m, v or the beta products. */
int s2d_learn_ppo_grad(const S2DLearnPPO *learner, const S2DLearnPPOBatch *batch, void *stream);
/* ---- the Soft Actor-Critic update (s2d_learn.hip): the actor's step through min(Q1, Q2) and the temperature's step ----
 * SAC's critic loss 0.5 * (mse(q1, t) + mse(q2, t)) is, per critic, s2d_learn_critic with S2D_LEARN_MSE (loss e^2 / 2, delta e / B),
 * called once per critic: there is no SAC critic call.  s2d_learn_sac_actor is one step of the squashed-Gaussian actor on
 * loss = mean_b (alpha * logp_b - min(Q1, Q2)(obs_b, a_b)), reparameterised, and (with alpha_state) one Adam step of log_alpha.
 * Engine-independent like s2d_learn_q: no handle, raw device pointers, any stream of the current device, everything read WHEN THE
 * KERNELS RUN; a linear chain of four launches on one stream (block kernel, reduce, finish, then ONE THREAD for the mean of logp,
 * the temperature and the draw counter; the _grad twin with a fixed coefficient has nothing for it to do and stops at three), capturable, no float atomics, no result depends on the grid.  tests/learn_sac_ref.c
 * restates every operation below.
 *
 * Networks, all on the learner's grid above: the actor D -> h... -> 2A (D in 1 .. 248, A in 1 .. 8: n_out even, in [2, 16]), each
 * critic (D + A) -> h... -> 1; the three may differ in hidden shape and activation; critic2 may be NULL.  Of the critics only shape
 * and params are read (READ-ONLY; workspace fields ignored): no critic dW or db is formed or written.  actor_state->loss_kind is
 * ignored, its error word neither required nor written.
 * Per row b (b the absolute row of the batch), every step one fp32 operation unless an fmaf is written:
 *   forward, actor   y = actor(obs[b]) by s2d_learn_q's forward chain; mean_j = y[j], v_j = y[A + j]
 *   head             the head of s2d_rollout_sac and s2d_td_target_sac, the same function, never deterministic: ls_j = v_j > 2 ? 2 :
 *                    (v_j >= -20 ? v_j : -20) (a NaN gives -20); sigma_j = exp_spec(ls_j); u_j = fmaf(sigma_j, z_j, mean_j);
 *                    a_j = tanh_spec(u_j); t_j = (fmaf(-0.5f * z_j, z_j, -ls_j) - 0.91893853f) - log_spec(fmaf(-a_j, a_j, 1.0f) + 1e-6f);
 *                    logp = t_0 (+ t_1 ... in ascending j).  z from Philox4x32-10 with key `seed` at counter
 *                    {b, draws_lo, draws_hi, (S2D_LEARN_SAC_STREAM << 16) | m}: m = 0 gives z0..z3, m = 1 (drawn only if A > 4) z4..z7,
 *                    words x, y -> (z0, z1) and z, w -> (z2, z3) through the engine's Box-Muller, as in s2d_td_target_sac
 *   forward, critics q_i = critic_i([obs[b] | a])[0]; q = q1, or with critic2 q2 < q1 ? q2 : q1 (a tie or a NaN q2 keeps critic 1)
 *   row loss         l_b = (alpha * logp) - q: one multiply, then one subtract, never contracted
 *   critic backward  only the CHOSEN critic's: output delta -1.0f / (float)B, s2d_learn_actor's delta chain down to the A action
 *                    columns of its input: s_j = +0; k ascending over h_1: s_j = fmaf(W_1[k][D + j], delta_1[k], s_j).  (The kernel runs
 *                    both critics' chains and takes the chosen one's words; the other's bits never reach a result.)
 *   head backward    w = alpha / (float)B; om = fmaf(-a_j, a_j, 1.0f); r = om / (om + 1e-6f); du = ((w * (2.0f * a_j)) * r) + (s_j * om);
 *                    dmean_j = du; dls = (du * (sigma_j * z_j)) - w; dv_j = (v_j >= -20.0f && v_j <= 2.0f) ? dls : +0 (torch's clamp,
 *                    inclusive at both bounds; a NaN v gives +0); a saturated a_j = +-1 has om = 0, so du = 0 and dls = -w
 *   actor backward   s2d_learn_q's spec with the 2A words [dmean | dv] as the output delta; the same block partials, norm, clip and Adam on
 *                    actor_state
 * actor_state->stats <- {(sum of l_b) / (float)B, norm, scale}; alpha_state->stats[0] <- (sum of logp_b) / (float)B; both sums per block
 * of S2D_LEARN_BLOCK_ROWS rows s = +0, rows ascending s = s + x, then the blocks' sums added ascending (the first block starts the sum).
 * Temperature (only with alpha_state): g = -(mean_logp + target_entropy); stats[1] = log_alpha * g (the pre-step log_alpha); its own
 * beta products hyper[5] *= hyper[1], hyper[6] *= hyper[2], once; s2d_learn_q's Adam formula on the one word with scale 1 and m = m_v[0],
 * v = m_v[1] (hyper[4] is ignored: one scalar is never clipped); *alpha = exp_spec(log_alpha_new), and stats[2] the same.  The actor's
 * rows read *alpha BEFORE any of this; the next target launch reads the new value.  alpha_state NULL: a fixed entropy coefficient,
 * *alpha is only read.
 * The step then sets *draws += 1 (after its rows have read it), so a replayed graph draws fresh noise.
 * out_action [B][A] <- a, out_logp [B] <- logp, out_q [B] <- q where given (all before the update).
 * S2D_EINVAL without a launch and with nothing written, the text naming the field: all that s2d_learn_actor rejects (for both critics),
 * plus the actor's n_out odd or outside [2, 16], NULL or misaligned alpha (4 bytes) or draws (8 bytes), NULL or misaligned members of a
 * non-NULL alpha_state, and alpha, draws or alpha_state's arrays overlapping one another, the actor's params, m, v, grad or workspace,
 * a critic's params or an output. */
#define S2D_LEARN_SAC_STREAM 14 /* Philox stream id of the SAC actor step's action noise (no other draw uses it) */
typedef struct S2DLearnSacAlpha {
  float *log_alpha;        /* [1] READ-WRITE */
  float *m_v;              /* [2] Adam's m and v of log_alpha */
  float *hyper;            /* [7] as S2DLearnState.hyper; word 4 (max_grad_norm) ignored */
  float *stats;            /* [3]: mean logp, alpha loss, alpha after the call */
  float target_entropy;    /* SB3: -A */
} S2DLearnSacAlpha;
int s2d_learn_sac_actor(int64_t batch, const S2DLearnNet *actor /* n_out = 2A */, const S2DLearnState *actor_state,
                        const S2DLearnNet *critic1 /* params only read */, const S2DLearnNet *critic2 /* the same, or NULL */,
                        const float *obs /* [B][D] */, float *alpha /* [1]; READ, and with alpha_state WRITTEN after the step */,
                        const S2DLearnSacAlpha *alpha_state /* or NULL */, uint64_t *draws, uint64_t seed,
                        float *out_action /* [B][A] or NULL */, float *out_logp /* [B] or NULL */, float *out_q /* [B] or NULL */,
                        void *stream);
/* The same up to and including the actor's grad and stats, alpha_state->stats[0..1] and the optional outputs, WITHOUT touching the
 * actor's params, m, v or beta products, log_alpha, m_v, the temperature's beta products, alpha_state->stats[2], *alpha or *draws: two
 * calls in a row see the same noise. */
int s2d_learn_sac_actor_grad(int64_t batch, const S2DLearnNet *actor, const S2DLearnState *actor_state, const S2DLearnNet *critic1,
                             const S2DLearnNet *critic2, const float *obs, float *alpha, const S2DLearnSacAlpha *alpha_state,
                             uint64_t *draws, uint64_t seed, float *out_action, float *out_logp, float *out_q, void *stream);
/* bytes of the ACTOR's workspace for s2d_learn_sac_actor with these shapes (the pointers are not read; critic2_shape may be NULL) and
 * batches up to max_batch: s2d_learn_actor_workspace_bytes' parts, a second row of block partials (the rows' logp) and, where 64 rows of
 * all the networks and the head's words do not fit the LDS, the blocks' images.  0 for shapes off the grid or max_batch outside
 * [1, 2^31 - 1].  Host only, needs no GPU. */
size_t s2d_learn_sac_workspace_bytes(const S2DLearnNet *actor_shape, const S2DLearnNet *critic1_shape,
                                     const S2DLearnNet *critic2_shape /* or NULL */, int64_t max_batch);
/* fill derived protobuf-mirroring fields from the current state */
int s2d_world_model(S2DHandle h, const S2DWorldModel *out, void *stream);
/* zero the statistics counters */
int s2d_stats_reset(S2DHandle h, void *stream);
/* name of the most recently launched kernel variant (for profiling reports) */
const char *s2d_kernel_name(S2DHandle h);
/* debug guard (the reference's desync recovery, soccer_2d_env.py:154-159, 257-260, has no counterpart in a
 * lockstep engine; what remains to watch is a state word leaving its domain).  counts_dev[8] (device memory) receives the
 * number of envs with: [0] a non-finite state word, [1] |body| or |prev_angle| > 180, [2] stamina outside [0, stamina_max] or a
 * negative capacity, [3] effort / recovery outside their ServerParam ranges, [4] a negative step / episode counter or
 * distance carry, [5] a non-finite observation; [6..7] reserved.  All zero for every state the engine produces. */
int s2d_validate_state(S2DHandle h, uint32_t *counts_dev, void *stream);
/* new Philox key for all later draws (gym's env.seed(); the reference's `random` / `np.random` are unseeded).  Takes
 * effect at the next launch on `stream`; stream-ordered like every other call (abi 3: the episodes s2d_step keeps prepared
 * are dropped by a hipMemsetAsync on `stream`, behind whatever is already queued there); callers normally follow it with
 * s2d_reset on the same stream. */
int s2d_set_seed(S2DHandle h, uint64_t seed, void *stream);
/* diagnostic: evaluate one primitive of the fp32 math spec / Philox on the device so that
 * tests can compare it bit for bit with the CPU oracle.  op: 0 sincos_deg (in[n] -> out[n][2]),
 * 1 atan2_deg (in[n][2]=y,x -> out[n]), 2 exp, 3 norm_deg, 4 philox4x32-10 (in = uint32[n][6]
 * ctr+key -> out = uint32[n][4]), 5 hypot (in[n][2] -> out[n]).
 * The three hooks of ReachBallEnv, evaluated stand-alone so that the device code can be checked against the
 * golden vectors produced by the reference's own Python (tests/golden):
 * 6 state_to_observation (reach_ball_env.py:87-111): in[n][9] = bx,by,bvx,bvy,px,py,body,1/half_length,1/half_width
 *   -> out[n][10];
 * 7 action_to_rpc_actions (:53-85): in[n][8] = a0,a1,a2,a3,u,mode(0 discrete,1 continuous,2 turning),360/n,0
 *   -> out[n][3] = S2D_CMD_*, power, relative direction;
 * 8 check_trainer_observation (:113-161): in[n][12] = bx,by,px,py,body,step_number,prev_dist,prev_angle,
 *   min_distance_to_ball,max_steps,half_length,half_width -> out[n][5] = done,reward,S2D_RESULT_*,dist,angle. */
/* 9 reset_sample_coop against reset_sample (in = uint32[n][4], n a multiple of 256; out[n][14]);
 * 10 the movement-noise draw of one commanded cycle (one Philox word per object and cycle -- magnitude uniform
 *   k / 65536 from its high half, direction a WHOLE degree from its low half): in = uint32[n][4] = global env id lo, hi, policy step k,
 *   seed (low word) -> out[n][6] = player magnitude uniform, sin, cos; ball magnitude uniform, sin, cos.
 * 11 the S2D_NOISE_RCSSSERVER draw of one commanded cycle (Philox block 2 of stream 3 at counter k; each word w ->
 *   (w >> 8) * 2^-24 * 2 - 1, in [-1, 1)): in = uint32[n][4] = global env id lo, hi, counter k, seed (low word)
 *   -> out[n][4] = player c_x, c_y, ball c_x, c_y (the velocity gains c * rand * |v| per axis);
 * 12 the same for the command-less cycle of a reset (block 2 of stream 5, counter = the reset's episode key).
 * The primitives of s2d_rollout_actor (DESIGN.md sections 4, 5): 13 tanh_spec (in[n] -> out[n]), 14 log_spec (in[n] -> out[n]),
 * 15 the Gaussian block of its action noise (Box-Muller on Philox block 3 of stream POLICY): in = uint32[n][4] = global env id
 *   lo, hi, counter, seed (low word) -> out[n][4] = z0..z3. */
int s2d_debug_eval(int op, const void *in_dev, void *out_dev, int64_t n, void *stream);
/* diagnostic: the fused actors' network (s2d_rollout_qnet / s2d_rollout_actor) on caller observations, with the rollout
 * kernels' weight packing, LDS plan and matrix-core layers, so that tests can compare its output bit for bit with the fmaf
 * spec (DESIGN.md sections 4, 5).  params_dev = the network of S2DQNet.params (10-h1-h2-na, nn.Sequential order, 16-byte
 * aligned); obs_dev = float[n][10]; y_dev = float[n][na] <- the output layer's pre-activations; greedy_dev = int32[n] <- their
 * argmax (ties: lowest index; a NaN never replaces the best).  name = NULL or >= 96 bytes <- the kernel's name with its waves
 * per workgroup.  S2D_EINVAL without a launch: widths not in {16, ..., 128} step 16, na not in 1..64, n not in 1..2^31 - 1,
 * NULL or misaligned pointers. */
int s2d_debug_net_forward(int h1, int h2, int na, const void *params_dev, const void *obs_dev, int64_t n, void *y_dev,
                          void *greedy_dev, char *name, void *stream);
/* diagnostic: the same for the general MLP of s2d_rollout_qnet_mlp / s2d_rollout_actor_mlp, with their packing, LDS plan and
 * layer loop.  shape: n_hidden, hidden, n_out (1 .. 64), activation and params are used, epsilon / noise / noise_kind ignored;
 * obs_dev, y_dev = float[n][n_out], greedy_dev and name as above.  S2D_EINVAL without a launch: a shape s2d_rollout_qnet_mlp
 * refuses, n not in 1..2^31 - 1, NULL or misaligned pointers. */
int s2d_debug_mlp_forward(const S2DMlpNet *shape, const void *obs_dev, int64_t n, void *y_dev, void *greedy_dev, char *name,
                          void *stream);
/* diagnostic: the same for the streamed-weight network of s2d_rollout_qnet_wide / s2d_rollout_actor_wide, with their pack kernel,
 * LDS plan and layer loop.  shape: n_hidden, hidden, n_out (1 .. 64), activation, params, workspace and workspace_bytes are used.
 * S2D_EINVAL without a launch: a shape or workspace s2d_rollout_qnet_wide refuses, n not in 1..2^31 - 1, NULL or misaligned
 * pointers. */
int s2d_debug_wide_forward(const S2DWideNet *shape, const void *obs_dev, int64_t n, void *y_dev, void *greedy_dev, char *name,
                           void *stream);
/* diagnostic: the head of s2d_rollout_policy alone, on caller logits or means, so that its edge cases can be compared bit for
 * bit with the spec without running a rollout.  mode: 0 discrete (n_out = A in 1..64), 1 continuous (n_out = 1), 2 turning
 * (n_out = 4).  y_dev = float[n][n_out]; log_std_dev = float[n_out] (may be NULL with mode 0); gid_dev = uint64[n] global env
 * ids; k_dev = uint32[n] policy steps; seed = the Philox key; deterministic as the device word of S2DPolicyNet.  action_dev =
 * int32[n] (mode 0) or float[n][n_out] <- the recorded action; logp_dev = float[n].  S2D_EINVAL without a launch: a mode or
 * n_out outside the above, n not in 1..2^31 - 1, NULL or misaligned pointers. */
int s2d_debug_policy_head(int mode, int n_out, const void *y_dev, const void *log_std_dev, const void *gid_dev, const void *k_dev,
                          uint64_t seed, int deterministic, int64_t n, void *action_dev, void *logp_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* S2D_H_ */
