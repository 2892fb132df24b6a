/*
 * s2d_gtc.h -- C ABI of the GoToCenter surrogate task: the reference's
 * pure-Python kinematic stand-in for reach_ball, GoToCenterEnv (python_sample_soccer_env.py:46-255),
 * as a second built-in batched task of libs2d_hip.so.  Same conventions as s2d.h.
 *
 *   s2d_gtc_reset   GoToCenterEnv.reset   python_sample_soccer_env.py:115-134
 *   s2d_gtc_step    GoToCenterEnv.step    python_sample_soccer_env.py:136-233
 *   obs             GoToCenterEnv._get_obs :235-255  [angle_diff/180, body/180, x/52.5, y/34]
 */
#ifndef S2D_GTC_H_
#define S2D_GTC_H_
#include "s2d.h"
#ifdef __cplusplus
extern "C" {
#endif

#define S2D_GTC_OBS_DIM 4

typedef struct S2DGtcConfig {
  uint32_t abi_version, struct_bytes;
  double x_min, x_max, y_min, y_max;      /* -52.5 52.5 -34 34      :93-94  */
  double min_distance_to_center;          /* 5.0                    :98     */
  int32_t max_steps;                      /* 200                    :97     */
  int32_t continuous;                     /* 0: Discrete(16) dash_r = (a/16 - .5)*2  :163-166; 1: Box(-1,1,(1,)) clipped :159-162 */
  uint64_t seed;
  int64_t env_id_offset;
  int32_t auto_reset;
  /* the script's --turn / --useturn / --actor_out_size switches (:70-79, :142-158; argparse defaults
   * True / True / 4, :356-359).  turn && continuous: Box(-1,1,(actor_out_size,)), actions[0] = dash angle;
   * with use_turn also actions[1] = turn angle, [2] = dash logit, [3] = turn logit, softmax([turn, dash]),
   * turn chosen iff U(0,1) < p[0] (:149-152); a turn changes the body, a dash does not. */
  int32_t turn, use_turn, actor_out_size;   /* 0, 0, 1 by default (the class's own defaults, :66) */
} S2DGtcConfig;

typedef struct S2DGtcBuffers {
  int64_t n_envs;
  float *x, *y, *body, *prev_distance, *prev_angle_diff;   /* :98-109 */
  int32_t *step_count, *episode;
  float *obs;            /* [N][4] */
  float *reward;         /* [N] */
  uint8_t *done;         /* [N] terminated or truncated */
  uint8_t *result;       /* [N] S2D_RESULT_* ('' / 'Goal' / 'Out' / 'Timeout', :198-217) */
  float *terminal_obs;   /* [N][4] */
  unsigned long long *stats;   /* [S2D_STATS_STRIPES][8]: env-steps, Goal, Out, Timeout */
} S2DGtcBuffers;

typedef struct S2DGtcRollout { float *obs; void *action; float *reward; uint8_t *done; uint8_t *result; } S2DGtcRollout;
typedef struct S2DGtcEngine *S2DGtcHandle;

void s2d_gtc_default_config(S2DGtcConfig *cfg);
size_t s2d_gtc_arena_bytes(const S2DGtcConfig *cfg, int64_t n_envs);
int s2d_gtc_create(const S2DGtcConfig *cfg, int64_t n_envs, int device, void *arena_dev, size_t arena_bytes,
                   void *stream, S2DGtcHandle *out);
void s2d_gtc_destroy(S2DGtcHandle h);
int s2d_gtc_buffer_offsets(S2DGtcHandle h, int64_t *offsets, int n_offsets);
int s2d_gtc_reset(S2DGtcHandle h, const uint8_t *mask_dev, void *stream);
/* actions: int32[N] (discrete), float[N] (continuous) or float[N][actor_out_size] (turn && continuous);
 * NULL = uniform random policy */
int s2d_gtc_step(S2DGtcHandle h, const void *actions_dev, void *stream);
/* same, with the turn / dash selection uniforms of :151 supplied by the caller (float[N] in [0,1)) instead of
 * the engine's Philox SELECT stream -- for callers that own the RNG, and for the reference-fixture tests */
int s2d_gtc_step_u(S2DGtcHandle h, const void *actions_dev, const float *select_u_dev, void *stream);
int s2d_gtc_rollout(S2DGtcHandle h, int n_steps, const S2DGtcRollout *out, void *stream);   /* random policy */

/* The fused actors (DESIGN.md sections 4, 5): the caller's network evaluated inside the rollout kernel on each env's own
 * 4-word observation -- an epsilon-greedy Q-network on a discrete engine (s2d_gtc_rollout_qnet, n_out = 16) and a
 * deterministic tanh policy with optional Gaussian action noise on a continuous or turn-mode engine (s2d_gtc_rollout_actor,
 * n_out = the engine's action width: actor_out_size in the turn mode, else 1).
 *   network   S2DWideNet (s2d.h) read with "10 ->" as "4 ->": 4 -> h_1 -> ... -> h_L -> n_out, L in 1..5, widths multiples of 4 in
 *             [8, 400], relu / tanh_spec / sigmoid_spec, linear output; params in nn.Sequential(...).parameters() order
 *             (W_1[h_1][4], b_1, ...); every unit acc = b[j]; for k ascending: acc = fmaf(W[j][k], in[k], acc).
 *   layer 1   runs over exactly k = 0 .. 3: no zero pad, so an accumulator of -0 STAYS -0 (S2DWideNet's padded layer 1 on the
 *             10-word observation turns it into +0).
 *   draws     env g in episode j at step s = step_count: philox(g, j, (stream << 16) | s, seed), s2d_gtc_rollout's keying.
 *             explore = (uint64)w.x < threshold(epsilon) with w from stream 9 (eps >= 1: always; eps <= 0 or NaN: never).
 *             Exploring: the random policy's own action (stream POLICY), no action noise: epsilon = 1 IS s2d_gtc_rollout.
 *             Else Q head: the first maximum of y (a NaN never wins); tanh head: a_j = tanh_spec(y_j), with noise_kind = 1
 *             a_j = clip(a_j + fmaf(sigma_j, z_j, mu_j), -1, 1), z0, z1 = box_muller(w.x, w.y), z2, z3 = box_muller(w.z, w.w) of
 *             stream 10, noise = [2][n_out] (mu, sigma).  The turn / dash uniform of use_turn stays the SELECT stream's.
 *   records   S2DGtcRollout's, and terminal_obs [T][N][4] (may be NULL; 16-byte aligned), written only where done: the
 *             observation the episode ended on.  State planes, per-step outputs and statistics as s2d_gtc_rollout leaves them.
 *   workspace at least s2d_gtc_actor_workspace_bytes() bytes (0 for a shape off the grid; needs no device), 256-byte aligned:
 *             every call first writes the fragments there (a pack kernel on `stream`), then the rollout reads them; params,
 *             epsilon and noise are read when the kernels run.  One launch at a time per workspace.
 * S2D_WIDE_PLAN=waves,tiles overrides the LDS plan (testing; the result does not depend on it).  Refusals return S2D_EINVAL
 * with a text and launch nothing; n_steps = 0 is a no-op.  s2d_gtc_debug_forward: the network alone on obs [n][4] -> y [n][n_out]
 * and the first maximum greedy [n] (name: 96 bytes or NULL).  s2d_gtc_kernel_name: the last fused launch of the handle. */
size_t s2d_gtc_actor_workspace_bytes(const S2DWideNet *shape);
int s2d_gtc_rollout_qnet(S2DGtcHandle h, int n_steps, const S2DWideNet *net, const S2DGtcRollout *out, float *terminal_obs,
                         void *stream);
int s2d_gtc_rollout_actor(S2DGtcHandle h, int n_steps, const S2DWideNet *net, const S2DGtcRollout *out, float *terminal_obs,
                          void *stream);
int s2d_gtc_debug_forward(const S2DWideNet *shape, const void *obs_dev, int64_t n, void *y_dev, void *greedy_dev, char *name,
                          void *stream);
const char *s2d_gtc_kernel_name(S2DGtcHandle h);

#ifdef __cplusplus
}
#endif
#endif
