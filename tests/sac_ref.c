/* sac_ref.c -- host restatement of Soft Actor-Critic's collection and target (include/s2d.h s2d_rollout_sac, s2d_td_target_sac;
 * DESIGN.md section 5): the squashed-Gaussian head, the rollout policy's z layout on Philox block 3 of stream POLICY, the target's
 * z on stream S2D_TD_STREAM, the critics' input row, the twin minimum and the entropy term.  Written from the spec: plain loops
 * over rows.  The networks are td_ref.c's / wide_ref.c's, exp_spec / log_spec / tanh_spec / Box-Muller / Philox actor_ref.c's,
 * included as they stand.  TEST INFRASTRUCTURE: built on demand with gcc -O2 -ffp-contract=off (tests/sac_ref.py). */
#include "td_ref.c"

#include "s2d.h" /* S2D_TD_STREAM */

/* one action dimension: *a = the squashed action; returns the dimension's term of logp */
float sac_term(float mean, float v, float z, int det, float *a) {
  const float ls = v > 2.0f ? 2.0f : (v >= -20.0f ? v : -20.0f);
  const float sigma = exp_spec(ls);
  const float zj = det ? 0.0f : z;
  const float u = det ? mean : fmaf(sigma, zj, mean);
  *a = tanh_spec(u);
  const volatile float half = -0.5f * zj;
  const volatile float gauss = fmaf(half, zj, -ls) - 0.91893853f;
  const volatile float one_minus = fmaf(-*a, *a, 1.0f);
  const volatile float arg = one_minus + 1e-6f;
  return gauss - log_spec(arg);
}

/* the head on n rows y[n][2A] with z[n][A]: action[n][A], logp[n] = t_0 (+ t_1 ... in ascending j) */
void sac_head(int64_t n, int A, const float *y, const float *z, int det, float *action, float *logp) {
  for (int64_t e = 0; e < n; ++e) {
    float lp = 0.0f;
    for (int j = 0; j < A; ++j) {
      const float t = sac_term(y[2 * A * e + j], y[2 * A * e + A + j], z[A * e + j], det, &action[A * e + j]);
      lp = j == 0 ? t : lp + t;
    }
    logp[e] = lp;
  }
}

/* the rollout's z of n envs (global ids gid0 + e) at policy steps k[e]: mode 1 continuous (A = 1: z_{k & 3} of POLICY block 3 at
 * counter k >> 2), 2 turning (A = 4: z0..z3 of the block at counter k) */
void sac_rollout_z(int64_t n, int mode, uint64_t seed, uint64_t gid0, const uint32_t *k, float *z) {
  for (int64_t e = 0; e < n; ++e) {
    uint32_t w[4];
    float zz[4];
    policy_block(seed, gid0 + (uint64_t)e, mode == 2 ? k[e] : k[e] >> 2, 3, w);
    box_muller(w[0], w[1], &zz[0], &zz[1]);
    box_muller(w[2], w[3], &zz[2], &zz[3]);
    if (mode == 2) for (int j = 0; j < 4; ++j) z[4 * e + j] = zz[j];
    else z[e] = zz[k[e] & 3];
  }
}

/* the rollout policy: observations x[n][10] -> action[n][A], logp[n]; y_scratch[n][2A], z_scratch[n][A] */
void sac_actions(int64_t n, const float *x, const float *params, int n_hidden, const int32_t *hidden, int activation, int mode, int det,
                 uint64_t seed, uint64_t gid0, const uint32_t *k, float *y_scratch, float *z_scratch, float *action, float *logp) {
  const int A = mode == 2 ? 4 : 1;
  wide_forward(n, x, params, n_hidden, hidden, 2 * A, activation, y_scratch);
  sac_rollout_z(n, mode, seed, gid0, k, z_scratch);
  sac_head(n, A, y_scratch, z_scratch, det, action, logp);
}

/* the target's z of rows 0 .. n-1 at call `draws`: z[n][A], A in 1..8 */
void sac_td_z(int64_t n, int A, uint64_t seed, uint64_t draws, float *z) {
  for (int64_t b = 0; b < n; ++b) {
    float zz[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int m = 0; m < (A > 4 ? 2 : 1); ++m) {
      uint32_t w[4] = {(uint32_t)b, (uint32_t)draws, (uint32_t)(draws >> 32), ((uint32_t)S2D_TD_STREAM << 16) | (uint32_t)m};
      philox(w, (uint32_t)seed, (uint32_t)(seed >> 32));
      box_muller(w[0], w[1], &zz[4 * m], &zz[4 * m + 1]);
      box_muller(w[2], w[3], &zz[4 * m + 2], &zz[4 * m + 3]);
    }
    for (int j = 0; j < A; ++j) z[A * b + j] = zz[j];
  }
}

/* s2d_td_target_sac (det: its diagnostic form): critic2, out_q, out_action, out_logp may be NULL */
void sac_target(int64_t n, const TdNet *actor, const TdNet *critic1, const TdNet *critic2, const float *next_obs, const float *reward,
                const float *discount, float alpha, uint64_t draws, uint64_t seed, int det, float *out_target, float *out_q,
                float *out_action, float *out_logp) {
  const int D = actor->n_in, A = actor->n_out / 2;
  float y[64], row[256], z[8], q1, q2, lp;
  for (int64_t e = 0; e < n; ++e) {
    const float *x = next_obs + e * D;
    td_row(actor, x, y);
    for (int k = 0; k < D; ++k) row[k] = x[k];
    for (int j = 0; j < 8; ++j) z[j] = 0.0f;
    if (!det) {
      for (int m = 0; m < (A > 4 ? 2 : 1); ++m) {
        uint32_t w[4] = {(uint32_t)e, (uint32_t)draws, (uint32_t)(draws >> 32), ((uint32_t)S2D_TD_STREAM << 16) | (uint32_t)m};
        philox(w, (uint32_t)seed, (uint32_t)(seed >> 32));
        box_muller(w[0], w[1], &z[4 * m], &z[4 * m + 1]);
        box_muller(w[2], w[3], &z[4 * m + 2], &z[4 * m + 3]);
      }
    }
    sac_head(1, A, y, z, det, row + D, &lp);
    td_row(critic1, row, &q1);
    float q = q1;
    if (critic2) {
      td_row(critic2, row, &q2);
      q = q2 < q1 ? q2 : q1;
    }
    const volatile float ent = alpha * lp;
    const volatile float v = q - ent;
    out_target[e] = td_value(reward[e], discount[e], v);
    if (out_q) out_q[e] = q;
    if (out_logp) out_logp[e] = lp;
    if (out_action)
      for (int j = 0; j < A; ++j) out_action[e * A + j] = row[D + j];
  }
}
