/* td3_ref.c -- host restatement of TD3's target with target-policy smoothing (include/s2d.h s2d_td_target_td3; DESIGN.md section
 * 4): the target actor's tanh head, z on Philox stream S2D_TD3_STREAM, the clipped noise, the clamped sum, the critics' input row,
 * the twin minimum and the two-rounding target.  Written from the spec: plain loops over rows.  The networks and td_value are
 * td_ref.c's, tanh_spec / Box-Muller / Philox actor_ref.c's, included as they stand.  TEST INFRASTRUCTURE: built on demand with
 * gcc -O2 -ffp-contract=off (tests/td3.py). */
#include "td_ref.c"

#include "s2d.h" /* S2D_TD3_STREAM */

/* Philox blocks drawn since the library was loaded (tests: A <= 4 never draws block 1) */
uint64_t td3_blocks = 0;

/* z0 .. z7 of global row b at call `draws`: block 0 gives z0..z3, block 1 (drawn only if A > 4) z4..z7; what is not drawn is 0 */
static void td3_row_z(int64_t b, int A, uint64_t seed, uint64_t draws, float z[8]) {
  for (int j = 0; j < 8; ++j) z[j] = 0.0f;
  for (int blk = 0; blk < (A > 4 ? 2 : 1); ++blk) {
    uint32_t w[4] = {(uint32_t)b, (uint32_t)draws, (uint32_t)(draws >> 32), ((uint32_t)S2D_TD3_STREAM << 16) | (uint32_t)blk};
    philox(w, (uint32_t)seed, (uint32_t)(seed >> 32));
    box_muller(w[0], w[1], &z[4 * blk], &z[4 * blk + 1]);
    box_muller(w[2], w[3], &z[4 * blk + 2], &z[4 * blk + 3]);
    td3_blocks += 1;
  }
}

/* z[n][A] of rows row0 .. row0 + n - 1 */
void td3_z(int64_t n, int64_t row0, int A, uint64_t seed, uint64_t draws, float *z) {
  float zz[8];
  for (int64_t e = 0; e < n; ++e) {
    td3_row_z(row0 + e, A, seed, draws, zz);
    for (int j = 0; j < A; ++j) z[A * e + j] = zz[j];
  }
}

/* one action word: clamp(m + clamp(sigma z, -clip, clip), -1, 1); one multiply, one add, a NaN passes through both clamps */
float td3_smooth(float m, float sigma, float clip, float z) {
  const volatile float p = sigma * z;
  const float n = p < -clip ? -clip : (p > clip ? clip : p);
  const volatile float s = m + n;
  return s < -1.0f ? -1.0f : (s > 1.0f ? 1.0f : s);
}

/* n words at once */
void td3_smooth_n(int64_t n, const float *m, float sigma, float clip, const float *z, float *out) {
  for (int64_t i = 0; i < n; ++i) out[i] = td3_smooth(m[i], sigma, clip, z[i]);
}

/* s2d_td_target_td3: critic2, out_q, out_action may be NULL; out_mean (the unsmoothed tanh_spec(y)) is the restatement's own */
void td3_target(int64_t n, const TdNet *actor, const TdNet *critic1, const TdNet *critic2, const float *next_obs, const float *reward,
                const float *discount, float sigma, float clip, uint64_t draws, uint64_t seed, float *out_target, float *out_q,
                float *out_action, float *out_mean) {
  const int D = actor->n_in, A = actor->n_out;
  float y[64], row[256], z[8], q1, q2;
  for (int64_t e = 0; e < n; ++e) {
    const float *x = next_obs + e * D;
    td_row(actor, x, y);
    td3_row_z(e, A, seed, draws, z);
    for (int k = 0; k < D; ++k) row[k] = x[k];
    for (int i = 0; i < A; ++i) {
      const float m = tanh_spec(y[i]);
      row[D + i] = td3_smooth(m, sigma, clip, z[i]);
      if (out_mean) out_mean[e * A + i] = m;
    }
    td_row(critic1, row, &q1);
    float q = q1;
    if (critic2) {
      td_row(critic2, row, &q2);
      q = q2 < q1 ? q2 : q1;
    }
    out_target[e] = td_value(reward[e], discount[e], q);
    if (out_q) out_q[e] = q;
    if (out_action)
      for (int i = 0; i < A; ++i) out_action[e * A + i] = row[D + i];
  }
}
