/* learn_sac_ref.c -- host restatement of the fused Soft Actor-Critic actor and temperature step (include/s2d.h s2d_learn_sac_actor /
 * s2d_learn_sac_actor_grad): actor forward, the squashed-Gaussian head on the Philox stream
 * S2D_LEARN_SAC_STREAM, both critics forward, the row's minimum and loss, the CHOSEN critic's deltas down to the action columns of
 * its input (the other critic's backward pass is never run here: there is nothing of it that could reach a result), the head's
 * derivative through the tanh correction and the clamped log-std, the actor's backward pass, norm, clip, Adam, and the
 * temperature's scalar Adam.  Written from the spec, not from the kernels: plain loops over rows and units, one block of rows at a
 * time.  The forward chain, the delta chain, the norm and Adam are learn_ref.c's / learn_ac_ref.c's, exp_spec / log_spec /
 * tanh_spec / Box-Muller / Philox actor_ref.c's, included as they stand; SAC's critic step is learn_ac_critic_step with loss kind 0.
 * TEST INFRASTRUCTURE: built on demand with gcc -O2 -ffp-contract=off (tests/learn_sac.py). */
#include "learn_ac_ref.c"

#include "s2d.h" /* S2D_LEARN_SAC_STREAM */

/* one action dimension of the head (s2d_sac_head.h, never deterministic): *a = the squashed action, *sigma = exp_spec of the clamped
 * log-std; returns the dimension's term of logp */
static float sacl_term(float mean, float v, float z, float *a, float *sigma) {
  const float ls = v > 2.0f ? 2.0f : (v >= -20.0f ? v : -20.0f);
  *sigma = exp_spec(ls);
  const float u = fmaf(*sigma, z, mean);
  *a = tanh_spec(u);
  const volatile float half = -0.5f * z;
  const volatile float gauss = fmaf(half, z, -ls) - 0.91893853f;
  const volatile float one_minus = fmaf(-*a, *a, 1.0f);
  const volatile float arg = one_minus + 1e-6f;
  return gauss - log_spec(arg);
}

/* the step's z of row b at call `draws`: zz[8], the first A used */
static void sacl_row_z(int64_t b, int A, uint64_t seed, uint64_t draws, float *zz) {
  for (int j = 0; j < 8; ++j) zz[j] = 0.0f;
  for (int m = 0; m < (A > 4 ? 2 : 1); ++m) {
    uint32_t w[4] = {(uint32_t)b, (uint32_t)draws, (uint32_t)(draws >> 32), ((uint32_t)S2D_LEARN_SAC_STREAM << 16) | (uint32_t)m};
    philox(w, (uint32_t)seed, (uint32_t)(seed >> 32));
    box_muller(w[0], w[1], &zz[4 * m], &zz[4 * m + 1]);
    box_muller(w[2], w[3], &zz[4 * m + 2], &zz[4 * m + 3]);
  }
}

/* z[n][A] of rows 0 .. n-1 at call `draws` */
void learn_sac_z(int64_t n, int A, uint64_t seed, uint64_t draws, float *z) {
  float zz[8];
  for (int64_t b = 0; b < n; ++b) {
    sacl_row_z(b, A, seed, draws, zz);
    for (int j = 0; j < A; ++j) z[A * b + j] = zz[j];
  }
}

/* s2d_learn_sac_actor_grad.  z_in != NULL: z[B][A] given (the host tests' comparison with autograd), else drawn at (seed, draws).
 * critic2 may be NULL.  grad[P of the actor] (unclipped), stats = {mean of alpha * logp - q, norm, scale}, *mean_logp, and where given
 * out_action [B][A], out_logp [B], out_q [B], out_du [B][A], out_dls [B][A] (the head's derivative before the clamp's mask). */
void learn_sac_actor_grad(int64_t B, const LearnNet *actor, const LearnNet *critic1, const LearnNet *critic2, const float *obs, float alpha,
                          const float *z_in, uint64_t seed, uint64_t draws, float max_grad_norm, float *grad, float *stats,
                          float *mean_logp, float *out_action, float *out_logp, float *out_q, float *out_du, float *out_dls) {
  const int La = actor->n_hidden, R = LEARN_BLOCK_ROWS, D = actor->n_in, A = actor->n_out / 2, N = critic1->n_in;
  const int64_t P = learn_param_count(actor), nb = (B + R - 1) / R;
  AcStore sa, sc;
  ac_store(&sa);
  ac_store(&sc);
  float *x = (float *)malloc(sizeof(float) * R * N), *part = (float *)malloc(sizeof(float) * (size_t)P);
  float *zs = (float *)malloc(sizeof(float) * R * 8), *sg = (float *)malloc(sizeof(float) * R * 8), *vs = (float *)malloc(sizeof(float) * R * 8);
  AcStore s2;
  ac_store(&s2);
  const volatile float w = alpha / (float)B;
  float loss_sum = 0.0f, logp_sum = 0.0f;
  for (int64_t blk = 0; blk < nb; ++blk) {
    const int64_t row0 = blk * R;
    const int rows = (int)(B - row0 < R ? B - row0 : R);
    float loss_part = 0.0f, logp_part = 0.0f;
    for (int r = 0; r < rows; ++r) {
      const int64_t b = row0 + r;
      ac_row(&sa, r);
      learn_row_forward(actor, obs + b * D, sa.rowp);
      memcpy(x + r * N, obs + b * D, sizeof(float) * D);
      float zz[8], lp = 0.0f;
      if (z_in) {
        for (int j = 0; j < A; ++j) zz[j] = z_in[b * A + j];
      } else {
        sacl_row_z(b, A, seed, draws, zz);
      }
      const float *y = sa.rowp[La];
      for (int j = 0; j < A; ++j) {
        float a, sigma;
        const float t = sacl_term(y[j], y[A + j], zz[j], &a, &sigma);
        lp = j == 0 ? t : lp + t;
        x[r * N + D + j] = a;
        zs[r * 8 + j] = zz[j];
        sg[r * 8 + j] = sigma;
        vs[r * 8 + j] = y[A + j];
        if (out_action) out_action[b * A + j] = a;
      }
      /* the critics on [obs | a]; the chosen one's layers are kept in sc for the delta pass */
      ac_row(&sc, r);
      learn_row_forward(critic1, x + r * N, sc.rowp);
      float q = sc.rowp[critic1->n_hidden][0];
      const LearnNet *chosen = critic1;
      if (critic2) {
        ac_row(&s2, 0);
        learn_row_forward(critic2, x + r * N, s2.rowp);
        const float q2 = s2.rowp[critic2->n_hidden][0];
        if (q2 < q) { /* a tie or a NaN q2 keeps critic 1 */
          q = q2;
          chosen = critic2;
          for (int l = 0; l <= critic2->n_hidden; ++l) memcpy(sc.rowp[l], s2.rowp[l], sizeof(float) * AC_W);
        }
      }
      if (out_q) out_q[b] = q;
      if (out_logp) out_logp[b] = lp;
      const volatile float ent = alpha * lp;
      const float l = ent - q;
      loss_part = loss_part + l;
      logp_part = logp_part + lp;
      /* the chosen critic's delta pass for this row alone (rows are independent in a pass without dW), down to layer 1's delta */
      sc.rowp[chosen->n_hidden][0] = -1.0f / (float)B;
      {
        float *yy[6];
        for (int l2 = 0; l2 < 6; ++l2) yy[l2] = sc.rowp[l2];
        ac_backward(chosen, 1, x + r * N, N, yy, NULL);
      }
      const int h1 = learn_width(chosen, 0);
      for (int j = 0; j < A; ++j) {
        float s = 0.0f;
        for (int k = 0; k < h1; ++k) s = fmaf(chosen->params[k * N + D + j], sc.rowp[0][k], s);
        const float a = x[r * N + D + j], v = vs[r * 8 + j];
        const volatile float om = fmaf(-a, a, 1.0f);
        const volatile float omd = om + 1e-6f;
        const volatile float rr = om / omd;
        const volatile float two_a = 2.0f * a;
        const volatile float w2a = w * two_a;
        const volatile float t1 = w2a * rr, t2 = s * om;
        const float du = t1 + t2;
        const volatile float sz = sg[r * 8 + j] * zs[r * 8 + j];
        const volatile float dsz = du * sz;
        const float dls = dsz - w;
        if (out_du) out_du[b * A + j] = du;
        if (out_dls) out_dls[b * A + j] = dls;
        sa.y[La][r * AC_W + j] = du;
        sa.y[La][r * AC_W + A + j] = (v >= -20.0f && v <= 2.0f) ? dls : 0.0f;
      }
    }
    ac_backward(actor, rows, obs + row0 * D, D, sa.y, part);
    for (int64_t p = 0; p < P; ++p) grad[p] = blk ? grad[p] + part[p] : part[p];
    loss_sum = blk ? loss_sum + loss_part : loss_part;
    logp_sum = blk ? logp_sum + logp_part : logp_part;
  }
  stats[0] = loss_sum / (float)B;
  *mean_logp = logp_sum / (float)B;
  ac_norm_clip(P, grad, max_grad_norm, stats);
  free(part);
  free(x);
  free(zs);
  free(sg);
  free(vs);
  free(sa.mem);
  free(sc.mem);
  free(s2.mem);
}

/* the temperature: astats[0] = mean_logp, astats[1] = log_alpha * g with g = -(mean_logp + target_entropy); step != 0: the beta products,
 * learn_ref.c's Adam on the one word with scale 1, *alpha = astats[2] = exp_spec(log_alpha) */
void learn_sac_alpha(float mean_logp, float target_entropy, int step, float *log_alpha, float *m_v, float *hyper, float *astats,
                     float *alpha) {
  const volatile float sum = mean_logp + target_entropy;
  const float g = -sum;
  astats[0] = mean_logp;
  astats[1] = *log_alpha * g;
  if (!step) return;
  learn_adam(1, log_alpha, &m_v[0], &m_v[1], &g, hyper, 1.0f);
  *alpha = exp_spec(*log_alpha);
  astats[2] = *alpha;
}

/* s2d_learn_sac_actor: the gradient of the current parameters at the current *alpha and *draws, Adam on the actor, then (log_alpha !=
 * NULL) the temperature, then *draws += 1 */
void learn_sac_actor_step(int64_t B, const LearnNet *actor, const LearnNet *critic1, const LearnNet *critic2, const float *obs, float *alpha,
                          float *log_alpha, float *m_v, float *ahyper, float *astats, float target_entropy, uint64_t *draws, uint64_t seed,
                          float *m, float *v, float *grad, float *hyper, float *stats, float *out_action, float *out_logp, float *out_q) {
  float mean_logp;
  learn_sac_actor_grad(B, actor, critic1, critic2, obs, *alpha, NULL, seed, *draws, hyper[4], grad, stats, &mean_logp, out_action, out_logp,
                       out_q, NULL, NULL);
  learn_adam(learn_param_count(actor), actor->params, m, v, grad, hyper, stats[2]);
  if (log_alpha) learn_sac_alpha(mean_logp, target_entropy, 1, log_alpha, m_v, ahyper, astats, alpha);
  *draws += 1;
}
