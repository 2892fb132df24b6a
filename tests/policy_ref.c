/* policy_ref.c -- host restatement of the fused stochastic policy and of the advantage scan (include/s2d.h s2d_rollout_policy,
 * s2d_debug_policy_head, s2d_gae; DESIGN.md sections 4, 5): the forward pass with either hidden activation, the categorical
 * head, the Gaussian head, logp, the deterministic switch and gae.  Every fp32 operation in the order the device code fixes.
 * exp_spec / log_spec / tanh_spec / Box-Muller / Philox are those of actor_ref.c, included as they are.
 * TEST INFRASTRUCTURE: built on demand with gcc -O2 -ffp-contract=off (tests/policy_ref.py). */
#include "actor_ref.c"

/* out[j] = f(b[j] + sum_k W[j][k] in[k]), k ascending; pad: two more fmaf(0, 0, acc) (layer 1 runs over k = 0 .. 11 on the
 * device: an accumulator of -0 becomes +0); act: 0 relu, 1 tanh_spec, -1 none */
static void pdense(const float *W, const float *b, const float *in, int m, int k, int pad, int act, float *out) {
  for (int j = 0; j < m; ++j) {
    float acc = b[j];
    for (int i = 0; i < k; ++i) acc = fmaf(W[j * k + i], in[i], acc);
    for (int i = 0; i < pad; ++i) acc = fmaf(0.0f, 0.0f, acc);
    out[j] = act == 0 ? relu(acc) : act == 1 ? tanh_spec(acc) : acc;
  }
}

/* x[n][10], params in nn.Sequential order, act 0 relu / 1 tanh -> y[n][na] (logits or means) */
void policy_forward(int64_t n, const float *x, const float *params, int h1, int h2, int na, int act, float *y) {
  const float *W1 = params, *b1 = W1 + 10 * h1, *W2 = b1 + h1, *b2 = W2 + h2 * h1, *W3 = b2 + h2, *b3 = W3 + na * h2;
  float a1[128], a2[128];
  for (int64_t e = 0; e < n; ++e) {
    pdense(W1, b1, x + 10 * e, h1, 10, 2, act, a1);
    pdense(W2, b2, a1, h2, h1, 0, act, a2);
    pdense(W3, b3, a2, na, h2, 0, -1, y + na * e);
  }
}

/* the categorical head on logits q[0 .. A-1] with the uniform word w */
static int categorical(const float *q, int A, int det, uint32_t w, float *logp) {
  int g = 0;
  float m = q[0];
  for (int a = 1; a < A; ++a) if (q[a] > m) { m = q[a]; g = a; }
  float S = exp_spec(q[0] - m);
  for (int a = 1; a < A; ++a) S += exp_spec(q[a] - m);
  int act = g;
  if (!det) {
    const float u = (float)(w >> 8) * 5.9604644775390625e-8f;
    const float target = u * S;
    float c = 0.0f;
    for (int a = 0; a < A; ++a) {
      c += exp_spec(q[a] - m);
      if (c > target) { act = a; break; }
    }
  }
  *logp = (q[act] - m) - log_spec(S);
  return act;
}

/* n rows of logits with caller-supplied uniform words (the edge cases of the draw) */
void policy_categorical(int64_t n, int A, const float *y, const uint32_t *w, int det, int32_t *action, float *logp) {
  for (int64_t e = 0; e < n; ++e) action[e] = categorical(y + A * e, A, det, w[e], logp + e);
}

static float clip1(float v) { return v < -1.0f ? -1.0f : v > 1.0f ? 1.0f : v; }

/* the head alone: mode 0 discrete (action = int32[n]), 1 continuous (float[n][1]), 2 turning (float[n][4]) */
void policy_head(int mode, int na, int64_t n, const float *y, const float *log_std, const uint64_t *gid, const uint32_t *k,
                 uint64_t seed, int det, void *action, float *logp) {
  for (int64_t e = 0; e < n; ++e) {
    const uint32_t ke = k[e];
    uint32_t w[4];
    if (mode == 0) {
      policy_block(seed, gid[e], ke >> 2, 4, w);
      ((int32_t *)action)[e] = categorical(y + na * e, na, det, w[ke & 3], logp + e);
      continue;
    }
    float z[4] = {0, 0, 0, 0};
    if (!det) {
      if (mode == 2) {
        policy_block(seed, gid[e], ke, 3, w);
        box_muller(w[0], w[1], &z[0], &z[1]);
        box_muller(w[2], w[3], &z[2], &z[3]);
      } else {
        float zz[4];
        policy_block(seed, gid[e], ke >> 2, 3, w);
        box_muller(w[0], w[1], &zz[0], &zz[1]);
        box_muller(w[2], w[3], &zz[2], &zz[3]);
        z[0] = zz[ke & 3];
      }
    }
    float lp = 0.0f;
    for (int j = 0; j < na; ++j) {
      const float yj = y[na * e + j], zj = det ? 0.0f : z[j];
      ((float *)action)[na * e + j] = det ? clip1(yj) : fmaf(exp_spec(log_std[j]), zj, yj);
      const float term = fmaf(-0.5f * zj, zj, -log_std[j]) - 0.91893853f;
      lp = j == 0 ? term : lp + term;
    }
    logp[e] = lp;
  }
}

/* the policy's action and logp of n envs (global ids gid0 + e) at policy steps k[e] on observations x; y_scratch[n][na] */
void policy_actions(int64_t n, const float *x, const float *params, int h1, int h2, int na, int act, int mode, const float *log_std,
                    int det, uint64_t seed, uint64_t gid0, const uint32_t *k, float *y_scratch, uint64_t *gid_scratch, void *action,
                    float *logp) {
  policy_forward(n, x, params, h1, h2, na, act, y_scratch);
  for (int64_t e = 0; e < n; ++e) gid_scratch[e] = gid0 + (uint64_t)e;
  policy_head(mode, na, n, y_scratch, log_std, gid_scratch, k, seed, det, action, logp);
}

/* s2d_gae: result / tval NULL or both given; 3 = S2D_RESULT_TIMEOUT */
void policy_gae(int T, int64_t N, const float *reward, const uint8_t *done, const float *value, const float *last_value,
                const uint8_t *result, const float *tval, float gamma, float lam, float *adv, float *ret) {
  const float gl = gamma * lam;
  for (int64_t i = 0; i < N; ++i) {
    float next_v = last_value[i], gae = 0.0f;
    for (int t = T - 1; t >= 0; --t) {
      const int64_t idx = (int64_t)t * N + i;
      float r = reward[idx];
      if (result && result[idx] == 3) r = fmaf(gamma, tval[idx], r);
      const float nt = done[idx] ? 0.0f : 1.0f;
      const float v = value[idx];
      const float delta = fmaf(gamma * nt, next_v, r) - v;
      gae = fmaf(gl * nt, gae, delta);
      adv[idx] = gae;
      ret[idx] = gae + v;
      next_v = v;
    }
  }
}
