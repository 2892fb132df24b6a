/* qnet_ref.c -- host restatement of the fused actor's policy (include/s2d.h s2d_rollout_qnet; DESIGN.md sections 4, 5):
 * the forward pass (fmaf chains from the bias in ascending k), relu (v > 0 ? v : +0), the argmax scan and the epsilon
 * threshold.  TEST INFRASTRUCTURE: built on demand with gcc -O2 -ffp-contract=off (tests/qnet_ref.py). */
#include <math.h>
#include <stdint.h>

static float relu(float v) { return v > 0.0f ? v : 0.0f; }

/* out[j] = (relu)(b[j] + sum_k W[j][k] in[k]), k ascending */
static void dense(const float *W, const float *b, const float *in, int m, int k, int use_relu, float *out) {
  for (int j = 0; j < m; ++j) {
    float acc = b[j];
    for (int i = 0; i < k; ++i) acc = fmaf(W[j * k + i], in[i], acc);
    out[j] = use_relu ? relu(acc) : acc;
  }
}

/* x[n][10], params in nn.Sequential order -> q[n][na] */
void qnet_forward(int64_t n, const float *x, const float *params, int h1, int h2, int na, float *q) {
  const float *W1 = params, *b1 = W1 + 10 * h1, *W2 = b1 + h1, *b2 = W2 + h2 * h1, *W3 = b2 + h2, *b3 = W3 + na * h2;
  float a1[128], a2[128];
  for (int64_t e = 0; e < n; ++e) {
    dense(W1, b1, x + 10 * e, h1, 10, 1, a1);
    dense(W2, b2, a1, h2, h1, 1, a2);
    dense(W3, b3, a2, na, h2, 0, q + na * e);
  }
}

/* best = 0; for a = 1 .. A-1: if (q[a] > q[best]) best = a */
void qnet_argmax(int64_t n, const float *q, int na, int32_t *out) {
  for (int64_t e = 0; e < n; ++e) {
    const float *r = q + na * e;
    int best = 0;
    for (int a = 1; a < na; ++a)
      if (r[a] > r[best]) best = a;
    out[e] = best;
  }
}

/* greedy actions of n observations */
void qnet_greedy(int64_t n, const float *x, const float *params, int h1, int h2, int na, float *q_scratch, int32_t *out) {
  qnet_forward(n, x, params, h1, h2, na, q_scratch);
  qnet_argmax(n, q_scratch, na, out);
}

/* eps >= 1 -> 2^32; eps > 0 -> (uint64)(eps * 2^32); else (0, negative, NaN) 0 */
uint64_t qnet_threshold(float eps) {
  if (eps >= 1.0f) return 1ull << 32;
  if (eps > 0.0f) return (uint64_t)(eps * 4294967296.0f);
  return 0;
}
