/* wide_ref.c -- host restatement of the streamed-weight MLP of the fused actors (include/s2d.h S2DWideNet, s2d_rollout_qnet_wide /
 * s2d_rollout_actor_wide): one to five hidden layers of 8 .. 400 units (multiples of 4), every unit an fmaf
 * chain from its bias in ascending k, layer 1 over k = 0 .. 11 with x_10 = x_11 = 0 against zero weights, relu (v > 0 ? v : +0),
 * tanh_spec or sigmoid_spec between the layers, a linear output layer.  Written from the spec, not from the kernel: plain loops
 * over units, no tiles, no fragments.  exp_spec and tanh_spec are actor_ref.c's, included as they stand; the argmax, the draws and
 * the tanh actor's head on the outputs are mlp_ref's (tests/wide_ref.py calls them).  TEST INFRASTRUCTURE: built on demand with
 * gcc -O2 -ffp-contract=off (tests/wide_ref.py). */
#include "actor_ref.c"

/* the logistic function, every step one fp32 operation: a = |v| but at most 87 (NaN too), t = exp_spec(-a), d = 1 + t,
 * v >= 0: 1 / d, else t / d; NaN passes */
float sigmoid_spec(float v) {
  if (v != v) return v;
  float a = fabsf(v);
  if (!(a < 87.0f)) a = 87.0f;
  const volatile float t = exp_spec(-a);
  const volatile float d = 1.0f + t;
  return v >= 0.0f ? 1.0f / d : t / d;
}

void wide_sigmoid(int64_t n, const float *v, float *out) {
  for (int64_t i = 0; i < n; ++i) out[i] = sigmoid_spec(v[i]);
}

/* act: 0 relu, 1 tanh_spec, 2 sigmoid_spec, 3 none; kk >= k terms, those past k are fmaf(0, 0, acc) */
static void wide_dense(const float *W, const float *b, const float *in, int m, int k, int kk, int act, float *out) {
  for (int j = 0; j < m; ++j) {
    float acc = b[j];
    for (int i = 0; i < kk; ++i) {
      const volatile float w = i < k ? W[j * k + i] : 0.0f, v = i < k ? in[i] : 0.0f;
      acc = fmaf(w, v, acc);
    }
    out[j] = act == 0 ? relu(acc) : act == 1 ? tanh_spec(acc) : act == 2 ? sigmoid_spec(acc) : acc;
  }
}

/* x[n][10], params in nn.Sequential order, hidden[n_hidden], activation 0 / 1 / 2 -> y[n][na] */
void wide_forward(int64_t n, const float *x, const float *params, int n_hidden, const int32_t *hidden, int na, int activation,
                  float *y) {
  float a[2][400];
  for (int64_t e = 0; e < n; ++e) {
    const float *p = params, *in = x + 10 * e;
    int win = 10, kk = 12, cur = 0;
    for (int l = 0; l < n_hidden; ++l) {
      const int w = hidden[l];
      wide_dense(p, p + w * win, in, w, win, kk, activation, a[cur]);
      p += w * win + w;
      in = a[cur]; cur ^= 1; win = w; kk = w;
    }
    wide_dense(p, p + na * win, in, na, win, kk, 3, y + na * e);
  }
}
