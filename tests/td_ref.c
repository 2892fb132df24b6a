/* td_ref.c -- host restatement of the TD-target kernels (include/s2d.h S2DTdNet, s2d_td_target_q / s2d_td_target_ac; DESIGN.md
 * section 4): S2DWideNet's MLP with a general input width (layer 1 over 4 ceil(n_in / 4) terms, x_k = 0 against zero weights past
 * n_in), the argmax scan, the two-rounding target, the tanh head, the critics' concatenated input row and the twin minimum.
 * Written from the spec, not from the kernel: plain loops over rows and units.  relu / tanh_spec / sigmoid_spec are wide_ref.c's,
 * included as it stands.  TEST INFRASTRUCTURE: built on demand with gcc -O2 -ffp-contract=off (tests/td.py). */
#include "wide_ref.c"

typedef struct TdNet {
  int32_t n_in, n_hidden, hidden[5], n_out, activation;
  const float *params;
} TdNet;

/* one dense layer: kk >= k terms, those past k are fmaf(+0, +0, acc); act 0 relu, 1 tanh_spec, 2 sigmoid_spec, 3 none */
static void td_dense(const float *W, const float *b, const float *in, int m, int k, int kk, int act, float *out) {
  for (int j = 0; j < m; ++j) {
    float acc = b[j];
    for (int i = 0; i < kk; ++i) {
      const volatile float w = i < k ? W[j * k + i] : 0.0f, v = i < k ? in[i] : 0.0f;
      acc = fmaf(w, v, acc);
    }
    out[j] = act == 0 ? relu(acc) : act == 1 ? tanh_spec(acc) : act == 2 ? sigmoid_spec(acc) : acc;
  }
}

/* one row x[n_in] -> y[n_out] */
static void td_row(const TdNet *net, const float *x, float *y) {
  float a[2][400];
  const float *p = net->params, *in = x;
  int win = net->n_in, kk = (net->n_in + 3) / 4 * 4, cur = 0;
  for (int l = 0; l < net->n_hidden; ++l) {
    const int w = net->hidden[l];
    td_dense(p, p + w * win, in, w, win, kk, net->activation, a[cur]);
    p += w * win + w;
    in = a[cur]; cur ^= 1; win = w; kk = w;
  }
  td_dense(p, p + net->n_out * win, in, net->n_out, win, kk, 3, y);
}

/* x[n][n_in] -> y[n][n_out] */
void td_forward(int64_t n, const TdNet *net, const float *x, float *y) {
  for (int64_t e = 0; e < n; ++e) td_row(net, x + e * net->n_in, y + e * net->n_out);
}

/* best = 0; for a = 1 .. A-1: if (y[a] > y[best]) best = a */
static int td_argmax(const float *y, int na) {
  int best = 0;
  for (int a = 1; a < na; ++a)
    if (y[a] > y[best]) best = a;
  return best;
}

/* reward + (discount * q): one fp32 multiply, then one fp32 add */
static float td_value(float reward, float discount, float q) {
  const volatile float m = discount * q;
  return reward + m;
}

/* s2d_td_target_q: online may be NULL; out_q / out_index may be NULL */
void td_target_q(int64_t n, const TdNet *target, const TdNet *online, const float *next_obs, const float *reward, const float *discount,
                 float *out_target, float *out_q, int32_t *out_index) {
  float y[64], yo[64];
  for (int64_t e = 0; e < n; ++e) {
    const float *x = next_obs + e * target->n_in;
    td_row(target, x, y);
    int best = td_argmax(y, target->n_out);
    if (online) {
      td_row(online, x, yo);
      best = td_argmax(yo, online->n_out);
    }
    out_target[e] = td_value(reward[e], discount[e], y[best]);
    if (out_q) out_q[e] = y[best];
    if (out_index) out_index[e] = best;
  }
}

/* s2d_td_target_ac: critic2 may be NULL; out_q / out_action may be NULL */
void td_target_ac(int64_t n, const TdNet *actor, const TdNet *critic1, const TdNet *critic2, const float *next_obs, const float *reward,
                  const float *discount, float *out_target, float *out_q, float *out_action) {
  const int D = actor->n_in, A = actor->n_out;
  float y[64], row[256], q1, q2;
  for (int64_t e = 0; e < n; ++e) {
    const float *x = next_obs + e * D;
    td_row(actor, x, y);
    for (int k = 0; k < D; ++k) row[k] = x[k];
    for (int i = 0; i < A; ++i) row[D + i] = tanh_spec(y[i]);
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
