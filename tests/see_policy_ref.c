/* see_policy_ref.c -- host restatement of the forward pass of the 11v11 engine's see policy slots (include/s2d_match.h, "See
 * policy slots"): D-H1-H2-K logits in the k-ordered fmaf spec, the input width D as an argument (192 for the see row), relu or
 * tanh_spec on both hidden layers, a linear output layer.  tanh_spec is actor_ref.c's, included as it is.  The categorical head
 * and the slot's Philox block are tests/match_policy_ref.c's (tests/see_policy.py calls that library): nothing of them is
 * restated here.  TEST INFRASTRUCTURE: built on demand with gcc -O2 -ffp-contract=off (tests/see_policy.py). */
#include "actor_ref.c"

/* one layer: out[j] = f(b[j] + sum_k W[j][k] in[k]), k ascending, one fmaf per term; act 0: none, 1: relu, 2: tanh_spec */
static void sp_layer(const float *w, const float *b, const float *in, int n_in, int n_out, int act, float *out) {
  for (int j = 0; j < n_out; ++j) {
    float acc = b[j];
    for (int k = 0; k < n_in; ++k) acc = fmaf(w[j * n_in + k], in[k], acc);
    out[j] = act == 1 ? relu(acc) : act == 2 ? tanh_spec(acc) : acc;
  }
}

/* y[i][K] for n rows x[i][dim]; params in nn.Sequential order W1[h1][dim] b1 W2 b2 W3 b3; act 0: relu, 1: tanh_spec */
void spol_forward(int64_t n, int dim, const float *x, const float *params, int h1, int h2, int na, int act, float *y) {
  const float *w1 = params, *b1 = w1 + h1 * dim, *w2 = b1 + h1, *b2 = w2 + h2 * h1, *w3 = b2 + h2, *b3 = w3 + na * h2;
  const int f = act ? 2 : 1;
  float ha[64], hb[64];
  for (int64_t i = 0; i < n; ++i) {
    sp_layer(w1, b1, x + i * dim, dim, h1, f, ha);
    sp_layer(w2, b2, ha, h1, h2, f, hb);
    sp_layer(w3, b3, hb, h2, na, 0, y + i * na);
  }
}
