/* see_net_ref.c -- host restatement of the 11v11 engine's see network (include/s2d_match.h, "See network"): the D-H1-H2-K forward
 * pass in the k-ordered fmaf spec with the input width D as an argument (192 for the see row).  The argmax, the epsilon threshold
 * and the exploration draws are those of the network slots (tests/match_net_ref.c, tests/match_net.py).  TEST INFRASTRUCTURE: built
 * with -ffp-contract=off (the fp32 contract). */
#include <math.h>
#include <stdint.h>

static float relu(float v) { return v > 0.0f ? v : 0.0f; }   /* NaN and -0 -> +0 */

/* one layer: out[j] = (relu)(b[j] + sum_k W[j][k] in[k]), k ascending, one fmaf per term */
static void layer(const float *w, const float *b, const float *in, int n_in, int n_out, int act, float *out) {
  for (int j = 0; j < n_out; ++j) {
    float acc = b[j];
    for (int k = 0; k < n_in; ++k) acc = fmaf(w[j * n_in + k], in[k], acc);
    out[j] = act ? relu(acc) : acc;
  }
}

/* q[i][K] for n rows x[i][dim]; params in nn.Sequential order W1[h1][dim] b1 W2 b2 W3 b3 */
void snet_forward(int64_t n, int dim, const float *x, const float *params, int h1, int h2, int na, float *q) {
  const float *w1 = params, *b1 = w1 + h1 * dim, *w2 = b1 + h1, *b2 = w2 + h2 * h1, *w3 = b2 + h2, *b3 = w3 + na * h2;
  float ha[64], hb[64];
  for (int64_t i = 0; i < n; ++i) {
    layer(w1, b1, x + i * dim, dim, h1, 1, ha);
    layer(w2, b2, ha, h1, h2, 1, hb);
    layer(w3, b3, hb, h2, na, 0, q + i * na);
  }
}
