/* mlp_ref.c -- host restatement of the general MLP of the fused actors (include/s2d.h S2DMlpNet, s2d_rollout_qnet_mlp /
 * s2d_rollout_actor_mlp): one to four hidden layers, every unit an fmaf chain from its bias in ascending
 * k, layer 1 over k = 0 .. 11 with x_10 = x_11 = 0 against zero weights, relu (v > 0 ? v : +0) or tanh_spec between the layers,
 * a linear output layer, the argmax scan; and the tanh actor's head on its outputs.  tanh_spec, the Gaussian block, the
 * exploration draws and the random action are actor_ref.c's, included here as they stand.  TEST INFRASTRUCTURE: built on
 * demand with gcc -O2 -ffp-contract=off (tests/mlp_ref.py). */
#include "actor_ref.c"

/* out[j] = act(b[j] + sum_k W[j][k] in[k]), k ascending over kk >= k terms: the terms past k are fmaf(0, 0, acc);
 * act: 0 none, 1 relu, 2 tanh_spec */
static void mlp_dense(const float *W, const float *b, const float *in, int m, int k, int kk, int act, float *out) {
  for (int j = 0; j < m; ++j) {
    float acc = b[j];
    for (int i = 0; i < kk; ++i) {
      const volatile float w = i < k ? W[j * k + i] : 0.0f, v = i < k ? in[i] : 0.0f;
      acc = fmaf(w, v, acc);
    }
    out[j] = act == 1 ? relu(acc) : act == 2 ? tanh_spec(acc) : acc;
  }
}

/* x[n][10], params in nn.Sequential order, hidden[n_hidden], activation 0 relu / 1 tanh_spec -> y[n][na].  first_k = the
 * k-range of layer 1: 12 is the spec; 10 (no padding terms) exists so that a test can show the difference. */
void mlp_forward(int64_t n, const float *x, const float *params, int n_hidden, const int32_t *hidden, int na, int activation,
                 int first_k, float *y) {
  float a[2][128];
  for (int64_t e = 0; e < n; ++e) {
    const float *p = params, *in = x + 10 * e;
    int win = 10, kk = first_k, cur = 0;
    for (int l = 0; l < n_hidden; ++l) {
      const int w = hidden[l];
      mlp_dense(p, p + w * win, in, w, win, kk, activation ? 2 : 1, a[cur]);
      p += w * win + w;
      in = a[cur]; cur ^= 1; win = w; kk = w;
    }
    mlp_dense(p, p + na * win, in, na, win, kk, 0, y + na * e);
  }
}

/* best = 0; for a = 1 .. A-1: if (y[a] > y[best]) best = a */
void mlp_argmax(int64_t n, const float *y, int na, int32_t *out) {
  for (int64_t e = 0; e < n; ++e) {
    const float *r = y + na * e;
    int best = 0;
    for (int a = 1; a < na; ++a)
      if (r[a] > r[best]) best = a;
    out[e] = best;
  }
}

/* the tanh actor's action of n envs from its network's outputs y[n][na]: actor_actions of actor_ref.c (the same draws, in
 * the same order) behind another network */
void mlp_actor_actions(int64_t n, const float *y, int na, float eps, int kind, const float *noise, uint64_t seed, uint64_t gid0,
                       const uint32_t *k, float *out) {
  const uint64_t thr = threshold(eps);
  for (int64_t e = 0; e < n; ++e) {
    const uint64_t gid = gid0 + (uint64_t)e;
    const uint32_t ke = k[e];
    uint32_t w[4];
    float *a = out + na * e;
    policy_block(seed, gid, ke >> 2, 2, w);
    if ((uint64_t)w[ke & 3] < thr) {
      if (na == 4) {
        policy_block(seed, gid, ke, 1, w);
        for (int j = 0; j < 4; ++j) a[j] = rnd_pm1(w[j]);
      } else {
        policy_block(seed, gid, ke >> 2, 0, w);
        a[0] = rnd_pm1(w[ke & 3]);
      }
      continue;
    }
    float z[4] = {0, 0, 0, 0};
    if (kind == 1) {
      if (na == 4) {
        policy_block(seed, gid, ke, 3, w);
        box_muller(w[0], w[1], &z[0], &z[1]);
        box_muller(w[2], w[3], &z[2], &z[3]);
      } else {
        float zz[4];
        policy_block(seed, gid, ke >> 2, 3, w);
        box_muller(w[0], w[1], &zz[0], &zz[1]);
        box_muller(w[2], w[3], &zz[2], &zz[3]);
        z[0] = zz[ke & 3];
      }
    }
    for (int j = 0; j < na; ++j) {
      float v = tanh_spec(y[na * e + j]);
      if (kind == 1) {
        v = v + fmaf(noise[na + j], z[j], noise[j]);
        v = v < -1.0f ? -1.0f : v > 1.0f ? 1.0f : v;
      }
      a[j] = v;
    }
  }
}
