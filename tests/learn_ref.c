/* learn_ref.c -- host restatement of the fused Q-learner step (include/s2d.h S2DLearnNet / S2DLearnState, s2d_learn_q /
 * s2d_learn_q_grad): the forward pass of S2DTdNet's MLP with every layer's output kept, the TD error and its
 * MSE / Huber derivative, the backward pass, the parameter gradients as per-block row-ascending fmaf chains summed in ascending
 * block order, the gradient norm over fixed chunks, the clip scale and Adam with its running beta products.  Written from the
 * spec, not from the kernels: plain loops over rows and units, one block of rows at a time.  relu / tanh_spec / sigmoid_spec are
 * wide_ref.c's, included as it stands.  TEST INFRASTRUCTURE: built on demand with gcc -O2 -ffp-contract=off (tests/learn.py). */
#include <stdlib.h>
#include <string.h>

#include "wide_ref.c"

#define LEARN_BLOCK_ROWS 64   /* S2D_LEARN_BLOCK_ROWS */
#define LEARN_NORM_CHUNK 256  /* S2D_LEARN_NORM_CHUNK */

typedef struct LearnNet {
  int32_t n_in, n_hidden, hidden[5], n_out, activation;
  float *params;
} LearnNet;

static int learn_width(const LearnNet *net, int l) { return l < net->n_hidden ? net->hidden[l] : net->n_out; }

int64_t learn_param_count(const LearnNet *net) {
  int64_t n = 0;
  int win = net->n_in;
  for (int l = 0; l <= net->n_hidden; ++l) {
    n += (int64_t)learn_width(net, l) * win + learn_width(net, l);
    win = learn_width(net, l);
  }
  return n;
}

/* one row: x[n_in] -> y[l] = the output of layer l (hidden: after the activation; last: linear), kept for the backward pass */
static void learn_row_forward(const LearnNet *net, const float *x, float **y) {
  const float *p = net->params, *in = x;
  int win = net->n_in, kk = (net->n_in + 3) / 4 * 4;
  for (int l = 0; l <= net->n_hidden; ++l) {
    const int w = learn_width(net, l), act = l < net->n_hidden ? net->activation : 3;
    const float *W = p, *b = p + w * win;
    for (int j = 0; j < w; ++j) {
      float acc = b[j];
      for (int i = 0; i < kk; ++i) {
        const volatile float wt = i < win ? W[j * win + i] : 0.0f, v = i < win ? in[i] : 0.0f;
        acc = fmaf(wt, v, acc);
      }
      y[l][j] = act == 0 ? relu(acc) : act == 1 ? tanh_spec(acc) : act == 2 ? sigmoid_spec(acc) : acc;
    }
    p += w * win + w;
    in = y[l]; win = w; kk = w;
  }
}

/* x[n][n_in] -> q[n][n_out] */
void learn_forward(int64_t n, const LearnNet *net, const float *x, float *q) {
  float buf[6][256], *y[6];
  for (int l = 0; l < 6; ++l) y[l] = buf[l];
  for (int64_t e = 0; e < n; ++e) {
    learn_row_forward(net, x + e * net->n_in, y);
    memcpy(q + e * net->n_out, y[net->n_hidden], sizeof(float) * net->n_out);
  }
}

/* the activation's derivative from its stored output, times s: separate, uncontracted operations */
static float learn_dact(int act, float y, float s) {
  if (act == 0) return y > 0.0f ? s : 0.0f;
  if (act == 1) {
    const volatile float t = y * y;
    const volatile float u = 1.0f - t;
    return s * u;
  }
  const volatile float u = 1.0f - y;
  const volatile float t = y * u;
  return s * t;
}

/* The summed gradient grad[P] (unclipped), stats = {mean loss, norm, scale}, td_abs[B] and out_q[B][n_out] where given; *error
 * |= 1 for an action outside [0, n_out).  loss_kind 0: MSE (loss e^2 / 2, derivative e), 1: Huber with delta 1. */
void learn_grad(int64_t B, const LearnNet *net, int loss_kind, const float *obs, const int32_t *action, const float *target,
                const float *weight, float max_grad_norm, float *grad, float *stats, float *td_abs, float *out_q, int32_t *error) {
  const int L = net->n_hidden, A = net->n_out, R = LEARN_BLOCK_ROWS;
  const int64_t P = learn_param_count(net), nb = (B + R - 1) / R;
  /* y[l][r][.]: layer l's output of row r of the block, later overwritten by its delta */
  float *store = (float *)malloc(sizeof(float) * R * 6 * 256), *y[6], *rowp[6];
  float *part = (float *)malloc(sizeof(float) * (size_t)P);
  for (int l = 0; l < 6; ++l) y[l] = store + (size_t)l * R * 256;
  float loss_sum = 0.0f;
  for (int64_t blk = 0; blk < nb; ++blk) {
    const int64_t row0 = blk * R;
    const int rows = (int)(B - row0 < R ? B - row0 : R);
    float loss_part = 0.0f;
    for (int r = 0; r < rows; ++r) {
      const int64_t b = row0 + r;
      for (int l = 0; l <= L; ++l) rowp[l] = y[l] + r * 256;
      learn_row_forward(net, obs + b * net->n_in, rowp);
      float *q = rowp[L];
      if (out_q) memcpy(out_q + b * A, q, sizeof(float) * A);
      const int32_t a = action[b];
      const int ok = a >= 0 && a < A;
      if (!ok) *error |= 1;
      const float e = ok ? q[a] - target[b] : 0.0f;
      if (td_abs) td_abs[b] = fabsf(e);
      const float w = weight ? weight[b] : 1.0f;
      const volatile float half = 0.5f * e;
      const float sq = half * e, ab = fabsf(e);
      const float l1 = loss_kind == 0 ? sq : (ab <= 1.0f ? sq : ab - 0.5f);
      const float d = loss_kind == 0 ? e : (e < -1.0f ? -1.0f : (e > 1.0f ? 1.0f : e));
      const volatile float wl = w * l1, wd = w * d;
      loss_part = loss_part + (ok ? wl : 0.0f);
      const float g = wd / (float)B;
      for (int j = 0; j < A; ++j) q[j] = (ok && j == a) ? g : 0.0f;
    }
    /* backward, layer L down to 0: this block's parameter gradients (rows ascending), then the delta of the layer below */
    int64_t off = P;
    for (int l = L; l >= 0; --l) {
      const int w = learn_width(net, l), win = l ? learn_width(net, l - 1) : net->n_in;
      off -= (int64_t)w * win + w;
      const float *W = net->params + off;
      for (int j = 0; j < w; ++j) {
        for (int k = 0; k < win; ++k) {
          float acc = 0.0f;
          for (int r = 0; r < rows; ++r) {
            const float in = l ? y[l - 1][r * 256 + k] : obs[(row0 + r) * net->n_in + k];
            acc = fmaf(y[l][r * 256 + j], in, acc);
          }
          part[off + j * win + k] = acc;
        }
        float acc = 0.0f;
        for (int r = 0; r < rows; ++r) acc = fmaf(y[l][r * 256 + j], 1.0f, acc);
        part[off + (int64_t)w * win + j] = acc;
      }
      if (l)
        for (int r = 0; r < rows; ++r)
          for (int k = 0; k < win; ++k) {
            float s = 0.0f;
            for (int j = 0; j < w; ++j) s = fmaf(W[j * win + k], y[l][r * 256 + j], s);
            y[l - 1][r * 256 + k] = learn_dact(net->activation, y[l - 1][r * 256 + k], s);
          }
    }
    /* block partials in ascending block order, plain adds; the first block starts the sums */
    for (int64_t p = 0; p < P; ++p) grad[p] = blk ? grad[p] + part[p] : part[p];
    loss_sum = blk ? loss_sum + loss_part : loss_part;
  }
  /* the norm: chunks of LEARN_NORM_CHUNK words, fmaf(g, g, .) ascending from +0 within a chunk, chunks added ascending */
  float ss = 0.0f;
  for (int64_t c = 0; c * LEARN_NORM_CHUNK < P; ++c) {
    float s = 0.0f;
    for (int64_t p = c * LEARN_NORM_CHUNK; p < P && p < (c + 1) * LEARN_NORM_CHUNK; ++p) s = fmaf(grad[p], grad[p], s);
    ss = c ? ss + s : s;
  }
  const float norm = sqrtf(ss);
  float scale = 1.0f;
  if (max_grad_norm > 0.0f) {
    const volatile float den = norm + 1e-6f;
    const float c = max_grad_norm / den;
    scale = c < 1.0f ? c : 1.0f;
  }
  stats[0] = loss_sum / (float)B;
  stats[1] = norm;
  stats[2] = scale;
  free(part);
  free(store);
}

/* Adam on g' = g * scale; hyper = {lr, beta1, beta2, eps, max_grad_norm, beta1^t, beta2^t}: the products are multiplied first */
void learn_adam(int64_t P, float *params, float *m, float *v, const float *grad, float *hyper, float scale) {
  const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3];
  const volatile float b1t = hyper[5] * b1, b2t = hyper[6] * b2;
  hyper[5] = b1t;
  hyper[6] = b2t;
  const volatile float omb1 = 1.0f - b1, omb2 = 1.0f - b2, bc1 = 1.0f - b1t, bc2 = 1.0f - b2t;
  const volatile float bc2s = sqrtf(bc2), step = lr / bc1;
  for (int64_t p = 0; p < P; ++p) {
    const volatile float gp = grad[p] * scale;
    const volatile float dm = gp - m[p];
    const volatile float dm1 = dm * omb1;
    const float mn = m[p] + dm1;
    const volatile float v1 = v[p] * b2, g1 = omb2 * gp;
    const volatile float g2 = g1 * gp;
    const float vn = v1 + g2;
    const volatile float sv = sqrtf(vn);
    const volatile float q = sv / bc2s;
    const volatile float den = q + eps;
    const volatile float r = mn / den;
    const volatile float up = step * r;
    m[p] = mn;
    v[p] = vn;
    params[p] = params[p] - up;
  }
}

/* s2d_learn_q: the gradient of the current parameters, then Adam */
void learn_step(int64_t B, const LearnNet *net, int loss_kind, const float *obs, const int32_t *action, const float *target,
                const float *weight, float *m, float *v, float *grad, float *hyper, float *stats, float *td_abs, float *out_q,
                int32_t *error) {
  learn_grad(B, net, loss_kind, obs, action, target, weight, hyper[4], grad, stats, td_abs, out_q, error);
  learn_adam(learn_param_count(net), net->params, m, v, grad, hyper, stats[2]);
}
