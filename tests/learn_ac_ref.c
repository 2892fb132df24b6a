/* learn_ac_ref.c -- host restatement of the fused DDPG / TD3 update (include/s2d.h s2d_learn_critic / s2d_learn_critic_grad,
 * s2d_learn_actor / s2d_learn_actor_grad): the critic's step on the row [obs | action] with the MSE, Huber and
 * square losses, and the actor's step on loss = -mean Q(obs, tanh(mu(obs))) -- actor forward, tanh head, critic forward, the critic's
 * deltas down to the action columns of its input (its parameter gradients are never formed: there is no array to hold them), the
 * head's derivative, the actor's backward pass.  Written from the spec, not from the kernels: plain loops over rows and units, one
 * block of rows at a time.  The forward chain, the activation derivatives and Adam are learn_ref.c's, included as it stands.
 * TEST INFRASTRUCTURE: built on demand with gcc -O2 -ffp-contract=off (tests/learn_ac.py). */
#include "learn_ref.c"

#define AC_W 256 /* words kept per layer and row */

/* One block's backward pass from the output layer's deltas in y[L]: layer l's input is y[l - 1] (x, `xs` words a row, for l = 0).
 * part != NULL: dW and db of every layer, rows ascending.  Every hidden layer's delta overwrites its stored output.  part == NULL:
 * deltas only, and the pass ends with layer 1's delta in y[0]. */
static void ac_backward(const LearnNet *net, int rows, const float *x, int xs, float **y, float *part) {
  int64_t off = learn_param_count(net);
  for (int l = net->n_hidden; l >= 0; --l) {
    const int w = learn_width(net, l), win = l ? learn_width(net, l - 1) : net->n_in;
    off -= (int64_t)w * win + w;
    const float *W = net->params + off;
    if (part)
      for (int j = 0; j < w; ++j) {
        for (int k = 0; k < win; ++k) {
          float acc = 0.0f;
          for (int r = 0; r < rows; ++r) acc = fmaf(y[l][r * AC_W + j], l ? y[l - 1][r * AC_W + k] : x[r * xs + k], acc);
          part[off + j * win + k] = acc;
        }
        float acc = 0.0f;
        for (int r = 0; r < rows; ++r) acc = fmaf(y[l][r * AC_W + j], 1.0f, acc);
        part[off + (int64_t)w * win + j] = acc;
      }
    if (l)
      for (int r = 0; r < rows; ++r)
        for (int k = 0; k < win; ++k) {
          float s = 0.0f;
          for (int j = 0; j < w; ++j) s = fmaf(W[j * win + k], y[l][r * AC_W + j], s);
          y[l - 1][r * AC_W + k] = learn_dact(net->activation, y[l - 1][r * AC_W + k], s);
        }
  }
}

/* stats[1] = the norm over chunks of LEARN_NORM_CHUNK words, stats[2] = the clip scale */
static void ac_norm_clip(int64_t P, const float *grad, float max_grad_norm, float *stats) {
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
  stats[1] = norm;
  stats[2] = scale;
}

typedef struct AcStore {
  float *mem, *y[6], *rowp[6];
} AcStore;
static void ac_store(AcStore *s) {
  s->mem = (float *)malloc(sizeof(float) * LEARN_BLOCK_ROWS * 6 * AC_W);
  for (int l = 0; l < 6; ++l) s->y[l] = s->mem + (size_t)l * LEARN_BLOCK_ROWS * AC_W;
}
static void ac_row(AcStore *s, int r) {
  for (int l = 0; l < 6; ++l) s->rowp[l] = s->y[l] + r * AC_W;
}

/* s2d_learn_critic_grad: net->n_in == D + A, net->n_out == 1.  loss_kind 0: e^2 / 2 and d = e, 1: Huber with delta 1, 2: e * e and
 * d = 2 e.  grad[P] (unclipped), stats = {mean loss, norm, scale}, td_abs[B] and out_q[B] where given. */
void learn_ac_critic_grad(int64_t B, const LearnNet *net, int A, int loss_kind, const float *obs, const float *action, const float *target,
                          const float *weight, float max_grad_norm, float *grad, float *stats, float *td_abs, float *out_q) {
  const int L = net->n_hidden, R = LEARN_BLOCK_ROWS, N = net->n_in, D = N - A;
  const int64_t P = learn_param_count(net), nb = (B + R - 1) / R;
  AcStore s;
  ac_store(&s);
  float *x = (float *)malloc(sizeof(float) * R * N), *part = (float *)malloc(sizeof(float) * (size_t)P);
  float loss_sum = 0.0f;
  for (int64_t blk = 0; blk < nb; ++blk) {
    const int64_t row0 = blk * R;
    const int rows = (int)(B - row0 < R ? B - row0 : R);
    float loss_part = 0.0f;
    for (int r = 0; r < rows; ++r) {
      const int64_t b = row0 + r;
      memcpy(x + r * N, obs + b * D, sizeof(float) * D);
      memcpy(x + r * N + D, action + b * A, sizeof(float) * A);
      ac_row(&s, r);
      learn_row_forward(net, x + r * N, s.rowp);
      float *q = s.rowp[L];
      if (out_q) out_q[b] = q[0];
      const float e = q[0] - target[b];
      if (td_abs) td_abs[b] = fabsf(e);
      const float w = weight ? weight[b] : 1.0f;
      const volatile float half = 0.5f * e, ee = e * e, two = 2.0f * e;
      const float sq = half * e, ab = fabsf(e);
      const float l1 = loss_kind == 2 ? ee : loss_kind == 0 ? sq : (ab <= 1.0f ? sq : ab - 0.5f);
      const float d = loss_kind == 2 ? two : loss_kind == 0 ? e : (e < -1.0f ? -1.0f : (e > 1.0f ? 1.0f : e));
      const volatile float wl = w * l1, wd = w * d;
      loss_part = loss_part + wl;
      q[0] = wd / (float)B;
    }
    ac_backward(net, rows, x, N, s.y, part);
    for (int64_t p = 0; p < P; ++p) grad[p] = blk ? grad[p] + part[p] : part[p];
    loss_sum = blk ? loss_sum + loss_part : loss_part;
  }
  stats[0] = loss_sum / (float)B;
  ac_norm_clip(P, grad, max_grad_norm, stats);
  free(part);
  free(x);
  free(s.mem);
}

/* s2d_learn_actor_grad: the ACTOR's grad[P_actor] (unclipped) of -mean_b critic([obs_b | tanh(actor(obs_b))])[0], stats = {-(sum of
 * q) / B, norm, scale}, out_action[B][A] and out_q[B] where given.  The critic's parameters are only read. */
void learn_ac_actor_grad(int64_t B, const LearnNet *actor, const LearnNet *critic, const float *obs, float max_grad_norm, float *grad,
                         float *stats, float *out_action, float *out_q) {
  const int La = actor->n_hidden, Lc = critic->n_hidden, R = LEARN_BLOCK_ROWS, D = actor->n_in, A = actor->n_out, N = critic->n_in;
  const int64_t P = learn_param_count(actor), nb = (B + R - 1) / R;
  const int h1 = learn_width(critic, 0);
  AcStore sa, sc;
  ac_store(&sa);
  ac_store(&sc);
  float *x = (float *)malloc(sizeof(float) * R * N), *part = (float *)malloc(sizeof(float) * (size_t)P);
  float q_sum = 0.0f;
  for (int64_t blk = 0; blk < nb; ++blk) {
    const int64_t row0 = blk * R;
    const int rows = (int)(B - row0 < R ? B - row0 : R);
    float q_part = 0.0f;
    for (int r = 0; r < rows; ++r) {
      const int64_t b = row0 + r;
      ac_row(&sa, r);
      ac_row(&sc, r);
      learn_row_forward(actor, obs + b * D, sa.rowp);
      memcpy(x + r * N, obs + b * D, sizeof(float) * D);
      for (int i = 0; i < A; ++i) {
        const float a = tanh_spec(sa.rowp[La][i]);
        sa.rowp[La][i] = a;
        x[r * N + D + i] = a;
        if (out_action) out_action[b * A + i] = a;
      }
      learn_row_forward(critic, x + r * N, sc.rowp);
      const float q = sc.rowp[Lc][0];
      if (out_q) out_q[b] = q;
      q_part = q_part + q;
      sc.rowp[Lc][0] = -1.0f / (float)B;
    }
    ac_backward(critic, rows, x, N, sc.y, NULL);
    /* the action columns of the critic's input delta, then the head: dz = s * (1 - a * a) */
    for (int r = 0; r < rows; ++r)
      for (int i = 0; i < A; ++i) {
        float sum = 0.0f;
        for (int j = 0; j < h1; ++j) sum = fmaf(critic->params[j * N + D + i], sc.y[0][r * AC_W + j], sum);
        sa.y[La][r * AC_W + i] = learn_dact(1, sa.y[La][r * AC_W + i], sum);
      }
    ac_backward(actor, rows, obs + row0 * D, D, sa.y, part);
    for (int64_t p = 0; p < P; ++p) grad[p] = blk ? grad[p] + part[p] : part[p];
    q_sum = blk ? q_sum + q_part : q_part;
  }
  stats[0] = -q_sum / (float)B;
  ac_norm_clip(P, grad, max_grad_norm, stats);
  free(part);
  free(x);
  free(sa.mem);
  free(sc.mem);
}

/* s2d_learn_critic / s2d_learn_actor: the gradient of the current parameters, then learn_ref.c's Adam on the stepped network */
void learn_ac_critic_step(int64_t B, const LearnNet *net, int A, int loss_kind, const float *obs, const float *action, const float *target,
                          const float *weight, float *m, float *v, float *grad, float *hyper, float *stats, float *td_abs, float *out_q) {
  learn_ac_critic_grad(B, net, A, loss_kind, obs, action, target, weight, hyper[4], grad, stats, td_abs, out_q);
  learn_adam(learn_param_count(net), net->params, m, v, grad, hyper, stats[2]);
}

void learn_ac_actor_step(int64_t B, const LearnNet *actor, const LearnNet *critic, const float *obs, float *m, float *v, float *grad,
                         float *hyper, float *stats, float *out_action, float *out_q) {
  learn_ac_actor_grad(B, actor, critic, obs, hyper[4], grad, stats, out_action, out_q);
  learn_adam(learn_param_count(actor), actor->params, m, v, grad, hyper, stats[2]);
}
