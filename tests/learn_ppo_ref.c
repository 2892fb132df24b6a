/* learn_ppo_ref.c -- host restatement of the fused PPO update (include/s2d.h S2DLearnPPO / S2DLearnPPOBatch, s2d_learn_ppo /
 * s2d_learn_ppo_grad): the advantage pre-pass, both forward passes, the categorical and the Gaussian head, the
 * clipped surrogate, the value error, the output deltas, both backward passes with the row sums grouped as the header says, the
 * log_std terms, the norm over the combined buffer, the clip scale, the eight statistics and Adam.  Written from the spec, not from
 * the kernels: plain loops over rows and units.  The forward chain, the activation derivatives and Adam are learn_ref.c's, exp_spec /
 * log_spec actor_ref.c's, included as they stand.  TEST INFRASTRUCTURE: built on demand with gcc -O2 -ffp-contract=off
 * (tests/learn_ppo.py). */
#include "learn_ref.c"

#define PPO_MAX_GROUPS 256 /* S2D_LEARN_PPO_MAX_GROUPS */
#define PPO_W 256          /* words kept per layer and row */

typedef struct PpoCall {
  int32_t head, normalize; /* 0 categorical / 1 Gaussian; normalize_advantage */
  int64_t R, B;
  const float *obs;
  const void *action;
  const float *logp_old, *adv, *ret;
  const int32_t *index;    /* or NULL */
} PpoCall;

int64_t ppo_param_count(const LearnNet *pi, const LearnNet *vf, int head) {
  return learn_param_count(pi) + learn_param_count(vf) + (head ? pi->n_out : 0);
}

/* blocks a group: a function of B alone */
int64_t ppo_blocks_per_group(int64_t B) {
  const int64_t blocks = (B + LEARN_BLOCK_ROWS - 1) / LEARN_BLOCK_ROWS;
  return (blocks + PPO_MAX_GROUPS - 1) / PPO_MAX_GROUPS;
}

static int64_t ppo_source(const PpoCall *c, int64_t b) {
  const int64_t i = c->index ? (int64_t)c->index[b] : b;
  return i >= 0 && i < c->R ? i : -1;
}

/* the pre-pass: mean and unbiased standard deviation of the advantages the minibatch names, by blocks of 64 rows */
void ppo_advantage_stats(const PpoCall *c, float *mean_out, float *std_out) {
  const int64_t blocks = (c->B + LEARN_BLOCK_ROWS - 1) / LEARN_BLOCK_ROWS;
  float mean = 0.0f, total = 0.0f;
  for (int pass = 0; pass < 2; ++pass) {
    for (int64_t blk = 0; blk < blocks; ++blk) {
      float s = 0.0f;
      for (int64_t b = blk * LEARN_BLOCK_ROWS; b < c->B && b < (blk + 1) * LEARN_BLOCK_ROWS; ++b) {
        const int64_t i = ppo_source(c, b);
        if (i < 0) continue;
        if (pass) {
          const float d = c->adv[i] - mean;
          s = fmaf(d, d, s);
        } else {
          s = s + c->adv[i];
        }
      }
      total = blk ? total + s : s;
    }
    if (pass == 0) mean = total / (float)c->B;
  }
  *mean_out = mean;
  *std_out = sqrtf(total / (float)(c->B - 1));
}

/* One block's backward pass of one network from the output deltas in y[L] (layer l's input is y[l - 1]; x, D words a row, for l = 0).
 * Every dW / db chain starts at +0 where `first`, else goes on from part[]. */
static void ppo_backward(const LearnNet *net, int rows, const float *x, float **y, float *part, int first) {
  int64_t off = learn_param_count(net);
  for (int l = net->n_hidden; l >= 0; --l) {
    const int w = learn_width(net, l), win = l ? learn_width(net, l - 1) : net->n_in;
    off -= (int64_t)w * win + w;
    const float *W = net->params + off;
    for (int j = 0; j < w; ++j) {
      for (int k = 0; k < win; ++k) {
        float acc = first ? 0.0f : part[off + j * win + k];
        for (int r = 0; r < rows; ++r) acc = fmaf(y[l][r * PPO_W + j], l ? y[l - 1][r * PPO_W + k] : x[r * net->n_in + k], acc);
        part[off + j * win + k] = acc;
      }
      float acc = first ? 0.0f : part[off + (int64_t)w * win + j];
      for (int r = 0; r < rows; ++r) acc = fmaf(y[l][r * PPO_W + j], 1.0f, acc);
      part[off + (int64_t)w * win + j] = acc;
    }
    if (l)
      for (int r = 0; r < rows; ++r)
        for (int k = 0; k < win; ++k) {
          float s = 0.0f;
          for (int j = 0; j < w; ++j) s = fmaf(W[j * win + k], y[l][r * PPO_W + j], s);
          y[l - 1][r * PPO_W + k] = learn_dact(net->activation, y[l - 1][r * PPO_W + k], s);
        }
  }
}

typedef struct PpoStore {
  float *mem, *y[6], *rowp[6];
} PpoStore;
static void ppo_store(PpoStore *s) {
  s->mem = (float *)malloc(sizeof(float) * LEARN_BLOCK_ROWS * 6 * PPO_W);
  for (int l = 0; l < 6; ++l) s->y[l] = s->mem + (size_t)l * LEARN_BLOCK_ROWS * PPO_W;
}
static void ppo_row(PpoStore *s, int r) {
  for (int l = 0; l < 6; ++l) s->rowp[l] = s->y[l] + r * PPO_W;
}

/* s2d_learn_ppo_grad.  pi->params, vf->params and log_std are the three parts of the flat buffer; hyper[10]; grad[P] (unclipped),
 * stats[8], out_logp[B] and out_value[B] where given, *error |= 1 (action) | 2 (index). */
void ppo_grad(const LearnNet *pi, const LearnNet *vf, const float *log_std, const PpoCall *c, const float *hyper, float *grad,
              float *stats, float *out_logp, float *out_value, int32_t *error) {
  const int Lp = pi->n_hidden, Lv = vf->n_hidden, A = pi->n_out, D = pi->n_in, RB = LEARN_BLOCK_ROWS;
  const int64_t Ppi = learn_param_count(pi), Pvf = learn_param_count(vf), P = ppo_param_count(pi, vf, c->head), B = c->B;
  const int64_t blocks = (B + RB - 1) / RB, G = ppo_blocks_per_group(B), groups = (blocks + G - 1) / G;
  const float clip = hyper[7], vf_coef = hyper[8], ent_coef = hyper[9], fB = (float)B;
  const float lo = 1.0f - clip, hi = 1.0f + clip;
  const int normalize = c->normalize && B > 1;
  float mean = 0.0f, std = 0.0f;
  if (normalize) ppo_advantage_stats(c, &mean, &std);
  PpoStore sp, sv;
  ppo_store(&sp);
  ppo_store(&sv);
  float *x = (float *)malloc(sizeof(float) * RB * D), *lsd = (float *)malloc(sizeof(float) * RB * 8);
  float *part = (float *)malloc(sizeof(float) * (size_t)P);
  float total[5] = {0, 0, 0, 0, 0};
  for (int64_t g = 0; g < groups; ++g) {
    float st[5] = {0, 0, 0, 0, 0};
    for (int64_t blk = g * G; blk < blocks && blk < (g + 1) * G; ++blk) {
      const int64_t row0 = blk * RB;
      const int rows = (int)(B - row0 < RB ? B - row0 : RB), first = blk == g * G;
      for (int r = 0; r < rows; ++r) {
        const int64_t b = row0 + r, s = ppo_source(c, b);
        int live = s >= 0;
        if (!live) *error |= 2;
        for (int k = 0; k < D; ++k) x[r * D + k] = live ? c->obs[s * D + k] : 0.0f;
        ppo_row(&sp, r);
        ppo_row(&sv, r);
        learn_row_forward(pi, x + r * D, sp.rowp);
        learn_row_forward(vf, x + r * D, sv.rowp);
        float *y = sp.rowp[Lp], *vq = sv.rowp[Lv];
        int a = 0;
        if (live && c->head == 0) {
          a = ((const int32_t *)c->action)[s];
          if (a < 0 || a >= A) {
            *error |= 1;
            live = 0;
          }
        }
        if (!live) {                                   /* a dropped row: nothing */
          for (int j = 0; j < A; ++j) y[j] = lsd[r * 8 + (j & 7)] = 0.0f;
          vq[0] = 0.0f;
          if (out_logp) out_logp[b] = 0.0f;
          if (out_value) out_value[b] = 0.0f;
          continue;
        }
        float logp = 0.0f, H, m = 0.0f, S = 0.0f, logS = 0.0f;
        if (c->head == 0) {
          m = y[0];
          for (int j = 1; j < A; ++j) if (y[j] > m) m = y[j];
          S = exp_spec(y[0] - m);
          for (int j = 1; j < A; ++j) S += exp_spec(y[j] - m);
          logS = log_spec(S);
          logp = (y[a] - m) - logS;
          float h = 0.0f;
          for (int j = 0; j < A; ++j) {
            const float p = exp_spec(y[j] - m) / S, lp = (y[j] - m) - logS;
            h = fmaf(p, lp, h);
          }
          H = -h;
        } else {
          const float *act = (const float *)c->action + s * A;
          float hs = 0.0f;
          for (int j = 0; j < A; ++j) {
            const float ls = log_std[j], z = (act[j] - y[j]) / exp_spec(ls);
            const float half = -0.5f * z;
            const float term = fmaf(half, z, -ls) - 0.91893853f;
            logp = j ? logp + term : term;
            hs = j ? hs + ls : ls;
          }
          const float c0 = (float)A * 1.4189385f;
          H = hs + c0;
        }
        float adv = c->adv[s];
        if (normalize) {
          const float den = std + 1e-8f;
          adv = (adv - mean) / den;
        }
        const float d = logp - c->logp_old[s], ratio = exp_spec(d);
        const float rc = ratio < lo ? lo : (ratio > hi ? hi : ratio);
        const float s1 = ratio * adv, s2 = rc * adv;
        const float mn = (s1 < s2 || s1 != s1) ? s1 : s2;
        const int clipped = (ratio > hi && adv > 0.0f) || (ratio < lo && adv < 0.0f);
        const float gl = clipped ? 0.0f : -s1;
        const float v = vq[0], e = v - c->ret[s];
        const float rm1 = ratio - 1.0f;
        const float rowstat[5] = {-mn, e * e, H, rm1 - d, fabsf(rm1) > clip ? 1.0f : 0.0f};
        for (int k = 0; k < 5; ++k) st[k] = st[k] + rowstat[k];
        if (out_logp) out_logp[b] = logp;
        if (out_value) out_value[b] = v;
        const float e2 = 2.0f * e;
        const float ve = vf_coef * e2;
        vq[0] = ve / fB;
        if (c->head == 0) {
          for (int j = 0; j < A; ++j) {
            const float p = exp_spec(y[j] - m) / S, lp = (y[j] - m) - logS;
            const float ind = (j == a ? 1.0f : 0.0f) - p, ep = ent_coef * p, lh = lp + H;
            const float t1 = gl * ind, t2 = ep * lh;
            const float t = t1 + t2;
            y[j] = t / fB;
          }
        } else {
          const float *act = (const float *)c->action + s * A;
          for (int j = 0; j < A; ++j) {
            const float sg = exp_spec(log_std[j]), z = (act[j] - y[j]) / sg;
            const float gz = gl * z, zz = z * z;
            const float q = gz / sg, zz1 = zz - 1.0f;
            const float gq = gl * zz1;
            y[j] = q / fB;
            lsd[r * 8 + j] = gq / fB;
          }
        }
      }
      ppo_backward(pi, rows, x, sp.y, part, first);
      ppo_backward(vf, rows, x, sv.y, part + Ppi, first);
      if (c->head)
        for (int j = 0; j < A; ++j) {
          float acc = first ? 0.0f : part[Ppi + Pvf + j];
          for (int r = 0; r < rows; ++r) acc = fmaf(lsd[r * 8 + j], 1.0f, acc);
          part[Ppi + Pvf + j] = acc;
        }
    }
    for (int64_t p = 0; p < P; ++p) grad[p] = g ? grad[p] + part[p] : part[p];
    for (int k = 0; k < 5; ++k) total[k] = g ? total[k] + st[k] : st[k];
  }
  if (c->head)
    for (int j = 0; j < A; ++j) grad[Ppi + Pvf + j] = grad[Ppi + Pvf + j] - ent_coef;
  /* norm over chunks of LEARN_NORM_CHUNK words of the whole buffer, the clip scale */
  float ss = 0.0f;
  for (int64_t ch = 0; ch * LEARN_NORM_CHUNK < P; ++ch) {
    float s = 0.0f;
    for (int64_t p = ch * LEARN_NORM_CHUNK; p < P && p < (ch + 1) * LEARN_NORM_CHUNK; ++p) s = fmaf(grad[p], grad[p], s);
    ss = ch ? ss + s : s;
  }
  const float norm = sqrtf(ss);
  float scale = 1.0f;
  if (hyper[4] > 0.0f) {
    const float den = norm + 1e-6f;
    const float q = hyper[4] / den;
    scale = q < 1.0f ? q : 1.0f;
  }
  for (int k = 0; k < 5; ++k) stats[3 + k] = total[k] / fB;
  const float vl = vf_coef * stats[4], el = ent_coef * stats[5];
  const float pv = stats[3] + vl;
  stats[0] = pv - el;
  stats[1] = norm;
  stats[2] = scale;
  free(part);
  free(lsd);
  free(x);
  free(sp.mem);
  free(sv.mem);
}

/* s2d_learn_ppo: the gradient of the current parameters, then learn_ref.c's Adam over the whole flat buffer (flat == pi->params) */
void ppo_step(const LearnNet *pi, const LearnNet *vf, const float *log_std, const PpoCall *c, float *flat, float *m, float *v, float *grad,
              float *hyper, float *stats, float *out_logp, float *out_value, int32_t *error) {
  ppo_grad(pi, vf, log_std, c, hyper, grad, stats, out_logp, out_value, error);
  learn_adam(ppo_param_count(pi, vf, c->head), flat, m, v, grad, hyper, stats[2]);
}
