/* actor_ref.c -- host restatement of the fused tanh actor's policy (include/s2d.h s2d_rollout_actor; DESIGN.md sections 4, 5):
 * the forward pass (fmaf chains from the bias in ascending k, relu v > 0 ? v : +0), tanh_spec, log_spec, the Box-Muller draw
 * of the Gaussian action noise, clip, epsilon exploration and the random action.  Every fp32 operation in the order the
 * device code fixes.  TEST INFRASTRUCTURE: built on demand with gcc -O2 -ffp-contract=off (tests/actor_ref.py). */
#include <math.h>
#include <stdint.h>

static float relu(float v) { return v > 0.0f ? v : 0.0f; }

static void dense(const float *W, const float *b, const float *in, int m, int k, int use_relu, float *out) {
  for (int j = 0; j < m; ++j) {
    float acc = b[j];
    for (int i = 0; i < k; ++i) acc = fmaf(W[j * k + i], in[i], acc);
    out[j] = use_relu ? relu(acc) : acc;
  }
}

/* x[n][10], params in nn.Sequential order -> pre-activations y[n][na] */
void actor_forward(int64_t n, const float *x, const float *params, int h1, int h2, int na, float *y) {
  const float *W1 = params, *b1 = W1 + 10 * h1, *W2 = b1 + h1, *b2 = W2 + h2 * h1, *W3 = b2 + h2, *b3 = W3 + na * h2;
  float a1[128], a2[128];
  for (int64_t e = 0; e < n; ++e) {
    dense(W1, b1, x + 10 * e, h1, 10, 1, a1);
    dense(W2, b2, a1, h2, h1, 1, a2);
    dense(W3, b3, a2, na, h2, 0, y + na * e);
  }
}

static float exp_spec(float x) {
  float k = rintf(x * 1.44269504088896341f);
  float r = fmaf(-k, 0.693359375f, x);
  r = fmaf(-k, -2.12194440e-4f, r);
  float z = r * r;
  float p = 1.9875691500e-4f;
  p = fmaf(p, r, 1.3981999507e-3f);
  p = fmaf(p, r, 8.3334519073e-3f);
  p = fmaf(p, r, 4.1665795894e-2f);
  p = fmaf(p, r, 1.6666665459e-1f);
  p = fmaf(p, r, 5.0000001201e-1f);
  float y = fmaf(p, z, r) + 1.0f;
  return ldexpf(y, (int)k);
}

float tanh_spec(float y) {
  const float a = fabsf(y);
  if (a != a) return y;
  if (a > 9.0f) return copysignf(1.0f, y);
  float r;
  if (a < 0.625f) {
    const float z = a * a;
    float p = -5.70498872745e-3f;
    p = fmaf(p, z, 2.06390887954e-2f);
    p = fmaf(p, z, -5.37397155531e-2f);
    p = fmaf(p, z, 1.33314422036e-1f);
    p = fmaf(p, z, -3.33332819422e-1f);
    r = fmaf(z * p, a, a);
  } else {
    r = 1.0f - 2.0f / (exp_spec(a + a) + 1.0f);
  }
  return copysignf(r, y);
}

float log_spec(float v) {
  if (v != v || v < 0.0f) return NAN;
  if (v == 0.0f) return -INFINITY;
  if (v == INFINITY) return v;
  int e;
  float m = frexpf(v, &e);
  float x;
  if (m < 0.70710678118654752f) { e -= 1; x = (m + m) - 1.0f; } else { x = m - 1.0f; }
  const float z = x * x;
  float p = 7.0376836292e-2f;
  p = fmaf(p, x, -1.1514610310e-1f);
  p = fmaf(p, x, 1.1676998740e-1f);
  p = fmaf(p, x, -1.2420140846e-1f);
  p = fmaf(p, x, 1.4249322787e-1f);
  p = fmaf(p, x, -1.6668057665e-1f);
  p = fmaf(p, x, 2.0000714765e-1f);
  p = fmaf(p, x, -2.4999993993e-1f);
  p = fmaf(p, x, 3.3333331174e-1f);
  const float fe = (float)e;
  float y = (p * x) * z;
  y = fmaf(fe, -2.12194440e-4f, y);
  y = fmaf(-0.5f, z, y);
  return fmaf(fe, 0.693359375f, x + y);
}

static void sincos_deg(float deg, float *s, float *c) {
  float q = rintf(deg * 0.011111111111111112f);
  float r = fmaf(-q, 90.0f, deg);
  float x = r * 0.017453292519943295f;
  float z = x * x;
  float ps = fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f);
  ps = fmaf(z, ps, -1.6666654611e-1f);
  ps = fmaf(x * z, ps, x);
  float pc = fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f);
  pc = fmaf(z, pc, 4.166664568298827e-2f);
  pc = fmaf(z * z, pc, fmaf(-0.5f, z, 1.0f));
  int n = ((int)q) & 3;
  float ss = (n & 1) ? pc : ps;
  float cc = (n & 1) ? ps : pc;
  *s = (n & 2) ? -ss : ss;
  *c = ((n + 1) & 2) ? -cc : cc;
}

static void box_muller(uint32_t wa, uint32_t wb, float *zc, float *zs) {
  const float u1 = (float)((wa >> 8) + 1u) * 5.9604644775390625e-8f;
  const float r = sqrtf(-2.0f * log_spec(u1));
  float s, c;
  sincos_deg((float)(wb >> 8) * 2.1457672119140625e-5f, &s, &c);
  *zc = r * c; *zs = r * s;
}

static void philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}
/* Philox block `block` of stream POLICY (1) at `ctr` for global env id gid */
static void policy_block(uint64_t seed, uint64_t gid, uint32_t ctr, uint32_t block, uint32_t w[4]) {
  w[0] = (uint32_t)gid; w[1] = (uint32_t)(gid >> 32); w[2] = ctr; w[3] = (1u << 16) | block;
  philox(w, (uint32_t)seed, (uint32_t)(seed >> 32));
}

/* the Gaussian block (z0..z3) of n (gid, counter) pairs */
void actor_gauss(int64_t n, uint64_t seed, const uint64_t *gid, const uint32_t *ctr, float *z) {
  for (int64_t e = 0; e < n; ++e) {
    uint32_t w[4];
    policy_block(seed, gid[e], ctr[e], 3, w);
    box_muller(w[0], w[1], z + 4 * e, z + 4 * e + 1);
    box_muller(w[2], w[3], z + 4 * e + 2, z + 4 * e + 3);
  }
}

void actor_tanh(int64_t n, const float *in, float *out) { for (int64_t i = 0; i < n; ++i) out[i] = tanh_spec(in[i]); }
void actor_log(int64_t n, const float *in, float *out) { for (int64_t i = 0; i < n; ++i) out[i] = log_spec(in[i]); }

static uint64_t threshold(float eps) {
  if (eps >= 1.0f) return 1ull << 32;
  if (eps > 0.0f) return (uint64_t)(eps * 4294967296.0f);
  return 0;
}
static float rnd_pm1(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-8f * 2.0f - 1.0f; }

/* the actor's action of n envs (global ids gid0 + e) at policy steps k[e]: na = 1 (continuous) or 4 (turning); kind 0 / 1
 * (no / Gaussian action noise, noise = [2][na] mu, sigma); y_scratch[n][na]; out[n][na] */
void actor_actions(int64_t n, const float *x, const float *params, int h1, int h2, int na, float eps, int kind,
                   const float *noise, uint64_t seed, uint64_t gid0, const uint32_t *k, float *y_scratch, float *out) {
  actor_forward(n, x, params, h1, h2, na, y_scratch);
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
      float v = tanh_spec(y_scratch[na * e + j]);
      if (kind == 1) {
        v = v + fmaf(noise[na + j], z[j], noise[j]);
        v = v < -1.0f ? -1.0f : v > 1.0f ? 1.0f : v;
      }
      a[j] = v;
    }
  }
}
