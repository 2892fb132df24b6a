/* gtc_actor_ref.c -- host restatement of the GoToCenter fused actors (include/s2d_gtc.h s2d_gtc_rollout_qnet / s2d_gtc_rollout_actor;
 * DESIGN.md sections 4, 5): the 4 -> h_1 -> ... -> h_L -> A network (every unit an fmaf chain from its bias in ascending k; layer 1
 * over exactly k = 0 .. 3, no zero pad; relu, tanh_spec or sigmoid_spec between the layers; linear output), Philox with the
 * GoToCenter keys (gid, episode, (stream << 16) | step_count), the exploration threshold and both heads.  Written from the spec,
 * not from the kernel: plain loops over units, no tiles, no fragments.  exp_spec, tanh_spec, log_spec, box_muller and philox are
 * actor_ref.c's, sigmoid_spec and the dense layer wide_ref.c's, included as they stand.  TEST INFRASTRUCTURE: built on demand with
 * gcc -O2 -ffp-contract=off (tests/gtc_actor_ref.py). */
#include "wide_ref.c"

enum { GST_POLICY = 1, GST_EXPLORE = 9, GST_GAUSS = 10 };

/* x[n][4], params in nn.Sequential order, hidden[n_hidden], activation 0 / 1 / 2 -> y[n][na] */
void gtc_forward(int64_t n, const float *x, const float *params, int n_hidden, const int32_t *hidden, int na, int activation, float *y) {
  float a[2][400];
  for (int64_t e = 0; e < n; ++e) {
    const float *p = params, *in = x + 4 * e;
    int win = 4, cur = 0;
    for (int l = 0; l < n_hidden; ++l) {
      const int w = hidden[l];
      wide_dense(p, p + w * win, in, w, win, win, activation, a[cur]);
      p += w * win + w;
      in = a[cur]; cur ^= 1; win = w;
    }
    wide_dense(p, p + na * win, in, na, win, win, 3, y + na * e);
  }
}

static void gtc_block(uint64_t seed, uint64_t gid, uint32_t episode, uint32_t stream, uint32_t step, uint32_t w[4]) {
  w[0] = (uint32_t)gid; w[1] = (uint32_t)(gid >> 32); w[2] = episode; w[3] = (stream << 16) | step;
  philox(w, (uint32_t)seed, (uint32_t)(seed >> 32));
}

uint64_t gtc_threshold(float eps) { return threshold(eps); }

/* word x of stream 9 of n (gid0 + e, episode[e], step[e]) keys */
void gtc_explore_words(int64_t n, uint64_t seed, uint64_t gid0, const int32_t *episode, const int32_t *step, uint32_t *out) {
  for (int64_t e = 0; e < n; ++e) {
    uint32_t w[4];
    gtc_block(seed, gid0 + (uint64_t)e, (uint32_t)episode[e], GST_EXPLORE, (uint32_t)step[e], w);
    out[e] = w[0];
  }
}

/* z0 .. z3 of stream 10 */
void gtc_gauss(int64_t n, uint64_t seed, uint64_t gid0, const int32_t *episode, const int32_t *step, float *z) {
  for (int64_t e = 0; e < n; ++e) {
    uint32_t w[4];
    gtc_block(seed, gid0 + (uint64_t)e, (uint32_t)episode[e], GST_GAUSS, (uint32_t)step[e], w);
    box_muller(w[0], w[1], z + 4 * e, z + 4 * e + 1);
    box_muller(w[2], w[3], z + 4 * e + 2, z + 4 * e + 3);
  }
}

/* best = 0; for a = 1 .. na - 1: if (y[a] > y[best]) best = a */
void gtc_argmax(int64_t n, const float *y, int na, int32_t *out) {
  for (int64_t e = 0; e < n; ++e) {
    int best = 0;
    for (int a = 1; a < na; ++a) if (y[na * e + a] > y[na * e + best]) best = a;
    out[e] = best;
  }
}

/* the Q head: y[n][na] -> action[n]; explored[n] (may be NULL) says which envs explored */
void gtc_q_actions(int64_t n, const float *y, int na, float eps, uint64_t seed, uint64_t gid0, const int32_t *episode,
                   const int32_t *step, int32_t *out, uint8_t *explored) {
  const uint64_t thr = threshold(eps);
  gtc_argmax(n, y, na, out);
  for (int64_t e = 0; e < n; ++e) {
    uint32_t w[4];
    gtc_block(seed, gid0 + (uint64_t)e, (uint32_t)episode[e], GST_EXPLORE, (uint32_t)step[e], w);
    const int ex = (uint64_t)w[0] < thr;
    if (explored) explored[e] = (uint8_t)ex;
    if (!ex) continue;
    gtc_block(seed, gid0 + (uint64_t)e, (uint32_t)episode[e], GST_POLICY, (uint32_t)step[e], w);
    out[e] = (int32_t)(((uint64_t)w[0] * 16u) >> 32);
  }
}

/* the tanh head: y[n][na] (na = the action width, 1 .. 4) -> out[n][na]; kind 0 / 1, noise = [2][na] (mu, sigma) */
void gtc_actor_actions(int64_t n, const float *y, int na, float eps, int kind, const float *noise, uint64_t seed, uint64_t gid0,
                       const int32_t *episode, const int32_t *step, float *out, uint8_t *explored) {
  const uint64_t thr = threshold(eps);
  for (int64_t e = 0; e < n; ++e) {
    const uint64_t gid = gid0 + (uint64_t)e;
    uint32_t w[4];
    float *a = out + na * e;
    gtc_block(seed, gid, (uint32_t)episode[e], GST_EXPLORE, (uint32_t)step[e], w);
    const int ex = (uint64_t)w[0] < thr;
    if (explored) explored[e] = (uint8_t)ex;
    if (ex) {
      gtc_block(seed, gid, (uint32_t)episode[e], GST_POLICY, (uint32_t)step[e], w);
      for (int j = 0; j < na; ++j) a[j] = rnd_pm1(w[j]);
      continue;
    }
    float z[4] = {0, 0, 0, 0};
    if (kind == 1) {
      gtc_block(seed, gid, (uint32_t)episode[e], GST_GAUSS, (uint32_t)step[e], w);
      box_muller(w[0], w[1], &z[0], &z[1]);
      box_muller(w[2], w[3], &z[2], &z[3]);
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
