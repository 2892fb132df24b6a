/* match_policy_ref.c -- host restatement of the 11v11 engine's policy slots (include/s2d_match.h, "Policy slots"): the
 * 224-H1-H2-K forward pass with either hidden activation, the categorical head on word z of the slot's ST_NET block, logp and
 * the deterministic switch.  The relu forward is match_net_ref.c's, the head policy_ref.c's, exp_spec / log_spec / tanh_spec /
 * Philox actor_ref.c's: the three files are included as they are.  TEST INFRASTRUCTURE: built on demand with
 * gcc -O2 -ffp-contract=off (tests/match_policy.py). */
#define relu mnet_relu       /* (match_net_ref.c and actor_ref.c each have a static relu) */
#include "match_net_ref.c"
#undef relu
#include "policy_ref.c"

#define MP_ST_NET 7u

/* y[i][K] for n rows x[i][224]; act 0: relu (mnet_forward itself), 1: tanh_spec on both hidden layers */
void mpol_forward(int64_t n, const float *x, const float *params, int h1, int h2, int na, int act, float *y) {
  if (!act) { mnet_forward(n, x, params, h1, h2, na, y); return; }
  const float *w1 = params, *b1 = w1 + h1 * DIM, *w2 = b1 + h1, *b2 = w2 + h2 * h1, *w3 = b2 + h2, *b3 = w3 + na * h2;
  float ha[64], hb[64];
  for (int64_t i = 0; i < n; ++i) {
    for (int j = 0; j < h1; ++j) {
      float acc = b1[j];
      for (int k = 0; k < DIM; ++k) acc = fmaf(w1[j * DIM + k], x[i * DIM + k], acc);
      ha[j] = tanh_spec(acc);
    }
    for (int j = 0; j < h2; ++j) {
      float acc = b2[j];
      for (int k = 0; k < h1; ++k) acc = fmaf(w2[j * h1 + k], ha[k], acc);
      hb[j] = tanh_spec(acc);
    }
    for (int j = 0; j < na; ++j) {
      float acc = b3[j];
      for (int k = 0; k < h2; ++k) acc = fmaf(w3[j * h2 + k], hb[k], acc);
      y[i * na + j] = acc;
    }
  }
}

/* the slot's block: counter = the match's tick, stream ST_NET, block = the slot (the keys of every match draw) */
void mpol_block(uint64_t seed, uint64_t gid, uint32_t tick, uint32_t slot, uint32_t w[4]) {
  w[0] = (uint32_t)gid; w[1] = (uint32_t)(gid >> 32); w[2] = tick; w[3] = (MP_ST_NET << 16) | slot;
  philox(w, (uint32_t)seed, (uint32_t)(seed >> 32));
}

/* the head of n rows of logits y[i][K] with caller-supplied blocks w[i][4]: word z (index 2) is the uniform word */
void mpol_head_words(int64_t n, int na, const float *y, const uint32_t *w, int det, int32_t *index, float *logp) {
  for (int64_t i = 0; i < n; ++i) index[i] = categorical(y + na * i, na, det, w[4 * i + 2], logp + i);
}

/* the head of n rows, row i the slot slot[i] of match gid[i] at tick[i] */
void mpol_head(int64_t n, int na, const float *y, uint64_t seed, const uint64_t *gid, const uint32_t *tick, const uint32_t *slot,
               int det, int32_t *index, float *logp) {
  for (int64_t i = 0; i < n; ++i) {
    uint32_t w[4];
    mpol_block(seed, gid[i], tick[i], slot[i], w);
    index[i] = categorical(y + na * i, na, det, w[2], logp + i);
  }
}

void mpol_tanh(int64_t n, const float *in, float *out) { for (int64_t i = 0; i < n; ++i) out[i] = tanh_spec(in[i]); }
