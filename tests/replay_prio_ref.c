/* Host restatement of prioritized replay (s2d_replay_prio_push / s2d_replay_prio_update / s2d_replay_sample_prio,
 * include/s2d.h).  TEST INFRASTRUCTURE.  Written from the header's text, not from the kernels: plain loops, and after every
 * change of a leaf the WHOLE tree is rebuilt level by level (one fp32 add per node, left + right).  Compiled on demand with
 * -ffp-contract=off (the fp32 contract); the only fused operation is the fmaf the spec names. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define PRIO_MIN 0x1p-40f
#define PRIO_MAX 0x1p+40f
enum { REPLAY_PRIO_STREAM = 12 };

int64_t prio_leaves(int64_t capacity) {
  int64_t P = 1;
  while (P < capacity) P *= 2;
  return P;
}

float prio_clamp(float p) { return p >= PRIO_MIN ? (p <= PRIO_MAX ? p : PRIO_MAX) : PRIO_MIN; }

static float max_seen(const float *tree) { return tree[0] >= PRIO_MIN ? tree[0] : 1.0f; }

void prio_rebuild(int64_t capacity, float *tree) {
  for (int64_t i = prio_leaves(capacity) - 1; i >= 1; --i) tree[i] = tree[2 * i] + tree[2 * i + 1];
}

/* cursor = uint64[4] = pos, size, pushes, samples; untouched here */
void prio_push(int64_t n, int64_t capacity, float *tree, const uint64_t *cursor) {
  const int64_t P = prio_leaves(capacity);
  const uint64_t pos = cursor[0] % (uint64_t)capacity;
  const float p0 = max_seen(tree);
  for (int64_t j = 0; j < n; ++j) tree[P + (int64_t)((pos + (uint64_t)j) % (uint64_t)capacity)] = p0;
  prio_rebuild(capacity, tree);
}

void prio_update(int64_t B, int64_t capacity, float *tree, const uint64_t *cursor, const int32_t *index, const float *priority) {
  const int64_t P = prio_leaves(capacity);
  const int64_t size = cursor[1] < (uint64_t)capacity ? (int64_t)cursor[1] : capacity;
  float top = max_seen(tree);
  for (int64_t b = 0; b < B; ++b)                       /* first forget the old priority of every named slot ... */
    if (index[b] >= 0 && index[b] < size) tree[P + index[b]] = 0.0f;
  for (int64_t b = 0; b < B; ++b)                       /* ... then the largest of the new ones wins */
    if (index[b] >= 0 && index[b] < size) {
      const float p = prio_clamp(priority[b]);
      if (p > tree[P + index[b]]) tree[P + index[b]] = p;
      if (p > top) top = p;
    }
  tree[0] = top;
  prio_rebuild(capacity, tree);
}

static void philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

/* the mass element b of a batch of B aims at in sample call number `samples` */
float prio_mass(uint64_t seed, uint64_t samples, uint32_t b, uint32_t B, float total) {
  uint32_t w[4] = {b >> 2, (uint32_t)samples, (uint32_t)(samples >> 32), (uint32_t)REPLAY_PRIO_STREAM << 16};
  philox(w, (uint32_t)seed, (uint32_t)(seed >> 32));
  const float seg = total / (float)B;
  const float u = (float)(w[b & 3u] >> 8) * 0x1p-24f;
  return fmaf(u, seg, (float)b * seg);
}

/* the walk from the root with mass m: the slot it ends on */
int32_t prio_descend(int64_t capacity, const float *tree, float m) {
  const int64_t P = prio_leaves(capacity);
  int64_t i = 1;
  while (i < P) {
    const float l = tree[2 * i], r = tree[2 * i + 1];
    if (m >= l && r > 0.0f) { m = m - l; i = 2 * i + 1; }
    else i = 2 * i;
  }
  return (int32_t)(i - P);
}

void prio_sample(int64_t B, int D, int AW, int64_t capacity, const uint32_t *r_obs, const uint32_t *r_next, const uint32_t *r_action,
                 const float *r_reward, const float *r_discount, const float *tree, uint64_t *cursor, uint64_t seed, uint32_t *b_obs,
                 uint32_t *b_next, uint32_t *b_action, float *b_reward, float *b_discount, int32_t *b_index, float *b_priority,
                 float *b_total) {
  const int64_t P = prio_leaves(capacity);
  const uint64_t size = cursor[1] < (uint64_t)capacity ? cursor[1] : (uint64_t)capacity, samples = cursor[3];
  const float total = tree[1];
  const int empty = size == 0 || !(total > 0.0f);
  b_total[0] = empty ? 0.0f : total;
  for (int64_t b = 0; b < B; ++b) {
    if (empty) {
      b_index[b] = -1;
      memset(b_obs + b * D, 0, (size_t)D * 4);
      memset(b_next + b * D, 0, (size_t)D * 4);
      memset(b_action + b * AW, 0, (size_t)AW * 4);
      b_reward[b] = 0.0f;
      b_discount[b] = 0.0f;
      b_priority[b] = 0.0f;
      continue;
    }
    const int64_t j = prio_descend(capacity, tree, prio_mass(seed, samples, (uint32_t)b, (uint32_t)B, total));
    b_index[b] = (int32_t)j;
    b_priority[b] = tree[P + j];
    memcpy(b_obs + b * D, r_obs + j * D, (size_t)D * 4);
    memcpy(b_next + b * D, r_next + j * D, (size_t)D * 4);
    memcpy(b_action + b * AW, r_action + j * AW, (size_t)AW * 4);
    b_reward[b] = r_reward[j];
    b_discount[b] = r_discount[j];
  }
  cursor[3] += 1;
}
