/* Host restatement of the device replay buffer (s2d_replay_push / s2d_replay_sample, include/s2d.h).  TEST INFRASTRUCTURE.
 * Written from the header's text, not from the kernels: one plain loop per transition, rows copied word by word, the cursor
 * advanced at the end.  Compiled on demand with -ffp-contract=off (the fp32 contract); the only fused
 * operation is the fmaf the spec names. */
#include <math.h>
#include <stdint.h>
#include <string.h>

enum { RESULT_TIMEOUT = 3, REPLAY_STREAM = 11 };

/* ring: obs / next = uint32[C][D], action = uint32[C][AW], reward / discount = float[C]; cursor = uint64[4] = pos, size, pushes,
 * samples */
void replay_push(int T, int64_t N, int D, int AW, int n_step, float gamma, const uint32_t *first_obs, const uint32_t *obs,
                 const uint32_t *terminal_obs, const uint32_t *action, const float *reward, const uint8_t *done, const uint8_t *result,
                 int64_t C, uint32_t *r_obs, uint32_t *r_next, uint32_t *r_action, float *r_reward, float *r_discount,
                 uint64_t *cursor) {
  const uint64_t pos = cursor[0];
  for (int t = 0; t < T; ++t)
    for (int64_t i = 0; i < N; ++i) {
      float R = reward[t * N + i], g = gamma, discount;
      int s = t;
      while (!done[s * N + i] && s + 1 < T && s + 1 - t < n_step) {
        s += 1;
        R = fmaf(g, reward[s * N + i], R);
        g = g * gamma;
      }
      const uint32_t *next;
      if (done[s * N + i]) {
        next = terminal_obs + (s * N + i) * D;
        discount = (result && result[s * N + i] == RESULT_TIMEOUT) ? g : 0.0f;
      } else {
        next = obs + (s * N + i) * D;
        discount = g;
      }
      const uint32_t *from = t == 0 ? first_obs + i * D : obs + ((t - 1) * N + i) * D;
      const uint64_t slot = (pos + (uint64_t)t * (uint64_t)N + (uint64_t)i) % (uint64_t)C;
      memcpy(r_obs + slot * D, from, (size_t)D * 4);
      memcpy(r_next + slot * D, next, (size_t)D * 4);
      memcpy(r_action + slot * AW, action + (t * N + i) * AW, (size_t)AW * 4);
      r_reward[slot] = R;
      r_discount[slot] = discount;
    }
  const uint64_t n = (uint64_t)T * (uint64_t)N;
  cursor[0] = (pos + n) % (uint64_t)C;
  cursor[1] = cursor[1] + n < (uint64_t)C ? cursor[1] + n : (uint64_t)C;
  cursor[2] += 1;
}

static void philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

/* the slot element b of sample call number `samples` draws from `size` transitions (size >= 1) */
int32_t replay_index(uint64_t seed, uint64_t samples, uint32_t b, uint32_t size) {
  uint32_t w[4] = {b >> 2, (uint32_t)samples, (uint32_t)(samples >> 32), (uint32_t)REPLAY_STREAM << 16};
  philox(w, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (int32_t)(((uint64_t)w[b & 3u] * size) >> 32);
}

void replay_sample(int64_t B, int D, int AW, int64_t C, const uint32_t *r_obs, const uint32_t *r_next, const uint32_t *r_action,
                   const float *r_reward, const float *r_discount, uint64_t *cursor, uint64_t seed, uint32_t *b_obs, uint32_t *b_next,
                   uint32_t *b_action, float *b_reward, float *b_discount, int32_t *b_index) {
  const uint64_t size = cursor[1], samples = cursor[3];
  (void)C;
  for (int64_t b = 0; b < B; ++b) {
    if (size == 0) {
      b_index[b] = -1;
      memset(b_obs + b * D, 0, (size_t)D * 4);
      memset(b_next + b * D, 0, (size_t)D * 4);
      memset(b_action + b * AW, 0, (size_t)AW * 4);
      b_reward[b] = 0.0f;
      b_discount[b] = 0.0f;
      continue;
    }
    const int64_t j = replay_index(seed, samples, (uint32_t)b, (uint32_t)size);
    b_index[b] = (int32_t)j;
    memcpy(b_obs + b * D, r_obs + j * D, (size_t)D * 4);
    memcpy(b_next + b * D, r_next + j * D, (size_t)D * 4);
    memcpy(b_action + b * AW, r_action + j * AW, (size_t)AW * 4);
    b_reward[b] = r_reward[j];
    b_discount[b] = r_discount[j];
  }
  cursor[3] += 1;
}
