/* episodes_ref.c -- plain C restatement of s2d_episode_stats (include/s2d.h): a serial double loop over t, then i, which meets
 * the episodes in rank order.  TEST INFRASTRUCTURE: compiled on demand with -ffp-contract=off (tests/episodes.py). */
#include <stddef.h>
#include <stdint.h>

void episode_stats(int T, int64_t N, const float *reward, const uint8_t *done, const uint8_t *result, float *acc_return,
                   int32_t *acc_length, int64_t C, float *ring_ret, int32_t *ring_len, uint8_t *ring_res, int32_t *ring_env,
                   int64_t *ring_step, uint64_t *totals) {
  const uint64_t e0 = totals[0], s0 = totals[1];
  uint64_t n = 0, k = 0;
  for (int64_t j = 0; j < (int64_t)T * N; ++j) n += done[j] != 0;
  for (int t = 0; t < T; ++t) {
    for (int64_t i = 0; i < N; ++i) {
      const int64_t j = (int64_t)t * N + i;
      const float R = acc_return[i] + (reward ? reward[j] : 0.0f);
      const int32_t L = acc_length[i] + 1;
      if (!done[j]) {
        acc_return[i] = R;
        acc_length[i] = L;
        continue;
      }
      const uint8_t r = result ? result[j] : 0;
      if (k + (uint64_t)C >= n) {
        const uint64_t slot = (e0 + k) % (uint64_t)C;
        ring_ret[slot] = R;
        ring_len[slot] = L;
        ring_res[slot] = r;
        ring_env[slot] = (int32_t)i;
        ring_step[slot] = (int64_t)(s0 + (uint64_t)t);
      }
      totals[2 + (r <= 3 ? r : 0)] += 1;
      totals[6] += (uint64_t)L;
      acc_return[i] = 0.0f;
      acc_length[i] = 0;
      k += 1;
    }
  }
  totals[0] = e0 + n;
  totals[1] = s0 + (uint64_t)T;
  totals[7] += n > (uint64_t)C ? n - (uint64_t)C : 0;
}
