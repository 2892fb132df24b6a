// s2d_sac_head.h -- the squashed-Gaussian head of Soft Actor-Critic, shared by the SAC rollout (s2d_wide_actor.hip,
// s2d_rollout_sac), the entropy-regularised TD target (s2d_td.hip: TdSacHead, the head of s2d_td_target_ac_kernel behind
// s2d_td_target_sac) and the SAC actor step (s2d_learn.hip).  include/s2d.h has the spec, and
// tests/sac_ref.c::sac_term restates it on the host.
#pragma once
#include <hip/hip_runtime.h>

#include "s2d_device.h"

// One action dimension: mean = y[j], v = y[A + j] (the raw log-std), z = its standard normal (ignored when det).  a <- the
// squashed action; returns the dimension's term of logp (the caller adds the terms in ascending j, the first starts the sum).
S2D_DEV float sac_head_term(float mean, float v, float z, bool det, float& a) {
  const float ls = v > 2.0f ? 2.0f : (v >= -20.0f ? v : -20.0f);   // SB3's LOG_STD_MAX / LOG_STD_MIN; a NaN becomes -20
  const float sigma = exp_spec(ls);
  const float zj = det ? 0.0f : z;
  const float u = det ? mean : fmaf(sigma, zj, mean);              // det: the mean itself, so that -0 stays -0
  a = tanh_spec(u);
  const float gauss = fmaf(-0.5f * zj, zj, -ls) - 0.91893853f;
  return gauss - log_spec(fmaf(-a, a, 1.0f) + 1e-6f);              // SB3's log(1 - tanh^2 + 1e-6) correction
}
