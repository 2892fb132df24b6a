// s2d_head.h -- the categorical head of the stochastic policies, shared by the reach-ball policy rollout (s2d_policy.hip) and the
// 11v11 engine's policy slots (s2d_match_slots.h).  (Moved out of s2d_policy.hip unchanged; include/s2d.h has the spec, and
// tests/policy_ref.c::categorical restates it on the host.)
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "s2d_device.h"

// categorical head on the logits q[0 .. A-1] of one env; w = the env's uniform word of this step; returns the action
S2D_DEV int categorical_head(const float* __restrict__ q, int A, bool det, uint32_t w, float& logp) {
  int g = 0;
  float m = q[0];
  for (int a = 1; a < A; ++a) {
    const float v = q[a];
    if (v > m) { m = v; g = a; }
  }
  float S = exp_spec(q[0] - m);
  for (int a = 1; a < A; ++a) S += exp_spec(q[a] - m);
  int act = g;
  if (!det) {
    const float target = rnd_u01(w) * S;
    float c = 0.0f;
    for (int a = 0; a < A; ++a) {
      c += exp_spec(q[a] - m);
      if (c > target) { act = a; break; }
    }
  }
  logp = (q[act] - m) - log_spec(S);
  return act;
}
