// s2d_gtc_device.h -- the device side of the GoToCenter task (include/s2d_gtc.h), shared by its two units: s2d_gtc.hip (reset,
// per-step API, random-policy rollout) and s2d_gtc_actor.hip (the fused actors' rollout): the kernel arguments, the env in
// registers, wrap / observation / reset / step and the state planes' load and store.  (Moved out of s2d_gtc.hip unchanged.)
// Behind them the engine behind a handle, which both units' entry points take.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "s2d_device.h"
#include "../../include/s2d_gtc.h"

struct GParams { float x_min, x_max, y_min, y_max, min_dist; int max_steps, continuous, auto_reset; uint32_t seed_lo, seed_hi, gid_lo, gid_hi;
                 int turn, use_turn, adim; };   // adim = floats per action row (actor_out_size in the turn mode, else 1)
struct GEnv { float x, y, body, prev_distance, prev_angle_diff; int step_count, episode; };
enum { GF_X, GF_Y, GF_BODY, GF_PREV_D, GF_PREV_A, GF_STEP, GF_EPISODE, GF_PLANES };
struct GPtrs { float* S; int64_t stride; float* obs; float* reward; uint8_t* done; uint8_t* result; float* terminal_obs; unsigned long long* stats; };

S2D_DEV float g_wrap(float a) {                        // wrap_angle_deg :18-25 -> [-180, 180)
  float t = a + 180.0f;
  return (t - 360.0f * floorf(t * 0.002777777777777778f)) - 180.0f;
}
S2D_DEV float g_angle_to_center(float x, float y) { return g_wrap(atan2_deg(0.0f - y, 0.0f - x)); }   // :27-37
S2D_DEV float g_diff_abs(float a, float b) { return fabsf(g_wrap(a - b)); }                            // :39-44
S2D_DEV float4 g_obs(const GEnv& e) {                  // _get_obs :235-255
  float diff = g_wrap(g_angle_to_center(e.x, e.y) - e.body);
  return make_float4(diff * 0.005555555555555556f, e.body * 0.005555555555555556f, e.x * 0.01904761904761905f,
                     e.y * 0.029411764705882353f);
}
S2D_DEV void g_reset(const GParams& p, GEnv& e, uint32_t gl, uint32_t gh) {   // reset :115-134
  U4 w = philox4x32_10(gl, gh, (uint32_t)e.episode, (S2D_ST_RESET << 16) | 0u, p.seed_lo, p.seed_hi);
  e.x = p.x_min + rnd_u01(w.x) * (p.x_max - p.x_min);
  e.y = p.y_min + rnd_u01(w.y) * (p.y_max - p.y_min);
  e.body = -180.0f + rnd_u01(w.z) * 360.0f;
  e.step_count = 0; e.episode += 1;
  e.prev_distance = hypot2(e.x, e.y);
  e.prev_angle_diff = g_diff_abs(e.body, g_angle_to_center(e.x, e.y));
}
S2D_DEV float g_clip1(float v) { return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v); }
// a = the action row (a.a0 only outside the turn mode), u = the selection uniform of :151
S2D_DEV void g_step(const GParams& p, GEnv& e, const Action4& a, float u, float& reward, int& done, int& result) {   // step :136-233
  float dash_r, turn_r = 0.0f;
  bool dash_selected = true, turn_selected = false;
  if (p.turn && p.continuous) {                         // :142-158
    dash_r = g_clip1(a.a0);                             // :143-144
    if (p.use_turn) {
      turn_r = g_clip1(a.a1);                           // :146
      const float dash_p = g_clip1(a.a2), turn_p = g_clip1(a.a3);   // :147-148
      const float et = exp_spec(turn_p), ed = exp_spec(dash_p);     // :149-150  softmax([turn_p, dash_p])
      const float p0 = et / (et + ed);
      turn_selected = u < p0;                           // :151  (p[0] is the TURN probability here, unlike reach_ball)
      dash_selected = !turn_selected;                   // :152
    }
  } else if (p.continuous) dash_r = g_clip1(a.a0);      // :159-162
  else dash_r = ((float)(int)a.a0 * 0.0625f - 0.5f) * 2.0f;   // :163-166
  if (dash_selected) {
    float dir = g_wrap(e.body + dash_r * 180.0f);       // :169
    float sn, cs;
    sincos_deg(dir, sn, cs);                            // :173-175
    e.x += cs; e.y += sn;                               // :178-179
  }
  if (turn_selected) e.body = g_wrap(e.body + turn_r * 180.0f);   // :181-183
  float d = hypot2(e.x, e.y);                           // :186
  float adiff = g_diff_abs(e.body, g_angle_to_center(e.x, e.y));   // :187-188
  float r = (e.prev_distance - d) + (e.prev_angle_diff - adiff) * 0.005555555555555556f;   // :191-194
  e.step_count += 1;                                    // :196
  int dn = 0, res = S2D_RESULT_NONE;
  if (e.x < p.x_min || e.x > p.x_max || e.y < p.y_min || e.y > p.y_max) { dn = 1; r -= 10.0f; res = S2D_RESULT_OUT; }   // :203-207
  else if (d < p.min_dist) { dn = 1; r += 10.0f; res = S2D_RESULT_GOAL; }                // :209-212
  else if (e.step_count >= p.max_steps) { dn = 1; r -= 5.0f; res = S2D_RESULT_TIMEOUT; }   // :214-217
  e.prev_distance = d; e.prev_angle_diff = adiff;       // :223-224
  reward = r; done = dn; result = res;
}
S2D_DEV void g_load(const GPtrs& q, int64_t i, GEnv& e) {
  e.x = q.S[GF_X * q.stride + i]; e.y = q.S[GF_Y * q.stride + i]; e.body = q.S[GF_BODY * q.stride + i];
  e.prev_distance = q.S[GF_PREV_D * q.stride + i]; e.prev_angle_diff = q.S[GF_PREV_A * q.stride + i];
  e.step_count = __float_as_int(q.S[GF_STEP * q.stride + i]); e.episode = __float_as_int(q.S[GF_EPISODE * q.stride + i]);
}
S2D_DEV void g_store(const GPtrs& q, int64_t i, const GEnv& e) {
  q.S[GF_X * q.stride + i] = e.x; q.S[GF_Y * q.stride + i] = e.y; q.S[GF_BODY * q.stride + i] = e.body;
  q.S[GF_PREV_D * q.stride + i] = e.prev_distance; q.S[GF_PREV_A * q.stride + i] = e.prev_angle_diff;
  q.S[GF_STEP * q.stride + i] = __int_as_float(e.step_count); q.S[GF_EPISODE * q.stride + i] = __int_as_float(e.episode);
}

struct GRoll { float* obs; void* action; float* reward; uint8_t* done; uint8_t* result; };

// ---------------------------------------------------------------- host
// name: the last fused launch (s2d_gtc_kernel_name), written by s2d_gtc_actor.hip
struct S2DGtcEngine { S2DGtcConfig cfg; GParams gp; int64_t n, stride; int device; char* arena; size_t bytes; bool owns; GPtrs q; char name[192]; };
