// s2d_see.hip -- the vision layer of the 11v11 match engine for MI355X (gfx950): view cone, neck, see-message quantisation and
// see timing (include/s2d_match.h, "Vision").  Restated from the published behaviour of rcssserver's synchronous see mode
// (EXT: parity to rcssserver unpinned); tests/see_ref.c is an independent CPU restatement this file matches bit for bit.
//
// A unit of its own: it reads an engine through the public s2d_match_buffers() and one library-internal accessor for the
// Philox keys; the engine holds no vision state, so nothing in s2d_match.hip's kernels knows of this file.
//
// Mapping of the see kernel, as s2d_match_agent_obs_kernel: ONE MATCH PER HALF-WAVE, lane = object (0..21 players, 22 the ball).
// The loop over the mask's agents is uniform.  Per agent every lane derives the eight words of its object; the place of a
// player's row (left to right across the view) is a COUNT over the half-wave's keys (22 broadcast reads of an LDS tile, no
// sort loop and no divergence over agents); the row is assembled in LDS and leaves as whole 64-byte lines, one float4 per lane
// and store instruction.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "s2d_device.h"
#include "../../include/s2d_match.h"

#define S2D_API extern "C" __attribute__((visibility("default")))

extern "C" void s2d_internal_set_error(const char* msg);
extern "C" int s2d_match_internal_keys(S2DMatchHandle h, uint32_t keys[4], int* device);

namespace {

constexpr int kBlock = 256;
constexpr int kHalf = 32;
constexpr int kEnvsPerBlock = kBlock / kHalf;
constexpr int NP = S2D_MATCH_PLAYERS;
constexpr int BALL = S2D_MATCH_BALL;
constexpr int SLOTS = S2D_MATCH_SLOTS;
constexpr int kSeeVec = S2D_SEE_DIM / 4;                 // 48 float4 per row
constexpr int kSeeOthers = NP - 1;                       // 21 player rows
static_assert(S2D_SEE_DIM == S2D_SEE_PLAYERS + kSeeOthers * S2D_SEE_ROW_WORDS, "row layout");
static_assert(S2D_SEE_SELF == 0 && S2D_SEE_BALL == 16 && S2D_SEE_PLAYERS == 24 && S2D_SEE_ROW_WORDS == 8, "row layout");
static_assert(kSeeVec > kHalf && kSeeVec <= 2 * kHalf, "a half-wave stores a row as two float4 per lane");
enum { SIDE_NONE = 0, SIDE_LEFT = 1, SIDE_RIGHT = 2 };

// S2DVisionParams rounded once (double -> float); the reciprocals are the floats of the double quotients
struct SeeParams {
  float view_angle[3]; int interval[3];
  float visible, dist_q, inv_dist_q, dist_r, inv_dist_r, dchg_q, inv_dchg_q, rchg_q, inv_rchg_q;
  float unum_far, unum_too_far, inv_unum_band, team_far, team_too_far, inv_team_band;
  float min_moment, max_moment, min_neck, max_neck;
  uint32_t seed_lo, seed_hi, gid_lo, gid_hi;
};
// the planes ([N][24]) and words ([N]) of S2DMatchBuffers the layer reads
struct SeeState {
  const float *x, *y, *vx, *vy, *body, *stamina, *effort, *recovery, *capacity;
  const int32_t *card, *cycle, *mode, *mode_side, *tick;
};

S2D_DEV void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
S2D_DEV uint32_t hballot(bool pred, int half) { return (uint32_t)(__ballot(pred) >> (half * kHalf)); }
S2D_DEV float own_body(float b, bool right) { return right ? (b > 0.0f ? b - 180.0f : b + 180.0f) : b; }
S2D_DEV float side_word(int side, int ours) { return side == ours ? 1.0f : (side == SIDE_NONE ? 0.0f : -1.0f); }
S2D_DEV int width_index(int code) { return code == 1 ? 0 : (code == 3 ? 2 : 1); }   // anything but narrow / wide reads as normal
// (constant indices and selects: a lane-varying index into a kernel argument would go through scratch memory)
S2D_DEV float pick3(const float (&a)[3], int i) { return i == 0 ? a[0] : (i == 2 ? a[2] : a[1]); }
S2D_DEV int pick3(const int (&a)[3], int i) { return i == 0 ? a[0] : (i == 2 ? a[2] : a[1]); }
S2D_DEV float quant(float v, float q, float inv_q) { return rintf(v * inv_q) * q; }

struct SeeShared {                                       // one match (half-wave): the lanes' state, the order keys, the row
  float x[kHalf], y[kHalf], vx[kHalf], vy[kHalf], body[kHalf], neck[kHalf];
  int width[kHalf], wait[kHalf], card[kHalf];
  float2 key[kHalf];
  float4 row[kSeeVec];
};

__global__ __launch_bounds__(kBlock) void s2d_match_see_kernel(SeeParams p, SeeState s, S2DMatchVision vis, int64_t n, uint32_t mask,
                                                               float* __restrict__ see) {
  __shared__ SeeShared sh_all[kEnvsPerBlock];
  SeeShared& sh = sh_all[threadIdx.x / kHalf];
  const int l = threadIdx.x & (kHalf - 1);
  const int half = (threadIdx.x >> 5) & 1;
  const int64_t e = (int64_t)blockIdx.x * kEnvsPerBlock + threadIdx.x / kHalf;
  const bool valid = e < n;
  const int64_t ec = valid ? e : n - 1;
  const bool is_player = l < NP;
  float x = 0.0f, y = 0.0f, vx = 0.0f, vy = 0.0f, body = 0.0f, neck = 0.0f;
  float stamina = 0.0f, effort = 0.0f, recovery = 0.0f, capacity = 0.0f;
  int card = 0, width = 0, wait = 0;
  const int64_t k = ec * SLOTS + l;
  if (l <= BALL) { x = s.x[k]; y = s.y[k]; vx = s.vx[k]; vy = s.vy[k]; }
  if (is_player) {
    body = s.body[k]; stamina = s.stamina[k]; effort = s.effort[k]; recovery = s.recovery[k]; capacity = s.capacity[k];
    card = s.card[k]; neck = vis.neck[k]; width = vis.view_width[k]; wait = vis.see_wait[k];
  }
  const int mode = s.mode[ec], mode_side = s.mode_side[ec], cycle = s.cycle[ec];
  const uint32_t tick = (uint32_t)s.tick[ec];
  const uint64_t gid = (((uint64_t)p.gid_hi << 32) | p.gid_lo) + (uint64_t)ec;
  sh.x[l] = x; sh.y[l] = y; sh.vx[l] = vx; sh.vy[l] = vy; sh.body[l] = body; sh.neck[l] = neck;
  sh.width[l] = width; sh.wait[l] = wait; sh.card[l] = card;
  const bool active = l == BALL || (is_player && card < S2D_CARD_RED);
  wave_fence();
  const int nrows = __builtin_popcount(mask);
  float* out = see + (e * (int64_t)nrows) * S2D_SEE_DIM;
  uint32_t rest = mask;
  for (int r = 0; r < nrows; ++r) {
    const int pa = __builtin_ctz(rest);                  // the agent (uniform: the mask is a kernel argument)
    rest &= rest - 1u;
    const bool right = pa >= 11;
    const int ours = right ? SIDE_RIGHT : SIDE_LEFT;
    const float sg = right ? -1.0f : 1.0f;
    // the agent, in its team's frame
    const float ax = sg * sh.x[pa], ay = sg * sh.y[pa], avx = sg * sh.vx[pa], avy = sg * sh.vy[pa];
    const float abody = own_body(sh.body[pa], right), aneck = sh.neck[pa];
    const float face = norm_deg_any(abody + aneck);
    const int wi = width_index(sh.width[pa]);
    const bool fresh = sh.wait[pa] == pick3(p.interval, wi);
    const bool can_see = fresh && sh.card[pa] < S2D_CARD_RED;
    // this lane's object in that frame
    const float ox = sg * x, oy = sg * y, ovx = sg * vx, ovy = sg * vy, obody = own_body(body, right);
    const float dx = ox - ax, dy = oy - ay;
    const float d = hypot2(dx, dy);
    const bool here = d == 0.0f;
    const float rel = here ? 0.0f : norm_deg_any(atan2_deg(dy, dx) - face);
    const bool in_cone = fabsf(rel) <= 0.5f * pick3(p.view_angle, wi);
    const bool felt = d <= p.visible;
    const bool object = can_see && active && l != pa;    // something this agent could see in this cycle
    int level = 0;
    if (object) {
      if (in_cone) {
        level = 4;
        if (is_player) {
          const bool band = (d > p.unum_far && d < p.unum_too_far) || (d > p.team_far && d < p.team_too_far);
          float u1 = 0.0f, u2 = 0.0f;
          if (band) {
            const U4 w = philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), tick,
                                       ((uint32_t)S2D_MATCH_ST_SEE << 16) | (uint32_t)(pa * SLOTS + l), p.seed_lo, p.seed_hi);
            u1 = rnd_u01(w.x); u2 = rnd_u01(w.y);
          }
          if (d <= p.unum_far) level = 4;
          else if (d < p.unum_too_far && u1 >= (d - p.unum_far) * p.inv_unum_band) level = 4;
          else if (d <= p.team_far) level = 3;
          else if (d < p.team_too_far && u2 >= (d - p.team_far) * p.inv_team_band) level = 3;
          else level = 2;
        }
      } else if (felt) {
        level = 1;
      }
    }
    float dist = 0.0f, dir = 0.0f, dist_chg = 0.0f, dir_chg = 0.0f, body_rel = 0.0f;
    if (level >= 1 && !here) {
      dist = quant(exp_spec(quant(log_spec(d), p.dist_q, p.inv_dist_q)), p.dist_r, p.inv_dist_r);
      dir = rintf(rel);
    }
    if (level == 4) {
      if (!here) {
        const float ex = dx / d, ey = dy / d, rvx = ovx - avx, rvy = ovy - avy;
        dist_chg = dist * quant(fmaf(rvx, ex, rvy * ey) / d, p.dchg_q, p.inv_dchg_q);
        dir_chg = quant((fmaf(rvy, ex, -(rvx * ey)) / d) * 57.29577951308232f, p.rchg_q, p.inv_rchg_q);
      }
      body_rel = rintf(norm_deg_any(obody - face));
    }
    // the place of a player's row: seen ones ascending by (dir, dist, own-frame slot), then the unseen ones
    const bool seen = is_player && level >= 1;
    sh.key[l] = make_float2(dir, dist);
    const uint32_t seen_mask = hballot(seen, half) & 0x3FFFFFu;
    wave_fence();
    int rank = 0;
    const int own_l = right ? (l < 11 ? l + 11 : l - 11) : l;   // the slot in the agent's frame: his team first
    if (seen) {
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const float2 kj = sh.key[j];
        const int own_j = right ? (j + 11) % NP : j;       // (a constant per side after unrolling)
        const bool before = kj.x < dir || (kj.x == dir && (kj.y < dist || (kj.y == dist && own_j < own_l)));
        rank += (((seen_mask >> j) & 1u) != 0u && before) ? 1 : 0;
      }
    } else {
      const uint32_t unseen = 0x3FFFFFu & ~seen_mask & ~(1u << pa);
      rank = __builtin_popcount(seen_mask) + __builtin_popcount(unseen & ((1u << l) - 1u));
    }
    if (is_player && l != pa) {
      const float team = level >= 3 ? ((l < 11) == !right ? 1.0f : -1.0f) : 0.0f;
      const float unum = level == 4 ? (float)(l % 11 + 1) : 0.0f;
      sh.row[S2D_SEE_PLAYERS / 4 + 2 * rank] = make_float4((float)level, team, unum, dist);
      sh.row[S2D_SEE_PLAYERS / 4 + 2 * rank + 1] = make_float4(dir, dist_chg, dir_chg, body_rel);
    } else if (l == pa) {
      sh.row[0] = make_float4(ox, oy, ovx, ovy);
      sh.row[1] = make_float4(obody, aneck, face, (float)(wi + 1));
      sh.row[2] = make_float4(fresh ? 1.0f : 0.0f, (float)wait, stamina, effort);
      sh.row[3] = make_float4(recovery, capacity, (l == S2D_MATCH_GOALIE_LEFT || l == S2D_MATCH_GOALIE_RIGHT) ? 1.0f : 0.0f, (float)card);
    } else if (l == BALL) {
      sh.row[S2D_SEE_BALL / 4] = make_float4((float)level, dist, dir, dist_chg);
      sh.row[S2D_SEE_BALL / 4 + 1] = make_float4(dir_chg, (float)mode, side_word(mode_side, ours), (float)cycle);
    }
    wave_fence();
    if (valid) {                                         // 512 + 256 B: every 64-byte line written whole by one instruction
      float4* dst = reinterpret_cast<float4*>(out + (int64_t)r * S2D_SEE_DIM);
      dst[l] = sh.row[l];
      if (l + kHalf < kSeeVec) dst[l + kHalf] = sh.row[l + kHalf];
    }
    wave_fence();
  }
}

// one thread per slot of the [N][24] planes; the two pad slots (ball, pad) are left alone
__global__ __launch_bounds__(kBlock) void s2d_match_vision_step_kernel(SeeParams p, const int32_t* __restrict__ card, S2DMatchVision vis,
                                                                       const float* __restrict__ act, const uint8_t* __restrict__ done,
                                                                       int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n * SLOTS) return;
  const int64_t e = i / SLOTS;
  const int l = (int)(i - e * SLOTS);
  if (l >= NP) return;
  float neck = vis.neck[i];
  int width = vis.view_width[i], wait = vis.see_wait[i];
  if (done && done[e]) {
    neck = 0.0f; width = 2; wait = 0;
  } else if (card[i] >= S2D_CARD_RED) {
    return;                                              // sent off: the state stands
  } else if (act) {
    const float m_in = act[(e * NP + l) * 2], c = act[(e * NP + l) * 2 + 1];
    const float m = m_in != m_in ? 0.0f : clampf(m_in, p.min_moment, p.max_moment);
    neck = clampf(norm_deg_any(neck + m), p.min_neck, p.max_neck);
    const int code = c == 1.0f ? 1 : (c == 2.0f ? 2 : (c == 3.0f ? 3 : 0));
    if (code != 0) {
      width = code;
      const int lim = pick3(p.interval, code - 1);
      wait = wait > lim ? lim : wait;                    // a pending wait never exceeds the new width's interval
    }
  }
  wait = wait > 1 ? wait - 1 : 0;
  if (wait == 0) wait = pick3(p.interval, width_index(width));
  vis.neck[i] = neck; vis.view_width[i] = width; vis.see_wait[i] = wait;
}

__global__ __launch_bounds__(kBlock) void s2d_match_vision_reset_kernel(S2DMatchVision vis, const uint8_t* __restrict__ mask, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n * SLOTS) return;
  if (mask && !mask[i / SLOTS]) return;
  vis.neck[i] = 0.0f; vis.view_width[i] = 2; vis.see_wait[i] = 0;
}

int vfail(int code, const std::string& msg) { s2d_internal_set_error(msg.c_str()); return code; }

struct DeviceGuard {
  int prev = -1; bool ok = false;
  explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) == hipSuccess) ok = (prev == dev) || (hipSetDevice(dev) == hipSuccess); }
  ~DeviceGuard() { if (ok && prev >= 0) (void)hipSetDevice(prev); }
};

const char* vision_params_error(const S2DVisionParams* v) {
  if (!v) return "NULL vision parameters";
  const double all[] = {v->view_angle[0], v->view_angle[1], v->view_angle[2], v->see_interval[0], v->see_interval[1], v->see_interval[2],
                        v->visible_distance, v->dist_quantize_step, v->dist_round, v->dist_chg_quantize, v->dir_chg_quantize,
                        v->unum_far_length, v->unum_too_far_length, v->team_far_length, v->team_too_far_length,
                        v->min_neck_moment, v->max_neck_moment, v->min_neck_angle, v->max_neck_angle};
  for (double d : all) if (!std::isfinite(d)) return "vision parameters must be finite";
  for (int i = 0; i < 3; ++i) {
    if (!(v->view_angle[i] > 0.0 && v->view_angle[i] <= 360.0)) return "view_angle must lie in (0, 360]";
    if (!(v->see_interval[i] >= 1.0 && v->see_interval[i] <= 1.0e6) || v->see_interval[i] != std::floor(v->see_interval[i]))
      return "see_interval must be a whole number of cycles in [1, 1e6]";
  }
  if (v->visible_distance < 0.0) return "visible_distance must be >= 0";
  if (!(v->dist_quantize_step > 0.0 && v->dist_round > 0.0 && v->dist_chg_quantize > 0.0 && v->dir_chg_quantize > 0.0))
    return "the quantisation steps must be > 0";
  if (v->unum_far_length < 0.0 || v->team_far_length < 0.0) return "the far lengths must be >= 0";
  if (v->unum_far_length > v->unum_too_far_length) return "unum_far_length must not exceed unum_too_far_length";
  if (v->team_far_length > v->team_too_far_length) return "team_far_length must not exceed team_too_far_length";
  if (v->min_neck_moment > v->max_neck_moment) return "min_neck_moment must not exceed max_neck_moment";
  if (v->min_neck_angle > v->max_neck_angle) return "min_neck_angle must not exceed max_neck_angle";
  return nullptr;
}

SeeParams see_params(const S2DVisionParams& v, const uint32_t keys[4]) {
  SeeParams p;
  for (int i = 0; i < 3; ++i) { p.view_angle[i] = (float)v.view_angle[i]; p.interval[i] = (int)v.see_interval[i]; }
  p.visible = (float)v.visible_distance;
  p.dist_q = (float)v.dist_quantize_step; p.inv_dist_q = (float)(1.0 / v.dist_quantize_step);
  p.dist_r = (float)v.dist_round; p.inv_dist_r = (float)(1.0 / v.dist_round);
  p.dchg_q = (float)v.dist_chg_quantize; p.inv_dchg_q = (float)(1.0 / v.dist_chg_quantize);
  p.rchg_q = (float)v.dir_chg_quantize; p.inv_rchg_q = (float)(1.0 / v.dir_chg_quantize);
  p.unum_far = (float)v.unum_far_length; p.unum_too_far = (float)v.unum_too_far_length;
  p.team_far = (float)v.team_far_length; p.team_too_far = (float)v.team_too_far_length;
  const double ub = v.unum_too_far_length - v.unum_far_length, tb = v.team_too_far_length - v.team_far_length;
  p.inv_unum_band = ub > 0.0 ? (float)(1.0 / ub) : 0.0f;
  p.inv_team_band = tb > 0.0 ? (float)(1.0 / tb) : 0.0f;
  p.min_moment = (float)v.min_neck_moment; p.max_moment = (float)v.max_neck_moment;
  p.min_neck = (float)v.min_neck_angle; p.max_neck = (float)v.max_neck_angle;
  p.seed_lo = keys[0]; p.seed_hi = keys[1]; p.gid_lo = keys[2]; p.gid_hi = keys[3];
  return p;
}

const char* vision_planes_error(const S2DMatchVision* vis) {
  if (!vis || !vis->neck || !vis->view_width || !vis->see_wait) return "NULL vision plane";
  if ((reinterpret_cast<uintptr_t>(vis->neck) | reinterpret_cast<uintptr_t>(vis->view_width) | reinterpret_cast<uintptr_t>(vis->see_wait)) & 3u)
    return "the vision planes must be 4-byte aligned";
  return nullptr;
}

// what every entry point needs of the engine
struct EngineView { S2DMatchBuffers buf; uint32_t keys[4]; int device; };
int engine_view(S2DMatchHandle h, EngineView& v) {
  if (!h) return vfail(S2D_EINVAL, "NULL handle");
  int rc = s2d_match_buffers(h, &v.buf);
  if (rc != S2D_OK) return rc;
  return s2d_match_internal_keys(h, v.keys, &v.device);
}
unsigned plane_grid(int64_t n) { return (unsigned)((n * SLOTS + kBlock - 1) / kBlock); }

}  // namespace

S2D_API void s2d_match_vision_default_params(S2DVisionParams* v) {
  if (!v) return;
  v->view_angle[0] = 60.0; v->view_angle[1] = 120.0; v->view_angle[2] = 180.0;
  v->see_interval[0] = 1.0; v->see_interval[1] = 2.0; v->see_interval[2] = 3.0;
  v->visible_distance = 3.0;
  v->dist_quantize_step = 0.1; v->dist_round = 0.1; v->dist_chg_quantize = 0.02; v->dir_chg_quantize = 0.1;
  v->unum_far_length = 20.0; v->unum_too_far_length = 40.0; v->team_far_length = 40.0; v->team_too_far_length = 60.0;
  v->min_neck_moment = -180.0; v->max_neck_moment = 180.0; v->min_neck_angle = -90.0; v->max_neck_angle = 90.0;
}

S2D_API int s2d_match_vision_validate(const S2DVisionParams* v) {
  const char* err = vision_params_error(v);
  return err ? vfail(S2D_EINVAL, err) : S2D_OK;
}

S2D_API int s2d_match_vision_reset(S2DMatchHandle h, const S2DMatchVision* vis, const uint8_t* mask_dev, void* stream) {
  EngineView ev;
  int rc = engine_view(h, ev);
  if (rc != S2D_OK) return rc;
  if (const char* err = vision_planes_error(vis)) return vfail(S2D_EINVAL, err);
  DeviceGuard guard(ev.device);
  hipLaunchKernelGGL(s2d_match_vision_reset_kernel, dim3(plane_grid(ev.buf.n_envs)), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                     *vis, mask_dev, ev.buf.n_envs);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return vfail(S2D_EHIP, std::string("vision reset launch: ") + hipGetErrorString(e));
  return S2D_OK;
}

S2D_API int s2d_match_vision_step(S2DMatchHandle h, const S2DVisionParams* prm, const S2DMatchVision* vis, const float* view_actions_dev,
                                  const uint8_t* done_dev, void* stream) {
  EngineView ev;
  int rc = engine_view(h, ev);
  if (rc != S2D_OK) return rc;
  if (const char* err = vision_params_error(prm)) return vfail(S2D_EINVAL, err);
  if (const char* err = vision_planes_error(vis)) return vfail(S2D_EINVAL, err);
  if (reinterpret_cast<uintptr_t>(view_actions_dev) & 3u) return vfail(S2D_EINVAL, "view_actions must be 4-byte aligned (float)");
  DeviceGuard guard(ev.device);
  hipLaunchKernelGGL(s2d_match_vision_step_kernel, dim3(plane_grid(ev.buf.n_envs)), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                     see_params(*prm, ev.keys), ev.buf.card, *vis, view_actions_dev, done_dev, ev.buf.n_envs);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return vfail(S2D_EHIP, std::string("vision step launch: ") + hipGetErrorString(e));
  return S2D_OK;
}

S2D_API int s2d_match_see(S2DMatchHandle h, const S2DVisionParams* prm, const S2DMatchVision* vis, uint32_t slot_mask, float* see_dev,
                          void* stream) {
  EngineView ev;
  int rc = engine_view(h, ev);
  if (rc != S2D_OK) return rc;
  if (!see_dev) return vfail(S2D_EINVAL, "NULL argument");
  if (const char* err = vision_params_error(prm)) return vfail(S2D_EINVAL, err);
  if (const char* err = vision_planes_error(vis)) return vfail(S2D_EINVAL, err);
  if (slot_mask == 0u || (slot_mask >> NP) != 0u)
    return vfail(S2D_EINVAL, "slot_mask must be a non-empty set of bits 0..21 (0x3FFFFF = all agents)");
  if (reinterpret_cast<uintptr_t>(see_dev) & 15u) return vfail(S2D_EINVAL, "see buffer must be 16-byte aligned");
  const S2DMatchBuffers& b = ev.buf;
  const SeeState st{b.x, b.y, b.vx, b.vy, b.body, b.stamina, b.effort, b.recovery, b.stamina_capacity,
                    b.card, b.cycle, b.mode, b.mode_side, b.tick};
  DeviceGuard guard(ev.device);
  const unsigned grid = (unsigned)((b.n_envs + kEnvsPerBlock - 1) / kEnvsPerBlock);
  hipLaunchKernelGGL(s2d_match_see_kernel, dim3(grid), dim3(kBlock), 0, static_cast<hipStream_t>(stream), see_params(*prm, ev.keys), st,
                     *vis, b.n_envs, slot_mask, see_dev);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return vfail(S2D_EHIP, std::string("see launch: ") + hipGetErrorString(e));
  return S2D_OK;
}
