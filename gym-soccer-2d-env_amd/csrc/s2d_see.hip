// s2d_see.hip -- the vision layer of the 11v11 match engine for MI355X (gfx950): view cone, neck, see-message quantisation and
// see timing (include/s2d_match.h, "Vision").  Restated from the published behaviour of rcssserver's synchronous see mode
// (EXT: parity to rcssserver unpinned); tests/see_ref.c is an independent CPU restatement this file matches bit for bit.
//
// A unit of its own: it reads an engine through the public s2d_match_buffers() and one library-internal accessor for the
// Philox keys; the engine holds no vision state, so nothing in the match engine's kernels knows of this file
// (a see network, s2d_match_set_see_network, is the cycle kernel's own use of s2d_see_row.h).
//
// Mapping of the see kernel, as s2d_match_agent_obs_kernel: ONE MATCH PER HALF-WAVE, lane = object (0..21 players, 22 the ball).
// The loop over the mask's agents is uniform.  The row itself -- and one player's vision step -- are device functions in
// s2d_see_row.h, which the cycle kernel's SEE instantiations (s2d_match_cycle.h) execute too; here the row is assembled in LDS and
// leaves as whole 64-byte lines, one float4 per lane and store instruction.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "s2d_device.h"
#include "s2d_see_row.h"
#include "../../include/s2d_match.h"

#define S2D_API extern "C" __attribute__((visibility("default")))

extern "C" void s2d_internal_set_error(const char* msg);
extern "C" int s2d_match_internal_keys(S2DMatchHandle h, uint32_t keys[4], int* device);

namespace {

using namespace s2d_see;

constexpr int kBlock = 256;
constexpr int kHalf = kSeeHalf;
constexpr int kEnvsPerBlock = kBlock / kHalf;
constexpr int NP = S2D_MATCH_PLAYERS;
constexpr int BALL = S2D_MATCH_BALL;
constexpr int SLOTS = S2D_MATCH_SLOTS;

// the planes ([N][24]) and words ([N]) of S2DMatchBuffers the layer reads
struct SeeState {
  const float *x, *y, *vx, *vy, *body, *stamina, *effort, *recovery, *capacity;
  const int32_t *card, *cycle, *mode, *mode_side, *tick;
};

struct SeeShared : SeeFacts {                            // one match (half-wave): the facts (s2d_see_row.h), then the row
  float4 row[kSeeVec];
};

// The lane mapping, the loads, the agent loop and the stores around see_row() (s2d_see_row.h: the object derivation, the ranking by
// counting keys and the row assembly, shared with the cycle kernel's SEE instantiations).
__global__ __launch_bounds__(kBlock) void s2d_match_see_kernel(SeeParams p, SeeState s, S2DMatchVision vis, int64_t n, uint32_t mask,
                                                               float* __restrict__ see) {
  __shared__ SeeShared sh_all[kEnvsPerBlock];
  SeeShared& sh = sh_all[threadIdx.x / kHalf];
  const int l = threadIdx.x & (kHalf - 1);
  const int half = (threadIdx.x >> 5) & 1;
  const int64_t e = (int64_t)blockIdx.x * kEnvsPerBlock + threadIdx.x / kHalf;
  const bool valid = e < n;
  const int64_t ec = valid ? e : n - 1;
  SeeIn in{};
  const int64_t k = ec * SLOTS + l;
  if (l <= BALL) { in.x = s.x[k]; in.y = s.y[k]; in.vx = s.vx[k]; in.vy = s.vy[k]; }
  if (l < NP) {
    in.body = s.body[k]; in.stamina = s.stamina[k]; in.effort = s.effort[k]; in.recovery = s.recovery[k]; in.capacity = s.capacity[k];
    in.card = s.card[k]; in.neck = vis.neck[k]; in.width = vis.view_width[k]; in.wait = vis.see_wait[k];
  }
  in.mode = s.mode[ec]; in.mode_side = s.mode_side[ec]; in.cycle = s.cycle[ec];
  in.tick = (uint32_t)s.tick[ec];
  const uint64_t gid = (((uint64_t)p.gid_hi << 32) | p.gid_lo) + (uint64_t)ec;
  see_facts(sh, in, l);
  const int nrows = __builtin_popcount(mask);
  float* out = see + (e * (int64_t)nrows) * S2D_SEE_DIM;
  uint32_t rest = mask;
  for (int r = 0; r < nrows; ++r) {
    const int pa = __builtin_ctz(rest);                  // the agent (uniform: the mask is a kernel argument)
    rest &= rest - 1u;
    see_row(p, sh, in, l, half, pa, gid, sh.row);
    if (valid) see_row_store(out + (int64_t)r * S2D_SEE_DIM, sh.row, l);
    see_fence();
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
  const bool is_done = done && done[e];
  const bool sent_off = card[i] >= S2D_CARD_RED;
  if (!is_done && sent_off) return;
  float m_in = 0.0f, c = 0.0f;
  if (act && !is_done) { m_in = act[(e * NP + l) * 2]; c = act[(e * NP + l) * 2 + 1]; }
  vision_advance(p, neck, width, wait, is_done, sent_off, act != nullptr, m_in, c);
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
