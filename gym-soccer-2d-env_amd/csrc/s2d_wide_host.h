// s2d_wide_host.h -- the host side that the users of the streamed-weight MLP (s2d_wide_net.h) share: the reach-ball actors
// (s2d_wide_actor.hip, input width 10), the GoToCenter actors (s2d_gtc_actor.hip, 4) and the TD targets (s2d_td.hip, 1 .. 256);
// and the host utilities of those units and of s2d_learn.hip.  One place for the shape's grid and its refusals, the fragment
// count, the workspace's size and check, the network's text, the waves,tiles override and the (waves, tiles) search, and for the
// pack kernel's launch (s2d_wide_pack.hip, which also defines what is only declared here: same library, hidden symbols).
// Host code only: no device code crosses a unit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <string>

#include "s2d_actor_net.h"

extern "C" void s2d_internal_set_error(const char* msg);

static constexpr int kWideMaxHidden = 5;
static constexpr int kWideMaxWidth = 400;
static const char* const kActName[3] = {"relu", "tanh", "sigmoid"};

// ------------------------------------------------------------------------------------------ utilities
// S2D_EINVAL with the text "who: msg"
static inline int fail(const std::string& who, const std::string& msg) {
  s2d_internal_set_error((who + ": " + msg).c_str());
  return S2D_EINVAL;
}
static inline bool misaligned(const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; }
// what a launch (or a chain of them) left: S2D_OK, or S2D_EHIP with the text set
static inline int launched(const std::string& who) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return S2D_OK;
  s2d_internal_set_error((who + ": launch: " + hipGetErrorString(e)).c_str());
  return S2D_EHIP;
}

// The dynamic-LDS limit is a per-device property of the function: set it once per (device, instantiation `slot`), under a lock
// (engines on several devices may be driven from several threads); the caller has made the device current.  One table
// per Owner: every back end numbers its instantiations from 0 (Owner = its Dims; s2d_policy.hip, s2d_td.hip and s2d_learn.hip
// have tags of their own).
// kLdsSlots: the most instantiations an Owner has -- a back end's 16 (the Q head's 3, the tanh head's 2 x 3 x 2, then its
// diagnostic kernel in the last slot); s2d_policy.hip uses 9 (3 modes x 3 noise kinds)
static constexpr int kLdsSlots = 16;
template <typename Owner>
static bool allow_lds_slot(const void* fn, int slot) {
  static std::mutex attr_mu;
  static bool attr_set[kMaxDevices][kLdsSlots] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return false;
  std::lock_guard<std::mutex> lock(attr_mu);
  if (!attr_set[dev][slot]) {
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax) != hipSuccess) return false;
    attr_set[dev][slot] = true;
  }
  return true;
}

// ------------------------------------------------------------------------------------------ shape, counts, workspace
// is (n_hidden, hidden[]) on the grid: 1 .. 5 layers, every width a multiple of 4 in [8, 400], zeros past n_hidden
static inline bool wide_shape_ok(int n_hidden, const int32_t* hidden) {
  if (n_hidden < 1 || n_hidden > kWideMaxHidden) return false;
  for (int l = 0; l < kWideMaxHidden; ++l) {
    const int w = hidden[l];
    if (l < n_hidden ? (w < 8 || w > kWideMaxWidth || w % 4 != 0) : w != 0) return false;
  }
  return true;
}
// The shape of a network: S2D_OK, or S2D_EINVAL with the text "prefix: <field> must be ..." set.  n_in: the input width where
// the caller chooses it (1 .. 256), else NULL.
int s2d_internal_wide_shape(const std::string& prefix, const int32_t* n_in, int n_hidden, const int32_t* hidden, int activation, int n_out);

// What a shape on the grid comes to: layer l has ceil(h_l / 16) tiles of 16 rows x its k-steps (ceil(n_in / 4) for layer 1,
// h_(l-1) / 4 after it) fragments of 64 words, and its biases are padded to its tiles.
struct WideCounts {
  int nfrag, nbias;          // fragments of all layers; words of the bias block behind them
  int wmax;                  // the widest hidden layer, padded to its tiles
  int na16;                  // outputs rounded up to 16
  uint64_t widths;           // h_l / 4 in bits 7 (l - 1) .. 7 l - 1; 0 past L
};
WideCounts s2d_internal_wide_counts(int n_in, int n_hidden, const int32_t* hidden, int n_out);
static inline size_t wide_workspace_bytes(int nfrag, int nbias) { return ((size_t)nfrag * kWave + nbias) * sizeof(float); }

// "n_in-h1-...-n_out"
std::string s2d_internal_wide_text(int n_in, int n_hidden, const int32_t* hidden, int n_out);
// The workspace of a network (`text`) that needs `need` bytes: S2D_OK, or S2D_EINVAL with the text set if it is NULL, not
// 256-byte aligned or too small.  bytes_fn: the entry point that tells the size.
int s2d_internal_wide_workspace(const std::string& prefix, const void* workspace, size_t workspace_bytes, size_t need, const std::string& text,
                                const char* bytes_fn);

// ------------------------------------------------------------------------------------------ the pack kernel
// what the pack kernel reads of a network
struct WidePackArgs {
  int n_in, n_hidden;
  uint64_t widths;           // as WideCounts
  int na, nfrag, nbias;
};
// params (nn.Sequential order) -> workspace in fragment order, then the biases: one launch on `stream`
void s2d_internal_wide_pack(const WidePackArgs& a, const float* params, void* workspace, hipStream_t stream);
// of a network as its kernels see it (Dims = WideDims with its input width, or s2d_td.hip's TdNetDev with its own)
template <typename Dims>
static inline WidePackArgs wide_pack_args(const Dims& d, int n_in) { return WidePackArgs{n_in, d.n_hidden, d.widths, d.na, d.nfrag, d.nbias}; }

// The actors' S2DWideNet with input width n_in.  Bytes of its workspace (n_hidden, hidden and n_out are read); 0 off the grid
static inline size_t wide_net_workspace_bytes(const S2DWideNet* shape, int n_in) {
  if (!shape || !wide_shape_ok(shape->n_hidden, shape->hidden) || shape->n_out < 1 || shape->n_out > 64) return 0;
  const WideCounts c = s2d_internal_wide_counts(n_in, shape->n_hidden, shape->hidden, shape->n_out);
  return wide_workspace_bytes(c.nfrag, c.nbias);
}
// and the workspace of a planned one: S2D_EINVAL with the text set if it is NULL, misaligned or too small
static inline int wide_net_workspace(const std::string& who, const S2DWideNet* net, const WidePackArgs& a, const char* bytes_fn) {
  return s2d_internal_wide_workspace(who, net->workspace, net->workspace_bytes, wide_workspace_bytes(a.nfrag, a.nbias),
                                     s2d_internal_wide_text(a.n_in, net->n_hidden, net->hidden, net->n_out), bytes_fn);
}

// ------------------------------------------------------------------------------------------ the plan
// VAR=waves,tiles in the environment, read at every launch, overrides a plan's choice of waves per workgroup and row tiles per
// pass (testing: the results do not depend on them).  0 = the plan's choice; ok: both are of {4, 2, 1} (or not given).
struct WidePlanOverride {
  int waves, tiles;
  bool ok;
  std::string text;          // "VAR=<what the variable holds>"
};
WidePlanOverride s2d_internal_plan_override(const char* var);
static inline std::string wide_plan_refusal(const WidePlanOverride& o) { return o.text + " is not waves,tiles of {4, 2, 1} that fit the LDS"; }

// The first of (waves, tiles) = (most, 4) (most, 2) (most, 1) (most / 2, 4) ... (1, 1) that the override allows and 160 KiB hold:
// more waves go before more tiles (one wave per workgroup leaves three SIMDs of the CU idle).  shared_words: the block-shared
// part; wave_words(tiles): a wave's part.  false if nothing fits (only under an override: (1, 1) fits every shape).
template <typename WaveWords>
static bool wide_plan_search(const WidePlanOverride& o, int most, size_t shared_words, WaveWords wave_words, int& waves, int& tiles, int& words,
                             size_t& lds) {
  if (!o.ok) return false;
  for (int wv = most; wv >= 1; wv /= 2) {
    if (o.waves && wv != o.waves) continue;
    for (int t = 4; t >= 1; t /= 2) {
      if (o.tiles && t != o.tiles) continue;
      const int ww = wave_words(t);
      const size_t bytes = (shared_words + (size_t)wv * ww) * sizeof(float);
      if (bytes <= kLdsMax) {
        waves = wv; tiles = t; words = ww; lds = bytes;
        return true;
      }
    }
  }
  return false;
}
