// s2d_match_host.h -- 11v11: the host side that every unit launching the cycle kernel needs.
//
// Holds: MRole, S2DMatchEngine, mfail, MHIP_TRY, MDeviceGuard, m_grid, the variant table, m_net_allow_lds, m_net_launch and
// m_dispatch, and the prototypes of the three launches that live in units of their own.  What exists once in the library (the
// non-template kernels, the arena layout, the C ABI) is s2d_match.hip's.
// Included by s2d_match.hip, s2d_match_reward.hip, s2d_match_see_policy.hip and s2d_match_belief_net.hip.
#pragma once
#include "s2d_match_cycle.h"

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// One agent-row network of an engine.  A role that is not set equals MRole{} (an empty slot mask).
struct MRole {
  bool set = false;                                    // a setter installed a network here: launches use the NET kernels (both roles: two passes)
  S2DMatchNet net{};                                   // ... its pointers (the caller's buffers, read at run time); a policy's epsilon is NULL
  bool pol = false;                                    // s2d_match_set_policy_network: a stochastic policy, launches use the POL kernels
  int act = 0;                                         // ... its hidden activation (0 relu, 1 tanh)
  const uint32_t* det = nullptr;                       // ... its deterministic word (the caller's, read at run time)
};
static_assert(S2D_MATCH_ROLE_NETWORK == 0 && S2D_MATCH_ROLE_OPPONENT == 1, "the roles index S2DMatchEngine::role, the other role is role ^ 1");
struct S2DMatchEngine {
  S2DMatchConfig cfg; MParams mp; float ptab[PT_WORDS][kHalf]; int64_t n, stride; int device;
  bool stock = false;                                  // mp's configuration words equal MStock: launches use the constant-folded kernels
  bool stock_types = false;                            // ... and every player is of the stock PlayerType (ptab's entries equal MStockTypes)
  bool stock_sched = false;                            // stock rules, physics and types, the engine's own schedule (MStockSched)
  bool has_ctl = false;                                // s2d_match_set_controllers installed a table: launches use the CTL kernels
  MRole role[2];                                       // the agent-row networks, by S2D_MATCH_ROLE_NETWORK / S2D_MATCH_ROLE_OPPONENT
  float* net_frags = nullptr;                          // the fragment-order copies the pack kernel writes (2 x kNetFragsMax words, one half per role)
  bool has_see = false;                                // s2d_match_set_see_network installed a see network: launches use the SEE kernels
  S2DMatchSeeNet see{};                                // ... its pointers and planes (the caller's buffers), its parameters (a copy)
  bool see_pol = false;                                // s2d_match_set_see_policy_network: `see` holds a policy (epsilon NULL), launches use the SEEPOL kernels
  int see_act = 0;                                     // ... its hidden activation (0 relu, 1 tanh)
  const uint32_t* see_det = nullptr;                   // ... its deterministic word (the caller's, read at run time)
  bool has_bel = false;                                // s2d_match_set_belief_network: `see` holds a belief network (see_act, see_det: its words;
                                                       // see.epsilon: head 0's), launches use the BEL kernels
  int bel_head = 0;                                    // ... its head: 0 epsilon-greedy Q-network, 1 categorical policy
  S2DBeliefParams bel_prm{};                           // ... the belief parameters (a copy)
  float* bel_rows = nullptr;                           // ... the caller's state buffer [N][popcount(bel_mask)][192]
  uint32_t bel_mask = 0;                               // ... and its layout
  uint32_t ctl_random = 0, ctl_script = 0;             // its slot masks (S2D_CTL_RANDOM, S2D_CTL_SCRIPTED)
  MAgentTab atab;                                      // per-slot words of s2d_match_agent_obs
  bool has_rw = false;                                 // s2d_match_set_agent_reward installed the weights: the reward record may be asked for
  MRw rw{nullptr, nullptr, 0};                         // ... the caller's weights (read at run time) and the chaser gate; out: per launch
  char* arena; size_t arena_bytes; bool owns_arena;
  S2DMatchBuffers buf; MPtrs ptrs;
};

// errors share the thread-local text of s2d_last_error() (defined in s2d_engine.hip)
extern "C" void s2d_internal_set_error(const char* msg);
static int mfail(int code, const std::string& msg) { s2d_internal_set_error(msg.c_str()); return code; }
#define MHIP_TRY(expr)                                                                          \
  do {                                                                                          \
    hipError_t _e = (expr);                                                                     \
    if (_e != hipSuccess) return mfail(S2D_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

struct MDeviceGuard {
  int prev = -1; bool ok = false;
  explicit MDeviceGuard(int dev) { if (hipGetDevice(&prev) == hipSuccess) ok = (prev == dev) || (hipSetDevice(dev) == hipSuccess); }
  ~MDeviceGuard() { if (ok && prev >= 0) (void)hipSetDevice(prev); }
};
static unsigned m_grid(int64_t n) { return (unsigned)((n + kEnvsPerBlock - 1) / kEnvsPerBlock); }

// The five variants of the cycle kernel, in the order an engine is tried against them, and the one this engine runs.
struct MVariant { bool stock, stock_types, sched, ill; const char* text; };
static constexpr MVariant kVariant[5] = {{true, true, true, false, "stock rules, own schedule"},
                                         {true, true, false, false, "stock, stock types"},
                                         {true, false, false, false, "stock"},
                                         {false, false, false, true, "general, illegal defense"},
                                         {false, false, false, false, "general"}};
static int m_variant(const S2DMatchEngine* h) {
  return h->stock_sched ? 0 : h->stock_types ? 1 : h->stock ? 2 : h->mp.illegal_defense_number > 0 ? 3 : 4;
}
// f(std::integral_constant<int, v>{}) for the run-time v: the variant as a compile-time index
template <class F> static int m_with_variant(int v, F&& f) {
  switch (v) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}

// NET instantiations: the dynamic LDS limit is a per-device property of the function; raise it once per (device, instantiation) to
// what the CU leaves beside the kernel's static LDS, under a lock (engines on several devices may be driven from several threads)
static constexpr size_t kNetLdsMax = 160 * 1024;   // gfx950: LDS of a CU, all of it available to one workgroup
static constexpr int kNetMaxDevices = 64;
static std::mutex m_net_lds_mutex;
template <auto Kernel> static bool m_net_allow_lds(size_t dyn) {
  static size_t limit[kNetMaxDevices] = {};            // of this instantiation, per device
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kNetMaxDevices) return false;
  std::lock_guard<std::mutex> lock(m_net_lds_mutex);
  if (!limit[dev]) {
    const void* const fn = reinterpret_cast<const void*>(Kernel);
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, fn) != hipSuccess || fa.sharedSizeBytes >= kNetLdsMax) return false;
    const size_t room = kNetLdsMax - fa.sharedSizeBytes;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)room) != hipSuccess) return false;
    limit[dev] = room;
  }
  return dyn <= limit[dev];
}
template <auto Kernel, class CA, class NA>
static int m_net_launch(dim3 grid, dim3 block, hipStream_t st, const MParams& mp, const MPtrs& ptrs, int64_t n, int n_steps,
                        const float* actions, const MRoll& ro, const CA& ctl /* MCtl, or MCtlRw */, const NA& na) {
  constexpr bool BEL = std::is_same<NA, MBelArg>::value, SEEPOL = std::is_same<NA, MSeePolArg>::value;
  constexpr bool SEE = std::is_same<NA, MSeeArg>::value || SEEPOL || BEL;
  // The belief network's budget: W2 .. b3 of a 192-64-64-64 network are 33 536 B, a wave's tile, facts, index and log-probability
  // words 20 096 B and its two staging rows with their scratch 3 072 B: 33 536 + 4 x 23 168 = 126 208 B beside at most 14 576 B.
  constexpr int wave_words = BEL ? kBelWaveWords : SEEPOL ? kSeePolWaveWords : SEE ? kSeeWaveWords
                             : std::is_same<NA, MPolArg>::value ? kPolWaveWords : kNetWaveWords;
  constexpr const char* what = BEL ? "the belief network's LDS (its weights, tiles and staging rows: " : "the network's LDS (";
  size_t dyn = ((size_t)na.net.shared_words + (size_t)(kMBlock / 64) * wave_words) * sizeof(float);
  if constexpr (!SEE) {
    // The budget: a 64-64-64 network's W2 .. b3 are 33 536 B, a wave's tile, facts and index words 20 784 B, so two widest
    // networks ask for 2 x 33 536 + 4 x 20 784 = 150 208 B.  Beside the stock kernels' 12 288 B of static LDS the CU leaves
    // 151 552 B: they fit.  Beside the general kernels' 14 208 / 14 576 B (their parameter block) it leaves 149 632 / 149 264 B:
    // there two networks of 64-64-(49..64) do not fit, and the second one's W2 .. b3 stay in memory (the kernel reads them
    // there, the same words in the same order).  Every other pair fits every kernel.
    // The POL kernels' waves hold 64 more words each (kPolWaveWords): 151 232 B for the widest pair, which the stock kernels
    // still stage; the general ones fall back as above.
    const size_t second = (size_t)na.net.opp.shared_words * sizeof(float);
    dyn += second;
    if (second != 0 && !m_net_allow_lds<Kernel>(dyn)) {
      NA unstaged = na;
      unstaged.net.opp.shared_words = 0;
      if (!m_net_allow_lds<Kernel>(dyn - second))
        return mfail(S2D_EHIP, "the network's LDS (" + std::to_string(dyn - second) + " B) does not fit beside the cycle kernel's");
      hipLaunchKernelGGL(Kernel, grid, block, dyn - second, st, mp, ptrs, n, n_steps, actions, ro, ctl, unstaged);
      return S2D_OK;
    }
  }
  if (!m_net_allow_lds<Kernel>(dyn))
    return mfail(S2D_EHIP, std::string(what) + std::to_string(dyn) + " B) does not fit beside the cycle kernel's");
  hipLaunchKernelGGL(Kernel, grid, block, dyn, st, mp, ptrs, n, n_steps, actions, ro, ctl, na);
  return S2D_OK;
}

// One launch of the instantiation this engine runs; CTL (with one MCtl in `extra`): the controller variant of the same one;
// NET (with an MCtl and an MNetArg, MPolArg or MSeeArg): the network variant, with its dynamic LDS.
template <bool CTL, bool NET = false, class... X>
static int m_dispatch(S2DMatchHandle h, int n_steps, const float* actions, const MRoll& ro, hipStream_t st, X... extra) {
  MDeviceGuard guard(h->device);
  const dim3 grid(m_grid(h->n)), block(kMBlock);
  const int rc = m_with_variant(m_variant(h), [&](auto v) -> int {
    constexpr MVariant V = kVariant[decltype(v)::value];
    constexpr auto kernel = s2d_match_rollout_kernel<V.stock, V.stock_types, V.sched, V.ill, CTL, NET, X...>;
    if constexpr (NET) return m_net_launch<kernel>(grid, block, st, h->mp, h->ptrs, h->n, n_steps, actions, ro, extra...);
    else hipLaunchKernelGGL(kernel, grid, block, 0, st, h->mp, h->ptrs, h->n, n_steps, actions, ro, extra...);
    return S2D_OK;
  });
  if (rc != S2D_OK) return rc;
  MHIP_TRY(hipGetLastError());
  return S2D_OK;
}

// The launches that live in units of their own (s2d_match.hip's m_launch says when each runs).
// s2d_match_reward.hip, the RW instantiations -- na: the network launch, pa: the policy launch, neither: the controller launch.
int s2d_match_internal_reward_launch(S2DMatchHandle h, int n_steps, const float* actions, const MRoll& ro, hipStream_t st, const MCtlRw& ctl,
                                     const MNetArg* na, const MPolArg* pa);
// s2d_match_see_policy.hip, the SEEPOL instantiations.
int s2d_match_internal_see_policy_launch(S2DMatchHandle h, int n_steps, const float* actions, const MRoll& ro, hipStream_t st,
                                         const MCtl& ctl, const MSeePolArg& pa);
// s2d_match_belief_net.hip, the BEL instantiations.
int s2d_match_internal_belief_net_launch(S2DMatchHandle h, int n_steps, const float* actions, const MRoll& ro, hipStream_t st,
                                         const MCtl& ctl, const MBelArg& ba);
