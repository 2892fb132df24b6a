// s2d_match_cycle.h -- 11v11: the cycle kernel.
//
// Holds: MRoll, MShared, match_rollout_body, the argument pickers and the template s2d_match_rollout_kernel, whose instantiations
// the match units divide among themselves (s2d_match.hip, s2d_match_reward.hip, s2d_match_see_policy.hip, s2d_match_belief_net.hip).
// Included by s2d_match_host.h (and through it by those units).
#pragma once
#include "s2d_match_slots.h"

struct MRoll { float* obs; float* reward; int32_t* mode; uint8_t* done; };

// n_steps cycles; actions = [T][N][22][3] or NULL (random policy).  n_steps = 1 with ro = {} is the per-step API.
struct MShared {                                      // the workgroup's LDS (declared by the kernel)
  float4 (*pos_tile)[kTileSlots]; PTab* pt; unsigned int* lds_cnt; MRare* rare; float (*obs_tile)[2 * SLOTS * S2D_MATCH_OBJ_WORDS];
};
// CTL: the slots' controllers come from `ctl` (per-slot: caller's row, random, scripted) and the record of what they chose is written
// when ctl.actions_out is set; otherwise every slot takes the caller's row, or the random policy when actions == NULL.
// NET (with CTL): the network slots of `nin` override the table: the action of the caller's network on the slot's agent row.
// NA = MSeeArg (with NET): the see network -- the network acts on the slot's see row and chooses the view action too; the vision
// state of all 22 players is stepped here, once per cycle, after the body cycle.
// RW (with CTL, not SEE): the agent reward record of `rw`.  A lane's start-of-cycle words are the end-of-cycle ones of the cycle
// before, carried in registers; the start-of-cycle mode and card are read before the cycle.
template <bool CTL, bool NET = false, bool RW = false, class P, class TY, class NA = MNetArg>
S2D_DEV void match_rollout_body(const P& p, const TY& pt, const MShared& sh, const MPtrs& q, int64_t n, int n_steps,
                                const float* __restrict__ actions, const MRoll& ro, const MCtl& ctl, const NA* nin = nullptr,
                                const MRw& rw = MRw{nullptr, nullptr, 0}) {
  static_assert(!RW || (CTL && !(NET && (std::is_same<NA, MSeeArg>::value || std::is_same<NA, MSeePolArg>::value ||
                                         std::is_same<NA, MBelArg>::value))),
                "the agent reward: the CTL family, not the see network");
  constexpr bool SEEPOL = NET && std::is_same<NA, MSeePolArg>::value;   // see policy slots: SEE with the policy's head and record
  constexpr bool BEL = NET && std::is_same<NA, MBelArg>::value;   // belief network: SEE on belief rows, either head, the policy's record
  constexpr bool SEE = NET && (std::is_same<NA, MSeeArg>::value || SEEPOL || BEL);
  constexpr bool POL = NET && std::is_same<NA, MPolArg>::value;   // policy slots: an instantiation of its own (the NET ones keep their code)
  const int l = threadIdx.x & (kHalf - 1), l_launch = l;
  const int half = (threadIdx.x >> 5) & 1, half_launch = half;
  const int64_t e = (int64_t)blockIdx.x * kEnvsPerBlock + threadIdx.x / kHalf;
  const bool valid = e < n;
  const int64_t ec = valid ? e : n - 1;              // lanes of out-of-range matches shadow the last match (no stores)
  MObj o; MGame g;
  MRare& r = sh.rare[threadIdx.x / kHalf];
  m_load(q, ec, l, o, g, r);
  float vneck = 0.0f; int vwidth = 0, vwait = 0;          // SEE: the vision state of this lane's player, in registers for the launch
  if constexpr (SEE) {
    if (l < NP) {
      const int64_t k = ec * SLOTS + l;
      vneck = nin->vis.neck[k]; vwidth = nin->vis.view_width[k]; vwait = nin->vis.see_wait[k];
    }
  }
  m_derive(p, g);
  tile_init(sh.pos_tile[threadIdx.x / kHalf], l, pt[PT_SIZE][l]);
  const uint64_t gid = (((uint64_t)p.gid_hi << 32) | p.gid_lo) + (uint64_t)ec;
  const uint32_t gl = (uint32_t)gid, gh = (uint32_t)(gid >> 32);
  MCounts cnt{sh.lds_cnt, valid, 0u};
  U4 pol{0, 0, 0, 0};                                     // the policy block of the current pair of cycles
  // The state loaded above is first used inside the loop, and that is where the compiler would wait for it -- with s_waitcnt
  // vmcnt(k), a counter that on gfx9 also counts STORES: from the second cycle on those waits would hold the wave until the
  // previous cycles' record stores had been acknowledged by memory.  Waiting for the loads here leaves no wait in the loop.
  __builtin_amdgcn_s_waitcnt(0x0F70);                     // vmcnt(0)
  // The record rows of cycle t lie n matches behind those of cycle t - 1: one uniform pointer per array, advanced once per cycle
  // (scalar adds), plus a small per-lane offset inside the workgroup's stretch of the row -- 32 bits, so the stores take their base
  // from scalar registers.  (Formed per cycle from t, n and the match index, the four addresses were 64-bit vector arithmetic: ~45
  // of the cycle's ~550 vector instructions.)
  constexpr int kVecPerMatch = SLOTS * S2D_MATCH_OBJ_WORDS / 4;   // 30 float4 per match
  const int64_t eb = (int64_t)blockIdx.x * kEnvsPerBlock;  // the workgroup's first match
  char* obs_row = reinterpret_cast<char*>(ro.obs) + eb * (int64_t)(kVecPerMatch * 16);
  float* reward_row = ro.reward + eb; int32_t* mode_row = ro.mode + eb; uint8_t* done_row = ro.done + eb;
  float* act_row = CTL ? ctl.actions_out + eb * (NP * 3) : nullptr;   // the action record: [T][N][22][3], same scheme
  [[maybe_unused]] float* rw_row = RW ? rw.out + eb * NP : nullptr;   // the agent reward record: [T][N][22], same scheme
  const uint32_t lane = threadIdx.x & 63u, m_in_wg = threadIdx.x / kHalf;
  const uint32_t obs_off = ((threadIdx.x >> 6) * 2u * kVecPerMatch + lane) * 16u;
  const int64_t e0 = e - half;                             // first match of this wave (matches of a wave: e0, e0 + 1)
  const bool obs_lane = (int)lane < (e0 + 1 < n ? 2 * kVecPerMatch : (e0 < n ? kVecPerMatch : 0));
  float* const obs_slot = sh.obs_tile[threadIdx.x >> 6] + (half * SLOTS + l) * S2D_MATCH_OBJ_WORDS;
  const float4* const obs_vec = reinterpret_cast<const float4*>(sh.obs_tile[threadIdx.x >> 6]) + lane;
  // Fair shares of the SIMD.  Among waves of equal priority the issue arbiter prefers the OLDEST: of the four waves a SIMD holds,
  // the first one dispatched ran its 64 cycles in 322 k clocks, the fourth in 470 k (profiles/r03/match_wave_durations.txt) -- same
  // work, and the launch waits for the fourth.  The waves therefore take turns at the four priority levels, a new turn every four
  // cycles, starting from their slot number on the SIMD (HW_ID.wave_id): at any time the four hold four different levels, and over
  // a launch every wave spends the same time at each.
  const int simd_slot = (int)__builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 4);   // HW_REG_HW_ID bits 3:0
  uint64_t net_thr = 0;
  uint32_t net_slots = 0u, net_k = 0u;                     // NET: the slots on a network; this lane's network: its K and table
  const float* net_tab = nullptr;
  [[maybe_unused]] uint32_t pol_det = 0u;                  // POL, SEEPOL: the passes' deterministic words, read once per launch like epsilon
  if constexpr (POL) {
    const MPol& pl = nin->pol;
    if (pl.kind[0]) pol_det |= *pl.det[0] != 0u ? 1u : 0u;
    if (pl.kind[1]) pol_det |= *pl.det[1] != 0u ? 2u : 0u;
    // a policy has no epsilon (its pointer is NULL): the thresholds below are read for the Q-network passes only
    net_thr = nin->net.net_mask && !pl.kind[0] ? explore_threshold(*nin->net.epsilon) : 0;
    net_slots = nin->net.net_mask; net_k = (uint32_t)nin->net.na; net_tab = nin->net.table;
    if (nin->net.opp.mask != 0u) {
      const uint64_t thr2 = pl.kind[1] ? 0 : explore_threshold(*nin->net.opp.epsilon);
      net_slots |= nin->net.opp.mask;
      if ((nin->net.opp.mask >> l) & 1u) { net_thr = thr2; net_k = (uint32_t)nin->net.opp.na; net_tab = nin->net.opp.table; }
    }
  } else if constexpr (BEL) {                              // (the launch's head reads its own word; the other's pointer is NULL)
    if (nin->head != 0) pol_det = *nin->det != 0u ? 1u : 0u;
    else net_thr = explore_threshold(*nin->net.epsilon);
    net_slots = nin->net.net_mask; net_k = (uint32_t)nin->net.na; net_tab = nin->net.table;
  } else if constexpr (SEEPOL) {                           // (no epsilon: its pointer is NULL)
    pol_det = *nin->det != 0u ? 1u : 0u;
    net_slots = nin->net.net_mask; net_k = (uint32_t)nin->net.na; net_tab = nin->net.table;
  } else if constexpr (NET) {
    net_thr = nin->net.net_mask ? explore_threshold(*nin->net.epsilon) : 0;   // (records only: no network)
    net_slots = nin->net.net_mask; net_k = (uint32_t)nin->net.na; net_tab = nin->net.table;
    if constexpr (!SEE) {
      if (nin->net.opp.mask != 0u) {                       // the second network: its slots take its threshold, K and table
        const uint64_t thr2 = explore_threshold(*nin->net.opp.epsilon);
        net_slots |= nin->net.opp.mask;
        if ((nin->net.opp.mask >> l) & 1u) { net_thr = thr2; net_k = (uint32_t)nin->net.opp.na; net_tab = nin->net.opp.table; }
      }
    }
  }
  [[maybe_unused]] bool bel_reset = false;                 // BEL: the match's done of the cycle before (first cycle: the engine's plane)
  if constexpr (BEL) bel_reset = nin->done0[ec] != 0;
  [[maybe_unused]] MRwView rw_view{0.0f, 0.0f, 0.0f, 0.0f};      // RW: this lane's words of the current state
  [[maybe_unused]] float rw_w[S2D_MATCH_REWARD_TERMS] = {};
  if constexpr (RW) {
    rw_view = m_reward_view(o, l, half);
#pragma unroll
    for (int k = 0; k < S2D_MATCH_REWARD_TERMS; ++k) rw_w[k] = rw.w[k];   // (uniform: scalar loads)
  }
  for (int t = 0; t < n_steps; ++t) {
    if ((t & 3) == 0) {
      switch ((simd_slot + (t >> 2)) & 3) {
        case 0: __builtin_amdgcn_s_setprio(0); break;
        case 1: __builtin_amdgcn_s_setprio(1); break;
        case 2: __builtin_amdgcn_s_setprio(2); break;
        default: __builtin_amdgcn_s_setprio(3); break;
      }
    }
    // Everything that depends only on the lane number -- masks such as "is a player", "is the ball", bit positions, Philox block
    // words -- is loop-invariant, and the compiler computes it all once per launch and keeps it: ~90 scalar and ~20 vector
    // registers more than there are, spilled and reloaded inside the loop.  One instruction each to recompute: opaque copies of
    // the lane number and the half make them per-cycle values.
    int l = l_launch, half = half_launch;
    asm volatile("" : "+v"(l), "+v"(half));
    [[maybe_unused]] int rw_mode0 = 0;                     // RW: the start-of-cycle mode, card and gate
    [[maybe_unused]] bool rw_act0 = false, rw_gate0 = false;
    if constexpr (RW) {
      rw_mode0 = g.mode; rw_act0 = o.card < S2D_CARD_RED;
      rw_gate0 = m_reward_gate(o, rw_view, rw.chaser_only, l);
    }
    int cmd = S2D_MCMD_NONE; float a = 0.0f, b = 0.0f;
    float view_m = 0.0f, view_c = 0.0f;                    // SEE: this slot's view action (TurnNeck moment, ChangeView code) ...
    bool view_act = false;                                 // ... and whether it has one
    if constexpr (CTL) {
      int scmd = S2D_MCMD_NONE; float sa = 0.0f, sb = 0.0f;
      if (ctl.script_mask != 0u) m_scripted_action(p, pt, o, g, r, l, half, scmd, sa, sb);   // (uniform: a kernel argument)
      int nidx = -1;                                       // NET: the network's index of this slot, -1 = not a network slot
      if constexpr (NET) {
        int greedy;
        [[maybe_unused]] float lp = 0.0f;
        if constexpr (BEL) {
          const MPick pick = m_see_greedy(p, *nin, o, g, vneck, vwidth, vwait, l, half, valid, gid, (int64_t)t * n + ec, pol_det != 0u,
                                          ec, bel_reset);
          greedy = pick.idx; lp = pick.logp;
        }
        else if constexpr (SEEPOL) {
          const MPick pick = m_see_greedy(p, *nin, o, g, vneck, vwidth, vwait, l, half, valid, gid, (int64_t)t * n + ec, pol_det != 0u);
          greedy = pick.idx; lp = pick.logp;
        }
        else if constexpr (SEE) greedy = m_see_greedy(p, *nin, o, g, vneck, vwidth, vwait, l, half, valid, gid, (int64_t)t * n + ec);
        else if constexpr (POL) {
          const MPick pick = m_net_greedy(p, *nin, o, g, r, l, half, valid, (int64_t)t * n + ec, pol_det, gl, gh);
          greedy = pick.idx; lp = pick.logp;
        }
        else greedy = m_net_greedy(p, *nin, o, g, r, l, half, valid, (int64_t)t * n + ec);
        if (l < NP && ((net_slots >> l) & 1u)) {           // explore: word x < thr, then the index is word y's draw below K
          bool pol_lane = false;                           // POL: the slot is on a policy: its head has sampled (word z of this block)
          if constexpr (POL)
            pol_lane = (nin->pol.kind[0] && ((nin->net.net_mask >> l) & 1u)) || (nin->pol.kind[1] && ((nin->net.opp.mask >> l) & 1u));
          if constexpr (SEEPOL) pol_lane = true;           // (every network slot is the policy's)
          if constexpr (BEL) pol_lane = nin->head != 0;    // (... or the Q-network's: the draw below)
          if (pol_lane) {
            nidx = greedy;
          } else {
            const U4 w = m_draw(p, gl, gh, (uint32_t)g.tick, S2D_ST_NET, (uint32_t)l);
            nidx = (uint64_t)w.x < net_thr ? rnd_below(w.y, net_k) : greedy;
          }
        }
        if constexpr (POL) {
          // (wave-uniform pointer; 0.0f for every slot that is not on a policy)
          if (nin->pol.logp && valid && l < NP) nin->pol.logp[((int64_t)t * n + e) * NP + l] = lp;
        }
        if constexpr (SEEPOL || BEL) {
          if (nin->logp && valid && l < NP) nin->logp[((int64_t)t * n + e) * NP + l] = lp;
        }
        if (nin->net.net_index && valid && l < NP) nin->net.net_index[((int64_t)t * n + e) * NP + l] = nidx;
      }
      if (l < NP) {
        const uint32_t bit = 1u << l;
        if (NET && nidx >= 0) {
          if constexpr (SEE) {
            const float* tr = net_tab + 5 * nidx;
            cmd = (int)tr[0]; a = tr[1]; b = tr[2]; view_m = tr[3]; view_c = tr[4]; view_act = true;
          } else {
            const float* tr = net_tab + 3 * nidx;
            cmd = (int)tr[0]; a = tr[1]; b = tr[2];
          }
        } else if (ctl.script_mask & bit) {
          cmd = scmd; a = sa; b = sb;
        } else if (ctl.random_mask & bit) {
          m_random_action(p, gl, gh, (uint32_t)g.tick, l, t == 0, pol, cmd, a, b);
        } else {
          const float* ap = actions + (((int64_t)t * n + ec) * NP + l) * 3;
          cmd = (int)ap[0]; a = ap[1]; b = ap[2];
        }
        if constexpr (SEE) {
          if (nidx < 0 && nin->net.view_actions) {         // (the pointer: wave-uniform)
            const float* vp = nin->net.view_actions + (((int64_t)t * n + ec) * NP + l) * 2;
            view_m = vp[0]; view_c = vp[1]; view_act = true;
          }
        }
      }
      if (ctl.actions_out) {                               // wave-uniform
        if (valid && l < NP) {
          float* w = act_row + (m_in_wg * NP + l) * 3;
          w[0] = (float)cmd; w[1] = a; w[2] = b;
        }
        act_row += n * (NP * 3);
      }
    } else if (l < NP) {
      if (actions) {
        const float* ap = actions + (((int64_t)t * n + ec) * NP + l) * 3;
        cmd = (int)ap[0]; a = ap[1]; b = ap[2];
      } else {
        m_random_action(p, gl, gh, (uint32_t)g.tick, l, t == 0, pol, cmd, a, b);
      }
    }
    match_cycle(p, pt, o, g, r, l, half, gl, gh, cmd, a, b, cnt, sh.pos_tile[threadIdx.x / kHalf]);
    if constexpr (SEE) {                                   // the vision step: this cycle's done, the card after the body cycle
      if (l < NP) s2d_see::vision_advance(nin->sp, vneck, vwidth, vwait, g.done != 0, o.card >= S2D_CARD_RED, view_act, view_m, view_c);
    }
    if constexpr (BEL) bel_reset = g.done != 0;            // a finished match's rows are forgotten at the next row
    if (ro.obs) {                                          // wave-uniform
      if (l < SLOTS) { obs_slot[0] = o.x; obs_slot[1] = o.y; obs_slot[2] = o.vx; obs_slot[3] = o.vy; obs_slot[4] = o.body; }
      wave_fence();
      if (obs_lane) *reinterpret_cast<float4*>(obs_row + obs_off) = *obs_vec;
      wave_fence();
      obs_row += n * (int64_t)(kVecPerMatch * 16);
    }
    if (valid && l == BALL) {
      if (ro.reward) reward_row[m_in_wg] = g.reward;
      if (ro.mode) mode_row[m_in_wg] = g.mode;
      if (ro.done) done_row[m_in_wg] = (uint8_t)g.done;
    }
    reward_row += n; mode_row += n; done_row += n;         // (never dereferenced when the array is absent)
    if constexpr (RW) {
      const MRwView v1 = m_reward_view(o, l, half);
      const float rwd = m_agent_reward(rw_view, rw_mode0, rw_act0, rw_gate0, v1, o, g, pt[PT_KICKABLE_AREA2][l], rw_w, l);
      if (valid && l < NP) rw_row[m_in_wg * NP + l] = rwd;
      rw_row += n * NP;
      rw_view = v1;
    }
  }
  match_nearest(o, g, l);
  if (valid) m_store(q, e, l, o, g, r);
  if constexpr (SEE) {
    if (valid && l < NP) {
      const int64_t k = e * SLOTS + l;
      nin->vis.neck[k] = vneck; nin->vis.view_width[k] = vwidth; nin->vis.see_wait[k] = vwait;
    }
  }
  {                                                     // tackles: per-lane counters -> wave sum -> LDS
    unsigned int tk = valid ? cnt.tackles : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tk += __shfl_down(tk, off);
    if ((threadIdx.x & 63) == 0 && tk) atomicAdd(&sh.lds_cnt[5], tk);
  }
  m_flush_counts(q.stats, sh.lds_cnt);
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&q.stats[0], (unsigned long long)n * (unsigned long long)n_steps);
}

// STOCK: the configuration words are MStock's constants (m_is_stock() said they equal this engine's); else they are read from LDS.
// STOCK_TYPES (with STOCK): all 22 players of the stock PlayerType, the table's entries are constants too.
// SCHED (with STOCK and STOCK_TYPES): the schedule words are the engine's own (MStockSched).  ILL (general only): the engine has
// IllegalDefense_ switched on.
// CTL: per-slot controllers (MCtl, the one extra argument: the instantiations without it keep their argument list and code).
// NET (with CTL): network slots (MNetArg, a second extra argument), the network's LDS in dynamic shared memory; one workgroup per CU
// holds it, so these instantiations have the register file of one wave per SIMD.
// SEE: the NET instantiations whose second extra argument is an MSeeArg -- the see network, a family of its own (the existing
// instantiations keep their template and kernel arguments).
// POL: the NET instantiations whose second extra argument is an MPolArg -- policy slots, likewise a family of its own: a launch
// takes one only when a role holds a policy network, so the NET kernels and their LDS plan are what they were.
// SEEPOL: the SEE instantiations whose second extra argument is an MSeePolArg -- see policy slots, a family of its own as well,
// instantiated in a translation unit of its own (s2d_match_see_policy.hip): the SEE kernels are what they were.
// BEL: the SEE instantiations whose second extra argument is an MBelArg -- the belief network, a family of its own too,
// instantiated in a translation unit of its own (s2d_match_belief_net.hip): the SEE and SEEPOL kernels are what they were.
// RW: the CTL / NET / POL instantiations whose first extra argument is an MCtlRw -- the agent reward record, likewise a family of
// its own, instantiated in a translation unit of its own (s2d_match_reward.hip): this unit's kernels are what they were.
S2D_DEV MCtl m_ctl_arg() { return MCtl{0u, 0u, nullptr}; }
S2D_DEV MCtl m_ctl_arg(const MCtl& c) { return c; }
S2D_DEV MCtl m_ctl_arg(const MCtl& c, const MNetArg&) { return c; }
S2D_DEV MCtl m_ctl_arg(const MCtl& c, const MSeeArg&) { return c; }
S2D_DEV MCtl m_ctl_arg(const MCtl& c, const MPolArg&) { return c; }
S2D_DEV MCtl m_ctl_arg(const MCtl& c, const MSeePolArg&) { return c; }
S2D_DEV MCtl m_ctl_arg(const MCtl& c, const MBelArg&) { return c; }
template <class... A> S2D_DEV MCtl m_ctl_arg(const MCtlRw& c, const A&...) { return c.ctl; }
S2D_DEV const MNetArg* m_net_arg() { return nullptr; }
S2D_DEV const MNetArg* m_net_arg(const MCtl&) { return nullptr; }
S2D_DEV const MNetArg* m_net_arg(const MCtl&, const MNetArg& a) { return &a; }
S2D_DEV const MSeeArg* m_net_arg(const MCtl&, const MSeeArg& a) { return &a; }
S2D_DEV const MPolArg* m_net_arg(const MCtl&, const MPolArg& a) { return &a; }
S2D_DEV const MSeePolArg* m_net_arg(const MCtl&, const MSeePolArg& a) { return &a; }
S2D_DEV const MBelArg* m_net_arg(const MCtl&, const MBelArg& a) { return &a; }
S2D_DEV const MNetArg* m_net_arg(const MCtlRw&) { return nullptr; }
template <class A> S2D_DEV const A* m_net_arg(const MCtlRw&, const A& a) { return &a; }
template <class... A> S2D_DEV MRw m_rw_arg(const A&...) { return MRw{nullptr, nullptr, 0}; }
template <class... A> S2D_DEV MRw m_rw_arg(const MCtlRw& c, const A&...) { return c.rw; }
template <class... A> struct MIsSee : std::false_type {};
template <> struct MIsSee<MCtl, MSeeArg> : std::true_type {};
template <> struct MIsSee<MCtl, MSeePolArg> : std::true_type {};
template <> struct MIsSee<MCtl, MBelArg> : std::true_type {};
template <class... A> struct MIsPol : std::false_type {};
template <> struct MIsPol<MCtl, MPolArg> : std::true_type {};
template <> struct MIsPol<MCtlRw, MPolArg> : std::true_type {};
template <class... A> struct MIsRw : std::false_type {};
template <class... A> struct MIsRw<MCtlRw, A...> : std::true_type {};
template <bool STOCK, bool STOCK_TYPES, bool SCHED = false, bool ILL = false, bool CTL = false, bool NET = false, class... CtlArg>
__global__ __launch_bounds__(kMBlock, NET ? 1 : 4) void s2d_match_rollout_kernel(MParams p_arg, MPtrs q, int64_t n, int n_steps,
                                                                     const float* __restrict__ actions, MRoll ro, CtlArg... ctl_arg) {
  static_assert(sizeof...(CtlArg) == (NET ? 2 : CTL ? 1 : 0), "the CTL instantiations take an MCtl, NET ones an MNetArg too, the others nothing more");
  static_assert(!NET || CTL, "network slots come with the controller table");
  constexpr bool SEE = MIsSee<CtlArg...>::value;
  constexpr bool POL = MIsPol<CtlArg...>::value;
  constexpr bool RW = MIsRw<CtlArg...>::value;
  static_assert(!RW || !SEE, "the see network has no agent reward");
  const MCtl ctl = m_ctl_arg(ctl_arg...);
  [[maybe_unused]] const MRw rw = m_rw_arg(ctl_arg...);
  const auto* const nin = m_net_arg(ctl_arg...);
  __shared__ float4 pos_tile[kEnvsPerBlock][kTileSlots];
  __shared__ PTab pt[PT_WORDS];                       // per-slot PlayerType parameters, shared by the 8 matches
  __shared__ unsigned int lds_cnt[8];
  __shared__ MRare rare[kEnvsPerBlock];                // per-match words only events touch (see MRare)
  // rollout observations: the two matches of a wave are neighbours in [T][N][24][5], i.e. 960 contiguous bytes per cycle.  Each lane
  // puts its five words into a wave-private tile (stride 5: no bank conflicts) and the wave stores the block as 60 x 16 bytes --
  // instead of five 20-byte-strided dword stores per lane (partial lines: what the reach kernels' store-pattern study priced)
  __shared__ __attribute__((aligned(16))) float obs_tile[kMBlock / 64][2 * SLOTS * S2D_MATCH_OBJ_WORDS];
  const MShared sh{pos_tile, pt, lds_cnt, rare, obs_tile};
  static_assert(STOCK || !STOCK_TYPES, "constant types come with constant rules");
  if constexpr (!STOCK_TYPES)
    for (int k = threadIdx.x; k < PT_WORDS * kHalf; k += kMBlock) (&pt[0][0])[k] = q.ptab[k];
  if (threadIdx.x < 8) lds_cnt[threadIdx.x] = 0u;
  if constexpr (SEE) m_see_stage(nin->net);              // (the barrier of every branch below covers it)
  else if constexpr (NET) m_net_stage(nin->net);
  static_assert(!SCHED || (STOCK && STOCK_TYPES), "the engine's own schedule comes with constant rules and types");
  if constexpr (SCHED) {
    __syncthreads();
#define X(name) , p_arg.name
    const MStockSched p{p_arg.auto_reset, p_arg.noise, p_arg.seed_lo, p_arg.seed_hi, p_arg.gid_lo, p_arg.gid_hi M_SCHEDULE_INTS(X)};
#undef X
    const MStockTypes types{__int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(q.ptab[PT_KICKABLE_AREA2 * kHalf])))};
    match_rollout_body<CTL, NET, RW>(p, types, sh, q, n, n_steps, actions, ro, ctl, nin, rw);
  } else if constexpr (STOCK) {
    __syncthreads();
    const MStock p{p_arg.auto_reset, p_arg.noise, p_arg.penalty_shoot_outs, p_arg.seed_lo, p_arg.seed_hi, p_arg.gid_lo, p_arg.gid_hi};
    if constexpr (STOCK_TYPES) {
      const MStockTypes types{__int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(q.ptab[PT_KICKABLE_AREA2 * kHalf])))};
      match_rollout_body<CTL, NET, RW>(p, types, sh, q, n, n_steps, actions, ro, ctl, nin, rw);
    } else {
      match_rollout_body<CTL, NET, RW>(p, static_cast<const PTab*>(pt), sh, q, n, n_steps, actions, ro, ctl, nin, rw);
    }
  } else {
    // The ~70 uniform parameters are read from LDS (broadcast reads) where they are used instead of
    // occupying SGPRs for the whole kernel: as kernargs they cost 142 SGPR spills and 48 B of scratch at
    // the 128-VGPR cap (26 spills / 12 B this way, +14 % throughput).
    static_assert(!ILL || !STOCK, "the stock configurations have the rule off");
    // The CTL kernels read the block through a type of their own (no data added): every helper templated on it is then an
    // instantiation of theirs.  Helpers shared with the CTL kernels were optimised differently in the kernels without them.
    // The NET kernels likewise (sharing the CTL kernels' type changed those kernels' code), and the SEE kernels.
    using PBase = std::conditional_t<ILL, MParams, MParamsNoIll>;
    using PBlockNet = std::conditional_t<POL, MParamsPol<PBase>, MParamsNet<PBase>>;
    using PBlock = std::conditional_t<SEE, MParamsSee<PBase>,
                                      std::conditional_t<NET, PBlockNet, std::conditional_t<CTL, MParamsCtl<PBase>, PBase>>>;
    __shared__ PBlock p_lds;
    static_assert(sizeof(MParams) / 4 <= kMBlock, "one thread per parameter word");
    if (threadIdx.x < sizeof(MParams) / 4)
      reinterpret_cast<uint32_t*>(&p_lds)[threadIdx.x] = reinterpret_cast<const uint32_t*>(&p_arg)[threadIdx.x];
    __syncthreads();
    match_rollout_body<CTL, NET, RW>(p_lds, static_cast<const PTab*>(pt), sh, q, n, n_steps, actions, ro, ctl, nin, rw);
  }
}
