// s2d_match_slots.h -- 11v11: what a slot of the cycle kernel can be driven by and what it reports.
//
// Holds: the agent observations (facts and rows) and the agent reward, the network slots, the policy slots, the see network and
// the see policy, the belief network -- device code only, on top of the rule book of s2d_match_rules.h.
// Included by s2d_match_cycle.h (and through it by the match units).
#pragma once
#include "s2d_match_rules.h"
#include "s2d_belief_row.h"

// Per-agent observations (include/s2d_match.h, s2d_match_agent_obs).  Per-slot words the cycle kernels do not keep (the PT table
// stays as it is): built on the host at create time, passed by value.
struct MAgentTab {
  float ka[kHalf], ka2[kHalf], speed_max[kHalf], kick_rate[kHalf], inv_margin[kHalf], size[kHalf], type_id[kHalf];
  float ball_size, ball_decay;
};
constexpr int kAObsVec = S2D_AGENT_OBS_DIM / 4;                       // 56 float4 per row
static_assert(S2D_AGENT_OBS_DIM % 4 == 0 && kAObsVec <= 2 * kHalf, "a half-wave stores a row as two float4 per lane");
static_assert(S2D_AGENT_OBS_TEAMMATES == 48 && S2D_AGENT_OBS_OPPONENTS == 136 && S2D_AGENT_OBS_ROW_WORDS == 8, "row layout");
constexpr uint32_t kOurSetPlayModes = (1u << S2D_GM_KICK_OFF) | (1u << S2D_GM_KICK_IN) | (1u << S2D_GM_FREE_KICK) |
                                      (1u << S2D_GM_CORNER_KICK) | (1u << S2D_GM_GOAL_KICK) | (1u << S2D_GM_IND_FREE_KICK) |
                                      (1u << S2D_GM_GOALIE_CATCH) | (1u << S2D_GM_PENALTY_KICK);
struct MAObsFacts {                                    // one match (half-wave): the lanes' facts
  float x[kHalf], y[kHalf], vx[kHalf], vy[kHalf], reach[kHalf], catch_ban[kHalf];
  int rank_slot[2][3];                                 // per team: slots of the three smallest (reach, slot) keys, -1 = none
};
struct MAObsShared : MAObsFacts {                      // ... then the row being assembled
  float4 row[kAObsVec];
};
S2D_DEV float m_own_body(float b, bool right) { return right ? (b > 0.0f ? b - 180.0f : b + 180.0f) : b; }
S2D_DEV float m_side_word(int side, int ours) { return side == ours ? 1.0f : (side == SIDE_NONE ? 0.0f : -1.0f); }

// What the rows read of one lane's object and of its match: the state words, zero where the lane has no such word (x .. vy up to
// the ball, the rest for players only).  s2d_match_agent_obs_kernel loads them from memory, the network rollout takes them from
// its registers at the start of a cycle.
struct MAgentIn {
  float x, y, vx, vy, body, stamina, effort, recovery, capacity;
  int tackle, card, catch_ban;
  int cycle, mode, mode_side, last_touch, score_l, score_r, holder, stopped;
};
// ... and what m_agent_facts derives from them once per match: the lane's kickable / active / reach facts, the match's masks and
// the per-side lines (index 0 = left, 1 = right; every lane the same value)
struct MAgentDerived {
  bool is_player, active;
  int reach;
  uint32_t kick_mask;
  float offside_line[2], def_ours[2], def_theirs[2];
};

// Mapping as the relative kernel: a half-wave per match, lane l = slot (22 = the ball).  Each lane derives its object's facts once
// (kickable, reach steps, rank among its team); per-side lines once per match.  Called by all 64 lanes; ends with a wave fence.
S2D_DEV MAgentDerived m_agent_facts(const MAgentTab& tab, MAObsFacts& sh, const MAgentIn& in, int l, int half) {
  MAgentDerived f;
  f.is_player = l < NP;
  f.active = f.is_player && in.card < S2D_CARD_RED;
  const float x = in.x, y = in.y;
  const bool active = f.active;
  sh.x[l] = x; sh.y[l] = y; sh.vx[l] = in.vx; sh.vy[l] = in.vy; sh.catch_ban[l] = (float)in.catch_ban;
  wave_fence();
  const float bx = sh.x[BALL], by = sh.y[BALL], bvx = sh.vx[BALL], bvy = sh.vy[BALL];
  // object facts (frame-free: negating every input negates every difference exactly)
  const int lc = f.is_player ? l : 0;
  const float ka2 = tab.ka2[lc];
  const bool kickable = active && sq2(bx - x, by - y) <= ka2;
  int reach = S2D_AGENT_REACH_NONE;
  if (active) {
    if (sq2(bx - x, by - y) <= ka2) {
      reach = 0;
    } else {
      const float ka = tab.ka[lc], smax = tab.speed_max[lc], decay = tab.ball_decay;
      float cx = bx, cy = by, cvx = bvx, cvy = bvy;
      for (int t = 1; t <= S2D_AGENT_REACH_MAX; ++t) {
        cx = cx + cvx; cy = cy + cvy; cvx = cvx * decay; cvy = cvy * decay;
        const float r = ka + (float)t * smax;
        if (sq2(cx - x, cy - y) <= r * r) { reach = t; break; }
      }
    }
  }
  f.reach = reach;
  sh.reach[l] = (float)reach;
  f.kick_mask = hballot(kickable, half) & 0x3FFFFFu;
  const uint32_t act_mask = hballot(active, half) & 0x3FFFFFu;
  if (l < 6) sh.rank_slot[l / 3][l % 3] = -1;
  wave_fence();
  if (active) {                                        // rank of (reach, slot) among the active players of the team
    const int t0 = l < 11 ? 0 : 11;
    int rank = 0;
    for (int j = t0; j < t0 + 11; ++j) {
      const int rj = (int)sh.reach[j];
      rank += (((act_mask >> j) & 1u) != 0u && (rj < reach || (rj == reach && j < l))) ? 1 : 0;
    }
    if (rank < 3) sh.rank_slot[l < 11 ? 0 : 1][rank] = l;
  }
  // per-side lines, in the frame of side S
  for (int S = 0; S < 2; ++S) {
    const float sg = S == 0 ? 1.0f : -1.0f;
    const int us = S == 0 ? 0 : 11, them = S == 0 ? 11 : 0;
    const float obx = sg * bx;
    float first = -1.0e9f, second = -1.0e9f;
    for (int j = 0; j < 11; ++j) {
      const float v = sg * sh.x[them + j];
      if (v > first) { second = first; first = v; } else if (v > second) second = v;
    }
    float line = 0.0f;
    if (second > line) line = second;
    if (obx > line) line = obx;
    float mn = obx, mx = obx;
    for (int j = 1; j < 11; ++j) {                     // (slot 0 of each team is the goalie)
      const bool act_us = ((act_mask >> (us + j)) & 1u) != 0u, act_them = ((act_mask >> (them + j)) & 1u) != 0u;
      const float vu = sg * sh.x[us + j], vt = sg * sh.x[them + j];
      if (act_us && vu < mn) mn = vu;
      if (act_them && vt > mx) mx = vt;
    }
    f.offside_line[S] = line; f.def_ours[S] = mn; f.def_theirs[S] = mx;
  }
  wave_fence();
  return f;
}

// The row of agent pa (uniform within the half-wave) into `row` (LDS, 56 float4): every lane writes its part (objects: their 8
// words; the agent's lane: the self block; the ball's lane: ball words and the kick rate; lanes 23..28: the game block), so that
// after a wave fence all 56 float4 hold the row.  This is THE definition of a row: s2d_match_agent_obs_kernel and the network
// rollout both call it.
template <class P>
S2D_DEV void m_agent_row(const P& p, const MAgentTab& tab, const MAObsFacts& sh, const MAgentIn& in, const MAgentDerived& f, int l,
                         int pa, float4* row) {
  const float x = in.x, y = in.y, vx = in.vx, vy = in.vy, body = in.body;
  const bool is_player = f.is_player, active = f.active;
  const bool right = pa >= 11;
  const int ours = right ? SIDE_RIGHT : SIDE_LEFT, S = right ? 1 : 0;
  const float sg = right ? -1.0f : 1.0f;
  const float ax = sg * sh.x[pa], ay = sg * sh.y[pa];
  const float abody = m_own_body(__shfl(body, pa, kHalf), right);
  // this lane's object in the agent's frame
  const float ox = sg * x, oy = sg * y, ovx = sg * vx, ovy = sg * vy, obody = m_own_body(body, right);
  const float dx = ox - ax, dy = oy - ay;
  float dist = hypot2(dx, dy);
  float bearing = norm_deg_any(atan2_deg(dy, dx) - abody);
  if (l == pa) { dist = 0.0f; bearing = 0.0f; }
  if (is_player) {
    const int idx = ((l < 11) == !right ? S2D_AGENT_OBS_TEAMMATES : S2D_AGENT_OBS_OPPONENTS) / 4 + 2 * (l % 11);
    row[idx] = active ? make_float4(ox, oy, ovx, ovy) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    row[idx + 1] = active ? make_float4(obody, dist, bearing, (float)f.reach) : make_float4(0.0f, 0.0f, 0.0f, (float)f.reach);
    if (l == pa) {                                   // self block, words 0..11
      row[0] = make_float4(ox, oy, ovx, ovy);
      row[1] = make_float4(obody, in.stamina, in.effort, in.recovery);
      row[2] = make_float4(in.capacity, (l == S2D_MATCH_GOALIE_LEFT || l == S2D_MATCH_GOALIE_RIGHT) ? 1.0f : 0.0f, (float)in.tackle,
                           (float)in.card);
    }
  } else if (l == BALL) {                            // ball words; self words 12..15 (they need the ball's distance and bearing)
    const bool akick = ((f.kick_mask >> pa) & 1u) != 0u;
    float rate = 0.0f;
    if (akick) {
      const float dir_diff = fabsf(bearing);
      const float dist_ball = dist - tab.size[pa] - tab.ball_size;    // (hypot2 == sqrtf of the same square)
      rate = tab.kick_rate[pa] * (1.0f - 0.25f * (dir_diff * 0.005555555555555556f) - 0.25f * (dist_ball * tab.inv_margin[pa]));
    }
    row[3] = make_float4(akick ? 1.0f : 0.0f, rate, sh.catch_ban[pa], tab.type_id[pa]);
    row[4] = make_float4(ox, oy, ovx, ovy);
    const int hside = in.holder > 0 ? side_of(in.holder - 1) : SIDE_NONE;
    row[5] = make_float4(dist, bearing, m_side_word(in.last_touch, ours), m_side_word(hside, ours));
  } else if (l <= BALL + 6) {                        // game block: lane 23 + g writes words 4g..4g+3
    const int g = l - (BALL + 1);
    const uint32_t team = right ? 0x3FF800u : 0x7FFu;
    const uint32_t km_tm = f.kick_mask & team & ~(1u << pa), km_op = f.kick_mask & (0x3FFFFFu ^ team);
    const float k_tm = km_tm ? (float)(__builtin_ctz(km_tm) % 11 + 1) : 0.0f;
    const float k_op = km_op ? (float)(__builtin_ctz(km_op) % 11 + 1) : 0.0f;
    const int* rs = sh.rank_slot[S];
    const int t1 = rs[0] == pa ? rs[1] : rs[0];
    const int t2 = (rs[0] == pa || rs[1] == pa) ? rs[2] : rs[1];
    const int* ro = sh.rank_slot[1 - S];
    const float t1r = t1 >= 0 ? sh.reach[t1] : (float)S2D_AGENT_REACH_NONE, t1u = t1 >= 0 ? (float)(t1 % 11 + 1) : 0.0f;
    const float t2r = t2 >= 0 ? sh.reach[t2] : (float)S2D_AGENT_REACH_NONE, t2u = t2 >= 0 ? (float)(t2 % 11 + 1) : 0.0f;
    const float o1r = ro[0] >= 0 ? sh.reach[ro[0]] : (float)S2D_AGENT_REACH_NONE, o1u = ro[0] >= 0 ? (float)(ro[0] % 11 + 1) : 0.0f;
    const float o2r = ro[1] >= 0 ? sh.reach[ro[1]] : (float)S2D_AGENT_REACH_NONE, o2u = ro[1] >= 0 ? (float)(ro[1] % 11 + 1) : 0.0f;
    const int mode = in.mode, cycle = in.cycle;
    const float sp = in_modes(mode, kOurSetPlayModes) ? 1.0f : 0.0f;
    const float side_w = m_side_word(in.mode_side, ours);
    float4 w;
    switch (g) {
      case 0: w = make_float4((float)mode, side_w, (float)(right ? in.score_r : in.score_l), (float)(right ? in.score_l : in.score_r)); break;
      case 1: w = make_float4((float)cycle, (float)in.stopped, (float)cycles_to_period_end(p, cycle),
                              in_modes(mode, kPenaltyModes) ? 1.0f : 0.0f); break;
      case 2: w = make_float4(f.offside_line[S], f.def_ours[S], f.def_theirs[S], k_tm); break;
      case 3: w = make_float4(k_op, sh.reach[pa], t1r, t1u); break;
      case 4: w = make_float4(t2r, t2u, o1r, o1u); break;
      default: w = make_float4(o2r, o2u, side_w > 0.0f ? sp : 0.0f, side_w < 0.0f ? sp : 0.0f); break;
    }
    row[S2D_AGENT_OBS_GAME / 4 + g] = w;
  }
}

// The half-wave stores a row assembled in LDS as two contiguous float4 stores (512 + 384 B), every line written whole by one instruction.
S2D_DEV void m_agent_row_store(float* __restrict__ dst, const float4* row, int l) {
  float4* d = reinterpret_cast<float4*>(dst);
  d[l] = row[l];
  if (l + kHalf < kAObsVec) d[l + kHalf] = row[l + kHalf];
}

// Agent reward (include/s2d_match.h): what lane l's reward reads of its own row -- the ball's place (field frame: the own-frame x is
// sgn * bx, exact), ball.dist_from_self and |ball.bearing|, in m_agent_row's own expressions (its ball lane, pa = l), so that the
// words are bitwise the row's.  Called by all 64 lanes (the ball broadcast); lanes >= 22 get words nobody reads.
struct MRwView { float bx, by, dist, abear; };
S2D_DEV MRwView m_reward_view(const MObj& o, int l, int half) {
  const float bx = hbcast_c<BALL>(o.x, half), by = hbcast_c<BALL>(o.y, half);
  const bool right = l >= 11;
  const float sg = right ? -1.0f : 1.0f;
  const float dx = sg * bx - sg * o.x, dy = sg * by - sg * o.y;
  return MRwView{bx, by, hypot2(dx, dy), fabsf(norm_deg_any(atan2_deg(dy, dx) - m_own_body(o.body, right)))};
}
// gate of the individual terms on the start-of-cycle side: active, and with chaser_only the team's rule-5 chaser (the search of
// m_scripted_action: the same keys, the same reduction).  chaser_only is wave-uniform; all 64 lanes call.
S2D_DEV bool m_reward_gate(const MObj& o, const MRwView& v, int chaser_only, int l) {
  bool gate = o.card < S2D_CARD_RED;
  if (chaser_only) {
    const float d2 = sq2(v.bx - o.x, v.by - o.y);
    const bool field = l < NP && l != S2D_MATCH_GOALIE_LEFT && l != S2D_MATCH_GOALIE_RIGHT && o.card < S2D_CARD_RED;
    unsigned long long kl = (field && l < 11) ? nearest_key(d2, l) : ~0ull;
    unsigned long long kr = (field && l >= 11) ? nearest_key(d2, l) : ~0ull;
    half_min_keys(kl, kr);
    gate = gate && (int)((l < 11 ? kl : kr) & 0xFFull) == l;
  }
  return gate;
}
// The reward of lane l's agent for the cycle S -> S': v0 / mode0 / act0 (card < RED) / gate0 (m_reward_gate) of S, v1 / o / g of S'; ka2 = the
// slot's kickable bound; w = the six weights.  Terms and their order: the table of include/s2d_match.h.
S2D_DEV float m_agent_reward(const MRwView& v0, int mode0, bool act0, bool gate0, const MRwView& v1, const MObj& o, const MGame& g, float ka2,
                             const float (&w)[S2D_MATCH_REWARD_TERMS], int l) {
  const bool right = l >= 11;
  const float sg = right ? -1.0f : 1.0f;
  const bool play1 = g.mode == S2D_GM_PLAY_ON, live = mode0 == S2D_GM_PLAY_ON && play1;
  const bool act1 = o.card < S2D_CARD_RED;
  const bool indiv = live && gate0 && act1;
  const bool kickable = act1 && sq2(v1.bx - o.x, v1.by - o.y) <= ka2;      // row(S')[self.is_kickable]
  const float term[S2D_MATCH_REWARD_TERMS] = {
      sg * g.reward,
      live ? sg * v1.bx - sg * v0.bx : 0.0f,
      indiv ? v0.dist - v1.dist : 0.0f,
      indiv ? (v0.abear - v1.abear) * 0.005555555555555556f : 0.0f,
      (play1 && act0 && kickable) ? 1.0f : 0.0f,
      play1 ? m_side_word(g.last_touch, right ? SIDE_RIGHT : SIDE_LEFT) : 0.0f};
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < S2D_MATCH_REWARD_TERMS; ++k) acc = fmaf(w[k], term[k], acc);
  return acc;
}


// ------------------------------------------------------------------------------------------
// network slots (s2d_match_set_network, include/s2d_match.h): the caller's Q-network on each network slot's agent row
// ------------------------------------------------------------------------------------------
// A wave holds two matches; the rows built in a cycle are those of the row mask (network slots, plus the recorded ones) in slot
// order, interleaved by match: tile row 2 j + half = the j-th agent of the tile's eight.  Each 16-row tile is built in LDS, then
// pushed through the three layers (s2d_net.h: layer 1's 56 k-steps read W1's fragments from memory, layers 2 and 3 theirs from
// LDS), and the argmax of each row is kept; pad rows of the last tile are zero and their results are never read.
// Two networks (s2d_match_set_opponent_network): a tile never mixes networks -- the rows go in two passes, each over one network's
// slots in slot order with that network's fragments, widths, LDS block and K; rows that are only recorded go with the first pass.
// The passes' argmax tiles follow each other in the wave's index words (at most four tiles: ceil(a / 8) + ceil(b / 8), a + b <= 22).
constexpr int kNetK1 = S2D_AGENT_OBS_DIM / 4;          // 56 k-steps of layer 1
constexpr int kNetRowPitch = S2D_AGENT_OBS_DIM + 4;    // LDS pitch of a row (228: the 16 rows of a B fragment hit 64 banks)
constexpr int kNetHidPitch = 64 + 4;                   // ... of the hidden and Q images
constexpr int kNetMaxRows = 48;                        // 2 matches x 22 agents, in tiles of 16
constexpr int kNetIdxWords = 64;                       // ... and of two passes: at most four tiles of 16
struct MNetOpp {                           // the second network (empty mask: none): the words of its own pass
  uint32_t mask;                           // its slots (disjoint from net_mask)
  int h1, h2, na, na16;
  const float* frags;                      // its fragment-order copy, laid out as the first one's
  int shared_words;                        // words of its W2 .. b3 staged into LDS behind the first network's; 0: the two do not fit the
                                           // CU's LDS, and its pass reads them from frags, as both read W1
  const float* epsilon;
  const float* table;
};
struct MNet {
  uint32_t net_mask, row_mask, obs_mask;   // first network's slots; slots whose rows are built (both networks' | obs); slots recorded in agent_obs
  int h1, h2, na, na16;
  const float* frags;                      // the engine's fragment-order copy: W1 (read from memory), then W2 | W3 | b1 | b2 | b3
  int shared_words;                        // words of W2 .. b3 (staged into LDS)
  const float* epsilon;                    // device float, read once per launch
  const float* table;                      // device float[na][3]
  int32_t* net_index;                      // [T][N][22] or NULL
  float* agent_obs;                        // [T][N][popcount(obs_mask)][224] or NULL
  MNetOpp opp;
};
struct MNetArg { MNet net; MAgentTab tab; };   // kernel argument of the NET instantiations (with their MCtl)
// Policy slots (s2d_match_set_policy_network): the words a pass needs beyond MNet's, [0] the first pass, [1] the second.
struct MPol {
  int kind[2];                             // 0: a Q-network (argmax here, epsilon in the body), 1: a stochastic policy (the head below)
  int act[2];                              // hidden activation of the pass: 0 relu, 1 tanh_spec
  const uint32_t* det[2];                  // a policy's device word (read once per launch): != 0 -> greedy
  float* logp;                             // [T][N][22] or NULL
};
struct MPolArg { MNet net; MAgentTab tab; MPol pol; };   // kernel argument of the POL instantiations: an MNetArg, then the policy words
constexpr int kNetWaveWords = 16 * kNetRowPitch + 16 * kNetHidPitch + 2 * (int)(sizeof(MAObsFacts) / 4) + kNetIdxWords;
static_assert((2 * sizeof(MAObsFacts)) % 16 == 0 && (16 * kNetRowPitch + 16 * kNetHidPitch) % 4 == 0, "16-byte aligned LDS parts");
// POL: one log-probability word beside each index word.  4 waves x 64 words = 1 024 B of the 1 344 B that two 64-64-64 networks
// leave beside the stock kernels: that pair stays staged there.
constexpr int kPolWaveWords = kNetWaveWords + kNetIdxWords;

S2D_DEV float* m_net_lds() {                           // dynamic LDS: [W2 | W3 | b1 | b2 | b3] of each network, then kNetWaveWords per wave
  extern __shared__ __attribute__((aligned(16))) float net_smem[];
  return net_smem;
}
// the block-shared part of the network into LDS (every thread of the block; the kernel's barrier follows)
S2D_DEV void m_net_stage(const MNet& net) {
  const float4* src = reinterpret_cast<const float4*>(net.frags + net.h1 / 16 * kNetK1 * 64);
  float4* dst = reinterpret_cast<float4*>(m_net_lds());
  for (int i = threadIdx.x; i < net.shared_words / 4; i += kMBlock) dst[i] = src[i];
  if (net.opp.shared_words != 0) {
    const float4* src2 = reinterpret_cast<const float4*>(net.opp.frags + net.opp.h1 / 16 * kNetK1 * 64);
    dst += net.shared_words / 4;
    for (int i = threadIdx.x; i < net.opp.shared_words / 4; i += kMBlock) dst[i] = src2[i];
  }
}

// One 16-row tile (LDS, `tile`) through the three layers of one network and the argmax of each row into idx[0..15].  w1: W1's
// fragments (memory); w2s: W2 | W3 | b1 | b2 | b3, in LDS (staged) or in memory -- one inlined copy of this function per kind.
S2D_DEV void m_net_tile_forward(const float* __restrict__ w1, const float* __restrict__ w2s, int h1, int h2, int nact, int na16,
                                float* tile, float* hid, int* idx, int lane) {
  const int gq = lane >> 4, c = lane & 15;
  const float* const w2 = w2s;
  const float* const w3 = w2 + (h2 / 16) * (h1 / 4) * 64;
  const float* const b1 = w3 + (na16 / 16) * (h2 / 4) * 64;
  const float* const b2 = b1 + h1;
  const float* const b3 = b2 + h2;
  const float* const x = tile + c * kNetRowPitch;
  layer_tile<true, 4>(w1, b1, h1 / 16, kNetK1, [&](int s) { return x[4 * s + gq]; }, hid, kNetHidPitch, lane);
  wave_fence();
  layer_tile<true, 4>(w2, b2, h2 / 16, h1 / 4, [&](int s) { return hid[c * kNetHidPitch + 4 * s + gq]; }, tile, kNetHidPitch, lane);
  wave_fence();
  layer_tile<false, 4>(w3, b3, na16 / 16, h2 / 4, [&](int s) { return tile[c * kNetHidPitch + 4 * s + gq]; }, hid, kNetHidPitch, lane);
  wave_fence();
  if (lane < 16) {   // best = 0; for a = 1 .. K-1: if (q[a] > q[best]) best = a  (ties: lowest index; a NaN never replaces the best)
    const float* q = hid + lane * kNetHidPitch;
    int best = 0;
    float bv = q[0];
    for (int a = 1; a < nact; ++a) {
      const float v = q[a];
      if (v > bv) { bv = v; best = a; }
    }
    idx[lane] = best;
  }
  wave_fence();
}

// The same tile through the three layers of a network of a POL instantiation, hidden activation ACT (both are compiled in, the
// pass says which); the logits stay in `hid`.  ACT relu is m_net_tile_forward's forward word for word.
template <int ACT>
S2D_DEV void m_pol_tile_layers(const float* __restrict__ w1, const float* __restrict__ w2s, int h1, int h2, int na16, float* tile,
                               float* hid, int lane) {
  const int gq = lane >> 4, c = lane & 15;
  const float* const w2 = w2s;
  const float* const w3 = w2 + (h2 / 16) * (h1 / 4) * 64;
  const float* const b1 = w3 + (na16 / 16) * (h2 / 4) * 64;
  const float* const b2 = b1 + h1;
  const float* const b3 = b2 + h2;
  const float* const x = tile + c * kNetRowPitch;
  layer_tile<ACT, 4>(w1, b1, h1 / 16, kNetK1, [&](int s) { return x[4 * s + gq]; }, hid, kNetHidPitch, lane);
  wave_fence();
  layer_tile<ACT, 4>(w2, b2, h2 / 16, h1 / 4, [&](int s) { return hid[c * kNetHidPitch + 4 * s + gq]; }, tile, kNetHidPitch, lane);
  wave_fence();
  layer_tile<S2D_ACT_FN_NONE, 4>(w3, b3, na16 / 16, h2 / 4, [&](int s) { return tile[c * kNetHidPitch + 4 * s + gq]; }, hid, kNetHidPitch, lane);
  wave_fence();
}
// The pass's head on the tile's logits.  A Q-network pass (pol == false): m_net_tile_forward's argmax.  A policy pass: the head is
// categorical_head (s2d_head.h), run by the tile's 16 head lanes, one row each, on the logits where layer 3 left them -- the next
// tile overwrites them, and the slot's own lane is in another part of the wave.  So the head lane derives whose row it holds:
// tile row r = 2 j + half is the j-th slot of `tile_mask` (the tile's slots, a uniform word) of the match in that half, whose id
// and tick it takes from that half's first lane (gl, gh, tick: every lane's own match; shuffled here, not once per cycle, so
// that they are not live across the layers).  It draws the slot's ST_NET block itself and takes word z; the sums stay the
// sequential ones of the spec.  Rows past `rn` pairs are pads: no head.
template <class P>
S2D_DEV void m_pol_tile_head(const P& p, int nact, const float* hid, int* idx, float* lp, int lane, bool pol, bool det,
                             uint32_t tile_mask, int rn, uint32_t gl, uint32_t gh, uint32_t tick) {
  uint32_t hgl = 0u, hgh = 0u, htick = 0u;
  if (pol) {                                               // (uniform; all 64 lanes shuffle)
    const int src = (lane & 1) * kHalf;
    hgl = (uint32_t)__shfl((int)gl, src, 64); hgh = (uint32_t)__shfl((int)gh, src, 64); htick = (uint32_t)__shfl((int)tick, src, 64);
  }
  if (lane < 16) {
    const float* q = hid + lane * kNetHidPitch;
    if (!pol) {          // best = 0; for a = 1 .. K-1: if (q[a] > q[best]) best = a  (ties: lowest index; a NaN never replaces the best)
      int best = 0;
      float bv = q[0];
      for (int a = 1; a < nact; ++a) {
        const float v = q[a];
        if (v > bv) { bv = v; best = a; }
      }
      idx[lane] = best;
    } else if ((lane >> 1) < rn) {
      uint32_t m = tile_mask;
      for (int j = 0; j < (lane >> 1); ++j) m &= m - 1u;
      const int slot = __builtin_ctz(m);
      uint32_t w = 0u;
      if (!det) w = m_draw(p, hgl, hgh, htick, S2D_ST_NET, (uint32_t)slot).z;
      float logp;
      idx[lane] = categorical_head(q, nact, det, w, logp);
      lp[lane] = logp;
    }
  }
  wave_fence();
}

// One cycle's network step of the wave, from the start-of-cycle state (o, g, r): the rows, their record, the forward pass and
// the argmax.  Returns the greedy index of this lane's slot (meaningful for network slots).  All 64 lanes, uniform control flow.
// POL (NA = MPolArg): the pass's kind, activation and `det` bit (bit 0 the first pass, bit 1 the second) pick the forward above;
// gl, gh: this lane's match id; returns an MPick: the index and its log-probability (policy slots; 0 elsewhere).
struct MPick { int idx; float logp; };
template <class P, class NA>
S2D_DEV auto m_net_greedy(const P& p, const NA& na, const MObj& o, const MGame& g, const MRare& r, int l, int half, bool valid,
                          int64_t rec_row, uint32_t det = 0u, uint32_t gl = 0u, uint32_t gh = 0u) {
  constexpr bool POL = std::is_same<NA, MPolArg>::value;
  const MNet& net = na.net;
  const int lane = threadIdx.x & 63;
  float* const shared = m_net_lds();
  float* const tile = shared + net.shared_words + net.opp.shared_words + (threadIdx.x >> 6) * (POL ? kPolWaveWords : kNetWaveWords);
  float* const hid = tile + 16 * kNetRowPitch;
  MAObsFacts* const facts = reinterpret_cast<MAObsFacts*>(hid + 16 * kNetHidPitch);
  int* const gidx = reinterpret_cast<int*>(facts + 2);
  float* const glp = reinterpret_cast<float*>(gidx + kNetIdxWords);   // (POL only: the words kPolWaveWords adds)
  MAgentIn in{};
  if (l <= BALL) { in.x = o.x; in.y = o.y; in.vx = o.vx; in.vy = o.vy; }
  if (l < NP) {
    in.body = o.body; in.stamina = o.stamina; in.effort = o.effort; in.recovery = o.recovery; in.capacity = o.capacity;
    in.tackle = o.tackle; in.card = o.card; in.catch_ban = o.catch_ban;
  }
  in.cycle = g.cycle; in.mode = g.mode; in.mode_side = g.mode_side; in.last_touch = g.last_touch;
  in.score_l = r.score_l; in.score_r = r.score_r; in.holder = r.holder; in.stopped = r.stopped;
  MAObsFacts& fs = facts[half];
  const MAgentDerived f = m_agent_facts(na.tab, fs, in, l, half);
  const int nobs = __builtin_popcount(net.obs_mask);
  const uint32_t first_rows = net.row_mask & ~net.opp.mask;   // the first pass: the first network's slots and the only-recorded ones
  const int first_tiles = (__builtin_popcount(first_rows) + 7) >> 3;
#pragma nounroll
  for (int pass = 0; pass < 2; ++pass) {                 // (every word of a pass is a kernel argument: uniform)
    const bool second = pass != 0;
    uint32_t rest = second ? net.opp.mask : first_rows;
    if (rest == 0u) continue;
    const bool forward = second || net.net_mask != 0u;   // (first pass without a network: records only)
    const int h1 = second ? net.opp.h1 : net.h1, h2 = second ? net.opp.h2 : net.h2;
    const int nact = second ? net.opp.na : net.na, na16 = second ? net.opp.na16 : net.na16;
    const float* const w1 = second ? net.opp.frags : net.frags;
    const bool staged = !second || net.opp.shared_words != 0;
    int* const pidx = gidx + (second ? 16 * first_tiles : 0);
    const int nrows = __builtin_popcount(rest);
    for (int nt = 0; 8 * nt < nrows; ++nt) {
      const int rn = nrows - 8 * nt < 8 ? nrows - 8 * nt : 8;
      [[maybe_unused]] const uint32_t tile_mask = rest;    // (POL: its lowest rn bits are this tile's slots)
      for (int i = lane; i < (16 - 2 * rn) * (kNetRowPitch / 4); i += 64)   // pad rows of the last tile
        reinterpret_cast<float4*>(tile + 2 * rn * kNetRowPitch)[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      for (int j = 0; j < rn; ++j) {
        const int pa = __builtin_ctz(rest);              // the agent (uniform: the mask is a kernel argument)
        rest &= rest - 1u;
        float4* const row = reinterpret_cast<float4*>(tile + (2 * j + half) * kNetRowPitch);
        m_agent_row(p, na.tab, fs, in, f, l, pa, row);
        if (net.agent_obs && ((net.obs_mask >> pa) & 1u)) {
          wave_fence();
          const int k = __builtin_popcount(net.obs_mask & ((1u << pa) - 1u));
          if (valid) m_agent_row_store(net.agent_obs + (rec_row * nobs + k) * S2D_AGENT_OBS_DIM, row, l);
        }
      }
      wave_fence();
      if constexpr (POL) {
        if (forward) {
          const bool pol = (second ? na.pol.kind[1] : na.pol.kind[0]) != 0, pdet = ((second ? det >> 1 : det) & 1u) != 0u;
          const bool tanh_act = (second ? na.pol.act[1] : na.pol.act[0]) != 0;
          const auto run = [&](const float* __restrict__ w2s) __attribute__((always_inline)) {   // (inlined per address space, as below)
            if (tanh_act) m_pol_tile_layers<S2D_ACT_FN_TANH>(w1, w2s, h1, h2, na16, tile, hid, lane);
            else m_pol_tile_layers<S2D_ACT_FN_RELU>(w1, w2s, h1, h2, na16, tile, hid, lane);
          };
          if (staged) run(shared + (second ? net.shared_words : 0));
          else run(w1 + h1 / 16 * kNetK1 * 64);
          m_pol_tile_head(p, nact, hid, pidx + 16 * nt, glp + (pidx - gidx) + 16 * nt, lane, pol, pdet, tile_mask, rn, gl, gh,
                          (uint32_t)g.tick);
        }
      } else if (forward) {
        if (staged) m_net_tile_forward(w1, shared + (second ? net.shared_words : 0), h1, h2, nact, na16, tile, hid, pidx + 16 * nt, lane);
        else m_net_tile_forward(w1, w1 + h1 / 16 * kNetK1 * 64, h1, h2, nact, na16, tile, hid, pidx + 16 * nt, lane);
      }
    }
  }
  int greedy = 0;
  [[maybe_unused]] float lp = 0.0f;
  if (l < NP) {                                          // the slot's place among its own pass's rows
    const uint32_t below = (1u << l) - 1u;
    if ((net.net_mask >> l) & 1u) greedy = gidx[2 * __builtin_popcount(first_rows & below) + half];
    else if ((net.opp.mask >> l) & 1u) greedy = gidx[16 * first_tiles + 2 * __builtin_popcount(net.opp.mask & below) + half];
    if constexpr (POL) {
      if (((net.net_mask >> l) & 1u) && na.pol.kind[0]) lp = glp[2 * __builtin_popcount(first_rows & below) + half];
      else if (((net.opp.mask >> l) & 1u) && na.pol.kind[1]) lp = glp[16 * first_tiles + 2 * __builtin_popcount(net.opp.mask & below) + half];
    }
  }
  wave_fence();
  if constexpr (POL) return MPick{greedy, lp};
  else return greedy;
}

// ------------------------------------------------------------------------------------------
// see network (s2d_match_set_see_network, include/s2d_match.h): the Q-network on each slot's SEE row, the vision state stepped here
// ------------------------------------------------------------------------------------------
// The scheme of the network slots above with the 192-word see row in the place of the agent row: 8 agents per match per tile,
// zeroed pad rows, the three layers on f32 MFMA (layer 1: 48 k-steps), hidden and Q images at pitch 68.  The row is s2d_see_row.h's
// see_row(), the function s2d_match_see_kernel runs.  Neck, view width and see wait of the lane's player live in registers across
// the launch's cycles (like MObj); each cycle they go into the half-wave's facts for the row builder.
constexpr int kSeeK1 = S2D_SEE_DIM / 4;                // 48 k-steps of layer 1
constexpr int kSeeRowPitch = S2D_SEE_DIM + 4;          // LDS pitch of a row (196: 16-byte aligned, the 16 rows of a B fragment hit 64 banks)
struct MSee {
  uint32_t net_mask, row_mask, obs_mask;   // network slots; slots whose rows are built (net | obs); slots recorded in see_out
  int h1, h2, na, na16;
  const float* frags;                      // the engine's fragment-order copy: W1 (read from memory), then W2 | W3 | b1 | b2 | b3
  int shared_words;                        // words of W2 .. b3 (staged into LDS)
  const float* epsilon;                    // device float, read once per launch
  const float* table;                      // device float[na][5]: command, a, b, TurnNeck moment, ChangeView code
  int32_t* net_index;                      // [T][N][22] or NULL
  float* see_out;                          // [T][N][popcount(obs_mask)][192] or NULL
  const float* view_actions;               // [T][N][22][2] or NULL: the view actions of the slots without the network
};
struct MSeeArg { MSee net; s2d_see::SeeParams sp; S2DMatchVision vis; };   // kernel argument of the SEE instantiations (with their MCtl)
constexpr int kSeeWaveWords = 16 * kSeeRowPitch + 16 * kNetHidPitch + 2 * (int)(sizeof(s2d_see::SeeFacts) / 4) + kNetMaxRows;
static_assert((2 * sizeof(s2d_see::SeeFacts)) % 16 == 0 && (16 * kSeeRowPitch + 16 * kNetHidPitch) % 4 == 0 && kSeeRowPitch % 4 == 0,
              "16-byte aligned LDS parts");
static_assert(16 * kSeeRowPitch >= 16 * kNetHidPitch, "layer 2's image fits where the rows were");
// See policy slots (s2d_match_set_see_policy_network): the kernel argument of the SEEPOL instantiations, an MSeeArg (epsilon NULL)
// and then the policy words; one log-probability word beside each index word of the wave (768 B more per workgroup).
struct MSeePolArg {
  MSee net; s2d_see::SeeParams sp; S2DMatchVision vis;
  int act;                                 // hidden activation: 0 relu, 1 tanh_spec
  const uint32_t* det;                     // the policy's device word (read once per launch): != 0 -> greedy
  float* logp;                             // [T][N][22] or NULL
};
constexpr int kSeePolWaveWords = kSeeWaveWords + kNetMaxRows;
static_assert(kSeeWaveWords % 4 == 0 && kSeePolWaveWords % 4 == 0, "a wave's part starts 16-byte aligned");
// Belief network (s2d_match_set_belief_network): the kernel argument of the BELIEF instantiations, an MSeePolArg (net.epsilon: the
// Q head's) and then the belief words.  The network reads the slot's BELIEF row: per cycle and agent the see row is built into a
// staging row of the half-wave, the belief row comes from memory into the tile row, s2d_belief_row.h's belief_update() takes the
// see row into it there, and it goes back to memory.  A wave's part: a see policy wave's, then per half-wave the staging row and
// belief_update's scratch (2 x 768 B each half, 3 KB more per wave).
struct MBelArg {
  MSee net; s2d_see::SeeParams sp; S2DMatchVision vis;
  int act;                                 // hidden activation: 0 relu, 1 tanh_spec (head 0: relu)
  const uint32_t* det;                     // head 1: the policy's device word (read once per launch): != 0 -> greedy
  float* logp;                             // [T][N][22] or NULL
  int head;                                // 0: epsilon-greedy Q-network (net.epsilon), 1: categorical policy (det)
  s2d_belief::BeliefParams bp;
  float* belief;                           // the state: [N][popcount(belief_mask)][192], a slot's row = its rank in belief_mask
  uint32_t belief_mask;                    // (net.row_mask lies inside it)
  float* belief_out;                       // [T][N][popcount(obs_mask)][192] or NULL: the rows the network acted on
  const uint8_t* done0;                    // the engine's done plane as the launch finds it: the first cycle's reset flags
};
struct MBelStage { float4 see[s2d_see::kSeeVec]; s2d_belief::BeliefScratch scratch; };   // one half-wave
constexpr int kBelWaveWords = kSeePolWaveWords + 2 * (int)(sizeof(MBelStage) / 4);
static_assert(sizeof(MBelStage) % 16 == 0 && kBelWaveWords % 4 == 0, "16-byte aligned LDS parts");

// the block-shared part of the network into LDS (every thread of the block; the kernel's barrier follows)
S2D_DEV void m_see_stage(const MSee& net) {
  const float4* src = reinterpret_cast<const float4*>(net.frags + net.h1 / 16 * kSeeK1 * 64);
  float4* dst = reinterpret_cast<float4*>(m_net_lds());
  for (int i = threadIdx.x; i < net.shared_words / 4; i += kMBlock) dst[i] = src[i];
}

// A see-row tile through the three layers of a SEEPOL instantiation, hidden activation ACT (both are compiled in, the launch says
// which); the logits stay in `hid`.  ACT relu is m_see_greedy's forward word for word.
template <int ACT>
S2D_DEV void m_see_pol_tile_layers(const MSee& net, const float* shared, float* tile, float* hid, int lane) {
  const int gq = lane >> 4, c = lane & 15;
  const float* const w2 = shared;
  const float* const w3 = w2 + (net.h2 / 16) * (net.h1 / 4) * 64;
  const float* const b1 = w3 + (net.na16 / 16) * (net.h2 / 4) * 64;
  const float* const b2 = b1 + net.h1;
  const float* const b3 = b2 + net.h2;
  const float* const x = tile + c * kSeeRowPitch;
  layer_tile<ACT, 4>(net.frags, b1, net.h1 / 16, kSeeK1, [&](int s) { return x[4 * s + gq]; }, hid, kNetHidPitch, lane);
  wave_fence();
  layer_tile<ACT, 4>(w2, b2, net.h2 / 16, net.h1 / 4, [&](int s) { return hid[c * kNetHidPitch + 4 * s + gq]; }, tile, kNetHidPitch, lane);
  wave_fence();
  layer_tile<S2D_ACT_FN_NONE, 4>(w3, b3, net.na16 / 16, net.h2 / 4, [&](int s) { return tile[c * kNetHidPitch + 4 * s + gq]; }, hid,
                                 kNetHidPitch, lane);
  wave_fence();
}

// One cycle's see-network step of the wave, from the start-of-cycle state (o, g), the lane's vision words and the match's tick: the
// see rows, their record, the forward pass and the argmax.  Returns the greedy index of this lane's slot (meaningful for network
// slots).  All 64 lanes, uniform control flow.
// SEEPOL (SA = MSeePolArg): the policy's forward and the categorical head of the policy slots (m_pol_tile_head; `det`: the
// launch's deterministic bit); returns an MPick: the index and its log-probability (0 for a slot outside the mask).
// BEL (SA = MBelArg): SEEPOL on the slot's BELIEF row -- the see row goes into the half-wave's staging row, the slot's belief row
// (match ec, the slot's rank in belief_mask) comes from memory into the tile row, belief_update() takes the see row into it (reset:
// the match's flag), it is stored back and recorded (valid matches only).  The head is the launch's: the categorical one, or the
// first maximum (the exploration draw is the body's), whose log-probability is 0.
template <class P, class SA>
S2D_DEV auto m_see_greedy(const P& p, const SA& sa, const MObj& o, const MGame& g, float vneck, int vwidth, int vwait, int l, int half,
                          bool valid, uint64_t gid, int64_t rec_row, bool det = false, int64_t ec = 0, bool reset = false) {
  constexpr bool BEL = std::is_same<SA, MBelArg>::value;
  constexpr bool SEEPOL = std::is_same<SA, MSeePolArg>::value || BEL;
  const MSee& net = sa.net;
  const int lane = threadIdx.x & 63, gq = lane >> 4, c = lane & 15;
  float* const shared = m_net_lds();
  float* const tile = shared + net.shared_words + (threadIdx.x >> 6) * (BEL ? kBelWaveWords : SEEPOL ? kSeePolWaveWords : kSeeWaveWords);
  float* const hid = tile + 16 * kSeeRowPitch;
  s2d_see::SeeFacts* const facts = reinterpret_cast<s2d_see::SeeFacts*>(hid + 16 * kNetHidPitch);
  int* const gidx = reinterpret_cast<int*>(facts + 2);
  [[maybe_unused]] float* const glp = reinterpret_cast<float*>(gidx + kNetMaxRows);   // (SEEPOL only: the words kSeePolWaveWords adds)
  [[maybe_unused]] MBelStage* const stage = reinterpret_cast<MBelStage*>(glp + kNetMaxRows) + half;   // (BEL only: kBelWaveWords' words)
  s2d_see::SeeIn in{};
  if (l <= BALL) { in.x = o.x; in.y = o.y; in.vx = o.vx; in.vy = o.vy; }
  if (l < NP) {
    in.body = o.body; in.stamina = o.stamina; in.effort = o.effort; in.recovery = o.recovery; in.capacity = o.capacity;
    in.card = o.card; in.neck = vneck; in.width = vwidth; in.wait = vwait;
  }
  in.mode = g.mode; in.mode_side = g.mode_side; in.cycle = g.cycle; in.tick = (uint32_t)g.tick;
  s2d_see::SeeFacts& fs = facts[half];
  s2d_see::see_facts(fs, in, l);                         // (ends with a wave fence)
  const int nrows = __builtin_popcount(net.row_mask), nobs = __builtin_popcount(net.obs_mask);
  const float* const w2 = shared;
  const float* const w3 = w2 + (net.h2 / 16) * (net.h1 / 4) * 64;
  const float* const b1 = w3 + (net.na16 / 16) * (net.h2 / 4) * 64;
  const float* const b2 = b1 + net.h1;
  const float* const b3 = b2 + net.h2;
  uint32_t rest = net.row_mask;
  for (int nt = 0; 8 * nt < nrows; ++nt) {
    const int rn = nrows - 8 * nt < 8 ? nrows - 8 * nt : 8;
    [[maybe_unused]] const uint32_t tile_mask = rest;      // (SEEPOL: its lowest rn bits are this tile's slots)
    for (int i = lane; i < (16 - 2 * rn) * (kSeeRowPitch / 4); i += 64)   // pad rows of the last tile
      reinterpret_cast<float4*>(tile + 2 * rn * kSeeRowPitch)[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int j = 0; j < rn; ++j) {
      const int pa = __builtin_ctz(rest);              // the agent (uniform: the mask is a kernel argument)
      rest &= rest - 1u;
      float4* const row = reinterpret_cast<float4*>(tile + (2 * j + half) * kSeeRowPitch);
      if constexpr (BEL) {
        // the belief row is in flight while the see row is built (the same lanes wrote these words in the cycle before)
        float4* const brow = reinterpret_cast<float4*>(sa.belief) +
                             (ec * __builtin_popcount(sa.belief_mask) + __builtin_popcount(sa.belief_mask & ((1u << pa) - 1u))) *
                                 (int64_t)s2d_belief::kVec;
        const bool has2 = l + kHalf < s2d_belief::kVec;
        const float4 b0 = brow[l], b1 = has2 ? brow[l + kHalf] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        s2d_see::see_row(sa.sp, fs, in, l, half, pa, gid, stage->see);   // (ends with a wave fence: the row is whole)
        row[l] = b0;
        if (has2) row[l + kHalf] = b1;
        wave_fence();
        s2d_belief::belief_update(sa.bp, row, stage->see, stage->scratch, l, half, pa % 11, reset);   // (ends with a fence)
        if (valid) { brow[l] = row[l]; if (has2) brow[l + kHalf] = row[l + kHalf]; }
        if ((net.obs_mask >> pa) & 1u) {
          const int k = __builtin_popcount(net.obs_mask & ((1u << pa) - 1u));
          if (net.see_out && valid) s2d_see::see_row_store(net.see_out + (rec_row * nobs + k) * S2D_SEE_DIM, stage->see, l);
          if (sa.belief_out && valid) s2d_see::see_row_store(sa.belief_out + (rec_row * nobs + k) * S2D_BELIEF_DIM, row, l);
        }
      } else {
        s2d_see::see_row(sa.sp, fs, in, l, half, pa, gid, row);   // (ends with a wave fence: the row is whole)
        if (net.see_out && ((net.obs_mask >> pa) & 1u)) {
          const int k = __builtin_popcount(net.obs_mask & ((1u << pa) - 1u));
          if (valid) s2d_see::see_row_store(net.see_out + (rec_row * nobs + k) * S2D_SEE_DIM, row, l);
        }
      }
    }
    wave_fence();
    if constexpr (SEEPOL) {                              // (a see policy always has slots: no record-only launch here)
      if (sa.act) m_see_pol_tile_layers<S2D_ACT_FN_TANH>(net, shared, tile, hid, lane);
      else m_see_pol_tile_layers<S2D_ACT_FN_RELU>(net, shared, tile, hid, lane);
      if constexpr (BEL)                                   // (head 0: the first maximum; no log-probability word is written)
        m_pol_tile_head(p, net.na, hid, gidx + 16 * nt, glp + 16 * nt, lane, sa.head != 0, det, tile_mask, rn, (uint32_t)gid,
                        (uint32_t)(gid >> 32), (uint32_t)g.tick);
      else
        m_pol_tile_head(p, net.na, hid, gidx + 16 * nt, glp + 16 * nt, lane, true, det, tile_mask, rn, (uint32_t)gid,
                        (uint32_t)(gid >> 32), (uint32_t)g.tick);
    } else if (net.net_mask != 0u) {
      const float* const x = tile + c * kSeeRowPitch;
      layer_tile<true, 4>(net.frags, b1, net.h1 / 16, kSeeK1, [&](int s) { return x[4 * s + gq]; }, hid, kNetHidPitch, lane);
      wave_fence();
      layer_tile<true, 4>(w2, b2, net.h2 / 16, net.h1 / 4, [&](int s) { return hid[c * kNetHidPitch + 4 * s + gq]; }, tile,
                          kNetHidPitch, lane);
      wave_fence();
      layer_tile<false, 4>(w3, b3, net.na16 / 16, net.h2 / 4, [&](int s) { return tile[c * kNetHidPitch + 4 * s + gq]; }, hid,
                           kNetHidPitch, lane);
      wave_fence();
      if (lane < 16) {   // best = 0; for a = 1 .. K-1: if (q[a] > q[best]) best = a  (ties: lowest index; a NaN never replaces the best)
        const float* q = hid + lane * kNetHidPitch;
        int best = 0;
        float bv = q[0];
        for (int a = 1; a < net.na; ++a) {
          const float v = q[a];
          if (v > bv) { bv = v; best = a; }
        }
        gidx[16 * nt + lane] = best;
      }
      wave_fence();
    }
  }
  int greedy = 0;
  if (l < NP && ((net.net_mask >> l) & 1u)) greedy = gidx[2 * __builtin_popcount(net.row_mask & ((1u << l) - 1u)) + half];
  if constexpr (SEEPOL) {
    float lp = 0.0f;
    if constexpr (BEL) {
      if (l < NP && ((net.net_mask >> l) & 1u) && sa.head != 0) lp = glp[2 * __builtin_popcount(net.row_mask & ((1u << l) - 1u)) + half];
    } else {
      if (l < NP && ((net.net_mask >> l) & 1u)) lp = glp[2 * __builtin_popcount(net.row_mask & ((1u << l) - 1u)) + half];
    }
    wave_fence();
    return MPick{greedy, lp};
  } else {
    wave_fence();
    return greedy;
  }
}
