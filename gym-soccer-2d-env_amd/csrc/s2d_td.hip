// s2d_td.hip -- the off-policy learners' TD targets from their target networks, one launch per batch (include/s2d.h S2DTdNet,
// s2d_td_target_q / s2d_td_target_ac): reward + discount * max_a Q'(next_obs, a) of DQN, the same with the
// online network's argmax of Double DQN, reward + discount * Q'(next_obs, tanh(mu'(next_obs))) of DDPG and the smaller of two
// critics of TD3.  Engine-independent, as s2d_gae and s2d_replay_*: raw device pointers, any stream of the current device,
// everything read when the kernels run, so sample -> target sits in one captured graph.
// The three actor-critic targets are ONE kernel, s2d_td_target_ac_kernel<HEAD, TWIN>, and one host path, td_target_actor_critic<HEAD>;
// a HEAD is what turns the actor's outputs into the action the critics see and the critics' value into what is bootstrapped from:
//   TdTanhHead    s2d_td_target_ac   a' = tanh_spec(y), the value is q
//   TdSacHead     s2d_td_target_sac  Soft Actor-Critic's: the ONLINE actor's squashed-Gaussian head (s2d_sac_head.h) draws the next
//                                    action with a Philox stream of its own, and the value carries the entropy term, q - alpha * logp
//   TdTd3Head     s2d_td_target_td3  TD3's whole target: the tanh head with clipped Gaussian noise on the target actor's action
//                                    (target-policy smoothing), drawn from a third Philox stream
//
// The network is the streamed-weight MLP of s2d_wide_net.h (wide_group / wide_layer and the fragment order are its) with a RUN-TIME
// input width n_in in [1, 256]: layer 1 takes ceil(n_in / 4) k-steps over x_k = 0 against zero weights past n_in, so at n_in = 10 it
// is the reach-ball actors' 12-term layer and at n_in = 4 the GoToCenter actors' single k-step.  The pack kernel (s2d_wide_pack.hip,
// one launch per network) writes the parameters in fragment order into the caller's workspace on the same stream ahead of the
// target kernel; the shape's checks, the fragment count, the workspace's check, the S2D_TD_PLAN override and the (waves, tiles)
// search are s2d_wide_host.h's, shared with the actors.  The biases are read
// from there too (one float4 per output tile), so the kernel has no block-shared LDS and no barrier: a wave is on its own.
//
// lane = batch row, 64 rows a wave, four 16-row tiles, T = 4, 2 or 1 of them per pass.  LDS of a wave:
//   [input image X: T x 16 x xpitch | image A: T x 16 x rpitch | image B: T x 16 x rpitch | output image: 64 x qpitch]
// X holds the pass's padded input rows and stays as it is while the pass's networks run: the online and the target Q-network read
// the same rows; the actor reads the observation words (its k-steps end before the action), its head's action words are written
// behind them and the critics read the whole row.  xpitch covers the widest padded input row of the call (n_in = 256 is wider
// than a [8] hidden layer), rpitch the widest hidden layer, both == 4 mod 64 words (conflict-free fragment reads).  Every chain is
// acc = b[j]; k ascending: acc = fmaf(W[j][k], in[k], acc): neither T nor the waves per workgroup enters it.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <mutex>
#include <string>

#include "s2d_sac_head.h"
#include "s2d_wide_net.h"

static constexpr int kTdMaxIn = 256;
static constexpr int kTdMaxAction = 8;

// one network as the kernels see it (no array indexed by the layer: see WideDims)
struct TdNetDev {
  int n_in;                  // 1 .. 256
  int ks1;                   // layer 1's k-steps: ceil(n_in / 4)
  int n_hidden;              // L, 1 .. 5
  int act;                   // hidden activation: 0 relu, 1 tanh_spec, 2 sigmoid_spec
  uint64_t widths;           // h_l / 4 in bits 7 (l - 1) .. 7 l - 1; 0 past L
  int na;                    // outputs (1 .. 64)
  int nfrag;                 // fragments in all; the bias block follows them in the workspace
  int nbias;                 // words of the bias block: every layer's width rounded up to 16
  const float* wf;           // the workspace
};
// the call's LDS plan
struct TdPlanDev {
  int xpitch, rpitch, qpitch;   // row pitches of the input image, the hidden images and the output image (words)
  int tiles;                    // T: row tiles per pass, 4 | 2 | 1
  int wave_words;               // T 16 (xpitch + 2 rpitch) + 64 qpitch
};
S2D_DEV int td_width(const TdNetDev& d, int l) { return 4 * (int)((d.widths >> (7 * l)) & 127u); }

// wave-uniform choice between the networks of a call, field by field (a pointer into the kernel arguments would be a copy)
S2D_DEV TdNetDev td_pick(bool first, const TdNetDev& a, const TdNetDev& b) {
  TdNetDev r;
  r.n_in = first ? a.n_in : b.n_in; r.ks1 = first ? a.ks1 : b.ks1; r.n_hidden = first ? a.n_hidden : b.n_hidden;
  r.act = first ? a.act : b.act; r.widths = first ? a.widths : b.widths; r.na = first ? a.na : b.na;
  r.nfrag = first ? a.nfrag : b.nfrag; r.nbias = first ? a.nbias : b.nbias; r.wf = first ? a.wf : b.wf;
  return r;
}

// The network on the pass's T row tiles: x = the input image (pitch xp; layer 1 reads d.ks1 k-steps of it), ia / ib = the hidden
// images (pitch rp), q = the pass's first row of the output image (pitch qp): q[row][j] = the output layer's pre-activations.
// One call site of wide_layer for all layers: its code exists once per T.
template <int T>
S2D_DEV void td_layers(const TdNetDev& d, const float* __restrict__ x, int xp, float* __restrict__ ia, float* __restrict__ ib, int rp,
                       float* __restrict__ q, int qp, int lane) {
  const float* wf = d.wf;
  const float* bias = d.wf + (size_t)d.nfrag * kWave;
  const float* in = x;
  int ip = xp, ks = d.ks1;
  float* a = ia;
  float* b = ib;
  for (int l = 0; l <= d.n_hidden; ++l) {
    const bool last = l == d.n_hidden;
    const int wout = last ? d.na : td_width(d, l), m16 = (wout + 15) >> 4;
    float* const out = last ? q : a;
    const int op = last ? qp : rp;
    wide_layer<T>(wf, bias, m16, ks, in, ip, 16 * ip, out, op, 16 * op, last ? (int)S2D_WIDE_LINEAR : d.act, lane);
    wave_lds_fence();
    wf += (size_t)m16 * ks * kWave;
    bias += 16 * m16;
    ks = wout >> 2;
    in = a; ip = rp;
    float* const swap = a; a = b; b = swap;
  }
}

// a wave's part of the dynamic LDS (the file's head): the input image, the two hidden images, the output image
struct TdWaveLds {
  float *x, *ia, *ib, *qv;
};
S2D_DEV TdWaveLds td_wave_lds(float* smem, int wv, const TdPlanDev& pl) {
  TdWaveLds w;
  w.x = smem + (size_t)wv * pl.wave_words;
  w.ia = w.x + pl.tiles * 16 * pl.xpitch;
  w.ib = w.ia + pl.tiles * 16 * pl.rpitch;
  w.qv = w.ib + pl.tiles * 16 * pl.rpitch;
  return w;
}
// network d on the pass's row tiles, its outputs from row q of the output image on: td_layers at the plan's T
S2D_DEV void td_forward(const TdNetDev& d, const TdWaveLds& w, const TdPlanDev& pl, float* q, int lane) {
  if (pl.tiles == 4) td_layers<4>(d, w.x, pl.xpitch, w.ia, w.ib, pl.rpitch, q, pl.qpitch, lane);
  else if (pl.tiles == 2) td_layers<2>(d, w.x, pl.xpitch, w.ia, w.ib, pl.rpitch, q, pl.qpitch, lane);
  else td_layers<1>(d, w.x, pl.xpitch, w.ia, w.ib, pl.rpitch, q, pl.qpitch, lane);
}

// rows row0 .. row0 + 16 T - 1 of obs[batch][D] into the input image, `kp` words a row (a multiple of 4 >= D): zeros past D and
// in the rows past the batch.  The rows are contiguous in memory; row and column are carried, so there is one division per call.
// Eight loads are issued before the first is stored: a word that does not exist is loaded from obs[0] (always there) and replaced
// by zero, so no load sits behind a branch and a 256-word row costs four round trips to memory, not thirty-two.
S2D_DEV void td_load_rows(const float* __restrict__ obs, int64_t row0, int64_t batch, int D, int kp, int rows, float* __restrict__ x,
                          int xp, int lane) {
  constexpr int U = 8;
  const int total = rows * kp, q = kWave / kp, m = kWave % kp;
  int r = lane / kp, k = lane % kp;
  for (int f0 = lane; f0 < total + lane; f0 += U * kWave) {
    float v[U];
    int at[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool in = f0 + u * kWave < total, real = in && k < D && row0 + r < batch;
      const float w = obs[real ? (row0 + r) * D + k : 0];
      v[u] = real ? w : 0.0f;
      at[u] = in ? r * xp + k : -1;
      r += q; k += m;
      if (k >= kp) { k -= kp; r += 1; }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (at[u] >= 0) x[at[u]] = v[u];
  }
}

// target = reward + (discount * q): one fp32 multiply, then one fp32 add (what eager torch's r + d * q computes)
S2D_DEV float td_target(float reward, float discount, float q) { return __fadd_rn(reward, __fmul_rn(discount, q)); }

// s2d_td_target_q.  DOUBLE: the index is the argmax of the online network, the value the target network's at that index.
template <bool DOUBLE>
__global__ __launch_bounds__(kBlock) void s2d_td_target_q_kernel(TdNetDev tgt, TdNetDev onl, TdPlanDev pl, int64_t batch,
                                                                 const float* __restrict__ next_obs, const float* __restrict__ reward,
                                                                 const float* __restrict__ discount, float* __restrict__ out_target,
                                                                 float* __restrict__ out_q, int32_t* __restrict__ out_index) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t wave_first = i - lane;
  if (wave_first >= batch) return;
  const int T = pl.tiles;
  const TdWaveLds w = td_wave_lds(smem, wv, pl);
  const int kp = 4 * tgt.ks1;
  int best = 0;
  float qbest = 0.0f;
  for (int nt = 0; nt < 4; nt += T) {
    td_load_rows(next_obs, wave_first + 16 * nt, batch, tgt.n_in, kp, 16 * T, w.x, pl.xpitch, lane);
    wave_lds_fence();
    const bool mine = (lane >> 4) >= nt && (lane >> 4) < nt + T;
    const float* const q = w.qv + lane * pl.qpitch;
#pragma unroll 1
    for (int v = DOUBLE ? 0 : 1; v < 2; ++v) {
      const TdNetDev d = DOUBLE ? td_pick(v == 0, onl, tgt) : tgt;
      td_forward(d, w, pl, w.qv + 16 * nt * pl.qpitch, lane);
      if (mine) {
        if (v == (DOUBLE ? 0 : 1)) {
          // best = 0; for a = 1 .. A-1: if (y[a] > y[best]) best = a   (ties: lowest index; a NaN never replaces the best)
          int bi = 0;
          float bv = q[0];
          for (int a = 1; a < d.na; ++a) {
            const float y = q[a];
            if (y > bv) { bv = y; bi = a; }
          }
          best = bi;
        }
        if (v == 1) qbest = q[best];
      }
      wave_lds_fence();
    }
  }
  if (i < batch) {
    out_target[i] = td_target(reward[i], discount[i], qbest);
    if (out_q) out_q[i] = qbest;
    if (out_index) out_index[i] = best;
  }
}

// ---- the actor-critic targets' heads.  What a head sees of pass nt of a wave: batch rows row0() .. row0() + 16 T - 1 are rows
// 0 .. 16 T - 1 of x (pitch xpitch) and rows 16 nt .. of qv, the output image with the actor's pre-activations (pitch qpitch; row
// `lane` is batch row i, the lane's own).  The head writes the A action words of a row behind its D observation words (the words
// past D + A stay zero), and to out_action where the row is of the batch.
struct TdPass {
  float* x;
  const float* qv;
  int xpitch, qpitch;
  int T, nt, D, A;
  int64_t i, batch;
  int lane;
  float* out_action;
  S2D_DEV int64_t row0() const { return i - lane + 16 * nt; }
  S2D_DEV bool mine() const { return (lane >> 4) >= nt && (lane >> 4) < nt + T; }   // the lane's own row is of this pass
};
// "a lane runs the head of its own batch row" (a lane of the pass: p.mine()): a'[j] = f(j, the row's pre-activations), j ascending
template <class F>
S2D_DEV void td_row_head(const TdPass& p, F f) {
  const float* const y = p.qv + p.lane * p.qpitch;
  float* const xa = p.x + (p.lane - 16 * p.nt) * p.xpitch + p.D;
#pragma unroll
  for (int j = 0; j < kTdMaxAction; ++j) {
    if (j < p.A) {
      const float a = f(j, y);
      xa[j] = a;
      if (p.out_action && p.i < p.batch) p.out_action[p.i * p.A + j] = a;
    }
  }
}
// A head is passed to the kernel by value and has four parts: actions(na), the action words the actor's n_out stands for;
// read(), what it reads once per launch; act(), the step from the pass's pre-activations to the action words (logp: a word the lane
// keeps from the head to the value); value(), what row i bootstraps from, given the critics' q.  Behind them its host side, for
// td_target_actor_critic: the dynamic-LDS slots of its two instantiations, the actor's n_out rule and its text, the phrase of the
// critic-shape refusal, the check of its own device words, and the draws counter that a one-thread kernel advances behind the
// target kernel (NULL: none).

// s2d_td_target_ac: a' = tanh_spec(y), wave-strided over the pass's 16 T A words; tanh_spec(-0) = -0 reaches the critics as it is
struct TdTanhHead {
  struct Words {};
  static constexpr int actions(int na) { return na; }
  S2D_DEV Words read() const { return Words{}; }
  S2D_DEV void act(const Words&, const TdPass& p, float&) const {
    const float* const y = p.qv + 16 * p.nt * p.qpitch;
    const int64_t row0 = p.row0();
    for (int idx = p.lane; idx < 16 * p.T * p.A; idx += kWave) {
      const int r = idx / p.A, k = idx - r * p.A;
      const float a = tanh_spec(y[r * p.qpitch + k]);
      p.x[r * p.xpitch + p.D + k] = a;
      if (p.out_action && row0 + r < p.batch) p.out_action[(row0 + r) * p.A + k] = a;
    }
  }
  S2D_DEV float value(const Words&, int64_t, float q, float) const { return q; }

  static constexpr int kSlot = 2;
  static bool n_out_ok(int n_out) { return n_out <= kTdMaxAction; }
  static constexpr const char* kNOutText = "actor: n_out must be in [1, 8]";
  static constexpr const char* kCriticIn = "n_in + n_out";
  int check_words(const std::string&, int64_t, int, const float*, const float*, const float*) const { return S2D_OK; }
  uint64_t* counter() const { return nullptr; }
};

// s2d_td_target_sac: the online actor has 2A outputs, the squashed-Gaussian head of s2d_sac_head.h gives a' and logp, and the value
// is q - (alpha * logp).  z: row_normals on stream S2D_TD_STREAM.
struct TdSacHead {
  const float* alpha;          // one device word: ent_coef
  uint64_t* draws;             // one device word: the calls so far
  uint32_t seed_lo, seed_hi;
  int det;                     // s2d_debug_td_target_sac: z = 0, the action is tanh_spec(mean), no Philox draw
  float* out_logp;

  struct Words {
    float alpha;
    uint64_t draws;
  };
  static constexpr int actions(int na) { return na >> 1; }
  S2D_DEV Words read() const { return Words{*alpha, *draws}; }
  S2D_DEV void act(const Words& w, const TdPass& p, float& logp) const {
    if (!p.mine()) return;
    const bool d = det != 0;
    const int A = p.A;
    float z[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (!d) row_normals(p.i, w.draws, S2D_TD_STREAM, seed_lo, seed_hi, A, z);
    float lp = 0.0f;
    td_row_head(p, [&](int j, const float* y) {
      float a;
      const float term = sac_head_term(y[j], y[A + j], z[j], d, a);
      lp = j == 0 ? term : lp + term;
      return a;
    });
    logp = lp;
  }
  S2D_DEV float value(const Words& w, int64_t i, float q, float logp) const {
    if (out_logp) out_logp[i] = logp;
    return __fsub_rn(q, __fmul_rn(w.alpha, logp));   // one multiply, then one subtract
  }

  static constexpr int kSlot = 4;
  static bool n_out_ok(int n_out) { return n_out >= 2 && n_out <= 2 * kTdMaxAction && n_out % 2 == 0; }
  static constexpr const char* kNOutText = "actor: n_out must be 2 A (A means, then A log-std rows), even and in [2, 16]";
  static constexpr const char* kCriticIn = "n_in + n_out / 2";
  int check_words(const std::string& who, int64_t batch, int A, const float* out_target, const float* out_q, const float* out_action) const;
  uint64_t* counter() const { return draws; }
};

// s2d_td_target_td3: the target actor's tanh head with TD3's target-policy smoothing, a' = clamp(tanh_spec(y) + clamp(sigma z, -c, c),
// -1, 1).  z: row_normals on stream S2D_TD3_STREAM.
// one action word: a multiply, a clamp, an add, a clamp; a NaN passes through both clamps (torch.clamp)
S2D_DEV float td3_smooth(float m, float sigma, float clip, float z) {
  float n = __fmul_rn(sigma, z);
  n = n < -clip ? -clip : (n > clip ? clip : n);
  const float s = __fadd_rn(m, n);
  return s < -1.0f ? -1.0f : (s > 1.0f ? 1.0f : s);
}
struct TdTd3Head {
  const float* noise;          // two device words: sigma (target_policy_noise), clip (target_noise_clip)
  uint64_t* draws;             // one device word: the calls so far
  uint32_t seed_lo, seed_hi;

  struct Words {
    float sigma, clip;
    uint64_t draws;
  };
  static constexpr int actions(int na) { return na; }
  S2D_DEV Words read() const { return Words{noise[0], noise[1], *draws}; }
  S2D_DEV void act(const Words& w, const TdPass& p, float&) const {
    if (!p.mine()) return;
    float z[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    row_normals(p.i, w.draws, S2D_TD3_STREAM, seed_lo, seed_hi, p.A, z);
    td_row_head(p, [&](int j, const float* y) { return td3_smooth(tanh_spec(y[j]), w.sigma, w.clip, z[j]); });
  }
  S2D_DEV float value(const Words&, int64_t, float q, float) const { return q; }

  static constexpr int kSlot = 6;
  static bool n_out_ok(int n_out) { return n_out <= kTdMaxAction; }
  static constexpr const char* kNOutText = "actor: n_out must be in [1, 8]";
  static constexpr const char* kCriticIn = "n_in + n_out";
  int check_words(const std::string& who, int64_t batch, int A, const float* out_target, const float* out_q, const float* out_action) const;
  uint64_t* counter() const { return draws; }
};

// The actor-critic target: the actor, its HEAD into the critics' input row, critic 1 and (TWIN) critic 2 on one row tile, the
// smaller of the critics' values through the head into the target.
template <class HEAD, bool TWIN>
__global__ __launch_bounds__(kBlock) void s2d_td_target_ac_kernel(TdNetDev actor, TdNetDev c1, TdNetDev c2, TdPlanDev pl, int64_t batch,
                                                                  const float* __restrict__ next_obs, const float* __restrict__ reward,
                                                                  const float* __restrict__ discount, HEAD head,
                                                                  float* __restrict__ out_target, float* __restrict__ out_q,
                                                                  float* __restrict__ out_action) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t wave_first = i - lane;
  if (wave_first >= batch) return;
  const int T = pl.tiles;
  const TdWaveLds w = td_wave_lds(smem, wv, pl);
  const int D = actor.n_in, A = HEAD::actions(actor.na), kp = 4 * c1.ks1;   // the critics' padded row covers the actor's
  const typename HEAD::Words hw = head.read();
  float qmin = 0.0f, logp = 0.0f;
  for (int nt = 0; nt < 4; nt += T) {
    const int64_t row0 = wave_first + 16 * nt;
    td_load_rows(next_obs, row0, batch, D, kp, 16 * T, w.x, pl.xpitch, lane);
    wave_lds_fence();
    const bool mine = (lane >> 4) >= nt && (lane >> 4) < nt + T;
    float* const qp = w.qv + 16 * nt * pl.qpitch;
#pragma unroll 1
    for (int v = 0; v < (TWIN ? 3 : 2); ++v) {
      const TdNetDev d = v == 0 ? actor : TWIN ? td_pick(v == 1, c1, c2) : c1;
      td_forward(d, w, pl, qp, lane);
      if (v == 0) {
        head.act(hw, TdPass{w.x, w.qv, pl.xpitch, pl.qpitch, T, nt, D, A, i, batch, lane, out_action}, logp);
      } else if (mine) {
        const float q = w.qv[lane * pl.qpitch];
        qmin = (v == 1 || q < qmin) ? q : qmin;              // q2 < q1 ? q2 : q1: a NaN in q2 never replaces q1
      }
      wave_lds_fence();
    }
  }
  if (i < batch) {
    out_target[i] = td_target(reward[i], discount[i], head.value(hw, i, qmin, logp));
    if (out_q) out_q[i] = qmin;
  }
}

// what follows the target kernel on the same stream: the next call (the next replay of a captured graph) draws fresh noise
__global__ void s2d_td_draws_kernel(uint64_t* __restrict__ draws) { *draws += 1; }

// ------------------------------------------------------------------------------------------ host
namespace {
struct TdLds {};   // the owner of the target kernels' dynamic-LDS slots (allow_lds_slot)

// the kernels' view of a shape on the grid (wf left NULL); wmax: raised to its widest padded hidden layer
TdNetDev net_dev(const S2DTdNet* n, int* wmax) {
  const WideCounts c = s2d_internal_wide_counts(n->n_in, n->n_hidden, n->hidden, n->n_out);
  TdNetDev d{};
  d.n_in = n->n_in; d.ks1 = (n->n_in + 3) / 4; d.n_hidden = n->n_hidden; d.act = n->activation; d.na = n->n_out;
  d.widths = c.widths; d.nfrag = c.nfrag; d.nbias = c.nbias;
  if (wmax && c.wmax > *wmax) *wmax = c.wmax;
  return d;
}
size_t workspace_bytes(const TdNetDev& d) { return wide_workspace_bytes(d.nfrag, d.nbias); }
std::string net_text(const S2DTdNet* n) { return s2d_internal_wide_text(n->n_in, n->n_hidden, n->hidden, n->n_out); }

// one network of a call (`name`: what the header calls it): the shape, the parameters and the workspace
int check_net(const std::string& who, const char* name, const S2DTdNet* n, TdNetDev& d, int& wmax) {
  const std::string nm = who + ": " + name;
  if (s2d_internal_wide_shape(nm, &n->n_in, n->n_hidden, n->hidden, n->activation, n->n_out) != S2D_OK) return S2D_EINVAL;
  if (!n->params || misaligned(n->params, 16)) return fail(nm, "params must be a non-NULL, 16-byte aligned device pointer");
  d = net_dev(n, &wmax);
  if (s2d_internal_wide_workspace(nm, n->workspace, n->workspace_bytes, workspace_bytes(d), net_text(n), "s2d_td_workspace_bytes") != S2D_OK)
    return S2D_EINVAL;
  d.wf = static_cast<const float*>(n->workspace);
  return S2D_OK;
}
bool share(const S2DTdNet* a, const TdNetDev& da, const S2DTdNet* b, const TdNetDev& db) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(a->workspace), q = reinterpret_cast<uintptr_t>(b->workspace);
  return p < q + workspace_bytes(db) && q < p + workspace_bytes(da);
}
void pack(const S2DTdNet* n, const TdNetDev& d, hipStream_t s) { s2d_internal_wide_pack(wide_pack_args(d, d.n_in), n->params, n->workspace, s); }

// compute units of the current device (0: unknown), asked once per device
int compute_units() {
  static std::mutex mu;
  static int cus[kMaxDevices] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 0;
  std::lock_guard<std::mutex> lock(mu);
  if (!cus[dev] && hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus[dev] = 0;
  return cus[dev];
}

// The plan of a call: pitches from the widest padded hidden layer (wmax), the widest input (n_in) and the most outputs (na) of
// its networks; the first of (waves, tiles) = (4, 4) (4, 2) (4, 1) (2, 4) ... (1, 1) that 160 KiB hold (more waves go before more
// tiles, as wide_plan_lds; (1, 1) always fits: 16 x (324 + 2 x 452) + 64 x 68 words).  A learner's batch is small beside a
// rollout's env count (B = 4096 is 64 waves): the search starts at 2 waves per workgroup while the batch has fewer than 4 waves per
// compute unit and at 1 while it has fewer than 2, so that the workgroups spread over the device instead of filling a few units.
// S2D_TD_PLAN=waves,tiles in the environment, read at every launch, overrides the choice (testing: the results do not depend
// on it); a pair that is not of {4, 2, 1} or does not fit is refused.
int make_plan(const std::string& who, int64_t batch, int wmax, int n_in, int na, TdPlanDev& pl, int& waves, size_t& lds) {
  pl.rpitch = (wmax + 63) / 64 * 64 + 4;
  pl.xpitch = ((n_in + 3) / 4 * 4 + 63) / 64 * 64 + 4;
  pl.qpitch = (na + 15) / 16 * 16 + 4;
  const WidePlanOverride force = s2d_internal_plan_override("S2D_TD_PLAN");
  const int64_t batch_waves = (batch + kWave - 1) / kWave, cus = compute_units();
  const int most = force.waves ? kWavesPerBlock : batch_waves >= 4 * cus ? kWavesPerBlock : batch_waves >= 2 * cus ? 2 : 1;
  const auto words = [&](int t) { return t * 16 * (pl.xpitch + 2 * pl.rpitch) + kWave * pl.qpitch; };
  if (wide_plan_search(force, most, 0, words, waves, pl.tiles, pl.wave_words, lds)) return S2D_OK;
  return fail(who, wide_plan_refusal(force) + " of this call");
}
// the dynamic-LDS limit of a target kernel (`slot`: its number among the unit's instantiations) and the grid of a plan
int allow_lds(const std::string& who, const void* kernel, int slot) {
  if (allow_lds_slot<TdLds>(kernel, slot)) return S2D_OK;
  s2d_internal_set_error((who + ": hipGetDevice or hipFuncSetAttribute failed").c_str());
  return S2D_EHIP;
}
dim3 grid_of(int64_t batch, int waves) { return dim3((unsigned)((batch + waves * kWave - 1) / (waves * kWave))); }

// what both entry points ask of the batch arrays
int check_batch(const std::string& who, int64_t batch, const void* next_obs, const void* reward, const void* discount, const void* out_target,
                const void* opt1, const void* opt2) {
  if (batch < 1 || batch > INT32_MAX) return fail(who, "batch must be in [1, 2^31 - 1]");
  if (!next_obs || !reward || !discount || !out_target || misaligned(next_obs, 4) || misaligned(reward, 4) || misaligned(discount, 4) ||
      misaligned(out_target, 4))
    return fail(who, "next_obs, reward, discount and out_target must be non-NULL, 4-byte aligned device pointers");
  if (misaligned(opt1, 4) || misaligned(opt2, 4)) return fail(who, "the optional outputs must be 4-byte aligned device pointers (or NULL)");
  return S2D_OK;
}

// "<name> must not overlap an output" for the first of a head's device `words` that shares a byte with one of `outs` (NULL: not given)
struct TdSpan {
  const void* p;
  size_t bytes;
  const char* name;
};
int check_overlap(const std::string& who, std::initializer_list<TdSpan> words, std::initializer_list<TdSpan> outs) {
  for (const TdSpan& w : words) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(w.p);
    for (const TdSpan& o : outs) {
      const uintptr_t q = reinterpret_cast<uintptr_t>(o.p);
      if (o.p && p < q + o.bytes && q < p + w.bytes) return fail(who, std::string(w.name) + " must not overlap an output");
    }
  }
  return S2D_OK;
}
}  // namespace

int TdSacHead::check_words(const std::string& who, int64_t batch, int A, const float* out_target, const float* out_q, const float* out_action) const {
  const size_t rows = (size_t)batch * 4;
  if (misaligned(out_logp, 4)) return fail(who, "the optional outputs must be 4-byte aligned device pointers (or NULL)");
  if (!alpha || misaligned(alpha, 4)) return fail(who, "alpha must be a non-NULL, 4-byte aligned device pointer");
  if (!draws || misaligned(draws, 8)) return fail(who, "draws must be a non-NULL, 8-byte aligned device pointer");
  return check_overlap(who, {{draws, sizeof(uint64_t), "draws"}},
                       {{out_target, rows, "out_target"}, {out_q, rows, "out_q"}, {out_action, rows * A, "out_action"}, {out_logp, rows, "out_logp"}});
}
int TdTd3Head::check_words(const std::string& who, int64_t batch, int A, const float* out_target, const float* out_q, const float* out_action) const {
  const size_t rows = (size_t)batch * 4;
  if (!noise || misaligned(noise, 4)) return fail(who, "noise must be a non-NULL, 4-byte aligned device pointer (sigma, clip)");
  if (!draws || misaligned(draws, 8)) return fail(who, "draws must be a non-NULL, 8-byte aligned device pointer");
  return check_overlap(who, {{draws, sizeof(uint64_t), "draws"}, {noise, 2 * sizeof(float), "noise"}},
                       {{out_target, rows, "out_target"}, {out_q, rows, "out_q"}, {out_action, rows * A, "out_action"}});
}

S2D_API size_t s2d_td_workspace_bytes(const S2DTdNet* shape) {
  if (!shape || shape->n_in < 1 || shape->n_in > kTdMaxIn || !wide_shape_ok(shape->n_hidden, shape->hidden) || shape->n_out < 1 ||
      shape->n_out > 64)
    return 0;
  return workspace_bytes(net_dev(shape, nullptr));
}

S2D_API int s2d_td_target_q(int64_t batch, const S2DTdNet* target, const S2DTdNet* online, const float* next_obs, const float* reward,
                            const float* discount, float* out_target, float* out_q, int32_t* out_index, void* stream) {
  static const std::string who = "s2d_td_target_q";
  if (!target) return fail(who, "target is NULL");
  TdNetDev dt{}, dn{};
  int wmax = 0;
  if (check_net(who, "target", target, dt, wmax) != S2D_OK) return S2D_EINVAL;
  if (online) {
    if (check_net(who, "online", online, dn, wmax) != S2D_OK) return S2D_EINVAL;
    if (online->n_in != target->n_in || online->n_out != target->n_out)
      return fail(who, "online is " + net_text(online) + ", target " + net_text(target) + ": n_in and n_out must be the same");
    if (share(target, dt, online, dn)) return fail(who, "target and online share a workspace: every network of a call needs its own");
  }
  if (check_batch(who, batch, next_obs, reward, discount, out_target, out_q, out_index) != S2D_OK) return S2D_EINVAL;
  TdPlanDev pl{};
  int waves = 0;
  size_t lds = 0;
  if (make_plan(who, batch, wmax, target->n_in, target->n_out, pl, waves, lds) != S2D_OK) return S2D_EINVAL;
  const auto k = online ? s2d_td_target_q_kernel<true> : s2d_td_target_q_kernel<false>;
  if (allow_lds(who, reinterpret_cast<const void*>(k), online ? 1 : 0) != S2D_OK) return S2D_EHIP;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  pack(target, dt, s);
  if (online) pack(online, dn, s);
  hipLaunchKernelGGL(k, grid_of(batch, waves), dim3(waves * kWave), lds, s, dt, dn, pl, batch, next_obs, reward, discount, out_target, out_q,
                     out_index);
  return launched(who);
}

// The three actor-critic entry points (and SAC's diagnostic form).  The checks in order: the networks, the actor's n_out by the
// head's rule, the critics' shapes, shared workspaces, the batch arrays, the head's own words and their overlap with the outputs,
// the plan.  Then the pack launches, the target kernel and, where the head draws, the one-thread kernel that advances its counter.
template <class HEAD>
static int td_target_actor_critic(const std::string& who, int64_t batch, const S2DTdNet* actor, const S2DTdNet* critic1, const S2DTdNet* critic2,
                                  const float* next_obs, const float* reward, const float* discount, const HEAD& head, float* out_target,
                                  float* out_q, float* out_action, void* stream) {
  if (!actor || !critic1) return fail(who, "actor and critic1 must be non-NULL");
  TdNetDev da{}, d1{}, d2{};
  int wmax = 0;
  if (check_net(who, "actor", actor, da, wmax) != S2D_OK || check_net(who, "critic1", critic1, d1, wmax) != S2D_OK) return S2D_EINVAL;
  if (critic2 && check_net(who, "critic2", critic2, d2, wmax) != S2D_OK) return S2D_EINVAL;
  if (!HEAD::n_out_ok(actor->n_out)) return fail(who, HEAD::kNOutText);
  const int A = HEAD::actions(actor->n_out);
  for (const S2DTdNet* c : {critic1, critic2}) {
    if (!c) continue;
    if (c->n_in != actor->n_in + A || c->n_out != 1)
      return fail(who, std::string(c == critic1 ? "critic1" : "critic2") + " is " + net_text(c) + ", the actor " + net_text(actor) +
                           ": a critic's n_in must be the actor's " + HEAD::kCriticIn + ", its n_out 1");
  }
  if (share(actor, da, critic1, d1) || (critic2 && (share(actor, da, critic2, d2) || share(critic1, d1, critic2, d2))))
    return fail(who, "two networks share a workspace: every network of a call needs its own");
  if (check_batch(who, batch, next_obs, reward, discount, out_target, out_q, out_action) != S2D_OK) return S2D_EINVAL;
  if (head.check_words(who, batch, A, out_target, out_q, out_action) != S2D_OK) return S2D_EINVAL;
  TdPlanDev pl{};
  int waves = 0;
  size_t lds = 0;
  if (make_plan(who, batch, wmax, critic1->n_in, actor->n_out, pl, waves, lds) != S2D_OK) return S2D_EINVAL;
  const auto k = critic2 ? s2d_td_target_ac_kernel<HEAD, true> : s2d_td_target_ac_kernel<HEAD, false>;
  if (allow_lds(who, reinterpret_cast<const void*>(k), HEAD::kSlot + (critic2 ? 1 : 0)) != S2D_OK) return S2D_EHIP;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  pack(actor, da, s);
  pack(critic1, d1, s);
  if (critic2) pack(critic2, d2, s);
  hipLaunchKernelGGL(k, grid_of(batch, waves), dim3(waves * kWave), lds, s, da, d1, d2, pl, batch, next_obs, reward, discount, head, out_target,
                     out_q, out_action);
  if (uint64_t* const draws = head.counter()) hipLaunchKernelGGL(s2d_td_draws_kernel, dim3(1), dim3(1), 0, s, draws);
  return launched(who);
}

S2D_API int s2d_td_target_ac(int64_t batch, const S2DTdNet* actor, const S2DTdNet* critic1, const S2DTdNet* critic2, const float* next_obs,
                             const float* reward, const float* discount, float* out_target, float* out_q, float* out_action, void* stream) {
  static const std::string who = "s2d_td_target_ac";
  return td_target_actor_critic(who, batch, actor, critic1, critic2, next_obs, reward, discount, TdTanhHead{}, out_target, out_q, out_action,
                                stream);
}

S2D_API int s2d_td_target_td3(int64_t batch, const S2DTdNet* actor, const S2DTdNet* critic1, const S2DTdNet* critic2, const float* next_obs,
                              const float* reward, const float* discount, const float* noise, uint64_t* draws, uint64_t seed,
                              float* out_target, float* out_q, float* out_action, void* stream) {
  static const std::string who = "s2d_td_target_td3";
  const TdTd3Head head{noise, draws, (uint32_t)seed, (uint32_t)(seed >> 32)};
  return td_target_actor_critic(who, batch, actor, critic1, critic2, next_obs, reward, discount, head, out_target, out_q, out_action, stream);
}

S2D_API int s2d_td_target_sac(int64_t batch, const S2DTdNet* actor, const S2DTdNet* critic1, const S2DTdNet* critic2, const float* next_obs,
                              const float* reward, const float* discount, const float* alpha, uint64_t* draws, uint64_t seed,
                              float* out_target, float* out_q, float* out_action, float* out_logp, void* stream) {
  static const std::string who = "s2d_td_target_sac";
  const TdSacHead head{alpha, draws, (uint32_t)seed, (uint32_t)(seed >> 32), 0, out_logp};
  return td_target_actor_critic(who, batch, actor, critic1, critic2, next_obs, reward, discount, head, out_target, out_q, out_action, stream);
}

// its diagnostic form (deterministic != 0: z = 0, no draw)
S2D_API int s2d_debug_td_target_sac(int64_t batch, const S2DTdNet* actor, const S2DTdNet* critic1, const S2DTdNet* critic2,
                                    const float* next_obs, const float* reward, const float* discount, const float* alpha, uint64_t* draws,
                                    uint64_t seed, int deterministic, float* out_target, float* out_q, float* out_action, float* out_logp,
                                    void* stream) {
  static const std::string who = "s2d_debug_td_target_sac";
  const TdSacHead head{alpha, draws, (uint32_t)seed, (uint32_t)(seed >> 32), deterministic, out_logp};
  return td_target_actor_critic(who, batch, actor, critic1, critic2, next_obs, reward, discount, head, out_target, out_q, out_action, stream);
}
