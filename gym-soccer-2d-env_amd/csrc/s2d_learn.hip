// s2d_learn.hip -- one gradient step of a Q-network on a sampled batch (include/s2d.h S2DLearnNet / S2DLearnState, s2d_learn_q /
// s2d_learn_q_grad): forward, TD error and its MSE / Huber derivative, backward, gradient-norm clip and Adam,
// the link between s2d_td_target_q and the priority update.  Engine-independent, as s2d_td_* and s2d_replay_*: raw device
// pointers, any stream of the current device, parameters, hyper-parameters and step state all read when the kernels run, a linear
// chain of three launches on one stream.  The same chain steps a DDPG / TD3 critic on [obs | action] (s2d_learn_critic) and the
// actor through a critic whose parameters are only read (s2d_learn_actor: loss = -mean Q(obs, tanh(mu(obs)))).
//
// Every chain is the spec's (tests/learn_ref.c), on the VALU:
//   forward    acc = b[j]; k ascending: acc = fmaf(W[j][k], in[k], acc)      -- the bits of s2d_td_target_q and the wide actors
//   backward   s = +0; j ascending: s = fmaf(W[j][k], delta[j], s), times the activation's derivative from the stored output
//   dW, db     per block of S2D_LEARN_BLOCK_ROWS rows: acc = +0; rows ascending: acc = fmaf(delta[row][j], in[row][k], acc)
// so no result depends on the grid, the waves of a workgroup, where the activations live or the number of compute units, and there
// is no float atomic anywhere: block partials go to the workspace and are added in ascending block order.
//
//   s2d_learn_block_kernel   one workgroup (4 waves) per block of 64 rows.  A row of the block's image holds
//                            [x: 4 ceil(n_in / 4) | y_1: h_1 | ... | y_L: h_L | q: n_out]; a layer's delta overwrites its output once
//                            that has been used.  The image is in LDS where 64 rows (and the rows' 64 losses) fit 160 KiB,
//                            else in the workspace.
//                            forward and delta: lane = row, a wave takes tiles of 8 units, the weights are wave-uniform;
//                            dW: a thread takes 4 units x one input, the rows are the chain.
//   s2d_learn_critic_kernel  the same for a critic on [obs | action], the row assembled in the kernel; its loops are the device
//                            functions learn_forward / learn_backward, which restate the block kernel's (that kernel keeps its
//                            inlined text: through the functions it ran 3-5 % slower).
//   s2d_learn_actor_kernel   the same workgroup and block with both networks' rows in the image: actor forward, tanh head, critic
//                            forward, the critic's deltas down to the action columns of its input (no critic dW or db), the head's
//                            derivative, the actor's backward pass.
//   s2d_learn_reduce_kernel  grad[p] = block partials in ascending order; per chunk of S2D_LEARN_NORM_CHUNK words the sum of
//                            squares, fmaf ascending; (step) the beta products are multiplied here, once per call.
//   s2d_learn_finish_kernel  chunks added ascending, norm, clip scale, mean loss; (step) Adam on every word.
// The PPO step (s2d_learn_ppo: a policy net and a value net on one observation, a categorical or Gaussian head, one flat
// [pi | vf | log_std] buffer under one clip and one Adam; tests/learn_ppo_ref.c) adds
//   s2d_learn_ppo_norm_kernel   the advantage's mean and standard deviation over the rows the minibatch names, a launch of its own
//   s2d_learn_ppo_block_kernel  one workgroup per GROUP of ceil(blocks / 256) consecutive blocks: rows gathered by index, both
//                               forwards, the head and the clipped surrogate (lane = row), both backward passes with the dW / db
//                               chains continued across the group's blocks, so the partials are at most 256 x P words
// and runs the reduce and finish kernels with their PPO flag (log_std's entropy term, eight statistics).
// The SAC actor step (s2d_learn_sac_actor: the squashed-Gaussian actor through min(Q1, Q2), reparameterised, and the temperature;
// tests/learn_sac_ref.c) adds
//   s2d_learn_sac_kernel        the actor kernel's workgroup and block with three networks' rows and the head's z in the image: actor
//                               forward, the head of s2d_sac_head.h on a Philox stream of its own (lane = row), both critics forward,
//                               the row's minimum, both critics' delta passes, the head's derivative on the chosen critic's action
//                               columns, the actor's backward pass; two rows of block partials (loss, logp)
//   s2d_learn_sac_alpha_kernel  ONE THREAD, a launch of its own behind the finish kernel: the mean of logp, log_alpha's Adam step,
//                               *alpha and *draws += 1.  (The other choice, a flag on the finish kernel as PPO took, would have
//                               changed that kernel's text; this way its existing instantiations are the ones the other learners run.)
// and runs the reduce and finish kernels as the DDPG actor step does, so the call stays a linear chain on one stream.
//
// The host path is one for the four learners.  layout() places every workspace from the stepped parameter count, the image's pitch,
// the words a row keeps beside the image, the rows of partials and the learner's extra parts.  An entry point reads what it steps
// into a Stepped view (from S2DLearnNet + S2DLearnState, or from S2DLearnPPO), on which buffers_error checks the pointers and
// layout_error the workspace's size and, through a Spans list, the overlaps; pair_error checks an actor with its critic(s).
// launch_block picks the block kernel's instantiation, sizes its LDS, takes the 48 KiB attribute step and launches;
// reduce_and_finish enqueues the two kernels behind it.  The order of the checks is the order of the refusals, which
// tests/test_learn_refusals_host.py pins sentence by sentence.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "s2d_sac_head.h"
#include "s2d_wide_net.h"

static constexpr int kLearnRows = S2D_LEARN_BLOCK_ROWS;
static constexpr int kLearnChunk = S2D_LEARN_NORM_CHUNK;
static constexpr int kLearnThreads = 256;
static constexpr int kLearnMaxHidden = 4;
static constexpr int kLearnMaxAction = 8;   // the actor's outputs, as s2d_td_target_ac
static constexpr int kLearnMaxObs = 248;    // so that [obs | action] stays within the grid's 256 inputs
static constexpr int kPpoMaxGroups = S2D_LEARN_PPO_MAX_GROUPS;
static constexpr int kPpoStatWords = 8;     // a group's partials of the five statistics, padded
static constexpr int kPpoRowWords = 6;      // beside the image, per row of the block: its source row and its five statistics
static constexpr int kPpoNormThreads = 1024;
static constexpr int kSacRowWords = 3;     // beside the image, per row of the block: its loss, its logp and the critic it chose
static_assert(kLearnRows == kWave, "lane = row of the block");
static_assert(kLearnChunk == kLearnThreads, "one thread per word of a chunk");

// the network as the kernels see it (no array indexed by the layer: it would live in scratch)
struct LearnDev {
  int n_in, kp;        // input width and its padded row: 4 ceil(n_in / 4)
  int n_hidden, act;   // L in 1 .. 4; 0 relu, 1 tanh_spec, 2 sigmoid_spec
  uint32_t widths;     // h_l / 8 in bits 8 (l - 1) .. 8 l - 1
  int na;              // outputs, 1 .. 64
  int P;               // parameters
  int pitch;           // words of a row of the block's image
};
S2D_DEV int learn_width(const LearnDev& d, int l) { return l < d.n_hidden ? 8 * (int)((d.widths >> (8 * l)) & 255u) : d.na; }

S2D_DEV float learn_dact(int act, float y, float s) {
  if (act == 0) return y > 0.0f ? s : 0.0f;
  if (act == 1) return s * (1.0f - y * y);
  return s * (y * (1.0f - y));
}

template <bool LDS>
__global__ __launch_bounds__(kLearnThreads) void s2d_learn_block_kernel(LearnDev d, int64_t batch, int loss_kind,
                                                                        const float* __restrict__ params, float* __restrict__ part,
                                                                        float* __restrict__ loss_part, float* __restrict__ image,
                                                                        const float* __restrict__ obs, const int32_t* __restrict__ action,
                                                                        const float* __restrict__ target, const float* __restrict__ weight,
                                                                        float* __restrict__ out_td_abs, float* __restrict__ out_q,
                                                                        int32_t* __restrict__ error) {
  extern __shared__ __attribute__((aligned(16))) float smem[];   // [the rows' losses: 64 | the image, if it lives here]
  float* const row_loss = smem;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int64_t row0 = (int64_t)blockIdx.x * kLearnRows;
  const int rows = (int)(batch - row0 < kLearnRows ? batch - row0 : kLearnRows);
  const int pitch = d.pitch, L = d.n_hidden, A = d.na;
  float* const img = LDS ? smem + kLearnRows : image + (size_t)blockIdx.x * kLearnRows * pitch;

  // the block's input rows, zeros past n_in and past the batch
  for (int idx = tid; idx < kLearnRows * d.kp; idx += kLearnThreads) {
    const int r = idx / d.kp, k = idx - r * d.kp;
    img[r * pitch + k] = (r < rows && k < d.n_in) ? obs[(row0 + r) * d.n_in + k] : 0.0f;
  }
  __syncthreads();

  // ---- forward
  int in_off = 0, win = d.n_in, kk = d.kp, po = 0;
  for (int l = 0; l <= L; ++l) {
    const int wout = learn_width(d, l), out_off = in_off + kk;
    const float* const W = params + po;
    const float* const b = W + wout * win;
    const float* const in = img + lane * pitch + in_off;
    float* const out = img + lane * pitch + out_off;
    const int act = l < L ? d.act : 3;
    for (int j0 = 8 * wv; j0 < wout; j0 += 8 * (kLearnThreads / kWave)) {
      float acc[8];
      int jc[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        jc[u] = j0 + u < wout ? j0 + u : wout - 1;
        acc[u] = b[jc[u]];
      }
      for (int k = 0; k < win; ++k) {
        const float x = in[k];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] = fmaf(W[jc[u] * win + k], x, acc[u]);
      }
      for (int k = win; k < kk; ++k) {            // layer 1's terms past n_in: x_k = 0 against zero weights
        const float x = in[k];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] = fmaf(0.0f, x, acc[u]);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float v = acc[u];
        const float y = act == 0 ? (v > 0.0f ? v : 0.0f) : act == 1 ? tanh_spec(v) : act == 2 ? sigmoid_spec(v) : v;
        if (j0 + u < wout) out[j0 + u] = y;
      }
    }
    __syncthreads();
    po += wout * win + wout;
    in_off = out_off; win = wout; kk = wout;
  }
  // in_off: the output layer's columns; po == P

  // ---- the rows' outputs, TD errors, losses and output deltas
  if (out_q)
    for (int idx = tid; idx < rows * A; idx += kLearnThreads) {
      const int r = idx / A, j = idx - r * A;
      out_q[(row0 + r) * A + j] = img[r * pitch + in_off + j];
    }
  __syncthreads();
  if (tid < kLearnRows) {
    float* const q = img + tid * pitch + in_off;
    float g = 0.0f, wl = 0.0f;
    int a = -1;
    if (tid < rows) {
      const int64_t i = row0 + tid;
      const int32_t ai = action[i];
      const bool ok = ai >= 0 && ai < A;
      if (!ok) atomicOr(error, 1);
      const float e = ok ? q[ai] - target[i] : 0.0f;
      if (out_td_abs) out_td_abs[i] = fabsf(e);
      const float w = weight ? weight[i] : 1.0f;
      const float sq = (0.5f * e) * e, ab = fabsf(e);
      const float l1 = loss_kind == 0 ? sq : (ab <= 1.0f ? sq : ab - 0.5f);
      const float dd = loss_kind == 0 ? e : (e < -1.0f ? -1.0f : (e > 1.0f ? 1.0f : e));
      wl = ok ? w * l1 : 0.0f;
      g = (w * dd) / (float)batch;
      a = ok ? ai : -1;
    }
    for (int j = 0; j < A; ++j) q[j] = j == a ? g : 0.0f;
    row_loss[tid] = wl;
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.0f;
    for (int r = 0; r < rows; ++r) s = s + row_loss[r];
    loss_part[blockIdx.x] = s;
  }

  // ---- backward, layer L down to 0
  float* const mine = part + (size_t)blockIdx.x * d.P;
  int out_off = in_off;
  for (int l = L; l >= 0; --l) {
    const int wout = learn_width(d, l);
    win = l ? learn_width(d, l - 1) : d.n_in;
    in_off = out_off - (l ? win : d.kp);
    po -= wout * win + wout;
    // this block's dW: 4 units x one input per thread, rows ascending
    const int items = ((wout + 3) >> 2) * win;
    for (int idx = tid; idx < items; idx += kLearnThreads) {
      const int jt = idx / win, k = idx - jt * win, j0 = 4 * jt;
      int jc[4];
      float acc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        jc[u] = out_off + (j0 + u < wout ? j0 + u : wout - 1);
        acc[u] = 0.0f;
      }
      for (int r = 0; r < rows; ++r) {
        const float* const row = img + r * pitch;
        const float x = row[in_off + k];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = fmaf(row[jc[u]], x, acc[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (j0 + u < wout) mine[po + (j0 + u) * win + k] = acc[u];
    }
    for (int j = tid; j < wout; j += kLearnThreads) {
      float acc = 0.0f;
      for (int r = 0; r < rows; ++r) acc = fmaf(img[r * pitch + out_off + j], 1.0f, acc);
      mine[po + wout * win + j] = acc;
    }
    __syncthreads();
    if (l) {
      // the delta of the layer below over its stored output: lane = row, 8 units a tile (hidden widths are multiples of 8)
      const float* const W = params + po;
      const float* const dl = img + lane * pitch + out_off;
      float* const y = img + lane * pitch + in_off;
      for (int k0 = 8 * wv; k0 < win; k0 += 8 * (kLearnThreads / kWave)) {
        float s[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) s[u] = 0.0f;
        for (int j = 0; j < wout; ++j) {
          const float dj = dl[j];
#pragma unroll
          for (int u = 0; u < 8; ++u) s[u] = fmaf(W[j * win + k0 + u], dj, s[u]);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) y[k0 + u] = learn_dact(d.act, y[k0 + u], s[u]);
      }
      __syncthreads();
    }
    out_off = in_off;
  }
}

// The layers of `d` on the block's image, lane = row, a wave takes tiles of 8 units, the weights are wave-uniform.  Layer 1 reads
// d.n_in words at column x_off (and the zeros up to d.kp against zero weights); layer l's output follows layer l - 1's from column
// y_off on.  Returns the column of the output layer (linear).  Ends behind a barrier.
S2D_DEV int learn_forward(const LearnDev& d, const float* __restrict__ params, float* img, int pitch, int x_off, int y_off, int lane, int wv) {
  const int L = d.n_hidden;
  int in_off = x_off, out_off = y_off, win = d.n_in, kk = d.kp, po = 0;
  for (int l = 0; l <= L; ++l) {
    const int wout = learn_width(d, l);
    const float* const W = params + po;
    const float* const b = W + wout * win;
    const float* const in = img + lane * pitch + in_off;
    float* const out = img + lane * pitch + out_off;
    const int act = l < L ? d.act : 3;
    for (int j0 = 8 * wv; j0 < wout; j0 += 8 * (kLearnThreads / kWave)) {
      float acc[8];
      int jc[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        jc[u] = j0 + u < wout ? j0 + u : wout - 1;
        acc[u] = b[jc[u]];
      }
      for (int k = 0; k < win; ++k) {
        const float x = in[k];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] = fmaf(W[jc[u] * win + k], x, acc[u]);
      }
      for (int k = win; k < kk; ++k) {            // layer 1's terms past n_in: x_k = 0 against zero weights
        const float x = in[k];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] = fmaf(0.0f, x, acc[u]);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float v = acc[u];
        const float y = act == 0 ? (v > 0.0f ? v : 0.0f) : act == 1 ? tanh_spec(v) : act == 2 ? sigmoid_spec(v) : v;
        if (j0 + u < wout) out[j0 + u] = y;
      }
    }
    __syncthreads();
    po += wout * win + wout;
    in_off = out_off; win = wout; kk = wout;
    if (l < L) out_off += wout;
  }
  return out_off;
}

// Backward from the output layer's deltas at column q_off (the layout is learn_forward's), layer L down to 0.  GRADS: this block's
// dW and db into mine[P], 4 units x one input per thread, rows ascending.  Every hidden layer's delta overwrites its stored
// output; !GRADS (a network whose parameters are only read) stops with layer 1's delta at column y_off.  Called behind a barrier,
// ends behind one.
// CONT (s2d_learn_ppo: a workgroup takes several blocks): every dW / db chain starts at +0 only where `first`, else it goes on from the
// partial stored in mine[].
template <bool GRADS, bool CONT = false>
S2D_DEV void learn_backward(const LearnDev& d, const float* __restrict__ params, float* __restrict__ mine, float* img, int pitch, int rows,
                            int x_off, int q_off, int tid, int lane, int wv, bool first = true) {
  int out_off = q_off, po = d.P;
  for (int l = d.n_hidden; l >= 0; --l) {
    const int wout = learn_width(d, l), win = l ? learn_width(d, l - 1) : d.n_in;
    const int in_off = l ? out_off - win : x_off;
    po -= wout * win + wout;
    if (GRADS) {
      const int items = ((wout + 3) >> 2) * win;
      for (int idx = tid; idx < items; idx += kLearnThreads) {
        const int jt = idx / win, k = idx - jt * win, j0 = 4 * jt;
        int jc[4];
        float acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = j0 + u < wout ? j0 + u : wout - 1;
          jc[u] = out_off + j;
          acc[u] = CONT && !first ? mine[po + j * win + k] : 0.0f;
        }
        for (int r = 0; r < rows; ++r) {
          const float* const row = img + r * pitch;
          const float x = row[in_off + k];
#pragma unroll
          for (int u = 0; u < 4; ++u) acc[u] = fmaf(row[jc[u]], x, acc[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (j0 + u < wout) mine[po + (j0 + u) * win + k] = acc[u];
      }
      for (int j = tid; j < wout; j += kLearnThreads) {
        float acc = CONT && !first ? mine[po + wout * win + j] : 0.0f;
        for (int r = 0; r < rows; ++r) acc = fmaf(img[r * pitch + out_off + j], 1.0f, acc);
        mine[po + wout * win + j] = acc;
      }
      __syncthreads();
    }
    if (l) {
      // the delta of the layer below over its stored output: lane = row, 8 units a tile (hidden widths are multiples of 8)
      const float* const W = params + po;
      const float* const dl = img + lane * pitch + out_off;
      float* const y = img + lane * pitch + in_off;
      for (int k0 = 8 * wv; k0 < win; k0 += 8 * (kLearnThreads / kWave)) {
        float s[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) s[u] = 0.0f;
        for (int j = 0; j < wout; ++j) {
          const float dj = dl[j];
#pragma unroll
          for (int u = 0; u < 8; ++u) s[u] = fmaf(W[j * win + k0 + u], dj, s[u]);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) y[k0 + u] = learn_dact(d.act, y[k0 + u], s[u]);
      }
      __syncthreads();
    }
    out_off = in_off;
  }
}

// s2d_learn_critic: the row is [obs[b]: D words | act_in[b]: n_in - D words], assembled here; the one output column takes the delta.
// The loops are learn_forward's and learn_backward's, the chains s2d_learn_block_kernel's.
template <bool LDS>
__global__ __launch_bounds__(kLearnThreads) void s2d_learn_critic_kernel(LearnDev d, int64_t batch, int loss_kind,
                                                                         const float* __restrict__ params, float* __restrict__ part,
                                                                         float* __restrict__ loss_part, float* __restrict__ image,
                                                                         const float* __restrict__ obs, int D, const float* __restrict__ act_in,
                                                                         const float* __restrict__ target, const float* __restrict__ weight,
                                                                         float* __restrict__ out_td_abs, float* __restrict__ out_q) {
  extern __shared__ __attribute__((aligned(16))) float smem[];   // [the rows' losses: 64 | the image, if it lives here]
  float* const row_loss = smem;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int64_t row0 = (int64_t)blockIdx.x * kLearnRows;
  const int rows = (int)(batch - row0 < kLearnRows ? batch - row0 : kLearnRows);
  const int pitch = d.pitch;
  float* const img = LDS ? smem + kLearnRows : image + (size_t)blockIdx.x * kLearnRows * pitch;

  for (int idx = tid; idx < kLearnRows * d.kp; idx += kLearnThreads) {
    const int r = idx / d.kp, k = idx - r * d.kp;
    float x = 0.0f;
    if (r < rows && k < d.n_in) x = k < D ? obs[(row0 + r) * D + k] : act_in[(row0 + r) * (d.n_in - D) + (k - D)];
    img[r * pitch + k] = x;
  }
  __syncthreads();
  const int q_off = learn_forward(d, params, img, pitch, 0, d.kp, lane, wv);

  // ---- the rows' values, TD errors, losses and output deltas
  if (tid < kLearnRows) {
    float g = 0.0f, wl = 0.0f;
    if (tid < rows) {
      const int64_t i = row0 + tid;
      const float q = img[tid * pitch + q_off];
      if (out_q) out_q[i] = q;
      const float e = q - target[i];
      if (out_td_abs) out_td_abs[i] = fabsf(e);
      const float w = weight ? weight[i] : 1.0f;
      const float sq = (0.5f * e) * e, ab = fabsf(e);
      const float l1 = loss_kind == S2D_LEARN_SQUARE ? e * e : loss_kind == S2D_LEARN_MSE ? sq : (ab <= 1.0f ? sq : ab - 0.5f);
      const float dd = loss_kind == S2D_LEARN_SQUARE ? 2.0f * e : loss_kind == S2D_LEARN_MSE ? e : (e < -1.0f ? -1.0f : (e > 1.0f ? 1.0f : e));
      wl = w * l1;
      g = (w * dd) / (float)batch;
    }
    img[tid * pitch + q_off] = g;
    row_loss[tid] = wl;
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.0f;
    for (int r = 0; r < rows; ++r) s = s + row_loss[r];
    loss_part[blockIdx.x] = s;
  }
  learn_backward<true>(d, params, part + (size_t)blockIdx.x * d.P, img, pitch, rows, 0, q_off, tid, lane, wv);
}

// s2d_learn_actor: loss = -mean_b Q(obs_b, tanh(mu(obs_b))).  A row of the image holds both networks' rows:
// [x: c.kp = 4 ceil((D + A) / 4) | the actor's y_1 .. y_L | a: A | the critic's y_1 .. y_L | q: 1].  The actor reads the D
// observation words (its padded terms end before the action or on the zeros behind D, as in s2d_td_target_ac), its tanh'ed outputs
// go behind them and stay in the actor's output columns for the head's derivative; the critic reads the whole row.  The critic's
// backward pass forms deltas only (no dW, no db) and ends with the A action columns of its input delta.
template <bool LDS>
__global__ __launch_bounds__(kLearnThreads) void s2d_learn_actor_kernel(LearnDev a, LearnDev c, int pitch, int64_t batch,
                                                                        const float* __restrict__ aparams, const float* __restrict__ cparams,
                                                                        float* __restrict__ part, float* __restrict__ loss_part,
                                                                        float* __restrict__ image, const float* __restrict__ obs,
                                                                        float* __restrict__ out_action, float* __restrict__ out_q) {
  extern __shared__ __attribute__((aligned(16))) float smem[];   // [the rows' q: 64 | the image, if it lives here]
  float* const row_q = smem;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int64_t row0 = (int64_t)blockIdx.x * kLearnRows;
  const int rows = (int)(batch - row0 < kLearnRows ? batch - row0 : kLearnRows);
  const int D = a.n_in, A = a.na;
  float* const img = LDS ? smem + kLearnRows : image + (size_t)blockIdx.x * kLearnRows * pitch;

  for (int idx = tid; idx < kLearnRows * c.kp; idx += kLearnThreads) {
    const int r = idx / c.kp, k = idx - r * c.kp;
    img[r * pitch + k] = (r < rows && k < D) ? obs[(row0 + r) * D + k] : 0.0f;
  }
  __syncthreads();
  // ---- forward: the actor, its head, the critic
  const int a_off = learn_forward(a, aparams, img, pitch, 0, c.kp, lane, wv);
  for (int idx = tid; idx < kLearnRows * A; idx += kLearnThreads) {
    const int r = idx / A, i = idx - r * A;
    const float v = tanh_spec(img[r * pitch + a_off + i]);
    img[r * pitch + a_off + i] = v;
    img[r * pitch + D + i] = v;
    if (out_action && r < rows) out_action[(row0 + r) * A + i] = v;
  }
  __syncthreads();
  const int cy_off = a_off + A;
  const int q_off = learn_forward(c, cparams, img, pitch, 0, cy_off, lane, wv);
  if (tid < kLearnRows) {
    const float q = img[tid * pitch + q_off];
    if (tid < rows && out_q) out_q[row0 + tid] = q;
    row_q[tid] = q;
    img[tid * pitch + q_off] = tid < rows ? -1.0f / (float)batch : 0.0f;
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.0f;
    for (int r = 0; r < rows; ++r) s = s + row_q[r];
    loss_part[blockIdx.x] = s;                      // the finish kernel negates the sum
  }
  // ---- backward through the critic: deltas only, then the action columns D .. D + A - 1 of its input delta and the head
  learn_backward<false>(c, cparams, nullptr, img, pitch, rows, 0, q_off, tid, lane, wv);
  {
    const int h1 = learn_width(c, 0), win = c.n_in;
    const float* const d1 = img + lane * pitch + cy_off;
    for (int i = wv; i < A; i += kLearnThreads / kWave) {
      float s = 0.0f;
      for (int j = 0; j < h1; ++j) s = fmaf(cparams[j * win + D + i], d1[j], s);
      float* const y = img + lane * pitch + a_off + i;
      *y = learn_dact(1, *y, s);
    }
  }
  __syncthreads();
  learn_backward<true>(a, aparams, part + (size_t)blockIdx.x * a.P, img, pitch, rows, 0, a_off, tid, lane, wv);
}

// ------------------------------------------------------------------------------------------ SAC (s2d_learn_sac_actor)
// what the SAC actor kernel reads of a call besides the three networks
struct SacArgs {
  int pitch, z_off, twin;                    // the image's row; the column of the head's z words; critic 2 is there
  int64_t batch;
  const float* aparams;
  const float* c1params;
  const float* c2params;
  float* part;                               // [blocks][P of the actor]
  float* loss_part;                          // [blocks]: the rows' alpha * logp - q
  float* logp_part;                          // [blocks]: the rows' logp
  float* image;                              // [blocks][64][pitch], if not in LDS
  const float* obs;
  const float* alpha;                        // one device word: ent_coef
  const uint64_t* draws;                     // one device word: the steps so far
  uint32_t seed_lo, seed_hi;
  float* out_action;
  float* out_logp;
  float* out_q;
};

// s2d_learn_sac_actor: loss = mean_b (alpha * logp_b - min(Q1, Q2)(obs_b, a_b)), a_b drawn by the squashed-Gaussian head.  A row of
// the image holds all three networks' rows and the head's words:
// [x: c1.kp = 4 ceil((D + A) / 4) | the actor's y_1 .. y_L | mean: A, v: A | critic 1's y_1 .. y_L | q1: 1 | critic 2's y_1 .. y_L | q2: 1 | z: A].
// The head (lane = row) writes a behind the observation words, where the critics read it and the head's derivative finds it again; v
// stays in the actor's output columns and z in its own until the derivative has been formed.  Both critics' backward passes form
// deltas only (no dW, no db) with the output delta -1 / B; the head's derivative takes the action columns of the CHOSEN critic's
// input delta (row_sel), so the other's words never reach a result.
template <bool LDS>
__global__ __launch_bounds__(kLearnThreads) void s2d_learn_sac_kernel(LearnDev a, LearnDev c1, LearnDev c2, SacArgs g) {
  extern __shared__ __attribute__((aligned(16))) float smem[];   // [the rows' losses: 64 | logp: 64 | chosen critic: 64 | the image, if it lives here]
  float* const row_loss = smem;
  float* const row_logp = smem + kLearnRows;
  int* const row_sel = reinterpret_cast<int*>(smem + 2 * kLearnRows);
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int64_t row0 = (int64_t)blockIdx.x * kLearnRows;
  const int rows = (int)(g.batch - row0 < kLearnRows ? g.batch - row0 : kLearnRows);
  const int D = a.n_in, A = a.na >> 1, pitch = g.pitch, z_off = g.z_off;
  const bool twin = g.twin != 0;
  float* const img = LDS ? smem + kSacRowWords * kLearnRows : g.image + (size_t)blockIdx.x * kLearnRows * pitch;
  const float alpha = *g.alpha;
  const uint64_t draws = *g.draws;

  for (int idx = tid; idx < kLearnRows * c1.kp; idx += kLearnThreads) {
    const int r = idx / c1.kp, k = idx - r * c1.kp;
    img[r * pitch + k] = (r < rows && k < D) ? g.obs[(row0 + r) * D + k] : 0.0f;
  }
  __syncthreads();
  // ---- forward: the actor, its head, the critics
  const int y_off = learn_forward(a, g.aparams, img, pitch, 0, c1.kp, lane, wv);
  if (tid < kLearnRows) {
    float* const row = img + tid * pitch;
    const int64_t i = row0 + tid;                      // the absolute row: nothing depends on the grid
    float z[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const U4 w = philox4x32_10((uint32_t)i, (uint32_t)draws, (uint32_t)(draws >> 32), (uint32_t)S2D_LEARN_SAC_STREAM << 16, g.seed_lo,
                               g.seed_hi);
    box_muller(w.x, w.y, z[0], z[1]);
    box_muller(w.z, w.w, z[2], z[3]);
    if (A > 4) {
      const U4 w2 = philox4x32_10((uint32_t)i, (uint32_t)draws, (uint32_t)(draws >> 32), ((uint32_t)S2D_LEARN_SAC_STREAM << 16) | 1u,
                                  g.seed_lo, g.seed_hi);
      box_muller(w2.x, w2.y, z[4], z[5]);
      box_muller(w2.z, w2.w, z[6], z[7]);
    }
    float lp = 0.0f;
#pragma unroll
    for (int j = 0; j < kLearnMaxAction; ++j) {
      if (j < A) {
        float act;
        const float term = sac_head_term(row[y_off + j], row[y_off + A + j], z[j], false, act);
        lp = j == 0 ? term : lp + term;
        row[D + j] = act;
        row[z_off + j] = z[j];
        if (g.out_action && tid < rows) g.out_action[i * A + j] = act;
      }
    }
    row_logp[tid] = lp;
  }
  __syncthreads();
  const int c1y_off = y_off + 2 * A;
  const int q1_off = learn_forward(c1, g.c1params, img, pitch, 0, c1y_off, lane, wv);
  const int c2y_off = q1_off + 1;
  const int q2_off = twin ? learn_forward(c2, g.c2params, img, pitch, 0, c2y_off, lane, wv) : q1_off;
  if (tid < kLearnRows) {
    float* const row = img + tid * pitch;
    const float q1 = row[q1_off], lp = row_logp[tid];
    float q = q1;
    int sel = 0;
    if (twin) {
      const float q2 = row[q2_off];
      if (q2 < q1) {                                   // a tie or a NaN q2 keeps critic 1
        q = q2;
        sel = 1;
      }
    }
    if (tid < rows) {
      if (g.out_q) g.out_q[row0 + tid] = q;
      if (g.out_logp) g.out_logp[row0 + tid] = lp;
    }
    row_loss[tid] = __fsub_rn(__fmul_rn(alpha, lp), q);   // one multiply, then one subtract
    row_sel[tid] = sel;
    const float dq = tid < rows ? -1.0f / (float)g.batch : 0.0f;
    row[q1_off] = dq;
    if (twin) row[q2_off] = dq;
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.0f;
    for (int r = 0; r < rows; ++r) s = s + row_loss[r];
    g.loss_part[blockIdx.x] = s;
  }
  if (tid == kWave) {                                    // another wave's lane 0
    float s = 0.0f;
    for (int r = 0; r < rows; ++r) s = s + row_logp[r];
    g.logp_part[blockIdx.x] = s;
  }
  // ---- backward through both critics: deltas only; then the action columns of the chosen critic's input delta and the head
  learn_backward<false>(c1, g.c1params, nullptr, img, pitch, rows, 0, q1_off, tid, lane, wv);
  if (twin) learn_backward<false>(c2, g.c2params, nullptr, img, pitch, rows, 0, q2_off, tid, lane, wv);
  {
    const float w = alpha / (float)g.batch;
    float* const row = img + lane * pitch;
    const int win = c1.n_in;
    for (int j = wv; j < A; j += kLearnThreads / kWave) {
      float s = 0.0f;
      {
        const int h1 = learn_width(c1, 0);
        const float* const d1 = row + c1y_off;
        for (int k = 0; k < h1; ++k) s = fmaf(g.c1params[k * win + D + j], d1[k], s);
      }
      if (twin) {
        const int h1 = learn_width(c2, 0);
        const float* const d1 = row + c2y_off;
        float s2 = 0.0f;
        for (int k = 0; k < h1; ++k) s2 = fmaf(g.c2params[k * win + D + j], d1[k], s2);
        s = row_sel[lane] ? s2 : s;
      }
      const float act = row[D + j], v = row[y_off + A + j], zj = row[z_off + j];
      const float ls = v > 2.0f ? 2.0f : (v >= -20.0f ? v : -20.0f);
      const float sigma = exp_spec(ls);
      const float om = fmaf(-act, act, 1.0f);          // the forward's value
      const float r = om / (om + 1e-6f);
      const float du = ((w * (2.0f * act)) * r) + (s * om);
      const float dls = (du * (sigma * zj)) - w;
      row[y_off + j] = du;
      row[y_off + A + j] = (v >= -20.0f && v <= 2.0f) ? dls : 0.0f;   // torch's clamp: inclusive bounds, a NaN gives +0
    }
  }
  __syncthreads();
  learn_backward<true>(a, g.aparams, g.part + (size_t)blockIdx.x * a.P, img, pitch, rows, 0, y_off, tid, lane, wv);
}

// what the temperature's one thread reads of a call; log_alpha == nullptr: a fixed entropy coefficient
struct SacAlphaDev {
  float* log_alpha;
  float* m_v;
  float* hyper;
  float* stats;
  float target_entropy;
};
// One thread behind the finish kernel: the mean of logp (the blocks' partials ascending), the temperature's loss and (UPDATE) its Adam
// step with scale 1, *alpha = exp_spec(log_alpha), and *draws += 1 so that the next call draws fresh noise.
template <bool UPDATE>
__global__ void s2d_learn_sac_alpha_kernel(int64_t batch, int64_t blocks, const float* __restrict__ logp_part, SacAlphaDev t,
                                           float* __restrict__ alpha, uint64_t* __restrict__ draws) {
  if (t.log_alpha) {
    float ls = logp_part[0];
    for (int64_t b = 1; b < blocks; ++b) ls = ls + logp_part[b];
    const float mean = ls / (float)batch;
    const float la = *t.log_alpha;
    const float gr = -(mean + t.target_entropy);
    t.stats[0] = mean;
    t.stats[1] = la * gr;
    if (UPDATE) {
      const float lr = t.hyper[0], b1 = t.hyper[1], b2 = t.hyper[2], eps = t.hyper[3];
      const float b1t = t.hyper[5] * b1, b2t = t.hyper[6] * b2;
      t.hyper[5] = b1t;
      t.hyper[6] = b2t;
      const float omb1 = 1.0f - b1, omb2 = 1.0f - b2;
      const float bc2s = sqrtf(1.0f - b2t), step = lr / (1.0f - b1t);
      const float gp = gr * 1.0f;
      const float m0 = t.m_v[0];
      const float mn = m0 + (gp - m0) * omb1;
      const float vn = t.m_v[1] * b2 + (omb2 * gp) * gp;
      const float den = sqrtf(vn) / bc2s + eps;
      t.m_v[0] = mn;
      t.m_v[1] = vn;
      const float ln = la - step * (mn / den);
      const float an = exp_spec(ln);
      *t.log_alpha = ln;
      *alpha = an;
      t.stats[2] = an;
    }
  }
  if (UPDATE) *draws += 1;
}

// ------------------------------------------------------------------------------------------ PPO (s2d_learn_ppo)
// what the PPO kernels read of a call besides the two networks
struct PpoArgs {
  int head, A, normalize, pitch, P;          // 0 categorical / 1 Gaussian; outputs of pi; the pre-pass ran; the image's row; all parameters
  int64_t batch, src_rows, blocks, per_group;   // B, R, blocks of 64 rows, blocks a group
  const float* params;                       // [pi | vf | log_std]
  float* part;                               // [groups][P]
  float* stat_part;                          // [groups][kPpoStatWords]
  float* image;                              // [groups][64][pitch], if not in LDS
  const float* nrm;                          // mean, std of the pre-pass
  const float* hyper;
  const float* obs;
  const void* action;
  const float* logp_old;
  const float* adv;
  const float* ret;
  const int32_t* index;
  float* out_logp;
  float* out_value;
  int32_t* error;
};

// row b of the minibatch is row index[b] of the rollout arrays (b itself without an index); -1 if that is outside [0, R)
S2D_DEV int64_t ppo_source(const int32_t* __restrict__ index, int64_t b, int64_t src_rows) {
  const int64_t i = index ? (int64_t)index[b] : b;
  return i >= 0 && i < src_rows ? i : -1;
}

// The advantage's mean and unbiased standard deviation over the rows the minibatch names: per block of 64 rows s = +0, rows
// ascending s = s + adv; the blocks' sums added ascending; mean = S / B; then the same with s = fmaf(d, d, s), d = adv - mean;
// std = sqrt(S2 / (B - 1)).  One workgroup, a thread per block; bsum[blocks] is its scratch.
__global__ __launch_bounds__(kPpoNormThreads) void s2d_learn_ppo_norm_kernel(int64_t batch, int64_t src_rows, int64_t blocks,
                                                                            const float* __restrict__ adv, const int32_t* __restrict__ index,
                                                                            float* __restrict__ bsum, float* __restrict__ nrm) {
  __shared__ float sh_mean;
  float mean = 0.0f;
  for (int pass = 0; pass < 2; ++pass) {
    for (int64_t blk = threadIdx.x; blk < blocks; blk += kPpoNormThreads) {
      const int64_t row0 = blk * kLearnRows;
      const int rows = (int)(batch - row0 < kLearnRows ? batch - row0 : kLearnRows);
      float s = 0.0f;
      for (int r = 0; r < rows; ++r) {
        const int64_t i = ppo_source(index, row0 + r, src_rows);
        if (i < 0) continue;
        const float d = adv[i] - mean;
        s = pass ? fmaf(d, d, s) : s + adv[i];
      }
      bsum[blk] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      float t = bsum[0];
      for (int64_t blk = 1; blk < blocks; ++blk) t = t + bsum[blk];
      if (pass == 0) {
        sh_mean = t / (float)batch;
      } else {
        nrm[0] = mean;
        nrm[1] = sqrtf(t / (float)(batch - 1));
      }
    }
    __syncthreads();
    mean = sh_mean;
  }
}

// One workgroup per GROUP of consecutive blocks.  A row of a block's image holds both networks on one input:
// [x: 4 ceil(D / 4) | pi's y_1 .. y_L | logits or means: A | vf's y_1 .. y_L | v: 1 | (Gaussian) the rows' d log_std terms: A].
// Per block: the rows gathered by index, both forwards, the head (lane = row: logp, entropy, ratio, clipped surrogate, value error,
// the output deltas of both networks), the rows' five statistics, both backward passes continuing the group's dW / db chains.
template <bool LDS>
__global__ __launch_bounds__(kLearnThreads) void s2d_learn_ppo_block_kernel(LearnDev pi, LearnDev vf, PpoArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];   // [the rows' sources: 64 | their statistics: 5 x 64 | the image, if it lives here]
  int* const src = reinterpret_cast<int*>(smem);
  float* const rstat = smem + kLearnRows;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int pitch = a.pitch, A = a.A, D = pi.n_in;
  float* const img = LDS ? smem + kPpoRowWords * kLearnRows : a.image + (size_t)blockIdx.x * kLearnRows * pitch;
  float* const mine = a.part + (size_t)blockIdx.x * a.P;
  const float* const vparams = a.params + pi.P;
  const float* const log_std = vparams + vf.P;
  const float clip = a.hyper[7], vf_coef = a.hyper[8], ent_coef = a.hyper[9], fB = (float)a.batch;
  const int64_t blk0 = (int64_t)blockIdx.x * a.per_group;
  const int64_t blk1 = blk0 + a.per_group < a.blocks ? blk0 + a.per_group : a.blocks;
  float chain = 0.0f;                                  // threads 0 .. 4: the group's sum of statistic tid, rows ascending

  for (int64_t blk = blk0; blk < blk1; ++blk) {
    const bool first = blk == blk0;
    const int64_t row0 = blk * kLearnRows;
    const int rows = (int)(a.batch - row0 < kLearnRows ? a.batch - row0 : kLearnRows);
    if (tid < kLearnRows) {
      int64_t s = -1;
      if (tid < rows) {
        s = ppo_source(a.index, row0 + tid, a.src_rows);
        if (s < 0) atomicOr(a.error, 2);
      }
      src[tid] = (int)s;
    }
    __syncthreads();
    for (int idx = tid; idx < kLearnRows * pi.kp; idx += kLearnThreads) {
      const int r = idx / pi.kp, k = idx - r * pi.kp, s = src[r];
      img[r * pitch + k] = (s >= 0 && k < D) ? a.obs[(int64_t)s * D + k] : 0.0f;
    }
    __syncthreads();
    const int a_off = learn_forward(pi, a.params, img, pitch, 0, pi.kp, lane, wv);
    const int v_off = learn_forward(vf, vparams, img, pitch, 0, a_off + A, lane, wv);
    const int ls_off = v_off + 1;

    // ---- the head: lane = row
    if (tid < kLearnRows) {
      float* const row = img + tid * pitch;
      float* const y = row + a_off;
      const int s = src[tid];
      float st0 = 0.0f, st1 = 0.0f, st2 = 0.0f, st3 = 0.0f, st4 = 0.0f, o_logp = 0.0f, o_value = 0.0f;
      bool live = s >= 0;
      int ai = 0;
      float logp = 0.0f, H = 0.0f, m = 0.0f, S = 1.0f, logS = 0.0f;
      if (live && a.head == 0) {
        ai = static_cast<const int32_t*>(a.action)[s];
        if (ai < 0 || ai >= A) {
          atomicOr(a.error, 1);
          live = false;
        }
      }
      if (live && a.head == 0) {
        m = y[0];
        for (int j = 1; j < A; ++j) m = y[j] > m ? y[j] : m;
        S = exp_spec(y[0] - m);
        for (int j = 1; j < A; ++j) S += exp_spec(y[j] - m);
        logS = log_spec(S);
        logp = (y[ai] - m) - logS;
        float h = 0.0f;
        for (int j = 0; j < A; ++j) {
          const float p = exp_spec(y[j] - m) / S, lp = (y[j] - m) - logS;
          h = fmaf(p, lp, h);
        }
        H = -h;
      } else if (live) {
        const float* const act = static_cast<const float*>(a.action) + (int64_t)s * A;
        float hs = 0.0f;
        for (int j = 0; j < A; ++j) {
          const float ls = log_std[j], z = (act[j] - y[j]) / exp_spec(ls);
          const float term = fmaf(-0.5f * z, z, -ls) - 0.91893853f;
          logp = j ? logp + term : term;
          hs = j ? hs + ls : ls;
        }
        H = hs + (float)A * 1.4189385f;
      }
      if (live) {
        float adv = a.adv[s];
        if (a.normalize) adv = (adv - a.nrm[0]) / (a.nrm[1] + 1e-8f);
        const float d = logp - a.logp_old[s], r = exp_spec(d);
        const float lo = 1.0f - clip, hi = 1.0f + clip;
        const float rc = r < lo ? lo : (r > hi ? hi : r);
        const float s1 = r * adv, s2 = rc * adv;
        const float mn = (s1 < s2 || s1 != s1) ? s1 : s2;                 // torch.min: a NaN wins
        const bool clipped = (r > hi && adv > 0.0f) || (r < lo && adv < 0.0f);
        const float g = clipped ? 0.0f : -s1;                             // d(-min(s1, s2)) / d logp
        const float v = row[v_off], e = v - a.ret[s];
        st0 = -mn; st1 = e * e; st2 = H; st3 = (r - 1.0f) - d; st4 = fabsf(r - 1.0f) > clip ? 1.0f : 0.0f;
        o_logp = logp; o_value = v;
        row[v_off] = (vf_coef * (2.0f * e)) / fB;
        if (a.head == 0) {
          for (int j = 0; j < A; ++j) {
            const float p = exp_spec(y[j] - m) / S, lp = (y[j] - m) - logS;
            const float t1 = g * ((j == ai ? 1.0f : 0.0f) - p), t2 = (ent_coef * p) * (lp + H);
            y[j] = (t1 + t2) / fB;
          }
        } else {
          const float* const act = static_cast<const float*>(a.action) + (int64_t)s * A;
          for (int j = 0; j < A; ++j) {
            const float sg = exp_spec(log_std[j]), z = (act[j] - y[j]) / sg;
            y[j] = ((g * z) / sg) / fB;
            row[ls_off + j] = (g * (z * z - 1.0f)) / fB;
          }
        }
      } else {                                                            // past the batch, a bad index or a bad action: nothing
        for (int j = 0; j < A; ++j) y[j] = 0.0f;
        row[v_off] = 0.0f;
        if (a.head) for (int j = 0; j < A; ++j) row[ls_off + j] = 0.0f;
      }
      if (tid < rows) {
        if (a.out_logp) a.out_logp[row0 + tid] = o_logp;
        if (a.out_value) a.out_value[row0 + tid] = o_value;
      }
      rstat[0 * kLearnRows + tid] = st0; rstat[1 * kLearnRows + tid] = st1; rstat[2 * kLearnRows + tid] = st2;
      rstat[3 * kLearnRows + tid] = st3; rstat[4 * kLearnRows + tid] = st4;
    }
    __syncthreads();
    if (tid < 5)
      for (int r = 0; r < rows; ++r) chain = chain + rstat[tid * kLearnRows + r];

    // ---- backward: both networks, then log_std's terms like a bias
    learn_backward<true, true>(pi, a.params, mine, img, pitch, rows, 0, a_off, tid, lane, wv, first);
    learn_backward<true, true>(vf, vparams, mine + pi.P, img, pitch, rows, 0, v_off, tid, lane, wv, first);
    if (a.head && tid < A) {
      float* const out = mine + pi.P + vf.P + tid;
      float acc = first ? 0.0f : *out;
      for (int r = 0; r < rows; ++r) acc = fmaf(img[r * pitch + ls_off + tid], 1.0f, acc);
      *out = acc;
    }
    __syncthreads();                                   // the next block overwrites the sources, the statistics and the image
  }
  if (tid < 5) a.stat_part[(size_t)blockIdx.x * kPpoStatWords + tid] = chain;
}

// grad[p] = the blocks' partials added in ascending block order; chunk_ss[c] = fmaf(g, g, .) ascending over the chunk's words
// PPO (s2d_learn_ppo): the partials are the groups'; the words from ent_from on are log_std's, whose sum then loses ent_coef (hyper[9])
template <bool UPDATE, bool PPO = false>
__global__ __launch_bounds__(kLearnThreads) void s2d_learn_reduce_kernel(int P, int64_t blocks, const float* __restrict__ part,
                                                                         float* __restrict__ grad, float* __restrict__ chunk_ss,
                                                                         float* __restrict__ hyper, int ent_from) {
  __shared__ float g2[kLearnChunk];
  const int tid = threadIdx.x, p = blockIdx.x * kLearnChunk + tid;
  float s = 0.0f;
  if (p < P) {
    s = part[p];
    for (int64_t b = 1; b < blocks; ++b) s = s + part[(size_t)b * P + p];
    if (PPO && p >= ent_from) s = s - hyper[9];
    grad[p] = s;
  }
  g2[tid] = s;
  __syncthreads();
  if (tid == 0) {
    const int n = P - blockIdx.x * kLearnChunk < kLearnChunk ? P - blockIdx.x * kLearnChunk : kLearnChunk;
    float ss = 0.0f;
    for (int i = 0; i < n; ++i) ss = fmaf(g2[i], g2[i], ss);
    chunk_ss[blockIdx.x] = ss;
    if (UPDATE && blockIdx.x == 0) {                 // beta1^t, beta2^t: multiplied once per call, read by the finish kernel
      hyper[5] = hyper[5] * hyper[1];
      hyper[6] = hyper[6] * hyper[2];
    }
  }
}

// norm, clip scale and mean loss (workgroup 0 stores them; negate: minus the mean); UPDATE: Adam on the chunk's words with g' = g * scale
// PPO (s2d_learn_ppo): loss_part holds the groups' partials of five statistics, kPpoStatWords words a group, and stats has 8 words
template <bool UPDATE, bool PPO = false>
__global__ __launch_bounds__(kLearnThreads) void s2d_learn_finish_kernel(int P, int64_t batch, int64_t blocks, int chunks, bool negate,
                                                                         const float* __restrict__ chunk_ss,
                                                                         const float* __restrict__ loss_part, const float* __restrict__ grad,
                                                                         const float* __restrict__ hyper, float* __restrict__ stats,
                                                                         float* __restrict__ params, float* __restrict__ m,
                                                                         float* __restrict__ v) {
  __shared__ float sh_scale;
  const int tid = threadIdx.x;
  if (tid == 0) {
    float ss = chunk_ss[0];
    for (int c = 1; c < chunks; ++c) ss = ss + chunk_ss[c];
    const float norm = sqrtf(ss), mx = hyper[4];
    float scale = 1.0f;
    if (mx > 0.0f) {
      const float c = mx / (norm + 1e-6f);
      scale = c < 1.0f ? c : 1.0f;
    }
    sh_scale = scale;
    if (blockIdx.x == 0 && PPO) {
      float mean[5];                                   // policy loss, value loss, entropy, approx_kl, clip_fraction
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        float ls = loss_part[k];
        for (int64_t b = 1; b < blocks; ++b) ls = ls + loss_part[b * kPpoStatWords + k];
        mean[k] = ls / (float)batch;
        stats[3 + k] = mean[k];
      }
      stats[0] = (mean[0] + hyper[8] * mean[1]) - hyper[9] * mean[2];
      stats[1] = norm;
      stats[2] = scale;
    } else if (blockIdx.x == 0) {
      float ls = loss_part[0];
      for (int64_t b = 1; b < blocks; ++b) ls = ls + loss_part[b];
      stats[0] = (negate ? -ls : ls) / (float)batch;   // the actor's loss is -mean q
      stats[1] = norm;
      stats[2] = scale;
    }
  }
  if (!UPDATE) return;
  __syncthreads();
  const int p = blockIdx.x * kLearnChunk + tid;
  if (p >= P) return;
  const float scale = sh_scale;
  const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], b1t = hyper[5], b2t = hyper[6];
  const float omb1 = 1.0f - b1, omb2 = 1.0f - b2;
  const float bc2s = sqrtf(1.0f - b2t), step = lr / (1.0f - b1t);
  const float gp = grad[p] * scale;
  const float m0 = m[p];
  const float mn = m0 + (gp - m0) * omb1;
  const float vn = v[p] * b2 + (omb2 * gp) * gp;
  const float den = sqrtf(vn) / bc2s + eps;
  m[p] = mn;
  v[p] = vn;
  params[p] = params[p] - step * (mn / den);
}

// ------------------------------------------------------------------------------------------ host
namespace {
struct LearnLds {};   // the owner of the block kernels' dynamic-LDS slots (allow_lds_slot: 0 Q, 1 critic, 2 actor, 3 PPO, 4 SAC); fail, misaligned and launched are s2d_wide_host.h's

bool in_range(int64_t n) { return n >= 1 && n <= INT32_MAX; }   // a batch, a max_batch, the rows of a rollout
const char* const kBatchText = "batch must be in [1, 2^31 - 1]";
// "" if the shape is on the learner's grid, else the text naming the field
std::string shape_error(const S2DLearnNet* n) {
  if (n->n_in < 1 || n->n_in > 256) return "n_in must be in [1, 256]";
  if (n->n_hidden < 1 || n->n_hidden > kLearnMaxHidden) return "n_hidden must be in [1, 4]";
  for (int l = 0; l < 5; ++l) {
    const int w = n->hidden[l];
    if (l < n->n_hidden ? (w < 8 || w > 256 || w % 8) : w != 0) return "hidden widths must be multiples of 8 in [8, 256], and 0 past n_hidden";
  }
  if (n->n_out < 1 || n->n_out > 64) return "n_out must be in [1, 64]";
  if (n->activation < 0 || n->activation > 2) return "activation must be 0 (ReLU), 1 (Tanh) or 2 (Sigmoid)";
  return "";
}
// the first shape_error of the networks of a call (a NULL one is skipped), behind its name and ": "
struct NamedNet {
  const char* name;
  const S2DLearnNet* net;
};
std::string shapes_error(std::initializer_list<NamedNet> nets) {
  for (const NamedNet& n : nets) {
    const std::string bad = n.net ? shape_error(n.net) : "";
    if (!bad.empty()) return std::string(n.name) + ": " + bad;
  }
  return "";
}
LearnDev net_dev(const S2DLearnNet* n) {
  LearnDev d{};
  d.n_in = n->n_in; d.kp = (n->n_in + 3) / 4 * 4; d.n_hidden = n->n_hidden; d.act = n->activation; d.na = n->n_out;
  int win = n->n_in, row = d.kp;
  for (int l = 0; l <= n->n_hidden; ++l) {
    const int w = l < n->n_hidden ? n->hidden[l] : n->n_out;
    if (l < n->n_hidden) d.widths |= (uint32_t)(w / 8) << (8 * l);
    d.P += w * win + w;
    row += w;
    win = w;
  }
  d.pitch = row | 1;                                  // odd: lanes that read one column of 64 rows hit 64 different banks
  return d;
}
// the workspace in words: [partials: rows x P | chunk sums | loss partials: rows x loss_words | the learner's extra parts | images,
// if not in LDS], every part rounded up to 64 words.  P parameters are stepped; `rows` is the batch's blocks, or PPO's groups
struct LearnLayout {
  size_t part, chunk, loss, extra[2], image, words;
  bool lds;   // 64 rows of `pitch` words of the image and of the row_words beside it fit the LDS
};
size_t round64(size_t w) { return (w + 63) & ~(size_t)63; }
int64_t blocks_of(int64_t batch) { return (batch + kLearnRows - 1) / kLearnRows; }
LearnLayout layout(int P, int pitch, int row_words, size_t rows, size_t loss_words, size_t extra0 = 0, size_t extra1 = 0) {
  LearnLayout y{};
  const size_t chunks = ((size_t)P + kLearnChunk - 1) / kLearnChunk;
  y.lds = (size_t)kLearnRows * (pitch + row_words) * sizeof(float) <= kLdsMax;
  y.part = 0;
  y.chunk = round64(rows * P);
  y.loss = y.chunk + round64(chunks);
  y.extra[0] = y.loss + round64(rows * loss_words);
  y.extra[1] = y.extra[0] + round64(extra0);
  y.image = y.extra[1] + round64(extra1);
  y.words = y.image + (y.lds ? 0 : round64(rows * kLearnRows * pitch));
  return y;
}
// the Q, critic and DDPG actor steps: a loss word per block
LearnLayout block_layout(int P, int pitch, int64_t batch) { return layout(P, pitch, 1, (size_t)blocks_of(batch), 1); }
// the words of an image's row up to the last network's outputs: the padded input row, then each network's layers (none of a NULL one)
int row_words(int n_in, std::initializer_list<const S2DLearnNet*> nets) {
  int w = (n_in + 3) / 4 * 4;
  for (const S2DLearnNet* n : nets)
    for (int l = 0; n && l <= n->n_hidden; ++l) w += l < n->n_hidden ? n->hidden[l] : n->n_out;
  return w;
}
int pair_pitch(const S2DLearnNet* a, const S2DLearnNet* c) { return row_words(c->n_in, {a, c}) | 1; }
// "" if an actor with A actions and its critic(s) on n_in + A inputs, one output, are on the grid: s2d_learn_actor's pair (A = n_out,
// one critic) or s2d_learn_sac_actor's (sac: A = n_out / 2, critic2 may be NULL)
std::string pair_error(const S2DLearnNet* actor, bool sac, const S2DLearnNet* critic1, const S2DLearnNet* critic2) {
  const NamedNet critics[2] = {{sac ? "critic1" : "critic", critic1}, {"critic2", critic2}};
  const std::string bad = shapes_error({{"actor", actor}, critics[0], critics[1]});
  if (!bad.empty()) return bad;
  const int A = sac ? actor->n_out / 2 : actor->n_out;
  if (A < 1 || A > kLearnMaxAction || (sac && actor->n_out % 2))
    return sac ? "actor: n_out (means, then raw log-std) must be even and in [2, 16]" : "actor: n_out (the action width) must be in [1, 8]";
  if (actor->n_in > kLearnMaxObs) return "actor: n_in must be in [1, 248]";
  for (const NamedNet& c : critics)
    if (c.net && (c.net->n_in != actor->n_in + A || c.net->n_out != 1))
      return std::string(c.name) + ": n_in must be the actor's n_in + n_out" + (sac ? " / 2" : "") + ", its n_out 1";
  return "";
}
// what a call steps and how its refusals name it: filled from (S2DLearnNet, S2DLearnState) or from S2DLearnPPO
struct Stepped {
  const char *net, *state;   // "net: " / "actor: " and "state: ", or "" twice for PPO's one struct
  float *params, *m, *v, *grad, *hyper, *stats;
  int32_t* error;
  bool error_word;           // the call has one (the actor steps have not)
  void* workspace;
  size_t workspace_bytes;
};
Stepped stepped(const char* name, const S2DLearnNet* n, const S2DLearnState* st, bool error_word) {
  return Stepped{name, "state: ", n->params, st->m, st->v, st->grad, st->hyper, st->stats, st->error, error_word, n->workspace, n->workspace_bytes};
}
Stepped stepped(const S2DLearnPPO* q) {
  return Stepped{"", "", q->params, q->m, q->v, q->grad, q->hyper, q->stats, q->error, true, q->workspace, q->workspace_bytes};
}
// "" or the refusal of a parameter pointer, the stepped network's or a critic's that is only read (`net`: "critic: ", ...)
std::string params_error(const char* net, const float* params) {
  if (params && !misaligned(params, 16)) return "";
  return std::string(net) + "params must be a non-NULL, 16-byte aligned device pointer";
}
// the pointers of what is stepped; "" if acceptable
template <bool UPDATE>
std::string buffers_error(const Stepped& b) {
  const std::string bad = params_error(b.net, b.params);
  if (!bad.empty()) return bad;
  if (!b.workspace || misaligned(b.workspace, 256)) return std::string(b.net) + "workspace must be a non-NULL, 256-byte aligned device pointer";
  if (!b.grad || misaligned(b.grad, 16) || !b.hyper || misaligned(b.hyper, 4) || !b.stats || misaligned(b.stats, 4) ||
      (b.error_word && (!b.error || misaligned(b.error, 4))))
    return std::string(b.state) + "grad (16 bytes), hyper, stats" + (b.error_word ? " and error" : "") +
           " (4 bytes) must be non-NULL, aligned device pointers";
  if (UPDATE && (!b.m || !b.v || misaligned(b.m, 16) || misaligned(b.v, 16)))
    return std::string(b.state) + "m and v must be non-NULL, 16-byte aligned device pointers";
  return "";
}
// what the two actor steps check alike, in their order: the pair, the batch, the actor's buffers, the critics' parameters, obs
template <bool UPDATE>
std::string actor_error(const Stepped& b, int64_t batch, const S2DLearnNet* actor, bool sac, const S2DLearnNet* critic1,
                        const S2DLearnNet* critic2, const float* obs) {
  std::string err = pair_error(actor, sac, critic1, critic2);
  if (err.empty() && !in_range(batch)) err = kBatchText;
  if (err.empty()) err = buffers_error<UPDATE>(b);
  if (err.empty()) err = params_error(sac ? "critic1: " : "critic: ", critic1->params);
  if (err.empty() && critic2) err = params_error("critic2: ", critic2->params);
  if (err.empty() && (!obs || misaligned(obs, 4))) err = "obs must be a non-NULL, 4-byte aligned device pointer";
  return err;
}
// The device arrays of a call that must not overlap.  An array of group 0 must overlap nothing behind it in the list; arrays of
// another group are checked against those of group 0 alone.  NULL arrays are skipped
struct Spans {
  uintptr_t p[16];
  size_t bytes[16];
  int group[16], n = 0;
  Spans& add(const void* q, size_t b, int g = 0) {
    p[n] = reinterpret_cast<uintptr_t>(q), bytes[n] = b, group[n++] = g;
    return *this;
  }
  // what a call writes of the stepped network: params, grad, the workspace and (UPDATE) m and v
  template <bool UPDATE>
  Spans& add_stepped(const Stepped& b, int P, const LearnLayout& y, int g = 0) {
    const size_t pb = (size_t)P * sizeof(float);
    return add(b.params, pb, g).add(b.grad, pb, g).add(b.workspace, y.words * sizeof(float), g).add(UPDATE ? b.m : nullptr, pb, g)
        .add(UPDATE ? b.v : nullptr, pb, g);
  }
  // -1, or the group of the later array of the first pair that overlaps: the list's order, the earlier array counting first
  int clash() const {
    for (int i = 0; i < n; ++i)
      for (int j = i + 1; p[i] && group[i] == 0 && j < n; ++j)
        if (p[j] && p[i] < p[j] + bytes[j] && p[j] < p[i] + bytes[i]) return group[j];
    return -1;
  }
};
const char* const kActorOverlapText = "the actor's params, m, v, grad and workspace must not overlap one another or the critic's params";
// the workspace's size and the overlaps of what a call writes (and, for the actor steps, the first critic's parameters it reads)
template <bool UPDATE>
std::string layout_error(const Stepped& b, const LearnLayout& y, int P, int64_t batch, const char* bytes_fn, const float* read_only = nullptr,
                         size_t read_only_bytes = 0) {
  if (b.workspace_bytes < y.words * sizeof(float))
    return std::string(b.net) + "workspace_bytes is " + std::to_string(b.workspace_bytes) + ", a batch of " + std::to_string(batch) +
           " needs " + std::to_string(y.words * sizeof(float)) + " (" + bytes_fn + ": batch is above the workspace's max_batch)";
  if (Spans().add_stepped<UPDATE>(b, P, y).add(read_only, read_only_bytes).clash() >= 0)
    return read_only ? kActorOverlapText : "params, m, v, grad and the workspace must not overlap one another";
  return "";
}
// A learner's block kernel on `grid` workgroups: the instantiation for where the image lives, its dynamic LDS (64 rows of `beside`
// words, then the image if it lives there), above 48 KiB the attribute step under the kernel's `slot` of LearnLds, before() (what
// the call enqueues ahead of the kernel) and the launch.  S2D_OK, or S2D_EHIP with the text set and nothing enqueued
template <typename... Params, typename Before, typename... Args>
int launch_block(const std::string& who, void (*in_lds)(Params...), void (*in_workspace)(Params...), int slot, const LearnLayout& y, int beside,
                 int pitch, int64_t grid, hipStream_t s, Before before, Args... args) {
  const auto kb = y.lds ? in_lds : in_workspace;
  const size_t lds = (size_t)kLearnRows * ((y.lds ? pitch : 0) + beside) * sizeof(float);
  if (lds > 48 * 1024 && !allow_lds_slot<LearnLds>(reinterpret_cast<const void*>(kb), slot)) {
    s2d_internal_set_error((who + ": hipGetDevice or hipFuncSetAttribute failed").c_str());
    return S2D_EHIP;
  }
  before();
  hipLaunchKernelGGL(kb, dim3((unsigned)grid), dim3(kLearnThreads), lds, s, args...);
  return S2D_OK;
}
const auto nothing_before = [] {};
// what follows the block kernel: the reduction over the `rows` rows of partials, then norm, clip, stats and (UPDATE) Adam.
// PPO: the words from ent_from on are log_std's, and the loss partials are the groups' statistics; else ent_from = P
template <bool UPDATE, bool PPO = false>
void reduce_and_finish(const Stepped& b, int P, int64_t batch, int64_t rows, int ent_from, bool negate, const LearnLayout& y, hipStream_t s) {
  float* const ws = static_cast<float*>(b.workspace);
  const int chunks = (P + kLearnChunk - 1) / kLearnChunk;
  hipLaunchKernelGGL((s2d_learn_reduce_kernel<UPDATE, PPO>), dim3((unsigned)chunks), dim3(kLearnThreads), 0, s, P, rows, ws + y.part, b.grad,
                     ws + y.chunk, b.hyper, ent_from);
  hipLaunchKernelGGL((s2d_learn_finish_kernel<UPDATE, PPO>), dim3(UPDATE ? (unsigned)chunks : 1u), dim3(kLearnThreads), 0, s, P, batch, rows,
                     chunks, negate, ws + y.chunk, ws + y.loss, b.grad, b.hyper, b.stats, b.params, b.m, b.v);
}

// s2d_learn_q[_grad] (CRITIC = false: action is int32 [B]) and s2d_learn_critic[_grad] (CRITIC = true: action is float [B][A])
template <bool UPDATE, bool CRITIC>
int learn(const std::string& who, int64_t batch, const S2DLearnNet* net, const S2DLearnState* st, const float* obs, int A, const void* action,
          const float* target, const float* weight, float* out_td_abs, float* out_q, void* stream) {
  if (!net || !st) return fail(who, "net and state must be non-NULL");
  std::string err = shapes_error({{"net", net}});
  if (!err.empty()) return fail(who, err);
  if (CRITIC) {
    if (A < 1 || A > kLearnMaxAction) return fail(who, "action_dim must be in [1, 8]");
    if (net->n_out != 1) return fail(who, "net: n_out must be 1 (a critic)");
    if (net->n_in - A < 1 || net->n_in - A > kLearnMaxObs)
      return fail(who, "net: n_in must be obs_dim + action_dim with obs_dim in [1, 248]");
    if (st->loss_kind < S2D_LEARN_MSE || st->loss_kind > S2D_LEARN_SQUARE)
      return fail(who, "state: loss_kind must be 0 (MSE), 1 (Huber) or 2 (square)");
  } else if (st->loss_kind != S2D_LEARN_MSE && st->loss_kind != S2D_LEARN_HUBER) {
    return fail(who, "state: loss_kind must be 0 (MSE) or 1 (Huber)");
  }
  if (!in_range(batch)) return fail(who, kBatchText);
  const Stepped b = stepped("net: ", net, st, true);
  err = buffers_error<UPDATE>(b);
  if (!err.empty()) return fail(who, err);
  if (!obs || !action || !target || misaligned(obs, 4) || misaligned(action, 4) || misaligned(target, 4))
    return fail(who, "obs, action and target must be non-NULL, 4-byte aligned device pointers");
  if (misaligned(weight, 4) || misaligned(out_td_abs, 4) || misaligned(out_q, 4))
    return fail(who, "weight, out_td_abs and out_q must be 4-byte aligned device pointers (or NULL)");
  const LearnDev d = net_dev(net);
  const LearnLayout y = block_layout(d.P, d.pitch, batch);
  err = layout_error<UPDATE>(b, y, d.P, batch, "s2d_learn_workspace_bytes");
  if (!err.empty()) return fail(who, err);
  float* const ws = static_cast<float*>(net->workspace);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t blocks = blocks_of(batch);
  const int rc =
      CRITIC ? launch_block(who, s2d_learn_critic_kernel<true>, s2d_learn_critic_kernel<false>, 1, y, 1, d.pitch, blocks, s, nothing_before, d,
                            batch, (int)st->loss_kind, net->params, ws + y.part, ws + y.loss, ws + y.image, obs, net->n_in - A,
                            static_cast<const float*>(action), target, weight, out_td_abs, out_q)
             : launch_block(who, s2d_learn_block_kernel<true>, s2d_learn_block_kernel<false>, 0, y, 1, d.pitch, blocks, s, nothing_before, d,
                            batch, (int)st->loss_kind, net->params, ws + y.part, ws + y.loss, ws + y.image, obs,
                            static_cast<const int32_t*>(action), target, weight, out_td_abs, out_q, st->error);
  if (rc != S2D_OK) return rc;
  reduce_and_finish<UPDATE>(b, d.P, batch, blocks, d.P, false, y, s);
  return launched(who);
}

template <bool UPDATE>
int learn_actor(const std::string& who, int64_t batch, const S2DLearnNet* actor, const S2DLearnState* st, const S2DLearnNet* critic,
                const float* obs, float* out_action, float* out_q, void* stream) {
  if (!actor || !st || !critic) return fail(who, "actor, state and critic must be non-NULL");
  const Stepped b = stepped("actor: ", actor, st, false);
  std::string err = actor_error<UPDATE>(b, batch, actor, false, critic, nullptr, obs);
  if (!err.empty()) return fail(who, err);
  if (misaligned(out_action, 4) || misaligned(out_q, 4)) return fail(who, "out_action and out_q must be 4-byte aligned device pointers (or NULL)");
  const LearnDev a = net_dev(actor), c = net_dev(critic);
  const int pitch = pair_pitch(actor, critic);
  const LearnLayout y = block_layout(a.P, pitch, batch);
  err = layout_error<UPDATE>(b, y, a.P, batch, "s2d_learn_actor_workspace_bytes", critic->params, (size_t)c.P * sizeof(float));
  if (!err.empty()) return fail(who, err);
  float* const ws = static_cast<float*>(actor->workspace);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t blocks = blocks_of(batch);
  if (const int rc = launch_block(who, s2d_learn_actor_kernel<true>, s2d_learn_actor_kernel<false>, 2, y, 1, pitch, blocks, s, nothing_before, a, c,
                                  pitch, batch, actor->params, critic->params, ws + y.part, ws + y.loss, ws + y.image, obs, out_action, out_q))
    return rc;
  reduce_and_finish<UPDATE>(b, a.P, batch, blocks, a.P, true, y, s);
  return launched(who);
}
// ---- SAC
// the column of the head's z words, behind every network's layers; the row has A more words
int sac_z_off(const S2DLearnNet* a, const S2DLearnNet* c1, const S2DLearnNet* c2) { return row_words(c1->n_in, {a, c1, c2}); }
int sac_pitch(const S2DLearnNet* a, const S2DLearnNet* c1, const S2DLearnNet* c2) { return (sac_z_off(a, c1, c2) + a->n_out / 2) | 1; }
// the actor's workspace: the actor step's, with the blocks' logp partials (extra[0]) behind their loss partials
LearnLayout sac_layout(int P, int pitch, int64_t batch) {
  const size_t blocks = (size_t)blocks_of(batch);
  return layout(P, pitch, kSacRowWords, blocks, 1, blocks);
}

template <bool UPDATE>
int learn_sac(const std::string& who, int64_t batch, const S2DLearnNet* actor, const S2DLearnState* st, const S2DLearnNet* critic1,
              const S2DLearnNet* critic2, const float* obs, float* alpha, const S2DLearnSacAlpha* as, uint64_t* draws, uint64_t seed,
              float* out_action, float* out_logp, float* out_q, void* stream) {
  if (!actor || !st || !critic1) return fail(who, "actor, state and critic1 must be non-NULL");
  const Stepped b = stepped("actor: ", actor, st, false);
  std::string err = actor_error<UPDATE>(b, batch, actor, true, critic1, critic2, obs);
  if (!err.empty()) return fail(who, err);
  if (!alpha || misaligned(alpha, 4)) return fail(who, "alpha must be a non-NULL, 4-byte aligned device pointer");
  if (!draws || misaligned(draws, 8)) return fail(who, "draws must be a non-NULL, 8-byte aligned device pointer");
  if (as && (!as->log_alpha || !as->m_v || !as->hyper || !as->stats || misaligned(as->log_alpha, 4) || misaligned(as->m_v, 4) ||
             misaligned(as->hyper, 4) || misaligned(as->stats, 4)))
    return fail(who, "alpha_state: log_alpha, m_v, hyper and stats must be non-NULL, 4-byte aligned device pointers");
  if (misaligned(out_action, 4) || misaligned(out_logp, 4) || misaligned(out_q, 4))
    return fail(who, "out_action, out_logp and out_q must be 4-byte aligned device pointers (or NULL)");
  const LearnDev a = net_dev(actor), c1 = net_dev(critic1), c2 = critic2 ? net_dev(critic2) : LearnDev{};
  const int A = actor->n_out / 2, pitch = sac_pitch(actor, critic1, critic2);
  const LearnLayout y = sac_layout(a.P, pitch, batch);
  err = layout_error<UPDATE>(b, y, a.P, batch, "s2d_learn_sac_workspace_bytes", critic1->params, (size_t)c1.P * sizeof(float));
  if (!err.empty()) return fail(who, err);
  {
    // the call's new arrays (group 0) against one another, then against what the call writes, the critics' parameters and the
    // outputs (group 1); last the second critic's parameters against what the call writes, as layout_error did the first's
    const size_t fb = sizeof(float), B = (size_t)batch, c2b = (size_t)c2.P * fb;
    const float* const c2p = critic2 ? critic2->params : nullptr;
    Spans z;
    z.add(alpha, fb).add(draws, sizeof(uint64_t)).add(as ? as->log_alpha : nullptr, fb).add(as ? as->m_v : nullptr, 2 * fb)
        .add(as ? as->hyper : nullptr, 7 * fb).add(as ? as->stats : nullptr, 3 * fb);
    z.add_stepped<UPDATE>(b, a.P, y, 1).add(critic1->params, (size_t)c1.P * fb, 1).add(c2p, c2b, 1).add(out_action, B * A * fb, 1)
        .add(out_logp, B * fb, 1).add(out_q, B * fb, 1);
    const int group = z.clash();
    if (group == 0) return fail(who, "alpha, draws and alpha_state's log_alpha, m_v, hyper and stats must not overlap one another");
    if (group == 1)
      return fail(who, "alpha, draws and alpha_state's arrays must not overlap the actor's params, m, v, grad or workspace, a critic's "
                       "params or an output");
    if (Spans().add(c2p, c2b).add_stepped<UPDATE>(b, a.P, y, 1).clash() >= 0) return fail(who, kActorOverlapText);
  }
  float* const ws = static_cast<float*>(actor->workspace);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t blocks = blocks_of(batch);
  SacArgs g{};
  g.pitch = pitch; g.z_off = sac_z_off(actor, critic1, critic2); g.twin = critic2 ? 1 : 0; g.batch = batch;
  g.aparams = actor->params; g.c1params = critic1->params; g.c2params = critic2 ? critic2->params : nullptr;
  g.part = ws + y.part; g.loss_part = ws + y.loss; g.logp_part = ws + y.extra[0]; g.image = ws + y.image;
  g.obs = obs; g.alpha = alpha; g.draws = draws; g.seed_lo = (uint32_t)seed; g.seed_hi = (uint32_t)(seed >> 32);
  g.out_action = out_action; g.out_logp = out_logp; g.out_q = out_q;
  if (const int rc = launch_block(who, s2d_learn_sac_kernel<true>, s2d_learn_sac_kernel<false>, 4, y, kSacRowWords, pitch, blocks, s,
                                  nothing_before, a, c1, c2, g))
    return rc;
  reduce_and_finish<UPDATE>(b, a.P, batch, blocks, a.P, false, y, s);
  if (UPDATE || as) {
    SacAlphaDev t{};
    if (as) {
      t.log_alpha = as->log_alpha; t.m_v = as->m_v; t.hyper = as->hyper; t.stats = as->stats; t.target_entropy = as->target_entropy;
    }
    hipLaunchKernelGGL(s2d_learn_sac_alpha_kernel<UPDATE>, dim3(1), dim3(1), 0, s, batch, blocks, ws + y.extra[0], t, alpha, draws);
  }
  return launched(who);
}
// ---- PPO
// "" if the pair of networks and the head are on the grid of s2d_learn_ppo
std::string ppo_error(const S2DLearnNet* pi, const S2DLearnNet* vf, int head) {
  const std::string bad = shapes_error({{"pi", pi}, {"vf", vf}});
  if (!bad.empty()) return bad;
  if (vf->n_out != 1 || vf->n_in != pi->n_in) return "vf: n_in must be pi's n_in, its n_out 1";
  if (head != S2D_LEARN_PPO_CATEGORICAL && head != S2D_LEARN_PPO_GAUSSIAN) return "head must be 0 (categorical) or 1 (diagonal Gaussian)";
  if (head == S2D_LEARN_PPO_GAUSSIAN && pi->n_out > kLearnMaxAction) return "pi: n_out (the action width) must be in [1, 8] with the Gaussian head";
  return "";
}
int ppo_pitch(const S2DLearnNet* pi, const S2DLearnNet* vf, int head) { return (row_words(pi->n_in, {pi, vf}) + (head ? pi->n_out : 0)) | 1; }
// the workspace: g = min(blocks, 256) rows of partials -- at least the groups of every smaller batch -- with the groups' statistics
// (8 words each) as their loss partials, then [mean, std] (extra[0]) and the pre-pass's block sums (extra[1])
LearnLayout ppo_layout(int P, int pitch, int64_t batch) {
  const size_t blocks = (size_t)blocks_of(batch), most = kPpoMaxGroups;
  return layout(P, pitch, kPpoRowWords, blocks < most ? blocks : most, kPpoStatWords, 2, blocks);
}

template <bool UPDATE>
int learn_ppo(const std::string& who, const S2DLearnPPO* q, const S2DLearnPPOBatch* b, void* stream) {
  if (!q || !b) return fail(who, "learner and batch must be non-NULL");
  std::string err = ppo_error(&q->pi, &q->vf, q->head);
  if (!err.empty()) return fail(who, err);
  const int64_t B = b->batch, R = b->rows;
  if (!in_range(R)) return fail(who, "rows must be in [1, 2^31 - 1]");
  if (!in_range(B)) return fail(who, kBatchText);
  if (!b->index && B > R) return fail(who, "batch must be at most rows where index is NULL");
  const Stepped st = stepped(q);
  err = buffers_error<UPDATE>(st);
  if (!err.empty()) return fail(who, err);
  if (!b->obs || !b->action || !b->logp_old || !b->advantage || !b->ret || misaligned(b->obs, 4) || misaligned(b->action, 4) ||
      misaligned(b->logp_old, 4) || misaligned(b->advantage, 4) || misaligned(b->ret, 4))
    return fail(who, "obs, action, logp_old, advantage and ret must be non-NULL, 4-byte aligned device pointers");
  if (misaligned(b->index, 4) || misaligned(b->out_logp, 4) || misaligned(b->out_value, 4))
    return fail(who, "index, out_logp and out_value must be 4-byte aligned device pointers (or NULL)");
  const LearnDev pi = net_dev(&q->pi), vf = net_dev(&q->vf);
  const int A = q->pi.n_out, P = pi.P + vf.P + (q->head ? A : 0), pitch = ppo_pitch(&q->pi, &q->vf, q->head);
  const LearnLayout y = ppo_layout(P, pitch, B);
  err = layout_error<UPDATE>(st, y, P, B, "s2d_learn_ppo_workspace_bytes");
  if (!err.empty()) return fail(who, err);
  // one workgroup per group of per_group consecutive blocks
  const int64_t blocks = blocks_of(B), per_group = (blocks + kPpoMaxGroups - 1) / kPpoMaxGroups, groups = (blocks + per_group - 1) / per_group;
  float* const ws = static_cast<float*>(q->workspace);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const bool normalize = q->normalize_advantage && B > 1;
  PpoArgs a{};
  a.head = q->head; a.A = A; a.normalize = normalize; a.pitch = pitch; a.P = P;
  a.batch = B; a.src_rows = R; a.blocks = blocks; a.per_group = per_group;
  a.params = q->params; a.part = ws + y.part; a.stat_part = ws + y.loss; a.image = ws + y.image; a.nrm = ws + y.extra[0]; a.hyper = q->hyper;
  a.obs = b->obs; a.action = b->action; a.logp_old = b->logp_old; a.adv = b->advantage; a.ret = b->ret; a.index = b->index;
  a.out_logp = b->out_logp; a.out_value = b->out_value; a.error = q->error;
  const auto advantage_pre_pass = [&] {
    if (normalize)
      hipLaunchKernelGGL(s2d_learn_ppo_norm_kernel, dim3(1), dim3(kPpoNormThreads), 0, s, B, R, blocks, b->advantage, b->index, ws + y.extra[1],
                         ws + y.extra[0]);
  };
  if (const int rc = launch_block(who, s2d_learn_ppo_block_kernel<true>, s2d_learn_ppo_block_kernel<false>, 3, y, kPpoRowWords, pitch, groups, s,
                                  advantage_pre_pass, pi, vf, a))
    return rc;
  reduce_and_finish<UPDATE, true>(st, P, B, groups, pi.P + vf.P, false, y, s);
  return launched(who);
}
}  // namespace

S2D_API size_t s2d_learn_ppo_workspace_bytes(const S2DLearnNet* pi_shape, const S2DLearnNet* vf_shape, int32_t head, int64_t max_batch) {
  if (!pi_shape || !vf_shape || !ppo_error(pi_shape, vf_shape, head).empty() || !in_range(max_batch)) return 0;
  const int P = net_dev(pi_shape).P + net_dev(vf_shape).P + (head ? pi_shape->n_out : 0);
  return ppo_layout(P, ppo_pitch(pi_shape, vf_shape, head), max_batch).words * sizeof(float);
}

S2D_API int s2d_learn_ppo(const S2DLearnPPO* learner, const S2DLearnPPOBatch* batch, void* stream) {
  return learn_ppo<true>("s2d_learn_ppo", learner, batch, stream);
}

S2D_API int s2d_learn_ppo_grad(const S2DLearnPPO* learner, const S2DLearnPPOBatch* batch, void* stream) {
  return learn_ppo<false>("s2d_learn_ppo_grad", learner, batch, stream);
}

S2D_API size_t s2d_learn_workspace_bytes(const S2DLearnNet* shape, int64_t max_batch) {
  if (!shape || !shape_error(shape).empty() || !in_range(max_batch)) return 0;
  const LearnDev d = net_dev(shape);
  return block_layout(d.P, d.pitch, max_batch).words * sizeof(float);
}

S2D_API size_t s2d_learn_actor_workspace_bytes(const S2DLearnNet* actor_shape, const S2DLearnNet* critic_shape, int64_t max_batch) {
  if (!actor_shape || !critic_shape || !pair_error(actor_shape, false, critic_shape, nullptr).empty() || !in_range(max_batch)) return 0;
  const LearnDev a = net_dev(actor_shape);
  return block_layout(a.P, pair_pitch(actor_shape, critic_shape), max_batch).words * sizeof(float);
}

S2D_API int s2d_learn_q(int64_t batch, const S2DLearnNet* net, const S2DLearnState* state, const float* obs, const int32_t* action,
                        const float* target, const float* weight, float* out_td_abs, float* out_q, void* stream) {
  return learn<true, false>("s2d_learn_q", batch, net, state, obs, 0, action, target, weight, out_td_abs, out_q, stream);
}

S2D_API int s2d_learn_q_grad(int64_t batch, const S2DLearnNet* net, const S2DLearnState* state, const float* obs, const int32_t* action,
                             const float* target, const float* weight, float* out_td_abs, float* out_q, void* stream) {
  return learn<false, false>("s2d_learn_q_grad", batch, net, state, obs, 0, action, target, weight, out_td_abs, out_q, stream);
}

S2D_API int s2d_learn_critic(int64_t batch, const S2DLearnNet* net, const S2DLearnState* state, const float* obs, int32_t action_dim,
                             const float* action, const float* target, const float* weight, float* out_td_abs, float* out_q, void* stream) {
  return learn<true, true>("s2d_learn_critic", batch, net, state, obs, action_dim, action, target, weight, out_td_abs, out_q, stream);
}

S2D_API int s2d_learn_critic_grad(int64_t batch, const S2DLearnNet* net, const S2DLearnState* state, const float* obs, int32_t action_dim,
                                  const float* action, const float* target, const float* weight, float* out_td_abs, float* out_q,
                                  void* stream) {
  return learn<false, true>("s2d_learn_critic_grad", batch, net, state, obs, action_dim, action, target, weight, out_td_abs, out_q, stream);
}

S2D_API int s2d_learn_actor(int64_t batch, const S2DLearnNet* actor, const S2DLearnState* actor_state, const S2DLearnNet* critic,
                            const float* obs, float* out_action, float* out_q, void* stream) {
  return learn_actor<true>("s2d_learn_actor", batch, actor, actor_state, critic, obs, out_action, out_q, stream);
}

S2D_API int s2d_learn_actor_grad(int64_t batch, const S2DLearnNet* actor, const S2DLearnState* actor_state, const S2DLearnNet* critic,
                                 const float* obs, float* out_action, float* out_q, void* stream) {
  return learn_actor<false>("s2d_learn_actor_grad", batch, actor, actor_state, critic, obs, out_action, out_q, stream);
}

S2D_API size_t s2d_learn_sac_workspace_bytes(const S2DLearnNet* actor_shape, const S2DLearnNet* critic1_shape, const S2DLearnNet* critic2_shape,
                                             int64_t max_batch) {
  if (!actor_shape || !critic1_shape || !pair_error(actor_shape, true, critic1_shape, critic2_shape).empty() || !in_range(max_batch)) return 0;
  return sac_layout(net_dev(actor_shape).P, sac_pitch(actor_shape, critic1_shape, critic2_shape), max_batch).words * sizeof(float);
}

S2D_API int s2d_learn_sac_actor(int64_t batch, const S2DLearnNet* actor, const S2DLearnState* actor_state, const S2DLearnNet* critic1,
                                const S2DLearnNet* critic2, const float* obs, float* alpha, const S2DLearnSacAlpha* alpha_state,
                                uint64_t* draws, uint64_t seed, float* out_action, float* out_logp, float* out_q, void* stream) {
  return learn_sac<true>("s2d_learn_sac_actor", batch, actor, actor_state, critic1, critic2, obs, alpha, alpha_state, draws, seed, out_action,
                         out_logp, out_q, stream);
}

S2D_API int s2d_learn_sac_actor_grad(int64_t batch, const S2DLearnNet* actor, const S2DLearnState* actor_state, const S2DLearnNet* critic1,
                                     const S2DLearnNet* critic2, const float* obs, float* alpha, const S2DLearnSacAlpha* alpha_state,
                                     uint64_t* draws, uint64_t seed, float* out_action, float* out_logp, float* out_q, void* stream) {
  return learn_sac<false>("s2d_learn_sac_actor_grad", batch, actor, actor_state, critic1, critic2, obs, alpha, alpha_state, draws, seed,
                          out_action, out_logp, out_q, stream);
}
