// s2d_wide_pack.hip -- the pack kernel of the streamed-weight MLP (s2d_wide_net.h) and what s2d_wide_host.h declares: the one
// host path of the network's users (s2d_wide_actor.hip, s2d_gtc_actor.hip, s2d_td.hip) for the shape, the fragment count, the
// workspace, the network's text and the waves,tiles override.  Only host functions are called across units.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>

#include "s2d_wide_host.h"

S2D_DEV int pack_width(const WidePackArgs& d, int l) { return 4 * (int)((d.widths >> (7 * l)) & 127u); }

// The caller's parameters (nn.Sequential order: W_1 [h_1][n_in], b_1, ..., W_L [h_L][h_(L-1)], b_L, W_out [A][h_L], b_out) into the
// workspace in fragment order (fragment (jt, s) = 64 words, word l = W[16 jt + (l & 15)][4 s + (l >> 4)]; by layer, then jt, then
// s), then the biases, every layer's padded with zeros to its tiles' 16 rows: one word per thread.  Rows past a layer's width and
// layer 1's k >= n_in are zero.  Enqueued ahead of every launch that reads the workspace.
__global__ __launch_bounds__(256) void s2d_wide_pack_kernel(WidePackArgs d, const float* __restrict__ params, float* __restrict__ ws) {
  const int L = d.n_hidden;
  const int nw = d.nfrag * kWave;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nw + d.nbias) return;
  if (idx < nw) {
    const int f = idx / kWave, lw = idx & (kWave - 1);
    const int row = lw & 15, kk = lw >> 4;
    // the layer of fragment f: its first fragment, widths in and out, k-steps and the offset of its W in params
    int f0 = 0, win = d.n_in, wout = pack_width(d, 0), ks = (d.n_in + 3) >> 2, ow = 0;
#pragma unroll
    for (int l = 1; l <= kWideMaxHidden; ++l) {
      const int next = f0 + ((wout + 15) >> 4) * ks;         // the first fragment of the layer after this one
      if (l <= L && f >= next) {
        ow += wout * win + wout;
        f0 = next;
        win = wout;
        wout = l < L ? pack_width(d, l) : d.na;
        ks = win >> 2;
      }
    }
    const int r = f - f0, jt = r / ks, s = r - jt * ks, j = 16 * jt + row, k = 4 * s + kk;
    ws[idx] = (j < wout && k < win) ? params[ow + j * win + k] : 0.0f;
  } else {
    const int bi = idx - nw;
    int b0 = 0, win = d.n_in, wout = pack_width(d, 0), ob = wout * win;   // ob: the offset of the layer's bias in params
#pragma unroll
    for (int l = 1; l <= kWideMaxHidden; ++l) {
      const int pad = (wout + 15) & ~15;
      if (l <= L && bi >= b0 + pad) {
        b0 += pad;
        win = wout;
        wout = l < L ? pack_width(d, l) : d.na;
        ob += win + wout * win;
      }
    }
    const int j = bi - b0;
    ws[idx] = j < wout ? params[ob + j] : 0.0f;
  }
}

void s2d_internal_wide_pack(const WidePackArgs& a, const float* params, void* workspace, hipStream_t stream) {
  const int words = a.nfrag * kWave + a.nbias;
  hipLaunchKernelGGL(s2d_wide_pack_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, a, params,
                     static_cast<float*>(workspace));
}

int s2d_internal_wide_shape(const std::string& prefix, const int32_t* n_in, int n_hidden, const int32_t* hidden, int activation, int n_out) {
  if (n_in && (*n_in < 1 || *n_in > 256)) return fail(prefix, "n_in must be in [1, 256]");
  if (n_hidden < 1 || n_hidden > kWideMaxHidden) return fail(prefix, "n_hidden must be in [1, 5]");
  if (!wide_shape_ok(n_hidden, hidden)) return fail(prefix, "hidden widths must be multiples of 4 in [8, 400], and 0 past n_hidden");
  if (activation < 0 || activation > 2) return fail(prefix, "activation must be 0 (ReLU), 1 (Tanh) or 2 (Sigmoid)");
  if (n_out < 1 || n_out > 64) return fail(prefix, "n_out must be in [1, 64]");
  return S2D_OK;
}

WideCounts s2d_internal_wide_counts(int n_in, int n_hidden, const int32_t* hidden, int n_out) {
  WideCounts c{};
  c.na16 = (n_out + 15) / 16 * 16;
  int ksteps = (n_in + 3) / 4;
  for (int l = 0; l < n_hidden; ++l) {
    const int w = hidden[l], m16 = (w + 15) / 16;
    c.widths |= (uint64_t)(w / 4) << (7 * l);
    c.nfrag += m16 * ksteps;
    c.nbias += 16 * m16;
    if (16 * m16 > c.wmax) c.wmax = 16 * m16;
    ksteps = w / 4;
  }
  c.nfrag += (c.na16 / 16) * ksteps;
  c.nbias += c.na16;
  return c;
}

std::string s2d_internal_wide_text(int n_in, int n_hidden, const int32_t* hidden, int n_out) {
  std::string s = std::to_string(n_in);
  for (int l = 0; l < n_hidden; ++l) s += "-" + std::to_string(hidden[l]);
  return s + "-" + std::to_string(n_out);
}

int s2d_internal_wide_workspace(const std::string& prefix, const void* workspace, size_t workspace_bytes, size_t need, const std::string& text,
                                const char* bytes_fn) {
  if (!workspace || misaligned(workspace, 256)) return fail(prefix, "workspace must be a non-NULL, 256-byte aligned device pointer");
  if (workspace_bytes < need)
    return fail(prefix, "workspace_bytes is " + std::to_string(workspace_bytes) + ", the network " + text + " needs " + std::to_string(need) +
                            " (" + bytes_fn + ")");
  return S2D_OK;
}

WidePlanOverride s2d_internal_plan_override(const char* var) {
  WidePlanOverride o{0, 0, true, std::string(var) + "="};
  const char* const env = std::getenv(var);
  if (!env) return o;
  o.text += env;
  if (*env && std::sscanf(env, "%d,%d", &o.waves, &o.tiles) != 2) o.waves = o.tiles = -1;
  const auto one_of = [](int v) { return v == 4 || v == 2 || v == 1; };
  o.ok = (!o.waves || one_of(o.waves)) && (!o.tiles || one_of(o.tiles));
  return o;
}
