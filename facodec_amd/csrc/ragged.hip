// Batches of clips with different lengths: the per-row pieces of the offline path.  The clips of a batch are
// right-padded with zeros to one length T; `lens` (B,) int32 holds every row's own length in SAMPLES and stays on the device --
// no launch here needs a host copy of it.  A length is clamped to [0, T] before it is used as an index, so a wrong value can
// zero the wrong columns but can never address memory outside its row.  (fac_edge_tail, DESIGN.md 23, counts in FRAMES times a
// per-tensor multiplier instead; the same clamp.)
#include "common.h"
#include <limits.h>

namespace fac {

__device__ __forceinline__ int row_len(const int* __restrict__ lens, int b, int T) {
  const int L = lens[b];
  return L < 0 ? 0 : (L > T ? T : L);
}

// stft_frames_kernel (misc.hip) with the reflection at the end of the CLIP instead of the end of the tensor: row b is framed as if
// it were lens[b] samples long (the same gather, hence the same bits as fac_stft_frames on wave[b, :lens[b]]) and has
// lens[b] / hop frames; the frame columns behind them are written as zeros.  Grid (chunks of n_win * n_frames, B): 32-bit indices.
__global__ __launch_bounds__(256) void stft_frames_ragged_kernel(const float* __restrict__ wave, const int* __restrict__ lens,
                                                                 float* __restrict__ frames, int T, int n_win, int n_frames,
                                                                 int hop, int pad, int n_off) {
  const int b = blockIdx.y;
  const int L = row_len(lens, b, T);
  const int nf = min(L / hop, n_frames);
  const int per_b = n_win * n_frames;
  const float* w = wave + (long long)b * T;
  float* fr = frames + (long long)b * per_b;
  for (int r = blockIdx.x * 256 + threadIdx.x; r < per_b; r += gridDim.x * 256) {
    const int nn = r / n_frames;
    const int f = r - nn * n_frames;
    float v = 0.f;
    if (f < nf) {
      int t = f * hop + nn + n_off - pad;
      if (t < 0) t = -t;
      if (t >= L) t = 2 * (L - 1) - t;
      if (t >= 0 && t < L) v = w[t];
    }
    fr[r] = v;
  }
}

// x (rows, Tw) 32-bit words, rows = B * C, Tw = T * wpe words per row (wpe = 1: fp32, 2: int64): zeroes the words from
// (lens[b] / unit) * wpe on.  Store-only traffic: the kept columns are neither read nor written.  A row's tail is a scalar
// head up to the next 16-byte boundary, 16-byte stores, and a scalar rest.  `tpr` = 1 << tpr_log2 threads share a row and a
// workgroup holds 256 / tpr rows, so frame-rate tensors (rows of a few dozen columns) keep their lanes busy as well as the
// decoder's sample-rate output (a few rows of 10^5 columns, split over blockIdx.x).
__global__ __launch_bounds__(256) void mask_tail_kernel(float* __restrict__ x, const int* __restrict__ lens, int rows, int C,
                                                        int T, int wpe, int unit, int tpr_log2) {
  const int tpr = 1 << tpr_log2;
  const int lane = threadIdx.x & (tpr - 1);
  const int rpb = 256 >> tpr_log2;
  const int Tw = T * wpe;
  for (int row = blockIdx.y * rpb + (threadIdx.x >> tpr_log2); row < rows; row += gridDim.y * rpb) {
    const int b = row / C;
    const int n0 = (row_len(lens, b, INT_MAX) / unit);
    if (n0 >= T) continue;
    const int w0 = n0 * wpe;
    float* r = x + (long long)row * Tw;
    int head = w0 + (int)((4u - (unsigned)(((uintptr_t)(r + w0) >> 2) & 3u)) & 3u);
    if (head > Tw) head = Tw;
    const int nvec = (Tw - head) >> 2;
    if (blockIdx.x == 0) {
      for (int t = w0 + lane; t < head; t += tpr) r[t] = 0.f;
      for (int t = head + 4 * nvec + lane; t < Tw; t += tpr) r[t] = 0.f;
    }
    float4* v = reinterpret_cast<float4*>(r + head);
    for (int i = blockIdx.x * tpr + lane; i < nvec; i += gridDim.x * tpr) v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// mask[b, f] = f < lens[b] / unit (float 0 / 1, the mask argument of fac_attention / fac_masked_mean / fac_mul_mask);
// n_valid[b] = min(lens[b] / unit, F) when asked for.
__global__ __launch_bounds__(256) void frame_mask_kernel(const int* __restrict__ lens, float* __restrict__ mask,
                                                         int* __restrict__ n_valid, int F, int unit) {
  const int b = blockIdx.y;
  const int nf = min(row_len(lens, b, INT_MAX) / unit, F);
  for (int f = blockIdx.x * 256 + threadIdx.x; f < F; f += gridDim.x * 256) mask[(long long)b * F + f] = f < nf ? 1.f : 0.f;
  if (n_valid && blockIdx.x == 0 && threadIdx.x == 0) n_valid[b] = nf;
}

// x (B, C, T): behind every clip's own end L_b = clamp(lens[b] * mul, 0, T) the next min(n, T - L_b) columns become what a
// non-causal conv pads there when it sees the clip alone -- its reflection x[L_b - 2 - j] (0 where that lies in front of the
// clip), or zeros.  One thread per (row, j): reads lie below L_b and writes at or above it, both inside the row, so the
// in-place form has no hazard.  Store-only but for the reflected sources; nothing else is touched.
__global__ __launch_bounds__(256) void edge_tail_kernel(float* __restrict__ x, const int* __restrict__ lens, int rows, int C,
                                                        int T, int mul, int n, int reflect) {
  const long long total = (long long)rows * n;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int row = (int)(i / n);
    const int j = (int)(i - (long long)row * n);
    const long long Lw = (long long)row_len(lens, row / C, INT_MAX) * mul;
    const int L = Lw > T ? T : (int)Lw;
    if (j >= T - L) continue;
    float* r = x + (long long)row * T;
    const int src = L - 2 - j;
    r[L + j] = (reflect && src >= 0) ? r[src] : 0.f;
  }
}

static int launch_mask_tail(void* x, const int* lens, int B, int C, int T, int wpe, int unit, fac_stream_t stream, const char* what) {
  FAC_REQUIRE(x && lens && B > 0 && C > 0 && T > 0 && unit > 0, "%s: bad arguments", what);
  FAC_REQUIRE((long long)B * C <= (1 << 30) && (long long)T * wpe <= INT_MAX, "%s: B*C = %lld rows of %lld words do not fit 32-bit indices",
              what, (long long)B * C, (long long)T * wpe);
  FAC_REQUIRE(((uintptr_t)x & 3) == 0, "%s: x is not 4-byte aligned", what);
  const int rows = B * C;
  const int nvec = (T * wpe + 3) / 4;
  int tpr_log2 = 0;
  while (tpr_log2 < 8 && (1 << tpr_log2) < nvec) ++tpr_log2;
  const int tpr = 1 << tpr_log2, rpb = 256 >> tpr_log2;
  int gx = (nvec + tpr * 4 - 1) / (tpr * 4);            // up to 4 16-byte stores per thread
  if (gx > 1024) gx = 1024;
  long long gy = ((long long)rows + rpb - 1) / rpb;
  if (gy > 65535) gy = 65535;
  hipLaunchKernelGGL(mask_tail_kernel, dim3(gx, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<float*>(x), lens,
                     rows, C, T, wpe, unit, tpr_log2);
  return check_launch(what);
}

}  // namespace fac

using namespace fac;

extern "C" int fac_stft_frames_ragged(const float* wave, const int32_t* lens, float* frames, int B, int T, int n_win, int n_frames,
                                      int hop, int pad, int n_off, fac_stream_t stream) {
  FAC_REQUIRE(wave && lens && frames && B > 0 && T > 0 && n_win > 0 && n_frames > 0 && hop > 0 && pad >= 0,
              "stft_frames_ragged: bad arguments");
  FAC_REQUIRE(B <= 65535 && (long long)n_win * n_frames <= INT_MAX && (long long)n_frames * hop + n_win + n_off <= INT_MAX,
              "stft_frames_ragged: B = %d rows of %d x %d frame entries do not fit the grid / 32-bit indices", B, n_win, n_frames);
  const int per_b = n_win * n_frames;
  int gx = (per_b + 1023) / 1024;                        // four entries per thread
  if (gx > 4096) gx = 4096;
  hipLaunchKernelGGL(stft_frames_ragged_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, wave, lens, frames, T, n_win,
                     n_frames, hop, pad, n_off);
  return check_launch("stft_frames_ragged");
}

extern "C" int fac_mask_tail(float* x, const int32_t* lens, int B, int C, int T, int unit, fac_stream_t stream) {
  return launch_mask_tail(x, lens, B, C, T, 1, unit, stream, "mask_tail");
}

extern "C" int fac_mask_tail_i64(int64_t* x, const int32_t* lens, int B, int C, int T, int unit, fac_stream_t stream) {
  return launch_mask_tail(x, lens, B, C, T, 2, unit, stream, "mask_tail_i64");
}

extern "C" int fac_edge_tail(float* x, const int32_t* lens, int B, int C, int T, int mul, int n, int mode, fac_stream_t stream) {
  FAC_REQUIRE(x && lens && B > 0 && C > 0 && T > 0 && mul > 0 && n > 0, "edge_tail: bad arguments");
  FAC_REQUIRE(mode == FAC_PAD_ZERO || mode == FAC_PAD_REFLECT, "edge_tail: mode %d is neither FAC_PAD_ZERO nor FAC_PAD_REFLECT", mode);
  FAC_REQUIRE((long long)B * C <= (1 << 30), "edge_tail: B*C = %lld rows do not fit 32-bit indices", (long long)B * C);
  FAC_REQUIRE(((uintptr_t)x & 3) == 0, "edge_tail: x is not 4-byte aligned");
  if (n > T) n = T;                                          // a row has no more than T columns behind any end
  const long long total = (long long)B * C * n;
  long long g = (total + 255) / 256;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(edge_tail_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, x, lens, B * C, C, T, mul, n,
                     mode == FAC_PAD_REFLECT ? 1 : 0);
  return check_launch("edge_tail");
}

extern "C" int fac_frame_mask(const int32_t* lens, float* mask, int32_t* n_valid, int B, int F, int unit, fac_stream_t stream) {
  FAC_REQUIRE(lens && mask && B > 0 && B <= 65535 && F > 0 && unit > 0, "frame_mask: bad arguments");
  int gx = (F + 255) / 256;
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(frame_mask_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, lens, mask, n_valid, F, unit);
  return check_launch("frame_mask");
}
