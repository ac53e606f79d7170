// Pitch on the device: the glue of the JDC F0 extractor (modules/JDC/model.py) around the conv and LSTM kernels, and the two
// target kernels of train.py:215-256 (F0 normalisation per clip, log of the mel norm).
//
// Working layout (the spectrogram discriminator's, stride 1): every channel is one signal of rows * P floats, row
// r = b * (T + 1) + t holds the W valid frequency bins of frame t followed by zeros up to the row pitch P; row t = T of every clip
// is all zero.  A 3 x 3 Conv2d is then ONE two-level-tap 1-D conv over the signal (fac_conv1d_fwd, K = 9, K1 = 3, dilation2 = P,
// pad_left = P + 1): the gap columns and the separator rows are its zero padding.  The kernels here are HBM-bound layout /
// elementwise passes: 16-byte accesses where the pitch allows, no atomics, reductions in a fixed order.
#include "common.h"
#include "../../include/facodec_hip.h"

namespace fac {

#define JDC_GRID_STRIDE(i, n) for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long long)gridDim.x * blockDim.x)
static inline int jdc_grid(long long n) { return (int)((n + 255) / 256 < 65535 ? (n + 255) / 256 : 65535); }

__device__ __forceinline__ float jdc_act(float x, float sc, float sh, float slope) {
  const float v = fmaf(x, sc, sh);
  return v > 0.f ? v : v * slope;
}

// y[c, r, j] = max_{i < pool} lrelu(scale[c] * x[c, r, j * pool + i] + shift[c]) for j < W_in / pool on the valid rows; exact zeros
// everywhere else.  One output element per thread: any pitch, any pool.
__global__ void jdc_pool_kernel(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                                float* __restrict__ y, int rows, int rpg, int W_in, int P_in, int pool, int P_out, float slope,
                                long long n) {
  const int W_out = W_in / pool;
  JDC_GRID_STRIDE(i, n) {
    const int j = (int)(i % P_out);
    const long long cr = i / P_out;
    const int r = (int)(cr % rows);
    const int c = (int)(cr / rows);
    float m = 0.f;
    if (j < W_out && r % rpg < rpg - 1) {
      const float sc = scale ? scale[c] : 1.f, sh = shift ? shift[c] : 0.f;
      const float* xr = x + ((long long)c * rows + r) * P_in + (long long)j * pool;
      m = jdc_act(xr[0], sc, sh, slope);                // the running maximum starts from the first element, not from 0
      for (int k = 1; k < pool; ++k) {
        const float v = jdc_act(xr[k], sc, sh, slope);
        m = v > m ? v : m;
      }
    }
    y[i] = m;
  }
}

// Four consecutive outputs per thread: POOL 16-byte loads, one 16-byte store.  Needs P_out % 4 == 0 (a quad never straddles two
// rows; P_in = POOL * P_out is then a multiple of 4 as well) and 16-byte aligned tensors.  Separator rows are not read at all; of a
// valid row the gap columns inside the quads that also hold data are loaded and dropped.
template <int POOL>
__global__ void jdc_pool_quad_kernel(const float4* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                                     float4* __restrict__ y, int rows, int rpg, int W_in, int P_out4, float slope, long long n4) {
  const int W_out = W_in / POOL;
  JDC_GRID_STRIDE(q, n4) {
    const int j4 = (int)(q % P_out4);
    const long long cr = q / P_out4;
    const int r = (int)(cr % rows);
    const int c = (int)(cr / rows);
    const int left = (r % rpg < rpg - 1) ? W_out - 4 * j4 : 0;      // how many of the quad's outputs carry data
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (left > 0) {
      const float sc = scale ? scale[c] : 1.f, sh = shift ? shift[c] : 0.f;
      const float4* xq = x + (cr * P_out4 + j4) * POOL;
      float in[4 * POOL];
#pragma unroll
      for (int k = 0; k < POOL; ++k) {
        const float4 v = xq[k];
        in[4 * k] = v.x; in[4 * k + 1] = v.y; in[4 * k + 2] = v.z; in[4 * k + 3] = v.w;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float m = jdc_act(in[u * POOL], sc, sh, slope);
#pragma unroll
        for (int k = 1; k < POOL; ++k) {
          const float v = jdc_act(in[u * POOL + k], sc, sh, slope);
          m = v > m ? v : m;
        }
        o[u] = u < left ? m : 0.f;
      }
    }
    y[q] = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// mel (B, 1, W, T) -> the stage-0 signal (rows * P): a transpose into rows of pitch P, zeros in the gaps and separator rows.
__global__ void jdc_layout_in_kernel(const float* __restrict__ mel, float* __restrict__ out, int W, int T, int P, long long n) {
  JDC_GRID_STRIDE(i, n) {
    const int j = (int)(i % P);
    const long long r = i / P;
    const int t = (int)(r % (T + 1));
    const long long b = r / (T + 1);
    out[i] = (j < W && t < T) ? mel[(b * W + j) * T + t] : 0.f;
  }
}

// Stage signal (C channels, valid width W) -> time-major LSTM input (C * W, T, BP), feature c * W + w, zero batch padding;
// reverse: time flipped.
__global__ void jdc_to_time_major_kernel(const float* __restrict__ x, float* __restrict__ xT, int B, int T, int W, int P, int BP,
                                         int reverse, long long n) {
  JDC_GRID_STRIDE(i, n) {
    const int b = (int)(i % BP);
    const long long ft = i / BP;
    const int to = (int)(ft % T);
    const long long f = ft / T;
    const int w = (int)(f % W);
    const long long c = f / W;
    const int t = reverse ? T - 1 - to : to;
    xT[i] = b < B ? x[(c * B * (T + 1) + (long long)b * (T + 1) + t) * P + w] : 0.f;
  }
}

// Stage signal -> (B, C, T, W) (transposed = 0) or (B, C, W, T) (transposed = 1), contiguous.
__global__ void jdc_to_nchw_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int C, int T, int W, int P,
                                   int transposed, long long n) {
  JDC_GRID_STRIDE(i, n) {
    int t, w;
    long long bc;
    if (transposed) { t = (int)(i % T); w = (int)((i / T) % W); bc = i / ((long long)T * W); }
    else { w = (int)(i % W); t = (int)((i / W) % T); bc = i / ((long long)T * W); }
    const int c = (int)(bc % C);
    const long long b = bc / C;
    out[i] = x[((long long)c * B * (T + 1) + b * (T + 1) + t) * P + w];
  }
}

// |w . [h_fwd(t) | h_bwd(T - 1 - t)] + bias| -> out (B, T).  One workgroup per (time step, block of 32 batch columns): 8 groups of
// 32 lanes each sum a contiguous eighth of the 2H features in order, the eight partial sums are added in order.
__global__ __launch_bounds__(256) void jdc_head_kernel(const float* __restrict__ hf, const float* __restrict__ hb,
                                                       const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ out, int B, int T, int H, int BP) {
  __shared__ float red[8][32];
  const int t = blockIdx.x, b = blockIdx.y * 32 + (threadIdx.x & 31), g = threadIdx.x >> 5;
  const int per = 2 * H / 8;
  float s = 0.f;
  if (b < BP) {
    for (int f = g * per; f < (g + 1) * per; ++f) {
      const float h = f < H ? hf[((long long)f * T + t) * BP + b] : hb[((long long)(f - H) * T + (T - 1 - t)) * BP + b];
      s = fmaf(w[f], h, s);
    }
  }
  red[g][threadIdx.x & 31] = s;
  __syncthreads();
  if (g == 0 && b < B) {
    float a = red[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < 8; ++k) a += red[k][threadIdx.x];
    out[(long long)b * T + t] = fabsf(a + bias[0]);
  }
}

// Fixed-order tree over the 256 threads' values.
__device__ __forceinline__ float jdc_block_sum(float v, float* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  return red[0];
}

// train.py:224-256, one workgroup per clip.  The sums run over d = log2(f0) - pivot with the first voiced frame's log2 as the
// pivot (0 when that is not finite): small terms, and a clip whose voiced frames are all equal has every d, the mean of d and
// the standard deviation exactly 0, hence 0 / 0 = NaN -> -10 on every frame, like a clip with one voiced frame (0 / (n - 1) = NaN).
__global__ __launch_bounds__(256) void f0_normalize_kernel(const float* __restrict__ f0, float* __restrict__ out,
                                                           float* __restrict__ mean_out, int T) {
  __shared__ float red[256];
  __shared__ int redi[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* fr = f0 + (long long)b * T;
  int first = T, cnt = 0;
  for (int t = tid; t < T; t += 256) {
    if (fr[t] > 5.0f) { first = t < first ? t : first; ++cnt; }
  }
  redi[tid] = first;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) redi[tid] = redi[tid + o] < redi[tid] ? redi[tid + o] : redi[tid];
    __syncthreads();
  }
  first = redi[0];
  const float n = jdc_block_sum((float)cnt, red);        // exact: integers below 2^24
  if (first >= T) {                                      // no voiced frame
    for (int t = tid; t < T; t += 256) out[(long long)b * T + t] = -10.0f;
    if (mean_out && tid == 0) mean_out[b] = 0.f;
    return;
  }
  const float l0 = log2f(fr[first]);
  const float piv = isfinite(l0) ? l0 : 0.f;
  float s = 0.f;
  for (int t = tid; t < T; t += 256) {
    if (fr[t] > 5.0f) s += log2f(fr[t]) - piv;
  }
  const float md = jdc_block_sum(s, red) / n;
  float ss = 0.f;
  for (int t = tid; t < T; t += 256) {
    if (fr[t] > 5.0f) { const float d = (log2f(fr[t]) - piv) - md; ss = fmaf(d, d, ss); }
  }
  const float sd = sqrtf(jdc_block_sum(ss, red) / (n - 1.0f));
  for (int t = tid; t < T; t += 256) {
    float v = -10.0f;
    if (fr[t] > 5.0f) {
      v = ((log2f(fr[t]) - piv) - md) / sd;
      if (!isfinite(v)) v = -10.0f;
    }
    out[(long long)b * T + t] = v;
  }
  if (mean_out && tid == 0) mean_out[b] = piv + md;
}

// modules/commons.py:176-181 with its defaults: out[b, t] = log(sqrt(sum_m exp(4 mel[b, m, t] - 4)^2)), the sum in bin order.
__global__ void mel_log_norm_kernel(const float* __restrict__ mel, float* __restrict__ out, int M, int T, long long n) {
  JDC_GRID_STRIDE(i, n) {
    const int t = (int)(i % T);
    const long long b = i / T;
    const float* p = mel + b * M * T + t;
    float s = 0.f;
    for (int m = 0; m < M; ++m) {
      const float e = expf(p[(long long)m * T] * 4.0f + -4.0f);
      s = fmaf(e, e, s);
    }
    out[i] = logf(sqrtf(s));
  }
}

}  // namespace fac

#define JL1(kern, n, ...) hipLaunchKernelGGL(fac::kern, dim3(fac::jdc_grid(n)), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__)

static inline bool jdc_al16(const void* a, const void* b) {
  return ((reinterpret_cast<unsigned long long>(a) | reinterpret_cast<unsigned long long>(b)) & 15) == 0;
}

extern "C" int fac_jdc_affine_lrelu_pool(const float* x, const float* scale, const float* shift, float* y, int C, int rows,
                                         int rows_per_group, int W_in, int P_in, int pool, int P_out, float slope,
                                         fac_stream_t stream) {
  FAC_REQUIRE(x && y && x != y && C > 0 && rows > 0 && rows_per_group > 1 && rows % rows_per_group == 0 && pool >= 1 && W_in >= pool &&
                  W_in <= P_in && P_out >= 1 && (long long)P_out * pool == P_in && (!scale) == (!shift),
              "jdc_affine_lrelu_pool: bad arguments (C=%d rows=%d rows_per_group=%d W_in=%d P_in=%d pool=%d P_out=%d)", C, rows,
              rows_per_group, W_in, P_in, pool, P_out);
  const long long n = (long long)C * rows * P_out;
  if (P_out % 4 == 0 && (pool == 1 || pool == 2 || pool == 4) && jdc_al16(x, y)) {
    const float4* x4 = reinterpret_cast<const float4*>(x);
    float4* y4 = reinterpret_cast<float4*>(y);
    const long long n4 = n / 4;
    if (pool == 1) JL1(jdc_pool_quad_kernel<1>, n4, x4, scale, shift, y4, rows, rows_per_group, W_in, P_out / 4, slope, n4);
    else if (pool == 2) JL1(jdc_pool_quad_kernel<2>, n4, x4, scale, shift, y4, rows, rows_per_group, W_in, P_out / 4, slope, n4);
    else JL1(jdc_pool_quad_kernel<4>, n4, x4, scale, shift, y4, rows, rows_per_group, W_in, P_out / 4, slope, n4);
  } else {
    JL1(jdc_pool_kernel, n, x, scale, shift, y, rows, rows_per_group, W_in, P_in, pool, P_out, slope, n);
  }
  return fac::check_launch("jdc_affine_lrelu_pool");
}

extern "C" int fac_jdc_layout_in(const float* mel, float* out, int B, int W, int T, int P, fac_stream_t stream) {
  FAC_REQUIRE(mel && out && B > 0 && W > 0 && T > 0 && P > W, "jdc_layout_in: bad arguments (B=%d W=%d T=%d P=%d)", B, W, T, P);
  const long long n = (long long)B * (T + 1) * P;
  JL1(jdc_layout_in_kernel, n, mel, out, W, T, P, n);
  return fac::check_launch("jdc_layout_in");
}

extern "C" int fac_jdc_to_time_major(const float* x, float* xT, int B, int C, int T, int W, int P, int BP, int reverse,
                                     fac_stream_t stream) {
  FAC_REQUIRE(x && xT && B > 0 && C > 0 && T > 0 && W > 0 && W <= P && BP >= B, "jdc_to_time_major: bad arguments");
  const long long n = (long long)C * W * T * BP;
  JL1(jdc_to_time_major_kernel, n, x, xT, B, T, W, P, BP, reverse ? 1 : 0, n);
  return fac::check_launch("jdc_to_time_major");
}

extern "C" int fac_jdc_to_nchw(const float* x, float* out, int B, int C, int T, int W, int P, int transposed, fac_stream_t stream) {
  FAC_REQUIRE(x && out && B > 0 && C > 0 && T > 0 && W > 0 && W <= P, "jdc_to_nchw: bad arguments");
  const long long n = (long long)B * C * T * W;
  JL1(jdc_to_nchw_kernel, n, x, out, B, C, T, W, P, transposed ? 1 : 0, n);
  return fac::check_launch("jdc_to_nchw");
}

extern "C" int fac_jdc_head(const float* h_fwd, const float* h_bwd, const float* w, const float* bias, float* out, int B, int T,
                            int H, int BP, fac_stream_t stream) {
  FAC_REQUIRE(h_fwd && h_bwd && w && bias && out && B > 0 && T > 0 && H > 0 && H % 4 == 0 && BP >= B && (BP + 31) / 32 <= 65535,
              "jdc_head: bad arguments (B=%d T=%d H=%d BP=%d)", B, T, H, BP);
  hipLaunchKernelGGL(fac::jdc_head_kernel, dim3(T, (BP + 31) / 32), dim3(256), 0, (hipStream_t)stream, h_fwd, h_bwd, w, bias, out, B,
                     T, H, BP);
  return fac::check_launch("jdc_head");
}

extern "C" int fac_f0_normalize(const float* f0, float* out, float* mean_out, int B, int T, fac_stream_t stream) {
  FAC_REQUIRE(f0 && out && B > 0 && T > 0, "f0_normalize: bad arguments (B=%d T=%d)", B, T);
  hipLaunchKernelGGL(fac::f0_normalize_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, f0, out, mean_out, T);
  return fac::check_launch("f0_normalize");
}

extern "C" int fac_mel_log_norm(const float* mel, float* out, int B, int n_mels, int T, fac_stream_t stream) {
  FAC_REQUIRE(mel && out && B > 0 && n_mels > 0 && T > 0, "mel_log_norm: bad arguments (B=%d n_mels=%d T=%d)", B, n_mels, T);
  const long long n = (long long)B * T;
  JL1(mel_log_norm_kernel, n, mel, out, n_mels, T, n);
  return fac::check_launch("mel_log_norm");
}
