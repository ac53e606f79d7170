// Backward kernels of the voice-conversion Redecoder's training step (train_redecoder.py:195-328, modules/redecoder.py,
// modules/wavenet.py:138-166 with gin_channels):
//   * fac_embed_sum_bwd   dense gradient of the code-embedding tables (the adjoint of fac_embed_sum), a scatter-add by code;
//   * fac_gate_bwd_cond   backward of the conditioned tanh/sigmoid gate, plus the per-clip conditioning gradient
//                         dcond[b, :] = sum_t d(pre-gate)[b, :, t].
// Both are deterministic: no floating-point atomics, every sum is taken in one fixed order.
#include "common.h"
#include "../../include/facodec_hip.h"

namespace fac {

// ----------------------------------------------------------------------------------------------------- embedding backward
// One workgroup per (table, slice of EB_CH channels).  The slice of the table's gradient, V x EB_CH fp32 (32 KB at V = 1024),
// lives in LDS for the whole launch.  dx is staged in chunks of EB_FR frames (rows padded by one float: lane c reads row c at
// one frame, a different bank per lane).  Lane (c, part) owns channel c of the codes with code % EB_PARTS == part, so two frames
// that share a code (silence repeats one code) are always added by the same lane, in frame order (b major, then t): no race,
// and the summation order of every table element is fixed.
constexpr int EB_CH = 8, EB_THREADS = 256, EB_PARTS = EB_THREADS / EB_CH, EB_FR = 256, EB_VMAX = 1024;

__global__ __launch_bounds__(EB_THREADS) void embed_sum_bwd_kernel(const float* __restrict__ dx, const long long* __restrict__ codes,
                                                                  float* __restrict__ dtab, int B, int n_codes, int code_row0, int V,
                                                                  int E, int T) {
  __shared__ float acc[EB_VMAX * EB_CH];
  __shared__ float xs[EB_CH][EB_FR + 1];
  __shared__ int cs[EB_FR];
  const int tab = blockIdx.y, e0 = blockIdx.x * EB_CH, tid = threadIdx.x;
  const int nch = E - e0 < EB_CH ? E - e0 : EB_CH;
  const int c = tid % EB_CH, part = tid / EB_CH;
  for (int i = tid; i < V * EB_CH; i += EB_THREADS) acc[i] = 0.f;
  for (int b = 0; b < B; ++b) {
    const long long* crow = codes + ((long long)b * n_codes + code_row0 + tab) * T;
    for (int t0 = 0; t0 < T; t0 += EB_FR) {
      const int nf = T - t0 < EB_FR ? T - t0 : EB_FR;
      __syncthreads();                                        // the previous chunk is consumed (first pass: acc is zeroed)
      for (int i = tid; i < EB_CH * EB_FR; i += EB_THREADS) {  // row-contiguous loads: consecutive lanes, consecutive frames
        const int r = i / EB_FR, f = i - r * EB_FR;
        xs[r][f] = (r < nch && f < nf) ? dx[((long long)b * E + e0 + r) * T + t0 + f] : 0.f;
      }
      for (int f = tid; f < nf; f += EB_THREADS) {
        const long long id = crow[t0 + f];
        cs[f] = (id >= 0 && id < V) ? (int)id : -1;           // a code outside the table contributes nothing
      }
      __syncthreads();
      if (c < nch) {
        for (int f = 0; f < nf; ++f) {
          const int id = cs[f];
          if (id >= 0 && id % EB_PARTS == part) acc[id * EB_CH + c] = __fadd_rn(acc[id * EB_CH + c], xs[c][f]);
        }
      }
    }
  }
  __syncthreads();
  float* out = dtab + (long long)tab * V * E;
  for (int i = tid; i < V * EB_CH; i += EB_THREADS) {
    const int v = i / EB_CH, r = i - v * EB_CH;
    if (r < nch) out[(long long)v * E + e0 + r] = acc[i];
  }
}

// ----------------------------------------------------------------------------------------------------- conditioned gate backward
// acts = tanh(a1 + g1) * sigmoid(a2 + g2) (fac_gate_tanh_sigmoid with g): da1 = d sig (1 - th^2), da2 = d th sig (1 - sig) -- the
// arithmetic of gate_bwd_kernel on the conditioned pre-activations -- and dcond = sum over t of da.  One wave per (clip, channel):
// lanes stride over time, then a fixed shuffle tree.
constexpr int GC_WAVES = 4;

__global__ __launch_bounds__(64 * GC_WAVES) void gate_bwd_cond_kernel(const float* __restrict__ a, const float* __restrict__ g,
                                                                     long long g_bs, const float* __restrict__ d, float* __restrict__ da,
                                                                     float* __restrict__ dcond, long long dc_bs, int B, int C, int T) {
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const long long row = (long long)blockIdx.x * GC_WAVES + wave;     // b * C + c
  if (row >= (long long)B * C) return;
  const int b = (int)(row / C), c = (int)(row - (long long)b * C);
  const float g1 = g[b * g_bs + c], g2 = g[b * g_bs + C + c];
  const long long o1 = ((long long)b * 2 * C + c) * T, o2 = o1 + (long long)C * T;
  const float* drow = d + row * T;
  float s1 = 0.f, s2 = 0.f;
  for (int t = lane; t < T; t += 64) {
    const float ta = __fadd_rn(a[o1 + t], g1), sa = __fadd_rn(a[o2 + t], g2);
    const float th = tanhf(ta), sg = 1.f / (1.f + expf(-sa));
    const float v1 = drow[t] * sg * (1.f - th * th);
    const float v2 = drow[t] * th * sg * (1.f - sg);
    da[o1 + t] = v1;
    da[o2 + t] = v2;
    s1 += v1;
    s2 += v2;
  }
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_down(s1, off, 64);
    s2 += __shfl_down(s2, off, 64);
  }
  if (lane == 0) {
    dcond[b * dc_bs + c] = s1;
    dcond[b * dc_bs + C + c] = s2;
  }
}

}  // namespace fac

extern "C" int fac_embed_sum_bwd(const float* dx, const int64_t* codes, float* dtables, int B, int n_tab, int n_codes, int code_row0,
                                 int V, int E, int T, fac_stream_t stream) {
  FAC_REQUIRE(dx && codes && dtables && B > 0 && n_tab > 0 && n_tab <= 65535 && V > 0 && V <= fac::EB_VMAX && E > 0 && T > 0 &&
                  code_row0 >= 0 && code_row0 + n_tab <= n_codes,
              "embed_sum_bwd: bad arguments (B=%d n_tab=%d n_codes=%d code_row0=%d V=%d E=%d T=%d)", B, n_tab, n_codes, code_row0,
              V, E, T);
  dim3 grid((E + fac::EB_CH - 1) / fac::EB_CH, n_tab);
  hipLaunchKernelGGL(fac::embed_sum_bwd_kernel, grid, dim3(fac::EB_THREADS), 0, (hipStream_t)stream, dx, (const long long*)codes,
                     dtables, B, n_codes, code_row0, V, E, T);
  return fac::check_launch("embed_sum_bwd");
}

extern "C" int fac_gate_bwd_cond(const float* a, const float* g, int64_t g_bs, const float* d, float* da, float* dcond, int64_t dcond_bs,
                                 int B, int C, int T, fac_stream_t stream) {
  FAC_REQUIRE(a && g && d && da && dcond && B > 0 && C > 0 && T > 0 && g_bs >= 2 * (int64_t)C && dcond_bs >= 2 * (int64_t)C,
              "gate_bwd_cond: bad arguments (B=%d C=%d T=%d g_bs=%lld dcond_bs=%lld)", B, C, T, (long long)g_bs, (long long)dcond_bs);
  const long long rows = (long long)B * C;
  const long long blocks = (rows + fac::GC_WAVES - 1) / fac::GC_WAVES;
  FAC_REQUIRE(blocks < (1ll << 31), "gate_bwd_cond: too many rows");
  hipLaunchKernelGGL(fac::gate_bwd_cond_kernel, dim3((unsigned)blocks), dim3(64 * fac::GC_WAVES), 0, (hipStream_t)stream, a, g,
                     (long long)g_bs, d, da, dcond, (long long)dcond_bs, B, C, T);
  return fac::check_launch("gate_bwd_cond");
}
