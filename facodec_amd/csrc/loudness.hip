// Loudness on the device: the ITU-R BS.1770-4 K-weighting filter bank fused with the sub-block energy sums, the
// two-gate integrated loudness over those energies, and the level normalisation built on it.  What is computed is stated in
// include/facodec_hip.h above fac_kweight_desc; this comment is about how.
//
// fac_kweight_energy.  The two biquads in transposed direct form II are one linear recurrence state' = M state + v x on the state
// (s1, s2, t1, t2), so a row's time axis is cut into chunks of LD_L samples, one lane each, LD_W = 64 chunks (one wave, one
// "segment" of 16384 samples) to a workgroup:
//   kweight_kernel<false>  every chunk runs from zero state; the wave then combines its 64 end states by a Kogge-Stone scan,
//                          step k adding M^(L 2^k) times the state 2^k lanes below: lane i ends up with the state at the end of
//                          chunk i for a segment entered with zero state.  Written to the workspace.
//   kweight_scan_kernel    one wave per row hands states across segments with P = M^(64 L): 64 segment ends at a time go through
//                          the same scan (with P^(2^k), squared in the kernel) and one carry steps over the 64 with P^64.  This
//                          is the only serial step: T / 2^20 rounds per row (83 for an hour at 24 kHz, about 110 us; walking the
//                          5274 segment states one by one took 380 us).  Not launched for a single segment.
//   kweight_kernel<true>   every chunk rebuilds its true start state -- M^(L lane) times the segment's start, by the binary
//                          digits of the lane with the same seven matrices, plus the scanned state of the chunk before it --,
//                          re-runs its samples and sums squares, split where a sub-block boundary crosses the chunk (S >= L: at
//                          most one), and takes max |x|.  A call of one chunk (a short streaming push) launches only this.
//   kweight_reduce_kernel  e[b, j] = the partial sums of the chunks that overlap sub-block j, added in ascending chunk order
//                          (S / L + 2 of them at most); the row's peak from the per-segment peaks.
// No atomics and no order that depends on scheduling: two runs give the same bits.  The input is read twice (three times by
// normalize: the gain launch), the filtered signal stays in registers.
//
// Input staging.  A lane walks its own chunk, so the lanes of a wave read L floats apart.  Per step of LD_TILE = 32 samples the
// wave copies its 64 x 32 block through LDS: loads with 32 consecutive lanes on 128 consecutive bytes, stored at a row pitch of
// 33 words so that the per-lane reads (lane * 33 + i) fall on 32 different banks.  Any row pitch and alignment of x works.
// The 32 loads of a step are issued together, one step ahead of the arithmetic that needs them (a first version loaded
// conditionally, which the compiler turned into 32 load-wait-store rounds per step: 522 instead of 188 us for an hour of audio
// in 64 rows).
//
// What bounds it: two floors that lie close together, neither of which it reaches.  A sample costs about 14 vector instructions
// per lane in the state pass and 22 in the energy pass (12 fp64 fma / mul, the conversion, the square, two selected sums, the peak)
// plus the staging, ~45 in all at 4 cycles each per wave: an hour of audio is 1.35 M wave-samples, ~100 us of VALU issue on 1024
// SIMDs.  Its two reads take 110 us at the 6.3 TB/s a plain copy reaches.  Measured: 188 us for an hour in 64 rows, 3.7 TB/s of
// input traffic, 46 % of the 8 TB/s peak: the staging and arithmetic phases of a wave alternate between barriers
// and the dependent chain s -> y1 -> s' leaves issue slots empty, which the 4 to 5 waves per SIMD (100 VGPRs) cover only in part.
#include "common.h"
#include <limits.h>
#include <math.h>

namespace fac {

constexpr int LD_L = FAC_LOUDNESS_CHUNK;   // samples per chunk (one lane)
constexpr int LD_W = 64;                   // chunks per workgroup = one wave = one segment
constexpr int LD_TILE = 32;                // samples per chunk staged per step
constexpr int LD_PITCH = LD_TILE + 1;
constexpr int LD_SCAN_T = 64;              // lanes of the scan kernel: segments per round
static_assert(LD_L % LD_TILE == 0 && LD_W == 64 && (LD_W * LD_TILE) % 64 == 0, "loudness tile geometry");

struct KwArgs {
  fac_kweight_desc d;
  int n_chunks, n_seg, n_sub;
  double* ws_state;   // (B, n_chunks, 4) scanned end states of the chunks (segment entered with zero state)
  double* ws_seg;     // (B, n_seg, 4)    true start state of every segment
  double* ws_part;    // (B, n_chunks, 2) sums of squares before / behind the sub-block boundary inside the chunk
  float* ws_peak;     // (B, n_seg)       max |x| per segment
};

struct St {
  double s1, s2, t1, t2;
};

__device__ __forceinline__ St st_load(const double* p) { return St{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ void st_store(double* p, const St& s) { p[0] = s.s1, p[1] = s.s2, p[2] = s.t1, p[3] = s.t2; }
__device__ __forceinline__ St st_add(const St& a, const St& b) { return St{a.s1 + b.s1, a.s2 + b.s2, a.t1 + b.t1, a.t2 + b.t2}; }
// m (row-major 4 x 4) times v, every row in the same fixed order
__device__ __forceinline__ St st_mul(const double* m, const St& v) {
  St r;
  r.s1 = fma(m[3], v.t2, fma(m[2], v.t1, fma(m[1], v.s2, m[0] * v.s1)));
  r.s2 = fma(m[7], v.t2, fma(m[6], v.t1, fma(m[5], v.s2, m[4] * v.s1)));
  r.t1 = fma(m[11], v.t2, fma(m[10], v.t1, fma(m[9], v.s2, m[8] * v.s1)));
  r.t2 = fma(m[15], v.t2, fma(m[14], v.t1, fma(m[13], v.s2, m[12] * v.s1)));
  return r;
}

__device__ __forceinline__ int row_len(const int32_t* lens, int b, int T) {
  if (!lens) return T;
  const int L = lens[b];
  return L < 0 ? 0 : (L > T ? T : L);
}

template <bool ENERGY>
__global__ __launch_bounds__(LD_W) void kweight_kernel(KwArgs a) {
  __shared__ float xs[LD_W * LD_PITCH];
  const fac_kweight_desc& d = a.d;
  const int b = blockIdx.y, seg = blockIdx.x, lane = threadIdx.x;
  const int len = row_len(d.lens, b, d.T);
  const int c = seg * LD_W + lane;
  const bool have = c < a.n_chunks;
  const int t_seg = seg * (LD_W * LD_L);          // < T + 2^14 <= 2^30 + 2^14
  const int t0 = t_seg + lane * LD_L;
  const float* __restrict__ xrow = d.x + b * d.x_bs;
  double* st_row = a.ws_state + (long long)b * a.n_chunks * 4;
  double* part_row = a.ws_part + (long long)b * a.n_chunks * 2;

  if (t_seg >= len) {
    // the whole segment lies behind the clip: nothing to filter (never the case without lens, so state_out is not concerned)
    if (ENERGY) {
      if (have) part_row[2 * c] = 0.0, part_row[2 * c + 1] = 0.0;
      if (lane == 0) a.ws_peak[(long long)b * a.n_seg + seg] = 0.f;
    } else if (have) {
      st_store(st_row + 4ll * c, St{0.0, 0.0, 0.0, 0.0});
    }
    return;
  }

  St s{0.0, 0.0, 0.0, 0.0};
  int tb = INT_MAX;                               // first sample of the chunk's second sub-block
  if (ENERGY) {
    St p{0.0, 0.0, 0.0, 0.0};
    if (a.n_seg > 1) p = st_load(a.ws_seg + ((long long)b * a.n_seg + seg) * 4);
    else if (d.state_in) p = st_load(d.state_in + 4ll * b);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const St q = st_mul(d.pw[k], p);
      if ((lane >> k) & 1) p = q;
    }
    if (lane > 0 && have) p = st_add(p, st_load(st_row + 4ll * (c - 1)));
    s = p;
    tb = ((d.offset + t0) / d.S + 1) * d.S - d.offset;
  }
  const double b0 = d.coef[0], b1 = d.coef[1], b2 = d.coef[2], a1 = d.coef[3], a2 = d.coef[4];
  const double c0 = d.coef[5], c1 = d.coef[6], c2 = d.coef[7], d1 = d.coef[8], d2 = d.coef[9];
  double acc0 = 0.0, acc1 = 0.0;
  float pk = 0.f;

  // The loads of a step are unconditional (index clamped into the clip, which has a sample at t_seg; what lies behind the clip
  // becomes 0 on the way into LDS) and are issued one step ahead, into registers, so that they fly during the arithmetic.
  const int sub_ch = lane >> 5, sub_i = lane & (LD_TILE - 1);      // idx = k * 64 + lane -> chunk 2 k + sub_ch, sample sub_i
  float r[LD_TILE];
#pragma unroll
  for (int k = 0; k < LD_TILE; ++k) r[k] = xrow[min(t_seg + (2 * k + sub_ch) * LD_L + sub_i, len - 1)];

  for (int i0 = 0; i0 < LD_L; i0 += LD_TILE) {
    if (i0) __syncthreads();                      // the previous step's reads of xs are done
#pragma unroll
    for (int k = 0; k < LD_TILE; ++k) {
      const int ch = 2 * k + sub_ch;
      xs[ch * LD_PITCH + sub_i] = t_seg + ch * LD_L + i0 + sub_i < len ? r[k] : 0.f;
    }
    __syncthreads();
    if (i0 + LD_TILE < LD_L) {
#pragma unroll
      for (int k = 0; k < LD_TILE; ++k) r[k] = xrow[min(t_seg + (2 * k + sub_ch) * LD_L + i0 + LD_TILE + sub_i, len - 1)];
    }
    int cnt = LD_TILE;
    if (ENERGY) {
      cnt = len - (t0 + i0);                      // only the clip's own samples are filtered and summed
      cnt = cnt < 0 ? 0 : (cnt > LD_TILE ? LD_TILE : cnt);
    }
    const float* __restrict__ xl = xs + lane * LD_PITCH;
#pragma unroll 8
    for (int i = 0; i < cnt; ++i) {
      const float xf = xl[i];
      const double x = (double)xf;
      const double y1 = fma(b0, x, s.s1);
      s.s1 = fma(-a1, y1, fma(b1, x, s.s2));
      s.s2 = fma(-a2, y1, b2 * x);
      const double y = fma(c0, y1, s.t1);
      s.t1 = fma(-d1, y, fma(c1, y1, s.t2));
      s.t2 = fma(-d2, y, c2 * y1);
      if (ENERGY) {
        const double sq = y * y;
        const bool first = t0 + i0 + i < tb;
        acc0 += first ? sq : 0.0;
        acc1 += first ? 0.0 : sq;
        pk = fmaxf(pk, fabsf(xf));
      }
    }
  }

  if (ENERGY) {
    if (have) part_row[2 * c] = acc0, part_row[2 * c + 1] = acc1;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o, 64));
    if (lane == 0) a.ws_peak[(long long)b * a.n_seg + seg] = pk;
    if (d.state_out && c == a.n_chunks - 1) st_store(d.state_out + 4ll * b, s);
  } else {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int dl = 1 << k;
      St lo;
      lo.s1 = __shfl_up(s.s1, dl, 64), lo.s2 = __shfl_up(s.s2, dl, 64);
      lo.t1 = __shfl_up(s.t1, dl, 64), lo.t2 = __shfl_up(s.t2, dl, 64);
      const St q = st_add(st_mul(d.pw[k], lo), s);
      if (lane >= dl) s = q;
    }
    if (have) st_store(st_row + 4ll * c, s);
  }
}

// One wave per row.  P = pw[6] = M^(64 L) steps a state over one segment; q[k] = P^(2^k), k = 0 .. 6, is squared here, in LDS, in a
// fixed order (P is tiny -- 1e-72 at 24 kHz -- so what it carries across a segment needs no better).  64 segments at a time: lane
// i takes the zero-state end of segment base + i, the same Kogge-Stone scan as in kweight_kernel<false> turns it into the end
// for a group entered with zero state, and segment base + i starts from P^i carry plus the scanned end of the segment before;
// the carry then steps over the group with P^64.  The serial part is n_seg / 64 rounds (83 for an hour at 24 kHz).
__global__ __launch_bounds__(LD_SCAN_T) void kweight_scan_kernel(KwArgs a) {
  __shared__ double q[7][16];
  const fac_kweight_desc& d = a.d;
  const int b = blockIdx.x, lane = threadIdx.x;
  if (lane < 16) q[0][lane] = d.pw[6][lane];
  __syncthreads();
  for (int k = 0; k < 6; ++k) {
    if (lane < 16) {
      const int i = lane >> 2, j = lane & 3;
      const double* m = q[k];
      q[k + 1][lane] = fma(m[4 * i + 3], m[12 + j], fma(m[4 * i + 2], m[8 + j], fma(m[4 * i + 1], m[4 + j], m[4 * i] * m[j])));
    }
    __syncthreads();
  }
  const double* st_row = a.ws_state + (long long)b * a.n_chunks * 4;
  double* seg_row = a.ws_seg + (long long)b * a.n_seg * 4;
  St carry{0.0, 0.0, 0.0, 0.0};
  if (d.state_in) carry = st_load(d.state_in + 4ll * b);
  for (int base = 0; base < a.n_seg; base += LD_SCAN_T) {
    const int seg = base + lane;
    const long long last = (long long)seg * LD_W + LD_W - 1;   // the segment's last chunk; the row's last segment may be short,
    St s{0.0, 0.0, 0.0, 0.0};                                  // and nothing follows it
    if (seg < a.n_seg && last < a.n_chunks) s = st_load(st_row + 4 * last);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int dl = 1 << k;
      St lo;
      lo.s1 = __shfl_up(s.s1, dl, 64), lo.s2 = __shfl_up(s.s2, dl, 64);
      lo.t1 = __shfl_up(s.t1, dl, 64), lo.t2 = __shfl_up(s.t2, dl, 64);
      const St v = st_add(st_mul(q[k], lo), s);
      if (lane >= dl) s = v;
    }
    St p = carry;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const St v = st_mul(q[k], p);
      if ((lane >> k) & 1) p = v;
    }
    St prev;
    prev.s1 = __shfl_up(s.s1, 1, 64), prev.s2 = __shfl_up(s.s2, 1, 64);
    prev.t1 = __shfl_up(s.t1, 1, 64), prev.t2 = __shfl_up(s.t2, 1, 64);
    if (lane > 0) p = st_add(p, prev);
    if (seg < a.n_seg) st_store(seg_row + 4ll * seg, p);
    St top;
    top.s1 = __shfl(s.s1, 63, 64), top.s2 = __shfl(s.s2, 63, 64);
    top.t1 = __shfl(s.t1, 63, 64), top.t2 = __shfl(s.t2, 63, 64);
    carry = st_add(st_mul(q[6], carry), top);
  }
}

__global__ __launch_bounds__(256) void kweight_reduce_kernel(KwArgs a) {
  __shared__ float pks[256];
  const fac_kweight_desc& d = a.d;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int j = blockIdx.x * 256 + tid;
  if (j < a.n_sub) {
    long long lo = (long long)j * d.S - d.offset, hi = lo + d.S;
    if (lo < 0) lo = 0;
    if (hi > d.T) hi = d.T;
    double sum = 0.0;
    if (hi > lo) {
      const double* part_row = a.ws_part + (long long)b * a.n_chunks * 2;
      const int c_lo = (int)(lo / LD_L), c_hi = (int)((hi - 1) / LD_L);
      for (int c = c_lo; c <= c_hi; ++c) {
        const int jc = (int)(((long long)d.offset + (long long)c * LD_L) / d.S);   // the sub-block the chunk starts in
        sum += part_row[2 * c + (jc == j ? 0 : 1)];
      }
    }
    double* e = d.e + b * d.e_bs + j;
    *e = (j == 0 && d.offset > 0) ? *e + sum : sum;
  }
  if (d.peak && blockIdx.x == 0) {
    float pk = 0.f;
    for (int s = tid; s < a.n_seg; s += 256) pk = fmaxf(pk, a.ws_peak[(long long)b * a.n_seg + s]);
    pks[tid] = pk;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
      if (tid < o) pks[tid] = fmaxf(pks[tid], pks[tid + o]);
      __syncthreads();
    }
    if (tid == 0) d.peak[b] = d.peak_accumulate ? fmaxf(d.peak[b], pks[0]) : pks[0];
  }
}

// ---- gating

constexpr int LG_T = 256;
constexpr double LG_ABS = -70.0, LG_OFS = -0.691;

// sum of v over the workgroup in a fixed tree order; every thread gets it
__device__ __forceinline__ double wg_sum(double v, double* red, int tid) {
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int o = LG_T / 2; o >= 1; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ double lufs(double z) { return z > 0.0 ? LG_OFS + 10.0 * log10(z) : -INFINITY; }

__global__ __launch_bounds__(LG_T) void loudness_gate_kernel(const double* __restrict__ e_all, long long e_bs, const int32_t* lens,
                                                             long long n_samples, int S, int last_n, const float* peaks, int n_peaks,
                                                             double* L_out, float* peak_out) {
  __shared__ double red[LG_T];
  __shared__ float pks[LG_T];
  const int b = blockIdx.x, tid = threadIdx.x;
  long long len = n_samples;
  if (lens) {
    const long long L = lens[b];
    len = L < 0 ? 0 : (L > n_samples ? n_samples : L);
  }
  const double* __restrict__ e = e_all + b * e_bs;
  const long long n_sub = (len + S - 1) / S;

  if (peaks) {
    float pk = 0.f;
    for (int i = tid; i < n_peaks; i += LG_T) pk = fmaxf(pk, peaks[(long long)b * n_peaks + i]);
    pks[tid] = pk;
    __syncthreads();
    for (int o = LG_T / 2; o >= 1; o >>= 1) {
      if (tid < o) pks[tid] = fmaxf(pks[tid], pks[tid + o]);
      __syncthreads();
    }
    if (tid == 0 && peak_out) peak_out[b] = pks[0];
  }

  if (last_n > 0) {
    double v = 0.0;
    const long long j_lo = n_sub > last_n ? n_sub - last_n : 0;
    for (long long j = j_lo + tid; j < n_sub; j += LG_T) v += e[j];
    const double z = wg_sum(v, red, tid) / ((double)last_n * (double)S);
    const double l = lufs(z);
    if (tid == 0) L_out[b] = l > LG_ABS ? l : LG_ABS;
    return;
  }

  const long long n_blocks = len <= 0 ? 0 : (len < 4ll * S ? 1 : (len - 4ll * S) / S + 1);
  const double inv = 1.0 / (4.0 * (double)S);
  // pass 1: the absolute gate
  double sum = 0.0, cnt = 0.0;
  for (long long j = tid; j < n_blocks; j += LG_T) {
    double z = e[j];
    if (j + 1 < n_sub) z += e[j + 1];
    if (j + 2 < n_sub) z += e[j + 2];
    if (j + 3 < n_sub) z += e[j + 3];
    z *= inv;
    if (lufs(z) > LG_ABS) sum += z, cnt += 1.0;
  }
  sum = wg_sum(sum, red, tid);
  cnt = wg_sum(cnt, red, tid);
  if (cnt == 0.0) {
    if (tid == 0) L_out[b] = LG_ABS;
    return;
  }
  const double gr = lufs(sum / cnt) - 10.0;
  // pass 2: both gates
  sum = 0.0, cnt = 0.0;
  for (long long j = tid; j < n_blocks; j += LG_T) {
    double z = e[j];
    if (j + 1 < n_sub) z += e[j + 1];
    if (j + 2 < n_sub) z += e[j + 2];
    if (j + 3 < n_sub) z += e[j + 3];
    z *= inv;
    const double l = lufs(z);
    if (l > LG_ABS && l > gr) sum += z, cnt += 1.0;
  }
  sum = wg_sum(sum, red, tid);
  cnt = wg_sum(cnt, red, tid);
  if (tid == 0) {
    const double l = cnt > 0.0 ? lufs(sum / cnt) : LG_ABS;
    L_out[b] = l > LG_ABS ? l : LG_ABS;
  }
}

// ---- gain: store-only behind the clip, one multiply in front of it

constexpr int LN_T = 256, LN_PER = 4;

__global__ __launch_bounds__(LN_T) void loudness_gain_kernel(const float* x_all, long long x_bs, const int32_t* lens, const double* L,
                                                             const float* peak, const double* target_rows, double target, int guard,
                                                             float* y_all, long long y_bs, float* g_out, int T, int vec_ok) {
  __shared__ float g_s;
  const int b = blockIdx.y, tid = threadIdx.x;
  if (tid == 0) {
    const double Lb = L[b];
    const double tg = target_rows ? target_rows[b] : target;
    double g = 1.0;
    if (tg == tg && Lb > LG_ABS) g = pow(10.0, (tg - Lb) / 20.0);
    if (guard) {
      const double pk = (double)peak[b];
      if (g * pk > 1.0) g = 1.0 / pk;
    }
    g_s = (float)g;
    if (g_out && blockIdx.x == 0) g_out[b] = (float)g;
  }
  __syncthreads();
  const float g = g_s;
  const int len = row_len(lens, b, T);
  const float* x = x_all + b * x_bs;
  float* y = y_all + b * y_bs;
  const int t = (blockIdx.x * LN_T + tid) * LN_PER;
  if (t >= T) return;
  if (vec_ok && t + LN_PER <= T) {
    f32x4 v{0.f, 0.f, 0.f, 0.f};
    if (t < len) v = *reinterpret_cast<const f32x4*>(x + t);
    v.x = t < len ? v.x * g : 0.f;
    v.y = t + 1 < len ? v.y * g : 0.f;
    v.z = t + 2 < len ? v.z * g : 0.f;
    v.w = t + 3 < len ? v.w * g : 0.f;
    *reinterpret_cast<f32x4*>(y + t) = v;
  } else {
    for (int i = t; i < T && i < t + LN_PER; ++i) y[i] = i < len ? x[i] * g : 0.f;
  }
}

static void kw_geometry(int T, int* n_chunks, int* n_seg) {
  *n_chunks = (int)(((long long)T + LD_L - 1) / LD_L);
  *n_seg = (*n_chunks + LD_W - 1) / LD_W;
}

}  // namespace fac

using namespace fac;

extern "C" int fac_loudness_chunk(int which) { return which == 0 ? LD_L : LD_W; }

extern "C" int64_t fac_kweight_ws_bytes(int B, int T) {
  if (B <= 0 || T < 0 || T > (1 << 30)) return -1;
  int n_chunks, n_seg;
  kw_geometry(T, &n_chunks, &n_seg);
  const int64_t doubles = (int64_t)B * ((int64_t)n_chunks * 6 + (int64_t)n_seg * 4);
  return doubles * 8 + (((int64_t)B * n_seg * 4 + 7) & ~(int64_t)7) + 8;
}

extern "C" int fac_kweight_energy(const fac_kweight_desc* d, fac_stream_t stream) {
  FAC_REQUIRE(d, "kweight_energy: null descriptor");
  FAC_REQUIRE(d->B >= 1 && d->B <= 65535, "kweight_energy: B = %d outside 1 .. 65535", d->B);
  FAC_REQUIRE(d->S >= 1, "kweight_energy: S = %d samples per sub-block", d->S);
  FAC_REQUIRE(d->S >= LD_L, "kweight_energy: S = %d is below the chunk of %d samples (rates from %d Hz)", d->S, LD_L, 10 * LD_L);
  FAC_REQUIRE(d->T >= 0 && d->T <= (1 << 30), "kweight_energy: T = %d outside 0 .. 2^30", d->T);
  FAC_REQUIRE(d->offset >= 0 && d->offset < d->S, "kweight_energy: offset = %d outside 0 .. S - 1 = %d", d->offset, d->S - 1);
  if (d->T == 0) return FAC_OK;
  FAC_REQUIRE(d->x && d->e && d->ws, "kweight_energy: null pointer (x, e, ws)");
  FAC_REQUIRE(!d->state_out || !d->lens, "kweight_energy: state_out needs lens == NULL");
  FAC_REQUIRE(((uintptr_t)d->ws & 7) == 0, "kweight_energy: ws must be 8-byte aligned");
  KwArgs a;
  a.d = *d;
  kw_geometry(d->T, &a.n_chunks, &a.n_seg);
  a.n_sub = (int)(((long long)d->offset + d->T + d->S - 1) / d->S);
  const long long B = d->B;
  a.ws_state = (double*)d->ws;
  a.ws_seg = a.ws_state + B * a.n_chunks * 4;
  a.ws_part = a.ws_seg + B * a.n_seg * 4;
  a.ws_peak = (float*)(a.ws_part + B * a.n_chunks * 2);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)a.n_seg, (unsigned)d->B);
  if (a.n_chunks > 1) hipLaunchKernelGGL(kweight_kernel<false>, grid, dim3(LD_W), 0, st, a);
  if (a.n_seg > 1) hipLaunchKernelGGL(kweight_scan_kernel, dim3((unsigned)d->B), dim3(LD_SCAN_T), 0, st, a);
  hipLaunchKernelGGL(kweight_kernel<true>, grid, dim3(LD_W), 0, st, a);
  hipLaunchKernelGGL(kweight_reduce_kernel, dim3((unsigned)((a.n_sub + 255) / 256), (unsigned)d->B), dim3(256), 0, st, a);
  return check_launch("kweight_energy");
}

extern "C" int fac_loudness_gate(const double* e, int64_t e_bs, const int32_t* lens, int64_t n_samples, int S, int last_n, const float* peaks,
                                 int n_peaks, double* L_out, float* peak_out, int B, fac_stream_t stream) {
  FAC_REQUIRE(B >= 1, "loudness_gate: B = %d", B);
  FAC_REQUIRE(S >= 1, "loudness_gate: S = %d samples per sub-block", S);
  FAC_REQUIRE(n_samples >= 0, "loudness_gate: negative length n_samples = %lld", (long long)n_samples);
  FAC_REQUIRE(last_n >= 0, "loudness_gate: last_n = %d", last_n);
  FAC_REQUIRE(e && L_out, "loudness_gate: null pointer (e, L_out)");
  FAC_REQUIRE(!peaks == !peak_out && (!peaks || n_peaks >= 1), "loudness_gate: peaks (%d per row) and peak_out come together", n_peaks);
  hipLaunchKernelGGL(loudness_gate_kernel, dim3((unsigned)B), dim3(LG_T), 0, (hipStream_t)stream, e, (long long)e_bs, lens,
                     (long long)n_samples, S, last_n, peaks, n_peaks, L_out, peak_out);
  return check_launch("loudness_gate");
}

extern "C" int fac_loudness_gain(const float* x, int64_t x_bs, const int32_t* lens, const double* L, const float* peak,
                                 const double* target_rows, double target, int guard, float* y, int64_t y_bs, float* g_out, int B, int T,
                                 fac_stream_t stream) {
  FAC_REQUIRE(B >= 1 && B <= 65535, "loudness_gain: B = %d outside 1 .. 65535", B);
  FAC_REQUIRE(T >= 0, "loudness_gain: negative length T = %d", T);
  FAC_REQUIRE(x && y && L, "loudness_gain: null pointer (x, y, L)");
  FAC_REQUIRE(!guard || peak, "loudness_gain: the peak guard needs peak");
  if (T == 0) return FAC_OK;
  const int vec_ok = (((uintptr_t)x | (uintptr_t)y) & 15) == 0 && x_bs % 4 == 0 && y_bs % 4 == 0;
  const unsigned gx = (unsigned)(((long long)T + LN_T * LN_PER - 1) / (LN_T * LN_PER));
  hipLaunchKernelGGL(loudness_gain_kernel, dim3(gx, (unsigned)B), dim3(LN_T), 0, (hipStream_t)stream, x, (long long)x_bs, lens, L, peak,
                     target_rows, target, guard, y, (long long)y_bs, g_out, T, vec_ok);
  return check_launch("loudness_gain");
}
