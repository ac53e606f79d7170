// Level control on the device: fac_agc_gains turns the K-weighted sub-block energies of fac_kweight_energy into one
// gain per completed 100 ms sub-block (the two-gate loudness of a finite window, no recurrence); fac_agc_apply ramps between those
// gains sample by sample, runs a look-ahead peak limiter behind the ramp and carries the last 2 LA gained samples of a stream
// from one carry buffer into the other; fac_true_peak is the maximum over the outputs of fac_resample without the outputs.
// Arithmetic, order and contracts: the header comment of include/facodec_hip.h.  All fp64 on the vector pipe, no matrix pipe, no
// atomics, every word has one writer; the build runs with -ffp-contract=off and the pinned operations are spelled __d*_rn.
#include "common.h"
#include <math.h>

namespace fac {

constexpr int AGC_GT = 64;                       // gains per workgroup of agc_gains_kernel (one thread each)
constexpr int AGC_TILE = 1024;                   // outputs per workgroup of agc_apply_kernel
constexpr int AGC_T = 256;                       // its threads
constexpr int TP_T = 256;                        // threads of the true-peak kernels

// ---- gains

struct AgcGainsArgs {
  fac_agc_gains_desc d;
};

__device__ __forceinline__ double agc_lufs(double z) { return z > 0.0 ? __dadd_rn(-0.691, __dmul_rn(10.0, log10(z))) : -INFINITY; }

// LDS: sub-block g of the tile and its W - 1 older neighbours at e_s[g - lo_t], lo_t = t0 - W + 1 (entries with g < 0 are never read).
__global__ __launch_bounds__(AGC_GT) void agc_gains_kernel(AgcGainsArgs a) {
  __shared__ double e_s[AGC_GT + FAC_AGC_MAX_WINDOW - 1];
  const fac_agc_gains_desc& d = a.d;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int i0 = blockIdx.x * AGC_GT;
  const int n_t = d.n_new - i0 < AGC_GT ? d.n_new - i0 : AGC_GT;
  const long long t0 = d.j0 + i0;
  const long long lo_t = t0 - d.W + 1;
  for (int i = tid; i < n_t + d.W - 1; i += AGC_GT) {
    const long long g = lo_t + i;
    e_s[i] = g >= 0 ? d.e[(long long)b * d.e_bs + g % d.R] : 0.0;
  }
  __syncthreads();
  if (tid >= n_t) return;
  const long long j = t0 + tid;
  const long long js = d.j_start ? (d.j_start[b] > 0 ? d.j_start[b] : 0) : 0;
  bool complete = j >= js;
  if (d.lens) {
    const long long len = d.lens[b];
    complete = complete && (j + 1) * (long long)d.S <= len;
  }
  const long long lo = js > j - d.W + 1 ? js : j - d.W + 1;
  double L = -70.0;
  if (complete && j - lo >= 3) {
    const double* ew = e_s + (lo - lo_t);          // ew[i] = e of sub-block lo + i
    const int nb = (int)(j - lo) - 2;              // gating blocks lo .. j - 3
    const double den = __dmul_rn(4.0, (double)d.S);
    double A = 0.0, nA = 0.0;
    for (int k = 0; k < nb; ++k) {
      const double z = __ddiv_rn(__dadd_rn(__dadd_rn(__dadd_rn(ew[k], ew[k + 1]), ew[k + 2]), ew[k + 3]), den);
      if (agc_lufs(z) > -70.0) A = __dadd_rn(A, z), nA = __dadd_rn(nA, 1.0);
    }
    if (nA > 0.0) {
      const double gr = __dsub_rn(agc_lufs(__ddiv_rn(A, nA)), 10.0);
      double Z = 0.0, nZ = 0.0;
      for (int k = 0; k < nb; ++k) {
        const double z = __ddiv_rn(__dadd_rn(__dadd_rn(__dadd_rn(ew[k], ew[k + 1]), ew[k + 2]), ew[k + 3]), den);
        const double l = agc_lufs(z);
        if (l > -70.0 && l > gr) Z = __dadd_rn(Z, z), nZ = __dadd_rn(nZ, 1.0);
      }
      if (nZ > 0.0) {
        const double l = agc_lufs(__ddiv_rn(Z, nZ));
        L = l > -70.0 ? l : -70.0;
      }
    }
  }
  double G = 0.0;
  if (L > -70.0) {
    G = __dsub_rn(d.target_db, L);
    G = G < -d.max_cut_db ? -d.max_cut_db : G;
    G = G > d.max_boost_db ? d.max_boost_db : G;
  }
  const long long at = (long long)b * d.g_bs + j % d.R;
  if (d.G) d.G[at] = G;
  if (d.g) d.g[at] = pow(10.0, __ddiv_rn(G, 20.0));
}

// ---- apply and limit

struct AgcApplyArgs {
  fac_agc_apply_desc d;
  int n_tiles;
};

// Where block sample r0 >= 0 lies: sub-block jb (and its ring column jm) and position ub, by the one 64-bit division of a
// workgroup; the samples behind it are reached with 32-bit arithmetic.
struct AgcRef {
  long long jb;
  int r0, ub, jm;
};
__device__ __forceinline__ AgcRef agc_ref(const fac_agc_apply_desc& d, int r0) {
  const long long n = d.n0 + r0;
  AgcRef f;
  f.jb = n / d.S;
  f.r0 = r0, f.ub = (int)(n - f.jb * d.S), f.jm = (int)(f.jb % d.R);
  return f;
}

// v of the sample r of the block (r < 0: the carry, r >= -2 LA; r >= 0 needs r >= f.r0), kb = the samples of the block that exist
// in this row
__device__ __forceinline__ double agc_v(const fac_agc_apply_desc& d, int b, int r, int kb, long long js, const AgcRef& f) {
  if (r < 0) return d.carry_in ? d.carry_in[(long long)b * (2 * d.LA) + 2 * d.LA + r] : 0.0;
  if (r >= kb) return 0.0;
  const unsigned off = (unsigned)(f.ub + (r - f.r0));
  const unsigned dj = off / (unsigned)d.S;                           // sub-blocks behind jb: a few at most
  const int u = (int)(off - dj * (unsigned)d.S);
  const long long j = f.jb + dj;
  const int R = d.R;
  const int c1 = (f.jm + (int)(dj % (unsigned)R) + R - 1) % R;       // column (j - 1) % R of g_{j-1}; R <= 2^28 on the host
  const int c2 = (c1 + R - 1) % R;                                   // column (j - 2) % R of g_{j-2}
  const double* grow = d.g + (long long)b * d.g_bs;
  const double g2 = j - 2 >= js ? grow[c2] : 1.0;
  const double g1 = j - 1 >= js ? grow[c1] : 1.0;
  const double frac = __ddiv_rn((double)(u + 1), (double)d.S);
  const double gain = __dadd_rn(g2, __dmul_rn(__dsub_rn(g1, g2), frac));
  return __dmul_rn((double)d.x[(long long)b * d.x_bs + r], gain);
}

// blockIdx.x < n_tiles: outputs i0 .. i0 + cnt - 1 of the row.  LDS: v_s[t], c_s[t] = v, c of block sample i0 - 2 LA + t,
// t < cnt + 2 LA; p_s[u] = p of block sample i0 - LA + 1 + u = min c_s[u + 1 .. u + LA + 1], u < cnt + LA - 1.  Output i0 + i
// (m = n0 + i0 + i) takes v_s[i + LA], c_s[i + LA] and p_s[i .. i + LA - 1].  blockIdx.x == n_tiles: the row's next carry.
__global__ __launch_bounds__(AGC_T) void agc_apply_kernel(AgcApplyArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char agc_lds[];
  const fac_agc_apply_desc& d = a.d;
  const int b = blockIdx.y, tid = threadIdx.x, LA = d.LA;
  int kb = d.k;
  if (d.lens) {
    const int len = d.lens[b];
    kb = len < 0 ? 0 : (len < d.k ? len : d.k);
  }
  const long long js = d.j_start ? (d.j_start[b] > 0 ? d.j_start[b] : 0) : 0;
  if ((int)blockIdx.x == a.n_tiles) {
    if (!d.carry_out) return;
    const AgcRef f = agc_ref(d, d.k > 2 * LA ? d.k - 2 * LA : 0);
    for (int t = tid; t < 2 * LA; t += AGC_T) d.carry_out[(long long)b * (2 * LA) + t] = agc_v(d, b, d.k - 2 * LA + t, kb, js, f);
    return;
  }
  double* v_s = reinterpret_cast<double*>(agc_lds);
  double* c_s = v_s + (AGC_TILE + 2 * LA);
  double* p_s = c_s + (AGC_TILE + 2 * LA);
  const int i0 = blockIdx.x * AGC_TILE;
  const int cnt = d.n_out - i0 < AGC_TILE ? d.n_out - i0 : AGC_TILE;
  const double C = d.ceiling;
  const AgcRef f = agc_ref(d, i0 > 2 * LA ? i0 - 2 * LA : 0);
  int* limited_s = reinterpret_cast<int*>(p_s + (AGC_TILE + LA));    // one word behind p_s: does any c of the tile lie below 1
  if (tid == 0) *limited_s = 0;
  __syncthreads();
  int limited = 0;
  for (int t = tid; t < cnt + 2 * LA; t += AGC_T) {
    const double v = agc_v(d, b, i0 - 2 * LA + t, kb, js, f);
    const double m = fabs(v);
    const double c = m > C ? __ddiv_rn(C, m) : 1.0;
    v_s[t] = v, c_s[t] = c;
    limited |= c < 1.0;
  }
  if (limited) *limited_s = 1;                                        // every writer stores the same value
  __syncthreads();
  float* yrow = d.y + (long long)b * d.y_bs + i0;
  if (!*limited_s) {                                                  // every c is 1: p = 1, the mean is LA / LA = 1, s = 1
    for (int i = tid; i < cnt; i += AGC_T) yrow[i] = (float)v_s[i + LA];
    return;
  }
  for (int u = tid; u < cnt + LA - 1; u += AGC_T) {
    double p = c_s[u + 1];
    for (int w = 2; w <= LA + 1; ++w) p = fmin(p, c_s[u + w]);
    p_s[u] = p;
  }
  __syncthreads();
  const double den = (double)LA;
  for (int i = tid; i < cnt; i += AGC_T) {
    double sum = p_s[i];
    for (int w = 1; w < LA; ++w) sum = __dadd_rn(sum, p_s[i + w]);
    const double s = fmin(__ddiv_rn(sum, den), c_s[i + LA]);
    yrow[i] = (float)__dmul_rn(v_s[i + LA], s);
  }
}

static size_t agc_apply_lds(int LA) { return ((size_t)2 * (AGC_TILE + 2 * LA) + (size_t)(AGC_TILE + LA) + 1) * sizeof(double); }

// ---- true peak

struct TruePeakArgs {
  fac_resample_desc d;
  float* ws;
  int tm, span_cap, n_tiles, ts;
};

__device__ __forceinline__ float tp_fetch(const float* __restrict__ xrow, int r, int Lb) { return r >= 0 && r < Lb ? xrow[r] : 0.f; }

// One workgroup per (row, tile of tm outputs): the contiguous input span the tile reads staged in LDS (what lies outside the
// row's signal as 0), fac_resample's dot product per output, the tile's max |y| by a tree in LDS.  TAB_LDS: the coefficient
// table sits in LDS in front of the span, rows at the odd pitch ts (lanes hold consecutive phases, i.e. rows); else it is read
// from global memory (a table too big to sit beside the span).
template <bool TAB_LDS>
__global__ __launch_bounds__(TP_T) void true_peak_kernel(TruePeakArgs a) {
  extern __shared__ float tp_lds[];
  __shared__ float red[TP_T];
  const fac_resample_desc& d = a.d;
  const int b = blockIdx.y, tid = threadIdx.x, tile = blockIdx.x;
  const int o = d.o, n = d.n, taps = d.taps;
  int Lb = d.T;
  if (d.lens) {
    const int L = d.lens[b];
    Lb = L < 0 ? 0 : (L > d.T ? d.T : L);
  }
  const float* __restrict__ xrow = d.x + b * d.x_bs;
  const long long m_end = ((long long)Lb * n + o - 1) / o;
  const int m0 = tile * a.tm;
  const int cnt = min(a.tm, d.n_out - m0);
  if (cnt <= 0) {                                                     // n_out = 0: the one tile of an empty signal
    if (tid == 0) a.ws[(long long)b * a.n_tiles + tile] = 0.f;
    return;
  }
  const int k0 = m0 / n, p0 = m0 - k0 * n;
  const int base = k0 * o;
  const int r_lo = base + d.offs[p0];
  const int ppl = p0 + cnt - 1, dkl = ppl / n;
  int span = base + dkl * o + d.offs[ppl - dkl * n] + taps - r_lo;
  span = span < 0 ? 0 : (span > a.span_cap ? a.span_cap : span);
  float* tp_xs = tp_lds + (TAB_LDS ? n * a.ts : 0);
  if (TAB_LDS) {
    for (int idx = tid; idx < n * taps; idx += TP_T) {
      const int r = idx / taps;
      tp_lds[r * a.ts + (idx - r * taps)] = d.table[idx];
    }
  }
  for (int idx = tid; idx < span; idx += TP_T) tp_xs[idx] = tp_fetch(xrow, r_lo + idx, Lb);
  __syncthreads();
  float pk = 0.f;
  for (int ii = tid; ii < cnt; ii += TP_T) {
    if (m0 + ii >= m_end) continue;
    const int pp = p0 + ii, dk = pp / n, p = pp - dk * n;
    const int rf = base + dk * o + d.offs[p];
    const float* __restrict__ c = TAB_LDS ? tp_lds + p * a.ts : d.table + (long long)p * taps;
    const int s = rf - r_lo;
    float acc = 0.f;
    if (s >= 0 && s + taps <= span) {
#pragma unroll 4
      for (int j = 0; j < taps; ++j) acc = fmaf(c[j], tp_xs[s + j], acc);
    } else {
      for (int j = 0; j < taps; ++j) acc = fmaf(c[j], tp_fetch(xrow, rf + j, Lb), acc);
    }
    pk = fmaxf(pk, fabsf(acc));
  }
  red[tid] = pk;
  __syncthreads();
  for (int w = TP_T / 2; w >= 1; w >>= 1) {
    if (tid < w) red[tid] = fmaxf(red[tid], red[tid + w]);
    __syncthreads();
  }
  if (tid == 0) a.ws[(long long)b * a.n_tiles + tile] = red[0];
}

__global__ __launch_bounds__(TP_T) void true_peak_reduce_kernel(const float* __restrict__ ws, int n_tiles, float* peak) {
  __shared__ float red[TP_T];
  const int b = blockIdx.x, tid = threadIdx.x;
  float pk = 0.f;
  for (int i = tid; i < n_tiles; i += TP_T) pk = fmaxf(pk, ws[(long long)b * n_tiles + i]);
  red[tid] = pk;
  __syncthreads();
  for (int w = TP_T / 2; w >= 1; w >>= 1) {
    if (tid < w) red[tid] = fmaxf(red[tid], red[tid + w]);
    __syncthreads();
  }
  if (tid == 0) peak[b] = red[0];
}

constexpr int TP_TILE = 1024;
static int tp_tiles(int n_out) { return n_out <= 0 ? 1 : (n_out + TP_TILE - 1) / TP_TILE; }

}  // namespace fac

using namespace fac;

extern "C" int fac_agc_gains(const fac_agc_gains_desc* d, fac_stream_t stream) {
  FAC_REQUIRE(d, "agc_gains: null descriptor");
  FAC_REQUIRE(d->e, "agc_gains: null energy pointer");
  FAC_REQUIRE(d->G || d->g, "agc_gains: neither G nor g to write");
  FAC_REQUIRE(d->B > 0 && d->B <= 65535, "agc_gains: B = %d outside 1 .. 65535", d->B);
  FAC_REQUIRE(d->n_new >= 1, "agc_gains: n_new = %d (at least one sub-block)", d->n_new);
  FAC_REQUIRE(d->W >= 4 && d->W <= FAC_AGC_MAX_WINDOW, "agc_gains: window = %d outside 4 .. %d sub-blocks", d->W, (int)FAC_AGC_MAX_WINDOW);
  FAC_REQUIRE(d->S >= 1, "agc_gains: S = %d samples per sub-block", d->S);
  FAC_REQUIRE(d->j0 >= 0, "agc_gains: j0 = %lld is negative", (long long)d->j0);
  FAC_REQUIRE(isfinite(d->target_db), "agc_gains: target_db = %g is not finite", d->target_db);
  FAC_REQUIRE(isfinite(d->max_boost_db) && d->max_boost_db >= 0.0 && isfinite(d->max_cut_db) && d->max_cut_db >= 0.0,
              "agc_gains: max_boost_db = %g, max_cut_db = %g (finite, not negative)", d->max_boost_db, d->max_cut_db);
  // nothing older than sub-block j0 + n_new - R is in the ring any more; a gain's window reaches W - 1 sub-blocks back
  const long long seen = d->j0 + d->n_new, need = (long long)d->W + d->n_new - 1;
  FAC_REQUIRE(d->R >= 1 && d->R >= (seen < need ? seen : need), "agc_gains: R = %d below W + n_new - 1 = %d + %d - 1", d->R, d->W, d->n_new);
  FAC_REQUIRE(d->e_bs >= d->R || d->B == 1, "agc_gains: e_bs = %lld below R = %d", (long long)d->e_bs, d->R);
  FAC_REQUIRE(d->g_bs >= d->R || d->B == 1, "agc_gains: g_bs = %lld below R = %d", (long long)d->g_bs, d->R);
  AgcGainsArgs a;
  a.d = *d;
  hipLaunchKernelGGL(agc_gains_kernel, dim3((unsigned)((d->n_new + AGC_GT - 1) / AGC_GT), (unsigned)d->B), dim3(AGC_GT), 0,
                     (hipStream_t)stream, a);
  return check_launch("agc_gains");
}

extern "C" int fac_agc_apply(const fac_agc_apply_desc* d, fac_stream_t stream) {
  FAC_REQUIRE(d, "agc_apply: null descriptor");
  FAC_REQUIRE(d->g && d->y, "agc_apply: null gain or output pointer");
  FAC_REQUIRE(d->B > 0 && d->B <= 65535, "agc_apply: B = %d outside 1 .. 65535", d->B);
  FAC_REQUIRE(d->k >= 0 && d->k <= (1 << 30), "agc_apply: k = %d outside 0 .. 2^30 samples", d->k);
  FAC_REQUIRE(d->x || d->k == 0, "agc_apply: null block pointer with k = %d", d->k);
  FAC_REQUIRE(d->LA >= 1 && d->LA <= FAC_AGC_MAX_LOOKAHEAD, "agc_apply: LA = %d outside 1 .. %d samples", d->LA, (int)FAC_AGC_MAX_LOOKAHEAD);
  FAC_REQUIRE(d->n_out >= 1 && d->n_out >= d->k && (long long)d->n_out <= (long long)d->k + d->LA,
              "agc_apply: n_out = %d outside max(k, 1) .. k + LA = %d + %d", d->n_out, d->k, d->LA);
  FAC_REQUIRE(d->S >= 1 && d->S <= (1 << 30), "agc_apply: S = %d samples per sub-block (1 .. 2^30)", d->S);
  FAC_REQUIRE(d->ceiling > 0.0 && isfinite(d->ceiling), "agc_apply: ceiling = %g (linear, above 0)", d->ceiling);
  FAC_REQUIRE(d->n0 >= 0, "agc_apply: n0 = %lld is negative", (long long)d->n0);
  FAC_REQUIRE(!d->carry_out || d->carry_out != d->carry_in, "agc_apply: carry_out is carry_in (the two buffers ping-pong)");
  FAC_REQUIRE(!d->lens || (!d->carry_in && !d->carry_out), "agc_apply: lens does not go with a carried stream");
  FAC_REQUIRE(d->x_bs >= d->k || d->B == 1, "agc_apply: x_bs = %lld below k = %d", (long long)d->x_bs, d->k);
  FAC_REQUIRE(d->y_bs >= d->n_out || d->B == 1, "agc_apply: y_bs = %lld below n_out = %d", (long long)d->y_bs, d->n_out);
  FAC_REQUIRE(d->R >= 1 && d->R <= (1 << 28), "agc_apply: R = %d outside 1 .. 2^28", d->R);
  if (d->k > 0) {
    // the block reads g of sub-blocks jf - 2 .. jl - 1: they must sit in different columns (that the ring still holds them is
    // the business of whoever writes it)
    const long long jf = d->n0 / d->S, jl = (d->n0 + d->k - 1) / d->S;
    const long long held = jl, reach = jl - jf + 2;
    FAC_REQUIRE(d->R >= (held < reach ? held : reach), "agc_apply: R = %d below the %lld gains the block reaches", d->R,
                (long long)(held < reach ? held : reach));
  }
  FAC_REQUIRE(d->g_bs >= d->R || d->B == 1, "agc_apply: g_bs = %lld below R = %d", (long long)d->g_bs, d->R);
  AgcApplyArgs a;
  a.d = *d;
  a.n_tiles = (d->n_out + AGC_TILE - 1) / AGC_TILE;
  allow_dynamic_lds<agc_apply_kernel>();                               // 64 KB and a word at LA = 1024; the kernel has no static LDS
  hipLaunchKernelGGL(agc_apply_kernel, dim3((unsigned)(a.n_tiles + (d->carry_out ? 1 : 0)), (unsigned)d->B), dim3(AGC_T),
                     agc_apply_lds(d->LA), (hipStream_t)stream, a);
  return check_launch("agc_apply");
}

extern "C" int64_t fac_true_peak_ws_bytes(int B, int n_out) {
  if (B <= 0 || n_out < 0) return -1;
  return (int64_t)B * tp_tiles(n_out) * (int64_t)sizeof(float);
}

extern "C" int fac_true_peak(const fac_resample_desc* d, float* peak, void* ws, fac_stream_t stream) {
  FAC_REQUIRE(d, "true_peak: null descriptor");
  FAC_REQUIRE(d->x && d->table && d->offs && peak && ws, "true_peak: null pointer (x, table, offs, peak, ws)");
  FAC_REQUIRE(!d->hist && !d->hist_out && d->n_hist == 0 && d->q0 == 0 && d->m_lo == 0, "true_peak: the offline form only (no history, q0 = m_lo = 0)");
  FAC_REQUIRE(d->o >= 1 && d->o <= 640 && d->n >= 1 && d->n <= 640, "true_peak: o = %d, n = %d outside 1 .. 640", d->o, d->n);
  FAC_REQUIRE(d->taps >= 1 && (long long)d->taps * d->n < (1 << 28), "true_peak: bad table geometry (n = %d, taps = %d)", d->n, d->taps);
  FAC_REQUIRE(d->B >= 1 && d->B <= 65535 && d->T >= 0 && d->n_out >= 0, "true_peak: bad sizes (B = %d, T = %d, n_out = %d)", d->B, d->T, d->n_out);
  FAC_REQUIRE(d->x_bs >= d->T || d->B == 1, "true_peak: x_bs = %lld below T = %d", (long long)d->x_bs, d->T);
  FAC_REQUIRE((long long)d->T + ((long long)d->n_out / d->n + 2) * d->o + d->taps < (1ll << 30), "true_peak: the launch spans more than 2^30 samples");
  TruePeakArgs a;
  a.d = *d;
  a.ws = (float*)ws;
  a.tm = TP_TILE;
  a.n_tiles = tp_tiles(d->n_out);
  a.span_cap = (int)(((long long)(a.tm - 1) * d->o + d->n - 1) / d->n) + d->taps + 2;
  FAC_REQUIRE((size_t)a.span_cap * sizeof(float) <= 48 * 1024, "true_peak: o / n = %d / %d with %d taps needs a span of %d samples per tile (12288 at most)",
              d->o, d->n, d->taps, a.span_cap);
  a.ts = d->taps | 1;
  const size_t span_b = (size_t)a.span_cap * sizeof(float), tab_b = (size_t)d->n * a.ts * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)a.n_tiles, (unsigned)d->B);
  if (tab_b + span_b <= 60 * 1024) hipLaunchKernelGGL(true_peak_kernel<true>, grid, dim3(TP_T), tab_b + span_b, st, a);   // + 1 KB static
  else hipLaunchKernelGGL(true_peak_kernel<false>, grid, dim3(TP_T), span_b, st, a);
  hipLaunchKernelGGL(true_peak_reduce_kernel, dim3((unsigned)d->B), dim3(TP_T), 0, st, a.ws, a.n_tiles, peak);
  return check_launch("true_peak");
}
