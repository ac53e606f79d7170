// Noise suppression on the device: a spectral suppressor on 512-sample sine-windowed frames at a hop of 256.
// fac_ns_power transforms the frames a block completes and writes their power spectra into a ring; fac_ns_gains turns the ring
// into one gain per frame and bin (a finite mean, a finite minimum, a Wiener-shaped rule; no recurrence); fac_ns_synth transforms
// the two frames that overlap every output segment again, masks them, transforms back, windows and adds.  Arithmetic, order and
// contracts: the header comment of include/facodec_hip.h.  All fp64 on the vector pipe, no matrix pipe, no atomics, every word
// has one writer; the build runs with -ffp-contract=off.
//
// The transform is fft512_f64.h's: one wave per frame, four frames per 256-thread workgroup, a 512-entry double2 buffer per
// wave, transformed in place (bin k ends at the bit-reversed index; the inverse starts from that order).  A wave's buffer is
// private to it while it transforms, so the stages are ordered inside the wave and a wave without a frame skips the transform;
// workgroup barriers stand only where waves exchange data: behind the tables, and around the synthesis kernel's overlap-add.
// The input is a StreamSrc (stream_src.h) over [carry | block] with a carry of NS_CARRY samples.
#include "common.h"
#include "fft512_f64.h"
#include "stream_src.h"
#include <math.h>

namespace fac {

constexpr int NS_T = 256;                          // threads of every kernel here
constexpr int NS_N = FAC_NS_N, NS_H = FAC_NS_H, NS_BINS = FAC_NS_BINS, NS_CARRY = FAC_NS_CARRY;
constexpr int NS_PF = 16;                          // frames per workgroup of the power kernel (4 rounds of 4 waves)
constexpr int NS_SF = 16;                          // frames per workgroup of the synthesis kernel: NS_SF - 1 segments
constexpr int NS_GF = 64, NS_GK = 16, NS_GQ = 4;   // the gain kernel's tile: frames x bins; consecutive frames per thread
static_assert(NS_GF == (NS_T / NS_GK) * NS_GQ, "one thread per (bin, four frames) of the tile");
static_assert(NS_N == 2 * NS_H && NS_BINS == NS_H + 1 && NS_CARRY == 2 * NS_N - 1, "noise suppressor geometry");

static_assert(NS_N == FFT512_N && NS_T == FFT512_N / 2, "one thread per twiddle and per two window entries");

// win[n] = sin(pi n / 512)
__device__ __forceinline__ void ns_window(double* win, int tid) {
  win[tid] = sinpi((double)tid / (double)NS_N);
  win[tid + NS_T] = sinpi((double)(tid + NS_T) / (double)NS_N);
}

// z[n] = (w[n] * sample((f - 1) H + n), 0)
__device__ __forceinline__ void ns_load(double2* z, const double* win, const StreamSrc& src, long long f, int lane) {
  const long long base = (f - 1) * NS_H;
#pragma unroll
  for (int r = 0; r < NS_N / 64; ++r) {
    const int n = lane + 64 * r;
    z[n] = make_double2(win[n] * (double)src.sample(base + n), 0.0);
  }
}

// ---- power

struct NsPowerArgs {
  fac_ns_power_desc d;
  int n_tiles;
};

// blockIdx.x < n_tiles: frames f0 + 16 blockIdx.x .. of the row, wave w of round i takes frame 4 i + w.  blockIdx.x == n_tiles:
// the row's next carry.
__global__ __launch_bounds__(NS_T) void ns_power_kernel(NsPowerArgs a) {
  __shared__ double2 buf[4][NS_N];
  __shared__ double2 tw[NS_N / 2];
  __shared__ double win[NS_N];
  const fac_ns_power_desc& d = a.d;
  const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const StreamSrc src = stream_src(d.carry_in, NS_CARRY, d.x, d.x_bs, d.lens, d.starts, d.n0, d.k, b);
  if ((int)blockIdx.x == a.n_tiles) {
    stream_carry_out(src, d.carry_out, d.k, b, tid, NS_T);
    return;
  }
  fft512_table(tw, tid);
  ns_window(win, tid);
  __syncthreads();                                     // the tables: written by all four waves, read by each
  const int i0 = blockIdx.x * NS_PF;
  const int n_t = d.n_new - i0 < NS_PF ? d.n_new - i0 : NS_PF;
  double2* z = buf[wave];
  // no wave reads another's buffer: no workgroup barrier in this loop, and its trip count is the wave's own
  for (int i = wave; i < n_t; i += 4) {
    const long long f = d.f0 + i0 + i;
    ns_load(z, win, src, f, lane);
    fft512_forward(z, tw, lane);
    const long long at = (long long)b * d.p_bs + (f % d.R) * NS_BINS;
    for (int k = lane; k < NS_BINS; k += 64) {
      const double2 v = z[fft512_rev(k)];
      d.P[at + k] = v.x * v.x + v.y * v.y;
      if (d.X) reinterpret_cast<double2*>(d.X)[at + k] = v;
    }
    fft512_wave_sync();                                // the lanes have read the spectrum before the next frame overwrites it
  }
}

// ---- gains

struct NsGainsArgs {
  fac_ns_gains_desc d;
};

// LDS: P of frame g at p_s[(g - lo_t) * NS_GK + kb], lo_t = t0 - (M + W - 2); S of frame g at s_s[(g - (t0 - W + 1)) * NS_GK + kb].
// Frames before the row's first are never read.
__global__ __launch_bounds__(NS_T) void ns_gains_kernel(NsGainsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ns_lds[];
  const fac_ns_gains_desc& d = a.d;
  const int b = blockIdx.z, tid = threadIdx.x;
  const int kb = tid & (NS_GK - 1), row = tid / NS_GK;
  constexpr int ROWS = NS_T / NS_GK;
  const int k = blockIdx.y * NS_GK + kb;
  const bool bin = k < NS_BINS;
  const int i0 = blockIdx.x * NS_GF;
  const int n_t = d.n_new - i0 < NS_GF ? d.n_new - i0 : NS_GF;
  const int M = d.M, W = d.W;
  const long long t0 = d.f0 + i0;
  const long long lo_t = t0 - (M + W - 2), lo_s = t0 - (W - 1);
  long long fs = d.starts ? (d.starts[b] > 0 ? d.starts[b] : 0) / NS_H : 0;
  double* p_s = reinterpret_cast<double*>(ns_lds);
  double* s_s = p_s + (NS_GF + M + W - 2) * NS_GK;
  const double* Prow = d.P + (long long)b * d.p_bs;
  for (int i = row; i < n_t + M + W - 2; i += ROWS) {
    const long long g = lo_t + i;
    p_s[i * NS_GK + kb] = (bin && g >= fs) ? Prow[(g % d.R) * NS_BINS + k] : 0.0;
  }
  __syncthreads();
  for (int i = row; i < n_t + W - 1; i += ROWS) {
    const long long g = lo_s + i;
    double S = 0.0;
    if (g >= fs) {
      const long long lo = fs > g - M + 1 ? fs : g - M + 1;
      const double* pp = p_s + (lo - lo_t) * NS_GK + kb;
      const int cnt = (int)(g - lo) + 1;
      S = pp[0];
      for (int h = 1; h < cnt; ++h) S = __dadd_rn(S, pp[h * NS_GK]);
      S = __ddiv_rn(S, (double)cnt);
    }
    s_s[i * NS_GK + kb] = S;
  }
  __syncthreads();
  // One thread per (bin, NS_GQ consecutive frames fa .. fa + 3): the S all four windows share, [c_lo, fa], is read once (the
  // minimum is exact in any order), every frame then adds the few S on either side that are its own: 105 LDS reads for four
  // gains at W = 96 where one window each would take 384.
  const int ia = row * NS_GQ;
  if (ia >= n_t) return;
  const long long fa = t0 + ia;
  const long long c_far = fa + NS_GQ - W;                              // the first frame of the last window, not truncated
  const long long c_lo = fs > c_far ? fs : c_far;
  const bool shared = fa >= fs && c_lo <= fa;
  double common = INFINITY;
  if (shared) {
    const double* sp = s_s + (c_lo - lo_s) * NS_GK + kb;
    const int cnt = (int)(fa - c_lo) + 1;
    double n0 = sp[0], n1 = n0, n2 = n0, n3 = n0;                      // four chains keep four LDS reads in flight
    int h = 1;
    for (; h + 3 < cnt; h += 4) {
      n0 = fmin(n0, sp[h * NS_GK]), n1 = fmin(n1, sp[(h + 1) * NS_GK]);
      n2 = fmin(n2, sp[(h + 2) * NS_GK]), n3 = fmin(n3, sp[(h + 3) * NS_GK]);
    }
    for (; h < cnt; ++h) n0 = fmin(n0, sp[h * NS_GK]);
    common = fmin(fmin(n0, n1), fmin(n2, n3));
  }
  const double* sk = s_s + kb;                                         // S of frame g: sk[(g - lo_s) * NS_GK]
  for (int j = 0; j < NS_GQ && ia + j < n_t; ++j) {
    const long long f = fa + j;
    double G = 1.0;
    if (f >= fs) {
      const long long lo = fs > f - W + 1 ? fs : f - W + 1;
      double Nf = common;
      if (shared) {
        for (long long g = lo; g < c_lo; ++g) Nf = fmin(Nf, sk[(g - lo_s) * NS_GK]);
        for (long long g = fa + 1; g <= f; ++g) Nf = fmin(Nf, sk[(g - lo_s) * NS_GK]);
      } else {
        Nf = sk[(lo - lo_s) * NS_GK];
        for (long long g = lo + 1; g <= f; ++g) Nf = fmin(Nf, sk[(g - lo_s) * NS_GK]);
      }
      if (Nf != 0.0) {
        const double S = sk[(f - lo_s) * NS_GK];
        double xi = __dsub_rn(__ddiv_rn(S, __dmul_rn(d.over, Nf)), 1.0);
        xi = xi > 0.0 ? xi : 0.0;
        G = __ddiv_rn(xi, __dadd_rn(1.0, xi));
        G = G > d.g_min ? G : d.g_min;
      }
    }
    if (bin) d.G[(long long)b * d.g_bs + (f % d.R) * NS_BINS + k] = G;
  }
}

// 41.6 KB at the defaults (M = 8, W = 96), 89.7 KB at the largest windows
static size_t ns_gains_lds(int M, int W) { return (size_t)(2 * NS_GF + M + 2 * W - 3) * NS_GK * sizeof(double); }

// ---- synthesis

struct NsSynthArgs {
  fac_ns_synth_desc d;
  long long s_first, s_last;                         // the segments the outputs lie in
};

// Workgroup c of a row takes segments s0 = s_first + 15 c .. min(s0 + 14, s_last), that is frames s0 .. s_end + 1: wave w of
// round i computes v of frame s0 + 4 i + w into the real parts of its buffer; segment f - 1 is then the second half of the
// frame before (the wave before's buffer, or prev[] from the round before) plus the first half of v_f.
__global__ __launch_bounds__(NS_T) void ns_synth_kernel(NsSynthArgs a) {
  __shared__ double2 buf[4][NS_N];
  __shared__ double2 tw[NS_N / 2];
  __shared__ double win[NS_N];
  __shared__ double prev[NS_H];
  const fac_ns_synth_desc& d = a.d;
  const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const StreamSrc src = stream_src(d.carry_in, NS_CARRY, d.x, d.x_bs, d.lens, d.starts, d.n0, d.k, b);
  const long long fs = src.start / NS_H;
  const long long s0 = a.s_first + (long long)blockIdx.x * (NS_SF - 1);
  const long long s_end = s0 + NS_SF - 2 < a.s_last ? s0 + NS_SF - 2 : a.s_last;
  const int n_f = (int)(s_end - s0) + 2;             // frames s0 .. s_end + 1
  fft512_table(tw, tid);
  ns_window(win, tid);
  __syncthreads();                                     // the tables: written by all four waves, read by each
  double2* z = buf[wave];
  float* yrow = d.y + (long long)b * d.y_bs;
  for (int it = 0; it * 4 < n_f; ++it) {               // two workgroup barriers per round: the trip count is the workgroup's
    const bool valid = it * 4 + wave < n_f;            // wave-uniform
    const long long f = s0 + it * 4 + wave;
    const bool live = valid && f >= fs;                // f >= fs >= 0: a frame of the row's current stream
    const long long gat = (long long)b * d.g_bs + (live ? f % d.R : 0) * NS_BINS;
    if (live) {                                        // the wave alone in its buffer
      if (!d.X) {
        ns_load(z, win, src, f, lane);
        fft512_forward(z, tw, lane);
      }
      // Y[k] = G[k] X[k], k = 0 .. 256; Y[512 - k] = conj(Y[k]), k = 1 .. 255
      for (int k = lane; k < NS_BINS; k += 64) {
        const double2 v = d.X ? reinterpret_cast<const double2*>(d.X)[gat + k] : z[fft512_rev(k)];
        const double g = d.G[gat + k];
        const double2 y = make_double2(g * v.x, g * v.y);
        z[fft512_rev(k)] = y;
        if (k >= 1 && k < NS_H) z[fft512_rev(NS_N - k)] = make_double2(y.x, -y.y);
      }
      fft512_inverse(z, tw, lane);
    }
    if (valid) {
#pragma unroll
      for (int r = 0; r < NS_N / 64; ++r) {
        const int n = lane + 64 * r;
        z[n].x = live ? win[n] * (z[n].x * (1.0 / NS_N)) : 0.0;
      }
    }
    __syncthreads();                                   // every wave's v_f, and prev[] of the round before, for the overlap-add
    if (valid && it * 4 + wave > 0) {                  // segment f - 1 >= s0
      const long long mb = (f - 1) * NS_H;
#pragma unroll
      for (int r = 0; r < NS_H / 64; ++r) {
        const int j = lane + 64 * r;
        const long long m = mb + j, i = m - d.m0;
        if (i >= 0 && i < d.n_out) {
          const double older = wave > 0 ? buf[wave - 1][NS_H + j].x : prev[j];
          const double v = older + z[j].x;
          yrow[i] = (m < src.start || m >= src.end) ? 0.f : (float)v;
        }
      }
    }
    // the overlap-add has read prev[] and the neighbours' buffers: wave 3 may overwrite prev[], the next round the buffers
    __syncthreads();
    if (wave == 3) {
#pragma unroll
      for (int r = 0; r < NS_H / 64; ++r) prev[lane + 64 * r] = z[NS_H + lane + 64 * r].x;
      fft512_wave_sync();                              // read by its lanes before the next round's spectrum goes into z
    }
  }
}

}  // namespace fac

using namespace fac;

static long long ns_fdiv(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

extern "C" int fac_ns_power(const fac_ns_power_desc* d, fac_stream_t stream) {
  FAC_REQUIRE(d, "ns_power: null descriptor");
  FAC_REQUIRE(d->P, "ns_power: null power pointer");
  FAC_REQUIRE(d->B > 0 && d->B <= 65535, "ns_power: B = %d outside 1 .. 65535", d->B);
  FAC_REQUIRE(d->k >= 0 && d->k <= (1 << 30), "ns_power: k = %d outside 0 .. 2^30 samples", d->k);
  FAC_REQUIRE(d->x || d->k == 0, "ns_power: null block pointer with k = %d", d->k);
  FAC_REQUIRE(d->n_new >= 0 && (d->n_new > 0 || d->carry_out), "ns_power: n_new = %d and no carry to write: nothing to do", d->n_new);
  FAC_REQUIRE(d->n0 >= 0 && d->f0 >= 0, "ns_power: n0 = %lld, f0 = %lld (not negative)", (long long)d->n0, (long long)d->f0);
  FAC_REQUIRE(!d->carry_out || d->carry_out != d->carry_in, "ns_power: carry_out is carry_in (the two buffers ping-pong)");
  FAC_REQUIRE(!d->lens || (!d->carry_in && !d->carry_out), "ns_power: lens does not go with a carried stream");
  FAC_REQUIRE(d->x_bs >= d->k || d->B == 1, "ns_power: x_bs = %lld below k = %d", (long long)d->x_bs, d->k);
  // the frames of the call must not reach in front of the carry: frame f0 starts at sample (f0 - 1) H
  FAC_REQUIRE(d->n_new == 0 || !d->carry_in || (d->f0 - 1) * (long long)FAC_NS_H >= d->n0 - FAC_NS_CARRY,
              "ns_power: frame f0 = %lld starts more than %d samples in front of n0 = %lld", (long long)d->f0, (int)FAC_NS_CARRY, (long long)d->n0);
  FAC_REQUIRE(d->R >= 1 && d->R <= (1 << 22) && d->R >= d->n_new, "ns_power: R = %d below n_new = %d (or above 2^22)", d->R, d->n_new);
  FAC_REQUIRE(d->p_bs >= (long long)d->R * FAC_NS_BINS || d->B == 1, "ns_power: p_bs = %lld below R * 257 = %lld", (long long)d->p_bs,
              (long long)d->R * FAC_NS_BINS);
  NsPowerArgs a;
  a.d = *d;
  a.n_tiles = (d->n_new + NS_PF - 1) / NS_PF;
  hipLaunchKernelGGL(ns_power_kernel, dim3((unsigned)(a.n_tiles + (d->carry_out ? 1 : 0)), (unsigned)d->B), dim3(NS_T), 0,
                     (hipStream_t)stream, a);
  return check_launch("ns_power");
}

extern "C" int fac_ns_gains(const fac_ns_gains_desc* d, fac_stream_t stream) {
  FAC_REQUIRE(d, "ns_gains: null descriptor");
  FAC_REQUIRE(d->P && d->G, "ns_gains: null power or gain pointer");
  FAC_REQUIRE(d->B > 0 && d->B <= 65535, "ns_gains: B = %d outside 1 .. 65535", d->B);
  FAC_REQUIRE(d->n_new >= 1, "ns_gains: n_new = %d (at least one frame)", d->n_new);
  FAC_REQUIRE(d->M >= 1 && d->M <= FAC_NS_MAX_M, "ns_gains: M = %d outside 1 .. %d frames", d->M, (int)FAC_NS_MAX_M);
  FAC_REQUIRE(d->W >= 1 && d->W <= FAC_NS_MAX_W, "ns_gains: W = %d outside 1 .. %d frames", d->W, (int)FAC_NS_MAX_W);
  FAC_REQUIRE(d->over > 0.0 && isfinite(d->over), "ns_gains: over = %g (finite, above 0)", d->over);
  FAC_REQUIRE(d->g_min > 0.0 && d->g_min <= 1.0, "ns_gains: g_min = %g outside (0, 1] (max_atten_db is not negative)", d->g_min);
  FAC_REQUIRE(d->f0 >= 0, "ns_gains: f0 = %lld is negative", (long long)d->f0);
  // nothing older than frame f0 + n_new - R is in the ring any more; a gain reaches M + W - 2 frames back
  const long long seen = d->f0 + d->n_new, need = (long long)d->M + d->W - 2 + d->n_new;
  FAC_REQUIRE(d->R >= 1 && d->R <= (1 << 22) && d->R >= (seen < need ? seen : need), "ns_gains: R = %d below M + W - 2 + n_new = %d + %d - 2 + %d", d->R,
              d->M, d->W, d->n_new);
  FAC_REQUIRE(d->p_bs >= (long long)d->R * FAC_NS_BINS || d->B == 1, "ns_gains: p_bs = %lld below R * 257", (long long)d->p_bs);
  FAC_REQUIRE(d->g_bs >= (long long)d->R * FAC_NS_BINS || d->B == 1, "ns_gains: g_bs = %lld below R * 257", (long long)d->g_bs);
  NsGainsArgs a;
  a.d = *d;
  allow_dynamic_lds<ns_gains_kernel>();
  hipLaunchKernelGGL(ns_gains_kernel, dim3((unsigned)((d->n_new + NS_GF - 1) / NS_GF), (unsigned)((NS_BINS + NS_GK - 1) / NS_GK), (unsigned)d->B),
                     dim3(NS_T), ns_gains_lds(d->M, d->W), (hipStream_t)stream, a);
  return check_launch("ns_gains");
}

extern "C" int fac_ns_synth(const fac_ns_synth_desc* d, fac_stream_t stream) {
  FAC_REQUIRE(d, "ns_synth: null descriptor");
  FAC_REQUIRE(d->G && d->y, "ns_synth: null gain or output pointer");
  FAC_REQUIRE(d->B > 0 && d->B <= 65535, "ns_synth: B = %d outside 1 .. 65535", d->B);
  FAC_REQUIRE(d->k >= 0 && d->k <= (1 << 30), "ns_synth: k = %d outside 0 .. 2^30 samples", d->k);
  FAC_REQUIRE(d->x || d->k == 0 || d->X, "ns_synth: null block pointer with k = %d", d->k);
  FAC_REQUIRE(d->n_out >= 1 && d->n_out <= (1 << 30), "ns_synth: n_out = %d outside 1 .. 2^30", d->n_out);
  FAC_REQUIRE(d->n0 >= 0, "ns_synth: n0 = %lld is negative", (long long)d->n0);
  FAC_REQUIRE(!d->lens || !d->carry_in, "ns_synth: lens does not go with a carried stream");
  FAC_REQUIRE(d->x_bs >= d->k || d->B == 1, "ns_synth: x_bs = %lld below k = %d", (long long)d->x_bs, d->k);
  FAC_REQUIRE(d->y_bs >= d->n_out || d->B == 1, "ns_synth: y_bs = %lld below n_out = %d", (long long)d->y_bs, d->n_out);
  NsSynthArgs a;
  a.d = *d;
  a.s_first = ns_fdiv(d->m0, FAC_NS_H);
  a.s_last = ns_fdiv(d->m0 + d->n_out - 1, FAC_NS_H);
  // the oldest frame read starts at (s_first - 1) H: the carry (or, without one, the start of the signal) must reach it
  FAC_REQUIRE(!d->carry_in || d->X || (a.s_first - 1) * (long long)FAC_NS_H >= d->n0 - FAC_NS_CARRY,
              "ns_synth: output %lld needs samples more than %d in front of n0 = %lld", (long long)d->m0, (int)FAC_NS_CARRY, (long long)d->n0);
  FAC_REQUIRE(d->carry_in || d->X || d->n0 == 0 || (a.s_first - 1) * (long long)FAC_NS_H >= d->n0,
              "ns_synth: output %lld needs samples in front of n0 = %lld and there is no carry", (long long)d->m0, (long long)d->n0);
  // frames s_first .. s_last + 1 are read from the ring: they must sit in different slots
  const long long span = a.s_last - a.s_first + 2, held = a.s_last + 2;
  FAC_REQUIRE(d->R >= 1 && d->R <= (1 << 22) && d->R >= (held < span ? held : span), "ns_synth: R = %d below the %lld frames the outputs reach", d->R,
              (long long)(held < span ? held : span));
  FAC_REQUIRE(d->g_bs >= (long long)d->R * FAC_NS_BINS || d->B == 1, "ns_synth: g_bs = %lld below R * 257", (long long)d->g_bs);
  const long long n_wg = (span - 1 + NS_SF - 2) / (NS_SF - 1);
  hipLaunchKernelGGL(ns_synth_kernel, dim3((unsigned)n_wg, (unsigned)d->B), dim3(NS_T), 0, (hipStream_t)stream, a);
  return check_launch("ns_synth");
}
