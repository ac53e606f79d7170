// Objective scores on the device: SI-SDR, STOI and ESTOI of an estimate against a reference, batched over ragged
// rows.  What is computed is stated in include/facodec_hip.h above fac_si_sdr; this comment is about how.
//
// fac_si_sdr.  Three passes over both rows, each a grid of (chunks, rows) workgroups that write one pair of fp64 partial sums per
// chunk of SD_CHUNK samples, each followed by one workgroup per row that adds the row's partials and leaves what the next pass
// needs in a four-double row record (the two means; the scale a; then the score itself):
//   pass 1  sum x, sum y                          -> mean(x), mean(y)
//   pass 2  sum e r, sum r r on centred samples   -> a
//   pass 3  sum (a r)^2, sum (e - a r)^2          -> 10 log10(. / . + eps)
// A thread adds its 16 samples of the chunk in ascending order, the workgroup's 256 sums go through a fixed tree, a row's chunk
// sums through thread-strided sums and the same tree.  Chunks behind a row's end contribute exact zeros, so the sums do not
// depend on how long the batch is.  Six launches; the input is read three times (2 x 4 bytes per sample and pass).
//
// STOI / ESTOI.  Four stages, all fp64:
//   stoi_energy_kernel  one wave per frame of the reference (lane = 4 strided samples, butterfly sum), 32 frames per workgroup.
//   stoi_select_kernel  one workgroup per row: maximum of E, then blocks of 256 frames: keep flag, inclusive scan in LDS, carried
//                       offset; writes the kept frame indices in order (-1 behind them) and n_frames / n_kept.
//   stoi_bands_kernel   one wave per (kept frame, signal): the frame of the compacted signal is rebuilt from the kept frame and
//                       its kept neighbours, windowed again and transformed in LDS by the wave's own 512-point transform of
//                       fft512_f64.h (twiddles from a 256-entry table the workgroup computes once with sincospi); bin k then
//                       sits at the bit-reversed index.  The 212 powers of bins 7 .. 218 go to LDS and 15 lanes add their
//                       band in ascending bin order, both ordered inside the wave.  32 frames per workgroup:
//                       4 waves x 16 rounds, wave w of round i takes transform 4 i + w = (frame 2 i + w / 2, signal w & 1).
//                       x and y are transformed separately (not packed as real and imaginary part of one transform): a zero
//                       reference must give exact zeros, which the packed form's 1e-16 leakage from y would not.
//   stoi_score_kernel   32 segments per workgroup: the (2, 15, 32 + 29) tile of band magnitudes in LDS, one wave per segment
//                       and round; lanes 0 .. 14 take one band row each (STOI's clipped correlation and ESTOI's row
//                       normalisation, written to LDS), lanes 0 .. 29 then one column each, lane 0 adds both in ascending order.
//   stoi_finish_kernel  per row, the segment sums in a fixed order -> stoi, estoi, n_segments.
// Nothing depends on scheduling and nothing is accumulated with atomics: two runs, and a row alone or in a batch, give the same
// bits.  All LDS of the band and score kernels is private to one wave except the read-only tables and tile: the band kernel
// has one workgroup barrier, behind its tables, and orders a wave's own LDS traffic inside the wave; the score kernel's barriers
// between its stages do the same job, and every loop with a barrier has a workgroup-uniform trip count.
#include "common.h"
#include "fft512_f64.h"
#include <math.h>

namespace fac {

constexpr int MT_T = 256;                      // threads of every kernel here
constexpr int SD_CHUNK = FAC_SI_SDR_CHUNK;
constexpr int SD_PER = SD_CHUNK / MT_T;
static_assert(SD_CHUNK % MT_T == 0, "si_sdr chunk geometry");

constexpr int ST_FRAME = 256, ST_HOP = 128, ST_NFFT = 512, ST_BANDS = 15, ST_SEG = 30;
constexpr int ST_FE = 32;                      // frames per workgroup of the energy kernel (8 per wave)
constexpr int ST_SCAN = MT_T;                  // frames per block of the scan
constexpr int ST_FB = 32;                      // frames per workgroup of the band kernel
constexpr int ST_SS = 32;                      // segments per workgroup of the score kernel
constexpr int ST_TILE = ST_SS + ST_SEG - 1;    // columns of band magnitudes 32 segments read
constexpr int ST_BIN0 = 7, ST_BIN1 = 219;      // bins the bands cover
constexpr double ST_EPS = 2.220446049250313e-16;
constexpr double ST_DYN = 40.0;
constexpr double SD_EPS = 1e-8;
static_assert(ST_NFFT == FFT512_N && MT_T == FFT512_N / 2 && MT_T == ST_FRAME, "one thread per twiddle and per window entry");
static_assert(ST_FE % 4 == 0 && ST_FB % 2 == 0 && ST_SS % 4 == 0, "four waves share a workgroup's frames / segments evenly");

__constant__ int st_lo[ST_BANDS] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174};
__constant__ int st_hi[ST_BANDS] = {9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

__device__ __forceinline__ int mt_row_len(const int32_t* lens, int b, int T) {
  if (!lens) return T;
  const int L = lens[b];
  return L < 0 ? 0 : (L > T ? T : L);
}

__host__ __device__ constexpr int st_frames(int len) { return len < ST_FRAME ? 0 : (len - ST_FRAME) / ST_HOP + 1; }

// sums of a and of b over the workgroup in a fixed tree order; every thread gets both.  red: 2 * MT_T doubles.
__device__ __forceinline__ void wg_sum2(double& a, double& b, double* red, int tid) {
  __syncthreads();
  red[tid] = a, red[MT_T + tid] = b;
  __syncthreads();
  for (int o = MT_T / 2; o >= 1; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o], red[MT_T + tid] += red[MT_T + tid + o];
    __syncthreads();
  }
  a = red[0], b = red[MT_T];
}

// ---- SI-SDR

struct SdArgs {
  const float* x;
  const float* y;
  const int32_t* lens;
  double* part;      // (3, B, n_chunks, 2)
  double* rowv;      // (B, 4): mean x, mean y, a, unused
  double* out;
  long long x_bs, y_bs;
  int B, T, n_chunks;
};

template <int P>
__global__ __launch_bounds__(MT_T) void sd_pass_kernel(SdArgs a) {
  __shared__ double red[2 * MT_T];
  const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const int len = mt_row_len(a.lens, b, a.T);
  const float* __restrict__ x = a.x + b * a.x_bs;
  const float* __restrict__ y = a.y + b * a.y_bs;
  const double* rv = a.rowv + 4ll * b;
  double mx = 0.0, my = 0.0, al = 0.0;
  if (P >= 2) mx = rv[0], my = rv[1];
  if (P == 3) al = rv[2];
  double s0 = 0.0, s1 = 0.0;
  const int t0 = c * SD_CHUNK;                      // < T + SD_CHUNK <= 2^30 + 2^12
#pragma unroll 4
  for (int k = 0; k < SD_PER; ++k) {
    const int t = t0 + k * MT_T + tid;
    if (t < len) {
      const double xv = (double)x[t], yv = (double)y[t];
      if (P == 1) {
        s0 += xv, s1 += yv;
      } else {
        const double r = xv - mx, e = yv - my;
        if (P == 2) {
          s0 += e * r, s1 += r * r;
        } else {
          const double s = al * r;
          const double n = e - s;
          s0 += s * s, s1 += n * n;
        }
      }
    }
  }
  wg_sum2(s0, s1, red, tid);
  if (tid == 0) {
    double* p = a.part + (((long long)(P - 1) * a.B + b) * a.n_chunks + c) * 2;
    p[0] = s0, p[1] = s1;
  }
}

template <int P>
__global__ __launch_bounds__(MT_T) void sd_finish_kernel(SdArgs a) {
  __shared__ double red[2 * MT_T];
  const int b = blockIdx.x, tid = threadIdx.x;
  const double* p = a.part + ((long long)(P - 1) * a.B + b) * a.n_chunks * 2;
  double s0 = 0.0, s1 = 0.0;
  for (int c = tid; c < a.n_chunks; c += MT_T) s0 += p[2ll * c], s1 += p[2ll * c + 1];
  wg_sum2(s0, s1, red, tid);
  if (tid != 0) return;
  double* rv = a.rowv + 4ll * b;
  if (P == 1) {
    const double n = (double)mt_row_len(a.lens, b, a.T);
    rv[0] = s0 / n, rv[1] = s1 / n;                 // an empty row: 0 / 0 = NaN, which no sample ever meets
  } else if (P == 2) {
    rv[2] = (s0 + SD_EPS) / (s1 + SD_EPS);
  } else {
    a.out[b] = 10.0 * log10(s0 / s1 + SD_EPS);
  }
}

// ---- STOI

struct StArgs {
  const float* x;
  const float* y;
  const int32_t* lens;
  int32_t* kept_idx;
  int32_t* n_frames;
  int32_t* n_kept;
  int32_t* n_segments;
  double* stoi;
  double* estoi;
  double* E;         // (B, M_max)
  double* Tb;        // (B, 2, 15, M_max)
  double* seg;       // (B, 2, S_max)
  long long x_bs, y_bs;
  int B, T, M_max, S_max;
};

__device__ __forceinline__ double st_window(int n) { return 0.5 - 0.5 * cospi(2.0 * (double)(n + 1) / (double)(ST_FRAME + 1)); }

__global__ __launch_bounds__(MT_T) void stoi_energy_kernel(StArgs a) {
  const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int M = st_frames(mt_row_len(a.lens, b, a.T));
  const float* __restrict__ x = a.x + b * a.x_bs;
  double w[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) w[q] = st_window(lane + 64 * q);
  for (int i = 0; i < ST_FE / 4; ++i) {
    const int m = blockIdx.x * ST_FE + wave * (ST_FE / 4) + i;
    if (m >= M) break;                              // wave-uniform; no barrier in this kernel
    const float* f = x + (long long)m * ST_HOP;     // the frame ends at 128 m + 255 < len <= T
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double v = w[q] * (double)f[lane + 64 * q];
      acc += v * v;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) a.E[(long long)b * a.M_max + m] = 20.0 * log10(sqrt(acc) + ST_EPS);
  }
}

__global__ __launch_bounds__(MT_T) void stoi_select_kernel(StArgs a) {
  __shared__ double mxs[MT_T];
  __shared__ int sc[MT_T];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int M = st_frames(mt_row_len(a.lens, b, a.T));
  const double* __restrict__ E = a.E + (long long)b * a.M_max;
  int32_t* kept = a.kept_idx + (long long)b * a.M_max;
  double mx = -INFINITY;
  for (int m = tid; m < M; m += MT_T) mx = fmax(mx, E[m]);
  mxs[tid] = mx;
  __syncthreads();
  for (int o = MT_T / 2; o >= 1; o >>= 1) {
    if (tid < o) mxs[tid] = fmax(mxs[tid], mxs[tid + o]);
    __syncthreads();
  }
  const double top = mxs[0];
  int carry = 0;                                    // every thread keeps the same count
  for (int base = 0; base < M; base += ST_SCAN) {   // M is uniform over the workgroup
    const int m = base + tid;
    const int flag = (m < M && top - ST_DYN - E[m] < 0.0) ? 1 : 0;
    sc[tid] = flag;
    __syncthreads();
    for (int o = 1; o < ST_SCAN; o <<= 1) {
      const int v = tid >= o ? sc[tid - o] : 0;
      __syncthreads();
      sc[tid] += v;
      __syncthreads();
    }
    if (flag) kept[carry + sc[tid] - 1] = m;        // carry + sc[tid] - 1 <= m < M <= M_max
    carry += sc[ST_SCAN - 1];
    __syncthreads();
  }
  for (int i = carry + tid; i < a.M_max; i += MT_T) kept[i] = -1;   // behind the kept frames: no frame
  if (tid == 0) a.n_frames[b] = M, a.n_kept[b] = carry;
}

__global__ __launch_bounds__(MT_T) void stoi_bands_kernel(StArgs a) {
  __shared__ double2 buf[4][ST_NFFT];
  __shared__ double2 tw[ST_NFFT / 2];
  __shared__ double win[ST_FRAME];
  __shared__ double pw[4][ST_BIN1 - ST_BIN0 + 4];
  const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int K = a.n_kept[b];
  const int j0 = blockIdx.x * ST_FB;
  if (j0 >= K) return;                              // the whole workgroup, before any barrier
  fft512_table(tw, tid);
  win[tid] = st_window(tid);
  __syncthreads();                                  // the tables: written by all four waves, read by each
  const int32_t* __restrict__ kept = a.kept_idx + (long long)b * a.M_max;
  double2* z = buf[wave];

  // buf[wave] and pw[wave] are the wave's own and nothing else is written: no workgroup barrier in this loop, the wave orders
  // its own LDS traffic and leaves when its frames run out
  for (int it = 0; it < ST_FB / 2; ++it) {
    const int q = it * 4 + wave;
    const int jj = j0 + (q >> 1), sig = q & 1;
    if (jj >= K) break;                             // wave-uniform, and jj only grows
    const float* __restrict__ src = sig ? a.y + b * a.y_bs : a.x + b * a.x_bs;
    const long long k = kept[jj];
    const long long kp = jj > 0 ? kept[jj - 1] : -1, kn = jj + 1 < K ? kept[jj + 1] : -1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = lane + 64 * r;
      double c = win[n] * (double)src[k * ST_HOP + n];
      if (n < ST_HOP) {
        if (kp >= 0) c = win[n + ST_HOP] * (double)src[kp * ST_HOP + n + ST_HOP] + c;
      } else {
        if (kn >= 0) c = c + win[n - ST_HOP] * (double)src[kn * ST_HOP + n - ST_HOP];
      }
      z[n] = make_double2(win[n] * c, 0.0);
      z[n + ST_FRAME] = make_double2(0.0, 0.0);
    }
    fft512_forward(z, tw, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int kbin = ST_BIN0 + lane + 64 * r;
      if (kbin < ST_BIN1) {
        const double2 v = z[fft512_rev(kbin)];
        pw[wave][kbin - ST_BIN0] = v.x * v.x + v.y * v.y;
      }
    }
    fft512_wave_sync();                             // the powers, for the lanes that add the bands
    if (lane < ST_BANDS) {
      double s = 0.0;
      for (int kbin = st_lo[lane]; kbin < st_hi[lane]; ++kbin) s += pw[wave][kbin - ST_BIN0];
      a.Tb[(((long long)b * 2 + sig) * ST_BANDS + lane) * a.M_max + jj] = sqrt(s);
    }
    fft512_wave_sync();                             // read before the next round overwrites pw[wave] and the buffer
  }
}

__global__ __launch_bounds__(MT_T) void stoi_score_kernel(StArgs a) {
  __shared__ double tile[2][ST_BANDS][ST_TILE];
  __shared__ double xr[4][ST_BANDS][ST_SEG];
  __shared__ double yr[4][ST_BANDS][ST_SEG];
  __shared__ double col[4][32];
  __shared__ double cj[4][16];
  const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int K = a.n_kept[b];
  const int n_seg = K >= ST_SEG ? K - ST_SEG + 1 : 0;
  const int s0 = blockIdx.x * ST_SS;
  if (s0 >= n_seg) return;                          // the whole workgroup, before any barrier
  const int n_col = K - s0 < ST_TILE ? K - s0 : ST_TILE;
  for (int i = tid; i < 2 * ST_BANDS * ST_TILE; i += MT_T) {
    const int c = i % ST_TILE, rj = i / ST_TILE;    // rj = sig * 15 + band
    (&tile[0][0][0])[i] = c < n_col ? a.Tb[((long long)b * 2 * ST_BANDS + rj) * a.M_max + s0 + c] : 0.0;
  }
  __syncthreads();
  const double clip = 1.0 + pow(10.0, 15.0 / 20.0);

  for (int it = 0; it < ST_SS / 4; ++it) {
    const int off = it * 4 + wave;
    const int s = s0 + off;
    const bool valid = s < n_seg;                   // wave-uniform
    if (valid && lane < ST_BANDS) {
      const double* xs = &tile[0][lane][off];
      const double* ys = &tile[1][lane][off];
      double sxx = 0.0, syy = 0.0, sx = 0.0, sy = 0.0;
      for (int m = 0; m < ST_SEG; ++m) sxx += xs[m] * xs[m], syy += ys[m] * ys[m], sx += xs[m], sy += ys[m];
      const double alpha = sqrt(sxx) / (sqrt(syy) + ST_EPS);
      const double mx = sx / ST_SEG, my = sy / ST_SEG;
      double sp = 0.0;
      for (int m = 0; m < ST_SEG; ++m) sp += fmin(alpha * ys[m], xs[m] * clip);
      const double mp = sp / ST_SEG;
      double nx = 0.0, ny = 0.0, np = 0.0;
      for (int m = 0; m < ST_SEG; ++m) {
        const double dx = xs[m] - mx, dy = ys[m] - my, dp = fmin(alpha * ys[m], xs[m] * clip) - mp;
        nx += dx * dx, ny += dy * dy, np += dp * dp;
      }
      const double ix = sqrt(nx) + ST_EPS, iy = sqrt(ny) + ST_EPS, ip = sqrt(np) + ST_EPS;
      double dot = 0.0;
      for (int m = 0; m < ST_SEG; ++m) {
        const double ux = (xs[m] - mx) / ix;
        dot += ux * ((fmin(alpha * ys[m], xs[m] * clip) - mp) / ip);
        xr[wave][lane][m] = ux;
        yr[wave][lane][m] = (ys[m] - my) / iy;
      }
      cj[wave][lane] = dot;
    }
    __syncthreads();
    if (valid && lane < ST_SEG) {
      double sx = 0.0, sy = 0.0;
      for (int j = 0; j < ST_BANDS; ++j) sx += xr[wave][j][lane], sy += yr[wave][j][lane];
      const double mx = sx / ST_BANDS, my = sy / ST_BANDS;
      double nx = 0.0, ny = 0.0;
      for (int j = 0; j < ST_BANDS; ++j) {
        const double dx = xr[wave][j][lane] - mx, dy = yr[wave][j][lane] - my;
        nx += dx * dx, ny += dy * dy;
      }
      const double ix = sqrt(nx) + ST_EPS, iy = sqrt(ny) + ST_EPS;
      double dot = 0.0;
      for (int j = 0; j < ST_BANDS; ++j) dot += ((xr[wave][j][lane] - mx) / ix) * ((yr[wave][j][lane] - my) / iy);
      col[wave][lane] = dot;
    }
    __syncthreads();
    if (valid && lane == 0) {
      double c = 0.0, d = 0.0;
      for (int j = 0; j < ST_BANDS; ++j) c += cj[wave][j];
      for (int m = 0; m < ST_SEG; ++m) d += col[wave][m];
      a.seg[((long long)b * 2) * a.S_max + s] = c;
      a.seg[((long long)b * 2 + 1) * a.S_max + s] = d / ST_SEG;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(MT_T) void stoi_finish_kernel(StArgs a) {
  __shared__ double red[2 * MT_T];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int K = a.n_kept[b];
  const int n_seg = K >= ST_SEG ? K - ST_SEG + 1 : 0;  // <= S_max, since K <= M_max
  const double* c = a.seg + ((long long)b * 2) * a.S_max;
  const double* d = c + a.S_max;
  double sc = 0.0, sd = 0.0;
  for (int s = tid; s < n_seg; s += MT_T) sc += c[s], sd += d[s];
  wg_sum2(sc, sd, red, tid);
  if (tid != 0) return;
  a.n_segments[b] = n_seg;
  a.stoi[b] = n_seg ? sc / ((double)ST_BANDS * (double)n_seg) : (double)NAN;
  a.estoi[b] = n_seg ? sd / (double)n_seg : (double)NAN;
}

static int64_t st_row_doubles(int M_max) {
  const int S_max = M_max >= ST_SEG ? M_max - ST_SEG + 1 : 0;
  return (int64_t)M_max * (1 + 2 * ST_BANDS) + 2 * (int64_t)S_max;
}

// the checks of the three launches, which share the descriptor; fills the kernels' arguments
static int st_args(const fac_stoi_desc* d, const char* what, StArgs* a) {
  FAC_REQUIRE(d, "%s: null descriptor", what);
  FAC_REQUIRE(d->B >= 1 && d->B <= 65535, "%s: B = %d outside 1 .. 65535", what, d->B);
  FAC_REQUIRE(d->T >= 0 && d->T <= (1 << 28), "%s: T = %d outside 0 .. 2^28", what, d->T);
  FAC_REQUIRE(d->x && d->y && d->kept_idx && d->n_frames && d->n_kept && d->n_segments && d->stoi && d->estoi && d->ws,
              "%s: null pointer (x, y, kept_idx, n_frames, n_kept, n_segments, stoi, estoi, ws)", what);
  FAC_REQUIRE(((uintptr_t)d->ws & 7) == 0, "%s: ws must be 8-byte aligned", what);
  const int M_max = st_frames(d->T);
  const int64_t need = 8 * st_row_doubles(M_max) * d->B;
  FAC_REQUIRE(d->ws_bytes >= need, "%s: workspace of %lld bytes, %lld needed (fac_stoi_geometry)", what, (long long)d->ws_bytes,
              (long long)need);
  a->x = d->x, a->y = d->y, a->lens = d->lens;
  a->kept_idx = d->kept_idx, a->n_frames = d->n_frames, a->n_kept = d->n_kept, a->n_segments = d->n_segments;
  a->stoi = d->stoi, a->estoi = d->estoi;
  a->x_bs = d->x_bs, a->y_bs = d->y_bs;
  a->B = d->B, a->T = d->T, a->M_max = M_max, a->S_max = M_max >= ST_SEG ? M_max - ST_SEG + 1 : 0;
  a->E = (double*)d->ws;
  a->Tb = a->E + (int64_t)d->B * M_max;
  a->seg = a->Tb + (int64_t)d->B * 2 * ST_BANDS * M_max;
  return FAC_OK;
}

}  // namespace fac

using namespace fac;

extern "C" int64_t fac_si_sdr_ws_bytes(int B, int T) {
  if (B <= 0 || T < 0 || T > (1 << 30)) return -1;
  const int64_t n_chunks = ((int64_t)T + SD_CHUNK - 1) / SD_CHUNK;
  return 8 * (int64_t)B * (6 * n_chunks + 4);
}

extern "C" int fac_si_sdr(const float* x, int64_t x_bs, const float* y, int64_t y_bs, const int32_t* lens, double* out, void* ws,
                          int64_t ws_bytes, int B, int T, fac_stream_t stream) {
  FAC_REQUIRE(B >= 1 && B <= 65535, "si_sdr: B = %d outside 1 .. 65535", B);
  FAC_REQUIRE(T >= 0 && T <= (1 << 30), "si_sdr: T = %d outside 0 .. 2^30", T);
  FAC_REQUIRE(x && y && out && ws, "si_sdr: null pointer (x, y, out, ws)");
  FAC_REQUIRE(((uintptr_t)ws & 7) == 0, "si_sdr: ws must be 8-byte aligned");
  const int64_t need = fac_si_sdr_ws_bytes(B, T);
  FAC_REQUIRE(ws_bytes >= need, "si_sdr: workspace of %lld bytes, %lld needed (fac_si_sdr_ws_bytes)", (long long)ws_bytes, (long long)need);
  SdArgs a;
  a.x = x, a.y = y, a.lens = lens, a.out = out;
  a.x_bs = x_bs, a.y_bs = y_bs;
  a.B = B, a.T = T, a.n_chunks = (int)(((int64_t)T + SD_CHUNK - 1) / SD_CHUNK);
  a.part = (double*)ws;
  a.rowv = a.part + 6ll * B * a.n_chunks;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)a.n_chunks, (unsigned)B), rows((unsigned)B), block(MT_T);
  if (a.n_chunks) hipLaunchKernelGGL(sd_pass_kernel<1>, grid, block, 0, st, a);
  hipLaunchKernelGGL(sd_finish_kernel<1>, rows, block, 0, st, a);
  if (a.n_chunks) hipLaunchKernelGGL(sd_pass_kernel<2>, grid, block, 0, st, a);
  hipLaunchKernelGGL(sd_finish_kernel<2>, rows, block, 0, st, a);
  if (a.n_chunks) hipLaunchKernelGGL(sd_pass_kernel<3>, grid, block, 0, st, a);
  hipLaunchKernelGGL(sd_finish_kernel<3>, rows, block, 0, st, a);
  return check_launch("si_sdr");
}

extern "C" int fac_stoi_geometry(int T, int64_t* out6) {
  FAC_REQUIRE(out6, "stoi_geometry: null output");
  FAC_REQUIRE(T >= 0 && T <= (1 << 28), "stoi_geometry: T = %d outside 0 .. 2^28", T);
  const int M_max = st_frames(T);
  out6[0] = M_max, out6[1] = 8 * st_row_doubles(M_max);
  out6[2] = ST_FE, out6[3] = ST_SCAN, out6[4] = ST_FB, out6[5] = ST_SS;
  return FAC_OK;
}

extern "C" int fac_stoi_select(const fac_stoi_desc* d, fac_stream_t stream) {
  StArgs a;
  if (int rc = st_args(d, "stoi_select", &a)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (a.M_max)
    hipLaunchKernelGGL(stoi_energy_kernel, dim3((unsigned)((a.M_max + ST_FE - 1) / ST_FE), (unsigned)a.B), dim3(MT_T), 0, st, a);
  hipLaunchKernelGGL(stoi_select_kernel, dim3((unsigned)a.B), dim3(MT_T), 0, st, a);
  return check_launch("stoi_select");
}

extern "C" int fac_stoi_bands(const fac_stoi_desc* d, fac_stream_t stream) {
  StArgs a;
  if (int rc = st_args(d, "stoi_bands", &a)) return rc;
  if (!a.M_max) return FAC_OK;
  hipLaunchKernelGGL(stoi_bands_kernel, dim3((unsigned)((a.M_max + ST_FB - 1) / ST_FB), (unsigned)a.B), dim3(MT_T), 0, (hipStream_t)stream, a);
  return check_launch("stoi_bands");
}

extern "C" int fac_stoi_score(const fac_stoi_desc* d, fac_stream_t stream) {
  StArgs a;
  if (int rc = st_args(d, "stoi_score", &a)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (a.S_max)
    hipLaunchKernelGGL(stoi_score_kernel, dim3((unsigned)((a.S_max + ST_SS - 1) / ST_SS), (unsigned)a.B), dim3(MT_T), 0, st, a);
  hipLaunchKernelGGL(stoi_finish_kernel, dim3((unsigned)a.B), dim3(MT_T), 0, st, a);
  return check_launch("stoi_score");
}
