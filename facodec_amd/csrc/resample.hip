// Sample-rate conversion by a rational ratio: o input samples per n output samples, a polyphase windowed-sinc
// filter whose coefficients the host builds in float64 and rounds once (dsp.py resample_table): table (n phases, taps) and the
// first-tap offsets offs (n).  Output m = k n + p is the dot product of table[p] with the taps inputs from k o + offs[p] on.
//
// One workgroup takes tiles of `tm` consecutive outputs of one row.  Per tile it stages the contiguous input span those outputs
// read into LDS (coalesced 4-byte loads: the span starts wherever the tile's first output starts, so no wider load is aligned;
// what lies outside the row's signal is staged as 0, which is how the padding behind lens[b] is never read), then every lane
// produces outputs m0 + lane, m0 + lane + threads, ... by a dot product in ascending tap order with one fma per tap.  The order of
// an output's additions therefore depends on its phase only -- not on the tile, the row, the batch or the streaming block it falls
// in -- which is what makes a padded batch equal its rows alone and a stream equal the offline call, bit for bit.
//
// LDS layout.  Neighbouring lanes read the span o / n words apart (2 for 48 -> 24 kHz, 1 or 2 for 147 / 80) and ds_read_b32 banks
// per 32 lanes modulo 32 words, so a stride of 2, 4, ... would put 2, 4, ... lanes on a bank.  Word i of the span is stored at
// i + (i >> 5): after every 32 words the image shifts by one bank, and 32 lanes at any power-of-two stride up to 32 fall on 32
// different banks (odd strides were conflict-free before and stay so).  Table rows are padded to an odd pitch `ts`: lanes hold
// consecutive phases, i.e. rows, and an odd pitch spreads them over all banks; with one phase every lane reads the same word
// (a broadcast).
//
// Three forms of one template (fac_resample_form):
//   0  table resident in LDS for the life of the workgroup (which loops over tiles when the table is big enough for the reload to
//      matter), beside the span;
//   1  the table does not fit beside a span: coefficients come from global memory (a few hundred KB at most, L2-resident);
//   2  not even the span of 64 outputs fits (o / n in the hundreds): inputs come from global memory too.  Slow, and only there
//      so that every ratio up to 640 works.
#include "common.h"
#include <limits.h>

namespace fac {

struct ResampleArgs {
  fac_resample_desc d;
  int tm, span_cap, n_tiles, ts;
};

struct ResamplePlan {
  int form, tm, threads, span_cap, n_tiles, ts;
  size_t lds;
  unsigned gx;
};

// r = q - q0: the block for r >= 0, the carried history below, 0 outside the signal (and below absolute sample 0: r_min)
__device__ __forceinline__ float rs_fetch(const float* __restrict__ hrow, const float* __restrict__ xrow, int r, int Lb, int r_min,
                                          int n_hist) {
  if (r >= 0) return r < Lb ? xrow[r] : 0.f;
  return r >= r_min ? hrow[n_hist + r] : 0.f;
}

template <bool TAB_LDS, bool X_LDS>
__global__ __launch_bounds__(1024) void resample_kernel(ResampleArgs a) {
  extern __shared__ float rs_smem[];
  const fac_resample_desc& d = a.d;
  const int b = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
  const int o = d.o, n = d.n, taps = d.taps, ts = a.ts, n_hist = d.n_hist;
  int Lb = d.T;
  if (d.lens) {
    const int L = d.lens[b];
    Lb = L < 0 ? 0 : (L > d.T ? d.T : L);
  }
  const int r_min = d.q0 < (long long)n_hist ? -(int)d.q0 : -n_hist;
  const float* hrow = d.hist ? d.hist + b * d.hist_bs : nullptr;
  const float* xrow = d.x + b * d.x_bs;
  float* yrow = d.y + b * d.y_bs;
  const long long m_end = ((d.q0 + Lb) * n + o - 1) / o;

  if (d.hist_out && blockIdx.x == 0) {
    float* ho = d.hist_out + b * d.hist_bs;
    for (int j = tid; j < n_hist; j += nt) ho[j] = rs_fetch(hrow, xrow, d.T - n_hist + j, Lb, r_min, n_hist);
  }

  float* tab_s = rs_smem;
  float* xs = rs_smem + (TAB_LDS ? n * ts : 0);
  if (TAB_LDS) {
    const int total = n * taps;
    for (int idx = tid; idx < total; idx += nt) {
      const int r = idx / taps;
      tab_s[r * ts + (idx - r * taps)] = d.table[idx];
    }
  }

  for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    const int i0 = tile * a.tm;
    const int cnt = min(a.tm, d.n_out - i0);
    const long long m0 = d.m_lo + i0;
    long long k0 = m0 / n;
    int p0 = (int)(m0 - k0 * n);
    if (p0 < 0) {
      p0 += n;
      --k0;
    }
    const int base = (int)(k0 * o - d.q0);
    const int r_lo = base + d.offs[p0];
    if (X_LDS) {
      const int ppl = p0 + cnt - 1;
      const int dkl = ppl / n;
      int span = base + dkl * o + d.offs[ppl - dkl * n] + taps - r_lo;
      if (span > a.span_cap) span = a.span_cap;
      if (tile != (int)blockIdx.x) __syncthreads();          // the previous tile's reads of the span are done
      for (int idx = tid; idx < span; idx += nt) xs[idx + (idx >> 5)] = rs_fetch(hrow, xrow, r_lo + idx, Lb, r_min, n_hist);
    }
    if (X_LDS || TAB_LDS) __syncthreads();
    for (int ii = tid; ii < cnt; ii += nt) {
      const long long m = m0 + ii;
      float acc = 0.f;
      if (m >= 0 && m < m_end) {
        const int pp = p0 + ii;
        const int dk = pp / n;
        const int p = pp - dk * n;
        const int rf = base + dk * o + d.offs[p];
        const float* __restrict__ c = TAB_LDS ? tab_s + p * ts : d.table + (long long)p * taps;
        if (X_LDS) {
          const int s = rf - r_lo;
#pragma unroll 4
          for (int j = 0; j < taps; ++j) {
            const int w = s + j;
            acc = fmaf(c[j], xs[w + (w >> 5)], acc);
          }
        } else {
          for (int j = 0; j < taps; ++j) acc = fmaf(c[j], rs_fetch(hrow, xrow, rf + j, Lb, r_min, n_hist), acc);
        }
      }
      yrow[i0 + ii] = acc;
    }
  }
}

static size_t span_bytes(int span_cap) { return ((size_t)span_cap + span_cap / 32 + 1) * sizeof(float); }
static int span_cap_for(int tm, int o, int n, int taps) { return (int)(((long long)(tm - 1) * o + n - 1) / n) + taps + 2; }

static int resample_plan(const fac_resample_desc* d, ResamplePlan* pl) {
  FAC_REQUIRE(d, "resample: null descriptor");
  FAC_REQUIRE(d->x && d->y && d->table && d->offs, "resample: null pointer (x, y, table, offs)");
  FAC_REQUIRE(d->o >= 1 && d->o <= 640 && d->n >= 1 && d->n <= 640, "resample: o = %d, n = %d outside 1 .. 640", d->o, d->n);
  FAC_REQUIRE(d->taps >= 1 && (long long)d->taps * d->n < (1 << 28), "resample: bad table geometry (n = %d, taps = %d)", d->n, d->taps);
  FAC_REQUIRE(d->B >= 1 && d->B <= 65535 && d->T >= 0 && d->n_out >= 0 && d->n_hist >= 0, "resample: bad sizes (B = %d, T = %d, n_out = %d, n_hist = %d)",
              d->B, d->T, d->n_out, d->n_hist);
  FAC_REQUIRE(d->n_hist == 0 || d->hist, "resample: n_hist = %d without a history span", d->n_hist);
  FAC_REQUIRE(!d->hist_out || (!d->lens && d->n_hist > 0), "resample: hist_out needs a history span and no lens");
  FAC_REQUIRE(d->q0 >= 0 && d->q0 < (1ll << 52) && d->m_lo > -(1ll << 52) && d->m_lo < (1ll << 52), "resample: absolute indices out of range");
  // every index relative to q0 that the kernel forms must fit an int with room to spare
  const long long lead = d->m_lo / d->n * d->o - d->q0;
  const long long reach = (lead < 0 ? -lead : lead) + d->n_hist + d->T + ((long long)d->n_out / d->n + 2) * d->o + d->taps;
  FAC_REQUIRE(reach < (1ll << 30), "resample: the launch spans %lld samples around its block; 2^30 at most", reach);
  const int o = d->o, n = d->n, taps = d->taps;
  const int ts = taps | 1;
  const size_t tab = (size_t)n * ts * sizeof(float);
  int want = (d->n_out + 63) / 64 * 64;
  if (want < 64) want = 64;
  pl->ts = ts;
  pl->form = -1;
  if (tab <= 96 * 1024) {
    int threads = tab > 24 * 1024 ? 1024 : 256;
    int tm = threads * 4 < want ? threads * 4 : want;
    while (tm > 64 && tab + span_bytes(span_cap_for(tm, o, n, taps)) > FAC_LDS_MAX) tm = tm / 2 < 64 ? 64 : tm / 2 / 64 * 64;
    if (tab + span_bytes(span_cap_for(tm, o, n, taps)) <= FAC_LDS_MAX) {
      pl->form = 0, pl->tm = tm, pl->threads = threads < tm ? threads : tm;
      pl->lds = tab + span_bytes(span_cap_for(tm, o, n, taps));
    }
  }
  if (pl->form < 0) {
    int tm = 1024 < want ? 1024 : want;
    while (tm > 64 && span_bytes(span_cap_for(tm, o, n, taps)) > 64 * 1024) tm = tm / 2 < 64 ? 64 : tm / 2 / 64 * 64;
    if (span_bytes(span_cap_for(tm, o, n, taps)) <= FAC_LDS_MAX) {
      pl->form = 1, pl->tm = tm, pl->threads = 256 < tm ? 256 : tm;
      pl->lds = span_bytes(span_cap_for(tm, o, n, taps));
    } else {
      pl->form = 2, pl->tm = 256 < want ? 256 : want, pl->threads = pl->tm, pl->lds = 0;
    }
  }
  pl->span_cap = span_cap_for(pl->tm, o, n, taps);
  pl->n_tiles = (d->n_out + pl->tm - 1) / pl->tm;
  long long gx = pl->n_tiles;
  if (pl->form == 0 && tab > 8 * 1024) {
    // a table worth keeping: as many workgroups as the device holds at once, each looping over its tiles
    int cus = device_cus();
    if (cus <= 0) cus = 256;
    int per_cu = (int)(FAC_LDS_MAX / pl->lds);
    const int by_threads = 2048 / pl->threads;
    if (per_cu > by_threads) per_cu = by_threads;
    if (per_cu < 1) per_cu = 1;
    const long long cap = ((long long)cus * per_cu + d->B - 1) / d->B;
    if (gx > cap) gx = cap;
  }
  pl->gx = (unsigned)(gx < 1 ? 1 : gx);
  return FAC_OK;
}

template <bool TAB_LDS, bool X_LDS>
static void resample_launch(const ResampleArgs& a, const ResamplePlan& pl, hipStream_t stream) {
  allow_dynamic_lds<resample_kernel<TAB_LDS, X_LDS>>();
  hipLaunchKernelGGL((resample_kernel<TAB_LDS, X_LDS>), dim3(pl.gx, (unsigned)a.d.B), dim3(pl.threads), pl.lds, stream, a);
}

}  // namespace fac

using namespace fac;

extern "C" int fac_resample_form(const fac_resample_desc* d, int32_t* out4) {
  ResamplePlan pl;
  if (resample_plan(d, &pl) != FAC_OK) return -1;
  if (out4) out4[0] = pl.tm, out4[1] = pl.threads, out4[2] = (int32_t)pl.lds, out4[3] = (int32_t)pl.gx;
  return pl.form;
}

extern "C" int fac_resample(const fac_resample_desc* d, fac_stream_t stream) {
  ResamplePlan pl;
  const int rc = resample_plan(d, &pl);
  if (rc != FAC_OK) return rc;
  ResampleArgs a;
  a.d = *d;
  a.tm = pl.tm, a.span_cap = pl.span_cap, a.n_tiles = pl.n_tiles, a.ts = pl.ts;
  if (pl.form == 0) resample_launch<true, true>(a, pl, (hipStream_t)stream);
  else if (pl.form == 1) resample_launch<false, true>(a, pl, (hipStream_t)stream);
  else resample_launch<false, false>(a, pl, (hipStream_t)stream);
  return check_launch("resample");
}
