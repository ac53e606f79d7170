// The echo delay on the device: per row, a PHAT-weighted, recursively smoothed cross-spectrum between the
// microphone's frame and each of the far end's last L + 1 frames, the lag and the sample of its peak, a latch policy on that
// raw delay, and the aligner that hands the canceller (csrc/aec.hip) the far end moved by the latched delay.  Arithmetic, order
// and contracts: the header comment of include/facodec_hip.h.  All fp64 on the vector pipe, no atomics, every word has one
// writer; the build runs with -ffp-contract=off.
//
// The recursion is serial in time, so one 512-thread workgroup per row walks the blocks of the call: it aligns block j's samples
// with what the frames up to j - 1 decided, then computes frame j if the call completes it.  The trip counts are the row's,
// hence workgroup-uniform under every barrier.  Per frame: waves 0 and 1 window, measure and transform the far-end and the
// microphone frame; wave w updates the cross-spectra of lags w, w + 8, .. and sums their scores; wave 0 picks the lag, transforms
// its cross-spectrum back, picks the sample and runs the policy.  Three workgroup barriers per frame.  C and the X ring stay in
// global memory (L2): LDS holds the twiddles, the window, two transform buffers and a few small vectors, so several rows share a
// compute unit.  The two sample rings are indexed by the absolute sample and take the call's samples behind the last read.
#include "common.h"
#include "fft512_f64.h"
#include <math.h>

namespace fac {

constexpr int ED_T = 512, ED_WAVES = ED_T / 64;
constexpr int ED_N = FFT512_N, ED_H = ED_N / 2, ED_BINS = ED_H + 1, ED_LAGS = FAC_EDELAY_MAX_LAGS;
static_assert(ED_N == FAC_AEC_N && ED_H == FAC_AEC_H && ED_BINS == FAC_AEC_BINS, "the canceller's block grid");
static_assert((ED_LAGS - 1) * ED_H == FAC_EDELAY_MAX_DELAY && FAC_EDELAY_MIC_RING == ED_N - 1, "echo delay geometry");

struct EdArgs {
  fac_edelay_desc d;
};

static int ed_lags(int max_delay) { return (max_delay + ED_H - 1) / ED_H + 1; }

// One row's signal: sample n, absolute, of [ring | block]; the block's first sample is n0, the ring holds the rn samples in
// front of it, sample n at slot n % rn.  A sample before the row's start, at or behind its end, or older than the ring is 0.
struct RingSrc {
  const float* ring;
  const float* x;
  int rn;
  long long n0, start, end;
  __device__ __forceinline__ float sample(long long n) const {
    if (n < start || n >= end) return 0.f;
    const long long r = n - n0;
    if (r >= 0) return x[r];
    return ring && r >= -(long long)rn ? ring[n % rn] : 0.f;
  }
};

// behind the workgroup's last read of the ring: the last rn samples of the block
__device__ __forceinline__ void ring_store(float* ring, int rn, const float* x, long long n0, int k, int tid) {
  for (long long n = (k > rn ? n0 + k - rn : n0) + tid; n < n0 + k; n += ED_T) ring[n % rn] = x[n - n0];
}

__global__ __launch_bounds__(ED_T) void edelay_kernel(EdArgs a) {
  __shared__ __attribute__((aligned(16))) double2 tw[ED_N / 2];
  __shared__ __attribute__((aligned(16))) double2 zb[2][ED_N];     // far end (later the cross-spectrum's inverse), microphone
  __shared__ double win[ED_N];
  __shared__ double sc[ED_LAGS + 7];
  __shared__ double s_conf;
  __shared__ int s_act[ED_LAGS + 7];
  __shared__ int s_pol[FAC_EDELAY_POL];
  __shared__ int s_now[2];                                         // actx_m, actd_m
  const fac_edelay_desc& d = a.d;
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int L1 = (d.max_delay + ED_H - 1) / ED_H + 1, nb = d.k_hi - d.k_lo;

  int kb = d.k;
  if (d.lens) {
    const int len = d.lens[b];
    kb = len < 0 ? 0 : (len < d.k ? len : d.k);
  }
  const long long n0 = d.n0, end = n0 + kb;
  const long long start = d.starts ? (d.starts[b] > 0 ? d.starts[b] : 0) : 0;
  const float* mrow = d.mic + (long long)b * d.mic_bs;
  const float* frow = d.far + (long long)b * d.far_bs;
  float* mring = d.mic_ring ? d.mic_ring + (long long)b * FAC_EDELAY_MIC_RING : nullptr;
  float* fring = d.far_ring ? d.far_ring + (long long)b * d.far_rn : nullptr;
  const RingSrc mic = {mring, mrow, FAC_EDELAY_MIC_RING, n0, start, end};
  const RingSrc far = {fring, frow, d.far_rn, n0, start, end};

  const long long mfirst = start / ED_H + 1;
  const long long mlo = d.frm0 > mfirst ? d.frm0 : mfirst;
  long long mhi = d.frm0 + d.n_frm < end / ED_H ? d.frm0 + d.n_frm : end / ED_H;
  if (mhi < mlo) mhi = mlo;

  double2* Cg = reinterpret_cast<double2*>(d.C + (long long)b * d.c_bs);
  double2* Xg = reinterpret_cast<double2*>(d.X + (long long)b * d.xr_bs);
  int32_t* actg = d.act + (long long)b * L1;
  int32_t* polg = d.pol + (long long)b * FAC_EDELAY_POL;
  float* yrow = d.y + (long long)b * d.y_bs;
  const long long frow_out = (long long)b * d.f_bs;

  // every column of the per-frame outputs that is no frame of this row (without a ring of columns)
  if (!d.f_ring) {
    for (int i = tid; i < d.n_frm; i += ED_T) {
      const long long m = d.frm0 + i;
      if (m >= mlo && m < mhi) continue;
      if (d.raw) d.raw[frow_out + i] = -1;
      if (d.locked) d.locked[frow_out + i] = -1;
      if (d.used) d.used[frow_out + i] = -1;
      if (d.conf) d.conf[frow_out + i] = 0.0;
      if (d.ok) d.ok[frow_out + i] = 0;
    }
    if (d.score) {
      for (long long i = tid; i < (long long)d.n_frm * L1; i += ED_T) {
        const long long m = d.frm0 + i / L1;
        if (m < mlo || m >= mhi) d.score[frow_out * L1 + i] = 0.0;
      }
    }
  }

  if (tid < ED_N / 2) fft512_table(tw, tid);
  win[tid] = sinpi(((double)tid + 0.5) / (double)ED_N);
  if (tid < L1) s_act[tid] = actg[tid];
  if (tid < FAC_EDELAY_POL) s_pol[tid] = polg[tid];
  if (tid == 0) s_conf = d.conf_last[b];
  const double ca = d.a, oma = 1.0 - d.a;
  __syncthreads();

  const long long j0 = n0 / ED_H, j1 = (n0 + d.k - 1) / ED_H;
  for (long long m = j0; m <= j1; ++m) {
    // the aligner: block m's samples of this call, by what the frames up to m - 1 decided
    {
      const int u = m - 1 >= mfirst ? s_pol[3] : d.delay0;
      const long long lo = m * ED_H > n0 ? m * ED_H : n0;
      const long long hi = (m + 1) * ED_H < n0 + d.k ? (m + 1) * ED_H : n0 + d.k;
      for (long long n = lo + tid; n < hi; n += ED_T) yrow[n - n0] = n >= start && n < end ? far.sample(n - u) : 0.f;
    }
    if (m < mlo || m >= mhi) continue;                   // row-uniform
    const int slot = (int)(m % L1);
    const long long col = d.f_ring ? m % d.f_ring : m - d.frm0;

    if (m == mfirst) {                                   // the row's first frame: behind the barrier below for everyone else
      for (int i = tid; i < L1 * ED_BINS; i += ED_T) Cg[i] = make_double2(0.0, 0.0);
      if (tid == 0) s_pol[0] = -1, s_pol[1] = 0, s_pol[2] = -1, s_pol[3] = d.delay0, s_conf = 0.0;
    }
    // 1., 2.: the two windowed spectra and the two activities
    if (wave < 2) {
      const RingSrc& s = wave == 0 ? far : mic;
      double2* z = zb[wave];
      const long long base = (m - 1) * ED_H;
      double v[ED_N / 64];
#pragma unroll
      for (int r = 0; r < ED_N / 64; ++r) {
        const int n = lane + 64 * r;
        const double f = (double)s.sample(base + n);
        v[r] = f * f;
        z[n] = make_double2(win[n] * f, 0.0);
      }
      double sum = ((v[0] + v[4]) + (v[2] + v[6])) + ((v[1] + v[5]) + (v[3] + v[7]));
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) sum = sum + __shfl_down(sum, off);
      const int active = sum / (double)ED_N > d.gate ? 1 : 0;
      fft512_forward(z, tw, lane);
      if (wave == 0) {
        for (int k = d.k_lo + lane; k < d.k_hi; k += 64) Xg[slot * ED_BINS + k] = z[fft512_rev(k)];
        if (lane == 0) s_act[slot] = active, actg[slot] = active, s_now[0] = active;
      } else if (lane == 0) {
        s_now[1] = active;
      }
    }
    __syncthreads();
    // 3., 4.: one wave per lag
    const bool actd = s_now[1] != 0;
    for (int l = wave; l < L1; l += ED_WAVES) {
      const long long ml = m - l;
      const bool upd = actd && ml >= mfirst && s_act[ml % L1] != 0;
      const int xs = upd ? (int)(ml % L1) : 0;
      double v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = lane + 64 * r;
        v[r] = 0.0;
        if (j < nb) {
          const int k = d.k_lo + j;
          double2 c = Cg[l * ED_BINS + k];
          if (upd) {
            const double2 x = Xg[xs * ED_BINS + k], dd = zb[1][fft512_rev(k)];
            const double pr = x.x * dd.x + x.y * dd.y, pi = x.x * dd.y - x.y * dd.x;
            const double den = sqrt(x.x * x.x + x.y * x.y) * sqrt(dd.x * dd.x + dd.y * dd.y) + d.eps;
            c = make_double2(oma * c.x + ca * (pr / den), oma * c.y + ca * (pi / den));
            Cg[l * ED_BINS + k] = c;
          }
          v[r] = c.x * c.x + c.y * c.y;
        }
      }
      double s = (v[0] + v[2]) + (v[1] + v[3]);
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_down(s, off);
      if (lane == 0) {
        s = s / (double)nb;
        sc[l] = s;
        if (d.score) d.score[(frow_out + col) * L1 + l] = s;
      }
    }
    __syncthreads();
    // 5. to 8.
    if (wave == 0) {
      int ls = 0;
      double conf = sc[0];
      for (int l = 1; l < L1; ++l) {
        const double s = sc[l];
        if (s > conf) conf = s, ls = l;
      }
      double2* z = zb[0];
#pragma unroll
      for (int r = 0; r < ED_N / 64; ++r) z[lane + 64 * r] = make_double2(0.0, 0.0);
      fft512_wave_sync();
      for (int k = d.k_lo + lane; k < d.k_hi; k += 64) {
        double2 c = Cg[ls * ED_BINS + k];
        if (k == 0 || k == ED_H) c.y = 0.0;
        z[fft512_rev(k)] = c;
        if (k >= 1 && k < ED_H) z[fft512_rev(ED_N - k)] = make_double2(c.x, -c.y);
      }
      fft512_inverse(z, tw, lane);
      double bv = -1.0;
      int bn = 0;
#pragma unroll
      for (int r = 0; r < ED_N / 64; ++r) {
        const int n = lane + 64 * r;
        const double av = fabs(z[n].x);
        if (av > bv) bv = av, bn = n;
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const int on = __shfl_xor(bn, off);
        if (ov > bv || (ov == bv && on < bn)) bv = ov, bn = on;
      }
      const int rr = bn < ED_H ? bn : bn - ED_N;
      const int raw = ls * ED_H + rr > 0 ? ls * ED_H + rr : 0;
      const long long ml = m - ls;
      const bool ok = conf >= d.thr && actd && ml >= mfirst && s_act[ml % L1] != 0;
      int cand = s_pol[0], run = s_pol[1], locked = s_pol[2];
      if (ok) {
        const int dist = raw > cand ? raw - cand : cand - raw;
        if (cand >= 0 && dist <= d.tol) run += 1;
        else cand = raw, run = 1;
      }
      if (run >= d.hold) {
        const int dist = cand > locked ? cand - locked : locked - cand;
        if (locked < 0 || dist >= d.move) locked = cand;
      }
      const int used = locked < 0 ? d.delay0 : (locked - d.margin > 0 ? locked - d.margin : 0);
      fft512_wave_sync();                                // every lane has read the old policy
      if (lane == 0) {
        s_pol[0] = cand, s_pol[1] = run, s_pol[2] = locked, s_pol[3] = used, s_conf = conf;
        if (d.raw) d.raw[frow_out + col] = raw;
        if (d.locked) d.locked[frow_out + col] = locked;
        if (d.used) d.used[frow_out + col] = used;
        if (d.conf) d.conf[frow_out + col] = conf;
        if (d.ok) d.ok[frow_out + col] = ok ? 1 : 0;
      }
    }
    __syncthreads();
  }

  __syncthreads();                                       // the last block's aligner has read the rings
  if (mring) ring_store(mring, FAC_EDELAY_MIC_RING, mrow, n0, d.k, tid);
  if (fring) ring_store(fring, d.far_rn, frow, n0, d.k, tid);
  if (mlo < mhi) {
    if (tid < FAC_EDELAY_POL) polg[tid] = s_pol[tid];
    if (tid == 0) d.conf_last[b] = s_conf;
  }
}

}  // namespace fac

using namespace fac;

extern "C" int fac_edelay_state_sizes(int max_delay, int64_t* sizes) {
  FAC_REQUIRE(sizes, "edelay_state_sizes: null sizes pointer");
  FAC_REQUIRE(max_delay >= 1 && max_delay <= FAC_EDELAY_MAX_DELAY, "edelay_state_sizes: max_delay = %d outside 1 .. %d samples", max_delay,
              (int)FAC_EDELAY_MAX_DELAY);
  const int L1 = ed_lags(max_delay);
  sizes[0] = sizes[1] = (int64_t)L1 * FAC_AEC_BINS * 2;
  sizes[2] = L1;
  sizes[3] = FAC_EDELAY_POL;
  sizes[4] = FAC_EDELAY_MIC_RING;
  sizes[5] = (int64_t)L1 * FAC_AEC_H + FAC_AEC_H - 1;
  return FAC_OK;
}

extern "C" int fac_edelay_run(const fac_edelay_desc* d, fac_stream_t stream) {
  FAC_REQUIRE(d, "edelay_run: null descriptor");
  FAC_REQUIRE(d->mic && d->far && d->y, "edelay_run: null mic, far or output pointer");
  FAC_REQUIRE(d->C && d->X && d->act && d->pol && d->conf_last, "edelay_run: null state pointer (C, X, act, pol or conf_last)");
  FAC_REQUIRE(d->B > 0 && d->B <= 65535, "edelay_run: B = %d outside 1 .. 65535", d->B);
  FAC_REQUIRE(d->k >= 1 && d->k <= (1 << 30), "edelay_run: k = %d outside 1 .. 2^30 samples", d->k);
  FAC_REQUIRE(d->max_delay >= 1 && d->max_delay <= FAC_EDELAY_MAX_DELAY, "edelay_run: max_delay = %d outside 1 .. %d samples", d->max_delay,
              (int)FAC_EDELAY_MAX_DELAY);
  FAC_REQUIRE(d->k_lo >= 0 && d->k_lo < d->k_hi && d->k_hi <= FAC_AEC_BINS && d->k_hi - d->k_lo <= FAC_AEC_H,
              "edelay_run: band k_lo = %d, k_hi = %d (0 <= k_lo < k_hi <= 257, at most 256 bins)", d->k_lo, d->k_hi);
  FAC_REQUIRE(d->a > 0.0 && d->a <= 1.0, "edelay_run: a = %g outside (0, 1]", d->a);
  FAC_REQUIRE(d->eps > 0.0 && isfinite(d->eps), "edelay_run: eps = %g (finite, positive)", d->eps);
  FAC_REQUIRE(d->gate >= 0.0 && isfinite(d->gate), "edelay_run: gate = %g (finite, not negative)", d->gate);
  FAC_REQUIRE(d->thr >= 0.0 && isfinite(d->thr), "edelay_run: thr = %g (finite, not negative)", d->thr);
  FAC_REQUIRE(d->hold >= 1, "edelay_run: hold = %d below 1 frame", d->hold);
  FAC_REQUIRE(d->tol >= 0 && d->move >= 0 && d->margin >= 0, "edelay_run: tol = %d, move = %d, margin = %d (not negative)", d->tol, d->move, d->margin);
  FAC_REQUIRE(d->delay0 >= 0 && d->delay0 <= d->max_delay, "edelay_run: delay0 = %d outside 0 .. max_delay = %d", d->delay0, d->max_delay);
  FAC_REQUIRE(d->n0 >= 0, "edelay_run: n0 = %lld (not negative)", (long long)d->n0);
  const long long first = d->n0 / FAC_AEC_H > 1 ? d->n0 / FAC_AEC_H : 1;
  FAC_REQUIRE(d->frm0 >= first, "edelay_run: frm0 = %lld below max(n0 / 256, 1) = %lld", (long long)d->frm0, first);
  FAC_REQUIRE(d->n_frm >= 0 && d->n_frm <= (1 << 22), "edelay_run: n_frm = %d outside 0 .. 2^22 frames", d->n_frm);
  FAC_REQUIRE(d->n_frm == 0 || (d->frm0 + d->n_frm) * (long long)FAC_AEC_H <= d->n0 + d->k,
              "edelay_run: frame %lld ends behind the call's last sample %lld", (long long)(d->frm0 + d->n_frm - 1), (long long)(d->n0 + d->k - 1));
  FAC_REQUIRE(!d->mic_ring == !d->far_ring, "edelay_run: one ring without the other");
  const int L1 = ed_lags(d->max_delay);
  FAC_REQUIRE(!d->far_ring || d->far_rn == L1 * FAC_AEC_H + FAC_AEC_H - 1, "edelay_run: far ring of %d samples, not 256 (L + 1) + 255 = %d", d->far_rn,
              L1 * FAC_AEC_H + FAC_AEC_H - 1);
  FAC_REQUIRE(!d->lens || !d->far_ring, "edelay_run: lens does not go with a carried stream");
  FAC_REQUIRE(d->f_ring >= 0 && (d->f_ring == 0 || d->f_ring >= d->n_frm), "edelay_run: f_ring = %d columns for n_frm = %d frames", d->f_ring, d->n_frm);
  FAC_REQUIRE(d->C != d->X, "edelay_run: C and X are the same buffer");
  const long long state = (long long)L1 * FAC_AEC_BINS * 2, cols = d->f_ring ? d->f_ring : d->n_frm;
  FAC_REQUIRE(d->B == 1 || (d->c_bs >= state && d->xr_bs >= state), "edelay_run: state pitches c_bs = %lld, xr_bs = %lld below 514 (L + 1) = %lld",
              (long long)d->c_bs, (long long)d->xr_bs, state);
  FAC_REQUIRE(d->B == 1 || (d->mic_bs >= d->k && d->far_bs >= d->k), "edelay_run: mic_bs = %lld or far_bs = %lld below k = %d", (long long)d->mic_bs,
              (long long)d->far_bs, d->k);
  FAC_REQUIRE(d->B == 1 || d->y_bs >= d->k, "edelay_run: y_bs = %lld below k = %d", (long long)d->y_bs, d->k);
  const bool per_frame = d->raw || d->locked || d->used || d->conf || d->ok || d->score;
  FAC_REQUIRE(d->B == 1 || !per_frame || d->f_bs >= cols, "edelay_run: f_bs = %lld below %lld columns", (long long)d->f_bs, cols);
  EdArgs a;
  a.d = *d;
  hipLaunchKernelGGL(edelay_kernel, dim3((unsigned)d->B), dim3(ED_T), 0, (hipStream_t)stream, a);
  return check_launch("edelay_run");
}
