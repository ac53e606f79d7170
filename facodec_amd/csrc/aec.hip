// Echo cancellation on the device: a partitioned-block frequency-domain adaptive filter, overlap-save, with a
// fully constrained gradient and a step normalised by the far-end power in the filter's span plus the error power.  Arithmetic,
// order and contracts: the header comment of include/facodec_hip.h.  All fp64 on the vector pipe, no matrix pipe, no atomics,
// every word has one writer; the build runs with -ffp-contract=off.
//
// The recursion is serial in time, so one 512-thread workgroup per row walks the blocks a call completes: the trip count is
// the row's, hence workgroup-uniform under every barrier.  Per block: wave 0 transforms the far-end frame (wave 1 fetches the
// microphone block meanwhile); one thread per bin forms the echo estimate's spectrum and the far-end power in the span; wave 0
// transforms it back, forms the error, writes the output and transforms the error; one thread per bin forms the step; wave w
// constrains and applies the gradient of partitions w, w + 8, ..  Five workgroup barriers per block (three on a row that does
// not adapt); the stages of a transform are ordered inside its wave (fft512_f64.h).  The same kernel, with the same per-block
// arithmetic, serves the offline call and a stream's push; only where W and the X ring live during the call differs:
// P <= FAC_AEC_LDS_P keeps them in LDS (aec_kernel<true>), a larger P works on the global buffers, which stay in L2.
#include "common.h"
#include "fft512_f64.h"
#include "stream_src.h"
#include <math.h>

namespace fac {

constexpr int AEC_T = 512, AEC_WAVES = AEC_T / 64;
constexpr int AEC_N = FAC_AEC_N, AEC_H = FAC_AEC_H, AEC_BINS = FAC_AEC_BINS;
constexpr int AEC_BINS_PAD = 264;
static_assert(AEC_N == FFT512_N && AEC_N == 2 * AEC_H && AEC_BINS == AEC_H + 1, "echo canceller geometry");
static_assert(FAC_AEC_MIC_CARRY == AEC_H - 1 && FAC_AEC_FAR_CARRY == AEC_N - 1 && FAC_AEC_LDS_P == AEC_WAVES, "echo canceller geometry");

struct AecArgs {
  fac_aec_desc d;
};

// fixed LDS: the twiddles, one transform buffer per wave, E, S / step, the microphone block, the three rows of squares
constexpr size_t AEC_LDS_FIXED = sizeof(double2) * (AEC_N / 2 + AEC_WAVES * AEC_N + AEC_BINS_PAD) + sizeof(double) * (AEC_BINS_PAD + AEC_H + 3 * AEC_H);
static size_t aec_lds(int P) { return AEC_LDS_FIXED + (P <= FAC_AEC_LDS_P ? (size_t)2 * P * AEC_BINS * sizeof(double2) : 0); }

template <bool RES>
__global__ __launch_bounds__(AEC_T) void aec_kernel(AecArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char aec_smem[];
  const fac_aec_desc& d = a.d;
  const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int P = d.P;
  const StreamSrc mic = stream_src(d.mic_carry_in, FAC_AEC_MIC_CARRY, d.mic, d.mic_bs, d.lens, d.starts, d.n0, d.k, b);
  const StreamSrc far = stream_src_like(mic, d.far_carry_in, d.far_cn, d.far, d.far_bs, b);
  const long long start = mic.start, end = mic.end;

  if (blockIdx.x == 1) {                                 // the row's next carries
    if (d.mic_carry_out) stream_carry_out(mic, d.mic_carry_out, d.k, b, tid, AEC_T);
    if (d.far_carry_out) stream_carry_out(far, d.far_carry_out, d.k, b, tid, AEC_T);
    return;
  }

  double2* tw = reinterpret_cast<double2*>(aec_smem);
  double2* buf = tw + AEC_N / 2;                         // [AEC_WAVES][AEC_N]
  double2* Es = buf + AEC_WAVES * AEC_N;                 // [AEC_BINS_PAD]
  double* stp = reinterpret_cast<double*>(Es + AEC_BINS_PAD);   // [AEC_BINS_PAD]: S, then step
  double* dm = stp + AEC_BINS_PAD;                       // [AEC_H]
  double* sq = dm + AEC_H;                               // [3][AEC_H]
  double2* Wg = reinterpret_cast<double2*>(d.W + (long long)b * d.w_bs);
  double2* Xg = reinterpret_cast<double2*>(d.X + (long long)b * d.xr_bs);
  double2* W = RES ? reinterpret_cast<double2*>(sq + 3 * AEC_H) : Wg;
  double2* X = RES ? W + P * AEC_BINS : Xg;

  const long long ms = start / AEC_H;
  const long long m_row = (end + AEC_H - 1) / AEC_H;
  const long long mlo = d.blk0 > ms ? d.blk0 : ms;
  long long mhi = d.blk0 + d.n_blk < m_row ? d.blk0 + d.n_blk : m_row;
  if (mhi < mlo) mhi = mlo;
  float* yrow = d.y + (long long)b * d.y_bs;
  float* ring = d.e_ring ? d.e_ring + (long long)b * AEC_H : nullptr;
  double* srow = d.stats ? d.stats + (long long)b * d.s_bs : nullptr;

  // every output that no block of this call writes: an e of an earlier call from the ring, else 0
  for (int i = tid; i < d.n_out; i += AEC_T) {
    const long long n = d.m0 + i;
    if (n >= mlo * AEC_H && n < mhi * AEC_H) continue;
    float v = 0.f;
    if (ring && n >= 0 && n >= start && n < end && n < d.blk0 * AEC_H && n >= d.blk0 * AEC_H - AEC_H) v = ring[n & (AEC_H - 1)];
    yrow[i] = v;
  }
  if (srow) {
    for (int i = tid; i < 3 * d.n_blk; i += AEC_T) {
      const long long m = d.blk0 + i / 3;
      if (m < mlo || m >= mhi) srow[i] = 0.0;
    }
  }
  if (mlo >= mhi) return;                                // row-uniform

  if (tid < AEC_N / 2) fft512_table(tw, tid);
  const bool fresh = mlo == ms;                          // the call holds the row's first block: W = 0, X_j = 0
  if (RES || fresh) {
    for (int i = tid; i < P * AEC_BINS; i += AEC_T) {
      W[i] = fresh ? make_double2(0.0, 0.0) : Wg[i];
      X[i] = fresh ? make_double2(0.0, 0.0) : Xg[i];
    }
  }
  const bool adapt = d.adapt ? d.adapt[b] != 0 : true;
  const double mu = d.mu, c = d.c, delta = d.delta;
  double2* z0 = buf;
  __syncthreads();

  for (long long m = mlo; m < mhi; ++m) {
    const int mm = (int)(m % P);
    // 1. X_m
    if (wave == 0) {
      const long long base = (m - 1) * AEC_H - d.delay;
#pragma unroll
      for (int r = 0; r < AEC_N / 64; ++r) {
        const int n = lane + 64 * r;
        z0[n] = make_double2((double)far.sample(base + n), 0.0);
      }
      fft512_forward(z0, tw, lane);
      for (int k = lane; k < AEC_BINS; k += 64) X[mm * AEC_BINS + k] = z0[fft512_rev(k)];
    } else if (wave == 1) {
#pragma unroll
      for (int r = 0; r < AEC_H / 64; ++r) {
        const int n = lane + 64 * r;
        dm[n] = (double)mic.sample(m * AEC_H + n);
      }
    }
    __syncthreads();
    // 2. Yh and 6's S, one thread per bin; 3's full spectrum into wave 0's buffer
    if (tid < AEC_BINS) {
      const int k = tid;
      double yr = 0.0, yi = 0.0, S = 0.0;
      for (int p = 0; p < P; ++p) {
        const int slot = mm - p < 0 ? mm - p + P : mm - p;
        const double2 w = W[p * AEC_BINS + k], x = X[slot * AEC_BINS + k];
        const double pr = w.x * x.x - w.y * x.y, pi = w.x * x.y + w.y * x.x;
        yr = yr + pr, yi = yi + pi;
        S = S + (x.x * x.x + x.y * x.y);
      }
      if (k == 0 || k == AEC_H) yi = 0.0;
      z0[fft512_rev(k)] = make_double2(yr, yi);
      if (k >= 1 && k < AEC_H) z0[fft512_rev(AEC_N - k)] = make_double2(yr, -yi);
      stp[k] = S;
    }
    __syncthreads();
    // 3. to 5.
    if (wave == 0) {
      fft512_inverse(z0, tw, lane);
#pragma unroll
      for (int r = 0; r < AEC_H / 64; ++r) {
        const int n = lane + 64 * r;
        const long long idx = m * AEC_H + n;
        const bool real = idx < end;
        const double yh = real ? z0[AEC_H + n].x * (1.0 / AEC_N) : 0.0;
        const double dv = dm[n];
        const double e = real ? dv - yh : 0.0;
        sq[n] = dv * dv, sq[AEC_H + n] = yh * yh, sq[2 * AEC_H + n] = e * e;
        const float o = idx < start ? 0.f : (float)e;
        const long long i = idx - d.m0;
        if (i >= 0 && i < d.n_out) yrow[i] = o;
        else if (i >= d.n_out && ring) ring[idx & (AEC_H - 1)] = o;
        z0[n] = make_double2(0.0, 0.0);
        z0[AEC_H + n] = make_double2(e, 0.0);
      }
      if (adapt) fft512_forward(z0, tw, lane);
    }
    __syncthreads();
    // 8. one wave per sum: the two upper levels of the tree in the lane, the other six across the lanes
    if (srow && wave >= 1 && wave <= 3) {
      const double* v = sq + (wave - 1) * AEC_H;
      double s = (v[lane] + v[lane + 128]) + (v[lane + 64] + v[lane + 192]);
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_down(s, off);
      if (lane == 0) srow[(m - d.blk0) * 3 + (wave - 1)] = s;
    }
    if (!adapt) continue;                                // row-uniform
    // 6. the step
    if (tid < AEC_BINS) {
      const int k = tid;
      const double2 E = z0[fft512_rev(k)];
      const double den = (stp[k] + c * (E.x * E.x + E.y * E.y)) + delta;
      Es[k] = E;
      stp[k] = den == 0.0 ? 0.0 : mu / den;
    }
    __syncthreads();
    // 7. the constrained update, one wave per partition
    double2* z = buf + wave * AEC_N;
    for (int p = wave; p < P; p += AEC_WAVES) {
      const int slot = mm - p < 0 ? mm - p + P : mm - p;
      for (int k = lane; k < AEC_BINS; k += 64) {
        const double2 x = X[slot * AEC_BINS + k], E = Es[k];
        const double st = stp[k];
        const double gr = x.x * E.x + x.y * E.y, gi = x.x * E.y - x.y * E.x;
        double2 g = make_double2(st * gr, st * gi);
        if (k == 0 || k == AEC_H) g.y = 0.0;
        z[fft512_rev(k)] = g;
        if (k >= 1 && k < AEC_H) z[fft512_rev(AEC_N - k)] = make_double2(g.x, -g.y);
      }
      fft512_inverse(z, tw, lane);
#pragma unroll
      for (int r = 0; r < AEC_N / 64; ++r) {
        const int n = lane + 64 * r;
        z[n] = make_double2(n < AEC_H ? z[n].x * (1.0 / AEC_N) : 0.0, 0.0);
      }
      fft512_forward(z, tw, lane);
      for (int k = lane; k < AEC_BINS; k += 64) {
        const double2 g = z[fft512_rev(k)], w = W[p * AEC_BINS + k];
        W[p * AEC_BINS + k] = make_double2(w.x + g.x, w.y + g.y);
      }
    }
    __syncthreads();
  }

  if (RES) {                                             // behind the loop's last barrier
    for (int i = tid; i < P * AEC_BINS; i += AEC_T) Wg[i] = W[i], Xg[i] = X[i];
  }
}

}  // namespace fac

using namespace fac;

extern "C" int fac_aec_state_sizes(int P, int delay, int64_t* sizes) {
  FAC_REQUIRE(sizes, "aec_state_sizes: null sizes pointer");
  FAC_REQUIRE(P >= 1 && P <= FAC_AEC_MAX_P, "aec_state_sizes: P = %d outside 1 .. %d partitions", P, (int)FAC_AEC_MAX_P);
  FAC_REQUIRE(delay >= 0 && delay <= FAC_AEC_MAX_DELAY, "aec_state_sizes: delay = %d outside 0 .. %d samples", delay, (int)FAC_AEC_MAX_DELAY);
  sizes[0] = sizes[1] = (int64_t)P * FAC_AEC_BINS * 2;
  sizes[2] = FAC_AEC_MIC_CARRY;
  sizes[3] = FAC_AEC_FAR_CARRY + delay;
  sizes[4] = FAC_AEC_H;
  return FAC_OK;
}

extern "C" int fac_aec_run(const fac_aec_desc* d, fac_stream_t stream) {
  FAC_REQUIRE(d, "aec_run: null descriptor");
  FAC_REQUIRE(d->W && d->X && d->y, "aec_run: null W, X or output pointer");
  FAC_REQUIRE(d->B > 0 && d->B <= 65535, "aec_run: B = %d outside 1 .. 65535", d->B);
  FAC_REQUIRE(d->P >= 1 && d->P <= FAC_AEC_MAX_P, "aec_run: P = %d outside 1 .. %d partitions", d->P, (int)FAC_AEC_MAX_P);
  FAC_REQUIRE(d->mu >= 0.0 && d->mu <= 1.0, "aec_run: mu = %g outside [0, 1]", d->mu);
  FAC_REQUIRE(d->c >= 0.0 && isfinite(d->c), "aec_run: c = beta * P = %g (finite, not negative)", d->c);
  FAC_REQUIRE(d->delta >= 0.0 && isfinite(d->delta), "aec_run: delta = %g (finite, not negative)", d->delta);
  FAC_REQUIRE(d->delay >= 0 && d->delay <= FAC_AEC_MAX_DELAY, "aec_run: delay = %d outside 0 .. %d samples", d->delay, (int)FAC_AEC_MAX_DELAY);
  FAC_REQUIRE(d->k >= 0 && d->k <= (1 << 30), "aec_run: k = %d outside 0 .. 2^30 samples", d->k);
  FAC_REQUIRE((d->mic && d->far) || d->k == 0, "aec_run: null mic or far pointer with k = %d", d->k);
  FAC_REQUIRE(d->n_out >= 1 && d->n_out <= (1 << 30), "aec_run: n_out = %d outside 1 .. 2^30", d->n_out);
  FAC_REQUIRE(d->n_blk >= 0 && d->n_blk <= (1 << 22), "aec_run: n_blk = %d outside 0 .. 2^22 blocks", d->n_blk);
  FAC_REQUIRE(d->n0 >= 0 && d->blk0 >= 0, "aec_run: n0 = %lld, blk0 = %lld (not negative)", (long long)d->n0, (long long)d->blk0);
  const bool carried = d->mic_carry_in || d->mic_carry_out || d->far_carry_in || d->far_carry_out || d->e_ring;
  FAC_REQUIRE(!d->lens || !carried, "aec_run: lens does not go with a carried stream");
  FAC_REQUIRE(!d->mic_carry_out || d->mic_carry_out != d->mic_carry_in, "aec_run: mic_carry_out is mic_carry_in (the two buffers ping-pong)");
  FAC_REQUIRE(!d->far_carry_out || d->far_carry_out != d->far_carry_in, "aec_run: far_carry_out is far_carry_in (the two buffers ping-pong)");
  FAC_REQUIRE(d->W != d->X, "aec_run: W and X are the same buffer");
  FAC_REQUIRE(!(d->far_carry_in || d->far_carry_out) || d->far_cn >= FAC_AEC_FAR_CARRY + d->delay,
              "aec_run: far carry of %d samples below 511 + delay = %d", d->far_cn, (int)FAC_AEC_FAR_CARRY + d->delay);
  const long long state = (long long)d->P * FAC_AEC_BINS * 2;
  FAC_REQUIRE(d->B == 1 || (d->w_bs >= state && d->xr_bs >= state), "aec_run: state pitches w_bs = %lld, xr_bs = %lld below 514 P = %lld",
              (long long)d->w_bs, (long long)d->xr_bs, state);
  FAC_REQUIRE(d->B == 1 || (d->mic_bs >= d->k && d->far_bs >= d->k), "aec_run: mic_bs = %lld or far_bs = %lld below k = %d", (long long)d->mic_bs,
              (long long)d->far_bs, d->k);
  FAC_REQUIRE(d->B == 1 || d->y_bs >= d->n_out, "aec_run: y_bs = %lld below n_out = %d", (long long)d->y_bs, d->n_out);
  FAC_REQUIRE(d->B == 1 || !d->stats || d->s_bs >= 3LL * d->n_blk, "aec_run: s_bs = %lld below 3 n_blk = %d", (long long)d->s_bs, 3 * d->n_blk);
  // block blk0 reads the microphone from blk0 H and the far end from (blk0 - 1) H - delay: the carries must reach them
  FAC_REQUIRE(d->n_blk == 0 || !d->mic_carry_in || d->blk0 * (long long)FAC_AEC_H >= d->n0 - FAC_AEC_MIC_CARRY,
              "aec_run: block blk0 = %lld starts more than %d samples in front of n0 = %lld", (long long)d->blk0, (int)FAC_AEC_MIC_CARRY, (long long)d->n0);
  FAC_REQUIRE(d->n_blk == 0 || !d->far_carry_in || (d->blk0 - 1) * (long long)FAC_AEC_H - d->delay >= d->n0 - d->far_cn,
              "aec_run: block blk0 = %lld reaches in front of the far carry of %d samples before n0 = %lld", (long long)d->blk0, d->far_cn, (long long)d->n0);
  if (d->e_ring) {
    FAC_REQUIRE(d->m0 >= d->blk0 * (long long)FAC_AEC_H - FAC_AEC_H, "aec_run: output m0 = %lld lies more than 256 samples in front of block blk0 = %lld",
                (long long)d->m0, (long long)d->blk0);
    FAC_REQUIRE((d->blk0 + d->n_blk) * (long long)FAC_AEC_H - (d->m0 + d->n_out) <= FAC_AEC_H,
                "aec_run: more than 256 computed samples behind output %lld are not due: the ring holds 256", (long long)(d->m0 + d->n_out));
  }
  AecArgs a;
  a.d = *d;
  const dim3 grid(d->mic_carry_out || d->far_carry_out ? 2u : 1u, (unsigned)d->B);
  const size_t lds = aec_lds(d->P);
  if (d->P <= FAC_AEC_LDS_P) {
    allow_dynamic_lds<aec_kernel<true>>();
    hipLaunchKernelGGL(aec_kernel<true>, grid, dim3(AEC_T), lds, (hipStream_t)stream, a);
  } else {
    allow_dynamic_lds<aec_kernel<false>>();
    hipLaunchKernelGGL(aec_kernel<false>, grid, dim3(AEC_T), lds, (hipStream_t)stream, a);
  }
  return check_launch("aec_run");
}
