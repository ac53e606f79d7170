// Packet-loss concealment on the device: fac_plc_select substitutes, per row, the codes a push is decoded from
// (primary, the redundant low-rate copy, or the last played frame) and advances the per-row gain state; fac_plc_gain applies the
// resulting piecewise-linear gain to the decoded wave.  State machines and contracts: the header comment of
// include/facodec_hip.h.  Both are store/bandwidth kernels: no LDS, no matrix pipe, no atomics.
#include "common.h"

namespace fac {

struct PlcArgs {
  const long long* prim[3];
  long long prim_bs[3], prim_qs[3];
  const long long* red[3];
  long long red_bs[3], red_qs[3];
  long long* dst[3];
  long long dst_bs[3], dst_qs[3];
  int n_q[3], n_red[3];
  const int* status;
  long long* last_codes;
  int* last_n;
  float* g;
  int* run;
  int* n_use;
  long long n_use_bs, n_use_ts;
  float* ramp;
  int B, k, Q, hold, fade, recover, have_red;
};

// Thread j of row b: j < Q walks the k frames of quantizer j, j == Q does the counts and the gain recurrence.  A row's status
// word is read by all of its threads; every other word has one reader-writer.
__global__ __launch_bounds__(256) void plc_select_kernel(PlcArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.B * (a.Q + 1)) return;
  const int b = i / (a.Q + 1), j = i - b * (a.Q + 1);
  int st = a.status[b];
  if (st != FAC_PLC_PRIMARY && !(st == FAC_PLC_REDUNDANT && a.have_red)) st = FAC_PLC_LOST;
  if (j < a.Q) {
    const int r = j < a.n_q[0] ? 0 : (j < a.n_q[0] + a.n_q[1] ? 1 : 2);
    const int qi = j - (r > 0 ? a.n_q[0] : 0) - (r > 1 ? a.n_q[1] : 0);
    long long* dp = a.dst[r] + (long long)b * a.dst_bs[r] + (long long)qi * a.dst_qs[r];
    long long* lc = a.last_codes + (long long)b * a.Q + j;
    if (st == FAC_PLC_LOST) {
      const long long v = *lc;
      for (int f = 0; f < a.k; ++f) dp[f] = v;
    } else if (st == FAC_PLC_PRIMARY || qi < a.n_red[r]) {
      const long long* sp = st == FAC_PLC_PRIMARY ? a.prim[r] + (long long)b * a.prim_bs[r] + (long long)qi * a.prim_qs[r]
                                                  : a.red[r] + (long long)b * a.red_bs[r] + (long long)qi * a.red_qs[r];
      long long v = 0;
      for (int f = 0; f < a.k; ++f) {
        v = sp[f];
        dp[f] = v;
      }
      *lc = v;
    } else {
      for (int f = 0; f < a.k; ++f) dp[f] = 0;
    }
    return;
  }
  int n[3];
  for (int r = 0; r < 3; ++r)
    n[r] = st == FAC_PLC_PRIMARY ? a.n_q[r] : (st == FAC_PLC_REDUNDANT ? a.n_red[r] : a.last_n[b * 3 + r]);
  if (st != FAC_PLC_LOST)
    for (int r = 0; r < 3; ++r) a.last_n[b * 3 + r] = n[r];
  int* nu = a.n_use + (long long)b * a.n_use_bs;
  float* rp = a.ramp + (long long)b * (a.k + 1);
  float g = a.g[b];
  int run = a.run[b];
  const float down = __fdiv_rn(1.0f, (float)a.fade), up = __fdiv_rn(1.0f, (float)a.recover);
  rp[0] = g;
  for (int f = 0; f < a.k; ++f) {
    for (int r = 0; r < 3; ++r) nu[(long long)f * a.n_use_ts + r] = n[r];
    if (st == FAC_PLC_LOST) {
      run += 1;
      if (run > a.hold) g = fmaxf(0.0f, __fsub_rn(g, down));
    } else {
      run = 0;
      g = fminf(1.0f, __fadd_rn(g, up));
    }
    rp[f + 1] = g;
  }
  a.g[b] = g;
  a.run[b] = run;
}

__global__ __launch_bounds__(256) void plc_gain_kernel(const float* __restrict__ x, long long x_bs, float* y, long long y_bs,
                                                       const float* __restrict__ ramp, int B, int k, int frame) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int row = k * frame;
  if (i >= B * row) return;
  const int b = i / row, s = i - b * row;
  const int f = s / frame, n = s - f * frame;
  const float r0 = ramp[b * (k + 1) + f], r1 = ramp[b * (k + 1) + f + 1];
  const float t = __fdiv_rn((float)(n + 1), (float)frame);
  const float gain = __fadd_rn(r0, __fmul_rn(__fsub_rn(r1, r0), t));
  y[(long long)b * y_bs + s] = __fmul_rn(x[(long long)b * x_bs + s], gain);
}

}  // namespace fac

using namespace fac;

extern "C" int fac_plc_select(const fac_plc_select_desc* d, fac_stream_t stream) {
  FAC_REQUIRE(d, "plc_select: null descriptor");
  FAC_REQUIRE(d->status && d->last_codes && d->last_n && d->g && d->run, "plc_select: null status or state pointer");
  FAC_REQUIRE(d->n_use && d->ramp, "plc_select: null n_use or ramp");
  FAC_REQUIRE(d->B > 0 && d->B <= (1 << 20), "plc_select: B = %d outside 1 .. 2^20", d->B);
  FAC_REQUIRE(d->k >= 1 && d->k <= FAC_PLC_MAX_FRAMES, "plc_select: k = %d outside 1 .. %d", d->k, FAC_PLC_MAX_FRAMES);
  FAC_REQUIRE(d->hold >= 0 && d->fade >= 1 && d->recover >= 1, "plc_select: policy (hold=%d fade=%d recover=%d): hold >= 0, fade >= 1, recover >= 1",
              d->hold, d->fade, d->recover);
  PlcArgs a;
  int Q = 0, n_red = 0;
  for (int r = 0; r < 3; ++r) {
    FAC_REQUIRE(d->n_q[r] >= 0 && d->n_red[r] >= 0, "plc_select: negative quantizer count of RVQ %d", r);
    FAC_REQUIRE(d->n_red[r] <= d->n_q[r], "plc_select: RVQ %d has %d redundant quantizers but %d primary", r, d->n_red[r], d->n_q[r]);
    FAC_REQUIRE(d->n_q[r] == 0 || (d->prim[r] && d->dst[r]), "plc_select: RVQ %d has %d quantizers but no primary or destination codes", r,
                d->n_q[r]);
    FAC_REQUIRE(d->n_red[r] == 0 || d->red[r], "plc_select: RVQ %d has %d redundant quantizers but no redundant codes", r, d->n_red[r]);
    Q += d->n_q[r];
    n_red += d->n_red[r];
    a.prim[r] = reinterpret_cast<const long long*>(d->prim[r]); a.prim_bs[r] = d->prim_bs[r]; a.prim_qs[r] = d->prim_qs[r];
    a.red[r] = reinterpret_cast<const long long*>(d->red[r]); a.red_bs[r] = d->red_bs[r]; a.red_qs[r] = d->red_qs[r];
    a.dst[r] = reinterpret_cast<long long*>(d->dst[r]); a.dst_bs[r] = d->dst_bs[r]; a.dst_qs[r] = d->dst_qs[r];
    a.n_q[r] = d->n_q[r];
    a.n_red[r] = d->n_red[r];
  }
  FAC_REQUIRE(Q >= 1 && Q <= FAC_VQ_DECODE_MAX_Q, "plc_select: %d quantizers (1 .. %d)", Q, FAC_VQ_DECODE_MAX_Q);
  FAC_REQUIRE((d->B == 1 || d->n_use_bs > 0) && (d->k == 1 || d->n_use_ts > 0),
              "plc_select: n_use strides (%lld, %lld) cannot address (B = %d, k = %d, 3)", (long long)d->n_use_bs, (long long)d->n_use_ts,
              d->B, d->k);
  a.status = d->status;
  a.last_codes = reinterpret_cast<long long*>(d->last_codes);
  a.last_n = d->last_n;
  a.g = d->g;
  a.run = d->run;
  a.n_use = d->n_use;
  a.n_use_bs = d->n_use_bs;
  a.n_use_ts = d->n_use_ts;
  a.ramp = d->ramp;
  a.B = d->B; a.k = d->k; a.Q = Q; a.hold = d->hold; a.fade = d->fade; a.recover = d->recover; a.have_red = n_red > 0;
  const int n = d->B * (Q + 1);
  hipLaunchKernelGGL(plc_select_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("plc_select");
}

extern "C" int fac_plc_gain(const float* x, int64_t x_bs, float* y, int64_t y_bs, const float* ramp, int B, int k, int frame,
                            fac_stream_t stream) {
  FAC_REQUIRE(x && y && ramp, "plc_gain: null pointer");
  FAC_REQUIRE(B > 0 && k > 0 && frame > 0, "plc_gain: bad shape (B=%d k=%d frame=%d)", B, k, frame);
  const long long row = (long long)k * frame;
  FAC_REQUIRE(row * B < (1ll << 31), "plc_gain: %d x %d x %d samples (below 2^31)", B, k, frame);
  FAC_REQUIRE(x_bs >= row && y_bs >= row, "plc_gain: row pitches (%lld, %lld) below %lld samples", (long long)x_bs, (long long)y_bs, row);
  const long long n = row * B;
  hipLaunchKernelGGL(plc_gain_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (long long)x_bs, y,
                     (long long)y_bs, ramp, B, k, frame);
  return check_launch("plc_gain");
}
