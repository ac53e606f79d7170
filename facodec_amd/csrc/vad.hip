// Voice activity on the device: fac_vad_energy sums the pre-emphasised power of every frame in fp64 in a fixed
// order (one 64-lane wave per frame) and carries the unprocessed tail of a stream from one carry buffer into the other;
// fac_vad_decide turns a ring of frame energies into flags (minimum statistics over a finite window, a finite hangover, no
// recurrence); fac_vad_take gathers flags out of the flag ring; fac_sid_apply stores and replays the codes of a silence
// descriptor for the receiver's comfort frames.  Arithmetic, order and contracts: the header comment of include/facodec_hip.h.
// All four are small bandwidth kernels: no matrix pipe, no atomics, every word has one writer.
#include "common.h"

namespace fac {

constexpr int VAD_WAVES = 4;                     // frames per workgroup of vad_energy_kernel
constexpr int VAD_TILE = 256;                    // frames per workgroup of vad_decide_kernel

struct VadEnergyArgs {
  const float* carry_in;
  float* carry_out;
  const float* x;
  const int* lens;
  double* e;
  long long x_bs, e_bs, f0;
  int B, k, frame, carry_n, n_frames, n_whole, R, frame_blocks;
};

// Sample s of row b of the virtual concatenation [carry | block]; s = -1 is the sample before the first unprocessed one.
__device__ __forceinline__ float vad_sample(const VadEnergyArgs& a, int b, long long s) {
  if (s < a.carry_n) return a.carry_in ? a.carry_in[(long long)b * a.frame + 1 + s] : 0.0f;
  return a.x[(long long)b * a.x_bs + (s - a.carry_n)];
}

// blockIdx.x < frame_blocks: wave w of the block sums frame blockIdx.x * VAD_WAVES + w.  blockIdx.x == frame_blocks: the block
// writes the row's next carry.  carry_out is never carry_in (refused on the host), e and x are read-only / write-only here.
__global__ __launch_bounds__(64 * VAD_WAVES) void vad_energy_kernel(VadEnergyArgs a) {
  const int b = blockIdx.y;
  const long long total = (long long)a.carry_n + a.k;
  if ((int)blockIdx.x == a.frame_blocks) {
    if (!a.carry_out) return;
    const long long base = (long long)a.n_whole * a.frame;
    const int rem = (int)(total - base);                              // 0 .. frame - 1 unprocessed samples
    for (int i = threadIdx.x; i <= rem; i += 64 * VAD_WAVES)
      a.carry_out[(long long)b * a.frame + i] = vad_sample(a, b, base + i - 1);
    return;
  }
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * VAD_WAVES + (threadIdx.x >> 6);
  if (f >= a.n_frames) return;
  long long n_valid = total;
  if (a.lens) {
    const long long len = a.lens[b];
    n_valid = len < 0 ? 0 : (len < total ? len : total);
  }
  const long long s0 = (long long)f * a.frame;
  double acc = 0.0;
  for (int n = lane; n < a.frame && s0 + n < n_valid; n += 64) {
    const double cur = (double)vad_sample(a, b, s0 + n);
    const double prev = (double)vad_sample(a, b, s0 + n - 1);
    const double d = __dsub_rn(cur, __dmul_rn(0.97, prev));
    acc = __dadd_rn(acc, __dmul_rn(d, d));
  }
  for (int dist = 32; dist >= 1; dist >>= 1) acc = __dadd_rn(acc, __shfl_xor(acc, dist, 64));
  if (lane == 0) a.e[(long long)b * a.e_bs + (a.f0 + f) % a.R] = acc;
}

struct VadDecideArgs {
  const double* e;
  const int* lens;
  unsigned char* flags;
  unsigned char* ring;
  long long e_bs, flags_bs, ring_bs, f0;
  double margin, thr_abs;
  int B, n_new, R, W, H, frame;
};

// One workgroup per (row, tile of VAD_TILE new frames).  LDS: the energies of the tile and its W - 1 + H older neighbours, then
// raw[] of the tile and its H older neighbours; global frame g sits at e_s[g - lo], lo = t0 - H - W + 1 (entries with g < 0 are
// never read).
__global__ __launch_bounds__(VAD_TILE) void vad_decide_kernel(VadDecideArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char vad_lds[];
  double* e_s = reinterpret_cast<double*>(vad_lds);
  const int n_e = VAD_TILE + a.W - 1 + a.H;
  unsigned char* raw_s = vad_lds + (size_t)n_e * sizeof(double);
  const int b = blockIdx.y;
  const int i0 = blockIdx.x * VAD_TILE;                               // first new frame of the tile, relative to f0
  const int n_t = a.n_new - i0 < VAD_TILE ? a.n_new - i0 : VAD_TILE;
  const long long t0 = a.f0 + i0;
  const long long lo = t0 - a.H - a.W + 1;
  for (int j = threadIdx.x; j < n_e - (VAD_TILE - n_t); j += VAD_TILE) {
    const long long g = lo + j;
    e_s[j] = g >= 0 ? a.e[(long long)b * a.e_bs + g % a.R] : 0.0;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < a.H + n_t; j += VAD_TILE) {
    const long long g = t0 - a.H + j;
    unsigned char r = 0;
    if (g >= 0) {
      const int at = (int)(g - lo);
      const double eg = e_s[at];
      double mn = eg;
      for (int w = 1; w < a.W && g - w >= 0; ++w) mn = fmin(mn, e_s[at - w]);
      r = (eg > a.thr_abs && eg > __dmul_rn(a.margin, mn)) ? 1 : 0;
    }
    raw_s[j] = r;
  }
  __syncthreads();
  const int i = threadIdx.x;
  if (i >= n_t) return;
  const long long g = t0 + i;
  unsigned char act = 0;
  for (int h = 0; h <= a.H; ++h) act |= raw_s[a.H + i - h];           // raw_s of g - h; 0 where g - h < 0
  if (a.lens) {
    const long long len = a.lens[b];
    const long long n_row = len <= 0 ? 0 : (len + a.frame - 1) / a.frame;
    if (g >= n_row) act = 0;
  }
  if (a.flags) a.flags[(long long)b * a.flags_bs + i0 + i] = act;
  if (a.ring) a.ring[(long long)b * a.ring_bs + g % a.R] = act;
}

__global__ __launch_bounds__(256) void vad_take_kernel(const unsigned char* __restrict__ ring, long long ring_bs, int R, long long f0,
                                                       int k, unsigned char* out, long long out_bs, int B) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * k) return;
  const int b = i / k, j = i - b * k;
  out[(long long)b * out_bs + j] = ring[(long long)b * ring_bs + (f0 + j) % R];
}

struct SidArgs {
  long long* dst[3];
  long long dst_bs[3], dst_qs[3];
  int n_q[3];
  const int* mode;
  long long* sid_codes;
  int B, k, Q;
};

// Thread (row b, quantizer j): the only reader and writer of sid_codes[b, j, :] and of its k destination words.
__global__ __launch_bounds__(256) void sid_apply_kernel(SidArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.B * a.Q) return;
  const int b = i / a.Q, j = i - b * a.Q;
  const int m = a.mode[b];
  const int kind = m & 0xff, phase = (m >> 8) & 0xff, sid_k = (m >> 16) & 0xff;
  if (kind != FAC_SID_STORE && kind != FAC_SID_FILL) return;
  const int r = j < a.n_q[0] ? 0 : (j < a.n_q[0] + a.n_q[1] ? 1 : 2);
  const int qi = j - (r > 0 ? a.n_q[0] : 0) - (r > 1 ? a.n_q[1] : 0);
  long long* dp = a.dst[r] + (long long)b * a.dst_bs[r] + (long long)qi * a.dst_qs[r];
  long long* sc = a.sid_codes + ((long long)b * a.Q + j) * FAC_PLC_MAX_FRAMES;
  if (kind == FAC_SID_STORE) {
    for (int f = 0; f < a.k; ++f) sc[f] = dp[f];
  } else if (sid_k >= 1 && sid_k <= FAC_PLC_MAX_FRAMES) {             // a FILL without a stored descriptor touches nothing
    for (int f = 0; f < a.k; ++f) dp[f] = sc[(phase + f) % sid_k];
  }
}

}  // namespace fac

using namespace fac;

extern "C" int fac_vad_energy(const fac_vad_energy_desc* d, fac_stream_t stream) {
  FAC_REQUIRE(d, "vad_energy: null descriptor");
  FAC_REQUIRE(d->x && d->e, "vad_energy: null block or energy pointer");
  FAC_REQUIRE(d->B > 0 && d->B <= 65535, "vad_energy: B = %d outside 1 .. 65535", d->B);
  FAC_REQUIRE(d->frame >= 1 && d->frame <= FAC_VAD_MAX_FRAME, "vad_energy: frame = %d outside 1 .. %d", d->frame, FAC_VAD_MAX_FRAME);
  FAC_REQUIRE(d->k >= 1 && d->k <= (1 << 30), "vad_energy: k = %d outside 1 .. 2^30 samples", d->k);
  FAC_REQUIRE(d->carry_n >= 0 && d->carry_n < d->frame, "vad_energy: carry_n = %d outside 0 .. frame - 1 = %d", d->carry_n, d->frame - 1);
  FAC_REQUIRE(d->carry_n == 0 || d->carry_in, "vad_energy: carry_n = %d without a carry buffer", d->carry_n);
  FAC_REQUIRE(!d->carry_out || d->carry_out != d->carry_in, "vad_energy: carry_out is carry_in (the two buffers ping-pong)");
  FAC_REQUIRE(!d->lens || (!d->carry_in && !d->carry_out), "vad_energy: lens does not go with a carried stream");
  FAC_REQUIRE(d->x_bs >= d->k || d->B == 1, "vad_energy: x_bs = %lld below k = %d", (long long)d->x_bs, d->k);
  FAC_REQUIRE(d->f0 >= 0, "vad_energy: f0 = %lld is negative", (long long)d->f0);
  const long long total = (long long)d->carry_n + d->k;
  const int n_whole = (int)(total / d->frame);
  const int n_frames = n_whole + ((d->is_final && total % d->frame) ? 1 : 0);
  FAC_REQUIRE(d->R >= 1 && d->R >= n_frames, "vad_energy: R = %d below the %d frames of this call", d->R, n_frames);
  FAC_REQUIRE(d->e_bs >= d->R || d->B == 1, "vad_energy: e_bs = %lld below R = %d", (long long)d->e_bs, d->R);
  VadEnergyArgs a;
  a.carry_in = d->carry_in; a.carry_out = d->carry_out; a.x = d->x; a.lens = d->lens; a.e = d->e;
  a.x_bs = d->x_bs; a.e_bs = d->e_bs; a.f0 = d->f0;
  a.B = d->B; a.k = d->k; a.frame = d->frame; a.carry_n = d->carry_n; a.n_frames = n_frames; a.n_whole = n_whole; a.R = d->R;
  a.frame_blocks = (n_frames + VAD_WAVES - 1) / VAD_WAVES;
  if (a.frame_blocks == 0 && !d->carry_out) return FAC_OK;
  hipLaunchKernelGGL(vad_energy_kernel, dim3((unsigned)(a.frame_blocks + 1), (unsigned)d->B), dim3(64 * VAD_WAVES), 0,
                     (hipStream_t)stream, a);
  return check_launch("vad_energy");
}

extern "C" int fac_vad_decide(const fac_vad_decide_desc* d, fac_stream_t stream) {
  FAC_REQUIRE(d, "vad_decide: null descriptor");
  FAC_REQUIRE(d->e, "vad_decide: null energy pointer");
  FAC_REQUIRE(d->flags || d->ring, "vad_decide: neither flags nor a flag ring to write");
  FAC_REQUIRE(d->B > 0 && d->B <= 65535, "vad_decide: B = %d outside 1 .. 65535", d->B);
  FAC_REQUIRE(d->n_new >= 1, "vad_decide: n_new = %d (at least one frame)", d->n_new);
  FAC_REQUIRE(d->W >= 1 && d->W <= FAC_VAD_MAX_WINDOW, "vad_decide: W = %d outside 1 .. %d", d->W, FAC_VAD_MAX_WINDOW);
  FAC_REQUIRE(d->H >= 0 && d->H <= FAC_VAD_MAX_WINDOW, "vad_decide: H = %d outside 0 .. %d", d->H, FAC_VAD_MAX_WINDOW);
  FAC_REQUIRE(d->margin > 1.0, "vad_decide: margin = %g (a power ratio above 1)", d->margin);
  FAC_REQUIRE(d->thr_abs >= 0.0, "vad_decide: thr_abs = %g is negative", d->thr_abs);
  FAC_REQUIRE(d->f0 >= 0, "vad_decide: f0 = %lld is negative", (long long)d->f0);
  FAC_REQUIRE(d->frame >= 1 && d->frame <= FAC_VAD_MAX_FRAME, "vad_decide: frame = %d outside 1 .. %d", d->frame, FAC_VAD_MAX_FRAME);
  // nothing older than frame f0 + n_new - R is in the ring any more; a frame's window reaches W + H - 1 frames back
  const long long seen = d->f0 + d->n_new, need = (long long)d->W + d->H + d->n_new;
  FAC_REQUIRE(d->R >= 1 && d->R >= (seen < need ? seen : need), "vad_decide: R = %d below W + H + n_new = %d + %d + %d", d->R, d->W,
              d->H, d->n_new);
  FAC_REQUIRE(d->e_bs >= d->R || d->B == 1, "vad_decide: e_bs = %lld below R = %d", (long long)d->e_bs, d->R);
  FAC_REQUIRE(!d->flags || d->flags_bs >= d->n_new || d->B == 1, "vad_decide: flags_bs = %lld below n_new = %d", (long long)d->flags_bs,
              d->n_new);
  FAC_REQUIRE(!d->ring || d->ring_bs >= d->R || d->B == 1, "vad_decide: ring_bs = %lld below R = %d", (long long)d->ring_bs, d->R);
  VadDecideArgs a;
  a.e = d->e; a.lens = d->lens; a.flags = d->flags; a.ring = d->ring;
  a.e_bs = d->e_bs; a.flags_bs = d->flags_bs; a.ring_bs = d->ring_bs; a.f0 = d->f0;
  a.margin = d->margin; a.thr_abs = d->thr_abs;
  a.B = d->B; a.n_new = d->n_new; a.R = d->R; a.W = d->W; a.H = d->H; a.frame = d->frame;
  const size_t lds = (size_t)(VAD_TILE + d->W - 1 + d->H) * sizeof(double) + (size_t)(VAD_TILE + d->H);
  hipLaunchKernelGGL(vad_decide_kernel, dim3((unsigned)((d->n_new + VAD_TILE - 1) / VAD_TILE), (unsigned)d->B), dim3(VAD_TILE), lds,
                     (hipStream_t)stream, a);
  return check_launch("vad_decide");
}

extern "C" int fac_vad_take(const uint8_t* ring, int64_t ring_bs, int R, int64_t f0, int k, uint8_t* out, int64_t out_bs, int B,
                            fac_stream_t stream) {
  FAC_REQUIRE(ring && out, "vad_take: null pointer");
  FAC_REQUIRE(B > 0 && k > 0 && R > 0 && (long long)B * k < (1ll << 31), "vad_take: bad shape (B=%d k=%d R=%d)", B, k, R);
  FAC_REQUIRE(k <= R && f0 >= 0, "vad_take: %d frames from %lld do not lie in a ring of %d", k, (long long)f0, R);
  FAC_REQUIRE(B == 1 || (ring_bs >= R && out_bs >= k), "vad_take: row pitches (%lld, %lld) below (%d, %d)", (long long)ring_bs,
              (long long)out_bs, R, k);
  hipLaunchKernelGGL(vad_take_kernel, dim3((unsigned)((B * k + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ring, (long long)ring_bs,
                     R, (long long)f0, k, out, (long long)out_bs, B);
  return check_launch("vad_take");
}

extern "C" int fac_sid_apply(const fac_sid_apply_desc* d, fac_stream_t stream) {
  FAC_REQUIRE(d, "sid_apply: null descriptor");
  FAC_REQUIRE(d->mode && d->sid_codes, "sid_apply: null mode or code store");
  FAC_REQUIRE(d->B > 0 && d->B <= (1 << 20), "sid_apply: B = %d outside 1 .. 2^20", d->B);
  FAC_REQUIRE(d->k >= 1 && d->k <= FAC_PLC_MAX_FRAMES, "sid_apply: k = %d outside 1 .. %d", d->k, FAC_PLC_MAX_FRAMES);
  SidArgs a;
  int Q = 0;
  for (int r = 0; r < 3; ++r) {
    FAC_REQUIRE(d->n_q[r] >= 0, "sid_apply: negative quantizer count of RVQ %d", r);
    FAC_REQUIRE(d->n_q[r] == 0 || d->dst[r], "sid_apply: RVQ %d has %d quantizers but no codes", r, d->n_q[r]);
    FAC_REQUIRE(d->n_q[r] == 0 || ((d->B == 1 || d->dst_bs[r] > 0) && (d->n_q[r] == 1 || d->dst_qs[r] >= d->k)),
                "sid_apply: strides (%lld, %lld) of RVQ %d cannot address (B = %d, %d, k = %d)", (long long)d->dst_bs[r],
                (long long)d->dst_qs[r], r, d->B, d->n_q[r], d->k);
    Q += d->n_q[r];
    a.dst[r] = reinterpret_cast<long long*>(d->dst[r]); a.dst_bs[r] = d->dst_bs[r]; a.dst_qs[r] = d->dst_qs[r];
    a.n_q[r] = d->n_q[r];
  }
  FAC_REQUIRE(Q >= 1 && Q <= FAC_VQ_DECODE_MAX_Q, "sid_apply: %d quantizers (1 .. %d)", Q, FAC_VQ_DECODE_MAX_Q);
  a.mode = d->mode;
  a.sid_codes = reinterpret_cast<long long*>(d->sid_codes);
  a.B = d->B; a.k = d->k; a.Q = Q;
  const int n = d->B * Q;
  hipLaunchKernelGGL(sid_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("sid_apply");
}
