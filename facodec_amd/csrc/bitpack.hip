// FA codes <-> packed bitstream payload, on the device (the layout comment of include/facodec_hip.h is normative).
//
// One clip of F frames and Q = n_p + n_c + n_r quantizers is the little-endian byte string of the integer
//   N = sum over t < F, q < Q of (code[q][t] & (2^bits - 1)) << (bits * (t * Q + q))
// i.e. frame-major, within a frame prosody rows, content rows, residual rows, every field `bits` wide, LSB first, no padding
// between fields or frames.  A device row is row_bytes = 4 * ceil(ceil(T Q bits / 8) / 4) bytes: whole 32-bit words.
//
// pack     one thread owns one 32-bit word w of one row: it gathers the fields floor(32 w / bits) .. floor((32 w + 31) / bits)
//          (33 at bits = 1, 4 or 5 at bits = 10, 2 at bits = 16), each masked to `bits` and shifted to its place, and writes the word once.
//          Store-only: no atomics, `out` is never read, every word of [0, row_bytes) of every row is written (fields of frames
//          t >= lens[b] contribute 0) and no byte outside it.  Adjacent lanes write adjacent words.
// unpack   one thread owns one code (b, q, t), consecutive lanes consecutive t of one row (coalesced int64 stores): it reads the
//          1 .. 3 bytes its field overlaps, byte by byte (no alignment of `in` or of its row stride is assumed), and writes the
//          field; frames t >= lens[b] are written as code 0 without a read.
// Bit offsets are 64-bit throughout: a recording's whole code stream is one row, and T Q bits passes 2^31 after 29 hours at
// 16 quantizers of 16 bits.
#include "common.h"
#include <limits.h>

namespace fac {

struct CodesPackArgs {
  const long long* codes[3];
  long long codes_bs[3], codes_qs[3];
  int n_q[3];
  const int* lens;
  unsigned* out;
  long long out_ws;        // row stride of out in 32-bit words
  long long row_words;
  int T, Q, bits;
};

struct CodesUnpackArgs {
  const unsigned char* in;
  long long in_bs;
  long long* codes[3];
  long long codes_bs[3], codes_qs[3];
  int n_q[3];
  const int* lens;
  int T, Q, bits;
};

__device__ __forceinline__ int codes_row_frames(const int* __restrict__ lens, int b, int T) {
  if (!lens) return T;
  const int L = lens[b];
  return L < 0 ? 0 : (L > T ? T : L);
}

__global__ __launch_bounds__(256) void codes_pack_kernel(CodesPackArgs a) {
  const int b = blockIdx.y;
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w >= a.row_words) return;
  const long long n_fields = (long long)codes_row_frames(a.lens, b, a.T) * a.Q;
  const long long bit0 = w * 32;
  long long f = bit0 / a.bits;
  const long long f_last = (bit0 + 31) / a.bits;
  long long t = f / a.Q;
  int q = (int)(f - t * a.Q);
  const unsigned mask = (1u << a.bits) - 1u;               // bits <= 16
  const int q1 = a.n_q[0], q2 = q1 + a.n_q[1];
  unsigned word = 0;
  for (; f <= f_last && f < n_fields; ++f) {
    const int r = q < q1 ? 0 : (q < q2 ? 1 : 2);
    const int qi = q - (r > 0 ? q1 : 0) - (r > 1 ? a.n_q[1] : 0);
    const unsigned v = (unsigned)a.codes[r][(long long)b * a.codes_bs[r] + (long long)qi * a.codes_qs[r] + t] & mask;
    const int sh = (int)(f * a.bits - bit0);                // in (-bits, 32)
    word |= sh >= 0 ? v << sh : v >> -sh;
    if (++q == a.Q) q = 0, ++t;
  }
  a.out[(long long)b * a.out_ws + w] = word;
}

__global__ __launch_bounds__(256) void codes_unpack_kernel(CodesUnpackArgs a) {
  const int b = blockIdx.z, q = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= a.T) return;
  const int q1 = a.n_q[0], q2 = q1 + a.n_q[1];
  const int r = q < q1 ? 0 : (q < q2 ? 1 : 2);
  const int qi = q - (r > 0 ? q1 : 0) - (r > 1 ? a.n_q[1] : 0);
  unsigned v = 0;
  if (t < codes_row_frames(a.lens, b, a.T)) {
    const long long bit = ((long long)t * a.Q + q) * a.bits;
    const unsigned char* p = a.in + (long long)b * a.in_bs + (bit >> 3);
    const int sh = (int)(bit & 7);
    const int nb = (sh + a.bits + 7) >> 3;                   // 1 .. 3 bytes, all below ceil(T Q bits / 8)
    v = p[0];
    if (nb > 1) v |= (unsigned)p[1] << 8;
    if (nb > 2) v |= (unsigned)p[2] << 16;
    v = (v >> sh) & ((1u << a.bits) - 1u);
  }
  a.codes[r][(long long)b * a.codes_bs[r] + (long long)qi * a.codes_qs[r] + t] = (long long)v;
}

static long long payload_bytes(int T, int Q, int bits) { return ((long long)T * Q * bits + 7) / 8; }

// The checks the two entries share; fills Q.  `what` names the entry in the message.
static int check_codes_shape(const char* what, const void* const* codes, const int32_t* n_q, int B, int T, int bits, int* Q_out) {
  FAC_REQUIRE(bits >= 1 && bits <= 16, "%s: bits = %d is outside 1..16", what, bits);
  FAC_REQUIRE(B >= 1 && T >= 1, "%s: bad shape (B = %d, T = %d)", what, B, T);
  FAC_REQUIRE(B <= 65535, "%s: B too large", what);
  int Q = 0;
  for (int r = 0; r < 3; ++r) {
    FAC_REQUIRE(n_q[r] >= 0 && n_q[r] <= FAC_VQ_DECODE_MAX_Q, "%s: RVQ %d has %d quantizers (0..%d)", what, r, n_q[r], FAC_VQ_DECODE_MAX_Q);
    FAC_REQUIRE(n_q[r] == 0 || codes[r], "%s: RVQ %d has %d quantizers but no codes", what, r, n_q[r]);
    Q += n_q[r];
  }
  FAC_REQUIRE(Q >= 1 && Q <= FAC_VQ_DECODE_MAX_Q, "%s: %d quantizers in all (1..%d)", what, Q, FAC_VQ_DECODE_MAX_Q);
  *Q_out = Q;
  return FAC_OK;
}

}  // namespace fac

using namespace fac;

extern "C" int64_t fac_codes_row_bytes(int T, int Q, int bits) {
  if (T < 1 || Q < 1 || bits < 1) return -1;
  return 4 * ((payload_bytes(T, Q, bits) + 3) / 4);
}

extern "C" int fac_codes_pack(const fac_codes_pack_desc* d, fac_stream_t stream) {
  FAC_REQUIRE(d, "codes_pack: null descriptor");
  int Q = 0;
  if (int rc = check_codes_shape("codes_pack", reinterpret_cast<const void* const*>(d->codes), d->n_q, d->B, d->T, d->bits, &Q)) return rc;
  FAC_REQUIRE(d->out, "codes_pack: null pointer (out)");
  const long long row_bytes = fac_codes_row_bytes(d->T, Q, d->bits);
  FAC_REQUIRE(d->out_bs % 4 == 0, "codes_pack: out_bs = %lld is not a multiple of 4", (long long)d->out_bs);
  FAC_REQUIRE(d->out_bs >= row_bytes, "codes_pack: out_bs = %lld is too small for rows of %lld bytes", (long long)d->out_bs, row_bytes);
  FAC_REQUIRE(((uintptr_t)d->out & 3) == 0, "codes_pack: out is not 4-byte aligned");
  const long long row_words = row_bytes / 4;
  FAC_REQUIRE(row_words <= (long long)INT_MAX * 128, "codes_pack: rows of %lld words do not fit the grid", row_words);
  CodesPackArgs a;
  for (int r = 0; r < 3; ++r) {
    a.codes[r] = reinterpret_cast<const long long*>(d->codes[r]);
    a.codes_bs[r] = d->codes_bs[r];
    a.codes_qs[r] = d->codes_qs[r];
    a.n_q[r] = d->n_q[r];
  }
  a.lens = d->lens;
  a.out = reinterpret_cast<unsigned*>(d->out);
  a.out_ws = d->out_bs / 4;
  a.row_words = row_words;
  a.T = d->T; a.Q = Q; a.bits = d->bits;
  hipLaunchKernelGGL(codes_pack_kernel, dim3((unsigned)((row_words + 255) / 256), d->B), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("codes_pack");
}

extern "C" int fac_codes_unpack(const fac_codes_unpack_desc* d, fac_stream_t stream) {
  FAC_REQUIRE(d, "codes_unpack: null descriptor");
  int Q = 0;
  if (int rc = check_codes_shape("codes_unpack", reinterpret_cast<const void* const*>(d->codes), d->n_q, d->B, d->T, d->bits, &Q)) return rc;
  FAC_REQUIRE(d->in, "codes_unpack: null pointer (in)");
  FAC_REQUIRE(d->in_bs >= payload_bytes(d->T, Q, d->bits), "codes_unpack: in_bs = %lld is too small for rows of %lld bytes",
              (long long)d->in_bs, payload_bytes(d->T, Q, d->bits));
  CodesUnpackArgs a;
  for (int r = 0; r < 3; ++r) {
    a.codes[r] = reinterpret_cast<long long*>(d->codes[r]);
    a.codes_bs[r] = d->codes_bs[r];
    a.codes_qs[r] = d->codes_qs[r];
    a.n_q[r] = d->n_q[r];
  }
  a.in = d->in;
  a.in_bs = d->in_bs;
  a.lens = d->lens;
  a.T = d->T; a.Q = Q; a.bits = d->bits;
  hipLaunchKernelGGL(codes_unpack_kernel, dim3((unsigned)((d->T + 255) / 256), Q, d->B), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("codes_unpack");
}
