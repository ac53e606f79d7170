// Codes -> quantized latents -> timbre-normed decoder input, in one launch.
// Reference: VectorQuantize.decode_code / ResidualVectorQuantize.from_codes (dac/nn/quantize.py:72-76, 200-220) for the
// prosody, content and residual RVQs, then the tail of FAquantizer.forward_v2 (modules/quantize.py:436-449, eval:
// res_mask = 1):
//   z_q_i = out_proj(codebook_i[code_i])       out_proj weight = v * (g / ||v||)  (weight norm, 1x1 conv 8 -> D)
//   z_p / z_c / z_r = 0 + z_q_0 + z_q_1 + ...   in quantizer order
//   outs = LayerNorm_C((z_p + z_c) + z_r) * gamma + beta,   [gamma | beta] = style = timbre_linear(timbre)
//
// Per value the arithmetic is vq_fwd_kernel's out-projection (vq.hip: fmul_rn(v, scale), an fma chain over the eight
// code dimensions, + bias) applied to the raw codebook row, the sums are the zq_acc / fac_add chain of the forward, and
// the norm is layernorm_c_kernel's (misc.hip: four sequential channel chains per frame, the same combine and roundings).
// A decode therefore differs from the forward's `outs` only by the forward's straight-through term z_e + (z_q - z_e).
//
// Layout: one workgroup per (clip, tile of TT <= 16 frames).  The decode is write-bound (B x D x T floats out, ~0.4 MB of
// codebooks and weights in), so the D x TT column block of the tile lives in LDS (64 KB at D = 1024) between the
// projection and the norm:
//   gather    the tile's codebook rows (n_q x TT x 8 floats) into LDS; indices are clamped to [0, Kc) for the load
//             (range checking is the caller's job; the clamp only keeps the kernel inside the codebook);
//   project   lane = channel: its weight rows (4 quantizers' rows per load batch) are loaded once and stay in registers
//             while it walks the TT frames; the codebook rows are wave-uniform LDS broadcasts; the pre-norm sum goes to
//             the LDS block (row stride TT + 1: conflict-free for lanes on consecutive channels);
//   norm      4 x TT threads run the four channel chains of layernorm_c_kernel per frame out of LDS;
//   store     lane = frame: every row segment of the tile is written with consecutive lanes on consecutive frames.
// The optional per-RVQ sums z_p / z_c / z_r (from_codes) are stored straight from the projection (lane = channel, TT
// consecutive frames per lane); they are off the decode path.
//
// fac_vq_decode_masked is the same kernel body with MASKED = true: quantizer counts per (row, frame).  The tile's
// counts (3 x TT int32, clamped to [0, n_q[r]]) are read once into LDS; in the projection a quantizer's term of frame t is
// computed and added only when its index within its RVQ is below the frame's count -- the predicate is wave-uniform (it does not
// depend on the channel), and a skipped term's __fadd_rn is not executed, so a frame's chain is exactly the chain of the unmasked
// kernel launched with that frame's counts.  Gather, finish order, norm and store are untouched.
#include <type_traits>

#include "common.h"

namespace fac {

constexpr int VD_TT = 16;                     // frames per workgroup (smaller power of two for T < 16)
constexpr int VD_CD = 8;                      // codebook_dim
constexpr int VD_MAXQ = FAC_VQ_DECODE_MAX_Q;
constexpr int VD_QB = 4;                      // quantizers whose weights are loaded together

struct VqDecArgs {
  const long long* codes[3];
  long long codes_bs[3], codes_qs[3];
  int n_q[3];
  const float* codebook[VD_MAXQ];
  const float* w_out[VD_MAXQ];
  const float* w_out_scale[VD_MAXQ];
  const float* b_out[VD_MAXQ];
  const float* style;
  float* outs;
  float* z[3];
  int B, D, T, Kc, tt_log2;
};

struct VqDecMaskedArgs : VqDecArgs {
  const int* n_use;                           // [b * n_use_bs + t * n_use_ts + r]
  long long n_use_bs, n_use_ts;
};

template <bool MASKED>
__global__ __launch_bounds__(256) void vq_decode_kernel(std::conditional_t<MASKED, VqDecMaskedArgs, VqDecArgs> a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int TT = 1 << a.tt_log2;
  const int XS = TT + 1;                                 // LDS row stride of the column block
  const int nqt = a.n_q[0] + a.n_q[1] + a.n_q[2];
  float* xs = sm;                                        // [D][TT + 1]  (z_p + z_c) + z_r
  float* rows = xs + (((long long)a.D * XS + 3) & ~3ll); // [nqt][16][8] codebook rows, 16-byte aligned
  float* red = rows + nqt * VD_TT * VD_CD;               // [2][4][16]
  float* stat = red + 2 * 4 * VD_TT;                     // [2][16]  mean, rstd
  int* nu = reinterpret_cast<int*>(stat + 2 * VD_TT);    // [3][16]  MASKED only: the tile's quantizer counts

  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * TT;
  const long long bofs = (long long)b * a.D * a.T;

  if constexpr (MASKED) {
    if (tid < 3 * TT) {
      const int r = tid >> a.tt_log2, l = tid & (TT - 1);
      const int t = min(t0 + l, a.T - 1);
      const int n = a.n_use[(long long)b * a.n_use_bs + (long long)t * a.n_use_ts + r];
      nu[r * VD_TT + l] = n < 0 ? 0 : (n > a.n_q[r] ? a.n_q[r] : n);
    }
  }

  // ---- gather the tile's codebook rows
  for (int i = tid; i < nqt * TT; i += 256) {
    const int q = i >> a.tt_log2, l = i & (TT - 1);
    const int r = q < a.n_q[0] ? 0 : (q < a.n_q[0] + a.n_q[1] ? 1 : 2);
    const int qi = q - (r > 0 ? a.n_q[0] : 0) - (r > 1 ? a.n_q[1] : 0);
    const int t = min(t0 + l, a.T - 1);
    long long k = a.codes[r][(long long)b * a.codes_bs[r] + (long long)qi * a.codes_qs[r] + t];
    k = k < 0 ? 0 : (k >= a.Kc ? a.Kc - 1 : k);
    const float* cr = a.codebook[q] + k * VD_CD;
    float* dst = rows + (q * VD_TT + l) * VD_CD;
    *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(cr);
    *reinterpret_cast<float4*>(dst + 4) = *reinterpret_cast<const float4*>(cr + 4);
  }
  __syncthreads();

  // ---- project: lane = channel
  int q_end[3];
  q_end[0] = a.n_q[0];
  q_end[1] = q_end[0] + a.n_q[1];
  q_end[2] = q_end[1] + a.n_q[2];
  const int nt_valid = min(TT, a.T - t0);
  for (int c = tid; c < a.D; c += 256) {
    float zs[VD_TT], ov[VD_TT];
#pragma unroll
    for (int t = 0; t < VD_TT; ++t) zs[t] = 0.f, ov[t] = 0.f;
    int r = 0;
    // closes RVQ r: optional store of its sum, then ov = z_p / ov + z_c / ov + z_r (the forward's fac_add order)
    auto finish = [&](int rr) {
      float* zo = a.z[rr];
      if (zo) {
        float* zrow = zo + bofs + (long long)c * a.T + t0;
#pragma unroll
        for (int t = 0; t < VD_TT; ++t)
          if (t < nt_valid) zrow[t] = zs[t];
      }
#pragma unroll
      for (int t = 0; t < VD_TT; ++t) {
        ov[t] = rr == 0 ? zs[t] : __fadd_rn(ov[t], zs[t]);
        zs[t] = 0.f;
      }
    };
    while (r < 3 && q_end[r] == 0) finish(r++);
    for (int q0 = 0; q0 < nqt; q0 += VD_QB) {
      float w[VD_QB][VD_CD], bo[VD_QB];
#pragma unroll
      for (int u = 0; u < VD_QB; ++u) {          // all loads of the batch first, then the math
        const int q = min(q0 + u, nqt - 1);
        const float* wr = a.w_out[q] + (long long)c * VD_CD;
        const float4 lo = *reinterpret_cast<const float4*>(wr);
        const float4 hi = *reinterpret_cast<const float4*>(wr + 4);
        const float sc = a.w_out_scale[q] ? a.w_out_scale[q][c] : 1.0f;
        bo[u] = a.b_out[q][c];
        w[u][0] = __fmul_rn(lo.x, sc); w[u][1] = __fmul_rn(lo.y, sc); w[u][2] = __fmul_rn(lo.z, sc); w[u][3] = __fmul_rn(lo.w, sc);
        w[u][4] = __fmul_rn(hi.x, sc); w[u][5] = __fmul_rn(hi.y, sc); w[u][6] = __fmul_rn(hi.z, sc); w[u][7] = __fmul_rn(hi.w, sc);
      }
#pragma unroll
      for (int u = 0; u < VD_QB; ++u) {
        const int q = q0 + u;
        if (q >= nqt) break;
        const float* rq = rows + q * VD_TT * VD_CD;
        const int qi = q - (r > 0 ? q_end[r - 1] : 0);   // MASKED: index within RVQ r (r is q's RVQ here)
#pragma unroll
        for (int t = 0; t < VD_TT; ++t) {
          if (t < TT && (!MASKED || qi < nu[r * VD_TT + t])) {
            const float4 lo = *reinterpret_cast<const float4*>(rq + t * VD_CD);
            const float4 hi = *reinterpret_cast<const float4*>(rq + t * VD_CD + 4);
            float o = __fmul_rn(w[u][0], lo.x);
            o = fmaf(w[u][1], lo.y, o);
            o = fmaf(w[u][2], lo.z, o);
            o = fmaf(w[u][3], lo.w, o);
            o = fmaf(w[u][4], hi.x, o);
            o = fmaf(w[u][5], hi.y, o);
            o = fmaf(w[u][6], hi.z, o);
            o = fmaf(w[u][7], hi.w, o);
            o = __fadd_rn(o, bo[u]);
            zs[t] = __fadd_rn(zs[t], o);
          }
        }
        if (q == q_end[r] - 1) {
          finish(r++);
          while (r < 3 && q_end[r] == q + 1) finish(r++);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < VD_TT; ++t)
      if (t < TT) xs[c * XS + t] = ov[t];
  }
  __syncthreads();

  // ---- LayerNorm over channels: chain k sums channels k, k + 4, ... of frame l (layernorm_c_kernel's order)
  const int C = a.D;
  const bool chain = tid < 4 * TT;
  const int k = tid >> a.tt_log2, l = tid & (TT - 1);
  float mean = 0.f;
  if (chain) {
    float s = 0.f;
    for (int c = k; c < C; c += 4) s += xs[c * XS + l];
    red[k * VD_TT + l] = s;
  }
  __syncthreads();
  if (chain) {
    mean = ((red[0 * VD_TT + l] + red[1 * VD_TT + l]) + (red[2 * VD_TT + l] + red[3 * VD_TT + l])) / (float)C;
    float vs = 0.f;
    for (int c = k; c < C; c += 4) {
      const float d = xs[c * XS + l] - mean;
      vs = fmaf(d, d, vs);
    }
    red[(4 + k) * VD_TT + l] = vs;
  }
  __syncthreads();
  if (chain && k == 0) {
    const float var = ((red[4 * VD_TT + l] + red[5 * VD_TT + l]) + (red[6 * VD_TT + l] + red[7 * VD_TT + l])) / (float)C;
    stat[l] = mean;
    stat[VD_TT + l] = __fdiv_rn(1.0f, sqrtf(var + 1e-5f));
  }
  __syncthreads();

  // ---- normalise, * gamma + beta, store: lane = frame
  const int G = 256 >> a.tt_log2;
  const int g = tid >> a.tt_log2;
  if (l < nt_valid) {
    const float mu = stat[l], rs = stat[VD_TT + l];
    const float* gm = a.style + (long long)b * 2 * C;
    float* ob = a.outs + bofs + t0 + l;
    for (int c = g; c < C; c += G) {
      const float nv = __fmul_rn(xs[c * XS + l] - mu, rs);
      ob[(long long)c * a.T] = __fadd_rn(__fmul_rn(nv, gm[c]), gm[C + c]);
    }
  }
}

}  // namespace fac

namespace fac {

static int vq_decode_launch(const fac_vq_decode_desc* d, const int32_t* n_use, int64_t n_use_bs, int64_t n_use_ts,
                            fac_stream_t stream) {
  FAC_REQUIRE(d && d->style && d->outs, "vq_decode: null pointer");
  FAC_REQUIRE(d->B > 0 && d->D > 0 && d->T > 0 && d->Kc > 0, "vq_decode: bad shape");
  FAC_REQUIRE(d->B <= 65535, "vq_decode: B too large");
  int nqt = 0;
  for (int r = 0; r < 3; ++r) {
    FAC_REQUIRE(d->n_q[r] >= 0, "vq_decode: negative quantizer count");
    FAC_REQUIRE(d->n_q[r] == 0 || d->codes[r], "vq_decode: RVQ %d has %d quantizers but no codes", r, d->n_q[r]);
    nqt += d->n_q[r];
  }
  FAC_REQUIRE(nqt <= FAC_VQ_DECODE_MAX_Q, "vq_decode: %d quantizers (at most %d)", nqt, FAC_VQ_DECODE_MAX_Q);
  for (int q = 0; q < nqt; ++q)
    FAC_REQUIRE(d->codebook[q] && d->w_out[q] && d->b_out[q], "vq_decode: null weight of quantizer %d", q);
  if (n_use)
    FAC_REQUIRE((d->B == 1 || n_use_bs > 0) && (d->T == 1 || n_use_ts > 0),
                "vq_decode_masked: n_use strides (%lld, %lld) cannot address (B = %d, T = %d, 3)", (long long)n_use_bs,
                (long long)n_use_ts, d->B, d->T);
  int tt_log2 = 0;
  while ((1 << tt_log2) < VD_TT && (1 << tt_log2) < d->T) ++tt_log2;
  const int TT = 1 << tt_log2;
  const size_t lds = ((((size_t)d->D * (TT + 1) + 3) & ~(size_t)3) + (size_t)nqt * VD_TT * VD_CD + 2 * 4 * VD_TT + 2 * VD_TT +
                      (n_use ? 3 * VD_TT : 0)) * 4;
  FAC_REQUIRE(lds <= FAC_LDS_MAX, "vq_decode: %d channels x %d frames do not fit LDS", d->D, TT);
  VqDecMaskedArgs a;
  for (int r = 0; r < 3; ++r) {
    a.codes[r] = reinterpret_cast<const long long*>(d->codes[r]);
    a.codes_bs[r] = d->codes_bs[r];
    a.codes_qs[r] = d->codes_qs[r];
    a.n_q[r] = d->n_q[r];
    a.z[r] = d->z[r];
  }
  for (int q = 0; q < VD_MAXQ; ++q) {
    const bool used = q < nqt;
    a.codebook[q] = used ? d->codebook[q] : nullptr;
    a.w_out[q] = used ? d->w_out[q] : nullptr;
    a.w_out_scale[q] = used ? d->w_out_scale[q] : nullptr;
    a.b_out[q] = used ? d->b_out[q] : nullptr;
  }
  a.style = d->style;
  a.outs = d->outs;
  a.B = d->B; a.D = d->D; a.T = d->T; a.Kc = d->Kc; a.tt_log2 = tt_log2;
  a.n_use = n_use;
  a.n_use_bs = n_use_bs;
  a.n_use_ts = n_use_ts;
  const int n_tiles = (d->T + TT - 1) / TT;
  if (n_use) {
    allow_dynamic_lds<vq_decode_kernel<true>>();
    hipLaunchKernelGGL(vq_decode_kernel<true>, dim3(n_tiles, d->B), dim3(256), lds, (hipStream_t)stream, a);
    return check_launch("vq_decode_masked");
  }
  allow_dynamic_lds<vq_decode_kernel<false>>();
  hipLaunchKernelGGL(vq_decode_kernel<false>, dim3(n_tiles, d->B), dim3(256), lds, (hipStream_t)stream,
                     static_cast<const VqDecArgs&>(a));
  return check_launch("vq_decode");
}

}  // namespace fac

extern "C" int fac_vq_decode(const fac_vq_decode_desc* d, fac_stream_t stream) {
  return fac::vq_decode_launch(d, nullptr, 0, 0, stream);
}

extern "C" int fac_vq_decode_masked(const fac_vq_decode_masked_desc* d, fac_stream_t stream) {
  FAC_REQUIRE(d, "vq_decode_masked: null descriptor");
  return fac::vq_decode_launch(&d->base, d->n_use, d->n_use_bs, d->n_use_ts, stream);
}
