// fp32 convolution on the bf16 matrix pipe, without giving up fp32 accuracy.
//
// Every fp32 value is EXACTLY the sum of three round-to-nearest bf16 terms (8 + 8 + 8 significand bits:
// x = hi + mid + lo), and a product of two bf16 values is exact in fp32.  So w*x = sum of 9 exact cross
// products accumulated in fp32; the three smallest (mid*lo, lo*mid, lo*lo, <= 2^-24 relative) are below the
// rounding of the fp32 accumulation itself and are dropped: SIX v_mfma_f32_32x32x16_bf16 per K = 16 step.
// Measured on MI355X (tools/microbench/bf16_split_probe.hip): the bf16 pipe sustains 2 184 TFLOP/s, the fp32
// pipe 138 TFLOP/s, so six bf16 MFMAs cost 1/2.6 of the fp32 MFMAs they replace; error against fp64 of a
// K = 4 096 dot product: 2.16e-6 (this scheme) vs 2.57e-6 (v_mfma_f32_32x32x2_f32) relative to max|ref|.
// Inputs, outputs, bias, Snake, residuals and the accumulators stay fp32; nothing is stored in bf16 in HBM
// except the (pre-split, lossless) weights.
//
// Tile: 64 output channels x 256 time steps per workgroup, 4 MFMA waves (each 64 x 64 = 2 x 2 MFMA blocks)
// + NSW staging waves.  Stage = G groups of 8 input channels x all K taps = H = G*K "half slots" (8 channels
// of one tap, ordered tap-major); one MFMA contracts K = 16 = two half slots (half-wave 0: slot 2s, half-wave
// 1: slot 2s+1), an odd H is padded with a zero slot.  G = 2, K = 7: 7 MFMA steps per 16 channels, no padding.
//   weights : pre-split in HBM as [co tile][stage][plane][half slot][64 co][8 ci] bf16 -- one contiguous slab
//             per stage, moved by LDS-DMA; an A fragment (8 ci of one co) is one ds_read_b128;
//   inputs  : fp32 (B, C, T) rows -> the staging waves split each value (5 VALU ops) and write
//             [plane][ci group][column][8 ci] -- a B fragment of any tap is one aligned ds_read_b128 at column
//             t + k*dilation (no alignment constraints on dilation, unlike the fp32 slab).  The fp32 loads of
//             stage c+2 are issued one stage before they are split (register double buffer).
// Two stages of LDS (146 KB): one workgroup per CU.  Measured alternatives that fit two workgroups per CU
// (8-channel stages with tap pairs: 80 KB; a single stage of 73 KB with the co-resident workgroup as the
// second pipeline stage) ran at 100-120 TFLOP/s-equivalent against 125-180 for this layout.
#include "conv1d_bsplit_kernel.h"

namespace fac {

// v (C_out, C_in, K) [* scale per C_out] -> split layout described above.  One thread per (tile, stage, half
// slot, co): 8 input channels -> three 16-byte pieces.  CO: output channels per co tile (64; 96 for the 96-row form).
__device__ __forceinline__ void pack_conv_split_body(const float* __restrict__ v, const float* __restrict__ scale,
                                                     bf16x8* __restrict__ out, int C_out, int C_in, int K, int G, int H, int n_st,
                                                     int CO, long long n, int vb, int vg) {
  for (long long idx = (long long)vb * 256 + threadIdx.x; idx < n; idx += (long long)vg * 256) {
    const int co = (int)(idx % CO);
    long long r = idx / CO;
    const int hs = (int)(r % H);          // half slot -> (ci group, tap)
    r /= H;
    const int s = (int)(r % n_st);
    const int ct = (int)(r / n_st);
    const int g = hs % G, k = hs / G;     // slot = tap-major, group-minor: both half slots of a step share the tap (G = 2)
    const int cog = ct * CO + co;
    const float sc = (scale != nullptr && cog < C_out) ? scale[cog] : 1.0f;
    bf16x8 h, m, l;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int ci = (s * G + g) * 8 + i;
      float w = 0.f;
      if (cog < C_out && ci < C_in && k < K) {
        w = v[((long long)cog * C_in + ci) * K + k];
        if (scale != nullptr) w = __fmul_rn(w, sc);
      }
      __bf16 a, b2, c;
      split3(w, a, b2, c);
      h[i] = a; m[i] = b2; l[i] = c;
    }
    const long long base = ((long long)ct * n_st + s) * 3;
    out[((base + 0) * H + hs) * CO + co] = h;
    out[((base + 1) * H + hs) * CO + co] = m;
    out[((base + 2) * H + hs) * CO + co] = l;
  }
}

__global__ __launch_bounds__(256) void pack_conv_split_kernel(const float* __restrict__ v, const float* __restrict__ scale,
                                                              bf16x8* __restrict__ out, int C_out, int C_in, int K, int G, int H,
                                                              int n_st, int CO, long long n) {
  pack_conv_split_body(v, scale, out, C_out, C_in, K, G, H, n_st, CO, n, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(256) void bsplit_batch_kernel(const PrepJob* __restrict__ jobs, const int* __restrict__ first, int njobs) {
  const int j = prep_find_job(first, njobs, blockIdx.x);
  const PrepJob& J = jobs[j];
  pack_conv_split_body(static_cast<const float*>(J.a), static_cast<const float*>(J.b), static_cast<bf16x8*>(J.out), J.i[0], J.i[1],
                       J.i[2], J.i[3], J.i[4], J.i[5], J.i[6], J.n, blockIdx.x - first[j], J.nblocks);
}

int prep_launch_bsplit(const PrepJob* jobs, const int* first, int njobs, int total, hipStream_t s) {
  hipLaunchKernelGGL(bsplit_batch_kernel, dim3(total), dim3(256), 0, s, jobs, first, njobs);
  return check_launch("bsplit_batch");
}

bool conv_bsplit_ok(const ConvArgs& a) {
  if (!((a.K == 7 || a.K == 5 || a.K == 3) && a.stride == 1 && a.n_phase == 1 && a.phase_shift == 0 && a.y_tstride == 1 && !a.alpha_in &&
        !a.w1 && !a.w_batched && (long long)a.B * a.T_out > 640))
    return false;
  const int G = bs_group(a.C_in), tt = G == 2 ? 256 : 512;
  const int kp = G == 2 ? a.K - 1 : ((a.K + 1) & ~1) - 1;                        // G = 1 also reads the zero tap
  return a.C_in % (8 * G) == 0 && G * ((tt + kp * a.dil + 63) / 64) <= BS_NSW * BS_XU &&
         a.x_cs * (long long)a.C_in < (1ll << 31);
}

bool conv_bsplit_p8_ok(const ConvArgs& a) {
  return conv_bsplit_ok(a) && bs_group(a.C_in) == 2 && (long long)a.T_in * 16 < (1ll << 32);
}

int conv_dispatch_bsplit(ConvArgs& a, hipStream_t s) {
  if (a.K == 5)   // the discriminators' (5,1) convs and their data gradients, the WaveNet / style-encoder k = 5 convs
    return bs_group(a.C_in) == 2 ? bsplit_launch<5, 2, 4, BS_NSW_WIDE>(a, s) : bsplit_launch<5, 1, 8, BS_NSW>(a, s);
  if (a.K == 3)   // the encoder's output conv (1024 -> 1024)
    return bs_group(a.C_in) == 2 ? bsplit_launch<3, 2, 4, BS_NSW_WIDE>(a, s) : bsplit_launch<3, 1, 8, BS_NSW>(a, s);
  return bs_group(a.C_in) == 2 ? bsplit_launch<7, 2, 4, BS_NSW_WIDE>(a, s) : bsplit_launch<7, 1, 8, BS_NSW>(a, s);
}

}  // namespace fac

// tuning aid: resident workgroups per CU the runtime computes for the split kernel at a given LDS size
extern "C" int fac_debug_bsplit_occupancy(int lds_bytes) {
  int n = -1;
  auto kern = fac::conv1d_bsplit_kernel<7, 2, 4, fac::BS_NSW_WIDE>;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fac::FAC_LDS_MAX);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, (4 + fac::BS_NSW) * 64, (size_t)lds_bytes) != hipSuccess) return -1;
  return n;
}

// rows: output channels per co tile -- 64 (stage shape by C_in, see bs_group) or 96 (k = 7 only: G = 1 stages of 8 channels with
// tap pairs, conv1d_bsplit96.hip)
static bool split_rows_ok(int K, int rows) { return rows == fac::BS_CO || (rows == fac::BS96_CO && K == 7); }

extern "C" int64_t fac_conv_w_split_rows_bytes(int C_out, int C_in, int K, int rows) {
  using namespace fac;
  if (!split_rows_ok(K, rows)) return -1;
  const int G = rows == BS96_CO ? 1 : bs_group(C_in);
  const int64_t n_ct = (C_out + rows - 1) / rows, n_st = (C_in + 8 * G - 1) / (8 * G);
  return n_ct * n_st * 3 * bs_slots(K, G) * rows * 16;
}

extern "C" int64_t fac_conv_w_split_bytes(int C_out, int C_in, int K) { return fac_conv_w_split_rows_bytes(C_out, C_in, K, fac::BS_CO); }

extern "C" int fac_pack_conv_w_split_rows(const float* v, const float* scale, void* out, int C_out, int C_in, int K, int rows,
                                          fac_stream_t stream) {
  using namespace fac;
  FAC_REQUIRE(v && out && C_out > 0 && C_in > 0 && K > 0, "pack_conv_w_split: bad arguments");
  FAC_REQUIRE(split_rows_ok(K, rows), "pack_conv_w_split: no %d-row tile for K=%d", rows, K);
  const int G = rows == BS96_CO ? 1 : bs_group(C_in);
  const int n_ct = (C_out + rows - 1) / rows, n_st = (C_in + 8 * G - 1) / (8 * G), H = bs_slots(K, G);
  const long long n = (long long)n_ct * n_st * H * rows;
  const int blocks = (int)((n + 255) / 256 < 65535 ? (n + 255) / 256 : 65535);
  if (prep_recording()) {
    PrepJob j{}; j.a = v; j.b = scale; j.out = out; j.kind = PK_CONV_SPLIT; j.nblocks = blocks; j.n = n;
    j.i[0] = C_out; j.i[1] = C_in; j.i[2] = K; j.i[3] = G; j.i[4] = H; j.i[5] = n_st; j.i[6] = rows;
    return prep_record(PU_BSPLIT, j);
  }
  hipLaunchKernelGGL(pack_conv_split_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, v, scale,
                     reinterpret_cast<bf16x8*>(out), C_out, C_in, K, G, H, n_st, rows, n);
  return check_launch("pack_conv_w_split");
}

extern "C" int fac_pack_conv_w_split(const float* v, const float* scale, void* out, int C_out, int C_in, int K,
                                     fac_stream_t stream) {
  return fac_pack_conv_w_split_rows(v, scale, out, C_out, C_in, K, fac::BS_CO, stream);
}
