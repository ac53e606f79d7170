// C-ABI entry points of the MFMA conv (kernel: conv1d_mfma.h; instantiations: conv1d_tile_*.hip).
#include "conv1d_mfma.h"
#include <stdlib.h>

namespace fac {

// The forward conv kernels.  The values are the ids fac_conv1d_variant hands out through the C ABI: append, never renumber.
enum ConvKernel : int {
  CK_128x32 = 0,     // fp32 MFMA tiles (conv1d_tile_*.hip), named rows x columns
  CK_32x256 = 1,
  CK_64x128 = 2,
  CK_96x128 = 3,
  CK_128x128 = 4,
  CK_128x256 = 5,    // also the all-phases ConvTranspose1d (row_phases > 1) outside the split kernels' shapes
  CK_96x256 = 6,
  CK_FUSED_RU = 7,   // fused ResidualUnit (w_k1)
  CK_128x160 = 8,
  CK_NARROW = 9,     // VALU kernel for C_out <= 2 over many (batch, 1024-step) tiles
  CK_SKINNY = 10,    // split reduction, <= 640 columns (its single-launch sub-path for <= 4 columns included: named apart)
  CK_BSPLIT = 11,    // split-bf16 kernel, K = 3 / 5 / 7
  CK_CIN1 = 12,      // store-stream kernel for C_in = 1
  CK_THIN = 13,      // channel-split VALU kernel for C_out <= 8 over few tiles
  CK_PW = 14,        // streaming k = 1 kernel, fp32 weights resident in LDS
  CK_GSPLIT = 15,    // split-bf16 GEMM kernel, 1 / 2 taps (strided: K <= 2 * stride)
  CK_BSPLIT2 = 16,   // split-bf16 kernel for few output channels, 9 / 3 taps
  CK_PWS = 17,       // streaming k = 1 kernel on the bf16 pipe (pw_split)
  CK_PWT = 18,       // streaming kernel with taps on the bf16 pipe (pw_split, stride 2)
  CK_BSPLIT96 = 19,  // split-bf16 kernel, K = 7, 96-row tile (split_rows = 96)
};

// Tile selection: M tile by output channels, narrow-N tile for short sequences (LSTM batches).
static ConvKernel select_variant(const fac_conv_desc* d) {
  const int co = d->C_out;
  if (d->row_phases > 1) return CK_128x256;      // (channel, phase) rows: the 128 x 256 tile with the all-waves LDS epilogue
  if (d->T_out <= 32) return CK_128x32;
  if (co <= 32) return CK_32x256;
  if (co <= 64) return CK_64x128;
  // k = 1 convs re-use nothing across taps: per staged byte they do 7x less MFMA work than k = 7 and are
  // LDS-DMA-bound on 128-wide time tiles; long sequences take 256-wide tiles with 8 MFMA waves
  // (measured +15..30 % on the k = 1 layers, neutral on k = 7).
  const bool wide = d->K == 1 && d->n_phase == 1 && d->T_out >= 512;   // (wide tiles measured slower for K = 2)
  // 2 s clips are 160 latent frames: a 160-wide tile wastes nothing where 128 + 32 would waste 37 %
  if (d->T_out > 128 && d->T_out <= 160 && co > 64) {
    // ... but it is one workgroup per (clip, 128 rows), and a k = 1 conv has nothing else to spread: the style path's 1025 -> 80,
    // 80 -> 512 (+ Mish) and 20 -> 256 at 32 clips are 32 / 128 / 64 workgroups on 256 CUs, each walking all 160 columns of every
    // stage and of the epilogue alone.  Five 32-column tiles per clip instead, while the wide tiles would leave CUs empty; a
    // k = 1 tile has no halo, so nothing is staged twice but the weights.  keep_tile160 holds the wide tile (A/B, tests).
    const long long wide_tiles = (long long)d->B * ((co + 127) / 128);
    if (d->K == 1 && d->stride == 1 && d->n_phase == 1 && !d->keep_tile160 && wide_tiles < 256) return CK_128x32;
    return CK_128x160;
  }
  if (co % 128 != 0 && co % 96 == 0) return wide ? CK_96x256 : CK_96x128;
  return wide ? CK_128x256 : CK_128x128;
}

// One or two output channels, plain stride-1 conv with nothing but bias / activation in the epilogue.
// (it parallelises over (batch, 1024-step tile) only: with fewer than ~128 such tiles -- the period discriminators' 1024 -> 1
// output conv over one row-concatenated signal -- the MFMA tile is 10x faster despite wasting 31 of its 32 rows)
static bool narrow_ok(const fac_conv_desc* d) {
  return d->C_out <= 2 && d->stride == 1 && d->n_phase == 1 && d->phase_shift == 0 && d->y_tstride == 1 && !d->res && !d->y2 &&
         !d->w_batched && d->y && (long long)d->B <= 65535 && (long long)d->B * ((d->T_out + 1023) / 1024) >= 128;
}

// FAC_PW=0 sends the k = 1 / stride-2 streaming kernels' layers back to the MFMA tiles: the independent second path of
// tests/test_train_golden.py (a child process's environment), read once.
static bool pw_enabled() {
  static const bool on = !(getenv("FAC_PW") && getenv("FAC_PW")[0] == '0');
  return on;
}

// The one place that decides what a descriptor launches: validates it, fills `a` completely and names the kernel.
// fac_conv1d_fwd launches `k` with `a`; fac_conv1d_variant only reports `k`.  Touches no device.
static int conv_plan(const fac_conv_desc* d, ConvArgs& a, ConvKernel& k) {
  FAC_REQUIRE(d && (d->x || d->x_p8) && (d->w || d->w_split) && (d->y || d->y2 || d->y2_p8), "conv1d: null pointer");
  FAC_REQUIRE(!d->y2 || d->alpha_y2 || d->act == FAC_ACT_WN_RES_SKIP, "conv1d: y2 needs alpha_y2");
  FAC_REQUIRE(d->B > 0 && d->C_in > 0 && d->C_out > 0 && d->T_in > 0 && d->T_out > 0,
              "conv1d: bad shape B=%d C_in=%d C_out=%d T_in=%d T_out=%d", d->B, d->C_in, d->C_out,
              d->T_in, d->T_out);
  FAC_REQUIRE(d->K >= 1 && d->stride >= 1 && d->dilation >= 1 && d->pad_left >= 0,
              "conv1d: bad K/stride/dilation/pad");
  FAC_REQUIRE(d->C_out_pad % 32 == 0 && (d->C_out_pad >= d->C_out || d->row_phases > 1), "conv1d: C_out_pad must be a multiple of 32");
  FAC_REQUIRE(d->n_phase >= 1 && d->y_tstride >= 1, "conv1d: bad phase config");
  FAC_REQUIRE((long long)d->B * d->n_phase <= 65535, "conv1d: B*n_phase too large for grid.z");
  a.x = d->x; a.w = d->w; a.bias = d->bias; a.alpha_in = d->alpha_in; a.alpha_out = d->alpha_out;
  a.res = d->res; a.y = d->y; a.y2 = d->y2; a.alpha2 = d->alpha_y2;
  a.w1 = d->w_k1; a.bias1 = d->bias_k1;
  a.x_p8 = reinterpret_cast<const unsigned char*>(d->x_p8); a.x_p8_ps = d->x_p8_plane_bytes;
  a.y2_p8 = reinterpret_cast<unsigned char*>(d->y2_p8); a.y2_p8_ps = d->y2_p8_plane_bytes;
  FAC_REQUIRE(!d->y2_p8 || d->alpha_y2, "conv1d: y2_p8 needs alpha_y2");
  if (d->w_k1) {
    FAC_REQUIRE(d->C_in == d->C_out && d->C_out_pad == d->C_out && d->n_phase == 1 && d->stride == 1 &&
                    d->alpha_out && d->act == FAC_ACT_NONE && !d->w_batched,
                "conv1d: fused ResidualUnit needs C_in == C_out (multiple of 32), stride 1, a Snake alpha_out");
  }
  a.x_bs = d->x_bs; a.x_cs = d->x_cs; a.y_bs = d->y_bs; a.y_cs = d->y_cs; a.w_bs = d->w_bs;
  a.B = d->B; a.C_in = d->C_in; a.T_in = d->T_in; a.C_out = d->C_out; a.C_out_pad = d->C_out_pad;
  a.T_out = d->T_out; a.K = d->K; a.stride = d->stride; a.dil = d->dilation;
  a.pad_left = d->pad_left; a.pad_mode = d->pad_mode; a.n_phase = d->n_phase;
  a.y_tstride = d->y_tstride; a.act = d->act; a.w_batched = d->w_batched;
  a.phase_shift = d->phase_shift;
  a.rp = d->row_phases > 1 ? d->row_phases : 1;
  FAC_REQUIRE(!d->gate_cond || (d->act == FAC_ACT_GATE && d->gate_cond_bs >= 0),
              "conv1d: gate_cond is the conditioning row of the FAC_ACT_GATE epilogue (act=%d gate_cond_bs=%lld)", d->act,
              (long long)d->gate_cond_bs);
  a.gate_cond = d->gate_cond; a.gate_cond_bs = d->gate_cond_bs;
  if (a.rp > 1) {
    FAC_REQUIRE(d->n_phase == 1 && d->y_tstride == 1 && d->phase_shift == 0 && d->stride == 1 && a.rp <= 128 && !d->w_k1 &&
                    !d->w_batched && d->C_out_pad == fac_convtr_rows(d->C_out, a.rp) && !(d->K1 > 0 && d->K1 < d->K),
                "conv1d: row_phases needs a plain stride-1 launch on weights from fac_pack_convtr_w_rows");
  }
  a.K1 = d->K1 > 0 ? d->K1 : d->K; a.dil2 = d->dilation2;
  FAC_REQUIRE(a.K1 <= d->K && d->K % a.K1 == 0 && (a.K1 == d->K || d->dilation2 > 0), "conv1d: bad two-level taps (K=%d K1=%d)", d->K, d->K1);
  FAC_REQUIRE(!conv_two_level(a) || (!d->w_k1 && d->n_phase == 1 && d->pad_mode == FAC_PAD_ZERO && !d->w_batched),
              "conv1d: two-level taps need a plain, zero-padded conv");
  conv_set_virtual(a);
  FAC_REQUIRE(d->phase_shift >= 0 && d->phase_shift < d->n_phase + (d->n_phase == 1), "conv1d: bad phase_shift");
  // length of pad1d's temporary zero extension (only differs from T_in for inputs shorter than the pad)
  {
    long long last = (long long)(d->T_out - 1) * d->stride + (long long)conv_max_tap_offset(a) - d->pad_left;
    int pad_right = last >= d->T_in ? (int)(last - d->T_in + 1) : 0;
    int max_pad = d->pad_left > pad_right ? d->pad_left : pad_right;
    a.T_ext = d->T_in > max_pad ? d->T_in : max_pad + 1;
  }
  if (d->x_p8 || d->y2_p8) {      // P8 operands exist only in the kernels listed at fac_conv_desc.x_p8: no silent fp32 detour
    const bool gs = d->w_split && (d->K <= 2 || (d->stride > 1 && d->K <= 2 * d->stride)) && conv_gsplit_ok(a) &&
                    !conv_skinny_ok(a, d->ws, d->ws_bytes) && d->C_in % 8 == 0 && d->x_p8_plane_bytes < (1ll << 32);
    const bool ok = !d->y2_p8 && (gs || (d->w_split && !conv_two_level(a) && (d->split_rows == 96 ? conv_bsplit96_p8_ok(a) : conv_bsplit_p8_ok(a)) &&
                                       !conv_cin1_ok(a)));
    FAC_REQUIRE(ok, "conv1d: P8 operands given but the launch does not run on a kernel that takes them (K=%d stride=%d C_in=%d columns=%lld)",
                d->K, d->stride, d->C_in, (long long)d->B * d->T_out);
  }
  if (d->act == FAC_ACT_GATE || d->act == FAC_ACT_WN_RES_SKIP) {    // epilogues of the split-reduction kernel only
    FAC_REQUIRE(d->w && !d->w_k1 && !d->x_p8 && !conv_two_level(a) && conv_skinny_ok(a, d->ws, d->ws_bytes),
                "conv1d: FAC_ACT_GATE / FAC_ACT_WN_RES_SKIP exist only for few-column launches (B * T_out <= 640) with a workspace");
    k = CK_SKINNY;
    return FAC_OK;
  }
  if (d->w_k1) { k = CK_FUSED_RU; return FAC_OK; }
  a.gflat = 0;
  a.grt = 0;
  a.gs_ncb = 0;
  a.gs_cols_req = 0;
  // few-output-channel 9- / 3-tap convs (two-level taps included) with split weights of fac_pack_conv_w_split2
  if (d->w_split && (a.KV == 9 || a.KV == 3) && d->C_out <= 32 && conv_bsplit2_ok(a)) {
    a.w = reinterpret_cast<const float*>(d->w_split);
    k = CK_BSPLIT2;
    return FAC_OK;
  }
  FAC_REQUIRE(!conv_two_level(a) || d->w, "conv1d: two-level taps outside the split kernel's shapes need fp32 weights");
  const bool pw_on = pw_enabled();
  // stride-2 layers with few channels (weights resident in LDS as bf16 planes, inputs streamed): conv1d_pw_split.hip
  if (pw_on && d->pw_split && d->w && conv_pwt_ok(a)) { k = CK_PWT; return FAC_OK; }
  // 1- / 2-tap convs with split weights in the GEMM layout (fac_pack_gemm_w_split): the bf16 matrix pipe, fp32-grade
  if (d->w_split && (d->K <= 2 || (d->stride > 1 && d->K <= 2 * d->stride)) && conv_gsplit_ok(a) &&
      !conv_skinny_ok(a, d->ws, d->ws_bytes)) {
    a.w = reinterpret_cast<const float*>(d->w_split);
    k = CK_GSPLIT;
    if (d->x_p8) {
      FAC_REQUIRE(d->gsplit_p8_cols == 0 || d->gsplit_p8_cols == -1 || d->gsplit_p8_cols == 128 || d->gsplit_p8_cols == 256,
                  "conv1d: gsplit_p8_cols must be 0, -1, 128 or 256 (got %d)", d->gsplit_p8_cols);
      a.gs_cols_req = d->gsplit_p8_cols;
      a.gs_ncb = conv_gsplit_p8_ncb(a);     // > 0: the form that reads its input fragments straight from the P8 planes
    }
    return FAC_OK;
  }
  if (a.rp > 1) {
    FAC_REQUIRE(d->w != nullptr && d->w != (const float*)d->w_split, "conv1d: row_phases launch outside the split kernel's shapes needs fp32 weights");
    k = CK_128x256;
    return FAC_OK;
  }
  const bool two_level = conv_two_level(a);
  FAC_REQUIRE(d->split_rows == 0 || d->split_rows == 64 || d->split_rows == 96, "conv1d: split_rows must be 0, 64 or 96");
  // weights packed for the 96-row tile fit no other kernel: the launch runs on it or fails
  if (d->split_rows == 96) {
    FAC_REQUIRE(d->w_split && !two_level && conv_bsplit96_ok(a) && !conv_cin1_ok(a),
                "conv1d: split_rows = 96 needs a stride-1 k = 7 launch with C_out %% 96 == 0, C_in %% 8 == 0 and more than 640 columns "
                "(K=%d stride=%d C_in=%d C_out=%d columns=%lld)", d->K, d->stride, d->C_in, d->C_out, (long long)d->B * d->T_out);
    a.w = reinterpret_cast<const float*>(d->w_split);
    k = CK_BSPLIT96;
    return FAC_OK;
  }
  // K = 3 / 5 / 7 split kernel first (its shapes exclude the few-column launches the split-reduction kernel takes)
  if (d->w_split && !two_level && conv_bsplit_ok(a) && !conv_cin1_ok(a)) {
    a.w = reinterpret_cast<const float*>(d->w_split);
    k = CK_BSPLIT;
    return FAC_OK;
  }
  // every kernel below reads fp32 weights: a split-only launch (w == w_split or NULL) must not get here
  FAC_REQUIRE(d->w != nullptr && (const void*)d->w != d->w_split,
              "conv1d: shape does not qualify for a split-bf16 kernel (K=%d stride=%d C_in=%d C_out=%d columns=%lld) and no fp32 "
              "weights were given", d->K, d->stride, d->C_in, d->C_out, (long long)d->B * d->T_out);
  if (!two_level && conv_skinny_ok(a, d->ws, d->ws_bytes)) k = CK_SKINNY;
  else if (narrow_ok(d) && (!two_level || (a.KV - 1) * a.dil <= 64)) k = CK_NARROW;
  else if (conv_thin_ok(a, d->ws, d->ws_bytes)) k = CK_THIN;   // C_out <= 2 without enough tiles for narrow
  else if (conv_cin1_ok(a)) k = CK_CIN1;
  else if (pw_on && d->pw_split && conv_pw_ok(a) && conv_pws_ok(a)) k = CK_PWS;   // k = 1 tails at C <= 192 on the bf16 pipe
  else if (pw_on && conv_pw_ok(a)) k = CK_PW;
  else k = select_variant(d);
  return FAC_OK;
}

}  // namespace fac

extern "C" int fac_conv1d_fwd(const fac_conv_desc* d, fac_stream_t stream) {
  using namespace fac;
  ConvArgs a;
  ConvKernel k;
  if (const int rc = conv_plan(d, a, k)) return rc;
  hipStream_t s = (hipStream_t)stream;
  switch (k) {
    case CK_128x32: return conv_dispatch_128x32(a, s);
    case CK_32x256: return conv_dispatch_32x256(a, s);
    case CK_64x128: return conv_dispatch_64x128(a, s);
    case CK_96x128: return conv_dispatch_96x128(a, s);
    case CK_128x128: return conv_dispatch_128x128(a, s);
    case CK_128x256: return conv_dispatch_128x256(a, s);
    case CK_96x256: return conv_dispatch_96x256(a, s);
    case CK_FUSED_RU: return conv_dispatch_fused_ru(a, s);
    case CK_128x160: return conv_dispatch_128x160(a, s);
    case CK_NARROW: return conv_dispatch_narrow(a, s);
    case CK_SKINNY: return conv_dispatch_skinny(a, d->ws, d->ws_bytes, s);
    case CK_BSPLIT: return conv_dispatch_bsplit(a, s);
    case CK_CIN1: return conv_dispatch_cin1(a, s);
    case CK_THIN: return conv_dispatch_thin(a, d->ws, s);
    case CK_PW: return conv_dispatch_pw(a, s);
    case CK_GSPLIT: return a.gs_ncb ? conv_dispatch_gsplit_p8(a, s) : conv_dispatch_gsplit(a, s);
    case CK_BSPLIT2: return conv_dispatch_bsplit2(a, s);
    case CK_PWS: return conv_dispatch_pws(a, s);
    case CK_PWT: return conv_dispatch_pwt(a, s);
    case CK_BSPLIT96: return conv_dispatch_bsplit96(a, s);
  }
  return FAC_ERR_ARG;   // not reached: conv_plan sets one of the above
}

extern "C" int fac_conv1d_variant(const fac_conv_desc* d, char* name, int name_len) {
  using namespace fac;
  ConvArgs a;
  ConvKernel k;
  if (const int rc = conv_plan(d, a, k)) return rc;
  if (!name || name_len <= 0) return k;
  switch (k) {
    case CK_128x32: snprintf(name, name_len, "conv1d_mfma_kernel<1,1,4,1,K> 128x32"); break;
    case CK_32x256: snprintf(name, name_len, "conv1d_mfma_kernel<1,2,1,4,K> 32x256"); break;
    case CK_64x128: snprintf(name, name_len, "conv1d_mfma_kernel<2,1,1,4,K> 64x128"); break;
    case CK_96x128: snprintf(name, name_len, "conv1d_mfma_kernel<3,1,1,4,K> 96x128"); break;
    case CK_128x128: snprintf(name, name_len, "conv1d_mfma_kernel<2,2,2,2,K> 128x128"); break;
    case CK_128x256:
      snprintf(name, name_len, a.rp > 1 ? "conv1d_mfma_kernel<2,2,2,4,2> 128x256 (convtr, all phases per tile)" : "conv1d_mfma_kernel<2,2,2,4,K> 128x256");
      break;
    case CK_96x256: snprintf(name, name_len, "conv1d_mfma_kernel<3,1,1,8,K> 96x256"); break;
    case CK_FUSED_RU: snprintf(name, name_len, "conv1d_mfma_kernel<C/32,1,1,4,7,fused RU> Cx128"); break;
    case CK_128x160: snprintf(name, name_len, "conv1d_mfma_kernel<1,5,4,1,K> 128x160"); break;
    case CK_NARROW:
      snprintf(name, name_len, conv_two_level(a) ? "conv1d_narrow_kernel (VALU, C_out<=2, two-level taps)" : "conv1d_narrow_kernel (VALU, C_out<=2)");
      break;
    case CK_SKINNY:
      snprintf(name, name_len, conv_skinny_single_launch(a) ? "conv1d_gemv_kernel (single launch, <=4 columns)"
                                                            : "conv1d_skinny_kernel (split reduction, <=640 columns)");
      break;
    case CK_BSPLIT: snprintf(name, name_len, "conv1d_bsplit_kernel<%d> 64x256 (bf16x3 split, fp32-grade)", a.K); break;
    case CK_CIN1: snprintf(name, name_len, "conv1d_cin1_kernel (VALU, C_in=1, store stream)"); break;
    case CK_THIN: snprintf(name, name_len, "conv1d_thin_kernel (VALU, C_out<=8, split channels)"); break;
    case CK_PW: snprintf(name, name_len, "conv1d_pw_kernel (k=1 streaming, W in LDS)"); break;
    case CK_GSPLIT:
      if (a.gs_ncb) snprintf(name, name_len, "conv1d_gemm_split_kernel<%d> 64x%d (bf16x3 split GEMM, fp32-grade, P8 fragments)", a.stride > 1 ? 2 : a.K, 64 * a.gs_ncb);
      else snprintf(name, name_len, "conv1d_gemm_split_kernel<%d> 128x128 (bf16x3 split GEMM, fp32-grade)", a.stride > 1 ? 2 : a.K);
      break;
    case CK_BSPLIT2: snprintf(name, name_len, "conv1d_bsplit2_kernel<%d,%d> 32x512 (bf16x3 split, fp32-grade)", a.KV, a.stride); break;
    case CK_PWS: snprintf(name, name_len, "conv1d_pws_kernel (k=1 streaming, W planes in LDS, bf16x3 split, fp32-grade)"); break;
    case CK_PWT: snprintf(name, name_len, "conv1d_pwt_kernel<%d taps> (streaming, W planes in LDS, bf16x3 split, fp32-grade)", a.K); break;
    case CK_BSPLIT96: snprintf(name, name_len, "conv1d_bsplit_kernel<%d> 96x256 (bf16x3 split, fp32-grade)", a.K); break;
  }
  return k;
}
