/*
 * facodec_hip.h -- C ABI of libfacodec_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the FAcodec encode -> factorized-VQ -> decode (+ multi-scale
 * spectral loss) hot path.  The reference (Plachtaa/FAcodec) is pure Python/PyTorch and has
 * no FFI; what it binds to underneath its nn.Modules are ATen ops.  Each entry point below
 * names the reference op (file:line under /root/reference) it replaces.  The Python host
 * (facodec_amd/) keeps the reference's module surface (build_model / encoder / quantizer /
 * decoder, modules/commons.py:283-348) and calls these through ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer borrowed from the caller (torch tensor storage);
 *     dense row-major fp32 unless noted; codes are int64.
 *   - every call is asynchronous on the hipStream_t passed as `stream` (void*); the library
 *     never allocates, frees or synchronises device memory.
 *   - return 0 on success, negative on error; fac_last_error() gives a thread-local message.
 *   - activations use the reference layout (B, C, T), T contiguous.
 */
#ifndef FACODEC_HIP_H
#define FACODEC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* fac_stream_t; /* hipStream_t */

#define FAC_OK 0
#define FAC_ERR_ARG (-1)
#define FAC_ERR_LAUNCH (-2)

#define FAC_PAD_ZERO 0
#define FAC_PAD_REFLECT 1

#define FAC_ACT_NONE 0
#define FAC_ACT_TANH 1  /* nn.Tanh, dac/model/dac.py:159 */
#define FAC_ACT_MISH 2  /* x*tanh(softplus(x)), modules/style_encoder.py:6-10 */
#define FAC_ACT_LOG_MEL 3 /* (log(1e-5+x)+4)/4, modules/quantize.py:241 */
/* The two epilogues of a WaveNet layer (modules/wavenet.py:138-166), taken only by the few-column split-reduction launches of
 * the streaming hop (B * T_out <= 640; fac_conv1d_fwd fails for any other shape -- there the elementwise kernels
 * fac_gate_tanh_sigmoid / fac_wn_res_skip do the same arithmetic):
 *   FAC_ACT_GATE        : y (B, C_out / 2, T) = tanh(c[:, :C_out/2]) * sigmoid(c[:, C_out/2:]) of c = conv + bias
 *                         (fused_add_tanh_sigmoid_multiply, modules/commons.py:113-120; its conditioning input is
 *                         fac_conv_desc.gate_cond); C_out % 256 == 0.
 *   FAC_ACT_WN_RES_SKIP : c = conv + bias; y (B, C_out / 2, T) = res + c[:, :C_out/2] (res may be y itself) and
 *                         y2 (B, C_out / 2, T) += c[:, C_out/2:] (no alpha_y2; y2 is the running skip sum). */
#define FAC_ACT_GATE 4
#define FAC_ACT_WN_RES_SKIP 5

/* ABI version; bumped whenever a signature changes. */
int fac_version(void);
/* Thread-local description of the last failure (never NULL). */
const char* fac_last_error(void);

/* ------------------------------------------------------------------------------------------
 * K6  weight-norm materialisation + packing to the GEMM-friendly layout the conv kernels read.
 * Replaces torch.nn.utils.weight_norm's  w = v * (g / ||v||)  recomputed every forward
 * (dac/model/encodec.py:42-51, dac/nn/layers.py:9-14).
 * ---------------------------------------------------------------------------------------- */

/* scale[i] = g[i] / ||v[i,:]||_2  for i < n_slices (slice = all dims but 0, contiguous,
 * slice_len floats).  g == NULL -> scale[i] = 1 (plain, un-normed weight). */
int fac_wn_scale(const float* v, const float* g, float* scale, int n_slices, int slice_len,
                 fac_stream_t stream);

/* Conv1d / Linear weight v (C_out, C_in, K) -> packed (C_in_pad, K, C_out_pad), co fastest,
 * packed[ci][k][co] = v[co][ci][k] * scale[co]; columns C_out..C_out_pad-1 and rows
 * C_in..C_in_pad-1 are zero: this call writes the WHOLE (C_in_pad, K, C_out_pad) buffer, padding included (an
 * uninitialised allocation is fine).  C_out_pad = fac_pad32(C_out), C_in_pad = fac_cin_pad(C_in). scale may be NULL (== 1). */
int fac_pack_conv_w(const float* v, const float* scale, float* packed, int C_out, int C_in,
                    int K, int C_out_pad, fac_stream_t stream);

/* ConvTranspose1d weight v (C_in, C_out, K = 2*stride) with weight-norm over dim 0 (= C_in,
 * dac/model/encodec.py:163) -> `stride` polyphase 2-tap sub-filters:
 * packed[p][ci][j][co] = v[ci][co][p + stride*(1-j)] * scale[ci],  p < stride, j in {0,1},
 * ci < C_in_pad (rows >= C_in written as zeros, as above).
 * Output phase p of the transposed conv is then a causal 2-tap conv (see fac_conv1d_fwd). */
int fac_pack_convtr_w(const float* v, const float* scale, float* packed, int C_in, int C_out,
                      int stride, int C_out_pad, fac_stream_t stream);

/* The same sub-filters for the all-phases-per-workgroup launch (fac_conv_desc.row_phases = stride): rows r = (co, p), phase
 * fastest, in tiles of 128 rows holding cpt = 128 / stride channels each (rows cpt * stride .. 127 of a tile are zero):
 * packed[ci][j][tile * 128 + (co % cpt) * stride + p] = v[ci][co][p + stride * (1 - j)] * scale[ci], tile = co / cpt;
 * the buffer is (fac_cin_pad(C_in), 2, fac_convtr_rows(C_out, stride)) floats, written completely. */
static inline int fac_convtr_rows(int C_out, int stride) {
  const int cpt = 128 / stride;
  return ((C_out + cpt - 1) / cpt) * 128;
}
int fac_pack_convtr_w_rows(const float* v, const float* scale, float* packed, int C_in, int C_out, int stride,
                           fac_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K1-K4  Conv1d / polyphase ConvTranspose1d as implicit GEMM on fp32 MFMA
 * (v_mfma_f32_32x32x2_f32), with fused Snake prologue, bias, Snake/tanh epilogue and
 * residual add.  Replaces SConv1d.forward (dac/model/encodec.py:212-228: pad1d + F.conv1d),
 * SConvTranspose1d.forward (:248-270), snake (dac/nn/layers.py:18-24), ResidualUnit's skip
 * add (dac/model/dac.py:38-42) and nn.Conv1d / nn.Linear calls of the quantizer.
 *
 *   y[b, co, (t*y_tstride + y_toff)] = act( snake_out( bias[co] +
 *        sum_{ci,k} w[phase][ci][k][co] * snake_in( xpad[b, ci, t*stride + k*dilation - pad_left] ) ) )
 *        + res[b, co, ...]
 *
 * xpad is x extended by reflection (FAC_PAD_REFLECT: index -j -> j on the left, T-1+j -> T-1-j
 * on the right, zero where the mirror falls outside x as pad1d :104-111 does) or zeros.
 * ---------------------------------------------------------------------------------------- */
#define FAC_CONV_WS_BYTES (32ll << 20)

typedef struct fac_conv_desc {
  const float* x;         /* (B, C_in, T_in); element (b,c,t) at x[b*x_bs + c*x_cs + t] */
  const float* w;         /* packed weights, see fac_pack_conv_w / fac_pack_convtr_w */
  const float* bias;      /* (C_out) or NULL */
  const float* alpha_in;  /* (C_in) Snake alpha applied to x on load, or NULL */
  const float* alpha_out; /* (C_out) Snake alpha applied after bias, or NULL */
  const float* res;       /* residual, same indexing as y, or NULL */
  float* y;               /* element (b,c,u) at y[b*y_bs + c*y_cs + u]; may be NULL when y2 is given */
  float* y2;              /* optional second output, same indexing: y2 = snake(y, alpha_y2) -- the
                             pre-activated copy the next Snake->conv consumes, so that consumer can
                             stage its input by pure LDS-DMA (no VALU work beside the MFMAs) */
  const float* alpha_y2;  /* (C_out) Snake alpha of y2; required iff y2 != NULL */
  const float* w_k1;      /* optional fused ResidualUnit tail (dac/model/dac.py:33-34): packed 1x1 weights
                             (fac_pack_conv_w of (C, C, 1)); then y = w_k1 * snake(conv + bias, alpha_out)
                             + bias_k1 + res.  Needs C_in == C_out in {64, 96, 128}, K = 7, stride 1. */
  const float* bias_k1;   /* (C_out) bias of the 1x1 conv, or NULL */
  int64_t x_bs, x_cs;
  int64_t y_bs, y_cs;
  int32_t B, C_in, T_in, C_out, C_out_pad;
  int32_t T_out;          /* number of t positions computed per phase */
  int32_t K, stride, dilation, pad_left, pad_mode;
  int32_t n_phase;        /* 1 for Conv1d; = upsampling stride for polyphase ConvTranspose1d */
  int32_t y_tstride;      /* 1 for Conv1d; = n_phase for ConvTranspose1d (y_toff = phase) */
  int32_t phase_shift;    /* non-causal ConvTranspose1d trims `phase_shift` samples on the LEFT
                             (dac/model/encodec.py:265-269): phase p then lands at offset p - shift, and
                             phases with p < shift read x[t], x[t+1] instead of x[t-1], x[t]; 0 = causal */
  int32_t act;            /* FAC_ACT_* applied last (before residual) */
  int32_t w_batched;      /* 0: shared weights; 1: per-b weights at w + b*w_bs (attention-style) */
  int64_t w_bs;
  /* Optional scratch for launches with few output columns (B*T_out <= 128: streaming hops, per-clip
   * Linears): lets the library split the C_in*K reduction across workgroups (conv1d_skinny.hip).  At least
   * FAC_CONV_WS_BYTES, owned by ONE stream at a time (partial sums live there between the two kernels of a
   * launch).  NULL: the tiled kernel is used for every shape. */
  void* ws;
  int64_t ws_bytes;
  /* Optional: the same weights in the split-bf16 layout of fac_pack_conv_w_split (K = 5 / 7) or fac_pack_gemm_w_split
   * (K = 1 / 2).  When given and the shape qualifies (stride 1, no Snake prologue, C_in % 16 == 0 resp. % 32 == 0, enough
   * columns), the conv runs on the bf16 matrix pipe with fp32-grade operand splitting (conv1d_bsplit.hip /
   * conv1d_gemm_split.hip); `w` is still required for every other shape. */
  const void* w_split;
  /* Optional two-level taps (0 = plain): tap k = k2 * K1 + k1 reads the input at offset k2 * dilation2 + k1 * dilation
   * (K % K1 == 0).  A (3, k) Conv2d over a row-concatenated (time, frequency) signal -- the multi-resolution
   * discriminator, dac/model/discriminator.py:101-170 -- is such a conv along the concatenated axis: K1 = k taps along
   * frequency, dilation2 = the row pitch.  Runs on the generic fp32-MFMA tile. */
  int32_t K1, dilation2;
  /* Optional (0 / 1 = off): causal ConvTranspose1d with ALL `row_phases` = stride output phases computed by one workgroup.
   * The GEMM's output rows are (channel, phase) pairs, phase fastest, 128 / row_phases channels per 128-row tile
   * (weights from fac_pack_convtr_w_rows, C_out_pad = its padded row count, n_phase = 1, K = 2, pad_left = 1, y_tstride = 1,
   * T_out = input length); the epilogue interleaves the phases through LDS and stores CONTIGUOUS runs of y (B, C_out,
   * T_out * row_phases).  (The polyphase launch, n_phase = stride, lets every phase store with stride `stride`: partial
   * cache lines, measured 2.9x the algorithmic HBM traffic.) */
  int32_t row_phases;
  /* Optional "P8" operands: an activation tensor as three bf16 planes hi / mid / lo with hi + mid + lo == value exactly
   * (round-to-nearest splits), each plane laid out [b][c / 8][t][8 channels] (16 bytes per (8-channel group, time step); C a
   * multiple of 8; planes `*_plane_bytes` apart; every plane is CLOSED BY ONE ZERO UNIT of 16 bytes at offset B * C/8 * T * 16,
   * which consumers read for columns outside the signal, so a plane takes (B * C/8 * T + 1) * 16 bytes).  That is the operand format of the split-bf16 kernels' LDS stages, so a
   * consumer copies it (16 B per lane, no arithmetic beside the matrix instructions) instead of loading fp32 and splitting it:
   * in-kernel splitting costs every split kernel 15 - 50 % of its matrix-pipe time, because vector ALU instructions of the
   * staging waves and the MFMAs of the same SIMD do not overlap.
   *   x_p8  : the INPUT in P8 (then `x` may be NULL); taken by the K = 3 / 5 / 7 split kernel (C_in % 16 == 0) and by the 1- / 2-tap
   *           split GEMM kernel (plain, strided and all-phases transposed launches; C_in % 8 == 0), where both operands then move by
   *           LDS-DMA -- or, on the shapes where that measured faster, the input fragments go straight from the planes into registers
   *           (see gsplit_p8_cols below; the same bits).
   *   y2_p8 : reserved -- the pre-activated second output snake(y, alpha_y2) in P8 instead of (or beside) fp32 `y2`.  No kernel
   *           writes it: fac_conv1d_fwd / fac_conv1d_variant refuse every descriptor that sets it (FAC_ERR_ARG, "P8 operands given
   *           but the launch does not run on a kernel that takes them"; without alpha_y2, "y2_p8 needs alpha_y2").  Leave it NULL. */
  const void* x_p8;
  int64_t x_p8_plane_bytes;
  void* y2_p8;
  int64_t y2_p8_plane_bytes;
  /* Optional (0 = off): launches the streaming kernels take (weights resident in LDS, inputs straight from global memory) may
   * split BOTH operands into three bf16 planes inside the kernel (weights once per workgroup, inputs per load) and run on the
   * bf16 matrix pipe with fp32-grade results instead of fp32 MFMAs: k = 1 with C_in == C_out in {64, 96, 128, 192, 256, 384} and
   * many columns; with fp32 weights `w` of fac_pack_convtr_w_rows also the all-phases ConvTranspose1d with stride 2 (row_phases
   * = 2), and with `w` of fac_pack_conv_w the k = 4 stride-2 conv, each with C_in * taps <= 384 (conv1d_pw_split.hip).  Needs only
   * `w`; ignored elsewhere.  The host side sets it wherever it hands `w_split` to the other layers. */
  int32_t pw_split;
  /* Optional (0 = 64): output rows per tile the split weights `w_split` of a K = 7 stride-1 launch were packed for
   * (fac_pack_conv_w_split_rows).  96 selects the 96-row form of the split kernel (conv1d_bsplit96.hip: C_out % 96 == 0, C_in % 8 ==
   * 0); such weights fit no other kernel, so a launch outside its shapes is an error. */
  int32_t split_rows;
  /* Optional, FAC_ACT_GATE only (any other act with it is an error): per-clip conditioning rows of the gate, clip b's 2 * (C_out / 2)
   * values at gate_cond + b * gate_cond_bs (a row slice of a wider (B, n) tensor is fine), added to the pre-activations after the
   * bias: y = tanh((c + g)[:C_out/2]) * sigmoid((c + g)[C_out/2:]), the same fp32 sums in the same order as fac_conv1d_fwd
   * followed by fac_gate_tanh_sigmoid with g (WN with gin_channels, modules/wavenet.py:146-155).  NULL: no conditioning. */
  const float* gate_cond;
  int64_t gate_cond_bs;
  /* Optional (0 = off): keep the 128 x 160 fp32 tile for a k = 1 launch of 129 .. 160 columns per clip that would otherwise run on
   * five 128 x 32 tiles per clip because B * ceil(C_out / 128) wide tiles are fewer than 256 workgroups.  For A/B runs and for the
   * test that holds the two forms against each other; ignored by every other launch. */
  int32_t keep_tile160;
  /* Optional (0 = the library's choice): the form of the split GEMM kernel for a launch with a P8 input.  -1 keeps the 128 x 128
   * form (conv1d_gemm_split.hip) for a shape that would otherwise run on the form that reads its input fragments straight from the
   * P8 planes (64-row tiles, two workgroups per CU: conv1d_gemm_split_p8.hip); 256 / 128 take that form with so many columns per
   * tile, whatever the library would choose.  Every form gives the same bits.  For A/B runs and for the tests that hold the forms
   * against each other; any other value is an error, and launches without a P8 input ignore the field. */
  int32_t gsplit_p8_cols;
} fac_conv_desc;

int fac_conv1d_fwd(const fac_conv_desc* d, fac_stream_t stream);
/* Columns per tile (256 or 128) the P8-fragment form of the split GEMM picks for a launch of `rows` output rows over `cols` columns
 * in each of `ranges` column ranges (clips; 1 when flattened) on `slots` co-resident workgroups (two per CU): the cheaper of the two
 * by rounds of `slots` workgroups x columns per tile, ties to 256.  Host arithmetic only; 0 for a non-positive argument. */
int fac_gsplit_p8_tile_cols(int64_t rows, int64_t cols, int64_t ranges, int slots);
/* x (B, C, T) fp32 [-> snake(x, alpha) when alpha != NULL] -> the P8 planes described at fac_conv_desc.x_p8
 * (out: 3 planes of (B * (C / 8) * T + 1) * 16 bytes one after the other, the zero unit included).  C % 8 == 0. */
int fac_to_p8(const float* x, const float* alpha, void* out, int B, int C, int T, fac_stream_t stream);
/* Weights (C_out, C_in, K) [* scale per output channel, as fac_pack_conv_w] -> three bf16 planes hi/mid/lo with
 * hi + mid + lo == w exactly, laid out per (64-channel tile, 16-input-channel stage) for LDS-DMA.
 * `out` must hold fac_conv_w_split_bytes(C_out, C_in, K) bytes. */
int64_t fac_conv_w_split_bytes(int C_out, int C_in, int K);
/* The same for tiles of `rows` output channels: 64 (what the two functions above/below use) or, K = 7 only, 96 -- co tiles of 96
 * channels, stages of 8 input channels x 4 tap pairs (fac_conv_desc.split_rows = 96).  _bytes returns -1 for any other (K, rows). */
int64_t fac_conv_w_split_rows_bytes(int C_out, int C_in, int K, int rows);
int fac_pack_conv_w_split_rows(const float* v, const float* scale, void* out, int C_out, int C_in, int K, int rows, fac_stream_t stream);
int fac_pack_conv_w_split(const float* v, const float* scale, void* out, int C_out, int C_in, int K,
                          fac_stream_t stream);
/* Split weights of the few-output-channel 9- / 3-tap convs (conv1d_bsplit2.hip: C_out <= 32, K1 = 9 stride 1 / 2 or K1 = 3 stride
 * 1, plain or two-level taps K = K2 * K1 -- the (3, 9) / (3, 3) Conv2d stacks of dac/model/discriminator.py:101-170): v (C_out,
 * C_in, K) [* scale per C_out] as bf16 planes per (32-channel tile, 8 virtual channels).  Passed as fac_conv_desc.w_split. */
int64_t fac_conv_w_split2_bytes(int C_out, int C_in, int K, int K1);
int fac_pack_conv_w_split2(const float* v, const float* scale, void* out, int C_out, int C_in, int K, int K1, fac_stream_t stream);
/* Split weights of the 1- and 2-tap convs (conv1d_gemm_split.hip): rows r < R (output channels, or the (channel, phase) rows of
 * fac_pack_convtr_w_rows), element (r, ci, k) read at v[r * row_stride + ci * ci_stride + k * k_stride] [* row_scale[r]], written
 * as three bf16 planes per (128-row tile, 32-channel chunk) in the kernel's swizzled LDS image (one flat LDS-DMA copy per
 * stage).  C_in is padded to a multiple of 32 with zeros.  Passed as fac_conv_desc.w_split of a K = 1 / K = 2 launch.
 * in_stride S > 1: a strided conv with S < K <= 2 S taps (the encoder's k = 2 s downsampling convs, the period discriminators'
 * (5, 1) stride-3 convs): stored as 2 taps over S phase sub-signals x[S u + p] per 32-channel chunk; the launch passes
 * stride = S, K = the conv's tap count. */
int64_t fac_gemm_w_split_bytes(int R, int C_in, int K, int in_stride);
int fac_pack_gemm_w_split(const float* v, int64_t row_stride, int64_t ci_stride, int64_t k_stride, const float* row_scale, void* out,
                          int R, int C_in, int K, int in_stride, fac_stream_t stream);
/* Which kernel instantiation fac_conv1d_fwd picks for this descriptor: returns its id (>= 0) and
 * writes a printable name; lets a profiler attribute per-launch timings without re-deriving
 * the selection rule.  It runs the very planner fac_conv1d_fwd launches from (validation included) and stops before the launch,
 * so it touches no device, and a descriptor fac_conv1d_fwd rejects gets the same negative code and the same fac_last_error text
 * here.  The ids are the values of fac::ConvKernel (csrc/conv1d_api.hip), which lists what each one is; they are stable. */
int fac_conv1d_variant(const fac_conv_desc* d, char* name, int name_len);

/* Standalone Snake  y = x + sin(alpha*x)^2 / (alpha + 1e-9)  (dac/nn/layers.py:18-33) for the
 * places where it cannot be fused; alpha (C). In-place allowed. */
int fac_snake_fwd(const float* x, const float* alpha, float* y, int B, int C, int T,
                  fac_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K5  SLSTM (dac/model/encodec.py:272-288): nn.LSTM(H, H, L) over time with zero initial
 * state, gates ordered i,f,g,o, then + x (skip).
 * Work buffers are channel-major with the batch innermost and padded to a multiple of 32:
 *   BP = fac_pad32(B);  xT/yT: (H, T, BP);  pre: (4H, T, BP);  c: (H, BP).
 * (each channel's (t, b) plane is contiguous, so W_ih x + b is one GEMM with C = H, "T" = T*BP)
 * ---------------------------------------------------------------------------------------- */

/* (B, H, T) -> (H, T, BP), zero-filling batch columns B..BP-1. */
int fac_lstm_to_time_major(const float* x, float* xT, int B, int H, int T, fac_stream_t stream);
/* out(B,H,T) = yT(H,T,BP) transposed back + skip(B,H,T) (skip may be NULL); if alpha (H) is given the
 * Snake that follows the SLSTM in the model (dac/model/dac.py:95,112) is applied on the way out. */
int fac_lstm_from_time_major(const float* yT, const float* skip, const float* alpha, float* out, int B, int H, int T,
                             fac_stream_t stream);
/* W_hh (4H, H) -> layout streamed by the recurrent kernel (same element count). */
int fac_pack_lstm_whh(const float* w_hh, float* packed, int H, fac_stream_t stream);
/* One layer's recurrence: for t in 0..T-1:  gates = pre[t] + W_hh h_{t-1};  c,h update;
 * yT[:, t] = h_t.  pre already holds W_ih x_t + b_ih + b_hh.  c is scratch of 3*H*BP floats
 * (cell state + two copies of h in MFMA fragment order).
 * H must be a multiple of 64. */
int fac_lstm_layer_fwd(const float* pre, const float* whh_packed, float* yT, float* c, int T,
                       int H, int BP, fac_stream_t stream);
/* Same recurrence continued from a carried state (streaming inference): `c` is the scratch
 * of an earlier call on the same stream of frames, `step0` the number of steps already taken
 * (0 = zero initial state, identical to fac_lstm_layer_fwd). */
int fac_lstm_layer_fwd_from(const float* pre, const float* whh_packed, float* yT, float* c, int T,
                            int H, int BP, int64_t step0, fac_stream_t stream);
/* Training-mode recurrence: additionally stores the activated gates (4H, T, BP) and the cell states (H, T, BP)
 * that back-propagation through time needs (both NULL: identical to fac_lstm_layer_fwd_from). */
int fac_lstm_layer_fwd_train(const float* pre, const float* whh_packed, float* yT, float* c, float* gates_save,
                             float* c_save, int T, int H, int BP, int64_t step0, fac_stream_t stream);
/* Elementwise part of one BPTT step: dh = dy_t + rec (rec = W_hh^T dgates_{t+1}, NULL at the last step), gate
 * derivatives from the saved activations -> dgates_t (rows of stride rs), carried dc (H, BP) (first = last time step). */
int fac_lstm_gate_bwd(const float* dy_t, const float* rec, const float* gates_t, const float* c_t, const float* c_prev,
                      float* dc, float* dgates_t, int H, int BP, int64_t rs, int first, fac_stream_t stream);
/* Back-propagation through time of one layer in ONE call: for t = T-1 .. 0 the recurrent product W_hh^T dgates_{t+1} (weights from
 * fac_pack_lstm_whh_t, same element count as W_hh) and the gate derivatives.  dyT (H, T, BP): gradient w.r.t. the layer's h sequence;
 * gates (4H, T, BP) / cs (H, T, BP): what fac_lstm_layer_fwd_train saved; dgates (4H, T, BP): out.  scratch: 13 * H * BP floats. */
int fac_pack_lstm_whh_t(const float* w_hh, float* packed, int H, fac_stream_t stream);
int fac_lstm_layer_bwd(const float* dyT, const float* whh_t_packed, const float* gates, const float* cs, float* dgates, float* scratch,
                       int T, int H, int BP, fac_stream_t stream);

/* The same recurrence and its BPTT as ONE launch per layer (lstm_persist.hip): the H/8 workgroups stay resident for all T steps
 * with their slice of W_hh in registers and exchange h_t (dgates_t) through device-wide flags.  Covers zero-initial-state layers
 * with fac_lstm_persist_ok(H, B) != 0 (H in {512, 1024, 1536}, B <= 32, H/8 <= CUs, the grids of the forward and backward kernels co-resident by the runtime's occupancy figure, no earlier timeout); B = number of real batch columns, only the
 * column blocks ceil(B/16)*16 are computed and written (the caller zero-fills the padded columns of yT / saves / dgates).
 * whh16: fac_pack_lstm_whh16(W_hh, out (4H*H floats), H, transposed = 0 forward / 1 BPTT).  With NC = 16 * ceil(B/16): hfrag is
 * T * H * NC floats of scratch, fac_lstm_layer_bwd_persist's scratch (4 + 4 * T) * H * NC floats (one fresh exchange region per
 * step).  One resident layer per stream at a time (stream order guarantees it). */
int fac_lstm_persist_ok(int H, int B);
/* 1 when `stream` has (or can still get) one of the process's 64 exchange-flag slots; 0 -> run the per-step kernels on it.
 * The resident launches of one process are serialised on the device (an event chain across streams) and refuse to launch when
 * the runtime's occupancy figure says the H/8 workgroups would not be co-resident. */
int fac_lstm_persist_stream_ok(fac_stream_t stream);
int fac_pack_lstm_whh16(const float* w_hh, float* packed, int H, int transposed, fac_stream_t stream);
int fac_lstm_layer_fwd_persist(const float* pre, const float* whh16, float* hfrag, float* yT, float* gates_save, float* c_save,
                               int T, int H, int B, int BP, fac_stream_t stream);
int fac_lstm_layer_bwd_persist(const float* dyT, const float* whh16t, const float* gates, const float* cs, float* dgates,
                               float* scratch, int T, int H, int B, int BP, fac_stream_t stream);
/* Forward recurrence of a layer in one launch with W_hh . h on the bf16 matrix pipe (fp32-grade three-way bf16 split of both
 * operands, six products, fp32 accumulation -- the arithmetic of the k = 7 conv kernel): what the fp32 resident kernel cannot do
 * at 17 .. 32 batch columns, where its step is its fp32 MFMA time.  Inference only (no saved gates).  fac_lstm_persist_split_ok(H, B)
 * != 0 for H in {512, 1024, 1536}, B <= 32, H/8 <= CUs.  wsplit: fac_pack_lstm_whh_split(W_hh (4H, H), out (4H*H*6 bytes), H);
 * hsplit: T * H * 32 * 6 bytes of scratch (h_t crosses the device as three bf16 planes in MFMA B-fragment order, one fresh region
 * per step); all 32 columns of yT (H, T, BP) are computed.  Same stream / co-residency rules as the fp32 resident kernels.
 * Replaces the per-step launches of dac/model/encodec.py:272-288 at the benchmark batch. */
int fac_lstm_persist_split_ok(int H, int B);
/* Resident-kernel waits of this process that gave up after 4 s without progress (a workgroup of the grid never ran: the device
 * was shared, or a launch was not co-resident).  Such a launch finishes with meaningless results instead of trapping the
 * context; from then on fac_lstm_persist_ok / fac_lstm_persist_split_ok answer 0 (callers use the per-step kernels).  Reads a
 * host-mapped counter: no synchronisation. */
int fac_lstm_persist_timeouts(void);
/* Tells the current device where that counter lives (one one-thread kernel on `stream`, once per device; refuses inside a stream
 * capture).  Returns 1 when the device is armed.  An un-armed device answers fac_lstm_persist_ok / _split_ok = 0: a launch whose
 * waits may give up must be able to report it.  The launch entry points arm by themselves when they can. */
int fac_lstm_persist_arm(fac_stream_t stream);
/* Device-side hand-over of "a resident wait of this device has given up": dst[0] = 1.0f / 0.0f, ordered on `stream` (no host
 * synchronisation).  The optimiser puts the word behind its per-parameter flags, so it crosses the ranks with them, and then
 * fac_mask_flags_if(flags, n, poison): flags[0..n) = 0 when *poison > 0 -- fac_adamw_step_masked then steps nothing, on every
 * rank, instead of applying a gradient that came out of a bailed-out recurrence (optimizers.py:72-108 has no counterpart: the
 * reference's cuDNN LSTM cannot time out). */
int fac_lstm_abort_flag(float* dst, fac_stream_t stream);
int fac_mask_flags_if(float* flags, int n, const float* poison, fac_stream_t stream);
int fac_pack_lstm_whh_split(const float* w_hh, void* packed, int H, fac_stream_t stream);
int fac_lstm_layer_fwd_persist_split(const float* pre, const void* wsplit, void* hsplit, float* yT, int T, int H, int B, int BP,
                                     fac_stream_t stream);
/* dx = dy * (1 - y^2) */
int fac_tanh_bwd(const float* y, const float* dy, float* dx, int64_t n, fac_stream_t stream);
/* Backward of the spectral losses w.r.t. the estimate: da (+)= scale * d|a - b|/da (mode 0) or
 * scale * d|log10 max(a,eps) - log10 max(b,eps)|/da (mode 1); spec_power and stft_frames adjoints. */
int fac_pair_bwd(const float* a, const float* b, float* da, int64_t n, int mode, float eps, float scale, int accumulate,
                 fac_stream_t stream);
int fac_spec_power_bwd(const float* spec, const float* dout, float* dspec, int B, int F, int n_frames, int power,
                       fac_stream_t stream);
int fac_stft_frames_bwd(const float* dframes, float* dwave, int B, int T, int n_win, int n_frames, int hop, int pad,
                        int n_off, fac_stream_t stream);
/* Quantizer backward (dac/nn/quantize.py:55-67).  fac_vq_latent_bwd: d_ze = d_zst (straight-through, may be NULL) +
 * wc[b] * 2/(8T) * (z_e - codebook[idx]) (commitment term) and / or z_st = z_e + (codebook[idx] - z_e) (the out_proj
 * input the weight gradient needs).  fac_vq_codebook_grad: dcb[k] (+)= sum over positions that chose k of
 * wb[b] * 2/(8T) * (codebook[k] - z_e) (deterministic gather, one workgroup per code). */
int fac_vq_latent_bwd(const float* z_e, const float* codebook, const int64_t* codes, int64_t codes_bs, const float* d_zst,
                      const float* wc, float* d_ze, float* z_st, int B, int T, fac_stream_t stream);
int fac_vq_codebook_grad(const float* z_e, const float* codebook, const int64_t* codes, int64_t codes_bs, const float* wb,
                         float* dcb, int B, int T, int Kc, int accumulate, fac_stream_t stream);
/* Backward of fac_layernorm_c_affine: dx (B,C,T), dstyle (B, 2C) = [dgamma | dbeta]; stats: scratch of 2*B*T floats. */
int fac_layernorm_c_affine_bwd(const float* x, const float* style, const float* dout, float* dx, float* dstyle, float* stats,
                               int B, int C, int T, fac_stream_t stream);
/* out[b][i] = a[b][i] * w[b] + sign * c[b][i] over B rows of `per` elements (w and c may be NULL). */
int fac_rows_fma(const float* a, const float* w, const float* c, float* out, int B, int64_t per, float sign,
                 fac_stream_t stream);
/* Optimiser step on flat arenas (optimizers.py:72-108, train.py:362-374).  fac_grad_norm_clip: norm_out[0] = ||g||_2,
 * norm_out[1] = min(1, max_norm / (norm + 1e-6)) (torch clip_grad_norm_), scratch: 1024 floats.  fac_adamw_step: torch
 * AdamW with decoupled weight decay and bias correction for `step` (1-based); clip: norm_out of the call above (the
 * gradient is scaled by clip[1]) or NULL. */
int fac_grad_norm_clip(const float* g, int64_t n, float max_norm, float* scratch, float* norm_out, fac_stream_t stream);
int fac_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int64_t step, const float* clip, fac_stream_t stream);
/* The same step with the set of stepped parameters decided on the device: the arena holds n_params parameters, parameter j =
 * elements [offsets[j], offsets[j+1]) (offsets: n_params + 1 int64 device values, offsets[0] = 0, offsets[n_params] = n);
 * flags[j] > 0 <=> parameter j received a gradient on some rank (the flags ride at the tail of the gradient arena through
 * the data-parallel all-reduce, so no host round trip decides this); such a parameter's step count steps[j] (int32, device)
 * is advanced and it is updated with the bias correction of ITS count (torch keeps one count per parameter); the others are
 * left untouched -- no weight decay, no moment update -- as torch.optim.AdamW skips `grad is None` (optimizers.py:72-108
 * under accelerate's DDP, train.py:362-374).  bc: scratch of 2 * n_params floats. */
int fac_adamw_step_masked(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* offsets, int n_params,
                          const float* flags, int32_t* steps, float* bc, float lr, float beta1, float beta2, float eps,
                          float weight_decay, const float* clip, fac_stream_t stream);
/* dst[j][0..n[j]) = src[j][0..n[j]) for `count` fp32 tensors (host arrays of device pointers and element counts), a few launches
 * for all of them: folds the gradient tensors autograd produced into the optimiser's flat gradient arena (the arena is what
 * train.py:362-374's clip_grad_norm_ + optimizer.step() read). */
int fac_gather_copy(const void* const* src, void* const* dst, const int64_t* n, int count, fac_stream_t stream);
/* Training path of the FA-quantizer's side branches (modules/wavenet.py gate, modules/style_encoder.py Mish / GLU /
 * masked mean, modules/attentions.py attention): elementwise backward kernels, and attention with the probability
 * matrix P (B, H, T, T) kept in HBM so that dropout on it and the softmax backward are row kernels.
 * q, k, v, o are (B, H*dk, T); mask (B, T) float 0/1 or NULL. */
int fac_gate_bwd(const float* a, const float* d, float* da, int B, int C, int T, fac_stream_t stream);
int fac_mish_fwd(const float* x, float* y, int64_t n, fac_stream_t stream);
int fac_mish_bwd(const float* x, const float* d, float* dx, int64_t n, fac_stream_t stream);
int fac_glu_bwd(const float* a, const float* d, float* da, int B, int C, int T, fac_stream_t stream);
int fac_mul_scaled(const float* a, const float* b, float* out, float scale, int64_t n, fac_stream_t stream);
/* Training path of the voice-conversion Redecoder (train_redecoder.py:195-328).  Both kernels are deterministic: no floating-point
 * atomics, every sum in one fixed order, so the same inputs give bit-identical outputs.
 *   fac_embed_sum_bwd   adjoint of fac_embed_sum: dtables (n_tab, V, E) = for table i, the sum over (b, t) of dx[b, :, t] into row
 *                       codes[b, code_row0 + i, t] (frames added in order b, then t; rows no frame uses are zero).  V <= 1024;
 *                       codes outside [0, V) contribute nothing.  dx (B, E, T), codes (B, n_codes, T) int64.
 *   fac_gate_bwd_cond   backward of fac_gate_tanh_sigmoid WITH conditioning g (row b at g + b*g_bs): da (B, 2C, T) from
 *                       d (B, C, T), and dcond[b*dcond_bs + j] = sum over t of da[b, j, t] (j < 2C), summed in a fixed order. */
int fac_embed_sum_bwd(const float* dx, const int64_t* codes, float* dtables, int B, int n_tab, int n_codes, int code_row0, int V,
                      int E, int T, fac_stream_t stream);
int fac_gate_bwd_cond(const float* a, const float* g, int64_t g_bs, const float* d, float* da, float* dcond, int64_t dcond_bs,
                      int B, int C, int T, fac_stream_t stream);
int fac_masked_mean_bwd(const float* dout, const float* mask, float* dx, int B, int C, int T, fac_stream_t stream);
int fac_attention_probs(const float* q, const float* k, const float* mask, float* P, int B, int H, int dk, int T,
                        fac_stream_t stream);
int fac_attention_pv(const float* P, const float* v, float* o, int B, int H, int dk, int T, fac_stream_t stream);
int fac_attention_bwd_pv(const float* P_used, const float* v, const float* dO, float* dv, float* dP, int B, int H, int dk,
                         int T, fac_stream_t stream);
int fac_attention_bwd_qk(const float* P, float* dP, const float* q, const float* k, const float* mask, float* dq, float* dk_,
                         int B, int H, int dk, int T, fac_stream_t stream);
/* Backward of fac_aa_snakebeta_fwd: dx (B,C,T), dalpha / dbeta (C) w.r.t. the log-scale parameters;
 * scratch: 2 * B * C * ceil(T/256) floats. */
int fac_aa_snakebeta_bwd(const float* x, const float* alpha_log, const float* beta_log, const float* filter12, const float* dy,
                         float* dx, float* dalpha, float* dbeta, float* scratch, int B, int C, int T, fac_stream_t stream);
/* Discriminator path (dac/model/discriminator.py): layout / elementwise kernels; the convolutions run on
 * fac_conv1d_fwd (MPD: 1-D along the folded time axis, period as batch; MRD: 1-D along frequency over three stacked
 * time rows).  A non-NULL dy / non-zero `backward` selects the adjoint.
 *   leaky_relu: out = x > 0 ? x : slope*x   (backward: out = x > 0 ? dy : slope*dy); with pitch > 0 only positions
 *               t % pitch < valid of every length-T row are kept, the rest set to zero (row-concatenated MPD signals)
 *   period_fold: (B, T) -> B*period rows of `pitch` columns laid one after another (L data columns, then zeros),
 *               reflect-extended on the right to L*period samples
 *   zero_insert: (rows, T) -> (rows, (T-1)*stride + 1), zeros between samples (strided conv data gradient)
 *   row_stack3: (rows = B*T, C, F) -> (rows, 3C, F): time rows t-1, t, t+1 stacked (zero outside a clip)
 *   spec_to_rows: one frequency band [f0, f0+Fb) of spec (B, 2*Ft, T) = [re|im] -> (B*T, 2, Fb)
 *   pad_reflect: (B, T) -> (B, pad_l + T + pad_r)
 *   disc_preprocess: z = 0.8 (x - mean)/(max|x - mean| + 1e-9) per clip; stats: 4*B floats kept for the backward */
/* rows_per_group > 0: besides the column mask, rows (position / pitch) with row % rows_per_group >= valid_rows are zero
 * (the all-zero separator rows between clips of the row-concatenated spectrogram layout). */
int fac_leaky_relu(const float* x, const float* dy, float* out, int64_t n, float slope, int T, int pitch, int valid,
                   int rows_per_group, int valid_rows, fac_stream_t stream);
int fac_period_fold(const float* x, float* out, int B, int T, int period, int L, int pitch, int backward, fac_stream_t stream);
int fac_zero_insert(const float* dy, float* up, int64_t rows, int T, int stride, fac_stream_t stream);
int fac_row_stack3(const float* x, float* out, int64_t rows, int T, int C, int F, int backward, fac_stream_t stream);
/* Multi-resolution discriminator in the row-concatenated layout: spec (B, 2*Ft, T) [re | im] band [f0, f0 + Fb) ->
 * cat (2, B*(T+1)*pitch): row r = b*(T+1) + t holds the band's Fb bins followed by zeros; row t = T of every clip is an
 * all-zero separator (the time padding of the (3, k) convs).  backward: the adjoint, accumulating disjoint bands into a
 * zero-initialised dspec. */
int fac_spec_to_cat(const float* src, float* dst, int B, int Ft, int T, int f0, int Fb, int pitch, int backward, fac_stream_t stream);
int fac_spec_to_rows(const float* src, float* dst, int B, int Ft, int T, int f0, int Fb, int backward, fac_stream_t stream);
int fac_pad_reflect(const float* x, float* out, int B, int T, int pad_l, int pad_r, fac_stream_t stream);
int fac_disc_preprocess(const float* x, const float* dz, float* out, float* stats, int B, int T, fac_stream_t stream);
/* F.cross_entropy (mean) over rows: logits (N, C), labels (N) int64.  loss (1 float) and / or dlogits = (softmax -
 * onehot) * grad_scale; scratch: N floats. */
int fac_cross_entropy(const float* logits, const int64_t* labels, float* loss, float* dlogits, float* scratch, int64_t N,
                      int C, float grad_scale, fac_stream_t stream);
/* FocalLoss on the mean cross entropy (losses.py:264-276; train.py:153 gamma = 2): out2[0] = (1 - exp(-ce))^gamma * ce,
 * out2[1] = d out2[0] / d ce.  ce, out2: device scalars. */
int fac_focal_scalar(const float* ce, float* out2, float gamma, fac_stream_t stream);
/* Random-crop batching of train.py:188-212 on the device: dst[b][c][t] = src[b][c][start[b] * scale + t] (0 outside);
 * src (B, C, T_src), dst (B, C, T_dst), start (B) int64 device values in units of `scale` samples. */
int fac_crop_rows(const float* src, float* dst, const int64_t* start, int B, int C, int64_t T_src, int T_dst, int scale,
                  fac_stream_t stream);
/* Left-context buffer of a streaming causal conv: every row of buf (rows x cap) holds
 * [hist columns of history | n_prev columns appended last time]; moves the last `hist` columns to the
 * front (skipped when n_prev == 0) and appends src (rows x n_new, dense) behind them.  hist <= 2048. */
int fac_stream_push(float* buf, const float* src, int64_t rows, int64_t cap, int hist, int n_prev, int n_new,
                    fac_stream_t stream);

/* Weights of a conv's data-gradient conv for the split-bf16 kernels, materialised in one pass: out (C_in, C_out, K)[ci][co][k] =
 * v (C_out, C_in, K)[co][ci][K-1-k] * scale[co] (scale: fac_wn_scale or NULL).  Pack the result with fac_pack_conv_w_split* . */
int fac_flip_transpose_w(const float* v, const float* scale, float* out, int C_out, int C_in, int K, fac_stream_t stream);

/* Batched weight preparation (round 6).  The reference's weight_norm recomputes w = g * v / ||v|| in a pre-forward hook of every
 * conv (dac/model/encodec.py:42-51, dac/nn/layers.py:9-14); here that is one small launch per tensor and layout (fac_wn_scale, then
 * fac_pack_*): ~290 launches of a configs[1] forward, ~1 700 of a train step.  Between fac_prep_begin() and fac_prep_end() the calling
 * thread's fac_wn_scale, fac_pack_conv_w, fac_pack_convtr_w, fac_pack_convtr_w_rows, fac_flip_transpose_w, fac_pack_conv_w_split,
 * fac_pack_gemm_w_split, fac_pack_conv_w_split2 and fac_pack_conv_w_bwd calls are RECORDED (arguments checked, nothing launched) under
 * the phase set by fac_prep_set_phase (0 at begin; a job that reads another job's output needs a higher phase).  fac_prep_end() uploads
 * the job tables and returns a plan id (>= 0; negative = error code).  fac_prep_replay() re-runs every job of the plan from the CURRENT
 * contents of its input tensors -- one launch per (phase, kernel family), phases in order -- with the arithmetic of the single launches
 * (same device functions: results are bit-identical).  The pointers recorded must stay valid for the life of the plan.  fac_prep_free()
 * requires that no replay of the plan is still executing. */
int fac_prep_begin(void);
int fac_prep_set_phase(int phase);
int fac_prep_abort(void);
int fac_prep_end(void);
int fac_prep_replay(int plan, fac_stream_t stream);
int fac_prep_info(int plan, int* n_jobs, int* n_launches);
int fac_prep_free(int plan);

/* ------------------------------------------------------------------------------------------
 * Backward of the conv stack (first kernels of the training step; autograd semantics of
 * dac/model/encodec.py SConv1d / SConvTranspose1d, dac/nn/layers.py snake, weight_norm).
 *
 * bwd_data of a stride-1 conv: run fac_conv1d_fwd over dy with the weights packed by fac_pack_conv_w_bwd
 * (taps flipped, channels transposed; C_out becomes the input-channel axis: rows up to fac_cin_pad(C_out),
 * columns C_in_pad = pad32(C_in), zero-filled by the caller), pad_left = (K-1)*dilation, zero padding,
 * T_out = padded input length; then fac_pad_fold_bwd maps the gradient of the padded signal back to x
 * (reflection: a padded position's gradient is added to the sample it mirrors; a signal not longer than its pad mirrors
 * about the ends of pad1d's zero extension, as the forward reads it).  Strided convs (K = 2*stride):
 * the transposed-conv launch on the forward weights (fac_pack_convtr_w), then the same fold.
 * ---------------------------------------------------------------------------------------- */
int fac_pack_conv_w_bwd(const float* v, const float* scale, float* packed, int C_out, int C_in, int K, int C_in_pad,
                        fac_stream_t stream);
int fac_pad_fold_bwd(const float* dxpad, float* dx, int B, int C, int T, int Tp, int pad_left, int pad_mode,
                     fac_stream_t stream);
/* fac_pad_fold_bwd in place for reflect padding, edges only: adds every mirrored padded position of dxpad (B, C, Tp) onto the sample
 * it mirrors (dac/model/encodec.py:96-113 backward); afterwards dx[b][c][j] IS dxpad[b][c][pad_left + j].  Needs T > pad_left +
 * pad_right + 1 (the two edges' target samples disjoint).  Zero padding needs no call at all (the window is the gradient). */
int fac_pad_fold_edges(float* dxpad, int B, int C, int T, int Tp, int pad_left, fac_stream_t stream);
/* dW (C_out, C_in, K) = sum over (b, t) of dy[b][co][t] * xpad[b][ci][t*stride + k*dilation]; ws: scratch of
 * fac_conv1d_bwd_weight_ws_bytes(...) bytes (partial sums per (b, t) range, added in a fixed order). */
int64_t fac_conv1d_bwd_weight_ws_bytes(int B, int C_in, int C_out, int T_out, int K);
int fac_conv1d_bwd_weight(const float* x, const float* dy, float* dw, void* ws, int64_t ws_bytes, int B, int C_in,
                          int T_in, int C_out, int T_out, int K, int stride, int dilation, int pad_left, int pad_mode,
                          int K1, int dilation2, fac_stream_t stream);
/* The k = 1, stride-1 case with few channels and long signals (the ResidualUnit tails of dac/model/dac.py:25-42 at C = 64 / 96 / 192:
 * dW[co][ci] = sum over (b, t) of dy[b][co][t] * x[b][ci][t]) straight from the fp32 tensors on the fp32 matrix pipe
 * (conv1d_wgrad_k1.hip): both tensors are read once, no operand planes.  The query returns the workspace size (partial sums of the
 * workgroups, added in a fixed order) or -1 when the shape does not run here (channel counts: multiples of 32 in [64, 192];
 * T >= 4096, T % 4 == 0). */
int64_t fac_conv1d_bwd_weight_k1_ws_bytes(int B, int C_in, int C_out, int T);
/* The same query for the tensors at hand: also -1 when x or dy is not 16-byte aligned (the kernel reads both with 16-byte loads;
 * fac_conv1d_bwd_weight_k1 refuses such pointers). */
int64_t fac_conv1d_bwd_weight_k1_ws_bytes_for(const float* x, const float* dy, int B, int C_in, int C_out, int T);
int fac_conv1d_bwd_weight_k1(const float* x, const float* dy, float* dw, float* db, void* ws, int64_t ws_bytes, int B, int C_in, int C_out,
                             int T, fac_stream_t stream);   /* db: (C_out) bias gradient sum over (b, t) of dy, or NULL */
/* The same kernel for stride-1 convs with few input channels and taps (first layers: the encoder's 1 -> 64 k = 7 conv,
 * dac/model/dac.py:82; the multi-resolution discriminator's 2 -> 32 (3, 9) convs, dac/model/discriminator.py:101-130): the C_in * K
 * columns of dW are shifted views of the input rows.  xpad (B, C_in, Tx) is the conv's PADDED input (the caller pads: left padding,
 * right padding, then zeros up to Tx >= fac_conv1d_bwd_weight_taps_tx);
 * dW (C_out, C_in, K)[co][ci][k] = sum over (b, t < T_out) of dy[b][co][t] * xpad[b][ci][t + (k / K1) * dilation2 + (k % K1) * dilation]
 * (K1 = K: plain taps).  C_out = 32 or 64, C_in * K <= 64, T_out >= 4096; the query returns -1 otherwise.  db as above. */
int64_t fac_conv1d_bwd_weight_taps_tx(int T_out, int K, int K1, int dilation, int dilation2);
int64_t fac_conv1d_bwd_weight_taps_ws_bytes(int B, int C_in, int C_out, int T_out, int K, int K1, int dilation, int dilation2);
/* ... and for the dy at hand: also -1 when dy is not 16-byte aligned (xpad may sit anywhere: its taps are 4-byte aligned loads). */
int64_t fac_conv1d_bwd_weight_taps_ws_bytes_for(const float* dy, int B, int C_in, int C_out, int T_out, int K, int K1, int dilation,
                                                int dilation2);
int fac_conv1d_bwd_weight_taps(const float* xpad, const float* dy, float* dw, float* db, void* ws, int64_t ws_bytes, int B, int C_in, int Tx,
                               int C_out, int T_out, int K, int K1, int dilation, int dilation2, fac_stream_t stream);
/* The same gradient on the bf16 matrix pipe with fp32-grade operand splitting (conv1d_wgrad_split.hip; same arguments
 * and result layout as fac_conv1d_bwd_weight, error vs fp64 no larger than the fp32 MFMA's).  The workspace query
 * returns -1 for a (K, stride, dilation) the kernel does not cover: use fac_conv1d_bwd_weight then.  K1 / dilation2:
 * two-level taps as in fac_conv_desc (0 = plain); dW stays (C_out, C_in, K) with k = k2 * K1 + k1.  The workspace also
 * holds the pre-split bf16 planes of both operands. */
int64_t fac_conv1d_bwd_weight_split_ws_bytes(int B, int C_in, int T_in, int C_out, int T_out, int K, int stride, int dilation,
                                             int K1, int dilation2);
/* What fac_conv1d_bwd_weight_split / _split_db will do for this shape, from the host function the launch itself reads (no device
 * call).  Returns 0 and fills form[0..7], or -1 where the workspace query returns -1.  want_db: a bias gradient is requested.
 *   form[0] kernel: 0 kmajor, 1 kmajor_ksplit (k = 7 wave layout), 2 planes<10,3>, 3 planes<14,3>, 4 planes<19,2>
 *   form[1] slices S of the (b, t) range      form[2] 32-step tiles per slice      form[3] tiles of the last slice
 *   form[4] XCD-aware workgroup order         form[5] 128-row tiles of dW
 *   form[6] row tiles with <= 96 real rows on the column-split wave layouts (0 with FAC_WGRAD_NARROW=0 and on the planes kernels)
 *   form[7] the requested bias gradient is folded into the dy split pass (fac_conv1d_bwd_weight_split_db_ok) */
int fac_conv1d_bwd_weight_split_form(int B, int C_in, int T_in, int C_out, int T_out, int K, int stride, int dilation, int K1,
                                     int dilation2, int want_db, int* form);
int fac_conv1d_bwd_weight_split(const float* x, const float* dy, float* dw, void* ws, int64_t ws_bytes, int B, int C_in, int T_in,
                                int C_out, int T_out, int K, int stride, int dilation, int pad_left, int pad_mode, int K1,
                                int dilation2, fac_stream_t stream);
/* The same launch with the bias gradient db[co] = sum over (b, t) of dy folded into the dy operand's split pass (no separate
 * pass over dy); k-major shapes only: C_in * K2 >= 16 and B * C_out <= 65535 (query: fac_conv1d_bwd_weight_split_db_ok). */
int fac_conv1d_bwd_weight_split_db_ok(int B, int C_in, int T_in, int C_out, int T_out, int K, int stride, int dilation, int K1,
                                      int dilation2);
int fac_conv1d_bwd_weight_split_db(const float* x, const float* dy, float* dw, float* db, void* ws, int64_t ws_bytes, int B, int C_in,
                                   int T_in, int C_out, int T_out, int K, int stride, int dilation, int pad_left, int pad_mode, int K1,
                                   int dilation2, fac_stream_t stream);
/* w = g*v/||v|| per row (n_rows x row_len): dv, dg from dW. */
int fac_weight_norm_bwd(const float* v, const float* g, const float* dw, float* dv, float* dg, int n_rows, int row_len,
                        fac_stream_t stream);
/* y = x + sin^2(alpha x)/(alpha + 1e-9): dx (B,C,T) and dalpha (C).  scratch: 32*C floats (partial sums of the
 * two-stage, fixed-order channel reductions). */
int fac_snake_bwd(const float* x, const float* alpha, const float* dy, float* dx, float* dalpha, float* scratch, int B, int C,
                  int T, fac_stream_t stream);
/* The same with its neighbours fused in: dx = add + dy * dsnake/dx (add: the second gradient of a tensor with two consumers, the
 * ResidualUnit skip of dac/model/dac.py:38-42 -- NULL: none), dbias[c] = sum over (b, t) of dx (the bias gradient of the conv
 * that produced x -- NULL: skipped).  scratch: 64*C floats. */
int fac_snake_bwd_fused(const float* x, const float* alpha, const float* dy, const float* add, float* dx, float* dalpha,
                        float* dbias, float* scratch, int B, int C, int T, fac_stream_t stream);
/* The same with the rows of dy `dy_row_stride` (>= T) elements apart: dy is then typically the window [pad_left, pad_left + T) of the
 * padded gradient rows a data-gradient conv wrote, after fac_pad_fold_edges -- no separate un-padding pass over the tensor. */
int fac_snake_bwd_fused_rs(const float* x, const float* alpha, const float* dy, long long dy_row_stride, const float* add, float* dx,
                           float* dalpha, float* dbias, float* scratch, int B, int C, int T, fac_stream_t stream);
/* db[c] = sum over (b, t) of dy; scratch: 32*C floats. */
int fac_bias_grad(const float* dy, float* db, float* scratch, int B, int C, int T, fac_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K7  factorized VQ step (dac/nn/quantize.py:34-94 VectorQuantize.forward + the residual
 * bookkeeping of ResidualVectorQuantize.forward :173-193; search identical to
 * quantize/fvq.py:101-116):
 *   z_e = W_in r + b_in (1x1 conv D->8); e = z_e/max(||z_e||,1e-12); c~ = cb/max(||cb||,1e-12);
 *   idx = first argmax_k -( (||e||^2 - 2 e.c~_k) + ||c~_k||^2 );  z_q = cb[idx] (raw rows);
 *   z_st = z_e + (z_q - z_e);  out = W_out z_st + b_out;
 *   zq_acc += out * mask[b];  residual -= out;
 *   loss_part[b][tile] = sum_{d,t in tile} (z_e - z_q)^2   (commitment == codebook value).
 * Aliasing: residual may be z_in itself (every RVQ stage after the first updates the residual in place), and nothing else
 *   may overlap.  That is safe because a workgroup reads and writes only the frames it owns: frame (b, t) of z_in is read
 *   for the in-projection and once more, by the thread that then writes residual[b][c][t], before that write; no workgroup
 *   reads a frame another one writes.  zq_acc is read and written by the same thread in the same way.
 * Routes: with T <= 8, loss_part == NULL, D <= 4096 and the LDS formula below satisfied, one workgroup per (b, t) frame
 *   (streaming hops); otherwise one workgroup per (b, tile of 16 frames), on a grid padded to a multiple of 8.  Both
 *   routes give the same bits in every output they share; only the tile route writes loss_part.
 * Limits: B <= 65535; the codebook, its norms and the in-projection weights live in LDS (160 KiB), in floats
 *   tile route   8 Kc + roundup4(Kc) + 1152 + 8 D               <= 40960   (Kc = 1024: D <= 3824; rejected beyond)
 *   frame route  8 Kc + roundup4(Kc) + roundup4(D) + 8 D + 552  <= 40960   (Kc = 1024: D <= 3465; the tile route beyond)
 * ---------------------------------------------------------------------------------------- */
typedef struct fac_vq_desc {
  float* residual;        /* (B, D, T) in/out: r <- r - out ; may be NULL to skip the update */
  const float* z_in;      /* (B, D, T) the vectors to quantize (may alias residual) */
  float* zq_acc;          /* (B, D, T) in/out: += out*mask ; NULL to skip */
  float* zq_out;          /* (B, D, T) out (this quantizer's projected output) ; NULL to skip */
  const float* w_in;      /* packed (D, 1, 32) from fac_pack_conv_w (C_out = 8 -> pad 32) */
  const float* b_in;      /* (8) */
  const float* codebook;  /* (Kc, 8) raw */
  const float* w_out;     /* (D, 8) out_proj weight_v rows ([c][d], torch layout (D,8,1)) */
  const float* w_out_scale; /* (D) weight-norm scale g/||v|| from fac_wn_scale, or NULL (== 1) */
  const float* b_out;     /* (D) */
  const float* mask;      /* (B) multiplies out in zq_acc (quantizer dropout), NULL == 1 */
  int64_t* codes;         /* (B, T) at codes[b*codes_bs + t] */
  float* z_e;             /* (B, 8, T) projected latents, or NULL */
  float* loss_part;       /* (B, n_tiles) partial sums of (z_e-z_q)^2, n_tiles = fac_vq_loss_tiles(T) */
  int64_t codes_bs;
  int32_t B, D, T, Kc;
} fac_vq_desc;

int fac_vq_fwd(const fac_vq_desc* d, fac_stream_t stream);
/* Number of time tiles fac_vq_fwd cuts T frames into (= the row length of loss_part; 16 frames per workgroup). */
int fac_vq_loss_tiles(int T);

/* Codes -> decoder input (dac/nn/quantize.py:72-76 decode_code + :200-220 ResidualVectorQuantize.from_codes for the
 * prosody, content and residual RVQs, then the tail of FAquantizer.forward_v2, modules/quantize.py:436-449, eval):
 *   z_q_i = W_out_i cb_i[code_i] + b_out_i  (W_out = weight_v * scale, 1x1 conv 8 -> D);  z_r = 0 + z_q_0 + z_q_1 + ... per RVQ;
 *   outs = LayerNorm_C((z[0] + z[1]) + z[2]) (eps 1e-5, no affine) * gamma + beta,  style (B, 2D) = [gamma | beta].
 * Per value the same roundings as fac_vq_fwd's out-projection, fac_add and fac_layernorm_c_affine.  Any number of
 * quantizers per RVQ (0 included: that RVQ's sum is 0), at most FAC_VQ_DECODE_MAX_Q in all.  Codes are NOT range
 * checked: an index outside [0, Kc) is clamped for the load (memory safety only; validate on the host). */
#define FAC_VQ_DECODE_MAX_Q 16
typedef struct fac_vq_decode_desc {
  const int64_t* codes[3];  /* RVQ r (0 prosody, 1 content, 2 residual): code of its quantizer i for clip b, frame t at
                               codes[r][b*codes_bs[r] + i*codes_qs[r] + t]; may be NULL when n_q[r] == 0 */
  int64_t codes_bs[3];
  int64_t codes_qs[3];
  int32_t n_q[3];           /* quantizers of each RVQ */
  const float* codebook[FAC_VQ_DECODE_MAX_Q];    /* (Kc, 8) raw rows; quantizers of RVQ 0, then RVQ 1, then RVQ 2 */
  const float* w_out[FAC_VQ_DECODE_MAX_Q];       /* (D, 8) out_proj weight_v ([c][d], torch layout (D,8,1)) */
  const float* w_out_scale[FAC_VQ_DECODE_MAX_Q]; /* (D) weight-norm scale from fac_wn_scale, or NULL (== 1) */
  const float* b_out[FAC_VQ_DECODE_MAX_Q];       /* (D) */
  const float* style;       /* (B, 2D) = [gamma | beta] */
  float* outs;              /* (B, D, T) decoder input */
  float* z[3];              /* (B, D, T) per-RVQ sums z_p / z_c / z_r, each NULL to skip */
  int32_t B, D, T, Kc;
} fac_vq_decode_desc;

int fac_vq_decode(const fac_vq_decode_desc* d, fac_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Packed codes: the payload of the bitstream (csrc/bitpack.hip).  This comment is the normative layout.
 *
 * One clip of F frames with quantizer counts (n_p, n_c, n_r), Q = n_p + n_c + n_r in 1..FAC_VQ_DECODE_MAX_Q, and a field
 * width `bits` in 1..16 (default ceil(log2(codebook_size)), 10 for the shipped model) is the little-endian byte string of
 *     N = sum over t < F, q < Q of  (code[q][t] & (2^bits - 1)) << (bits * (t * Q + q))
 *     payload = N.to_bytes(ceil(F * Q * bits / 8), "little")
 * Frame-major; within a frame the fields run in quantizer order (prosody rows, content rows, residual rows); fields are
 * LSB-first with no padding between fields or frames; the unused high bits of the last byte are 0.  Any run of whole frames
 * is therefore a self-contained bit range (k frames of the shipped model: ceil(60 k / 8) bytes).
 *   bits = 10, p = [1], c = [2, 3], r = [4, 5, 1023], F = 1          ->  01 08 30 00 01 05 fc 0f
 *   ... then a frame p = [512], c = [0, 1], r = [1000, 7, 341]       ->  01 08 30 00 01 05 fc 0f 20 00 01 a0 7f 40 55
 *
 * Device buffer: (B, row_bytes) uint8 with row_bytes = fac_codes_row_bytes(T, Q, bits) = 4 * ceil(ceil(T Q bits / 8) / 4),
 * whole 32-bit words.  With lens ((B,) int32 FRAMES on the device, never read on the host, clamped to [0, T]) row b holds
 * its clip's min(lens[b], T) frames and every bit behind them up to row_bytes is 0.
 *
 * fac_codes_pack is store-only: one thread per 32-bit output word gathers the fields that overlap it, each masked to `bits`
 * (a code outside [0, 2^bits) cannot disturb its neighbours), and writes the word once -- no atomics, no read of `out`.
 * Every word of [0, row_bytes) of every row is written; nothing outside, the gap up to out_bs included.
 * fac_codes_unpack is the inverse: it reads `in` byte by byte (at most 3 per field; no alignment of `in` or in_bs assumed)
 * and writes every code of the (B, n_q[r], T) tensors, code 0 for frames t >= lens[b].  Neither checks code VALUES (validate
 * on the host, as everywhere else).  Both refuse, before any launch: bits outside 1..16, Q outside 1..16, a NULL code
 * pointer with n_q > 0, a row stride that is too small (pack: or no multiple of 4), B or T < 1.
 * ---------------------------------------------------------------------------------------- */
typedef struct fac_codes_pack_desc {
  const int64_t* codes[3];  /* as in fac_vq_decode_desc: codes[r][b*codes_bs[r] + i*codes_qs[r] + t]; NULL when n_q[r] == 0 */
  int64_t codes_bs[3];
  int64_t codes_qs[3];
  int32_t n_q[3];
  const int32_t* lens;      /* (B,) frames, or NULL (every row has T frames) */
  uint8_t* out;             /* (B, out_bs) bytes, 4-byte aligned */
  int64_t out_bs;           /* row stride in bytes: a multiple of 4, >= fac_codes_row_bytes(T, Q, bits) */
  int32_t B, T, bits;
} fac_codes_pack_desc;

typedef struct fac_codes_unpack_desc {
  const uint8_t* in;        /* (B, in_bs) bytes */
  int64_t in_bs;            /* row stride in bytes, any value >= ceil(T Q bits / 8) */
  int64_t* codes[3];        /* written: codes[r][b*codes_bs[r] + i*codes_qs[r] + t]; NULL when n_q[r] == 0 */
  int64_t codes_bs[3];
  int64_t codes_qs[3];
  int32_t n_q[3];
  const int32_t* lens;      /* (B,) frames, or NULL */
  int32_t B, T, bits;
} fac_codes_unpack_desc;

int fac_codes_pack(const fac_codes_pack_desc* d, fac_stream_t stream);
int fac_codes_unpack(const fac_codes_unpack_desc* d, fac_stream_t stream);
/* Bytes of one row of the device buffer (host helper); -1 for a non-positive argument. */
int64_t fac_codes_row_bytes(int T, int Q, int bits);

/* Nearest-code search only, on already-projected latents (N, 8) row-major -> idx (N) int64.
 * The isolated kernel of dac/nn/quantize.py:78-94 / quantize/fvq.py:101-116. */
int fac_vq_search(const float* latents, const float* codebook, int64_t* idx, int64_t N, int Kc,
                  fac_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Small fused elementwise / reduction ops of the quantizer (modules/quantize.py:375-454).
 * ---------------------------------------------------------------------------------------- */

/* acts = tanh((a+g)[:, :C]) * sigmoid((a+g)[:, C:])  (modules/commons.py:113-120), a (B,2C,T) -> (B,C,T);
 * g: optional per-clip conditioning (row b at g + b*g_bs, 2C values broadcast over time:
 * modules/wavenet.py:146-155 with gin_channels), or NULL. */
int fac_gate_tanh_sigmoid(const float* a, const float* g, int64_t g_bs, float* out, int B, int C, int T,
                          fac_stream_t stream);
/* Code-embedding sum of the Redecoder (modules/redecoder.py:35-45): out (B, E, T) (+)= sum over n_tab
 * tables (n_tab, V, E) of table_i[codes[b, code_row0 + i, t]]; codes (B, n_codes, T) int64. */
int fac_embed_sum(const int64_t* codes, const float* tables, float* out, int B, int n_tab, int n_codes,
                  int code_row0, int V, int E, int T, int accumulate, fac_stream_t stream);
/* GLU residual: out = res + a[:, :C] * sigmoid(a[:, C:])  (modules/style_encoder.py:26-31) */
int fac_glu_residual(const float* a, const float* res, float* out, int B, int C, int T,
                     fac_stream_t stream);
/* out = a + b (same shape, n elements);  out = a - b - c */
int fac_add(const float* a, const float* b, float* out, int64_t n, fac_stream_t stream);
int fac_sub2(const float* a, const float* b, const float* c, float* out, int64_t n,
             fac_stream_t stream);
/* x[b, c, t] *= mask[b, t]  in place (mask is float 0/1). */
int fac_mul_mask(float* x, const float* mask, int B, int C, int T, fac_stream_t stream);
/* WaveNet skip accumulation (modules/wavenet.py:160-165):
 *   rs (B, 2C, T): x = (x + rs[:, :C]) ; out += rs[:, C:]   (last layer: rs (B,C,T): out += rs) */
int fac_wn_res_skip(const float* rs, float* x, float* out, int B, int C, int T, int last,
                    fac_stream_t stream);
/* 2-head style self-attention core (modules/attentions.py:168-199) on q,k,v (B, H*dk, T):
 * scores = (q/sqrt(dk))^T k, masked_fill(mask==0,-1e4), softmax over keys, out = p v. */
int fac_attention(const float* q, const float* k, const float* v, const float* mask, float* out,
                  int B, int n_heads, int dk, int T, fac_stream_t stream);
/* The same attention with a running max and sum over key tiles (csrc/attention_stream.hip): no score row is ever held, LDS use
 * does not depend on T.  Semantics as fac_attention (a masked pair's score is REPLACED by -1e4; keys past T weigh exactly 0);
 * dk <= 256.  fac_attention takes this route by itself where fac_attention_route says so. */
int fac_attention_stream(const float* q, const float* k, const float* v, const float* mask, float* out,
                         int B, int n_heads, int dk, int T, fac_stream_t stream);
/* The kernel fac_attention launches for (dk, T), from the shapes alone: FAC_ATTN_LDS while (16 dk + 16 T) * 4 bytes fit the
 * 160 KiB of LDS, FAC_ATTN_STREAM past that. */
#define FAC_ATTN_LDS 0
#define FAC_ATTN_STREAM 1
int fac_attention_route(int dk, int T);
/* The form of fac_attention's launch for (dk, T), from the shapes alone.  On the FAC_ATTN_LDS route: FAC_ATTN_FORM_TILED, the
 * register-tiled kernel (csrc/attention_tiled.hip), while fac_attention_tiled_fits -- dk <= 256 and one pass of V (256 x 36
 * floats) plus 32 score rows of T rounded up to 32 keys fit the 160 KiB of LDS, i.e. T <= 992 -- and FAC_ATTN_FORM_SERIAL, the
 * kernel of csrc/misc.hip with one thread per output, past that.  The two return the same bits for the same inputs.
 * fac_attention_tiled / fac_attention_serial launch one form whatever fac_attention would choose (arguments as fac_attention;
 * a shape the form does not take is FAC_ERR_ARG). */
#define FAC_ATTN_FORM_TILED 0
#define FAC_ATTN_FORM_SERIAL 1
#define FAC_ATTN_FORM_STREAM 2
int fac_attention_form(int dk, int T);
int fac_attention_tiled_fits(int dk, int T);
int fac_attention_tiled(const float* q, const float* k, const float* v, const float* mask, float* out,
                        int B, int n_heads, int dk, int T, fac_stream_t stream);
int fac_attention_serial(const float* q, const float* k, const float* v, const float* mask, float* out,
                         int B, int n_heads, int dk, int T, fac_stream_t stream);
/* Tile sizes of fac_attention_stream: which = 0 queries per workgroup, 1 keys per LDS tile. */
int fac_attention_stream_tile(int which);
/* masked temporal average pool (modules/style_encoder.py:83-91): out[b,c] = sum_t x / sum_t mask */
int fac_masked_mean(const float* x, const float* mask, float* out, int B, int C, int T,
                    fac_stream_t stream);
/* Timbre-conditioned norm (modules/quantize.py:444-449): LayerNorm over C (eps 1e-5, no affine)
 * per (b,t), then * gamma[b,c] + beta[b,c];  style (B, 2C) = [gamma | beta]. */
int fac_layernorm_c_affine(const float* x, const float* style, float* out, int B, int C, int T,
                           fac_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K8 / K11  STFT framing + spectral losses (torchaudio MelSpectrogram in
 * modules/quantize.py:228-242; audiotools STFT/mel in dac/nn/loss.py:203-228,294-327).
 * The DFT itself runs through fac_conv1d_fwd as a GEMM against a windowed cos/sin basis.
 * ---------------------------------------------------------------------------------------- */

/* frames[b][n][f] = wave_reflectpad[b][f*hop + n + n_off - pad],  n < n_win, f < n_frames
 * (centre=True framing: pad = n_fft/2, reflect; n_off = offset of the first non-zero window
 * tap inside the n_fft frame). wave (B, T). */
int fac_stft_frames(const float* wave, float* frames, int B, int T, int n_win, int n_frames,
                    int hop, int pad, int n_off, fac_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Batches of clips with different lengths: the clips are right-padded with zeros to T samples, lens (B,) int32 on the
 * device holds every row's own length in samples.  No call reads lens on the host; a length is clamped to [0, T] before it
 * indexes anything, so validating it (e.g. pad < length) is the caller's business, where the lengths originate.
 * ---------------------------------------------------------------------------------------- */

/* fac_stft_frames with per-row lengths: row b reflects at lens[b] and has lens[b] / hop frames, bit-equal to
 * fac_stft_frames on wave[b, :lens[b]]; frame columns f >= lens[b] / hop are written as zeros.  frames (B, n_win, n_frames). */
int fac_stft_frames_ragged(const float* wave, const int32_t* lens, float* frames, int B, int T, int n_win, int n_frames,
                           int hop, int pad, int n_off, fac_stream_t stream);
/* x[b, :, t] = 0 for t >= lens[b] / unit, in place (unit = hop for frame-rate tensors, 1 for samples); x (B, C, T) fp32, or
 * int64 (code tensors) for the _i64 form.  Store-only: 16-byte stores over the tails, nothing else is touched. */
int fac_mask_tail(float* x, const int32_t* lens, int B, int C, int T, int unit, fac_stream_t stream);
int fac_mask_tail_i64(int64_t* x, const int32_t* lens, int B, int C, int T, int unit, fac_stream_t stream);
/* What a non-causal conv pads behind a clip that it sees alone, written behind every clip of a right-padded batch, in place
 * (DESIGN.md 23).  Here lens counts FRAMES and x (B, C, T) fp32 has `mul` columns per frame: L_b = clamp(lens[b] * mul, 0, T).
 * For j in [0, min(n, T - L_b)) and every channel: mode FAC_PAD_REFLECT writes x[b, c, L_b + j] = x[b, c, L_b - 2 - j] (0 where
 * that source index is negative), mode FAC_PAD_ZERO writes 0.  Reads lie below L_b, writes at or above it; nothing else is touched. */
int fac_edge_tail(float* x, const int32_t* lens, int B, int C, int T, int mul, int n, int mode, fac_stream_t stream);
/* mask[b, f] = f < lens[b] / unit ? 1 : 0  (B, F) fp32, the mask of fac_attention / fac_masked_mean;
 * n_valid (B,) int32 = min(lens[b] / unit, F), or NULL. */
int fac_frame_mask(const int32_t* lens, float* mask, int32_t* n_valid, int B, int F, int unit, fac_stream_t stream);
/* spec (B, 2F, n_frames) rows [0,F) = Re, [F,2F) = Im  ->  out (B, F, n_frames):
 * power == 2: re^2+im^2 ; power == 1: sqrt(re^2+im^2). */
int fac_spec_power(const float* spec, float* out, int B, int F, int n_frames, int power,
                   fac_stream_t stream);
/* Deterministic two-stage reduction:  out[0] = scale * sum_i f(a_i, b_i)
 *   mode 0: |a-b| ; mode 1: |log10(max(a,eps)) - log10(max(b,eps))| (pow folded in by caller);
 *   mode 2: (a-b)^2.  scratch >= 1024 floats. */
int fac_reduce_pair(const float* a, const float* b, float* out, float* scratch, int64_t n,
                    int mode, float eps, float scale, int accumulate, fac_stream_t stream);

/* K13  anti-aliased SnakeBeta activation of the predictor heads (alias_free_torch/act.py:24-29:
 * 2x Kaiser-sinc upsample -> SnakeBeta with log-scale alpha/beta, modules/quantize.py:77-90 -> 2x
 * low-pass downsample), fused into one pass.  x, y (B, C, T); alpha_log, beta_log (C); filter12 = the
 * 12-tap filter both resamplers share (alias_free_torch/filter.py:27-58). */
int fac_aa_snakebeta_fwd(const float* x, const float* alpha_log, const float* beta_log,
                         const float* filter12, float* y, int B, int C, int T, fac_stream_t stream);

/* losses.py:84:  out[0] (+)= scale * sum_{b,t} sqrt( mean_m (log(|a|+eps) - log(|b|+eps))^2 ),
 * a, b (B, M, T); scratch >= 1024 floats; deterministic two-stage reduction. */
int fac_logdiff_rms(const float* a, const float* b, float* out, float* scratch, int B, int M, int T,
                    float eps, float scale, int accumulate, fac_stream_t stream);

/* Backward of fac_logdiff_rms w.r.t. its SECOND operand (the estimate of losses.py:65-89 reconstruction_loss):
 * db (+)= scale * d/db sum_{b,t} sqrt( mean_m (log(|a|+eps) - log(|b|+eps))^2 ). */
int fac_logdiff_rms_bwd(const float* a, const float* b, float* db, int B, int M, int T, float eps, float scale,
                        int accumulate, fac_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Sample-rate conversion by a rational ratio: polyphase windowed-sinc filter, o = rate_in / g input samples per
 * n = rate_out / g output samples.  table (n, taps) fp32 and offs (n,) int32 come from the host (facodec_amd/dsp.py
 * resample_table): output m = k n + p reads the inputs k o + offs[p] + j, j = 0 .. taps - 1, and is
 *     y[m] = sum_j table[p][j] * x[k o + offs[p] + j]     accumulated in ascending j with one fma per tap,
 * so the order of an output's additions depends on its phase p alone.
 *
 * Row b's signal, in ABSOLUTE sample indices q (int64: a stream may run longer than 2^31 samples), is
 *     hist[b * hist_bs + (q - (q0 - n_hist))]   for q0 - n_hist <= q < q0       (carried history; NULL with n_hist = 0)
 *     x[b * x_bs + (q - q0)]                    for q0 <= q < q0 + L_b,         L_b = lens ? clamp(lens[b], 0, T) : T
 * and 0 everywhere else, below q = 0 included: nothing behind lens[b] is read.  The launch writes y[b * y_bs + i] for
 * i = 0 .. n_out - 1, the output of absolute index m = m_lo + i; it is 0 for m < 0 and for m >= ceil((q0 + L_b) n / o).
 * The offline call is n_hist = 0, q0 = 0, m_lo = 0, n_out = ceil(T n / o).
 * hist_out (or NULL; needs lens == NULL; must not overlap hist or x): hist_out[b * hist_bs + j] = the sample of absolute index
 * q0 + T - n_hist + j, j = 0 .. n_hist - 1 -- the history the next block of the stream is resampled with, written by the same
 * launch.  o, n <= 640; |q0 - m_lo o / n| + n_hist + T must fit 31 bits. */
typedef struct fac_resample_desc {
  const float* hist;
  const float* x;
  const int32_t* lens;
  float* y;
  float* hist_out;
  const float* table;
  const int32_t* offs;
  int64_t hist_bs, x_bs, y_bs;
  int64_t q0, m_lo;
  int32_t B, n_hist, T, n_out;
  int32_t o, n, taps;
} fac_resample_desc;
int fac_resample(const fac_resample_desc* d, fac_stream_t stream);
/* Which form of the kernel fac_resample launches for the descriptor (host logic only, nothing is launched):
 * 0 = coefficient table and input span in LDS, 1 = table read from global memory, span in LDS, 2 = both read from global memory
 * (a span too long for LDS: extreme ratios); -1 on error.  out4 (or NULL) = {outputs per tile, threads, LDS bytes, grid x}. */
int fac_resample_form(const fac_resample_desc* d, int32_t* out4);

/* ------------------------------------------------------------------------------------------
 * Pitch: the glue of the JDC F0 extractor (modules/JDC/model.py) and the predictor heads' targets (train.py:215-256).
 * The extractor's 3 x 3 Conv2ds run on fac_conv1d_fwd over the row-concatenated layout of the spectrogram discriminator
 * (see fac_spec_to_cat) at stride 1: every channel is one signal of rows * P floats, rows = B * (T + 1), row b * (T + 1) + t
 * holds the W valid frequency bins of frame t then zeros up to the pitch P, row t = T of every clip is all zero; the conv is
 * K = 9, K1 = 3, dilation2 = P, pad_left = P + 1, zero padding.
 *   jdc_affine_lrelu_pool  y[c, r, j] = max_{i < pool} lrelu(scale[c] * x[c, r, j * pool + i] + shift[c]), j < W_in / pool (the
 *                          floor drops trailing bins like MaxPool2d): eval BatchNorm (scale = gamma / sqrt(var + eps), shift =
 *                          beta - mean * scale, both NULL: identity) -> LeakyReLU -> MaxPool along frequency.  x (C, rows, P_in)
 *                          is a conv output: only valid columns of valid rows enter the result; y (C, rows, P_out) with
 *                          P_out * pool == P_in gets exact zeros in every gap column and separator row (row % rows_per_group ==
 *                          rows_per_group - 1).  The maximum starts from the first element.  pool = 1: no pooling.
 *   jdc_layout_in          mel (B, 1, W, T) -> the stage-0 signal (1, B * (T + 1) * P)
 *   jdc_to_time_major      stage signal (C channels of valid width W) -> LSTM input (C * W, T, BP), feature c * W + w (the
 *                          reference's permute(0, 2, 1, 3).view(-1, T, C * W)), batch padding zero; reverse: time flipped
 *   jdc_to_nchw            stage signal -> (B, C, T, W), or (B, C, W, T) with transposed != 0
 *   jdc_head               out[b, t] = |w . [h_fwd[:, t, b] | h_bwd[:, T - 1 - t, b]] + bias[0]|: h_fwd, h_bwd (H, T, BP) the two
 *                          directions' outputs (the backward one on flipped time), w (2H), out (B, T)
 *   f0_normalize           train.py:224-256, one workgroup per clip, fixed-order sums: voiced = f0 > 5; l = log2(f0) over the
 *                          voiced frames, out = (l - mean) / std (unbiased) there and -10 on unvoiced frames; any NaN / inf
 *                          result becomes -10 (one voiced frame, all voiced frames equal); mean_out (B) or NULL: the per-clip
 *                          mean of l, 0 without a voiced frame
 *   mel_log_norm           modules/commons.py:176-181 with its defaults: out[b, t] = log(sqrt(sum_m exp(4 mel[b, m, t] - 4)^2))
 * ---------------------------------------------------------------------------------------- */
int fac_jdc_affine_lrelu_pool(const float* x, const float* scale, const float* shift, float* y, int C, int rows,
                              int rows_per_group, int W_in, int P_in, int pool, int P_out, float slope, fac_stream_t stream);
int fac_jdc_layout_in(const float* mel, float* out, int B, int W, int T, int P, fac_stream_t stream);
int fac_jdc_to_time_major(const float* x, float* xT, int B, int C, int T, int W, int P, int BP, int reverse, fac_stream_t stream);
int fac_jdc_to_nchw(const float* x, float* out, int B, int C, int T, int W, int P, int transposed, fac_stream_t stream);
int fac_jdc_head(const float* h_fwd, const float* h_bwd, const float* w, const float* bias, float* out, int B, int T, int H, int BP,
                 fac_stream_t stream);
int fac_f0_normalize(const float* f0, float* out, float* mean_out, int B, int T, fac_stream_t stream);
int fac_mel_log_norm(const float* mel, float* out, int B, int n_mels, int T, fac_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Loudness: the ITU-R BS.1770-4 meter for mono signals and the level normalisation built on it.
 *
 * Rate fs, S = fs / 10 samples per 100 ms sub-block (fs % 10 == 0).  K-weighting is two biquads designed on the host in fp64
 * (facodec_amd/dsp.py k_weighting), a0 = 1:
 *   stage 1, shelf:      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196,
 *                        K = tan(pi f0 / fs), Vh = 10^(G/20), Vb = Vh^0.4996667741545416, d = 1 + K/Q + K^2,
 *                        b = [(Vh + Vb K/Q + K^2)/d, 2 (K^2 - Vh)/d, (Vh - Vb K/Q + K^2)/d], a = [1, 2 (K^2 - 1)/d, (1 - K/Q + K^2)/d]
 *   stage 2, high-pass:  f0 = 38.13547087602444, Q = 0.5003270373238773, same K, d;  b = [1, -2, 1] (not normalised, as in the
 *                        standard), a = [1, 2 (K^2 - 1)/d, (1 - K/Q + K^2)/d]
 * Energies: y = the clip's own len_b samples through both biquads from zero state (or from the carried state); nothing behind
 * the clip's end is filtered.  e[b, j] = sum of y^2 over sub-block j, j < ceil(len_b / S), the last one possibly partial; fp64.
 * Gating: block j = sub-blocks j .. j + 3, whole blocks only: n_blocks = (len_b - 4 S) / S + 1; a clip with 0 < len_b < 4 S counts
 * as zero-padded to one block.  z_j = (e_j + .. + e_{j+3}) / (4 S), l_j = -0.691 + 10 log10 z_j.  Absolute gate l_j > -70;
 * Gr = -0.691 + 10 log10(mean of z over the absolute-gated blocks) - 10; L = -0.691 + 10 log10(mean of z over the blocks with
 * l_j > -70 and l_j > Gr).  No block passes, or len_b = 0: L = -70.  L is never below -70.
 * Normalising to `target`: g = 10^((target - L) / 20); L <= -70 (silence): g = 1; peak guard: g * max|x| > 1 -> g = 1 / max|x|;
 * y = x * g in fp32 with g rounded once to fp32.
 *
 * fac_kweight_energy.  The two biquads in transposed direct form II are one linear system on the state (s1, s2, t1, t2):
 *     y1 = b0 x + s1;  s1' = (b1 x + s2) - a1 y1;  s2' = b2 x - a2 y1;     (stage 1: b = coef[0..2], a1, a2 = coef[3..4])
 *     y  = c0 y1 + t1; t1' = (c1 y1 + t2) - d1 y;  t2' = c2 y1 - d2 y      (stage 2: c = coef[5..7], d1, d2 = coef[8..9])
 * (every product-and-add one fma)
 * so the time axis is cut into chunks of FAC_LOUDNESS_CHUNK samples, 64 chunks to a workgroup: (1) every chunk runs from zero
 * state and the 64 end states of a workgroup are combined by a fixed 6-step scan with M^(chunk 2^k), k = 0 .. 5; (2) a short
 * serial scan hands states across workgroups with M^(64 chunk); (3) every chunk re-runs from its true state and sums squares.
 * pw[k] = M^(chunk 2^k), k = 0 .. 6, row-major 4 x 4 on (s1, s2, t1, t2), fp64, from the host.  Everything is fp64 and in a
 * fixed order: results are bit-identical run to run.  The filtered signal is never written to memory.
 *   x (B rows of T fp32 samples, row pitch x_bs), lens (B) int32 or NULL (clamped to [0, T]);
 *   offset: the position of the call's first sample within its sub-block, 0 <= offset < S; the call covers the
 *           n_sub = ceil((offset + T) / S) sub-blocks e[b * e_bs + j], j < n_sub, all of which are written (0 behind len_b);
 *           with offset > 0, e[b, 0] is read and the call's share is added to it (a stream's sub-block grid continues);
 *   state_in / state_out (B, 4) fp64 or NULL: the state before the first and after the last of the T samples (they may be the
 *           same buffer; state_out needs lens == NULL);
 *   peak (B) fp32 or NULL: max |x| over the row's samples; with peak_accumulate != 0 the maximum of that and what it held;
 *   ws: fac_kweight_ws_bytes(B, T) bytes of device scratch, 8-byte aligned.
 * S >= FAC_LOUDNESS_CHUNK (fs >= 2560), T <= 2^30, B <= 65535.  T == 0 launches nothing.
 *
 * fac_loudness_gate: one workgroup per row, fixed order.  e (B rows of pitch e_bs), n_samples = the samples every row holds
 * (int64: a stream), lens (B) int32 or NULL (clamped to [0, n_samples]).  last_n == 0: the two-gate integrated loudness above;
 * last_n > 0: -0.691 + 10 log10(sum of the row's last last_n sub-blocks / (last_n S)), ungated and not below -70 (momentary:
 * 4, short-term: 30; sub-blocks before the signal's start count as zero).  peaks (B, n_peaks) fp32 of pitch n_peaks or NULL:
 * peak_out[b] = their maximum.  L_out (B) fp64.
 *
 * fac_loudness_gain: g[b] from (L[b], target, peak[b]) by the rule above, on the device, then y[b, t] = x[b, t] * g[b] for
 * t < len_b and 0 behind, t < T; g_out (B) fp32 or NULL.  target_rows (B) fp64 or NULL replaces `target` per row, and a NaN
 * there means g = 1 (a row to leave alone).  guard == 0 skips the peak guard (peak may then be NULL).  y may be x.
 * ---------------------------------------------------------------------------------------- */
#define FAC_LOUDNESS_CHUNK 256
typedef struct fac_kweight_desc {
  const float* x;
  const int32_t* lens;
  double* e;
  const double* state_in;
  double* state_out;
  float* peak;
  void* ws;
  int64_t x_bs, e_bs;
  int32_t B, T, S, offset, peak_accumulate, reserved;
  double coef[10];
  double pw[7][16];
} fac_kweight_desc;
int64_t fac_kweight_ws_bytes(int B, int T);
int fac_kweight_energy(const fac_kweight_desc* d, fac_stream_t stream);
/* which = 0: samples per chunk (FAC_LOUDNESS_CHUNK), 1: chunks per workgroup. */
int fac_loudness_chunk(int which);
int fac_loudness_gate(const double* e, int64_t e_bs, const int32_t* lens, int64_t n_samples, int S, int last_n, const float* peaks,
                      int n_peaks, double* L_out, float* peak_out, int B, fac_stream_t stream);
int fac_loudness_gain(const float* x, int64_t x_bs, const int32_t* lens, const double* L, const float* peak, const double* target_rows,
                      double target, int guard, float* y, int64_t y_bs, float* g_out, int B, int T, fac_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Slots of a running streaming session (csrc/stream_pool.hip).  This comment is the normative layout.
 *
 * A session over B streams keeps every per-stream piece of state in static, batch-indexed fp32 buffers.  A SEGMENT describes
 * where one such buffer keeps the state of slot b: `rows` runs of `row_len` contiguous floats, `row_stride` elements apart,
 * the first at
 *     base + (b >> 5) * slot_hi + (b & 31) * slot_lo                                     (all strides in elements)
 *   left-context buffer (B, C, W), contiguous       rows 1,   row_len C W, row_stride 0,   slot_lo C W, slot_hi 32 C W
 *   LSTM state (3, H, BP) = [c | h ping | h pong] (fac_lstm_layer_fwd):
 *     c plane (H, BP)                               rows H,   row_len 1,   row_stride BP,  slot_lo 1,   slot_hi 32
 *     each h plane, MFMA-B fragment order
 *       [BP/32][H/8][2][32 batch][4]                rows H/4, row_len 4,   row_stride 128, slot_lo 4,   slot_hi 32 H
 *   (both h planes are copied: which one is live depends on the parity of the steps taken).
 * `elems` = rows * row_len.  The work of one copy is cut into TILES of up to FAC_SLOT_TILE elements of one segment's per-slot
 * element range: tile = {segment index, first element}, first element a multiple of FAC_SLOT_TILE.  Segment table and tile list
 * live on the device and are built once per pool (ops.SlotTable checks every run against its tensor's extent); the entry
 * trusts them.
 *
 * fac_slot_copy: for every destination d of dst[0 .. n_dst) (HOST array) and every segment, slot d's runs = slot src's runs,
 * in one launch of n_tiles x n_dst workgroups.  A run is moved with 16-byte loads and stores when row_len and (for rows > 1)
 * row_stride are multiples of 4 and both slots' first addresses are 16-byte aligned, with 4-byte accesses otherwise (decided
 * per segment and destination, uniform over the workgroup).  Plain vector stores, no atomics; nothing outside the destination
 * slots' runs is written.  Refused before any launch: a NULL table or tile list, n_seg or n_tiles < 1, B < 1, n_dst outside
 * 1 .. FAC_SLOT_MAX_DST, a slot outside [0, B), src among the destinations, a destination named twice.
 *
 * fac_rows_pick: dst[r, 0 .. row_words) = map[r] in [0, n_src) ? src[map[r] * src_stride + 0 .. row_words) : 0 for r < n_dst,
 * over 32-bit words (an int64 row of k values is 2 k words).  dst is dense (n_dst, row_words); map: n_dst int32 on the device.
 * Destination driven: every word of dst is written exactly once, the rows without a source by stores alone; src is only read.
 * 16-byte accesses when row_words and src_stride are multiples of 4 and both pointers are 16-byte aligned.  Refused: NULL
 * pointers, n_dst, n_src or row_words < 1, src_stride < row_words.
 * ---------------------------------------------------------------------------------------- */
#define FAC_SLOT_MAX_DST 8
#define FAC_SLOT_TILE 4096
typedef struct fac_slot_seg {
  float* base;
  int64_t slot_hi;
  int32_t rows, row_stride, row_len, slot_lo;
  int32_t elems, reserved;
} fac_slot_seg;
int fac_slot_copy(const fac_slot_seg* segs, int n_seg, const int32_t* tiles, int n_tiles, int B, int src, const int32_t* dst,
                  int n_dst, fac_stream_t stream);
int fac_rows_pick(const void* src, int64_t src_stride, void* dst, const int32_t* map, int n_dst, int n_src, int row_words,
                  fac_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Objective scores of a reconstruction (csrc/metrics.hip): SI-SDR, STOI (Taal et al. 2011) and ESTOI (Jensen &
 * Taal 2016).  This comment is the normative definition.
 *
 * Inputs: a reference x and an estimate y, B rows of T fp32 samples (row pitches x_bs, y_bs), lens (B) int32 on the device or
 * NULL (clamped to [0, T]): row b is its first len_b samples and nothing behind them is read as signal.  All results are fp64.
 *
 * SI-SDR (dac/nn/loss.py:91-130 with scaling = True, zero_mean = True, sign flipped: higher is better), eps = 1e-8:
 *     r = x - mean(x);  e = y - mean(y);  a = (sum e r + eps) / (sum r r + eps);  s = a r;  n = e - s;
 *     SI-SDR = 10 log10(sum s^2 / sum n^2 + eps) dB.
 * Three passes over the row (the means; sum e r and sum r r on the centred samples; sum s^2 and sum n^2 with n formed sample by
 * sample -- never expanded from sums, which cancels when y ~ x).  Whatever the formula gives in IEEE fp64 is the answer:
 * identical rows +inf, an empty or all-zero pair NaN, a zero reference with a non-zero estimate -80.  Every pass sums chunks of
 * FAC_SI_SDR_CHUNK samples (chunk c = samples [c chunk, (c + 1) chunk) of the row, whatever T is) in a fixed order and the
 * chunks of a row in a fixed order: a row scores the same bits alone as in any batch.
 *   fac_si_sdr: out (B) fp64; ws = fac_si_sdr_ws_bytes(B, T) bytes of device scratch, 8-byte aligned.  T <= 2^30, B <= 65535.
 *
 * STOI / ESTOI, at FS = 10000 Hz (the caller resamples): frame length 256, hop 128, NFFT 512, 15 third-octave bands from 150 Hz,
 * N = 30 frames per segment, BETA = -15 dB, dynamic range 40 dB, EPS = 2.220446049250313e-16, window
 * w[n] = 0.5 - 0.5 cos(2 pi (n + 1) / 257), n = 0 .. 255.
 *  1. Windowed frames f_m = w . x[128 m : 128 m + 256], m = 0 .. M - 1, M = (len - 256) / 128 + 1 (0 for len < 256).
 *  2. E_m = 20 log10(||f_m||_2 + EPS) from the REFERENCE only; frame m is kept iff max_m E - 40 - E_m < 0 (an all-silent
 *     reference keeps every frame).  Kept frames k_0 < .. < k_{K-1}.  The compacted signals are the overlap-add at hop 128 of
 *     the kept windowed frames of x and of y, 128 (K - 1) + 256 samples.
 *  3. The compacted signals are framed again (same window, length, hop: exactly K frames), zero-padded to 512; |X[k]|^2 of the
 *     one-sided DFT.  Frame j of a compacted signal is never stored: its first half is f_{k_j}[n] + f_{k_{j-1}}[n + 128], its
 *     second half f_{k_j}[n] + f_{k_{j+1}}[n - 128], the neighbour absent at the ends.
 *  4. Bands j = 0 .. 14: Tb[j, m] = sqrt(sum_{k = lo_j}^{hi_j - 1} |X[k, m]|^2), (lo, hi) = (7,9) (9,11) (11,14) (14,17) (17,22)
 *     (22,27) (27,34) (34,43) (43,55) (55,69) (69,87) (87,109) (109,138) (138,174) (174,219): the bins nearest
 *     150 2^(j/3) 2^(-+1/6) Hz on the grid k 10000 / 512.
 *  5. Segments s = 0 .. K - 30: X_s = Tx[:, s : s + 30], Y_s = Ty[:, s : s + 30] (15 x 30).  K < 30: no segment, both scores NaN.
 *  6. STOI, per band row of a segment: alpha = ||x|| / (||y|| + EPS); y' = min(alpha y, x (1 + 10^(15/20))); both vectors minus
 *     their mean, over (their norm + EPS); c = sum x^ y'^.  STOI = the mean of c over all bands and segments.
 *  7. ESTOI, per segment: rows of X_s and Y_s minus their mean over time, over (norm + EPS); then columns minus their mean over
 *     bands, over (norm + EPS); d_s = (1 / 30) sum_{j, m} X^ Y^.  ESTOI = the mean of d_s over the segments.
 * Everything is fp64 (the 512-point transform included), every reduction in a fixed order without atomics; a row scores the
 * same bits alone as in any batch.
 *
 * The three launches share one descriptor and run in this order on one stream; nothing is read back between them.
 *   fac_stoi_select  E_m per frame, then per row the maximum, the keep flags and an exclusive scan in blocks of out[3] frames
 *                    with a carried offset: kept_idx (B, M_max) int32 of pitch M_max (the first n_kept[b] entries of a row are
 *                    the kept frames, the others -1), n_frames, n_kept (B) int32.
 *   fac_stoi_bands   Tb (B, 2, 15, M_max) fp64 in ws for x and y from one launch; frames j >= n_kept[b] are not computed.
 *   fac_stoi_score   per (row, segment) sum_j c and d_s, then per row the fixed-order means: stoi, estoi (B) fp64, n_segments (B)
 *                    int32 (max(n_kept - 29, 0)).
 *   fac_stoi_geometry(T, out6), host only: out6 = {M_max, ws bytes per row, frames per workgroup of the energy launch, frames
 *                    per block of the scan, frames per workgroup of fac_stoi_bands, segments per workgroup of fac_stoi_score};
 *                    ws holds, in this order, E (B, M_max), Tb (B, 2, 15, M_max) and the segment sums (B, 2, max(M_max - 29, 0)),
 *                    all fp64: out6[1] * B bytes, 8-byte aligned.  -1 for T < 0 or T > 2^28.
 * Refused before any launch: a NULL descriptor or pointer, B outside 1 .. 65535, T outside 0 .. 2^28, ws_bytes below
 * out6[1] * B, ws not 8-byte aligned.
 * ---------------------------------------------------------------------------------------- */
#define FAC_SI_SDR_CHUNK 4096
int64_t fac_si_sdr_ws_bytes(int B, int T);
int fac_si_sdr(const float* x, int64_t x_bs, const float* y, int64_t y_bs, const int32_t* lens, double* out, void* ws, int64_t ws_bytes,
               int B, int T, fac_stream_t stream);
typedef struct fac_stoi_desc {
  const float* x;
  const float* y;
  const int32_t* lens;
  int32_t* kept_idx;
  int32_t* n_frames;
  int32_t* n_kept;
  int32_t* n_segments;
  double* stoi;
  double* estoi;
  void* ws;
  int64_t x_bs, y_bs, ws_bytes;
  int32_t B, T;
} fac_stoi_desc;
int fac_stoi_geometry(int T, int64_t* out6);
int fac_stoi_select(const fac_stoi_desc* d, fac_stream_t stream);
int fac_stoi_bands(const fac_stoi_desc* d, fac_stream_t stream);
int fac_stoi_score(const fac_stoi_desc* d, fac_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Surviving packet loss (csrc/vq_decode.hip, csrc/plc.hip).  This comment is the normative definition.
 *
 * fac_vq_decode_masked: fac_vq_decode with quantizer counts per row and frame.  n_use[b*n_use_bs + t*n_use_ts + r] (int32 on
 * the device) is the number of LEADING quantizers of RVQ r that contribute to frame (b, t), clamped to [0, base.n_q[r]].
 *   RULE: for every (b, t), outs[b, :, t] and the optional z[r][b, :, t] equal, bit for bit, what fac_vq_decode gives for
 *   that frame when called with n_q = n_use[b, t, :] (and the first n_q[r] code rows and weight sets of each RVQ).
 * The per-RVQ chain is 0 + z_q_0 + z_q_1 + ..., then (z_p + z_c) + z_r, then the LayerNorm; a skipped quantizer's add is not
 * executed (it does not add a zero).  Codes of skipped quantizers are ignored: they may hold anything (they are still loaded,
 * under the clamp of fac_vq_decode, so they must be addressable).  n_use == NULL is fac_vq_decode.  Same layout as
 * fac_vq_decode: one workgroup per (row, tile of <= 16 frames); the tile's counts are read once into LDS and the predicate is
 * per (quantizer, frame), uniform over the channels.  Refused before any launch: what fac_vq_decode refuses, and a non-NULL
 * n_use whose strides cannot address (B, T, 3): n_use_bs <= 0 with B > 1, or n_use_ts <= 0 with T > 1.
 *
 * fac_plc_select: per-row substitution of one push of k <= FAC_PLC_MAX_FRAMES frames, from device-resident state
 *   last_codes (B, Q) int64   the codes last played, quantizers in RVQ order, Q = n_q[0] + n_q[1] + n_q[2]
 *   last_n (B, 3) int32       the quantizer counts they were played with
 *   g (B) fp32                the gain at the end of the last emitted sample (initially 1)
 *   run (B) int32             concealed frames in a row (initially 0)
 * and status (B) int32 on the device: 0 PRIMARY, 1 REDUNDANT, 2 LOST; any other value counts as LOST, and so does REDUNDANT
 * when there is no redundant layer (n_red all 0).  Per row b, for every frame f < k:
 *   PRIMARY    dst = prim;  n_use[b, f, :] = n_q;  then last_codes = the codes of frame k - 1, last_n = n_q.
 *   REDUNDANT  quantizer i of RVQ r: dst = red when i < n_red[r], else 0 (which the mask ignores);  n_use[b, f, :] = n_red;
 *              then last_codes of the quantizers inside n_red = their codes of frame k - 1 (the others keep theirs), last_n = n_red.
 *   LOST       dst = last_codes for every frame;  n_use[b, f, :] = last_n;  last_codes and last_n unchanged.
 * Gain, fp32, round-to-nearest, in exactly this order:  ramp[b, 0] = g;  per frame f = 0 .. k - 1
 *   LOST       run += 1;  target = run <= hold ? g : max(0, g - 1.0f / (float)fade)
 *   otherwise  run = 0;   target = min(1, g + 1.0f / (float)recover)
 *   ramp[b, f + 1] = g = target.
 * dst may be the prim buffers themselves.  One thread per (row, quantizer) walks the k frames, one thread per row does the
 * counts and the gain: every word is written by exactly one thread, plain vector stores, no atomics, nothing read that
 * another thread of the launch writes.  n_use is (B, k, 3) with strides n_use_bs / n_use_ts, ramp is dense (B, k + 1).
 * Refused before any launch: a NULL descriptor, status or state pointer, n_use or ramp; B < 1; k outside
 * 1 .. FAC_PLC_MAX_FRAMES; Q outside 1 .. FAC_VQ_DECODE_MAX_Q or a negative count; n_red[r] > n_q[r]; a NULL prim or dst with
 * n_q[r] > 0; a NULL red with n_red[r] > 0; hold < 0, fade < 1, recover < 1; n_use strides that cannot address (B, k, 3).
 *
 * fac_plc_gain: y[b, f * frame + n] = x[b, f * frame + n] * gain,  gain = ramp[b, f] + (ramp[b, f + 1] - ramp[b, f]) * t,
 * t = (float)(n + 1) / (float)frame (frame = 300 for the shipped model), every operation a separate fp32 round-to-nearest
 * (no fused multiply-add).  Stateless, one thread per sample, y may be x.  A row whose ramp is 1 everywhere has gain == 1.0f
 * exactly: y is x bit for bit.  x and y are B rows of k * frame samples with pitches x_bs, y_bs.  Refused: NULL pointers,
 * B, k or frame < 1, a pitch below k * frame, B * k * frame >= 2^31.
 * ---------------------------------------------------------------------------------------- */
#define FAC_PLC_MAX_FRAMES 16
#define FAC_PLC_PRIMARY 0
#define FAC_PLC_REDUNDANT 1
#define FAC_PLC_LOST 2
typedef struct fac_vq_decode_masked_desc {
  fac_vq_decode_desc base;
  const int32_t* n_use;     /* (B, T, 3) counts, or NULL (== fac_vq_decode) */
  int64_t n_use_bs, n_use_ts;
} fac_vq_decode_masked_desc;
int fac_vq_decode_masked(const fac_vq_decode_masked_desc* d, fac_stream_t stream);

typedef struct fac_plc_select_desc {
  const int64_t* prim[3];   /* primary codes (B, n_q[r], k): prim[r][b*prim_bs[r] + i*prim_qs[r] + f] */
  int64_t prim_bs[3], prim_qs[3];
  const int64_t* red[3];    /* redundant codes (B, n_red[r], k), NULL when n_red[r] == 0 */
  int64_t red_bs[3], red_qs[3];
  int64_t* dst[3];          /* written: (B, n_q[r], k), may be prim */
  int64_t dst_bs[3], dst_qs[3];
  int32_t n_q[3], n_red[3];
  const int32_t* status;    /* (B) */
  int64_t* last_codes;      /* (B, Q) state */
  int32_t* last_n;          /* (B, 3) state */
  float* g;                 /* (B) state */
  int32_t* run;             /* (B) state */
  int32_t* n_use;           /* written: (B, k, 3) */
  int64_t n_use_bs, n_use_ts;
  float* ramp;              /* written: (B, k + 1) dense */
  int32_t B, k, hold, fade, recover, reserved;
} fac_plc_select_desc;
int fac_plc_select(const fac_plc_select_desc* d, fac_stream_t stream);
int fac_plc_gain(const float* x, int64_t x_bs, float* y, int64_t y_bs, const float* ramp, int B, int k, int frame,
                 fac_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Voice activity, silent-push suppression, comfort frames (csrc/vad.hip).  This comment is the normative
 * definition.  Every operation below is an IEEE fp64 operation with one round-to-nearest each; nothing is fused.
 *
 * fac_vad_energy: per row b the signal is the virtual concatenation [carry | block]:
 *   carry_in (B, frame) fp32, dense   element 0 is the sample BEFORE the first unprocessed one (0 at the start of a signal),
 *                                      elements 1 .. carry_n the unprocessed tail of earlier calls; NULL: carry_n = 0 and that
 *                                      sample is 0 (the offline call)
 *   x (B, k) fp32, pitch x_bs         this call's samples
 * Unprocessed sample s (s = 0 is the first) belongs to frame s / frame of this call.  n_whole = (carry_n + k) / frame whole
 * frames are processed, and the partial one behind them when is_final != 0 and (carry_n + k) % frame != 0.  For frame i:
 *   d[n] = (double)v[n] - 0.97 * (double)v[n - 1]                    v[-1] of frame 0 is the sample before (carry element 0)
 *   lane l of 64 adds d[n] * d[n] for n = l, l + 64, l + 128, ... < frame (only samples that exist) in increasing n, starting
 *   from 0.0;  then for dist = 32, 16, 8, 4, 2, 1 every lane replaces its sum by  own + sum of lane (l XOR dist);  E = lane 0.
 *   e[b * e_bs + (f0 + i) % R] = E.          f0: the global index of this call's first frame; a plain (B, F) array is R >= F, f0 = 0.
 * lens (B) int32, NULL or (only without carry buffers) the rows' lengths in samples: samples at and behind lens[b] do not
 * exist, frames at or past ceil(lens[b] / frame) get E = 0.
 * carry_out (B, frame), NULL or a buffer OTHER than carry_in: written with the carry of the next call, element 0 the last
 * processed sample (or carry_in's element 0 when no whole frame was processed), then the (carry_n + k) % frame unprocessed
 * ones; the host alternates two buffers, so no word is read by one thread and written by another in one launch.
 * Refused before any launch: a NULL descriptor, x or e; B outside 1 .. 65535; frame outside 1 .. FAC_VAD_MAX_FRAME; k < 1;
 * carry_n outside 0 .. frame - 1, or > 0 without carry_in; carry_out == carry_in; lens with a carry buffer; x_bs < k or
 * e_bs < R with B > 1; f0 < 0; R below the frames of the call.
 *
 * fac_vad_decide: flags for the n_new frames f0 .. f0 + n_new - 1 from the energy ring e (B, R) (frame g at column g % R):
 *   N[f]      = min E[g] over g = max(0, f - W + 1) .. f
 *   raw[f]    = E[f] > thr_abs  &&  E[f] > margin * N[f]
 *   active[f] = raw[g] for any g = max(0, f - H) .. f;  with lens, frames at or past ceil(lens[b] / frame) are 0.
 * All windows are finite, there is no recurrence: a flag depends on the W + H energies up to its frame and nothing older.
 * flags (NULL or uint8, pitch flags_bs): flags[b * flags_bs + i] = active[f0 + i];  ring (NULL or uint8 (B, R), pitch ring_bs):
 * ring[b * ring_bs + (f0 + i) % R] = the same.  One workgroup per (row, 256 frames): energies of the tile and its W - 1 + H
 * older neighbours in LDS, raw of the tile and its H older neighbours in LDS, barrier, flags.
 * Refused before any launch: a NULL descriptor or e; flags and ring both NULL; B outside 1 .. 65535; n_new < 1; W outside
 * 1 .. FAC_VAD_MAX_WINDOW; H outside 0 .. FAC_VAD_MAX_WINDOW; margin <= 1; thr_abs < 0; f0 < 0; frame outside
 * 1 .. FAC_VAD_MAX_FRAME; R < min(f0 + n_new, W + H + n_new) (a ring that has not wrapped yet holds every frame); pitches
 * below R (e, ring) or n_new (flags) with B > 1.
 *
 * fac_vad_take: out[b * out_bs + j] = ring[b * ring_bs + (f0 + j) % R] for j < k: the gather behind VoiceActivity.take(out=).
 *
 * fac_sid_apply: the receiver's comfort frames.  Device state: sid_codes (B, Q, FAC_PLC_MAX_FRAMES) int64, the codes of the
 * last silence descriptor of every row.  mode (B) int32 on the device is kind | phase << 8 | sid_k << 16:
 *   FAC_SID_PASS   the row is not touched (and so is a row of any other kind value)
 *   FAC_SID_STORE  sid_codes[b, q, f] = dst[b, q, f] for f < k
 *   FAC_SID_FILL   dst[b, q, f] = sid_codes[b, q, (phase + f) % sid_k] for f < k;  sid_k outside 1 .. FAC_PLC_MAX_FRAMES: not touched
 * dst are the three code buffers (B, n_q[r], k) of fac_plc_select, q runs over the quantizers in RVQ order.  phase and sid_k
 * are the host's (they are deterministic).  One thread per (row, quantizer): every word has one writer.  Refused before any
 * launch: a NULL descriptor, mode or sid_codes; B < 1; k outside 1 .. FAC_PLC_MAX_FRAMES; Q outside 1 .. FAC_VQ_DECODE_MAX_Q
 * or a negative count; a NULL dst with n_q[r] > 0; strides that cannot address (B, n_q[r], k).
 * ---------------------------------------------------------------------------------------- */
#define FAC_VAD_MAX_FRAME 4096
#define FAC_VAD_MAX_WINDOW 2048
#define FAC_SID_PASS 0
#define FAC_SID_STORE 1
#define FAC_SID_FILL 2
typedef struct fac_vad_energy_desc {
  const float* carry_in;    /* (B, frame) or NULL */
  float* carry_out;         /* (B, frame) or NULL, never carry_in */
  const float* x;           /* (B, k), pitch x_bs */
  const int32_t* lens;      /* (B) or NULL */
  double* e;                /* written: (B, R), pitch e_bs */
  int64_t x_bs, e_bs, f0;
  int32_t B, k, frame, carry_n, is_final, R;
} fac_vad_energy_desc;
int fac_vad_energy(const fac_vad_energy_desc* d, fac_stream_t stream);

typedef struct fac_vad_decide_desc {
  const double* e;          /* (B, R), pitch e_bs */
  const int32_t* lens;      /* (B) or NULL */
  uint8_t* flags;           /* written: (B, n_new), pitch flags_bs; or NULL */
  uint8_t* ring;            /* written: (B, R), pitch ring_bs; or NULL */
  int64_t e_bs, flags_bs, ring_bs, f0;
  double margin, thr_abs;
  int32_t B, n_new, R, W, H, frame;
} fac_vad_decide_desc;
int fac_vad_decide(const fac_vad_decide_desc* d, fac_stream_t stream);
int fac_vad_take(const uint8_t* ring, int64_t ring_bs, int R, int64_t f0, int k, uint8_t* out, int64_t out_bs, int B,
                 fac_stream_t stream);

typedef struct fac_sid_apply_desc {
  int64_t* dst[3];          /* (B, n_q[r], k): dst[r][b*dst_bs[r] + i*dst_qs[r] + f] */
  int64_t dst_bs[3], dst_qs[3];
  int32_t n_q[3];
  int32_t B;
  const int32_t* mode;      /* (B) */
  int64_t* sid_codes;       /* (B, Q, FAC_PLC_MAX_FRAMES) state */
  int32_t k, reserved;
} fac_sid_apply_desc;
int fac_sid_apply(const fac_sid_apply_desc* d, fac_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Level control (csrc/agc.hip): a causal automatic gain control on the sub-block energies of fac_kweight_energy, a
 * look-ahead peak limiter behind it, and a true-peak meter.  This comment is the normative definition.  Finite windows, no
 * recurrence: a gain depends on the W energies up to its sub-block, an output sample on 2 LA + 1 input samples and two gains.
 * Unless said otherwise every operation below is one IEEE fp64 operation with one round-to-nearest; nothing is fused.
 *
 * fac_agc_gains: S = fs / 10 samples per sub-block; e (B, R) fp64 holds the energy of sub-block j at column j % R (a plain
 * (B, n) array is R >= n, j0 = 0).  The gains of the n_new sub-blocks j = j0 .. j0 + n_new - 1, each known once its sub-block
 * is complete.  With js = j_start[b] (0 when j_start is NULL), the first sub-block of the row's current stream:
 *   lo = max(js, j - W + 1);   the gating blocks inside the window are k = lo .. j - 3, block k = sub-blocks k .. k + 3
 *   z_k = (((e_k + e_{k+1}) + e_{k+2}) + e_{k+3}) / (4 S);    l_k = -0.691 + 10 log10(z_k), -inf for z_k <= 0
 *   pass 1, k ascending, both sums from 0.0:  l_k > -70:  A += z_k, nA += 1.     nA = 0: L_j = -70.
 *   Gr = -0.691 + 10 log10(A / nA) - 10
 *   pass 2, k ascending, from 0.0:  l_k > -70 and l_k > Gr:  Z += z_k, nZ += 1
 *   L_j = max(-70, -0.691 + 10 log10(Z / nZ));   L_j = -70 when nZ = 0, when the window holds fewer than 4 sub-blocks (j - lo < 3)
 *   G_j = 0 for L_j <= -70, else min(max(target_db - L_j, -max_cut_db), max_boost_db);      g_j = pow(10, G_j / 20)
 * log10 and pow are the device math library's (correct to an ulp or two, not single roundings); everything else is.
 * lens (B) int32 or NULL: row b holds lens[b] samples, sub-block j is complete when (j + 1) S <= lens[b].  A sub-block that is
 * not complete, or lies before js, produces no gain: G = 0, g = 1 are stored.  G, g (either may be NULL, not both) fp64 (B, R) of
 * pitch g_bs, column j % R.  One workgroup of 64 threads per (row, 64 sub-blocks), the tile's energies and its W - 1 older
 * neighbours in LDS, one thread per gain.
 * Refused before any launch: a NULL descriptor or e; G and g both NULL; B outside 1 .. 65535; n_new < 1; W outside
 * 4 .. FAC_AGC_MAX_WINDOW; S < 1; j0 < 0; max_boost_db or max_cut_db negative or not finite, target_db not finite;
 * R < min(j0 + n_new, W + n_new - 1); e_bs or g_bs below R with B > 1.
 *
 * fac_agc_apply: per row the signal is [carry | block]: the block's sample i has the absolute index n = n0 + i, lies in
 * sub-block j = n / S at position u = n % S, and exists for i < k_b = lens ? clamp(lens[b], 0, k) : k.
 *   a(n) = g_{j-2} + (g_{j-1} - g_{j-2}) * ((double)(u + 1) / (double)S)      g_i = 1 for i < js (js >= 0): only gains of completed
 *   v[n] = (double)x[n] * a(n)                                               sub-blocks are used, and the gain is continuous
 *   v[n] = 0 for samples that do not exist (behind k_b) and before the stream's start; nothing at or behind lens[b] is read
 * g (B, R) fp64 of pitch g_bs, g_i at column i % R.  The limiter, C = ceiling (linear, fp64, from the host), LA = look-ahead:
 *   c[n] = |v[n]| > C ? C / |v[n]| : 1
 *   p[k] = min c[k - LA .. k]                                                (exact in any order)
 *   s[m] = min( (p[m-LA+1] + p[m-LA+2] + .. + p[m]) / (double)LA, c[m-LA] )   the sum left to right, starting from p[m-LA+1]
 *   y[m] = (float)( v[m-LA] * s[m] )                                         one fp64 product, one rounding to fp32
 * Every p in the mean contains c[m-LA], so |y[m]| <= C up to the roundings of the quotient, the mean and the product.  Where no
 * |v| > C lies in m - 2 LA + 1 .. m, s[m] is exactly 1 and y[m] = (float)v[m-LA].  The output runs LA samples behind the input:
 * the call writes y[b * y_bs + i] = y[n0 + i], i < n_out, k <= n_out <= k + LA (n_out = k for a block of a stream, k + LA where
 * the signal ends: row b then holds k_b + LA samples and zeros behind; k = 0, n_out = LA is the flush of a stream, x may be
 * NULL).
 *   carry_in (B, 2 LA) fp64, dense: v[n0 - 2 LA .. n0 - 1]; NULL: zeros (the start of a signal)
 *   carry_out (B, 2 LA), NULL or a buffer OTHER than carry_in: v[n0 + k - 2 LA .. n0 + k - 1], written by one extra workgroup per
 *   row of the same launch; the host alternates two buffers, so no word is read and written in one launch.
 * One workgroup of 256 threads per (row, 1024 outputs): v and c of the tile and its 2 LA older neighbours and p in LDS; a tile
 * none of whose c is below 1 skips the limiter (the same bits).
 * Refused before any launch: a NULL descriptor, g or y; x NULL with k > 0; B outside 1 .. 65535; k outside 0 .. 2^30; n_out
 * outside max(k, 1) .. k + LA; S outside 1 .. 2^30; R outside 1 .. 2^28; LA outside 1 .. FAC_AGC_MAX_LOOKAHEAD; ceiling not in (0, inf); n0 < 0; carry_out ==
 * carry_in; lens with a carry buffer; x_bs < k, y_bs < n_out or g_bs < R with B > 1; R below the gains the block reaches
 * (R >= min(jl, jl - jf + 2), jf and jl the sub-blocks of the block's first and last sample: g of jf - 2 .. jl - 1 in different
 * columns; that the ring still holds them is the business of whoever writes it).
 *
 * fac_true_peak: peak[b] = max |y| over the outputs of fac_resample for the same descriptor (offline form: hist, hist_out and y
 * NULL, n_hist = 0, q0 = 0, m_lo = 0, n_out = ceil(T n / o)), without writing y: every output is the same chain of fp32 fmas
 * in ascending tap order, so the result equals the maximum over fac_resample's output bit for bit.  The maximum itself is
 * exact in any order.  ws: fac_true_peak_ws_bytes(B, n_out) bytes of device scratch (one partial maximum per row and tile).
 * ---------------------------------------------------------------------------------------- */
enum { FAC_AGC_MAX_WINDOW = 1024, FAC_AGC_MAX_LOOKAHEAD = 1024 };
typedef struct fac_agc_gains_desc {
  const double* e;          /* (B, R), pitch e_bs */
  const int32_t* lens;      /* (B) or NULL */
  const int64_t* j_start;   /* (B) or NULL */
  double* G;                /* written: (B, R) dB, pitch g_bs; or NULL */
  double* g;                /* written: (B, R) linear, pitch g_bs; or NULL */
  int64_t e_bs, g_bs, j0;
  double target_db, max_boost_db, max_cut_db;
  int32_t B, n_new, R, W, S, reserved;
} fac_agc_gains_desc;
int fac_agc_gains(const fac_agc_gains_desc* d, fac_stream_t stream);

typedef struct fac_agc_apply_desc {
  const double* carry_in;   /* (B, 2 LA) or NULL */
  double* carry_out;        /* (B, 2 LA) or NULL, never carry_in */
  const float* x;           /* (B, k), pitch x_bs */
  const int32_t* lens;      /* (B) or NULL */
  const int64_t* j_start;   /* (B) or NULL */
  const double* g;          /* (B, R), pitch g_bs */
  float* y;                 /* written: (B, n_out), pitch y_bs */
  int64_t x_bs, g_bs, y_bs, n0;
  double ceiling;
  int32_t B, k, n_out, S, LA, R;
} fac_agc_apply_desc;
int fac_agc_apply(const fac_agc_apply_desc* d, fac_stream_t stream);

int64_t fac_true_peak_ws_bytes(int B, int n_out);
int fac_true_peak(const fac_resample_desc* d, float* peak, void* ws, fac_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Noise suppression (csrc/denoise.hip): a spectral suppressor of stationary background noise.  This comment is the
 * normative definition.  Finite windows, no recurrence in time: a gain depends on the M + W - 1 power spectra up to its frame,
 * an output sample on two frames, so every frame is computable in parallel and any chunking of a stream gives the bits of the
 * offline call.  Unless said otherwise every operation below is one IEEE fp64 operation with one round-to-nearest; nothing is
 * fused.
 *
 * Framing.  N = 512, H = 256, w[n] = sinpi(n / 512) (the device library's sinpi of the fp64 quotient), analysis and synthesis
 * window alike; w[n]^2 + w[n + H]^2 = 1.  Per row b the signal is the virtual concatenation [carry | block]: the block's sample i
 * has the absolute index n0 + i and exists for i < k_b = lens ? clamp(lens[b], 0, k) : k; carry_in (B, FAC_NS_CARRY) fp32, dense,
 * holds the samples n0 - FAC_NS_CARRY .. n0 - 1 (NULL: zeros).  A sample before start_b = starts ? max(starts[b], 0) : 0, at or
 * behind n0 + k_b, or before the carry is 0 and is not read.  Frame f >= 0 covers the samples (f - 1) H .. (f + 1) H - 1;
 * fs_b = start_b / H is the first frame of the row's current stream.
 *
 * Transform.  z[n] = (w[n] * (double)sample, 0), n < 512.  Forward: for half = 256, 128, .. 1, for every i < 256 with
 * pos = i % half, lo = 2 (i - pos) + pos, hi = lo + half, t = tw[pos * (256 / half)], tw[j] = (c, -s) of sincospi(j / 256):
 *   (u, v) = (z[lo], z[hi]);  z[lo] = u + v;  d = u - v;  z[hi] = (d.x t.x - d.y t.y,  d.x t.y + d.y t.x)
 * -- the radix-2 decimation in frequency of stoi_bands_kernel, butterfly for butterfly.  X[k] = z[rev9(k)] (the 9-bit reversal).
 * Inverse: for half = 1, 2, .. 256, same i, pos, lo, hi, t:
 *   q = (v.x t.x + v.y t.y,  v.y t.x - v.x t.y);  z[lo] = u + q;  z[hi] = u - q;      then every z[n] times 1 / 512 (exact).
 *
 * fac_ns_power: P_f[k] = X.x^2 + X.y^2, k = 0 .. 256, for the n_new frames f = f0 .. f0 + n_new - 1, written frame-major
 * (FAC_NS_BINS contiguous doubles per frame) into the ring P (B, R, 257) of row pitch p_bs doubles, frame f at slot f % R (a
 * plain (B, F, 257) array is R >= F, f0 = 0).  X, NULL or a ring of the same geometry in double2 units: the spectra themselves,
 * for fac_ns_synth.  carry_out (B, FAC_NS_CARRY), NULL or a buffer OTHER than carry_in: the samples n0 + k - FAC_NS_CARRY ..
 * n0 + k - 1, written by one extra workgroup per row of the same launch; n_new = 0 with carry_out only moves the carry.  After n
 * samples of a stream the frames below n / H are complete.  One wave per frame, 4 x 4 frames per 256-thread workgroup, 40 KB LDS.
 * Refused before any launch: a NULL descriptor or P; x NULL with k > 0; B outside 1 .. 65535; k outside 0 .. 2^30; n_new < 0, or
 * 0 without carry_out; n0 or f0 negative; carry_out == carry_in; lens with a carry buffer; x_bs < k or p_bs < 257 R with B > 1;
 * R outside max(n_new, 1) .. 2^22; with carry_in, a frame f0 that starts before the carry.
 *
 * fac_ns_gains: for the n_new frames f = f0 .. f0 + n_new - 1 and every bin k, from the ring P:
 *   S_f[k]  = (P_lo[k] + .. + P_f[k]) / (double)(f - lo + 1),  lo = max(fs_b, f - M + 1), the sum left to right from P_lo
 *   Nf_f[k] = min S_g[k] over g = max(fs_b, f - W + 1) .. f                        (exact in any order)
 *   Nf_f[k] == 0:  G_f[k] = 1                                    (digital silence in the window: nothing can be estimated)
 *   else  xi = max(S_f[k] / (over * Nf_f[k]) - 1, 0);   G_f[k] = max(xi / (1 + xi), g_min)
 * g_min = 10^(-max_atten_db / 20) is the host's, handed over as fp64.  A frame f < fs_b gets G = 1.  G (B, R, 257) fp64 of row
 * pitch g_bs, frame f at slot f % R.  One 256-thread workgroup per (row, 64 frames, 16 bins): P of the tile and its M + W - 2
 * older neighbours in LDS, then S of the tile and its W - 1 older neighbours, then the minimum and the gain, one thread per
 * (bin, four consecutive frames), which reads the S their windows share once; (125 + M + 2 W) * 128 bytes of dynamic LDS
 * (41.6 KB at M = 8, W = 96).
 * Refused before any launch: a NULL descriptor, P or G; B outside 1 .. 65535; n_new < 1; M outside 1 .. FAC_NS_MAX_M; W outside
 * 1 .. FAC_NS_MAX_W; over not in (0, inf); g_min not in (0, 1]; f0 < 0; R < min(f0 + n_new, M + W - 2 + n_new) or above 2^22;
 * p_bs or g_bs below 257 R with B > 1.
 *
 * fac_ns_synth: v_f = w * Re(inverse(Y_f)) with Y_f[k] = (G_f[k] X_f[k].x, G_f[k] X_f[k].y) for k = 0 .. 256 and
 * Y_f[512 - k] = conj(Y_f[k]) for k = 1 .. 255; v_f = 0 for f < fs_b.  X_f is transformed again from the samples (the same
 * bits as fac_ns_power's) or, with X != NULL, read from that ring (row pitch g_bs double2; no sample is read then).
 *   y[m] = (float)(v_f[m - (f - 1) H] + v_{f+1}[m - f H]),  f = m / H: the older frame first, one fp64 sum, one rounding to fp32
 *   y[m] = 0 for m < start_b (and so for m < 0) and for m >= n0 + k_b
 * The call writes y[b * y_bs + i] = y[m0 + i], i < n_out: store only.  Offline n0 = m0 = 0, n_out = k.  In a stream the caller
 * asks only for samples whose two frames are complete (m0 + n_out <= (floor((n0 + k) / H) - 1) H), or the signal ends with
 * this block; the constant delay of a block-in, block-out stream is D = 2 H = 512 samples: m0 = n0 - 512, n_out = k, and the
 * flush is k = 0, n_out = 512.  FAC_NS_CARRY = 1023 is what the oldest such output reaches back.  One workgroup per (row,
 * 15 segments) transforms their 16 frames, one wave per frame, and keeps the last half frame of a round in LDS for the next:
 * 42 KB LDS.
 * Refused before any launch: a NULL descriptor, G or y; x NULL with k > 0 and no X; B outside 1 .. 65535; k outside 0 .. 2^30;
 * n_out outside 1 .. 2^30; n0 < 0; lens with a carry buffer; x_bs < k, y_bs < n_out or g_bs < 257 R with B > 1; outputs that
 * reach in front of the carry (or, with n0 > 0 and no carry or X, in front of the block); R below the frames the outputs reach
 * (floor(m0 / H) .. floor((m0 + n_out - 1) / H) + 1 in different slots) or above 2^22.
 * ---------------------------------------------------------------------------------------- */
enum { FAC_NS_N = 512, FAC_NS_H = 256, FAC_NS_BINS = 257, FAC_NS_CARRY = 1023, FAC_NS_MAX_M = 64, FAC_NS_MAX_W = 256 };
typedef struct fac_ns_power_desc {
  const float* carry_in;    /* (B, FAC_NS_CARRY) or NULL */
  float* carry_out;         /* (B, FAC_NS_CARRY) or NULL, never carry_in */
  const float* x;           /* (B, k), pitch x_bs */
  const int32_t* lens;      /* (B) or NULL */
  const int64_t* starts;    /* (B) or NULL */
  double* P;                /* written: (B, R, 257), row pitch p_bs */
  double* X;                /* written: (B, R, 257, 2), row pitch p_bs double2; or NULL */
  int64_t x_bs, p_bs, n0, f0;
  int32_t B, k, n_new, R;
} fac_ns_power_desc;
int fac_ns_power(const fac_ns_power_desc* d, fac_stream_t stream);

typedef struct fac_ns_gains_desc {
  const double* P;          /* (B, R, 257), row pitch p_bs */
  const int64_t* starts;    /* (B) or NULL */
  double* G;                /* written: (B, R, 257), row pitch g_bs */
  int64_t p_bs, g_bs, f0;
  double over, g_min;
  int32_t B, n_new, R, M, W, reserved;
} fac_ns_gains_desc;
int fac_ns_gains(const fac_ns_gains_desc* d, fac_stream_t stream);

typedef struct fac_ns_synth_desc {
  const float* carry_in;    /* (B, FAC_NS_CARRY) or NULL */
  const float* x;           /* (B, k), pitch x_bs */
  const int32_t* lens;      /* (B) or NULL */
  const int64_t* starts;    /* (B) or NULL */
  const double* G;          /* (B, R, 257), row pitch g_bs */
  const double* X;          /* (B, R, 257, 2), row pitch g_bs double2; or NULL */
  float* y;                 /* written: (B, n_out), pitch y_bs */
  int64_t x_bs, g_bs, y_bs, n0, m0;
  int32_t B, k, n_out, R;
} fac_ns_synth_desc;
int fac_ns_synth(const fac_ns_synth_desc* d, fac_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Echo cancellation (csrc/aec.hip): a partitioned-block frequency-domain adaptive filter -- overlap-save, a fully
 * constrained gradient, a step normalised by the far-end power in the filter's span plus the error power.  This comment is the
 * normative definition.  The state is recursive in time: block m needs the weights block m - 1 left.  Any chunking of a stream
 * still gives the bits of the offline call, because the block grid is absolute (from sample 0 of the session), a block is
 * computed once, when its last sample is there, and the blocks of a row are computed in ascending order by one workgroup.
 * Unless said otherwise every operation below is one IEEE fp64 operation with one round-to-nearest; nothing is fused.
 *
 * Geometry.  N = 512, H = 256, bins k = 0 .. 256, P partitions (1 .. FAC_AEC_MAX_P; P H taps).  Row b has a microphone signal d
 * and a far-end signal x, both fp32, each the virtual concatenation [carry | block]: the block's sample i has the absolute index
 * n0 + i and exists for i < k_b = lens ? clamp(lens[b], 0, k) : k; mic_carry_in (B, FAC_AEC_MIC_CARRY) holds the samples
 * n0 - 255 .. n0 - 1, far_carry_in (B, far_cn), far_cn >= FAC_AEC_FAR_CARRY + delay, the samples n0 - far_cn .. n0 - 1 (NULL:
 * zeros).  A sample of either signal before start_b = starts ? max(starts[b], 0) : 0, at or behind n0 + k_b, or before the carry
 * is 0 and is not read.  The far end is used delayed: u[n] = x[n - delay], 0 <= delay <= FAC_AEC_MAX_DELAY.  Block m covers the
 * samples m H .. m H + H - 1; ms_b = start_b / H.  At block ms_b every W_p = 0 and X_j = 0 for j < ms_b; a block m < ms_b
 * computes nothing.  DFT512 and IDFT512 are the transform of the noise suppressor above, butterfly for butterfly, the inverse
 * with its factor 1 / 512; the imaginary input of every forward transform here is 0.
 *
 * Per block m >= ms_b, in this order:
 *   1. X_m = DFT512(a), a[n] = u[(m - 1) H + n], n < 512, no window; kept in the ring X (B, P, 257, 2) at slot m % P.
 *   2. Yh[k] = sum over p = 0 .. P - 1 of W_p[k] X_{m-p}[k], from (0, 0), p ascending, a product being
 *      (w.x x.x - w.y x.y,  w.x x.y + w.y x.x): four products, a difference, a sum; then the two additions into Yh.
 *   3. Yf[k] = Yh[k], k <= 256, with the imaginary parts of bins 0 and 256 set to 0; Yf[512 - k] = conj(Yh[k]), k = 1 .. 255;
 *      yh[n] = Re(IDFT512(Yf))[H + n], n < H.
 *   4. e[n] = (double)d[m H + n] - yh[n] for m H + n < n0 + k_b, 0 behind it.  The output is (float)e[n]; outputs before start_b
 *      and at or behind n0 + k_b are 0.
 *   5. E = DFT512([0^H | e]), from the fp64 e.
 *   6. S[k] = sum over p ascending of (X.x^2 + X.y^2)(X_{m-p}[k]), from 0;  den = (S[k] + c (E.x^2 + E.y^2)) + delta;
 *      step[k] = den == 0 ? 0 : mu / den.  c = beta P is the host's, handed over as fp64.
 *   7. Only if adapt[b] != 0 (adapt NULL: every row adapts): for every p, G_p[k] = step[k] * (conj(X_{m-p}[k]) E[k]), the product
 *      (x.x e.x + x.y e.y,  x.x e.y - x.y e.x) first, then each part times step[k]; the full spectrum as in 3;
 *      g = Re(IDFT512(.)), g[n] = 0 for n >= H;  W_p[k] += DFT512(g)[k], k = 0 .. 256.
 *   8. stats_m = (sum d^2, sum yh^2, sum e^2) over the block's samples n with m H + n < n0 + k_b (others count 0), each sum by
 *      the tree v[j] += v[j + s], j < s, for s = 128, 64, .. 1, over the 256 fp64 squares; the sum is v[0].
 *
 * fac_aec_run computes, per row, the blocks max(blk0, ms_b) .. min(blk0 + n_blk, ceil((n0 + k_b) / H)) - 1 and writes
 * y[b * y_bs + i] = (float)e[m0 + i], i < n_out: of a block of this call directly; of a block before blk0 from e_ring
 * (B, FAC_AEC_H) fp32, sample n at slot n % 256; 0 before start_b, behind the row's last block, below sample 0, and without a
 * ring.  An e of this call at or behind m0 + n_out is written into the ring for a later call (dropped without one).  stats,
 * NULL or (B, n_blk, 3) fp64 of row pitch s_bs: block m at index m - blk0, zeros for a block the row does not compute.
 * mic_carry_out / far_carry_out, NULL or buffers OTHER than the inputs: the last 255 / far_cn samples up to n0 + k - 1, written
 * by a second workgroup per row.  W (B, P, 257, 2) and X (B, P, 257, 2) fp64, row pitches w_bs and xr_bs doubles, are read
 * (unless the call contains block ms_b) and written in place; only row b's workgroup touches row b's state.  Offline: n0 = m0 =
 * blk0 = 0, n_out = k, n_blk = ceil(k / H), no carries, no ring.  A stream keeps the grid with a delay of D = H = 256 samples:
 * after n samples the blocks below n / H are complete, so a push of k samples at n0 is blk0 = n0 / H, n_blk = (n0 + k) / H - blk0,
 * m0 = n0 - 256, n_out = k; the flush is k = 0, n_blk = 1 if n0 % H else 0, m0 = n0 - 256, n_out = 256.
 * One 512-thread workgroup per row walks the blocks; steps 1 and 3 to 5 are one wave's transforms, 2 and 6 one thread per bin,
 * 7 one wave per partition in ceil(P / 8) rounds.  P <= FAC_AEC_LDS_P keeps W and the X ring in LDS for the call (84160 +
 * 8224 P bytes of dynamic LDS), a larger P works on them in global memory; the arithmetic is the same.
 * Refused before any launch: a NULL descriptor, W, X or y; mic or far NULL with k > 0; B outside 1 .. 65535; P outside 1 ..
 * FAC_AEC_MAX_P; mu not in [0, 1]; c or delta negative or not finite; delay outside 0 .. FAC_AEC_MAX_DELAY; k outside 0 .. 2^30;
 * n_out outside 1 .. 2^30; n_blk, n0 or blk0 negative; lens with a carry or a ring; a carry_out that is its carry_in; W and X
 * the same buffer; far_cn < 511 + delay with a far carry; w_bs or xr_bs below 514 P, mic_bs or far_bs below k, y_bs below n_out,
 * s_bs below 3 n_blk, with B > 1; a block blk0 that starts in front of the carries; with a ring, outputs that reach more than
 * 256 samples in front of block blk0, or more than 256 computed samples that are not due.
 *
 * fac_aec_state_sizes: the per-row sizes of a stream's state for (P, delay) into sizes[0 .. 4]: doubles of W, doubles of X,
 * floats of the mic carry, floats of the far carry, floats of the e ring.
 * ---------------------------------------------------------------------------------------- */
enum { FAC_AEC_N = 512, FAC_AEC_H = 256, FAC_AEC_BINS = 257, FAC_AEC_MAX_P = 32, FAC_AEC_LDS_P = 8, FAC_AEC_MAX_DELAY = 16384,
       FAC_AEC_MIC_CARRY = 255, FAC_AEC_FAR_CARRY = 511 };
typedef struct fac_aec_desc {
  const float* mic_carry_in;  /* (B, 255) or NULL */
  float* mic_carry_out;       /* (B, 255) or NULL, never mic_carry_in */
  const float* far_carry_in;  /* (B, far_cn) or NULL */
  float* far_carry_out;       /* (B, far_cn) or NULL, never far_carry_in */
  const float* mic;           /* (B, k), pitch mic_bs */
  const float* far;           /* (B, k), pitch far_bs */
  const int32_t* lens;        /* (B) or NULL */
  const int64_t* starts;      /* (B) or NULL */
  const int32_t* adapt;       /* (B) or NULL: every row adapts */
  double* W;                  /* read and written: (B, P, 257, 2), row pitch w_bs doubles */
  double* X;                  /* read and written: (B, P, 257, 2), row pitch xr_bs doubles, block j at slot j % P */
  float* e_ring;              /* read and written: (B, 256), or NULL */
  float* y;                   /* written: (B, n_out), pitch y_bs */
  double* stats;              /* written: (B, n_blk, 3), row pitch s_bs doubles, or NULL */
  int64_t mic_bs, far_bs, y_bs, w_bs, xr_bs, s_bs, n0, m0, blk0;
  double mu, c, delta;
  int32_t B, k, n_out, n_blk, P, delay, far_cn, reserved;
} fac_aec_desc;
int fac_aec_run(const fac_aec_desc* d, fac_stream_t stream);
int fac_aec_state_sizes(int P, int delay, int64_t* sizes);

/* ------------------------------------------------------------------------------------------
 * Echo delay (csrc/echo_delay.hip): a per-row estimator and tracker of the playout-to-capture delay -- a
 * PHAT-weighted, recursively smoothed cross-spectrum per lag of 256 samples, a latch policy on its peak -- and the aligner that
 * hands the canceller above a far end already moved by that delay, so that the canceller runs with delay = 0.  This comment is
 * the normative definition.  The state is recursive in time; any chunking of a stream gives the bits of the offline call,
 * because the frame grid is absolute, a frame is computed once, when its last sample is there, the frames of a row are computed
 * in ascending order by one workgroup, and a sample of block j is aligned by what the frames up to j - 1 decided, which are
 * complete before the block's first sample: the stage adds no latency.  Every operation below is one IEEE fp64 operation with
 * one round-to-nearest; nothing is fused.  No parameter was tuned by listening.
 *
 * Geometry.  N = 512, H = 256: the canceller's block grid.  Row b has a microphone signal d and a far-end signal x, both fp32;
 * the call's sample i has the absolute index n0 + i and exists for i < k_b = lens ? clamp(lens[b], 0, k) : k.  mic_ring (B,
 * FAC_EDELAY_MIC_RING) and far_ring (B, far_rn), far_rn = (L + 1) H + 255, hold the samples in front of n0, sample n at slot
 * n % 511 and n % far_rn (NULL: zeros).  A sample of either signal before start_b = starts ? max(starts[b], 0) : 0, at or behind
 * end_b = n0 + k_b, or further back than its ring is 0 and is not read.  Frame m >= 1 covers the samples (m - 1) H .. (m + 1) H -
 * 1 of both signals and is complete when sample (m + 1) H - 1 is there.  ms_b = start_b / H; the row's first frame is ms_b + 1,
 * its last floor(end_b / H) - 1.  Window w[n] = sinpi((n + 0.5) / 512).  Lags l = 0 .. L, L = ceil(max_delay / H), 1 <=
 * max_delay <= FAC_EDELAY_MAX_DELAY.  Bins k_lo .. k_hi - 1, 0 <= k_lo < k_hi <= 257, n_bins = k_hi - k_lo <= 256.  At frame
 * ms_b + 1 every C_l = 0, (cand, run, locked) = (-1, 0, -1), and no earlier frame is active.  DFT512 and IDFT512 are the transform
 * of the noise suppressor above, butterfly for butterfly.
 *
 * Per frame m, in this order:
 *   1. X_m = DFT512(w f), f[n] = (double)x[(m - 1) H + n], and D_m = DFT512(w g), g the same of d; each product w[n] f[n] once
 *      rounded, the imaginary input 0.  X_m is kept in the ring X (B, L + 1, 257, 2) at slot m % (L + 1), bins k_lo .. k_hi - 1.
 *   2. actx_m = (sum f^2) / 512 > gate, actd_m the same of g; each sum by the tree v[j] += v[j + s], j < s, for s = 256, 128, .. 1,
 *      over the 512 fp64 squares.  actx_m is kept in the ring act (B, L + 1) at slot m % (L + 1).
 *   3. If actd_m: for every lag l with m - l >= ms_b + 1 and actx_{m-l}, and every bin k of the band, with x = X_{m-l}[k], d =
 *      D_m[k]:  p = (x.x d.x + x.y d.y,  x.x d.y - x.y d.x), i.e. conj(x) d: four products, a sum, a difference;
 *      den = sqrt(x.x x.x + x.y x.y) * sqrt(d.x d.x + d.y d.y) + eps;  q = (p.x / den, p.y / den);
 *      C_l[k] = ((1 - a) C_l[k].x + a q.x,  (1 - a) C_l[k].y + a q.y), 1 - a computed once in fp64.  Any other C_l stays.
 *   4. score_l = (sum over the band of C_l[k].x^2 + C_l[k].y^2) / n_bins for every l: the squares at j = k - k_lo, zeros up to
 *      256 entries, summed by the tree v[j] += v[j + s], j < s, s = 128, 64, .. 1 (the canceller's step 8).
 *   5. l* = the l of the largest score, compared with > in ascending l (the lowest l wins a tie); conf_m = score_{l*}.
 *   6. G[k] = C_{l*}[k] in the band, 0 outside it, the imaginary parts of bins 0 and 256 set to 0, G[512 - k] = conj(G[k]) for k =
 *      1 .. 255;  g = Re(IDFT512(G)) (its factor 1 / 512 does not matter);  n* = the n of the largest |g[n]|, n = 0 .. 511,
 *      compared with > in ascending n;  r = n* < H ? n* : n* - N;  raw_m = max(0, l* H + r).
 *   7. ok_m = conf_m >= thr and actd_m and m - l* >= ms_b + 1 and actx_{m-l*}.
 *   8. The latch.  If ok_m: if cand >= 0 and |raw_m - cand| <= tol then run += 1, else cand = raw_m and run = 1.  Then, ok_m or
 *      not: if run >= hold and (locked < 0 or |cand - locked| >= move) then locked = cand.  locked_m is locked after this step;
 *      used_m = locked_m < 0 ? delay0 : max(0, locked_m - margin).  used_m = delay0 for m < ms_b + 1.
 * The aligner: y[n] = x[n - used_{n / H - 1}] for start_b <= n < end_b, where the source index is not before start_b; 0 otherwise.
 *
 * fac_edelay_run computes, per row, the frames max(frm0, ms_b + 1) .. min(frm0 + n_frm, floor(end_b / H)) - 1 and writes the k
 * aligned samples y[b * y_bs + i], sample n0 + i.  Per-frame outputs, each NULL or (B, f_n) of row pitch f_bs entries (score:
 * (B, f_n, L + 1), row pitch f_bs (L + 1)): raw, locked, used int32, conf fp64, ok uint8, score fp64.  With f_ring = 0, f_n =
 * n_frm and frame m is at column m - frm0; a column that is not a frame of the row holds raw = locked = used = -1, conf = 0, ok =
 * 0, score = 0.  With f_ring > 0 (a stream's rings), f_n = f_ring >= n_frm, frame m is at column m % f_ring and no other column is
 * written.  The state -- C (B, L + 1, 257, 2) fp64 of row pitch c_bs doubles, X of row pitch xr_bs doubles, act (B, L + 1) int32,
 * pol (B, 4) int32 = (cand, run, locked, used) after the row's last computed frame, conf_last (B) fp64, the two rings -- is read
 * (unless the call holds frame ms_b + 1) and written in place; only row b's workgroup touches row b's state, and the rings take
 * the call's last samples behind the workgroup's last read.  Offline: n0 = 0, frm0 = 1, n_frm = max(k / H - 1, 0), no rings,
 * zeroed state.  A stream: after n samples the frames below n / H are complete, so a push of k samples at n0 is frm0 = max(n0 /
 * H, 1), n_frm = max((n0 + k) / H - frm0, 0).  One 512-thread workgroup per row walks the call's blocks: it aligns block j's
 * samples, then computes frame j if the call completes it.  Steps 1 and 2 are one wave's per signal, 3 and 4 one wave per lag in
 * ceil((L + 1) / 8) rounds, 5 to 8 wave 0's.  C and X stay in global memory (L2); 25472 bytes of LDS.
 * Refused before any launch: a NULL descriptor, mic, far, C, X, act, pol, conf_last or y; B outside 1 .. 65535; k outside 1 ..
 * 2^30; max_delay outside 1 .. FAC_EDELAY_MAX_DELAY; a band outside 0 <= k_lo < k_hi <= 257 or wider than 256 bins; a outside
 * (0, 1]; eps not positive and finite; gate or thr negative or not finite; hold < 1; tol, move or margin negative; delay0 outside
 * 0 .. max_delay; n0 negative; frm0 < max(n0 / H, 1); n_frm negative or frames that end behind n0 + k; one ring without the other;
 * far_rn other than (L + 1) H + 255 with the rings; lens with the rings; f_ring negative or below n_frm; C and X the same buffer;
 * mic_bs, far_bs or y_bs below k, c_bs or xr_bs below 514 (L + 1), f_bs below the columns, with B > 1.
 *
 * fac_edelay_state_sizes: the per-row sizes of a stream's state for max_delay into sizes[0 .. 5]: doubles of C, doubles of X,
 * ints of act, ints of pol, floats of the mic ring, floats of the far ring.
 * ---------------------------------------------------------------------------------------- */
enum { FAC_EDELAY_MAX_DELAY = 16384, FAC_EDELAY_MAX_LAGS = 65, FAC_EDELAY_MIC_RING = 511, FAC_EDELAY_POL = 4 };
typedef struct fac_edelay_desc {
  const float* mic;           /* (B, k), pitch mic_bs */
  const float* far;           /* (B, k), pitch far_bs */
  const int32_t* lens;        /* (B) or NULL */
  const int64_t* starts;      /* (B) or NULL */
  float* mic_ring;            /* read and written: (B, 511), or NULL */
  float* far_ring;            /* read and written: (B, far_rn), or NULL */
  double* C;                  /* read and written: (B, L + 1, 257, 2), row pitch c_bs doubles */
  double* X;                  /* read and written: (B, L + 1, 257, 2), row pitch xr_bs doubles, frame j at slot j % (L + 1) */
  int32_t* act;               /* read and written: (B, L + 1), frame j at slot j % (L + 1) */
  int32_t* pol;               /* read and written: (B, 4): cand, run, locked, used */
  double* conf_last;          /* read and written: (B) */
  float* y;                   /* written: (B, k), pitch y_bs: the aligned far end */
  int32_t* raw;               /* written: (B, f_n), pitch f_bs, or NULL */
  int32_t* locked;            /* the same */
  int32_t* used;              /* the same */
  double* conf;               /* the same */
  uint8_t* ok;                /* the same */
  double* score;              /* written: (B, f_n, L + 1), pitch f_bs (L + 1), or NULL */
  int64_t mic_bs, far_bs, y_bs, c_bs, xr_bs, f_bs, n0, frm0;
  double a, eps, gate, thr;
  int32_t B, k, n_frm, f_ring, max_delay, far_rn, k_lo, k_hi, hold, tol, move, margin, delay0, reserved;
} fac_edelay_desc;
int fac_edelay_run(const fac_edelay_desc* d, fac_stream_t stream);
int fac_edelay_state_sizes(int max_delay, int64_t* sizes);

static inline int fac_pad32(int n) { return (n + 31) & ~31; }
/* packed weights carry zero rows up to a multiple of 48 input channels (lcm of the kernel's
 * channels-per-stage choices), so a partially filled last stage multiplies zeros */
static inline int fac_cin_pad(int c) { return ((c + 47) / 48) * 48; }

/* ------------------------------------------------------------------------------------------
 * Data-parallel gradient exchange as an explicit RCCL collective over a flat fp32 arena (what
 * DistributedDataParallel does behind train.py:110-111 / :289 / :361 -- bucketed all-reduce of the gradients, mean over the ranks).
 * facodec_amd/optim.py exchanges its arenas through torch.distributed by default (backend "nccl" is RCCL on ROCm) and through this
 * entry point with FAC_NATIVE_RCCL=1; a caller without torch binds it directly.  RCCL is resolved at run time (the librccl.so.1
 * already in the process, else dlopen): the library has no link-time dependency on it.
 *   fac_rccl_unique_id     one rank creates the 128-byte id and ships it to the others by any means (the Python side: the
 *                          torch.distributed store);
 *   fac_rccl_comm_init     collective over the ranks; binds the calling thread's current device;
 *   fac_allreduce_arena    in place over `count` floats on `stream` (asynchronous; average != 0: mean over the ranks, ncclAvg);
 *                          calls on one communicator must be issued in the same order on every rank.
 * ---------------------------------------------------------------------------------------- */
int fac_rccl_available(void);
int fac_rccl_unique_id(void* id128);
int fac_rccl_comm_init(void** comm, const void* id128, int nranks, int rank);
int fac_rccl_comm_destroy(void* comm);
int fac_allreduce_arena(void* comm, float* arena, int64_t count, int average, fac_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FACODEC_HIP_H */
