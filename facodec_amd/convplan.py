"""Which weight layout a conv packs and in which form it is launched: the policy, once, in pure Python over integers and booleans.
Every call site (layers.py, autograd.py, autograd_disc.py, the gradient launches of ops.py) asks `plan_conv` / `plan_convtr` /
`plan_gemm`, packs the layout the plan names and launches the form it names: a threshold is changed HERE and nowhere else.  The
predicates mirror the C++ planner's (conv1d_api.hip: conv_plan), which has the last word on the kernel (tests/test_conv_plan_cpu.py
holds the two against each other).  The switches (BF16_SPLIT, PW_SPLIT, PW_TAPS, FLAT_TRAIN, CONVTR_ROWS, ...) stay module
attributes of `ops`, where tests and tools set them; they are read at call time."""
from collections import namedtuple

__all__ = ["ConvPlan", "ConvTrPlan", "plan_conv", "plan_convtr", "plan_gemm", "tile_rows", "gemm_split_ok", "gemm_split_strided_ok", "split2_ok",
           "pw_taps_ok", "pw_split_tail_ok", "convtr_split_ok", "convtr_rows_ok", "flat_strided_ok", "flat_convtr_ok", "W_FP32", "W_TAPS",
           "W_GEMM", "W_GEMM_STRIDED", "W_SPLIT2", "W_FP32_PW_TAPS", "PER_CLIP", "FLAT_STRIDED", "FLAT_STRIDE1", "TR_POLYPHASE", "TR_ROWS",
           "TR_ROWS_SPLIT", "TR_ROWS_PW_TAPS", "TR_FLAT"]          # what `ops` re-exports

# Weight layouts of a conv: the fp32 pack (ops.pack_conv_weight); split taps k = 3 / 5 / 7 (ops.pack_conv_weight_split,
# conv1d_bsplit.hip); split GEMM (the same packer at k = 1, conv1d_gemm_split.hip); strided split GEMM (ops.pack_gemm_weight_split
# with in_stride: 2 taps over `stride` phase sub-signals); split2 (conv1d_bsplit2.hip); the fp32 pack for the streaming kernel with taps.
W_FP32, W_TAPS, W_GEMM, W_GEMM_STRIDED, W_SPLIT2, W_FP32_PW_TAPS = "fp32", "split_taps", "split_gemm", "split_gemm_strided", "split2", "fp32_pw_taps"
# Launch forms: per clip, or short clips padded and laid out as ONE signal (ops.conv1d_flat), strided (k = 2 s) or stride-1 (k = 7).
PER_CLIP, FLAT_STRIDED, FLAT_STRIDE1 = "per_clip", "flat_strided", "flat_stride1"
# p8: FLOP per input byte of a launch whose input may go through the P8 pre-pass (ops.p8_prepass decides), else None
ConvPlan = namedtuple("ConvPlan", "layout form p8")
# Layouts of a transposed conv (TR_FLAT: the rows-split weights, clips flattened by ops.conv_transpose1d_flat)
TR_POLYPHASE, TR_ROWS, TR_ROWS_SPLIT, TR_ROWS_PW_TAPS, TR_FLAT = "polyphase", "rows", "rows_split", "rows_pw_taps", "flat_rows_split"
ConvTrPlan = namedtuple("ConvTrPlan", "layout p8")


def _sw():
    from . import ops
    return ops


# ------------------------------------------------------------------------------------------ predicates (mirrors of conv_plan's)
def gemm_split_ok(c_out, c_in, k, n_cols, t_out=None):
    """1- / 2-tap stride-1 conv worth the bf16 pipe: many input channels (below ~256 the k = 1 layers are HBM-bound and the
    streaming kernel conv1d_pw.hip is the right tool), at least half a row tile, enough columns."""
    sw = _sw()
    if not (sw.BF16_SPLIT and k in (1, 2)):
        return False
    if c_in < sw.GEMM_SPLIT_MIN_CIN or c_out < 64 or n_cols < 1024:
        return False
    return k == 1 or (t_out is not None and t_out >= 256)


def gemm_split_strided_ok(c_out, c_in, k, stride, batch, t_out):
    """Strided conv with stride < k <= 2 * stride (the encoder's k = 2 s downsampling convs, the period discriminators' k = 5
    stride-3 convs) as a 2-tap split GEMM over the `stride` phase sub-signals: mirrors conv_gsplit_ok."""
    return (_sw().BF16_SPLIT and 1 < stride <= 16 and stride < k <= 2 * stride and c_in >= 32
            and c_out >= 64 and t_out >= 256 and batch * t_out >= 1024)


def split2_ok(c_out, k, k1, stride, n_cols):
    """Few-output-channel 9- / 3-tap conv (plain or two-level, taps per level k1) for conv1d_bsplit2.hip: mirrors
    conv_bsplit2_ok."""
    kv = k1 if 0 < k1 < k else k
    return (_sw().BF16_SPLIT and 8 <= c_out <= 32 and ((kv == 9 and stride in (1, 2)) or (kv == 3 and stride == 1))
            and n_cols >= 4096)


def pw_split_tail_ok(c_in, c_out, cols):
    """C = 256 / 384 ResidualUnit tails (and their data gradients) of the TRAINING step on the streaming bf16-plane kernel instead
    of the split GEMM kernel (round 6: 0.29 -> 0.2 ms per launch at 16 x 4800 columns)."""
    sw = _sw()
    return sw.BF16_SPLIT and sw.PW_SPLIT and c_in == c_out and c_in in (256, 384) and cols >= 65536


def pw_taps_ok(c_in, c_out, k, stride, transposed, batch, t_out):
    """Mirror of conv_pwt_ok: the causal ConvTranspose1d with stride 2 (all output phases as rows, fp32 weights of
    pack_convtr_weight_rows) or a k = 4 stride-2 conv (fp32 weights of pack_conv_weight) whose C_in * taps <= 384 virtual channels
    fit the LDS as bf16 planes for 64 output rows; t_out = output columns per clip at the INPUT rate (transposed) / output rate."""
    sw = _sw()
    if not (sw.BF16_SPLIT and sw.PW_SPLIT and sw.PW_TAPS and stride == 2):
        return False
    taps, rows = (2, 2 * c_out) if transposed else (4, c_out)
    if k != 4 or (c_in * taps) % 64 or c_in * taps > 384 or rows % 64:
        return False
    return batch * ((t_out + 31) // 32) >= 2 * (256 // (rows // 64)) * 12


def convtr_rows_ok(t_in, stride, causal=True):
    sw = _sw()
    return sw.CONVTR_ROWS and causal and 2 <= stride <= 16 and t_in >= sw.CONVTR_ROWS_MIN_T


def convtr_split_ok(c_in, c_out, stride, batch, t_in, causal=True, alpha_in=None):
    """All-phases ConvTranspose1d on the split-bf16 GEMM kernel (conv1d_gemm_split.hip, K = 2): mirrors conv_gsplit_ok."""
    return (_sw().BF16_SPLIT and causal and alpha_in is None and 2 <= stride <= 16 and c_in >= 64
            and t_in >= 256 and batch * t_in >= 1024 and c_out * stride >= 64)


def flat_strided_ok(c_out, c_in, k, s, batch, n_out):
    """A k = 2 s strided conv over `batch` clips of n_out outputs each, too short for per-clip tiles but long enough as one signal."""
    return (_sw().FLAT_TRAIN and k == 2 * s and s > 1 and n_out < 256 and not gemm_split_strided_ok(c_out, c_in, k, s, batch, n_out)
            and gemm_split_strided_ok(c_out, c_in, k, s, 1, batch * (n_out + 1) - 1))


def flat_convtr_ok(c_in, c_out, s, batch, t_cols):
    """An all-phases ConvTranspose1d launch over `batch` clips of t_cols input columns each (incl. their zero column), short clips."""
    return (_sw().FLAT_TRAIN and t_cols < 256 and not convtr_split_ok(c_in, c_out, s, batch, t_cols)
            and convtr_split_ok(c_in, c_out, s, 1, batch * t_cols))


def tile_rows(c_out, c_in, k, grad=False):
    """Output rows per tile of a W_TAPS launch, which is also the co-tile size its weights are packed for (ops.pack_conv_weight_split
    `rows`, fac_conv_desc.split_rows): 96 -- the 96 x 256 form of the k = 7 split kernel (conv1d_bsplit96.hip) -- for the output
    channel counts listed in ops.BS_ROWS96 (a module attribute: the A/B sets it to ()), else 64.  grad=True is what the training sites (autograd.py, the
    data gradients of ops.py) ask with: they keep the 64-row form, the training step was not part of the A/B that wired the channel
    counts.  The inference modules (layers.SConv1d) ask without it whether or not autograd is recording, so that a forward gives the
    same bits either way.  The figure refines a ConvPlan whose
    layout is W_TAPS; it is not a field of the tuple, whose three fields tests/golden/conv_plan_table.json records."""
    sw = _sw()
    return 96 if (sw.BF16_SPLIT and not grad and k == 7 and c_out in sw.BS_ROWS96 and c_in % 8 == 0) else 64


# ------------------------------------------------------------------------------------------ planners
def plan_conv(c_out, c_in, k, stride, dilation, batch, t_in, t_out, *, k1=0, alpha_in=False, plain=True, res=False,
              causal_reflect=False, grad=True, c_out_mult16=True, split_k=(1, 3, 5, 7), floor_k=(3, 5), tail="pw_split",
              pw_taps=True, split2=False, flat_infer=False, flat_stride1=False, flat_train=None):
    """Plan of one forward-conv launch: `batch` clips of t_in columns -> t_out columns each.  The data gradient of a stride-1 conv
    is this function with the channels swapped (ops.conv1d_bwd_data), the dx of a transposed conv a strided forward conv.
    A W_TAPS plan is completed by tile_rows(c_out, c_in, k, grad): the co-tile size of the pack and of the launch.
    Facts of the launch: k1 (taps per level of a two-level conv, 0: plain), alpha_in (a Snake fused on the input), plain (epilogue
    without res / act / alpha_out), res, causal_reflect (causal layer with reflect padding), grad (autograd is recording).
    The sites' rules grew apart; every difference found is kept as a named argument (defaults: the training rule):
      c_out_mult16          split taps need C_out % 16 == 0.  False: the inference forward, which only needs C_out > 2.
      split_k               stride-1 kernel sizes that may leave the fp32 pack.  Discriminators: (5, 7) -- no k = 1 GEMM, no k = 3.
      floor_k               kernel sizes whose split taps need C_in >= 64 and C_out > 32 (few taps per staged column: below that the
                            fp32 tile wins).  Discriminators: (); the style encoder's plain convs (quantize._PlainConv): (3, 5, 7).
      tail                  the C = 256 / 384 tails leave the split GEMM for the streaming kernel: "pw_split" -- only while PW_SPLIT is
                            on (pw_split_tail_ok); "always" -- the inference forward, regardless; None -- quantize._PlainConv, never.
      pw_taps               the streaming kernel with taps is a candidate.  False: the discriminators never ask for it.
      split2                conv1d_bsplit2.hip is a candidate: the discriminators only.
      flat_infer, flat_stride1  layers.FLAT_SHORT_CLIPS / FLAT_STRIDE1: the inference modules flatten short clips (never under grad).
      flat_train            how a training site pads the clips it flattens (gated by FLAT_TRAIN): "reflect" -- the forward conv, which
                            tests the flat form BEFORE the taps kernel; "zero" -- the dx of a transposed conv, which tests it last.
    """
    sw = _sw()
    cols = batch * t_out
    p8 = 2.0 * c_out * k / (4.0 * stride)          # 2 C_out k / s FLOP per fp32 input sample
    if split2 and split2_ok(c_out, k, k1, stride, cols):
        return ConvPlan(W_SPLIT2, PER_CLIP, None)                # 32-channel (3, 9) / (3, 3) stacks
    if stride > 1:
        strided = not alpha_in and dilation == 1 and not k1
        flat_t = (flat_train is not None and strided and plain and t_in % stride == 0
                  and (flat_train == "zero" or (causal_reflect and t_in > stride))
                  and flat_strided_ok(c_out, c_in, k, stride, batch, t_out))
        if flat_t and flat_train == "reflect":
            return ConvPlan(W_GEMM_STRIDED, FLAT_STRIDED, p8)
        if pw_taps and stride == 2 and strided and plain and pw_taps_ok(c_in, c_out, k, 2, False, batch, t_out):
            return ConvPlan(W_FP32_PW_TAPS, PER_CLIP, None)      # few channels: the streaming kernel with taps (fac_conv_desc.pw_split)
        if strided and gemm_split_strided_ok(c_out, c_in, k, stride, batch, t_out):
            return ConvPlan(W_GEMM_STRIDED, PER_CLIP, p8)        # downsampling conv: 2 taps over `stride` phase sub-signals
        if flat_t:
            return ConvPlan(W_GEMM_STRIDED, FLAT_STRIDED, p8)
        # short clips (160-frame latent rate): per-clip column tiles would be half empty, B (T / s + 1) - 1 flattened columns fill them
        if (flat_infer and strided and not res and causal_reflect and k == 2 * stride and t_in % stride == 0 and t_in > stride
                and not grad and gemm_split_strided_ok(c_out, c_in, k, stride, 1, batch * (t_in // stride + 1) - 1)):
            return ConvPlan(W_GEMM_STRIDED, FLAT_STRIDED, p8)
    elif not alpha_in and not k1 and k in split_k:
        if k == 1 and gemm_split_ok(c_out, c_in, 1, cols):       # 1x1 with many channels: split-bf16 GEMM
            # (the C = 256 / 384 ResidualUnit tails stay on the streaming k = 1 kernel: -0.7 ms per B = 32 forward, round 4)
            if not (pw_split_tail_ok(c_in, c_out, cols) if tail == "pw_split"
                    else tail is not None and c_in == c_out and c_in in (256, 384) and cols >= 65536):
                return ConvPlan(W_GEMM, PER_CLIP, None)
        # k = 7 everywhere; WaveNet / style-encoder k = 5, encoder output conv k = 3: enough channels only (floor_k)
        if (sw.BF16_SPLIT and k in (3, 5, 7) and c_in % 16 == 0 and c_out > 2 and (c_out % 16 == 0 or not c_out_mult16)
                and cols > 640 and (k not in floor_k or (c_in >= 64 and c_out > 32))):
            # decoder input conv 1024 -> 1536 at the latent rate: 160 of 256 tile columns; flattened 0.756 -> 0.517 ms (k = 3 / 5: no gain)
            if (flat_infer and flat_stride1 and k == 7 and not res and causal_reflect and not grad and batch >= 4
                    and (k - 1) * dilation < t_in <= 224 and c_in * c_out >= 1 << 20):
                return ConvPlan(W_TAPS, FLAT_STRIDE1, None)
            return ConvPlan(W_TAPS, PER_CLIP, None)
    return ConvPlan(W_FP32, PER_CLIP, None)


def plan_gemm(c_out, c_in, n_cols):
    """A plain matrix product run as a 1x1 conv over n_cols columns (LSTM input projections and their data gradient)."""
    ok = gemm_split_ok(c_out, c_in, 1, n_cols)
    return ConvPlan(W_GEMM if ok else W_FP32, PER_CLIP, 2.0 * c_out / 4.0 if ok else None)


def plan_convtr(c_in, c_out, stride, batch, t_in, *, causal=True, alpha_in=False, grad=True, flat_infer=False, flat_train_cols=None):
    """Plan of one ConvTranspose1d (k = 2 s) launch over `batch` clips of t_in columns.  flat_infer: layers.FLAT_SHORT_CLIPS (the
    inference module, tested last, clips of up to 255 columns plus their zero column); flat_train_cols: columns per clip INCLUDING
    the zero column where a training site can flatten (causal only, gated by FLAT_TRAIN, tested first)."""
    a = True if alpha_in else None
    p8 = 2.0 * c_out * 2 * stride / 4.0            # all output phases as GEMM rows: 2 s C_out MACs per input sample
    if causal and flat_train_cols is not None and flat_convtr_ok(c_in, c_out, stride, batch, flat_train_cols):
        return ConvTrPlan(TR_FLAT, p8)
    if causal and not alpha_in and pw_taps_ok(c_in, c_out, 2 * stride, stride, True, batch, t_in):
        return ConvTrPlan(TR_ROWS_PW_TAPS, None)   # stride 2, few channels: the streaming kernel with taps
    if convtr_split_ok(c_in, c_out, stride, batch, t_in, causal, a):
        return ConvTrPlan(TR_ROWS_SPLIT, p8)
    if flat_infer and not grad and t_in < 256 and convtr_split_ok(c_in, c_out, stride, 1, batch * (t_in + 1), causal, a):
        return ConvTrPlan(TR_FLAT, p8)
    return ConvTrPlan(TR_ROWS if convtr_rows_ok(t_in, stride, causal) else TR_POLYPHASE, None)
