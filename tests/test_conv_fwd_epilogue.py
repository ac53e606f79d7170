"""The forward conv (ops.conv1d / ops.conv1d_flat -> fac_conv1d_fwd) against float64: the Snake prologue and every fused epilogue,
kernel by kernel.  The kernels whose accumulators reach all waves through an fp32 tile share one epilogue (conv1d_epilogue.h); the
table still names every kernel family, because the gather of the quad, the output address and the ownership of a sample differ.

One table (BASES x the operand / alignment variants each kernel admits -> CASES) names, for every case, the weight layout, the
operands and the kernel fac_conv1d_variant must name; the CPU-only tests walk it without a GPU, the GPU test runs it.  Weights are
plain `v` (the weight-norm rounding belongs to test_wn_scale_fp64).  Every check is cut in two:

Step A, the sum.  The case is launched with `bias` only (plus `alpha_in` where it has one): c_gpu.  Reference, float64 from the same
fp32 inputs: F.conv1d(_pad(snake64(x)), w64) + bias (`_pad`: pad1d, zero extension of signals not longer than the pad included).
  |c_gpu - c64| <= (4 sqrt(n) + extra) 2^-24 mag + 4 * 2^-24 |c64|   at every element (`_sum_bound`, c = 4), n = C_in K,
  mag    the same conv over |w| and m_in, plus |bias|; m_in = |x| without the prologue and |x| + sin^2(alpha x) / (alpha + 1e-9)
         with it -- not |snake(x)|, which cancels for negative x;
  extra  0 on the fp32 kernels, 3 on the bf16 planes (the dropped products mid * lo, lo * mid, lo * lo, each <= 2^-24 of its term:
         tests/test_conv_bwd_data.py).  With the prologue + 7: the roundings of snake_apply (common.h) on top of sin_sq's stated
         1 ulp, in units of 2^-24 of m_in: 0.5 for fl(alpha x) (it moves sin^2 by |x| |sin 2 alpha x| 2^-24 <= m_in 2^-24), 4 for
         sin^2 (sin to 1 ulp = 2 * 2^-24, squared doubles it), 0.5 for the square, 1 for inv = fl(1 / fl(alpha + 1e-9)), 0.5 for
         inv * sin^2, 0.5 for the final add.

Step B, the epilogue as a map.  The full case is launched; through the spy both launches must name the same kernel, the one of the
table.  The reference starts from the kernel's OWN pre-activation, so the conditioning of sin(alpha c) never enters a tolerance:
  r64 = res + act64(snake64(c_gpu.double(), alpha_out)),  r32 the same expression in fp32 torch on the CPU (the yardstick),
  y2 against snake64(y_gpu.double(), alpha_y2);  `_bar(got, r64, r32, scale = per-channel max |r64|)`, factor 4, at every element.
Step B assumes the plain and the full launch share accumulator bits; where the kernel admits y2 the test verifies it: the `y` of a
launch that adds only alpha_y2 is bit-identical to c_gpu (`y2` variant).  Every kernel of the table shared them.

Snake parameters are 1 + 0.2 rand except two planted channels: alpha = 1 exactly on channel 0, and alpha = 1e-6 on channel 1,
whose weight row (alpha_out / alpha_y2) or input row (alpha_in) is scaled by 1e6 so that alpha * value = O(1) and the 1e-9 of the
denominator shows (the trick of test_snake_fwd_fp64).  For alpha_in the weight COLUMN of that input row is scaled by 1e-6 as well:
the row then contributes O(1) terms like every other row, and errors in the other channels stay visible beside it.

Outputs given to ops.conv1d sit inside a canary buffer that must be intact afterwards, and no output element may equal the canary.
(`y2` is allocated by ops.conv1d itself, and both outputs of ops.conv1d_flat are: those cannot be wrapped.)  Alignment variants:
`a` T_out % 4 == 0 and 16-byte aligned buffers, `odd` T_out % 4 in {1, 3}, `res1` / `out1` the residual / the output as a view one
float into a larger buffer.

Lost low plane: every split-bf16 case whose kernel or pack the gradient tables do not run (96-row split taps, bsplit2, the forward
split-GEMM packs, pws, forward pwt) runs again with ops.BF16_SPLIT = False on the fp32 pack and must stay within 1.5 x that
route's error + 1e-7 (max error over max |c64|), the bar of test_split_bf16_conv_matches_fp32_grade.

The fused ResidualUnit keeps h = snake(conv7 + b7) in registers, so it is held to the composite bound (test_fused_residual_unit).
"""
# Measured on MI355X.  Step A, worst error / bound of each kernel over its cases, without / with the prologue (every kernel is under
# 4 sqrt(n); the + 7 of the prologue was never needed: its cases sit lower than the plain ones):
#   fp32 tiles   128x32 0.138 / 0.084, 32x256 0.114 / 0.064, 64x128 0.089 / 0.047, 96x128 0.092 / 0.048, 128x128 0.293 (the mel shape,
#                n = 1025) / 0.041, 128x160 0.122 / 0.086, 96x256 0.180 / 0.118, 128x256 0.178 / 0.148
#   VALU         narrow - / 0.073, thin 0.028 / 0.009, cin1 0.220;  split reduction 0.116, single launch 0.085
#   bf16 planes  split taps k = 3 0.061, k = 5 0.055, k = 7 0.059, 96-row 0.048; split GEMM 0.075; bsplit2 0.110
#   streaming    pw 0.227, pws 0.143, pwt 0.141
#   fused ResidualUnit, error / composite bound: 0.0013 .. 0.0030 (the bound pushes the worst case of h through |W1|)
# Step B, worst GPU / fp32-CPU pair of each epilogue form (units of the per-channel max |r64|; bar 4 x the second + 4 ulp):
#   per-wave tiles 1.3e-7 / 8.1e-8, all-waves tiles 1.1e-7 / 8.6e-8, split taps 1.0e-7 / 8.4e-8 (tanh 8.4e-8 / 3.0e-8), bsplit2 1.0e-7 / 7.9e-8, split GEMM
#   1.1e-7 / 8.6e-8 (tanh 7.9e-8 / 3.0e-8), pw 9.8e-8 / 8.4e-8, pws 6.1e-8 / 5.5e-8, pwt 1.2e-7 / 1.0e-7, narrow 7.1e-8 / 3.0e-8, thin 7.2e-8 / 3.0e-8, cin1
#   8.3e-8 / 3.3e-8, split reduction 9.7e-8 / 5.4e-8 (log-mel), single launch 2.8e-7 / 8.3e-8; fused ResidualUnit y2 9.2e-8 / 7.8e-8.
#   The `y` of every launch that adds only alpha_y2 was bit-identical to the plain launch's: no kernel needed the composite bound.
# Ragged flattened quads (test_ragged_flattened_quads_against_fp64), measured on the commit before conv1d_epilogue.h and again with it,
# the same figures on the 128 x 128 and on the 64 x 128 form: Step A 0.104 of the bound; Step B full y 9.1e-8 / 9.1e-8, y2 1.0e-7 /
# 9.7e-8, tanh_res 6.6e-8 / 6.6e-8; the `y` of the launch that adds only alpha_y2 bit-identical to the plain launch's.
# Split against fp32 route (max error / max |c64|), 25 pairs: split 1.3e-7 .. 6.8e-7, fp32 1.8e-7 .. 9.9e-7; worst pair 4.8e-7
# against 3.8e-7 (96-row split taps), next 6.8e-7 against 6.4e-7 (split GEMM, k = 2).
# Wall time of this file's GPU tests together with tests/test_convtr_fwd.py: 48 s for 489 cases, the slowest 2.3 s (the streaming
# kernels' cases: 16 M outputs each and their float64 maps on the CPU).
from collections import namedtuple
import functools
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from facodec_amd import _lib, convplan, ops
from test_conv_launch_desc import FLAT, _Spy
from test_conv_plan_cpu import assert_same_launch, conv_launch, fake_operands, flat_conv_launch
from test_train_kernels_gen import CANARY, EPS32, _bar, _canary, _canary_intact, _record, _sum_bound
from test_wgrad_split import _pad

gpu = pytest.mark.gpu
REFLECT, ZERO = ops.PAD_REFLECT, ops.PAD_ZERO
FP32, TAPS, GEMM, GSTR, SPLIT2, PWT = (convplan.W_FP32, convplan.W_TAPS, convplan.W_GEMM, convplan.W_GEMM_STRIDED, convplan.W_SPLIT2,
                                       convplan.W_FP32_PW_TAPS)
SPLIT_LAYOUTS = (TAPS, GEMM, GSTR, SPLIT2)

# ------------------------------------------------------------------------------------------------ operand sets and variants
# aout: alpha_out; act; res: True, or "out" (the output buffer holds the residual: in place); y2: alpha_y2; want_y
Ops = namedtuple("Ops", "aout act res y2 want_y", defaults=(False, ops.ACT_NONE, False, False, True))
OPS = {
    "plain": Ops(),
    "full": Ops(aout=True, res=True, y2=True),
    "tanh_res": Ops(act=ops.ACT_TANH, res=True),
    "mish": Ops(act=ops.ACT_MISH),
    "y2only": Ops(y2=True, want_y=False),
    "inplace": Ops(aout=True, res="out"),
    "y2": Ops(y2=True),
    "aout_y2": Ops(aout=True, y2=True),
    "aout": Ops(aout=True),
    "tanh": Ops(act=ops.ACT_TANH),
    "log_mel": Ops(act=ops.ACT_LOG_MEL),
}
# what a kernel admits -> (operand set, alignment) list.  `full`: the six operand sets of the issue and the four alignments.
ADMITS = {
    "full": [("plain", "a"), ("y2", "a"), ("full", "a"), ("tanh_res", "res1"), ("mish", "out1"), ("y2only", "a"), ("inplace", "a"),
             ("full", "odd"), ("tanh_res", "odd")],
    "nores": [("plain", "a"), ("y2", "a"), ("aout_y2", "a"), ("tanh", "out1"), ("mish", "a"), ("y2only", "a"), ("aout_y2", "odd")],   # cin1: no res
    "noy2": [("plain", "a"), ("aout", "a"), ("tanh", "out1"), ("mish", "a"), ("aout", "odd")],               # narrow, thin: no res, no y2
    "y2": [("plain", "a"), ("y2", "a"), ("y2", "out1"), ("y2only", "a"), ("y2", "odd")],                                       # pwt: bias and alpha_y2 only
    "flat": [("plain", "a"), ("y2", "a"), ("aout_y2", "a"), ("tanh", "a"), ("y2only", "a")],                   # conv1d_flat: no res, no out
    "log_mel": [("log_mel", "a"), ("log_mel", "odd")],
}

# name; B, ci, co, T (T_out % 4 == 0), T_odd (T_out % 4 in {1, 3}); k, s, d, mode, causal; layout, rows (co tile of split taps);
# k1, dil2 (two-level taps); kern: substring of the kernel name; form: the epilogue code that runs (see FORMS); prologue: alpha_in;
# admits: key of ADMITS; pw_split: ops.PW_SPLIT during the case; flat: None or the flattened form; lowplane: rerun on the fp32 route
Base = namedtuple("Base", "name B ci co T T_odd k s d mode causal layout rows k1 dil2 kern form prologue admits pw_split flat lowplane")


def _b(name, B, ci, co, T, T_odd, k, s=1, d=1, mode=REFLECT, causal=True, layout=FP32, rows=64, k1=0, dil2=0, kern="", form="", prologue=False,
       admits="full", pw_split=True, flat=None, lowplane=False):
    return Base(name, B, ci, co, T, T_odd, k, s, d, mode, causal, layout, rows, k1, dil2, kern, form, prologue, admits, pw_split, flat, lowplane)


# The epilogue forms of the sources.  mfma_all_waves, gemm_split, bsplit2 and cin1 call the one quad epilogue of conv1d_epilogue.h
# (skinny and gemv its one-sample form) around gathers and address arithmetic of their own; bsplit (packed pairs), mfma_per_wave and
# the streaming and VALU kernels each keep theirs (conv1d_mfma.h has three forms; row_phases is tests/test_convtr_fwd.py's)
FORMS = {"mfma_per_wave", "mfma_all_waves", "bsplit", "bsplit2", "gemm_split", "pw", "pws", "pwt", "narrow", "thin", "cin1", "skinny", "gemv"}

BASES = [
    # ---- fp32 MFMA tiles, each without and with the prologue.  Per-wave epilogue (scalar stores) except the two 256-column
    # tiles, whose 8 MFMA waves hand the accumulators to all waves through LDS (ALLW: float4 or scalar by alignment and T_out % 4)
    _b("t128x32", 33, 40, 72, 20, 21, 1, kern="128x32", form="mfma_per_wave"),
    _b("t128x32_ain", 33, 40, 72, 20, 21, 1, kern="128x32", form="mfma_per_wave", prologue=True),
    _b("t32x256", 3, 24, 24, 220, 221, 3, d=2, kern="32x256", form="mfma_per_wave"),
    _b("t32x256_ain", 3, 24, 24, 220, 221, 3, d=2, causal=False, kern="32x256", form="mfma_per_wave", prologue=True),
    _b("t64x128", 2, 37, 45, 324, 325, 5, d=2, kern="64x128", form="mfma_per_wave"),
    _b("t64x128_ain", 2, 37, 45, 324, 325, 5, d=2, causal=False, kern="64x128", form="mfma_per_wave", prologue=True),
    _b("t96x128", 2, 40, 96, 324, 323, 5, kern="96x128", form="mfma_per_wave"),
    _b("t96x128_ain", 2, 40, 96, 324, 323, 5, mode=ZERO, kern="96x128", form="mfma_per_wave", prologue=True),
    _b("t128x128", 2, 130, 130, 324, 325, 3, kern="128x128", form="mfma_per_wave"),
    _b("t128x128_ain", 2, 130, 130, 324, 325, 3, causal=False, kern="128x128", form="mfma_per_wave", prologue=True),
    _b("t128x160", 5, 24, 72, 132, 133, 3, kern="128x160", form="mfma_per_wave"),              # 5 x 132 > 640 columns
    _b("t128x160_ain", 5, 24, 72, 132, 133, 3, kern="128x160", form="mfma_per_wave", prologue=True),
    _b("t96x256_ain", 2, 24, 96, 516, 517, 1, kern="96x256", form="mfma_all_waves", prologue=True),
    _b("t128x256_ain", 2, 24, 130, 516, 517, 1, kern="128x256", form="mfma_all_waves", prologue=True),
    # the same two tiles without the prologue: k = 1 with channel counts the streaming kernels do not take
    _b("t96x256", 2, 24, 96, 516, 517, 1, kern="96x256", form="mfma_all_waves"),
    _b("t128x256", 2, 24, 130, 516, 517, 1, kern="128x256", form="mfma_all_waves"),
    # ---- VALU kernels: each with the operands its predicate admits
    _b("narrow_ain", 128, 8, 2, 40, 41, 7, kern="narrow_kernel (VALU, C_out<=2)", form="narrow", prologue=True, admits="noy2"),
    _b("narrow_two_level", 128, 8, 2, 58, 59, 9, mode=ZERO, k1=3, dil2=8, kern="two-level", form="narrow", prologue=True, admits="noy2"),
    _b("thin_ain", 2, 130, 2, 100, 101, 7, kern="thin", form="thin", prologue=True, admits="noy2"),
    _b("thin_k2_co8", 2, 130, 8, 400, 401, 2, mode=ZERO, kern="thin", form="thin", admits="noy2"),
    _b("cin1", 256, 1, 5, 40, 41, 7, kern="cin1", form="cin1", admits="nores"),
    # ---- split reduction and single launch
    _b("skinny", 2, 40, 24, 100, 101, 5, kern="skinny", form="skinny"),
    _b("skinny_k1_tiles", 2, 24, 72, 320, 319, 1, kern="skinny", form="skinny"),      # 20 column blocks x 3 co tiles: no reduce kernel
    _b("gemv", 1, 24, 40, 4, 3, 1, kern="gemv", form="gemv"),
    # ---- split taps, every case above 640 columns: narrow-stage group (C_in < BS_WIDE_MIN = 64) and wide group, k = 3, 5, 7
    _b("taps_k7_narrow", 2, 32, 16, 324, 325, 7, layout=TAPS, kern="bsplit_kernel<7> 64x256", form="bsplit"),
    _b("taps_k5_narrow", 2, 32, 48, 324, 325, 5, d=3, causal=False, layout=TAPS, kern="bsplit_kernel<5> 64x256", form="bsplit"),
    _b("taps_k3_narrow", 2, 48, 48, 324, 323, 3, d=9, mode=ZERO, layout=TAPS, kern="bsplit_kernel<3> 64x256", form="bsplit"),
    _b("taps_k7_wide", 2, 64, 80, 324, 325, 7, d=9, layout=TAPS, kern="bsplit_kernel<7> 64x256", form="bsplit"),
    _b("taps_k5_wide", 2, 80, 48, 324, 323, 5, layout=TAPS, kern="bsplit_kernel<5> 64x256", form="bsplit"),
    _b("taps_k3_wide", 2, 64, 48, 324, 325, 3, causal=False, layout=TAPS, kern="bsplit_kernel<3> 64x256", form="bsplit"),
    _b("taps96", 2, 48, 96, 324, 325, 7, d=3, layout=TAPS, rows=96, kern="bsplit_kernel<7> 96x256", form="bsplit", lowplane=True),
    # ---- split GEMM
    _b("gemm_k1", 4, 256, 72, 260, 259, 1, layout=GEMM, kern="gemm_split_kernel<1>", form="gemm_split", lowplane=True),
    _b("gemm_k2", 4, 256, 64, 256, 257, 2, mode=ZERO, layout=GEMM, kern="gemm_split_kernel<2>", form="gemm_split", lowplane=True),
    _b("gemm_k4_s2", 4, 32, 64, 512, 513, 4, s=2, layout=GSTR, kern="gemm_split_kernel<2>", form="gemm_split", lowplane=True),   # T % s: 0 / 1
    _b("gemm_k10_s5", 4, 32, 72, 1300, 1283, 10, s=5, layout=GSTR, kern="gemm_split_kernel<2>", form="gemm_split", lowplane=True),  # T % s: 0 / 3
    _b("gemm_flat_strided", FLAT[5], FLAT[1], FLAT[0], FLAT[6], None, FLAT[2], s=FLAT[3], layout=GSTR, kern="gemm_split_kernel<2>",
       form="gemm_split", admits="flat", flat=convplan.FLAT_STRIDED, lowplane=True),
    _b("taps_flat_stride1", 4, 1024, 1024, 161, None, 7, layout=TAPS, kern="bsplit_kernel<7> 64x256", form="bsplit", admits="flat",
       flat=convplan.FLAT_STRIDE1),
    # ---- bsplit2: 8 <= C_out <= 32, zero padding, at least 4096 columns
    _b("split2_k9", 2, 8, 24, 2048, 2049, 9, mode=ZERO, layout=SPLIT2, kern="bsplit2_kernel<9,1>", form="bsplit2", lowplane=True),
    _b("split2_k9_s2", 2, 16, 32, 4096, 4098, 9, s=2, mode=ZERO, layout=SPLIT2, kern="bsplit2_kernel<9,2>", form="bsplit2", lowplane=True),
    _b("split2_k3", 2, 8, 8, 2048, 2049, 3, mode=ZERO, causal=False, layout=SPLIT2, kern="bsplit2_kernel<3,1>", form="bsplit2", lowplane=True),
    _b("split2_two_level", 2, 8, 32, 2100, 2101, 27, mode=ZERO, layout=SPLIT2, k1=9, dil2=20, kern="bsplit2_kernel<9,1>", form="bsplit2",
       lowplane=True),
    # ---- streaming kernels, at the smallest column count `items >= 2 * slots` admits (the one place where a case is large);
    # T % 32 != 0: the last column block is partial
    _b("pw_32to64", 16, 32, 64, 16356, 16353, 1, kern="pw_kernel", form="pw"),
    _b("pw_64to64", 16, 64, 64, 16356, 16353, 1, kern="pw_kernel", form="pw", pw_split=False),
    _b("pws_64", 16, 64, 64, 16356, 16353, 1, kern="pws", form="pws", lowplane=True),
    _b("pws_256", 16, 256, 256, 4068, 4065, 1, kern="pws", form="pws", lowplane=True),         # four weight slices of 64 rows per clip
    _b("pwt_k4_s2", 16, 16, 256, 6088, 6082, 4, s=2, layout=PWT, kern="pwt_kernel<4 taps>", form="pwt", admits="y2", lowplane=True),
    # ---- the mel front end's shape class (quantize.py, streaming.py): 1025 -> 80, k = 1, no bias, non-negative operands
    _b("log_mel_tile", 2, 1025, 80, 324, 325, 1, mode=ZERO, kern="128x128", form="mfma_per_wave", admits="log_mel"),
    _b("log_mel_skinny", 2, 1025, 80, 40, 41, 1, mode=ZERO, kern="skinny", form="skinny", admits="log_mel"),
    # ---- reflect padding not shorter than the signal (pad1d's zero extension), causal and non-causal, one per kernel family
    _b("short_tile_causal", 7, 37, 45, 52, 53, 7, d=9, kern="64x128", form="mfma_per_wave", prologue=True),       # T <= pad_left = 54
    _b("short_tile_noncausal", 9, 37, 45, 24, 27, 7, d=9, causal=False, kern="128x32", form="mfma_per_wave", prologue=True),   # T <= 27
    _b("short_skinny_causal", 2, 37, 45, 4, 5, 7, kern="skinny", form="skinny"),               # T <= pad_left = 6
    _b("short_skinny_noncausal", 2, 37, 45, 4, 3, 7, causal=False, kern="skinny", form="skinny"),    # pads 3 / 3; T = 4 is the ordinary edge
    _b("short_taps_causal", 13, 32, 16, 52, 53, 7, d=9, layout=TAPS, kern="bsplit_kernel<7> 64x256", form="bsplit"),
    _b("short_taps_noncausal", 27, 32, 16, 24, 27, 7, d=9, causal=False, layout=TAPS, kern="bsplit_kernel<7> 64x256", form="bsplit"),
    _b("short_narrow_causal", 128, 8, 2, 4, 5, 7, kern="narrow_kernel (VALU, C_out<=2)", form="narrow", prologue=True, admits="noy2"),
    _b("short_cin1_causal", 256, 1, 5, 4, 5, 7, kern="cin1", form="cin1", admits="nores"),
    _b("short_thin_noncausal", 2, 130, 2, 4, 3, 7, causal=False, kern="thin", form="thin", prologue=True, admits="noy2"),
]
BASE = {b.name: b for b in BASES}
assert len(BASE) == len(BASES)
assert {b.form for b in BASES} == FORMS

Case = namedtuple("Case", "id base T ops align")
CASES = [Case(f"{b.name}-{o}-{al}", b, b.T_odd if al == "odd" else b.T, OPS[o], al)
         for b in BASES for o, al in ADMITS[b.admits] if not (al == "odd" and b.T_odd is None)]
IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}

# fac::ConvKernel ids the table does not reach, with the reason (test_table_covers_every_forward_kernel)
EXCLUDED = {}           # (the fused ResidualUnit is reached by the RU list below: the composite bound, not the two-step check)
KERNEL_ID = {"128x32": "CK_128x32", "32x256": "CK_32x256", "64x128": "CK_64x128", "96x128": "CK_96x128", "128x128": "CK_128x128",
             "128x256": "CK_128x256", "96x256": "CK_96x256", "128x160": "CK_128x160", "narrow": "CK_NARROW", "skinny": "CK_SKINNY",
             "gemv": "CK_SKINNY", "64x256 (bf16x3": "CK_BSPLIT", "cin1": "CK_CIN1", "thin": "CK_THIN", "pw_kernel": "CK_PW",
             "gemm_split": "CK_GSPLIT", "bsplit2": "CK_BSPLIT2", "pws": "CK_PWS", "pwt": "CK_PWT", "96x256 (bf16x3": "CK_BSPLIT96"}


# ------------------------------------------------------------------------------------------------ geometry, descriptor
class _switches:
    """ops.PW_SPLIT as the case wants it (the pw kernel at C_in == C_out runs only with the plane kernel switched off)."""

    def __init__(self, b):
        self.want = b.pw_split

    def __enter__(self):
        self.old, ops.PW_SPLIT = ops.PW_SPLIT, self.want

    def __exit__(self, *exc):
        ops.PW_SPLIT = self.old
        return False


def _max_off(b):
    """Largest tap offset: tap kk = k2 * k1 + k1' reads k2 * dil2 + k1' * d (two-level), else kk * d."""
    if b.k1:
        return (b.k // b.k1 - 1) * b.dil2 + (b.k1 - 1) * b.d
    return (b.k - 1) * b.d


def _geometry(b, T):
    """(t_out, pad_left, pad_right) of the launch: the SConv1d rule (ops.conv_desc with pad_left=None), or no padding for the
    two-level and the flattened cases."""
    if b.k1 or b.flat:
        return T - _max_off(b), 0, 0
    d = ops.conv_desc(b.B, b.ci, T, b.co, b.k, b.s, b.d, None, b.mode, None, ops.ACT_NONE, b.causal)
    pr = max(0, (d.T_out - 1) * b.s + _max_off(b) + 1 - d.pad_left - T)
    return d.T_out, d.pad_left, pr


def _flat_geometry(b):
    """(L, n) of ops.conv1d_flat: every clip padded to L columns on the left as the site does, n outputs kept per clip."""
    if b.flat == convplan.FLAT_STRIDED:
        n = b.T // b.s
        return (n + 1) * b.s, n
    return b.T + (b.k - 1) * b.d, b.T


def _operand_names(c):
    o = c.ops
    return ((("bias",) if c.base.admits != "log_mel" else ()) + (("alpha_in",) if c.base.prologue else ()) + (("alpha_out",) if o.aout else ())
            + (("res",) if o.res else ()) + (("y2", "alpha_y2") if o.y2 else ()))


def _desc(c, layout=None):
    """The case's launch descriptor from the product's builders, pointers never dereferenced."""
    b = c.base
    layout = layout or b.layout
    kw = dict(rows=b.rows, operands=_operand_names(c))
    with _switches(b):
        if b.flat:
            L, n = _flat_geometry(b)
            d = flat_conv_launch(layout, b.B, b.ci, L, b.co, b.k, b.s, n, b.d, act=c.ops.act, **kw)
        elif b.k1:
            d = conv_launch(layout, b.B, b.ci, c.T, b.co, b.k, b.s, b.d, 0, b.mode, c.T - _max_off(b), c.ops.act, b.causal, k1=b.k1,
                            dilation2=b.dil2, **kw)
        else:
            d = conv_launch(layout, b.B, b.ci, c.T, b.co, b.k, b.s, b.d, None, b.mode, None, c.ops.act, b.causal, **kw)
    if not c.ops.want_y:
        d.y = None
    return d


def _is_split(b):
    return b.layout in SPLIT_LAYOUTS or b.form in ("pws", "pwt")


# ------------------------------------------------------------------------------------------------ references
def snake(x, alpha):
    """dac/nn/layers.py:18-24 in the dtype of x: x + sin^2(alpha x) / (alpha + 1e-9), alpha per channel."""
    a = alpha.to(x.dtype).view(1, -1, 1)
    return x + torch.sin(a * x) ** 2 / (a + 1e-9)


def act_ref(x, act):
    if act == ops.ACT_TANH:
        return torch.tanh(x)
    if act == ops.ACT_MISH:
        return x * torch.tanh(F.softplus(x))          # threshold 20, as the kernel's
    if act == ops.ACT_LOG_MEL:
        return (torch.log(1e-5 + x) + 4.0) / 4.0
    return x


def epilogue_ref(c, alpha_out, act, res, dtype):
    """res + act(snake(c, alpha_out)) in `dtype`: the documented order (facodec_hip.h: act applied last, before the residual)."""
    v = c.to(dtype)
    if alpha_out is not None:
        v = snake(v, alpha_out)
    v = act_ref(v, act)
    return v + res.to(dtype) if res is not None else v


def _dense_weight(b, w):
    """Two-level taps as a plain kernel of _max_off + 1 taps (zeros between), so that F.conv1d at dilation 1 is the reference."""
    if not b.k1:
        return w, b.d
    dense = torch.zeros(w.shape[0], w.shape[1], _max_off(b) + 1, dtype=w.dtype)
    for kk in range(b.k):
        dense[:, :, (kk // b.k1) * b.dil2 + (kk % b.k1) * b.d] = w[:, :, kk]
    return dense, 1


def conv_ref(b, T, x, w, bias, alpha_in=None):
    """(c64, mag): F.conv1d(_pad(snake64(x)), w64) + bias and the same conv over |w| and m_in plus |bias|.  x: the clips, or for
    a flattened case the already padded clips (then no padding, and the first n outputs of each clip)."""
    x, w = x.double(), w.double()
    m_in = x.abs()
    if alpha_in is not None:
        a = alpha_in.double().view(1, -1, 1)
        m_in = x.abs() + torch.sin(a * x) ** 2 / (a + 1e-9)
        x = snake(x, alpha_in)
    wd, dil = _dense_weight(b, w)
    if b.flat:
        n = _flat_geometry(b)[1]
        c64 = F.conv1d(x, wd, stride=b.s, dilation=dil)[..., :n]
        mag = F.conv1d(m_in, wd.abs(), stride=b.s, dilation=dil)[..., :n]
    else:
        t_out, pl, pr = _geometry(b, T)
        c64 = F.conv1d(_pad(x, pl, pr, b.mode), wd, stride=b.s, dilation=dil)[..., :t_out]
        mag = F.conv1d(_pad(m_in, pl, pr, b.mode), wd.abs(), stride=b.s, dilation=dil)[..., :t_out]
    if bias is not None:
        c64 = c64 + bias.double().view(1, -1, 1)
        mag = mag + bias.double().abs().view(1, -1, 1)
    return c64, mag


def _alpha(n, gen):
    """1 + 0.2 rand with the two planted channels: alpha = 1 exactly, and alpha = 1e-6 (its row is scaled by 1e6 by the caller)."""
    a = 1 + 0.2 * torch.rand(n, generator=gen)
    a[0] = 1.0
    if n > 1:
        a[1] = 1e-6
    return a


Inputs = namedtuple("Inputs", "x w bias alpha_in alpha_out alpha_y2 res")


def _inputs(b, T):
    gen = torch.Generator().manual_seed(4000 + 7 * BASES.index(b) + (T == b.T_odd))
    L = _flat_geometry(b)[0] if b.flat else T
    x = torch.randn(b.B, b.ci, L, generator=gen)
    w = torch.randn(b.co, b.ci, b.k, generator=gen) / (b.ci * b.k) ** 0.5
    bias = torch.randn(b.co, generator=gen) * 0.5
    alpha_in = alpha_out = alpha_y2 = None
    if b.admits == "log_mel":                        # power spectrum times mel filter bank: nothing negative, no bias
        x, w, bias = x.abs(), w.abs(), None
    if b.prologue:
        alpha_in = _alpha(b.ci, gen)
        x[:, 1] *= 1e6
        w[:, 1] *= 1e-6
    alpha_out, alpha_y2 = _alpha(b.co, gen), _alpha(b.co, gen)
    if b.co > 1 and b.admits != "log_mel":
        w[1] *= 1e6
    t_out = _flat_geometry(b)[1] if b.flat else _geometry(b, T)[0]
    res = torch.randn(b.B, b.co, t_out, generator=gen)
    return Inputs(x, w, bias, alpha_in, alpha_out, alpha_y2, res)


# ------------------------------------------------------------------------------------------------ CPU-only checks of the table
def test_table_names_the_kernel_of_every_case():
    """fac_conv1d_variant (host only) on the descriptor of every case: the kernel the table names, on bf16 planes exactly where the
    table says so.  For the split layouts convplan must give the table's layout at that shape.  The GPU test asserts the same name
    on the launch itself."""
    bad = []
    for c in CASES:
        kid, name = ops.conv_variant(_desc(c))
        if kid < 0 or c.base.kern not in name or ("bf16x3" in name) != _is_split(c.base):
            bad.append((c.id, kid, name))
    assert not bad, bad[:8]
    for b in BASES:
        t_out = _geometry(b, b.T)[0] if b.k1 else ops.conv_out_len(b.T, b.k, b.s, b.d)[0]
        if b.layout == GEMM and b.k == 2:                   # no stride-1 site plans k = 2 (the transposed convs do): the predicate alone
            assert convplan.gemm_split_ok(b.co, b.ci, 2, b.B * t_out, t_out), b.name
        elif b.layout in (TAPS, GEMM):
            flat = dict(flat_infer=True, flat_stride1=True, grad=False, causal_reflect=True) if b.flat else {}
            p = convplan.plan_conv(b.co, b.ci, b.k, b.s, b.d, b.B, b.T, t_out, c_out_mult16=False, floor_k=(), **flat)
            assert (p.layout, p.form) == (b.layout, b.flat or convplan.PER_CLIP), (b.name, p)
        elif b.layout == GSTR:
            flat = dict(flat_infer=True, grad=False, causal_reflect=True) if b.flat else {}
            p = convplan.plan_conv(b.co, b.ci, b.k, b.s, b.d, b.B, b.T, t_out, **flat)
            assert (p.layout, p.form) == (b.layout, b.flat or convplan.PER_CLIP), (b.name, p)
        elif b.layout == SPLIT2:
            assert convplan.plan_conv(b.co, b.ci, b.k, b.s, b.d, b.B, b.T, t_out, k1=b.k1, split2=True).layout == SPLIT2, b.name
        elif b.layout == PWT:
            assert convplan.plan_conv(b.co, b.ci, b.k, b.s, b.d, b.B, b.T, t_out).layout == PWT, b.name
    assert convplan.tile_rows(96, 48, 7) == 96 and BASE["taps96"].rows == 96          # the 96-row form is what the inference sites pack


def test_table_sits_on_the_thresholds_it_names():
    """Next to each threshold a case sits on, the neighbouring shape takes another kernel: the cases are the smallest their
    predicates admit (the kernel name is the requirement, the shape only the means)."""
    def name(bname, **change):
        b = BASE[bname]._replace(**change)
        return ops.conv_variant(_desc(Case("x", b, b.T, OPS["plain"], "a")))[1]

    assert "skinny" in name("t128x160", B=4)                          # 4 x 132 <= 640 columns: the split reduction takes it
    assert "128x128" in name("t128x160", T=164) and "128x32" in name("t128x32", T=32) and "128x32" not in name("t128x32", T=36)
    assert "96x128" in name("t96x256", T=508) and "128x128" in name("t128x256", T=508)
    assert "narrow" not in name("narrow_ain", B=127) and "cin1" not in name("cin1", B=255)
    assert "thin" not in name("thin_ain", ci=127) and "thin" not in name("thin_k2_co8", k=3)
    assert "gemv" not in name("gemv", T=5)
    assert "bsplit" not in name("taps_k7_narrow", T=320)              # 640 columns
    assert "gemm_split" not in name("gemm_k1", T=255) and "gemm_split" not in name("gemm_k2", T=255)
    assert "gemm_split" not in name("gemm_k4_s2", T=510) and "gemm_split" not in name("gemm_k10_s5", T=1275)
    assert "bsplit2" not in name("split2_k9", T=2047) and "bsplit2" not in name("split2_k3", co=7)
    assert "pw_kernel" not in name("pw_32to64", T=16352) and "pw_kernel" in name("pw_32to64", T=16353)
    assert "pws" not in name("pws_64", T=16352) and "pws" not in name("pws_256", T=4064)      # conv_pw_ok's floor, the larger of the two
    assert "pwt" not in name("pwt_k4_s2", T=6080)
    assert "pws" in name("pw_64to64", pw_split=True)                  # what the switch is for
    # the flattened stride-1 form at the smallest shape plan_conv admits: 4 clips, 2^20 weights per tap, more than 640 columns
    b = BASE["taps_flat_stride1"]
    kw = dict(c_out_mult16=False, floor_k=(), flat_infer=True, flat_stride1=True, grad=False, causal_reflect=True)
    assert convplan.plan_conv(b.co, b.ci, 7, 1, 1, 4, 161, 161, **kw).form == convplan.FLAT_STRIDE1
    for co, ci, B, T in ((b.co // 2, b.ci, 4, 161), (b.co, b.ci, 3, 220), (b.co, b.ci, 4, 160)):
        assert convplan.plan_conv(co, ci, 7, 1, 1, B, T, T, **kw).form == convplan.PER_CLIP, (co, ci, B, T)


def test_table_has_every_variant_the_issue_lists():
    for b in BASES:
        got = {(o, al) for o, al in ADMITS[b.admits]}
        if b.admits == "full":
            assert {o for o, _ in got} >= {"full", "tanh_res", "mish", "y2only", "inplace", "plain"}
            assert {al for _, al in got} == {"a", "odd", "res1", "out1"}
        t_out, t_odd = _geometry(b, b.T)[0], (_geometry(b, b.T_odd)[0] if b.T_odd else None)
        assert t_out % 4 == 0 or b.flat, (b.name, t_out)
        assert t_odd is None or t_odd % 4 in (1, 3), (b.name, t_odd)
    for form in FORMS - {"pwt", "narrow", "thin", "cin1"}:                # every form that admits the full epilogue has the four alignments
        assert any(b.form == form and b.admits == "full" for b in BASES), form
    strided = [b for b in BASES if b.layout == GSTR and not b.flat]
    assert {b.k for b in strided} == {4, 10} and all(b.T % b.s == 0 and b.T_odd % b.s != 0 for b in strided)
    assert {b.form for b in BASES if b.mode == REFLECT and not b.k1} >= {"mfma_per_wave", "mfma_all_waves", "bsplit", "skinny", "gemv", "narrow", "thin",
                                                                          "pw", "pws", "gemm_split", "cin1"}
    short = [b for b in BASES if b.name.startswith("short_")]
    for b in short:
        _, pl, pr = _geometry(b, b.T_odd)
        assert b.mode == REFLECT and b.T_odd <= max(pl, pr), b.name
    assert {(b.form, b.causal) for b in short} >= {(f, cz) for f in ("mfma_per_wave", "skinny", "bsplit") for cz in (True, False)}
    for b in BASES:
        if b.form in ("pw", "pws", "pwt"):
            assert _geometry(b, b.T)[0] % 32 != 0 and _geometry(b, b.T_odd)[0] % 32 != 0, b.name


def test_table_covers_every_forward_kernel():
    """fac::ConvKernel of conv1d_api.hip: the ids the table reaches plus EXCLUDED are the enum, so a kernel added later fails here
    until it has a case."""
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "conv1d_api.hip")).read()
    body = re.search(r"enum ConvKernel : int \{(.*?)\};", src, re.S).group(1)
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"(CK_\w+)\s*=\s*(\d+)", body)}
    assert len(enum) >= 20 and sorted(enum.values()) == list(range(len(enum)))
    reached = set()
    for c in CASES:
        kid, name = ops.conv_variant(_desc(c))
        key = [k for k in KERNEL_ID if k in name]
        assert len(key) >= 1, name
        ident = KERNEL_ID[max(key, key=len)]
        assert enum[ident] == kid, (c.id, name, ident, kid)
        reached.add(ident)
    for C, d, T in RU:
        kid, name = ops.conv_variant(_ru_desc(C, d, 2, T))
        assert "fused RU" in name and enum["CK_FUSED_RU"] == kid
        reached.add("CK_FUSED_RU")
    assert not (reached & set(EXCLUDED)) and reached | set(EXCLUDED) == set(enum), (set(enum) - reached - set(EXCLUDED), reached & set(EXCLUDED))


@pytest.mark.parametrize("bname,T", [("t64x128_ain", 325), ("short_skinny_noncausal", 3), ("gemm_k10_s5", 1283)])
def test_references_agree_with_the_fp32_oracle(bname, T):
    """conv_ref / snake / epilogue_ref against oracle.facodec_oracle (sconv1d, snake: fp32) to 1e-5 of the largest value, one case
    with the prologue, one with T <= pad and one strided with T % s != 0."""
    from oracle import facodec_oracle as O
    b = BASE[bname]._replace(B=2, ci=6, co=4)
    gen = torch.Generator().manual_seed(5)
    x, w, bias = torch.randn(2, 6, T, generator=gen), torch.randn(4, 6, b.k, generator=gen), torch.randn(4, generator=gen)
    a_in, a_out = 1 + 0.2 * torch.rand(6, generator=gen), 1 + 0.2 * torch.rand(4, generator=gen)
    c64, _ = conv_ref(b, T, x, w, bias, a_in if b.prologue else None)
    xin = O.snake(x, a_in.view(1, -1, 1)) if b.prologue else x
    want = O.sconv1d(xin, w, bias, stride=b.s, dilation=b.d, causal=b.causal, pad_mode="reflect" if b.mode == REFLECT else "constant")
    assert want.shape == c64.shape
    assert float((c64 - want.double()).abs().max()) <= 1e-5 * float(want.abs().max())
    r64 = epilogue_ref(c64, a_out, ops.ACT_NONE, None, torch.float64)
    want = O.snake(want, a_out.view(1, -1, 1))
    assert float((r64 - want.double()).abs().max()) <= 1e-5 * float(want.abs().max())


# ------------------------------------------------------------------------------------------------ Step B, on the CPU: the self-check
def _emulate(c32, alpha_out, act, res, alpha_y2, fault=None):
    """fp32 CPU emulation of the epilogue order from the sum: snake -> act -> + res -> y2, with one planted fault."""
    def sn(v, a, inv_plain=False):
        a = a.view(1, -1, 1)
        return v + torch.sin(a * v) ** 2 * (1.0 / a if inv_plain else 1.0 / (a + 1e-9))

    a_out = torch.roll(alpha_out, 1) if fault == "alpha_shift" else alpha_out
    if fault == "res_first":
        y = act_ref(sn(c32 + res, a_out), act)
    else:
        pre = act_ref(sn(c32, a_out, inv_plain=fault == "inv_plain"), act)
        y = pre + res
    y2 = sn(pre if fault == "y2_before_res" else y, alpha_y2)
    return y, y2


def _step_b_bars(name, c32, y, y2, alpha_out, act, res, alpha_y2):
    """Step B's two bars for outputs (y, y2) of the pre-activation c32."""
    r64 = epilogue_ref(c32, alpha_out, act, res, torch.float64)
    r32 = epilogue_ref(c32, alpha_out, act, res, torch.float32)
    _bar(f"{name}_y", y, r64, r32, scale=_channel_scale(r64))
    y2_64, y2_32 = snake(y.double(), alpha_y2), snake(y, alpha_y2)
    _bar(f"{name}_y2", y2, y2_64, y2_32, scale=_channel_scale(y2_64))


def _channel_scale(r64):
    return r64.abs().amax(dim=(0, 2), keepdim=True).expand_as(r64)


@pytest.mark.parametrize("act", [ops.ACT_NONE, ops.ACT_TANH], ids=["snake", "tanh"])
def test_step_b_catches_planted_faults(act, monkeypatch):
    """The unfaulted fp32 emulation passes Step B's bar on the planted-channel inputs; each planted fault fails it."""
    import test_train_kernels_gen as G
    monkeypatch.setattr(G, "_record", lambda *a: None)          # nothing measured on a GPU here: keep it out of the tolerance report
    gen = torch.Generator().manual_seed(9)
    B, C, T = 2, 6, 40
    c32 = torch.randn(B, C, T, generator=gen)
    c32[:, 1] *= 1e6                                            # the channel whose alpha is 1e-6
    res = torch.randn(B, C, T, generator=gen)
    alpha_out, alpha_y2 = _alpha(C, gen), _alpha(C, gen)
    args = (alpha_out, act, res, alpha_y2)
    y, y2 = _emulate(c32, *args)
    _step_b_bars("selfcheck", c32, y, y2, *args)
    for fault in ("res_first", "y2_before_res", "alpha_shift", "inv_plain"):
        if fault == "inv_plain" and act == ops.ACT_TANH:
            continue                                           # tanh saturates the only channel where the 1e-9 shows
        y, y2 = _emulate(c32, *args, fault=fault)
        with pytest.raises(AssertionError):
            _step_b_bars("selfcheck_" + fault, c32, y, y2, *args)
    if act == ops.ACT_TANH:
        return                                                 # |y| <= 2 there: alpha_y2 * y = 1e-6 hides the 1e-9 in y2 as well
    # 1 / alpha in the y2 Snake alone
    y, _ = _emulate(c32, *args)
    a2 = alpha_y2.view(1, -1, 1)
    with pytest.raises(AssertionError):
        _step_b_bars("selfcheck_inv_plain_y2", c32, y, y + torch.sin(a2 * y) ** 2 / a2, *args)


def test_y2_p8_is_refused():
    """conv_plan refuses every descriptor that sets y2_p8 (no kernel writes it): a negative code and its message, on a split-taps
    launch, a split-GEMM launch and an fp32 launch."""
    lib = _lib.load()
    for bname in ("taps_k7_wide", "gemm_k1", "t64x128"):
        c = BY_ID[bname + "-full-a"]
        d = _desc(c)
        assert ops.conv_variant(d)[0] >= 0
        fake_operands(d, "y2_p8")
        d.y2_p8_plane_bytes = 1 << 20
        kid, name = ops.conv_variant(d)
        assert kid < 0 and name == "", (bname, kid, name)
        msg = lib.fac_last_error().decode()
        assert "P8 operands given but the launch does not run on a kernel that takes them" in msg, msg
        d.y2 = d.alpha_y2 = None                              # y2_p8 as the only second output
        assert ops.conv_variant(d)[0] < 0 and "y2_p8 needs alpha_y2" in lib.fac_last_error().decode()


# ------------------------------------------------------------------------------------------------ the GPU test
def _pack(b, w, dev, layout=None):
    layout = layout or b.layout
    if layout == TAPS:
        return None, ops.pack_conv_weight_split(w.to(dev), rows=b.rows)
    return ops.pack_conv_for(layout, w.to(dev), None, stride=b.s, k1=b.k1)


def _buffer(shape, dev, off):
    """An output inside a canary buffer, `off` floats past a 16-byte boundary: (view, buffer, first, n)."""
    if off == 0:
        view, buf, pad = _canary(shape, dev)
        return view, buf, pad, view.numel()
    n = math.prod(shape)
    buf = torch.full((n + 132,), CANARY, device=dev)
    return buf[64 + off:64 + off + n].view(*shape), buf, 64 + off, n


def _intact(buf, first, n):
    c = buf.cpu()
    if first == 64 and c.numel() == n + 128:
        assert _canary_intact(buf, 64)
    return bool((c[:first] == CANARY).all()) and bool((c[first + n:] == CANARY).all())


def _launch(b, T, dev, packs, inp, o, align="a", alpha_in=True):
    """One launch of the case's conv with the operand set `o` -> (y, y2) on the CPU, as the product calls it.  The output handed to
    ops.conv1d sits in a canary buffer, which is checked."""
    wp, ws = packs
    bias = inp.bias.to(dev) if inp.bias is not None else None
    kw = dict(bias=bias, alpha_out=inp.alpha_out.to(dev) if o.aout else None, act=o.act,
              alpha_y2=inp.alpha_y2.to(dev) if o.y2 else None, want_y=o.want_y)
    if b.flat:
        _, n = _flat_geometry(b)
        if wp is not None:       # the fp32 route of a flattened case (ops.conv1d_flat is split-only): the padded clips one by one
            got = ops.conv1d(inp.x.to(dev), wp, b.co, b.k, stride=b.s, dilation=b.d, pad_left=0, pad_mode=ZERO, t_out=n, **kw)
        else:
            got = ops.conv1d_flat(inp.x.to(dev), ws, b.co, b.k, b.s, n, dilation=b.d, **kw)
        y, y2 = got if o.y2 else (got, None)
        return (y.cpu() if y is not None else None), (y2.cpu() if y2 is not None else None)
    t_out, pl, _ = _geometry(b, T)
    shape = (b.B, b.co, t_out)
    out = buf = None
    if o.want_y:
        out, buf, first, n = _buffer(shape, dev, 1 if align == "out1" else 0)
    res = None
    if o.res == "out":
        out.copy_(inp.res.to(dev))
        res = out
    elif o.res:
        if align == "res1":
            res = torch.empty(math.prod(shape) + 1, device=dev)[1:].view(*shape)
            res.copy_(inp.res.to(dev))
            assert res.data_ptr() % 16 == 4
        else:
            res = inp.res.to(dev)
    geo = dict(pad_left=0, t_out=t_out, k1=b.k1, dilation2=b.dil2) if b.k1 else {}
    got = ops.conv1d(inp.x.to(dev), wp, b.co, b.k, stride=b.s, dilation=b.d, pad_mode=b.mode, causal=b.causal,
                     alpha_in=inp.alpha_in.to(dev) if (b.prologue and alpha_in) else None, res=res, out=out, w_split=ws, **geo, **kw)
    torch.cuda.synchronize()
    y, y2 = got if o.y2 else (got, None)
    if o.want_y:
        assert y.data_ptr() == out.data_ptr() and _intact(buf, first, n), "canary"
        assert not bool((y == CANARY).any())
    else:
        assert y is None
    if y2 is not None:
        assert y2.shape == shape and not bool((y2 == CANARY).any())
    return (y.cpu() if y is not None else None), (y2.cpu() if y2 is not None else None)


@functools.lru_cache(maxsize=4)
def _step_a(bname, T):
    """Step A of a (base, length), once for all its variants: inputs, packed weights, c_gpu, the kernel's name; c_gpu is held to
    float64 here."""
    b = BASE[bname]
    dev = torch.device("cuda:0")
    inp = _inputs(b, T)
    with _switches(b):
        packs = _pack(b, inp.w, dev)
        with _Spy() as spy:
            c_gpu, _ = _launch(b, T, dev, packs, inp, OPS["plain"])
    assert len(spy.launched) == 1
    name = ops.conv_variant(spy.launched[0])[1]
    assert b.kern in name and ("bf16x3" in name) == _is_split(b), (name, b.kern)
    c64, mag = conv_ref(b, T, inp.x, inp.w, inp.bias, inp.alpha_in)
    assert c_gpu.shape == c64.shape
    extra = (3.0 if _is_split(b) else 0.0) + (7.0 if b.prologue else 0.0)
    _sum_bound(f"conv_fwd_sum_{bname}_T{T}", c_gpu, c64, mag, b.ci * b.k, extra=extra)
    if b.lowplane:
        try:
            ops.BF16_SPLIT = False
            with _switches(b), _Spy() as spy32:
                base, _ = _launch(b, T, dev, _pack(b, inp.w, dev, FP32), inp, OPS["plain"])
        finally:
            ops.BF16_SPLIT = True
        assert len(spy32.launched) == 1 and "bf16x3" not in ops.conv_variant(spy32.launched[0])[1]
        scale = float(c64.abs().max())
        e_split, e_fp32 = float((c_gpu.double() - c64).abs().max()) / scale, float((base.double() - c64).abs().max()) / scale
        _record(f"conv_fwd_{bname}_T{T}_split_vs_fp32", {"split": e_split, "fp32": e_fp32})
        print(f"[tol] conv_fwd_{bname}_T{T}: split {e_split:.3e} fp32 {e_fp32:.3e}")
        assert e_split <= 1.5 * e_fp32 + 1e-7, (e_split, e_fp32)
    return inp, packs, c_gpu, name


@gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("cid", IDS)
def test_conv_fwd_epilogue_against_fp64(cid, cuda):
    c = BY_ID[cid]
    b, o = c.base, c.ops
    assert ops.BF16_SPLIT
    inp, packs, c_gpu, plain_name = _step_a(b.name, c.T)
    if o == OPS["plain"]:
        return                                                  # Step A alone (canary and name included)
    with _switches(b), _Spy() as spy:
        y, y2 = _launch(b, c.T, cuda, packs, inp, o, c.align)
    assert len(spy.launched) == 1
    name = ops.conv_variant(spy.launched[0])[1]
    assert name == plain_name and b.kern in name, (name, plain_name)
    assert_same_launch(spy.launched[0], _desc(c), cid)          # the descriptor the CPU tests of the table judge is the one launched
    alpha_out = inp.alpha_out if o.aout else None
    res = inp.res if o.res else None
    if not o.want_y:                                            # y2 alone: the same bits as beside y, which Step B then judges
        with _switches(b):
            y, y2_beside = _launch(b, c.T, cuda, packs, inp, o._replace(want_y=True), c.align)
        assert torch.equal(y2, y2_beside)
    if o == OPS["y2"]:
        assert torch.equal(y, c_gpu), "the launch with alpha_y2 does not share the plain launch's accumulator bits"
    r64 = epilogue_ref(c_gpu, alpha_out, o.act, res, torch.float64)
    r32 = epilogue_ref(c_gpu, alpha_out, o.act, res, torch.float32)
    _bar(f"conv_fwd_map_{cid}_y", y, r64, r32, scale=_channel_scale(r64))
    if o.y2:
        y2_64 = snake(y.double(), inp.alpha_y2)
        _bar(f"conv_fwd_map_{cid}_y2", y2, y2_64, snake(y, inp.alpha_y2), scale=_channel_scale(y2_64))


# ------------------------------------------------------------------------------------------------ ragged flattened quads
@functools.lru_cache(maxsize=1)
def _ragged_flat_inputs():
    """The shape of test_gemm_split_p8_fragments.test_k1_flattened: K = 1, B 3, C_in 72 (ragged last chunk), C_out 136, T 347 =
    1 041 flattened columns, T % 4 = 3: quads straddle the clip boundaries and the last tile is ragged.  (inputs, c64, mag)."""
    B, ci, co, T = 3, 72, 136, 347
    gen = torch.Generator().manual_seed(4700)
    x = torch.randn(B, ci, T, generator=gen)
    w = torch.randn(co, ci, 1, generator=gen) / ci ** 0.5
    bias = torch.randn(co, generator=gen) * 0.5
    alpha_out, alpha_y2 = _alpha(co, gen), _alpha(co, gen)
    w[1] *= 1e6                                                 # the row whose alphas are 1e-6
    res = torch.randn(B, co, T, generator=gen)
    c64 = F.conv1d(x.double(), w.double()) + bias.double().view(1, -1, 1)
    mag = F.conv1d(x.double().abs(), w.double().abs()) + bias.double().abs().view(1, -1, 1)
    return Inputs(x, w, bias, None, alpha_out, alpha_y2, res), c64, mag


@gpu
@pytest.mark.parametrize("cols,tile", [(-1, " 128x128 "), (128, " 64x128 ")], ids=["128x128", "64x128"])
def test_ragged_flattened_quads_against_fp64(cols, tile, cuda, monkeypatch):
    """The sample-by-sample branch of the two split-GEMM forms (flattened quads that end inside a clip) against float64, on P8 planes:
    the 128 x 128 form and the 64 x 128 form, whose row ownership mask is live at 136 rows.  Both forms call one helper
    (conv1d_epilogue.h), so their equality (test_gemm_split_p8_fragments) says nothing about it.  Step A and Step B as above."""
    inp, c64, mag = _ragged_flat_inputs()
    co, ci = inp.w.shape[0], inp.w.shape[1]
    T = inp.x.shape[-1]
    assert T % 4 == 3
    monkeypatch.setattr(ops, "GSPLIT_P8_COLS", cols)
    ws = ops.pack_gemm_weight_split(inp.w.to(cuda))
    p8 = ops.to_p8(inp.x.to(cuda))

    def launch(o):
        with _Spy() as spy:
            got = ops.conv1d(p8, None, co, 1, pad_left=0, pad_mode=ZERO, t_out=T, w_split=ws, bias=inp.bias.to(cuda),
                             alpha_out=inp.alpha_out.to(cuda) if o.aout else None, act=o.act, res=inp.res.to(cuda) if o.res else None,
                             alpha_y2=inp.alpha_y2.to(cuda) if o.y2 else None)
            torch.cuda.synchronize()
        assert len(spy.launched) == 1
        name = ops.conv_variant(spy.launched[0])[1]
        assert "conv1d_gemm_split_kernel<1>" in name and tile in name, name
        y, y2 = got if o.y2 else (got, None)
        return y.cpu(), (y2.cpu() if y2 is not None else None)

    c_gpu, _ = launch(OPS["plain"])
    assert c_gpu.shape == c64.shape
    _sum_bound(f"conv_fwd_sum_ragged_flat_{cols}", c_gpu, c64, mag, ci, extra=3.0)
    y, _ = launch(OPS["y2"])
    assert torch.equal(y, c_gpu), "the launch with alpha_y2 does not share the plain launch's accumulator bits"
    for oname in ("full", "tanh_res"):
        o = OPS[oname]
        y, y2 = launch(o)
        alpha_out = inp.alpha_out if o.aout else None
        r64 = epilogue_ref(c_gpu, alpha_out, o.act, inp.res, torch.float64)
        r32 = epilogue_ref(c_gpu, alpha_out, o.act, inp.res, torch.float32)
        _bar(f"conv_fwd_map_ragged_flat_{cols}_{oname}_y", y, r64, r32, scale=_channel_scale(r64))
        if o.y2:
            y2_64 = snake(y.double(), inp.alpha_y2)
            _bar(f"conv_fwd_map_ragged_flat_{cols}_{oname}_y2", y2, y2_64, snake(y, inp.alpha_y2), scale=_channel_scale(y2_64))


# ------------------------------------------------------------------------------------------------ fused ResidualUnit
RU = [(C, d, T) for C in (64, 96, 128) for d, T in ((1, 132), (9, 133))]


def _ru_desc(C, d, B, T, y2=True):
    dd = conv_launch(FP32, B, C, T, C, 7, 1, d, None, REFLECT, None, ops.ACT_NONE, True, c_out_pad=C,
                     operands=("bias", "alpha_out", "res", "w_k1", "bias_k1") + (("y2", "alpha_y2") if y2 else ()))
    return dd


def test_fused_residual_unit_cases_name_the_fused_kernel():
    for C, d, T in RU:
        kid, name = ops.conv_variant(_ru_desc(C, d, 2, T))
        assert kid == 7 and "fused RU" in name, (C, d, name)


@gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("C,d,T", RU)
def test_fused_residual_unit(C, d, T, cuda):
    """y = W1 snake(conv7(x) + b7, alpha) + b1 + res and y2 = snake(y, alpha_y2) in one launch (reflect padding, causal), held to
    the composite bound because h = snake(c) never leaves the registers:
      e_c  the Step A bound of c = conv7 + b7 (n = 7 C);
      e_h  = 2 e_c + 4 * 2^-24 (|c| + sin^2(alpha c) / alpha): Snake is 2-Lipschitz, plus the map's own roundings;
      e_y  = |W1| e_h + (4 sqrt(C) 2^-24 (|W1| |h64| + |b1|)) + 4 * 2^-24 |y64|: e_h through the 1x1 conv, the 1x1 conv's own
             `_sum_bound` terms (n = C), the residual add.
    y2 is a map of the kernel's own y: Step B's bar."""
    B = 2
    gen = torch.Generator().manual_seed(C + d)
    x = torch.randn(B, C, T, generator=gen)
    w7 = torch.randn(C, C, 7, generator=gen) / (7 * C) ** 0.5
    w1 = torch.randn(C, C, 1, generator=gen) / C ** 0.5
    b7, b1 = torch.randn(C, generator=gen) * 0.5, torch.randn(C, generator=gen) * 0.5
    alpha = 1 + 0.2 * torch.rand(C, generator=gen)
    alpha[0] = 1.0
    alpha_y2 = _alpha(C, gen)
    w1[1] *= 1e6                                                # the row whose alpha_y2 is 1e-6
    res = torch.randn(B, C, T, generator=gen)
    pl = 6 * d
    c64 = F.conv1d(_pad(x.double(), pl, 0, REFLECT), w7.double(), dilation=d) + b7.double().view(1, -1, 1)
    cmag = F.conv1d(_pad(x.double().abs(), pl, 0, REFLECT), w7.double().abs(), dilation=d) + b7.double().abs().view(1, -1, 1)
    a = alpha.double().view(1, -1, 1)
    e_c = 4 * math.sqrt(7 * C) * EPS32 * cmag + 4 * EPS32 * c64.abs()
    h64 = snake(c64, alpha)
    e_h = 2 * e_c + 4 * EPS32 * (c64.abs() + torch.sin(a * c64) ** 2 / a)
    W1 = w1.double()
    y64 = F.conv1d(h64, W1) + b1.double().view(1, -1, 1) + res.double()
    ymag = F.conv1d(h64.abs(), W1.abs()) + b1.double().abs().view(1, -1, 1)
    bound = F.conv1d(e_h, W1.abs()) + 4 * math.sqrt(C) * EPS32 * ymag + 4 * EPS32 * y64.abs()
    out, buf, first, n = _buffer((B, C, T), cuda, 0)
    wp7, wp1 = ops.pack_conv_weight(w7.to(cuda)), ops.pack_conv_weight(w1.to(cuda))
    with _Spy() as spy:
        y, y2 = ops.conv1d(x.to(cuda), wp7, C, 7, bias=b7.to(cuda), dilation=d, alpha_out=alpha.to(cuda), res=res.to(cuda), w_k1=wp1,
                           bias_k1=b1.to(cuda), alpha_y2=alpha_y2.to(cuda), out=out, causal=True)
        torch.cuda.synchronize()
    assert len(spy.launched) == 1 and "fused RU" in ops.conv_variant(spy.launched[0])[1]
    assert_same_launch(spy.launched[0], _ru_desc(C, d, B, T), (C, d))
    assert _intact(buf, first, n) and not bool((y == CANARY).any()) and not bool((y2 == CANARY).any())
    y, y2 = y.cpu(), y2.cpu()
    ratio = float(((y.double() - y64).abs() / bound).max())
    _record(f"conv_fwd_fused_ru_C{C}_d{d}", {"gpu_over_bound": ratio})
    print(f"[tol] conv_fwd_fused_ru_C{C}_d{d}: error / bound {ratio:.3e}")
    assert ratio <= 1.0, ratio
    y2_64 = snake(y.double(), alpha_y2)
    _bar(f"conv_fwd_fused_ru_C{C}_d{d}_y2", y2, y2_64, snake(y, alpha_y2), scale=_channel_scale(y2_64))
    # y2 alone: the same bits
    _, y2_only = ops.conv1d(x.to(cuda), wp7, C, 7, bias=b7.to(cuda), dilation=d, alpha_out=alpha.to(cuda), res=res.to(cuda), w_k1=wp1,
                            bias_k1=b1.to(cuda), alpha_y2=alpha_y2.to(cuda), want_y=False, causal=True)
    assert torch.equal(y2_only.cpu(), y2)
