"""The conv data gradient (ops.conv1d_bwd_data, the dx of ops.conv_transpose1d_bwd) against float64, route by route and fold by fold.

One table (CASES) names, for every case, the plan convplan must give, the kernel fac_conv1d_variant must name and whether the launch
is one flattened signal; the CPU-only tests walk it without a GPU, the GPU test runs it.

Reference: float64 torch autograd on the CPU through an explicit pad (`_pad` of tests/test_wgrad_split.py: pad1d of
dac/model/encodec.py:96-113, zero extension of signals not longer than the pad included) and F.conv1d / F.conv_transpose1d, from
the same fp32 inputs.  The weights it convolves are the fp32 numbers the kernel convolves: with weight norm, fl32(v * scale) with
the scale read back from ops.wn_scale (every packer of this path multiplies v by the scale once, in fp32, before it packs or
splits: pack.hip, conv1d_bwd.hip, conv1d_gemm_split.hip, conv1d_bsplit.hip), so the rounding of the scale is charged to
test_wn_scale_fp64 and not to the conv.  `mag` is the same gradient from |dy| and |w|: the per-element sum of absolute terms.

Bound, at every output element:  |dx - ref64| <= (4 sqrt(n) + extra) 2^-24 mag + 4 * 2^-24 |ref64|   (`_sum_bound`, c = 4)
  n      products per output: C_out K (stride 1), C_out 2 (strided, k = 2 s: two taps per output phase), C_out 2 s for the dx of a
         transposed conv (a strided conv over all its taps);
  extra  0 on the fp32 routes; 3 on the split-bf16 routes (three 8-bit planes hold an fp32 value exactly, the kernels drop the
         products mid * lo, lo * mid and lo * lo, each at most 2^-24 of its term).  No route of this path applies the weight-norm
         scale inside the conv kernel (see above), so the further + 1 of such a kernel is charged nowhere.
A lost low plane hides under 4 sqrt(n): every split case runs again with ops.BF16_SPLIT = False and must stay within
1.5 x the fp32 route's error + 1e-7 (max error over max |ref64|, the bar of test_split_bf16_conv_matches_fp32_grade).
"""
# Measured on MI355X, worst error / bound of each route over its cases (every route is under 4 sqrt(n); none needed the rigorous
# (n + extra) 2^-24 mag ceiling):
#   conv1d_bwd_data, stride 1   split taps k = 7 0.066, k = 5 0.049, k = 3 0.057; transposed split GEMM 0.064; streaming plane
#                               kernel (256 / 384 tails) 0.080; fp32 pack: 64x128 0.190, 96x128 0.086, 128x128 0.093, 128x32 0.146,
#                               32x256 0.030, split reduction 0.033, single launch 0.042, narrow 0.025, thin 0.035, cin1 0.208
#   conv1d_bwd_data, strided    polyphase: split reduction 0.040, single launch 0.044, 32x256 0.135; all-phases split GEMM 0.093;
#                               streaming kernel with taps 0.165; flattened clips 0.097
#   conv_transpose1d_bwd dx     fp32: split reduction 0.016, 64x128 0.084; strided split GEMM 0.054; streaming kernel with taps 0.128;
#                               flattened clips 0.044
#   the forward of the short reflect cases 0.015; wn_scale 0.132
# Split against fp32 route (max error / max |ref64|), worst pair: 4.8e-7 against 3.9e-7 (all-phases split GEMM, s = 2); over the
# 31 split cases the split route's error is 1.4e-7 .. 7.5e-7, the fp32 route's 1.7e-7 .. 9.2e-7.
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

from facodec_amd import convplan, ops
from test_conv_plan_cpu import assert_same_launch, bwd_data_launch, convtr_bwd_launch
from test_train_kernels_gen import CANARY, _check_adjoint, _record, _sum_bound
from test_wgrad_split import _pad

gpu = pytest.mark.gpu
REFLECT, ZERO = ops.PAD_REFLECT, ops.PAD_ZERO

# kind: "s1" / "st" -- ops.conv1d_bwd_data at stride 1 / strided (ci -> co is the FORWARD conv); "tr" -- the dx of
# ops.conv_transpose1d_bwd (ci -> co is the transposed conv, T its input length).  layout / form: the plan of the launch; kern: a
# substring of the kernel's name; flat: the launch is one flattened signal (B == 1); split: the kernel runs on bf16 planes.
Case = namedtuple("Case", "name kind B ci co T k s d mode causal wn layout form kern flat split")


def _c(name, kind, B, ci, co, T, k=None, s=1, d=1, mode=REFLECT, causal=True, wn=True, layout=convplan.W_FP32, form=convplan.PER_CLIP,
       kern="", flat=False, split=None):
    if split is None:
        split = layout not in (convplan.W_FP32, convplan.TR_POLYPHASE, convplan.TR_ROWS)
    return Case(name, kind, B, ci, co, T, 2 * s if k is None else k, s, d, mode, causal, wn, layout, form if kind != "st" else None, kern,
                flat, split)


TAPS, GEMM, GSTR, FP32, PWT = convplan.W_TAPS, convplan.W_GEMM, convplan.W_GEMM_STRIDED, convplan.W_FP32, convplan.W_FP32_PW_TAPS
POLY, RSPLIT, RPWT, TFLAT = convplan.TR_POLYPHASE, convplan.TR_ROWS_SPLIT, convplan.TR_ROWS_PW_TAPS, convplan.TR_FLAT

CASES = [
    # ---- stride 1, flipped split taps (the gradient conv has the channels swapped: rows = forward C_in, 64-row tiles, 256-column
    # tiles; B * tp just above the 640-column floor).  k = 3 / 5 need (floor_k) 64 input channels and more than 32 rows of the
    # GRADIENT conv: forward 48 -> 64 is the smallest that qualifies, forward 64 -> 48 the mirror image that must stay on fp32.
    _c("taps_k7_d1_32to16_causal", "s1", 2, 32, 16, 315, 7, d=1, layout=TAPS, kern="bsplit_kernel<7>"),
    _c("taps_k5_d3_48to64_noncausal", "s1", 2, 48, 64, 309, 5, d=3, causal=False, layout=TAPS, kern="bsplit_kernel<5>"),
    _c("taps_k3_d9_48to64_zero", "s1", 2, 48, 64, 303, 3, d=9, mode=ZERO, layout=TAPS, kern="bsplit_kernel<3>"),
    _c("taps_k7_d9_80to48_two_row_tiles", "s1", 3, 80, 48, 333, 7, d=9, layout=TAPS, kern="bsplit_kernel<7>"),
    _c("fp32_k5_d3_64to48_below_floor", "s1", 2, 64, 48, 309, 5, d=3, causal=False, kern="64x128"),
    _c("fp32_k7_640_columns", "s1", 2, 32, 16, 314, 7, kern="skinny"),
    # ---- transposed split GEMM, k = 1: 72 rows in a 128-row tile, columns just above 1024; with weight norm through rows_fma
    _c("gemm_k1_72to256_wn", "s1", 3, 72, 256, 343, 1, layout=GEMM, kern="gemm_split_kernel<1>"),
    _c("gemm_k1_72to256_plain", "s1", 3, 72, 256, 343, 1, wn=False, layout=GEMM, kern="gemm_split_kernel<1>"),
    # ---- the 256 / 384 tails on the streaming plane kernel at its threshold of 65536 columns (the one large case), T % 32 != 0
    _c("pws_k1_256", "s1", 16, 256, 256, 4097, 1, kern="pws", split=True),
    _c("pws_k1_384", "s1", 16, 384, 384, 4097, 1, wn=False, kern="pws", split=True),
    # ---- fp32 pack of fac_pack_conv_w_bwd
    _c("fp32_k5_d2_37to45", "s1", 2, 37, 45, 400, 5, d=2, kern="64x128"),
    _c("fp32_k5_d2_37to45_zero", "s1", 2, 37, 45, 400, 5, d=2, mode=ZERO, causal=False, kern="64x128"),
    _c("fp32_k3_130to45_noncausal", "s1", 2, 130, 45, 391, 3, d=3, causal=False, kern="128x128"),
    _c("fp32_k5_96to40_tile96", "s1", 2, 96, 40, 391, 5, kern="96x128"),
    _c("fp32_k7_1to64_narrow", "s1", 128, 1, 64, 6, 7, kern="narrow"),
    _c("fp32_k7_1to64_tile", "s1", 2, 1, 64, 400, 7, kern="32x256"),
    _c("fp32_k7_2to130_thin", "s1", 2, 2, 130, 400, 7, kern="thin"),
    _c("fp32_k7_64to1_cin1", "s1", 256, 64, 1, 8, 7, kern="cin1"),
    _c("fp32_k7_64to1_tile", "s1", 2, 64, 1, 400, 7, kern="64x128"),
    _c("fp32_k1_5to200_thin", "s1", 3, 5, 200, 300, 1, kern="thin"),
    _c("fp32_k2_8to130_thin", "s1", 3, 8, 130, 300, 2, kern="thin"),
    _c("fp32_k5_40to24_skinny", "s1", 2, 40, 24, 100, 5, kern="skinny"),
    _c("fp32_k1_24to40_gemv", "s1", 2, 24, 40, 2, 1, kern="gemv"),
    _c("fp32_k1_200to72_short_tile", "s1", 40, 200, 72, 21, 1, kern="128x32"),
    # ---- reflect padding not shorter than the signal (pad1d's zero extension): causal, T <= pad_left, split and fp32 routes
    _c("short_k7_d1_T5_taps", "s1", 64, 32, 16, 5, 7, layout=TAPS, kern="bsplit_kernel<7>"),
    _c("short_k7_d9_T54_taps", "s1", 7, 32, 16, 54, 7, d=9, layout=TAPS, kern="bsplit_kernel<7>"),
    _c("short_k7_d1_T5_fp32", "s1", 2, 37, 45, 5, 7, kern="skinny"),
    _c("short_k7_d9_T54_fp32", "s1", 7, 37, 45, 54, 7, d=9, kern="64x128"),
    _c("short_k7_d1_T6_fp32", "s1", 2, 37, 45, 6, 7, kern="skinny"),
    # non-causal, T <= max(pad): 3 / 3 at d = 1, 27 / 27 at d = 9 (the adjoint test below runs these against the forward first)
    _c("short_nc_k7_d1_T3", "s1", 2, 37, 45, 3, 7, causal=False, kern="skinny"),
    _c("short_nc_k7_d1_T2", "s1", 2, 37, 45, 2, 7, causal=False, kern="skinny"),
    _c("short_nc_k7_d9_T27", "s1", 9, 32, 16, 27, 7, d=9, causal=False, layout=TAPS, kern="bsplit_kernel<7>"),
    _c("short_nc_k7_d9_T20", "s1", 2, 37, 45, 20, 7, d=9, causal=False, kern="skinny"),
    # ---- strided, k = 2 s, by way of the transposed conv; every route with T % s == 0 and T % s != 0 (`extra` right padding)
    # polyphase: few channels, a few frames (split-reduction kernel), and once with enough columns for a tile
    _c("poly_s2_T12", "st", 2, 20, 24, 12, s=2, layout=POLY, kern="skinny"),
    _c("poly_s2_T11", "st", 2, 20, 24, 11, s=2, layout=POLY, kern="skinny"),
    _c("poly_s5_T15", "st", 2, 20, 24, 15, s=5, layout=POLY, kern="skinny"),
    _c("poly_s5_T13", "st", 2, 20, 24, 13, s=5, layout=POLY, kern="skinny"),
    _c("poly_s6_T18", "st", 2, 20, 24, 18, s=6, layout=POLY, kern="skinny"),
    _c("poly_s6_T13", "st", 2, 20, 24, 13, s=6, layout=POLY, kern="skinny"),
    _c("poly_s6_T4_shorter_than_pad", "st", 2, 20, 24, 4, s=6, layout=POLY, kern="gemv"),
    _c("poly_s5_T13_noncausal", "st", 2, 20, 24, 13, s=5, causal=False, layout=POLY, kern="skinny"),
    _c("poly_s5_T1998_tile", "st", 2, 20, 24, 1998, s=5, mode=ZERO, layout=POLY, kern="32x256"),
    # all-phases split GEMM: t_out + 1 = 257 columns per clip, just above 1024 in all; (channel, phase) rows in 128-row tiles
    _c("rows_split_s2_T512", "st", 4, 40, 64, 512, s=2, layout=RSPLIT, kern="gemm_split_kernel<2>"),
    _c("rows_split_s2_T511", "st", 4, 40, 64, 511, s=2, layout=RSPLIT, kern="gemm_split_kernel<2>"),
    _c("rows_split_s5_T1280", "st", 4, 30, 64, 1280, s=5, layout=RSPLIT, kern="gemm_split_kernel<2>"),
    _c("rows_split_s5_T1277", "st", 4, 30, 64, 1277, s=5, layout=RSPLIT, kern="gemm_split_kernel<2>"),
    _c("rows_split_s6_T1536", "st", 4, 20, 64, 1536, s=6, layout=RSPLIT, kern="gemm_split_kernel<2>"),
    _c("rows_split_s6_T1531", "st", 4, 20, 64, 1531, s=6, layout=RSPLIT, kern="gemm_split_kernel<2>"),
    # stride-2 streaming kernel with taps at the threshold of pw_taps_ok: 256 rows -> 1536 column blocks of 32 = 16 clips x 96
    _c("pwt_s2_T6080", "st", 16, 128, 32, 6080, s=2, layout=RPWT, kern="pwt"),
    _c("pwt_s2_T6079", "st", 16, 128, 32, 6079, s=2, layout=RPWT, kern="pwt"),
    # flattened clips: t_out + 1 = 129 < 256 columns per clip, 8 x 129 = 1032 in all; at T % s != 0 the forward is not flattened
    _c("flat_s2_T256", "st", 8, 40, 64, 256, s=2, layout=TFLAT, kern="gemm_split_kernel<2>", flat=True),
    _c("flat_s2_T255", "st", 8, 40, 64, 255, s=2, layout=TFLAT, kern="gemm_split_kernel<2>", flat=True),
    _c("flat_s5_T640", "st", 8, 40, 64, 640, s=5, layout=TFLAT, kern="gemm_split_kernel<2>", flat=True),
    _c("flat_s5_T639", "st", 8, 40, 64, 639, s=5, layout=TFLAT, kern="gemm_split_kernel<2>", flat=True),
    _c("flat_s6_T768", "st", 8, 40, 64, 768, s=6, layout=TFLAT, kern="gemm_split_kernel<2>", flat=True),
    _c("flat_s6_T763", "st", 8, 40, 64, 763, s=6, layout=TFLAT, kern="gemm_split_kernel<2>", flat=True),
    # ---- dx of a transposed conv = the strided forward conv of dy: its four plans, causal and non-causal (shift s - s // 2 = 3 at
    # s = 5; the streaming kernel exists at s = 2 only, shift 1)
    _c("tr_fp32_s5_skinny", "tr", 2, 24, 20, 50, s=5, kern="skinny"),
    _c("tr_fp32_s5_skinny_noncausal", "tr", 2, 24, 20, 50, s=5, causal=False, kern="skinny"),
    _c("tr_fp32_s5_tile", "tr", 3, 40, 20, 300, s=5, kern="64x128"),
    _c("tr_fp32_s5_tile_noncausal", "tr", 3, 40, 20, 300, s=5, causal=False, kern="64x128"),
    _c("tr_gemm_s5", "tr", 4, 72, 40, 257, s=5, layout=GSTR, kern="gemm_split_kernel<2>"),
    _c("tr_gemm_s5_noncausal", "tr", 4, 72, 40, 257, s=5, causal=False, layout=GSTR, kern="gemm_split_kernel<2>"),
    _c("tr_pwt_s2", "tr", 16, 256, 16, 3041, s=2, layout=PWT, kern="pwt"),
    _c("tr_pwt_s2_noncausal", "tr", 16, 256, 16, 3041, s=2, causal=False, layout=PWT, kern="pwt"),
    _c("tr_flat_s5", "tr", 8, 72, 40, 129, s=5, layout=GSTR, form=convplan.FLAT_STRIDED, kern="gemm_split_kernel<2>", flat=True),
    _c("tr_flat_s5_noncausal", "tr", 8, 72, 40, 129, s=5, causal=False, layout=GSTR, form=convplan.FLAT_STRIDED,
       kern="gemm_split_kernel<2>", flat=True),
]
IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}


# ------------------------------------------------------------------------------------------------ geometry, plan, descriptor
def _geometry(c):
    """(t_out, pad_left, pad_right, tp) of the SConv1d whose data gradient the case takes, as ops.conv1d_bwd_data derives them."""
    return ops.plan_bwd_data(c.co, c.ci, c.k, c.s, c.d, c.B, c.T, c.causal)[1:]


def _plan(c):
    """The site's own planner call (ops.plan_bwd_data / ops.plan_convtr_bwd): (layout, form)."""
    if c.kind == "tr":
        p = ops.plan_convtr_bwd(c.ci, c.co, c.s, c.B, c.T)
        return p.layout, p.form
    p = ops.plan_bwd_data(c.co, c.ci, c.k, c.s, c.d, c.B, c.T, c.causal)[0]
    return p.layout, (p.form if c.kind == "s1" else None)


def _desc(c):
    """The launch descriptor of the case's gradient conv, from the product's builders, with pointers that are never dereferenced."""
    if c.kind == "tr":
        return convtr_bwd_launch(c.ci, c.co, c.s, c.B, c.T, c.causal)
    return bwd_data_launch(c.co, c.ci, c.k, c.s, c.d, c.B, c.T, c.causal)


# ------------------------------------------------------------------------------------------------ reference
def _ref_dx(c, dy, w):
    """float64 autograd: the gradient of sum(y * dy) w.r.t. the input of pad + conv1d (s1 / st) or of the trimmed
    conv_transpose1d (tr), on the weights `w` as given (cast to float64)."""
    dy, w = dy.double(), w.double()
    if c.kind == "tr":
        x = torch.zeros(c.B, c.ci, c.T, dtype=torch.float64, requires_grad=True)
        left = 0 if c.causal else c.s - c.s // 2
        y = F.conv_transpose1d(x, w, stride=c.s)[..., left:left + c.T * c.s]
    else:
        _, pl, pr, _ = _geometry(c)
        x = torch.zeros(c.B, c.ci, c.T, dtype=torch.float64, requires_grad=True)
        y = F.conv1d(_pad(x, pl, pr, c.mode), w, stride=c.s, dilation=c.d)
    assert y.shape == dy.shape, (y.shape, dy.shape)
    (y * dy).sum().backward()
    return x.grad


def _shapes(c):
    """(weight shape, dy shape): the transposed conv's weight is (C_in, C_out, K) with the weight norm over C_in."""
    if c.kind == "tr":
        return (c.ci, c.co, c.k), (c.B, c.co, c.T * c.s)
    return (c.co, c.ci, c.k), (c.B, c.co, _geometry(c)[0])


def _inputs(c):
    gen = torch.Generator().manual_seed(1000 + IDS.index(c.name))
    wshape, dshape = _shapes(c)
    fan = (c.ci * c.k) if c.kind != "tr" else c.ci * 2
    v = torch.randn(*wshape, generator=gen) / fan ** 0.5
    g = (torch.rand(wshape[0], 1, 1, generator=gen) + 0.5) if c.wn else None
    dy = torch.randn(*dshape, generator=gen)
    return v, g, dy


def _n_products(c):
    return c.co * c.k if c.kind != "st" else c.co * 2


# ------------------------------------------------------------------------------------------------ CPU-only checks of the table
def test_case_table_names_the_plan_of_every_case():
    """Every case's expected layout and form against convplan alone: a threshold that moves a case off its route fails here,
    without a GPU.  Next to each threshold the table sits on, the neighbouring shape must take the other route."""
    assert len(set(IDS)) == len(IDS)
    bad = [(c.name, _plan(c), (c.layout, c.form)) for c in CASES if _plan(c) != (c.layout, c.form)]
    assert not bad, bad
    for kind, layouts in (("s1", {TAPS, GEMM, FP32}), ("st", {POLY, RSPLIT, RPWT, TFLAT}), ("tr", {FP32, GSTR, PWT})):
        assert {c.layout for c in CASES if c.kind == kind} == layouts, kind
    assert {(c.form, c.causal) for c in CASES if c.kind == "tr" and c.layout == GSTR} == {(f, cz) for f in (convplan.PER_CLIP, convplan.FLAT_STRIDED)
                                                                                              for cz in (True, False)}
    # thresholds: 640 columns (taps), 1024 columns (k = 1 GEMM), 65536 columns (the 256 / 384 tails), pw_taps_ok's column blocks,
    # 256 columns per clip (all-phases GEMM against flattened), floor_k
    P = convplan.plan_conv
    assert P(32, 16, 7, 1, 1, 2, 314, 320).layout == FP32 and P(32, 16, 7, 1, 1, 2, 315, 321).layout == TAPS
    assert P(72, 256, 1, 1, 1, 3, 341, 341).layout == FP32 and P(72, 256, 1, 1, 1, 3, 342, 342).layout == GEMM
    for ch in (256, 384):
        assert P(ch, ch, 1, 1, 1, 16, 4096, 4096).layout == FP32 and P(ch, ch, 1, 1, 1, 1, 65535, 65535).layout == GEMM
    T = convplan.plan_convtr
    assert T(32, 128, 2, 16, 3041, flat_train_cols=3041).layout == RPWT and T(32, 128, 2, 16, 3040, flat_train_cols=3040).layout == POLY
    assert T(64, 40, 5, 4, 257, flat_train_cols=257).layout == RSPLIT and T(64, 40, 5, 4, 255, flat_train_cols=255).layout == POLY
    assert T(64, 40, 5, 8, 129, flat_train_cols=129).layout == TFLAT and T(64, 40, 5, 7, 129, flat_train_cols=129).layout == POLY
    assert P(256, 16, 4, 2, 1, 16, 6082, 3041, flat_train="zero").layout == PWT and P(256, 16, 4, 2, 1, 16, 6080, 3040, flat_train="zero").layout == FP32
    assert P(72, 40, 10, 5, 1, 8, 645, 129, flat_train="zero").form == convplan.FLAT_STRIDED
    assert P(72, 40, 10, 5, 1, 7, 645, 129, flat_train="zero") == convplan.ConvPlan(FP32, convplan.PER_CLIP, None)
    # the edges the table exists for are all in it
    st = [c for c in CASES if c.kind == "st"]
    for layout in (POLY, RSPLIT, RPWT, TFLAT):
        rem = {c.T % c.s == 0 for c in st if c.layout == layout}
        assert rem == {True, False}, layout
    assert {c.s for c in st if c.layout == POLY} == {c.s for c in st if c.layout == RSPLIT} == {c.s for c in st if c.layout == TFLAT} == {2, 5, 6}
    s1 = [c for c in CASES if c.kind == "s1"]
    assert {(c.k, c.d) for c in s1 if c.layout == TAPS} >= {(7, 1), (5, 3), (3, 9)}
    assert {(c.mode, c.causal) for c in s1 if c.layout == TAPS} >= {(REFLECT, True), (REFLECT, False), (ZERO, True)}
    assert any(c.mode == REFLECT and c.causal and c.T <= _geometry(c)[1] and c.split for c in s1)
    assert any(c.mode == REFLECT and not c.causal and c.T <= max(_geometry(c)[1:3]) for c in s1)
    for c in CASES:             # no gradient fills its kernel's column tile (128 columns at the least) exactly
        cols = c.T if c.kind == "tr" else _geometry(c)[3]
        assert cols % 128 != 0, c.name


def test_case_table_names_the_kernel_of_every_case():
    """The C++ planner (fac_conv1d_variant, host only) on the descriptor each case launches: the kernel family the table names.
    The GPU test asserts the same name on the launch itself."""
    bad = []
    for c in CASES:
        kid, name = ops.conv_variant(_desc(c))
        if kid < 0 or c.kern not in name or ("bf16x3" in name) != c.split:
            bad.append((c.name, kid, name))
    assert not bad, bad
    want = ("bsplit", "gemm_split", "pws", "pwt", "skinny", "gemv", "narrow", "cin1", "thin", "32x256", "64x128", "96x128", "128x128", "128x32")
    assert {c.kern for c in CASES} >= {k for k in want if k not in ("bsplit", "gemm_split")}
    assert any("bsplit" in c.kern for c in CASES) and any("gemm_split" in c.kern for c in CASES)


@pytest.mark.parametrize("name", IDS)
def test_reference_is_autograd_through_the_oracle_padding(name):
    """`_ref_dx` (explicit `_pad`, then F.conv1d / F.conv_transpose1d) against float64 autograd through the oracle's own
    restatement of SConv1d / SConvTranspose1d (oracle/facodec_oracle.py: _pad1d, the trims) at the case's length, kernel size,
    stride, dilation, padding mode and causality; two clips and a few channels are enough for the padding rule."""
    from oracle import facodec_oracle as O
    c = BY_NAME[name]._replace(B=2, ci=3, co=2)
    gen = torch.Generator().manual_seed(7)
    wshape, dshape = _shapes(c)
    w = torch.randn(*wshape, generator=gen, dtype=torch.float64)
    dy = torch.randn(*dshape, generator=gen, dtype=torch.float64)
    x = torch.randn(c.B, c.ci, c.T, generator=gen, dtype=torch.float64, requires_grad=True)
    if c.kind == "tr":
        y = O.sconvtr1d(x, w, None, c.s, causal=c.causal)
    else:
        y = O.sconv1d(x, w, None, stride=c.s, dilation=c.d, causal=c.causal, pad_mode="reflect" if c.mode == REFLECT else "constant")
    (y * dy).sum().backward()
    ref = _ref_dx(c, dy, w)
    assert float((ref - x.grad).abs().max()) <= 1e-12 * max(1.0, float(x.grad.abs().max()))


# ------------------------------------------------------------------------------------------------ the GPU test
class _Spy:
    """Records (batch, kernel name, descriptor) of every conv launch, as test_short_clip_training_convs_run_flattened does."""

    def __enter__(self):
        self.launches, self.orig = [], ops._launch_conv

        def spy(d, what):
            self.orig(d, what)               # first: the launch hands the descriptor its workspace, which the selection reads
            self.launches.append((d.B, ops.conv_variant(d)[1], d))

        ops._launch_conv = spy
        return self

    def __exit__(self, *exc):
        ops._launch_conv = self.orig
        return False


def _grad(c, cuda, vd, gd, dyd, xd, **kw):
    if c.kind == "tr":
        return ops.conv_transpose1d_bwd(xd, dyd, vd, gd, c.s, causal=c.causal)[0]
    return ops.conv1d_bwd_data(dyd, vd, gd, c.T, stride=c.s, dilation=c.d, pad_mode=c.mode, causal=c.causal, **kw)


def _effective_weight(v, g, cuda):
    """The fp32 weights every route convolves: fl32(v * scale[row]) with the scale ops.wn_scale computed (read back), or v."""
    if g is None:
        return v
    scale = ops.wn_scale(v.to(cuda), g.to(cuda)).cpu()
    return v * scale.view(-1, 1, 1)          # one fp32 multiply per element, round to nearest: __fmul_rn of the packers


@gpu
@pytest.mark.parametrize("name", IDS)
def test_conv_bwd_data_route_against_fp64(name, cuda):
    c = BY_NAME[name]
    v, g, dy = _inputs(c)
    w = _effective_weight(v, g, cuda)
    ref = _ref_dx(c, dy, w)
    mag = _ref_dx(c, dy.abs(), w.abs())
    vd, dyd = v.to(cuda), dy.to(cuda)
    gd = g.to(cuda) if g is not None else None
    xd = torch.randn(c.B, c.ci, c.T, generator=torch.Generator().manual_seed(3)).to(cuda) if c.kind == "tr" else None
    assert ops.BF16_SPLIT and ops.FOLD_IN_PLACE == 1
    with _Spy() as spy:
        dx = _grad(c, cuda, vd, gd, dyd, xd)
        torch.cuda.synchronize()
    # the route: one conv launch, the kernel the table names, flattened launches as one signal
    assert len(spy.launches) == 1, spy.launches
    b_launch, kernel, launched = spy.launches[0]
    assert_same_launch(launched, _desc(c), c.name)           # the descriptor the CPU tests of the table judge is the one launched
    assert c.kern in kernel and ("bf16x3" in kernel) == c.split, (kernel, c.kern)
    assert (b_launch == 1) == (c.flat or c.B == 1), (b_launch, kernel)
    assert dx.shape == (c.B, c.ci, c.T) and dx.is_contiguous()
    # extra: 3 on bf16 planes (mid * lo, lo * mid, lo * lo dropped, each <= 2^-24 of its term), 0 on the fp32 kernels; the scale
    # is folded into the weights before the kernel on every route (module docstring): no + 1
    _sum_bound(f"conv_bwd_data_{c.name}", dx.cpu(), ref, mag, _n_products(c), extra=3.0 if c.split else 0.0)
    if c.split:
        try:
            ops.BF16_SPLIT = False
            with _Spy() as spy32:
                base = _grad(c, cuda, vd, gd, dyd, xd)
                torch.cuda.synchronize()
        finally:
            ops.BF16_SPLIT = True
        assert len(spy32.launches) == 1 and "bf16x3" not in spy32.launches[0][1], spy32.launches
        scale = float(ref.abs().max())
        e_split = float((dx.cpu().double() - ref).abs().max()) / scale
        e_fp32 = float((base.cpu().double() - ref).abs().max()) / scale
        _record(f"conv_bwd_data_{c.name}_split_vs_fp32", {"split": e_split, "fp32": e_fp32})
        print(f"[tol] conv_bwd_data_{c.name}: split {e_split:.3e} fp32 {e_fp32:.3e}")
        assert e_split <= 1.5 * e_fp32 + 1e-7, (e_split, e_fp32)
    if c.kind == "tr":
        return
    # folds: allow_view=True gives the window of the padded rows where the in-place fold may run (always for zero padding, for
    # reflect padding with disjoint edges), and the same bits as the un-padding copy with both shortcuts off
    _, pl, pr, tp = _geometry(c)
    try:
        ops.FOLD_IN_PLACE = 0
        copied = _grad(c, cuda, vd, gd, dyd, xd)
    finally:
        ops.FOLD_IN_PLACE = 1
    assert copied.is_contiguous() and torch.equal(copied, dx)
    view = _grad(c, cuda, vd, gd, dyd, xd, allow_view=True)
    if tp == c.T:
        assert view.is_contiguous()                       # no padding: the padded rows are the gradient
    elif c.mode == ZERO or c.T > pl + pr + 1:
        assert not view.is_contiguous() and view.stride() == (c.ci * tp, tp, 1) and view.storage_offset() == pl
    else:
        assert view.is_contiguous()                       # overlapping edges: the copying fold
    assert torch.equal(view, copied)


# ------------------------------------------------------------------------------------------------ short non-causal reflect: adjoint first
@gpu
@pytest.mark.parametrize("name", [n for n in IDS if n.startswith("short_")])
def test_short_reflect_gradient_is_the_adjoint_of_the_forward(name, cuda):
    """<conv(x), dy> = <x, dx> in float64 with the project's own forward (ops.conv1d on the fp32 pack, reflect padding read through
    reflect_index), within 8 * 2^-24 sum |x| |dx|: the fold undoes what the forward pads, before either is held to pad1d."""
    c = BY_NAME[name]
    v, g, dy = _inputs(c)
    vd, dyd = v.to(cuda), dy.to(cuda)
    gd = g.to(cuda) if g is not None else None
    x = torch.randn(c.B, c.ci, c.T, generator=torch.Generator().manual_seed(11)).to(cuda)
    y = ops.conv1d(x, ops.pack_conv_weight(vd, gd), c.co, c.k, dilation=c.d, pad_mode=c.mode, causal=c.causal)
    dx = _grad(c, cuda, vd, gd, dyd, None)
    _check_adjoint(x, y, dyd, dx)
    # the forward itself against pad1d, so that a disagreement is pinned on the right side
    w = _effective_weight(v, g, cuda)
    _, pl, pr, _ = _geometry(c)
    y64 = F.conv1d(_pad(x.cpu().double(), pl, pr, c.mode), w.double(), dilation=c.d)
    ymag = F.conv1d(_pad(x.cpu().double().abs(), pl, pr, c.mode), w.double().abs(), dilation=c.d)
    _sum_bound(f"conv_fwd_{c.name}", y.cpu(), y64, ymag, c.ci * c.k)


# ------------------------------------------------------------------------------------------------ weight helpers
@gpu
@pytest.mark.parametrize("row_len", [1, 7, 3 * 1024, 1536 * 7])
def test_wn_scale_fp64(cuda, row_len):
    """fac_wn_scale: scale = g / ||v|| per row against float64.  The sum of squares S is a reduction of row_len positive terms
    (fma per lane, a fixed tree): relative error <= c sqrt(n) 2^-24; the root halves it; sqrtf is within one ulp (2 * 2^-24
    relative) and the correctly rounded divide within half an ulp (2^-24): (c sqrt(n) / 2) 2^-24 |ref| + 3 * 2^-24 |ref|, stated
    as _sum_bound with terms |ref| / 2 and its 4 * 2^-24 |ref| for the root and the divide."""
    gen = torch.Generator().manual_seed(row_len)
    rows = 5
    v = torch.randn(rows, row_len, 1, generator=gen)
    g = torch.randn(rows, 1, 1, generator=gen)
    got = ops.wn_scale(v.to(cuda), g.to(cuda))
    ref = g.double().view(-1) / v.double().reshape(rows, -1).norm(dim=1)
    _sum_bound(f"wn_scale_{row_len}", got.cpu(), ref, ref.abs() / 2, row_len, ulps=4.0)


HELPER_SHAPES = [(45, 37, 1), (45, 37, 2), (21, 50, 7), (50, 21, 12), (3, 1, 7), (1, 130, 12)]


def _fl32_scaled(v, scale):
    return v * scale.view(-1, 1, 1) if scale is not None else v


@gpu
@pytest.mark.parametrize("with_scale", [True, False], ids=["scaled", "plain"])
@pytest.mark.parametrize("co,ci,k", HELPER_SHAPES)
def test_flipped_weight_exact(cuda, co, ci, k, with_scale):
    """ops.flipped_weight: out[ci][co][k'] = fl32(v[co][ci][K - 1 - k'] * scale[co]), bit for bit, inside a canary."""
    gen = torch.Generator().manual_seed(co * 100 + k)
    v = torch.randn(co, ci, k, generator=gen)
    g = torch.randn(co, 1, 1, generator=gen) if with_scale else None
    vd = v.to(cuda)
    scale = ops.wn_scale(vd, g.to(cuda)) if with_scale else None
    buf = torch.full((ci * co * k + 128,), CANARY, device=cuda)
    out = buf[64:64 + ci * co * k].view(ci, co, k)
    got = ops.flipped_weight(vd, g.to(cuda) if with_scale else None, scale, out=out)
    want = _fl32_scaled(v, scale.cpu() if with_scale else None).flip(2).permute(1, 0, 2).contiguous()
    assert got.data_ptr() == out.data_ptr() and torch.equal(got.cpu(), want)
    assert bool((buf[:64] == CANARY).all()) and bool((buf[-64:] == CANARY).all())
    if with_scale:                                # the scale computed inside (from g) gives the same bits
        assert torch.equal(ops.flipped_weight(vd, g.to(cuda)), got)


@gpu
@pytest.mark.parametrize("with_scale", [True, False], ids=["scaled", "plain"])
@pytest.mark.parametrize("co,ci,k", HELPER_SHAPES)
def test_pack_conv_weight_bwd_exact(cuda, co, ci, k, with_scale):
    """ops.pack_conv_weight_bwd: packed[(co K + k') CP + ci] = fl32(v[co][ci][K - 1 - k'] * scale[co]) with CP = pad32(C_in) and
    cin_pad(C_out) rows; the padding rows and columns are zeros the kernel writes itself (the buffer starts as a canary)."""
    gen = torch.Generator().manual_seed(co * 100 + k + 1)
    v = torch.randn(co, ci, k, generator=gen)
    g = torch.randn(co, 1, 1, generator=gen) if with_scale else None
    vd = v.to(cuda)
    scale = ops.wn_scale(vd, g.to(cuda)) if with_scale else None
    rows, cp = ops.cin_pad(co), ops.pad32(ci)
    n = rows * k * cp
    buf = torch.full((n + 128,), CANARY, device=cuda)
    out = buf[64:64 + n].view(rows, k, cp)
    got = ops.pack_conv_weight_bwd(vd, None, scale, out=out)
    want = torch.zeros(rows, k, cp)
    want[:co, :, :ci] = _fl32_scaled(v, scale.cpu() if with_scale else None).flip(2).permute(0, 2, 1)
    assert torch.equal(got.cpu(), want)
    assert bool((buf[:64] == CANARY).all()) and bool((buf[-64:] == CANARY).all())
    if with_scale:
        assert torch.equal(ops.pack_conv_weight_bwd(vd, g.to(cuda)), got)


@gpu
@pytest.mark.parametrize("co,ci", [(45, 37), (256, 72), (130, 200), (1, 33)])
def test_pack_gemm_weight_split_t_planes_sum_to_the_transposed_weight(cuda, co, ci):
    """ops.pack_gemm_weight_split_t of w (C_out, C_in, 1): rows = C_in, contraction over C_out.  Layout of fac_pack_gemm_w_split
    (conv1d_gemm_split.hip): [row tile][32-channel chunk][plane 3][tap][row 128][slot 4][8 bf16], slot = piece ^ ((row >> 2) & 3).
    hi + mid + lo of every element is the fp32 weight exactly, at the transposed position, and the padding is zero."""
    gen = torch.Generator().manual_seed(co + ci)
    w = torch.randn(co, ci, 1, generator=gen)
    w[0, 0, 0], w[-1, -1, 0] = 1.0 + 2.0 ** -23, -(2.0 ** -126) * 3      # all 24 bits in use; a subnormal-range product of planes
    buf = ops.pack_gemm_weight_split_t(w.to(cuda))
    n_tiles, n_ch = -(-ci // 128), -(-co // 32)
    assert buf.numel() == n_tiles * n_ch * 3 * 128 * 64
    planes = buf.cpu().view(torch.bfloat16).reshape(n_tiles, n_ch, 3, 1, 128, 4, 8).double()
    total = planes.sum(2)                                                 # (tile, chunk, tap, row, slot, 8), exact in float64
    row = torch.arange(128)
    slot = torch.arange(4).view(1, 4) ^ ((row >> 2) & 3).view(128, 1)     # slot of (row, piece)
    idx = slot.view(1, 1, 1, 128, 4, 1).expand(n_tiles, n_ch, 1, 128, 4, 8)
    unsw = total.gather(4, idx)                                           # (tile, chunk, tap, row, piece, 8)
    full = unsw[:, :, 0].permute(0, 2, 1, 3, 4).reshape(n_tiles * 128, n_ch * 32)     # (row = C_in index, C_out index)
    want = torch.zeros(n_tiles * 128, n_ch * 32, dtype=torch.float64)
    want[:ci, :co] = w[:, :, 0].double().t()
    assert torch.equal(full, want)
    # every plane holds what the planes above it left over: 8 significant bits each, so |mid| < ulp(hi) <= 2^-7 |hi| and
    # |lo| < ulp(mid) <= 2^-14 |hi| whether the split rounds or truncates
    hi, mid, lo = planes[:, :, 0].abs(), planes[:, :, 1].abs(), planes[:, :, 2].abs()
    assert bool((mid <= hi * 2.0 ** -7).all()) and bool((lo <= hi * 2.0 ** -14).all())
