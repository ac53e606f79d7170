"""The conv weight gradient (ops._bwd_weight_launch, the dW of ops.conv_transpose1d_bwd) against float64, route by route and form
by form.

One table (CASES) names, for every case, the C entry ops._bwd_weight_launch_inner must call (`route`) and, on the split entry,
the kernel form fac_conv1d_bwd_weight_split_form must report (`form`: kernel, slices, tiles per slice, tiles of the last slice,
XCD order, row tiles, column-split row tiles, fused bias gradient).  The CPU-only tests walk the table with the host-only queries;
the GPU test runs it.

Reference: `_ref_dw` of tests/test_wgrad_split.py -- float64 torch autograd through an explicit pad (`_pad`: pad1d of
dac/model/encodec.py:96-113) and F.conv1d, from the same fp32 inputs; a two-level case is K / K1 such gradients over shifted
views of the zero-padded signal.  `mag` is the same gradient from |x| and |dy|: the per-element sum of absolute terms.

Bound, at every element of dW:  |dw - ref64| <= (4 sqrt(n) + extra) 2^-24 mag + 4 * 2^-24 |ref64|   (`_sum_bound`, c = 4)
  n      B * T_out products per element;
  extra  3 on the split-bf16 entry (three 8-bit planes hold an fp32 value exactly; the kernels drop mid * lo, lo * mid and lo * lo,
         each at most 2^-24 of its term: the data gradient's derivation, tests/test_conv_bwd_data.py); 0 on the k = 1 streaming
         kernel, the taps kernel and the fp32 MFMA kernel, which multiply the fp32 values themselves.
The bias gradient: the same bound with mag = sum |dy| over (b, t).

Size cap: B * T_out <= 4224 in every case.  The bound grows as n^1.5 with unit-normal inputs while one product does not grow: at
n <= 4224 a single product dropped from the last column ((b, t) = (B - 1, T_out - 1)) still puts at least 80 % of dW's elements
outside the bound (asserted on the CPU for every case), so a kernel that loses the tail of the signal cannot pass.  The two
transposed-conv cases drop the product of column T_out - 2 instead: in the last column half of the taps of a transposed conv
read the zero padding behind the signal (k >= s + shift), whatever the shape, so no product exists there to drop.
"""
# Measured on MI355X, worst error / bound of each route and form over its cases (dW; db in brackets where a case asks for it).  The
# bound is a sum of absolute terms times 4 sqrt(n): random signs leave every kernel two to three orders below it at n in the
# thousands, which is why the size-cap test above it matters.
#   fac_conv1d_bwd_weight_split(_db)   kmajor 0.089 at n = 10, 0.042 at n = 70, <= 0.013 from n = 200 (db 0.093 at n = 10, else 0.001);
#                                      kmajor_ksplit 0.026 at n = 129, <= 0.006 from n = 400 (db 0.002);
#                                      planes<10,3> 0.0025, planes<14,3> 0.0033, planes<19,2> 0.0026; transposed conv (kmajor) 0.0058
#   fac_conv1d_bwd_weight_k1           0.0023 (db 0.0005)       fac_conv1d_bwd_weight_taps   0.0017 (db 0.0004)
#   fac_conv1d_bwd_weight (fp32 MFMA)  0.021 at n = 260, 0.0035 .. 0.0085 at n = 600 .. 1600
# Max error / max |ref64| against the fp32 kernel's on the same case: the split entry 0.7e-7 .. 1.9e-7 against 0.7e-7 .. 6.7e-7, the
# k = 1 kernel 3.0e-7 .. 3.7e-7 against 2.6e-7 .. 3.1e-7 (worst pair 3.7e-7 / 2.9e-7), the taps kernel 2.5e-7 .. 3.6e-7 against
# 2.3e-7 .. 3.6e-7.
import functools
from collections import namedtuple

import pytest
import torch

from facodec_amd import _lib, ops
from test_train_kernels_gen import CANARY, EPS32, _canary, _record, _sum_bound
from test_wgrad_split import _pad, _ref_dw

gpu = pytest.mark.gpu
REFLECT, ZERO = ops.PAD_REFLECT, ops.PAD_ZERO
MAX_N = 4224

ENTRY = {"k1": "fac_conv1d_bwd_weight_k1", "taps": "fac_conv1d_bwd_weight_taps", "split_db": "fac_conv1d_bwd_weight_split_db",
         "split": "fac_conv1d_bwd_weight_split", "fp32": "fac_conv1d_bwd_weight"}
KM, KSP, P10, P14, P19 = ops.WGRAD_SPLIT_KERNELS
Form = ops.WgradSplitForm

# kind "conv": the dW of a causal SConv1d ci -> co over B clips of T samples (pad_left = (k - 1) d + 1 - s, T_out = ceil(T / s)); with
#   k1 > 0 the two-level conv of the discriminators over one row-concatenated signal of pitch d2: k = 3 k1 taps at k2 * d2 + k1' * d,
#   pad_left = d2 + k1 // 2, zero padding, T outputs from T + d2 + k1 samples (every tap of the last column reads a sample).
# kind "tr": the dW of SConvTranspose1d ci -> co (kernel 2 s) over B clips of T frames, through ops.conv_transpose1d_bwd: the roles
#   of input and output swapped, see `_shape`.
# db: a bias gradient is requested.  env: "" -- module switches as shipped; "nosplit" -- ops.BF16_SPLIT = False; "cap" --
#   ops.WGRAD_WS_CAP lowered below the split entry's workspace.
Case = namedtuple("Case", "name route B ci co T k s d mode k1 d2 db kind causal env form")
Shape = namedtuple("Shape", "B ci t_in co t_out k s d pl mode k1 d2")


def _c(name, route, B, ci, co, T, k, s=1, d=1, mode=REFLECT, k1=0, d2=0, db=False, kind="conv", causal=True, env="", form=None):
    return Case(name, route, B, ci, co, T, k, s, d, ZERO if k1 else mode, k1, d2, db, kind, causal, env, form)


CASES = [
    # ---- k-major kernel.  64 -> 64 k = 7: one-tile slices; B = 1 with 3 / 4 / 5 tiles sits on both thresholds (k-split from
    # S = 4, XCD order from S = 5); T_out % 32 = 28, 6, 0, 1
    _c("km_64_k7_44_slices_db", "split_db", 2, 64, 64, 700, 7, db=True, form=Form(KSP, 44, 1, 1, True, 1, 1, True)),
    _c("km_64_k7_S3", "split", 1, 64, 64, 70, 7, form=Form(KM, 3, 1, 1, False, 1, 1, False)),
    _c("km_64_k7_S4", "split", 1, 64, 64, 128, 7, form=Form(KSP, 4, 1, 1, False, 1, 1, False)),
    _c("km_64_k7_S5", "split", 1, 64, 64, 129, 7, form=Form(KSP, 5, 1, 1, True, 1, 1, False)),
    # 256 -> 256 k = 7 (two full row tiles): 2, 3 and 5 tiles per slice of the 3-stage pipeline, the last slice ragged (1 of 3, 2 of 5)
    _c("km_256_k7_2_tiles", "split", 2, 256, 256, 600, 7, form=Form(KSP, 19, 2, 2, True, 2, 0, False)),
    _c("km_256_k7_3_tiles_ragged", "split", 2, 256, 256, 900, 7, form=Form(KSP, 20, 3, 1, True, 2, 0, False)),
    _c("km_256_k7_5_tiles_ragged_db", "split_db", 2, 256, 256, 2100, 7, db=True, form=Form(KSP, 27, 5, 2, True, 2, 0, True)),
    # the bias gradient's row sums in two chunks of 2048 steps (UA = 2112)
    _c("km_48to64_k5_db_two_chunks", "split_db", 1, 48, 64, 2100, 5, mode=ZERO, db=True, form=Form(KM, 66, 1, 1, True, 1, 1, True)),
    # dilations 3 and 9; C_out = 192: a second row tile of 64
    _c("km_96_k7_d3", "split", 2, 96, 96, 500, 7, d=3, form=Form(KSP, 32, 1, 1, True, 1, 1, False)),
    _c("km_192_k7_d9_second_tile_64", "split", 2, 192, 192, 500, 7, d=9, form=Form(KSP, 32, 1, 1, True, 2, 1, False)),
    # channel counts that are no multiples of 32, the floor CV = 16, row tiles of <= 32, 33 .. 96, 97 .. 128 and 128 + 2 real rows
    _c("km_48to64_k5", "split", 2, 48, 64, 300, 5, mode=ZERO, form=Form(KM, 20, 1, 1, True, 1, 1, False)),
    _c("km_16to32_k7_floor_db", "split_db", 2, 16, 32, 200, 7, db=True, form=Form(KSP, 14, 1, 1, True, 1, 1, True)),
    _c("km_80to130_k7_d3", "split", 3, 80, 130, 257, 7, d=3, form=Form(KSP, 27, 1, 1, True, 2, 1, False)),
    _c("km_40to100_k3", "split", 2, 40, 100, 127, 3, form=Form(KM, 8, 1, 1, True, 1, 0, False)),
    _c("km_40to20_k3", "split", 2, 40, 20, 301, 3, mode=ZERO, form=Form(KM, 20, 1, 1, True, 1, 1, False)),
    # strides 2, 5, 6 with k = 2 s
    _c("km_64to128_k4_s2", "split", 2, 64, 128, 640, 4, s=2, form=Form(KM, 20, 1, 1, True, 1, 0, False)),
    _c("km_32to64_k10_s5", "split", 2, 32, 64, 650, 10, s=5, form=Form(KM, 10, 1, 1, True, 1, 1, False)),
    _c("km_24to48_k12_s6", "split", 2, 24, 48, 612, 12, s=6, form=Form(KM, 8, 1, 1, True, 1, 1, False)),
    # two-level taps (3, 9) over a row pitch of 32: 96 virtual channels
    _c("km_32to32_two_level", "split", 1, 32, 32, 3200, 27, k1=9, d2=32, form=Form(KM, 100, 1, 1, True, 1, 1, False)),
    # reflect padding not shorter than the signal (pad1d's zero extension): T = 5 <= 6, T = 54 <= 54
    _c("km_64_k7_T5_short_db", "split_db", 2, 64, 64, 5, 7, db=True, form=Form(KM, 2, 1, 1, False, 1, 1, True)),
    _c("km_32_k7_d9_T54_short", "split", 2, 32, 32, 54, 7, d=9, form=Form(KSP, 4, 1, 1, False, 1, 1, False)),
    # B * C_out = 66560 > 65535 rows: the bias gradient is not fused (the grid of the row-sum pass)
    _c("km_16to130_k3_B512_db_not_fused", "split", 512, 16, 130, 8, 3, db=True, form=Form(KM, 256, 2, 2, True, 2, 1, False)),
    # ---- planes kernel (C_in < 16): 9, 11 and 19 staged pieces per lane -> <10,3>, <14,3>, <19,2>; strided; two-level below the
    # taps kernel's T_out; never a fused bias gradient
    _c("pl_1to64_k7_d1_db_not_fused", "split", 2, 1, 64, 401, 7, db=True, form=Form(P10, 26, 1, 1, False, 1, 0, False)),
    _c("pl_1to64_k7_d3", "split", 2, 1, 64, 401, 7, d=3, form=Form(P14, 26, 1, 1, False, 1, 0, False)),
    _c("pl_1to64_k7_d9", "split", 2, 1, 64, 401, 7, d=9, form=Form(P19, 26, 1, 1, False, 1, 0, False)),
    _c("pl_4to32_k4_s2", "split", 2, 4, 32, 600, 4, s=2, form=Form(P14, 20, 1, 1, False, 1, 0, False)),
    _c("pl_2to32_two_level", "split", 1, 2, 32, 3200, 27, k1=9, d2=32, form=Form(P10, 100, 1, 1, False, 1, 0, False)),
    # ---- k = 1 streaming kernel: quadrants of 2 x 2 (Q = 2) or 3 x 3 (Q = 3) blocks, 1 .. 4 roles per workgroup; T % 4 == 0, T % 32 != 0
    _c("k1_64x64", "k1", 1, 64, 64, 4100, 1, mode=ZERO),
    _c("k1_96x96_db", "k1", 1, 96, 96, 4104, 1, mode=ZERO, db=True),
    _c("k1_128x128", "k1", 1, 128, 128, 4108, 1, mode=ZERO),
    _c("k1_192x192_db", "k1", 1, 192, 192, 4116, 1, mode=ZERO, db=True),
    _c("k1_64to192", "k1", 1, 64, 192, 4132, 1, mode=ZERO),
    _c("k1_192to96", "k1", 1, 192, 96, 4220, 1, mode=ZERO),
    # ---- taps kernel (virtual rows)
    _c("taps_1to64_k7_reflect_db", "taps", 1, 1, 64, 4099, 7, db=True),
    _c("taps_2to32_k9_zero", "taps", 1, 2, 32, 4099, 9, mode=ZERO),
    _c("taps_1to32_k5_d2", "taps", 1, 1, 32, 4099, 5, d=2),
    _c("taps_2to32_two_level", "taps", 1, 2, 32, 4114, 27, k1=9, d2=34),
    # ---- fp32 MFMA kernel on its own: k = 1, 7, 10 (stride 5), two-level taps, channel counts 1, 37, 130
    _c("fp32_37to130_k1", "fp32", 2, 37, 130, 300, 1, mode=ZERO, env="nosplit"),
    _c("fp32_1to64_k7", "fp32", 2, 1, 64, 401, 7, env="nosplit"),
    _c("fp32_37to45_k10_s5", "fp32", 2, 37, 45, 650, 10, s=5, env="nosplit"),
    _c("fp32_6to32_two_level", "fp32", 1, 6, 32, 1600, 27, k1=9, d2=32, env="nosplit"),
    _c("fp32_130to37_k7_d3", "fp32", 2, 130, 37, 300, 7, d=3, env="nosplit"),
    _c("fp32_64_k7_above_ws_cap", "fp32", 2, 64, 64, 700, 7, env="cap"),
    # ---- transposed conv, the roles swapped: s = 2 causal, s = 5 non-causal (shift 3)
    _c("tr_64to32_s2", "split", 2, 64, 32, 500, 4, s=2, kind="tr", form=Form(KM, 32, 1, 1, True, 1, 1, False)),
    _c("tr_96to48_s5_noncausal", "split", 2, 96, 48, 300, 10, s=5, kind="tr", causal=False, form=Form(KM, 20, 1, 1, True, 1, 1, False)),
]
IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
SPLIT_ROUTES = ("split", "split_db")


# ------------------------------------------------------------------------------------------------ geometry, route
def _shape(c):
    """The arguments ops._bwd_weight_launch gets for the case."""
    if c.kind == "tr":      # ops.conv_transpose1d_bwd: x = the transposed conv's dy (B, co, T s), dy = its x (B, ci, T); dW (ci, co, 2 s)
        return Shape(c.B, c.co, c.T * c.s, c.ci, c.T, c.k, c.s, 1, 0 if c.causal else c.s - c.s // 2, ZERO, 0, 0)
    if c.k1:
        return Shape(c.B, c.ci, c.T + c.d2 + c.k1, c.co, c.T, c.k, 1, c.d, c.d2 + c.k1 // 2, ZERO, c.k1, c.d2)
    t_out, pad_left, _ = ops.conv_out_len(c.T, c.k, c.s, c.d)
    return Shape(c.B, c.ci, c.T, c.co, t_out, c.k, c.s, c.d, pad_left, c.mode, 0, 0)


def _split_args(sh):
    return (sh.B, sh.ci, sh.t_in, sh.co, sh.t_out, sh.k, sh.s, sh.d, sh.k1, sh.d2)


def _ws_query(route, sh):
    """The workspace query of the route's C entry (host only)."""
    lib = _lib.load()
    kk1 = sh.k1 if 0 < sh.k1 < sh.k else sh.k
    if route == "k1":
        return lib.fac_conv1d_bwd_weight_k1_ws_bytes(sh.B, sh.ci, sh.co, sh.t_in)
    if route == "taps":
        return lib.fac_conv1d_bwd_weight_taps_ws_bytes(sh.B, sh.ci, sh.co, sh.t_out, sh.k, kk1, sh.d, sh.d2 if kk1 < sh.k else 0)
    if route in SPLIT_ROUTES:
        return lib.fac_conv1d_bwd_weight_split_ws_bytes(*_split_args(sh))
    return lib.fac_conv1d_bwd_weight_ws_bytes(sh.B, sh.ci * (sh.k // kk1), sh.co, sh.t_out, kk1)


def _route(sh, want_db, split=True, cap=ops.WGRAD_WS_CAP):
    """The conditions of ops._bwd_weight_launch_inner in its order, on the shape-only queries (tensors from torch's allocator are
    16-byte aligned, which is all the `_for` queries add)."""
    lib = _lib.load()
    if split and sh.k == 1 and sh.s == 1 and sh.pl == 0 and sh.t_in == sh.t_out and sh.k1 in (0, 1) and _ws_query("k1", sh) > 0:
        return "k1"
    if split and sh.k > 1 and sh.s == 1 and sh.ci * sh.k <= 64 and sh.co in (32, 64) and sh.t_out >= 4096 and _ws_query("taps", sh) > 0:
        return "taps"
    nbytes = _ws_query("split", sh) if split else -1
    if nbytes > cap:
        nbytes = -1
    if nbytes > 0:
        return "split_db" if want_db and lib.fac_conv1d_bwd_weight_split_db_ok(*_split_args(sh)) else "split"
    return "fp32"


def _case_route(c):
    sh = _shape(c)
    cap = _ws_query("split", sh) - 1 if c.env == "cap" else ops.WGRAD_WS_CAP
    return _route(sh, c.db, split=c.env != "nosplit", cap=cap)


def _form(c):
    return ops.wgrad_split_form(*_split_args(_shape(c)), want_db=c.db)


# ------------------------------------------------------------------------------------------------ reference
def _dw64(sh, x, dy):
    """float64 dW (C_out, C_in, K) of the launch `sh` describes; two-level taps as K / K1 plain gradients over shifted views."""
    if sh.k1:
        xp = torch.nn.functional.pad(x.double(), (sh.pl, 0))
        return torch.cat([_ref_dw(xp[..., k2 * sh.d2:], dy, sh.k1, 1, sh.d, 0, ZERO) for k2 in range(sh.k // sh.k1)], dim=2)
    return _ref_dw(x, dy, sh.k, sh.s, sh.d, sh.pl, sh.mode)


def _tap_offsets(sh):
    kk1 = sh.k1 if sh.k1 else sh.k
    return [(kk // kk1) * sh.d2 + (kk % kk1) * sh.d for kk in range(sh.k)]


def _one_product(sh, x, dy, b, t):
    """The term of column (b, t) in every element of dW: dy[b][co][t] * xpad[b][ci][t s + offset(k)]."""
    offs = _tap_offsets(sh)
    need = (sh.t_out - 1) * sh.s + max(offs) + 1
    xp = _pad(x[b:b + 1].double(), sh.pl, max(0, need - sh.pl - sh.t_in), sh.mode)[0]
    cols = torch.stack([xp[:, t * sh.s + o] for o in offs], dim=1)                      # (C_in, K)
    return dy[b, :, t].double().view(-1, 1, 1) * cols.unsqueeze(0)


def _inputs(c, sh):
    gen = torch.Generator().manual_seed(2000 + IDS.index(c.name))
    return torch.randn(sh.B, sh.ci, sh.t_in, generator=gen), torch.randn(sh.B, sh.co, sh.t_out, generator=gen)


Ref = namedtuple("Ref", "x dy dw mag db db_mag")


@functools.lru_cache(maxsize=None)
def _ref(name):
    """Inputs and float64 references of a case, computed once and shared by the CPU and the GPU tests; never modified."""
    c = BY_NAME[name]
    sh = _shape(c)
    x, dy = _inputs(c, sh)
    return Ref(x, dy, _dw64(sh, x, dy), _dw64(sh, x.abs(), dy.abs()), dy.double().sum((0, 2)), dy.double().abs().sum((0, 2)))


def _dw_bound(c, ref):
    n = c.B * _shape(c).t_out
    extra = 3.0 if c.route in SPLIT_ROUTES else 0.0
    return (4.0 * n ** 0.5 + extra) * EPS32 * ref.mag + 4.0 * EPS32 * ref.dw.abs()


# ------------------------------------------------------------------------------------------------ CPU-only checks of the table
def test_case_table_routes_follow_from_the_queries():
    """Every case's C entry from the *_ws_bytes queries in the order ops._bwd_weight_launch_inner asks them, without a GPU."""
    assert len(set(IDS)) == len(IDS)
    bad = [(c.name, _case_route(c), c.route) for c in CASES if _case_route(c) != c.route]
    assert not bad, bad
    assert {c.route for c in CASES} == set(ENTRY)
    for c in CASES:                 # every query the GPU test sizes a workspace with answers, in whole floats
        nb = _ws_query(c.route, _shape(c))
        assert nb > 0 and nb % 4 == 0, (c.name, nb)
        assert (c.form is not None) == (c.route in SPLIT_ROUTES), c.name
    # the fp32 cases are shapes the split entry would take: only the switch or the budget sends them to the fp32 kernel
    for c in CASES:
        if c.route == "fp32":
            assert _route(_shape(c), c.db) != "fp32", c.name


def test_case_table_forms_are_the_querys_answer():
    """fac_conv1d_bwd_weight_split_form (the plan the launch reads) on every split case: the form the table names."""
    bad = [(c.name, _form(c), c.form) for c in CASES if c.form is not None and _form(c) != c.form]
    assert not bad, bad
    lib = _lib.load()
    for c in CASES:                 # the older yes / no query is the same plan
        if c.form is not None and c.db:
            assert bool(lib.fac_conv1d_bwd_weight_split_db_ok(*_split_args(_shape(c)))) == c.form.db_fused, c.name
    # a shape the workspace query refuses has no form
    assert lib.fac_conv1d_bwd_weight_split_ws_bytes(2, 64, 700, 64, 700, 27, 1, 1, 9, 0) == -1
    assert ops.wgrad_split_form(2, 64, 700, 64, 700, 27, 1, 1, 9, 0) is None


def test_neighbouring_shapes_take_the_other_form():
    """Next to each threshold the table sits on, the neighbouring shape takes the other route or form."""
    F = ops.wgrad_split_form
    lib = _lib.load()

    def conv(B, ci, co, T, k, s=1, d=1, db=False):
        return F(B, ci, T, co, ops.conv_out_len(T, k, s, d)[0], k, s, d, 0, 0, want_db=db)

    # slices: 3 / 4 / 5 tiles of 32 steps at B = 1 -> k-split from S = 4, XCD order from S = 5
    assert [(conv(1, 64, 64, T, 7).slices, conv(1, 64, 64, T, 7).kernel, conv(1, 64, 64, T, 7).xcd_order) for T in (96, 97, 128, 129)] == \
        [(3, KM, False), (4, KSP, False), (4, KSP, False), (5, KSP, True)]
    # k-split: k = 7 at stride 1 only, and at most 256 workgroups per slice (544 -> 1024: 8 x 30 = 240, 608 -> 1024: 8 x 34 = 272;
    # the 8 x 32 of 576 -> 1024 never gets four slices from the cost model), four slices in both
    assert conv(2, 64, 64, 700, 5).kernel == KM and conv(2, 64, 64, 700, 7, d=3).kernel == KSP
    a, b = conv(2, 544, 1024, 700, 7), conv(2, 608, 1024, 700, 7)
    assert (a.kernel, b.kernel) == (KSP, KM) and a.slices == b.slices == 4
    # k-major from 16 (virtual) input channels; 6 real channels x 3 rows of taps = 18 virtual ones
    assert conv(2, 16, 32, 200, 7).kernel == KSP and conv(2, 15, 32, 200, 7).kernel == P10
    assert F(1, 6, 1641, 32, 1600, 27, 1, 1, 9, 32).kernel == KM and F(1, 5, 1641, 32, 1600, 27, 1, 1, 9, 32).kernel.startswith("planes")
    # planes kernel: staged pieces per lane <= 10 | <= 14 | more, over the dilation
    assert [conv(2, 1, 64, 401, 7, d=d).kernel for d in (1, 2, 3, 5, 6, 9)] == [P10, P10, P14, P14, P19, P19]
    # column-split row tiles: the last row tile with <= 96 real rows
    assert [conv(2, 40, co, 127, 3).narrow_row_tiles for co in (32, 96, 97, 128, 129, 224, 225)] == [1, 1, 0, 0, 1, 1, 0]
    assert [conv(2, 40, co, 127, 3).row_tiles for co in (128, 129)] == [1, 2]
    # fused bias gradient: at most 65535 rows B * C_out, k-major only, only when asked for
    assert conv(512, 16, 127, 8, 3, db=True).db_fused and conv(511, 16, 128, 8, 3, db=True).db_fused
    assert not conv(512, 16, 128, 8, 3, db=True).db_fused and not conv(2, 64, 64, 700, 7).db_fused
    # tiles per slice and the ragged last slice follow the tile count
    a, b = conv(2, 256, 256, 448, 7), conv(2, 256, 256, 449, 7)               # 28 and 30 tiles over 28 workgroups per slice
    assert (a.slices, a.tiles_per_slice, b.slices, b.tiles_per_slice) == (28, 1, 15, 2)
    # k = 1 streaming kernel: T >= 4096, T % 4 == 0, channel multiples of 64 or of 96 in 64 .. 192, at most four roles
    q = lib.fac_conv1d_bwd_weight_k1_ws_bytes
    assert q(1, 64, 64, 4096) > 0 and q(1, 64, 64, 4092) < 0 and q(1, 64, 64, 4098) < 0
    assert q(1, 128, 192, 4100) < 0 and q(1, 80, 96, 4100) < 0 and q(1, 256, 256, 4100) < 0 and q(1, 32, 64, 4100) < 0
    # taps kernel: T_out >= 4096, C_in * K <= 64, C_out 32 or 64
    t = lib.fac_conv1d_bwd_weight_taps_ws_bytes
    assert t(1, 1, 64, 4096, 7, 7, 1, 0) > 0 and t(1, 1, 64, 4095, 7, 7, 1, 0) < 0
    assert t(1, 2, 32, 4114, 27, 9, 1, 34) > 0 and t(1, 3, 32, 4114, 27, 9, 1, 34) < 0 and t(1, 1, 48, 4099, 7, 7, 1, 0) < 0
    # the workspace budget: one byte below the split entry's need sends the layer to the fp32 kernel
    sh = _shape(BY_NAME["fp32_64_k7_above_ws_cap"])
    nb = _ws_query("split", sh)
    assert _route(sh, False, cap=nb) == "split" and _route(sh, False, cap=nb - 1) == "fp32"


def test_case_table_holds_every_edge():
    km = [c for c in CASES if c.form is not None and c.form.kernel in (KM, KSP) and c.kind == "conv"]
    forms = [c.form for c in km]
    assert {min(f.tiles_per_slice, 4) for f in forms} == {1, 2, 3, 4}
    assert any(f.last_slice_tiles < f.tiles_per_slice for f in forms)
    assert {(f.kernel, f.slices >= 4) for f in forms if f.kernel == KSP} == {(KSP, True)} and any(f.kernel == KM for f in forms)
    assert any(c.k == 7 and c.s == 1 and c.form.kernel == KM and c.form.slices < 4 for c in km)
    assert {f.xcd_order for f in forms} == {True, False} and {f.slices for f in forms} >= {3, 4, 5, 44}
    last_rows = {c.co - 128 * (c.form.row_tiles - 1) for c in km}
    assert any(r <= 32 for r in last_rows) and any(32 < r <= 96 for r in last_rows) and any(96 < r <= 128 for r in last_rows)
    assert any(c.co == 192 for c in km) and any(c.co == 130 for c in km)
    assert any(c.ci % 32 for c in km) and any(c.ci == 16 for c in km)
    assert {(c.s, c.k) for c in km if c.s > 1} == {(2, 4), (5, 10), (6, 12)}
    assert {c.d for c in km} >= {1, 3, 9}
    assert any(c.k1 == 9 and c.k == 27 and c.d2 == 32 and (c.ci, c.co) == (32, 32) for c in km)
    assert any(c.mode == REFLECT and c.T <= _shape(c).pl for c in km)
    assert {_shape(c).t_out % 32 for c in km} >= {0, 1, 31}
    # planes kernel
    pl = [c for c in CASES if c.form is not None and c.form.kernel.startswith("planes")]
    assert {c.form.kernel for c in pl} == {P10, P14, P19} and all(c.ci < 16 for c in pl)
    assert {c.d for c in pl if (c.ci, c.co, c.k) == (1, 64, 7)} == {1, 3, 9}
    assert any((c.k, c.s) == (4, 2) for c in pl) and any(c.k1 == 9 and c.ci == 2 and _shape(c).t_out < 4096 for c in pl)
    # k = 1 streaming kernel
    k1 = [c for c in CASES if c.route == "k1"]
    assert {(c.ci, c.co) for c in k1} == {(64, 64), (96, 96), (128, 128), (192, 192), (64, 192), (192, 96)}
    assert all(c.B == 1 and 4096 <= c.T <= MAX_N and c.T % 4 == 0 and c.T % 32 != 0 for c in k1)
    # taps kernel
    taps = {(c.ci, c.co, c.k, c.d, c.mode, c.k1) for c in CASES if c.route == "taps"}
    assert taps == {(1, 64, 7, 1, REFLECT, 0), (2, 32, 9, 1, ZERO, 0), (1, 32, 5, 2, REFLECT, 0), (2, 32, 27, 1, ZERO, 9)}
    assert all(c.T == 4099 for c in CASES if c.route == "taps" and not c.k1)
    # fp32 MFMA kernel
    f32 = [c for c in CASES if c.route == "fp32"]
    assert sum(c.env == "nosplit" for c in f32) == 5 and sum(c.env == "cap" for c in f32) == 1
    assert {(c.k, c.s) for c in f32} >= {(1, 1), (7, 1), (10, 5)} and any(c.k1 for c in f32)
    assert {c.ci for c in f32} | {c.co for c in f32} >= {1, 37, 130}
    # bias gradient: one wave per row (UA <= 512), 256 threads per row, two row-sum chunks; not fused above 65535 rows and on the
    # planes kernel; riding on the k = 1 and the taps kernels
    ua = {-(-_shape(c).t_out // 32) * 32 for c in CASES if c.db and c.form is not None and c.form.db_fused}
    assert any(u <= 512 for u in ua) and any(512 < u <= 2048 for u in ua) and any(2048 < u <= 4096 for u in ua)
    assert any(c.db and c.route == "split" and c.B * c.co > 65535 for c in km)
    assert any(c.db and c.route == "split" for c in pl)
    assert any(c.db for c in k1) and any(c.db and c.route == "taps" for c in CASES)
    # transposed conv
    assert {(c.s, c.causal) for c in CASES if c.kind == "tr"} == {(2, True), (5, False)}


@pytest.mark.parametrize("name", IDS)
def test_reference_is_autograd_through_the_oracle(name):
    """`_dw64` (`_ref_dw` behind `_pad`) against float64 autograd through the oracle's own restatement of SConv1d /
    SConvTranspose1d (oracle/facodec_oracle.py) at the case's length, taps, stride, dilation, padding and causality, with the
    channels cut to 3 -> 2.  The oracle has no two-level conv: those cases are held to the defining sum over taps instead.  And
    `_one_product`, which the size-cap test drops, is the reference of a dy that is zero elsewhere."""
    from oracle import facodec_oracle as O
    c = BY_NAME[name]._replace(B=min(BY_NAME[name].B, 2), ci=3, co=2)
    sh = _shape(c)
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(sh.B, sh.ci, sh.t_in, generator=gen, dtype=torch.float64)
    dy = torch.randn(sh.B, sh.co, sh.t_out, generator=gen, dtype=torch.float64)
    got = _dw64(sh, x, dy)
    if c.kind == "tr":
        w = torch.zeros(c.ci, c.co, c.k, dtype=torch.float64, requires_grad=True)
        y = O.sconvtr1d(dy, w, None, c.s, causal=c.causal)             # dy: the launch's dy is the transposed conv's input
        (y * x).sum().backward()
        want = w.grad
    elif c.k1:
        xp = torch.nn.functional.pad(x, (sh.pl, 0))
        want = torch.stack([torch.einsum("bot,bit->oi", dy, xp[..., o:o + sh.t_out]) for o in _tap_offsets(sh)], dim=2)
    else:
        w = torch.zeros(c.co, c.ci, c.k, dtype=torch.float64, requires_grad=True)
        y = O.sconv1d(x, w, None, stride=c.s, dilation=c.d, causal=True, pad_mode="reflect" if c.mode == REFLECT else "constant")
        (y * dy).sum().backward()
        want = w.grad
    assert got.shape == want.shape == (sh.co, sh.ci, sh.k)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    t = sh.t_out - 1
    only = torch.zeros_like(dy)
    only[sh.B - 1, :, t] = dy[sh.B - 1, :, t]
    one = _one_product(sh, x, dy, sh.B - 1, t)
    assert float((one - _dw64(sh, x, only)).abs().max()) <= 1e-12 * max(1.0, float(one.abs().max()))


@pytest.mark.parametrize("name", IDS)
def test_a_dropped_last_column_product_lies_outside_the_bound(name):
    """The size cap (module docstring): B * T_out <= 4224, and the reference without the single product of the last column is
    outside the bound at 80 % of dW's elements or more."""
    c = BY_NAME[name]
    sh = _shape(c)
    assert sh.B * sh.t_out <= MAX_N
    ref = _ref(name)
    t = sh.t_out - (2 if c.kind == "tr" else 1)          # transposed conv: the last column in which every tap reads a sample
    drop = _one_product(sh, ref.x, ref.dy, sh.B - 1, t).abs()
    frac = float((drop > _dw_bound(c, ref)).double().mean())
    print(f"[cap] {name}: n = {sh.B * sh.t_out}, dropped products outside the bound {100 * frac:.1f} %")
    assert frac >= 0.8, (name, frac)


# ------------------------------------------------------------------------------------------------ the GPU test
class _Spy:
    """Records the weight-gradient C entries whose return code goes through _lib.check."""

    def __enter__(self):
        self.entries, self.orig = [], _lib.check

        def check(rc, what):
            if what.startswith("fac_conv1d_bwd_weight"):
                self.entries.append(what)
            return self.orig(rc, what)

        _lib.check = check
        return self

    def __exit__(self, *exc):
        _lib.check = self.orig
        return False


class _Env:
    """The module switches of a case's `env`, restored afterwards."""

    def __init__(self, c, sh, split=None):
        self.split = (c.env != "nosplit") if split is None else split
        self.cap = _ws_query("split", sh) - 1 if c.env == "cap" else ops.WGRAD_WS_CAP

    def __enter__(self):
        self.prev = (ops.BF16_SPLIT, ops.WGRAD_WS_CAP)
        ops.BF16_SPLIT, ops.WGRAD_WS_CAP = self.split, self.cap

    def __exit__(self, *exc):
        ops.BF16_SPLIT, ops.WGRAD_WS_CAP = self.prev
        return False


def _launch(sh, xd, dyd, want_db, cuda):
    """ops._bwd_weight_launch into canary buffers: (dw, db or None, fused, buffers)."""
    dw, dwbuf, pad = _canary((sh.co, sh.ci, sh.k), cuda)
    db, dbbuf, _ = _canary((sh.co,), cuda)
    fused = ops._bwd_weight_launch(xd, dyd, dw, sh.B, sh.ci, sh.t_in, sh.co, sh.t_out, sh.k, sh.s, sh.d, sh.pl, sh.mode, sh.k1, sh.d2,
                                   db=db if want_db else None)
    torch.cuda.synchronize()
    return dw, db, fused, (dwbuf, dbbuf, pad)


def _edges_intact(buf, pad):
    return bool((buf[:pad] == CANARY).all()) and bool((buf[-pad:] == CANARY).all())


WS_PAD = (1 << 20) // 4           # floats: 1 MB of canary on each side of the test-owned workspace


def _launch_direct(route, sh, xd, dyd, want_db, cuda):
    """The route's C entry itself, with a workspace of exactly the queried size between two 1 MB canaries, pre-filled with NaN."""
    lib = _lib.load()
    nb = _ws_query(route, sh)
    assert nb > 0 and nb % 4 == 0
    wsbuf = torch.full((nb // 4 + 2 * WS_PAD,), CANARY, device=cuda)
    ws = wsbuf[WS_PAD:WS_PAD + nb // 4]
    ws.fill_(float("nan"))
    dw, dwbuf, pad = _canary((sh.co, sh.ci, sh.k), cuda)
    db, dbbuf, _ = _canary((sh.co,), cuda)
    p, st = ops._ptr, ops._stream()
    dbp = p(db if want_db else None)
    kk1 = sh.k1 if 0 < sh.k1 < sh.k else sh.k
    if route == "k1":
        rc = lib.fac_conv1d_bwd_weight_k1(p(xd), p(dyd), p(dw), dbp, p(ws), nb, sh.B, sh.ci, sh.co, sh.t_in, st)
    elif route == "taps":
        # the caller pads (include/facodec_hip.h): left and right padding, then zeros up to fac_conv1d_bwd_weight_taps_tx
        d2 = sh.d2 if kk1 < sh.k else 0
        tx = lib.fac_conv1d_bwd_weight_taps_tx(sh.t_out, sh.k, kk1, sh.d, d2)
        need = (sh.t_out - 1) + max(_tap_offsets(sh)) + 1
        xp = _pad(xd, sh.pl, max(0, need - sh.pl - sh.t_in), sh.mode)
        xp = torch.nn.functional.pad(xp, (0, max(0, tx - xp.shape[-1]))).contiguous()
        rc = lib.fac_conv1d_bwd_weight_taps(p(xp), p(dyd), p(dw), dbp, p(ws), nb, sh.B, sh.ci, xp.shape[-1], sh.co, sh.t_out, sh.k, kk1,
                                            sh.d, d2, st)
    elif route == "split_db":
        rc = lib.fac_conv1d_bwd_weight_split_db(p(xd), p(dyd), p(dw), dbp, p(ws), nb, sh.B, sh.ci, sh.t_in, sh.co, sh.t_out, sh.k, sh.s,
                                                sh.d, sh.pl, sh.mode, sh.k1, sh.d2, st)
    elif route == "split":
        rc = lib.fac_conv1d_bwd_weight_split(p(xd), p(dyd), p(dw), p(ws), nb, sh.B, sh.ci, sh.t_in, sh.co, sh.t_out, sh.k, sh.s, sh.d,
                                             sh.pl, sh.mode, sh.k1, sh.d2, st)
    else:
        rc = lib.fac_conv1d_bwd_weight(p(xd), p(dyd), p(dw), p(ws), nb, sh.B, sh.ci, sh.t_in, sh.co, sh.t_out, sh.k, sh.s, sh.d, sh.pl,
                                       sh.mode, sh.k1, sh.d2, st)
    _lib.check(rc, ENTRY[route])
    torch.cuda.synchronize()
    assert _edges_intact(wsbuf, WS_PAD), "the kernel wrote outside the workspace its query reports"
    assert _edges_intact(dwbuf, pad) and _edges_intact(dbbuf, pad)
    return dw, db


@gpu
@pytest.mark.parametrize("name", IDS)
def test_wgrad_route_against_fp64(name, cuda):
    c = BY_NAME[name]
    sh = _shape(c)
    ref = _ref(name)
    xd, dyd = ref.x.to(cuda), ref.dy.to(cuda)
    n = sh.B * sh.t_out
    fused_want = c.db and c.route in ("k1", "taps", "split_db")
    label = f"{c.route}/{c.form.kernel}" if c.form is not None else c.route
    with _Env(c, sh):
        # the route: one C entry, the one the table names; on the split entry the form the query gives for the launched shape
        with _Spy() as spy:
            dw, db, fused, (dwbuf, dbbuf, pad) = _launch(sh, xd, dyd, c.db, cuda)
        assert spy.entries == [ENTRY[c.route]], spy.entries
        assert fused == fused_want
        if c.form is not None:
            assert _form(c) == c.form
        assert _edges_intact(dwbuf, pad) and _edges_intact(dbbuf, pad)
        # the bound at every element (module docstring)
        _sum_bound(f"wgrad_route_{name}[{label}]", dw.cpu(), ref.dw, ref.mag, n, extra=3.0 if c.route in SPLIT_ROUTES else 0.0)
        if fused_want:
            _sum_bound(f"wgrad_route_{name}[{label}]_db", db.cpu(), ref.db, ref.db_mag, n)
        else:
            assert bool((dbbuf == CANARY).all())             # no bias gradient asked for, or not fused: db is not touched
        # the older bar alongside
        scale = float(ref.dw.abs().max())
        e_route = float((dw.cpu().double() - ref.dw).abs().max()) / scale
        assert e_route < 1e-5, e_route
        # twice: identical bits, and the profile record names the entry and the form that ran
        prof = ops.ConvLaunchProfile()
        ops.set_conv_profile(prof)
        try:
            dw_b, db_b, _, _ = _launch(sh, xd, dyd, c.db, cuda)
        finally:
            ops.set_conv_profile(None)
        assert torch.equal(dw_b, dw) and torch.equal(db_b, db)
        (rec,) = prof.summary()
        want = {"k1": "k = 1 streaming", "taps": "virtual-row taps", "fp32": "conv1d_wgrad_kernel (fp32 MFMA)"}.get(c.route)
        assert (want or f"conv1d_wgrad_split/{c.form.kernel} ") in rec, rec
        # the C entry itself on a dirty workspace of exactly the queried size, inside canaries
        dw_c, db_c = _launch_direct(c.route, sh, xd, dyd, c.db and fused_want, cuda)
        assert torch.equal(dw_c, dw) and torch.equal(db_c, db)
        if c.kind == "tr":          # the same launch from ops.conv_transpose1d_bwd: x is the launch's dy, dy its x
            v = torch.randn(c.ci, c.co, c.k, generator=torch.Generator().manual_seed(5)).to(cuda) * 0.1
            with _Spy() as spy_tr:
                _, dw_tr = ops.conv_transpose1d_bwd(dyd, xd, v, None, c.s, causal=c.causal)
                torch.cuda.synchronize()
            assert spy_tr.entries == [ENTRY[c.route]], spy_tr.entries
            assert torch.equal(dw_tr, dw)
    if c.route == "fp32":
        _record(f"wgrad_route_{name}_max_over_max", {"fp32": e_route})
        return
    # the other older bar: within twice the fp32 kernel's error
    with _Env(c, sh, split=False):
        with _Spy() as spy32:
            base, _, _, _ = _launch(sh, xd, dyd, False, cuda)
    assert spy32.entries == [ENTRY["fp32"]], spy32.entries
    e_fp32 = float((base.cpu().double() - ref.dw).abs().max()) / scale
    _record(f"wgrad_route_{name}_max_over_max", {"route": e_route, "fp32": e_fp32})
    print(f"[tol] wgrad_route_{name}: {label} {e_route:.3e} fp32 {e_fp32:.3e}")
    assert e_fp32 < 1e-5, e_fp32
    assert e_route <= 2.0 * e_fp32 + 2e-7, (e_route, e_fp32)
