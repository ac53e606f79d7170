"""The weight-preparation path, one packer at a time and bit for bit: the weight-norm scale's consumers (fac_pack_conv_w,
fac_pack_convtr_w, fac_pack_convtr_w_rows, fac_flip_transpose_w, fac_pack_conv_w_split_rows, fac_pack_conv_w_split2,
fac_pack_gemm_w_split) and the recorded batch that replays them (fac_prep_*).

Measured on MI355X: the 71 GPU tests of this file take 2.9 s of wall time in all (pytest's own figure, import and device start-up
included); the slowest is the first (0.18 s, the device start-up), then the three-phase plan (0.13 s); every other 0.01 s or less.

How a packer is held.  Every layout is restated below from its DOCUMENTED form -- the comments of include/facodec_hip.h and the
one-line layout comments above pack_conv_split_body, pack_gemm_split_body and pack_conv_split2_body -- as a map from a weight
element (row, channel, tap) to its slot in the buffer (`_index_*`); `layout` scatters through that map into a buffer of +0,
`unlayout` gathers through it.  The kernels go the other way (one thread per slot, decomposing its index), so a slip in either
is not shared.  The effective weight is w = fl32(v * scale[row]): one fp32 multiply by torch on the CPU, what __fmul_rn does;
the split planes are the round-to-nearest-even three-way split of test_infer_kernels._p8_ref.  Everything is exact arithmetic:
every comparison in this file is bit equality and no tolerance appears anywhere.

On the GPU each output lies inside a canary buffer and is pre-filled with 0xFF bytes (NaN as fp32 and as bf16), so a slot the
packer leaves unwritten shows, and a padding slot must be +0 (not -0, not NaN).  Each case runs with scale = NULL and with the
scale fac_wn_scale itself produced on the GPU from (v, g), whose bits are read back for the restatement: the rounding of the
norm is test_wn_scale_fp64's business and none of it enters here.

Inputs: randn * exp(3 randn) clamped to 2^-96 <= |v| <= 2^96, with P8_EDGES (+-0, the halfway cases of the first and of the
second split, a very small and a very large value) in the first elements.  The three-plane split is exact for 2^-110 <= |w| <
2^127 (checked on the CPU, 200 000 values per binade, at 2^-110, -100, -60, 0, 60, 100, 120, 126; it fails at 2^-120 and below,
where the lo plane goes subnormal, and at 2^127, where hi rounds to infinity).  Two choices keep fl32(v * scale) inside that
range so that `hi + mid + lo == w` can be asserted at every element: the small and the large edge are rescaled to 2^-90 and
2^62.6 (the square of the large one must not overflow fac_wn_scale's fp32 sum of squares), and the gain g of a slice is its
own norm rounded to a power of two times a random factor in [0.5, 1.5), so scale stays near 1 with a random significand.
`_weights` asserts the range of what it hands out.

Cases are the smallest at which each index path exists, not model shapes (tables below; every id names what it reaches).

Left out, on purpose:
  * the LSTM packs: no scale, no padding.  fac_pack_lstm_whh, _whh16 and _whh_t feed the fp64 LSTM table of
    tests/test_train_kernels_gen.py, which fails on any misplacement; fac_pack_lstm_whh_split, which that table does not run, is
    pinned bit for bit to its documented layout in tests/test_lstm_split.py (with `_split3` and the 0xFF buffer of this file);
  * the grid-stride path past 65 535 workgroups of the one-thread-per-slot packers: it needs an 800 MB pack and no model shape
    reaches it."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from facodec_amd import _lib
from test_infer_kernels import P8_EDGES, _p8_ref, _same_bits
from test_train_kernels_gen import _call, _canary, _canary_intact, _g, _p

gpu = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "facodec_amd", "csrc")

# ======================================================================================================= 1. restatements (CPU)
# constants of the layouts, pinned to the source text by test_restated_constants_match_the_source
BS_CO, BS96_CO, BS_WIDE_MIN = 64, 96, 64        # conv1d_bsplit_kernel.h
B2_CO = 32                                      # conv1d_bsplit2.hip
GS_ROWS, GS_CI, GS_RB = 128, 32, 64             # conv1d_gemm_split.hip
CIN_PAD = 48                                    # fac_cin_pad / cin_pad_dev
SPLIT_KINDS = ("split_rows", "split2", "gemm")
LO, HI = 2.0 ** -110, 2.0 ** 127                # |w| for which hi + mid + lo == w (module docstring)
# P8_EDGES with its very small and very large value brought to 2^-90 and 2^62.6 (module docstring)
EDGES = P8_EDGES[:-2] + [P8_EDGES[-2] * 2.0 ** 8, P8_EDGES[-1] * 2.0 ** -40]


def _cdiv(a, b):
    return -(-a // b)


def pad32(n):
    return _cdiv(n, 32) * 32


def cin_pad(c):
    return _cdiv(c, CIN_PAD) * CIN_PAD


def bs_group(c_in):
    return 2 if c_in >= BS_WIDE_MIN else 1


def bs_slots(K, G):
    return G * K + (G * K) % 2                  # an odd number of half slots is padded with one zero slot


def b2_slots(K1):
    return K1 + K1 % 2


def convtr_rows(c_out, s):
    return _cdiv(c_out, 128 // s) * 128


def _ix(*dims):
    return torch.meshgrid(*[torch.arange(d) for d in dims], indexing="ij")


def _index_conv_w(C_out, C_in, K, C_out_pad=None, fault=None):
    """packed (C_in_pad, K, C_out_pad), co fastest: packed[ci][k][co] = v[co][ci][k]."""
    cop = C_out_pad or pad32(C_out)
    co, ci, k = _ix(C_out, C_in, K)
    return (cin_pad(C_in), K, cop), (ci * K + k) * cop + co


def _phase_tap(k, s):
    """k = p + s (1 - j): the first s taps of a ConvTranspose1d weight are j = 1, the last s are j = 0."""
    j = (k < s).long()
    return k - s * (1 - j), j


def _index_convtr_w(C_in, C_out, s, fault=None):
    """packed[p][ci][j][co] = v[ci][co][p + s (1 - j)], ci < C_in_pad, co < pad32(C_out)."""
    cip, cop = cin_pad(C_in), pad32(C_out)
    ci, co, k = _ix(C_in, C_out, 2 * s)
    p, j = _phase_tap(k, s)
    return (s, cip, 2, cop), ((p * cip + ci) * 2 + j) * cop + co


def _index_convtr_rows(C_in, C_out, s, fault=None):
    """packed[ci][j][tile * 128 + (co % cpt) * s + p], cpt = 128 / s channels per tile, tile = co / cpt."""
    cpt, R = 128 // s, convtr_rows(C_out, s)
    ci, co, k = _ix(C_in, C_out, 2 * s)
    p, j = _phase_tap(k, s)
    return (cin_pad(C_in), 2, R), (ci * 2 + j) * R + (co // cpt) * 128 + (co % cpt) * s + p


def _index_flip_t(C_out, C_in, K, fault=None):
    """out (C_in, C_out, K)[ci][co][K - 1 - k] = v[co][ci][k]."""
    co, ci, k = _ix(C_out, C_in, K)
    return (C_in, C_out, K), (ci * C_out + co) * K + (K - 1 - k)


def _split_rows_dims(C_out, C_in, K, rows):
    G = 1 if rows == BS96_CO else bs_group(C_in)
    return G, bs_slots(K, G), _cdiv(C_out, rows), _cdiv(C_in, 8 * G)


def _index_split_rows(C_out, C_in, K, rows, fault=None):
    """[co tile][stage][plane][half slot][co][8 ci]: a stage holds G groups of 8 input channels, a half slot 8 channels of one
    tap, slots ordered tap-major, group-minor; an odd count is padded with one zero slot at the END.  (The plane axis is added by
    `layout`.)"""
    G, H, n_ct, n_st = _split_rows_dims(C_out, C_in, K, rows)
    co, ci, k = _ix(C_out, C_in, K)
    stage, group = ci // (8 * G), (ci // 8) % G
    slot = k * G + group
    if fault == "group_major_slots":
        slot = group * K + k
    if fault == "zero_half_slot_first":
        slot = slot + (H - G * K)
    return (n_ct, n_st, H, rows, 8), ((((co // rows) * n_st + stage) * H + slot) * rows + co % rows) * 8 + ci % 8


def _index_split2(C_out, C_in, K, K1, fault=None):
    """[co tile of 32][chunk of 8 cv][plane][tap slot][32 co][8 cv]: v (C_out, C_in, K2 * K1) IS (C_out, CV, K1) with CV = C_in * K /
    K1 virtual channels; tap slots K1 .. H - 1 are zero."""
    if K1 <= 0 or K1 > K:
        K1 = K
    CV, H = C_in * (K // K1), b2_slots(K1)
    n_ch = _cdiv(CV, 8)
    co, cv, k1 = (t.reshape(C_out, C_in, K) for t in _ix(C_out, CV, K1))
    return (_cdiv(C_out, B2_CO), n_ch, H, B2_CO, 8), ((((co // B2_CO) * n_ch + cv // 8) * H + k1) * B2_CO + co % B2_CO) * 8 + cv % 8


def _index_gemm(R, C_in, K, S=1, fault=None):
    """[row tile][chunk][plane][tap][row 128][slot 4][8], slot = piece ^ ((row >> 2) & 3), piece = (ci % 32) / 8.  S == 1: chunk =
    32 channels, tap = k.  S > 1: chunk = (32 channels, input phase p), p fastest, holding the two taps k = p and k = S + p."""
    S = max(S, 1)
    Kt = 2 if S > 1 else K
    n_ch = _cdiv(C_in, GS_CI) * S
    r, ci, k = _ix(R, C_in, K)
    row, piece = r % GS_ROWS, (ci % GS_CI) // 8
    slot = piece if fault == "swizzle_dropped" else piece ^ ((row >> 2) & 3)
    chunk, tap = (ci // GS_CI) * S + k % S, k // S
    return (_cdiv(R, GS_ROWS), n_ch, Kt, GS_ROWS, GS_RB // 16, 8), \
        (((((r // GS_ROWS) * n_ch + chunk) * Kt + tap) * GS_ROWS + row) * (GS_RB // 16) + slot) * 8 + ci % 8


INDEX = dict(conv_w=_index_conv_w, convtr_w=_index_convtr_w, convtr_rows=_index_convtr_rows, flip_t=_index_flip_t,
             split_rows=_index_split_rows, split2=_index_split2, gemm=_index_gemm)
TILE_ROWS = dict(split_rows=lambda d: d[3], split2=lambda d: B2_CO, gemm=lambda d: GS_ROWS)


def _split3(x):
    """(..., 8) fp32 -> (3, ..., 8) bfloat16: the planes of _p8_ref (its units are rows of 8)."""
    n = x.numel() // 8
    return _p8_ref(x.reshape(n, 8).t().reshape(1, 8, n))[:, :-1].reshape(3, *x.shape)


def effective(v, scale, kind=None, dims=None, fault=None):
    """w = fl32(v * scale[row]), rows along dim 0."""
    if scale is None:
        return v
    s = scale
    if fault == "scale_from_row_in_tile":        # scale[co] for scale[ct * CO + co]
        s = scale[torch.arange(v.shape[0]) % TILE_ROWS[kind](dims)]
    return v * s.view(-1, *([1] * (v.dim() - 1)))


def layout(kind, w, dims, fault=None):
    """The buffer the packer must write for the effective weight w: fp32, or for the split kinds bfloat16 with the plane axis third."""
    shape, dest = INDEX[kind](*dims, fault=fault)
    flat = torch.zeros(math.prod(shape), dtype=torch.float32)
    flat[dest.reshape(-1)] = w.reshape(-1)
    if kind not in SPLIT_KINDS:
        return flat.view(shape)
    planes = _split3(flat.view(shape))
    if fault == "mid_lo_swapped":
        planes = planes[[0, 2, 1]]
    return planes.permute(1, 2, 0, *range(3, planes.dim())).contiguous()


def unlayout(kind, buf, dims):
    """The inverse: the weight in the shape of v, gathered from the buffer; for the split kinds hi + mid + lo in fp64."""
    shape, dest = INDEX[kind](*dims)
    if kind in SPLIT_KINDS:
        buf = buf.double().sum(dim=2)
    return buf.reshape(-1)[dest]


def buffer_shape(kind, dims):
    shape = INDEX[kind](*dims)[0]
    return shape if kind not in SPLIT_KINDS else shape[:2] + (3,) + shape[2:]


def compare(kind, dims, got, w):
    """What section 2 asserts of a packer's output `got` for the effective weight w; returns the failures."""
    fails = []
    want = layout(kind, w, dims)
    if not _same_bits(got, want):
        bad = (got.view(torch.int16 if kind in SPLIT_KINDS else torch.int32) != want.view(torch.int16 if kind in SPLIT_KINDS else torch.int32))
        fails.append(f"{int(bad.sum())} of {bad.numel()} slots differ from the documented layout, first at flat index "
                     f"{int(bad.reshape(-1).nonzero()[0])}")
    if kind in SPLIT_KINDS and not torch.equal(unlayout(kind, got, dims), w.double()):
        fails.append("hi + mid + lo != fl32(v * scale)")
    return fails


def _weights(shape, seed):
    """(v, g): v as the module docstring says, g (shape[0]) so that g / ||v[i]|| stays near 1."""
    gen = _g(seed)
    v = torch.randn(*shape, generator=gen) * torch.exp(3 * torch.randn(*shape, generator=gen))
    v = torch.where(v < 0, -1.0, 1.0) * v.abs().clamp(2.0 ** -96, 2.0 ** 96)
    if v[0].numel() > len(EDGES):
        v.view(-1)[:len(EDGES)] = torch.tensor(EDGES)
    norm = v.double().reshape(shape[0], -1).norm(dim=1)
    g = (torch.exp2(torch.round(torch.log2(norm))) * (0.5 + torch.rand(shape[0], generator=gen).double())).float()
    nz = v[v != 0].abs()
    assert float(nz.min()) >= 2.0 ** -96 and float(nz.max()) <= 2.0 ** 96
    return v.contiguous(), g.contiguous()


def _assert_splittable(w):
    nz = w[w != 0].abs().double()
    assert bool(torch.isfinite(w).all()) and (nz.numel() == 0 or (float(nz.min()) >= LO and float(nz.max()) < HI)), "test input out of range"


# ------------------------------------------------------------------------------------------------------- the cases
# kind -> [(id, dims, shape of v)]
def _conv_shape(d):
    return (d[0], d[1], d[2])


def _convtr_shape(d):
    return (d[0], d[1], 2 * d[2])


SPLIT64 = [(3, 5, 1), (3, 56, 64), (3, 64, 65), (3, 72, 1), (3, 72, 65), (5, 5, 64), (5, 56, 65), (5, 64, 1), (5, 72, 64), (5, 5, 65),
           (7, 5, 65), (7, 56, 1), (7, 64, 64), (7, 72, 65), (7, 64, 1)]          # (K, C_in, C_out)
CASES = {
    "conv_w": [("one", (1, 1, 1)), ("both_paddings_R15", (33, 5, 3)), ("cin_pads_to_96_R343_mid_tile", (40, 49, 7)),
               ("no_padding", (96, 48, 1)), ("pad_wider_than_pad32", (24, 24, 1, 64))],
    "convtr_w": [("one", (1, 1, 1)), ("s2", (5, 33, 2)), ("s5_cin_pads_to_96", (49, 40, 5)), ("s16", (24, 12, 16)),
                 ("s17_single_launch_only", (8, 8, 17))],
    "convtr_rows": [("one_full_tile", (24, 64, 2)), ("crosses_a_tile", (24, 65, 2)), ("cpt25_rows_125_127_empty", (5, 26, 5)),
                    ("s6_cin_pads_to_96", (49, 22, 6)), ("s3_cpt42", (7, 43, 3)), ("cpt1", (3, 2, 128))],
    "flip_t": [("one", (1, 1, 1)), ("k3", (33, 5, 3)), ("k7", (7, 40, 7))],
    "split_rows": [(f"rows64_k{K}_cin{ci}_G{bs_group(ci)}_cout{co}", (co, ci, K, 64)) for K, ci, co in SPLIT64]
                  + [("rows96_two_tiles_one_row", (97, 12, 7, 96)), ("rows96_exact", (96, 8, 7, 96))],
    "split2": [("plain_k9", (24, 8, 9, 0)), ("two_tiles_5_empty_lanes", (33, 3, 9, 9)), ("two_level_CV15", (8, 5, 27, 9)),
               ("k3_H4_one_zero_slot", (32, 16, 3, 3))],
    "gemm": [("k1_exact", (64, 64, 1, 1)), ("k1_two_tiles_cin33", (129, 33, 1, 1)), ("k2", (72, 40, 2, 1)),
             ("strided_k4_s2", (65, 33, 4, 2)), ("strided_k10_s5", (65, 33, 10, 5)), ("strided_k5_s3_zero_tap", (65, 33, 5, 3)),
             ("strided_k3_s2_zero_tap", (65, 33, 3, 2)), ("strided_k32_s16", (64, 32, 32, 16))],
}
V_SHAPE = dict(conv_w=_conv_shape, convtr_w=_convtr_shape, convtr_rows=_convtr_shape, flip_t=_conv_shape, split_rows=_conv_shape,
               split2=_conv_shape, gemm=_conv_shape)
ALL_CASES = [(kind, cid, dims) for kind, cs in CASES.items() for cid, dims in cs]
ALL_IDS = [f"{kind}-{cid}-{'x'.join(map(str, dims))}" for kind, cid, dims in ALL_CASES]


def _case_weights(kind, dims):
    return _weights(V_SHAPE[kind](dims), sum((i + 1) * d for i, d in enumerate(dims)) + len(kind))


# ------------------------------------------------------------------------------------------------------- CPU self-checks
@pytest.mark.parametrize("kind,cid,dims", ALL_CASES, ids=ALL_IDS)
def test_restatement_round_trips(kind, cid, dims):
    """unlayout(layout(w)) == w; the map is one-to-one, stays inside the buffer, and every slot it does not name is +0."""
    v, g = _case_weights(kind, dims)
    shape, dest = INDEX[kind](*dims)
    assert dest.shape == v.shape and int(dest.min()) >= 0 and int(dest.max()) < math.prod(shape)
    assert dest.unique().numel() == dest.numel()
    scale = g / v.reshape(v.shape[0], -1).norm(dim=1)
    for w in (v, effective(v, scale)):
        _assert_splittable(w)
        buf = layout(kind, w, dims)
        assert tuple(buf.shape) == buffer_shape(kind, dims)
        back = unlayout(kind, buf, dims)
        assert torch.equal(back, w.double() if kind in SPLIT_KINDS else w)
        assert compare(kind, dims, buf, w) == []
        words = buf.view(torch.int16 if kind in SPLIT_KINDS else torch.int32).reshape(-1)
        n_planes = 3 if kind in SPLIT_KINDS else 1
        assert int((words != 0).sum()) <= n_planes * int((w.view(torch.int32) != 0).sum())      # nothing but +0 off the map


def test_restated_constants_match_the_source():
    """Every constant the restatements use, read from the source text (no GPU)."""
    def const(path, name):
        m = re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, path)).read())
        assert m, (path, name)
        return int(m.group(1))

    assert const("conv1d_bsplit_kernel.h", "BS_CO") == BS_CO and const("conv1d_bsplit_kernel.h", "BS96_CO") == BS96_CO
    assert const("conv1d_bsplit_kernel.h", "BS_WIDE_MIN") == BS_WIDE_MIN
    assert const("conv1d_bsplit2.hip", "B2_CO") == B2_CO
    assert (const("conv1d_gemm_split.hip", "GS_ROWS"), const("conv1d_gemm_split.hip", "GS_CI"), const("conv1d_gemm_split.hip", "GS_RB")) \
        == (GS_ROWS, GS_CI, GS_RB)
    kh = open(os.path.join(CSRC, "conv1d_bsplit_kernel.h")).read()
    assert "constexpr int bs_group(int C_in) { return C_in >= BS_WIDE_MIN ? 2 : 1; }" in kh
    assert "constexpr int bs_slots(int K, int G) { return (G * K + 1) & ~1; }" in kh
    assert "constexpr int b2_slots(int K1) { return (K1 + 1) & ~1; }" in open(os.path.join(CSRC, "conv1d_bsplit2.hip")).read()
    assert all(bs_slots(K, G) == (G * K + 1) & ~1 for K in range(1, 9) for G in (1, 2)) and all(b2_slots(K) == (K + 1) & ~1 for K in range(1, 28))
    m = re.search(r"constexpr int cin_pad_dev\(int c\) \{ return \(\(c \+ (\d+)\) / (\d+)\) \* (\d+); \}", open(os.path.join(CSRC, "common.h")).read())
    assert m and [int(x) for x in m.groups()] == [CIN_PAD - 1, CIN_PAD, CIN_PAD]
    header = open(os.path.join(REPO, "include", "facodec_hip.h")).read()
    m = re.search(r"static inline int fac_cin_pad\(int c\) \{ return \(\(c \+ (\d+)\) / (\d+)\) \* (\d+);", header)
    assert m and [int(x) for x in m.groups()] == [CIN_PAD - 1, CIN_PAD, CIN_PAD]
    # fac_convtr_rows is an inline function of the header: its two lines, and the Python twin the wrappers allocate with
    assert re.search(r"fac_convtr_rows\(int C_out, int stride\) \{\s*const int cpt = 128 / stride;\s*return \(\(C_out \+ cpt - 1\) / cpt\) \* 128;", header)
    from facodec_amd import ops
    for _, dims in CASES["convtr_rows"]:
        assert ops.convtr_rows_pad(dims[1], dims[2]) == convtr_rows(dims[1], dims[2]) == buffer_shape("convtr_rows", dims)[2]
    assert all(ops.cin_pad(c) == cin_pad(c) and ops.pad32(c) == pad32(c) for c in (1, 32, 33, 47, 48, 49, 96, 97))
    # the layout sentences the index maps were written from
    assert "[co tile][stage][plane][half slot][64 co][8 ci] bf16" in open(os.path.join(CSRC, "conv1d_bsplit.hip")).read()
    assert "slot = tap-major, group-minor" in open(os.path.join(CSRC, "conv1d_bsplit.hip")).read()
    assert "[co tile of 32][chunk of 8 cv][plane][tap slot][32 co][8 cv] bf16" in open(os.path.join(CSRC, "conv1d_bsplit2.hip")).read()
    gs = open(os.path.join(CSRC, "conv1d_gemm_split.hip")).read()
    assert "[row tile][chunk][plane][tap][row 128][slot 4][8 bf16], slot = piece ^ ((row >> 2) & 3), piece = (ci % 32) / 8." in gs
    assert "chunk = (32 real channels, input phase p), p fastest; its K = 2 taps are" in gs


def test_restated_buffer_sizes_match_the_byte_count_functions():
    """The restated buffers have the sizes the host functions of the library give (they touch no device)."""
    lib = _lib.load()
    for _, d in CASES["split_rows"]:
        assert lib.fac_conv_w_split_rows_bytes(*d) == 2 * math.prod(buffer_shape("split_rows", d)), d
        if d[3] == BS_CO:
            assert lib.fac_conv_w_split_bytes(*d[:3]) == lib.fac_conv_w_split_rows_bytes(*d)
    for _, d in CASES["split2"]:
        assert lib.fac_conv_w_split2_bytes(*d) == 2 * math.prod(buffer_shape("split2", d)), d
    for _, d in CASES["gemm"] + [("t", (72, 40, 1, 1)), ("rows", (convtr_rows(26, 5), 40, 2, 1))]:
        assert lib.fac_gemm_w_split_bytes(*d) == 2 * math.prod(buffer_shape("gemm", d)), d
    assert lib.fac_conv_w_split_rows_bytes(64, 64, 5, 96) == -1 and lib.fac_conv_w_split_rows_bytes(64, 64, 7, 80) == -1


FAULTS = [  # (fault, kind, dims, with scale): each where the fault moves something
    ("swizzle_dropped", "gemm", (129, 33, 1, 1), False),
    ("group_major_slots", "split_rows", (65, 72, 7, 64), False),
    ("scale_from_row_in_tile", "split_rows", (65, 72, 7, 64), True),
    ("scale_from_row_in_tile", "gemm", (129, 33, 1, 1), True),
    ("scale_from_row_in_tile", "split2", (33, 3, 9, 9), True),
    ("mid_lo_swapped", "split_rows", (1, 5, 3, 64), False),
    ("mid_lo_swapped", "split2", (24, 8, 9, 0), False),
    ("mid_lo_swapped", "gemm", (64, 64, 1, 1), False),
    ("zero_half_slot_first", "split_rows", (1, 5, 3, 64), False),
    ("zero_half_slot_first", "split_rows", (97, 12, 7, 96), False),
]


@pytest.mark.parametrize("fault,kind,dims,scaled", FAULTS, ids=[f"{f}-{k}-{'x'.join(map(str, d))}" for f, k, d, _ in FAULTS])
def test_planted_faults_in_a_restatement_are_caught(fault, kind, dims, scaled):
    """A buffer built with one documented rule broken fails the comparison the GPU tests make (`compare`) against the sound
    restatement: the comparison can tell these layouts apart at these cases."""
    assert any(d == dims for _, d in CASES[kind])
    v, g = _case_weights(kind, dims)
    scale = g / v.reshape(v.shape[0], -1).norm(dim=1) if scaled else None
    w = effective(v, scale)
    wrong = layout(kind, effective(v, scale, kind, dims, fault), dims, fault=fault)
    assert compare(kind, dims, layout(kind, w, dims), w) == []
    fails = compare(kind, dims, wrong, w)
    assert fails and "documented layout" in fails[0], fails
    if fault == "mid_lo_swapped":
        assert len(fails) == 1                    # the sum of the planes cannot see it; the bits do
    elif fault == "scale_from_row_in_tile":
        assert len(fails) == 2


# ======================================================================================================= 2. each packer alone (GPU)
def _nwords(kind, dims):
    """4-byte words of the output."""
    if kind == "wn_scale":
        return dims[0]
    if kind == "conv_bwd":
        return cin_pad(dims[0]) * dims[2] * pad32(dims[1])
    n = math.prod(buffer_shape(kind, dims))
    return n // 2 if kind in SPLIT_KINDS else n


def _out_buffer(cuda, kind, dims):
    """(view, buffer, pad): the output inside canaries, every byte of it 0xFF (NaN as fp32 and as bf16)."""
    out, buf, pad = _canary((_nwords(kind, dims),), cuda)
    out.view(torch.uint8).fill_(0xFF)
    return out, buf, pad


def _launch(kind, dims, a, b, out, strides=None):
    """The C entry of `kind` (a = v, b = scale or NULL; for wn_scale b = g).  Recorded instead when the thread is recording."""
    if kind == "wn_scale":
        _call("fac_wn_scale", _p(a), _p(b), _p(out), dims[0], dims[1])
    elif kind == "conv_w":
        _call("fac_pack_conv_w", _p(a), _p(b), _p(out), dims[0], dims[1], dims[2], dims[3] if len(dims) > 3 else pad32(dims[0]))
    elif kind == "convtr_w":
        _call("fac_pack_convtr_w", _p(a), _p(b), _p(out), dims[0], dims[1], dims[2], pad32(dims[1]))
    elif kind == "convtr_rows":
        _call("fac_pack_convtr_w_rows", _p(a), _p(b), _p(out), *dims)
    elif kind == "flip_t":
        _call("fac_flip_transpose_w", _p(a), _p(b), _p(out), *dims)
    elif kind == "split_rows":
        _call("fac_pack_conv_w_split_rows", _p(a), _p(b), _p(out), *dims)
    elif kind == "split2":
        _call("fac_pack_conv_w_split2", _p(a), _p(b), _p(out), *dims)
    elif kind == "gemm":
        R, C_in, K, S = dims
        rs, cs, ks = strides or (C_in * K, K, 1)
        _call("fac_pack_gemm_w_split", _p(a), rs, cs, ks, _p(b), _p(out), R, C_in, K, S)
    elif kind == "conv_bwd":
        _call("fac_pack_conv_w_bwd", _p(a), _p(b), _p(out), dims[0], dims[1], dims[2], pad32(dims[1]))
    else:
        raise KeyError(kind)


def _read(kind, dims, out):
    """The output as the CPU tensor `layout` builds."""
    t = out.cpu()
    return (t.view(torch.bfloat16) if kind in SPLIT_KINDS else t).view(buffer_shape(kind, dims))


def _gpu_scale(cuda, v_d, g_d):
    """fac_wn_scale's own scale of (v, g) on the GPU, inside canaries."""
    n = v_d.shape[0]
    sc, buf, pad = _out_buffer(cuda, "wn_scale", (n,))
    _launch("wn_scale", (n, v_d.numel() // n), v_d, g_d, sc)
    torch.cuda.synchronize()
    assert _canary_intact(buf, pad), "fac_wn_scale wrote outside its output"
    return sc


def _pack_and_check(cuda, kind, dims, v, g, strides=None, logical=None, runs=(False, True)):
    """Both runs of one case (scale = NULL, scale = fac_wn_scale's); returns the raw outputs (device).  logical(w): the weight
    (R, C_in, K) the packer is to see when it reads w through `strides`."""
    v_d, g_d = v.to(cuda), g.to(cuda)
    outs = []
    for scaled in runs:
        sc_d = _gpu_scale(cuda, v_d, g_d) if scaled else None
        sc = sc_d.cpu().clone() if scaled else None
        out, buf, pad = _out_buffer(cuda, kind, dims)
        _launch(kind, dims, v_d, sc_d, out, strides)
        torch.cuda.synchronize()
        tag = f"{kind} {dims} scale={'wn_scale' if scaled else 'NULL'}"
        assert _canary_intact(buf, pad), f"{tag}: wrote outside its buffer"
        assert _same_bits(v_d, v) and _same_bits(g_d, g), f"{tag}: an input changed"
        if scaled:
            assert _same_bits(sc_d, sc) and bool(torch.isfinite(sc).all()), f"{tag}: the scale changed"
        w = effective(v, sc)
        _assert_splittable(w)
        fails = compare(kind, dims, _read(kind, dims, out), logical(w) if logical else w)
        assert not fails, (tag, fails)
        outs.append(out)
    return outs


@gpu
@pytest.mark.parametrize("kind,cid,dims", ALL_CASES, ids=ALL_IDS)
def test_packer_writes_the_documented_layout(cuda, kind, cid, dims):
    """The C entry alone, with scale = NULL and with fac_wn_scale's scale: the whole buffer bit for bit (padding +0, nothing left
    of the 0xFF fill), canaries intact, inputs unchanged, and for the split packs hi + mid + lo == fl32(v * scale) in fp64."""
    v, g = _case_weights(kind, dims)
    _pack_and_check(cuda, kind, dims, v, g)


@gpu
def test_gemm_pack_reads_a_transposed_weight_through_strides(cuda):
    """The read of ops.pack_gemm_weight_split_t: w (C_out, C_in, 1) = (40, 72, 1) packed as the 72 x 40 GEMM of the data gradient
    through (row_stride, ci_stride) = (1, C_in), without a row scale as the wrapper calls it (w is a materialised weight); the
    wrapper returns the same bits."""
    from facodec_amd import ops
    v, g = _weights((40, 72, 1), 11)
    dims = (72, 40, 1, 1)
    plain, = _pack_and_check(cuda, "gemm", dims, v, g, strides=(1, 72, 1), logical=lambda w: w.permute(1, 0, 2), runs=(False,))
    assert _same_bits(ops.pack_gemm_weight_split_t(v.to(cuda)).view(torch.int32), plain.view(torch.int32))


@gpu
def test_gemm_pack_reads_the_rows_buffer_of_a_transposed_conv(cuda):
    """The read of ops.pack_convtr_weight_rows_split at (C_in, C_out, s) = (40, 26, 5): the (cin_pad, 2, R) buffer of
    fac_pack_convtr_w_rows (its own case is above) read through row_stride = 1, the channels past C_in never touched; the
    wrapper, with g given, returns the bits of the restatement made with fac_wn_scale's scale."""
    from facodec_amd import ops
    c_in, c_out, s = 40, 26, 5
    v, g = _weights((c_in, c_out, 2 * s), 12)
    R = convtr_rows(c_out, s)
    dims = (R, c_in, 2, 1)
    v_d, g_d = v.to(cuda), g.to(cuda)
    sc_d = _gpu_scale(cuda, v_d, g_d)
    rows_out, rbuf, rpad = _out_buffer(cuda, "convtr_rows", (c_in, c_out, s))
    _launch("convtr_rows", (c_in, c_out, s), v_d, sc_d, rows_out)
    out, buf, pad = _out_buffer(cuda, "gemm", dims)
    _launch("gemm", dims, rows_out, None, out, strides=(1, 2 * R, R))
    torch.cuda.synchronize()
    assert _canary_intact(buf, pad) and _canary_intact(rbuf, rpad)
    rows = layout("convtr_rows", effective(v, sc_d.cpu()), (c_in, c_out, s))          # (cin_pad, 2, R)
    assert _same_bits(_read("convtr_rows", (c_in, c_out, s), rows_out), rows)
    w = rows[:c_in].permute(2, 0, 1).contiguous()                                    # the GEMM's weight (R, C_in, 2)
    assert compare("gemm", dims, _read("gemm", dims, out), w) == []
    got, r = ops.pack_convtr_weight_rows_split(v_d, g_d.view(-1, 1, 1), s)
    assert r == R and _same_bits(got.view(torch.int32), out.view(torch.int32))


WRAPPED = [("conv_w", (33, 5, 3)), ("convtr_w", (5, 33, 2)), ("convtr_rows", (5, 26, 5)), ("flip_t", (33, 5, 3)),
           ("split_rows", (65, 72, 7, 64)), ("split_rows", (97, 12, 7, 96)), ("split2", (8, 5, 27, 9)), ("gemm", (129, 33, 1, 1)),
           ("gemm", (65, 33, 5, 3))]


@gpu
@pytest.mark.parametrize("kind,dims", WRAPPED, ids=[f"{k}-{'x'.join(map(str, d))}" for k, d in WRAPPED])
def test_ops_wrapper_with_g_returns_the_bits_of_the_c_entry(cuda, kind, dims):
    """ops.pack_* with g given (it computes the scale itself) returns what the C entry wrote with fac_wn_scale's scale."""
    from facodec_amd import ops
    assert any(d == dims for _, d in CASES[kind])
    v, g = _case_weights(kind, dims)
    v_d, g_d = v.to(cuda), g.to(cuda)
    sc_d = _gpu_scale(cuda, v_d, g_d)
    out, buf, pad = _out_buffer(cuda, kind, dims)
    _launch(kind, dims, v_d, sc_d, out)
    g3 = g_d.view(-1, 1, 1)
    got = {"conv_w": lambda: ops.pack_conv_weight(v_d, g3), "convtr_w": lambda: ops.pack_convtr_weight(v_d, g3, dims[2]),
           "convtr_rows": lambda: ops.pack_convtr_weight_rows(v_d, g3, dims[2]), "flip_t": lambda: ops.flipped_weight(v_d, g3),
           "split_rows": lambda: ops.pack_conv_weight_split(v_d, g3, rows=dims[3]),
           "split2": lambda: ops.pack_conv_weight_split2(v_d, g3, dims[3]),
           "gemm": lambda: ops.pack_gemm_weight_split(v_d, g3, in_stride=dims[3])}[kind]()
    torch.cuda.synchronize()
    assert _canary_intact(buf, pad)
    assert got.numel() * got.element_size() == 4 * out.numel()
    assert _same_bits(got.reshape(-1).view(torch.int32), out.view(torch.int32))


# ======================================================================================================= 3. the recorded batch (GPU)
def _rc(name, *args):
    """(return code, fac_last_error text) of a C entry that may refuse."""
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    return rc, lib.fac_last_error().decode("utf-8", "replace")


class _Job:
    """One recordable call: its inputs on the device and two outputs (single launch, replay), both 0xFF-filled inside canaries."""

    def __init__(self, cuda, kind, dims, a, b, phase=0, strides=None):
        self.kind, self.dims, self.a, self.b, self.phase, self.strides, self.cuda = kind, dims, a, b, phase, strides, cuda
        self.single, self.sbuf, self.spad = _out_buffer(cuda, kind, dims)
        self.batch, self.bbuf, self.bpad = _out_buffer(cuda, kind, dims)

    def launch(self, out):
        _launch(self.kind, self.dims, self.a, self.b, out, self.strides)

    def refill(self):
        self.single.view(torch.uint8).fill_(0xFF)
        self.batch.view(torch.uint8).fill_(0xFF)


def _record(jobs, out=lambda j: j.batch):
    """Records the jobs in order (phase changes included) and returns the plan; the thread is left clean whatever happens."""
    lib = _lib.load()
    _lib.check(lib.fac_prep_begin(), "fac_prep_begin")
    try:
        phase = 0
        for j in jobs:
            if j.phase != phase:
                _lib.check(lib.fac_prep_set_phase(j.phase), "fac_prep_set_phase")
                phase = j.phase
            j.launch(out(j))
        plan = lib.fac_prep_end()
    except BaseException:
        lib.fac_prep_abort()
        raise
    assert plan >= 0, lib.fac_last_error()
    return plan


def _info(plan):
    n_jobs, n_launches = C.c_int(-1), C.c_int(-1)
    lib = _lib.load()
    _lib.check(lib.fac_prep_info(plan, C.byref(n_jobs), C.byref(n_launches)), "fac_prep_info")
    return n_jobs.value, n_launches.value


def _replay_equals_single(jobs, plan, single_out=lambda j: j.single, batch_out=lambda j: j.batch):
    """One replay against the single launches of the same jobs, in phase order: bits and canaries."""
    from facodec_amd import ops
    lib = _lib.load()
    for j in sorted(jobs, key=lambda j: j.phase):
        j.launch(single_out(j))
    _lib.check(lib.fac_prep_replay(plan, ops._stream()), "fac_prep_replay")
    torch.cuda.synchronize()
    for i, j in enumerate(jobs):
        tag = f"job {i} ({j.kind} {j.dims})"
        assert _canary_intact(j.sbuf, j.spad) and _canary_intact(j.bbuf, j.bpad), f"{tag}: wrote outside its buffer"
        s, b = j.single.cpu().view(torch.int32), j.batch.cpu().view(torch.int32)
        assert torch.equal(s, b), f"{tag}: {int((s != b).sum())} of {s.numel()} words of the replay differ from the single launch"
        assert not bool((b == -1).all()), f"{tag}: nothing was written"


def _dev_weights(cuda, shape, seed):
    v, g = _weights(shape, seed)
    return v.to(cuda), g.to(cuda)


ONE_JOB = [("wn_scale", (7, 33)), ("conv_w", (33, 5, 3)), ("convtr_w", (5, 33, 2)), ("convtr_rows", (5, 26, 5)), ("flip_t", (7, 40, 7)),
           ("split_rows", (65, 72, 7, 64)), ("gemm", (65, 33, 5, 3)), ("split2", (33, 3, 9, 9)), ("conv_bwd", (33, 5, 3))]


def _make_job(cuda, kind, dims, seed, phase=0):
    """A job of `kind` on fresh weights; the packs read a scale computed beforehand by a single fac_wn_scale launch."""
    if kind == "wn_scale":
        v_d, g_d = _dev_weights(cuda, (dims[0], dims[1]), seed)
        return _Job(cuda, kind, dims, v_d, g_d, phase)
    shape = V_SHAPE.get(kind, _conv_shape)(dims)
    v_d, g_d = _dev_weights(cuda, shape, seed)
    return _Job(cuda, kind, dims, v_d, _gpu_scale(cuda, v_d, g_d), phase)


@gpu
@pytest.mark.parametrize("kind,dims", ONE_JOB, ids=[k for k, _ in ONE_JOB])
def test_plan_of_one_job_replays_the_single_launch(cuda, kind, dims):
    """A plan holding one job of each PrepKind in turn (first = {0}, the search has nothing to halve)."""
    lib = _lib.load()
    job = _make_job(cuda, kind, dims, 20 + len(kind))
    plan = _record([job])
    try:
        assert _info(plan) == (1, 1)
        _replay_equals_single([job], plan)
    finally:
        _lib.check(lib.fac_prep_free(plan), "fac_prep_free")


@gpu
def test_forty_one_workgroup_jobs_find_their_own_job(cuda):
    """40 jobs of ONE workgroup each in one unit: prep_find_job runs at every boundary of a 40-entry table (first[j] = j), and
    each job has its own inputs, so a workgroup that picked a neighbour's job writes the wrong bits."""
    lib = _lib.load()
    jobs = []
    for i in range(40):
        if i % 2 == 0:
            jobs.append(_make_job(cuda, "wn_scale", (1, 1 + 37 * i), 100 + i))       # n_slices = 1: one workgroup
        else:
            jobs.append(_make_job(cuda, "flip_t", (1 + i % 3, 1 + i % 5, 1 + i % 7), 100 + i))   # at most 105 elements: one workgroup
    jobs[1] = _make_job(cuda, "flip_t", (1, 1, 1), 101)
    plan = _record(jobs)
    try:
        assert _info(plan) == (40, 1)
        _replay_equals_single(jobs, plan)
    finally:
        _lib.check(lib.fac_prep_free(plan), "fac_prep_free")


@gpu
def test_all_pack_kinds_in_one_phase_share_the_batch_kernels_lds(cuda):
    """The five kinds of pack.hip in one launch, the stride-16 fac_pack_convtr_w (whose 32 x (K + 1) floats are the batch kernel's
    whole sm[32 * 33]) between a wn_scale (four floats of it) and a pack_conv (its 32 x 33 tile): neighbouring workgroups use the
    shared array three ways."""
    lib = _lib.load()
    jobs = [_make_job(cuda, "convtr_rows", (5, 26, 5), 41), _make_job(cuda, "wn_scale", (7, 300), 42),
            _make_job(cuda, "convtr_w", (24, 12, 16), 43), _make_job(cuda, "conv_w", (33, 5, 3), 44),
            _make_job(cuda, "flip_t", (7, 40, 7), 45), _make_job(cuda, "convtr_w", (24, 12, 16), 46),
            _make_job(cuda, "wn_scale", (3, 5), 47)]
    plan = _record(jobs)
    try:
        assert _info(plan) == (len(jobs), 1)
        _replay_equals_single(jobs, plan)
        want = layout("convtr_w", effective(jobs[2].a.cpu(), jobs[2].b.cpu()), (24, 12, 16))
        assert _same_bits(_read("convtr_w", (24, 12, 16), jobs[2].batch), want)       # and the replay is the documented layout
    finally:
        _lib.check(lib.fac_prep_free(plan), "fac_prep_free")


@gpu
def test_three_phase_plan_follows_the_weights_current_contents(cuda):
    """The plan shape wprep produces: phase 0 the scale, phase 1 a split pack and the flipped weight reading that scale, phase 2
    the split pack of the flipped weight.  One launch per (phase, unit); after v is overwritten in place the next replay gives
    the packs of the new contents."""
    from facodec_amd import ops
    lib = _lib.load()
    c_out, c_in, K = 65, 72, 7
    v_d, g_d = _dev_weights(cuda, (c_out, c_in, K), 51)
    j_scale = _Job(cuda, "wn_scale", (c_out, c_in * K), v_d, g_d, phase=0)
    j_split = _Job(cuda, "split_rows", (c_out, c_in, K, 64), v_d, None, phase=1)
    j_flip = _Job(cuda, "flip_t", (c_out, c_in, K), v_d, None, phase=1)
    j_fsplit = _Job(cuda, "split_rows", (c_in, c_out, K, 64), None, None, phase=2)
    jobs = [j_scale, j_split, j_flip, j_fsplit]

    def wire(which):                                # every consumer reads its producer's output of the same chain
        j_split.b = j_flip.b = getattr(j_scale, which)
        j_fsplit.a = getattr(j_flip, which)

    wire("batch")
    plan = _record(jobs)
    try:
        assert _info(plan) == (4, 4)                # (0, pack), (1, pack), (1, bsplit), (2, bsplit)
        results = []
        for rnd in range(2):
            wire("single")
            for j in jobs:
                j.launch(j.single)
            wire("batch")
            _lib.check(lib.fac_prep_replay(plan, ops._stream()), "fac_prep_replay")
            torch.cuda.synchronize()
            for j in jobs:
                assert _canary_intact(j.sbuf, j.spad) and _canary_intact(j.bbuf, j.bpad)
                assert torch.equal(j.single.cpu().view(torch.int32), j.batch.cpu().view(torch.int32)), (rnd, j.kind, j.dims)
            w = effective(v_d.cpu(), j_scale.batch.cpu())
            assert compare("split_rows", j_split.dims, _read("split_rows", j_split.dims, j_split.batch), w) == []
            wf = layout("flip_t", w, (c_out, c_in, K))
            assert compare("split_rows", j_fsplit.dims, _read("split_rows", j_fsplit.dims, j_fsplit.batch), wf) == []
            results.append(j_fsplit.batch.cpu().clone())
            if rnd == 0:
                v_d.mul_(1.5).add_(0.25)            # the parameters move in place (an optimiser step)
                for j in jobs:
                    j.refill()
        assert not torch.equal(results[0].view(torch.int32), results[1].view(torch.int32))
    finally:
        _lib.check(lib.fac_prep_free(plan), "fac_prep_free")


# ======================================================================================================= 4. the recorder's refusals (CPU)
def test_recorder_and_packers_refuse_what_the_header_excludes():
    """Every refusal returns a negative code with its fac_last_error text; no device is touched (the arguments are checked before
    anything is launched or allocated), and fac_prep_abort leaves the thread clean after each."""
    lib = _lib.load()
    host = torch.zeros(64)
    a, o, null = _p(host), _p(host), C.c_void_p(0)
    n = C.c_int(0)

    def refused(got, text):
        rc, msg = got
        assert rc < 0 and text in msg, (rc, msg, text)
        assert lib.fac_prep_abort() == 0

    assert lib.fac_prep_abort() == 0
    assert lib.fac_prep_begin() == 0
    refused(_rc("fac_prep_begin"), "prep_begin: this thread is already recording")
    refused(_rc("fac_prep_set_phase", 1), "prep_set_phase: not recording, or a negative phase")
    refused(_rc("fac_prep_end"), "prep_end: not recording")
    assert lib.fac_prep_begin() == 0
    refused(_rc("fac_prep_set_phase", -1), "prep_set_phase: not recording, or a negative phase")
    assert lib.fac_prep_begin() == 0
    refused(_rc("fac_prep_end"), "prep_end: nothing was recorded")
    assert lib.fac_prep_begin() == 0
    refused(_rc("fac_pack_convtr_w", a, null, o, 8, 8, 17, 32, null), "pack_convtr_w: a recorded launch takes strides up to 16")
    refused(_rc("fac_prep_end"), "prep_end: not recording")          # the abort above ended that recording
    for plan in (-1, 1 << 20):
        refused(_rc("fac_prep_replay", plan, null), "prep_replay: no such plan")
        refused(_rc("fac_prep_info", plan, C.byref(n), C.byref(n)), "prep_info: no such plan")
        refused(_rc("fac_prep_free", plan), "prep_free: no such plan")
    refused(_rc("fac_pack_conv_w", a, null, o, 33, 5, 3, 40, null), "pack_conv_w: C_out_pad must be a multiple of 32")
    refused(_rc("fac_pack_conv_w", a, null, o, 33, 5, 3, 32, null), "pack_conv_w: C_out_pad must be a multiple of 32")   # 32 < C_out
    gemm_text = "pack_gemm_w_split: bad arguments (K must be 1 or 2, or in (S, 2S] for input stride S)"
    refused(_rc("fac_pack_gemm_w_split", a, 3, 3, 1, null, o, 1, 1, 3, 1, null), gemm_text)
    refused(_rc("fac_pack_gemm_w_split", a, 2, 2, 1, null, o, 1, 1, 2, 2, null), gemm_text)
    refused(_rc("fac_pack_conv_w_split2", a, null, o, 8, 5, 27, 8, null), "pack_conv_w_split2: bad arguments")
    refused(_rc("fac_pack_conv_w_split_rows", a, null, o, 64, 64, 5, 96, null), "pack_conv_w_split: no 96-row tile for K=5")
    refused(_rc("fac_pack_conv_w_split_rows", a, null, o, 64, 64, 7, 80, null), "pack_conv_w_split: no 80-row tile for K=7")
    refused(_rc("fac_prep_end"), "prep_end: not recording")          # and nothing above left a recording open


ENTRY_POINTS = ["fac_wn_scale", "fac_pack_conv_w", "fac_pack_convtr_w", "fac_pack_convtr_w_rows", "fac_flip_transpose_w",
                "fac_pack_conv_w_split_rows", "fac_pack_conv_w_split2", "fac_pack_gemm_w_split", "fac_pack_conv_w_bwd"]
PREP_ENTRIES = ["fac_prep_begin", "fac_prep_set_phase", "fac_prep_abort", "fac_prep_end", "fac_prep_replay", "fac_prep_info",
                "fac_prep_free"]
HOST_ENTRIES = ["fac_conv_w_split_rows_bytes", "fac_conv_w_split_bytes", "fac_conv_w_split2_bytes", "fac_gemm_w_split_bytes"]


def test_entry_points_of_this_file_are_declared():
    """Every C entry this file drives is declared in include/facodec_hip.h and bound in facodec_amd/_lib.py (the launching ones
    with a stream as their last argument), and every one of them is driven by a test here (runs without a GPU)."""
    header = open(os.path.join(REPO, "include", "facodec_hip.h")).read()
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "fac_adamw_step" in v)
    this = open(os.path.abspath(__file__)).read()
    for n in ENTRY_POINTS + PREP_ENTRIES + HOST_ENTRIES:
        assert n in table, n
        assert re.search(r"int(64_t)? %s\(" % n, header), n
    for n in ENTRY_POINTS:
        assert table[n][1][-1] is C.c_void_p, n
    called = {w.split(chr(34))[0] for w in this.split("_ca" + "ll(" + chr(34))[1:]}
    assert called == set(ENTRY_POINTS), called ^ set(ENTRY_POINTS)
    for n in PREP_ENTRIES + HOST_ENTRIES:
        assert "lib.%s(" % n in this, n
