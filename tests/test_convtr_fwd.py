"""The forward transposed conv (ops.conv_transpose1d / ops.conv_transpose1d_flat) in every layout against float64, by kernel name.

Same two-step check as tests/test_conv_fwd_epilogue.py, whose references and helpers this module imports:
Step A  the launch with `bias` (and `alpha_in` on the two fp32 layouts, the only ones that take it) against
        F.conv_transpose1d(snake64(x), w64, stride=s)[..., left:left + T s] + bias, `_sum_bound` with n = 2 C_in (two taps per output
        phase), extra = 3 on the bf16 planes, + 7 with the prologue (derivation: tests/test_conv_fwd_epilogue.py);
Step B  the launch with alpha_y2: its `y` is bit-identical to Step A's, and y2 is held to snake64(y_gpu.double(), alpha_y2) by `_bar`.
The transposed conv has no alpha_out / act / res (ops.conv_transpose1d sets none).

Layouts (ops.pack_convtr_for): polyphase -- causal, non-causal at s = 2, 5, 6 (phase_shift 1, 3, 3) and with a history column;
rows (all phases per tile on the 128 x 256 tile: the row_phases epilogue of conv1d_mfma.h); rows split (split GEMM kernel); rows on
the streaming kernel with taps (stride 2 only); flattened clips.  Every layout runs at s = 2 with even T (y_cs % 4 == 0: the float4
stores of the all-phases epilogues) and at s = 5 with odd T (y_cs odd: scalar stores throughout); the streaming kernel, which
exists at s = 2 only, at even and odd T; the flattened form is one signal of B (T + 1) columns, odd with B = 9.  Once per
all-phases layout the output is a view one float into a larger buffer.  The output sits inside a canary buffer (the flattened
form allocates its own).

has_history: x carries x[t0 - 1] as its first column, so its T + 1 columns give T s samples: those of columns 1 .. T of the full
transposed conv, its slice [s, s + T s).  With a zero first column that is the no-history output, which the CPU test below checks.
"""
# Measured on MI355X.  Step A, worst error / bound per layout and kernel: polyphase split reduction 0.065 (with history 0.063), tiles
# 0.141 (non-causal, s = 2), with the prologue 0.093; rows on the 128 x 256 tile 0.126, with the prologue 0.081; rows split 0.072;
# rows on the streaming kernel 0.124; flattened 0.074.  Step B (y2), worst GPU / fp32-CPU pair: polyphase 1.2e-7 / 8.9e-8, rows
# 1.2e-7 / 9.2e-8, rows split 1.2e-7 / 9.3e-8, streaming 1.0e-7 / 9.2e-8, flattened 1.0e-7 / 7.9e-8.  The `y` beside y2 was
# bit-identical to the plain launch's in every case.  Wall time: see tests/test_conv_fwd_epilogue.py (24 cases, under 1 s each).
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

from facodec_amd import convplan, ops
from test_conv_fwd_epilogue import _alpha, _buffer, _channel_scale, _intact, snake
from test_conv_launch_desc import _Spy
from test_conv_plan_cpu import assert_same_launch, convtr_launch, fake_operands
from test_train_kernels_gen import CANARY, _bar, _sum_bound

gpu = pytest.mark.gpu
POLY, ROWS, RSPLIT, RPWT, TFLAT = convplan.TR_POLYPHASE, convplan.TR_ROWS, convplan.TR_ROWS_SPLIT, convplan.TR_ROWS_PW_TAPS, convplan.TR_FLAT

# B clips of T columns (the history / zero column not counted), ci -> co at stride s; kern: substring of the kernel's name
Tr = namedtuple("Tr", "name B ci co T s causal layout history prologue kern split out1")


def _t(name, B, ci, co, T, s, causal=True, layout=POLY, history=False, prologue=False, kern="", split=False, out1=False):
    return Tr(name, B, ci, co, T, s, causal, layout, history, prologue, kern, split, out1)


CASES = [
    # ---- polyphase (fp32): few columns on the split-reduction kernel (its phase loop), more on a tile; with the prologue the tile
    _t("poly_s2_T50", 2, 20, 24, 50, 2, kern="skinny"),
    _t("poly_s5_T51", 2, 20, 24, 51, 5, kern="skinny"),
    _t("poly_s2_T330_tile", 2, 20, 24, 330, 2, kern="32x256"),
    _t("poly_s5_T331_tile", 2, 20, 72, 331, 5, kern="128x128"),
    _t("poly_s2_T50_ain", 2, 20, 24, 50, 2, prologue=True, kern="32x256"),
    _t("poly_s5_T51_ain", 2, 20, 40, 51, 5, prologue=True, kern="64x128"),
    _t("poly_s2_T50_noncausal", 2, 20, 24, 50, 2, causal=False, kern="32x256"),             # phase_shift 1
    _t("poly_s5_T51_noncausal", 2, 20, 24, 51, 5, causal=False, kern="32x256"),             # 3
    _t("poly_s6_T51_noncausal_ain", 2, 20, 40, 51, 6, causal=False, prologue=True, kern="64x128"),   # 3
    _t("poly_s2_T50_history", 2, 20, 24, 50, 2, history=True, kern="skinny"),
    _t("poly_s5_T51_history", 2, 20, 24, 51, 5, history=True, kern="skinny"),
    _t("poly_s5_T331_history_tile_ain", 2, 20, 24, 331, 5, history=True, prologue=True, kern="32x256"),
    # ---- rows (fp32): (channel, phase) rows on the 128 x 256 tile; 20 channels x 5 phases = one tile of 25 channels, 72 -> three
    _t("rows_s2_T70", 2, 24, 20, 70, 2, layout=ROWS, kern="128x256 (convtr"),
    _t("rows_s5_T71", 2, 24, 72, 71, 5, layout=ROWS, kern="128x256 (convtr"),
    _t("rows_s2_T70_ain", 2, 24, 72, 70, 2, layout=ROWS, prologue=True, kern="128x256 (convtr"),
    _t("rows_s5_T71_ain", 2, 24, 20, 71, 5, layout=ROWS, prologue=True, kern="128x256 (convtr"),
    _t("rows_s2_T70_out1", 2, 24, 20, 70, 2, layout=ROWS, kern="128x256 (convtr", out1=True),
    # ---- rows split: c_in >= 64, t_in >= 256, B t_in >= 1024
    _t("rows_split_s2_T256", 4, 64, 32, 256, 2, layout=RSPLIT, kern="gemm_split_kernel<2>", split=True),
    _t("rows_split_s5_T257", 4, 64, 40, 257, 5, layout=RSPLIT, kern="gemm_split_kernel<2>", split=True),
    _t("rows_split_s2_T256_out1", 4, 64, 32, 256, 2, layout=RSPLIT, kern="gemm_split_kernel<2>", split=True, out1=True),
    # ---- rows on the streaming kernel with taps: s = 2, C_in 2 <= 384; 256 rows -> 1536 column blocks = 16 clips x 96 (large)
    _t("rows_pwt_s2_T3042", 16, 32, 128, 3042, 2, layout=RPWT, kern="pwt_kernel<2 taps>", split=True),
    _t("rows_pwt_s2_T3041", 16, 32, 128, 3041, 2, layout=RPWT, kern="pwt_kernel<2 taps>", split=True),
    # ---- flattened: fewer than 256 columns per clip, 8 x 129 (T counts without the zero column in front of every clip)
    _t("flat_s2_8x129", 8, 64, 40, 128, 2, layout=TFLAT, kern="gemm_split_kernel<2>", split=True),
    _t("flat_s5_9x129", 9, 64, 40, 128, 5, layout=TFLAT, kern="gemm_split_kernel<2>", split=True),
]
IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def _desc(c, y2=False):
    operands = ("bias",) + (("alpha_in",) if c.prologue else ()) + (("y2", "alpha_y2") if y2 else ())
    if c.history:
        d = ops.convtr_desc(c.B, c.ci, c.T + 1, c.co, c.s, ops.pad32(c.co), True, True)
        return fake_operands(d, "w", *operands)
    return convtr_launch(c.layout, c.B, c.ci, c.T + (c.layout == TFLAT), c.co, c.s, c.causal, operands)


def ref_convtr(c, x, w, bias, alpha_in=None):
    """(c64, mag) of the trimmed transposed conv; with a history column the slice [s, s + T s) of the conv over all T + 1 columns."""
    x, w = x.double(), w.double()
    m_in = x.abs()
    if alpha_in is not None:
        a = alpha_in.double().view(1, -1, 1)
        m_in = x.abs() + torch.sin(a * x) ** 2 / (a + 1e-9)
        x = snake(x, alpha_in)
    left = c.s if c.history else (0 if c.causal else c.s - c.s // 2)
    c64 = F.conv_transpose1d(x, w, stride=c.s)[..., left:left + c.T * c.s]
    mag = F.conv_transpose1d(m_in, w.abs(), stride=c.s)[..., left:left + c.T * c.s]
    return c64 + bias.double().view(1, -1, 1), mag + bias.double().abs().view(1, -1, 1)


def _inputs(c):
    gen = torch.Generator().manual_seed(7000 + IDS.index(c.name))
    x = torch.randn(c.B, c.ci, c.T + c.history, generator=gen)
    w = torch.randn(c.ci, c.co, 2 * c.s, generator=gen) / (2 * c.ci) ** 0.5
    bias = torch.randn(c.co, generator=gen) * 0.5
    alpha_in = None
    if c.prologue:                                # the planted input row, as in tests/test_conv_fwd_epilogue.py
        alpha_in = _alpha(c.ci, gen)
        x[:, 1] *= 1e6
        w[1] *= 1e-6
    alpha_y2 = _alpha(c.co, gen)
    w[:, 1] *= 1e6                                # the output channel whose alpha_y2 is 1e-6
    return x, w, bias, alpha_in, alpha_y2


# ------------------------------------------------------------------------------------------------ CPU-only
def test_table_names_the_kernel_and_the_layout_of_every_case():
    bad = []
    for c in CASES:
        for y2 in (False, True):
            kid, name = ops.conv_variant(_desc(c, y2))
            if kid < 0 or c.kern not in name or ("bf16x3" in name) != c.split:
                bad.append((c.name, y2, kid, name))
    assert not bad, bad
    for c in CASES:
        if c.layout == RSPLIT:
            assert convplan.plan_convtr(c.ci, c.co, c.s, c.B, c.T).layout == RSPLIT, c.name
        elif c.layout == RPWT:
            assert convplan.plan_convtr(c.ci, c.co, c.s, c.B, c.T).layout == RPWT, c.name
        elif c.layout == TFLAT:
            assert convplan.plan_convtr(c.ci, c.co, c.s, c.B, c.T, flat_train_cols=c.T + 1).layout == TFLAT, c.name
            assert c.T + 1 < 256 and c.B * (c.T + 1) >= 1024
    # thresholds the table sits on
    P = convplan.plan_convtr
    assert P(64, 32, 2, 4, 255).layout != RSPLIT and P(63, 32, 2, 4, 256).layout != RSPLIT and P(64, 32, 2, 3, 256).layout != RSPLIT
    assert P(32, 128, 2, 16, 3040).layout != RPWT
    assert P(64, 40, 2, 7, 128, flat_train_cols=129).layout != TFLAT
    # what the table exists for
    by = lambda layout: [c for c in CASES if c.layout == layout]      # noqa: E731
    for layout in (POLY, ROWS, RSPLIT, TFLAT):
        assert {(c.s, c.T % 2) for c in by(layout)} >= {(2, 0), (5, 1)} or layout == TFLAT, layout
        assert any(c.s == 5 and (c.B * (c.T + 1) * c.s if layout == TFLAT else c.T * c.s) % 2 == 1 for c in by(layout)), layout
    assert {c.T % 2 for c in by(RPWT)} == {0, 1} and all(c.s == 2 for c in by(RPWT))
    assert {(c.s, c.s - c.s // 2) for c in CASES if not c.causal} == {(2, 1), (5, 3), (6, 3)}
    assert any(c.history for c in CASES) and {c.layout for c in CASES if c.prologue} == {POLY, ROWS}


def test_prologue_is_refused_outside_the_fp32_layouts():
    for name in ("rows_split_s2_T256", "rows_pwt_s2_T3042", "flat_s2_8x129"):
        c = BY_NAME[name]
        d = fake_operands(_desc(c), "alpha_in")
        kid, kname = ops.conv_variant(d)
        assert kid < 0 or "bf16x3" not in kname, (name, kname)      # refused (split-only weights) or off the plane kernels (fp32 rows)


def test_history_column_is_a_slice_of_the_full_transposed_conv():
    """has_history with a zero first column is the no-history launch: the reference's slice, checked without a GPU."""
    gen = torch.Generator().manual_seed(3)
    for s, T in ((2, 10), (5, 7)):
        c = _t("h", 2, 3, 4, T, s, history=True)
        x = torch.randn(2, 3, T, generator=gen)
        w, bias = torch.randn(3, 4, 2 * s, generator=gen), torch.randn(4, generator=gen)
        with_zero = ref_convtr(c, torch.cat([torch.zeros(2, 3, 1), x], 2), w, bias)[0]
        plain = ref_convtr(c._replace(history=False), x, w, bias)[0]
        assert with_zero.shape == (2, 4, T * s) and torch.equal(with_zero, plain)
        # and a non-zero history column adds W[p + s] x[t0 - 1] to the first s samples only
        h = torch.randn(2, 3, 1, generator=gen)
        got = ref_convtr(c, torch.cat([h, x], 2), w, bias)[0]
        add = torch.einsum("bi,iop->bop", h[..., 0].double(), w.double()[:, :, s:])
        assert torch.allclose(got[..., :s], plain[..., :s] + add, rtol=0, atol=1e-12) and torch.equal(got[..., s:], plain[..., s:])


def test_reference_agrees_with_the_fp32_oracle():
    from oracle import facodec_oracle as O
    gen = torch.Generator().manual_seed(4)
    for s, T, causal in ((2, 10, True), (5, 7, False), (6, 5, False)):
        c = _t("o", 2, 3, 4, T, s, causal=causal)
        x, w, bias = torch.randn(2, 3, T, generator=gen), torch.randn(3, 4, 2 * s, generator=gen), torch.randn(4, generator=gen)
        want = O.sconvtr1d(x, w, bias, s, causal=causal)
        got = ref_convtr(c, x, w, bias)[0]
        assert got.shape == want.shape and float((got - want.double()).abs().max()) <= 1e-5 * float(want.abs().max())


# ------------------------------------------------------------------------------------------------ GPU
def _run(c, dev, x, packed, bias, alpha_in, alpha_y2, off):
    kw = dict(bias=bias.to(dev), alpha_y2=alpha_y2.to(dev) if alpha_y2 is not None else None)
    if c.layout == TFLAT:
        xz = torch.cat([torch.zeros(c.B, c.ci, 1), x], 2).to(dev)          # the zero column in front of every clip
        got = ops.conv_transpose1d_flat(xz, packed, c.co, c.s, trim=c.s, **kw)
    else:
        out, buf, first, n = _buffer((c.B, c.co, c.T * c.s), dev, off)
        got = ops.conv_transpose1d(x.to(dev), packed, c.co, c.s, alpha_in=alpha_in.to(dev) if alpha_in is not None else None, out=out,
                                   causal=c.causal, has_history=c.history, **kw)
        torch.cuda.synchronize()
        assert _intact(buf, first, n), "canary"
    y, y2 = got if alpha_y2 is not None else (got, None)
    assert not bool((y == CANARY).any()) and (y2 is None or not bool((y2 == CANARY).any()))
    return y.cpu(), (y2.cpu() if y2 is not None else None)


@gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", IDS)
def test_convtr_fwd_against_fp64(name, cuda):
    c = BY_NAME[name]
    assert ops.BF16_SPLIT
    x, w, bias, alpha_in, alpha_y2 = _inputs(c)
    packed = ops.pack_convtr_for(c.layout, w.to(cuda), None, c.s)
    off = 1 if c.out1 else 0
    with _Spy() as spy:
        c_gpu, _ = _run(c, cuda, x, packed, bias, alpha_in, None, off)
        y, y2 = _run(c, cuda, x, packed, bias, alpha_in, alpha_y2, off)
    assert len(spy.launched) == 2
    names = [ops.conv_variant(d)[1] for d in spy.launched]
    assert names[0] == names[1] and c.kern in names[0] and ("bf16x3" in names[0]) == c.split, names
    assert_same_launch(spy.launched[0], _desc(c), name)
    assert_same_launch(spy.launched[1], _desc(c, y2=True), name)
    c64, mag = ref_convtr(c, x, w, bias, alpha_in)
    assert c_gpu.shape == c64.shape == (c.B, c.co, c.T * c.s)
    _sum_bound(f"convtr_fwd_sum_{name}", c_gpu, c64, mag, 2 * c.ci, extra=(3.0 if c.split else 0.0) + (7.0 if c.prologue else 0.0))
    assert torch.equal(y, c_gpu), "the launch with alpha_y2 does not share the plain launch's accumulator bits"
    y2_64 = snake(y.double(), alpha_y2)
    _bar(f"convtr_fwd_map_{name}_y2", y2, y2_64, snake(y, alpha_y2), scale=_channel_scale(y2_64))
