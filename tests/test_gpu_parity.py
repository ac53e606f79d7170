"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same seeded
inputs, and against the golden vectors produced by the real reference.

Bars (BASELINE.json north_star): code indices bit-exact; waveform / latents / losses within 1e-4
relative fp32.  Per-op tolerances below are tighter (1e-5) because single ops sit at the fp32
noise floor.
"""
import os

import numpy as np
import pytest
import torch

from facodec_amd import synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OP_TOL = 1e-5
E2E_TOL = 1e-4


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def O():
    from oracle import facodec_oracle
    return facodec_oracle


@pytest.fixture(scope="module")
def ops(cuda):
    from facodec_amd import ops as _ops
    from facodec_amd import _lib
    _lib.load()  # fails loudly if the extension is missing
    return _ops


def _g(seed=0):
    return torch.Generator().manual_seed(seed)


CONV_CASES = [
    # B, Cin, Cout, T, k, stride, dil, snake_in, snake_out, res, act, pad_mode
    (2, 64, 64, 1000, 7, 1, 1, False, False, False, 0, "reflect"),
    (2, 128, 128, 777, 7, 1, 3, True, True, False, 0, "reflect"),
    (1, 96, 96, 500, 7, 1, 9, True, False, False, 0, "reflect"),
    (2, 192, 192, 300, 1, 1, 1, False, False, True, 0, "reflect"),
    (2, 1, 64, 2400, 7, 1, 1, False, False, False, 0, "reflect"),
    (2, 64, 128, 2400, 4, 2, 1, True, False, False, 0, "reflect"),
    (2, 128, 256, 1201, 10, 5, 1, True, False, False, 0, "reflect"),   # ragged: extra right padding
    (1, 512, 1024, 960, 12, 6, 1, False, False, False, 0, "reflect"),
    (1, 1024, 1024, 160, 3, 1, 1, True, False, False, 0, "reflect"),
    (2, 96, 1, 3000, 7, 1, 1, True, False, False, 1, "reflect"),
    (1, 8, 16, 5, 7, 1, 1, False, False, False, 0, "reflect"),        # input shorter than the pad
    (3, 20, 256, 33, 1, 1, 1, False, False, False, 0, "zero"),
    (1, 1024, 1536, 160, 7, 1, 1, False, False, False, 0, "reflect"),
    (5, 256, 512, 32, 1, 1, 1, False, False, False, 0, "reflect"),     # narrow-N tile (LSTM projections)
    (1, 37, 45, 129, 5, 1, 2, True, True, True, 0, "reflect"),        # odd everything
    # few output columns, zero padding: the split-reduction ("skinny") kernel
    (1, 768, 768, 12, 7, 1, 3, False, True, True, 0, "zero"),
    (2, 1024, 1536, 2, 7, 1, 1, False, False, False, 0, "zero"),
    (3, 512, 1024, 30, 12, 6, 1, False, False, False, 1, "zero"),
    (1, 384, 200, 61, 7, 1, 9, False, True, True, 0, "zero"),         # C_out not a multiple of 128 / 32
    (8, 1024, 2048, 1, 1, 1, 1, False, False, False, 0, "zero"),      # per-clip Linear
    # one input channel (store-stream kernel) / one output channel (VALU kernel): ragged lengths, short taps, zero padding
    (3, 1, 64, 2051, 7, 1, 1, False, True, False, 0, "reflect"),
    (2, 1, 45, 1030, 3, 1, 1, False, False, False, 1, "zero"),
    (1, 1, 32, 5, 7, 1, 1, False, False, False, 0, "reflect"),
    (2, 50, 1, 1027, 3, 1, 1, False, False, False, 0, "zero"),
    (2, 24, 2, 2049, 9, 1, 1, True, False, False, 0, "reflect"),
    (140, 16, 1, 1500, 5, 1, 1, False, False, False, 0, "zero"),
    (2, 16, 24, 700, 9, 1, 2, True, False, False, 0, "reflect"),      # plain k = 9 / 27 on the run-time tap loop
    (1, 6, 32, 900, 27, 1, 1, False, False, False, 0, "zero"),
    # one / two output channels, too few tiles for the VALU kernel: channel-split partial sums + fixed-order sum
    (1, 1024, 1, 9001, 3, 1, 1, False, False, False, 0, "zero"),
    (2, 300, 2, 1500, 5, 1, 2, True, True, False, 1, "reflect"),
    # three to eight output channels over many input channels, 1 - 2 taps (round 6: the quantizer out-projections' data gradient)
    (16, 1024, 8, 160, 1, 1, 1, False, False, False, 0, "zero"),
    (3, 520, 5, 333, 2, 1, 1, False, True, False, 0, "zero"),
    (2, 256, 4, 700, 1, 1, 1, False, False, False, 1, "zero"),
    # one to four output columns, small weight matrix (round 6: the streaming hop's frame-rate layers on the single-launch VALU kernel)
    (1, 256, 512, 2, 5, 1, 1, False, False, False, 0, "zero"),
    (2, 256, 512, 2, 1, 1, 1, False, True, True, 0, "zero"),
    (1, 1025, 80, 1, 1, 1, 1, False, False, False, 1, "zero"),
    (1, 37, 45, 3, 5, 1, 2, False, True, True, 0, "reflect"),
    (4, 20, 256, 1, 1, 1, 1, False, False, False, 0, "zero"),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "B%d_%dto%d_T%d_k%d_s%d_d%d" % c[:7])
def test_conv1d_against_oracle(case, O, ops, cuda):
    B, ci, co, T, k, s, d, sin, sout, res, act, pad_mode = case
    g = _g(ci * 131 + co)
    x = torch.randn(B, ci, T, generator=g)
    w = torch.randn(co, ci, k, generator=g) / (ci * k) ** 0.5
    b = torch.randn(co, generator=g) * 0.1
    ai = 1 + 0.2 * torch.rand(ci, generator=g) if sin else None
    ao = 1 + 0.2 * torch.rand(co, generator=g) if sout else None
    xi = O.snake(x, ai.view(1, -1, 1)) if sin else x
    y = O.sconv1d(xi, w, b, stride=s, dilation=d, causal=True, pad_mode=pad_mode)
    if sout:
        y = O.snake(y, ao.view(1, -1, 1))
    if act == 1:
        y = torch.tanh(y)
    r = torch.randn(*y.shape, generator=g) if res else None
    if res:
        y = y + r
    wp = ops.pack_conv_weight(w.to(cuda))
    yg = ops.conv1d(x.to(cuda), wp, co, k, bias=b.to(cuda), stride=s, dilation=d,
                    pad_mode=ops.PAD_REFLECT if pad_mode == "reflect" else ops.PAD_ZERO,
                    alpha_in=ai.to(cuda) if sin else None, alpha_out=ao.to(cuda) if sout else None,
                    res=r.to(cuda) if res else None, act=act)
    assert yg.shape == y.shape
    assert rel(yg, y) < OP_TOL


@pytest.mark.parametrize("B,T", [(1, 1), (1, 2), (2, 2), (3, 2)])
def test_wavenet_layer_epilogues_in_the_conv_match_the_elementwise_kernels(B, T, ops, cuda):
    """FAC_ACT_GATE / FAC_ACT_WN_RES_SKIP (the gate and the residual / skip adds of a WaveNet layer, modules/wavenet.py:138-166, as
    epilogues of its two convs in a streaming hop) against conv + fac_gate_tanh_sigmoid / fac_wn_res_skip, bit for bit, plus the
    pre-activated second output on the same few-column launches; B * T <= 4 takes the single-launch kernel, B * T = 6 the
    split-reduction pair."""
    g = _g(17 + B + T)
    H = 256
    h = torch.randn(B, H, T + 4, generator=g).to(cuda)
    w_in = ops.pack_conv_weight((torch.randn(2 * H, H, 5, generator=g) / (5 * H) ** 0.5).to(cuda))
    b_in = (torch.randn(2 * H, generator=g) * 0.1).to(cuda)
    w_rs = ops.pack_conv_weight((torch.randn(2 * H, H, 1, generator=g) / H ** 0.5).to(cuda))
    b_rs = (torch.randn(2 * H, generator=g) * 0.1).to(cuda)
    kw = dict(pad_left=0, pad_mode=ops.PAD_ZERO, t_out=T)
    a = ops.conv1d(h, w_in, 2 * H, 5, bias=b_in, **kw)
    acts_ref = ops.gate_tanh_sigmoid(a)
    acts = ops.conv1d(h, w_in, 2 * H, 5, bias=b_in, act=ops.ACT_GATE, **kw)
    assert acts.shape == (B, H, T) and torch.equal(acts, acts_ref)
    x0 = torch.randn(B, H, T, generator=g).to(cuda)
    out0 = torch.randn(B, H, T, generator=g).to(cuda)
    x_ref, out_ref = x0.clone(), out0.clone()
    ops.wn_res_skip_(ops.conv1d(acts, w_rs, 2 * H, 1, bias=b_rs, **kw), x_ref, out_ref, last=False)
    x_got, out_got = x0.clone(), out0.clone()
    ops.conv1d(acts, w_rs, 2 * H, 1, bias=b_rs, res=x_got, out=x_got, skip_acc=out_got, act=ops.ACT_WN_RES_SKIP, **kw)
    assert torch.equal(x_got, x_ref) and torch.equal(out_got, out_ref)
    al = (1 + 0.2 * torch.rand(2 * H, generator=g)).to(cuda)
    y, y2 = ops.conv1d(acts, w_rs, 2 * H, 1, bias=b_rs, alpha_y2=al, **kw)
    assert torch.equal(y, ops.conv1d(acts, w_rs, 2 * H, 1, bias=b_rs, **kw)) and rel(y2, ops.snake(y, al)) < 1e-6


@pytest.mark.parametrize("B,ci,co,T,s", [(2, 256, 128, 160, 6), (2, 128, 64, 333, 5), (1, 192, 96, 1000, 2), (1, 24, 12, 7, 5)])
def test_conv_transpose_against_oracle(B, ci, co, T, s, O, ops, cuda):
    g = _g(s)
    x = torch.randn(B, ci, T, generator=g)
    v = torch.randn(ci, co, 2 * s, generator=g) / (ci * 2) ** 0.5
    gg = torch.rand(ci, 1, 1, generator=g) + 0.5
    b = torch.randn(co, generator=g) * 0.1
    al = 1 + 0.2 * torch.rand(ci, generator=g)
    y = O.sconvtr1d(O.snake(x, al.view(1, -1, 1)), O.weight_norm_weight(v, gg), b, s, causal=True)
    wp = ops.pack_convtr_weight(v.to(cuda), gg.to(cuda), s)
    yg = ops.conv_transpose1d(x.to(cuda), wp, co, s, bias=b.to(cuda), alpha_in=al.to(cuda))
    assert yg.shape == y.shape and rel(yg, y) < OP_TOL


@pytest.mark.parametrize("B,ci,co,T,s", [(1, 1536, 768, 2, 6), (1, 256, 128, 1, 6), (2, 128, 60, 2, 5), (1, 24, 12, 3, 2), (1, 768, 384, 12, 5)])
def test_conv_transpose_with_few_columns(B, ci, co, T, s, O, ops, cuda):
    """The polyphase ConvTranspose1d on 1 - 4 input frames (the streaming hop's first upsampling layer at B = 1: the single-launch
    VALU kernel, one workgroup row per phase) and on 12 (split-reduction pair), with the pre-activated second output."""
    g = _g(60 + s + T)
    x = torch.randn(B, ci, T, generator=g)
    v = torch.randn(ci, co, 2 * s, generator=g) / (ci * 2) ** 0.5
    gg = torch.rand(ci, 1, 1, generator=g) + 0.5
    b = torch.randn(co, generator=g) * 0.1
    al = 1 + 0.2 * torch.rand(co, generator=g)
    y = O.sconvtr1d(x, O.weight_norm_weight(v, gg), b, s, causal=True)
    wp = ops.pack_convtr_weight(v.to(cuda), gg.to(cuda), s)
    yg, y2 = ops.conv_transpose1d(x.to(cuda), wp, co, s, bias=b.to(cuda), alpha_y2=al.to(cuda))
    assert yg.shape == y.shape and rel(yg, y) < OP_TOL
    assert rel(y2, O.snake(y, al.view(1, -1, 1))) < OP_TOL


@pytest.mark.parametrize("B,ci,co,T,s", [(2, 192, 96, 1000, 2), (2, 96, 40, 777, 5), (1, 128, 64, 1333, 6), (3, 64, 22, 512, 3)])
def test_conv_transpose_all_phases_launch(B, ci, co, T, s, O, ops, cuda):
    """The all-phases-per-workgroup ConvTranspose1d (fac_conv_desc.row_phases: (channel, phase) rows, phases interleaved
    through the LDS epilogue, contiguous stores) against the oracle and against the polyphase launch, with bias, Snake
    prologue and the pre-activated second output; channel counts that do not fill the 128 / stride channels of a tile,
    ragged last time tile."""
    g = _g(40 + s)
    x = torch.randn(B, ci, T, generator=g)
    v = torch.randn(ci, co, 2 * s, generator=g) / (ci * 2) ** 0.5
    gg = torch.rand(ci, 1, 1, generator=g) + 0.5
    b = torch.randn(co, generator=g) * 0.1
    al = 1 + 0.2 * torch.rand(ci, generator=g)
    a2 = 1 + 0.2 * torch.rand(co, generator=g)
    y = O.sconvtr1d(O.snake(x, al.view(1, -1, 1)), O.weight_norm_weight(v, gg), b, s, causal=True)
    wr = ops.pack_convtr_weight_rows(v.to(cuda), gg.to(cuda), s)
    assert wr.dim() == 3 and wr.shape[-1] == ops.convtr_rows_pad(co, s)
    yg, y2 = ops.conv_transpose1d(x.to(cuda), wr, co, s, bias=b.to(cuda), alpha_in=al.to(cuda), alpha_y2=a2.to(cuda))
    assert yg.shape == y.shape and rel(yg, y) < OP_TOL
    assert rel(y2, O.snake(y, a2.view(1, -1, 1))) < OP_TOL
    yp = ops.conv_transpose1d(x.to(cuda), ops.pack_convtr_weight(v.to(cuda), gg.to(cuda), s), co, s, bias=b.to(cuda), alpha_in=al.to(cuda))
    assert rel(yg, yp) < 1e-6
    # opt-in (FAC_CONVTR_ROWS=1): measured slower than the polyphase launch on the fp32 pipe, the default all-phases path is
    # the split-bf16 GEMM (test_conv_transpose_on_split_gemm)
    prev = ops.CONVTR_ROWS
    try:
        ops.CONVTR_ROWS = True
        assert ops.convtr_rows_ok(T, s) and ops.convtr_weight_for(v.to(cuda), gg.to(cuda), s, T, alpha_in=al).dim() == 3
        ops.CONVTR_ROWS = False
        assert ops.convtr_weight_for(v.to(cuda), gg.to(cuda), s, T, alpha_in=al).dim() == 4
    finally:
        ops.CONVTR_ROWS = prev


def test_conv_second_output_is_snake_of_first(O, ops, cuda):
    """y2 = snake(y, alpha_y2) (the pre-activated copy a following Snake->conv consumes by LDS-DMA);
    also exercises the pure-DMA input path (no Snake prologue, interior tiles) against the oracle."""
    g = _g(21)
    x = torch.randn(2, 96, 5000, generator=g)
    w = torch.randn(96, 96, 7, generator=g) / 26.0
    b = torch.randn(96, generator=g) * 0.1
    r = torch.randn(2, 96, 5000, generator=g)
    a2 = 1 + 0.2 * torch.rand(96, generator=g)
    y_ref = O.sconv1d(x, w, b, dilation=3) + r
    wp = ops.pack_conv_weight(w.to(cuda))
    y, y2 = ops.conv1d(x.to(cuda), wp, 96, 7, bias=b.to(cuda), dilation=3, res=r.to(cuda), alpha_y2=a2.to(cuda))
    assert rel(y, y_ref) < OP_TOL and rel(y2, O.snake(y_ref, a2.view(1, -1, 1))) < OP_TOL
    none_y, y2b = ops.conv1d(x.to(cuda), wp, 96, 7, bias=b.to(cuda), dilation=3, res=r.to(cuda), alpha_y2=a2.to(cuda),
                             want_y=False)
    assert none_y is None and torch.equal(y2b, y2)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("C,T,B", [(64, 4101, 64), (96, 4101, 64), (128, 4099, 32), (192, 4100, 32), (256, 2100, 64), (384, 1101, 64)])
def test_pointwise_streaming_kernel(C, T, B, split, O, ops, cuda, monkeypatch):
    """k = 1 ResidualUnit tail on the streaming kernels (weights resident in LDS, inputs straight from global memory): bias +
    residual + second Snake output, ragged last column block, against the oracle; then the data-gradient form (no bias /
    residual, transposed weights).  split=False: conv1d_pw.hip, fp32 MFMAs, BIT-EQUAL to the tiled kernel (same summation
    order).  split=True (the default policy): C <= 192 on conv1d_pw_split.hip (both operands as three bf16 planes split inside
    the kernel, fp32-grade), wider layers unchanged."""
    monkeypatch.setattr(ops, "PW_SPLIT", split)
    g = _g(C + T)
    x = torch.randn(B, C, T, generator=g)
    w = torch.randn(C, C, 1, generator=g) / C ** 0.5
    b = torch.randn(C, generator=g) * 0.1
    r = torch.randn(B, C, T, generator=g)
    a2 = 1 + 0.2 * torch.rand(C, generator=g)
    y_ref = O.sconv1d(x, w, b) + r
    wp = ops.pack_conv_weight(w.to(cuda))
    prof = ops.ConvLaunchProfile()
    ops.set_conv_profile(prof)
    try:
        y, y2 = ops.conv1d(x.to(cuda), wp, C, 1, bias=b.to(cuda), res=r.to(cuda), alpha_y2=a2.to(cuda))
        # few columns: the same layer on the tiled kernel (the streaming kernels want a chip's worth of column blocks)
        n = 3
        y_t, y2_t = ops.conv1d(x[:n].to(cuda), wp, C, 1, bias=b.to(cuda), res=r[:n].to(cuda), alpha_y2=a2.to(cuda))
        dx = ops.conv1d(x.to(cuda), ops.pack_conv_weight_bwd(w.to(cuda)), C, 1, pad_left=0, pad_mode=ops.PAD_ZERO, t_out=T)
    finally:
        ops.set_conv_profile(None)
    names = [rec[0] for rec in prof.records]
    want = "conv1d_pws_kernel" if split else "conv1d_pw_kernel"
    assert names[0].startswith(want) and names[2].startswith(want) and "pw" not in names[1], names
    assert rel(y, y_ref) < OP_TOL and rel(y2, O.snake(y_ref, a2.view(1, -1, 1))) < OP_TOL
    if want == "conv1d_pw_kernel":
        assert torch.equal(y_t, y[:n]) and torch.equal(y2_t, y2[:n])
    else:
        # fp32-grade: as close to the fp64 answer as the fp32 tile is (the split drops only the lo*lo, lo*mid and mid*lo products)
        y64 = torch.einsum("oc,bct->bot", w[:, :, 0].double(), x[:n].double()) + b.double().view(1, -1, 1) + r[:n].double()
        e_split, e_tile = rel(y[:n].double(), y64), rel(y_t.double(), y64)
        assert e_split < 2e-6 and e_split < 4 * e_tile + 1e-7, (e_split, e_tile)
    assert rel(dx, torch.einsum("oc,bot->bct", w[:, :, 0], x)) < OP_TOL


@pytest.mark.parametrize("B,T", [(32, 4101), (64, 2050)])
def test_streaming_taps_kernel_conv_transpose_stride2(B, T, O, ops, cuda, monkeypatch):
    """The decoder's last ConvTranspose1d (192 -> 96, stride 2: dac/model/dac.py:107-128) on the streaming kernel with taps
    (conv1d_pw_split.hip, conv1d_pwt_kernel: both phases as rows, 8-byte interleaved stores), bias + pre-activated second output,
    ragged last column block, against the oracle and against the tiled all-phases launch; and the data-gradient shape of the
    encoder's first downsampling conv (128 -> 64, stride 2)."""
    for ci, co in ((192, 96), (128, 64)):
        g = _g(ci + T)
        x = torch.randn(B, ci, T, generator=g)
        v = torch.randn(ci, co, 4, generator=g) / (ci * 2) ** 0.5
        gg = torch.rand(ci, 1, 1, generator=g) + 0.5
        b = torch.randn(co, generator=g) * 0.1
        al = 1 + 0.2 * torch.rand(co, generator=g)
        y_ref = O.sconvtr1d(x, O.weight_norm_weight(v, gg), b, 2, causal=True)
        assert ops.pw_taps_ok(ci, co, 4, 2, True, B, T)
        wp = ops.pack_convtr_weight_rows(v.to(cuda), gg.to(cuda), 2)
        prof = ops.ConvLaunchProfile()
        ops.set_conv_profile(prof)
        try:
            y, y2 = ops.conv_transpose1d(x.to(cuda), wp, co, 2, bias=b.to(cuda), alpha_y2=al.to(cuda))
            monkeypatch.setattr(ops, "PW_TAPS", False)
            yt, y2t = ops.conv_transpose1d(x.to(cuda), wp, co, 2, bias=b.to(cuda), alpha_y2=al.to(cuda))
            monkeypatch.setattr(ops, "PW_TAPS", True)
        finally:
            ops.set_conv_profile(None)
        names = [rec[0] for rec in prof.records]
        assert names[0].startswith("conv1d_pwt_kernel") and "pwt" not in names[1], names
        assert y.shape == y_ref.shape and rel(y, y_ref) < OP_TOL and rel(y2, O.snake(y_ref, al.view(1, -1, 1))) < OP_TOL
        assert rel(y, yt) < 2e-6 and rel(y2, y2t) < 2e-6


@pytest.mark.parametrize("B,T", [(32, 8203), (64, 4100), (32, 8201)])
def test_streaming_taps_kernel_strided_conv(B, T, O, ops, cuda, monkeypatch):
    """The encoder's first downsampling conv (64 -> 128, k = 4, stride 2, causal reflect padding: dac/model/dac.py:45-66) and the
    data-gradient shape of the decoder's last ConvTranspose1d (96 -> 192) on the streaming kernel with taps; odd lengths exercise
    the extra right padding of dac/model/encodec.py:212-228."""
    for ci, co in ((64, 128), (96, 192)):
        g = _g(ci + T)
        x = torch.randn(B, ci, T, generator=g)
        w = torch.randn(co, ci, 4, generator=g) / (ci * 4) ** 0.5
        b = torch.randn(co, generator=g) * 0.1
        al = 1 + 0.2 * torch.rand(co, generator=g)
        y_ref = O.sconv1d(x, w, b, stride=2, causal=True)
        assert ops.pw_taps_ok(ci, co, 4, 2, False, B, y_ref.shape[-1])
        wp = ops.pack_conv_weight(w.to(cuda))
        prof = ops.ConvLaunchProfile()
        ops.set_conv_profile(prof)
        try:
            y, y2 = ops.conv1d(x.to(cuda), wp, co, 4, bias=b.to(cuda), stride=2, alpha_y2=al.to(cuda))
            monkeypatch.setattr(ops, "PW_TAPS", False)
            yt = ops.conv1d(x.to(cuda), wp, co, 4, bias=b.to(cuda), stride=2)
            monkeypatch.setattr(ops, "PW_TAPS", True)
        finally:
            ops.set_conv_profile(None)
        names = [rec[0] for rec in prof.records]
        assert names[0].startswith("conv1d_pwt_kernel") and "pwt" not in names[1], names
        assert y.shape == y_ref.shape and rel(y, y_ref) < OP_TOL and rel(y2, O.snake(y_ref, al.view(1, -1, 1))) < OP_TOL
        assert rel(y, yt) < 2e-6


def test_first_conv_two_outputs(O, ops, cuda):
    """Encoder input conv (1 -> 64, k = 7: dac/model/dac.py:84) with the pre-activated second output, ragged length (scalar
    tail stores) and the y2-only form."""
    g = _g(33)
    x = torch.randn(3, 1, 4098, generator=g)
    w = torch.randn(64, 1, 7, generator=g) / 2.6
    b = torch.randn(64, generator=g) * 0.1
    a2 = 1 + 0.2 * torch.rand(64, generator=g)
    y_ref = O.sconv1d(x, w, b)
    wp = ops.pack_conv_weight(w.to(cuda))
    y, y2 = ops.conv1d(x.to(cuda), wp, 64, 7, bias=b.to(cuda), alpha_y2=a2.to(cuda))
    assert rel(y, y_ref) < OP_TOL and rel(y2, O.snake(y_ref, a2.view(1, -1, 1))) < OP_TOL
    none_y, y2b = ops.conv1d(x.to(cuda), wp, 64, 7, bias=b.to(cuda), alpha_y2=a2.to(cuda), want_y=False)
    assert none_y is None and torch.equal(y2b, y2)


def test_conv_is_linear_in_its_input(ops, cuda):
    """Size-independent property at a full-size layer shape: conv(a x1 + b x2) == a conv(x1) + b conv(x2)."""
    g = _g(9)
    w = torch.randn(192, 192, 7, generator=g).to(cuda) / 36.0
    wp = ops.pack_conv_weight(w)
    x1 = torch.randn(2, 192, 24000, generator=g).to(cuda)
    x2 = torch.randn(2, 192, 24000, generator=g).to(cuda)
    y = ops.conv1d(2.0 * x1 + 0.5 * x2, wp, 192, 7, dilation=9)
    y12 = 2.0 * ops.conv1d(x1, wp, 192, 7, dilation=9) + 0.5 * ops.conv1d(x2, wp, 192, 7, dilation=9)
    assert rel(y, y12) < 1e-5


def test_weight_norm_packing(O, ops, cuda):
    g = _g(3)
    v = torch.randn(96, 48, 7, generator=g)
    gg = torch.rand(96, 1, 1, generator=g) + 0.5
    wp = ops.pack_conv_weight(v.to(cuda), gg.to(cuda))
    assert wp.shape == (48, 7, 96)                               # C_in 48 is already a multiple of 48
    assert rel(wp.permute(2, 0, 1), O.weight_norm_weight(v, gg)) < 1e-6
    sc = ops.wn_scale(v.to(cuda), gg.to(cuda)).cpu()             # exact against fl32(v * scale): the pack is one fp32 multiply
    assert torch.equal(wp.permute(2, 0, 1).cpu(), v * sc.view(-1, 1, 1))      # (every layout and edge: tests/test_weight_packs.py)
    v2 = torch.randn(40, 8, 1, generator=g)                      # C_out padded 40 -> 64, C_in 8 -> 48 with zeros
    wp2 = ops.pack_conv_weight(v2.to(cuda))
    assert wp2.shape == (48, 1, 64)
    assert float(wp2[:, :, 40:].abs().max()) == 0.0 and float(wp2[8:].abs().max()) == 0.0
    assert rel(wp2[:8, 0, :40].t(), v2[:, :, 0]) == 0.0


def test_snake_standalone(O, ops, cuda):
    g = _g(4)
    x = torch.randn(2, 33, 777, generator=g) * 3
    al = 1 + 0.3 * torch.rand(33, generator=g)
    assert rel(ops.snake(x.to(cuda), al.to(cuda)), O.snake(x, al.view(1, -1, 1))) < 1e-6


@pytest.mark.parametrize("B,H,T", [(3, 128, 20), (32, 256, 40), (2, 1024, 16), (33, 64, 5)])
def test_slstm_against_oracle(B, H, T, O, cuda):
    from facodec_amd.layers import SLSTM
    m = SLSTM(H, 2)
    sd = synth.load_synthetic(m, seed=5)
    x = torch.randn(B, H, T, generator=_g(H))
    y = O.slstm(x, sd, "lstm.", 2)
    with torch.no_grad():
        yg = m.to(cuda)(x.to(cuda))
    assert rel(yg, y) < OP_TOL


def test_vq_search_known_answers_and_sweep(ops, cuda, golden_dir):
    """Bit-exact code indices on the reference's own answers: ties -> lowest index, zero latent,
    262 144 random vectors (0 mismatches required)."""
    d = np.load(os.path.join(golden_dir, "vq_kat.npz"))
    cb = torch.from_numpy(d["codebook"]).to(cuda)
    lat = torch.from_numpy(d["latents"])
    idx = ops.vq_search(lat.permute(0, 2, 1).reshape(-1, 8).contiguous().to(cuda), cb).cpu().reshape(4, 300)
    assert torch.equal(idx, torch.from_numpy(d["indices"].astype(np.int64)))
    g = np.random.Generator(np.random.Philox(key=int(d["sweep_key"])))
    g.standard_normal((1024, 8)); g.standard_normal((4, 8, 300))
    big = torch.from_numpy(g.standard_normal((1, 8, 1 << 18)).astype(np.float32))
    idx2 = ops.vq_search(big[0].t().contiguous().to(cuda), cb).cpu()
    assert torch.equal(idx2, torch.from_numpy(d["sweep_indices"].astype(np.int64)))


def test_vq_search_idempotent_on_codebook_rows(ops, cuda):
    """Property: quantizing a codebook row returns that row's index (rows distinct)."""
    cb = torch.randn(1024, 8, generator=_g(11)).to(cuda)
    idx = ops.vq_search(cb * 3.7, cb).cpu()
    assert torch.equal(idx, torch.arange(1024))


@pytest.mark.parametrize("B,D,T,n", [(3, 256, 150, 3), (1, 64, 7, 1), (2, 1024, 160, 2), (5, 72, 17, 2), (1, 1024, 33, 1), (9, 128, 16, 3)])
def test_rvq_forward_against_oracle(B, D, T, n, O, cuda):
    from facodec_amd.quantize import ResidualVectorQuantize
    m = ResidualVectorQuantize(D, n, 1024, 8).eval()
    sd = synth.load_synthetic(m, seed=2)
    z = torch.randn(B, D, T, generator=_g(D + T))
    zq, codes, lat, cm, cb = O.rvq_forward(z, sd, "", n, n)
    with torch.no_grad():
        zq_g, codes_g, lat_g, cm_g, cb_g = m.to(cuda)(z.to(cuda), n)
    assert torch.equal(codes_g.cpu(), codes)
    assert rel(zq_g, zq) < OP_TOL and rel(lat_g, lat) < OP_TOL
    assert abs(float(cm_g) - float(cm)) / float(cm) < 1e-5 and abs(float(cb_g) - float(cb)) / float(cb) < 1e-5


@pytest.mark.parametrize("B,D,T", [(3, 1024, 8), (2, 256, 5), (33, 512, 1)])
def test_vq_tile_kernel_is_bit_identical_to_the_per_frame_kernel(B, D, T, ops, cuda):
    """fac_vq_fwd has two kernels: 16 frames per workgroup (offline; round 5: 64 before) and one workgroup per frame (streaming
    hops, T <= 8 without loss partials).  Both keep the in-proj's four sequential channel-quarter FMA chains, the strict '>'
    first-index scan and the per-element out-proj expressions, so every output is the same bits -- which is what lets the
    streaming session reproduce the offline codes exactly (test_streaming_matches_offline)."""
    from facodec_amd.quantize import VectorQuantize
    q = VectorQuantize(D, 1024, 8).eval()
    synth.load_synthetic(q, seed=5)
    q = q.to(cuda)
    z = torch.randn(B, D, T, generator=_g(B + D + T)).to(cuda)
    acc0 = torch.randn(B, D, T, generator=_g(7)).to(cuda)
    w_in, w_out, sc = q._weights()
    outs = []
    for with_loss in (True, False):         # loss partials requested -> the tile kernel; not requested and T <= 8 -> per-frame kernel
        codes = torch.empty(B, T, device=cuda, dtype=torch.int64)
        z_e = torch.empty(B, 8, T, device=cuda)
        res, acc, zq = torch.empty_like(z), acc0.clone(), torch.empty_like(z)
        lp = torch.empty(B, ops.vq_loss_tiles(T), device=cuda) if with_loss else None
        ops.vq_step(z, w_in, q.in_proj.bias.detach(), q.codebook.weight.detach(), w_out, sc, q.out_proj.bias.detach(), codes,
                    residual=res, zq_acc=acc, zq_out=zq, z_e=z_e, loss_part=lp)
        outs.append((codes, z_e, res, acc, zq))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_logmel_frontend_against_oracle(O, cuda):
    """Parity-unpinned row (torchaudio semantics restated on both sides)."""
    from facodec_amd.quantize import LogMelFrontend
    w = synth.synth_clips(2, 48000, seed=0)
    ref = O.logmel_frontend(w, 80)
    with torch.no_grad():
        out = LogMelFrontend().to(cuda)(w.to(cuda))
    assert out.shape == ref.shape == (2, 80, 160)
    assert rel(out, ref) < E2E_TOL


def test_style_encoder_and_wavenet_against_oracle(O, cuda):
    from facodec_amd.quantize import StyleEncoder, WN
    se = StyleEncoder(80, 512, 1024)
    sd = synth.load_synthetic(se, seed=7)
    mel = torch.randn(3, 80, 50, generator=_g(1))
    mask = torch.ones(3, 50)
    mask[1, 30:] = 0
    mask[2, 10:] = 0
    ref = O.style_encoder_forward(mel, sd, "", mask.unsqueeze(1))
    with torch.no_grad():
        out = se.to(cuda)(mel.to(cuda), mask.to(cuda))
        out_nomask = se(mel.to(cuda), None)
    assert rel(out, ref) < OP_TOL
    assert rel(out_nomask, O.style_encoder_forward(mel, sd, "")) < OP_TOL
    wn = WN(256, 5, 1, 8, causal=True)
    sdw = synth.load_synthetic(wn, seed=8)
    x = torch.randn(2, 256, 160, generator=_g(2))
    refw = O.wavenet_forward(x, sdw, "", 256, 8)
    with torch.no_grad():
        outw = wn.to(cuda)(x.to(cuda))
    assert rel(outw, refw) < OP_TOL


@pytest.mark.parametrize("B,H,dk,T", [(4, 2, 256, 188), (2, 2, 256, 1300), (3, 2, 128, 70)])
def test_attention_kernels_against_torch(B, H, dk, T, cuda):
    """The StyleEncoder's 2-head self-attention (modules/attentions.py:168-199) at the benchmark's frame count (188 per 2 s clip),
    at a length whose V tile no longer fits the LDS next to the scores (rows read in place) and at a ragged one: the inference
    kernel (V rows staged through LDS, round 6) and the training Function (probabilities materialised; o = P v, dv, dP, dq, dk on
    the tiled attn_gemm_kernel) against torch's softmax attention and its autograd, fp64."""
    from facodec_amd import ops
    from facodec_amd.autograd_quant import _Attention
    g = _g(B + T)
    q, k, v = (torch.randn(B, H * dk, T, generator=g) for _ in range(3))
    mask = torch.ones(B, T)
    mask[0, T - 17:] = 0

    def ref(q, k, v):
        qh, kh, vh = (t.double().view(B, H, dk, T).transpose(2, 3) for t in (q, k, v))          # (B, H, T, dk)
        sc = qh @ kh.transpose(2, 3) / dk ** 0.5
        m2 = (mask.unsqueeze(1) * mask.unsqueeze(2)).unsqueeze(1)
        sc = sc.masked_fill(m2 == 0, -1e4)
        return (torch.softmax(sc, -1) @ vh).transpose(2, 3).reshape(B, H * dk, T)

    qd, kd, vd = (t.clone().requires_grad_(True) for t in (q, k, v))
    o_ref = ref(qd, kd, vd)
    w = torch.randn(B, H * dk, T, generator=g)
    o_ref.backward(w.double())
    out = ops.attention(q.to(cuda), k.to(cuda), v.to(cuda), mask.to(cuda), H)
    assert rel(out, o_ref) < OP_TOL
    if T > 1000:
        return
    qc, kc, vc = (t.to(cuda).requires_grad_(True) for t in (q, k, v))
    o = _Attention.apply(qc, kc, vc, mask.to(cuda), H, None, 1.0)
    assert rel(o, o_ref) < OP_TOL
    o.backward(w.to(cuda))
    for a, b in ((qc, qd), (kc, kd), (vc, vd)):
        assert rel(a.grad, b.grad) < 2e-5


def test_small_encoder_decoder_vs_reference_golden(cuda, golden_dir):
    from facodec_amd.dac_model import Decoder, Encoder
    d = np.load(os.path.join(golden_dir, "small_layers.npz"))
    enc = Encoder(d_model=8, strides=[2, 5, 5, 6], d_latent=64, causal=True, lstm=2)
    dec = Decoder(input_channel=64, channels=128, rates=[6, 5, 5, 2], causal=True, lstm=2)
    synth.load_synthetic(enc, seed=1, prefix="encoder.")
    synth.load_synthetic(dec, seed=1, prefix="decoder.")
    with torch.no_grad():
        z = enc.to(cuda)(torch.from_numpy(d["x"]).to(cuda))
        y = dec.to(cuda)(torch.from_numpy(d["z"]).to(cuda))
    assert rel(z, d["z"]) < E2E_TOL and rel(y, d["y"]) < E2E_TOL


@pytest.fixture(scope="module")
def full_model(cuda):
    from facodec_amd.commons import build_model, default_model_params
    model = build_model(default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(cuda)
    return model


def test_end_to_end_vs_reference_golden(full_model, cuda, golden_dir):
    """configs[0]/[1] shape: 2 s clips through encoder -> FA-quantizer -> decoder with the
    reconstruct.py call sequence (:56-61).  Codes bit-exact, everything else within 1e-4."""
    d = np.load(os.path.join(golden_dir, "codec_e2e.npz"))
    wave = synth.synth_clips(2, 48000, seed=0).to(cuda)
    m = full_model
    with torch.no_grad():
        z = m.encoder(wave)
        outs, quantized, commit, cbl, timbre, codes = m.quantizer(z, wave, n_c=2, return_codes=True)
        y = m.decoder(outs)
    assert z.shape == (2, 1024, 160) and y.shape == (2, 1, 48000)
    for nm, c in zip(("codes_p", "codes_c", "codes_r"), codes):
        assert c.dtype == torch.int64
        assert torch.equal(c.cpu(), torch.from_numpy(d[nm].astype(np.int64))), nm
    assert rel(z[:, ::8], d["z_probe"]) < E2E_TOL
    assert rel(timbre, d["timbre"]) < E2E_TOL
    assert rel(outs[:, ::8], d["outs_probe"]) < E2E_TOL
    for nm, q in zip(("zq_p_probe", "zq_c_probe", "zq_r_probe"), quantized):
        assert rel(q[:, ::16], d[nm]) < E2E_TOL
    assert rel(y[:, 0, torch.from_numpy(d["probe_t"])], d["wave_probe"]) < E2E_TOL
    assert abs(float(commit) - float(d["commitment"])) / float(d["commitment"]) < E2E_TOL
    assert abs(float(cbl) - float(d["codebook"])) / float(d["codebook"]) < E2E_TOL


def test_five_tuple_return_and_batch_independence(full_model, cuda):
    """reconstruct.py:57-59 unpacks 5 values; clips are independent units: running a clip
    alone or inside a batch gives the same codes and (to fp32 noise) the same waveform."""
    m = full_model
    wave = synth.synth_clips(3, 48000, seed=5).to(cuda)
    with torch.no_grad():
        z = m.encoder(wave)
        out5 = m.quantizer(z, wave, n_c=2)
        assert len(out5) == 5
        outs, _, _, _, _, codes = m.quantizer(z, wave, n_c=2, return_codes=True)
        y = m.decoder(outs)
        z1 = m.encoder(wave[1:2])
        o1, _, _, _, _, c1 = m.quantizer(z1, wave[1:2], n_c=2, return_codes=True)
        y1 = m.decoder(o1)
    for a, b in zip(codes, c1):
        assert torch.equal(a[1:2], b)
    assert rel(y[1:2], y1) < 1e-5


def test_causality_of_encoder_and_decoder(full_model, cuda):
    """perturbing samples >= 24000 changes encoder frames >= 80 only."""
    m = full_model
    wave = synth.synth_clips(1, 48000, seed=6).to(cuda)
    w2 = wave.clone()
    w2[..., 24000:] += 0.1 * torch.randn(1, 1, 24000, device=cuda)
    with torch.no_grad():
        za, zb = m.encoder(wave), m.encoder(w2)
        assert float((za[..., :80] - zb[..., :80]).abs().max()) == 0.0
        assert float((za[..., 80:] - zb[..., 80:]).abs().max()) > 0.0
        lat = torch.randn(1, 1024, 160, device=cuda)
        l2 = lat.clone()
        l2[..., 80:] += 0.1
        ya, yb = m.decoder(lat), m.decoder(l2)
        assert float((ya[..., :24000] - yb[..., :24000]).abs().max()) == 0.0


def test_full_waves_timbre_path(full_model, O, cuda):
    """train.py:266-269 calls the quantizer with full_waves / wave_lens (masked timbre)."""
    m = full_model
    wave = synth.synth_clips(2, 24000, seed=8).to(cuda)
    full = synth.synth_clips(2, 36000, seed=9)[:, 0].to(cuda)
    lens = torch.tensor([36000, 21000], device=cuda)
    sd = {k: v.detach().cpu() for k, v in m.quantizer.state_dict().items()}
    with torch.no_grad():
        z = m.encoder(wave)
        outs, _, _, _, timbre, codes = m.quantizer(z, wave, n_c=2, full_waves=full, wave_lens=lens, return_codes=True)
        ref = O.quantizer_forward(sd, z.cpu(), wave.cpu(), n_c=2, full_waves=full.cpu(), wave_lens=lens.cpu())
    assert rel(timbre, ref[4]) < E2E_TOL and rel(outs, ref[0]) < E2E_TOL
    for a, b in zip(codes, ref[5]):
        assert torch.equal(a.cpu(), b)


def test_missing_extension_fails_loudly(monkeypatch):
    from facodec_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libfacodec_hip.so")
    with pytest.raises(_lib.FacodecHipError):
        _lib.load()


# ------------------------------------------------------------------------- SURVEY 8 rows a11, a15-a17
def test_named_fvq_variant_against_oracle(O, cuda):
    """quantize/fvq.py FactorizedVectorQuantize + quantize/rvq.py ResidualVQ (the variant the north star
    names): same search kernel, Linear-style parameters; indices bit-exact vs the oracle."""
    from facodec_amd.fvq import FactorizedVectorQuantize, ResidualVQ
    m = FactorizedVectorQuantize(dim=256, codebook_size=1024, codebook_dim=8, commitment=0.15).eval()
    sd = synth.load_synthetic(m, seed=4)
    z = torch.randn(2, 256, 130, generator=_g(8))
    out, idx, loss = O.fvq_forward(z, sd, "")
    with torch.no_grad():
        out_g, idx_g, loss_g = m.to(cuda)(z.to(cuda))
    assert torch.equal(idx_g.cpu(), idx) and rel(out_g, out) < OP_TOL and float(loss_g.abs().max()) == 0.0
    r = ResidualVQ(num_quantizers=2, codebook_size=10, dim=256, codebook_dim=8, commitment=0.15).eval()
    sdr = synth.load_synthetic(r, seed=6)
    res, acc, idxs = z, 0, []
    for i in range(2):
        q, ii, _ = O.fvq_forward(res, sdr, f"layers.{i}.")
        res, acc = res - q, acc + q
        idxs.append(ii)
    with torch.no_grad():
        qo, ai, al, aq = r.to(cuda)(z.to(cuda))
    assert torch.equal(ai.cpu(), torch.stack(idxs)) and rel(qo, acc) < OP_TOL and aq.shape == (2, 2, 256, 130)


def _fvq_upstream(shape, seed):
    """The fixed upstream-gradient weights of tests/golden/make_golden_fvq_train.py."""
    n = int(np.prod(shape))
    k = torch.arange(n, dtype=torch.float64)
    return torch.sin(0.37 * k + seed).reshape(tuple(shape)).float() / float(np.sqrt(n))


def test_fvq_train_mode_against_reference_golden(cuda, golden_dir):
    """Row a11 in TRAIN mode on the HIP path against the REAL reference's forward values AND autograd gradients
    (tests/golden/fvq_train.npz, made by make_golden_fvq_train.py from quantize/fvq.py + quantize/rvq.py): one
    FactorizedVectorQuantize (commitment + codebook loss with the reference's detach placements, straight-through estimator),
    then ResidualVQ with 'linear' and 'exp' quantizer dropout (the reference's recorded torch.randint draw handed in).
    Indices bit-exact; values and every parameter / input gradient at 1e-4 (measured ~1e-6)."""
    from facodec_amd.fvq import FactorizedVectorQuantize, ResidualVQ
    d = np.load(os.path.join(golden_dir, "fvq_train.npz"))
    vq = FactorizedVectorQuantize(dim=64, codebook_size=1024, codebook_dim=8, commitment=0.15)
    synth.load_synthetic(vq, seed=4, prefix="fvq.")
    vq.to(cuda).train()
    z = torch.from_numpy(d["fvq_z"]).to(cuda).requires_grad_()
    zq, idx, loss = vq(z)
    assert torch.equal(idx.cpu(), torch.from_numpy(d["fvq_idx"].astype(np.int64)))
    assert rel(zq, d["fvq_zq"]) < OP_TOL and float((loss.detach().cpu() - torch.from_numpy(d["fvq_loss"])).abs().max()) < 1e-6
    ((zq * _fvq_upstream(zq.shape, 1).to(cuda)).sum() + (loss * _fvq_upstream(loss.shape, 2).to(cuda)).sum()).backward()
    worst = {"dz": rel(z.grad, d["fvq_dz"])}
    for n, p in vq.named_parameters():
        worst[n] = rel(p.grad, d["fvq_grad." + n])
    assert max(worst.values()) < E2E_TOL, worst
    # eval mode of the same module object still returns the zero loss (fvq.py:73-74), no autograd node
    with torch.no_grad():
        assert float(vq.eval()(z.detach())[2].abs().max()) == 0.0
    for kind, nq in (("linear", 3), ("exp", 4)):
        rv = ResidualVQ(num_quantizers=nq, codebook_size=10, dim=64, codebook_dim=8, commitment=0.15, quantizer_dropout=0.75, dropout_type=kind)
        synth.load_synthetic(rv, seed=6, prefix="rvq.")
        rv.to(cuda).train()
        pre = f"rvq_{kind}_"
        x = torch.from_numpy(d[pre + "x"]).to(cuda).requires_grad_()
        draw = torch.from_numpy(d[pre + "draw"])
        draw = torch.pow(2, draw) if kind == "exp" else draw                # rvq.py:44
        q_out, all_idx, all_loss, all_q = rv(x, dropout=draw)
        assert torch.equal(all_idx.cpu(), torch.from_numpy(d[pre + "idx"].astype(np.int64))), kind
        assert rel(q_out, d[pre + "out"]) < OP_TOL and rel(all_q[:, :, ::4, ::5], d[pre + "quantized_probe"]) < OP_TOL
        assert float((all_loss.detach().cpu() - torch.from_numpy(d[pre + "losses"])).abs().max()) < 1e-6
        ((q_out * _fvq_upstream(q_out.shape, 3).to(cuda)).sum() + (all_loss * _fvq_upstream(all_loss.shape, 4).to(cuda)).sum()
         + (all_q * _fvq_upstream(all_q.shape, 5).to(cuda)).sum()).backward()
        worst = {"dx": rel(x.grad, d[pre + "dx"])}
        for n, p in rv.named_parameters():
            worst[n] = rel(p.grad, d[pre + "grad." + n])
        assert max(worst.values()) < E2E_TOL, (kind, worst)
    # the reference's own draw: same torch.randint call on the CPU generator -> same n_quantizers for the same seed
    rv3 = ResidualVQ(num_quantizers=3, codebook_size=10, dim=64, codebook_dim=8, commitment=0.15, quantizer_dropout=0.75, dropout_type="linear")
    torch.manual_seed(123)
    want = torch.randint(1, 3 + 1, (4,))
    torch.manual_seed(123)
    assert torch.equal(rv3._draw_n_quantizers(4, None), torch.tensor([float(want[0]), float(want[1]), float(want[2]), 4.0]))
    with pytest.raises(UnboundLocalError):            # rvq.py:45 with dropout_type=None
        ResidualVQ(num_quantizers=2, codebook_size=10, dim=64, codebook_dim=8, commitment=0.15).train()._draw_n_quantizers(4, None)


def test_standalone_rvq_train_mode_against_oracle(O, cuda):
    """dac/nn/quantize.py:127-198 called directly in .train() (what `model.quantizer.content_quantizer(z)` does for a caller with the
    reference's habits): masks drawn like :163-168 or handed in; z_q / codes / latents / both losses and the gradients of the input
    and of every parameter against torch autograd through the oracle."""
    from facodec_amd.quantize import ResidualVectorQuantize
    m = ResidualVectorQuantize(256, 3, 1024, 8, quantizer_dropout=0.5)
    sd = synth.load_synthetic(m, seed=9)
    m.to(cuda).train()
    B, T = 4, 90
    z = torch.randn(B, 256, T, generator=_g(21))
    masks = torch.tensor([[1, 1, 1, 1], [0, 1, 1, 1], [0, 0, 1, 1]], dtype=torch.float32)     # draws (1, 2) for the first two samples
    leaves = {k: v.clone().requires_grad_() for k, v in sd.items()}
    zc = z.clone().requires_grad_()
    zq_o, codes_o, lat_o, cm_o, cb_o = O.rvq_forward_train(zc, leaves, "", 3, masks, return_latents=True)
    up = _fvq_upstream(zq_o.shape, 7)
    ((zq_o * up).sum() + 0.25 * cm_o + cb_o).backward()
    zg = z.to(cuda).requires_grad_()
    zq, codes, lat, cm, cb = m(zg, masks=masks)
    assert torch.equal(codes.cpu(), codes_o) and rel(zq, zq_o) < OP_TOL and rel(lat, lat_o) < OP_TOL
    assert abs(float(cm) - float(cm_o)) / float(cm_o) < OP_TOL and abs(float(cb) - float(cb_o)) / float(cb_o) < OP_TOL
    ((zq * up.to(cuda)).sum() + 0.25 * cm + cb).backward()
    worst = {"dz": rel(zg.grad, zc.grad)}
    for n, p in m.named_parameters():
        worst[n] = rel(p.grad, leaves[n].grad)
    assert max(worst.values()) < E2E_TOL, worst
    torch.manual_seed(5)                      # default path: the module draws its own masks, shapes as the reference returns them
    out = m(z.to(cuda))
    assert out[0].shape == (B, 256, T) and out[1].shape == (B, 3, T) and out[2].shape == (B, 24, T) and out[3].dim() == 0


@pytest.mark.parametrize("B,C,T,k,d,pad", [(2, 64, 1000, 7, 1, "reflect"), (1, 192, 777, 7, 9, "reflect"), (2, 128, 400, 5, 1, "zero"),
                                            (1, 768, 700, 7, 3, "reflect"), (40, 64, 20, 7, 9, "reflect"), (1, 1024, 700, 3, 1, "reflect")])
def test_split_conv_takes_p8_input_bit_identically(ops, cuda, B, C, T, k, d, pad):
    """fac_conv_desc.x_p8: the split k = 3 / 5 / 7 kernel fed with the pre-split planes (fac_to_p8: exact round-to-nearest
    three-way bf16 split, [b][c/8][t][8]) multiplies the same bf16 operands in the same order as when it splits the fp32 tensor
    itself, so the outputs must be IDENTICAL -- interior tiles, reflect / zero edges, an input shorter than the pad; and the planes
    must add back up to the fp32 tensor exactly (with and without the Snake prologue of the producer)."""
    g = _g(90 + C)
    x = torch.randn(B, C, T, generator=g).to(cuda)
    w = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(cuda)
    bias = torch.randn(C, generator=g).to(cuda)
    al = (1 + 0.3 * torch.rand(C, generator=g)).to(cuda)
    ws = ops.pack_conv_weight_split(w)
    pm = ops.PAD_REFLECT if pad == "reflect" else ops.PAD_ZERO
    p8 = ops.to_p8(x)
    assert torch.equal(p8.to_float(), x)
    y_ref = ops.conv1d(x, None, C, k, bias=bias, dilation=d, alpha_out=al, pad_mode=pm, w_split=ws)
    y_p8 = ops.conv1d(p8, None, C, k, bias=bias, dilation=d, alpha_out=al, pad_mode=pm, w_split=ws)
    assert torch.equal(y_p8, y_ref)
    xs = ops.snake(x, al)
    assert torch.equal(ops.to_p8(x, al).to_float(), xs)


@pytest.mark.parametrize("kind,B,ci,co,T,k,s", [("flat", 4, 512, 512, 960, 1, 1), ("flat", 32, 1024, 4096, 160, 1, 1), ("flat", 3, 328, 200, 1001, 1, 1),
                                                ("strided", 3, 128, 256, 2400, 10, 5), ("strided", 2, 64, 128, 1203, 4, 2),
                                                ("strided_zero", 2, 128, 512, 2672, 5, 3)])
def test_split_gemm_takes_p8_input_bit_identically(ops, cuda, kind, B, ci, co, T, k, s):
    """conv1d_gemm_split.hip with fac_conv_desc.x_p8: flattened-column 1x1 GEMMs (tiles that span two clips, ragged channel and row
    counts), strided convs over the phase sub-signals (reflect and zero padding, ragged last frame): both operands by LDS-DMA,
    same bf16 operands as the in-kernel split -> identical outputs."""
    g = _g(200 + ci + k)
    x = torch.randn(B, ci, T, generator=g).to(cuda)
    w = (torch.randn(co, ci, k, generator=g) / (ci * k) ** 0.5).to(cuda)
    bias = torch.randn(co, generator=g).to(cuda)
    if kind == "flat":
        ws = ops.pack_gemm_weight_split(w)
        kw = dict(bias=bias, pad_left=0, pad_mode=ops.PAD_ZERO, t_out=T)
    elif kind == "strided":
        ws = ops.pack_gemm_weight_split(w, in_stride=s)
        kw = dict(bias=bias, stride=s)
    else:
        ws = ops.pack_gemm_weight_split(w, in_stride=s)
        kw = dict(bias=bias, stride=s, pad_left=2, pad_mode=ops.PAD_ZERO, t_out=(T + 4 - k) // s + 1)
    prof = ops.ConvLaunchProfile()
    ops.set_conv_profile(prof)
    try:
        y_ref = ops.conv1d(x, None, co, k, w_split=ws, **kw)
        y_p8 = ops.conv1d(ops.to_p8(x), None, co, k, w_split=ws, **kw)
        torch.cuda.synchronize()
    finally:
        ops.set_conv_profile(None)
    assert all("gemm_split" in n for n in prof.summary()), prof.summary().keys()
    assert torch.equal(y_p8, y_ref)


def test_short_clips_run_flattened_on_the_split_gemm(O, cuda, monkeypatch):
    """The 160-frame layers (encoder's last downsampling conv 512 -> 1024 k 12 s 6, decoder's first ConvTranspose1d 1536 -> 768 s 6)
    at B = 32: too short for per-clip column tiles, so they run as ONE flattened signal on the split GEMM kernel
    (ops.conv1d_flat / ops.conv_transpose1d_flat).  Same results as the oracle and as the per-clip launch (FAC_FLAT_SHORT=0 path)."""
    from facodec_amd import layers, ops
    B, T = 32, 960
    conv = layers.SConv1d(64, 128, 12, stride=6, causal=True, norm="weight_norm")
    tr = layers.SConvTranspose1d(128, 64, 12, stride=6, causal=True, norm="weight_norm")
    sd_c, sd_t = synth.load_synthetic(conv, seed=31), synth.load_synthetic(tr, seed=32)
    conv.to(cuda)
    tr.to(cuda)
    x = torch.randn(B, 64, T, generator=_g(33))
    z = torch.randn(B, 128, T // 6, generator=_g(34))
    a2 = 1 + 0.2 * torch.rand(128, generator=_g(35))
    prof = ops.ConvLaunchProfile()
    ops.set_conv_profile(prof)
    try:
        with torch.no_grad():
            y, y2 = conv.run(x.to(cuda), alpha_y2=a2.to(cuda))
            u = tr.run(z.to(cuda))
            torch.cuda.synchronize()
    finally:
        ops.set_conv_profile(None)
    assert all("gemm_split" in n for n in prof.summary()), prof.summary().keys()
    y_ref = O.sconv1d(x, O.conv_weight(sd_c, "conv.conv."), sd_c["conv.conv.bias"], stride=6, causal=True)
    al = a2.view(1, -1, 1)
    assert y.shape == y_ref.shape and rel(y, y_ref) < OP_TOL and rel(y2, y_ref + torch.sin(al * y_ref) ** 2 / (al + 1e-9)) < OP_TOL
    u_ref = O.sconvtr1d(z, O.weight_norm_weight(sd_t["convtr.convtr.weight_v"], sd_t["convtr.convtr.weight_g"]), sd_t["convtr.convtr.bias"], 6)
    assert u.shape == u_ref.shape and rel(u, u_ref) < OP_TOL
    monkeypatch.setattr(layers, "FLAT_SHORT_CLIPS", False)
    with torch.no_grad():
        y0 = conv.run(x.to(cuda))
        u0 = tr.run(z.to(cuda))
    assert rel(y, y0) < OP_TOL and rel(u, u0) < OP_TOL


@pytest.mark.parametrize("c_in,c_out,d,T,a2", [(1024, 1536, 1, 160, False), (1024, 1024, 3, 100, True)])
def test_short_clips_run_flattened_stride1_bit_identically(c_in, c_out, d, T, a2, O, cuda, monkeypatch):
    """The decoder's input conv (1024 -> 1536, k = 7) at the latent rate -- 160 frames fill 160 of the split kernel's 256 tile columns --
    runs as ONE flattened signal of reflect-padded clips (ops.conv1d_flat): the same products in the same order as the
    per-clip launch, so the outputs are the same bits; both within the op tolerance of the oracle."""
    from facodec_amd import layers, ops
    B = 8
    conv = layers.SConv1d(c_in, c_out, 7, dilation=d, causal=True, norm="weight_norm")
    sd = synth.load_synthetic(conv, seed=41)
    conv.to(cuda)
    x = torch.randn(B, c_in, T, generator=_g(42)).to(cuda)
    alpha2 = (1 + 0.2 * torch.rand(c_out, generator=_g(43))).to(cuda) if a2 else None
    calls = []
    orig = ops.conv1d_flat
    monkeypatch.setattr(ops, "conv1d_flat", lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1])
    with torch.no_grad():
        got = conv.run(x, alpha_y2=alpha2)
    assert len(calls) == 1
    monkeypatch.setattr(layers, "FLAT_STRIDE1", False)
    with torch.no_grad():
        ref = conv.run(x, alpha_y2=alpha2)
    assert len(calls) == 1
    if a2:
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
        y = got[0]
    else:
        assert torch.equal(got, ref)
        y = got
    assert y.shape == (B, c_out, T)
    y_ref = O.sconv1d(x.cpu(), O.conv_weight(sd, "conv.conv."), sd["conv.conv.bias"], dilation=d, causal=True)
    assert rel(y, y_ref) < OP_TOL


def test_quantizer_chains_on_side_streams_are_bit_identical(cuda, monkeypatch):
    """FAquantizer's eval forward runs its three independent chains -- timbre encoder, prosody branch + prosody RVQ, content RVQ
    (modules/quantize.py:378-405) -- side by side on side streams (ops.run_chains): same kernels on other streams, so every
    output and every code equals the serial order's, with and without the full-utterance timbre input, three trials each."""
    from facodec_amd import quantize as Q
    from facodec_amd.commons import build_model, default_model_params
    model = build_model(default_model_params())
    for k in ("encoder", "quantizer"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].to(cuda).eval()
    wave = synth.synth_clips(4, 48000, seed=11).to(cuda)
    full = synth.synth_clips(4, 60000, seed=12).squeeze(1).to(cuda)
    lens = torch.tensor([60000, 45000, 51000, 30000], dtype=torch.int64, device=cuda)
    assert Q.QUANT_STREAMS > 1
    with torch.no_grad():
        z = model.encoder(wave)
        monkeypatch.setattr(Q, "QUANT_STREAMS", 1)
        ref = [model.quantizer(z, wave, n_c=2, return_codes=True), model.quantizer(z, wave, n_c=2, full_waves=full, wave_lens=lens, return_codes=True)]
        monkeypatch.setattr(Q, "QUANT_STREAMS", 3)
        for _ in range(3):
            got = [model.quantizer(z, wave, n_c=2, return_codes=True), model.quantizer(z, wave, n_c=2, full_waves=full, wave_lens=lens, return_codes=True)]
            for g, r in zip(got, ref):
                assert torch.equal(g[0], r[0]) and torch.equal(g[4], r[4]) and torch.equal(g[2], r[2]) and torch.equal(g[3], r[3])
                assert all(torch.equal(a, b) for a, b in zip(g[1], r[1])) and all(torch.equal(a, b) for a, b in zip(g[5], r[5]))


def test_p8_prepass_policy_is_bit_identical(cuda, monkeypatch):
    """Inference launches of the split GEMM kernel with a small input next to the GEMM (LSTM input projections, transposed convs,
    the flattened last strided conv) take their input through ONE fac_to_p8 pass (ops.p8_prepass): same bf16 operands in the same
    order as the in-kernel split, so the outputs are the same bits with the policy on and off -- and the policy must actually fire."""
    from facodec_amd import layers, ops
    calls = []
    real = ops.to_p8

    def counting(x, alpha=None):
        calls.append(tuple(x.shape))
        return real(x, alpha)

    monkeypatch.setattr(ops, "to_p8", counting)
    tr = layers.SConvTranspose1d(384, 192, 10, stride=5, causal=True, norm="weight_norm")          # 960 FLOP per input byte
    tr_flat = layers.SConvTranspose1d(512, 256, 12, stride=6, causal=True, norm="weight_norm")     # short clips: flattened launch
    conv_flat = layers.SConv1d(256, 256, 12, stride=6, causal=True, norm="weight_norm")           # 256 FLOP / byte: below the bar
    conv_flat2 = layers.SConv1d(512, 1024, 12, stride=6, causal=True, norm="weight_norm")         # 1024: above
    lstm = layers.SLSTM(1024, 2)
    mods = (tr, tr_flat, conv_flat, conv_flat2, lstm)
    for i, m in enumerate(mods):
        synth.load_synthetic(m, seed=70 + i)
        m.to(cuda)
    ins = (torch.randn(4, 384, 700, generator=_g(81)), torch.randn(32, 512, 160, generator=_g(82)), torch.randn(32, 256, 960, generator=_g(83)),
           torch.randn(32, 512, 960, generator=_g(84)), torch.randn(20, 1024, 40, generator=_g(85)))

    def run_all():
        with torch.no_grad():
            return [(m.run if hasattr(m, "run") else m)(x.to(cuda)) for m, x in zip(mods, ins)]

    on = run_all()
    fired = list(calls)
    monkeypatch.setattr(ops, "P8_PREPASS_MIN_FLOP_PER_BYTE", 0.0)
    off = run_all()
    assert len(calls) == len(fired), "the pass must not run with the policy off"
    assert [c[1] for c in fired] == [384, 512, 512, 1024, 1024], fired      # tr, tr_flat, conv_flat2, two LSTM layers; not conv_flat
    for a, b in zip(on, off):
        assert torch.equal(a, b)


def test_spectral_losses_against_oracle(O, cuda):
    """MelSpectrogramLoss (train.py:155-163 arguments), MultiScaleSTFTLoss, L1Loss, reconstruction_loss on
    2 s clips; bar 1e-4 relative.  Third-party STFT/mel semantics restated on both sides: parity unpinned."""
    from facodec_amd import losses
    y = synth.synth_clips(3, 48000, seed=11)
    x = (0.6 * y + 0.1 * synth.synth_clips(3, 48000, seed=12)).contiguous()
    mel = losses.MelSpectrogramLoss(n_mels=[5, 10, 20, 40, 80, 160, 320], window_lengths=[32, 64, 128, 256, 512, 1024, 2048],
                                    mel_fmin=[0] * 7, mel_fmax=[None] * 7, pow=1.0, mag_weight=0.0, clamp_eps=1e-5)
    xs, ys = x.to(cuda), y.to(cuda)
    got = float(mel(xs, ys))
    ref = float(O.mel_spectrogram_loss(x, y))
    assert abs(got - ref) / ref < E2E_TOL, (got, ref)
    got = float(losses.MultiScaleSTFTLoss()(xs, ys))
    ref = float(O.multiscale_stft_loss(x, y))
    assert abs(got - ref) / ref < E2E_TOL, (got, ref)
    got = float(losses.L1Loss()(xs, ys))
    ref = float(O.waveform_l1_loss(x, y))
    assert abs(got - ref) / ref < 1e-5
    got = float(losses.reconstruction_loss(xs[:, 0], ys[:, 0]))
    ref = float(O.reconstruction_loss(x[:, 0], y[:, 0]))
    assert abs(got - ref) / ref < E2E_TOL, (got, ref)


def test_losses_on_golden_pair(full_model, cuda, golden_dir):
    """Loss values on the (reference input, decoded output) pair recorded by the golden generator through
    the reference's own dac/nn/loss.py (over the audiotools shim)."""
    from facodec_amd import losses
    d = np.load(os.path.join(golden_dir, "codec_e2e.npz"))
    wave = synth.synth_clips(2, 48000, seed=0).to(cuda)
    m = full_model
    with torch.no_grad():
        z = m.encoder(wave)
        outs = m.quantizer(z, wave, n_c=2)[0]
        y = m.decoder(outs)
    mel = losses.MelSpectrogramLoss(n_mels=[5, 10, 20, 40, 80, 160, 320], window_lengths=[32, 64, 128, 256, 512, 1024, 2048],
                                    mel_fmin=[0] * 7, mel_fmax=[None] * 7, pow=1.0, mag_weight=0.0, clamp_eps=1e-5)
    assert abs(float(mel(y, wave)) - float(d["loss_mel"])) / float(d["loss_mel"]) < E2E_TOL
    assert abs(float(losses.MultiScaleSTFTLoss()(y, wave)) - float(d["loss_stft"])) / float(d["loss_stft"]) < E2E_TOL
    assert abs(float(losses.L1Loss()(y, wave)) - float(d["loss_l1"])) / float(d["loss_l1"]) < E2E_TOL


def test_meldataset_preprocess_against_oracle(O, cuda):
    """meldataset.py:42-47 (sr-16000 filterbank quirk, all centred frames)."""
    from facodec_amd.meldataset import preprocess
    w = synth.synth_clips(1, 30000, seed=2)[0, 0]
    spec = O.stft_complex(w.unsqueeze(0), 2048, 300, 1200).abs().pow(2)
    fb = O.mel_filterbank_htk(1025, 80, 16000)
    ref = (torch.log(1e-5 + torch.matmul(spec.transpose(-1, -2), fb).transpose(-1, -2)) + 4) / 4
    got = preprocess(w.to(cuda))
    assert got.shape == ref.shape == (1, 80, 101) and rel(got, ref) < E2E_TOL


@pytest.mark.parametrize("C,T,d", [(64, 700, 1), (96, 1000, 3), (128, 517, 9)])
def test_fused_residual_unit_against_oracle(C, T, d, O, cuda):
    """Single-launch ResidualUnit (k7 -> Snake -> k1 -> +x out of the accumulators) vs the oracle's unit."""
    from facodec_amd.dac_model import ResidualUnit
    ru = ResidualUnit(C, dilation=d, causal=True)
    sd = synth.load_synthetic(ru, seed=C)
    x = torch.randn(2, C, T, generator=_g(C + d))
    ref = O.residual_unit(x, sd, "", d, True)
    a_next = 1 + 0.2 * torch.rand(C, generator=_g(1))
    ru = ru.to(cuda)
    xg = x.to(cuda)
    with torch.no_grad():
        y, y2 = ru.run(xg, ops_snake(xg, ru.alpha_in), alpha_next=a_next.to(cuda))
        y_only = ru(xg)
    assert rel(y, ref) < OP_TOL and rel(y_only, ref) < OP_TOL
    assert rel(y2, O.snake(ref, a_next.view(1, -1, 1))) < OP_TOL


def ops_snake(x, alpha):
    from facodec_amd import ops as _ops
    return _ops.snake(x, alpha)


def test_anti_aliased_snakebeta_against_oracle(O, ops, cuda):
    """K13: Activation1d(SnakeBeta) fused kernel, incl. the replicate-padded edges and a ragged tile."""
    from facodec_amd import dsp
    g = _g(31)
    filt = dsp.kaiser_sinc_filter1d(0.25, 0.3, 12)
    for (B, C, T) in ((2, 7, 160), (1, 3, 5), (1, 2, 777)):
        x = torch.randn(B, C, T, generator=g) * 2
        al = 0.3 * torch.randn(C, generator=g)
        be = 0.3 * torch.randn(C, generator=g)
        ref = O.aa_snakebeta(x, al, be, filt)
        got = ops.aa_snakebeta(x.to(cuda), al.to(cuda), be.to(cuda), filt.reshape(-1).to(cuda))
        assert got.shape == ref.shape and rel(got, ref) < OP_TOL


def test_predictors_vs_reference_golden(full_model, cuda, golden_dir):
    """train.py:270 `model.fa_predictors(quantized, timbre)` on the quantizer's outputs; values recorded
    from the real reference (tests/golden/predictors.npz)."""
    d = np.load(os.path.join(golden_dir, "predictors.npz"))
    from facodec_amd.commons import build_model, default_model_params
    pred = build_model(default_model_params()).fa_predictors
    synth.load_synthetic(pred, seed=0, prefix="fa_predictors.")
    pred.eval().to(cuda)
    m = full_model
    wave = synth.synth_clips(2, 48000, seed=0).to(cuda)
    with torch.no_grad():
        z = m.encoder(wave)
        outs, quantized, _, _, timbre = m.quantizer(z, wave, n_c=2)
        preds, rev = pred(quantized, timbre)
    assert preds["f0"].shape == (2, 160, 1) and preds["content"].shape == (2, 160, 1024) and preds["timbre"].shape == (2, 20000)
    assert rel(preds["f0"], d["f0"]) < E2E_TOL and rel(preds["uv"], d["uv"]) < E2E_TOL
    assert rel(preds["content"][:, ::4, ::16], d["content_probe"]) < E2E_TOL
    assert rel(preds["timbre"][:, ::50], d["timbre_probe"]) < E2E_TOL
    assert rel(rev["rev_f0"], d["rev_f0"]) < E2E_TOL and rel(rev["rev_uv"], d["rev_uv"]) < E2E_TOL
    assert rel(rev["rev_content"][:, ::4, ::16], d["rev_content_probe"]) < E2E_TOL
    assert rel(rev["x_timbre"][:, ::50], d["x_timbre_probe"]) < E2E_TOL


def test_long_clip_single_item_batch(full_model, O, cuda):
    """configs[0]-style call: ONE clip (B = 1), 10 s instead of 2 s -- many time tiles, ragged last tiles,
    T not a multiple of the 300-sample hop (encoder emits ceil(T/300) frames, quantizer crops to floor)."""
    m = full_model
    T = 240000 + 130
    wave = synth.synth_clips(1, T, seed=13).to(cuda)
    sds = {k: {n: v.detach().cpu() for n, v in m[k].state_dict().items()} for k in ("encoder", "quantizer", "decoder")}
    from facodec_amd.diagnostics import LatentCapture, classify_code_mismatches
    with torch.no_grad(), LatentCapture(m.quantizer) as cap:
        z = m.encoder(wave)
        outs, _, _, _, timbre, codes = m.quantizer(z, wave, n_c=2, return_codes=True)
        y = m.decoder(outs)
        r = O.codec_forward(sds, wave.cpu(), n_c=2)
    assert z.shape == r["z"].shape == (1, 1024, 801) and y.shape == r["wave"].shape == (1, 1, 800 * 300)
    # 4 806 arg-max decisions against an independent fp32 evaluation: flips between two codes whose distances differ by
    # <= 1e-5 (and the residual stages they drag along) would be legitimate; anything else is an error.  Today there are none.
    triage = {name: classify_code_mismatches(mod, cap.latents[name], c, e) for (name, mod), c, e in zip(cap.rvqs, codes, r["codes"])}
    assert all(t["genuine"] == 0 for t in triage.values()), triage
    mism = sum(t["mismatches"] for t in triage.values())
    assert mism == 0, f"{mism} near-tie code flips of {sum(c.numel() for c in codes)}: {triage}"
    assert rel(z, r["z"]) < E2E_TOL and rel(y, r["wave"]) < E2E_TOL and rel(timbre, r["timbre"]) < E2E_TOL


# ------------------------------------------------------------------------------ voice-conversion path
@pytest.mark.parametrize("B,ci,co,T,s", [(2, 256, 128, 160, 6), (2, 128, 64, 333, 5), (1, 192, 96, 1000, 2), (1, 24, 12, 7, 5)])
def test_noncausal_conv_transpose_against_oracle(B, ci, co, T, s, O, ops, cuda):
    """SConvTranspose1d with causal=False (dac/nn/layers.py: the k - stride trim is split right = total // 2,
    left = total - right): the phase-shifted polyphase launch."""
    g = _g(s + 40)
    x = torch.randn(B, ci, T, generator=g)
    v = torch.randn(ci, co, 2 * s, generator=g) / (ci * 2) ** 0.5
    gg = torch.rand(ci, 1, 1, generator=g) + 0.5
    b = torch.randn(co, generator=g) * 0.1
    a2 = 1 + 0.2 * torch.rand(co, generator=g)
    y = O.sconvtr1d(x, O.weight_norm_weight(v, gg), b, s, causal=False)
    wp = ops.pack_convtr_weight(v.to(cuda), gg.to(cuda), s)
    yg, yg2 = ops.conv_transpose1d(x.to(cuda), wp, co, s, bias=b.to(cuda), alpha_y2=a2.to(cuda), causal=False)
    assert yg.shape == y.shape and rel(yg, y) < OP_TOL
    assert rel(yg2, O.snake(y, a2.view(1, -1, 1))) < OP_TOL


@pytest.mark.parametrize("C,T,d", [(64, 700, 1), (96, 1000, 9), (192, 400, 3)])
def test_noncausal_residual_unit_against_oracle(C, T, d, O, cuda):
    from facodec_amd.dac_model import ResidualUnit
    ru = ResidualUnit(C, dilation=d, causal=False)
    sd = synth.load_synthetic(ru, seed=31)
    x = torch.randn(2, C, T, generator=_g(C))
    ref = O.residual_unit(x, sd, "", d, causal=False)
    with torch.no_grad():
        out = ru.to(cuda)(x.to(cuda))
    assert rel(out, ref) < OP_TOL


def test_conditioned_noncausal_wavenet_against_oracle(O, cuda):
    from facodec_amd.quantize import WN
    wn = WN(128, 5, 1, 4, gin_channels=96, causal=False)
    sd = synth.load_synthetic(wn, seed=9)
    x = torch.randn(3, 128, 77, generator=_g(3))
    gvec = torch.randn(3, 96, generator=_g(4))
    ref = O.wavenet_forward(x, sd, "", 128, 4, causal=False, g=gvec.unsqueeze(2))
    with torch.no_grad():
        out = wn.to(cuda)(x.to(cuda), None, g=gvec.to(cuda))
    assert rel(out, ref) < OP_TOL


def test_embed_sum_is_exact(ops, cuda):
    g = _g(12)
    tabs = torch.randn(3, 1024, 64, generator=g)
    codes = torch.randint(0, 1024, (2, 3, 50), generator=g)
    ref = sum(torch.nn.functional.embedding(codes[:, i], tabs[i]) for i in range(3)).transpose(1, 2)
    out = ops.embed_sum(codes.to(cuda), tabs.to(cuda))
    assert rel(out, ref) < 1e-6
    out2 = ops.embed_sum(codes.to(cuda), tabs[:2].to(cuda), 1)          # tables applied to rows 1..2
    ref2 = sum(torch.nn.functional.embedding(codes[:, 1 + i], tabs[i]) for i in range(2)).transpose(1, 2)
    assert rel(out2, ref2) < 1e-6


def test_redecoder_vs_reference_golden(full_model, cuda, golden_dir):
    """reconstruct_redecoder.py:95-122: codes of the source clip + timbre of the target -> Redecoder ->
    non-causal decoder.  Golden from the real reference (stage='redecoder', config_redecoder.yml)."""
    from facodec_amd.commons import build_model, default_redecoder_params
    d = np.load(os.path.join(golden_dir, "redecoder.npz"))
    rm = build_model(default_redecoder_params(), stage="redecoder")
    for k in ("encoder", "decoder"):
        synth.load_synthetic(rm[k], seed=0, prefix="redecoder." + k + ".")
        rm[k].eval().to(cuda)
    wave = synth.synth_clips(2, 48000, seed=0).to(cuda)
    m = full_model
    with torch.no_grad():
        z = m.encoder(wave)
        _, _, _, _, timbre, codes = m.quantizer(z, wave, n_c=2, return_codes=True)
        zr = rm.encoder(codes[0], codes[1], timbre.flip(0), use_p_code=False, n_c=1)
        yr = rm.decoder(zr)
    assert zr.shape == (2, 1024, 160) and yr.shape == (2, 1, 48000)
    assert rel(zr[:, ::8], d["z_probe"]) < E2E_TOL
    assert rel(yr[:, 0, torch.from_numpy(d["probe_t"])], d["wave_probe"]) < E2E_TOL
    assert abs(float(yr.abs().max()) - float(d["wave_absmax"])) < 1e-4


# ------------------------------------------------------------------------------ streaming (configs[4])
@pytest.mark.parametrize("use_graphs", [False, True])
def test_streaming_matches_offline(full_model, cuda, use_graphs):
    """480-sample hops with carried state == the offline causal model on the whole signal: codes bit-exact,
    waveform within 1e-4 (the reference has no streaming code, parity target = offline)."""
    from facodec_amd.streaming import HOP, StreamingCodec
    m = full_model
    n_hops = 27
    T = 4800 + n_hops * HOP                                   # 17 760 samples... must be a multiple of 300
    n_hops = 25
    T = 4800 + n_hops * HOP                                   # 16 800 = 56 frames
    wave = synth.synth_clips(2, T, seed=11).to(cuda)
    with torch.no_grad():
        z = m.encoder(wave)
        outs, _, _, _, timbre, codes = m.quantizer(z, wave, n_c=2, return_codes=True)
        y = m.decoder(outs)
        sess = StreamingCodec(m, timbre, n_c=2, use_graphs=use_graphs)
        got_codes, got_wave, frame = [[], [], []], [], 0
        pieces = [sess.prime(wave[:, :, :4800])]
        for h in range(n_hops):
            o = sess.push(wave[:, :, 4800 + h * HOP: 4800 + (h + 1) * HOP])
            pieces.append({k: ([c.clone() for c in v] if isinstance(v, list) else (v.clone() if torch.is_tensor(v) else v))
                           for k, v in o.items()})
        pieces.append(sess.finish())
    for o in pieces:
        if o["codes"] is None:
            continue
        assert o["frame0"] == frame
        frame += o["codes"][0].shape[-1]
        for i in range(3):
            got_codes[i].append(o["codes"][i])
        got_wave.append(o["wave"])
    assert frame == T // 300
    for i in range(3):
        assert torch.equal(torch.cat(got_codes[i], -1), codes[i]), f"codes[{i}]"
    assert rel(torch.cat(got_wave, -1), y) < E2E_TOL


def _run_session(m, wave, timbre, n_hops, use_graphs=True):
    from facodec_amd.streaming import HOP, StreamingCodec
    sess = StreamingCodec(m, timbre, n_c=2, use_graphs=use_graphs)
    outs = [sess.prime(wave[:, :, :4800])]
    for h in range(n_hops):
        o = sess.push(wave[:, :, 4800 + h * HOP: 4800 + (h + 1) * HOP])
        outs.append({k: ([c.clone() for c in v] if isinstance(v, list) else (v.clone() if torch.is_tensor(v) else v)) for k, v in o.items()})
    outs.append(sess.finish())
    return outs


def test_streaming_folded_epilogues_are_bit_identical(full_model, cuda, ops, monkeypatch):
    """Round 6: the hop's elementwise launches folded into its convs' reduction kernels (WaveNet gate and residual / skip adds,
    FAC_ACT_GATE / FAC_ACT_WN_RES_SKIP) and the left-context buffers written by their producers -- every code and every output
    sample equals the hop built from separate launches (FAC_STREAM_FOLD=0), graphs on, over three periods."""
    from facodec_amd.streaming import HOP
    m = full_model
    n_hops = 15
    wave = synth.synth_clips(2, 4800 + n_hops * HOP, seed=12).to(cuda)
    with torch.no_grad():
        timbre = m.quantizer(m.encoder(wave), wave, n_c=2)[4]
        monkeypatch.setattr(ops, "STREAM_FOLD", False)
        ref = _run_session(m, wave, timbre, n_hops)
        monkeypatch.setattr(ops, "STREAM_FOLD", True)
        got = _run_session(m, wave, timbre, n_hops)
    for other in (got,):
        n_frames = 0
        for r, g in zip(ref, other):
            assert r["frame0"] == g["frame0"] and (r["codes"] is None) == (g["codes"] is None)
            if r["codes"] is None:
                continue
            n_frames += r["codes"][0].shape[-1]
            for a, b in zip(r["codes"], g["codes"]):
                assert torch.equal(a, b)
            assert torch.equal(r["wave"], g["wave"])
        assert n_frames == (4800 + n_hops * HOP) // 300


def test_stream_push_kernel(ops, cuda):
    g = _g(3)
    buf = torch.zeros(2, 3, 10 + 7, device=cuda)
    ref = torch.zeros(2, 3, 0)
    n_prev = 0
    for n in (7, 3, 5, 1, 7):
        x = torch.randn(2, 3, n, generator=g)
        ops.stream_push(buf, x.to(cuda), 10, n_prev)
        ref = torch.cat([ref, x], -1)
        tail = ref[:, :, -(10 + n):]
        assert torch.equal(buf[:, :, 10 + n - tail.shape[-1]:10 + n].cpu(), tail)
        n_prev = n


def test_skinny_conv_variant_and_second_output(O, ops, cuda):
    """The few-column launches must actually take the split-reduction kernel, and its epilogue must emit
    the pre-activated copy; also the transposed conv with carried history (streaming)."""
    import ctypes
    from facodec_amd import _lib
    g = _g(77)
    x = torch.randn(1, 384, 40, generator=g)
    w = torch.randn(384, 384, 7, generator=g) / 52.0
    b = torch.randn(384, generator=g) * 0.1
    a2 = 1 + 0.2 * torch.rand(384, generator=g)
    r = torch.randn(1, 384, 34, generator=g)
    y_ref = torch.nn.functional.conv1d(x, w, b) + r
    wp = ops.pack_conv_weight(w.to(cuda))
    prof = ops.ConvLaunchProfile()
    ops.set_conv_profile(prof)
    try:
        y, y2 = ops.conv1d(x.to(cuda), wp, 384, 7, bias=b.to(cuda), pad_left=0, pad_mode=ops.PAD_ZERO, t_out=34,
                           res=r.to(cuda), alpha_y2=a2.to(cuda))
        torch.cuda.synchronize()
    finally:
        ops.set_conv_profile(None)
    assert any("skinny" in k for k in prof.summary()), prof.summary().keys()
    assert rel(y, y_ref) < OP_TOL and rel(y2, O.snake(y_ref, a2.view(1, -1, 1))) < OP_TOL
    # transposed conv, second chunk of a stream == the tail of the whole-signal result
    s = 5
    xx = torch.randn(2, 256, 9, generator=g)
    v = torch.randn(256, 128, 2 * s, generator=g) / 22.0
    gg = torch.rand(256, 1, 1, generator=g) + 0.5
    bb = torch.randn(128, generator=g) * 0.1
    full = O.sconvtr1d(xx, O.weight_norm_weight(v, gg), bb, s, causal=True)
    wpt = ops.pack_convtr_weight(v.to(cuda), gg.to(cuda), s)
    tail = ops.conv_transpose1d(xx[:, :, 5:].to(cuda), wpt, 128, s, bias=bb.to(cuda), has_history=True)
    assert rel(tail, full[:, :, 6 * s:]) < OP_TOL


# ------------------------------------------------------------------------------ fp32-grade bf16 split convs
@pytest.mark.parametrize("B,C,T,d,mode", [(2, 128, 1000, 1, "reflect"), (1, 192, 777, 3, "reflect"), (2, 768, 960, 9, "reflect"),
                                           (1, 96, 2000, 9, "zero"), (3, 256, 300, 1, "reflect")])
def test_split_bf16_conv_matches_fp32_grade(B, C, T, d, mode, O, ops, cuda):
    """conv1d_bsplit.hip: w and x as three exact bf16 terms, six bf16 MFMAs per K step, fp32 accumulation.
    Bar: the SAME tolerance as the fp32-MFMA kernel against the oracle, and an error against an fp64 conv no
    larger than 1.5x the fp32-MFMA kernel's."""
    g = _g(C + d)
    x = torch.randn(B, C, T, generator=g)
    w = torch.randn(C, C, 7, generator=g) / (C * 7) ** 0.5
    gg = torch.rand(C, 1, 1, generator=g) + 0.5
    b = torch.randn(C, generator=g) * 0.1
    ao = 1 + 0.2 * torch.rand(C, generator=g)
    a2 = 1 + 0.2 * torch.rand(C, generator=g)
    r = torch.randn(B, C, T, generator=g)
    wn = O.weight_norm_weight(w, gg)
    y_ref = O.snake(O.sconv1d(x, wn, b, dilation=d, causal=True, pad_mode=mode), ao.view(1, -1, 1)) + r
    pm = ops.PAD_REFLECT if mode == "reflect" else ops.PAD_ZERO
    kw = dict(bias=b.to(cuda), dilation=d, pad_mode=pm, alpha_out=ao.to(cuda), res=r.to(cuda), alpha_y2=a2.to(cuda))
    ws = ops.pack_conv_weight_split(w.to(cuda), gg.to(cuda))
    prof = ops.ConvLaunchProfile()
    ops.set_conv_profile(prof)
    try:
        y, y2 = ops.conv1d(x.to(cuda), None, C, 7, w_split=ws, **kw)
        torch.cuda.synchronize()
    finally:
        ops.set_conv_profile(None)
    assert any("bsplit" in k for k in prof.summary()), prof.summary().keys()
    yf, _ = ops.conv1d(x.to(cuda), ops.pack_conv_weight(w.to(cuda), gg.to(cuda)), C, 7, **kw)
    assert rel(y, y_ref) < OP_TOL and rel(y2, O.snake(y_ref, a2.view(1, -1, 1))) < OP_TOL
    # plain conv against fp64
    y64 = torch.nn.functional.conv1d(torch.nn.functional.pad(x.double(), (6 * d, 0)), wn.double(), b.double(), dilation=d)
    kw0 = dict(bias=b.to(cuda), dilation=d, pad_left=6 * d, pad_mode=ops.PAD_ZERO, t_out=T)
    e_split = rel(ops.conv1d(x.to(cuda), None, C, 7, w_split=ws, **kw0), y64)
    e_fp32 = rel(ops.conv1d(x.to(cuda), ops.pack_conv_weight(w.to(cuda), gg.to(cuda)), C, 7, **kw0), y64)
    assert e_split < 1.5 * e_fp32 + 1e-7, (e_split, e_fp32)
    assert rel(y, yf) < OP_TOL


@pytest.mark.parametrize("B,ci,co,T,act", [(8, 512, 512, 960, "none"), (32, 256, 512, 160, "mish"), (1, 1024, 4096, 2560, "none"),
                                           (4, 320, 200, 333, "none"), (2, 768, 96, 1001, "none"), (2, 1200, 2050, 600, "none")])
def test_gemm_split_1x1_matches_fp32_grade(B, ci, co, T, act, ops, cuda):
    """conv1d_gemm_split.hip, K = 1: many-channel 1x1 convs as a split-bf16 GEMM over the flattened (clip, time) columns --
    bias, activation, residual, second pre-activated output; row counts that do not fill a 128-row tile, T not a multiple of 4
    (sample-wise epilogue), 160-frame clips sharing a column tile.  Bars as for the k = 7 split kernel: the fp32 kernel's
    tolerance, and an fp64 error no larger than 1.5x the fp32-MFMA kernel's."""
    import torch.nn.functional as F
    g = _g(ci + co + T)
    x = torch.randn(B, ci, T, generator=g)
    w = torch.randn(co, ci, 1, generator=g) / ci ** 0.5
    gg = torch.rand(co, 1, 1, generator=g) + 0.5
    b = torch.randn(co, generator=g) * 0.1
    r = torch.randn(B, co, T, generator=g)
    a2 = 1 + 0.2 * torch.rand(co, generator=g)
    wn = w * (gg / w.reshape(co, -1).norm(dim=1).reshape(co, 1, 1))
    y64 = F.conv1d(x.double(), wn.double(), b.double())
    if act == "mish":
        y64 = y64 * torch.tanh(F.softplus(y64))
    y64 = y64 + r.double()
    al = a2.double().view(1, -1, 1)
    y2_64 = y64 + torch.sin(al * y64) ** 2 / (al + 1e-9)
    assert ops.gemm_split_ok(co, ci, 1, B * T)
    ws = ops.pack_conv_weight_split(w.to(cuda), gg.to(cuda))
    kw = dict(bias=b.to(cuda), pad_left=0, pad_mode=ops.PAD_ZERO, t_out=T, res=r.to(cuda), alpha_y2=a2.to(cuda),
              act=ops.ACT_MISH if act == "mish" else ops.ACT_NONE)
    prof = ops.ConvLaunchProfile()
    ops.set_conv_profile(prof)
    try:
        y, y2 = ops.conv1d(x.to(cuda), None, co, 1, w_split=ws, **kw)
        torch.cuda.synchronize()
    finally:
        ops.set_conv_profile(None)
    assert any("gemm_split" in k for k in prof.summary()), prof.summary().keys()
    yf, y2f = ops.conv1d(x.to(cuda), ops.pack_conv_weight(w.to(cuda), gg.to(cuda)), co, 1, **kw)
    e_split, e_fp32 = rel(y, y64), rel(yf, y64)
    assert e_split < OP_TOL and rel(y2, y2_64) < OP_TOL, (e_split, e_fp32)
    assert e_split < 1.5 * e_fp32 + 1e-7, (e_split, e_fp32)
    _record(f"gemm_split_1x1_{ci}to{co}_T{T}", e_split)
    # transposed form (data gradient of the 1x1): dx = W^T dy
    dy = torch.randn(B, co, T, generator=g)
    dx64 = F.conv_transpose1d(dy.double(), wn.double())
    if ops.gemm_split_ok(ci, co, 1, B * T):
        wt = ops.pack_gemm_weight_split_t(wn.to(cuda))
        dx = ops.conv1d(dy.to(cuda), None, ci, 1, pad_left=0, pad_mode=ops.PAD_ZERO, t_out=T, w_split=wt)
        assert rel(dx, dx64) < OP_TOL


@pytest.mark.parametrize("B,ci,co,T,s", [(2, 192, 96, 1000, 2), (2, 96, 40, 777, 5), (1, 128, 64, 1333, 6), (3, 64, 22, 512, 3),
                                         (2, 384, 192, 960, 5)])
def test_conv_transpose_on_split_gemm(B, ci, co, T, s, O, ops, cuda):
    """Causal ConvTranspose1d with every output phase as a GEMM row on the split-bf16 GEMM kernel (K = 2, row_phases
    epilogue): against the oracle, against fp64, with bias and the pre-activated second output."""
    import torch.nn.functional as F
    g = _g(50 + s + ci)
    x = torch.randn(B, ci, T, generator=g)
    v = torch.randn(ci, co, 2 * s, generator=g) / (ci * 2) ** 0.5
    gg = torch.rand(ci, 1, 1, generator=g) + 0.5
    b = torch.randn(co, generator=g) * 0.1
    a2 = 1 + 0.2 * torch.rand(co, generator=g)
    wn = O.weight_norm_weight(v, gg)
    y = O.sconvtr1d(x, wn, b, s, causal=True)
    assert ops.convtr_split_ok(ci, co, s, B, T)
    wsr = ops.convtr_weight_for(v.to(cuda), gg.to(cuda), s, T, batch=B)
    assert isinstance(wsr, tuple)
    prof = ops.ConvLaunchProfile()
    ops.set_conv_profile(prof)
    try:
        yg, y2 = ops.conv_transpose1d(x.to(cuda), wsr, co, s, bias=b.to(cuda), alpha_y2=a2.to(cuda))
        torch.cuda.synchronize()
    finally:
        ops.set_conv_profile(None)
    assert any("gemm_split" in k for k in prof.summary()), prof.summary().keys()
    assert yg.shape == y.shape and rel(yg, y) < OP_TOL
    assert rel(y2, O.snake(y, a2.view(1, -1, 1))) < OP_TOL
    y64 = F.conv_transpose1d(x.double(), wn.double(), b.double(), stride=s)[..., : T * s]
    yp = ops.conv_transpose1d(x.to(cuda), ops.pack_convtr_weight(v.to(cuda), gg.to(cuda), s), co, s, bias=b.to(cuda))
    e_split, e_fp32 = rel(yg, y64), rel(yp, y64)
    assert e_split < 1.5 * e_fp32 + 1e-7, (e_split, e_fp32)


@pytest.mark.parametrize("B,ci,co,T,k,s,mode", [(4, 64, 128, 641, 4, 2, "reflect"), (2, 128, 256, 2603, 10, 5, "reflect"),
                                                (2, 96, 192, 3070, 12, 6, "reflect"), (1, 128, 512, 3100, 5, 3, "zero"),
                                                (2, 512, 1024, 1600, 5, 3, "zero")])
def test_strided_conv_on_split_gemm(B, ci, co, T, k, s, mode, O, ops, cuda):
    """Strided convs (stride < k <= 2 stride) as 2-tap split GEMMs over the `stride` phase sub-signals: the encoder's causal
    reflect-padded k = 2 s downsampling convs (dac/model/dac.py:62-64) and the period discriminators' zero-padded k = 5 stride-3
    convs (dac/model/discriminator.py:40-46), ragged last frames included, against the oracle / fp64 and the fp32 kernel."""
    import torch.nn.functional as F
    g = _g(70 + k + ci)
    x = torch.randn(B, ci, T, generator=g)
    w = torch.randn(co, ci, k, generator=g) / (ci * k) ** 0.5
    gg = torch.rand(co, 1, 1, generator=g) + 0.5
    b = torch.randn(co, generator=g) * 0.1
    wn = O.weight_norm_weight(w, gg)
    if mode == "reflect":
        t_out = -(-T // s)
        y_ref = O.sconv1d(x, wn, b, stride=s, causal=True)
        kw = dict(bias=b.to(cuda), stride=s)
    else:
        pad = 2
        y_ref = F.conv1d(x.double(), wn.double(), b.double(), stride=s, padding=pad).float()
        t_out = y_ref.shape[-1]
        kw = dict(bias=b.to(cuda), stride=s, pad_left=pad, pad_mode=ops.PAD_ZERO, t_out=t_out)
    assert ops.gemm_split_strided_ok(co, ci, k, s, B, t_out)
    ws = ops.pack_gemm_weight_split(w.to(cuda), gg.to(cuda), in_stride=s)
    prof = ops.ConvLaunchProfile()
    ops.set_conv_profile(prof)
    try:
        y = ops.conv1d(x.to(cuda), None, co, k, w_split=ws, **kw)
        torch.cuda.synchronize()
    finally:
        ops.set_conv_profile(None)
    assert any("gemm_split" in n for n in prof.summary()), prof.summary().keys()
    yf = ops.conv1d(x.to(cuda), ops.pack_conv_weight(w.to(cuda), gg.to(cuda)), co, k, **kw)
    assert y.shape == y_ref.shape and rel(y, y_ref) < OP_TOL and rel(y, yf) < OP_TOL


@pytest.mark.parametrize("B,ci,co,T,k,mode", [(8, 256, 512, 160, 5, "zero"), (5, 1024, 1024, 160, 3, "reflect"), (2, 512, 1024, 333, 5, "zero")])
def test_split_bf16_conv_3_and_5_taps(B, ci, co, T, k, mode, O, ops, cuda):
    """conv1d_bsplit.hip with K = 3 / 5 (the WaveNet and style-encoder k = 5 convs, the encoder's k = 3 output conv at the
    160-frame latent rate): same bars as the K = 7 test."""
    import torch.nn.functional as F
    g = _g(90 + k + ci)
    x = torch.randn(B, ci, T, generator=g)
    w = torch.randn(co, ci, k, generator=g) / (ci * k) ** 0.5
    b = torch.randn(co, generator=g) * 0.1
    if mode == "zero":
        y64 = F.conv1d(x.double(), w.double(), b.double(), padding=k // 2)
        kw = dict(bias=b.to(cuda), pad_left=k // 2, pad_mode=ops.PAD_ZERO, t_out=T)
    else:
        y64 = O.sconv1d(x.double(), w.double(), b.double(), causal=True)
        kw = dict(bias=b.to(cuda))
    ws = ops.pack_conv_weight_split(w.to(cuda))
    prof = ops.ConvLaunchProfile()
    ops.set_conv_profile(prof)
    try:
        y = ops.conv1d(x.to(cuda), None, co, k, w_split=ws, **kw)
        torch.cuda.synchronize()
    finally:
        ops.set_conv_profile(None)
    assert any("bsplit" in n for n in prof.summary()), prof.summary().keys()
    yf = ops.conv1d(x.to(cuda), ops.pack_conv_weight(w.to(cuda)), co, k, **kw)
    e_split, e_fp32 = rel(y, y64), rel(yf, y64)
    assert e_split < OP_TOL and e_split < 1.5 * e_fp32 + 1e-7, (e_split, e_fp32)
    # a split-only launch whose shape no split kernel takes (640 columns: the split-reduction kernel's range) fails loudly
    # instead of reading the bf16 planes as fp32 weights
    with pytest.raises(Exception):
        ops.conv1d(x[:1, :, :100].contiguous().to(cuda), None, co, k, w_split=ws, **{**kw, "t_out": 100} if mode == "zero" else kw)


# ------------------------------------------------------------------------------ backward of the conv stack
BWD_TOL = 1e-4


@pytest.mark.parametrize("B,ci,co,T,k,s,d,mode", [(2, 64, 96, 500, 7, 1, 3, "reflect"), (2, 128, 128, 333, 7, 1, 9, "reflect"),
                                                    (3, 96, 96, 257, 1, 1, 1, "reflect"), (2, 64, 128, 480, 4, 2, 1, "reflect"),
                                                    (1, 256, 512, 300, 10, 5, 1, "reflect"), (2, 40, 24, 200, 5, 1, 2, "zero")])
def test_conv_backward_against_autograd(B, ci, co, T, k, s, d, mode, O, ops, cuda):
    """bwd_data / bwd_weight / weight-norm / bias gradients of SConv1d against torch autograd through the
    CPU oracle (dac/model/encodec.py:212-228 + weight_norm)."""
    g = _g(ci + co + k)
    x = torch.randn(B, ci, T, generator=g, requires_grad=True)
    v = (torch.randn(co, ci, k, generator=g) / (ci * k) ** 0.5).requires_grad_()
    gg = (torch.rand(co, 1, 1, generator=g) + 0.5).requires_grad_()
    b = (torch.randn(co, generator=g) * 0.1).requires_grad_()
    y = O.sconv1d(x, O.weight_norm_weight(v, gg), b, stride=s, dilation=d, causal=True, pad_mode=mode)
    r = torch.randn(*y.shape, generator=g)
    (y * r).sum().backward()
    pm = ops.PAD_REFLECT if mode == "reflect" else ops.PAD_ZERO
    dy = r.to(cuda)
    vd, gd = v.detach().to(cuda), gg.detach().to(cuda)
    dx = ops.conv1d_bwd_data(dy, vd, gd, T, stride=s, dilation=d, pad_mode=pm)
    dw = ops.conv1d_bwd_weight(x.detach().to(cuda), dy, k, stride=s, dilation=d, pad_mode=pm)
    dv, dg = ops.weight_norm_bwd(vd, gd, dw)
    db = ops.bias_grad(dy)
    assert rel(dx, x.grad) < BWD_TOL
    assert rel(dv, v.grad) < BWD_TOL and rel(dg, gg.grad) < BWD_TOL
    assert rel(db, b.grad) < BWD_TOL


def test_snake_backward_against_autograd(O, ops, cuda):
    g = _g(5)
    x = torch.randn(3, 48, 700, generator=g, requires_grad=True)
    al = (1 + 0.3 * torch.rand(48, generator=g)).requires_grad_()
    y = O.snake(x, al.view(1, -1, 1))
    r = torch.randn(*y.shape, generator=g)
    (y * r).sum().backward()
    dx, da = ops.snake_bwd(x.detach().to(cuda), al.detach().to(cuda), r.to(cuda))
    assert rel(dx, x.grad) < BWD_TOL and rel(da, al.grad) < BWD_TOL


@pytest.mark.parametrize("B,ci,co,T,s", [(2, 128, 64, 160, 6), (1, 96, 48, 333, 5), (2, 64, 32, 500, 2)])
def test_conv_transpose_backward_against_autograd(B, ci, co, T, s, O, ops, cuda):
    g = _g(ci + s)
    x = torch.randn(B, ci, T, generator=g, requires_grad=True)
    v = (torch.randn(ci, co, 2 * s, generator=g) / (ci * 2) ** 0.5).requires_grad_()
    gg = (torch.rand(ci, 1, 1, generator=g) + 0.5).requires_grad_()
    b = (torch.randn(co, generator=g) * 0.1).requires_grad_()
    y = O.sconvtr1d(x, O.weight_norm_weight(v, gg), b, s, causal=True)
    r = torch.randn(*y.shape, generator=g)
    (y * r).sum().backward()
    vd, gd = v.detach().to(cuda), gg.detach().to(cuda)
    dx, dw = ops.conv_transpose1d_bwd(x.detach().to(cuda), r.to(cuda), vd, gd, s)
    dv, dg = ops.weight_norm_bwd(vd, gd, dw)
    assert rel(dx, x.grad) < BWD_TOL and rel(dv, v.grad) < BWD_TOL and rel(dg, gg.grad) < BWD_TOL
    assert rel(ops.bias_grad(r.to(cuda)), b.grad) < BWD_TOL


def _grad_parity(mod, sd, out_fn, x, cuda, tol):
    """Gradients of sum(out * r) w.r.t. the input and every parameter: HIP autograd path vs torch autograd through
    the CPU oracle on the same state dict."""
    leaves = {k: v.clone().requires_grad_() for k, v in sd.items() if v.dtype.is_floating_point}
    xr = x.clone().requires_grad_()
    y_ref = out_fn(leaves, xr)
    r = torch.randn(*y_ref.shape, generator=_g(99))
    (y_ref * r).sum().backward()
    mod.to(cuda).train()
    xg = x.to(cuda).requires_grad_()
    y = mod(xg)
    assert rel(y, y_ref) < tol
    (y * r.to(cuda)).sum().backward()
    assert rel(xg.grad, xr.grad) < tol, "input grad"
    worst = ("", 0.0)
    for n, p in mod.named_parameters():
        assert p.grad is not None, n
        e = rel(p.grad, leaves[n].grad)
        if e > worst[1]:
            worst = (n, e)
    assert worst[1] < tol, worst


def test_encoder_backward_against_autograd(O, cuda):
    """Training-mode Encoder (convs, Snake, weight-norm, strided convs, 2-layer LSTM with BPTT): every gradient
    against autograd through the oracle."""
    from facodec_amd.dac_model import Encoder
    enc = Encoder(d_model=8, strides=[2, 5, 5, 6], d_latent=64, causal=True, lstm=2)
    sd = synth.load_synthetic(enc, seed=4, prefix="encoder.")
    x = synth.synth_clips(2, 4800, seed=6)      # every layer longer than its reflect pad (54 at 1/50 rate)
    _grad_parity(enc, sd, lambda s, xx: O.encoder_forward(s, xx, rates=(2, 5, 5, 6), lstm=2), x, cuda, 2e-4)


def test_in_place_reflect_fold_is_bit_identical_to_the_unpadding_copy(cuda):
    """Round 6: the data gradient of a ResidualUnit's k = 7 conv reaches the Snake backward of the producing node as the window
    [pad_left, pad_left + T) of the padded gradient rows -- mirrored edge samples added in place (fac_pad_fold_edges), rows read
    with a stride (fac_snake_bwd_fused_rs) -- instead of through an un-padding copy of the whole tensor (fac_pad_fold_bwd).  Same
    additions in the same order: every gradient of an Encoder backward equals the copying path's bit for bit
    (FAC_FOLD_IN_PLACE=0), and the view path is the one that runs."""
    from facodec_amd import ops
    from facodec_amd.dac_model import Encoder

    def grads(flag):
        ops.FOLD_IN_PLACE = flag
        taken = []
        orig = ops.snake_bwd_fused

        def spy(x, alpha, dy, add=None, want_bias=False):
            taken.append(bool(dy is not None and not dy.is_contiguous()))
            return orig(x, alpha, dy, add=add, want_bias=want_bias)

        ops.snake_bwd_fused = spy
        try:
            enc = Encoder(d_model=16, strides=[2, 5, 5, 6], d_latent=64, causal=True, lstm=0)
            synth.load_synthetic(enc, seed=4, prefix="encoder.")
            enc.to(cuda).train()
            x = synth.synth_clips(2, 4800, seed=6).to(cuda).requires_grad_()
            y = enc(x)
            (y * torch.randn(*y.shape, generator=_g(3)).to(cuda)).sum().backward()
            return [x.grad.clone()] + [p.grad.clone() for p in enc.parameters()], taken
        finally:
            ops.snake_bwd_fused = orig
            ops.FOLD_IN_PLACE = 1

    (a, took_view), (b, took_copy) = grads(1), grads(0)
    assert any(took_view) and not any(took_copy)
    assert len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


def test_short_clip_training_convs_run_flattened(cuda):
    """Round 6: at the 160-frame latent rate the training launches of the encoder's last strided conv and the decoder's first
    ConvTranspose1d (forward AND data gradient) run as ONE flattened signal on the split GEMM kernel (ops.conv1d_flat /
    conv_transpose1d_flat) instead of per clip on the fp32 128 x 160 tile.  Same mathematical products: outputs and gradients
    within 1e-5 of the per-clip path (FAC_FLAT_TRAIN=0), and the flattened launch is the one that runs."""
    from facodec_amd import autograd as A
    from facodec_amd import ops
    from facodec_amd.layers import SConv1d, SConvTranspose1d
    g = _g(12)
    B = 16
    down = SConv1d(128, 256, kernel_size=12, stride=6, causal=True, norm="weight_norm").to(cuda)
    up = SConvTranspose1d(256, 128, kernel_size=12, stride=6, causal=True, norm="weight_norm").to(cuda)
    x = torch.randn(B, 128, 960, generator=g).to(cuda)
    r1 = torch.randn(B, 256, 160, generator=g).to(cuda)
    r2 = torch.randn(B, 128, 960, generator=g).to(cuda)

    def run(flag):
        ops.FLAT_TRAIN = flag
        names = []
        orig = ops._launch_conv

        def spy(d, what):
            orig(d, what)                   # first: the launch hands the descriptor its workspace, which the selection reads
            names.append((d.B, ops.conv_variant(d)[1][:28]))

        ops._launch_conv = spy
        try:
            xi = x.clone().requires_grad_()
            y = A.conv(down, xi)
            z = A.conv_tr(up, y)
            ((y * r1).sum() + (z * r2).sum()).backward()
            grads = [xi.grad.clone()] + [p.grad.clone() for m in (down, up) for p in m.parameters()]
            for m in (down, up):
                for p in m.parameters():
                    p.grad = None
            return y.detach(), z.detach(), grads, names
        finally:
            ops._launch_conv = orig
            ops.FLAT_TRAIN = True

    y1, z1, g1, n1 = run(True)
    y0, z0, g0, n0 = run(False)
    assert sum(1 for b, n in n1 if b == 1 and "gemm_split" in n) >= 4 and not any(b == 1 for b, n in n0)       # fwd x 2, data gradient x 2
    assert rel(y1, y0) < 1e-5 and rel(z1, z0) < 1e-5
    for a, b in zip(g1, g0):
        assert rel(a, b) < 1e-5


_MEASURED = {}


def _record(name, value):
    """Keeps the measured worst-case errors of the gradient tests (gpurun_out/tolerance_report.json) so the bars in this
    file can be stated next to what the hardware actually does."""
    import json
    _MEASURED[name] = value
    os.makedirs("gpurun_out", exist_ok=True)
    json.dump(_MEASURED, open("gpurun_out/tolerance_report.json", "w"), indent=1, sort_keys=True)


def test_decoder_backward_against_autograd(O, cuda):
    from facodec_amd.dac_model import Decoder
    dec = Decoder(input_channel=64, channels=128, rates=[6, 5, 5, 2], causal=True, lstm=2)
    sd = synth.load_synthetic(dec, seed=5, prefix="decoder.")
    z = torch.randn(2, 64, 12, generator=_g(8))
    _grad_parity(dec, sd, lambda s, zz: O.decoder_forward(s, zz, rates=(6, 5, 5, 2), causal=True, lstm=2), z, cuda, 2e-4)


def test_mel_loss_backward_against_autograd(O, cuda):
    """d MelSpectrogramLoss / d estimate (train.py:155-163 configuration, 7 scales) against autograd through the
    oracle's STFT / mel restatement.  L1 of logs has kinks; the bar is on the whole gradient field."""
    from facodec_amd import losses
    y = synth.synth_clips(2, 24000, seed=21)
    x = (0.6 * y + 0.1 * synth.synth_clips(2, 24000, seed=22)).contiguous().requires_grad_()
    ref = O.mel_spectrogram_loss(x, y)
    ref.backward()
    mel = losses.MelSpectrogramLoss(n_mels=[5, 10, 20, 40, 80, 160, 320], window_lengths=[32, 64, 128, 256, 512, 1024, 2048],
                                    mel_fmin=[0] * 7, mel_fmax=[None] * 7, pow=1.0, mag_weight=0.0, clamp_eps=1e-5)
    xg = x.detach().to(cuda).requires_grad_()
    got = mel(xg, y.to(cuda))
    assert abs(float(got) - float(ref)) / float(ref) < E2E_TOL
    (3.0 * got).backward()
    _record("mel_loss_input_gradient", rel(xg.grad, 3.0 * x.grad))
    assert rel(xg.grad, 3.0 * x.grad) < 5e-5          # measured on MI355X: 3.1e-6 (profiles/r02_tolerance_report.json)


def test_reconstruction_loss_backward_against_autograd(O, cuda):
    """d reconstruction_loss / d G_x (losses.py:65-89: 100 MSE + six mel scales of L1 + sqrt(s/2) log-RMS) against autograd
    through the oracle's restatement; the value is unchanged by the autograd wrapper."""
    from facodec_amd import losses
    x = synth.synth_clips(2, 16000, seed=31)[:, 0]
    gx = (0.7 * x + 0.05 * synth.synth_clips(2, 16000, seed=32)[:, 0]).contiguous().requires_grad_()
    ref = O.reconstruction_loss(x, gx)
    ref.backward()
    gg = gx.detach().to(cuda).requires_grad_()
    got = losses.reconstruction_loss(x.to(cuda), gg)
    assert abs(float(got) - float(ref)) / float(ref) < E2E_TOL
    assert abs(float(got) - float(losses.reconstruction_loss(x.to(cuda), gg.detach()))) / float(ref) < 1e-6
    (2.0 * got).backward()
    _record("reconstruction_loss_input_gradient", rel(gg.grad, 2.0 * gx.grad))
    assert rel(gg.grad, 2.0 * gx.grad) < 1e-4


def test_rvq_backward_against_autograd(O, cuda):
    """Training-mode RVQ (3 quantizers, quantizer-dropout masks, straight-through, commitment 0.25 + codebook 1.0 as
    in train.py:357-358): gradients of the input and of every in_proj / codebook / out_proj parameter."""
    from facodec_amd import autograd as A
    from facodec_amd.quantize import ResidualVectorQuantize
    rvq = ResidualVectorQuantize(256, 3, 1024, 8)
    sd = synth.load_synthetic(rvq, seed=13)
    g = _g(31)
    z = torch.randn(4, 256, 150, generator=g)
    mask = torch.tensor([[1, 1, 1, 1], [1, 0, 1, 1], [0, 0, 1, 1]], dtype=torch.float32)
    r = torch.randn(4, 256, 150, generator=g)
    leaves = {k: v.clone().requires_grad_() for k, v in sd.items()}
    zr = z.clone().requires_grad_()
    zq_ref, codes_ref, c_ref, cb_ref = O.rvq_forward_train(zr, leaves, "", 3, mask)
    ((zq_ref * r).sum() + 0.25 * c_ref + 1.0 * cb_ref).backward()
    rvq.to(cuda).train()
    zg = z.to(cuda).requires_grad_()
    zq, codes, c, cb = A.rvq(rvq, zg, mask.to(cuda))
    assert torch.equal(codes.cpu(), codes_ref)
    assert rel(zq, zq_ref) < OP_TOL and abs(float(c) - float(c_ref)) / float(c_ref) < 1e-5
    ((zq * r.to(cuda)).sum() + 0.25 * c + 1.0 * cb).backward()
    assert rel(zg.grad, zr.grad) < BWD_TOL
    for n, p in rvq.named_parameters():
        assert rel(p.grad, leaves[n].grad) < BWD_TOL, n


def test_layernorm_affine_backward_against_autograd(O, cuda):
    from facodec_amd import autograd as A
    g = _g(41)
    x = torch.randn(3, 1024, 50, generator=g, requires_grad=True)
    style = torch.randn(3, 2048, generator=g, requires_grad=True)
    gamma, beta = style[:, :1024, None], style[:, 1024:, None]
    y = torch.nn.functional.layer_norm(x.transpose(1, 2), (1024,), eps=1e-5).transpose(1, 2) * gamma + beta
    r = torch.randn(3, 1024, 50, generator=g)
    (y * r).sum().backward()
    xg, sg = x.detach().to(cuda).requires_grad_(), style.detach().to(cuda).requires_grad_()
    out = A.layernorm_affine(xg, sg)
    assert rel(out, y) < OP_TOL
    (out * r.to(cuda)).sum().backward()
    assert rel(xg.grad, x.grad) < BWD_TOL and rel(sg.grad, style.grad) < BWD_TOL


def test_flat_adamw_matches_torch(cuda):
    """Fused arena AdamW + clip + ExponentialLR against torch.optim.AdamW / clip_grad_norm_ / ExponentialLR on CPU."""
    from facodec_amd.optim import FlatAdamW
    g = _g(77)
    shapes = [(64, 32, 7), (64, 1, 1), (64,), (1, 96, 1), (300, 17), (3 * 2048 + 5,)]     # the last: whole 2048-element chunks
    ref = [torch.randn(*s, generator=g).requires_grad_() for s in shapes]
    ours = [r.detach().clone().to(cuda).requires_grad_() for r in ref]
    p0 = [r.detach().clone() for r in ref]
    opt_ref = torch.optim.AdamW(ref, lr=1e-3, betas=(0.9, 0.98), eps=1e-9, weight_decay=0.1)
    sch = torch.optim.lr_scheduler.ExponentialLR(opt_ref, gamma=0.99)
    opt = FlatAdamW(ours, lr=1e-3, gamma=0.99, max_norm=2.0)
    for it in range(4):
        grads = [torch.randn(*s, generator=g) * (3.0 if it % 2 else 0.01) for s in shapes]
        for r, o, gr in zip(ref, ours, grads):
            r.grad = gr.clone()
            o.grad = gr.to(cuda)
        nrm = torch.nn.utils.clip_grad_norm_(ref, 2.0)
        opt_ref.step()
        sch.step()
        opt.step()
        assert abs(float(opt.grad_norm()) - float(nrm)) / float(nrm) < 1e-5
    for r, o in zip(ref, ours):
        assert rel(o, r) < 1e-5
    # the accumulated UPDATE, relative to the largest update: four steps move a parameter by about 4e-3, so the bar on p above is
    # 1e-2 of the movement.  Both sides round p (|p| < 8: half an ulp is at most 2^-22) once per step, so the two differ by at
    # most 8 * 2^-22 = 1.9e-6 = 4.8e-4 of a 4e-3 movement, plus the same fp32 formula in another order (a few 1e-7 relative):
    # bar 1e-3, a tenth of what a wrong bias correction at steps 1 .. 4 shows (> 1e-2).
    for r, o, p in zip(ref, ours, p0):
        du, du_ref = o.detach().cpu().double() - p.double(), r.detach().double() - p.double()
        assert float((du - du_ref).abs().max() / du_ref.abs().max()) < 1e-3


def test_gather_copy_folds_many_tensors_bit_exactly(cuda, monkeypatch):
    """fac_gather_copy (the fold of autograd's gradient tensors into the optimiser arena): 300 tensors -- one element to several
    workgroups' worth, odd lengths, destinations at element offsets that are not 16-byte aligned, non-contiguous and fp64 sources
    (left to torch) -- land exactly where `copy_` puts them, and nothing else of the arena changes."""
    from facodec_amd import optim
    g = _g(5)
    sizes = [1, 2, 3, 5, 64, 255, 1023, 4097, 8192, 8193, 70001] * 27 + [3, 1 << 20, 7]
    assert len(sizes) == 300
    arena = torch.full((sum(sizes) + 64,), -7.0, device=cuda)
    ref = arena.clone()
    dst, src, off = [], [], 5                       # first destination starts 20 bytes into the arena
    for j, n in enumerate(sizes):
        d = arena[off:off + n]
        if j % 50 == 7:
            s_ = torch.randn(n, 2, generator=g).to(cuda)[:, 0]            # non-contiguous
        elif j % 50 == 9:
            s_ = torch.randn(n, generator=g).double().to(cuda)           # another dtype
        else:
            s_ = torch.randn(n, generator=g).to(cuda)
        ref[off:off + n].copy_(s_)
        dst.append(d)
        src.append(s_)
        off += n
    optim._fold(dst, src)
    assert torch.equal(arena, ref)
    arena2 = torch.full_like(arena, -7.0)
    monkeypatch.setattr(optim, "GATHER_COPY", False)
    optim._fold([arena2[d.storage_offset():d.storage_offset() + d.numel()] for d in dst], src)
    assert torch.equal(arena2, ref)


def test_generator_step_gradients_against_autograd(O, cuda):
    """encoder -> FA-quantizer (training mode, fixed dropout masks) -> decoder -> 15 mel + 0.25 commitment + codebook:
    gradients of every trained parameter (timbre encoder and prosody WaveNet included; Bernoulli dropouts off for the
    comparison) against autograd through the oracle, then one optimiser step runs."""
    from facodec_amd.commons import build_model, default_model_params
    from facodec_amd.train import GeneratorStep
    model = build_model(default_model_params())
    sds = {}
    for k in ("encoder", "quantizer", "decoder"):
        sds[k] = synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].to(cuda)
    B, T = 2, 4800
    wave = synth.synth_clips(B, T, seed=17)
    masks = dict(p=torch.ones(1, B), c=torch.tensor([[1.0, 1.0], [1.0, 0.0]]), r=torch.tensor([[1.0, 1.0], [1.0, 1.0], [0.0, 1.0]]),
                 res=torch.tensor([1.0, 1.0]), dropout=False)
    # ---- reference: autograd through the oracle
    leaves = {k: {n: v.clone().requires_grad_() for n, v in sd.items() if v.dtype.is_floating_point} for k, sd in sds.items()}
    z = O.encoder_forward(leaves["encoder"], wave)
    outs, _, cm, cb, _, codes_ref = O.quantizer_forward_train(leaves["quantizer"], z, wave, masks, side_branches_no_grad=False)
    y = O.decoder_forward(leaves["decoder"], outs)
    mel_ref = O.mel_spectrogram_loss(y, wave)
    (15.0 * mel_ref + 0.25 * cm + 1.0 * cb).backward()
    # ---- product
    step = GeneratorStep(model)
    out = step.forward_backward(wave.to(cuda), masks)
    assert abs(float(out["mel"]) - float(mel_ref)) / float(mel_ref) < 2e-4
    assert abs(float(out["commitment"]) - float(cm)) / float(cm) < 2e-4
    worst = ("", 0.0)
    n_checked = 0
    for k in ("encoder", "quantizer", "decoder"):
        for n, p in model[k].named_parameters():
            ref = leaves[k][n].grad
            if ref is None:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, (k, n)   # no path in the reference: zero here
                continue
            if float(ref.abs().max()) < 1e-7:      # e.g. the key bias of an attention layer: softmax is shift-invariant
                assert float(p.grad.abs().max()) < 1e-6, (k, n)
                continue
            e = rel(p.grad, ref)
            n_checked += 1
            if e > worst[1]:
                worst = (k + "." + n, e)
    _record("generator_step_worst_parameter_gradient", list(worst))
    # measured worst of the 361 tensors: 2.1e-4 (residual_quantizer.quantizers.0.in_proj.weight_g, a 1024-term weight-norm
    # reduction of a gradient that is itself a sum over all frames); every other tensor is below 1e-4
    assert n_checked > 250 and worst[1] < 5e-4, (n_checked, worst)
    for k in ("encoder", "decoder", "quantizer"):
        step.opt[k].step()
    assert all(torch.isfinite(step.opt[k].p).all() for k in step.opt)


def test_style_encoder_and_wavenet_backward_against_autograd(O, cuda):
    from facodec_amd import autograd_quant as AQ
    from facodec_amd.quantize import StyleEncoder, WN
    se = StyleEncoder(80, 512, 1024)
    sd = synth.load_synthetic(se, seed=7)
    mel = torch.randn(3, 80, 50, generator=_g(1))
    mask = torch.ones(3, 50)
    mask[1, 30:] = 0
    mask[2, 10:] = 0
    leaves = {k: v.clone().requires_grad_() for k, v in sd.items()}
    ref = O.style_encoder_forward(mel, leaves, "", mask.unsqueeze(1))
    r = torch.randn(*ref.shape, generator=_g(2))
    (ref * r).sum().backward()
    se.to(cuda).train()
    out = AQ.style_encoder(se, mel.to(cuda), mask.to(cuda), use_dropout=False)
    assert rel(out, ref) < OP_TOL
    (out * r.to(cuda)).sum().backward()
    for n, p in se.named_parameters():
        if float(leaves[n].grad.abs().max()) < 1e-7:   # slf_attn.conv_k.bias: softmax is invariant to a key shift
            assert float(p.grad.abs().max()) < 1e-6, n
            continue
        assert rel(p.grad, leaves[n].grad) < BWD_TOL, n
    # dropout on: still finite, different from the deterministic output
    out_d = AQ.style_encoder(se, mel.to(cuda), mask.to(cuda), use_dropout=True)
    assert torch.isfinite(out_d).all() and rel(out_d, ref) > 1e-3
    wn = WN(256, 5, 1, 8, causal=True)
    sdw = synth.load_synthetic(wn, seed=8)
    x = torch.randn(2, 256, 160, generator=_g(3), requires_grad=True)
    lw = {k: v.clone().requires_grad_() for k, v in sdw.items()}
    refw = O.wavenet_forward(x, lw, "", 256, 8)
    rw = torch.randn(*refw.shape, generator=_g(4))
    (refw * rw).sum().backward()
    wn.to(cuda).train()
    xg = x.detach().to(cuda).requires_grad_()
    outw = AQ.wavenet(wn, xg, use_dropout=False)
    assert rel(outw, refw) < OP_TOL
    (outw * rw.to(cuda)).sum().backward()
    assert rel(xg.grad, x.grad) < BWD_TOL
    for n, p in wn.named_parameters():
        assert rel(p.grad, lw[n].grad) < BWD_TOL, n


def test_predictor_heads_backward_against_autograd(O, cuda):
    """A CNNLSTM head (3 anti-aliased-SnakeBeta residual units + Linear heads) in training mode: input and parameter
    gradients against autograd through the oracle; plus the gradient-reversal sign."""
    from facodec_amd import autograd_pred as AP
    from facodec_amd.predictors import CNNLSTM
    head = CNNLSTM(64, 5, 2)
    synth.load_synthetic(head, seed=21)
    params = {n for n, _ in head.named_parameters()}
    x = torch.randn(2, 64, 300, generator=_g(9), requires_grad=True)
    leaves = {k: (v.clone().requires_grad_() if k in params else v.clone()) for k, v in head.state_dict().items()}
    refs = O.cnnlstm_forward(x, leaves, "", 2)
    rs = [torch.randn(*r.shape, generator=_g(10 + i)) for i, r in enumerate(refs)]
    sum((r * w).sum() for r, w in zip(refs, rs)).backward()
    head.to(cuda).train()
    xg = x.detach().to(cuda).requires_grad_()
    outs = AP.cnnlstm(head, xg)
    for o, r in zip(outs, refs):
        assert rel(o, r) < OP_TOL
    sum((o * w.to(cuda)).sum() for o, w in zip(outs, rs)).backward()
    assert rel(xg.grad, x.grad) < BWD_TOL
    for n, p in head.named_parameters():
        assert rel(p.grad, leaves[n].grad) < BWD_TOL, n
    # gradient reversal: identity forward, negated gradient
    z = torch.randn(2, 8, 5, device=cuda, requires_grad=True)
    y = AP._GradReverse.apply(z, 1.0)
    y.sum().backward()
    assert torch.equal(y.detach(), z.detach()) and torch.allclose(z.grad, -torch.ones_like(z))


def test_discriminator_forward_backward(O, cuda, golden_dir):
    """MPD x5 + MRD x3 (dac/model/discriminator.py) on the 1-D conv kernels: logits against the real reference's golden
    (tests/golden/discriminator.npz), every feature map against the oracle, and the gradients of
    loss_d / loss_g + loss_feature (train.py:282-312) w.r.t. the waveform and every parameter against autograd."""
    from facodec_amd import discriminator as D
    disc = D.Discriminator(sample_rate=24000)
    sd = synth.load_synthetic(disc, seed=0, prefix="discriminator.")
    gold = np.load(os.path.join(golden_dir, "discriminator.npz"))
    x = synth.synth_clips(2, 24000, seed=5)
    disc.to(cuda)
    with torch.no_grad():
        fm = disc.forward_internal(x.to(cuda))
        ref_l = D.reference_layout(disc, fm, 2)
        views = disc(x.to(cuda))                         # the drop-in structure: zero-copy views of the same maps
    for a, v in zip(ref_l, views):
        for u, w in zip(a, v):
            assert u.shape == w.shape and torch.equal(u, w.contiguous())
    fm_or = O.discriminator_forward(sd, x)
    for i, (a, b) in enumerate(zip(ref_l, fm_or)):
        assert rel(a[-1], gold[f"logit{i}"]) < E2E_TOL, i
        for j, (u, w) in enumerate(zip(a, b)):
            assert u.shape == w.shape and rel(u, w) < E2E_TOL, (i, j)
    # gradients: generator-side losses w.r.t. the fake waveform, discriminator loss w.r.t. the parameters
    xr = synth.synth_clips(2, 24000, seed=6)
    leaves = {k: v.clone().requires_grad_() for k, v in sd.items()}
    xf_ref = x.clone().requires_grad_()
    df, dr = O.discriminator_forward(leaves, xf_ref), O.discriminator_forward(leaves, xr)
    ld, lg, lf = O.gan_losses(df, dr)
    (ld + 0.5 * lg + 0.25 * lf).backward()
    xf = x.to(cuda).requires_grad_()
    d_fake, d_real = disc(xf), disc(xr.to(cuda))
    loss_d, loss_g, loss_f = D.gan_losses(d_fake, d_real)
    assert abs(float(loss_d) - float(ld)) / float(ld) < 2e-4 and abs(float(loss_f) - float(lf)) / float(lf) < 2e-4
    (loss_d + 0.5 * loss_g + 0.25 * loss_f).backward()
    _record("discriminator_input_gradient", rel(xf.grad, xf_ref.grad))
    assert rel(xf.grad, xf_ref.grad) < 1e-4            # measured: 1.2e-6
    worst = ("", 0.0)
    for n, p in disc.named_parameters():
        e = rel(p.grad, leaves[n].grad)
        if e > worst[1]:
            worst = (n, e)
    _record("discriminator_worst_parameter_gradient", list(worst))
    # measured worst: 1.4e-3 on discriminators.2.convs.0.0.weight_v -- the 1 -> 32 channel first conv of a period
    # discriminator: each of its 160 weights is ONE fp32 sum over ~48 000 (clip, position) products with heavy cancellation,
    # and the reference side here is the oracle's fp32 autograd on the CPU with a different summation order.  The same
    # tensor family agrees with the real reference to 6e-6 in tests/test_train_golden.py (4 x 6000-sample clips).
    assert worst[1] < 2e-3, worst


def _disc_fp64_grads(O, sd, x, xr, kinks=None, l1_signs=None):
    """Gradients of loss_d + 0.5 loss_g + 0.25 loss_feature (as above) through the oracle in float64, from the same fp32 values.
    kinks: None, or one boolean mask per LeakyReLU call of the two forwards (fake clip, then real clip; call order = feature-map
    order): the slope-1 side is taken where the mask is set, whatever the sign of the fp64 pre-activation -- float64 arithmetic on
    the kink pattern of another evaluation.  l1_signs: None, or sign(fake - real) per feature-matching map (the L1 loss's kink):
    the feature loss is then taken as mean(sign * (fake - real)), whose gradient is that of the L1 loss on those signs.  Returns (waveform gradient, {parameter: gradient}, (fake maps, real maps) detached,
    {first MPD conv: conditioning max over its weights of sum|x dy| / |sum x dy|})."""
    import torch.nn.functional as F
    leaves = {k: v.double().clone().requires_grad_() for k, v in sd.items()}
    xf = x.double().clone().requires_grad_()
    first = []
    conv2d, leaky = F.conv2d, F.leaky_relu
    masks = iter(kinks) if kinks is not None else None

    def conv_spy(inp, w, *a, **kw):
        out = conv2d(inp, w, *a, **kw)
        if w.shape[1] == 1 and w.shape[2:] == (5, 1) and out.requires_grad:
            out.retain_grad()
            first.append((inp, out, a, kw))
        return out

    def leaky_kinked(inp, slope, *a, **kw):
        m = next(masks)
        assert m.shape == inp.shape, (m.shape, inp.shape)
        return torch.where(m, inp, inp * slope)

    O.F.conv2d = conv_spy
    if masks is not None:
        O.F.leaky_relu = leaky_kinked
    try:
        df, dr = O.discriminator_forward(leaves, xf), O.discriminator_forward(leaves, xr.double())
    finally:
        O.F.conv2d, O.F.leaky_relu = conv2d, leaky
    if masks is not None:
        assert next(masks, None) is None
    ld, lg, lf = O.gan_losses(df, dr)
    if l1_signs is not None:
        sg = iter(l1_signs)
        lf = sum((next(sg) * (a[j] - b[j].detach())).mean() for a, b in zip(df, dr) for j in range(len(a) - 1))
    (ld + 0.5 * lg + 0.25 * lf).backward()
    cond = {}
    for i, (inp, out, a, kw) in enumerate(first[:len(first) // 2]):      # the fake clip's five first convs (the real ones follow)
        stride = kw.get("stride", 1)
        padding = kw.get("padding", 0)
        num = torch.nn.grad.conv2d_weight(inp.detach().abs(), (out.shape[1], 1, 5, 1), out.grad.abs(), stride=stride, padding=padding)
        den = torch.nn.grad.conv2d_weight(inp.detach(), (out.shape[1], 1, 5, 1), out.grad, stride=stride, padding=padding)
        cond[f"discriminators.{i}.convs.0.0"] = float((num / den.abs().clamp_min(1e-300)).max())
    maps = tuple([[m.detach() for m in d] for d in dd] for dd in (df, dr))
    return xf.grad, {k: v.grad for k, v in leaves.items()}, maps, cond


def _starts(maps):
    """Index of each discriminator's first activated map in _activated(maps)."""
    out, n = [], 0
    for d in maps:
        out.append(n)
        n += len(d) - 1
    return out


def _activated(maps):
    """The LeakyReLU outputs among a discriminator output structure: every map but each discriminator's last (its logits)."""
    return [m for d in maps for m in d[:-1]]


# Bars on the max-relative error of every discriminator parameter gradient (worst tensor) and of the waveform gradient, against
# float64 autograd (a) on the HIP forward's own kinks and (b) plainly.  Measured on MI355X (2 clips each):
#   (a) worst tensor 7.0e-7 (T = 24000), 6.4e-7 (2310), 3.5e-6 (1500); waveform 1.0e-7, 3.2e-8, 1.3e-7.  This is the kernels' error.
#   (b) worst tensor 5.6e-4 (T = 24000, discriminators.5.band_convs.2.0.0.weight_v), 2.0e-5 (2310), 1.2e-2 (1500,
#       discriminators.6.band_convs.0.3.0.weight_v); waveform 2.1e-7, 3.3e-8, 2.5e-5.  The excess over (a) is kinks, not rounding:
#       at T = 24000 the HIP forward puts 13 LeakyReLU pre-activations (both clips) and 10 feature-matching differences
#       (fake - real) on the other side of 0 from fp64; at T = 1500 a single feature-matching difference of the 1024-point MRD's
#       lowest band does (its map has 6 frames per clip, so one element's sign(fake - real) carries a 1/n that large), and at
#       T = 2310 one of the first period discriminator.  With the same kinks as the HIP forward, fp64 agrees to (a).
DISC_KINKED_BARS = {24000: (5e-6, 1e-6), 2310: (5e-6, 3e-7), 1500: (2e-5, 1e-6)}
DISC_FP64_BARS = {24000: (1e-3, 1e-6), 2310: (1e-4, 2e-7), 1500: (2e-2, 1e-4)}


@pytest.mark.parametrize("T", [24000, 2310, 1500], ids=["T24000", "T2310_full_period_pads", "T1500_shorter_than_mrd_window"])
def test_discriminator_gradients_against_fp64(O, cuda, T):
    """Every discriminator parameter gradient and the waveform gradient of the HIP path against float64 autograd through the
    oracle, from the same fp32-rounded clips and weights.  T = 2310: every period divides T (MPD pads a full period); T = 1500:
    shorter than the 2048-point MRD window, long enough for its reflect pads.

    LeakyReLU is not differentiable at 0: where a pre-activation lies within rounding of 0, fp32 and fp64 can take different sides,
    and the gradient through that element moves by 0.9 |dy| -- not a rounding error.  So the HIP forward's pre-activation signs
    (the sign of each activated map: LeakyReLU keeps it) are compared with fp64's for BOTH clips, and the gradients are compared
    twice: against fp64 evaluated on the HIP forward's kink pattern, which isolates the kernels' own error, and against plain
    fp64.  The same holds for the feature-matching L1 (|fake - real| at fake ~ real), whose signs are matched too."""
    from facodec_amd import discriminator as D
    disc = D.Discriminator(sample_rate=24000)
    sd = synth.load_synthetic(disc, seed=0, prefix="discriminator.")
    x = synth.synth_clips(2, T, seed=5)
    xr = synth.synth_clips(2, T, seed=6)
    disc.to(cuda)
    xf = x.to(cuda).requires_grad_()
    d_fake, d_real = disc(xf), disc(xr.to(cuda))
    loss_d, loss_g, loss_f = D.gan_losses(d_fake, d_real)
    (loss_d + 0.5 * loss_g + 0.25 * loss_f).backward()
    torch.cuda.synchronize()
    hip_maps = [m.detach().cpu() for m in _activated(d_fake) + _activated(d_real)]
    gx, gp, maps64, cond = _disc_fp64_grads(O, sd, x, xr)
    ref_maps = _activated(maps64[0]) + _activated(maps64[1])
    names = [f"{c}.d{i}.m{j}" for c, mm in (("fake", maps64[0]), ("real", maps64[1])) for i, d in enumerate(mm) for j in range(len(d) - 1)]
    flips = {n: int(((h > 0) != (r > 0)).sum()) for n, h, r in zip(names, hip_maps, ref_maps)}
    flips = {n: c for n, c in flips.items() if c}
    fwd_err = max(rel(h, r) for h, r in zip(hip_maps, ref_maps))
    errs = {n: rel(p.grad, gp[n]) for n, p in disc.named_parameters()}
    worst = max(errs.items(), key=lambda kv: kv[1])
    ex = rel(xf.grad, gx)
    # the feature-matching loss is an L1 of (fake - real): a second kind of kink, where the two clips' maps nearly agree
    hf, hr = [[m.detach().cpu().double() for m in d[:-1]] for d in d_fake], [[m.detach().cpu().double() for m in d[:-1]] for d in d_real]
    hip_l1 = [torch.sign(a - b) for da, db in zip(hf, hr) for a, b in zip(da, db)]
    ref_l1 = [torch.sign(a - b) for da, db in zip(maps64[0], maps64[1]) for a, b in zip(da[:-1], db[:-1])]
    l1_flips = {f"d{i}": int(sum(int((a != b).sum()) for a, b in zip(hip_l1[n0:n0 + len(d) - 1], ref_l1[n0:n0 + len(d) - 1])))
                for i, (d, n0) in enumerate(zip(maps64[0], _starts(maps64[0])))}
    l1_flips = {k: v for k, v in l1_flips.items() if v}
    gxk, gpk, _, _ = _disc_fp64_grads(O, sd, x, xr, kinks=[h > 0 for h in hip_maps], l1_signs=hip_l1)
    errs_k = {n: rel(p.grad, gpk[n]) for n, p in disc.named_parameters()}
    worst_k = max(errs_k.items(), key=lambda kv: kv[1])
    ex_k = rel(xf.grad, gxk)
    rep = dict(worst_parameter=list(worst), waveform=ex, hip_kink_flips_vs_fp64=flips, hip_l1_sign_flips_vs_fp64=l1_flips,
               worst_feature_map=fwd_err,
               kinked_worst_parameter=list(worst_k), kinked_waveform=ex_k, first_conv_conditioning=cond,
               top5=sorted(errs.items(), key=lambda kv: -kv[1])[:5])
    _record(f"discriminator_fp64_T{T}", rep)
    print(f"[disc fp64 T={T}] {rep}")
    bar_p, bar_x = DISC_FP64_BARS[T]
    bar_pk, bar_xk = DISC_KINKED_BARS[T]
    assert ex_k < bar_xk and worst_k[1] < bar_pk, (ex_k, worst_k)
    assert ex < bar_x and worst[1] < bar_p, (ex, worst)


def test_full_train_step_runs(cuda):
    """train.py:265-374 minus the predictor losses: discriminator step + generator step on a small batch; finite losses,
    every model key's parameters move."""
    from facodec_amd.commons import build_model, default_model_params
    from facodec_amd.train import TrainStep
    model = build_model(default_model_params())
    for k in ("encoder", "quantizer", "decoder", "discriminator"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].to(cuda)
    step = TrainStep(model)
    before = {k: step.opt[k].p.clone() for k in step.opt}
    wave = synth.synth_clips(2, 12000, seed=3).to(cuda)
    out = step(wave)
    for k in ("loss", "loss_d", "loss_g", "feature", "mel", "commitment"):
        assert torch.isfinite(out[k]).all(), k
    for k in step.opt:
        assert torch.isfinite(step.opt[k].p).all() and not torch.equal(step.opt[k].p, before[k]), k
        assert float(out["grad_norm"][k]) > 0


def test_cross_entropy_and_smooth_l1_against_torch(cuda):
    from facodec_amd import autograd_disc as AD
    g = _g(61)
    logits = torch.randn(37, 1024, generator=g, requires_grad=True)
    labels = torch.randint(0, 1024, (37,), generator=g)
    ref = torch.nn.functional.cross_entropy(logits, labels)
    (2.0 * ref).backward()
    lg = logits.detach().to(cuda).requires_grad_()
    got = AD.CrossEntropy.apply(lg, labels.to(cuda))
    (2.0 * got).backward()
    assert abs(float(got.detach()) - float(ref.detach())) < 1e-5 and rel(lg.grad, logits.grad) < 1e-5
    a = (3 * torch.randn(5, 40, generator=g)).requires_grad_()
    b = torch.randn(5, 40, generator=g)
    r2 = torch.nn.functional.smooth_l1_loss(b, a)
    r2.backward()
    ag = a.detach().to(cuda).requires_grad_()
    g2 = AD.PairMean.apply(ag, b.to(cuda), 3)
    g2.backward()
    assert abs(float(g2.detach()) - float(r2.detach())) < 1e-6 and rel(ag.grad, a.grad) < 1e-5


def test_full_train_step_with_predictor_targets(cuda):
    """The complete loss of train.py:357-358 with caller-supplied predictor targets: runs, finite, all five optimisers step."""
    from facodec_amd.commons import build_model, default_model_params
    from facodec_amd.train import TrainStep
    model = build_model(default_model_params())
    for k in model:
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].to(cuda)
    step = TrainStep(model, with_predictors=True)
    B, T = 2, 12000
    F_ = T // 300
    g = _g(71)
    targets = dict(f0=torch.randn(B, F_, generator=g).to(cuda), uv=torch.randn(B, F_, generator=g).to(cuda),
                   phones=torch.randint(0, 1024, (B, F_), generator=g).to(cuda), speaker=torch.randint(0, 20000, (B,), generator=g).to(cuda))
    before = step.opt["fa_predictors"].p.clone()
    out = step(synth.synth_clips(B, T, seed=3).to(cuda), targets=targets)
    assert torch.isfinite(out["loss"]).all() and float(out["grad_norm"]["fa_predictors"]) > 0
    assert not torch.equal(step.opt["fa_predictors"].p, before)


def test_graphed_codec_matches_eager(full_model, cuda):
    """facodec_amd/graphs.py: the whole encoder -> quantizer -> decoder step replayed from one HIP graph gives bit-identical
    codes and waveform to the eagerly launched step, for fresh inputs copied into the captured buffer."""
    from facodec_amd.graphs import GraphedCodec
    m = full_model
    g = GraphedCodec(m, 2, 12000)
    for seed in (3, 4):
        wave = synth.synth_clips(2, 12000, seed=seed).to(cuda)
        out = g(wave)
        with torch.no_grad():
            z = m.encoder(wave)
            outs, _, _, _, timbre, codes = m.quantizer(z, wave, n_c=2, return_codes=True)
            y = m.decoder(outs)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out["codes"], codes))
        assert torch.equal(out["wave"], y) and torch.equal(out["timbre"], timbre)
    with pytest.raises(ValueError):
        g(torch.zeros(1, 1, 12000, device=cuda))
