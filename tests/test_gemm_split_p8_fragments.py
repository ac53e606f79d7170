"""The P8-fragment form of the split GEMM (conv1d_gemm_split_p8.hip: 64 x 256 / 64 x 128 tiles, input fragments straight from the
P8 planes, two workgroups per CU) against the 128 x 128 form of conv1d_gemm_split.hip forced through fac_conv_desc.gsplit_p8_cols.

Both forms read the same planes (ops.to_p8) and the same packed weights and run the same products in the same order, so every
comparison is torch.equal on y and y2: the 128 x 128 form is pinned to fp64 and to its fp32-input path by the existing tests
(test_conv_fwd_epilogue, test_convtr_fwd, test_gpu_parity), so equality is the whole proof.  Shapes: the smallest at which each
mechanism of the new form can go wrong (ragged last chunk, ragged 64-row tile, the odd half of a 128-row pack tile, clip boundaries
inside a tile, T % 4 != 0, channels of a transposed conv that straddle the 64-row split, reflect and zero padding at both ends)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

COLS = (256, 128)


@pytest.fixture(scope="module")
def ops(cuda):
    from facodec_amd import ops
    return ops


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _run_form(ops, monkeypatch, cols, fn):
    """fn() with every P8 split GEMM launch on the form `cols` (-1: the 128 x 128 form); returns (fn's result, kernel names)."""
    monkeypatch.setattr(ops, "GSPLIT_P8_COLS", cols)
    prof = ops.ConvLaunchProfile()
    ops.set_conv_profile(prof)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        ops.set_conv_profile(None)
    return out, list(prof.summary())


def _same(ops, monkeypatch, cols, fn):
    """Runs fn on the 128 x 128 form and on the P8-fragment form with `cols` columns per tile; every tensor fn returns must be equal."""
    ref, ref_names = _run_form(ops, monkeypatch, -1, fn)
    got, got_names = _run_form(ops, monkeypatch, cols, fn)
    assert ref_names and all("conv1d_gemm_split_kernel<" in n and " 128x128 " in n for n in ref_names), ref_names
    assert got_names and all("conv1d_gemm_split_kernel<" in n and f" 64x{cols} " in n for n in got_names), got_names
    ref = ref if isinstance(ref, (tuple, list)) else (ref,)
    got = got if isinstance(got, (tuple, list)) else (got,)
    assert len(ref) == len(got)
    for i, (r, g) in enumerate(zip(ref, got)):
        assert (r is None) == (g is None), i
        if r is not None:
            assert r.shape == g.shape and torch.isfinite(r).all() and torch.equal(r, g), (i, (r - g).abs().max().item())


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("epi", ["plain", "all", "y2_only"])
def test_k1_flattened(ops, cuda, monkeypatch, cols, epi):
    """K = 1: B 3, C_in 72 (ragged last chunk), 136 rows (ragged 64-row tile, odd half of a pack tile), T 347 = 1041 flattened columns
    (T % 4 != 0, clip boundaries inside a tile, ragged last tile); with and without bias / alpha_out / res / y2, and y2 alone."""
    B, ci, co, T = 3, 72, 136, 347
    g = _g(1)
    x = torch.randn(B, ci, T, generator=g).to(cuda)
    ws = ops.pack_gemm_weight_split((torch.randn(co, ci, 1, generator=g) / ci ** 0.5).to(cuda))
    bias = torch.randn(co, generator=g).to(cuda)
    a_out = (0.5 + torch.rand(co, generator=g)).to(cuda)
    a2 = (0.5 + torch.rand(co, generator=g)).to(cuda)
    res = torch.randn(B, co, T, generator=g).to(cuda)
    p8 = ops.to_p8(x)
    kw = dict(pad_left=0, pad_mode=ops.PAD_ZERO, t_out=T, w_split=ws)
    if epi == "all":
        kw.update(bias=bias, alpha_out=a_out, res=res, alpha_y2=a2)
    elif epi == "y2_only":
        kw.update(bias=bias, alpha_y2=a2, want_y=False)
    _same(ops, monkeypatch, cols, lambda: ops.conv1d(p8, None, co, 1, **kw))


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("T_out,pad_left", [(259, 0), (259, 1), (515, 0), (515, 1)])
def test_k2_stride1(ops, cuda, monkeypatch, cols, T_out, pad_left):
    """K = 2, stride 1, per-clip tiles: B 4, C_in 64, C_out 72; the halo column on either side of the signal."""
    B, ci, co = 4, 64, 72
    T_in = T_out + 1 - pad_left
    g = _g(2 + T_out + pad_left)
    x = torch.randn(B, ci, T_in, generator=g).to(cuda)
    ws = ops.pack_gemm_weight_split((torch.randn(co, ci, 2, generator=g) / (2 * ci) ** 0.5).to(cuda))
    bias = torch.randn(co, generator=g).to(cuda)
    p8 = ops.to_p8(x)
    _same(ops, monkeypatch, cols, lambda: ops.conv1d(p8, None, co, 2, bias=bias, pad_left=pad_left, pad_mode=ops.PAD_ZERO, t_out=T_out,
                                                     w_split=ws))


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("layout", ["clips", "flat"])
@pytest.mark.parametrize("s", [2, 5, 6])
def test_transposed_row_phases(ops, cuda, monkeypatch, cols, layout, s):
    """All-phases ConvTranspose1d (row_phases 2 / 5 / 6), C_in 64, C_out 40 -- at rp 5 (25 channels per 128 rows) and rp 6 (21) a channel
    straddles the 64-row split of a pack tile -- over 4 clips of 257 columns and over the flattened layout of 9 clips x 129 columns,
    with alpha_y2."""
    ci, co = 64, 40
    g = _g(30 + s)
    B, T = (4, 257) if layout == "clips" else (1, 9 * 129)
    x = torch.randn(B, ci, T, generator=g).to(cuda)
    if layout == "flat":
        x.view(ci, 9, 129)[:, :, 0] = 0          # the zero column in front of every clip (ops.conv_transpose1d_flat)
    v = (torch.randn(ci, co, 2 * s, generator=g) / (2 * ci) ** 0.5).to(cuda)
    gn = (0.5 + torch.rand(ci, 1, 1, generator=g)).to(cuda)
    w = ops.pack_convtr_weight_rows_split(v, gn, s)
    bias = torch.randn(co, generator=g).to(cuda)
    a2 = (0.5 + torch.rand(co, generator=g)).to(cuda)
    p8 = ops.to_p8(x)
    _same(ops, monkeypatch, cols, lambda: ops.conv_transpose1d(p8, w, co, s, bias=bias, alpha_y2=a2))


STRIDED = [(4, 2, 32, 512), (4, 2, 72, 517), (10, 5, 32, 1290), (10, 5, 72, 1303), (12, 6, 32, 1542), (12, 6, 72, 1561)]


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("mode", ["reflect", "zero"])
@pytest.mark.parametrize("k,s,ci,T", STRIDED)
def test_strided(ops, cuda, monkeypatch, cols, mode, k, s, ci, T):
    """Strided convs as 2 taps over s phase sub-signals: k 4 s 2, k 10 s 5, k 12 s 6; C_in 32 and 72 (ragged chunk); reflect padding
    (causal, the right end reflected too when T % s != 0) and zero padding; T_out 256 .. 261, T % s zero and non-zero."""
    B, co = 4, 72
    g = _g(100 * k + ci)
    x = torch.randn(B, ci, T, generator=g).to(cuda)
    ws = ops.pack_gemm_weight_split((torch.randn(co, ci, k, generator=g) / (ci * k) ** 0.5).to(cuda), in_stride=s)
    bias = torch.randn(co, generator=g).to(cuda)
    kw = dict(bias=bias, stride=s, w_split=ws)
    if mode == "zero":
        kw.update(pad_left=k - s, pad_mode=ops.PAD_ZERO, t_out=T // s)
    p8 = ops.to_p8(x)
    y_shape = []

    def run():
        y = ops.conv1d(p8, None, co, k, **kw)
        y_shape.append(y.shape[-1])
        return y

    _same(ops, monkeypatch, cols, run)
    assert 256 <= y_shape[0] <= 261 and (T % s == 0) == (ci == 32)


def test_two_launches_back_to_back(ops, cuda, monkeypatch):
    """Two launches of different shapes (and different tile widths) on one stream, no synchronisation between them: nothing carries over."""
    g = _g(7)
    x1 = torch.randn(3, 72, 347, generator=g).to(cuda)
    w1 = ops.pack_gemm_weight_split((torch.randn(136, 72, 1, generator=g) / 72 ** 0.5).to(cuda))
    x2 = torch.randn(4, 64, 260, generator=g).to(cuda)
    w2 = ops.pack_gemm_weight_split((torch.randn(72, 64, 2, generator=g) / 128 ** 0.5).to(cuda))
    p1, p2 = ops.to_p8(x1), ops.to_p8(x2)

    def pair(c1, c2):
        monkeypatch.setattr(ops, "GSPLIT_P8_COLS", c1)
        y1 = ops.conv1d(p1, None, 136, 1, pad_left=0, pad_mode=ops.PAD_ZERO, t_out=347, w_split=w1)
        monkeypatch.setattr(ops, "GSPLIT_P8_COLS", c2)
        y2 = ops.conv1d(p2, None, 72, 2, pad_left=1, pad_mode=ops.PAD_ZERO, t_out=260, w_split=w2)
        monkeypatch.setattr(ops, "GSPLIT_P8_COLS", c1)
        y3 = ops.conv1d(p1, None, 136, 1, pad_left=0, pad_mode=ops.PAD_ZERO, t_out=347, w_split=w1)
        torch.cuda.synchronize()
        return y1, y2, y3

    ref = pair(-1, -1)
    for c1, c2 in ((256, 128), (128, 256)):
        got = pair(c1, c2)
        assert all(torch.equal(a, b) for a, b in zip(ref, got)), (c1, c2)


@pytest.mark.parametrize("cols", COLS)
def test_output_does_not_depend_on_what_the_buffers_held(ops, cuda, monkeypatch, cols):
    """The same launch into an output buffer of 0xFF bytes and into one of zeros: the same bits, every element written."""
    g = _g(9)
    x = torch.randn(4, 64, 257, generator=g).to(cuda)
    v = (torch.randn(64, 40, 10, generator=g) / 128 ** 0.5).to(cuda)
    w = ops.pack_convtr_weight_rows_split(v, None, 5)
    p8 = ops.to_p8(x)
    monkeypatch.setattr(ops, "GSPLIT_P8_COLS", cols)
    outs = []
    for fill in (0xFF, 0x00):
        out = torch.empty(4, 40, 257 * 5, dtype=torch.float32, device=cuda)
        out.view(torch.uint8).fill_(fill)
        ops.conv_transpose1d(p8, w, 40, 5, out=out)
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
