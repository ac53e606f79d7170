"""The 96 x 256 form of the k = 7 split-bf16 kernel (facodec_amd/csrc/conv1d_bsplit96.hip): weights packed in co tiles of 96
(ops.pack_conv_weight_split(rows=96)), chosen by convplan.tile_rows for the channel counts in ops.BS_ROWS96.

Grade: the recipe and the bars of test_gpu_parity.py::test_split_bf16_conv_matches_fp32_grade (OP_TOL against the oracle for y and
y2, fp64 error <= 1.5 x the fp32-MFMA kernel's + 1e-7), on 96 / 192 channels, dilations 1 / 3 / 9, reflect and zero padding, with
residual and second output.  Column counts: 300 (a full column tile and a partial one); 40 (shorter than the dilation-9 halo of 54);
and one length at which a workgroup of a 256-CU device walks more than three tiles.  The split kernels only take launches of more
than 640 columns in all (fewer belong to the split-reduction kernel, which reads fp32 weights), so the 300-column cases run 3 clips
and the 40-column cases 17, the fewest that qualify; the long case runs 2.  In every case the profile must name the 96 x 256 kernel."""
import pytest
import torch

pytestmark = pytest.mark.gpu

OP_TOL = 1e-5                 # tests/test_gpu_parity.py
NAME96 = "96x256"


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _g(seed=0):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(scope="module")
def O():
    from oracle import facodec_oracle
    return facodec_oracle


@pytest.fixture(scope="module")
def ops(cuda):
    from facodec_amd import ops as _ops
    from facodec_amd import _lib
    _lib.load()
    return _ops


def _profiled(ops, fn):
    prof = ops.ConvLaunchProfile()
    ops.set_conv_profile(prof)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        ops.set_conv_profile(None)
    return out, list(prof.summary())


def _walk_T(C, B):
    """Columns per clip at which B clips x (C / 96) co tiles are a little over 3 tiles for each of 256 workgroups."""
    return 256 * (-(-3 * 256 // (B * (C // 96))) + 1) - 100


GRADE = ([(3, C, 300, d, mode) for C in (96, 192) for d in (1, 3, 9) for mode in ("reflect", "zero")]
         + [(17, C, 40, d, mode) for C in (96, 192) for d, mode in ((9, "reflect"), (9, "zero"), (3, "reflect"))]
         + [(2, 96, _walk_T(96, 2), 3, "reflect"), (2, 192, _walk_T(192, 2), 9, "zero")])


@pytest.mark.parametrize("B,C,T,d,mode", GRADE)
def test_rows96_conv_matches_fp32_grade(B, C, T, d, mode, O, ops, cuda):
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
    ws = ops.pack_conv_weight_split(w.to(cuda), gg.to(cuda), rows=96)
    xc = x.to(cuda)
    (y, y2), names = _profiled(ops, lambda: ops.conv1d(xc, None, C, 7, w_split=ws, **kw))
    assert names and all(NAME96 in n and "bsplit" in n for n in names), names
    wp = ops.pack_conv_weight(w.to(cuda), gg.to(cuda))
    yf, _ = ops.conv1d(xc, wp, C, 7, **kw)
    e_y, e_y2 = rel(y, y_ref), rel(y2, O.snake(y_ref, a2.view(1, -1, 1)))
    print("rows96 grade", (B, C, T, d, mode), "y", e_y, "y2", e_y2)
    assert e_y < OP_TOL and e_y2 < OP_TOL
    # plain conv against fp64
    y64 = torch.nn.functional.conv1d(torch.nn.functional.pad(x.double(), (6 * d, 0)), wn.double(), b.double(), dilation=d)
    kw0 = dict(bias=b.to(cuda), dilation=d, pad_left=6 * d, pad_mode=ops.PAD_ZERO, t_out=T)
    (y0, names) = _profiled(ops, lambda: ops.conv1d(xc, None, C, 7, w_split=ws, **kw0))
    assert names and all(NAME96 in n for n in names), names
    e_split = rel(y0, y64)
    e_fp32 = rel(ops.conv1d(xc, wp, C, 7, **kw0), y64)
    print("rows96 fp64", (B, C, T, d, mode), "split", e_split, "fp32", e_fp32)
    assert e_split < 1.5 * e_fp32 + 1e-7, (e_split, e_fp32)
    assert rel(y, yf) < OP_TOL


def test_rows96_takes_p8_input_bit_identically(ops, cuda):
    """The property of test_split_conv_takes_p8_input_bit_identically on the new tile: planes from fac_to_p8 in, same bits out."""
    B, C, T, d = 3, 96, 300, 3
    g = _g(90 + C)
    x = torch.randn(B, C, T, generator=g).to(cuda)
    w = (torch.randn(C, C, 7, generator=g) / (C * 7) ** 0.5).to(cuda)
    bias = torch.randn(C, generator=g).to(cuda)
    al = (1 + 0.3 * torch.rand(C, generator=g)).to(cuda)
    ws = ops.pack_conv_weight_split(w, rows=96)
    p8 = ops.to_p8(x)
    assert torch.equal(p8.to_float(), x)
    y_ref, n1 = _profiled(ops, lambda: ops.conv1d(x, None, C, 7, bias=bias, dilation=d, alpha_out=al, pad_mode=ops.PAD_REFLECT, w_split=ws))
    y_p8, n2 = _profiled(ops, lambda: ops.conv1d(p8, None, C, 7, bias=bias, dilation=d, alpha_out=al, pad_mode=ops.PAD_REFLECT, w_split=ws))
    assert all(NAME96 in n for n in n1 + n2) and n1 and n2, (n1, n2)
    assert torch.equal(y_p8, y_ref)


@pytest.mark.parametrize("row", [0, 31, 32, 63, 64, 95])
def test_rows96_output_row_comes_from_its_own_weight_row(row, ops, cuda):
    """C_out = 96, weights zero except one output row: the output is zero except that row (a wrong co index in the pack or in the
    epilogue at a seam of the 32-row MFMA blocks moves it)."""
    C, T = 96, 700
    g = _g(row)
    x = torch.randn(1, C, T, generator=g).to(cuda)
    w = torch.zeros(C, C, 7)
    w[row] = torch.randn(C, 7, generator=g) / (C * 7) ** 0.5
    w = w.to(cuda)
    ws = ops.pack_conv_weight_split(w, rows=96)
    y, names = _profiled(ops, lambda: ops.conv1d(x, None, C, 7, dilation=3, pad_mode=ops.PAD_ZERO, w_split=ws))
    assert names and all(NAME96 in n for n in names), names
    ref = torch.nn.functional.conv1d(torch.nn.functional.pad(x.double().cpu(), (18, 0)), w.double().cpu(), dilation=3)
    others = [i for i in range(C) if i != row]
    assert float(y[0, others].abs().max()) == 0.0
    assert float(y[0, row].abs().max()) > 0.0 and rel(y[0, row], ref[0, row]) < OP_TOL


def test_switch_names_the_64_row_form(ops, cuda, monkeypatch):
    """ops.BS_ROWS96 is the switch: with the list empty the planner names the 64-row form, the pack follows it, and the two forms
    agree within OP_TOL."""
    from facodec_amd import convplan
    assert ops.BS_ROWS96 == (96,)
    B, C, T, d = 3, 96, 300, 9
    g = _g(5)
    x = torch.randn(B, C, T, generator=g).to(cuda)
    w = (torch.randn(C, C, 7, generator=g) / (C * 7) ** 0.5).to(cuda)
    bias = torch.randn(C, generator=g).to(cuda)
    monkeypatch.setattr(ops, "BS_ROWS96", (96,))
    assert convplan.tile_rows(C, C, 7) == 96 and convplan.tile_rows(C, C, 7, grad=True) == 64 and convplan.tile_rows(C, C, 5) == 64
    y96, n96 = _profiled(ops, lambda: ops.conv1d(x, None, C, 7, bias=bias, dilation=d, w_split=ops.pack_conv_weight_split(w)))
    monkeypatch.setattr(ops, "BS_ROWS96", ())
    assert convplan.tile_rows(C, C, 7) == 64
    y64, n64 = _profiled(ops, lambda: ops.conv1d(x, None, C, 7, bias=bias, dilation=d, w_split=ops.pack_conv_weight_split(w)))
    assert all(NAME96 in n for n in n96) and all("64x256" in n for n in n64) and n96 and n64, (n96, n64)
    assert rel(y96, y64) < OP_TOL


def test_rows96_weights_are_refused_outside_the_kernels_shapes(ops, cuda):
    """Weights packed for the 96-row tile fit no other kernel: a launch the form does not take is an error, not a fallback."""
    from facodec_amd import _lib
    x = torch.randn(1, 96, 300, generator=_g(1)).to(cuda)          # 300 columns: below the split kernels' 640
    ws = ops.pack_conv_weight_split(torch.randn(96, 96, 7, generator=_g(2)).to(cuda), rows=96)
    with pytest.raises(_lib.FacodecHipError):
        ops.conv1d(x, None, 96, 7, w_split=ws)
    with pytest.raises(_lib.FacodecHipError):
        ops.pack_conv_weight_split(torch.randn(96, 96, 5, generator=_g(3)).to(cuda), rows=96)
