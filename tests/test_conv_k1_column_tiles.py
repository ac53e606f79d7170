"""The k = 1 convs of the style path at the frame rate -- 1025 -> 80 (log-mel), 80 -> 512 (+ Mish), 20 -> 256 -- on five 128 x 32
column tiles per clip instead of one 128 x 160 tile (conv1d_api.hip: select_variant; ops.K1_COLUMN_TILES = False keeps the wide tile).

The route covers 129 .. 160 columns per clip, so the T values sit on its tile edges: 160 (five full tiles), 159 (one column below
the fifth tile's end), 129 (one column above the fourth tile), 145 (a ragged last tile).  B = 5 reaches the tiles (800 columns);
B = 2 is 320 columns, which the split reduction (skinny) takes whatever the switch says: its name and bits must not move.

The bar is the forward conv tests' (tests/test_conv_fwd_epilogue.py), restated:
  step A, the sum, launched with the bias only:  |c_gpu - c64| <= 4 sqrt(n) 2^-24 mag + 4 * 2^-24 |c64| at every element, n = C_in,
          mag = the same conv over |w| and |x| plus |bias|, c64 float64 from the same fp32 inputs;
  step B, the activation as a map of the kernel's own pre-activation: |y_gpu - act64(c_gpu)| <= 4 e_cpu s + 4 ulp |r64|, s the
          per-channel max |r64|, e_cpu the worst error of the same map in fp32 on the CPU in units of s.
And the new form's worst step-A error is at most 1.5 x the wide tile's on the same inputs, measured here by forcing the wide tile."""
import ctypes
import math

import pytest
import torch

from facodec_amd import ops

gpu = pytest.mark.gpu
EPS32, ULP, CANARY = 2.0 ** -24, 2.0 ** -23, 12345.0
# name, C_in, C_out, act, bias, non-negative operands (power spectrum x mel basis)
SHAPES = [("log_mel", 1025, 80, ops.ACT_LOG_MEL, False, True), ("mish", 80, 512, ops.ACT_MISH, True, False),
          ("plain", 20, 256, ops.ACT_NONE, True, False)]
TS = (160, 159, 129, 145)
BS = (2, 5)
PARAMS = [(s, B, T) for s in SHAPES for B in BS for T in TS]


def _desc(B, ci, co, T, act=ops.ACT_NONE, k=1):
    d = ops.conv_desc(B, ci, T, co, k, pad_left=0 if k == 1 else None, pad_mode=ops.PAD_ZERO, t_out=T if k == 1 else None, act=act)
    fake = ctypes.c_void_p(0x10000)                 # never dereferenced: fac_conv1d_variant only reads the descriptor
    d.x = d.y = d.w = d.ws = fake
    d.ws_bytes = ops.CONV_WS_BYTES
    return d


def _name(*a, tiles=True, **k):
    old = ops.K1_COLUMN_TILES
    ops.K1_COLUMN_TILES = tiles
    try:
        return ops.conv_variant(_desc(*a, **k))[1]
    finally:
        ops.K1_COLUMN_TILES = old


def _want(B, T):
    """The kernel the planner must name with the switch on / off."""
    if B * T <= 640:
        return "skinny", "skinny"
    return "128x32", "128x160"


def test_planner_names():
    for (_, ci, co, act, _, _), B, T in PARAMS:
        on, off = _want(B, T)
        assert on in _name(B, ci, co, T, act) and off in _name(B, ci, co, T, act, tiles=False), (ci, co, B, T)
    for _, ci, co, act, _, _ in SHAPES:
        assert "128x32" in _name(32, ci, co, 160, act) and "128x160" in _name(32, ci, co, 160, act, tiles=False)   # the benchmark's launches
        for T in (128, 161, 324):                                       # outside 129 .. 160 columns nothing moves
            assert _name(5, ci, co, T, act) == _name(5, ci, co, T, act, tiles=False) and "128x32" not in _name(5, ci, co, T, act)
    # wide tiles that fill 256 workgroups stay: 64 clips x 4 co tiles, against 63 x 4
    assert "128x160" in _name(64, 80, 512, 160) and "128x32" in _name(63, 80, 512, 160)
    assert "128x160" in _name(5, 24, 72, 132, k=3)                      # taps keep the wide tile (the halo would be staged five times)


def _act(c, act):
    if act == ops.ACT_MISH:
        sp = torch.where(c > 20, c, torch.log1p(torch.exp(c)))          # softplus with torch's threshold 20
        return c * torch.tanh(sp)
    if act == ops.ACT_LOG_MEL:
        return (torch.log(1e-5 + c) + 4.0) / 4.0
    return c


def _run(x_d, w_packed, co, bias_d, act, T, tiles):
    """ops.conv1d into a canary-wrapped output with the switch set -> (output on the host, kernel name)."""
    B = x_d.shape[0]
    n, pad = B * co * T, 64
    buf = torch.full((n + 2 * pad,), CANARY, device=x_d.device)
    out = buf[pad:pad + n].view(B, co, T)
    old = ops.K1_COLUMN_TILES
    ops.K1_COLUMN_TILES = tiles
    try:
        y = ops.conv1d(x_d, w_packed, co, 1, bias=bias_d, pad_left=0, pad_mode=ops.PAD_ZERO, t_out=T, act=act, out=out)
    finally:
        ops.K1_COLUMN_TILES = old
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    c = buf.cpu()
    assert bool((c[:pad] == CANARY).all()) and bool((c[-pad:] == CANARY).all()), "canary overwritten"
    got = c[pad:pad + n].view(B, co, T)
    assert not bool((got == CANARY).any())
    return got


@gpu
@pytest.mark.parametrize("shape,B,T", PARAMS, ids=[f"{s[0]}_{s[1]}to{s[2]}_B{B}_T{T}" for s, B, T in PARAMS])
def test_column_tiles_fp64(cuda, shape, B, T):
    name, ci, co, act, has_bias, nonneg = shape
    g = torch.Generator().manual_seed(ci + 7 * T + B)
    x = torch.randn(B, ci, T, generator=g)
    w = torch.randn(co, ci, 1, generator=g) / math.sqrt(ci)
    if nonneg:
        x, w = x * x, w.abs()
    bias = torch.randn(co, generator=g) if has_bias else None
    x_d, w_p = x.to(cuda), ops.pack_conv_weight(w.to(cuda))
    b_d = bias.to(cuda) if has_bias else None
    # step A: the sum, on both forms
    c64 = torch.einsum("oc,bct->bot", w[:, :, 0].double(), x.double())
    mag = torch.einsum("oc,bct->bot", w[:, :, 0].double().abs(), x.double().abs())
    if has_bias:
        c64 = c64 + bias.double()[None, :, None]
        mag = mag + bias.double().abs()[None, :, None]
    bound = 4 * math.sqrt(ci) * EPS32 * mag + 4 * EPS32 * c64.abs()
    c_new, c_old = _run(x_d, w_p, co, b_d, ops.ACT_NONE, T, True), _run(x_d, w_p, co, b_d, ops.ACT_NONE, T, False)
    assert torch.equal(x_d.cpu(), x)
    e_new, e_old = (c_new.double() - c64).abs(), (c_old.double() - c64).abs()
    ratio = float((e_new / bound.clamp_min(1e-300)).max())
    print(f"[tol] k1_column_tiles_{name}_B{B}_T{T}: error / bound {ratio:.3e} (wide tile {float((e_old / bound.clamp_min(1e-300)).max()):.3e}); "
          f"max error {float(e_new.max()):.3e} against the wide tile's {float(e_old.max()):.3e}")
    assert bool(torch.isfinite(c_new).all()) and ratio <= 1.0, (name, B, T, ratio)
    assert float(e_new.max()) <= 1.5 * float(e_old.max()), (name, B, T, float(e_new.max()), float(e_old.max()))
    if B * T <= 640:
        assert torch.equal(c_new, c_old)            # the split reduction either way
    # step B: the activation as a map of the kernel's own pre-activation
    if act != ops.ACT_NONE:
        y = _run(x_d, w_p, co, b_d, act, T, True)
        r64, r32 = _act(c_new.double(), act), _act(c_new, act).double()
        s = r64.abs().amax(dim=(0, 2), keepdim=True).clamp_min(1e-300)
        e_cpu = float(((r32 - r64).abs() / s).max())
        err = (y.double() - r64).abs()
        print(f"[tol] k1_column_tiles_{name}_act_B{B}_T{T}: gpu {float((err / s).max()):.3e} fp32-cpu {e_cpu:.3e}")
        assert bool(torch.isfinite(y).all())
        assert float((err - (4.0 * e_cpu * s + 4 * ULP * r64.abs())).max()) <= 0.0, (name, B, T)
