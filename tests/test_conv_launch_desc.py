"""The descriptor a forward site launches against the one the CPU tests build for it (tests/test_conv_plan_cpu.py: launch_desc).

Every forward site of tests/golden/conv_plan_table.json is run once through its real entry point, at the smallest shape that reaches
it, with ops._launch_conv replaced by a spy; each launched descriptor must agree with launch_desc(site, args) in every non-pointer
field and in which pointers are null (assert_same_launch).  The builders do not depend on the route, so the fp32 routes are enough:
two clips, 16 - 64 channels, a few dozen to a few hundred columns.  The one exception is the flattened SConv1d form, which exists on
the split GEMM route only: FLAT, below, is the smallest shape convplan admits to it.  The data-gradient sites are compared the same
way by tests/test_conv_bwd_data.py on its own table.
"""
import pytest
import torch

from facodec_amd import convplan, ops
from test_conv_plan_cpu import assert_same_launch, launch_desc, plan

gpu = pytest.mark.gpu
Y2 = ("y2", "alpha_y2")

# (c_out, c_in, k, stride, dilation, B, T, alpha_in, plain, res, causal_reflect, grad) of layers.SConv1d.run, flattened: a k = 2 s
# strided conv needs 32 input and 64 output channels, fewer than 256 outputs per clip and 1024 columns in all, B (T / s + 1) - 1:
# five clips of 204 outputs.  Four clips, or 203 outputs each, stay per clip (test_flat_case_is_the_smallest_the_planner_admits).
FLAT = (64, 32, 4, 2, 1, 5, 408, False, True, False, True, False)


def test_flat_case_is_the_smallest_the_planner_admits():
    site = "layers.SConv1d.run"
    assert plan(site, FLAT)[:2] == [convplan.W_GEMM_STRIDED, convplan.FLAT_STRIDED]
    co, ci, k, s, d, B, T = FLAT[:7]
    for smaller in ((co, ci, k, s, d, B - 1, T), (co, ci, k, s, d, B, T - s), (co // 2, ci, k, s, d, B, T), (co, ci // 2, k, s, d, B, T)):
        assert plan(site, smaller + FLAT[7:])[1] == convplan.PER_CLIP, smaller
    d_ = launch_desc(site, FLAT)
    assert (d_.B, d_.T_in, d_.T_out) == (1, 5 * 410, 5 * 205 - 1)


class _Spy:
    """Keeps the descriptor of every conv launch."""

    def __enter__(self):
        self.launched, self.orig = [], ops._launch_conv

        def spy(d, what):
            self.orig(d, what)
            self.launched.append(d)

        ops._launch_conv = spy
        return self

    def __exit__(self, *exc):
        ops._launch_conv = self.orig
        return False


def _rand(cuda, *shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(cuda)


def _check(cuda, run, *want):
    """run() launches exactly the convs want = (site, args, operands) ..., in that order."""
    with _Spy() as spy:
        run()
        torch.cuda.synchronize()
    assert len(spy.launched) == len(want), [ops.conv_variant(d)[1] for d in spy.launched]
    for d, (site, a, operands) in zip(spy.launched, want):
        assert ops.conv_variant(d)[0] >= 0
        assert_same_launch(d, launch_desc(site, a, operands), (site, a))


# (args, operands, what run() gets beyond x) of layers.SConv1d.run
SCONV = {
    "causal_res_y2": ((32, 32, 7, 1, 3, 2, 100, False, False, True, True, False), ("bias", "res") + Y2, ("res", "alpha_y2")),
    "causal_k1_res_y2": ((32, 32, 1, 1, 1, 2, 100, False, False, True, True, False), ("bias", "res") + Y2, ("res", "alpha_y2")),
    "noncausal": ((48, 16, 5, 1, 1, 2, 90, False, True, False, False, False), ("bias",), ()),
    "strided": ((32, 16, 4, 2, 1, 2, 101, False, True, False, True, False), ("bias",), ()),
    "flat": (FLAT, ("bias",), ()),
}


@gpu
@pytest.mark.parametrize("name", list(SCONV))
def test_sconv1d_run_launches_the_built_descriptor(name, cuda):
    from facodec_amd.layers import SConv1d
    a, operands, extra = SCONV[name]
    co, ci, k, s, d, B, T, _, _, _, cr, _ = a
    m = SConv1d(ci, co, k, stride=s, dilation=d, causal=cr, norm="weight_norm").to(cuda)
    x = _rand(cuda, B, ci, T)
    kw = {}
    if "res" in extra:
        kw["res"] = _rand(cuda, B, co, T, seed=1)
    if "alpha_y2" in extra:
        kw["alpha_y2"] = torch.ones(co, device=cuda)
    with torch.no_grad():
        _check(cuda, lambda: m.run(x, **kw), ("layers.SConv1d.run", a, operands))


# (c_in, c_out, stride, B, T, causal, alpha_in, grad) of layers.SConvTranspose1d.run: polyphase causal and non-causal (phase_shift),
# and the all-phases rows form on the split GEMM kernel at its floor of 64 input channels, 256 columns per clip and 1024 in all
CONVTR = {
    "polyphase": ((32, 16, 4, 2, 50, True, False, False), convplan.TR_POLYPHASE),
    "polyphase_noncausal": ((32, 16, 5, 2, 40, False, False, False), convplan.TR_POLYPHASE),
    "rows_split": ((64, 32, 2, 2, 512, True, False, False), convplan.TR_ROWS_SPLIT),
}


@gpu
@pytest.mark.parametrize("name", list(CONVTR))
def test_sconvtranspose1d_run_launches_the_built_descriptor(name, cuda):
    from facodec_amd.layers import SConvTranspose1d
    a, layout = CONVTR[name]
    ci, co, s, B, T, causal = a[:6]
    assert plan("layers.SConvTranspose1d.run", a)[0] == layout
    m = SConvTranspose1d(ci, co, 2 * s, stride=s, causal=causal, norm="weight_norm").to(cuda)
    x = _rand(cuda, B, ci, T)
    with torch.no_grad():
        _check(cuda, lambda: m.run(x, alpha_y2=torch.ones(co, device=cuda)), ("layers.SConvTranspose1d.run", a, ("bias",) + Y2))


@gpu
def test_plain_conv_run_launches_the_built_descriptor(cuda):
    from facodec_amd.quantize import _PlainConv
    co, ci, k, B, T = a = (24, 16, 5, 2, 64)
    m = _PlainConv(ci, co, k).to(cuda)
    x = _rand(cuda, B, ci, T)
    with torch.no_grad():
        _check(cuda, lambda: m.run(x, pad=(k - 1) // 2), ("quantize._PlainConv.run", a, None))


@gpu
def test_training_forwards_launch_the_built_descriptors(cuda):
    """autograd._Conv.forward, _ResUnit.forward (its two convs) and _ConvTr.forward."""
    from facodec_amd import autograd as A
    from facodec_amd.layers import SConv1d, SConvTranspose1d
    B, C, T = 2, 32, 100
    conv = SConv1d(16, C, 7, dilation=3, causal=True, norm="weight_norm").to(cuda)
    _check(cuda, lambda: A.conv(conv, _rand(cuda, B, 16, T)), ("autograd._Conv.forward", (C, 16, 7, 1, 3, B, T, True, True), None))
    down = SConv1d(16, C, 4, stride=2, causal=True, norm="weight_norm").to(cuda)
    _check(cuda, lambda: A.conv(down, _rand(cuda, B, 16, T + 1), act=ops.ACT_TANH),
           ("autograd._Conv.forward", (C, 16, 4, 2, 1, B, T + 1, False, True), None))
    k7 = SConv1d(C, C, 7, dilation=3, causal=True, norm="weight_norm").to(cuda)
    k1 = SConv1d(C, C, 1, causal=True, norm="weight_norm").to(cuda)
    ones = torch.ones(1, C, 1, device=cuda)
    x, xa = _rand(cuda, B, C, T), _rand(cuda, B, C, T, seed=1)
    _check(cuda, lambda: A._ResUnit.apply(x, xa, k7.w.weight_v, k7.w.weight_g, k7.w.bias, ones, k1.w.weight_v, k1.w.weight_g, k1.w.bias,
                                          ones, (3, k7.pad_mode, True)),
           ("autograd._ResUnit.forward", (C, C, 7, 3, B, T), None), ("autograd._ResUnit.forward", (C, C, 1, 1, B, T), None))
    up = SConvTranspose1d(C, 16, 8, stride=4, causal=True, norm="weight_norm").to(cuda)
    _check(cuda, lambda: A.conv_tr(up, x), ("autograd._ConvTr.forward", (C, 16, 4, B, T, True), None))


@gpu
def test_disc_plain_conv_forward_launches_the_built_descriptor(cuda):
    """autograd_disc.PlainConv.forward with two-level taps: a (3, 3) kernel over rows of pitch 20, stride 2."""
    from facodec_amd import autograd_disc as D
    co, ci, k, k1, s, B, t_in, pad, dil2 = 16, 16, 9, 3, 2, 2, 200, 21, 20
    t_out = (t_in + 2 * pad - D.tap_span(k, k1, dil2) - 1) // s + 1
    v, g, bias = _rand(cuda, co, ci, k), torch.ones(co, 1, 1, device=cuda), torch.zeros(co, device=cuda)
    x = _rand(cuda, B, ci, t_in, seed=1)
    _check(cuda, lambda: D.PlainConv.apply(x, v, g, bias, k, s, pad, (k1, dil2)),
           ("autograd_disc.PlainConv.forward", (co, ci, k, k1, s, B, t_in, t_out, pad, dil2), None))
