"""The two-wide Snake (common.h: sin_sq2 / snake_apply2) of the all-waves epilogue of conv1d_bsplit_kernel.

Every packed operation is the IEEE operation of the scalar form on the same operands, and the per-row constants (EpiRow) are the
same loads and the same true division, only fewer of them.  So a launch with the fused Snake must give, bit for bit, what the same
launch without it gives when the stand-alone scalar kernel (ops.snake, misc.hip) is applied afterwards (the split GEMM kernel, whose
epilogue keeps the scalar form, is held to the same identity):

    c  = conv + bias                         (the launch without alpha_out, residual and second output)
    y  = snake(c, alpha_out) + res           (ops.snake, then one fp32 add: torch's add is the kernel's add)
    y2 = snake(y, alpha_y2)

Inputs: Gaussian activations and weights scaled so that the pre-activations have a standard deviation of about 0.05 (|alpha x| < 10 for
nearly all of them at alpha = 37); alpha cycles through 1e-3, 1, 37 over the channels (the second output's alpha is the same cycle,
shifted).  Input channel 0 is a plant channel: zero except at a few samples of 5e6, with a weight of exactly 1 on the tap that reads
the output's own column and 0 elsewhere, so single outputs of every row land beyond |alpha x| = 4096 (sin_sq_slow) for every alpha:
in the first component only of an aligned pair, in the second only, in both, and in the last column of the signal (at T % 4 = 1 the
only valid one of its quad).

The CPU test compiles the converted translation units to assembly and holds each converted kernel to at least one v_pk_fma_f32 and
to no scratch memory."""
import functools
import os
import re
import shutil
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

ALPHAS = (1e-3, 1.0, 37.0)
PLANT = 5e6
K64 = "64x256 (bf16x3"
K96 = "96x256 (bf16x3"

# name: (kernel name fragment, B, C_in, C_out, T, K, dilation, tile rows)
CONV_CASES = {
    "k7_rows64_d1": ("conv1d_bsplit_kernel<7> " + K64, 2, 64, 64, 333, 7, 1, 64),
    "k7_rows64_d9": ("conv1d_bsplit_kernel<7> " + K64, 2, 64, 64, 333, 7, 9, 64),
    "k7_rows64_cout96": ("conv1d_bsplit_kernel<7> " + K64, 2, 64, 96, 333, 7, 1, 64),
    "k7_rows96": ("conv1d_bsplit_kernel<7> " + K96, 3, 96, 96, 300, 7, 1, 96),
    "k3_rows64": ("conv1d_bsplit_kernel<3> " + K64, 2, 64, 64, 333, 3, 1, 64),
    "k5_rows64": ("conv1d_bsplit_kernel<5> " + K64, 2, 64, 64, 333, 5, 1, 64),
    "k7_tile_walk": ("conv1d_bsplit_kernel<7> " + K64, 8, 64, 64, 9000, 7, 1, 64),
    "gemm_k1": ("conv1d_gemm_split_kernel<1>", 2, 512, 128, 520, 1, 1, 0),
}
# (alpha_out, residual, second output)
VARIANTS = [(True, False, False), (True, True, False), (True, False, True), (True, True, True), (False, True, True)]


def _alpha(n, shift, dev):
    return torch.tensor([ALPHAS[(c + shift) % 3] for c in range(n)], dtype=torch.float32, device=dev)


def _plant_columns(T):
    """First component of a pair, second component, both, and the signal's last column."""
    return sorted({10, 21, 40, 41, 264, 267, T - 1})


class _Spy:
    def __enter__(self):
        from facodec_amd import ops
        self.ops, self.orig, self.launched = ops, ops._launch_conv, []

        def spy(d, what):
            self.launched.append(self.ops.conv_variant(d)[1])
            self.orig(d, what)

        ops._launch_conv = spy
        return self

    def __exit__(self, *exc):
        self.ops._launch_conv = self.orig


@functools.lru_cache(maxsize=2)
def _conv_setup(name):
    """Inputs, packed weights and the reference's pre-activation c of one case, shared by its variants and never written again."""
    from facodec_amd import ops
    kern, B, ci, co, T, k, dil, rows = CONV_CASES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1234 + len(name))
    x = torch.randn(B, ci, T, generator=g)
    w = torch.randn(co, ci, k, generator=g) * (0.05 / (ci * k) ** 0.5)
    x[:, 0, :] = 0.0
    w[:, 0, :] = 0.0
    w[:, 0, k - 1] = 1.0              # causal padding: the last tap reads the output's own column
    for t in _plant_columns(T):
        x[:, 0, t] = PLANT
    bias = torch.randn(co, generator=g) * 0.02
    res = torch.randn(B, co, T, generator=g)
    x, w, bias, res = x.to(dev), w.to(dev), bias.to(dev), res.to(dev)
    ws = ops.pack_conv_weight_split(w, rows=rows) if k > 2 else ops.pack_gemm_weight_split(w)
    with _Spy() as spy:
        c = ops.conv1d(x, None, co, k, bias=bias, dilation=dil, w_split=ws)
    torch.cuda.synchronize()
    assert len(spy.launched) == 1 and kern in spy.launched[0], spy.launched
    assert c.shape == (B, co, T)
    big = (c.abs() > 4096.0 / ALPHAS[0])
    assert int(big.sum()) == B * co * len(_plant_columns(T)), "the plants are single outputs"
    assert float((c.abs() * 37.0 < 10.0).float().mean()) > 0.97
    return dict(x=x, ws=ws, bias=bias, res=res, c=c, a1=_alpha(co, 0, dev), a2=_alpha(co, 1, dev))


def _check(got_y, got_y2, c, a1, a2, res, aout, has_res, has_y2):
    from facodec_amd import ops
    y = ops.snake(c, a1) if aout else c
    if has_res:
        y = y + res
    assert torch.equal(got_y, y), f"y: {int((got_y != y).sum())} of {y.numel()} elements differ"
    if has_y2:
        y2 = ops.snake(y, a2)
        assert torch.equal(got_y2, y2), f"y2: {int((got_y2 != y2).sum())} of {y2.numel()} elements differ"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_fused_snake_is_the_standalone_snake_bit_for_bit(name, cuda):
    from facodec_amd import ops
    kern, B, ci, co, T, k, dil, rows = CONV_CASES[name]
    s = _conv_setup(name)
    for aout, has_res, has_y2 in VARIANTS:
        with _Spy() as spy:
            got = ops.conv1d(s["x"], None, co, k, bias=s["bias"], dilation=dil, w_split=s["ws"], alpha_out=s["a1"] if aout else None,
                             res=s["res"] if has_res else None, alpha_y2=s["a2"] if has_y2 else None)
        assert len(spy.launched) == 1 and kern in spy.launched[0], spy.launched
        y, y2 = got if has_y2 else (got, None)
        _check(y, y2, s["c"], s["a1"], s["a2"], s["res"], aout, has_res, has_y2)


@pytest.mark.gpu
def test_transposed_conv_second_output_is_the_standalone_snake_bit_for_bit(cuda):
    """K = 2 through the stride-2 transposed conv on the split GEMM kernel: (channel, phase) rows, interleaved by the epilogue."""
    from facodec_amd import ops
    B, ci, co, T, stride = 4, 64, 32, 260, 2
    dev = cuda
    g = torch.Generator().manual_seed(77)
    x = torch.randn(B, ci, T, generator=g)
    w = torch.randn(ci, co, 2 * stride, generator=g) * (0.05 / (2 * ci) ** 0.5)
    # y[., 2 t + p] = W[p] x[t] + W[p + 2] x[t - 1].  Plant channels: 0 -> the even column, 1 -> the odd column, 2 -> both
    x[:, :3, :] = 0.0
    w[:3] = 0.0
    w[0, :, 0] = 1.0
    w[1, :, 1] = 1.0
    w[2, :, 0] = 1.0
    w[2, :, 1] = 1.0
    x[:, 0, 5] = PLANT
    x[:, 1, 17] = PLANT
    x[:, 2, 33] = PLANT
    x[:, 2, 140] = PLANT
    x[:, 1, T - 1] = PLANT          # the signal's last column
    bias = (torch.randn(co, generator=g) * 0.02).to(dev)
    x, w = x.to(dev), w.to(dev)
    a2 = _alpha(co, 1, dev)
    packs = ops.pack_convtr_weight_rows_split(w, None, stride)
    with _Spy() as spy:
        c = ops.conv_transpose1d(x, packs, co, stride, bias=bias)
        y, y2 = ops.conv_transpose1d(x, packs, co, stride, bias=bias, alpha_y2=a2)
    torch.cuda.synchronize()
    assert len(spy.launched) == 2 and all("conv1d_gemm_split_kernel<2>" in n for n in spy.launched), spy.launched
    assert c.shape == (B, co, T * stride)
    assert int((c.abs() > 4096.0 / ALPHAS[0]).sum()) == B * co * 7
    assert torch.equal(y, c)
    ref = ops.snake(c, a2)
    assert torch.equal(y2, ref), f"y2: {int((y2 != ref).sum())} of {ref.numel()} elements differ"


CONVERTED = {"conv1d_bsplit.hip": "conv1d_bsplit_kernel", "conv1d_bsplit96.hip": "conv1d_bsplit_kernel"}


def _kernel_facts(asm_path):
    """{kernel symbol: (v_pk_fma_f32 in its body, v_pk_mul_f32, scratch bytes, spilled VGPRs)} from the assembly and its metadata."""
    text = open(asm_path).read()
    meta = {}
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = (int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)),
                      int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)))
    out = {}
    for name, (scratch, spills) in meta.items():
        body = text[text.index("\n" + name + ":"):text.index(".Lfunc_end", text.index("\n" + name + ":"))]
        out[name] = (len(re.findall(r"\bv_pk_fma_f32\b", body)), len(re.findall(r"\bv_pk_mul_f32\b", body)), scratch, spills)
    return out


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
@pytest.mark.parametrize("src", list(CONVERTED))
def test_converted_kernels_use_packed_fma_and_no_scratch(src):
    import check_inflight_regs as C
    facts = _kernel_facts(C.compile_to_asm(os.path.join(REPO, "facodec_amd", "csrc", src)))
    mine = {k: v for k, v in facts.items() if CONVERTED[src] in k}
    assert mine, sorted(facts)
    for name, (pk_fma, pk_mul, scratch, spills) in mine.items():
        assert pk_fma > 0 and pk_mul > 0, (name, pk_fma, pk_mul)
        assert scratch == 0 and spills == 0, (name, scratch, spills)
