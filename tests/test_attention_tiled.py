"""The register-tiled form of fac_attention (csrc/attention_tiled.hip) against the serial kernel it replaces on the LDS route
(attention_kernel, csrc/misc.hip, reached through fac_attention_serial) and against float64 softmax attention.

The tiled kernel keeps every output's operations and their order, so the two kernels must agree bit for bit; the float64 bar is
the `maps` bar of test_attention_fused_fp64, restated here: |got - ref64| <= 4 e_cpu max|ref64| + 4 ulp |ref64| at every
element, e_cpu the worst error of the same formula evaluated in fp32 on the CPU, in units of max|ref64|.

T covers one key; below, at and above the 32 keys of one V pass (which is also one 32-query tile) and the 16-query tile of the
serial kernel; multiples of 32 and their neighbours; 160, the benchmark's frame count; 161 (rows that are not 16-byte aligned: the
scalar load path) and 192.  dk = 24 leaves most of the 256 rows of a V pass empty, dk = 256 fills them."""
import ctypes as C
import functools
import os

import pytest
import torch

from facodec_amd import _lib, ops

gpu = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -23
CANARY = 12345.0
B, H = 2, 2
DKS = (24, 256)
TS = (1, 15, 16, 17, 31, 32, 33, 160, 161, 192)
MASKS = ("mask_null", "partial_mask", "clip_fully_masked")
PARAMS = [(dk, T, m) for dk in DKS for T in TS for m in MASKS if T > 1 or m != "partial_mask"]     # one key: nothing to mask partly

# the tiled layout, restated from the shapes: at most 256 rows per head; one pass of V (256 rows x 36 floats) and 32 score rows of
# T rounded up to 32 keys in 160 KiB of LDS  =>  36864 + 128 * round32(T) <= 163840  =>  round32(T) <= 992
T_LAST_TILED, T_FIRST_SERIAL = 992, 993


def _tiled_fits(dk, T):
    return dk <= 256 and (256 * 36 + 32 * ((T + 31) // 32 * 32)) * 4 <= 160 * 1024


def _form(dk, T):
    if (16 * dk + 16 * T) * 4 > 160 * 1024:
        return "stream"
    return "tiled" if _tiled_fits(dk, T) else "serial"


def _attn_ref(q, k, v, mask, nb, dk, T):
    """softmax(q^T k / sqrt(dk)) v on (nb, H dk, T) tensors; a pair with mask[tq] * mask[tk] == 0 scores -1e4
    (modules/attentions.py:168-199)."""
    qh, kh, vh = (t.view(nb, H, dk, T).transpose(2, 3) for t in (q, k, v))
    sc = qh @ kh.transpose(2, 3) / dk ** 0.5
    if mask is not None:
        sc = sc.masked_fill((mask.unsqueeze(1) * mask.unsqueeze(2)).unsqueeze(1) == 0, -1e4)
    return (torch.softmax(sc, -1) @ vh).transpose(2, 3).reshape(nb, H * dk, T)


@functools.lru_cache(maxsize=None)
def _case(dk, T, mask_kind, nb=B):
    """Inputs and both references, computed once and shared (never written to): q, k, v (nb, H dk, T), mask (nb, T) or None --
    the last clip loses its last min(17, T // 2) frames, `clip_fully_masked` also zeroes clip 0's whole mask."""
    g = torch.Generator().manual_seed(1000 * dk + 7 * T + len(mask_kind))
    q, k, v = (torch.randn(nb, H * dk, T, generator=g) for _ in range(3))
    mask = None
    if mask_kind != "mask_null":
        mask = torch.ones(nb, T)
        mask[-1, T - min(17, T // 2):] = 0
        if mask_kind == "clip_fully_masked":
            mask[0] = 0
    o64 = _attn_ref(q.double(), k.double(), v.double(), None if mask is None else mask.double(), nb, dk, T)
    o32 = _attn_ref(q, k, v, mask, nb, dk, T)
    return q, k, v, mask, o64, o32


def _bar(name, got, ref64, ref32):
    """4 e_cpu + 4 ulp at every element, in units of the largest |ref64| (the bar of test_attention_fused_fp64)."""
    got, ref64, ref32 = (t.detach().double().cpu().reshape(-1) for t in (got, ref64, ref32))
    assert bool(torch.isfinite(got).all()), name
    s = ref64.abs().max().clamp_min(1e-300)
    err = (got - ref64).abs()
    e_cpu, e_gpu = float((ref32 - ref64).abs().max() / s), float(err.max() / s)
    print(f"[tol] {name}: gpu {e_gpu:.3e} fp32-cpu {e_cpu:.3e}")
    worst = float((err - (4.0 * e_cpu * s + 4 * ULP * ref64.abs())).max())
    assert worst <= 0.0, (name, e_gpu, e_cpu, worst)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _launch(entry, q_d, k_d, v_d, m_d, nb, dk, T, fill=CANARY):
    """`entry` into an output that held `fill`, inside a canary-filled buffer (64 floats each side keep the view 16-byte aligned)
    -> the output on the host, as int32 bit patterns."""
    n, pad = nb * H * dk * T, 64
    buf = torch.full((n + 2 * pad,), CANARY, device=q_d.device)
    out = buf[pad:pad + n].view(nb, H * dk, T)
    out.fill_(fill)
    _lib.check(getattr(_lib.load(), entry)(_p(q_d), _p(k_d), _p(v_d), _p(m_d), _p(out), nb, H, dk, T, ops._stream()), entry)
    torch.cuda.synchronize()
    c = buf.cpu()
    assert bool((c[:pad] == CANARY).all()) and bool((c[-pad:] == CANARY).all()), f"{entry}: canary overwritten"
    return c[pad:pad + n].view(nb, H * dk, T).view(torch.int32)


def _to(cuda, *ts):
    return [None if t is None else t.to(cuda) for t in ts]


@gpu
@pytest.mark.parametrize("dk,T,mask_kind", PARAMS, ids=[f"dk{dk}_T{T}_{m}" for dk, T, m in PARAMS])
def test_tiled_attention_equals_serial_bits_and_meets_fp64_bar(cuda, dk, T, mask_kind):
    """fac_attention takes the tiled kernel here; its output has the bits of fac_attention_serial's, meets the float64 bar, leaves
    the canaries round the output and the inputs alone, does not depend on what the output held before, and gives each clip the
    bits it gets when launched alone (B = 1)."""
    assert ops.attention_form(dk, T) == _form(dk, T) == "tiled"
    q, k, v, mask, o64, o32 = _case(dk, T, mask_kind)
    q_d, k_d, v_d, m_d = _to(cuda, q, k, v, mask)
    tiled = _launch("fac_attention", q_d, k_d, v_d, m_d, B, dk, T)
    assert torch.equal(tiled, _launch("fac_attention_tiled", q_d, k_d, v_d, m_d, B, dk, T, fill=float("nan")))
    serial = _launch("fac_attention_serial", q_d, k_d, v_d, m_d, B, dk, T)
    assert all(torch.equal(a.cpu(), b) for a, b in ((q_d, q), (k_d, k), (v_d, v)))
    assert mask is None or torch.equal(m_d.cpu(), mask)
    differ = int((tiled != serial).sum())
    assert differ == 0, f"{differ} of {tiled.numel()} outputs differ in bits from the serial kernel"
    _bar(f"attention_tiled_dk{dk}_T{T}_{mask_kind}", tiled.view(torch.float32), o64, o32)
    for b in range(B):
        one = _to(cuda, *(t[b:b + 1].contiguous() for t in (q, k, v)), None if mask is None else mask[b:b + 1].contiguous())
        assert torch.equal(_launch("fac_attention", *one, 1, dk, T)[0], tiled[b]), f"clip {b} alone"


@gpu
def test_unaligned_tensors_take_the_scalar_loads(cuda):
    """T % 4 == 0 but q, k, v and the output start 4 bytes off a 16-byte boundary: the same bits as the aligned launch."""
    dk, T = 24, 32
    q, k, v, mask, o64, o32 = _case(dk, T, "partial_mask")
    q_d, k_d, v_d, m_d = _to(cuda, q, k, v, mask)
    want = _launch("fac_attention", q_d, k_d, v_d, m_d, B, dk, T)
    n = B * H * dk * T
    off = [torch.cat([torch.zeros(1, device=cuda), t.reshape(-1)])[1:].view(B, H * dk, T) for t in (q_d, k_d, v_d)]
    buf = torch.full((n + 129,), CANARY, device=cuda)
    out = buf[65:65 + n].view(B, H * dk, T)
    assert all(t.data_ptr() % 16 == 4 for t in off + [out])
    _lib.check(_lib.load().fac_attention(_p(off[0]), _p(off[1]), _p(off[2]), _p(m_d), _p(out), B, H, dk, T, ops._stream()),
               "fac_attention")
    torch.cuda.synchronize()
    c = buf.cpu()
    assert bool((c[:65] == CANARY).all()) and bool((c[65 + n:] == CANARY).all())
    assert torch.equal(c[65:65 + n].view(B, H * dk, T).view(torch.int32), want)


@gpu
@pytest.mark.parametrize("T", [T_LAST_TILED, T_FIRST_SERIAL])
def test_route_at_the_end_of_the_tiled_layout(cuda, T):
    """dk = 256, one clip: T = 992 is the last T whose 32 score rows fit beside a V pass (160 KiB exactly) and runs tiled, T = 993
    runs the serial kernel, which fac_attention_tiled refuses.  Either way fac_attention returns the serial kernel's bits and
    meets the bar."""
    dk = 256
    assert ops.attention_form(dk, T) == _form(dk, T) == ("tiled" if T == T_LAST_TILED else "serial")
    q, k, v, mask, o64, o32 = _case(dk, T, "partial_mask", 1)
    q_d, k_d, v_d, m_d = _to(cuda, q, k, v, mask)
    got = _launch("fac_attention", q_d, k_d, v_d, m_d, 1, dk, T)
    assert torch.equal(got, _launch("fac_attention_serial", q_d, k_d, v_d, m_d, 1, dk, T))
    _bar(f"attention_tiled_cut_T{T}", got.view(torch.float32), o64, o32)
    if T == T_FIRST_SERIAL:
        with pytest.raises(_lib.FacodecHipError):
            _launch("fac_attention_tiled", q_d, k_d, v_d, m_d, 1, dk, T)
    else:
        assert torch.equal(ops.attention(q_d, k_d, v_d, m_d, H, kernel="serial"), ops.attention(q_d, k_d, v_d, m_d, H))


# ------------------------------------------------------------------------------------------------ no GPU
def test_form_is_the_shape_formula():
    assert _form(256, T_LAST_TILED) == "tiled" and _form(256, T_FIRST_SERIAL) == "serial"
    assert (256 * 36 + 32 * T_LAST_TILED) * 4 == 160 * 1024
    lib = _lib.load()
    for dk in (1, 24, 64, 255, 256, 257, 512):
        for T in (1, 31, 32, 33, 160, 960, 961, 991, 992, 993, 1024, 2048, 2049, 2304, 2305, 288000):
            assert ops.attention_form(dk, T) == _form(dk, T), (dk, T)
            assert bool(lib.fac_attention_tiled_fits(dk, T)) == _tiled_fits(dk, T), (dk, T)
            assert (ops.attention_form(dk, T) == "stream") == (ops.attention_route(dk, T) == "stream"), (dk, T)
    for dk, T, _ in PARAMS:
        assert _form(dk, T) == "tiled"


def test_cases_cover_the_tiling():
    assert {1, 15, 16, 17, 31, 32, 33, 160, 161, 192} <= set(TS) and set(DKS) == {24, 256}
    assert any(T % 4 for T in TS) and any(T % 32 == 0 for T in TS) and any(T % 32 == 1 for T in TS)
    assert ("clip_fully_masked" in MASKS) and ("partial_mask" in MASKS) and ("mask_null" in MASKS)


def test_entries_are_declared_and_the_fallback_stays():
    header = open(os.path.join(REPO, "include", "facodec_hip.h")).read()
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "fac_adamw_step" in v)
    for name in ("fac_attention_tiled", "fac_attention_serial"):
        assert f"int {name}(" in header and table[name] == table["fac_attention"]
    for name in ("fac_attention_form", "fac_attention_tiled_fits"):
        assert f"int {name}(" in header and name in table
    from facodec_amd import build
    assert "attention_tiled.hip" in build.SOURCES
    src = open(os.path.join(REPO, "facodec_amd", "csrc", "misc.hip")).read()
    assert "void attention_kernel(" in src          # the serial kernel stays in the library


def test_forced_kernel_is_checked_on_the_host():
    x = torch.zeros(1, 8, 4)
    with pytest.raises(ValueError):
        ops.attention(x, x, x, None, 2, kernel="nope")
    with pytest.raises(ValueError):
        ops.attention(x, x, x, None, 2, kernel="tiled")
