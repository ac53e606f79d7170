"""fac_attention_stream (csrc/attention_stream.hip): softmax attention with a running max and sum over key tiles, the route
fac_attention takes where its 16 x T score tile no longer fits the LDS.

The kernel against float64 softmax attention at every T where its tiling changes: one key, below / at / above one query tile and
one key tile (the tile sizes are the kernel's own, asked from the library), several key tiles with a ragged last one, and dk = 24
(zero-filled up to the 16-row output block).  Bound: the standing `maps` bar of tests/test_train_kernels_gen.py, 4 e_cpu + 4 ulp
in units of the largest |ref|, unchanged.  Two things are held apart on purpose: a MASKED key is still a key (its score is
replaced by -1e4, so a fully masked clip has uniform weights over all T keys), a key past T in the last tile is none (weight
exactly 0): the uniform-weights check (`_sum_bound` against the mean of V) fails on either confusion."""
import ctypes as C
import os

import pytest
import torch

from facodec_amd import _lib, ops

from test_train_kernels_gen import _attn_ref, _bar, _call, _canary, _canary_intact, _g, _p, _sum_bound

gpu = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 2
QT, KT = ops.attention_stream_tiles()
T_DK256 = sorted({1, QT - 1, QT, QT + 1, KT - 1, KT, KT + 1, 2 * KT + 3, 300})
CASES = [(256, T) for T in T_DK256] + [(24, 70)]
MASKS = ("mask_null", "partial_mask", "clip_fully_masked")
PARAMS = [(c, m) for c in CASES for m in MASKS if c[1] > 1 or m != "partial_mask"]     # one key: nothing to mask partly


def _inputs(dk, T, B, mask_kind, seed):
    """q, k, v (B, H dk, T) and the mask (B, T) or None, built as in test_attention_fused_fp64: the last clip loses its last
    min(17, T // 2) frames, `clip_fully_masked` also zeroes clip 0's whole mask."""
    g = _g(seed)
    q, k, v = (torch.randn(B, H * dk, T, generator=g) for _ in range(3))
    mask = None
    if mask_kind != "mask_null":
        mask = torch.ones(B, T)
        mask[-1, T - min(17, T // 2):] = 0
        if mask_kind == "clip_fully_masked":
            mask[0] = 0
    return q, k, v, mask


def _refs(q, k, v, mask, B, dk, T):
    o64 = _attn_ref(q.double(), k.double(), v.double(), mask.double() if mask is not None else None, B, H, dk, T)[0]
    return o64, _attn_ref(q, k, v, mask, B, H, dk, T)[0]


def _run(entry, q, k, v, mask, B, dk, T, cuda):
    """Launches `entry` on device copies; checks the canaries round `out` and that the inputs are untouched -> out (host)."""
    q_d, k_d, v_d = q.to(cuda), k.to(cuda), v.to(cuda)
    m_d = mask.to(cuda) if mask is not None else None
    out, buf, pad = _canary((B, H * dk, T), cuda)
    _call(entry, _p(q_d), _p(k_d), _p(v_d), _p(m_d), _p(out), B, H, dk, T)
    torch.cuda.synchronize()
    assert _canary_intact(buf, pad)
    assert all(torch.equal(a.cpu(), b) for a, b in ((q_d, q), (k_d, k), (v_d, v)))
    if mask is not None:
        assert torch.equal(m_d.cpu(), mask)
    o = out.cpu()
    assert bool(torch.isfinite(o).all())
    return o


@gpu
@pytest.mark.parametrize("case,mask_kind", PARAMS, ids=[f"dk{c[0]}_T{c[1]}_{m}" for c, m in PARAMS])
def test_attention_stream_fp64(cuda, case, mask_kind):
    """fac_attention_stream, B = 2, H = 2, against float64 softmax attention; on a fully masked clip also the T-term sum bound
    against the mean of V over ALL T keys (weights exp(0) / T: the sum T exact, 1 / T and each product rounded once: extra = 2)."""
    dk, T = case
    B = 2
    q, k, v, mask = _inputs(dk, T, B, mask_kind, dk + T + len(mask_kind))
    o64, o32 = _refs(q, k, v, mask, B, dk, T)
    out = _run("fac_attention_stream", q, k, v, mask, B, dk, T, cuda)
    tag = f"dk{dk}_T{T}_{mask_kind}"
    fails = []
    for fn, args, kw in [(_bar, (f"attention_stream_{tag}", out, o64, o32), {})] + ([] if mask_kind != "clip_fully_masked" else [
            (_sum_bound, (f"attention_stream_uniform_{tag}", out[0], v[0].double().mean(-1, keepdim=True).expand(H * dk, T),
                          (v[0].double().abs().sum(-1, keepdim=True) / T).expand(H * dk, T), T), dict(extra=2.0))]):
        try:
            fn(*args, **kw)
        except AssertionError as e:
            fails.append(str(e)[:300])
    assert not fails, fails


@gpu
@pytest.mark.parametrize("mask_kind", ["partial_mask", "mask_null"])
def test_attention_routes_past_the_lds_tile(cuda, mask_kind):
    """fac_attention at dk = 256, T = 2305: one frame past the LDS score tile.  It used to refuse ("too long for the LDS score
    tile"); it now takes the stream route and meets the same bar."""
    dk, T, B = 256, 2305, 1
    assert ops.attention_route(dk, T) == "stream"
    q, k, v, mask = _inputs(dk, T, B, mask_kind, 2305 + len(mask_kind))
    o64, o32 = _refs(q, k, v, mask, B, dk, T)
    out = _run("fac_attention", q, k, v, mask, B, dk, T, cuda)
    _bar(f"attention_routed_T{T}_{mask_kind}", out, o64, o32)


@gpu
def test_both_routes_meet_the_bar_at_the_cut(cuda):
    """T = 2304, the last T of the LDS route: fac_attention (LDS kernel) and fac_attention_stream each within the bar of the same
    float64 reference.  Equal bits are not asked: the two sum in different orders.  ops.attention(kernel=...) reaches both."""
    dk, T, B = 256, 2304, 1
    assert ops.attention_route(dk, T) == "lds"
    q, k, v, mask = _inputs(dk, T, B, "partial_mask", 2304)
    o64, o32 = _refs(q, k, v, mask, B, dk, T)
    for entry in ("fac_attention", "fac_attention_stream"):
        _bar(f"attention_cut_T{T}_{entry}", _run(entry, q, k, v, mask, B, dk, T, cuda), o64, o32)
    q_d, k_d, v_d, m_d = (t.to(cuda) for t in (q, k, v, mask))
    _bar("attention_cut_ops_stream", ops.attention(q_d, k_d, v_d, m_d, H, kernel="stream").cpu(), o64, o32)
    assert torch.equal(ops.attention(q_d, k_d, v_d, m_d, H, kernel="lds"), ops.attention(q_d, k_d, v_d, m_d, H))


# ------------------------------------------------------------------------------------------------ no GPU
def _lds_route(dk, T):
    """fac_attention's LDS route holds 16 queries (dk x 16) and 16 x T scores in 160 KiB."""
    return "lds" if (16 * dk + 16 * T) * 4 <= 160 * 1024 else "stream"


def test_attention_route_is_the_lds_formula():
    from test_infer_kernels import ATTN_CASES
    for dk, T, _, _ in ATTN_CASES:
        assert ops.attention_route(dk, T) == "lds", (dk, T)
    assert ops.attention_route(256, 2304) == "lds" and ops.attention_route(256, 2305) == "stream"
    for dk in (1, 8, 24, 64, 100, 128, 256, 512, 2048):
        t_max = (160 * 1024 // 4 - 16 * dk) // 16
        for T in (1, t_max - 1, t_max, t_max + 1, 10 * t_max, 288000):
            if T > 0:
                assert ops.attention_route(dk, T) == _lds_route(dk, T), (dk, T)
    src = open(os.path.join(REPO, "facodec_amd", "csrc", "misc.hip")).read()
    assert "if (fac_attention_route(dk, T) == FAC_ATTN_STREAM) return fac_attention_stream(" in src     # the entry asks the same function


def test_cases_cover_the_tiling():
    assert QT > 1 and KT > 1
    ts = {T for dk, T in CASES if dk == 256}
    assert {1, QT - 1, QT, QT + 1, KT - 1, KT, KT + 1, 2 * KT + 3, 300} <= ts
    assert any(T % KT and T > 2 * KT for T in ts)                     # several key tiles with a ragged last one
    assert (24, 70) in CASES and 24 % 16                              # dk below the 16-row output block


def test_stream_entry_is_declared():
    header = open(os.path.join(REPO, "include", "facodec_hip.h")).read()
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "fac_adamw_step" in v)
    assert "fac_attention_stream" in table and "int fac_attention_stream(" in header
    assert table["fac_attention_stream"][1][-1] is C.c_void_p
    assert table["fac_attention_stream"] == table["fac_attention"]
    assert "int fac_attention_route(" in header and "fac_attention_route" in table
    from facodec_amd import build
    assert "attention_stream.hip" in build.SOURCES


def test_forced_route_is_checked_on_the_host():
    x = torch.zeros(1, 8, 4)
    with pytest.raises(ValueError):
        ops.attention(x, x, x, None, 2, kernel="nope")
