"""The kernels the inference path runs between its convs, one at a time: the elementwise and layout glue of misc.hip (Snake, the
WaveNet gate and skip, GLU, the code-embedding sum, the streaming context buffer, the anti-aliased SnakeBeta, the fused
attention), the LSTM's time-major transposes (lstm.hip), the P8 pre-pass fac_to_p8, and the per-row kernels of ragged.hip.

Every reference is computed on the CPU from the same fp32 inputs; every output lies inside a canary buffer that is checked after
the call; every output is asserted finite.  Two kinds of bound, as in tests/test_train_kernels_gen.py (whose helpers are used):
  exact  copies, selections, layouts, untouched regions and the fp32 expressions include/facodec_hip.h defines: bit-equal to the
         same expression evaluated by torch on the CPU;
  maps   the SAME formula evaluated in fp32 by torch on the CPU has the error e_cpu against fp64; the kernel must stay within
         4 e_cpu + 4 ulp at EVERY element (`_bar`).  The factor 4 is nowhere raised.
The case ids begin with the branch of the dispatch they take (`pytest --collect-only -q` lists the coverage); each dispatch is
restated here and pinned to the source text by a test that needs no GPU.

Left out: fac_snake_fwd's flat fallback for B * C > 65535 rows at T >= 1024 (at least 65536 * 1024 floats: a quarter-gigabyte
tensor and its fp64 reference for one comparison)."""
import ctypes as C
import inspect
import os

import pytest
import torch

from facodec_amd import _lib
from test_train_kernels_gen import (CANARY, EPS32, ULP, _aa_snakebeta_fwd_ref, _attn_ref, _bar, _call, _canary, _canary_intact, _g,
                                    _kaiser_sinc_filter12, _p, _record, _sigmoid, _span, _sum_bound)

gpu = pytest.mark.gpu
# Measured on MI355X: NOT YET.  These tests were written and their references checked without access to a device; no GPU figure
# below is measured.  Every case prints and records its (GPU error, fp32-CPU error) pair ([tol] lines, the tolerance report of
# tests/test_gpu_parity.py): the worst GPU figure of each family belongs next to the fp32-CPU figure here after the first run.
# fp32-CPU error e_cpu, worst case of each family, in units of the scale the test states (deterministic: measured on the CPU):
#   snake_fwd 9.5e-8 (per-channel largest |ref|); lstm_from_time_major with alpha 1.3e-7 (same scale)
#   gate_tanh_sigmoid 1.6e-7 without g, 1.0e-6 with g (relative, at every element; the rounding of a + g at |a| = 20 is common to
#   the kernel and the fp32 reference); glu_residual 1.3e-7 (|res| + |a1| sigmoid(a2))
#   aa_snakebeta_fwd 1.8e-7, attention 1.8e-6 (largest |ref|)
# The bar is 4 e_cpu + 4 ulp throughout; no factor is raised.
REPO =os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    """The tensor's bit patterns, so that -0 / +0 and every rounding count in a comparison."""
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _finite(*ts):
    return all(bool(torch.isfinite(t.detach().float().cpu()).all()) for t in ts)


def _collect(fails, fn, *a, **k):
    try:
        return fn(*a, **k)
    except AssertionError as e:
        fails.append(str(e)[:300])


# ======================================================================================================= 1. exact
EW_N = [1, 255, 257, 8192 * 256 + 77]          # ew_grid caps the grid at 8192 blocks of 256: the last size takes the stride loop twice


@gpu
@pytest.mark.parametrize("n", EW_N, ids=[f"{'grid_stride_twice' if n > 8192 * 256 else 'one_pass'}_n{n}" for n in EW_N])
def test_add_and_sub2_exact(cuda, n):
    """fac_add: out = a + b; fac_sub2: out = (a - b) - c in that order (another association differs in the last bit, asserted on
    the inputs), through the C entries and through ops.add / ops.sub2."""
    from facodec_amd import ops
    g = _g(n)
    a, b, c = (torch.randn(n, generator=g) * s for s in (1.0, 3.0, 0.01))
    a_d, b_d, c_d = a.to(cuda), b.to(cuda), c.to(cuda)
    s, sbuf, pad = _canary((n,), cuda)
    d, dbuf, _ = _canary((n,), cuda)
    _call("fac_add", _p(a_d), _p(b_d), _p(s), n)
    _call("fac_sub2", _p(a_d), _p(b_d), _p(c_d), _p(d), n)
    s2, d2 = ops.add(a_d, b_d), ops.sub2(a_d, b_d, c_d)
    torch.cuda.synchronize()
    assert _canary_intact(sbuf, pad) and _canary_intact(dbuf, pad) and _finite(s, d)
    assert _same_bits(s, a + b) and _same_bits(s2, a + b)
    assert _same_bits(d, (a - b) - c) and _same_bits(d2, (a - b) - c)
    if n >= 255:
        assert not torch.equal((a - b) - c, a - (b + c))       # the order is visible in these inputs
    assert torch.equal(a_d.cpu(), a) and torch.equal(b_d.cpu(), b) and torch.equal(c_d.cpu(), c)


@gpu
@pytest.mark.parametrize("B,Cc,T", [(1, 1, 1), (3, 5, 63), (2, 7, 130)])
def test_mul_mask_exact(cuda, B, Cc, T):
    """fac_mul_mask: x[b, c, t] *= mask[b, t] in place, every clip with its own 0 / 1 mask."""
    from facodec_amd import ops
    g = _g(B * T)
    x = torch.randn(B, Cc, T, generator=g)
    mask = (torch.rand(B, T, generator=g) > 0.4).float()
    if T > 1:
        mask[:, 0], mask[:, -1] = 1.0, 0.0
        mask[0, T // 2:] = 0.0
        assert all(not torch.equal(mask[0], mask[b]) for b in range(1, B))
    xv, buf, pad = _canary((B, Cc, T), cuda)
    xv.copy_(x)
    m_d = mask.to(cuda)
    _call("fac_mul_mask", _p(xv), _p(m_d), B, Cc, T)
    x2 = ops.mul_mask_(x.to(cuda), m_d)
    torch.cuda.synchronize()
    want = x * mask.view(B, 1, T)
    assert _canary_intact(buf, pad) and _finite(xv)
    assert _same_bits(xv, want) and _same_bits(x2, want)
    assert torch.equal(m_d.cpu(), mask)


@gpu
@pytest.mark.parametrize("B,Cc,T", [(1, 1, 1), (3, 6, 33)])
@pytest.mark.parametrize("mode", ["middle", "last", "last_x_null"])
def test_wn_res_skip_exact(cuda, mode, B, Cc, T):
    """fac_wn_res_skip: last = 0: x += rs[:, :C], out += rs[:, C:] with rs (B, 2C, T); last = 1: out += rs (B, C, T), x is not
    touched and may be NULL.  The two halves of rs differ by 100, so swapped halves change every element."""
    g = _g(B * T + len(mode))
    last = mode != "middle"
    rs = torch.randn(B, Cc if last else 2 * Cc, T, generator=g)
    if not last:
        rs[:, Cc:] += 100.0
    x0, out0 = torch.randn(B, Cc, T, generator=g), torch.randn(B, Cc, T, generator=g)
    x, xbuf, pad = _canary((B, Cc, T), cuda)
    out, obuf, _ = _canary((B, Cc, T), cuda)
    x.copy_(x0)
    out.copy_(out0)
    rs_d = rs.to(cuda)
    _call("fac_wn_res_skip", _p(rs_d), _p(None if mode == "last_x_null" else x), _p(out), B, Cc, T, int(last))
    torch.cuda.synchronize()
    assert _canary_intact(xbuf, pad) and _canary_intact(obuf, pad) and _finite(x, out)
    if last:
        assert _same_bits(x, x0) and _same_bits(out, out0 + rs)
    else:
        assert _same_bits(x, x0 + rs[:, :Cc]) and _same_bits(out, out0 + rs[:, Cc:])
        assert not torch.equal(x0 + rs[:, :Cc], x0 + rs[:, Cc:])
    assert torch.equal(rs_d.cpu(), rs)


def _embed_ref(codes, tables, n_tab, row0, out0):
    """out0 (or zeros) + table_0[codes[:, row0]] + table_1[codes[:, row0 + 1]] + ..., added in fp32 in table order."""
    B, _, T = codes.shape
    s = out0.clone() if out0 is not None else torch.zeros(B, tables.shape[2], T)
    for k in range(n_tab):
        s = s + tables[k][codes[:, row0 + k]].permute(0, 2, 1)
    return s


@gpu
@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("E,T", [(1, 1), (5, 17)])
@pytest.mark.parametrize("n_tab", [0, 1, 3])
def test_embed_sum_exact(cuda, n_tab, E, T, accumulate):
    """fac_embed_sum: the sum starts at 0 (or at `out`) and runs in table order, table i reads code row code_row0 + i; n_codes =
    n_tab + 1 so code_row0 = 0 and 1 both leave one row unread (it holds other valid codes); codes reach 0 and V - 1; another
    order of the additions shows in the last bit (asserted on the inputs).  n_tab = 0: zeros when storing, `out` unchanged when
    accumulating."""
    from facodec_amd import ops
    B, V = 2, 7
    g = _g(100 * n_tab + 10 * E + T + accumulate)
    n_codes = n_tab + 1
    codes = torch.randint(0, V, (B, n_codes, T), generator=g)
    codes[0, :, 0] = 0
    codes[-1, :, -1] = V - 1
    codes[0, -1, 0] = V - 1
    tables = torch.randn(max(n_tab, 1), V, E, generator=g) * torch.tensor([1.0, 3.0, 0.3])[:max(n_tab, 1)].view(-1, 1, 1)
    out0 = torch.randn(B, E, T, generator=g) * 10
    c_d, t_d = codes.to(cuda), tables.to(cuda)
    for row0 in (0, 1):
        out, buf, pad = _canary((B, E, T), cuda)
        out.copy_(out0)
        _call("fac_embed_sum", _p(c_d), _p(t_d), _p(out), B, n_tab, n_codes, row0, V, E, T, accumulate)
        torch.cuda.synchronize()
        want = _embed_ref(codes, tables, n_tab, row0, out0 if accumulate else None)
        assert _canary_intact(buf, pad) and _finite(out)
        assert _same_bits(out, want), (row0, float((out.cpu() - want).abs().max()))
        if n_tab == 0:
            assert _same_bits(out, out0 if accumulate else torch.zeros(B, E, T))
        if n_tab > 0:                                            # the wrapper: accumulate = an `out` is given
            got = ops.embed_sum(c_d, t_d, row0, out0.to(cuda) if accumulate else None)
            torch.cuda.synchronize()
            assert _same_bits(got, want)
    if n_tab == 3 and T > 1:
        rev = (tables[2][codes[:, 2]] + tables[1][codes[:, 1]] + tables[0][codes[:, 0]]).permute(0, 2, 1)
        assert not torch.equal(rev, _embed_ref(codes, tables, 3, 0, None))     # the order is visible in these inputs
    assert torch.equal(c_d.cpu(), codes) and torch.equal(t_d.cpu(), tables)


def _push_ref(buf, src, hist, n_prev):
    new = buf.clone()
    if n_prev > 0 and hist > 0:
        new[:, :hist] = buf[:, n_prev:n_prev + hist]
    new[:, hist:hist + src.shape[1]] = src
    return new


def test_stream_push_restatement_keeps_the_latest_columns():
    """The restated push on rows that hold their own column numbers: after [hist | n_prev] + n_new the row holds the last `hist`
    columns of what it held, then the new ones (the header's semantics); n_prev = 0 moves nothing."""
    hist, n_prev, n_new = 4, 3, 2
    buf = torch.arange(10.0).view(1, 10)
    new = _push_ref(buf, torch.tensor([[100.0, 101.0]]), hist, n_prev)
    assert new[0].tolist() == [3.0, 4.0, 5.0, 6.0, 100.0, 101.0, 6.0, 7.0, 8.0, 9.0]
    assert _push_ref(buf, torch.tensor([[100.0]]), hist, 0)[0].tolist() == [0.0, 1.0, 2.0, 3.0, 100.0, 5.0, 6.0, 7.0, 8.0, 9.0]


@gpu
@pytest.mark.parametrize("hist", [0, 1, 255, 256, 257, 2048])
def test_stream_push_exact(cuda, hist):
    """fac_stream_push on 3 rows of `cap` columns: n_prev = 0 (nothing moves), n_prev < hist (source and destination of the move
    overlap) and n_prev > hist, each with n_new = 1 and 300; the whole buffer -- the columns behind hist + n_new and the canaries
    included -- against the restated move."""
    from facodec_amd import ops
    rows = 3
    for n_prev in sorted({0, hist // 2, hist + 3}):
        for n_new in (1, 300):
            cap = hist + max(n_prev, n_new) + 5
            g = _g(hist * 7 + n_prev + n_new)
            b0, src = torch.randn(rows, cap, generator=g), torch.randn(rows, n_new, generator=g)
            buf, cbuf, pad = _canary((rows, cap), cuda)
            buf.copy_(b0)
            s_d = src.to(cuda)
            _call("fac_stream_push", _p(buf), _p(s_d), rows, cap, hist, n_prev, n_new)
            torch.cuda.synchronize()
            want = _push_ref(b0, src, hist, n_prev)
            assert _canary_intact(cbuf, pad) and _finite(buf), (n_prev, n_new)
            assert _same_bits(buf, want), (n_prev, n_new)
            assert _same_bits(buf[:, hist + n_new:], b0[:, hist + n_new:])
            b3 = b0.view(1, rows, cap).to(cuda)
            ops.stream_push(b3, s_d.view(1, rows, n_new), hist, n_prev)
            torch.cuda.synchronize()
            assert _same_bits(b3[0], want)


def _snake_fwd_ref(x, alpha, dtype):
    """y = x + sin(alpha x)^2 / (alpha + 1e-9), alpha per channel (the header's formula)."""
    x = x.to(dtype)
    a = alpha.to(dtype).view(1, -1, 1)
    return x + torch.sin(a * x).pow(2) / (a + torch.as_tensor(1e-9, dtype=dtype))


def _chan_scale(ref64):
    """The largest |ref| of each channel, at every element of that channel."""
    return ref64.abs().amax((0, 2), keepdim=True).expand_as(ref64)


@gpu
@pytest.mark.parametrize("B", [1, 31, 32, 33])
def test_lstm_time_major_transposes(cuda, B):
    """fac_lstm_to_time_major: (B, H, T) -> (H, T, BP) with zeros in the columns b >= B; fac_lstm_from_time_major: back, + skip
    (exactly yT + skip, or exactly yT when skip is NULL; the padded columns of yT hold other values, which must not be read into
    the result); the round trip is the identity; with alpha the Snake of yT + skip under the maps bound, per channel.  T and H
    around the 32 x 32 tile."""
    from facodec_amd import ops
    BP = 32 * ((B + 31) // 32)
    fails = []
    for T in (1, 31, 33):
        for H in (1, 3):
            tag = f"B{B}_T{T}_H{H}"
            g = _g(1000 * B + 10 * T + H)
            x = torch.randn(B, H, T, generator=g)
            x_d = x.to(cuda)
            xT, tbuf, pad = _canary((H, T, BP), cuda)
            _call("fac_lstm_to_time_major", _p(x_d), _p(xT), B, H, T)
            torch.cuda.synchronize()
            want = torch.zeros(H, T, BP)
            want[..., :B] = x.permute(1, 2, 0)
            assert _canary_intact(tbuf, pad) and _finite(xT), tag
            assert _same_bits(xT, want), tag
            assert bool((xT.cpu()[..., B:] == 0).all()), tag
            assert _same_bits(ops.lstm_to_time_major(x_d), want), tag
            yT = torch.randn(H, T, BP, generator=g)
            skip = torch.randn(B, H, T, generator=g)
            y_d, s_d = yT.to(cuda), skip.to(cuda)
            back = yT[..., :B].permute(2, 0, 1)
            for sk, ref in ((None, back), (s_d, back + skip)):
                out, obuf, _ = _canary((B, H, T), cuda)
                _call("fac_lstm_from_time_major", _p(y_d), _p(sk), _p(None), _p(out), B, H, T)
                torch.cuda.synchronize()
                assert _canary_intact(obuf, pad) and _finite(out), tag
                assert _same_bits(out, ref), tag
                assert _same_bits(ops.lstm_from_time_major(y_d, sk, B), ref), tag
            rt, rbuf, _ = _canary((B, H, T), cuda)
            _call("fac_lstm_from_time_major", _p(xT), _p(None), _p(None), _p(rt), B, H, T)
            torch.cuda.synchronize()
            assert _canary_intact(rbuf, pad) and _same_bits(rt, x), tag
            # with alpha: channel 0 typical, channel 1 tiny (1e-6), channel 2 with alpha v reaching 30
            v = back + skip                                       # the fp32 sum the exact part above pins
            alpha = torch.tensor([1.3, 1e-6, 30.0 / float(v.abs().max())])[:H].contiguous()
            a_d = alpha.to(cuda)
            out, obuf, _ = _canary((B, H, T), cuda)
            _call("fac_lstm_from_time_major", _p(y_d), _p(s_d), _p(a_d), _p(out), B, H, T)
            torch.cuda.synchronize()
            assert _canary_intact(obuf, pad), tag
            r64 = _snake_fwd_ref(yT[..., :B].permute(2, 0, 1).double() + skip.double(), alpha, torch.float64)
            r32 = _snake_fwd_ref(v, alpha, torch.float32)
            _collect(fails, _bar, f"lstm_from_time_major_snake_{tag}", out, r64, r32, scale=_chan_scale(r64))
    assert not fails, fails


def _p8_ref(x):
    """fac_conv_desc.x_p8 restated with torch's round-to-nearest-even bfloat16 conversions: three planes hi / mid / lo, each
    [b][c / 8][t][8 channels] followed by ONE zero unit: (3, B * C / 8 * T + 1, 8) bfloat16."""
    B, Cc, T = x.shape
    u = x.view(B, Cc // 8, 8, T).permute(0, 1, 3, 2).reshape(-1, 8)
    h = u.bfloat16()
    r1 = u - h.float()
    m = r1.bfloat16()
    lo = (r1 - m.float()).bfloat16()
    planes = torch.zeros(3, u.shape[0] + 1, 8, dtype=torch.bfloat16)
    planes[0, :-1], planes[1, :-1], planes[2, :-1] = h, m, lo
    return planes


# 0 and -0; 1 + 2^-8 and -(1 + 2^-8): halfway between two bf16 numbers, the even neighbour is 1; 1 + 3 * 2^-8: halfway, the even
# neighbour is 1 + 2^-6 (upwards); 1 + 2^-9 + 2^-17: the residual x - hi = 2^-9 (1 + 2^-8) is halfway for the SECOND split
P8_EDGES = [0.0, -0.0, 1 + 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -9 + 2.0 ** -17, 3.0e-30, -7.7e30]


def _p8_input(B, Cc, T, seed):
    g = _g(seed)
    x = torch.randn(B, Cc, T, generator=g) * torch.exp(torch.randn(B, Cc, T, generator=g) * 3)
    x.view(-1)[:len(P8_EDGES)] = torch.tensor(P8_EDGES)
    return x


def _p8_run(cuda, x, alpha):
    B, Cc, T = x.shape
    n = B * (Cc // 8) * T
    raw, buf, pad = _canary((3 * (n + 1) * 4,), cuda)             # fp32 canaries around 3 (n + 1) units of 16 bytes
    x_d = x.to(cuda)
    a_d = alpha.to(cuda) if alpha is not None else None
    _call("fac_to_p8", _p(x_d), _p(a_d), _p(raw), B, Cc, T)
    torch.cuda.synchronize()
    assert _canary_intact(buf, pad), "fac_to_p8 wrote outside its three planes"
    assert torch.equal(x_d.cpu(), x)
    return raw.cpu().view(torch.bfloat16).view(3, n + 1, 8)


@gpu
@pytest.mark.parametrize("B,Cc,T", [(1, 8, 1), (2, 24, 37)])
def test_to_p8_layout_and_split_exact(cuda, B, Cc, T):
    """fac_to_p8 without alpha: the three planes bit for bit (the unit order [b][c / 8][t][8], the round-to-nearest-even splits,
    -0 kept in the hi plane), the closing zero unit of every plane (the buffer is pre-filled with a non-zero canary), the canary
    behind the third plane, and hi + mid + lo == x."""
    from facodec_amd import ops
    x = _p8_input(B, Cc, T, B * T)
    planes = _p8_run(cuda, x, None)
    want = _p8_ref(x)
    assert _finite(planes)
    for p, nm in enumerate(("hi", "mid", "lo")):
        assert _same_bits(planes[p, -1], torch.zeros(8, dtype=torch.bfloat16)), f"closing zero unit of the {nm} plane"
        assert _same_bits(planes[p, :-1], want[p, :-1]), f"{nm} plane"
    assert _same_bits(planes, want)
    assert torch.equal(ops.P8(planes, (B, Cc, T)).to_float(), x)  # three addends of disjoint significance: exact
    assert _same_bits(ops.to_p8(x.to(cuda)).planes, want)


@gpu
@pytest.mark.parametrize("B,Cc,T", [(1, 8, 1), (2, 24, 37)])
def test_to_p8_with_alpha_is_the_split_of_snake(cuda, B, Cc, T):
    """fac_to_p8 with alpha: the planes are the exact split of ops.snake(x, alpha) as the GPU computes it (fac_snake_fwd is held
    against fp64 below), zero units and canaries as without alpha."""
    from facodec_amd import ops
    g = _g(B + T)
    x = torch.randn(B, Cc, T, generator=g) * 2
    alpha = torch.exp(torch.randn(Cc, generator=g))
    y = ops.snake(x.to(cuda), alpha.to(cuda)).cpu()
    planes = _p8_run(cuda, x, alpha)
    assert _finite(planes) and _same_bits(planes, _p8_ref(y))


# ------------------------------------------------------------------------------------------------------- ragged.hip
INT_MAX = 2 ** 31 - 1


def _ragged_lens(T, unit):
    """Lengths in samples for rows of T columns of `unit` samples: 0, 1, unit - 1, exactly T * unit, one more, negative, 2^31 - 1,
    and one inside the row."""
    return [0, 1, unit - 1, T * unit, T * unit + 1, -5, INT_MAX, (T // 2) * unit + unit // 2]


def _tail_start(lens, unit, T):
    """First zeroed column of each row: the length clamped to [0, ...) before it is used, lens / unit columns kept, at most T
    (include/facodec_hip.h: `a length is clamped to [0, T] before it indexes anything`)."""
    return (torch.as_tensor(lens, dtype=torch.int64).clamp(min=0) // unit).clamp(max=T)


def test_tail_start_clamps_as_the_header_says():
    """The restated clamp, before a GPU test relies on it: negative -> 0 columns kept, beyond the row -> all T kept, unit - 1 -> 0."""
    for T, unit in ((1, 1), (3, 300), (5, 300), (7201, 1)):
        lens = _ragged_lens(T, unit)
        s = _tail_start(lens, unit, T).tolist()
        assert s[0] == 0 and s[1] == (1 if unit == 1 else 0) and s[2] == 0
        assert s[3] == T and s[4] == T and s[5] == 0 and s[6] == T and s[7] == T // 2
        assert all(0 <= v <= T for v in s)
    assert _tail_start([599, 600, 601], 300, 5).tolist() == [1, 2, 2]
    assert torch.tensor(_ragged_lens(5, 300), dtype=torch.int32).tolist() == _ragged_lens(5, 300)        # all fit int32


MASK_CASES = [(1, 3, 1), (1, 3, 2), (300, 2, 3), (300, 5, 5), (1, 2, 7201)]


@gpu
@pytest.mark.parametrize("off", [0, 1], ids=["base_16B_aligned", "base_one_element_in"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.int64], ids=["fp32", "i64"])
@pytest.mark.parametrize("unit,Cc,T", MASK_CASES, ids=[f"unit{u}_C{c}_T{t}" for u, c, t in MASK_CASES])
def test_mask_tail_edges_exact(cuda, unit, Cc, T, dtype, off):
    """fac_mask_tail / fac_mask_tail_i64 with the lengths of _ragged_lens (one row group each), rows too short for one 16-byte
    store (T = 1, 2, 3), C * T = 25 (odd row starts), a sample-rate row of 7201, and a tensor that starts one element into its
    buffer (fp32: the base is only 4-byte aligned).  The WHOLE buffer, canaries on both sides included, is compared bit for bit
    with torch indexing: nothing outside a row's own tail may change, whatever the length."""
    lens = _ragged_lens(T, unit)
    B = len(lens)
    n, pad = B * Cc * T, 64
    g = _g(unit + Cc + T + off)
    x = torch.randn(B, Cc, T, generator=g) if dtype == torch.float32 else torch.randint(1, 1 << 40, (B, Cc, T), generator=g)
    host = torch.full((n + 2 * pad,), CANARY, dtype=dtype)
    host[pad + off:pad + off + n] = x.view(-1)
    buf = host.to(cuda)
    view = buf[pad + off:pad + off + n].view(B, Cc, T)
    assert (view.data_ptr() % 16 == 0) == (off == 0)
    lens_d = torch.tensor(lens, dtype=torch.int32).to(cuda)
    _call("fac_mask_tail" if dtype == torch.float32 else "fac_mask_tail_i64", _p(view), _p(lens_d), B, Cc, T, unit)
    torch.cuda.synchronize()
    want = host.clone()
    wv = want[pad + off:pad + off + n].view(B, Cc, T)
    for b, s in enumerate(_tail_start(lens, unit, T).tolist()):
        wv[b, :, s:] = 0
    assert _same_bits(buf, want)
    assert torch.equal(lens_d.cpu(), torch.tensor(lens, dtype=torch.int32))


@gpu
@pytest.mark.parametrize("F", [1, 5, 300])
@pytest.mark.parametrize("with_n_valid", [True, False], ids=["n_valid", "n_valid_null"])
def test_frame_mask_edges_exact(cuda, F, with_n_valid):
    """fac_frame_mask: mask[b, f] = f < lens[b] / unit and n_valid[b] = min(lens[b] / unit, F) (or NULL) for the lengths of
    _ragged_lens, F below, at and above one block of 256."""
    unit = 300
    lens = _ragged_lens(F, unit)
    B = len(lens)
    lens_d = torch.tensor(lens, dtype=torch.int32).to(cuda)
    mask, mbuf, pad = _canary((B, F), cuda)
    nv, nbuf, _ = _canary((B,), cuda, dtype=torch.int32)
    _call("fac_frame_mask", _p(lens_d), _p(mask), _p(nv if with_n_valid else None), B, F, unit)
    torch.cuda.synchronize()
    start = _tail_start(lens, unit, F)
    assert _canary_intact(mbuf, pad) and _canary_intact(nbuf, pad) and _finite(mask)
    assert _same_bits(mask, (torch.arange(F).view(1, F) < start.view(B, 1)).float())
    assert torch.equal(nv.cpu(), start.to(torch.int32) if with_n_valid else torch.full((B,), int(CANARY), dtype=torch.int32))


def _frames_ref(w, lens, n_win, n_frames, hop, pad, n_off):
    """The gather of stft_frames_ragged_kernel's comment, in integers: row b is framed as if it were L = clamp(lens[b], 0, T)
    samples long and has min(L / hop, n_frames) frames; frames[b][n][f] = w[b][t], t = f hop + n + n_off - pad reflected at 0
    (-t) and at the clip's end (2 (L - 1) - t); what is still outside [0, L) reads as 0; the other frame columns are zeros."""
    B, T = w.shape
    out = torch.zeros(B, n_win, n_frames, dtype=w.dtype)
    for b in range(B):
        L = min(max(int(lens[b]), 0), T)
        nf = min(L // hop, n_frames)
        if nf == 0:
            continue
        t = torch.arange(nf).view(1, nf) * hop + torch.arange(n_win).view(n_win, 1) + (n_off - pad)
        t = torch.where(t < 0, -t, t)
        t = torch.where(t >= L, 2 * (L - 1) - t, t)
        ok = (t >= 0) & (t < L)
        out[b, :, :nf] = torch.where(ok, w[b][t.clamp(0, L - 1)], torch.zeros((), dtype=w.dtype))
    return out


# (n_win, hop, pad, n_off, T, n_frames, lens): a clip shorter than hop (no frame: an all-zero row), clips no longer than pad
# (fac_stft_frames refuses those: the reference is the gather above), the lengths of _ragged_lens, n_frames below T / hop
FRAME_CASES = {
    "small": (16, 4, 8, 0, 40, 10, [0, 1, 3, 4, 8, 9, 23, 40, 41, -5, INT_MAX]),
    "small_n_off3_fewer_frames": (16, 4, 8, 3, 40, 7, [0, 1, 3, 4, 8, 9, 23, 40, 41, -5, INT_MAX]),
    "logmel_1200_300": (1200, 300, 1024, 424, 7201, 24, [0, 1, 299, 300, 1024, 1025, 5130, 7200, 7201, 7202, -5, INT_MAX]),
}


@gpu
@pytest.mark.parametrize("off", [0, 1], ids=["base_16B_aligned", "base_4B_aligned"])
@pytest.mark.parametrize("case", list(FRAME_CASES))
def test_stft_frames_ragged_edges_exact(cuda, case, off):
    """fac_stft_frames_ragged against the restated gather, bit for bit.  The padding of every row holds 7.0 and the buffer
    around the wave holds the canary value: a sample read from outside the clip shows in the frames."""
    n_win, hop, pad_, n_off, T, n_frames, lens = FRAME_CASES[case]
    B = len(lens)
    g = _g(T + off)
    w = torch.randn(B, T, generator=g)
    for b, L in enumerate(lens):
        w[b, min(max(L, 0), T):] = 7.0
    host = torch.full((B * T + 128,), CANARY)
    host[64 + off:64 + off + B * T] = w.view(-1)
    wbuf = host.to(cuda)
    w_d = wbuf[64 + off:64 + off + B * T].view(B, T)
    assert (w_d.data_ptr() % 16 == 0) == (off == 0)
    lens_d = torch.tensor(lens, dtype=torch.int32).to(cuda)
    fr, fbuf, cp = _canary((B, n_win, n_frames), cuda)
    _call("fac_stft_frames_ragged", _p(w_d), _p(lens_d), _p(fr), B, T, n_win, n_frames, hop, pad_, n_off)
    torch.cuda.synchronize()
    assert _canary_intact(fbuf, cp) and _finite(fr)
    want = _frames_ref(w, lens, n_win, n_frames, hop, pad_, n_off)
    assert _same_bits(fr, want)
    got = fr.cpu()
    assert not bool((got == 7.0).any()) and not bool((got == CANARY).any())
    for b, L in enumerate(lens):
        if min(max(L, 0), T) < hop:
            assert bool((got[b] == 0).all()), b                  # shorter than one hop: no frame at all
    assert _same_bits(wbuf, host)


# ======================================================================================================= 2. maps
def _snake_branch(B, Cc, T):
    """fac_snake_fwd's dispatch (misc.hip), restated."""
    return "rows" if T >= 1024 and B * Cc <= 65535 else "flat"


SNAKE_T = [1, 1023, 1024, 1025, 2049]
SNAKE_B, SNAKE_C = 2, 3


@gpu
@pytest.mark.parametrize("T", SNAKE_T, ids=[f"{_snake_branch(SNAKE_B, SNAKE_C, T)}_T{T}" for T in SNAKE_T])
def test_snake_fwd_fp64(cuda, T):
    """fac_snake_fwd, the flat kernel (T < 1024) and the rows kernel (T >= 1024: 1024-column chunks, T = 1025 and 2049 leave a
    chunk of one column).  Channel 0: alpha = 1e-6 on samples of size 1e6, so alpha x = O(1) and the term sin^2 / (alpha + 1e-9) is
    as large as x -- the 1e-9 of the denominator is then 1e-3 of that term; channel 1: alpha = 30 / max|x| of that channel;
    channel 2: alpha = 1.  Error in units of each channel's largest |ref|.  In place gives the same bits."""
    B, Cc = SNAKE_B, SNAKE_C
    g = _g(T)
    x = torch.randn(B, Cc, T, generator=g)
    x[:, 0] *= 1e6
    alpha = torch.tensor([1e-6, 30.0 / float(x[:, 1].abs().max()), 1.0])
    r64, r32 = _snake_fwd_ref(x, alpha, torch.float64), _snake_fwd_ref(x, alpha, torch.float32)
    x_d, a_d = x.to(cuda), alpha.to(cuda)
    y, ybuf, pad = _canary((B, Cc, T), cuda)
    _call("fac_snake_fwd", _p(x_d), _p(a_d), _p(y), B, Cc, T)
    z, zbuf, _ = _canary((B, Cc, T), cuda)
    z.copy_(x)
    _call("fac_snake_fwd", _p(z), _p(a_d), _p(z), B, Cc, T)
    torch.cuda.synchronize()
    assert _canary_intact(ybuf, pad) and _canary_intact(zbuf, pad)
    assert torch.equal(x_d.cpu(), x)
    _bar(f"snake_fwd_{_snake_branch(B, Cc, T)}_T{T}", y, r64, r32, scale=_chan_scale(r64))
    assert _same_bits(z, y.cpu())


def _gate_ref(a, g, dtype):
    """acts = tanh((a + g)[:, :C]) sigmoid((a + g)[:, C:]), g (B, 2C) broadcast over time or None."""
    a = a.to(dtype)
    if g is not None:
        a = a + g.to(dtype).unsqueeze(2)
    Cc = a.shape[1] // 2
    return torch.tanh(a[:, :Cc]) * _sigmoid(a[:, Cc:])


def _glu_ref(a, res, dtype):
    """out = res + a[:, :C] sigmoid(a[:, C:])."""
    a, res = a.to(dtype), res.to(dtype)
    Cc = a.shape[1] // 2
    return res + a[:, :Cc] * _sigmoid(a[:, Cc:])


@gpu
@pytest.mark.parametrize("B,Cc,T", [(1, 1, 1), (3, 5, 63)])
@pytest.mark.parametrize("cond", ["g_null", "g_dense_bs2C", "g_row_slice_bs_gt_2C"])
def test_gate_tanh_sigmoid_fp64(cuda, cond, B, Cc, T):
    """fac_gate_tanh_sigmoid with arguments over [-20, 20] (both ends present), without conditioning, with a dense (B, 2C)
    conditioning row and with a row slice of a wider tensor (batch stride 2C + 7, offset 3: the neighbours hold 1e3).  Relative
    error at every element: the product has no cancellation."""
    from facodec_amd import ops
    n = B * Cc * T
    a = _span(2 * n, n + len(cond), 20.0).view(B, 2 * Cc, T)
    g = g_d = None
    g_bs = 0
    if cond != "g_null":
        wide = torch.full((B, 2 * Cc + 7), 1e3)
        wide[:, 3:3 + 2 * Cc] = torch.randn(B, 2 * Cc, generator=_g(n)) * 0.5
        g = wide[:, 3:3 + 2 * Cc]
        g_d = g.to(cuda).clone(memory_format=torch.contiguous_format) if cond == "g_dense_bs2C" else wide.to(cuda)[:, 3:3 + 2 * Cc]
        g_bs = 2 * Cc if cond == "g_dense_bs2C" else 2 * Cc + 7
        assert B == 1 or g_d.stride(0) == g_bs
    r64, r32 = _gate_ref(a, g, torch.float64), _gate_ref(a, g, torch.float32)
    a_d = a.to(cuda)
    out, buf, pad = _canary((B, Cc, T), cuda)
    _call("fac_gate_tanh_sigmoid", _p(a_d), _p(g_d), g_bs, _p(out), B, Cc, T)
    out2 = ops.gate_tanh_sigmoid(a_d, g_d)
    torch.cuda.synchronize()
    assert _canary_intact(buf, pad) and torch.equal(a_d.cpu(), a)
    assert float(a.abs().max()) == 20.0
    _bar(f"gate_tanh_sigmoid_{cond}_{B}x{Cc}x{T}", out, r64, r32, scale=r64.abs().clamp_min(1e-300))
    assert _same_bits(out2, out.cpu())


@gpu
@pytest.mark.parametrize("B,Cc,T", [(1, 1, 1), (3, 5, 63)])
def test_glu_residual_fp64(cuda, B, Cc, T):
    """fac_glu_residual: out = res + a1 sigmoid(a2) with a over [-20, 20]; the value half a1 and the gate half a2 are independent,
    so swapped halves are O(1) wrong.  Scale: |res| + |a1| sigmoid(a2), the terms before they cancel."""
    from facodec_amd import ops
    n = B * Cc * T
    a = _span(2 * n, n, 20.0).view(B, 2 * Cc, T)
    res = torch.randn(B, Cc, T, generator=_g(n + 1))
    r64, r32 = _glu_ref(a, res, torch.float64), _glu_ref(a, res, torch.float32)
    a_d, res_d = a.to(cuda), res.to(cuda)
    out, buf, pad = _canary((B, Cc, T), cuda)
    _call("fac_glu_residual", _p(a_d), _p(res_d), _p(out), B, Cc, T)
    out2 = ops.glu_residual(a_d, res_d)
    torch.cuda.synchronize()
    assert _canary_intact(buf, pad) and torch.equal(a_d.cpu(), a) and torch.equal(res_d.cpu(), res)
    a6 = a.double()
    scale = res.double().abs() + a6[:, :Cc].abs() * _sigmoid(a6[:, Cc:])
    _bar(f"glu_residual_{B}x{Cc}x{T}", out, r64, r32, scale=scale.clamp_min(1e-300))
    assert _same_bits(out2, out.cpu())
    if n > 1:
        swapped = torch.cat([a[:, Cc:], a[:, :Cc]], 1)
        assert float((_glu_ref(swapped, res, torch.float64) - r64).abs().max()) > 1.0


AA_T = [1, 5, 255, 256, 257, 513]


@gpu
@pytest.mark.parametrize("T", AA_T, ids=[f"tiles{(T + 255) // 256}_T{T}" for T in AA_T])
def test_aa_snakebeta_fwd_fp64(cuda, T):
    """fac_aa_snakebeta_fwd (one workgroup per 256-column tile with a halo) against the fp64 restatement that
    test_aa_snakebeta_bwd_fp64 differentiates, at lengths below the 12-tap filter, at, below and above one tile, and two tiles
    and one column.  The bound holds over all elements; the error at the first / last 8 columns (replicate padding) and at the
    columns on either side of a tile edge is recorded separately."""
    B, Cc = 2, 3
    g = _g(T)
    x = torch.randn(B, Cc, T, generator=g)
    al, be = torch.randn(Cc, generator=g) * 0.5, torch.randn(Cc, generator=g) * 0.5
    filt = _kaiser_sinc_filter12()
    r64 = _aa_snakebeta_fwd_ref(x.double(), al.double(), be.double(), filt.double())
    r32 = _aa_snakebeta_fwd_ref(x, al, be, filt)
    x_d, al_d, be_d, f_d = (t.to(cuda) for t in (x, al, be, filt))
    y, buf, pad = _canary((B, Cc, T), cuda)
    _call("fac_aa_snakebeta_fwd", _p(x_d), _p(al_d), _p(be_d), _p(f_d), _p(y), B, Cc, T)
    torch.cuda.synchronize()
    assert _canary_intact(buf, pad) and torch.equal(x_d.cpu(), x)
    yc = y.cpu()
    mag = float(r64.abs().max())
    e = min(8, T)
    parts = {"head8": list(range(e)), "tail8": list(range(T - e, T)),
             "tile_edge": [t for t in range(T) if t % 256 in (254, 255, 0, 1) and t > 1]}
    for nm, cols in parts.items():
        if cols:
            e_gpu = float((yc[..., cols].double() - r64[..., cols]).abs().max()) / mag
            e_cpu = float((r32[..., cols].double() - r64[..., cols]).abs().max()) / mag
            _record(f"aa_snakebeta_fwd_{nm}_T{T}", {"gpu": e_gpu, "fp32_cpu": e_cpu})
            print(f"[tol] aa_snakebeta_fwd_{nm}_T{T}: gpu {e_gpu:.3e} fp32-cpu {e_cpu:.3e}")
    _bar(f"aa_snakebeta_fwd_T{T}", yc, r64, r32)


def _attn_stages_v(dk, T):
    """fac_attention's staging decision (misc.hip), restated: queries (dk x 16), scores (16 x T) and 16 rows of V (T + 1 each) in
    160 KiB of LDS."""
    return (16 * dk + 16 * T + 16 * (T + 1)) * 4 <= 160 * 1024


# (dk, T, B, stages V through LDS)
ATTN_CASES = [(256, 1, 2, True), (256, 15, 2, True), (256, 16, 2, True), (256, 17, 2, True), (24, 70, 2, True),
              (256, 1151, 1, True), (256, 1152, 1, False)]
ATTN_PARAMS = [(c, m) for c in ATTN_CASES for m in ("mask_null", "partial_mask", "clip_fully_masked") if c[1] > 1 or m != "partial_mask"]


def _attn_id(case, mask_kind):
    dk, T, B, staged = case
    return f"{'stage_v_lds' if staged else 'v_in_place'}_dk{dk}_T{T}_B{B}_{mask_kind}"


@gpu
@pytest.mark.parametrize("case,mask_kind", ATTN_PARAMS, ids=[_attn_id(c, m) for c, m in ATTN_PARAMS])
def test_attention_fused_fp64(cuda, case, mask_kind):
    """fac_attention (H = 2) against float64 softmax attention: T below, at and above one 16-query tile, dk = 24 (the second pass
    over V is half filled), the longest T that stages V through LDS and the first that does not.  A masked pair scores -1e4
    (masked_fill, as the reference); a fully masked clip -- and every masked query of a partly masked one -- therefore has uniform
    weights, and its output is the mean of V over ALL keys: held also as a T-term sum.  Bound and scale as
    test_attention_kernels_fp64 (units of the largest |ref|)."""
    dk, T, B, staged = case
    H = 2
    assert _attn_stages_v(dk, T) == staged
    g = _g(dk + T + len(mask_kind))
    q, k, v = (torch.randn(B, H * dk, T, generator=g) for _ in range(3))
    mask = None
    if mask_kind != "mask_null":
        mask = torch.ones(B, T)
        mask[-1, T - min(17, T // 2):] = 0
        if mask_kind == "clip_fully_masked":
            mask[0] = 0
    o64 = _attn_ref(q.double(), k.double(), v.double(), mask.double() if mask is not None else None, B, H, dk, T)[0]
    o32 = _attn_ref(q, k, v, mask, B, H, dk, T)[0]
    q_d, k_d, v_d = q.to(cuda), k.to(cuda), v.to(cuda)
    m_d = mask.to(cuda) if mask is not None else None
    out, buf, pad = _canary((B, H * dk, T), cuda)
    _call("fac_attention", _p(q_d), _p(k_d), _p(v_d), _p(m_d), _p(out), B, H, dk, T)
    torch.cuda.synchronize()
    assert _canary_intact(buf, pad)
    assert all(torch.equal(a.cpu(), b) for a, b in ((q_d, q), (k_d, k), (v_d, v)))
    fails = []
    tag = _attn_id(case, mask_kind)
    _collect(fails, _bar, f"attention_fused_{tag}", out, o64, o32)
    if mask_kind == "clip_fully_masked":
        # weights exp(0) / T: the sum T is exact, 1 / T and each product are rounded once (extra = 2), T terms v / T
        v6 = v[0].double()
        _collect(fails, _sum_bound, f"attention_fused_uniform_{tag}", out[0], v6.mean(-1, keepdim=True).expand(H * dk, T),
                 (v6.abs().sum(-1, keepdim=True) / T).expand(H * dk, T), T, extra=2.0)
    assert not fails, fails


# ======================================================================================================= 3. housekeeping (no GPU)
ENTRY_POINTS = ["fac_add", "fac_sub2", "fac_mul_mask", "fac_wn_res_skip", "fac_embed_sum", "fac_stream_push", "fac_lstm_to_time_major",
                "fac_lstm_from_time_major", "fac_to_p8", "fac_mask_tail", "fac_mask_tail_i64", "fac_frame_mask",
                "fac_stft_frames_ragged", "fac_snake_fwd", "fac_gate_tanh_sigmoid", "fac_glu_residual", "fac_aa_snakebeta_fwd",
                "fac_attention"]


def test_entry_points_of_this_file_are_declared():
    """Every C entry this file drives is declared in include/facodec_hip.h and bound in facodec_amd/_lib.py with a stream as its
    last argument, and every one of them is driven by a test here (runs without a GPU)."""
    header = open(os.path.join(REPO, "include", "facodec_hip.h")).read()
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "fac_adamw_step" in v)
    this = open(os.path.abspath(__file__)).read()
    for n in ENTRY_POINTS:
        assert n in table, n
        assert f"int {n}(" in header, n
        assert table[n][1][-1] is C.c_void_p, n
    called = {w.split(chr(34))[0] for w in this.split("_ca" + "ll(" + chr(34))[1:]}
    assert called | {"fac_mask_tail_i64"} == set(ENTRY_POINTS), called ^ set(ENTRY_POINTS)      # the _i64 form: second arm of one call


def test_dispatch_restatements_match_the_source():
    """The dispatch conditions restated above, word for word in misc.hip; the cases reach both sides of each."""
    src = open(os.path.join(REPO, "facodec_amd", "csrc", "misc.hip")).read()
    assert "if (T >= 1024 && (long long)B * C <= 65535) {" in src
    assert {_snake_branch(SNAKE_B, SNAKE_C, T) for T in SNAKE_T} == {"flat", "rows"}
    assert _snake_branch(1, 65536, 1024) == "flat" and _snake_branch(SNAKE_B, SNAKE_C, 1023) == "flat"
    assert "size_t lds = ((size_t)dk * 16 + (size_t)16 * T) * sizeof(float);" in src
    assert "const size_t lds_v = lds + (size_t)16 * (T + 1) * sizeof(float);" in src
    assert "const int stage_v = lds_v <= FAC_LDS_MAX ? 1 : 0;" in src
    assert "constexpr size_t FAC_LDS_MAX = 160 * 1024;" in open(os.path.join(REPO, "facodec_amd", "csrc", "common.h")).read()
    assert _attn_stages_v(256, 1151) and not _attn_stages_v(256, 1152)
    assert {c[3] for c in ATTN_CASES} == {True, False} and all(_attn_stages_v(c[0], c[1]) == c[3] for c in ATTN_CASES)
    assert "if (g > 8192) g = 8192;" in src and max(EW_N) > 8192 * 256
    assert "constexpr int TT = 256;" in src and {(T + 255) // 256 for T in AA_T} == {1, 2, 3}


def test_references_against_the_oracle():
    """Every restatement this file holds a kernel against, checked on the CPU in float64 against the project's oracle
    (oracle/facodec_oracle.py) where it has the operation, before a GPU sees it."""
    from oracle import facodec_oracle as O
    F = torch.nn.functional
    g = _g(7)
    d = torch.float64
    # Snake
    x, alpha = torch.randn(2, 3, 50, generator=g, dtype=d), torch.rand(3, generator=g, dtype=d) + 0.1
    assert torch.allclose(_snake_fwd_ref(x, alpha, d), O.snake(x, alpha.view(1, -1, 1)), rtol=1e-13, atol=1e-13)
    # the gate, inside O.wavenet_forward: one layer whose skip conv is the identity returns the gate of in_layer(x) + cond(g)
    h, gin, B, T = 4, 3, 2, 9
    sd = {"in_layers.0.conv.conv.weight": torch.randn(2 * h, h, 1, generator=g, dtype=d),
          "in_layers.0.conv.conv.bias": torch.randn(2 * h, generator=g, dtype=d),
          "res_skip_layers.0.conv.conv.weight": torch.eye(h, dtype=d).unsqueeze(2),
          "res_skip_layers.0.conv.conv.bias": torch.zeros(h, dtype=d),
          "cond_layer.conv.conv.weight": torch.randn(2 * h, gin, 1, generator=g, dtype=d),
          "cond_layer.conv.conv.bias": torch.randn(2 * h, generator=g, dtype=d)}
    xx, gg = torch.randn(B, h, T, generator=g, dtype=d), torch.randn(B, gin, 1, generator=g, dtype=d)
    a = F.conv1d(xx, sd["in_layers.0.conv.conv.weight"], sd["in_layers.0.conv.conv.bias"])
    rows = F.conv1d(gg, sd["cond_layer.conv.conv.weight"], sd["cond_layer.conv.conv.bias"])[:, :, 0]
    assert torch.allclose(_gate_ref(a, rows, d), O.wavenet_forward(xx, sd, "", h, 1, kernel_size=1, g=gg), rtol=1e-12, atol=1e-13)
    assert torch.allclose(_gate_ref(a, None, d), O.wavenet_forward(xx, sd, "", h, 1, kernel_size=1), rtol=1e-12, atol=1e-13)
    # the WaveNet skip of the same function: x + rs[:, :h] feeds the next layer, out collects rs[:, h:] and the last layer's rs
    # GLU: the oracle has it as an expression of style_encoder_forward (Conv1dGLU), the same as torch's own F.glu
    assert "x = x + a[:, :half] * torch.sigmoid(a[:, half:])" in inspect.getsource(O.style_encoder_forward)
    a2, res = torch.randn(2, 8, 5, generator=g, dtype=d), torch.randn(2, 4, 5, generator=g, dtype=d)
    assert torch.allclose(_glu_ref(a2, res, d), res + F.glu(a2, 1), rtol=1e-13, atol=1e-13)
    # STFT framing: the gather with the whole row as the clip, windowed and transformed, is O.stft_complex (torch.stft, centre,
    # reflect); and a ragged row is the gather of its own slice
    n_fft, hop, T = 16, 4, 50
    w = torch.randn(3, T, generator=g, dtype=d)
    nf = T // hop                                                # the T / hop frames the product keeps of torch.stft's 1 + T / hop
    fr = _frames_ref(w, [T] * 3, n_fft, nf, hop, n_fft // 2, 0)
    spec = torch.fft.rfft(fr * O.hann_periodic(n_fft).double().view(1, -1, 1), dim=1)
    assert torch.allclose(spec, O.stft_complex(w, n_fft, hop)[..., :nf], rtol=1e-12, atol=1e-12)
    lens = [T, 33, 21]
    rag = _frames_ref(w, lens, n_fft, T // hop, hop, n_fft // 2, 0)
    for b, L in enumerate(lens):
        own = _frames_ref(w[b:b + 1, :L], [L], n_fft, L // hop, hop, n_fft // 2, 0)
        assert torch.equal(rag[b:b + 1, :, :L // hop], own) and not bool(rag[b, :, L // hop:].any())
        ref = torch.fft.rfft(own * O.hann_periodic(n_fft).double().view(1, -1, 1), dim=1)
        assert torch.allclose(ref, O.stft_complex(w[b:b + 1, :L], n_fft, hop)[..., :L // hop], rtol=1e-12, atol=1e-12)
    # anti-aliased SnakeBeta
    filt = _kaiser_sinc_filter12().double()
    for T in (1, 5, 40):
        x = torch.randn(2, 3, T, generator=g, dtype=d)
        al, be = torch.randn(3, generator=g, dtype=d), torch.randn(3, generator=g, dtype=d)
        assert torch.allclose(_aa_snakebeta_fwd_ref(x, al, be, filt), O.aa_snakebeta(x, al, be, filt.view(1, 1, 12)), rtol=1e-12,
                              atol=1e-13)
    # attention: O.style_attention with an identity output conv
    Cc, T, H = 8, 7, 2
    sd = {f"conv_{n}.weight": torch.randn(Cc, Cc, 1, generator=g, dtype=d) for n in "qkv"}
    sd.update({f"conv_{n}.bias": torch.randn(Cc, generator=g, dtype=d) for n in "qkv"})
    sd.update({"conv_o.weight": torch.eye(Cc, dtype=d).unsqueeze(2), "conv_o.bias": torch.zeros(Cc, dtype=d)})
    x = torch.randn(2, Cc, T, generator=g, dtype=d)
    q, k, v = (F.conv1d(x, sd[f"conv_{n}.weight"], sd[f"conv_{n}.bias"]) for n in "qkv")
    mask = torch.ones(2, T, dtype=d)
    mask[0, 4:] = 0
    mask[1] = 0
    m4 = (mask.unsqueeze(1) * mask.unsqueeze(2)).unsqueeze(1)
    assert torch.allclose(_attn_ref(q, k, v, mask, 2, H, Cc // H, T)[0], O.style_attention(x, sd, "", H, m4), rtol=1e-12, atol=1e-13)
    assert torch.allclose(_attn_ref(q, k, v, None, 2, H, Cc // H, T)[0], O.style_attention(x, sd, "", H), rtol=1e-12, atol=1e-13)
    # the three-way bfloat16 split: the planes add up to the value exactly, and ties go to the even neighbour
    x = _p8_input(2, 24, 37, 1)
    planes = _p8_ref(x)
    assert planes.shape == (3, 2 * 3 * 37 + 1, 8) and not bool(planes[:, -1].any())
    back = planes[:, :-1].float().sum(0).view(2, 3, 37, 8).permute(0, 1, 3, 2).reshape(2, 24, 37)
    assert torch.equal(back, x)
    e = _p8_ref(torch.tensor(P8_EDGES).view(1, 8, 1))[:, 0].float()
    assert e[0].tolist()[:6] == [0.0, -0.0, 1.0, -1.0, 1 + 2.0 ** -6, 1.0]
    assert _bits(e[0])[1] == torch.iinfo(torch.int32).min                  # -0 stays -0 in the hi plane
    assert e[1].tolist()[2:6] == [2.0 ** -8, -(2.0 ** -8), -(2.0 ** -8), 2.0 ** -9]
    assert e[2].tolist()[5] == 2.0 ** -17
    # the embedding sum, inside O.redecoder_forward's first lines: F.embedding rows added in table order
    codes, tables = torch.randint(0, 7, (2, 3, 5), generator=g), torch.randn(3, 7, 4, generator=g)
    want = torch.zeros(2, 5, 4)
    for i in range(3):
        want = want + F.embedding(codes[:, i, :], tables[i])
    assert torch.equal(_embed_ref(codes, tables, 3, 0, None), want.transpose(1, 2))
