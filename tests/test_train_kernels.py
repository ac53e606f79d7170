"""The training path's glue kernels one at a time against fp64: the discriminator's data-movement and activation kernels
(train_disc.hip), the spectral losses' framing / power / reduction kernels and the channel LayerNorm (misc.hip, conv1d_bwd.hip),
cross entropy and the crop (train_misc.hip), the in-place reflect fold (conv1d_bwd.hip) and the k = 1 / taps weight gradient's
alignment guard (conv1d_wgrad_k1.hip).

Each reference is a plain float64 restatement of the documented semantics (kernel comments, oracle/facodec_oracle.py) computed
from the same fp32 inputs.  Pure copies and gathers must match bit for bit, with canaries around the output; their adjoints
(scatter-adds) are checked against fp64 and through <fwd(x), y> = <x, bwd(y)>.  Reductions answer to a bound that grows like
sqrt(n) * 2^-24 * sum|terms| rather than to a fixed number.  Shapes are chosen to reach every dispatch branch and the edges where
index arithmetic goes wrong (reflections, pad / gap columns, separator rows, grid-stride tails)."""
import ctypes as C
import math

import pytest
import torch

from facodec_amd import _lib

gpu = pytest.mark.gpu
EPS32 = 2.0 ** -24
CANARY = 12345.0


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _p(t):
    """Raw pointer for a C entry.  Callers keep the tensor in a variable until the launch is enqueued: a freed temporary's block
    can go to the next allocation (and its host-to-device copy) first."""
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _call(name, *args):
    from facodec_amd import ops
    _lib.check(getattr(_lib.load(), name)(*args, ops._stream()), name)


def _canary(shape, dev, pad=64):
    """An output tensor that sits inside a canary-filled buffer: (view, buffer, pad).  pad = 64 floats keeps the view
    16-byte aligned (the buffer's base is)."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * pad,), CANARY, device=dev)
    return buf[pad:pad + n].view(*shape), buf, pad


def _canary_intact(buf, pad):
    c = buf.cpu()
    return bool((c[:pad] == CANARY).all()) and bool((c[-pad:] == CANARY).all())


def _gather_ref(x, idx):
    """out[i] = x[idx[i]] (idx < 0: zero) -- the fp64 reference of every gather kernel; returns the forward on x's dtype."""
    xf = x.reshape(-1)
    return torch.where(idx >= 0, xf[idx.clamp_min(0)], torch.zeros((), dtype=x.dtype))


def _scatter_ref(dout, idx, n):
    """The adjoint of _gather_ref in fp64: dx[j] = sum of dout[i] over idx[i] == j."""
    d = dout.reshape(-1).double()
    keep = idx >= 0
    return torch.zeros(n, dtype=torch.float64).index_add_(0, idx[keep], d[keep])


def _check_adjoint(x, fwd_out, y, bwd_out):
    """<fwd(x), y> == <x, bwd(y)> in fp64 (fwd exact; bwd sums at most a few fp32 terms per element)."""
    fwd_out, y, x, bwd_out = (t.detach().double().cpu().reshape(-1) for t in (fwd_out, y, x, bwd_out))
    lhs = float((fwd_out * y).sum())
    rhs = float((x * bwd_out).sum())
    mag = float((x.abs() * bwd_out.abs()).sum())
    assert abs(lhs - rhs) <= 8 * EPS32 * mag, (lhs, rhs, mag)


def _max_rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------------- fac_leaky_relu
def _leaky_mask(n, T, pitch, valid, rpg, vrows):
    if pitch == 0:
        return torch.ones(n, dtype=torch.bool)
    pos = torch.arange(n) % T
    row = pos // pitch
    ok = (pos - row * pitch) < valid
    if rpg:
        ok &= (row % rpg) < vrows
    return ok


def _leaky_branch(n, T, pitch, ptrs):
    """The dispatch of fac_leaky_relu (train_disc.hip), restated: which kernel a launch takes."""
    aligned = all(p % 16 == 0 for p in ptrs)
    if n % 4 == 0 and (pitch == 0 or (T % 4 == 0 and pitch % 4 == 0)) and aligned:
        return "quad"
    if pitch != 0 and n % 4 == 0 and aligned:
        return "quad_any"
    return "scalar"


# (case id, rows, T, pitch, valid, rows_per_group, valid_rows, misaligned view); the id names the branch the case reaches
LEAKY_CASES = [
    ("quad_pitch0", 6, 1000, 0, 0, 0, 0, False),
    ("scalar_pitch0_odd_n", 3, 1001, 0, 0, 0, 0, False),
    ("quad_full_valid", 4, 96, 12, 12, 0, 0, False),
    ("quad_valid_lt_pitch", 4, 96, 12, 9, 0, 0, False),
    ("quad_partial_last_row", 3, 100, 16, 13, 0, 0, False),       # T not a multiple of the pitch: a short last row
    ("quad_row_groups", 3, 8 * 10, 8, 6, 5, 3, False),            # rows 3, 4 of every group of 5 are separators
    ("quad_any_valid_lt_pitch", 4, 42, 7, 5, 0, 0, False),        # pitch 7: quads straddle rows
    ("quad_any_row_groups", 2, 7 * 8, 7, 5, 4, 3, False),
    ("quad_any_odd_T", 4, 45, 9, 9, 0, 0, False),                 # T % 4 != 0, n % 4 == 0: quads straddle rows of T
    ("quad_any_row_groups_wrap", 4, 7 * 9, 7, 6, 4, 2, False),    # T not a multiple of rpg * pitch
    ("scalar_odd_n", 3, 42, 7, 5, 0, 0, False),
    ("scalar_odd_n_row_groups", 3, 7 * 9, 7, 6, 4, 3, False),
    ("scalar_misaligned_quad_shape", 4, 96, 12, 9, 0, 0, True),   # would be quad, but buf[1:1+n] is not 16-byte aligned
    ("scalar_misaligned_pitch0", 4, 1000, 0, 0, 0, 0, True),
    ("scalar_misaligned_quad_any_shape", 4, 42, 7, 5, 0, 0, True),
    ("scalar_grid_stride_tail", 1, 65535 * 256 + 4099, 13, 11, 0, 0, False),   # past the 65535-block cap
]


@gpu
@pytest.mark.parametrize("backward", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("case", LEAKY_CASES, ids=[c[0] for c in LEAKY_CASES])
def test_leaky_relu_branch_bit_exact(cuda, case, backward):
    name, rows, T, pitch, valid, rpg, vrows, misaligned = case
    n = rows * T
    slope = 0.1
    g = _g(LEAKY_CASES.index(case))
    x = torch.randn(n, generator=g)
    x[::17] = 0.0                                           # exact zeros take the negative side (x > 0 is false)
    dy = torch.randn(n, generator=g)
    off = 1 if misaligned else 0
    xb = torch.zeros(n + 8, device=cuda)
    xb[off:off + n] = x.to(cuda)
    dyb = torch.zeros(n + 8, device=cuda)
    dyb[off:off + n] = dy.to(cuda)
    xd, dyd = xb[off:off + n], dyb[off:off + n]
    out, buf, pad = _canary((n + 4,), cuda)                # the kernel writes the first n; the last 4 and both pads stay
    outd = out[off:off + n] if misaligned else out[:n]
    ptrs = [xd.data_ptr(), outd.data_ptr()] + ([dyd.data_ptr()] if backward else [])
    want = "quad_any" if name.startswith("quad_any") else name.split("_")[0]
    assert _leaky_branch(n, T, pitch, ptrs) == want, name
    _call("fac_leaky_relu", _p(xd), _p(dyd if backward else None), _p(outd), n, C.c_float(slope), T, pitch, valid, rpg, vrows)
    torch.cuda.synchronize()
    ok = _leaky_mask(n, T, pitch, valid, rpg, vrows)
    src = dy if backward else x
    ref = torch.where(ok, torch.where(x > 0, src, src * torch.tensor(slope, dtype=torch.float32)), torch.zeros(()))
    assert torch.equal(outd.cpu(), ref)
    assert _canary_intact(buf, pad)
    rest = out.cpu()[n:] if not misaligned else torch.cat([out.cpu()[:1], out.cpu()[n + 1:]])
    assert bool((rest == CANARY).all())


# ------------------------------------------------------------------------------------------------------- period_fold
def _period_fold_idx(B, T, p, L, pitch):
    i = torch.arange(B * p * pitch)
    l, r = i % pitch, i // pitch
    j, b = r % p, r // p
    s = l * p + j
    s = torch.where(s >= T, 2 * (T - 1) - s, s)
    return torch.where(l < L, b * T + s, torch.full_like(s, -1))


# (T, period, L, pitch): the model's L = T // p + 1 (oracle mpd_forward pads a FULL period when p divides T), and the extreme
# L * p == 2T - 1 (the last folded sample reflects onto x[0])
FOLD_CASES = [(2310, 2, 1156, 1160), (2310, 11, 211, 211), (24000, 7, 3429, 3432), (1001, 5, 201, 205), (5, 3, 3, 4), (5, 9, 1, 3),
              (8, 5, 3, 7)]


@gpu
@pytest.mark.parametrize("T,p,L,pitch", FOLD_CASES)
def test_period_fold_and_adjoint(cuda, T, p, L, pitch):
    B = 3
    if T % p == 0:
        assert L * p == T + p                               # the full-period pad of the reference
    assert T <= L * p <= 2 * T - 1
    g = _g(T + p)
    x = torch.randn(B, T, generator=g)
    idx = _period_fold_idx(B, T, p, L, pitch)
    out, buf, pad = _canary((B * p * pitch,), cuda)
    x_d = x.to(cuda)
    _call("fac_period_fold", _p(x_d), _p(out), B, T, p, L, pitch, 0)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), _gather_ref(x, idx)) and _canary_intact(buf, pad)
    assert bool((out.cpu().view(B * p, pitch)[:, L:] == 0).all())
    dout = torch.randn(B * p * pitch, generator=g)
    dx, buf2, pad2 = _canary((B * T,), cuda)
    dout_d = dout.to(cuda)
    _call("fac_period_fold", _p(dout_d), _p(dx), B, T, p, L, pitch, 1)
    torch.cuda.synchronize()
    ref = _scatter_ref(dout, idx, B * T)
    assert _canary_intact(buf2, pad2)
    assert float((dx.cpu().double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    _check_adjoint(x, out.cpu(), dout, dx.cpu())


# ------------------------------------------------------------------------------------------------------- pad_reflect
@gpu
@pytest.mark.parametrize("T,pl,pr", [(2, 1, 1), (5, 4, 4), (100, 0, 37), (100, 37, 0), (24000, 768, 1279), (1500, 768, 804)])
def test_pad_reflect_exact(cuda, T, pl, pr):
    B = 2
    x = torch.randn(B, T, generator=_g(T))
    Tp = T + pl + pr
    u = torch.arange(B * Tp)
    s = (u % Tp) - pl
    s = torch.where(s < 0, -s, s)
    s = torch.where(s >= T, 2 * (T - 1) - s, s)
    idx = (u // Tp) * T + s
    out, buf, pad = _canary((B * Tp,), cuda)
    x_d = x.to(cuda)
    _call("fac_pad_reflect", _p(x_d), _p(out), B, T, pl, pr)
    torch.cuda.synchronize()
    ref = torch.nn.functional.pad(x.unsqueeze(1), (pl, pr), mode="reflect").reshape(-1)
    assert torch.equal(_gather_ref(x, idx), ref)
    assert torch.equal(out.cpu(), ref) and _canary_intact(buf, pad)


# ------------------------------------------------------------------------------------------------------- zero_insert
@gpu
@pytest.mark.parametrize("rows,T,stride", [(5, 1, 3), (7, 33, 2), (3, 1000, 5), (2, 4097, 4)])
def test_zero_insert_exact(cuda, rows, T, stride):
    dy = torch.randn(rows, T, generator=_g(T * stride))
    Tu = (T - 1) * stride + 1
    out, buf, pad = _canary((rows * Tu,), cuda)
    dy_d = dy.to(cuda)
    _call("fac_zero_insert", _p(dy_d), _p(out), rows, T, stride)
    torch.cuda.synchronize()
    ref = torch.zeros(rows, Tu)
    ref[:, ::stride] = dy
    assert torch.equal(out.cpu().view(rows, Tu), ref) and _canary_intact(buf, pad)


# ------------------------------------------------------------------------------------------------------- row_stack3
def _row_stack3_idx(rows, T, Cc, F):
    cf = Cc * F
    i = torch.arange(rows * 3 * cf)
    row, r = i // (3 * cf), i % (3 * cf)
    dt, rest = r // cf, r % cf
    t = row % T + dt - 1
    return torch.where((t >= 0) & (t < T), (row + dt - 1) * cf + rest, torch.full_like(i, -1))


@gpu
@pytest.mark.parametrize("B,T,Cc,F", [(1, 1, 2, 5), (2, 3, 2, 9), (3, 17, 5, 13), (2, 40, 32, 33)])
def test_row_stack3_and_adjoint(cuda, B, T, Cc, F):
    rows = B * T
    g = _g(rows * F)
    x = torch.randn(rows * Cc * F, generator=g)
    idx = _row_stack3_idx(rows, T, Cc, F)
    out, buf, pad = _canary((rows * 3 * Cc * F,), cuda)
    x_d = x.to(cuda)
    _call("fac_row_stack3", _p(x_d), _p(out), rows, T, Cc, F, 0)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), _gather_ref(x, idx)) and _canary_intact(buf, pad)
    d = torch.randn(rows * 3 * Cc * F, generator=g)
    dx, buf2, pad2 = _canary((rows * Cc * F,), cuda)
    d_d = d.to(cuda)
    _call("fac_row_stack3", _p(d_d), _p(dx), rows, T, Cc, F, 1)
    torch.cuda.synchronize()
    ref = _scatter_ref(d, idx, rows * Cc * F)
    assert _canary_intact(buf2, pad2)
    assert float((dx.cpu().double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    _check_adjoint(x, out.cpu(), d, dx.cpu())


# ------------------------------------------------------------------------------------------------------- spec_to_rows / spec_to_cat
def _spec_src(B, Ft, T, f0, Fb):
    """Flat index into spec (B, 2 Ft, T) of band element (b, t, c, f)."""
    b = torch.arange(B).view(B, 1, 1, 1)
    t = torch.arange(T).view(1, T, 1, 1)
    c = torch.arange(2).view(1, 1, 2, 1)
    f = torch.arange(Fb).view(1, 1, 1, Fb)
    return (b * 2 * Ft + c * Ft + f0 + f) * T + t          # (B, T, 2, Fb)


SPEC_CASES = [(1, 5, 1, 0, 5), (2, 1025, 7, 0, 102), (2, 1025, 7, 768, 257), (3, 257, 12, 25, 39), (2, 513, 4, 512, 1)]


@gpu
@pytest.mark.parametrize("B,Ft,T,f0,Fb", SPEC_CASES)
def test_spec_to_rows_and_adjoint(cuda, B, Ft, T, f0, Fb):
    g = _g(Ft + f0)
    spec = torch.randn(B * 2 * Ft * T, generator=g)
    idx = _spec_src(B, Ft, T, f0, Fb).reshape(-1)           # rows[(b T + t)][c][f]
    out, buf, pad = _canary((idx.numel(),), cuda)
    spec_d = spec.to(cuda)
    _call("fac_spec_to_rows", _p(spec_d), _p(out), B, Ft, T, f0, Fb, 0)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), _gather_ref(spec, idx)) and _canary_intact(buf, pad)
    d = torch.randn(idx.numel(), generator=g)
    dspec, buf2, pad2 = _canary((spec.numel(),), cuda)      # outside the band: untouched (the caller zero-fills)
    d_d = d.to(cuda)
    _call("fac_spec_to_rows", _p(d_d), _p(dspec), B, Ft, T, f0, Fb, 1)
    torch.cuda.synchronize()
    ref = torch.full((spec.numel(),), CANARY)
    ref[idx] = d
    assert torch.equal(dspec.cpu(), ref) and _canary_intact(buf2, pad2)


@gpu
@pytest.mark.parametrize("B,Ft,T,f0,Fb", SPEC_CASES)
@pytest.mark.parametrize("gap", [0, 3])
def test_spec_to_cat_and_adjoint(cuda, B, Ft, T, f0, Fb, gap):
    pitch = Fb + gap
    g = _g(Ft + f0 + gap)
    spec = torch.randn(B * 2 * Ft * T, generator=g)
    src = _spec_src(B, Ft, T, f0, Fb)                       # (B, T, 2, Fb)
    idx = torch.full((2, B, T + 1, pitch), -1, dtype=torch.long)
    idx[:, :, :T, :Fb] = src.permute(2, 0, 1, 3)
    idx = idx.reshape(-1)                                   # cat[c][(b (T+1) + t) pitch + f]; gap columns, separator row: -1
    out, buf, pad = _canary((idx.numel(),), cuda)
    spec_d = spec.to(cuda)
    _call("fac_spec_to_cat", _p(spec_d), _p(out), B, Ft, T, f0, Fb, pitch, 0)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), _gather_ref(spec, idx)) and _canary_intact(buf, pad)
    d = torch.randn(idx.numel(), generator=g)
    dspec, buf2, pad2 = _canary((spec.numel(),), cuda)
    d_d = d.to(cuda)
    _call("fac_spec_to_cat", _p(d_d), _p(dspec), B, Ft, T, f0, Fb, pitch, 1)
    torch.cuda.synchronize()
    ref = torch.full((spec.numel(),), CANARY)
    keep = idx >= 0
    ref[idx[keep]] = d[keep]
    assert torch.equal(dspec.cpu(), ref) and _canary_intact(buf2, pad2)


# ------------------------------------------------------------------------------------------------------- stft_frames (+ bwd)
def _stft_idx(B, T, n_win, nf, hop, pad, n_off):
    i = torch.arange(B * n_win * nf)
    b, r = i // (n_win * nf), i % (n_win * nf)
    nn, f = r // nf, r % nf
    t = f * hop + nn + n_off - pad
    t = torch.where(t < 0, -t, t)
    t = torch.where(t >= T, 2 * (T - 1) - t, t)
    return torch.where((t >= 0) & (t < T), b * T + t, torch.full_like(t, -1))


# (T, n_win, n_frames, hop, pad, n_off): n_off = 0 (window == n_fft) and (n_fft - win) // 2 (the reconstruction losses' short
# windows centred in a 512-point frame); T just above the pad; frame counts whose last frames reach past 2 (T - 1) (zeros)
STFT_CASES = [(33, 64, 3, 16, 32, 0), (257, 64, 40, 16, 256, 224), (300, 512, 8, 128, 256, 0), (1000, 64, 70, 16, 256, 224),
              (24000, 2048, 48, 512, 1024, 0), (4001, 128, 260, 32, 256, 192), (2, 4, 5, 1, 1, 0)]


@gpu
@pytest.mark.parametrize("T,n_win,nf,hop,pad,n_off", STFT_CASES)
def test_stft_frames_and_adjoint(cuda, T, n_win, nf, hop, pad, n_off):
    from facodec_amd import ops
    B = 2
    g = _g(T + n_win)
    wave = torch.randn(B, T, generator=g)
    idx = _stft_idx(B, T, n_win, nf, hop, pad, n_off)
    fr = ops.stft_frames(wave.to(cuda), n_win, nf, hop, pad, n_off)
    torch.cuda.synchronize()
    assert torch.equal(fr.cpu().reshape(-1), _gather_ref(wave, idx))
    # the index table itself against torch: reflect-pad by `pad`, then frames of n_win every hop from n_off on (torch.stft's
    # centre framing) -- every frame that lies inside the padded signal (past it the kernel reads zeros, which torch cannot pad)
    nfit = sum(1 for f in range(nf) if f * hop + n_off + n_win <= T + 2 * pad)
    assert nfit >= 1
    xp = torch.nn.functional.pad(wave.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    tref = xp[:, n_off:].unfold(1, n_win, hop)[:, :nfit].transpose(1, 2)         # (B, n_win, nfit)
    assert torch.equal(_gather_ref(wave, idx).view(B, n_win, nf)[:, :, :nfit], tref)
    dfr = torch.randn(B, n_win, nf, generator=g)
    dw = ops.stft_frames_bwd(dfr.to(cuda), T, hop, pad, n_off)
    torch.cuda.synchronize()
    ref = _scatter_ref(dfr, idx, B * T).view(B, T)
    mag = _scatter_ref(dfr.abs(), idx, B * T).view(B, T)
    # each sample sums at most ceil(n_win / hop) * 3 fp32 terms
    k = 3 * ((n_win + hop - 1) // hop)
    assert bool(((dw.cpu().double() - ref).abs() <= k * EPS32 * mag).all())
    _check_adjoint(wave, fr.cpu(), dfr, dw.cpu())
    if (nf - 1) * hop + n_win - 1 + n_off - pad > 2 * (T - 1):
        assert bool((idx.view(B, n_win, nf)[:, -1, -1] < 0).all())     # the case reaches the zero tail


# ------------------------------------------------------------------------------------------------------- reductions
def _pair_terms64(a, b, mode, eps):
    a, b = a.double(), b.double()
    if mode == 1:
        la, lb = torch.log10(a.clamp_min(eps)), torch.log10(b.clamp_min(eps))
        return (la - lb).abs(), la.abs() + lb.abs() + 1    # (term, the magnitude its fp32 evaluation rounds against)
    d = a - b
    if mode == 0:
        t = d.abs()
    elif mode == 2:
        t = d * d
    else:
        t = torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5)
    return t, t.abs() + d.abs()


def _pair_inputs(n, seed):
    g = _g(seed)
    a = torch.rand(n, generator=g) * 3 + 1e-7
    b = torch.rand(n, generator=g) * 3 + 1e-7
    b[::7] = a[::7]                                         # ties
    a[::11] = 1e-6                                          # below eps (mode 1 clamps)
    return a, b


@gpu
@pytest.mark.parametrize("n", [1, 257, 256 * 1024 + 40001], ids=["n1", "n257", "grid_stride"])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
def test_reduce_pair_against_fp64(cuda, n, mode, accumulate):
    from facodec_amd import ops
    a, b = _pair_inputs(n, 100 + mode)
    eps, scale = 1e-5, 0.37
    out = torch.tensor([2.5], device=cuda)
    scratch = torch.empty(1024, device=cuda)
    ops.reduce_pair(a.to(cuda), b.to(cuda), out, scratch, mode, eps, scale, accumulate)
    torch.cuda.synchronize()
    t, mag = _pair_terms64(a, b, mode, eps)
    ref = scale * float(t.sum()) + (2.5 if accumulate else 0.0)
    bound = 4 * math.sqrt(n) * EPS32 * scale * float(mag.sum()) + (4 * EPS32 * 2.5 if accumulate else 0.0)
    assert abs(float(out[0]) - ref) <= bound, (float(out[0]), ref, bound)


def _logdiff64(a, b, eps):
    la, lb = torch.log(a.double().abs() + eps), torch.log(b.double().abs() + eps)
    return la - lb, la.abs() + lb.abs() + 2            # (d, the magnitude the fp32 logs of |.| + eps round against)


def _logdiff_inputs(B, M, T, seed):
    g = _g(seed)
    a = torch.randn(B, M, T, generator=g).exp()
    b = torch.randn(B, M, T, generator=g).exp()
    b[..., ::9] = a[..., ::9]                               # whole columns with a == b: r = 0
    b[:, 0, 1::5] = -b[:, 0, 1::5]                          # |.|: negative entries
    b[:, -1, 3::13] = 0.0                                   # b = 0: sign 0
    return a, b


@gpu
@pytest.mark.parametrize("B,M,T", [(1, 1, 1), (2, 80, 301), (3, 5, 90000)])
@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
def test_logdiff_rms_against_fp64(cuda, B, M, T, accumulate):
    from facodec_amd import ops
    a, b = _logdiff_inputs(B, M, T, B * M + T)
    eps, scale = 1e-5, 0.11
    out = torch.tensor([-1.25], device=cuda)
    scratch = torch.empty(1024, device=cuda)
    ops.logdiff_rms(a.to(cuda), b.to(cuda), out, scratch, eps, scale, accumulate)
    torch.cuda.synchronize()
    d, m = _logdiff64(a, b, eps)
    cols = (d * d).mean(1).sqrt()
    ref = scale * float(cols.sum()) + (-1.25 if accumulate else 0.0)
    mag = float((m * m).mean(1).sqrt().sum())
    bound = 4 * math.sqrt(B * T * M) * EPS32 * scale * mag + (4 * EPS32 * 1.25 if accumulate else 0.0)
    assert abs(float(out[0]) - ref) <= bound, (float(out[0]), ref, bound)


@gpu
@pytest.mark.parametrize("B,M,T", [(1, 1, 7), (2, 80, 301), (2, 2, 4096 * 128 + 300)], ids=["tiny", "mel", "past_block_cap"])
@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
def test_logdiff_rms_bwd_against_fp64(cuda, B, M, T, accumulate):
    from facodec_amd import ops
    a, b = _logdiff_inputs(B, M, T, 7 * M + T)
    eps, scale = 1e-5, 0.11
    db0 = torch.randn(B, M, T, generator=_g(5)) if accumulate else torch.zeros(B, M, T)
    db = db0.to(cuda)
    ops.logdiff_rms_bwd(a.to(cuda), b.to(cuda), db, eps, scale, accumulate)
    torch.cuda.synchronize()
    d, m = _logdiff64(a, b, eps)
    r = (d * d).mean(1, keepdim=True).sqrt()
    k = torch.where(r > 0, scale / (M * r), torch.zeros_like(r))
    bd = b.double()
    dd = 1.0 / (bd.abs() + eps)
    g = -k * d * torch.sign(bd) * dd
    got = db.cpu().double() - db0.double()
    # d_m is a difference of two logs (absolute error ~ ulp(|la| + |lb|)); r sums M squares
    bound = 8 * EPS32 * (k * m * dd + (M + 4) * g.abs()) + 2 * EPS32 * (db0.double().abs() + g.abs())
    assert bool(((got - g).abs() <= bound).all())
    zero_cols = (r == 0).expand_as(g)
    assert bool(zero_cols.any()) and bool((got[zero_cols] == 0).all())


@gpu
@pytest.mark.parametrize("with_mask", [True, False], ids=["partial_mask", "mask_none"])
@pytest.mark.parametrize("B,Cc,T", [(1, 1, 1), (3, 5, 63), (2, 128, 1001)])
def test_masked_mean_against_fp64(cuda, B, Cc, T, with_mask):
    from facodec_amd import ops
    g = _g(B * Cc + T)
    x = torch.randn(B, Cc, T, generator=g) + 3.0
    mask = None
    if with_mask:
        lens = torch.tensor([max(1, T - 7 * i) for i in range(B)])
        mask = (torch.arange(T)[None] < lens[:, None]).float()
        x = x * mask[:, None]                               # style_encoder: the input is already masked
    out = ops.masked_mean(x.to(cuda), mask.to(cuda) if mask is not None else None)
    torch.cuda.synchronize()
    den = mask.double().sum(1) if mask is not None else torch.full((B,), float(T), dtype=torch.float64)
    ref = x.double().sum(2) / den[:, None]
    bound = 4 * math.sqrt(T) * EPS32 * x.double().abs().sum(2) / den[:, None] + 2 * EPS32 * ref.abs()
    assert bool(((out.cpu().double() - ref).abs() <= bound).all())


# ------------------------------------------------------------------------------------------------------- pair_bwd, spec_power
@gpu
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
def test_pair_bwd_against_fp64(cuda, mode, accumulate):
    from facodec_amd import ops
    g = _g(40 + mode)
    n = 70001
    a = torch.rand(n, generator=g) * 4 + 1e-3
    b = a * (1 + (torch.rand(n, generator=g) * 0.5 + 1e-3) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0))
    b[::5] = a[::5]                                         # ties: zero gradient in every mode
    eps = 1e-2
    a[::13] = 0.5 * eps                                     # a <= eps (mode 1: zero gradient)
    a[1::13] = eps
    d_set = torch.tensor([-2.0, -1.5, -1.0, -0.75, -0.25, 0.25, 0.75, 1.0, 1.5, 2.0])   # |d| on both sides of 1 (mode 3)
    b[2:2 + 13 * d_set.numel():13] = a[2:2 + 13 * d_set.numel():13] - d_set
    scale = 0.3
    da0 = torch.randn(n, generator=g) if accumulate else torch.zeros(n)
    da = da0.to(cuda)
    ops.pair_bwd(a.to(cuda), b.to(cuda), da, mode, eps, scale, accumulate)
    torch.cuda.synchronize()
    ad, bd = a.double(), b.double()
    if mode == 0:
        ref = torch.sign(ad - bd)
    elif mode == 1:
        dl = torch.log10(ad.clamp_min(eps)) - torch.log10(bd.clamp_min(eps))
        ref = torch.where(ad > eps, torch.sign(dl) / (ad * math.log(10.0)), torch.zeros_like(ad))
    elif mode == 2:
        ref = 2 * (ad - bd)
    else:
        ref = (ad - bd).clamp(-1.0, 1.0)
    ref = scale * ref
    got = da.cpu().double() - da0.double()
    bound = 6 * EPS32 * ref.abs() + 2 * EPS32 * (da0.double().abs() + ref.abs())
    assert bool(((got - ref).abs() <= bound).all())
    assert bool((got[::5][(a[::5] == b[::5])] == 0).all())


@gpu
@pytest.mark.parametrize("power", [1, 2])
def test_spec_power_and_bwd_against_fp64(cuda, power):
    from facodec_amd import ops
    B, F, nf = 3, 257, 41
    g = _g(power)
    spec = torch.randn(B, 2 * F, nf, generator=g)
    spec[:, 0, :] = 0.0                                     # the DC row: exact-zero bins, |z| = 0
    spec[:, F, :] = 0.0
    spec[:, 5, 3] = 0.0                                     # a zero real part alone
    spec[:, F + 7, 4] = 0.0                                 # a zero imaginary part alone
    out = ops.spec_power(spec.to(cuda), power)
    dout = torch.randn(B, F, nf, generator=g)
    dspec = ops.spec_power_bwd(spec.to(cuda), dout.to(cuda), power)
    torch.cuda.synchronize()
    re, im = spec[:, :F].double(), spec[:, F:].double()
    p = re * re + im * im
    ref = p if power == 2 else p.sqrt()
    assert bool(((out.cpu().double() - ref).abs() <= 3 * EPS32 * ref).all())
    if power == 2:
        cr, ci = 2 * re, 2 * im
    else:
        m = p.sqrt()
        cr = torch.where(m > 0, re / m.clamp_min(1e-300), torch.zeros_like(m))
        ci = torch.where(m > 0, im / m.clamp_min(1e-300), torch.zeros_like(m))
    dref = torch.cat([dout.double() * cr, dout.double() * ci], 1)
    got = dspec.cpu().double()
    assert bool(torch.isfinite(got).all())
    assert bool(((got - dref).abs() <= 6 * EPS32 * dref.abs()).all())
    assert bool((got[:, 0] == 0).all()) and bool((got[:, F] == 0).all())


# ------------------------------------------------------------------------------------------------------- layernorm_c_affine
def _ln_kernel(Cc, T):
    """The dispatch of fac_layernorm_c_affine (misc.hip), restated."""
    return "small_t" if T <= 8 and Cc * T * 4 <= 64 * 1024 else "tiled"


# (case id, B, C, T, offset): the branch name leads the id
LN_CASES = [
    ("small_t_T1", 2, 1024, 1, 0.0),
    ("small_t_T8", 3, 256, 8, 0.0),
    ("small_t_T8_C2048_64KB", 2, 2048, 8, 0.0),             # C * T * 4 == 64 KB exactly
    ("small_t_T5_offset", 2, 1024, 5, 1000.0),
    ("tiled_T9", 2, 1024, 9, 0.0),
    ("tiled_T5_over_64KB", 2, 4096, 5, 0.0),                # T <= 8 but the block does not fit the LDS budget
    ("tiled_T100", 2, 256, 100, 0.0),                       # T not a multiple of 64
    ("tiled_T130_C7", 3, 7, 130, 0.0),                      # C below the 4 waves x 16-unroll span
    ("tiled_T100_offset", 2, 512, 100, 1000.0),             # mean >> std: a one-pass variance would lose everything
]


def _ln_ref(x, style):
    x = x.double().requires_grad_()
    st = style.double().requires_grad_()
    Cc = x.shape[1]
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    y = (x - mu) / torch.sqrt(var + 1e-5) * st[:, :Cc, None] + st[:, Cc:, None]
    return x, st, y


@gpu
@pytest.mark.parametrize("case", LN_CASES, ids=[c[0] for c in LN_CASES])
def test_layernorm_c_affine_and_bwd_against_fp64(cuda, case):
    from facodec_amd import ops
    name, B, Cc, T, offset = case
    assert _ln_kernel(Cc, T) == name.split("_T")[0]
    g = _g(Cc * T)
    x = torch.randn(B, Cc, T, generator=g) * 0.5 + offset + torch.randn(B, 1, T, generator=g) * 0.1
    style = torch.cat([1 + 0.3 * torch.randn(B, Cc, generator=g), 0.2 * torch.randn(B, Cc, generator=g)], 1)
    out = ops.layernorm_c_affine(x.to(cuda), style.to(cuda))
    dout = torch.randn(B, Cc, T, generator=g)
    dx, dstyle = ops.layernorm_c_affine_bwd(x.to(cuda), style.to(cuda), dout.to(cuda))
    torch.cuda.synchronize()
    xr, st, y = _ln_ref(x, style)
    (y * dout.double()).sum().backward()
    std = float(((x.double() - x.double().mean(1, keepdim=True)) ** 2).mean(1).sqrt().min())
    # mean / variance are fp32 sums over C of values as large as max|x|: their error relative to the spread is at most about
    # cond = sqrt(C) 2^-24 max|x| / std, and every output inherits it (dstyle also sums T products).  Measured on MI355X, error /
    # scale over all cases: output <= 0.056, dx <= 0.056, dstyle <= 0.075 (offset cases: 0.038 - 0.075; a one-pass variance
    # would be off by O(1) there).  Bars: about 10x that.
    cond = math.sqrt(Cc) * EPS32 * float(x.abs().max()) / std
    sc = cond + EPS32
    sc_s = math.sqrt(T) * EPS32 + cond
    assert _max_rel(out, y) <= 0.6 * sc, (_max_rel(out, y), sc)
    assert _max_rel(dx, xr.grad) <= 0.6 * sc, (_max_rel(dx, xr.grad), sc)
    assert _max_rel(dstyle, st.grad) <= 0.75 * sc_s, (_max_rel(dstyle, st.grad), sc_s)


# ------------------------------------------------------------------------------------------------------- cross entropy, crop_rows
@gpu
@pytest.mark.parametrize("N,Cn", [(1, 1), (5, 3), (37, 257), (9, 1023), (3, 5001)])
def test_cross_entropy_against_fp64(cuda, N, Cn):
    g = _g(N * Cn)
    logits = torch.randn(N, Cn, generator=g) * 3
    labels = torch.randint(0, Cn, (N,), generator=g)
    labels[0] = Cn - 1                                      # the last class
    ld, lab = logits.to(cuda), labels.to(cuda)
    loss = torch.zeros(1, device=cuda)
    scratch = torch.empty(N, device=cuda)
    dl = torch.empty(N, Cn, device=cuda)
    scale = 0.7 / N
    _call("fac_cross_entropy", _p(ld), _p(lab), _p(loss), _p(None), _p(scratch), N, Cn, C.c_float(0.0))
    _call("fac_cross_entropy", _p(ld), _p(lab), _p(None), _p(dl), _p(scratch), N, Cn, C.c_float(scale))
    torch.cuda.synchronize()
    x = logits.double().requires_grad_()
    ref = torch.nn.functional.cross_entropy(x, labels)
    (0.7 * ref).backward()
    lse = torch.logsumexp(x.detach(), 1)
    mag = float((lse.abs() + x.detach()[torch.arange(N), labels].abs()).mean())
    assert abs(float(loss[0]) - float(ref)) <= 8 * math.sqrt(Cn) * EPS32 * mag
    p = torch.softmax(x.detach(), 1)
    bound = scale * EPS32 * (8 * math.sqrt(Cn) * p + 2)
    assert bool(((dl.cpu().double() - x.grad).abs() <= bound).all())


@gpu
def test_focal_cross_entropy_against_fp64(cuda):
    from facodec_amd import autograd_disc as AD
    g = _g(77)
    logits = torch.randn(29, 1023, generator=g)
    labels = torch.randint(0, 1023, (29,), generator=g)
    xl = logits.to(cuda).requires_grad_()
    loss = AD.focal_cross_entropy(xl, labels.to(cuda), gamma=2.0)
    (1.5 * loss).backward()
    torch.cuda.synchronize()
    x = logits.double().requires_grad_()
    ce = torch.nn.functional.cross_entropy(x, labels)
    ref = (1 - torch.exp(-ce)) ** 2 * ce
    (1.5 * ref).backward()
    assert abs(float(loss) - float(ref)) <= 64 * math.sqrt(1023) * EPS32 * float(ref)
    assert _max_rel(xl.grad, x.grad) <= 64 * math.sqrt(1023) * EPS32


@gpu
def test_crop_rows_exact(cuda):
    B, Cn, T_src, T_dst, scale = 5, 3, 3000, 600, 300
    src = torch.randn(B, Cn, T_src, generator=_g(8))
    # from the first sample; up to the last sample; running past the end (zero fill); before the start (zero fill); inside
    start = torch.tensor([0, 8, 9, -1, 4])
    out, buf, pad = _canary((B * Cn * T_dst,), cuda)
    src_d = src.to(cuda)
    start_d = start.to(cuda)
    _call("fac_crop_rows", _p(src_d), _p(out), _p(start_d), B, Cn, T_src, T_dst, scale)
    torch.cuda.synchronize()
    s = start[:, None, None] * scale + torch.arange(T_dst)
    ok = (s >= 0) & (s < T_src)
    ref = torch.where(ok, torch.gather(src, 2, s.clamp(0, T_src - 1).expand(B, Cn, T_dst)), torch.zeros(()))
    assert torch.equal(out.cpu().view(B, Cn, T_dst), ref) and _canary_intact(buf, pad)
    assert bool(ok[1, 0, -1]) and int(s[1, 0, -1]) == T_src - 1 and not bool(ok[2, 0, -1]) and not bool(ok[3, 0, 0])


# ------------------------------------------------------------------------------------------------------- disc_preprocess
def _clips(B, T, seed, negative_peak=False):
    g = _g(seed)
    x = torch.randn(B, T, generator=g) * 0.2 + 0.05
    x[:, T // 3] += 1.7                                     # one clear peak per clip
    if negative_peak:
        x[:, T // 3] -= 4.0
    return x


@gpu
@pytest.mark.parametrize("T,neg", [(100, False), (1000, False), (24000, False), (24000, True), (37, True)],
                         ids=["T100", "T1000", "T24000", "T24000_negative_peak", "T37_negative_peak"])
def test_disc_preprocess_and_bwd_against_fp64(cuda, T, neg):
    from oracle import facodec_oracle as O
    B = 3
    x = _clips(B, T, T, neg)
    xd = x.to(cuda)
    z = torch.empty(B, T, device=cuda)
    stats = torch.empty(B, 4, device=cuda)
    _call("fac_disc_preprocess", _p(xd), _p(None), _p(z), _p(stats), B, T)
    dz = torch.randn(B, T, generator=_g(T + 1))
    dx = torch.empty(B, T, device=cuda)
    dz_d = dz.to(cuda)
    _call("fac_disc_preprocess", _p(xd), _p(dz_d), _p(dx), _p(stats), B, T)
    torch.cuda.synchronize()
    x64 = x.double().requires_grad_()
    z64 = O.discriminator_preprocess(x64)
    (z64 * dz.double()).sum().backward()
    y0 = x.double() - x.double().mean(1, keepdim=True)
    mx = y0.abs().max(1).values
    st = stats.cpu().double()
    mean_tol = 4 * math.sqrt(T) * EPS32 * x.double().abs().mean(1)
    assert bool(((st[:, 0] - x.double().mean(1)).abs() <= mean_tol).all())
    assert bool(((st[:, 1] - mx).abs() <= 4 * EPS32 * mx + mean_tol).all())
    am = st[:, 2].long()
    assert bool((am == T // 3).all())                       # the arg-max points to the peak
    assert bool((y0[torch.arange(B), am].abs() >= mx - 2 * mean_tol).all())
    assert bool((st[:, 3] == (-1.0 if neg else 1.0)).all())
    cond = math.sqrt(T) * EPS32 * float(x.abs().max() / mx.min())
    assert _max_rel(z, z64) <= 8 * (EPS32 + cond)
    c = 0.8 / mx
    scale_bwd = float((c[:, None] * dz.double().abs()).max() + (0.8 / mx ** 2 * (dz.double() * y0).abs().sum(1)).max())
    err = float((dx.cpu().double() - x64.grad).abs().max())
    assert err <= 16 * math.sqrt(T) * EPS32 * scale_bwd, (err, scale_bwd)


# ------------------------------------------------------------------------------------------------------- in-place reflect fold
def test_pad_fold_edges_rejects_overlapping_edges_without_gpu():
    """At T == pad_left + pad_right + 1 both edges add onto x[pad_left] (two unsynchronised += on one element): refused, like
    every shorter signal.  The pointer is never dereferenced -- the checks fail on the host.  That one sample more is accepted
    (and folded correctly) is test_in_place_reflect_fold_at_shortest_signal's pl + pr + 2 cases, which need a GPU."""
    lib = _lib.load()
    fake = C.c_void_p(0x10000)
    for pl, pr in ((3, 3), (1, 1), (3, 0), (0, 4)):
        T = pl + pr + 1
        assert lib.fac_pad_fold_edges(fake, 1, 1, T, T + pl + pr, pl, None) == -1
        assert b"too short" in lib.fac_last_error()
        assert lib.fac_pad_fold_edges(fake, 1, 1, T - 1, T - 1 + pl + pr, pl, None) == -1


def _conv_bwd_data_ref(dy, v, t_in, pl, pr):
    """fp64 data gradient of reflect-pad (pl, pr) + conv1d(v) at input length t_in."""
    x = torch.zeros(dy.shape[0], v.shape[1], t_in, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(x, (pl, pr), mode="reflect"), v.double())
    (y * dy.double()).sum().backward()
    return x.grad


@gpu
@pytest.mark.parametrize("k,extra", [(7, 0), (7, 1), (5, 0), (5, 1), (3, 1)], ids=["k7_T_pl_pr_1", "k7_T_pl_pr_2", "k5_T_pl_pr_1",
                                                                                     "k5_T_pl_pr_2", "k3_T_pl_pr_2"])
def test_in_place_reflect_fold_at_shortest_signal(cuda, k, extra):
    """conv1d_bwd_data(allow_view=True) at T = pad_left + pad_right + 1 (now the copy path) and + 2 (the in-place fold, edges
    disjoint): bit-identical to the copy path (FAC_FOLD_IN_PLACE=0) and equal to the fp64 data gradient."""
    from facodec_amd import ops
    B, c_in, c_out = 2, 8, 8
    _, padding_total, _ = ops.conv_out_len(20, k, 1, 1)
    pl = padding_total - padding_total // 2                # non-causal: both pads non-zero
    pr = padding_total - pl
    t_in = pl + pr + 1 + extra
    t_out, _, _ = ops.conv_out_len(t_in, k, 1, 1)
    g = _g(k * 10 + extra)
    v = torch.randn(c_out, c_in, k, generator=g) * 0.3
    dy = torch.randn(B, c_out, t_out, generator=g)

    def run(flag):
        ops.FOLD_IN_PLACE = flag
        try:
            dx = ops.conv1d_bwd_data(dy.to(cuda), v.to(cuda), None, t_in, causal=False, allow_view=True)
            torch.cuda.synchronize()
            return dx.contiguous().cpu(), dx.is_contiguous()
        finally:
            ops.FOLD_IN_PLACE = 1

    (a, a_contig), (b, _) = run(1), run(0)
    assert a_contig == (extra == 0)                        # T = pl + pr + 1: not the in-place path any more
    assert torch.equal(a, b)
    ref = _conv_bwd_data_ref(dy, v, t_in, pl, pr)
    mag = _conv_bwd_data_ref(dy.abs(), v.abs(), t_in, pl, pr)
    assert bool(((a.double() - ref).abs() <= 4 * c_out * k * EPS32 * mag).all())


# ------------------------------------------------------------------------------------------------------- wgrad k1 / taps alignment
def test_wgrad_k1_refuses_misaligned_pointers_without_gpu():
    """The k = 1 / taps weight-gradient kernels read with 16-byte loads: a base pointer off 16 bytes makes the pointer-aware
    workspace queries answer -1 (ops then takes the split kernel) and the launches refuse.  Nothing is dereferenced."""
    lib = _lib.load()
    al, mis = C.c_void_p(0x10000), C.c_void_p(0x10004)
    assert lib.fac_conv1d_bwd_weight_k1_ws_bytes(2, 64, 64, 4096) > 0
    assert lib.fac_conv1d_bwd_weight_k1_ws_bytes_for(al, al, 2, 64, 64, 4096) == lib.fac_conv1d_bwd_weight_k1_ws_bytes(2, 64, 64, 4096)
    assert lib.fac_conv1d_bwd_weight_k1_ws_bytes_for(mis, al, 2, 64, 64, 4096) == -1
    assert lib.fac_conv1d_bwd_weight_k1_ws_bytes_for(al, mis, 2, 64, 64, 4096) == -1
    nb = lib.fac_conv1d_bwd_weight_k1_ws_bytes(2, 64, 64, 4096)
    for x, dy in ((mis, al), (al, mis)):
        assert lib.fac_conv1d_bwd_weight_k1(x, dy, al, None, al, nb, 2, 64, 64, 4096, None) == -1
        assert b"16-byte aligned" in lib.fac_last_error()
    args = (2, 1, 64, 4096, 7, 7, 1, 0)
    nbt = lib.fac_conv1d_bwd_weight_taps_ws_bytes(*args)
    assert nbt > 0 and lib.fac_conv1d_bwd_weight_taps_ws_bytes_for(al, *args) == nbt
    assert lib.fac_conv1d_bwd_weight_taps_ws_bytes_for(mis, *args) == -1
    tx = lib.fac_conv1d_bwd_weight_taps_tx(4096, 7, 7, 1, 0)
    assert lib.fac_conv1d_bwd_weight_taps(al, mis, al, None, al, nbt, 2, 1, tx, 64, 4096, 7, 7, 1, 0, None) == -1
    assert b"16-byte aligned" in lib.fac_last_error()


def _spy_launches(lib, names):
    """Counts calls of the named C entries made through _lib.load() while the spy is installed."""
    calls = {n: 0 for n in names}
    orig = {n: getattr(lib, n) for n in names}

    def wrap(n):
        def f(*a):
            calls[n] += 1
            return orig[n](*a)
        return f

    for n in names:
        setattr(lib, n, wrap(n))
    return calls, lambda: [setattr(lib, n, orig[n]) for n in names]


def _misaligned(t, dev):
    """A contiguous copy of t on dev whose storage starts one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@gpu
@pytest.mark.parametrize("which", ["aligned", "x_offset", "dy_offset"])
def test_wgrad_k1_misaligned_inputs_fall_back(cuda, which):
    from facodec_amd import ops
    B, Cc, T = 2, 64, 4096
    g = _g(3)
    x = torch.randn(B, Cc, T, generator=g)
    dy = torch.randn(B, Cc, T, generator=g)
    xd = _misaligned(x, cuda) if which == "x_offset" else x.to(cuda)
    dyd = _misaligned(dy, cuda) if which == "dy_offset" else dy.to(cuda)
    lib = _lib.load()
    calls, restore = _spy_launches(lib, ["fac_conv1d_bwd_weight_k1"])
    try:
        dw = ops.conv1d_bwd_weight(xd, dyd, 1, pad_left=0, pad_mode=ops.PAD_ZERO)
        torch.cuda.synchronize()
    finally:
        restore()
    if ops.WGRAD_K1_STREAM and ops.BF16_SPLIT:
        assert calls["fac_conv1d_bwd_weight_k1"] == (1 if which == "aligned" else 0)
    ref = torch.einsum("bct,bdt->dc", x.double(), dy.double())
    mag = torch.einsum("bct,bdt->dc", x.double().abs(), dy.double().abs())
    assert bool(((dw.cpu().double().view(Cc, Cc) - ref).abs() <= 4 * math.sqrt(B * T) * EPS32 * mag).all())


@gpu
@pytest.mark.parametrize("which", ["aligned", "dy_offset"])
def test_wgrad_taps_misaligned_dy_falls_back(cuda, which):
    from facodec_amd import ops
    B, c_in, c_out, T, k = 2, 1, 64, 4096, 7
    g = _g(4)
    x = torch.randn(B, c_in, T, generator=g)
    dy = torch.randn(B, c_out, T, generator=g)
    dyd = _misaligned(dy, cuda) if which == "dy_offset" else dy.to(cuda)
    lib = _lib.load()
    calls, restore = _spy_launches(lib, ["fac_conv1d_bwd_weight_taps"])
    try:
        dw = ops.conv1d_bwd_weight(x.to(cuda), dyd, k, pad_mode=ops.PAD_REFLECT, causal=True)
        torch.cuda.synchronize()
    finally:
        restore()
    if ops.WGRAD_K1_STREAM and ops.BF16_SPLIT:
        assert calls["fac_conv1d_bwd_weight_taps"] == (1 if which == "aligned" else 0)
    xp = torch.nn.functional.pad(x.double(), (k - 1, 0), mode="reflect")
    cols = xp.unfold(2, k, 1)                                # (B, c_in, T, k)
    ref = torch.einsum("bitk,bot->oik", cols, dy.double())
    mag = torch.einsum("bitk,bot->oik", cols.abs(), dy.double().abs())
    assert bool(((dw.cpu().double() - ref).abs() <= 4 * math.sqrt(B * T) * EPS32 * mag).all())
