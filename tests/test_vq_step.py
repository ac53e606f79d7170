"""fac_vq_fwd (facodec_amd/csrc/vq.hip), the fused VQ step, stage by stage against fp64 and torch fp32 on the CPU, on both of its
kernels (16 frames per workgroup: `tile`; one workgroup per frame: `small_t`).  Every launch goes through the C entry with a
VqDesc built here (one case per route also through ops.vq_step, one through VectorQuantize._weights()).  Every output lies in a
canary buffer, is pre-filled with NaN (codes: a negative sentinel) and must be finite (in [0, Kc)) afterwards, so a tile the
padded grid skipped shows; inputs must be unchanged.  Each stage is held against a reference computed from the kernel's OWN
earlier outputs (z_e for the codes, z_e and codes for the out-projection and the loss, zq_out for the bookkeeping): no error
cascades from one stage into the bound of the next.

  A  z_e       fp64 sum W_in x + b_in, `_sum_bound` with n = D + 1, terms |w||x| + |b|, no extra (weight norm: see the module test)
  B  codes     the decidability rule below; == ops.vq_search on the same z_e bits
  C  planted   one-hot in-projection, query = 3.7 x a codebook row at both sides of every range boundary of the route taken,
               duplicated rows (lowest index wins), a zero query
  D  zq_out    z_st = z_e + (z_q - z_e) restated in torch fp32 (bit-equal where a one-hot out-projection exports it), then
               sum_d (w sc) z_st + b_out in fp64, `_sum_bound` with n = 9, extra = 1: the product w sc is rounded once before the
               FMA chain, a relative error 2^-24 of every term
  E  exact     residual == z_in - zq_out, zq_acc == acc0 + zq_out * mask[b], bit for bit the torch fp32 expression
  F  loss_part per (b, tile) the fp64 sum of (z_e - z_q)^2 over the VALID frames, `_sum_bound` with n = 128 (8 dims x 16 frames),
               extra = 3: a term is fl(fl(z_e - z_q)^2), the difference's rounding counts twice in the square, the product's once
  G  forms     each nullable pointer absent, residual aliasing z_in, strided codes, a second launch, small_t against tile

The decidability rule (B).  dist_k = (|e|^2 - 2 e.c~_k) + |c~_k|^2 with e, c~ the normalised query and rows, as
include/facodec_hip.h states it, is evaluated in fp64 from the kernel's z_e bits and the fp32 codebook.  DELTA bounds the error
of ONE fp32 distance of the kernel against it, to first order in u = 2^-24, on |e| = |c~| = 1, |2 e.c~| <= 2, |dist| <= 4:
  normalisation (load_codebook and the query alike): the sum of 8 squares has 1 product + 7 add roundings, relative 8 u; the root
      halves that and adds its own rounding (2 u allowed: sqrtf need not be correctly rounded): the norm is off by 6 u relative;
      the division adds 1 u: every component of e and of c~ carries a relative error of at most 7 u;
  ee = sum e^2 and cc_k = sum c~_k^2: 2 x 7 u from the components, 8 u from the sum itself: 22 u each, on a value of 1;
  dot = (2 e).c~_k in scan_codes: 2 e is exact; 14 u relative on sum |2 e_d c~_d| <= 2 from the components: 28 u; 1 product + 7
      FMA roundings of partial sums bounded by 2: 16 u; together 44 u;
  the final two adds: fl(ee - dot), |.| <= 3: 3 u; fl(. + cc_k), |.| <= 4: 4 u.
  DELTA = (22 + 22 + 44 + 3 + 4) u = 95 u, stated as 96 * 2^-24 = 5.7e-6 for the second-order terms.  Not fitted: a torch-fp32
  restatement of the distance measures 19 * 2^-24 (test_fp32_distance_error_and_undecidable_positions_stay_within_the_cap).
TAU = 2 DELTA = 1.14e-5.  Two fp32 distances whose fp64 values differ by TAU or more cannot swap order, so where the fp64 top-2
gap is >= TAU the kernel's code must EQUAL the fp64 arg-min; elsewhere dist64[code] - min dist64 <= TAU.  Bit-identical codebook
rows count as one row in the gap, and among them the lowest index is required everywhere.  Undecidable positions are capped at
max(2, 0.5 % of B T) per case: a condition on the inputs, checked on the CPU for every case with torch's fp32 z_e.

Case ids begin with the route.  The route condition and both LDS formulas are restated here and pinned to the source text.

Measured on MI355X (tolerance report keys vq_step.*), worst case over the table, error / bound:
  A z_e 0.11 (D = 3; 0.015 with weight norm in the loop), D zq_out 0.21, F loss_part 0.053; C and E exact.
  B: none of the 4207 random positions of the table is undecidable and every one got the fp64 arg-min; the worst
  dist64[code] - min over TAU is 1.9e-3, at a planted near tie (each got one of its two rows), and 5.8e-11 at the planted zero
  queries, where every distance is 1.  fp32-CPU restatement of the distance: worst error 16.9 * 2^-24 over the table (DELTA = 96 * 2^-24), no
  undecidable position either.  The GPU tests of this file take 3 s together, the CPU tests 5 s.
Kernel faults planted by hand in vq.hip, each built once (the failing tests are named in DESIGN.md 20): the tile scan stopping at
k_end - 1, '>=' in the 16-way combine, the small-T tree without its tie clause, mk multiplied into residual, the loss keeping
invalid lanes.  `logical > B * n_tiles` in the padded-grid guard was NOT built: the extra workgroup would run clip b = B and
read and write past every tensor."""
import ctypes as C
import functools
import math
import os
import types

import pytest
import torch

from facodec_amd import _lib
from test_train_kernels_gen import EPS32, _call, _canary, _canary_intact, _g, _p, _record, _sum_bound

gpu = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CD = 8                                   # codebook_dim the kernel is built for
DELTA = 96 * EPS32                       # worst error of one fp32 distance, derived in the module docstring
TAU = 2 * DELTA
LDS_MAX = 160 * 1024
SENTINEL = -7
NAN = float("nan")


# ======================================================================================================= route, restated
def _r4(n):
    return (n + 3) & ~3


def _lds_tile(D, Kc):
    return (Kc * 8 + _r4(Kc) + 4 * 8 * 16 + 8 * 16 + 2 * 16 * 16 + D * 8) * 4


def _lds_small(D, Kc):
    return (Kc * 8 + _r4(Kc) + _r4(D) + D * 8 + 4 * 8 + 8 + 512) * 4


def _route(D, T, Kc, loss):
    if _lds_tile(D, Kc) > LDS_MAX:
        return "refused"
    if T <= 8 and not loss and D <= 4096 and _lds_small(D, Kc) <= LDS_MAX:
        return "small_t"
    return "tile"


def _n_ranges(route):
    return 16 if route == "tile" else 256


def _kper(Kc, route):
    return -(-Kc // _n_ranges(route))


# (B, D, T, Kc, loss_part requested)
TILE_CASES = [
    (3, 256, 150, 1024, True), (2, 1024, 33, 1024, True), (5, 72, 17, 1024, True), (4, 70, 37, 1000, True),
    (2, 64, 129, 37, True),          # Kc % 16 != 0: the ranges are 3 codes long, the 13th holds one code, the last three none
    (9, 128, 16, 3, True),           # Kc < 16
    (1, 8, 1, 1, True),              # Kc = 1
    (2, 3, 31, 16, True),            # D < 4: the fourth wave's channel quarter is empty; T % 16 = 15
    (1, 16, 16, 64, True), (7, 16, 5, 64, True), (3, 16, 40, 64, True), (1, 16, 260, 64, True),   # B * n_tiles = 1, 7, 9, 17
]
SMALL_CASES = [(33, 512, 1, 1024, False), (3, 1024, 8, 1024, False), (2, 256, 5, 1024, False), (2, 70, 3, 1000, False),
               (1, 9, 2, 5, False)]
THRESHOLD_CASES = [
    (2, 40, 8, 100, False), (2, 40, 9, 100, False),              # T = 8 / 9 without loss
    (1, 4096, 2, 16, False), (1, 4097, 2, 16, False),            # D = 4096 / 4097: both fit the LDS, the D limit decides
    (1, 3465, 1, 1024, False), (1, 3466, 1, 1024, False),        # the small-T kernel's own LDS limit at Kc = 1024
    (1, 3824, 3, 1024, False),                                   # the most the tile kernel's LDS takes at Kc = 1024
]
CASES = TILE_CASES + SMALL_CASES + THRESHOLD_CASES


def _case_id(case):
    B, D, T, Kc, loss = case
    return f"{_route(D, T, Kc, loss)}_B{B}_D{D}_T{T}_K{Kc}{'_loss' if loss else ''}"


FORM_CASES = [(4, 70, 37, 1000, True), (2, 70, 3, 1000, False)]
FORMS = ["no_residual", "no_zq_acc", "no_zq_out", "no_mask", "no_z_e", "no_loss_part", "no_w_out_scale", "alias", "codes_row",
         "second_launch"]
FORM_PARAMS = [(c, f) for c in FORM_CASES for f in FORMS if not (f == "no_loss_part" and not c[4])]


# ======================================================================================================= inputs
def _pack_w_in(W):
    """(8, D) -> the packed layout fac_pack_conv_w gives the in-projection: row c holds W[:, c] in its first 8 of 32 floats."""
    D = W.shape[1]
    p = torch.zeros(D, 1, 32)
    p[:, 0, :CD] = W.t()
    return p


def _make(x, W, b_in, cb, w_out, sc, b_out, mask, acc0):
    B, D, T = x.shape
    return types.SimpleNamespace(B=B, D=D, T=T, Kc=cb.shape[0], x=x, W=W, w_in=_pack_w_in(W), b_in=b_in, cb=cb, w_out=w_out, sc=sc,
                                 b_out=b_out, mask=mask, acc0=acc0)


@functools.lru_cache(maxsize=None)
def _inputs(B, D, T, Kc):
    """Random inputs of a case (shared by every test of the case and never written): unit-variance z_e, a bias of 0.5 to 1.5 in
    every dimension, a weight-norm scale, a mask with ones AND zeros in one batch and a non-trivial accumulator."""
    g = _g(100003 * B + 1009 * D + 17 * T + Kc)
    x = torch.randn(B, D, T, generator=g)
    W = torch.randn(CD, D, generator=g) / math.sqrt(D)
    b_in = (torch.rand(CD, generator=g) + 0.5) * (1 - 2 * (torch.arange(CD) % 2)).float()
    cb = torch.randn(Kc, CD, generator=g)
    w_out = torch.randn(D, CD, generator=g) * 0.3
    sc = torch.rand(D, generator=g) + 0.5
    b_out = torch.randn(D, generator=g) * 0.1
    mask = (1 - torch.arange(B) % 2).float()
    acc0 = torch.randn(B, D, T, generator=g)
    return _make(x, W, b_in, cb, w_out, sc, b_out, mask, acc0)


# ======================================================================================================= planted answers
def _planted_indices(Kc, route):
    """Rows 0, Kc - 1 and both sides of every range boundary of the route: g * ceil(Kc / 16) - 1 and g * ceil(Kc / 16) on the tile
    kernel, tid * ceil(Kc / 256) - 1 and tid * ceil(Kc / 256) on the small-T kernel."""
    kper = _kper(Kc, route)
    s = {0, Kc - 1}
    for r in range(1, _n_ranges(route)):
        s.update(k for k in (r * kper - 1, r * kper) if 0 <= k < Kc)
    return sorted(s)


def _planted_pairs(Kc, route):
    """Pairs (i < j) of rows to make bit-identical, disjoint: within one range, across two adjacent ranges, across two distant
    ranges and the two ends.  On the small-T kernel the distant pair sits in the ranges of threads 64 and 128: the tree compares
    slot 0, which by then holds thread 128's row, with slot 64 -- the lower index in the HIGHER slot, which only the tree's tie
    clause resolves (adjacent ranges and the two ends meet with the lower index in the lower slot)."""
    kper = _kper(Kc, route)
    pairs = {}
    if kper >= 2 and kper + 1 < Kc:
        pairs["within"] = (kper, kper + 1)
    if 3 * kper < Kc:
        pairs["adjacent"] = (3 * kper - 1, 3 * kper)
    if Kc > 1:
        pairs["ends"] = (0, Kc - 1)
    lo, hi = (5, 11) if route == "tile" else (64, 128)
    if hi * kper < Kc - 1:
        pairs["distant"] = (lo * kper, hi * kper)
    return pairs


PLANTED_T = {"tile": 21, "small_t": 7}
PLANTED_D = 12


@functools.lru_cache(maxsize=None)
def _planted(Kc, route, dup):
    """-> (inputs, planted: list of (position in B * T, row the query is 3.7 x of), zero: position of the zero query, near:
    (position, a, b) of a query half way between the normalised rows a and b, b the nearest row to a -- an undecidable position
    whose code must be a or b -- or None with duplicated rows).
    One-hot in-projection (z_e = x[:8] bit for bit) on D = 12 channels, one-hot out-projection rows 0..7 without scale and bias
    (zq_out[:, :8] = z_st bit for bit), the other channels random.  dup: the pairs of `_planted_pairs` are made identical and the
    queries are both rows of each pair; otherwise the rows are distinct and the queries are `_planted_indices`."""
    g = _g(7919 * Kc + (1 if route == "tile" else 2) + (10 if dup else 0))
    cb = torch.randn(Kc, CD, generator=g)
    rows = []
    if dup:
        for i, j in _planted_pairs(Kc, route).values():
            cb[j] = cb[i]
            rows += [i, j]
    else:
        rows = _planted_indices(Kc, route)
    T = PLANTED_T[route]
    n = len(rows) + 2 + 5                                    # + the zero query + the near tie + a few random ones
    B = -(-n // T)
    D = PLANTED_D
    x = torch.randn(B, D, T, generator=g)
    q = x.permute(0, 2, 1).reshape(B * T, D).clone()
    q[:len(rows), :CD] = 3.7 * cb[rows]
    zero = len(rows)
    q[zero, :CD] = 0.0
    near = None
    if not dup and Kc >= 3:
        cn = cb / cb.norm(dim=1, keepdim=True)
        a = Kc // 2
        sim = cn @ cn[a]
        sim[a] = -2.0
        b = int(sim.argmax())
        near = (zero + 1, min(a, b), max(a, b))
        q[zero + 1, :CD] = 2.5 * (cn[a] + cn[b])
    x = q.reshape(B, T, D).permute(0, 2, 1).contiguous()
    W = torch.zeros(CD, D)
    W[torch.arange(CD), torch.arange(CD)] = 1.0
    w_out = torch.randn(D, CD, generator=g) * 0.3
    w_out[:CD] = torch.eye(CD)
    b_out = torch.randn(D, generator=g) * 0.1
    b_out[:CD] = 0.0
    inp = _make(x, W, torch.zeros(CD), cb, w_out, None, b_out, (1 - torch.arange(B) % 2).float(), torch.randn(B, D, T, generator=g))
    return inp, list(enumerate(rows)), zero, near


# ======================================================================================================= references
def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _rows(z_e):
    """(B, 8, T) -> (B T, 8), position b T + t."""
    return z_e.permute(0, 2, 1).reshape(-1, CD)


def _dist64(z_e, cb):
    """The header's distance in fp64 from fp32 z_e (B, 8, T) and the fp32 codebook -> (B T, Kc)."""
    q, c = _rows(z_e).double(), cb.double()
    e = q / q.norm(dim=1, keepdim=True).clamp_min(1e-12)
    c = c / c.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return ((e * e).sum(1, keepdim=True) - (2 * e) @ c.t()) + (c * c).sum(1)[None]


def _dist32(z_e, cb):
    """The same expression in torch fp32, the dot product as eight elementwise steps so that bit-identical rows get bit-identical
    distances (a BLAS call may treat columns differently)."""
    q, c = _rows(z_e), cb
    e = q / q.norm(dim=1, keepdim=True).clamp_min(1e-12)
    c = c / c.norm(dim=1, keepdim=True).clamp_min(1e-12)
    e2 = 2 * e
    dot = e2[:, 0:1] * c[:, 0][None]
    for d in range(1, CD):
        dot = dot + e2[:, d:d + 1] * c[:, d][None]
    return ((e * e).sum(1, keepdim=True) - dot) + (c * c).sum(1)[None]


def _first_identical(cb):
    """For every row the lowest index of a bit-identical row."""
    Kc = cb.shape[0]
    _, inv = torch.unique(_bits(cb), dim=0, return_inverse=True)
    first = torch.full((int(inv.max()) + 1,), Kc, dtype=torch.int64).scatter_reduce(0, inv, torch.arange(Kc), "amin")
    return first[inv]


def _judge_codes(z_e, cb, codes):
    """The decidability rule on one launch's z_e bits and codes -> (undecidable positions, worst (dist64[code] - min) / TAU)."""
    Kc = cb.shape[0]
    k = codes.reshape(-1)
    assert bool(((k >= 0) & (k < Kc)).all()), "B.codes outside [0, Kc) (a position the launch did not write?)"
    d = _dist64(z_e, cb)
    first = _first_identical(cb)
    du = d.masked_fill((first != torch.arange(Kc))[None], float("inf"))      # identical rows count once, at their lowest index
    top = du.topk(min(2, Kc), dim=1, largest=False)
    best, dmin = top.indices[:, 0], top.values[:, 0]
    gap = top.values[:, 1] - dmin if Kc > 1 else torch.full_like(dmin, float("inf"))
    decidable = gap >= TAU
    assert bool((first[k] == k).all()), "B.codes: a higher index among bit-identical codebook rows"
    wrong = decidable & (k != best)
    assert not bool(wrong.any()), f"B.codes: {int(wrong.sum())} decidable positions differ from the fp64 arg-min, first at {int(wrong.nonzero()[0])}"
    excess = d.gather(1, k[:, None])[:, 0] - dmin
    worst = float(excess.max()) / TAU
    assert worst <= 1.0, f"B.codes: dist64[code] - min = {worst:.3f} TAU at an undecidable position"
    return int((~decidable).sum()), worst


def _cap(n_positions):
    return max(2, 0.005 * n_positions)


def _zst32(z_e, cb, codes):
    zq = cb[codes].permute(0, 2, 1)
    return z_e + (zq - z_e), zq


def _loss_ref(z_e, zq):
    """(B, ceil(T / 16)) fp64 sums of (z_e - z_q)^2 over the valid frames of each tile."""
    B, _, T = z_e.shape
    nt = -(-T // 16)
    sq = (z_e.double() - zq.double()) ** 2
    sq = torch.cat([sq, torch.zeros(B, CD, nt * 16 - T, dtype=torch.float64)], 2)
    return sq.view(B, CD, nt, 16).sum((1, 3))


def _check_stages(name, inp, out, mask="given", sc="given", W64=None, extra_A=0.0):
    """Stages A, B, D, E, F on whatever outputs the launch exported.  mask / sc: the tensors the launch was given (None: absent).
    W64: the exact in-projection weights where they are not the fp32 `inp.W` (weight norm), with extra_A for their rounding.
    -> (undecidable positions, worst excess / TAU) or None without z_e."""
    B, D, T = inp.B, inp.D, inp.T
    mask = inp.mask if isinstance(mask, str) else mask
    sc = inp.sc if isinstance(sc, str) else sc
    z_e, codes, zq_out = out.z_e, out.codes, out.zq_out
    x64 = inp.x.double()
    judged = None
    if z_e is not None:
        W = inp.W.double() if W64 is None else W64
        ref = torch.einsum("dc,bct->bdt", W, x64) + inp.b_in.double().view(1, CD, 1)
        mag = torch.einsum("dc,bct->bdt", W.abs(), x64.abs()) + inp.b_in.double().abs().view(1, CD, 1)
        _sum_bound(f"vq_step.{name}.A.z_e", z_e, ref, mag, D + 1, extra=extra_A)
        judged = _judge_codes(z_e, inp.cb, codes)
        _record(f"vq_step.{name}.B.codes", {"undecidable": judged[0], "worst_excess_over_tau": judged[1], "positions": B * T})
        print(f"[tol] vq_step.{name}.B.codes: {judged[0]} undecidable of {B * T}, worst excess / TAU {judged[1]:.3e}")
        assert judged[0] <= _cap(B * T), f"B.codes: {judged[0]} undecidable positions of {B * T}"
    if z_e is not None and zq_out is not None:
        z_st, _ = _zst32(z_e, inp.cb, codes)
        wsc = inp.w_out.double() * (sc.double().view(D, 1) if sc is not None else 1.0)
        ref = torch.einsum("cd,bdt->bct", wsc, z_st.double()) + inp.b_out.double().view(1, D, 1)
        mag = torch.einsum("cd,bdt->bct", wsc.abs(), z_st.double().abs()) + inp.b_out.double().abs().view(1, D, 1)
        _sum_bound(f"vq_step.{name}.D.zq_out", zq_out, ref, mag, CD + 1, extra=1.0)
    if zq_out is not None and out.residual is not None:
        assert _same_bits(out.residual, inp.x - zq_out), "E.residual is not z_in - zq_out bit for bit"
    if zq_out is not None and out.zq_acc is not None:
        m = mask.view(B, 1, 1) if mask is not None else torch.ones(B, 1, 1)
        assert _same_bits(out.zq_acc, inp.acc0 + zq_out * m), "E.zq_acc is not acc0 + zq_out * mask bit for bit"
    if out.loss_part is not None:
        assert tuple(out.loss_part.shape) == (B, -(-T // 16))
        assert bool(torch.isfinite(out.loss_part).all()), "F.loss_part not finite (a tile the launch skipped?)"
        if z_e is not None:
            ref = _loss_ref(z_e, inp.cb[codes].permute(0, 2, 1))
            _sum_bound(f"vq_step.{name}.F.loss_part", out.loss_part, ref, ref, 128, extra=3.0)
    return judged


# ======================================================================================================= CPU restatement
def _first_argmax(v):
    """First maximum along dim 1 -> (values, indices)."""
    m = v.max(1, keepdim=True).values
    idx = torch.where(v == m, torch.arange(v.shape[1])[None], v.shape[1]).min(1).values
    return m[:, 0], idx


def _search_restated(z_e, cb, route, fault=None):
    """The kernels' search on torch-fp32 distances: per range a strict '>' first-maximum scan, then the tile kernel's ascending
    16-way combine or the small-T kernel's tree with its tie clause.  fault: 'skip_last' (the scan stops one code early), 'ge'
    ('>=' in the combine), 'tree_no_tie' (the tree without its tie clause)."""
    neg = -_dist32(z_e, cb)
    N, Kc = neg.shape
    n, kper = _n_ranges(route), _kper(Kc, route)
    bv = torch.full((N, n), float("-inf"))
    bk = torch.zeros(N, n, dtype=torch.int64)
    for r in range(n):
        k0 = min(Kc, r * kper)
        k1 = min(Kc, k0 + kper)
        bk[:, r] = k0
        if fault == "skip_last":
            k1 -= 1
        if k0 < k1:
            v, i = _first_argmax(neg[:, k0:k1])
            bv[:, r], bk[:, r] = v, k0 + i
    if route == "tile":
        v, k = bv[:, 0].clone(), bk[:, 0].clone()
        for r in range(1, n):
            take = bv[:, r] >= v if fault == "ge" else bv[:, r] > v
            v, k = torch.where(take, bv[:, r], v), torch.where(take, bk[:, r], k)
        return k
    off = 128
    while off:
        av, ak, hv, hk = bv[:, :off], bk[:, :off], bv[:, off:2 * off], bk[:, off:2 * off]
        take = hv > av
        if fault != "tree_no_tie":
            take = take | ((hv == av) & (hk < ak))
        bv, bk = torch.where(take, hv, av), torch.where(take, hk, ak)
        off >>= 1
    return bk[:, 0]


def _restate(inp, route, loss, fault=None):
    """The whole step in torch fp32 on the CPU, as the kernel orders it -> the outputs of a launch.  fault: one of
    `_search_restated`'s, 'mask_on_residual', 'invalid_lane_kept' (a lane past T, whose z_e is b_in, stays in the loss) or
    'last_tile_skipped' (the last (clip, tile) pair keeps the NaN / sentinel fill)."""
    B, D, T = inp.B, inp.D, inp.T
    z_e = torch.einsum("dc,bct->bdt", inp.W, inp.x) + inp.b_in.view(1, CD, 1)
    codes = _search_restated(z_e, inp.cb, route, fault).view(B, T)
    z_st, zq = _zst32(z_e, inp.cb, codes)
    w = inp.w_out * (inp.sc.view(D, 1) if inp.sc is not None else 1.0)
    zq_out = torch.einsum("cd,bdt->bct", w, z_st) + inp.b_out.view(1, D, 1)
    m = inp.mask.view(B, 1, 1)
    residual = inp.x - (zq_out * m if fault == "mask_on_residual" else zq_out)
    zq_acc = inp.acc0 + zq_out * m
    loss_part = None
    if loss:
        loss_part = _loss_ref(z_e, zq).float()
        if fault == "invalid_lane_kept" and T % 16:
            ze_b = inp.b_in.view(1, CD, 1)
            k_b = _search_restated(ze_b, inp.cb, route)
            loss_part[:, -1] += (16 - T % 16) * float(((inp.b_in - inp.cb[k_b[0]]) ** 2).sum())
    out = types.SimpleNamespace(z_e=z_e, codes=codes, zq_out=zq_out, residual=residual, zq_acc=zq_acc, loss_part=loss_part)
    if fault == "last_tile_skipped":
        t0 = (-(-T // 16) - 1) * 16
        for t in (out.z_e, out.zq_out, out.residual):
            t[B - 1, :, t0:] = NAN
        out.codes[B - 1, t0:] = SENTINEL
        if loss:
            out.loss_part[B - 1, -1] = NAN
    return out


# ======================================================================================================= CPU tests
def test_route_and_lds_restatements_match_the_source():
    """The route condition and both LDS formulas above, word for word in vq.hip; the case table reaches both sides of each term of
    the condition, and the figures the header states follow from the formulas."""
    src = open(os.path.join(REPO, "facodec_amd", "csrc", "vq.hip")).read()
    assert "constexpr int VT = 16;" in src and "constexpr int VG = 16;" in src and "constexpr int VQ_CD = 8;" in src
    assert ("const size_t lds = ((size_t)d->Kc * VQ_CD + ((d->Kc + 3) & ~3) + 4 * VQ_CD * VT + VQ_CD * VT + 2 * VG * VT + "
            "(size_t)d->D * VQ_CD) * 4;") in src
    assert "FAC_REQUIRE(lds <= FAC_LDS_MAX," in src
    assert "if (d->T <= 8 && !d->loss_part && d->D <= 4096) {" in src
    assert ("const size_t lds_s = ((size_t)d->Kc * VQ_CD + ((d->Kc + 3) & ~3) + ((d->D + 3) & ~3) + (size_t)d->D * VQ_CD + "
            "4 * VQ_CD + VQ_CD + 512) * 4;") in src
    assert "if (lds_s <= FAC_LDS_MAX) {" in src
    # the small-T kernel carves what lds_s counts, every offset a whole number of float4s
    for line in ("float* cc = cbn + a.Kc * VQ_CD;", "float* xs = cc + ((a.Kc + 3) & ~3);", "float* wsm = xs + ((a.D + 3) & ~3);",
                 "float* part = wsm + a.D * VQ_CD;", "float* zes = part + 4 * VQ_CD;", "float* bestv = zes + VQ_CD;",
                 "int* bestk = reinterpret_cast<int*>(bestv + 256);"):
        assert line in src, line
    assert "const int kper = (a.Kc + VG - 1) / VG;" in src and "const int kper = (a.Kc + 255) / 256;" in src
    assert "if ((blockIdx.x >> 3) >= per_xcd || logical >= a.B * n_tiles) return;" in src
    assert "constexpr size_t FAC_LDS_MAX = 160 * 1024;" in open(os.path.join(REPO, "facodec_amd", "csrc", "common.h")).read()
    r = {c: _route(c[1], c[2], c[3], c[4]) for c in CASES}
    assert all(r[c] == "tile" for c in TILE_CASES) and all(r[c] == "small_t" for c in SMALL_CASES)
    assert [r[c] for c in THRESHOLD_CASES] == ["small_t", "tile", "small_t", "tile", "small_t", "tile", "tile"]
    assert _lds_small(4096, 16) <= LDS_MAX and _lds_small(4097, 16) <= LDS_MAX and _lds_tile(4097, 16) <= LDS_MAX   # D decides there
    assert _lds_small(3465, 1024) <= LDS_MAX < _lds_small(3466, 1024)                                           # the LDS decides here
    assert _lds_tile(3824, 1024) <= LDS_MAX < _lds_tile(3825, 1024) and _route(3825, 3, 1024, False) == "refused"
    assert _route(70, 3, 1000, True) == "tile"                     # loss partials requested: every small_t case has a tile twin
    assert {c[0] * -(-c[2] // 16) for c in TILE_CASES} >= {1, 7, 9, 17}      # grids the padding to a multiple of 8 extends
    assert {c[2] % 16 for c in TILE_CASES} >= {1, 15, 0}
    assert len({_case_id(c) for c in CASES}) == len(CASES)
    lib = _lib.load()
    assert all(lib.fac_vq_loss_tiles(T) == -(-T // 16) for T in (1, 15, 16, 17, 260))


def test_planted_index_lists():
    """The planted rows for both routes, derived from Kc: written out for small codebooks, structural for the shipped size."""
    assert _planted_indices(1024, "tile") == sorted({0, 1023} | {64 * g - 1 for g in range(1, 16)} | {64 * g for g in range(1, 16)})
    assert _planted_indices(1024, "small_t") == sorted({0, 1023} | {4 * t - 1 for t in range(1, 256)} | {4 * t for t in range(1, 256)})
    assert _planted_indices(37, "tile") == [0, 2, 3, 5, 6, 8, 9, 11, 12, 14, 15, 17, 18, 20, 21, 23, 24, 26, 27, 29, 30, 32, 33, 35, 36]
    assert _planted_indices(37, "small_t") == list(range(37))                    # ranges of one code: every row is a boundary
    assert _planted_indices(1000, "tile")[-3:] == [944, 945, 999]                 # 16 ranges of 63, the last holds 55 codes
    assert _planted_indices(1, "tile") == [0]
    assert _planted_pairs(1024, "tile") == {"within": (64, 65), "adjacent": (191, 192), "ends": (0, 1023), "distant": (320, 704)}
    assert _planted_pairs(1024, "small_t") == {"within": (4, 5), "adjacent": (11, 12), "ends": (0, 1023), "distant": (256, 512)}
    for Kc, route in PLANTED_PARAMS:
        kper, pairs = _kper(Kc, route), _planted_pairs(Kc, route)
        flat = [k for p in pairs.values() for k in p]
        assert len(set(flat)) == len(flat) and all(0 <= i < j < Kc for i, j in pairs.values())
        if "within" in pairs:
            assert pairs["within"][0] // kper == pairs["within"][1] // kper
        assert pairs["adjacent"][0] // kper + 1 == pairs["adjacent"][1] // kper
        if "distant" in pairs:
            assert pairs["distant"][1] // kper - pairs["distant"][0] // kper > 1


PLANTED_PARAMS = [(1024, "tile"), (1000, "tile"), (37, "tile"), (1024, "small_t"), (1000, "small_t"), (37, "small_t")]


def _check_planted(inp, planted, near, out):
    """The planted positions of a launch (or of the restatement): z_e is x[:8] bit for bit, the code is the lowest index of the row
    the query is a multiple of -- a decidable position of the rule, asserted --, the near tie gets one of its two rows and zq_out[:, :8] is z_st bit for bit."""
    assert _same_bits(out.z_e, inp.x[:, :CD]), "C.z_e is not x[:8] bit for bit under a one-hot in-projection"
    d = _dist64(out.z_e, inp.cb)
    first = _first_identical(inp.cb)
    k = out.codes.reshape(-1)
    for pos, row in planted:
        others = d[pos][first != first[row]]
        assert float(d[pos, row]) < 1e-12 and (others.numel() == 0 or float(others.min()) >= TAU)
        assert int(k[pos]) == int(first[row]), f"C.planted: the query 3.7 x row {row} got code {int(k[pos])}, not {int(first[row])}"
    if near is not None:
        pos, a, b = near
        third = d[pos][[i for i in range(inp.Kc) if i not in (a, b)]].min()
        assert abs(float(d[pos, a] - d[pos, b])) < TAU and float(third) > float(d[pos, [a, b]].min()) + TAU   # undecidable, and between a and b only
        assert int(k[pos]) in (a, b), f"C.near tie between rows {a} and {b} got code {int(k[pos])}"
    if out.zq_out is not None:
        z_st, _ = _zst32(out.z_e, inp.cb, out.codes)
        assert _same_bits(out.zq_out[:, :CD], z_st), "D.z_st: zq_out under a one-hot out-projection is not z_e + (z_q - z_e) bit for bit"


@pytest.mark.parametrize("Kc,route", PLANTED_PARAMS, ids=[f"{r}_K{k}" for k, r in PLANTED_PARAMS])
def test_planted_faults_in_the_search_restatement_are_caught(Kc, route):
    """The restated search passes the planted checks and the rule; a scan that stops one code early, '>=' in the tile kernel's
    combine and the small-T tree without its tie clause each fail them."""
    for dup in (False, True):
        inp, planted, zero, near = _planted(Kc, route, dup)
        out = _restate(inp, route, route == "tile")
        _check_planted(inp, planted, near, out)
        _check_stages(f"cpu.planted_{route}_K{Kc}_dup{int(dup)}", inp, out, sc=None)
    kper = _kper(Kc, route)
    if kper > 1:                                    # with ranges of one code the early stop empties every range
        inp, planted, zero, near = _planted(Kc, route, False)
        with pytest.raises(AssertionError, match="C.planted"):
            _check_planted(inp, planted, near, _restate(inp, route, False, "skip_last"))
        with pytest.raises(AssertionError, match="B.codes"):
            _judge_codes(inp.x[:, :CD].contiguous(), inp.cb, _restate(inp, route, False, "skip_last").codes)
    inp, planted, zero, near = _planted(Kc, route, True)
    fault = "ge" if route == "tile" else "tree_no_tie"
    if route == "tile" or "distant" in _planted_pairs(Kc, route):
        bad = _restate(inp, route, False, fault)
        with pytest.raises(AssertionError, match="C.planted"):
            _check_planted(inp, planted, near, bad)
        with pytest.raises(AssertionError, match="bit-identical"):
            _judge_codes(bad.z_e, inp.cb, bad.codes)


FAULT_CASE = (5, 72, 17, 1024, True)


def test_planted_faults_in_the_bookkeeping_restatement_are_caught():
    """The restated step passes every stage at a case with T % 16 = 1, a mask with zeros and a bias of at least 0.5 per dimension;
    the mask on the residual, an invalid lane kept in the loss and a skipped last tile each land outside their check.  The loss
    claim separately: one lane's sum of b_in^2 added to a tile's reference is outside that tile's bound."""
    B, D, T, Kc, loss = FAULT_CASE
    inp = _inputs(B, D, T, Kc)
    good = _restate(inp, "tile", True)
    _check_stages("cpu.restated", inp, good)
    with pytest.raises(AssertionError, match="E.residual"):
        _check_stages("cpu.fault", inp, _restate(inp, "tile", True, "mask_on_residual"))
    with pytest.raises(AssertionError, match="F.loss_part"):
        _check_stages("cpu.fault", inp, _restate(inp, "tile", True, "invalid_lane_kept"))
    with pytest.raises(AssertionError):
        _check_stages("cpu.fault", inp, _restate(inp, "tile", True, "last_tile_skipped"))
    with pytest.raises(AssertionError, match="B.codes"):
        _check_stages("cpu.fault", inp, _restate(inp, "tile", True, "skip_last"))
    for c in TILE_CASES:                            # every case with a partial last tile: T % 16 in {1, 15} among them
        if c[2] % 16:
            i = _inputs(*c[:4])
            out = _restate(i, "tile", True)
            ref = _loss_ref(out.z_e, i.cb[out.codes].permute(0, 2, 1))
            bound = (4 * math.sqrt(128) + 3) * EPS32 * ref[:, -1] + 4 * EPS32 * ref[:, -1]
            assert float((i.b_in.double() ** 2).sum()) > 1e3 * float(bound.max()), c


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_fp32_distance_error_and_undecidable_positions_stay_within_the_cap(case):
    """With z_e from torch in fp32: the positions whose fp64 top-2 gap is below TAU stay within the cap at every case of the table,
    the torch-fp32 restatement of the distance is within DELTA of fp64 (DELTA bounds any evaluation with the kernel's roundings),
    and its arg-min obeys the rule."""
    B, D, T, Kc, loss = case
    inp = _inputs(B, D, T, Kc)
    z_e = torch.einsum("dc,bct->bdt", inp.W, inp.x) + inp.b_in.view(1, CD, 1)
    err = float((_dist32(z_e, inp.cb).double() - _dist64(z_e, inp.cb)).abs().max())
    codes = _search_restated(z_e, inp.cb, "tile").view(B, T)
    n_und, worst = _judge_codes(z_e, inp.cb, codes)
    _record(f"vq_step.cpu.{_case_id(case)}", {"fp32_cpu_dist_err_over_eps": err / EPS32, "undecidable": n_und, "worst_excess_over_tau": worst})
    assert err <= DELTA, err / EPS32
    assert n_und <= _cap(B * T), (n_und, B * T)
    assert 19 * EPS32 <= DELTA


def test_references_against_the_oracle():
    """This file's fp64 references, chained over a two-stage RVQ, against the project's fp32 oracle O.rvq_forward at one shape:
    codes equal wherever the rule decides, z_q, latents and the loss to fp32 accuracy."""
    from oracle import facodec_oracle as O
    B, D, T, Kc = 3, 72, 37, 1024
    stages = [_inputs(B, D, T, Kc), _inputs(B + 1, D, T, Kc)]
    sd = {}
    for i, s in enumerate(stages):
        p = f"quantizers.{i}."
        sd.update({p + "in_proj.weight": s.W.view(CD, D, 1), p + "in_proj.bias": s.b_in, p + "codebook.weight": s.cb,
                   p + "out_proj.weight": (s.w_out * s.sc.view(D, 1)).view(D, CD, 1), p + "out_proj.bias": s.b_out})
    z = stages[0].x
    zq_o, codes_o, lat_o, cm_o, _ = O.rvq_forward(z, sd, "", 2, 2)
    res, acc, cm = z.double(), torch.zeros(B, D, T, dtype=torch.float64), 0.0
    for i, s in enumerate(stages):
        z_e = torch.einsum("dc,bct->bdt", s.W.double(), res) + s.b_in.double().view(1, CD, 1)
        assert float((z_e - lat_o[:, CD * i:CD * (i + 1)].double()).abs().max()) < 1e-5
        z_e32 = lat_o[:, CD * i:CD * (i + 1)].contiguous()            # the oracle's own bits decide the oracle's codes
        n_und, _ = _judge_codes(z_e32, s.cb, codes_o[:, i])
        assert n_und <= _cap(B * T)
        zq = s.cb[codes_o[:, i]].permute(0, 2, 1).double()
        cm = cm + float(_loss_ref(z_e32, zq.float()).sum(1).div(CD * T).mean())
        out = torch.einsum("cd,bdt->bct", (s.w_out * s.sc.view(D, 1)).double(), z_e + (zq - z_e)) + s.b_out.double().view(1, D, 1)
        acc, res = acc + out, res - out
    assert float((acc - zq_o.double()).abs().max()) < 1e-5 * float(acc.abs().max())
    assert abs(cm - float(cm_o)) < 1e-5 * cm


def test_vq_fwd_rejects_bad_descriptors_without_gpu():
    """Refusals that launch nothing: a null required pointer, B = 65536, and an in-projection one row too large for the LDS next to
    the shipped codebook (D = 3824 is accepted and run by test_vq_step_stages)."""
    lib = _lib.load()
    d = _lib.VqDesc()
    assert lib.fac_vq_fwd(C.byref(d), None) == -1 and b"null pointer" in lib.fac_last_error()
    fake = C.c_void_p(0x10000)                           # never dereferenced: every check below fails on the host
    required = ("z_in", "w_in", "b_in", "codebook", "w_out", "b_out", "codes")
    for name in required:
        setattr(d, name, fake)
    d.B, d.D, d.T, d.Kc, d.codes_bs = 2, 64, 4, 1024, 4
    for name in required:
        setattr(d, name, None)
        assert lib.fac_vq_fwd(C.byref(d), None) == -1 and b"null pointer" in lib.fac_last_error(), name
        setattr(d, name, fake)
    d.B = 65536
    assert lib.fac_vq_fwd(C.byref(d), None) == -1 and b"B too large" in lib.fac_last_error()
    d.B, d.D = 2, 3825
    assert lib.fac_vq_fwd(C.byref(d), None) == -1 and b"do not fit LDS" in lib.fac_last_error()
    d.D, d.T = 64, 0
    assert lib.fac_vq_fwd(C.byref(d), None) == -1 and b"bad shape" in lib.fac_last_error()


# ======================================================================================================= GPU
OUTPUTS = ("residual", "zq_acc", "zq_out", "z_e", "loss_part")


def _launch(dev, inp, loss, absent=(), alias=False, codes_row=None, mask="given", via="c", dev_weights=None):
    """One fac_vq_fwd launch -> its outputs on the CPU (None where absent).  Every output is a view inside a canary buffer, filled
    with NaN (codes: SENTINEL; zq_acc: acc0) before the launch; afterwards the canaries must be intact, every float output finite
    and every input unchanged.  alias: residual is z_in itself (holding x).  codes_row: codes are that row of a (B, 3, T) tensor.
    mask: 'given' (inp.mask), None, or a tensor.  dev_weights: (w_in, w_out, sc) already on the device (the module's own)."""
    B, D, T, Kc = inp.B, inp.D, inp.T, inp.Kc
    mask = inp.mask if isinstance(mask, str) else mask
    bufs, views = [], {}

    def boxed(name, shape, fill, dtype=torch.float32):
        v, buf, pad = _canary(shape, dev, dtype=dtype)
        if isinstance(fill, torch.Tensor):
            v.copy_(fill)
        else:
            v.fill_(fill)
        bufs.append((name, buf, pad))
        views[name] = v
        return v

    host = {"b_in": inp.b_in, "cb": inp.cb, "b_out": inp.b_out}
    if dev_weights is None:
        host.update({"w_in": inp.w_in, "w_out": inp.w_out})
        if inp.sc is not None and "w_out_scale" not in absent:
            host["sc"] = inp.sc
    if mask is not None:
        host["mask"] = mask
    if not alias:
        host["x"] = inp.x
    on = {k: v.to(dev) for k, v in host.items()}
    if dev_weights is not None:
        on["w_in"], on["w_out"], on["sc"] = dev_weights
        if "w_out_scale" in absent:
            on["sc"] = None
        kept = {k: on[k].clone() for k in ("w_in", "w_out", "sc") if on.get(k) is not None}
    if "residual" not in absent:
        boxed("residual", (B, D, T), inp.x if alias else NAN)
    z_in = views["residual"] if alias else on["x"]
    if "zq_acc" not in absent:
        boxed("zq_acc", (B, D, T), inp.acc0)
    if "zq_out" not in absent:
        boxed("zq_out", (B, D, T), NAN)
    if "z_e" not in absent:
        boxed("z_e", (B, CD, T), NAN)
    nt = -(-T // 16)
    if loss and "loss_part" not in absent:
        boxed("loss_part", (B, nt), NAN)
    if codes_row is None:
        codes = boxed("codes", (B, T), SENTINEL, torch.int64)
    else:
        codes = boxed("codes_all", (B, 3, T), SENTINEL, torch.int64)[:, codes_row]
    if via == "ops":
        from facodec_amd import ops
        ops.vq_step(z_in, on["w_in"], on["b_in"], on["cb"], on["w_out"], on.get("sc"), on["b_out"], codes, residual=views.get("residual"),
                    zq_acc=views.get("zq_acc"), zq_out=views.get("zq_out"), mask=on.get("mask"), z_e=views.get("z_e"),
                    loss_part=views.get("loss_part"))
    else:
        d = _lib.VqDesc()
        d.residual, d.z_in, d.zq_acc, d.zq_out = _p(views.get("residual")), _p(z_in), _p(views.get("zq_acc")), _p(views.get("zq_out"))
        d.w_in, d.b_in, d.codebook, d.w_out = _p(on["w_in"]), _p(on["b_in"]), _p(on["cb"]), _p(on["w_out"])
        d.w_out_scale, d.b_out, d.mask, d.codes = _p(on.get("sc")), _p(on["b_out"]), _p(on.get("mask")), _p(codes)
        d.z_e, d.loss_part = _p(views.get("z_e")), _p(views.get("loss_part"))
        d.codes_bs = codes.stride(0)
        d.B, d.D, d.T, d.Kc = B, D, T, Kc
        _call("fac_vq_fwd", C.byref(d))
    torch.cuda.synchronize()
    for name, buf, pad in bufs:
        assert _canary_intact(buf, pad), f"G.canary of {name} overwritten"
    for k, v in host.items():
        assert _same_bits(on[k], v), f"G.input {k} changed"
    if dev_weights is not None:
        for k, v in kept.items():
            assert _same_bits(on[k], v), f"G.input {k} changed"
    out = types.SimpleNamespace(**{k: (views[k].cpu() if k in views else None) for k in OUTPUTS})
    out.codes = codes.cpu().contiguous()
    out.codes_all = views["codes_all"].cpu() if codes_row is not None else None
    for k in OUTPUTS:
        t = getattr(out, k)
        assert t is None or bool(torch.isfinite(t).all()), f"G.{k} not finite (a position the launch did not write?)"
    assert bool(((out.codes >= 0) & (out.codes < Kc)).all()), "G.codes outside [0, Kc) (a position the launch did not write?)"
    return out


def _assert_same_outputs(a, b, what, names=OUTPUTS + ("codes",)):
    for k in names:
        x, y = getattr(a, k), getattr(b, k)
        if x is not None and y is not None:
            assert _same_bits(x, y), f"G.{what}: {k} differs"


_FULL = {}


def _full_run(dev, case):
    """The launch with every output, once per case for all the tests that compare against it."""
    if case not in _FULL:
        _FULL[case] = _launch(dev, _inputs(*case[:4]), case[4])
    return _FULL[case]


def _check_against_search(dev, inp, out):
    from facodec_amd import ops
    ref = ops.vq_search(_rows(out.z_e).contiguous().to(dev), inp.cb.to(dev)).cpu().view(inp.B, inp.T)
    assert torch.equal(out.codes, ref), "B.codes differ from fac_vq_search on the same z_e bits"


@gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_vq_step_stages(cuda, case):
    """Stages A, B, D, E, F of one launch with every output, the codes against fac_vq_search on the same z_e bits, identical bits on
    a second launch, and for every small_t case the same launch with loss partials -- the tile kernel -- bit-equal in every
    output the two share (and checked stage by stage itself)."""
    B, D, T, Kc, loss = case
    inp = _inputs(B, D, T, Kc)
    name = _case_id(case)
    out = _full_run(cuda, case)
    _check_stages(name, inp, out)
    _check_against_search(cuda, inp, out)
    _assert_same_outputs(out, _launch(cuda, inp, loss), "second launch")
    if _route(D, T, Kc, loss) == "small_t":
        assert _route(D, T, Kc, True) == "tile"
        twin = _launch(cuda, inp, True)
        _assert_same_outputs(out, twin, "small_t against tile")
        _check_stages(name + ".tile_twin", inp, twin)


@gpu
@pytest.mark.parametrize("case,form", FORM_PARAMS, ids=[f"{_case_id(c)}-{f}" for c, f in FORM_PARAMS])
def test_vq_step_forms(cuda, case, form):
    """Each nullable pointer absent in turn: what is still exported keeps the bits of the launch that exported everything (without
    the mask: of a launch with a mask of ones; without the scale: the stages hold with a scale of one, z_e and codes keep their
    bits).  residual aliasing z_in gives the bits of the launch that does not alias; codes written as row 1 of a (B, 3, T) tensor
    leave rows 0 and 2 at the sentinel."""
    B, D, T, Kc, loss = case
    inp = _inputs(B, D, T, Kc)
    full = _full_run(cuda, case)
    name = f"{_case_id(case)}.{form}"
    if form.startswith("no_") and form not in ("no_mask", "no_w_out_scale"):
        out = _launch(cuda, inp, loss, absent=(form[3:],))
        assert getattr(out, form[3:]) is None
        _assert_same_outputs(full, out, form)
        _check_stages(name, inp, out)
    elif form == "no_mask":
        out = _launch(cuda, inp, loss, mask=None)
        _assert_same_outputs(_launch(cuda, inp, loss, mask=torch.ones(B)), out, form)
        _check_stages(name, inp, out, mask=None)
        assert not _same_bits(out.zq_acc, full.zq_acc) and _same_bits(out.residual, full.residual)   # the mask reaches zq_acc alone
    elif form == "no_w_out_scale":
        out = _launch(cuda, inp, loss, absent=("w_out_scale",))
        _check_stages(name, inp, out, sc=None)
        _assert_same_outputs(full, out, form, names=("z_e", "codes", "loss_part"))
        assert not _same_bits(out.zq_out, full.zq_out)
    elif form == "alias":
        _assert_same_outputs(full, _launch(cuda, inp, loss, alias=True), form)
    elif form == "codes_row":
        out = _launch(cuda, inp, loss, codes_row=1)
        _assert_same_outputs(full, out, form)
        assert bool((out.codes_all[:, 0] == SENTINEL).all()) and bool((out.codes_all[:, 2] == SENTINEL).all())
    else:
        _assert_same_outputs(full, _launch(cuda, inp, loss), form)


@gpu
@pytest.mark.parametrize("Kc,route", PLANTED_PARAMS, ids=[f"{r}_K{k}" for k, r in PLANTED_PARAMS])
def test_vq_step_planted_answers(cuda, Kc, route):
    """Stage C through the fused kernel, on the kernel the id names: planted rows at 0, Kc - 1 and both sides of every range
    boundary, then duplicated rows (within a range, across adjacent and distant ranges, at the two ends: the lower index wins), a
    zero query (the code fac_vq_search gives a zero latent), z_e = x[:8] and zq_out[:, :8] = z_st bit for bit."""
    from facodec_amd import ops
    for dup in (False, True):
        inp, planted, zero, near = _planted(Kc, route, dup)
        loss = route == "tile"
        assert _route(inp.D, inp.T, Kc, loss) == route
        out = _launch(cuda, inp, loss)
        _check_planted(inp, planted, near, out)
        _check_stages(f"planted_{route}_K{Kc}_dup{int(dup)}", inp, out, sc=None)
        _check_against_search(cuda, inp, out)
        assert bool((_rows(out.z_e)[zero] == 0).all())
        k0 = ops.vq_search(torch.zeros(1, CD, device=cuda), inp.cb.to(cuda)).cpu()
        assert int(out.codes.reshape(-1)[zero]) == int(k0[0]), "C.zero query"


@gpu
@pytest.mark.parametrize("case", [(4, 70, 37, 1000, True), (2, 70, 3, 1000, False)], ids=_case_id)
def test_vq_step_through_ops(cuda, case):
    """ops.vq_step builds the same descriptor: every output of the C-entry launch bit for bit, with the codes a strided row."""
    B, D, T, Kc, loss = case
    inp = _inputs(B, D, T, Kc)
    out = _launch(cuda, inp, loss, codes_row=2, via="ops")
    _assert_same_outputs(_full_run(cuda, case), out, "ops.vq_step")
    assert bool((out.codes_all[:, :2] == SENTINEL).all())


@gpu
@pytest.mark.parametrize("case", [(3, 256, 37, 1024, True), (3, 256, 4, 1024, False)], ids=_case_id)
def test_vq_step_with_the_modules_weights(cuda, case):
    """VectorQuantize._weights() in the loop: the in-projection packed by pack_conv_weight from weight_v and weight_g, the
    out-projection's weight_v with its fac_wn_scale scale.  z_e is held against the fp64 sum with W = g v / |v| exact; the packed
    weight is fl(v fl(g / fl(sqrt(s)))) with s the fp32 sum of squares over D (at most ceil(D / 256) + 8 roundings deep: one FMA
    chain per thread, six shuffle adds, two more), so it carries a relative error of at most (ceil(D / 256) + 8) / 2 for the root
    of s, 2 for the root's own rounding, 1 for the division and 1 for the product: extra = (ceil(D / 256) + 8) / 2 + 4 in units
    of 2^-24 of every term.  The out-projection is conditioned on the scale the device computed, read back."""
    from facodec_amd import synth
    from facodec_amd.quantize import VectorQuantize
    B, D, T, Kc, loss = case
    q = VectorQuantize(D, Kc, CD).eval()
    sd = synth.load_synthetic(q, seed=11)
    q = q.to(cuda)
    w_in, w_out, sc = q._weights()
    torch.cuda.synchronize()
    v, g = sd["in_proj.weight_v"].double().view(CD, D), sd["in_proj.weight_g"].double().view(CD, 1)
    W64 = g * v / v.norm(dim=1, keepdim=True)
    base = _inputs(B, D, T, Kc)
    inp = _make(base.x, W64.float(), sd["in_proj.bias"].float(), sd["codebook.weight"].float(), sd["out_proj.weight_v"].float().view(D, CD),
                sc.cpu(), sd["out_proj.bias"].float(), base.mask, base.acc0)
    out = _launch(cuda, inp, loss, dev_weights=(w_in, w_out, sc))
    _check_stages(_case_id(case) + ".module", inp, out, W64=W64, extra_A=(-(-D // 256) + 8) / 2 + 4)
    _check_against_search(cuda, inp, out)
