"""The bf16 x 3 resident LSTM forward (lstm_fwd_persist_split_kernel, fac_lstm_layer_fwd_persist_split), its weight pack
(fac_pack_lstm_whh_split), and the two callers above the recurrence kernels -- layers.SLSTM.forward route by route and
streaming._LSTMState.run hop by hop -- each against float64, element by element.

  1. the pack: the layout comment above pack_whh_split_kernel restated as plain index arithmetic (slot -> (row, k)); the kernel
     decomposes a thread index the other way, so a slip in either is not shared.  Bit equality over the whole buffer, which lies
     0xFF-filled between guards.
  2. the kernel through its C entry: the `maps` bar of tests/test_train_kernels_gen.py (`_bar`: 4 x the fp32-CPU error + 4 ulp
     at EVERY element) against `_lstm_fwd_ref` in float64, the same yardstick the fp32 kernels are held to; plus what only this
     kernel has: the split exchange scratch (guards, independence of its previous contents), columns that must not mix, the B
     argument that only gates, the epoch carried from one launch to the next.
  3. SLSTM.forward: float64 restatement of dac/model/encodec.py:272-288 (+ the Snake of fac_lstm_from_time_major), a spy on the
     three recurrence wrappers says which route ran on every layer.
  4. _LSTMState.run: the concatenated hops against the float64 restatement of the whole sequence.

No number in a bound comes from the kernels: the bar is the fp32-CPU evaluation's own error.  What the bar can and cannot see
of the split arithmetic is worked out on the CPU (`test_planted_faults_*`): an emulation of the six-product recurrence in torch
passes it (at 0.8 .. 1.0 e_cpu), the same emulation without one of the 2^-9-class products (hi*mid, mid*hi) or without hi*hi
fails it by three orders of magnitude.  The three 2^-18-class products (mid*mid, lo*hi, hi*lo) are each the size of the largest
product the kernel drops by design, i.e. of fp32 rounding itself: without one of them the emulation lands at 3.6 .. 4.5 e_cpu at
H = 128 and 4.6 .. 6.7 e_cpu at H = 512, on the edge of factor 4, so nothing is asserted about them either way; the kernel
itself measures 1.0 .. 1.2 e_cpu, which such a loss would move visibly in the tolerance report.

Measured on MI355X, worst (GPU error / fp32-CPU error) of each family, in units of the scale the test states (the largest |ref|,
per channel under the Snake); every pair is under 4 e_cpu + 4 ulp with the factor 4 nowhere raised:
  lstm_split_fwd_y            1.8e-7 / 1.8e-7 (H = 1536, B = 32, T = 160); largest ratio 1.23e-7 / 1.10e-7 (H = 512, T = 1)
  lstm_split_fwd_y_last_step  1.4e-7 / 1.2e-7 (H = 1024, B = 32, T = 33); at the last of 160 steps no larger than over all steps
  back to back (T = 3, 2)     1.5e-7 / 1.1e-7
  slstm_fwd                   7.5e-7 / 1.0e-6 (B = 5, no skip, Snake); split route 6.2e-7 / 6.6e-7; largest ratio 1.60e-7 / 1.57e-7
  lstm_state_run              5.0e-8 / 5.0e-8 (B = 32)
Why the bit comparisons stand beside the bar: a build whose last wait of the register window was three loads short (pieces read
while still in flight) stayed inside the bar everywhere, the data having mostly arrived, and was caught at H = 1536, T = 33 by
the scratch-contents, B-argument and single-column comparisons, which differed from run to run.
The 59 tests of this file take 9.3 s in all, the slowest 2.1 s (the benchmark's shape: its fp64 recurrence on the CPU)."""
import ctypes as C
import functools
import os
import re
import types

import pytest
import torch

from facodec_amd import _lib, synth
from test_infer_kernels import _chan_scale, _same_bits, _snake_fwd_ref
from test_train_kernels_gen import CANARY, _bar, _call, _canary, _canary_intact, _lstm_fwd_ref, _lstm_inputs, _p, _pad_cols
from test_weight_packs import _ix, _out_buffer, _rc, _split3

gpu = pytest.mark.gpu
LS_NW = 8                     # waves per workgroup of the split kernel (lstm_persist.hip)
GUARD, GUARD_BYTE = 256, 0xA5   # bytes on either side of the exchange scratch


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ======================================================================================================= 1. the pack
def _index_whh_split(H, fault=None):
    """packed[((ub*8 + w)*NK + s)*3 + plane][lane] holds 8 bf16: element i of that piece is W[row][k] with
    row = (lane%32 / 8)*H + ub*8 + lane%8 (gate-major rows of the A fragment), k = (w*NK + s)*16 + 8*(lane/32) + i, NK = H/128.
    Returns (row, k), each of the buffer's shape without the plane axis: (H/8, 8, NK, 64, 8).
    fault "row_terms_swapped": lane%8 and lane%32/8 change places (rows taken modulo 4H so that the map stays inside W)."""
    NK = H // 128
    ub, w, s, lane, i = _ix(H // 8, LS_NW, NK, 64, 8)
    l31 = lane % 32
    hi, lo = l31 // 8, l31 % 8
    if fault == "row_terms_swapped":
        hi, lo = lo, hi
    row = (hi * H + ub * 8 + lo) % (4 * H)
    k = (w * NK + s) * 16 + 8 * (lane // 32) + i
    return row, k


def _whh_split_layout(w_hh, fault=None):
    """The buffer the pack must write: (H/8, 8, NK, 3, 64, 8) bfloat16."""
    row, k = _index_whh_split(w_hh.shape[1], fault)
    planes = _split3(w_hh[row, k].contiguous())                    # (3, H/8, 8, NK, 64, 8)
    return planes.permute(1, 2, 3, 0, 4, 5).contiguous()


def _whh_split_decode(buf):
    """The inverse through the same map: (3, 4H, H) bfloat16 planes of W."""
    H = buf.shape[0] * 8
    row, k = _index_whh_split(H)
    planes = torch.zeros(3, 4 * H, H, dtype=torch.bfloat16)
    for p in range(3):
        planes[p][row.reshape(-1), k.reshape(-1)] = buf[:, :, :, p].reshape(-1)
    return planes


ALL_PLANES = 1 + 2.0 ** -10 + 2.0 ** -20          # hi 1, mid 2^-10, lo 2^-20
PLANTED = [0.0, -0.0, 1.0, -1.0, 2.0 ** -126, 1 + 2.0 ** -8 + 2.0 ** -16, ALL_PLANES]


def _pack_weights(H):
    """uniform in +-1/sqrt(H) like a real W_hh, with PLANTED in the first elements of row 1 (0, -0, +-1, the smallest normal,
    1 + 2^-8 + 2^-16 whose hi rounds UP to 1 + 2^-7, and a value with three non-zero planes), row 5 holding its column index and
    column 9 its row index, so a transposition shows."""
    gen = _g(77 + H)
    w = (torch.rand(4 * H, H, generator=gen) * 2 - 1) / H ** 0.5
    w[5, :] = torch.arange(H, dtype=torch.float32)
    w[:, 9] = torch.arange(4 * H, dtype=torch.float32)
    w[1, :len(PLANTED)] = torch.tensor(PLANTED)
    return w.contiguous()


def _pack_compare(got, w_hh):
    """What the GPU test asserts of a pack output `got` (H/8, 8, NK, 3, 64, 8) bfloat16; returns the failures."""
    fails = []
    want = _whh_split_layout(w_hh)
    g16, w16 = got.contiguous().view(torch.int16), want.view(torch.int16)
    if bool((g16 == -1).any()):
        fails.append(f"{int((g16 == -1).sum())} bf16 slots still hold the 0xFF fill")
    if not _same_bits(got, want):
        bad = (g16 != w16).reshape(-1)
        fails.append(f"{int(bad.sum())} of {bad.numel()} slots differ from the documented layout, first at {int(bad.nonzero()[0])}")
    return fails


PACK_H = [128, 384, 512, 1536]


@pytest.mark.parametrize("H", PACK_H)
def test_pack_restatement_round_trips(H):
    """The restated map is a bijection between slots and elements of W; decoded through it the three planes sum to W within
    2^-24 |w| at every element (the split keeps 24 bits) and plane 0 is w.bfloat16()."""
    w = _pack_weights(H)
    row, k = _index_whh_split(H)
    assert row.shape == (H // 8, LS_NW, H // 128, 64, 8)
    flat = (row * H + k).reshape(-1)
    assert flat.numel() == 4 * H * H and torch.equal(flat.sort().values, torch.arange(4 * H * H))
    buf = _whh_split_layout(w)
    assert buf.numel() * 2 == 6 * 4 * H * H
    planes = _whh_split_decode(buf)
    assert _same_bits(planes[0], w.bfloat16())
    err = (planes.double().sum(0) - w.double()).abs()
    assert bool((err <= 2.0 ** -24 * w.double().abs()).all()), float((err / w.double().abs().clamp_min(1e-300)).max())
    p = planes[:, 1, PLANTED.index(ALL_PLANES)].double()
    assert bool((p != 0).all()) and float(p.sum()) == ALL_PLANES
    assert not _pack_compare(buf, w)


def test_planted_fault_in_the_pack_restatement_is_caught():
    """lane%8 and lane%32/8 swapped in the row formula: the comparison the GPU test makes fails, and so does the decode."""
    for H in (128, 384):
        w = _pack_weights(H)
        bad = _whh_split_layout(w, fault="row_terms_swapped")
        assert any("differ from the documented layout" in f for f in _pack_compare(bad, w))
        assert not _same_bits(_whh_split_decode(bad)[0], w.bfloat16())


def test_pack_refuses_what_it_cannot_tile():
    """H = 0 and H = 192 (no multiple of 128): non-zero return and a message, nothing launched."""
    host = torch.zeros(64)
    for H in (0, 192):
        rc, msg = _rc("fac_pack_lstm_whh_split", _p(host), _p(host), H, C.c_void_p(0))
        assert rc != 0 and "pack_lstm_whh_split: H must be a multiple of 128" in msg, (H, rc, msg)
    rc, msg = _rc("fac_pack_lstm_whh_split", C.c_void_p(0), _p(host), 128, C.c_void_p(0))
    assert rc != 0 and "pack_lstm_whh_split" in msg


@gpu
@pytest.mark.parametrize("H", PACK_H)
def test_pack_lstm_whh_split_writes_the_documented_layout(cuda, H):
    """fac_pack_lstm_whh_split into a 0xFF-filled buffer between canaries: all 6 * 4H * H bytes written, guards intact, the input
    unchanged, the bytes those of the restatement; ops.pack_lstm_whh_split returns the same bytes."""
    from facodec_amd import ops
    w = _pack_weights(H)
    w_d = w.to(cuda)
    nbytes = 6 * 4 * H * H
    out, buf, pad = _out_buffer(cuda, "wn_scale", (nbytes // 4,))
    _call("fac_pack_lstm_whh_split", _p(w_d), _p(out), H)
    torch.cuda.synchronize()
    assert _canary_intact(buf, pad), "wrote outside its buffer"
    assert _same_bits(w_d, w), "the input changed"
    shape = (H // 8, LS_NW, H // 128, 3, 64, 8)
    fails = _pack_compare(out.cpu().view(torch.bfloat16).view(shape), w)
    assert not fails, fails
    wrapped = ops.pack_lstm_whh_split(w_d)
    assert wrapped.dtype == torch.uint8 and wrapped.numel() == nbytes
    assert torch.equal(wrapped.cpu(), out.cpu().view(torch.uint8))


# ======================================================================================================= 2. the kernel
# smallest terms first (the kernel's TA / TB): mid*mid, lo*hi, hi*lo, mid*hi, hi*mid, hi*hi; planes 0 = hi, 1 = mid, 2 = lo
TERMS = ((1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0))


def _lstm_emul(pre, w_hh, dtype, split=False, drop=None, lag=1):
    """`_lstm_fwd_ref`'s recurrence with two switches.  split: W_hh . h as the kernel forms it, both operands split into three
    bf16 planes (`_split3`), the products of TERMS (without index `drop`) accumulated in fp32.  lag: the step whose h feeds step
    t is t - lag (2 is the fault of the self-check).  Returns y (H, T, N)."""
    pre, w = pre.to(dtype), w_hh.to(dtype)
    H = w.shape[1]
    _, T, N = pre.shape
    wp = _split3(w_hh.contiguous()).float() if split else None
    c = torch.zeros(H, N, dtype=dtype)
    hist = [torch.zeros(H, N, dtype=dtype)] * lag
    ys = []
    for t in range(T):
        h = hist[-lag]
        if split:
            hp = _split3(h.float().contiguous()).float()
            rec = torch.zeros(4 * H, N)
            for q, (a, b) in enumerate(TERMS):
                if q != drop:
                    rec = rec + wp[a] @ hp[b]
            z = pre[:, t] + rec.to(dtype)
        else:
            z = pre[:, t] + w @ h
        i, f, o = torch.sigmoid(z[:H]), torch.sigmoid(z[H:2 * H]), torch.sigmoid(z[3 * H:])
        g = torch.tanh(z[2 * H:3 * H])
        c = f * c + i * g
        h = o * torch.tanh(c)
        hist.append(h)
        ys.append(h)
    return torch.stack(ys, 1)


def _plant(pre):
    """The three planted real columns: 0 saturates every gate (+20: c grows by 1 a step, h reaches exactly 1.0 = planes (1, 0, 0)),
    1 closes the output gate (pre_o = -30: h ~ 1e-14, far below the other columns), 2 is all zero (h = 0 exactly at every step).
    |pre| <= 30 keeps every bf16 plane of h normal, so the matrix pipe's flushing of denormals cannot enter the comparison."""
    H = pre.shape[0] // 4
    pre = pre.clone()
    pre[:, :, 0] = 20.0
    pre[3 * H:, :, 1] = -30.0
    pre[:, :, 2] = 0.0
    assert float(pre.abs().max()) <= 30.0
    return pre


@functools.lru_cache(maxsize=1)
def _split_case(H, B, T):
    """(pre with the planted columns, w_hh, y float64, y fp32-CPU).  The random part and its references are `_lstm_inputs`' (one
    key of which the existing table shares); the recurrence never mixes columns, so only the planted ones are evaluated again."""
    pre, w_hh, _, ref64, ref32 = _lstm_inputs(H, B, T)
    pre = _plant(pre)
    y64, y32 = ref64[0].clone(), ref32[0].clone()
    y64[..., :3] = _lstm_fwd_ref(pre[..., :3], w_hh, torch.float64)[0]
    y32[..., :3] = _lstm_fwd_ref(pre[..., :3], w_hh, torch.float32)[0]
    return pre, w_hh, y64, y32


def _split_ok(H, B):
    from facodec_amd import ops
    ops._lstm_arm()
    lib = _lib.load()
    return bool(lib.fac_lstm_persist_split_ok(H, B)) and bool(lib.fac_lstm_persist_stream_ok(ops._stream()))


def _scratch(cuda, T, H, fill):
    """The exchange scratch, exactly T * H * 32 * 6 bytes of `fill` between two guards: (view, whole buffer)."""
    n = T * H * 32 * 6
    buf = torch.full((n + 2 * GUARD,), GUARD_BYTE, device=cuda, dtype=torch.uint8)
    view = buf[GUARD:GUARD + n]
    view.fill_(fill)
    assert view.data_ptr() % 16 == 0
    return view, buf


def _guards_intact(buf):
    c = buf.cpu()
    return bool((c[:GUARD] == GUARD_BYTE).all()) and bool((c[-GUARD:] == GUARD_BYTE).all())


def _run_split(cuda, pre_d, wsplit, T, H, B, BP, fill=0xFF):
    """One launch into fresh buffers: yT (H, T, BP) inside canaries, the scratch pre-filled with `fill` inside guards."""
    yT, ybuf, pad = _canary((H, T, BP), cuda)
    hs, hbuf = _scratch(cuda, T, H, fill)
    _call("fac_lstm_layer_fwd_persist_split", _p(pre_d), _p(wsplit), _p(hs), _p(yT), T, H, B, BP)
    torch.cuda.synchronize()
    assert _canary_intact(ybuf, pad), "wrote outside yT"
    assert _guards_intact(hbuf), "wrote outside the exchange scratch"
    return yT.cpu()


def _pack_split(cuda, w_hh):
    w_d = w_hh.to(cuda)
    wsplit = torch.empty(6 * w_d.numel(), device=cuda, dtype=torch.uint8)
    _call("fac_pack_lstm_whh_split", _p(w_d), _p(wsplit), w_hh.shape[1])
    return wsplit


# (H, B, T, what the case reaches).  NK = H / 128 MFMA steps per wave against a register window of 4: NK = 4 never refills it,
# NK = 8 refills every slot once, NK = 12 twice.  T = 1 has no exchange, T = 2 one (and nothing published at the last step), T = 3
# two regions in flight.  B = 5 is inside the kernel (persist_split_shape_ok) though ops.lstm_persist_split_ok never sends it there.
SPLIT_CASES = [
    (512, 17, 1, "no_exchange"), (512, 32, 2, "one_exchange"), (512, 20, 3, "two_regions"), (1024, 17, 5, "NK8_one_refill"),
    (1024, 32, 33, "NK8"), (1536, 32, 2, "NK12"), (1536, 24, 33, "NK12_slots_reused_twice"), (1536, 32, 160, "bench_shape"),
    (512, 5, 9, "B_below_policy"),
]
BP64 = {(512, 20, 3), (1024, 17, 5), (1536, 32, 2)}
SPLIT_PARAMS = [(c, bp) for c in SPLIT_CASES for bp in (32, 64) if bp == 32 or c[:3] in BP64]      # a case's two widths share its inputs


def _split_id(case, BP):
    H, B, T, what = case
    return f"H{H}_B{B}_T{T}_BP{BP}_{what}"


@gpu
@pytest.mark.parametrize("case,BP", SPLIT_PARAMS, ids=[_split_id(c, bp) for c, bp in SPLIT_PARAMS])
def test_lstm_layer_fwd_persist_split(cuda, case, BP):
    """fac_lstm_layer_fwd_persist_split of ONE layer, the `resident_split` counterpart of test_lstm_layer_fwd_train_and_bptt: yT
    against the fp64 recurrence under `_bar` (factor 4) at every element of the real columns, again at the last step with the
    whole-sequence scale; padded columns B..31 exactly 0; columns >= 32 of a 64-column buffer untouched; canaries around yT and
    guards around the exactly-sized scratch; pre unchanged; no timed-out wait.  Then what the output may NOT depend on: the
    scratch's previous contents (0xFF = NaN in every plane, against zeros), the B argument (17 against 32), the other columns (one
    real column alone reproduces its bits in the full launch)."""
    from facodec_amd import ops
    H, B, T, _ = case
    if not _split_ok(H, B):
        pytest.skip("fac_lstm_persist_split_ok == 0 on this device")
    pre, w_hh, y64, y32 = _split_case(H, B, T)
    pre_p = _pad_cols(pre, BP)
    if BP > 32:
        pre_p[..., 32:] = 7.0                                  # nothing there is the kernel's business
    pre_d = pre_p.to(cuda)
    wsplit = _pack_split(cuda, w_hh)
    y = _run_split(cuda, pre_d, wsplit, T, H, B, BP, fill=0xFF)
    assert ops.lstm_timeouts() == 0
    assert _same_bits(pre_d, pre_p), "pre changed"
    assert bool(torch.isfinite(y).all())
    assert bool((y[..., B:32] == 0).all()), "padded columns (pre = 0) must stay exactly 0"
    assert bool((y[..., 32:] == CANARY).all()), "columns >= 32 were written"
    assert bool((y[..., 2] == 0).all()), "the all-zero planted column must stay exactly 0"
    fails = []

    def check(fn, *a, **k):
        try:
            fn(*a, **k)
        except AssertionError as e:
            fails.append(str(e)[:400])

    tag = _split_id(case, BP)
    check(_bar, f"lstm_split_fwd_y_{tag}", y[..., :B], y64, y32)
    check(_bar, f"lstm_split_fwd_y_last_step_{tag}", y[:, T - 1, :B], y64[:, T - 1], y32[:, T - 1],
          scale=y64.abs().max().expand_as(y64[:, T - 1]))
    # ---- the scratch's previous contents
    y0 = _run_split(cuda, pre_d, wsplit, T, H, B, BP, fill=0x00)
    if not torch.equal(y0, y):
        fails.append("yT depends on what the exchange scratch held before the launch")
    # ---- B only gates the shape
    for B2 in {5, 17, 32} - {B}:
        if not torch.equal(_run_split(cuda, pre_d, wsplit, T, H, B2, BP), y):
            fails.append(f"launched with B = {B2} the same pre gives other bits than with B = {B}")
    # ---- columns do not mix
    for c in (0, 15, 16, 31):
        if c >= B:
            continue
        alone = torch.zeros_like(pre_p)
        alone[..., c] = pre_p[..., c]
        yc = _run_split(cuda, alone.to(cuda), wsplit, T, H, B, BP)
        if not torch.equal(yc[..., c], y[..., c]):
            fails.append(f"column {c} alone differs from column {c} of the full launch")
        others = [j for j in range(32) if j != c]
        if not bool((yc[..., others] == 0).all()):
            fails.append(f"column {c} alone leaks into other columns")
    assert ops.lstm_timeouts() == 0
    assert not fails, fails


@gpu
@pytest.mark.parametrize("H", [512, 1536])
def test_split_launches_back_to_back_carry_the_epoch(cuda, H):
    """T = 3, then T = 2, on one stream with no synchronisation between, on the SAME scratch and output memory: each equals its
    own fresh-buffer launch.  The flags of the first launch must all lie below the second one's targets (the epoch advances by T)."""
    B, BP = 20, 32
    if not _split_ok(H, B):
        pytest.skip("fac_lstm_persist_split_ok == 0 on this device")
    from facodec_amd import ops
    pre3 = _pad_cols(_plant(torch.randn(4 * H, 3, B, generator=_g(H + 3))), BP)
    pre2 = _pad_cols(_plant(torch.randn(4 * H, 2, B, generator=_g(H + 2))), BP)
    w_hh = (torch.rand(4 * H, H, generator=_g(H)) * 2 - 1) / H ** 0.5
    wsplit = _pack_split(cuda, w_hh)
    p3, p2 = pre3.to(cuda), pre2.to(cuda)
    fresh3 = _run_split(cuda, p3, wsplit, 3, H, B, BP)
    fresh2 = _run_split(cuda, p2, wsplit, 2, H, B, BP)
    ymem, ybuf, pad = _canary((H, 3, BP), cuda)
    hs, hbuf = _scratch(cuda, 3, H, 0xFF)
    y3 = ymem
    y2 = ymem.view(-1)[:H * 2 * BP].view(H, 2, BP)
    _call("fac_lstm_layer_fwd_persist_split", _p(p3), _p(wsplit), _p(hs), _p(y3), 3, H, B, BP)
    got3 = y3.clone()
    _call("fac_lstm_layer_fwd_persist_split", _p(p2), _p(wsplit), _p(hs), _p(y2), 2, H, B, BP)
    torch.cuda.synchronize()
    assert ops.lstm_timeouts() == 0
    assert _canary_intact(ybuf, pad) and _guards_intact(hbuf)
    assert torch.equal(got3.cpu(), fresh3), "first launch (T = 3)"
    assert torch.equal(y2.cpu(), fresh2), "second launch (T = 2) on the first one's scratch"
    for y_, pre_ in ((fresh3, pre3), (fresh2, pre2)):
        r64 = _lstm_fwd_ref(pre_[..., :B], w_hh, torch.float64)[0]
        r32 = _lstm_fwd_ref(pre_[..., :B], w_hh, torch.float32)[0]
        _bar(f"lstm_split_fwd_y_back_to_back_H{H}_T{pre_.shape[1]}", y_[..., :B], r64, r32)


def test_split_entry_refuses_before_any_device_query():
    """Null pointers, T = 0, BP = 16, BP = 48, BP < B and H = 768: non-zero return and a message; the entry checks these before
    it asks the device anything, so this runs without one."""
    host = torch.zeros(64)
    a, null = _p(host), C.c_void_p(0)
    name = "fac_lstm_layer_fwd_persist_split"
    for i in range(4):
        ptrs = [a, a, a, a]
        ptrs[i] = null
        rc, msg = _rc(name, *ptrs, 2, 512, 17, 32, null)
        assert rc != 0 and "lstm_layer_fwd_persist_split: null pointer" in msg, (i, rc, msg)
    for T, H, B, BP in ((0, 512, 17, 32), (2, 512, 5, 16), (2, 512, 17, 48), (2, 512, 40, 32), (2, 512, 33, 32)):
        rc, msg = _rc(name, a, a, a, a, T, H, B, BP, null)
        assert rc != 0 and "lstm_layer_fwd_persist_split: bad T / BP" in msg, (T, H, B, BP, rc, msg)
    rc, msg = _rc(name, a, a, a, a, 2, 768, 17, 32, null)
    assert rc != 0 and "H=768 B=17 is outside the kernel" in msg, (rc, msg)


EMUL = (128, 4, 6)              # H, B, T of the CPU self-checks


@functools.lru_cache(maxsize=1)
def _emul_inputs():
    H, B, T = EMUL
    gen = _g(5)
    pre = _plant(torch.randn(4 * H, T, B, generator=gen))
    w = (torch.rand(4 * H, H, generator=gen) * 2 - 1) / H ** 0.5
    return pre, w, _lstm_fwd_ref(pre, w, torch.float64)[0], _lstm_fwd_ref(pre, w, torch.float32)[0]


def test_six_product_recurrence_emulated_in_torch_passes_the_bar():
    """The emulation is `_lstm_fwd_ref` when its switches are off (same bits, both precisions), and with the kernel's arithmetic
    -- three bf16 planes per operand, six products, fp32 accumulation -- it is inside the bar the GPU test applies.  This is where
    the expectation "factor 4 holds" comes from; the kernel is not asked."""
    pre, w, y64, y32 = _emul_inputs()
    assert torch.equal(_lstm_emul(pre, w, torch.float64), y64) and torch.equal(_lstm_emul(pre, w, torch.float32), y32)
    _bar("cpu.lstm_split_emulated", _lstm_emul(pre, w, torch.float32, split=True), y64, y32)


@pytest.mark.parametrize("drop", [3, 4, 5], ids=["mid*hi", "hi*mid", "hi*hi"])
def test_planted_fault_a_dropped_product_is_caught(drop):
    """One of the six products left out of the term table: outside the bar for every product above the 2^-18 class (module
    docstring)."""
    pre, w, y64, y32 = _emul_inputs()
    with pytest.raises(AssertionError, match="cpu.fault"):
        _bar("cpu.fault", _lstm_emul(pre, w, torch.float32, split=True, drop=drop), y64, y32)


def test_planted_fault_a_reference_that_reads_h_two_steps_back_is_caught():
    """h_{t-2} for h_{t-1} (a region read before it is published would look like this): outside the bar, in the plain and in the
    six-product form."""
    pre, w, y64, y32 = _emul_inputs()
    for split in (False, True):
        with pytest.raises(AssertionError, match="cpu.fault"):
            _bar("cpu.fault", _lstm_emul(pre, w, torch.float32, split=split, lag=2), y64, y32)


# ======================================================================================================= 3. SLSTM.forward
SL_H, SL_L, SL_T = 512, 2, 9


def _slstm_ref(x, sd, dtype, skip=True, alpha=None, prefix="lstm.", num_layers=SL_L):
    """dac/model/encodec.py:272-288 restated on the work-buffer layout: per layer pre = W_ih x + (b_ih + b_hh), then
    `_lstm_fwd_ref`; + x when skip; then the Snake of fac_lstm_from_time_major when alpha is given.  x (B, H, T) -> (B, H, T)."""
    seq = x.to(dtype)
    inp = seq.permute(1, 2, 0)                                   # (H, T, B)
    for l in range(num_layers):
        w_ih, w_hh = sd[f"{prefix}weight_ih_l{l}"].to(dtype), sd[f"{prefix}weight_hh_l{l}"]
        bias = sd[f"{prefix}bias_ih_l{l}"].to(dtype) + sd[f"{prefix}bias_hh_l{l}"].to(dtype)
        pre = torch.einsum("gh,htb->gtb", w_ih, inp) + bias.view(-1, 1, 1)
        inp = _lstm_fwd_ref(pre, w_hh, dtype)[0]
    y = inp.permute(2, 0, 1)
    if skip:
        y = y + seq
    return y if alpha is None else _snake_fwd_ref(y, alpha, dtype)


def test_slstm_restatement_against_the_oracle():
    """The float64 restatement is oracle.facodec_oracle.slstm's function (which adds the two biases at other places of the sum)."""
    from facodec_amd.layers import SLSTM
    from oracle import facodec_oracle as O
    H, B, T = 64, 3, 5
    sd = synth.load_synthetic(SLSTM(H, 2), seed=5)
    x = torch.randn(B, H, T, generator=_g(1))
    want = O.slstm(x.double(), {k: v.double() for k, v in sd.items()}, "lstm.", 2)
    got = _slstm_ref(x, sd, torch.float64)
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
    core = _slstm_ref(x, sd, torch.float64, skip=False)
    assert torch.equal(core + x.double(), got) and torch.equal(_finish(core, x, torch.float64, True, None), got)
    alpha = 1 + 0.2 * torch.rand(H, generator=_g(2))
    assert torch.equal(_finish(core, x, torch.float64, True, alpha), _slstm_ref(x, sd, torch.float64, alpha=alpha))
    snaked = O.snake(want, alpha.double().view(1, -1, 1))
    assert float((_slstm_ref(x, sd, torch.float64, alpha=alpha) - snaked).abs().max()) <= 1e-13 * float(snaked.abs().max())


@functools.lru_cache(maxsize=4)
def _slstm_case(B):
    from facodec_amd.layers import SLSTM
    m = SLSTM(SL_H, SL_L)
    sd = synth.load_synthetic(m, seed=5)
    x = torch.randn(B, SL_H, SL_T, generator=_g(SL_H + B))
    gen = _g(B)
    alpha = 1 + 0.2 * torch.rand(SL_H, generator=gen)
    alpha[0] = 1.0
    core = {dt: _slstm_ref(x, sd, dt, skip=False) for dt in (torch.float64, torch.float32)}
    return m, sd, x, alpha, core


def _finish(core, x, dtype, skip, alpha):
    y = core + x.to(dtype) if skip else core
    return y if alpha is None else _snake_fwd_ref(y, alpha, dtype)


SCRATCH_9 = SL_T * SL_H * 32 * 6
# (id, B, LSTM_PERSIST, scratch cap or None, the wrapper that must run on every layer)
ROUTES = [
    ("B5_fp32_resident", 5, True, None, "lstm_layer_persist"),
    ("B17_split", 17, True, None, "lstm_layer_persist_split"),
    ("B32_split", 32, True, None, "lstm_layer_persist_split"),
    ("B32_persist_off_per_step", 32, False, None, "lstm_layer"),
    ("B17_scratch_cap_one_byte_short", 17, True, SCRATCH_9 - 1, "lstm_layer"),
    ("B17_scratch_cap_exact", 17, True, SCRATCH_9, "lstm_layer_persist_split"),
]


@gpu
@pytest.mark.parametrize("with_alpha", [False, True], ids=["alpha_none", "alpha"])
@pytest.mark.parametrize("skip", [True, False], ids=["skip", "noskip"])
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_slstm_forward_route_by_route(cuda, monkeypatch, route, skip, with_alpha):
    """SLSTM.forward (input projection through ops.lstm_input_proj, two layers, skip, the Snake of fac_lstm_from_time_major) under
    `_bar` against the float64 restatement, per-channel scale under the Snake; a spy on the three recurrence wrappers asserts
    the route of EVERY layer."""
    from facodec_amd import ops
    rid, B, persist, cap, want = route
    ops._lstm_arm()
    lib = _lib.load()
    if want == "lstm_layer_persist" and not lib.fac_lstm_persist_ok(SL_H, B):
        pytest.skip("fac_lstm_persist_ok == 0 on this device")
    if want == "lstm_layer_persist_split" and not _split_ok(SL_H, B):
        pytest.skip("fac_lstm_persist_split_ok == 0 on this device")
    monkeypatch.setattr(ops, "LSTM_PERSIST", persist)
    monkeypatch.setattr(ops, "LSTM_PERSIST_MAX_BATCH", 16)
    monkeypatch.setattr(ops, "LSTM_PERSIST_SPLIT", True)
    monkeypatch.setattr(ops, "BF16_SPLIT", True)
    if cap is not None:
        monkeypatch.setattr(ops, "LSTM_PERSIST_SPLIT_MAX_SCRATCH", cap)
    ran = []
    for name in ("lstm_layer_persist_split", "lstm_layer_persist", "lstm_layer"):
        def spy(*a, _name=name, _real=getattr(ops, name), **k):
            ran.append(_name)
            return _real(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    m, sd, x, alpha, core = _slstm_case(B)
    m = m.to(cuda)
    m.skip = skip
    a = alpha if with_alpha else None
    with torch.no_grad():
        y = m(x.to(cuda), alpha_out=a.to(cuda) if with_alpha else None)
    torch.cuda.synchronize()
    assert ops.lstm_timeouts() == 0
    assert ran == [want] * SL_L, ran
    assert y.shape == x.shape
    r64, r32 = (_finish(core[dt], x, dt, skip, a) for dt in (torch.float64, torch.float32))
    _bar(f"slstm_fwd_{rid}_{'skip' if skip else 'noskip'}_{'alpha' if with_alpha else 'alpha_none'}", y, r64, r32,
         scale=_chan_scale(r64) if with_alpha else None)


# ======================================================================================================= 4. _LSTMState.run
STREAM_CASES = [(1, (1, 1, 2, 4, 5), "few_and_general"), (2, (1, 2, 3), "few_up_to_4_columns_then_general"), (32, (4, 5), "never_few")]


@gpu
@pytest.mark.parametrize("B,hops,what", STREAM_CASES, ids=[f"B{b}_{w}" for b, _, w in STREAM_CASES])
def test_lstm_state_run_hop_by_hop(cuda, B, hops, what):
    """streaming._LSTMState.run fed one sequence in hops: the concatenated outputs under `_bar` against the float64 restatement of
    the WHOLE sequence (the state carried across hops, `step0` of both parities selecting both h buffers, the "few columns"
    projection through permuted views and the general one), c[0] = frames pushed after every hop, and a second carrier over the
    same hops gives the same bits."""
    from facodec_amd import ops
    from facodec_amd.layers import SLSTM
    from facodec_amd.streaming import _LSTMState
    T = sum(hops)
    m = SLSTM(SL_H, SL_L)
    sd = synth.load_synthetic(m, seed=7)
    m = m.to(cuda)
    x = torch.randn(B, SL_H, T, generator=_g(100 + B))
    x_d = x.to(cuda)
    few = [t * B <= 4 and B < 32 for t in hops]
    assert any(few) == (B < 32) and not all(few), "the hops must reach the branches the id names"

    def run():
        sess = types.SimpleNamespace(device=cuda, _counters=[])
        st = _LSTMState(sess, m, B)
        assert sess._counters == [st] and st.c == [0]
        outs, t0 = [], 0
        with torch.no_grad():
            for n in hops:
                outs.append(st.run(x_d[:, :, t0:t0 + n].contiguous(), None))
                t0 += n
                assert st.c[0] == t0
        torch.cuda.synchronize()
        return torch.cat(outs, dim=2).cpu()

    y = run()
    assert ops.lstm_timeouts() == 0
    assert torch.equal(run(), y), "a second carrier over the same hops gives other bits"
    _bar(f"lstm_state_run_B{B}_{what}", y, _slstm_ref(x, sd, torch.float64), _slstm_ref(x, sd, torch.float32))


def test_entry_points_of_this_file_are_declared():
    """The C entries this file drives are declared in include/facodec_hip.h and bound in facodec_amd/_lib.py."""
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "facodec_hip.h")).read()
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "fac_adamw_step" in v)
    for n in ("fac_pack_lstm_whh_split", "fac_lstm_layer_fwd_persist_split", "fac_lstm_persist_split_ok"):
        assert n in table and re.search(r"int %s\(" % n, header), n
