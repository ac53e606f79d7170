"""The generator side of the training step, one kernel at a time against fp64: the LSTM recurrence with its saves and BPTT
(lstm.hip, lstm_persist.hip), the optimiser (optim.hip), the quantizer / Snake / weight-norm / bias backward kernels
(conv1d_bwd.hip) and the predictor- and quantizer-side glue (train_pred.hip, train_quant.hip, train_misc.hip).

Every reference is a plain float64 restatement of the documented semantics (include/facodec_hip.h, the kernel comments,
oracle/facodec_oracle.py), computed from the same fp32 inputs.  Three kinds of bound:
  exact       copies, selections, fp32 expressions the header defines, untouched regions, canaries, run-to-run determinism;
  reductions  |got - ref64| <= c sqrt(n) 2^-24 sum|terms| + a few ulp, c as in tests/test_train_kernels.py;
  maps        elementwise transcendental maps and the recurrences: the SAME formula is evaluated in fp32 by torch on the CPU,
              its error against fp64 is the reference's own fp32 error e_cpu, and the kernel must stay within 4 e_cpu + 4 ulp
              (`_bar`).  The factor covers another legitimate evaluation order, fast exp / sin and the MFMA accumulation
              order of W_hh h; a missing term shows at 1e-3 or worse.
Every (GPU error, fp32-CPU error) pair goes to the tolerance report of tests/test_gpu_parity.py through `_record`."""
import ctypes as C
import functools
import math
import os

import pytest
import torch

from facodec_amd import _lib

gpu = pytest.mark.gpu
EPS32 = 2.0 ** -24
ULP = 2.0 ** -23
CANARY = 12345.0


def _record(name, value):
    """Measured errors next to the fp32-CPU errors they are held against, through the tolerance report of tests/test_gpu_parity.py
    (its `_record`: one file and one dictionary for both modules, the same keys-per-test style)."""
    from test_gpu_parity import _record as record
    record(name, value)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _p(t):
    """Raw pointer for a C entry; callers keep the tensor alive in a variable until the launch is enqueued."""
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _call(name, *args):
    from facodec_amd import ops
    _lib.check(getattr(_lib.load(), name)(*args, ops._stream()), name)


def _canary(shape, dev, pad=64, dtype=torch.float32):
    """An output tensor inside a canary-filled buffer: (view, buffer, pad); pad = 64 elements keeps the view 16-byte aligned."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * pad,), CANARY, device=dev, dtype=dtype)
    return buf[pad:pad + n].view(*shape), buf, pad


def _canary_intact(buf, pad):
    c = buf.cpu()
    return bool((c[:pad] == CANARY).all()) and bool((c[-pad:] == CANARY).all())


def _check_adjoint(x, fwd_out, y, bwd_out):
    """<fwd(x), y> == <x, bwd(y)> in fp64."""
    fwd_out, y, x, bwd_out = (t.detach().double().cpu().reshape(-1) for t in (fwd_out, y, x, bwd_out))
    lhs = float((fwd_out * y).sum())
    rhs = float((x * bwd_out).sum())
    mag = float((x.abs() * bwd_out.abs()).sum())
    assert abs(lhs - rhs) <= 8 * EPS32 * mag, (lhs, rhs, mag)


def _bar(name, got, ref64, ref32, scale=None, factor=4.0):
    """The `maps` bound: |got - ref64| <= factor * e_cpu * scale + 4 ulp |ref64| at EVERY element, where e_cpu is the worst error
    of the fp32-CPU evaluation in units of `scale` (elementwise tensor, or the largest |ref64| when None).  Records and returns
    (e_gpu, e_cpu), both in units of scale.  No element is excluded."""
    got, ref64, ref32 = (t.detach().double().cpu().reshape(-1) for t in (got, ref64, ref32))
    assert bool(torch.isfinite(got).all()), name
    s = ref64.abs().max().clamp_min(1e-300).expand_as(ref64) if scale is None else scale.detach().double().cpu().reshape(-1)
    s = s.clamp_min(1e-300)
    err = (got - ref64).abs()
    e_cpu = float(((ref32 - ref64).abs() / s).max())
    e_gpu = float((err / s).max())
    _record(name, {"gpu": e_gpu, "fp32_cpu": e_cpu, "factor": factor})
    print(f"[tol] {name}: gpu {e_gpu:.3e} fp32-cpu {e_cpu:.3e}")
    worst = float((err - (factor * e_cpu * s + 4 * ULP * ref64.abs())).max())
    assert worst <= 0.0, (name, e_gpu, e_cpu, worst)
    return e_gpu, e_cpu


# Measured on MI355X, worst case of each family: GPU error / fp32-CPU error, both in units of the scale the test states (the
# largest |ref| unless a scale is given); every pair is under the 4 e_cpu + 4 ulp bar with the factor 4 nowhere raised.
#   lstm fwd  y 2.4e-7 / 3.8e-7, gates 1.5e-7 / 6.9e-7, c 1.8e-7 / 2.4e-7; at the last of 160 steps (H = 1536, B = 32) y 1.5e-7 /
#             1.3e-7 against 2.2e-7 / 2.1e-7 over all steps: the recurrence forgets, the error does not grow with T
#   lstm bptt 1.6e-7 / 3.6e-7 (step 0 of 160: 8.6e-8 / 8.6e-8); fac_lstm_gate_bwd 1.6e-7 / 1.6e-7; SLSTM(1024) node 7.5e-7 / 6.3e-7
#   snake dx 3.8e-6 / 3.8e-6 (the rounding of alpha x at |alpha x| = 30, common to both); aa_snakebeta dx 1.4e-6 / 2.4e-6
#   mish fwd 2.2e-7 / 2.2e-7, bwd 6.2e-7 / 6.2e-7; gate 2.9e-7 / 2.9e-7; glu 2.8e-7 / 2.8e-7
#   attention P 9.8e-7 / 1.1e-6, o 1.1e-6 / 1.1e-6, dq 9.7e-7 / 9.7e-7, dk 1.3e-6 / 1.4e-6, dv 1.4e-6 / 8.5e-7
#   adamw m 1.4e-7 / 1.4e-7, v 8.3e-8 / 8.3e-8, update: see _check_adamw
# Reductions, worst error / bound: snake dalpha 0.21, dbias 0.08, bias_grad 0.07, weight_norm dg 0.15, dv 0.71, vq_codebook_grad
# 0.12, aa_snakebeta dalpha 0.15, dbeta 0.10, grad_norm 0.07.
def _sum_bound(name, got, ref64, terms_abs_sum, n, c=4.0, ulps=4.0, extra=0.0, abs_extra=None):
    """The `reductions` bound: |got - ref64| <= (c sqrt(n) + extra) 2^-24 sum|terms| + ulps * 2^-24 |ref64| (elementwise over the
    outputs).  `extra` covers the rounding of the terms themselves where they are not plain inputs; it is stated per call.
    abs_extra: a further absolute allowance per output (the conditioning of a sin / cos argument), derived at the call."""
    got, ref64, mag = (torch.as_tensor(t).detach().double().cpu().reshape(-1) for t in (got, ref64, terms_abs_sum))
    assert bool(torch.isfinite(got).all()), name
    bound = (c * math.sqrt(n) + extra) * EPS32 * mag + ulps * EPS32 * ref64.abs()
    if abs_extra is not None:
        bound = bound + torch.as_tensor(abs_extra).detach().double().cpu().reshape(-1)
    err = (got - ref64).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    _record(name, {"gpu_over_bound": ratio, "n": n})
    print(f"[tol] {name}: error / bound {ratio:.3e} (n = {n})")
    assert ratio <= 1.0, (name, ratio)


# ======================================================================================================= A. LSTM
def _lstm_fwd_ref(pre, w_hh, dtype):
    """Single-layer LSTM on the work-buffer layout: pre (4H, T, N) = W_ih x + b, gates i, f, g, o, zero initial state.
    Returns y (H, T, N), the activated gates (4H, T, N) and the cell states (H, T, N)."""
    pre, w = pre.to(dtype), w_hh.to(dtype)
    H = w.shape[1]
    _, T, N = pre.shape
    h = torch.zeros(H, N, dtype=dtype)
    c = torch.zeros(H, N, dtype=dtype)
    ys, gs, cs = [], [], []
    for t in range(T):
        z = pre[:, t] + w @ h
        i, f, o = torch.sigmoid(z[:H]), torch.sigmoid(z[H:2 * H]), torch.sigmoid(z[3 * H:])
        g = torch.tanh(z[2 * H:3 * H])
        c = f * c + i * g
        h = o * torch.tanh(c)
        ys.append(h)
        gs.append(torch.cat([i, f, g, o]))
        cs.append(c)
    return torch.stack(ys, 1), torch.stack(gs, 1), torch.stack(cs, 1)


def _lstm_bptt_ref(dy, w_hh, gates, cs, dtype, forget_uses_c_t=False):
    """dgates (4H, T, N) = gradient w.r.t. the pre-activations, from dy (H, T, N) = gradient w.r.t. h_t and the saved activations.
    forget_uses_c_t is the fault of the self-check (never set by a test)."""
    dy, w, gates, cs = dy.to(dtype), w_hh.to(dtype), gates.to(dtype), cs.to(dtype)
    H, T, N = dy.shape
    out = torch.zeros(4 * H, T, N, dtype=dtype)
    dc_next = torch.zeros(H, N, dtype=dtype)
    for t in range(T - 1, -1, -1):
        dh = dy[:, t] + (w.t() @ out[:, t + 1] if t + 1 < T else 0)
        i, f, g, o = gates[:H, t], gates[H:2 * H, t], gates[2 * H:3 * H, t], gates[3 * H:, t]
        c = cs[:, t]
        c_prev = cs[:, t - 1] if t > 0 else torch.zeros_like(c)
        if forget_uses_c_t:
            c_prev = c
        tc = torch.tanh(c)
        dc = dh * o * (1 - tc * tc) + dc_next
        out[:H, t] = dc * g * i * (1 - i)
        out[H:2 * H, t] = dc * c_prev * f * (1 - f)
        out[2 * H:3 * H, t] = dc * i * (1 - g * g)
        out[3 * H:, t] = dh * tc * o * (1 - o)
        dc_next = dc * f
    return out


def _fwd_branch(H):
    """fac_lstm_layer_fwd_train's dispatch (lstm.hip), restated."""
    kgs = H // 8
    if kgs % 16:
        return "fwd8w"
    return {12: "fwd16x12", 8: "fwd16x8", 4: "fwd16x4", 2: "fwd16x2", 1: "fwd16x1"}.get(kgs // 16, "fwd16xrt")


def _bwd_branch(H):
    """fac_lstm_layer_bwd's dispatch."""
    kgs = H // 8
    if kgs % 16:
        return "bwd8w"
    return {12: "bwd16x12", 8: "bwd16x8"}.get(kgs // 16, "bwd16xrt")


@functools.lru_cache(maxsize=4)
def _lstm_inputs(H, B, T):
    g = _g(1000 * H + 10 * T + B)
    pre = torch.randn(4 * H, T, B, generator=g)
    w_hh = (torch.rand(4 * H, H, generator=g) * 2 - 1) / H ** 0.5
    dy = torch.randn(H, T, B, generator=g)
    ref64 = _lstm_fwd_ref(pre, w_hh, torch.float64)
    ref32 = _lstm_fwd_ref(pre, w_hh, torch.float32)
    return pre, w_hh, dy, ref64, ref32


def _pad_cols(t, BP):
    out = torch.zeros(*t.shape[:-1], BP, dtype=t.dtype)
    out[..., :t.shape[-1]] = t
    return out


def _persist_ok(H, B):
    from facodec_amd import ops
    ops._lstm_arm()
    lib = _lib.load()
    return bool(lib.fac_lstm_persist_ok(H, B)) and bool(lib.fac_lstm_persist_stream_ok(ops._stream()))


# (H, B, T, dy pattern).  Shipped sizes 512 / 1024 / 1536 at T = 1, 2, 160; the other H reach the remaining dispatch branches.
LSTM_CASES = [
    (64, 5, 33, "dense"), (192, 1, 2, "dense"), (128, 17, 33, "dense"), (256, 16, 160, "dense"), (768, 32, 33, "dense"),
    (1280, 1, 2, "dense"),
    (512, 32, 1, "dense"), (512, 17, 2, "dense"), (512, 5, 160, "dense"), (512, 5, 33, "only_t0"),
    (1024, 1, 1, "dense"), (1024, 5, 2, "dense"), (1024, 16, 160, "dense"), (1024, 16, 33, "only_tlast"),
    (1536, 16, 1, "dense"), (1536, 17, 2, "dense"), (1536, 32, 160, "dense"), (1536, 1, 33, "only_t0"), (1536, 5, 33, "only_tlast"),
]
RESIDENT_H = (512, 1024, 1536)


def _lstm_id(case, path):
    H, B, T, pat = case
    return f"{path}_{_fwd_branch(H)}_{_bwd_branch(H)}_H{H}_B{B}_T{T}_{pat}"


LSTM_PARAMS = [(c, p) for c in LSTM_CASES for p in ("per_step", "resident") if p == "per_step" or c[0] in RESIDENT_H]


@gpu
@pytest.mark.parametrize("case,path", LSTM_PARAMS, ids=[_lstm_id(c, p) for c, p in LSTM_PARAMS])
def test_lstm_layer_fwd_train_and_bptt(cuda, case, path):
    """fac_lstm_layer_fwd_train + fac_lstm_layer_bwd (per_step) and fac_lstm_layer_fwd_persist + fac_lstm_layer_bwd_persist
    (resident) of ONE layer: yT, gates_save and c_save against the fp64 recurrence, then dgates against the fp64 BPTT evaluated on
    the GPU forward's own fp32 saves (the same function of the same inputs: the bound absorbs no forward error).  The error at the
    last step of each recurrence is recorded next to the maximum, so growth over T is visible.
    Padded batch columns (pre = 0 there): the recurrence keeps h = c = 0 exactly and gates (0.5, 0.5, 0, 0.5); the per-step
    kernels compute all BP columns, the resident ones only the 16 * ceil(B / 16) they own and leave the rest to the caller."""
    H, B, T, pat = case
    resident = path == "resident"
    if resident and not _persist_ok(H, B):
        pytest.skip("fac_lstm_persist_ok == 0 on this device (the per_step case of the same shape runs)")
    BP = 32 * ((B + 31) // 32)
    nc = 16 * ((B + 15) // 16) if resident else BP
    pre, w_hh, dy, ref64, ref32 = _lstm_inputs(H, B, T)
    if pat == "only_t0":
        dy = dy.clone()
        dy[:, 1:] = 0
    elif pat == "only_tlast":
        dy = dy.clone()
        dy[:, :T - 1] = 0
    pre_d, w_d = _pad_cols(pre, BP).to(cuda), w_hh.to(cuda)
    yT, ybuf, pad = _canary((H, T, BP), cuda)
    gs, gbuf, _ = _canary((4 * H, T, BP), cuda)
    cs, cbuf, _ = _canary((H, T, BP), cuda)
    packed = torch.empty_like(w_d)
    if resident:
        _call("fac_pack_lstm_whh16", _p(w_d), _p(packed), H, 0)
        hfrag = torch.empty(T * H * nc, device=cuda)
        _call("fac_lstm_layer_fwd_persist", _p(pre_d), _p(packed), _p(hfrag), _p(yT), _p(gs), _p(cs), T, H, B, BP)
    else:
        _call("fac_pack_lstm_whh", _p(w_d), _p(packed), H)
        state = torch.empty(3 * H * BP, device=cuda)
        _call("fac_lstm_layer_fwd_train", _p(pre_d), _p(packed), _p(yT), _p(state), _p(gs), _p(cs), T, H, BP, 0)
    torch.cuda.synchronize()
    from facodec_amd import ops
    assert ops.lstm_timeouts() == 0
    fails = []

    def check(fn, *a, **k):
        try:
            fn(*a, **k)
        except AssertionError as e:
            fails.append(str(e)[:400])

    assert _canary_intact(ybuf, pad) and _canary_intact(gbuf, pad) and _canary_intact(cbuf, pad)
    y_c, g_c, c_c = yT.cpu(), gs.cpu(), cs.cpu()
    for t_ in (y_c, g_c, c_c):
        assert bool((t_[..., nc:] == CANARY).all()), "columns the kernel does not own were written"
    if nc > B:                                            # zero pre: h = c = 0 exactly, gates (0.5, 0.5, 0, 0.5) exactly
        assert bool((y_c[..., B:nc] == 0).all()) and bool((c_c[..., B:nc] == 0).all())
        half = torch.cat([g_c[:2 * H, :, B:nc], g_c[3 * H:, :, B:nc]])
        assert bool((half == 0.5).all()) and bool((g_c[2 * H:3 * H, :, B:nc] == 0).all())
    tag = _lstm_id(case, path)
    # measured worst over these cases (gpu / fp32-cpu, units of the largest |ref|): y 2.4e-7 / 3.8e-7, gates 1.5e-7 / 6.9e-7,
    # c 1.8e-7 / 2.4e-7, dgates 1.6e-7 / 3.6e-7
    for nm, got, r64, r32 in (("y", y_c, ref64[0], ref32[0]), ("gates", g_c, ref64[1], ref32[1]), ("c", c_c, ref64[2], ref32[2])):
        check(_bar, f"lstm_fwd_{nm}_{tag}", got[..., :B], r64, r32)
        check(_bar, f"lstm_fwd_{nm}_last_step_{tag}", got[:, T - 1, :B], r64[:, T - 1], r32[:, T - 1],
              scale=r64.abs().max().expand_as(r64[:, T - 1]))
    # ---- BPTT on the GPU's own saves
    gs_in, cs_in = g_c[..., :B].clone(), c_c[..., :B].clone()
    d64 = _lstm_bptt_ref(dy, w_hh, gs_in, cs_in, torch.float64)
    d32 = _lstm_bptt_ref(dy, w_hh, gs_in, cs_in, torch.float32)
    if nc < BP:                                           # the caller zero-fills what the resident kernels leave (header)
        gs[..., nc:] = 0
        cs[..., nc:] = 0
    dy_d = _pad_cols(dy, BP).to(cuda)
    dg, dbuf, _ = _canary((4 * H, T, BP), cuda)
    if resident:
        _call("fac_pack_lstm_whh16", _p(w_d), _p(packed), H, 1)
        scratch = torch.empty((4 + 4 * T) * H * nc, device=cuda)
        _call("fac_lstm_layer_bwd_persist", _p(dy_d), _p(packed), _p(gs), _p(cs), _p(dg), _p(scratch), T, H, B, BP)
    else:
        _call("fac_pack_lstm_whh_t", _p(w_d), _p(packed), H)
        scratch, sbuf, _ = _canary((13 * H * BP,), cuda)
        _call("fac_lstm_layer_bwd", _p(dy_d), _p(packed), _p(gs), _p(cs), _p(dg), _p(scratch), T, H, BP)
    torch.cuda.synchronize()
    assert ops.lstm_timeouts() == 0
    assert _canary_intact(dbuf, pad) and (resident or _canary_intact(sbuf, pad))
    dg_c = dg.cpu()
    assert bool((dg_c[..., nc:] == CANARY).all())
    if nc > B:
        assert bool((dg_c[..., B:nc] == 0).all())        # zero dy columns stay exactly zero
    if pat == "only_t0" and T > 1:
        assert bool((dg_c[:, 1:, :B] == 0).all())        # nothing flows forward in time
    check(_bar, f"lstm_bptt_{tag}", dg_c[..., :B], d64, d32)
    check(_bar, f"lstm_bptt_step0_{tag}", dg_c[:, 0, :B], d64[:, 0], d32[:, 0], scale=d64.abs().max().expand_as(d64[:, 0]))
    assert not fails, fails


@gpu
@pytest.mark.parametrize("H,split", [(256, (4, 5)), (1024, (4, 5)), (192, (3, 6))],
                         ids=["fwd16x2_4+5", "fwd16x8_4+5", "fwd8w_3+6_odd_step0"])
def test_lstm_layer_fwd_from_split_gives_the_bits_of_one_call(cuda, H, split):
    """fac_lstm_layer_fwd_from: T = 9 as two calls on the carried scratch (`step0` = steps already taken selects the h ping / pong
    buffer) must give exactly the single call's h sequence."""
    B, BP, T = 5, 32, 9
    g = _g(H)
    pre = _pad_cols(torch.randn(4 * H, T, B, generator=g), BP)
    w_d = ((torch.rand(4 * H, H, generator=g) * 2 - 1) / H ** 0.5).to(cuda)
    packed = torch.empty_like(w_d)
    _call("fac_pack_lstm_whh", _p(w_d), _p(packed), H)
    pre_d = pre.to(cuda)
    y1 = torch.empty(H, T, BP, device=cuda)
    st1 = torch.empty(3 * H * BP, device=cuda)
    _call("fac_lstm_layer_fwd_from", _p(pre_d), _p(packed), _p(y1), _p(st1), T, H, BP, 0)
    a, b = split
    st2 = torch.full((3 * H * BP,), float("nan"), device=cuda)      # a zero initial state must not be read from the scratch
    pa, pb = pre[:, :a].contiguous().to(cuda), pre[:, a:].contiguous().to(cuda)
    ya, yb = torch.empty(H, a, BP, device=cuda), torch.empty(H, b, BP, device=cuda)
    _call("fac_lstm_layer_fwd_from", _p(pa), _p(packed), _p(ya), _p(st2), a, H, BP, 0)
    _call("fac_lstm_layer_fwd_from", _p(pb), _p(packed), _p(yb), _p(st2), b, H, BP, a)
    torch.cuda.synchronize()
    assert torch.equal(ya.cpu(), y1.cpu()[:, :a]) and torch.equal(yb.cpu(), y1.cpu()[:, a:])
    ref = _lstm_fwd_ref(pre[..., :B], w_d.cpu(), torch.float64)[0]
    assert float((y1.cpu()[..., :B].double() - ref).abs().max()) < 1e-5


def _gate_bwd_ref(dy_t, rec, gates_t, c_t, c_prev, dc_in, first, dtype):
    dy_t, gates_t, c_t = dy_t.to(dtype), gates_t.to(dtype), c_t.to(dtype)
    H = dy_t.shape[0]
    dh = dy_t + (rec.to(dtype) if rec is not None else 0)
    i, f, g, o = gates_t[:H], gates_t[H:2 * H], gates_t[2 * H:3 * H], gates_t[3 * H:]
    cp = c_prev.to(dtype) if c_prev is not None else torch.zeros_like(c_t)
    tc = torch.tanh(c_t)
    dc = dh * o * (1 - tc * tc) + (0 if first else dc_in.to(dtype))
    dg = torch.cat([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)])
    return dg, dc * f


@gpu
@pytest.mark.parametrize("first,has_prev", [(1, True), (0, True), (0, False), (1, False)],
                         ids=["first_rec_null", "middle", "t0_c_prev_null", "T1_first_and_c_prev_null"])
def test_lstm_gate_bwd_alone(cuda, first, has_prev):
    """fac_lstm_gate_bwd: one BPTT step's elementwise part on views of (rows, T, BP) buffers whose row stride rs = T * BP is larger
    than BP; `first` = last time step (rec NULL, the carried dc is not read: it holds NaN here), c_prev NULL = step t = 0."""
    H, BP, T, t = 96, 32, 3, 1
    rs = T * BP
    g = _g(10 * first + has_prev)
    gates = torch.cat([torch.rand(2 * H, T, BP, generator=g), torch.rand(H, T, BP, generator=g) * 2 - 1,
                       torch.rand(H, T, BP, generator=g)])
    cs = torch.randn(H, T, BP, generator=g) * 2
    dy = torch.randn(H, T, BP, generator=g)
    rec = None if first else torch.randn(H, BP, generator=g)
    dc0 = torch.full((H, BP), float("nan")) if first else torch.randn(H, BP, generator=g)
    c_prev = cs[:, t - 1] if has_prev else None
    r64 = _gate_bwd_ref(dy[:, t], rec, gates[:, t], cs[:, t], c_prev, dc0, first, torch.float64)
    r32 = _gate_bwd_ref(dy[:, t], rec, gates[:, t], cs[:, t], c_prev, dc0, first, torch.float32)
    gates_d, cs_d, dy_d = gates.to(cuda), cs.to(cuda), dy.to(cuda)
    rec_d = rec.to(cuda) if rec is not None else None
    dc_d, dcbuf, pad = _canary((H, BP), cuda)
    dc_d.copy_(dc0)
    dg, dgbuf, _ = _canary((4 * H, T, BP), cuda)
    off = t * BP
    _call("fac_lstm_gate_bwd", _p(dy_d.view(-1)[off:]), _p(rec_d), _p(gates_d.view(-1)[off:]), _p(cs_d.view(-1)[off:]),
          _p(cs_d.view(-1)[off - BP:]) if has_prev else _p(None), _p(dc_d), _p(dg.view(-1)[off:]), H, BP, rs, first)
    torch.cuda.synchronize()
    assert _canary_intact(dcbuf, pad) and _canary_intact(dgbuf, pad)
    dg_c = dg.cpu()
    assert bool((dg_c[:, [0, 2]] == CANARY).all())        # the other time steps of the strided buffer
    nm = f"lstm_gate_bwd_first{first}_prev{int(has_prev)}"
    _bar(nm + "_dgates", dg_c[:, t], r64[0], r32[0])
    _bar(nm + "_dc", dc_d.cpu(), r64[1], r32[1])


@gpu
def test_slstm_node_fp64_autograd_H1024(cuda):
    """The whole SLSTM autograd node (autograd.slstm: two layers, fac_lstm_layer_fwd_train / _bwd or their resident forms, the input
    GEMMs, the skip) at a shipped size -- SLSTM(1024, 2), B = 4, T = 40 -- against float64 autograd through torch.nn.LSTM carrying
    the same weights: output, input gradient and weight_ih / weight_hh / bias_ih / bias_hh gradients of both layers.  The fp32-CPU
    error is torch.nn.LSTM in fp32 on the CPU."""
    from facodec_amd import autograd as A
    from facodec_amd import synth
    from facodec_amd.layers import SLSTM
    H, B, T = 1024, 4, 40
    m = SLSTM(H, 2)
    synth.load_synthetic(m, seed=9)
    sd = {k: v.detach().clone() for k, v in m.lstm.named_parameters()}
    x = torch.randn(B, H, T, generator=_g(1))
    r = torch.randn(B, H, T, generator=_g(2))

    def torch_ref(dtype):
        lstm = torch.nn.LSTM(H, H, 2).to(dtype)
        with torch.no_grad():
            for k, v in sd.items():
                getattr(lstm, k).copy_(v.to(dtype))
        xx = x.to(dtype).clone().requires_grad_()
        seq = xx.permute(2, 0, 1)
        y = (lstm(seq)[0] + seq).permute(1, 2, 0)
        (y * r.to(dtype)).sum().backward()
        return y.detach(), xx.grad, {k: getattr(lstm, k).grad for k in sd}

    y64, dx64, g64 = torch_ref(torch.float64)
    y32, dx32, g32 = torch_ref(torch.float32)
    m = m.to(cuda)
    xc = x.to(cuda).requires_grad_()
    y = A.slstm(m, xc)
    (y * r.to(cuda)).sum().backward()
    torch.cuda.synchronize()
    got = {k: v.grad for k, v in m.lstm.named_parameters()}
    assert set(got) == set(sd) and len(sd) == 8
    fails = []
    for nm, a, b64, b32 in [("y", y, y64, y32), ("dx", xc.grad, dx64, dx32)] + [(k, got[k], g64[k], g32[k]) for k in sorted(sd)]:
        try:
            _bar(f"slstm_node_H1024_{nm}", a, b64, b32)
        except AssertionError as e:
            fails.append(str(e)[:300])
    assert not fails, fails


# ======================================================================================================= B. optimiser
B1, B2, ADAM_EPS, WD, LR = 0.9, 0.98, 1e-9, 0.1, 1e-3      # optim.hip's header comment (optimizers.py:72-108)


def _f32(v):
    """The value a C float argument carries."""
    return float(torch.tensor(v, dtype=torch.float32))


def _adamw_ref(p, g, m, v, step, clip, dtype, bias_step_shift=0):
    """torch.optim.AdamW written out: decoupled decay, bias correction, eps added outside the square root of the corrected v.
    Hyper-parameters enter as the fp32 values the kernel receives.  Returns (update = p_new - p as the formula gives it, before
    it is rounded into p, m_new, v_new).  bias_step_shift is the fault of the self-check."""
    t = lambda a: torch.as_tensor(a, dtype=dtype)
    lr, b1, b2, eps, wd = (t(_f32(a)) for a in (LR, B1, B2, ADAM_EPS, WD))
    p, g, m, v = (a.to(dtype) for a in (p, g, m, v))
    step = torch.as_tensor(step).to(dtype) + bias_step_shift
    if clip is not None:
        g = g * t(_f32(clip))
    m_new = b1 * m + (1 - b1) * g
    v_new = b2 * v + (1 - b2) * g * g
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    den = v_new.sqrt() / bc2.sqrt() + eps
    upd = -lr * wd * p - (lr / bc1) * m_new / den
    # magnitude of the update's terms before any of them cancel (b1 m against (1 - b1) g, decay against the Adam term)
    mag = lr * wd * p.abs() + (lr / bc1) * (b1 * m.abs() + (1 - b1) * g.abs()) / den
    return upd, m_new, v_new, mag


def _adamw_state(n, seed):
    g_ = _g(seed)
    p = torch.randn(n, generator=g_) * torch.logspace(-3, 0, n)[torch.randperm(n, generator=g_)]
    g = torch.randn(n, generator=g_)
    m = torch.randn(n, generator=g_) * 0.1
    v = torch.rand(n, generator=g_) * 0.5
    k = max(1, n // 16)
    g[:k] = 0                      # g = 0 and v = 0: the denominator is eps alone (m = 0: a pure decay step; m != 0: m / eps)
    v[:k] = 0
    m[:k:2] = 0
    return p, g, m, v


def _check_adamw(tag, p0, got_p, got_m, got_v, g, m, v, step, clip):
    """update, m, v against fp64.  The update bound is 4 e_cpu mag + 4 ulp |p|: e_cpu is the error of the fp32-CPU update formula
    in units of mag, the size of its terms before they cancel (measured 3.2e-7 on MI355X against e_cpu 4.0e-7 at worst), and the second term is the rounding of p itself when the update is added (p is about 1e3 updates large)."""
    u64, m64, v64, umag = _adamw_ref(p0, g, m, v, step, clip, torch.float64)
    u32, m32, v32, _ = _adamw_ref(p0, g, m, v, step, clip, torch.float32)
    assert bool(torch.isfinite(got_p).all()) and bool(torch.isfinite(u64).all())
    upd = got_p.double() - p0.double()
    s = umag.clamp_min(1e-300)
    e_cpu = float(((u32.double() - u64).abs() / s).max())
    err = (upd - u64).abs()
    e_gpu = float(((err - 4 * ULP * (p0.double() + u64).abs()).clamp_min(0) / s).max())
    _record(f"adamw_update_{tag}", {"gpu": e_gpu, "fp32_cpu": e_cpu, "factor": 4})
    print(f"[tol] adamw_update_{tag}: gpu (beyond the rounding of p) {e_gpu:.3e} fp32-cpu {e_cpu:.3e}")
    assert e_gpu <= 4 * e_cpu, (tag, e_gpu, e_cpu)
    gs = g * (_f32(clip) if clip is not None else 1.0)
    _bar(f"adamw_m_{tag}", got_m, m64, m32, scale=_f32(B1) * m.double().abs() + (1 - _f32(B1)) * gs.double().abs())
    _bar(f"adamw_v_{tag}", got_v, v64, v32)


@gpu
@pytest.mark.parametrize("clip", [None, 0.37], ids=["noclip", "clip"])
@pytest.mark.parametrize("step", [1, 2, 1000, 200000])
def test_adamw_step_update_fp64(cuda, step, clip):
    """fac_adamw_step: the UPDATE p_after - p_before, m and v against the fp64 AdamW at step counts where 1 - beta^s is small
    (1, 2) and where it is 1 to fp32 (1000, 200 000; the entry computes its corrections with powf)."""
    n = 65535 * 256 // 64 + 77 if step == 2 else 5000
    p, g, m, v = _adamw_state(n, step)
    bufs = [_canary((n,), cuda) for _ in range(4)]
    for (view, _, _), src in zip(bufs, (p, g, m, v)):
        view.copy_(src)
    clip_d = torch.tensor([123.0, clip], device=cuda) if clip is not None else None
    _call("fac_adamw_step", *[_p(b[0]) for b in bufs], n, LR, B1, B2, ADAM_EPS, WD, step, _p(clip_d))
    torch.cuda.synchronize()
    assert all(_canary_intact(b[1], b[2]) for b in bufs)
    assert torch.equal(bufs[1][0].cpu(), g)
    _check_adamw(f"step{step}_{'clip' if clip else 'noclip'}", p, bufs[0][0].cpu(), bufs[2][0].cpu(), bufs[3][0].cpu(), g, m, v,
                 step, clip)


# about 40 parameters; sizes chosen so that chunks of 2048 fall inside one parameter (whole-chunk, 16-byte path), straddle several
# parameters, and the arena's tail chunk is short.  FlatAdamW builds its offsets from p.numel() of torch Parameters, which may be
# empty, so a zero-length parameter (offsets[j] == offsets[j + 1]) can occur; one sits in the middle.
MASKED_SIZES = [1, 3, 2047, 2048, 2049, 3 * 2048 + 5, 70001, 5, 7, 0, 11, 2048, 2048, 13, 4096, 1, 1, 1, 6000, 17, 300, 1024, 1024,
                19, 8192, 2, 3, 4, 5, 6, 7, 8, 9, 10, 4099, 23, 29, 31, 2048 * 2 + 1, 37]
STRADDLE_OWNER = 4          # the parameter of 2049 elements: its last element opens a chunk that later parameters share


def _masked_run(cuda, flags, steps0, clip, shift, seed=5):
    """One fac_adamw_step_masked launch on the MASKED_SIZES arena; shift = 1 places all four arenas one float off 16-byte
    alignment.  Returns CPU copies (p, m, v, steps) and the inputs."""
    n = sum(MASKED_SIZES)
    P = len(MASKED_SIZES)
    p, g, m, v = _adamw_state(n, seed)
    off = torch.tensor([0] + list(torch.tensor(MASKED_SIZES).cumsum(0)), dtype=torch.int64)
    bufs = [_canary((n + 4,), cuda) for _ in range(4)]
    views = []
    for (view, _, _), src in zip(bufs, (p, g, m, v)):
        view[shift:shift + n].copy_(src)
        views.append(view[shift:shift + n])
    assert all((t.data_ptr() % 16 == 0) == (shift == 0) for t in views)
    off_d, flags_d = off.to(cuda), torch.tensor(flags, dtype=torch.float32, device=cuda)
    steps_d, sbuf, spad = _canary((P,), cuda, dtype=torch.int32)
    steps_d.copy_(torch.tensor(steps0, dtype=torch.int32))
    bc, bcbuf, bpad = _canary((2 * P,), cuda)
    clip_d = torch.tensor([123.0, clip], device=cuda) if clip is not None else None
    _call("fac_adamw_step_masked", *[_p(t) for t in views], n, _p(off_d), P, _p(flags_d), _p(steps_d), _p(bc), LR, B1, B2, ADAM_EPS,
          WD, _p(clip_d))
    torch.cuda.synchronize()
    assert all(_canary_intact(b[1], b[2]) for b in bufs) and _canary_intact(sbuf, spad) and _canary_intact(bcbuf, bpad)
    for (view, _, _) in bufs:                                   # the floats of the buffer outside the shifted arena
        rest = torch.cat([view.cpu()[:shift], view.cpu()[shift + n:]])
        assert bool((rest == CANARY).all())
    assert torch.equal(views[1].cpu(), g)
    return (views[0].cpu(), views[2].cpu(), views[3].cpu(), steps_d.cpu()), (p, g, m, v, off)


def _flag_sets():
    P = len(MASKED_SIZES)
    return {"all_on": [1.0] * P, "all_off": [0.0] * P, "alternating": [float(j % 2) for j in range(P)],
            "only_straddle_owner": [float(j == STRADDLE_OWNER) for j in range(P)]}


@gpu
@pytest.mark.parametrize("clip", [None, 0.37], ids=["noclip", "clip"])
@pytest.mark.parametrize("flagset", ["all_on", "all_off", "alternating", "only_straddle_owner"])
def test_adamw_step_masked_whole_chunk_straddle_tail_skip(cuda, flagset, clip):
    """fac_adamw_step_masked on an arena whose chunks of 2048 reach all three paths of adamw_masked_kernel (whole chunk inside one
    parameter; a chunk that straddles parameter boundaries or is the short tail; skip), with a zero-length parameter in the
    middle and per-parameter step counts 1, 2, 1000, 200 000, ...: flagged parameters advance steps[j] by exactly 1 and take the
    update of THEIR count (update, m, v against fp64); unflagged ones keep p, m, v and steps[j] bit for bit.  The same arena one
    float off 16-byte alignment (aligned16 false: every chunk on the 4-byte path) must give the bits of the aligned run."""
    P = len(MASKED_SIZES)
    n = sum(MASKED_SIZES)
    assert n % 2048 != 0 and MASKED_SIZES[9] == 0
    flags = _flag_sets()[flagset]
    steps0 = [(0, 1, 999, 199999, 7)[j % 5] for j in range(P)]
    (p1, m1, v1, s1), (p, g, m, v, off) = _masked_run(cuda, flags, steps0, clip, 0)
    # chunk census: the cases this arena is built for
    starts = torch.arange(0, n, 2048)
    owner = torch.searchsorted(off[1:], starts, right=True)
    whole = (off[owner + 1] >= starts + 2048) & (starts + 2048 <= n)
    assert int(whole.sum()) >= 30 and int((~whole).sum()) >= 8 and not bool(whole[-1])
    ci = int(off[STRADDLE_OWNER + 1] - 1) // 2048              # the chunk that STRADDLE_OWNER opens and later parameters share
    assert int(owner[ci]) == STRADDLE_OWNER and not bool(whole[ci]) and int(off[STRADDLE_OWNER + 1]) < (ci + 1) * 2048
    fl = torch.tensor(flags)
    assert torch.equal(s1, torch.tensor(steps0, dtype=torch.int32) + (fl > 0).int())
    el_flag = torch.repeat_interleave(fl, torch.tensor(MASKED_SIZES)) > 0
    el_step = torch.repeat_interleave(torch.tensor(steps0) + 1, torch.tensor(MASKED_SIZES))
    off_ = ~el_flag
    assert torch.equal(p1[off_], p[off_]) and torch.equal(m1[off_], m[off_]) and torch.equal(v1[off_], v[off_])
    if bool(el_flag.any()):
        on = el_flag
        _check_adamw(f"masked_{flagset}_{'clip' if clip else 'noclip'}", p[on], p1[on], m1[on], v1[on], g[on], m[on], v[on],
                     el_step[on], clip)
    (p2, m2, v2, s2), _ = _masked_run(cuda, flags, steps0, clip, 1)
    assert torch.equal(s2, s1)
    assert torch.equal(p2, p1) and torch.equal(m2, m1) and torch.equal(v2, v1), "misaligned arena: not the bits of the aligned run"


@gpu
@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned_scalar_path"])
@pytest.mark.parametrize("n", [1, 3, 4, 1023, 4 * 256 * 1024 + 7, 30000001])
def test_grad_norm_clip_fp64(cuda, n, misaligned):
    """fac_grad_norm_clip: the norm against a float64 sum of squares (16-byte path with its n % 4 tail, the scalar path of a
    misaligned g, n below and far above the fixed 1024-block grid), the coefficient EXACTLY min(1, max_norm / (norm + 1e-6)) in
    fp32 from the kernel's own norm, for max_norm above and below the norm, and two calls bit-identical (fixed order)."""
    g = torch.randn(n, generator=_g(n))
    buf = torch.zeros(n + 8, device=cuda)
    off = 1 if misaligned else 0
    buf[off:off + n].copy_(g)
    g_d = buf[off:off + n]
    assert (g_d.data_ptr() % 16 != 0) == misaligned
    ref = float(g.double().pow(2).sum().sqrt())
    outs = []
    for max_norm in (ref * 0.25, ref * 4.0, ref * 0.25):
        scratch, sbuf, pad = _canary((1024,), cuda)
        out, obuf, _ = _canary((2,), cuda)
        _call("fac_grad_norm_clip", _p(g_d), n, max_norm, _p(scratch), _p(out))
        torch.cuda.synchronize()
        assert _canary_intact(sbuf, pad) and _canary_intact(obuf, pad)
        o = out.cpu()
        outs.append(o)
        nrm = o[0]
        coef = torch.tensor(max_norm, dtype=torch.float32) / (nrm + torch.tensor(1e-6, dtype=torch.float32))
        assert torch.equal(o[1], torch.minimum(coef, torch.ones(())))
        assert (float(o[1]) < 1.0) == (max_norm < ref)
    assert torch.equal(outs[0], outs[2])
    # sum of n squares (terms g^2, all positive): 4 sqrt(n) 2^-24 sum|terms| on the sum; the square root halves the relative error
    s = float(outs[0][0]) ** 2
    s_ref = ref * ref
    ratio = abs(s - s_ref) / ((4 * math.sqrt(n) + 4) * EPS32 * s_ref)
    _record(f"grad_norm_clip_n{n}_{'mis' if misaligned else ''}aligned", {"gpu_over_bound": ratio, "n": n})
    assert ratio <= 1.0, (float(outs[0][0]), ref, ratio)


# ======================================================================================================= C. VQ, Snake, weight norm, bias
VQ_CD = 8


def _vq_case(B, T, Kc, seed, n_q=3, row=1):
    g = _g(seed)
    z_e = torch.randn(B, VQ_CD, T, generator=g)
    cb = torch.randn(Kc, VQ_CD, generator=g)
    all_codes = torch.randint(0, Kc, (B, n_q, T), generator=g)           # the kernel sees ONE row of it: codes_bs = n_q * T
    return z_e, cb, all_codes, row


@gpu
@pytest.mark.parametrize("T", [1, 7, 160, 1001])
@pytest.mark.parametrize("outs", ["d_ze", "z_st", "both"])
@pytest.mark.parametrize("with_dzst", [True, False], ids=["dzst", "dzst_null"])
def test_vq_latent_bwd(cuda, T, outs, with_dzst):
    """fac_vq_latent_bwd: d_ze = d_zst (or 0 when NULL) + wc[b] * 2 / (8 T) * (z_e - cb[idx]) against fp64 and z_st bit for bit the
    fp32 expression z_e + (cb[idx] - z_e); codes are one row of a (B, n_q, T) tensor (codes_bs = n_q * T), wc includes 0 and is NULL
    when only z_st is asked for."""
    B, Kc = 3, 64
    z_e, cb, all_codes, row = _vq_case(B, T, Kc, T)
    codes = all_codes[:, row]
    g = _g(T + 1)
    d_zst = torch.randn(B, VQ_CD, T, generator=g) if with_dzst else None
    wc = torch.tensor([0.7, 0.0, 1.3])
    want_d, want_s = outs in ("d_ze", "both"), outs in ("z_st", "both")
    z_d, cb_d, codes_d = z_e.to(cuda), cb.to(cuda), all_codes.to(cuda)
    dz_d = d_zst.to(cuda) if with_dzst else None
    wc_d = wc.to(cuda) if want_d else None
    d_ze, dbuf, pad = _canary((B, VQ_CD, T), cuda)
    z_st, sbuf, _ = _canary((B, VQ_CD, T), cuda)
    n_q = all_codes.shape[1]
    _call("fac_vq_latent_bwd", _p(z_d), _p(cb_d), _p(codes_d[:, row]), n_q * T, _p(dz_d), _p(wc_d), _p(d_ze if want_d else None),
          _p(z_st if want_s else None), B, T)
    torch.cuda.synchronize()
    assert _canary_intact(dbuf, pad) and _canary_intact(sbuf, pad)
    zq = cb[codes].permute(0, 2, 1)                                     # (B, 8, T)
    if want_s:
        assert torch.equal(z_st.cpu(), z_e + (zq - z_e))
    else:
        assert bool((z_st.cpu() == CANARY).all())
    if want_d:
        commit = wc.double().view(B, 1, 1) * 2.0 / (VQ_CD * T) * (z_e.double() - zq.double())
        ref = commit + (d_zst.double() if with_dzst else 0)
        # five rounded fp32 operations per element (2 / (8 T), wc * inv, z_e - cb, the product, the add), no reduction
        mag = (d_zst.double().abs() if with_dzst else 0) + \
            wc.double().view(B, 1, 1) * 2.0 / (VQ_CD * T) * (z_e.double().abs() + zq.double().abs())
        assert bool(((d_ze.cpu().double() - ref).abs() <= 6 * EPS32 * mag).all())
        assert bool((d_ze.cpu()[1] == (d_zst[1] if with_dzst else torch.zeros(VQ_CD, T))).all())       # wc = 0: straight-through only
    else:
        assert bool((d_ze.cpu() == CANARY).all())


@gpu
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("Kc,mode", [(2, "random"), (1024, "random"), (1024, "one_code_everywhere"), (2, "one_code_everywhere")])
def test_vq_codebook_grad(cuda, Kc, mode, accumulate):
    """fac_vq_codebook_grad against a float64 index_add_: dcb[k] (+)= sum over positions that chose k of wb[b] * 2 / (8 T) *
    (cb[k] - z_e); a code chosen by every position, codes never chosen (row exactly 0, or untouched when accumulating), wb with a
    zero, non-dense codes, and two runs bit-identical."""
    B, T = 4, 333
    z_e, cb, all_codes, row = _vq_case(B, T, Kc, Kc + accumulate)
    if mode == "one_code_everywhere":
        all_codes[:, row] = Kc - 1
    codes = all_codes[:, row]
    wb = torch.tensor([0.25, 0.0, 1.0, 0.5])
    dcb0 = torch.randn(Kc, VQ_CD, generator=_g(3))
    z_d, cb_d, codes_d, wb_d = z_e.to(cuda), cb.to(cuda), all_codes.to(cuda), wb.to(cuda)
    n_q = all_codes.shape[1]
    res = []
    for _ in range(2):
        dcb, buf, pad = _canary((Kc, VQ_CD), cuda)
        dcb.copy_(dcb0)
        _call("fac_vq_codebook_grad", _p(z_d), _p(cb_d), _p(codes_d[:, row]), n_q * T, _p(wb_d), _p(dcb), B, T, Kc, accumulate)
        torch.cuda.synchronize()
        assert _canary_intact(buf, pad)
        res.append(dcb.cpu())
    assert torch.equal(res[0], res[1])
    w = (wb.double() * 2.0 / (VQ_CD * T)).view(B, 1, 1)
    zq = cb[codes].permute(0, 2, 1).double()
    terms = (w * (zq - z_e.double())).permute(0, 2, 1).reshape(B * T, VQ_CD)
    tmag = (w * (zq.abs() + z_e.double().abs())).permute(0, 2, 1).reshape(B * T, VQ_CD)
    idx = codes.reshape(-1)
    ref = torch.zeros(Kc, VQ_CD, dtype=torch.float64).index_add_(0, idx, terms)
    mag = torch.zeros(Kc, VQ_CD, dtype=torch.float64).index_add_(0, idx, tmag)
    count = torch.bincount(idx, minlength=Kc)
    if accumulate:
        ref = ref + dcb0.double()
        mag = mag + dcb0.double().abs()
    unused = count == 0
    assert bool(unused.any()) or Kc == 2
    assert torch.equal(res[0][unused], dcb0[unused] if accumulate else torch.zeros(int(unused.sum()), VQ_CD))
    # n = positions that chose the code; every term is three rounded fp32 operations on inputs (extra = 4)
    _sum_bound(f"vq_codebook_grad_K{Kc}_{mode}_acc{accumulate}", res[0], ref, mag, int(count.max()), extra=4.0)


def _snake_ref(x, alpha, dy, add, dtype, drop_sin2_term=False):
    """y = x + sin^2(alpha x) / (alpha + 1e-9): dx = add + dy (1 + alpha sin(2 alpha x) / (alpha + eps)), the per-element terms of
    dalpha = dy (x sin(2 alpha x) / (alpha + eps) - sin^2(alpha x) / (alpha + eps)^2), and |terms| without the cancellation."""
    x, dy = x.to(dtype), dy.to(dtype)
    a = alpha.to(dtype).view(1, -1, 1)
    ae = a + torch.as_tensor(1e-9, dtype=dtype)
    s2 = torch.sin(2 * a * x)
    sn2 = torch.sin(a * x) ** 2
    dx = dy * (1 + a * s2 / ae)
    if add is not None:
        dx = dx + add.to(dtype)
    second = 0 if drop_sin2_term else sn2 / (ae * ae)
    terms = dy * (x * s2 / ae - second)
    tmag = dy.abs() * ((x * s2).abs() / ae + sn2 / (ae * ae))
    # the argument theta = alpha x is itself a rounded fp32 product: d theta = 2^-24 |theta| moves the term by |d term / d theta|
    argmag = dy.abs() * (a * x).abs() * (2 * x.abs() * torch.cos(2 * a * x).abs() / ae + s2.abs() / (ae * ae))
    return dx, terms, tmag, argmag


# (B, C, T, add, dbias, extra row stride of dy, entry point)
SNAKE_CASES = [
    ("plain_1x1x1", 1, 1, 1, False, False, 0, "fac_snake_bwd"),
    ("plain_3x48x701", 3, 48, 701, False, False, 0, "fac_snake_bwd"),
    ("plain_2x1536x7", 2, 1536, 7, False, False, 0, "fac_snake_bwd"),
    ("fused_1x1x1_add_dbias", 1, 1, 1, True, True, 0, "fac_snake_bwd_fused"),
    ("fused_v4_2x64x1000_add_dbias", 2, 64, 1000, True, True, 0, "fac_snake_bwd_fused"),
    ("fused_v4_2x64x1000_no_add_no_dbias", 2, 64, 1000, False, False, 0, "fac_snake_bwd_fused"),
    ("fused_scalar_3x48x701_add", 3, 48, 701, True, False, 0, "fac_snake_bwd_fused"),
    ("fused_scalar_3x48x701_dbias", 3, 48, 701, False, True, 0, "fac_snake_bwd_fused"),
    ("fused_scalar_3x48x701_no_add_no_dbias", 3, 48, 701, False, False, 0, "fac_snake_bwd_fused"),
    ("fused_2x1536x7_add_dbias", 2, 1536, 7, True, True, 0, "fac_snake_bwd_fused"),
    ("fused_v4_16x1x38400_add_dbias", 16, 1, 38400, True, True, 0, "fac_snake_bwd_fused"),
    ("fused_v4_16x48x38400_dbias", 16, 48, 38400, False, True, 0, "fac_snake_bwd_fused"),
    ("rs_v4_2x64x1000_stride1006_add_dbias", 2, 64, 1000, True, True, 6, "fac_snake_bwd_fused_rs"),
    ("rs_scalar_odd_stride_2x64x1000_dbias", 2, 64, 1000, False, True, 7, "fac_snake_bwd_fused_rs"),
    ("rs_scalar_3x48x701_stride713_add", 3, 48, 701, True, False, 12, "fac_snake_bwd_fused_rs"),
    ("rs_1x1x1_stride3", 1, 1, 1, False, True, 2, "fac_snake_bwd_fused_rs"),
]


@gpu
@pytest.mark.parametrize("case", SNAKE_CASES, ids=[c[0] for c in SNAKE_CASES])
def test_snake_bwd_family(cuda, case):
    """fac_snake_bwd, fac_snake_bwd_fused, fac_snake_bwd_fused_rs: dx elementwise (maps bound), dalpha and dbias as reductions over
    B x T, alpha in [0.05, 5].  With a row stride the columns between the rows of dy hold canaries: a read past the window would
    change the result by 1e4.  fac_snake_bwd_fused without add / dbias must give the bits of fac_snake_bwd: dx always, dalpha on
    the scalar path (the 16-byte path sums dalpha in another order)."""
    name, B, Cc, T, has_add, has_db, extra, entry = case
    g = _g(len(name) + B * T)
    x = torch.randn(B, Cc, T, generator=g) * 2
    alpha = torch.exp(torch.rand(Cc, generator=g) * math.log(100.0)) * 0.05
    alpha[0], alpha[-1] = (0.05, 5.0) if Cc > 1 else (5.0, 5.0)
    dy = torch.randn(B, Cc, T, generator=g)
    add = torch.randn(B, Cc, T, generator=g) if has_add else None
    rs = T + extra
    dy_d = dy.to(cuda)
    if extra:
        dy_d = torch.full((B, Cc, rs), CANARY, device=cuda)
        dy_d[..., :T] = dy.to(cuda)
    x_d, a_d = x.to(cuda), alpha.to(cuda)
    add_d = add.to(cuda) if has_add else None
    dx, xbuf, pad = _canary((B, Cc, T), cuda)
    da, abuf, _ = _canary((Cc,), cuda)
    db, bbuf, _ = _canary((Cc,), cuda)
    scratch, sbuf, _ = _canary((64 * Cc,), cuda)
    if entry == "fac_snake_bwd":
        _call(entry, _p(x_d), _p(a_d), _p(dy_d), _p(dx), _p(da), _p(scratch), B, Cc, T)
    elif entry == "fac_snake_bwd_fused":
        _call(entry, _p(x_d), _p(a_d), _p(dy_d), _p(add_d), _p(dx), _p(da), _p(db if has_db else None), _p(scratch), B, Cc, T)
    else:
        _call(entry, _p(x_d), _p(a_d), _p(dy_d), rs, _p(add_d), _p(dx), _p(da), _p(db if has_db else None), _p(scratch), B, Cc, T)
    torch.cuda.synchronize()
    assert all(_canary_intact(b, pad) for b in (xbuf, abuf, bbuf, sbuf))
    if not has_db:
        assert bool((db.cpu() == CANARY).all())
    if entry == "fac_snake_bwd":
        assert bool((scratch.cpu()[32 * Cc:] == CANARY).all())        # documented scratch: 32 * C floats
    dx64, t64, tmag, argmag = _snake_ref(x, alpha, dy, add, torch.float64)
    dx32 = _snake_ref(x, alpha, dy, add, torch.float32)[0]
    # scale: |add| + |dy| (1 + |sin 2 alpha x|), the terms before the cancellation 1 + sin(..) -> 0
    scale = dy.double().abs() * (1 + torch.sin(2 * alpha.double().view(1, -1, 1) * x.double()).abs()) + \
        (add.double().abs() if has_add else 0)
    _bar(f"snake_bwd_dx_{name}", dx.cpu(), dx64, dx32, scale=scale)
    n = B * T
    # every dalpha term: sin, cos (<= 2 ulp each), about eight rounded operations -> extra = 16 half-ulps of |terms|; and the
    # rounding of the argument alpha x (|alpha x| reaches 30 here), which sin 2 theta and sin^2 theta amplify by |theta|: 2 half-ulps
    # of theta (the product, and alpha + 1e-9 against alpha), each worth |d term / d theta|
    _sum_bound(f"snake_bwd_dalpha_{name}", da.cpu(), t64.sum((0, 2)), tmag.sum((0, 2)), n, extra=16.0,
               abs_extra=2 * EPS32 * argmag.sum((0, 2)))
    if has_db:
        # dbias sums the kernel's own fp32 dx; its terms carry dx's error (extra: the maps bound of dx, in half-ulps of the scale)
        _sum_bound(f"snake_bwd_dbias_{name}", db.cpu(), dx64.sum((0, 2)), scale.sum((0, 2)), n, extra=16.0)
    if entry == "fac_snake_bwd_fused" and not has_add and not has_db:
        dx2 = torch.empty(B, Cc, T, device=cuda)
        da2 = torch.empty(Cc, device=cuda)
        sc2 = torch.empty(32 * Cc, device=cuda)
        _call("fac_snake_bwd", _p(x_d), _p(a_d), _p(dy_d), _p(dx2), _p(da2), _p(sc2), B, Cc, T)
        torch.cuda.synchronize()
        assert torch.equal(dx2.cpu(), dx.cpu())
        # dalpha: the scalar fused kernel walks the positions in fac_snake_bwd's order (same bits); the 16-byte kernel (T % 4 == 0)
        # gives every lane four neighbouring positions, another summation order, so it answers to the reduction bound above only
        assert torch.equal(da2.cpu(), da.cpu()) or T % 4 == 0


@gpu
@pytest.mark.parametrize("B,Cc,T", [(1, 1, 1), (1, 3, 7), (7, 5, 1024), (7, 2, 1536), (2050, 1, 1), (3, 2050, 5), (16, 3, 38400)])
def test_bias_grad_fp64(cuda, B, Cc, T):
    """fac_bias_grad: db[c] = sum over (b, t) of dy against a float64 sum; row lengths B * T = 1, 7, 1024 x 7, 1536 x 7 (the longest
    row in the model) and beyond, 1 and 2050 channels."""
    dy = torch.randn(B, Cc, T, generator=_g(B + Cc + T))
    dy_d = dy.to(cuda)
    db, buf, pad = _canary((Cc,), cuda)
    scratch, sbuf, _ = _canary((32 * Cc,), cuda)
    _call("fac_bias_grad", _p(dy_d), _p(db), _p(scratch), B, Cc, T)
    torch.cuda.synchronize()
    assert _canary_intact(buf, pad) and _canary_intact(sbuf, pad)
    _sum_bound(f"bias_grad_{B}x{Cc}x{T}", db.cpu(), dy.double().sum((0, 2)), dy.double().abs().sum((0, 2)), B * T)


@gpu
@pytest.mark.parametrize("g_is_norm", [False, True], ids=["g_free", "g_eq_norm"])
@pytest.mark.parametrize("n_rows,row_len", [(1, 1), (1, 7), (2050, 7), (1, 1024 * 7), (3, 1536 * 7), (2050, 1)])
def test_weight_norm_bwd_fp64(cuda, n_rows, row_len, g_is_norm):
    """fac_weight_norm_bwd: w = g v / ||v|| per row; dg = <dw, v> / ||v||, dv = g / ||v|| (dw - v <dw, v> / ||v||^2) against fp64,
    the identity <dv, v> = 0 (dv is tangent to the sphere once dg is folded out), and the g = ||v|| case of a fresh weight_norm."""
    g_ = _g(n_rows * 31 + row_len)
    v = torch.randn(n_rows, row_len, generator=g_)
    dw = torch.randn(n_rows, row_len, generator=g_)
    gg = v.norm(dim=1) if g_is_norm else torch.randn(n_rows, generator=g_)
    v_d, g_d, dw_d = v.to(cuda), gg.to(cuda), dw.to(cuda)
    dv, vbuf, pad = _canary((n_rows, row_len), cuda)
    dg, gbuf, _ = _canary((n_rows,), cuda)
    _call("fac_weight_norm_bwd", _p(v_d), _p(g_d), _p(dw_d), _p(dv), _p(dg), n_rows, row_len)
    torch.cuda.synchronize()
    assert _canary_intact(vbuf, pad) and _canary_intact(gbuf, pad)
    v64, dw64, g64 = v.double(), dw.double(), gg.double()
    nrm = v64.norm(dim=1)
    dot = (dw64 * v64).sum(1)
    dotmag = (dw64 * v64).abs().sum(1)
    dg_ref = dot / nrm
    tag = f"{n_rows}x{row_len}_{'gnorm' if g_is_norm else 'gfree'}"
    # dg: the dot product's reduction error, plus the relative error of ||v|| (a sum of squares: sqrt(n) 2^-24, halved by the root)
    _sum_bound(f"weight_norm_bwd_dg_{tag}", dg.cpu(), dg_ref, dotmag / nrm, row_len, extra=4.0)
    # dv = g/||v|| (dw - v c), c = dot / ||v||^2: error of c (reduction bound on dot / ||v||^2) times |v|, plus the elementwise ops
    k = (4 * math.sqrt(row_len) + 8) * EPS32
    c_mag = dotmag / (nrm * nrm)
    bound = (g64 / nrm).abs().view(-1, 1) * (k * c_mag.view(-1, 1) * v64.abs() + 4 * EPS32 * (dw64.abs() + v64.abs() * c_mag.view(-1, 1)))
    dv_ref = (g64 / nrm).view(-1, 1) * (dw64 - v64 * (dot / (nrm * nrm)).view(-1, 1))
    err = (dv.cpu().double() - dv_ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    _record(f"weight_norm_bwd_dv_{tag}", {"gpu_over_bound": ratio, "n": row_len})
    assert ratio <= 1.0, ratio
    # <dv, v> = 0: what is left is the rounding above, summed over the row
    tang = (dv.cpu().double() * v64).sum(1).abs()
    assert bool((tang <= (bound * v64.abs()).sum(1) + 1e-300).all())


# ======================================================================================================= D. predictor / quantizer side
def _aa_snakebeta_fwd_ref(x, alpha_log, beta_log, filt):
    """fac_aa_snakebeta_fwd restated: replicate-pad 5 / 5, upsample by 2 with the 12-tap filter (x 2), SnakeBeta with exp of the
    log-scale parameters, replicate-pad 5 / 6, the same filter at stride 2 (oracle/facodec_oracle.py aa_snakebeta)."""
    F = torch.nn.functional
    Cc = x.shape[1]
    f = filt.view(1, 1, 12).expand(Cc, -1, -1)
    u = 2 * F.conv_transpose1d(F.pad(x, (5, 5), mode="replicate"), f, stride=2, groups=Cc)[..., 15:-15]
    a = torch.exp(alpha_log).view(1, -1, 1)
    b = torch.exp(beta_log).view(1, -1, 1)
    u = u + torch.sin(u * a).pow(2) / (b + 1e-9)
    return F.conv1d(F.pad(u, (5, 6), mode="replicate"), f, stride=2, groups=Cc)


def _kaiser_sinc_filter12():
    """alias_free_torch/filter.py kaiser_sinc_filter1d(cutoff 0.25, half_width 0.3, 12 taps)."""
    k, cutoff, hw = 12, 0.25, 0.3
    A = 2.285 * (k // 2 - 1) * math.pi * 4 * hw + 7.95
    beta = 0.1102 * (A - 8.7) if A > 50 else (0.5842 * (A - 21) ** 0.4 + 0.07886 * (A - 21) if A >= 21 else 0.0)
    win = torch.kaiser_window(k, beta=beta, periodic=False, dtype=torch.float64)
    t = torch.arange(-(k // 2), k // 2, dtype=torch.float64) + 0.5
    f = 2 * cutoff * win * torch.sinc(2 * cutoff * t)
    return (f / f.sum()).float()


@gpu
@pytest.mark.parametrize("B,Cc", [(1, 1), (2, 64), (3, 130)])
@pytest.mark.parametrize("T", [1, 11, 12, 255, 256, 257, 3000])
def test_aa_snakebeta_bwd_fp64(cuda, B, Cc, T):
    """fac_aa_snakebeta_bwd against float64 autograd through the restated forward, at lengths around the filter (12) and the 128 /
    256-sample tiles; dx at the first and last 12 samples (edge handling: replicate padding folds several taps onto x[0] and
    x[T-1]) separately from the interior; dalpha / dbeta as reductions; a canary around the documented scratch."""
    g = _g(B * 1000 + Cc + T)
    x = torch.randn(B, Cc, T, generator=g)
    al = torch.randn(Cc, generator=g) * 0.5
    be = torch.randn(Cc, generator=g) * 0.5
    dy = torch.randn(B, Cc, T, generator=g)
    filt = _kaiser_sinc_filter12()

    def autograd_ref(dtype):
        xx, aa, bb = (t.to(dtype).clone().requires_grad_() for t in (x, al, be))
        y = _aa_snakebeta_fwd_ref(xx, aa, bb, filt.to(dtype))
        per = torch.autograd.grad((y * dy.to(dtype)).sum(), [xx, aa, bb])
        return per

    r64, r32 = autograd_ref(torch.float64), autograd_ref(torch.float32)
    x_d, al_d, be_d, f_d, dy_d = (t.to(cuda) for t in (x, al, be, filt, dy))
    dx, xbuf, pad = _canary((B, Cc, T), cuda)
    da, abuf, _ = _canary((Cc,), cuda)
    db, bbuf, _ = _canary((Cc,), cuda)
    scratch, sbuf, _ = _canary((2 * B * Cc * ((T + 255) // 256),), cuda)
    _call("fac_aa_snakebeta_bwd", _p(x_d), _p(al_d), _p(be_d), _p(f_d), _p(dy_d), _p(dx), _p(da), _p(db), _p(scratch), B, Cc, T)
    torch.cuda.synchronize()
    assert all(_canary_intact(b, pad) for b in (xbuf, abuf, bbuf, sbuf))
    dxc = dx.cpu()
    mag = r64[0].abs().max().clamp_min(1e-300)
    tag = f"{B}x{Cc}x{T}"
    e = min(12, T)
    parts = [("head12", slice(0, e)), ("tail12", slice(T - e, T))] + ([("interior", slice(12, T - 12))] if T > 24 else [])
    fails = []
    # dx is a 12 x 12-tap double convolution around the activation: the fp32-CPU conv is the same sum in another order
    for nm, sl in parts:
        try:
            _bar(f"aa_snakebeta_bwd_dx_{nm}_{tag}", dxc[..., sl], r64[0][..., sl], r32[0][..., sl],
                 scale=mag.expand_as(r64[0][..., sl]))
        except AssertionError as err:
            fails.append(str(err)[:300])
    # dalpha / dbeta: sums over B * 2T activation positions of products of O(1) factors; the per-position terms are not exposed by
    # autograd, so the magnitude is the sum over positions of |d a[m]| * |d act / d param|, recomputed here in fp64
    with torch.no_grad():
        Fn = torch.nn.functional
        f64 = filt.double().view(1, 1, 12).expand(Cc, -1, -1)
        u = 2 * Fn.conv_transpose1d(Fn.pad(x.double(), (5, 5), mode="replicate"), f64, stride=2, groups=Cc)[..., 15:-15]
    uu = u.clone().requires_grad_()
    a64, b64 = torch.exp(al.double()).view(1, -1, 1), torch.exp(be.double()).view(1, -1, 1)
    act = uu + torch.sin(uu * a64).pow(2) / (b64 + 1e-9)
    y = Fn.conv1d(Fn.pad(act, (5, 6), mode="replicate"), f64, stride=2, groups=Cc)
    (d_act,) = torch.autograd.grad((y * dy.double()).sum(), [act])
    ud = u
    ta = (d_act * torch.sin(2 * ud * a64) * ud * a64 / (b64 + 1e-9)).abs().sum((0, 2))
    tb = (d_act * torch.sin(ud * a64).pow(2) * b64 / (b64 + 1e-9) ** 2).abs().sum((0, 2))
    # the sin / cos argument theta = u e^alpha is a rounded quantity: u is a 6-tap fp32 sum (<= 4 half-ulps of sum |x f|, which
    # cancellation can leave far above |u|), e^alpha an expf (2 half-ulps) and the product one more: d theta below, and each
    # term moves by |d term / d theta| d theta
    with torch.no_grad():
        umag = 2 * Fn.conv_transpose1d(Fn.pad(x.double().abs(), (5, 5), mode="replicate"), f64.abs(), stride=2, groups=Cc)[..., 15:-15]
    th = ud * a64
    dth = EPS32 * (4 * a64 * umag + 4 * th.abs())
    ea_ = (d_act.abs() * dth * (2 * th.abs() * torch.cos(2 * th).abs() + torch.sin(2 * th).abs()) / (b64 + 1e-9)).sum((0, 2))
    eb_ = (d_act.abs() * dth * torch.sin(2 * th).abs() * b64 / (b64 + 1e-9) ** 2).sum((0, 2))
    n = B * 2 * T
    for nm, got, ref, tm, ae_ in (("dalpha", da, r64[1], ta, ea_), ("dbeta", db, r64[2], tb, eb_)):
        try:
            # each term: d a[m] is itself a 6-tap fp32 sum, u a 6-tap sum, sincos, exp: extra = 32 half-ulps of |terms|
            _sum_bound(f"aa_snakebeta_bwd_{nm}_{tag}", got.cpu(), ref, tm, n, extra=32.0, abs_extra=ae_)
        except AssertionError as err:
            fails.append(str(err)[:300])
    assert not fails, fails


def _span(n, seed, lim=30.0):
    """n values covering [-lim, lim] (the ends included) in random order."""
    g = _g(seed)
    v = (torch.rand(n, generator=g) * 2 - 1) * lim
    v[0] = -lim
    v[-1] = lim
    if n > 2:
        v[1] = 0.0
    return v


ELEMENTWISE_N = [1, 1001, 65535 * 256 + 4099]


def _sigmoid(t):
    return 1 / (1 + torch.exp(-t))


def _softplus_tanh(x):
    return torch.tanh(torch.log1p(torch.exp(-x.abs())) + x.clamp_min(0))       # tanh(softplus(x)), overflow-free


@gpu
@pytest.mark.parametrize("n", ELEMENTWISE_N)
def test_mish_fwd_and_bwd_fp64(cuda, n):
    """fac_mish_fwd: y = x tanh(softplus(x)); fac_mish_bwd: dx = d (tanh(sp) + x (1 - tanh(sp)^2) sigmoid(x)), x over [-30, 30]."""
    x, d = _span(n, n), torch.randn(n, generator=_g(n + 1))

    def ref(dtype):
        xx, dd = x.to(dtype), d.to(dtype)
        th = _softplus_tanh(xx)
        return xx * th, dd * (th + xx * (1 - th * th) * _sigmoid(xx))

    (y64, dx64), (y32, dx32) = ref(torch.float64), ref(torch.float32)
    x_d, d_d = x.to(cuda), d.to(cuda)
    y, ybuf, pad = _canary((n,), cuda)
    dx, xbuf, _ = _canary((n,), cuda)
    _call("fac_mish_fwd", _p(x_d), _p(y), n)
    _call("fac_mish_bwd", _p(x_d), _p(d_d), _p(dx), n)
    torch.cuda.synchronize()
    assert _canary_intact(ybuf, pad) and _canary_intact(xbuf, pad)
    _bar(f"mish_fwd_n{n}", y.cpu(), y64, y32, scale=y64.abs().clamp_min(1e-300))
    x6 = x.double()
    th = _softplus_tanh(x6)
    scale = d.double().abs() * (th + (x6 * (1 - th * th) * _sigmoid(x6)).abs())
    _bar(f"mish_bwd_n{n}", dx.cpu(), dx64, dx32, scale=scale.clamp_min(1e-300))


@gpu
@pytest.mark.parametrize("B,Cc,T", [(1, 1, 1), (3, 7, 11), (2, 64, 65535 * 2 + 33)])
@pytest.mark.parametrize("kind", ["gate", "glu"])
def test_gate_bwd_and_glu_bwd_fp64(cuda, kind, B, Cc, T):
    """fac_gate_bwd (acts = tanh(a1) sigmoid(a2): da1 = d sig (1 - th^2), da2 = d th sig (1 - sig)) and fac_glu_bwd (y = res + a1
    sigmoid(a2): da1 = d sig, da2 = d a1 sig (1 - sig)) on a = [a1 | a2] (B, 2C, T), arguments over [-30, 30]."""
    n = B * Cc * T
    a = _span(2 * n, n).view(B, 2 * Cc, T)
    d = torch.randn(B, Cc, T, generator=_g(n + 2))

    def ref(dtype):
        aa, dd = a.to(dtype), d.to(dtype)
        a1, a2 = aa[:, :Cc], aa[:, Cc:]
        sg = _sigmoid(a2)
        if kind == "gate":
            th = torch.tanh(a1)
            return torch.cat([dd * sg * (1 - th * th), dd * th * sg * (1 - sg)], 1)
        return torch.cat([dd * sg, dd * a1 * sg * (1 - sg)], 1)

    r64, r32 = ref(torch.float64), ref(torch.float32)
    a_d, d_d = a.to(cuda), d.to(cuda)
    da, buf, pad = _canary((B, 2 * Cc, T), cuda)
    _call(f"fac_{kind}_bwd", _p(a_d), _p(d_d), _p(da), B, Cc, T)
    torch.cuda.synchronize()
    assert _canary_intact(buf, pad)
    # scale: without the cancelling factors (1 - th^2) = (1 - th)(1 + th) and (1 - sig), whose fp32 forms lose all digits at |a| > 9
    a6, d6 = a.double(), d.double().abs()
    sg = _sigmoid(a6[:, Cc:])
    scale = torch.cat([d6 * sg, d6 * sg * (a6[:, :Cc].abs() if kind == "glu" else 1.0)], 1)
    _bar(f"{kind}_bwd_{B}x{Cc}x{T}", da.cpu(), r64, r32, scale=scale.clamp_min(1e-300))


@gpu
@pytest.mark.parametrize("n", ELEMENTWISE_N)
def test_tanh_bwd_and_mul_scaled_fp64(cuda, n):
    """fac_tanh_bwd: dx = dy (1 - y^2) from the saved output y; fac_mul_scaled: out = a b scale.  Two / three rounded fp32
    operations on inputs: 4 ulp of the uncancelled terms."""
    g = _g(n)
    y = torch.tanh(_span(n, n, 10.0))
    dy, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    y_d, dy_d, b_d = y.to(cuda), dy.to(cuda), b.to(cuda)
    dx, xbuf, pad = _canary((n,), cuda)
    out, obuf, _ = _canary((n,), cuda)
    _call("fac_tanh_bwd", _p(y_d), _p(dy_d), _p(dx), n)
    _call("fac_mul_scaled", _p(dy_d), _p(b_d), _p(out), -0.37, n)
    torch.cuda.synchronize()
    assert _canary_intact(xbuf, pad) and _canary_intact(obuf, pad)
    ref = dy.double() * (1 - y.double() ** 2)
    assert bool(((dx.cpu().double() - ref).abs() <= 4 * EPS32 * dy.double().abs() * (1 + y.double() ** 2)).all())
    ref2 = dy.double() * b.double() * _f32(-0.37)
    assert bool(((out.cpu().double() - ref2).abs() <= 4 * EPS32 * ref2.abs()).all())


@gpu
@pytest.mark.parametrize("B,per", [(1, 1), (3, 1001), (2, 65535 * 128 + 77)])
@pytest.mark.parametrize("has_w,has_c,sign", [(True, True, 1.0), (True, True, -1.0), (False, True, -1.0), (True, False, 1.0),
                                              (False, False, 1.0)], ids=["w_c_plus", "w_c_minus", "c_minus", "w_only", "copy"])
def test_rows_fma_fp64(cuda, B, per, has_w, has_c, sign):
    """fac_rows_fma: out[b][i] = a[b][i] w[b] + sign c[b][i], w and / or c NULL, both signs; without w and c an exact copy."""
    g = _g(B + per)
    a, c, w = torch.randn(B, per, generator=g), torch.randn(B, per, generator=g), torch.randn(B, generator=g)
    a_d, c_d, w_d = a.to(cuda), c.to(cuda), w.to(cuda)
    out, buf, pad = _canary((B, per), cuda)
    _call("fac_rows_fma", _p(a_d), _p(w_d if has_w else None), _p(c_d if has_c else None), _p(out), B, per, sign)
    torch.cuda.synchronize()
    assert _canary_intact(buf, pad)
    t1 = a.double() * (w.double().view(-1, 1) if has_w else 1.0)
    t2 = sign * c.double() if has_c else torch.zeros_like(t1)
    if not has_w and not has_c:
        assert torch.equal(out.cpu(), a)
    assert bool(((out.cpu().double() - (t1 + t2)).abs() <= 2 * EPS32 * (t1.abs() + t2.abs())).all())


@gpu
@pytest.mark.parametrize("mask_kind", ["null", "ragged", "zero_row"])
@pytest.mark.parametrize("B,Cc,T", [(1, 1, 1), (3, 5, 77), (4, 512, 188)])
def test_masked_mean_bwd_fp64(cuda, B, Cc, T, mask_kind):
    """fac_masked_mean_bwd: the forward is x.sum(2) / mask.sum(2) (modules/style_encoder.py:83-91 as restated in the oracle's
    style_encoder_forward: x is NOT multiplied by the mask in the pooling), so dx[b, c, t] = dout[b, c] / len_b at EVERY t.  A clip
    whose mask is all zero has len = 0: the reference divides by zero, the gradient of non-zero dout is +-inf there -- never NaN."""
    g = _g(B * T + Cc)
    dout = torch.randn(B, Cc, generator=g)
    dout[dout == 0] = 1.0
    mask = None
    if mask_kind != "null":
        lens = torch.randint(1, T + 1, (B,), generator=g)
        lens[0] = T
        if mask_kind == "zero_row":
            lens[-1] = 0
        mask = (torch.arange(T).view(1, T) < lens.view(B, 1)).float()
    d_d = dout.to(cuda)
    m_d = mask.to(cuda) if mask is not None else None
    dx, buf, pad = _canary((B, Cc, T), cuda)
    _call("fac_masked_mean_bwd", _p(d_d), _p(m_d), _p(dx), B, Cc, T)
    torch.cuda.synchronize()
    assert _canary_intact(buf, pad)
    ln = mask.double().sum(1) if mask is not None else torch.full((B,), float(T), dtype=torch.float64)
    ref = (dout.double() / ln.view(B, 1)).unsqueeze(2).expand(B, Cc, T)
    got = dx.cpu().double()
    assert not bool(torch.isnan(got).any())
    fin = torch.isfinite(ref)
    assert torch.equal(got[~fin], ref[~fin])                                # +-inf with dout's sign where len = 0
    assert bool(((got[fin] - ref[fin]).abs() <= 2 * EPS32 * ref[fin].abs()).all())       # one correctly rounded division


def _attn_ref(q, k, v, mask, B, H, dk, T, keep=None):
    """softmax(q^T k / sqrt(dk) + mask) v on (B, H*dk, T) tensors; masked pairs get the score -1e4 (modules/attentions.py:168-199);
    keep (B, H, T, T): dropout factor applied to P.  Returns o (B, H*dk, T) and P."""
    qh, kh, vh = (t.view(B, H, dk, T).transpose(2, 3) for t in (q, k, v))
    sc = qh @ kh.transpose(2, 3) / dk ** 0.5
    if mask is not None:
        m2 = (mask.unsqueeze(1) * mask.unsqueeze(2)).unsqueeze(1)
        sc = sc.masked_fill(m2 == 0, -1e4)
    P = torch.softmax(sc, -1)
    Pu = P * keep if keep is not None else P
    return (Pu @ vh).transpose(2, 3).reshape(B, H * dk, T), P


@gpu
@pytest.mark.parametrize("dropout", [False, True], ids=["P_used_is_P", "P_used_dropout"])
@pytest.mark.parametrize("masked", [False, True], ids=["mask_null", "ragged_mask"])
@pytest.mark.parametrize("T", [1, 50, 257])
def test_attention_kernels_fp64(cuda, T, masked, dropout):
    """fac_attention_probs, fac_attention_pv, fac_attention_bwd_pv, fac_attention_bwd_qk against float64 softmax attention and its
    autograd; P_used != P is dropout applied to P (the backward takes both).  Adding a constant to every key's score leaves the
    softmax unchanged, so the score gradient dS has zero row sums: asserted on the kernel's own dS instead of comparing noise."""
    B, H, dk = 2, 2, 64
    g = _g(T + 2 * masked + dropout)
    q, k, v = (torch.randn(B, H * dk, T, generator=g) for _ in range(3))
    w = torch.randn(B, H * dk, T, generator=g)
    mask = None
    if masked:
        mask = torch.ones(B, T)
        mask[0, T - min(17, T // 2):] = 0
    keep = ((torch.rand(B, H, T, T, generator=g) > 0.25).float() / 0.75) if dropout else None

    def ref(dtype):
        qq, kk, vv = (t.to(dtype).clone().requires_grad_() for t in (q, k, v))
        o, P = _attn_ref(qq, kk, vv, mask.to(dtype) if masked else None, B, H, dk, T, keep.to(dtype) if dropout else None)
        grads = torch.autograd.grad((o * w.to(dtype)).sum(), [qq, kk, vv])
        return o.detach(), P.detach(), grads

    (o64, P64, g64), (o32, P32, g32) = ref(torch.float64), ref(torch.float32)
    q_d, k_d, v_d, w_d = (t.to(cuda) for t in (q, k, v, w))
    m_d = mask.to(cuda) if masked else None
    P, pbuf, pad = _canary((B, H, T, T), cuda)
    _call("fac_attention_probs", _p(q_d), _p(k_d), _p(m_d), _p(P), B, H, dk, T)
    Pu = P * keep.to(cuda) if dropout else P
    o, obuf, _ = _canary((B, H * dk, T), cuda)
    _call("fac_attention_pv", _p(Pu), _p(v_d), _p(o), B, H, dk, T)
    dv, vbuf, _ = _canary((B, H * dk, T), cuda)
    dP, dpbuf, _ = _canary((B, H, T, T), cuda)
    _call("fac_attention_bwd_pv", _p(Pu), _p(v_d), _p(w_d), _p(dv), _p(dP), B, H, dk, T)
    if dropout:
        dP.mul_(keep.to(cuda))                                  # the dropout's own backward (fac_mul_scaled in the Function)
    dP_in = dP.clone()
    dq, qbuf, _ = _canary((B, H * dk, T), cuda)
    dkk, kbuf, _ = _canary((B, H * dk, T), cuda)
    _call("fac_attention_bwd_qk", _p(P), _p(dP), _p(q_d), _p(k_d), _p(m_d), _p(dq), _p(dkk), B, H, dk, T)
    torch.cuda.synchronize()
    assert all(_canary_intact(b, pad) for b in (pbuf, obuf, vbuf, dpbuf, qbuf, kbuf))
    tag = f"T{T}_{'mask' if masked else 'nomask'}_{'drop' if dropout else 'nodrop'}"
    Pc = P.cpu()
    assert bool(((Pc.double().sum(-1) - 1).abs() <= 4 * math.sqrt(T) * EPS32 + 4 * EPS32).all())
    fails = []
    for nm, got, r64, r32 in (("P", Pc, P64, P32), ("o", o.cpu(), o64, o32), ("dq", dq.cpu(), g64[0], g32[0]),
                              ("dk", dkk.cpu(), g64[1], g32[1]), ("dv", dv.cpu(), g64[2], g32[2])):
        try:
            _bar(f"attention_{nm}_{tag}", got, r64, r32)
        except AssertionError as e:
            fails.append(str(e)[:300])
    # dS (dP after fac_attention_bwd_qk, in place) = P (dP - s), s = sum_j P_j dP_j: its rows sum to s (1 - sum P) = 0 up to the
    # rounding of a T-term sum of |P_j| (|dP_j| + |s|)
    dS, Pd, dPd = dP.cpu().double(), Pc.double(), dP_in.cpu().double()
    srow = (Pd * dPd).sum(-1, keepdim=True)
    mag = (Pd * (dPd.abs() + srow.abs())).sum(-1)
    rowsum = dS.sum(-1).abs()
    assert bool((rowsum <= (4 * math.sqrt(T) + 8) * EPS32 * mag + 1e-300).all()), float((rowsum / mag.clamp_min(1e-300)).max())
    assert not fails, fails


# ======================================================================================================= argument validation (no GPU)
def test_entry_points_of_this_file_are_declared():
    """Every C entry this file drives is declared in facodec_amd/_lib.py with a stream as its last argument (runs without a GPU:
    a renamed or re-ordered prototype fails here, not as a crash in a launch)."""
    names = ["fac_lstm_layer_fwd_train", "fac_lstm_layer_fwd_from", "fac_lstm_layer_fwd_persist", "fac_lstm_layer_bwd",
             "fac_lstm_layer_bwd_persist", "fac_lstm_gate_bwd", "fac_lstm_persist_ok", "fac_adamw_step", "fac_adamw_step_masked",
             "fac_grad_norm_clip", "fac_vq_latent_bwd", "fac_vq_codebook_grad", "fac_snake_bwd", "fac_snake_bwd_fused",
             "fac_snake_bwd_fused_rs", "fac_bias_grad", "fac_weight_norm_bwd", "fac_aa_snakebeta_bwd", "fac_gate_bwd", "fac_mish_fwd",
             "fac_mish_bwd", "fac_glu_bwd", "fac_mul_scaled", "fac_masked_mean_bwd", "fac_tanh_bwd", "fac_rows_fma",
             "fac_attention_probs", "fac_attention_pv", "fac_attention_bwd_pv", "fac_attention_bwd_qk"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "facodec_hip.h")).read()
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "fac_adamw_step" in v)
    for n in names:
        assert n in table, n
        assert f"int {n}(" in header, n
        if n != "fac_lstm_persist_ok":
            assert table[n][1][-1] is C.c_void_p, n


def test_lstm_dispatch_restatement_covers_every_branch():
    """The H values of LSTM_CASES reach every instantiation fac_lstm_layer_fwd_train and fac_lstm_layer_bwd choose from H / 8."""
    fwd = {_fwd_branch(c[0]) for c in LSTM_CASES}
    bwd = {_bwd_branch(c[0]) for c in LSTM_CASES}
    assert fwd == {"fwd8w", "fwd16x1", "fwd16x2", "fwd16x4", "fwd16xrt", "fwd16x8", "fwd16x12"}
    assert bwd == {"bwd8w", "bwd16xrt", "bwd16x8", "bwd16x12"}
    assert {c[2] for c in LSTM_CASES} >= {1, 2, 33, 160} and {c[1] for c in LSTM_CASES} >= {1, 5, 16, 17, 32}
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "facodec_amd", "csrc", "lstm.hip")).read()
    for inst in ("lstm_step_kernel<16, 12>", "lstm_step_kernel<16, 8>", "lstm_step_kernel<16, 4>", "lstm_step_kernel<16, 2>",
                 "lstm_step_kernel<16, 1>", "lstm_step_kernel<16, 0>", "lstm_step_kernel<8, 0>", "lstm_rec_bwd_kernel<16, 12>",
                 "lstm_rec_bwd_kernel<16, 8>", "lstm_rec_bwd_kernel<16, 0>", "lstm_rec_bwd_kernel<8, 0>"):
        assert inst in src, inst
