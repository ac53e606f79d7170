"""The layout / launch-form planner (facodec_amd/convplan.py) on the model's own layers, without a GPU.

1. Decision table: every conv of the codec and of the discriminators, at the benchmark's inference shape (B = 32 x 2 s) and its
   training shape (B = 16 x 2 s) -- encoder, FA quantizer (WaveNet, style encoder), decoder, the redecoder's WaveNet and non-causal
   decoder --, gets the plan recorded in tests/golden/conv_plan_table.json.  That file was written from the
   if / elif chains the planner replaced (the commit before it), evaluated on the rows this module enumerates -- not from the
   planner -- so it pins the policy across the move: one row per distinct (site, shape).
2. Every row's launch descriptor goes through fac_conv1d_variant (host only): the C++ planner must pick the kernel family the
   Python plan packed weights for.  The plan is asked of the site's own shape-only function and the descriptor is built by the
   product's builders (ops.conv_desc / ops.convtr_desc and the flat-geometry functions): `launch_desc` below.  The GPU tests
   (tests/test_conv_launch_desc.py, tests/test_conv_bwd_data.py) hold a real launch's descriptor to the same `launch_desc`.
3. The data-gradient plan of a stride-1 conv is the forward plan of the conv with the channels swapped.
"""
import ctypes
import json
import os

import pytest
import torch

from facodec_amd import _lib, convplan, layers, ops
from facodec_amd.commons import build_model, default_model_params

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_table.json")
SAMPLES = 48000                 # bench.py: CLIP_SECONDS * SAMPLE_RATE
B_INFER, B_TRAIN = 32, 16       # bench.py: --batch default, TRAIN_BATCH


def _stack_rows(net, T, units, tanh_last=False, frames=None):
    """(site, args) of every planner call a stack of SConv1d / SConvTranspose1d / SLSTM / _PlainConv modules makes at both
    benchmark shapes; args are the site's own facts.  units: k = 7 / k = 1 convs with C_in == C_out sit in ResidualUnits; a
    WaveNet's cond_layer and the style encoder's `fc` see one column (the timbre vector / the pooled frame)."""
    from facodec_amd.quantize import _PlainConv
    rows = []
    mods = [(n, m) for n, m in net.named_modules() if isinstance(m, (layers.SConv1d, layers.SConvTranspose1d, layers.SLSTM, _PlainConv))]
    last = [m for _, m in mods if isinstance(m, layers.SConv1d)][-1:]
    for B, train in ((B_INFER, False), (B_TRAIN, True)):
        t = T
        for name, m in mods:
            if isinstance(m, layers.SConv1d):
                co, ci, k, s, d = m.w.c_out, m.w.c_in, m.kernel_size, m.stride, m.dilation
                cr = m.causal and m.pad_mode == ops.PAD_REFLECT
                tt = 1 if name.endswith("cond_layer") else t
                unit = units and k in (7, 1) and co == ci and m is not last[0]
                tanh = tanh_last and m is last[0]
                if not train:       # SConv1d.run: (..., alpha_in, plain, res, causal_reflect, grad)
                    plain, res = (False, k == 1) if unit else (not tanh, False)
                    rows.append(("layers.SConv1d.run", (co, ci, k, s, d, B, tt, False, plain, res, cr, False)))
                else:
                    if unit:
                        rows.append(("autograd._ResUnit.forward", (co, ci, k, d, B, tt)))
                    else:
                        rows.append(("autograd._Conv.forward", (co, ci, k, s, d, B, tt, not tanh, cr)))
                    if s == 1:
                        rows.append(("ops.conv1d_bwd_data(stride 1)", (co, ci, k, d, B, tt, m.causal)))
                    else:
                        rows.append(("ops.conv1d_bwd_data(strided)", (co, ci, s, B, -(-tt // s))))
                if tt == t:
                    t = -(-t // s)
            elif isinstance(m, layers.SConvTranspose1d):
                ci, co, s = m.w.c_in, m.w.c_out, m.stride
                if not train:
                    rows.append(("layers.SConvTranspose1d.run", (ci, co, s, B, t, m.causal, False, False)))
                else:
                    rows.append(("autograd._ConvTr.forward", (ci, co, s, B, t, m.causal)))
                    rows.append(("ops.conv_transpose1d_bwd", (ci, co, s, B, t)))
                t *= s
            elif isinstance(m, layers.SLSTM):
                H, cols = m.dimension, t * ops.pad32(B)
                rows.append(("plan_gemm", (4 * H, H, cols)))
                if train:
                    rows.append(("plan_gemm", (H, 4 * H, cols)))
            else:                   # _PlainConv: `same` zero padding, plain weights
                tt = 1 if name.endswith("fc") else t
                if not train:
                    rows.append(("quantize._PlainConv.run", (m.c_out, m.c_in, m.k, B, tt)))
                else:               # autograd_quant.plain_conv: _Conv with zero padding (the spectral convs carry a Mish)
                    rows.append(("autograd._Conv.forward", (m.c_out, m.c_in, m.k, 1, 1, B, tt, "spectral" not in name, False)))
                    rows.append(("ops.conv1d_bwd_data(stride 1)", (m.c_out, m.c_in, m.k, 1, B, tt, False)))
    return rows


def _disc_rows(disc):
    """PlainConv launches of the period / resolution discriminators on B_TRAIN clips: (c_out, c_in, k, k1, stride, pad, t_in) of
    the single row-concatenated signal (batch 1)."""
    from facodec_amd import autograd_disc
    from facodec_amd.discriminator import MPD, MRD
    rows = []
    for m in disc.modules():
        if isinstance(m, MPD):
            L, P = m.geometry(SAMPLES)
            ch = [1, 32, 128, 512, 1024, 1024]
            for i, s in enumerate(m.strides):
                rows.append((ch[i + 1], ch[i], 5, 0, s, 2, B_TRAIN * m.period * P[i], 0))
            rows.append((1, 1024, 3, 0, 1, 1, B_TRAIN * m.period * P[5], 0))
        elif isinstance(m, MRD):
            win, hop = m.window_length, m.window_length // 4
            pad = (win - hop) // 2
            frames = (SAMPLES + 2 * pad + (-(-SAMPLES // hop) * hop - SAMPLES)) // hop + 1 - 4      # autograd_disc.Spectrogram
            R = B_TRAIN * (frames + 1)
            widths = []
            for lo, hi in m.bands:
                F, P = m.geometry(hi - lo)
                for i, sf in enumerate(m.fstrides):
                    kf = 3 if i == 4 else 9
                    rows.append((32, 2 if i == 0 else 32, 3 * kf, kf, sf, P[i] + kf // 2, R * P[i], P[i]))
                widths.append(F[5])
            Pp = sum(widths) + 2
            rows.append((1, 32, 9, 3, 1, Pp + 1, R * Pp, Pp))
    out = []
    for co, ci, k, k1, s, pad, t_in, dil2 in rows:
        max_off = autograd_disc.tap_span(k, k1, dil2)
        t_out = (t_in + 2 * pad - max_off - 1) // s + 1
        out.append(("autograd_disc.PlainConv.forward", (co, ci, k, k1, s, 1, t_in, t_out, pad, dil2)))
        if s > 1 and not k1 and k <= 2 * s:
            out.append(("autograd_disc.PlainConv.backward(transposed)", (co, ci, s, 1, t_out + 1)))
        elif ci > 2:                                                             # (the first layers' inputs need no gradient rows)
            tu = (t_out - 1) * s + 1
            out.append(("autograd_disc.PlainConv.backward(stride-1 conv)", (co, ci, k, k1, 1, tu, t_in, max_off - pad, dil2)))
    return out


def _stub(**kw):
    return type("Stub", (), kw)()


def plan(site, a):
    """What the site asks the planner, as plain lists (JSON): every site is asked through its own shape-only function -- the one
    its launch code calls -- or, for the modules, its plan method on a stub that carries only the attributes that method reads."""
    from facodec_amd import autograd, autograd_disc
    from facodec_amd.quantize import _PlainConv
    if site == "layers.SConv1d.run":
        co, ci, k, s, d, B, T, alpha, plain, res, cr, grad = a
        m = _stub(w=_stub(c_out=co, c_in=ci), kernel_size=k, stride=s, dilation=d, causal=cr, pad_mode=ops.PAD_REFLECT)
        with torch.set_grad_enabled(grad):
            p = layers.SConv1d.plan(m, B, T, alpha, plain, res)
    elif site == "quantize._PlainConv.run":
        co, ci, k, B, T = a
        p = _PlainConv.plan(_stub(c_out=co, c_in=ci, k=k), B, T)
    elif site == "autograd._Conv.forward":
        p = autograd.plan_conv_fwd(*a)
    elif site == "autograd._ResUnit.forward":
        co, ci, k, d, B, T = a
        p = autograd.plan_res_unit(co, ci, d, B, T)[0 if k == 7 else 1]
    elif site == "ops.conv1d_bwd_data(stride 1)":
        co, ci, k, d, B, T, causal = a
        p = ops.plan_bwd_data(co, ci, k, 1, d, B, T, causal)[0]
    elif site == "ops.conv1d_bwd_data(strided)":
        co, ci, s, B, t_out = a
        p, t_o = ops.plan_bwd_data(co, ci, 2 * s, s, 1, B, t_out * s)[:2]
        assert t_o == t_out
    elif site == "ops.conv_transpose1d_bwd":
        p = ops.plan_convtr_bwd(*a)
    elif site == "layers.SConvTranspose1d.run":
        ci, co, s, B, T, causal, alpha, grad = a
        with torch.set_grad_enabled(grad):
            p = layers.SConvTranspose1d.plan(_stub(w=_stub(c_in=ci, c_out=co), stride=s, causal=causal), B, T, alpha)
    elif site == "autograd._ConvTr.forward":
        p = autograd.plan_convtr_fwd(*a)
    elif site == "autograd_disc.PlainConv.forward":
        co, ci, k, k1, s, B, t_in, t_out = a[:8]
        p = autograd_disc._plan(co, ci, k, s, B, t_in, t_out, k1)
    elif site == "autograd_disc.PlainConv.backward(stride-1 conv)":
        p = _disc_bwd_stride1(a)[0]
    elif site == "autograd_disc.PlainConv.backward(transposed)":
        p = autograd_disc.plan_bwd_transposed(*a)
    else:                                    # plan_gemm rows: the LSTM input projection (4H, H) and its data gradient (H, 4H)
        co, ci, cols = a
        p = ops.plan_lstm_proj(ci, cols) if co == 4 * ci else ops.plan_lstm_proj_bwd(co, cols)
    return list(p)


def _disc_bwd_stride1(a):
    """PlainConv.backward's own (plan, max_off, pl, tp, shift) for a table row, whose tp and shift columns it must reproduce."""
    from facodec_amd import autograd_disc
    co, ci, k, k1, B, tu, tp, shift, dil2 = a
    got = autograd_disc.plan_bwd_stride1(co, ci, k, k1, dil2, autograd_disc.tap_span(k, k1, dil2) - shift, B, tu, tp)
    assert got[3:] == (tp, shift), (a, got)
    return got


def all_rows():
    """Codec (encoder, FA quantizer, decoder), discriminators, and the redecoder with its non-causal, LSTM-free decoder."""
    from facodec_amd.commons import default_redecoder_params
    model = build_model(default_model_params())
    red = build_model(default_redecoder_params(), stage="redecoder")
    frames = SAMPLES // 300
    return (_stack_rows(model.encoder, SAMPLES, True) + _stack_rows(model.quantizer, frames, False)
            + _stack_rows(model.decoder, frames, True, tanh_last=True) + _disc_rows(model.discriminator)
            + _stack_rows(red.encoder, frames, False) + _stack_rows(red.decoder, frames, True, tanh_last=True))


@pytest.fixture(scope="module")
def rows():
    torch.manual_seed(0)
    seen, out = set(), []
    for r in all_rows():
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


def test_plans_match_the_recorded_decision_table(rows):
    table = json.load(open(GOLDEN))
    want = {(r["site"], tuple(r["args"])): r["plan"] for r in table}
    assert len(want) == len(table) and {(s, a) for s, a in rows} == set(want), "the table has one row per distinct (site, shape)"
    bad = [(s, a, plan(s, a), want[(s, a)]) for s, a in rows if plan(s, a) != want[(s, a)]]
    assert not bad, bad[:5]
    layouts = {p[0] for p in want.values()}
    assert {"split_taps", "split_gemm", "split_gemm_strided", "split2", "fp32", "fp32_pw_taps", "rows_split", "flat_rows_split",
            "polyphase"} <= layouts, layouts                    # the table exercises every family the model uses
    sconv = [a for s, a in rows if s == "layers.SConv1d.run"]
    assert any(a[2] == 5 for a in sconv) and any(not a[10] for a in sconv), "k = 5 WaveNet layers and non-causal layers are in the table"


FAMILY = {"split_taps": 11, "split_gemm": 15, "split_gemm_strided": 15, "split2": 16, "fp32_pw_taps": 18,
          "rows_split": 15, "flat_rows_split": 15, "rows_pw_taps": 18}
ROWS96 = 19         # a split_taps plan that convplan.tile_rows completes with 96: the 96 x 256 form of the same kernel has an id of its own
SPLIT_ONLY = ("split_taps", "split_gemm", "split_gemm_strided", "split2", "rows_split", "flat_rows_split")


def fake_operands(d, *names, gate_cond_bs=0):
    """Non-null pointers for x, y, the workspace and the operands named (w, w_split, bias, res, alpha_out, y2, alpha_y2, gate_cond,
    ...) on a descriptor from ops.conv_desc / ops.convtr_desc.  Never dereferenced: fac_conv1d_variant only reads the descriptor."""
    fake = ctypes.c_void_p(0x10000)
    d.x = d.y = d.ws = fake
    d.ws_bytes = ops.CONV_WS_BYTES
    for n in names:
        setattr(d, n, fake)
    if "gate_cond" in names:
        d.gate_cond_bs = gate_cond_bs
    return d


def assert_same_launch(got, want, what=""):
    """A launched descriptor against a CPU-built one: every non-pointer field equal, every pointer null in both or in neither
    (the workspace, which the launch itself hands over, aside)."""
    bad = []
    for name, ctype in _lib.ConvDesc._fields_:
        if name in ("ws", "ws_bytes"):
            continue
        g, w = getattr(got, name), getattr(want, name)
        if ctype is ctypes.c_void_p:
            g, w = bool(g), bool(w)
        if g != w:
            bad.append((name, g, w))
    assert not bad, (what, bad)


def conv_launch(layout, *shape, rows=64, operands=(), **kw):
    """ops.conv1d's descriptor for a plan layout: conv_desc(*shape, **kw) with the co-tile figure of a split-taps buffer (rows: 64
    at the training sites, convplan.tile_rows at the inference sites) and the weights the layout packs -- a split-only launch hands
    its buffer over as `w` too."""
    d = ops.conv_desc(*shape, split_rows=rows if layout == convplan.W_TAPS else 0, **kw)
    return fake_operands(d, "w", *(("w_split",) if layout in SPLIT_ONLY else ()), *operands)


def convtr_launch(layout, B, c_in, T, c_out, s, causal=True, operands=()):
    """ops.conv_transpose1d's descriptor for a transposed plan layout over B clips of T columns (flattened: as one signal)."""
    split = layout in (convplan.TR_ROWS_SPLIT, convplan.TR_FLAT)
    cp = ops.pad32(c_out) if layout == convplan.TR_POLYPHASE else ops.convtr_rows_pad(c_out, s)
    if layout == convplan.TR_FLAT:
        B, T = 1, ops.flat_convtr_cols(B, T)
    d = ops.convtr_desc(B, c_in, T, c_out, s, cp, causal, False, layout in (convplan.TR_ROWS, convplan.TR_ROWS_PW_TAPS), split)
    return fake_operands(d, "w_split" if split else "w", *operands)


def flat_conv_launch(layout, B, c_in, L, c_out, k, s, n, dilation=1, **kw):
    """ops.conv1d_flat's descriptor: B clips padded to L columns as one unpadded signal, n outputs kept per clip."""
    _, t_in, t_out = ops.flat_conv_cols(B, L, s, n)
    return conv_launch(layout, 1, c_in, t_in, c_out, k, s, dilation, 0, ops.PAD_ZERO, t_out, **kw)


def bwd_data_launch(co, ci, k, s, d, B, T, causal=True):
    """The gradient launch of ops.conv1d_bwd_data for the SConv1d ci -> co over B clips of T columns."""
    p, t_out, _, _, tp = ops.plan_bwd_data(co, ci, k, s, d, B, T, causal)
    if s > 1:
        return convtr_launch(p.layout, B, co, t_out + 1, ci, s)
    if p.layout == convplan.W_GEMM:
        return conv_launch(p.layout, B, co, t_out, ci, 1, 1, 1, 0, ops.PAD_ZERO, tp)
    return conv_launch(p.layout, B, co, t_out, ci, k, 1, d, (k - 1) * d, ops.PAD_ZERO, tp)


def convtr_bwd_launch(ci, co, s, B, T, causal=True):
    """The dx launch of ops.conv_transpose1d_bwd for the transposed conv ci -> co over B clips of T columns."""
    p = ops.plan_convtr_bwd(ci, co, s, B, T)
    if p.form == convplan.FLAT_STRIDED:
        return flat_conv_launch(p.layout, B, co, (T + 1) * s, ci, 2 * s, s, T)
    return conv_launch(p.layout, B, co, T * s, ci, 2 * s, s, 1, 0 if causal else s - s // 2, ops.PAD_ZERO, T)


def sconv_launch(p, co, ci, k, s, d, B, T, causal, pad_mode=ops.PAD_REFLECT, act=ops.ACT_NONE, rows=64, operands=("bias",)):
    """An SConv1d launch as layers.SConv1d.run / autograd._Conv.forward make it: per clip with the layer's padding rule, or the
    clips reflect-padded on the left by the causal padding and flattened."""
    if p[1] == convplan.PER_CLIP:
        return conv_launch(p[0], B, ci, T, co, k, s, d, None, pad_mode, None, act, causal, rows=rows, operands=operands)
    return flat_conv_launch(p[0], B, ci, T + ops.conv_out_len(T, k, s, d)[1], co, k, s, T // s, d, act=act, rows=rows, operands=operands)


def launch_desc(site, a, operands=None):
    """The descriptor of the conv the site launches for the table row (site, a), built by the product's own builders from the
    site's own plan.  operands: the optional operands the launch carries (default: what the model's layers hand that site)."""
    p = plan(site, a)
    Y2 = ("y2", "alpha_y2")
    if site == "layers.SConv1d.run":
        co, ci, k, s, d, B, T, _, plain, res, cr, _ = a
        if operands is None:
            operands = ("bias",) + (("res",) if res else ()) + (("alpha_out",) if not plain and not res else ()) + Y2
        return sconv_launch(p, co, ci, k, s, d, B, T, cr, rows=ops.tile_rows(co, ci, k), operands=operands)
    if site == "autograd._Conv.forward":
        co, ci, k, s, d, B, T, plain, cr = a
        return sconv_launch(p, co, ci, k, s, d, B, T, cr, ops.PAD_REFLECT if cr else ops.PAD_ZERO, ops.ACT_NONE if plain else ops.ACT_TANH)
    if site == "quantize._PlainConv.run":
        co, ci, k, B, T = a
        return conv_launch(p[0], B, ci, T, co, k, 1, 1, (k - 1) // 2, ops.PAD_ZERO, T, rows=ops.tile_rows(co, ci, k), operands=("bias",))
    if site == "autograd._ResUnit.forward":
        co, ci, k, d, B, T = a
        return conv_launch(p[0], B, ci, T, co, k, 1, d, operands=("bias",) + (("res",) if k == 1 else ()) + Y2)
    if site == "ops.conv1d_bwd_data(stride 1)":
        co, ci, k, d, B, T, causal = a
        return bwd_data_launch(co, ci, k, 1, d, B, T, causal)
    if site == "ops.conv1d_bwd_data(strided)":
        co, ci, s, B, t_out = a
        return bwd_data_launch(co, ci, 2 * s, s, 1, B, t_out * s)
    if site == "ops.conv_transpose1d_bwd":
        return convtr_bwd_launch(*a)
    if site in ("layers.SConvTranspose1d.run", "autograd._ConvTr.forward"):
        ci, co, s, B, T, causal = a[:6]               # flattened: a zero column in front of every clip
        return convtr_launch(p[0], B, ci, T + (p[0] == convplan.TR_FLAT), co, s, causal, ("bias",) if operands is None else operands)
    if site == "autograd_disc.PlainConv.forward":
        co, ci, k, k1, s, B, t_in, t_out, pad, dil2 = a
        return conv_launch(p[0], B, ci, t_in, co, k, s, 1, pad, ops.PAD_ZERO, t_out, k1=k1, dilation2=dil2, operands=("bias",))
    if site == "autograd_disc.PlainConv.backward(stride-1 conv)":
        co, ci, k, k1, B, tu = a[:6]
        _, _, _, tp, shift = _disc_bwd_stride1(a)
        return conv_launch(p[0], B, co, tu, ci, k, 1, 1, shift, ops.PAD_ZERO, tp, k1=k1, dilation2=a[8])
    if site == "autograd_disc.PlainConv.backward(transposed)":
        co, ci, s, B, T = a
        return convtr_launch(p[0], B, co, T, ci, s)
    co, ci, cols = a                         # plan_gemm rows: one signal of `cols` columns
    return conv_launch(p[0], 1, ci, cols, co, 1, 1, 1, 0, ops.PAD_ZERO, cols, operands=("bias",) if co == 4 * ci else ())


def test_cpp_planner_picks_the_family_the_python_plan_packed_for(rows):
    """The docstring claims "mirrors conv_gsplit_ok" etc. as a check: for every table row whose plan names a split / streaming-taps
    layout, fac_conv1d_variant on the descriptor the site launches names that kernel family."""
    checked, bad = 0, []
    for site, a in rows:
        p = plan(site, a)
        if p[0] not in FAMILY:
            continue
        d = launch_desc(site, a)
        got = ops.conv_variant(d)
        checked += 1
        if got[0] != (ROWS96 if d.split_rows == 96 else FAMILY[p[0]]):
            bad.append((site, a, p, got))
    assert checked > 40 and not bad, bad[:5]


def test_data_gradient_plan_is_the_forward_plan_with_channels_swapped():
    """ops.conv1d_bwd_data asks plan_conv(c_in, c_out, ...): equal to the training forward's plan of the swapped conv, and the
    split-taps channel floor moves with the roles (C_out >= 64 and C_in > 32 for the gradient of a k = 3 / 5 conv)."""
    for co in (16, 32, 48, 64, 256, 384, 1024):
        for ci in (16, 32, 48, 64, 256, 384, 1024):
            for k in (1, 3, 5, 7):
                for B, T in ((1, 640), (1, 641), (16, 4800), (32, 160)):
                    grad, _, _, _, tp = ops.plan_bwd_data(co, ci, k, 1, 1, B, T)      # the site's own call
                    assert tp == T + (k - 1)
                    fwd = convplan.plan_conv(c_out=ci, c_in=co, k=k, stride=1, dilation=1, batch=B, t_in=T, t_out=tp)
                    assert grad == fwd
                    if k in (3, 5) and grad.layout == convplan.W_TAPS:
                        assert co >= 64 and ci > 32
    assert convplan.plan_conv(48, 64, 5, 1, 1, 16, 4800, 4804).layout == convplan.W_TAPS       # gradient of a 48 -> 64 conv: floor met
    assert convplan.plan_conv(64, 48, 5, 1, 1, 16, 4800, 4804).layout == convplan.W_FP32       # gradient of a 64 -> 48 conv: not met
