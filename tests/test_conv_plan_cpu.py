"""The layout / launch-form planner (facodec_amd/convplan.py) on the model's own layers, without a GPU.

1. Decision table: every conv of the codec and of the discriminators, at the benchmark's inference shape (B = 32 x 2 s) and its
   training shape (B = 16 x 2 s) -- encoder, FA quantizer (WaveNet, style encoder), decoder, the redecoder's WaveNet and non-causal
   decoder --, gets the plan recorded in tests/golden/conv_plan_table.json.  That file was written from the
   if / elif chains the planner replaced (the commit before it), evaluated on the rows this module enumerates -- not from the
   planner -- so it pins the policy across the move: one row per distinct (site, shape).
2. Every row's launch descriptor goes through fac_conv1d_variant (host only): the C++ planner must pick the kernel family the
   Python plan packed weights for.
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
        max_off = (k // k1 - 1) * dil2 + (k1 - 1) if k1 else k - 1
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
    """What the site asks the planner, as plain lists (JSON).  The inference modules, _PlainConv and the discriminators are asked
    through their own plan methods (on stubs that carry only the attributes those read), so their flags are the sites' own."""
    from facodec_amd import autograd_disc
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
        co, ci, k, s, d, B, T, plain, cr = a
        p = convplan.plan_conv(co, ci, k, s, d, B, T, -(-T // s), plain=plain, causal_reflect=cr, flat_train="reflect")
    elif site == "autograd._ResUnit.forward":
        co, ci, k, d, B, T = a
        p = convplan.plan_conv(co, ci, k, 1, d, B, T, T)
    elif site == "ops.conv1d_bwd_data(stride 1)":
        co, ci, k, d, B, T, causal = a
        p = convplan.plan_conv(ci, co, k, 1, d, B, T, T + (k - 1) * d)
    elif site == "ops.conv1d_bwd_data(strided)":
        co, ci, s, B, t_out = a
        p = convplan.plan_convtr(co, ci, s, B, t_out + 1, flat_train_cols=t_out + 1)
        p = p._replace(p8=p.p8 if p.layout == convplan.TR_FLAT else None)       # this site's per-clip launch takes no pre-pass
    elif site == "ops.conv_transpose1d_bwd":
        ci, co, s, B, T = a
        p = convplan.plan_conv(ci, co, 2 * s, s, 1, B, T * s, T, flat_train="zero")
        p = p._replace(p8=p.p8 if p.form == convplan.FLAT_STRIDED else None)    # this site's per-clip launch takes no pre-pass
    elif site == "layers.SConvTranspose1d.run":
        ci, co, s, B, T, causal, alpha, grad = a
        with torch.set_grad_enabled(grad):
            p = layers.SConvTranspose1d.plan(_stub(w=_stub(c_in=ci, c_out=co), stride=s, causal=causal), B, T, alpha)
    elif site == "autograd._ConvTr.forward":
        ci, co, s, B, T, causal = a
        p = convplan.plan_convtr(ci, co, s, B, T, causal=causal, flat_train_cols=T + 1)
    elif site == "autograd_disc.PlainConv.forward":
        co, ci, k, k1, s, B, t_in, t_out = a[:8]
        p = autograd_disc._plan(co, ci, k, s, B, t_in, t_out, k1)
    elif site == "autograd_disc.PlainConv.backward(stride-1 conv)":
        co, ci, k, k1, B, tu, tp = a[:7]
        p = autograd_disc._plan(ci, co, k, 1, B, tu, tp, k1)
    elif site == "autograd_disc.PlainConv.backward(transposed)":
        co, ci, s, B, T = a
        p = convplan.plan_convtr(co, ci, s, B, T)
    else:
        p = convplan.plan_gemm(*a)
    return list(p)


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
SPLIT_ONLY = ("split_taps", "split_gemm", "split_gemm_strided", "split2", "rows_split", "flat_rows_split")


def _variant(layout, B, c_in, t_in, c_out, t_out, k, stride=1, dil=1, pad_left=0, k1=0, dil2=0, res=False, alpha_out=False, y2=False,
             row_phases=0, c_out_pad=None):
    d = _lib.ConvDesc()
    fake = ctypes.c_void_p(0x10000)          # never dereferenced: fac_conv1d_variant only reads the descriptor
    d.x, d.y, d.bias = fake, fake, fake
    d.w = None if layout in SPLIT_ONLY else fake           # split-only launch: the plan packed no fp32 weights
    d.w_split = fake if layout in SPLIT_ONLY else None
    d.res = fake if res else None
    d.alpha_out = fake if alpha_out else None
    d.y2 = d.alpha_y2 = fake if y2 else None
    d.ws, d.ws_bytes = fake, ops.CONV_WS_BYTES
    d.x_bs, d.x_cs, d.y_bs, d.y_cs = c_in * t_in, t_in, c_out * t_out * max(1, row_phases), t_out * max(1, row_phases)
    d.B, d.C_in, d.T_in, d.C_out, d.C_out_pad, d.T_out = B, c_in, t_in, c_out, c_out_pad or ops.pad32(c_out), t_out
    d.K, d.stride, d.dilation, d.pad_left, d.pad_mode = k, stride, dil, pad_left, ops.PAD_ZERO
    d.n_phase, d.y_tstride, d.phase_shift, d.act, d.w_batched, d.w_bs = 1, 1, 0, 0, 0, 0
    d.K1, d.dilation2, d.row_phases = k1, dil2, row_phases
    if row_phases:                           # ops.conv_transpose1d
        d.pw_split = 1 if (ops.BF16_SPLIT and ops.PW_SPLIT and ops.PW_TAPS and layout not in SPLIT_ONLY and row_phases == 2) else 0
    else:                                    # ops.conv1d
        d.pw_split = 1 if (ops.BF16_SPLIT and ops.PW_SPLIT and (k == 1 or (ops.PW_TAPS and k == 4 and stride == 2))) else 0
    return ops.conv_variant(d)


def _conv_desc(p, co, ci, k, s, d, B, T, causal=True, **kw):
    """An SConv1d launch as the site makes it: per clip with the layer's left padding, or (causal) flattened without padding."""
    P = (k - 1) * d + 1 - s
    if p[1] == "per_clip":
        return _variant(p[0], B, ci, T, co, -(-T // s), k, s, d, pad_left=P if causal else P - P // 2, **kw)
    pitch, n = (T + P) // s, T // s
    return _variant(p[0], 1, ci, B * (T + P), co, B * pitch - (pitch - n), k, s, d, **kw)


def _convtr_desc(layout, ci, co, s, B, T):
    rows = -(-co // (128 // s)) * 128        # ops.convtr_rows_pad
    return _variant(layout, B, ci, T, co, T, 2, pad_left=1, row_phases=s, c_out_pad=rows)


def test_cpp_planner_picks_the_family_the_python_plan_packed_for(rows):
    """The docstring claims "mirrors conv_gsplit_ok" etc. as a check: for every table row whose plan names a split / streaming-taps
    layout, fac_conv1d_variant on the descriptor the site launches names that kernel family."""
    checked, bad = 0, []
    for site, a in rows:
        p = plan(site, a)
        if p[0] not in FAMILY:
            continue
        if site == "layers.SConv1d.run":
            co, ci, k, s, d, B, T, _, plain, res, _, _ = a
            got = _conv_desc(p, co, ci, k, s, d, B, T, causal=a[10], res=res, alpha_out=not plain and not res, y2=True)
        elif site == "autograd._Conv.forward":
            got = _conv_desc(p, *a[:7], causal=a[8])
        elif site == "quantize._PlainConv.run":
            co, ci, k, B, T = a
            got = _variant(p[0], B, ci, T, co, T, k, pad_left=(k - 1) // 2)
        elif site == "autograd._ResUnit.forward":
            co, ci, k, d, B, T = a
            got = _conv_desc(p, co, ci, k, 1, d, B, T, res=k == 1, y2=True)
        elif site == "ops.conv1d_bwd_data(stride 1)":
            co, ci, k, d, B, T, _ = a
            got = _variant(p[0], B, co, T, ci, T + (k - 1) * d, k, 1, d, pad_left=(k - 1) * d)
        elif site == "ops.conv_transpose1d_bwd":
            ci, co, s, B, T = a
            if p[1] == "per_clip":
                got = _variant(p[0], B, co, T * s, ci, T, 2 * s, s)
            else:
                got = _variant(p[0], 1, co, B * (T + 1) * s, ci, B * (T + 1) - 1, 2 * s, s)
        elif site == "autograd_disc.PlainConv.forward":
            co, ci, k, k1, s, B, t_in, t_out, pad, dil2 = a
            got = _variant(p[0], B, ci, t_in, co, t_out, k, s, pad_left=pad, k1=k1, dil2=dil2)
        elif site == "autograd_disc.PlainConv.backward(stride-1 conv)":
            co, ci, k, k1, B, tu, tp, shift, dil2 = a
            got = _variant(p[0], B, co, tu, ci, tp, k, pad_left=shift, k1=k1, dil2=dil2)
        elif site in ("layers.SConvTranspose1d.run", "autograd._ConvTr.forward"):
            ci, co, s, B, T = a[:5]
            got = _convtr_desc(p[0], ci, co, s, B, T) if p[0] != "flat_rows_split" else _convtr_desc(p[0], ci, co, s, 1, B * (T + 1))
        elif site in ("ops.conv1d_bwd_data(strided)", "autograd_disc.PlainConv.backward(transposed)"):
            co, ci, s, B, T1 = a[0], a[1], a[2], a[3], a[4] + (1 if site.startswith("ops") else 0)
            got = _convtr_desc(p[0], co, ci, s, B, T1) if p[0] != "flat_rows_split" else _convtr_desc(p[0], co, ci, s, 1, B * T1)
        else:                                # plan_gemm: one signal of `cols` columns
            co, ci, cols = a
            got = _variant(p[0], 1, ci, cols, co, cols, 1)
        checked += 1
        if got[0] != FAMILY[p[0]]:
            bad.append((site, a, p, got))
    assert checked > 40 and not bad, bad[:5]


def test_data_gradient_plan_is_the_forward_plan_with_channels_swapped():
    """ops.conv1d_bwd_data asks plan_conv(c_in, c_out, ...): equal to the training forward's plan of the swapped conv, and the
    split-taps channel floor moves with the roles (C_out >= 64 and C_in > 32 for the gradient of a k = 3 / 5 conv)."""
    for co in (16, 32, 48, 64, 256, 384, 1024):
        for ci in (16, 32, 48, 64, 256, 384, 1024):
            for k in (1, 3, 5, 7):
                for B, T in ((1, 640), (1, 641), (16, 4800), (32, 160)):
                    tp = T + (k - 1)
                    grad = convplan.plan_conv(ci, co, k, 1, 1, B, T, tp)              # the call of ops.conv1d_bwd_data
                    fwd = convplan.plan_conv(c_out=ci, c_in=co, k=k, stride=1, dilation=1, batch=B, t_in=T, t_out=tp)
                    assert grad == fwd
                    if k in (3, 5) and grad.layout == convplan.W_TAPS:
                        assert co >= 64 and ci > 32
    assert convplan.plan_conv(48, 64, 5, 1, 1, 16, 4800, 4804).layout == convplan.W_TAPS       # gradient of a 48 -> 64 conv: floor met
    assert convplan.plan_conv(64, 48, 5, 1, 1, 16, 4800, 4804).layout == convplan.W_FP32       # gradient of a 64 -> 48 conv: not met
