"""Autograd Functions of the discriminator path (dac/model/discriminator.py; train.py:280-312) over the HIP C ABI."""
import ctypes as C

import torch
from torch.autograd import Function

from . import _lib, ops


def _call(name, *args):
    _lib.check(getattr(_lib.load(), name)(*args, ops._stream()), name)


_p = ops._ptr


def _plan(c_out, c_in, k, stride, batch, t_in, t_out, k1):
    """The discriminators' conv rule: k = 5 / 7 split taps without a channel floor, split2 stacks, no 1x1 GEMM, no streaming taps."""
    return ops.plan_conv(c_out, c_in, k, stride, 1, batch, t_in, t_out, k1=k1, split_k=(5, 7), floor_k=(), pw_taps=False,
                         split2=True)


def tap_span(k, k1=0, dil2=0):
    """Largest tap offset of a conv with k taps (PlainConv's `taps`: k1 per level, the levels dil2 apart; plain: k - 1)."""
    return (k // k1 - 1) * dil2 + (k1 - 1) if k1 else k - 1


def plan_bwd_transposed(c_out, c_in, stride, batch, t_ext):
    """PlainConv.backward, strided conv with at most two taps per output phase: the transposed conv over dy and its zero column
    (t_ext columns per clip)."""
    return ops.plan_convtr(c_out, c_in, stride, batch, t_ext)


def plan_bwd_stride1(c_out, c_in, k, k1, dil2, pad, batch, t_up, t_in):
    """PlainConv.backward's stride-1 flipped-weight conv over the (zero-inserted) gradient of t_up columns, from shapes alone:
    (plan, max_off, pl, tp, shift).  The conv is launched with its left padding max_off reduced by `pad` (pl) and exactly
    tp = t_in outputs; a padding larger than the taps' span (pl < 0, no layer of the model) keeps the full padding and is sliced."""
    max_off = tap_span(k, k1, dil2)
    pl = max_off - pad
    tp, shift = (t_in, pl) if pl >= 0 else (t_up + max_off, max_off)
    return _plan(c_in, c_out, k, 1, batch, t_up, tp, k1), max_off, pl, tp, shift      # the forward rule with the channels swapped


class PlainConv(Function):
    """torch-semantics Conv1d (zero padding `pad` both sides, stride) with optional weight-norm gain g (C_out,1,1).
    taps = (k1, dilation2): two-level taps -- tap k = k2 * k1 + k1' reads offset k2 * dilation2 + k1' (a (K2, k1) Conv2d over
    a row-concatenated signal of row pitch dilation2); `pad` is then the padding along the concatenated axis."""

    @staticmethod
    def forward(ctx, x, v, g, bias, k, stride, pad, taps=None):
        B, c_in, t_in = x.shape
        k1, dil2 = taps if taps is not None else (0, 0)
        t_out = (t_in + 2 * pad - tap_span(k, k1, dil2) - 1) // stride + 1
        vd, gd = v.detach().contiguous(), (g.detach().contiguous() if g is not None else None)
        sc = ops.wn_scale(vd, gd) if gd is not None else None           # once per forward, re-used by the backward
        # 32-channel (3, 9) / (3, 3) stacks: conv1d_bsplit2.hip; (5, 1) stride-3 convs: split GEMM over 3 phases; k = 5 / 7: split taps
        plan = _plan(v.shape[0], c_in, k, stride, B, t_in, t_out, k1)
        wp, ws = ops.pack_conv_for(plan.layout, vd, gd, stride, k1, scale=sc)
        ctx.scale = sc
        xin = ops.p8_prepass(x.detach(), plan.p8)       # (5, 1) stride-3 convs on the split GEMM kernel
        y = ops.conv1d(xin, wp, v.shape[0], k, bias=bias.detach() if bias is not None else None,
                       stride=stride, pad_left=pad, pad_mode=ops.PAD_ZERO, t_out=t_out, w_split=ws, k1=k1, dilation2=dil2)
        ctx.cfg = (k, stride, pad, t_in, t_out, k1, dil2)
        ctx.save_for_backward(x, v, g, bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, v, g, bias = ctx.saved_tensors
        k, stride, pad, t_in, t_out, k1, dil2 = ctx.cfg
        dy = dy.contiguous()
        B, c_out, _ = dy.shape
        c_in = v.shape[1]
        vd, gd = v.detach().contiguous(), (g.detach().contiguous() if g is not None else None)
        dx = None
        if ctx.needs_input_grad[0]:
            up = dy
            if stride > 1 and not k1 and k <= 2 * stride:
                # strided conv, at most two taps per output phase: dxpad[s u + r] = w[r] dy[u] + w[r + s] dy[u - 1] is the
                # polyphase transposed conv (no zero-inserted columns: 1.2x the useful flops for k = 5, s = 3 instead of 3x)
                v6 = torch.cat([vd, vd.new_zeros(c_out, c_in, 2 * stride - k)], dim=2) if k < 2 * stride else vd
                dy_ext = torch.cat([dy, dy.new_zeros(B, c_out, 1)], dim=2)
                tplan = plan_bwd_transposed(c_out, c_in, stride, B, dy_ext.shape[-1])
                wt = ops.pack_convtr_for(tplan.layout, v6, gd, stride)
                dy_ext = ops.p8_prepass(dy_ext, tplan.p8)
                with ops.flop_scale(k / (2.0 * stride)):      # the zero taps that pad k to 2 * stride are not algorithmic work
                    dxp = ops.conv_transpose1d(dy_ext, wt, c_in, stride)
                if dxp.shape[-1] < pad + t_in:
                    dxp = torch.cat([dxp, dxp.new_zeros(B, c_in, pad + t_in - dxp.shape[-1])], dim=2)
                dx = dxp[:, :, pad:pad + t_in].contiguous()
                up = None
            elif stride > 1:          # strided two-level conv: zero-insert, then the stride-1 flipped-weight conv
                tu = (t_out - 1) * stride + 1
                up = torch.empty(B, c_out, tu, device=dy.device)
                _call("fac_zero_insert", _p(dy), _p(up), B * c_out, t_out, stride)
            if up is not None:
                # dx[j] = dxpad[j + pad], dxpad[i] = sum_k wflip[k] up[i - max_off + off'_k]: the conv is launched with its left padding
                # reduced by `pad` and exactly t_in outputs (columns past `up` read zeros), so no padded tensor is sliced or extended
                plan, _, pl, tp, shift = plan_bwd_stride1(c_out, c_in, k, k1, dil2, pad, B, up.shape[-1], t_in)
                layout = plan.layout
                wp, ws = ((ops.pack_conv_weight_bwd(vd, gd, ctx.scale), None) if layout == ops.W_FP32
                          else ops.pack_conv_for(layout, ops.flipped_weight(vd, gd, ctx.scale), None, k1=k1))
                # zero-inserted columns (stride > 1) are not algorithmic work (the split-taps launch has always counted them)
                with ops.flop_scale(1.0 if layout == ops.W_TAPS else 1.0 / stride):
                    dxp = ops.conv1d(up, wp, c_in, k, pad_left=shift, pad_mode=ops.PAD_ZERO, t_out=tp, w_split=ws, k1=k1, dilation2=dil2)
                if pl >= 0:
                    dx = dxp
                else:
                    if tp < pad + t_in:       # trailing inputs no window reads
                        dxp = torch.cat([dxp, torch.zeros(B, c_in, pad + t_in - tp, device=dy.device)], dim=2)
                    dx = dxp[:, :, pad:pad + t_in].contiguous()
        dv = dg = db = None
        want_db = bias is not None and ctx.needs_input_grad[3]
        if ctx.needs_input_grad[1]:       # frozen discriminator (generator step): no weight gradients
            r = ops.conv1d_bwd_weight(x.detach(), dy, k, stride=stride, pad_mode=ops.PAD_ZERO, pad_left=pad, k1=k1, dilation2=dil2,
                                      want_db=want_db)
            dw, db = r if want_db else (r, None)
            if g is not None:
                dv, dg = ops.weight_norm_bwd(vd, gd, dw)
            else:
                dv = dw
        elif want_db:
            db = ops.bias_grad(dy)
        return dx, dv, dg, db, None, None, None, None


class LeakyReLU(Function):
    """LeakyReLU; with rows = (pitch, valid[, rows_per_group, valid_rows]) also zeroes the gap columns (and the separator rows)
    of a row-concatenated signal."""

    @staticmethod
    def forward(ctx, x, slope, rows=None):
        ctx.save_for_backward(x)
        pitch, valid, rpg, vrows = (tuple(rows) + (0, 0))[:4] if rows is not None else (0, 0, 0, 0)
        ctx.cfg = (slope, x.shape[-1], pitch, valid, rpg, vrows)
        y = torch.empty_like(x)
        _call("fac_leaky_relu", _p(x.detach().contiguous()), _p(None), _p(y), x.numel(), C.c_float(slope), x.shape[-1], pitch, valid,
              rpg, vrows)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        slope, T, pitch, valid, rpg, vrows = ctx.cfg
        dx = torch.empty_like(x)
        _call("fac_leaky_relu", _p(x.detach().contiguous()), _p(dy.contiguous()), _p(dx), x.numel(), C.c_float(slope), T, pitch, valid,
              rpg, vrows)
        return dx, None, None


class PeriodFold(Function):
    """(B, 1, T) -> (1, 1, B*period*pitch): MPD.pad_to_period + rearrange (discriminator.py:39-48) with the B*period
    rows laid one after another, `pitch` columns each (L data columns, then zeros standing in for the convs' padding)."""

    @staticmethod
    def forward(ctx, x, period, pitch):
        B, _, T = x.shape
        L = (T + (period - T % period)) // period
        out = torch.empty(1, 1, B * period * pitch, device=x.device)
        _call("fac_period_fold", _p(x.detach().contiguous()), _p(out), B, T, period, L, pitch, 0)
        ctx.cfg = (B, T, period, L, pitch)
        return out

    @staticmethod
    def backward(ctx, d):
        B, T, period, L, pitch = ctx.cfg
        dx = torch.empty(B, 1, T, device=d.device)
        _call("fac_period_fold", _p(d.contiguous()), _p(dx), B, T, period, L, pitch, 1)
        return dx, None, None


class RowStack3(Function):
    """(B*T, C, F) -> (B*T, 3C, F): the three time rows a (3, k) Conv2d reads, stacked into channels."""

    @staticmethod
    def forward(ctx, x, T):
        rows, c, f = x.shape
        out = torch.empty(rows, 3 * c, f, device=x.device)
        _call("fac_row_stack3", _p(x.detach().contiguous()), _p(out), rows, T, c, f, 0)
        ctx.cfg = (rows, T, c, f)
        return out

    @staticmethod
    def backward(ctx, d):
        rows, T, c, f = ctx.cfg
        dx = torch.empty(rows, c, f, device=d.device)
        _call("fac_row_stack3", _p(d.contiguous()), _p(dx), rows, T, c, f, 1)
        return dx, None


class Spectrogram(Function):
    """wave (B, T) -> complex STFT with audiotools' match_stride framing (discriminator.py:121-125,150-151) as
    (B, 2F, frames) = [re | im] rows: reflect pad, plain framing (the centre padding of torch.stft is exactly the two
    frames dropped at either end when hop = window / 4), windowed-DFT GEMM."""

    @staticmethod
    def forward(ctx, wave, scale):
        B, T = wave.shape
        L, hop = scale.win, scale.hop
        pad = (L - hop) // 2
        right = -(-T // hop) * hop - T
        T1 = T + 2 * pad + right
        xp = torch.empty(B, T1, device=wave.device)
        _call("fac_pad_reflect", _p(wave.detach().contiguous()), _p(xp), B, T, pad, pad + right)
        nf = T1 // hop + 1 - 4
        frames = ops.stft_frames(xp, L, nf, hop, 0, 0)
        spec = scale.dft(frames, nf)
        ctx.cfg = (scale, B, T, T1, pad, nf)
        return spec

    @staticmethod
    def backward(ctx, dspec):
        scale, B, T, T1, pad, nf = ctx.cfg
        dfr = scale.dft_adjoint(dspec.contiguous(), nf)
        dxp = ops.stft_frames_bwd(dfr, T1, scale.hop, 0, 0)
        dx = torch.empty(B, 1, T, device=dspec.device)
        _lib.check(_lib.load().fac_pad_fold_bwd(_p(dxp), _p(dx), B, 1, T, T1, pad, ops.PAD_REFLECT, ops._stream()), "fac_pad_fold_bwd")
        return dx.reshape(B, T), None


class SpecBand(Function):
    """One frequency band of the spectrogram as conv rows: (B, 2F, T) -> (B*T, 2, Fb)."""

    @staticmethod
    def forward(ctx, spec, f0, fb):
        B, f2, T = spec.shape
        out = torch.empty(B * T, 2, fb, device=spec.device)
        _call("fac_spec_to_rows", _p(spec.detach().contiguous()), _p(out), B, f2 // 2, T, f0, fb, 0)
        ctx.cfg = (B, f2 // 2, T, f0, fb)
        return out

    @staticmethod
    def backward(ctx, d):
        B, Ft, T, f0, fb = ctx.cfg
        dspec = torch.zeros(B, 2 * Ft, T, device=d.device)
        _call("fac_spec_to_rows", _p(d.contiguous()), _p(dspec), B, Ft, T, f0, fb, 1)
        return dspec, None, None


class SpecCat(Function):
    """One frequency band of the spectrogram in the row-concatenated layout: (B, 2F, T) -> (1, 2, B*(T+1)*pitch); row
    r = b*(T+1) + t holds the band's bins then zeros, row t = T of each clip is a zero separator."""

    @staticmethod
    def forward(ctx, spec, f0, fb, pitch):
        B, f2, T = spec.shape
        out = torch.empty(1, 2, B * (T + 1) * pitch, device=spec.device)
        _call("fac_spec_to_cat", _p(spec.detach().contiguous()), _p(out), B, f2 // 2, T, f0, fb, pitch, 0)
        ctx.cfg = (B, f2 // 2, T, f0, fb, pitch)
        return out

    @staticmethod
    def backward(ctx, d):
        B, Ft, T, f0, fb, pitch = ctx.cfg
        dspec = torch.zeros(B, 2 * Ft, T, device=d.device)
        _call("fac_spec_to_cat", _p(d.contiguous()), _p(dspec), B, Ft, T, f0, fb, pitch, 1)
        return dspec, None, None, None


class Preprocess(Function):
    """Discriminator.preprocess (discriminator.py:200-205)."""

    @staticmethod
    def forward(ctx, x):
        B, _, T = x.shape
        xd = x.detach().contiguous()
        z = torch.empty_like(xd)
        stats = torch.empty(B * 4, device=x.device)
        _call("fac_disc_preprocess", _p(xd), _p(None), _p(z), _p(stats), B, T)
        ctx.save_for_backward(xd, stats)
        return z

    @staticmethod
    def backward(ctx, dz):
        xd, stats = ctx.saved_tensors
        B, _, T = xd.shape
        dx = torch.empty_like(xd)
        _call("fac_disc_preprocess", _p(xd), _p(dz.contiguous()), _p(dx), _p(stats), B, T)
        return dx


class PairMean(Function):
    """mean over elements of |a - b| (mode 0), (a - b)^2 (mode 2) or smooth-L1 (mode 3); gradient to `a` only."""

    @staticmethod
    def forward(ctx, a, b, mode, count=None):
        """count: number of elements the mean runs over (default all; smaller when a and b carry zero gap columns)."""
        ad, bd = a.detach().contiguous(), b.detach().contiguous()
        out = torch.zeros(1, device=a.device)
        scratch = torch.empty(1024, device=a.device)
        ctx.inv = 1.0 / (count if count is not None else ad.numel())
        ops.reduce_pair(ad, bd, out, scratch, mode, 0.0, ctx.inv, False)
        ctx.save_for_backward(ad, bd)
        ctx.mode = mode
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        ad, bd = ctx.saved_tensors
        da = torch.empty_like(ad)
        ops.pair_bwd(ad, bd, da, ctx.mode, 0.0, ctx.inv, False)
        return ops.rows_fma(da.reshape(1, -1), g.reshape(1).to(da.dtype)).reshape(ad.shape), None, None, None


class CrossEntropy(Function):
    """F.cross_entropy(logits (N, C), labels (N)), mean reduction."""

    @staticmethod
    def forward(ctx, logits, labels):
        ld = logits.detach().contiguous()
        N, Cn = ld.shape
        loss = torch.zeros(1, device=ld.device)
        scratch = torch.empty(N, device=ld.device)
        _call("fac_cross_entropy", _p(ld), C.c_void_p(labels.data_ptr()), _p(loss), _p(None), _p(scratch), N, Cn, C.c_float(0.0))
        ctx.save_for_backward(ld, labels)
        return loss[0].clone()

    @staticmethod
    def backward(ctx, g):
        ld, labels = ctx.saved_tensors
        N, Cn = ld.shape
        dl = torch.empty_like(ld)
        scratch = torch.empty(N, device=ld.device)
        _call("fac_cross_entropy", _p(ld), C.c_void_p(labels.data_ptr()), _p(None), _p(dl), _p(scratch), N, Cn, C.c_float(1.0 / N))
        return ops.rows_fma(dl.reshape(1, -1), g.reshape(1).to(dl.dtype)).reshape(ld.shape), None


class Focal(Function):
    """FocalLoss on a mean cross entropy (losses.py:264-276; train.py:153 gamma = 2): (1 - exp(-ce))**gamma * ce."""

    @staticmethod
    def forward(ctx, ce, gamma):
        out = torch.empty(2, device=ce.device)
        _call("fac_focal_scalar", _p(ce.detach().reshape(1).contiguous()), _p(out), C.c_float(gamma))
        ctx.save_for_backward(out)
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        return ops.rows_fma(out[1:2].reshape(1, 1), g.reshape(1).to(out.dtype)).reshape(()), None


def focal_cross_entropy(logits, labels, gamma=2.0):
    """content_criterion of train.py:153,334-336."""
    return Focal.apply(CrossEntropy.apply(logits, labels), gamma)


class CropRows(Function):
    """dst[b, c, t] = src[b, c, start[b] * scale + t]: the random-crop batching of train.py:188-212 without host loops."""

    @staticmethod
    def forward(ctx, src, start, t_dst, scale):
        B, Cn, T = src.shape
        out = torch.empty(B, Cn, t_dst, device=src.device)
        _call("fac_crop_rows", _p(src.detach().contiguous()), _p(out), C.c_void_p(start.data_ptr()), B, Cn, T, t_dst, scale)
        return out

    @staticmethod
    def backward(ctx, d):
        raise NotImplementedError("crop_rows feeds constant inputs (waves / mel targets): no gradient path")
