"""Parameter-holding leaf modules with the reference's state-dict names, executing on the HIP
C ABI.  The module tree exists so that `state_dict()` / `load_state_dict()` / optimisers see exactly
the reference's parameter names and shapes; the arithmetic lives in
libfacodec_hip.so and is driven by the fused plans in dac_model.py / quantize.py.

Reference counterparts: dac/model/encodec.py (SConv1d :192-228, SConvTranspose1d :231-270,
SLSTM :272-288, NormConv1d :125-139), dac/nn/layers.py (Snake1d :27-33, WNConv1d :9-10).
"""
import math

import torch
from torch import nn

from . import ops


def _uniform_(t, bound):
    with torch.no_grad():
        return t.uniform_(-bound, bound)


class ConvWeights(nn.Module):
    """weight_g / weight_v / bias of an old-style weight-normed conv (or plain weight / bias), in
    torch's layout: Conv1d (C_out, C_in, K); ConvTranspose1d (C_in, C_out, K) with the norm taken
    over dim 0 = C_in.  `packed()` materialises w = g*v/||v|| straight into the MFMA kernel's layout
    (K6); like the reference it is recomputed on every forward unless `freeze_packed` is set."""

    def __init__(self, c_in, c_out, k, weight_norm=True, transposed=False, stride=1, bias=True):
        super().__init__()
        self.c_in, self.c_out, self.k = c_in, c_out, k
        self.transposed, self.stride, self.weight_norm = transposed, stride, weight_norm
        shape = (c_in, c_out, k) if transposed else (c_out, c_in, k)
        fan_in = (c_out if transposed else c_in) * k
        w = _uniform_(torch.empty(shape), 1.0 / math.sqrt(fan_in))
        if weight_norm:
            self.weight_g = nn.Parameter(w.reshape(shape[0], -1).norm(dim=1).reshape(shape[0], 1, 1))
            self.weight_v = nn.Parameter(w)
        else:
            self.weight = nn.Parameter(w)
        self.bias = nn.Parameter(_uniform_(torch.empty(c_out), 1.0 / math.sqrt(fan_in))) if bias else None
        self._packed = None
        self._split = None
        self._rows = None
        self._rows_split = None
        self.freeze_packed = False

    def _vg(self):
        return (self.weight_v.detach(), self.weight_g.detach()) if self.weight_norm else (self.weight.detach(), None)

    def _cached(self, slot, pack, *a, **kw):
        """The packed copy kept in `slot`: repacked into the same buffer on every call unless `freeze_packed`."""
        cur = getattr(self, slot)
        if cur is None or not self.freeze_packed:
            cur = pack(*self._vg(), *a, out=cur[0] if isinstance(cur, tuple) else cur, **kw)
            setattr(self, slot, cur)
        return cur

    def packed(self):
        if self.transposed:
            return self._cached("_packed", ops.pack_convtr_weight, self.stride)
        return self._cached("_packed", ops.pack_conv_weight)

    def packed_rows(self):
        """ConvTranspose1d weights for the all-phases launch (ops.pack_convtr_weight_rows)."""
        return self._cached("_rows", ops.pack_convtr_weight_rows, self.stride)

    def packed_rows_split(self):
        """ConvTranspose1d weights for the all-phases launch on the split-bf16 GEMM kernel: (buffer, rows)."""
        return self._cached("_rows_split", ops.pack_convtr_weight_rows_split, self.stride)

    def packed_split_strided(self, stride):
        """Split GEMM weights of a strided conv (stride < k <= 2 * stride), ops.pack_gemm_weight_split(in_stride=stride)."""
        return self._cached("_split", ops.pack_gemm_weight_split, in_stride=stride)

    def packed_split(self, rows=64):
        """The same weights as three exact bf16 planes (ops.pack_conv_weight_split) for the k = 7 convs, in co tiles of `rows`."""
        return self._cached("_split", ops.pack_conv_weight_split, rows=rows)

    def _apply(self, fn, *a, **kw):
        self._packed = None  # device / dtype moves invalidate the packed copies
        self._split = None
        self._rows = None
        self._rows_split = None
        return super()._apply(fn, *a, **kw)


class _Norm(nn.Module):
    """Mirrors the NormConv1d / NormConvTranspose1d naming level (`.conv` / `.convtr`)."""

    def __init__(self, name, weights):
        super().__init__()
        setattr(self, name, weights)


# Short clips through the split GEMM kernel as one flattened signal (ops.conv1d_flat / conv_transpose1d_flat): inference only.
FLAT_SHORT_CLIPS = True
FLAT_STRIDE1 = True      # wide stride-1 k = 7 convs on short clips too


def write_edge(conv, x, edge):
    """edge = (lens (B,) int32 frames on the device, columns per frame of x) or None: where `conv` looks to the right
    (conv.edge_rule()), its padding is written behind every clip of x, in place (ops.edge_tail_)."""
    rule = conv.edge_rule() if edge is not None else None
    if rule is not None:
        ops.edge_tail_(x, edge[0], edge[1], rule[0], rule[1])


class SConv1d(nn.Module):
    """Causal / asymmetric-padded Conv1d (dac/model/encodec.py:192-228).  State-dict keys:
    conv.conv.{weight_g,weight_v,bias} (norm='weight_norm') or conv.conv.{weight,bias}."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, dilation=1, causal=False,
                 norm="none", pad_mode="reflect", bias=True):
        super().__init__()
        self.conv = _Norm("conv", ConvWeights(in_channels, out_channels, kernel_size, norm == "weight_norm", bias=bias))
        self.kernel_size, self.stride, self.dilation = kernel_size, stride, dilation
        self.causal = causal
        self.pad_mode = ops.PAD_REFLECT if pad_mode == "reflect" else ops.PAD_ZERO

    @property
    def w(self):
        return self.conv.conv

    def plan(self, B, T, alpha_in=False, plain=True, res=False):
        """The inference forward's variant of the conv rule (convplan.plan_conv) for B clips of T columns."""
        return ops.plan_conv(self.w.c_out, self.w.c_in, self.kernel_size, self.stride, self.dilation, B, T, -(-T // self.stride),
                             alpha_in=alpha_in, plain=plain, res=res, causal_reflect=self.causal and self.pad_mode == ops.PAD_REFLECT,
                             grad=torch.is_grad_enabled(), c_out_mult16=False, tail="always", flat_infer=FLAT_SHORT_CLIPS,
                             flat_stride1=FLAT_STRIDE1)

    def edge_rule(self):
        """What this conv reads behind the last column of a clip it sees alone: (columns, pad mode), or None when it does not look
        to the right (causal, or a non-causal 1x1).  A non-causal strided conv has an extra right padding that depends on the
        length (dac/model/encodec.py:71-78): no rule, NotImplementedError."""
        if self.causal:
            return None
        if self.stride != 1:
            raise NotImplementedError(f"a non-causal strided SConv1d (k = {self.kernel_size}, stride {self.stride}) pads its right "
                                      "side by an amount that depends on the clip's length: no per-clip edge rule")
        n = ((self.kernel_size - 1) * self.dilation) // 2
        return (n, self.pad_mode) if n > 0 else None

    def run(self, x, alpha_in=None, alpha_out=None, res=None, act=ops.ACT_NONE, alpha_y2=None, want_y=True, edge=None):
        """alpha_y2: additionally emit snake(y, alpha_y2) for the next Snake->conv (returns (y, y2)).
        edge = (lens (B,) int32 frames on the device, columns per frame): a right-padded batch of clips -- the
        columns behind every clip's own end are first overwritten IN PLACE with this conv's padding (ops.edge_tail_), then the
        unchanged launch follows."""
        w, k, s_ = self.w, self.kernel_size, self.stride
        write_edge(self, x, edge)
        B, _, T = x.shape       # (x is an fp32 tensor: no caller hands a P8 to a module, so the old chains' isinstance guards are gone)
        plan = self.plan(B, T, alpha_in is not None, alpha_out is None and res is None and act == ops.ACT_NONE, res is not None)
        split = (w.packed_split_strided(s_) if plan.layout == ops.W_GEMM_STRIDED
                 else w.packed_split(ops.tile_rows(w.c_out, w.c_in, k)) if plan.layout == ops.W_TAPS
                 else w.packed_split() if plan.layout == ops.W_GEMM else None)
        if plan.form != ops.PER_CLIP:
            # every clip reflect-padded on the left (the causal padding of dac/model/encodec.py:212-222, materialised: data movement
            # only; strided: T % s == 0, so there is no right padding) and all of them laid out as ONE signal
            P = (k - 1) * self.dilation + 1 - s_
            return ops.conv1d_flat(torch.nn.functional.pad(x, (P, 0), mode="reflect"), split, w.c_out, k, s_, T // s_,
                                   dilation=self.dilation, bias=w.bias, p8=plan.p8, alpha_out=alpha_out, act=act, alpha_y2=alpha_y2,
                                   want_y=want_y)
        x = ops.p8_prepass(x, plan.p8)      # split GEMM over the phase sub-signals: P8 input where it pays
        return ops.conv1d(x, w.packed() if split is None else None, w.c_out, k, bias=w.bias,
                          stride=s_, dilation=self.dilation, pad_mode=self.pad_mode, alpha_in=alpha_in,
                          alpha_out=alpha_out, res=res, act=act, causal=self.causal, alpha_y2=alpha_y2, want_y=want_y,
                          w_split=split)

    def forward(self, x):
        return self.run(x)


class SConvTranspose1d(nn.Module):
    """Causal ConvTranspose1d with right trim (dac/model/encodec.py:231-270).  Keys:
    convtr.convtr.{weight_g (C_in,1,1), weight_v (C_in,C_out,K), bias}."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, causal=False, norm="none"):
        super().__init__()
        self.convtr = _Norm("convtr", ConvWeights(in_channels, out_channels, kernel_size, norm == "weight_norm",
                                                  transposed=True, stride=stride))
        self.stride = stride
        self.causal = causal

    @property
    def w(self):
        return self.convtr.convtr

    def plan(self, B, T, alpha_in=False):
        return ops.plan_convtr(self.w.c_in, self.w.c_out, self.stride, B, T, causal=self.causal, alpha_in=alpha_in,
                               grad=torch.is_grad_enabled(), flat_infer=FLAT_SHORT_CLIPS)

    def edge_rule(self):
        """Non-causal (trimmed on both sides): the last ceil(stride / 2) outputs of a clip also take the column behind its end, which
        is no signal -- (1, PAD_ZERO).  Causal: None."""
        return None if self.causal else (1, ops.PAD_ZERO)

    def run(self, x, alpha_in=None, alpha_y2=None, edge=None):
        """edge = (lens, columns per frame of x): see SConv1d.run; the column behind every clip is zeroed in place first."""
        w = self.w
        write_edge(self, x, edge)
        B, c_in, T = x.shape
        plan = self.plan(B, T, alpha_in is not None)
        if plan.layout == ops.TR_FLAT:
            # short clips: ONE signal of B (T + 1) columns with a zero column in front of every clip (the x[t - 1] of its first frame)
            xz = torch.cat([torch.zeros(B, c_in, 1, device=x.device, dtype=x.dtype), x], -1)
            return ops.conv_transpose1d_flat(xz, w.packed_rows_split(), w.c_out, self.stride, trim=self.stride, bias=w.bias,
                                             alpha_y2=alpha_y2, p8=plan.p8)
        wp = (w.packed_rows_split() if plan.layout == ops.TR_ROWS_SPLIT
              else w.packed() if plan.layout == ops.TR_POLYPHASE else w.packed_rows())
        return ops.conv_transpose1d(ops.p8_prepass(x, plan.p8), wp, w.c_out, self.stride, bias=w.bias, alpha_in=alpha_in,
                                    alpha_y2=alpha_y2, causal=self.causal)

    def forward(self, x):
        return self.run(x)


class Snake1d(nn.Module):
    """alpha (1, C, 1) of dac/nn/layers.py:27-33.  Normally fused into the neighbouring conv."""

    def __init__(self, channels):
        super().__init__()
        self.alpha = nn.Parameter(torch.ones(1, channels, 1))

    def flat(self):
        return self.alpha.detach().reshape(-1)

    def forward(self, x):
        return ops.snake(x, self.flat())


class _LSTMParams(nn.Module):
    """nn.LSTM's parameter names/shapes (weight_ih_l{k} (4H,H), weight_hh_l{k}, bias_ih_l{k}, bias_hh_l{k})."""

    def __init__(self, hidden, num_layers):
        super().__init__()
        b = 1.0 / math.sqrt(hidden)
        for l in range(num_layers):
            for n, shp in (("weight_ih", (4 * hidden, hidden)), ("weight_hh", (4 * hidden, hidden)),
                           ("bias_ih", (4 * hidden,)), ("bias_hh", (4 * hidden,))):
                setattr(self, f"{n}_l{l}", nn.Parameter(_uniform_(torch.empty(shp), b)))


class SLSTM(nn.Module):
    """dac/model/encodec.py:272-288: multi-layer LSTM over time on (B, C, T) plus skip.
    Input projections run as ONE GEMM per layer on the MFMA conv kernel over the channel-major
    (H, T*BP) work buffer; the recurrence is one resident launch per layer (fac_lstm_layer_fwd_persist) where it
    applies, else fac_lstm_layer_fwd (one launch per step)."""

    def __init__(self, dimension, num_layers=2, skip=True):
        super().__init__()
        self.lstm = _LSTMParams(dimension, num_layers)
        self.dimension, self.num_layers, self.skip = dimension, num_layers, skip

    def forward(self, x, alpha_out=None):
        """alpha_out: Snake alpha applied to the (skip-added) output by the transpose-back kernel, for
        the Snake that follows the LSTM in the Encoder / precedes the first DecoderBlock's ConvTranspose."""
        B, H, T = x.shape
        inp = ops.lstm_to_time_major(x)
        for l in range(self.num_layers):
            p = self.lstm
            w_raw = getattr(p, f"weight_ih_l{l}").detach()
            bias = ops.add(getattr(p, f"bias_ih_l{l}").detach(), getattr(p, f"bias_hh_l{l}").detach())
            w_hh = getattr(p, f"weight_hh_l{l}").detach()
            persist = ops.lstm_persist_ok(H, B)
            T_, BP = inp.shape[1], inp.shape[2]
            with ops.flop_scale(B / BP):
                pre = ops.lstm_input_proj(inp, w_raw, bias)
                if ops.lstm_persist_split_ok(H, B, T_):      # 17 .. 32 columns: resident, W_hh . h on the bf16 matrix pipe
                    inp = ops.lstm_layer_persist_split(pre, w_hh, H, B)
                elif persist:     # whole layer in one launch, W_hh resident in registers (lstm_persist.hip)
                    inp = ops.lstm_layer_persist(pre, w_hh, H, B)
                else:
                    inp = ops.lstm_layer(pre, ops.pack_lstm_whh(w_hh), H)
        return ops.lstm_from_time_major(inp, x if self.skip else None, B, alpha_out)
