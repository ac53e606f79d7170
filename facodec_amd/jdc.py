"""The reference's F0 extractor on the HIP path: JDCNet (modules/JDC/model.py; built by modules/commons.py:183-191 as
JDCNet(num_class=1, seq_len=192) and called by train.py:216 on the cropped log-mel segment).

State-dict keys, shapes and dtypes equal the reference class's (77 entries: BatchNorm running statistics and
`num_batches_tracked` included, both BiLSTMs with their `_reverse` tensors, the detector branch), so `load_state_dict(strict=True)`
of a checkpoint's `['net']` works.  The detector branch (`detector_conv`, `bilstm_detector`, `detector`) is held and never run,
as in the reference's `forward`.

EVAL ARITHMETIC ONLY.  The reference leaves the frozen extractor in `.train()` (modules/commons.py:189): BatchNorm then
normalises with the statistics of the batch at hand and `Dropout(0.2)` is live -- an accident of the training script that depends on
its RNG stream and cannot (and should not) be reproduced.  This module always computes what `model.eval()` computes: BatchNorm on
its running statistics, no dropout.  `.train()` changes nothing, and there is no backward (the extractor is frozen).

Execution.  x (B, 1, 80, T) is transposed into the row-concatenated layout of the spectrogram discriminator (discriminator.MRD) at
stride 1: every channel is ONE signal (1, C, B * (T + 1) * P_i); row r = b * (T + 1) + t holds the W_i valid frequency bins of frame t
followed by zeros up to the row pitch P_i, row t = T of every clip is all zero (`stage_geometry`).  Every 3 x 3 Conv2d is then one
two-level-tap 1-D conv (ops.conv1d, k = 9, k1 = 3, dilation2 = P_i, pad_left = P_i + 1) whose padding along frequency and time
is those zeros; a BatchNorm that follows a bias-free conv is folded into its weights and a bias when the weights are loaded; each
ResBlock's 1 x 1 shortcut is a k = 1 conv that the block's second 3 x 3 takes as `res`.  BatchNorm -> LeakyReLU -> MaxPool in
front of a block is one kernel (ops.jdc_affine_lrelu_pool) that also restores the zeros.  The BiLSTM is two chains on two streams
(ops.run_chains): the time-major gather (flipped for the backward direction), the (1024, 512) input projection as a 1 x 1 conv over
the T * pad32(B) columns, and the per-step LSTM kernel (H = 256 is none of the resident kernels' sizes); the 512 -> 1 Linear, the
abs and the gather out of time-major are one small kernel (ops.jdc_head).

Out of scope: clips of different lengths (the backward direction would read the padded tail), streaming, num_class != 1."""
import torch
from torch import nn

from . import _lib, ops

N_STREAMS = 2      # the two LSTM directions side by side


def stage_geometry(n_bins=80):
    """(widths W_0..W_4, pitches P_0..P_4, pools) of the five stages for an input of n_bins frequency bins: the convs of
    conv_block read stage 0, those of res_block i stage i, stage 4 is the pooled LSTM input.  W halves at the three ResBlocks and is
    divided by 4 (floor) at pool_block; P_{i+1} * pool_i == P_i, and P_i >= W_i + 1 wherever a 3 x 3 conv reads the stage (one zero
    column between the rows is the convs' padding along frequency).  80 bins: W = 80, 40, 20, 10, 2 and P = 96, 48, 24, 12, 3."""
    pools = (2, 2, 2, 4)
    W = [int(n_bins)]
    for p in pools:
        W.append(W[-1] // p)
    if W[-1] < 1:
        raise ValueError(f"JDCNet needs at least {2 * 2 * 2 * 4} frequency bins, got {n_bins}")
    down = [1, 2, 4, 8, 32]                                   # P_0 / P_i
    p4 = max([W[4]] + [-(-(W[i] + 1) * down[i] // 32) for i in range(4)])
    return tuple(W), tuple(p4 * 32 // d for d in down), pools


def bn_scale_shift(weight, bias, running_mean, running_var, eps):
    """Eval-mode BatchNorm as y = scale * x + shift: scale = gamma / sqrt(var + eps), shift = beta - mean * scale, computed on the
    host in float64 and rounded once to float32."""
    g, b, m, v = (t.detach().to("cpu", torch.float64) for t in (weight, bias, running_mean, running_var))
    scale = g / torch.sqrt(v + eps)
    return scale.float(), (b - m * scale).float()


def fold_bn(conv_weight, bn):
    """A bias-free conv followed by eval BatchNorm `bn` = one conv with weights scale[co] * w[co] and bias shift[co] (float64 on
    the host, rounded once).  Returns (weights (C_out, C_in, kh * kw) float32, bias (C_out,) float32) on the CPU."""
    g, b, m, v = (t.detach().to("cpu", torch.float64) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
    scale = g / torch.sqrt(v + bn.eps)
    w = conv_weight.detach().to("cpu", torch.float64)
    return (w * scale.view(-1, 1, 1, 1)).flatten(2).float(), (b - m * scale).float()


def _block(c_in, c_out, slope):
    """The parameter holders of one ResBlock (model.py:158-190) under the reference's names; indices without parameters are
    placeholders.  Nothing here is ever called: JDCNet runs the HIP path on the tensors."""
    m = nn.Module()
    m.pre_conv = nn.Sequential(nn.BatchNorm2d(c_in), nn.Identity(), nn.Identity())
    m.conv = nn.Sequential(nn.Conv2d(c_in, c_out, 3, padding=1, bias=False), nn.BatchNorm2d(c_out), nn.Identity(),
                           nn.Conv2d(c_out, c_out, 3, padding=1, bias=False))
    if c_in != c_out:
        m.conv1by1 = nn.Conv2d(c_in, c_out, 1, bias=False)
    else:
        m.conv1by1 = None
    return m


class JDCNet(nn.Module):
    """See the module docstring.  forward(x (B, 1, 80, T)) -> (F0 (B, T), GAN_feature (B, 256, 10, T), poolblock_out (B, 256, T, 2))."""

    def __init__(self, num_class=722, seq_len=31, leaky_relu_slope=0.01):
        super().__init__()
        self.num_class, self.seq_len, self.slope = num_class, seq_len, float(leaky_relu_slope)
        self.conv_block = nn.Sequential(nn.Conv2d(1, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64), nn.Identity(),
                                        nn.Conv2d(64, 64, 3, padding=1, bias=False))
        self.res_block1 = _block(64, 128, self.slope)
        self.res_block2 = _block(128, 192, self.slope)
        self.res_block3 = _block(192, 256, self.slope)
        self.pool_block = nn.Sequential(nn.BatchNorm2d(256), nn.Identity(), nn.Identity(), nn.Identity())
        self.detector_conv = nn.Sequential(nn.Conv2d(640, 256, 1, bias=False), nn.BatchNorm2d(256), nn.Identity(), nn.Identity())
        self.bilstm_classifier = nn.LSTM(input_size=512, hidden_size=256, batch_first=True, bidirectional=True)
        self.bilstm_detector = nn.LSTM(input_size=512, hidden_size=256, batch_first=True, bidirectional=True)
        self.classifier = nn.Linear(512, num_class)
        self.detector = nn.Linear(512, 2)
        for p in self.parameters():
            p.requires_grad_(False)
        self._prep = None

    # ------------------------------------------------------------------------------------------ derived weights
    def _apply(self, fn, *a, **kw):
        self._prep = None
        return super()._apply(fn, *a, **kw)

    def load_state_dict(self, *a, **kw):
        self._prep = None
        return super().load_state_dict(*a, **kw)

    def _prepare(self, dev):
        """Folded / packed weights and BatchNorm scale / shift on `dev`, once per load_state_dict / .to()."""
        if self._prep is not None and self._prep["dev"] == dev:
            return self._prep
        up = lambda t: t.to(dev).contiguous()        # noqa: E731
        pack = lambda w: ops.pack_conv_weight(up(w))   # noqa: E731  (C_out, C_in, K) -> the fp32 pack
        p = dict(dev=dev)
        w, b = fold_bn(self.conv_block[0].weight, self.conv_block[1])
        p["cb0"] = (pack(w), up(b))
        p["cb3"] = pack(self.conv_block[3].weight.detach().flatten(2))
        for i, blk in enumerate((self.res_block1, self.res_block2, self.res_block3), 1):
            sc, sh = bn_scale_shift(blk.pre_conv[0].weight, blk.pre_conv[0].bias, blk.pre_conv[0].running_mean,
                                    blk.pre_conv[0].running_var, blk.pre_conv[0].eps)
            w, b = fold_bn(blk.conv[0].weight, blk.conv[1])
            p[f"rb{i}"] = dict(pre=(up(sc), up(sh)), c0=(pack(w), up(b)), c3=pack(blk.conv[3].weight.detach().flatten(2)),
                               sc=pack(blk.conv1by1.weight.detach().flatten(2)) if blk.conv1by1 is not None else None,
                               c_out=blk.conv[0].weight.shape[0])
        bn = self.pool_block[0]
        sc, sh = bn_scale_shift(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
        p["pool"] = (up(sc), up(sh))
        lstm = self.bilstm_classifier
        for d, suf in (("fwd", ""), ("bwd", "_reverse")):
            w_ih = up(getattr(lstm, "weight_ih_l0" + suf).detach())
            bias = (getattr(lstm, "bias_ih_l0" + suf).detach().cpu() + getattr(lstm, "bias_hh_l0" + suf).detach().cpu())
            p[d] = dict(w_ih=w_ih, w_ih_fp32=ops.pack_conv_weight(w_ih), w_ih_split=None, bias=up(bias),
                        w_hh=ops.pack_lstm_whh(up(getattr(lstm, "weight_hh_l0" + suf).detach())))
        p["head"] = (up(self.classifier.weight.detach().reshape(-1)), up(self.classifier.bias.detach()))
        self._prep = p
        return p

    # ------------------------------------------------------------------------------------------ the stages
    @staticmethod
    def _conv3(x, wp, c_out, pitch, bias=None, res=None):
        """3 x 3 Conv2d, padding 1, over the row-concatenated signal."""
        return ops.conv1d(x, wp, c_out, 9, bias=bias, pad_left=pitch + 1, pad_mode=ops.PAD_ZERO, t_out=x.shape[-1], k1=3,
                          dilation2=pitch, res=res)

    def _features(self, x):
        """x (B, 1, n_bins, T) -> (stage-3 signal after pool_block[0..1], (B, T, W_3, P_3))."""
        if not (torch.is_tensor(x) and x.is_cuda):
            raise _lib.FacodecHipError(f"JDCNet input must live on the GPU (got {getattr(x, 'device', type(x))}); there is no CPU path")
        if x.dim() != 4 or x.shape[1] != 1:
            raise ValueError(f"JDCNet takes (B, 1, n_bins, T), got {tuple(x.shape)}")
        B, _, n_bins, T = x.shape
        W, P, pools = stage_geometry(n_bins)
        p = self._prepare(x.device)
        rows, rpg = B * (T + 1), T + 1
        lrelu = lambda h, i: ops.leaky_relu_rows(h, self.slope, P[i], W[i], rpg, T)      # noqa: E731
        with ops.flop_scale(W[0] * T / float(P[0] * rpg)):          # gap columns and separator rows are not algorithmic work
            h = ops.jdc_layout_in(x, P[0])
            h = lrelu(self._conv3(h, p["cb0"][0], 64, P[0], bias=p["cb0"][1]), 0)
            h = self._conv3(h, p["cb3"], 64, P[0])
        for i in (1, 2, 3):
            q = p[f"rb{i}"]
            h = ops.jdc_affine_lrelu_pool(h, q["pre"][0], q["pre"][1], rows, rpg, W[i - 1], P[i - 1], pools[i - 1], self.slope)
            with ops.flop_scale(W[i] * T / float(P[i] * rpg)):
                c = lrelu(self._conv3(h, q["c0"][0], q["c_out"], P[i], bias=q["c0"][1]), i)
                short = h if q["sc"] is None else ops.conv1d(h, q["sc"], q["c_out"], 1, pad_left=0, pad_mode=ops.PAD_ZERO,
                                                              t_out=h.shape[-1])
                h = self._conv3(c, q["c3"], q["c_out"], P[i], res=short)
        h = ops.jdc_affine_lrelu_pool(h, p["pool"][0], p["pool"][1], rows, rpg, W[3], P[3], 1, self.slope)
        return h, (B, T, W, P, pools)

    def _pooled(self, s3, geo):
        B, T, W, P, pools = geo
        return ops.jdc_affine_lrelu_pool(s3, None, None, B * (T + 1), T + 1, W[3], P[3], pools[3], 1.0)     # MaxPool2d((1, 4)) alone

    def _direction(self, s4, geo, q, reverse):
        """One LSTM direction over the stage-4 signal -> its outputs (256, T, BP) time-major (on flipped time if reverse)."""
        B, T, W, P, _ = geo
        inp = ops.jdc_to_time_major(s4, B, T, W[4], P[4], reverse)
        F, _, BP = inp.shape
        H = q["w_ih"].shape[0] // 4
        plan = ops.plan_gemm(4 * H, F, T * BP)
        if plan.layout == ops.W_GEMM and q["w_ih_split"] is None:
            q["w_ih_split"] = ops.pack_gemm_weight_split(q["w_ih"])
        with ops.flop_scale(B / BP):
            sig = ops.p8_prepass(inp.view(1, F, T * BP), plan.p8)
            pre = ops.conv1d(sig, q["w_ih_fp32"] if plan.layout == ops.W_FP32 else None, 4 * H, 1, bias=q["bias"], pad_left=0,
                             t_out=T * BP, pad_mode=ops.PAD_ZERO, w_split=q["w_ih_split"] if plan.layout == ops.W_GEMM else None)
            return ops.lstm_layer(pre.view(4 * H, T, BP), q["w_hh"], H)

    # ------------------------------------------------------------------------------------------ the reference's surface
    @torch.no_grad()
    def forward(self, x):
        """model.py:102-137 in eval arithmetic -> (|classifier| (B, T), GAN_feature (B, 256, 10, T), poolblock_out (B, 256, T, 2))."""
        if self.num_class != 1:
            raise NotImplementedError("JDCNet on the HIP path is the F0 regressor (num_class = 1, modules/commons.py:186)")
        s3, geo = self._features(x)
        B, T, W, P, _ = geo
        s4 = self._pooled(s3, geo)
        gan = ops.jdc_to_nchw(s3, B, T, W[3], P[3], transposed=True)
        pooled = ops.jdc_to_nchw(s4, B, T, W[4], P[4])
        p = self._prep
        hf, hb = ops.run_chains([lambda: self._direction(s4, geo, p["fwd"], False), lambda: self._direction(s4, geo, p["bwd"], True)],
                                x.device, N_STREAMS, inputs=[s4])
        return ops.jdc_head(hf, hb, p["head"][0], p["head"][1], B), gan, pooled

    @torch.no_grad()
    def get_feature_GAN(self, x):
        """model.py:74-86: the activations after pool_block[0..1], (B, 256, 10, T)."""
        s3, (B, T, W, P, _) = self._features(x)
        return ops.jdc_to_nchw(s3, B, T, W[3], P[3], transposed=True)

    @torch.no_grad()
    def get_feature(self, x):
        """model.py:88-100: the pooled activations, (B, 256, T, 2)."""
        s3, geo = self._features(x)
        B, T, W, P, _ = geo
        return ops.jdc_to_nchw(self._pooled(s3, geo), B, T, W[4], P[4])
