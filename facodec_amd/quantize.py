"""FA-quantizer (reference: modules/quantize.py:156-454 FAquantizer.forward_v2) and its parts
(dac/nn/quantize.py VectorQuantize / ResidualVectorQuantize, modules/wavenet.py WN,
modules/style_encoder.py StyleEncoder, modules/attentions.py MultiHeadAttention), inference
(eval-mode) forward on the HIP C ABI.  State-dict keys follow the reference module tree.

Launch plan of forward_v2 (B clips):
  log-mel front-end: frames -> windowed-DFT GEMM (MFMA) -> |.|^2 -> mel GEMM with log epilogue,
                     computed ONCE and shared by the 80-bin timbre and 20-bin prosody branches
                     (the reference computes it twice, modules/quantize.py:378,385);
  timbre:  1x1 convs (+Mish epilogue) -> 2x (conv k5 -> GLU+residual) -> QKV convs -> attention ->
           out conv (+residual epilogue) -> fc -> masked mean;
  prosody: 1x1 conv -> 8x (conv k5 -> tanh*sigmoid gate -> 1x1 conv -> res/skip update) -> 1x1 conv;
  VQ:      6 fused fac_vq_fwd steps (1 prosody + 2 content + 3 residual);
  output:  LayerNorm over channels * gamma + beta (one kernel).
"""
import math
import os

import numpy as np
import torch
from torch import nn

from . import dsp, ops
from .wprep import cached_forward
from .layers import ConvWeights, SConv1d, _uniform_


# ------------------------------------------------------------------------------------ VQ
class _Codebook(nn.Module):
    def __init__(self, size, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(size, dim))


class VectorQuantize(nn.Module):
    """dac/nn/quantize.py:13-94.  Keys: in_proj.{weight_g,weight_v,bias}, out_proj.{...}, codebook.weight."""

    def __init__(self, input_dim, codebook_size, codebook_dim):
        super().__init__()
        if codebook_dim != 8:
            raise NotImplementedError("the VQ kernel is specialised for codebook_dim = 8 (modules/commons.py:303)")
        self.codebook_size, self.codebook_dim, self.input_dim = codebook_size, codebook_dim, input_dim
        self.in_proj = ConvWeights(input_dim, codebook_dim, 1, weight_norm=True)
        self.out_proj = ConvWeights(codebook_dim, input_dim, 1, weight_norm=True)
        self.codebook = _Codebook(codebook_size, codebook_dim)

    def _weights(self):
        """(packed in_proj (D,1,32), out_proj weight_v (D,8,1) as stored, its weight-norm scale (D,))."""
        v = self.out_proj.weight_v.detach()
        return self.in_proj.packed(), v, ops.wn_scale(v, self.out_proj.weight_g.detach())

    def decode_weights(self):
        """(codebook (Kc, 8), out_proj weight_v (D, 8, 1), its weight-norm scale (D,), bias (D,)): what fac_vq_decode reads."""
        v = self.out_proj.weight_v.detach()
        return self.codebook.weight.detach(), v, ops.wn_scale(v, self.out_proj.weight_g.detach()), self.out_proj.bias.detach()

    @torch.no_grad()
    def decode_code(self, embed_id):
        """dac/nn/quantize.py:72-76: codes (B, T) int64 -> raw codebook rows (B, 8, T)."""
        check_codes([embed_id.unsqueeze(1)], self.codebook_size)
        return ops.embed_sum(embed_id.unsqueeze(1).contiguous(), self.codebook.weight.detach().unsqueeze(0))

    def forward(self, z):
        B, D, T = z.shape
        codes = torch.empty(B, T, device=z.device, dtype=torch.int64)
        z_e = torch.empty(B, 8, T, device=z.device, dtype=torch.float32)
        out = torch.empty_like(z)
        nt = ops.vq_loss_tiles(T)
        lp = torch.empty(B, nt, device=z.device, dtype=torch.float32)
        w_in, w_out, w_out_scale = self._weights()
        ops.vq_step(z, w_in, self.in_proj.bias.detach(), self.codebook.weight.detach(), w_out, w_out_scale,
                    self.out_proj.bias.detach(), codes, zq_out=out, z_e=z_e, loss_part=lp)
        loss = lp.sum(1) / float(8 * T)
        return out, loss, loss.clone(), codes, z_e


class ResidualVectorQuantize(nn.Module):
    """dac/nn/quantize.py:97-198.  eval: `n_quantizers` codebooks for every sample.  train (:163-168): the first
    int(B * quantizer_dropout) samples keep only `torch.randint(1, n_codebooks + 1)` codebooks (drawn on the CPU's default
    generator exactly like the reference, or handed in as `masks` (n, B) of 0/1), forward and backward on the HIP path
    (`autograd.rvq`: straight-through estimator, commitment / codebook losses with the reference's detach placements);
    `latents` carry no gradient."""

    def __init__(self, input_dim=512, n_codebooks=9, codebook_size=1024, codebook_dim=8, quantizer_dropout=0.0):
        super().__init__()
        self.n_codebooks, self.codebook_size, self.codebook_dim = n_codebooks, codebook_size, codebook_dim
        self.quantizers = nn.ModuleList([VectorQuantize(input_dim, codebook_size, codebook_dim) for _ in range(n_codebooks)])
        self.quantizer_dropout = quantizer_dropout

    def forward(self, z, n_quantizers=None, masks=None):
        if self.training:
            from . import autograd as A
            B, _, T = z.shape
            if masks is None:
                masks = A.draw_quantizer_masks(self.n_codebooks, B, self.quantizer_dropout)
            latents = torch.empty(B, 8 * self.n_codebooks, T, device=z.device, dtype=torch.float32)
            z_q, codes, commit, cbl = A.rvq(self, z, ops.h2d(masks, z.device, torch.float32), latents=latents)
            return z_q, codes, latents, commit, cbl
        n = self.n_codebooks if n_quantizers is None else min(int(n_quantizers), self.n_codebooks)
        B, D, T = z.shape
        dev = z.device
        z_q = torch.zeros_like(z)
        codes = torch.empty(B, n, T, device=dev, dtype=torch.int64)
        latents = torch.empty(B, 8 * n, T, device=dev, dtype=torch.float32)
        nt = ops.vq_loss_tiles(T)
        lp = torch.empty(n, B, nt, device=dev, dtype=torch.float32)
        residual = torch.empty_like(z) if n > 1 else None
        src = z
        for i in range(n):
            q = self.quantizers[i]
            w_in, w_out, w_out_scale = q._weights()
            z_e_i = torch.empty(B, 8, T, device=dev, dtype=torch.float32)
            ops.vq_step(src, w_in, q.in_proj.bias.detach(), q.codebook.weight.detach(), w_out, w_out_scale,
                        q.out_proj.bias.detach(), codes[:, i], residual=residual if i < n - 1 else None,
                        zq_acc=z_q, z_e=z_e_i, loss_part=lp[i])
            latents[:, 8 * i: 8 * (i + 1)] = z_e_i
            src = residual
        per = lp.sum(2) / float(8 * T)       # (n, B)  mean over (8, T) per sample
        loss = per.mean(1).sum()             # mean over batch, summed over quantizers
        return z_q, codes, latents, loss, loss.clone()


    @torch.no_grad()
    def from_codes(self, codes):
        """dac/nn/quantize.py:200-220: codes (B, N, T) int64, N <= n_codebooks -> (z_q (B, D, T), z_p (B, 8N, T) = the looked-up
        codebook rows, codes).  z_q is the sum of the first N quantizers' out_proj(codebook[code]) (fac_vq_decode)."""
        B, N, T = codes.shape
        if N > self.n_codebooks:
            raise ValueError(f"from_codes: {N} code rows for {self.n_codebooks} quantizers")
        check_codes([codes], self.codebook_size)
        D = self.quantizers[0].input_dim
        z_q = torch.empty(B, D, T, device=codes.device, dtype=torch.float32)
        style = torch.zeros(B, 2 * D, device=codes.device, dtype=torch.float32)       # the kernel's normed output is not used
        ops.vq_decode([codes, None, None], [[q.decode_weights() for q in self.quantizers[:N]], [], []], style,
                      self.codebook_size, z_out=(z_q, None, None))
        z_p = [self.quantizers[i].decode_code(codes[:, i]) for i in range(N)]
        return z_q, (torch.cat(z_p, dim=1) if z_p else z_q.new_zeros(B, 0, T)), codes


def check_codes(codes, codebook_size):
    """Host-side validation of code tensors before a decode: int64, on the GPU, every index in [0, codebook_size) -- the range
    check is one device-to-host read for all tensors.  The kernels clamp indices only to stay inside the codebook."""
    flags = []
    for c in codes:
        if not isinstance(c, torch.Tensor) or c.dtype != torch.int64:
            raise TypeError(f"codes must be int64 tensors (got {getattr(c, 'dtype', type(c))})")
        if not c.is_cuda:
            from ._lib import FacodecHipError
            raise FacodecHipError(f"codes must live on the GPU (got {c.device}); there is no CPU path")
        if c.numel():
            flags.append(((c < 0) | (c >= codebook_size)).any())
    if flags and bool(torch.stack(flags).any()):
        raise ValueError(f"codes outside [0, {codebook_size})")


# ------------------------------------------------------------------------------------ WaveNet
class WN(nn.Module):
    """modules/wavenet.py:103-166.  Keys: [cond_layer.conv.conv.*,] in_layers.i.conv.conv.*,
    res_skip_layers.i.conv.conv.*.  With gin_channels the conditioning g (B, gin, 1) goes through one
    1x1 conv (2*hidden*n_layers rows) and layer i adds its slice before the tanh/sigmoid gate -- here
    inside the gate kernel (the reference broadcasts it over time first)."""

    def __init__(self, hidden_channels, kernel_size, dilation_rate, n_layers, gin_channels=0, p_dropout=0, causal=False):
        super().__init__()
        self.hidden_channels, self.n_layers, self.gin_channels = hidden_channels, n_layers, gin_channels
        self.in_layers = nn.ModuleList()
        self.res_skip_layers = nn.ModuleList()
        if gin_channels != 0:
            self.cond_layer = SConv1d(gin_channels, 2 * hidden_channels * n_layers, 1, norm="weight_norm")
        for i in range(n_layers):
            self.in_layers.append(SConv1d(hidden_channels, 2 * hidden_channels, kernel_size,
                                          dilation=dilation_rate ** i, norm="weight_norm", causal=causal))
            rs = 2 * hidden_channels if i < n_layers - 1 else hidden_channels
            self.res_skip_layers.append(SConv1d(hidden_channels, rs, 1, norm="weight_norm", causal=causal))

    def forward(self, x, x_mask=None, g=None, edge=None):
        """edge = (lens (B,) int32 frames on the device, 1): a right-padded batch of clips -- every in_layer's padding is written
        behind each clip of the running x before that layer reads it (SConv1d.run; x is this call's own copy)."""
        x = x.clone()
        out = torch.zeros_like(x)
        cond = None
        if g is not None:
            cond = self.cond_layer.run(g.reshape(g.shape[0], -1, 1)).reshape(g.shape[0], -1)   # (B, 2*H*L)
        H2 = 2 * self.hidden_channels
        for i in range(self.n_layers):
            a = self.in_layers[i].run(x, edge=edge)
            acts = ops.gate_tanh_sigmoid(a, None if cond is None else cond[:, i * H2:(i + 1) * H2])
            rs = self.res_skip_layers[i].run(acts)
            ops.wn_res_skip_(rs, x, out, last=(i == self.n_layers - 1))
        return out


# ------------------------------------------------------------------------------------ StyleEncoder
class _PlainConv(nn.Module):
    """nn.Conv1d parameters (weight (C_out,C_in,K), bias) + packed copy."""

    def __init__(self, c_in, c_out, k):
        super().__init__()
        b = 1.0 / math.sqrt(c_in * k)
        self.weight = nn.Parameter(_uniform_(torch.empty(c_out, c_in, k), b))
        self.bias = nn.Parameter(_uniform_(torch.empty(c_out), b))
        self.c_in, self.c_out, self.k = c_in, c_out, k

    def plan(self, B, T):
        """This class's variant of the conv rule (convplan.plan_conv): no C_out % 16, the channel floor at k = 7 too, no tail rule."""
        return ops.plan_conv(self.c_out, self.c_in, self.k, 1, 1, B, T, T, c_out_mult16=False, floor_k=(3, 5, 7), tail=None)

    def run(self, x, pad=0, **kw):
        """`same` convs: pad = (k - 1) / 2 (the 1x1 convs are never padded)."""
        layout, w = self.plan(x.shape[0], x.shape[-1]).layout, self.weight.detach()
        if layout == ops.W_GEMM:                # 1x1, many channels: bf16 pipe
            ws = ops.pack_gemm_weight_split(w)
        else:                                   # k = 5 convs of the style encoder: split-bf16 kernel (conv1d_bsplit.hip)
            ws = ops.pack_conv_weight_split(w) if layout == ops.W_TAPS else None
        return ops.conv1d(x, ops.pack_conv_weight(w) if ws is None else None, self.c_out, self.k, bias=self.bias.detach(),
                          pad_left=pad, pad_mode=ops.PAD_ZERO, t_out=x.shape[-1], w_split=ws, **kw)


class _Conv1dGLU(nn.Module):
    def __init__(self, c, k):
        super().__init__()
        self.conv1 = _PlainConv(c, 2 * c, k)


class MultiHeadAttention(nn.Module):
    """modules/attentions.py:120-199 without relative window / proximal bias."""

    def __init__(self, channels, out_channels, n_heads):
        super().__init__()
        self.n_heads = n_heads
        self.conv_q = _PlainConv(channels, channels, 1)
        self.conv_k = _PlainConv(channels, channels, 1)
        self.conv_v = _PlainConv(channels, channels, 1)
        self.conv_o = _PlainConv(channels, out_channels, 1)

    def forward(self, x, mask, res=None):
        q, k, v = self.conv_q.run(x), self.conv_k.run(x), self.conv_v.run(x)
        o = ops.attention(q, k, v, mask, self.n_heads)
        return self.conv_o.run(o, res=res)


class StyleEncoder(nn.Module):
    """modules/style_encoder.py:33-91 (eval).  Keys: spectral.{0,3}, temporal.{0,1}.conv1, slf_attn.*, fc."""

    def __init__(self, in_dim=513, hidden_dim=128, out_dim=256):
        super().__init__()
        # indices 0 and 3 of the reference's Sequential(conv, Mish, Dropout, conv, Mish, Dropout)
        self.spectral = nn.ModuleDict({"0": _PlainConv(in_dim, hidden_dim, 1), "3": _PlainConv(hidden_dim, hidden_dim, 1)})
        self.temporal = nn.ModuleList([_Conv1dGLU(hidden_dim, 5), _Conv1dGLU(hidden_dim, 5)])
        self.slf_attn = MultiHeadAttention(hidden_dim, hidden_dim, 2)
        self.fc = _PlainConv(hidden_dim, out_dim, 1)

    def forward(self, x, mask=None):
        """x (B, in_dim, T); mask (B, T) float 0/1 or None (= all frames valid) -> (B, out_dim)."""
        x = self.spectral["0"].run(x, act=ops.ACT_MISH)
        x = self.spectral["3"].run(x, act=ops.ACT_MISH)
        if mask is not None:
            ops.mul_mask_(x, mask)
        for glu in self.temporal:
            a = glu.conv1.run(x, pad=2)
            x = ops.glu_residual(a, x)
        if mask is not None:
            ops.mul_mask_(x, mask)
        x = self.slf_attn(x, mask, res=x)
        x = self.fc.run(x)
        return ops.masked_mean(x, mask)

    def forward_ragged(self, x, lens, mask, unit):
        """Per-clip-exact mode for a right-padded batch: x (B, in_dim, T), lens (B,) int32 sample counts on the device, row b
        has lens[b] // unit frames, mask (B, T) = ops.frame_mask(lens, T, unit) -> (B, out_dim), every row what `forward(x[b:b+1,
        :, :n_b])` gives.  Unlike the `mask=` path above (the reference's: only the first k = 5 GLU conv sees a zeroed tail, the
        second one reads what the first wrote past the clip's end), the tail is zeroed in front of EACH conv, which is the zero
        padding that conv has on the clip alone; keys past the end are masked out of the attention and the mean runs over the
        clip's own frames."""
        x = self.spectral["0"].run(x, act=ops.ACT_MISH)
        x = self.spectral["3"].run(x, act=ops.ACT_MISH)
        for glu in self.temporal:
            ops.mask_tail_(x, lens, unit)
            a = glu.conv1.run(x, pad=2)
            x = ops.glu_residual(a, x)
        ops.mask_tail_(x, lens, unit)
        x = self.slf_attn(x, mask, res=x)
        x = self.fc.run(x)
        ops.mask_tail_(x, lens, unit)                # fac_masked_mean sums every column and divides by the mask's sum
        return ops.masked_mean(x, mask)


# ------------------------------------------------------------------------------------ front-end
class LogMelFrontend(nn.Module):
    """FAquantizer.to_mel + preprocess (modules/quantize.py:219-242): torchaudio MelSpectrogram
    (sr 24000, n_fft 2048, win 1200 periodic Hann, hop 300, centre reflect, power 2, HTK 80 mels)
    then (log(1e-5 + mel) + 4) / 4.  Buffer names follow torchaudio so real checkpoints load."""

    def __init__(self, sample_rate=24000, n_fft=2048, win_length=1200, hop_length=300, n_mels=80):
        super().__init__()
        self.n_fft, self.win, self.hop, self.n_mels = n_fft, win_length, hop_length, n_mels
        self.spectrogram = nn.Module()
        self.spectrogram.register_buffer("window", torch.from_numpy(dsp.hann_periodic(win_length)))
        self.mel_scale = nn.Module()
        self.mel_scale.register_buffer("fb", torch.from_numpy(dsp.mel_fbank_htk(n_fft // 2 + 1, n_mels, sample_rate)))
        self._basis = None
        self._basis_split = None
        self._fb_packed = None

    def _consts(self, device):
        if self._basis is None or self._basis.device != device:
            win = self.spectrogram.window.detach().cpu().numpy()
            basis, self._off = dsp.dft_basis(self.n_fft, self.win, win)
            bt = torch.from_numpy(basis).to(device).unsqueeze(-1)
            self._basis = ops.pack_conv_weight(bt)
            self._basis_split = ops.pack_gemm_weight_split(bt) if ops.BF16_SPLIT else None
            fb = self.mel_scale.fb.detach().to(device).t().contiguous()  # (n_mels, F)
            self._fb_packed = ops.pack_conv_weight(fb.unsqueeze(-1))
        return self._basis, self._fb_packed, self._off

    def _apply(self, fn, *a, **kw):
        self._basis = None
        return super()._apply(fn, *a, **kw)

    def _load_from_state_dict(self, *a, **kw):
        """The packed DFT basis / filterbank are derived from the `to_mel.*` buffers: a checkpoint loaded after a forward
        must not keep the tables of the old buffers (hooked on the children too: the buffers live one level down)."""
        self._basis = None
        return super()._load_from_state_dict(*a, **kw)

    def forward(self, wave, all_frames=False):
        """wave (B, 1, T) or (B, T) -> normalised log-mel (B, n_mels, T // hop) (the quantizer's crop,
        modules/quantize.py:242) or, with all_frames, all 1 + T // hop centred frames (meldataset.py:45)."""
        w = wave.reshape(wave.shape[0], wave.shape[-1])
        n_frames = w.shape[1] // self.hop + (1 if all_frames else 0)
        off = self._consts(w.device)[2]
        return self._from_frames(ops.stft_frames(w, self.win, n_frames, self.hop, self.n_fft // 2, off))

    def forward_ragged(self, wave, lens):
        """Right-padded batch: wave (B, 1, T) or (B, T), lens (B,) int32 sample counts on the device -> (B, n_mels, T // hop); row
        b's first lens[b] // hop frames are `forward(wave[b:b+1, ..., :lens[b]])` (the frames reflect at the clip's own end), the
        columns behind them are the log-mel of silence."""
        w = wave.reshape(wave.shape[0], wave.shape[-1])
        off = self._consts(w.device)[2]
        return self._from_frames(ops.stft_frames_ragged(w, lens, self.win, w.shape[1] // self.hop, self.hop, self.n_fft // 2, off))

    def _from_frames(self, frames):
        B, _, n_frames = frames.shape
        basis, fbp, _ = self._consts(frames.device)
        F_ = self.n_fft // 2 + 1
        with ops.flop_key("dft"):
            if self._basis_split is not None and ops.plan_gemm(2 * F_, self.win, B * n_frames).layout == ops.W_GEMM:
                spec = ops.conv1d(frames, None, 2 * F_, 1, pad_left=0, pad_mode=ops.PAD_ZERO, t_out=n_frames, w_split=self._basis_split)
            else:
                spec = ops.conv1d(frames, basis, 2 * F_, 1, pad_left=0, pad_mode=ops.PAD_ZERO, t_out=n_frames)
            power = ops.spec_power(spec, 2)
            return ops.conv1d(power, fbp, self.n_mels, 1, pad_left=0, pad_mode=ops.PAD_ZERO, t_out=n_frames,
                              act=ops.ACT_LOG_MEL)


class _Linear(nn.Module):
    def __init__(self, c_in, c_out):
        super().__init__()
        b = 1.0 / math.sqrt(c_in)
        self.weight = nn.Parameter(_uniform_(torch.empty(c_out, c_in), b))
        self.bias = nn.Parameter(_uniform_(torch.empty(c_out), b))

    def forward(self, x):
        """x (B, C_in) -> (B, C_out) through the conv kernel on the (B, C_in, 1) view."""
        y = ops.conv1d(x.reshape(x.shape[0], x.shape[1], 1), ops.pack_conv_weight(self.weight.detach()),
                       self.weight.shape[0], 1, bias=self.bias.detach(), pad_left=0, pad_mode=ops.PAD_ZERO, t_out=1)
        return y.reshape(x.shape[0], -1)


class TimbreNorm(nn.Module):
    """`nn.LayerNorm(1024, elementwise_affine=False)` of modules/quantize.py:199, called on the (B, T, C) transpose at
    :447 and from outside the module at train.py:450-453 / eval.py:155-158.  Parameter- and buffer-free (no state-dict
    entry, like the reference's).  Runs fac_layernorm_c_affine with gamma = 1, beta = 0 (x_hat * 1 + 0 == x_hat
    bit for bit) on the (B, C, T) storage behind the caller's transpose; differentiable through the same kernel's
    backward.  forward_v2 itself uses the fused norm + gamma/beta launch (one pass instead of three)."""

    def __init__(self, normalized_shape=1024, eps=1e-5):
        super().__init__()
        self.normalized_shape, self.eps, self.elementwise_affine = (int(normalized_shape),), eps, False
        if eps != 1e-5:
            raise NotImplementedError("the LayerNorm kernel is built for eps = 1e-5 (modules/quantize.py:199)")

    def forward(self, x):
        """x (..., C), normalised over the last dimension."""
        from . import autograd as A
        C = self.normalized_shape[0]
        if x.shape[-1] != C:
            raise RuntimeError(f"TimbreNorm: expected last dimension {C}, got {tuple(x.shape)}")
        shape = x.shape
        xt = x.reshape(-1, shape[-2] if x.dim() > 1 else 1, C) if x.dim() != 3 else x
        bct = xt.transpose(1, 2)                      # the caller's x.transpose(1, 2) of a (B, C, T) tensor: already dense
        if not bct.is_contiguous():
            bct = bct.contiguous()
        style = torch.zeros(bct.shape[0], 2 * C, device=x.device, dtype=torch.float32)
        style[:, :C] = 1.0
        if torch.is_grad_enabled() and x.requires_grad:
            y = A.layernorm_affine(bct, style)
        else:
            y = ops.layernorm_c_affine(bct.detach(), style)
        return y.transpose(1, 2).reshape(shape)


# ------------------------------------------------------------------------------------ FAquantizer
def sequence_mask(length, max_length=None):
    """modules/quantize.py:127-131."""
    if max_length is None:
        max_length = int(length.max())
    x = torch.arange(max_length, dtype=length.dtype, device=length.device)
    return x.unsqueeze(0) < length.unsqueeze(1)


def mel_chunk_plan(T, chunk_frames, hop=300, n_fft=2048):
    """Chunks of the centred STFT of a T-sample signal, T // hop frames: -> [(f0, f1, s_lo, s_hi, pad)]: frames [f0, f1) are
    ops.stft_frames of wave[s_lo:s_hi] with `pad` samples of reflect padding on the left.  Frame f reads the samples
    [hop f - n_fft / 2, hop f + n_fft / 2): the slice is what the chunk's frames reach, cut at the signal's two ends, where --
    and only where -- the call reflects (pad > 0 only with s_lo = 0; the right reflection only with s_hi = T)."""
    half = n_fft // 2
    plan = []
    for f0 in range(0, T // hop, chunk_frames):
        f1 = min(T // hop, f0 + chunk_frames)
        lo, hi = hop * f0 - half, hop * (f1 - 1) + half
        plan.append((f0, f1, max(lo, 0), min(hi, T), max(-lo, 0)))
    return plan


QUANT_STREAMS = int(os.environ.get("FAC_QUANT_STREAMS", "3"))     # concurrent chains of FAquantizer's eval forward (1 = serial)


class FAquantizer(nn.Module):
    """modules/quantize.py:156-454 with timbre_norm=True / separate_prosody_encoder=True
    (configs/config.yml:27-46); `forward` is the reference's forward_v2 (:235-237)."""

    def __init__(self, in_dim=1024, n_p_codebooks=1, n_c_codebooks=2, n_t_codebooks=2, n_r_codebooks=3,
                 codebook_size=1024, codebook_dim=8, quantizer_dropout=0.5, causal=False,
                 separate_prosody_encoder=False, timbre_norm=False):
        super().__init__()
        if not (timbre_norm and separate_prosody_encoder):
            raise NotImplementedError("only the shipped configuration (timbre_norm + separate_prosody_encoder) is built")
        rvq = lambda n: ResidualVectorQuantize(in_dim, n, codebook_size, codebook_dim, quantizer_dropout)  # noqa: E731
        self.prosody_quantizer = rvq(n_p_codebooks)
        self.content_quantizer = rvq(n_c_codebooks)
        self.timbre_encoder = StyleEncoder(in_dim=80, hidden_dim=512, out_dim=in_dim)
        self.timbre_linear = _Linear(1024, 1024 * 2)
        with torch.no_grad():
            self.timbre_linear.bias[:1024] = 1
            self.timbre_linear.bias[1024:] = 0
        self.timbre_norm = TimbreNorm(1024)
        self.residual_quantizer = rvq(n_r_codebooks)
        self.melspec_linear = SConv1d(20, 256, 1, causal=causal)
        self.melspec_encoder = WN(hidden_channels=256, kernel_size=5, dilation_rate=1, n_layers=8, gin_channels=0,
                                  p_dropout=0.2, causal=causal)
        self.melspec_linear2 = SConv1d(256, 1024, 1, causal=causal)
        self.to_mel = LogMelFrontend(24000, 2048, 1200, 300, 80)
        self.hop_length = 300
        self.in_dim = in_dim
        self.is_timbre_norm = True
        self.separate_prosody_encoder = True

    def preprocess(self, wave_tensor, n_bins=20):
        return self.to_mel(wave_tensor)[:, :n_bins]

    prob_random_mask_residual = 0.75     # modules/quantize.py:217

    def _forward_train(self, x, wave_segments, full_waves, wave_lens, return_codes, masks=None):
        """forward_v2 in training mode (modules/quantize.py:375-454) with HIP forward + backward.
        Every branch carries gradient: the three RVQs (straight-through, commitment / codebook losses, quantizer
        dropout), the residual path into the encoder latent, LayerNorm + timbre_linear, the timbre encoder
        (Mish / GLU / attention / masked mean, dropout 0.1) and the prosody WaveNet (gates, dropout 0.2).
        masks: optional dict(p=, c=, r= (n, B) quantizer-dropout masks, res= (B,) residual mask, dropout=False to
        switch the Bernoulli dropouts off) for reproducible steps; drawn like the reference otherwise."""
        from . import autograd as A
        from . import autograd_quant as AQ
        import numpy as np
        B = x.shape[0]
        dev = x.device
        use_drop = bool((masks or {}).get("dropout", True))      # WaveNet p = 0.2, StyleEncoder p = 0.1
        mel = self.to_mel(wave_segments)                           # constant input features (no gradient)
        n = min(mel.shape[-1], x.shape[2])
        if x.shape[2] != n:
            x = x[:, :, :n].contiguous()
        masks = masks or {}

        def qmask(key, rvq):
            mk = masks.get(key)
            if mk is None:
                mk = A.draw_quantizer_masks(rvq.n_codebooks, B, rvq.quantizer_dropout)
            return ops.h2d(mk, dev)                     # asynchronous: a blocking copy here costs the host its lead over the device

        # The same three independent chains as the eval forward, side by side (ops.run_chains; autograd replays each chain's backward
        # on the chain's stream).  The chains are ISSUED one after the other by the host, so the random draws keep their order:
        # StyleEncoder dropout, WaveNet dropout, prosody quantizer-dropout draw, content draw (then the residual draw below).
        def timbre_chain():
            if full_waves is None:
                return AQ.style_encoder(self.timbre_encoder, mel, None, use_dropout=use_drop)
            mel_full = self.to_mel(full_waves)
            m = sequence_mask(ops.h2d(wave_lens, dev) // self.hop_length, mel_full.shape[-1]).to(torch.float32).contiguous()
            return AQ.style_encoder(self.timbre_encoder, mel_full, m, use_dropout=use_drop)

        def prosody_chain():
            f0 = A.conv(self.melspec_linear, mel[:, :20].contiguous())
            f0 = A.conv(self.melspec_linear2, AQ.wavenet(self.melspec_encoder, f0, use_dropout=use_drop))
            if f0.shape[2] != n:
                f0 = f0[:, :, :n].contiguous()
            return A.rvq(self.prosody_quantizer, f0, qmask("p", self.prosody_quantizer))

        timbre, (z_p, codes_p, cm_p, cb_p), (z_c, codes_c, cm_c, cb_c) = ops.run_chains(
            [timbre_chain, prosody_chain, lambda: A.rvq(self.content_quantizer, x, qmask("c", self.content_quantizer))], dev, QUANT_STREAMS,
            inputs=[mel, x, full_waves, wave_lens, [v for v in masks.values() if torch.is_tensor(v)]])
        z_r, codes_r, cm_r, cb_r = A.rvq(self.residual_quantizer, A.sub_detached(x, z_p, z_c), qmask("r", self.residual_quantizer))
        res = masks.get("res")
        if res is None:
            res = torch.from_numpy(np.random.choice([0, 1], size=B, p=[self.prob_random_mask_residual,
                                                                       1 - self.prob_random_mask_residual]))
        res = ops.h2d(res, dev, torch.float32).contiguous()
        outs = A.mix_outs(z_p, z_c, z_r, res)
        outs = A.layernorm_affine(outs, A.linear(self.timbre_linear, timbre))
        quantized = [z_p, z_c, z_r]
        commitment, codebook = cm_p + cm_c + cm_r, cb_p + cb_c + cb_r
        if return_codes:
            return outs, quantized, commitment, codebook, timbre, [codes_p, codes_c, codes_r]
        return outs, quantized, commitment, codebook, timbre

    @cached_forward
    def forward(self, x, wave_segments, n_c=1, n_t=2, full_waves=None, wave_lens=None, return_codes=False, masks=None):
        if self.training:
            return self._forward_train(x, wave_segments, full_waves, wave_lens, return_codes, masks)
        mel = self.to_mel(wave_segments)                      # (B, 80, F) computed once
        n = min(mel.shape[-1], x.shape[2])
        if x.shape[2] != n:
            x = x[:, :, :n].contiguous()

        # Three independent chains (round 5): the timbre encoder, the prosody branch (1x1 -> WaveNet -> 1x1 -> prosody RVQ) and the
        # content RVQ depend only on the log-mel features / the latent; at the 160-frame latent rate their ~60 launches have
        # 128 - 256 workgroups each, less than one round of the chip.  Side by side on side streams (ops.run_chains, as the eight
        # discriminators and the predictor heads in training): same kernels, same results, FAC_QUANT_STREAMS=1 runs them in turn.
        def timbre_chain():
            if full_waves is None:
                return self.timbre_encoder(mel, None)
            mel_full = self.to_mel(full_waves)
            m = sequence_mask(ops.h2d(wave_lens, mel_full.device) // self.hop_length, mel_full.shape[-1]).to(torch.float32).contiguous()
            return self.timbre_encoder(mel_full, m)

        def prosody_chain():
            f0 = ops.conv1d(mel[:, :20], self.melspec_linear.w.packed(), 256, 1, bias=self.melspec_linear.w.bias,
                            pad_left=0, pad_mode=ops.PAD_ZERO, t_out=mel.shape[-1])
            f0 = self.melspec_linear2.run(self.melspec_encoder(f0))
            if f0.shape[2] != n:
                f0 = f0[:, :, :n].contiguous()
            return self.prosody_quantizer(f0, 1)

        timbre, (z_p, codes_p, _, cm_p, cb_p), (z_c, codes_c, _, cm_c, cb_c) = ops.run_chains(
            [timbre_chain, prosody_chain, lambda: self.content_quantizer(x, n_c)], x.device, QUANT_STREAMS, inputs=[mel, x, full_waves, wave_lens])
        residual_feature = ops.sub2(x, z_p, z_c)
        z_r, codes_r, _, cm_r, cb_r = self.residual_quantizer(residual_feature, 3)
        outs = ops.add(ops.add(z_p, z_c), z_r)

        style = self.timbre_linear(timbre)                    # (B, 2D) = [gamma | beta]
        outs = ops.layernorm_c_affine(outs, style)

        quantized = [z_p, z_c, z_r]
        commitment = cm_p + cm_c + cm_r
        codebook = cb_p + cb_c + cb_r
        if return_codes:
            return outs, quantized, commitment, codebook, timbre, [codes_p, codes_c, codes_r]
        return outs, quantized, commitment, codebook, timbre

    forward_v2 = forward

    @cached_forward
    def forward_ragged(self, x, waves, lens, n_c=2):
        """Eval forward of a right-padded batch of clips with different lengths: x (B, D, F) the encoder's latent of waves
        (B, 1, T), lens (B,) int32 sample counts on the device (never read back) -> (outs (B, D, n), [codes_p, codes_c, codes_r],
        timbre (B, D), frame_lens (B,) int32 = lens // hop), n = T // hop.  Row b's first frame_lens[b] frames and its timbre are
        what `forward(x[b:b+1, :, :n_b], waves[b:b+1, :, :lens[b]], n_c, return_codes=True)` gives: the log-mel frames reflect at
        the clip's own end, the timbre encoder runs in its per-clip-exact mode (StyleEncoder.forward_ragged), everything else is
        causal or per-frame (the caller checks the configuration: commons.encode_clips).  outs and codes behind a clip's last
        frame are zeros.  The lengths are validated where they originate, on the host (commons.min_clip_samples)."""
        if self.training:
            raise RuntimeError("FAquantizer.forward_ragged is an eval-mode forward (call .eval() first); training batches are equal-length crops")
        hop = self.hop_length
        mel = self.to_mel.forward_ragged(waves, lens)         # (B, 80, n) computed once
        n = min(mel.shape[-1], x.shape[2])
        if x.shape[2] != n:
            x = x[:, :, :n].contiguous()
        mask, frame_lens = ops.frame_mask(lens, mel.shape[-1], hop)

        def prosody_chain():                                  # as in `forward`
            f0 = ops.conv1d(mel[:, :20], self.melspec_linear.w.packed(), 256, 1, bias=self.melspec_linear.w.bias,
                            pad_left=0, pad_mode=ops.PAD_ZERO, t_out=mel.shape[-1])
            f0 = self.melspec_linear2.run(self.melspec_encoder(f0))
            if f0.shape[2] != n:
                f0 = f0[:, :, :n].contiguous()
            return self.prosody_quantizer(f0, 1)

        timbre, (z_p, codes_p, _, _, _), (z_c, codes_c, _, _, _) = ops.run_chains(
            [lambda: self.timbre_encoder.forward_ragged(mel, lens, mask, hop), prosody_chain, lambda: self.content_quantizer(x, n_c)],
            x.device, QUANT_STREAMS, inputs=[mel, x, lens, mask])
        z_r, codes_r, _, _, _ = self.residual_quantizer(ops.sub2(x, z_p, z_c), 3)
        outs = ops.layernorm_c_affine(ops.add(ops.add(z_p, z_c), z_r), self.timbre_linear(timbre))
        ops.mask_tail_(outs, lens, hop)
        codes = [ops.mask_tail_(c, lens, hop) for c in (codes_p, codes_c, codes_r)]
        return outs, codes, timbre, frame_lens

    @torch.no_grad()
    def log_mel_chunked(self, wave, chunk_frames=4096):
        """`to_mel(wave)` (B, 80, T // hop) with the STFT in chunks of `chunk_frames` frames: the (n_win, F) frame tensor and the
        (2050, F) spectrum exist per chunk only.  A chunk is framed from the samples its frames reach, so the reflect padding
        applies at the two ends of the signal and nowhere else (the explicit-pad call of streaming._QuantizerStream._mel)."""
        fe = self.to_mel
        w = wave.reshape(wave.shape[0], wave.shape[-1])
        B, T = w.shape
        F = T // fe.hop
        chunk_frames = int(chunk_frames)
        if chunk_frames < 1:
            raise ValueError(f"chunk_frames = {chunk_frames}")
        if T <= fe.n_fft // 2:
            raise ValueError(f"{T} samples: the log-mel front-end reflects n_fft / 2 = {fe.n_fft // 2} samples at either end")
        off = fe._consts(w.device)[2]
        mel = torch.empty(B, fe.n_mels, F, device=w.device, dtype=torch.float32)
        for f0, f1, s_lo, s_hi, pad in mel_chunk_plan(T, chunk_frames, fe.hop, fe.n_fft):
            view = w[:, s_lo:s_hi].contiguous()
            mel[:, :, f0:f1] = fe._from_frames(ops.stft_frames(view, fe.win, f1 - f0, fe.hop, pad, off))
        return mel

    @torch.no_grad()
    def timbre_long(self, wave, lens=None, chunk_frames=4096):
        """The timbre vector (B, 1024) of recordings of any length: wave (B, 1, T) or (B, T) fp32 on the GPU -> what
        `forward(z, wave)[4]` gives, within fp32 noise, in memory that grows with T only through frame-rate tensors of 80 to 1024
        rows: the log-mel front-end runs in chunks (log_mel_chunked), the style encoder over all frames, its attention on whichever
        kernel ops.attention_route names (past 2304 frames the running-max kernel: no T x T tensor, no score row).
        lens: per-row sample counts (a sequence of ints, or a tensor that is read back once); every row is then run on its own
        samples alone, one after the other."""
        if self.training:
            raise RuntimeError("FAquantizer.timbre_long is an eval-mode call (call .eval() first)")
        if not isinstance(wave, torch.Tensor) or not wave.is_cuda:
            from ._lib import FacodecHipError
            raise FacodecHipError(f"wave must live on the GPU (got {getattr(wave, 'device', type(wave))}); there is no CPU path")
        w = wave.reshape(wave.shape[0], 1, wave.shape[-1])
        if lens is not None:
            lens = [int(n) for n in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
            if len(lens) != w.shape[0] or any(n < 1 or n > w.shape[-1] for n in lens):
                raise ValueError(f"lens must give {w.shape[0]} sample counts in [1, {w.shape[-1]}]")
            return torch.cat([self.timbre_long(w[b:b + 1, :, :n], None, chunk_frames) for b, n in enumerate(lens)])
        return self.timbre_encoder(self.log_mel_chunked(w, chunk_frames), None)

    def decode_weights(self):
        """Per RVQ (prosody, content, residual) the decode_weights() of every quantizer."""
        return [[q.decode_weights() for q in rvq.quantizers]
                for rvq in (self.prosody_quantizer, self.content_quantizer, self.residual_quantizer)]

    def _check_decode_inputs(self, codes, timbre):
        """-> quantizer counts (n_p, n_c, n_r) from the code tensors' row counts; validates the rest (ValueError / TypeError, and
        FacodecHipError for CPU tensors like every product call)."""
        if not isinstance(codes, (list, tuple)) or len(codes) != 3:
            raise ValueError("codes must be [codes_p (B,n_p,T), codes_c (B,n_c,T), codes_r (B,n_r,T)]")
        for c in codes:
            if not isinstance(c, torch.Tensor) or c.dim() != 3:
                raise ValueError("every code tensor must be (B, N, T)")
        B, T = codes[0].shape[0], codes[0].shape[2]
        for c, rvq in zip(codes, (self.prosody_quantizer, self.content_quantizer, self.residual_quantizer)):
            if c.shape[0] != B or c.shape[2] != T:
                raise ValueError(f"code tensors disagree on (B, T): {[tuple(x.shape) for x in codes]}")
            if c.shape[1] > rvq.n_codebooks:
                raise ValueError(f"{c.shape[1]} code rows for an RVQ of {rvq.n_codebooks} quantizers")
        if T < 1:
            raise ValueError("codes have no frames")
        if not isinstance(timbre, torch.Tensor) or tuple(timbre.shape) != (B, self.in_dim) or timbre.dtype != torch.float32:
            raise ValueError(f"timbre must be float32 ({B}, {self.in_dim}), got {getattr(timbre, 'shape', None)}")
        if not timbre.is_cuda:
            from ._lib import FacodecHipError
            raise FacodecHipError(f"timbre must live on the GPU (got {timbre.device}); there is no CPU path")
        check_codes(codes, self.prosody_quantizer.codebook_size)
        return [c.shape[1] for c in codes]

    def _decode(self, codes, timbre, want_quantized):
        n_q = self._check_decode_inputs(codes, timbre)
        B, T = codes[0].shape[0], codes[0].shape[2]
        style = self.timbre_linear(timbre.contiguous())                    # (B, 2D) = [gamma | beta]
        weights = [w[:n] for w, n in zip(self.decode_weights(), n_q)]
        z = [torch.empty(B, self.in_dim, T, device=timbre.device, dtype=torch.float32) for _ in range(3)] if want_quantized else None
        outs = ops.vq_decode([c if n else None for c, n in zip(codes, n_q)], weights, style, self.prosody_quantizer.codebook_size,
                             z_out=z if want_quantized else (None, None, None))
        return outs, z

    @torch.no_grad()
    @cached_forward
    def from_codes(self, codes, timbre):
        """Codes + timbre -> decoder input: per RVQ ResidualVectorQuantize.from_codes (dac/nn/quantize.py:200-220), then the tail
        of forward_v2 (modules/quantize.py:436-449, eval: res_mask = 1) -- what `forward` hands the decoder, minus the
        ulp-level straight-through term z_e + (z_q - z_e).  The reference's own `decode` (:244-255) reads a timbre_quantizer
        that the shipped configuration (timbre_norm=True) does not build.

        codes = [codes_p (B, n_p, T), codes_c (B, n_c, T), codes_r (B, n_r, T)] int64 as `forward(..., return_codes=True)`
        returns them; the quantizer counts come from the row counts (0 included: n_c = 1, no residual ...).  timbre (B, 1024):
        the clip's own (`forward`'s 5th output) or another speaker's (timbre swap, the paper's zero-shot voice conversion).
        -> (outs (B, 1024, T), [z_p, z_c, z_r]).  One fac_vq_decode launch; codes outside [0, codebook_size) raise ValueError."""
        outs, z = self._decode(codes, timbre, True)
        return outs, z

    @torch.no_grad()
    @cached_forward
    def decode_input(self, codes, timbre):
        """`from_codes(codes, timbre)[0]` without writing the per-RVQ sums (the decode path)."""
        return self._decode(codes, timbre, False)[0]
