"""Voice-conversion re-decoder (reference: modules/redecoder.py:4-48, `encoder_type: wavenet`; call site
reconstruct_redecoder.py:110-122): code embeddings summed per frame -> 16-layer WaveNet conditioned on the
timbre vector -> 1x1 conv back to the 1024-d latent that the (non-causal, LSTM-free) Decoder consumes.
The `mamba` branch of the reference imports a module that is not in its tree (modules.mamba): not built."""
import torch
from torch import nn
from torch.autograd import Function

from . import ops
from .quantize import WN, _PlainConv


class _Embedding(nn.Module):
    def __init__(self, n, d):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(n, d))


class Redecoder(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.n_p_codebooks, self.n_c_codebooks = args.n_p_codebooks, args.n_c_codebooks
        self.codebook_size = 1024
        self.encoder_type = args.encoder_type
        if args.encoder_type != "wavenet":
            raise NotImplementedError("only encoder_type 'wavenet' is built (the reference's 'mamba' module is absent)")
        self.embed_dim = args.wavenet_embed_dim
        self.encoder = WN(hidden_channels=self.embed_dim, kernel_size=5, dilation_rate=1, n_layers=16, gin_channels=1024,
                          p_dropout=0.2, causal=args.decoder_causal)
        self.conv_out = _PlainConv(self.embed_dim, 1024, 1)
        self.prosody_embed = nn.ModuleList([_Embedding(self.codebook_size, self.embed_dim) for _ in range(self.n_p_codebooks)])
        self.content_embed = nn.ModuleList([_Embedding(self.codebook_size, self.embed_dim) for _ in range(self.n_c_codebooks)])

    def forward(self, p_code, c_code, timbre_vec, use_p_code=True, use_c_code=True, n_c=2, dropout=True):
        """p_code (B, n_p, T), c_code (B, >= n_c, T) int64; timbre_vec (B, 1024) -> (B, 1024, T).
        In .train() mode the pass runs with autograd (_forward_train); dropout=False there turns the WaveNet's dropout off
        (golden tests)."""
        if self.training:
            return self._forward_train(p_code, c_code, timbre_vec, use_p_code, use_c_code, n_c, dropout)
        return self._forward_eval(p_code, c_code, timbre_vec, use_p_code, use_c_code, n_c)

    def forward_ragged(self, p_code, c_code, timbre_vec, lens, use_p_code=True, use_c_code=True, n_c=2):
        """forward on a right-padded batch of clips of different lengths: codes (B, n, F') padded with any valid
        code, lens (B,) int32 on the device, every clip's length in frames -> (B, 1024, F'), of which [b, :, :lens[b]] is what
        forward gives clip b alone; what sits behind a clip is meaningless.  F' must leave commons.ragged_slack_frames columns
        behind the longest clip.  Every non-causal WaveNet layer is preceded by one ops.edge_tail_ launch that writes the
        layer's reflection at each clip's own end; a causal WaveNet gets none.  Eval only."""
        if self.training:
            raise RuntimeError("Redecoder.forward_ragged is an eval-mode forward (call .eval() first); training batches are equal-length crops")
        return self._forward_eval(p_code, c_code, timbre_vec, use_p_code, use_c_code, n_c, edge=(lens, 1))

    def _forward_eval(self, p_code, c_code, timbre_vec, use_p_code, use_c_code, n_c, edge=None):
        B, _, T = p_code.shape
        x = torch.zeros(B, self.embed_dim, T, device=p_code.device, dtype=torch.float32)
        if use_p_code and self.n_p_codebooks:
            tabs = torch.stack([e.weight.detach() for e in self.prosody_embed])
            ops.embed_sum(p_code, tabs, 0, out=x)
        if use_c_code and n_c:
            tabs = torch.stack([e.weight.detach() for e in list(self.content_embed)[:n_c]])
            ops.embed_sum(c_code, tabs, 0, out=x)
        x = self.encoder(x, None, g=timbre_vec, edge=edge)
        return self.conv_out.run(x)

    def _forward_train(self, p_code, c_code, timbre_vec, use_p_code, use_c_code, n_c, dropout):
        """Training mode (train_redecoder.py:220-228): the embedding tables in use (prosody, the first n_c content tables), the
        WaveNet (its cond_layer included, dropout p = 0.2 after every gate) and conv_out get gradients; the codes and the
        timbre vector, outputs of the frozen codec, do not."""
        from . import autograd_quant as AQ
        p_tabs = [e.weight for e in self.prosody_embed] if use_p_code and self.n_p_codebooks else []
        c_tabs = [e.weight for e in list(self.content_embed)[:n_c]] if use_c_code and n_c else []
        x = _EmbedSum.apply(p_code, c_code, len(p_tabs), self.embed_dim, *p_tabs, *c_tabs)
        x = AQ.wavenet(self.encoder, x, p_dropout=0.2, use_dropout=dropout, g=timbre_vec)
        return AQ.plain_conv(self.conv_out, x)


class _EmbedSum(Function):
    """x (B, E, T) = sum of the prosody tables at p_code rows + the content tables at c_code rows (the launches of the eval
    forward); backward: one deterministic fac_embed_sum_bwd launch per code tensor for the dense table gradients."""

    @staticmethod
    def forward(ctx, p_code, c_code, n_p, E, *tabs):
        B, _, T = p_code.shape
        ctx.n_p, ctx.V = n_p, tabs[0].shape[0] if tabs else 0
        ctx.save_for_backward(p_code, c_code)
        x = torch.zeros(B, E, T, device=p_code.device, dtype=torch.float32)
        if n_p:
            ops.embed_sum(p_code, torch.stack([t.detach() for t in tabs[:n_p]]), 0, out=x)
        if len(tabs) > n_p:
            ops.embed_sum(c_code, torch.stack([t.detach() for t in tabs[n_p:]]), 0, out=x)
        ctx.n_c = len(tabs) - n_p
        return x

    @staticmethod
    def backward(ctx, dx):
        p_code, c_code = ctx.saved_tensors
        dx = dx.contiguous()
        grads = []
        if ctx.n_p:
            grads += list(ops.embed_sum_bwd(dx, p_code, ctx.n_p, ctx.V).unbind(0))
        if ctx.n_c:
            grads += list(ops.embed_sum_bwd(dx, c_code, ctx.n_c, ctx.V).unbind(0))
        return (None, None, None, None, *grads)
