"""The training iteration of the voice-conversion redecoder (reference train_redecoder.py:195-328, `encoder_type: wavenet`) on
the HIP path.

    wav_seg = crop(waves, mel_input_length)                                                     train_redecoder.py:197-217
    with no_grad:  z = codec.encoder(wav_seg)
                   ..., timbre, codes = codec.quantizer(z, wav_seg, n_c=2, full_waves=waves,
                                                        wave_lens=wave_lens, return_codes=True)    :219-227
    pred = decoder(encoder(codes[0], codes[1], timbre))                                          :228, :262-270
    discriminator:  LSGAN loss_d; clip 10; AdamW; ExponentialLR                                  :273-290
    generator:      15 mel + feature matching + adversarial; clip encoder and decoder to 1000 each; AdamW x2   :298-328

The frozen codec is the `stage='encoder'` model in eval mode (commons.build_model + load_checkpoint); the redecoder is the
`stage='redecoder'` Munch(encoder=Redecoder, decoder=Decoder) in train mode; the discriminator is discriminator.Discriminator with
the reference's redecoder arguments (modules/commons.py:401-407), whose state-dict keys are the reference's.

Reference defect: train_redecoder.py:220-226 passes two positional flags (`torch.ones(B).bool()` twice) before `n_c`.  With
`timbre_norm: True` the quantizer's forward IS forward_v2 (modules/quantize.py:236-237, :375), which has no such parameters, so
the call raises `TypeError: got multiple values for argument 'n_c'`.  The flags are the `noise_added_flags` / `recon_noisy_flags`
of the old forward (:303); this step makes the call without them.
"""
import torch

from . import losses, optim
from .train import crop_segments

OPT_KEYS = ("encoder", "decoder", "discriminator")


def redecoder_discriminator(sample_rate=24000):
    """modules/commons.py:401-407: the redecoder's discriminator (the codec's arguments, the dac default bands)."""
    from .discriminator import Discriminator
    return Discriminator(rates=[], periods=[2, 3, 5, 7, 11], fft_sizes=[2048, 1024, 512], sample_rate=sample_rate,
                         bands=[(0.0, 0.1), (0.1, 0.25), (0.25, 0.5), (0.5, 0.75), (0.75, 1.0)])


class RedecoderTrainStep:
    """One train_redecoder.py iteration per call.  After a call every `p.grad` of the three optimised keys still holds the step's
    unclipped gradient (the discriminator's: of loss_d); the arenas are cleared at the start of the next call.  Single rank."""

    def __init__(self, model, codec, discriminator, lr=1e-4, sample_rate=24000, max_frame_len=80, hop=300, dropout=True):
        """model: Munch(encoder=Redecoder, decoder=Decoder); codec: Munch(encoder, quantizer), frozen; dropout=False turns the
        WaveNet's dropout off (golden tests: the reference fixture runs with p = 0)."""
        self.model, self.codec, self.disc = model, codec, discriminator
        self.max_frame_len, self.hop, self.dropout = max_frame_len, hop, dropout
        model.encoder.train()
        model.decoder.train()
        discriminator.train()
        for k in ("encoder", "quantizer"):
            codec[k].eval()
            for p in codec[k].parameters():
                p.requires_grad_(False)
        # optimizers.py:93-105: AdamW(lr, (0.9, 0.98), 1e-9, wd 0.1) + ExponentialLR(0.999996) per key; clips of :288, :321-322
        self.opt = {"encoder": optim.FlatAdamW(model.encoder.parameters(), lr=lr, max_norm=1000.0),
                    "decoder": optim.FlatAdamW(model.decoder.parameters(), lr=lr, max_norm=1000.0),
                    "discriminator": optim.FlatAdamW(discriminator.parameters(), lr=lr, max_norm=10.0)}
        self.mel = losses.MelSpectrogramLoss(n_mels=[5, 10, 20, 40, 80, 160, 320], window_lengths=[32, 64, 128, 256, 512, 1024, 2048],
                                             mel_fmin=[0] * 7, mel_fmax=[None] * 7, pow=1.0, mag_weight=0.0, clamp_eps=1e-5,
                                             sample_rate=sample_rate)          # train_redecoder.py:142-150
        self.stft = losses.MultiScaleSTFTLoss()
        self.l1 = losses.L1Loss()

    def codec_forward(self, wav_seg, waves, wave_lens):
        """Frozen codec, no_grad, eval mode (train_redecoder.py:219-227 without the two stray flags): -> (codes, timbre)."""
        with torch.no_grad():
            z = self.codec.encoder(wav_seg)
            _, _, _, _, timbre, codes = self.codec.quantizer(z, wav_seg, n_c=2, full_waves=waves, wave_lens=wave_lens, return_codes=True)
        return codes, timbre

    def __call__(self, waves, wave_lens, mel_input_length, starts=None, generator=None):
        """waves (B, T_full) padded batch on the device; wave_lens (B,) samples; mel_input_length: per-clip frame counts (host
        sequence); starts: optional (B,) crop offsets in frames (else drawn as the reference does).  Returns the loss scalars and
        the three pre-clip gradient norms (device tensors)."""
        from .discriminator import gan_loss_d_batched, gan_losses
        m, opt, disc = self.model, self.opt, self.disc
        for k in OPT_KEYS:
            opt[k].zero_grad(unbind=opt[k].data_parallel)
        wav_seg, _, _ = crop_segments(waves, mel_input_length, self.max_frame_len, self.hop, starts=starts, generator=generator)
        codes, timbre = self.codec_forward(wav_seg, waves, wave_lens)
        pred = m.decoder(m.encoder(codes[0], codes[1], timbre, dropout=self.dropout))
        target = wav_seg
        len_diff = target.size(-1) - pred.size(-1)                       # train_redecoder.py:268-270
        if len_diff > 0:
            target = target[..., len_diff // 2:-len_diff // 2].contiguous()
        # ---- discriminator (:273-290): one pass over [fake | real]
        loss_d = gan_loss_d_batched(disc.forward_internal(torch.cat([pred.detach(), target], 0)))
        loss_d.backward()
        opt["discriminator"].launch_all_reduce()
        mel = self.mel(pred, target)
        with torch.no_grad():                                            # logged only (:294-297)
            stft, waveform = self.stft(pred, target), self.l1(pred, target)
        opt["discriminator"].step(zero_grad=False)
        # ---- generator (:298-328): the updated discriminator, differentiated w.r.t. its input only
        for p in opt["discriminator"].params:
            p.requires_grad_(False)
        try:
            d_fake = disc.forward_internal(pred)
            with torch.no_grad():
                d_real = disc.forward_internal(target)
            _, loss_g, loss_feat = gan_losses(d_fake, d_real)
            loss = 15.0 * mel + 1.0 * loss_feat + 1.0 * loss_g
            loss.backward()
        finally:
            for p in opt["discriminator"].params:
                p.requires_grad_(True)
        for k in ("decoder", "encoder"):
            opt[k].launch_all_reduce()
        for k in ("encoder", "decoder"):                                  # clipped separately (:321-322), then stepped (:324-328)
            opt[k].step(zero_grad=False)
        return dict(loss_d=loss_d.detach(), loss_gen_all=loss.detach(), mel=mel.detach(), loss_g=loss_g.detach(),
                    feature=loss_feat.detach(), stft=stft.detach(), waveform=waveform.detach(),
                    grad_norm={k: opt[k].grad_norm() for k in OPT_KEYS}, codes=codes, timbre=timbre)
