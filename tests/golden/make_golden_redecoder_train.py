"""Train-mode golden vectors of the voice-conversion redecoder from the REAL reference (build container only; the reference never
travels).

Run:  python tests/golden/make_golden_redecoder_train.py            (a few minutes on 8 cores)

What it does: builds the reference's frozen codec (`stage='encoder'`, modules/commons.py:414-439) and the redecoder
(`stage='redecoder'`, :385-413: Redecoder, non-causal LSTM-free Decoder, Discriminator) with the formula weights of
facodec_amd/synth.py (prefixes `encoder.*` for the codec, `redecoder.*` for the redecoder, `discriminator.*`), puts the redecoder in
.train() mode and executes the iteration of train_redecoder.py:195-328 (`encoder_type: wavenet`) on fixed inputs, with its random
sites replaced by recorded values:

  * np.random.randint      train_redecoder.py:206   (random crop start)
  * every nn.Dropout       p = 0                    (the WaveNet's 0.2)

Reference defect worked around here: train_redecoder.py:220-226 passes `torch.ones(B).bool()` twice as positional arguments before
`n_c`.  With `timbre_norm: True` FAquantizer.forward is forward_v2 (modules/quantize.py:236-237, :375), which has no such
parameters: the call as written raises `TypeError: got multiple values for argument 'n_c'`.  The flags are the old forward's
noise_added_flags / recon_noisy_flags (:303); the call below omits them.

Stored in redecoder_train.npz: the inputs, the frozen codec's codes and timbre (cross-check), every loss scalar, the three pre-clip
gradient norms, gradient probes (norm + strided slice; for the embedding tables: the rows the codes select) of ~30 generator tensors and ~8 discriminator tensors taken where
train_redecoder.py calls clip_grad_norm_ (:288, :321-322), discriminator parameter probes after its AdamW step, and the
parameters that receive no gradient.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402
from facodec_amd import synth  # noqa: E402

B, T_FULL = 4, 12000
WAVE_LENS = [12000, 6000, 10500, 12000]
MEL_LENS = [n // 300 for n in WAVE_LENS]     # 40, 20, 35, 40 frames: seg = min(min(MEL_LENS), 80) = 20
CROP_START = [3, 0, 7, 10]                   # np.random.randint(0, mel_length - seg) (0 where mel_length == seg)
GEN_PROBES = {
    "encoder": ["prosody_embed.0.weight", "content_embed.0.weight", "content_embed.1.weight",
                "encoder.cond_layer.conv.conv.weight_v", "encoder.cond_layer.conv.conv.weight_g", "encoder.cond_layer.conv.conv.bias",
                "encoder.in_layers.0.conv.conv.weight_v", "encoder.in_layers.0.conv.conv.weight_g", "encoder.in_layers.0.conv.conv.bias",
                "encoder.res_skip_layers.0.conv.conv.weight_v", "encoder.in_layers.15.conv.conv.weight_v",
                "encoder.in_layers.15.conv.conv.bias", "encoder.res_skip_layers.15.conv.conv.weight_v",
                "encoder.res_skip_layers.15.conv.conv.weight_g", "conv_out.weight", "conv_out.bias"],
    "decoder": ["model.0.conv.conv.weight_v", "model.0.conv.conv.bias", "model.1.block.0.alpha", "model.1.block.1.convtr.convtr.weight_v",
                "model.1.block.1.convtr.convtr.weight_g", "model.1.block.1.convtr.convtr.bias", "model.2.block.1.convtr.convtr.weight_v",
                "model.3.block.1.convtr.convtr.weight_v", "model.4.block.1.convtr.convtr.weight_v", "model.4.block.1.convtr.convtr.weight_g",
                "model.2.block.4.block.1.conv.conv.weight_v", "model.4.block.4.block.3.conv.conv.bias", "model.6.conv.conv.weight_v",
                "model.6.conv.conv.weight_g"],
}
DISC_PROBE_PREFIXES = ("discriminators.0.convs.0.", "discriminators.4.convs.3.0.weight_v", "discriminators.2.conv_post.",
                       "discriminators.5.band_convs.0.0.", "discriminators.7.band_convs.4.3.0.weight_g", "discriminators.6.conv_post.")


def probe_index(numel, n=64):
    step = max(1, numel // n)
    return np.arange(0, numel, step)[:n]


def grad_probes(module, key, names, rows=None):
    """Norm + strided slice of each gradient.  rows: {name: code rows} for the embedding tables, whose gradient is zero outside the
    rows the codes select (a strided slice would mostly read zeros): there the probe is every 64th channel of those rows."""
    out = {}
    params = dict(module.named_parameters())
    for n in names:
        g = params[n].grad
        flat = g.reshape(-1)
        out[f"grad.{key}.{n}.norm"] = np.float64(flat.double().norm())
        if rows is not None and n in rows:
            out[f"grad.{key}.{n}.probe_rows"] = rows[n]
            out[f"grad.{key}.{n}.probe"] = g[torch.from_numpy(rows[n])][:, ::64].reshape(-1).numpy().copy()
        else:
            out[f"grad.{key}.{n}.probe"] = flat[probe_index(flat.numel())].numpy().copy()
    return out


def redecoder_params():
    return dict(encoder_causal=True, decoder_causal=False, encoder_lstm=2, decoder_lstm=0, n_c_codebooks=2, n_p_codebooks=1,
                timbre_norm=True, separate_prosody_encoder=True, encoder_type="wavenet", wavenet_embed_dim=512, mamba_embed_dim=768,
                prob_random_mask_prosody=1.0, prob_random_mask_content=[0.0, 1.0],
                DAC=dict(encoder_dim=64, encoder_rates=[2, 5, 5, 6], decoder_dim=1536, decoder_rates=[6, 5, 5, 2], sr=24000))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(os.cpu_count())
    build_model, recursive_munch = MG.ref_imports()
    args = recursive_munch(redecoder_params())
    codec = build_model(args, stage="encoder")
    model = build_model(args, stage="redecoder")
    synth.load_synthetic(codec.encoder, seed=0, prefix="encoder.encoder.")
    synth.load_synthetic(codec.quantizer, seed=0, prefix="encoder.quantizer.")
    synth.load_synthetic(model.encoder, seed=0, prefix="redecoder.encoder.")
    synth.load_synthetic(model.decoder, seed=0, prefix="redecoder.decoder.")
    synth.load_synthetic(model.discriminator, seed=0, prefix="discriminator.")
    for k in codec:
        codec[k].eval()
    for k in model:
        model[k].train()
        for m in model[k].modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
    out = {}
    # ------------------------------------------------------------------ inputs and crop (train_redecoder.py:197-217)
    waves = synth.synth_clips(B, T_FULL, seed=29).squeeze(1)
    for b, n in enumerate(WAVE_LENS):
        waves[b, n:] = 0.0
    wave_lengths = torch.tensor(WAVE_LENS)
    seg = min(min(MEL_LENS), 80)
    wav_seg = torch.stack([waves[b, s * 300:(s + seg) * 300] for b, s in enumerate(CROP_START)]).float().unsqueeze(1)
    out.update(waves=waves.numpy(), wave_lens=np.array(WAVE_LENS), mel_input_length=np.array(MEL_LENS), crop_start=np.array(CROP_START),
               seg_frames=np.int64(seg))
    # ------------------------------------------------------------------ frozen codec (:219-227, without the two stray flags)
    with torch.no_grad():
        z = codec.encoder(wav_seg)
        _, _, _, _, timbre, codes = codec.quantizer(z, wav_seg, n_c=2, full_waves=waves, wave_lens=wave_lengths, return_codes=True)
    out.update(codes_p=codes[0].numpy().astype(np.int16), codes_c=codes[1].numpy().astype(np.int16),
               codes_r=codes[2].numpy().astype(np.int16), timbre=timbre.numpy())
    encoder_out = model.encoder(codes[0], codes[1], timbre)
    pred_wave = model.decoder(encoder_out)
    len_diff = wav_seg.size(-1) - pred_wave.size(-1)
    assert len_diff == 0, len_diff
    # ------------------------------------------------------------------ discriminator (:273-290)
    d_fake = model.discriminator(pred_wave.detach())
    d_real = model.discriminator(wav_seg)
    loss_d = 0
    for x_fake, x_real in zip(d_fake, d_real):
        loss_d += torch.mean(x_fake[-1] ** 2)
        loss_d += torch.mean((1 - x_real[-1]) ** 2)
    for k in model:
        model[k].zero_grad()
    loss_d.backward()
    disc_names = [n for n, _ in model.discriminator.named_parameters() if n.startswith(DISC_PROBE_PREFIXES)]
    out.update(grad_probes(model.discriminator, "discriminator", disc_names))
    out["grad_norm64_discriminator"] = np.float64(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in model.discriminator.parameters())))
    gn_d = torch.nn.utils.clip_grad_norm_(model.discriminator.parameters(), 10.0)
    opt_d = torch.optim.AdamW(model.discriminator.parameters(), lr=1e-4, betas=(0.9, 0.98), eps=1e-9, weight_decay=0.1)
    opt_d.step()
    out.update(loss_d=np.float64(loss_d.detach()), grad_norm_discriminator=np.float64(gn_d))
    pd = dict(model.discriminator.named_parameters())
    for n in disc_names[:4]:
        flat = pd[n].detach().reshape(-1)
        out[f"param_after.discriminator.{n}.probe"] = flat[probe_index(flat.numel())].numpy().copy()
    # ------------------------------------------------------------------ generator (:292-328)
    from audiotools import AudioSignal
    from dac.nn.loss import L1Loss, MelSpectrogramLoss, MultiScaleSTFTLoss
    mel_criterion = MelSpectrogramLoss(n_mels=[5, 10, 20, 40, 80, 160, 320], window_lengths=[32, 64, 128, 256, 512, 1024, 2048],
                                       mel_fmin=[0] * 7, mel_fmax=[None] * 7, pow=1.0, mag_weight=0.0, clamp_eps=1e-5)
    signal, recons = AudioSignal(wav_seg, sample_rate=24000), AudioSignal(pred_wave, sample_rate=24000)
    stft_loss = MultiScaleSTFTLoss()(recons, signal)
    mel_loss = mel_criterion(recons, signal)
    waveform_loss = L1Loss()(recons, signal)
    d_fake = model.discriminator(pred_wave)
    d_real = model.discriminator(wav_seg)
    loss_g = 0
    for x_fake in d_fake:
        loss_g += torch.mean((1 - x_fake[-1]) ** 2)
    loss_feature = 0
    for i in range(len(d_fake)):
        for j in range(len(d_fake[i]) - 1):
            loss_feature += F.l1_loss(d_fake[i][j], d_real[i][j].detach())
    loss_gen_all = mel_loss * 15.0 + loss_feature * 1.0 + loss_g * 1.0
    for k in model:
        model[k].zero_grad()
    loss_gen_all.backward()
    for k, names in GEN_PROBES.items():
        have = dict(model[k].named_parameters())
        missing = [n for n in names if n not in have]
        assert not missing, (k, missing, list(have)[:40])
        rows = {"prosody_embed.0.weight": np.unique(codes[0][:, 0].numpy()), "content_embed.0.weight": np.unique(codes[1][:, 0].numpy()),
                "content_embed.1.weight": np.unique(codes[1][:, 1].numpy())} if k == "encoder" else None
        out.update(grad_probes(model[k], k, names, rows))
    out["params_without_grad"] = np.array(json.dumps({k: [n for n, p in model[k].named_parameters() if p.grad is None]
                                                      for k in ("encoder", "decoder")}))
    for k in ("encoder", "decoder"):
        out[f"grad_norm64_{k}"] = np.float64(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in model[k].parameters() if p.grad is not None)))
    gn = {k: torch.nn.utils.clip_grad_norm_(model[k].parameters(), 1000.0) for k in ("encoder", "decoder")}
    scal = dict(loss_gen_all=loss_gen_all, mel_loss=mel_loss, stft_loss=stft_loss, waveform_loss=waveform_loss, loss_g=loss_g,
                loss_feature=loss_feature)
    out.update({k: np.float64(v.detach()) for k, v in scal.items()})
    out.update({f"grad_norm_{k}": np.float64(v) for k, v in gn.items()})
    out.update(pred_wave_probe=pred_wave.detach()[:, 0, ::13].numpy(), encoder_out_probe=encoder_out.detach()[:, ::8, :].numpy())
    np.savez_compressed(os.path.join(HERE, "redecoder_train.npz"), **out)
    print({k: float(v) for k, v in out.items() if isinstance(v, np.floating)})


if __name__ == "__main__":
    main()
