"""Generates tests/golden/redecoder_causal.npz by importing the REAL reference (build container only, as make_golden.py, whose
import shims and helpers are used): the voice-conversion path of reconstruct_redecoder.py:110-122 in the configuration a live
conversion needs -- stage 'redecoder' with decoder_causal=True, decoder_lstm=2 -- which tests/golden/redecoder.npz (the shipped
non-causal config_redecoder.yml) does not pin.

Run:  python tests/golden/make_golden_redecoder_causal.py            (well under a minute)

Inputs: the codes and the timbre of the two 2 s clips synth_clips(2, 48000, seed=0), read from codec_e2e.npz -- they are the real
reference's own outputs (make_golden.py section 4), and the HIP path reproduces those codes bit for bit
(tests/test_gpu_parity.py).  The timbre is flipped between the clips ("target speaker" = the other clip) and the call is
use_p_code=False, n_c=1, as in make_golden.py's non-causal block.  Weights: synth.load_synthetic, seed 0.

Output (data only): z_probe (every 8th channel of the redecoder's latent), wave_probe at probe_t, wave_absmax -- the probes of
redecoder.npz -- and the relative errors of the oracle's redecoder_forward(causal=True) / decoder_forward(causal=True, lstm=2)
against the reference on the same inputs.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import O, ref_imports, rel_err, synth  # noqa: E402


def causal_redecoder_params():
    """configs/config_redecoder.yml:28-48 `model_params` with the two switches of a live conversion."""
    return dict(encoder_causal=True, decoder_causal=True, encoder_lstm=2, decoder_lstm=2, n_c_codebooks=2, n_p_codebooks=1,
                timbre_norm=True, separate_prosody_encoder=True, encoder_type="wavenet", wavenet_embed_dim=512, mamba_embed_dim=768,
                prob_random_mask_prosody=1.0, prob_random_mask_content=[0.0, 1.0],
                DAC=dict(encoder_dim=64, encoder_rates=[2, 5, 5, 6], decoder_dim=1536, decoder_rates=[6, 5, 5, 2], sr=24000))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(os.cpu_count())
    build_model, recursive_munch = ref_imports()
    e2e = np.load(os.path.join(HERE, "codec_e2e.npz"))
    codes_p = torch.from_numpy(e2e["codes_p"].astype(np.int64))
    codes_c = torch.from_numpy(e2e["codes_c"].astype(np.int64))
    timbre_tgt = torch.from_numpy(e2e["timbre"]).flip(0)          # "target speaker" = the other clip's timbre
    with torch.no_grad():
        rmodel = build_model(recursive_munch(causal_redecoder_params()), stage="redecoder")
        for k in ("encoder", "decoder"):
            rmodel[k].eval()
        sd_re = synth.load_synthetic(rmodel.encoder, seed=0, prefix="redecoder.encoder.")
        sd_rd = synth.load_synthetic(rmodel.decoder, seed=0, prefix="redecoder.decoder.")
        zr = rmodel.encoder(codes_p, codes_c, timbre_tgt, use_p_code=False, n_c=1)
        yr = rmodel.decoder(zr)
        o_zr = O.redecoder_forward(sd_re, codes_p, codes_c, timbre_tgt, use_p_code=False, n_c=1, causal=True)
        o_yr = O.decoder_forward(sd_rd, zr, causal=True, lstm=2)
    assert zr.shape == (2, 1024, 160) and yr.shape == (2, 1, 48000)
    probe_t = np.arange(0, 48000, 47)
    report = dict(redecoder_causal_oracle_rel=rel_err(o_zr, zr), redecoder_causal_decoder_oracle_rel=rel_err(o_yr, yr))
    np.savez_compressed(os.path.join(HERE, "redecoder_causal.npz"), z_probe=zr[:, ::8, :].numpy(),
                        wave_probe=yr[:, 0, probe_t].numpy(), probe_t=probe_t, wave_absmax=np.float32(yr.abs().max()),
                        **{k: np.float64(v) for k, v in report.items()})
    print(report)


if __name__ == "__main__":
    main()
