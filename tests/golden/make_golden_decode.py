"""Generates tests/golden/decode_from_codes.npz by importing the REAL reference from /root/reference (build container only --
the reference never travels to the GPU box).

Run:  python tests/golden/make_golden_decode.py            (about a minute on 8 cores)

Same import shims, model configuration and synthetic weights as make_golden.py (imported from it, not restated).  Input: the
codes and timbre of codec_e2e.npz (real config, 2 clips of 2 s).  For each RVQ the reference's own
ResidualVectorQuantize.from_codes (dac/nn/quantize.py:200-220), then the tail of FAquantizer.forward_v2
(modules/quantize.py:436-449, eval: res_mask = 1: timbre_linear, timbre_norm, * gamma + beta) and the reference decoder --
once with the fixture's timbre ("own") and once with the two clips' timbre rows swapped ("swap", timbre.flip(0): decoding
clip 0's codes with clip 1's speaker, FAcodec's zero-shot voice conversion).

Outputs (small): zq_{p,c,r}_probe (every 16th channel of the per-RVQ sums), zp_{p,c,r}_probe (the looked-up codebook rows,
every 2nd of 8N), outs_probe_{own,swap} (every 8th channel of the decoder input), wave_probe_{own,swap} (every 47th sample),
wave_absmax_{own,swap}.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (shims, model_params, the repository on sys.path)
from facodec_amd import synth  # noqa: E402


def main():
    torch.manual_seed(0)
    torch.set_num_threads(os.cpu_count())
    build_model, recursive_munch = G.ref_imports()
    d = np.load(os.path.join(HERE, "codec_e2e.npz"))
    codes = [torch.from_numpy(d[n].astype(np.int64)) for n in ("codes_p", "codes_c", "codes_r")]
    timbre = torch.from_numpy(d["timbre"])
    probe_t = d["probe_t"]
    out = dict(probe_t=probe_t)
    with torch.no_grad():
        model = build_model(recursive_munch(G.model_params()))
        for k in ("quantizer", "decoder"):
            model[k].eval()
            synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        q = model.quantizer
        z = {}
        for nm, rvq, c in (("p", q.prosody_quantizer, codes[0]), ("c", q.content_quantizer, codes[1]),
                           ("r", q.residual_quantizer, codes[2])):
            z_q, z_lat, _ = rvq.from_codes(c)
            z[nm] = z_q
            out[f"zq_{nm}_probe"] = z_q[:, ::16].numpy()
            out[f"zp_{nm}_probe"] = z_lat[:, ::2].numpy()
        for tag, tim in (("own", timbre), ("swap", timbre.flip(0))):
            outs = z["p"] + z["c"]                                    # modules/quantize.py:436-437 (res_mask = 1 in eval)
            outs = outs + z["r"] * torch.ones(outs.shape[0], 1, 1)
            style = q.timbre_linear(tim).unsqueeze(2)                 # :444-449
            gamma, beta = style.chunk(2, 1)
            outs = q.timbre_norm(outs.transpose(1, 2)).transpose(1, 2)
            outs = outs * gamma + beta
            y = model.decoder(outs)
            out[f"outs_probe_{tag}"] = outs[:, ::8].numpy()
            out[f"wave_probe_{tag}"] = y[:, 0, probe_t].numpy()
            out[f"wave_absmax_{tag}"] = np.float32(y.abs().max())
            print(tag, tuple(outs.shape), tuple(y.shape), float(y.abs().max()))
    np.savez_compressed(os.path.join(HERE, "decode_from_codes.npz"), **out)


if __name__ == "__main__":
    main()
