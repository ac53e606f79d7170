#!/usr/bin/env python
"""Redecoder training step timing (train_redecoder.py:195-328 at config_redecoder.yml: max_len 80 frames): ms per step at the
reference's batch (4 x 80 frames) and at 16 x 80, timed with device events after warm-up, no profiler.  FLOPs are counted from the
launch shapes of one extra, untimed step (ops.FlopCounter: GEMM-shaped work of the frozen codec's forward, the redecoder's forward
and backward and the discriminator's, STFT front-ends listed apart).  Synthetic weights and clips; one JSON line per batch size.

    python tools/redecoder_train_bench.py [--batches 4,16] [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facodec_amd import ops, synth  # noqa: E402
from facodec_amd.commons import build_model, default_redecoder_params  # noqa: E402
from facodec_amd.train_redecoder import RedecoderTrainStep  # noqa: E402

FRAMES_FULL = 120          # 3.6 s utterances: every clip longer than max_len, so the crop is 80 frames


def run(batch, steps, warmup, dev):
    args = default_redecoder_params()
    codec = build_model(args, stage="encoder")
    model = build_model(args, stage="redecoder", with_discriminator=True)
    for k, m in (("encoder.encoder", codec.encoder), ("encoder.quantizer", codec.quantizer), ("redecoder.encoder", model.encoder),
                 ("redecoder.decoder", model.decoder), ("discriminator", model.discriminator)):
        synth.load_synthetic(m, seed=0, prefix=k + ".")
        m.to(dev)
    step = RedecoderTrainStep(model, codec, model.discriminator)
    n = FRAMES_FULL * 300
    waves = synth.synth_clips(batch, n, seed=1).squeeze(1).to(dev)
    wave_lens = torch.full((batch,), n, dtype=torch.int64, device=dev)
    mel_lens = [FRAMES_FULL] * batch
    gen = torch.Generator().manual_seed(0)
    for _ in range(warmup):
        step(waves, wave_lens, mel_lens, generator=gen)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        out = step(waves, wave_lens, mel_lens, generator=gen)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    fc = ops.FlopCounter()
    ops.set_flop_counter(fc)
    try:
        step(waves, wave_lens, mel_lens, generator=gen)
        torch.cuda.synchronize()
    finally:
        ops.set_flop_counter(None)
    return dict(batch=batch, frames=80, steps=steps, warmup=warmup, ms_per_step=round(ms, 3), gflop_per_step=round(fc.total / 1e9, 2),
                tflops=round(fc.total / (ms * 1e-3) / 1e12, 2), flops_by_kind={k: round(v / 1e9, 2) for k, v in fc.flops.items()},
                loss_gen_all=float(out["loss_gen_all"]), loss_d=float(out["loss_d"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4,16")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for b in (int(v) for v in a.batches.split(",")):
        print(json.dumps(run(b, a.steps, a.warmup, dev)), flush=True)


if __name__ == "__main__":
    main()
