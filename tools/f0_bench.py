#!/usr/bin/env python
"""Time of the pitch extractor and of the predictor heads' mel-derived targets on one MI355X.

    python tools/f0_bench.py [--batch 16] [--frames 160] [--iters 30] [--warmup 5] [--out file.json]

Rows (one JSON line each): a `jdc.JDCNet` forward and a `targets.predictor_targets` call (the forward + the F0 normalisation + the
mel log-norm) on the training step's segment, batch x frames log-mel frames; the two target kernels alone.  Method: `warmup` untimed
calls, then `iters` calls each bracketed by its own pair of HIP events on the launch stream, one synchronise at the end; the median
is reported with the minimum and the maximum.  FLOPs are the algorithmic ones ops.FlopCounter books (gap columns, separator rows
and batch padding excluded), counted over one extra untimed call.  Compare with the training step of the same box:
`python tools/train_bench.py --predictors`."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facodec_amd import jdc, ops, synth, targets  # noqa: E402


def timed_ms(fn, iters, warmup):
    """[median, min, max] milliseconds per call of fn over `iters` event-bracketed calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in evs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
    return [round(ms[len(ms) // 2], 4), round(ms[0], 4), round(ms[-1], 4)]


def counted_flops(fn):
    c = ops.FlopCounter()
    ops.set_flop_counter(c)
    try:
        fn()
    finally:
        ops.set_flop_counter(None)
    torch.cuda.synchronize()
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("f0_bench: no GPU (a timing needs the device; there is no CPU path)")
    dev = torch.device("cuda:0")
    model = jdc.JDCNet(num_class=1, seq_len=192)
    model.load_state_dict(synth.synth_jdc_state_dict(0), strict=True)
    model.to(dev)
    mel = (3.0 * torch.rand(a.batch, 80, a.frames, generator=torch.Generator().manual_seed(0)) - 1.5).to(dev)
    x = mel.unsqueeze(1).contiguous()
    f0 = 60.0 + 300.0 * torch.rand(a.batch, a.frames, device=dev)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    shape = dict(batch=a.batch, frames=a.frames, iters=a.iters, warmup=a.warmup)
    c = counted_flops(lambda: model(x))
    ms = timed_ms(lambda: model(x), a.iters, a.warmup)
    emit(dict(op="JDCNet forward", **shape, ms_median_min_max=ms, algorithmic_GFLOP=round(c.total / 1e9, 2),
              GFLOP_by_key={k: round(v / 1e9, 3) for k, v in c.flops.items() if v}, launches=dict(c.launches),
              TFLOPs_at_median=round(c.total / ms[0] / 1e9, 1)))
    ms = timed_ms(lambda: targets.predictor_targets(model, mel), a.iters, a.warmup)
    emit(dict(op="predictor_targets (JDCNet + normalize_f0 + mel_log_norm)", **shape, ms_median_min_max=ms))
    emit(dict(op="normalize_f0", **shape, ms_median_min_max=timed_ms(lambda: targets.normalize_f0(f0), a.iters, a.warmup)))
    emit(dict(op="mel_log_norm", **shape, ms_median_min_max=timed_ms(lambda: targets.mel_log_norm(mel), a.iters, a.warmup)))
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
