#!/usr/bin/env python
"""What level control costs (facodec_amd.streaming.AutoGain, ops.level, ops.true_peak).

    python tools/agc_bench.py [--repeats 7] [--out profiles/agc_bench_mi355x.json]

HIP events around back-to-back calls after a warm-up (the method of tools/vad_bench.py), `repeats` windows, median and range in
microseconds per call:
  - AutoGain.push of one 480-sample hop at B = 1, 32 and 128, once on speech-level noise (the limiter idle) and once on noise
    far above the ceiling (the limiter at work on every tile); beside it, as context, VoiceActivity.push at the same B in the
    same process.  One push in five completes a sub-block and runs fac_agc_gains too.
  - ops.level on 1024 rows of 2 s (K-weighting, gains, apply), and fac_agc_apply alone on the same rows with the gains given;
  - ops.true_peak on the same rows.
No threshold anywhere: what was measured is recorded.  One JSON line on stdout, the same object in --out."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from elementwise_bench import timed  # noqa: E402
from facodec_amd import ops  # noqa: E402
from facodec_amd.streaming import HOP, AutoGain, VoiceActivity  # noqa: E402


def windows(fn, repeats, n, warm=2):
    us = sorted(timed(fn, n=n, warm=warm) for _ in range(repeats))
    return dict(us_median=round(statistics.median(us), 1), us_min=round(us[0], 1), us_max=round(us[-1], 1), calls_per_window=n, windows=repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "agc_bench_mi355x.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("agc_bench: no GPU; there is no CPU path and no number to report")
    dev = torch.device("cuda:0")
    rows = []

    def emit(row):
        rows.append(row)
        print("[agc_bench]", json.dumps(row), file=sys.stderr, flush=True)

    gen = torch.Generator(device="cpu").manual_seed(0)
    for B in (1, 32, 128):
        for what, rms in (("limiter idle", 0.05), ("limiter at work", 50.0)):
            agc = AutoGain(B, device=dev)
            hop = (rms * torch.randn(B, HOP, generator=gen)).to(dev)
            emit(dict(op="AutoGain.push", B=B, samples=HOP, signal=what, **windows(lambda: agc.push(hop), a.repeats, 200, warm=20)))
        va = VoiceActivity(B, device=dev)
        hop = (0.1 * torch.randn(B, HOP, generator=gen)).to(dev)
        emit(dict(op="VoiceActivity.push", B=B, samples=HOP, **windows(lambda: va.push(hop), a.repeats, 200, warm=20)))

    x = (0.05 * torch.randn(1024, 48000, generator=gen)).to(dev)
    mb = round(x.numel() * 4 / 1e6, 1)
    t = windows(lambda: ops.level(x), a.repeats, 10)
    emit(dict(op="ops.level", shape="1024 x 2 s", input_MB=mb, **t))
    p = ops.agc_params()
    g = ops.level(x).g.contiguous()
    t = windows(lambda: ops.agc_apply(x, g, p), a.repeats, 10)
    emit(dict(op="ops.agc_apply, gains given, limiter idle", shape="1024 x 2 s", input_MB=mb, **t,
              TBps=round(2 * x.numel() * 4 / t["us_median"] / 1e6, 3)))
    loud = x * 100.0
    t = windows(lambda: ops.agc_apply(loud, g, p), a.repeats, 10)
    emit(dict(op="ops.agc_apply, gains given, limiter at work on every tile", shape="1024 x 2 s", input_MB=mb, **t))
    del loud
    for quality in ("best", "fast"):
        t = windows(lambda: ops.true_peak(x, quality=quality), a.repeats, 10)
        emit(dict(op="ops.true_peak", quality=quality, shape="1024 x 2 s", input_MB=mb, **t))
        t = windows(lambda: ops.resample(x, 24000, 96000, quality=quality).abs().amax(-1), a.repeats, 10)
        emit(dict(op="ops.resample(x, 24000, 96000).abs().amax(-1)", quality=quality, shape="1024 x 2 s", input_MB=mb, **t))
    res = dict(metric="level control: time per call", device=torch.cuda.get_device_name(0), rows=rows)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
