#!/usr/bin/env python
"""What finding the echo delay costs (facodec_amd.streaming.EchoDelayTracker, ops.echo_delay).

    python tools/echo_delay_bench.py [--repeats 7] [--out profiles/echo_delay_bench_mi355x.json]

HIP events around back-to-back calls after a warm-up (the method of tools/agc_bench.py), `repeats` windows, median and range in
microseconds per call:
  - EchoDelayTracker.push of one 480-sample hop at B = 1, 32 and 128, at the defaults (65 lags of 128 bins) and with
    max_delay = 2048 (9 lags); fifteen pushes in sixteen complete two frames, one a single frame, so a push is 1.875 frames;
  - next to it, in the same run: EchoCanceller.push (P = 8) of the same hop, and AlignedEchoCanceller.push, which is the two;
  - ops.echo_delay on 256 rows of 2 s (186 frames a row, one workgroup per row), and ops.echo_cancel on the same rows.
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
from facodec_amd.streaming import HOP, AlignedEchoCanceller, EchoCanceller, EchoDelayTracker  # noqa: E402


def windows(fn, repeats, n, warm=2):
    us = sorted(timed(fn, n=n, warm=warm) for _ in range(repeats))
    return dict(us_median=round(statistics.median(us), 1), us_min=round(us[0], 1), us_max=round(us[-1], 1), calls_per_window=n, windows=repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "echo_delay_bench_mi355x.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("echo_delay_bench: no GPU; there is no CPU path and no number to report")
    dev = torch.device("cuda:0")
    rows = []

    def emit(row):
        rows.append(row)
        print("[echo_delay_bench]", json.dumps(row), file=sys.stderr, flush=True)

    gen = torch.Generator(device="cpu").manual_seed(0)
    for B in (1, 32, 128):
        far = (0.05 * torch.randn(B, HOP, generator=gen)).to(dev)
        mic = 0.5 * far.roll(7, dims=1) + (0.01 * torch.randn(B, HOP, generator=gen)).to(dev)
        for max_delay in (16384, 2048):
            trk = EchoDelayTracker(B, max_delay=max_delay, device=dev)
            r = windows(lambda: trk.push(mic, far), a.repeats, 160, warm=16)
            emit(dict(op="EchoDelayTracker.push", B=B, max_delay=max_delay, lags=trk.p.L + 1, samples=HOP, frames_per_push=HOP / ops.AEC_H, **r,
                      us_per_frame=round(r["us_median"] / (HOP / ops.AEC_H), 2)))
        aec = EchoCanceller(B, P=8, device=dev)
        emit(dict(op="EchoCanceller.push", B=B, P=8, samples=HOP, **windows(lambda: aec.push(mic, far), a.repeats, 160, warm=16)))
        both = AlignedEchoCanceller(B, P=8, device=dev)
        emit(dict(op="AlignedEchoCanceller.push", B=B, P=8, max_delay=16384, samples=HOP, **windows(lambda: both.push(mic, far), a.repeats, 160, warm=16)))

    n_rows = 256
    far = (0.05 * torch.randn(n_rows, 48000, generator=gen)).to(dev)
    mic = 0.5 * far.roll(700, dims=1) + (0.01 * torch.randn(n_rows, 48000, generator=gen)).to(dev)
    r = windows(lambda: ops.echo_delay(mic, far), a.repeats, 3, warm=1)
    emit(dict(op="ops.echo_delay", shape=f"{n_rows} x 2 s", frames=ops.echo_delay_frames(48000), input_MB=round(2 * mic.numel() * 4 / 1e6, 1), **r,
              us_per_frame_of_a_row=round(r["us_median"] / ops.echo_delay_frames(48000), 2)))
    r = windows(lambda: ops.echo_cancel(mic, far, P=8), a.repeats, 3, warm=1)
    emit(dict(op="ops.echo_cancel", shape=f"{n_rows} x 2 s", P=8, blocks=ops.aec_blocks(48000), **r))
    res = dict(metric="echo delay: time per call", device=torch.cuda.get_device_name(0), rows=rows)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
