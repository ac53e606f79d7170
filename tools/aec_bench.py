#!/usr/bin/env python
"""What echo cancellation costs (facodec_amd.streaming.EchoCanceller, ops.echo_cancel).

    python tools/aec_bench.py [--repeats 7] [--out profiles/aec_bench_mi355x.json]

HIP events around back-to-back calls after a warm-up (the method of tools/agc_bench.py), `repeats` windows, median and range in
microseconds per call:
  - EchoCanceller.push of one 480-sample hop at B = 1, 32 and 128, with P = 8 (W and the X ring in LDS for the call) and
    P = 32 (in global memory); fifteen pushes in sixteen complete two blocks, one a single block, so a push is 1.875 blocks;
  - ops.echo_cancel on 256 and 1024 rows of 2 s (188 blocks a row, one workgroup per row), P = 8 and 32;
  - for context only: NoiseSuppressor.push of the same hop on the same box.
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
from facodec_amd.streaming import HOP, EchoCanceller, NoiseSuppressor  # noqa: E402


def windows(fn, repeats, n, warm=2):
    us = sorted(timed(fn, n=n, warm=warm) for _ in range(repeats))
    return dict(us_median=round(statistics.median(us), 1), us_min=round(us[0], 1), us_max=round(us[-1], 1), calls_per_window=n, windows=repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "aec_bench_mi355x.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aec_bench: no GPU; there is no CPU path and no number to report")
    dev = torch.device("cuda:0")
    rows = []

    def emit(row):
        rows.append(row)
        print("[aec_bench]", json.dumps(row), file=sys.stderr, flush=True)

    gen = torch.Generator(device="cpu").manual_seed(0)
    for B in (1, 32, 128):
        far = (0.05 * torch.randn(B, HOP, generator=gen)).to(dev)
        mic = 0.5 * far.roll(7, dims=1) + (0.01 * torch.randn(B, HOP, generator=gen)).to(dev)
        for P in (8, 32):
            aec = EchoCanceller(B, P=P, device=dev)
            r = windows(lambda: aec.push(mic, far), a.repeats, 160, warm=16)
            emit(dict(op="EchoCanceller.push", B=B, P=P, samples=HOP, blocks_per_push=HOP / ops.AEC_H, **r,
                      us_per_block=round(r["us_median"] / (HOP / ops.AEC_H), 2)))
        ns = NoiseSuppressor(B, device=dev)
        emit(dict(op="NoiseSuppressor.push (context)", B=B, samples=HOP, **windows(lambda: ns.push(mic), a.repeats, 160, warm=16)))

    for n_rows in (256, 1024):
        far = (0.05 * torch.randn(n_rows, 48000, generator=gen)).to(dev)
        mic = 0.5 * far.roll(700, dims=1) + (0.01 * torch.randn(n_rows, 48000, generator=gen)).to(dev)
        for P in (8, 32):
            r = windows(lambda: ops.echo_cancel(mic, far, P=P), a.repeats, 3, warm=1)
            emit(dict(op="ops.echo_cancel", shape=f"{n_rows} x 2 s", P=P, blocks=ops.aec_blocks(48000), input_MB=round(2 * mic.numel() * 4 / 1e6, 1), **r,
                      us_per_block_of_a_row=round(r["us_median"] / ops.aec_blocks(48000), 2)))
    res = dict(metric="echo cancellation: time per call", device=torch.cuda.get_device_name(0), rows=rows)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
