#!/usr/bin/env python
"""What noise suppression costs (facodec_amd.streaming.NoiseSuppressor, ops.denoise).

    python tools/denoise_bench.py [--repeats 7] [--out profiles/denoise_bench_mi355x.json]

HIP events around back-to-back calls after a warm-up (the method of tools/agc_bench.py), `repeats` windows, median and range in
microseconds per call:
  - NoiseSuppressor.push of one 480-sample hop at B = 1, 32 and 128 (fifteen pushes in sixteen complete two frames, one a
    single frame);
  - ops.denoise on 1024 rows of 2 s, once with the synthesis transforming every frame again and once reading the spectra
    fac_ns_power kept in a workspace (keep_spectra=True; 16 bytes per frame and bin);
  - the three launches alone on the same rows: fac_ns_power (with and without writing the spectra), fac_ns_gains, fac_ns_synth
    (both forms);
  - the yardstick: the same algorithm written here with torch.stft / torch.istft in fp64 on the same device, in the same
    process (not part of the package), and how far its samples lie from ops.denoise's.
No threshold anywhere: what was measured is recorded.  One JSON line on stdout, the same object in --out."""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from elementwise_bench import timed  # noqa: E402
from facodec_amd import ops  # noqa: E402
from facodec_amd.streaming import HOP, NoiseSuppressor  # noqa: E402


def windows(fn, repeats, n, warm=2):
    us = sorted(timed(fn, n=n, warm=warm) for _ in range(repeats))
    return dict(us_median=round(statistics.median(us), 1), us_min=round(us[0], 1), us_max=round(us[-1], 1), calls_per_window=n, windows=repeats)


def torch_denoise(x, M=8, W=96, over=4.0, max_atten_db=15.0):
    """DESIGN.md 33.1 with torch.stft / torch.istft in fp64: x (B, T) float32 -> y (B, T) float32."""
    N, H = ops.NS_N, ops.NS_H
    B, T = x.shape
    n_f = ops.ns_frames(T)
    win = torch.sin(math.pi * torch.arange(N, device=x.device, dtype=torch.float64) / N)
    xp = F.pad(x.double(), (H, (n_f + 1) * H - T - H))                        # frame f is xp[f H : f H + 512]
    X = torch.stft(xp, N, H, N, window=win, center=False, return_complex=True)      # (B, 257, n_f)
    P = X.real * X.real + X.imag * X.imag
    c = F.pad(P.cumsum(-1), (M, 0))
    cnt = torch.arange(1, n_f + 1, device=x.device, dtype=torch.float64).clamp(max=M)
    S = (c[..., M:] - c[..., :-M]) / cnt
    Nf = -F.max_pool1d(F.pad(-S, (W - 1, 0), value=-math.inf), W, 1)
    xi = (S / (over * Nf) - 1.0).clamp(min=0.0)
    G = torch.where(Nf == 0.0, torch.ones_like(S), (xi / (1.0 + xi)).clamp(min=10.0 ** (-max_atten_db / 20.0)))
    # center=True only trims the first and last 256 samples of the overlap-add: the half frames in front of sample 0 and behind the end
    y = torch.istft(G * X, N, H, N, window=win, center=True, length=T)
    return y.float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "denoise_bench_mi355x.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("denoise_bench: no GPU; there is no CPU path and no number to report")
    dev = torch.device("cuda:0")
    rows = []

    def emit(row):
        rows.append(row)
        print("[denoise_bench]", json.dumps(row), file=sys.stderr, flush=True)

    gen = torch.Generator(device="cpu").manual_seed(0)
    for B in (1, 32, 128):
        ns = NoiseSuppressor(B, device=dev)
        hop = (0.05 * torch.randn(B, HOP, generator=gen)).to(dev)
        emit(dict(op="NoiseSuppressor.push", B=B, samples=HOP, **windows(lambda: ns.push(hop), a.repeats, 200, warm=20)))

    x = (0.05 * torch.randn(1024, 48000, generator=gen)).to(dev)
    mb = round(x.numel() * 4 / 1e6, 1)
    shape = "1024 x 2 s"
    emit(dict(op="ops.denoise, frames transformed again in synthesis", shape=shape, input_MB=mb, **windows(lambda: ops.denoise(x), a.repeats, 5)))
    emit(dict(op="ops.denoise, spectra kept in a workspace", shape=shape, input_MB=mb,
              **windows(lambda: ops.denoise(x, keep_spectra=True), a.repeats, 5)))
    p = ops.ns_params()
    n_f = ops.ns_frames(x.shape[1])
    P = torch.empty(1024, n_f, ops.NS_BINS, device=dev, dtype=torch.float64)
    X = torch.empty(1024, n_f, ops.NS_BINS, 2, device=dev, dtype=torch.float64)
    G = torch.empty_like(P)
    y = torch.empty_like(x)
    emit(dict(op="fac_ns_power", shape=shape, frames=n_f, **windows(lambda: ops.ns_power(x, P), a.repeats, 5)))
    emit(dict(op="fac_ns_power, spectra written", shape=shape, frames=n_f, **windows(lambda: ops.ns_power(x, P, X=X), a.repeats, 5)))
    emit(dict(op="fac_ns_gains", shape=shape, frames=n_f, **windows(lambda: ops.ns_gains(P, p, 0, n_f, G=G), a.repeats, 5)))
    emit(dict(op="fac_ns_synth, frames transformed again", shape=shape, frames=n_f, **windows(lambda: ops.ns_synth(x, G, out=y), a.repeats, 5)))
    emit(dict(op="fac_ns_synth, spectra read", shape=shape, frames=n_f, **windows(lambda: ops.ns_synth(x, G, X=X, out=y), a.repeats, 5)))
    del P, X, G
    ours = ops.denoise(x).y
    ref = torch_denoise(x)
    diff = float((ours - ref).abs().max()) / float(x.abs().max())
    del ours, ref
    emit(dict(op="torch.stft / torch.istft fp64 yardstick (this tool)", shape=shape, input_MB=mb, max_diff_of_peak=diff,
              **windows(lambda: torch_denoise(x), a.repeats, 3, warm=1)))
    res = dict(metric="noise suppression: time per call", device=torch.cuda.get_device_name(0), rows=rows)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
