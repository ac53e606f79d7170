#!/usr/bin/env python
"""What scoring a batch of reconstructions costs, on one MI355X.

    python tools/metrics_bench.py [--repeats 7] [--out profiles/metrics_bench_mi355x.json]

B = 32, 256 and 1024 pairs of 2 s clips at 24 kHz: ops.si_sdr and ops.stoi_scores, HIP events around back-to-back calls after a
warm-up, `repeats` windows, median and range in microseconds.  The stages of one ops.stoi_scores call are then timed one by one
(the two ops.resample launches to 10 kHz, then fac_stoi_select, fac_stoi_bands and fac_stoi_score on one descriptor) next to
the bytes each must move once (its inputs read once, its outputs written once) and that traffic as a share of the 6.3 TB/s an
elementwise copy reaches on this chip: none of the stages is an elementwise kernel, the share says how far from a memory-bound
pass it is.  The 32-pair batch (12 MB) fits the Infinity Cache, so its rates are no HBM figures.
For context only, the fp64 numpy restatement of tests/test_metrics_cpu.py scores the first 32 pairs on 16 threads.
No threshold is set on any of these times.

Every step runs in a child process of its own under its own time limit; the parent never opens the GPU and stops at the first
step that fails or runs out of time."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
COPY_RATE = 6.3e12
STEPS = (("gpu", 32, 120), ("gpu", 256, 120), ("gpu", 1024, 180), ("numpy", 32, 300))
T24, T10 = 48000, 20000


def clips(B, seed=0):
    import torch
    gen = torch.Generator(device="cpu").manual_seed(seed)
    x = 0.1 * torch.randn(B, T24, generator=gen) * (1.0 + 0.8 * torch.sin(2.0 * torch.pi * 3.0 * torch.arange(T24) / 24000.0))
    y = x + 0.03 * torch.randn(B, T24, generator=gen)
    return x, y


def gpu_step(B, repeats):
    import torch
    sys.path.insert(0, HERE)
    sys.path.insert(0, REPO)
    from elementwise_bench import timed
    from facodec_amd import _lib, ops
    dev = torch.device("cuda:0")
    x, y = (t.to(dev) for t in clips(B))
    n = 20 if B <= 256 else 5

    def windows(fn):
        us = sorted(timed(fn, n=n, warm=2) for _ in range(repeats))
        return dict(us_median=round(statistics.median(us), 1), us_min=round(us[0], 1), us_max=round(us[-1], 1), calls_per_window=n, windows=repeats)

    def with_bytes(t, nbytes):
        return dict(t, moved_MB=round(nbytes / 1e6, 2), TBps=round(nbytes / t["us_median"] / 1e6, 3),
                    share_of_copy_rate=round(nbytes / t["us_median"] * 1e6 / COPY_RATE, 3))

    rows = []
    audio_s = B * T24 / 24000.0
    t = windows(lambda: ops.si_sdr(x, y))
    rows.append(dict(op="ops.si_sdr", B=B, seconds_of_audio=audio_s, **with_bytes(t, 3 * 2 * 4 * B * T24), passes_over_both_inputs=3,
                     audio_s_per_s=round(audio_s / t["us_median"] * 1e6)))
    t = windows(lambda: ops.stoi_scores(x, y, 24000))
    rows.append(dict(op="ops.stoi_scores at 24 kHz", B=B, seconds_of_audio=audio_s, **t, audio_s_per_s=round(audio_s / t["us_median"] * 1e6)))
    t = windows(lambda: (ops.resample(x, 24000, 10000), ops.resample(y, 24000, 10000)))
    stages = dict(resample_both=with_bytes(t, 2 * 4 * B * (T24 + T10)))
    x10, y10 = ops.resample(x, 24000, 10000), ops.resample(y, 24000, 10000)
    res, d, ws = ops._stoi_setup(x10, y10, None)
    lib, st = _lib.load(), ops._stream
    geo = ops.stoi_geometry(T10)
    M = geo.n_frames
    for name, fn, nbytes in (("fac_stoi_select", lib.fac_stoi_select, B * (4 * T10 + 8 * M + 4 * M)),
                             ("fac_stoi_bands", lib.fac_stoi_bands, B * (2 * 4 * T10 + 4 * M + 2 * 15 * 8 * M)),
                             ("fac_stoi_score", lib.fac_stoi_score, B * (2 * 15 * 8 * M + 2 * 8 * (M - 29)))):
        stages[name] = with_bytes(windows(lambda: _lib.check(fn(C.byref(d), st()), name)), nbytes)
    rows.append(dict(op="stages of ops.stoi_scores", B=B, frames_per_row=M, segments_per_row=M - 29, **stages,
                     kept_frames_mean=round(float(res.n_kept.double().mean()), 2), stoi_mean=round(float(res.stoi.mean()), 4),
                     estoi_mean=round(float(res.estoi.mean()), 4)))
    return rows


def numpy_step(B, threads=16):
    from concurrent.futures import ThreadPoolExecutor
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, REPO)
    import numpy as np
    from facodec_amd import dsp
    from test_metrics_cpu import si_sdr_ref, stoi_ref
    x, y = (t.numpy() for t in clips(B))
    geo = dsp.resample_table(24000, 10000, "best")
    # resampling is not part of the comparison: the restatement is fed 10 kHz rows picked from the 24 kHz ones by nearest
    # neighbour, which costs nothing, so that the scoring alone is timed
    idx = np.minimum((np.arange(T10) * geo["o"]) // geo["n"], T24 - 1)
    x10, y10 = x[:, idx], y[:, idx]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as ex:
        s = list(ex.map(lambda b: stoi_ref(x10[b], y10[b])[:2], range(B)))
    t1 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as ex:
        list(ex.map(lambda b: si_sdr_ref(x[b], y[b]), range(B)))
    t2 = time.perf_counter()
    return [dict(op="numpy fp64 restatement (context only)", B=B, threads=threads, stoi_ref_ms=round(1e3 * (t1 - t0), 1),
                 si_sdr_ref_ms=round(1e3 * (t2 - t1), 1), stoi_ref_ms_per_clip=round(1e3 * (t1 - t0) / B, 2), stoi_mean=round(float(np.mean([v[0] for v in s])), 4),
                 note="10 kHz rows by nearest-neighbour decimation, not the resampler: the scoring alone is timed")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="internal: kind:B of the one step this process runs")
    a = ap.parse_args()
    if a.step:
        kind, B = a.step.split(":")
        rows = gpu_step(int(B), a.repeats) if kind == "gpu" else numpy_step(int(B))
        print("ROWS " + json.dumps(rows), flush=True)
        return 0
    rows = []
    for kind, B, limit in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(a.repeats), "--step", f"{kind}:{B}"]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"step {kind}:{B} ran past its limit of {limit} s; stopping", file=sys.stderr)
            return 1
        if out.returncode != 0:
            print(f"step {kind}:{B} failed with status {out.returncode}; stopping\n{out.stderr[-2000:]}", file=sys.stderr)
            return 1
        got = [json.loads(line[5:]) for line in out.stdout.splitlines() if line.startswith("ROWS ")][0]
        for r in got:
            print(json.dumps(r), flush=True)
        rows += got
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
