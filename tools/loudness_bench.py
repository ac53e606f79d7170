#!/usr/bin/env python
"""What the loudness meter and the level normalisation cost, on one MI355X.

    python tools/loudness_bench.py [--repeats 7] [--out file.json]

ops.loudness and ops.normalize_loudness at the benchmark batch (B = 32 x 2 s) and at one row of one hour, 24 kHz: HIP events
around back-to-back calls after a warm-up, `repeats` windows, median and range in microseconds -- next to the bytes the call
must move (loudness reads the input TWICE: the zero-state pass and the energy pass; normalize reads it THREE times and writes
it once) and that traffic's share of the 8 TB/s HBM peak.  The 32 x 2 s batch (6 MB) fits the Infinity Cache, so its rate is
no HBM figure; the hour (346 MB) does not fit.  The kernels of one ops.loudness call are timed one by one for the hour with
events around each C call split by hand (energies, then gate), and the serial scan is reported from the difference between
the hour and 64 rows of 1/64 hour, which run the same chunks with a 40 times shorter scan per row.
Then commons.compress of the benchmark batch with and without normalize_db, same process, alternating."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from elementwise_bench import timed  # noqa: E402
from facodec_amd import commons, ops, synth  # noqa: E402

HBM_PEAK = 8.0e12


def windows(fn, repeats, n):
    us = sorted(timed(fn, n=n, warm=2) for _ in range(repeats))
    return dict(us_median=round(statistics.median(us), 1), us_min=round(us[0], 1), us_max=round(us[-1], 1), calls_per_window=n, windows=repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    gen = torch.Generator(device="cpu").manual_seed(0)
    for name, B, T, n in (("32 x 2 s", 32, 48000, 50), ("64 x 56.25 s", 64, 1350000, 5), ("1 x 1 h", 1, 86400000, 5)):
        x = (0.1 * torch.randn(B, T, generator=gen)).to(dev)
        nbytes = 4 * B * T
        for op, fn, passes in (("ops.loudness", lambda: ops.loudness(x), 2), ("ops.normalize_loudness", lambda: ops.normalize_loudness(x, -16.0), 4)):
            t = windows(fn, a.repeats, n)
            moved = passes * nbytes
            emit(dict(op=op, shape=name, input_MB=round(nbytes / 1e6, 2), passes_over_the_input=passes, moved_MB=round(moved / 1e6, 2), **t,
                      TBps=round(moved / t["us_median"] / 1e6, 3), share_of_hbm_peak=round(moved / t["us_median"] * 1e6 / HBM_PEAK, 3),
                      audio_s_per_s=round(B * T / 24000 / t["us_median"] * 1e6)))
        en = ops.loudness_energies(x)
        t_e = windows(lambda: ops.loudness_energies(x), a.repeats, n)
        t_g = windows(lambda: ops.loudness_gate(en.e, T), a.repeats, n)
        L = ops.loudness_gate(en.e, T)
        t_n = windows(lambda: ops.loudness_gain(x, L, en.peak), a.repeats, n)
        emit(dict(op="parts", shape=name, kweight_energy=t_e, gate=t_g, gain=t_n, chunks_per_row=-(-T // ops.loudness_chunk()),
                  scan_steps_per_row=-(-T // (ops.loudness_chunk() * ops.loudness_chunk_group())),
                  gain_TBps=round(2 * nbytes / t_n["us_median"] / 1e6, 3)))
        del x, en
    hour = next(r for r in rows if r["op"] == "parts" and r["shape"] == "1 x 1 h")["kweight_energy"]["us_median"]
    wide = next(r for r in rows if r["op"] == "parts" and r["shape"] == "64 x 56.25 s")["kweight_energy"]["us_median"]
    emit(dict(op="serial scan at one hour", us_hour_one_row=hour, us_same_samples_in_64_rows=wide, difference_us=round(hour - wide, 1),
              note="the same chunks; one row hands its 5274 segment states across in 83 rounds of one wave, 64 rows in 2 rounds each, side by side"))

    model = commons.build_model(commons.default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(dev)
    wave = (0.3 * synth.synth_clips(32, 48000, seed=0)).to(dev)
    plain, levelled = [], []
    for _ in range(a.repeats):                                   # alternating, so that drift hits both alike
        plain.append(timed(lambda: commons.compress(model, wave), n=3, warm=1))
        levelled.append(timed(lambda: commons.compress(model, wave, normalize_db=-16.0), n=3, warm=1))
    emit(dict(op="commons.compress 32 x 2 s", plain_ms_median=round(statistics.median(plain) / 1e3, 3),
              plain_ms_range=[round(min(plain) / 1e3, 3), round(max(plain) / 1e3, 3)],
              normalize_db_ms_median=round(statistics.median(levelled) / 1e3, 3),
              normalize_db_ms_range=[round(min(levelled) / 1e3, 3), round(max(levelled) / 1e3, 3)],
              added_ms=round((statistics.median(levelled) - statistics.median(plain)) / 1e3, 3),
              added_share=round(statistics.median(levelled) / statistics.median(plain) - 1.0, 4)))
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
