#!/usr/bin/env python
"""Throughput of the device-side resampler (ops.resample) and what a ResampledSession adds to a streaming hop, on
one MI355X.

    python tools/resample_bench.py [--hops 500] [--out file.json]

Offline: the benchmark batch (B = 32 clips x 2 s) 48 k -> 24 k, 44.1 k -> 24 k and 24 k -> 48 k at both qualities, HIP events
around back-to-back launches (tools/elementwise_bench.py's `timed`): microseconds, algorithmic bytes (input read once + output
written once) per second, multiply-adds per second, the launch form (fac_resample_form) -- next to the rate of an elementwise
kernel of the same process (Snake forward on the step's largest activation, tools/elementwise_bench.py's row).
Streaming: p50 / p99 of a hop of a StreamingCodec wrapped at 48 kHz in and out against the bare session, same process, same
audio (host wall clock around push() incl. the device sync, tools/vc_stream_bench.py's method).  One JSON line per row."""
import argparse
import gc
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from elementwise_bench import timed  # noqa: E402
from facodec_amd import ops, synth  # noqa: E402
from facodec_amd.commons import build_model, default_model_params  # noqa: E402
from facodec_amd.streaming import HOP, ResampledSession, StreamingCodec  # noqa: E402

B, SECONDS = 32, 2


def hop_latencies(sess, wave, prime, hop, hops):
    with torch.no_grad():
        sess.prime(wave[:, :, :prime])
        torch.cuda.synchronize()
        lat, pos = [], prime
        gc.collect()
        gc.disable()
        try:
            for _ in range(hops):
                if pos + hop > wave.shape[-1]:
                    pos = 0
                blk = wave[:, :, pos:pos + hop]
                pos += hop
                t0 = time.perf_counter()
                sess.push(blk)
                torch.cuda.synchronize()
                lat.append(time.perf_counter() - t0)
        finally:
            gc.enable()
    lat.sort()
    return dict(hops=hops, p50_ms=round(1e3 * lat[len(lat) // 2], 4), p99_ms=round(1e3 * lat[min(len(lat) - 1, int(0.99 * len(lat)))], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hops", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    x = torch.randn(16, 192, 24000, device=dev)
    alpha = torch.rand(192, device=dev) + 0.5
    us = timed(lambda: ops.snake(x, alpha))
    emit(dict(op="Snake forward (elementwise reference)", shape=list(x.shape), algorithmic_MB=round(8 * x.numel() / 1e6, 2),
              us=round(us, 1), TBps=round(8 * x.numel() / us / 1e6, 3)))
    del x
    for rate_in, rate_out in ((48000, 24000), (44100, 24000), (24000, 48000)):
        for quality in ("best", "fast"):
            x = torch.randn(B, 1, SECONDS * rate_in, device=dev)
            geo, table, offs = ops._resample_device_table(rate_in, rate_out, quality, dev)
            y = ops.resample(x, rate_in, rate_out, quality=quality)
            form = ops.resample_form(ops.resample_desc(geo, table, offs, x.view(B, -1), y.view(B, -1), y.shape[-1]))
            us = timed(lambda: ops.resample(x, rate_in, rate_out, quality=quality))
            nbytes = 4 * (x.numel() + y.numel())
            emit(dict(op=f"resample {rate_in} -> {rate_out} {quality}", phases=geo["n"], taps=geo["taps"], table_KB=round(geo["table"].nbytes / 1024, 1),
                      form=form[0], tile=form[1], threads=form[2], lds_KB=round(form[3] / 1024, 1), grid=[form[4], B],
                      algorithmic_MB=round(nbytes / 1e6, 2), us=round(us, 1), TBps=round(nbytes / us / 1e6, 3),
                      Gmac_per_s=round(y.numel() * geo["taps"] / us / 1e3, 1), audio_s_per_s=round(B * SECONDS / us * 1e6)))
    model = build_model(default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(dev)
    timbre = torch.randn(1, 1024, device=dev)
    hops = a.hops - a.hops % 5
    w48 = synth.synth_clips(1, 48000 * 20, seed=0).to(dev)
    w24 = ops.resample(w48, 48000, 24000).contiguous()
    bare = hop_latencies(StreamingCodec(model, timbre), w24, 4800, HOP, hops)
    wrapped_sess = ResampledSession(StreamingCodec(model, timbre), in_rate=48000, out_rate=48000)
    wrapped = hop_latencies(wrapped_sess, w48, 9600, 2 * HOP, hops)
    emit(dict(op="StreamingCodec hop, B = 1", bare_24k=bare, wrapped_48k_in_out=wrapped,
              added_p50_ms=round(wrapped["p50_ms"] - bare["p50_ms"], 4),
              latency_in_ms=round(1e3 * wrapped_sess.latency_in, 3), latency_out_ms=round(1e3 * wrapped_sess.latency_out, 3)))
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
