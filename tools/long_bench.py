"""Recordings of any length on one GPU, one JSON line:
  * long_form: commons.encode_long + decode_long of one 10-minute B = 1 signal at chunks of 2, 10 and 30 s -> audio-s/s of the
    pair (host clock round work that ends in a device synchronise, after a warm-up on the first 3 chunks of the same size) and
    torch.cuda.max_memory_allocated of each run; the timbre (FAquantizer.timbre_long over all 48 000 frames) is timed alone;
  * attention: the two attention kernels alone, H = 2, dk = 256, B = 1: both routes at T = 2304 in this one process, the stream
    route at 24 000 and 96 000 frames -> ms per launch (HIP events) and TFLOP/s = 8 dk T^2 / time against the 157.3 TFLOP/s of
    the fp32 matrix pipe.
  python tools/long_bench.py [--minutes M] [--attention-only] [--out FILE]"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facodec_amd import commons, ops, synth  # noqa: E402
from facodec_amd.commons import build_model, default_model_params  # noqa: E402

SR = 24000
PEAK_TFLOPS = 157.3
H, DK = 2, 256


def events_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def attention_alone(dev):
    rows = []
    for T, kernels in ((2304, ("lds", "stream")), (24000, ("stream",)), (96000, ("stream",))):
        g = torch.Generator().manual_seed(T)
        q, k, v = (torch.randn(1, H * DK, T, generator=g).to(dev) for _ in range(3))
        flop = 8.0 * DK * T * T
        for kern in kernels:
            run = lambda: ops.attention(q, k, v, None, H, kernel=kern)          # noqa: E731
            run()
            torch.cuda.synchronize()
            n = 20 if T <= 2304 else 3 if T <= 24000 else 1
            ms = events_ms(run, n)
            tf = flop / ms / 1e9
            rows.append(dict(T=T, kernel=kern, ms=round(ms, 3), tflops=round(tf, 2), share_of_fp32_mfma_peak=round(tf / PEAK_TFLOPS, 3)))
            print(f"attention T={T} {kern}: {ms:.3f} ms, {tf:.1f} TFLOP/s", file=sys.stderr, flush=True)
        del q, k, v
    return rows


def main():
    minutes = float(sys.argv[sys.argv.index("--minutes") + 1]) if "--minutes" in sys.argv else 10.0
    dev = torch.device("cuda:0")
    model = build_model(default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(dev)
    T = int(minutes * 60 * SR)
    wave = synth.synth_clips(1, T, seed=0).to(dev)
    res = dict(device=torch.cuda.get_device_name(0), B=1, seconds=T / SR, frames=T // 300)

    res["attention"] = attention_alone(dev)
    if "--attention-only" in sys.argv:
        print(json.dumps(res))
        return

    q = model.quantizer
    q.timbre_long(wave[:, :, :SR * 40])                                          # warm-up: every kernel of the path, both mel chunk sizes
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t_timbre, timbre = wall(lambda: q.timbre_long(wave))
    res["timbre_long"] = dict(ms=round(1e3 * t_timbre, 1), peak_MiB=round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1))
    print(f"timbre_long: {res['timbre_long']}", file=sys.stderr, flush=True)

    rows = []
    for chunk in (2, 10, 30):
        head = wave[:, :, :min(T, 3 * chunk * SR + 3000)]
        warm = commons.encode_long(model, head, chunk_seconds=chunk, timbre=timbre)
        commons.decode_long(model, warm["codes"], timbre, chunk_seconds=chunk)
        del warm
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t_enc, enc = wall(lambda: commons.encode_long(model, wave, chunk_seconds=chunk, timbre=timbre))
        t_dec, y = wall(lambda: commons.decode_long(model, enc["codes"], timbre, chunk_seconds=chunk))
        peak = torch.cuda.max_memory_allocated() - base
        assert y.shape[-1] == 300 * (T // 300)
        rows.append(dict(chunk_seconds=chunk, encode_s=round(t_enc, 3), decode_s=round(t_dec, 3),
                         audio_s_per_s=round(T / SR / (t_enc + t_dec), 1), peak_MiB=round(peak / 2 ** 20, 1)))
        print(f"chunk {chunk} s: {rows[-1]}", file=sys.stderr, flush=True)
        del enc, y
    res["long_form"] = rows
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
