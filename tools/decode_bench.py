"""Decoding from FA codes on one GPU, one JSON line:
  * vq_decode_kernel: fac_vq_decode alone at B = 32 clips x 160 frames (1 + 2 + 3 quantizers, D = 1024), HIP events over
    200 launches -> us per launch and the algorithmic traffic rate (outs written + codes read, B D T 4 + 6 B T 8 bytes);
  * offline: commons.decode_codes (codes + timbre -> wave) at bench.py's shape (32 clips x 2 s) in audio-s/s, next to the
    full encoder -> quantizer -> decoder forward of bench.py's step on the same clips;
  * streaming: StreamingDecoder (B = 1, graphs on) per-push wall time including a device sync, p50 / p99 over 300 pushes of
    k = 1 and of k = 2 frames (after the eager and capture pushes).
  python tools/decode_bench.py [--out FILE]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facodec_amd import ops, synth  # noqa: E402
from facodec_amd.commons import build_model, decode_codes, default_model_params  # noqa: E402
from facodec_amd.streaming import StreamingDecoder  # noqa: E402

B, SECONDS, SR = 32, 2.0, 24000


def events_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def wall_s(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    dev = torch.device("cuda:0")
    model = build_model(default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(dev)
    q = model.quantizer
    wave = synth.synth_clips(B, int(SECONDS * SR), seed=0).to(dev)
    with torch.no_grad():
        z = model.encoder(wave)
        _, _, _, _, timbre, codes = q(z, wave, n_c=2, return_codes=True)
    T = codes[0].shape[-1]
    res = dict(device=torch.cuda.get_device_name(0), B=B, T=T)

    # ---- kernel alone
    with torch.no_grad():
        style = q.timbre_linear(timbre).contiguous()
        weights = q.decode_weights()
    outs = torch.empty(B, 1024, T, device=dev)
    run = lambda: ops.vq_decode(codes, weights, style, 1024, out=outs)      # noqa: E731
    for _ in range(20):
        run()
    torch.cuda.synchronize()
    us = 1e3 * events_ms(run, 200)
    nbytes = B * 1024 * T * 4 + 6 * B * T * 8
    res["vq_decode_kernel"] = dict(us_per_launch=round(us, 2), GBps=round(nbytes / us / 1e3, 1), bytes=nbytes)

    # ---- offline decode vs full forward
    def fwd():
        with torch.no_grad():
            zz = model.encoder(wave)
            o, *_ = q(zz, wave, n_c=2, return_codes=True)
            return model.decoder(o)
    dec = lambda: decode_codes(model, codes, timbre)                    # noqa: E731
    t_dec = wall_s(dec, 10, 3)
    t_fwd = wall_s(fwd, 10, 3)
    audio = B * SECONDS
    res["offline"] = dict(decode_codes_ms=round(1e3 * t_dec, 2), decode_codes_audio_s_per_s=round(audio / t_dec, 1),
                          forward_ms=round(1e3 * t_fwd, 2), forward_audio_s_per_s=round(audio / t_fwd, 1))

    # ---- streaming receiver, one stream
    tim1 = timbre[:1].contiguous()
    c1 = [c[:1] for c in codes]
    stream = {}
    for k in (1, 2):
        rx = StreamingDecoder(model, tim1, use_graphs=True)
        rx.prime([c[:, :, :13] for c in c1])
        f, times = 13, []
        for i in range(310):
            if f + k > T:
                f = 13
            chunk = [c[:, :, f:f + k] for c in c1]
            f += k
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rx.push(chunk)
            torch.cuda.synchronize()
            if i >= 10:
                times.append(time.perf_counter() - t0)
        ms = 1e3 * np.array(times)
        stream[f"k{k}"] = dict(p50_ms=round(float(np.percentile(ms, 50)), 3), p99_ms=round(float(np.percentile(ms, 99)), 3),
                               audio_ms_per_push=12.5 * k, pushes=len(times))
    res["streaming_B1"] = stream
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
