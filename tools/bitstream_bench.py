#!/usr/bin/env python
"""What the bitstream costs and saves on one MI355X.

    python tools/bitstream_bench.py [--out profiles/bitstream_bench_mi355x.json]

  * ops.pack_codes / ops.unpack_codes at B = 32 x 160 frames (the benchmark batch) and B = 1 x 8 frames (one streaming period),
    (1, 2, 3) quantizers at 10 bits: HIP events around windows of back-to-back launches after a warm-up, the median window's
    microseconds per launch (these kernels run for less than the host takes to enqueue one: the figure is the cost of a launch in
    a stream of launches, which is what a caller pays), with the bytes each launch reads and writes.
  * the per-hop device-to-host traffic: bytes and host wall time (the copies end in a synchronise) of packing + one copy of the
    packed rows against the three int64 copies callers make today, median over many hops.
  * compressed size and bitrate of a 2 s clip for n_r = 0 .. 3 (commons.compress on the synthetic-weight model).
One JSON document; a run without a GPU fails."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facodec_amd import bitstream, commons, ops, synth  # noqa: E402

N_Q, BITS = (1, 2, 3), 10


def launch_us(fn, per_window=200, windows=25, warm=50):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per_window):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(1e3 * e0.elapsed_time(e1) / per_window)
    return dict(us_per_launch_median=round(statistics.median(us), 3), us_per_launch_min=round(min(us), 3),
                us_per_launch_max=round(max(us), 3), launches=per_window * windows)


def wall_us(fn, n=300, warm=30):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        t.append(1e6 * (time.perf_counter() - t0))
    t.sort()
    return dict(p50_us=round(t[len(t) // 2], 2), p99_us=round(t[int(0.99 * len(t))], 2), calls=n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "bitstream_bench_mi355x.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bitstream_bench needs a GPU: nothing here can be measured without one")
    dev = torch.device("cuda:0")
    doc = dict(device=torch.cuda.get_device_name(0), n_q=list(N_Q), bits=BITS, kernels=[], hop_traffic=[], clip_2s=[])
    gen = torch.Generator().manual_seed(0)
    for B, T in ((32, 160), (1, 8)):
        codes = [torch.randint(0, 1 << BITS, (B, n, T), generator=gen, dtype=torch.int64).to(dev) for n in N_Q]
        rb = ops.codes_row_bytes(T, sum(N_Q), BITS)
        packed = torch.empty(B, rb, dtype=torch.uint8, device=dev)
        outs = [torch.empty_like(c) for c in codes]
        ops.pack_codes(codes, bits=BITS, out=packed)
        back = ops.unpack_codes(packed, N_Q, T, bits=BITS, out=outs)
        assert all(torch.equal(x, y) for x, y in zip(back, codes))
        code_bytes = 8 * B * sum(N_Q) * T
        doc["kernels"].append(dict(B=B, frames=T, int64_bytes=code_bytes, packed_bytes=B * rb,
                                   pack=launch_us(lambda: ops.pack_codes(codes, bits=BITS, out=packed)),
                                   unpack=launch_us(lambda: ops.unpack_codes(packed, N_Q, T, bits=BITS, out=outs))))
        doc["hop_traffic"].append(dict(
            B=B, frames=T, packed_bytes=B * rb, int64_bytes=code_bytes,
            pack_and_one_copy=wall_us(lambda: ops.pack_codes(codes, bits=BITS, out=packed).cpu()),
            three_int64_copies=wall_us(lambda: [c.cpu() for c in codes])))
    model = commons.build_model(commons.default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(dev)
    wave = synth.synth_clips(1, 48000, seed=0).to(dev)
    for n_r in range(4):
        blob = commons.compress(model, wave, n_r=n_r)[0]
        hdr = bitstream.read(blob)[0]
        doc["clip_2s"].append(dict(n_r=n_r, n_q=list(hdr.n_q), frames=hdr.n_frames, blob_bytes=len(blob),
                                   payload_bytes=bitstream.payload_bytes(hdr.n_frames, hdr.Q, hdr.bits),
                                   blob_bytes_without_timbre=len(blob) - 4 * hdr.timbre_dim,
                                   payload_bit_per_s=bitstream.bitrate(hdr.n_q, hdr.bits),
                                   int64_codes_bit_per_s=64 * hdr.Q * 80))
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
