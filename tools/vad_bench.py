#!/usr/bin/env python
"""What voice activity detection and discontinuous transmission cost and save (facodec_amd.streaming).

    python tools/vad_bench.py [--repeats 7] [--batch 8] [--out profiles/vad_bench_mi355x.json]

HIP events around back-to-back calls after a warm-up (the method of tools/loudness_bench.py and DESIGN.md 26), `repeats` windows,
median and range in microseconds per call:
  - VoiceActivity.push of one 480-sample hop at B = 1 and B = 32 (two launches; three pushes in five complete two frames);
  - ops.vad on 1024 rows of 2 s (two launches; 188 MB read once);
  - a StreamingReceiver tick with dtx off and on, same packets (all rows speaking: the dtx tick's extra work is the fac_sid_apply
    launch and B more staged words), each window 20 ticks of one session that goes on.
Then the packets and bytes of a scripted session of `--batch` streams in which every stream is silent for half of the pushes
(scripted flags, in runs of 25 pushes), with and without dtx=dict(sid_every=8).  No threshold anywhere: what was measured is
recorded.  One JSON line on stdout, the same object in --out."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from elementwise_bench import timed  # noqa: E402
from facodec_amd import bitstream, ops, synth  # noqa: E402
from facodec_amd.commons import build_model, default_model_params  # noqa: E402
from facodec_amd.streaming import HOP, CodePacketizer, StreamingCodec, StreamingReceiver, VoiceActivity  # noqa: E402

N_Q = (1, 2, 3)
SID_EVERY = 8
TICKS_PER_WINDOW = 20


def windows(fn, repeats, n, warm=2):
    us = sorted(timed(fn, n=n, warm=warm) for _ in range(repeats))
    return dict(us_median=round(statistics.median(us), 1), us_min=round(us[0], 1), us_max=round(us[-1], 1), calls_per_window=n, windows=repeats)


def send(model, B, n_push, dev):
    """One StreamingCodec session over B looped synthetic rows -> (timbre, the codes of n_push pushes)."""
    audio = synth.synth_clips(B, 24000 * 4, seed=B).to(dev)
    n_audio = (audio.shape[-1] - 4800) // HOP
    timbre = (0.5 * torch.randn(B, 1024, generator=torch.Generator().manual_seed(B))).to(dev)
    sess = StreamingCodec(model, timbre, n_c=2, use_graphs=True)
    chunks = []
    with torch.no_grad():
        out = sess.prime(audio[:, :, :4800])
        h = 0
        while True:
            if out["codes"] is not None:
                chunks.append([c.clone() for c in out["codes"]])
            if len(chunks) >= n_push:
                break
            c = h % n_audio
            out = sess.push(audio[:, :, 4800 + c * HOP:4800 + (c + 1) * HOP])
            h += 1
    return timbre, chunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "vad_bench_mi355x.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vad_bench: no GPU; there is no CPU path and no number to report")
    dev = torch.device("cuda:0")
    rows = []

    def emit(row):
        rows.append(row)
        print("[vad_bench]", json.dumps(row), file=sys.stderr, flush=True)

    gen = torch.Generator(device="cpu").manual_seed(0)
    for B in (1, 32):
        va = VoiceActivity(B, device=dev)
        hop = (0.1 * torch.randn(B, HOP, generator=gen)).to(dev)
        emit(dict(op="VoiceActivity.push", B=B, samples=HOP, **windows(lambda: va.push(hop), a.repeats, 200, warm=20)))
    x = (0.1 * torch.randn(1024, 48000, generator=gen)).to(dev)
    t = windows(lambda: ops.vad(x), a.repeats, 20)
    emit(dict(op="ops.vad", shape="1024 x 2 s", input_MB=round(x.numel() * 4 / 1e6, 1), **t, TBps=round(x.numel() * 4 / t["us_median"] / 1e6, 3)))
    del x

    model = build_model(default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(dev)
    B = a.batch
    warm = 20
    n_push = 1 + warm + a.repeats * TICKS_PER_WINDOW
    timbre, chunks = send(model, B, n_push, dev)
    plain = CodePacketizer(N_Q)
    headers = plain.header(timbre)
    full = [plain.packet(c) for c in chunks]
    for dtx in (False, True):
        rx = StreamingReceiver(model, headers, dtx=dtx)
        rx.prime(full[0])
        j = [1]

        def tick():
            rx.tick(full[j[0]])
            j[0] += 1
        for _ in range(warm):
            tick()
        emit(dict(op="StreamingReceiver.tick", B=B, dtx=dtx, **windows(tick, a.repeats, TICKS_PER_WINDOW, warm=0)))

    # every stream silent for half of the pushes, in runs of 25, the streams out of step
    tx = CodePacketizer(N_Q, dtx=dict(sid_every=SID_EVERY))
    ref = CodePacketizer(N_Q)
    count = dict(dtx=[0, 0, 0], plain=[0, 0])                               # normal, SID, bytes / packets, bytes
    for i, c in enumerate(chunks):
        k = c[0].shape[-1]
        speaking = torch.tensor([((i + 25 * b) // 25) % 2 == 0 for b in range(B)], dtype=torch.uint8)
        active = ops.h2d(speaking[:, None].expand(B, k).contiguous(), dev)
        for p in tx.packet(c, active):
            if p is not None:
                count["dtx"][0 if p[:2] == bitstream.PACKET_MAGIC else 1] += 1
                count["dtx"][2] += len(p)
        for p in ref.packet(c):
            count["plain"][0] += 1
            count["plain"][1] += len(p)
    emit(dict(op="scripted session, half of every stream silent", B=B, pushes=len(chunks), sid_every=SID_EVERY,
              plain=dict(packets=count["plain"][0], bytes=count["plain"][1]),
              dtx=dict(packets=count["dtx"][0] + count["dtx"][1], sid_packets=count["dtx"][1], bytes=count["dtx"][2]),
              bytes_ratio=round(count["dtx"][2] / count["plain"][1], 4),
              derived_payload_rate_bps=dict(plain=bitstream.bitrate(N_Q, 10), dtx=bitstream.bitrate(N_Q, 10, dtx_silence=0.5, sid_every=SID_EVERY))))
    res = dict(metric="voice activity detection and discontinuous transmission: time per call, packets and bytes sent",
               device=torch.cuda.get_device_name(0), rows=rows)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
