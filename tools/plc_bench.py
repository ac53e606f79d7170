#!/usr/bin/env python
"""What surviving packet loss costs per tick: StreamingReceiver (facodec_amd.streaming) at 0 %, 5 % and 20 % seeded
per-stream packet loss with delay 0 and 1, next to the CodeDepacketizer + StreamingDecoder pair on the lossless stream in the same
process.

    python tools/plc_bench.py [--batch 1 32] [--ticks 300] [--warm 30] [--out profiles/plc_bench_mi355x.json]

For every B one StreamingCodec session over B rows of synthetic audio is sent once, as plain packets and as packets with the
(1, 2, 0) redundant layer; the bytes stay on the host.  The six receivers and the lossless pair then walk the same packets in
lockstep: at tick j each of the seven sessions plays its tick j, one after the other, each timed on its own -- HIP events around
the tick (device time of its launches) and the host clock around the tick including the device synchronise.  So every session
sees the same neighbours on the machine.  Reported per session: p50 / p99 of both clocks over the `--ticks` ticks after
`--warm` warm-up ticks (every graph of the 5-hop period is captured by then), the launches a tick makes outside its captured
graph (counted by wrapping the ops entry points: the copy to the device, unpack, select, gain; the pair's three code copies are
torch kernels and are stated, not counted), and the loss statistics.  Informational only, no threshold: the median over the
streams of the whole session's SI-SDR (ops.si_sdr) against the lossless pair's output -- with delay 0 every lost push is
concealed, with delay 1 a lost push is recovered at (1, 2, 0) unless its successor is lost too.  The weights are synthetic: the
SI-SDR figures say how far the substituted frames are from the lossless ones, not how anything sounds.  One JSON line on stdout,
the same object in --out."""
import argparse
import gc
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facodec_amd import ops, synth  # noqa: E402
from facodec_amd.commons import build_model, default_model_params  # noqa: E402
from facodec_amd.streaming import (HOP, CodeDepacketizer, CodePacketizer, StreamingCodec, StreamingDecoder,  # noqa: E402
                                   StreamingReceiver)

N_Q, N_RED = (1, 2, 3), (1, 2, 0)
LOSSES = (0.0, 0.05, 0.20)
COUNTED = ("h2d", "unpack_codes", "plc_select", "plc_gain")


def quantiles(ms):
    s = sorted(ms)
    n = len(s)
    return dict(p50=round(s[n // 2], 4), p99=round(s[min(n - 1, int(0.99 * n))], 4), max=round(s[-1], 4))


class Session:
    """One receiver under the clock: tick(j) -> wave or None; device and wall time and the counted launches per timed tick."""

    def __init__(self, name, tick):
        self.name, self.tick = name, tick
        self.dev, self.wall, self.calls, self._ev, self.waves = [], [], [], [], {}

    def step(self, j, timed, counter):
        before = sum(counter.values())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        w = self.tick(j)
        e1.record()
        torch.cuda.synchronize()
        if timed:
            self.wall.append(1e3 * (time.perf_counter() - t0))
            self._ev.append((e0, e1))
            self.calls.append(sum(counter.values()) - before)
        return w

    def summary(self):
        self.dev += [a.elapsed_time(b) for a, b in self._ev]
        self._ev = []
        return dict(ticks=len(self.wall), device_ms=quantiles(self.dev), wall_ms=quantiles(self.wall),
                    launches_outside_graph_mean=round(sum(self.calls) / max(len(self.calls), 1), 3))


def send(model, B, n_push, dev):
    """-> (headers, plain packets per push, packets with the redundant layer per push)."""
    audio = synth.synth_clips(B, 24000 * 4, seed=B).to(dev)                    # 4 s per row, looped
    n_audio = (audio.shape[-1] - 4800) // HOP
    timbre = (0.5 * torch.randn(B, 1024, generator=torch.Generator().manual_seed(B))).to(dev)
    tx, tq = CodePacketizer(N_Q), CodePacketizer(N_Q, redundancy=N_RED)
    sess = StreamingCodec(model, timbre, n_c=2, use_graphs=True)
    fp, fq = [], []
    with torch.no_grad():
        out = sess.prime(audio[:, :, :4800])
        h = 0
        while True:
            if out["codes"] is not None:
                fp.append(tx.packet(out["codes"]))
                fq.append(tq.packet(out["codes"]))
            if len(fp) >= n_push:
                break
            c = h % n_audio
            out = sess.push(audio[:, :, 4800 + c * HOP:4800 + (c + 1) * HOP])
            h += 1
    return tx.header(timbre), fp, fq


def _median_db(x):
    x = sorted(float(v) for v in x)
    m = x[len(x) // 2]
    return round(m, 2) if math.isfinite(m) else repr(m)


def bench_batch(model, B, ticks, warm, dev):
    n_push = 1 + warm + ticks + 1                                              # prime, warm-up, timed, one more for delay=1
    headers, fp, fq = send(model, B, n_push, dev)
    counter = {n: 0 for n in COUNTED}
    originals = {n: getattr(ops, n) for n in COUNTED}

    def counted(name):
        def f(*a, **kw):
            counter[name] += 1
            return originals[name](*a, **kw)
        return f
    for n in COUNTED:
        setattr(ops, n, counted(n))
    try:
        rng = np.random.default_rng(B)
        sessions, receivers = [], {}
        rxc = CodeDepacketizer(headers)
        pair = StreamingDecoder(model, rxc.timbre)
        ref = [pair.prime(rxc.feed(fp[0])).clone()]
        sessions.append(Session("lossless_pair", lambda j: pair.push(rxc.feed(fp[j]))))
        for delay in (0, 1):
            for loss in LOSSES:
                rx = StreamingReceiver(model, headers, delay=delay)
                src = fq if delay else fp
                rx.prime(src[0])
                drop = rng.random((n_push, B)) < loss

                def tick(j, rx=rx, src=src, drop=drop, delay=delay):
                    k = int.from_bytes(src[j - delay][0][4:6], "little")       # n_frames of the push this tick plays
                    return rx.tick([None if drop[j, b] else p for b, p in enumerate(src[j])], k=k)
                name = f"receiver_delay{delay}_loss{int(100 * loss)}"
                receivers[name] = (rx, delay)
                sessions.append(Session(name, tick))
        gc.collect()
        gc.disable()
        try:
            for j in range(1, n_push):
                for s in sessions:
                    w = s.step(j, j > warm and len(s.wall) < ticks, counter)
                    if s.name == "lossless_pair":
                        ref.append(w.clone())
                    elif w is not None:
                        s.waves[j - receivers[s.name][1]] = w.clone()          # delay=1: tick j played push j - 1
        finally:
            gc.enable()
    finally:
        for n in COUNTED:
            setattr(ops, n, originals[n])
    rows = {}
    for s in sessions:
        row = s.summary()
        if s.name in receivers:
            rx, delay = receivers[s.name]
            pushes = sorted(s.waves)
            est = torch.cat([s.waves[j] for j in pushes], -1)[:, 0]
            want = torch.cat([ref[j] for j in pushes], -1)[:, 0]
            st = rx.stats
            row.update(si_sdr_db_vs_lossless_median=_median_db(ops.si_sdr(want.contiguous(), est.contiguous()).cpu().tolist()),
                       packets_received=sum(d["received"] for d in st), frames_recovered=sum(d["recovered"] for d in st),
                       frames_concealed=sum(d["concealed"] for d in st), frames_played=est.shape[-1] // 300 * B)
        else:
            row.update(launches_outside_graph_note="counted: the copy to the device and unpack; plus three torch copies of the codes "
                                                   "into the decoder's static buffers")
        rows[s.name] = row
    base = rows["lossless_pair"]
    for name in receivers:
        rows[name]["device_p50_over_pair"] = round(rows[name]["device_ms"]["p50"] / base["device_ms"]["p50"], 4)
        rows[name]["wall_p50_over_pair"] = round(rows[name]["wall_ms"]["p50"] / base["wall_ms"]["p50"], 4)
    return dict(B=B, sessions=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--warm", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "plc_bench_mi355x.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plc_bench: no GPU; there is no CPU path and no number to report")
    dev = torch.device("cuda:0")
    model = build_model(default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(dev)
    rows = []
    for B in a.batch:
        rows.append(bench_batch(model, B, a.ticks, a.warm, dev))
        print("[plc_bench]", json.dumps(rows[-1]), file=sys.stderr, flush=True)
        gc.collect()
        torch.cuda.empty_cache()
    res = dict(metric="StreamingReceiver per-tick time under packet loss vs CodeDepacketizer + StreamingDecoder on the lossless stream",
               device=torch.cuda.get_device_name(0), ticks=a.ticks, warm=a.warm, n_q=N_Q, redundancy=N_RED,
               policy=dict(hold=2, fade=6, recover=1), tick_ms=1e3 * HOP / 24000, rows=rows)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
