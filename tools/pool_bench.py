#!/usr/bin/env python
"""How many calls one MI355X carries: per-tick time of a StreamPool (facodec_amd.streaming) with streams that join
and leave, next to a lockstep StreamingCodec of the same B = slots + 1 in the same process -- the path the pool is built on and
the baseline: what the pool adds is one scatter, the gathers, and a slot copy per join.

    python tools/pool_bench.py [--slots 1 8 32] [--ticks 500] [--windows 5] [--churn 10] [--out profiles/pool_bench_mi355x.json]

For every `slots`: a pool with every slot taken, synthetic audio resident in HBM, one leave and one join every `--churn` ticks
(so `slots` - 1 .. `slots` streams are live, up to one draining), and a StreamingCodec over B rows pushed (B, 1, 480) hops of the
same audio.  The `--ticks` ticks are timed in `--windows` windows that alternate between the two sessions (pool, lockstep, pool,
...), each tick twice over: HIP events around the tick (device time of its launches) and the host clock around the tick
including the device synchronise (what a 20 ms deadline sees).  Reported: p50 / p99 / max of both clocks for both sessions, the
pool's overhead (p50 over p50), fac_slot_copy alone (20 back-to-back launches between two events, bytes read + written), and the largest `slots` among those tried whose p99 wall tick stays under
20 ms.  One JSON line on stdout, the same object in --out."""
import argparse
import gc
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facodec_amd import synth  # noqa: E402
from facodec_amd.commons import build_model, default_model_params  # noqa: E402
from facodec_amd.streaming import HOP, StreamingCodec, StreamPool  # noqa: E402

TICK_MS = 1e3 * HOP / 24000


def quantiles(ms):
    s = sorted(ms)
    n = len(s)
    return dict(p50=round(s[n // 2], 4), p99=round(s[min(n - 1, int(0.99 * n))], 4), max=round(s[-1], 4))


class Timed:
    """Collects (HIP-event ms, wall ms) per call of step(); the events are read after the window's last synchronise."""

    def __init__(self):
        self.dev, self.wall, self._ev = [], [], []

    def step(self, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        self.wall.append(1e3 * (time.perf_counter() - t0))
        self._ev.append((e0, e1))

    def close_window(self):
        self.dev += [a.elapsed_time(b) for a, b in self._ev]
        self._ev = []

    def summary(self):
        return dict(ticks=len(self.wall), device_ms=quantiles(self.dev), wall_ms=quantiles(self.wall))


def bench_slots(model, slots, ticks, windows, churn, dev):
    B = slots + 1
    audio = synth.synth_clips(B, 24000 * 4, seed=slots).to(dev)               # 4 s per row, looped
    n_audio = audio.shape[-1] // HOP
    timbres = (0.5 * torch.randn(B, 1024, generator=torch.Generator().manual_seed(slots))).to(dev)
    pool = StreamPool(model, slots=slots, n_c=2, use_graphs=True)
    lock = StreamingCodec(model, timbres, n_c=2, use_graphs=True)
    with torch.no_grad():
        lock.prime(audio[:, :, :4800])
        for h in range(10):                                                    # both periods: eager, then captured
            lock.push(audio[:, :, h * HOP:(h + 1) * HOP])
    live = [pool.join(timbres[i + 1]) for i in range(slots)]
    state = dict(tick=0, joins=0)

    def pool_tick():
        t = state["tick"]
        state["tick"] += 1
        if churn and t % churn == churn - 1 and live:
            pool.leave(live.pop(0))                                            # the oldest stream leaves ...
        if len(live) < slots:
            try:
                live.append(pool.join(timbres[1 + t % slots]))                # ... and a new one joins as soon as its slot is free
                state["joins"] += 1
            except RuntimeError:
                pass                                                           # PoolFull: the leaver is still draining
        c = t % n_audio
        pool.tick(live, audio[:len(live), 0, c * HOP:(c + 1) * HOP])

    def lock_tick():
        c = state["tick"] % n_audio
        with torch.no_grad():
            lock.push(audio[:, :, c * HOP:(c + 1) * HOP])

    for _ in range(3 * max(churn, 5)):                                         # warm every path: leave, drain, join, new maps
        pool_tick()
        lock_tick()
    torch.cuda.synchronize()
    tp, tl = Timed(), Timed()
    per = ticks // windows
    state["joins"] = 0
    gc.collect()
    gc.disable()
    try:
        for _ in range(windows):
            for _ in range(per):
                tp.step(pool_tick)
            tp.close_window()
            for _ in range(per):
                tl.step(lock_tick)
            tl.close_window()
    finally:
        gc.enable()
    sp, sl = tp.summary(), tl.summary()
    copy = {}
    for n_dst in sorted({1, min(8, slots)}):                                   # the join's launch alone, after the timed run
        dsts = list(range(1, 1 + n_dst))
        for _ in range(3):
            pool.table.copy(0, dsts)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            pool.table.copy(0, dsts)
        e1.record()
        torch.cuda.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / 20
        copy[str(n_dst)] = dict(us=round(us, 2), gb_per_s=round(8 * pool.table.elems * n_dst / us / 1e3, 1))   # read + write
    return dict(slots=slots, B=B, state_mib_per_slot=round(pool.table.elems * 4 / 2 ** 20, 2), segments=pool.table.n_seg,
                tiles=pool.table.n_tiles, joins=state["joins"], pool=sp, lockstep=sl, slot_copy_by_destinations=copy,
                overhead_device_p50=round(sp["device_ms"]["p50"] / sl["device_ms"]["p50"], 4),
                overhead_wall_p50=round(sp["wall_ms"]["p50"] / sl["wall_ms"]["p50"], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--ticks", type=int, default=500)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--churn", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "pool_bench_mi355x.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pool_bench: no GPU; there is no CPU path and no number to report")
    dev = torch.device("cuda:0")
    model = build_model(default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(dev)
    rows = []
    for slots in a.slots:
        rows.append(bench_slots(model, slots, a.ticks, a.windows, a.churn, dev))
        print("[pool_bench]", json.dumps(rows[-1]), file=sys.stderr, flush=True)
        gc.collect()
        torch.cuda.empty_cache()
    fits = [r["slots"] for r in rows if r["pool"]["wall_ms"]["p99"] < TICK_MS]
    res = dict(metric="StreamPool per-tick time vs a lockstep StreamingCodec of the same B", device=torch.cuda.get_device_name(0),
               ticks=a.ticks, windows=a.windows, churn_every=a.churn, tick_budget_ms=TICK_MS, rows=rows,
               largest_slots_under_budget_p99_wall=max(fits) if fits else None)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
