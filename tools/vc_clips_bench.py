"""Voice conversion of clips of different lengths through the shipped (non-causal) redecoder on one GPU, one JSON line: the 32
seeded clips of tools/ragged_bench.py (1 - 3 s), encoded once by commons.encode_clips, then three legs on those codes,
  * batched:   commons.redecode_clips (sorted, grouped under the sample budget, padded batches with the per-clip edges written:
               34 fac_edge_tail launches and ragged_slack_frames of slack per group);
  * per_clip:  the same clips one at a time through redecoder.encoder -> redecoder.decoder at B = 1;
  * no_edge:   batched with ops.edge_tail_ turned into a no-op, on the same padded groups -- WRONG output, timed only to price
               the edge launches;
in the same process, alternating in a rotating order, HIP events around each pass (host work of the pass included: it ends in the event), median of
--reps passes after --warmup passes of each.  Also the grouping's padding share (slack included) and, per clip, how far batched
and per_clip are apart.
  python tools/vc_clips_bench.py [--reps 12] [--warmup 3] [--budget SAMPLES] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from facodec_amd import commons, ops, synth  # noqa: E402

N_CLIPS, SR, SEED, HOP = 32, 24000, 0, 300


def make_clips(dev):
    lengths = np.random.default_rng(SEED).integers(1 * SR, 3 * SR + 1, N_CLIPS)
    pool = synth.synth_clips(N_CLIPS, 3 * SR, seed=SEED)
    return [pool[i, :, :int(n)].contiguous().to(dev) for i, n in enumerate(lengths)], [int(n) for n in lengths]


def timed_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)        # a multiple of 3: every leg runs in every position equally often
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--budget", type=int, default=commons.MAX_BATCH_SAMPLES)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "vc_clips_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vc_clips_bench: no GPU (timings are taken on the device; there is no CPU path)")
    dev = torch.device("cuda:0")
    codec = commons.build_model(commons.default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(codec[k], seed=0, prefix=k + ".")
        codec[k].eval().to(dev)
    rm = commons.build_model(commons.default_redecoder_params(), stage="redecoder")
    for k in ("encoder", "decoder"):
        synth.load_synthetic(rm[k], seed=0, prefix="redecoder." + k + ".")
        rm[k].eval().to(dev)
    clips, lengths = make_clips(dev)
    enc = commons.encode_clips(codec, clips, n_c=2, max_batch_samples=args.budget)
    codes = [[c.contiguous() for c in e["codes"]] for e in enc]
    timbres = [e["timbre"] for e in enc]
    timbres = timbres[1:] + timbres[:1]                          # every clip with its neighbour's voice
    del codec, enc
    frames = [n // HOP for n in lengths]
    slack = commons.ragged_slack_frames(rm)
    padded_lengths = [HOP * (f + slack) for f in frames]
    groups = commons.plan_groups(padded_lengths, args.budget)
    padded = sum(len(g) * max(padded_lengths[i] for i in g) for g in groups)

    def batched():
        return commons.redecode_clips(rm, codes, timbres, max_batch_samples=args.budget)

    def per_clip():
        with torch.no_grad():
            return [rm.decoder(rm.encoder(c[0][None], c[1][None], t[None], use_p_code=False, n_c=1))[0] for c, t in zip(codes, timbres)]

    real_edge = ops.edge_tail_

    def no_edge():
        ops.edge_tail_ = lambda x, *a, **kw: x
        try:
            return batched()
        finally:
            ops.edge_tail_ = real_edge

    legs = dict(batched=batched, per_clip=per_clip, no_edge=no_edge)
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times, outs = {k: [] for k in legs}, {}
    names = list(legs)
    for r in range(args.reps):                 # alternating: all legs see the same box in the same minutes; the order rotates, so that
        for k in names[r % 3:] + names[:r % 3]:   # no leg always runs behind the same neighbour (allocator and cache state)
            ms, outs[k] = timed_ms(legs[k])
            times[k].append(ms)

    rel = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(outs["batched"], outs["per_clip"])]
    rel_no_edge = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(outs["no_edge"], outs["per_clip"])]
    audio_s = sum(HOP * f for f in frames) / SR
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = dict(device=torch.cuda.get_device_name(0), clips=N_CLIPS, audio_s=round(audio_s, 2), length_range_s=[1, 3], seed=SEED,
               budget_samples=args.budget, slack_frames=slack, edge_launches_per_group=len(commons.edge_plan(rm)),
               groups=[len(g) for g in groups], padding_share=round(1.0 - sum(HOP * f for f in frames) / padded, 4),
               batched_ms=round(med["batched"], 2), batched_ms_min_max=[round(min(times["batched"]), 2), round(max(times["batched"]), 2)],
               per_clip_ms=round(med["per_clip"], 2), per_clip_ms_min_max=[round(min(times["per_clip"]), 2), round(max(times["per_clip"]), 2)],
               no_edge_ms=round(med["no_edge"], 2), no_edge_ms_min_max=[round(min(times["no_edge"]), 2), round(max(times["no_edge"]), 2)],
               speedup=round(med["per_clip"] / med["batched"], 2), edge_overhead=round(med["batched"] / med["no_edge"] - 1.0, 4),
               batched_audio_s_per_s=round(audio_s / (med["batched"] / 1e3), 1),
               per_clip_audio_s_per_s=round(audio_s / (med["per_clip"] / 1e3), 1), reps=args.reps, warmup=args.warmup,
               wave_rel_max_batched_vs_per_clip=max(rel), wave_rel_max_no_edge_vs_per_clip=max(rel_no_edge))
    line = json.dumps(res)
    print(line)
    print("per clip, batched vs per_clip:", " ".join(f"{f}f:{r:.1e}" for f, r in zip(frames, rel)), file=sys.stderr)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
