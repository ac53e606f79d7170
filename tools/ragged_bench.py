"""Clips of different lengths on one GPU, one JSON line: 32 clips with seeded lengths uniform in 1 - 3 s,
  * batched:  commons.encode_clips + commons.decode_clips (sorted, grouped under the sample budget, zero-padded batches);
  * per_clip: the same clips one at a time through the existing calls (encoder -> quantizer(return_codes) -> decode_codes at B = 1);
both in the same process, alternating, HIP events around each pass (host work of the pass included: it ends in the event), median
of --reps passes after --warmup passes of each.  Also the grouping's padding share and how far the two paths' outputs are apart.
  python tools/ragged_bench.py [--reps 10] [--warmup 3] [--budget SAMPLES] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facodec_amd import commons, synth  # noqa: E402

N_CLIPS, SR, SEED = 32, 24000, 0


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--budget", type=int, default=commons.MAX_BATCH_SAMPLES)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ragged_bench: no GPU (timings are taken on the device; there is no CPU path)")
    dev = torch.device("cuda:0")
    model = commons.build_model(commons.default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(dev)
    clips, lengths = make_clips(dev)
    groups = commons.plan_groups(lengths, args.budget)

    def batched():
        enc = commons.encode_clips(model, clips, n_c=2, max_batch_samples=args.budget)
        return enc, commons.decode_clips(model, [e["codes"] for e in enc], [e["timbre"] for e in enc], max_batch_samples=args.budget)

    def per_clip():
        enc, waves = [], []
        with torch.no_grad():
            for w in clips:
                w = w.unsqueeze(0)
                _, _, _, _, timbre, codes = model.quantizer(model.encoder(w), w, n_c=2, return_codes=True)
                enc.append(dict(codes=[c[0] for c in codes], timbre=timbre[0]))
                waves.append(commons.decode_codes(model, codes, timbre)[0])
        return enc, waves

    for _ in range(args.warmup):
        batched()
        per_clip()
    torch.cuda.synchronize()
    t_b, t_p = [], []
    for _ in range(args.reps):                 # alternating: both see the same box in the same minutes
        ms, out_b = timed_ms(batched)
        t_b.append(ms)
        ms, out_p = timed_ms(per_clip)
        t_p.append(ms)

    # the two paths on the same clips: differing code positions (near-tie flips included) and the waves of the clips whose codes agree
    code_diff = sum(int((a != b).sum()) for eb, ep in zip(out_b[0], out_p[0]) for a, b in zip(eb["codes"], ep["codes"]))
    same = [i for i, (eb, ep) in enumerate(zip(out_b[0], out_p[0])) if all(torch.equal(a, b) for a, b in zip(eb["codes"], ep["codes"]))]
    wave_rel = max(float((out_b[1][i] - out_p[1][i]).abs().max() / out_p[1][i].abs().max()) for i in same) if same else None
    audio_s = sum(n // 300 * 300 for n in lengths) / SR
    med_b, med_p = float(np.median(t_b)), float(np.median(t_p))
    res = dict(device=torch.cuda.get_device_name(0), clips=N_CLIPS, audio_s=round(audio_s, 2), length_range_s=[1, 3], seed=SEED,
               budget_samples=args.budget, groups=[len(g) for g in groups], padding_share=round(commons.padding_share(lengths, groups), 4),
               batched_ms=round(med_b, 2), batched_ms_min_max=[round(min(t_b), 2), round(max(t_b), 2)],
               per_clip_ms=round(med_p, 2), per_clip_ms_min_max=[round(min(t_p), 2), round(max(t_p), 2)],
               speedup=round(med_p / med_b, 2), batched_audio_s_per_s=round(audio_s / (med_b / 1e3), 1),
               per_clip_audio_s_per_s=round(audio_s / (med_p / 1e3), 1), reps=args.reps, warmup=args.warmup,
               code_positions_differing=code_diff, code_positions=sum(6 * (n // 300) for n in lengths),
               clips_with_equal_codes=len(same), wave_rel_max_on_those=wave_rel)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
