#!/usr/bin/env python
"""Per-hop latency / real-time factor of a streaming voice-conversion session (facodec_amd.streaming.StreamingConverter) at
B = 1 on one MI355X: 24 kHz audio in 480-sample hops through the codec's encoder, prosody branch and content RVQ, then the
causal redecoder (16-layer timbre-conditioned WaveNet) and its decoder, with carried state and HIP-graph replay.

    python tools/vc_stream_bench.py [--seconds 60] [--decoder-lstm 2] [--no-graphs] [--use-p-code] [--n-c 1]

Prints one JSON line: p50 / p99 / p99.9 ms per hop (host wall clock around push() incl. the device sync) and RTF = processing
time / audio time of the conversion session, and -- same process, same signal, right after it -- of a StreamingCodec session
(encode -> quantize -> decode, tools/stream_bench.py's workload) for comparison: boxes differ by more than the two hops do.
Synthetic weights and audio (resident in HBM); the source's timbre comes from a 2 s enrolment clip, the target's from another.
"""
import argparse
import gc
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facodec_amd import synth  # noqa: E402
from facodec_amd.commons import build_model, default_model_params, default_redecoder_params  # noqa: E402
from facodec_amd.streaming import HOP, StreamingCodec, StreamingConverter  # noqa: E402


def timed_session(sess, wave, hops):
    """prime + `hops` pushes over `wave`, looped -> (sorted per-hop seconds, frames emitted, all outputs finite)."""
    frames, finite = 0, True
    with torch.no_grad():
        out = sess.prime(wave[:, :, :4800])
        frames += out["codes"][0].shape[-1]
        torch.cuda.synchronize()
        lat, pos = [], 4800
        gc_was_on = gc.isenabled()
        gc.collect()
        gc.disable()
        try:
            for h in range(hops):
                if pos + HOP > wave.shape[-1]:
                    pos = 0
                hop = wave[:, :, pos:pos + HOP]
                pos += HOP
                t0 = time.perf_counter()
                out = sess.push(hop)
                torch.cuda.synchronize()
                lat.append(time.perf_counter() - t0)
                assert out["frame0"] == frames, (out["frame0"], frames)
                frames += out["codes"][0].shape[-1]
                if h % 500 == 0:
                    finite = finite and bool(torch.isfinite(out["wave"]).all())
                if h % 5000 == 4999:
                    gc.collect()
        finally:
            if gc_was_on:
                gc.enable()
        finite = finite and bool(torch.isfinite(out["wave"]).all())
    return sorted(lat), frames, finite


def summary(lat, sample_rate=24000):
    n = len(lat)

    def q(p):
        return round(1e3 * lat[min(n - 1, int(p * n))], 4)
    return dict(hops=n, p50_ms=q(0.50), p99_ms=q(0.99), p999_ms=q(0.999), max_ms=round(1e3 * lat[-1], 4),
                rtf=round(sum(lat) / (n * HOP / sample_rate), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--decoder-lstm", type=int, default=2)
    ap.add_argument("--no-graphs", action="store_true")
    ap.add_argument("--use-p-code", action="store_true")
    ap.add_argument("--n-c", type=int, default=1)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    codec = build_model(default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(codec[k], seed=0, prefix=k + ".")
        codec[k].eval().to(dev)
    rargs = default_redecoder_params()
    rargs.decoder_causal, rargs.decoder_lstm = True, a.decoder_lstm
    red = build_model(rargs, stage="redecoder")
    for k in ("encoder", "decoder"):
        synth.load_synthetic(red[k], seed=0, prefix="redecoder." + k + ".")
        red[k].eval().to(dev)
    hops = int(a.seconds * 24000 // HOP)
    hops -= hops % 5
    wave = synth.synth_clips(1, min(24000 * 60, max(24000 * 20, 4800 + hops * HOP)), seed=0).to(dev)
    other = synth.synth_clips(1, 48000, seed=1).to(dev)
    with torch.no_grad():
        enrol = wave[:, :, :48000]
        source = codec.quantizer(codec.encoder(enrol), enrol, n_c=2)[4]
        target = codec.quantizer(codec.encoder(other), other, n_c=2)[4]
    vc = StreamingConverter(codec, red, target, source_timbre=source, use_p_code=a.use_p_code, n_c=a.n_c, use_graphs=not a.no_graphs)
    lat_vc, frames_vc, ok_vc = timed_session(vc, wave, hops)
    del vc
    lat_c, frames_c, ok_c = timed_session(StreamingCodec(codec, source, n_c=2, use_graphs=not a.no_graphs), wave, hops)
    want = (4800 + hops * HOP - 1024) // 300 + 1          # frames whose 1 024-sample look-ahead is complete
    ok = ok_vc and ok_c and frames_vc == frames_c == want
    print(json.dumps(dict(metric="streaming voice conversion per-hop latency / RTF", streams=1, graphs=not a.no_graphs,
                          decoder_lstm=a.decoder_lstm, use_p_code=a.use_p_code, n_c=a.n_c, converter=summary(lat_vc),
                          codec_same_process=summary(lat_c), frames=frames_vc, ok=ok)))
    if not ok:
        raise SystemExit("non-finite output or a wrong frame count")


if __name__ == "__main__":
    main()
