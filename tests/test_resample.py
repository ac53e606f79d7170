"""The device-side polyphase resampler on the GPU: fac_resample against the definition in float64, a padded batch
against its rows alone, StreamingResampler against the offline call, and the clip-list calls and streaming sessions that take
and give audio at other rates than 24 kHz.

The float64 reference is the defining sum written out here from the formula (window, sinc, the |t| < W support); it does not use
the product's coefficient table.  The bound is derived, not measured: a coefficient rounded once to fp32, one rounding per
product and per addition of at most `taps` terms give |y - y64| <= (taps + 2) 2^-24 sum_q |h| |x[q]| to first order.  Everything
else is an equality of bits: the kernel adds an output's taps in an order that depends on the output's phase alone.
"""
import math

import numpy as np
import pytest
import torch

from facodec_amd import commons, synth

gpu = pytest.mark.gpu

QUALITIES = {"best": (64, 0.9475937167399596, 14.769656459379492), "fast": (16, 0.85, 8.555504641634386)}
# the issue's pairs (11 025 -> 24 000: the table that does not fit LDS, read from global memory) and 640 -> 1, where not even the
# input span of a tile fits and the kernel reads inputs from global memory too: every form of the kernel is launched
KERNEL_PAIRS = [(48000, 24000), (44100, 24000), (24000, 44100), (16000, 24000), (24000, 16000), (11025, 24000), (640, 1)]
FORMS = {(11025, 24000, "best"): 1, (640, 1, "best"): 2, (640, 1, "fast"): 2}       # every other case: 0, table and span in LDS
LENS = (1, 137, 4801)           # two rows shorter than the filter, one ending off a tile edge
LONG = 20011                    # one row over several workgroup tiles, ending off a tile edge
FILL = 1e30                     # what sits behind lens[b]: read once as signal, it would swamp every output


@pytest.fixture(scope="module")
def ops(cuda):
    from facodec_amd import ops as _ops
    from facodec_amd import _lib
    _lib.load()
    return _ops


def ref64(x, rate_in, rate_out, quality):
    """The definition in float64 for one row x (L,) -> (y64, sum |h| |x|, taps) over ceil(L n / o) outputs; taps = the most
    terms |t| < W gives any of these outputs, whether or not they fall inside the row."""
    W, rolloff, beta = QUALITIES[quality]
    g = math.gcd(rate_in, rate_out)
    o, n = rate_in // g, rate_out // g
    base = min(o, n) * rolloff
    L = len(x)
    m = np.arange(-(-L * n // o), dtype=np.int64)[:, None]
    reach = int(math.ceil(W * o / base)) + 2
    q = m * o // n + np.arange(-reach, reach + 1, dtype=np.int64)[None, :]
    t = (q * n - m * o).astype(np.float64) / (o * n) * base                    # (q / o - m / n) base from its integer numerator
    win = np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (t / W) ** 2))) / np.i0(beta)
    h = np.where(np.abs(t) < W, np.sinc(t) * win * base / o, 0.0)
    xv = np.where((q >= 0) & (q < L), x.astype(np.float64)[np.clip(q, 0, L - 1)], 0.0)
    return (h * xv).sum(axis=1), (np.abs(h) * np.abs(xv)).sum(axis=1), int((np.abs(t) < W).sum(axis=1).max())


def out_len(L, rate_in, rate_out):
    g = math.gcd(rate_in, rate_out)
    return -(-L * (rate_out // g) // (rate_in // g))


@pytest.fixture(scope="module")
def signals():
    """Seeded randn: the padded batch (3, 4801) with FILL behind every row's length, and the long single row."""
    gen = torch.Generator().manual_seed(5)
    batch = torch.randn(len(LENS), max(LENS), generator=gen)
    for b, L in enumerate(LENS):
        batch[b, L:] = FILL
    return batch, torch.randn(1, LONG, generator=gen)


def _check_row(y, x, rate_in, rate_out, quality, what):
    y64, mag, taps = ref64(x.numpy(), rate_in, rate_out, quality)
    assert y.shape[-1] == len(y64)
    err = np.abs(y.double().cpu().numpy() - y64)
    bound = 1.001 * (taps + 2) * 2.0 ** -24 * mag
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"[tol] resample {rate_in}->{rate_out} {quality} {what}: max |y - y64| = {err.max():.3e}, {worst:.3f} of the bound")
    assert np.all(err <= bound), (what, worst)


@gpu
@pytest.mark.parametrize("quality", sorted(QUALITIES))
@pytest.mark.parametrize("rate_in,rate_out", KERNEL_PAIRS)
def test_kernel_against_fp64_and_rows_alone(ops, cuda, signals, rate_in, rate_out, quality):
    batch, long_row = signals
    xb = batch.to(cuda)
    lens = torch.tensor(LENS, dtype=torch.int32).to(cuda)
    y = ops.resample(xb, rate_in, rate_out, lens=lens, quality=quality)
    geo, table, offs = ops._resample_device_table(rate_in, rate_out, quality, xb.device)
    form = ops.resample_form(ops.resample_desc(geo, table, offs, xb, y, y.shape[-1], lens=lens))[0]
    assert form == FORMS.get((rate_in, rate_out, quality), 0)
    assert y.shape == (len(LENS), out_len(max(LENS), rate_in, rate_out))
    for b, L in enumerate(LENS):
        Lo = out_len(L, rate_in, rate_out)
        _check_row(y[b, :Lo], batch[b, :L], rate_in, rate_out, quality, f"row {b} ({L} samples)")
        assert torch.count_nonzero(y[b, Lo:]) == 0                             # the tail is written, as zeros
        alone = ops.resample(xb[b:b + 1, :L].contiguous(), rate_in, rate_out, quality=quality)
        assert alone.shape == (1, Lo) and torch.equal(y[b, :Lo], alone[0])     # ragged = alone, bit for bit
    yl = ops.resample(long_row.to(cuda).unsqueeze(1), rate_in, rate_out, quality=quality)
    assert yl.shape == (1, 1, out_len(LONG, rate_in, rate_out))
    _check_row(yl[0, 0], long_row[0], rate_in, rate_out, quality, f"single row ({LONG} samples)")


@gpu
def test_equal_rates_and_argument_checks(ops, cuda):
    x = torch.randn(2, 1, 100, device=cuda)
    assert ops.resample(x, 24000, 24000) is x
    assert ops.resample(torch.zeros(2, 0, device=cuda), 48000, 24000).shape == (2, 0)
    with pytest.raises(ValueError):
        ops.resample(x, 24000, 0)
    with pytest.raises(ValueError):
        ops.resample(x[:, 0, 0], 48000, 24000)


STREAMS = [   # rate_in, rate_out, the 12 blocks
    (48000, 24000, [960] * 12),
    (44100, 24000, [882] * 12),
    (44100, 24000, [147, 882, 294, 441, 147, 1470, 882, 147, 588, 294, 735, 147]),
    (24000, 48000, [300, 600] * 6),
]


@gpu
@pytest.mark.parametrize("quality", ["fast", "best"])
@pytest.mark.parametrize("rate_in,rate_out,blocks", STREAMS)
def test_streaming_equals_offline_delayed(ops, cuda, rate_in, rate_out, blocks, quality):
    from facodec_amd.streaming import StreamingResampler
    W, rolloff, _ = QUALITIES[quality]
    g = math.gcd(rate_in, rate_out)
    o, n = rate_in // g, rate_out // g
    D = math.ceil(math.ceil(W * o / (min(o, n) * rolloff)) * n / o)
    x = torch.randn(2, 1, sum(blocks), generator=torch.Generator().manual_seed(9)).to(cuda)
    rs = StreamingResampler(2, rate_in, rate_out, quality=quality, device=cuda)
    assert rs.delay == D and rs.latency == D / rate_out
    parts, t = [], 0
    for k in blocks:
        parts.append(rs.push(x[:, :, t:t + k]))
        assert parts[-1].shape == (2, 1, k * n // o)
        t += k
    tail = rs.finish()
    assert tail.shape == (2, 1, D)
    y = torch.cat(parts + [tail], dim=-1)
    off = ops.resample(x, rate_in, rate_out, quality=quality)
    assert torch.count_nonzero(y[:, :, :D]) == 0
    assert torch.equal(y[:, :, D:], off)
    if o > 1:                                                                  # o + 1 samples are no whole number of outputs
        with pytest.raises(ValueError):
            StreamingResampler(2, rate_in, rate_out, quality=quality, device=cuda).push(x[:, :, :o + 1])


# ------------------------------------------------------------------------------------------------------------- clip lists
CLIP_LENGTHS_48K = (14402, 7203, 14001, 6605)     # at 24 kHz: 7201, 3602, 7001, 3303 -- none a multiple of 300; two groups of two


@pytest.fixture(scope="module")
def full_model(cuda):
    from facodec_amd.commons import build_model, default_model_params
    model = build_model(default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(cuda)
    return model


@gpu
def test_clip_lists_at_other_rates(ops, full_model, cuda):
    w = synth.synth_clips(len(CLIP_LENGTHS_48K), max(CLIP_LENGTHS_48K), seed=31)
    clips = [w[i, :, :L].contiguous().to(cuda) for i, L in enumerate(CLIP_LENGTHS_48K)]
    budget = 2 * 7300
    lens24 = [-(-L // 2) for L in CLIP_LENGTHS_48K]
    assert all(L % 300 for L in lens24) and len(commons.plan_groups(lens24, budget)) == 2
    got = commons.encode_clips(full_model, clips, sample_rate=48000, max_batch_samples=budget)
    want = commons.encode_clips(full_model, [ops.resample(c, 48000, 24000) for c in clips], max_batch_samples=budget)
    for a, b, L in zip(got, want, lens24):
        assert all(torch.equal(ca, cb) for ca, cb in zip(a["codes"], b["codes"])) and a["codes"][0].shape[-1] == L // 300
        assert torch.equal(a["timbre"], b["timbre"])
    codes, timbres = [c["codes"] for c in want], [c["timbre"] for c in want]
    w24 = commons.decode_clips(full_model, codes, timbres, max_batch_samples=budget)
    w16 = commons.decode_clips(full_model, codes, timbres, max_batch_samples=budget, sample_rate=16000)
    for a, b, c in zip(w16, w24, codes):
        F = c[0].shape[-1]
        assert a.shape == (1, -(-300 * F * 16000 // 24000))
        assert torch.equal(a, ops.resample(b.contiguous(), 24000, 16000))
    both = commons.reconstruct_clips(full_model, clips[:2], sample_rate=48000, max_batch_samples=budget)
    assert [tuple(y.shape) for y in both] == [(1, 600 * (L // 300)) for L in lens24[:2]]
    # 5 999 samples at 48 kHz are 3 000 at 24 kHz, the shortest clip the path takes; 5 998 are 2 999
    need = commons.min_clip_samples(full_model)
    assert need == 3000
    commons.encode_clips(full_model, [clips[0][:, :2 * need - 1]], sample_rate=48000)
    with pytest.raises(ValueError, match=f"clip 0 has {need - 1} samples"):
        commons.encode_clips(full_model, [clips[0][:, :2 * need - 2]], sample_rate=48000)


# --------------------------------------------------------------------------------------------------------------- sessions
N_HOPS = 15          # prime + 15 hops = 12 000 samples = 40 frames (finish() wants whole frames); hops 10 - 14 replay graphs


def _keep(o):
    return {k: ([c.clone() for c in v] if isinstance(v, list) else (v.clone() if torch.is_tensor(v) else v)) for k, v in o.items()}


def _run(sess, wave, prime, hop, between=None):
    with torch.no_grad():
        outs = [_keep(sess.prime(wave[:, :, :prime]))]
        for h in range(N_HOPS):
            if between is not None:
                between(sess, h)
            outs.append(_keep(sess.push(wave[:, :, prime + h * hop: prime + (h + 1) * hop])))
        outs.append(_keep(sess.finish()))
    return outs


def _joined(outs):
    codes = [o["codes"] for o in outs if o["codes"] is not None]
    return [torch.cat([c[i] for c in codes], -1) for i in range(len(codes[0]))], torch.cat([o["wave"] for o in outs if o["wave"] is not None], -1)


def _check_wrapped(ops, cuda, make, between=None):
    """make() -> a fresh session.  The session wrapped at 48 kHz in / 16 kHz out against the bare one fed the delayed offline
    resample of the same audio, cut into the same calls."""
    from facodec_amd.streaming import ResampledSession
    x48 = synth.synth_clips(2, 2 * (4800 + N_HOPS * 480), seed=17).to(cuda)
    wrapped = ResampledSession(make(), in_rate=48000, out_rate=16000)
    assert wrapped.prime_samples == 9600 and wrapped.hop_samples == 960
    assert wrapped.latency_in == wrapped.delay_in / 24000 and wrapped.latency_out == wrapped.delay_out / 16000
    got_codes, got_wave = _joined(_run(wrapped, x48, 9600, 960, between))
    x24 = torch.cat([torch.zeros(2, 1, wrapped.delay_in, device=cuda), ops.resample(x48, 48000, 24000, quality="fast")], -1)
    want_codes, wave24 = _joined(_run(make(), x24[:, :, :4800 + N_HOPS * 480].contiguous(), 4800, 480, between))
    assert len(got_codes) == len(want_codes) and all(torch.equal(a, b) for a, b in zip(got_codes, want_codes))
    assert got_codes[0].shape[-1] == (4800 + N_HOPS * 480) // 300
    want_wave = torch.cat([torch.zeros(2, 1, wrapped.delay_out, device=cuda), ops.resample(wave24, 24000, 16000, quality="fast")], -1)
    assert got_wave.shape == want_wave.shape and torch.equal(got_wave, want_wave)


@gpu
def test_resampled_decoder_session(ops, full_model, cuda):
    """A StreamingDecoder wrapped at 16 kHz out: codes pass through, every call returns the wave alone, and the wrapper's
    finish() (the receiver has none) gives what the resampler held back."""
    from facodec_amd.streaming import ResampledSession, StreamingDecoder
    wave = synth.synth_clips(2, 7200, seed=23).to(cuda)
    with torch.no_grad():
        _, _, _, _, timbre, codes = full_model.quantizer(full_model.encoder(wave), wave, n_c=2, return_codes=True)
    cuts = [(0, 12), (12, 16), (16, 17), (17, 24)]

    def run(rx):
        out = [rx.prime([c[:, :, :12].contiguous() for c in codes]).clone()]
        for a, b in cuts[1:]:
            out.append(rx.push([c[:, :, a:b].contiguous() for c in codes]).clone())
        return out
    wrapped = ResampledSession(StreamingDecoder(full_model, timbre), out_rate=16000)
    assert wrapped.prime_samples is None and wrapped.rs_in is None
    got = run(wrapped)
    assert [g.shape[-1] for g in got] == [200 * (b - a) for a, b in cuts]
    got.append(wrapped.finish())
    wave24 = torch.cat(run(StreamingDecoder(full_model, timbre)), -1)
    want = torch.cat([torch.zeros(2, 1, wrapped.delay_out, device=cuda), ops.resample(wave24, 24000, 16000, quality="fast")], -1)
    assert torch.equal(torch.cat(got, -1), want)
    with pytest.raises(ValueError, match="codes"):
        ResampledSession(StreamingDecoder(full_model, timbre), in_rate=48000)


@gpu
def test_resampled_codec_session(ops, full_model, cuda):
    from facodec_amd.streaming import StreamingCodec
    timbre = torch.randn(2, 1024, generator=torch.Generator().manual_seed(3)).to(cuda)
    _check_wrapped(ops, cuda, lambda: StreamingCodec(full_model, timbre, use_graphs=True))


@gpu
def test_resampled_converter_session_with_set_target(ops, full_model, cuda):
    from facodec_amd.commons import build_model, default_redecoder_params
    from facodec_amd.streaming import StreamingConverter
    args = default_redecoder_params()
    args.decoder_causal, args.decoder_lstm = True, 2
    rm = build_model(args, stage="redecoder")
    for k in ("encoder", "decoder"):
        synth.load_synthetic(rm[k], seed=0, prefix="redecoder." + k + ".")
        rm[k].eval().to(cuda)
    gen = torch.Generator().manual_seed(4)
    t0, t1 = (torch.randn(2, 1024, generator=gen).to(cuda) for _ in range(2))

    def between(sess, h):
        if h == 7:
            sess.set_target(t1)                                  # passes through the wrapper to the converter
    _check_wrapped(ops, cuda, lambda: StreamingConverter(full_model, rm, t0), between)
