"""Level control on the device: fac_agc_gains, fac_agc_apply, fac_true_peak and what is built on them
(ops.level, streaming.AutoGain / LevelledSession, commons.level_clips) against the fp64 numpy restatement of the header's
definitions in tests/test_agc_cpu.py.

Gains: within 1e-9 dB of the restatement on the kernel's own input energies (device and numpy log10 differ by ulps, below 1e-13
here; a wrong window or gate moves a gain by 1e-3 or more).  Apply: with the gains given, bit for bit, for the offline call and
for any chunking of a stream.  End to end, streamed against offline: gains within L_TOL = 1e-6 dB (the project's bound for
streamed against offline loudness: the K-weighting filter's chunk boundaries move with the blocks), samples within G_TOL =
2.4e-7 of the row's largest (1e-6 dB is 1.15e-7 relative, plus one fp32 rounding).  True peak: the bits of the maximum over
ops.resample's output."""
import math

import numpy as np
import pytest
import torch

from facodec_amd import synth
from test_agc_cpu import DEFAULTS, RATE, S, apply_ref, ceiling, check_refusals, gains_ref

pytestmark = pytest.mark.gpu

L_TOL = 1e-6
G_TOL = 2.4e-7
T = 72000
LENS = [72000, 30001, 7000, 0, 9000]                                 # 3 s; mid sub-block; under 3 sub-blocks; empty; under 4 S


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _blocks(first, hop, total):
    sizes, n = [], 0
    for k in first:
        sizes.append(k)
        n += k
    while n < total:
        sizes.append(min(hop, total - n))
        n += sizes[-1]
    return sizes


CHUNKINGS = [(1, 7, 479, 2400), ()]
CHUNK_IDS = ["ragged-blocks", "480-hops"]


@pytest.fixture(scope="module")
def batch():
    """Five rows of one launch, computed once and never written to: row 0 jumps from 0.003 to 0.5 rms half way (the limiter has
    work), the others are stationary at different levels; what lies behind a clip's end is 7.0 and must never be read."""
    g = np.random.default_rng(21)
    r0 = g.standard_normal(72000)
    r0[:36000] *= 0.003
    r0[36000:] *= 0.5
    rows = [r0.astype(np.float32), (0.02 * g.standard_normal(30001)).astype(np.float32), (0.2 * g.standard_normal(7000)).astype(np.float32),
            np.zeros(0, dtype=np.float32), (0.01 * g.standard_normal(9000)).astype(np.float32)]
    assert [len(r) for r in rows] == LENS
    x = np.full((5, T), 7.0, dtype=np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return dict(rows=rows, x=x)


@pytest.fixture(scope="module")
def on_device(cuda, batch):
    from facodec_amd import ops
    x = torch.from_numpy(batch["x"]).to(cuda)
    lens = torch.tensor(LENS, dtype=torch.int32, device=cuda)
    e = ops.loudness_energies(x, RATE, lens=lens).e
    return dict(x=x, lens=lens, e=e, e_host=e.cpu().numpy())


def params(window, lookahead):
    from facodec_amd import ops
    return ops.agc_params(RATE, window=window, lookahead=lookahead)


# ---------------------------------------------------------------------------------------------------------------- gains
@pytest.mark.parametrize("window", [5, 30])
def test_gains_of_a_ragged_batch(cuda, on_device, window):
    from facodec_amd import ops
    p = params(window, 120)
    n = T // S
    G, g = ops.agc_gains(on_device["e"], p, 0, n, R=n, lens=on_device["lens"])
    G, g = G.cpu().numpy(), g.cpu().numpy()
    worst = 0.0
    for b, L in enumerate(LENS):
        G_ref, g_ref = gains_ref(on_device["e_host"][b], L, **dict(DEFAULTS, window=window))
        nb = L // S
        assert len(G_ref) == nb
        worst = max(worst, float(np.max(np.abs(G[b, :nb] - G_ref), initial=0.0)))
        assert np.all(G[b, nb:] == 0.0) and np.all(g[b, nb:] == 1.0)             # partial and absent sub-blocks produce no gain
        assert np.allclose(g[b, :nb], 10.0 ** (G[b, :nb] / 20.0), rtol=1e-14, atol=0.0)
        if nb < 4:
            assert np.all(G[b] == 0.0)
    print(f"window {window}: max |G - G_ref| = {worst:.3e} dB")
    assert worst <= 1e-9
    assert np.abs(G[0]).max() > 10.0 and np.abs(G[1, 3:12]).min() > 1.0          # the gains are no zeros


def test_gains_in_a_wrapped_ring_and_from_a_row_start(cuda, on_device):
    """The ring: sub-block j at column j % R, fed four sub-blocks at a time through a ring of 12 (it wraps twice): the bits of
    the plain call.  j_start: a row whose stream starts at sub-block 4 has no gain before it and a fresh window from it on."""
    from facodec_amd import ops
    p = params(5, 120)
    n, R = T // S, 12
    e = torch.stack([on_device["e"][0], on_device["e"][0].flip(0)])
    js = torch.tensor([0, 4], dtype=torch.int64, device=cuda)
    G_plain, g_plain = ops.agc_gains(e, p, 0, n, R=n, j_start=js)
    ring = torch.zeros(2, R, device=cuda, dtype=torch.float64)
    Gr, gr = torch.full((2, R), 9.0, device=cuda, dtype=torch.float64), torch.full((2, R), 9.0, device=cuda, dtype=torch.float64)
    G_got, g_got = torch.empty_like(G_plain), torch.empty_like(g_plain)
    for j0 in range(0, n, 4):
        k = min(4, n - j0)
        cols = torch.arange(j0, j0 + k, device=cuda)
        ring[:, cols % R] = e[:, cols]
        ops.agc_gains(ring, p, j0, k, R=R, j_start=js, G=Gr, g=gr)
        G_got[:, cols], g_got[:, cols] = Gr[:, cols % R], gr[:, cols % R]
    assert torch.equal(G_got, G_plain) and torch.equal(g_got, g_plain)
    e1 = e[1].cpu().numpy()
    want = gains_ref(e1, T, **dict(DEFAULTS, window=5), j_start=4)[0]
    assert np.all(want[:7] == 0.0) and np.abs(want[7:]).min() > 1.0
    assert np.max(np.abs(G_plain[1].cpu().numpy() - want)) <= 1e-9
    assert np.max(np.abs(G_plain[0].cpu().numpy() - gains_ref(e[0].cpu().numpy(), T, **dict(DEFAULTS, window=5))[0])) <= 1e-9


# ---------------------------------------------------------------------------------------------------------------- apply
@pytest.fixture(scope="module")
def given_gains(on_device):
    """The restatement's own gains (window 5: they move fast) for the five rows, padded with ones: the kernel is handed these."""
    g = np.ones((5, T // S))
    for b, L in enumerate(LENS):
        gb = gains_ref(on_device["e_host"][b], L, **dict(DEFAULTS, window=5))[1]
        g[b, :len(gb)] = gb
    return g


@pytest.fixture(scope="module")
def apply_refs(batch, given_gains):
    return {LA: [apply_ref(r, given_gains[b], LA) for b, r in enumerate(batch["rows"])] for LA in (7, 120)}


@pytest.mark.parametrize("LA", [7, 120])
def test_apply_of_a_ragged_batch_bit_for_bit(cuda, on_device, given_gains, apply_refs, LA):
    from facodec_amd import ops
    p = params(5, LA)
    g = torch.from_numpy(given_gains).to(cuda)
    y = ops.agc_apply(on_device["x"], g, p, lens=on_device["lens"], flush=True).cpu().numpy()
    assert y.shape == (5, T + LA) and y.dtype == np.float32
    bound = float(np.float32(p.ceiling)) * (1.0 + 2.0 ** -22)
    for b, L in enumerate(LENS):
        ref = apply_refs[LA][b]
        assert len(ref) == L + LA
        assert np.array_equal(bits(y[b, :L + LA]), bits(ref)), f"row {b}"
        assert np.all(y[b, L + LA:] == 0.0)
    assert np.max(np.abs(y.astype(np.float64))) <= bound
    assert np.max(np.abs(y[0])) > 0.99 * p.ceiling                               # row 0 was held at the ceiling ...
    lim = np.abs(apply_refs[LA][0].astype(np.float64) - np.concatenate([np.zeros(LA), batch_v(on_device, given_gains, 0)]))
    assert (lim > 1e-3).sum() > 1000                                             # ... over many samples


def batch_v(on_device, given_gains, b):
    from test_agc_cpu import gained_ref
    return gained_ref(on_device["x"][b, :LENS[b]].cpu().numpy(), given_gains[b])


@pytest.mark.parametrize("LA", [7, 120])
def test_limiter_events_on_the_edges(cuda, LA):
    """One row of 5000 samples (five tiles of 1024 outputs, the last one partial) of quiet noise with spikes of +-3 where the
    kernel's index arithmetic could slip: within 2 LA of the start, around every tile boundary of the outputs (output m takes
    input m - LA and looks 2 LA back), and in the last LA samples; the gains ramp between 0.5 and 2."""
    from facodec_amd import ops
    n = 5000
    g = np.random.default_rng(22)
    x = (0.05 * g.standard_normal(n)).astype(np.float32)
    at = {0, 1, LA - 1, LA, 2 * LA - 1, 2 * LA, n - 1, n - 2, n - LA, n - LA - 1, n - 2 * LA}
    for edge in (1024, 2048, 3072, 4096):
        at |= {edge - 2 * LA - 1, edge - 2 * LA, edge - LA - 1, edge - LA, edge - LA + 1, edge - 1, edge, edge + 1}
    for i, pos in enumerate(sorted(at)):
        x[pos] = 3.0 if i % 2 else -3.0
    gains = np.array([[0.5, 2.0]])
    p = params(5, LA)
    y = ops.agc_apply(torch.from_numpy(x).to(cuda)[None], torch.from_numpy(gains).to(cuda), p, flush=True).cpu().numpy()[0]
    ref = apply_ref(x, gains[0], LA)
    assert y.shape == ref.shape == (n + LA,)
    assert np.array_equal(bits(y), bits(ref))
    assert np.max(np.abs(y.astype(np.float64))) <= float(np.float32(p.ceiling)) * (1.0 + 2.0 ** -22)
    assert np.abs(y[-LA:]).max() > 0.5 and np.abs(y[:3 * LA]).max() > 0.5        # the events at both ends reached the output


@pytest.fixture(scope="module")
def chunk_refs(batch, given_gains):
    """Rows 0 and 1 of the batch array over their first 2 s, without lens: row 1's 7.0 behind sample 30001 is signal here, and
    far above the ceiling.  The restatement's output for both look-aheads, computed once."""
    n = 48000
    return {LA: [apply_ref(batch["x"][b, :n], given_gains[b], LA) for b in range(2)] for LA in (7, 120)}


@pytest.mark.parametrize("first", CHUNKINGS, ids=CHUNK_IDS)
@pytest.mark.parametrize("LA", [7, 120])
def test_apply_in_chunks_gives_the_offline_bits(cuda, on_device, given_gains, chunk_refs, LA, first):
    """Two rows as streams with the gains given: carry buffers alternating, outputs LA late, the flush at the end.
    Concatenated: the offline call's bits, and the restatement's."""
    from facodec_amd import ops
    p = params(5, LA)
    n = 48000
    x = on_device["x"][:2, :n]
    g = torch.from_numpy(given_gains[:2]).to(cuda)
    carry = [torch.zeros(2, 2 * LA, device=cuda, dtype=torch.float64) for _ in range(2)]
    cur, t, parts = 0, 0, []
    for k in _blocks(first, 480, n):
        parts.append(ops.agc_apply(x[:, t:t + k], g, p, n0=t, carry_in=carry[cur], carry_out=carry[1 - cur], flush=False))
        assert parts[-1].shape == (2, k)
        cur, t = 1 - cur, t + k
    parts.append(ops.agc_apply(None, g, p, n0=t, carry_in=carry[cur], flush=True, k=0))
    assert parts[-1].shape == (2, LA)
    got = torch.cat(parts, dim=1).cpu().numpy()
    off = ops.agc_apply(x, g, p, flush=True).cpu().numpy()
    assert np.array_equal(bits(got), bits(off))
    for b in range(2):
        assert np.array_equal(bits(got[b]), bits(chunk_refs[LA][b])), f"row {b}"
    assert np.max(np.abs(got.astype(np.float64))) <= float(np.float32(p.ceiling)) * (1.0 + 2.0 ** -22)


# ---------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def offline(cuda, on_device):
    from facodec_amd import ops
    x = on_device["x"][:2, :48000].clone()
    x[1, :30001] = on_device["x"][1, :30001]
    x[1, 30001:] = on_device["x"][0, 30001:48000] * 0.25                        # row 1: two seconds without padding
    return dict(x=x, out={(w, la): ops.level(x, RATE, window=w, lookahead=la) for w, la in ((30, 120), (5, 7))})


def _stream(agc, x, first):
    t, parts = 0, []
    for k in _blocks(first, 480, x.shape[-1]):
        parts.append(agc.push(x[..., t:t + k]))
        assert parts[-1].shape == x[..., t:t + k].shape
        t += k
    return parts


@pytest.mark.parametrize("first", CHUNKINGS, ids=CHUNK_IDS)
@pytest.mark.parametrize("window,LA", [(30, 120), (5, 7)])
def test_autogain_against_the_offline_call(cuda, offline, window, LA, first):
    from facodec_amd.streaming import AutoGain
    x, off = offline["x"], offline["out"][(window, LA)]
    assert off.y.shape == (2, 48000 + LA) and off.G.shape == (2, 20)
    agc = AutoGain(2, RATE, window=window, lookahead=LA)
    assert agc.latency == LA / RATE and agc.lookahead == LA
    parts = _stream(agc, x, first)
    G, g = agc.gains(20)
    parts.append(agc.finish())
    got = torch.cat(parts, dim=-1)
    dG = float((G - off.G).abs().max())
    dy = ((got - off.y).abs().amax(-1) / off.y.abs().amax(-1)).cpu().tolist()
    print(f"window {window}, LA {LA}: max |G - G_offline| = {dG:.3e} dB, max |y - y_offline| / max |y_offline| = {dy}")
    assert dG <= L_TOL
    assert float((g / off.g - 1.0).abs().max()) <= 1.2e-7
    assert max(dy) <= G_TOL
    assert float(off.G.abs().max()) > 10.0 and float(off.y.abs().max()) > 0.99 * ceiling()
    with pytest.raises(RuntimeError):
        agc.push(x[:, :480])


def test_autogain_row_alone_equals_the_row_in_a_batch(cuda, offline):
    from facodec_amd import ops
    from facodec_amd.streaming import AutoGain
    x = offline["x"][:, :12000]
    both, alone = AutoGain(2, RATE, window=5), AutoGain(1, RATE, window=5)
    a = torch.cat(_stream(both, x[:, None], CHUNKINGS[0]) + [both.finish()[:, None]], dim=-1)
    b = torch.cat(_stream(alone, x[1:, None], CHUNKINGS[0]) + [alone.finish()[:, None]], dim=-1)
    assert a.shape == (2, 1, 12120) and torch.equal(a[1:], b)
    assert all(torch.equal(u[1:], v) for u, v in zip(both.gains(5), alone.gains(5)))
    assert torch.equal(ops.level(x[1:], RATE, window=5).y, ops.level(x, RATE, window=5).y[1:])


def test_reset_rows_is_a_fresh_stream(cuda, offline):
    """Three rows run for two sub-blocks; row 1 is reset there (on the 100 ms grid) and all rows run on.  Row 1 then gives what
    a fresh stream gives for the same blocks, bit for bit; rows 0 and 2 what they give without the reset."""
    from facodec_amd.streaming import AutoGain
    x = torch.cat([offline["x"], offline["x"][:1].flip(-1)])[:, 26400:26400 + 4800 + 16800].contiguous()
    assert x.shape == (3, 21600)
    run, plain, fresh = (AutoGain(3, RATE, window=5) for _ in range(3))
    head, rest = x[:, :4800], x[:, 4800:]
    h_run, h_plain = torch.cat(_stream(run, head, ()), -1), torch.cat(_stream(plain, head, ()), -1)
    assert torch.equal(h_run, h_plain)
    run.reset([1])
    r_run, r_plain, r_fresh = (torch.cat(_stream(a, rest, ()) + [a.finish()], -1) for a in (run, plain, fresh))
    assert torch.equal(r_run[1], r_fresh[1]) and not torch.equal(r_run[1], r_plain[1])
    assert torch.equal(r_run[[0, 2]], r_plain[[0, 2]])
    for got, want, other in zip(run.gains(7), fresh.gains(7), plain.gains(7)):
        assert torch.equal(got[1], want[1]) and torch.equal(got[[0, 2]], other[[0, 2]])
    assert float(fresh.gains(7)[0][1].abs().max()) > 1.0


def test_level_clips_does_not_depend_on_the_grouping(cuda):
    """Gains within 1e-9 dB (the bound loudness_clips holds between a clip alone and in a group), samples within one fp32
    rounding, 2^-23, of the clip's largest."""
    from facodec_amd import commons, ops
    lengths = [24000, 4800, 48000, 11111, 30001]
    g = np.random.default_rng(23)
    clips = [torch.from_numpy((0.02 * (i + 1) * g.standard_normal(n)).astype(np.float32)).to(cuda) for i, n in enumerate(lengths)]
    clips[2] = clips[2][None]
    assert len(commons.plan_groups(lengths, 60002)) == 3
    got = commons.level_clips(clips, RATE, max_batch_samples=60002, window=5)
    one = commons.level_clips(clips, window=5)
    for c, n, a, b in zip(clips, lengths, got, one):
        alone = ops.level(c.reshape(1, -1), RATE, window=5)
        assert alone.y.shape == (1, n + 120) and a.y.shape == b.y.shape == (n + 120,) and a.G.shape == (n // S,)
        for r in (a, b):
            assert float((r.G - alone.G[0]).abs().max()) <= 1e-9
            assert float((r.y - alone.y[0]).abs().max()) <= 2.0 ** -23 * float(alone.y.abs().max())
    assert float(got[0].G.abs().max()) > 1.0


# ---------------------------------------------------------------------------------------------------------------- the session
@pytest.fixture(scope="module")
def full_model(cuda):
    from facodec_amd.commons import build_model, default_model_params
    model = build_model(default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(cuda)
    return model


def _keep(o):
    return {k: ([c.clone() for c in v] if isinstance(v, list) else (v.clone() if torch.is_tensor(v) else v)) for k, v in o.items()}


def test_levelled_session(full_model, cuda):
    """A StreamingCodec behind LevelledSession: what the session is fed is AutoGain's output -- `lookahead` zeros, then the
    levelled input --, and the dicts are those of the bare session fed that signal."""
    from facodec_amd import ops
    from facodec_amd.streaming import HOP, AutoGain, LevelledSession, StreamingCodec
    m = full_model
    n_hops = 15                                                              # 12000 samples: five sub-blocks, two of them with a gain
    n = 4800 + n_hops * HOP
    wave = (0.02 * synth.synth_clips(2, n, seed=47)).to(cuda)
    with torch.no_grad():
        timbre = m.quantizer(m.encoder(wave), wave, n_c=2, return_codes=True)[4].clone()
        agc = AutoGain(2, RATE, window=5, lookahead=120)
        fed = [agc.push(wave[:, :, :4800])] + [agc.push(wave[:, :, 4800 + h * HOP:4800 + (h + 1) * HOP]) for h in range(n_hops)]
        lev = torch.cat(fed, dim=-1)
        off = ops.level(wave, RATE, window=5, lookahead=120)
        assert torch.all(lev[:, :, :120] == 0.0)
        assert float((lev - off.y[:, :, :n]).abs().max()) <= G_TOL * float(off.y.abs().max())
        assert float(off.G.abs().max()) > 1.0                                    # the session does not see the raw input
        bare = StreamingCodec(m, timbre, n_c=2, use_graphs=False)
        want = [_keep(bare.prime(fed[0]))] + [_keep(bare.push(f)) for f in fed[1:]] + [_keep(bare.finish())]
        sess = LevelledSession(StreamingCodec(m, timbre, n_c=2, use_graphs=False), window=5, lookahead=120)
        assert sess.latency_in == 120 / RATE and sess.prime_samples == 4800 and sess.lookahead == 120
        got = [_keep(sess.prime(wave[:, :, :4800]))]
        got += [_keep(sess.push(wave[:, :, 4800 + h * HOP:4800 + (h + 1) * HOP])) for h in range(n_hops)]
        got.append(_keep(sess.finish()))
    n_codes = 0
    for a, b in zip(got, want):
        assert a.keys() == b.keys()
        for k in a:
            if isinstance(a[k], list):
                assert len(a[k]) == len(b[k]) and all(torch.equal(u, v) for u, v in zip(a[k], b[k])), k
                n_codes += sum(u.numel() for u in a[k]) if k == "codes" else 0
            elif torch.is_tensor(a[k]):
                assert torch.equal(a[k], b[k]), k
            else:
                assert a[k] == b[k], k
    assert n_codes > 0


# ---------------------------------------------------------------------------------------------------------------- true peak
def _band_limited(g, n, scale, total=5000):
    """n samples of Gaussian noise with nothing above a quarter of the sampling rate (a brick wall on the rfft bins) under a
    Hann window over the n samples -- a clip that ends in a cut is not band-limited, whatever it was cut from --, zeros up to
    `total`; float32."""
    out = np.zeros(total, dtype=np.float32)
    if n:
        spec = np.fft.rfft(g.standard_normal(n))
        spec[n // 4 + 1:] = 0.0
        y = np.fft.irfft(spec, n) * np.hanning(n)
        out[:n] = (scale * y / np.abs(y).max()).astype(np.float32)
    return out


@pytest.mark.parametrize("quality", ["best", "fast"])
def test_true_peak_is_the_maximum_over_the_resampled_signal(cuda, quality):
    """(4, 5000) with lens [5000, 4999, 301, 0], what lies behind a row's end poisoned with 7.0: the bits of the maximum over
    ops.resample's output, and never below the sample peak.  The rows are what a true-peak meter is defined for: noise
    band-limited to a quarter of the sampling rate, every row tapered over its own length.  The oversampled signal then passes
    through the samples to the filter's pass-band ripple (1e-4 or so) and reaches the crest between them to within an eighth of
    a sample; it can read under the sample peak only where the largest sample sits within about 0.01 samples of its crest.
    Signals that are not band-limited are held to the bit-equality alone, and what the meter reads is printed: the oversampling
    filter removes what lies in its transition band under the Nyquist frequency, so its output does not pass through the
    samples.  Measured on an MI355X: the white row of 0.5 rms below reads 1.8362 against a sample peak of 1.9259 at quality
    "fast" (2.0718 at "best"); while this test was written, band-limited noise cut off hard after 301 samples read 0.8245
    against 0.8276."""
    from facodec_amd import ops
    g = np.random.default_rng(24)
    lens_host = [5000, 4999, 301, 0]
    lens = torch.tensor(lens_host, dtype=torch.int32, device=cuda)
    x_host = np.stack([_band_limited(g, L, s) for L, s in zip(lens_host, (0.5, 0.1, 0.9, 0.3))])
    white = g.standard_normal((4, 5000)).astype(np.float32) * np.array([[0.5], [0.1], [0.9], [0.3]], dtype=np.float32)
    for name, arr in (("band-limited", x_host), ("white", white)):
        x = torch.from_numpy(arr).to(cuda)
        x_poison = x.clone()
        for b, L in enumerate(lens_host):
            x_poison[b, L:] = 7.0
        got = ops.true_peak(x_poison, RATE, lens=lens, quality=quality)
        want = ops.resample(x_poison, RATE, 4 * RATE, lens=lens, quality=quality).abs().amax(-1)
        assert got.shape == (4,) and got.dtype == torch.float32
        assert torch.equal(got, want)
        sample = torch.stack([x_poison[b, :L].abs().max() if L else x.new_zeros(()) for b, L in enumerate(lens_host)])
        print(f"{name}, quality {quality}: true peak {got.cpu().tolist()}, sample peak {sample.cpu().tolist()}")
        assert float(got[3]) == 0.0
        if name == "band-limited":
            assert torch.all(got >= sample)
        assert torch.equal(ops.true_peak(x, RATE, quality=quality), ops.resample(x, RATE, 4 * RATE, quality=quality).abs().amax(-1))
        assert torch.equal(ops.true_peak(x[:, None], RATE, quality=quality), ops.true_peak(x, RATE, quality=quality))


def test_true_peak_of_a_tone_between_its_samples(cuda):
    """6 kHz at 24 kHz sampled 45 degrees off its crest: every sample is +-0.7071, the crest of 1.0 lies between them."""
    from facodec_amd import ops
    t = np.arange(4800)
    x = torch.from_numpy(np.sin(2.0 * math.pi * 0.25 * t + math.pi / 4.0).astype(np.float32)).to(cuda)[None]
    assert abs(float(x.abs().max()) - math.sqrt(0.5)) < 1e-6
    for quality in ("best", "fast"):
        got = ops.true_peak(x, RATE, quality=quality)
        want = ops.resample(x, RATE, 4 * RATE, quality=quality).abs().amax(-1)
        print(f"true peak of the 6 kHz tone, quality {quality}: {float(got[0]):.6f} (sample peak 0.707107)")
        assert torch.equal(got, want)
        assert float(got[0]) > 0.9


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_before_any_launch(cuda):
    check_refusals()
    from facodec_amd import ops
    from facodec_amd.streaming import AutoGain
    agc = AutoGain(2, RATE)
    with pytest.raises(ValueError):
        agc.push(torch.zeros(2, 0, device=cuda))
    with pytest.raises(ValueError):
        agc.push(torch.zeros(3, 480, device=cuda))
    with pytest.raises(ValueError):
        agc.gains(1)
    with pytest.raises(ValueError):
        agc.reset([2])
    with pytest.raises(ValueError, match="carry_in"):
        ops.agc_apply(torch.zeros(2, 480, device=cuda), agc._g, agc.p, carry_in=torch.zeros(2, 7, device=cuda, dtype=torch.float64), flush=False)
