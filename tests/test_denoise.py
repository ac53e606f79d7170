"""Noise suppression on the device: fac_ns_power, fac_ns_gains, fac_ns_synth and what is built on them
(ops.denoise, streaming.NoiseSuppressor / DenoisedSession, commons.denoise_clips) against the fp64 numpy restatement of the
header's definition in tests/test_denoise_cpu.py.

Against the restatement only broadband rows are compared: Gaussian noise of at least 1e-3 of the row's peak plus louder bursts,
or exact zeros.  A bin whose power sits at eps^2 of its frame's energy has no defined gain (device and numpy would legitimately
disagree there); exact zeros transform to exact zeros on both sides.  Bounds: P within 1e-13 of its frame's total power (the
transform's error is about 9 stages x 1.1e-16 of the frame's norm, and P's twice that, relative to the total: 2e-15, with 50 x
headroom); G within 1e-9 (a wrong window, a wrong first frame or a swapped overlap moves it by 1e-3 or more); y within 2^-22
of the row's largest sample (one fp32 rounding plus fp64 noise).  Device against device -- streamed against offline, a row
alone against the row in a batch, grouped clips, a reset row against the offline call with `starts` -- is bit for bit.

Measured on an MI355X (worst over the rows of the batch, both (M, W)): P 3.8e-17, G 2.7e-14, y 0."""
import numpy as np
import pytest
import torch

from facodec_amd import _lib, synth
from test_denoise_cpu import (BINS, DELAY, H, broadband, check_refusals, denoise_ref, g_min_of, n_frames, synthetic_mix)

pytestmark = pytest.mark.gpu

T = 30000
LENS = (30000, 2561, 256, 255, 1, 0)      # a full window; one sample into a new frame; exactly one hop; one less; one sample; empty
MW = [(8, 96), (2, 5)]
MW_IDS = ["M8-W96", "M2-W5"]
# the last: 3, 4, 5 and 2 frames in one push, so that the power kernel's last round of four waves holds 3, 4, 1 and 2 frames
FIRST = [(1, 7, 479, 2400), (), (768, 1024, 1280, 512)]
FIRST_IDS = ["ragged-blocks", "480-hops", "whole-frame-blocks"]


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float32).view(np.int32)


def _blocks(first, hop, total):
    sizes, n = [], 0
    for k in first:
        sizes.append(k)
        n += k
    while n < total:
        sizes.append(min(hop, total - n))
        n += sizes[-1]
    return sizes


@pytest.fixture(scope="module")
def batch():
    """Six rows of one launch, computed once and never written to; what lies behind a clip's end is 7.0 and must never be read."""
    rows = [broadband(n, 31 + b) for b, n in enumerate(LENS)]
    x = np.full((len(LENS), T), 7.0, dtype=np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return dict(rows=rows, x=x)


@pytest.fixture(scope="module")
def on_device(cuda, batch):
    return dict(x=torch.from_numpy(batch["x"]).to(cuda), lens=torch.tensor(LENS, dtype=torch.int32, device=cuda))


@pytest.fixture(scope="module")
def refs(batch):
    """(y, G, P) of the restatement per (M, W) and row, at the batch's width."""
    return {mw: [denoise_ref(r, M=mw[0], W=mw[1], T=T) for r in batch["rows"]] for mw in MW}


@pytest.fixture(scope="module")
def offline(cuda, on_device):
    from facodec_amd import ops
    return {mw: ops.denoise(on_device["x"], lens=on_device["lens"], M=mw[0], W=mw[1]) for mw in MW}


# ---------------------------------------------------------------------------------------------- 1: against the restatement
@pytest.mark.parametrize("mw", MW, ids=MW_IDS)
def test_power_gains_and_samples_of_a_ragged_batch(cuda, on_device, refs, offline, mw):
    from facodec_amd import ops
    F = n_frames(T)
    x, lens = on_device["x"], on_device["lens"]
    P = ops.ns_power(x, torch.empty(len(LENS), F, BINS, device=cuda, dtype=torch.float64), lens=lens).cpu().numpy()
    got = offline[mw]
    assert got.y.shape == x.shape and got.y.dtype == torch.float32 and got.G.shape == (len(LENS), F, BINS) and got.G.dtype == torch.float64
    y, G = got.y.cpu().numpy(), got.G.cpu().numpy()
    worst = dict(P=0.0, G=0.0, y=0.0)
    for b, n in enumerate(LENS):
        y_ref, G_ref, P_ref = refs[mw][b]
        Fb = n_frames(n)
        assert (P[b, Fb:] == 0.0).all()                                       # frames behind the row's last see only zeros,
        assert (G[b, Fb + mw[0] - 1:] == 1.0).all()                           # and so does the mean M - 1 frames later
        assert (y[b, n:] == 0.0).all()
        if n == 0:
            continue
        total = P_ref.sum(axis=1, keepdims=True)
        eP = float((np.abs(P[b] - P_ref) / np.where(total > 0, total, 1.0)).max())
        eG = float(np.abs(G[b] - G_ref).max())
        peak = float(np.abs(on_device["x"][b, :n].cpu().numpy()).max())
        ey = float(np.abs(y[b].astype(np.float64) - y_ref.astype(np.float64)).max()) / peak
        print(f"{mw} row {b} (len {n}): P {eP:.3g} of the frame's power, G {eG:.3g}, y {ey:.3g} of the peak = {ey * 2 ** 23:.3f} x 2^-23")
        worst = dict(P=max(worst["P"], eP), G=max(worst["G"], eG), y=max(worst["y"], ey))
        assert eP <= 1e-13
        assert eG <= 1e-9
        assert ey <= 2.0 ** -22
        assert G[b].min() >= g_min_of(15.0) and G[b].max() <= 1.0
    print(f"{mw} worst: {worst}")
    assert float(got.G[0, :n_frames(LENS[0])].min()) < 0.5                    # the suppressor has work


def test_unit_gain_while_digital_silence_is_in_the_window(cuda):
    """3 s of exact zeros, then noise: G is exactly 1 while a silent frame is in the window, and the restatement's after."""
    from facodec_amd import ops
    x = np.concatenate([np.zeros(72000, dtype=np.float32), broadband(30000, 41, bursts=1)])
    got = ops.denoise(torch.from_numpy(x)[None].to(cuda))
    y_ref, G_ref, _ = denoise_ref(x)
    G = got.G[0].cpu().numpy()
    last_silent = 72000 // H - 1                                              # frame f covers (f - 1) H .. (f + 1) H - 1: 72000 = 281.25 H
    assert last_silent == 280 and (x[:(last_silent + 1) * H] == 0.0).all()
    assert (G[:last_silent + 96] == 1.0).all()
    assert (G[last_silent + 96:-2] < 1.0).any()
    assert float(np.abs(G - G_ref).max()) <= 1e-9
    assert torch.all(got.y[0, :last_silent * H] == 0.0)
    assert float(np.abs(got.y[0].cpu().numpy().astype(np.float64) - y_ref).max()) <= 2.0 ** -22 * float(np.abs(x).max())


# ---------------------------------------------------------------------------------------------- 2: streamed against offline
@pytest.fixture(scope="module")
def streams(cuda):
    """Three full rows for the streaming tests and their offline results per (M, W)."""
    from facodec_amd import ops
    x = torch.from_numpy(np.stack([broadband(T, 51 + b) for b in range(3)])).to(cuda)
    return dict(x=x, off={mw: ops.denoise(x, M=mw[0], W=mw[1]) for mw in MW})


def _stream(ns, x, first, hop=480):
    out, t = [], 0
    for k in _blocks(first, hop, x.shape[-1]):
        out.append(ns.push(x[..., t:t + k]))
        assert out[-1].shape == x[..., t:t + k].shape
        t += k
    out.append(ns.finish())
    return torch.cat(out, dim=-1)


@pytest.mark.parametrize("first", FIRST, ids=FIRST_IDS)
@pytest.mark.parametrize("mw,ring", [((8, 96), 128), ((2, 5), 128), ((2, 5), 12)], ids=["M8-W96-ring128", "M2-W5-ring128", "M2-W5-ring12"])
def test_streamed_equals_offline_bit_for_bit(cuda, streams, mw, ring, first):
    """Any chunking gives 512 zeros and then the offline call's bits, finish() included; a ring of 12 frames wraps ten times in
    119 frames and makes the 2400-sample push run as two."""
    from facodec_amd.streaming import NoiseSuppressor
    x, off = streams["x"], streams["off"][mw]
    ns = NoiseSuppressor(3, M=mw[0], W=mw[1], ring=ring)
    assert ns.delay == DELAY and ns.latency == DELAY / 24000
    got = _stream(ns, x, first)
    assert ns.samples == T and got.shape == (3, T + DELAY)
    assert torch.all(got[:, :DELAY] == 0.0)
    assert np.array_equal(bits(got[:, DELAY:]), bits(off.y))
    n = min(ring, n_frames(T))
    assert torch.equal(ns.gains(n), off.G[:, n_frames(T) - n:])


def test_streamed_three_dimensional_blocks_and_short_streams(cuda, streams):
    from facodec_amd import ops
    from facodec_amd.streaming import NoiseSuppressor
    for n in (1, 255, 256, 257, 700):
        x = streams["x"][:1, None, :n].contiguous()
        ns = NoiseSuppressor(1)
        got = torch.cat([ns.push(x), ns.finish()[:, None]], dim=-1)
        assert got.shape == (1, 1, n + DELAY) and torch.all(got[..., :DELAY] == 0.0)
        assert np.array_equal(bits(got[..., DELAY:]), bits(ops.denoise(x).y))


# ---------------------------------------------------------------------------------------------- 3: other bit-for-bit checks
@pytest.mark.parametrize("mw", MW, ids=MW_IDS)
def test_a_row_alone_equals_the_row_in_the_batch(cuda, on_device, offline, mw):
    from facodec_amd import ops
    for b, n in enumerate(LENS):
        alone = ops.denoise(on_device["x"][b:b + 1, :n].contiguous(), M=mw[0], W=mw[1])
        assert alone.y.shape == (1, n) and alone.G.shape == (1, n_frames(n), BINS)
        assert np.array_equal(bits(alone.y[0]), bits(offline[mw].y[b, :n]))
        assert torch.equal(alone.G[0], offline[mw].G[b, :n_frames(n)])


def test_spectra_kept_in_a_workspace_give_the_same_bits(cuda, on_device, offline):
    from facodec_amd import ops
    got = ops.denoise(on_device["x"], lens=on_device["lens"], keep_spectra=True)
    assert np.array_equal(bits(got.y), bits(offline[(8, 96)].y)) and torch.equal(got.G, offline[(8, 96)].G)


def test_denoise_clips_does_not_depend_on_the_grouping(cuda):
    from facodec_amd import commons, ops
    lengths = [24000, 4800, 48000, 11111, 30001]
    clips = [torch.from_numpy(broadband(n, 61 + i)).to(cuda) for i, n in enumerate(lengths)]
    clips[2] = clips[2][None]
    assert len(commons.plan_groups(lengths, 60002)) == 3
    got = commons.denoise_clips(clips, max_batch_samples=60002, W=20)
    one = commons.denoise_clips(clips, W=20)
    for c, n, a, b in zip(clips, lengths, got, one):
        alone = ops.denoise(c.reshape(1, -1), W=20)
        assert a.y.shape == b.y.shape == (n,) and a.G.shape == b.G.shape == (n_frames(n), BINS)
        for r in (a, b):
            assert np.array_equal(bits(r.y), bits(alone.y[0])) and torch.equal(r.G, alone.G[0])
    assert float(got[0].G.min()) < 0.5


@pytest.mark.parametrize("at", [2400, 2560])
def test_reset_rows_is_the_offline_call_with_starts(cuda, streams, at):
    """Row 1 is reset after `at` samples (2400: inside a frame; 2560: on the hop grid): from there on it gives, 512 samples late,
    ops.denoise of the whole input with starts = at -- whatever lay before the start counts as zero, and the 512 samples of
    the old stream that were not played yet come out as zeros.  Row 0 goes on as if nothing had happened."""
    from facodec_amd import ops
    from facodec_amd.streaming import NoiseSuppressor
    n = 12000
    x = streams["x"][:2, :n].contiguous()
    starts = torch.tensor([0, at], dtype=torch.int32, device=cuda)
    want = ops.denoise(x, starts=starts, M=2, W=5)
    zeroed = x.clone()
    zeroed[1, :at] = 0.0
    same = ops.denoise(zeroed, starts=starts, M=2, W=5)
    assert np.array_equal(bits(same.y), bits(want.y)) and torch.equal(same.G, want.G)
    assert torch.all(want.y[1, :at] == 0.0) and torch.all(want.G[1, :at // H] == 1.0)
    ns = NoiseSuppressor(2, M=2, W=5, ring=16)
    out = [ns.push(x[:, :at])]
    ns.reset([1])
    out += [ns.push(x[:, t:t + 480]) for t in range(at, n, 480)]
    out.append(ns.finish())
    got = torch.cat(out, dim=-1)
    assert got.shape == (2, n + DELAY)
    assert np.array_equal(bits(got[0, DELAY:]), bits(want.y[0]))
    assert np.array_equal(bits(got[1, at:]), bits(want.y[1, at - DELAY:]))
    assert torch.all(got[1, at:at + DELAY] == 0.0) and float(got[1, at + DELAY:].abs().max()) > 0.0
    k = 16
    assert torch.equal(ns.gains(k), want.G[:, n_frames(n) - k:])


# ---------------------------------------------------------------------------------------------- 4: identity
def test_no_attenuation_returns_the_input(cuda, on_device):
    from facodec_amd import ops
    got = ops.denoise(on_device["x"], lens=on_device["lens"], max_atten_db=0.0)
    assert torch.all(got.G == 1.0)
    for b, n in enumerate(LENS):
        if n:
            x = on_device["x"][b, :n]
            err = float((got.y[b, :n].double() - x.double()).abs().max()) / float(x.abs().max())
            print(f"identity row {b}: {err * 2 ** 23:.3f} x 2^-23 of the row's largest")
            assert err <= 2.0 ** -23
        assert torch.all(got.y[b, n:] == 0.0)


# ---------------------------------------------------------------------------------------------- 5: sessions
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


def _same_dicts(got, want):
    n_codes = 0
    assert len(got) == len(want)
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


@pytest.mark.parametrize("order", ["denoise", "denoise-level", "level-denoise"])
def test_denoised_session(full_model, cuda, order):
    """A StreamingCodec behind DenoisedSession, and both nestings with LevelledSession: the dicts are those of the bare session
    fed the stages' outputs, the outer stage first."""
    from facodec_amd.streaming import HOP, AutoGain, DenoisedSession, LevelledSession, NoiseSuppressor, StreamingCodec
    m = full_model
    n_hops = 5                                                               # 7200 samples: a multiple of the codec's 300-sample frame
    n = 4800 + n_hops * HOP
    wave = (0.02 * synth.synth_clips(2, n, seed=47)).to(cuda)
    wave = wave + torch.from_numpy(np.stack([broadband(n, 71 + b) for b in range(2)]))[:, None].to(cuda)
    blocks = [wave[:, :, :4800]] + [wave[:, :, 4800 + h * HOP:4800 + (h + 1) * HOP] for h in range(n_hops)]
    ns_kw, agc_kw = dict(M=2, W=5), dict(window=5, lookahead=120)
    with torch.no_grad():
        timbre = m.quantizer(m.encoder(wave), wave, n_c=2, return_codes=True)[4].clone()
        codec = StreamingCodec(m, timbre, n_c=2, use_graphs=False)
        ns, agc = NoiseSuppressor(2, **ns_kw), AutoGain(2, 24000, **agc_kw)
        if order == "denoise":
            stages, sess, lat = [ns], DenoisedSession(codec, **ns_kw), DELAY / 24000
        elif order == "denoise-level":
            stages, sess, lat = [ns, agc], DenoisedSession(LevelledSession(codec, **agc_kw), **ns_kw), (DELAY + 120) / 24000
        else:
            stages, sess, lat = [agc, ns], LevelledSession(DenoisedSession(codec, **ns_kw), **agc_kw), (DELAY + 120) / 24000
        assert abs(sess.latency_in - lat) < 1e-12 and sess.prime_samples == 4800
        fed = []
        for blk in blocks:
            for st in stages:
                blk = st.push(blk)
            fed.append(blk)
        assert not torch.equal(torch.cat(fed, dim=-1), wave)                    # the session does not see the raw input
        bare = StreamingCodec(m, timbre, n_c=2, use_graphs=False)
        want = [_keep(bare.prime(fed[0]))] + [_keep(bare.push(f)) for f in fed[1:]] + [_keep(bare.finish())]
        got = [_keep(sess.prime(blocks[0]))] + [_keep(sess.push(b)) for b in blocks[1:]] + [_keep(sess.finish())]
    _same_dicts(got, want)


# ---------------------------------------------------------------------------------------------- 6: the synthetic mix
def test_synthetic_mix_bounds_on_the_device(cuda):
    """The CPU test's 10 dB mix, seed 0, defaults: the noise-only stretch falls by at least 12 dB and the SI-SDR over the tone
    (ops.si_sdr) rises by at least 7 dB."""
    from facodec_amd import ops
    s, x, speech, quiet = synthetic_mix(0)
    xd = torch.from_numpy(x)[None].to(cuda)
    y = ops.denoise(xd).y
    q = torch.from_numpy(quiet).to(cuda)
    att = 10.0 * float(torch.log10(xd[0, q].double().square().sum() / y[0, q].double().square().sum()))
    i0, i1 = int(np.argmax(speech)), len(speech) - int(np.argmax(speech[::-1]))
    assert speech[i0:i1].all() and speech.sum() == i1 - i0
    sd = torch.from_numpy(s.astype(np.float32))[None, i0:i1].to(cuda)
    before, after = float(ops.si_sdr(sd, xd[:, i0:i1].contiguous())[0]), float(ops.si_sdr(sd, y[:, i0:i1].contiguous())[0])
    print(f"device, seed 0: noise-only attenuation {att:.2f} dB, SI-SDR {before:.2f} -> {after:.2f} dB")
    assert att >= 12.0
    assert after - before >= 7.0


# ---------------------------------------------------------------------------------------------- 7: refusals
def test_refusals_before_any_launch(cuda):
    check_refusals()
    from facodec_amd import ops
    from facodec_amd.streaming import NoiseSuppressor
    ns = NoiseSuppressor(2)
    with pytest.raises(ValueError):
        ns.push(torch.zeros(2, 0, device=cuda))
    with pytest.raises(ValueError):
        ns.push(torch.zeros(3, 480, device=cuda))
    with pytest.raises(ValueError):
        ns.gains(1)
    with pytest.raises(ValueError):
        ns.reset([2])
    with pytest.raises(ValueError, match="carry_in"):
        ops.ns_synth(torch.zeros(2, 480, device=cuda), ns._G, carry_in=torch.zeros(2, 7, device=cuda))
    with pytest.raises(ValueError, match="starts"):
        ops.denoise(torch.zeros(2, 480, device=cuda), starts=torch.zeros(3, dtype=torch.int32, device=cuda))
    P = torch.zeros(2, 20, BINS, device=cuda, dtype=torch.float64)
    with pytest.raises(_lib.FacodecHipError, match="R = 20"):                  # the C entry speaks through fac_last_error
        ops.ns_gains(P, ops.ns_params(), f0=1000, n_new=20)
    with pytest.raises(_lib.FacodecHipError, match="in front of n0"):
        ops.ns_synth(torch.zeros(2, 480, device=cuda), ns._G, n0=4800, m0=4800 - 1024, n_out=480, carry_in=ns._carry[0])
    ns.finish()
    with pytest.raises(RuntimeError):
        ns.push(torch.zeros(2, 480, device=cuda))
