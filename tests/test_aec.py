"""Echo cancellation on the device: fac_aec_run and what is built on it (ops.echo_cancel, streaming.EchoCanceller /
EchoCancelledSession, commons.echo_cancel_clips) against the fp64 numpy restatement of the header's definition in
tests/test_aec_cpu.py.

Against the restatement only broadband rows are compared: the far end is test_denoise_cpu's broadband() (Gaussian noise of at
least 1e-3 of the row's peak plus louder bursts), the microphone is the far end through a short random path plus an independent
broadband row, so every bin of every block holds power far above the rounding of the rest and no step divides rounding noise by
rounding noise.  Bounds, those of tests/test_denoise.py for the same transform: e within 2^-22 of the row's largest microphone
sample (one fp32 rounding plus fp64 noise), W within 1e-9 of the row's largest |W| (the recursion carries the transform's
1e-16 per block over 118 blocks; a wrong partition, a missing constraint or a swapped conjugate moves it by 1e-3 or more), the
block statistics within 1e-12 of the reference's own value.  Device against device -- streamed against offline, a row alone
against the row in a batch, grouped clips, a reset row against the offline call with `starts` -- is bit for bit.

Measured on an MI355X (worst over the rows of the batch and the three (P, delay)): e 0 (every sample rounds to the restatement's
float), W 2.1e-15, stats 1.2e-13 -- on the row of 2561 samples at P = 8, which has blocks whose estimate lies three orders of
magnitude below the far end it is summed from, so that its square carries that much more relative rounding; 7.3e-15 at worst on
the other two settings."""
import numpy as np
import pytest
import torch

from facodec_amd import _lib, synth
from test_aec_cpu import (BINS, DELAY, ERLE_EARLY_MIN, ERLE_LATE_MIN, FS, H, SI_SDR_NEAR_MIN, aec_ref, broadband_pair, check_refusals,
                          n_blocks, synthetic_call)

pytestmark = pytest.mark.gpu

T = 30000
LENS = (30000, 2561, 256, 255, 1, 0)      # many blocks; one sample into a new block; exactly one block; one less; one sample; empty
PD = [(8, 0), (2, 300), (32, 0)]          # W and X in LDS; the same with a delayed far end; W and X in global memory
PD_IDS = ["P8", "P2-delay300", "P32"]
FIRST = [(1, 7, 479, 2400), ()]
FIRST_IDS = ["ragged-blocks", "480-hops"]


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
    """Six rows of one launch, computed once and never written to; what lies behind a row's end is 7.0 in both signals and must
    never be read."""
    rows = [broadband_pair(n, 31 + b) for b, n in enumerate(LENS)]
    mic = np.full((len(LENS), T), 7.0, dtype=np.float32)
    far = np.full((len(LENS), T), 7.0, dtype=np.float32)
    for b, (m, f) in enumerate(rows):
        mic[b, :len(m)], far[b, :len(f)] = m, f
    return dict(rows=rows, mic=mic, far=far)


@pytest.fixture(scope="module")
def on_device(cuda, batch):
    return dict(mic=torch.from_numpy(batch["mic"]).to(cuda), far=torch.from_numpy(batch["far"]).to(cuda),
                lens=torch.tensor(LENS, dtype=torch.int32, device=cuda))


@pytest.fixture(scope="module")
def refs(batch):
    """(e, W, stats) of the restatement per (P, delay) and row, at the batch's width."""
    return {pd: [aec_ref(m, f, P=pd[0], delay=pd[1], T=T) for m, f in batch["rows"]] for pd in PD}


@pytest.fixture(scope="module")
def offline(cuda, on_device):
    from facodec_amd import ops
    return {pd: ops.echo_cancel(on_device["mic"], on_device["far"], lens=on_device["lens"], P=pd[0], delay=pd[1]) for pd in PD}


def _complex(W):
    W = W.cpu().numpy()
    return W[..., 0] + 1j * W[..., 1]


# ---------------------------------------------------------------------------------------------- 1: against the restatement
@pytest.mark.parametrize("pd", PD, ids=PD_IDS)
def test_error_weights_and_statistics_of_a_ragged_batch(cuda, on_device, refs, offline, pd):
    got = offline[pd]
    M = n_blocks(T)
    assert got.e.shape == on_device["mic"].shape and got.e.dtype == torch.float32
    assert got.W.shape == (len(LENS), pd[0], BINS, 2) and got.W.dtype == torch.float64 and got.stats.shape == (len(LENS), M, 3)
    e, W, stats = got.e.cpu().numpy(), _complex(got.W), got.stats.cpu().numpy()
    worst = dict(e=0.0, W=0.0, stats=0.0)
    for b, n in enumerate(LENS):
        e_ref, W_ref, s_ref = refs[pd][b]
        assert (e[b, n:] == 0.0).all() and (stats[b, n_blocks(n):] == 0.0).all()
        if n == 0:
            assert (W[b] == 0.0).all()
            continue
        peak = float(np.abs(on_device["mic"][b, :n].cpu().numpy()).max())
        ee = float(np.abs(e[b].astype(np.float64) - e_ref.astype(np.float64)).max()) / peak
        wmax = float(np.abs(W_ref).max())
        eW = float(np.abs(W[b] - W_ref).max()) / wmax if wmax > 0 else float(np.abs(W[b]).max())
        nz = s_ref != 0.0
        assert (stats[b][~nz] == 0.0).all()
        es = float((np.abs(stats[b] - s_ref)[nz] / s_ref[nz]).max())
        print(f"{pd} row {b} (len {n}): e {ee:.3g} of the peak = {ee * 2 ** 23:.3f} x 2^-23, W {eW:.3g} of the largest, stats {es:.3g}")
        worst = dict(e=max(worst["e"], ee), W=max(worst["W"], eW), stats=max(worst["stats"], es))
        assert ee <= 2.0 ** -22
        assert eW <= 1e-9
        assert es <= 1e-12
    print(f"{pd} worst: {worst}")
    s = got.stats[0]
    assert float(s[:, 2].sum() / s[:, 0].sum()) < 0.5                           # the canceller has work: it removes most of the microphone


# ---------------------------------------------------------------------------------------------- 2: streamed against offline
@pytest.fixture(scope="module")
def streams(cuda):
    """Three full rows for the streaming tests and their offline results per (P, delay)."""
    from facodec_amd import ops
    pairs = [broadband_pair(T, 51 + b) for b in range(3)]
    mic = torch.from_numpy(np.stack([p[0] for p in pairs])).to(cuda)
    far = torch.from_numpy(np.stack([p[1] for p in pairs])).to(cuda)
    return dict(mic=mic, far=far, off={pd: ops.echo_cancel(mic, far, P=pd[0], delay=pd[1]) for pd in PD})


def _stream(aec, mic, far, first, hop=480):
    out, t = [], 0
    for k in _blocks(first, hop, mic.shape[-1]):
        out.append(aec.push(mic[..., t:t + k], far[..., t:t + k]))
        assert out[-1].shape == mic[..., t:t + k].shape
        t += k
    out.append(aec.finish())
    return torch.cat(out, dim=-1)


@pytest.mark.parametrize("first", FIRST, ids=FIRST_IDS)
@pytest.mark.parametrize("pd", PD, ids=PD_IDS)
def test_streamed_equals_offline_bit_for_bit(cuda, streams, pd, first):
    """Any chunking gives 256 zeros and then the offline call's bits, finish() included, and leaves the offline call's weights."""
    from facodec_amd.streaming import EchoCanceller
    off = streams["off"][pd]
    aec = EchoCanceller(3, P=pd[0], delay=pd[1])
    assert aec.delay == DELAY and aec.latency == DELAY / 24000 and aec.far_delay == pd[1]
    got = _stream(aec, streams["mic"], streams["far"], first)
    assert aec.samples == T and got.shape == (3, T + DELAY)
    assert torch.all(got[:, :DELAY] == 0.0)
    assert np.array_equal(bits(got[:, DELAY:]), bits(off.e))
    assert torch.equal(aec.weights(), off.W)


def test_streamed_three_dimensional_blocks_and_short_streams(cuda, streams):
    from facodec_amd import ops
    from facodec_amd.streaming import EchoCanceller
    for n in (1, 255, 256, 257, 700):
        mic, far = streams["mic"][:1, None, :n].contiguous(), streams["far"][:1, None, :n].contiguous()
        aec = EchoCanceller(1)
        got = torch.cat([aec.push(mic, far), aec.finish()[:, None]], dim=-1)
        assert got.shape == (1, 1, n + DELAY) and torch.all(got[..., :DELAY] == 0.0)
        off = ops.echo_cancel(mic, far)
        assert np.array_equal(bits(got[..., DELAY:]), bits(off.e)) and torch.equal(aec.weights(), off.W)


# ---------------------------------------------------------------------------------------------- 3: other bit-for-bit checks
@pytest.mark.parametrize("pd", PD, ids=PD_IDS)
def test_a_row_alone_equals_the_row_in_the_batch(cuda, on_device, offline, pd):
    from facodec_amd import ops
    for b, n in enumerate(LENS):
        alone = ops.echo_cancel(on_device["mic"][b:b + 1, :n].contiguous(), on_device["far"][b:b + 1, :n].contiguous(), P=pd[0], delay=pd[1])
        assert alone.e.shape == (1, n) and alone.stats.shape == (1, n_blocks(n), 3)
        assert np.array_equal(bits(alone.e[0]), bits(offline[pd].e[b, :n]))
        assert torch.equal(alone.W[0], offline[pd].W[b]) and torch.equal(alone.stats[0], offline[pd].stats[b, :n_blocks(n)])


def test_echo_cancel_clips_does_not_depend_on_the_grouping(cuda):
    from facodec_amd import commons, ops
    lengths = [24000, 4800, 48000, 11111, 30001]
    pairs = [broadband_pair(n, 61 + i) for i, n in enumerate(lengths)]
    mics, fars = [torch.from_numpy(p[0]).to(cuda) for p in pairs], [torch.from_numpy(p[1]).to(cuda) for p in pairs]
    mics[2], fars[2] = mics[2][None], fars[2][None]
    assert len(commons.plan_groups(lengths, 60002)) == 3
    got = commons.echo_cancel_clips(mics, fars, max_batch_samples=60002, P=4)
    one = commons.echo_cancel_clips(mics, fars, P=4)
    for m, f, n, a, b in zip(mics, fars, lengths, got, one):
        alone = ops.echo_cancel(m.reshape(1, -1), f.reshape(1, -1), P=4)
        assert a.e.shape == b.e.shape == (n,) and a.W.shape == b.W.shape == (4, BINS, 2) and a.stats.shape == b.stats.shape == (n_blocks(n), 3)
        for r in (a, b):
            assert np.array_equal(bits(r.e), bits(alone.e[0])) and torch.equal(r.W, alone.W[0]) and torch.equal(r.stats, alone.stats[0])
    assert float(got[0].W.abs().max()) > 0.0


@pytest.mark.parametrize("at", [2400, 2560])
def test_reset_rows_is_the_offline_call_with_starts(cuda, streams, at):
    """Row 1 is reset after `at` samples (2400: inside a block; 2560: on the block grid): from there on it gives, 256 samples late,
    ops.echo_cancel of the whole input with starts = at -- whatever lay before the start counts as zero in both signals, the
    filter starts from zero, and the 256 samples of the old stream that were not played yet come out as zeros.  Row 0 goes on
    as if nothing had happened."""
    from facodec_amd import ops
    from facodec_amd.streaming import EchoCanceller
    n = 12000
    mic, far = streams["mic"][:2, :n].contiguous(), streams["far"][:2, :n].contiguous()
    starts = torch.tensor([0, at], dtype=torch.int32, device=cuda)
    want = ops.echo_cancel(mic, far, starts=starts, P=2, delay=300)
    zm, zf = mic.clone(), far.clone()
    zm[1, :at], zf[1, :at] = 0.0, 0.0
    same = ops.echo_cancel(zm, zf, starts=starts, P=2, delay=300)
    assert np.array_equal(bits(same.e), bits(want.e)) and torch.equal(same.W, want.W)
    assert torch.all(want.e[1, :at] == 0.0) and torch.all(want.stats[1, :at // H] == 0.0)
    assert torch.equal(want.e[0], ops.echo_cancel(mic[:1], far[:1], P=2, delay=300).e[0])
    aec = EchoCanceller(2, P=2, delay=300)
    out = [aec.push(mic[:, :at], far[:, :at])]
    aec.reset([1])
    out += [aec.push(mic[:, t:t + 480], far[:, t:t + 480]) for t in range(at, n, 480)]
    out.append(aec.finish())
    got = torch.cat(out, dim=-1)
    assert got.shape == (2, n + DELAY)
    assert np.array_equal(bits(got[0, DELAY:]), bits(want.e[0]))
    assert np.array_equal(bits(got[1, at:]), bits(want.e[1, at - DELAY:]))
    assert torch.all(got[1, at:at + DELAY] == 0.0) and float(got[1, at + DELAY:].abs().max()) > 0.0
    assert torch.equal(aec.weights(), want.W)


def test_set_adapt_freezes_the_weights_of_those_rows(cuda, streams):
    """Row 1 stops adapting at a block edge: its weights() no longer change, it still filters (bit for bit the offline call on
    the rest of the signal would need the frozen filter, so the check is on the weights and on the output's being neither mic
    nor the adapting row's); row 0 goes on as the offline call."""
    from facodec_amd.streaming import EchoCanceller
    n, at = 12000, 10 * H
    mic, far = streams["mic"][:2, :n].contiguous(), streams["far"][:2, :n].contiguous()
    mic[1], far[1] = mic[0], far[0]                                              # two copies of one call
    aec = EchoCanceller(2)
    out = [aec.push(mic[:, :at], far[:, :at])]
    frozen = aec.weights()
    assert torch.equal(frozen[0], frozen[1]) and float(frozen.abs().max()) > 0.0
    aec.set_adapt([1], False)
    out += [aec.push(mic[:, t:t + 480], far[:, t:t + 480]) for t in range(at, n, 480)]
    out.append(aec.finish())
    W = aec.weights()
    assert torch.equal(W[1], frozen[1]) and not torch.equal(W[0], frozen[0])
    got = torch.cat(out, dim=-1)
    full = n // H * H                                                             # the offline call's last block here is not cut off at n
    assert np.array_equal(bits(got[0, DELAY:DELAY + full]), bits(streams["off"][(8, 0)].e[0, :full]))
    assert np.array_equal(bits(got[1, :at + DELAY]), bits(got[0, :at + DELAY]))   # the same until the first block without an update is out,
    assert not torch.equal(got[1, at + H + DELAY:], got[0, at + H + DELAY:])      # (block 10 still used the weights both rows had) then not
    assert not torch.equal(got[1, DELAY:], mic[1])
    aec.set_adapt([1], True)                                                      # accepted after finish(): only a flag


# ---------------------------------------------------------------------------------------------- 4: pass-through
def test_a_silent_far_end_or_no_step_returns_the_microphone(cuda, on_device):
    from facodec_amd import ops
    mic, far, lens = on_device["mic"], on_device["far"], on_device["lens"]
    for got in (ops.echo_cancel(mic, torch.zeros_like(far), lens=lens), ops.echo_cancel(mic, far, lens=lens, mu=0.0),
                ops.echo_cancel(mic, far, lens=lens, adapt=False), ops.echo_cancel(mic, torch.zeros_like(far), lens=lens, P=32, delta=0.0)):
        assert torch.all(got.W == 0.0)
        for b, n in enumerate(LENS):
            assert torch.all(got.e[b, :n] == mic[b, :n]) and torch.all(got.e[b, n:] == 0.0)
        assert torch.all(got.stats[..., 1] == 0.0) and torch.equal(got.stats[..., 0], got.stats[..., 2])
    some = ops.echo_cancel(mic, far, lens=lens, adapt=[True, False, True, False, True, False])
    assert torch.equal(some.e[0], ops.echo_cancel(mic, far, lens=lens).e[0]) and torch.all(some.e[1, :LENS[1]] == mic[1, :LENS[1]])


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


@pytest.mark.parametrize("order", ["cancel", "cancel-denoise-level"])
def test_echo_cancelled_session(full_model, cuda, order):
    """A StreamingCodec behind EchoCancelledSession, alone and around DenoisedSession(LevelledSession(..)): the dicts are those
    of the bare session fed the stages' outputs, the canceller first."""
    from facodec_amd.streaming import (HOP, AutoGain, DenoisedSession, EchoCancelledSession, EchoCanceller, LevelledSession, NoiseSuppressor,
                                       StreamingCodec)
    m = full_model
    n_hops = 5                                                               # 7200 samples: a multiple of the codec's 300-sample frame
    n = 4800 + n_hops * HOP
    pairs = [broadband_pair(n, 71 + b) for b in range(2)]
    far = torch.from_numpy(np.stack([p[1] for p in pairs]))[:, None].to(cuda)
    wave = (0.02 * synth.synth_clips(2, n, seed=47)).to(cuda) + torch.from_numpy(np.stack([p[0] for p in pairs]))[:, None].to(cuda)
    cut = [(0, 4800)] + [(4800 + h * HOP, 4800 + (h + 1) * HOP) for h in range(n_hops)]
    aec_kw, ns_kw, agc_kw = dict(P=2, delay=10), dict(M=2, W=5), dict(window=5, lookahead=120)
    with torch.no_grad():
        timbre = m.quantizer(m.encoder(wave), wave, n_c=2, return_codes=True)[4].clone()
        codec = StreamingCodec(m, timbre, n_c=2, use_graphs=False)
        aec, ns, agc = EchoCanceller(2, **aec_kw), NoiseSuppressor(2, **ns_kw), AutoGain(2, 24000, **agc_kw)
        if order == "cancel":
            stages, sess, lat = [], EchoCancelledSession(codec, **aec_kw), DELAY / 24000
        else:
            stages, sess = [ns, agc], EchoCancelledSession(DenoisedSession(LevelledSession(codec, **agc_kw), **ns_kw), **aec_kw)
            lat = (DELAY + 512 + 120) / 24000
        assert abs(sess.latency_in - lat) < 1e-12 and sess.prime_samples == 4800
        fed = []
        for a, b in cut:
            blk = aec.push(wave[:, :, a:b], far[:, :, a:b])
            for st in stages:
                blk = st.push(blk)
            fed.append(blk)
        assert not torch.equal(torch.cat(fed, dim=-1), wave)                    # the session does not see the raw input
        bare = StreamingCodec(m, timbre, n_c=2, use_graphs=False)
        want = [_keep(bare.prime(fed[0]))] + [_keep(bare.push(f)) for f in fed[1:]] + [_keep(bare.finish())]
        got = [_keep(sess.prime(wave[:, :, :4800], far[:, :, :4800]))] + [_keep(sess.push(wave[:, :, a:b], far[:, :, a:b])) for a, b in cut[1:]]
        got.append(_keep(sess.finish()))
    _same_dicts(got, want)


# ---------------------------------------------------------------------------------------------- 6: the synthetic call
def test_synthetic_call_bounds_on_the_device(cuda):
    """The CPU test's two-way call, seed 0, defaults, against its bounds (the restatement's figures less 3 dB): ERLE over
    2 .. 3 s and over 4.5 .. 5.5 s by plain sums, the near-end SI-SDR over 3 .. 4 s by ops.si_sdr."""
    from facodec_amd import ops
    mic, far, echo, near = synthetic_call(0)
    md, fd = torch.from_numpy(mic)[None].to(cuda), torch.from_numpy(far)[None].to(cuda)
    e = ops.echo_cancel(md, fd).e
    ed = torch.from_numpy(echo)[None].to(cuda)

    def erle(a, b):
        return 10.0 * float(torch.log10(ed[0, a:b].square().sum() / e[0, a:b].double().square().sum()))

    early, late = erle(2 * FS, 3 * FS), erle(int(4.5 * FS), int(5.5 * FS))
    a, b = 3 * FS, 4 * FS
    nd = torch.from_numpy(near.astype(np.float32))[None, a:b].to(cuda)
    before, after = float(ops.si_sdr(nd, md[:, a:b].contiguous())[0]), float(ops.si_sdr(nd, e[:, a:b].contiguous())[0])
    print(f"device, seed 0: ERLE {early:.2f} dB over 2 .. 3 s, {late:.2f} dB over 4.5 .. 5.5 s, near-end SI-SDR {before:.2f} -> {after:.2f} dB")
    assert early >= ERLE_EARLY_MIN
    assert late >= ERLE_LATE_MIN
    assert after >= SI_SDR_NEAR_MIN


# ---------------------------------------------------------------------------------------------- 7: refusals
def test_refusals_before_any_launch(cuda):
    check_refusals()
    from facodec_amd import ops
    from facodec_amd.streaming import EchoCanceller
    aec = EchoCanceller(2)
    z = torch.zeros(2, 480, device=cuda)
    with pytest.raises(ValueError):
        aec.push(torch.zeros(2, 0, device=cuda), torch.zeros(2, 0, device=cuda))
    with pytest.raises(ValueError):
        aec.push(torch.zeros(3, 480, device=cuda), torch.zeros(3, 480, device=cuda))
    with pytest.raises(ValueError):
        aec.push(z, torch.zeros(2, 481, device=cuda))
    with pytest.raises(ValueError):
        aec.reset([2])
    with pytest.raises(ValueError, match="differ"):
        ops.echo_cancel(z, torch.zeros(2, 481, device=cuda))
    with pytest.raises(ValueError, match="starts"):
        ops.echo_cancel(z, z, starts=torch.zeros(3, dtype=torch.int32, device=cuda))
    with pytest.raises(ValueError, match="negative"):
        ops.echo_cancel(z, z, starts=torch.tensor([0, -1], dtype=torch.int32))
    with pytest.raises(ValueError, match="adapt"):
        ops.echo_cancel(z, z, adapt=[True])
    p = ops.aec_params()
    with pytest.raises(ValueError, match="far carry"):
        ops.aec_run(z, z, p, aec._W, aec._X, far_carry=(torch.zeros(2, 7, device=cuda), None))
    with pytest.raises(_lib.FacodecHipError, match="W and X are the same buffer"):     # the C entry speaks through fac_last_error
        ops.aec_run(z, z, p, aec._W, aec._W)
    with pytest.raises(_lib.FacodecHipError, match="lens does not go with a carried stream"):
        ops.aec_run(z, z, p, aec._W, aec._X, lens=torch.tensor([480, 480], dtype=torch.int32, device=cuda), e_ring=aec._ring)
    with pytest.raises(_lib.FacodecHipError, match="starts more than 255 samples in front"):
        ops.aec_run(z, z, p, aec._W, aec._X, n0=4800, m0=4800 - 256, blk0=17, n_blk=2, mic_carry=(aec._mic[0], aec._mic[1]))
    aec.finish()
    with pytest.raises(RuntimeError):
        aec.push(z, z)
