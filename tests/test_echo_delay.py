"""The echo delay tracker on the GPU: fac_edelay_run against the numpy restatement of tests/test_echo_delay_cpu.py
-- decisions frame by frame where the restatement can decide them, conf, score and C to a relative bound, the aligned far end
as a bit-exact gather -- then what the stream, the batch and the composites promise bit for bit, the synthetic call end to
end, and the refusals."""
import numpy as np
import pytest
import torch

from facodec_amd import _lib, synth
from test_aec_cpu import FS, broadband_pair
from test_echo_delay_cpu import BINS, H, call_run, check_refusals, delay_ref, erle_late_auto, gather, locks_of, n_frames, policy

pytestmark = pytest.mark.gpu

T = 30000
LENS = (30000, 2561, 768, 767, 512, 511, 1, 0)      # many frames; nine; two; one (a sample short of two); one; none; none; empty
KW = [dict(), dict(max_delay=512), dict(max_delay=300), dict(k_lo=3, k_hi=103, max_delay=512)]     # L = 64, 2, 2 (ceil); 100 bins
KW_IDS = ["L64", "max512", "max300", "band100"]
# conf, score and C against the restatement, relative to the row's largest value: the canceller's precedent for W.  Measured: DESIGN.md 36.4
REL = 1e-9
DECIDABLE = 1e-6


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float32).view(np.int32)


def _blocks(first, hop, total):
    sizes, n = list(first), sum(first)
    while n < total:
        sizes.append(min(hop, total - n))
        n += sizes[-1]
    return sizes


@pytest.fixture(scope="module")
def batch():
    """Eight rows of one launch, computed once and never written to; what lies behind a row's end is 7.0 in both signals and
    must never be read."""
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


def _check_row(got, b, ref, far_row, length, start=0, state=None, report=None):
    """Row b of an EchoDelay against the restatement `ref` of that row (its frames are first .. first + F - 1)."""
    first, F = ref.mfirst, len(ref.raw)
    M = got.raw.shape[1]
    cols = slice(first - 1, first - 1 + F)
    raw, locked, used = (t[b].cpu().numpy().astype(np.int64) for t in (got.raw, got.locked, got.used))
    conf, ok, score = got.conf[b].cpu().numpy(), got.ok[b].cpu().numpy(), got.score[b].cpu().numpy()
    outside = np.ones(M, dtype=bool)
    outside[cols] = False
    assert (raw[outside] == -1).all() and (locked[outside] == -1).all() and (used[outside] == -1).all()
    assert (conf[outside] == 0.0).all() and (ok[outside] == 0).all() and (score[outside] == 0.0).all()
    p = ref.p
    if F:
        margins = np.array(ref.margins)
        decidable = (margins > DECIDABLE).all(axis=1)
        quiet = np.array(ref.conf) < p["thr"] / 2                          # no peak to speak of: only ok is compared
        assert (~decidable).sum() <= 0.01 * F, f"{(~decidable).sum()} of {F} frames undecidable"
        r_raw, r_ok = np.array(ref.raw), np.array(ref.ok).astype(np.uint8)
        full = decidable & ~quiet
        assert np.array_equal(raw[cols][full], r_raw[full])
        assert np.array_equal(ok[cols][decidable], r_ok[decidable])
        if np.array_equal(ok[cols], r_ok) and np.array_equal(raw[cols][r_ok == 1], r_raw[r_ok == 1]):
            assert np.array_equal(locked[cols], np.array(ref.locked)) and np.array_equal(used[cols], np.array(ref.used))
        # always: the device's latch is the policy on the device's own raw and ok
        want_locked, want_used = policy(raw[cols], ok[cols], p["hold"], p["tol"], p["move"], p["margin"], p["delay0"])
        assert np.array_equal(locked[cols], want_locked) and np.array_equal(used[cols], want_used)
        rs = np.array(ref.score)
        top = rs.max()
        e_conf = np.abs(conf[cols] - np.array(ref.conf)).max() / top
        e_score = np.abs(score[cols] - rs).max() / top
        assert e_conf <= REL and e_score <= REL, (e_conf, e_score)
        if state is not None:
            C = state["C"][b].cpu().numpy()
            C = (C[..., 0] + 1j * C[..., 1])[:, p["k_lo"]:p["k_hi"]]
            e_c = np.abs(C - ref.C).max() / np.abs(ref.C).max()
            assert e_c <= REL, e_c
            if report is not None:
                report.append((F, int((~decidable).sum()), e_conf, e_score, e_c, margins.min(axis=0)))
    y = got.far[b].cpu().numpy()
    want = gather(far_row[:length], used[cols], first, start, p["delay0"])
    assert np.array_equal(bits(y[:length]), bits(want)) and (y[length:] == 0.0).all() and (y[:start] == 0.0).all()


@pytest.mark.parametrize("kw", KW, ids=KW_IDS)
def test_decisions_scores_and_alignment_of_a_ragged_batch(cuda, batch, on_device, kw):
    from facodec_amd import ops
    p = ops.echo_delay_params(**kw)
    state = ops.edelay_state(len(LENS), p, cuda)
    got = ops.echo_delay(on_device["mic"], on_device["far"], lens=on_device["lens"], state=state, **kw)
    assert got.far.shape == (len(LENS), T) and got.raw.shape == (len(LENS), n_frames(T)) and got.score.shape == (len(LENS), n_frames(T), p.L + 1)
    report = []
    for b, (n, (m, f)) in enumerate(zip(LENS, batch["rows"])):
        ref = delay_ref(m, f, **kw)
        assert len(ref.raw) == n_frames(n)
        _check_row(got, b, ref, batch["far"][b], n, state=state, report=report)
    F, und, e_conf, e_score, e_c, margins = report[0]
    print(f"{kw}: row 0: {und} of {F} frames undecidable, smallest margins (score, |g|, thr) {margins}; worst relative error of conf "
          f"{max(r[2] for r in report):.2e}, of score {max(r[3] for r in report):.2e}, of C {max(r[4] for r in report):.2e}")
    locks = locks_of(got.locked[0].tolist())
    assert len(locks) == 1 and 320 <= locks[0][1] < 470                        # the path's lead
    assert int(got.locked[1:].max()) == -1                                     # nine frames and fewer: hold = 8 is not reached above thr


def test_starts_in_mid_block(cuda, batch):
    from facodec_amd import ops
    n = 12000
    starts = (0, 2400, 2560, 300)
    rows = [broadband_pair(n - s, 41 + b) for b, s in enumerate(starts)]
    mic = np.stack([np.concatenate([np.full(s, 0.5, dtype=np.float32), m]) for s, (m, f) in zip(starts, rows)])
    far = np.stack([np.concatenate([np.full(s, 0.5, dtype=np.float32), f]) for s, (m, f) in zip(starts, rows)])
    st = torch.tensor(starts, dtype=torch.int64, device=cuda)
    p = ops.echo_delay_params(max_delay=512)
    state = ops.edelay_state(4, p, cuda)
    got = ops.echo_delay(torch.from_numpy(mic).to(cuda), torch.from_numpy(far).to(cuda), starts=st, state=state, max_delay=512)
    for b, s in enumerate(starts):
        ref = delay_ref(mic[b], far[b], start=s, max_delay=512)
        assert ref.mfirst == s // H + 1
        _check_row(got, b, ref, far[b], n, start=s, state=state)
    assert int(got.locked[0].max()) >= 320 and int(got.used.max()) >= 192         # the aligner moved something


# ---------------------------------------------------------------------------------------------- streaming
@pytest.fixture(scope="module")
def streams(cuda):
    n = 12000
    pairs = [broadband_pair(n, 51 + b) for b in range(3)]
    return dict(n=n, mic=torch.from_numpy(np.stack([p[0] for p in pairs])).to(cuda), far=torch.from_numpy(np.stack([p[1] for p in pairs])).to(cuda))


def _frames_equal(got, want, F):
    """The last F frames of a tracker against columns of the offline call's EchoDelay."""
    for g, w in zip(got, (want.raw, want.locked, want.used, want.conf, want.ok)):
        assert g.shape == w[:, -F:].shape and torch.equal(g, w[:, -F:])


@pytest.mark.parametrize("first", [(1, 7, 479, 2400), ()], ids=["ragged-blocks", "480-hops"])
@pytest.mark.parametrize("kw", KW[:3], ids=KW_IDS[:3])
def test_streamed_equals_offline_bit_for_bit(cuda, streams, kw, first):
    from facodec_amd import ops
    from facodec_amd.streaming import EchoDelayTracker
    n, mic, far = streams["n"], streams["mic"], streams["far"]
    want = ops.echo_delay(mic, far, **kw)
    assert int(want.locked.max()) >= 320
    trk = EchoDelayTracker(3, ring=8 if first else 64, **kw)          # ring = 8: the push of 2400 completes nine frames and is run as two
    out, t = [], 0
    for k in _blocks(first, 480, n):
        y = trk.push(mic[:, None, t:t + k], far[:, None, t:t + k]) if t == 0 else trk.push(mic[:, t:t + k], far[:, t:t + k])
        out.append(y.reshape(3, -1))
        t += k
    assert trk.samples == n and trk.n_frames == n_frames(n) and trk.latency == 0.0
    assert np.array_equal(bits(torch.cat(out, dim=1)), bits(want.far))
    _frames_equal(trk.frames(trk.R if trk.R < n_frames(n) else n_frames(n)), want, min(trk.R, n_frames(n)))
    assert torch.equal(trk.delay(), want.locked[:, -1]) and torch.equal(trk.confidence(), want.conf[:, -1])


@pytest.mark.parametrize("at", [2400, 2560])
def test_reset_rows_is_the_offline_call_with_starts(cuda, streams, at):
    """Row 1 is reset after `at` samples (inside a block; on the grid): from there on it gives ops.echo_delay of the whole input
    with starts = at; rows 0 and 2 go on as if nothing had happened."""
    from facodec_amd import ops
    from facodec_amd.streaming import EchoDelayTracker
    n, mic, far = streams["n"], streams["mic"], streams["far"]
    starts = torch.tensor([0, at, 0], dtype=torch.int32, device=cuda)
    want = ops.echo_delay(mic, far, starts=starts, max_delay=512)
    plain = ops.echo_delay(mic, far, max_delay=512)
    assert torch.equal(want.far[0], plain.far[0]) and torch.equal(want.locked[2], plain.locked[2]) and torch.all(want.far[1, :at] == 0.0)
    trk = EchoDelayTracker(3, max_delay=512)
    out = [trk.push(mic[:, :at], far[:, :at])]
    trk.reset([1])
    assert trk.delay().tolist()[1] == -1 and trk.confidence().tolist()[1] == 0.0
    out += [trk.push(mic[:, t:t + 480], far[:, t:t + 480]) for t in range(at, n, 480)]
    got = torch.cat(out, dim=1)
    assert np.array_equal(bits(got[0]), bits(want.far[0])) and np.array_equal(bits(got[2]), bits(want.far[2]))
    assert np.array_equal(bits(got[1, at:]), bits(want.far[1, at:]))
    F = n_frames(n) - (at // H + 1) + 1                                          # row 1's frames of the new stream
    for g, w in zip(trk.frames(F), (want.raw, want.locked, want.used, want.conf, want.ok)):
        assert torch.equal(g, w[:, -F:])
    assert torch.equal(trk.delay(), want.locked[:, -1]) and int(want.locked[1, -1]) >= 320


# ---------------------------------------------------------------------------------------------- batching
def test_a_row_alone_equals_the_row_in_the_batch(cuda, on_device):
    from facodec_amd import ops
    whole = ops.echo_delay(on_device["mic"], on_device["far"], lens=on_device["lens"], max_delay=512)
    for b in (0, 1, 3):
        alone = ops.echo_delay(on_device["mic"][b:b + 1], on_device["far"][b:b + 1], lens=on_device["lens"][b:b + 1], max_delay=512)
        for a, w in zip(alone, whole):
            assert torch.equal(a[0], w[b])


def test_clips_do_not_depend_on_the_grouping(cuda):
    from facodec_amd import commons, ops
    lengths = [24000, 4800, 48000, 11111, 30001]
    pairs = [broadband_pair(n, 61 + i) for i, n in enumerate(lengths)]
    mics, fars = [torch.from_numpy(p[0]).to(cuda) for p in pairs], [torch.from_numpy(p[1]).to(cuda) for p in pairs]
    mics[2], fars[2] = mics[2][None], fars[2][None]
    assert len(commons.plan_groups(lengths, 60002)) == 3
    got, one = commons.echo_delay_clips(mics, fars, max_batch_samples=60002, max_delay=512), commons.echo_delay_clips(mics, fars, max_delay=512)
    c3 = commons.echo_cancel_clips(mics, fars, max_batch_samples=60002, P=4, delay="auto", max_delay=512)
    c1 = commons.echo_cancel_clips(mics, fars, P=4, delay="auto", max_delay=512)
    for m, f, n, a, b, u, v in zip(mics, fars, lengths, got, one, c3, c1):
        alone = ops.echo_delay(m.reshape(1, -1), f.reshape(1, -1), max_delay=512)
        last = (int(alone.locked[0, -1]), float(alone.conf[0, -1])) if n >= 512 else (-1, 0.0)
        assert a == b == last
        e = ops.echo_cancel(m.reshape(1, -1), f.reshape(1, -1), P=4, delay="auto", max_delay=512)
        same = ops.echo_cancel(m.reshape(1, -1), alone.far, P=4, delay=0)
        assert np.array_equal(bits(e.e), bits(same.e)) and torch.equal(e.W, same.W)
        for r in (u, v):
            assert r.e.shape == (n,) and np.array_equal(bits(r.e), bits(e.e[0])) and torch.equal(r.W, e.W[0]) and torch.equal(r.stats, e.stats[0])
    assert 320 <= got[0][0] < 470 and got[0][1] > 0.1 and got[1][0] == -1
    assert commons.echo_delay_clips([mics[0][:300]], [fars[0][:300]]) == [(-1, 0.0)]     # under 512 samples: no frame


# ---------------------------------------------------------------------------------------------- composites
def test_aligned_canceller_is_the_two_stages(cuda, streams):
    from facodec_amd.streaming import AlignedEchoCanceller, EchoCanceller, EchoDelayTracker
    n, mic, far = streams["n"], streams["mic"], streams["far"]
    both = AlignedEchoCanceller(3, P=2, max_delay=512)
    trk, aec = EchoDelayTracker(3, max_delay=512), EchoCanceller(3, P=2, delay=0)
    for t in range(0, n, 480):
        m, f = mic[:, t:t + 480], far[:, t:t + 480]
        assert torch.equal(both.push(m, f), aec.push(m, trk.push(m, f)))
        if t == 4800:
            both.reset([1]), trk.reset([1]), aec.reset([1])
    assert both.samples == n and torch.equal(both.tracker.delay(), trk.delay())
    assert int(trk.delay()[0]) >= 320 and int(trk.delay()[2]) >= 320           # row 1's new stream is too short to latch again
    assert torch.equal(both.finish(), aec.finish()) and torch.equal(both.weights(), aec.weights()) and float(aec.weights().abs().max()) > 0.0


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


@pytest.mark.parametrize("order", ["auto", "auto-denoise-level", "delay0"])
def test_echo_cancelled_session_with_a_tracked_delay(full_model, cuda, order):
    """A StreamingCodec behind EchoCancelledSession(delay="auto"), alone and around DenoisedSession(LevelledSession(..)): the
    dicts are those of the bare session fed the stages' outputs, tracker and canceller first.  With delay=0 the session is what
    it was: an EchoCanceller built directly."""
    from facodec_amd.streaming import (HOP, AutoGain, DenoisedSession, EchoCancelledSession, EchoCanceller, EchoDelayTracker, LevelledSession,
                                       NoiseSuppressor, StreamingCodec)
    m = full_model
    n_hops = 5
    n = 4800 + n_hops * HOP
    pairs = [broadband_pair(n, 71 + b) for b in range(2)]
    far = torch.from_numpy(np.stack([p[1] for p in pairs]))[:, None].to(cuda)
    wave = (0.02 * synth.synth_clips(2, n, seed=47)).to(cuda) + torch.from_numpy(np.stack([p[0] for p in pairs]))[:, None].to(cuda)
    cut = [(0, 4800)] + [(4800 + h * HOP, 4800 + (h + 1) * HOP) for h in range(n_hops)]
    ns_kw, agc_kw = dict(M=2, W=5), dict(window=5, lookahead=120)
    ed_kw = dict(max_delay=512, hold=4, thr=0.05)        # the restatement latches rows 0 and 1 at frames 18 and 15 of these 27
    with torch.no_grad():
        timbre = m.quantizer(m.encoder(wave), wave, n_c=2, return_codes=True)[4].clone()
        codec = StreamingCodec(m, timbre, n_c=2, use_graphs=False)
        trk, aec, ns, agc = EchoDelayTracker(2, **ed_kw), EchoCanceller(2, P=2, delay=0), NoiseSuppressor(2, **ns_kw), AutoGain(2, 24000, **agc_kw)
        if order == "auto":
            stages, sess = [], EchoCancelledSession(codec, delay="auto", P=2, **ed_kw)
        elif order == "delay0":
            trk, stages, sess = None, [], EchoCancelledSession(codec, delay=0, P=2)
            assert type(sess.aec) is EchoCanceller
        else:
            stages, sess = [ns, agc], EchoCancelledSession(DenoisedSession(LevelledSession(codec, **agc_kw), **ns_kw), delay="auto", P=2, **ed_kw)
        assert abs(sess.latency_in - (256 + (632 if stages else 0)) / 24000) < 1e-12 and sess.prime_samples == 4800
        fed = []
        for a, b in cut:
            w, f = wave[:, :, a:b], far[:, :, a:b]
            blk = aec.push(w, trk.push(w, f) if trk else f)
            for st in stages:
                blk = st.push(blk)
            fed.append(blk)
        bare = StreamingCodec(m, timbre, n_c=2, use_graphs=False)
        want = [_keep(bare.prime(fed[0]))] + [_keep(bare.push(f)) for f in fed[1:]] + [_keep(bare.finish())]
        got = [_keep(sess.prime(wave[:, :, :4800], far[:, :, :4800]))] + [_keep(sess.push(wave[:, :, a:b], far[:, :, a:b])) for a, b in cut[1:]]
        got.append(_keep(sess.finish()))
    _same_dicts(got, want)
    if trk:
        print(f"{order}: latched delays {trk.delay().tolist()}")
        assert torch.equal(sess.aec.tracker.delay(), trk.delay()) and trk.n_frames == n_frames(n) and int(trk.delay().min()) >= 320


# ---------------------------------------------------------------------------------------------- the synthetic call
def test_synthetic_call_on_the_device(cuda):
    """Seed 0, the microphone 3000 samples late, ops.echo_cancel(delay="auto"): the lock is the restatement's, and the ERLE over
    4.5 .. 5.5 s by plain sums is at least the CPU figure (test_echo_delay_cpu, (g)) less 3 dB."""
    from facodec_amd import ops
    mic, far, echo, near, ref = call_run(0, 3000)
    md, fd = torch.from_numpy(mic)[None].to(cuda), torch.from_numpy(far)[None].to(cuda)
    got = ops.echo_delay(md, fd)
    locks, want = locks_of(got.locked[0].tolist()), locks_of(ref.locked)
    margins = np.array(ref.margins)
    print(f"device locks {locks}, restatement {want}; undecidable frames {(~(margins > DECIDABLE).all(axis=1)).sum()} of {len(margins)}, "
          f"smallest margins {margins.min(axis=0)}")
    assert locks == want == [(29, 3031)]                                       # frame 30
    _check_row(got, 0, ref, far, len(far))
    e = ops.echo_cancel(md, fd, delay="auto").e
    assert np.array_equal(bits(e), bits(ops.echo_cancel(md, got.far, delay=0).e))
    ed = torch.from_numpy(echo)[None].to(cuda)
    a, b = int(4.5 * FS), int(5.5 * FS)
    late = 10.0 * float(torch.log10(ed[0, a:b].square().sum() / e[0, a:b].double().square().sum()))
    blind = ops.echo_cancel(md, fd).e
    late_blind = 10.0 * float(torch.log10(ed[0, a:b].square().sum() / blind[0, a:b].double().square().sum()))
    print(f"device, seed 0, 3000 samples late: ERLE over 4.5 .. 5.5 s {late:.2f} dB with the tracked delay (CPU {erle_late_auto():.2f} dB), "
          f"{late_blind:.2f} dB with delay = 0")
    assert late >= erle_late_auto() - 3.0
    assert late_blind < 3.0


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_before_any_launch(cuda):
    check_refusals()
    from facodec_amd import ops
    from facodec_amd.streaming import EchoDelayTracker
    trk = EchoDelayTracker(2)
    z = torch.zeros(2, 480, device=cuda)
    with pytest.raises(ValueError):
        trk.push(torch.zeros(2, 0, device=cuda), torch.zeros(2, 0, device=cuda))
    with pytest.raises(ValueError):
        trk.push(torch.zeros(3, 480, device=cuda), torch.zeros(3, 480, device=cuda))
    with pytest.raises(ValueError):
        trk.push(z, torch.zeros(2, 481, device=cuda))
    with pytest.raises(ValueError, match="differ"):
        ops.echo_delay(z, torch.zeros(2, 481, device=cuda))
    with pytest.raises(ValueError, match="starts"):
        ops.echo_delay(z, z, starts=torch.zeros(3, dtype=torch.int64, device=cuda))
    with pytest.raises(ValueError, match="starts must not be negative"):
        ops.echo_delay(z, z, starts=torch.tensor([0, -1]))
    with pytest.raises(_lib.FacodecHipError, match="lens"):
        ops.echo_delay(z, z, lens=torch.zeros(2, dtype=torch.int64, device=cuda))
    p = ops.echo_delay_params()
    st = ops.edelay_state(2, p, cuda)
    with pytest.raises(_lib.FacodecHipError, match="frm0 = 0 below"):      # through fac_last_error
        ops.edelay_run(z, z, p, st, frm0=0)
    with pytest.raises(_lib.FacodecHipError, match="ends behind the call's last sample"):
        ops.edelay_run(z, z, p, st, n_frm=1)
    with pytest.raises(ValueError, match="edelay_run: C"):
        ops.edelay_run(z, z, ops.echo_delay_params(max_delay=512), st)
    empty = ops.echo_delay(torch.zeros(2, 0, device=cuda), torch.zeros(2, 0, device=cuda))
    assert empty.far.shape == (2, 0) and empty.raw.shape == (2, 0) and empty.score.shape == (2, 0, 65)
    short = ops.echo_delay(z, z)
    assert short.raw.shape == (2, 0) and torch.all(short.far == 0.0)
    assert trk.push(z, z).shape == (2, 480) and trk.samples == 480
