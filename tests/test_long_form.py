"""Recordings of any length in bounded memory: FAquantizer.timbre_long, streaming.ChunkedCodec and
commons.encode_long / decode_long / reconstruct_long.

The timbre of a 2305-frame clip -- one frame past what the attention's LDS route takes -- against the oracle's float64 style
encoder; the chunked session against the offline product on signals whose chunking has a short last chunk (7 frames), a
one-frame last chunk and no push at all; the public calls against the single-clip calls.  Signals: synth.synth_clips(2, T,
seed=11), the signal family on which the 480-sample-hop session holds strict code equality (test_streaming_matches_offline)."""
import pytest
import torch

from facodec_amd import commons, synth

gpu = pytest.mark.gpu

E2E_TOL = 1e-4
HOP = 300
SEED = 11
MAX_NEAR_TIE_FRAMES = 1        # per comparison (one signal of <= 56 frames x 2 streams x 6 arg-max decisions)
# (chunk_samples, T): a 7-frame last chunk; a one-frame last chunk; prime then finish only
SESSION_CASES = {"a_last_chunk_7_frames": (4800, 3 * 4800 + 2100), "b_last_chunk_1_frame": (7200, 2 * 7200 + 300),
                 "c_prime_then_finish": (4800, 4800)}


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def O():
    from oracle import facodec_oracle
    return facodec_oracle


@pytest.fixture(scope="module")
def full_model(cuda):
    from facodec_amd.commons import build_model, default_model_params
    model = build_model(default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(cuda)
    return model


@pytest.fixture(scope="module")
def offline(full_model, cuda):
    """The offline product on every signal of SESSION_CASES, computed once: wave, codes, timbre, decoder output and the projected
    latents of the three RVQs (for the code triage)."""
    from facodec_amd.diagnostics import LatentCapture
    m, out = full_model, {}
    for name, (chunk, T) in SESSION_CASES.items():
        wave = synth.synth_clips(2, T, seed=SEED).to(cuda)
        with torch.no_grad(), LatentCapture(m.quantizer) as cap:
            outs, _, _, _, timbre, codes = m.quantizer(m.encoder(wave), wave, n_c=2, return_codes=True)
            y = m.decoder(outs)
        out[name] = dict(wave=wave, codes=codes, timbre=timbre, y=y, cap=cap)
    return out


def _triage(cap, offline_codes, other_codes):
    """diagnostics.classify_code_mismatches of the three code streams, as test_ragged_batch._triage: the offline run is the one whose
    latents were captured, so it is the `got` side and the chunked codes the `expected` side (a near tie is one either way: the
    two candidates' distances differ by <= tie_tol) -> (genuine, near-tie frames, report)."""
    from facodec_amd.diagnostics import classify_code_mismatches, flipped_frames
    report, upstream = {}, None
    for (name, mod), c, e in zip(cap.rvqs, offline_codes, other_codes):
        report[name] = classify_code_mismatches(mod, cap.latents[name], c, e.cpu(), upstream_flips=upstream if name.startswith("residual") else None)
        f = flipped_frames(c, e.cpu())
        upstream = f if upstream is None else (upstream | f)
    return sum(r["genuine"] for r in report.values()), sum(r["near_tie"] for r in report.values()), report


def _assert_codes(cap, offline_codes, other_codes, what):
    genuine, near, report = _triage(cap, offline_codes, other_codes)
    print(f"[codes] {what}: {report}")
    assert genuine == 0, (what, report)
    assert near <= MAX_NEAR_TIE_FRAMES, (what, report)


# ------------------------------------------------------------------------------------------------ 1. timbre
@gpu
def test_timbre_of_2305_frames_against_the_fp64_oracle(full_model, O, cuda):
    """One clip of 691 500 samples = 2305 frames, one past the attention's LDS route: `model.quantizer(z, wave)[4]` (it used to
    raise "too long for the LDS score tile") and timbre_long(wave, chunk_frames=512) both within E2E_TOL of the oracle's
    style_encoder_forward in float64 on the product's log-mel."""
    m = full_model
    q = m.quantizer
    T = 2305 * HOP
    wave = synth.synth_clips(1, T, seed=SEED).to(cuda)
    with torch.no_grad():
        mel = q.to_mel(wave)
        assert mel.shape[-1] == 2305
        sd = {n: v.detach().cpu().double() for n, v in q.state_dict().items() if n.startswith("timbre_encoder.")}
        ref = O.style_encoder_forward(mel.cpu().double(), sd, "timbre_encoder.")
        z = torch.zeros(1, q.in_dim, 2305, device=cuda)           # the timbre does not depend on the latent
        got = q(z, wave, n_c=2)[4]
        long = q.timbre_long(wave, chunk_frames=512)
    assert got.shape == long.shape == (1, 1024)
    e1, e2 = rel(got, ref), rel(long, ref)
    print(f"[tol] timbre 2305 frames: quantizer {e1:.3e} timbre_long {e2:.3e}")
    assert e1 < E2E_TOL and e2 < E2E_TOL, (e1, e2)


@gpu
def test_timbre_long_in_small_chunks_is_the_single_clip_timbre(full_model, cuda):
    """7200 samples = 24 frames in chunks of 8 frames: a chunk that reflects at the start, an interior one, one that reflects at
    the end -- the existing single-clip timbre within E2E_TOL, the chunked log-mel within E2E_TOL of to_mel; lens runs every row
    on its own samples."""
    q = full_model.quantizer
    wave = synth.synth_clips(2, 7200, seed=SEED).to(cuda)
    with torch.no_grad():
        ref = q(torch.zeros(2, q.in_dim, 24, device=cuda), wave, n_c=2)[4]
        assert rel(q.log_mel_chunked(wave, 8), q.to_mel(wave)) < E2E_TOL
        assert rel(q.log_mel_chunked(wave, 5), q.to_mel(wave)) < E2E_TOL        # a last chunk of 4 frames
        assert rel(q.timbre_long(wave, chunk_frames=8), ref) < E2E_TOL
        short = q(torch.zeros(1, q.in_dim, 17, device=cuda), wave[1:, :, :5130].contiguous(), n_c=2)[4]
        both = q.timbre_long(wave, lens=[7200, 5130], chunk_frames=8)
    assert rel(both[:1], ref[:1]) < E2E_TOL and rel(both[1:], short) < E2E_TOL


def test_mel_chunk_plan_covers_every_frame_and_reflects_at_the_ends_only():
    from facodec_amd.quantize import mel_chunk_plan
    for T, cf in ((7200, 8), (7200, 5), (691500, 512), (4801, 4096), (2400, 1)):
        plan = mel_chunk_plan(T, cf)
        assert [p[0] for p in plan] == list(range(0, T // HOP, cf)) and plan[-1][1] == T // HOP
        for f0, f1, s_lo, s_hi, pad in plan:
            assert 0 < f1 - f0 <= cf and 0 <= s_lo < s_hi <= T
            assert s_lo - pad == HOP * f0 - 1024 and (pad == 0 or s_lo == 0)                  # left reflection only at sample 0
            assert s_hi == min(T, HOP * (f1 - 1) + 1024)                                       # right reflection only at sample T


# ------------------------------------------------------------------------------------------------ 2. chunked session
@gpu
@pytest.mark.parametrize("case", list(SESSION_CASES))
def test_chunked_session_matches_offline(full_model, offline, cuda, case):
    """ChunkedCodec == the offline model on the whole signal: contiguous frame0, T // 300 frames in all, codes equal up to at most
    one near-tie frame and no genuine mismatch, waveform within E2E_TOL of model.decoder(outs).
    Measured on MI355X: see DESIGN.md 19."""
    from facodec_amd.streaming import ChunkedCodec
    chunk, T = SESSION_CASES[case]
    ref = offline[case]
    wave = ref["wave"]
    sess = ChunkedCodec(full_model, ref["timbre"], n_c=2, chunk_samples=chunk)
    pieces = [sess.prime(wave[:, :, :chunk])]
    pieces += [sess.push(wave[:, :, s:min(s + chunk, T)]) for s in range(chunk, T, chunk)]
    pieces.append(sess.finish())
    frame, codes, waves = 0, [[], [], []], []
    for o in pieces:
        if o["codes"] is None:
            continue
        assert o["frame0"] == frame
        frame += o["codes"][0].shape[-1]
        for i in range(3):
            codes[i].append(o["codes"][i])
        assert o["wave"].shape == (2, 1, HOP * o["codes"][0].shape[-1])
        waves.append(o["wave"])
    assert frame == T // HOP
    _assert_codes(ref["cap"], ref["codes"], [torch.cat(c, -1) for c in codes], case)
    err = rel(torch.cat(waves, -1), ref["y"])
    print(f"[tol] chunked session {case}: wave {err:.3e}")
    assert err < E2E_TOL
    with pytest.raises(RuntimeError):
        sess.push(wave[:, :, :HOP])                                # closed


@gpu
def test_chunked_session_encode_only(full_model, offline, cuda):
    from facodec_amd.streaming import ChunkedCodec
    chunk, T = SESSION_CASES["a_last_chunk_7_frames"]
    ref = offline["a_last_chunk_7_frames"]
    wave = ref["wave"]
    sess = ChunkedCodec(full_model, ref["timbre"], n_c=2, chunk_samples=chunk, encode_only=True)
    assert sess.dec is None
    pieces = [sess.prime(wave[:, :, :chunk])] + [sess.push(wave[:, :, s:min(s + chunk, T)]) for s in range(chunk, T, chunk)] + [sess.finish()]
    assert all(o["wave"] is None for o in pieces)
    _assert_codes(ref["cap"], ref["codes"], [torch.cat([o["codes"][i] for o in pieces], -1) for i in range(3)], "encode_only")


# ------------------------------------------------------------------------------------------------ 3. public calls
@gpu
def test_long_calls_match_the_single_clip_calls(full_model, offline, cuda):
    """Case (a) through encode_long / decode_long / reconstruct_long at a chunk of 4800 samples = 16 frames (0.2 s): codes and timbre
    against the single-clip calls, decode_long against decode_codes, reconstruct_long == encode_long then decode_long."""
    from facodec_amd.streaming import StreamingDecoder
    m, ref = full_model, offline["a_last_chunk_7_frames"]
    wave = ref["wave"]
    enc = commons.encode_long(m, wave, n_c=2, chunk_seconds=0.2)
    assert [tuple(c.shape) for c in enc["codes"]] == [(2, 1, 55), (2, 2, 55), (2, 3, 55)] and all(c.dtype == torch.int64 for c in enc["codes"])
    _assert_codes(ref["cap"], ref["codes"], enc["codes"], "encode_long")
    assert enc["timbre"].shape == (2, 1024) and rel(enc["timbre"], ref["timbre"]) < E2E_TOL
    # the codes do not depend on the timbre; a given timbre is handed through, timbre_seconds enrols on the head of the signal
    other = commons.encode_long(m, wave, n_c=2, chunk_seconds=0.2, timbre=ref["timbre"][[1, 0]].contiguous())
    assert all(torch.equal(a, b) for a, b in zip(other["codes"], enc["codes"])) and torch.equal(other["timbre"], ref["timbre"][[1, 0]])
    head = commons.encode_long(m, wave, n_c=2, chunk_seconds=0.2, timbre_seconds=0.3)
    with torch.no_grad():
        want = m.quantizer(torch.zeros(2, 1024, 24, device=cuda), wave[:, :, :7200].contiguous(), n_c=2)[4]
    assert rel(head["timbre"], want) < E2E_TOL
    # decode: chunks of 16 frames (>= the decoder's first chunk, min_prime)
    assert 16 >= StreamingDecoder(m, ref["timbre"], use_graphs=False, max_frames=16).min_prime
    y_ref = commons.decode_codes(m, ref["codes"], ref["timbre"])
    y = commons.decode_long(m, ref["codes"], ref["timbre"], chunk_seconds=0.2)
    assert y.shape == (2, 1, HOP * 55) and rel(y, y_ref) < E2E_TOL
    rec = commons.reconstruct_long(m, wave, n_c=2, chunk_seconds=0.2)
    assert torch.equal(rec, commons.decode_long(m, enc["codes"], enc["timbre"], chunk_seconds=0.2))
    assert rel(rec, ref["y"]) < E2E_TOL


@gpu
def test_long_calls_on_short_and_cropped_signals(full_model, cuda):
    """At most one chunk: the whole-clip calls, bit for bit (it is the same call).  T = 16 650 is cropped to 16 500 = 55 frames."""
    m = full_model
    wave = synth.synth_clips(2, 16650, seed=SEED).to(cuda)
    short = wave[:, :, :7200].contiguous()
    with torch.no_grad():
        outs, _, _, _, timbre, codes = m.quantizer(m.encoder(short), short, n_c=2, return_codes=True)
        y = m.decoder(outs)
    enc = commons.encode_long(m, short, n_c=2, chunk_seconds=0.3)                 # 7200 samples: one chunk
    assert all(torch.equal(a, b) for a, b in zip(enc["codes"], codes)) and torch.equal(enc["timbre"], timbre)
    assert torch.equal(commons.decode_long(m, codes, timbre, chunk_seconds=0.3), commons.decode_codes(m, codes, timbre))
    assert rel(commons.reconstruct_long(m, short, chunk_seconds=0.3), y) < E2E_TOL
    enc = commons.encode_long(m, wave, n_c=2, chunk_seconds=0.2)
    assert all(c.shape[-1] == 55 for c in enc["codes"])
    cropped = commons.encode_long(m, wave[:, :, :16500].contiguous(), n_c=2, chunk_seconds=0.2)
    assert all(torch.equal(a, b) for a, b in zip(enc["codes"], cropped["codes"])) and torch.equal(enc["timbre"], cropped["timbre"])
    assert commons.reconstruct_long(m, wave, chunk_seconds=0.2).shape == (2, 1, 16500)


@gpu
def test_long_calls_refuse_what_they_cannot_take(full_model, cuda):
    from facodec_amd._lib import FacodecHipError
    from facodec_amd.commons import build_model, default_model_params
    from facodec_amd.streaming import ChunkedCodec
    m = full_model
    wave = synth.synth_clips(1, 9600, seed=SEED)
    with pytest.raises(FacodecHipError):
        commons.encode_long(m, wave)                                             # a CPU tensor
    with pytest.raises(ValueError):
        commons.encode_long(m, wave.to(cuda), chunk_seconds=0.25)                # 6000 samples: no multiple of 2400
    with pytest.raises(ValueError):
        commons.encode_long(m, wave.to(cuda)[:, 0])                              # not (B, 1, T)
    timbre = torch.zeros(1, 1024, device=cuda)
    with pytest.raises(ValueError):
        ChunkedCodec(m, timbre, chunk_samples=6000)
    sess = ChunkedCodec(m, timbre, chunk_samples=4800, encode_only=True)
    with pytest.raises(RuntimeError):
        sess.push(wave.to(cuda)[:, :, :300])                                     # prime() first
    with pytest.raises(ValueError):
        sess.prime(wave.to(cuda)[:, :, :2400])
    sess.prime(wave.to(cuda)[:, :, :4800])
    for n in (299, 450, 5100):
        with pytest.raises(ValueError):
            sess.push(wave.to(cuda)[:, :, :n])
    params = default_model_params()
    params.causal = False
    nc = build_model(params)                      # refused on the host, before anything of it is needed on the device
    with pytest.raises(NotImplementedError):
        commons.encode_long(nc, wave.to(cuda), chunk_seconds=0.2)
    with pytest.raises(NotImplementedError):
        ChunkedCodec(nc, timbre, chunk_samples=4800)


# ------------------------------------------------------------------------------------------------ 4. no GPU
def test_plan_long_lists_the_chunks_and_the_fallback():
    assert commons.plan_long(16500, 4800) == (16500, [(0, 4800), (4800, 9600), (9600, 14400), (14400, 16500)])
    assert commons.plan_long(16650, 4800)[0] == 16500 and commons.plan_long(16650, 4800)[1][-1] == (14400, 16500)
    assert commons.plan_long(14700, 7200) == (14700, [(0, 7200), (7200, 14400), (14400, 14700)])
    assert commons.plan_long(4800, 4800) == (4800, None) and commons.plan_long(5099, 4800) == (4800, None)       # fallback: one chunk
    assert commons.plan_long(5100, 4800) == (5100, [(0, 4800), (4800, 5100)])
    assert commons.plan_long(299, 4800) == (0, None)
    Tc, plan = commons.plan_long(14_400_000 + 17, 240000)
    assert Tc == 14_400_000 and len(plan) == 60 and plan[0] == (0, 240000) and all(e - s == 240000 for s, e in plan)
    for T in (9600, 9900, 16650, 100_000):
        Tc, plan = commons.plan_long(T, 4800)
        assert plan[0] == (0, 4800) and plan[-1][1] == Tc and all(a[1] == b[0] for a, b in zip(plan, plan[1:]))
        assert all(0 < e - s <= 4800 and (e - s) % HOP == 0 for s, e in plan)
    for bad in (0, 2400, 6000, 4801):
        with pytest.raises(ValueError):
            commons.plan_long(16500, bad)


def test_long_calls_check_their_arguments_without_a_gpu():
    from facodec_amd._lib import FacodecHipError
    wave = torch.zeros(1, 1, 9600)
    with pytest.raises(FacodecHipError):
        commons.encode_long(None, wave)
    with pytest.raises(FacodecHipError):
        commons.reconstruct_long(None, wave)
    with pytest.raises(TypeError):
        commons.encode_long(None, [0.0] * 9600)
    assert commons._chunk_samples(0.2) == 4800 and commons._chunk_samples(10) == 240000 and commons._chunk_samples(0.1) == 2400
    with pytest.raises(ValueError):
        commons._chunk_samples(1 / 7)
