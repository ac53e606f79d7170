"""Batches of clips with different lengths: commons.encode_clips / decode_clips / reconstruct_clips,
FAquantizer.forward_ragged and the kernels under them (fac_stft_frames_ragged, fac_mask_tail, fac_frame_mask).

Every clip of a zero-padded batch must come out as the single-clip calls give it.  The three clips have 7 200, 5 130 and 3 301
samples (24, 17 and 11 frames; two lengths that are no multiple of the 300-sample hop, each clip shorter than the one before):
the smallest batch in which the end reflection of the log-mel frames, the frame crop, the masking and the ordering can each go
wrong.  The clips come from synth.synth_clips(3, 7200, seed=SEED), cut to their lengths.
"""
import numpy as np
import pytest
import torch

from facodec_amd import commons, synth

gpu = pytest.mark.gpu

OP_TOL = 1e-5
E2E_TOL = 1e-4
LENGTHS = (7200, 5130, 3301)
ORDER = (1, 2, 0)              # the order the clip-list calls get the clips in: neither ascending nor descending
HOP = 300
SEED = 21
MAX_NEAR_TIE_FRAMES = 1        # of 52 frames x 6 arg-max decisions, per comparison


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def O():
    from oracle import facodec_oracle
    return facodec_oracle


@pytest.fixture(scope="module")
def ops(cuda):
    from facodec_amd import ops as _ops
    from facodec_amd import _lib
    _lib.load()  # fails loudly if the extension is missing
    return _ops


@pytest.fixture(scope="module")
def full_model(cuda):
    from facodec_amd.commons import build_model, default_model_params
    model = build_model(default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(cuda)
    return model


@pytest.fixture(scope="module")
def clips():
    """Three (1, T_i) host clips, longest first."""
    w = synth.synth_clips(3, LENGTHS[0], seed=SEED)
    return [w[i, :, :n].clone() for i, n in enumerate(LENGTHS)]


@pytest.fixture(scope="module")
def padded(clips, cuda):
    """(waves (3, 1, 7200) zero-padded, lens (3,) int32) on the device."""
    batch = torch.zeros(3, 1, LENGTHS[0])
    for i, c in enumerate(clips):
        batch[i, :, :c.shape[-1]] = c
    return batch.to(cuda), torch.tensor(LENGTHS, dtype=torch.int32).to(cuda)


@pytest.fixture(scope="module")
def oracle_ref(full_model, O, clips):
    """O.codec_forward of every clip alone, on the CPU."""
    sds = {k: {n: v.detach().cpu() for n, v in full_model[k].state_dict().items()} for k in ("encoder", "quantizer", "decoder")}
    with torch.no_grad():
        return [O.codec_forward(sds, c.unsqueeze(0), n_c=2) for c in clips]


@pytest.fixture(scope="module")
def ragged(full_model, clips, cuda):
    """encode_clips / reconstruct_clips on the clips in ORDER, results put back into the clips' own order; the projected latents
    of the one padded batch (rows in sorted order) for the code triage."""
    from facodec_amd.diagnostics import LatentCapture
    waves = [clips[i].to(cuda) for i in ORDER]
    with LatentCapture(full_model.quantizer) as cap:
        enc = commons.encode_clips(full_model, waves, n_c=2)
    rec = commons.reconstruct_clips(full_model, waves, n_c=2)
    torch.cuda.synchronize()
    back = {i: j for j, i in enumerate(ORDER)}
    rows = {i: r for r, i in enumerate(sorted(range(3), key=lambda i: LENGTHS[i]))}       # clip -> row of the padded batch
    return dict(enc=[enc[back[i]] for i in range(3)], rec=[rec[back[i]] for i in range(3)], cap=cap, rows=rows)


@pytest.fixture(scope="module")
def single(full_model, clips, cuda):
    """The existing product path on every clip alone (B = 1)."""
    out = []
    with torch.no_grad():
        for c in clips:
            w = c.unsqueeze(0).to(cuda)
            z = full_model.encoder(w)
            outs, _, _, _, timbre, codes = full_model.quantizer(z, w, n_c=2, return_codes=True)
            out.append(dict(codes=codes, timbre=timbre, wave=full_model.decoder(outs)))
    return out


def _triage(full_model, ragged, i, expected):
    """classify_code_mismatches of clip i's three code streams (diagnostics.classify_faquantizer_codes on the clip's row and
    frames of the padded batch's latents) -> (genuine, near-tie frames, report)."""
    from facodec_amd.diagnostics import classify_code_mismatches, flipped_frames
    cap, row, F = ragged["cap"], ragged["rows"][i], LENGTHS[i] // HOP
    report, upstream = {}, None
    for (name, mod), c, e in zip(cap.rvqs, ragged["enc"][i]["codes"], expected):
        c, e = c.unsqueeze(0), torch.as_tensor(e).reshape(1, -1, F)
        lat = cap.latents[name][row:row + 1, :, :F]
        report[name] = classify_code_mismatches(mod, lat, c, e, upstream_flips=upstream if name.startswith("residual") else None)
        f = flipped_frames(c, e)
        upstream = f if upstream is None else (upstream | f)
    return sum(r["genuine"] for r in report.values()), sum(r["near_tie"] for r in report.values()), report


# ------------------------------------------------------------------------------------------------ 1. framing kernel
@gpu
@pytest.mark.parametrize("n_win,hop,pad,n_off", [(1200, 300, 1024, None), (512, 128, 256, 0)])
def test_stft_frames_ragged_is_the_per_clip_gather(full_model, ops, padded, cuda, n_win, hop, pad, n_off):
    """Row b == ops.stft_frames of wave[b, :lens[b]] bit for bit (own end reflection, lens[b] // hop frames), zeros behind; the
    padding holds non-zero values here, which the kernel must not read."""
    if n_off is None:
        n_off = full_model.quantizer.to_mel._consts(cuda)[2]
    waves, lens = padded
    w = waves[:, 0].clone()
    for b, n in enumerate(LENGTHS):
        w[b, n:] = 7.0
    n_frames = w.shape[1] // hop
    fr = ops.stft_frames_ragged(w, lens, n_win, n_frames, hop, pad, n_off)
    assert fr.shape == (3, n_win, n_frames)
    for b, n in enumerate(LENGTHS):
        own = ops.stft_frames(w[b:b + 1, :n].contiguous(), n_win, n // hop, hop, pad, n_off)
        assert torch.equal(fr[b:b + 1, :, :n // hop], own), b
        assert float(fr[b, :, n // hop:].abs().sum()) == 0.0, b
        if n < LENGTHS[0]:           # the end reflection is the clip's: framing the padded row as a whole gives other last frames
            whole = ops.stft_frames(w[b:b + 1].contiguous(), n_win, n_frames, hop, pad, n_off)
            assert not torch.equal(whole[:, :, :n // hop], own)


# ------------------------------------------------------------------------------------------------ 2. mask_tail, frame mask
@gpu
@pytest.mark.parametrize("unit,C,T,dtype", [
    (1, 3, 7201, torch.float32),       # sample rate: two column blocks per row, odd row length, row 0 ends one sample early
    (1, 1, 7200, torch.float32),       # the decoder's output shape; row 0 is full: nothing is zeroed
    (300, 7, 24, torch.float32),       # frame rate, several rows per workgroup; row 0 is full
    (300, 5, 25, torch.float32),       # C * T = 125: no multiple of the vector width, unaligned row starts
    (300, 3, 24, torch.int64),         # code tensors
])
def test_mask_tail_matches_torch(ops, cuda, unit, C, T, dtype):
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(3, C, T, generator=g) if dtype == torch.float32 else torch.randint(1, 1024, (3, C, T), generator=g)).to(cuda)
    lens = torch.tensor(LENGTHS, dtype=torch.int32).to(cuda)
    want = x.clone()
    for b, n in enumerate(LENGTHS):
        want[b, :, n // unit:] = 0
    got = ops.mask_tail_(x.clone(), lens, unit)
    assert torch.equal(got, want)
    if LENGTHS[0] // unit >= T:
        assert torch.equal(got[0], x[0])


@gpu
def test_frame_mask_matches_torch(ops, cuda):
    lens = torch.tensor(LENGTHS, dtype=torch.int32).to(cuda)
    for F in (24, 20, 300):
        mask, frame_lens = ops.frame_mask(lens, F, HOP)
        want = (torch.arange(F, device=cuda)[None] < (lens // HOP)[:, None]).to(torch.float32)
        assert mask.dtype == torch.float32 and torch.equal(mask, want)
        assert frame_lens.dtype == torch.int32 and torch.equal(frame_lens, (lens // HOP).clamp(max=F).to(torch.int32))


# ------------------------------------------------------------------------------------------------ 3. timbre encoder
@gpu
def test_timbre_encoder_ragged_mode_is_per_clip_exact(full_model, ops, padded, cuda):
    """StyleEncoder.forward_ragged on the padded batch against the unmasked forward on every clip alone, at the per-op bar; the
    existing `mask=` path (the reference's: the second GLU conv reads what the first wrote past the clip's end) is not."""
    q = full_model.quantizer
    waves, lens = padded
    with torch.no_grad():
        mel = q.to_mel.forward_ragged(waves, lens)
        mask, _ = ops.frame_mask(lens, mel.shape[-1], HOP)
        got = q.timbre_encoder.forward_ragged(mel, lens, mask, HOP)
        old = q.timbre_encoder(mel, mask)
        errs, errs_old = [], []
        for b, n in enumerate(LENGTHS):
            own_mel = q.to_mel(waves[b:b + 1, :, :n].contiguous())
            assert torch.equal(mel[b:b + 1, :, :n // HOP], own_mel) or rel(mel[b:b + 1, :, :n // HOP], own_mel) < OP_TOL
            own = q.timbre_encoder(own_mel, None)
            errs.append(rel(got[b:b + 1], own))
            errs_old.append(rel(old[b:b + 1], own))
    print("timbre encoder, ragged mode vs per clip:", errs, " existing mask= path:", errs_old)
    assert got.shape == (3, 1024)
    assert max(errs) < OP_TOL, errs
    assert errs_old[2] > OP_TOL, errs_old


# ------------------------------------------------------------------------------------------------ 4. against the oracle
@gpu
def test_encode_and_reconstruct_clips_vs_oracle(full_model, ragged, oracle_ref):
    """Clips handed over in ORDER; every clip against O.codec_forward of that clip alone: shapes per clip, timbre and wave at
    the end-to-end bar, no genuine code mismatch and at most one near-tie frame in the whole test (a condition on the seed,
    SEED above: should it ever be exceeded, the single-clip path is checked against the oracle on the same clips first)."""
    near_total = 0
    for i, n in enumerate(LENGTHS):
        F, ref, enc, rec = n // HOP, oracle_ref[i], ragged["enc"][i], ragged["rec"][i]
        assert [tuple(c.shape) for c in enc["codes"]] == [(1, F), (2, F), (3, F)] and all(c.dtype == torch.int64 for c in enc["codes"])
        assert enc["timbre"].shape == (1024,) and rec.shape == (1, HOP * F)
        genuine, near, report = _triage(full_model, ragged, i, [c[0] for c in ref["codes"]])
        print(f"clip {i} vs oracle: timbre {rel(enc['timbre'], ref['timbre'][0]):.2e} wave {rel(rec, ref['wave'][0]):.2e} codes {report}")
        assert genuine == 0, report
        near_total += near
        assert rel(enc["timbre"], ref["timbre"][0]) < E2E_TOL
        assert rel(rec, ref["wave"][0]) < E2E_TOL
    assert near_total <= MAX_NEAR_TIE_FRAMES, near_total


# ------------------------------------------------------------------------------------------------ 5. against the single-clip path
@gpu
def test_clips_match_the_single_clip_product_path(full_model, ragged, single, padded):
    near_total = 0
    for i, n in enumerate(LENGTHS):
        F, one, enc, rec = n // HOP, single[i], ragged["enc"][i], ragged["rec"][i]
        genuine, near, report = _triage(full_model, ragged, i, [c[0].cpu() for c in one["codes"]])
        print(f"clip {i} vs B = 1: timbre {rel(enc['timbre'], one['timbre'][0]):.2e} wave {rel(rec, one['wave'][0]):.2e} codes {report}")
        assert genuine == 0, report              # every differing frame is a near-tie flip (and its cascade)
        near_total += near
        assert rel(enc["timbre"], one["timbre"][0]) < E2E_TOL
        assert one["wave"].shape == (1, 1, HOP * F) and rel(rec, one["wave"][0]) < E2E_TOL
        # the prosody codes of the last frames hang on the log-mel frames that reflect at the clip's end
        assert torch.equal(enc["codes"][0][:, F - 4:], one["codes"][0][0, :, F - 4:]), i
    assert near_total <= MAX_NEAR_TIE_FRAMES, near_total

    # negative control: the existing forward on the zero-padded batch does NOT give the shortest clip its own result
    waves, _ = padded
    with torch.no_grad():
        z = full_model.encoder(waves)
        _, _, _, _, timbre, codes = full_model.quantizer(z, waves, n_c=2, return_codes=True)
    F = LENGTHS[2] // HOP
    timbre_err = rel(timbre[2], single[2]["timbre"][0])
    tail_differs = not torch.equal(codes[0][2, :, F - 4:F], single[2]["codes"][0][0, :, F - 4:])
    print(f"zero-padded existing forward, shortest clip: timbre {timbre_err:.2e}, last prosody codes differ: {tail_differs}")
    assert timbre_err > E2E_TOL or tail_differs


# ------------------------------------------------------------------------------------------------ 6. decode_clips
@gpu
def test_decode_clips_with_a_swapped_timbre(full_model, ragged):
    codes = [e["codes"] for e in ragged["enc"]]
    timbres = [ragged["enc"][j]["timbre"] for j in (1, 0, 2)]          # clips 0 and 1 speak with each other's timbre
    waves = commons.decode_clips(full_model, [codes[i] for i in ORDER], [timbres[i] for i in ORDER])
    for j, i in enumerate(ORDER):
        F = LENGTHS[i] // HOP
        want = commons.decode_codes(full_model, [c.unsqueeze(0) for c in codes[i]], timbres[i].unsqueeze(0))
        assert waves[j].shape == (1, HOP * F) and want.shape == (1, 1, HOP * F)
        assert rel(waves[j], want[0]) < E2E_TOL, i
    assert rel(waves[ORDER.index(0)], ragged["rec"][0]) > E2E_TOL       # the swap is audible in the wave


# ------------------------------------------------------------------------------------------------ 7. errors
@gpu
def test_errors(full_model, clips, padded, cuda):
    from facodec_amd._lib import FacodecHipError
    need = commons.min_clip_samples(full_model)
    assert commons.encode_clips(full_model, []) == [] and commons.decode_clips(full_model, [], []) == []
    assert commons.reconstruct_clips(full_model, []) == []
    with pytest.raises(ValueError, match=str(need)):
        commons.encode_clips(full_model, [clips[0].to(cuda), clips[1][:, :need - 1].to(cuda)])
    short = [torch.zeros(n, need // HOP - 1, dtype=torch.int64, device=cuda) for n in (1, 2, 3)]
    with pytest.raises(ValueError, match=str(need)):
        commons.decode_clips(full_model, [short], [torch.zeros(1024, device=cuda)])
    with pytest.raises(FacodecHipError):
        commons.encode_clips(full_model, [clips[0].to(cuda), clips[1]])
    waves, lens = padded
    q = full_model.quantizer
    with torch.no_grad():
        z = full_model.encoder(waves)
        q.train()
        try:
            with pytest.raises(RuntimeError, match="eval"):
                q.forward_ragged(z, waves, lens, n_c=2)
        finally:
            q.eval()
        with pytest.raises(FacodecHipError):
            q.forward_ragged(z, waves, lens.cpu(), n_c=2)


# ------------------------------------------------------------------------------------------------ 8. host side (no GPU)
def test_plan_groups():
    rng = np.random.default_rng(0)
    cases = [([7200, 5130, 3301], 10 ** 9), ([7200, 5130, 3301], 7200), ([5, 5, 5, 5], 10), ([720000] + [24000] * 31, 32 * 48000),
             (list(rng.integers(24000, 72001, 32)), 32 * 48000), (list(rng.integers(3000, 10 ** 6, 200)), 500000), ([], 100)]
    for lengths, budget in cases:
        lengths = [int(n) for n in lengths]
        groups = commons.plan_groups(lengths, budget)
        assert sorted(i for g in groups for i in g) == list(range(len(lengths)))          # every clip exactly once
        order = sorted(range(len(lengths)), key=lambda i: (lengths[i], i))
        assert [i for g in groups for i in g] == order                                     # groups are runs of the sorted order
        for g in groups:
            assert g and (len(g) == 1 or len(g) * max(lengths[i] for i in g) <= budget)
        assert 0.0 <= commons.padding_share(lengths, groups) < 1.0
    long_one = commons.plan_groups([720000] + [24000] * 31, 32 * 48000)
    assert long_one[-1] == [0] and len(long_one) == 2           # the 30 s clip does not pad the 31 short ones up to itself
    assert commons.plan_groups([7200, 5130, 3301], 10 ** 9) == [[2, 1, 0]]


def test_min_clip_samples_and_causality_requirement():
    """The minimum comes from the modules' reflect paddings (shipped configuration: the decoder's k = 7, dilation 9 convs at 6
    columns per frame need 10 frames); a non-causal configuration is refused."""
    params = commons.default_model_params()
    params.DAC.encoder_dim, params.DAC.decoder_dim = 8, 64              # the paddings do not depend on the widths
    model = commons.build_model(params)
    assert commons.min_clip_samples(model) == 3000
    params.causal = False
    with pytest.raises(NotImplementedError, match="causal"):
        commons.min_clip_samples(commons.build_model(params))
