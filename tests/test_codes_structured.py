"""Code indices against the REFERENCE on structured signals and odd lengths (DESIGN.md "Structured signals and odd lengths").

Every other reference-made code fixture is synth.synth_clips: N(0, 1) noise at T = 48 000.  Here the real reference ran, in fp32 on
all threads, fp32 on one thread and fp64 (tests/golden/make_golden_bench.py structured / lengths), on

  * tests/structured_clips.structured_clips(48000): 32 clips on the 16-bit PCM grid in eight families -- silence and dither, clipped
    sines, chirps, amplitude-modulated noise, voiced with pauses, impulse trains, DC and steps, mixtures
    (tests/golden/codec_structured_decidable.npz, with the fp64 run's probes of one clip per family);
  * six lengths from the shortest the reference takes to its 30 s cut plus one sample, T in LENGTHS, a Gaussian and a voiced clip
    each (tests/golden/codec_lengths_decidable.npz); 691 500 samples are 2305 frames, the first on the stream attention route.

The rule is facodec_amd.diagnostics.check_codes_decidable_noise, unchanged: a position is decidable where the reference's three runs
agree and its fp64 top-2 gap is at least its own fp32-vs-fp64 margin noise; a decidable position must equal the reference's code,
no allowance.  The length cases are too short to measure that noise by themselves, so all of them use the largest noise the
reference showed anywhere (every length case, the structured batch, the four Gaussian batches).  The offline model, the clip-list
call commons.encode_clips and the streaming session are all judged by this rule; what goes uncompared (a noise flip and the stages
of its frame that follow it) is bounded by the fixture: at most six positions per frame that holds an undecidable position.

Measured on MI355X (one run; profiles/codes_structured_mi355x.md holds the table, from the report the GPU tests write):
  structured batch, offline: 0 mismatches of 30 720 positions (30 716 decidable), equal to all three reference runs; per probed
    clip and its own absmax the product is at 2.3e-07 .. 6.7e-06 (latent <= 4.8e-06, quantizer output <= 4.2e-06, waveform
    <= 6.7e-06, timbre <= 6.4e-06), the reference's own fp32 run at 3.1e-07 .. 7.3e-06; the bar is 1e-4
  lengths, offline and through encode_clips: 0 mismatches at every length; shapes and output lengths the reference's; at
    T = 691 500 the reference's two fp32 runs differ at two positions and the product equals the one-thread run
  streaming, graphs off and on: 0 mismatches of 3 840, equal to all three runs
  uncompared positions (noise flips + cascades): 0 everywhere, against bounds of 24 (structured), 18 / 12 / 96 / 60 (T = 47 999 /
    48 001 / 691 500 / 720 001) and 0 (the two short lengths, the streaming rows)
  prosody codes in use: 285 on the structured batch, 11 on the Gaussian batch; the 10 GPU tests take 7.5 s together
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from facodec_amd import commons, synth
from facodec_amd.diagnostics import REFERENCE_RUNS, check_codes_decidable_noise

import structured_clips as S

gpu = pytest.mark.gpu

E2E_TOL = 1e-4
HOP = 300
LENGTHS = (1025, 2101, 47999, 48001, 691500, 720001)
LONG = (691500, 720001)
MIN_DECIDABLE = 0.98                 # of every structured clip's positions
MAX_UNDECIDED_FRAMES = 0.02          # of every structured clip's frames may hold an undecidable position
KEYS = ("codes_f32_mt", "codes_f32_1t", "codes_f64", "second_f64", "gap_f64", "agree", "decidable")
# where the GPU tests leave their verdicts: codes_structured_report.json under FAC_TEST_REPORT_DIR (default: test_reports/)
REPORT = os.path.join(os.environ.get("FAC_TEST_REPORT_DIR", "test_reports"), "codes_structured_report.json")
REPORT_FIELDS = ("ok", "positions", "decidable", "noise", "mismatches", "noise_flips", "cascade_positions", "differs_from_fp32",
                 "differs_from_fp64", "equals_run")


# ------------------------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def fxs(golden_dir):
    return np.load(os.path.join(golden_dir, "codec_structured_decidable.npz"))


@pytest.fixture(scope="module")
def probes(fxs):
    """The fp64 run's probes of one clip per family live in the same file."""
    return fxs


@pytest.fixture(scope="module")
def fxl(golden_dir):
    return np.load(os.path.join(golden_dir, "codec_lengths_decidable.npz"))


@pytest.fixture(scope="module")
def structured(fxs):
    """(names, wave (32, 1, 48000)) regenerated on this host; fails -- never skips -- if they are not the fixture's inputs."""
    names, wave = S.structured_clips(48000)
    assert S.pcm_sha256(wave) == str(fxs["input_sha256"]), "this host regenerates other structured clips than the fixture was made from"
    assert names == fxs["names"].tolist()
    return names, wave


def length_clips(fxl, T):
    """(2, 1, T): synth_clips(1, T, seed=T) and the voiced generator at that length, checked against the fixture's hash."""
    wave = torch.cat([synth.synth_clips(1, T, seed=T), S.voiced_clip(T)], 0)
    got = hashlib.sha256(np.ascontiguousarray(wave.numpy()).tobytes()).hexdigest()
    assert got == str(fxl[f"input_sha256_{T}"]), f"this host regenerates other clips of {T} samples than the fixture was made from"
    return wave


def case_view(fxl, T):
    """The T case of the lengths fixture in the layout check_codes_decidable_noise reads (leading batch axis of 1)."""
    view = {k: fxl[f"{k}_{T}"] for k in KEYS}
    view["noise"] = fxl["noise"]
    return view


def rows_view(fx, rows):
    """Rows (clips) of a one-batch fixture as a fixture of their own; the batch's noise stays."""
    view = {k: fx[k][:, list(rows)] for k in KEYS}
    view["noise"] = fx["noise"]
    return view


def undecided_frames(view):
    return int((~view["decidable"][0].astype(bool)).any(1).sum())


def judge(codes, view, what, report):
    """check_codes_decidable_noise with zero mismatches, and the rule may not swallow more than the fixture allows: the positions
    it leaves uncompared (noise flips and their cascades) are at most six per frame that holds an undecidable position."""
    v = check_codes_decidable_noise(codes, view, 0)
    uncompared, bound = len(v["noise_flips"]) + v["cascade_positions"], 6 * undecided_frames(view)
    entry = {k: v[k] for k in REPORT_FIELDS}
    entry.update(uncompared=uncompared, uncompared_bound=bound, mismatch_positions=v["mismatch_positions"], mismatch_fp64_gaps=v["mismatch_fp64_gaps"])
    report[what] = entry
    print(f"[codes] {what}: {json.dumps(entry)}")
    assert v["ok"] and v["mismatches"] == 0, (what, entry)
    assert uncompared <= bound, (what, entry)
    return v


@pytest.fixture(scope="module")
def report():
    """Verdicts of this module's GPU tests, merged into the REPORT file when the module is done."""
    entries = {}
    yield entries
    if not entries:
        return
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    held = json.load(open(REPORT)) if os.path.exists(REPORT) else {}
    held.update(entries)
    json.dump(held, open(REPORT, "w"), indent=1)


@pytest.fixture(scope="module")
def full_model(cuda):
    from facodec_amd import _lib
    _lib.load()  # fails loudly if the extension is missing
    model = commons.build_model(commons.default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(cuda)
    return model


def offline(model, wave):
    with torch.no_grad():
        z = model.encoder(wave)
        outs, _, _, _, timbre, codes = model.quantizer(z, wave, n_c=2, return_codes=True)
        y = model.decoder(outs)
    return z, outs, timbre, codes, y


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_generator_contract(structured):
    names, wave = structured
    assert wave.shape == (32, 1, 48000) and wave.dtype == torch.float32 and len(names) == 32
    assert [n.split("/")[0] for n in names] == [f for f in S.FAMILIES for _ in range(4)]
    pcm = S.to_int16(wave)                                             # asserts that every sample is on the 16-bit grid
    assert not pcm[0].any() and set(np.unique(pcm[1:4]).tolist()) == {-1, 0, 1}           # digital silence; +-1 LSB dither
    # hard-clipped at full scale: at least half of the samples sit there (3 000 Hz has 8 samples per period, 4 of them clipped)
    assert all((np.abs(pcm[i, 0]) == 32767).mean() >= 0.5 and pcm[i].min() == -32767 and pcm[i].max() == 32767 for i in range(4, 8))
    for i in (16, 17, 18, 19):                                         # voiced: real pauses at the start, in the middle, at the end
        assert not pcm[i, 0, :2400].any() and not pcm[i, 0, 22500:26000].any() and not pcm[i, 0, -3000:].any() and pcm[i].any()
    assert int((pcm[23] != 0).sum()) == 1 and not pcm[27, 0, 28800:].any() and not pcm[30, 0, 24000:].any()
    assert S.voiced_clip(2101).shape == (1, 1, 2101) and S.sha256 is S.pcm_sha256


def test_inputs_regenerate_to_the_stored_hashes(structured, fxs, probes, fxl):
    assert str(fxs["input_sha256"]) == S.pcm_sha256(structured[1]) and probes["probe_clips"].tolist() == list(S.PROBE_CLIPS)
    assert fxl["lengths"].tolist() == list(LENGTHS)
    for T in LENGTHS:
        assert length_clips(fxl, T).shape == (2, 1, T)


def test_fixture_conditions(fxs, fxl, golden_dir):
    """From the reference alone: every structured clip has >= 98 % decidable positions and <= 2 % of its frames hold an
    undecidable one; `decidable` is what the stored arrays say; the length cases share the largest noise measured anywhere."""
    assert fxs["codes_f64"].shape == (1, 32, 6, 160)
    agree = (fxs["codes_f32_mt"] == fxs["codes_f32_1t"]) & (fxs["codes_f32_mt"] == fxs["codes_f64"])
    noise = float(fxs["noise"][0])
    assert 1e-7 < noise < 1e-4                    # fp32-vs-fp64 margin noise of the reference itself, as on the Gaussian batches
    assert np.array_equal(agree, fxs["agree"]) and np.array_equal(fxs["decidable"], agree & (fxs["gap_f64"].astype(np.float64) >= noise))
    dec = fxs["decidable"][0]
    for b in range(32):
        assert dec[b].sum() >= MIN_DECIDABLE * dec[b].size, (b, int(dec[b].sum()))
        assert (~dec[b]).any(0).sum() <= MAX_UNDECIDED_FRAMES * dec.shape[-1], (b, int((~dec[b]).any(0).sum()))
    assert fxs["family_positions"].tolist() == [4 * 6 * 160] * 8
    assert fxs["family_decidable"].tolist() == [int(dec[4 * f:4 * f + 4].sum()) for f in range(8)]
    rep = json.loads(str(fxl["report"]))
    fx4 = np.load(os.path.join(golden_dir, "codec_b32x4_decidable.npz"))
    everywhere = [c["own_margin_noise"] for c in rep["cases"]] + [noise] + fx4["noise"].tolist()
    assert float(fxl["noise"][0]) == max(everywhere) and rep["noise_sources"]["structured"] == noise
    assert rep["noise_sources"]["gaussian_batches"] == fx4["noise"].tolist()
    for T, c in zip(LENGTHS, rep["cases"]):
        view = case_view(fxl, T)
        assert view["codes_f64"].shape == (1, 2, 6, T // HOP) and c["T"] == T
        a = (view["codes_f32_mt"] == view["codes_f32_1t"]) & (view["codes_f32_mt"] == view["codes_f64"])
        assert np.array_equal(a, view["agree"])
        assert np.array_equal(view["decidable"], a & (view["gap_f64"].astype(np.float64) >= float(fxl["noise"][0])))
        # the reference's length rule: T // 300 code frames and 300 samples of output each; one more latent frame unless T % 300 == 0
        assert int(fxl[f"wave_len_{T}"]) == HOP * (T // HOP) and int(fxl[f"latent_frames_{T}"]) == -(-T // HOP)


def test_every_reference_run_passes_the_rule(fxs, fxl):
    views = [("structured", fxs)] + [(f"T={T}", case_view(fxl, T)) for T in LENGTHS]
    for what, view in views:
        for k in REFERENCE_RUNS:
            v = check_codes_decidable_noise(view["codes_" + k][0], view, 0)
            assert v["ok"] and v["mismatches"] == 0 and not v["noise_flips"] and v["cascade_positions"] == 0 and k in v["equals_run"], (what, k, v)


def test_one_planted_wrong_code_is_one_mismatch(fxs, fxl):
    """A single wrong code at a decidable position of the LAST stage (nothing follows it): exactly one mismatch, at that position --
    on the clip of digital silence, in the middle of a voiced clip, and at the last frame of the T = 47 999 case."""
    last = 47999 // HOP - 1
    for what, view, (b, t) in (("silence", fxs, (0, 80)), ("voiced", fxs, (17, 41)), ("T=47999", case_view(fxl, 47999), (1, last))):
        assert view["decidable"][0][b, :, t].all(), (what, b, t)
        c = view["codes_f32_mt"][0].astype(np.int64).copy()
        c[b, 5, t] = (c[b, 5, t] + 1) % 1024
        if c[b, 5, t] == view["second_f64"][0][b, 5, t]:
            c[b, 5, t] = (c[b, 5, t] + 1) % 1024
        v = check_codes_decidable_noise(c, view, 0)
        assert not v["ok"] and v["mismatches"] == 1 and v["decidable_mismatches"] == 1 and v["mismatch_positions"] == [[b, 5, t]], (what, v)
    # ... and at the first stage of a frame every later stage is still compared with the runs that went the product's way: none did
    c = fxs["codes_f64"][0].astype(np.int64).copy()
    c[0, 0, 80] = (c[0, 0, 80] + 1) % 1024
    v = check_codes_decidable_noise(c, fxs, 0)
    assert not v["ok"] and v["mismatch_positions"][0] == [0, 0, 80] and v["cascade_positions"] == 0


def test_structured_batch_reaches_more_of_the_prosody_codebook_than_the_gaussian_batch(fxs, golden_dir):
    held = np.load(os.path.join(golden_dir, "codec_b32.npz"))
    structured_codes, gaussian_codes = np.unique(fxs["codes_f64"][0][:, 0]), np.unique(held["codes"][:, 0])
    print(f"[prosody] distinct codes: structured {len(structured_codes)}, Gaussian {len(gaussian_codes)}")
    assert len(structured_codes) > len(gaussian_codes)


# ------------------------------------------------------------------------------------------------------------------ GPU
@gpu
def test_structured_batch_offline(full_model, structured, fxs, probes, report, cuda):
    """The 32 structured clips through model.encoder -> model.quantizer(n_c=2, return_codes=True) -> model.decoder: no mismatch
    under the reference's rule; latent, quantizer output, waveform and timbre of one clip per family within E2E_TOL of THAT clip's
    fp64 absmax (the batch's would hide a quiet clip)."""
    wave = structured[1].to(cuda)
    z, outs, timbre, codes, y = offline(full_model, wave)
    assert sum(c.shape[1] for c in codes) == 6 and y.shape == (32, 1, 48000)
    pc = probes["probe_clips"].tolist()
    assert pc == list(S.PROBE_CLIPS)
    got = {"z": z[pc][:, ::8, :], "outs": outs[pc][:, ::8, :], "wave": y[pc][:, 0, torch.from_numpy(probes["probe_t"]).to(cuda)], "timbre": timbre[pc]}
    errs = {}
    for k, g in got.items():
        d = np.abs(g.detach().cpu().double().numpy() - probes[k + "_probe"].astype(np.float64)).reshape(len(pc), -1).max(1)
        errs[k] = (d / probes[k + "_absmax"]).tolist()
    report["structured_offline_probe_rel_err"] = {"probe_clips": pc, "product": errs,
                                                  "reference_fp32": {k: probes[k + "_ref_f32_rel_err"].tolist() for k in got}}
    print(f"[tol] structured probes (per clip, own absmax): {json.dumps(report['structured_offline_probe_rel_err'])}")
    judge(codes, fxs, "structured_offline", report)
    for f in range(8):
        report[f"structured_offline_family_{S.FAMILIES[f]}"] = {
            k: v for k, v in check_codes_decidable_noise([c[4 * f:4 * f + 4] for c in codes], rows_view(fxs, range(4 * f, 4 * f + 4)), 0).items()
            if k in REPORT_FIELDS}
    for k, e in errs.items():
        assert max(e) < E2E_TOL, (k, e)


@gpu
@pytest.mark.parametrize("T", LENGTHS)
def test_lengths_offline(full_model, fxl, report, cuda, T):
    """Both clips of every length case through the same three calls: the code shape and the output length are the reference's,
    no mismatch under its rule.  The two long cases run the timbre attention on the stream route."""
    from facodec_amd import ops
    wave = length_clips(fxl, T).to(cuda)
    attn = full_model.quantizer.timbre_encoder.slf_attn
    route = ops.attention_route(attn.conv_q.c_out // attn.n_heads, T // HOP)      # the timbre attention's shape: dk = 64, T // 300 keys
    if T in LONG:
        assert route == "stream", (T, route)
    else:
        assert route == "lds", (T, route)
    z, outs, timbre, codes, y = offline(full_model, wave)
    assert [tuple(c.shape) for c in codes] == [(2, n, T // HOP) for n in (1, 2, 3)]
    assert y.shape == (2, 1, int(fxl[f"wave_len_{T}"]))
    judge(codes, case_view(fxl, T), f"lengths_offline_T={T}", report)


@gpu
def test_clip_list_call(full_model, fxl, report, cuda):
    """commons.encode_clips on the clips of the length cases as ONE list in a scrambled order, every clip judged by the reference's
    rule (no near-tie allowance: the reference is the arbiter, not the product's own single-clip run).  plan_groups puts the
    list into three padded batches (the two long lengths get one each), so no short clip is padded to 30 s.  The clip-list calls
    refuse clips under commons.min_clip_samples (3000 samples: a padded batch cannot reproduce the zero extension the encoder's
    reflect paddings fall back to below it; tests/test_ragged_batch.py pins that refusal), so the 1 025- and 2 101-sample clips must
    be refused, by a ValueError that names the limit, and the eight clips of the other four lengths are encoded."""
    need = commons.min_clip_samples(full_model)
    taken = [T for T in LENGTHS if T >= need]
    assert taken == [47999, 48001, 691500, 720001]
    clips = {T: length_clips(fxl, T).to(cuda) for T in LENGTHS}
    for T in LENGTHS:
        if T < need:
            with pytest.raises(ValueError, match=str(need)):
                commons.encode_clips(full_model, [clips[48001][0], clips[T][1]], n_c=2)
    order = [(720001, 1), (47999, 0), (691500, 1), (48001, 1), (47999, 1), (720001, 0), (48001, 0), (691500, 0)]
    enc = commons.encode_clips(full_model, [clips[T][i] for T, i in order], n_c=2)
    torch.cuda.synchronize()
    for T in taken:
        per_clip = [enc[order.index((T, i))] for i in (0, 1)]
        codes = [torch.stack([c["codes"][s] for c in per_clip]) for s in range(3)]
        assert [tuple(c.shape) for c in codes] == [(2, n, T // HOP) for n in (1, 2, 3)]
        judge(codes, case_view(fxl, T), f"clip_list_T={T}", report)


@gpu
@pytest.mark.parametrize("use_graphs", [False, True])
def test_streaming_session(full_model, structured, fxs, report, cuda, use_graphs):
    """StreamingCodec on four structured clips (silence-dither, voiced with pauses, clipped sine, impulse train): primed with 4 800
    samples, 90 hops of 480, finish; the timbre is the offline product's.  The concatenated codes against those clips' rows of
    the structured fixture (the batch's noise), no mismatch."""
    from facodec_amd.streaming import HOP as STREAM_HOP, StreamingCodec
    rows = list(S.STREAMING_CLIPS)
    assert [structured[0][i].split("/")[0] for i in rows] == ["silence", "voiced", "clipped_sine", "impulses"] and STREAM_HOP == 480
    wave = structured[1][rows].to(cuda)
    keep = lambda o: {k: ([c.clone() for c in v] if isinstance(v, list) else (v.clone() if torch.is_tensor(v) else v)) for k, v in o.items()}   # noqa: E731
    with torch.no_grad():
        timbre = full_model.quantizer(full_model.encoder(wave), wave, n_c=2)[4]
        sess = StreamingCodec(full_model, timbre, n_c=2, use_graphs=use_graphs)
        pieces = [keep(sess.prime(wave[:, :, :4800]))]
        for h in range(90):
            pieces.append(keep(sess.push(wave[:, :, 4800 + h * 480: 4800 + (h + 1) * 480])))
        pieces.append(keep(sess.finish()))
    got, frame = [[], [], []], 0
    for o in pieces:
        if o["codes"] is None:
            continue
        assert o["frame0"] == frame
        frame += o["codes"][0].shape[-1]
        for i in range(3):
            got[i].append(o["codes"][i])
    assert frame == 160
    judge([torch.cat(g, -1) for g in got], rows_view(fxs, rows), f"streaming_graphs={use_graphs}", report)
