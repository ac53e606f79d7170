"""Loudness on the GPU: fac_kweight_energy against a float64 direct-form recurrence on chunk, segment and
sub-block boundaries; fac_loudness_gate against the restated two-gate rule; ops.normalize_loudness against the fp64 gain rule;
clip lists, the streaming meter, and the level-normalised compress / decompress.

The reference is tests/test_loudness_cpu.py's (`biquad`, `kweight_energies`, `gated`), which that file pins to the standard.
Bounds.  Energies: |e - e_ref| <= 1e-10 * max_j e_ref[b, j] per row -- the chunked hand-over against the direct form differs by
fp64 rounding amplified by the high-pass poles (measured: 1.1e-15 .. 1.3e-14 of the row's maximum at 24 kHz, 1.2e-13 at
384 kHz), a wrong hand-over by 1e-3 and more; the bound is relative to the row's maximum because a quiet sub-block behind a loud one carries the loud one's rounding.  Loudness:
1e-6 LU.  Gain: 2.4e-7 relative, one fp32 rounding of g and one of the product."""
import math

import numpy as np
import pytest
import torch

from facodec_amd import bitstream, synth
from test_loudness_cpu import gain_ref, gated, kweight_energies, loudness_ref

pytestmark = pytest.mark.gpu

RATE, S = 24000, 2400
E_TOL, L_TOL, G_TOL = 1e-10, 1e-6, 2.4e-7
LENS = [72000, 30001, 7000, 0]


def momentary_ref(e, n=4):
    z = float(np.sum(e[-n:])) / (n * S)
    return max(-70.0, -0.691 + 10.0 * math.log10(z)) if z > 0.0 else -70.0


def row0():
    """1 s of Gaussian noise at 0.1, 1 s at 0.001, 1 s of zeros."""
    g = np.random.default_rng(1770)
    return np.concatenate([0.1 * g.standard_normal(24000), 0.001 * g.standard_normal(24000), np.zeros(24000)]).astype(np.float32)


@pytest.fixture(scope="module")
def batch():
    """The four rows of one launch and their reference energies, computed once and never written to."""
    g = np.random.default_rng(4)
    rows = [row0(), (0.05 * g.standard_normal(30001)).astype(np.float32), (0.2 * g.standard_normal(7000)).astype(np.float32),
            np.zeros(0, dtype=np.float32)]
    x = np.full((4, 72000), 7.0, dtype=np.float32)                 # what lies behind a clip's end must never be read as signal
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    e_ref = [kweight_energies(r) for r in rows]
    return dict(rows=rows, x=x, e_ref=e_ref, L_ref=[gated(e, len(r), S) for e, r in zip(e_ref, rows)])


def check_energies(e, e_ref, what=""):
    e = np.asarray(e)
    assert e.shape[0] >= len(e_ref)
    if len(e_ref) and not np.any(e_ref):                            # a silent row: exact zeros
        assert not np.any(e[:len(e_ref)]), what
    elif len(e_ref):
        err = float(np.max(np.abs(e[:len(e_ref)] - e_ref))) / float(np.max(e_ref))
        print(f"{what}: energy error {err:.3e} of the row's maximum")
        assert err <= E_TOL, (what, err)
    assert not np.any(e[len(e_ref):]), what


# ---------------------------------------------------------------------------------------------------------------- energies
def test_energies_of_a_ragged_batch(cuda, batch):
    from facodec_amd import ops
    x = torch.from_numpy(batch["x"]).to(cuda)
    lens = torch.tensor(LENS, dtype=torch.int32, device=cuda)
    en = ops.loudness_energies(x, RATE, lens=lens)
    assert en.e.shape == (4, 30) and en.e.dtype == torch.float64 and en.peak.dtype == torch.float32 and en.state is None
    e = en.e.cpu().numpy()
    for b in range(4):
        check_energies(e[b], batch["e_ref"][b], f"row {b}")
    assert en.peak.cpu().tolist() == [float(np.max(np.abs(r))) if len(r) else 0.0 for r in batch["rows"]]
    again = ops.loudness_energies(x.unsqueeze(1), RATE, lens=lens)                  # (B, 1, T), and bit for bit the same
    assert torch.equal(again.e, en.e) and torch.equal(again.peak, en.peak)
    # a row alone is the row of the batch, bit for bit; rows of another pitch are taken as they are
    alone = ops.loudness_energies(x[1:2, :30001].contiguous(), RATE)
    assert torch.equal(alone.e[0], en.e[1, :13])
    wide = torch.zeros(4, 72000 + 3, device=cuda)
    wide[:, 1:72001] = x
    assert torch.equal(ops.loudness_energies(wide[:, 1:72001], RATE, lens=lens).e, en.e)


def _boundary_lengths():
    from facodec_amd import ops
    L, W = ops.loudness_chunk(), ops.loudness_chunk_group()
    return L, W, [L - 1, L, L + 1, 2 * L + 1, W * L - 1, W * L, W * L + 1, 2 * W * L + 1, 65 * W * L + 1]


@pytest.mark.parametrize("case", range(9))
def test_energies_on_chunk_and_segment_boundaries(cuda, case):
    """T on both sides of a chunk and of a segment (workgroup) boundary, with an impulse as the last sample of the first chunk,
    of the first segment and of the 64th: the hand-over has to carry it into the next chunk / segment.  The last case has more
    than 64 segments, where the scan across segments goes into its second round (a million samples: the smallest such size)."""
    from facodec_amd import ops
    L, W, lengths = _boundary_lengths()
    assert (L, W) == (256, 64)
    T = lengths[case]
    g = np.random.default_rng(100 + case)
    x = (0.01 * g.standard_normal(T)).astype(np.float32)
    for at in (L - 1, W * L - 1, 64 * W * L - 1):
        if at < T:
            x[at] = 0.9
    en = ops.loudness_energies(torch.from_numpy(x).to(cuda)[None], RATE)
    assert en.e.shape == (1, -(-T // S))
    check_energies(en.e[0].cpu().numpy(), kweight_energies(x), f"T = {T}")
    assert float(en.peak[0]) == float(np.max(np.abs(x)))
    assert abs(float(ops.loudness(torch.from_numpy(x).to(cuda)[None])[0]) - loudness_ref(x)) <= L_TOL


def test_hand_over_across_segments_at_a_rate_where_it_shows(cuda):
    """At 24 kHz the high-pass forgets a state within one segment (0.990^16384), so no 24 kHz signal can tell whether states cross
    segment boundaries correctly.  At 384 kHz the pole radius is 0.99938 and 3e-5 of a state survives a segment: a loud burst at
    the end of segment 0 and of segment 63 (the last of the scan's first round) in front of near-silence.  The test first shows,
    on the reference alone, that resetting the state at the round's boundary moves an energy by more than 1e-6 of the maximum."""
    from facodec_amd import dsp, ops
    from test_loudness_cpu import biquad
    rate, seg = 384000, ops.loudness_chunk() * ops.loudness_chunk_group()
    T, cut = 66 * seg, 64 * seg
    g = np.random.default_rng(384)
    x = (1e-6 * g.standard_normal(T)).astype(np.float32)
    for end in (seg, cut):
        x[end - 512:end] = (0.5 * g.standard_normal(512)).astype(np.float32)
    (b1, a1), (b2, a2) = dsp.k_weighting(rate)

    def energies(parts):
        y = np.concatenate([biquad(biquad(p, b1, a1), b2, a2) for p in parts])
        return np.array([np.sum(y[j:j + rate // 10] ** 2) for j in range(0, T, rate // 10)])

    e_ref, e_reset = energies([x]), energies([x[:cut], x[cut:]])
    assert float(np.max(np.abs(e_ref - e_reset))) > 1e-6 * float(np.max(e_ref))
    en = ops.loudness_energies(torch.from_numpy(x).to(cuda)[None], rate)
    err = float(np.max(np.abs(en.e[0].cpu().numpy() - e_ref))) / float(np.max(e_ref))
    print(f"384 kHz, 66 segments: energy error {err:.3e} of the row's maximum")
    assert err <= E_TOL


# ---------------------------------------------------------------------------------------------------------------- gates
def test_gates(cuda, batch):
    """Row 0 is built so that each gate moves the result by more than 1.3 LU: 27 blocks, of which 20 pass the absolute gate and
    10 both.  (The figures the design was made with, for another draw of the same noise: -17.8116 fully gated, -20.8214 with the
    absolute gate alone, -22.1248 ungated; a second of white noise fixes its level to about 0.04 LU, so this draw must land
    within 0.15 LU of them.)"""
    from facodec_amd import ops
    e0 = batch["e_ref"][0]
    from test_loudness_cpu import block_levels
    z, l = block_levels(e0, 72000, S)
    full, absolute, ungated = gated(e0, 72000, S), gated(e0, 72000, S, gates=1), gated(e0, 72000, S, gates=0)
    print(f"row 0: {full:.4f} gated, {absolute:.4f} absolute gate alone, {ungated:.4f} ungated")
    assert len(z) == 27 and int(np.sum(l > -70.0)) == 20
    gr = -0.691 + 10.0 * math.log10(z[l > -70.0].mean()) - 10.0
    assert int(np.sum((l > -70.0) & (l > gr))) == 10
    assert abs(full + 17.8116) < 0.15 and abs(absolute + 20.8214) < 0.15 and abs(ungated + 22.1248) < 0.15
    assert absolute < full - 1.3 and ungated < absolute - 1.3
    # no block within 1e-3 LU of either gate, in any row: a decision cannot flip in rounding
    for e, r in zip(batch["e_ref"][:3], batch["rows"][:3]):
        zz, ll = block_levels(e, len(r), S)
        keep = ll > -70.0
        g2 = -0.691 + 10.0 * math.log10(zz[keep].mean()) - 10.0
        assert np.min(np.abs(ll - (-70.0))) > 1e-3 and np.min(np.abs(ll - g2)) > 1e-3

    x = torch.from_numpy(batch["x"]).to(cuda)
    lens = torch.tensor(LENS, dtype=torch.int32, device=cuda)
    Lg = ops.loudness(x, RATE, lens=lens)
    assert Lg.shape == (4,) and Lg.dtype == torch.float64 and Lg.is_cuda
    got = Lg.cpu().tolist()
    for b in range(4):
        print(f"row {b}: {got[b]:.9f} LUFS, reference {batch['L_ref'][b]:.9f}")
        assert abs(got[b] - batch["L_ref"][b]) <= L_TOL
    assert len(block_levels(batch["e_ref"][2], 7000, S)[0]) == 1                     # under 400 ms: one zero-padded block
    assert got[3] == -70.0                                                          # the empty clip
    assert ops.loudness(torch.zeros(2, 1, 30000, device=cuda)).cpu().tolist() == [-70.0, -70.0]
    # the other modes of the gate entry, on the same energies
    en = ops.loudness_energies(x, RATE, lens=lens)
    mom = ops.loudness_gate(en.e, 72000, RATE, lens=lens, last_n=4).cpu().tolist()
    for b in range(3):
        assert abs(mom[b] - momentary_ref(batch["e_ref"][b])) <= L_TOL
    assert mom[3] == -70.0


def test_the_standards_tone(cuda):
    from facodec_amd import ops
    t = np.arange(48000) / 24000.0
    x = torch.from_numpy((0.5 * np.sin(2.0 * math.pi * 997.0 * t)).astype(np.float32)).to(cuda)
    got = float(ops.loudness(x[None])[0])
    print(f"997 Hz at 0.5: {got:.4f} LUFS")
    assert abs(got - (-2.9843 + 20.0 * math.log10(0.5))) <= 0.01


# ---------------------------------------------------------------------------------------------------------------- normalise
def test_normalize_loudness(cuda):
    from facodec_amd import ops
    g = np.random.default_rng(16)
    T = 48000
    x = np.zeros((4, T), dtype=np.float32)
    x[0] = 0.05 * g.standard_normal(T)
    x[1] = 0.001 * g.standard_normal(T)
    x[1, 12345] = -0.99                                         # the guard's row: levelled, this sample would leave full scale
    x[3] = 0.02 * g.standard_normal(T)
    lens_h = [T, T, T, 30001]                                   # row 2 is silent, row 3 ends early
    x_dev = torch.from_numpy(x).to(cuda)
    x_dev[3, 30001:] = 5.0
    lens = torch.tensor(lens_h, dtype=torch.int32, device=cuda)
    y, L, gain = ops.normalize_loudness(x_dev, -16.0, RATE, lens=lens)
    assert y.shape == x_dev.shape and L.dtype == torch.float64 and gain.dtype == torch.float32 and y.is_cuda and L.is_cuda and gain.is_cuda
    y_h, L_h, g_h = y.cpu().numpy(), L.cpu().tolist(), gain.cpu().numpy()
    for b in range(4):
        xb = x[b, :lens_h[b]]
        L_ref = loudness_ref(xb)
        g_ref = gain_ref(L_ref, -16.0, float(np.max(np.abs(xb))))
        print(f"row {b}: input {L_h[b]:.6f} LUFS (reference {L_ref:.6f}), gain {g_h[b]:.8g} (reference {g_ref:.8g})")
        assert abs(L_h[b] - L_ref) <= L_TOL
        assert abs(float(g_h[b]) - g_ref) <= G_TOL * g_ref
        want = xb.astype(np.float64) * g_ref
        assert np.all(np.abs(y_h[b, :lens_h[b]] - want) <= G_TOL * np.abs(want))
        assert np.array_equal(y_h[b, :lens_h[b]], xb * g_h[b])                      # one fp32 product with the gain it reports
        assert not np.any(y_h[b, lens_h[b]:])                                       # zeros behind the clip
    after = ops.loudness(y, RATE, lens=lens).cpu().tolist()
    for b in (0, 3):
        assert abs(after[b] + 16.0) <= 1e-5, (b, after[b])
    assert g_h[1] == np.float32(1.0 / float(np.float32(0.99)))                      # the guard: gain == 1 / peak ...
    top = float(np.max(np.abs(y_h[1])))
    assert abs(top - 1.0) <= float(np.spacing(np.float32(1.0)))                     # ... and max |y| == 1 within one ulp
    assert g_h[2] == 1.0 and L_h[2] == -70.0 and not np.any(y_h[2])                  # silence comes back as it is
    y3, _, _ = ops.normalize_loudness(x_dev.unsqueeze(1), -16.0, RATE, lens=lens)
    assert y3.shape == (4, 1, T) and torch.equal(y3[:, 0], y)


# ---------------------------------------------------------------------------------------------------------------- lists
def test_loudness_of_clip_lists_does_not_depend_on_the_grouping(cuda):
    from facodec_amd import commons, ops
    lengths = [24000, 4800, 48000, 11111, 30001]                                    # 0.2 .. 2 s, in no order
    g = np.random.default_rng(5)
    clips = [torch.from_numpy((0.1 * (i + 1) * g.standard_normal(n)).astype(np.float32)).to(cuda) for i, n in enumerate(lengths)]
    clips[2] = clips[2][None]                                                       # (1, T) is a clip too
    assert len(commons.plan_groups(lengths, 60002)) == 3
    got = commons.loudness_clips(clips, RATE, max_batch_samples=60002)
    assert isinstance(got, list) and all(isinstance(v, float) for v in got)
    alone = [float(ops.loudness(c.reshape(1, -1))[0]) for c in clips]
    one_group = commons.loudness_clips(clips)
    for a, b, c in zip(got, alone, one_group):
        assert abs(a - b) <= 1e-9 and abs(c - b) <= 1e-9
    assert len({round(v, 3) for v in alone}) == 5
    assert commons.loudness_clips([]) == []
    with pytest.raises(ValueError, match="resample first"):
        commons.loudness_clips(clips, 11025)


# ---------------------------------------------------------------------------------------------------------------- streaming
def _blocks(first, hop, total):
    sizes, n = [], 0
    for k in first:
        sizes.append(k)
        n += k
    while n < total:
        sizes.append(min(hop, total - n))
        n += sizes[-1]
    return sizes


@pytest.mark.parametrize("first", [(1, 7, 479, 2400), ()], ids=["ragged-blocks", "480-hops"])
def test_streaming_meter(cuda, batch, first):
    """Two streams, row 0 and row 0 backwards (the loud second last, so that the momentary figure is no -70), fed in blocks
    that start and end anywhere in a chunk and in a sub-block.  The energy history starts at 1 s and has to double twice."""
    from facodec_amd import ops
    from facodec_amd.streaming import LoudnessMeter
    x = np.stack([batch["rows"][0], batch["rows"][0][::-1].copy()])
    e_ref = [batch["e_ref"][0], kweight_energies(x[1])]
    x_dev = torch.from_numpy(x).to(cuda)
    offline = ops.loudness_energies(x_dev, RATE).e.cpu().numpy()
    meter = LoudnessMeter(2, RATE, device=cuda, seconds=1)
    n, mid = 0, None
    for k in _blocks(first, 480, 72000):
        meter.push(x_dev[:, None, n:n + k] if n % 960 else x_dev[:, n:n + k])
        n += k
        if n == 2887 + 10 * 480 or (not first and n == 16 * 480):
            mid = (n, meter.momentary().cpu().tolist(), meter.energies.cpu().numpy().copy())
    assert meter.samples == 72000 and meter.energies.shape == (2, 30)
    e = meter.energies.cpu().numpy()
    for b in range(2):
        check_energies(e[b], e_ref[b], f"stream {b}")
        assert float(np.max(np.abs(e[b] - offline[b]))) <= E_TOL * float(np.max(e_ref[b]))
    integ, mom, short = meter.integrated().cpu().tolist(), meter.momentary().cpu().tolist(), meter.short_term().cpu().tolist()
    for b in range(2):
        assert abs(integ[b] - gated(e_ref[b], 72000, S)) <= L_TOL
        assert abs(mom[b] - momentary_ref(e_ref[b], 4)) <= L_TOL
        assert abs(short[b] - momentary_ref(e_ref[b], 30)) <= L_TOL
    assert mom[1] > -30.0
    assert meter.peak.cpu().tolist() == [float(np.max(np.abs(x[0])))] * 2
    # in the middle of a sub-block: the last four sub-blocks, the open one included
    n_mid, mom_mid, e_mid = mid
    assert n_mid % S
    for b in range(2):
        part = kweight_energies(x[b, :n_mid])
        check_energies(e_mid[b], part, f"stream {b} at {n_mid}")
        assert abs(mom_mid[b] - momentary_ref(part, 4)) <= L_TOL
    with pytest.raises(ValueError):
        meter.push(x_dev[:, :0])


# ---------------------------------------------------------------------------------------------------------------- the codec
@pytest.fixture(scope="module")
def full_model(cuda):
    from facodec_amd.commons import build_model, default_model_params
    model = build_model(default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(cuda)
    return model


def _f32(v):
    return float(np.float32(v))


def _restored(out, plain, input_db):
    """What decompress owes a flagged row: its loudness back at input_db within 1e-4 LU -- unless the decoded audio measures -70,
    which the rule leaves alone.  -> True when the row was restored."""
    from facodec_amd import ops
    L_plain = float(ops.loudness(plain.reshape(1, -1))[0])
    L_out = float(ops.loudness(out.reshape(1, -1))[0])
    print(f"decoded at {L_plain:.4f} LUFS, restored to {L_out:.4f}, input_db {input_db:.4f}")
    if L_plain <= -70.0:
        assert torch.equal(out, plain)
        return False
    assert abs(L_out - input_db) <= 1e-4
    return True


def test_compress_levels_and_decompress_restores(full_model, cuda):
    """B = 2 x 0.5 s.  With the seeded synthetic weights the decoder's output is audible (it does not measure -70), so the
    restoring branch is the one that runs here; the -70 branch is the silent-row case of test_normalize_loudness's rule."""
    from facodec_amd import commons, ops
    m = full_model
    w = (0.3 * synth.synth_clips(2, 12000, seed=46)).to(cuda)
    w[1] *= 0.2
    plain = commons.compress(m, w)
    assert plain == commons.compress(m, w, normalize_db=None)
    assert all(bitstream.read(b)[0].input_db is None and bitstream.read(b)[0].flags == 1 for b in plain)

    blobs = commons.compress(m, w, normalize_db=-16.0)
    L_in = ops.loudness(w).cpu().tolist()
    y, _, gain = ops.normalize_loudness(w, -16.0)
    with torch.no_grad():
        out = m.quantizer(m.encoder(y), y, n_c=2, return_codes=True)
    timbre, codes = out[4], out[5]
    rows = ops.pack_codes(codes, bits=10).cpu().numpy()
    for b, blob in enumerate(blobs):
        hdr, tim, payload = bitstream.read(blob)
        assert len(blob) == len(plain[b]) + 4 and hdr.flags == 5 and hdr.version == 1
        assert hdr.input_db == _f32(L_in[b])
        assert payload == rows[b, :bitstream.payload_bytes(40, 6, 10)].tobytes()      # the codes of the levelled audio ...
        assert np.array_equal(tim, timbre[b].cpu().numpy())                           # ... and its timbre
    assert abs(float(gain[0]) - 10.0 ** ((-16.0 - L_in[0]) / 20.0)) <= G_TOL * float(gain[0])
    quiet = commons.compress(m, 0.25 * w, normalize_db=-16.0)
    for b in range(2):
        assert abs(bitstream.read(blobs[b])[0].input_db - bitstream.read(quiet[b])[0].input_db - 20.0 * math.log10(4.0)) <= 1e-5

    same_codes = commons.decode_codes(m, codes, timbre)
    off = commons.decompress(m, blobs, restore_loudness=False)
    assert torch.equal(torch.stack(off), same_codes)
    on = commons.decompress(m, blobs)
    assert all(o.shape == (1, 12000) for o in on)
    assert [_restored(on[b], off[b], bitstream.read(blobs[b])[0].input_db) for b in range(2)] == [True, True]
    # flagged and unflagged blobs in one call: the gain is per row
    mixed = commons.decompress(m, [blobs[0], plain[1]])
    assert torch.equal(mixed[0], on[0]) and torch.equal(mixed[1], commons.decompress(m, plain)[1])
    one = commons.compress(m, w[0, 0], normalize_db=-16.0)
    assert isinstance(one, bytes) and bitstream.read(one)[0].input_db == _f32(L_in[0])


def test_compress_clips_levels_every_clip_on_its_own_samples(full_model, cuda):
    from facodec_amd import commons, ops
    m = full_model
    w = (0.3 * synth.synth_clips(3, 4500, seed=47)).to(cuda)
    clips = [w[0, 0, :3000], 0.1 * w[1, :, :4500], w[2, 0, :3650]]
    assert commons.compress_clips(m, clips) == commons.compress_clips(m, clips, normalize_db=None)
    blobs = commons.compress_clips(m, clips, normalize_db=-16.0)
    headers = [bitstream.read(b)[0] for b in blobs]
    assert [h.n_frames for h in headers] == [10, 15, 12]
    alone = [float(ops.loudness(c.reshape(1, -1))[0]) for c in clips]
    assert [h.input_db for h in headers] == [_f32(v) for v in alone]
    levelled = [ops.normalize_loudness(c.reshape(1, -1).contiguous(), -16.0)[0][0] for c in clips]
    want = commons.compress_clips(m, levelled)
    for b in range(3):
        assert bitstream.read(blobs[b])[2] == bitstream.read(want[b])[2]             # the codes of every clip levelled alone
    on = commons.decompress(m, blobs)
    off = commons.decompress(m, blobs, restore_loudness=False)
    assert all(_restored(on[b], off[b], headers[b].input_db) for b in range(3))


def test_compress_long_levels_the_whole_recording(full_model, cuda):
    from facodec_amd import commons, ops
    m = full_model
    wave = (0.1 * synth.synth_clips(2, 9750, seed=48)).to(cuda)                      # 32 frames in chunks of 0.2 s = 16 frames
    assert commons.compress_long(m, wave, chunk_seconds=0.2) == commons.compress_long(m, wave, chunk_seconds=0.2, normalize_db=None)
    blobs = commons.compress_long(m, wave, chunk_seconds=0.2, normalize_db=-16.0)
    headers = [bitstream.read(b)[0] for b in blobs]
    L_in = ops.loudness(wave).cpu().tolist()
    assert [h.input_db for h in headers] == [_f32(v) for v in L_in] and headers[0].n_frames == 32
    want = commons.compress_long(m, ops.normalize_loudness(wave, -16.0)[0], chunk_seconds=0.2)
    for b in range(2):
        (_, tim, payload), (_, tim_w, payload_w) = bitstream.read(blobs[b]), bitstream.read(want[b])
        assert np.array_equal(tim, tim_w) and payload == payload_w                   # codes and timbre of the levelled recording
    on = commons.decompress_long(m, blobs, chunk_seconds=0.2)
    off = commons.decompress_long(m, blobs, chunk_seconds=0.2, restore_loudness=False)
    assert on.shape == (2, 1, 9600)
    assert torch.equal(off, commons.decompress_long(m, want, chunk_seconds=0.2))
    assert all(_restored(on[b], off[b], headers[b].input_db) for b in range(2))
