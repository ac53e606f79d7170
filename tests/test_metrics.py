"""Objective scores on the GPU: ops.si_sdr, ops.stoi_scores and the clip-list calls against the float64 numpy
restatement of tests/test_metrics_cpu.py (`si_sdr_ref`, `stoi_ref`), which that file pins on its own.

Decidability.  Which frames STOI keeps is a threshold on the reference's frame energies; the kept indices are compared exactly,
so every row's reference must be decidable: its keep margin min_m |max E - 40 - E_m| is asserted to be at least 1e-3 dB from
the reference alone before anything is compared (the rows here have 19.5 dB and more; the device's E differs from numpy's by
about 1e-13 dB).  Seeds are chosen so that this holds; no case is skipped on that ground.

Bounds, against the reference and never against the code under test: a hundred times the largest error measured on an MI355X,
which lies far inside the caps of 1e-6 (STOI / ESTOI; the smallest mutation test_metrics_cpu.py measures moves STOI by 1e-3)
and 1e-9 dB (SI-SDR).  Measured maxima over all cases of this file: |STOI - ref| 2.22e-16, |ESTOI - ref| 2.22e-16 (the device's
transform is fp64 like the reference's, and both scores are means of correlations of size <= 1), |SI-SDR - ref| 7.11e-15 dB."""
import math

import numpy as np
import pytest
import torch

from facodec_amd import synth
from test_metrics_cpu import at_snr, gap_row, noise_row, si_sdr_ref, stoi_ref

pytestmark = pytest.mark.gpu

STOI_TOL, SDR_TOL, MARGIN = 2.3e-14, 7.2e-13, 1e-3
PAD = 7.0                                                # what lies behind a row's end must never be read as signal


def _padded(rows, T=None):
    T = max(len(r) for r in rows) if T is None else T
    out = np.full((len(rows), T), PAD, dtype=np.float32)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def same_bits(a, b):
    return all(torch.equal(_bits(u), _bits(v)) for u, v in zip(a[:5], b[:5]))


def check_stoi(got, xs, ys, what):
    """got: StoiScores of the batch whose rows are xs / ys (numpy, each row's own samples).  -> (max STOI error, max ESTOI error)."""
    stoi, estoi = got.stoi.cpu().numpy(), got.estoi.cpu().numpy()
    n_frames, n_kept, n_seg, kept = (t.cpu().numpy() for t in (got.n_frames, got.n_kept, got.n_segments, got.kept_idx))
    worst = [0.0, 0.0]
    for b, (x, y) in enumerate(zip(xs, ys)):
        s_ref, e_ref, k_ref, margin = stoi_ref(x, y)
        assert margin >= MARGIN, (what, b, margin)                                   # decidable from the reference alone
        assert n_frames[b] == ((len(x) - 256) // 128 + 1 if len(x) >= 256 else 0), (what, b)
        assert n_kept[b] == len(k_ref) and np.array_equal(kept[b, :len(k_ref)], k_ref), (what, b)
        assert np.all(kept[b, len(k_ref):] == -1), (what, b)
        assert n_seg[b] == max(len(k_ref) - 29, 0), (what, b)
        if math.isnan(s_ref):
            assert math.isnan(stoi[b]) and math.isnan(estoi[b]) and n_seg[b] == 0, (what, b)
            continue
        worst = [max(worst[0], abs(stoi[b] - s_ref)), max(worst[1], abs(estoi[b] - e_ref))]
        assert abs(stoi[b] - s_ref) <= STOI_TOL and abs(estoi[b] - e_ref) <= STOI_TOL, (what, b, stoi[b], s_ref, estoi[b], e_ref)
    print(f"{what}: max |STOI - ref| = {worst[0]:.3e}, max |ESTOI - ref| = {worst[1]:.3e}")
    return worst


# ---------------------------------------------------------------------------------------------------------------- STOI / ESTOI
@pytest.fixture(scope="module")
def ragged():
    """The rows of one launch at 10 kHz, built once and never written to."""
    gap = gap_row()
    xs = [noise_row(3968, 11), noise_row(3840, 12), gap, noise_row(200, 13), np.zeros(0, dtype=np.float32),
          np.zeros(4500, dtype=np.float32), gap]
    ys = [at_snr(xs[0], 20.0, 21), at_snr(xs[1], 20.0, 22), at_snr(gap, -5.0, 23), at_snr(xs[3], 5.0, 24), np.zeros(0, dtype=np.float32),
          noise_row(4500, 25), at_snr(gap, 20.0, 26)]
    return dict(xs=xs, ys=ys, x=_padded(xs), y=_padded(ys), lens=[len(r) for r in xs])


def test_stoi_of_a_ragged_batch(cuda, ragged):
    """One segment exactly (K = 30), one frame short of it (NaN), kept frames that are not adjacent, a row under one frame, an
    empty row, a zero reference (0.0 on both scores), estimates at +20 and -5 dB."""
    from facodec_amd import ops
    x, y = torch.from_numpy(ragged["x"]).to(cuda), torch.from_numpy(ragged["y"]).to(cuda)
    lens = torch.tensor(ragged["lens"], dtype=torch.int32, device=cuda)
    got = ops.stoi_scores(x, y, 10000, lens)
    assert got.stoi.dtype == torch.float64 and got.stoi.shape == (7,) and got.kept_idx.shape == (7, 45)
    check_stoi(got, ragged["xs"], ragged["ys"], "ragged batch")
    assert got.n_kept.cpu().tolist() == [30, 29, 39, 0, 0, 34, 39] and got.n_segments.cpu().tolist() == [1, 0, 10, 0, 0, 5, 10]
    assert got.stoi.cpu().tolist()[5] == 0.0 and got.estoi.cpu().tolist()[5] == 0.0
    assert float(got.stoi[6]) > float(got.stoi[2]) and float(got.estoi[6]) > float(got.estoi[2])
    assert torch.equal(_bits(ops.stoi(x, y, 10000, lens)), _bits(got.stoi))
    assert torch.equal(_bits(ops.stoi(x, y, 10000, lens, extended=True)), _bits(got.estoi))
    from facodec_amd._lib import FacodecHipError
    for bad in (lens.to(torch.int64), lens[:3], lens.cpu()):
        with pytest.raises(FacodecHipError, match="lens must"):
            ops.stoi_scores(x, y, 10000, bad)
        with pytest.raises(FacodecHipError, match="lens must"):
            ops.si_sdr(x, y, lens=bad)
    # (B, 1, T) and rows of another pitch and alignment: the same bits
    assert same_bits(ops.stoi_scores(x.unsqueeze(1), y.unsqueeze(1), 10000, lens), got)
    wide_x, wide_y = torch.zeros(7, 6003, device=cuda), torch.zeros(7, 6005, device=cuda)
    wide_x[:, 1:6001], wide_y[:, 3:6003] = x, y
    assert same_bits(ops.stoi_scores(wide_x[:, 1:6001], wide_y[:, 3:6003], 10000, lens), got)
    # every row alone scores the bits it scores in the batch
    for b, n in enumerate(ragged["lens"]):
        alone = ops.stoi_scores(x[b:b + 1, :n].contiguous(), y[b:b + 1, :n].contiguous(), 10000)
        assert all(torch.equal(_bits(u[0]), _bits(v[b])) for u, v in zip(alone[:5], got[:5])), b
        assert torch.equal(alone.kept_idx[0, :int(alone.n_kept[0])], got.kept_idx[b, :int(got.n_kept[b])])


def _tile_sizes():
    from facodec_amd import ops
    geo = ops.stoi_geometry(10000)
    return sorted({geo.energy_frames, geo.scan_block, geo.band_frames, geo.score_segments})


@pytest.mark.parametrize("which", range(2))
def test_stoi_on_tile_boundaries(cuda, which):
    """Rows of G - 1, G, G + 1 and 2 G + 1 frames for every tile constant G of the launches (frames per workgroup of the energy and
    band kernels, frames per scan block, segments per workgroup of the score kernel), and a row of 2 G + 1 frames with a silent
    stretch that drops frames G - 3 .. G + 1: the carried offset of the scan, the neighbours of a rebuilt frame and a segment's 30
    columns all cross a boundary there."""
    from facodec_amd import ops
    sizes = _tile_sizes()
    assert sizes == [32, 256]
    G = sizes[which]
    xs = [noise_row(128 * (m - 1) + 256, 100 * G + m) for m in (G - 1, G, G + 1, 2 * G + 1)]
    hole = noise_row(128 * 2 * G + 256, 100 * G + 7).copy()
    hole[128 * (G - 3):128 * (G + 3)] *= 1e-4
    xs.append(hole)
    ys = [at_snr(x, 5.0, 200 * G + i) for i, x in enumerate(xs)]
    lens = torch.tensor([len(x) for x in xs], dtype=torch.int32, device=cuda)
    got = ops.stoi_scores(torch.from_numpy(_padded(xs)).to(cuda), torch.from_numpy(_padded(ys)).to(cuda), 10000, lens)
    check_stoi(got, xs, ys, f"G = {G}")
    assert got.n_kept.cpu().tolist() == [G - 1, G, G + 1, 2 * G + 1, 2 * G + 1 - 5]
    kept = got.kept_idx[4].cpu().tolist()
    assert kept[G - 4:G - 2] == [G - 4, G + 2]


def test_stoi_at_24_khz(cuda):
    """Another rate is ops.resample to 10 kHz with the rows' lengths, then the 10 kHz path: bit for bit, and within the bound of the
    reference fed the resampled rows."""
    from facodec_amd import ops
    n24 = [48000, 30001, 12345]
    g = np.random.default_rng(24)
    xs = [(0.1 * g.standard_normal(n) * (1.0 + 0.8 * np.sin(2.0 * np.pi * 3.0 * np.arange(n) / 24000.0))).astype(np.float32) for n in n24]
    ys = [at_snr(x, snr, 240 + i) for i, (x, snr) in enumerate(zip(xs, (10.0, 0.0, 20.0)))]
    x24, y24 = torch.from_numpy(_padded(xs)).to(cuda), torch.from_numpy(_padded(ys)).to(cuda)
    lens = torch.tensor(n24, dtype=torch.int32, device=cuda)
    got = ops.stoi_scores(x24, y24, 24000, lens)
    n10 = [-(-n * 5 // 12) for n in n24]
    x10, y10 = ops.resample(x24, 24000, 10000, lens=lens), ops.resample(y24, 24000, 10000, lens=lens)
    assert x10.shape == (3, 20000)
    again = ops.stoi_scores(x10, y10, 10000, torch.tensor(n10, dtype=torch.int32, device=cuda))
    assert same_bits(again, got) and torch.equal(again.kept_idx, got.kept_idx)
    xh, yh = x10.cpu().numpy(), y10.cpu().numpy()
    check_stoi(got, [xh[b, :n] for b, n in enumerate(n10)], [yh[b, :n] for b, n in enumerate(n10)], "24 kHz")
    assert got.n_frames.cpu().tolist() == [(n - 256) // 128 + 1 for n in n10]


# ---------------------------------------------------------------------------------------------------------------- SI-SDR
def test_si_sdr_of_a_ragged_batch(cuda):
    """About 40, 5 and -5 dB on rows of one chunk - 1, one chunk, one chunk + 1 and three chunks + 1 samples, a row of one sample,
    identical rows (+inf), an empty row (NaN) and a zero reference (-80)."""
    from facodec_amd import ops
    C = ops.si_sdr_chunk()
    assert C == 4096
    xs = [noise_row(3 * C + 1, 31), noise_row(C - 1, 32), noise_row(C, 33), noise_row(C + 1, 34), noise_row(1, 35), noise_row(5000, 36),
          np.zeros(0, dtype=np.float32), np.zeros(5000, dtype=np.float32)]
    ys = [at_snr(xs[0], 40.0, 41), at_snr(xs[1], 5.0, 42), at_snr(xs[2], -5.0, 43), at_snr(xs[3], 40.0, 44), noise_row(1, 45), xs[5],
          np.zeros(0, dtype=np.float32), noise_row(5000, 47)]
    ref = [si_sdr_ref(x, y) for x, y in zip(xs, ys)]
    assert abs(ref[0] - 40.0) < 0.5 and abs(ref[1] - 5.0) < 0.5 and abs(ref[2] + 5.0) < 0.5
    assert math.isnan(ref[4]) and ref[5] == float("inf") and math.isnan(ref[6]) and abs(ref[7] + 80.0) < 1e-9
    x, y = torch.from_numpy(_padded(xs)).to(cuda), torch.from_numpy(_padded(ys)).to(cuda)
    lens = torch.tensor([len(r) for r in xs], dtype=torch.int32, device=cuda)
    got = ops.si_sdr(x, y, lens=lens)
    assert got.dtype == torch.float64 and got.shape == (8,)
    out = got.cpu().tolist()
    worst = 0.0
    for b, (g, r) in enumerate(zip(out, ref)):
        if math.isnan(r) or math.isinf(r):
            assert (math.isnan(g) and math.isnan(r)) or g == r, (b, g, r)
        else:
            worst = max(worst, abs(g - r))
            assert abs(g - r) <= SDR_TOL, (b, g, r)
    print(f"SI-SDR: max |got - ref| = {worst:.3e} dB")
    assert torch.equal(_bits(ops.si_sdr(x.unsqueeze(1), y.unsqueeze(1), lens=lens)), _bits(got))
    wide = torch.zeros(8, x.shape[1] + 3, device=cuda)
    wide[:, 1:-2] = x
    assert torch.equal(_bits(ops.si_sdr(wide[:, 1:-2], y, lens=lens)), _bits(got))
    for b, r in enumerate(xs):
        if len(r):
            alone = ops.si_sdr(x[b:b + 1, :len(r)].contiguous(), y[b:b + 1, :len(r)].contiguous())
            assert torch.equal(_bits(alone), _bits(got[b:b + 1])), b
    assert math.isnan(float(ops.si_sdr(x[:1, :0], y[:1, :0])[0]))


# ---------------------------------------------------------------------------------------------------------------- clip lists
@pytest.fixture(scope="module")
def full_model(cuda):
    from facodec_amd.commons import build_model, default_model_params
    model = build_model(default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(cuda)
    return model


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def test_score_clips_and_evaluate_clips(full_model, cuda):
    """Five clips of different lengths through the codec with synthetic weights, grouped three and two: every dict is what the
    single-clip ops calls give on that pair, in the caller's order."""
    from facodec_amd import commons, ops
    lengths = [12000, 9000, 7500, 15100, 10250]
    waves = [(0.3 * synth.synth_clips(1, n, seed=60 + i)).to(cuda).reshape(-1) for i, n in enumerate(lengths)]
    waves[1] = waves[1].reshape(1, -1)
    scores, outs = commons.evaluate_clips(full_model, waves, max_batch_samples=3 * 12000)
    assert len(scores) == 5 and [o.shape[-1] for o in outs] == [300 * (n // 300) for n in lengths]
    for i, (w, o, sc) in enumerate(zip(waves, outs, scores)):
        n = min(w.shape[-1], o.shape[-1])
        r, e = w.reshape(1, -1)[:, :n].contiguous(), o.reshape(1, -1)[:, :n].contiguous()
        s = ops.stoi_scores(r, e, 24000)
        want = dict(si_sdr=float(ops.si_sdr(r, e)[0]), stoi=float(s.stoi[0]), estoi=float(s.estoi[0]))
        print(i, sc)
        assert list(sc) == ["si_sdr", "stoi", "estoi"] and all(_same(sc[k], want[k]) for k in want), (i, sc, want)
        # 9000 and 7500 samples are 28 and 23 frames at 10 kHz: no segment; the others have 32 frames and more
        assert math.isnan(sc["stoi"]) == (i in (1, 2)) and math.isnan(sc["estoi"]) == (i in (1, 2)) and not math.isnan(sc["si_sdr"])
    only = commons.score_clips(waves, outs, metrics=("estoi",))
    assert [list(d) for d in only] == [["estoi"]] * 5 and all(_same(d["estoi"], sc["estoi"]) for d, sc in zip(only, scores))
    assert commons.score_clips([], []) == []
    with pytest.raises(ValueError, match="5 references but 4 estimates"):
        commons.score_clips(waves, outs[:4])
    with pytest.raises(Exception, match="no CPU path"):
        commons.score_clips([w.cpu() for w in waves], outs)
