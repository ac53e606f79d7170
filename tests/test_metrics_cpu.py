"""Objective scores without a GPU: the float64 numpy restatement of SI-SDR, STOI and ESTOI that both metrics
test files measure against, pinned by what it must do on its own -- the band table from its formula, a score of 1 for identical
signals, scores that fall with the SNR, and the sensitivity of the score to three plausible mistakes, which is what the bound of
the GPU tests rests on -- and the host side of the C entries: fac_stoi_geometry and the argument checks.

Nothing of the package enters the reference.  It restates the definition in the header comment of include/facodec_hip.h."""
import ctypes
import math

import numpy as np
import pytest

from facodec_amd import _lib

FS, FRAME, HOP, NFFT, NBANDS, MINFREQ, NSEG, BETA, DYN = 10000, 256, 128, 512, 15, 150.0, 30, -15.0, 40.0
EPS = 2.220446049250313e-16
BANDS = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
         (109, 138), (138, 174), (174, 219))
WINDOW = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(1, FRAME + 1) / (FRAME + 1))


# ---------------------------------------------------------------------------------------------------------------- the reference
def si_sdr_ref(x, y, eps=1e-8):
    """dac/nn/loss.py:91-130 with scaling and zero_mean, sign flipped, in float64; whatever IEEE gives (inf, NaN) is the answer."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = x - (np.sum(x) / len(x) if len(x) else np.float64("nan"))
        e = y - (np.sum(y) / len(y) if len(y) else np.float64("nan"))
        a = (np.sum(e * r) + eps) / (np.sum(r * r) + eps)
        s = a * r
        n = e - s
        return float(10.0 * np.log10(np.float64(np.sum(s * s)) / np.float64(np.sum(n * n)) + eps))


def band_table():
    """(lo, hi) per band: the bins nearest the lower and upper edge of the third-octave band on the grid k FS / NFFT."""
    f = np.arange(NFFT // 2 + 1) * (FS / NFFT)
    centre = MINFREQ * 2.0 ** (np.arange(NBANDS) / 3.0)
    return tuple((int(np.argmin((f - c * 2.0 ** (-1.0 / 6.0)) ** 2)), int(np.argmin((f - c * 2.0 ** (1.0 / 6.0)) ** 2))) for c in centre)


def windowed_frames(x):
    """(M, 256) float64: f_m = w . x[128 m : 128 m + 256]."""
    x = np.asarray(x, dtype=np.float64)
    M = (len(x) - FRAME) // HOP + 1 if len(x) >= FRAME else 0
    if M == 0:
        return np.zeros((0, FRAME))
    return WINDOW * x[HOP * np.arange(M)[:, None] + np.arange(FRAME)[None, :]]


def overlap_add(frames):
    out = np.zeros(HOP * (len(frames) - 1) + FRAME)
    for j, f in enumerate(frames):
        out[HOP * j:HOP * j + FRAME] += f
    return out


def third_octaves(sig, bands):
    """(15, K) float64 band magnitudes of the compacted signal."""
    power = np.abs(np.fft.rfft(windowed_frames(sig), n=NFFT, axis=1)) ** 2               # (K, 257)
    return np.stack([np.sqrt(np.sum(power[:, lo:hi], axis=1)) for lo, hi in bands])


def _unit(v, axis):
    v = v - np.mean(v, axis=axis, keepdims=True)
    return v / (np.sqrt(np.sum(v * v, axis=axis, keepdims=True)) + EPS)


def stoi_ref(x, y, bands=BANDS, beta=BETA, first_segment=0):
    """-> (stoi, estoi, kept frame indices, keep margin in dB).  x, y: one row each at 10 kHz, the same length.  The margin is
    min_m |max E - 40 - E_m| (inf without a frame): how far the nearest frame is from changing sides of the keep decision.
    bands / beta / first_segment exist for the mutation tests below."""
    fx, fy = windowed_frames(x), windowed_frames(y)
    if len(fx) == 0:
        return float("nan"), float("nan"), np.zeros(0, dtype=np.int64), float("inf")
    E = 20.0 * np.log10(np.sqrt(np.sum(fx * fx, axis=1)) + EPS)
    gap = np.max(E) - DYN - E
    kept = np.nonzero(gap < 0)[0]
    margin = float(np.min(np.abs(gap)))
    K = len(kept)
    if K - first_segment < NSEG:
        return float("nan"), float("nan"), kept, margin
    tx, ty = third_octaves(overlap_add(fx[kept]), bands), third_octaves(overlap_add(fy[kept]), bands)
    clip = 1.0 + 10.0 ** (-beta / 20.0)
    c, d = [], []
    for s in range(first_segment, K - NSEG + 1):
        X, Y = tx[:, s:s + NSEG], ty[:, s:s + NSEG]
        alpha = np.sqrt(np.sum(X * X, axis=1, keepdims=True)) / (np.sqrt(np.sum(Y * Y, axis=1, keepdims=True)) + EPS)
        Yp = np.minimum(alpha * Y, X * clip)
        c.append(np.sum(_unit(X, 1) * _unit(Yp, 1), axis=1))
        d.append(np.sum(_unit(_unit(X, 1), 0) * _unit(_unit(Y, 1), 0)) / NSEG)
    return float(np.mean(np.array(c))), float(np.mean(np.array(d))), kept, margin


# ---------------------------------------------------------------------------------------------------------------- test signals
def noise_row(n, seed, amp=0.1):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def gap_row(seed=2011, n=6000, lo=2500, hi=3500):
    """Noise under a 4 Hz modulation with a stretch at -80 dB: frames 20 .. 25 lie inside the stretch and are dropped, so the kept
    frames are not adjacent in the signal."""
    g = np.random.default_rng(seed)
    x = 0.1 * g.standard_normal(n) * (1.0 + 0.8 * np.sin(2.0 * np.pi * 4.0 * np.arange(n) / FS))
    x[lo:hi] *= 1e-4
    return x.astype(np.float32)


def at_snr(x, snr_db, seed):
    """x plus white noise at snr_db below it, float32."""
    x64 = np.asarray(x, dtype=np.float64)
    n = np.random.default_rng(seed).standard_normal(len(x))
    n *= math.sqrt(np.sum(x64 * x64) / np.sum(n * n)) * 10.0 ** (-snr_db / 20.0)
    return (x64 + n).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- pins
def test_band_table_is_the_formula():
    assert band_table() == BANDS
    assert all(BANDS[j][1] == BANDS[j + 1][0] for j in range(NBANDS - 1))
    assert abs(WINDOW[127] - WINDOW[128]) < 1e-15 and WINDOW[0] > 0.0 and abs(WINDOW[0] - WINDOW[255]) < 1e-15


def test_identical_signals_score_one():
    x = gap_row()
    s, e, kept, margin = stoi_ref(x, x)
    assert abs(s - 1.0) <= 1e-12 and abs(e - 1.0) <= 1e-12
    assert len(kept) == 39 and list(kept[18:22]) == [18, 19, 26, 27] and margin >= 1e-3
    assert si_sdr_ref(x, x) == float("inf")


def test_scores_fall_with_the_snr():
    x = gap_row()
    got = [stoi_ref(x, at_snr(x, snr, 7))[:2] for snr in (20.0, 5.0, 0.0, -5.0)]
    print("STOI / ESTOI at 20, 5, 0, -5 dB:", ["%.3f / %.3f" % g for g in got])
    for k in range(3):
        assert got[k][0] > got[k + 1][0] and got[k][1] > got[k + 1][1]
    assert got[0][0] > 0.9 and got[3][0] < 0.7
    sd = [si_sdr_ref(x, at_snr(x, snr, 7)) for snr in (40.0, 5.0, -5.0)]
    assert all(abs(v - snr) < 0.5 for v, snr in zip(sd, (40.0, 5.0, -5.0))), sd


def test_short_and_silent_rows():
    assert len(windowed_frames(np.zeros(255))) == 0 and len(windowed_frames(np.zeros(256))) == 1
    s, e, kept, _ = stoi_ref(noise_row(200, 1), noise_row(200, 2))
    assert math.isnan(s) and math.isnan(e) and len(kept) == 0
    s, e, kept, _ = stoi_ref(noise_row(3840, 1), noise_row(3840, 2))                       # 29 frames: one short of a segment
    assert math.isnan(s) and len(kept) == 29
    s, e, kept, margin = stoi_ref(np.zeros(3968, dtype=np.float32), noise_row(3968, 2))    # a silent reference keeps every frame
    assert (s, e) == (0.0, 0.0) and len(kept) == 30 and margin == 40.0
    assert math.isnan(si_sdr_ref(np.zeros(0), np.zeros(0))) and math.isnan(si_sdr_ref(np.zeros(8), np.zeros(8)))
    assert abs(si_sdr_ref(np.zeros(100), noise_row(100, 3)) + 80.0) < 1e-9


def test_mutations_move_the_score_far_beyond_the_gpu_bound():
    """What the 1e-6 cap of tests/test_metrics.py can tell apart: one band edge off by a bin, segments that start a frame late
    and a clipping level of -14 instead of -15 dB each move STOI by at least a hundred times that."""
    x = gap_row()
    y = at_snr(x, 0.0, 7)
    base = stoi_ref(x, y)[0]
    for j, (lo, hi) in ((3, (14, 18)), (9, (56, 69))):
        bands = list(BANDS)
        bands[j] = (lo, hi)
        moved = abs(stoi_ref(x, y, bands=tuple(bands))[0] - base)
        print(f"band {j} as {lo, hi}: STOI moves by {moved:.2e}")
        assert moved >= 1e-3
    late = abs(stoi_ref(x, y, first_segment=1)[0] - base)
    beta = abs(stoi_ref(x, y, beta=-14.0)[0] - base)
    print(f"segments one frame late: {late:.2e}; BETA = -14: {beta:.2e}")
    assert late >= 1e-4 and beta >= 1e-5


# ---------------------------------------------------------------------------------------------------------------- the C entries
def _geometry(T):
    out = (ctypes.c_int64 * 6)()
    rc = _lib.load().fac_stoi_geometry(T, out)
    return rc, list(out)


def test_geometry_on_the_host():
    rc, (m_max, row_bytes, g_energy, g_scan, g_bands, g_score) = _geometry(20000)
    assert rc == 0 and m_max == (20000 - 256) // 128 + 1 == 155
    assert row_bytes == 8 * (m_max + 2 * NBANDS * m_max + 2 * (m_max - 29))
    assert all(g >= 1 for g in (g_energy, g_scan, g_bands, g_score))
    assert _geometry(255)[1][:2] == [0, 0] and _geometry(256)[1][0] == 1 and _geometry(0)[0] == 0
    assert _geometry(3968)[1][0] == 30 and _geometry(3968)[1][1] == 8 * (31 * 30 + 2)
    lib = _lib.load()
    assert _geometry(-1)[0] == -1 and b"T = -1" in lib.fac_last_error()
    assert _geometry((1 << 28) + 1)[0] == -1
    assert lib.fac_stoi_geometry(100, None) == -1 and b"null" in lib.fac_last_error()
    from facodec_amd import ops
    geo = ops.stoi_geometry(20000)
    assert (geo.n_frames, geo.ws_bytes_per_row, geo.energy_frames, geo.scan_block, geo.band_frames, geo.score_segments) == \
        (m_max, row_bytes, g_energy, g_scan, g_bands, g_score)


def _stoi_desc(**kw):
    d = _lib.StoiDesc()
    fake = 0x10000                                   # never dereferenced: every case below is refused before a launch
    for name in ("x", "y", "kept_idx", "n_frames", "n_kept", "n_segments", "stoi", "estoi", "ws"):
        setattr(d, name, fake)
    d.x_bs, d.y_bs, d.B, d.T = 4000, 4000, 2, 4000
    d.ws_bytes = 2 * _geometry(4000)[1][1]
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_c_entries_refuse_bad_arguments_without_a_gpu():
    """Error code and message before any launch.  Whether a pointer is device memory and whether lens is int32 is not visible
    through a C pointer: the Python surface refuses CPU tensors and other dtypes (below)."""
    lib = _lib.load()
    short = 2 * _geometry(4000)[1][1] - 8
    for fn in (lib.fac_stoi_select, lib.fac_stoi_bands, lib.fac_stoi_score):
        assert fn(None, None) == -1 and b"null descriptor" in lib.fac_last_error()
        for kw, msg in ((dict(x=None), b"null pointer"), (dict(y=None), b"null pointer"), (dict(ws=None), b"null pointer"),
                        (dict(kept_idx=None), b"null pointer"), (dict(n_kept=None), b"null pointer"), (dict(stoi=None), b"null pointer"),
                        (dict(B=0), b"B = 0"), (dict(B=70000), b"B = 70000"), (dict(T=-1), b"T = -1"), (dict(T=(1 << 28) + 1), b"T = "),
                        (dict(ws_bytes=short), b"workspace"), (dict(ws_bytes=0), b"workspace"), (dict(ws=0x10004), b"8-byte aligned")):
            assert fn(ctypes.byref(_stoi_desc(**kw)), None) == -1, kw
            assert msg in lib.fac_last_error(), (kw, lib.fac_last_error())
    P = ctypes.c_void_p
    fake = P(0x10000)
    need = lib.fac_si_sdr_ws_bytes(2, 10000)
    chunk = 4096
    assert need == 8 * 2 * (6 * -(-10000 // chunk) + 4) and lib.fac_si_sdr_ws_bytes(0, 10) == -1 and lib.fac_si_sdr_ws_bytes(1, -1) == -1

    def si(x=fake, y=fake, out=fake, ws=fake, ws_bytes=need, B=2, T=10000):
        return lib.fac_si_sdr(x, 10000, y, 10000, None, out, ws, ws_bytes, B, T, None)

    for kw, msg in ((dict(x=None), b"null pointer"), (dict(y=None), b"null pointer"), (dict(out=None), b"null pointer"),
                    (dict(ws=None), b"null pointer"), (dict(B=0), b"B = 0"), (dict(T=-1), b"T = -1"), (dict(ws_bytes=need - 8), b"workspace"),
                    (dict(ws=P(0x10004)), b"8-byte aligned")):
        assert si(**kw) == -1, kw
        assert msg in lib.fac_last_error(), (kw, lib.fac_last_error())


def test_python_surface_refuses_cpu_tensors_and_other_dtypes():
    import torch
    from facodec_amd import commons, ops
    x = torch.zeros(2, 4000)
    for call in (lambda: ops.si_sdr(x, x), lambda: ops.stoi(x, x, 10000), lambda: ops.stoi_scores(x, x, 10000),
                 lambda: commons.score_clips([x[0]], [x[0]])):
        with pytest.raises(_lib.FacodecHipError, match="no CPU path"):
            call()
    with pytest.raises(ValueError, match="same shape"):
        ops.stoi_scores(x, x[:, :100], 10000)
    with pytest.raises(ValueError, match="1 references but 2 estimates"):
        commons.score_clips([x[0]], [x[0], x[1]])
    with pytest.raises(ValueError, match="unknown metric"):
        commons.score_clips([x[0]], [x[0]], metrics=("pesq",))


def test_desc_layout_matches_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "facodec_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", '
                   "sizeof(fac_stoi_desc), offsetof(fac_stoi_desc, stoi), offsetof(fac_stoi_desc, x_bs), offsetof(fac_stoi_desc, ws_bytes), "
                   "offsetof(fac_stoi_desc, T));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(repo, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    k = _lib.StoiDesc
    assert [int(v) for v in out] == [ctypes.sizeof(k), k.stoi.offset, k.x_bs.offset, k.ws_bytes.offset, k.T.offset]
