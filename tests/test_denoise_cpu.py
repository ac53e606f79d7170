"""Noise suppression without a GPU: an fp64 numpy restatement of the definition in include/facodec_hip.h (the
transform is np.fft: the definition's values, not the kernel's roundings), the properties the definition promises, the bounds
of the issue on a synthetic harmonic signal in white noise, and the refusals of the C entries and of the Python surface.
tests/test_denoise.py holds the kernels to this restatement on the GPU."""
import ctypes
import math

import numpy as np
import pytest

from facodec_amd import _lib
from test_metrics_cpu import si_sdr_ref

N, H, BINS, DELAY = 512, 256, 257, 512
WIN = np.sin(np.pi * np.arange(N) / N)


def n_frames(n):
    return -(-n // H) + 1 if n > 0 else 0


def g_min_of(max_atten_db):
    return 10.0 ** (-float(max_atten_db) / 20.0)


def _rfft_rows(fr):
    return np.stack([np.fft.rfft(r) for r in fr]) if len(fr) else np.zeros((0, BINS), dtype=np.complex128)


def _irfft_rows(Y):
    return np.stack([np.fft.irfft(r, N) for r in Y]) if len(Y) else np.zeros((0, N))


def spectra_ref(x, start=0, F=None, frames=None):
    """X (F, 257) complex128 of the frames of x (1-D; samples before `start` count as zero): frame f covers (f - 1) H .. (f + 1) H - 1.
    frames: the frame indices wanted (default all F)."""
    x = np.asarray(x, dtype=np.float64).copy()
    x[:start] = 0.0
    F = n_frames(len(x)) if F is None else F
    frames = np.arange(F) if frames is None else np.asarray(frames)
    top = (int(frames.max()) + 2) * H if len(frames) else 0
    pad = np.concatenate([np.zeros(H), x, np.zeros(max(top - len(x), 0))])
    idx = frames[:, None] * H + np.arange(N)[None, :]
    return _rfft_rows(pad[idx] * WIN)


def power_ref(X):
    return X.real * X.real + X.imag * X.imag


def gains_ref(P, M=8, W=96, over=4.0, max_atten_db=15.0, fs=0, f_lo=0, first=0):
    """G of frames f_lo .. first + len(P) - 1 from P, whose row i is frame first + i (only frames >= fs and within M + W - 2 of a
    wanted frame are read)."""
    g_min = g_min_of(max_atten_db)
    F = first + len(P)
    S = {}

    def mean(g):
        if g not in S:
            lo = max(fs, g - M + 1)
            acc = P[lo - first].copy()
            for h in range(lo + 1, g + 1):
                acc = acc + P[h - first]
            S[g] = acc / float(g - lo + 1)
        return S[g]

    G = np.ones((F - f_lo, BINS))
    for f in range(max(f_lo, fs), F):
        lo = max(fs, f - W + 1)
        Nf = mean(lo).copy()
        for g in range(lo + 1, f + 1):
            Nf = np.minimum(Nf, mean(g))
        nz = Nf != 0.0
        with np.errstate(all="ignore"):
            xi = np.maximum(mean(f) / (over * np.where(nz, Nf, 1.0)) - 1.0, 0.0)
            G[f - f_lo] = np.where(nz, np.maximum(xi / (1.0 + xi), g_min), 1.0)
    return G


def frames_out_ref(X, G):
    """v (F, 512): the masked, inverse-transformed, windowed frames."""
    return _irfft_rows(G * X) * WIN


def denoise_ref(x, start=0, M=8, W=96, over=4.0, max_atten_db=15.0, T=None):
    """-> (y (T,) float32, G (F, 257), P (F, 257)) of one row x (its own length; T >= len(x): the batch's width)."""
    x = np.asarray(x)
    T = len(x) if T is None else T
    F = n_frames(T)
    X = spectra_ref(x, start, F)
    P = power_ref(X)
    G = gains_ref(P, M, W, over, max_atten_db, fs=start // H)
    v = frames_out_ref(X, G)
    acc = np.zeros((F + 1) * H)
    for f in range(start // H, F):
        acc[f * H:f * H + H] = acc[f * H:f * H + H] + v[f, :H]          # the older frame's half is already there
        acc[f * H + H:f * H + N] = v[f, H:]
    y = acc[H:H + T].copy()
    y[:start] = 0.0
    y[len(x):] = 0.0
    return y.astype(np.float32), G, P


class StreamRef:
    """The block-in, block-out form: what streaming.NoiseSuppressor does, on the host.  Keeps the samples, P and G of every frame."""

    def __init__(self, **kw):
        self.kw = kw
        self.M, self.W = kw.get("M", 8), kw.get("W", 96)
        self.x = np.zeros(0, dtype=np.float32)
        self.P = np.zeros((0, BINS))
        self.G = np.zeros((0, BINS))

    def _decide(self, upto):
        f0 = len(self.P)
        if upto > f0:
            Pn = power_ref(spectra_ref(self.x, 0, frames=np.arange(f0, upto)))
            self.P = np.concatenate([self.P, Pn])
            first = max(0, f0 - (self.M + self.W - 2))
            self.G = np.concatenate([self.G, gains_ref(self.P[first:], fs=0, f_lo=f0, first=first, **self.kw)])

    def _out(self, m0, n_out):
        s_first, s_last = m0 // H, (m0 + n_out - 1) // H
        fr = np.arange(max(s_first, 0), s_last + 2)
        v = dict(zip(fr.tolist(), frames_out_ref(spectra_ref(self.x, 0, frames=fr), self.G[fr]))) if len(fr) else {}
        y = np.zeros(n_out, dtype=np.float32)
        for i in range(n_out):
            m = m0 + i
            if 0 <= m < len(self.x):
                f = m // H
                y[i] = np.float32(v[f][m - (f - 1) * H] + v[f + 1][m - f * H])
        return y

    def push(self, block):
        n = len(self.x)
        self.x = np.concatenate([self.x, np.asarray(block, dtype=np.float32)])
        self._decide(len(self.x) // H)
        return self._out(n - DELAY, len(block))

    def finish(self):
        self._decide(n_frames(len(self.x)))
        return self._out(len(self.x) - DELAY, DELAY)


def broadband(T, seed, floor=1e-3, bursts=3):
    """Gaussian noise at `floor` plus louder bursts: every bin of every frame holds power far above the rounding of the rest."""
    rng = np.random.default_rng(seed)
    x = floor * rng.standard_normal(T)
    for _ in range(bursts):
        a = int(rng.integers(0, max(T - 1, 1)))
        n = int(rng.integers(1, max(T // 4, 2)))
        x[a:a + n] += 0.2 * rng.standard_normal(len(x[a:a + n]))
    return x.astype(np.float32)


FS = 24000


def synthetic_mix(seed, T=6 * FS):
    """The issue's mix: a frequency-modulated harmonic tone in 4 Hz syllables on 2 s < t < 5 s, white noise 10 dB below it."""
    t = np.arange(T) / FS
    f0 = 120.0 + 20.0 * np.sin(2 * np.pi * 0.7 * t)
    phase = 2 * np.pi * np.cumsum(f0) / FS
    env = np.where((t > 2) & (t < 5), np.clip(np.sin(2 * np.pi * 2 * t), 0, None) ** 2, 0.0)
    s = 0.1 * sum(np.sin(h * phase) / h for h in range(1, 25)) * env
    speech = (t > 2) & (t < 5)
    noise = np.random.default_rng(seed).standard_normal(T) * (np.sqrt(np.mean(s[speech] ** 2)) * 10.0 ** (-10.0 / 20.0))
    return s, (s + noise).astype(np.float32), speech, (t > 1.2) & (t < 1.9)


def mix_figures(x, y, s, speech, quiet):
    """(attenuation of the noise-only stretch in dB, SI-SDR against s before, after)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    att = 10.0 * np.log10(np.sum(x[quiet] ** 2) / np.sum(y[quiet] ** 2))
    return att, si_sdr_ref(s[speech], x[speech]), si_sdr_ref(s[speech], y[speech])


# ---------------------------------------------------------------------------------------- the definition's properties

def test_window_is_power_complementary():
    assert np.abs(WIN[:H] ** 2 + WIN[H:] ** 2 - 1.0).max() <= 1e-15           # a few roundings of 1.1e-16 each


@pytest.mark.parametrize("T", [30000, 2561, 256, 255, 1])
def test_identity_without_attenuation(T):
    """max_atten_db = 0: every gain is 1 and the overlap-add returns x (the issue's bound: 1e-12 of the peak; the session's
    prototype measured 9.7e-17)."""
    x = broadband(T, 3).astype(np.float64)
    F = n_frames(T)
    X = spectra_ref(x, 0, F)
    v = frames_out_ref(X, gains_ref(power_ref(X), max_atten_db=0.0))
    acc = np.zeros((F + 1) * H)
    for f in range(F):
        acc[f * H:f * H + N] += v[f]
    err = np.abs(acc[H:H + T] - x).max() / np.abs(x).max()
    print(f"identity T={T}: {err:.3g} of the peak")
    assert err <= 1e-12
    assert (gains_ref(power_ref(X), max_atten_db=0.0) == 1.0).all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_synthetic_mix_bounds(seed):
    """Defaults on the 10 dB mix: the noise-only stretch falls by at least 12 dB, the SI-SDR over the tone rises by at least 7 dB."""
    s, x, speech, quiet = synthetic_mix(seed)
    y, G, _ = denoise_ref(x)
    att, before, after = mix_figures(x, y, s, speech, quiet)
    print(f"seed {seed}: noise-only attenuation {att:.2f} dB, SI-SDR {before:.2f} -> {after:.2f} dB")
    assert att >= 12.0
    assert after - before >= 7.0
    assert G.min() >= g_min_of(15.0) and G.max() <= 1.0


def test_unit_gain_while_silence_is_in_the_window():
    """Digital silence first: the mean over the silent frames is 0, so is the floor of every window that still holds one of
    them, and those frames pass at G = 1; the first frame whose window has left the silence is suppressed."""
    M, W = 2, 5
    x = np.concatenate([np.zeros(4 * H, dtype=np.float32), broadband(20 * H, 5, bursts=0)])
    _, G, P = denoise_ref(x, M=M, W=W)
    last_silent = 3                                                  # frames 0 .. 3 see only zeros (frame 4 covers 3 H .. 5 H - 1)
    assert (P[:last_silent + 1] == 0.0).all() and (P[last_silent + 1] > 0.0).any()
    assert (G[:last_silent + W] == 1.0).all()
    assert (G[last_silent + W:-2] < 1.0).any()
    assert (G >= g_min_of(15.0)).all() and (G <= 1.0).all()


@pytest.mark.parametrize("MW", [(8, 96), (2, 5)])
def test_a_row_with_a_start_equals_the_shifted_fresh_row(MW):
    M, W = MW
    x = broadband(9000, 7)
    y0, G0, _ = denoise_ref(x, M=M, W=W)
    for start in (H, 10 * H):
        junk = np.full(start, 0.5, dtype=np.float32)                 # what lies before the start counts as zero
        y1, G1, _ = denoise_ref(np.concatenate([junk, x]), start=start, M=M, W=W)
        assert (y1[:start] == 0.0).all() and np.array_equal(y1[start:], y0)
        assert (G1[:start // H] == 1.0).all() and np.array_equal(G1[start // H:], G0)
    y2, _, _ = denoise_ref(np.concatenate([np.full(2400, 0.5, dtype=np.float32), x]), start=2400, M=M, W=W)
    assert (y2[:2400] == 0.0).all() and np.abs(y2[2400:]).max() > 0.0


@pytest.mark.parametrize("MW", [(8, 96), (2, 5)])
def test_chunked_restatement_equals_offline(MW):
    M, W = MW
    T = 9000
    x = broadband(T, 11)
    y, G, _ = denoise_ref(x, M=M, W=W)
    for chunks in ([1, 7, 479, 2400] + [480] * 20, [480] * 19):
        st, out, t = StreamRef(M=M, W=W), [], 0
        for k in chunks:
            k = min(k, T - t)
            if k:
                out.append(st.push(x[t:t + k]))
                t += k
        assert t == T
        out.append(st.finish())
        got = np.concatenate(out)
        assert len(got) == T + DELAY and (got[:DELAY] == 0.0).all()
        assert np.array_equal(got[DELAY:], y)
        assert np.array_equal(st.G, G)


# ---------------------------------------------------------------------------------------- refusals

FAKE = 0x10000                                                       # never dereferenced: every case below is refused before a launch


def _power_desc(**kw):
    d = _lib.NsPowerDesc()
    d.x, d.P = FAKE, FAKE
    d.x_bs, d.p_bs, d.n0, d.f0 = 4800, 20 * BINS, 0, 0
    d.B, d.k, d.n_new, d.R = 2, 4800, 20, 20
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _gains_desc(**kw):
    d = _lib.NsGainsDesc()
    d.P, d.G = FAKE, FAKE
    d.p_bs, d.g_bs, d.f0 = 120 * BINS, 120 * BINS, 0
    d.over, d.g_min = 4.0, g_min_of(15.0)
    d.B, d.n_new, d.R, d.M, d.W = 2, 20, 120, 8, 96
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _synth_desc(**kw):
    d = _lib.NsSynthDesc()
    d.x, d.G, d.y = FAKE, FAKE, FAKE
    d.x_bs, d.g_bs, d.y_bs, d.n0, d.m0 = 4800, 20 * BINS, 4800, 0, 0
    d.B, d.k, d.n_out, d.R = 2, 4800, 4800, 20
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def check_refusals():
    """Error code and message of every refusal the header lists, before any launch (no pointer is dereferenced)."""
    lib = _lib.load()

    def err():
        return lib.fac_last_error()

    assert lib.fac_ns_power(None, None) == -1 and b"null descriptor" in err()
    for kw, msg in ((dict(P=None), b"null power"), (dict(x=None), b"null block pointer"), (dict(B=0), b"B = 0"), (dict(B=65536), b"B = 65536"),
                    (dict(k=-1), b"k = -1"), (dict(n_new=-1), b"n_new = -1"), (dict(n_new=0), b"nothing to do"), (dict(n0=-1), b"n0 = -1"),
                    (dict(f0=-1), b"f0 = -1"), (dict(carry_in=FAKE, carry_out=FAKE), b"carry_out is carry_in"),
                    (dict(lens=FAKE, carry_in=FAKE), b"lens does not go with a carried stream"),
                    (dict(lens=FAKE, carry_out=FAKE), b"lens does not go with a carried stream"),
                    (dict(x_bs=4799), b"x_bs = 4799"), (dict(R=19), b"R = 19"), (dict(R=0, n_new=0, carry_out=FAKE), b"R = 0"),
                    (dict(p_bs=20 * BINS - 1), b"p_bs"), (dict(carry_in=FAKE, n0=2560, f0=6), b"in front of n0")):
        assert lib.fac_ns_power(ctypes.byref(_power_desc(**kw)), None) == -1, kw
        assert msg in err(), (kw, err())

    assert lib.fac_ns_gains(None, None) == -1 and b"null descriptor" in err()
    for kw, msg in ((dict(P=None), b"null power or gain"), (dict(G=None), b"null power or gain"), (dict(B=0), b"B = 0"), (dict(n_new=0), b"n_new = 0"),
                    (dict(M=0), b"M = 0"), (dict(M=_lib.NS_MAX_M + 1), b"M = 65"), (dict(W=0), b"W = 0"), (dict(W=_lib.NS_MAX_W + 1), b"W = 257"),
                    (dict(over=0.0), b"over = 0"), (dict(over=float("inf")), b"over = inf"), (dict(g_min=0.0), b"g_min = 0"),
                    (dict(g_min=1.5), b"g_min = 1.5"), (dict(g_min=float("nan")), b"g_min"), (dict(f0=-1), b"f0 = -1"),
                    (dict(f0=1000, R=121), b"R = 121"), (dict(R=19), b"R = 19"), (dict(p_bs=120 * BINS - 1), b"p_bs"), (dict(g_bs=120 * BINS - 1), b"g_bs")):
        assert lib.fac_ns_gains(ctypes.byref(_gains_desc(**kw)), None) == -1, kw
        assert msg in err(), (kw, err())

    assert lib.fac_ns_synth(None, None) == -1 and b"null descriptor" in err()
    for kw, msg in ((dict(G=None), b"null gain or output"), (dict(y=None), b"null gain or output"), (dict(x=None), b"null block pointer"),
                    (dict(B=0), b"B = 0"), (dict(k=-1), b"k = -1"), (dict(n_out=0), b"n_out = 0"), (dict(n0=-1), b"n0 = -1"),
                    (dict(lens=FAKE, carry_in=FAKE), b"lens does not go with a carried stream"), (dict(x_bs=4799), b"x_bs = 4799"),
                    (dict(y_bs=4799), b"y_bs = 4799"), (dict(R=19), b"R = 19"), (dict(g_bs=20 * BINS - 1), b"g_bs"),
                    (dict(carry_in=FAKE, n0=4800, m0=4800 - 1024, n_out=480), b"in front of n0"),
                    (dict(n0=4800, m0=4800 - 512, n_out=480), b"there is no carry")):
        assert lib.fac_ns_synth(ctypes.byref(_synth_desc(**kw)), None) == -1, kw
        assert msg in err(), (kw, err())


def test_c_entries_refuse_bad_arguments_without_a_gpu():
    check_refusals()


def test_parameter_checks_of_the_python_surface():
    import torch
    from facodec_amd import commons, ops, streaming
    p = ops.ns_params()
    assert (p.M, p.W, p.over) == (8, 96, 4.0) and p.g_min == g_min_of(15.0)
    assert ops.ns_params(max_atten_db=0.0).g_min == 1.0
    for kw in (dict(M=0), dict(M=65), dict(M=2.5), dict(W=0), dict(W=257), dict(over=0.0), dict(over=-1.0), dict(over=float("inf")),
               dict(max_atten_db=-1.0), dict(max_atten_db=float("nan")), dict(max_atten_db=float("inf"))):
        with pytest.raises(ValueError):
            ops.ns_params(**kw)
        with pytest.raises(ValueError):
            commons.denoise_clips([torch.zeros(100)], **kw)
    assert [ops.ns_frames(n) for n in (0, 1, 255, 256, 257, 30000)] == [0, 2, 2, 2, 3, 119]
    assert commons.denoise_clips([]) == []
    with pytest.raises(_lib.FacodecHipError, match="no CPU path"):
        ops.denoise(torch.zeros(1, 4800))
    with pytest.raises(_lib.FacodecHipError, match="no CPU path"):
        commons.denoise_clips([torch.zeros(100)])
    with pytest.raises(ValueError, match="ring"):
        streaming.NoiseSuppressor(1, ring=8 + 96 - 2 + 1, device="cpu")         # M + W - 2 older frames and two of the push's own
    with pytest.raises(ValueError, match="ring"):
        streaming.NoiseSuppressor(1, M=1, W=1, ring=3, device="cpu")
    with pytest.raises(ValueError, match="M = 0"):
        streaming.NoiseSuppressor(1, M=0, device="cpu")
    with pytest.raises(ValueError, match="takes codes"):
        streaming.DenoisedSession(object())
    assert math.isclose(ops.NS_DELAY / 24000, 0.0213, abs_tol=1e-4)


def test_desc_layouts_match_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    structs = {"fac_ns_power_desc": (_lib.NsPowerDesc, ("P", "X", "x_bs", "f0", "B", "R")),
               "fac_ns_gains_desc": (_lib.NsGainsDesc, ("G", "p_bs", "over", "g_min", "B", "W")),
               "fac_ns_synth_desc": (_lib.NsSynthDesc, ("X", "y", "x_bs", "m0", "B", "R"))}
    args = [f"sizeof({s})" for s in structs] + [f"offsetof({s}, {f})" for s, (_, fs) in structs.items() for f in fs]
    consts = ["FAC_NS_N", "FAC_NS_H", "FAC_NS_BINS", "FAC_NS_CARRY", "FAC_NS_MAX_M", "FAC_NS_MAX_W"]
    args += [f"(size_t){c}" for c in consts]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "facodec_hip.h"\nint main(){printf("' + "%zu " * len(args) +
                   '\\n", ' + ", ".join(args) + ");return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(repo, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(c) for c, _ in structs.values()] + [getattr(c, f).offset for c, fs in structs.values() for f in fs]
    want += [_lib.NS_N, _lib.NS_H, _lib.NS_BINS, _lib.NS_CARRY, _lib.NS_MAX_M, _lib.NS_MAX_W]
    assert out == want
