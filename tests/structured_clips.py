"""Structured test signals on the 16-bit PCM grid (DESIGN.md "Structured signals"): what the Gaussian clips of
facodec_amd/synth.py leave out -- digital silence and dither, hard clipping, chirps, amplitude-modulated noise, harmonic "voiced"
clips with real pauses, impulse trains, DC and steps, and mixtures of those.

    names, wave = structured_clips(48000)          # 32 names, (32, 1, 48000) fp32: eight families of four clips
    wave = voiced_clip(47999)                      # (1, 1, 47999): the voiced generator at any length
    pcm_sha256(wave)                               # sha256 of the int16 samples: what the fixtures store and every test asserts

Every clip is computed in float64 numpy and rounded to the PCM grid, clip(rint(x * 32768), -32768, 32767) / 32768: real inputs are
PCM, every grid value is exact in fp32, and the rounding absorbs last-ulp differences of sin / exp between hosts (a sample within
1e-9 LSB of a rounding tie is an error here, so a generator cannot sit on one).  Random parts come from a seeded torch.Generator on
the CPU.  Shared by tests/golden/make_golden_bench.py (which feeds the clips to the real reference) and by the tests; it imports
neither the reference nor the oracle."""
import hashlib

import numpy as np
import torch

SR = 24000
FULL_SCALE = 32767.0 / 32768.0
FAMILIES = ("silence", "clipped_sine", "chirp", "am_noise", "voiced", "impulses", "dc_steps", "mixture")
PROBE_CLIPS = (0, 5, 9, 13, 17, 21, 25, 29)          # one clip of every family
STREAMING_CLIPS = (1, 17, 4, 20)                     # silence-dither, voiced with pauses, clipped sine, impulse train


def _pcm(x):
    """float64 samples -> float64 samples on the 16-bit grid (exact in fp32)."""
    s = np.asarray(x, np.float64) * 32768.0
    frac = np.abs(s - np.floor(s) - 0.5)
    inside = np.abs(s) < 32767.0                      # clipped samples do not round
    if inside.any() and float(frac[inside].min()) < 1e-9:
        raise ValueError("a sample sits on a rounding tie of the PCM grid: change the generator's constants")
    return np.clip(np.rint(s), -32768, 32767) / 32768.0


def _randn(n, seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    return torch.randn(int(n), generator=g, dtype=torch.float64).numpy()


def _rand(n, seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    return torch.rand(int(n), generator=g, dtype=torch.float64).numpy()


def _t(n):
    return np.arange(n, dtype=np.float64) / SR


def _db(level):
    return 10.0 ** (level / 20.0)


# ------------------------------------------------------------------------------------------------------------------ the families
def _tpdf_dither(n, seed):
    """Triangular dither of +-1 LSB peak: the grid values -1, 0, +1 LSB with probabilities 1/8, 3/4, 1/8."""
    return (_rand(n, seed) - _rand(n, seed + 1000)) / 32768.0


def _clipped_sine(n, freq, phase):
    """Gain 2 into a hard clipper at full scale: two thirds of the samples sit at +-32767/32768."""
    return np.clip(2.0 * np.sin(2 * np.pi * freq * _t(n) + phase), -FULL_SCALE, FULL_SCALE)


def _chirp(n, f0, f1, log, amp):
    t, dur = _t(n), n / SR
    if log:
        k = np.log(f1 / f0) / dur
        phase = 2 * np.pi * f0 * (np.exp(k * t) - 1.0) / k
    else:
        phase = 2 * np.pi * (f0 * t + 0.5 * (f1 - f0) / dur * t * t)
    return amp * np.sin(phase + 0.3)


def _am_noise(n, level_db, rate, seed):
    """Gaussian noise of `level_db` dBFS rms under a raised-sine envelope of `rate` Hz."""
    env = 0.5 * (1.0 + np.sin(2 * np.pi * rate * _t(n) + 0.7))
    return _db(level_db) * env * _randn(n, seed)


def _voiced(n, f_lo=90.0, f_hi=260.0, glide_hz=0.45, syl_hz=3.7, amp=0.6, pauses=((0.0, 0.06), (0.46, 0.55), (0.93, 1.0))):
    """30 harmonics at 1 / k of an f0 gliding between f_lo and f_hi (80 - 300 Hz), under a syllabic envelope; `pauses` are
    fractions of the clip that are exact zeros (start, middle, end)."""
    t = _t(n)
    f0 = f_lo + (f_hi - f_lo) * 0.5 * (1.0 - np.cos(2 * np.pi * glide_hz * t + 0.4))
    ph = 2 * np.pi * np.cumsum(f0) / SR
    x = np.zeros(n)
    for k in range(1, 31):
        x += np.sin(k * ph + 0.37 * k) / k
    env = 0.15 + 0.85 * (0.5 * (1.0 - np.cos(2 * np.pi * syl_hz * t))) ** 1.5
    x = x * env
    x = amp * x / max(float(np.abs(x).max()), 1e-30)
    for lo, hi in pauses:
        x[int(round(lo * n)):int(round(hi * n))] = 0.0
    return x


def _impulses(n, period, amp, alternate=False):
    x = np.zeros(n)
    idx = np.arange(period // 3, n, period)
    x[idx] = amp * (np.where(np.arange(len(idx)) % 2 == 0, 1.0, -1.0) if alternate else 1.0)
    return x


def _single_click(n, amp):
    x = np.zeros(n)
    x[(n * 5) // 9] = amp
    return x


def _gaussian(n, level_db, seed):
    """synth.synth_clips' family (N(0, 1), peak-normalised), scaled to a peak of `level_db` dBFS."""
    w = _randn(n, seed)
    return _db(level_db) * w / np.abs(w).max()


def _family_clips(n):
    t = _t(n)
    half, sixty = n // 2, (n * 3) // 5
    step = np.where(np.arange(n) < half, 0.3, -0.3)
    into_silence = np.where(np.arange(n) < sixty, 0.4, 0.0)
    v_a = dict(f_lo=85.0, f_hi=210.0, glide_hz=0.45, syl_hz=3.7, amp=0.6)
    v_b = dict(f_lo=120.0, f_hi=295.0, glide_hz=0.8, syl_hz=4.6, amp=0.45)
    v_c = dict(f_lo=80.0, f_hi=150.0, glide_hz=0.3, syl_hz=2.9, amp=0.8)
    v_d = dict(f_lo=180.0, f_hi=300.0, glide_hz=1.1, syl_hz=5.3, amp=0.25)
    voiced_half = _voiced(n, **v_b)
    voiced_half[half:] = 0.0
    return [
        ("silence/zeros", np.zeros(n)),
        ("silence/tpdf_1", _tpdf_dither(n, 101)),
        ("silence/tpdf_2", _tpdf_dither(n, 102)),
        ("silence/tpdf_3", _tpdf_dither(n, 103)),
        ("clipped_sine/110Hz", _clipped_sine(n, 110.0, 0.1)),
        ("clipped_sine/440Hz", _clipped_sine(n, 440.0, 0.2)),
        ("clipped_sine/3000Hz", _clipped_sine(n, 3000.0, 0.3)),
        ("clipped_sine/11900Hz", _clipped_sine(n, 11900.0, 0.4)),
        ("chirp/linear_up", _chirp(n, 50.0, 11000.0, False, 0.7)),
        ("chirp/linear_down", _chirp(n, 11000.0, 50.0, False, 0.5)),
        ("chirp/log_up", _chirp(n, 50.0, 11000.0, True, 0.6)),
        ("chirp/log_down", _chirp(n, 11000.0, 50.0, True, 0.35)),
        ("am_noise/-20dB_3Hz", _am_noise(n, -20.0, 3.0, 201)),
        ("am_noise/-40dB_5Hz", _am_noise(n, -40.0, 5.0, 202)),
        ("am_noise/-20dB_6.5Hz", _am_noise(n, -20.0, 6.5, 203)),
        ("am_noise/-40dB_8Hz", _am_noise(n, -40.0, 8.0, 204)),
        ("voiced/a", _voiced(n, **v_a)),
        ("voiced/b", _voiced(n, **v_b)),
        ("voiced/c", _voiced(n, **v_c)),
        ("voiced/d", _voiced(n, **v_d)),
        ("impulses/period_96", _impulses(n, 96, 0.9)),
        ("impulses/period_150", _impulses(n, 150, 0.5, alternate=True)),
        ("impulses/period_240", _impulses(n, 240, -0.7)),
        ("impulses/single_click", _single_click(n, 0.8)),
        ("dc_steps/offset", np.full(n, 0.25)),
        ("dc_steps/step", step),
        ("dc_steps/ramp", -0.4991 + 0.9987 * t / (n / SR)),
        ("dc_steps/step_into_silence", into_silence),
        ("mixture/voiced_over_noise_floor", _voiced(n, **v_a) + _db(-50.0) * _randn(n, 301)),
        ("mixture/clipped_voiced", np.clip(3.0 * _voiced(n, **v_c), -FULL_SCALE, FULL_SCALE)),
        ("mixture/voiced_then_silence", voiced_half),
        ("mixture/gaussian_-60dB", _gaussian(n, -60.0, 302)),
    ]


def structured_clips(n_samples=48000):
    """-> (names [32], wave (32, 1, n_samples) fp32 on the PCM grid): FAMILIES[i // 4] is clip i's family."""
    clips = _family_clips(int(n_samples))
    assert len(clips) == 4 * len(FAMILIES) and all(name.split("/")[0] == FAMILIES[i // 4] for i, (name, _) in enumerate(clips))
    wave = np.stack([_pcm(x) for _, x in clips]).astype(np.float32)
    return [name for name, _ in clips], torch.from_numpy(wave).unsqueeze(1)


def voiced_clip(n_samples):
    """(1, 1, n_samples) fp32: the voiced generator (pauses at the start, in the middle and at the end) at any length."""
    return torch.from_numpy(_pcm(_voiced(int(n_samples))).astype(np.float32)).reshape(1, 1, -1)


def to_int16(wave):
    a = torch.as_tensor(wave).detach().cpu().double().numpy() * 32768.0
    assert np.array_equal(a, np.rint(a)) and a.min() >= -32768 and a.max() <= 32767, "not on the 16-bit PCM grid"
    return a.astype(np.int16)


def pcm_sha256(wave):
    """sha256 of the clips' int16 samples (C order)."""
    return hashlib.sha256(np.ascontiguousarray(to_int16(wave)).tobytes()).hexdigest()


sha256 = pcm_sha256
