"""Host-side construction (numpy, float64 -> float32) of the constant operands of the spectral
kernels: windows, mel filterbanks and the windowed real-DFT bases that turn an STFT into a GEMM
for the MFMA conv kernel.  These are computed once per module and uploaded; no signal arithmetic
happens here.

Third-party semantics being matched (not vendored in the reference):
  * torchaudio.transforms.MelSpectrogram -> periodic Hann, HTK mel, norm=None, power 2
    (modules/quantize.py:228-230, meldataset.py:37-38, losses.py:75-83);
  * audiotools AudioSignal.stft / mel_spectrogram -> scipy periodic Hann, magnitude,
    librosa Slaney-scale + Slaney-norm filterbank (dac/nn/loss.py:221-227,319-320).
"""
import math

import numpy as np


def hann_periodic(n):
    k = np.arange(n, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * math.pi * k / n)).astype(np.float32)


def mel_fbank_htk(n_freqs, n_mels, sample_rate, f_min=0.0, f_max=None):
    """(n_freqs, n_mels) triangular HTK filterbank.  Built with torch float32 tensor ops in the
    same order torchaudio.functional.melscale_fbanks uses, because construction precision alone
    moves these weights at the 1e-5 level."""
    import torch
    if f_max is None:
        f_max = float(sample_rate // 2)
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_min = 2595.0 * math.log10(1.0 + f_min / 700.0)
    m_max = 2595.0 * math.log10(1.0 + f_max / 700.0)
    m_pts = torch.linspace(m_min, m_max, n_mels + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.clamp(torch.min(down, up), min=0.0).numpy()


def _hz_to_mel_slaney(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz_slaney(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_fbank_slaney(sr, n_fft, n_mels, fmin=0.0, fmax=None):
    """(n_mels, 1 + n_fft//2) Slaney-scale, area-normalised filterbank (librosa.filters.mel defaults)."""
    if fmax is None:
        fmax = sr / 2.0
    fftfreqs = np.fft.rfftfreq(n=n_fft, d=1.0 / sr)
    mel_f = _mel_to_hz_slaney(np.linspace(_hz_to_mel_slaney(fmin), _hz_to_mel_slaney(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    weights = np.zeros((n_mels, 1 + n_fft // 2), dtype=np.float32)
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2: n_mels + 2] - mel_f[:n_mels])
    weights *= enorm[:, np.newaxis]
    return weights


def dft_basis(n_fft, win_length=None, window=None):
    """Windowed one-sided real-DFT basis as a (2F, n_win) float32 matrix, F = n_fft//2 + 1:
    rows [0,F) = w[n] cos(2 pi f (n+off)/n_fft), rows [F,2F) = -w[n] sin(...), where the window of
    win_length taps sits centred in the n_fft frame (off = (n_fft - win_length)//2, torch.stft).
    Returns (basis, off).  Angles are reduced mod n_fft in integers before the float64 cos/sin."""
    win_length = win_length or n_fft
    if window is None:
        window = hann_periodic(win_length)
    off = (n_fft - win_length) // 2
    F = n_fft // 2 + 1
    f = np.arange(F, dtype=np.int64)[:, None]
    n = (np.arange(win_length, dtype=np.int64) + off)[None, :]
    ang = 2.0 * math.pi * ((f * n) % n_fft).astype(np.float64) / n_fft
    w = window.astype(np.float64)[None, :]
    return np.concatenate([np.cos(ang) * w, -np.sin(ang) * w], 0).astype(np.float32), off


def kaiser_sinc_filter1d(cutoff, half_width, kernel_size):
    """alias_free_torch/filter.py:27-58 restated with torch float32 ops in the same order (so the buffer
    equals the one a reference checkpoint carries).  Returns (1, 1, kernel_size)."""
    import torch
    even = kernel_size % 2 == 0
    half_size = kernel_size // 2
    delta_f = 4 * half_width
    A = 2.285 * (half_size - 1) * math.pi * delta_f + 7.95
    if A > 50.0:
        beta = 0.1102 * (A - 8.7)
    elif A >= 21.0:
        beta = 0.5842 * (A - 21) ** 0.4 + 0.07886 * (A - 21.0)
    else:
        beta = 0.0
    window = torch.kaiser_window(kernel_size, beta=beta, periodic=False)
    time = (torch.arange(-half_size, half_size) + 0.5) if even else (torch.arange(kernel_size) - half_size)
    if cutoff == 0:
        return torch.zeros(1, 1, kernel_size)
    filt = 2 * cutoff * window * torch.sinc(2 * cutoff * time)
    filt = filt / filt.sum()
    return filt.view(1, 1, kernel_size)


# ------------------------------------------------------------------------------------ sample-rate conversion
# quality -> (W = half width in zero crossings, rolloff, Kaiser beta).  "best" is the kaiser_best parameter set of resampy /
# torchaudio.functional.resample (lowpass_filter_width 64), "fast" a quarter of the width with an earlier roll-off.
RESAMPLE_QUALITIES = {
    "best": (64, 0.9475937167399596, 14.769656459379492),
    "fast": (16, 0.85, 8.555504641634386),
}
RESAMPLE_MAX_RATIO = 640          # largest o = rate_in / gcd and n = rate_out / gcd the kernel is launched with

_RESAMPLE_TABLES = {}


def resample_ratio(rate_in, rate_out):
    """-> (o, n) = (rate_in, rate_out) / gcd; ValueError for rates that are no positive integers or reduce to more than 640."""
    for r in (rate_in, rate_out):
        if isinstance(r, bool) or int(r) != r or r <= 0:
            raise ValueError(f"sample rates must be positive integers, got {rate_in!r} -> {rate_out!r}")
    rate_in, rate_out = int(rate_in), int(rate_out)
    g = math.gcd(rate_in, rate_out)
    o, n = rate_in // g, rate_out // g
    if o > RESAMPLE_MAX_RATIO or n > RESAMPLE_MAX_RATIO:
        raise ValueError(f"{rate_in} -> {rate_out} Hz reduces to {o} : {n}; both sides of the ratio must be at most {RESAMPLE_MAX_RATIO}")
    return o, n


def resample_table(rate_in, rate_out, quality="best"):
    """Coefficients of the polyphase windowed-sinc resampler, built in float64 and rounded ONCE to float32.

    With o, n = rate_in, rate_out over their gcd, base = min(o, n) * rolloff and
        win(t) = I0(beta sqrt(1 - (t / W)^2)) / I0(beta)  for |t| < W, else 0;     h(t) = sinc(t) win(t) base / o,
    output m of a signal x is  y[m] = sum_q h((q / o - m / n) base) x[q]  over the q with |(q / o - m / n) base| < W.  h depends on m
    through p = m mod n only: with m = k n + p and q = k o + d the argument is (d n - p o) base / (o n), evaluated here from that
    integer numerator.  Row p of the table holds h for d = offs[p], offs[p] + 1, ..., offs[p] being the first d inside the window;
    rows with fewer taps than the longest end in zeros.

    -> dict(o, n, taps, W, rolloff, beta, base, half = ceil(W o / base) input samples reached on either side,
            offs (n,) int32, table64 (n, taps) float64, table (n, taps) float32); cached, treat the arrays as read-only."""
    if quality not in RESAMPLE_QUALITIES:
        raise ValueError(f"unknown resampling quality {quality!r}: one of {sorted(RESAMPLE_QUALITIES)}")
    o, n = resample_ratio(rate_in, rate_out)
    key = (o, n, quality)
    if key in _RESAMPLE_TABLES:
        return _RESAMPLE_TABLES[key]
    W, rolloff, beta = RESAMPLE_QUALITIES[quality]
    base = min(o, n) * rolloff
    U = W * o * n / base                                        # |d n - p o| < U  <=>  |t| < W
    p = np.arange(n, dtype=np.int64)[:, None]

    def h_of(d):
        t = (d * n - p * o).astype(np.float64) / (o * n) * base
        inside = np.abs(t) < W
        win = np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (t / W) ** 2))) / np.i0(beta)
        return np.where(inside, np.sinc(t) * win * (base / o), 0.0), inside

    first = np.floor((p * o - U) / n).astype(np.int64) - 1       # one or two candidates before the window on either side
    cand = first + np.arange(int(2 * U / n) + 6, dtype=np.int64)[None, :]
    _, inside = h_of(cand)
    offs = cand[np.arange(n), np.argmax(inside, axis=1)]
    taps = int(inside.sum(axis=1).max())
    table64, _ = h_of(offs[:, None] + np.arange(taps, dtype=np.int64)[None, :])
    out = dict(o=o, n=n, taps=taps, W=W, rolloff=rolloff, beta=beta, base=base, half=int(math.ceil(W * o / base)),
               offs=offs.astype(np.int32), table64=table64, table=table64.astype(np.float32))
    _RESAMPLE_TABLES[key] = out
    return out



# ------------------------------------------------------------------------------------ loudness
def k_weighting(rate):
    """The two K-weighting sections of ITU-R BS.1770-4 designed for `rate` in float64: -> ((b, a) shelf, (b, a) high-pass), each a
    pair of (3,) float64 arrays with a[0] = 1 (the high-pass numerator is [1, -2, 1], not normalised, as in the standard).  At
    48000 this is the standard's coefficient table.  ValueError when the rate is no whole number of 100 ms sub-blocks."""
    if isinstance(rate, bool) or int(rate) != rate or rate <= 0:
        raise ValueError(f"k_weighting: rate = {rate!r} is no positive integer")
    rate = int(rate)
    if rate % 10:
        raise ValueError(f"k_weighting: {rate} Hz is no whole number of samples per 100 ms sub-block; resample first "
                         "(ops.resample) to a rate that is a multiple of 10")
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / rate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    d = 1.0 + K / Q + K * K
    shelf = (np.array([(Vh + Vb * K / Q + K * K) / d, 2.0 * (K * K - Vh) / d, (Vh - Vb * K / Q + K * K) / d]),
             np.array([1.0, 2.0 * (K * K - 1.0) / d, (1.0 - K / Q + K * K) / d]))
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / rate)
    d = 1.0 + K / Q + K * K
    high = (np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (K * K - 1.0) / d, (1.0 - K / Q + K * K) / d]))
    return shelf, high


def k_weighting_transitions(rate, chunk, n=7):
    """What fac_kweight_energy takes beside the signal: coef (10,) = [b0 b1 b2 a1 a2 | c0 c1 c2 d1 d2] and pw (n, 16), pw[k] the
    row-major 4 x 4 matrix M^(chunk 2^k), M the zero-input step of both sections in transposed direct form II on the state
    (s1, s2, t1, t2) (include/facodec_hip.h).  float64, by repeated squaring."""
    (b, a), (c, d) = k_weighting(rate)
    coef = np.concatenate([b, a[1:], c, d[1:]])
    M = np.array([[-a[1], 1.0, 0.0, 0.0],
                  [-a[2], 0.0, 0.0, 0.0],
                  [c[1] - d[1] * c[0], 0.0, -d[1], 1.0],
                  [c[2] - d[2] * c[0], 0.0, -d[2], 0.0]])
    if chunk < 1 or chunk & (chunk - 1):
        raise ValueError(f"k_weighting_transitions: chunk = {chunk} is no power of two")
    # the high-pass has a double pole near z = 1 (radius 0.990 at 24 kHz), which amplifies rounding by ~1 / (1 - r)^2: square in
    # extended precision where the platform has it and round once
    P = M.astype(np.longdouble)
    for _ in range(chunk.bit_length() - 1):
        P = P @ P
    pw = []
    for _ in range(n):
        pw.append(P.astype(np.float64).reshape(16))
        P = P @ P
    return coef, np.stack(pw)
