"""The resampler's host side, no GPU: filter quality of the float64 coefficient table against its stated pass band,
roll-off and stop band, the table's geometry and rounding, the launch form chosen per table size, and every refusal that is made
on the host before a launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

from facodec_amd import _lib, dsp, ops, streaming

PAIRS = [(48000, 24000), (44100, 24000), (16000, 24000), (24000, 16000), (24000, 48000), (24000, 44100), (8000, 24000)]
QUALITIES = ("best", "fast")


def _apply(geo, x):
    """The definition with the table's coefficients, float64: y[m] = sum_j table64[p][j] x[k o + offs[p] + j], m = k n + p."""
    o, n, taps = geo["o"], geo["n"], geo["taps"]
    L = len(x)
    m = np.arange(-(-L * n // o))
    k, p = m // n, m % n
    q = (k * o + geo["offs"][p])[:, None] + np.arange(taps)[None, :]
    xv = np.where((q >= 0) & (q < L), x[np.clip(q, 0, L - 1)], 0.0)
    return (geo["table64"][p] * xv).sum(axis=1)


def _amplitude(rate_in, rate_out, quality, freq):
    """sqrt(2) RMS over the middle half of the resampled 0.1 s sine of `freq` Hz."""
    t = np.arange(int(0.1 * rate_in)) / rate_in
    y = _apply(dsp.resample_table(rate_in, rate_out, quality), np.sin(2 * np.pi * freq * t))
    mid = y[len(y) // 4: 3 * len(y) // 4]
    return math.sqrt(2.0 * np.mean(mid ** 2))


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("rate_in,rate_out", PAIRS)
def test_pass_band_roll_off_and_stop_band(rate_in, rate_out, quality):
    nyq = min(rate_in, rate_out) / 2
    assert abs(_amplitude(rate_in, rate_out, quality, 1000.0) - 1.0) < 1e-3
    edge = _amplitude(rate_in, rate_out, quality, 0.8 * nyq)
    if quality == "best":
        assert abs(edge - 1.0) < 1e-3, edge
    else:
        assert abs(edge - 0.8439) < 1e-3, edge                 # the stated roll-off of "fast" at 0.8 of the lower Nyquist
    if rate_out < rate_in:
        alias = _amplitude(rate_in, rate_out, quality, 1.15 * nyq)
        assert alias < (1e-5 if quality == "best" else 1e-4), alias


def _h_formula(t, W, beta, base, o):
    win = np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (t / W) ** 2))) / np.i0(beta)
    return np.where(np.abs(t) < W, np.sinc(t) * win * base / o, 0.0)


GEOMETRY = {   # (rate_in, rate_out) -> (o, n)
    (48000, 24000): (2, 1), (44100, 24000): (147, 80), (16000, 24000): (2, 3), (24000, 16000): (3, 2), (24000, 48000): (1, 2),
    (24000, 44100): (80, 147), (8000, 24000): (1, 3), (11025, 24000): (147, 320),
}


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("rate_in,rate_out", sorted(GEOMETRY))
def test_table_geometry_and_rounding(rate_in, rate_out, quality):
    geo = ops.resample_table(rate_in, rate_out, quality)
    o, n = GEOMETRY[(rate_in, rate_out)]
    W, rolloff, beta = dsp.RESAMPLE_QUALITIES[quality]
    # taps = the most integers d any phase has inside the window |d n - p o| base / (o n) < W, counted one by one
    reach = int(W * o / (min(o, n) * rolloff)) + 2
    d_all = np.arange(-reach, o + reach + 1)[None, :]
    count = (np.abs((d_all * n - np.arange(n)[:, None] * o) / (o * n) * (min(o, n) * rolloff)) < W).sum(axis=1)
    assert (geo["o"], geo["n"], geo["taps"]) == (o, n, count.max())
    assert abs(geo["taps"] - (2 * W * o / (min(o, n) * rolloff) + 1)) <= 2.5          # taps ~ 2 W o / base + 1
    assert geo["table"].dtype == np.float32 and geo["table"].shape == (n, geo["taps"]) and geo["offs"].shape == (n,)
    assert np.array_equal(geo["table"], geo["table64"].astype(np.float32))               # rounded once
    # every row is the formula at d = offs[p] + j, and the taps before and behind each row lie outside the window
    base = min(o, n) * rolloff
    p = np.arange(n)[:, None]
    d = geo["offs"][:, None].astype(np.int64) + np.arange(-1, geo["taps"] + 1)[None, :]
    h = _h_formula((d * n - p * o) / (o * n) * base, W, beta, base, o)
    assert np.all(h[:, 0] == 0.0) and np.all(h[:, -1] == 0.0)
    assert np.allclose(h[:, 1:-1], geo["table64"], rtol=0, atol=1e-15)
    if n > o:
        assert np.all(np.abs(geo["table64"].sum(axis=1) - 1.0) < 1e-3)                   # unity DC gain in every phase
    assert geo["half"] == math.ceil(W * o / base)


def _desc(geo, B, T, n_out=None):
    d = _lib.ResampleDesc()
    d.x = d.y = d.table = d.offs = 0x10000                         # never dereferenced: fac_resample_form stops before the launch
    d.B, d.T, d.n_out = B, T, -(-T * geo["n"] // geo["o"]) if n_out is None else n_out
    d.o, d.n, d.taps = geo["o"], geo["n"], geo["taps"]
    return d


def test_launch_form_follows_the_table_size():
    """Where the table lives: in LDS beside the span while it fits, in global memory beyond; extreme ratios read inputs from
    global memory too.  The staged span must hold what the tile's outputs read, for every phase a tile can start at."""
    form = lambda a, b, q, B=32, T=96000: ops.resample_form(_desc(ops.resample_table(a, b, q), B, T))
    assert form(48000, 24000, "best")[0] == 0 and form(44100, 24000, "best")[0] == 0 and form(24000, 44100, "best")[0] == 0
    assert form(11025, 24000, "best")[0] == 1                       # 320 x 136 coefficients = 174 KB: more than a CU's LDS
    assert form(11025, 24000, "fast")[0] == 0
    assert form(640, 1, "fast", 1, 64000)[0] == 2 and form(1, 640, "best", 1, 100)[0] == 1
    for a, b, q in [(48000, 24000, "best"), (44100, 24000, "best"), (24000, 44100, "fast"), (11025, 24000, "best"), (640, 639, "best"),
                    (24000, 16000, "fast"), (639, 640, "fast")]:
        geo = ops.resample_table(a, b, q)
        o, n, taps, offs = geo["o"], geo["n"], geo["taps"], geo["offs"].astype(np.int64)
        f, tm, threads, lds, gx = ops.resample_form(_desc(geo, 3, 20011))
        assert f in (0, 1) and threads % 64 == 0 and 64 <= threads <= 1024 and lds <= 160 * 1024 and gx >= 1
        cap = ((tm - 1) * o + n - 1) // n + taps + 2               # span_cap_for (resample.hip)
        first = lambda m: m // n * o + offs[m % n]
        p0 = np.arange(n)
        assert np.all(first(p0 + tm - 1) + taps - first(p0) <= cap)
        words = cap + cap // 32 + 1
        assert lds == 4 * (words + (n * (taps | 1) if f == 0 else 0))
        assert np.all(np.diff(first(np.arange(3 * n))) >= 0)        # first taps never step back: a tile's span starts at its first output


def test_refusals_on_the_host():
    with pytest.raises(ValueError, match="640"):
        ops.resample_table(48000, 44099, "best")                    # coprime: 48000 : 44099
    with pytest.raises(ValueError, match="640"):
        ops.resample_table(641, 1, "fast")
    assert ops.resample_table(640, 1, "fast")["o"] == 640 and ops.resample_table(1, 640, "fast")["n"] == 640
    with pytest.raises(ValueError, match="quality"):
        ops.resample_table(48000, 24000, "better")
    for bad in (0, -16000, 22050.5):
        with pytest.raises(ValueError):
            ops.resample_table(bad, 24000, "best")
    with pytest.raises(ValueError):
        ops.resample(torch.zeros(2, 100), 48000, 24000, quality="better")
    with pytest.raises(_lib.FacodecHipError):
        ops.resample(torch.zeros(2, 100), 48000, 24000)
    with pytest.raises(_lib.FacodecHipError):
        ops.resample(torch.zeros(2, 1, 100), 24000, 24000)          # equal rates: still no CPU path
    lib = _lib.load()
    d = _desc(ops.resample_table(48000, 24000, "best"), 1, 100)
    d.o = 641
    assert lib.fac_resample(ctypes.byref(d), None) == -1 and b"640" in lib.fac_last_error()
    d = _desc(ops.resample_table(48000, 24000, "best"), 1, 100)
    d.n_hist = 8
    assert lib.fac_resample(ctypes.byref(d), None) == -1 and b"history" in lib.fac_last_error()


class _Stub:
    """What ResampledSession reads of a session before it allocates anything."""
    B, prime_samples, device = 2, 4800, torch.device("cpu")


def test_resampled_session_refuses_rates_that_split_a_hop_or_a_frame():
    with pytest.raises(ValueError, match="in_rate"):
        streaming.ResampledSession(_Stub(), in_rate=11025)           # 480 samples at 24 kHz = 220.5 at 11 025 Hz
    with pytest.raises(ValueError, match="out_rate"):
        streaming.ResampledSession(_Stub(), out_rate=44100)          # 300 samples = 551.25 at 44 100 Hz
    with pytest.raises(ValueError, match="quality"):
        streaming.ResampledSession(_Stub(), in_rate=48000, quality="better")
    with pytest.raises(ValueError, match="640"):
        streaming.ResampledSession(_Stub(), in_rate=24001)
    codes_only = type("Rx", (), dict(B=2, device=torch.device("cpu")))()
    with pytest.raises(ValueError, match="codes"):
        streaming.ResampledSession(codes_only, in_rate=48000)
    s = streaming.ResampledSession(_Stub())                            # both sides at 24 kHz: nothing to build, nothing added
    assert s.rs_in is None and s.rs_out is None and s.hop_samples == 480 and s.prime_samples == 4800
    assert s.latency_in == 0.0 and s.latency_out == 0.0


def test_stream_delay_reaches_nothing_right_of_the_block():
    """delay = ceil(ceil(W o / base) n / o): the last output a block of the delayed stream emits reads no input behind the block."""
    for a, b, q in [(48000, 24000, "fast"), (44100, 24000, "best"), (24000, 48000, "fast"), (24000, 16000, "fast")]:
        geo = ops.resample_table(a, b, q)
        o, n = geo["o"], geo["n"]
        W, rolloff, _ = dsp.RESAMPLE_QUALITIES[q]
        D = math.ceil(math.ceil(W * o / (min(o, n) * rolloff)) * n / o)
        for blocks in range(1, 4):
            q_end = blocks * o                                     # the shortest admissible blocks
            m_last = q_end * n // o - 1 - D
            start = m_last // n * o + int(geo["offs"][m_last % n])
            used = np.nonzero(geo["table64"][m_last % n])[0]
            assert start + used.max() < q_end


def test_stream_descriptors_pass_the_host_checks():
    """The descriptors a stream makes -- a block with carried history, the empty block of finish() (T = 0 over a buffer that has
    a pointer: an empty tensor has none), absolute indices past 2^31 -- are accepted by the planner; nothing is launched."""
    geo = ops.resample_table(48000, 24000, "fast")
    table, offs = torch.from_numpy(geo["table"]), torch.from_numpy(geo["offs"])
    D, n_hist = 19, 77
    hist = [torch.zeros(2, n_hist), torch.zeros(2, n_hist)]
    assert torch.zeros(2, n_hist)[:, :0].data_ptr() == 0
    for q0 in (0, 960, 3 * 2 ** 33):
        d = ops.resample_desc(geo, table, offs, torch.zeros(2, 960), torch.empty(2, 480), 480, hist=hist[0], hist_out=hist[1],
                              q0=q0, m_lo=q0 // 2 - D)
        assert ops.resample_form(d)[0] == 0 and d.T == 960 and d.n_hist == n_hist
        d = ops.resample_desc(geo, table, offs, hist[0], torch.empty(2, D), D, hist=hist[0], q0=q0, m_lo=q0 // 2 - D, T=0)
        assert ops.resample_form(d)[0] == 0 and d.T == 0 and d.x
