"""Level control without a GPU: an fp64 numpy restatement of the definitions in include/facodec_hip.h
(fac_agc_gains, fac_agc_apply) and the properties that follow from them -- the limiter's bound, identity where the limiter is
idle, the gain clamps, the gates, the steady state --, the descriptors' layout, and the argument checks of the C entries.

The reference arithmetic of both level-control test files lives here: `gains_ref` (the window rule on top of
test_loudness_cpu's `gated`) and `apply_ref` (ramp and limiter; every numpy operation is one IEEE fp64 operation, the sum of the
mean runs left to right).  These tests check the restatement, not the kernels; tests/test_agc.py holds the kernels to it."""
import ctypes

import numpy as np
import pytest

from facodec_amd import _lib
from test_loudness_cpu import gated, kweight_energies, loudness_ref

RATE = 24000
S = RATE // 10
DEFAULTS = dict(target_db=-23.0, window=30, max_boost_db=30.0, max_cut_db=30.0)


def ceiling(ceiling_db=-1.0):
    return 10.0 ** (float(ceiling_db) / 20.0)


# ---------------------------------------------------------------------------------------------------------------- the reference
def gains_ref(e, n_samples, target_db=-23.0, window=30, max_boost_db=30.0, max_cut_db=30.0, j_start=0, S=S):
    """-> (G dB, g linear) of the n_samples // S completed sub-blocks: the two-gate loudness of sub-blocks max(j_start, j - W + 1)
    .. j (test_loudness_cpu.gated on that slice: whole gating blocks inside the window), clamped distance from the target."""
    n = int(n_samples) // S
    G = np.zeros(n)
    for j in range(n):
        lo = max(j_start, j - window + 1)
        if j < j_start or j - lo < 3:
            continue
        win = np.asarray(e[lo:j + 1], dtype=np.float64)
        L = gated(win, len(win) * S, S)
        if L > -70.0:
            G[j] = min(max(target_db - L, -max_cut_db), max_boost_db)
    return G, 10.0 ** (G / 20.0)


def gained_ref(x, g, S=S):
    """v[n] = (double)x[n] * (g[j-2] + (g[j-1] - g[j-2]) * ((u + 1) / S)), g[-1] = g[-2] = 1."""
    x = np.asarray(x, dtype=np.float32)
    n = np.arange(len(x))
    j, u = n // S, n % S
    gp = np.concatenate([[1.0, 1.0], np.asarray(g, dtype=np.float64)])
    g2, g1 = gp[j], gp[j + 1]
    return x.astype(np.float64) * (g2 + (g1 - g2) * ((u + 1).astype(np.float64) / float(S)))


def limit_ref(v, LA, C):
    """-> (y (len(v) + LA,) float32, s (len(v) + LA,) float64, c of samples -2 LA .. len(v) + LA - 1)."""
    N = len(v)
    vp = np.concatenate([np.zeros(2 * LA), v, np.zeros(LA)])                   # samples -2 LA .. N + LA - 1
    mag = np.abs(vp)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(mag > C, C / mag, 1.0)
    M = N + LA
    # p of samples -LA + 1 .. N + LA - 1: index i <-> sample i - LA + 1 = vp index i + LA + 1; its window is vp indices i + 1 .. i + LA + 1
    P = M + LA - 1
    p = c[1:1 + P].copy()
    for w in range(2, LA + 2):
        p = np.minimum(p, c[w:w + P])
    # output m = 0 .. M - 1 sums p of samples m - LA + 1 .. m = indices m .. m + LA - 1, left to right
    acc = p[0:M].copy()
    for w in range(1, LA):
        acc = acc + p[w:w + M]
    s = np.minimum(acc / float(LA), c[LA:LA + M])                               # c[m - LA] sits at vp index m + LA
    y = (vp[LA:LA + M] * s).astype(np.float32)
    return y, s, c


def apply_ref(x, g, LA=120, C=None, S=S):
    return limit_ref(gained_ref(x, g, S), LA, ceiling() if C is None else C)[0]


def level_ref(x, lookahead=120, ceiling_db=-1.0, **kw):
    par = dict(DEFAULTS, **kw)
    G, g = gains_ref(kweight_energies(x, RATE), len(x), **par)
    return apply_ref(x, g, lookahead, ceiling(ceiling_db)), G, g


@pytest.fixture(scope="module")
def jump():
    """3 s: 1.5 s of 0.003 rms Gaussian noise, then 0.5 rms; its energies, computed once."""
    g = np.random.default_rng(11)
    x = g.standard_normal(72000)
    x[:36000] *= 0.003
    x[36000:] *= 0.5
    x = x.astype(np.float32)
    return dict(x=x, e=kweight_energies(x, RATE))


# ---------------------------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("LA", [7, 120])
def test_limiter_bound(jump, LA):
    """|y| <= fp32(C) (1 + 2^-22) on every sample: every p in the mean contains c[m - LA], so s <= c[m - LA] up to the roundings
    of the quotient C / |v|, the mean and the product (fp64, 2^-52 each), and one rounding to fp32 (2^-24 relative)."""
    G, g = gains_ref(jump["e"], 72000, window=5, **{k: v for k, v in DEFAULTS.items() if k != "window"})
    assert G.max() > 20.0                                            # the quiet half was boosted: the jump arrives with that gain
    C = ceiling()
    v = gained_ref(jump["x"], g)
    assert np.max(np.abs(v)) > 4.0 * C                               # and has to be held
    y, s, _ = limit_ref(v, LA, C)
    assert y.dtype == np.float32 and len(y) == 72000 + LA
    bound = float(np.float32(C)) * (1.0 + 2.0 ** -22)
    print(f"LA = {LA}: max |y| = {np.max(np.abs(y)):.9f}, fp32(C) = {float(np.float32(C)):.9f}, min s = {s.min():.4f}")
    assert np.max(np.abs(y.astype(np.float64))) <= bound


@pytest.mark.parametrize("LA", [7, 120])
def test_identity_where_the_limiter_is_idle(jump, LA):
    """s[m] = 1 exactly wherever no |v| > C lies in m - 2 LA + 1 .. m: the output there is (float)v, LA samples late."""
    g = gains_ref(jump["e"], 72000, **DEFAULTS)[1]
    C = ceiling()
    v = gained_ref(jump["x"], g)
    y, s, c = limit_ref(v, LA, C)
    hit = (c < 1.0).astype(np.int64)                                 # c of samples -2 LA .. ; output m's window is indices m + 1 .. m + 2 LA
    cs = np.concatenate([[0], np.cumsum(hit)])
    m = np.arange(len(y))
    idle = (cs[m + 2 * LA + 1] - cs[m + 1]) == 0
    assert idle.sum() > 30000 and (~idle).sum() > 1000
    assert np.all(s[idle] == 1.0)
    delayed = np.concatenate([np.zeros(LA), v]).astype(np.float32)
    assert np.array_equal(y[idle], delayed[idle])
    assert np.all(s[~idle] <= 1.0) and s[~idle].min() < 1.0


def test_gain_clamps():
    g = np.random.default_rng(12)
    loud = (0.5 * g.standard_normal(12000)).astype(np.float32)
    quiet = (0.0005 * g.standard_normal(12000)).astype(np.float32)
    for x, kw, want in ((loud, dict(max_cut_db=6.0), -6.0), (quiet, dict(max_boost_db=12.0), 12.0)):
        e = kweight_energies(x, RATE)
        G, lin = gains_ref(e, len(x), **dict(DEFAULTS, **kw))
        free = gains_ref(e, len(x), **dict(DEFAULTS, max_boost_db=100.0, max_cut_db=100.0))[0]
        assert np.all(G[:3] == 0.0) and np.all(lin[:3] == 1.0)       # fewer than 4 sub-blocks in the window: no gain yet
        assert np.all(np.abs(free[3:]) > abs(want) + 3.0)            # the unclamped gain lies well outside
        assert np.all(G[3:] == want)
        assert np.allclose(lin[3:], 10.0 ** (want / 20.0), rtol=1e-15)


def test_rows_under_the_absolute_gate_are_left_alone():
    g = np.random.default_rng(13)
    x = (1e-5 * g.standard_normal(24000)).astype(np.float32)         # about -100 LUFS
    assert loudness_ref(x) == -70.0
    y, G, lin = level_ref(x)
    assert np.all(G == 0.0) and np.all(lin == 1.0)
    assert np.array_equal(y[120:], x) and np.all(y[:120] == 0.0)
    # and a window that has left the loud part behind falls back to no gain
    x2 = np.concatenate([(0.1 * g.standard_normal(12000)).astype(np.float32), x])
    G2 = gains_ref(kweight_energies(x2, RATE), len(x2), **dict(DEFAULTS, window=5))[0]
    # (sub-block 5 still holds the high-pass filter's decaying tail of the loud part, so the window is clear from j = 10 on)
    assert np.all(G2[3:5] < 0.0) and np.all(G2[10:] == 0.0)


def test_window_start_of_a_restarted_row():
    """j_start: the sub-blocks before it are outside every window and get no gain; from it on the row is a fresh stream."""
    g = np.random.default_rng(14)
    x = (0.05 * g.standard_normal(24000)).astype(np.float32)
    e = kweight_energies(x, RATE)
    fresh = gains_ref(e[4:], 6 * S, **DEFAULTS)[0]
    moved = gains_ref(e, 10 * S, j_start=4, **DEFAULTS)[0]
    assert np.all(moved[:4] == 0.0) and np.array_equal(moved[4:], fresh)


def test_steady_state_reaches_the_target():
    """A stationary Gaussian row at -47.5 LUFS levelled to -23 (a boost of 24.5 dB, inside the clamp) measures -23 within 0.1 LU
    over seconds 4 to 6 (test_loudness_cpu.loudness_ref).  The gain of sub-block j comes from the 3 s before it, so the
    levelled signal misses the target only by the window's own estimation noise: a numpy prototype of this rule read -22.989 on
    another row, this row reads -22.971; 0.1 LU is some four times that, and a wrong window, gate or ramp misses by 1 LU or more."""
    g = np.random.default_rng(15)
    x = g.standard_normal(6 * RATE)
    x = (x * 10.0 ** ((-47.5 - loudness_ref(x)) / 20.0)).astype(np.float32)
    assert abs(loudness_ref(x) + 47.5) < 1e-3
    y, G, _ = level_ref(x, lookahead=120)
    got = loudness_ref(y[120 + 4 * RATE:120 + 6 * RATE].astype(np.float64))
    print(f"steady state: {got:.4f} LUFS over seconds 4 .. 6 (target -23), gains {G[30:].min():.3f} .. {G[30:].max():.3f} dB")
    assert abs(got + 23.0) <= 0.1
    assert np.max(np.abs(y)) < ceiling()                             # the limiter had nothing to do here


# ---------------------------------------------------------------------------------------------------------------- the C entries
FAKE = 0x10000                                                       # never dereferenced: every case below is refused before a launch


def _gains_desc(**kw):
    d = _lib.AgcGainsDesc()
    d.e, d.G, d.g = FAKE, FAKE, FAKE
    d.e_bs, d.g_bs, d.j0 = 30, 30, 0
    d.target_db, d.max_boost_db, d.max_cut_db = -23.0, 30.0, 30.0
    d.B, d.n_new, d.R, d.W, d.S = 2, 30, 30, 30, 2400
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _apply_desc(**kw):
    d = _lib.AgcApplyDesc()
    d.x, d.g, d.y = FAKE, FAKE, FAKE
    d.x_bs, d.g_bs, d.y_bs, d.n0 = 4800, 2, 4920, 0
    d.ceiling = ceiling()
    d.B, d.k, d.n_out, d.S, d.LA, d.R = 2, 4800, 4920, 2400, 120, 2
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def check_refusals():
    """Error code and message of every refusal the header lists, before any launch (no pointer is dereferenced)."""
    lib = _lib.load()

    def err():
        return lib.fac_last_error()

    assert lib.fac_agc_gains(None, None) == -1 and b"null descriptor" in err()
    for kw, msg in ((dict(e=None), b"null energy"), (dict(G=None, g=None), b"neither G nor g"), (dict(B=0), b"B = 0"),
                    (dict(B=65536), b"B = 65536"), (dict(n_new=0), b"n_new = 0"), (dict(W=3), b"window = 3"),
                    (dict(W=_lib.AGC_MAX_WINDOW + 1), b"window = 1025"), (dict(S=0), b"S = 0"), (dict(j0=-1), b"j0 = -1"),
                    (dict(max_boost_db=-1.0), b"max_boost_db"), (dict(max_cut_db=float("nan")), b"max_cut_db"),
                    (dict(target_db=float("inf")), b"target_db"), (dict(R=29), b"R = 29"), (dict(j0=100, R=58), b"R = 58"),
                    (dict(e_bs=29), b"e_bs = 29"), (dict(g_bs=29), b"g_bs = 29")):
        assert lib.fac_agc_gains(ctypes.byref(_gains_desc(**kw)), None) == -1, kw
        assert msg in err(), (kw, err())

    assert lib.fac_agc_apply(None, None) == -1 and b"null descriptor" in err()
    for kw, msg in ((dict(g=None), b"null gain or output"), (dict(y=None), b"null gain or output"), (dict(x=None), b"null block pointer"),
                    (dict(B=0), b"B = 0"), (dict(k=-1), b"k = -1"), (dict(LA=0), b"LA = 0"),
                    (dict(LA=_lib.AGC_MAX_LOOKAHEAD + 1), b"LA = 1025"), (dict(n_out=4799), b"n_out = 4799"),
                    (dict(n_out=4921), b"n_out = 4921"), (dict(k=0, n_out=0), b"n_out = 0"), (dict(S=0), b"S = 0"),
                    (dict(ceiling=0.0), b"ceiling"), (dict(ceiling=float("inf")), b"ceiling"), (dict(n0=-1), b"n0 = -1"),
                    (dict(carry_in=FAKE, carry_out=FAKE), b"carry_out is carry_in"),
                    (dict(lens=FAKE, carry_in=FAKE), b"lens does not go with a carried stream"),
                    (dict(lens=FAKE, carry_out=FAKE), b"lens does not go with a carried stream"),
                    (dict(x_bs=4799), b"x_bs = 4799"), (dict(y_bs=4919), b"y_bs = 4919"), (dict(R=0), b"R = 0"),
                    (dict(k=7200, n_out=7320, x_bs=7200, y_bs=7320, R=1), b"R = 1"), (dict(n0=240000, R=2), b"R = 2"), (dict(R=4, g_bs=3), b"g_bs = 3")):
        assert lib.fac_agc_apply(ctypes.byref(_apply_desc(**kw)), None) == -1, kw
        assert msg in err(), (kw, err())

    def tp(**kw):
        d = _lib.ResampleDesc()
        d.x, d.table, d.offs = FAKE, FAKE, FAKE
        d.x_bs, d.B, d.T, d.n_out, d.o, d.n, d.taps = 5000, 4, 5000, 20000, 1, 4, 65
        peak, ws = kw.pop("peak", FAKE), kw.pop("ws", FAKE)
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.fac_true_peak(ctypes.byref(d), peak, ws, None)

    assert lib.fac_true_peak(None, FAKE, FAKE, None) == -1 and b"null descriptor" in err()
    for kw, msg in ((dict(x=None), b"null pointer"), (dict(peak=None), b"null pointer"), (dict(ws=None), b"null pointer"),
                    (dict(hist=FAKE), b"offline form"), (dict(q0=1), b"offline form"), (dict(o=0), b"o = 0"), (dict(n=641), b"n = 641"),
                    (dict(taps=0), b"table geometry"), (dict(B=0), b"bad sizes"), (dict(T=-1), b"bad sizes"), (dict(x_bs=4999), b"x_bs = 4999"),
                    (dict(o=640, n=1), b"span")):
        assert tp(**kw) == -1, kw
        assert msg in err(), (kw, err())
    assert lib.fac_true_peak_ws_bytes(0, 10) == -1 and lib.fac_true_peak_ws_bytes(1, -1) == -1
    assert lib.fac_true_peak_ws_bytes(3, 20000) >= 3 * 4 * 20


def test_c_entries_refuse_bad_arguments_without_a_gpu():
    check_refusals()


def test_parameter_checks_of_the_python_surface():
    import torch
    from facodec_amd import commons, ops, streaming
    p = ops.agc_params()
    assert (p.S, p.W, p.LA) == (2400, 30, 120) and p.ceiling == ceiling(-1.0)
    for kw in (dict(window=3), dict(window=1025), dict(lookahead=0), dict(lookahead=1025), dict(max_boost_db=-1.0),
               dict(max_cut_db=float("inf")), dict(target_db=float("nan")), dict(ceiling_db=float("inf"))):
        with pytest.raises(ValueError):
            ops.agc_params(**kw)
    with pytest.raises(ValueError, match="resample first"):
        ops.agc_params(11025)
    with pytest.raises(ValueError, match="resample first"):
        commons.level_clips([torch.zeros(100)], 11025)
    assert commons.level_clips([]) == []
    with pytest.raises(_lib.FacodecHipError, match="no CPU path"):
        ops.level(torch.zeros(1, 4800))
    with pytest.raises(_lib.FacodecHipError, match="no CPU path"):
        ops.true_peak(torch.zeros(1, 4800))
    with pytest.raises(ValueError, match="quality"):
        ops.true_peak(torch.zeros(1, 4800), quality="nope")
    with pytest.raises(ValueError, match="ring"):
        streaming.AutoGain(1, ring=32, device="cpu")
    with pytest.raises(ValueError, match="takes codes"):
        streaming.LevelledSession(object())


def test_desc_layouts_match_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    fields = [("fac_agc_gains_desc", f) for f in ("e_bs", "j0", "target_db", "B", "S")] + \
             [("fac_agc_apply_desc", f) for f in ("x_bs", "n0", "ceiling", "B", "R")]
    args = ", ".join(["sizeof(fac_agc_gains_desc)", "sizeof(fac_agc_apply_desc)"] + [f"offsetof({s}, {f})" for s, f in fields])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "facodec_hip.h"\nint main(){printf("' + "%zu " * (2 + len(fields)) +
                   '\\n", ' + args + ");return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(repo, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    gd, ad = _lib.AgcGainsDesc, _lib.AgcApplyDesc
    want = [ctypes.sizeof(gd), ctypes.sizeof(ad)] + [getattr(gd if s == "fac_agc_gains_desc" else ad, f).offset for s, f in fields]
    assert out == want
    assert (_lib.AGC_MAX_WINDOW, _lib.AGC_MAX_LOOKAHEAD) == (1024, 1024)
