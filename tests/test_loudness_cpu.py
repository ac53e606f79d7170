"""Loudness without a GPU: the K-weighting design against the coefficient table of ITU-R BS.1770-4, the 997 Hz
gain, the rate rule, the container's loudness field, and the argument checks of the three C entries.

The reference arithmetic of both loudness test files lives here: `biquad` (a plain float64 direct-form-I recurrence),
`kweight_energies` and `gated` (the gating rule of include/facodec_hip.h / the standard, restated).  Nothing of the package
enters it except the coefficients, which this file pins to the standard's table first."""
import ctypes
import math
import struct

import numpy as np
import pytest

from facodec_amd import _lib, bitstream, dsp

# ITU-R BS.1770-4, tables 1 and 2 (48 kHz), and the same design at 24 kHz
SHELF_48 = ([1.53512485958697, -2.69169618940638, 1.19839281085285], [1.0, -1.69065929318241, 0.73248077421585])
HIGH_48 = ([1.0, -2.0, 1.0], [1.0, -1.99004745483398, 0.99007225036621])
SHELF_24 = ([1.4879002209622763, -2.2462054681411368, 0.904909123246438], [1.0, -1.3902346051928203, 0.5368384812603979])
HIGH_24 = ([1.0, -2.0, 1.0], [1.0, -1.9801441262289323, 0.9802428178592764])


# ---------------------------------------------------------------------------------------------------------------- the reference
def biquad(x, b, a):
    """y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2] from zero state, float64 (Python floats are doubles)."""
    b0, b1, b2 = (float(v) for v in b)
    a1, a2 = float(a[1]), float(a[2])
    x1 = x2 = y1 = y2 = 0.0
    out = []
    for xn in np.asarray(x, dtype=np.float64).tolist():
        yn = b0 * xn + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        x2, x1, y2, y1 = x1, xn, y1, yn
        out.append(yn)
    return np.array(out, dtype=np.float64)


def kweight_energies(x, rate=24000):
    """Sub-block energies of the clip's own samples: (ceil(len / S),) float64."""
    (b1, a1), (b2, a2) = dsp.k_weighting(rate)
    S = rate // 10
    y = biquad(biquad(x, b1, a1), b2, a2)
    return np.array([np.sum(y[j:j + S] ** 2) for j in range(0, len(y), S)], dtype=np.float64)


def block_levels(e, n_samples, S):
    """-> (z per gating block, l per gating block)."""
    if n_samples <= 0:
        return np.zeros(0), np.zeros(0)
    n_blocks = 1 if n_samples < 4 * S else (n_samples - 4 * S) // S + 1
    z = np.array([np.sum(e[j:j + 4]) / (4 * S) for j in range(n_blocks)])
    with np.errstate(divide="ignore"):
        return z, -0.691 + 10.0 * np.log10(z)


def gated(e, n_samples, S, gates=2):
    """Integrated loudness from sub-block energies; gates = 2 the standard's, 1 the absolute gate alone, 0 none."""
    z, l = block_levels(e, n_samples, S)
    keep = np.ones(len(z), dtype=bool)
    if gates >= 1:
        keep = l > -70.0
    if gates >= 2 and keep.any():
        keep &= l > -0.691 + 10.0 * math.log10(z[keep].mean()) - 10.0
    if not keep.any() or z[keep].mean() <= 0.0:
        return -70.0
    return max(-70.0, -0.691 + 10.0 * math.log10(z[keep].mean()))


def loudness_ref(x, rate=24000):
    return gated(kweight_energies(x, rate), len(x), rate // 10)


def gain_ref(L, target, peak):
    g = 1.0 if L <= -70.0 else 10.0 ** ((target - L) / 20.0)
    if g * peak > 1.0:
        g = 1.0 / peak
    return g


# ---------------------------------------------------------------------------------------------------------------- the design
@pytest.mark.parametrize("rate,shelf,high", [(48000, SHELF_48, HIGH_48), (24000, SHELF_24, HIGH_24)])
def test_k_weighting_is_the_standards_table(rate, shelf, high):
    (b1, a1), (b2, a2) = dsp.k_weighting(rate)
    for got, want in ((b1, shelf[0]), (a1, shelf[1]), (b2, high[0]), (a2, high[1])):
        assert got.dtype == np.float64 and got.shape == (3,)
        assert np.max(np.abs(got - np.array(want))) <= 1e-13


def _gain_997(rate):
    w = 2.0 * math.pi * 997.0 / rate
    z = np.exp(-1j * w * np.arange(3))
    h = 1.0
    for b, a in dsp.k_weighting(rate):
        h *= np.dot(b, z) / np.dot(a, z)
    return -0.691 + 10.0 * math.log10(abs(h) ** 2 / 2.0)


def test_gain_at_997_hz():
    """A full-scale 997 Hz sine reads -3.01 LUFS at 48 kHz (the standard's calibration); the 24 kHz design reads -2.9843."""
    assert abs(_gain_997(48000) - (-3.0103)) <= 1e-4
    assert abs(_gain_997(24000) - (-2.9843)) <= 1e-4


def test_rates_that_are_no_whole_sub_block_raise():
    import torch
    from facodec_amd import ops
    with pytest.raises(ValueError, match="resample first"):
        dsp.k_weighting(11025)
    with pytest.raises(ValueError, match="resample first"):
        ops.loudness(torch.zeros(1, 11025), rate=11025)
    with pytest.raises(ValueError, match="resample first"):
        ops.normalize_loudness(torch.zeros(1, 11025), rate=11025)
    with pytest.raises(_lib.FacodecHipError, match="no CPU path"):
        ops.loudness(torch.zeros(1, 24000))
    with pytest.raises(_lib.FacodecHipError, match="no CPU path"):
        ops.loudness_energies(torch.zeros(1, 24000))
    with pytest.raises(_lib.FacodecHipError, match="no CPU path"):
        ops.normalize_loudness(torch.zeros(1, 1, 24000))


def test_transition_matrices_are_the_recurrence():
    """pw[k] of dsp.k_weighting_transitions is the zero-input response of the two sections over chunk * 2^k samples, on the state
    (s1, s2, t1, t2) of the transposed direct form II that include/facodec_hip.h writes out: checked by running that form in
    float64.  The bound: the high-pass poles (a double pole of radius 0.990) amplify the run's own rounding by about
    1 / (1 - r)^2 = 1e4, i.e. to ~1e-12 of the largest entry; 1e-10 leaves room for that and is far below a wrong power or a
    transposed matrix, which are wrong in the first digit."""
    chunk = 256
    coef, pw = dsp.k_weighting_transitions(24000, chunk)
    (b, a), (c, d) = dsp.k_weighting(24000)
    assert np.array_equal(coef, np.concatenate([b, a[1:], c, d[1:]])) and pw.shape == (7, 16)

    def run(state, n):
        s1, s2, t1, t2 = state
        for _ in range(n):
            y1 = s1
            s1, s2 = s2 - a[1] * y1, -a[2] * y1
            y = c[0] * y1 + t1
            t1, t2 = (c[1] * y1 + t2) - d[1] * y, c[2] * y1 - d[2] * y
        return np.array([s1, s2, t1, t2])

    for k in (0, 1, 3):
        M = pw[k].reshape(4, 4)
        for i in range(4):
            unit = np.zeros(4)
            unit[i] = 1.0
            want = run(unit, chunk << k)
            assert np.max(np.abs(M[:, i] - want)) <= 1e-10 * max(1.0, np.max(np.abs(want)))


# ---------------------------------------------------------------------------------------------------------------- the container
HEAD = dict(bits=10, n_q=(1, 2, 3), sample_rate=24000, n_frames=2, n_samples=600, codebook_size=1024)
PLAIN_BLOB = bytes.fromhex("46414342010a010203000000c05d000002000000580200000004000000000000"
                           "000000000000000000000000000000" "5cf9dd93")


def test_blob_without_loudness_is_the_blob_of_before():
    """The bytes of one small case, written down when the field did not exist: header (flags 0, reserved 0), 15 payload bytes, CRC."""
    blob = bitstream.write(HEAD, None, bytes(15))
    assert blob == PLAIN_BLOB
    assert bitstream.write(dict(HEAD, input_db=None), None, bytes(15)) == PLAIN_BLOB
    hdr, tim, payload = bitstream.read(blob)
    assert hdr.input_db is None and not hdr.has_loudness and hdr.flags == 0 and tim is None and payload == bytes(15)
    assert hdr.version == 1


def test_blob_with_loudness_round_trips_through_float32():
    timbre = np.arange(8, dtype=np.float32)
    payload = bytes(range(15))
    for db in (-23.456789, -70.0, 0.0):
        blob = bitstream.write(dict(HEAD, input_db=db), timbre, payload)
        plain = bitstream.write(HEAD, timbre, payload)
        assert len(blob) == len(plain) + 4 and blob[4] == 1 and blob[28:32] == bytes(4)             # version 1, reserved 0
        assert blob[9] == bitstream.FLAG_TIMBRE | bitstream.FLAG_LOUDNESS and bitstream.FLAG_LOUDNESS == 4
        assert blob[32 + 32:32 + 36] == struct.pack("<f", db)                                       # behind the timbre, before the payload
        hdr, tim, got = bitstream.read(blob)
        assert hdr.input_db == float(np.float32(db)) and hdr.has_loudness
        assert np.array_equal(tim, timbre) and got == payload
        assert bitstream.write(hdr, tim, got) == blob                                               # a Header goes back in unchanged
    hdr = bitstream.read(bitstream.write(dict(HEAD, input_db=-20.0), None, payload))[0]
    assert hdr.flags == bitstream.FLAG_LOUDNESS and hdr.input_db == -20.0


def _with_crc(body):
    import zlib
    return body + struct.pack("<I", zlib.crc32(body))


def test_loudness_flag_keeps_the_length_checks():
    payload = bytes(15)
    blob = bitstream.write(dict(HEAD, input_db=-20.0), None, payload)
    for cut in (1, 4, 5, 19):
        with pytest.raises(ValueError, match="truncated"):
            bitstream.read(blob[:-cut])
    # the flag set on a blob that has no room for the field: the length disagrees (here: is too short) whatever the CRC says
    plain = bytearray(bitstream.write(HEAD, None, payload))
    plain[9] |= bitstream.FLAG_LOUDNESS
    with pytest.raises(ValueError, match="truncated"):
        bitstream.read(_with_crc(bytes(plain[:-4])))
    # ... and cleared on a blob that carries it: four bytes too many
    long = bytearray(blob)
    long[9] &= ~bitstream.FLAG_LOUDNESS
    with pytest.raises(ValueError, match="disagrees"):
        bitstream.read(_with_crc(bytes(long[:-4])))
    with pytest.raises(ValueError, match="disagrees"):
        bitstream.read(blob + b"\0")
    bad = bytearray(blob)
    bad[33] ^= 0x10                                                                                 # inside input_db
    with pytest.raises(ValueError, match="CRC"):
        bitstream.read(bytes(bad))


def test_bit3_is_still_an_unknown_flag():
    blob = bytearray(bitstream.write(dict(HEAD, input_db=-20.0), None, bytes(15)))
    blob[9] |= 8
    with pytest.raises(ValueError, match="unknown flags"):
        bitstream.read(_with_crc(bytes(blob[:-4])))


# ---------------------------------------------------------------------------------------------------------------- the C entries
def _kw_desc(**kw):
    d = _lib.KweightDesc()
    fake = 0x10000                                   # never dereferenced: every case below is refused before a launch
    d.x, d.e, d.ws = fake, fake, fake
    d.x_bs, d.e_bs, d.B, d.T, d.S, d.offset = 4800, 2, 1, 4800, 2400, 0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_c_entries_refuse_bad_arguments_without_a_gpu():
    """Error code and message, before any launch.  `lens` itself lives on the device and is clamped there, like every lens of
    this ABI; what the host can refuse is a negative LENGTH argument (T, n_samples)."""
    lib = _lib.load()
    P = ctypes.c_void_p
    fake = P(0x10000)

    def err():
        return lib.fac_last_error()

    assert lib.fac_kweight_energy(None, None) == -1 and b"null descriptor" in err()
    for kw, msg in ((dict(x=None), b"null pointer"), (dict(e=None), b"null pointer"), (dict(ws=None), b"null pointer"),
                    (dict(B=0), b"B = 0"), (dict(B=-3), b"B = -3"), (dict(S=0), b"S = 0"), (dict(S=-1), b"S = -1"),
                    (dict(S=100), b"below the chunk"), (dict(T=-1), b"T = -1"), (dict(offset=2400), b"offset"),
                    (dict(offset=-1), b"offset"), (dict(state_out=0x10000, lens=0x10000), b"state_out needs lens == NULL")):
        assert lib.fac_kweight_energy(ctypes.byref(_kw_desc(**kw)), None) == -1, kw
        assert msg in err(), (kw, err())
    assert lib.fac_kweight_ws_bytes(0, 100) == -1 and lib.fac_kweight_ws_bytes(1, -1) == -1
    chunk, group = lib.fac_loudness_chunk(0), lib.fac_loudness_chunk(1)
    assert (chunk, group) == (256, 64)
    # states, segment starts, partial sums (6 + 4 / 64 doubles per chunk), one peak per segment
    n_chunks = -(-72000 // chunk)
    n_seg = -(-n_chunks // group)
    assert lib.fac_kweight_ws_bytes(4, 72000) >= 4 * 8 * (6 * n_chunks + 4 * n_seg) + 4 * 4 * n_seg

    def gate(e=fake, lens=None, n=4800, S=2400, last_n=0, peaks=None, n_peaks=0, L=fake, pk=None, B=1):
        return lib.fac_loudness_gate(e, 2, lens, n, S, last_n, peaks, n_peaks, L, pk, B, None)

    for kw, msg in ((dict(e=None), b"null pointer"), (dict(L=None), b"null pointer"), (dict(B=0), b"B = 0"), (dict(B=-1), b"B = -1"),
                    (dict(S=0), b"S = 0"), (dict(n=-5), b"negative length"), (dict(last_n=-1), b"last_n"),
                    (dict(peaks=fake, n_peaks=1), b"come together"), (dict(peaks=fake, n_peaks=0, pk=fake), b"come together")):
        assert gate(**kw) == -1, kw
        assert msg in err(), (kw, err())

    def gain(x=fake, L=fake, peak=fake, guard=1, y=fake, B=1, T=4800):
        return lib.fac_loudness_gain(x, 4800, None, L, peak, None, -16.0, guard, y, 4800, None, B, T, None)

    for kw, msg in ((dict(x=None), b"null pointer"), (dict(y=None), b"null pointer"), (dict(L=None), b"null pointer"),
                    (dict(peak=None), b"needs peak"), (dict(B=0), b"B = 0"), (dict(T=-1), b"negative length")):
        assert gain(**kw) == -1, kw
        assert msg in err(), (kw, err())


def test_desc_layout_matches_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "facodec_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", '
                   "sizeof(fac_kweight_desc), offsetof(fac_kweight_desc, x_bs), offsetof(fac_kweight_desc, B), "
                   "offsetof(fac_kweight_desc, coef), offsetof(fac_kweight_desc, pw));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(repo, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    k = _lib.KweightDesc
    assert [int(v) for v in out] == [ctypes.sizeof(k), k.x_bs.offset, k.B.offset, k.coef.offset, k.pw.offset]


# ---------------------------------------------------------------------------------------------------------------- the reference itself
def test_reference_reads_the_standards_tone():
    """The restated arithmetic on the calibration signal: 2 s of 997 Hz at amplitude 0.5 and 24 kHz read -2.9843 - 6.0206."""
    t = np.arange(48000) / 24000.0
    x = 0.5 * np.sin(2.0 * math.pi * 997.0 * t)
    assert abs(loudness_ref(x) - (-2.9843 + 20.0 * math.log10(0.5))) <= 0.01
    assert loudness_ref(np.zeros(24000)) == -70.0 and loudness_ref(np.zeros(0)) == -70.0
    assert gain_ref(-70.0, -16.0, 0.0) == 1.0 and gain_ref(-26.0, -16.0, 0.99) == 1.0 / 0.99
    assert abs(gain_ref(-26.0, -16.0, 0.1) - 10.0 ** 0.5) < 1e-15
