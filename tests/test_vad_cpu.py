"""Voice activity, SID packets and the DTX state machines without a device: the numpy fp64 restatement of
fac_vad_energy / fac_vad_decide (which tests/test_vad.py holds the kernels to, bit for bit) and its properties, a scripted
noise-and-bursts signal, the SID packets field by field, the sender's and the receiver's host state machines, the ctypes mirrors
of the new descriptors and the host-side refusals."""
import ctypes
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from facodec_amd import _lib, bitstream
from facodec_amd.streaming import CodePacketizer, dtx_row, dtx_step

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WH = [(1, 0), (4, 3), (120, 16)]
MARGIN = 10.0 ** (6.0 / 10.0)


# ------------------------------------------------------------------------------ the definitions the tests hold the code to
def energy_ref(x, frame, length=None):
    """x (T,) float32 -> E (ceil(T / frame),) float64 in fac_vad_energy's order: d[n] = x[n] - 0.97 x[n - 1] (x[-1] = 0), lane l of
    64 adds d[n]^2 over n = l, l + 64, ... of the frame in increasing n from 0.0, then the butterfly over 32, 16, 8, 4, 2, 1.
    length: samples at and behind it do not exist."""
    x = np.asarray(x, np.float32)
    T = len(x) if length is None else max(0, min(int(length), len(x)))
    xd = x.astype(np.float64)
    d = xd - np.float64(0.97) * np.concatenate([[0.0], xd[:-1]])
    p = d * d
    F = -(-len(x) // frame)
    E = np.zeros(F, np.float64)
    lane_ids = np.arange(64)
    for f in range(F):
        seg = p[f * frame:min((f + 1) * frame, T)]
        lanes = np.zeros(64, np.float64)
        for j in range(0, len(seg), 64):
            chunk = seg[j:j + 64]
            lanes[:len(chunk)] = lanes[:len(chunk)] + chunk
        for dist in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[lane_ids ^ dist]
        E[f] = lanes[0]
    return E


def raw_ref(E, W, margin, thr_abs):
    E = np.asarray(E, np.float64)
    raw = np.zeros(len(E), bool)
    for f in range(len(E)):
        N = E[max(0, f - W + 1):f + 1].min()
        raw[f] = E[f] > thr_abs and E[f] > np.float64(margin) * N
    return raw


def hang_ref(raw, H):
    return np.array([raw[max(0, f - H):f + 1].any() for f in range(len(raw))], bool)


def decide_ref(E, W, H, margin, thr_abs, n_row=None):
    """E (F,) float64 -> flags (F,) uint8 by fac_vad_decide's definition; n_row: frames at or past it are 0."""
    act = hang_ref(raw_ref(E, W, margin, thr_abs), H)
    if n_row is not None:
        act[n_row:] = False
    return act.astype(np.uint8)


def vad_ref(x, frame=300, W=120, H=16, margin=MARGIN, thr_abs=None, length=None):
    thr_abs = frame * 10.0 ** (-70.0 / 10.0) if thr_abs is None else thr_abs
    E = energy_ref(x, frame, length)
    n_row = None if length is None else -(-max(0, int(length)) // frame)
    return decide_ref(E, W, H, margin, thr_abs, n_row), E


# ------------------------------------------------------------------------------ properties of the restatement
def test_energy_order_is_lanes_then_butterfly_not_a_plain_sum():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(905) * 0.1).astype(np.float32)
    E = energy_ref(x, 300)
    assert E.shape == (4,)
    xd = x.astype(np.float64)
    d = xd - 0.97 * np.concatenate([[0.0], xd[:-1]])
    exact = [float(np.sum((d * d)[f * 300:(f + 1) * 300])) for f in range(4)]
    assert np.allclose(E, exact, rtol=1e-13, atol=0)
    short = energy_ref(x, 300, length=301)
    assert short[0] == E[0] and short[2] == 0 and short[3] == 0 and short[1] == (d[300] * d[300])
    # one sample per frame: E is d^2, the butterfly adds zeros
    assert np.array_equal(energy_ref(x[:7], 1), (d * d)[:7])


@pytest.mark.parametrize("W,H", WH)
def test_constant_level_gives_no_active_frame(W, H):
    assert not decide_ref(np.full(400, 0.37), W, H, MARGIN, 3e-5).any()
    flags, E = vad_ref(np.full(300 * 40, 0.25, np.float32), W=W, H=H)                 # DC: frame 0 is the loudest, the rest equal
    assert E[0] > E[1] and np.all(E[1:] == E[1]) and not flags.any()


@pytest.mark.parametrize("W,H", WH)
def test_frame_zero_is_never_active(W, H):
    rng = np.random.default_rng(W * 100 + H)
    for _ in range(50):
        E = 10.0 ** rng.uniform(-8, 2, 30)
        assert decide_ref(E, W, H, MARGIN, 3e-5)[0] == 0
    assert decide_ref(np.array([1e9]), W, H, MARGIN, 0.0)[0] == 0


@pytest.mark.parametrize("W,H", WH)
def test_an_isolated_raw_frame_gives_exactly_hangover_plus_one_active_frames(W, H):
    for j in (1, 7, 150):
        raw = np.zeros(400, bool)
        raw[j] = True
        act = hang_ref(raw, H)
        assert act.sum() == H + 1 and act[j:j + H + 1].all()
        E = np.ones(400)
        E[j] = 100.0
        flags = decide_ref(E, W, H, MARGIN, 3e-5)
        if W == 1:                                   # N[f] = E[f]: no frame can exceed margin > 1 times itself
            assert not flags.any()
        else:                                        # the frames after the peak are no louder than the floor: not raw
            assert raw_ref(E, W, MARGIN, 3e-5).tolist() == raw.tolist()
            assert flags.sum() == H + 1 and flags[j:j + H + 1].all()


@pytest.mark.parametrize("W,H", WH)
def test_flags_depend_on_nothing_older_than_window_plus_hangover(W, H):
    rng = np.random.default_rng(W + 7 * H)
    F = 2 * (W + H) + 40
    E = 10.0 ** rng.uniform(-6, 0, F)
    base = decide_ref(E, W, H, MARGIN, 3e-5)
    for f in (W + H, W + H + 13, F - 1):
        other = E.copy()
        other[:f - (W + H) + 1] = 10.0 ** rng.uniform(-6, 0, f - (W + H) + 1)     # everything older than the W + H frames up to f
        assert np.array_equal(decide_ref(other, W, H, MARGIN, 3e-5)[f:], base[f:])
    if W > 1:                                       # ... and the oldest frame inside does matter
        f = W + H + 5
        E = np.ones(F)
        E[f + H] = 3.0                              # 3 < margin * 1: not raw on a floor of 1, raw on a floor of 0.5
        inside, outside = E.copy(), E.copy()
        inside[f + H - W + 1] = 0.5                 # the oldest frame of the window of frame f + H ...
        outside[f + H - W] = 0.5                    # ... and the one before it
        assert decide_ref(E, W, H, MARGIN, 3e-5)[f + H] == 0 and decide_ref(outside, W, H, MARGIN, 3e-5)[f + H] == 0
        got = decide_ref(inside, W, H, MARGIN, 3e-5)
        assert got[f + H:f + 2 * H + 1].all() and got[f + 2 * H + 1] == 0


BURSTS = [(130, 140), (200, 203), (260, 300)]       # frames [a, b) at -20 dBFS in -60 dBFS noise; 420 frames in all


def _scripted():
    rng = np.random.default_rng(20)
    x = rng.standard_normal(420 * 300) * 1e-3
    for a, b in BURSTS:                             # a burst ends one sample short of its last frame: x[n] - 0.97 x[n - 1] carries
        n = (b - a) * 300 - 1                       # the burst's last sample one sample on, and that stays in the burst's frame
        x[a * 300:a * 300 + n] = rng.standard_normal(n) * 1e-1
    return x.astype(np.float32)


@pytest.mark.parametrize("W,H", [(120, 16), (4, 3)])
def test_scripted_noise_and_bursts(W, H):
    """White noise at -60 dBFS (seed 20) with three bursts at -20 dBFS: the active set is the bursts' frames plus H frames each,
    for the defaults (120, 16) and, with only the bursts up to W - 1 = 3 frames long counted on, for (4, 3).  Measured on the
    CPU with the defaults: the quietest burst frame is 34.0 dB above margin * N (a factor 2500), the loudest noise frame
    3.7 dB below it (a factor 0.427), and every noise frame is 11.6 dB or more above thr_abs (a factor 14.6) -- so the decision
    is the margin's alone, and no frame sits near it."""
    x = _scripted()
    thr = 300 * 10.0 ** -7.0
    flags, E = vad_ref(x, W=W, H=H)
    bursts = [(a, b) for a, b in BURSTS if b - a < W]
    want = np.zeros(420, bool)
    for a, b in bursts:
        want[a:b + H] = True
    if W == 4:                                      # a burst of W frames or more raises its own floor: only its first W - 1 are raw
        for a, b in BURSTS:
            if b - a >= W:
                want[a:a + W - 1 + H] = True
    assert np.array_equal(flags.astype(bool), want)
    if W == 120:
        ratio = np.array([E[f] / (MARGIN * E[max(0, f - W + 1):f + 1].min()) for f in range(420)])
        inb = np.zeros(420, bool)
        for a, b in BURSTS:
            inb[a:b] = True
        print("burst min ratio", ratio[inb].min(), "noise max ratio", ratio[~inb].max(), "noise min E / thr", (E[~inb] / thr).min())
        assert ratio[inb].min() > 1.0 > ratio[~inb].max() and (E[~inb] / thr).min() > 1.0


# ------------------------------------------------------------------------------ SID packets
def test_sid_packets_differ_in_one_byte_and_the_crc():
    pay, red = bytes(range(38)), bytes(range(100, 112))
    for plain, sid, magic, smagic in (
            (bitstream.write_packet(0x1234, 5, pay), bitstream.write_packet(0x1234, 5, pay, sid=True), b"FP", b"Fp"),
            (bitstream.write_packet_fec(0x1234, 5, pay, 3, (1, 2, 0), red), bitstream.write_packet_fec(0x1234, 5, pay, 3, (1, 2, 0), red, sid=True),
             b"FQ", b"Fq")):
        assert len(plain) == len(sid) and plain[:2] == magic and sid[:2] == smagic
        assert sid[0] == plain[0] and sid[1] == plain[1] | 0x20                     # the second letter in lower case
        assert sid[2:-4] == plain[2:-4]                                               # seq, n_frames, (n_red_frames, n_red,) payloads
        assert [i for i in range(len(plain) - 4) if plain[i] != sid[i]] == [1]
        assert int.from_bytes(sid[-4:], "little") == zlib.crc32(sid[:-4]) != int.from_bytes(plain[-4:], "little")
    assert bitstream.write_packet(7, 5, pay, sid=False) == bitstream.write_packet(7, 5, pay)
    assert bitstream.write_packet_fec(7, 5, pay, 3, (1, 2, 0), red, sid=False) == bitstream.write_packet_fec(7, 5, pay, 3, (1, 2, 0), red)


def test_plain_readers_refuse_sid_packets_and_the_lossy_reader_reads_them_with_dtx():
    n_q, bits, k = (1, 2, 3), 10, 5
    pay = bytes(range(bitstream.payload_bytes(k, 6, bits)))
    red = bytes(range(bitstream.payload_bytes(3, 3, bits)))
    fp, fps = bitstream.write_packet(0, k, pay), bitstream.write_packet(0, k, pay, sid=True)
    fq, fqs = bitstream.write_packet_fec(0, k, pay, 3, (1, 2, 0), red), bitstream.write_packet_fec(0, k, pay, 3, (1, 2, 0), red, sid=True)
    with pytest.raises(ValueError, match="wrong magic"):
        bitstream.read_packet(fps, 6, bits)
    with pytest.raises(ValueError, match="wrong magic"):
        bitstream.read_packet_fec(fqs, n_q, bits)
    with pytest.raises(ValueError, match="wrong magic"):
        bitstream.read_packet(fqs, 6, bits)
    assert bitstream.read_packet(fp, 6, bits) == (0, k, pay)
    # dtx off: SID packets are corrupt, exactly as an unknown magic is
    rd = bitstream.LossyPacketReader(4, n_q, bits)
    assert rd.feed([fp, fps, fqs, b"ZZ" + fp[2:]])[1:] == [None, None, None]
    assert rd.corrupt == [0, 1, 1, 1] and rd.received == [1, 0, 0, 0]
    # dtx on: all four parse; the packet is the plain one's with sid set
    rd = bitstream.LossyPacketReader(4, n_q, bits, dtx=True)
    got = rd.feed([fp, fps, fq, fqs])
    assert rd.corrupt == [0] * 4 and rd.received == [1] * 4
    assert got[0] == bitstream.Packet(0, k, pay, 0, (0, 0, 0), b"") and got[0].sid is False
    assert got[1] == got[0]._replace(sid=True)
    assert got[2] == bitstream.Packet(0, k, pay, 3, (1, 2, 0), red, False) and got[3] == got[2]._replace(sid=True)
    assert bitstream.Packet._fields[-1] == "sid"
    bad = bytearray(fps)
    bad[8] ^= 1
    assert rd.feed([bytes(bad), None, None, None]) == [None] * 4 and rd.corrupt[0] == 1            # the CRC still covers a SID packet


def test_bitrate_under_dtx():
    assert bitstream.bitrate((1, 2, 3), 10) == 4800 and isinstance(bitstream.bitrate((1, 2, 3), 10), int)
    assert bitstream.bitrate((1, 2, 3), 10, dtx_silence=0.0) == 4800.0
    assert bitstream.bitrate((1, 2, 3), 10, dtx_silence=0.5) == 4800 * (0.5 + 0.5 / 8)
    assert bitstream.bitrate((1, 2, 3), 10, redundancy=(1, 2, 0), dtx_silence=1.0, sid_every=4) == 7200 / 4
    with pytest.raises(ValueError):
        bitstream.bitrate(6, 10, dtx_silence=1.5)
    with pytest.raises(ValueError):
        bitstream.bitrate(6, 10, dtx_silence=0.5, sid_every=0)


# ------------------------------------------------------------------------------ the sender's host machine
def _kind(p):
    return None if p is None else {b"FP": "n", b"FQ": "n", b"Fp": "s", b"Fq": "s"}[p[:2]]


def _want_kinds(active, sid_every):
    out, silent = [], 0
    for a in active:
        if a:
            silent = 0
            out.append("n")
        else:
            silent += 1
            out.append("s" if (silent - 1) % sid_every == 0 else None)
    return out


@pytest.mark.parametrize("sid_every", [1, 3, 8])
@pytest.mark.parametrize("red", [None, (1, 2, 0)])
def test_sender_emits_normal_sid_and_none_by_the_rule(sid_every, red):
    rng = np.random.default_rng(sid_every)
    n_q, bits, k, B, n = (1, 2, 3), 10, 6, 3, 40
    pattern = np.zeros((n, B, k), np.uint8)
    pattern[:, 0] = 1                                                               # stream 0 speaks throughout
    pattern[:12, 1, 2] = 1                                                          # stream 1: one active frame per push, then silence
    pattern[25, 1, 5] = 1                                                           # ... and one push in between
    pattern[20:, 2] = rng.integers(0, 2, (n - 20, k))                               # stream 2 starts silent
    pattern[30:33, 2] = 0
    tx = CodePacketizer(n_q, bits=bits, redundancy=red, dtx=dict(sid_every=sid_every))
    ref = CodePacketizer(n_q, bits=bits, redundancy=red)
    n1 = bitstream.payload_bytes(k, 6, bits)
    n2 = bitstream.payload_bytes(k, 3, bits)
    kinds = [[] for _ in range(B)]
    for j in range(n):
        rows = rng.integers(0, 256, (B, n1 + 3), dtype=np.uint8)
        rr = rng.integers(0, 256, (B, n2 + 1), dtype=np.uint8) if red else None
        got = tx._emit(k, rows, rr, pattern[j])
        plain = ref._emit(k, rows, rr)
        assert tx.seq == ref.seq == j + 1
        for b in range(B):
            kinds[b].append(_kind(got[b]))
            if got[b] is None:
                continue
            # what is sent is the packet that would have been sent -- seq, payload and the previous push's redundant layer, also
            # across suppressed pushes -- with at most the magic's case and the CRC changed
            assert got[b][2:-4] == plain[b][2:-4] and got[b][:2].upper() == plain[b][:2]
            assert int.from_bytes(got[b][2:4], "little") == j
            assert int.from_bytes(got[b][-4:], "little") == zlib.crc32(got[b][:-4])
            if kinds[b][-1] == "n":
                assert got[b] == plain[b]
    for b in range(B):
        assert kinds[b] == _want_kinds(pattern[:, b].any(axis=1), sid_every), b
    assert kinds[0] == ["n"] * n and kinds[2][0] == "s"
    if sid_every == 8:
        assert kinds[1][12:25] == ["s"] + [None] * 7 + ["s"] + [None] * 4 and kinds[1][25:28] == ["n", "s", None]
    if sid_every == 1:
        assert None not in kinds[1] + kinds[2]


def test_sender_refuses_flags_without_dtx_and_bad_dtx():
    tx = CodePacketizer((1, 2, 3))
    rows = np.zeros((2, 40), np.uint8)
    with pytest.raises(ValueError, match="without dtx"):
        tx._emit(5, rows, None, np.ones((2, 5), np.uint8))
    with pytest.raises(ValueError, match="without dtx"):
        tx.active_view(2, 5, "cpu")
    with pytest.raises(ValueError, match="sid_every"):
        CodePacketizer((1, 2, 3), dtx=dict(sid_every=0))
    with pytest.raises(ValueError, match="sid_every"):
        CodePacketizer((1, 2, 3), dtx=dict(every=3))
    # dtx set, no flags given: every push counts as active
    tx = CodePacketizer((1, 2, 3), dtx=dict())
    assert tx.sid_every == 8 and tx._emit(5, rows) == CodePacketizer((1, 2, 3))._emit(5, rows)


# ------------------------------------------------------------------------------ the receiver's host machine
def _walk(events, k=4, sid_timeout=24):
    row, out = dtx_row(), []
    for ev in events:
        word, comfort = dtx_step(row, ev, k, sid_timeout)
        out.append((word & 0xFF, (word >> 8) & 0xFF, (word >> 16) & 0xFF, comfort, row["in_dtx"]))
    return out


def test_receiver_host_machine():
    PASS, STORE, FILL = _lib.SID_PASS, _lib.SID_STORE, _lib.SID_FILL
    # a lost first SID: nothing arrives and the row is not in DTX -> concealment; DTX is entered at the refresh
    got = _walk(["normal", None, None, "sid", None, None, "normal", None])
    assert [g[0] for g in got] == [PASS, PASS, PASS, STORE, FILL, FILL, PASS, PASS]
    assert [g[3] for g in got] == [False, False, False, False, True, True, False, False]
    assert [g[4] for g in got] == [False, False, False, True, True, True, False, False]
    assert got[3][2] == 4                                                            # STORE carries sid_k = k
    # the phase walks through the stored frames: k = 4 comfort frames per push out of sid_k = 3 stored ones
    row = dtx_row()
    dtx_step(row, "sid", 3)
    phases = []
    for _ in range(5):
        word, comfort = dtx_step(row, None, 4)
        assert comfort and word & 0xFF == FILL and (word >> 16) & 0xFF == 3
        phases.append((word >> 8) & 0xFF)
    assert phases == [0, 1, 2, 0, 1]
    # a refresh restarts the count and the phase; the redundant layer leaves the state alone
    got = _walk(["sid"] + [None] * 3 + ["sid"] + [None] * 3 + ["redundant", None], sid_timeout=3)
    assert [g[3] for g in got] == [False, True, True, True, False, True, True, True, False, False]
    assert got[5][1] == 0 and got[8][4] is True and got[9][4] is False              # timed out at the last event
    # the timeout: sid_timeout comfort pushes, then the row leaves DTX and stays out until the next SID packet
    got = _walk(["sid"] + [None] * 6, sid_timeout=4)
    assert [g[3] for g in got] == [False, True, True, True, True, False, False]
    assert [g[4] for g in got] == [True, True, True, True, True, False, False]
    assert _walk(["sid", None], sid_timeout=0)[1][3:] == (False, False)


# ------------------------------------------------------------------------------ the C ABI, without a device
def test_vad_desc_layouts_match_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    structs = [("fac_vad_energy_desc", _lib.VadEnergyDesc), ("fac_vad_decide_desc", _lib.VadDecideDesc), ("fac_sid_apply_desc", _lib.SidApplyDesc)]
    prints, want = [], []
    for name, S in structs:
        prints.append(f'printf("%zu\\n", sizeof({name}));')
        want.append(ctypes.sizeof(S))
        for f, _ in S._fields_:
            prints.append(f'printf("%zu\\n", offsetof({name}, {f}));')
            want.append(getattr(S, f).offset)
    prints.append('printf("%d %d %d %d %d\\n", FAC_VAD_MAX_FRAME, FAC_VAD_MAX_WINDOW, FAC_SID_PASS, FAC_SID_STORE, FAC_SID_FILL);')
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "facodec_hip.h"\nint main(){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == want + [_lib.VAD_MAX_FRAME, _lib.VAD_MAX_WINDOW, _lib.SID_PASS, _lib.SID_STORE, _lib.SID_FILL]


FAKE = 0x10000                                   # never dereferenced: every check below fails on the host


def _good_energy():
    d = _lib.VadEnergyDesc()
    d.carry_in, d.carry_out, d.x, d.e = FAKE, FAKE + 0x8000, FAKE, FAKE
    d.x_bs, d.e_bs, d.f0 = 480, 256, 0
    d.B, d.k, d.frame, d.carry_n, d.is_final, d.R = 2, 480, 300, 10, 0, 256
    return d


@pytest.mark.parametrize("field,value,msg", [
    ("x", None, b"null block or energy"), ("e", None, b"null block or energy"),
    ("B", 0, b"B = 0"), ("B", 65536, b"B = 65536"), ("frame", 0, b"frame = 0"), ("frame", 4097, b"frame = 4097"), ("k", 0, b"k = 0"),
    ("carry_n", -1, b"carry_n = -1"), ("carry_n", 300, b"carry_n = 300"), ("carry_in", None, b"without a carry buffer"),
    ("carry_out", FAKE, b"carry_out is carry_in"), ("lens", FAKE, b"lens does not go"),
    ("x_bs", 479, b"x_bs = 479"), ("e_bs", 255, b"e_bs = 255"), ("f0", -1, b"f0 = -1"), ("R", 0, b"R = 0"),
])
def test_vad_energy_refuses_bad_descriptors_before_any_launch(field, value, msg):
    lib = _lib.load()
    d = _good_energy()
    setattr(d, field, value)
    assert lib.fac_vad_energy(ctypes.byref(d), None) == -1 and msg in lib.fac_last_error(), lib.fac_last_error()


def _good_decide():
    d = _lib.VadDecideDesc()
    d.e, d.flags, d.ring = FAKE, FAKE, FAKE
    d.e_bs, d.flags_bs, d.ring_bs, d.f0 = 256, 8, 256, 1000
    d.margin, d.thr_abs = 3.98, 3e-5
    d.B, d.n_new, d.R, d.W, d.H, d.frame = 2, 8, 256, 120, 16, 300
    return d


@pytest.mark.parametrize("field,value,msg", [
    ("e", None, b"null energy"), ("B", 0, b"B = 0"), ("n_new", 0, b"n_new = 0"),
    ("W", 0, b"W = 0"), ("W", 2049, b"W = 2049"), ("H", -1, b"H = -1"), ("H", 2049, b"H = 2049"),
    ("margin", 1.0, b"margin = 1"), ("thr_abs", -1.0, b"thr_abs"), ("f0", -1, b"f0 = -1"), ("frame", 0, b"frame = 0"),
    ("R", 143, b"R = 143 below W + H + n_new"), ("R", 0, b"R = 0"),
    ("e_bs", 255, b"e_bs = 255"), ("flags_bs", 7, b"flags_bs = 7"), ("ring_bs", 255, b"ring_bs = 255"),
])
def test_vad_decide_refuses_bad_descriptors_before_any_launch(field, value, msg):
    lib = _lib.load()
    d = _good_decide()
    setattr(d, field, value)
    assert lib.fac_vad_decide(ctypes.byref(d), None) == -1 and msg in lib.fac_last_error(), lib.fac_last_error()


def test_vad_entries_refuse_null_descriptors_and_the_rest():
    lib = _lib.load()
    assert lib.fac_vad_energy(None, None) == -1 and b"null descriptor" in lib.fac_last_error()
    assert lib.fac_vad_decide(None, None) == -1 and b"null descriptor" in lib.fac_last_error()
    assert lib.fac_sid_apply(None, None) == -1 and b"null descriptor" in lib.fac_last_error()
    d = _good_decide()
    d.flags = d.ring = None
    assert lib.fac_vad_decide(ctypes.byref(d), None) == -1 and b"neither flags nor a flag ring" in lib.fac_last_error()
    # a ring that has not wrapped yet holds every frame: R = F is enough for the offline call, one frame less is not
    d = _good_decide()
    d.f0, d.n_new, d.R, d.e_bs, d.ring_bs, d.flags_bs = 0, 100, 99, 100, 100, 100
    assert lib.fac_vad_decide(ctypes.byref(d), None) == -1 and b"below W + H + n_new" in lib.fac_last_error()
    t = lib.fac_vad_take
    assert t(None, 8, 8, 0, 4, FAKE, 4, 1, None) == -1 and b"null pointer" in lib.fac_last_error()
    assert t(FAKE, 8, 8, 0, 4, None, 4, 1, None) == -1 and b"null pointer" in lib.fac_last_error()
    for B, k, R in ((0, 4, 8), (1, 0, 8), (1, 4, 0)):
        assert t(FAKE, 8, R, 0, k, FAKE, 4, B, None) == -1 and b"bad shape" in lib.fac_last_error()
    assert t(FAKE, 8, 8, 0, 9, FAKE, 9, 1, None) == -1 and b"do not lie in a ring" in lib.fac_last_error()
    assert t(FAKE, 8, 8, -1, 4, FAKE, 4, 1, None) == -1 and b"do not lie in a ring" in lib.fac_last_error()
    assert t(FAKE, 7, 8, 0, 4, FAKE, 4, 2, None) == -1 and b"row pitches" in lib.fac_last_error()
    assert t(FAKE, 8, 8, 0, 4, FAKE, 3, 2, None) == -1 and b"row pitches" in lib.fac_last_error()


def _good_sid():
    d = _lib.SidApplyDesc()
    for r, n in enumerate((1, 2, 3)):
        d.dst[r], d.dst_bs[r], d.dst_qs[r], d.n_q[r] = FAKE, 16 * n, 16, n
    d.mode = d.sid_codes = FAKE
    d.B, d.k = 2, 16
    return d


def test_sid_apply_refuses_bad_descriptors_before_any_launch():
    lib = _lib.load()
    for field, value, msg in (("mode", None, b"null mode or code store"), ("sid_codes", None, b"null mode or code store"),
                              ("B", 0, b"B = 0"), ("k", 0, b"k = 0"), ("k", 17, b"k = 17")):
        d = _good_sid()
        setattr(d, field, value)
        assert lib.fac_sid_apply(ctypes.byref(d), None) == -1 and msg in lib.fac_last_error(), field
    d = _good_sid()
    d.n_q[1] = -1
    assert lib.fac_sid_apply(ctypes.byref(d), None) == -1 and b"negative" in lib.fac_last_error()
    d = _good_sid()
    d.dst[2] = None
    assert lib.fac_sid_apply(ctypes.byref(d), None) == -1 and b"no codes" in lib.fac_last_error()
    d = _good_sid()
    d.n_q[2] = 14
    assert lib.fac_sid_apply(ctypes.byref(d), None) == -1 and b"17 quantizers" in lib.fac_last_error()
    d = _good_sid()
    d.n_q[0] = d.n_q[1] = d.n_q[2] = 0
    assert lib.fac_sid_apply(ctypes.byref(d), None) == -1 and b"0 quantizers" in lib.fac_last_error()
    for name, idx, value in (("dst_bs", 0, 0), ("dst_qs", 1, 15)):
        d = _good_sid()
        getattr(d, name)[idx] = value
        assert lib.fac_sid_apply(ctypes.byref(d), None) == -1 and b"cannot address" in lib.fac_last_error(), name


def test_python_surface_refuses_bad_parameters():
    from facodec_amd import ops
    assert ops.vad_params() == (300, 120, 16, 10.0 ** 0.6, 300 * 10.0 ** -7.0)
    for kw in (dict(frame=0), dict(frame=4097), dict(window=0), dict(hangover=-1), dict(margin_db=0.0), dict(window=2049)):
        with pytest.raises(ValueError):
            ops.vad_params(**kw)
    from facodec_amd.commons import active_segments
    assert active_segments([0, 1, 1, 0, 0, 1], 300, 1700) == [(300, 900), (1500, 1700)]
    assert active_segments([0, 0], 300, 600) == [] and active_segments([1], 300, 7) == [(0, 7)]
