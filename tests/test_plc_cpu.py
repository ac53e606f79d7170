"""Surviving packet loss without a device: the b"FQ" packet against a big-integer definition, LossyPacketReader,
the numpy float32 restatement of the fac_plc_select / fac_plc_gain state machines (which tests/test_plc.py holds the kernels to,
bit for bit) and its properties, the ctypes mirrors of the two new descriptors, and the host-side refusals."""
import ctypes
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from facodec_amd import _lib, bitstream

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIMARY, REDUNDANT, LOST = 0, 1, 2
POLICIES = [(2, 6, 1), (0, 1, 1), (1, 3, 3)]


# ------------------------------------------------------------------------------ the definitions the tests hold the code to
def pack_ref(codes, bits):
    """codes: int array (Q, F) -> the normative payload (include/facodec_hip.h): one big integer, little-endian."""
    codes = np.asarray(codes)
    Q, F = codes.shape
    N = 0
    for t in range(F):
        for q in range(Q):
            N |= (int(codes[q, t]) & ((1 << bits) - 1)) << (bits * (t * Q + q))
    return N.to_bytes((F * Q * bits + 7) // 8, "little")


def fq_ref(seq, codes, prev_red, n_red, bits):
    """The b"FQ" packet of one stream from the definition: codes (Q, k) of this push, prev_red (R, k_prev) the previous push's
    leading quantizers or None."""
    k = codes.shape[1]
    k_prev = 0 if prev_red is None else prev_red.shape[1]
    body = b"FQ" + struct.pack("<HHH", seq & 0xFFFF, k, k_prev) + bytes(n_red) + pack_ref(codes, bits)
    if k_prev:
        body += pack_ref(prev_red, bits)
    return body + struct.pack("<I", zlib.crc32(body))


def red_rows(codes3, n_red):
    """[p (n_p, k), c, r] -> the (R, k) rows of the redundant layer: the leading n_red[r] quantizers of each RVQ."""
    return np.concatenate([np.asarray(c)[:n] for c, n in zip(codes3, n_red)], 0)


class PlcRef:
    """numpy restatement of fac_plc_select's state machine (include/facodec_hip.h); float32 throughout, one rounding per op."""

    def __init__(self, B, n_q, hold=2, fade=6, recover=1):
        self.B, self.n_q, self.Q = B, tuple(n_q), sum(n_q)
        self.hold, self.fade, self.recover = hold, fade, recover
        self.last_codes = np.zeros((B, self.Q), np.int64)
        self.last_n = np.zeros((B, 3), np.int32)
        self.g = np.ones(B, np.float32)
        self.run = np.zeros(B, np.int32)

    def select(self, prim, red, n_red, status):
        """prim: three (B, n_q[r], k) arrays; red: three (B, n_red[r], k) or None -> (dst three arrays, n_use (B, k, 3), ramp)."""
        B, n_q = self.B, self.n_q
        k = next(p.shape[-1] for p, n in zip(prim, n_q) if n)
        n_red = tuple(n_red) if red is not None else (0, 0, 0)
        dst = [np.zeros((B, n, k), np.int64) for n in n_q]
        n_use = np.zeros((B, k, 3), np.int32)
        ramp = np.zeros((B, k + 1), np.float32)
        down, up = np.float32(1.0) / np.float32(self.fade), np.float32(1.0) / np.float32(self.recover)
        offs = [0, n_q[0], n_q[0] + n_q[1]]
        for b in range(B):
            st = int(status[b])
            if st != PRIMARY and not (st == REDUNDANT and sum(n_red)):
                st = LOST
            for r in range(3):
                for i in range(n_q[r]):
                    j = offs[r] + i
                    if st == LOST:
                        dst[r][b, i] = self.last_codes[b, j]
                    elif st == PRIMARY or i < n_red[r]:
                        dst[r][b, i] = (prim if st == PRIMARY else red)[r][b, i]
                        self.last_codes[b, j] = dst[r][b, i, k - 1]
            if st != LOST:
                self.last_n[b] = n_q if st == PRIMARY else n_red
            n_use[b] = self.last_n[b]
            g, run = self.g[b], int(self.run[b])
            ramp[b, 0] = g
            for f in range(k):
                if st == LOST:
                    run += 1
                    if run > self.hold:
                        g = max(np.float32(0.0), np.float32(g - down))
                else:
                    run = 0
                    g = min(np.float32(1.0), np.float32(g + up))
                ramp[b, f + 1] = g
            self.g[b], self.run[b] = g, run
        return dst, n_use, ramp


def gain_ref(wave, ramp, frame=300):
    """wave (B, k * frame) float32, ramp (B, k + 1) -> wave * gain with fac_plc_gain's operation order, one float32 rounding each."""
    wave = np.asarray(wave, np.float32)
    B, k = ramp.shape[0], ramp.shape[1] - 1
    t = (np.arange(1, frame + 1, dtype=np.float32) / np.float32(frame)).astype(np.float32)
    r0, r1 = ramp[:, :-1, None].astype(np.float32), ramp[:, 1:, None].astype(np.float32)
    d = (r1 - r0).astype(np.float32)
    gain = (r0 + (d * t[None, None, :]).astype(np.float32)).astype(np.float32)
    return (wave.reshape(B, k, frame) * gain).astype(np.float32).reshape(wave.shape)


# ------------------------------------------------------------------------------ packets
def test_fq_round_trip_field_by_field():
    rng = np.random.default_rng(0)
    n_q, n_red, bits, k, k_prev = (1, 2, 3), (1, 2, 0), 10, 5, 3
    codes = rng.integers(0, 1024, (6, k))
    prev = rng.integers(0, 1024, (3, k_prev))
    pay, red = pack_ref(codes, bits), pack_ref(prev, bits)
    blob = bitstream.write_packet_fec(0x1234, k, pay, k_prev, n_red, red)
    assert blob == fq_ref(0x1234, codes, prev, n_red, bits)
    assert blob[0:2] == b"FQ"
    assert int.from_bytes(blob[2:4], "little") == 0x1234
    assert int.from_bytes(blob[4:6], "little") == k
    assert int.from_bytes(blob[6:8], "little") == k_prev
    assert tuple(blob[8:11]) == n_red
    assert blob[11:11 + len(pay)] == pay and len(pay) == bitstream.payload_bytes(k, 6, bits) == 38
    assert blob[11 + len(pay):-4] == red and len(red) == bitstream.payload_bytes(k_prev, 3, bits) == 12
    assert int.from_bytes(blob[-4:], "little") == zlib.crc32(blob[:-4])
    assert len(blob) == bitstream.FEC_OVERHEAD + 38 + 12 and bitstream.FEC_OVERHEAD == 15 == bitstream.PACKET_OVERHEAD + 5
    p = bitstream.read_packet_fec(blob, n_q, bits)
    assert p == bitstream.Packet(0x1234, k, pay, k_prev, n_red, red)
    # seq wraps, the first push carries no redundant payload
    first = bitstream.write_packet_fec(65536 + 7, k, pay, 0, n_red, b"")
    p = bitstream.read_packet_fec(first, n_q, bits)
    assert (p.seq, p.n_red_frames, p.n_red, p.red_payload) == (7, 0, n_red, b"")
    assert first == fq_ref(7, codes, None, n_red, bits)


def test_bitrate_with_the_redundant_share():
    assert bitstream.bitrate((1, 2, 3), 10) == 4800                                  # as before
    assert bitstream.bitrate((1, 2, 3), 10, redundancy=(1, 2, 0)) == 4800 + 2400
    assert bitstream.bitrate(6, 10, redundancy=3) == 7200
    assert bitstream.bitrate((1, 2, 3), 10, redundancy=None) == 4800


def _reseal(body):
    return body + struct.pack("<I", zlib.crc32(body))


def test_read_packet_fec_refuses_each_corruption():
    n_q, n_red, bits = (1, 2, 3), (1, 2, 0), 10
    pay, red = bytes(range(38)), bytes(range(12))
    good = bitstream.write_packet_fec(3, 5, pay, 3, n_red, red)
    bitstream.read_packet_fec(good, n_q, bits)
    for cut in (0, 5, 14):
        with pytest.raises(ValueError, match="truncated"):
            bitstream.read_packet_fec(good[:cut], n_q, bits)
    with pytest.raises(ValueError, match="CRC"):
        bitstream.read_packet_fec(good[:-5], n_q, bits)                              # cut behind the header: the CRC no longer fits
    with pytest.raises(ValueError, match="magic"):
        bitstream.read_packet_fec(_reseal(b"FP" + good[2:-4]), n_q, bits)
    flipped = bytearray(good)
    flipped[20] ^= 0x40
    with pytest.raises(ValueError, match="CRC"):
        bitstream.read_packet_fec(bytes(flipped), n_q, bits)
    with pytest.raises(ValueError, match="payload bytes"):                         # primary payload one byte short
        bitstream.read_packet_fec(bitstream.write_packet_fec(3, 5, pay[:-1], 3, n_red, red), n_q, bits)
    with pytest.raises(ValueError, match="payload bytes"):                         # redundant payload one byte long
        bitstream.read_packet_fec(bitstream.write_packet_fec(3, 5, pay, 3, n_red, red + b"\0"), n_q, bits)
    with pytest.raises(ValueError, match="payload bytes"):                         # redundant payload missing altogether
        bitstream.read_packet_fec(bitstream.write_packet_fec(3, 5, pay, 3, n_red, b""), n_q, bits)
    with pytest.raises(ValueError, match="payload bytes"):                         # n_frames disagrees with the bytes
        bitstream.read_packet_fec(bitstream.write_packet_fec(3, 6, pay, 3, n_red, red), n_q, bits)
    with pytest.raises(ValueError, match="payload bytes"):                         # another layout handed in
        bitstream.read_packet_fec(good, (1, 2, 2), bits)
    for bad in ((2, 2, 0), (1, 3, 0), (1, 2, 4)):                                    # n_red beyond the layout handed in
        with pytest.raises(ValueError, match="within n_q"):
            bitstream.read_packet_fec(bitstream.write_packet_fec(3, 5, pay, 3, bad, red), n_q, bits)
    with pytest.raises(ValueError, match="no quantizers"):
        bitstream.read_packet_fec(bitstream.write_packet_fec(3, 5, pay, 3, (0, 0, 0), b""), n_q, bits)
    with pytest.raises(ValueError):
        bitstream.write_packet_fec(0, 70000, b"")
    with pytest.raises(ValueError):
        bitstream.write_packet_fec(0, 1, b"", 0, (1, 2))


def test_packetizer_host_part_without_redundancy_writes_the_packets_of_before():
    from facodec_amd.streaming import CodePacketizer
    rng = np.random.default_rng(1)
    tx = CodePacketizer((1, 2, 3))
    assert tx.redundancy is None
    for j, k in enumerate((10, 5, 3)):
        rows = rng.integers(0, 256, (2, 4 * ((bitstream.payload_bytes(k, 6, 10) + 3) // 4)), dtype=np.uint8)
        n = bitstream.payload_bytes(k, 6, 10)
        assert tx._emit(k, rows) == [bitstream.write_packet(j, k, rows[b, :n].tobytes()) for b in range(2)]


def test_packetizer_host_part_with_redundancy_carries_the_previous_push():
    from facodec_amd.streaming import CodePacketizer
    rng = np.random.default_rng(2)
    n_q, n_red, bits = (1, 2, 3), (1, 2, 0), 10
    tx = CodePacketizer(n_q, redundancy=n_red)
    prev = [None, None]
    for j, k in enumerate((10, 5, 3, 3)):
        codes = [[rng.integers(0, 1024, (n, k)) for n in n_q] for _ in range(2)]
        allq = [np.concatenate(c, 0) for c in codes]
        red = [red_rows(c, n_red) for c in codes]
        rows = np.stack([np.frombuffer(pack_ref(a, bits).ljust(80, b"\0"), np.uint8) for a in allq])
        rrows = np.stack([np.frombuffer(pack_ref(a, bits).ljust(40, b"\0"), np.uint8) for a in red])
        got = tx._emit(k, rows, rrows)
        assert got == [fq_ref(j, allq[b], prev[b], n_red, bits) for b in range(2)]
        assert all(bitstream.read_packet_fec(p, n_q, bits).n_red_frames == (0 if j == 0 else prev[0].shape[1]) for p in got)
        prev = red
    for bad in ((2, 2, 0), (0, 0, 0), (1, 2)):
        with pytest.raises(ValueError):
            CodePacketizer(n_q, redundancy=bad)


def test_lossy_reader_judges_every_stream_on_its_own():
    n_q, bits, k = (1, 2, 3), 10, 2
    pay = bytes(range(bitstream.payload_bytes(k, 6, bits)))
    red = bytes(range(bitstream.payload_bytes(k, 3, bits)))
    fp = lambda seq: bitstream.write_packet(seq, k, pay)
    fq = lambda seq: bitstream.write_packet_fec(seq, k, pay, k, (1, 2, 0), red)
    rd = bitstream.LossyPacketReader(4, n_q, bits, first_seq=65534)
    got = rd.feed([fp(65534), None, fq(65534), fq(65534)[:-1]])                      # good FP, missing, good FQ, corrupt
    assert got[0] == bitstream.Packet(65534, k, pay, 0, (0, 0, 0), b"")
    assert got[1] is None and got[3] is None
    assert got[2] == bitstream.Packet(65534, k, pay, k, (1, 2, 0), red)
    got = rd.feed([fp(65535), fp(65534), b"", b"XX" + fq(65535)[2:]])                # good, stale seq, empty, wrong magic
    assert got[0].seq == 65535 and got[1:] == [None, None, None]
    got = rd.feed([fq(0), fq(65536), fp(1), fq(0)])                                  # 65535 -> 0 wrap; a packet from the future
    assert [None if g is None else g.seq for g in got] == [0, 0, None, 0]
    got = rd.feed([None] * 4)                                                        # everything lost: still no exception
    assert got == [None] * 4 and rd.expected == 2
    assert rd.received == [3, 1, 1, 1]
    assert rd.corrupt == [0, 0, 1, 2]
    assert rd.misordered == [0, 1, 1, 0]
    with pytest.raises(ValueError):
        rd.feed([None] * 3)
    with pytest.raises(ValueError):
        bitstream.LossyPacketReader(1, (0, 0, 0), 10)


# ------------------------------------------------------------------------------ the restatement's properties
def _ramp_run(policy, statuses, k=1, B=1):
    ref = PlcRef(B, (1, 2, 3), *policy)
    prim = [np.zeros((B, n, k), np.int64) for n in (1, 2, 3)]
    red = [np.zeros((B, n, k), np.int64) for n in (1, 2, 0)]
    out = [np.float32(1.0)]
    for st in statuses:
        _, _, ramp = ref.select(prim, red, (1, 2, 0), [st] * B)
        assert ramp[0, 0] == out[-1]                                                 # a push starts where the last one ended
        out += list(ramp[0, 1:])
    return np.array(out, np.float32), ref


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("k", [1, 3])
def test_ramp_holds_fades_to_exact_zero_and_recovers(policy, k):
    hold, fade, recover = policy
    n_lost = -(-(hold + fade + 3) // k)
    ramp, ref = _ramp_run(policy, [LOST] * n_lost, k)
    assert np.all(np.diff(ramp) <= 0)                                                # non-increasing under loss
    assert np.all(ramp[:hold + 1] == np.float32(1.0))                                # exactly flat for `hold` frames
    if hold + 1 < len(ramp):
        assert ramp[hold + 1] < 1.0
    assert np.all(ramp[hold + fade + 1:] == 0.0) and ramp[hold + fade + 1].tobytes() == np.float32(0).tobytes()
    assert int(ref.run[0]) == n_lost * k
    # back at exactly 1.0 within recover + 1 received frames, from any state reached on the way down
    for n in range(0, n_lost + 1):
        for st in (PRIMARY, REDUNDANT):
            r2, ref2 = _ramp_run(policy, [LOST] * n + [st] * (recover + 1), 1)
            assert np.all(r2[n + recover + 1:] == np.float32(1.0)), (n, st)
            assert np.all(np.diff(r2[n:]) >= 0) and int(ref2.run[0]) == 0
    # a never-lost row is 1.0 everywhere
    r3, _ = _ramp_run(policy, [PRIMARY] * 7, k)
    assert np.all(r3 == np.float32(1.0))


def test_default_policy_is_25_ms_hold_and_75_ms_fade():
    import inspect
    from facodec_amd.streaming import StreamingReceiver
    sig = inspect.signature(StreamingReceiver.__init__).parameters
    assert (sig["hold"].default, sig["fade"].default, sig["recover"].default, sig["delay"].default) == (2, 6, 1, 0)
    ramp, _ = _ramp_run((2, 6, 1), [LOST] * 10)
    step = np.float32(1.0) / np.float32(6)
    want = [np.float32(1.0)] * 3
    for _ in range(6):
        want.append(max(np.float32(0), np.float32(want[-1] - step)))
    assert list(ramp[:9]) == want and ramp[9] == 0.0


def test_select_restatement_substitutes_and_keeps_state():
    rng = np.random.default_rng(3)
    n_q, n_red, B, k = (1, 2, 3), (1, 2, 0), 4, 3
    ref = PlcRef(B, n_q)
    prim = [rng.integers(0, 1024, (B, n, k)) for n in n_q]
    dst, n_use, _ = ref.select(prim, None, (0, 0, 0), [PRIMARY] * B)
    assert all(np.array_equal(d, p) for d, p in zip(dst, prim)) and np.all(n_use == np.array(n_q))
    last = np.concatenate([p[:, :, -1] for p in prim], 1)
    assert np.array_equal(ref.last_codes, last)
    prim2 = [rng.integers(0, 1024, (B, n, k)) for n in n_q]
    red2 = [rng.integers(0, 1024, (B, n, k)) for n in n_red]
    dst, n_use, ramp = ref.select(prim2, red2, n_red, [PRIMARY, REDUNDANT, LOST, 7])
    assert np.array_equal(dst[1][0], prim2[1][0]) and np.array_equal(dst[1][1], red2[1][1]) and np.all(dst[2][1] == 0)
    for b in (2, 3):                                                                 # LOST and an unknown status: the last frame repeated
        assert np.array_equal(np.concatenate([d[b] for d in dst], 0), np.repeat(last[b][:, None], k, 1))
    assert n_use[:, 0].tolist() == [[1, 2, 3], [1, 2, 0], [1, 2, 3], [1, 2, 3]]
    assert ref.last_n.tolist() == [[1, 2, 3], [1, 2, 0], [1, 2, 3], [1, 2, 3]]
    assert np.array_equal(ref.last_codes[1, :3], np.concatenate([r[1, :, -1] for r in red2])) and np.array_equal(ref.last_codes[1, 3:], last[1, 3:])
    assert np.array_equal(ref.last_codes[2], last[2])
    assert ramp[:2].tolist() == [[1.0] * (k + 1)] * 2 and ref.run.tolist() == [0, 0, 3, 3]
    # REDUNDANT without a redundant layer counts as LOST
    dst, n_use, _ = ref.select(prim2, None, (0, 0, 0), [REDUNDANT] * B)
    assert np.array_equal(dst[0][0], np.repeat(prim2[0][0][:, -1:], k, 1)) and ref.run[0] == 3


def test_gain_restatement_is_exact_for_a_flat_ramp():
    rng = np.random.default_rng(4)
    wave = rng.standard_normal((2, 900)).astype(np.float32)
    ramp = np.ones((2, 4), np.float32)
    ramp[1] = [1.0, 0.5, 0.0, 0.0]
    out = gain_ref(wave, ramp)
    assert out[0].tobytes() == wave[0].tobytes()
    assert np.all(out[1, 600:] == 0) and out[1, 299] == np.float32(wave[1, 299] * np.float32(0.5))


# ------------------------------------------------------------------------------ the C ABI, without a device
def test_new_desc_layouts_match_the_header(tmp_path):
    """ctypes mirrors of fac_vq_decode_masked_desc and fac_plc_select_desc have the size and field offsets gcc gives the header's
    structs."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    mf = [n for n, _ in _lib.VqDecodeMaskedDesc._fields_]
    pf = [n for n, _ in _lib.PlcSelectDesc._fields_]
    prints = ['printf("%zu\\n", sizeof(fac_vq_decode_masked_desc));'] + [f'printf("%zu\\n", offsetof(fac_vq_decode_masked_desc, {f}));' for f in mf]
    prints += ['printf("%zu\\n", sizeof(fac_plc_select_desc));'] + [f'printf("%zu\\n", offsetof(fac_plc_select_desc, {f}));' for f in pf]
    prints += ['printf("%d %d %d %d\\n", FAC_PLC_MAX_FRAMES, FAC_PLC_PRIMARY, FAC_PLC_REDUNDANT, FAC_PLC_LOST);']
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "facodec_hip.h"\nint main(){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    M, P = _lib.VqDecodeMaskedDesc, _lib.PlcSelectDesc
    want = [ctypes.sizeof(M)] + [getattr(M, f).offset for f in mf] + [ctypes.sizeof(P)] + [getattr(P, f).offset for f in pf]
    assert out == want + [_lib.PLC_MAX_FRAMES, _lib.PLC_PRIMARY, _lib.PLC_REDUNDANT, _lib.PLC_LOST]
    assert M.base.offset == 0 and ctypes.sizeof(M) == ctypes.sizeof(_lib.VqDecodeDesc) + 24


FAKE = 0x10000                                   # never dereferenced: every check below fails on the host


def _err(lib):
    return lib.fac_last_error()


def test_masked_decode_refuses_bad_descriptors_before_any_launch():
    lib = _lib.load()
    assert lib.fac_vq_decode_masked(None, None) == -1 and b"null descriptor" in _err(lib)
    d = _lib.VqDecodeMaskedDesc()
    assert lib.fac_vq_decode_masked(ctypes.byref(d), None) == -1 and b"null pointer" in _err(lib)
    d.base.style, d.base.outs = FAKE, FAKE
    d.base.B, d.base.D, d.base.T, d.base.Kc = 2, 1024, 4, 1024
    d.base.n_q[0] = 2
    assert lib.fac_vq_decode_masked(ctypes.byref(d), None) == -1 and b"no codes" in _err(lib)
    d.base.n_q[0] = -1
    assert lib.fac_vq_decode_masked(ctypes.byref(d), None) == -1 and b"negative" in _err(lib)
    for r in range(3):
        d.base.codes[r] = FAKE
    d.base.n_q[0], d.base.n_q[1], d.base.n_q[2] = 2, 10, 5
    assert lib.fac_vq_decode_masked(ctypes.byref(d), None) == -1 and b"at most 16" in _err(lib)
    d.base.n_q[1], d.base.n_q[2] = 0, 0
    assert lib.fac_vq_decode_masked(ctypes.byref(d), None) == -1 and b"null weight" in _err(lib)
    for q in range(2):
        d.base.codebook[q], d.base.w_out[q], d.base.b_out[q] = FAKE, FAKE, FAKE
    d.n_use = FAKE
    for bs, ts in ((0, 3), (12, 0), (-12, 3), (0, 0)):                               # strides that cannot address (2, 4, 3)
        d.n_use_bs, d.n_use_ts = bs, ts
        assert lib.fac_vq_decode_masked(ctypes.byref(d), None) == -1 and b"cannot address" in _err(lib), (bs, ts)
    d.n_use_bs, d.n_use_ts = 12, 3
    d.base.D = 1 << 20
    assert lib.fac_vq_decode_masked(ctypes.byref(d), None) == -1 and b"do not fit LDS" in _err(lib)


def _good_select():
    d = _lib.PlcSelectDesc()
    for r, (n, nr) in enumerate(zip((1, 2, 3), (1, 2, 0))):
        d.prim[r], d.red[r], d.dst[r] = FAKE, (FAKE if nr else None), FAKE
        d.n_q[r], d.n_red[r] = n, nr
    d.status = d.last_codes = d.last_n = d.g = d.run = d.n_use = d.ramp = FAKE
    d.n_use_bs, d.n_use_ts = 48, 3
    d.B, d.k, d.hold, d.fade, d.recover = 2, 16, 2, 6, 1
    return d


@pytest.mark.parametrize("field,value,msg", [
    ("status", None, b"null status or state"), ("last_codes", None, b"null status or state"), ("last_n", None, b"null status or state"),
    ("g", None, b"null status or state"), ("run", None, b"null status or state"),
    ("n_use", None, b"null n_use or ramp"), ("ramp", None, b"null n_use or ramp"),
    ("B", 0, b"B = 0"), ("k", 0, b"k = 0"), ("k", 17, b"k = 17"),
    ("hold", -1, b"policy"), ("fade", 0, b"policy"), ("recover", 0, b"policy"),
    ("n_use_bs", 0, b"cannot address"), ("n_use_ts", 0, b"cannot address"),
])
def test_plc_select_refuses_bad_descriptors_before_any_launch(field, value, msg):
    lib = _lib.load()
    d = _good_select()
    setattr(d, field, value)
    assert lib.fac_plc_select(ctypes.byref(d), None) == -1 and msg in _err(lib)


def test_plc_select_and_gain_refuse_bad_counts_and_shapes():
    lib = _lib.load()
    assert lib.fac_plc_select(None, None) == -1 and b"null descriptor" in _err(lib)
    d = _good_select()
    d.n_red[2] = 4
    assert lib.fac_plc_select(ctypes.byref(d), None) == -1 and b"4 redundant quantizers but 3 primary" in _err(lib)
    d = _good_select()
    d.n_q[1] = -1
    assert lib.fac_plc_select(ctypes.byref(d), None) == -1 and b"negative" in _err(lib)
    d = _good_select()
    d.n_q[2] = 14
    assert lib.fac_plc_select(ctypes.byref(d), None) == -1 and b"17 quantizers" in _err(lib)
    d = _good_select()
    d.n_q[0] = d.n_q[1] = d.n_q[2] = d.n_red[0] = d.n_red[1] = 0
    assert lib.fac_plc_select(ctypes.byref(d), None) == -1 and b"0 quantizers" in _err(lib)
    for name, msg in (("prim", b"no primary or destination"), ("dst", b"no primary or destination"), ("red", b"no redundant codes")):
        d = _good_select()
        getattr(d, name)[1] = None
        assert lib.fac_plc_select(ctypes.byref(d), None) == -1 and msg in _err(lib), name
    g = lib.fac_plc_gain
    assert g(None, 300, FAKE, 300, FAKE, 1, 1, 300, None) == -1 and b"null pointer" in _err(lib)
    assert g(FAKE, 300, None, 300, FAKE, 1, 1, 300, None) == -1 and b"null pointer" in _err(lib)
    assert g(FAKE, 300, FAKE, 300, None, 1, 1, 300, None) == -1 and b"null pointer" in _err(lib)
    for B, k, frame in ((0, 1, 300), (1, 0, 300), (1, 1, 0)):
        assert g(FAKE, 300, FAKE, 300, FAKE, B, k, frame, None) == -1 and b"bad shape" in _err(lib)
    assert g(FAKE, 599, FAKE, 600, FAKE, 2, 2, 300, None) == -1 and b"row pitches" in _err(lib)
    assert g(FAKE, 600, FAKE, 599, FAKE, 2, 2, 300, None) == -1 and b"row pitches" in _err(lib)
    assert g(FAKE, 1 << 40, FAKE, 1 << 40, FAKE, 65536, 16, 4096, None) == -1 and b"below 2^31" in _err(lib)
