"""The bitstream without a GPU: the packed layout's fixed vectors against the big-integer definition, the
container (facodec_amd/bitstream.py) field by field and refusal by refusal, the packet framing, and the host-side refusals and
struct layouts of fac_codes_pack / fac_codes_unpack.

The independent reference is `bigint_payload` below: include/facodec_hip.h's definition written with Python integers."""
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


def bigint_payload(rows, bits):
    """rows: Q sequences of F codes in quantizer order (prosody, content, residual rows) -> the payload bytes."""
    Q, F = len(rows), len(rows[0])
    N = 0
    for t in range(F):
        for q in range(Q):
            N |= (int(rows[q][t]) & ((1 << bits) - 1)) << (bits * (t * Q + q))
    return N.to_bytes((F * Q * bits + 7) // 8, "little")


# ------------------------------------------------------------------------------------------------ layout
def test_fixed_vectors():
    one = [[1], [2], [3], [4], [5], [1023]]
    assert bigint_payload(one, 10) == bytes.fromhex("01083000010 5fc0f".replace(" ", ""))
    two = [[1, 512], [2, 0], [3, 1], [4, 1000], [5, 7], [1023, 341]]
    got = bigint_payload(two, 10)
    assert len(got) == 15 and got == bytes.fromhex("010830000105fc0f200001a07f4055")
    assert got[:7] == bigint_payload(one, 10)[:7]              # whole frames are self-contained bit ranges (60 bits: 7.5 bytes)


def test_payload_bytes_and_bitrate():
    assert bitstream.bitrate((1, 2, 3), 10) == 4800
    assert bitstream.bitrate((1, 2, 0), 10) == 2400 and bitstream.bitrate(6, 10, frame_rate=80) == 4800
    assert bitstream.payload_bytes(160, 6, 10) == 1200
    assert bitstream.payload_bytes(1, 6, 10) == 8 and bitstream.payload_bytes(2, 6, 10) == 15
    assert bitstream.payload_bytes(3, 1, 1) == 1 and bitstream.payload_bytes(9, 1, 1) == 2
    for k in (1, 2, 8, 13):
        assert bitstream.payload_bytes(k, 6, 10) == -(-60 * k // 8)


def test_row_bytes_helper():
    lib = _lib.load()
    for T, Q, bits in ((1, 6, 10), (2, 6, 10), (160, 6, 10), (3, 1, 1), (53, 16, 16), (1000, 5, 7), (40_000_000, 16, 16)):
        pb = (T * Q * bits + 7) // 8
        assert lib.fac_codes_row_bytes(T, Q, bits) == 4 * ((pb + 3) // 4)
    assert lib.fac_codes_row_bytes(0, 6, 10) == -1


# ------------------------------------------------------------------------------------------------ container
def _fields(**kw):
    f = dict(bits=10, n_q=(1, 2, 3), sample_rate=16000, n_frames=160, n_samples=31999, codebook_size=1024)
    f.update(kw)
    return f


def _blob(with_timbre=True, **kw):
    rng = np.random.default_rng(5)
    f = _fields(**kw)
    payload = rng.integers(0, 256, bitstream.payload_bytes(f["n_frames"], sum(f["n_q"]), f["bits"]), dtype=np.uint8).tobytes()
    timbre = rng.standard_normal(1024).astype(np.float32) if with_timbre else None
    return bitstream.write(f, timbre.tobytes() if with_timbre else None, payload), timbre, payload


def test_container_round_trip():
    blob, timbre, payload = _blob(True)
    assert len(blob) == 32 + 4096 + 1200 + 4
    assert blob[:4] == b"FACB" and blob[4] == 1
    assert struct.unpack("<I", blob[-4:])[0] == zlib.crc32(blob[:-4])
    hdr, tim, pl = bitstream.read(blob)
    assert (hdr.version, hdr.bits, hdr.n_p, hdr.n_c, hdr.n_r) == (1, 10, 1, 2, 3)
    assert (hdr.flags, hdr.timbre_dim, hdr.sample_rate, hdr.n_frames, hdr.n_samples, hdr.codebook_size) == (1, 1024, 16000, 160, 31999, 1024)
    assert hdr.n_q == (1, 2, 3) and hdr.Q == 6 and hdr.has_timbre and not hdr.is_stream_header
    assert tim.dtype == np.float32 and np.array_equal(tim, timbre) and pl == payload
    # the documented offsets
    assert struct.unpack_from("<H", blob, 10)[0] == 1024 and struct.unpack_from("<IIIII", blob, 12) == (16000, 160, 31999, 1024, 0)
    assert blob[5] == 10 and tuple(blob[6:9]) == (1, 2, 3) and blob[9] == 1
    assert blob[32:32 + 4096] == timbre.tobytes() and blob[32 + 4096:-4] == payload


def test_container_without_timbre_and_stream_header():
    blob, _, payload = _blob(False, n_q=(1, 1, 0), bits=11, n_frames=7, timbre_dim=1024)
    assert len(blob) == 32 + bitstream.payload_bytes(7, 2, 11) + 4
    hdr, tim, pl = bitstream.read(blob)
    assert tim is None and pl == payload and hdr.flags == 0 and hdr.timbre_dim == 1024 and hdr.n_q == (1, 1, 0) and hdr.bits == 11
    head = bitstream.write(_fields(n_frames=0, n_samples=0, stream=True), np.arange(4, dtype=np.float32), b"")
    hdr, tim, pl = bitstream.read(head)
    assert hdr.is_stream_header and hdr.has_timbre and hdr.flags == 3 and hdr.n_frames == 0 and pl == b"" and list(tim) == [0, 1, 2, 3]
    with pytest.raises(ValueError, match="payload"):
        bitstream.write(_fields(), None, bytes(1199))
    with pytest.raises(ValueError, match="bits"):
        bitstream.write(_fields(bits=17), None, bytes(10))


def _flip(blob, i):
    return blob[:i] + bytes([blob[i] ^ 0x10]) + blob[i + 1:]


def test_read_refuses_each_corruption():
    blob, _, _ = _blob(True)
    with pytest.raises(ValueError, match="magic"):
        bitstream.read(b"FACX" + blob[4:])
    with pytest.raises(ValueError, match="magic"):
        bitstream.read(_flip(blob, 0))
    with pytest.raises(ValueError, match="version 2"):
        bitstream.read(blob[:4] + b"\x02" + blob[5:])
    with pytest.raises(ValueError, match="truncated"):
        bitstream.read(blob[:-1])
    with pytest.raises(ValueError, match="truncated"):
        bitstream.read(blob[:20])
    with pytest.raises(ValueError, match="truncated"):
        bitstream.read(b"")
    with pytest.raises(ValueError, match="disagrees with the header"):
        bitstream.read(blob + b"\x00")
    with pytest.raises(ValueError, match="CRC"):
        bitstream.read(_flip(blob, 21))                       # header: n_samples (informational, only the CRC notices)
    with pytest.raises(ValueError, match="CRC"):
        bitstream.read(_flip(blob, 32 + 100))                 # timbre
    with pytest.raises(ValueError, match="CRC"):
        bitstream.read(_flip(blob, 32 + 4096 + 600))          # payload
    with pytest.raises(ValueError, match="CRC"):
        bitstream.read(_flip(blob, len(blob) - 2))            # the CRC itself
    with pytest.raises(ValueError, match="reserved"):
        bitstream.read(_flip(blob, 29))
    for i in range(32):                                      # any flipped header byte is refused, whatever the cause
        with pytest.raises(ValueError):
            bitstream.read(_flip(blob, i))
    # a reserved word that a writer set, with a matching CRC, is still refused
    body = blob[:28] + struct.pack("<I", 7) + blob[32:-4]
    with pytest.raises(ValueError, match="reserved"):
        bitstream.read(body + struct.pack("<I", zlib.crc32(body)))


# ------------------------------------------------------------------------------------------------ packets
def _packets(seq, k, n_streams=2, Q=6, bits=10, seed=0):
    rng = np.random.default_rng(seed)
    pl = [rng.integers(0, 256, bitstream.payload_bytes(k, Q, bits), dtype=np.uint8).tobytes() for _ in range(n_streams)]
    return [bitstream.write_packet(seq, k, p) for p in pl], pl


def test_packet_framing():
    (pkt,), (pl,) = _packets(300, 8, n_streams=1)
    assert pkt[:2] == b"FP" and struct.unpack_from("<HH", pkt, 2) == (300, 8) and pkt[6:-4] == pl and len(pl) == 60
    assert struct.unpack("<I", pkt[-4:])[0] == zlib.crc32(pkt[:-4])
    assert bitstream.read_packet(pkt, 6, 10) == (300, 8, pl)
    with pytest.raises(ValueError, match="CRC"):
        bitstream.read_packet(_flip(pkt, 10), 6, 10)
    with pytest.raises(ValueError, match="CRC"):
        bitstream.read_packet(_flip(pkt, 3), 6, 10)
    with pytest.raises(ValueError, match="magic"):
        bitstream.read_packet(b"XP" + pkt[2:], 6, 10)
    with pytest.raises(ValueError, match="truncated"):
        bitstream.read_packet(pkt[:9], 6, 10)
    with pytest.raises(ValueError, match="payload"):
        bitstream.read_packet(pkt, 5, 10)                      # the stream header said otherwise


def test_packet_sequence_wrap_gap_and_disagreement():
    rd = bitstream.PacketReader(2, 6, 10, first_seq=65534)
    for seq, k in ((65534, 8), (65535, 1), (0, 2), (1, 8)):   # wraps 65535 -> 0
        pk, pl = _packets(seq, k, seed=seq)
        assert bitstream.write_packet(seq + 65536, k, pl[0]) == pk[0]     # the writer wraps too
        assert rd.feed(pk) == (k, pl)
    assert rd.expected == 2
    pk, pl = _packets(5, 8)                                   # 2, 3, 4 never arrived
    with pytest.raises(bitstream.PacketLoss) as e:
        rd.feed(pk)
    assert e.value.missing == 3
    assert rd.feed(pk) == (8, pl) and rd.expected == 6        # resynchronised: the same packets are accepted now
    rd = bitstream.PacketReader(2, 6, 10, first_seq=65535)
    with pytest.raises(bitstream.PacketLoss) as e:
        rd.feed(_packets(1, 8)[0])                            # a gap across the wrap
    assert e.value.missing == 2
    rd = bitstream.PacketReader(2, 6, 10)
    pk, _ = _packets(0, 8)
    with pytest.raises(ValueError, match="CRC"):
        rd.feed([pk[0], _flip(pk[1], 20)])
    with pytest.raises(ValueError, match="n_frames"):
        rd.feed([pk[0], _packets(0, 7)[0][1]])
    with pytest.raises(ValueError, match="seq"):
        rd.feed([pk[0], _packets(1, 8)[0][1]])
    with pytest.raises(ValueError, match="2 streams"):
        rd.feed(pk[:1])
    assert rd.expected == 0 and rd.feed(pk)[0] == 8            # a refused feed consumes nothing


# ------------------------------------------------------------------------------------------------ C ABI, no launch
FAKE = 0x10000          # never dereferenced: every case below is refused before the launch


def _pack_desc(**kw):
    d = _lib.CodesPackDesc()
    for r, n in enumerate((1, 2, 3)):
        d.codes[r], d.codes_bs[r], d.codes_qs[r], d.n_q[r] = FAKE, n * 16, 16, n
    d.out, d.out_bs, d.B, d.T, d.bits = FAKE, 120, 2, 16, 10
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _unpack_desc(**kw):
    d = _lib.CodesUnpackDesc()
    for r, n in enumerate((1, 2, 3)):
        d.codes[r], d.codes_bs[r], d.codes_qs[r], d.n_q[r] = FAKE, n * 16, 16, n
    d.in_, d.in_bs, d.B, d.T, d.bits = FAKE, 120, 2, 16, 10
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _nq(d, *n):
    for r in range(3):
        d.n_q[r] = n[r]
    return d


def _null_codes(d, r):
    d.codes[r] = None
    return d


@pytest.mark.parametrize("which", ["pack", "unpack"])
def test_bad_descriptors_are_refused_before_any_launch(which):
    lib = _lib.load()
    make, fn, stride = (_pack_desc, lib.fac_codes_pack, "out_bs") if which == "pack" else (_unpack_desc, lib.fac_codes_unpack, "in_bs")
    cases = [
        (make(bits=0), b"bits"), (make(bits=17), b"bits"), (make(bits=-3), b"bits"),
        (_nq(make(), 0, 0, 0), b"quantizers"), (_nq(make(), 5, 6, 6), b"quantizers"), (_nq(make(), 1, -1, 3), b"quantizers"),
        (_null_codes(make(), 1), b"no codes"),
        (make(**{stride: 116}), b"too small"),                # 16 frames x 60 bits = 120 bytes
        (make(B=0), b"bad shape"), (make(T=0), b"bad shape"), (make(B=-1), b"bad shape"),
    ]
    if which == "pack":
        cases += [(make(out_bs=122), b"multiple of 4"), (make(out=None), b"null pointer")]
    else:
        cases += [(make(in_=None), b"null pointer")]
    for d, msg in cases:
        assert fn(ctypes.byref(d), None) == -1
        err = lib.fac_last_error()
        assert msg in err and (b"codes_" + which.encode()) in err, (msg, err)
    assert fn(None, None) == -1 and b"null descriptor" in lib.fac_last_error()


def test_codes_desc_layouts_match_the_header(tmp_path):
    """ctypes mirrors of the two descriptors have the size and field offsets gcc gives the header's structs."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    pf = ["codes", "codes_bs", "codes_qs", "n_q", "lens", "out", "out_bs", "B", "T", "bits"]
    uf = ["in", "in_bs", "codes", "codes_bs", "codes_qs", "n_q", "lens", "B", "T", "bits"]
    prints = ['printf("%zu\\n", sizeof(fac_codes_pack_desc));'] + [f'printf("%zu\\n", offsetof(fac_codes_pack_desc, {f}));' for f in pf]
    prints += ['printf("%zu\\n", sizeof(fac_codes_unpack_desc));'] + [f'printf("%zu\\n", offsetof(fac_codes_unpack_desc, {f}));' for f in uf]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "facodec_hip.h"\nint main(){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    p, u = _lib.CodesPackDesc, _lib.CodesUnpackDesc
    want = [ctypes.sizeof(p)] + [getattr(p, f).offset for f in pf]
    want += [ctypes.sizeof(u)] + [getattr(u, "in_" if f == "in" else f).offset for f in uf]
    assert out == want
