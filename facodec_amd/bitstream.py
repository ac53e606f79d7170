"""The codec's bitstream on the host: a self-describing container around one clip's packed codes, and the packets
of the streaming pair.  Host only -- struct and zlib.crc32, no torch and no device call: the payload is produced and consumed on
the device by ops.pack_codes / ops.unpack_codes (csrc/bitpack.hip), whose layout include/facodec_hip.h defines.

Container, everything little-endian:

     0  4s  b"FACB"          12  I  sample_rate (rate of the audio given to compress)
     4  B   version = 1      16  I  n_frames F
     5  B   bits             20  I  n_samples (original length at sample_rate; informational)
     6  3B  n_p, n_c, n_r    24  I  codebook_size
     9  B   flags (bit0: timbre present, bit1: stream header, bit2: input loudness present)
    10  H   timbre_dim       28  I  reserved = 0
    32      timbre, fp32 x timbre_dim (absent when bit0 = 0)
    ..  f   input_db, fp32: the integrated loudness (LUFS) the audio had before compress levelled it (absent when bit2 = 0)
    ..      payload, ceil(F Q bits / 8) bytes
    ..  I   CRC-32 of every preceding byte

Packet of one streaming push, per stream:  b"FP", seq uint16 (wrapping), n_frames uint16, payload ceil(n_frames Q bits / 8)
bytes, CRC-32 of every preceding byte.  What Q and bits are is the stream header's business (a container with flag bit1 and
F = 0, sent once per stream).  A lost packet is reported (PacketLoss), not concealed.
"""
import struct
import zlib
from collections import namedtuple

import numpy as np

MAGIC = b"FACB"
VERSION = 1
FLAG_TIMBRE, FLAG_STREAM, FLAG_LOUDNESS = 1, 2, 4
MAX_Q = 16                                   # FAC_VQ_DECODE_MAX_Q
_HEAD = struct.Struct("<4sBB3BBHIIIII")
HEADER_BYTES = _HEAD.size                    # 32
assert HEADER_BYTES == 32

PACKET_MAGIC = b"FP"
_PHEAD = struct.Struct("<2sHH")
PACKET_OVERHEAD = _PHEAD.size + 4            # 10 bytes around the payload


class Header(namedtuple("Header", "version bits n_p n_c n_r flags timbre_dim sample_rate n_frames n_samples codebook_size input_db",
                        defaults=(None,))):
    """input_db: the float32 behind the timbre when flag bit2 is set, else None."""
    __slots__ = ()

    @property
    def n_q(self):
        return (self.n_p, self.n_c, self.n_r)

    @property
    def Q(self):
        return self.n_p + self.n_c + self.n_r

    @property
    def has_timbre(self):
        return bool(self.flags & FLAG_TIMBRE)

    @property
    def is_stream_header(self):
        return bool(self.flags & FLAG_STREAM)

    @property
    def has_loudness(self):
        return bool(self.flags & FLAG_LOUDNESS)


class PacketLoss(Exception):
    """A gap in the packet sequence: `missing` packets were not seen before the one just fed."""

    def __init__(self, missing):
        super().__init__(f"{missing} packet(s) lost")
        self.missing = missing


def payload_bytes(F, Q, bits):
    """Bytes of the packed codes of F frames of Q quantizers at `bits` per code."""
    return (int(F) * int(Q) * int(bits) + 7) // 8


def bitrate(n_q, bits, frame_rate=80):
    """Payload bits per second for quantizer counts n_q = (n_p, n_c, n_r) (or their sum): Q * bits * frame_rate."""
    Q = sum(n_q) if isinstance(n_q, (tuple, list)) else int(n_q)
    return Q * bits * frame_rate


def _check_layout(bits, n_q, what):
    if not 1 <= bits <= 16:
        raise ValueError(f"{what}: bits = {bits} is outside 1..16")
    if len(n_q) != 3 or any(not 0 <= n <= MAX_Q for n in n_q) or not 1 <= sum(n_q) <= MAX_Q:
        raise ValueError(f"{what}: quantizer counts {tuple(n_q)} (three counts, 1..{MAX_Q} in all)")


def write(header_fields, timbre_bytes, payload):
    """One container blob.  header_fields: a mapping (or Header) with bits, n_p, n_c, n_r (or n_q = the three), sample_rate,
    n_frames, n_samples, codebook_size, optionally timbre_dim (else the timbre's length), stream (flag bit1) and input_db (a
    number: flag bit2 and one float32 behind the timbre; None or absent: neither, the blob of before); version, flags and the
    reserved word are written here.  timbre_bytes: timbre_dim float32 values as bytes (or a float32 array), or None.
    payload: exactly payload_bytes(n_frames, Q, bits) bytes."""
    h = header_fields._asdict() if isinstance(header_fields, Header) else dict(header_fields)
    n_q = tuple(h["n_q"]) if "n_q" in h else (h["n_p"], h["n_c"], h["n_r"])
    bits = int(h["bits"])
    _check_layout(bits, n_q, "bitstream.write")
    if timbre_bytes is not None and not isinstance(timbre_bytes, (bytes, bytearray, memoryview)):
        timbre_bytes = np.ascontiguousarray(timbre_bytes, dtype="<f4").tobytes()
    timbre_bytes = b"" if timbre_bytes is None else bytes(timbre_bytes)
    if len(timbre_bytes) % 4:
        raise ValueError(f"bitstream.write: a timbre of {len(timbre_bytes)} bytes is no whole number of float32 values")
    flags = (FLAG_TIMBRE if timbre_bytes else 0) | (FLAG_STREAM if h.get("stream") or h.get("flags", 0) & FLAG_STREAM else 0)
    loud = b""
    if h.get("input_db") is not None:
        flags |= FLAG_LOUDNESS
        loud = struct.pack("<f", float(h["input_db"]))
    dim = int(h.get("timbre_dim") or len(timbre_bytes) // 4)
    if timbre_bytes and len(timbre_bytes) != 4 * dim:
        raise ValueError(f"bitstream.write: timbre of {len(timbre_bytes) // 4} values, timbre_dim = {dim}")
    F = int(h["n_frames"])
    payload = bytes(payload)
    if len(payload) != payload_bytes(F, sum(n_q), bits):
        raise ValueError(f"bitstream.write: payload of {len(payload)} bytes, {F} frames x {sum(n_q)} x {bits} bits need "
                         f"{payload_bytes(F, sum(n_q), bits)}")
    body = _HEAD.pack(MAGIC, VERSION, bits, *n_q, flags, dim, int(h["sample_rate"]), F, int(h["n_samples"]),
                      int(h["codebook_size"]), 0) + timbre_bytes + loud + payload
    return body + struct.pack("<I", zlib.crc32(body))


def read(blob):
    """-> (Header, timbre float32 ndarray (timbre_dim,) or None, payload bytes).  ValueError naming the cause for: a wrong magic,
    a version other than 1, a truncated blob, a length that disagrees with the header, a CRC mismatch, a non-zero reserved word."""
    blob = bytes(blob)
    if len(blob) < 4 or blob[:4] != MAGIC:
        if len(blob) < 4 and MAGIC.startswith(blob):
            raise ValueError(f"bitstream: truncated blob ({len(blob)} bytes, the header alone has {HEADER_BYTES})")
        raise ValueError(f"bitstream: wrong magic {blob[:4]!r} (expected {MAGIC!r})")
    if len(blob) >= 5 and blob[4] != VERSION:
        raise ValueError(f"bitstream: version {blob[4]} (this reader knows version {VERSION})")
    if len(blob) < HEADER_BYTES + 4:
        raise ValueError(f"bitstream: truncated blob ({len(blob)} bytes, header and CRC alone have {HEADER_BYTES + 4})")
    _, version, bits, n_p, n_c, n_r, flags, dim, rate, F, n_samples, cb, reserved = _HEAD.unpack_from(blob)
    hdr = Header(version, bits, n_p, n_c, n_r, flags, dim, rate, F, n_samples, cb)
    if reserved != 0:
        raise ValueError(f"bitstream: reserved word is {reserved:#x}, not 0")
    if flags & ~(FLAG_TIMBRE | FLAG_STREAM | FLAG_LOUDNESS):
        raise ValueError(f"bitstream: unknown flags {flags:#x}")
    _check_layout(bits, hdr.n_q, "bitstream")
    n_t = (4 * dim if hdr.has_timbre else 0) + (4 if hdr.has_loudness else 0)
    n_p_bytes = payload_bytes(F, hdr.Q, bits)
    want = HEADER_BYTES + n_t + n_p_bytes + 4
    if len(blob) < want:
        raise ValueError(f"bitstream: truncated blob ({len(blob)} bytes, the header describes {want})")
    if len(blob) != want:
        raise ValueError(f"bitstream: length {len(blob)} disagrees with the header, which describes {want} bytes")
    crc, = struct.unpack_from("<I", blob, want - 4)
    if zlib.crc32(blob[:want - 4]) != crc:
        raise ValueError("bitstream: CRC mismatch (corrupt blob)")
    timbre = np.frombuffer(blob, dtype="<f4", count=dim, offset=HEADER_BYTES).copy() if hdr.has_timbre else None
    if hdr.has_loudness:
        hdr = hdr._replace(input_db=struct.unpack_from("<f", blob, HEADER_BYTES + n_t - 4)[0])
    return hdr, timbre, blob[HEADER_BYTES + n_t:want - 4]


# ------------------------------------------------------------------------------------ packets of the streaming pair
def write_packet(seq, n_frames, payload):
    """One push of one stream: b"FP", seq (taken modulo 65536), n_frames, payload, CRC-32."""
    if not 0 <= n_frames <= 0xFFFF:
        raise ValueError(f"packet: n_frames = {n_frames} does not fit 16 bits")
    body = _PHEAD.pack(PACKET_MAGIC, seq & 0xFFFF, n_frames) + bytes(payload)
    return body + struct.pack("<I", zlib.crc32(body))


def read_packet(blob, Q, bits):
    """-> (seq, n_frames, payload bytes).  ValueError for a short packet, a wrong magic, a CRC failure, or a payload whose
    length is not payload_bytes(n_frames, Q, bits)."""
    blob = bytes(blob)
    if len(blob) < PACKET_OVERHEAD:
        raise ValueError(f"packet: truncated ({len(blob)} bytes)")
    magic, seq, n_frames = _PHEAD.unpack_from(blob)
    if magic != PACKET_MAGIC:
        raise ValueError(f"packet: wrong magic {magic!r} (expected {PACKET_MAGIC!r})")
    crc, = struct.unpack_from("<I", blob, len(blob) - 4)
    if zlib.crc32(blob[:-4]) != crc:
        raise ValueError("packet: CRC mismatch (corrupt packet)")
    want = payload_bytes(n_frames, Q, bits)
    if len(blob) - PACKET_OVERHEAD != want:
        raise ValueError(f"packet: payload of {len(blob) - PACKET_OVERHEAD} bytes, {n_frames} frames x {Q} x {bits} bits need {want}")
    return seq, n_frames, blob[_PHEAD.size:-4]


class PacketReader:
    """Byte-level half of the receiver: one packet per stream and push in, the streams' payloads out, the sequence checked.

        rd = PacketReader(n_streams, Q, bits)
        n_frames, payloads = rd.feed(packets)

    ValueError: a corrupt packet, a wrong packet count, streams that disagree on seq or n_frames.  PacketLoss(missing): the
    packets' seq is `missing` ahead of the expected one (modulo 65536); the reader is then resynchronised to the packets just
    refused, so feeding them again accepts them -- what to play for the gap is the caller's decision (no concealment here)."""

    def __init__(self, n_streams, Q, bits, first_seq=0):
        self.n_streams, self.Q, self.bits = int(n_streams), int(Q), int(bits)
        self.expected = first_seq & 0xFFFF

    def feed(self, packets):
        packets = list(packets)
        if len(packets) != self.n_streams:
            raise ValueError(f"{len(packets)} packets for {self.n_streams} streams")
        parsed = [read_packet(p, self.Q, self.bits) for p in packets]
        seq, n_frames = parsed[0][0], parsed[0][1]
        if any(p[0] != seq for p in parsed):
            raise ValueError(f"the streams' packets disagree on seq: {[p[0] for p in parsed]}")
        if any(p[1] != n_frames for p in parsed):
            raise ValueError(f"the streams' packets disagree on n_frames: {[p[1] for p in parsed]}")
        missing = (seq - self.expected) & 0xFFFF
        if missing:
            self.expected = seq
            raise PacketLoss(missing)
        self.expected = (seq + 1) & 0xFFFF
        return n_frames, [p[2] for p in parsed]
