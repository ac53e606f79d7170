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

Packet with in-band redundancy, per stream:

     0  2s  b"FQ"             6  H   n_red_frames (0: no redundant payload, the first push)
     2  H   seq (wrapping)    8  3B  n_red = (rp, rc, rr), each <= the stream's n_q
     4  H   n_frames         11      primary payload, ceil(n_frames Q bits / 8) bytes
    ..      redundant payload, ceil(n_red_frames (rp + rc + rr) bits / 8) bytes: the PREVIOUS push's leading rp / rc / rr
            quantizers of the three RVQs, in the same normative layout (frame-major, quantizer order, LSB-first)
    ..  I   CRC-32 of every preceding byte

LossyPacketReader reads both kinds per stream and never raises for a loss; what is played for one is StreamingReceiver's business.

SID packet: "silence follows".  It is the packet that would have been sent with the second magic byte in lower
case -- b"Fp" for the b"FP" layout, b"Fq" for b"FQ" -- and nothing else changed (the CRC covers the body, so it differs too).
read_packet / read_packet_fec refuse it like any unknown magic; LossyPacketReader(dtx=True) reads all four.
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


def bitrate(n_q, bits, frame_rate=80, redundancy=None, dtx_silence=None, sid_every=8):
    """Payload bits per second for quantizer counts n_q = (n_p, n_c, n_r) (or their sum): Q * bits * frame_rate.  redundancy =
    (rp, rc, rr) (or their sum) adds the share of the in-band redundant copy: (Q + R) * bits * frame_rate.  dtx_silence = the
    fraction of pushes without an active frame under discontinuous transmission: of those only one in sid_every
    is sent, so the rate (then a float) is that times (1 - dtx_silence) + dtx_silence / sid_every."""
    Q = sum(n_q) if isinstance(n_q, (tuple, list)) else int(n_q)
    if redundancy is not None:
        Q += sum(redundancy) if isinstance(redundancy, (tuple, list)) else int(redundancy)
    rate = Q * bits * frame_rate
    if dtx_silence is None:
        return rate
    if not 0.0 <= dtx_silence <= 1.0 or int(sid_every) < 1:
        raise ValueError(f"bitrate: dtx_silence = {dtx_silence} (0 .. 1), sid_every = {sid_every} (>= 1)")
    return rate * ((1.0 - dtx_silence) + dtx_silence / int(sid_every))


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
PACKET_MAGIC_SID = b"Fp"                      # a SID packet: "silence follows" 


def write_packet(seq, n_frames, payload, sid=False):
    """One push of one stream: b"FP" (sid: b"Fp"), seq (taken modulo 65536), n_frames, payload, CRC-32."""
    if not 0 <= n_frames <= 0xFFFF:
        raise ValueError(f"packet: n_frames = {n_frames} does not fit 16 bits")
    body = _PHEAD.pack(PACKET_MAGIC_SID if sid else PACKET_MAGIC, seq & 0xFFFF, n_frames) + bytes(payload)
    return body + struct.pack("<I", zlib.crc32(body))


def read_packet(blob, Q, bits, _magic=PACKET_MAGIC):
    """-> (seq, n_frames, payload bytes).  ValueError for a short packet, a wrong magic (a SID packet's included), a CRC failure,
    or a payload whose length is not payload_bytes(n_frames, Q, bits)."""
    blob = bytes(blob)
    if len(blob) < PACKET_OVERHEAD:
        raise ValueError(f"packet: truncated ({len(blob)} bytes)")
    magic, seq, n_frames = _PHEAD.unpack_from(blob)
    if magic != _magic:
        raise ValueError(f"packet: wrong magic {magic!r} (expected {_magic!r})")
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


# ------------------------------------------------------------------------------------ packets that survive a loss
FEC_MAGIC = b"FQ"
FEC_MAGIC_SID = b"Fq"
_QHEAD = struct.Struct("<2sHHH3B")
FEC_OVERHEAD = _QHEAD.size + 4               # 15 bytes around the two payloads
assert _QHEAD.size == 11

Packet = namedtuple("Packet", "seq n_frames payload n_red_frames n_red red_payload sid", defaults=(False,))
Packet.__doc__ = """A parsed packet of either kind; an b"FP" packet has n_red_frames = 0, n_red = (0, 0, 0), red_payload = b"".
sid: a SID packet (b"Fp" / b"Fq"), which only LossyPacketReader(dtx=True) reads."""


def _check_red(n_red, n_q, what):
    n_red = tuple(int(n) for n in n_red)
    if len(n_red) != 3 or any(not 0 <= r <= n for r, n in zip(n_red, n_q)):
        raise ValueError(f"{what}: redundant quantizer counts {n_red} are not three counts within n_q = {tuple(n_q)}")
    return n_red


def write_packet_fec(seq, n_frames, payload, n_red_frames=0, n_red=(0, 0, 0), red_payload=b"", sid=False):
    """One push of one stream with the previous push's redundant layer: b"FQ" (sid: b"Fq"), seq (modulo 65536), n_frames,
    n_red_frames, n_red, primary payload, redundant payload, CRC-32.  The payload lengths are the caller's (read_packet_fec
    checks them against the layout it is handed)."""
    if not 0 <= n_frames <= 0xFFFF or not 0 <= n_red_frames <= 0xFFFF:
        raise ValueError(f"packet: n_frames = {n_frames} / n_red_frames = {n_red_frames} do not fit 16 bits")
    n_red = tuple(int(n) for n in n_red)
    if len(n_red) != 3 or any(not 0 <= n <= MAX_Q for n in n_red):
        raise ValueError(f"packet: redundant quantizer counts {n_red} (three counts, 0..{MAX_Q})")
    body = _QHEAD.pack(FEC_MAGIC_SID if sid else FEC_MAGIC, seq & 0xFFFF, n_frames, n_red_frames, *n_red) + bytes(payload) + bytes(red_payload)
    return body + struct.pack("<I", zlib.crc32(body))


def read_packet_fec(blob, n_q, bits, _magic=FEC_MAGIC):
    """-> Packet(seq, n_frames, payload, n_red_frames, n_red, red_payload) for the stream layout n_q = (n_p, n_c, n_r), bits.
    ValueError for a short packet, a wrong magic (a SID packet's included), a CRC failure, n_red beyond n_q, redundant frames without redundant
    quantizers, or a length that is not 15 + payload_bytes(n_frames, Q, bits) + payload_bytes(n_red_frames, R, bits)."""
    blob = bytes(blob)
    if len(blob) < FEC_OVERHEAD:
        raise ValueError(f"packet: truncated ({len(blob)} bytes)")
    magic, seq, n_frames, n_red_frames, rp, rc, rr = _QHEAD.unpack_from(blob)
    if magic != _magic:
        raise ValueError(f"packet: wrong magic {magic!r} (expected {_magic!r})")
    crc, = struct.unpack_from("<I", blob, len(blob) - 4)
    if zlib.crc32(blob[:-4]) != crc:
        raise ValueError("packet: CRC mismatch (corrupt packet)")
    n_red = _check_red((rp, rc, rr), n_q, "packet")
    if n_red_frames and not sum(n_red):
        raise ValueError(f"packet: {n_red_frames} redundant frames of no quantizers")
    n1, n2 = payload_bytes(n_frames, sum(n_q), bits), payload_bytes(n_red_frames, sum(n_red), bits)
    if len(blob) - FEC_OVERHEAD != n1 + n2:
        raise ValueError(f"packet: {len(blob) - FEC_OVERHEAD} payload bytes, {n_frames} frames x {sum(n_q)} x {bits} bits and "
                         f"{n_red_frames} redundant frames x {sum(n_red)} x {bits} bits need {n1} + {n2}")
    return Packet(seq, n_frames, blob[_QHEAD.size:_QHEAD.size + n1], n_red_frames, n_red, blob[_QHEAD.size + n1:-4],
                  _magic == FEC_MAGIC_SID)


class LossyPacketReader:
    """Byte-level half of a receiver that survives loss: per push one entry per stream in -- a packet (b"FP" or b"FQ") or None --
    and per stream the parsed Packet or None out.  Every stream is judged on its own:

        rd = LossyPacketReader(n_streams, n_q, bits)
        parsed = rd.feed(packets)                  # parsed[b] is a Packet, or None: missing, corrupt or of the wrong seq

    Every feed() is one push: the expected seq advances by one (modulo 65536) whatever arrived.  A packet that does not parse
    (truncation, magic, CRC, a length that disagrees with the layout) counts in corrupt[b], one with another seq than the expected
    in misordered[b], a good one in received[b]; the first two are treated as missing.  feed() never raises for a loss (only for
    a list that has not one entry per stream).  dtx=True: SID packets (b"Fp", b"Fq") parse too, as Packets with sid = True;
    with dtx=False they count as corrupt, as any unknown magic does."""

    def __init__(self, n_streams, n_q, bits, first_seq=0, dtx=False):
        self.dtx = bool(dtx)
        self.n_streams, self.n_q, self.bits = int(n_streams), tuple(int(n) for n in n_q), int(bits)
        _check_layout(self.bits, self.n_q, "LossyPacketReader")
        self.expected = first_seq & 0xFFFF
        self.received, self.corrupt, self.misordered = ([0] * self.n_streams for _ in range(3))

    def parse(self, blob):
        """One packet of either kind -> Packet; ValueError as read_packet / read_packet_fec."""
        blob = bytes(blob)
        sid = self.dtx and blob[:2] in (PACKET_MAGIC_SID, FEC_MAGIC_SID)
        if blob[:2] == (FEC_MAGIC_SID if sid else FEC_MAGIC):
            return read_packet_fec(blob, self.n_q, self.bits, blob[:2])
        seq, n_frames, payload = read_packet(blob, sum(self.n_q), self.bits, PACKET_MAGIC_SID if sid else PACKET_MAGIC)
        return Packet(seq, n_frames, payload, 0, (0, 0, 0), b"", sid)

    def feed(self, packets):
        packets = list(packets)
        if len(packets) != self.n_streams:
            raise ValueError(f"{len(packets)} entries for {self.n_streams} streams")
        out = []
        for b, blob in enumerate(packets):
            pkt = None
            if blob is not None:
                try:
                    pkt = self.parse(blob)
                except ValueError:
                    self.corrupt[b] += 1
                if pkt is not None and pkt.seq != self.expected:
                    self.misordered[b] += 1
                    pkt = None
                if pkt is not None:
                    self.received[b] += 1
            out.append(pkt)
        self.expected = (self.expected + 1) & 0xFFFF
        return out
