"""The bitstream on the GPU: fac_codes_pack / fac_codes_unpack bit for bit against the big-integer definition of
the layout (include/facodec_hip.h) over field widths, quantizer counts, frame counts and batch sizes that put field boundaries
on, before and after 32-bit word boundaries; strided inputs, guarded outputs, ragged lengths, out-of-range codes, unaligned
input; the fixture's real codes; compress / decompress and their clip-list and long-form variants against the calls they wrap;
the packetizer pair around a streaming session.

The independent reference is the Python big-integer arithmetic below, nothing of the product."""
import os

import numpy as np
import pytest
import torch

from facodec_amd import _lib, bitstream, synth

pytestmark = pytest.mark.gpu

BITS = [1, 7, 8, 10, 11, 16]
N_Q = [(1, 2, 3), (1, 0, 0), (0, 2, 0), (1, 1, 3), (4, 6, 6)]
FRAMES = [1, 2, 3, 7, 8, 9, 53, 160]
E2E_TOL = 1e-4
GUARD = 0xA5


# ------------------------------------------------------------------------------------------------ the reference
def bigint_payload(rows, bits):
    """rows (Q, F) integers in quantizer order -> the payload bytes of include/facodec_hip.h's definition."""
    Q, F = len(rows), len(rows[0]) if len(rows) else 0
    mask = (1 << bits) - 1
    N = 0
    for t in range(F):
        for q in range(Q):
            N |= (int(rows[q][t]) & mask) << (bits * (t * Q + q))
    return N.to_bytes((F * Q * bits + 7) // 8, "little")


def bigint_fields(payload, Q, F, bits):
    """The inverse: payload bytes -> (Q, F) list of codes."""
    N = int.from_bytes(payload, "little")
    mask = (1 << bits) - 1
    return [[(N >> (bits * (t * Q + q))) & mask for t in range(F)] for q in range(Q)]


def row_bytes(T, Q, bits):
    return 4 * (((T * Q * bits + 7) // 8 + 3) // 4)


def ref_rows(codes_cpu, bits, lens=None):
    """codes_cpu: three (B, n, T) int64 CPU tensors -> (B, row_bytes) uint8: every clip's own frames, zeros behind."""
    B, T = codes_cpu[0].shape[0], codes_cpu[0].shape[2]
    Q = sum(c.shape[1] for c in codes_cpu)
    out = torch.zeros(B, row_bytes(T, Q, bits), dtype=torch.uint8)
    for b in range(B):
        F = T if lens is None else max(0, min(int(lens[b]), T))
        rows = [r[:F] for c in codes_cpu for r in c[b].tolist()]
        pl = bigint_payload(rows, bits)
        out[b, :len(pl)] = torch.frombuffer(bytearray(pl), dtype=torch.uint8) if pl else out[b, :0]
    return out


def make_codes(n_q, B, T, bits, gen, dev, lo=None, hi=None):
    """Three strided views (a row slice and a time slice of a wider tensor each), values over the full [0, 2^bits)."""
    lo, hi = (0 if lo is None else lo), ((1 << bits) if hi is None else hi)
    views = []
    for n in n_q:
        base = torch.randint(lo, hi, (B, n + 1, T + 5), generator=gen, dtype=torch.int64).to(dev)
        v = base[:, :n, 2:2 + T]
        views.append(v)
    return views


def guarded_out(B, rb, dev, gap=8):
    """out (B, rb + gap) inside a larger 0xA5 buffer -> (whole buffer, the view to pack into, row stride)."""
    bs = rb + gap
    buf = torch.full((8 + B * bs + 8,), GUARD, dtype=torch.uint8, device=dev)
    return buf, buf[8:8 + B * bs].view(B, bs), bs


def check_guarded(buf, B, rb, bs, want):
    host = buf.cpu()
    assert bool((host[:8] == GUARD).all()) and bool((host[8 + B * bs:] == GUARD).all())
    body = host[8:8 + B * bs].view(B, bs)
    assert bool((body[:, rb:] == GUARD).all()), "the gap between row_bytes and out_bs was written"
    assert torch.equal(body[:, :rb], want)


# ------------------------------------------------------------------------------------------------ pack
@pytest.mark.parametrize("n_q", N_Q, ids=str)
@pytest.mark.parametrize("bits", BITS)
def test_pack_matches_bigint(cuda, bits, n_q):
    from facodec_amd import ops
    gen = torch.Generator().manual_seed(1000 * bits + sum(n * 7 ** i for i, n in enumerate(n_q)))
    Q = sum(n_q)
    for T in FRAMES:
        for B in (1, 3):
            codes = make_codes(n_q, B, T, bits, gen, cuda)
            rb = row_bytes(T, Q, bits)
            assert ops.codes_row_bytes(T, Q, bits) == rb
            buf, out, bs = guarded_out(B, rb, cuda)
            got = ops.pack_codes([c if c.shape[1] else None for c in codes] if T % 2 else codes, bits=bits, out=out)
            assert got.shape == (B, rb) and got.data_ptr() == out.data_ptr()
            check_guarded(buf, B, rb, bs, ref_rows([c.cpu() for c in codes], bits))


@pytest.mark.parametrize("B,T", [(32, 160), (1, 1000)])
def test_pack_benchmark_and_long_rows(cuda, B, T):
    from facodec_amd import ops
    gen = torch.Generator().manual_seed(B + T)
    codes = make_codes((1, 2, 3), B, T, 10, gen, cuda)
    got = ops.pack_codes(codes)
    assert got.dtype == torch.uint8 and got.shape == (B, row_bytes(T, 6, 10)) and got.is_contiguous()
    assert torch.equal(got.cpu(), ref_rows([c.cpu() for c in codes], 10))
    back = ops.unpack_codes(got, (1, 2, 3), T)
    assert all(torch.equal(a, b) for a, b in zip(back, codes))


@pytest.mark.parametrize("bits,n_q,T", [(10, (1, 2, 3), 9), (10, (1, 2, 3), 53), (7, (1, 1, 3), 8), (16, (4, 6, 6), 3), (1, (1, 0, 0), 53),
                                        (11, (0, 2, 0), 1)], ids=str)
def test_pack_ragged(cuda, bits, n_q, T):
    """lens containing 0, 1, T - 1, T, a value above T and a negative one: the clip's own frames, then zeros up to row_bytes."""
    from facodec_amd import ops
    lens = [0, 1, T - 1, T, T + 3, -2]
    B = len(lens)
    gen = torch.Generator().manual_seed(bits * 31 + T)
    codes = make_codes(n_q, B, T, bits, gen, cuda)
    rb = row_bytes(T, sum(n_q), bits)
    buf, out, bs = guarded_out(B, rb, cuda, gap=4)
    ops.pack_codes(codes, bits=bits, lens=torch.tensor(lens, dtype=torch.int32, device=cuda), out=out)
    want = ref_rows([c.cpu() for c in codes], bits, lens)
    assert not want[0].any() and not want[5].any()
    check_guarded(buf, B, rb, bs, want)


@pytest.mark.parametrize("bits", [1, 7, 10, 16])
def test_pack_masks_out_of_range_codes(cuda, bits):
    """Codes above 2^bits - 1 (and negative ones) in some positions: the field is the masked value, the neighbours are untouched."""
    from facodec_amd import ops
    gen = torch.Generator().manual_seed(bits)
    B, T, n_q = 2, 9, (1, 2, 3)
    clean = [c.contiguous() for c in make_codes(n_q, B, T, bits, gen, cuda)]
    dirty = [c.clone() for c in clean]
    for c in dirty:
        hit = torch.rand(c.shape, generator=gen).to(cuda) < 0.3
        junk = (torch.randint(1, 1 << 20, c.shape, generator=gen, dtype=torch.int64).to(cuda) << bits)
        sign = torch.where(torch.rand(c.shape, generator=gen).to(cuda) < 0.5, 1, -1)
        c += torch.where(hit, junk * sign, torch.zeros_like(junk))
    assert any(bool((d != c).any()) for d, c in zip(dirty, clean))
    want = ref_rows([c.cpu() for c in clean], bits)
    assert torch.equal(ref_rows([c.cpu() for c in dirty], bits), want)      # the definition masks; so must the kernel
    assert torch.equal(ops.pack_codes(dirty, bits=bits).cpu(), want)


# ------------------------------------------------------------------------------------------------ unpack
@pytest.mark.parametrize("n_q", N_Q, ids=str)
@pytest.mark.parametrize("bits", BITS)
def test_unpack_inverts_pack_and_matches_bigint(cuda, bits, n_q):
    from facodec_amd import ops
    gen = torch.Generator().manual_seed(77 * bits + sum(n_q))
    Q = sum(n_q)
    for T in FRAMES:
        for B in (1, 3):
            codes = make_codes(n_q, B, T, bits, gen, cuda)
            back = ops.unpack_codes(ops.pack_codes(codes, bits=bits), n_q, T, bits=bits)
            assert [tuple(x.shape) for x in back] == [(B, n, T) for n in n_q] and all(x.dtype == torch.int64 for x in back)
            assert all(torch.equal(a, b) for a, b in zip(back, codes))
            # random bytes, at an odd row stride behind a one-byte offset: big-int field extraction
            need = (T * Q * bits + 7) // 8
            in_bs = need + 1 + (need % 2)                                   # odd
            raw = torch.randint(0, 256, (1 + B * in_bs,), generator=gen, dtype=torch.uint8)
            packed = raw.to(cuda)[1:].view(B, in_bs)
            assert packed.data_ptr() % 2 == 1 and in_bs % 2 == 1
            got = torch.cat(ops.unpack_codes(packed, n_q, T, bits=bits), dim=1).cpu()
            rows = raw[1:].view(B, in_bs)
            want = torch.tensor([bigint_fields(bytes(rows[b, :need].tolist()), Q, T, bits) for b in range(B)], dtype=torch.int64)
            assert torch.equal(got, want)


def test_unpack_ragged_tails_and_untouched_surroundings(cuda):
    from facodec_amd import ops
    bits, n_q, T = 10, (1, 2, 3), 53
    lens = [0, 1, T - 1, T, T + 3, -2]
    B = len(lens)
    gen = torch.Generator().manual_seed(3)
    codes = [c.contiguous() for c in make_codes(n_q, B, T, bits, gen, cuda)]
    packed = ops.pack_codes(codes, bits=bits)                              # full rows: unpack must zero the tails itself
    bases = [torch.full((B + 1, n + 2, T + 7), -7, dtype=torch.int64, device=cuda) for n in n_q]
    outs = [b[:B, 1:1 + n, 3:3 + T] for b, n in zip(bases, n_q)]
    got = ops.unpack_codes(packed, n_q, T, bits=bits, lens=torch.tensor(lens, dtype=torch.int32, device=cuda), out=outs)
    for r, (g, c, base) in enumerate(zip(got, codes, bases)):
        assert g.data_ptr() == outs[r].data_ptr()
        for b, L in enumerate(lens):
            L = max(0, min(L, T))
            assert torch.equal(g[b, :, :L], c[b, :, :L]) and not g[b, :, L:].any()
        guard = torch.ones_like(base, dtype=torch.bool)
        guard[:B, 1:1 + n_q[r], 3:3 + T] = False
        assert bool((base[guard] == -7).all()), "unpack wrote outside its output views"


# ------------------------------------------------------------------------------------------------ real codes
def test_golden_codes_through_the_container(cuda, golden_dir):
    from facodec_amd import ops
    d = np.load(os.path.join(golden_dir, "codec_e2e.npz"))
    codes = [torch.from_numpy(d[n].astype(np.int64)) for n in ("codes_p", "codes_c", "codes_r")]
    timbre = d["timbre"]
    rows = ops.pack_codes([c.to(cuda) for c in codes]).cpu()
    assert rows.shape == (2, 1200) and torch.equal(rows, ref_rows(codes, 10))
    blobs = [bitstream.write(dict(bits=10, n_q=(1, 2, 3), sample_rate=24000, n_frames=160, n_samples=48000, codebook_size=1024),
                             timbre[b].tobytes(), rows[b].numpy().tobytes()) for b in range(2)]
    assert all(len(b) == 32 + 4096 + 1200 + 4 for b in blobs)
    parsed = [bitstream.read(b) for b in blobs]
    assert all(np.array_equal(p[1], timbre[b]) for b, p in enumerate(parsed))
    packed = torch.from_numpy(np.stack([np.frombuffer(p[2], dtype=np.uint8) for p in parsed])).to(cuda)
    back = ops.unpack_codes(packed, parsed[0][0].n_q, parsed[0][0].n_frames, bits=parsed[0][0].bits)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(back, codes))


# ------------------------------------------------------------------------------------------------ end to end, synthetic weights
@pytest.fixture(scope="module")
def full_model(cuda):
    from facodec_amd.commons import build_model, default_model_params
    model = build_model(default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(cuda)
    return model


@pytest.fixture(scope="module")
def forward(full_model, cuda):
    """One forward of B = 2 clips of the shortest length the clip calls take: wave, codes, timbre, and the decodes the tests share."""
    from facodec_amd import commons
    m = full_model
    n = commons.min_clip_samples(m)
    assert n == 3000
    wave = synth.synth_clips(2, n, seed=41).to(cuda)
    with torch.no_grad():
        out = m.quantizer(m.encoder(wave), wave, n_c=2, return_codes=True)
    timbre, codes = out[4], [c.clone() for c in out[5]]
    return dict(wave=wave, codes=codes, timbre=timbre.clone(), decoded=commons.decode_codes(m, codes, timbre).clone())


def test_compress_decompress_is_decode_codes(full_model, forward):
    from facodec_amd import commons
    m, F = full_model, 10
    blobs = commons.compress(m, forward["wave"])
    assert isinstance(blobs, list) and len(blobs) == 2 and all(isinstance(b, bytes) for b in blobs)
    assert all(len(b) == 32 + 4096 + bitstream.payload_bytes(F, 6, 10) + 4 for b in blobs)
    for b, blob in enumerate(blobs):
        hdr, tim, payload = bitstream.read(blob)
        assert (hdr.bits, hdr.n_q, hdr.n_frames, hdr.n_samples, hdr.sample_rate, hdr.codebook_size, hdr.timbre_dim, hdr.flags) == \
            (10, (1, 2, 3), F, 3000, 24000, 1024, 1024, 1)
        assert np.array_equal(tim, forward["timbre"][b].cpu().numpy())
        assert payload == bigint_payload([r for c in forward["codes"] for r in c[b].tolist()], 10)
    waves = commons.decompress(m, blobs)
    assert isinstance(waves, list) and all(w.shape == (1, 300 * F) for w in waves)
    assert torch.equal(torch.stack(waves), forward["decoded"])
    one = commons.compress(m, forward["wave"][0, 0])                         # one clip in, one blob out, one wave back
    assert isinstance(one, bytes) and bitstream.read(one)[0].n_frames == F
    w = commons.decompress(m, one)
    assert isinstance(w, torch.Tensor) and w.shape == (1, 300 * F)


def test_compress_fewer_residual_rows(full_model, forward):
    from facodec_amd import commons
    m = full_model
    p, c, r = forward["codes"]
    full = len(commons.compress(m, forward["wave"])[0])
    for n_r in (1, 0):
        blobs = commons.compress(m, forward["wave"], n_r=n_r)
        assert bitstream.read(blobs[0])[0].n_q == (1, 2, n_r)
        assert full - len(blobs[0]) == bitstream.payload_bytes(10, 6, 10) - bitstream.payload_bytes(10, 3 + n_r, 10)
        want = commons.decode_codes(m, [p, c, r[:, :n_r]], forward["timbre"])
        assert torch.equal(torch.stack(commons.decompress(m, blobs)), want)
    with pytest.raises(ValueError, match="n_r"):
        commons.compress(m, forward["wave"], n_r=4)


def test_timbre_override_and_missing_timbre(full_model, forward):
    from facodec_amd import commons
    m = full_model
    swapped = forward["timbre"].flip(0).contiguous()
    want = commons.decode_codes(m, forward["codes"], swapped)
    blobs = commons.compress(m, forward["wave"])
    assert torch.equal(torch.stack(commons.decompress(m, blobs, timbre=swapped)), want)
    bare = commons.compress(m, forward["wave"], with_timbre=False)
    assert all(len(b) == 32 + 75 + 4 for b in bare) and bitstream.read(bare[0])[1] is None
    with pytest.raises(ValueError, match="timbre"):
        commons.decompress(m, bare)
    assert torch.equal(torch.stack(commons.decompress(m, bare, timbre=swapped)), want)
    assert torch.equal(torch.stack(commons.decompress(m, bare, timbre=[swapped[0], swapped[1]])), want)


def test_decompress_checks_headers_and_groups_layouts(full_model, forward):
    from facodec_amd import commons
    m = full_model
    blobs = commons.compress(m, forward["wave"])
    hdr, tim, payload = bitstream.read(blobs[0])
    for bad in (dict(codebook_size=512), dict(timbre_dim=512)):
        f = dict(hdr._asdict(), **bad)
        t = tim if "timbre_dim" not in bad else tim[:512]
        with pytest.raises(ValueError, match=next(iter(bad))):
            commons.decompress(m, bitstream.write(f, t.tobytes(), payload))
    with pytest.raises(ValueError, match="CRC"):
        commons.decompress(m, [blobs[0], blobs[1][:100] + bytes([blobs[1][100] ^ 1]) + blobs[1][101:]])
    # blobs that disagree on the quantizer counts: separate groups, each within fp32 noise of its row of the batch decode
    # (a B = 1 decode and a B = 2 decode may pick different conv kernels: E2E_TOL is the suite's bound for that)
    mixed = [blobs[0], commons.compress(m, forward["wave"], n_r=1)[1]]
    waves = commons.decompress(m, mixed)
    p, c, r = forward["codes"]
    want1 = commons.decode_codes(m, [p, c, r[:, :1]], forward["timbre"])[1]
    for w, ref in ((waves[0], forward["decoded"][0]), (waves[1], want1)):
        assert w.shape == ref.shape
        assert float((w.double() - ref.double()).abs().max() / ref.double().abs().max()) < E2E_TOL


def test_compress_at_another_sample_rate(full_model, cuda):
    from facodec_amd import commons
    m = full_model
    wave = synth.synth_clips(2, 2200, seed=43).to(cuda)                      # 2200 samples at 16 kHz -> 3300 at 24 kHz: 11 frames
    blobs = commons.compress(m, wave, sample_rate=16000)
    hdr = bitstream.read(blobs[0])[0]
    assert (hdr.sample_rate, hdr.n_samples, hdr.n_frames) == (16000, 2200, 11)
    waves = commons.decompress(m, blobs)
    assert all(w.shape == (1, 2200) for w in waves)                          # ceil(3300 * 16000 / 24000)
    assert all(w.shape == (1, 3300) for w in commons.decompress(m, blobs, sample_rate=24000))


def test_compress_clips_is_reconstruct_clips(full_model, cuda):
    from facodec_amd import commons
    m = full_model
    w = synth.synth_clips(3, 4500, seed=44).to(cuda)
    clips = [w[0, 0, :3000], w[1, :, :4500], w[2, 0, :3650]]
    blobs = commons.compress_clips(m, clips)
    assert [bitstream.read(b)[0].n_frames for b in blobs] == [10, 15, 12]
    assert [bitstream.read(b)[0].n_samples for b in blobs] == [3000, 4500, 3650]
    assert [len(b) for b in blobs] == [32 + 4096 + bitstream.payload_bytes(F, 6, 10) + 4 for F in (10, 15, 12)]
    got = commons.decompress(m, blobs)
    want = commons.reconstruct_clips(m, clips)
    for g, r, F in zip(got, want, (10, 15, 12)):
        assert g.shape == (1, 300 * F) and torch.equal(g, r)


def test_compress_long_is_reconstruct_long(full_model, cuda):
    from facodec_amd import commons
    m = full_model
    wave = synth.synth_clips(2, 9750, seed=45).to(cuda)                      # 32 frames in chunks of 0.2 s = 16 frames
    blobs = commons.compress_long(m, wave, chunk_seconds=0.2)
    hdr = bitstream.read(blobs[0])[0]
    assert len(blobs) == 2 and (hdr.n_frames, hdr.n_samples, hdr.n_q) == (32, 9750, (1, 2, 3))
    got = commons.decompress_long(m, blobs, chunk_seconds=0.2)
    assert got.shape == (2, 1, 9600) and torch.equal(got, commons.reconstruct_long(m, wave, chunk_seconds=0.2))
    with pytest.raises(ValueError, match="one recording batch"):
        commons.decompress_long(m, [blobs[0], commons.compress_long(m, wave, n_r=1, chunk_seconds=0.2)[1]], chunk_seconds=0.2)


# ------------------------------------------------------------------------------------------------ streaming
def test_streaming_session_through_packets(full_model, cuda):
    """Every chunk of codes a StreamingCodec session emits goes through CodePacketizer -> bytes -> CodeDepacketizer into one
    StreamingDecoder; a second StreamingDecoder gets the code tensors directly.  The same samples, bit for bit."""
    from facodec_amd.streaming import HOP, CodeDepacketizer, CodePacketizer, StreamingCodec, StreamingDecoder
    m = full_model
    n_hops = 5                                                               # one 5-hop period: 7200 samples = 24 frames
    wave = synth.synth_clips(2, 4800 + n_hops * HOP, seed=46).to(cuda)
    with torch.no_grad():
        timbre = m.quantizer(m.encoder(wave), wave, n_c=2, return_codes=True)[4].clone()
    tx = CodePacketizer((1, 2, 3))
    headers = tx.header(timbre)
    assert len(headers) == 2 and all(len(h) == 32 + 4096 + 4 for h in headers)
    h0 = bitstream.read(headers[0])[0]
    assert h0.is_stream_header and h0.n_frames == 0 and h0.n_q == (1, 2, 3)
    rxc = CodeDepacketizer(headers)
    assert rxc.timbre.is_cuda and torch.equal(rxc.timbre, timbre) and rxc.n_q == (1, 2, 3) and rxc.bits == 10
    rx_bytes = StreamingDecoder(m, rxc.timbre, use_graphs=False)
    rx_direct = StreamingDecoder(m, timbre, use_graphs=False)
    sess = StreamingCodec(m, timbre, n_c=2, use_graphs=False)
    outs = [sess.prime(wave[:, :, :4800])]
    outs += [sess.push(wave[:, :, 4800 + h * HOP:4800 + (h + 1) * HOP]) for h in range(n_hops)]
    outs.append(sess.finish())
    n_sent, frames, last = 0, 0, None
    for o in outs:
        if o["codes"] is None:
            continue
        k = o["codes"][0].shape[-1]
        packets = tx.packet(o["codes"])
        assert len(packets) == 2 and all(isinstance(p, bytes) and len(p) == 10 + -(-60 * k // 8) for p in packets)
        assert all(p[:2] == b"FP" and int.from_bytes(p[2:4], "little") == n_sent and int.from_bytes(p[4:6], "little") == k for p in packets)
        codes = rxc.feed(packets)
        assert all(torch.equal(a, b) for a, b in zip(codes, o["codes"]))
        a = (rx_bytes.prime if n_sent == 0 else rx_bytes.push)(codes)
        b = (rx_direct.prime if n_sent == 0 else rx_direct.push)(o["codes"])
        assert a.shape == (2, 1, 300 * k) and torch.equal(a, b)
        n_sent, frames, last = n_sent + 1, frames + k, o["codes"]
    assert n_sent >= 3 and frames == wave.shape[-1] // 300
    # one packet dropped on the way
    tx.packet(last)
    late = tx.packet(last)
    with pytest.raises(bitstream.PacketLoss) as e:
        rxc.feed(late)
    assert e.value.missing == 1
    assert all(torch.equal(a, b) for a, b in zip(rxc.feed(late), last))
    with pytest.raises(ValueError, match="CRC"):
        rxc.feed([late[0], late[1][:8] + bytes([late[1][8] ^ 4]) + late[1][9:]])
    # a converter's [p, c] codes: n_q with a trailing zero, the residual comes back as (B, 0, k)
    tx2 = CodePacketizer((1, 1))
    rx2 = CodeDepacketizer(tx2.header(timbre))
    back = rx2.feed(tx2.packet([last[0], last[1][:, :1]]))
    assert torch.equal(back[0], last[0]) and torch.equal(back[1], last[1][:, :1]) and back[2].shape == (2, 0, last[0].shape[-1])


# ------------------------------------------------------------------------------------------------ guards
def test_guards_raise_before_any_launch(cuda):
    from facodec_amd import ops
    codes = [torch.zeros(2, n, 9, dtype=torch.int64, device=cuda) for n in (1, 2, 3)]
    packed = torch.zeros(2, 68, dtype=torch.uint8, device=cuda)
    with pytest.raises(_lib.FacodecHipError):
        ops.pack_codes([c.cpu() for c in codes])
    with pytest.raises(_lib.FacodecHipError):
        ops.pack_codes([codes[0], codes[1].int(), codes[2]])
    with pytest.raises(ValueError):
        ops.pack_codes([codes[0], codes[1], codes[2][:, :, :5]])
    with pytest.raises(ValueError):
        ops.pack_codes([codes[0], codes[1], codes[2][:1]])
    with pytest.raises(ValueError):
        ops.pack_codes([codes[0][:, :0], codes[1][:, :0], None])              # no quantizer at all
    with pytest.raises(ValueError):
        ops.pack_codes([torch.zeros(2, 6, 9, dtype=torch.int64, device=cuda)] * 3)    # 18 quantizers
    for bits in (0, 17):
        with pytest.raises(ValueError):
            ops.pack_codes(codes, bits=bits)
        with pytest.raises(ValueError):
            ops.unpack_codes(packed, (1, 2, 3), 9, bits=bits)
    with pytest.raises(_lib.FacodecHipError):
        ops.pack_codes(codes, lens=torch.tensor([9, 9], dtype=torch.int32))   # lens on the host
    with pytest.raises(_lib.FacodecHipError):
        ops.pack_codes(codes, lens=torch.tensor([9, 9], device=cuda))         # int64 lens
    with pytest.raises(ValueError):
        ops.pack_codes(codes, out=torch.zeros(2, 64, dtype=torch.uint8, device=cuda))         # 9 frames need 68 bytes a row
    with pytest.raises(ValueError):
        ops.pack_codes(codes, out=torch.zeros(2, 70, dtype=torch.uint8, device=cuda))         # a row stride that is no multiple of 4
    with pytest.raises(_lib.FacodecHipError):
        ops.unpack_codes(packed.cpu(), (1, 2, 3), 9)
    with pytest.raises(_lib.FacodecHipError):
        ops.unpack_codes(packed.to(torch.int8), (1, 2, 3), 9)
    with pytest.raises(ValueError, match="too short"):
        ops.unpack_codes(packed[:, :67], (1, 2, 3), 9)
    with pytest.raises(ValueError):
        ops.unpack_codes(packed, (0, 0, 0), 9)
    with pytest.raises(ValueError):
        ops.unpack_codes(packed, (1, 2, 3), 0)
    assert ops.unpack_codes(packed, (1, 2, 3), 9)[2].shape == (2, 3, 9)
