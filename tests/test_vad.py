"""Voice activity, silent-push suppression and comfort frames on the device: ops.vad and VoiceActivity against the
fp64 restatement of tests/test_vad_cpu.py (flags equal, energies equal in every bit), fac_sid_apply against numpy, and the DTX
link end to end against the plain receiver and a plain StreamingDecoder fed the substituted codes."""
import numpy as np
import pytest
import torch

from facodec_amd import _lib
from test_plc import _NoReadback, _session, full_model  # noqa: F401  (full_model: the module-scoped fixture)
from test_vad_cpu import MARGIN, vad_ref

pytestmark = pytest.mark.gpu
N_Q = (1, 2, 3)
W_S, H_S = 4, 3                                  # the small window and hangover of the long cases
GUARD = 0xA5


def _signal(B, T, seed):
    """Noise whose level jumps by up to 50 dB every few hundred samples: flags that switch often, energies over many binades."""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, T), np.float32)
    for b in range(B):
        t = 0
        while t < T:
            n = int(rng.integers(40, 900))
            x[b, t:t + n] = (rng.standard_normal(min(n, T - t)) * 10.0 ** rng.uniform(-4.5, -0.5)).astype(np.float32)
            t += n
    return x


def _bits(t):
    return t.contiguous().view(torch.int64)


def _ref_batch(x, frame, W, H, lens=None, floor_db=-70.0):
    thr = frame * 10.0 ** (floor_db / 10.0)
    out = [vad_ref(x[b], frame, W, H, MARGIN, thr, None if lens is None else lens[b]) for b in range(x.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("frame", [1, 63, 64, 65, 300])
def test_vad_matches_the_restatement_bit_for_bit(B, frame, cuda):
    from facodec_amd import ops
    lengths = sorted({1, 299, 300, 301, 599, 600, 64, 65, 300 * (W_S + H_S) + 7, frame - 1, frame, frame + 1, 2 * frame - 1, 2 * frame,
                      frame * (W_S + H_S) + 7} - {0})
    active = 0
    for T in lengths:
        if frame == 1 and T > 700:
            continue                                                     # one wave per sample: kept small
        x = _signal(B, T, seed=1000 * frame + T)
        want_f, want_e = _ref_batch(x, frame, W_S, H_S)
        flags, e = ops.vad(torch.from_numpy(x).to(cuda), frame=frame, window=W_S, hangover=H_S)
        F = -(-T // frame)
        assert flags.shape == (B, F) and flags.dtype == torch.uint8 and e.shape == (B, F) and e.dtype == torch.float64
        assert torch.equal(_bits(e).cpu(), torch.from_numpy(want_e).view(torch.int64)), (T, frame)
        assert torch.equal(flags.cpu(), torch.from_numpy(want_f)), (T, frame)
        active += int(want_f.sum())
        assert not want_f[:, 0].any()
    assert active > 0                                                    # the signals do switch the detector on


def test_vad_defaults_ragged_lens_and_guards(cuda):
    """The default parameters on 3 x 12 000 samples with lens = (all, 301, 0) -- and, through the two entries with preallocated
    outputs, a 0xA5 guard on either side of every output row."""
    from facodec_amd import ops
    B, T, frame = 3, 12000, 300
    x = _signal(B, T, seed=5)
    lens = [T, 301, 0]
    xd = torch.from_numpy(x).to(cuda)
    ld = torch.tensor(lens, dtype=torch.int32, device=cuda)
    want_f, want_e = _ref_batch(x, frame, 120, 16, lens)
    flags, e = ops.vad(xd, lens=ld)
    assert torch.equal(_bits(e).cpu(), torch.from_numpy(want_e).view(torch.int64)) and torch.equal(flags.cpu(), torch.from_numpy(want_f))
    assert want_f[0].any() and not want_f[1, 2:].any() and not want_e[1, 2:].any() and not want_e[2].any()
    flags3, _ = ops.vad(xd[:, None, :], lens=ld)                                      # (B, 1, T)
    assert torch.equal(flags3, flags)
    F = T // frame
    e_full = torch.full((B, F + 4), float("nan"), dtype=torch.float64, device=cuda)
    e_full.view(torch.uint8).fill_(GUARD)
    f_full = torch.full((B, F + 6), GUARD, dtype=torch.uint8, device=cuda)
    ev, fv = e_full[:, 2:F + 2], f_full[:, 3:F + 3]
    frame_, W, H, margin, thr = ops.vad_params()
    assert ops.vad_energy(xd, ev, frame_, lens=ld, R=F) == F
    ops.vad_decide(ev, 0, F, W, H, margin, thr, frame_, R=F, lens=ld, flags=fv)
    assert torch.equal(_bits(ev).cpu(), torch.from_numpy(want_e).view(torch.int64)) and torch.equal(fv.cpu(), torch.from_numpy(want_f))
    eb, fb = e_full.view(torch.uint8).cpu(), f_full.cpu()
    assert bool((eb[:, :16] == GUARD).all()) and bool((eb[:, 8 * (F + 2):] == GUARD).all())
    assert bool((fb[:, :3] == GUARD).all()) and bool((fb[:, F + 3:] == GUARD).all())


CHUNKINGS = {
    "480s": lambda T: [480] * (T // 480) + ([T % 480] if T % 480 else []),
    "odd": lambda T: [1, 299, 301, 7, 1024, 3, 600, 2, 297, 1500, 64],
    "all": lambda T: [T],
}


@pytest.mark.parametrize("chunking", sorted(CHUNKINGS))
@pytest.mark.parametrize("B", [1, 3])
def test_voice_activity_is_chunk_invariant(chunking, B, cuda):
    """Pushes of any sizes, then finish(): flags and energies are ops.vad's on the whole signal, bit for bit -- with the ring just
    above W + H + the most frames a push completes, so it wraps several times."""
    from facodec_amd import ops
    from facodec_amd.streaming import VoiceActivity
    T = 480 * 30 + 123
    x = torch.from_numpy(_signal(B, T, seed=77 + B)).to(cuda)
    want_f, want_e = ops.vad(x, window=W_S, hangover=H_S)
    sizes, left = [], T
    for n in CHUNKINGS[chunking](T) * 20:
        if left == 0:
            break
        sizes.append(min(n, left))
        left -= sizes[-1]
    assert left == 0
    most = max(-(-n // 300) + 1 for n in sizes)
    va = VoiceActivity(B, window=W_S, hangover=H_S, ring=W_S + H_S + most + 1, device=cuda)
    fl, en, t = [], [], 0
    for i, n in enumerate(sizes):
        blk = x[:, t:t + n]
        va.push(blk[:, None, :] if i % 2 else blk)
        t += n
        new = va.frames - va.taken
        if new:
            en.append(va.energies(new))
            fl.append(va.take(new))
    va.finish()
    new = va.frames - va.taken
    if new:
        en.append(va.energies(new))
        fl.append(va.take(new))
    va.finish()                                                          # idempotent
    assert va.frames == want_f.shape[1] == -(-T // 300)
    if chunking != "all":
        assert va.frames > 3 * va.R                                      # the ring has wrapped
    assert torch.equal(torch.cat(fl, 1), want_f)
    assert torch.equal(_bits(torch.cat(en, 1)), _bits(want_e))
    with pytest.raises(RuntimeError):
        va.push(x[:, :10])


def test_take_into_a_strided_view_and_its_two_errors(cuda):
    from facodec_amd import ops
    from facodec_amd.streaming import VoiceActivity
    B, R = 2, 12
    x = torch.from_numpy(_signal(B, 300 * 40, seed=9)).to(cuda)
    want = ops.vad(x, window=W_S, hangover=H_S)[0]
    va = VoiceActivity(B, window=W_S, hangover=H_S, ring=R, device=cuda)
    with pytest.raises(ValueError, match="not yet taken"):
        va.take(1)
    va.push(x[:, :300 * 5])
    big = torch.full((B, 40), GUARD, dtype=torch.uint8, device=cuda)
    out = va.take(3, out=big[:, 30:33])                                  # the tail columns of another buffer
    assert out.data_ptr() == big[:, 30:33].data_ptr() and torch.equal(big[:, 30:33], want[:, :3])
    assert bool((big[:, :30] == GUARD).all()) and bool((big[:, 33:] == GUARD).all())
    with pytest.raises(ValueError, match="not yet taken"):
        va.take(3)                                                       # too early: two frames are left
    with pytest.raises(ValueError):
        va.take(2, out=big[:, :3])                                       # the wrong shape
    assert torch.equal(va.take(2), want[:, 3:5])
    for j in range(5, 5 + R + 1, 3):                                     # 15 more frames, none taken
        va.push(x[:, 300 * j:300 * (j + 3)])
    assert va.frames == 20 and va.taken == 5
    with pytest.raises(ValueError, match="has left the ring"):
        va.take(1)                                                       # frame 5 was overwritten by frame 17
    with pytest.raises(ValueError, match="completes"):
        va.push(x[:, :300 * (R - W_S - H_S + 1)])                        # more frames than the ring can decide in one push


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("k", [1, 2, 16])
def test_sid_apply_matches_numpy(B, k, cuda):
    """STORE, FILL and PASS rows side by side, sid_k in {1, 2, 3} and the k of an earlier STORE, phases that wrap; codes beyond
    2^32; the buffers' unused columns, PASS rows and the store of rows that do not STORE keep their guard pattern."""
    from facodec_amd import ops
    rng = np.random.default_rng(B * 100 + k)
    Q, pad = sum(N_Q), 3
    store = rng.integers(-2 ** 40, 2 ** 40, (B, Q, _lib.PLC_MAX_FRAMES))
    store_d = torch.from_numpy(store).to(cuda)
    for trial, sid_k in enumerate([1, 2, 3, k, 0, 17]):
        full = [rng.integers(0, 2 ** 40, (B, n, k + pad)) for n in N_Q]
        full_d = [torch.from_numpy(f).to(cuda) for f in full]
        dst_d = [f[:, :, 1:k + 1] for f in full_d]
        kinds = [(trial + b) % 3 for b in range(B)]                      # every kind in every position over the trials
        if B == 1:
            kinds = [_lib.SID_FILL if trial % 2 == 0 else _lib.SID_STORE]
        phases = [int(rng.integers(0, max(sid_k, 1))) if sid_k <= 16 else 3 for _ in range(B)]
        words = [kd | ph << 8 | (k if kd == _lib.SID_STORE else sid_k) << 16 for kd, ph in zip(kinds, phases)]
        if B == 5:
            words[4] = 7 | 1 << 8 | 2 << 16                              # an unknown kind passes
            kinds[4] = _lib.SID_PASS
        want_full, want_store = [f.copy() for f in full], store.copy()
        offs = [0, N_Q[0], N_Q[0] + N_Q[1]]
        for b in range(B):
            for r in range(3):
                for i in range(N_Q[r]):
                    q = offs[r] + i
                    if kinds[b] == _lib.SID_STORE:
                        want_store[b, q, :k] = full[r][b, i, 1:k + 1]
                    elif kinds[b] == _lib.SID_FILL and 1 <= sid_k <= 16:
                        for f in range(k):
                            want_full[r][b, i, 1 + f] = store[b, q, (phases[b] + f) % sid_k]
        ops.sid_apply(dst_d, torch.tensor(words, dtype=torch.int32, device=cuda), store_d, N_Q)
        for r in range(3):
            assert np.array_equal(full_d[r].cpu().numpy(), want_full[r]), (trial, r)
        assert np.array_equal(store_d.cpu().numpy(), want_store), trial
        store = want_store
    with pytest.raises(ValueError):
        ops.sid_apply(dst_d, torch.zeros(B, dtype=torch.int64, device=cuda), store_d, N_Q)
    with pytest.raises(ValueError):
        ops.sid_apply(dst_d, torch.zeros(B, dtype=torch.int32, device=cuda), store_d[:, :, :8], N_Q)


def test_clip_lists_find_and_trim_the_speech(cuda):
    from facodec_amd import commons, ops
    rng = np.random.default_rng(12)
    specs = [(2500, [(4, 7)]), (1234, []), (9050, [(3, 5), (20, 23)]), (301, [])]      # bursts under W frames: every frame is raw
    waves = []
    for T, bursts in specs:
        x = rng.standard_normal(T) * 1e-3
        for a, b in bursts:
            x[a * 300:b * 300 - 1] = rng.standard_normal((b - a) * 300 - 1) * 1e-1
        waves.append(torch.from_numpy(x.astype(np.float32)).to(cuda))
    waves[2] = waves[2][None, :]
    got = commons.vad_clips(waves, window=W_S, hangover=2)
    for (T, bursts), w, g in zip(specs, waves, got):
        want = vad_ref(w.reshape(-1).cpu().numpy(), 300, W_S, 2)[0]
        assert g["flags"].dtype == np.uint8 and np.array_equal(g["flags"], want), T
        assert g["segments"] == [(a * 300, min((b + 2) * 300, T)) for a, b in bursts], (T, g["segments"])
        alone = ops.vad(w.reshape(1, -1), window=W_S, hangover=2)[0][0].cpu().numpy()      # what the clip gets alone
        assert np.array_equal(g["flags"], alone)
    trimmed = commons.trim_clips(waves, window=W_S, hangover=2)
    assert [tuple(t.shape) for t in trimmed] == [(1300,), (0,), (1, 6600), (0,)]
    assert trimmed[0].data_ptr() == waves[0][1200:].data_ptr() and torch.equal(trimmed[2], waves[2][:, 900:7500])
    padded = commons.trim_clips(waves, pad_frames=5, window=W_S, hangover=2)
    assert tuple(padded[0].shape) == (2500,) and tuple(padded[2].shape) == (1, 9000) and padded[1].numel() == 0
    assert commons.vad_clips([]) == []
    with pytest.raises(ValueError):
        commons.vad_clips(waves, window=0)


# ------------------------------------------------------------------------------------------------ the link, end to end
SID_EVERY = 8
T_SILENT, T_SPEAKS = 20, 27                      # row 1 falls silent at push 20; row 2 is silent until push 27


@pytest.fixture(scope="module")
def dtx_link(full_model, cuda):
    """One sender session over three streams, 60 pushes: row 0 speaks throughout, row 1 falls silent, row 2 starts silent.  The
    flags are scripted (the detector itself is held to its restatement above)."""
    from facodec_amd.streaming import CodePacketizer
    timbre, chunks = _session(full_model, 3, 60, 46, cuda)
    n = len(chunks)
    assert n >= 58
    act = []
    for j, c in enumerate(chunks):
        a = torch.zeros(3, c[0].shape[-1], dtype=torch.uint8)
        a[0] = 1
        a[1] = 1 if j < T_SILENT else 0
        a[2, -1] = 0 if j < T_SPEAKS else 1                              # one active frame is enough
        act.append(a.to(cuda))
    tx = CodePacketizer(N_Q, dtx=dict(sid_every=SID_EVERY))
    plain = CodePacketizer(N_Q)
    headers = tx.header(timbre)
    sent = [tx.packet(c, a) for c, a in zip(chunks, act)]
    full = [plain.packet(c) for c in chunks]
    host = [[c.cpu().numpy() for c in ch] for ch in chunks]
    return dict(timbre=timbre, chunks=chunks, host=host, headers=headers, sent=sent, full=full, n=n)


def test_sender_suppresses_silent_pushes(dtx_link):
    s = dtx_link
    for j, (got, full) in enumerate(zip(s["sent"], s["full"])):
        assert got[0] == full[0]                                                      # an active row: the bytes of before
        s1 = j - T_SILENT
        want1 = "n" if s1 < 0 else ("s" if s1 % SID_EVERY == 0 else None)
        want2 = "n" if j >= T_SPEAKS else ("s" if j % SID_EVERY == 0 else None)
        for b, want in ((1, want1), (2, want2)):
            p = got[b]
            if want is None:
                assert p is None, (j, b)
            elif want == "n":
                assert p == full[b], (j, b)
            else:
                assert p[:2] == b"Fp" and p[2:-4] == full[b][2:-4] and p != full[b], (j, b)
    sent = sum(len(p) for got in s["sent"] for p in got if p is not None)
    assert sent < 0.75 * sum(len(p) for full in s["full"] for p in full)


def _substituted(s, packets_per_tick):
    """Per tick the codes a DTX receiver plays when nothing is lost, from the definition: a packet's own codes, or the last SID
    packet's frames, cycled from where the last comfort push stopped."""
    out, sid, phase = [], [None] * 3, [0] * 3
    for j, packets in enumerate(packets_per_tick):
        codes = [c.copy() for c in s["host"][j]]
        k = codes[0].shape[-1]
        for b, p in enumerate(packets):
            if p is not None and p[:2] == b"Fp":
                sid[b], phase[b] = [c[b].copy() for c in s["host"][j]], 0
            elif p is None:
                sk = sid[b][0].shape[-1]
                for r in range(3):
                    for f in range(k):
                        codes[r][b, :, f] = sid[b][r][:, (phase[b] + f) % sk]
                phase[b] = (phase[b] + k) % sk
        out.append(codes)
    return out


def test_dtx_receiver_plays_comfort_frames_bit_for_bit(full_model, dtx_link, cuda, monkeypatch):
    """Nothing lost.  Row 0 is the dtx=False receiver's row on every tick; every row is a plain StreamingDecoder fed the
    substituted codes (the SID packet's frames, cycled), bit for bit; comfort frames are counted as such and nothing as
    concealed; a steady-state tick reads nothing back."""
    from facodec_amd.streaming import StreamingDecoder, StreamingReceiver
    s = dtx_link
    rx = StreamingReceiver(full_model, s["headers"], dtx=True)
    rx0 = StreamingReceiver(full_model, s["headers"])
    sub = StreamingDecoder(full_model, s["timbre"])
    want_codes = _substituted(s, s["sent"])
    comfort = [0, 0, 0]
    for j, p in enumerate(s["sent"]):
        k = s["host"][j][0].shape[-1]
        plain = (sub.prime if j == 0 else sub.push)([torch.from_numpy(c).to(cuda) for c in want_codes[j]]).clone()
        if j == 0:
            got, got0 = rx.prime(p), rx0.prime(s["full"][0])
        else:
            if j >= 16:                                                  # every graph of the 5-hop period is captured by now
                with _NoReadback(monkeypatch) as spy:
                    got = rx.tick(p)
                assert spy.calls == [], (j, spy.calls)
            else:
                got = rx.tick(p)
            got0 = rx0.tick([p[0], None, None])
        assert torch.equal(got[0], got0[0]), j
        assert torch.equal(got, plain), j
        assert rx.last_status == [_lib.PLC_PRIMARY] * 3
        for b in range(3):
            comfort[b] += k if p[b] is None else 0
    assert comfort[0] == 0 and comfort[1] > 0 and comfort[2] > 0
    n_sent = [sum(p[b] is not None for p in s["sent"]) for b in range(3)]
    assert rx.stats == [dict(received=n_sent[b], recovered=0, concealed=0, corrupt=0, misordered=0, comfort=comfort[b]) for b in range(3)]
    assert [r["in_dtx"] for r in rx._dtx_rows] == [False, True, False]


def test_a_dropped_first_sid_is_concealed_and_dtx_starts_at_the_refresh(full_model, dtx_link, cuda):
    """Row 1's first SID packet is lost: the pushes up to the refresh are LOST (concealed, fading), the refresh enters DTX and the
    pushes behind it are comfort frames.  A receiver with sid_timeout = 3 leaves DTX again and conceals.  Row 0 never notices."""
    from facodec_amd.streaming import StreamingReceiver
    s = dtx_link
    rx = StreamingReceiver(full_model, s["headers"], dtx=True)
    rxt = StreamingReceiver(full_model, s["headers"], dtx=True, sid_timeout=3)
    rx0 = StreamingReceiver(full_model, s["headers"])
    concealed = comfort = concealed_t = comfort_t = 0
    for j, p in enumerate(s["sent"]):
        k = s["host"][j][0].shape[-1]
        p = list(p)
        if j == T_SILENT:
            assert p[1][:2] == b"Fp"
            p[1] = None
        if j == 0:
            got, got_t, got0 = rx.prime(p), rxt.prime(p), rx0.prime(s["full"][0])
        else:
            got, got_t, got0 = rx.tick(p), rxt.tick(p), rx0.tick([p[0], None, None])
        assert torch.equal(got[0], got0[0]) and torch.equal(got_t[0], got0[0]), j
        if T_SILENT <= j < T_SILENT + SID_EVERY:
            assert rx.last_status[1] == _lib.PLC_LOST and not rx._dtx_rows[1]["in_dtx"], j
            concealed += k
            concealed_t += k
        elif j >= T_SILENT + SID_EVERY:
            assert rx.last_status[1] == _lib.PLC_PRIMARY and rx._dtx_rows[1]["in_dtx"], j
            since = (j - T_SILENT) % SID_EVERY                           # pushes since the last SID packet that arrived
            comfort += k if since else 0
            assert rxt.last_status[1] == (_lib.PLC_PRIMARY if since <= 3 else _lib.PLC_LOST), j
            comfort_t += k if 1 <= since <= 3 else 0
            concealed_t += k if since > 3 else 0
        if j == T_SILENT + 6:
            assert bool((got[1, 0, -300:] == 0).all())                   # hold 2, fade 6: silent by now
    assert rx.stats[1]["concealed"] == concealed > 0 and rx.stats[1]["comfort"] == comfort > 0
    assert rxt.stats[1]["concealed"] == concealed_t > concealed and rxt.stats[1]["comfort"] == comfort_t > 0
    assert rx.stats[0]["concealed"] == rx.stats[0]["comfort"] == 0 and rx.stats[2]["concealed"] == 0 and rx.stats[2]["comfort"] > 0
    with pytest.raises(ValueError, match="pass k="):
        rx.tick([None, None, None])
    assert rx.tick([None, None, None], k=2).shape == (3, 1, 600)


def test_packet_with_flags_is_one_copy_and_take_writes_into_the_pack_buffer(dtx_link, cuda, monkeypatch):
    from facodec_amd.streaming import CodePacketizer, VoiceActivity
    s = dtx_link
    codes = s["chunks"][3]
    k = codes[0].shape[-1]
    va = VoiceActivity(3, window=W_S, hangover=H_S, ring=64, device=cuda)
    x = torch.from_numpy(_signal(3, 300 * 12, seed=4)).to(cuda)
    x[1] = 0                                                             # a silent row
    va.push(x)
    va.take(12 - k)
    want = va._flags[:, 12 - k:12].clone()
    tx, ty = (CodePacketizer(N_Q, redundancy=(1, 2, 0), dtx=dict(sid_every=2)) for _ in range(2))
    view = tx.active_view(3, k, cuda)
    assert va.take(k, out=view) is view
    with _NoReadback(monkeypatch) as spy:
        got = tx.packet(codes, view)
    assert spy.calls.count("cpu") == 1 and set(spy.calls) <= {"cpu", "numpy"}, spy.calls
    assert got == ty.packet(codes, want)                                 # the same bytes from a tensor of its own
    assert got[1][:2] == b"Fq" and got[0][:2] == (b"FQ" if bool(want[0].any()) else b"Fq")
    with pytest.raises(ValueError):
        tx.packet(codes, want.to(torch.int32))
    with pytest.raises(ValueError, match="without dtx"):
        CodePacketizer(N_Q).packet(codes, want)


def test_defaults_give_the_bytes_and_bits_of_before(full_model, dtx_link, cuda):
    from facodec_amd.streaming import CodePacketizer, StreamingReceiver
    s = dtx_link
    for red in (None, (1, 2, 0)):
        a, b = CodePacketizer(N_Q, redundancy=red), CodePacketizer(N_Q, redundancy=red, dtx=None)
        for c in s["chunks"][:8]:
            assert a.packet(c) == b.packet(c, active=None)
    rxa = StreamingReceiver(full_model, s["headers"])
    rxb = StreamingReceiver(full_model, s["headers"], dtx=False, sid_timeout=24)
    for j, p in enumerate(s["full"][:14]):
        p = [p[0], None if j in (5, 6) else p[1], p[2]]
        wa, wb = ((rx.prime if j == 0 else rx.tick)(p) for rx in (rxa, rxb))
        assert torch.equal(wa, wb), j
    assert rxa.stats == rxb.stats and "comfort" not in rxa.stats[0] and rxa.stats[1]["concealed"] > 0
    assert rxa.reader.feed([s["sent"][T_SILENT][1], None, None])[0] is None and rxa.reader.corrupt[0] == 1   # a SID packet without dtx
