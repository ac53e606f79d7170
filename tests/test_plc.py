"""Surviving packet loss on the device: fac_vq_decode_masked against fac_vq_decode (bit for bit), fac_plc_select
and fac_plc_gain against the numpy restatement of tests/test_plc_cpu.py (bit for bit), LayeredDecoder against StreamingDecoder
and the offline blend, StreamingReceiver against the lossless pair, the substituted-codes decoder and the restatement's gain."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from facodec_amd import _lib, bitstream, synth
from test_plc_cpu import LOST, POLICIES, PRIMARY, REDUNDANT, PlcRef, fq_ref, gain_ref, red_rows

E2E_TOL = 1e-4                                   # the streaming-versus-offline bound of tests/test_decode_codes.py
N_Q, N_RED = (1, 2, 3), (1, 2, 0)

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------ fac_vq_decode_masked
def _weights(n_q, D, Kc, gen, dev, no_scale):
    from facodec_amd import ops
    ws = []
    for n in n_q:
        w_r = []
        for _ in range(n):
            cb = torch.randn(Kc, 8, generator=gen).to(dev)
            v = (torch.randn(D, 8, 1, generator=gen) * 0.3).to(dev)
            g = (torch.rand(D, 1, 1, generator=gen) + 0.5).to(dev)
            b = (torch.randn(D, generator=gen) * 0.1).to(dev)
            w_r.append((cb, v, None if no_scale else ops.wn_scale(v, g), b))
        ws.append(w_r)
    return ws


def _plain(codes, ws, style, Kc, tri, B, D, T):
    """fac_vq_decode with n_q = tri: the first tri[r] code rows and weight sets of each RVQ -> (outs, z_p, z_c, z_r)."""
    from facodec_amd import ops
    z = [torch.full((B, D, T), float("nan"), device=style.device) for _ in range(3)]
    if sum(tri):
        outs = ops.vq_decode([c[:, :a] if a else None for c, a in zip(codes, tri)], [w[:a] for w, a in zip(ws, tri)], style, Kc, z_out=z)
    else:                                        # no quantizer at all: ops.vq_decode has no frame count then; the C entry has
        outs = torch.full((B, D, T), float("nan"), device=style.device)
        d = _lib.VqDecodeDesc()
        d.style, d.outs = style.data_ptr(), outs.data_ptr()
        for r in range(3):
            d.z[r] = z[r].data_ptr()
        d.B, d.D, d.T, d.Kc = B, D, T, Kc
        _lib.check(_lib.load().fac_vq_decode(ctypes.byref(d), ops._stream()), "fac_vq_decode")
    return [outs] + z


def _masked(codes, ws, style, Kc, n_use, B, D, T, out=None):
    from facodec_amd import ops
    z = [torch.full((B, D, T), float("nan"), device=style.device) for _ in range(3)]
    outs = ops.vq_decode(codes, ws, style, Kc, out=out, z_out=z, n_use=n_use)
    return [outs] + z


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("n_q", [(1, 2, 3), (1, 2, 0), (2, 0, 1)])
@pytest.mark.parametrize("D,Kc", [(96, 37), (96, 1024), (1024, 37), (1024, 1024)])
def test_masked_decode_equals_the_plain_decode_with_those_counts(D, Kc, n_q, cuda):
    """Per (B, T): every uniform triple <= n_q against fac_vq_decode with that n_q on outs and all z[r]; random per-(b, t) counts
    frame by frame against those uniform launches; garbage codes in skipped rows; counts outside [0, n_q]; a strided n_use view;
    n_use=None; a 0xA5 guard around outs."""
    from facodec_amd import ops
    gen = torch.Generator().manual_seed(D * 7 + Kc + sum(n_q) * 100 + n_q[0])
    ws = _weights(n_q, D, Kc, gen, cuda, no_scale=(D == 96))
    triples = list(itertools.product(*[range(n + 1) for n in n_q]))
    nq_t = torch.tensor(n_q, dtype=torch.int32, device=cuda)
    for B in (1, 3):
        for T in (1, 2, 3, 16, 17, 40):
            codes = [torch.randint(0, Kc, (B, n + 2, T + 3), generator=gen).to(cuda)[:, 1:1 + n, 2:2 + T] if n else None for n in n_q]
            style = torch.cat([torch.rand(B, D, generator=gen) + 0.5, torch.randn(B, D, generator=gen) * 0.2], 1).to(cuda)
            tag = (B, T)
            plain = {}
            for tri in triples:
                plain[tri] = _plain(codes, ws, style, Kc, tri, B, D, T)
                nu = torch.tensor(tri, dtype=torch.int32, device=cuda).expand(B, T, 3).contiguous()
                assert _same(_masked(codes, ws, style, Kc, nu, B, D, T), plain[tri]), (tag, tri)
            assert _same(plain[n_q], [ops.vq_decode(codes, ws, style, Kc)] + plain[n_q][1:]), tag
            assert torch.equal(ops.vq_decode(codes, ws, style, Kc, n_use=None), plain[n_q][0]), tag
            # random counts per (b, t): every frame equals the frame of the uniform launch with its triple
            nu = torch.stack([torch.randint(0, n + 1, (B, T), generator=gen) for n in n_q], -1).to(torch.int32).to(cuda)
            want = [torch.zeros(B, D, T, device=cuda) for _ in range(4)]
            for tri in triples:
                m = (nu == torch.tensor(tri, dtype=torch.int32, device=cuda)).all(-1)[:, None, :]
                want = [torch.where(m, p, w) for p, w in zip(plain[tri], want)]
            n = B * D * T
            guard = torch.full(((n + 512) * 4,), 0xA5, dtype=torch.uint8, device=cuda)
            out = guard.view(torch.float32)[256:256 + n].view(B, D, T)
            got = _masked(codes, ws, style, Kc, nu, B, D, T, out=out)
            assert got[0].data_ptr() == out.data_ptr() and _same(got, want), tag
            assert bool((guard[:1024] == 0xA5).all()) and bool((guard[(256 + n) * 4:] == 0xA5).all()), tag
            # codes of skipped quantizers may be anything
            junk = []
            for r, c in enumerate(codes):
                if c is None:
                    junk.append(None)
                    continue
                idx = torch.arange(n_q[r], device=cuda)[None, :, None]
                skipped = idx >= nu[:, :, r][:, None, :]
                bad = torch.where((torch.arange(T, device=cuda) & 1).bool(), torch.tensor(-7, device=cuda), torch.tensor(1 << 40, device=cuda))
                junk.append(torch.where(skipped, bad[None, None, :].expand_as(c), c))
            assert _same(_masked(junk, ws, style, Kc, nu, B, D, T), want), tag
            # counts outside [0, n_q[r]] are clamped
            wild = torch.where(nu >= nq_t, nu + 1000, torch.where(nu <= 0, nu - 5, nu))
            assert _same(_masked(codes, ws, style, Kc, wild, B, D, T), want), tag
            # a strided view of a larger count buffer
            big = torch.full((B, T + 3, 4), 77, dtype=torch.int32, device=cuda)
            big[:, 2:2 + T, :3] = nu
            view = big[:, 2:2 + T, :3]
            assert not view.is_contiguous() or T == 1
            assert _same(_masked(codes, ws, style, Kc, view, B, D, T), want), tag


def test_masked_decode_python_surface_refuses(cuda):
    from facodec_amd import ops
    gen = torch.Generator().manual_seed(5)
    ws = _weights((1, 1, 0), 96, 37, gen, cuda, True)
    codes = [torch.zeros(2, 1, 4, dtype=torch.int64, device=cuda)] * 2 + [None]
    style = torch.ones(2, 192, device=cuda)
    nu = torch.ones(2, 4, 3, dtype=torch.int32, device=cuda)
    ops.vq_decode(codes, ws, style, 37, n_use=nu)
    with pytest.raises(_lib.FacodecHipError):
        ops.vq_decode(codes, ws, style, 37, n_use=nu.cpu())
    for bad in (nu.long(), nu[:, :3], nu[:1], torch.ones(2, 4, 6, dtype=torch.int32, device=cuda)[:, :, ::2]):
        with pytest.raises(ValueError):
            ops.vq_decode(codes, ws, style, 37, n_use=bad)


# ------------------------------------------------------------------------------------------------ fac_plc_select / fac_plc_gain
def _state_equal(state, ref):
    return (np.array_equal(state.last_codes.cpu().numpy(), ref.last_codes) and np.array_equal(state.last_n.cpu().numpy(), ref.last_n)
            and state.g.cpu().numpy().tobytes() == ref.g.tobytes() and np.array_equal(state.run.cpu().numpy(), ref.run))


@pytest.mark.parametrize("alias", [True, False])
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("B", [1, 5])
def test_plc_select_matches_the_restatement_over_twenty_ticks(B, policy, alias, cuda):
    """Twenty seeded ticks with k cycling over 1, 2, 3, 16 and every status (3 and -1 included) carry the state along; every
    output and the whole state are compared after every tick.  alias: dst is the primary buffer (a [:, :, :k] slice of a static
    (B, n, 16) buffer, as in the receiver), else separate dense tensors (and the primary codes stay what they were)."""
    from facodec_amd import ops
    rng = np.random.default_rng(B * 31 + policy[1] + alias)
    ref = PlcRef(B, N_Q, *policy)
    state = ops.PlcState(B, N_Q, cuda)
    static = [torch.zeros(B, n, 16, dtype=torch.int64, device=cuda) for n in N_Q]
    seen = set()
    for tick in range(20):
        k = (1, 2, 3, 16)[tick % 4]
        if tick == 0:
            status = np.zeros(B, np.int32)
        elif tick < 6:
            status = np.array([(0, 1, 2, 3, -1)[(tick + b) % 5] for b in range(B)], np.int32)
        else:
            status = rng.choice(np.array([0, 0, 1, 2, 2, 2, 3, -1], np.int32), B)
        seen |= set(status.tolist())
        with_red = tick % 5 != 4                                   # every fifth tick has no redundant layer: REDUNDANT is LOST
        prim = [rng.integers(0, 1024, (B, n, k)) for n in N_Q]
        red = [rng.integers(0, 1024, (B, n, k)) for n in N_RED] if with_red else None
        want_dst, want_n, want_ramp = ref.select(prim, red, N_RED, status)
        p_dev = [s[:, :, :k] for s in static] if alias else [torch.empty(B, n, k, dtype=torch.int64, device=cuda) for n in N_Q]
        for d, p in zip(p_dev, prim):
            d.copy_(torch.from_numpy(p))
        dst = p_dev if alias else [torch.full((B, n, k), -1, dtype=torch.int64, device=cuda) for n in N_Q]
        r_dev = [torch.from_numpy(r).to(cuda) for r in red] if with_red else None
        n_use = torch.full((B, 16, 3), -9, dtype=torch.int32, device=cuda)
        ramp = torch.full((B, k + 1), float("nan"), device=cuda)
        ops.plc_select(p_dev, r_dev, torch.from_numpy(status).to(cuda), state, dst, n_use[:, :k], ramp,
                       N_RED if with_red else (0, 0, 0), *policy)
        for r in range(3):
            assert np.array_equal(dst[r].cpu().numpy(), want_dst[r]), (tick, r)
            if not alias:
                assert np.array_equal(p_dev[r].cpu().numpy(), prim[r]), (tick, r)
        assert np.array_equal(n_use[:, :k].cpu().numpy(), want_n) and bool((n_use[:, k:] == -9).all()), tick
        assert ramp.cpu().numpy().tobytes() == want_ramp.tobytes(), (tick, ramp, want_ramp)
        assert _state_equal(state, ref), tick
    assert seen >= ({0, 1, 2, 3, -1} if B > 1 else {0, 1, 2})


@pytest.mark.parametrize("B", [1, 5])
def test_plc_gain_matches_the_restatement_bit_for_bit(B, cuda):
    """Ramps from the restatement's own fades and recoveries and random ones; k in {1, 2, 3, 16}; in place and out of place; a
    flat ramp of ones returns the input bits."""
    from facodec_amd import ops
    rng = np.random.default_rng(B)
    ref = PlcRef(B, N_Q, 1, 3, 3)
    prim = lambda k: [np.zeros((B, n, k), np.int64) for n in N_Q]
    for i, k in enumerate((1, 2, 3, 16, 3, 2, 1, 16)):
        status = [LOST if (i + b) % 3 else PRIMARY for b in range(B)] if i < 6 else [PRIMARY] * B
        _, _, ramp = ref.select(prim(k), None, (0, 0, 0), status)
        if i == 4:
            ramp = rng.random((B, k + 1)).astype(np.float32)
        wave = rng.standard_normal((B, 1, 300 * k)).astype(np.float32)
        want = gain_ref(wave.reshape(B, -1), ramp).reshape(wave.shape)
        x = torch.from_numpy(wave).to(cuda)
        r = torch.from_numpy(ramp).to(cuda)
        y = ops.plc_gain(x, r)
        assert y.data_ptr() != x.data_ptr() and y.cpu().numpy().tobytes() == want.tobytes(), (i, k)
        assert x.cpu().numpy().tobytes() == wave.tobytes()
        y2 = ops.plc_gain(x, r, out=x)
        assert y2.data_ptr() == x.data_ptr() and x.cpu().numpy().tobytes() == want.tobytes(), (i, k)
        for b in range(B):
            if np.all(ramp[b] == 1.0):
                assert want[b].tobytes() == wave[b].tobytes()
    ones = torch.ones(B, 17, device=cuda)
    x = torch.randn(B, 4800, device=cuda)
    assert torch.equal(ops.plc_gain(x, ones), x)
    with pytest.raises(ValueError):
        ops.plc_gain(x[:, :4799], ones)


# ------------------------------------------------------------------------------------------------ sessions
@pytest.fixture(scope="module")
def full_model(cuda):
    from facodec_amd.commons import build_model, default_model_params
    model = build_model(default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(cuda)
    return model


def _session(m, B, n_hops, seed, cuda):
    """The code chunks a StreamingCodec session over B streams emits -> (timbre, [codes per push])."""
    from facodec_amd.streaming import HOP, StreamingCodec
    wave = synth.synth_clips(B, 4800 + n_hops * HOP, seed=seed).to(cuda)
    with torch.no_grad():
        timbre = m.quantizer(m.encoder(wave), wave, n_c=2, return_codes=True)[4].clone()
    sess = StreamingCodec(m, timbre, n_c=2, use_graphs=True)
    outs = [sess.prime(wave[:, :, :4800])]
    outs += [sess.push(wave[:, :, 4800 + h * HOP:4800 + (h + 1) * HOP]) for h in range(n_hops)]
    chunks = [[c.clone() for c in o["codes"]] for o in outs if o["codes"] is not None]
    fin = sess.finish()
    if fin["codes"] is not None:
        chunks.append([c.clone() for c in fin["codes"]])
    return timbre, chunks


def _run(rx, chunks, n_use=None, cut=None):
    """prime + push of every chunk -> the concatenated wave.  n_use: per chunk a (B, k, 3) tensor or None; cut: row counts the
    codes are cut to (for a plain StreamingDecoder session at a lower rate)."""
    waves = []
    for i, c in enumerate(chunks):
        if cut is not None:
            c = [x[:, :n] for x, n in zip(c, cut)]
        args = (c,) if n_use is None else (c, n_use[i])
        waves.append((rx.prime if i == 0 else rx.push)(*args).clone())
    return torch.cat(waves, -1)


@pytest.fixture(scope="module")
def two_streams(full_model, cuda):
    from facodec_amd.streaming import StreamingDecoder
    m = full_model
    timbre, chunks = _session(m, 2, 25, 11, cuda)
    full = _run(StreamingDecoder(m, timbre), chunks)
    low = _run(StreamingDecoder(m, timbre), chunks, cut=N_RED)
    return dict(timbre=timbre, chunks=chunks, full=full, low=low)


def _counts(chunks, rows, cuda):
    """Per chunk a (B, k, 3) int32 tensor with row b at rows[b]."""
    return [torch.tensor(rows, dtype=torch.int32, device=cuda)[:, None, :].expand(len(rows), c[0].shape[-1], 3).contiguous() for c in chunks]


def test_layered_decoder_full_counts_are_the_streaming_decoder(full_model, two_streams, cuda):
    from facodec_amd.streaming import LayeredDecoder
    s = two_streams
    assert len(s["chunks"]) >= 20
    rx = LayeredDecoder(full_model, s["timbre"])
    assert torch.equal(_run(rx, s["chunks"]), s["full"])                     # n_use=None
    assert len(rx._graphs) >= 2
    got = _run(LayeredDecoder(full_model, s["timbre"]), s["chunks"], _counts(s["chunks"], [N_Q, N_Q], cuda))
    assert torch.equal(got, s["full"])


def test_layered_decoder_rows_at_different_rates_do_not_see_each_other(full_model, two_streams, cuda):
    """Uniform (1, 2, 0) is the StreamingDecoder session primed with [p, c, r[:, :0]]; with row 0 at the full rate and row 1 at
    (1, 2, 0), each row is its row of the corresponding uniform session, bit for bit."""
    from facodec_amd.streaming import LayeredDecoder
    s = two_streams
    assert not torch.equal(s["low"], s["full"])
    got = _run(LayeredDecoder(full_model, s["timbre"]), s["chunks"], _counts(s["chunks"], [N_RED, N_RED], cuda))
    assert torch.equal(got, s["low"])
    got = _run(LayeredDecoder(full_model, s["timbre"]), s["chunks"], _counts(s["chunks"], [N_Q, N_RED], cuda))
    assert torch.equal(got[0], s["full"][0]) and torch.equal(got[1], s["low"][1])


def _offline_blend(m, timbre, chunks, counts):
    """ops.vq_decode twice (full rate, (1, 2, 0)), torch.where per frame, model.decoder."""
    from facodec_amd import ops
    q = m.quantizer
    codes = [torch.cat([c[i] for c in chunks], -1) for i in range(3)]
    nu = torch.cat(counts, 1)
    ws = q.decode_weights()
    with torch.no_grad():
        style = q.timbre_linear(timbre.contiguous()).contiguous()
        hi = ops.vq_decode(codes, [w[:n] for w, n in zip(ws, N_Q)], style, q.prosody_quantizer.codebook_size)
        lo = ops.vq_decode([codes[0], codes[1], None], [w[:n] for w, n in zip(ws, N_RED)], style, q.prosody_quantizer.codebook_size)
        low = (nu == torch.tensor(N_RED, dtype=torch.int32, device=nu.device)).all(-1)
        assert bool((low | (nu == torch.tensor(N_Q, dtype=torch.int32, device=nu.device)).all(-1)).all())
        return m.decoder(torch.where(low[:, None, :], lo, hi))


def test_layered_decoder_counts_that_change_over_time(full_model, two_streams, cuda):
    """Counts that switch between the full rate and (1, 2, 0) per frame and per row: within E2E_TOL of the offline blend, and the
    same bits with graphs on and off."""
    from facodec_amd.streaming import LayeredDecoder
    s = two_streams
    gen = torch.Generator().manual_seed(8)
    counts = []
    for c in s["chunks"]:
        low = torch.rand(2, c[0].shape[-1], generator=gen) < 0.4
        counts.append(torch.where(low[:, :, None], torch.tensor(N_RED), torch.tensor(N_Q)).to(torch.int32).to(cuda))
    rx = LayeredDecoder(full_model, s["timbre"], use_graphs=True)
    got_g = _run(rx, s["chunks"], counts)
    assert len(rx._graphs) >= 2
    got_e = _run(LayeredDecoder(full_model, s["timbre"], use_graphs=False), s["chunks"], counts)
    assert torch.equal(got_g, got_e)
    off = _offline_blend(full_model, s["timbre"], s["chunks"], counts)
    assert got_g.shape == off.shape
    err = rel(got_g, off)
    print("layered vs offline blend: rel", err)
    assert err <= E2E_TOL
    assert rel(got_g, s["full"]) > 10 * E2E_TOL                          # and the lower rate is audible in the numbers
    with pytest.raises(ValueError):
        rx.push(s["chunks"][-1], counts[-1][:, :, :2])
    with pytest.raises(ValueError):
        rx.push(s["chunks"][-1], counts[-1].long())


# ------------------------------------------------------------------------------------------------ StreamingReceiver
@pytest.fixture(scope="module")
def three_streams(full_model, cuda):
    """One sender session over three streams as plain packets and as packets with the (1, 2, 0) redundant layer, and the
    lossless CodeDepacketizer + StreamingDecoder waves per push."""
    from facodec_amd.streaming import CodeDepacketizer, CodePacketizer, StreamingDecoder
    m = full_model
    timbre, chunks = _session(m, 3, 25, 46, cuda)
    tx, tq = CodePacketizer(N_Q), CodePacketizer(N_Q, redundancy=N_RED)
    headers = tx.header(timbre)
    fp = [tx.packet(c) for c in chunks]
    fq = [tq.packet(c) for c in chunks]
    rxc = CodeDepacketizer(headers)
    rx = StreamingDecoder(m, rxc.timbre)
    waves = [(rx.prime if i == 0 else rx.push)(rxc.feed(p)).clone() for i, p in enumerate(fp)]
    host = [[c.cpu().numpy() for c in ch] for ch in chunks]
    return dict(timbre=timbre, chunks=chunks, host=host, headers=headers, fp=fp, fq=fq, waves=waves)


def test_packetizer_with_redundancy_writes_the_restatements_bytes(three_streams):
    s = three_streams
    assert len(s["fq"]) >= 24
    for j, (ch, packets) in enumerate(zip(s["host"], s["fq"])):
        for b in range(3):
            allq = np.concatenate([c[b] for c in ch], 0)
            prev = red_rows([c[b] for c in s["host"][j - 1]], N_RED) if j else None
            assert packets[b] == fq_ref(j, allq, prev, N_RED, 10), (j, b)
    assert all(p[:2] == b"FP" for p in s["fp"][3]) and s["fp"][3][0] == bitstream.write_packet(3, s["host"][3][0].shape[-1],
                                                                                               s["fq"][3][0][11:11 + len(s["fp"][3][0]) - 10])


class _NoReadback:
    """Counts every way a tick could read the device back or wait for it."""
    NAMES = [(torch.Tensor, "cpu"), (torch.Tensor, "item"), (torch.Tensor, "tolist"), (torch.Tensor, "numpy"), (torch.cuda, "synchronize"),
             (torch.cuda.Stream, "synchronize"), (torch.cuda.Event, "synchronize")]

    def __init__(self, monkeypatch):
        self.mp, self.calls = monkeypatch, []

    def __enter__(self):
        for owner, name in self.NAMES:
            orig = getattr(owner, name)

            def spy(*a, _orig=orig, _name=name, **kw):
                self.calls.append(_name)
                return _orig(*a, **kw)
            self.mp.setattr(owner, name, spy)
        return self

    def __exit__(self, *exc):
        self.mp.undo()


def test_receiver_without_loss_is_the_lossless_pair(full_model, three_streams, cuda, monkeypatch):
    """delay=0: every tick's wave equals CodeDepacketizer + StreamingDecoder's; a steady-state tick reads nothing back.  delay=1
    (packets with the redundant layer): the same waves one tick later, flush() gives the last."""
    from facodec_amd.streaming import StreamingReceiver
    s = three_streams
    rx = StreamingReceiver(full_model, s["headers"])
    assert rx.min_prime == 10 and rx.n_q == N_Q
    assert torch.equal(rx.prime(s["fp"][0]), s["waves"][0])
    for i, p in enumerate(s["fp"][1:], 1):
        if i >= 16:                                                   # every graph of the 5-hop period is captured by now
            with _NoReadback(monkeypatch) as spy:
                w = rx.tick(p)
            assert spy.calls == [], (i, spy.calls)
        else:
            w = rx.tick(p)
        assert w.shape == s["waves"][i].shape and torch.equal(w, s["waves"][i]), i
    assert len(rx.dec._graphs) >= 2
    n = len(s["fp"])
    assert rx.stats == [dict(received=n, recovered=0, concealed=0, corrupt=0, misordered=0)] * 3
    rx = StreamingReceiver(full_model, s["headers"], delay=1)
    assert torch.equal(rx.prime(s["fq"][0]), s["waves"][0]) and rx.n_red == N_RED
    assert rx.tick(s["fq"][1]) is None
    for i in range(2, n):
        assert torch.equal(rx.tick(s["fq"][i]), s["waves"][i - 1]), i
    assert torch.equal(rx.flush(), s["waves"][n - 1]) and rx.flush() is None
    assert rx.stats == [dict(received=n, recovered=0, concealed=0, corrupt=0, misordered=0)] * 3 and rx.last_status == [PRIMARY] * 3


def test_receiver_conceals_one_row_and_leaves_its_neighbours_alone(full_model, three_streams, cuda):
    """Row 1 loses ticks 4-5 and 9-20 (delay=0).  Rows 0 and 2 are the lossless run on every tick.  Row 1 is a plain
    StreamingDecoder (same B) fed the substituted codes, which the restatement builds from the definition, times the restatement's
    gain -- bit for bit; exactly zero where the restatement's ramp is; and the substituted-codes decoder itself once the ramp is
    back at 1."""
    from facodec_amd.streaming import StreamingDecoder, StreamingReceiver
    s = three_streams
    lost = {4, 5} | set(range(9, 21))
    assert len(s["fp"]) > 23
    rx = StreamingReceiver(full_model, s["headers"])
    sub = StreamingDecoder(full_model, s["timbre"])
    ref = PlcRef(3, N_Q)
    zero_seen = back_at_one = False
    for i, p in enumerate(s["fp"]):
        status = [PRIMARY, LOST if i in lost else PRIMARY, PRIMARY]
        dst, n_use, ramp = ref.select(s["host"][i], None, (0, 0, 0), status)
        assert np.all(n_use == np.array(N_Q))                               # nothing but full-rate frames: a plain decoder will do
        codes = [torch.from_numpy(d).to(cuda) for d in dst]
        plain = (sub.prime if i == 0 else sub.push)(codes).clone()
        if i == 0:
            got = rx.prime(p)
        else:
            got = rx.tick([p[0], None if i in lost else p[1], p[2]])
        assert rx.last_status == status, i
        assert torch.equal(got[0], s["waves"][i][0]) and torch.equal(got[2], s["waves"][i][2]), i
        want = gain_ref(plain.cpu().numpy().reshape(3, -1), ramp)
        assert got.cpu().numpy().reshape(3, -1).tobytes() == want.tobytes(), i
        for f in range(ramp.shape[1] - 1):
            if ramp[1, f] == 0.0 and ramp[1, f + 1] == 0.0:
                zero_seen = True
                assert bool((got[1, 0, 300 * f:300 * (f + 1)] == 0).all()), (i, f)
        if i > 21 and np.all(ramp[1] == 1.0):
            back_at_one = True
            assert torch.equal(got[1], plain[1])
        if i in lost:
            assert not torch.equal(got[1], s["waves"][i][1])
    assert zero_seen and back_at_one
    frames = sum(s["host"][i][0].shape[-1] for i in lost)
    assert rx.stats[1] == dict(received=len(s["fp"]) - len(lost), recovered=0, concealed=frames, corrupt=0, misordered=0)
    assert rx.stats[0]["concealed"] == 0 and rx.stats[2]["received"] == len(s["fp"])


def test_receiver_recovers_a_lost_packet_from_the_redundant_layer(full_model, three_streams, cuda):
    """delay=1, packets with the (1, 2, 0) layer, the packet of push 6 lost on row 2: that push is played from packet 7's
    redundant layer (status REDUNDANT, stats.recovered == its frames) and the whole session is within E2E_TOL of the offline blend
    (full rate everywhere, (1, 2, 0) on row 2's frames of push 6)."""
    from facodec_amd.streaming import StreamingReceiver
    s = three_streams
    n = len(s["fq"])
    rx = StreamingReceiver(full_model, s["headers"], delay=1)
    waves = [rx.prime(s["fq"][0]).clone()]
    assert rx.tick(s["fq"][1]) is None
    for i in range(2, n):
        p = list(s["fq"][i])
        if i == 6:
            p[2] = None
        w = rx.tick(p)                                                       # plays push i - 1
        assert rx.last_status == [PRIMARY, PRIMARY, REDUNDANT if i - 1 == 6 else PRIMARY], i
        if i - 1 == 6:
            assert not torch.equal(w[2], s["waves"][6][2]) and torch.equal(w[:2], s["waves"][6][:2])
        waves.append(w.clone())
    waves.append(rx.flush().clone())
    k6 = s["host"][6][0].shape[-1]
    assert rx.stats[2] == dict(received=n - 1, recovered=k6, concealed=0, corrupt=0, misordered=0)
    assert rx.stats[0]["recovered"] == 0
    counts = []
    for i, ch in enumerate(s["chunks"]):
        c = torch.tensor(N_Q, dtype=torch.int32, device=cuda).expand(3, ch[0].shape[-1], 3).clone()
        if i == 6:
            c[2] = torch.tensor(N_RED, dtype=torch.int32, device=cuda)
        counts.append(c)
    off = _offline_blend(full_model, s["timbre"], s["chunks"], counts)
    got = torch.cat(waves, -1)
    err = rel(got, off)
    print("receiver with one recovered push vs offline blend: rel", err)
    assert got.shape == off.shape and err <= E2E_TOL


def test_receiver_falls_back_to_concealment_counts_corruption_and_needs_k(full_model, three_streams, cuda):
    """delay=1: two consecutive losses on row 2 -- the first push has no redundant copy in reach (LOST), the second is recovered
    from the packet after it; a corrupt packet is counted and treated as lost; a tick without any readable packet needs k=."""
    from facodec_amd.streaming import StreamingReceiver
    s = three_streams
    rx = StreamingReceiver(full_model, s["headers"], delay=1)
    with pytest.raises(ValueError):
        rx.prime([s["fq"][0][0], None, s["fq"][0][2]])
    rx = StreamingReceiver(full_model, s["headers"], delay=1)
    with pytest.raises(ValueError):
        rx.prime([s["fq"][0][0], s["fq"][0][1][:-1], s["fq"][0][2]])
    rx = StreamingReceiver(full_model, s["headers"], delay=1)
    with pytest.raises(RuntimeError):
        rx.tick(s["fq"][1])
    rx.prime(s["fq"][0])
    seen = {}
    bad = bytearray(s["fq"][8][0])
    bad[13] ^= 1
    for i in range(1, 11):
        p = list(s["fq"][i])
        if i in (4, 5):
            p[2] = None
        if i == 8:
            p[0] = bytes(bad)
        w = rx.tick(p)
        if i > 1:
            seen[i - 1] = list(rx.last_status)
            assert w.shape == s["waves"][i - 1].shape
    assert seen[4] == [PRIMARY, PRIMARY, LOST] and seen[5] == [PRIMARY, PRIMARY, REDUNDANT]
    assert seen[8] == [REDUNDANT, PRIMARY, PRIMARY]                          # the corrupt packet's push came from packet 9
    assert all(v == [PRIMARY] * 3 for i, v in seen.items() if i not in (4, 5, 8))
    k4, k5, k8 = (s["host"][i][0].shape[-1] for i in (4, 5, 8))
    assert rx.stats[2] == dict(received=9, recovered=k5, concealed=k4, corrupt=0, misordered=0)       # prime's packet counts
    assert rx.stats[0] == dict(received=10, recovered=k8, concealed=0, corrupt=1, misordered=0)
    # push 10 is held; packet 11 of every stream is lost: k comes from the held packets.  Then nothing is readable at all.
    w = rx.tick([None] * 3)
    assert rx.last_status == [PRIMARY] * 3 and torch.equal(w[1], s["waves"][10][1])      # row 1 never lost anything
    before = [dict(d) for d in rx.stats]
    with pytest.raises(ValueError, match="k="):
        rx.tick([None] * 3)
    assert rx.stats == before and rx.reader.expected == 12                   # the refused tick did not happen
    w = rx.tick([None] * 3, k=2)
    assert rx.last_status == [LOST] * 3 and w.shape == (3, 1, 600)
    assert [d["concealed"] for d in rx.stats] == [2, 2, k4 + 2]
    # delay=0: the same rule
    rx0 = StreamingReceiver(full_model, s["headers"])
    rx0.prime(s["fp"][0])
    with pytest.raises(ValueError, match="k="):
        rx0.tick([None] * 3)
    w = rx0.tick([None] * 3, k=1)
    assert w.shape == (3, 1, 300) and rx0.last_status == [LOST] * 3
    stale = rx0.tick(s["fp"][1], k=1)                                        # seq 1 after two ticks: misordered, concealed
    assert rx0.last_status == [LOST] * 3 and [d["misordered"] for d in rx0.stats] == [1, 1, 1] and stale.shape == (3, 1, 300)
    with pytest.raises(ValueError):
        StreamingReceiver(full_model, s["headers"], delay=2)
    with pytest.raises(ValueError):
        StreamingReceiver(full_model, s["headers"], fade=0)
