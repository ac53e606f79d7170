"""StreamPool on the GPU: fac_slot_copy and fac_rows_pick against torch indexing, bit for bit, and pooled streams
against the rows of lockstep sessions of the same B that heard silence and then the stream -- every code and every sample equal,
pre-roll frames and drain ticks included."""
import pytest
import torch

from facodec_amd import _lib, ops, synth

pytestmark = pytest.mark.gpu

TICKS = 30
WARM = 10                # zero hops every session is warmed with behind its 4 800 zero samples of prime()


# ==================================================================================================================== kernels
def _slot_tensors(cuda, B, seed):
    g = torch.Generator().manual_seed(seed)
    bufs = [torch.randn(B, 1, 13, generator=g), torch.randn(B, 4, 8, generator=g), torch.randn(B, 3, 3000, generator=g)]
    state = torch.randn(3, 64, ops.pad32(B), generator=g)
    return [b.to(cuda) for b in bufs], state.to(cuda)


def _expect_slot_copy(bufs, state, src, dsts):
    bufs, state = [b.clone() for b in bufs], state.clone()
    H, BP = state.shape[1], state.shape[2]
    for d in dsts:
        for b in bufs:
            b[d] = b[src]
        state[0][:, d] = state[0][:, src]
        for plane in (1, 2):
            frag = state[plane].view(BP // 32, H // 8, 2, 32, 4)
            frag[d // 32, :, :, d % 32, :] = frag[src // 32, :, :, src % 32, :]
    return bufs, state


def _table(B, bufs, state):
    table = ops.SlotTable(B)
    for b in bufs:
        table.add_edge(b)
    table.add_lstm_state(state)
    return table.freeze()


def test_slot_copy_moves_one_slot_of_every_tensor_and_nothing_else(cuda):
    """Misaligned slots (13 floats), aligned ones, three tiles with a partial last one, an LSTM state with slots in both column
    blocks: slot 3 -> slots 1 and 35 in one launch; every tensor as a whole equals the torch-indexed expectation."""
    B = 40
    bufs, state = _slot_tensors(cuda, B, 1)
    want_bufs, want_state = _expect_slot_copy(bufs, state, 3, [1, 35])
    table = _table(B, bufs, state)
    assert table.n_tiles == 1 + 1 + 3 + 3 and table.elems == 13 + 32 + 9000 + 3 * 64
    table.copy(3, [1, 35])
    for got, want in zip(bufs, want_bufs):
        assert torch.equal(got, want), tuple(got.shape)
    assert torch.equal(state, want_state)


def test_slot_copy_takes_more_than_eight_destinations_in_several_launches(cuda):
    B = 40
    bufs, state = _slot_tensors(cuda, B, 2)
    dsts = [1, 2, 5, 8, 13, 21, 31, 32, 33, 39, 4]
    want_bufs, want_state = _expect_slot_copy(bufs, state, 0, dsts)
    _table(B, bufs, state).copy(0, dsts)
    for got, want in zip(bufs, want_bufs):
        assert torch.equal(got, want), tuple(got.shape)
    assert torch.equal(state, want_state)


def test_slot_copy_refusals_leave_the_tensors_alone(cuda):
    B = 40
    bufs, state = _slot_tensors(cuda, B, 3)
    keep = [b.clone() for b in bufs] + [state.clone()]
    table = _table(B, bufs, state)
    for src, dsts, msg in ((3, [3], "both source and destination"), (3, [1, 1], "duplicate destination"), (3, [40], "outside [0, 40)"),
                           (40, [1], "outside [0, 40)"), (3, list(range(4, 13)), "9 destinations"), (3, [], "0 destinations")):
        with pytest.raises(_lib.FacodecHipError, match=msg.replace("[", r"\[").replace(")", r"\)")):
            ops.slot_copy_raw(table, src, dsts)
    with pytest.raises(_lib.FacodecHipError):
        ops.SlotTable(B).add_edge(torch.zeros(B, 1, 13))                          # a CPU tensor
    torch.cuda.synchronize()
    for got, want in zip(bufs + [state], keep):
        assert torch.equal(got, want)


@pytest.mark.parametrize("L", [480, 481])
def test_rows_pick_scatters_fp32_rows_and_zeroes_the_rest(cuda, L):
    g = torch.Generator().manual_seed(L)
    src = torch.randn(3, L, generator=g).to(cuda)
    out = torch.full((5, 1, L), 7.0, device=cuda)
    got = ops.rows_pick(src, ops.rows_pick_map([-1, 2, 0, -1, 1], 1, cuda), out=out)
    want = torch.zeros(5, 1, L, device=cuda)
    want[1, 0], want[2, 0], want[4, 0] = src[2], src[0], src[1]
    assert got is out and torch.equal(out, want)


def test_rows_pick_gathers_int64_rows_of_a_wider_static_buffer(cuda):
    g = torch.Generator().manual_seed(4)
    wide = torch.randint(-2 ** 62, 2 ** 62, (5, 3, 16), generator=g).to(cuda)
    keep = wide.clone()
    got = ops.rows_pick(wide[:, :, :2], ops.rows_pick_map([4, 1], 3, cuda))
    assert got.shape == (2, 3, 2) and got.dtype == torch.int64
    assert torch.equal(got, wide[[4, 1]][:, :, :2]) and torch.equal(wide, keep)


def test_rows_pick_treats_a_row_past_the_source_as_none(cuda):
    src = torch.randn(5, 480, generator=torch.Generator().manual_seed(5)).to(cuda)
    got = ops.rows_pick(src, ops.rows_pick_map([4, 7, 5, 0], 1, cuda))
    want = torch.stack([src[4], torch.zeros_like(src[0]), torch.zeros_like(src[0]), src[0]])
    assert torch.equal(got, want)


def test_rows_pick_gathers_the_rows_of_a_b_1_t_wave(cuda):
    wave = torch.randn(4, 1, 600, generator=torch.Generator().manual_seed(6)).to(cuda)
    out = torch.zeros(3, 1, 600, device=cuda)
    ops.rows_pick(wave, ops.rows_pick_map([3, 1], 1, cuda), out=out[:2])
    assert torch.equal(out[:2], wave[[3, 1]]) and not out[2].any()
    with pytest.raises(_lib.FacodecHipError):
        ops.rows_pick(wave.cpu(), ops.rows_pick_map([0], 1, cuda))


# ==================================================================================================================== sessions
@pytest.fixture(scope="module")
def codec(cuda):
    from facodec_amd.commons import build_model, default_model_params
    model = build_model(default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(cuda)
    return model


@pytest.fixture(scope="module")
def material(cuda):
    """Four streams of TICKS hops and four timbres.  Stream 1 is silent in the hop of tick 9 (it joins at tick 4): the pool run
    that omits it there and the runs that pass those zeros must agree."""
    wave = synth.synth_clips(4, TICKS * 480, seed=5)[:, 0].contiguous()
    wave[1, (9 - 4) * 480:(10 - 4) * 480] = 0
    timbre = 0.5 * torch.randn(4, 1024, generator=torch.Generator().manual_seed(8))
    return wave.to(cuda), timbre.to(cuda)


def _style_row(model, timbre):
    with torch.no_grad():
        return model.quantizer.timbre_linear(timbre.reshape(1, -1).contiguous()).reshape(-1)


class _Lockstep:
    """A plain session of B = 3 rows under the zero timbre, warmed like a pool; rows = {row: (stream, join tick, leave tick)}: the
    row is silent before its join tick and from its leave tick on, and its style (or cond) row is written at the join tick."""

    def __init__(self, sess, rows, write_row, material, cuda):
        self.sess, self.rows, self.write_row = sess, rows, write_row
        self.wave, self.timbre = material
        self.hop = torch.zeros(3, 1, 480, device=cuda)
        with torch.no_grad():
            sess.prime(torch.zeros(3, 1, 4800, device=cuda))
            for _ in range(WARM):
                sess.push(self.hop)

    def tick(self, t):
        self.hop.zero_()
        for row, (s, t0, t1) in self.rows.items():
            if t == t0:
                self.write_row(self.sess, row, self.timbre[s])
            if t0 <= t < t1:
                self.hop[row, 0] = self.wave[s, (t - t0) * 480:(t - t0 + 1) * 480]
        with torch.no_grad():
            return self.sess.push(self.hop)


def _drive(pool, plan, refs, material, omit=()):
    """Runs TICKS ticks of `pool` under plan = {stream: (join tick, leave tick)} next to the lockstep sessions refs = [(_Lockstep,
    {stream: row})] and compares every output row of every tick.  omit: (stream, tick) pairs left out of `sids` although live.
    -> {stream: [(codes clones, wave clone) per tick]}, and the per-stream observations."""
    from facodec_amd.streaming import pool_preroll
    wave, timbre = material
    sid, kept, lasts, frames = {}, {s: [] for s in plan}, {s: 0 for s in plan}, {s: 0 for s in plan}
    bad = []
    for t in range(TICKS):
        for s, (t0, t1) in plan.items():
            if t == t0:
                sid[s] = pool.join(timbre[s])
                assert pool.preroll(sid[s]) == pool_preroll(4800 + 480 * (WARM + t)) == (900, 780, 960, 840, 1020)[t % 5]
            if t == t1:
                pool.leave(sid[s])
        fed = [s for s, (t0, t1) in plan.items() if t0 <= t < t1 and (s, t) not in omit]
        hops = torch.stack([wave[s, (t - plan[s][0]) * 480:(t - plan[s][0] + 1) * 480] for s in fed]) if fed else None
        out = pool.tick([sid[s] for s in fed], hops)
        ref_out = [(r.tick(t), rows) for r, rows in refs]
        here = {s for s, (t0, t1) in plan.items() if t0 <= t < t1 + 3}
        by_sid = {v: k for k, v in sid.items()}
        assert [by_sid[i] for i in out["sids"]][:len(fed)] == fed and {by_sid[i] for i in out["sids"]} == here, t
        k = out["wave"].shape[-1] // 300
        assert out["wave"].shape == (len(here), 1, 300 * k) and all(c.shape[0] == len(here) and c.shape[2] == k for c in out["codes"])
        for i, ident in enumerate(out["sids"]):
            s = by_sid[ident]
            assert out["frame0"][ident] == frames[s] and out["preroll"][ident] == pool_preroll(4800 + 480 * (WARM + plan[s][0]))
            frames[s] += k
            lasts[s] += bool(out["last"][ident])
            assert bool(out["last"][ident]) == (t == plan[s][1] + 2), (s, t)
            kept[s].append(([c[i].clone() for c in out["codes"]], out["wave"][i].clone()))
            for o, rows in ref_out:
                if s not in rows:
                    continue
                for j, c in enumerate(o["codes"]):
                    if not torch.equal(out["codes"][j][i], c[rows[s]]):
                        bad.append((t, s, f"codes[{j}]"))
                if not torch.equal(out["wave"][i], o["wave"][rows[s]]):
                    bad.append((t, s, "wave", float((out["wave"][i] - o["wave"][rows[s]]).abs().max())))
    assert not bad, bad[:12]
    return kept, lasts, sid


def _write_style(model):
    def write(sess, row, timbre):
        sess.qs.style[row].copy_(_style_row(model, timbre))
    return write


@pytest.fixture(scope="module", params=[True, False], ids=["graphs", "eager"])
def two_runs(request, codec, material, cuda):
    """The schedule of the issue on a pool of 2 slots (B = 3), next to two lockstep sessions, and the same pool run without
    streams 0 and 2 (plus a late joiner), next to a third: computed once per graph mode, shared by the tests below."""
    from facodec_amd.streaming import StreamingCodec, StreamPool
    use_graphs = request.param
    zero = torch.zeros(3, 1024, device=cuda)

    def lockstep(rows):
        return _Lockstep(StreamingCodec(codec, zero, n_c=2, use_graphs=use_graphs), rows, _write_style(codec), material, cuda)

    # stream 0 joins at tick 2 and leaves at 12 (slot 1, free again at 15); stream 1 joins at 4 (slot 2) and misses tick 9;
    # stream 2 joins at 17 into slot 1; streams 1 and 2 leave at 27 and drain until the last tick
    plan = {0: (2, 12), 1: (4, 27), 2: (17, 27)}
    pool = StreamPool(codec, slots=2, n_c=2, use_graphs=use_graphs)
    ref_a = lockstep({1: (0, 2, 12), 2: (1, 4, 27)})
    ref_b = lockstep({1: (2, 17, 27), 2: (1, 4, 27)})
    first = _drive(pool, plan, [(ref_a, {0: 1, 1: 2}), (ref_b, {2: 1, 1: 2})], material, omit={(1, 9)})
    underruns = dict(pool.underruns)
    del pool, ref_a, ref_b
    # stream 1 alone (now in slot 1, fed its zeros at tick 9), and stream 3 joining at tick 25 into slot 2
    plan2 = {1: (4, 27), 3: (25, TICKS)}
    pool2 = StreamPool(codec, slots=2, n_c=2, use_graphs=use_graphs)
    ref_c = lockstep({1: (1, 4, 27), 2: (3, 25, TICKS)})
    second = _drive(pool2, plan2, [(ref_c, {1: 1, 3: 2})], material)
    return first, underruns, second, dict(pool2.underruns)


def test_pool_equals_lockstep(two_runs):
    """Every tick, every stream: codes and wave equal the stream's row of a lockstep session (asserted while the runs were
    driven); `last` exactly once per stream that left, on its third drain tick; a slot is reused after its drain."""
    (kept, lasts, sid), _, _, _ = two_runs
    assert lasts == {0: 1, 1: 1, 2: 1}
    assert len(kept[0]) == 12 - 2 + 3 and len(kept[1]) == TICKS - 4 and len(kept[2]) == TICKS - 17
    assert sid == {0: 0, 1: 1, 2: 2}


def test_neighbours_and_the_slot_do_not_matter(two_runs):
    (kept, _, _), _, (kept2, _, _), _ = two_runs
    assert len(kept[1]) == len(kept2[1])
    for t, ((codes, wave), (codes2, wave2)) in enumerate(zip(kept[1], kept2[1])):
        assert all(torch.equal(a, b) for a, b in zip(codes, codes2)) and torch.equal(wave, wave2), t


def test_the_donor_stays_clean(two_runs):
    """A stream that joins 25 ticks (35 hops) after the session began still equals its lockstep row (asserted in the drive)."""
    _, _, (kept2, lasts2, _), _ = two_runs
    assert len(kept2[3]) == TICKS - 25 and lasts2 == {1: 1, 3: 0}


def test_an_omitted_stream_hears_silence_and_is_counted(two_runs):
    """Run 1 leaves stream 1 out of tick 9, run 2 and the lockstep sessions feed it that hop's zeros: equal (the two tests above)."""
    _, underruns, _, underruns2 = two_runs
    assert underruns == {0: 0, 1: 1, 2: 0} and underruns2 == {0: 0, 1: 0}


@pytest.mark.parametrize("use_graphs", [True, False], ids=["graphs", "eager"])
def test_conversion_pool_equals_lockstep_converter(codec, cuda, use_graphs):
    from facodec_amd.commons import build_model
    from facodec_amd.streaming import StreamingConverter, StreamPool
    from test_streaming_converter import _redecoder_params
    red = build_model(_redecoder_params(lstm=2), stage="redecoder")
    for k in ("encoder", "decoder"):
        synth.load_synthetic(red[k], seed=0, prefix="redecoder." + k + ".")
        red[k].eval().to(cuda)
    wave = synth.synth_clips(1, 15 * 480, seed=6)[0, 0].to(cuda)
    timbre = (0.5 * torch.randn(2, 1024, generator=torch.Generator().manual_seed(9))).to(cuda)

    def cond_row(t):
        with torch.no_grad():
            return red.encoder.encoder.cond_layer.run(t.reshape(1, -1, 1).contiguous()).reshape(-1)

    pool = StreamPool(codec, slots=2, redecoder=red, use_p_code=False, n_c=1, use_graphs=use_graphs)
    ref = StreamingConverter(codec, red, torch.zeros(3, 1024, device=cuda), use_p_code=False, n_c=1, use_graphs=use_graphs)
    hop = torch.zeros(3, 1, 480, device=cuda)
    with torch.no_grad():
        ref.prime(torch.zeros(3, 1, 4800, device=cuda))
        for _ in range(WARM):
            ref.push(hop)
    sid, bad = None, []
    for t in range(15):
        if t == 3:
            sid = pool.join(timbre[0])
            ref.red.cond[1].copy_(cond_row(timbre[0]))
        if t == 9:
            pool.set_timbre(sid, timbre[1])
            ref.red.cond[1].copy_(cond_row(timbre[1]))
        if t >= 3:
            hop[1, 0] = wave[(t - 3) * 480:(t - 2) * 480]
            out = pool.tick([sid], hop[1])
        else:
            out = pool.tick([])
        with torch.no_grad():
            o = ref.push(hop)
        if t < 3:
            assert out["sids"] == [] and out["wave"].shape[0] == 0
            continue
        assert out["sids"] == [sid] and len(out["codes"]) == 2
        for j, c in enumerate(o["codes"]):
            if not torch.equal(out["codes"][j][0], c[1]):
                bad.append((t, f"codes[{j}]"))
        if not torch.equal(out["wave"][0], o["wave"][1]):
            bad.append((t, "wave", float((out["wave"][0] - o["wave"][1]).abs().max())))
    assert not bad, bad[:12]
    assert float(out["wave"].abs().max()) > 0


def test_pool_errors(codec, cuda):
    from facodec_amd.commons import build_model
    from facodec_amd.streaming import PoolFull, StreamPool
    from test_streaming_converter import _redecoder_params
    with pytest.raises(NotImplementedError, match="not causal"):
        StreamPool(codec, slots=1, redecoder=build_model(_redecoder_params(causal=False), stage="redecoder"))
    pool = StreamPool(codec, slots=1, n_c=2, use_graphs=False)
    timbre = torch.zeros(1024, device=cuda)
    for bad in (timbre.cpu(), timbre[:1000], timbre.double(), None):
        with pytest.raises(ValueError):
            pool.join(bad)
    sid = pool.join(timbre)
    with pytest.raises(PoolFull):
        pool.join(timbre)
    hop = torch.zeros(1, 480, device=cuda)
    for sids, hops in (([sid + 1], hop), ([sid, sid], torch.zeros(2, 480, device=cuda)), ([sid], hop[:, :479]), ([sid], hop[0]),
                       ([sid], hop.double()), ([sid], hop.cpu()), ([sid], None), ([], hop)):
        with pytest.raises(ValueError):
            pool.tick(sids, hops)
    with pytest.raises(ValueError):
        pool.set_timbre(sid + 1, timbre)
    assert pool.ticks == 0 and pool.underruns == {sid: 0}
    pool.leave(sid)
    with pytest.raises(ValueError):
        pool.tick([sid], hop)                                 # draining
    with pytest.raises(ValueError):
        pool.leave(sid)
    with pytest.raises(ValueError):
        pool.set_timbre(sid, timbre)
    lasts = [pool.tick([])["last"][sid] for _ in range(3)]
    assert lasts == [False, False, True] and pool.tick([])["sids"] == []
    assert pool.join(timbre) == sid + 1
