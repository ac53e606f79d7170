"""StreamPool without a device: the slot book-keeping, the pre-roll formula, the drain length and the segment
form of the session's state tensors, applied with plain index arithmetic on flat arrays."""
import pytest
import torch

from facodec_amd import ops
from facodec_amd.streaming import DRAIN_HOPS, FRAME, HOP, LOOKAHEAD, PoolFull, SlotBook, pool_preroll


# ------------------------------------------------------------------------------ slot book-keeping
def test_lowest_free_slot_and_pool_full():
    book = SlotBook(3)
    got = [book.join() for _ in range(3)]
    assert got == [(0, 1), (1, 2), (2, 3)]                     # ids count up, slot 0 (the donor) is never handed out
    with pytest.raises(PoolFull):
        book.join()
    assert issubclass(PoolFull, RuntimeError)
    with pytest.raises(ValueError):
        SlotBook(0)


def test_drain_takes_exactly_three_ticks_then_the_slot_is_reused():
    assert DRAIN_HOPS == 3
    book = SlotBook(2)
    a, _ = book.join()
    b, _ = book.join()
    book.leave(a)
    with pytest.raises(PoolFull):
        book.join()                                           # a draining stream still holds its slot
    for t in range(3):
        out, scatter, last = book.tick([b])
        assert out == [b, a]                                  # live streams first, then the draining ones
        assert scatter == [-1, -1, 0]                         # donor and draining slot hear silence, slot 2 takes row 0
        assert book.slot_of == [2, 1]
        assert last == {b: False, a: t == 2}
        if t < 2:
            with pytest.raises(PoolFull):
                book.join()
    out, scatter, last = book.tick([b])
    assert out == [b] and last == {b: False}
    c, slot = book.join()
    assert (c, slot) == (2, 1)                                # the freed slot, a new id


def test_lowest_free_slot_after_leaves_in_any_order():
    book = SlotBook(4)
    ids = [book.join()[0] for _ in range(4)]
    book.leave(ids[2])
    book.leave(ids[0])
    for _ in range(3):
        book.tick([ids[1], ids[3]])
    assert book.join()[1] == 1 and book.join()[1] == 3


def test_leave_twice_unknown_draining_and_duplicate_ids_raise():
    book = SlotBook(2)
    a, _ = book.join()
    b, _ = book.join()
    book.leave(a)
    with pytest.raises(ValueError):
        book.leave(a)
    with pytest.raises(ValueError):
        book.leave(17)
    before = (dict(book.draining), dict(book.underruns))
    with pytest.raises(ValueError):
        book.tick([a])                                        # draining
    with pytest.raises(ValueError):
        book.tick([b, 17])                                    # unknown
    with pytest.raises(ValueError):
        book.tick([b, b])                                     # twice
    assert (dict(book.draining), dict(book.underruns)) == before          # a refused tick changes nothing


def test_underruns_are_counted_and_unfed_streams_stay_in_the_output():
    book = SlotBook(3)
    a, b, c = (book.join()[0] for _ in range(3))
    out, scatter, _ = book.tick([c, a])
    assert out == [c, a, b] and scatter == [-1, 1, -1, 0]
    assert book.underruns == {a: 0, b: 1, c: 0}
    book.tick([])
    assert book.underruns == {a: 1, b: 2, c: 1}
    book.leave(b)
    book.tick([a, c])
    assert book.underruns == {a: 1, b: 2, c: 1}               # a draining stream is not an underrun


# ------------------------------------------------------------------------------ pre-roll
def test_preroll_formula_cycle_and_range():
    got = []
    for h in range(10, 25):
        N = 4800 + HOP * h
        p = pool_preroll(N)
        assert p == N - 300 * ((N - 1024) // 300 + 1)
        assert 724 <= p <= 1023
        got.append(p)
    assert got == [900, 780, 960, 840, 1020] * 3
    for N in range(4800, 4800 + 2400):                        # any sample count: the emitted frames end inside the look-ahead
        assert LOOKAHEAD - FRAME <= pool_preroll(N) <= LOOKAHEAD - 1


# ------------------------------------------------------------------------------ drain length
def _covered(N, L, drain):
    """A stream of L samples joins after N session samples, is fed ceil(L / 480) hops (the last one zero padded) and `drain`
    more hops of silence: do the frames emitted by then reach behind its last sample?"""
    M = N + HOP * (-(-L // HOP) + drain)
    frames = (M - LOOKAHEAD) // FRAME + 1
    return FRAME * frames >= N + L


def test_three_drain_hops_cover_every_length_and_two_do_not():
    short = 0
    for phase in range(5):
        N = 4800 + HOP * (10 + phase)
        for L in range(1, 2401):
            assert _covered(N, L, DRAIN_HOPS), (phase, L)
            short += not _covered(N, L, DRAIN_HOPS - 1)
    assert short > 0                                          # the constant is tight


# ------------------------------------------------------------------------------ segment table
def _slot_elements(seg, b):
    """Flat element indices of slot b of one segment (offset, rows, row_stride, row_len, slot_lo, slot_hi), in run order."""
    off, rows, row_stride, row_len, slot_lo, slot_hi = seg
    first = off + (b >> 5) * slot_hi + (b & 31) * slot_lo
    return [first + r * row_stride + j for r in range(rows) for j in range(row_len)]


@pytest.mark.parametrize("B,C,W", [(5, 1, 13), (5, 4, 8), (40, 3, 7)])
def test_edge_segment_is_the_slots_block(B, C, W):
    buf = torch.arange(B * C * W, dtype=torch.float32).view(B, C, W)
    segs = ops.edge_segments(C, W)
    assert len(segs) == 1
    for b in (3, 35):
        if b >= B:
            continue
        idx = _slot_elements(segs[0], b)
        assert torch.equal(buf.reshape(-1)[idx], buf[b].reshape(-1))


def test_lstm_state_segments_are_the_slots_cell_column_and_fragment_lanes():
    H, BP = 64, 64
    state = torch.arange(3 * H * BP, dtype=torch.float32).view(3, H, BP)
    flat = state.reshape(-1)
    segs = ops.lstm_state_segments(H, BP)
    assert len(segs) == 3
    for b in (3, 35):
        assert torch.equal(flat[_slot_elements(segs[0], b)], state[0][:, b])
        for plane in (1, 2):
            frag = state[plane].reshape(BP // 32, H // 8, 2, 32, 4)[b // 32, :, :, b % 32, :]
            assert torch.equal(flat[_slot_elements(segs[plane], b)], frag.reshape(-1))
    # the slots of one table partition every plane: no element belongs to two slots, none is left out
    for plane in range(3):
        seen = sorted(i for b in range(BP) for i in _slot_elements(segs[plane], b))
        assert seen == list(range(plane * H * BP, (plane + 1) * H * BP))


def test_lstm_state_segments_refuse_other_layouts():
    with pytest.raises(ValueError):
        ops.lstm_state_segments(60, 64)
    with pytest.raises(ValueError):
        ops.lstm_state_segments(64, 40)


def test_slot_table_refuses_cpu_tensors_and_wrong_shapes():
    from facodec_amd import _lib
    table = ops.SlotTable(5)
    with pytest.raises(_lib.FacodecHipError):
        table.add_edge(torch.zeros(5, 1, 13))
    with pytest.raises(ValueError):
        table.add_edge(torch.zeros(4, 1, 13))
    with pytest.raises(ValueError):
        table.add_lstm_state(torch.zeros(2, 64, 32))
    with pytest.raises(ValueError):
        table.freeze()


def test_slot_copy_and_rows_pick_refuse_on_the_host():
    """Error code + message before any launch (no device needed: the pointers are never dereferenced)."""
    import ctypes
    from facodec_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x10000)
    dst = lambda *v: (ctypes.c_int32 * len(v))(*v)
    assert lib.fac_slot_copy(None, 1, fake, 1, 40, 3, dst(1), 1, None) == -1 and b"null table" in lib.fac_last_error()
    assert lib.fac_slot_copy(fake, 1, fake, 1, 40, 3, dst(1, 3), 2, None) == -1 and b"both source and destination" in lib.fac_last_error()
    assert lib.fac_slot_copy(fake, 1, fake, 1, 40, 3, dst(1, 35, 1), 3, None) == -1 and b"duplicate destination" in lib.fac_last_error()
    assert lib.fac_slot_copy(fake, 1, fake, 1, 40, 3, dst(40), 1, None) == -1 and b"outside [0, 40)" in lib.fac_last_error()
    assert lib.fac_slot_copy(fake, 1, fake, 1, 40, 40, dst(1), 1, None) == -1 and b"outside [0, 40)" in lib.fac_last_error()
    assert lib.fac_slot_copy(fake, 1, fake, 1, 40, 3, dst(*range(4, 13)), 9, None) == -1 and b"9 destinations" in lib.fac_last_error()
    assert lib.fac_rows_pick(None, 480, fake, fake, 5, 3, 480, None) == -1 and b"null pointer" in lib.fac_last_error()
    assert lib.fac_rows_pick(fake, 100, fake, fake, 5, 3, 480, None) == -1 and b"src_stride=100" in lib.fac_last_error()


def test_segment_struct_layout_matches_the_header(tmp_path):
    """The ctypes mirror of fac_slot_seg has the size and field offsets gcc gives the header's struct."""
    import ctypes
    import os
    import shutil
    import subprocess
    from facodec_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "facodec_hip.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(fac_slot_seg), offsetof(fac_slot_seg, slot_hi),'
                   ' offsetof(fac_slot_seg, rows), offsetof(fac_slot_seg, slot_lo), offsetof(fac_slot_seg, elems),'
                   ' FAC_SLOT_MAX_DST, FAC_SLOT_TILE);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(repo, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    s = _lib.SlotSeg
    assert out == [ctypes.sizeof(s), s.slot_hi.offset, s.rows.offset, s.slot_lo.offset, s.elems.offset, _lib.SLOT_MAX_DST, _lib.SLOT_TILE]
