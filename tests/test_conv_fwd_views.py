"""The forward conv kernels on strided and offset views: ops.conv1d and ops.conv_transpose1d(has_history=True) consume any input
with x.stride(2) == 1 in place (its pointer, x.stride(0) -> x_bs, x.stride(1) -> x_cs), and ops.conv1d writes an `out=` that is a
time-contiguous view of a wider buffer (y_bs, y_cs).  tests/test_conv_fwd_epilogue.py pins every kernel to float64 on contiguous,
16-byte aligned tensors; this file launches the same BASES (its shapes, inputs, packs and kernels, by import) on views and asks for
the BITS of the contiguous launch: a view changes how a value reaches LDS or a register, never which operations form an output or
their order.  There is no new tolerance; the contiguous result is `_step_a`'s c_gpu, which that file holds to float64.

Input views of x (B, ci, T), built on the device inside a parent filled with the finite poison 1e30 (a value read under a zero
weight stays harmless, any other read swamps the output):
  off1         flat buffer of numel + 1 floats, [1:]                      contiguous strides, pointer % 16 == 4
  win          parent (B, ci, T + 11), [:, :, 5:5 + T]                    the streaming ring: pointer 20 bytes off, pitch T + 11
  win4         parent (B, ci, T + 12 rounded up to 4), [:, :, 8:8 + T]    pointer and strides keep the float4 / DMA route, x_cs != T_in
               (T + 12 itself wherever T % 4 == 0; narrow_two_level has T = 58, and the convtr history inputs have T + 1 columns)
  chan         parent (B, ci + 5, T), [:, 3:3 + ci]                       x_bs != ci x_cs, live channels above and below
  interleaved  parent (ci, B, T + 3), .permute(1, 0, 2)[:, :, :T]         x_bs < x_cs: the LSTM projection's layout (x_bs == x_cs at B = 1)
`win` and `chan` run at T and at T_odd, the others at T.  Output views mirror them (owin, owin4, ochan, ointerleaved) inside a
canary-filled parent, with the operand set `plain` and a second one with an epilogue (SECOND_OP) at T, and `plain` on owin / ochan
at T_odd.  ops.conv1d admits a strided `out=` only without res and y2.

Every case, through one function (`_check_view`) that takes the launcher as an argument:
  1. the descriptor launched carries the view's pointer and strides (a silent .contiguous() fails), pointer class as stated above;
  2. the kernel is the one of the contiguous launch (ROUTED: views the planner legitimately sends elsewhere -- none);
  3. the output has the bits of the contiguous launch (EXCEPTIONS: kernels that legitimately reorder -- none -- are held to
     `_sum_bound` against conv_ref, as Step A does);
  4. the input parent is unchanged and holds the poison outside the view; the output parent holds the canary outside the view and
     no canary inside.
The CPU-only tests run the same function on an fp32 emulation that addresses the parents' storage by raw index arithmetic, faithful
and with one planted fault at a time (FAULTS), and ask the planner for the kernel of every (base, kind) on descriptors alone.

The transposed conv's three has_history cases (tests/test_convtr_fwd.py) run with x as `win` and `win4` windows, and one case
restates streaming._LSTMState.run's `few` branch (H = 64, T = 2, B = 2, BP = 32) on both sides at once.
"""
# Measured on MI355X.  931 view cases over the 55 non-flattened bases (385 input views, 546 output views, of which 216 with the
# second operand set), 6 transposed-conv windows and the LSTM projection: every one bit-identical to the contiguous launch, on the
# contiguous launch's kernel, every parent intact.  ROUTED and EXCEPTIONS are empty: no view was re-routed by the planner, no kernel
# reorders its sum on a view, and none needed a fix.  Kernels reached, by the spy's names: the eight fp32 tiles (vec_ok of
# conv1d_mfma.h holds on win4 and, at T % 4 == 0, on chan: the LDS-DMA route inside the signal and float4 loads at its edges; off1,
# win and interleaved take the scalar route), split taps k = 3, 5, 7 on 64 rows and k = 7 on 96, split GEMM with 1 and 2 taps
# (strided included), bsplit2 <9,1> <9,2> <3,1>, pw, pws, pwt, narrow in both tap forms, thin, cin1, split reduction, single launch.
# The LSTM projection sits at 0.052 of Step A's bound (n = 64) on top of its bit equality.
# Wall time of this file's GPU tests: 12 s for 938 cases, Step A of each (base, length) included (cached for its kinds; the epilogue
# file's own cache is not shared across files); the slowest 0.8 s (the streaming kernels' first case per length: 16 M outputs and
# their float64 reference), every other case under 0.1 s.  Far below the minute at which the T_odd repetitions of `chan`
# would have been dropped: they are kept.
from collections import namedtuple
import functools
import types

import pytest
import torch
import torch.nn.functional as F

from facodec_amd import ops
import test_convtr_fwd as TR
from test_conv_fwd_epilogue import (BASE, BASES, CANARY, OPS, Case, _desc, _geometry, _is_split, _step_a, _switches, conv_ref)
from test_conv_launch_desc import _Spy
from test_train_kernels_gen import _record, _sum_bound

gpu = pytest.mark.gpu
POISON = 1e30
IN_KINDS = ("off1", "win", "win4", "chan", "interleaved")
OUT_KINDS = ("owin", "owin4", "ochan", "ointerleaved")
ODD_KINDS = ("win", "chan", "owin", "ochan")               # repeated at T_odd
VIEW_BASES = [b for b in BASES if b.flat is None]           # conv1d_flat and P8 inputs carry no strides
# the second operand set of the output views: one that runs the epilogue's Snake or activation and that the kernel admits without
# res and y2 (ADMITS of tests/test_conv_fwd_epilogue.py; pwt takes bias and alpha_y2 only, the mel shapes their own activation)
SECOND_OP = {"full": "aout", "noy2": "aout", "nores": "tanh", "y2": None, "log_mel": "log_mel"}

# (base name, kind) -> (substring of the kernel the planner names for the view, the predicate that routes it).  Empty: no predicate
# of conv_plan reads a pointer or a stride that these views change (test_planner_names_the_same_kernel_for_every_view).
ROUTED = {}
# kernel-name substring -> the source line that legitimately reorders the sum on a view; such cases are held to `_sum_bound`.
EXCEPTIONS = {}


# ------------------------------------------------------------------------------------------------ views
def _round4(n):
    return (n + 3) // 4 * 4


def _side_free(kind):
    """An output kind names the input kind it mirrors: `owin` is `win` on the other side."""
    return kind[1:] if kind in OUT_KINDS else kind


def _parent_shape(kind, shape):
    B, C, T = shape
    return {"off1": (B * C * T + 1,), "pad64": (B * C * T + 128,),
            "win": (B, C, T + 11), "win4": (B, C, _round4(T + 12)), "chan": (B, C + 5, T), "interleaved": (C, B, T + 3)}[_side_free(kind)]


def _carve(kind, parent, shape):
    """The view of `shape` inside a parent of _parent_shape(kind, shape).  `pad64`: the contiguous tensor 64 floats into a flat
    buffer (the plain side of a case: the output of an input-view case and the other way round)."""
    B, C, T = shape
    kind = _side_free(kind)
    if kind == "off1":
        return parent[1:].view(B, C, T)
    if kind == "pad64":
        return parent[64:64 + B * C * T].view(B, C, T)
    if kind == "win":
        return parent[:, :, 5:5 + T]
    if kind == "win4":
        return parent[:, :, 8:8 + T]
    if kind == "chan":
        return parent[:, 3:3 + C]
    assert kind == "interleaved", kind
    return parent.permute(1, 0, 2)[:, :, :T]


def _make(kind, shape, fill, dev):
    """(view, parent, outside): the parent filled with `fill`, the view of `shape` in it, and a mask of the parent that is True
    outside the view."""
    parent = torch.full(_parent_shape(kind, shape), fill, device=dev)
    outside = torch.ones(parent.shape, dtype=torch.bool, device=dev)
    _carve(kind, outside, shape).zero_()
    return _carve(kind, parent, shape), parent, outside


FAKE = 0x10000              # a 16-byte aligned address that is never dereferenced


def _meta_view(kind, shape):
    """(pointer, batch stride, channel stride) of the view from its construction alone, on a parent at FAKE."""
    v = _carve(kind, torch.empty(_parent_shape(kind, shape), device="meta"), shape)
    assert v.shape == tuple(shape) and v.stride(2) == 1
    return FAKE + 4 * v.storage_offset(), v.stride(0), v.stride(1)


def _lengths(b, kind):
    return (b.T, b.T_odd) if kind in ODD_KINDS else (b.T,)


# one parametrized list for both sides, ordered by (base, T) so that each contiguous launch and its float64 check run once
ViewCase = namedtuple("ViewCase", "id base T kind op")
VIEW_CASES = []
for _b in VIEW_BASES:
    for _T in (_b.T, _b.T_odd):
        for _k in IN_KINDS + OUT_KINDS:
            if _T in _lengths(_b, _k):
                VIEW_CASES.append(ViewCase(f"{_b.name}-T{_T}-{_k}", _b, _T, _k, "plain"))
                if _k in OUT_KINDS and _T == _b.T and SECOND_OP[_b.admits]:
                    VIEW_CASES.append(ViewCase(f"{_b.name}-T{_T}-{_k}-{SECOND_OP[_b.admits]}", _b, _T, _k, SECOND_OP[_b.admits]))
VIEW_IDS = [c.id for c in VIEW_CASES]
VIEW_BY_ID = {c.id: c for c in VIEW_CASES}
assert len(VIEW_BY_ID) == len(VIEW_CASES)


# ------------------------------------------------------------------------------------------------ the comparison
# what a launcher reports of the launch it made: the descriptor's input pointer and strides, output strides, the kernel's name
Seen = namedtuple("Seen", "x x_bs x_cs y_bs y_cs name")


def _check_view(launch, x, want, want_name, in_kind, out_kind, need_bits=True):
    """One launch of `launch(x_view, out_view) -> Seen` with x (contiguous, on its device) copied into a poisoned parent as
    `in_kind` and the output as `out_kind` inside a canary parent (None: the plain side, contiguous and 16-byte aligned), against
    `want`, the contiguous launch's output, and `want_name`, its kernel.  Checks 1 - 4 of the module docstring; with need_bits
    False the bit comparison is left to the caller (EXCEPTIONS).  Returns (Seen, out_view)."""
    dev = x.device
    if in_kind is None:
        xv, xparent, x_outside = x, None, None
    else:
        xv, xparent, x_outside = _make(in_kind, x.shape, POISON, dev)
        xv.copy_(x)
        before = xparent.clone()
        assert bool((xparent[x_outside] == POISON).all()) and torch.equal(xv, x)
    ov, oparent, o_outside = _make(out_kind or "pad64", want.shape, CANARY, dev)
    seen = launch(xv, ov)
    # 1. consumed in place
    assert seen.x == xv.data_ptr(), f"input pointer {seen.x:#x}, the view's is {xv.data_ptr():#x}: not consumed in place"
    assert (seen.x_bs, seen.x_cs) == (xv.stride(0), xv.stride(1)), (seen, xv.stride())
    assert (seen.y_bs, seen.y_cs) == (ov.stride(0), ov.stride(1)), (seen, ov.stride())
    if in_kind in ("off1", "win"):
        assert seen.x % 16 == 4, seen.x % 16
    if in_kind == "win4":
        assert seen.x % 16 == 0 and seen.x_cs % 4 == 0 and seen.x_bs % 4 == 0 and seen.x_cs > x.shape[2], seen
    if out_kind == "owin4":
        assert ov.data_ptr() % 16 == 0 and seen.y_cs % 4 == 0 and seen.y_bs % 4 == 0 and seen.y_cs > want.shape[2], seen
    # 2. the same kernel (None: a ROUTED case, whose caller names the other kernel)
    assert want_name is None or seen.name == want_name, (seen.name, want_name)
    # 4. the parents (before 3: a stray store explains a wrong bit, not the other way round)
    if xparent is not None:
        assert torch.equal(xparent, before), "the input parent was written"
        assert bool((xparent[x_outside] == POISON).all())
    assert bool((oparent[o_outside] == CANARY).all()), "the output parent was written outside the view"
    assert not bool((ov == CANARY).any()), "an output element was left unwritten"
    # 3. the bits
    if need_bits:
        assert ov.shape == want.shape and torch.equal(ov, want), \
            f"not the contiguous launch's bits: {int((ov != want).sum())} of {want.numel()} differ, worst {float((ov - want).abs().max()):.3e}"
    return seen, ov


# ------------------------------------------------------------------------------------------------ CPU: the table
def test_every_base_has_every_kind_and_the_kinds_are_what_they_claim():
    ids = set(VIEW_IDS)
    for b in VIEW_BASES:
        t_out, t_odd = _geometry(b, b.T)[0], _geometry(b, b.T_odd)[0]
        for k in IN_KINDS + OUT_KINDS:
            assert f"{b.name}-T{b.T}-{k}" in ids, (b.name, k)
            assert (f"{b.name}-T{b.T_odd}-{k}" in ids) == (k in ODD_KINDS), (b.name, k)
        second = SECOND_OP[b.admits]
        assert all((f"{b.name}-T{b.T}-{k}-{second}" in ids) for k in OUT_KINDS) or second is None
        for T in (b.T, b.T_odd):
            shape = (b.B, b.ci, T)
            p, bs, cs = _meta_view("off1", shape)
            assert p % 16 == 4 and (bs, cs) == (b.ci * T, T)
            p, bs, cs = _meta_view("win", shape)
            assert p % 16 == 4 and (bs, cs) == (b.ci * (T + 11), T + 11)
            p, bs, cs = _meta_view("win4", shape)
            assert p % 16 == 0 and cs % 4 == 0 and bs % 4 == 0 and cs > T and (cs == T + 12 or T % 4)
            p, bs, cs = _meta_view("chan", shape)
            assert bs == (b.ci + 5) * T != b.ci * cs and cs == T and p == FAKE + 4 * 3 * T
            p, bs, cs = _meta_view("interleaved", shape)
            assert (bs < cs or b.B == 1) and bs == T + 3 and cs == b.B * bs and p == FAKE
        p, bs, cs = _meta_view("owin4", (b.B, b.co, t_out))
        assert p % 16 == 0 and cs == t_out + 12 and bs % 4 == 0               # t_out % 4 == 0 at b.T: the float4 stores stay eligible
        assert t_odd % 4 in (1, 3)
    assert sum(b.B > 1 for b in VIEW_BASES) >= len(VIEW_BASES) - 1          # gemv alone has one clip; the LSTM case interleaves it
    assert {b.form for b in VIEW_BASES} == {b.form for b in BASES}          # no kernel family is reached by flattened cases alone
    # the arithmetic above is what torch does with a real allocation
    for kind in IN_KINDS:
        shape = (3, 5, 20)
        v = _carve(kind, torch.zeros(_parent_shape(kind, shape)), shape)
        base = v.untyped_storage().data_ptr()
        assert base % 16 == 0
        assert (v.data_ptr() - base + FAKE, v.stride(0), v.stride(1)) == _meta_view(kind, shape), kind


def test_planner_names_the_same_kernel_for_every_view():
    """fac_conv1d_variant on the descriptor of every (base, kind, T) with the view's pointer and strides written over the
    contiguous ones: the kernel of the contiguous descriptor, or the ROUTED entry.  The GPU test asserts the same on the launch."""
    bad = []
    for c in VIEW_CASES:
        b = c.base
        case = Case("view", b, c.T, OPS[c.op], "a")
        name0 = ops.conv_variant(_desc(case))[1]
        d = _desc(case)
        if c.kind in IN_KINDS:
            p, d.x_bs, d.x_cs = _meta_view(c.kind, (b.B, b.ci, c.T))
            d.x = p
        else:
            p, d.y_bs, d.y_cs = _meta_view(c.kind, (b.B, b.co, _geometry(b, c.T)[0]))
            d.y = p
        kid, name = ops.conv_variant(d)
        want = ROUTED.get((b.name, c.kind), (name0,))[0]
        if kid < 0 or want not in name or b.kern not in name0:
            bad.append((c.id, kid, name, name0))
    assert not bad, bad[:8]
    assert all(k[0] in BASE and k[1] in IN_KINDS + OUT_KINDS and len(v) == 2 for k, v in ROUTED.items())


# ------------------------------------------------------------------------------------------------ CPU: the self-check
def _flat(t):
    """The whole storage of t as a flat tensor (shares memory)."""
    return torch.as_strided(t, (t.untyped_storage().nbytes() // t.element_size(),), (1,), 0)


def _emulated(w, fault=None):
    """An fp32 conv `launch` for _check_view that reads and writes the parents' storage by raw index arithmetic from (offset,
    batch stride, channel stride), as a kernel does from (pointer, x_bs, x_cs) -- with one planted fault.  Indices wrap around
    the storage: a faulty kernel's stray access stays inside the test's own memory here."""
    def launch(xv, ov):
        B, C, T = xv.shape
        flat, off, bs, cs = _flat(xv), xv.storage_offset(), xv.stride(0), xv.stride(1)
        seen = (xv.data_ptr(), bs, cs)
        if fault == "contiguous":                                 # a silent copy: right values from the wrong place
            xc = xv.clone(memory_format=torch.contiguous_format)
            flat, off, bs, cs = xc.view(-1), 0, C * T, T
            seen = (xc.data_ptr(), bs, cs)
        if fault == "ptr_round":                                  # the pointer rounded down to 16 bytes
            off &= ~3
        if fault == "pitch_T":                                    # T_in as the channel pitch
            cs = T
        if fault == "bs_dense":                                   # C_in x_cs as the batch stride
            bs = C * cs
        ar = torch.arange
        idx = off + ar(B).view(-1, 1, 1) * bs + ar(C).view(1, -1, 1) * cs + ar(T).view(1, 1, -1)
        y = F.conv1d(flat[idx % flat.numel()], w)
        _, co, t_out = y.shape
        assert ov.shape == y.shape
        oflat, ooff, ybs, ycs = _flat(ov), ov.storage_offset(), ov.stride(0), ov.stride(1)
        if fault == "y_pitch_T":                                  # T_out as the output row pitch
            ycs = t_out
        oidx = ooff + ar(B).view(-1, 1, 1) * ybs + ar(co).view(1, -1, 1) * ycs + ar(t_out).view(1, 1, -1)
        oflat[oidx.reshape(-1) % oflat.numel()] = y.reshape(-1)
        if fault == "store_past":                                 # one store one element past the last row of every clip
            oflat[(ooff + ar(B) * ybs + (co - 1) * ycs + t_out) % oflat.numel()] = 1.0
        return Seen(*seen, ov.stride(0), ov.stride(1), "emulated")
    return launch


# fault -> the kinds built to catch it
FAULTS = {
    "ptr_round": ("off1", "win"),
    "pitch_T": ("win", "win4", "interleaved"),
    "bs_dense": ("chan", "interleaved"),
    "contiguous": IN_KINDS,
    "y_pitch_T": ("owin4", "owin", "ointerleaved"),
    "store_past": OUT_KINDS + (None,),
}


def _emulation_inputs():
    gen = torch.Generator().manual_seed(11)
    x, w = torch.randn(3, 5, 20, generator=gen), torch.randn(4, 5, 5, generator=gen)       # T % 4 == 0 and T_out = 16: win4 / owin4 as stated
    want = torch.empty(3, 4, 16)
    _emulated(w)(x, want)
    assert torch.equal(want, F.conv1d(x, w))
    return x, w, want


def test_faithful_emulation_passes_every_kind():
    x, w, want = _emulation_inputs()
    for kind in IN_KINDS:
        _check_view(_emulated(w), x, want, "emulated", kind, None)
    for kind in OUT_KINDS:
        _check_view(_emulated(w), x, want, "emulated", None, kind)
    _check_view(_emulated(w), x, want, "emulated", "interleaved", "ointerleaved")          # both sides at once, as the LSTM case


@pytest.mark.parametrize("fault", list(FAULTS))
def test_check_catches_planted_faults(fault):
    """Each planted fault fails _check_view on every kind built to catch it."""
    x, w, want = _emulation_inputs()
    for kind in FAULTS[fault]:
        sides = (kind, None) if kind in IN_KINDS else (None, kind)
        with pytest.raises(AssertionError):
            _check_view(_emulated(w, fault), x, want, "emulated", *sides)
    with pytest.raises(AssertionError):                           # and another kernel's name
        _check_view(_emulated(w), x, want, "another kernel", "win", None)
    # where the fault is invisible by construction the check passes: the kinds isolate what their table row says
    if fault == "pitch_T":
        for kind in ("off1", "chan"):
            _check_view(_emulated(w, fault), x, want, "emulated", kind, None)
    if fault == "bs_dense":
        for kind in ("off1", "win", "win4"):
            _check_view(_emulated(w, fault), x, want, "emulated", kind, None)
    if fault == "ptr_round":
        for kind in ("win4", "chan", "interleaved"):
            _check_view(_emulated(w, fault), x, want, "emulated", kind, None)
    if fault == "y_pitch_T":
        _check_view(_emulated(w, fault), x, want, "emulated", None, "ochan")


# ------------------------------------------------------------------------------------------------ GPU: ops.conv1d
def _conv(b, T, ctx, o, xv, out):
    """ops.conv1d as tests/test_conv_fwd_epilogue.py's _launch calls it, on the input and the output given."""
    wp, ws = ctx.packs
    inp, dev = ctx.inp, xv.device
    geo = dict(pad_left=0, t_out=_geometry(b, T)[0], k1=b.k1, dilation2=b.dil2) if b.k1 else {}
    return ops.conv1d(xv, wp, b.co, b.k, bias=inp.bias.to(dev) if inp.bias is not None else None, stride=b.s, dilation=b.d,
                      pad_mode=b.mode, causal=b.causal, alpha_in=inp.alpha_in.to(dev) if b.prologue else None,
                      alpha_out=inp.alpha_out.to(dev) if o.aout else None, act=o.act, out=out, w_split=ws, **geo)


def _spied(run):
    """launch(x_view, out_view) -> Seen around run(x_view, out_view), which must launch one conv into out_view."""
    def launch(xv, ov):
        with _Spy() as spy:
            got = run(xv, ov)
        assert len(spy.launched) == 1 and got.data_ptr() == ov.data_ptr()
        d = spy.launched[0]
        return Seen(d.x, d.x_bs, d.x_cs, d.y_bs, d.y_cs, ops.conv_variant(d)[1])
    return launch


@functools.lru_cache(maxsize=2)
def _contiguous(bname, T):
    """The contiguous side of a (base, length), once for all its kinds: Step A's inputs, packs, kernel name and c_gpu (held to
    float64 there) on the device; the contiguous results of the other operand sets are added as they are asked for."""
    inp, packs, c_gpu, name = _step_a(bname, T)
    dev = torch.device("cuda:0")
    ctx = types.SimpleNamespace(inp=inp, packs=packs, name=name, x=inp.x.to(dev), want={})
    b = BASE[bname]
    with _switches(b):
        assert torch.equal(_want(b, T, ctx, "plain"), c_gpu.to(dev)), "this file's launch is not Step A's"
    return ctx


def _want(b, T, ctx, op):
    if op not in ctx.want:
        out = torch.full((b.B, b.co, _geometry(b, T)[0]), CANARY, device=ctx.x.device)
        seen = _spied(lambda xv, ov: _conv(b, T, ctx, OPS[op], xv, ov))(ctx.x, out)
        assert seen.name == ctx.name and not bool((out == CANARY).any())
        ctx.want[op] = out
    return ctx.want[op]


@gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("cid", VIEW_IDS)
def test_conv_fwd_on_views_has_the_contiguous_bits(cid, cuda):
    c = VIEW_BY_ID[cid]
    b = c.base
    assert ops.BF16_SPLIT
    ctx = _contiguous(b.name, c.T)
    with _switches(b):
        want = _want(b, c.T, ctx, c.op)
        sides = (c.kind, None) if c.kind in IN_KINDS else (None, c.kind)
        routed = ROUTED.get((b.name, c.kind))                    # another kernel: its name, then Step A's bound
        excepted = bool(routed) or any(k in ctx.name for k in EXCEPTIONS)
        launch = _spied(lambda xv, ov: _conv(b, c.T, ctx, OPS[c.op], xv, ov))
        seen, ov = _check_view(launch, ctx.x, want, None if routed else ctx.name, *sides, need_bits=not excepted)
        assert not routed or routed[0] in seen.name, (seen.name, routed)
    bits = torch.equal(ov, want)
    if excepted:
        assert c.op == "plain" or bits, "only the sum is held to float64 here"
        c64, mag = conv_ref(b, c.T, ctx.inp.x, ctx.inp.w, ctx.inp.bias, ctx.inp.alpha_in)
        extra = (3.0 if _is_split(b) else 0.0) + (7.0 if b.prologue else 0.0)
        _sum_bound(f"conv_fwd_view_sum_{cid}", ov.cpu(), c64, mag, b.ci * b.k, extra=extra)
    _record(f"conv_fwd_view_{cid}", {"kernel": seen.name, "bits": bits, "exception": bool(excepted)})


# ------------------------------------------------------------------------------------------------ GPU: transposed conv with a history column
TR_HISTORY = [n for n in TR.IDS if TR.BY_NAME[n].history]


def test_transposed_history_cases_are_the_three_of_the_table():
    assert TR_HISTORY == ["poly_s2_T50_history", "poly_s5_T51_history", "poly_s5_T331_history_tile_ain"]


@gpu
@pytest.mark.parametrize("kind", ["win", "win4"])
@pytest.mark.parametrize("name", TR_HISTORY)
def test_convtr_history_window_has_the_contiguous_bits(name, kind, cuda):
    """conv_transpose1d(has_history=True) on a time window of a wider buffer (the streaming decoder's rings): the bits of the
    contiguous launch, which tests/test_convtr_fwd.py holds to float64, on the same kernel, the parent intact."""
    c = TR.BY_NAME[name]
    x, w, bias, alpha_in, _ = TR._inputs(c)
    packed = ops.pack_convtr_for(c.layout, w.to(cuda), None, c.s)
    bias = bias.to(cuda)
    alpha_in = alpha_in.to(cuda) if alpha_in is not None else None
    launch = _spied(lambda xv, ov: ops.conv_transpose1d(xv, packed, c.co, c.s, bias=bias, alpha_in=alpha_in, out=ov, causal=True,
                                                        has_history=True))
    x = x.to(cuda)
    want = torch.full((c.B, c.co, c.T * c.s), CANARY, device=cuda)
    plain = launch(x, want)
    assert c.kern in plain.name and not bool((want == CANARY).any())
    seen, _ = _check_view(launch, x, want, plain.name, kind, None)
    _record(f"convtr_fwd_view_{name}_{kind}", {"kernel": seen.name, "bits": True, "exception": False})


# ------------------------------------------------------------------------------------------------ GPU: the LSTM projection
@gpu
def test_lstm_projection_views_as_the_streaming_session_passes_them(cuda):
    """streaming._LSTMState.run, `few` branch: the input projection of T B <= 4 real columns as T `clips` of B columns, both sides
    views of the time-major work buffers (H, T, BP) / (4H, T, BP) -- batch stride BP below the channel stride T BP.  Against the
    same conv on contiguous copies: the same bits on the single-launch kernel, the padding columns B .. BP of `pre` untouched."""
    H, T, B, BP = 64, 2, 2, 32
    gen = torch.Generator().manual_seed(12)
    w = (torch.randn(4 * H, H, generator=gen) / H ** 0.5).to(cuda)
    bias = torch.randn(4 * H, generator=gen).to(cuda)
    wp = ops.pack_conv_weight(w)
    inp = torch.full((H, T, BP), POISON, device=cuda)
    inp[:, :, :B] = torch.randn(H, T, B, generator=gen).to(cuda)
    pre = torch.full((4 * H, T, BP), CANARY, device=cuda)
    before = inp.clone()
    xv, ov = inp.view(H, T, BP).permute(1, 0, 2)[:, :, :B], pre.permute(1, 0, 2)[:, :, :B]
    assert (xv.stride(0), xv.stride(1)) == (BP, T * BP) and (ov.stride(0), ov.stride(1)) == (BP, T * BP)
    launch = _spied(lambda x_, o_: ops.conv1d(x_, wp, 4 * H, 1, bias=bias, pad_left=0, t_out=B, pad_mode=ops.PAD_ZERO, out=o_))
    want = torch.full((T, 4 * H, B), CANARY, device=cuda)
    plain = launch(xv.contiguous(), want)
    assert "gemv" in plain.name and "single launch" in plain.name, plain.name
    seen = launch(xv, ov)
    assert seen.name == plain.name
    assert seen.x == xv.data_ptr() == inp.data_ptr() and (seen.x_bs, seen.x_cs, seen.y_bs, seen.y_cs) == (BP, T * BP, BP, T * BP)
    assert torch.equal(inp, before), "the input buffer was written"
    assert bool((pre[:, :, B:] == CANARY).all()), "the padding columns of the pre-activations were written"
    assert not bool((pre[:, :, :B] == CANARY).any())
    assert torch.equal(ov, want), "not the bits of the conv on contiguous copies"
    # fp64 on top: the projection itself (n = H terms), as Step A bounds every sum
    x64 = xv.double().cpu()
    c64 = torch.einsum("oh,thb->tob", w.double().cpu(), x64) + bias.double().cpu().view(1, -1, 1)
    mag = torch.einsum("oh,thb->tob", w.double().cpu().abs(), x64.abs()) + bias.double().cpu().abs().view(1, -1, 1)
    _sum_bound("conv_fwd_view_lstm_projection", ov.cpu(), c64, mag, H)
    _record("conv_fwd_view_lstm_projection_kernel", {"kernel": seen.name, "bits": True, "exception": False})
