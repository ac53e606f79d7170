"""Tensor-level wrappers over the C ABI: borrow device pointers from torch tensors, enqueue on
torch's current HIP stream, allocate outputs with torch's caching allocator.  No arithmetic
happens in Python / ATen here -- every op below is one or more kernels of libfacodec_hip.so.
"""
import ctypes as C
import math
import os
from collections import namedtuple

import torch

from . import _lib
from .wprep import prepared
# the layout / launch-form policy, its predicates and the layout names live in convplan.py; re-exported for call sites, tests and tools
from .convplan import *  # noqa: F401,F403
from ._lib import ConvDesc, VqDesc, VqDecodeDesc, ResampleDesc, PAD_REFLECT, PAD_ZERO, ACT_NONE, ACT_TANH, ACT_MISH, ACT_LOG_MEL, ACT_GATE, ACT_WN_RES_SKIP  # noqa: F401


def pad32(n):
    return (n + 31) & ~31


def cin_pad(c):
    """Packed weights carry zero rows up to a multiple of 48 input channels (fac_cin_pad)."""
    return ((c + 47) // 48) * 48


# torch.cuda.current_stream() builds a Stream object through five layers of Python (7 us per call, 11 000 calls = 40 ms of host time
# per train step: tools/tune/host_profile.py, round 6); the raw handle is one C call.  Same value: the current stream of the
# current device, side-stream contexts included.
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_GET_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def _raw_stream(device_index=None):
    """The current HIP stream of the (current) device as an integer handle."""
    if _RAW_STREAM is not None and _GET_DEVICE is not None:
        return _RAW_STREAM(_GET_DEVICE() if device_index is None else device_index)
    return torch.cuda.current_stream(device_index).cuda_stream


def _stream():
    return C.c_void_p(_raw_stream())


def h2d(t, device, dtype=None):
    """Small host tensor (masks, lengths, offsets) -> device WITHOUT blocking the host: through the pinned caching allocator and an
    asynchronous copy on the current stream.  `t.to(device)` from pageable memory makes the host wait until the device has drained
    everything queued before it on that stream -- four such copies per train step (the quantizer-dropout masks) cost the step the
    whole lead of the host over the device and ~11 ms of idle GPU (tools/gpu_idle.py, round 6).  Tensors already on the device
    only change dtype."""
    if t.is_cuda:
        return t if dtype is None or t.dtype == dtype else t.to(dtype)
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    if torch.device(device).type != "cuda":
        return t.to(device)
    staged = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    staged.copy_(t)
    return staged.to(device, non_blocking=True)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _on_gpu(t, what):
    """The refusal every entry shares: a missing kernel path is an error, not a detour over the CPU."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.FacodecHipError(f"{what} must live on the GPU (got {getattr(t, 'device', type(t))}); there is no CPU path")
    return t


def _row_pitch(t, B, k):
    """The row pitch of t (B, ...) for a descriptor, in elements: its stride, or k where a single row's stride says nothing
    (and for no tensor at all)."""
    return t.stride(0) if t is not None and B > 1 else k


def _arg(t, what, dtype, shape, at_least=False, optional=False):
    """A tensor argument of a descriptor builder: `dtype`, on the GPU, and either exactly `shape` and contiguous or, with
    at_least, shape = (B, n): (B, >= n) with dense columns at any row pitch.  None passes where it is optional.  ValueError names
    the argument by `what`."""
    if t is None and optional:
        return None
    if isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype:
        if not at_least:
            if t.shape == shape and t.is_contiguous():
                return t
        elif t.dim() == 2 and t.shape[0] == shape[0] and t.shape[1] >= shape[1] and (t.shape[1] <= 1 or t.stride(1) == 1):
            return t
    name = str(dtype).replace("torch.", "")
    want = f"{name} ({shape[0]}, >= {shape[1]}) on the GPU with dense rows" if at_least else f"contiguous {name} {tuple(shape)} on the GPU"
    raise ValueError(f"{what} must be {want}, got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")


def _dev(t, what="tensor"):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.FacodecHipError(f"{what} must live on the GPU (got {t.device}); there is no CPU path")
    if t.dtype != torch.float32:
        raise _lib.FacodecHipError(f"{what} must be float32 (got {t.dtype})")
    return t if t.is_contiguous() else t.contiguous()


# --------------------------------------------------------------------------------- weights (K6)
@prepared
def wn_scale(v, g, out=None):
    """scale[i] = g[i]/||v[i]|| (dac/model/encodec.py:42-51)."""
    v = _dev(v, "weight_v")
    g = _dev(g, "weight_g")
    n = v.shape[0]
    scale = out if out is not None else torch.empty(n, device=v.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_wn_scale(_ptr(v), _ptr(g), _ptr(scale), n, v.numel() // n, _stream()), "fac_wn_scale")
    return scale


@prepared
def pack_conv_weight(v, g=None, out=None, scale=None):
    """(C_out, C_in, K) [+ weight-norm gain g (C_out,1,1)] -> packed (cin_pad(C_in), K, pad32(C_out));
    the rows of the padding channels are written as zeros by the kernel (no separate fill)."""
    v = _dev(v, "weight")
    if v.dim() == 2:
        v = v.unsqueeze(-1)
    c_out, c_in, k = v.shape
    cp = pad32(c_out)
    if scale is None and g is not None:
        scale = wn_scale(v, g)
    if out is None:
        out = torch.empty(cin_pad(c_in), k, cp, device=v.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_pack_conv_w(_ptr(v), _ptr(scale), _ptr(out), c_out, c_in, k, cp, _stream()),
               "fac_pack_conv_w")
    return out


@prepared
def pack_convtr_weight(v, g, stride, out=None):
    """ConvTranspose1d (C_in, C_out, 2*stride) -> polyphase packed (stride, cin_pad(C_in), 2, pad32(C_out))."""
    v = _dev(v, "weight")
    c_in, c_out, k = v.shape
    if k != 2 * stride:
        raise _lib.FacodecHipError(f"polyphase ConvTranspose1d needs kernel_size == 2*stride (got {k}, {stride})")
    cp = pad32(c_out)
    scale = wn_scale(v, g) if g is not None else None
    if out is None:
        out = torch.empty(stride, cin_pad(c_in), 2, cp, device=v.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_pack_convtr_w(_ptr(v), _ptr(scale), _ptr(out), c_in, c_out, stride, cp, _stream()),
               "fac_pack_convtr_w")
    return out


# All-phases-per-workgroup launch of the causal ConvTranspose1d (fac_conv_desc.row_phases): contiguous stores through the
# LDS epilogue instead of `stride` interleaved strided streams (2.9x the algorithmic HBM traffic).  Needs the 256-column
# tile, so it takes over from CONVTR_ROWS_MIN_T input columns; CONVTR_ROWS = False keeps the polyphase launch everywhere.
CONVTR_ROWS = False
CONVTR_ROWS_MIN_T = 512


def convtr_rows_pad(c_out, stride):
    cpt = 128 // stride
    return -(-c_out // cpt) * 128


@prepared
def pack_convtr_weight_rows(v, g, stride, out=None):
    """ConvTranspose1d (C_in, C_out, 2*stride) -> (cin_pad(C_in), 2, rows) with rows = (channel, phase) pairs in 128-row
    tiles (fac_pack_convtr_w_rows); conv_transpose1d recognises the layout by its 3 dimensions."""
    v = _dev(v, "weight")
    c_in, c_out, k = v.shape
    if k != 2 * stride:
        raise _lib.FacodecHipError(f"ConvTranspose1d needs kernel_size == 2*stride (got {k}, {stride})")
    scale = wn_scale(v, g) if g is not None else None
    if out is None:
        out = torch.empty(cin_pad(c_in), 2, convtr_rows_pad(c_out, stride), device=v.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_pack_convtr_w_rows(_ptr(v), _ptr(scale), _ptr(out), c_in, c_out, stride, _stream()),
               "fac_pack_convtr_w_rows")
    return out


# --------------------------------------------------------------------------------- conv (K1-K4)
class ConvLaunchProfile:
    """Opt-in per-launch timing of the conv kernel with HIP events recorded on the launch stream
    (bench.py's `roofline` leg).  Collects (variant name, algorithmic FLOPs, start, end)."""

    def __init__(self):
        self.records = []

    def summary(self):
        """{variant: dict(launches, flops, ms)}; call after a device synchronise."""
        out = {}
        for name, flops, e0, e1 in self.records:
            r = out.setdefault(name, dict(launches=0, flops=0.0, ms=0.0))
            r["launches"] += 1
            r["flops"] += flops
            r["ms"] += e0.elapsed_time(e1)
        return out


_PROFILE = None


class FlopCounter:
    """Algorithmic FLOPs of the GEMM-shaped work, counted where the C ABI is called (2 FLOP per multiply-add of the
    mathematical definition -- padding, tile remainders, the polyphase zero taps and the six-term bf16 split are NOT
    counted): conv forward / data gradients 2 B C_out T_out C_in K (a stride-s data gradient as the transposed conv it
    is: 2 B C_in T_in C_out K / s per ... i.e. one MAC per (output sample, tap that exists)), weight gradients
    2 B C_out C_in K T_out, LSTM recurrences 2 * 4H * H per (clip, step).  Elementwise work, FFT-free losses' small GEMMs
    booked as "dft" and left out of `total`, attention score products excluded (< 0.1 %).  Install with set_flop_counter();
    by key: conv, wgrad, lstm, dft."""

    def __init__(self):
        self.flops = dict(conv=0.0, wgrad=0.0, lstm=0.0, dft=0.0)
        self.launches = dict(conv=0, wgrad=0, lstm=0, dft=0)

    def add(self, key, f):
        self.flops[key] += f * _FLOP_SCALE
        self.launches[key] += 1

    @property
    def total(self):
        """Model MACs x 2: everything but the DFT-as-GEMM front-ends."""
        return sum(v for k, v in self.flops.items() if k != "dft")


_FLOPS = None
_FLOP_SCALE = 1.0


def set_flop_counter(c):
    global _FLOPS
    _FLOPS = c


_FLOP_KEY = "conv"


class flop_key:
    """Conv launches inside are booked under `key` instead of "conv": the windowed-DFT and mel-filterbank GEMMs of the STFT
    front-ends ("dft") are this build's way of doing an FFT, not MACs of the model."""

    def __init__(self, key):
        self.key = key

    def __enter__(self):
        global _FLOP_KEY
        self.prev, _FLOP_KEY = _FLOP_KEY, self.key

    def __exit__(self, *a):
        global _FLOP_KEY
        _FLOP_KEY = self.prev


class flop_scale:
    """Launches inside count `s` times their nominal FLOPs: the LSTM buffers carry the batch padded to 32 columns per time
    step, and the padding is not algorithmic work (s = B / BP)."""

    def __init__(self, s):
        self.s = s

    def __enter__(self):
        global _FLOP_SCALE
        self.prev, _FLOP_SCALE = _FLOP_SCALE, self.s

    def __exit__(self, *a):
        global _FLOP_SCALE
        _FLOP_SCALE = self.prev

# k = 7 convs on the bf16 matrix pipe with fp32-grade operand splitting (conv1d_bsplit.hip).  Results have
# fp32-MFMA-grade error; BF16_SPLIT = False keeps every conv on the fp32 MFMA kernel.
BF16_SPLIT = True
# Output channel counts whose k = 7 inference convs run the 96 x 256 form of the split kernel (conv1d_bsplit96.hip), read by
# convplan.tile_rows at call time.  Wired per channel count on a same-box A/B; () puts every layer on the 64 x 256 form.
BS_ROWS96 = (96,)


def set_conv_profile(p):
    global _PROFILE
    _PROFILE = p


_CONV_WS = {}
CONV_WS_BYTES = 32 << 20


_STREAM_SLOTS = {}


def register_stream_slot(stream):
    """Gives `stream` (a torch.cuda.Stream that will carry launches concurrently with other streams: the streaming session's
    second chain, the discriminators' side streams) its own conv scratch buffer; returns the slot.  Unregistered streams --
    the caller's stream, a graph-capture stream -- share slot 0, so nothing is allocated inside a capture."""
    key = stream.cuda_stream
    if key not in _STREAM_SLOTS:
        _STREAM_SLOTS[key] = len(_STREAM_SLOTS) + 1
    return _STREAM_SLOTS[key]


_SIDE_STREAMS = {}


def side_streams(device, n):
    """n cached side streams of `device`, each with its own conv scratch (register_stream_slot)."""
    key = (device, n)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = [torch.cuda.Stream(device=device) for _ in range(n)]
        for st in _SIDE_STREAMS[key]:
            register_stream_slot(st)
    return _SIDE_STREAMS[key]


def join_side_streams(device):
    """The current stream waits for everything queued so far on the concurrent-chain side streams of `device`.  Used in front of a
    gradient collective launched from inside backward: autograd orders a node behind the nodes that feed it, not behind the
    parameter-gradient kernels other chains queued on their own streams, and the collective reads the whole bucket."""
    if device.type != "cuda":
        return
    cur = torch.cuda.current_stream(device)
    for (dev, _), streams in _SIDE_STREAMS.items():
        if dev.type == "cuda" and (dev.index is None or device.index is None or dev.index == device.index):
            for st in streams:
                if st != cur:
                    cur.wait_stream(st)


def run_chains(chains, device, n_streams, inputs=()):
    """Independent chains of launches (callables) side by side on up to n_streams side streams that fork from and join the
    caller's stream; returns their results in order.  Kernels with fewer workgroups than CUs (or a partly filled last round)
    then overlap with another chain's kernels; autograd replays every node's backward on the stream of its forward, so the
    backward passes of the chains overlap the same way.

    inputs: the tensors the chains READ that were allocated on the caller's stream (nested lists / dicts are walked).  They are
    recorded on every side stream in use (Tensor.record_stream), because of what happens in BACKWARD: a chain's node saves such a
    tensor, its backward runs on the side stream, and the moment that backward function returns -- its kernels merely queued --
    the engine drops the saved tensor; the caching allocator then hands the block to the next allocation on the CALLER's stream,
    which is not ordered behind the side stream at that point.  Found in round 6 as a flaky 1 - 2 % error in ONE gradient
    (timbre_encoder.spectral.0.weight: the last backward node of the timbre chain reads the log-mel features, allocated on the main
    stream and freed right after; tools/tune/race_probe.py, profiles/r06_race_probe.log).  The forward has no such window: the join
    below orders the caller's stream behind everything the chains queued."""
    n = min(n_streams, len(chains))
    if n <= 1 or device.type != "cuda":
        return [c() for c in chains]
    main = torch.cuda.current_stream(device)
    streams = side_streams(device, n)
    for st in streams:
        st.wait_stream(main)
        _record_stream(inputs, st)
    outs = []
    for j, c in enumerate(chains):
        with torch.cuda.stream(streams[j % n]):
            outs.append(c())
    for st in streams:
        main.wait_stream(st)
    # The results live in the side streams' allocator pools but are consumed (and saved for backward) by nodes of the caller's
    # stream: tell the caching allocator, or a block freed on the host while the main-stream reader is still queued could be
    # handed to another chain's side-stream kernel (the forward is covered by the fork / join above, backward frees
    # are not).
    _record_stream(outs, main)
    return outs


def _record_stream(obj, stream):
    if torch.is_tensor(obj):
        if obj.is_cuda:
            obj.record_stream(stream)
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            _record_stream(o, stream)
    elif isinstance(obj, dict):
        for o in obj.values():
            _record_stream(o, stream)


_CUDA_DEVICES = {}


def _cuda_device(index):
    d = _CUDA_DEVICES.get(index)
    if d is None:
        d = _CUDA_DEVICES[index] = torch.device("cuda", index)
    return d


def _conv_workspace(device):
    """Zero-filled scratch handed to every conv launch (fac_conv_desc.ws), used by the split-reduction kernel for launches
    with few output columns: the partial sums live there between the two kernels of a launch, so it belongs to ONE stream
    at a time -- one buffer per (device, registered stream)."""
    slot = _STREAM_SLOTS.get(_raw_stream(device.index), 0) if _STREAM_SLOTS else 0
    key = (device, slot)
    ws = _CONV_WS.get(key)
    if ws is None:
        ws = _CONV_WS[key] = torch.zeros(CONV_WS_BYTES // 4, device=device, dtype=torch.float32)
    return ws


def conv_variant(d):
    """(id, name) of the kernel fac_conv1d_fwd launches for descriptor `d` (fac_conv1d_variant: the same planner, no launch);
    id < 0 with an empty name where fac_conv1d_fwd would reject `d`."""
    buf = C.create_string_buffer(96)
    return _lib.load().fac_conv1d_variant(C.byref(d), buf, 96), buf.value.decode()


def _launch_conv(d, what):
    lib = _lib.load()
    ws = _conv_workspace(_cuda_device(_GET_DEVICE() if _GET_DEVICE is not None else torch.cuda.current_device()))
    d.ws, d.ws_bytes = ws.data_ptr(), CONV_WS_BYTES
    if _FLOPS is not None or _PROFILE is not None:
        flops = 2.0 * d.B * d.n_phase * max(1, d.row_phases) * d.C_out * d.T_out * d.C_in * d.K
        if d.w_k1:
            flops += 2.0 * d.B * d.C_out * d.T_out * d.C_out   # fused 1x1 conv
    if _FLOPS is not None:
        _FLOPS.add(_FLOP_KEY, flops)
    if _PROFILE is None:
        _lib.check(lib.fac_conv1d_fwd(C.byref(d), _stream()), what)
        return
    name = conv_variant(d)[1][:63]      # the profile's keys have always been the first 63 bytes of the name
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.check(lib.fac_conv1d_fwd(C.byref(d), _stream()), what)
    e1.record()
    _PROFILE.records.append((name, flops, e0, e1))


GEMM_SPLIT_MIN_CIN = 256     # 1- / 2-tap convs as split-bf16 GEMMs (conv1d_gemm_split.hip): fewest input channels (convplan.gemm_split_ok)


@prepared
def pack_gemm_weight_split(v, g=None, out=None, in_stride=1, scale=None):
    """(C_out, C_in, K) [weight-normed with g over dim 0] -> fac_pack_gemm_w_split layout (uint8 buffer); K <= 2, or a strided
    conv's taps (in_stride < K <= 2 * in_stride)."""
    v = _dev(v, "weight")
    if v.dim() == 2:
        v = v.unsqueeze(-1)
    c_out, c_in, k = v.shape
    lib = _lib.load()
    if scale is None and g is not None:
        scale = wn_scale(v, g)
    nbytes = lib.fac_gemm_w_split_bytes(c_out, c_in, k, in_stride)
    if out is None:
        out = torch.empty(nbytes, device=v.device, dtype=torch.uint8)
    _lib.check(lib.fac_pack_gemm_w_split(_ptr(v), c_in * k, k, 1, _ptr(scale), out.data_ptr(), c_out, c_in, k, in_stride, _stream()),
               "fac_pack_gemm_w_split")
    return out


def pack_gemm_weight_split_t(w, out=None):
    """Materialised conv weight w (C_out, C_in, 1) -> split GEMM weights of the TRANSPOSED 1x1 (rows = C_in, contraction over
    C_out): the data gradient of a 1x1 conv, read through strides (no transposed copy)."""
    w = _dev(w, "weight")
    if w.dim() == 2:
        w = w.unsqueeze(-1)
    c_out, c_in, k = w.shape
    assert k == 1
    lib = _lib.load()
    nbytes = lib.fac_gemm_w_split_bytes(c_in, c_out, 1, 1)
    if out is None:
        out = torch.empty(nbytes, device=w.device, dtype=torch.uint8)
    _lib.check(lib.fac_pack_gemm_w_split(_ptr(w), 1, c_in, 1, None, out.data_ptr(), c_in, c_out, 1, 1, _stream()),
               "fac_pack_gemm_w_split(transposed)")
    return out


@prepared
def pack_conv_weight_split2(v, g=None, k1=0, out=None, scale=None):
    """(C_out <= 32, C_in, K) [weight-normed with g] -> fac_pack_conv_w_split2 layout (uint8 buffer); k1: taps per level."""
    v = _dev(v, "weight")
    c_out, c_in, k = v.shape
    lib = _lib.load()
    if scale is None and g is not None:
        scale = wn_scale(v, g)
    nbytes = lib.fac_conv_w_split2_bytes(c_out, c_in, k, k1)
    if out is None:
        out = torch.empty(nbytes, device=v.device, dtype=torch.uint8)
    _lib.check(lib.fac_pack_conv_w_split2(_ptr(v), _ptr(scale), out.data_ptr(), c_out, c_in, k, k1, _stream()),
               "fac_pack_conv_w_split2")
    return out


@prepared
def pack_convtr_weight_rows_split(v, g, stride, out=None):
    """ConvTranspose1d (C_in, C_out, 2*stride) -> split GEMM weights of the all-phases launch: the (channel, phase) rows of
    pack_convtr_weight_rows, each row's (C_in, 2) taps as bf16 planes.  Returns (split buffer, rows)."""
    rows = pack_convtr_weight_rows(v, g, stride)                  # (cin_pad, 2, R) fp32, weight-norm applied
    cip, _, R = rows.shape
    c_in = v.shape[0]
    lib = _lib.load()
    nbytes = lib.fac_gemm_w_split_bytes(R, c_in, 2, 1)
    if out is None:
        out = torch.empty(nbytes, device=v.device, dtype=torch.uint8)
    _lib.check(lib.fac_pack_gemm_w_split(_ptr(rows), 1, 2 * R, R, None, out.data_ptr(), R, c_in, 2, 1, _stream()),
               "fac_pack_gemm_w_split(convtr rows)")
    return out, R


@prepared
def pack_conv_weight_split(v, g=None, out=None, scale=None, rows=None):
    """(C_out, C_in, K) [weight-normed with g] -> split-bf16 layout of fac_pack_conv_w_split_rows (K = 3 / 5 / 7; uint8 buffer) or of
    fac_pack_gemm_w_split (K = 1 / 2).  rows: co-tile size, 64 or (K = 7) 96; None: what convplan.tile_rows names for an inference
    launch.  The buffer carries the figure as `.split_rows`, which conv1d hands to the launch with it."""
    v = _dev(v, "weight")
    c_out, c_in, k = v.shape
    if k <= 2:
        return pack_gemm_weight_split(v, g, out=out, scale=scale)
    lib = _lib.load()
    if scale is None and g is not None:
        scale = wn_scale(v, g)
    if rows is None:
        rows = tile_rows(c_out, c_in, k)
    nbytes = lib.fac_conv_w_split_rows_bytes(c_out, c_in, k, rows)
    if nbytes < 0:
        raise _lib.FacodecHipError("pack_conv_weight_split: no %d-row tile for k = %d" % (rows, k))
    if out is None or out.numel() != nbytes:         # (a buffer packed for the other tile: the switch was flipped in between)
        out = torch.empty(nbytes, device=v.device, dtype=torch.uint8)
    _lib.check(lib.fac_pack_conv_w_split_rows(_ptr(v), _ptr(scale), out.data_ptr(), c_out, c_in, k, rows, _stream()),
               "fac_pack_conv_w_split_rows")
    out.split_rows = rows
    return out


def conv_out_len(t_in, k, stride, dilation):
    """Output length and (pad_left, extra_right) of a causal SConv1d (dac/model/encodec.py:71-78,212-222)."""
    k_eff = (k - 1) * dilation + 1
    padding_total = k_eff - stride
    n_frames = (t_in - k_eff + padding_total) / stride + 1
    ideal = (math.ceil(n_frames) - 1) * stride + (k_eff - padding_total)
    extra = ideal - t_in
    t_out = (t_in + padding_total + extra - k_eff) // stride + 1
    return t_out, padding_total, extra


class P8:
    """An activation tensor (B, C, T) as three bf16 planes hi / mid / lo (hi + mid + lo == value exactly), each laid out
    [b][c / 8][t][8] -- the operand format of the split-bf16 kernels' LDS stages (fac_conv_desc.x_p8): `planes` is a (3, B, C / 8, T, 8)
    bfloat16 tensor; every plane ends with one zero unit (what consumers read for padding columns), so `planes` is stored as
    (3, B * C / 8 * T + 1, 8) bfloat16."""

    def __init__(self, planes, shape):
        self.planes, self.shape = planes, tuple(shape)

    @staticmethod
    def empty(B, C, T, device):
        return P8(torch.empty(3, B * (C // 8) * T + 1, 8, device=device, dtype=torch.bfloat16), (B, C, T))

    @property
    def plane_bytes(self):
        return self.planes.stride(0) * 2

    def to_float(self):
        """The fp32 tensor the planes add up to (tests)."""
        B, C, T = self.shape
        v = self.planes[:, :-1].float().sum(0).reshape(B, C // 8, T, 8)     # exact: three addends of disjoint significance
        return v.permute(0, 1, 3, 2).reshape(B, C, T).contiguous()


def to_p8(x, alpha=None):
    """fp32 (B, C, T) [-> snake(x, alpha)] -> P8 (fac_to_p8)."""
    x = _dev(x, "x")
    B, C, T = x.shape
    out = P8.empty(B, C, T, x.device)
    _lib.check(_lib.load().fac_to_p8(_ptr(x), _ptr(alpha), _ptr(out.planes), B, C, T, _stream()), "fac_to_p8")
    return out


# Inference launches of the split GEMM kernel whose every input byte feeds at least this many FLOPs take their input as P8
# planes made by ONE extra pass over it (fac_to_p8: 4 bytes read, 6 written per element at ~6 TB/s): the kernel then stages both
# operands by LDS-DMA instead of splitting fp32 values in its staging waves (+11 .. 20 % on such a launch), which
# pays for the pass when the input is small next to the GEMM -- the LSTM input projections, the transposed convs with many output
# rows per input sample, the last two strided convs of the encoder (threshold sweep 150 / 300 / 450 / 700 on one box: 56.3 / 56.0 /
# 55.5 / 56.0 ms per forward).  0 disables.
P8_PREPASS_MIN_FLOP_PER_BYTE = 450.0


def p8_prepass(x, flop_per_in_byte):
    """x (B, C, T) fp32 -> P8 when the policy above says the pass pays for itself (inference only: no autograd node), else x.
    flop_per_in_byte: a plan's `p8` figure (None: the plan's launch takes fp32 input)."""
    if (flop_per_in_byte is None or P8_PREPASS_MIN_FLOP_PER_BYTE <= 0 or flop_per_in_byte < P8_PREPASS_MIN_FLOP_PER_BYTE or not BF16_SPLIT or isinstance(x, P8)
            or torch.is_grad_enabled() or not x.is_cuda or x.shape[1] % 8 != 0 or x.shape[0] * (x.shape[1] // 8) * x.shape[2] * 16 >= (1 << 32)):
        return x
    return to_p8(x)


def conv_y_channels(c_out, act):
    """Channels of a conv's output tensor: the gated epilogues write c_out / 2."""
    return c_out // 2 if act in (ACT_GATE, ACT_WN_RES_SKIP) else c_out


def conv_desc(B, c_in, t_in, c_out, k, stride=1, dilation=1, pad_left=None, pad_mode=PAD_REFLECT, t_out=None, act=ACT_NONE, causal=True,
              k1=0, dilation2=0, c_out_pad=None, split_rows=0):
    """The launch descriptor of conv1d from shapes and flags alone (no tensor, no GPU): every non-pointer field of fac_conv_desc --
    the fields this function does not name stay the zeros of a fresh ConvDesc.  With pad_left=None the SConv1d padding rule gives
    pad_left and T_out (causal: everything on the left; non-causal: asymmetric split).  The strides are those of contiguous
    (B, c_in, t_in) / (B, conv_y_channels, T_out) tensors; conv1d overrides them for views and fills in the pointers.
    c_out_pad: padded row count of the fp32 pack (None: pad32); split_rows: co-tile size a split-taps buffer was packed for."""
    if pad_left is None:
        t_o, padding_total, _ = conv_out_len(t_in, k, stride, dilation)
        pad_left = padding_total if causal else padding_total - padding_total // 2
        if t_out is None:
            t_out = t_o
    if t_out is None:
        raise ValueError("t_out required with explicit pad_left")
    d = ConvDesc()
    d.x_bs, d.x_cs = c_in * t_in, t_in
    d.y_bs, d.y_cs = conv_y_channels(c_out, act) * t_out, t_out
    d.B, d.C_in, d.T_in, d.C_out, d.C_out_pad, d.T_out = B, c_in, t_in, c_out, (pad32(c_out) if c_out_pad is None else c_out_pad), t_out
    d.K, d.stride, d.dilation, d.pad_left, d.pad_mode = k, stride, dilation, pad_left, pad_mode
    d.n_phase, d.y_tstride, d.act, d.w_batched, d.w_bs = 1, 1, act, 0, 0
    d.K1, d.dilation2, d.split_rows = k1, dilation2, split_rows
    d.pw_split = 1 if (BF16_SPLIT and PW_SPLIT and (k == 1 or (PW_TAPS and k == 4 and stride == 2))) else 0
    d.keep_tile160 = 0 if K1_COLUMN_TILES else 1
    d.gsplit_p8_cols = GSPLIT_P8_COLS
    return d


def conv1d(x, w_packed, c_out, k, bias=None, stride=1, dilation=1, pad_left=None, pad_mode=PAD_REFLECT,
           t_out=None, alpha_in=None, alpha_out=None, res=None, act=ACT_NONE, out=None, causal=True,
           alpha_y2=None, want_y=True, w_k1=None, bias_k1=None, w_split=None, k1=0, dilation2=0, skip_acc=None, gate_cond=None):
    """Fused conv (see fac_conv1d_fwd).  x (B, C_in, T).  With pad_left=None the SConv1d padding
    rule is applied (causal: everything on the left; non-causal: asymmetric split).
    k1 / dilation2: two-level taps (tap k = k2 * k1 + k1' reads offset k2 * dilation2 + k1' * dilation), see fac_conv_desc.
    alpha_y2: also produce y2 = snake(y, alpha_y2) (returned as (y, y2); y is None if not want_y).
    w_k1 / bias_k1: fused ResidualUnit tail -- y = w_k1 * snake(conv + bias, alpha_out) + bias_k1 + res.
    act=ACT_GATE / ACT_WN_RES_SKIP (streaming hops only, facodec_hip.h): the output has c_out / 2 channels; ACT_WN_RES_SKIP adds
    the first half of the channels to `res` (-> out, which may be res itself) and the second half onto `skip_acc` in place.
    gate_cond (act=ACT_GATE only): (B, c_out) conditioning rows added to the pre-activations before the gate, as
    gate_tanh_sigmoid(a, g) adds them (bit-identical to that pair of launches); may be a column slice of a wider (B, n) tensor.
    The shape-only part of the launch is conv_desc; this function adds what needs the tensors."""
    x_p8 = x if isinstance(x, P8) else None
    if x_p8 is not None:
        B, c_in, t_in = x_p8.shape
    else:
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.stride(2) == 1):
            x = _dev(x, "x")     # channel-sliced views (time contiguous) are consumed in place
        B, c_in, t_in = x.shape
    dev_ = x_p8.planes.device if x_p8 is not None else x.device
    d = conv_desc(B, c_in, t_in, c_out, k, stride, dilation, pad_left, pad_mode, t_out, act, causal, k1, dilation2,
                  w_packed.shape[-1] if w_packed is not None else None,
                  getattr(w_split, "split_rows", 0))         # co-tile size the buffer was packed for (pack_conv_weight_split)
    t_out, c_y = d.T_out, conv_y_channels(c_out, act)
    if out is None and want_y:
        out = torch.empty(B, c_y, t_out, device=dev_, dtype=torch.float32)
    y2 = torch.empty(B, c_out, t_out, device=dev_, dtype=torch.float32) if alpha_y2 is not None else None
    if act == ACT_WN_RES_SKIP:
        assert skip_acc is not None and skip_acc.is_contiguous() and skip_acc.shape == out.shape and alpha_y2 is None
        y2 = skip_acc
    res = _dev(res, "res")
    d.bias = bias.data_ptr() if bias is not None else None
    if x_p8 is not None:
        d.x, d.x_p8, d.x_p8_plane_bytes = None, x_p8.planes.data_ptr(), x_p8.plane_bytes
    else:
        d.x = x.data_ptr()
        d.x_bs, d.x_cs = x.stride(0), x.stride(1)
    d.w = w_packed.data_ptr() if w_packed is not None else w_split.data_ptr()   # split-only launch: see fac_conv_desc.w_split
    d.alpha_in = alpha_in.data_ptr() if alpha_in is not None else None
    d.alpha_out = alpha_out.data_ptr() if alpha_out is not None else None
    d.res = res.data_ptr() if res is not None else None
    d.y = out.data_ptr() if out is not None else None
    d.y2 = y2.data_ptr() if y2 is not None else None
    d.alpha_y2 = alpha_y2.data_ptr() if alpha_y2 is not None else None
    d.w_k1 = w_k1.data_ptr() if w_k1 is not None else None
    d.bias_k1 = bias_k1.data_ptr() if bias_k1 is not None else None
    d.w_split = w_split.data_ptr() if w_split is not None else None
    if out is not None and (out.stride(0), out.stride(1)) != (d.y_bs, d.y_cs) and out.shape[0] * out.shape[1] > 1:
        # a time-contiguous view of a wider buffer as the output (streaming: the LSTM pre-activations of the real batch columns)
        assert out.stride(2) == 1 and y2 is None and res is None and out.shape == (B, c_y, t_out)
        d.y_bs, d.y_cs = out.stride(0), out.stride(1)
    if gate_cond is not None:
        if not (gate_cond.is_cuda and gate_cond.dtype == torch.float32 and gate_cond.dim() == 2 and gate_cond.shape == (B, c_out)
                and (gate_cond.stride(1) == 1 or c_out == 1)):
            raise ValueError(f"gate_cond must be a float32 GPU tensor (B={B}, c_out={c_out}) with contiguous rows, "
                             f"got {tuple(gate_cond.shape)} {gate_cond.dtype} {gate_cond.device}")
        d.gate_cond, d.gate_cond_bs = gate_cond.data_ptr(), gate_cond.stride(0)
    _launch_conv(d, "fac_conv1d_fwd")
    return (out, y2) if alpha_y2 is not None else out


# Streaming hops: the WaveNet's elementwise launches folded into the reduction kernels of its convs (STREAM_FOLD = False: separate
# launches, the round-5 hop; bit-identical either way -- tests/test_gpu_parity.py::test_streaming_folded_epilogues_are_bit_identical)
STREAM_FOLD = True
SKINNY_MAX_COLS = 640


def convtr_desc(B, c_in, t_in, c_out, stride, c_out_pad, causal=True, has_history=False, rows=False, split=False):
    """The launch descriptor of conv_transpose1d from shapes and flags alone, as conv_desc is conv1d's.  t_in: columns of x, the
    history column included.  c_out_pad: padded rows of the weights (pad32(c_out) polyphase, convtr_rows_pad for the rows layouts).
    rows: one of the rows layouts (all phases per workgroup, contiguous stores); split: its split GEMM form (no fp32 weights)."""
    t_cols = t_in - 1 if has_history else t_in
    t_total = t_cols * stride
    d = ConvDesc()
    d.x_bs, d.x_cs = c_in * t_in, t_in
    d.y_bs, d.y_cs = c_out * t_total, t_total
    d.B, d.C_in, d.T_in, d.C_out, d.C_out_pad, d.T_out = B, c_in, t_in, c_out, c_out_pad, t_cols
    d.K, d.stride, d.dilation, d.pad_left, d.pad_mode = 2, 1, 1, (0 if has_history else 1), PAD_ZERO
    d.n_phase, d.y_tstride, d.act, d.w_batched, d.w_bs = stride, stride, ACT_NONE, 0, 0
    # non-causal: trim ceil(s/2) on the left, floor(s/2) on the right (dac/model/encodec.py:265-269)
    d.phase_shift = 0 if causal else stride - stride // 2
    d.gsplit_p8_cols = GSPLIT_P8_COLS
    if rows or split:
        if not causal or has_history:
            raise _lib.FacodecHipError("the all-phases ConvTranspose1d launch is causal and offline only")
        d.n_phase, d.y_tstride, d.phase_shift, d.row_phases = 1, 1, 0, stride
        d.pw_split = 1 if (BF16_SPLIT and PW_SPLIT and PW_TAPS and not split and stride == 2) else 0
    return d


def conv_transpose1d(x, w_packed, c_out, stride, bias=None, alpha_in=None, out=None, alpha_y2=None, causal=True,
                     has_history=False):
    """Causal SConvTranspose1d (kernel 2*stride, right trim k-stride: dac/model/encodec.py:248-270)
    as `stride` polyphase 2-tap convs: y[., t*s+p] = W[p] x[t] + W[p+s] x[t-1].
    has_history (streaming): x's first column is x[t0-1] of an earlier chunk (instead of the zero of
    the start of the signal); x may then be a time-contiguous view of a wider buffer.
    The shape-only part of the launch is convtr_desc."""
    x_p8 = x if isinstance(x, P8) else None
    if x_p8 is not None:       # all-phases split-GEMM launch only (fac_conv1d_fwd rejects P8 operands anywhere else)
        assert not has_history
        B, c_in, t_in = x_p8.shape
    else:
        if not (has_history and x.is_cuda and x.dtype == torch.float32 and x.stride(2) == 1):
            x = _dev(x, "x")
        B, c_in, t_in = x.shape
    dev_ = x_p8.planes.device if x_p8 is not None else x.device
    if has_history:
        assert causal
    split_rows = isinstance(w_packed, tuple)       # (split GEMM buffer, rows) from pack_convtr_weight_rows_split
    d = convtr_desc(B, c_in, t_in, c_out, stride, w_packed[1] if split_rows else w_packed.shape[-1], causal, has_history,
                    not split_rows and w_packed.dim() == 3, split_rows)
    if out is None:
        out = torch.empty(B, c_out, d.T_out * stride, device=dev_, dtype=torch.float32)
    d.bias = bias.data_ptr() if bias is not None else None
    if x_p8 is not None:
        d.x, d.x_p8, d.x_p8_plane_bytes = None, x_p8.planes.data_ptr(), x_p8.plane_bytes
    else:
        d.x = x.data_ptr()
        d.x_bs, d.x_cs = x.stride(0), x.stride(1)
    if split_rows:
        d.w, d.w_split = None, w_packed[0].data_ptr()
    else:
        d.w = w_packed.data_ptr()
    d.alpha_in = alpha_in.data_ptr() if alpha_in is not None else None
    d.alpha_out, d.res, d.y = None, None, out.data_ptr()
    y2 = torch.empty_like(out) if alpha_y2 is not None else None
    d.y2 = y2.data_ptr() if y2 is not None else None
    d.alpha_y2 = alpha_y2.data_ptr() if alpha_y2 is not None else None
    _launch_conv(d, "fac_conv1d_fwd(convtr)")
    return (out, y2) if alpha_y2 is not None else out


# Short clips on the split GEMM kernel as ONE flattened signal (conv1d_flat / conv_transpose1d_flat; round 4, inference) for the
# TRAINING launches too (round 6): per-clip column tiles would be half empty at the 160-frame latent rate, so the encoder's last strided
# conv, the decoder's first ConvTranspose1d and their data gradients fell to the fp32 128 x 160 tile (r06_train_layers_serial.log: 3.9 ms).
FLAT_TRAIN = True
# k = 1 ResidualUnit tails at C = 64 .. 384 on the bf16 pipe inside the streaming kernel (conv1d_pw_split.hip); 0: fp32 MFMAs (rounds 2-5)
PW_SPLIT = os.environ.get("FAC_PW_SPLIT", "1") != "0"
# stride-2 layers with few channels on the streaming kernel with taps (conv1d_pw_split.hip, conv1d_pwt_kernel); follows PW_SPLIT
PW_TAPS = True
# k = 1 fp32 launches of 129 .. 160 columns per clip whose 128 x 160 tiles would be fewer than 256 workgroups (the style path's
# 1025 -> 80, 80 -> 512, 20 -> 256 at 32 clips) on five 128 x 32 tiles per clip (conv1d_api.hip: select_variant); False: the wide tile
K1_COLUMN_TILES = True
# Split GEMM launches with a P8 input on the form that reads its input fragments straight from the planes, 64 x 256 / 64 x 128 tiles,
# two workgroups per CU (conv1d_gemm_split_p8.hip; which shapes: conv_gsplit_p8_ncb there).  fac_conv_desc.gsplit_p8_cols: 0 = the
# library chooses; -1 = every such launch stays on the 128 x 128 form, what the tree launched before that form existed; 256 / 128 =
# that tile on every such launch (tests) -- the same bits whichever.
GSPLIT_P8_COLS = 0


def pack_conv_for(layout, v, g, stride=1, k1=0, scale=None):
    """(fp32 pack, split buffer), one of them None: the weights in the layout a ConvPlan names."""
    if layout in (W_FP32, W_FP32_PW_TAPS):
        return pack_conv_weight(v, g, scale=scale), None
    if layout == W_GEMM_STRIDED:
        return None, pack_gemm_weight_split(v, g, in_stride=stride, scale=scale)
    if layout == W_SPLIT2:
        return None, pack_conv_weight_split2(v, g, k1, scale=scale)
    return None, pack_conv_weight_split(v, g, scale=scale, rows=64)          # W_TAPS / W_GEMM (training sites: tile_rows(grad=True))


def pack_convtr_for(layout, v, g, stride):
    """The weights conv_transpose1d wants in the layout a ConvTrPlan names ((split GEMM buffer, rows) for the bf16-pipe launches)."""
    if layout in (TR_ROWS_SPLIT, TR_FLAT):
        return pack_convtr_weight_rows_split(v, g, stride)
    return pack_convtr_weight(v, g, stride) if layout == TR_POLYPHASE else pack_convtr_weight_rows(v, g, stride)


def convtr_weight_for(v, g, stride, t_in, causal=True, batch=1, alpha_in=None):
    """The packed weights of the per-clip launch for an input of `batch` clips of t_in columns."""
    return pack_convtr_for(plan_convtr(v.shape[0], v.shape[1], stride, batch, t_in, causal=causal, alpha_in=alpha_in is not None).layout,
                           v, g, stride)


def flat_conv_cols(B, L, s, n):
    """(pitch, t_in, t_out) of conv1d_flat's one signal: B clips padded to L columns each, n outputs kept per clip."""
    pitch = L // s
    return pitch, B * L, B * pitch - (pitch - n)


def flat_convtr_cols(B, T1):
    """Columns of conv_transpose1d_flat's one signal: B clips of T1 columns, their zero column included."""
    return B * T1


def conv1d_flat(xp, w_split, c_out, k, s, n, dilation=1, bias=None, p8=None, alpha_out=None, act=ACT_NONE, alpha_y2=None, want_y=True):
    """Short clips as ONE signal.  xp (B, C_in, L): every clip already padded to length L -- reflected on the left by k - s = s
    samples (causal strided conv, L = (n + 1) s) or by (k - 1) d samples (causal stride-1 conv, L = n + (k - 1) d), or zeros
    around the dy of a transposed conv.  The clips are laid one after another and the conv runs WITHOUT padding at stride s:
    with pitch = L // s output columns per clip, column b pitch + t is output t of clip b -- the same products in the same order as
    the per-clip launch, so the same bits -- and the pitch - n columns where the window straddles two clips are dropped on the way
    back -> (B, C_out, n); t_out = B pitch - (pitch - n).  p8: the plan's figure for ops.p8_prepass.  Returns what conv1d returns."""
    B, c_in, L = xp.shape
    pitch, t_in, t_out = flat_conv_cols(B, L, s, n)
    xf = p8_prepass(xp.permute(1, 0, 2).reshape(1, c_in, t_in), p8)                 # data movement only
    got = conv1d(xf, None, c_out, k, bias=bias, stride=s, dilation=dilation, pad_left=0, pad_mode=PAD_ZERO, t_out=t_out,
                 alpha_out=alpha_out, act=act, alpha_y2=alpha_y2, want_y=want_y, w_split=w_split)

    def back(y):
        if y is None:
            return None
        full = torch.empty(c_out, B * pitch, device=y.device, dtype=y.dtype)
        full[:, :t_out] = y[0]
        return full.reshape(c_out, B, pitch)[:, :, :n].permute(1, 0, 2).contiguous()

    return (back(got[0]), back(got[1])) if alpha_y2 is not None else back(got)


def conv_transpose1d_flat(xz, w_rows_split, c_out, s, trim=0, bias=None, alpha_y2=None, p8=None):
    """xz (B, C_in, T'): clips that already hold their zero column -- in FRONT for the forward transposed conv (the x[t - 1] of a
    clip's first frame; trim = s drops that column's s output samples), at the END for the data gradient of a strided conv (where
    it is the next clip's x[t - 1] as well; nothing to trim).  One signal of B T' columns through the all-phases split-GEMM launch
    -> (B, C_out, T' s - trim): per clip exactly the per-clip launch's output (y[t s + p] = W[p] x[t] + W[p + s] x[t - 1])."""
    B, c_in, T1 = xz.shape
    xf = p8_prepass(xz.permute(1, 0, 2).reshape(1, c_in, flat_convtr_cols(B, T1)), p8)
    got = conv_transpose1d(xf, w_rows_split, c_out, s, bias=bias, alpha_y2=alpha_y2, causal=True)
    back = lambda y: y.reshape(c_out, B, T1 * s)[:, :, trim:].permute(1, 0, 2).contiguous()   # noqa: E731
    return (back(got[0]), back(got[1])) if alpha_y2 is not None else back(got)


def snake(x, alpha, out=None):
    x = _dev(x, "x")
    B, c, t = x.shape
    if out is None:
        out = torch.empty_like(x)
    _lib.check(_lib.load().fac_snake_fwd(_ptr(x), _ptr(alpha), _ptr(out), B, c, t, _stream()), "fac_snake_fwd")
    return out


# --------------------------------------------------------------------------------- LSTM (K5)
def lstm_to_time_major(x):
    x = _dev(x, "x")
    B, H, T = x.shape
    xT = torch.empty(H, T, pad32(B), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_lstm_to_time_major(_ptr(x), _ptr(xT), B, H, T, _stream()), "fac_lstm_to_time_major")
    return xT


def lstm_from_time_major(yT, skip, B, alpha=None):
    H, T, BP = yT.shape
    out = torch.empty(B, H, T, device=yT.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_lstm_from_time_major(_ptr(yT), _ptr(skip), _ptr(alpha), _ptr(out), B, H, T, _stream()),
               "fac_lstm_from_time_major")
    return out


def plan_lstm_proj(H, cols):
    """An LSTM layer's input projection W_ih (4H, H) over the cols = T * BP columns of the time-major buffer, as one 1x1 conv."""
    return plan_gemm(4 * H, H, cols)


def plan_lstm_proj_bwd(H, cols):
    """Its data gradient W_ih^T dgates over the same columns."""
    return plan_gemm(H, 4 * H, cols)


def lstm_input_proj(inp, w_ih, bias):
    """inp (H, T, BP) time-major, raw w_ih (4H, H), bias = b_ih + b_hh -> the pre-activations (4H, T, BP): one GEMM over every
    (t, b), the channel-major buffer as a (1, H, T * BP) "signal" (plan, pre-pass, pack, conv1d)."""
    H, T, BP = inp.shape
    plan = plan_lstm_proj(H, T * BP)
    sig = p8_prepass(inp.view(1, H, T * BP), plan.p8)
    pre = conv1d(sig, pack_conv_weight(w_ih) if plan.layout == W_FP32 else None, 4 * H, 1, bias=bias, pad_left=0, t_out=T * BP,
                 pad_mode=PAD_ZERO, w_split=pack_gemm_weight_split(w_ih) if plan.layout == W_GEMM else None)
    return pre.view(4 * H, T, BP)


def pack_lstm_whh(w_hh, out=None):
    w_hh = _dev(w_hh, "weight_hh")
    H = w_hh.shape[1]
    if out is None:
        out = torch.empty_like(w_hh)
    _lib.check(_lib.load().fac_pack_lstm_whh(_ptr(w_hh), _ptr(out), H, _stream()), "fac_pack_lstm_whh")
    return out


LSTM_PERSIST = True
LSTM_PERSIST_MAX_BATCH = 16


_LSTM_ARMED = set()


def _lstm_arm():
    """The resident kernels' waits give up after 4 s without progress and count that in a host-mapped word the device has to be
    told about (fac_lstm_persist_arm: one one-thread kernel, once per device, outside any stream capture).  A device whose word is
    not armed answers fac_lstm_persist_ok = 0, so the word is armed here, eagerly, the first time anybody asks."""
    dev = torch.cuda.current_device()
    if dev in _LSTM_ARMED:
        return
    if torch.cuda.is_current_stream_capturing():
        return                                   # not now; the per-step kernels take this call, a later eager call arms
    if _lib.load().fac_lstm_persist_arm(_stream()):
        _LSTM_ARMED.add(dev)


def lstm_timeouts():
    """Resident-LSTM waits that gave up in this process so far (host-mapped counter: no synchronisation; it counts what the device
    has EXECUTED, so a caller that wants the verdict on launches it just queued synchronises first)."""
    return int(_lib.load().fac_lstm_persist_timeouts())


def raise_if_lstm_timed_out(what="resident LSTM launch"):
    """Results of a resident launch whose wait gave up are meaningless.  Training is protected on the device (optim.FlatAdamW: the
    abort flag travels with the per-parameter flags and the masked AdamW step steps nothing on ANY rank); this is the host-side
    report for inference callers and benchmarks, to be called behind a synchronisation point."""
    n = lstm_timeouts()
    if n:
        raise _lib.FacodecHipError(f"{what}: {n} resident-LSTM wait(s) timed out on this device -- the outputs of that launch are "
                                   "meaningless (later layers use the per-step kernels: fac_lstm_persist_ok answers 0 from now on)")


def lstm_persist_ok(H, batch):
    """True when the one-launch-per-layer recurrence (lstm_persist.hip) is used for an (H, batch) zero-initial-state
    layer on this device: H in {512, 1024, 1536}, H/8 workgroups <= CUs, batch <= 16.  The kernels cover batch <= 32
    (two 16-column blocks) but measure no faster than the per-step launches there (profiles/r03_lstm_bench.log)."""
    if not (LSTM_PERSIST and batch is not None and batch <= LSTM_PERSIST_MAX_BATCH) or _ranks_share_a_device():
        return False
    _lstm_arm()
    return (bool(_lib.load().fac_lstm_persist_ok(int(H), int(batch)))
            and bool(_lib.load().fac_lstm_persist_stream_ok(_stream())))


LSTM_PERSIST_SPLIT = True
LSTM_PERSIST_SPLIT_MIN_BATCH = 17


LSTM_PERSIST_SPLIT_MAX_SCRATCH = int(float(os.environ.get("FAC_LSTM_PERSIST_SPLIT_MAX_SCRATCH_GB", "1")) * 2 ** 30)


def lstm_persist_split_ok(H, batch, T=None):
    """True when an inference layer runs on the resident kernel with bf16 x 3 operands (lstm_persist.hip,
    fac_lstm_layer_fwd_persist_split): 17 .. 32 batch columns, where the fp32 resident kernel is bound by its fp32 MFMA time and
    the per-step kernel by re-streaming W_hh.  Follows BF16_SPLIT like the conv kernels of the same arithmetic.
    T (frames): the kernel needs one fresh exchange region per step, T * H * 32 * 6 bytes of scratch per layer call -- 47 MB at the
    benchmark's 160 frames, but 1.5 - 3 GB for 30-second clips; above FAC_LSTM_PERSIST_SPLIT_MAX_SCRATCH_GB (1) the per-step kernels,
    which need none, take the layer."""
    if T is not None and int(T) * int(H) * 32 * 6 > LSTM_PERSIST_SPLIT_MAX_SCRATCH:
        return False
    if not (LSTM_PERSIST and LSTM_PERSIST_SPLIT and BF16_SPLIT and batch is not None
            and LSTM_PERSIST_SPLIT_MIN_BATCH <= batch <= 32) or _ranks_share_a_device():
        return False
    _lstm_arm()
    return (bool(_lib.load().fac_lstm_persist_split_ok(int(H), int(batch)))
            and bool(_lib.load().fac_lstm_persist_stream_ok(_stream())))


def pack_lstm_whh_split(w_hh):
    """W_hh (4H, H) as the three-plane bf16 A fragments of the split resident kernel (fac_pack_lstm_whh_split)."""
    w_hh = _dev(w_hh, "weight_hh")
    out = torch.empty(w_hh.numel() * 6, device=w_hh.device, dtype=torch.uint8)
    _lib.check(_lib.load().fac_pack_lstm_whh_split(_ptr(w_hh), _ptr(out), w_hh.shape[1], _stream()), "fac_pack_lstm_whh_split")
    return out


def lstm_layer_persist_split(pre, w_hh, H, batch):
    """The whole inference layer in ONE launch on the bf16 matrix pipe: pre (4H, T, BP), raw W_hh (4H, H) -> yT (H, T, BP)."""
    _, T, BP = pre.shape
    if _FLOPS is not None:
        _FLOPS.add("lstm", 2.0 * 4 * H * H * T * BP)
    yT = torch.empty(H, T, BP, device=pre.device, dtype=torch.float32)
    if BP > 32:
        yT[..., 32:].zero_()
    hsplit = torch.empty(T * H * 32 * 6, device=pre.device, dtype=torch.uint8)       # one fresh exchange region per step
    _lib.check(_lib.load().fac_lstm_layer_fwd_persist_split(_ptr(pre), _ptr(pack_lstm_whh_split(w_hh)), _ptr(hsplit), _ptr(yT),
                                                            T, H, batch, BP, _stream()), "fac_lstm_layer_fwd_persist_split")
    return yT


def _ranks_share_a_device():
    """The resident LSTM grids of two PROCESSES on one GPU could each hold part of the CUs and spin on workgroups that never get
    one (launches are only serialised inside a process, lstm_persist.hip): with more local ranks than visible devices (the
    two-ranks-on-one-GPU smoke mode of tools/ddp_smoke.py) the per-step kernels are used instead."""
    try:
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", "1"))
    except ValueError:
        local_world = 1
    return local_world > max(1, torch.cuda.device_count())


def pack_lstm_whh16(w_hh, transposed=False):
    """W_hh (4H, H) as the register fragments of the resident kernels (fac_pack_lstm_whh16)."""
    w_hh = _dev(w_hh, "weight_hh")
    out = torch.empty_like(w_hh)
    _lib.check(_lib.load().fac_pack_lstm_whh16(_ptr(w_hh), _ptr(out), w_hh.shape[1], 1 if transposed else 0, _stream()),
               "fac_pack_lstm_whh16")
    return out


def _zero_pad_cols(t, nc):
    """Columns >= nc of a (rows, T, BP) work buffer are batch padding the resident kernels never touch."""
    if nc < t.shape[-1]:
        t[..., nc:].zero_()


def lstm_layer_persist(pre, w_hh, H, batch, save=None):
    """The whole layer in ONE launch (fac_lstm_layer_fwd_persist): pre (4H, T, BP), raw W_hh (4H, H) -> yT (H, T, BP)."""
    _, T, BP = pre.shape
    nc = 16 * ((batch + 15) // 16)
    if _FLOPS is not None:
        _FLOPS.add("lstm", 2.0 * 4 * H * H * T * BP)
    yT = torch.empty(H, T, BP, device=pre.device, dtype=torch.float32)
    _zero_pad_cols(yT, nc)
    sg, sc = save if save is not None else (None, None)
    if save is not None:
        _zero_pad_cols(sg, nc)
        _zero_pad_cols(sc, nc)
    hfrag = torch.empty(T * H * nc, device=pre.device, dtype=torch.float32)       # one fresh exchange region per step
    _lib.check(_lib.load().fac_lstm_layer_fwd_persist(_ptr(pre), _ptr(pack_lstm_whh16(w_hh)), _ptr(hfrag), _ptr(yT), _ptr(sg),
                                                      _ptr(sc), T, H, batch, BP, _stream()), "fac_lstm_layer_fwd_persist")
    return yT


def lstm_layer(pre, whh_packed, H, state=None, step0=0, save=None):
    """pre (4H, T, BP) -> yT (H, T, BP).  state (3, H, BP): carried cell / hidden buffers of a streaming
    session with `step0` steps already taken (None: fresh zero state).  save = (gates (4H,T,BP), c (H,T,BP)):
    training mode, the activations back-propagation through time needs are stored there."""
    _, T, BP = pre.shape
    if _FLOPS is not None:
        _FLOPS.add("lstm", 2.0 * 4 * H * H * T * BP)
    yT = torch.empty(H, T, BP, device=pre.device, dtype=torch.float32)
    if state is None:
        state = torch.empty(3, H, BP, device=pre.device, dtype=torch.float32)   # cell state + 2 fragment-ordered h
        step0 = 0
    sg, sc = save if save is not None else (None, None)
    _lib.check(_lib.load().fac_lstm_layer_fwd_train(_ptr(pre), _ptr(whh_packed), _ptr(yT), _ptr(state), _ptr(sg), _ptr(sc),
                                                    T, H, BP, step0, _stream()), "fac_lstm_layer_fwd")
    return yT


def stream_push(buf, src, hist, n_prev):
    """buf (B, C, cap) left-context buffer; appends src (B, C, n) behind the last `hist` columns."""
    src = _dev(src, "src")
    B, c, cap = buf.shape
    assert buf.is_contiguous() and src.shape[:2] == buf.shape[:2]
    _lib.check(_lib.load().fac_stream_push(_ptr(buf), _ptr(src), B * c, cap, hist, n_prev, src.shape[-1], _stream()),
               "fac_stream_push")


# --------------------------------------------------------------------------------- VQ (K7)
def vq_step(z_in, w_in_packed, b_in, codebook, w_out, w_out_scale, b_out, codes_out, residual=None, zq_acc=None,
            zq_out=None, mask=None, z_e=None, loss_part=None):
    """One VectorQuantize.forward (dac/nn/quantize.py:34-70) + RVQ bookkeeping (:173-193).
    codes_out: int64 view (B, T) (may be a strided slice of a (B, N, T) tensor)."""
    z_in = _dev(z_in, "z")
    B, D, T = z_in.shape
    assert codes_out.dtype == torch.int64 and codes_out.stride(-1) == 1
    d = VqDesc()
    d.residual = residual.data_ptr() if residual is not None else None
    d.z_in = z_in.data_ptr()
    d.zq_acc = zq_acc.data_ptr() if zq_acc is not None else None
    d.zq_out = zq_out.data_ptr() if zq_out is not None else None
    d.w_in, d.b_in, d.codebook = w_in_packed.data_ptr(), b_in.data_ptr(), codebook.data_ptr()
    d.w_out, d.b_out = w_out.data_ptr(), b_out.data_ptr()
    d.w_out_scale = w_out_scale.data_ptr() if w_out_scale is not None else None
    d.mask = mask.data_ptr() if mask is not None else None
    d.codes = codes_out.data_ptr()
    d.z_e = z_e.data_ptr() if z_e is not None else None
    d.loss_part = loss_part.data_ptr() if loss_part is not None else None
    d.codes_bs = codes_out.stride(0)
    d.B, d.D, d.T, d.Kc = B, D, T, codebook.shape[0]
    _lib.check(_lib.load().fac_vq_fwd(C.byref(d), _stream()), "fac_vq_fwd")


def vq_decode(codes, weights, style, Kc, out=None, z_out=(None, None, None), n_use=None):
    """Codes of the prosody / content / residual RVQs -> decoder input (fac_vq_decode: from_codes of each RVQ, their sum, the
    timbre-conditioned LayerNorm).  codes: three int64 (B, n_r, T) tensors (any batch / row stride, unit frame stride) or None
    for an RVQ without quantizers; weights: per RVQ a list of n_r tuples (codebook (Kc, 8), out_proj weight_v (D, 8, 1),
    weight-norm scale (D) or None, bias (D)); style (B, 2D) = [gamma | beta].  z_out: optional (B, D, T) buffers for the
    per-RVQ sums.  Codes are not range checked here (the kernel clamps them for the load).
    n_use: optional int32 (B, T, 3) on the device (any batch / frame stride, unit stride over the three counts): the number of
    leading quantizers of each RVQ that frame (b, t) is decoded from (fac_vq_decode_masked) -- every frame then
    equals, bit for bit, the frame of a call whose codes and weights are cut to those counts."""
    style = _dev(style, "style")
    B, D2 = style.shape
    D = D2 // 2
    md = _lib.VqDecodeMaskedDesc() if n_use is not None else None
    d = md.base if md is not None else VqDecodeDesc()
    T, q = None, 0
    for r in range(3):
        c, ws = codes[r], weights[r]
        n = 0 if c is None else c.shape[1]
        if n != len(ws):
            raise ValueError(f"vq_decode: RVQ {r} has {n} code rows but {len(ws)} weight sets")
        if c is not None:
            if not c.is_cuda:
                raise _lib.FacodecHipError(f"codes must live on the GPU (got {c.device}); there is no CPU path")
            assert c.dtype == torch.int64 and c.dim() == 3 and c.shape[0] == B and (c.stride(-1) == 1 or c.shape[-1] == 1)
            if T is None:
                T = c.shape[-1]
            assert c.shape[-1] == T
            d.codes[r], d.codes_bs[r], d.codes_qs[r] = c.data_ptr(), c.stride(0), c.stride(1)
        d.n_q[r] = n
        for cb, wv, sc, bo in ws:
            if q >= _lib.VQ_DECODE_MAX_Q:
                raise ValueError(f"vq_decode: more than {_lib.VQ_DECODE_MAX_Q} quantizers")
            d.codebook[q], d.w_out[q], d.b_out[q] = _dev(cb, "codebook").data_ptr(), _dev(wv, "weight_v").data_ptr(), _dev(bo, "bias").data_ptr()
            d.w_out_scale[q] = _dev(sc, "scale").data_ptr() if sc is not None else None
            q += 1
    if T is None:
        raise ValueError("vq_decode: no codes (the frame count comes from them)")
    if out is None:
        out = torch.empty(B, D, T, device=style.device, dtype=torch.float32)
    d.style, d.outs = style.data_ptr(), out.data_ptr()
    for r in range(3):
        zo = z_out[r]
        if zo is not None:
            assert zo.is_contiguous() and tuple(zo.shape) == (B, D, T) and zo.dtype == torch.float32
        d.z[r] = zo.data_ptr() if zo is not None else None
    assert out.is_contiguous() and tuple(out.shape) == (B, D, T)
    d.B, d.D, d.T, d.Kc = B, D, T, Kc
    if md is not None:
        if not isinstance(n_use, torch.Tensor) or not n_use.is_cuda:
            raise _lib.FacodecHipError(f"vq_decode: n_use must live on the GPU (got {getattr(n_use, 'device', type(n_use))}); there is no CPU path")
        if n_use.dtype != torch.int32 or tuple(n_use.shape) != (B, T, 3) or n_use.stride(2) != 1:
            raise ValueError(f"vq_decode: n_use must be int32 ({B}, {T}, 3) with unit stride over the counts, got {n_use.dtype} "
                             f"{tuple(n_use.shape)} strides {tuple(n_use.stride())}")
        md.n_use, md.n_use_bs, md.n_use_ts = n_use.data_ptr(), n_use.stride(0), n_use.stride(1)
        _lib.check(_lib.load().fac_vq_decode_masked(C.byref(md), _stream()), "fac_vq_decode_masked")
        return out
    _lib.check(_lib.load().fac_vq_decode(C.byref(d), _stream()), "fac_vq_decode")
    return out


class PlcState:
    """Device-resident concealment state of B rows (fac_plc_select): last_codes (B, Q) int64, last_n (B, 3) int32, the gain g (B)
    fp32 (1: nothing is faded) and run (B) int32, the concealed frames in a row."""

    def __init__(self, B, n_q, device):
        self.B, self.n_q = int(B), tuple(int(n) for n in n_q)
        self.last_codes = torch.zeros(self.B, sum(self.n_q), dtype=torch.int64, device=device)
        self.last_n = torch.zeros(self.B, 3, dtype=torch.int32, device=device)
        self.g = torch.ones(self.B, dtype=torch.float32, device=device)
        self.run = torch.zeros(self.B, dtype=torch.int32, device=device)


def _plc_codes(d, name, codes, counts, B, k, what):
    ptr, bs, qs = getattr(d, name), getattr(d, name + "_bs"), getattr(d, name + "_qs")
    for r in range(3):
        if counts[r] == 0:
            continue
        c = codes[r] if codes is not None else None
        if not isinstance(c, torch.Tensor) or not c.is_cuda:
            raise _lib.FacodecHipError(f"plc_select: {what} codes must live on the GPU (RVQ {r}: {getattr(c, 'device', type(c))}); there is no CPU path")
        if c.dtype != torch.int64 or tuple(c.shape) != (B, counts[r], k) or (k > 1 and c.stride(2) != 1):
            raise ValueError(f"plc_select: {what} codes of RVQ {r} must be int64 ({B}, {counts[r]}, {k}) with unit frame stride, got "
                             f"{c.dtype} {tuple(c.shape)} strides {tuple(c.stride())}")
        ptr[r], bs[r], qs[r] = c.data_ptr(), c.stride(0), c.stride(1)


def plc_select(prim, red, status, state, dst, n_use, ramp, n_red=(0, 0, 0), hold=2, fade=6, recover=1):
    """One push of the concealment state machine (fac_plc_select): per row, status (B) int32 (0 PRIMARY, 1 REDUNDANT,
    2 LOST) picks what dst -- three int64 (B, n_q[r], k) tensors, possibly prim itself -- is filled with: prim, the redundant
    codes red ((B, n_red[r], k), quantizers beyond n_red written as 0), or the state's last played frame.  Writes n_use (B, k, 3)
    int32 for ops.vq_decode, ramp (B, k + 1) fp32 for plc_gain, and advances `state` (PlcState).  One launch, nothing read back."""
    B, n_q = state.B, state.n_q
    n_red = tuple(int(n) for n in n_red)
    k = next(c for c, n in zip(prim, n_q) if n).shape[-1]
    d = _lib.PlcSelectDesc()
    _plc_codes(d, "prim", prim, n_q, B, k, "primary")
    _plc_codes(d, "red", red, n_red, B, k, "redundant")
    _plc_codes(d, "dst", dst, n_q, B, k, "destination")
    for r in range(3):
        d.n_q[r], d.n_red[r] = n_q[r], n_red[r]
    for t, dt, shape, what in ((status, torch.int32, (B,), "status"), (n_use, torch.int32, (B, k, 3), "n_use"),
                               (ramp, torch.float32, (B, k + 1), "ramp")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.FacodecHipError(f"plc_select: {what} must live on the GPU; there is no CPU path")
        if t.dtype != dt or tuple(t.shape) != shape:
            raise ValueError(f"plc_select: {what} must be {dt} {shape}, got {t.dtype} {tuple(t.shape)}")
    if not status.is_contiguous() or not ramp.is_contiguous() or n_use.stride(2) != 1:
        raise ValueError("plc_select: status and ramp must be dense, n_use needs unit stride over the counts")
    d.status, d.last_codes, d.last_n, d.g, d.run = status.data_ptr(), state.last_codes.data_ptr(), state.last_n.data_ptr(), \
        state.g.data_ptr(), state.run.data_ptr()
    d.n_use, d.n_use_bs, d.n_use_ts, d.ramp = n_use.data_ptr(), n_use.stride(0), n_use.stride(1), ramp.data_ptr()
    d.B, d.k, d.hold, d.fade, d.recover = B, k, int(hold), int(fade), int(recover)
    _lib.check(_lib.load().fac_plc_select(C.byref(d), _stream()), "fac_plc_select")


def plc_gain(wave, ramp, out=None, frame=300):
    """wave (B, 1, k frame) or (B, k frame) fp32 times the piecewise-linear gain through ramp (B, k + 1) (fac_plc_gain): sample n
    of frame f is scaled by ramp[f] + (ramp[f + 1] - ramp[f]) * ((n + 1) / frame), each operation rounded on its own.  out may be
    wave (in place); a row whose ramp is 1 everywhere comes back bit for bit."""
    wave = _dev(wave, "wave")
    ramp = _dev(ramp, "ramp")
    B, k = ramp.shape[0], ramp.shape[1] - 1
    if wave.shape[0] != B or wave.numel() != B * k * frame or (wave.shape[-1] > 1 and wave.stride(-1) != 1) or not ramp.is_contiguous():
        raise ValueError(f"plc_gain: wave {tuple(wave.shape)} does not hold {B} rows of {k} x {frame} samples (ramp {tuple(ramp.shape)})")
    if out is None:
        out = torch.empty_like(wave, memory_format=torch.contiguous_format)
    if out.shape != wave.shape or out.dtype != torch.float32 or not out.is_cuda or (out.shape[-1] > 1 and out.stride(-1) != 1):
        raise ValueError(f"plc_gain: out must be a float32 device tensor of shape {tuple(wave.shape)}")
    x_bs = wave.stride(0) if B > 1 else k * frame
    y_bs = out.stride(0) if B > 1 else k * frame
    _lib.check(_lib.load().fac_plc_gain(_ptr(wave), x_bs, _ptr(out), y_bs, _ptr(ramp), B, k, int(frame), _stream()), "fac_plc_gain")
    return out


# --------------------------------------------------------------------------------- voice activity
def vad_params(frame=300, window=120, hangover=16, margin_db=6.0, floor_db=-70.0):
    """-> (frame, W, H, margin, thr_abs) of fac_vad_decide: margin = 10 ** (margin_db / 10) (a linear power ratio above 1) and
    thr_abs = frame * 10 ** (floor_db / 10) (a per-frame energy sum), both in Python floats.  The defaults -- 1.5 s of minimum
    statistics, 200 ms of hangover, 6 dB over the noise floor, -70 dBFS absolute -- were not tuned by listening."""
    frame, W, H = int(frame), int(window), int(hangover)
    if not 1 <= frame <= _lib.VAD_MAX_FRAME:
        raise ValueError(f"vad: frame = {frame} outside 1 .. {_lib.VAD_MAX_FRAME}")
    if not 1 <= W <= _lib.VAD_MAX_WINDOW or not 0 <= H <= _lib.VAD_MAX_WINDOW:
        raise ValueError(f"vad: window = {W} (1 .. {_lib.VAD_MAX_WINDOW}), hangover = {H} (0 .. {_lib.VAD_MAX_WINDOW})")
    margin = 10.0 ** (float(margin_db) / 10.0)
    if not margin > 1.0:
        raise ValueError(f"vad: margin_db = {margin_db} (above 0 dB)")
    return frame, W, H, margin, frame * 10.0 ** (float(floor_db) / 10.0)


def vad_energy(x, e, frame, f0=0, R=None, lens=None, carry_in=None, carry_n=0, carry_out=None, final=True):
    """fac_vad_energy: frame energies of x (B, k) float32 behind the carry into e (B, >= R) float64 (ring of R columns, first
    frame at column f0 % R) -> the number of frames written."""
    B, k = x.shape
    R = e.shape[1] if R is None else int(R)
    d = _lib.VadEnergyDesc()
    d.carry_in = carry_in.data_ptr() if carry_in is not None else None
    d.carry_out = carry_out.data_ptr() if carry_out is not None else None
    d.x, d.lens, d.e = x.data_ptr(), (_lens(lens, B).data_ptr() if lens is not None else None), e.data_ptr()
    d.x_bs, d.e_bs, d.f0 = (x.stride(0) if B > 1 else k), (e.stride(0) if B > 1 else e.shape[1]), int(f0)
    d.B, d.k, d.frame, d.carry_n, d.is_final, d.R = B, k, int(frame), int(carry_n), 1 if final else 0, R
    _lib.check(_lib.load().fac_vad_energy(C.byref(d), _stream()), "fac_vad_energy")
    total = int(carry_n) + k
    return total // frame + (1 if final and total % frame else 0)


def vad_decide(e, f0, n_new, W, H, margin, thr_abs, frame, R=None, lens=None, flags=None, ring=None):
    """fac_vad_decide over the energy ring e (B, >= R) float64: flags (B, >= n_new) uint8 (any row pitch) and / or the flag ring
    (B, >= R) uint8 for frames f0 .. f0 + n_new - 1."""
    B = e.shape[0]
    R = e.shape[1] if R is None else int(R)
    d = _lib.VadDecideDesc()
    d.e, d.lens = e.data_ptr(), (_lens(lens, B).data_ptr() if lens is not None else None)
    d.e_bs = e.stride(0) if B > 1 else e.shape[1]
    for name, t, n in (("flags", flags, n_new), ("ring", ring, R)):
        if t is None:
            continue
        if not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 2 or t.shape[0] != B or t.shape[1] < n or (t.shape[1] > 1 and t.stride(1) != 1):
            raise ValueError(f"vad_decide: {name} must be uint8 ({B}, >= {n}) on the GPU with dense rows, got {t.dtype} {tuple(t.shape)}")
        setattr(d, name, t.data_ptr())
        setattr(d, name + "_bs", t.stride(0) if B > 1 else t.shape[1])
    d.f0, d.margin, d.thr_abs = int(f0), float(margin), float(thr_abs)
    d.B, d.n_new, d.R, d.W, d.H, d.frame = B, int(n_new), R, int(W), int(H), int(frame)
    _lib.check(_lib.load().fac_vad_decide(C.byref(d), _stream()), "fac_vad_decide")


def vad(x, lens=None, frame=300, window=120, hangover=16, margin_db=6.0, floor_db=-70.0):
    """Voice activity of x (B, T) or (B, 1, T) float32 on the GPU -> (flags (B, F) uint8, energy (B, F) float64), F = ceil(T /
    frame) frames of `frame` samples (the last one may be partial).  energy is the fp64 sum over the frame of the squared
    pre-emphasised signal x[n] - 0.97 x[n - 1]; a frame is raw-active when its energy exceeds thr_abs = frame * 10 ** (floor_db /
    10) and margin = 10 ** (margin_db / 10) times the minimum energy of the last `window` frames, and active when any of the
    last hangover + 1 frames is raw-active (fac_vad_energy, fac_vad_decide: two launches, the arithmetic is pinned in
    include/facodec_hip.h).  lens (B,) int32 on the device: row b is its first lens[b] samples, the frames behind are energy 0
    and flag 0.  The defaults (1.5 s, 200 ms, 6 dB, -70 dBFS) were not tuned by listening."""
    frame, W, H, margin, thr_abs = vad_params(frame, window, hangover, margin_db, floor_db)
    x = _rows(x, "vad")
    B, T = x.shape
    F = -(-T // frame)
    e = torch.empty(B, F, device=x.device, dtype=torch.float64)
    flags = torch.empty(B, F, device=x.device, dtype=torch.uint8)
    if B == 0 or F == 0:
        return flags, e
    vad_energy(x, e, frame, lens=lens)
    vad_decide(e, 0, F, W, H, margin, thr_abs, frame, lens=lens, flags=flags)
    return flags, e


def vad_take(ring, f0, k, out):
    """fac_vad_take: out (B, k) uint8 (any row pitch, e.g. the tail columns of another buffer) = columns (f0 + j) % R of ring."""
    B, R = ring.shape
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.uint8 or tuple(out.shape) != (B, k) or (k > 1 and out.stride(1) != 1):
        raise ValueError(f"vad_take: out must be uint8 ({B}, {k}) on the GPU with dense rows, got {getattr(out, 'dtype', type(out))} "
                         f"{tuple(getattr(out, 'shape', ()))}")
    _lib.check(_lib.load().fac_vad_take(_ptr(ring), ring.stride(0) if B > 1 else R, R, int(f0), int(k), _ptr(out),
                                        out.stride(0) if B > 1 else k, B, _stream()), "fac_vad_take")
    return out


def sid_apply(dst, mode, sid_codes, n_q):
    """fac_sid_apply on the three code buffers dst (B, n_q[r], k) int64: per row mode (B) int32 on the device = kind | phase << 8
    | sid_k << 16 -- 0 PASS, 1 STORE (sid_codes[b, q, :k] = dst), 2 FILL (dst[b, q, f] = sid_codes[b, q, (phase + f) % sid_k]).
    sid_codes (B, Q, 16) int64 is the device state.  One launch, nothing read back."""
    n_q = tuple(int(n) for n in n_q)
    B = mode.shape[0]
    k = next(c for c, n in zip(dst, n_q) if n).shape[-1]
    d = _lib.SidApplyDesc()
    _plc_codes(d, "dst", dst, n_q, B, k, "sid_apply destination")
    for r in range(3):
        d.n_q[r] = n_q[r]
    if not mode.is_cuda or mode.dtype != torch.int32 or mode.dim() != 1 or not mode.is_contiguous():
        raise ValueError(f"sid_apply: mode must be dense int32 ({B},) on the GPU, got {mode.dtype} {tuple(mode.shape)}")
    if not sid_codes.is_cuda or sid_codes.dtype != torch.int64 or tuple(sid_codes.shape) != (B, sum(n_q), _lib.PLC_MAX_FRAMES) \
            or not sid_codes.is_contiguous():
        raise ValueError(f"sid_apply: sid_codes must be contiguous int64 ({B}, {sum(n_q)}, {_lib.PLC_MAX_FRAMES}) on the GPU")
    d.B, d.k, d.mode, d.sid_codes = B, k, mode.data_ptr(), sid_codes.data_ptr()
    _lib.check(_lib.load().fac_sid_apply(C.byref(d), _stream()), "fac_sid_apply")


def codes_row_bytes(T, Q, bits=10):
    """Bytes of one row of pack_codes' buffer: 4 * ceil(ceil(T Q bits / 8) / 4) (fac_codes_row_bytes)."""
    return int(_lib.load().fac_codes_row_bytes(int(T), int(Q), int(bits)))


def _codes_desc(d, codes, what, B=None, T=None):
    """Fills codes / codes_bs / codes_qs / n_q of a pack or unpack descriptor from three (B, n, T) int64 device tensors (any batch /
    row stride, unit frame stride; None or n == 0 for an RVQ without quantizers) -> (B, T, Q)."""
    if len(codes) != 3:
        raise ValueError(f"{what}: codes is [prosody, content, residual], got {len(codes)} entries")
    Q = 0
    for r, c in enumerate(codes):
        if c is None:
            continue
        if not isinstance(c, torch.Tensor) or not c.is_cuda:
            raise _lib.FacodecHipError(f"{what}: codes must live on the GPU (got {getattr(c, 'device', type(c))}); there is no CPU path")
        if c.dtype != torch.int64 or c.dim() != 3:
            raise _lib.FacodecHipError(f"{what}: codes must be int64 (B, n, T), got {c.dtype} {tuple(c.shape)}")
        if B is None:
            B, T = c.shape[0], c.shape[2]
        if c.shape[0] != B or c.shape[2] != T:
            raise ValueError(f"{what}: RVQ {r} is {tuple(c.shape)} but the others have B = {B}, T = {T}")
        n = c.shape[1]
        if n == 0:
            continue
        if T > 1 and c.stride(2) != 1:
            raise ValueError(f"{what}: codes need unit stride along time (RVQ {r} has {c.stride(2)})")
        d.codes[r], d.codes_bs[r], d.codes_qs[r], d.n_q[r] = c.data_ptr(), c.stride(0), c.stride(1), n
        Q += n
    if B is None:
        raise ValueError(f"{what}: no codes")
    if not 1 <= Q <= _lib.VQ_DECODE_MAX_Q:
        raise ValueError(f"{what}: {Q} quantizers in all (1..{_lib.VQ_DECODE_MAX_Q})")
    return B, T, Q


def _check_bits(bits, what):
    if not isinstance(bits, int) or not 1 <= bits <= 16:
        raise ValueError(f"{what}: bits = {bits!r} is outside 1..16")


def pack_codes(codes, bits=10, lens=None, out=None):
    """[codes_p, codes_c, codes_r] int64 (B, n, T) -> uint8 (B, row_bytes), the packed payload rows of DESIGN.md 24 (fac_codes_pack:
    one store-only launch).  lens: (B,) int32 FRAMES on the device; row b then holds its min(lens[b], T) frames and zeros behind.
    out: an optional uint8 (B, >= row_bytes) buffer with a row stride that is a multiple of 4; only [0, row_bytes) of each row is
    written and the (B, row_bytes) view of it is returned."""
    _check_bits(bits, "pack_codes")
    d = _lib.CodesPackDesc()
    B, T, Q = _codes_desc(d, codes, "pack_codes")
    if B < 1 or T < 1:
        raise ValueError(f"pack_codes: empty codes (B = {B}, T = {T})")
    rb = codes_row_bytes(T, Q, bits)
    dev = next(c for c in codes if c is not None).device
    if out is None:
        out = torch.empty(B, rb, device=dev, dtype=torch.uint8)
    else:
        if not out.is_cuda:
            raise _lib.FacodecHipError(f"pack_codes: out must live on the GPU (got {out.device}); there is no CPU path")
        if out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != B or out.shape[1] < rb or (B > 1 and out.stride(0) % 4) \
                or (out.shape[1] > 1 and out.stride(1) != 1):
            raise ValueError(f"pack_codes: out must be uint8 ({B}, >= {rb}) with a row stride that is a multiple of 4, got {out.dtype} "
                             f"{tuple(out.shape)} strides {tuple(out.stride())}")
    d.lens = _lens(lens, B).data_ptr() if lens is not None else None
    d.out, d.out_bs = out.data_ptr(), (out.stride(0) if B > 1 else rb)
    d.B, d.T, d.bits = B, T, bits
    _lib.check(_lib.load().fac_codes_pack(C.byref(d), _stream()), "fac_codes_pack")
    return out[:, :rb]


def unpack_codes(packed, n_q, T, bits=10, lens=None, out=None):
    """uint8 (B, >= ceil(T Q bits / 8)) packed rows (any row stride and alignment) -> [codes_p, codes_c, codes_r] int64 (B, n_q[r], T)
    (fac_codes_unpack: one launch); an RVQ with n_q[r] == 0 comes back as (B, 0, T).  lens: (B,) int32 frames on the device;
    frames t >= lens[b] come back as code 0.  out: optional three int64 (B, n_q[r], T) tensors to write (strided views allowed)."""
    _check_bits(bits, "unpack_codes")
    if not isinstance(packed, torch.Tensor) or not packed.is_cuda:
        raise _lib.FacodecHipError(f"unpack_codes: packed must live on the GPU (got {getattr(packed, 'device', type(packed))}); there is no CPU path")
    if packed.dtype != torch.uint8 or packed.dim() != 2:
        raise _lib.FacodecHipError(f"unpack_codes: packed must be uint8 (B, bytes), got {packed.dtype} {tuple(packed.shape)}")
    n_q = tuple(int(n) for n in n_q)
    T = int(T)
    if len(n_q) != 3 or min(n_q) < 0 or not 1 <= sum(n_q) <= _lib.VQ_DECODE_MAX_Q:
        raise ValueError(f"unpack_codes: n_q = {n_q} is not three counts with 1..{_lib.VQ_DECODE_MAX_Q} quantizers in all")
    B, Q = packed.shape[0], sum(n_q)
    if B < 1 or T < 1:
        raise ValueError(f"unpack_codes: empty input (B = {B}, T = {T})")
    need = (T * Q * bits + 7) // 8
    if packed.shape[1] < need:
        raise ValueError(f"unpack_codes: packed rows of {packed.shape[1]} bytes are too short for T = {T}, Q = {Q}, bits = {bits} ({need} bytes)")
    if packed.shape[1] > 1 and packed.stride(1) != 1:
        packed = packed.contiguous()
    if out is None:
        out = [torch.empty(B, n, T, device=packed.device, dtype=torch.int64) for n in n_q]
    d = _lib.CodesUnpackDesc()
    _codes_desc(d, out, "unpack_codes", B, T)
    if tuple(d.n_q) != n_q:
        raise ValueError(f"unpack_codes: out has {tuple(d.n_q)} rows, n_q = {n_q}")
    d.in_, d.in_bs = packed.data_ptr(), (packed.stride(0) if B > 1 else packed.shape[1])
    d.lens = _lens(lens, B).data_ptr() if lens is not None else None
    d.B, d.T, d.bits = B, T, bits
    _lib.check(_lib.load().fac_codes_unpack(C.byref(d), _stream()), "fac_codes_unpack")
    return list(out)


def vq_loss_tiles(T):
    """Row length of `vq_step`'s loss_part buffer (one partial sum per time tile of the kernel)."""
    return int(_lib.load().fac_vq_loss_tiles(int(T)))


def vq_search(latents, codebook):
    """latents (N, 8) -> int64 (N,) nearest normalised code (dac/nn/quantize.py:78-94)."""
    latents = _dev(latents, "latents")
    codebook = _dev(codebook, "codebook")
    n = latents.shape[0]
    idx = torch.empty(n, device=latents.device, dtype=torch.int64)
    _lib.check(_lib.load().fac_vq_search(_ptr(latents), _ptr(codebook), _ptr(idx), n, codebook.shape[0], _stream()),
               "fac_vq_search")
    return idx


# --------------------------------------------------------------------------------- small fused ops
def gate_tanh_sigmoid(a, g=None):
    """g: optional (B, 2C) conditioning rows (may be a strided slice of a wider (B, n) tensor)."""
    a = _dev(a)
    B, c2, T = a.shape
    out = torch.empty(B, c2 // 2, T, device=a.device, dtype=torch.float32)
    g_bs = g.stride(0) if g is not None else 0
    _lib.check(_lib.load().fac_gate_tanh_sigmoid(_ptr(a), _ptr(g), g_bs, _ptr(out), B, c2 // 2, T, _stream()),
               "fac_gate_tanh_sigmoid")
    return out


def embed_sum(codes, tables, code_row0=0, out=None, accumulate=None):
    """out (B, E, T) (+)= sum_i tables[i][codes[:, code_row0 + i]]; tables (n, V, E), codes (B, N, T) int64.
    A given `out` is added to unless accumulate=False (a static buffer that the launch overwrites)."""
    B, n_codes, T = codes.shape
    n_tab, V, E = tables.shape
    acc = out is not None if accumulate is None else bool(accumulate) and out is not None
    if out is None:
        out = torch.empty(B, E, T, device=codes.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_embed_sum(_ptr(codes.contiguous()), _ptr(_dev(tables)), _ptr(out), B, n_tab, n_codes,
                                         code_row0, V, E, T, 1 if acc else 0, _stream()), "fac_embed_sum")
    return out


def embed_sum_bwd(dx, codes, n_tab, V, code_row0=0):
    """Adjoint of embed_sum (fac_embed_sum_bwd): dx (B, E, T), codes (B, N, T) int64 -> (n_tab, V, E), the gradient of table i
    summed over the frames whose code row code_row0 + i selects each entry.  Deterministic (fixed order, no atomics)."""
    dx = _dev(dx, "dx")
    B, E, T = dx.shape
    if codes.dtype != torch.int64 or not codes.is_cuda or codes.shape[0] != B or codes.shape[2] != T:
        raise _lib.FacodecHipError(f"embed_sum_bwd: codes must be (B, N, T) int64 on the GPU, got {tuple(codes.shape)} {codes.dtype}")
    codes = codes.contiguous()
    out = torch.empty(n_tab, V, E, device=dx.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_embed_sum_bwd(_ptr(dx), _ptr(codes), _ptr(out), B, n_tab, codes.shape[1], code_row0, V, E, T, _stream()),
               "fac_embed_sum_bwd")
    return out


def gate_bwd_cond(a, g, d, dcond):
    """Backward of gate_tanh_sigmoid(a, g) with conditioning (fac_gate_bwd_cond): -> da (B, 2C, T); writes
    dcond[b, :2C] = sum_t da[b, :, t] into `dcond` ((B, >= 2C) rows, may be a strided slice of a wider tensor)."""
    a, d = _dev(a, "a"), _dev(d, "d")
    B, c2, T = a.shape
    assert g.stride(1) == 1 and dcond.stride(1) == 1 and dcond.shape == (B, c2), (g.stride(), dcond.shape)
    da = torch.empty_like(a)
    _lib.check(_lib.load().fac_gate_bwd_cond(_ptr(a), _ptr(g), g.stride(0), _ptr(d), _ptr(da), _ptr(dcond), dcond.stride(0), B, c2 // 2, T,
                                             _stream()), "fac_gate_bwd_cond")
    return da


def glu_residual(a, res):
    a, res = _dev(a), _dev(res)
    B, c2, T = a.shape
    out = torch.empty(B, c2 // 2, T, device=a.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_glu_residual(_ptr(a), _ptr(res), _ptr(out), B, c2 // 2, T, _stream()), "fac_glu_residual")
    return out


def add(a, b, out=None):
    a, b = _dev(a), _dev(b)
    if out is None:
        out = torch.empty_like(a)
    _lib.check(_lib.load().fac_add(_ptr(a), _ptr(b), _ptr(out), a.numel(), _stream()), "fac_add")
    return out


def sub2(a, b, c, out=None):
    a, b, c = _dev(a), _dev(b), _dev(c)
    if out is None:
        out = torch.empty_like(a)
    _lib.check(_lib.load().fac_sub2(_ptr(a), _ptr(b), _ptr(c), _ptr(out), a.numel(), _stream()), "fac_sub2")
    return out


def mul_mask_(x, mask):
    """x (B,C,T) *= mask (B,T) in place."""
    B, c, T = x.shape
    _lib.check(_lib.load().fac_mul_mask(_ptr(x), _ptr(mask), B, c, T, _stream()), "fac_mul_mask")
    return x


def wn_res_skip_(rs, x, out, last):
    B, c, T = out.shape
    _lib.check(_lib.load().fac_wn_res_skip(_ptr(rs), _ptr(x), _ptr(out), B, c, T, 1 if last else 0, _stream()),
               "fac_wn_res_skip")


def attention_route(dk, T):
    """The kernel fac_attention launches for (dk, T), from the shapes alone (the C entry decides with this same function): "lds"
    (16 queries x T scores in LDS, csrc/misc.hip) while (16 dk + 16 T) * 4 bytes fit 160 KiB, "stream" (running max and sum over
    key tiles, csrc/attention_stream.hip: any T) past that."""
    return ("lds", "stream")[_lib.load().fac_attention_route(int(dk), int(T))]


def attention_stream_tiles():
    """(queries per workgroup, keys per LDS tile) of the "stream" attention kernel."""
    lib = _lib.load()
    return lib.fac_attention_stream_tile(0), lib.fac_attention_stream_tile(1)


def attention_form(dk, T):
    """The form of fac_attention's launch for (dk, T): on the "lds" route "tiled" (csrc/attention_tiled.hip: dk <= 256 and
    T <= 992) or "serial" (attention_kernel of csrc/misc.hip, the same bits); "stream" on the other route."""
    return ("tiled", "serial", "stream")[_lib.load().fac_attention_form(int(dk), int(T))]


def attention(q, k, v, mask, n_heads, kernel=None):
    """kernel: None (attention_route decides), or "lds" / "stream" to force a route (tests, A/B runs; "lds" past its LDS limit is
    an error), or "serial" to force the LDS route's one-thread-per-output kernel where attention_form would say "tiled"."""
    if kernel not in (None, "lds", "stream", "serial"):
        raise ValueError(f"attention: kernel={kernel!r} (None, 'lds', 'stream' or 'serial')")
    q, k, v = _dev(q), _dev(k), _dev(v)
    B, c, T = q.shape
    dk = c // n_heads
    out = torch.empty_like(q)
    if kernel in ("lds", "serial") and attention_route(dk, T) != "lds":
        raise _lib.FacodecHipError(f"attention: T={T} too long for the LDS score tile at dk={dk}")
    name = {"stream": "fac_attention_stream", "serial": "fac_attention_serial"}.get(kernel, "fac_attention")
    _lib.check(getattr(_lib.load(), name)(_ptr(q), _ptr(k), _ptr(v), _ptr(mask), _ptr(out), B, n_heads, dk, T, _stream()), name)
    return out


def masked_mean(x, mask):
    x = _dev(x)
    B, c, T = x.shape
    out = torch.empty(B, c, device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_masked_mean(_ptr(x), _ptr(mask), _ptr(out), B, c, T, _stream()), "fac_masked_mean")
    return out


def layernorm_c_affine(x, style):
    x, style = _dev(x), _dev(style)
    B, c, T = x.shape
    out = torch.empty_like(x)
    _lib.check(_lib.load().fac_layernorm_c_affine(_ptr(x), _ptr(style), _ptr(out), B, c, T, _stream()),
               "fac_layernorm_c_affine")
    return out


# --------------------------------------------------------------------------------- STFT pieces
def stft_frames(wave, n_win, n_frames, hop, pad, n_off):
    wave = _dev(wave, "wave")
    B, T = wave.shape
    frames = torch.empty(B, n_win, n_frames, device=wave.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_stft_frames(_ptr(wave), _ptr(frames), B, T, n_win, n_frames, hop, pad, n_off, _stream()),
               "fac_stft_frames")
    return frames


# --------------------------------------------------------------------------------- batches of clips with different lengths
def _lens(lens, B):
    """lens (B,) int32 on the device (every row's length in samples); never copied to the host."""
    if not isinstance(lens, torch.Tensor) or not lens.is_cuda:
        raise _lib.FacodecHipError(f"lens must live on the GPU (got {getattr(lens, 'device', type(lens))}); there is no CPU path")
    if lens.dtype != torch.int32 or tuple(lens.shape) != (B,):
        raise _lib.FacodecHipError(f"lens must be int32 ({B},), got {lens.dtype} {tuple(lens.shape)}")
    return lens if lens.is_contiguous() else lens.contiguous()


def stft_frames_ragged(wave, lens, n_win, n_frames, hop, pad, n_off):
    """stft_frames on a right-padded batch: row b is framed as wave[b, :lens[b]] (its own end reflection, lens[b] // hop
    frames, bit-equal to stft_frames of that slice), the frame columns behind are zeros."""
    wave = _dev(wave, "wave")
    B, T = wave.shape
    frames = torch.empty(B, n_win, n_frames, device=wave.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_stft_frames_ragged(_ptr(wave), _ptr(_lens(lens, B)), _ptr(frames), B, T, n_win, n_frames, hop, pad,
                                                  n_off, _stream()), "fac_stft_frames_ragged")
    return frames


def mask_tail_(x, lens, unit):
    """x (B, C, T) fp32 or int64, contiguous: x[b, :, t] = 0 for t >= lens[b] // unit, in place."""
    if not x.is_cuda:
        raise _lib.FacodecHipError(f"tensor must live on the GPU (got {x.device}); there is no CPU path")
    if x.dim() != 3 or not x.is_contiguous() or x.dtype not in (torch.float32, torch.int64):
        raise _lib.FacodecHipError(f"mask_tail_: a contiguous (B, C, T) float32 / int64 tensor, got {x.dtype} {tuple(x.shape)}")
    B, c, T = x.shape
    lib = _lib.load()
    fn, name = (lib.fac_mask_tail, "fac_mask_tail") if x.dtype == torch.float32 else (lib.fac_mask_tail_i64, "fac_mask_tail_i64")
    _lib.check(fn(_ptr(x), _ptr(_lens(lens, B)), B, c, T, unit, _stream()), name)
    return x


def edge_tail_(x, lens, mul, n, mode):
    """x (B, C, T) fp32, contiguous, of `mul` columns per frame; lens (B,) int32 in FRAMES.  Behind every clip's own end
    L_b = min(lens[b] * mul, T) the next min(n, T - L_b) columns become, in place, what a non-causal conv pads there when it
    sees the clip alone: PAD_REFLECT x[b, :, L_b + j] = x[b, :, L_b - 2 - j] (0 in front of the clip), PAD_ZERO zeros."""
    if not x.is_cuda:
        raise _lib.FacodecHipError(f"tensor must live on the GPU (got {x.device}); there is no CPU path")
    if x.dim() != 3 or not x.is_contiguous() or x.dtype != torch.float32:
        raise _lib.FacodecHipError(f"edge_tail_: a contiguous (B, C, T) float32 tensor, got {x.dtype} {tuple(x.shape)}")
    B, c, T = x.shape
    _lib.check(_lib.load().fac_edge_tail(_ptr(x), _ptr(_lens(lens, B)), B, c, T, mul, n, mode, _stream()), "fac_edge_tail")
    return x


def frame_mask(lens, n_frames, unit):
    """-> (mask (B, n_frames) float 0 / 1 with mask[b, f] = f < lens[b] // unit, frame_lens (B,) int32 = min(lens // unit, n_frames))."""
    B = lens.shape[0]
    lens = _lens(lens, B)
    mask = torch.empty(B, n_frames, device=lens.device, dtype=torch.float32)
    n_valid = torch.empty(B, device=lens.device, dtype=torch.int32)
    _lib.check(_lib.load().fac_frame_mask(_ptr(lens), _ptr(mask), _ptr(n_valid), B, n_frames, unit, _stream()), "fac_frame_mask")
    return mask, n_valid


# --------------------------------------------------------------------------------- sample-rate conversion
_RESAMPLE_DEV = {}


def resample_table(rate_in, rate_out, quality="best"):
    """The resampler's coefficients and geometry on the host (dsp.resample_table): dict(o, n, taps, offs (n,) int32 first-tap
    offsets, table (n, taps) float32 = table64 rounded once, half, W, rolloff, beta, base).  ValueError for an unknown quality,
    rates that are no positive integers, or a ratio with a side above 640."""
    from . import dsp
    return dsp.resample_table(rate_in, rate_out, quality)


def _resample_device_table(rate_in, rate_out, quality, device):
    """-> (geometry dict, table, offs) on `device`, uploaded once per (rate_in, rate_out, quality, device)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(rate_in), int(rate_out), quality, device)
    hit = _RESAMPLE_DEV.get(key)
    if hit is None:
        geo = resample_table(rate_in, rate_out, quality)
        hit = _RESAMPLE_DEV[key] = (geo, h2d(torch.from_numpy(geo["table"]), device), h2d(torch.from_numpy(geo["offs"]), device))
    return hit


def resample_desc(geo, table, offs, x, y, n_out, lens=None, hist=None, hist_out=None, q0=0, m_lo=0, T=None):
    """fac_resample_desc for x (B, T) -> y (B, >= n_out) rows (last dimension dense); hist / hist_out (B, n_hist) or None.
    T: how many columns of x are the block, where that is not all of them (T = 0: the end of a stream, any x)."""
    d = _lib.ResampleDesc()
    d.hist, d.x, d.lens, d.y, d.hist_out, d.table, d.offs = (t.data_ptr() if t is not None else None
                                                             for t in (hist, x, lens, y, hist_out, table, offs))
    d.hist_bs = hist.stride(0) if hist is not None else 0
    d.x_bs, d.y_bs, d.q0, d.m_lo = x.stride(0), y.stride(0), q0, m_lo
    d.B, d.n_hist, d.T, d.n_out = x.shape[0], hist.shape[1] if hist is not None else 0, x.shape[1] if T is None else T, n_out
    d.o, d.n, d.taps = geo["o"], geo["n"], geo["taps"]
    return d


def resample_form(d):
    """-> (form, outputs per tile, threads, LDS bytes, grid x) of the launch fac_resample makes for the descriptor (host only)."""
    out = (C.c_int32 * 4)()
    form = _lib.load().fac_resample_form(C.byref(d), out)
    if form < 0:
        _lib.check(-1, "fac_resample_form")
    return (form,) + tuple(out)


def resample(x, rate_in, rate_out, lens=None, quality="best"):
    """x (B, T) or (B, 1, T) fp32 at rate_in -> the same rank with ceil(T n / o) columns at rate_out (o, n = the rates over their
    gcd), one launch; the input itself when the rates are equal.  lens (B,) int32 on the device: row b is resampled as
    x[b, :lens[b]] -- what sits behind is never read as signal -- and the outputs from ceil(lens[b] n / o) on are zeros; row b
    is bit-equal to the call on that slice alone."""
    geo = resample_table(rate_in, rate_out, quality)                 # ValueError: quality, rates, ratio
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3) or (x.dim() == 3 and x.shape[1] != 1):
        raise ValueError(f"resample takes (B, T) or (B, 1, T), got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}")
    x = _dev(x, "x")
    if int(rate_in) == int(rate_out):
        return x
    B, T = x.shape[0], x.shape[-1]
    geo, table, offs = _resample_device_table(rate_in, rate_out, quality, x.device)
    n_out = -(-T * geo["n"] // geo["o"])
    y = torch.empty(x.shape[:-1] + (n_out,), device=x.device, dtype=torch.float32)
    if B == 0 or n_out == 0:
        return y
    d = resample_desc(geo, table, offs, x.view(B, T), y.view(B, n_out), n_out, lens=_lens(lens, B) if lens is not None else None)
    _lib.check(_lib.load().fac_resample(C.byref(d), _stream()), "fac_resample")
    return y


# --------------------------------------------------------------------------------- loudness
_KWEIGHT = {}
LoudnessEnergies = namedtuple("LoudnessEnergies", "e peak state")


def loudness_chunk():
    """Samples per chunk of fac_kweight_energy: a row is filtered in chunks of this length, whose states are handed across by a
    scan inside groups of loudness_chunk_group() chunks and a serial scan across those groups."""
    return _lib.load().fac_loudness_chunk(0)


def loudness_chunk_group():
    """Chunks per workgroup of fac_kweight_energy (the unit of its serial scan)."""
    return _lib.load().fac_loudness_chunk(1)


def _kweight_tables(rate):
    """-> (S, coef (10,), pw (7, 16)) float64 on the host, once per rate (dsp.k_weighting_transitions).  ValueError: the rate."""
    hit = _KWEIGHT.get(rate)
    if hit is None:
        from . import dsp
        coef, pw = dsp.k_weighting_transitions(rate, loudness_chunk())
        hit = _KWEIGHT[rate] = (int(rate) // 10, coef, pw)
    return hit


def _rows(x, what):
    """(B, T) or (B, 1, T) float32 on the device -> the (B, T) view with dense samples."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3) or (x.dim() == 3 and x.shape[1] != 1):
        raise ValueError(f"{what} takes (B, T) or (B, 1, T), got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}")
    if not x.is_cuda:                                               # checked in line: every push comes through here
        _on_gpu(x, f"{what}: x")
    if x.dtype != torch.float32:
        raise _lib.FacodecHipError(f"{what}: x must be float32 (got {x.dtype})")
    x2 = x.reshape(x.shape[0], x.shape[-1]) if x.dim() == 3 else x
    return x2 if x2.shape[-1] <= 1 or x2.stride(-1) == 1 else x2.contiguous()


def loudness_energies(x, rate=24000, lens=None, state=None, offset=0, out=None, peak=None, state_out=None, ws=None):
    """K-weighted energies per 100 ms sub-block (fac_kweight_energy): x (B, T) or (B, 1, T) float32 -> LoudnessEnergies(e (B, n_sub)
    float64, peak (B,) float32 = max |x|, state (B, 4) float64 or None), n_sub = ceil((offset + T) / S), S = rate / 10.  lens (B,)
    int32 on the device: row b is its first lens[b] samples, the energies behind are zeros.

    A stream continues with state= (B, 4) float64, the filter state the previous call returned (then `state` of the result is
    the state after this call; not with lens), and offset = samples so far modulo S; with offset > 0 the first sub-block is
    ADDED to out[:, 0].  out / peak / state_out / ws: preallocated buffers (out (B, >= n_sub) float64 with dense rows; peak
    accumulates by maximum when given; state_out may be `state`; ws uint8 of fac_kweight_ws_bytes) -- the call then allocates
    nothing."""
    S, coef, pw = _kweight_tables(rate)                             # ValueError: fs % 10
    x = _rows(x, "loudness_energies")
    B, T = x.shape
    if not 0 <= offset < S:
        raise ValueError(f"loudness_energies: offset = {offset} outside 0 .. {S - 1}")
    if lens is not None and (state is not None or state_out is not None or offset):
        raise ValueError("loudness_energies: a carried state or an offset (a stream) does not go with lens")
    n_sub = -(-(offset + T) // S)
    dev = x.device
    if out is None:
        if offset:
            raise ValueError("loudness_energies: offset > 0 adds to out[:, 0]; pass out=")
        out = torch.empty(B, n_sub, device=dev, dtype=torch.float64)
    else:
        _arg(out, "loudness_energies: out", torch.float64, (B, n_sub), at_least=True)
    acc = peak is not None
    if peak is None:
        peak = torch.empty(B, device=dev, dtype=torch.float32)
    if state is not None and state_out is None:
        state_out = torch.empty(B, 4, device=dev, dtype=torch.float64)
    _arg(state, "loudness_energies: state", torch.float64, (B, 4), optional=True)
    _arg(state_out, "loudness_energies: state_out", torch.float64, (B, 4), optional=True)
    if B == 0:
        return LoudnessEnergies(out[:, :n_sub], peak, state_out)
    lib = _lib.load()
    if T == 0:
        if not acc:
            peak.zero_()
        if state is not None and state_out is not state:
            state_out.copy_(state)
        return LoudnessEnergies(out[:, :n_sub], peak, state_out)
    need = lib.fac_kweight_ws_bytes(B, T)
    if need < 0:
        raise ValueError(f"loudness_energies: B = {B}, T = {T} (T up to 2^30 samples per call)")
    if ws is None:
        ws = torch.empty(need, device=dev, dtype=torch.uint8)
    elif ws.numel() < need or ws.dtype != torch.uint8 or ws.data_ptr() % 8:
        raise ValueError(f"loudness_energies: ws must be uint8, 8-byte aligned, of at least {need} bytes")
    d = _lib.KweightDesc()
    d.x, d.lens, d.e = x.data_ptr(), (_lens(lens, B).data_ptr() if lens is not None else None), out.data_ptr()
    d.state_in = state.data_ptr() if state is not None else None
    d.state_out = state_out.data_ptr() if state_out is not None else None
    d.peak, d.ws = peak.data_ptr(), ws.data_ptr()
    d.x_bs, d.e_bs = _row_pitch(x, B, T), _row_pitch(out, B, out.shape[1])
    d.B, d.T, d.S, d.offset, d.peak_accumulate = B, T, S, offset, 1 if acc else 0
    d.coef[:] = coef.tolist()
    for k in range(7):
        d.pw[k][:] = pw[k].tolist()
    _lib.check(lib.fac_kweight_energy(C.byref(d), _stream()), "fac_kweight_energy")
    return LoudnessEnergies(out[:, :n_sub], peak, state_out)


def loudness_gate(e, n_samples, rate=24000, lens=None, last_n=0, peaks=None):
    """fac_loudness_gate over energies e (B, >= ceil(n_samples / S)) float64: -> L (B,) float64, or (L, peak (B,) float32) with
    peaks (B, n) float32.  last_n = 0: the two-gate integrated loudness of BS.1770-4; last_n > 0: the last last_n sub-blocks,
    ungated (4: momentary, 30: short-term).  Never below -70."""
    S = _kweight_tables(rate)[0]
    B = e.shape[0]
    _on_gpu(e, "loudness_gate: e")
    if e.dtype != torch.float64 or e.dim() != 2 or (e.shape[1] > 1 and e.stride(1) != 1) or e.shape[1] < -(-int(n_samples) // S):
        raise ValueError(f"loudness_gate: e must be float64 (B, >= {-(-int(n_samples) // S)}) with dense rows, got {e.dtype} {tuple(e.shape)}")
    L = torch.empty(B, device=e.device, dtype=torch.float64)
    pk = None
    if peaks is not None:
        peaks = _dev(peaks.reshape(B, -1), "peaks")
        pk = torch.empty(B, device=e.device, dtype=torch.float32)
    if B == 0:
        return L if peaks is None else (L, pk)
    # a row without sub-blocks is never read; keep the pointer valid all the same
    e_ptr = e if e.numel() else torch.zeros(1, device=e.device, dtype=torch.float64)
    _lib.check(_lib.load().fac_loudness_gate(_ptr(e_ptr), _row_pitch(e, B, e.shape[1]), _ptr(_lens(lens, B) if lens is not None else None),
                                             int(n_samples), S, int(last_n), _ptr(peaks), peaks.shape[1] if peaks is not None else 0,
                                             _ptr(L), _ptr(pk), B, _stream()), "fac_loudness_gate")
    return L if peaks is None else (L, pk)


def loudness(x, rate=24000, lens=None):
    """Integrated loudness of ITU-R BS.1770-4 for mono signals: x (B, T) or (B, 1, T) float32 -> (B,) float64 on the device, in
    LUFS, -70.0 for silence, an empty clip or a clip no block of which passes the gates.  lens (B,) int32 on the device: row b is
    x[b, :lens[b]] and measures what that slice measures alone.  Two C calls (fac_kweight_energy, fac_loudness_gate), no host
    read.  ValueError for a rate that is no multiple of 10 (resample first)."""
    en = loudness_energies(x, rate, lens=lens)
    return loudness_gate(en.e, x.shape[-1], rate, lens=lens)


def loudness_gain(x, L, peak=None, target_db=-16.0, target_rows=None, lens=None, guard=True, out=None):
    """fac_loudness_gain: g from (L, target, peak) on the device, y = x * g on every row's samples and 0 behind lens -> (y, g (B,)
    float32).  target_rows (B,) float64 replaces target_db per row (NaN: leave the row alone); guard=False skips the peak
    guard; out may be x."""
    x2 = _rows(x, "loudness_gain")
    B, T = x2.shape
    y = torch.empty_like(x2) if out is None else _rows(out, "loudness_gain")
    g = torch.empty(B, device=x2.device, dtype=torch.float32)
    if B and T:
        _lib.check(_lib.load().fac_loudness_gain(_ptr(x2), _row_pitch(x2, B, T), _ptr(_lens(lens, B) if lens is not None else None),
                                                 _ptr(L), _ptr(peak), _ptr(target_rows), float(target_db), 1 if guard else 0,
                                                 _ptr(y), _row_pitch(y, B, T), _ptr(g), B, T, _stream()), "fac_loudness_gain")
    elif B:
        g.fill_(1.0)
    return y.view(x.shape) if out is None else out, g


def normalize_loudness(x, target_db=-16.0, rate=24000, lens=None):
    """Level x to target_db LUFS as the reference's compress does (normalize, then ensure_max_of_audio): -> (y, input_db (B,)
    float64, gain (B,) float32), all on the device and without a host read in between.  gain = 10^((target_db - input_db) / 20),
    1 for a silent row (input_db = -70), 1 / max|x| where the levelled row would exceed full scale; y = x * gain in fp32 on every
    row's own samples, zeros behind lens."""
    en = loudness_energies(x, rate, lens=lens)
    L = loudness_gate(en.e, x.shape[-1], rate, lens=lens)
    y, g = loudness_gain(x, L, en.peak, target_db=target_db, lens=lens)
    return y, L, g


# --------------------------------------------------------------------------------- level control
AgcParams = namedtuple("AgcParams", "S W target_db max_boost_db max_cut_db ceiling LA")
Levelled = namedtuple("Levelled", "y G g")


def agc_params(rate=24000, target_db=-23.0, window=30, max_boost_db=30.0, max_cut_db=30.0, ceiling_db=-1.0, lookahead=120):
    """-> AgcParams(S, W, target_db, max_boost_db, max_cut_db, ceiling, LA) of fac_agc_gains / fac_agc_apply: S = rate / 10, the
    window in sub-blocks of 100 ms, ceiling = 10 ** (ceiling_db / 20) (linear, a Python float: the kernel and a restatement of
    it take the same bits), the look-ahead in samples.  The defaults -- a 3 s window levelled to -23 LUFS, +-30 dB of gain, a
    sample-peak ceiling of -1 dBFS 5 ms ahead -- were not tuned by listening."""
    S = _kweight_tables(rate)[0]                                    # ValueError: the rate
    W, LA = int(window), int(lookahead)
    if not 4 <= W <= _lib.AGC_MAX_WINDOW:
        raise ValueError(f"agc: window = {W} outside 4 .. {_lib.AGC_MAX_WINDOW} sub-blocks")
    if not 1 <= LA <= _lib.AGC_MAX_LOOKAHEAD:
        raise ValueError(f"agc: lookahead = {LA} outside 1 .. {_lib.AGC_MAX_LOOKAHEAD} samples")
    target_db, max_boost_db, max_cut_db = float(target_db), float(max_boost_db), float(max_cut_db)
    if not (math.isfinite(target_db) and 0.0 <= max_boost_db < math.inf and 0.0 <= max_cut_db < math.inf):
        raise ValueError(f"agc: target_db = {target_db}, max_boost_db = {max_boost_db}, max_cut_db = {max_cut_db} (finite, limits not negative)")
    ceiling = 10.0 ** (float(ceiling_db) / 20.0)
    if not 0.0 < ceiling < math.inf:
        raise ValueError(f"agc: ceiling_db = {ceiling_db}")
    return AgcParams(S, W, target_db, max_boost_db, max_cut_db, ceiling, LA)


def agc_gains(e, p, j0=0, n_new=None, R=None, lens=None, j_start=None, G=None, g=None):
    """fac_agc_gains over the sub-block energies e (B, >= R) float64 (sub-block j at column j % R; a plain array is R = its
    width, j0 = 0) with p = agc_params(...): the gains of sub-blocks j0 .. j0 + n_new - 1 -> (G dB, g linear), float64 (B, R)
    written at columns j % R (allocated when not given).  lens (B,) int32: the rows' lengths in samples, sub-blocks that are
    not complete get G = 0, g = 1.  j_start (B,) int64: the first sub-block of every row's current stream."""
    B = _on_gpu(e, "agc_gains: e").shape[0]
    R = e.shape[1] if R is None else int(R)
    n_new = R - int(j0) if n_new is None else int(n_new)
    _arg(e, "agc_gains: e", torch.float64, (B, R), at_least=True)
    if G is None:
        G = torch.zeros(B, R, device=e.device, dtype=torch.float64)
    if g is None:
        g = torch.ones(B, R, device=e.device, dtype=torch.float64)
    _arg(G, "agc_gains: G", torch.float64, (B, R), at_least=True), _arg(g, "agc_gains: g", torch.float64, (B, R), at_least=True)
    if G.stride(0) != g.stride(0) and B > 1:
        raise ValueError("agc_gains: G and g must have the same row pitch")
    if B == 0 or n_new == 0:
        return G, g
    d = _lib.AgcGainsDesc()
    d.e, d.lens = e.data_ptr(), (_lens(lens, B).data_ptr() if lens is not None else None)
    d.j_start = _ptr(_arg(j_start, "agc_gains: j_start", torch.int64, (B,), optional=True))
    d.G, d.g = G.data_ptr(), g.data_ptr()
    d.e_bs, d.g_bs, d.j0 = _row_pitch(e, B, e.shape[1]), _row_pitch(g, B, g.shape[1]), int(j0)
    d.target_db, d.max_boost_db, d.max_cut_db = p.target_db, p.max_boost_db, p.max_cut_db
    d.B, d.n_new, d.R, d.W, d.S = B, n_new, R, p.W, p.S
    _lib.check(_lib.load().fac_agc_gains(C.byref(d), _stream()), "fac_agc_gains")
    return G, g


def agc_apply(x, g, p, n0=0, R=None, lens=None, j_start=None, carry_in=None, carry_out=None, flush=True, k=None, out=None):
    """fac_agc_apply: x (B, k) float32 gained by the ramp between the decided gains g (B, >= R) float64 (g_j at column j % R) and
    limited to p.ceiling with p.LA samples of look-ahead -> y (B, n_out) float32, n_out = k + LA with flush (the signal ends
    with this block) and k without; y runs LA samples behind x.  n0: the absolute index of x[:, 0].  carry_in / carry_out
    (B, 2 LA) float64, two different buffers of a stream; lens (B,) int32 only without them.  k = 0 with flush is the flush of
    a stream alone (x may be None).  out: a preallocated (B, >= n_out) float32 buffer with dense rows."""
    B = _on_gpu(g, "agc_apply: g").shape[0]
    if x is not None:
        x = _rows(x, "agc_apply")
    k = (x.shape[1] if x is not None else 0) if k is None else int(k)
    R = g.shape[1] if R is None else int(R)
    _arg(g, "agc_apply: g", torch.float64, (B, R), at_least=True)
    n_out = k + p.LA if flush else k
    if out is None:
        out = torch.empty(B, n_out, device=g.device, dtype=torch.float32)
    else:
        _arg(out, "agc_apply: out", torch.float32, (B, n_out), at_least=True)
    if B == 0 or n_out == 0:
        return out[:, :n_out]
    d = _lib.AgcApplyDesc()
    d.carry_in = _ptr(_arg(carry_in, "agc_apply: carry_in", torch.float64, (B, 2 * p.LA), optional=True))
    d.carry_out = _ptr(_arg(carry_out, "agc_apply: carry_out", torch.float64, (B, 2 * p.LA), optional=True))
    d.x = x.data_ptr() if x is not None and k > 0 else None
    d.lens = _lens(lens, B).data_ptr() if lens is not None else None
    d.j_start = _ptr(_arg(j_start, "agc_apply: j_start", torch.int64, (B,), optional=True))
    d.g, d.y = g.data_ptr(), out.data_ptr()
    d.x_bs = _row_pitch(x, B, max(k, 1))
    d.g_bs, d.y_bs, d.n0 = _row_pitch(g, B, g.shape[1]), _row_pitch(out, B, out.shape[1]), int(n0)
    d.ceiling = p.ceiling
    d.B, d.k, d.n_out, d.S, d.LA, d.R = B, k, n_out, p.S, p.LA, R
    _lib.check(_lib.load().fac_agc_apply(C.byref(d), _stream()), "fac_agc_apply")
    return out[:, :n_out]


def level(x, rate=24000, lens=None, target_db=-23.0, window=30, max_boost_db=30.0, max_cut_db=30.0, ceiling_db=-1.0, lookahead=120):
    """Causal level control of x (B, T) or (B, 1, T) float32 on the GPU -> Levelled(y (B, T + lookahead) or
    (B, 1, T + lookahead) float32, G (B, n) float64 dB, g (B, n) float64 linear), n = T // S completed sub-blocks of S = rate / 10
    samples: what streaming.AutoGain gives for the same signal.  Sub-block j's gain G[:, j] is the clamped distance from
    target_db of the two-gate BS.1770 loudness of the last `window` sub-blocks up to j; sample n in sub-block j is multiplied by
    the ramp from g[j - 2] to g[j - 1] (only completed sub-blocks: causal, continuous), then a peak limiter with `lookahead`
    samples keeps every sample at or under 10 ** (ceiling_db / 20); y is the levelled signal `lookahead` samples late, so row b
    holds lens[b] + lookahead samples and zeros behind.  Three C calls (fac_kweight_energy, fac_agc_gains, fac_agc_apply), no
    host read; the arithmetic is pinned in include/facodec_hip.h.  The defaults were not tuned by listening."""
    p = agc_params(rate, target_db, window, max_boost_db, max_cut_db, ceiling_db, lookahead)
    x2 = _rows(x, "level")
    B, T = x2.shape
    n = T // p.S
    dev = x2.device
    if B == 0 or T == 0:
        y = torch.zeros(B, T + p.LA, device=dev, dtype=torch.float32)
        G, g = torch.zeros(B, n, device=dev, dtype=torch.float64), torch.ones(B, n, device=dev, dtype=torch.float64)
    else:
        en = loudness_energies(x2, rate, lens=lens)
        G = torch.zeros(B, max(n, 1), device=dev, dtype=torch.float64)
        g = torch.ones(B, max(n, 1), device=dev, dtype=torch.float64)
        if n:
            agc_gains(en.e, p, 0, n, R=n, lens=lens, G=G, g=g)
        y = agc_apply(x2, g, p, lens=lens, flush=True)
        G, g = G[:, :n], g[:, :n]
    return Levelled(y.view(x.shape[:-1] + (T + p.LA,)), G, g)


def true_peak(x, rate=24000, lens=None, quality="best"):
    """True peak of x (B, T) or (B, 1, T) float32 on the GPU -> (B,) float32: max |y| of the signal oversampled 4 x with the
    project's polyphase filter (dsp.resample_table(rate, 4 rate, quality)), computed without writing the oversampled signal
    (fac_true_peak: fac_resample's arithmetic and order): equal to resample(x, rate, 4 * rate, lens, quality).abs().amax(-1) bit
    for bit.  lens (B,) int32 on the device: row b is x[b, :lens[b]].  A meter: the limiter's ceiling is a sample-peak ceiling."""
    resample_table(rate, 4 * int(rate), quality)                    # ValueError: quality, rate
    x2 = _rows(x, "true_peak")
    B, T = x2.shape
    peak = torch.zeros(B, device=x2.device, dtype=torch.float32)
    if B == 0 or T == 0:
        return peak
    geo, table, offs = _resample_device_table(rate, 4 * int(rate), quality, x2.device)
    n_out = -(-T * geo["n"] // geo["o"])
    ws = torch.empty(_lib.load().fac_true_peak_ws_bytes(B, n_out) // 4, device=x2.device, dtype=torch.float32)
    d = resample_desc(geo, table, offs, x2, x2, n_out, lens=_lens(lens, B) if lens is not None else None)
    d.y, d.y_bs = None, 0
    _lib.check(_lib.load().fac_true_peak(C.byref(d), _ptr(peak), _ptr(ws), _stream()), "fac_true_peak")
    return peak


# --------------------------------------------------------------------------------- noise suppression
NsParams = namedtuple("NsParams", "M W over g_min")
Denoised = namedtuple("Denoised", "y G")
NS_N, NS_H, NS_BINS, NS_CARRY, NS_DELAY = _lib.NS_N, _lib.NS_H, _lib.NS_BINS, _lib.NS_CARRY, 2 * _lib.NS_H


def ns_params(M=8, W=96, over=4.0, max_atten_db=15.0):
    """-> NsParams(M, W, over, g_min) of fac_ns_gains: the power spectra are averaged over M frames, the noise floor is the
    minimum of that average over W frames (frames of 512 samples at a hop of 256), a bin passes in proportion to what its
    average holds above `over` times the floor, and never falls below g_min = 10 ** (-max_atten_db / 20) (a Python float: the
    kernel and a restatement of it take the same bits).  The defaults -- 8 frames, 96 frames (1.02 s at 24 kHz), 4.0, 15 dB --
    were not tuned by listening."""
    if int(M) != M or not 1 <= int(M) <= _lib.NS_MAX_M:
        raise ValueError(f"denoise: M = {M} outside 1 .. {_lib.NS_MAX_M} frames")
    if int(W) != W or not 1 <= int(W) <= _lib.NS_MAX_W:
        raise ValueError(f"denoise: W = {W} outside 1 .. {_lib.NS_MAX_W} frames")
    over, max_atten_db = float(over), float(max_atten_db)
    if not 0.0 < over < math.inf:
        raise ValueError(f"denoise: over = {over} (finite, above 0)")
    if not 0.0 <= max_atten_db < math.inf:
        raise ValueError(f"denoise: max_atten_db = {max_atten_db} (finite, not negative)")
    g_min = 10.0 ** (-max_atten_db / 20.0)
    if not g_min > 0.0:
        raise ValueError(f"denoise: max_atten_db = {max_atten_db} leaves no gain floor above 0")
    return NsParams(int(M), int(W), over, g_min)


def ns_frames(n):
    """Frames of a signal of n samples: ceil(n / 256) + 1, 0 for an empty one."""
    return -(-int(n) // NS_H) + 1 if n > 0 else 0


def _ns_ring(t, B, R, what, dtype=torch.float64, last=()):
    shape = (B, R, NS_BINS) + last
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or t.dim() != len(shape) or t.shape[0] != B or t.shape[1] < R \
            or tuple(t.shape[2:]) != shape[2:] or not t[0].is_contiguous():
        raise ValueError(f"{what} must be {dtype} {shape} on the GPU with dense rows, got {getattr(t, 'dtype', type(t))} "
                         f"{tuple(getattr(t, 'shape', ()))}")
    return t


def _ns_pitch(t, B):
    """Row pitch of a (B, R, 257[, 2]) ring in elements of 8 (or, for spectra, 16) bytes."""
    per = 2 if t.dim() == 4 else 1
    return (t.stride(0) if B > 1 else t.shape[1] * NS_BINS * per) // per


def ns_power(x, P, n0=0, f0=0, n_new=None, R=None, lens=None, starts=None, carry_in=None, carry_out=None, X=None, k=None):
    """fac_ns_power: the power spectra of frames f0 .. f0 + n_new - 1 of [carry | x] (x (B, k) float32, sample i at the absolute
    index n0 + i) into the ring P (B, >= R, 257) float64, frame f at slot f % R; X (B, >= R, 257, 2) float64 also takes the
    spectra.  n_new defaults to the frames of an offline signal of k samples.  carry_in / carry_out (B, 1023) float32: two
    different buffers of a stream; lens (B,) int32 only without them; starts (B,) int64: the rows' first samples."""
    B = _on_gpu(P, "ns_power: P").shape[0]
    if x is not None:
        x = _rows(x, "ns_power")
    k = (x.shape[1] if x is not None else 0) if k is None else int(k)
    R = P.shape[1] if R is None else int(R)
    n_new = ns_frames(k) if n_new is None else int(n_new)
    P = _ns_ring(P, B, R, "ns_power: P")
    if X is not None:
        X = _ns_ring(X, B, R, "ns_power: X", last=(2,))
        if B > 1 and _ns_pitch(X, B) != _ns_pitch(P, B):
            raise ValueError("ns_power: X and P must have the same row pitch")
    if B == 0 or (n_new == 0 and carry_out is None):
        return P
    d = _lib.NsPowerDesc()
    d.carry_in = _ptr(_arg(carry_in, "ns_power: carry_in", torch.float32, (B, NS_CARRY), optional=True))
    d.carry_out = _ptr(_arg(carry_out, "ns_power: carry_out", torch.float32, (B, NS_CARRY), optional=True))
    d.x = x.data_ptr() if x is not None and k > 0 else None
    d.lens = _lens(lens, B).data_ptr() if lens is not None else None
    d.starts = _ptr(_arg(starts, "ns_power: starts", torch.int64, (B,), optional=True))
    d.P, d.X = P.data_ptr(), _ptr(X)
    d.x_bs = _row_pitch(x, B, max(k, 1))
    d.p_bs, d.n0, d.f0 = _ns_pitch(P, B), int(n0), int(f0)
    d.B, d.k, d.n_new, d.R = B, k, n_new, R
    _lib.check(_lib.load().fac_ns_power(C.byref(d), _stream()), "fac_ns_power")
    return P


def ns_gains(P, p, f0=0, n_new=None, R=None, starts=None, G=None):
    """fac_ns_gains over the ring P (B, >= R, 257) float64 with p = ns_params(...): the gains of frames f0 .. f0 + n_new - 1 -> G
    (B, R, 257) float64, frame f at slot f % R (allocated when not given)."""
    B = _on_gpu(P, "ns_gains: P").shape[0]
    R = P.shape[1] if R is None else int(R)
    n_new = R - int(f0) if n_new is None else int(n_new)
    P = _ns_ring(P, B, R, "ns_gains: P")
    if G is None:
        G = torch.ones(B, R, NS_BINS, device=P.device, dtype=torch.float64)
    G = _ns_ring(G, B, R, "ns_gains: G")
    if B == 0 or n_new == 0:
        return G
    d = _lib.NsGainsDesc()
    d.P, d.G, d.starts = P.data_ptr(), G.data_ptr(), _ptr(_arg(starts, "ns_gains: starts", torch.int64, (B,), optional=True))
    d.p_bs, d.g_bs, d.f0 = _ns_pitch(P, B), _ns_pitch(G, B), int(f0)
    d.over, d.g_min = p.over, p.g_min
    d.B, d.n_new, d.R, d.M, d.W = B, n_new, R, p.M, p.W
    _lib.check(_lib.load().fac_ns_gains(C.byref(d), _stream()), "fac_ns_gains")
    return G


def ns_synth(x, G, n0=0, m0=0, n_out=None, R=None, lens=None, starts=None, carry_in=None, X=None, k=None, out=None):
    """fac_ns_synth: y[m0 .. m0 + n_out) (B, n_out) float32 of [carry | x] masked with the gains G (B, >= R, 257) float64 (frame
    f at slot f % R): both frames over every output segment are transformed (or, with X, read from that ring), masked,
    transformed back, windowed and added.  n_out defaults to k (with n0 = m0 = 0: the offline call)."""
    B = _on_gpu(G, "ns_synth: G").shape[0]
    if x is not None:
        x = _rows(x, "ns_synth")
    k = (x.shape[1] if x is not None else 0) if k is None else int(k)
    R = G.shape[1] if R is None else int(R)
    n_out = k if n_out is None else int(n_out)
    G = _ns_ring(G, B, R, "ns_synth: G")
    if X is not None:
        X = _ns_ring(X, B, R, "ns_synth: X", last=(2,))
        if B > 1 and _ns_pitch(X, B) != _ns_pitch(G, B):
            raise ValueError("ns_synth: X and G must have the same row pitch")
    if out is None:
        out = torch.empty(B, n_out, device=G.device, dtype=torch.float32)
    else:
        _arg(out, "ns_synth: out", torch.float32, (B, n_out), at_least=True)
    if B == 0 or n_out == 0:
        return out[:, :n_out]
    d = _lib.NsSynthDesc()
    d.carry_in = _ptr(_arg(carry_in, "ns_synth: carry_in", torch.float32, (B, NS_CARRY), optional=True))
    d.x = x.data_ptr() if x is not None and k > 0 else None
    d.lens = _lens(lens, B).data_ptr() if lens is not None else None
    d.starts = _ptr(_arg(starts, "ns_synth: starts", torch.int64, (B,), optional=True))
    d.G, d.X, d.y = G.data_ptr(), _ptr(X), out.data_ptr()
    d.x_bs = _row_pitch(x, B, max(k, 1))
    d.g_bs, d.y_bs, d.n0, d.m0 = _ns_pitch(G, B), _row_pitch(out, B, out.shape[1]), int(n0), int(m0)
    d.B, d.k, d.n_out, d.R = B, k, n_out, R
    _lib.check(_lib.load().fac_ns_synth(C.byref(d), _stream()), "fac_ns_synth")
    return out[:, :n_out]


def denoise(x, lens=None, starts=None, M=8, W=96, over=4.0, max_atten_db=15.0, keep_spectra=False):
    """Spectral noise suppression of x (B, T) or (B, 1, T) float32 on the GPU -> Denoised(y, G): y of x's shape,
    float32, aligned with x; G (B, F, 257) float64, F = ceil(T / 256) + 1, the gain of every frame (512 samples, sine window,
    hop 256) and bin.  A bin's gain is xi / (1 + xi), xi = S / (over * Nf) - 1 clipped at 0, S the mean power of the last M
    frames, Nf the minimum of S over the last W frames, never below -max_atten_db; 1 while the window holds digital silence.
    lens (B,) int32: row b is x[b, :lens[b]], what lies behind it is not read and comes out 0.  starts (B,) int32: row b's
    stream begins at sample starts[b]; earlier samples count as zero, frames below starts[b] // 256 are in no window, outputs
    before starts[b] are 0.  Three C calls (fac_ns_power, fac_ns_gains, fac_ns_synth), no host read; what streaming.
    NoiseSuppressor gives for the same signal, 512 samples earlier.  keep_spectra: synthesis reads the spectra fac_ns_power
    wrote (16 bytes per frame and bin of scratch) where it otherwise transforms every frame again; the same bits.  A stream
    that starts in speech has that speech for its floor until the window has seen a pause.  The arithmetic is pinned in
    include/facodec_hip.h; the defaults were not tuned by listening."""
    p = ns_params(M, W, over, max_atten_db)
    x2 = _rows(x, "denoise")
    B, T = x2.shape
    F = ns_frames(T)
    dev = x2.device
    G = torch.ones(B, F, NS_BINS, device=dev, dtype=torch.float64)
    if B == 0 or T == 0:
        return Denoised(torch.zeros_like(x), G)
    if starts is not None:
        if not isinstance(starts, torch.Tensor) or not starts.is_cuda or tuple(starts.shape) != (B,) or starts.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"denoise: starts must be int32 ({B},) on the GPU")
        starts = starts.to(torch.int64).contiguous()
    P = torch.empty(B, F, NS_BINS, device=dev, dtype=torch.float64)
    X = torch.empty(B, F, NS_BINS, 2, device=dev, dtype=torch.float64) if keep_spectra else None
    ns_power(x2, P, lens=lens, starts=starts, X=X)
    ns_gains(P, p, 0, F, starts=starts, G=G)
    y = ns_synth(x2, G, lens=lens, starts=starts, X=X)
    return Denoised(y.view(x.shape), G)


# --------------------------------------------------------------------------------- echo cancellation
AecParams = namedtuple("AecParams", "P mu beta delta delay c")
EchoCancelled = namedtuple("EchoCancelled", "e W stats")
AEC_H, AEC_BINS, AEC_DELAY = _lib.AEC_H, _lib.AEC_BINS, _lib.AEC_H


def aec_params(P=8, mu=0.5, beta=1.0, delta=1e-6, delay=0):
    """-> AecParams(P, mu, beta, delta, delay, c) of fac_aec_run: P partitions of 256 taps; the step is mu over the far-end
    power in the filter's span plus c = beta * P times the error power plus delta (c a Python float: the kernel and a
    restatement of it take the same bits); the far end is used `delay` samples late.  The error term is what keeps the filter
    from diverging under double talk.  The defaults -- 8, 0.5, 1.0, 1e-6, 0 -- were not tuned by listening."""
    if int(P) != P or not 1 <= int(P) <= _lib.AEC_MAX_P:
        raise ValueError(f"echo_cancel: P = {P} outside 1 .. {_lib.AEC_MAX_P} partitions")
    mu, beta, delta = float(mu), float(beta), float(delta)
    if not 0.0 <= mu <= 1.0:
        raise ValueError(f"echo_cancel: mu = {mu} outside [0, 1]")
    if not 0.0 <= beta < math.inf:
        raise ValueError(f"echo_cancel: beta = {beta} (finite, not negative)")
    if not 0.0 <= delta < math.inf:
        raise ValueError(f"echo_cancel: delta = {delta} (finite, not negative)")
    if int(delay) != delay or not 0 <= int(delay) <= _lib.AEC_MAX_DELAY:
        raise ValueError(f"echo_cancel: delay = {delay} outside 0 .. {_lib.AEC_MAX_DELAY} samples")
    return AecParams(int(P), mu, beta, delta, int(delay), beta * int(P))


def aec_blocks(n):
    """Blocks of a signal of n samples: ceil(n / 256)."""
    return -(-int(n) // AEC_H)


def aec_state_sizes(P, delay=0):
    """fac_aec_state_sizes: per-row (doubles of W, doubles of the X ring, floats of the mic carry, of the far carry, of the e ring)."""
    sizes = (C.c_int64 * 5)()
    _lib.check(_lib.load().fac_aec_state_sizes(int(P), int(delay), sizes), "fac_aec_state_sizes")
    return tuple(int(v) for v in sizes)


def aec_run(mic, far, p, W, X, n0=0, m0=0, n_out=None, blk0=0, n_blk=None, lens=None, starts=None, adapt=None, mic_carry=(None, None),
            far_carry=(None, None), e_ring=None, stats=None, k=None):
    """fac_aec_run with p = aec_params(...): the blocks blk0 .. blk0 + n_blk - 1 of [carry | mic], [carry | far] (both (B, k)
    float32, sample i at the absolute index n0 + i) on the state W, X (B, P, 257, 2) float64, updated in place -> e[m0 .. m0 +
    n_out) (B, n_out) float32.  mic_carry / far_carry: (in, out) pairs of two different buffers (B, 255) / (B, 511 + delay);
    e_ring (B, 256) float32; stats (B, n_blk, 3) float64; adapt (B,) int32; lens (B,) int32 only offline; starts (B,) int64."""
    B = _on_gpu(W, "aec_run: W").shape[0]
    if mic is not None:
        mic, far = _rows(mic, "aec_run"), _rows(far, "aec_run")
        if mic.shape != far.shape:
            raise ValueError(f"aec_run: mic {tuple(mic.shape)} and far {tuple(far.shape)} differ")
    k = (mic.shape[1] if mic is not None else 0) if k is None else int(k)
    n_out = k if n_out is None else int(n_out)
    n_blk = aec_blocks(k) if n_blk is None else int(n_blk)
    _arg(W, "aec_run: W", torch.float64, (B, p.P, AEC_BINS, 2)), _arg(X, "aec_run: X", torch.float64, (B, p.P, AEC_BINS, 2))
    far_cn = _lib.AEC_FAR_CARRY + p.delay
    y = torch.empty(B, n_out, device=W.device, dtype=torch.float32)
    if B == 0 or n_out == 0:
        return y
    _arg(stats, "aec_run: stats", torch.float64, (B, n_blk, 3), optional=True)
    _arg(adapt, "aec_run: adapt", torch.int32, (B,), optional=True)
    d = _lib.AecDesc()
    d.mic_carry_in, d.mic_carry_out = (_ptr(_arg(t, "aec_run: mic carry", torch.float32, (B, _lib.AEC_MIC_CARRY), optional=True)) for t in mic_carry)
    d.far_carry_in, d.far_carry_out = (_ptr(_arg(t, "aec_run: far carry", torch.float32, (B, far_cn), optional=True)) for t in far_carry)
    d.mic = mic.data_ptr() if mic is not None and k > 0 else None
    d.far = far.data_ptr() if far is not None and k > 0 else None
    d.lens = _lens(lens, B).data_ptr() if lens is not None else None
    d.starts = _ptr(_arg(starts, "aec_run: starts", torch.int64, (B,), optional=True))
    d.adapt = _ptr(adapt)
    d.W, d.X, d.e_ring, d.y, d.stats = W.data_ptr(), X.data_ptr(), _ptr(_arg(e_ring, "aec_run: e_ring", torch.float32, (B, AEC_H), optional=True)), y.data_ptr(), _ptr(stats)
    d.mic_bs, d.far_bs = _row_pitch(mic, B, max(k, 1)), _row_pitch(far, B, max(k, 1))
    d.y_bs, d.w_bs, d.xr_bs, d.s_bs = n_out, p.P * AEC_BINS * 2, p.P * AEC_BINS * 2, 3 * n_blk
    d.n0, d.m0, d.blk0 = int(n0), int(m0), int(blk0)
    d.mu, d.c, d.delta = p.mu, p.c, p.delta
    d.B, d.k, d.n_out, d.n_blk, d.P, d.delay, d.far_cn = B, k, n_out, n_blk, p.P, p.delay, far_cn
    _lib.check(_lib.load().fac_aec_run(C.byref(d), _stream()), "fac_aec_run")
    return y


def _aec_adapt(adapt, B, device):
    """None, a bool, or B of them -> None or (B,) int32 on the device."""
    if adapt is None:
        return None
    if isinstance(adapt, torch.Tensor):
        if tuple(adapt.shape) != (B,):
            raise ValueError(f"echo_cancel: adapt must be ({B},), got {tuple(adapt.shape)}")
        return h2d(adapt, device).to(torch.int32).contiguous()
    flags = [bool(adapt)] * B if isinstance(adapt, (bool, int)) else [bool(a) for a in adapt]
    if len(flags) != B:
        raise ValueError(f"echo_cancel: adapt has {len(flags)} entries for {B} rows")
    return h2d(torch.tensor(flags, dtype=torch.int32), device)


def echo_cancel(mic, far, lens=None, starts=None, P=8, mu=0.5, beta=1.0, delta=1e-6, delay=0, adapt=None, **delay_params):
    """Acoustic echo cancellation of mic against the far-end reference far, both (B, T) or (B, 1, T) float32 on the GPU
     -> EchoCancelled(e, W, stats): e of mic's shape, float32, aligned with it: the microphone less the estimate
    of the echo; W (B, P, 257, 2) float64, the filter after the row's last block (partition p holds taps 256 p .. 256 p + 255
    as the first half of a 512-point spectrum); stats (B, M, 3) float64, M = ceil(T / 256): per block the sums of mic^2, of the
    estimate^2 and of e^2.  A partitioned-block frequency-domain adaptive filter on blocks of 256 samples with P partitions
    (P * 256 taps: 85 ms at 24 kHz for P = 8), overlap-save, a fully constrained gradient, the step mu / (far-end power in
    the span + beta * P * error power + delta) per bin; the far end is used `delay` samples late, so the filter's span begins
    there.  adapt: None, a bool or one per row; a row that does not adapt only filters.  lens (B,) int32: row b is its first
    lens[b] samples, nothing behind them is read and e comes out 0 there.  starts (B,) int: row b's stream begins at sample
    starts[b]; earlier samples of both signals count as zero, the filter starts from zero at block starts[b] // 256, outputs
    before starts[b] are 0.  One C call (fac_aec_run), one workgroup per row that walks the blocks in order, no host read;
    what streaming.EchoCanceller gives for the same signals, 256 samples earlier.  delay="auto" (with **delay_params,
    echo_delay_params') finds the delay on the device: it is echo_cancel(mic, echo_delay(mic, far, ...).far, delay=0, ...)
    (DESIGN.md 36).  There is no residual-echo suppressor and no double-talk detector beyond the error term of the step.  The
    arithmetic is pinned in include/facodec_hip.h; the defaults were not tuned by listening."""
    if isinstance(delay, str):
        if delay != "auto":
            raise ValueError(f"echo_cancel: delay = {delay!r} (an integer or \"auto\")")
        aec_params(P, mu, beta, delta, 0), echo_delay_params(**delay_params)       # every refusal before the first launch
        far, delay = echo_delay(mic, far, lens=lens, starts=starts, **delay_params).far, 0
    elif delay_params:
        raise TypeError(f"echo_cancel: {sorted(delay_params)} go with delay=\"auto\" only")
    p = aec_params(P, mu, beta, delta, delay)
    m2, f2 = _rows(mic, "echo_cancel"), _rows(far, "echo_cancel")
    if m2.shape != f2.shape:
        raise ValueError(f"echo_cancel: mic {tuple(m2.shape)} and far {tuple(f2.shape)} differ")
    B, T = m2.shape
    dev = m2.device
    M = aec_blocks(T)
    W = torch.zeros(B, p.P, AEC_BINS, 2, device=dev, dtype=torch.float64)
    stats = torch.zeros(B, M, 3, device=dev, dtype=torch.float64)
    if B == 0 or T == 0:
        return EchoCancelled(torch.zeros_like(mic), W, stats)
    if starts is not None:
        if not isinstance(starts, torch.Tensor) or tuple(starts.shape) != (B,) or starts.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"echo_cancel: starts must be an int32 or int64 tensor ({B},)")
        if not starts.is_cuda and bool((starts < 0).any()):
            raise ValueError("echo_cancel: starts must not be negative")
        starts = h2d(starts, dev).to(torch.int64).contiguous()
    X = torch.zeros(B, p.P, AEC_BINS, 2, device=dev, dtype=torch.float64)
    e = aec_run(m2, f2, p, W, X, lens=lens, starts=starts, adapt=_aec_adapt(adapt, B, dev), stats=stats)
    return EchoCancelled(e.view(mic.shape), W, stats)


# --------------------------------------------------------------------------------- echo delay
EchoDelayParams = namedtuple("EchoDelayParams", "max_delay k_lo k_hi a eps gate thr hold tol move margin delay0 L")
EchoDelay = namedtuple("EchoDelay", "far raw locked used conf ok score")
ECHO_DELAY_NAMES = EchoDelayParams._fields[:-1]


def echo_delay_params(max_delay=16384, k_lo=6, k_hi=134, a=0.05, eps=1e-20, gate=1e-8, thr=0.1, hold=8, tol=128, move=256, margin=128, delay0=0):
    """-> EchoDelayParams(max_delay, k_lo, k_hi, a, eps, gate, thr, hold, tol, move, margin, delay0, L) of fac_edelay_run: lags 0 ..
    L = ceil(max_delay / 256) of 256 samples; the bins k_lo .. k_hi - 1 of a 512-point transform (about 0.28 to 6.2 kHz at
    24 kHz); a the smoothing of the cross-spectra, eps what keeps their normalisation finite; gate the mean square above which a
    frame is active; a raw delay counts when the best lag's score reaches thr; hold agreeing frames (within tol samples) latch
    it, a later run re-latches only move samples or more away; the far end is moved by the latched delay less margin samples,
    by delay0 before the first latch.  None of the defaults was tuned by listening."""
    for name, v in (("max_delay", max_delay), ("k_lo", k_lo), ("k_hi", k_hi), ("hold", hold), ("tol", tol), ("move", move), ("margin", margin),
                    ("delay0", delay0)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"echo_delay: {name} = {v} is not an integer")
    max_delay, k_lo, k_hi, hold, tol, move, margin, delay0 = (int(v) for v in (max_delay, k_lo, k_hi, hold, tol, move, margin, delay0))
    a, eps, gate, thr = float(a), float(eps), float(gate), float(thr)
    if not 1 <= max_delay <= _lib.EDELAY_MAX_DELAY:
        raise ValueError(f"echo_delay: max_delay = {max_delay} outside 1 .. {_lib.EDELAY_MAX_DELAY} samples")
    if not (0 <= k_lo < k_hi <= AEC_BINS and k_hi - k_lo <= AEC_H):
        raise ValueError(f"echo_delay: band k_lo = {k_lo}, k_hi = {k_hi} (0 <= k_lo < k_hi <= 257, at most 256 bins)")
    if not 0.0 < a <= 1.0:
        raise ValueError(f"echo_delay: a = {a} outside (0, 1]")
    if not 0.0 < eps < math.inf:
        raise ValueError(f"echo_delay: eps = {eps} (finite, positive)")
    if not 0.0 <= gate < math.inf:
        raise ValueError(f"echo_delay: gate = {gate} (finite, not negative)")
    if not 0.0 <= thr < math.inf:
        raise ValueError(f"echo_delay: thr = {thr} (finite, not negative)")
    if hold < 1:
        raise ValueError(f"echo_delay: hold = {hold} below 1 frame")
    if tol < 0 or move < 0 or margin < 0:
        raise ValueError(f"echo_delay: tol = {tol}, move = {move}, margin = {margin} (not negative)")
    if not 0 <= delay0 <= max_delay:
        raise ValueError(f"echo_delay: delay0 = {delay0} outside 0 .. max_delay = {max_delay}")
    return EchoDelayParams(max_delay, k_lo, k_hi, a, eps, gate, thr, hold, tol, move, margin, delay0, -(-max_delay // AEC_H))


def echo_delay_frames(n):
    """Frames of a signal of n samples: frame m >= 1 covers the blocks m - 1 and m, so max(n // 256 - 1, 0)."""
    return max(int(n) // AEC_H - 1, 0)


def edelay_state_sizes(max_delay=16384):
    """fac_edelay_state_sizes: per-row (doubles of C, doubles of the X ring, ints of the activity ring, ints of the policy, floats
    of the mic ring, floats of the far ring)."""
    sizes = (C.c_int64 * 6)()
    _lib.check(_lib.load().fac_edelay_state_sizes(int(max_delay), sizes), "fac_edelay_state_sizes")
    return tuple(int(v) for v in sizes)


def edelay_state(B, p, device, rings=False):
    """A fresh state of fac_edelay_run for B rows: dict(C, X, act, pol, conf_last[, mic_ring, far_ring]) on `device`."""
    n_c, n_x, n_act, n_pol, n_mic, n_far = edelay_state_sizes(p.max_delay)
    L1 = p.L + 1
    assert n_c == n_x == L1 * AEC_BINS * 2 and n_act == L1
    st = dict(C=torch.zeros(B, L1, AEC_BINS, 2, device=device, dtype=torch.float64), X=torch.zeros(B, L1, AEC_BINS, 2, device=device, dtype=torch.float64),
              act=torch.zeros(B, n_act, device=device, dtype=torch.int32),
              pol=torch.tensor([-1, 0, -1, p.delay0], dtype=torch.int32).repeat(B, 1).to(device),
              conf_last=torch.zeros(B, device=device, dtype=torch.float64))
    if rings:
        st["mic_ring"] = torch.zeros(B, n_mic, device=device, dtype=torch.float32)
        st["far_ring"] = torch.zeros(B, n_far, device=device, dtype=torch.float32)
    return st


def edelay_run(mic, far, p, state, n0=0, frm0=1, n_frm=None, lens=None, starts=None, frames=None, f_ring=0):
    """fac_edelay_run with p = echo_delay_params(...): the frames frm0 .. frm0 + n_frm - 1 of [ring | mic], [ring | far] (both
    (B, k) float32, sample i at the absolute index n0 + i) on `state` (edelay_state: updated in place) -> the aligned far end
    (B, k) float32.  frames: None, or a dict of per-frame output buffers raw, locked, used (int32), conf (float64), ok (uint8),
    all (B, f_n), and score (B, f_n, L + 1) float64, any of them missing; f_n = n_frm, or f_ring > 0 columns used as a ring.
    lens (B,) int32 only without rings; starts (B,) int64."""
    mic, far = _rows(mic, "edelay_run"), _rows(far, "edelay_run")
    if mic.shape != far.shape:
        raise ValueError(f"edelay_run: mic {tuple(mic.shape)} and far {tuple(far.shape)} differ")
    B, k = mic.shape
    L1 = p.L + 1
    n_frm = echo_delay_frames(k) if n_frm is None else int(n_frm)
    y = torch.empty(B, k, device=mic.device, dtype=torch.float32)
    if B == 0 or k == 0:
        return y
    f_n = int(f_ring) if f_ring else n_frm
    frames = frames or {}
    d = _lib.EdelayDesc()
    d.mic, d.far, d.y = mic.data_ptr(), far.data_ptr(), y.data_ptr()
    d.lens = _lens(lens, B).data_ptr() if lens is not None else None
    d.starts = _ptr(_arg(starts, "edelay_run: starts", torch.int64, (B,), optional=True))
    d.C = _arg(state["C"], "edelay_run: C", torch.float64, (B, L1, AEC_BINS, 2)).data_ptr()
    d.X = _arg(state["X"], "edelay_run: X", torch.float64, (B, L1, AEC_BINS, 2)).data_ptr()
    d.act = _arg(state["act"], "edelay_run: act", torch.int32, (B, L1)).data_ptr()
    d.pol = _arg(state["pol"], "edelay_run: pol", torch.int32, (B, _lib.EDELAY_POL)).data_ptr()
    d.conf_last = _arg(state["conf_last"], "edelay_run: conf_last", torch.float64, (B,)).data_ptr()
    far_rn = L1 * AEC_H + AEC_H - 1
    d.mic_ring = _ptr(_arg(state.get("mic_ring"), "edelay_run: mic_ring", torch.float32, (B, _lib.EDELAY_MIC_RING), optional=True))
    d.far_ring = _ptr(_arg(state.get("far_ring"), "edelay_run: far_ring", torch.float32, (B, far_rn), optional=True))
    for name, dtype in (("raw", torch.int32), ("locked", torch.int32), ("used", torch.int32), ("conf", torch.float64), ("ok", torch.uint8)):
        setattr(d, name, _ptr(_arg(frames.get(name), f"edelay_run: {name}", dtype, (B, f_n), optional=True)))
    d.score = _ptr(_arg(frames.get("score"), "edelay_run: score", torch.float64, (B, f_n, L1), optional=True))
    d.mic_bs, d.far_bs, d.y_bs = _row_pitch(mic, B, k), _row_pitch(far, B, k), k
    d.c_bs = d.xr_bs = L1 * AEC_BINS * 2
    d.f_bs, d.n0, d.frm0 = f_n, int(n0), int(frm0)
    d.a, d.eps, d.gate, d.thr = p.a, p.eps, p.gate, p.thr
    d.B, d.k, d.n_frm, d.f_ring, d.max_delay, d.far_rn = B, k, n_frm, int(f_ring), p.max_delay, far_rn
    d.k_lo, d.k_hi, d.hold, d.tol, d.move, d.margin, d.delay0 = p.k_lo, p.k_hi, p.hold, p.tol, p.move, p.margin, p.delay0
    _lib.check(_lib.load().fac_edelay_run(C.byref(d), _stream()), "fac_edelay_run")
    return y


def _starts(starts, B, dev, what):
    if starts is None:
        return None
    if not isinstance(starts, torch.Tensor) or tuple(starts.shape) != (B,) or starts.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: starts must be an int32 or int64 tensor ({B},)")
    if not starts.is_cuda and bool((starts < 0).any()):
        raise ValueError(f"{what}: starts must not be negative")
    return h2d(starts, dev).to(torch.int64).contiguous()


def echo_delay(mic, far, lens=None, starts=None, state=None, **params):
    """The playout-to-capture delay of every row, frame by frame, and the far end moved by it: mic and far (B, T)
    or (B, 1, T) float32 on the GPU -> EchoDelay(far, raw, locked, used, conf, ok, score).  far, of far's shape: the aligned far
    end, far[n - used] with the `used` of the frame that ended before the sample's block of 256 -- no latency; what
    ops.echo_cancel(mic, ., delay=0) wants.  Per frame m = 1 .. M = max(T // 256 - 1, 0), at column m - 1: raw (B, M) int32, the
    delay the frame saw; locked int32, the latched delay, -1 before the first latch; used int32, what the aligner takes from the
    next block on; conf float64, the best lag's score; ok uint8, whether raw counted; score (B, M, L + 1) float64.  A column
    that is no frame of its row (behind lens[b] // 256 - 1 frames, before the frame starts[b] // 256 + 1) holds raw = locked =
    used = -1 and conf = ok = score = 0.  lens, starts: as ops.echo_cancel's.  state: an ops.edelay_state to use and leave
    updated (tests read C from it).  One C call, one workgroup per row, no host read.  **params: echo_delay_params'."""
    p = echo_delay_params(**params)
    m2, f2 = _rows(mic, "echo_delay"), _rows(far, "echo_delay")
    if m2.shape != f2.shape:
        raise ValueError(f"echo_delay: mic {tuple(m2.shape)} and far {tuple(f2.shape)} differ")
    B, T = m2.shape
    dev, M, L1 = m2.device, echo_delay_frames(T), p.L + 1
    fr = dict(raw=torch.full((B, M), -1, device=dev, dtype=torch.int32), locked=torch.full((B, M), -1, device=dev, dtype=torch.int32),
              used=torch.full((B, M), -1, device=dev, dtype=torch.int32), conf=torch.zeros(B, M, device=dev, dtype=torch.float64),
              ok=torch.zeros(B, M, device=dev, dtype=torch.uint8), score=torch.zeros(B, M, L1, device=dev, dtype=torch.float64))
    if B == 0 or T == 0:
        return EchoDelay(torch.zeros_like(far), *fr.values())
    starts = _starts(starts, B, dev, "echo_delay")
    state = edelay_state(B, p, dev) if state is None else state
    y = edelay_run(m2, f2, p, state, lens=lens, starts=starts, frames=fr if M else None)
    return EchoDelay(y.view(far.shape), fr["raw"], fr["locked"], fr["used"], fr["conf"], fr["ok"], fr["score"])


# --------------------------------------------------------------------------------- objective scores
STOI_RATE = 10000
StoiGeometry = namedtuple("StoiGeometry", "n_frames ws_bytes_per_row energy_frames scan_block band_frames score_segments")
StoiScores = namedtuple("StoiScores", "stoi estoi n_frames n_kept n_segments kept_idx")


def si_sdr_chunk():
    """Samples per chunk (one workgroup's partial sums) of fac_si_sdr."""
    return _lib.SI_SDR_CHUNK


def stoi_geometry(T):
    """fac_stoi_geometry for rows of T samples at 10 kHz (host only): frames per row, workspace bytes per row, and the tile
    constants of the launches -- frames per workgroup of the energy pass, frames per block of the keep scan, frames per
    workgroup of fac_stoi_bands, segments per workgroup of fac_stoi_score."""
    out = (C.c_int64 * 6)()
    _lib.check(_lib.load().fac_stoi_geometry(int(T), out), "fac_stoi_geometry")
    return StoiGeometry(*(int(v) for v in out))


def _score_pair(ref, est, lens, what):
    """-> the (B, T) views of ref and est with dense samples and lens checked (or None)."""
    if isinstance(ref, torch.Tensor) and isinstance(est, torch.Tensor) and ref.shape != est.shape:
        raise ValueError(f"{what}: reference and estimate must have the same shape, got {tuple(ref.shape)} and {tuple(est.shape)}")
    x, y = _rows(ref, what), _rows(est, what)
    return x, y, (_lens(lens, x.shape[0]) if lens is not None else None)


def si_sdr(ref, est, lens=None):
    """Scale-invariant signal-to-distortion ratio in dB, higher is better (dac/nn/loss.py:91-130 with scaling and zero_mean, sign
    flipped): ref, est (B, T) or (B, 1, T) float32 -> (B,) float64 on the device, evaluated in fp64 in three passes
    (fac_si_sdr; include/facodec_hip.h states the formula).  lens (B,) int32 on the device: row b is its first lens[b] samples.
    Identical rows give +inf, an empty or all-zero pair NaN, a zero reference with a non-zero estimate -80."""
    x, y, lens = _score_pair(ref, est, lens, "si_sdr")
    B, T = x.shape
    out = torch.full((B,), float("nan"), device=x.device, dtype=torch.float64)
    if B == 0 or T == 0:
        return out
    lib = _lib.load()
    need = lib.fac_si_sdr_ws_bytes(B, T)
    if need < 0:
        raise ValueError(f"si_sdr: B = {B}, T = {T} (T up to 2^30 samples per call)")
    ws = torch.empty(need, device=x.device, dtype=torch.uint8)
    _lib.check(lib.fac_si_sdr(_ptr(x), x.stride(0) if B > 1 else T, _ptr(y), y.stride(0) if B > 1 else T, _ptr(lens), _ptr(out), _ptr(ws),
                              need, B, T, _stream()), "fac_si_sdr")
    return out


def _stoi_setup(x, y, lens):
    """Results, descriptor and workspace of the three STOI launches for dense rows x, y (B, T) at 10 kHz -> (StoiScores,
    fac_stoi_desc or None when there is nothing to launch, ws).  The results hold NaN / 0 until the launches have run."""
    B, T = x.shape
    dev = x.device
    geo = stoi_geometry(T)
    stoi, estoi = (torch.full((B,), float("nan"), device=dev, dtype=torch.float64) for _ in range(2))
    n_frames, n_kept, n_seg = (torch.zeros(B, device=dev, dtype=torch.int32) for _ in range(3))
    kept = torch.empty(B, geo.n_frames, device=dev, dtype=torch.int32)
    res = StoiScores(stoi, estoi, n_frames, n_kept, n_seg, kept)
    if B == 0 or T == 0:
        return res, None, None
    ws = torch.empty(max(8, B * geo.ws_bytes_per_row), device=dev, dtype=torch.uint8)
    d = _lib.StoiDesc()
    d.x, d.y, d.lens = x.data_ptr(), y.data_ptr(), (lens.data_ptr() if lens is not None else None)
    d.kept_idx = kept.data_ptr() if kept.numel() else ws.data_ptr()          # M_max = 0: nothing is written there
    d.n_frames, d.n_kept, d.n_segments = n_frames.data_ptr(), n_kept.data_ptr(), n_seg.data_ptr()
    d.stoi, d.estoi, d.ws = stoi.data_ptr(), estoi.data_ptr(), ws.data_ptr()
    d.x_bs, d.y_bs, d.ws_bytes = (x.stride(0) if B > 1 else T), (y.stride(0) if B > 1 else T), ws.numel()
    d.B, d.T = B, T
    return res, d, ws


def stoi_scores(ref, est, rate=24000, lens=None):
    """STOI and ESTOI of est against ref, both from one pass: ref, est (B, T) or (B, 1, T) float32 at `rate` -> StoiScores(stoi,
    estoi (B,) float64; n_frames, n_kept, n_segments (B,) int32; kept_idx (B, M_max) int32, the first n_kept[b] entries of row b
    the kept frames in order and -1 behind them), all on the device.  lens (B,) int32 on the device: row b is its first lens[b] samples.  A rate
    other than 10000 goes through ops.resample(., rate, 10000, lens=lens, quality="best") first, with lengths ceil(lens n / o).
    Rows with fewer than 30 kept frames (under 0.4 s) have no segment: NaN and n_segments = 0.  Three C calls
    (fac_stoi_select, fac_stoi_bands, fac_stoi_score) on one descriptor, no host read in between."""
    x, y, lens = _score_pair(ref, est, lens, "stoi_scores")
    if int(rate) != STOI_RATE:
        geo = resample_table(rate, STOI_RATE, "best")
        x, y = resample(x, rate, STOI_RATE, lens=lens), resample(y, rate, STOI_RATE, lens=lens)
        if lens is not None:
            lens = ((lens.to(torch.int64) * geo["n"] + (geo["o"] - 1)) // geo["o"]).to(torch.int32)
    res, d, _ = _stoi_setup(x, y, lens)
    if d is not None:
        lib = _lib.load()
        _lib.check(lib.fac_stoi_select(C.byref(d), _stream()), "fac_stoi_select")
        _lib.check(lib.fac_stoi_bands(C.byref(d), _stream()), "fac_stoi_bands")
        _lib.check(lib.fac_stoi_score(C.byref(d), _stream()), "fac_stoi_score")
    return res


def stoi(ref, est, rate=24000, lens=None, extended=False):
    """Short-time objective intelligibility (Taal et al. 2011), or with extended=True ESTOI (Jensen & Taal 2016): -> (B,) float64
    on the device; see stoi_scores, which gives both from the same pass."""
    s = stoi_scores(ref, est, rate, lens)
    return s.estoi if extended else s.stoi


def spec_power(spec, power):
    B, f2, nf = spec.shape
    out = torch.empty(B, f2 // 2, nf, device=spec.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_spec_power(_ptr(spec), _ptr(out), B, f2 // 2, nf, power, _stream()), "fac_spec_power")
    return out


def reduce_pair(a, b, out, scratch, mode, eps=0.0, scale=1.0, accumulate=False):
    a, b = _dev(a), _dev(b)
    _lib.check(_lib.load().fac_reduce_pair(_ptr(a), _ptr(b), _ptr(out), _ptr(scratch), a.numel(), mode, eps, scale,
                                           1 if accumulate else 0, _stream()), "fac_reduce_pair")
    return out


def logdiff_rms(a, b, out, scratch, eps, scale=1.0, accumulate=False):
    """losses.py:84 term on (B, M, T) tensors, accumulated into out[0]."""
    a, b = _dev(a), _dev(b)
    B, M, T = a.shape
    _lib.check(_lib.load().fac_logdiff_rms(_ptr(a), _ptr(b), _ptr(out), _ptr(scratch), B, M, T, eps, scale,
                                           1 if accumulate else 0, _stream()), "fac_logdiff_rms")
    return out


def logdiff_rms_bwd(a, b, db, eps, scale=1.0, accumulate=False):
    """db (+)= scale * d/db sum_{b,t} sqrt(mean_m (log(|a|+eps) - log(|b|+eps))^2); a, b, db (B, M, T)."""
    a, b = _dev(a), _dev(b)
    B, M, T = a.shape
    _lib.check(_lib.load().fac_logdiff_rms_bwd(_ptr(a), _ptr(b), _ptr(db), B, M, T, eps, scale, 1 if accumulate else 0, _stream()),
               "fac_logdiff_rms_bwd")


def aa_snakebeta(x, alpha_log, beta_log, filter12):
    """Anti-aliased SnakeBeta (Activation1d(SnakeBeta(alpha_logscale=True)))."""
    x = _dev(x)
    B, c, T = x.shape
    y = torch.empty_like(x)
    _lib.check(_lib.load().fac_aa_snakebeta_fwd(_ptr(x), _ptr(alpha_log), _ptr(beta_log), _ptr(filter12), _ptr(y), B, c, T,
                                                _stream()), "fac_aa_snakebeta_fwd")
    return y


# --------------------------------------------------------------------------------- backward of the conv stack
@prepared
def flipped_weight(v, g=None, scale=None, out=None):
    """(C_out, C_in, K) [weight-normed] -> (C_in, C_out, K) weights of the data-gradient conv (channels swapped, taps flipped),
    one launch (fac_flip_transpose_w)."""
    v = _dev(v, "weight")
    c_out, c_in, k = v.shape
    if scale is None and g is not None:
        scale = wn_scale(v, g)
    if out is None:
        out = torch.empty(c_in, c_out, k, device=v.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_flip_transpose_w(_ptr(v), _ptr(scale), _ptr(out), c_out, c_in, k, _stream()), "fac_flip_transpose_w")
    return out


@prepared
def pack_conv_weight_bwd(v, g=None, scale=None, out=None):
    """(C_out, C_in, K) [weight-normed] -> packed weights of the bwd-data conv (taps flipped, channels swapped)."""
    v = _dev(v, "weight")
    c_out, c_in, k = v.shape
    packed = out if out is not None else torch.empty(cin_pad(c_out), k, pad32(c_in), device=v.device, dtype=torch.float32)
    if scale is None and g is not None:
        scale = wn_scale(v, g)
    _lib.check(_lib.load().fac_pack_conv_w_bwd(_ptr(v), _ptr(scale), _ptr(packed), c_out, c_in, k, pad32(c_in), _stream()),
               "fac_pack_conv_w_bwd")
    return packed


def plan_bwd_data(c_out, c_in, k, stride, dilation, B, t_in, causal=True):
    """What conv1d_bwd_data launches for the SConv1d c_in -> c_out over B clips of t_in columns, from shapes alone:
    (plan, t_out, pad_left, pad_right, tp) with tp = pad_left + t_in + pad_right the columns of the padded gradient.
    Stride 1: the forward plan of the conv with the channels swapped (a ConvPlan).  Strided (k = 2 s): the transposed conv over
    dy and its zero column (a ConvTrPlan); its p8 is None off the flattened form, whose per-clip launch takes no pre-pass."""
    t_out, padding_total, extra = conv_out_len(t_in, k, stride, dilation)
    pad_left = padding_total if causal else padding_total - padding_total // 2
    pad_right = (padding_total - pad_left) + extra
    tp = pad_left + t_in + pad_right
    if stride == 1:
        return plan_conv(c_in, c_out, k, 1, dilation, B, t_out, tp), t_out, pad_left, pad_right, tp
    if k != 2 * stride or dilation != 1:
        raise NotImplementedError("strided bwd_data is built for the model's k = 2*stride convs")
    plan = plan_convtr(c_out, c_in, stride, B, t_out + 1, flat_train_cols=t_out + 1)
    return plan._replace(p8=plan.p8 if plan.layout == TR_FLAT else None), t_out, pad_left, pad_right, tp


def conv1d_bwd_data(dy, v, g, t_in, stride=1, dilation=1, pad_mode=PAD_REFLECT, causal=True, scale=None, allow_view=False):
    """Gradient w.r.t. the input of SConv1d (dac/model/encodec.py:212-228) given dy (B, C_out, T_out).
    scale: the weight-norm scale g / ||v|| if the caller already has it (the forward computed it).
    allow_view: the caller's consumer takes rows with a stride (snake_bwd_fused): the result may then be the window
    [pad_left, pad_left + t_in) of the padded gradient rows -- a non-contiguous (B, C, t_in) view, mirrored edge samples added in
    place (fac_pad_fold_edges) -- instead of a copy (fac_pad_fold_bwd: 8 bytes per element to move the tensor by <= 54 samples)."""
    dy = _dev(dy, "dy")
    if scale is None and g is not None:
        scale = wn_scale(v, g)
    c_out, c_in, k = v.shape
    B, _, t_out = dy.shape
    plan, t_o, pad_left, pad_right, tp = plan_bwd_data(c_out, c_in, k, stride, dilation, B, t_in, causal)
    assert t_o == t_out, (t_o, t_out)
    layout = plan.layout
    if stride == 1:
        if layout == W_TAPS:
            # the flipped / transposed conv on the bf16 pipe too: materialise w = g v/||v||, swap channels, flip taps
            wt = flipped_weight(v, g, scale)                                   # (C_in, C_out, K) = weights of the bwd conv
            dxpad = conv1d(dy, None, c_in, k, dilation=dilation, pad_left=(k - 1) * dilation, pad_mode=PAD_ZERO, t_out=tp,
                           w_split=pack_conv_weight_split(wt, rows=64))
        elif layout == W_GEMM:
            w = rows_fma(v, scale) if g is not None else v                    # 1x1: the transposed GEMM on the bf16 pipe
            dxpad = conv1d(dy, None, c_in, 1, pad_left=0, pad_mode=PAD_ZERO, t_out=tp, w_split=pack_gemm_weight_split_t(w))
        else:
            dxpad = conv1d(dy, pack_conv_weight_bwd(v, g, scale), c_in, k, dilation=dilation, pad_left=(k - 1) * dilation,
                           pad_mode=PAD_ZERO, t_out=tp)
    else:
        dy_ext = torch.cat([dy, torch.zeros(B, c_out, 1, device=dy.device)], dim=2)
        wt = pack_convtr_for(layout, v, g, stride)
        if layout == TR_FLAT:            # short clips: one flattened signal (the trailing zero column of a clip is the x[t - 1] of
            dxpad = conv_transpose1d_flat(dy_ext, wt, c_in, stride, p8=plan.p8)      # the next clip's first frame)
        else:
            dxpad = conv_transpose1d(dy_ext, wt, c_in, stride)
        assert dxpad.shape[-1] == tp, (dxpad.shape, tp)
    if tp == t_in and FOLD_IN_PLACE in (1, 2):
        return dxpad                                  # no padding (the 1x1 convs): the padded gradient IS the gradient
    if allow_view and FOLD_IN_PLACE in (1, 3) and dxpad.is_contiguous() and (pad_mode == PAD_ZERO or t_in > pad_left + pad_right + 1):
        if pad_mode == PAD_REFLECT:
            _lib.check(_lib.load().fac_pad_fold_edges(_ptr(dxpad), B, c_in, t_in, tp, pad_left, _stream()), "fac_pad_fold_edges")
        return dxpad[:, :, pad_left:pad_left + t_in]
    dx = torch.empty(B, c_in, t_in, device=dy.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_pad_fold_bwd(_ptr(dxpad), _ptr(dx), B, c_in, t_in, tp, pad_left, pad_mode, _stream()),
               "fac_pad_fold_bwd")
    return dx


# 1 (default): both shortcuts; 0: neither (rounds 1-5); 2: only "no padding -> no copy"; 3: only the in-place edge fold + row-stride view
FOLD_IN_PLACE = 1


def _rows_view(t):
    """(tensor, row stride) for a (B, C, T) fp32 CUDA tensor whose rows are time-contiguous and evenly spaced (a window of a wider
    buffer, see conv1d_bwd_data(allow_view=True)); anything else is made contiguous first."""
    if t is None:
        return None, 0
    if (t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.stride(2) == 1 and t.stride(1) >= t.shape[2]
            and t.stride(0) == t.shape[1] * t.stride(1)):
        return t, t.stride(1)
    t = _dev(t, "dy")
    return t, t.shape[2]


def conv1d_bwd_weight(x, dy, k, stride=1, dilation=1, pad_mode=PAD_REFLECT, causal=True, pad_left=None, k1=0, dilation2=0,
                      want_db=False):
    """dW (C_out, C_in, K) of SConv1d (or of a plain conv when pad_left is given explicitly; k1 / dilation2: two-level taps).
    want_db: also return the bias gradient sum_{b,t} dy -- folded into the split kernel's pass over dy where that kernel runs."""
    x, dy = _dev(x, "x"), _dev(dy, "dy")
    B, c_in, t_in = x.shape
    _, c_out, t_out = dy.shape
    if pad_left is None:
        _, padding_total, _ = conv_out_len(t_in, k, stride, dilation)
        pad_left = padding_total if causal else padding_total - padding_total // 2
    dw = torch.empty(c_out, c_in, k, device=x.device, dtype=torch.float32)
    db = torch.empty(c_out, device=x.device, dtype=torch.float32) if want_db else None
    fused = _bwd_weight_launch(x, dy, dw, B, c_in, t_in, c_out, t_out, k, stride, dilation, pad_left, pad_mode, k1, dilation2, db=db)
    if want_db:
        return dw, (db if fused else bias_grad(dy))
    return dw


# One grow-only scratch per device for the split weight-gradient kernel (bf16 planes of both operands + partial sums): every
# launch goes to torch's current stream in program order, so consecutive layers can share it -- no per-layer allocation of
# hundreds of MB, and its size shows up once in peak_mem instead of as allocator churn.  FAC_WGRAD_WS_GB caps it.
_WGRAD_WS = {}
WGRAD_K1_STREAM = True      # k = 1 tails with few channels on conv1d_wgrad_k1.hip
WGRAD_WS_CAP = int(float(os.environ.get("FAC_WGRAD_WS_GB", "6")) * (1 << 30))


def _wgrad_workspace(device, nbytes):
    """One grow-only buffer per (device, stream): the discriminators' backward passes run on several streams at once
    (discriminator.py), and a launch's operand planes / partial sums must not be overwritten by another stream's launch."""
    key = (device, _raw_stream(device.index))
    ws = _WGRAD_WS.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        if ws is not None:
            del _WGRAD_WS[key]
            ws = None
        ws = _WGRAD_WS[key] = torch.empty((nbytes + (64 << 20)) // 4, device=device, dtype=torch.float32)
    return ws


def _bwd_weight_launch(x, dy, dw, B, c_in, t_in, c_out, t_out, k, stride, dilation, pad_left, pad_mode, k1=0, dilation2=0, db=None):
    """Weight gradient of one conv (see _bwd_weight_launch_inner); counted by the FLOP counter and, under a ConvLaunchProfile,
    timed as ONE record per conv: operand planes + GEMM + split-K reduction together."""
    flops = 2.0 * B * c_out * c_in * k * t_out
    if _FLOPS is not None:
        _FLOPS.add("wgrad", flops)
    if _PROFILE is None:
        return _bwd_weight_launch_inner(x, dy, dw, B, c_in, t_in, c_out, t_out, k, stride, dilation, pad_left, pad_mode, k1, dilation2, db)[0]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r, entry = _bwd_weight_launch_inner(x, dy, dw, B, c_in, t_in, c_out, t_out, k, stride, dilation, pad_left, pad_mode, k1, dilation2, db)
    e1.record()
    _PROFILE.records.append((wgrad_profile_label(entry, B, c_in, t_in, c_out, t_out, k, stride, dilation, k1, dilation2, db is not None),
                             flops, e0, e1))
    return r


WgradSplitForm = namedtuple("WgradSplitForm", "kernel slices tiles_per_slice last_slice_tiles xcd_order row_tiles narrow_row_tiles db_fused")
WGRAD_SPLIT_KERNELS = ("kmajor", "kmajor_ksplit", "planes<10,3>", "planes<14,3>", "planes<19,2>")


def wgrad_split_form(B, c_in, t_in, c_out, t_out, k, stride=1, dilation=1, k1=0, dilation2=0, want_db=False):
    """What the split weight-gradient entry does for this shape (fac_conv1d_bwd_weight_split_form: host only, the launch reads the
    same plan), or None where its workspace query answers -1."""
    out = (C.c_int * 8)()
    if _lib.load().fac_conv1d_bwd_weight_split_form(B, c_in, t_in, c_out, t_out, k, stride, dilation, k1, dilation2, int(want_db), out) != 0:
        return None
    return WgradSplitForm(WGRAD_SPLIT_KERNELS[out[0]], out[1], out[2], out[3], bool(out[4]), out[5], out[6], bool(out[7]))


def wgrad_profile_label(entry, B, c_in, t_in, c_out, t_out, k, stride, dilation, k1, dilation2, want_db):
    """The profile record's name for the C entry _bwd_weight_launch_inner called; the split entry's kernel form appended."""
    if entry == "fac_conv1d_bwd_weight_k1":
        return "weight gradient: wgrad_k1_kernel (k = 1 streaming, fp32 MFMA) + reduce"
    if entry == "fac_conv1d_bwd_weight_taps":
        return "weight gradient: wgrad_k1_kernel (virtual-row taps, fp32 MFMA) + reduce"
    if entry == "fac_conv1d_bwd_weight":
        return "weight gradient: conv1d_wgrad_kernel (fp32 MFMA) + reduce"
    form = wgrad_split_form(B, c_in, t_in, c_out, t_out, k, stride, dilation, k1, dilation2, want_db)
    return "weight gradient: split_planes + conv1d_wgrad_split/%s + reduce (bf16x3 split)" % form.kernel


def _bwd_weight_launch_inner(x, dy, dw, B, c_in, t_in, c_out, t_out, k, stride, dilation, pad_left, pad_mode, k1=0, dilation2=0, db=None):
    """dW on the bf16 matrix pipe with fp32-grade splitting (conv1d_wgrad_split.hip) when the shape qualifies and
    BF16_SPLIT is on, else on the fp32 MFMA kernel.  db: optional (C_out) buffer for the bias gradient; returns True when the
    launch filled it, and with it the name of the C entry called."""
    lib = _lib.load()
    if WGRAD_K1_STREAM and BF16_SPLIT and k == 1 and stride == 1 and pad_left == 0 and t_in == t_out and k1 in (0, 1):
        # few channels, long signal (the ResidualUnit tails at C = 64 / 96 / 192): both tensors once through the fp32 matrix pipe
        # instead of two operand-split passes + plane reads (conv1d_wgrad_k1.hip); the bias gradient rides on the dy fragments
        nb = lib.fac_conv1d_bwd_weight_k1_ws_bytes_for(_ptr(x), _ptr(dy), B, c_in, c_out, t_in)     # -1 also for misaligned x / dy
        if nb > 0:
            ws = _wgrad_workspace(x.device, nb)
            _lib.check(lib.fac_conv1d_bwd_weight_k1(_ptr(x), _ptr(dy), _ptr(dw), _ptr(db), _ptr(ws), nb, B, c_in, c_out, t_in, _stream()),
                       "fac_conv1d_bwd_weight_k1")
            return db is not None, "fac_conv1d_bwd_weight_k1"
    if WGRAD_K1_STREAM and BF16_SPLIT and k > 1 and stride == 1 and c_in * k <= 64 and c_out in (32, 64) and t_out >= 4096:
        # first layers (1 -> 64 k = 7 of the encoder, 2 -> 32 (3, 9) of the multi-resolution discriminator): the C_in * K columns of dW
        # are shifted views of one or two input rows -- the same kernel with virtual rows (fac_conv1d_bwd_weight_taps) on the padded input
        kk1 = k1 if 0 < k1 < k else k
        d2 = dilation2 if 0 < k1 < k else 0
        nb = lib.fac_conv1d_bwd_weight_taps_ws_bytes_for(_ptr(dy), B, c_in, c_out, t_out, k, kk1, dilation, d2)
        if nb > 0:
            tx = lib.fac_conv1d_bwd_weight_taps_tx(t_out, k, kk1, dilation, d2)
            need = (t_out - 1) + (k // kk1 - 1) * d2 + (kk1 - 1) * dilation + 1          # positions of the padded input the outputs read
            right = max(0, need - pad_left - t_in)
            if pad_mode == PAD_REFLECT and max(pad_left, right) > 0:
                xp = torch.nn.functional.pad(x, (pad_left, right), mode="reflect")         # data movement only (a 1- / 2-channel signal)
            else:
                xp = torch.nn.functional.pad(x, (pad_left, right))
            if xp.shape[-1] < tx:
                xp = torch.nn.functional.pad(xp, (0, tx - xp.shape[-1]))
            ws = _wgrad_workspace(x.device, nb)
            _lib.check(lib.fac_conv1d_bwd_weight_taps(_ptr(xp), _ptr(dy), _ptr(dw), _ptr(db), _ptr(ws), nb, B, c_in, xp.shape[-1], c_out,
                                                      t_out, k, kk1, dilation, d2, _stream()), "fac_conv1d_bwd_weight_taps")
            return db is not None, "fac_conv1d_bwd_weight_taps"
    nbytes = lib.fac_conv1d_bwd_weight_split_ws_bytes(B, c_in, t_in, c_out, t_out, k, stride, dilation, k1, dilation2) if BF16_SPLIT else -1
    if nbytes > WGRAD_WS_CAP:       # beyond the workspace budget: the fp32 kernel (no operand planes) takes the layer
        nbytes = -1
    if nbytes > 0:
        ws = _wgrad_workspace(x.device, nbytes)
        if db is not None and lib.fac_conv1d_bwd_weight_split_db_ok(B, c_in, t_in, c_out, t_out, k, stride, dilation, k1, dilation2):
            _lib.check(lib.fac_conv1d_bwd_weight_split_db(_ptr(x), _ptr(dy), _ptr(dw), _ptr(db), _ptr(ws), nbytes, B, c_in, t_in, c_out,
                                                          t_out, k, stride, dilation, pad_left, pad_mode, k1, dilation2, _stream()),
                       "fac_conv1d_bwd_weight_split_db")
            return True, "fac_conv1d_bwd_weight_split_db"
        _lib.check(lib.fac_conv1d_bwd_weight_split(_ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), nbytes, B, c_in, t_in, c_out, t_out, k,
                                                   stride, dilation, pad_left, pad_mode, k1, dilation2, _stream()),
                   "fac_conv1d_bwd_weight_split")
        return False, "fac_conv1d_bwd_weight_split"
    kk1 = k1 if 0 < k1 < k else k                      # the fp32 kernel sees k / kk1 virtual channels per input channel
    nbytes = lib.fac_conv1d_bwd_weight_ws_bytes(B, c_in * (k // kk1), c_out, t_out, kk1)
    ws = torch.empty(nbytes // 4, device=x.device, dtype=torch.float32)
    _lib.check(lib.fac_conv1d_bwd_weight(_ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), nbytes, B, c_in, t_in, c_out, t_out, k,
                                         stride, dilation, pad_left, pad_mode, k1, dilation2, _stream()), "fac_conv1d_bwd_weight")
    return False, "fac_conv1d_bwd_weight"


def weight_norm_bwd(v, g, dw):
    v, g, dw = _dev(v), _dev(g), _dev(dw)
    n = v.shape[0]
    dv, dg = torch.empty_like(v), torch.empty_like(g)
    _lib.check(_lib.load().fac_weight_norm_bwd(_ptr(v), _ptr(g), _ptr(dw), _ptr(dv), _ptr(dg), n, v.numel() // n, _stream()),
               "fac_weight_norm_bwd")
    return dv, dg


def snake_bwd(x, alpha, dy):
    x, dy = _dev(x, "x"), _dev(dy, "dy")
    B, c, t = x.shape
    dx, dalpha = torch.empty_like(x), torch.empty(c, device=x.device, dtype=torch.float32)
    scratch = torch.empty(32 * c, device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_snake_bwd(_ptr(x), _ptr(alpha), _ptr(dy), _ptr(dx), _ptr(dalpha), _ptr(scratch), B, c, t,
                                         _stream()), "fac_snake_bwd")
    return dx, dalpha


def snake_bwd_fused(x, alpha, dy, add=None, want_bias=False):
    """Snake backward with the fan-in add and the producing conv's bias gradient fused in (fac_snake_bwd_fused):
    dx = add + dy * dsnake/dx, dalpha, [dbias = sum over (b, t) of dx]."""
    x, add = _dev(x, "x"), _dev(add, "add")
    dy, dy_rs = _rows_view(dy)              # dy may be a window of padded gradient rows (conv1d_bwd_data(allow_view=True))
    B, c, t = x.shape
    dx, dalpha = torch.empty_like(x), torch.empty(c, device=x.device, dtype=torch.float32)
    db = torch.empty(c, device=x.device, dtype=torch.float32) if want_bias else None
    scratch = torch.empty(64 * c, device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_snake_bwd_fused_rs(_ptr(x), _ptr(alpha), _ptr(dy), dy_rs, _ptr(add), _ptr(dx), _ptr(dalpha), _ptr(db),
                                                  _ptr(scratch), B, c, t, _stream()), "fac_snake_bwd_fused")
    return dx, dalpha, db


def bias_grad(dy):
    dy = _dev(dy, "dy")
    B, c, t = dy.shape
    db = torch.empty(c, device=dy.device, dtype=torch.float32)
    scratch = torch.empty(32 * c, device=dy.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_bias_grad(_ptr(dy), _ptr(db), _ptr(scratch), B, c, t, _stream()), "fac_bias_grad")
    return db


def plan_convtr_bwd(c_in, c_out, stride, B, t_in):
    """The dx launch of conv_transpose1d_bwd, from shapes alone: the strided forward conv of dy (B clips of t_in * stride columns)
    on the transposed conv's own weights.  p8 is None off the flattened form: the per-clip launch takes no pre-pass."""
    plan = plan_conv(c_in, c_out, 2 * stride, stride, 1, B, t_in * stride, t_in, flat_train="zero")
    return plan._replace(p8=plan.p8 if plan.form == FLAT_STRIDED else None)


def conv_transpose1d_bwd(x, dy, v, g, stride, causal=True):
    """SConvTranspose1d (kernel 2*stride): -> (dx, dW (C_in, C_out, K)).  dx is the strided forward conv of dy
    on the same weights; dW the weight-gradient kernel with the roles of input and output swapped.
    The full transposed output has (T_in + 1) s columns; the causal layer keeps the first T_in s, the non-causal one drops
    ceil(s/2) on the left and floor(s/2) on the right (dac/model/encodec.py:265-269, conv_transpose1d's phase_shift).  So dy sits
    at offset `shift` = 0 or ceil(s/2) inside the full-length gradient, whose trimmed columns are zero: both launches read dy with
    that zero-padded offset (pad_left = shift), no copy."""
    x, dy = _dev(x, "x"), _dev(dy, "dy")
    B, c_in, t_in = x.shape
    c_out, k = v.shape[1], v.shape[2]
    assert k == 2 * stride and dy.shape == (B, c_out, t_in * stride)
    shift = 0 if causal else stride - stride // 2
    plan = plan_convtr_bwd(c_in, c_out, stride, B, t_in)
    wp, ws = pack_conv_for(plan.layout, v, g, stride)
    if plan.form == FLAT_STRIDED:
        # short clips: every clip gets its s columns of zeros (shift in front, s - shift behind) and the clips run as one flattened
        # signal -- the kernel cannot offset inside the concatenation, so this is the one path that pads with a copy (as causal)
        dx = conv1d_flat(torch.nn.functional.pad(dy, (shift, stride - shift)), ws, c_in, k, stride, t_in, p8=plan.p8)
    else:
        dx = conv1d(dy, wp, c_in, k, stride=stride, pad_left=shift, pad_mode=PAD_ZERO, t_out=t_in, w_split=ws)
    dw = torch.empty(c_in, c_out, k, device=x.device, dtype=torch.float32)
    _bwd_weight_launch(dy, x, dw, B, c_out, t_in * stride, c_in, t_in, k, stride, 1, shift, PAD_ZERO)
    return dx, dw


def lstm_layer_bwd(d_out, w_hh, gates, cs, H, batch=None):
    """BPTT of one layer (fac_lstm_layer_bwd): d_out (H, T, BP) gradient of the layer's h sequence -> dgates (4H, T, BP).
    batch: number of real columns; with it the resident kernel (fac_lstm_layer_bwd_persist) runs where it applies."""
    _, T, BP = d_out.shape
    lib = _lib.load()
    if lstm_persist_ok(H, batch):
        dgates = torch.empty(4 * H, T, BP, device=d_out.device, dtype=torch.float32)
        nc = 16 * ((batch + 15) // 16)
        _zero_pad_cols(dgates, nc)
        scratch = torch.empty((4 + 4 * T) * H * nc, device=d_out.device, dtype=torch.float32)
        _lib.check(lib.fac_lstm_layer_bwd_persist(_ptr(_dev(d_out)), _ptr(pack_lstm_whh16(w_hh, transposed=True)), _ptr(gates),
                                                  _ptr(cs), _ptr(dgates), _ptr(scratch), T, H, batch, BP, _stream()),
                   "fac_lstm_layer_bwd_persist")
        return dgates
    wt = torch.empty(4 * H * H, device=d_out.device, dtype=torch.float32)
    _lib.check(lib.fac_pack_lstm_whh_t(_ptr(_dev(w_hh)), _ptr(wt), H, _stream()), "fac_pack_lstm_whh_t")
    dgates = torch.empty(4 * H, T, BP, device=d_out.device, dtype=torch.float32)
    scratch = torch.empty(13 * H * BP, device=d_out.device, dtype=torch.float32)
    _lib.check(lib.fac_lstm_layer_bwd(_ptr(_dev(d_out)), _ptr(wt), _ptr(gates), _ptr(cs), _ptr(dgates), _ptr(scratch), T, H, BP,
                                      _stream()), "fac_lstm_layer_bwd")
    return dgates


def lstm_gate_bwd(dy_t, rec, gates_t, c_t, c_prev, dc, dgates_t, H, BP, rs, first):
    """Views into (rows, T, BP) buffers at one time step (row stride rs); rec / dc dense (H, BP)."""
    _lib.check(_lib.load().fac_lstm_gate_bwd(_ptr(dy_t), _ptr(rec), _ptr(gates_t), _ptr(c_t), _ptr(c_prev), _ptr(dc),
                                             _ptr(dgates_t), H, BP, rs, 1 if first else 0, _stream()), "fac_lstm_gate_bwd")


def tanh_bwd(y, dy):
    y, dy = _dev(y), _dev(dy)
    dx = torch.empty_like(dy)
    _lib.check(_lib.load().fac_tanh_bwd(_ptr(y), _ptr(dy), _ptr(dx), dy.numel(), _stream()), "fac_tanh_bwd")
    return dx


def pair_bwd(a, b, da, mode, eps, scale, accumulate):
    a, b = _dev(a), _dev(b)
    _lib.check(_lib.load().fac_pair_bwd(_ptr(a), _ptr(b), _ptr(da), a.numel(), mode, eps, scale, 1 if accumulate else 0,
                                        _stream()), "fac_pair_bwd")
    return da


def spec_power_bwd(spec, dout, power):
    spec, dout = _dev(spec), _dev(dout)
    B, f2, nf = spec.shape
    dspec = torch.empty_like(spec)
    _lib.check(_lib.load().fac_spec_power_bwd(_ptr(spec), _ptr(dout), _ptr(dspec), B, f2 // 2, nf, power, _stream()),
               "fac_spec_power_bwd")
    return dspec


def stft_frames_bwd(dframes, T, hop, pad, n_off):
    dframes = _dev(dframes)
    B, n_win, nf = dframes.shape
    dwave = torch.empty(B, T, device=dframes.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_stft_frames_bwd(_ptr(dframes), _ptr(dwave), B, T, n_win, nf, hop, pad, n_off, _stream()),
               "fac_stft_frames_bwd")
    return dwave


# --------------------------------------------------------------------------------- quantizer / LayerNorm backward
def vq_latent_bwd(z_e, codebook, codes, d_zst=None, wc=None, want_dze=True, want_zst=False):
    z_e = _dev(z_e)
    B, _, T = z_e.shape
    d_ze = torch.empty_like(z_e) if want_dze else None
    z_st = torch.empty_like(z_e) if want_zst else None
    _lib.check(_lib.load().fac_vq_latent_bwd(_ptr(z_e), _ptr(codebook), C.c_void_p(codes.data_ptr()), codes.stride(0),
                                             _ptr(d_zst), _ptr(wc), _ptr(d_ze), _ptr(z_st), B, T, _stream()), "fac_vq_latent_bwd")
    return d_ze, z_st


def vq_codebook_grad(z_e, codebook, codes, wb):
    z_e = _dev(z_e)
    B, _, T = z_e.shape
    dcb = torch.empty_like(codebook)
    _lib.check(_lib.load().fac_vq_codebook_grad(_ptr(z_e), _ptr(codebook), C.c_void_p(codes.data_ptr()), codes.stride(0),
                                                _ptr(wb), _ptr(dcb), B, T, codebook.shape[0], 0, _stream()), "fac_vq_codebook_grad")
    return dcb


def layernorm_c_affine_bwd(x, style, dout):
    x, style, dout = _dev(x), _dev(style), _dev(dout)
    B, c, T = x.shape
    dx, dstyle = torch.empty_like(x), torch.empty_like(style)
    stats = torch.empty(B * T * 2, device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_layernorm_c_affine_bwd(_ptr(x), _ptr(style), _ptr(dout), _ptr(dx), _ptr(dstyle), _ptr(stats),
                                                      B, c, T, _stream()), "fac_layernorm_c_affine_bwd")
    return dx, dstyle


def rows_fma(a, w=None, c=None, sign=1.0):
    """a[b] * w[b] + sign * c[b] for (B, ...) tensors (w (B,), c like a; both optional)."""
    a = _dev(a)
    B = a.shape[0]
    out = torch.empty_like(a)
    _lib.check(_lib.load().fac_rows_fma(_ptr(a), _ptr(w), _ptr(_dev(c)), _ptr(out), B, a.numel() // B, sign, _stream()),
               "fac_rows_fma")
    return out


# --------------------------------------------------------------------------------- pitch: JDC glue and the predictor targets (jdc.hip)
def leaky_relu_rows(x, slope, pitch, valid, rows_per_group, valid_rows):
    """LeakyReLU over a row-concatenated signal (1, C, rows * pitch); gap columns and separator rows come out zero (fac_leaky_relu)."""
    x = _dev(x, "x")
    y = torch.empty_like(x)
    _lib.check(_lib.load().fac_leaky_relu(_ptr(x), _ptr(None), _ptr(y), x.numel(), C.c_float(slope), x.shape[-1], pitch, valid,
                                          rows_per_group, valid_rows, _stream()), "fac_leaky_relu")
    return y


def jdc_affine_lrelu_pool(x, scale, shift, rows, rows_per_group, w_in, p_in, pool, slope):
    """x (1, C, rows * p_in) -> (1, C, rows * p_in / pool): eval BatchNorm (scale / shift (C,), or None for identity) -> LeakyReLU ->
    max over `pool` neighbouring bins; exact zeros in the gaps and separator rows (fac_jdc_affine_lrelu_pool)."""
    x, scale, shift = _dev(x, "x"), _dev(scale, "scale"), _dev(shift, "shift")
    c = x.shape[-2]
    if x.shape[-1] != rows * p_in or p_in % pool:
        raise ValueError(f"jdc_affine_lrelu_pool: signal of {x.shape[-1]} columns is not {rows} rows of pitch {p_in} (pool {pool})")
    p_out = p_in // pool
    y = torch.empty(1, c, rows * p_out, device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_jdc_affine_lrelu_pool(_ptr(x), _ptr(scale), _ptr(shift), _ptr(y), c, rows, rows_per_group, w_in, p_in,
                                                     pool, p_out, C.c_float(slope), _stream()), "fac_jdc_affine_lrelu_pool")
    return y


def jdc_layout_in(mel, pitch):
    """mel (B, 1, W, T) -> the stage-0 signal (1, 1, B * (T + 1) * pitch)."""
    mel = _dev(mel, "mel")
    B, _, W, T = mel.shape
    out = torch.empty(1, 1, B * (T + 1) * pitch, device=mel.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_jdc_layout_in(_ptr(mel), _ptr(out), B, W, T, pitch, _stream()), "fac_jdc_layout_in")
    return out


def jdc_to_time_major(x, B, T, W, pitch, reverse=False):
    """Stage signal (1, C, B * (T + 1) * pitch) -> time-major LSTM input (C * W, T, pad32(B)); reverse: time flipped."""
    x = _dev(x, "x")
    c, BP = x.shape[-2], pad32(B)
    out = torch.empty(c * W, T, BP, device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_jdc_to_time_major(_ptr(x), _ptr(out), B, c, T, W, pitch, BP, 1 if reverse else 0, _stream()),
               "fac_jdc_to_time_major")
    return out


def jdc_to_nchw(x, B, T, W, pitch, transposed=False):
    """Stage signal (1, C, B * (T + 1) * pitch) -> (B, C, T, W), or (B, C, W, T) with transposed."""
    x = _dev(x, "x")
    c = x.shape[-2]
    out = torch.empty((B, c, W, T) if transposed else (B, c, T, W), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_jdc_to_nchw(_ptr(x), _ptr(out), B, c, T, W, pitch, 1 if transposed else 0, _stream()), "fac_jdc_to_nchw")
    return out


def jdc_head(h_fwd, h_bwd, w, bias, B):
    """|Linear(2H -> 1)| over [h_fwd(t) | h_bwd(T - 1 - t)], both (H, T, BP) time-major -> (B, T)."""
    h_fwd, h_bwd, w, bias = _dev(h_fwd, "h_fwd"), _dev(h_bwd, "h_bwd"), _dev(w, "weight"), _dev(bias, "bias")
    H, T, BP = h_fwd.shape
    if h_bwd.shape != h_fwd.shape or w.numel() != 2 * H or bias.numel() != 1:
        raise ValueError("jdc_head: the two directions must have one shape (H, T, BP), the weight 2H entries, the bias one")
    out = torch.empty(B, T, device=h_fwd.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_jdc_head(_ptr(h_fwd), _ptr(h_bwd), _ptr(w), _ptr(bias), _ptr(out), B, T, H, BP, _stream()), "fac_jdc_head")
    return out


def f0_normalize(f0, want_mean=False):
    """f0 (B, T) -> the normalised log-F0 targets of train.py:224-256 (fac_f0_normalize) [, per-clip means (B,)]."""
    f0 = _dev(f0, "f0")
    if f0.dim() != 2:
        raise ValueError(f"f0 must be (B, T), got {tuple(f0.shape)}")
    B, T = f0.shape
    out = torch.empty_like(f0)
    mean = torch.empty(B, device=f0.device, dtype=torch.float32) if want_mean else None
    _lib.check(_lib.load().fac_f0_normalize(_ptr(f0), _ptr(out), _ptr(mean), B, T, _stream()), "fac_f0_normalize")
    return (out, mean) if want_mean else out


def mel_log_norm(mel):
    """mel (B, n_mels, T) -> (B, T): log of the L2 norm over the bins of exp(4 mel - 4) (fac_mel_log_norm)."""
    mel = _dev(mel, "mel")
    if mel.dim() != 3:
        raise ValueError(f"mel must be (B, n_mels, T), got {tuple(mel.shape)}")
    B, M, T = mel.shape
    out = torch.empty(B, T, device=mel.device, dtype=torch.float32)
    _lib.check(_lib.load().fac_mel_log_norm(_ptr(mel), _ptr(out), B, M, T, _stream()), "fac_mel_log_norm")
    return out


# --------------------------------------------------------------------------------- slots of a running streaming session
def edge_segments(C, W):
    """Where a contiguous left-context buffer (B, C, W) keeps slot b (the segment form of include/facodec_hip.h):
    [(offset, rows, row_stride, row_len, slot_lo, slot_hi)], elements relative to the tensor's first."""
    return [(0, 1, 0, C * W, C * W, 32 * C * W)]


def lstm_state_segments(H, BP):
    """The same for a carried LSTM state (3, H, BP) = [c | h ping | h pong] (fac_lstm_layer_fwd): the cell plane is row-major
    (H, BP), the two hidden planes are in MFMA-B fragment order [BP/32][H/8][2][32 batch][4]."""
    if H % 8 or BP % 32:
        raise ValueError(f"LSTM state with H = {H}, BP = {BP}: H must be a multiple of 8, BP of 32")
    plane = H * BP
    return [(0, H, BP, 1, 1, 32), (plane, H // 4, 128, 4, 4, 32 * H), (2 * plane, H // 4, 128, 4, 4, 32 * H)]


def _segment_extent(seg, b):
    off, rows, row_stride, row_len, slot_lo, slot_hi = seg
    first = off + (b >> 5) * slot_hi + (b & 31) * slot_lo
    return first, first + (rows - 1) * row_stride + row_len


class SlotTable:
    """The device-resident segment table and tile list of fac_slot_copy over B slots, built once:

        table = SlotTable(B); table.add_edge(buf) ...; table.add_lstm_state(state) ...; table.freeze()
        table.copy(src, [dst, ...])               # any number of destinations, FAC_SLOT_MAX_DST per launch

    Every run of every slot is checked against its tensor's extent here, on the host: the entry trusts the table."""

    def __init__(self, B):
        self.B = int(B)
        self._tensors, self._segs = [], []
        self._dev = None
        self.elems = 0                                # floats one slot holds

    def _add(self, t, segs, what):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.FacodecHipError(f"{what} must live on the GPU (got {getattr(t, 'device', type(t).__name__)}); there is no CPU path")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.FacodecHipError(f"{what} must be contiguous float32 (got {t.dtype})")
        if self._dev is not None:
            raise RuntimeError("the table is frozen")
        for seg in segs:
            for b in range(self.B):
                lo, hi = _segment_extent(seg, b)
                if lo < 0 or hi > t.numel():
                    raise ValueError(f"{what} {tuple(t.shape)}: slot {b} reaches element {hi} of {t.numel()}")
            if seg[1] * seg[3] >= 1 << 31:
                raise ValueError(f"{what} {tuple(t.shape)}: a slot of 2^31 elements or more")
            self._segs.append((t.data_ptr() + 4 * seg[0],) + tuple(seg[1:]))
        self._tensors.append(t)                       # the table holds raw pointers: keep their owners alive

    def add_edge(self, buf):
        if buf.dim() != 3 or buf.shape[0] != self.B:
            raise ValueError(f"a left-context buffer is (B = {self.B}, C, W), got {tuple(buf.shape)}")
        self._add(buf, edge_segments(buf.shape[1], buf.shape[2]), "left-context buffer")

    def add_lstm_state(self, state):
        if state.dim() != 3 or state.shape[0] != 3 or state.shape[2] < self.B:
            raise ValueError(f"an LSTM state is (3, H, BP >= B = {self.B}), got {tuple(state.shape)}")
        self._add(state, lstm_state_segments(state.shape[1], state.shape[2]), "LSTM state")

    def freeze(self):
        if not self._segs:
            raise ValueError("an empty slot table")
        arr = (_lib.SlotSeg * len(self._segs))()
        tiles = []
        for i, (ptr, rows, row_stride, row_len, slot_lo, slot_hi) in enumerate(self._segs):
            s = arr[i]
            s.base, s.slot_hi, s.rows, s.row_stride, s.row_len, s.slot_lo, s.elems = ptr, slot_hi, rows, row_stride, row_len, slot_lo, rows * row_len
            tiles += [(i, e) for e in range(0, rows * row_len, _lib.SLOT_TILE)]
            self.elems += rows * row_len
        device = self._tensors[0].device
        self._segs_dev = h2d(torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8), device)
        self._tiles_dev = h2d(torch.tensor(tiles, dtype=torch.int32), device)
        self.n_seg, self.n_tiles = len(self._segs), len(tiles)
        self._dev = device
        return self

    def copy(self, src, dsts):
        """Slot `src` -> every slot of `dsts` on the current stream; refusals are fac_slot_copy's."""
        if self._dev is None:
            raise RuntimeError("freeze() the table first")
        dsts = [int(d) for d in dsts]
        if len(set(dsts)) != len(dsts):
            raise _lib.FacodecHipError(f"fac_slot_copy: duplicate destination slot in {dsts}")
        lib = _lib.load()
        for i in range(0, max(len(dsts), 1), _lib.SLOT_MAX_DST):
            part = dsts[i:i + _lib.SLOT_MAX_DST]
            _lib.check(lib.fac_slot_copy(_ptr(self._segs_dev), self.n_seg, _ptr(self._tiles_dev), self.n_tiles, self.B, int(src),
                                         (C.c_int32 * max(len(part), 1))(*part), len(part), _stream()), "fac_slot_copy")


def slot_copy_raw(table, src, dsts):
    """fac_slot_copy exactly as given (one launch, no splitting): what the refusal tests call."""
    dsts = [int(d) for d in dsts]
    _lib.check(_lib.load().fac_slot_copy(_ptr(table._segs_dev), table.n_seg, _ptr(table._tiles_dev), table.n_tiles, table.B, int(src),
                                         (C.c_int32 * max(len(dsts), 1))(*dsts), len(dsts), _stream()), "fac_slot_copy")


def rows_pick_map(rows, inner, device):
    """Host list of source rows (-1: none) -> the device int32 map of rows_pick for a source with `inner` sub-rows per row
    ((B, n_q, k) codes: inner = n_q), through h2d (no host stall)."""
    flat = [(-1 if r < 0 else r * inner + q) for r in rows for q in range(inner)]
    return h2d(torch.tensor(flat, dtype=torch.int32), device)


def rows_pick(src, row_map, out=None):
    """out[r] = src[row_map[r]] where row_map[r] names a row of src, zeros elsewhere (fac_rows_pick).  src (n_src, L) or
    (n, q, L) taken as n q rows, float32 / int32 / int64, last dimension dense, rows of one pitch (a [:, :, :k] slice of a wider
    static buffer is read in place); row_map: int32 on the device, one entry per output row; out: dense, row_map.numel() rows."""
    if not src.is_cuda or not row_map.is_cuda:
        raise _lib.FacodecHipError(f"rows_pick: src and row_map must live on the GPU (got {src.device}, {row_map.device}); there is no CPU path")
    if src.dtype not in (torch.float32, torch.int32, torch.int64) or row_map.dtype != torch.int32 or not row_map.is_contiguous():
        raise _lib.FacodecHipError(f"rows_pick: src float32 / int32 / int64 and a dense int32 row_map (got {src.dtype}, {row_map.dtype})")
    if src.dim() not in (2, 3) or (src.shape[-1] > 1 and src.stride(-1) != 1):
        raise ValueError(f"rows_pick: src must be (n, L) or (n, q, L) with a dense last dimension, got {tuple(src.shape)}")
    L = src.shape[-1]
    n_src = src.numel() // L
    pitch = src.stride(-2)
    if src.dim() == 3 and src.shape[0] > 1 and src.shape[1] > 1 and src.stride(0) != src.shape[1] * pitch:
        raise ValueError("rows_pick: the rows of src do not have one pitch")
    if src.dim() == 3 and src.shape[1] == 1:
        pitch = src.stride(0)
    if n_src == 1:
        pitch = L
    words = src.element_size() // 4
    n_dst = row_map.numel()
    if out is None:
        out = torch.empty((n_dst, L) if src.dim() == 2 else (n_dst // src.shape[1], src.shape[1], L), device=src.device, dtype=src.dtype)
    elif out.dtype != src.dtype or not out.is_contiguous() or out.numel() != n_dst * L or not out.is_cuda:
        raise ValueError(f"rows_pick: out must be dense {src.dtype} with {n_dst} rows of {L}, got {tuple(out.shape)} {out.dtype}")
    _lib.check(_lib.load().fac_rows_pick(_ptr(src), pitch * words, _ptr(out), _ptr(row_map), n_dst, n_src, L * words, _stream()),
               "fac_rows_pick")
    return out
