"""Real-time voice conversion (facodec_amd.streaming.StreamingConverter) and the kernel change under it, the per-clip conditioning
row of the folded WaveNet gate (fac_conv_desc.gate_cond).

  host   what the session refuses before any launch; the planner's handling of gate_cond; the oracle's causal redecoder path
         against tests/golden/redecoder_causal.npz (made from the real reference by tests/golden/make_golden_redecoder_causal.py);
  gpu    the conditioned gate epilogue bit-equal to conv1d -> gate_tanh_sigmoid(a, g) on both few-column kernels; the session
         against the offline redecoder on the same signal, against the reference fixture, folded against unfolded, set_target.

The GPU tests print their figures ([tol] lines).  Measured on MI355X: gated epilogue against the fp64 gate 2.5e-7 .. 4.4e-7 (fp32-CPU
2.5e-7 .. 5.2e-7), bit-equal to the unfolded pair in every case; session against the offline redecoder 4.6e-6 .. 5.0e-6, against the
reference fixture's wave probes 2.7e-6; first / second hop after a mid-stream set_target 5.7e-3 / 1.6e-2 away from the unswitched
session, the two voices 5.8e-2 apart.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from facodec_amd import _lib, ops, synth
from test_conv_plan_cpu import fake_operands

gpu = pytest.mark.gpu
E2E_TOL = 1e-4           # tests/test_gpu_parity.py: end-to-end fp32 noise of the project's paths against each other / the reference
GEMV_NAME = "conv1d_gemv_kernel (single launch, <=4 columns)"
SKINNY_NAME = "conv1d_skinny_kernel (split reduction, <=640 columns)"


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _redecoder_params(causal=True, lstm=2):
    from facodec_amd.commons import default_redecoder_params
    args = default_redecoder_params()
    args.decoder_causal, args.decoder_lstm = causal, lstm
    return args


# ================================================================================================================ host only
def test_converter_refuses_on_the_host():
    """Non-causal redecoder (the shipped config_redecoder.yml): NotImplementedError naming the first offending conv; a timbre of
    the wrong shape, an n_c beyond the redecoder's content tables: ValueError.  CPU models, no launch is reached."""
    from facodec_amd.commons import build_model, default_model_params, default_redecoder_params
    from facodec_amd.streaming import StreamingConverter
    codec = build_model(default_model_params())
    with pytest.raises(NotImplementedError, match=r"redecoder\.encoder\.encoder\.in_layers\.0 is not causal"):
        StreamingConverter(codec, build_model(default_redecoder_params(), stage="redecoder"), torch.zeros(2, 1024))
    red = build_model(_redecoder_params(), stage="redecoder")
    with pytest.raises(ValueError, match=r"target_timbre must be a float32 GPU tensor \(B, 1024\), got \(2, 512\)"):
        StreamingConverter(codec, red, torch.zeros(2, 512))
    with pytest.raises(ValueError, match="target_timbre must be float32"):
        StreamingConverter(codec, red, torch.zeros(2, 1024, dtype=torch.float64))
    with pytest.raises(ValueError, match="must live on the GPU"):
        StreamingConverter(codec, red, torch.zeros(2, 1024))
    with pytest.raises(ValueError, match="n_c = 3"):
        StreamingConverter(codec, red, torch.zeros(2, 1024), n_c=3)
    # a causal WaveNet in front of a non-causal decoder: the decoder's first conv is named
    mixed = build_model(_redecoder_params(), stage="redecoder")
    mixed.decoder = build_model(default_redecoder_params(), stage="redecoder").decoder
    with pytest.raises(NotImplementedError, match=r"redecoder\.decoder\.model\.0 is not causal"):
        StreamingConverter(codec, mixed, torch.zeros(2, 1024))


def _gate_desc(B, c_in, c_out, T_out, K, cond=True, act=ops.ACT_GATE):
    d = ops.conv_desc(B, c_in, T_out + K - 1, c_out, K, pad_left=0, pad_mode=ops.PAD_ZERO, t_out=T_out, act=act)
    return fake_operands(d, "w", "bias", *(("gate_cond",) if cond else ()), gate_cond_bs=16 * c_out)


def test_planner_takes_gate_cond_with_the_gate_only():
    """gate_cond is an input of FAC_ACT_GATE: both few-column kernels take it (named apart by fac_conv1d_variant), any other
    epilogue with it is refused on the host, by the planner and by the launch entry alike."""
    lib = _lib.load()
    assert ctypes.sizeof(_lib.ConvDesc) >= _lib.ConvDesc.gate_cond_bs.offset + 8
    assert ops.conv_variant(_gate_desc(1, 512, 1024, 2, 5)) == (10, GEMV_NAME)
    assert ops.conv_variant(_gate_desc(2, 512, 1024, 13, 5)) == (10, SKINNY_NAME)
    for act in (0, 1, 5):
        d = _gate_desc(2, 512, 1024, 13, 5, act=act)
        d.res = d.y2 = d.x                                   # what FAC_ACT_WN_RES_SKIP needs; ignored by the others' check
        d.alpha_y2 = d.x if act != 5 else None
        assert ops.conv_variant(d)[0] == -1 and b"gate_cond" in lib.fac_last_error(), act
        assert lib.fac_conv1d_fwd(ctypes.byref(d), None) == -1 and b"gate_cond" in lib.fac_last_error(), act
    d = _gate_desc(2, 512, 1024, 13, 5)
    d.gate_cond_bs = -1
    assert ops.conv_variant(d)[0] == -1 and b"gate_cond" in lib.fac_last_error()


def test_oracle_causal_redecoder_against_reference_fixture(golden_dir):
    """The oracle's redecoder_forward(causal=True) and decoder_forward(causal=True, lstm=2) reproduce the real reference's causal
    voice-conversion path from committed data alone, at the 1e-5 tests/test_oracle_golden.py holds the non-causal one to
    (oracle_pinning_report.json: redecoder_oracle_rel, redecoder_decoder_oracle_rel); so do the errors the generator recorded."""
    from oracle import facodec_oracle as O
    from facodec_amd.commons import build_model
    d = np.load(os.path.join(golden_dir, "redecoder_causal.npz"))
    e2e = np.load(os.path.join(golden_dir, "codec_e2e.npz"))
    assert float(d["redecoder_causal_oracle_rel"]) < 1e-5 and float(d["redecoder_causal_decoder_oracle_rel"]) < 1e-5
    rm = build_model(_redecoder_params(), stage="redecoder")
    sd_re = synth.load_synthetic(rm.encoder, seed=0, prefix="redecoder.encoder.")
    sd_rd = synth.load_synthetic(rm.decoder, seed=0, prefix="redecoder.decoder.")
    codes_p, codes_c = (torch.from_numpy(e2e[k].astype(np.int64)) for k in ("codes_p", "codes_c"))
    tgt = torch.from_numpy(e2e["timbre"]).flip(0)
    with torch.no_grad():
        zr = O.redecoder_forward(sd_re, codes_p, codes_c, tgt, use_p_code=False, n_c=1, causal=True)
        yr = O.decoder_forward(sd_rd, zr, causal=True, lstm=2)
    assert d["z_probe"].shape == (2, 128, 160) and d["wave_probe"].shape == (2, len(d["probe_t"]))
    assert rel(zr[:, ::8], d["z_probe"]) < 1e-5
    assert rel(yr[:, 0, torch.from_numpy(d["probe_t"])], d["wave_probe"]) < 1e-5
    assert abs(float(yr.abs().max()) - float(d["wave_absmax"])) < 1e-4
    # the causal configuration is another function of the same codes than the non-causal fixture's
    assert rel(zr[:, ::8], np.load(os.path.join(golden_dir, "redecoder.npz"))["z_probe"]) > 1e-2


# ====================================================================================================================== kernel
# (C_in, C_out, K, T_out, kernel) at B = 2.  Which kernel a gated launch takes (conv1d_skinny.hip): the single-launch kernel at
# B * T_out <= 4 columns when a workgroup's 8 weight columns are at most 100 KB (C_in * K * 32 bytes), else the split reduction,
# whose gate needs C_out % 256 == 0.
#   (512, 1024, 5): the redecoder's in_layers; 80 KB per workgroup -> single launch at 2 and 4 columns, split reduction at 6
#   (16, 8, 5):     the smallest gate the single-launch kernel takes (8 output channels = one workgroup, 40 >= 24 reduction rows)
#   (1288, 256, 5): the smallest C_in (multiple of 8) whose k = 5 launch at <= 4 columns is a split reduction folded AND unfolded
#                   (C_in * K * 16 > 100 KB: the plain conv's 4-channel single-launch form does not take it either), at the
#                   fewest output channels the split reduction's gate accepts
GATE_CASES = [(512, 1024, 5, 1, GEMV_NAME), (512, 1024, 5, 2, GEMV_NAME), (512, 1024, 5, 3, SKINNY_NAME),
              (16, 8, 5, 1, GEMV_NAME), (16, 8, 5, 2, GEMV_NAME),
              (1288, 256, 5, 1, SKINNY_NAME), (1288, 256, 5, 2, SKINNY_NAME), (1288, 256, 5, 3, SKINNY_NAME)]


@gpu
@pytest.mark.parametrize("c_in,c_out,K,T_out,kernel", GATE_CASES,
                         ids=[f"{'gemv' if k == GEMV_NAME else 'split'}_{ci}x{co}k{kk}_T{t}" for ci, co, kk, t, k in GATE_CASES])
def test_conditioned_gate_epilogue_is_the_unfolded_pair(cuda, c_in, c_out, K, T_out, kernel):
    """ops.conv1d(act=ACT_GATE, gate_cond=g) == ops.conv1d -> ops.gate_tanh_sigmoid(a, g) bit for bit, two clips with their own
    rows, g a column slice of a wider tensor (batch stride 2H + 7, offset 3, neighbours 1e3); the launch is the kernel the case
    names; and against the fp64 restatement of the gate on the conv's fp32 output at the bar of
    tests/test_infer_kernels.py::test_gate_tanh_sigmoid_fp64 (4 e_cpu + 4 ulp at every element).  Without gate_cond the folded
    launch still equals the unconditioned pair."""
    from facodec_amd import ops
    from test_infer_kernels import _gate_ref
    from test_train_kernels_gen import _bar, _canary, _canary_intact
    B, H = 2, c_out // 2
    g = torch.Generator().manual_seed(c_in + 7 * T_out)
    x = torch.randn(B, c_in, T_out + K - 1, generator=g)
    w = torch.randn(c_out, c_in, K, generator=g) * (2.0 / (c_in * K) ** 0.5)
    bias = torch.randn(c_out, generator=g) * 0.3
    wide = torch.full((B, c_out + 7), 1e3)
    wide[:, 3:3 + c_out] = torch.randn(B, c_out, generator=g)
    assert not torch.equal(wide[0], wide[1])
    wide_d = wide.to(cuda)
    cond = wide_d[:, 3:3 + c_out]
    assert cond.stride(0) == c_out + 7
    x_d, b_d = x.to(cuda), bias.to(cuda)
    wp = ops.pack_conv_weight(w.to(cuda))
    kw = dict(bias=b_d, pad_left=0, pad_mode=ops.PAD_ZERO, t_out=T_out)
    names = []
    orig = ops._launch_conv

    def spy(d, what):
        orig(d, what)                       # first: the launch hands the descriptor its workspace, which the selection reads
        names.append(ops.conv_variant(d)[1])

    a = ops.conv1d(x_d, wp, c_out, K, **kw)
    want, want_plain = ops.gate_tanh_sigmoid(a, cond), ops.gate_tanh_sigmoid(a)
    out, buf, pad = _canary((B, H, T_out), cuda)
    ops._launch_conv = spy
    try:
        ops.conv1d(x_d, wp, c_out, K, act=ops.ACT_GATE, gate_cond=cond, out=out, **kw)
        got_plain = ops.conv1d(x_d, wp, c_out, K, act=ops.ACT_GATE, **kw)
    finally:
        ops._launch_conv = orig
    torch.cuda.synchronize()
    assert names == [kernel, kernel], names
    assert _canary_intact(buf, pad)
    assert torch.equal(out, want)
    assert torch.equal(got_plain, want_plain)
    assert not torch.equal(want, want_plain)
    assert torch.equal(wide_d.cpu(), wide) and torch.equal(x_d.cpu(), x)
    a_c, g_c = a.cpu(), wide[:, 3:3 + c_out]
    r64, r32 = _gate_ref(a_c, g_c, torch.float64), _gate_ref(a_c, g_c, torch.float32)
    _bar(f"conv_gate_cond_{c_in}x{c_out}k{K}_T{T_out}", out, r64, r32, scale=r64.abs().clamp_min(1e-300))
    with pytest.raises(ValueError, match="gate_cond"):
        ops.conv1d(x_d, wp, c_out, K, act=ops.ACT_GATE, gate_cond=wide_d[:, :c_out - 1], **kw)


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
def redecoders(cuda):
    """decoder_lstm -> the causal stage-'redecoder' model with the fixture's weights, built on first use."""
    from facodec_amd.commons import build_model
    made = {}

    def get(lstm):
        if lstm not in made:
            rm = build_model(_redecoder_params(lstm=lstm), stage="redecoder")
            for k in ("encoder", "decoder"):
                synth.load_synthetic(rm[k], seed=0, prefix="redecoder." + k + ".")
                rm[k].eval().to(cuda)
            made[lstm] = rm
        return made[lstm]
    return get


N_HOPS = 25
T_SHORT = 4800 + N_HOPS * 480          # 16 800 samples = 56 frames


@pytest.fixture(scope="module")
def offline(codec, cuda):
    """The whole-signal quantizer on the test signal, computed once: wave, timbre, codes [p (B, 1, T), c (B, 2, T), r]."""
    wave = synth.synth_clips(2, T_SHORT, seed=11).to(cuda)
    with torch.no_grad():
        _, _, _, _, timbre, codes = codec.quantizer(codec.encoder(wave), wave, n_c=2, return_codes=True)
    return wave, timbre, codes


def _keep(o):
    return {k: ([c.clone() for c in v] if isinstance(v, list) else (v.clone() if torch.is_tensor(v) else v)) for k, v in o.items()}


def _run(vc, wave, n_hops, finish=True, between=None):
    """prime + n_hops pushes (+ finish) -> the calls' outputs, copied; between(h) runs before push h."""
    with torch.no_grad():
        outs = [_keep(vc.prime(wave[:, :, :4800]))]
        for h in range(n_hops):
            if between is not None:
                between(h)
            outs.append(_keep(vc.push(wave[:, :, 4800 + h * 480: 4800 + (h + 1) * 480])))
        if finish:
            outs.append(_keep(vc.finish()))
    return outs


def _joined(outs):
    """-> (codes_p, codes_c, wave) concatenated over the calls; frame0 must run on without a gap."""
    frame, cp, cc, wv = 0, [], [], []
    for o in outs:
        if o["codes"] is None:
            assert o["wave"] is None
            continue
        assert o["frame0"] == frame
        assert len(o["codes"]) == 2 and o["wave"].shape[-1] == 300 * o["codes"][0].shape[-1]
        frame += o["codes"][0].shape[-1]
        cp.append(o["codes"][0])
        cc.append(o["codes"][1])
        wv.append(o["wave"])
    return torch.cat(cp, -1), torch.cat(cc, -1), torch.cat(wv, -1)


@gpu
@pytest.mark.parametrize("lstm", [0, 2])
@pytest.mark.parametrize("use_p_code,n_c,use_graphs", [(False, 1, True), (True, 2, False)])
def test_converter_matches_offline(codec, redecoders, offline, cuda, use_p_code, n_c, use_graphs, lstm):
    """480-sample hops == the offline path on the whole signal, per-stream targets timbre.flip(0): the emitted prosody and
    content codes equal the offline quantizer's, the concatenated wave is within E2E_TOL of redecoder.encoder(codes, target) ->
    redecoder.decoder, frame0 runs on without a gap and every frame of the signal comes out."""
    from facodec_amd.streaming import StreamingConverter
    wave, timbre, codes = offline
    rm = redecoders(lstm)
    tgt = timbre.flip(0).contiguous()
    with torch.no_grad():
        y = rm.decoder(rm.encoder(codes[0], codes[1], tgt, use_p_code=use_p_code, n_c=n_c))
    vc = StreamingConverter(codec, rm, tgt, use_p_code=use_p_code, n_c=n_c, use_graphs=use_graphs)
    cp, cc, wv = _joined(_run(vc, wave, N_HOPS))
    assert cp.shape[-1] == T_SHORT // 300 and wv.shape == y.shape == (2, 1, T_SHORT)
    assert torch.equal(cp, codes[0])
    assert cc.shape[1] == n_c and torch.equal(cc, codes[1][:, :n_c])
    e = rel(wv, y)
    print(f"[tol] converter_vs_offline p={use_p_code} n_c={n_c} graphs={use_graphs} lstm={lstm}: {e:.3e}")
    assert e < E2E_TOL


@gpu
def test_converter_matches_reference_fixture(codec, redecoders, cuda, golden_dir):
    """The two 2 s clips of codec_e2e.npz through a streaming session (graphs on, 90 hops), target = the other clip's timbre,
    use_p_code=False, n_c=1: the wave probes of the REAL reference's causal redecoder + decoder (decoder_lstm=2)."""
    from facodec_amd.streaming import StreamingConverter
    d = np.load(os.path.join(golden_dir, "redecoder_causal.npz"))
    e2e = np.load(os.path.join(golden_dir, "codec_e2e.npz"))
    wave = synth.synth_clips(2, 48000, seed=0).to(cuda)
    tgt = torch.from_numpy(e2e["timbre"]).flip(0).contiguous().to(cuda)
    vc = StreamingConverter(codec, redecoders(2), tgt)
    cp, cc, wv = _joined(_run(vc, wave, (48000 - 4800) // 480))
    assert wv.shape == (2, 1, 48000)
    assert torch.equal(cp.cpu(), torch.from_numpy(e2e["codes_p"].astype(np.int64)))
    assert torch.equal(cc.cpu(), torch.from_numpy(e2e["codes_c"].astype(np.int64))[:, :1])
    e = rel(wv[:, 0, torch.from_numpy(d["probe_t"]).to(cuda)], d["wave_probe"])
    print(f"[tol] converter_vs_reference wave_probe: {e:.3e}")
    assert e < E2E_TOL
    assert abs(float(wv.abs().max()) - float(d["wave_absmax"])) < 1e-4


@gpu
def test_converter_folded_epilogues_are_bit_identical(codec, redecoders, offline, cuda, monkeypatch):
    """The conditioned gate and the residual / skip adds as epilogues of the WaveNet's convs against the hop built from separate
    launches (ops.STREAM_FOLD = False): every code and every sample equal, graphs on, over three periods."""
    from facodec_amd import ops
    from facodec_amd.streaming import StreamingConverter
    wave, timbre, _ = offline
    tgt = timbre.flip(0).contiguous()
    n_hops = 15
    runs = []
    for fold in (False, True):
        monkeypatch.setattr(ops, "STREAM_FOLD", fold)
        runs.append(_run(StreamingConverter(codec, redecoders(2), tgt), wave[:, :, :4800 + n_hops * 480], n_hops))
    n_frames = 0
    for r, g in zip(*runs):
        assert r["frame0"] == g["frame0"] and (r["codes"] is None) == (g["codes"] is None)
        if r["codes"] is None:
            continue
        n_frames += r["codes"][0].shape[-1]
        for a, b in zip(r["codes"], g["codes"]):
            assert torch.equal(a, b)
        assert torch.equal(r["wave"], g["wave"])
    assert n_frames == (4800 + n_hops * 480) // 300


@gpu
def test_converter_set_target(codec, redecoders, offline, cuda):
    """set_target with the session's own timbre is a bit-for-bit no-op, during the capture period and under replayed graphs;
    another timbre changes the output from the next hop on and nothing before it; and with equal sources on both streams, a
    session with the targets swapped gives each stream the other's output (same function of the same inputs in the other batch
    slot: within E2E_TOL, the project's bar between two of its own evaluation orders -- while the two voices differ by far more).

    What "changes" is held to.  The target enters a hop through `cond` alone, so (i) a session switched to a target BEFORE its
    first chunk must equal, bit for bit, a session constructed with that target: set_target installs the new voice completely.
    (ii) A switch in mid-stream leaves the left contexts (16 WaveNet taps, the decoder's taps, its LSTM state) as the previous
    voice wrote them -- set_target's documented behaviour -- so the first hops after it are a blend and no size of the change
    follows from the model; what does follow is that the output is no longer the unswitched session's: it differs by more
    than E2E_TOL, the bar under which this project counts two outputs as the same.  (An earlier version of this test asked for
    1e-2 there, a figure with no derivation; the first hop after the switch measures 5.7e-3 on an MI355X with the synthetic
    weights, the steady-state difference of the two voices is above 1e-2.)"""
    from facodec_amd.streaming import StreamingConverter
    wave, timbre, _ = offline
    n_hops, switch = 13, 11
    wave = wave[:1, :, :4800 + n_hops * 480].expand(2, -1, -1).contiguous()            # the same source on both streams
    t01, t10 = timbre.contiguous(), timbre.flip(0).contiguous()
    rm = redecoders(2)
    base = _run(StreamingConverter(codec, rm, t01), wave, n_hops, finish=False)
    vc = StreamingConverter(codec, rm, t01)
    same = _run(vc, wave, n_hops, finish=False, between=lambda h: vc.set_target(t01.clone()) if h in (7, switch) else None)
    vc2 = StreamingConverter(codec, rm, t01)
    other = _run(vc2, wave, n_hops, finish=False, between=lambda h: vc2.set_target(t10) if h == switch else None)
    swapped = _run(StreamingConverter(codec, rm, t10), wave, n_hops, finish=False)
    vc3 = StreamingConverter(codec, rm, t01)
    vc3.set_target(t10)                                                     # before prime(): the whole session speaks as t10
    early = _run(vc3, wave, n_hops, finish=False)
    with pytest.raises(ValueError, match="timbre must be a float32 GPU tensor"):
        vc.set_target(t01[:1])
    changed = 0
    for i, (b, s, o, w, e) in enumerate(zip(base, same, other, swapped, early)):
        assert (b["wave"] is None) == (s["wave"] is None) == (o["wave"] is None) == (w["wave"] is None) == (e["wave"] is None)
        if b["wave"] is None:
            continue
        assert torch.equal(b["wave"], s["wave"]), i
        assert torch.equal(w["wave"], e["wave"]), i
        for x in (s, o, w):
            assert all(torch.equal(p, q) for p, q in zip(b["codes"], x["codes"])), i      # codes do not depend on the target
        if i <= switch:                         # call i is push i - 1: pushes 0 .. switch - 1 ran before the switch
            assert torch.equal(b["wave"], o["wave"]), i
        else:
            d = rel(o["wave"], b["wave"])
            print(f"[tol] set_target call {i}: switched vs unswitched {d:.3e}, switched vs t10 all along {rel(o['wave'], w['wave']):.3e}, "
                  f"the two voices {rel(b['wave'][:1], b['wave'][1:]):.3e}")
            assert d > E2E_TOL, i
            changed += 1
        assert rel(w["wave"].flip(0), b["wave"]) < E2E_TOL, i
        assert rel(b["wave"][:1], b["wave"][1:]) > 1e-2, i
    assert changed == n_hops - switch
