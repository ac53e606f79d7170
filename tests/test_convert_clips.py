"""Voice conversion of clip lists through the redecoder, non-causal included: fac_edge_tail / ops.edge_tail_,
commons.edge_plan and the two figures derived from it, Redecoder.forward_ragged / Decoder.forward_ragged, commons.redecode_clips
and commons.convert_clips.

Every clip of a right-padded batch must come out as the B = 1 calls give it alone, although the shipped redecoder's convs look
to the right.  The clips have 24, 22 and 11 frames and are handed over in the order (1, 2, 0): the longest shows a slack that is
too small, the 22-frame clip needs an edge that is written past the longest clip's end, the 11-frame clip an edge in the middle of
the tensor.  Weights: synth.load_synthetic(seed=0, prefix="redecoder.<key>."); codes and timbres are seeded draws.

E2E_TOL = 1e-4 relative max is the project's bar for waves and latents against the oracle and against the B = 1 path
(tests/test_ragged_batch.py); the CPU restatement of the scheme sits at 7e-6.
"""
import pytest
import torch

from facodec_amd import commons, synth

gpu = pytest.mark.gpu

E2E_TOL = 1e-4
FRAMES = (24, 22, 11)
ORDER = (1, 2, 0)              # the order the clip-list calls get the clips in: neither ascending nor descending
HOP = 300
SEED = 23
PAD_ZERO, PAD_REFLECT = 0, 1   # FAC_PAD_ZERO / FAC_PAD_REFLECT of include/facodec_hip.h
SRC_SAMPLES = (7200, 6750, 3301)   # 24, 22 and 11 frames, two of them no multiple of the hop
TGT_SAMPLES = (6000, 4650, 3900)


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def edge_write(x, lens, mul, n, mode):
    """The contract of fac_edge_tail (include/facodec_hip.h) by torch indexing, on a copy."""
    x = x.clone()
    T = x.shape[-1]
    for b, F in enumerate(lens):
        L = min(max(int(F) * mul, 0), T)
        for j in range(min(n, T - L)):
            s = L - 2 - j
            x[b, :, L + j] = x[b, :, s] if (mode == PAD_REFLECT and s >= 0) else 0.0
    return x


# ---------------------------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def O():
    from oracle import facodec_oracle
    return facodec_oracle


def _redecoder(causal):
    args = commons.default_redecoder_params()
    if causal:
        args.decoder_causal, args.decoder_lstm = True, 2
    rm = commons.build_model(args, stage="redecoder")
    sds = {}
    for k in ("encoder", "decoder"):
        sds[k] = {n: v.clone() for n, v in synth.load_synthetic(rm[k], seed=0, prefix="redecoder." + k + ".").items()}
        rm[k].eval()
    return rm, sds


@pytest.fixture(scope="module")
def shipped():
    """(the shipped, non-causal redecoder on the CPU, its state dicts on the CPU)."""
    return _redecoder(causal=False)


@pytest.fixture(scope="module")
def case():
    """Seeded codes [p (1, F), c (2, F)] and a timbre (1024,) per clip, on the host."""
    g = torch.Generator().manual_seed(SEED)
    return dict(codes=[[torch.randint(0, 1024, (1, F), generator=g), torch.randint(0, 1024, (2, F), generator=g)] for F in FRAMES],
                timbres=[torch.randn(1024, generator=g) for _ in FRAMES])


@pytest.fixture(scope="module")
def oracle_each(O, shipped, case):
    """[(latent (1, 1024, F), wave (1, 1, 300 F))] of the oracle on every clip alone: computed once, never modified."""
    sds = shipped[1]
    out = []
    with torch.no_grad():
        for (p, c), t in zip(case["codes"], case["timbres"]):
            z = O.redecoder_forward(sds["encoder"], p[None], c[None], t[None], causal=False)
            out.append((z, O.decoder_forward(sds["decoder"], z, causal=False, lstm=0)))
    return out


def _padded(case, Fp):
    """The three clips' codes padded with code 0 to Fp frames -> (p (3, 1, Fp), c (3, 2, Fp), timbre (3, 1024))."""
    pad = torch.nn.functional.pad
    p = torch.stack([pad(c[0], (0, Fp - c[0].shape[1])) for c in case["codes"]])
    c = torch.stack([pad(c[1], (0, Fp - c[1].shape[1])) for c in case["codes"]])
    return p, c, torch.stack(case["timbres"])


@pytest.fixture(scope="module")
def ops(cuda):
    from facodec_amd import ops as _ops
    from facodec_amd import _lib
    _lib.load()  # fails loudly if the extension is missing
    return _ops


@pytest.fixture(scope="module")
def shipped_gpu(shipped, cuda):
    rm = shipped[0]
    for k in ("encoder", "decoder"):
        rm[k].to(cuda)
    return rm


@pytest.fixture(scope="module")
def causal_gpu(cuda):
    rm = _redecoder(causal=True)[0]
    for k in ("encoder", "decoder"):
        rm[k].to(cuda)
    return rm


@pytest.fixture(scope="module")
def codec(cuda):
    model = commons.build_model(commons.default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(cuda)
    return model


def _single(rm, codes, timbre, **kw):
    """The existing forward on one clip alone (B = 1): -> (latent, wave)."""
    with torch.no_grad():
        z = rm.encoder(codes[0][None].contiguous(), codes[1][None].contiguous(), timbre[None].contiguous(), **kw)
        return z, rm.decoder(z)


# ------------------------------------------------------------------------------------------------------ 1. plan figures (CPU)
def test_edge_plan_of_the_shipped_and_the_causal_configuration(shipped):
    """The shipped redecoder: 16 WaveNet in_layers (2 columns, reflect, frame rate), decoder.model.0 (3), four blocks of
    [transposed conv (1, zero), k = 7 convs of dilation 1 / 3 / 9 (3, 9, 27, reflect)] at 6 / 30 / 150 / 300 columns per frame
    behind the transposed conv, decoder.model.6 (3 at 300): 16 + 1 + 4 * 4 + 1 = 34 entries, the 34 edge launches of a group."""
    plan = commons.edge_plan(shipped[0])
    want = [(f"encoder.encoder.in_layers.{i}", 1, 2, PAD_REFLECT) for i in range(16)] + [("decoder.model.0", 1, 3, PAD_REFLECT)]
    cols = 1
    for blk, s in zip((1, 2, 3, 4), (6, 5, 5, 2)):
        want.append((f"decoder.model.{blk}.block.1", cols, 1, PAD_ZERO))
        cols *= s
        want += [(f"decoder.model.{blk}.block.{u}.block.1", cols, 3 * d, PAD_REFLECT) for u, d in ((2, 1), (3, 3), (4, 9))]
    want.append(("decoder.model.6", 300, 3, PAD_REFLECT))
    assert plan == want and len(plan) == 34
    assert commons.ragged_slack_frames(shipped[0]) == 5 and commons.min_redecode_frames(shipped[0]) == 5
    causal = _redecoder(causal=True)[0]
    assert commons.edge_plan(causal) == []
    assert commons.ragged_slack_frames(causal) == 0 and commons.min_redecode_frames(causal) == 0


def test_edge_plan_refuses_a_non_causal_strided_conv():
    from facodec_amd.layers import SConv1d
    rm = commons.Munch(encoder=torch.nn.Sequential(SConv1d(4, 4, kernel_size=3, causal=False)),
                       decoder=torch.nn.Sequential(SConv1d(4, 4, kernel_size=3, causal=True),
                                                   SConv1d(4, 8, kernel_size=4, stride=2, causal=False)))
    with pytest.raises(NotImplementedError, match=r"decoder\.1"):
        commons.edge_plan(rm)
    rm.decoder[1].causal = True                                     # causal and strided: nothing to the right, no entry
    assert commons.edge_plan(rm) == [("encoder.0", 1, 1, PAD_REFLECT)]


def test_edge_tail_entry_validates_on_the_host():
    """fac_edge_tail rejects bad arguments before any launch (no GPU needed): error code and message."""
    import ctypes
    from facodec_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(0x10000)                                     # never dereferenced: every call below fails validation
    assert lib.fac_edge_tail(None, p, 1, 1, 8, 1, 2, PAD_REFLECT, None) == -1 and b"bad arguments" in lib.fac_last_error()
    assert lib.fac_edge_tail(p, None, 1, 1, 8, 1, 2, PAD_REFLECT, None) == -1 and b"bad arguments" in lib.fac_last_error()
    for B, C, T, mul, n in ((0, 1, 8, 1, 2), (1, 0, 8, 1, 2), (1, 1, 0, 1, 2), (1, 1, 8, 0, 2), (1, 1, 8, 1, 0)):
        assert lib.fac_edge_tail(p, p, B, C, T, mul, n, PAD_ZERO, None) == -1 and b"bad arguments" in lib.fac_last_error()
    assert lib.fac_edge_tail(p, p, 1, 1, 8, 1, 2, 7, None) == -1 and b"neither" in lib.fac_last_error()
    assert lib.fac_edge_tail(p, p, 1 << 16, 1 << 15, 8, 1, 2, PAD_ZERO, None) == -1 and b"32-bit" in lib.fac_last_error()
    assert lib.fac_edge_tail(ctypes.c_void_p(0x10002), p, 1, 1, 8, 1, 2, PAD_ZERO, None) == -1 and b"aligned" in lib.fac_last_error()


# ------------------------------------------------------------------------- 2. the plan is sufficient and necessary (CPU, oracle)
def _restated(O, sds, plan, p_code, c_code, timbre, lens):
    """Redecoder -> decoder layer by layer with the oracle's sconv1d / sconvtr1d / snake / conv_weight on a padded batch; in
    front of every conv that `plan` names, the pure-torch edge write of the entry.  -> (latent, wave)."""
    import torch.nn.functional as F
    rule = {name: (cols, n, mode) for name, cols, n, mode in plan}

    def edge(name, x):
        return edge_write(x, lens, *rule[name]) if name in rule else x

    def conv(sd, q, x, **kw):
        return O.sconv1d(x, O.conv_weight(sd, q), sd[q + "bias"], causal=False, **kw)

    sd, hidden = sds["encoder"], 512
    x = (F.embedding(p_code[:, 0], sd["prosody_embed.0.weight"]) + F.embedding(c_code[:, 0], sd["content_embed.0.weight"])
         + F.embedding(c_code[:, 1], sd["content_embed.1.weight"])).transpose(1, 2)
    g = conv(sd, "encoder.cond_layer.conv.conv.", timbre.unsqueeze(2))
    out = torch.zeros_like(x)
    for i in range(16):
        a = conv(sd, f"encoder.in_layers.{i}.conv.conv.", edge(f"encoder.encoder.in_layers.{i}", x)) + g[:, i * 2 * hidden:(i + 1) * 2 * hidden]
        rs = conv(sd, f"encoder.res_skip_layers.{i}.conv.conv.", torch.tanh(a[:, :hidden]) * torch.sigmoid(a[:, hidden:]))
        if i < 15:
            x, out = x + rs[:, :hidden], out + rs[:, hidden:]
        else:
            out = out + rs
    z = F.conv1d(out, sd["conv_out.weight"], sd["conv_out.bias"])

    sd = sds["decoder"]
    x = conv(sd, "model.0.conv.conv.", edge("decoder.model.0", z))
    for blk, s in zip((1, 2, 3, 4), (6, 5, 5, 2)):
        q = f"model.{blk}.block."
        x = O.snake(x, sd[q + "0.alpha"])
        x = O.sconvtr1d(edge(f"decoder.model.{blk}.block.1", x), O.conv_weight(sd, q + "1.convtr.convtr."), sd[q + "1.convtr.convtr.bias"],
                        s, causal=False)
        for u, d in ((2, 1), (3, 3), (4, 9)):
            r = f"{q}{u}.block."
            y = edge(f"decoder.model.{blk}.block.{u}.block.1", O.snake(x, sd[r + "0.alpha"]))
            y = O.snake(conv(sd, r + "1.conv.conv.", y, dilation=d), sd[r + "2.alpha"])
            x = x + conv(sd, r + "3.conv.conv.", y)
    x = edge("decoder.model.6", O.snake(x, sd["model.5.alpha"]))
    return z, torch.tanh(conv(sd, "model.6.conv.conv.", x))


def _errors(got, oracle_each):
    """[(latent error, wave error)] of every clip's own part of a padded batch's (latent, wave)."""
    z, y = got
    return [(rel(z[b:b + 1, :, :F], oracle_each[b][0]), rel(y[b:b + 1, :, :HOP * F], oracle_each[b][1])) for b, F in enumerate(FRAMES)]


def test_edge_plan_is_sufficient_and_necessary_on_the_oracle(O, shipped, case, oracle_each):
    """On the CPU, in the oracle's arithmetic: with every edge of edge_plan written and ragged_slack_frames of slack, every clip of
    the padded batch is the oracle's result on that clip alone; with one slack frame less the longest clip is not; without the
    zero entries no clip is; and the oracle's own whole-batch forward on the zero-padded codes misses the two shorter clips.
    (Measured: 7e-6 at most in the first case; 0.35, 0.8 .. 1.25 and 1.2 wave error in the others -- DESIGN.md 23.3.)"""
    rm, sds = shipped
    plan, slack = commons.edge_plan(rm), commons.ragged_slack_frames(rm)
    with torch.no_grad():
        full = _errors(_restated(O, sds, plan, *_padded(case, FRAMES[0] + slack), FRAMES), oracle_each)
        print("edges written, slack", slack, ":", full)
        assert all(max(e) < E2E_TOL for e in full), full

        short = _errors(_restated(O, sds, plan, *_padded(case, FRAMES[0] + slack - 1), FRAMES), oracle_each)
        print("slack", slack - 1, ":", short)
        assert short[0][1] > E2E_TOL, short

        no_zero = _errors(_restated(O, sds, [e for e in plan if e[3] != PAD_ZERO], *_padded(case, FRAMES[0] + slack), FRAMES), oracle_each)
        print("zero entries dropped:", no_zero)
        assert all(e[1] > E2E_TOL for e in no_zero), no_zero

        p, c, t = _padded(case, FRAMES[0])
        z = O.redecoder_forward(sds["encoder"], p, c, t, causal=False)
        plain = _errors((z, O.decoder_forward(sds["decoder"], z, causal=False, lstm=0)), oracle_each)
        print("whole-batch oracle forward on the zero-padded codes:", plain)
        assert all(min(e) > E2E_TOL for e in plain[1:]), plain


# -------------------------------------------------------------------------------------------------- 3. the kernel (GPU, exact)
def _edge_case(ops, cuda, C, T, lens, mul, n, mode):
    g = torch.Generator().manual_seed(SEED + C + T + n)
    buf = torch.randn(len(lens) + 2, C, T, generator=g)             # a row in front and one behind: they must not move either
    want = buf.clone()
    want[1:-1] = edge_write(buf[1:-1], lens, mul, n, mode)
    dev = buf.to(cuda)
    x = dev[1:-1]
    assert x.is_contiguous()
    got = ops.edge_tail_(x, torch.tensor(lens, dtype=torch.int32).to(cuda), mul, n, mode)
    torch.cuda.synchronize()
    assert got.data_ptr() == x.data_ptr()
    assert torch.equal(dev.cpu(), want)
    return want


@gpu
@pytest.mark.parametrize("mode", [PAD_ZERO, PAD_REFLECT], ids=["zero", "reflect"])
@pytest.mark.parametrize("mul,T,n", [(1, 64, 27), (6, 384, 27), (6, 384, 162)])
@pytest.mark.parametrize("C", [1, 5, 96])
def test_edge_tail_matches_torch_indexing(ops, cuda, C, mul, T, n, mode):
    """ops.edge_tail_ against the contract by torch indexing, torch.equal on the whole tensor and its neighbours: lens * mul =
    (T, T - 14 mul, 28 mul) -- nothing for clip 0; clip 1 has 14 mul columns behind it (clamped where n is larger: (1, 64, 27) and
    (6, 384, 162)); clip 2 is L = n + 1 at (1, 64, 27), the smallest legal clip."""
    lens = (64, 50, 28)
    want = _edge_case(ops, cuda, C, T, lens, mul, n, mode)
    assert T == 64 * mul and 28 * mul >= n + 1
    if mode == PAD_REFLECT and mul == 1:
        assert torch.equal(want[2, :, 50:64], want[2, :, 35:49].flip(-1))       # the reference itself: reflection about column 49


@gpu
@pytest.mark.parametrize("mode", [PAD_ZERO, PAD_REFLECT], ids=["zero", "reflect"])
@pytest.mark.parametrize("lens,n", [((0, 1, 2), 2), ((70, -3, 5), 9)])
def test_edge_tail_short_and_out_of_range_lengths(ops, cuda, lens, n, mode):
    """Clips shorter than the reflection (sources in front of the clip give zeros, nothing traps) and lengths outside [0, T]
    (clamped)."""
    want = _edge_case(ops, cuda, 5, 64, lens, 1, n, mode)
    if lens == (0, 1, 2):
        assert not want[1, :, :2].any() and not want[2, :, 1:3].any()           # L = 0: zeros; L = 1: sources -1, -2
        if mode == PAD_REFLECT:
            assert torch.equal(want[3, :, 2], want[3, :, 0]) and not want[3, :, 3].any()


@gpu
def test_edge_tail_refuses_what_mask_tail_refuses(ops, cuda):
    from facodec_amd._lib import FacodecHipError
    lens = torch.tensor([3, 2], dtype=torch.int32).to(cuda)
    x = torch.zeros(2, 4, 8, device=cuda)
    for bad in (torch.zeros(2, 4, 8), x.half(), x.transpose(1, 2), x[:, :, ::2]):
        with pytest.raises(FacodecHipError):
            ops.edge_tail_(bad, lens, 1, 2, PAD_REFLECT)
    with pytest.raises(FacodecHipError):
        ops.edge_tail_(x, lens.cpu(), 1, 2, PAD_REFLECT)
    with pytest.raises(FacodecHipError, match="neither"):
        ops.edge_tail_(x, lens, 1, 2, 7)
    assert not x.any()


# ------------------------------------------------------------------------------------------- 4. the ragged forwards (GPU)
@gpu
def test_forward_ragged_matches_each_clip_alone_and_the_oracle(shipped_gpu, case, oracle_each, cuda):
    """Redecoder.forward_ragged -> Decoder.forward_ragged on the padded batch: every clip within E2E_TOL of the existing forward
    on that clip alone (B = 1) and of the oracle, latent and wave; the existing forward on the zero-padded batch is not (the
    22-frame clip); the ragged calls refuse .train()."""
    rm = shipped_gpu
    Fp = FRAMES[0] + commons.ragged_slack_frames(rm)
    p, c, t = (x.to(cuda) for x in _padded(case, Fp))
    lens = torch.tensor(FRAMES, dtype=torch.int32).to(cuda)
    with torch.no_grad():
        z = rm.encoder.forward_ragged(p, c, t, lens)
        z_kept = z.clone()
        y = rm.decoder.forward_ragged(z, lens)
        torch.cuda.synchronize()
        assert z.shape == (3, 1024, Fp) and y.shape == (3, 1, HOP * Fp)
        for b, F in enumerate(FRAMES):
            assert torch.equal(z[b, :, :F], z_kept[b, :, :F])                    # only the tails of the caller's latent are written
            one_z, one_y = _single(rm, [x.to(cuda) for x in case["codes"][b]], case["timbres"][b].to(cuda))
            errs = dict(latent_b1=rel(z[b:b + 1, :, :F], one_z), wave_b1=rel(y[b:b + 1, :, :HOP * F], one_y),
                        latent_oracle=rel(z[b:b + 1, :, :F], oracle_each[b][0]), wave_oracle=rel(y[b:b + 1, :, :HOP * F], oracle_each[b][1]))
            print(F, "frames:", errs)
            assert max(errs.values()) < E2E_TOL, (F, errs)
        p0, c0, t0 = (x.to(cuda) for x in _padded(case, FRAMES[0]))
        y0 = rm.decoder(rm.encoder(p0, c0, t0))
        miss = rel(y0[1:2, :, :HOP * FRAMES[1]], oracle_each[1][1])
        print("existing forward on the zero-padded batch, 22-frame clip:", miss)
        assert miss > E2E_TOL
    for k in ("encoder", "decoder"):
        rm[k].train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            rm.encoder.forward_ragged(p, c, t, lens)
        with pytest.raises(RuntimeError, match="eval"):
            rm.decoder.forward_ragged(z_kept, lens)
    finally:
        for k in ("encoder", "decoder"):
            rm[k].eval()


# --------------------------------------------------------------------------------------------- 5. redecode_clips, causal (GPU)
@gpu
def test_redecode_clips_causal_makes_no_edge_launch(causal_gpu, case, cuda, ops, monkeypatch):
    """The causal redecoder (decoder_causal=True, decoder_lstm=2): no slack, no fac_edge_tail launch, every clip within E2E_TOL
    of the B = 1 path."""
    def refuse(*a, **kw):
        raise AssertionError("a causal redecoder must not launch fac_edge_tail")
    monkeypatch.setattr(ops, "edge_tail_", refuse)
    codes = [[x.to(cuda) for x in case["codes"][i]] for i in ORDER]
    timbres = [case["timbres"][i].to(cuda) for i in ORDER]
    waves = commons.redecode_clips(causal_gpu, codes, timbres)
    torch.cuda.synchronize()
    for j, i in enumerate(ORDER):
        one = _single(causal_gpu, codes[j], timbres[j], use_p_code=False, n_c=1)[1]
        assert waves[j].shape == (1, HOP * FRAMES[i])
        err = rel(waves[j], one[0])
        print(FRAMES[i], "frames:", err)
        assert err < E2E_TOL, (FRAMES[i], err)


@gpu
def test_redecode_clips_shipped_matches_each_clip_alone(shipped_gpu, case, cuda):
    """The shipped non-causal redecoder through the public call, clips in ORDER, and in two groups under a small budget."""
    codes = [[x.to(cuda) for x in case["codes"][i]] for i in ORDER]
    timbres = [case["timbres"][i].to(cuda) for i in ORDER]
    for budget in (commons.MAX_BATCH_SAMPLES, 2 * HOP * (FRAMES[1] + 5)):
        waves = commons.redecode_clips(shipped_gpu, codes, timbres, use_p_code=True, n_c=2, max_batch_samples=budget)
        for j, i in enumerate(ORDER):
            one = _single(shipped_gpu, codes[j], timbres[j])[1]
            assert waves[j].shape == (1, HOP * FRAMES[i])
            assert rel(waves[j], one[0]) < E2E_TOL, (budget, FRAMES[i], rel(waves[j], one[0]))


# ------------------------------------------------------------------------------------------------ 6. convert_clips (GPU)
@pytest.fixture(scope="module")
def speech(cuda):
    """(sources, targets): host clips (1, T) of SRC_SAMPLES / TGT_SAMPLES samples, in the clips' own order."""
    s = synth.synth_clips(3, SRC_SAMPLES[0], seed=SEED)
    t = synth.synth_clips(3, TGT_SAMPLES[0], seed=SEED + 1)
    return ([s[i, :, :n].clone() for i, n in enumerate(SRC_SAMPLES)], [t[i, :, :n].clone() for i, n in enumerate(TGT_SAMPLES)])


@pytest.fixture(scope="module")
def converted(codec, shipped_gpu, speech, cuda):
    """convert_clips on the clips in ORDER (target i with source i), computed once."""
    src = [speech[0][i].to(cuda) for i in ORDER]
    tgt = [speech[1][i].to(cuda) for i in ORDER]
    waves = commons.convert_clips(codec, shipped_gpu, src, tgt)
    torch.cuda.synchronize()
    return src, tgt, waves


@gpu
def test_convert_clips_end_to_end(codec, shipped_gpu, converted, cuda):
    """Shapes and order; every wave within E2E_TOL of the B = 1 redecoder path on the encode_clips codes of its source and the
    encode_clips timbre of its target (the same codes on both sides: near-tie code flips are the existing ragged tests'
    business); a single target for all clips equals the list form; exchanging two targets is audible."""
    src, tgt, waves = converted
    enc_s, enc_t = commons.encode_clips(codec, src, n_c=2), commons.encode_clips(codec, tgt, n_c=2)
    assert len(waves) == 3
    for j, i in enumerate(ORDER):
        assert waves[j].shape == (1, HOP * FRAMES[i])
        one = _single(shipped_gpu, enc_s[j]["codes"], enc_t[j]["timbre"], use_p_code=False, n_c=1)[1]
        err = rel(waves[j], one[0])
        print(FRAMES[i], "frames:", err)
        assert err < E2E_TOL, (FRAMES[i], err)
    alone = commons.convert_clips(codec, shipped_gpu, src, tgt[0])
    listed = commons.convert_clips(codec, shipped_gpu, src, [tgt[0]] * 3)
    one_list = commons.convert_clips(codec, shipped_gpu, src, [tgt[0]])
    for a, b, c in zip(alone, listed, one_list):
        assert rel(a, b) < E2E_TOL and rel(c, b) < E2E_TOL
    swapped = commons.convert_clips(codec, shipped_gpu, src, [tgt[1], tgt[0], tgt[2]])
    assert rel(swapped[0], waves[0]) > E2E_TOL and rel(swapped[1], waves[1]) > E2E_TOL
    assert rel(swapped[2], waves[2]) < E2E_TOL


# ------------------------------------------------------------------------------------------------ 7. another sample rate (GPU)
@gpu
def test_convert_clips_at_16_khz(codec, shipped_gpu, ops, cuda):
    """sample_rate=16000 against the same steps by hand: ops.resample per clip -> convert_clips at 24 kHz -> ops.resample per clip.
    The sources have 4800 / 4500 / 2201 samples at 16 kHz = 7200 / 6750 / 3302 at 24 kHz (24, 22 and 11 frames)."""
    s = synth.synth_clips(3, 4800, seed=SEED + 2)
    t = synth.synth_clips(3, 4000, seed=SEED + 3)
    src = [s[i, :, :n].to(cuda).contiguous() for i, n in zip(ORDER, (4500, 2201, 4800))]
    tgt = [t[i, :, :n].to(cuda).contiguous() for i, n in zip(ORDER, (3100, 2600, 4000))]
    got = commons.convert_clips(codec, shipped_gpu, src, tgt, sample_rate=16000)
    up = lambda ws: [ops.resample(w, 16000, 24000) for w in ws]
    by_hand = [ops.resample(w.contiguous(), 24000, 16000) for w in commons.convert_clips(codec, shipped_gpu, up(src), up(tgt))]
    for j, i in enumerate(ORDER):
        assert got[j].shape == (1, -(-HOP * FRAMES[i] * 16000 // 24000))
        assert got[j].shape == by_hand[j].shape
        err = rel(got[j], by_hand[j])
        print(FRAMES[i], "frames:", err)
        assert err < E2E_TOL, (FRAMES[i], err)


# ----------------------------------------------------------------------------------------------------------- 8. errors (GPU)
@gpu
def test_errors_are_raised_on_the_host_before_any_launch(codec, shipped_gpu, case, speech, cuda, ops, monkeypatch):
    from facodec_amd._lib import FacodecHipError
    rm = shipped_gpu

    def no_launch(*a, **kw):
        raise AssertionError("launched before the arguments were checked")
    monkeypatch.setattr(ops, "edge_tail_", no_launch)
    monkeypatch.setattr(ops, "embed_sum", no_launch)
    codes = [[x.to(cuda) for x in c] for c in case["codes"]]
    timbres = [t.to(cuda) for t in case["timbres"]]
    need = commons.min_redecode_frames(rm)
    assert need == 5
    with pytest.raises(ValueError, match=r"clip 1 has 4 frames.* 5 frames"):
        commons.redecode_clips(rm, [codes[0], [x[:, :4] for x in codes[1]], codes[2]], timbres)
    assert commons.redecode_clips(rm, [], []) == []
    with pytest.raises(ValueError, match="3 clips but 2 timbres"):
        commons.redecode_clips(rm, codes, timbres[:2])
    with pytest.raises(ValueError, match="quantizer counts"):
        commons.redecode_clips(rm, [codes[0], [codes[1][0], codes[1][1][:1]], codes[2]], timbres)
    with pytest.raises(ValueError, match=r"n_c = 3.* 2 content tables"):
        commons.redecode_clips(rm, codes, timbres, n_c=3)
    with pytest.raises(ValueError, match=r"n_c = 2 but the clips carry 1 content"):
        commons.redecode_clips(rm, [[c[0], c[1][:1]] for c in codes], timbres, n_c=2)
    with pytest.raises(FacodecHipError):
        commons.redecode_clips(rm, [[x.cpu() for x in c] for c in codes], timbres)
    with pytest.raises(FacodecHipError):
        commons.redecode_clips(rm, codes, [t.cpu() for t in timbres])
    src, tgt = ([w.to(cuda) for w in ws] for ws in speech)
    with pytest.raises(ValueError, match="3 sources but 2 targets"):
        commons.convert_clips(codec, rm, src, tgt[:2])
    with pytest.raises(ValueError, match=r"n_c = 3.* 2 content tables"):
        commons.convert_clips(codec, rm, src, tgt, n_c=3)
    with pytest.raises(FacodecHipError):
        commons.convert_clips(codec, rm, [w.cpu() for w in src], tgt)
