"""Training of the voice-conversion redecoder (train_redecoder.py:195-328) on the HIP path.

* the whole RedecoderTrainStep against tests/golden/redecoder_train.npz, made by tests/golden/make_golden_redecoder_train.py from
  the real reference (dropout p = 0, recorded crop starts), at the bars of tests/test_train_golden.py;
* each new backward against a float64 torch restatement written out in this file: the non-causal ConvTranspose1d (strides 2, 5, 6
  and the decoder's real channel counts), the conditioned non-causal WaveNet, the code-embedding scatter (also bit-identical
  across runs), a non-causal reflect-padded ResidualUnit at and above the short-signal guard of fac_pad_fold_edges;
* redecoder inference after a .train() / .eval() round trip still equals tests/golden/redecoder.npz.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from facodec_amd import synth

LOSS_TOL = 1e-5
NORM_TOL = 2e-4
PROBE_BAR = dict(encoder=5e-4, decoder=5e-4, discriminator=3e-3)
SCALARS = dict(loss_d="loss_d", loss_gen_all="loss_gen_all", mel_loss="mel", loss_g="loss_g", loss_feature="feature",
               stft_loss="stft", waveform_loss="waveform")


def _fixture(golden_dir):
    d = np.load(os.path.join(golden_dir, "redecoder_train.npz"))
    return {k: d[k] for k in d.files}


def probe_index(numel, n=64):
    step = max(1, numel // n)
    return np.arange(0, numel, step)[:n]


def _wn(v, g):
    """weight_norm over dim 0 in float64."""
    return g * v / v.reshape(v.shape[0], -1).norm(dim=1).reshape(-1, *([1] * (v.dim() - 1)))


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------------------- CPU checks
def test_fixture_is_consistent(golden_dir):
    """The fixture's inputs describe one train_redecoder.py crop: seg = min(min(mel lengths), 80), starts inside every clip, the
    20-frame segment above fac_pad_fold_edges' short-signal guard for every reflect-padded conv of the decoder (T > 55 at d = 9)."""
    fx = _fixture(golden_dir)
    mel = [int(n) for n in fx["mel_input_length"]]
    seg = int(fx["seg_frames"])
    assert seg == min(min(mel), 80) == 20
    for n, s, w in zip(mel, fx["crop_start"], fx["wave_lens"]):
        assert 0 <= s and (s < n - seg or (s == 0 and n == seg)) and n == int(w) // 300
    assert fx["codes_p"].shape == (4, 1, seg) and fx["codes_c"].shape == (4, 2, seg) and fx["timbre"].shape == (4, 1024)
    assert seg * 6 > 55
    assert json.loads(str(fx["params_without_grad"])) == {"encoder": [], "decoder": []}


def test_discriminator_keys_cover_the_fixture(golden_dir):
    from facodec_amd.train_redecoder import redecoder_discriminator
    names = {n for n, _ in redecoder_discriminator().named_parameters()}
    fx = _fixture(golden_dir)
    probed = {k[len("grad.discriminator."):-len(".norm")] for k in fx if k.startswith("grad.discriminator.") and k.endswith(".norm")}
    assert probed and probed <= names


# ------------------------------------------------------------------------------------------------------------- whole step
def _models(cuda):
    from facodec_amd.commons import build_model, default_redecoder_params
    from facodec_amd.train_redecoder import redecoder_discriminator
    args = default_redecoder_params()
    codec = build_model(args, stage="encoder")
    model = build_model(args, stage="redecoder")
    synth.load_synthetic(codec.encoder, seed=0, prefix="encoder.encoder.")
    synth.load_synthetic(codec.quantizer, seed=0, prefix="encoder.quantizer.")
    synth.load_synthetic(model.encoder, seed=0, prefix="redecoder.encoder.")
    synth.load_synthetic(model.decoder, seed=0, prefix="redecoder.decoder.")
    disc = redecoder_discriminator()
    synth.load_synthetic(disc, seed=0, prefix="discriminator.")
    for m in (codec.encoder, codec.quantizer, model.encoder, model.decoder, disc):
        m.to(cuda)
    return codec, model, disc


@pytest.mark.gpu
def test_redecoder_train_step_against_reference_golden(cuda, golden_dir):
    """RedecoderTrainStep against the reference's own iteration: codes bit-exact and timbre of the frozen codec, 7 loss scalars at
    1e-5, the three pre-clip key norms and ~30 per-tensor gradient norms at 2e-4, gradient probes per key (generator 5e-4,
    discriminator 3e-3 -- the bars of tests/test_train_golden.py, whose comment gives the measured conditioning of this kind of
    loss), no parameter without gradient, discriminator weights after its AdamW step."""
    from facodec_amd.train_redecoder import RedecoderTrainStep
    fx = _fixture(golden_dir)
    codec, model, disc = _models(cuda)
    step = RedecoderTrainStep(model, codec, disc, dropout=False)
    out = step(torch.from_numpy(fx["waves"]).to(cuda), torch.from_numpy(fx["wave_lens"]).to(torch.int64).to(cuda),
               [int(n) for n in fx["mel_input_length"]], starts=torch.from_numpy(fx["crop_start"]).to(torch.int64))
    torch.cuda.synchronize()
    for i, k in enumerate(("codes_p", "codes_c", "codes_r")):
        assert np.array_equal(out["codes"][i].cpu().numpy(), fx[k].astype(np.int64)), k
    report = {"timbre_rel": _rel(out["timbre"], torch.from_numpy(fx["timbre"])), "loss_rel": {}, "grad_norm_rel": {}, "worst": {}}
    for k, o in SCALARS.items():
        report["loss_rel"][k] = abs(float(out[o]) - float(fx[k])) / abs(float(fx[k]))
    params = {"encoder": dict(model.encoder.named_parameters()), "decoder": dict(model.decoder.named_parameters()),
              "discriminator": dict(disc.named_parameters())}
    for key in params:
        report["grad_norm_rel"][key] = abs(float(out["grad_norm"][key]) - float(fx[f"grad_norm64_{key}"])) / float(fx[f"grad_norm64_{key}"])
        worst = {"norm": ("", 0.0), "probe": ("", 0.0)}
        pre = f"grad.{key}."
        for name in sorted(k[len(pre):-len(".norm")] for k in fx if k.startswith(pre) and k.endswith(".norm")):
            g = params[key][name].grad.detach().cpu().reshape(-1)
            ref_norm, ref_probe = float(fx[f"{pre}{name}.norm"]), fx[f"{pre}{name}.probe"]
            e_norm = abs(float(g.double().norm()) - ref_norm) / max(ref_norm, 1e-30)
            if f"{pre}{name}.probe_rows" in fx:            # embedding tables: every 64th channel of the rows the codes select
                rows = torch.from_numpy(fx[f"{pre}{name}.probe_rows"].astype(np.int64))
                got = params[key][name].grad.detach().cpu()[rows][:, ::64].reshape(-1).numpy()
            else:
                got = g[probe_index(g.numel())].numpy()
            e_probe = float(np.abs(got - ref_probe).max() / max(np.abs(ref_probe).max(), 1e-30))
            if e_norm > worst["norm"][1]:
                worst["norm"] = (name, e_norm)
            if e_probe > worst["probe"][1]:
                worst["probe"] = (name, e_probe)
        report["worst"][key] = worst
    if os.environ.get("FAC_REPORT_DIR"):
        os.makedirs(os.environ["FAC_REPORT_DIR"], exist_ok=True)
        json.dump(report, open(os.path.join(os.environ["FAC_REPORT_DIR"], "redecoder_train_report.json"), "w"), indent=1)
    print(json.dumps(report))
    assert report["timbre_rel"] < 1e-4, report["timbre_rel"]
    for k, e in report["loss_rel"].items():
        assert e < LOSS_TOL, (k, e)
    for k, e in report["grad_norm_rel"].items():
        assert e < NORM_TOL, (k, e)
    for k, w in report["worst"].items():
        assert w["norm"][1] < NORM_TOL and w["probe"][1] < PROBE_BAR[k], (k, w)
    for k in ("encoder", "decoder"):
        assert step.opt[k].params_without_grad() == [], k
    for key in fx:
        if key.startswith("param_after.discriminator."):
            n = key[len("param_after.discriminator."):-len(".probe")]
            flat = params["discriminator"][n].detach().cpu().reshape(-1)
            assert np.abs(flat[probe_index(flat.numel())].numpy() - fx[key]).max() < 2e-6, n


@pytest.mark.gpu
def test_redecoder_inference_after_train_eval_round_trip(cuda, golden_dir):
    """A .train() / .eval() round trip leaves the inference path as it was: tests/golden/redecoder.npz at the bars of
    tests/test_gpu_parity.py::test_redecoder_vs_reference_golden."""
    from facodec_amd.commons import build_model, default_model_params, default_redecoder_params
    d = np.load(os.path.join(golden_dir, "redecoder.npz"))
    m = build_model(default_model_params())
    for k in ("encoder", "quantizer"):
        synth.load_synthetic(m[k], seed=0, prefix=k + ".")
        m[k].eval().to(cuda)
    rm = build_model(default_redecoder_params(), stage="redecoder")
    for k in ("encoder", "decoder"):
        synth.load_synthetic(rm[k], seed=0, prefix="redecoder." + k + ".")
        rm[k].to(cuda).train()
        rm[k].eval()
    wave = synth.synth_clips(2, 48000, seed=0).to(cuda)
    with torch.no_grad():
        z = m.encoder(wave)
        _, _, _, _, timbre, codes = m.quantizer(z, wave, n_c=2, return_codes=True)
        zr = rm.encoder(codes[0], codes[1], timbre.flip(0), use_p_code=False, n_c=1)
        yr = rm.decoder(zr)
    assert _rel(zr[:, ::8], torch.from_numpy(d["z_probe"])) < 1e-4
    assert _rel(yr[:, 0, torch.from_numpy(d["probe_t"]).to(cuda)], torch.from_numpy(d["wave_probe"])) < 1e-4
    assert abs(float(yr.abs().max()) - float(d["wave_absmax"])) < 1e-4


# ------------------------------------------------------------------------------------------------------------- single ops vs fp64
@pytest.mark.gpu
@pytest.mark.parametrize("c_in,c_out,s,B,T", [(64, 32, 2, 2, 300), (64, 64, 5, 2, 300), (96, 64, 6, 3, 100), (192, 96, 2, 16, 4096),
                                              (768, 384, 5, 4, 480), (1536, 768, 6, 4, 80)])
def test_noncausal_convtr_backward_against_fp64(cuda, c_in, c_out, s, B, T):
    """Non-causal SConvTranspose1d (kernel 2 s, weight-normed): torch's ConvTranspose1d in float64 with ceil(s/2) columns trimmed on
    the left and floor(s/2) on the right.  (1536, 768, 6) at 80 frames and (768, 384, 5) are the decoder's first two layers at the
    reference's B = 4 x 80 crop; (192, 96, 2) at B = 16 takes the streaming kernel with taps."""
    from facodec_amd import autograd as A
    from facodec_amd.layers import SConvTranspose1d
    m = SConvTranspose1d(c_in, c_out, 2 * s, stride=s, causal=False, norm="weight_norm")
    synth.load_synthetic(m, seed=s, prefix=f"convtr{c_in}.")
    m.to(cuda)
    gen = torch.Generator().manual_seed(c_in + s)
    x = torch.randn(B, c_in, T, generator=gen)
    r = torch.randn(B, c_out, T * s, generator=gen)
    xg = x.to(cuda).requires_grad_()
    y = A.conv_tr(m, xg)
    (y * r.to(cuda)).sum().backward()
    w = m.w
    leaves = {n: t.detach().cpu().double().requires_grad_() for n, t in (("v", w.weight_v), ("g", w.weight_g), ("b", w.bias))}
    x64 = x.double().requires_grad_()
    full = F.conv_transpose1d(x64, _wn(leaves["v"], leaves["g"]), leaves["b"], stride=s)
    y64 = full[..., s - s // 2: full.shape[-1] - s // 2]
    assert y64.shape[-1] == T * s
    (y64 * r.double()).sum().backward()
    assert _rel(y, y64) < 1e-5
    for got, ref in ((xg.grad, x64.grad), (w.weight_v.grad, leaves["v"].grad), (w.weight_g.grad, leaves["g"].grad),
                     (w.bias.grad, leaves["b"].grad)):
        assert got.shape == ref.shape
        assert _rel(got, ref) < 1e-5, (got.shape, _rel(got, ref))


def _sconv64(sd, pre, x, k, dilation=1):
    """Non-causal reflect-padded weight-normed SConv1d (stride 1) in float64."""
    pad = (k - 1) * dilation
    if pad:
        x = F.pad(x, (pad - pad // 2, pad // 2), mode="reflect")
    return F.conv1d(x, _wn(sd[pre + ".conv.conv.weight_v"], sd[pre + ".conv.conv.weight_g"]), sd[pre + ".conv.conv.bias"], dilation=dilation)


@pytest.mark.gpu
def test_conditioned_wavenet_backward_against_fp64(cuda):
    """WN(hidden 64, k 5, 4 layers, gin 128, non-causal) in training mode with a conditioning vector g: every parameter gradient
    (cond_layer included) and the input gradient against modules/wavenet.py:138-166 restated in float64; g gets no gradient."""
    from facodec_amd import autograd_quant as AQ
    from facodec_amd.quantize import WN
    H, L, GIN, B, T = 64, 4, 128, 3, 150
    m = WN(hidden_channels=H, kernel_size=5, dilation_rate=1, n_layers=L, gin_channels=GIN, p_dropout=0.0, causal=False)
    synth.load_synthetic(m, seed=3, prefix="wn.")
    m.to(cuda)
    gen = torch.Generator().manual_seed(11)
    x, g, r = torch.randn(B, H, T, generator=gen), torch.randn(B, GIN, generator=gen), torch.randn(B, H, T, generator=gen)
    xg = x.to(cuda).requires_grad_()
    gg = g.to(cuda)
    out = AQ.wavenet(m, xg, use_dropout=False, g=gg)
    (out * r.to(cuda)).sum().backward()
    sd = {n: p.detach().cpu().double().requires_grad_() for n, p in m.named_parameters()}
    x64 = x.double().requires_grad_()
    cond = _sconv64(sd, "cond_layer", g.double().unsqueeze(-1), 1)
    h, o = x64, torch.zeros_like(x64)
    for i in range(L):
        xin = _sconv64(sd, f"in_layers.{i}", h, 5) + cond[:, 2 * H * i: 2 * H * (i + 1)]
        acts = torch.tanh(xin[:, :H]) * torch.sigmoid(xin[:, H:])
        rs = _sconv64(sd, f"res_skip_layers.{i}", acts, 1)
        if i < L - 1:
            h = h + rs[:, :H]
            o = o + rs[:, H:]
        else:
            o = o + rs
    (o * r.double()).sum().backward()
    assert _rel(out, o) < 1e-5
    assert _rel(xg.grad, x64.grad) < 1e-5
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        assert _rel(p.grad, sd[n].grad) < 1e-5, (n, _rel(p.grad, sd[n].grad))


def _embed_ref(dx, codes, n_tab, V, row0=0):
    B, E, T = dx.shape
    rows = dx.double().permute(0, 2, 1).reshape(-1, E)
    ref = torch.zeros(n_tab, V, E, dtype=torch.float64)
    mag = torch.zeros(n_tab, V, E, dtype=torch.float64)
    for i in range(n_tab):
        idx = codes[:, row0 + i, :].reshape(-1)
        ref[i].index_add_(0, idx, rows)
        mag[i].index_add_(0, idx, rows.abs())
    return ref, mag


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["redecoder", "ragged", "one_code"])
def test_embed_sum_backward_against_fp64_and_deterministic(cuda, case):
    """fac_embed_sum_bwd against float64 index_add_: within the recursive-summation bound n 2^-24 sum|terms| per element (n = frames
    sharing the entry), untouched rows exactly zero, and bit-identical across two runs.  'one_code' puts every frame on one code (the
    silence case at its worst: B T frames into one row)."""
    from facodec_amd import ops
    B, E, T, n_codes, n_tab, V, row0 = dict(redecoder=(4, 512, 80, 3, 3, 1024, 0), ragged=(3, 20, 700, 4, 2, 37, 1),
                                            one_code=(16, 512, 80, 2, 2, 1024, 0))[case]
    gen = torch.Generator().manual_seed(5)
    dx = torch.randn(B, E, T, generator=gen)
    codes = torch.randint(0, V, (B, n_codes, T), generator=gen)
    if case == "redecoder":
        codes[:, 0, : T // 2] = 520                  # long silence on the prosody row
    if case == "one_code":
        codes[:] = 7
    got = ops.embed_sum_bwd(dx.to(cuda), codes.to(cuda), n_tab, V, code_row0=row0)
    again = ops.embed_sum_bwd(dx.to(cuda), codes.to(cuda), n_tab, V, code_row0=row0)
    torch.cuda.synchronize()
    assert torch.equal(got, again)
    ref, mag = _embed_ref(dx, codes, n_tab, V, row0)
    n = torch.stack([torch.bincount(codes[:, row0 + i].reshape(-1), minlength=V) for i in range(n_tab)]).double().unsqueeze(-1)
    err = (got.cpu().double() - ref).abs()
    assert bool((err <= n * 2.0 ** -24 * mag).all()), float((err / (n * 2.0 ** -24 * mag).clamp_min(1e-300)).max())
    assert bool((got.cpu()[(n == 0).expand_as(got.cpu())] == 0).all())


@pytest.mark.gpu
def test_redecoder_train_forward_gradients_reach_every_table(cuda):
    """Redecoder.forward in .train() mode: the prosody table, the first n_c content tables, the WaveNet (cond_layer included) and
    conv_out get gradients; a content table beyond n_c gets none; the eval forward of the same weights gives the same output."""
    from facodec_amd.commons import build_model, default_redecoder_params
    args = default_redecoder_params()
    rm = build_model(args, stage="redecoder")
    synth.load_synthetic(rm.encoder, seed=0, prefix="redecoder.encoder.")
    enc = rm.encoder.to(cuda)
    gen = torch.Generator().manual_seed(2)
    p = torch.randint(0, 1024, (2, 1, 40), generator=gen).to(cuda)
    c = torch.randint(0, 1024, (2, 2, 40), generator=gen).to(cuda)
    tv = torch.randn(2, 1024, generator=gen).to(cuda)
    with torch.no_grad():
        ref = enc.eval()(p, c, tv, n_c=1)
    y = enc.train()(p, c, tv, n_c=1, dropout=False)
    assert _rel(y, ref) < 1e-5
    y.square().sum().backward()
    for n, q in enc.named_parameters():
        if n == "content_embed.1.weight":
            assert q.grad is None
        else:
            assert q.grad is not None and float(q.grad.abs().sum()) > 0, n


@pytest.mark.gpu
@pytest.mark.parametrize("T", [55, 56])
def test_noncausal_residual_unit_backward_at_fold_guard(cuda, T):
    """A non-causal reflect-padded ResidualUnit (C 64, dilation 9: 27 + 27 padding) through the fused training node at the
    fac_pad_fold_edges guard (T = 55: both edges fold onto one sample, the copying fold takes it) and one above it (in-place fold)."""
    from facodec_amd import autograd as A
    from facodec_amd.dac_model import ResidualUnit
    from facodec_amd.layers import Snake1d
    C, B = 64, 2
    ru, nxt = ResidualUnit(C, dilation=9, causal=False), Snake1d(C)
    synth.load_synthetic(ru, seed=9, prefix="ru.")
    synth.load_synthetic(nxt, seed=9, prefix="nxt.")
    ru.to(cuda).train()
    nxt.to(cuda)
    gen = torch.Generator().manual_seed(T)
    x, r1, r2 = (torch.randn(B, C, T, generator=gen) for _ in range(3))
    xg = x.to(cuda).requires_grad_()
    xr, xa = A.snake_dual(xg, ru.block[0].alpha)
    y, ya = A.res_unit(ru, xr, xa, nxt.alpha)
    ((y * r1.to(cuda)).sum() + (ya * r2.to(cuda)).sum()).backward()

    def snake(v, a):
        return v + torch.sin(a * v) ** 2 / (a + 1e-9)

    sd = {n: q.detach().cpu().double().requires_grad_() for n, q in ru.named_parameters()}
    an = nxt.alpha.detach().cpu().double().requires_grad_()
    x64 = x.double().requires_grad_()
    h = snake(_sconv64(sd, "block.1", snake(x64, sd["block.0.alpha"]), 7, dilation=9), sd["block.2.alpha"])
    y64 = x64 + _sconv64(sd, "block.3", h, 1)
    ((y64 * r1.double()).sum() + (snake(y64, an) * r2.double()).sum()).backward()
    assert _rel(xg.grad, x64.grad) < 1e-5
    assert _rel(nxt.alpha.grad, an.grad) < 1e-5
    for n, q in ru.named_parameters():
        assert _rel(q.grad, sd[n].grad) < 1e-5, (n, _rel(q.grad, sd[n].grad))
