"""The JDC F0 extractor on the HIP path (facodec_amd/jdc.py, csrc/jdc.hip): state dict, stage geometry and host-side folding on the
CPU; on the GPU each new kernel alone against exact / fp64 references, one 3 x 3 layer through the row-concatenated layout against
fp64 F.conv2d, the BiLSTM + head against fp64 nn.LSTM, and the whole network against the real reference's outputs
(tests/golden/jdc.npz, made by tests/golden/make_golden_jdc.py).

Measured on an MI355X (worst error / bound, or error relative to max |ref|): see DESIGN.md 18."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from facodec_amd import _lib, commons, jdc, ops, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ULP = 2.0 ** -23


# ===================================================================================================== CPU
def test_state_dict_matches_the_reference_class():
    want = json.load(open(os.path.join(GOLDEN, "jdc_state_shapes.json")))
    sd = jdc.JDCNet(num_class=1, seq_len=192).state_dict()
    assert len(want) == 77
    assert {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()} == want
    m = jdc.JDCNet(num_class=1, seq_len=192)
    res = m.load_state_dict(synth.synth_jdc_state_dict(0), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(not p.requires_grad for p in m.parameters())


def test_stage_geometry():
    W, P, pools = jdc.stage_geometry(80)
    assert W == (80, 40, 20, 10, 2) and pools == (2, 2, 2, 4)
    for i in range(4):
        assert P[i] >= W[i] + 1, (i, W, P)                  # a zero column between the rows wherever a 3 x 3 conv reads
        assert P[i + 1] * pools[i] == P[i], (i, P)
        assert W[i + 1] == W[i] // pools[i]
    assert P[4] >= W[4]
    assert P == (96, 48, 24, 12, 3)
    for n in (32, 33, 81, 128, 513):                        # other bin counts keep the same invariants
        W, P, pools = jdc.stage_geometry(n)
        assert all(P[i] >= W[i] + 1 and P[i + 1] * pools[i] == P[i] for i in range(4)) and P[4] >= W[4], (n, W, P)
    with pytest.raises(ValueError):
        jdc.stage_geometry(31)


def _within_ulps(got, ref64, n):
    got, ref64 = got.double().reshape(-1), ref64.reshape(-1)
    ulp = torch.from_numpy(np.spacing(np.abs(ref64.numpy()).astype(np.float32)).astype(np.float64))
    return bool(((got - ref64).abs() <= n * ulp).all())


def test_host_folding_against_fp64():
    m = jdc.JDCNet(num_class=1, seq_len=192)
    m.load_state_dict(synth.synth_jdc_state_dict(0))
    for conv, bn in ((m.conv_block[0], m.conv_block[1]), (m.res_block2.conv[0], m.res_block2.conv[1])):
        g, b, mu, var = (t.double() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
        scale = g / (var + bn.eps).sqrt()
        shift = b - mu * scale
        sc, sh = jdc.bn_scale_shift(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
        assert sc.dtype == sh.dtype == torch.float32
        assert _within_ulps(sc, scale, 2) and _within_ulps(sh, shift, 2)
        w, bias = jdc.fold_bn(conv.weight, bn)
        assert w.shape == (conv.weight.shape[0], conv.weight.shape[1], 9) and w.dtype == torch.float32
        assert _within_ulps(w, (conv.weight.double() * scale.view(-1, 1, 1, 1)).flatten(2), 2) and _within_ulps(bias, shift, 2)


def test_cpu_tensors_raise():
    m = jdc.JDCNet(num_class=1, seq_len=192)
    with pytest.raises(_lib.FacodecHipError):
        m(torch.zeros(1, 1, 80, 4))
    with pytest.raises(_lib.FacodecHipError):
        ops.jdc_layout_in(torch.zeros(1, 1, 80, 4), 96)
    with pytest.raises(_lib.FacodecHipError):
        ops.jdc_affine_lrelu_pool(torch.zeros(1, 2, 24), None, None, 2, 2, 10, 12, 2, 0.01)


def test_load_F0_models_reads_a_checkpoint(tmp_path):
    sd = synth.synth_jdc_state_dict(3)
    path = tmp_path / "bst.t7"
    torch.save({"net": sd, "epoch": 1}, path)
    m = commons.load_F0_models(str(path))
    assert isinstance(m, jdc.JDCNet) and m.num_class == 1
    got = m.state_dict()
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)


# ===================================================================================================== GPU helpers
def _to_signal(x, P):
    """x (B, C, T, W) -> (1, C, B * (T + 1) * P) with zero gaps and separator rows (host-side restatement of the layout)."""
    B, C, T, W = x.shape
    s = torch.zeros(C, B, T + 1, P, dtype=x.dtype)
    s[:, :, :T, :W] = x.permute(1, 0, 2, 3)
    return s.reshape(1, C, -1)


def _from_signal(s, B, T, W, P):
    C = s.shape[-2]
    return s.reshape(C, B, T + 1, P)[:, :, :T, :W].permute(1, 0, 2, 3)


def _g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(scope="module")
def model(cuda):
    m = jdc.JDCNet(num_class=1, seq_len=192)
    m.load_state_dict(synth.synth_jdc_state_dict(0), strict=True)
    return m.to(cuda)


# ===================================================================================================== 1. affine-LReLU-pool alone
@pytest.mark.gpu
@pytest.mark.parametrize("W,P,pool", [(10, 12, 2), (10, 12, 4), (10, 12, 1),       # one output per thread (P / pool % 4 != 0), 16-byte form at pool 1
                                      (20, 24, 2), (18, 32, 4)])                  # the 16-byte forms at pool 2 and 4
@pytest.mark.parametrize("negative", [False, True])
def test_affine_lrelu_pool(cuda, W, P, pool, negative):
    C, B, T, slope = 3, 2, 3, 0.01
    rows, Wo, Po = B * (T + 1), W // pool, P // pool
    g = _g(100 * W + 10 * pool + negative)
    x = torch.randn(B, C, T, W, generator=g)
    if negative:
        x = -x.abs() - 0.01                       # all valid entries negative: the maximum must be negative, not the 0 it could start from
        scale = shift = None
    else:
        scale, shift = torch.randn(C, generator=g), torch.randn(C, generator=g)
    sig = torch.full((C, B, T + 1, P), 1e30)      # gaps and separator rows hold what a conv leaves there: anything
    sig[:, :, :T, :W] = x.permute(1, 0, 2, 3)
    y = ops.jdc_affine_lrelu_pool(sig.reshape(1, C, -1).to(cuda), None if scale is None else scale.to(cuda),
                                  None if shift is None else shift.to(cuda), rows, T + 1, W, P, pool, slope)
    assert y.shape == (1, C, rows * Po)
    y = y.cpu().reshape(C, B, T + 1, Po)
    s64 = (scale if scale is not None else torch.ones(C)).double().view(1, C, 1, 1)
    h64 = (shift if shift is not None else torch.zeros(C)).double().view(1, C, 1, 1)
    v = s64 * x.double() + h64
    act = torch.where(v > 0, v, v * float(np.float32(slope)))
    mag = (s64 * x.double()).abs() + h64.abs()
    # the floor drops the trailing bins (10 -> 2 at pool 4 never sees bins 8 and 9)
    ref = act[..., :Wo * pool].reshape(B, C, T, Wo, pool).max(-1).values
    bound = 2 * ULP * mag[..., :Wo * pool].reshape(B, C, T, Wo, pool).max(-1).values
    got = y[:, :, :T, :Wo].permute(1, 0, 2, 3).double()
    ratio = float(((got - ref).abs() / bound).max())
    print(f"[tol] jdc_affine_lrelu_pool pool={pool} negative={negative}: error / bound {ratio:.3e}")
    assert ratio <= 1.0
    if negative:
        assert bool((got < 0).all())
    if W % pool:
        x2 = x.clone()
        x2[..., Wo * pool:] = 1e6
        sig[:, :, :T, :W] = x2.permute(1, 0, 2, 3)
        y2 = ops.jdc_affine_lrelu_pool(sig.reshape(1, C, -1).to(cuda), None if scale is None else scale.to(cuda),
                                       None if shift is None else shift.to(cuda), rows, T + 1, W, P, pool, slope)
        assert torch.equal(y2.cpu().reshape(C, B, T + 1, Po), y)
    assert bool((y[:, :, :T, Wo:] == 0).all()) and bool((y[:, :, T, :] == 0).all())      # exact zeros: the next conv's padding


# ===================================================================================================== 2. one 3 x 3 layer
def _variant(c_in, c_out, n, k, pad_left, k1=0, dil2=0, res=False, bias=False):
    d = ops.conv_desc(1, c_in, n, c_out, k, pad_left=pad_left, pad_mode=ops.PAD_ZERO, t_out=n, k1=k1, dilation2=dil2)
    fake = ctypes.c_void_p(0x10000)                 # never dereferenced: fac_conv1d_variant only reads the descriptor
    d.x, d.w, d.y = fake, fake, fake
    d.bias, d.res = (fake if bias else None), (fake if res else None)
    d.ws, d.ws_bytes = fake, ops.CONV_WS_BYTES
    vid, name = ops.conv_variant(d)
    assert vid >= 0, name
    return name


@pytest.mark.gpu
@pytest.mark.parametrize("c_in,c_out,W,P,shortcut", [(1, 64, 10, 12, False), (64, 64, 10, 12, False), (64, 128, 5, 8, True)])
def test_conv3x3_through_the_layout(cuda, c_in, c_out, W, P, shortcut):
    from test_train_kernels_gen import _sum_bound
    B, T = 2, 5
    g = _g(c_in + c_out)
    x = torch.randn(B, c_in, T, W, generator=g)
    w = torch.randn(c_out, c_in, 3, 3, generator=g) / (9 * c_in) ** 0.5
    w1 = torch.randn(c_out, c_in, 1, 1, generator=g) / c_in ** 0.5 if shortcut else None

    def run(xin):
        if c_in == 1:                             # the layout-in kernel takes (B, 1, bins, frames)
            sig = ops.jdc_layout_in(xin.transpose(-1, -2).contiguous().to(cuda), P)
        else:
            sig = _to_signal(xin, P).to(cuda)
        n = sig.shape[-1]
        assert n == B * (T + 1) * P
        res = None
        if shortcut:
            res = ops.conv1d(sig, ops.pack_conv_weight(w1.flatten(2).to(cuda)), c_out, 1, pad_left=0, pad_mode=ops.PAD_ZERO, t_out=n)
        y = jdc.JDCNet._conv3(sig, ops.pack_conv_weight(w.flatten(2).to(cuda)), c_out, P, res=res)
        return _from_signal(y.cpu(), B, T, W, P)

    got = run(x)
    ref = F.conv2d(x.double(), w.double(), padding=1)
    mag = F.conv2d(x.double().abs(), w.double().abs(), padding=1)
    n_terms = 9 * c_in
    names = [_variant(c_in, c_out, B * (T + 1) * P, 9, P + 1, 3, P, res=shortcut)]
    if shortcut:
        ref = ref + F.conv2d(x.double(), w1.double())
        mag = mag + F.conv2d(x.double().abs(), w1.double().abs())
        n_terms += c_in
        names.append(_variant(c_in, c_out, B * (T + 1) * P, 1, 0))
    extra = 3.0 if any("bf16x3" in n for n in names) else 0.0
    print(f"[route] conv3x3 {c_in}->{c_out}: {names}")
    _sum_bound(f"jdc.conv3x3.{c_in}x{c_out}" + (".shortcut" if shortcut else ""), got, ref, mag, n_terms, extra=extra)
    x2 = x.clone()
    x2[1] = torch.randn(c_in, T, W, generator=g) * 50.0
    assert torch.equal(run(x2)[0], got[0])         # the separator row keeps the clips apart


# ===================================================================================================== 3. layout in / out
@pytest.mark.gpu
def test_layout_in_and_out_are_exact(cuda):
    B, C, T, W, P = 3, 5, 4, 2, 3
    x = torch.randn(B, C, T, W, generator=_g(3))
    sig = _to_signal(x, P).to(cuda)
    BP = ops.pad32(B)
    want = torch.zeros(C * W, T, BP)
    want[:, :, :B] = x.permute(0, 2, 1, 3).contiguous().view(B, T, C * W).permute(2, 1, 0)     # the reference's permute / view, time-major
    got = ops.jdc_to_time_major(sig, B, T, W, P)
    assert got.shape == (C * W, T, BP) and torch.equal(got.cpu(), want)
    assert torch.equal(ops.jdc_to_time_major(sig, B, T, W, P, reverse=True).cpu(), want.flip(1))
    assert torch.equal(ops.jdc_to_nchw(sig, B, T, W, P).cpu(), x)
    assert torch.equal(ops.jdc_to_nchw(sig, B, T, W, P, transposed=True).cpu(), x.transpose(-1, -2).contiguous())
    mel = torch.randn(2, 1, 7, 5, generator=_g(4))
    assert torch.equal(ops.jdc_layout_in(mel.to(cuda), 9).cpu(), _to_signal(mel.transpose(-1, -2), 9))


# ===================================================================================================== 4. BiLSTM + head
@pytest.mark.gpu
def test_bilstm_and_head_against_fp64(cuda, model):
    B, T = 3, 5
    W, P, pools = jdc.stage_geometry(80)
    x = torch.randn(B, 256, T, W[4], generator=_g(5))
    s4 = _to_signal(x, P[4]).to(cuda)
    geo = (B, T, W, P, pools)
    p = model._prepare(cuda)
    hf = model._direction(s4, geo, p["fwd"], False)
    hb = model._direction(s4, geo, p["bwd"], True)
    assert hf.shape == hb.shape == (256, T, 32)
    got = ops.jdc_head(hf, hb, p["head"][0], p["head"][1], B).cpu()
    lstm = torch.nn.LSTM(512, 256, batch_first=True, bidirectional=True).double()
    lstm.load_state_dict({k: v.double().cpu() for k, v in model.bilstm_classifier.state_dict().items()})
    with torch.no_grad():
        h, _ = lstm(x.double().permute(0, 2, 1, 3).reshape(B, T, 512))
        ref = (h @ model.classifier.weight.double().cpu().t() + model.classifier.bias.double().cpu()).squeeze(-1).abs()
    err = float((got.double() - ref).abs().max() / ref.abs().max())
    print(f"[tol] jdc.bilstm_head: {err:.3e} of max |ref| (bound 1e-5)")
    assert got.shape == (B, T) and err <= 1e-5


# ===================================================================================================== 5. the whole network
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "jdc.npz"))


@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, 1])
def test_network_against_the_reference(cuda, model, golden, i):
    x = torch.from_numpy(golden[f"x{i}"]).to(cuda)
    B, _, _, T = x.shape
    model.eval()
    f0, gan, pooled = model(x)
    assert f0.shape == (B, T) and gan.shape == (B, 256, 10, T) and pooled.shape == (B, 256, T, 2)
    assert f0.dtype == gan.dtype == pooled.dtype == torch.float32 and f0.is_cuda
    for name, got, key in (("F0", f0, "F0"), ("GAN_feature", gan[:, ::8], "gan"), ("poolblock_out", pooled[:, ::8], "pool")):
        ref = torch.from_numpy(golden[f"{key}_{i}"]).double()
        err = float((got.cpu().double() - ref).abs().max() / ref.abs().max())
        print(f"[tol] jdc.network input {i} {name}: {err:.3e} of max |ref| (bound 1e-4; the reference's own fp32 vs fp64: "
              f"{float(golden[f'err_{key}_{i}']):.3e})")
        assert err <= 1e-4, (name, err)
    assert torch.equal(model.get_feature_GAN(x), gan) and torch.equal(model.get_feature(x), pooled)
    model.train()                                   # eval arithmetic in either mode
    again = model(x)
    model.eval()
    assert all(torch.equal(a, b) for a, b in zip(again, (f0, gan, pooled)))
    for b in range(B):                              # each clip alone agrees with its row of the batch
        alone = model(x[b:b + 1].contiguous())
        for a, full in zip(alone, (f0, gan, pooled)):
            err = float((a[0].double() - full[b].double()).abs().max() / full.double().abs().max())
            assert err <= 1e-6, (b, err)
