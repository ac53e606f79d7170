"""The predictor heads' two mel-derived targets on the device (facodec_amd/targets.py, csrc/jdc.hip): the per-clip F0 normalisation
of train.py:224-256 against that loop restated in fp64, `log_norm` (modules/commons.py:176-181) against fp64, and
`predictor_targets` / `commons.extract_f0` against the explicit chains.  Measured figures: DESIGN.md 18."""
import pytest
import torch

from facodec_amd import commons, jdc, synth, targets


def test_frame_rate_other_than_80_is_not_built():
    with pytest.raises(NotImplementedError, match="258-260"):
        targets.predictor_targets(None, torch.zeros(1, 80, 4), frame_rate=50)


def test_cpu_tensors_raise():
    from facodec_amd._lib import FacodecHipError
    with pytest.raises(FacodecHipError):
        targets.normalize_f0(torch.zeros(2, 5))
    with pytest.raises(FacodecHipError):
        targets.mel_log_norm(torch.zeros(2, 80, 5))


def _normalize_ref(F0_real):
    """train.py:224-256 in float64 -> (f0_targets, gt_glob_f0s)."""
    out, means = [], []
    for row in F0_real:
        voiced = row > 5.0
        f0_voiced = row[voiced]
        if len(f0_voiced) != 0:
            log_f0 = f0_voiced.log2()
            mean_f0 = log_f0.mean()
            seq = torch.zeros_like(row)
            seq[voiced] = (log_f0 - mean_f0) / log_f0.std()
            seq[~voiced] = -10
            means.append(mean_f0)
        else:
            seq = torch.zeros_like(row) - 10.0
            means.append(torch.tensor(0.0, dtype=row.dtype))
        out.append(seq)
    out = torch.stack(out)
    out[torch.isnan(out)] = -10.0
    out[torch.isinf(out)] = -10.0
    return out, torch.stack(means)


def _f0_batch():
    """(6, 17): mixed, no voiced frame, one voiced frame, all voiced and equal, a ramp 80 -> 400, a NaN and an inf frame.  Every value
    is <= 4 or >= 6: the `> 5` decision never hinges on rounding."""
    g = torch.Generator().manual_seed(6)
    T = 17
    mixed = 90.0 + 300.0 * torch.rand(T, generator=g)
    mixed[[0, 3, 4, 11, 16]] = torch.tensor([0.0, 3.5, 1.0, 4.0, 0.25])
    none = 4.0 * torch.rand(T, generator=g)
    one = 4.0 * torch.rand(T, generator=g)
    one[7] = 210.0
    equal = torch.full((T,), 256.0)          # log2 exact: mean and deviations are exactly 8 and 0 in any precision and order
    ramp = torch.linspace(80.0, 400.0, T)
    bad = 100.0 + 200.0 * torch.rand(T, generator=g)
    bad[2], bad[9], bad[12] = float("nan"), float("inf"), 2.0
    f0 = torch.stack([mixed, none, one, equal, ramp, bad])
    fin = f0[torch.isfinite(f0)]
    assert bool(((fin <= 4.0) | (fin >= 6.0)).all())
    return f0


@pytest.mark.gpu
def test_normalize_f0_against_the_training_loop(cuda):
    f0 = _f0_batch()
    ref, ref_mean = _normalize_ref(f0.double())
    got, mean = targets.normalize_f0(f0.to(cuda), want_mean=True)
    got, mean = got.cpu(), mean.cpu()
    assert got.shape == f0.shape and got.dtype == torch.float32 and mean.shape == (6,)
    flat = ref == -10.0
    assert bool(flat[1].all() and flat[2].all() and flat[3].all() and flat[5].all()) and not bool(flat[4].any())
    assert bool((got[flat] == -10.0).all())                       # unvoiced / degenerate positions: exactly -10
    err = float((got.double() - ref)[~flat].abs().max())
    fin = torch.isfinite(ref_mean)
    rel = float(((mean.double() - ref_mean)[fin].abs() / ref_mean[fin].abs().clamp_min(1e-300)).max())
    print(f"[tol] f0_normalize: values {err:.3e} absolute (bound 1e-5), per-clip means {rel:.3e} relative (bound 1e-6)")
    assert err <= 1e-5
    assert rel <= 1e-6 and float(mean[1]) == 0.0
    assert bool((mean[~fin].double() == ref_mean[~fin]).all())    # the clip with an inf frame: the reference's mean is inf
    assert torch.equal(targets.normalize_f0(f0.to(cuda)).cpu(), got)


@pytest.mark.gpu
def test_mel_log_norm_against_fp64(cuda):
    mel = 3.0 * torch.rand(2, 80, 17, generator=torch.Generator().manual_seed(7)) - 1.5
    ref = torch.log(torch.exp(mel.double().unsqueeze(1) * 4 + -4).norm(dim=2)).squeeze(1)
    got = targets.mel_log_norm(mel.to(cuda)).cpu()
    rel = float(((got.double() - ref).abs() / ref.abs()).max())
    print(f"[tol] mel_log_norm: {rel:.3e} relative (bound 1e-6); min |ref| {float(ref.abs().min()):.3f}")
    assert got.shape == (2, 17) and got.dtype == torch.float32 and rel <= 1e-6


@pytest.mark.gpu
def test_predictor_targets_and_extract_f0(cuda):
    from facodec_amd import autograd_disc as AD
    from facodec_amd import meldataset
    m = jdc.JDCNet(num_class=1, seq_len=192)
    m.load_state_dict(synth.synth_jdc_state_dict(0), strict=True)
    m = m.to(cuda)
    B, Fr = 2, 24
    mel = (3.0 * torch.rand(B, 80, Fr, generator=torch.Generator().manual_seed(8)) - 1.5).to(cuda)
    t = targets.predictor_targets(m, mel)
    raw = m(mel.unsqueeze(1))[0]
    assert set(t) == {"f0", "uv"}
    for v in t.values():
        assert v.shape == (B, Fr) and v.dtype == torch.float32 and v.is_cuda
    assert torch.equal(t["f0"], targets.normalize_f0(raw)) and torch.equal(t["uv"], targets.mel_log_norm(mel))
    assert torch.equal(targets.predictor_targets(m, mel, norm_f0=False)["f0"], raw)
    # TrainStep.predictor_losses' own slicing and its smooth-L1 against a prediction of 20 frames
    pred = torch.randn(B, 20, 1, device=cuda)
    n = min(pred.shape[-2], t["f0"].shape[-1])
    for k in ("f0", "uv"):
        loss = AD.PairMean.apply(pred.squeeze(-1)[..., :n].contiguous(), t[k][..., :n].contiguous(), 3)
        assert bool(torch.isfinite(loss).all())
    waves = synth.synth_clips(2, 7200, seed=9)[:, 0].to(cuda)
    f0 = commons.extract_f0(m, waves)
    assert f0.shape == (2, 25)
    assert torch.equal(f0, m(meldataset.preprocess(waves).unsqueeze(1))[0])
