"""The two regression targets of the predictor heads that the training script derives from the mel segment itself
(train.py:214-260): `targets["f0"]` -- the frozen pitch extractor's F0, normalised per clip -- and `targets["uv"]` -- the log of the
mel norm.  Both on the device, ready to merge into `train.TrainStep`'s `targets`.  The phoneme and speaker targets come from
networks outside this package."""
from . import ops


def normalize_f0(f0, want_mean=False):
    """train.py:224-256 on the device: f0 (B, T) -> (B, T).  Voiced = f0 > 5; log2 over the voiced frames, minus their mean, over their
    unbiased standard deviation; -10 on unvoiced frames and wherever the result is NaN or inf (a clip with one voiced frame, or whose
    voiced frames are all equal); a clip without a voiced frame is all -10.  want_mean: also the per-clip means (`gt_glob_f0s`, 0 for
    a clip without a voiced frame)."""
    return ops.f0_normalize(f0, want_mean)


def mel_log_norm(mel):
    """modules/commons.py:176-181 (`log_norm` with its defaults on mel.unsqueeze(1), squeezed): mel (B, n_mels, T) -> (B, T),
    log(||exp(4 mel - 4)||_2 over the bins)."""
    return ops.mel_log_norm(mel)


def predictor_targets(pitch_extractor, mel_seg, norm_f0=True, frame_rate=80):
    """mel_seg (B, 80, F): the meldataset.preprocess features cropped as train.py:200 -> dict(f0=(B, F), uv=(B, F)) float32 on the
    device (train.py:215-256).  norm_f0=False returns the extractor's raw F0 (train.py:221-222)."""
    if frame_rate != 80:
        raise NotImplementedError("frame_rate != 80 (the F.interpolate of train.py:258-260) is not built")
    f0 = pitch_extractor(mel_seg.unsqueeze(1))[0]
    return dict(f0=normalize_f0(f0) if norm_f0 else f0, uv=mel_log_norm(mel_seg))
