"""Model factory with the reference's surface (modules/commons.py:283-348, :446-479):

    model = build_model(recursive_munch(config['model_params']))      # stage='codec'
    z = model.encoder(wave); z, quantized, commit, codebook, timbre = model.quantizer(z, wave, n_c=2)
    wave_hat = model.decoder(z)

so reconstruct.py / train.py-style drivers keep working unchanged.  `munch` is not installed in this
image, hence the small attribute-dict below (same behaviour for the keys the callers use).
"""
import torch


class Munch(dict):
    """dict with attribute access (stand-in for munch.Munch, modules/commons.py:6)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v


def recursive_munch(d):
    """modules/commons.py:473-479."""
    if isinstance(d, dict):
        return Munch((k, recursive_munch(v)) for k, v in d.items())
    if isinstance(d, list):
        return [recursive_munch(v) for v in d]
    return d


def build_model(args, stage="codec", with_discriminator=False):
    """modules/commons.py:283-348.  Returns Munch(encoder, quantizer, decoder, discriminator, fa_predictors)
    with the reference's key order.  with_discriminator: stage 'redecoder' also builds its discriminator (:401-407), for
    training (train_redecoder.RedecoderTrainStep); by default that stage returns exactly {encoder, decoder}."""
    from .dac_model import Encoder, Decoder
    from .quantize import FAquantizer

    if stage == "redecoder":      # modules/commons.py:385-413 (discriminator: train-only, on request)
        from .redecoder import Redecoder
        nets = Munch(encoder=Redecoder(args),
                     decoder=Decoder(input_channel=1024, channels=args.DAC.decoder_dim, rates=args.DAC.decoder_rates,
                                     causal=args.decoder_causal, lstm=args.decoder_lstm))
        if with_discriminator:
            from .train_redecoder import redecoder_discriminator
            nets.discriminator = redecoder_discriminator(args.DAC.sr)
        return nets
    if stage == "encoder":        # modules/commons.py:414-439
        return Munch(encoder=Encoder(d_model=args.DAC.encoder_dim, strides=args.DAC.encoder_rates, d_latent=1024,
                                     causal=args.encoder_causal, lstm=args.encoder_lstm),
                     quantizer=FAquantizer(in_dim=1024, n_p_codebooks=1, n_c_codebooks=args.n_c_codebooks,
                                           n_t_codebooks=2, n_r_codebooks=3, codebook_size=1024, codebook_dim=8,
                                           quantizer_dropout=0.5, causal=args.encoder_causal,
                                           separate_prosody_encoder=args.separate_prosody_encoder,
                                           timbre_norm=args.timbre_norm))
    if stage != "codec":
        raise ValueError(f"Unknown stage: {stage}")

    encoder = Encoder(d_model=args.DAC.encoder_dim, strides=args.DAC.encoder_rates, d_latent=1024,
                      causal=args.causal, lstm=args.lstm)
    quantizer = FAquantizer(in_dim=1024, n_p_codebooks=1, n_c_codebooks=args.n_c_codebooks, n_t_codebooks=2,
                            n_r_codebooks=3, codebook_size=1024, codebook_dim=8, quantizer_dropout=0.5,
                            causal=args.causal, separate_prosody_encoder=args.separate_prosody_encoder,
                            timbre_norm=args.timbre_norm)
    decoder = Decoder(input_channel=1024, channels=args.DAC.decoder_dim, rates=args.DAC.decoder_rates,
                      causal=args.causal, lstm=args.lstm)
    from .predictors import FApredictors
    fa_predictors = FApredictors(in_dim=1024, use_gr_content_f0=args.use_gr_content_f0,
                                 use_gr_prosody_phone=args.use_gr_prosody_phone, use_gr_residual_f0=True,
                                 use_gr_residual_phone=True, use_gr_timbre_content=True,
                                 use_gr_timbre_prosody=args.use_gr_timbre_prosody, use_gr_x_timbre=True,
                                 norm_f0=args.norm_f0, timbre_norm=args.timbre_norm,
                                 use_gr_content_global_f0=args.use_gr_content_global_f0)
    from .discriminator import Discriminator
    discriminator = Discriminator(rates=[], periods=[2, 3, 5, 7, 11], fft_sizes=[2048, 1024, 512],
                                  sample_rate=args.DAC.sr)                      # modules/commons.py:334-340
    return Munch(encoder=encoder, quantizer=quantizer, decoder=decoder, discriminator=discriminator,
                 fa_predictors=fa_predictors)


def default_model_params():
    """configs/config.yml:27-46 `model_params`."""
    return recursive_munch(dict(
        fixed=True, causal=True, lstm=2, norm_f0=True, use_gr_content_f0=False, use_gr_prosody_phone=False,
        use_gr_timbre_prosody=False, separate_prosody_encoder=True, n_c_codebooks=2, timbre_norm=True,
        use_gr_content_global_f0=True, w2v="w2v-ctc",
        DAC=dict(encoder_dim=64, encoder_rates=[2, 5, 5, 6], decoder_dim=1536, decoder_rates=[6, 5, 5, 2], sr=24000)))


def default_redecoder_params():
    """configs/config_redecoder.yml:28-48 `model_params`."""
    return recursive_munch(dict(
        encoder_causal=True, decoder_causal=False, encoder_lstm=2, decoder_lstm=0, n_c_codebooks=2, n_p_codebooks=1,
        timbre_norm=True, separate_prosody_encoder=True, encoder_type="wavenet", wavenet_embed_dim=512,
        mamba_embed_dim=768, prob_random_mask_prosody=1.0, prob_random_mask_content=[0.0, 1.0],
        DAC=dict(encoder_dim=64, encoder_rates=[2, 5, 5, 6], decoder_dim=1536, decoder_rates=[6, 5, 5, 2], sr=24000)))


@torch.no_grad()
def decode_codes(model, codes, timbre):
    """Codes + timbre -> waveform, the counterpart of reconstruct.py's encode -> quantize -> decode:

        z = model.encoder(wave)
        _, _, _, _, timbre, codes = model.quantizer(z, wave, n_c=2, return_codes=True)
        wave_hat = decode_codes(model, codes, timbre)                  # (B, 1, 300 T)
        converted = decode_codes(model, codes, other_timbre)           # timbre swap (zero-shot voice conversion)

    codes = [codes_p, codes_c, codes_r] (B, n, T) int64; timbre (B, 1024).  FAquantizer.decode_input (one fac_vq_decode launch)
    then the decoder."""
    return model.decoder(model.quantizer.decode_input(codes, timbre))


# ------------------------------------------------------------------------------------ clips of different lengths
# Sample budget of one padded batch (clips x longest clip): the benchmark's 32 clips x 2 s, the batch every kernel is tuned on.
MAX_BATCH_SAMPLES = 32 * 48000


def plan_groups(lengths, max_batch_samples=MAX_BATCH_SAMPLES):
    """Groups clips into padded batches: -> list of index lists.  The clips are sorted by length (ascending, ties in the caller's
    order) and cut into runs of neighbours; a run grows while count x longest clip (what the padded batch holds) stays within
    the budget, so a long clip is batched with clips of its own size and never pads the short ones up to itself.  A single
    clip longer than the budget is a group of its own."""
    order = sorted(range(len(lengths)), key=lambda i: (lengths[i], i))
    groups, cur = [], []
    for i in order:
        if cur and (len(cur) + 1) * lengths[i] > max_batch_samples:
            groups.append(cur)
            cur = []
        cur.append(i)
    if cur:
        groups.append(cur)
    return groups


def padding_share(lengths, groups):
    """Fraction of the padded batches' samples that is padding."""
    padded = sum(len(g) * max(lengths[i] for i in g) for g in groups)
    return 1.0 - sum(lengths) / padded if padded else 0.0


def _reflect_convs(model):
    """-> [(name, reflect pad in columns, samples per column or None, columns per frame or None)] of every reflect-padded conv of
    encoder, quantizer and decoder, walking each module tree in execution order; raises NotImplementedError for a non-causal
    conv (a right-padded batch gives every clip its own result only if nothing looks to the right)."""
    from .layers import SConv1d, SConvTranspose1d
    from . import ops
    found = []
    for key in ("encoder", "quantizer", "decoder"):
        rate = 1                                   # encoder: samples per column; decoder: columns per frame; quantizer: frame rate
        for name, m in model[key].named_modules():
            if isinstance(m, (SConv1d, SConvTranspose1d)) and not m.causal:
                raise NotImplementedError(f"{key}.{name} is not causal: batches of clips with different lengths need the causal "
                                          "configuration (right padding must not reach back into a clip)")
            if isinstance(m, SConvTranspose1d):
                rate *= m.stride
            elif isinstance(m, SConv1d):
                pad = (m.kernel_size - 1) * m.dilation + 1 - m.stride
                if m.pad_mode == ops.PAD_REFLECT and pad > 0:
                    found.append((f"{key}.{name}", pad, rate if key == "encoder" else None,
                                  rate if key == "decoder" else 1 if key == "quantizer" else None))
                if key == "encoder":
                    rate *= m.stride
    return found


def min_clip_samples(model):
    """Shortest clip the clip-list calls take: every reflect padding of the path needs a signal longer than the pad (as
    StreamingDecoder._min_prime derives it for the decoder's first chunk) -- the log-mel front-end's n_fft / 2 samples, a causal
    conv of the encoder `pad` columns of its own rate, a conv of the quantizer or decoder pad // (columns per frame) + 1 whole
    frames.  Below it the single-clip calls fail or fall back to a zero extension that depends on the clip's length, which a
    padded batch cannot reproduce.  (The shipped configuration: 3000 samples = 10 frames, the decoder's k = 7 convs of dilation 9
    at 6 columns per frame.)"""
    hop = model.quantizer.hop_length
    need = model.quantizer.to_mel.n_fft // 2 + 1
    for _, pad, per_col, per_frame in _reflect_convs(model):
        need = max(need, pad * per_col + 1 if per_col is not None else hop * (pad // per_frame + 1))
    return need


def _need_gpu(tensors, what):
    from ._lib import FacodecHipError
    for t in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what} must be tensors (got {type(t)})")
        if not t.is_cuda:
            raise FacodecHipError(f"{what} must live on the GPU (got {t.device}); there is no CPU path")


MODEL_RATE = 24000   # the codec's sample rate (DAC.sr); the clip-list calls resample from / to any other (ops.resample)


def _clip_lengths(model, tensors, what, per_item=1, ratio=None):
    """Lengths in samples at the model's rate, checked against min_clip_samples; ratio (o, n): the clips are at another rate and
    are resampled by n / o first, so what counts is ceil(T n / o)."""
    _need_gpu(tensors, what)
    lengths = [int(t.shape[-1]) * per_item for t in tensors]
    if ratio is not None:
        lengths = [-(-n * ratio[1] // ratio[0]) for n in lengths]
    need = min_clip_samples(model)
    hop = model.quantizer.hop_length
    for i, n in enumerate(lengths):
        if n < need:
            raise ValueError(f"clip {i} has {n} samples; the shortest clip this path takes has {need} samples "
                             f"({-(-need // hop)} frames: the longest reflect padding of encoder, log-mel front-end and decoder)")
    return lengths


@torch.no_grad()
def encode_clips(model, waves, n_c=2, max_batch_samples=MAX_BATCH_SAMPLES, sample_rate=MODEL_RATE, quality="best"):
    """Clips of different lengths -> codes and timbre per clip, in the caller's order:

        clips = encode_clips(model, [wave_0 (T_0,), wave_1 (1, T_1), ...])         # GPU tensors, float32, 24 kHz
        clips[i] == dict(codes=[p (1, T_i // 300), c (n_c, T_i // 300), r (3, T_i // 300)] int64, timbre=(1024,))

    every entry what the single-clip calls `model.encoder(w)`, `model.quantizer(z, w, n_c, return_codes=True)` give on that clip
    alone.  The clips are sorted by length and grouped into zero-padded batches under a sample budget (plan_groups); each group
    is one encoder pass and one FAquantizer.forward_ragged.  The reference's `collate` output (zero-padded `waves` (B, T) and
    `wave_lens`) maps onto it as `[waves[b, :wave_lens[b]] for b in range(B)]`.

    sample_rate: the clips' rate.  Other than 24000, every group is resampled to 24 kHz as one padded batch with its lengths in
    one ops.resample launch (`quality`), which gives every clip what ops.resample gives it alone; groups are planned and
    the shortest-clip check is made on the lengths AFTER resampling, ceil(T_i 24000 / sample_rate)."""
    from . import ops
    ratio = None
    if sample_rate != MODEL_RATE:
        geo = ops.resample_table(sample_rate, MODEL_RATE, quality)
        ratio = (geo["o"], geo["n"])
    waves = list(waves)
    if not waves:
        return []
    for w in waves:
        if isinstance(w, torch.Tensor) and not (w.dim() == 1 or (w.dim() == 2 and w.shape[0] == 1)):
            raise ValueError(f"every clip must be (T,) or (1, T), got {tuple(w.shape)}")
    lengths = _clip_lengths(model, waves, "clips", ratio=ratio)
    dev, hop = waves[0].device, model.quantizer.hop_length
    out = [None] * len(waves)
    for group in plan_groups(lengths, max_batch_samples):
        batch = torch.nn.utils.rnn.pad_sequence([waves[i].reshape(-1).to(torch.float32) for i in group], batch_first=True).unsqueeze(1)
        lens = ops.h2d(torch.tensor([lengths[i] for i in group], dtype=torch.int32), dev)
        if ratio is not None:
            lens_in = ops.h2d(torch.tensor([waves[i].shape[-1] for i in group], dtype=torch.int32), dev)
            batch = ops.resample(batch, sample_rate, MODEL_RATE, lens=lens_in, quality=quality)
        z = model.encoder(batch)
        _, codes, timbre, _ = model.quantizer.forward_ragged(z, batch, lens, n_c=n_c)
        for j, i in enumerate(group):
            out[i] = dict(codes=[c[j, :, :lengths[i] // hop] for c in codes], timbre=timbre[j])
    return out


@torch.no_grad()
def decode_clips(model, codes_list, timbres, max_batch_samples=MAX_BATCH_SAMPLES, sample_rate=MODEL_RATE, quality="best"):
    """Codes of clips of different lengths -> list of waves (1, 300 F_i), in the caller's order.  codes_list[i] =
    [p (n_p, F_i), c (n_c, F_i), r (n_r, F_i)] int64 as encode_clips returns them (the same row counts for every clip);
    timbres[i] (1024,): the clip's own or another clip's / speaker's (timbre swap, as in decode_codes).  Per group of
    plan_groups the codes are padded with code 0 and decoded by one fac_vq_decode launch and one decoder pass (causal: the
    padding cannot reach back into a clip); every wave is cropped to its clip.

    sample_rate other than 24000: every group's waves are resampled to it in one ops.resample launch with the clips' lengths,
    and clip i comes back with ceil(300 F_i sample_rate / 24000) samples, what ops.resample gives its 24 kHz wave alone."""
    from . import ops
    ratio = None
    if sample_rate != MODEL_RATE:
        geo = ops.resample_table(MODEL_RATE, sample_rate, quality)
        ratio = (geo["o"], geo["n"])
    codes_list = [list(c) for c in codes_list]
    if not codes_list:
        return []
    timbres = list(timbres)
    if len(timbres) != len(codes_list):
        raise ValueError(f"{len(codes_list)} clips but {len(timbres)} timbres")
    for c in codes_list:
        if len(c) != 3 or any(not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != c[0].shape[1] for x in c):
            raise ValueError("every clip's codes must be [codes_p (n_p, F), codes_c (n_c, F), codes_r (n_r, F)]")
        if [x.shape[0] for x in c] != [x.shape[0] for x in codes_list[0]]:
            raise ValueError("the clips disagree on the quantizer counts (n_p, n_c, n_r)")
    hop = model.quantizer.hop_length
    lengths = _clip_lengths(model, [c[0] for c in codes_list], "codes", per_item=hop)
    _need_gpu(timbres, "timbres")
    out = [None] * len(codes_list)
    for group in plan_groups(lengths, max_batch_samples):
        codes = [torch.nn.utils.rnn.pad_sequence([codes_list[i][s].t() for i in group], batch_first=True).transpose(1, 2).contiguous()
                 for s in range(3)]
        timbre = torch.stack([timbres[i].reshape(-1) for i in group])
        wave = decode_codes(model, codes, timbre)
        if ratio is not None:
            lens = ops.h2d(torch.tensor([lengths[i] for i in group], dtype=torch.int32), wave.device)
            wave = ops.resample(wave, MODEL_RATE, sample_rate, lens=lens, quality=quality)
        for j, i in enumerate(group):
            out[i] = wave[j, :, :lengths[i] if ratio is None else -(-lengths[i] * ratio[1] // ratio[0])]
    return out


@torch.no_grad()
def reconstruct_clips(model, waves, n_c=2, max_batch_samples=MAX_BATCH_SAMPLES, sample_rate=MODEL_RATE, quality="best"):
    """encode_clips then decode_clips with every clip's own timbre: list of waves (1, 300 (T_i // 300)) -- at sample_rate,
    which is the rate of the clips going in and of the waves coming out."""
    clips = encode_clips(model, waves, n_c=n_c, max_batch_samples=max_batch_samples, sample_rate=sample_rate, quality=quality)
    return decode_clips(model, [c["codes"] for c in clips], [c["timbre"] for c in clips], max_batch_samples=max_batch_samples,
                        sample_rate=sample_rate, quality=quality)


# ------------------------------------------------------------------------------------ voice conversion of clip lists
def edge_plan(redecoder):
    """-> [(name, columns per frame, n, pad mode)], in execution order: every conv of redecoder.encoder (the WaveNet) and
    redecoder.decoder that looks to the right of its output column, with the n columns it reads behind a clip's end and what it
    expects there (its own rule: SConv1d.edge_rule / SConvTranspose1d.edge_rule).  These are the ops.edge_tail_ launches of
    Redecoder.forward_ragged and Decoder.forward_ragged, each on the conv's input.  Causal modules contribute nothing; a
    non-causal strided SConv1d raises NotImplementedError naming it.  Host only: no launch."""
    from .layers import SConv1d, SConvTranspose1d
    plan = []
    for key in ("encoder", "decoder"):
        cols = 1
        for name, m in redecoder[key].named_modules():
            if not isinstance(m, (SConv1d, SConvTranspose1d)):
                continue
            try:
                rule = m.edge_rule()
            except NotImplementedError as e:
                raise NotImplementedError(f"{key}.{name}: {e}") from None
            if rule is not None:
                plan.append((f"{key}.{name}", cols, rule[0], rule[1]))
            if isinstance(m, SConvTranspose1d):
                cols *= m.stride
    return plan


def ragged_slack_frames(redecoder):
    """Frames a padded batch must hold behind its longest clip: every edge of edge_plan has to fit into the tensor, so that the
    kernel's own padding at the end of the tensor only serves columns nobody keeps.  max ceil(n / columns per frame)."""
    return max((-(-n // cols) for _, cols, n, _ in edge_plan(redecoder)), default=0)


def min_redecode_frames(redecoder):
    """Shortest clip whose every reflection stays inside the clip: max n // (columns per frame) + 1 over the reflect edges."""
    from . import ops
    return max((n // cols + 1 for _, cols, n, mode in edge_plan(redecoder) if mode == ops.PAD_REFLECT), default=0)


def _redecoder_hop(redecoder):
    from .layers import SConvTranspose1d
    hop = 1
    for m in redecoder.decoder.modules():
        if isinstance(m, SConvTranspose1d):
            hop *= m.stride
    return hop


def _check_redecode(redecoder, frames, n_c):
    """The host-side checks redecode_clips and convert_clips share, before any launch."""
    tables = redecoder.encoder.n_c_codebooks
    if not 0 <= n_c <= tables:
        raise ValueError(f"n_c = {n_c}: the redecoder has {tables} content tables")
    need = max(min_redecode_frames(redecoder), 1)
    for i, F in enumerate(frames):
        if F < need:
            raise ValueError(f"clip {i} has {F} frames; the shortest clip the redecoder takes has {need} frames "
                             "(its longest reflect padding must stay inside the clip)")


@torch.no_grad()
def redecode_clips(redecoder, codes_list, timbres, use_p_code=False, n_c=1, max_batch_samples=MAX_BATCH_SAMPLES,
                   sample_rate=MODEL_RATE, quality="best"):
    """Codes of clips of different lengths + one timbre per clip -> list of waves (1, 300 F_i) through the voice-conversion
    redecoder, in the caller's order: the counterpart of decode_clips for build_model(..., stage="redecoder"), causal,
    non-causal (the shipped configuration) or mixed.  codes_list[i] = [p (n_p, F_i), c (>= n_c, F_i), ...] int64 as encode_clips
    returns them; timbres[i] (1024,): the target speaker's.  use_p_code / n_c as in Redecoder.forward (the reference converts with
    use_p_code=False, n_c=1).

    Per group of plan_groups (on the lengths plus ragged_slack_frames) the codes are padded with code 0 to F' = longest clip +
    slack frames and go through one Redecoder.forward_ragged and one Decoder.forward_ragged, which write every non-causal
    conv's padding behind each clip's own end (edge_plan); every wave is cropped to its clip and equals the B = 1 calls
    `redecoder.decoder(redecoder.encoder(p, c, timbre, ...))` on that clip alone within fp32 noise.  sample_rate: as decode_clips."""
    from . import ops
    ratio = None
    if sample_rate != MODEL_RATE:
        geo = ops.resample_table(MODEL_RATE, sample_rate, quality)
        ratio = (geo["o"], geo["n"])
    codes_list = [list(c) for c in codes_list]
    if not codes_list:
        return []
    timbres = list(timbres)
    if len(timbres) != len(codes_list):
        raise ValueError(f"{len(codes_list)} clips but {len(timbres)} timbres")
    for c in codes_list:
        if len(c) < 2 or any(not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != c[0].shape[1] for x in c):
            raise ValueError("every clip's codes must be [codes_p (n_p, F), codes_c (n_c, F), ...]")
        if [x.shape[0] for x in c[:2]] != [x.shape[0] for x in codes_list[0][:2]]:
            raise ValueError("the clips disagree on the quantizer counts (n_p, n_c)")
    frames = [int(c[0].shape[1]) for c in codes_list]
    _check_redecode(redecoder, frames, n_c)
    if n_c > codes_list[0][1].shape[0]:
        raise ValueError(f"n_c = {n_c} but the clips carry {codes_list[0][1].shape[0]} content code rows")
    _need_gpu([x for c in codes_list for x in c[:2]], "codes")
    _need_gpu(timbres, "timbres")
    hop, slack = _redecoder_hop(redecoder), ragged_slack_frames(redecoder)
    out = [None] * len(codes_list)
    for group in plan_groups([hop * (F + slack) for F in frames], max_batch_samples):
        Fp = max(frames[i] for i in group) + slack
        codes = [torch.stack([torch.nn.functional.pad(codes_list[i][s], (0, Fp - frames[i])) for i in group]) for s in range(2)]
        timbre = torch.stack([timbres[i].reshape(-1) for i in group])
        lens = ops.h2d(torch.tensor([frames[i] for i in group], dtype=torch.int32), timbre.device)
        z = redecoder.encoder.forward_ragged(codes[0], codes[1], timbre, lens, use_p_code=use_p_code, n_c=n_c)
        wave = redecoder.decoder.forward_ragged(z, lens)
        if ratio is not None:
            lens_s = ops.h2d(torch.tensor([hop * frames[i] for i in group], dtype=torch.int32), wave.device)
            wave = ops.resample(wave, MODEL_RATE, sample_rate, lens=lens_s, quality=quality)
        for j, i in enumerate(group):
            n = hop * frames[i]
            out[i] = wave[j, :, :n if ratio is None else -(-n * ratio[1] // ratio[0])]
    return out


@torch.no_grad()
def convert_clips(codec, redecoder, sources, targets, use_p_code=False, n_c=1, max_batch_samples=MAX_BATCH_SAMPLES,
                  sample_rate=MODEL_RATE, quality="best"):
    """Zero-shot voice conversion of a list of clips (reconstruct_redecoder.py:110-122 per clip): sources[i] (T_i,) or (1, T_i)
    spoken with the voice of targets[i] -> list of waves (1, 300 (T_i // 300)) in the caller's order.  targets: one clip per
    source, or a single clip (a tensor, or a list of one) for all of them.  Sources and targets go through
    encode_clips(codec, ., n_c=2); clip i's codes are redecoded with target i's timbre by redecode_clips.  sample_rate is the
    rate of the sources, the targets and the output."""
    sources = list(sources)
    targets = [targets] if isinstance(targets, torch.Tensor) else list(targets)
    if len(targets) not in (1, len(sources)):
        raise ValueError(f"{len(sources)} sources but {len(targets)} targets (one per source, or a single one for all)")
    if not sources:
        return []
    from . import ops
    ratio = None
    if sample_rate != MODEL_RATE:
        geo = ops.resample_table(sample_rate, MODEL_RATE, quality)
        ratio = (geo["o"], geo["n"])
    hop = codec.quantizer.hop_length
    _check_redecode(redecoder, [n // hop for n in _clip_lengths(codec, sources, "sources", ratio=ratio)], n_c)
    kw = dict(max_batch_samples=max_batch_samples, sample_rate=sample_rate, quality=quality)
    src = encode_clips(codec, sources, n_c=2, **kw)
    tgt = encode_clips(codec, targets, n_c=2, **kw)
    if len(tgt) == 1:
        tgt = tgt * len(src)
    return redecode_clips(redecoder, [s["codes"] for s in src], [t["timbre"] for t in tgt], use_p_code=use_p_code, n_c=n_c, **kw)


# ------------------------------------------------------------------------------------ recordings of any length
LONG_CHUNK_SECONDS = 30      # default chunk of the *_long calls: the fastest of 2 / 10 / 30 s measured


def plan_long(T, chunk_samples, hop=300):
    """Chunk plan of the *_long calls for a T-sample recording: -> (cropped length 300 (T // 300), [(start, end)] or None).
    None: the cropped signal fits one chunk and goes through the whole-clip path.  Otherwise the first chunk is exactly
    chunk_samples (ChunkedCodec.prime), the others up to chunk_samples (push), the last one what is left (a multiple of 300)."""
    chunk_samples = int(chunk_samples)
    if chunk_samples % 2400 or chunk_samples < 4800:
        raise ValueError(f"a chunk must be a multiple of 2400 samples and at least 4800, got {chunk_samples}")
    Tc = hop * (int(T) // hop)
    if Tc <= chunk_samples:
        return Tc, None
    return Tc, [(s, min(s + chunk_samples, Tc)) for s in range(0, Tc, chunk_samples)]


def _chunk_samples(chunk_seconds):
    n = chunk_seconds * MODEL_RATE
    if abs(n - round(n)) > 1e-6:                          # 0.2 s is 4800 samples, whatever 0.2 * 24000 rounds to
        raise ValueError(f"chunk_seconds = {chunk_seconds} is no whole number of samples at {MODEL_RATE} Hz")
    return int(round(n))


def _long_wave(model, wave, what):
    from .streaming import _first_non_causal
    _need_gpu([wave], what)
    if wave.dim() != 3 or wave.shape[1] != 1 or wave.dtype != torch.float32:
        raise ValueError(f"{what} must be float32 (B, 1, T), got {wave.dtype} {tuple(wave.shape)}")
    bad = _first_non_causal(model, ("encoder", "decoder"), "model")
    if bad is not None:
        raise NotImplementedError(f"{bad} is not causal: the chunked calls need the causal configuration "
                                  "(a chunk cannot wait for the samples to the right of it)")


@torch.no_grad()
def encode_long(model, wave, n_c=2, chunk_seconds=LONG_CHUNK_SECONDS, timbre=None, timbre_seconds=None):
    """A recording of any length -> codes and timbre in the memory of one chunk (plus the frame-rate tensors of the timbre):

        enc = encode_long(model, wave)                  # wave (B, 1, T) float32 on the GPU, 24 kHz, equal lengths
        enc == dict(codes=[p (B, 1, F), c (B, n_c, F), r (B, 3, F)] int64, timbre=(B, 1024)),  F = T // 300

    The signal is cropped to 300 F samples first; the codes are those of `model.encoder` -> `model.quantizer` on the cropped
    signal, produced chunk_seconds at a time by streaming.ChunkedCodec (encode_only).  For T not a multiple of 300 the last four
    prosody frames can therefore differ from the single-clip call on the uncropped signal, which reflects at the uncropped end.
    timbre: taken as given (B, 1024), else FAquantizer.timbre_long over the whole recording, or over its first timbre_seconds.
    The codes do not depend on the timbre.  A cropped signal of at most one chunk goes through the whole-clip calls."""
    from .streaming import ChunkedCodec
    _long_wave(model, wave, "wave")
    Tc, plan = plan_long(wave.shape[-1], _chunk_samples(chunk_seconds), model.quantizer.hop_length)
    if Tc < wave.shape[-1]:
        wave = wave[:, :, :Tc]
    q = model.quantizer
    if plan is None:
        wave = wave.contiguous()
        out = q(model.encoder(wave), wave, n_c=n_c, return_codes=True)
        own, codes = out[4], out[5]
    else:
        own = None
        sess = ChunkedCodec(model, torch.zeros(wave.shape[0], q.in_dim, device=wave.device), n_c=n_c,
                            chunk_samples=plan[0][1], encode_only=True)
        parts = [sess.prime(wave[:, :, plan[0][0]:plan[0][1]])]
        parts += [sess.push(wave[:, :, s:e]) for s, e in plan[1:]]
        parts.append(sess.finish())
        codes = [torch.cat([p["codes"][r] for p in parts if p["codes"] is not None], dim=-1) for r in range(3)]
    if timbre is None:
        if timbre_seconds is not None:
            n = min(Tc, _chunk_samples(timbre_seconds))
            timbre = q.timbre_long(wave[:, :, :n])
        elif own is not None:
            timbre = own
        else:
            timbre = q.timbre_long(wave)
    return dict(codes=codes, timbre=timbre)


@torch.no_grad()
def decode_long(model, codes, timbre, chunk_seconds=LONG_CHUNK_SECONDS):
    """Codes of any length + timbre -> (B, 1, 300 F), decode_codes within fp32 noise, chunk_seconds of frames at a time through
    streaming.StreamingDecoder (no graphs).  At most one chunk of frames goes through decode_codes itself."""
    from .streaming import StreamingDecoder, _first_non_causal
    hop = model.quantizer.hop_length
    chunk = _chunk_samples(chunk_seconds)
    plan_long(chunk, chunk, hop)                                            # the chunk rule
    bad = _first_non_causal(model, ("decoder",), "model")
    if bad is not None:
        raise NotImplementedError(f"{bad} is not causal: the chunked calls need the causal configuration")
    model.quantizer._check_decode_inputs(codes, timbre)
    F, k = codes[0].shape[-1], chunk // hop
    if F <= k:
        return decode_codes(model, codes, timbre)
    rx = StreamingDecoder(model, timbre, use_graphs=False, max_frames=k)
    if k < rx.min_prime:
        raise ValueError(f"a chunk of {k} frames is below the decoder's first chunk of {rx.min_prime} frames")
    out = torch.empty(codes[0].shape[0], 1, hop * F, device=timbre.device, dtype=torch.float32)
    for f0 in range(0, F, k):
        f1 = min(F, f0 + k)
        part = [c[:, :, f0:f1] for c in codes]
        out[:, :, hop * f0:hop * f1] = rx.prime(part) if f0 == 0 else rx.push(part)
    return out


@torch.no_grad()
def reconstruct_long(model, wave, n_c=2, chunk_seconds=LONG_CHUNK_SECONDS, timbre=None, timbre_seconds=None):
    """encode_long then decode_long: (B, 1, T) -> (B, 1, 300 (T // 300)); timbre: another speaker's for a timbre swap."""
    enc = encode_long(model, wave, n_c=n_c, chunk_seconds=chunk_seconds, timbre=timbre, timbre_seconds=timbre_seconds)
    return decode_long(model, enc["codes"], enc["timbre"], chunk_seconds=chunk_seconds)


# ------------------------------------------------------------------------------------ the bitstream
def code_bits(model):
    """Field width of the model's codes: ceil(log2(codebook_size)), 10 for the shipped 1024-entry codebooks."""
    return max(1, (model.quantizer.prosody_quantizer.codebook_size - 1).bit_length())


def _blobs_from_codes(model, codes, timbre, frames, sample_rate, n_samples, lens=None, input_db=None):
    """codes [p, c, r] (B, n, T) int64 on the device (strided views welcome) -> B container blobs: one ops.pack_codes launch, one
    device-to-host copy of the uint8 rows (and one of the timbres, when they are stored), then host slicing to every clip's own
    payload_bytes.  frames[b] / n_samples[b]: clip b's frame count and original length; lens: the frame counts on the device
    when they differ.  input_db (B,) float64 on the device, or None: the loudness the clips had before they were levelled; it
    rides as one float32 behind every packed row, in the same copy, and goes into the blob (flag bit2)."""
    import numpy as np
    from . import bitstream, ops
    bits = code_bits(model)
    n_q = tuple(int(c.shape[1]) for c in codes)
    loud = None
    if input_db is None:
        rows = ops.pack_codes(codes, bits=bits, lens=lens).cpu().numpy()
    else:
        B, T = codes[0].shape[0], codes[0].shape[-1]
        rb = ops.codes_row_bytes(T, sum(n_q), bits)
        buf = torch.empty(B, rb + 4, device=input_db.device, dtype=torch.uint8)
        ops.pack_codes(codes, bits=bits, lens=lens, out=buf)
        buf[:, rb:].view(torch.float32).copy_(input_db.reshape(B, 1))
        rows = buf.cpu().numpy()
        loud = np.ascontiguousarray(rows[:, rb:]).view("<f4").reshape(B)
    tim = timbre.detach().to(torch.float32).cpu().numpy() if timbre is not None else None
    q = model.quantizer
    out = []
    for b, F in enumerate(frames):
        head = dict(bits=bits, n_q=n_q, sample_rate=sample_rate, n_frames=F, n_samples=n_samples[b],
                    codebook_size=q.prosody_quantizer.codebook_size, timbre_dim=q.in_dim,
                    input_db=float(loud[b]) if loud is not None else None)
        out.append(bitstream.write(head, tim[b].tobytes() if tim is not None else None,
                                   rows[b, :bitstream.payload_bytes(F, sum(n_q), bits)].tobytes()))
    return out


def _check_n_r(model, n_r):
    top = model.quantizer.residual_quantizer.n_codebooks
    if not 0 <= n_r <= top:
        raise ValueError(f"n_r = {n_r}: the model has {top} residual quantizers")


@torch.no_grad()
def compress(model, wave, n_c=2, n_r=3, with_timbre=True, sample_rate=MODEL_RATE, quality="best", normalize_db=None):
    """Audio -> bytes.  wave (B, 1, T) float32 on the GPU -> list of B container blobs (bitstream.py); one clip (T,) or (1, T)
    -> one blob.

        blob = compress(model, wave)                         # 4.8 kbit/s of payload + the timbre (4 KiB) + 36 bytes
        wave_hat = decompress(model, blob)                   # decode_codes(model, codes, timbre) of the same forward

    The codes are those of `model.encoder` -> `model.quantizer(z, wave, n_c, return_codes=True)` on the batch; n_r < 3 stores
    the first n_r residual rows only (the strided view codes_r[:, :n_r]: bitrate scalability, nothing is re-encoded).  One
    ops.pack_codes launch and one device-to-host copy of the packed rows per call.  with_timbre=False leaves the timbre out
    (decompress then needs timbre=).  sample_rate: the rate of `wave`; other than 24000 it is resampled first (ops.resample,
    `quality`), and the header records the rate so that decompress returns audio at it.

    normalize_db: None encodes the audio at the level it has.  A number levels it first, in the reference's order (dac/model/
    base.py:166-180): resample to 24 kHz, measure the integrated loudness (ops.loudness), bring it to normalize_db LUFS, guard
    the peak (ops.normalize_loudness), then encoder and quantizer -- the timbre is that of the levelled audio.  The measured
    loudness travels to the host with the packed rows and is stored in the blob (Header.input_db); decompress restores it."""
    from . import ops
    _need_gpu([wave], "wave")
    _check_n_r(model, n_r)
    single = wave.dim() <= 2
    if single:
        if not (wave.dim() == 1 or wave.shape[0] == 1):
            raise ValueError(f"one clip must be (T,) or (1, T), a batch (B, 1, T); got {tuple(wave.shape)}")
        wave = wave.reshape(1, 1, -1)
    if wave.dim() != 3 or wave.shape[1] != 1 or wave.dtype != torch.float32:
        raise ValueError(f"wave must be float32 (B, 1, T), got {wave.dtype} {tuple(wave.shape)}")
    B, n_in = wave.shape[0], wave.shape[-1]
    x = wave.contiguous()
    if sample_rate != MODEL_RATE:
        x = ops.resample(x, sample_rate, MODEL_RATE, quality=quality)
    _clip_lengths(model, [x[0, 0]], "wave")
    input_db = None
    if normalize_db is not None:
        x, input_db, _ = ops.normalize_loudness(x, float(normalize_db), MODEL_RATE)
    out = model.quantizer(model.encoder(x), x, n_c=n_c, return_codes=True)
    timbre, codes = out[4], out[5]
    codes = [codes[0], codes[1], codes[2][:, :n_r]]
    F = codes[0].shape[-1]
    blobs = _blobs_from_codes(model, codes, timbre if with_timbre else None, [F] * B, sample_rate, [n_in] * B, input_db=input_db)
    return blobs[0] if single else blobs


@torch.no_grad()
def compress_clips(model, waves, n_c=2, n_r=3, with_timbre=True, max_batch_samples=MAX_BATCH_SAMPLES, sample_rate=MODEL_RATE,
                   quality="best", normalize_db=None):
    """Clips of different lengths -> one container blob per clip, in the caller's order: encode_clips' groups and forward, then
    per group one ops.pack_codes launch with the group's frame counts as `lens` and one device-to-host copy.  normalize_db: as
    in compress, every clip measured and levelled on its own samples (ops.normalize_loudness with the group's lengths)."""
    from . import ops
    _check_n_r(model, n_r)
    ratio = None
    if sample_rate != MODEL_RATE:
        geo = ops.resample_table(sample_rate, MODEL_RATE, quality)
        ratio = (geo["o"], geo["n"])
    waves = list(waves)
    if not waves:
        return []
    for w in waves:
        if isinstance(w, torch.Tensor) and not (w.dim() == 1 or (w.dim() == 2 and w.shape[0] == 1)):
            raise ValueError(f"every clip must be (T,) or (1, T), got {tuple(w.shape)}")
    lengths = _clip_lengths(model, waves, "clips", ratio=ratio)
    dev, hop = waves[0].device, model.quantizer.hop_length
    out = [None] * len(waves)
    for group in plan_groups(lengths, max_batch_samples):
        batch = torch.nn.utils.rnn.pad_sequence([waves[i].reshape(-1).to(torch.float32) for i in group], batch_first=True).unsqueeze(1)
        lens = ops.h2d(torch.tensor([lengths[i] for i in group], dtype=torch.int32), dev)
        if ratio is not None:
            lens_in = ops.h2d(torch.tensor([waves[i].shape[-1] for i in group], dtype=torch.int32), dev)
            batch = ops.resample(batch, sample_rate, MODEL_RATE, lens=lens_in, quality=quality)
        input_db = None
        if normalize_db is not None:
            batch, input_db, _ = ops.normalize_loudness(batch, float(normalize_db), MODEL_RATE, lens=lens)
        z = model.encoder(batch)
        _, codes, timbre, frame_lens = model.quantizer.forward_ragged(z, batch, lens, n_c=n_c)
        codes = [codes[0], codes[1], codes[2][:, :n_r]]
        blobs = _blobs_from_codes(model, codes, timbre if with_timbre else None, [lengths[i] // hop for i in group], sample_rate,
                                  [int(waves[i].shape[-1]) for i in group], lens=frame_lens, input_db=input_db)
        for j, i in enumerate(group):
            out[i] = blobs[j]
    return out


def _parse_blobs(model, blobs):
    """bitstream.read of every blob + the checks against the model -> [(Header, timbre ndarray | None, payload)]."""
    from . import bitstream
    q = model.quantizer
    parsed = []
    for i, blob in enumerate(blobs):
        hdr, tim, payload = bitstream.read(blob)
        if hdr.is_stream_header:
            raise ValueError(f"blob {i} is a stream header (streaming.CodeDepacketizer reads those), not a clip")
        if hdr.codebook_size != q.prosody_quantizer.codebook_size:
            raise ValueError(f"blob {i}: codebook_size {hdr.codebook_size}, the model has {q.prosody_quantizer.codebook_size}")
        if hdr.timbre_dim != q.in_dim:
            raise ValueError(f"blob {i}: timbre_dim {hdr.timbre_dim}, the model has {q.in_dim}")
        for n, rvq, name in zip(hdr.n_q, (q.prosody_quantizer, q.content_quantizer, q.residual_quantizer), "pcr"):
            if n > rvq.n_codebooks:
                raise ValueError(f"blob {i}: n_{name} = {n}, the model has {rvq.n_codebooks} such quantizers")
        if hdr.n_frames < 1:
            raise ValueError(f"blob {i} has no frames")
        parsed.append((hdr, tim, payload))
    return parsed


def _timbres_for(model, parsed, timbre, dev):
    """(B, dim) float32 on the device: the override (one (dim,) / (1, dim) vector for all, or (B, dim), or a list), else the
    stored timbres in one host-to-device copy."""
    import numpy as np
    from . import ops
    B, dim = len(parsed), model.quantizer.in_dim
    if timbre is not None:
        if isinstance(timbre, (list, tuple)):
            _need_gpu(timbre, "timbre")
            timbre = torch.stack([t.reshape(-1) for t in timbre])
        _need_gpu([timbre], "timbre")
        timbre = timbre.reshape(-1, timbre.shape[-1]).to(torch.float32)
        if timbre.shape[0] == 1 and B > 1:
            timbre = timbre.expand(B, -1)
        if tuple(timbre.shape) != (B, dim):
            raise ValueError(f"timbre must be ({dim},) or ({B}, {dim}), got {tuple(timbre.shape)}")
        return timbre.contiguous()
    for i, (_, tim, _) in enumerate(parsed):
        if tim is None:
            raise ValueError(f"blob {i} carries no timbre (compressed with with_timbre=False): pass timbre=")
    return ops.h2d(torch.from_numpy(np.stack([tim for _, tim, _ in parsed])), dev)


def _codes_from_payloads(headers, payloads, dev, ragged):
    """Payloads of clips that agree on (n_q, bits) -> [p, c, r] (B, n, T) int64 on the device, T the longest clip, code 0 behind
    every clip's own frames: one host-to-device copy of the zero-padded rows and one ops.unpack_codes launch."""
    import numpy as np
    from . import ops
    h0 = headers[0]
    T = max(h.n_frames for h in headers)
    rows = np.zeros((len(headers), ops.codes_row_bytes(T, h0.Q, h0.bits)), dtype=np.uint8)
    for b, p in enumerate(payloads):
        rows[b, :len(p)] = np.frombuffer(p, dtype=np.uint8)
    lens = ops.h2d(torch.tensor([h.n_frames for h in headers], dtype=torch.int32), dev) if ragged else None
    return ops.unpack_codes(ops.h2d(torch.from_numpy(rows), dev), h0.n_q, T, bits=h0.bits, lens=lens)


def _blob_device(model):
    return next(model.decoder.parameters()).device


@torch.no_grad()
def _restore_loudness(wave, headers, lens=None):
    """The decoder's side of compress(normalize_db=): wave (B, 1, T) at 24 kHz, decoded from blobs with `headers`.  Rows whose
    blob carries input_db are measured (ops.loudness, on their own lens[b] samples) and scaled by 10^((input_db - L_out) / 20), in
    place and without a peak guard (dac/model/base.py:285); a row that measures -70 is left as it is, and so is a row without
    the field.  One host-to-device copy of the targets, no host read."""
    from . import ops
    if not any(h.input_db is not None for h in headers):
        return wave
    target = ops.h2d(torch.tensor([h.input_db if h.input_db is not None else float("nan") for h in headers], dtype=torch.float64),
                     wave.device)
    L = ops.loudness(wave, MODEL_RATE, lens=lens)
    ops.loudness_gain(wave, L, target_rows=target, lens=lens, guard=False, out=wave)
    return wave


@torch.no_grad()
def loudness_clips(waves, sample_rate=MODEL_RATE, max_batch_samples=MAX_BATCH_SAMPLES):
    """Integrated loudness (ITU-R BS.1770-4, LUFS) of clips of different lengths -> list of floats in the caller's order.  The
    clips (T_i,) or (1, T_i), float32 on the GPU at sample_rate (a multiple of 10), go through plan_groups' zero-padded groups
    with their lengths: one ops.loudness call and one device-to-host copy per group; a clip measures what it measures alone,
    whatever it is grouped with."""
    from . import ops
    ops._kweight_tables(sample_rate)                                # ValueError: the rate
    waves = list(waves)
    if not waves:
        return []
    _need_gpu(waves, "clips")
    for w in waves:
        if not (w.dim() == 1 or (w.dim() == 2 and w.shape[0] == 1)):
            raise ValueError(f"every clip must be (T,) or (1, T), got {tuple(w.shape)}")
    lengths = [int(w.shape[-1]) for w in waves]
    out = [None] * len(waves)
    for group in plan_groups(lengths, max_batch_samples):
        batch = torch.nn.utils.rnn.pad_sequence([waves[i].reshape(-1).to(torch.float32) for i in group], batch_first=True)
        lens = ops.h2d(torch.tensor([lengths[i] for i in group], dtype=torch.int32), batch.device)
        L = ops.loudness(batch, sample_rate, lens=lens).cpu().tolist()
        for j, i in enumerate(group):
            out[i] = L[j]
    return out


@torch.no_grad()
def level_clips(waves, sample_rate=MODEL_RATE, max_batch_samples=MAX_BATCH_SAMPLES, **parameters):
    """Causal level control (ops.level) of clips of different lengths -> per clip, in the caller's order,
    ops.Levelled(y (T_i + lookahead,) float32, G (T_i // S,) float64 dB, g (T_i // S,) float64), on the device.  The clips (T_i,)
    or (1, T_i), float32 on the GPU at sample_rate (a multiple of 10), go through plan_groups' zero-padded groups with their
    lengths: one ops.level call (three C calls) per group, nothing is read back; a clip comes out as the single-clip call gives
    it, whatever it is grouped with.  **parameters: ops.level's target_db, window, max_boost_db, max_cut_db,
    ceiling_db, lookahead -- whose defaults were not tuned by listening."""
    from . import ops
    p = ops.agc_params(sample_rate, **parameters)                   # ValueError: the rate, the parameters
    waves = list(waves)
    if not waves:
        return []
    _need_gpu(waves, "clips")
    for w in waves:
        if not (w.dim() == 1 or (w.dim() == 2 and w.shape[0] == 1)):
            raise ValueError(f"every clip must be (T,) or (1, T), got {tuple(w.shape)}")
    lengths = [int(w.shape[-1]) for w in waves]
    out = [None] * len(waves)
    for group in plan_groups(lengths, max_batch_samples):
        batch = torch.nn.utils.rnn.pad_sequence([waves[i].reshape(-1).to(torch.float32) for i in group], batch_first=True)
        lens = ops.h2d(torch.tensor([lengths[i] for i in group], dtype=torch.int32), batch.device)
        r = ops.level(batch, sample_rate, lens=lens, **parameters)
        for j, i in enumerate(group):
            n = lengths[i] // p.S
            out[i] = ops.Levelled(r.y[j, :lengths[i] + p.LA], r.G[j, :n], r.g[j, :n])
    return out


@torch.no_grad()
def denoise_clips(waves, max_batch_samples=MAX_BATCH_SAMPLES, **parameters):
    """Spectral noise suppression (ops.denoise) of clips of different lengths -> per clip, in the caller's order,
    ops.Denoised(y (T_i,) float32, G (ceil(T_i / 256) + 1, 257) float64), on the device.  The clips (T_i,) or (1, T_i), float32
    on the GPU at any sample rate, go through plan_groups' zero-padded groups with their lengths: one ops.denoise call (three
    C calls) per group, nothing is read back; a clip comes out as the single-clip call gives it, bit for bit, whatever it is
    grouped with.  **parameters: ops.denoise's M, W, over, max_atten_db -- whose defaults were not tuned by listening."""
    from . import ops
    ops.ns_params(**parameters)                                     # ValueError: the parameters
    waves = list(waves)
    if not waves:
        return []
    _need_gpu(waves, "clips")
    for w in waves:
        if not (w.dim() == 1 or (w.dim() == 2 and w.shape[0] == 1)):
            raise ValueError(f"every clip must be (T,) or (1, T), got {tuple(w.shape)}")
    lengths = [int(w.shape[-1]) for w in waves]
    out = [None] * len(waves)
    for group in plan_groups(lengths, max_batch_samples):
        batch = torch.nn.utils.rnn.pad_sequence([waves[i].reshape(-1).to(torch.float32) for i in group], batch_first=True)
        lens = ops.h2d(torch.tensor([lengths[i] for i in group], dtype=torch.int32), batch.device)
        r = ops.denoise(batch, lens=lens, **parameters)
        for j, i in enumerate(group):
            out[i] = ops.Denoised(r.y[j, :lengths[i]], r.G[j, :ops.ns_frames(lengths[i])])
    return out


def echo_cancel_clips(mics, fars, max_batch_samples=MAX_BATCH_SAMPLES, **parameters):
    """Echo cancellation (ops.echo_cancel) of clips of different lengths -> per clip, in the caller's order,
    ops.EchoCancelled(e (T_i,) float32, W (P, 257, 2) float64, stats (ceil(T_i / 256), 3) float64), on the device.  mics[i] and
    fars[i], (T_i,) or (1, T_i), float32 on the GPU, are one call's microphone and far-end signals, of one length.  They go
    through plan_groups' zero-padded groups with their lengths: one ops.echo_cancel call (one C call) per group, nothing is
    read back; a clip comes out as the single-clip call gives it, bit for bit, whatever it is grouped with.  **parameters:
    ops.echo_cancel's P, mu, beta, delta, delay -- whose defaults were not tuned by listening; with delay="auto" also
    ops.echo_delay_params', and each group is two C calls."""
    from . import ops
    if parameters.get("delay") == "auto":                           # ValueError: the parameters
        ops.aec_params(**{k: v for k, v in parameters.items() if k != "delay" and k not in ops.ECHO_DELAY_NAMES})
        ops.echo_delay_params(**{k: v for k, v in parameters.items() if k in ops.ECHO_DELAY_NAMES})
    else:
        ops.aec_params(**parameters)
    mics, fars = list(mics), list(fars)
    if len(mics) != len(fars):
        raise ValueError(f"{len(mics)} microphone clips and {len(fars)} far-end clips")
    if not mics:
        return []
    _need_gpu(mics, "clips")
    _need_gpu(fars, "clips")
    for m, f in zip(mics, fars):
        if not (m.dim() == 1 or (m.dim() == 2 and m.shape[0] == 1)) or not (f.dim() == 1 or (f.dim() == 2 and f.shape[0] == 1)):
            raise ValueError(f"every clip must be (T,) or (1, T), got {tuple(m.shape)} and {tuple(f.shape)}")
        if m.shape[-1] != f.shape[-1]:
            raise ValueError(f"a microphone clip of {m.shape[-1]} samples with a far-end clip of {f.shape[-1]}")
    lengths = [int(m.shape[-1]) for m in mics]
    out = [None] * len(mics)
    for group in plan_groups(lengths, max_batch_samples):
        mic = torch.nn.utils.rnn.pad_sequence([mics[i].reshape(-1).to(torch.float32) for i in group], batch_first=True)
        far = torch.nn.utils.rnn.pad_sequence([fars[i].reshape(-1).to(torch.float32) for i in group], batch_first=True)
        lens = ops.h2d(torch.tensor([lengths[i] for i in group], dtype=torch.int32), mic.device)
        r = ops.echo_cancel(mic, far, lens=lens, **parameters)
        for j, i in enumerate(group):
            out[i] = ops.EchoCancelled(r.e[j, :lengths[i]], r.W[j], r.stats[j, :ops.aec_blocks(lengths[i])])
    return out


def echo_delay_clips(mics, fars, max_batch_samples=MAX_BATCH_SAMPLES, **parameters):
    """The playout-to-capture delay (ops.echo_delay) of clips of different lengths -> per clip, in the caller's
    order, (locked, conf): the latched delay in samples after the clip's last frame (-1: never latched) and that frame's
    confidence, on the host; (-1, 0.0) for a clip under 512 samples, which has no frame.  mics[i] and fars[i] as
    echo_cancel_clips takes them.  They go through plan_groups' zero-padded groups with their lengths: one ops.echo_delay call
    (one C call) and one device-to-host copy per group.  **parameters: ops.echo_delay_params', not tuned by listening."""
    from . import ops
    p = ops.echo_delay_params(**parameters)                         # ValueError: the parameters
    mics, fars = list(mics), list(fars)
    if len(mics) != len(fars):
        raise ValueError(f"{len(mics)} microphone clips and {len(fars)} far-end clips")
    if not mics:
        return []
    _need_gpu(mics, "clips")
    _need_gpu(fars, "clips")
    for m, f in zip(mics, fars):
        if not (m.dim() == 1 or (m.dim() == 2 and m.shape[0] == 1)) or not (f.dim() == 1 or (f.dim() == 2 and f.shape[0] == 1)):
            raise ValueError(f"every clip must be (T,) or (1, T), got {tuple(m.shape)} and {tuple(f.shape)}")
        if m.shape[-1] != f.shape[-1]:
            raise ValueError(f"a microphone clip of {m.shape[-1]} samples with a far-end clip of {f.shape[-1]}")
    lengths = [int(m.shape[-1]) for m in mics]
    out = [None] * len(mics)
    for group in plan_groups(lengths, max_batch_samples):
        mic = torch.nn.utils.rnn.pad_sequence([mics[i].reshape(-1).to(torch.float32) for i in group], batch_first=True)
        far = torch.nn.utils.rnn.pad_sequence([fars[i].reshape(-1).to(torch.float32) for i in group], batch_first=True)
        lens = ops.h2d(torch.tensor([lengths[i] for i in group], dtype=torch.int32), mic.device)
        state = ops.edelay_state(len(group), p, mic.device)
        ops.echo_delay(mic, far, lens=lens, state=state, **parameters)
        last = torch.cat([state["pol"][:, 2].to(torch.float64)[:, None], state["conf_last"][:, None]], dim=1).cpu()     # the one copy
        for j, i in enumerate(group):
            out[i] = (int(last[j, 0]), float(last[j, 1]))
    return out


def active_segments(flags, frame, length):
    """flags: one clip's 0 / 1 frame flags (host sequence) -> [(start_sample, end_sample)] of its runs of active frames, the last
    end clipped to the clip's length.  Host only."""
    segs, start = [], None
    for f, a in enumerate(list(flags) + [0]):
        if a and start is None:
            start = f
        elif not a and start is not None:
            segs.append((start * frame, min(f * frame, int(length))))
            start = None
    return segs


@torch.no_grad()
def vad_clips(waves, max_batch_samples=MAX_BATCH_SAMPLES, **vad):
    """Voice activity of clips of different lengths -> per clip, in the caller's order, dict(flags (F_i,) uint8 on
    the host, F_i = ceil(T_i / frame); segments [(start_sample, end_sample)], the runs of active frames clipped to the clip).
    The clips (T_i,) or (1, T_i), float32 on the GPU at the model's rate, go through plan_groups' zero-padded groups with their
    lengths: one ops.vad call (two launches) and one device-to-host copy of the flags per group, the run lengths are computed
    on the host; a clip gets what it gets alone.  **vad: ops.vad's frame, window, hangover, margin_db, floor_db -- whose
    defaults were not tuned by listening."""
    from . import ops
    frame = ops.vad_params(**vad)[0]                                # ValueError: the parameters
    waves = list(waves)
    if not waves:
        return []
    _need_gpu(waves, "clips")
    for w in waves:
        if not (w.dim() == 1 or (w.dim() == 2 and w.shape[0] == 1)):
            raise ValueError(f"every clip must be (T,) or (1, T), got {tuple(w.shape)}")
    lengths = [int(w.shape[-1]) for w in waves]
    out = [None] * len(waves)
    for group in plan_groups(lengths, max_batch_samples):
        batch = torch.nn.utils.rnn.pad_sequence([waves[i].reshape(-1).to(torch.float32) for i in group], batch_first=True)
        lens = ops.h2d(torch.tensor([lengths[i] for i in group], dtype=torch.int32), batch.device)
        flags = ops.vad(batch, lens=lens, **vad)[0].cpu().numpy()
        for j, i in enumerate(group):
            fl = flags[j, :-(-lengths[i] // frame)].copy()
            out[i] = dict(flags=fl, segments=active_segments(fl.tolist(), frame, lengths[i]))
    return out


@torch.no_grad()
def trim_clips(waves, pad_frames=0, max_batch_samples=MAX_BATCH_SAMPLES, **vad):
    """Every clip cut to its speech: the slice (a view) from its first to its last active frame, widened by pad_frames frames on
    either side and kept within the clip; a clip without an active frame gives an empty tensor.  vad_clips does the work."""
    from . import ops
    frame = ops.vad_params(**vad)[0]
    waves = list(waves)
    out = []
    for w, r in zip(waves, vad_clips(waves, max_batch_samples, **vad)):
        if not r["segments"]:
            out.append(w[..., :0])
            continue
        a = max(0, r["segments"][0][0] - int(pad_frames) * frame)
        b = min(int(w.shape[-1]), r["segments"][-1][1] + int(pad_frames) * frame)
        out.append(w[..., a:b])
    return out


SCORE_METRICS = ("si_sdr", "stoi", "estoi")


@torch.no_grad()
def score_clips(refs, ests, sample_rate=MODEL_RATE, metrics=SCORE_METRICS, max_batch_samples=MAX_BATCH_SAMPLES):
    """Objective scores of estimates against references, clip by clip -> list of dicts {metric: float} in the
    caller's order.  refs[i], ests[i]: (T,) or (1, T) float32 on the GPU at sample_rate; every pair is cropped to the shorter of
    the two (the codec gives back 300 (T // 300) samples).  metrics: any of "si_sdr" (dB, ops.si_sdr), "stoi", "estoi"
    (ops.stoi_scores; NaN for a clip under 30 kept frames of 12.8 ms).  The pairs go through plan_groups' zero-padded groups with
    their lengths: per group one ops call per metric family and one device-to-host copy; a pair scores what it scores alone."""
    from . import ops
    metrics = tuple(metrics)
    for m in metrics:
        if m not in SCORE_METRICS:
            raise ValueError(f"unknown metric {m!r}; this build scores {SCORE_METRICS}")
    refs, ests = list(refs), list(ests)
    if len(refs) != len(ests):
        raise ValueError(f"{len(refs)} references but {len(ests)} estimates")
    if not refs:
        return []
    _need_gpu(refs + ests, "clips")
    for w in refs + ests:
        if not (w.dim() == 1 or (w.dim() == 2 and w.shape[0] == 1)):
            raise ValueError(f"every clip must be (T,) or (1, T), got {tuple(w.shape)}")
    lengths = [min(int(r.shape[-1]), int(e.shape[-1])) for r, e in zip(refs, ests)]
    out = [None] * len(refs)
    for group in plan_groups(lengths, max_batch_samples):
        x, y = (torch.nn.utils.rnn.pad_sequence([ws[i].reshape(-1)[:lengths[i]].to(torch.float32) for i in group], batch_first=True)
                for ws in (refs, ests))
        lens = ops.h2d(torch.tensor([lengths[i] for i in group], dtype=torch.int32), x.device)
        rows = {}
        if "si_sdr" in metrics:
            rows["si_sdr"] = ops.si_sdr(x, y, lens=lens)
        if "stoi" in metrics or "estoi" in metrics:
            s = ops.stoi_scores(x, y, sample_rate, lens)
            rows["stoi"], rows["estoi"] = s.stoi, s.estoi
        table = torch.stack([rows[m] for m in metrics]).cpu().tolist() if metrics else []
        for j, i in enumerate(group):
            out[i] = {m: table[k][j] for k, m in enumerate(metrics)}
    return out


@torch.no_grad()
def evaluate_clips(model, waves, n_c=2, sample_rate=MODEL_RATE, metrics=SCORE_METRICS, max_batch_samples=MAX_BATCH_SAMPLES,
                   quality="best"):
    """What the codec does to clips, in numbers: reconstruct_clips (encode, quantize with n_c content codebooks, decode with every
    clip's own timbre) then score_clips of the results against the inputs -> (scores, waves_out): a list of dicts as score_clips
    returns them and the reconstructed waves (1, 300 (T_i // 300)), both in the caller's order and at sample_rate."""
    waves = list(waves)
    waves_out = reconstruct_clips(model, waves, n_c=n_c, max_batch_samples=max_batch_samples, sample_rate=sample_rate, quality=quality)
    return score_clips(waves, waves_out, sample_rate=sample_rate, metrics=metrics, max_batch_samples=max_batch_samples), waves_out


@torch.no_grad()
def decompress(model, blobs, timbre=None, sample_rate=None, max_batch_samples=MAX_BATCH_SAMPLES, quality="best",
               restore_loudness=True):
    """Bytes -> audio: a list of container blobs -> list of waves (1, N_i) in the caller's order; one blob -> one wave.

    The headers are read on the host (bitstream.read: magic, version, length, CRC), the blobs grouped by their layout
    (n_p, n_c, n_r, bits) and, within one layout, by plan_groups; per group one host-to-device copy of the payload rows, one
    ops.unpack_codes launch with the clips' frame counts, then decode_clips' path (decode_codes on the padded batch, every wave
    cropped to its clip).  timbre: overrides the stored timbres (timbre swap): one vector for all blobs or one per blob;
    required for blobs written with with_timbre=False.  sample_rate: None gives every clip back at its header's rate; a value
    resamples every clip to it.  A header whose codebook_size or timbre_dim is not the model's raises ValueError.
    restore_loudness: a blob written with compress(normalize_db=) carries the loudness its audio had; the decoded 24 kHz audio
    is measured and brought back to it before resampling and cropping (_restore_loudness; blobs with and without the field may
    be mixed, the gain is per row).  False returns the audio at the level it was encoded at."""
    from . import ops
    single = isinstance(blobs, (bytes, bytearray, memoryview))
    blobs = [blobs] if single else list(blobs)
    if not blobs:
        return []
    parsed = _parse_blobs(model, blobs)
    dev = timbre[0].device if isinstance(timbre, (list, tuple)) else timbre.device if timbre is not None else _blob_device(model)
    timbres = _timbres_for(model, parsed, timbre, dev)
    hop = model.quantizer.hop_length
    need = min_clip_samples(model)
    for i, (h, _, _) in enumerate(parsed):
        if h.n_frames * hop < need:
            raise ValueError(f"blob {i} has {h.n_frames} frames; the shortest clip this path takes has {-(-need // hop)} frames")
    layouts = {}
    for i, (h, _, _) in enumerate(parsed):
        layouts.setdefault((h.n_q, h.bits, sample_rate if sample_rate is not None else h.sample_rate), []).append(i)
    out = [None] * len(blobs)
    for (_, _, rate), members in layouts.items():
        ratio = None
        if rate != MODEL_RATE:
            geo = ops.resample_table(MODEL_RATE, rate, quality)
            ratio = (geo["o"], geo["n"])
        lengths = [parsed[i][0].n_frames * hop for i in members]
        for g in plan_groups(lengths, max_batch_samples):
            group = [members[j] for j in g]
            headers = [parsed[i][0] for i in group]
            codes = _codes_from_payloads(headers, [parsed[i][2] for i in group], dev, len({h.n_frames for h in headers}) > 1)
            wave = decode_codes(model, codes, timbres if group == list(range(len(blobs))) else timbres[group])
            lens = None
            if ratio is not None or (restore_loudness and any(h.input_db is not None for h in headers)):
                lens = ops.h2d(torch.tensor([h.n_frames * hop for h in headers], dtype=torch.int32), dev)
            if restore_loudness:
                wave = _restore_loudness(wave, headers, lens)
            if ratio is not None:
                wave = ops.resample(wave, MODEL_RATE, rate, lens=lens, quality=quality)
            for j, i in enumerate(group):
                n = headers[j].n_frames * hop
                out[i] = wave[j, :, :n if ratio is None else -(-n * ratio[1] // ratio[0])]
    return out[0] if single else out


@torch.no_grad()
def compress_long(model, wave, n_c=2, n_r=3, with_timbre=True, chunk_seconds=LONG_CHUNK_SECONDS, timbre=None, timbre_seconds=None,
                  normalize_db=None):
    """encode_long into the container: wave (B, 1, T) float32 on the GPU at 24 kHz, any length -> list of B blobs.  The whole
    code stream of the recording is packed by one ops.pack_codes launch (64-bit bit offsets) and copied to the host once.
    normalize_db: as in compress; the loudness is that of the whole recording, and the levelled recording is ONE extra copy of
    it (one float per sample) that lives until the codes are packed -- the chunks are cut from it."""
    from . import ops
    _check_n_r(model, n_r)
    input_db = None
    if normalize_db is not None:
        _long_wave(model, wave, "wave")
        wave, input_db, _ = ops.normalize_loudness(wave, float(normalize_db), MODEL_RATE)
    enc = encode_long(model, wave, n_c=n_c, chunk_seconds=chunk_seconds, timbre=timbre, timbre_seconds=timbre_seconds)
    codes = [enc["codes"][0], enc["codes"][1], enc["codes"][2][:, :n_r]]
    B, F = wave.shape[0], codes[0].shape[-1]
    return _blobs_from_codes(model, codes, enc["timbre"] if with_timbre else None, [F] * B, MODEL_RATE, [int(wave.shape[-1])] * B,
                             input_db=input_db)


@torch.no_grad()
def decompress_long(model, blobs, timbre=None, chunk_seconds=LONG_CHUNK_SECONDS, restore_loudness=True):
    """Blobs of compress_long (equal frame counts and one layout, as one recording batch has) -> (B, 1, 300 F) through decode_long:
    one host-to-device copy and one ops.unpack_codes launch for the whole code stream, then the chunked decoder.
    restore_loudness: as in decompress, on the whole decoded recording, in place."""
    blobs = [blobs] if isinstance(blobs, (bytes, bytearray, memoryview)) else list(blobs)
    parsed = _parse_blobs(model, blobs)
    headers = [h for h, _, _ in parsed]
    if len({(h.n_q, h.bits, h.n_frames) for h in headers}) != 1:
        raise ValueError("decompress_long takes the blobs of one recording batch: equal n_frames, quantizer counts and bits "
                         f"(got {sorted({(h.n_q, h.bits, h.n_frames) for h in headers})}); decompress handles mixed lists")
    dev = timbre.device if isinstance(timbre, torch.Tensor) else _blob_device(model)
    timbres = _timbres_for(model, parsed, timbre, dev)
    codes = _codes_from_payloads(headers, [p for _, _, p in parsed], dev, False)
    wave = decode_long(model, codes, timbres, chunk_seconds=chunk_seconds)
    return _restore_loudness(wave, headers) if restore_loudness else wave


def load_checkpoint(model, optimizer, path, load_only_params=True, ignore_modules=(), is_distributed=False):
    """modules/commons.py:446-471: {'net': {key: state_dict}, ...}; strips DDP's 'module.' prefix."""
    state = torch.load(path, map_location="cpu")
    params = state["net"]
    for key in model:
        if key in params and key not in ignore_modules:
            sd = params[key]
            if not is_distributed:
                sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
            model[key].load_state_dict(sd, strict=True)
    for key in model:
        model[key].eval()
    epoch, iters = state.get("epoch", 0) + 1, state.get("iters", 0)
    if not load_only_params and optimizer is not None:
        optimizer.load_state_dict(state["optimizer"])
        optimizer.load_scheduler_state_dict(state["scheduler"])
    return model, optimizer, epoch, iters


def load_F0_models(path):
    """modules/commons.py:183-191: JDCNet(num_class=1, seq_len=192) with the checkpoint's ['net'] loaded (strict).  The reference
    then leaves the model in .train(); ours computes eval arithmetic in either mode (see jdc.py).  Returned on the CPU like the
    reference's: move it with .to(device)."""
    from .jdc import JDCNet
    model = JDCNet(num_class=1, seq_len=192)
    params = torch.load(path, map_location="cpu")["net"]
    model.load_state_dict(params)
    return model


def extract_f0(pitch_extractor, waves):
    """Equal-length clips (B, T) at 24 kHz on the GPU -> the extractor's F0 track (B, 1 + T // 300), one value per 12.5 ms frame:
    meldataset.preprocess (the features the extractor was trained on) then JDCNet.  The value is whatever the checkpoint was trained
    to emit (Hz for the reference's bst.t7; train.py:226 calls a frame voiced where it exceeds 5)."""
    from . import meldataset
    waves = torch.as_tensor(waves)
    if waves.dim() != 2:
        raise ValueError(f"extract_f0 takes equal-length clips (B, T), got {tuple(waves.shape)}")
    return pitch_extractor(meldataset.preprocess(waves).unsqueeze(1))[0]
