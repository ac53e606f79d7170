"""Streaming causal inference (BASELINE.json configs[4]): encode -> FA-quantize -> decode in
480-sample hops with carried state, matching the OFFLINE causal model on the same signal.

The reference has no streaming code (its README only says the causal model "supports" it,
/root/reference README.md:105-107); the contract here is therefore: for every frame / sample the session
emits, codes equal and waveform within fp32 noise of `model.encoder -> model.quantizer -> model.decoder` run
on the whole signal (tests/test_gpu_parity.py::test_streaming_matches_offline).

How the offline arithmetic is reproduced incrementally
  * every causal conv (dac/model/encodec.py:212-228) owns a left-context buffer `[ (k-1)*d history | new ]`
    (`_Tap`): a hop appends its new input columns (fac_stream_push) and the SAME conv kernel runs over the
    window that the new outputs need -- no padding, so per-output arithmetic (accumulation order included) is
    the offline kernel's.  Strided convs keep their unconsumed remainder inside the same history.
  * the FIRST chunk ("prime") is run with the offline reflect padding on the left: the reference's causal convs
    reflect-pad the start of the signal, so sample 0 of the output depends on up to 2 750 later samples
    (k7, dilation 9 at 1/50 rate).  Priming therefore takes >= 4 800 samples (a multiple of 2 400 so that the
    8-frames-per-5-hops pattern starts aligned).
  * LSTMs carry (h, c) (fac_lstm_layer_fwd_from).
  * prosody branch: the centred 2 048-point STFT of frame f needs samples up to 300 f + 1 023, so the quantizer
    and decoder run 1 024 samples (2.1 hops) behind the encoder; latents wait in a small FIFO.  The timbre vector
    is fixed for the session (enrolment clip), as in any streaming use of the model.
  * a period of 5 hops (2 400 samples = 8 frames) repeats every launch geometry exactly, so hops 5..9 are
    captured into five HIP graphs and replayed from then on (launch-bound: ~450 small launches per hop).
  * `finish()` flushes the frames that were waiting for look-ahead, with the reflect padding of the END of the
    signal the offline front-end applies.
"""
import torch

from . import ops
from .commons import MODEL_RATE
from .dac_model import FUSED_RU_CHANNELS, DecoderBlock, EncoderBlock
from .layers import ConvWeights
from .quantize import check_codes

HOP = 480            # samples per streaming hop (20 ms @ 24 kHz)
FRAME = 300          # encoder hop (prod of strides 2*5*5*6)
PERIOD = 2400        # lcm(HOP, FRAME): 5 hops = 8 frames
LOOKAHEAD = 1024     # n_fft / 2 of the prosody log-mel front-end


class _Edge:
    """(B, C, hist + max_new) buffer: [history | columns of the last push]; counts are host-side ints."""

    def __init__(self, sess, B, C, hist, max_new):
        self.hist = hist
        self.buf = torch.zeros(B, C, hist + max_new, device=sess.device, dtype=torch.float32)
        self.c = [0, 0]          # [columns pushed so far, columns of the last push]
        sess._counters.append(self)

    def push(self, x):
        n = x.shape[-1]
        ops.stream_push(self.buf, x, self.hist, self.c[1])
        self.c[0] += n
        self.c[1] = n

    def window(self, g0, length):
        col = self.hist + g0 - (self.c[0] - self.c[1])
        if col < 0 or col + length > self.hist + self.c[1]:
            raise RuntimeError(f"stream window [{g0}, {g0 + length}) outside the retained context")
        return self.buf[:, :, col:col + length]


class _Tap(_Edge):
    """Input side of one causal conv: history (k-1)*d, consumer cursor = outputs produced so far."""

    def __init__(self, sess, B, C, k, stride, dilation, max_new):
        super().__init__(sess, B, C, (k - 1) * dilation, max_new)
        self.k, self.s, self.d = k, stride, dilation
        self.pad = (k - 1) * dilation + 1 - stride
        self.c.append(0)         # c[2] = outputs so far

    def feed(self, x):
        """-> (x view, pad_left, pad_mode, t_out) for ops.conv1d."""
        first = self.c[0] == 0
        n = x.shape[-1]
        self.push(x)
        t_out = self.c[0] // self.s - self.c[2]
        if t_out <= 0:
            raise RuntimeError("streaming chunk too short to produce an output column")
        if first:
            if n % self.s or n <= self.pad:
                raise RuntimeError("first chunk must be a stride multiple longer than the reflect padding")
            view, pad_left, mode = self.window(0, n), self.pad, ops.PAD_REFLECT
        else:
            g0 = self.c[2] * self.s - self.pad
            view = self.window(g0, (t_out - 1) * self.s + (self.k - 1) * self.d + 1)
            pad_left, mode = 0, ops.PAD_ZERO
        self.c[2] += t_out
        return view, pad_left, mode, t_out


class _LSTMState:
    def __init__(self, sess, slstm, B):
        H, L = slstm.dimension, slstm.num_layers
        self.m, self.H = slstm, H
        self.state = [torch.zeros(3, H, ops.pad32(B), device=sess.device) for _ in range(L)]
        p = slstm.lstm
        self.w_ih = [ops.pack_conv_weight(getattr(p, f"weight_ih_l{l}").detach()) for l in range(L)]
        self.bias = [ops.add(getattr(p, f"bias_ih_l{l}").detach(), getattr(p, f"bias_hh_l{l}").detach()) for l in range(L)]
        self.whh = [ops.pack_lstm_whh(getattr(p, f"weight_hh_l{l}").detach()) for l in range(L)]
        self.c = [0]             # steps taken
        self._pre = {}           # (layer, T) -> zero-initialised (4H, T, BP) pre-activation buffer, real batch columns rewritten per hop
        sess._counters.append(self)

    def run(self, x, alpha_out):
        """SLSTM.forward (dac/model/encodec.py:282-288) continued from the carried state."""
        B, H, T = x.shape
        inp = ops.lstm_to_time_major(x)
        BP = inp.shape[2]
        few = T * B <= 4 and B < BP
        for l in range(len(self.state)):
            if few:
                # The recurrence kernel wants the batch padded to 32 columns; the input projection does not: as T "clips" of B
                # columns (views of the time-major buffers) it is a 1 - 4 column conv on the single-launch kernel instead of a
                # 32 T column one whose other columns are padding (33 -> 10 us per layer of the decoder's LSTM, tools/tune/hop_layers.py)
                pre = self._pre.get((l, T))
                if pre is None:
                    pre = self._pre[(l, T)] = torch.zeros(4 * H, T, BP, device=x.device)
                ops.conv1d(inp.view(H, T, BP).permute(1, 0, 2)[:, :, :B], self.w_ih[l], 4 * H, 1, bias=self.bias[l], pad_left=0,
                           t_out=B, pad_mode=ops.PAD_ZERO, out=pre.permute(1, 0, 2)[:, :, :B])
            else:
                pre = ops.conv1d(inp.view(1, H, T * BP), self.w_ih[l], 4 * H, 1, bias=self.bias[l], pad_left=0,
                                 t_out=T * BP, pad_mode=ops.PAD_ZERO).view(4 * H, T, BP)
            inp = ops.lstm_layer(pre.view(4 * H, T, BP), self.whh[l], H, state=self.state[l], step0=self.c[0])
        self.c[0] += T
        return ops.lstm_from_time_major(inp, x if self.m.skip else None, B, alpha_out)


def _conv(m, tap, x, **kw):
    view, pad_left, mode, t_out = tap.feed(x)
    w = m.w
    return ops.conv1d(view, w.packed(), w.c_out, m.kernel_size, bias=w.bias, stride=m.stride, dilation=m.dilation,
                      pad_left=pad_left, pad_mode=mode, t_out=t_out, **kw)


class _RUStream:
    """ResidualUnit (dac/model/dac.py:25-42) with a left-context buffer in front of its k7 conv."""

    def __init__(self, sess, ru, B, C, max_new):
        self.ru = ru
        self.tap = _Tap(sess, B, C, 7, 1, ru.block[1].dilation, max_new)

    def run(self, x, x_act, alpha_next, want_raw):
        b = self.ru.block
        k7, k1 = b[1], b[3]
        # small chunks: two split-reduction launches beat the fused single-tile kernel (latency, not throughput)
        if k7.w.c_out in FUSED_RU_CHANNELS and x.shape[0] * x.shape[-1] > 640:
            pair = _conv(k7, self.tap, x_act, alpha_out=b[2].flat(), res=x, w_k1=k1.w.packed(), bias_k1=k1.w.bias,
                         alpha_y2=alpha_next, want_y=want_raw or alpha_next is None)
            return pair if alpha_next is not None else (pair, None)
        h = _conv(k7, self.tap, x_act, alpha_out=b[2].flat())
        if alpha_next is None:
            return k1.run(h, res=x), None
        return k1.run(h, res=x, alpha_y2=alpha_next, want_y=want_raw)


def _run_units(units, x, x_act, alpha_after):
    for j, u in enumerate(units):
        last = j == len(units) - 1
        nxt = alpha_after if last else units[j + 1].ru.alpha_in
        x, x_act = u.run(x, x_act, alpha_next=nxt, want_raw=not last)
    return x_act


class _EncoderStream:
    """Encoder.forward (dac/model/dac.py:103-104) one chunk at a time; same fused plan as dac_model.Encoder."""

    def __init__(self, sess, enc, B, max_new):
        mods = list(enc.block)
        self.enc, self.mods = enc, mods
        self.blocks = [m for m in mods if isinstance(m, EncoderBlock)]
        self.tap0 = _Tap(sess, B, 1, 7, 1, 1, max_new)
        self.units, self.down = [], []
        rate = 1
        for blk in self.blocks:
            b = blk.block
            C = b[0].block[1].w.c_out
            self.units.append([_RUStream(sess, b[i], B, C, max_new // rate) for i in range(3)])
            self.down.append(_Tap(sess, B, C, b[4].kernel_size, b[4].stride, 1, max_new // rate))
            rate *= b[4].stride
        self.rate = rate
        self.lstm = _LSTMState(sess, mods[-3], B) if enc.use_lstm else None
        self.tap_out = _Tap(sess, B, enc.enc_dim, mods[-1].kernel_size, 1, 1, max_new // rate)

    def run(self, wave):
        mods, blocks = self.mods, self.blocks
        final_alpha = mods[-2].flat()
        x, x_act = _conv(mods[0], self.tap0, wave, alpha_y2=blocks[0].alpha_in)
        for i, blk in enumerate(blocks):
            b = blk.block
            if i + 1 < len(blocks):
                nxt = blocks[i + 1].alpha_in
            else:
                nxt = None if self.lstm is not None else final_alpha
            z_act = _run_units(self.units[i], x, x_act, b[3].flat())
            if nxt is not None:
                x, x_act = _conv(b[4], self.down[i], z_act, alpha_y2=nxt)
            else:
                x, x_act = _conv(b[4], self.down[i], z_act), None
        if self.lstm is not None:
            x_act = self.lstm.run(x, final_alpha)
        return _conv(mods[-1], self.tap_out, x_act)


class _DecoderStream:
    """Decoder.forward (dac/model/dac.py:164-165) one chunk of frames at a time."""

    def __init__(self, sess, dec, B, max_frames):
        mods = list(dec.model)
        self.dec, self.mods = dec, mods
        self.blocks = [m for m in mods if isinstance(m, DecoderBlock)]
        self.tap0 = _Tap(sess, B, mods[0].w.c_in, 7, 1, 1, max_frames)
        self.lstm = _LSTMState(sess, mods[1], B) if dec.use_lstm else None
        self.up, self.units = [], []
        n = max_frames
        for blk in self.blocks:
            b = blk.block
            self.up.append(_Tap(sess, B, b[1].w.c_in, 2, 1, 1, n))     # x[t-1] of the 2-tap polyphase form
            n *= b[1].stride
            C = b[1].w.c_out
            self.units.append([_RUStream(sess, b[i], B, C, n) for i in (2, 3, 4)])
        self.tap_out = _Tap(sess, B, mods[-2].w.c_in, 7, 1, 1, n)

    def _convtr(self, m, tap, x_act, alpha_y2):
        first = tap.c[0] == 0
        n = x_act.shape[-1]
        tap.push(x_act)
        tap.c[2] += n
        w = m.w
        if first:
            return ops.conv_transpose1d(tap.window(0, n), w.packed(), w.c_out, m.stride, bias=w.bias, alpha_y2=alpha_y2)
        return ops.conv_transpose1d(tap.window(tap.c[0] - n - 1, n + 1), w.packed(), w.c_out, m.stride, bias=w.bias,
                                    alpha_y2=alpha_y2, has_history=True)

    def run(self, z):
        mods, blocks = self.mods, self.blocks
        final_alpha = mods[-3].flat()
        if self.lstm is not None:
            x = _conv(mods[0], self.tap0, z)
            x_act = self.lstm.run(x, blocks[0].alpha_in)
        else:
            _, x_act = _conv(mods[0], self.tap0, z, alpha_y2=blocks[0].alpha_in, want_y=False)
        for i, blk in enumerate(blocks):
            b = blk.block
            nxt = blocks[i + 1].alpha_in if i + 1 < len(blocks) else final_alpha
            y, y_act = self._convtr(b[1], self.up[i], x_act, b[2].alpha_in)
            x_act = _run_units(self.units[i], y, y_act, nxt)
        return _conv(mods[-2], self.tap_out, x_act, act=ops.ACT_TANH)


def _wn_layers(wn, taps, h, n, cond=None):
    """WN.forward (modules/wavenet.py:138-166) over one chunk of n frames: a left-context tap in front of every in_layer;
    h (B, H, n) is consumed (the residual sums are written into it) -> the skip sum (B, H, n).  cond: the (B, 2 H L) output of
    cond_layer, constant over time; layer i adds its column slice to the gate's pre-activations."""
    out = torch.zeros_like(h)
    H2 = 2 * wn.hidden_channels
    fold = ops.STREAM_FOLD and h.shape[0] * n <= ops.SKINNY_MAX_COLS
    for i in range(wn.n_layers):                       # WN.forward, modules/wavenet.py:138-166
        last = i == wn.n_layers - 1
        g = None if cond is None else cond[:, i * H2:(i + 1) * H2]
        if not fold:
            a = _conv(wn.in_layers[i], taps[i], h)
            rs = wn.res_skip_layers[i].run(ops.gate_tanh_sigmoid(a, g))
            ops.wn_res_skip_(rs, h, out, last=last)
            continue
        # the same arithmetic with the gate and the residual / skip adds as epilogues of the two convs' reduction kernels
        acts = _conv(wn.in_layers[i], taps[i], h, act=ops.ACT_GATE, gate_cond=g)
        rsl = wn.res_skip_layers[i]
        w = rsl.w
        if last:
            ops.conv1d(acts, w.packed(), w.c_out, 1, bias=w.bias, pad_left=0, pad_mode=ops.PAD_ZERO, t_out=n, res=out, out=out)
        else:
            ops.conv1d(acts, w.packed(), w.c_out, 1, bias=w.bias, pad_left=0, pad_mode=ops.PAD_ZERO, t_out=n, res=h, out=h,
                       skip_acc=out, act=ops.ACT_WN_RES_SKIP)
    return out


class _QuantizerStream:
    """FAquantizer.forward_v2 (modules/quantize.py:375-454), eval, per chunk of frames, with a fixed timbre."""

    def __init__(self, sess, q, B, timbre, max_frames, wave_cap):
        self.q = q
        self.wave = _Edge(sess, B, 1, 2 * LOOKAHEAD, wave_cap)              # sample history for the STFT frames
        self.z_fifo = _Edge(sess, B, q.in_dim, 4, max_frames)               # latents waiting for look-ahead
        wn = q.melspec_encoder
        self.wn_taps = [_Tap(sess, B, wn.hidden_channels, 5, 1, 1, max_frames) for _ in range(wn.n_layers)]
        self.style = q.timbre_linear(timbre).contiguous()                   # (B, 2D) = [gamma | beta], fixed
        self.c = [0]                                                        # frames quantized so far
        sess._counters.append(self)
        self._rvq_w = {}

    def frames_ready(self, n_samples, final):
        return n_samples // FRAME if final else max(0, (n_samples - LOOKAHEAD) // FRAME + 1)

    def _mel(self, f0, n, final):
        fe = self.q.to_mel
        basis, fbp, off = fe._consts(self.wave.buf.device)
        total = self.wave.c[0]
        if f0 == 0:            # start of the signal: offline reflect padding on the left
            view, pad = self.wave.window(0, total), fe.n_fft // 2
        else:                  # interior (or, at finish(), reflect padding of the END of the signal)
            s0 = FRAME * f0 - fe.n_fft // 2
            length = total - s0 if final else FRAME * (n - 1) + fe.n_fft
            view, pad = self.wave.window(s0, length), 0
        w = view.reshape(view.shape[0], view.shape[-1])
        if not w.is_contiguous():
            w = w.contiguous()
        F_ = fe.n_fft // 2 + 1
        frames = ops.stft_frames(w, fe.win, n, fe.hop, pad, off)
        spec = ops.conv1d(frames, basis, 2 * F_, 1, pad_left=0, pad_mode=ops.PAD_ZERO, t_out=n)
        power = ops.spec_power(spec, 2)
        return ops.conv1d(power, fbp, fe.n_mels, 1, pad_left=0, pad_mode=ops.PAD_ZERO, t_out=n, act=ops.ACT_LOG_MEL)

    def _rvq(self, rvq, z, n_q):
        """ResidualVectorQuantize.forward (dac/nn/quantize.py:127-198), eval, codes + z_q only."""
        B, D, T = z.shape
        z_q = torch.zeros_like(z)
        codes = torch.empty(B, n_q, T, device=z.device, dtype=torch.int64)
        residual = torch.empty_like(z) if n_q > 1 else None
        src = z
        for i in range(n_q):
            vq = rvq.quantizers[i]
            if vq not in self._rvq_w:
                self._rvq_w[vq] = vq._weights()
            w_in, w_out, w_out_scale = self._rvq_w[vq]
            ops.vq_step(src, w_in, vq.in_proj.bias.detach(), vq.codebook.weight.detach(), w_out, w_out_scale,
                        vq.out_proj.bias.detach(), codes[:, i], residual=residual if i < n_q - 1 else None, zq_acc=z_q)
            src = residual
        return z_q, codes

    def push(self, wave_new, z_new):
        if wave_new is not None:
            self.wave.push(wave_new)
        if z_new is not None:
            self.z_fifo.push(z_new)

    def take_latents(self, final=False):
        """The latents of the frames whose look-ahead is complete, copied out of the FIFO -- or None when some of them are
        still to be produced by the encoder call of this very step (prime(), finish()).  In a steady-state hop they all come
        from earlier hops (the prosody front-end lags 1 024 samples, a hop brings 480), so the quantizer + decoder half of
        the hop does not depend on the encoder half and the two can run on two streams."""
        f0 = self.c[0]
        n = self.frames_ready(self.wave.c[0], final) - f0
        if n <= 0 or f0 + n > self.z_fifo.c[0]:
            return None
        return self.z_fifo.window(f0, n).contiguous()

    def prosody(self, final=False):
        """The branch of the frames whose look-ahead is complete that depends on the WAVEFORM only (log-mel -> 1x1 -> WaveNet -> 1x1 ->
        prosody RVQ, modules/quantize.py:398-413) -> (n, z_p, codes_p) or None."""
        q = self.q
        f0 = self.c[0]
        n = self.frames_ready(self.wave.c[0], final) - f0
        if n <= 0:
            return None
        mel = self._mel(f0, n, final)
        h = ops.conv1d(mel[:, :20], q.melspec_linear.w.packed(), 256, 1, bias=q.melspec_linear.w.bias, pad_left=0,
                       pad_mode=ops.PAD_ZERO, t_out=n)
        out = _wn_layers(q.melspec_encoder, self.wn_taps, h, n)
        f0_feat = q.melspec_linear2.run(out)
        z_p, codes_p = self._rvq(q.prosody_quantizer, f0_feat, 1)
        return n, z_p, codes_p

    def content(self, n_c, x):
        """Content RVQ of the due latents (modules/quantize.py:415-420): depends on the latents only."""
        return self._rvq(self.q.content_quantizer, x, n_c)

    def rest(self, x, pros, cont):
        """Residual RVQ of what the first two leave, sum, timbre-conditioned LayerNorm (modules/quantize.py:422-453)."""
        q = self.q
        n, z_p, codes_p = pros
        z_c, codes_c = cont
        z_r, codes_r = self._rvq(q.residual_quantizer, ops.sub2(x, z_p, z_c), 3)
        outs = ops.layernorm_c_affine(ops.add(ops.add(z_p, z_c), z_r), self.style)
        self.c[0] += n
        return outs, [codes_p, codes_c, codes_r]

    def run(self, n_c, final=False, x=None):
        """Quantizes the frames whose look-ahead is complete -> (outs, [codes_p, codes_c, codes_r]) or None.
        x: their latents if `take_latents` already copied them out."""
        f0 = self.c[0]
        pros = self.prosody(final)
        if pros is None:
            return None
        if x is None:
            x = self.z_fifo.window(f0, pros[0]).contiguous()
        return self.rest(x, pros, self.content(n_c, x))


class _HopSession:
    """What the sessions that take 480-sample hops share: prime / push / finish, the two-stream split of a steady-state hop
    and the five-phase graph capture.  A subclass builds its chains in __init__ (after _init_hops, before which no stream object
    may register its counters) and supplies `_back_half`."""

    def _init_hops(self, device, B, prime_samples, use_graphs):
        if prime_samples % PERIOD or prime_samples < 2 * PERIOD:
            raise ValueError(f"prime_samples must be a multiple of {PERIOD} and at least {2 * PERIOD}")
        self.device = device
        self.B, self.prime_samples = B, prime_samples
        self._counters = []
        self.n_samples = 0
        self.hops = 0
        self.use_graphs = use_graphs
        self._side = torch.cuda.Stream(device=self.device) if self.device.type == "cuda" else None
        if self._side is not None:
            ops.register_stream_slot(self._side)            # its own split-reduction scratch
        self._graphs = {}
        self._snap = {}
        self._hop_in = torch.zeros(B, 1, HOP, device=self.device)

    def _back_half(self, final, x=None):
        """Everything behind the latent FIFO for the frames whose look-ahead is complete -> (codes, wave) or None when no frame
        is due.  x: their latents if `take_latents` already copied them out."""
        raise NotImplementedError

    # ------------------------------------------------------------------------------------------ steps
    def _step(self, wave_new, final=False):
        first = self.qs.c[0]
        if wave_new is not None and self._side is not None:
            # steady-state hop: [encoder -> latent FIFO] and [quantizer -> decoder] touch disjoint state once the samples are in
            # the STFT history and the due latents are copied out -- two chains of ~100 latency-bound launches side by side
            self.qs.push(wave_new, None)
            x = self.qs.take_latents(final)
            if x is not None:
                main = torch.cuda.current_stream(self.device)
                self._side.wait_stream(main)
                with torch.cuda.stream(self._side):
                    codes, wave = self._back_half(final, x=x)
                self.qs.push(None, self.enc.run(wave_new))
                # join: everything later on the caller's stream (reading the outputs, the next hop's fork) is ordered behind both
                main.wait_stream(self._side)
                return dict(frame0=first, codes=codes, wave=wave)
            self.qs.push(None, self.enc.run(wave_new))
        elif wave_new is not None:
            z = self.enc.run(wave_new)
            self.qs.push(wave_new, z)
        r = self._back_half(final)
        if r is None:
            return dict(frame0=first, codes=None, wave=None)
        return dict(frame0=first, codes=r[0], wave=r[1])

    def prime(self, wave):
        if self.n_samples:
            raise RuntimeError("prime() must be the first call")
        if wave.shape[-1] != self.prime_samples:
            raise ValueError(f"prime() wants exactly {self.prime_samples} samples")
        self.n_samples = wave.shape[-1]
        return self._step(wave.contiguous())

    def _state(self):
        return [list(o.c) for o in self._counters]

    def _slot_state(self):
        """Every tensor that carries per-stream state from one hop to the next, as ("edge", (B, C, W)) / ("lstm", (3, H, BP)):
        the buffers the captured graphs read in place (StreamPool re-initialises a slot by overwriting its rows of them)."""
        for o in self._counters:
            if isinstance(o, _Edge):
                yield "edge", o.buf
            elif isinstance(o, _LSTMState):
                for s in o.state:
                    yield "lstm", s

    def _set_state(self, base, delta, k):
        for o, b, d in zip(self._counters, base, delta):
            o.c[:] = [bi + k * di for bi, di in zip(b, d)]

    def push(self, hop):
        if not self.n_samples:
            raise RuntimeError("call prime() first")
        if hop.shape[-1] != HOP:
            raise ValueError(f"push() wants exactly {HOP} samples")
        h, phase = self.hops, self.hops % 5
        self.hops += 1
        self.n_samples += HOP
        if not self.use_graphs:
            return self._step(hop.contiguous())
        self._hop_in.copy_(hop)
        if h < 5:                                         # first period: eager (also warms every kernel up)
            out = self._step(self._hop_in)
            self._snap[h] = self._state()
            return out
        if h < 10:                                        # second period: capture one graph per phase
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = self._step(self._hop_in)
            g.replay()                                    # capture does not execute
            after = self._state()
            delta = [[a - b for a, b in zip(sa, sb)] for sa, sb in zip(after, self._snap[h - 5])]
            self._graphs[phase] = (g, out, after, delta, h)
            return out
        g, out, base, delta, h0 = self._graphs[phase]
        g.replay()
        k = (h - h0) // 5
        self._set_state(base, delta, k)
        return dict(out, frame0=out["frame0"] + 8 * k)

    def finish(self):
        """End of the signal (length must be a multiple of 300): emits the remaining frames."""
        if self.n_samples % FRAME:
            raise ValueError("finish(): stream length must be a multiple of 300 samples")
        return self._step(None, final=True)


class StreamingCodec(_HopSession):
    """One streaming session over B parallel streams.

        sess = StreamingCodec(model, timbre)            # model = build_model(...) (causal), timbre (B, 1024)
        out = sess.prime(wave[:, :, :4800])             # first chunk, >= 4 800 samples, multiple of 2 400
        out = sess.push(wave[:, :, t:t + 480])          # every hop: dict(codes=[p, c, r], wave=(B, 1, 300 n))
        out = sess.finish()                             # frames that were waiting for look-ahead

    Each call returns the frames completed by it (`frames` = index of the first one).  With graphs enabled the
    returned tensors are static buffers, valid until the next call.
    """

    def __init__(self, model, timbre, n_c=2, prime_samples=4800, use_graphs=True):
        enc, q, dec = model.encoder, model.quantizer, model.decoder
        self._init_hops(timbre.device, timbre.shape[0], prime_samples, use_graphs)
        self.n_c = n_c
        for m in list(enc.modules()) + list(q.modules()) + list(dec.modules()):
            if isinstance(m, ConvWeights):
                m.freeze_packed = True               # inference: materialise w = g v/||v|| once
        B = self.B
        max_frames = prime_samples // FRAME
        self.enc = _EncoderStream(self, enc, B, prime_samples)
        self.qs = _QuantizerStream(self, q, B, timbre, max_frames, prime_samples)
        self.dec = _DecoderStream(self, dec, B, max_frames)

    def _back_half(self, final, x=None):
        r = self.qs.run(self.n_c, final, x=x)
        if r is None:
            return None
        outs, codes = r
        return codes, self.dec.run(outs)


class ChunkedCodec:
    """Offline counterpart of StreamingCodec for recordings of any length: the same encoder / quantizer / decoder streams
    (left-context taps, carried LSTM state, the prosody front-end's 1 024 samples of look-ahead), fed chunks of seconds instead
    of 480-sample hops.  Memory is that of one chunk, whatever the recording's length; throughput is the offline kernels'.

        sess = ChunkedCodec(model, timbre, chunk_samples=240000)       # model = build_model(...) (causal), timbre (B, 1024)
        out = sess.prime(wave[:, :, :240000])           # exactly chunk_samples (a multiple of 2 400, at least 4 800)
        out = sess.push(wave[:, :, t:t + n])            # any multiple of 300 up to chunk_samples
        out = sess.finish()                             # the frames that were waiting for look-ahead

    Each call returns dict(frame0, codes=[p, c, r] | None, wave=(B, 1, 300 n) | None) for the frames it completed, as
    StreamingCodec does, and they concatenate to the offline model's output on the whole signal (codes equal, waveform within fp32
    noise).  No phase graphs and no side stream: every call runs eagerly on the caller's stream, and the returned tensors are
    the caller's.  encode_only=True builds no decoder and returns wave=None."""

    def __init__(self, model, timbre, n_c=2, chunk_samples=240000, encode_only=False):
        chunk_samples = int(chunk_samples)
        if chunk_samples % PERIOD or chunk_samples < 2 * PERIOD:
            raise ValueError(f"chunk_samples must be a multiple of {PERIOD} and at least {2 * PERIOD}, got {chunk_samples}")
        bad = _first_non_causal(model, ("encoder",) if encode_only else ("encoder", "decoder"), "model")
        if bad is None and not model.quantizer.melspec_encoder.in_layers[0].causal:
            bad = "model.quantizer.melspec_encoder"
        if bad is not None:
            raise NotImplementedError(f"{bad} is not causal: a chunk cannot wait for the samples to the right of it")
        enc, q = model.encoder, model.quantizer
        _check_timbre(timbre, None, q.in_dim, "timbre")
        self.device, self.B = timbre.device, timbre.shape[0]
        self.chunk_samples, self.n_c, self.encode_only = chunk_samples, int(n_c), bool(encode_only)
        self._counters = []
        self.n_samples = 0
        self._closed = False
        mods = list(enc.modules()) + list(q.modules()) + ([] if encode_only else list(model.decoder.modules()))
        for m in mods:
            if isinstance(m, ConvWeights):
                m.freeze_packed = True               # inference: materialise w = g v/||v|| once
        max_frames = chunk_samples // FRAME
        with torch.no_grad():
            self.enc = _EncoderStream(self, enc, self.B, chunk_samples)
            self.qs = _QuantizerStream(self, q, self.B, timbre, max_frames, chunk_samples)
            self.dec = None if encode_only else _DecoderStream(self, model.decoder, self.B, max_frames)

    def _check_wave(self, wave):
        if not isinstance(wave, torch.Tensor) or wave.dim() != 3 or wave.shape[0] != self.B or wave.shape[1] != 1:
            got = tuple(wave.shape) if isinstance(wave, torch.Tensor) else type(wave).__name__
            raise ValueError(f"a chunk is (B = {self.B}, 1, n) float32, got {got}")
        if not wave.is_cuda or wave.dtype != torch.float32:
            raise ops._lib.FacodecHipError(f"a chunk must be float32 on the GPU (got {wave.dtype} on {wave.device}); there is no CPU path")

    @torch.no_grad()
    def _step(self, wave_new, final=False):
        first = self.qs.c[0]
        if wave_new is not None:
            self.qs.push(wave_new, self.enc.run(wave_new))
        r = self.qs.run(self.n_c, final)
        if r is None:
            return dict(frame0=first, codes=None, wave=None)
        outs, codes = r
        return dict(frame0=first, codes=codes, wave=None if self.dec is None else self.dec.run(outs))

    def prime(self, chunk):
        if self.n_samples:
            raise RuntimeError("prime() must be the first call")
        self._check_wave(chunk)
        if chunk.shape[-1] != self.chunk_samples:
            raise ValueError(f"prime() wants exactly {self.chunk_samples} samples, got {chunk.shape[-1]}")
        self.n_samples = chunk.shape[-1]
        return self._step(chunk.contiguous())

    def push(self, chunk):
        if not self.n_samples or self._closed:
            raise RuntimeError("call prime() first" if not self.n_samples else "the session is finished")
        self._check_wave(chunk)
        n = chunk.shape[-1]
        if n < FRAME or n % FRAME or n > self.chunk_samples:
            raise ValueError(f"push() wants a multiple of {FRAME} samples up to {self.chunk_samples}, got {n}")
        self.n_samples += n
        return self._step(chunk.contiguous())

    def finish(self):
        """End of the signal: emits the frames that were waiting for look-ahead, framed with the reflect padding of the signal's
        end, and closes the session."""
        if not self.n_samples or self._closed:
            raise RuntimeError("call prime() first" if not self.n_samples else "the session is finished")
        self._closed = True
        return self._step(None, final=True)


def _first_non_causal(model, keys, prefix):
    """Name of the first conv under model[key], in execution order, that looks to the right of its output column, or None.
    (A k = 1 conv pads nothing, whatever its `causal` flag says: the WaveNet's cond_layer.)"""
    from .layers import SConv1d, SConvTranspose1d
    for key in keys:
        for name, m in model[key].named_modules():
            if isinstance(m, SConvTranspose1d) and not m.causal:
                return f"{prefix}.{key}.{name}"
            if isinstance(m, SConv1d) and not m.causal and (m.kernel_size - 1) * m.dilation + 1 - m.stride > 0:
                return f"{prefix}.{key}.{name}"
    return None


def _check_timbre(timbre, B, dim, what):
    if not isinstance(timbre, torch.Tensor) or timbre.dim() != 2 or timbre.shape[1] != dim or (B is not None and timbre.shape[0] != B):
        got = tuple(timbre.shape) if isinstance(timbre, torch.Tensor) else type(timbre).__name__
        raise ValueError(f"{what} must be a float32 GPU tensor ({'B' if B is None else B}, {dim}), got {got}")
    if timbre.dtype != torch.float32:
        raise ValueError(f"{what} must be float32, got {timbre.dtype}")
    if not timbre.is_cuda:
        raise ValueError(f"{what} must live on the GPU, got {timbre.device}; there is no CPU path")


class _RedecoderStream:
    """Redecoder.forward (modules/redecoder.py:35-48), eval, per chunk of frames: code embeddings summed into a static buffer ->
    16-layer causal WaveNet with a left-context tap per layer, conditioned on a target timbre through `cond` -> 1x1 conv.
    cond = cond_layer(timbre) is constant over time: computed once per target (set_target) into a static (B, 2 H L) buffer whose
    column slices the gate epilogues read, so nothing is broadcast per hop and captured graphs survive a change of target."""

    def __init__(self, sess, r, B, timbre, use_p_code, n_c, max_frames):
        self.r = r
        wn = r.encoder
        E = r.embed_dim
        dev = sess.device
        # the tables in use, stacked once per session (Redecoder.forward stacks them on every call)
        self.p_tabs = torch.stack([e.weight.detach() for e in r.prosody_embed]) if use_p_code and r.n_p_codebooks else None
        self.c_tabs = torch.stack([e.weight.detach() for e in list(r.content_embed)[:n_c]])
        self.x = torch.zeros(B * E * max_frames, device=dev)                 # (B, E, n) of the chunk, n <= max_frames
        self.max_frames = max_frames
        self.taps = [_Tap(sess, B, E, m.kernel_size, 1, m.dilation, max_frames) for m in wn.in_layers]
        self.cond = torch.zeros(B, 2 * wn.hidden_channels * wn.n_layers, device=dev)
        self.w_out = ops.pack_conv_weight(r.conv_out.weight.detach())
        self.b_out = r.conv_out.bias.detach()
        self.set_target(timbre)

    def set_target(self, timbre):
        B = timbre.shape[0]
        self.cond.copy_(self.r.encoder.cond_layer.run(timbre.contiguous().reshape(B, -1, 1)).reshape(B, -1))

    def run(self, codes_p, codes_c, n):
        r = self.r
        B, E = codes_c.shape[0], r.embed_dim
        if n > self.max_frames:
            raise RuntimeError(f"a chunk of {n} frames exceeds the session's {self.max_frames}")
        x = self.x[:B * E * n].view(B, E, n)
        first = True
        for codes, tabs in ((codes_p, self.p_tabs), (codes_c, self.c_tabs)):
            if tabs is not None:
                ops.embed_sum(codes, tabs, 0, out=x, accumulate=not first)
                first = False
        out = _wn_layers(r.encoder, self.taps, x, n, cond=self.cond)
        return ops.conv1d(out, self.w_out, r.conv_out.c_out, 1, bias=self.b_out, pad_left=0, pad_mode=ops.PAD_ZERO, t_out=n)


class StreamingConverter(_HopSession):
    """Real-time voice conversion over B parallel streams: source audio in 480-sample hops in, the same speech in the target
    voice out (reconstruct_redecoder.py:95-122, one hop at a time).

        vc  = StreamingConverter(codec, redecoder, target_timbre)     # codec = build_model(...) (causal stage 'codec'),
                                                                      # redecoder = build_model(..., stage='redecoder') with
                                                                      # decoder_causal=True; target_timbre (B, 1024) fp32, GPU
        out = vc.prime(wave[:, :, :4800])              # dict(frame0, codes=[p, c], wave=(B, 1, 300 n) | None)
        out = vc.push(wave[:, :, t:t + 480])
        out = vc.finish()
        vc.set_target(timbre)                          # switch the target voice between hops

    A hop runs the codec's encoder, the prosody branch and the content RVQ with n_c quantizers on the source (no residual RVQ, no
    timbre LayerNorm, no codec decoder), then the redecoder -- code embeddings, the timbre-conditioned causal WaveNet, conv_out --
    and the redecoder's decoder.  The prosody branch runs even with use_p_code=False: codes[0] is emitted either way, as the
    reference derives the prosody codes from the waveform regardless of what the redecoder consumes.  Codes equal the offline
    quantizer's, the concatenated waveform equals `redecoder.encoder(codes ...) -> redecoder.decoder` on the whole signal within
    fp32 noise.  The defaults use_p_code=False, n_c=1 are the call of reconstruct_redecoder.py:121.

    target_timbre comes from the offline quantizer on an enrolment clip of the target speaker.  source_timbre is accepted for
    symmetry with StreamingCodec and checked, but no step of the conversion hop reads the source's timbre.

    prime / push / finish, the two-stream split and the graph capture are StreamingCodec's (_HopSession); with graphs enabled the
    returned tensors are static buffers, valid until the next call.
    """

    def __init__(self, codec, redecoder, target_timbre, source_timbre=None, use_p_code=False, n_c=1, prime_samples=4800,
                 use_graphs=True):
        enc, q = codec.encoder, codec.quantizer
        red, dec = redecoder.encoder, redecoder.decoder
        # ---- everything that can be refused is refused here, on the host, before any launch
        if getattr(red, "encoder_type", None) != "wavenet":
            raise NotImplementedError(f"redecoder encoder_type {getattr(red, 'encoder_type', None)!r}: only 'wavenet' streams")
        bad = _first_non_causal(redecoder, ("encoder", "decoder"), "redecoder")
        if bad is not None:
            raise NotImplementedError(f"{bad} is not causal: a streaming conversion needs the redecoder built with "
                                      "decoder_causal=True (a hop cannot wait for frames to the right of it)")
        n_c = int(n_c)
        if n_c < 1 or n_c > red.n_c_codebooks or n_c > q.content_quantizer.n_codebooks:
            raise ValueError(f"n_c = {n_c}: the redecoder has {red.n_c_codebooks} content tables, the codec's content RVQ "
                             f"{q.content_quantizer.n_codebooks} quantizers (1 .. the smaller of the two)")
        _check_timbre(target_timbre, None, q.in_dim, "target_timbre")
        B = target_timbre.shape[0]
        if source_timbre is not None:
            _check_timbre(source_timbre, B, q.in_dim, "source_timbre")
        self._init_hops(target_timbre.device, B, prime_samples, use_graphs)
        self.n_c, self.use_p_code = n_c, bool(use_p_code)
        self._dim = q.in_dim
        for m in list(enc.modules()) + list(q.modules()) + list(red.modules()) + list(dec.modules()):
            if isinstance(m, ConvWeights):
                m.freeze_packed = True               # inference: materialise w = g v/||v|| once
        max_frames = prime_samples // FRAME
        with torch.no_grad():
            self.enc = _EncoderStream(self, enc, B, prime_samples)
            style_src = source_timbre if source_timbre is not None else torch.zeros_like(target_timbre)
            self.qs = _QuantizerStream(self, q, B, style_src, max_frames, prime_samples)
            self.red = _RedecoderStream(self, red, B, target_timbre, self.use_p_code, n_c, max_frames)
            self.dec = _DecoderStream(self, dec, B, max_frames)

    def set_target(self, timbre):
        """Switches the target voice: recomputes cond = cond_layer(timbre) into the static buffer the gate epilogues read, so
        captured graphs stay valid and the next hop already speaks with the new voice.  Call it between hops, on the stream the
        hops are pushed on.  The left contexts (WaveNet taps, decoder taps, LSTM state) are not reset: they keep what the previous
        voice wrote, so the first frames after a switch see up to a receptive field of the old voice's activations."""
        _check_timbre(timbre, self.B, self._dim, "timbre")
        with torch.no_grad():
            self.red.set_target(timbre)

    def _back_half(self, final, x=None):
        qs = self.qs
        f0 = qs.c[0]
        pros = qs.prosody(final)
        if pros is None:
            return None
        n, _, codes_p = pros
        if x is None:
            x = qs.z_fifo.window(f0, n).contiguous()
        _, codes_c = qs.content(self.n_c, x)             # z_p is no input of the content RVQ (modules/quantize.py:415-420)
        qs.c[0] += n
        z = self.red.run(codes_p, codes_c, n)
        return [codes_p, codes_c], self.dec.run(z)

    def _step(self, wave_new, final=False):
        with torch.no_grad():
            return super()._step(wave_new, final)


class StreamingDecoder:
    """Receiver side of a streaming codec: codes in, audio out, over B parallel streams with a timbre fixed for the session.

        rx = StreamingDecoder(model, timbre)                 # model = build_model(...) (causal), timbre (B, 1024)
        wave = rx.prime(codes)                               # first chunk: >= rx.min_prime frames
        wave = rx.push(codes)                                # any chunk of k >= 1 frames -> (B, 1, 300 k)

    `codes` = [codes_p (B, n_p, k), codes_c (B, n_c, k), codes_r (B, n_r, k)] int64, the layout StreamingCodec emits
    (`out["codes"]`); the row counts are fixed by prime().  The concatenated output equals decode_codes() of all codes
    (commons.py) within fp32 noise: the codes-to-latent step is fac_vq_decode on a static code buffer, the decoder is the
    sender's _DecoderStream (causal convs with left-context buffers, carried LSTM state).

    Codes are NOT range checked per push (that would be one device-to-host read per hop and end the hop's independence from
    the host): an index outside [0, codebook_size) decodes as the clamped index, without reading outside the codebook.
    prime() does check its codes.

    With use_graphs the hop is captured into one HIP graph per (previous k, k, LSTM step parity) -- a push's launches depend on
    its own size, through the left-context shifts (fac_stream_push) on the previous push's, and through the LSTM's alternating
    hidden-state buffers (fac_lstm_layer_fwd: they swap on every step) on the parity of the frames decoded so far -- after one
    eager push with that key, and replayed from the third such push on, the host-side counters advanced by the delta the
    captured push made (as in StreamingCodec.push, whose 5-hop period is 8 frames: even).  The hop is one chain on the caller's stream (no side-stream fork inside the graph).  With graphs the
    returned wave is a static buffer, valid until the next call.
    """

    def __init__(self, model, timbre, use_graphs=True, max_frames=16):
        q, dec = model.quantizer, model.decoder
        self.device = timbre.device
        self.B = timbre.shape[0]
        self.max_frames = int(max_frames)
        self._counters = []
        for m in list(q.modules()) + list(dec.modules()):
            if isinstance(m, ConvWeights):
                m.freeze_packed = True               # inference: materialise w = g v/||v|| once
        self.q = q
        if tuple(timbre.shape) != (self.B, q.in_dim) or timbre.dtype != torch.float32:
            raise ValueError(f"timbre must be float32 (B, {q.in_dim}), got {tuple(timbre.shape)} {timbre.dtype}")
        with torch.no_grad():
            self.style = q.timbre_linear(timbre.contiguous()).contiguous()         # (B, 2D) = [gamma | beta], fixed
            self._weights = q.decode_weights()
        self.dec = _DecoderStream(self, dec, self.B, self.max_frames)
        self.min_prime = self._min_prime()
        self.use_graphs = use_graphs
        self.frames = 0
        self._n_q = None
        self._codes = None
        self._last_k = 0
        self._graphs = {}
        self._warm = set()

    def _min_prime(self):
        """Fewest frames the first chunk may have: every causal conv of the decoder reflect-pads the start of the signal by
        pad = (k - 1) d + 1 - s columns (_Tap), which needs more than `pad` input columns; a tap running at `rate` columns per
        frame therefore needs floor(pad / rate) + 1 frames (k7 with dilation 9 at 6 columns per frame: 10 frames)."""
        taps = [self.dec.tap0, self.dec.tap_out] + [u.tap for units in self.dec.units for u in units]
        need = 1
        for tap in taps:
            assert tap.s == 1                             # the decoder's causal convs are unstrided (upsampling: ConvTranspose)
            rate = (tap.buf.shape[-1] - tap.hist) // self.max_frames
            need = max(need, tap.pad // rate + 1)
        return need

    def _check(self, codes):
        if not isinstance(codes, (list, tuple)) or len(codes) != 3:
            raise ValueError("codes must be [codes_p, codes_c, codes_r], each (B, n, k) int64")
        k = codes[0].shape[-1]
        for c in codes:
            if not isinstance(c, torch.Tensor) or c.dtype != torch.int64 or c.dim() != 3 or c.shape[0] != self.B or c.shape[-1] != k:
                raise ValueError(f"codes must be three int64 (B={self.B}, n, k) tensors with the same k")
        if k < 1 or k > self.max_frames:
            raise ValueError(f"a chunk of {k} frames (1 .. max_frames = {self.max_frames})")
        if self._n_q is not None and [c.shape[1] for c in codes] != self._n_q:
            raise ValueError(f"code row counts {[c.shape[1] for c in codes]} differ from the session's {self._n_q}")
        return k

    def _step(self, k):
        codes = [self._codes[r][:, :, :k] if self._n_q[r] else None for r in range(3)]
        outs = ops.vq_decode(codes, self._wsel, self.style, self.q.prosody_quantizer.codebook_size)
        return self.dec.run(outs)

    def _load(self, codes, k):
        for r in range(3):
            if self._n_q[r]:
                self._codes[r][:, :, :k].copy_(codes[r])

    def prime(self, codes):
        if self._n_q is not None:
            raise RuntimeError("prime() must be the first call")
        k = self._check(codes)
        if k < self.min_prime:
            raise ValueError(f"prime() needs at least {self.min_prime} frames (the decoder's reflect-padded first taps), got {k}")
        rvqs = (self.q.prosody_quantizer, self.q.content_quantizer, self.q.residual_quantizer)
        for c, rvq in zip(codes, rvqs):
            if c.shape[1] > rvq.n_codebooks:
                raise ValueError(f"{c.shape[1]} code rows for an RVQ of {rvq.n_codebooks} quantizers")
        check_codes(codes, self.q.prosody_quantizer.codebook_size)
        self._n_q = [c.shape[1] for c in codes]
        self._wsel = [w[:n] for w, n in zip(self._weights, self._n_q)]
        self._codes = [torch.zeros(self.B, max(n, 1), self.max_frames, dtype=torch.int64, device=self.device) for n in self._n_q]
        self._load(codes, k)
        with torch.no_grad():
            wave = self._step(k)
        self.frames, self._last_k = k, k
        return wave

    def _state(self):
        return [list(o.c) for o in self._counters]

    def push(self, codes):
        if self._n_q is None:
            raise RuntimeError("call prime() first")
        k = self._check(codes)
        key = (self._last_k, k, self.dec.lstm.c[0] & 1 if self.dec.lstm is not None else 0)
        self._last_k = k
        self.frames += k
        self._load(codes, k)
        with torch.no_grad():
            if not self.use_graphs or key not in self._warm:
                self._warm.add(key)                       # first push with this key: eager (also warms every kernel up)
                return self._step(k)
            if key not in self._graphs:                   # second: capture (capture does not execute: replay once)
                before = self._state()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    wave = self._step(k)
                g.replay()
                delta = [[a - b for a, b in zip(sa, sb)] for sa, sb in zip(self._state(), before)]
                self._graphs[key] = (g, wave, delta)
                return wave
            g, wave, delta = self._graphs[key]
            g.replay()
            for o, d in zip(self._counters, delta):
                o.c[:] = [ci + di for ci, di in zip(o.c, d)]
            return wave


class LayeredDecoder(StreamingDecoder):
    """StreamingDecoder whose quantizer counts may differ per stream, per push and per frame:

        rx = LayeredDecoder(model, timbre)
        wave = rx.prime(codes)                               # as StreamingDecoder (n_use= as in push)
        wave = rx.push(codes, n_use)                         # n_use (B, k, 3) int32 on the device, or None: every quantizer

    n_use[b, t, r] is the number of leading quantizers of RVQ r that frame t of stream b is decoded from (clamped to the
    session's counts; the codes of the others are ignored).  The counts are copied into a static (B, max_frames, 3) buffer and
    the hop's codes-to-latent launch is fac_vq_decode_masked on that buffer, so it sits inside the captured graphs, whose
    keying is StreamingDecoder's.  With n_use=None, or full counts, the output is StreamingDecoder's bit for bit; a row decoded
    with (a, b, c) throughout is, bit for bit, its row in a StreamingDecoder session primed with the codes cut to (a, b, c)."""

    def __init__(self, model, timbre, use_graphs=True, max_frames=16):
        super().__init__(model, timbre, use_graphs=use_graphs, max_frames=max_frames)
        self._n_use = self._n_full = self._pending = None
        self._static = False

    def _step(self, k):
        codes = [self._codes[r][:, :, :k] if self._n_q[r] else None for r in range(3)]
        outs = ops.vq_decode(codes, self._wsel, self.style, self.q.prosody_quantizer.codebook_size, n_use=self._n_use[:, :k])
        return self.dec.run(outs)

    def _load(self, codes, k):
        if self._n_use is None:
            self._n_full = torch.tensor(self._n_q, dtype=torch.int32, device=self.device).expand(self.B, self.max_frames, 3).contiguous()
            self._n_use = self._n_full.clone()
        if self._static:
            return
        super()._load(codes, k)
        self._n_use[:, :k].copy_(self._n_full[:, :k] if self._pending is None else self._pending)

    def _check_n_use(self, codes, n_use):
        if n_use is None:
            return
        k = codes[0].shape[-1]
        if not isinstance(n_use, torch.Tensor) or n_use.dtype != torch.int32 or tuple(n_use.shape) != (self.B, k, 3) \
                or n_use.device != codes[0].device:
            raise ValueError(f"n_use must be an int32 (B={self.B}, k={k}, 3) tensor on the codes' device")

    def prime(self, codes, n_use=None):
        self._check(codes)
        self._check_n_use(codes, n_use)
        self._pending = n_use
        try:
            return super().prime(codes)
        finally:
            self._pending = None

    def push(self, codes, n_use=None):
        self._check(codes)
        self._check_n_use(codes, n_use)
        self._pending = n_use
        try:
            return super().push(codes)
        finally:
            self._pending = None

    def buffers(self, k):
        """The session's static buffers for a push of k frames: ([codes_p, codes_c, codes_r] views (B, n_q[r], k), n_use (B, k, 3)).
        A caller that fills them on the device (fac_plc_select) plays them with push_buffers(k), without a copy."""
        if self._n_q is None:
            raise RuntimeError("call prime() first")
        return [self._codes[r][:, :self._n_q[r], :k] for r in range(3)], self._n_use[:, :k]

    def push_buffers(self, k):
        """push() of what buffers(k) holds now."""
        codes, _ = self.buffers(k)
        self._static = True
        try:
            return super().push(codes)
        finally:
            self._static = False


class StreamingResampler:
    """ops.resample one block at a time, over B parallel streams:

        rs = StreamingResampler(B, 48000, 24000)             # quality "fast" (W = 16) unless asked otherwise
        y = rs.push(block)                                   # (B, 1, k) at rate_in, k n % o == 0  ->  (B, 1, k n / o) at rate_out
        tail = rs.finish()                                   # the last rs.delay samples

    An output needs the inputs up to ceil(W o / base) samples to its right, so the stream runs `delay` = ceil(ceil(W o / base) n / o)
    output samples (`latency` seconds) behind the offline call: the pushes and finish(), concatenated, are `delay` zeros followed
    by ops.resample of the whole signal -- bit for bit and for any split into admissible blocks, because the kernel's per-output
    arithmetic depends on the output's phase alone.  The state is the last `n_hist` input samples a later output can still reach,
    in two buffers that swap roles: the launch that resamples a block also writes the next block's history (fac_resample
    hist_out), so a push is ONE launch, reads nothing back to the host and allocates nothing but its output.  Equal rates pass
    the blocks through (delay 0)."""

    def __init__(self, B, rate_in, rate_out, quality="fast", device="cuda"):
        geo = ops.resample_table(rate_in, rate_out, quality)
        self.B, self.rate_in, self.rate_out, self.quality = int(B), int(rate_in), int(rate_out), quality
        self.o, self.n = geo["o"], geo["n"]
        self.device = torch.device(device)
        self.samples = 0                                      # input samples taken so far
        self.identity = self.rate_in == self.rate_out
        if self.identity:
            self.delay, self.latency, self.n_hist = 0, 0.0, 0
            return
        half = geo["half"]
        self.delay = -(-half * self.n // self.o)
        self.latency = self.delay / self.rate_out
        # the earliest output of a block lies `delay` outputs = up to ceil(delay o / n) inputs before it and reaches `half` further back
        self.n_hist = -(-self.delay * self.o // self.n) + half + 1
        self._geo, self._table, self._offs = ops._resample_device_table(rate_in, rate_out, quality, self.device)
        self._hist = [torch.zeros(self.B, self.n_hist, device=self.device) for _ in range(2)]
        self._cur = 0

    def _launch(self, x, n_out, carry, T=None):
        y = torch.empty(self.B, 1, n_out, device=self.device)
        hist = self._hist[self._cur]
        d = ops.resample_desc(self._geo, self._table, self._offs, x, y.view(self.B, n_out), n_out, hist=hist,
                              hist_out=self._hist[1 - self._cur] if carry else None, q0=self.samples,
                              m_lo=self.samples * self.n // self.o - self.delay, T=T)
        ops._lib.check(ops._lib.load().fac_resample(ops.C.byref(d), ops._stream()), "fac_resample")
        return y

    def push(self, block):
        if not isinstance(block, torch.Tensor) or block.dim() != 3 or block.shape[0] != self.B or block.shape[1] != 1:
            raise ValueError(f"push() takes (B = {self.B}, 1, k), got {tuple(block.shape) if isinstance(block, torch.Tensor) else type(block)}")
        k = block.shape[-1]
        if k < 1 or k * self.n % self.o:
            raise ValueError(f"a block of {k} samples at {self.rate_in} Hz is no whole number of samples at {self.rate_out} Hz "
                             f"(k must be a positive multiple of {self.o})")
        if not block.is_cuda or block.dtype != torch.float32:
            raise ops._lib.FacodecHipError(f"block must be float32 on the GPU (got {block.dtype} on {block.device}); there is no CPU path")
        if self.identity:
            self.samples += k
            return block
        # rows of any pitch are taken as they are (fac_resample_desc.x_bs): a slice wave[:, :, t:t + k] of a longer buffer is not copied
        x = block[:, 0, :]
        if k > 1 and x.stride(1) != 1:
            x = x.contiguous()
        y = self._launch(x, k * self.n // self.o, carry=True)
        self._cur ^= 1
        self.samples += k
        return y

    def finish(self):
        """The `delay` output samples the stream was still holding back (the signal ends where the last block ended)."""
        if self.identity:
            return torch.empty(self.B, 1, 0, device=self.device)
        # an empty block: x only has to be a valid pointer (an empty tensor has none), none of its columns is read
        return self._launch(self._hist[self._cur], self.delay, carry=False, T=0)


class LoudnessMeter:
    """The BS.1770-4 meter over B parallel streams, one block at a time:

        meter = LoudnessMeter(B)                             # rate 24000
        meter.push(block)                                    # (B, 1, k) or (B, k) float32 on the GPU, any k >= 1
        meter.momentary(), meter.short_term(), meter.integrated()      # (B,) float64 on the device, LUFS

    push is one fac_kweight_energy call that carries the filter state (fp64, updated in place) and the position inside the
    current 100 ms sub-block, so the sub-block grid and the energies are those of the offline call on the whole signal (up to
    fp64 rounding: chunk boundaries move with the blocks).  It reads nothing back to the host and, in the steady state,
    allocates nothing: the energy history is a preallocated device buffer (8 bytes per stream and 100 ms) that doubles when it
    is full, the scratch grows only with the largest block seen.  momentary() is the last 400 ms, short_term() the last 3 s,
    both ungated and counting what lies before the stream's start as silence; integrated() is the two-gate loudness of
    everything pushed so far.  `peak` holds max |x| so far.  A session's caller can level its input with it or watch its output;
    the sessions themselves do not use it (AutoGain / LevelledSession below level a session's input)."""

    def __init__(self, B, rate=MODEL_RATE, device="cuda", seconds=60):
        self.S = ops._kweight_tables(rate)[0]                 # ValueError: the rate
        self.B, self.rate, self.device = int(B), int(rate), torch.device(device)
        self.samples = 0
        self._e = torch.zeros(self.B, max(8, int(seconds) * 10), device=self.device, dtype=torch.float64)
        self._state = torch.zeros(self.B, 4, device=self.device, dtype=torch.float64)
        self.peak = torch.zeros(self.B, device=self.device, dtype=torch.float32)
        self._ws = None

    def push(self, block):
        if not isinstance(block, torch.Tensor) or block.dim() not in (2, 3) or block.shape[0] != self.B or (block.dim() == 3 and block.shape[1] != 1):
            raise ValueError(f"push() takes (B = {self.B}, 1, k) or (B, k), got {tuple(block.shape) if isinstance(block, torch.Tensor) else type(block)}")
        k = block.shape[-1]
        if k < 1:
            raise ValueError("push() takes at least one sample")
        j0, offset = divmod(self.samples, self.S)
        n_sub = -(-(offset + k) // self.S)
        if j0 + n_sub > self._e.shape[1]:
            grown = torch.zeros(self.B, max(2 * self._e.shape[1], j0 + n_sub), device=self.device, dtype=torch.float64)
            grown[:, :self._e.shape[1]] = self._e
            self._e = grown
        need = ops._lib.load().fac_kweight_ws_bytes(self.B, k)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 0), device=self.device, dtype=torch.uint8)
        ops.loudness_energies(block, self.rate, state=self._state, offset=offset, out=self._e[:, j0:], peak=self.peak,
                              state_out=self._state, ws=self._ws)
        self.samples += k

    @property
    def energies(self):
        """(B, ceil(samples / S)) float64: the sub-block energies so far (a view of the history buffer)."""
        return self._e[:, :-(-self.samples // self.S)]

    def _gate(self, last_n):
        return ops.loudness_gate(self._e, self.samples, self.rate, last_n=last_n)

    def momentary(self):
        return self._gate(4)

    def short_term(self):
        return self._gate(30)

    def integrated(self):
        return self._gate(0)


class _Stage:
    """What the streaming stages in front of a session share (VoiceActivity, AutoGain, NoiseSuppressor, EchoCanceller, each over
    B rows on one device, with rings of R entries where it has any): the guards of push and finish, the check of a pushed
    block, row indices on the device, the last entries of a ring, and a long push run as several."""
    _done = False

    def __init_subclass__(cls):
        cls._what = cls.__name__ + ".push"                  # how push's refusals name their caller

    def _close(self):
        if self._done:
            raise RuntimeError("finish() twice")
        self._done = True

    def _block(self, block):
        """push()'s argument, (B, 1, k) or (B, k) float32 on the GPU with k >= 1 -> its (B, k) view."""
        if self._done:
            raise RuntimeError("push() after finish()")
        x = ops._rows(block, self._what)
        if x.shape[0] != self.B or x.shape[1] < 1:
            raise ValueError(f"push() takes (B = {self.B}, 1, k) or (B, k) with k >= 1, got {tuple(block.shape)}")
        return x

    def _rows_idx(self, rows, what):
        """Row indices on the host -> an int64 tensor on the device, None for no rows."""
        rows = [int(r) for r in rows]
        if any(not 0 <= r < self.B for r in rows):
            raise ValueError(f"{what}({rows}): rows are 0 .. {self.B - 1}")
        return ops.h2d(torch.tensor(rows, dtype=torch.int64), self.device) if rows else None

    def _ring_tail(self, ring, have, n):
        """Entries have - n .. have - 1 of a ring (B, R, ...) that holds entry j at slot j % R: a copy."""
        return ring[:, torch.arange(have - n, have, device=self.device) % self.R]

    def _push_pieces(self, block):
        """push() of a stage whose rings bound what one run may take: self._run on consecutive pieces of the block, each of at
        most self._room() samples (asked again before every piece) -> the pieces' outputs, concatenated, in the block's shape."""
        x = self._block(block)
        parts, t, k = [], 0, x.shape[1]
        while t < k:
            n = min(k - t, self._room())
            parts.append(self._run(x[:, t:t + n]))
            t += n
        return (parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)).view(block.shape)


class VoiceActivity(_Stage):
    """Voice activity detection over B parallel streams, one block at a time:

        vad = VoiceActivity(B)                               # frames of 300 samples: the codec's frames
        vad.push(block)                                      # (B, 1, k) or (B, k) float32 on the GPU, any k >= 1
        flags = vad.take(n)                                  # (B, n) uint8: the next n frames not yet taken
        vad.finish()                                         # decides the partial last frame

    For any chunking of the signal, flags and energies are those of ops.vad on the whole signal, bit for bit.  push is two
    launches -- fac_vad_energy, which also moves the unprocessed tail (under one frame) from one carry buffer into the other,
    and fac_vad_decide -- or one when the block completes no frame; nothing is read back and, in the steady state, nothing is
    allocated.  `frames` counts the frames decided so far (on the host).  Energies and flags live in device rings of `ring`
    frames; a push may complete at most ring - window - hangover frames, and take() can only reach frames still in the ring.
    take(n, out=) gathers into the caller's (B, n) uint8 buffer of any row pitch, e.g. CodePacketizer.active_view().  The
    defaults (1.5 s of minimum statistics, 200 ms of hangover, 6 dB over the floor, -70 dBFS) were not tuned by listening."""

    def __init__(self, B, frame=300, window=120, hangover=16, margin_db=6.0, floor_db=-70.0, ring=256, device="cuda"):
        self.frame, self.window, self.hangover, self.margin, self.thr_abs = ops.vad_params(frame, window, hangover, margin_db, floor_db)
        self.B, self.R, self.device = int(B), int(ring), torch.device(device)
        if self.B < 1:
            raise ValueError(f"VoiceActivity: B = {B}")
        if self.R < self.window + self.hangover + 1:
            raise ValueError(f"VoiceActivity: ring = {ring} below window + hangover + 1 = {self.window + self.hangover + 1}")
        self.frames = self.taken = 0
        self._carry = [torch.zeros(self.B, self.frame, device=self.device, dtype=torch.float32) for _ in range(2)]
        self._carry_n = self._cur = 0
        self._e = torch.zeros(self.B, self.R, device=self.device, dtype=torch.float64)
        self._flags = torch.zeros(self.B, self.R, device=self.device, dtype=torch.uint8)

    def _run(self, x, final):
        k = x.shape[-1]
        total = self._carry_n + k
        n_new = total // self.frame + (1 if final and total % self.frame else 0)
        if n_new > self.R - self.window - self.hangover:
            raise ValueError(f"a push that completes {n_new} frames; ring = {self.R} holds window + hangover + "
                             f"{self.R - self.window - self.hangover}")
        src, dst = self._carry[self._cur], self._carry[1 - self._cur]
        ops.vad_energy(x, self._e, self.frame, f0=self.frames, R=self.R, carry_in=src, carry_n=self._carry_n, carry_out=dst, final=final)
        self._cur, self._carry_n = 1 - self._cur, (0 if final else total % self.frame)
        if n_new:
            ops.vad_decide(self._e, self.frames, n_new, self.window, self.hangover, self.margin, self.thr_abs, self.frame, R=self.R,
                           ring=self._flags)
            self.frames += n_new

    def push(self, block):
        self._run(self._block(block), False)

    def finish(self):
        """Decides the partial last frame, if there is one; the session takes no more audio."""
        if not self._done and self._carry_n:
            # the unprocessed tail is the block; the carry keeps only the sample before it
            tail = self._carry[self._cur][:, 1:1 + self._carry_n]
            self._carry_n = 0
            self._run(tail, True)
        self._done = True

    def _window(self, n):
        n = int(n)
        if n < 1:
            raise ValueError(f"take({n}): at least one frame")
        if self.taken + n > self.frames:
            raise ValueError(f"take({n}): only {self.frames - self.taken} decided frames are not yet taken")
        if self.taken < self.frames - self.R:
            raise ValueError(f"take({n}): frame {self.taken} has left the ring of {self.R} (frames decided: {self.frames})")
        return n

    def take(self, n, out=None):
        n = self._window(n)
        if out is None:
            out = torch.empty(self.B, n, device=self.device, dtype=torch.uint8)
        ops.vad_take(self._flags, self.taken, n, out)
        self.taken += n
        return out

    def energies(self, n):
        """(B, n) float64: the energies of the last n decided frames (a copy out of the ring; for tests and meters)."""
        if not 1 <= n <= min(self.frames, self.R):
            raise ValueError(f"energies({n}): {min(self.frames, self.R)} frames are in the ring")
        return self._ring_tail(self._e, self.frames, n)


class AutoGain(_Stage):
    """Causal level control over B parallel streams, one block at a time:

        agc = AutoGain(B)                                    # rate 24000, -23 LUFS over 3 s, ceiling -1 dBFS, 120 samples ahead
        y = agc.push(block)                                  # (B, 1, k) or (B, k) float32 on the GPU, any k >= 1 -> the same shape
        tail = agc.finish()                                  # the last `lookahead` samples

    The pushes and finish(), concatenated, are ops.level of the whole signal: `lookahead` zeros' worth of delay (`latency`
    seconds), then the levelled signal.  For the same gains the samples are the offline call's bit for bit, for any chunking;
    the gains themselves agree to fp64 rounding (the K-weighting filter's chunk boundaries move with the blocks, as in
    LoudnessMeter).  push is at most three launches' worth of C calls -- fac_kweight_energy, carrying the filter state and the
    position inside the current 100 ms sub-block; fac_agc_gains when the block completes a sub-block; fac_agc_apply, which
    also moves the last 2 * lookahead gained samples from one carry buffer into the other -- reads nothing back and allocates
    nothing but its output once the scratch has seen the largest block.  Energies and gains live in device rings of `ring`
    sub-blocks; a push that crosses the end of the ring (once every ring / 10 seconds), or is longer than ring - window - 2
    sub-blocks, is run as two or more.  It runs eagerly, outside the sessions' captured graphs.

    reset(rows) restarts the given rows on the device, so that a pool can hand a slot to a new stream: filter state, limiter
    carry, energies and gains of those rows are cleared and their window and ramp start over at the next line of the 100 ms
    grid, which all rows share.  Called when `samples` is a multiple of the sub-block (rate / 10), the rows then equal a fresh
    stream bit for bit; in between, the samples up to the next grid line pass at unit gain and are not measured.  The other
    rows are not touched.  The defaults were not tuned by listening."""

    def __init__(self, B, rate=MODEL_RATE, target_db=-23.0, window=30, max_boost_db=30.0, max_cut_db=30.0, ceiling_db=-1.0,
                 lookahead=120, ring=256, device="cuda"):
        self.p = ops.agc_params(rate, target_db, window, max_boost_db, max_cut_db, ceiling_db, lookahead)
        self.B, self.rate, self.R, self.device = int(B), int(rate), int(ring), torch.device(device)
        if self.B < 1:
            raise ValueError(f"AutoGain: B = {B}")
        if self.R < self.p.W + 8:
            raise ValueError(f"AutoGain: ring = {ring} below window + 8 = {self.p.W + 8}")
        self.S, self.lookahead, self.latency = self.p.S, self.p.LA, self.p.LA / self.rate
        self.samples = 0
        f64 = dict(device=self.device, dtype=torch.float64)
        self._e = torch.zeros(self.B, self.R, **f64)
        self._G = torch.zeros(self.B, self.R, **f64)
        self._g = torch.ones(self.B, self.R, **f64)
        self._state = torch.zeros(self.B, 4, **f64)
        self._j_start = torch.zeros(self.B, device=self.device, dtype=torch.int64)
        self._carry = [torch.zeros(self.B, 2 * self.p.LA, **f64) for _ in range(2)]
        self._cur = 0
        self.peak = torch.zeros(self.B, device=self.device, dtype=torch.float32)
        self._ws = None

    @property
    def decided(self):
        """Sub-blocks whose gain is decided (on the host)."""
        return self.samples // self.S

    def _run(self, x):
        k = x.shape[1]
        j0, offset = divmod(self.samples, self.S)
        need = ops._lib.load().fac_kweight_ws_bytes(self.B, k)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, device=self.device, dtype=torch.uint8)
        ops.loudness_energies(x, self.rate, state=self._state, offset=offset, out=self._e[:, j0 % self.R:], peak=self.peak,
                              state_out=self._state, ws=self._ws)
        n_new = (self.samples + k) // self.S - j0
        if n_new:
            ops.agc_gains(self._e, self.p, j0, n_new, R=self.R, j_start=self._j_start, G=self._G, g=self._g)
        src, dst = self._carry[self._cur], self._carry[1 - self._cur]
        y = ops.agc_apply(x, self._g, self.p, n0=self.samples, R=self.R, j_start=self._j_start, carry_in=src, carry_out=dst, flush=False)
        self._cur ^= 1
        self.samples += k
        return y

    def _room(self):
        j0, offset = divmod(self.samples, self.S)
        return min(self.R - j0 % self.R, self.R - self.p.W - 2) * self.S - offset          # up to the ring's end, and within its reach

    push = _Stage._push_pieces

    def finish(self):
        """(B, lookahead) float32: the samples the limiter was still holding back; the stream takes no more audio."""
        self._close()
        return ops.agc_apply(None, self._g, self.p, n0=self.samples, R=self.R, j_start=self._j_start, carry_in=self._carry[self._cur],
                             flush=True, k=0)

    def gains(self, n):
        """-> (G (B, n) float64 dB, g (B, n) float64 linear) of the last n decided sub-blocks (a copy out of the rings; for tests
        and meters)."""
        if not 1 <= n <= min(self.decided, self.R):
            raise ValueError(f"gains({n}): {min(self.decided, self.R)} decided gains are in the ring")
        return self._ring_tail(self._G, self.decided, n), self._ring_tail(self._g, self.decided, n)

    def reset(self, rows):
        """Puts the given rows (indices on the host) back into the state of a fresh stream, on the device."""
        idx = self._rows_idx(rows, "reset")
        if idx is None:
            return
        for t, v in ((self._state, 0.0), (self._carry[self._cur], 0.0), (self._e, 0.0), (self._G, 0.0), (self._g, 1.0), (self.peak, 0.0)):
            t.index_fill_(0, idx, v)
        self._j_start.index_fill_(0, idx, -(-self.samples // self.S))


class _FrontEndSession:
    """A session that takes audio, with one front-end stage in front of it: what LevelledSession, DenoisedSession and
    EchoCancelledSession share.  `stage` is the stage's class, built with the session's B, the rate it takes its audio at and
    its device, and kept under the attribute `name`; prime and push hand the session what the stage's push makes of their
    arguments, every other attribute of the session reads through."""

    def __init__(self, session, stage, name, **parameters):
        if not hasattr(session, "prime_samples") or not session.prime_samples:
            raise ValueError(f"{type(self).__name__}: this session takes codes, not audio")
        self.session = session
        self.rate = int(getattr(session, "in_rate", MODEL_RATE))
        inner = session
        while not hasattr(inner, "B"):                               # a ResampledSession keeps them on the session it wraps
            inner = inner.session
        self.B, self.device = inner.B, inner.device
        self._stage = stage(self.B, self.rate, device=self.device, **parameters)
        setattr(self, name, self._stage)
        self.latency_in = self._stage.latency + getattr(session, "latency_in", 0.0)

    def __getattr__(self, name):
        if name == "session":
            raise AttributeError(name)
        return getattr(self.session, name)

    def prime(self, *audio):
        return self.session.prime(self._stage.push(*audio))

    def push(self, *audio):
        return self.session.push(self._stage.push(*audio))

    def finish(self):
        return self.session.finish()

    def set_target(self, timbre):
        return self.session.set_target(timbre)


class LevelledSession(_FrontEndSession):
    """A StreamingCodec, a StreamingConverter or a ResampledSession of one whose input goes through an AutoGain first:

        codec = LevelledSession(StreamingCodec(model, timbre), target_db=-23.0)
        out = codec.prime(wave[:, :, :4800]); out = codec.push(wave[:, :, t:t + 480]); out = codec.finish()

    Same surface and the same dicts as the wrapped session (whose other attributes read through).  The AutoGain runs at the
    rate the session takes its audio at, eagerly, around the session's captured graphs: at most three C calls per push.  The
    session sees `lookahead` zeros and then the levelled input, cut off where the pushed audio ends; `latency_in` is that delay
    in seconds, on top of the wrapped session's own.  **parameters: AutoGain's (target_db, window, max_boost_db, max_cut_db,
    ceiling_db, lookahead, ring), whose defaults were not tuned by listening.  The applied gain does not travel with the codes."""

    def __init__(self, session, **parameters):
        super().__init__(session, AutoGain, "agc", **parameters)
        self.lookahead = self.agc.lookahead


class NoiseSuppressor(_Stage):
    """Spectral noise suppression over B parallel streams, one block at a time:

        ns = NoiseSuppressor(B)                              # M = 8, W = 96, over = 4.0, max_atten_db = 15.0
        y = ns.push(block)                                   # (B, 1, k) or (B, k) float32 on the GPU, any k >= 1 -> the same shape
        tail = ns.finish()                                   # the last 512 samples

    The pushes and finish(), concatenated, are 512 zeros and then ops.denoise(whole signal).y, bit for bit, for any chunking
    (`latency` seconds at `rate`; the definition is in samples, any rate is accepted).  push is three C calls -- fac_ns_power
    for the frames the block completes, which also moves the last 1023 input samples from one carry buffer into the other;
    fac_ns_gains for those frames, when there are any; fac_ns_synth for the block's outputs -- reads nothing back and allocates
    nothing but its output.  Power spectra and gains live in device rings of `ring` frames; a push that completes more than
    ring - max(M + W - 2, 2) frames is run as several.  The synthesis transforms the frames over its outputs again instead of
    keeping half-finished output between pushes: the state is the input carry, the two rings and the rows' starts.  It runs
    eagerly, outside the sessions' captured graphs.

    reset(rows) restarts the given rows on the device: their carry and rings are cleared and their stream begins at `samples`;
    the 512 samples of the old stream that were not played yet come out as zeros, and the rows then give row b of
    ops.denoise(concat(zeros(samples), new), starts=samples), 512 samples late, bit for bit.  The other rows are not touched.
    A stream that starts in speech has that speech for its noise floor until the window has seen a pause.  The defaults were
    not tuned by listening."""

    def __init__(self, B, rate=MODEL_RATE, M=8, W=96, over=4.0, max_atten_db=15.0, ring=128, device="cuda"):
        self.p = ops.ns_params(M, W, over, max_atten_db)
        self.B, self.rate, self.R, self.device = int(B), int(rate), int(ring), torch.device(device)
        if self.B < 1:
            raise ValueError(f"NoiseSuppressor: B = {B}")
        self._reach = max(self.p.M + self.p.W - 2, 2)                # older frames a push still reads in the rings
        if self.R < self._reach + 2:
            raise ValueError(f"NoiseSuppressor: ring = {ring} below the {self._reach} older frames a push reaches plus the two frames of its own")
        self.delay, self.latency = ops.NS_DELAY, ops.NS_DELAY / self.rate
        self.samples = 0
        f64 = dict(device=self.device, dtype=torch.float64)
        self._P = torch.zeros(self.B, self.R, ops.NS_BINS, **f64)
        self._G = torch.ones(self.B, self.R, ops.NS_BINS, **f64)
        self._start = torch.zeros(self.B, device=self.device, dtype=torch.int64)
        self._carry = [torch.zeros(self.B, ops.NS_CARRY, device=self.device, dtype=torch.float32) for _ in range(2)]
        self._cur = 0

    @property
    def frames(self):
        """Frames whose gains are decided (on the host)."""
        return self.samples // ops.NS_H

    def _run(self, x):
        k = x.shape[1]
        f0 = self.frames
        n_new = (self.samples + k) // ops.NS_H - f0
        src, dst = self._carry[self._cur], self._carry[1 - self._cur]
        ops.ns_power(x, self._P, n0=self.samples, f0=f0, n_new=n_new, R=self.R, starts=self._start, carry_in=src, carry_out=dst)
        if n_new:
            ops.ns_gains(self._P, self.p, f0, n_new, R=self.R, starts=self._start, G=self._G)
        y = ops.ns_synth(x, self._G, n0=self.samples, m0=self.samples - self.delay, n_out=k, R=self.R, starts=self._start, carry_in=src)
        self._cur ^= 1
        self.samples += k
        return y

    def _room(self):
        return (self.R - self._reach) * ops.NS_H - self.samples % ops.NS_H         # completes at most ring - reach frames

    push = _Stage._push_pieces

    def finish(self):
        """(B, 512) float32: the samples still held back; the stream takes no more audio."""
        self._close()
        f0 = self.frames
        n_new = ops.ns_frames(self.samples) - f0                     # the one or two frames that reach past the end
        src = self._carry[self._cur]
        if n_new:
            ops.ns_power(None, self._P, n0=self.samples, f0=f0, n_new=n_new, R=self.R, starts=self._start, carry_in=src, k=0)
            ops.ns_gains(self._P, self.p, f0, n_new, R=self.R, starts=self._start, G=self._G)
        self._final = f0 + n_new
        return ops.ns_synth(None, self._G, n0=self.samples, m0=self.samples - self.delay, n_out=self.delay, R=self.R, starts=self._start,
                            carry_in=src, k=0)

    def gains(self, n):
        """-> G (B, n, 257) float64: the gains of the last n decided frames (a copy out of the ring; for tests and meters)."""
        have = self._final if self._done else self.frames
        if not 1 <= n <= min(have, self.R):
            raise ValueError(f"gains({n}): {min(have, self.R)} decided frames are in the ring")
        return self._ring_tail(self._G, have, n)

    def reset(self, rows):
        """Puts the given rows (indices on the host) back into the state of a fresh stream that begins at `samples`, on the device."""
        idx = self._rows_idx(rows, "reset")
        if idx is None:
            return
        for t, v in ((self._carry[self._cur], 0.0), (self._P, 0.0), (self._G, 1.0)):
            t.index_fill_(0, idx, v)
        self._start.index_fill_(0, idx, self.samples)


class DenoisedSession(_FrontEndSession):
    """A StreamingCodec, a StreamingConverter, a ResampledSession or a LevelledSession of one whose input goes through a
    NoiseSuppressor first:

        codec = DenoisedSession(StreamingCodec(model, timbre), max_atten_db=15.0)
        out = codec.prime(wave[:, :, :4800]); out = codec.push(wave[:, :, t:t + 480]); out = codec.finish()

    Same surface and the same dicts as the wrapped session (whose other attributes read through).  The suppressor runs at the
    rate the session takes its audio at, eagerly, around the session's captured graphs: three C calls per push.  The session
    sees 512 zeros and then the suppressed input, cut off where the pushed audio ends; `latency_in` is that delay in seconds, on
    top of the wrapped session's own.  It nests with LevelledSession either way round: the outer stage runs first.
    **parameters: NoiseSuppressor's (M, W, over, max_atten_db, ring), whose defaults were not tuned by listening."""

    def __init__(self, session, **parameters):
        super().__init__(session, NoiseSuppressor, "ns", **parameters)


class EchoCanceller(_Stage):
    """Acoustic echo cancellation over B parallel streams, one block at a time:

        aec = EchoCanceller(B)                               # P = 8, mu = 0.5, beta = 1.0, delta = 1e-6, delay = 0
        e = aec.push(mic, far)                               # two (B, 1, k) or (B, k) float32 on the GPU, any k >= 1 -> mic's shape
        tail = aec.finish()                                  # the last 256 samples

    far is what goes to the loudspeaker (the `wave` of a StreamingDecoder or StreamingReceiver in the same process: a device
    tensor already), mic what comes back from the microphone, sample for sample alongside it; `delay` samples of known
    playout-to-capture delay move the filter's P * 256 taps to where the echo is.  The pushes and finish(), concatenated, are
    256 zeros and then ops.echo_cancel(whole mic, whole far).e, bit for bit, for any chunking (`latency` seconds at `rate`;
    the definition is in samples, any rate is accepted).  The filter is recursive in time; the chunking cannot show because
    the blocks lie on an absolute grid of 256 samples and a block is computed once, when a push completes it, by the kernel of
    the offline call.  push is one C call -- fac_aec_run, which computes the blocks the push completes, hands out the e of
    earlier blocks that were not due yet, keeps those that are not due now, and moves the pending microphone samples and the
    last 511 + delay far-end samples from one carry buffer into the other -- reads nothing back and allocates nothing but its
    output.  The state is all on the device: the two carries, the spectra of the last P far-end blocks, the weights, a ring
    of 256 e samples, the rows' starts and adapt flags.  It runs eagerly, outside the sessions' captured graphs.

    set_adapt(rows, on) freezes or releases the given rows' filters from the next block on; a frozen row still filters.
    reset(rows) restarts the given rows on the device: their stream begins at `samples`, the filter starts from zero at the
    block that holds that sample, the 256 samples of the old stream that were not played yet come out as zeros, and the rows
    then give row b of ops.echo_cancel(concat(old, new), concat(old, new), starts=samples), 256 samples late, bit for bit.
    The other rows are not touched.  A delay nobody knows is found by AlignedEchoCanceller.  There is no
    clock-drift compensation and no residual-echo suppressor; the defaults were not tuned by listening."""

    def __init__(self, B, rate=MODEL_RATE, P=8, mu=0.5, beta=1.0, delta=1e-6, delay=0, adapt=True, device="cuda"):
        self.p = ops.aec_params(P, mu, beta, delta, delay)
        self.B, self.rate, self.device = int(B), int(rate), torch.device(device)
        if self.B < 1:
            raise ValueError(f"EchoCanceller: B = {B}")
        self.delay, self.latency = ops.AEC_DELAY, ops.AEC_DELAY / self.rate
        self.far_delay = self.p.delay
        self.samples = 0
        n_w, n_x, n_mic, n_far, n_e = ops.aec_state_sizes(self.p.P, self.p.delay)
        f32 = dict(device=self.device, dtype=torch.float32)
        self._W = torch.zeros(self.B, self.p.P, ops.AEC_BINS, 2, device=self.device, dtype=torch.float64)
        self._X = torch.zeros_like(self._W)
        assert self._W[0].numel() == n_w == n_x
        self._mic = [torch.zeros(self.B, n_mic, **f32) for _ in range(2)]
        self._far = [torch.zeros(self.B, n_far, **f32) for _ in range(2)]
        self._ring = torch.zeros(self.B, n_e, **f32)
        self._start = torch.zeros(self.B, device=self.device, dtype=torch.int64)
        self._adapt = torch.full((self.B,), 1 if adapt else 0, device=self.device, dtype=torch.int32)
        self._cur = 0

    @property
    def blocks(self):
        """Blocks that are complete (on the host)."""
        return self.samples // ops.AEC_H

    def _run(self, mic, far, k, n_blk, n_out, carry_out):
        c = self._cur
        return ops.aec_run(mic, far, self.p, self._W, self._X, n0=self.samples, m0=self.samples - self.delay, n_out=n_out, blk0=self.blocks,
                           n_blk=n_blk, starts=self._start, adapt=self._adapt, mic_carry=(self._mic[c], self._mic[1 - c] if carry_out else None),
                           far_carry=(self._far[c], self._far[1 - c] if carry_out else None), e_ring=self._ring, k=k)

    def push(self, mic, far):
        m, f = self._block(mic), ops._rows(far, self._what)
        if m.shape != f.shape:
            raise ValueError(f"push() takes two (B = {self.B}, 1, k) or (B, k) of one length k >= 1, got {tuple(mic.shape)} and {tuple(far.shape)}")
        k = m.shape[1]
        y = self._run(m, f, k, (self.samples + k) // ops.AEC_H - self.blocks, k, True)
        self._cur ^= 1
        self.samples += k
        return y.view(mic.shape)

    def finish(self):
        """(B, 256) float32: the samples still held back, the open block padded with zeros; the stream takes no more audio."""
        self._close()
        return self._run(None, None, 0, 1 if self.samples % ops.AEC_H else 0, self.delay, False)

    def weights(self):
        """-> W (B, P, 257, 2) float64: the filters after the last complete block (a copy; for tests and meters)."""
        return self._W.clone()

    def set_adapt(self, rows, on):
        """The given rows (indices on the host) adapt, or only filter, from the next block on."""
        idx = self._rows_idx(rows, "set_adapt")
        if idx is not None:
            self._adapt.index_fill_(0, idx, 1 if on else 0)

    def reset(self, rows):
        """Restarts the given rows (indices on the host) as a stream that begins at `samples`, on the device."""
        idx = self._rows_idx(rows, "reset")
        if idx is not None:
            self._start.index_fill_(0, idx, self.samples)


class EchoCancelledSession(_FrontEndSession):
    """A StreamingCodec, a StreamingConverter, a ResampledSession, a LevelledSession or a DenoisedSession of one whose input
    goes through an EchoCanceller first:

        codec = EchoCancelledSession(DenoisedSession(StreamingCodec(model, timbre)), P=8, delay=0)
        out = codec.prime(mic[:, :, :4800], far[:, :, :4800]); out = codec.push(mic[:, :, t:t + 480], far[:, :, t:t + 480])
        out = codec.finish()

    The surface and the dicts of the wrapped session (whose other attributes read through), except that prime and push take
    the far end next to the microphone, as a device tensor of the same shape: typically the `wave` a StreamingDecoder or a
    StreamingReceiver in the same process has just produced.  This is the outermost stage: the canceller models a linear path,
    so it must see the microphone before any gain control or suppressor has changed it, and the other wrappers' push takes one
    argument.  The canceller runs at the rate the session takes its audio at, eagerly, around the session's captured graphs:
    one C call per push.  The session sees 256 zeros and then the cancelled input, cut off where the pushed audio ends;
    `latency_in` is that delay, 256 / rate seconds, on top of the wrapped session's own.  **parameters: EchoCanceller's (P, mu,
    beta, delta, delay, adapt), whose defaults were not tuned by listening.  delay="auto" puts an AlignedEchoCanceller there
    instead (two C calls per push, the same latency), which also takes ops.echo_delay_params' names."""

    def __init__(self, session, **parameters):
        auto = isinstance(parameters.get("delay"), str)
        if auto:
            if parameters["delay"] != "auto":
                raise ValueError(f"EchoCancelledSession: delay = {parameters['delay']!r} (an integer or \"auto\")")
            parameters = {k: v for k, v in parameters.items() if k != "delay"}
        super().__init__(session, AlignedEchoCanceller if auto else EchoCanceller, "aec", **parameters)


class EchoDelayTracker(_Stage):
    """The playout-to-capture delay of B parallel streams, found and followed on the device, and the far end moved by it
    (DESIGN.md 36):

        trk = EchoDelayTracker(B)                            # max_delay = 16384, thr = 0.1, hold = 8, .. (ops.echo_delay_params)
        aligned = trk.push(mic, far)                         # two (B, 1, k) or (B, k) float32 on the GPU, any k >= 1 -> far's shape
        trk.delay(), trk.confidence()                        # (B,) int32, -1 while not latched; (B,) float64

    aligned is far[n - used], `used` being the latched delay less a margin as of the last frame that ended before the sample's
    block of 256: every sample comes out in the push that brings it (`latency` is 0), and the pushes, concatenated, are
    ops.echo_delay(whole mic, whole far).far, bit for bit, for any chunking -- frames lie on the canceller's absolute grid and a
    frame is computed once, when a push completes it, by the kernel of the offline call.  push is one C call (fac_edelay_run;
    a push that completes more than `ring` frames is run as several), reads nothing back and allocates nothing but its output.
    The state is all on the device: the cross-spectra of the L + 1 lags, the far-end spectra and activities of the last L + 1
    frames, the policy's integers, the last 511 microphone samples and the last max_delay + 511 far-end samples in rings indexed
    by the absolute sample, the rows' starts, and rings of the last `ring` frames' decisions (frames(n)).

    reset(rows) restarts the given rows on the device: their stream begins at `samples`, and they then give row b of
    ops.echo_delay(concat(old, new), concat(old, new), starts=samples), bit for bit.  The other rows are not touched.  There is
    no finish(): nothing is held back.  The defaults were not tuned by listening."""

    latency = 0.0

    def __init__(self, B, rate=MODEL_RATE, ring=64, device="cuda", **params):
        self.p = ops.echo_delay_params(**params)
        self.B, self.rate, self.R, self.device = int(B), int(rate), int(ring), torch.device(device)
        if self.B < 1:
            raise ValueError(f"EchoDelayTracker: B = {B}")
        if self.R < 1:
            raise ValueError(f"EchoDelayTracker: ring = {ring} below 1 frame")
        self.samples = 0
        self._st = ops.edelay_state(self.B, self.p, self.device, rings=True)
        self._start = torch.zeros(self.B, device=self.device, dtype=torch.int64)
        i32 = dict(device=self.device, dtype=torch.int32)
        self._fr = dict(raw=torch.full((self.B, self.R), -1, **i32), locked=torch.full((self.B, self.R), -1, **i32),
                        used=torch.full((self.B, self.R), -1, **i32), conf=torch.zeros(self.B, self.R, device=self.device, dtype=torch.float64),
                        ok=torch.zeros(self.B, self.R, device=self.device, dtype=torch.uint8))

    @property
    def n_frames(self):
        """Frames that are complete (on the host): frame m = 1 .. n_frames."""
        return ops.echo_delay_frames(self.samples)

    def _run(self, m, f):
        k = m.shape[1]
        frm0 = max(self.samples // ops.AEC_H, 1)
        y = ops.edelay_run(m, f, self.p, self._st, n0=self.samples, frm0=frm0, n_frm=max((self.samples + k) // ops.AEC_H - frm0, 0),
                           starts=self._start, frames=self._fr, f_ring=self.R)
        self.samples += k
        return y

    def push(self, mic, far):
        m, f = self._block(mic), ops._rows(far, self._what)
        if m.shape != f.shape:
            raise ValueError(f"push() takes two (B = {self.B}, 1, k) or (B, k) of one length k >= 1, got {tuple(mic.shape)} and {tuple(far.shape)}")
        parts, t, k = [], 0, m.shape[1]
        while t < k:
            n = min(k - t, self.R * ops.AEC_H - self.samples % ops.AEC_H)     # completes at most `ring` frames
            parts.append(self._run(m[:, t:t + n], f[:, t:t + n]))
            t += n
        return (parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)).view(far.shape)

    def delay(self):
        """-> (B,) int32 on the device: the latched delay in samples, -1 while a row has not latched (a copy)."""
        return self._st["pol"][:, 2].clone()

    def confidence(self):
        """-> (B,) float64 on the device: the best lag's score at the last frame (a copy)."""
        return self._st["conf_last"].clone()

    def frames(self, n):
        """-> (raw, locked, used, conf, ok), each (B, n): the last n frames' decisions (copies out of the rings; for tests and meters)."""
        have = self.n_frames + 1                                     # frame m lies at slot m % ring; there is no frame 0
        if not 1 <= n <= min(have - 1, self.R):
            raise ValueError(f"frames({n}): {min(have - 1, self.R)} frames are in the ring")
        return tuple(self._ring_tail(self._fr[name], have, n) for name in ("raw", "locked", "used", "conf", "ok"))

    def reset(self, rows):
        """Restarts the given rows (indices on the host) as a stream that begins at `samples`, on the device."""
        idx = self._rows_idx(rows, "reset")
        if idx is None:
            return
        self._start.index_fill_(0, idx, self.samples)
        pol = self._st["pol"]
        pol[:, 0].index_fill_(0, idx, -1), pol[:, 1].index_fill_(0, idx, 0), pol[:, 2].index_fill_(0, idx, -1)
        pol[:, 3].index_fill_(0, idx, self.p.delay0)
        self._st["conf_last"].index_fill_(0, idx, 0.0)


class AlignedEchoCanceller(_Stage):
    """An EchoDelayTracker and, behind it, an EchoCanceller with delay = 0: echo cancellation for streams whose
    playout-to-capture delay nobody knows:

        aec = AlignedEchoCanceller(B, P=8, max_delay=16384)
        e = aec.push(mic, far); tail = aec.finish(); aec.tracker.delay()

    EchoCanceller's surface (push, finish, weights, set_adapt, reset, `latency`, `delay`, `samples`); the output is, bit for bit,
    EchoCanceller(delay=0).push(mic, EchoDelayTracker.push(mic, far)): two C calls per push, nothing read back.  **params go to
    the two stages by name: ops.echo_delay_params' names and `ring` to the tracker (`tracker`), P, mu, beta, delta and adapt to
    the canceller (`canceller`); a name of neither, and `delay`, is refused.  reset(rows) resets both.  When the tracker
    re-latches, the canceller's filter is not restarted: it re-converges on the moved far end by itself."""

    def __init__(self, B, rate=MODEL_RATE, device="cuda", **params):
        mine = {k: v for k, v in params.items() if k in ops.ECHO_DELAY_NAMES or k == "ring"}
        rest = {k: v for k, v in params.items() if k not in mine}
        unknown = sorted(k for k in rest if k not in ("P", "mu", "beta", "delta", "adapt"))
        if unknown:
            raise ValueError(f"AlignedEchoCanceller: {unknown} are parameters of neither the tracker nor the canceller (the delay is tracked)")
        self.tracker = EchoDelayTracker(B, rate, device=device, **mine)
        self.canceller = EchoCanceller(B, rate, delay=0, device=device, **rest)
        self.B, self.rate, self.device, self.p = self.canceller.B, self.canceller.rate, self.canceller.device, self.canceller.p
        self.delay, self.latency, self.far_delay = self.canceller.delay, self.canceller.latency, "auto"

    @property
    def samples(self):
        return self.canceller.samples

    def push(self, mic, far):
        self._block(mic)
        return self.canceller.push(mic, self.tracker.push(mic, far))

    def finish(self):
        self._close()
        return self.canceller.finish()

    def weights(self):
        return self.canceller.weights()

    def set_adapt(self, rows, on):
        self.canceller.set_adapt(rows, on)

    def reset(self, rows):
        self.tracker.reset(rows)
        self.canceller.reset(rows)


class ResampledSession:
    """A StreamingCodec / StreamingConverter / StreamingDecoder that takes its audio at `in_rate` and gives it at `out_rate`:

        vc = ResampledSession(StreamingConverter(codec, redecoder, timbre), in_rate=48000, out_rate=48000)
        out = vc.prime(wave48[:, :, :9600])              # prime_samples * in_rate / 24000 samples
        out = vc.push(wave48[:, :, t:t + 960])           # 480 * in_rate / 24000 samples per hop
        out = vc.finish()

    Same surface and the same dicts as the wrapped session (a StreamingDecoder's calls take codes and return the wave alone), with
    `wave` at out_rate and the codes untouched; finish() appends what the output resampler was holding back.  Each side is one
    StreamingResampler launch run eagerly around the session's captured graphs, and adds that resampler's `latency`
    (`latency_in`, `latency_out`; a rate of None or 24000 adds nothing).  The session sees `delay_in` zeros and then the
    resampled input, cut off where the pushed audio ends."""

    def __init__(self, session, in_rate=None, out_rate=None, quality="fast"):
        in_rate = MODEL_RATE if in_rate is None else in_rate
        out_rate = MODEL_RATE if out_rate is None else out_rate
        ops.resample_table(in_rate, MODEL_RATE, quality)                   # ValueError: rates, ratio, quality
        ops.resample_table(MODEL_RATE, out_rate, quality)
        takes_audio = hasattr(session, "prime_samples")
        if not takes_audio and in_rate != MODEL_RATE:
            raise ValueError("in_rate: this session takes codes, not audio")
        if HOP * in_rate % MODEL_RATE:
            raise ValueError(f"in_rate {in_rate}: a hop of {HOP} samples at {MODEL_RATE} Hz is no whole number of samples there")
        if FRAME * out_rate % MODEL_RATE:
            raise ValueError(f"out_rate {out_rate}: a frame of {FRAME} samples at {MODEL_RATE} Hz is no whole number of samples there")
        self.session = session
        self.in_rate, self.out_rate = int(in_rate), int(out_rate)
        self.hop_samples = HOP * self.in_rate // MODEL_RATE
        self.prime_samples = session.prime_samples * self.in_rate // MODEL_RATE if takes_audio else None
        B, dev = session.B, session.device
        self.rs_in = StreamingResampler(B, self.in_rate, MODEL_RATE, quality, dev) if self.in_rate != MODEL_RATE else None
        self.rs_out = StreamingResampler(B, MODEL_RATE, self.out_rate, quality, dev) if self.out_rate != MODEL_RATE else None
        self.delay_in = self.rs_in.delay if self.rs_in else 0
        self.delay_out = self.rs_out.delay if self.rs_out else 0
        self.latency_in = self.rs_in.latency if self.rs_in else 0.0
        self.latency_out = self.rs_out.latency if self.rs_out else 0.0

    def _in(self, wave, want):
        if self.rs_in is None:
            return wave
        if wave.shape[-1] != want:
            raise ValueError(f"this call wants exactly {want} samples at {self.in_rate} Hz, got {wave.shape[-1]}")
        return self.rs_in.push(wave)

    def _out(self, r, final=False):
        if self.rs_out is None:
            return r
        wave = r["wave"] if isinstance(r, dict) else r
        parts = [self.rs_out.push(wave)] if wave is not None else []
        if final:
            parts.append(self.rs_out.finish())
        wave = None if not parts else parts[0] if len(parts) == 1 else torch.cat(parts, dim=-1)
        return dict(r, wave=wave) if isinstance(r, dict) else wave

    def prime(self, first):
        return self._out(self.session.prime(self._in(first, self.prime_samples) if self.prime_samples else first))

    def push(self, hop):
        return self._out(self.session.push(self._in(hop, self.hop_samples) if self.prime_samples else hop))

    def finish(self):
        if hasattr(self.session, "finish"):
            return self._out(self.session.finish(), final=True)
        return self.rs_out.finish() if self.rs_out is not None else None

    def set_target(self, timbre):
        return self.session.set_target(timbre)


# ------------------------------------------------------------------------------------ what travels between the two halves
class CodePacketizer:
    """Sender side of the link between StreamingCodec / StreamingConverter and StreamingDecoder: every push's codes as bytes.

        tx = CodePacketizer(n_q=(1, 2, 3))                   # quantizer counts of the codes that will be sent
        headers = tx.header(timbre)                          # once: one stream-header blob per stream (timbre (B, 1024) or None)
        packets = tx.packet(out["codes"])                    # every call that returned codes: one packet per stream

    packet() is one ops.pack_codes launch on the current stream and one device-to-host copy of the packed rows ((B, 4 ceil(k Q
    bits / 32)) bytes instead of three int64 tensors); the codes may be a session's static graph buffers, they are read before
    packet() returns.  It sits outside the captured graphs.  A packet is b"FP", seq uint16 (wrapping, the same for all streams
    of a push), n_frames uint16, ceil(k Q bits / 8) payload bytes, CRC-32 (bitstream.write_packet).  codes with fewer entries
    than three (StreamingConverter emits [p, c]) stand for n_q with trailing zeros.

    redundancy = (rp, rc, rr), elementwise <= n_q (e.g. (1, 2, 0)): in-band redundancy.  Packets are then b"FQ"
    (bitstream.write_packet_fec): call j carries its own codes and, behind them, the leading rp / rc / rr quantizers of call
    j - 1 (none on the first call), so a receiver that waits one push (StreamingReceiver(delay=1)) can play a lost push at the
    lower rate.  Two pack launches into one buffer, still one device-to-host copy.  With None the packets are the bytes of before.

    dtx = dict(sid_every=8): discontinuous transmission.  packet(codes, active) then takes the push's voice
    activity flags, (B, k) uint8 on the device (VoiceActivity.take), which ride in the tail columns of the pack buffer: still one
    device-to-host copy -- and none of the flags on their own when VoiceActivity.take(k, out=tx.active_view(B, k, device)) wrote
    them there.  Per stream: a push with any active frame is a normal packet; of a run of pushes without one, the first and
    then every sid_every-th are SID packets (the same bytes with the magic's second letter in lower case: "silence follows"), the
    others are None: nothing is sent.  seq advances and the redundant layer is kept on every call, whatever is emitted.  With
    dtx=None (and no `active`) every byte is the byte of before."""

    def __init__(self, n_q, bits=10, codebook_size=1024, redundancy=None, dtx=None):
        from . import bitstream
        self.n_q = tuple(int(n) for n in n_q) + (0,) * (3 - len(n_q))
        bitstream._check_layout(bits, self.n_q, "CodePacketizer")
        self.bits, self.codebook_size, self.seq = int(bits), int(codebook_size), 0
        self.redundancy = None
        if redundancy is not None:
            self.redundancy = bitstream._check_red(redundancy, self.n_q, "CodePacketizer")
            if not sum(self.redundancy):
                raise ValueError("CodePacketizer: redundancy without a quantizer (pass None for plain packets)")
        self._red_prev = None                    # (k, per-stream redundant payload bytes) of the previous call
        self.sid_every = None
        if dtx is not None:
            dtx = dict(dtx)
            self.sid_every = int(dtx.pop("sid_every", 8))
            if dtx or self.sid_every < 1:
                raise ValueError(f"CodePacketizer: dtx = dict(sid_every >= 1), got sid_every = {self.sid_every} and {sorted(dtx)}")
        self._silent = None                      # per stream: pushes without an active frame in a row
        self._buf = {}                           # dtx: (B, k, device) -> the pack buffer, codes in front, flags in the tail

    def _pack_buf(self, B, k, device):
        key = (int(B), int(k), torch.device(device))
        if key not in self._buf:
            rb = ops.codes_row_bytes(k, sum(self.n_q), self.bits)
            rb_red = ops.codes_row_bytes(k, sum(self.redundancy), self.bits) if self.redundancy is not None else 0
            # rows of whole words (fac_codes_pack's row stride): the k flags are padded up to a multiple of 4 bytes
            self._buf[key] = (torch.zeros(key[0], rb + rb_red + (key[1] + 3) // 4 * 4, dtype=torch.uint8, device=key[2]), rb, rb_red)
        return self._buf[key]

    def active_view(self, B, k, device="cuda"):
        """dtx: the (B, k) uint8 tail columns of the pack buffer of pushes of k frames -- where packet(codes, active) wants the
        flags.  Pass it as VoiceActivity.take(k, out=...) and then as `active`: no copy is made."""
        if self.sid_every is None:
            raise ValueError("active_view(): the packetizer was built without dtx=")
        buf, rb, rb_red = self._pack_buf(B, k, device)
        return buf[:, rb + rb_red:rb + rb_red + int(k)]

    def header(self, timbre=None):
        from . import bitstream
        if not isinstance(timbre, torch.Tensor) or timbre.dim() != 2:
            raise ValueError("header(timbre): the receiver takes its timbre from the stream header; pass the session's (B, dim) tensor")
        _check_timbre(timbre, None, timbre.shape[1], "timbre")
        tim = timbre.detach().cpu().numpy()
        head = dict(bits=self.bits, n_q=self.n_q, sample_rate=MODEL_RATE, n_frames=0, n_samples=0,
                    codebook_size=self.codebook_size, timbre_dim=tim.shape[1], stream=True)
        return [bitstream.write(head, tim[b].tobytes(), b"") for b in range(tim.shape[0])]

    def packet(self, codes, active=None):
        codes = list(codes) + [None] * (3 - len(codes))
        got = tuple(0 if c is None else int(c.shape[1]) for c in codes)
        if got != self.n_q:
            raise ValueError(f"codes with {got} rows, the packetizer was built for n_q = {self.n_q}")
        k = next(c for c in codes if c is not None).shape[-1]
        if active is not None:
            return self._packet_dtx(codes, active, k)
        if self.redundancy is None:
            return self._emit(k, ops.pack_codes(codes, bits=self.bits).cpu().numpy())
        # primary rows and this push's redundant layer (its leading quantizers: strided views of the same codes) side by side
        # in one device buffer, one copy to the host
        red = [c[:, :n] if n else None for c, n in zip(codes, self.redundancy)]
        rb = ops.codes_row_bytes(k, sum(self.n_q), self.bits)
        rb_red = ops.codes_row_bytes(k, sum(self.redundancy), self.bits)
        dev = next(c for c in codes if c is not None).device
        buf = torch.empty(next(c for c in codes if c is not None).shape[0], rb + rb_red, dtype=torch.uint8, device=dev)
        ops.pack_codes(codes, bits=self.bits, out=buf[:, :rb])
        ops.pack_codes(red, bits=self.bits, out=buf[:, rb:])
        rows = buf.cpu().numpy()
        return self._emit(k, rows[:, :rb], rows[:, rb:])

    def _packet_dtx(self, codes, active, k):
        if self.sid_every is None:
            raise ValueError("packet(codes, active): the packetizer was built without dtx=")
        first = next(c for c in codes if c is not None)
        B = first.shape[0]
        if not isinstance(active, torch.Tensor) or not active.is_cuda or active.dtype != torch.uint8 or tuple(active.shape) != (B, k):
            raise ValueError(f"active must be a uint8 ({B}, {k}) tensor on the GPU (VoiceActivity.take), got "
                             f"{getattr(active, 'dtype', type(active))} {tuple(getattr(active, 'shape', ()))}")
        buf, rb, rb_red = self._pack_buf(B, k, first.device)
        ops.pack_codes(codes, bits=self.bits, out=buf[:, :rb])
        if rb_red:
            ops.pack_codes([c[:, :n] if n else None for c, n in zip(codes, self.redundancy)], bits=self.bits, out=buf[:, rb:rb + rb_red])
        tail = buf[:, rb + rb_red:rb + rb_red + k]
        if active.data_ptr() != tail.data_ptr() or active.stride() != tail.stride():
            tail.copy_(active)                                   # device to device; active_view() avoids it
        rows = buf.cpu().numpy()
        return self._emit(k, rows[:, :rb], rows[:, rb:rb + rb_red] if rb_red else None, rows[:, rb + rb_red:rb + rb_red + k])

    def _emit(self, k, rows, red_rows=None, active_rows=None):
        """Host part of packet(): the packed rows of this push (uint8 (B, >= payload bytes) arrays; red_rows: its redundant
        layer, kept for the next call; active_rows: its (B, k) voice activity flags under dtx) -> one entry per stream: a
        packet, or None for a suppressed push."""
        from . import bitstream
        B = rows.shape[0]
        n = bitstream.payload_bytes(k, sum(self.n_q), self.bits)
        seq, self.seq = self.seq, (self.seq + 1) & 0xFFFF
        kind = [0] * B                                           # 0 normal, 1 SID, None suppressed
        if self.sid_every is not None:
            if self._silent is None:
                self._silent = [0] * B
            for b in range(B):
                if active_rows is None or active_rows[b, :k].any():
                    self._silent[b] = 0
                else:
                    self._silent[b] += 1
                    kind[b] = 1 if (self._silent[b] - 1) % self.sid_every == 0 else None
        elif active_rows is not None:
            raise ValueError("voice activity flags for a packetizer built without dtx=")
        if self.redundancy is None:
            return [None if kind[b] is None else bitstream.write_packet(seq, k, rows[b, :n].tobytes(), sid=bool(kind[b]))
                    for b in range(B)]
        k_prev, prev = self._red_prev if self._red_prev is not None else (0, [b""] * B)
        n_red = bitstream.payload_bytes(k, sum(self.redundancy), self.bits)
        self._red_prev = (k, [red_rows[b, :n_red].tobytes() for b in range(B)])
        return [None if kind[b] is None else
                bitstream.write_packet_fec(seq, k, rows[b, :n].tobytes(), k_prev, self.redundancy, prev[b], sid=bool(kind[b]))
                for b in range(B)]


class CodeDepacketizer:
    """Receiver side: stream headers and packets in, code tensors for StreamingDecoder out.

        rx_codes = CodeDepacketizer(headers)                 # .timbre (B, dim) on the device, .n_q, .bits, .codebook_size
        rx = StreamingDecoder(model, rx_codes.timbre)
        wave = rx.prime(rx_codes.feed(packets))              # then rx.push(rx_codes.feed(packets)) per push

    feed() checks the packets on the host (bitstream.PacketReader: CRC, equal n_frames and seq across the streams, the
    sequence), then makes one host-to-device copy of the payload rows and one ops.unpack_codes launch -> [p, c, r] (B, n, k)
    int64.  ValueError for a corrupt packet or streams that disagree; bitstream.PacketLoss(missing=n) for a gap in the sequence,
    after which the same packets are accepted when fed again.  Nothing is concealed: what to play for lost frames is the
    caller's decision (StreamingDecoder has no notion of a missing push)."""

    def __init__(self, header_blobs, device="cuda"):
        import numpy as np
        from . import bitstream
        parsed = [bitstream.read(b) for b in header_blobs]
        if not parsed:
            raise ValueError("no stream headers")
        for i, (h, tim, _) in enumerate(parsed):
            if not h.is_stream_header:
                raise ValueError(f"blob {i} is a clip, not a stream header (commons.decompress reads those)")
            if tim is None:
                raise ValueError(f"stream header {i} carries no timbre")
        h0 = parsed[0][0]
        if any((h.n_q, h.bits, h.codebook_size, h.timbre_dim) != (h0.n_q, h0.bits, h0.codebook_size, h0.timbre_dim) for h, _, _ in parsed):
            raise ValueError("the stream headers disagree on (n_q, bits, codebook_size, timbre_dim)")
        self.n_q, self.bits, self.codebook_size, self.B = h0.n_q, h0.bits, h0.codebook_size, len(parsed)
        self.device = torch.device(device)
        self.timbre = ops.h2d(torch.from_numpy(np.stack([tim for _, tim, _ in parsed])), self.device)
        self.reader = bitstream.PacketReader(self.B, h0.Q, h0.bits)

    def feed(self, packets):
        import numpy as np
        k, payloads = self.reader.feed(packets)
        if k < 1:
            raise ValueError("a packet without frames")
        rows = np.stack([np.frombuffer(p, dtype=np.uint8) for p in payloads])
        return ops.unpack_codes(ops.h2d(torch.from_numpy(rows), self.device), self.n_q, k, bits=self.bits)


def dtx_row():
    """Host state of one receiver row under discontinuous transmission."""
    return dict(in_dtx=False, since=0, sid_k=0, phase=0)


def dtx_step(row, arrived, k, sid_timeout=24):
    """One tick of one row of the receiver's DTX state machine, host only.  arrived: "normal" (a valid packet is played), "sid"
    (a valid SID packet is played), "redundant" (the push is played from the redundant layer) or None (nothing playable).
    Advances `row` (dtx_row()) and -> (fac_sid_apply's mode word, comfort): comfort is True when the push is k comfort frames,
    i.e. played as PRIMARY from the stored SID codes; False with arrived None is today's concealment (a timed-out row has then
    left DTX)."""
    from . import _lib
    if arrived == "normal":
        row["in_dtx"] = False
        return _lib.SID_PASS, False
    if arrived == "sid":
        row.update(in_dtx=True, since=0, sid_k=int(k), phase=0)
        return _lib.SID_STORE | int(k) << 16, False
    if arrived == "redundant":
        return _lib.SID_PASS, False
    if row["in_dtx"] and row["since"] < sid_timeout:
        mode = _lib.SID_FILL | row["phase"] << 8 | row["sid_k"] << 16
        row["since"] += 1
        row["phase"] = (row["phase"] + int(k)) % row["sid_k"]
        return mode, True
    row["in_dtx"] = False
    return _lib.SID_PASS, False


class StreamingReceiver:
    """Receiver that keeps playing through packet loss: per tick one entry per stream, a packet or None, in; audio
    out.  Streams are judged one by one -- a caller's lost packet does not touch its neighbours.

        rx = StreamingReceiver(model, headers, delay=1)      # headers: CodePacketizer.header(timbre)
        wave = rx.prime(packets)                             # call set-up is reliable: every stream's packet, >= rx.min_prime frames
        wave = rx.tick(packets)                              # packets[b]: bytes or None -> (B, 1, 300 k)
        wave = rx.flush()                                    # delay=1: the push still held

    delay=0: a row whose packet arrived plays it (PRIMARY), any other row repeats its last frame (LOST).  delay=1: tick j plays
    push j - 1, from its own packet (kept as bytes for one tick) if that arrived, else from the redundant layer in packet j
    (REDUNDANT: the leading n_red quantizers, decoded at that lower rate), else LOST; the first tick after prime() returns None.
    Concealment is fac_plc_select's state machine: a lost row repeats its last frame for `hold` frames at its gain, fades to
    silence over `fade` frames and comes back within `recover` frames of the next good packet.  The defaults (25 ms, 75 ms, one
    frame) follow the order of magnitude of G.711 Appendix I; they were not tuned by listening.

    k, the frames of a tick, comes from any readable packet of the push being played (delay=1: or from the next packet's
    n_red_frames); when no stream has one, pass k= (ValueError otherwise).  Per tick: one host-to-device copy (status words and
    both payload rows in one buffer), ops.unpack_codes once (twice when a row is REDUNDANT), fac_plc_select, the LayeredDecoder
    hop (a graph replay), fac_plc_gain in place -- no device-to-host copy and no synchronisation; `stats` comes from the host's
    parsing: per stream received, corrupt, misordered (packets), recovered, concealed (frames).  `last_status` is the status
    list of the last tick.  With graphs the returned wave is a static buffer, valid until the next call.

    dtx=True: the receiving half of discontinuous transmission (the sender is CodePacketizer(dtx=...)).  A SID
    packet plays as it is and its k frames of codes are kept on the device; from then on a row for which nothing playable
    arrives is not concealed: it plays comfort frames -- those codes, cycled, through the unchanged decoder at gain 1 -- for up
    to sid_timeout pushes after the last SID packet (counted in stats[b]["comfort"], not in "concealed").  A normal packet ends
    that; a row that times out fades through the concealment above, so a dead link still goes silent.  One more small launch
    per tick (fac_sid_apply, between the unpack and fac_plc_select); its mode words ride in the same staging buffer: still one
    host-to-device copy.  sid_timeout = 24 pushes (three refreshes at the sender's default) was not tuned by listening."""

    def __init__(self, model, header_blobs, delay=0, hold=2, fade=6, recover=1, use_graphs=True, max_frames=16, device="cuda",
                 dtx=False, sid_timeout=24):
        from . import bitstream
        from . import _lib
        if delay not in (0, 1):
            raise ValueError(f"delay = {delay}: 0 (play at once) or 1 (wait one push for the redundant layer); no deeper reorder buffer")
        if hold < 0 or fade < 1 or recover < 1:
            raise ValueError(f"hold >= 0, fade >= 1, recover >= 1 (got {hold}, {fade}, {recover})")
        if not 1 <= max_frames <= _lib.PLC_MAX_FRAMES:
            raise ValueError(f"max_frames = {max_frames} (1 .. {_lib.PLC_MAX_FRAMES})")
        head = CodeDepacketizer(header_blobs, device=device)
        self.n_q, self.bits, self.B, self.device = tuple(head.n_q), head.bits, head.B, head.device
        self.delay, self.policy = delay, (int(hold), int(fade), int(recover))
        self.dtx, self.sid_timeout = bool(dtx), int(sid_timeout)
        if self.dtx and self.sid_timeout < 0:
            raise ValueError(f"sid_timeout = {sid_timeout} (>= 0 pushes)")
        self.reader = bitstream.LossyPacketReader(self.B, self.n_q, self.bits, dtx=self.dtx)
        self._dtx_rows = [dtx_row() for _ in range(self.B)] if self.dtx else None
        self._sid_codes = torch.zeros(self.B, sum(self.n_q), _lib.PLC_MAX_FRAMES, dtype=torch.int64, device=self.device) if self.dtx else None
        self.comfort = [0] * self.B
        self.dec = LayeredDecoder(model, head.timbre, use_graphs=use_graphs, max_frames=max_frames)
        self.min_prime, self.max_frames = self.dec.min_prime, int(max_frames)
        self.state = ops.PlcState(self.B, self.n_q, self.device)
        self.n_red = (0, 0, 0)
        self._red = None
        self._ramp = {}
        self._held = None
        self.recovered, self.concealed = [0] * self.B, [0] * self.B
        self.last_status = None

    @property
    def stats(self):
        rd = self.reader
        out = [dict(received=rd.received[b], recovered=self.recovered[b], concealed=self.concealed[b], corrupt=rd.corrupt[b],
                    misordered=rd.misordered[b]) for b in range(self.B)]
        if self.dtx:
            for b in range(self.B):
                out[b]["comfort"] = self.comfort[b]
        return out

    def prime(self, packets):
        if self.dec._n_q is not None:
            raise RuntimeError("prime() must be the first call")
        packets = list(packets)
        if len(packets) != self.B or any(p is None for p in packets):
            raise ValueError(f"prime() needs one packet per stream ({self.B}); call set-up is reliable")
        seq0 = self.reader.expected
        parsed = self.reader.feed(packets)
        if any(p is None for p in parsed):
            raise ValueError(f"prime(): the packets of streams {[b for b, p in enumerate(parsed) if p is None]} are corrupt or not seq {seq0}")
        k = parsed[0].n_frames
        if any(p.n_frames != k for p in parsed):
            raise ValueError(f"prime(): the streams' packets disagree on n_frames: {[p.n_frames for p in parsed]}")
        if k < self.min_prime:
            raise ValueError(f"prime() needs at least {self.min_prime} frames, got {k}")
        self.n_red = parsed[0].n_red
        if sum(self.n_red):
            self._red = [torch.zeros(self.B, max(n, 1), self.max_frames, dtype=torch.int64, device=self.device)[:, :n] for n in self.n_red]
        status = [0] * self.B
        mode = [dtx_step(self._dtx_rows[b], "sid" if p.sid else "normal", k, self.sid_timeout)[0] for b, p in enumerate(parsed)] \
            if self.dtx else None
        buf, n1, _ = self._stage(status, [p.payload for p in parsed], None, k, mode)
        wave = self.dec.prime(ops.unpack_codes(buf[1], self.n_q, k, bits=self.bits))
        dst, n_use = self.dec.buffers(k)
        if self.dtx:                                      # a stream that starts in silence: its first packet is a SID packet
            ops.sid_apply(dst, buf[2], self._sid_codes, self.n_q)
        ops.plc_select(dst, None, buf[0], self.state, dst, n_use, self._ramp_buf(k), (0, 0, 0), *self.policy)
        self.last_status = status
        return wave

    def _ramp_buf(self, k):
        if k not in self._ramp:
            self._ramp[k] = torch.empty(self.B, k + 1, dtype=torch.float32, device=self.device)
        return self._ramp[k]

    def _stage(self, status, prim, red, k, mode=None):
        """One host buffer [B status words | B rows of (primary payload | redundant payload)], one copy to the device ->
        ((status (B) int32, rows (B, n1 + n2) uint8) device views, n1, n2).  mode (dtx): B more words behind the status words,
        and a third view, mode (B) int32, in the result."""
        import numpy as np
        from . import bitstream
        n1 = bitstream.payload_bytes(k, sum(self.n_q), self.bits)
        n2 = bitstream.payload_bytes(k, sum(self.n_red), self.bits) if red is not None else 0
        nw = 4 * self.B * (1 if mode is None else 2)
        host = np.zeros(nw + self.B * (n1 + n2), dtype=np.uint8)
        host[:4 * self.B].view("<i4")[:] = status
        if mode is not None:
            host[4 * self.B:nw].view("<i4")[:] = mode
        rows = host[nw:].reshape(self.B, n1 + n2)
        for b in range(self.B):
            if prim[b] is not None:
                rows[b, :n1] = np.frombuffer(prim[b], dtype=np.uint8)
            if red is not None and red[b] is not None:
                rows[b, n1:] = np.frombuffer(red[b], dtype=np.uint8)
        dev = ops.h2d(torch.from_numpy(host), self.device)
        views = (dev[:4 * self.B].view(torch.int32), dev[nw:].view(self.B, n1 + n2))
        if mode is not None:
            views += (dev[4 * self.B:nw].view(torch.int32),)
        return views, n1, n2

    def _play(self, prim, red, k):
        """prim[b] / red[b]: the Packet a row is played from, or None.  A packet of another frame count than k is of no use."""
        from . import _lib
        status, p_rows, r_rows, mode = [], [], [], ([] if self.dtx else None)
        for b in range(self.B):
            p, r = prim[b], red[b] if red is not None else None
            arrived = None
            if p is not None and p.n_frames == k:
                st, arrived = _lib.PLC_PRIMARY, "sid" if p.sid else "normal"
            elif r is not None and r.n_red_frames == k and r.n_red == self.n_red and sum(self.n_red):
                st, arrived = _lib.PLC_REDUNDANT, "redundant"
            else:
                st = _lib.PLC_LOST
            comfort = False
            if self.dtx:
                word, comfort = dtx_step(self._dtx_rows[b], arrived, k, self.sid_timeout)
                mode.append(word)
            if comfort:                                       # the stored SID codes, cycled: played like a packet that arrived
                st = _lib.PLC_PRIMARY
                self.comfort[b] += k
            elif st == _lib.PLC_REDUNDANT:
                self.recovered[b] += k
            elif st == _lib.PLC_LOST:
                self.concealed[b] += k
            status.append(st)
            p_rows.append(p.payload if arrived in ("normal", "sid") else None)
            r_rows.append(r.red_payload if st == _lib.PLC_REDUNDANT else None)
        any_red = _lib.PLC_REDUNDANT in status
        staged, n1, n2 = self._stage(status, p_rows, r_rows if any_red else None, k, mode)
        st_dev, rows = staged[0], staged[1]
        dst, n_use = self.dec.buffers(k)
        ops.unpack_codes(rows[:, :n1] if n2 else rows, self.n_q, k, bits=self.bits, out=dst)
        if self.dtx:
            ops.sid_apply(dst, staged[2], self._sid_codes, self.n_q)
        red_codes = None
        if any_red:
            red_codes = [c[:, :, :k] for c in self._red]
            ops.unpack_codes(rows[:, n1:], self.n_red, k, bits=self.bits, out=red_codes)
        ramp = self._ramp_buf(k)
        ops.plc_select(dst, red_codes, st_dev, self.state, dst, n_use, ramp, self.n_red if any_red else (0, 0, 0), *self.policy)
        wave = self.dec.push_buffers(k)
        self.last_status = status
        return ops.plc_gain(wave, ramp, out=wave)

    def _frames(self, prim, red, k):
        n = next((p.n_frames for p in prim if p is not None), None)
        if n is None and red is not None:
            n = next((r.n_red_frames for r in red if r is not None and r.n_red_frames), None)
        if n is None:
            n = k
        if n is None:
            raise ValueError("no stream has a readable packet for this push: pass k=, the frames to conceal")
        if not 1 <= n <= self.max_frames:
            raise ValueError(f"a push of {n} frames (1 .. max_frames = {self.max_frames})")
        return int(n)

    def tick(self, packets, k=None):
        if self.dec._n_q is None:
            raise RuntimeError("call prime() first")
        rd = self.reader
        snap = (rd.expected, list(rd.received), list(rd.corrupt), list(rd.misordered))
        parsed = rd.feed(packets)
        if self.delay == 0:
            prim, red = parsed, None
        else:
            prim, red = self._held, parsed
            if prim is None:
                self._held = parsed
                return None                               # the first tick after prime(): push 1 is held, nothing is due yet
        try:
            k = self._frames(prim, red, k)
        except ValueError:                                # nothing was played: the tick did not happen
            rd.expected, rd.received, rd.corrupt, rd.misordered = snap
            raise
        if self.delay:
            self._held = parsed
        return self._play(prim, red, k)

    def flush(self, k=None):
        """delay=1: plays the push still held (its rows PRIMARY or LOST) -> wave, or None when nothing is held."""
        if self._held is None:
            return None
        held, self._held = self._held, None
        return self._play(held, None, self._frames(held, None, k))


# ------------------------------------------------------------------------------------ streams that join and leave
DRAIN_HOPS = 3       # ticks of silence a leaving stream is still run for: the 1 024 samples of look-ahead, in whole hops


class PoolFull(RuntimeError):
    """StreamPool.join(): every slot is taken by a live or a draining stream."""


def pool_preroll(n_consumed):
    """Output samples a stream joining after `n_consumed` session samples receives that lie before its own first input sample:
    the session has emitted (n - 1024) // 300 + 1 frames of its n samples, the next frame it emits starts there."""
    return n_consumed - FRAME * ((n_consumed - LOOKAHEAD) // FRAME + 1)


class SlotBook:
    """The host-side book-keeping of a StreamPool, no device in sight: which stream holds which slot, who is draining, who
    missed a tick.  Slot 0 is the donor and is never handed out; ids count up from 0 and are never reused."""

    def __init__(self, slots):
        slots = int(slots)
        if slots < 1:
            raise ValueError(f"slots = {slots}: a pool has at least one slot")
        self.slots = slots
        self.free = list(range(1, slots + 1))
        self.slot = {}           # id -> slot, live and draining streams
        self.live = []           # ids in join order
        self.draining = {}       # id -> ticks left, in leave order
        self.underruns = {}      # id -> ticks a live stream was not fed
        self._next = 0

    def join(self):
        if not self.free:
            raise PoolFull(f"all {self.slots} slots are taken ({len(self.live)} live, {len(self.draining)} draining)")
        b = min(self.free)
        self.free.remove(b)
        sid, self._next = self._next, self._next + 1
        self.slot[sid] = b
        self.live.append(sid)
        self.underruns[sid] = 0
        return sid, b

    def leave(self, sid):
        if sid not in self.live:
            raise ValueError(f"stream {sid!r} is {'already leaving' if sid in self.draining else 'unknown'}")
        self.live.remove(sid)
        self.draining[sid] = DRAIN_HOPS

    def check(self, sids):
        seen = set()
        for s in sids:
            if s in self.draining:
                raise ValueError(f"stream {s!r} has left and is draining: it takes no more audio")
            if s not in self.slot:
                raise ValueError(f"unknown stream {s!r}")
            if s in seen:
                raise ValueError(f"stream {s!r} named twice")
            seen.add(s)

    def tick(self, sids):
        """One tick fed the streams `sids` (in that order) -> (out, scatter, last): the ids whose outputs the tick returns -- the
        fed streams, the live ones that were not fed, the draining ones --, for every slot 0 .. slots the index into `sids` of
        the stream to feed it or -1 (silence), and {id: True on a draining stream's last tick}.  Slots of streams that drained
        out are free on return; their ids stay valid in `out` for this tick only (`slot_of` = their slots)."""
        sids = list(sids)
        self.check(sids)
        fed = set(sids)
        missed = [s for s in self.live if s not in fed]
        for s in missed:
            self.underruns[s] += 1
        out = sids + missed + list(self.draining)
        scatter = [-1] * (self.slots + 1)
        for i, s in enumerate(sids):
            scatter[self.slot[s]] = i
        self.slot_of = [self.slot[s] for s in out]
        last = {s: False for s in out}
        for s in list(self.draining):
            self.draining[s] -= 1
            if self.draining[s] == 0:
                last[s] = True
                del self.draining[s]
                self.free.append(self.slot.pop(s))
        return out, scatter, last


class StreamPool:
    """A running streaming session whose streams join and leave one by one:

        pool = StreamPool(model, slots=16, n_c=2)                                    # codec pool
        pool = StreamPool(codec, slots=16, redecoder=red, use_p_code=False, n_c=1)   # conversion pool
        sid = pool.join(timbre)                  # (1024,) fp32 on the device: source timbre (codec) / target voice (converter)
        out = pool.tick(sids, hops)              # sids: ids in any order; hops (len(sids), 480) fp32 on the device
        pool.set_timbre(sid, timbre)
        pool.leave(sid)

    One StreamingCodec / StreamingConverter over B = slots + 1 streams runs every tick, whoever is there: the hop is launch
    bound, so a tick costs what a lockstep hop of B streams costs plus three small launches.  Slot 0 is the donor: it hears
    silence under the all-zero timbre for ever, so its rows of the session's state tensors (left-context buffers, LSTM states;
    _HopSession._slot_state) are at every tick those of a stream that has been silent since the session began.  join() copies
    them into the lowest free slot (fac_slot_copy on the current stream, before the next tick; joins before one tick share a
    launch) and writes the slot's style row (converter: cond row).  From that tick on the stream is, bit for bit, its row of a
    lockstep session of the same B that heard silence and then the stream.

    tick() scatters the hops into the session's input (fac_rows_pick; donor, idle, draining and unfed slots get zeros), pushes,
    and gathers the rows of the live and draining streams into pool-owned buffers, valid until the next tick ->
        dict(sids=[fed streams in the order given, live streams that were not fed, draining streams],
             codes=[p, c, r] ((n, n_q, k) int64; a converter pool: [p, c]), wave=(n, 1, 300 k), rows in the order of sids,
             frame0={sid: frames the stream had received before this tick}, preroll={sid: ...}, last={sid: bool})
    A live stream missing from `sids` hears silence for that tick and pool.underruns[sid] counts it.  A stream's first
    preroll(sid) output samples lie before its own first input sample (900 / 780 / 960 / 840 / 1020 by the phase of the join
    in the session's 5-hop period): the codec's look-ahead plus the offset of the stream's start on the POOL's 300-sample
    frame grid.  leave() feeds the stream DRAIN_HOPS more ticks of silence, which emits the frame that holds its last sample
    for every alignment; its outputs keep coming, the last with last[sid] = True, then the slot is free.  No finish() and no
    reflect padding of a stream's end.

    Limits: until its join a stream's left context is silence under the null timbre; the frame grid is the pool's; kernel routes
    depend on B as everywhere, so outputs equal a B-row lockstep session bit for bit and a one-stream session up to near ties.
    Everything runs on the stream that is current at the call; the device maps are uploaded again (ops.h2d) only when the
    membership or the order of `sids` changes."""

    def __init__(self, model, slots=16, n_c=None, use_graphs=True, redecoder=None, use_p_code=False, device="cuda"):
        self.book = SlotBook(slots)
        self.slots, self.B = self.book.slots, self.book.slots + 1
        self.device = torch.device(device)
        q = model.quantizer
        self._dim = q.in_dim
        zero = torch.zeros(self.B, q.in_dim, device=self.device)
        if redecoder is None:
            self.session = StreamingCodec(model, zero, n_c=2 if n_c is None else n_c, use_graphs=use_graphs)
        else:
            self.session = StreamingConverter(model, redecoder, zero, use_p_code=use_p_code, n_c=1 if n_c is None else n_c,
                                              use_graphs=use_graphs)
        self.converter = redecoder is not None
        self._q = q
        sess = self.session
        self._in = sess._hop_in                                   # the session's own static input: push() then copies nothing
        with torch.no_grad():
            sess.prime(torch.zeros(self.B, 1, sess.prime_samples, device=self.device))
            for _ in range(10):                                   # both periods: every phase's graph captured, every edge in
                self._in.zero_()                                  # its steady-state layout
                o = sess.push(self._in)
        self._n_q = [c.shape[1] for c in o["codes"]]              # quantizers per code tensor: [1, n_c, 3] / [1, n_c]
        self.table = ops.SlotTable(self.B)
        for kind, t in sess._slot_state():
            (self.table.add_edge if kind == "edge" else self.table.add_lstm_state)(t)
        self.table.freeze()
        self._pending = []                                        # slots joined since the last tick
        self._preroll, self._frames = {}, {}
        self._key, self._maps = None, None
        self._wave, self._codes = {}, {}
        self.ticks = 0

    # ------------------------------------------------------------------------------------------ membership
    @property
    def underruns(self):
        return self.book.underruns

    @property
    def live(self):
        return list(self.book.live)

    def preroll(self, sid):
        return self._preroll[sid]

    def _row(self, timbre):
        if not isinstance(timbre, torch.Tensor) or timbre.numel() != self._dim or timbre.dim() > 2:
            got = tuple(timbre.shape) if isinstance(timbre, torch.Tensor) else type(timbre).__name__
            raise ValueError(f"timbre must be a float32 GPU tensor ({self._dim},), got {got}")
        timbre = timbre.reshape(1, self._dim)
        _check_timbre(timbre, 1, self._dim, "timbre")
        with torch.no_grad():
            if self.converter:
                return self.session.red.r.encoder.cond_layer.run(timbre.contiguous().reshape(1, -1, 1)).reshape(-1)
            return self._q.timbre_linear(timbre.contiguous()).reshape(-1)

    def _write_row(self, slot, row):
        (self.session.red.cond if self.converter else self.session.qs.style)[slot].copy_(row)

    def join(self, timbre):
        row = self._row(timbre)                                   # refuses before a slot is taken
        sid, slot = self.book.join()
        self._pending.append(slot)
        self._write_row(slot, row)
        self._preroll[sid] = pool_preroll(self.session.n_samples)
        self._frames[sid] = 0
        return sid

    def set_timbre(self, sid, timbre):
        """Codec pool: the stream's style row; conversion pool: its cond row (StreamingConverter.set_target for one row).  Between
        ticks; the next tick already uses it.  Left contexts are not reset."""
        if sid not in self.book.live:
            raise ValueError(f"stream {sid!r} is not live")
        self._write_row(self.book.slot[sid], self._row(timbre))

    def leave(self, sid):
        self.book.leave(sid)

    # ------------------------------------------------------------------------------------------ the tick
    def _out_buffers(self, codes, k):
        if k not in self._wave:
            self._wave[k] = torch.zeros(self.slots, 1, FRAME * k, device=self.device)
            self._codes[k] = [torch.zeros(self.slots, c.shape[1], k, device=self.device, dtype=torch.int64) for c in codes]
        return self._wave[k], self._codes[k]

    def tick(self, sids, hops=None):
        sids = list(sids)
        self.book.check(sids)
        n_in = len(sids)
        if n_in or hops is not None:
            if not isinstance(hops, torch.Tensor) or tuple(hops.shape) != (n_in, HOP):
                got = tuple(hops.shape) if isinstance(hops, torch.Tensor) else type(hops).__name__
                raise ValueError(f"hops must be ({n_in}, {HOP}) float32 on {self.device}, got {got}")
            if hops.dtype != torch.float32 or hops.device.type != self.device.type or not hops.is_cuda:
                raise ValueError(f"hops must be float32 on {self.device}, got {hops.dtype} on {hops.device}")
            if hops.stride(-1) != 1:
                hops = hops.contiguous()
        out_sids, scatter, last = self.book.tick(sids)
        slot_of = self.book.slot_of
        n_out = len(out_sids)
        if self._pending:
            self.table.copy(0, self._pending)
            self._pending = []
        key = (tuple(scatter), tuple(slot_of))
        if key != self._key:
            inners = sorted({1} | set(self._n_q))
            flat, spans = list(scatter), {}
            for q in inners:
                spans[q] = (len(flat), len(flat) + n_out * q)
                flat += [b * q + i for b in slot_of for i in range(q)]
            dev = ops.h2d(torch.tensor(flat, dtype=torch.int32), self.device)
            self._key, self._maps = key, (dev, spans)
        dev, spans = self._maps
        if n_in:
            ops.rows_pick(hops, dev[:self.B], out=self._in)
        else:
            self._in.zero_()
        with torch.no_grad():
            o = self.session.push(self._in)
        codes_s, wave_s = o["codes"], o["wave"]
        k = codes_s[0].shape[-1]
        wave, codes = self._out_buffers(codes_s, k)
        if n_out:
            ops.rows_pick(wave_s, dev[spans[1][0]:spans[1][1]], out=wave[:n_out])
            for c_s, c in zip(codes_s, codes):
                a, b = spans[c_s.shape[1]]
                ops.rows_pick(c_s, dev[a:b], out=c[:n_out])
        frame0 = {s: self._frames[s] for s in out_sids}
        for s in out_sids:
            self._frames[s] += k
        res = dict(sids=out_sids, codes=[c[:n_out] for c in codes], wave=wave[:n_out], frame0=frame0,
                   preroll={s: self._preroll[s] for s in out_sids}, last=last)
        for s, done in last.items():
            if done:
                del self._frames[s], self._preroll[s]
        self.ticks += 1
        return res
