"""Decoding from FA codes: fac_vq_decode (codes -> per-RVQ sums -> timbre-normed decoder input), VectorQuantize.decode_code,
ResidualVectorQuantize.from_codes, FAquantizer.from_codes, commons.decode_codes (timbre swap included) and the streaming
receiver StreamingDecoder.

References: an fp64 restatement of dac/nn/quantize.py:200-220 (from_codes) + modules/quantize.py:436-449 (LayerNorm over
channels, * gamma + beta) below, pinned on the CPU to tests/golden/decode_from_codes.npz (made by make_golden_decode.py from
the real reference); the model's own forward (round trip) and the offline decode (streaming)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from facodec_amd import _lib, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E2E_TOL = 1e-4


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def ref_decode(codes, weights, style):
    """fp64 CPU restatement.  codes: 3 int64 (B, n_r, T) or None; weights: per RVQ list of (codebook, weight_v (D,8,1),
    weight_g (D,1,1) or None (no norm), bias); style (B, 2D).  -> (outs, [z_p, z_c, z_r])."""
    B, D2 = style.shape
    D = D2 // 2
    T = next(c.shape[-1] for c in codes if c is not None)
    zs = []
    for c, ws in zip(codes, weights):
        z = torch.zeros(B, D, T, dtype=torch.float64)
        for i, (cb, v, g, b) in enumerate(ws):
            rows = cb.double().cpu()[c[:, i].cpu().clamp(0, cb.shape[0] - 1)]           # (B, T, 8)  decode_code
            w = v.double().cpu().reshape(D, 8)
            if g is not None:
                w = w * (g.double().cpu().reshape(D, 1) / w.norm(dim=1, keepdim=True))  # weight norm
            z = z + torch.einsum("dk,btk->bdt", w, rows) + b.double().cpu()[None, :, None]
        zs.append(z)
    x = (zs[0] + zs[1]) + zs[2]
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    st = style.double().cpu()
    outs = (x - mean) / torch.sqrt(var + 1e-5) * st[:, :D, None] + st[:, D:, None]
    return outs, zs


def _quantizer_cpu():
    from facodec_amd.quantize import FAquantizer
    q = FAquantizer(in_dim=1024, n_p_codebooks=1, n_c_codebooks=2, n_t_codebooks=2, n_r_codebooks=3, codebook_size=1024,
                    codebook_dim=8, quantizer_dropout=0.5, causal=True, separate_prosody_encoder=True, timbre_norm=True)
    synth.load_synthetic(q, seed=0, prefix="quantizer.")
    return q.eval()


def _module_weights(q):
    return [[(vq.codebook.weight.detach(), vq.out_proj.weight_v.detach(), vq.out_proj.weight_g.detach(), vq.out_proj.bias.detach())
             for vq in rvq.quantizers] for rvq in (q.prosody_quantizer, q.content_quantizer, q.residual_quantizer)]


def _golden_codes(golden_dir):
    d = np.load(os.path.join(golden_dir, "codec_e2e.npz"))
    return [torch.from_numpy(d[n].astype(np.int64)) for n in ("codes_p", "codes_c", "codes_r")], torch.from_numpy(d["timbre"])


# ------------------------------------------------------------------------------------------------ CPU
def test_fp64_restatement_matches_reference_golden(golden_dir):
    """The test's own fp64 restatement reproduces the real reference's from_codes + forward_v2 tail on the fixture codes, for the
    clips' own timbre and the swapped one."""
    g = np.load(os.path.join(golden_dir, "decode_from_codes.npz"))
    q = _quantizer_cpu()
    codes, timbre = _golden_codes(golden_dir)
    W = _module_weights(q)
    lin_w, lin_b = q.timbre_linear.weight.detach().double(), q.timbre_linear.bias.detach().double()
    for tag, tim in (("own", timbre), ("swap", timbre.flip(0))):
        style = tim.double() @ lin_w.t() + lin_b
        outs, zs = ref_decode(codes, W, style)
        assert rel(outs[:, ::8], g[f"outs_probe_{tag}"]) < 1e-5, tag
    for nm, z in zip("pcr", zs):
        assert rel(z[:, ::16], g[f"zq_{nm}_probe"]) < 1e-5, nm
    assert rel(outs[:, ::8], g["outs_probe_own"]) > 1e-2           # swapping the timbre changes the decoder input


def test_vq_decode_desc_layout_matches_header(tmp_path):
    """The ctypes mirror of fac_vq_decode_desc has the size / field offsets gcc gives the header's struct."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    fields = ("codes", "codes_bs", "codes_qs", "n_q", "codebook", "w_out", "w_out_scale", "b_out", "style", "outs", "z", "B", "Kc")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "facodec_hip.h"\nint main(){printf("%zu %d'
                   + " %zu" * len(fields) + '\\n", sizeof(fac_vq_decode_desc), FAC_VQ_DECODE_MAX_Q'
                   + "".join(f", offsetof(fac_vq_decode_desc, {f})" for f in fields) + ");return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    D = _lib.VqDecodeDesc
    assert out == [ctypes.sizeof(D), _lib.VQ_DECODE_MAX_Q] + [getattr(D, f).offset for f in fields]


def test_vq_decode_rejects_bad_descriptors_without_gpu():
    lib = _lib.load()
    d = _lib.VqDecodeDesc()
    assert lib.fac_vq_decode(ctypes.byref(d), None) == -1 and b"null pointer" in lib.fac_last_error()
    fake = ctypes.c_void_p(0x10000)                    # never dereferenced: every check below fails on the host
    d.style, d.outs = fake, fake
    d.B, d.D, d.T, d.Kc = 1, 1024, 4, 1024
    d.n_q[0] = 2
    assert lib.fac_vq_decode(ctypes.byref(d), None) == -1 and b"no codes" in lib.fac_last_error()
    d.codes[0], d.codes[1], d.codes[2] = fake, fake, fake
    d.n_q[1], d.n_q[2] = 10, 5
    assert lib.fac_vq_decode(ctypes.byref(d), None) == -1 and b"at most 16" in lib.fac_last_error()
    d.n_q[1], d.n_q[2] = 0, 0
    assert lib.fac_vq_decode(ctypes.byref(d), None) == -1 and b"null weight" in lib.fac_last_error()


def test_from_codes_refuses_cpu_tensors(golden_dir):
    q = _quantizer_cpu()
    codes, timbre = _golden_codes(golden_dir)
    with pytest.raises(_lib.FacodecHipError):
        q.from_codes(codes, timbre)


# ------------------------------------------------------------------------------------------------ GPU
def _rand_weights(n_q, D, Kc, gen, dev, no_scale=False):
    from facodec_amd import ops
    ws, refs = [], []
    for n in n_q:
        w_r, ref_r = [], []
        for _ in range(n):
            cb = torch.randn(Kc, 8, generator=gen)
            v = torch.randn(D, 8, 1, generator=gen) * 0.3
            g = torch.rand(D, 1, 1, generator=gen) + 0.5
            b = torch.randn(D, generator=gen) * 0.1
            vd = v.to(dev)
            sc = None if no_scale else ops.wn_scale(vd, g.to(dev))
            w_r.append((cb.to(dev), vd, sc, b.to(dev)))
            ref_r.append((cb, v, None if no_scale else g, b))
        ws.append(w_r)
        refs.append(ref_r)
    return ws, refs


def _strided_codes(n_q, B, T, Kc, gen, dev):
    """Codes as slices of larger (B, n + 2, T + 3) tensors: batch stride and row stride differ from a dense (B, n, T)."""
    out = []
    for n in n_q:
        if n == 0:
            out.append(None)
            continue
        big = torch.randint(0, Kc, (B, n + 2, T + 3), generator=gen)
        out.append(big.to(dev)[:, 1:1 + n, 2:2 + T])
    return out


def _check_kernel(B, T, n_q, cuda, D=1024, Kc=1024, seed=0, no_scale=False):
    from facodec_amd import ops
    gen = torch.Generator().manual_seed(seed)
    ws, refs = _rand_weights(n_q, D, Kc, gen, cuda, no_scale)
    codes = _strided_codes(n_q, B, T, Kc, gen, cuda)
    style = torch.cat([torch.rand(B, D, generator=gen) + 0.5, torch.randn(B, D, generator=gen) * 0.2], 1)
    z = [torch.full((B, D, T), float("nan"), device=cuda) for _ in range(3)]
    outs = ops.vq_decode(codes, ws, style.to(cuda), Kc, z_out=z)
    o_ref, z_ref = ref_decode(codes, refs, style)
    for r in range(3):
        assert rel(z[r], z_ref[r]) <= 1e-6 if n_q[r] else torch.equal(z[r].cpu(), torch.zeros(B, D, T)), (r, n_q)
    assert rel(outs, o_ref) <= 2e-6, n_q
    return outs


BT = [(b, t) for b in (1, 3, 32) for t in (1, 2, 7, 160, 1000) if (b, t) != (32, 1000)] + [(8, 1000)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", BT)
def test_vq_decode_kernel_vs_fp64(B, T, cuda):
    """Shipped quantizer counts (1 prosody, 2 content, 3 residual) on every (B, T) of the sweep, strided code slices."""
    _check_kernel(B, T, (1, 2, 3), cuda, seed=B * 1000 + T)


@pytest.mark.gpu
@pytest.mark.parametrize("n_q", [(1, 1, 0), (0, 3, 1), (2, 0, 0), (3, 3, 3), (0, 0, 1), (1, 2, 0), (3, 1, 2)])
@pytest.mark.parametrize("B,T", [(3, 7), (2, 160), (1, 1)])
def test_vq_decode_kernel_quantizer_counts(n_q, B, T, cuda):
    """0 - 3 quantizers per RVQ (n_c = 1, no residual, no prosody, ...)."""
    _check_kernel(B, T, n_q, cuda, seed=sum(n_q) * 7 + T)


@pytest.mark.gpu
def test_vq_decode_kernel_unnormed_and_small_codebook(cuda):
    """w_out_scale NULL (== 1), a codebook size that is no power of two, fewer channels."""
    _check_kernel(2, 37, (1, 2, 3), cuda, D=96, Kc=37, no_scale=True)


@pytest.mark.gpu
def test_vq_decode_null_outputs_are_not_written(cuda):
    """Only the requested outputs are written: outs and z_c live in one canary buffer with gaps (and the slot where z_p
    would go); everything else keeps its canary bits."""
    from facodec_amd import ops
    B, T, D, Kc = 3, 23, 1024, 1024
    gen = torch.Generator().manual_seed(3)
    ws, refs = _rand_weights((1, 2, 3), D, Kc, gen, cuda)
    codes = _strided_codes((1, 2, 3), B, T, Kc, gen, cuda)
    style = torch.cat([torch.ones(B, D), torch.zeros(B, D)], 1).to(cuda)
    n = B * D * T
    canary = torch.full((5 * n,), 12345.0, device=cuda)
    outs, z_c = canary[n:2 * n].view(B, D, T), canary[3 * n:4 * n].view(B, D, T)
    ops.vq_decode(codes, ws, style, Kc, out=outs, z_out=(None, z_c, None))
    c = canary.cpu()
    for lo in (0, 2 * n, 4 * n):
        assert bool((c[lo:lo + n] == 12345.0).all()), lo
    o_ref, z_ref = ref_decode(codes, refs, style.cpu())
    assert rel(outs, o_ref) <= 2e-6 and rel(z_c, z_ref[1]) <= 1e-6


@pytest.mark.gpu
def test_vq_decode_clamps_out_of_range_codes(cuda):
    """The kernel itself does not range check: an index outside [0, Kc) decodes as the clamped index (and stays inside the
    codebook).  The Python surface refuses such codes (next test)."""
    from facodec_amd import ops
    B, T, D, Kc = 2, 5, 1024, 1024
    gen = torch.Generator().manual_seed(4)
    ws, refs = _rand_weights((1, 1, 0), D, Kc, gen, cuda)
    codes = [torch.tensor([[[0, 5000, -7, 1023, 1024]], [[1, 2, 3, -1, 99999]]], dtype=torch.int64, device=cuda)] * 2 + [None]
    style = torch.cat([torch.ones(B, D), torch.zeros(B, D)], 1).to(cuda)
    z = [torch.empty(B, D, T, device=cuda) for _ in range(3)]
    outs = ops.vq_decode(codes, ws, style, Kc, z_out=z)
    o_ref, z_ref = ref_decode(codes, refs, style.cpu())
    assert rel(z[0], z_ref[0]) <= 1e-6 and rel(outs, o_ref) <= 2e-6


@pytest.fixture(scope="module")
def full_model(cuda):
    from facodec_amd.commons import build_model, default_model_params
    model = build_model(default_model_params())
    for k in ("encoder", "quantizer", "decoder"):
        synth.load_synthetic(model[k], seed=0, prefix=k + ".")
        model[k].eval().to(cuda)
    return model


@pytest.mark.gpu
def test_from_codes_validates_inputs(full_model, cuda):
    q = full_model.quantizer
    codes = [torch.zeros(2, n, 9, dtype=torch.int64, device=cuda) for n in (1, 2, 3)]
    timbre = torch.zeros(2, 1024, device=cuda)
    q.from_codes(codes, timbre)
    for bad in (1024, -1):
        c = [x.clone() for x in codes]
        c[2][1, 2, 4] = bad
        with pytest.raises(ValueError, match="outside"):
            q.from_codes(c, timbre)
    with pytest.raises(ValueError):
        q.from_codes([codes[0], codes[1], codes[2][:, :, :5]], timbre)            # T disagrees
    with pytest.raises(ValueError):
        q.from_codes([codes[0], codes[1], codes[2][:1]], timbre)                  # B disagrees
    with pytest.raises(ValueError):
        q.from_codes(codes, timbre[:, :512])
    with pytest.raises(ValueError):
        q.from_codes([codes[0], torch.zeros(2, 3, 9, dtype=torch.int64, device=cuda), codes[2]], timbre)   # 3 content rows
    with pytest.raises(TypeError):
        q.from_codes([codes[0].int(), codes[1], codes[2]], timbre)
    with pytest.raises(_lib.FacodecHipError):
        q.from_codes([c.cpu() for c in codes], timbre)
    with pytest.raises(ValueError, match="outside"):
        q.content_quantizer.quantizers[0].decode_code(torch.full((1, 3), 4096, dtype=torch.int64, device=cuda))


@pytest.mark.gpu
def test_from_codes_and_decode_vs_reference_golden(full_model, cuda, golden_dir):
    """The real reference's from_codes + forward_v2 tail + decoder (decode_from_codes.npz) on the codec_e2e codes, with the clips'
    own timbre and with the timbre rows swapped (zero-shot voice conversion)."""
    from facodec_amd.commons import decode_codes
    g = np.load(os.path.join(golden_dir, "decode_from_codes.npz"))
    m = full_model
    codes, timbre = _golden_codes(golden_dir)
    codes, timbre = [c.to(cuda) for c in codes], timbre.to(cuda)
    probe_t = torch.from_numpy(g["probe_t"])
    for tag, tim in (("own", timbre), ("swap", timbre.flip(0).contiguous())):
        outs, zs = m.quantizer.from_codes(codes, tim)
        assert outs.shape == (2, 1024, 160)
        assert rel(outs[:, ::8], g[f"outs_probe_{tag}"]) < E2E_TOL, tag
        for nm, z in zip("pcr", zs):
            assert rel(z[:, ::16], g[f"zq_{nm}_probe"]) < E2E_TOL, (tag, nm)
        y = decode_codes(m, codes, tim)
        assert y.shape == (2, 1, 48000)
        assert rel(y[:, 0, probe_t], g[f"wave_probe_{tag}"]) < E2E_TOL, tag
        assert abs(float(y.abs().max()) - float(g[f"wave_absmax_{tag}"])) < 1e-4
        assert torch.equal(y, m.decoder(outs))
    for nm, rvq, c in zip("pcr", (m.quantizer.prosody_quantizer, m.quantizer.content_quantizer, m.quantizer.residual_quantizer),
                          codes):
        z_q, z_lat, c_out = rvq.from_codes(c)
        assert c_out is c
        assert rel(z_q[:, ::16], g[f"zq_{nm}_probe"]) < E2E_TOL, nm
        assert torch.equal(z_lat[:, ::2].cpu(), torch.from_numpy(g[f"zp_{nm}_probe"])), nm     # raw codebook rows: exact
        assert torch.equal(z_lat[:, :8], rvq.quantizers[0].decode_code(c[:, 0]))


@pytest.mark.gpu
@pytest.mark.parametrize("n_c", [2, 1])
def test_round_trip_encode_then_from_codes(full_model, cuda, n_c):
    """encode -> codes -> from_codes == forward's decoder input up to its straight-through term; the decoded wave == the
    decoder on forward's outs.  (Codes re-encoded from the decoded wave are not asserted.)"""
    from facodec_amd.commons import decode_codes
    m = full_model
    wave = synth.synth_clips(3, 24000, seed=21).to(cuda)
    with torch.no_grad():
        z = m.encoder(wave)
        outs_f, quantized, _, _, timbre, codes = m.quantizer(z, wave, n_c=n_c, return_codes=True)
        y_f = m.decoder(outs_f)
    assert codes[1].shape[1] == n_c
    outs, zs = m.quantizer.from_codes(codes, timbre)
    assert rel(outs, outs_f) <= 1e-5
    for a, b in zip(zs, quantized):
        assert rel(a, b) <= 1e-5
    assert rel(decode_codes(m, codes, timbre), y_f) <= 1e-4
    assert torch.equal(m.quantizer.decode_input(codes, timbre), outs)


def _sender_chunks(m, wave, timbre, n_hops):
    from facodec_amd.streaming import HOP, StreamingCodec
    sess = StreamingCodec(m, timbre, n_c=2, use_graphs=True)
    chunks = [sess.prime(wave[:, :, :4800])]
    for h in range(n_hops):
        o = sess.push(wave[:, :, 4800 + h * HOP: 4800 + (h + 1) * HOP])
        chunks.append({k: ([c.clone() for c in v] if isinstance(v, list) else (v.clone() if torch.is_tensor(v) else v))
                       for k, v in o.items()})
    chunks.append(sess.finish())
    return [c for c in chunks if c["codes"] is not None]


def _receive(m, timbre, chunks, use_graphs):
    from facodec_amd.streaming import StreamingDecoder
    rx = StreamingDecoder(m, timbre, use_graphs=use_graphs)
    waves = [rx.prime(chunks[0]["codes"]).clone()]
    for c in chunks[1:]:
        w = rx.push(c["codes"])
        assert w.shape == (timbre.shape[0], 1, 300 * c["codes"][0].shape[-1])
        waves.append(w.clone())
    return torch.cat(waves, -1), rx


@pytest.mark.gpu
def test_streaming_decoder_matches_offline_and_sender(full_model, cuda):
    """The codes a StreamingCodec session emits, fed to StreamingDecoder in exactly the emitted chunks over five 5-hop periods:
    the concatenated wave matches the offline decode_codes of all codes and the sender's own wave; graphs on and off give the
    same samples bit for bit."""
    from facodec_amd.commons import decode_codes
    from facodec_amd.streaming import HOP
    m = full_model
    n_hops = 25
    wave = synth.synth_clips(2, 4800 + n_hops * HOP, seed=11).to(cuda)
    with torch.no_grad():
        _, _, _, _, timbre, _ = m.quantizer(m.encoder(wave), wave, n_c=2, return_codes=True)
    chunks = _sender_chunks(m, wave, timbre, n_hops)
    all_codes = [torch.cat([c["codes"][i] for c in chunks], -1) for i in range(3)]
    sent = torch.cat([c["wave"] for c in chunks], -1)
    assert all_codes[0].shape[-1] == wave.shape[-1] // 300
    got_g, rx = _receive(m, timbre, chunks, use_graphs=True)
    assert len(rx._graphs) >= 2                              # the steady-state pairs were captured (and replayed)
    got_e, _ = _receive(m, timbre, chunks, use_graphs=False)
    assert torch.equal(got_g, got_e)
    off = decode_codes(m, all_codes, timbre)
    assert got_g.shape == off.shape
    assert rel(got_g, off) <= E2E_TOL
    assert rel(got_g, sent) <= E2E_TOL


@pytest.mark.gpu
def test_streaming_decoder_prime_minimum(full_model, cuda):
    from facodec_amd.streaming import StreamingDecoder
    m = full_model
    timbre = torch.randn(1, 1024, device=cuda)
    rx = StreamingDecoder(m, timbre)
    assert rx.min_prime == 10                 # k7 / dilation 9 conv at 6 columns per frame: 54 // 6 + 1
    codes = [torch.zeros(1, n, rx.min_prime - 1, dtype=torch.int64, device=cuda) for n in (1, 2, 3)]
    with pytest.raises(ValueError, match="at least"):
        rx.prime(codes)
    with pytest.raises(RuntimeError):
        rx.push([c[:, :, :1] for c in codes])
    w = rx.prime([torch.zeros(1, n, rx.min_prime, dtype=torch.int64, device=cuda) for n in (1, 2, 3)])
    assert w.shape == (1, 1, 300 * rx.min_prime)
    with pytest.raises(ValueError):
        rx.push([torch.zeros(1, n, 1, dtype=torch.int64, device=cuda) for n in (1, 1, 3)])   # row counts changed
