"""Host side of the P8-fragment form of the split GEMM (conv1d_gemm_split_p8.hip), no GPU: the tile-width cost model
(fac_gsplit_p8_tile_cols), which form fac_conv1d_variant names for the nine P8 launches of a bench step and for fp32-input
descriptors, and that fac_conv_desc.gsplit_p8_cols = -1 (ops.GSPLIT_P8_COLS) restores the 128 x 128 form everywhere."""
import ctypes

import pytest

from facodec_amd import _lib, ops

OLD = "conv1d_gemm_split_kernel<%d> 128x128 (bf16x3 split GEMM, fp32-grade)"
NEW = "conv1d_gemm_split_kernel<%d> 64x%d (bf16x3 split GEMM, fp32-grade, P8 fragments)"


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _operands(d, p8):
    """Non-null pointers (never dereferenced: fac_conv1d_variant reads the descriptor only); p8: the input as P8 planes."""
    fake = ctypes.c_void_p(0x10000)
    d.y = d.ws = d.w = d.w_split = fake
    d.ws_bytes = ops.CONV_WS_BYTES
    if p8:
        d.x, d.x_p8, d.x_p8_plane_bytes = None, fake, (d.B * (d.C_in // 8) * d.T_in + 1) * 16
    else:
        d.x = fake
    return d


# the nine launches of a B = 32 x 2 s forward step whose input ops.p8_prepass turns into planes: (builder, K of the kernel, form)
def _bench_shapes():
    tr = lambda B, ci, T, co, s: ops.convtr_desc(B, ci, T, co, s, ops.convtr_rows_pad(co, s), split=True)       # noqa: E731
    k1 = lambda ci, co, n: ops.conv_desc(1, ci, n, co, 1, pad_left=0, pad_mode=ops.PAD_ZERO, t_out=n)            # noqa: E731
    return [
        ("convtr 1536->768 s6 flattened", lambda: tr(1, 1536, 5152, 768, 6), 2, None),       # measured slower on the new form
        ("convtr 768->384 s5", lambda: tr(32, 768, 960, 384, 5), 2, 256),
        ("convtr 384->192 s5", lambda: tr(32, 384, 4800, 192, 5), 2, 256),
        ("lstm 1024->4096 a", lambda: k1(1024, 4096, 5120), 1, 128),
        ("lstm 1024->4096 b", lambda: k1(1024, 4096, 5120), 1, 128),
        ("lstm 1536->6144 a", lambda: k1(1536, 6144, 5120), 1, 256),
        ("lstm 1536->6144 b", lambda: k1(1536, 6144, 5120), 1, 256),
        ("strided 256->512 k10 s5", lambda: ops.conv_desc(32, 256, 4800, 512, 10, stride=5), 2, None),   # measured slower
        ("strided 512->1024 k12 s6 flattened",
         lambda: ops.conv_desc(1, 512, 30912, 1024, 12, stride=6, pad_left=0, pad_mode=ops.PAD_ZERO, t_out=5151), 2, None),
    ]


def test_tile_width_cost_model(lib):
    """Rounds of `slots` workgroups x columns per tile, ties to the wide tile."""
    f = lib.fac_gsplit_p8_tile_cols
    # 1024 -> 4096 over 5120 columns on 512 slots: 64 x 256 is 1280 workgroups = 3 rounds x 256; 64 x 128 is 2560 = 5 rounds x 128
    assert f(4096, 5120, 1, 512) == 128
    # 1536 -> 6144: 96 row tiles x 20 = 1920 -> 4 rounds x 256 = 1024; x 40 = 3840 -> 8 rounds x 128 = 1024: tie -> 256
    assert f(6144, 5120, 1, 512) == 256
    # per-clip T = 960: 4 tiles of 256 or 8 of 128 per clip pad the same 64 columns; 32 row tiles x 32 clips: 8 x 256 = 16 x 128
    assert f(2048, 960, 32, 512) == 256
    # one round either way: the narrow tile's round is half as long
    assert f(136, 1041, 1, 512) == 128
    # 513 .. 1024 narrow workgroups against at most 512 wide ones: two short rounds = one long round -> 256
    assert f(64, 256 * 300, 1, 512) == 256
    # a ragged column count: 257 columns are two tiles of 256 (one round of 256) or three of 128 (one round of 128)
    assert f(64, 257, 1, 512) == 128
    # fewer slots (a smaller part): 1280 wide workgroups = 5 rounds of 256 slots x 256 = 1280; 2560 narrow = 10 x 128 = 1280 -> 256
    assert f(4096, 5120, 1, 256) == 256
    assert f(0, 5120, 1, 512) == 0 and f(4096, 0, 1, 512) == 0 and f(4096, 5120, 0, 512) == 0 and f(4096, 5120, 1, 0) == 0


def test_form_chosen_for_the_bench_shapes(monkeypatch):
    """With a P8 input the wired shapes run on the new form at the width the cost model picks (256 CUs = 512 slots, also what the
    library assumes where it sees no device); the shapes measured slower there keep the 128 x 128 form.  The id stays 15."""
    monkeypatch.setattr(ops, "GSPLIT_P8_COLS", 0)
    for what, build, K, cols in _bench_shapes():
        vid, name = ops.conv_variant(_operands(build(), True))
        assert vid == 15 and name == (NEW % (K, cols) if cols else OLD % K), (what, name)
        assert name.startswith("conv1d_gemm_split_kernel<%d>" % K)


def test_fp32_input_descriptors_keep_the_old_kernel(monkeypatch):
    """The new form exists for P8 inputs only: the same nine shapes with an fp32 input resolve to the 128 x 128 form whatever the
    switch says."""
    for req in (0, -1, 128, 256):
        monkeypatch.setattr(ops, "GSPLIT_P8_COLS", req)
        for what, build, K, _ in _bench_shapes():
            assert ops.conv_variant(_operands(build(), False)) == (15, OLD % K), (req, what)


def test_switch_restores_the_old_choice_everywhere(monkeypatch):
    """gsplit_p8_cols = -1: every P8 launch names the 128 x 128 form; 128 / 256 force that width on every P8 shape, wired or not;
    any other value is refused."""
    monkeypatch.setattr(ops, "GSPLIT_P8_COLS", -1)
    for what, build, K, _ in _bench_shapes():
        assert ops.conv_variant(_operands(build(), True)) == (15, OLD % K), what
    for req in (128, 256):
        monkeypatch.setattr(ops, "GSPLIT_P8_COLS", req)
        for what, build, K, _ in _bench_shapes():
            assert ops.conv_variant(_operands(build(), True)) == (15, NEW % (K, req)), (req, what)
    monkeypatch.setattr(ops, "GSPLIT_P8_COLS", 64)
    d = _operands(_bench_shapes()[1][1](), True)
    assert d.gsplit_p8_cols == 64 and ops.conv_variant(d)[0] < 0
    assert ops.conv_variant(_operands(_bench_shapes()[1][1](), False))[0] == 15      # ignored without a P8 input


def test_descriptor_field_is_appended_and_defaults_to_the_library_choice():
    names = [n for n, _ in _lib.ConvDesc._fields_]
    assert names[-1] == "gsplit_p8_cols" and names[-2] == "keep_tile160"
    assert ops.GSPLIT_P8_COLS == 0 and ops.conv_desc(1, 64, 1024, 64, 1, t_out=1024, pad_left=0).gsplit_p8_cols == 0
