"""The bf16 GEMM kernels under each matrix-instruction shape (s6d_set_gemm_mfma_shape: 16 = v_mfma_f32_16x16x32_bf16, 32 =
v_mfma_f32_32x32x16_bf16; csrc/s6d_gemm.hip).  The bodies are those of tests/test_gpu_gemm.py, imported and called with the shape
pinned -- their bounds are the bounds here: 2^-8 |ref| + 1e-5 (x 1.01) against the float product, 3e-3 relative rms for the folded
LayerNorm, the statistics bounds of test_residual_gemm_row_statistics.  Shape 32 is pinned too: the library's choice may be either,
and the path it does not take must stay covered.  The shapes are the smallest at which each part of the kernel is exercised (one
tile / two K tiles, ragged M with a padded row stride, one K tile per output tile on few workgroups, the stream changing tile with
the ring wrapping, the 256 x 128 form, the residual prefetch across tiles, 40 and 32 statistics groups, column blocks of 64 and 80).

Between the two shapes nothing is asserted on the GPU: the hardware's summation order inside the two instructions is not documented
(profiles/gemm_mfma_shape.md records the share of differing outputs); tests/test_emu_gemm_shape.py compares them where the order
is known."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [16, 32]


class pinned:
    """the matrix-instruction shape for the duration of a test; both switches back to the library's choice afterwards"""

    def __init__(self, shape):
        self.shape = shape

    def __enter__(self):
        from sam6d_amd import ops
        ops.set_gemm_mfma_shape(self.shape)

    def __exit__(self, *exc):
        from sam6d_amd import ops
        ops.set_gemm_mfma_shape(0)
        ops.set_gemm_wave_tile(0)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("M,N,K,pad,blocks", [
    (256, 256, 128, 0, 0),         # one tile, two K tiles
    (300, 256, 320, 8, 0),         # ragged M, padded lda, the ring wraps
    (1280, 768, 64, 0, 8),         # 15 tiles on 8 workgroups: every K tile is first and last
    (2560, 512, 128, 0, 8),        # the stream changes tile in every other K tile
    (1536, 768, 192, 0, 8),        # the ring wraps inside a tile
    (520, 384, 256, 0, 0),         # N % 256 = 128: the 256 x 128 form
])
@pytest.mark.parametrize("kind", ["plain", "gelu", "nobias"])
def test_plain_gelu_and_no_bias_products(M, N, K, pad, blocks, kind, shape):
    from tests import test_gpu_gemm as T
    with pinned(shape):
        T.test_shapes_edges_and_persistent_streams(M, K, N, kind == "gelu", kind != "nobias", pad, blocks)


@pytest.mark.parametrize("shape", SHAPES)
def test_residual_in_the_accumulators(shape):
    from tests import test_gpu_gemm as T
    with pinned(shape):
        T.test_residual_gemm_sums_in_the_accumulators(300, 256, 64, True)       # in place
        T.test_residual_gemm_sums_in_the_accumulators(700, 768, 192, False)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["res", "res_nobias"])
def test_residual_prefetch_across_tiles_on_8_workgroups(kind, shape):
    """20 tiles on 8 workgroups, two K tiles each: a tile's residual values are fetched during the previous tile's epilogue.  The body
    compares the two wave-tile settings, repeats the launch ten times bit for bit and checks the result against the float sum; with
    shape 16 pinned both settings run the eight-wave form on 16x16x32 (the four-wave form has no such shape)."""
    from tests import test_gpu_gemm as T
    with pinned(shape):
        T.test_four_wave_form_gives_the_bits_of_the_eight_wave_form(2560, 512, 128, kind, 8)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("M,N,K", [(260, 1280, 64), (300, 1024, 128)])
def test_partial_row_statistics(M, N, K, shape):
    from tests import test_gpu_gemm as T
    with pinned(shape):
        T.test_residual_gemm_row_statistics(M, N, K)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("M,N,K,gelu,cb", [(700, 768, 192, False, 0), (300, 256, 320, True, 0), (520, 768, 256, False, 64),
                                             (512, 1280, 128, False, 80)])
def test_folded_layernorm(M, N, K, gelu, cb, shape):
    from tests import test_gpu_gemm as T
    with pinned(shape):
        T.test_lnfold_gemm_vs_layernorm_then_linear(M, N, K, gelu, cb)


@pytest.mark.parametrize("shape", SHAPES)
def test_folded_layernorm_with_offset_rows(shape):
    from tests import test_gpu_gemm as T
    with pinned(shape):
        T.test_lnfold_gemm_with_offset_rows(300, 256, 320)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("M,N,K,gelu,blocks", [(4096, 256, 1280, False, 0), (300, 256, 320, True, 0), (700, 768, 192, False, 16),
                                                 (261, 512, 64, True, 8)])
def test_the_two_tile_forms_give_each_others_bits(M, N, K, gelu, blocks, shape):
    from tests import test_gpu_gemm as T
    with pinned(shape):
        T.test_small_tile_form_gives_the_bits_of_the_256_tile_form(M, N, K, gelu, False, blocks)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("M,N,K,inplace,stats,bias", [(700, 768, 192, False, True, True), (300, 256, 64, True, False, True),
                                                     (261, 1280, 128, False, True, False)])
def test_the_two_tile_forms_give_each_others_bits_with_residual_and_statistics(M, N, K, inplace, stats, bias, shape):
    from tests import test_gpu_gemm as T
    with pinned(shape):
        T.test_small_tile_residual_form_gives_the_bits_of_the_256_tile_form(M, N, K, inplace, stats, bias)


@pytest.mark.parametrize("shape", SHAPES)
def test_repeated_launches_bit_identical(shape):
    from tests import test_gpu_gemm as T
    with pinned(shape):
        T.test_repeated_launches_are_bit_identical_and_rows_past_m_untouched()


def test_shape_switch_accepts_0_16_32_only():
    from sam6d_amd import _lib
    L = _lib.lib()
    try:
        assert L.s6d_set_gemm_mfma_shape(8) == -1          # S6D_EINVAL
        assert L.s6d_set_gemm_mfma_shape(64) == -1
        assert L.s6d_set_gemm_mfma_shape(16) == 0
        assert L.s6d_set_gemm_mfma_shape(32) == 0
    finally:
        assert L.s6d_set_gemm_mfma_shape(0) == 0


def _operands(M, N, K, dt, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(M, K, generator=g, device="cuda").to(dt)
    w = (torch.randn(N, K, generator=g, device="cuda") / K ** 0.5).to(dt)
    return a, w, torch.randn(N, generator=g, device="cuda")


@pytest.mark.parametrize("M,N,K,gelu", [(768, 512, 256, True), (520, 384, 128, False)])
def test_a_pinned_wave_tile_pins_the_32x32x16_instruction(M, N, K, gelu):
    """Wave tile 64 with the shape left to the library == shape 32 with the wave tile left to the library, bit for bit (the second
    case: the 256 x 128 form)."""
    from sam6d_amd import ops
    a, w, b = _operands(M, N, K, torch.bfloat16, M + N)
    try:
        ops.set_gemm_wave_tile(64)
        by_tile = ops.gemm_bf16(a, w, b, gelu=gelu).clone()
        ops.set_gemm_wave_tile(0)
        ops.set_gemm_mfma_shape(32)
        by_shape = ops.gemm_bf16(a, w, b, gelu=gelu).clone()
    finally:
        ops.set_gemm_mfma_shape(0)
        ops.set_gemm_wave_tile(0)
    assert torch.equal(by_tile, by_shape)


@pytest.mark.parametrize("M,N,K", [(768, 512, 256), (300, 768, 192)])
def test_the_half_product_does_not_depend_on_the_shape_setting(M, N, K):
    """IEEE half has one matrix instruction (the PEM's 1e-3 mm bar rests on it): the same bits under 0, 16 and 32; the second case
    takes the 256 x 128 form."""
    from sam6d_amd import ops
    a, w, b = _operands(M, N, K, torch.float16, M + K)
    out = {}
    try:
        for s in (0, 16, 32):
            ops.set_gemm_mfma_shape(s)
            out[s] = ops.gemm_bf16(a, w, b, gelu=True).clone()
    finally:
        ops.set_gemm_mfma_shape(0)
    assert out[0].dtype == torch.float16 and torch.equal(out[0], out[16]) and torch.equal(out[0], out[32])
