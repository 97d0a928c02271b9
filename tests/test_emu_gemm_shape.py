"""The two bf16 matrix-instruction shapes of the GEMM kernels (csrc/s6d_gemm.hip, s6d_set_gemm_mfma_shape: 32 = 32x32x16,
16 = 16x16x32) on the emulator.  Its matrix instructions accumulate k-ascending in fp32 whatever their shape, so HERE -- and only
here; the hardware's summation order inside the two instructions is not documented -- both shapes must give equal bits for every
epilogue: a wrong lane map, W row order, start value or exchange in the 16x16x32 path shows as a differing output at once.

Every product the emulator tests of tests/test_emu_gemm.py run (its CASES and the bodies its column-block and residual runs call)
is run under shape 32 and under shape 16 with their own bounds; every tensor the GEMM entry points returned and every partial
row-statistics buffer they filled is recorded and compared between the shapes with torch.equal."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bodies():
    from tests import test_emu_gemm as E
    from tests import test_gpu_gemm as T
    from sam6d_amd import ops
    for M, N, K, bias, gelu, mb, pad in E.CASES:
        E._check(ops, M, N, K, bias, gelu, mb, pad, seed=M + K)
    # what test_emu_gemm._run_cblk calls
    T.test_column_block_output_equals_the_plain_product(700, 768, 192, 64)
    T.test_column_block_output_equals_the_plain_product(300, 256, 64, 32)
    # what test_emu_gemm._run_res calls
    T.test_residual_gemm_sums_in_the_accumulators(700, 768, 192, False)
    T.test_residual_gemm_sums_in_the_accumulators(300, 256, 64, True)
    T.test_residual_gemm_row_statistics(700, 768, 192)
    T.test_lnfold_gemm_vs_layernorm_then_linear(700, 768, 192, False, 0)
    T.test_residual_gemm_row_statistics(260, 1280, 64)
    T.test_lnfold_gemm_vs_layernorm_then_linear(300, 256, 320, True, 0)
    T.test_lnfold_gemm_vs_layernorm_then_linear(520, 768, 256, False, 64)
    T.test_lnfold_gemm_with_offset_rows(300, 256, 320)
    T.test_float16_gemm_vs_float(300, 256, 320, True)
    T.test_float16_gemm_vs_float(700, 768, 192, False)
    T.test_small_tile_form_gives_the_bits_of_the_256_tile_form(300, 256, 320, True, False, 0)
    T.test_small_tile_form_gives_the_bits_of_the_256_tile_form(700, 768, 192, False, False, 16)
    T.test_small_tile_form_gives_the_bits_of_the_256_tile_form(261, 512, 64, True, True, 8)
    T.test_small_tile_residual_form_gives_the_bits_of_the_256_tile_form(700, 768, 192, False, True, True)
    T.test_small_tile_residual_form_gives_the_bits_of_the_256_tile_form(300, 256, 64, True, False, True)
    T.test_small_tile_residual_form_gives_the_bits_of_the_256_tile_form(261, 1280, 128, False, True, False)


def _run():
    from tests import hipemu  # noqa: F401
    import ctypes

    from sam6d_amd import _lib, ops
    L = ctypes.CDLL(hipemu.build())
    L.s6d_strerror.restype = ctypes.c_char_p
    L.s6d_strerror.argtypes = [ctypes.c_int]
    L.s6d_last_hip_error.restype = ctypes.c_char_p
    _lib._lib = L
    ops._stream = lambda: ctypes.c_void_p(0)
    torch.Tensor.is_cuda = property(lambda self: True)
    torch.Tensor.cuda = lambda self, *a, **k: self

    log = []

    def recording(fn):
        def call(*a, **k):
            out = fn(*a, **k)
            log.append(out.clone())
            if k.get("stats_partial") is not None:
                log.append(k["stats_partial"].clone())
            return out
        return call

    ops.gemm_bf16 = recording(ops.gemm_bf16)
    ops.gemm_bf16_lnfold = recording(ops.gemm_bf16_lnfold)
    got = {}
    try:
        for shape in (32, 16):
            assert L.s6d_set_gemm_mfma_shape(shape) == 0
            del log[:]
            _bodies()
            got[shape] = list(log)
    finally:
        L.s6d_set_gemm_mfma_shape(0)
    print(len(got[16]), "recorded tensors per shape")
    assert len(got[16]) == len(got[32]) >= 2 * 8 + 18        # two launches per CASE, at least one per body
    n_stats = 0
    for i, (a, b) in enumerate(zip(got[16], got[32])):
        assert a.shape == b.shape and a.dtype == b.dtype, i
        n_stats += a.dtype == torch.float32
        # statistics buffers start as NaN and are filled completely; compare the bit patterns
        same = torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)
        assert same, f"call {i} {tuple(a.shape)} {a.dtype}: {int((a != b).sum())} values differ between the shapes"
    assert n_stats >= 6


@pytest.mark.parametrize("mode", ["early", "late"])
def test_both_mfma_shapes_give_equal_bits_on_the_emulator(mode):
    """One interpreter per LDS-DMA completion model (HIPEMU_GLDS is read once per process)."""
    r = subprocess.run([sys.executable, "-c", f"import sys; sys.path.insert(0, {ROOT!r}); "
                        f"from tests import test_emu_gemm_shape as t; t._run()"], env=dict(os.environ, HIPEMU_GLDS=mode),
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
