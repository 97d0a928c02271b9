"""The GEMM launcher's status codes and kernel selection (csrc/s6d_gemm.hip: gemm_launch) on the HOST build: the bodies of
tests/test_gpu_gemm_dispatch.py through the emulated HIP runtime.  The four-wave form is a stub there (it is assembly), so the wave-tile
switch stays at 0; the launches are kept to one per kernel instantiation (EMU_SETTINGS)."""
from tests import test_gpu_gemm_dispatch as T


def test_status_codes_on_the_emulator(emu):
    T.check_status_table(emu)


def test_every_instantiation_launches_and_is_right_on_the_emulator(emu):
    # N = 256: all 22 combinations on the 256 x 256 kernels at 32x32x16, the 8 bf16 ones again at 16x16x32, the 10 plain / GELU /
    # residual ones (bf16 and half) on the 256 x 128 kernel at 32x32x16 and its 6 bf16 ones at 16x16x32; N = 384: 4
    assert T.check_launches(emu, T.EMU_SETTINGS) == 22 + 8 + 10 + 6 + 4
