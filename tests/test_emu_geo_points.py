"""The points-fed index stage of the geometric structure embedding executed on the HOST through the emulated HIP runtime: the
bodies of tests/test_gpu_geo_points.py at their small shapes (the kernel sources themselves run: wave-wide neighbour selection,
tie rule, the points-fed prologues of both embedding kernels)."""
import pytest

from tests import test_gpu_geo_points as T


@pytest.mark.parametrize("B,N", [(1, 37), (2, 5)])
def test_indices_vs_fp64_on_the_emulator(emu, B, N):
    T.check_indices_vs_fp64(emu, B, N)


def test_ties_and_degenerate_points_on_the_emulator(emu):
    T.check_ties_and_degenerate_points(emu)


@pytest.mark.parametrize("B,N", [(1, 37), (2, 5)])
def test_fused_equals_two_step_on_the_emulator(emu, B, N):
    T.check_fused_equals_two_step(emu, B, N)


@pytest.mark.parametrize("B,N", [(2, 37), (3, 5)])
def test_batch_invariance_on_the_emulator(emu, B, N):
    T.check_batch_invariance(emu, B, N)


def test_bad_arguments_on_the_emulator(emu):
    T.check_bad_arguments(emu)
