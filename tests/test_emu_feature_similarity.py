"""The feature-similarity kernel (csrc/s6d_sim.hip) executed on the HOST through the emulated HIP runtime: the bodies of
tests/test_gpu_feature_similarity.py at their small shapes (the kernel source itself runs: row normalisation, zero-filled tail
fragments, guarded stores, the k order of the matrix instructions, several chunks of f2)."""
import pytest

from tests import test_gpu_feature_similarity as T


@pytest.mark.parametrize("B,M1,M2,C", T.SMALL_SHAPES)
def test_vs_float64_on_the_emulator(emu, B, M1, M2, C):
    T.check_vs_float64(emu, B, M1, M2, C)


def test_hostile_rows_on_the_emulator(emu):
    T.check_hostile_rows(emu, 2, 37, 21, 32)


@pytest.mark.parametrize("B,M1,M2,C", T.SMALL_SHAPES)
def test_batch_invariance_on_the_emulator(emu, B, M1, M2, C):
    T.check_batch_invariance(emu, M1, M2, C)


@pytest.mark.parametrize("B,M1,M2,C", T.SMALL_SHAPES)
def test_transpose_symmetry_on_the_emulator(emu, B, M1, M2, C):
    T.check_transpose_symmetry(emu, B, M1, M2, C)


def test_into_sampling_head_on_the_emulator(emu):
    T.check_into_sampling_head(emu, 2, 40, 32, 300, 30)


def test_arguments_on_the_emulator(emu):
    T.check_arguments(emu)
