"""The ADD / ADD-S kernels (csrc/s6d_adderr.hip) executed on the HOST through the emulated HIP runtime: the bodies of
tests/test_gpu_add_eval.py at the same shapes (the kernel source itself runs: the float32 statements, the LDS tiles with their source
and target tails, the minimum on the bits, the fixed-order float64 sum with its butterfly), the case of several source blocks per
estimate at every sources-per-lane setting (V = 4099, about two seconds) included."""
import pytest

from tests import test_gpu_add_eval as T


@pytest.mark.parametrize("N", T.SHAPES_N)
@pytest.mark.parametrize("V", T.SHAPES_V)
def test_add_errors_vs_restatement_on_the_emulator(emu, V, N):
    T.check_errors(emu, V, N)


def test_add_errors_several_source_blocks_on_the_emulator(emu):
    T.check_errors(emu, 4099, 2)


def test_known_answers_on_the_emulator(emu):
    T.check_known_answers(emu)


def test_hostile_inputs_on_the_emulator(emu):
    T.check_hostile(emu)


def test_arguments_on_the_emulator(emu):
    T.check_arguments(emu)


def test_modules_on_the_emulator(emu, monkeypatch):
    T.check_modules(emu, monkeypatch)
