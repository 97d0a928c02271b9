"""The BOP ground-truth kernels (csrc/s6d_bopgt.hip) executed on the HOST through the emulated HIP runtime: the bodies of
tests/test_gpu_bop_gt.py at the same shapes (the kernel source itself runs: the float32 statements, the wave and LDS reductions, the
integer atomics, the persistent tile loop of the diameter)."""
import pytest

from tests import test_gpu_bop_gt as T


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N", [1, 3, 5])
@pytest.mark.parametrize("kind", T.MARGINS)
@pytest.mark.parametrize("hw", sorted(T.SIZES))
def test_visibility_vs_restatement_on_the_emulator(emu, hw, kind, N, M):
    T.check_visibility(emu, hw, kind, N, M)


def test_visibility_torus_on_the_emulator(emu):
    T.check_visibility(emu, (48, 64), "image", 3, 2, "torus")


def test_visibility_known_answers_on_the_emulator(emu):
    T.check_visibility_known_answers(emu)


@pytest.mark.parametrize("V", T.DIAMETER_V)
def test_diameter_vs_restatement_on_the_emulator(emu, V):
    T.check_diameter(emu, V)


def test_diameter_hostile_inputs_on_the_emulator(emu):
    T.check_diameter_hostile(emu)


def test_arguments_on_the_emulator(emu):
    T.check_arguments(emu)


def test_modules_on_the_emulator(emu, monkeypatch):
    T.check_modules(emu, monkeypatch)
