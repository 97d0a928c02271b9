"""The pose verification kernels (csrc/s6d_verify.hip) executed on the HOST through the emulated HIP runtime: the bodies of
tests/test_gpu_verify.py at the same shapes (the kernel source itself runs: the two float32 statements, the ballots and popcounts,
the LDS reductions, the integer atomics, the claimed bitmap in LDS and in the workspace)."""
import pytest

from tests import test_gpu_verify as T


@pytest.mark.parametrize("with_masks", [False, True])
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N", [1, 3, 5])
@pytest.mark.parametrize("hw", sorted(T.SIZES))
def test_evidence_vs_restatement_on_the_emulator(emu, hw, N, M, with_masks):
    T.check_evidence(emu, hw, N, M, with_masks)


def test_evidence_torus_on_the_emulator(emu):
    T.check_evidence(emu, (48, 64), 3, 2, True, "torus")


def test_evidence_hostile_pixels_on_the_emulator(emu):
    T.check_hostile(emu)


@pytest.mark.parametrize("lds_words", [0, 1])
def test_selection_vs_restatement_on_the_emulator(emu, lds_words):
    T.check_selection(emu, lds_words)


def test_known_answers_on_the_emulator(emu):
    T.check_known_answers(emu)


def test_arguments_on_the_emulator(emu):
    T.check_arguments(emu)


def test_modules_on_the_emulator(emu, monkeypatch):
    T.check_modules(emu, monkeypatch)
