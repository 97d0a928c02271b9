"""The pose-refinement kernels (csrc/s6d_refine.hip) executed on the HOST through the emulated HIP runtime: the bodies of
tests/test_gpu_refine.py at the same shapes (the kernel source itself runs: the float64 statements, the lane stride, the butterfly,
the wave and chunk order, the Cholesky solve and the Cayley update; the renders they read come from the emulated rasteriser)."""
import pytest

from tests import test_gpu_refine as T


@pytest.mark.parametrize("hw,T_,M,with_mask,name", T.CASES)
def test_normal_equations_equal_the_restatement_on_the_emulator(emu, hw, T_, M, with_mask, name):
    T.check_normal_eq(emu, hw, T_, M, with_mask, name)


def test_every_predicate_passes_and_rejects_on_the_emulator(emu):
    T.check_predicates(emu)


def test_batch_invariance_and_repeatability_on_the_emulator(emu):
    T.check_batch_invariance(emu)


def test_update_known_answers_and_restatement_on_the_emulator(emu):
    T.check_update(emu)


def test_hostile_inputs_on_the_emulator(emu):
    T.check_hostile(emu)


def test_loop_equals_chained_restatement_on_the_emulator(emu):
    T.check_loop(emu)


def test_convergence_on_the_emulator(emu):
    T.check_convergence(emu)


def test_arguments_on_the_emulator(emu):
    T.check_arguments(emu)


def test_modules_on_the_emulator(emu, monkeypatch):
    T.check_modules(emu, monkeypatch)
