"""The BOP pose-error kernels (csrc/s6d_boperr.hip, the depth entry of csrc/s6d_raster.hip) executed on the HOST through the
emulated HIP runtime: the bodies of tests/test_gpu_bop_eval.py at the same shapes (the kernel source itself runs: the float32
statements, the wave and LDS reductions, the atomics on the float's bits, both work shapes of the depth render)."""
import pytest

from tests import test_gpu_bop_eval as T


@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("S", [1, 2, 7, 315])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 257, 1000])
def test_pose_errors_vs_restatement_on_the_emulator(emu, V, S, N):
    T.check_pose_errors(emu, V, S, N)


def test_pose_known_answers_on_the_emulator(emu):
    T.check_pose_known_answers(emu)


def test_pose_hostile_inputs_on_the_emulator(emu):
    T.check_pose_hostile(emu)


@pytest.mark.parametrize("name", ["cube", "torus"])
def test_render_depth_equals_render_views_on_the_emulator(emu, name):
    T.check_render_depth(emu, name)


def test_render_depth_counts_skipped_on_the_emulator(emu):
    T.check_render_depth_skipped(emu)


@pytest.mark.parametrize("NT", [1, 10])
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N", [1, 3, 5])
@pytest.mark.parametrize("hw", sorted(T.SIZES))
def test_vsd_counts_vs_restatement_on_the_emulator(emu, hw, N, M, NT):
    T.check_vsd_counts(emu, hw, N, M, NT)


def test_vsd_counts_torus_on_the_emulator(emu):
    T.check_vsd_counts(emu, (48, 64), 3, 2, 10, "torus")


def test_vsd_known_answers_on_the_emulator(emu):
    T.check_vsd_known_answers(emu)


def test_arguments_on_the_emulator(emu):
    T.check_arguments(emu)


def test_modules_on_the_emulator(emu, monkeypatch):
    T.check_modules(emu, monkeypatch)
