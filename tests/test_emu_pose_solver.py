"""The bodies of tests/test_gpu_pose_solver.py on the HOST build of the kernel sources (the `emu` fixture), at the same shapes."""
import pytest

from tests import test_gpu_pose_solver as T


def test_rot_from_h_on_the_emulator(emu):
    T.check_rot_from_h(emu)


@pytest.mark.parametrize("N1,N2", [(40, 40), (33, 50)])
def test_pose_hypotheses_on_the_emulator(emu, N1, N2):
    T.check_pose_hypotheses(emu, N1, N2)


def test_weighted_procrustes_on_the_emulator(emu):
    for N in (1, 255, 256, 257, 513):
        T.check_weighted_procrustes_sizes(emu, N)
    T.check_weighted_procrustes_degenerate(emu)
    for scale in (1e-4, 1e3):
        T.check_weighted_procrustes_scales(emu, scale)
    T.check_weighted_procrustes_nan_neighbours(emu)


@pytest.mark.parametrize("M1,M2", T.COARSE_SHAPES)
def test_coarse_sample_shapes_on_the_emulator(emu, M1, M2):
    T.check_coarse_sample_shape(emu, M1, M2)


def test_coarse_sample_classes_on_the_emulator(emu):
    T.check_coarse_sample_refused(emu)
    T.check_coarse_sample_all_background(emu)
    for M in (17, 40, 70):
        T.check_coarse_sample_ties(emu, M)
    for mag in (10, 32):
        T.check_coarse_sample_magnitudes(emu, mag)


@pytest.mark.parametrize("n,k", T.SMALLEST_K)
def test_smallest_k_on_the_emulator(emu, n, k):
    T.check_smallest_k(emu, n, k)


def test_selections_on_the_emulator(emu):
    T.check_smallest_k_refused(emu)
    for P in (1, 4, 5, 300):
        for N in (1, 63, 64, 65, 196):
            T.check_hypothesis_select(emu, P, N)


def test_min_dist_on_the_emulator(emu):
    for Nm in (1, 2, 3, 4, 5, 1021, 5460):
        T.check_min_dist(emu, Nm, 257)
    for N in (1, 255, 256):
        T.check_min_dist(emu, 1021, N)
    T.check_min_dist(emu, 1021, 257, scale=1e3)
    T.check_min_dist_refused(emu)


@pytest.mark.parametrize("M1,M2", T.FINE_SHAPES)
def test_fine_kernels_shapes_on_the_emulator(emu, M1, M2):
    T.check_fine_shape(emu, M1, M2)


@pytest.mark.parametrize("cls", T.FINE_CLASSES)
def test_fine_kernels_input_classes_on_the_emulator(emu, cls):
    T.check_fine_class(emu, cls)


def test_fine_kernels_exact_ties_on_the_emulator(emu):
    T.check_fine_ties(emu)


def test_temperature_domain_on_the_emulator(emu):
    T.check_temperature_domain(emu)


def test_pem_caller_temperature_on_the_emulator(emu, monkeypatch):
    T.check_pem_caller_temperature(emu, monkeypatch)
