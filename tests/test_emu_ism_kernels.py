"""The bodies of tests/test_gpu_ism_kernels.py on the HOST build of the kernel source (the `emu` fixture), at every shape of the device
test: none takes the emulator more than a few seconds, so no shape is dropped."""
import pytest

from tests import test_gpu_ism_kernels as T


@pytest.mark.parametrize("P,R,C", T.COSINE_SHAPES)
def test_pairwise_cosine_on_the_emulator(emu, P, R, C):
    T.check_cosine(emu, P, R, C)
    T.check_cosine_power_of_two_scaling(emu, P, R, C)


def test_pairwise_cosine_rows_on_the_emulator(emu):
    T.check_cosine_row_independence(emu)


@pytest.mark.parametrize("P,O,T_", T.SELECT_SHAPES)
def test_semantic_select_on_the_emulator(emu, P, O, T_):
    T.check_select(emu, P, O, T_)


def test_semantic_select_tie_rules_on_the_emulator(emu):
    T.check_select_ties(emu)
    T.check_select_refused(emu)


@pytest.mark.parametrize("S,N1,N2,C", list(T.PATCH_SHAPES))
def test_patch_scores_on_the_emulator(emu, S, N1, N2, C):
    T.check_patch_scores(emu, S, N1, N2, C)


def test_patch_scores_selection_form_on_the_emulator(emu):
    T.check_patch_sel(emu, 17, 15, 64)
    T.check_patch_sel(emu, 257, 250, 64)
    T.check_patch_refused(emu)


@pytest.mark.parametrize("H,W", T.DEPTH_SHAPES)
def test_masked_depth_mean_on_the_emulator(emu, H, W):
    T.check_masked_depth(emu, H, W)


def test_masked_depth_mean_refusals_on_the_emulator(emu):
    T.check_masked_depth_refused(emu)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_project_bbox_on_the_emulator(emu, N, S):
    T.check_project(emu, N, S)


def test_pairwise_similarity_guard_on_the_emulator(emu):
    T.check_guard_pairwise(emu)


def test_masked_depth_guard_on_the_emulator(emu):
    T.check_guard_masked_depth(emu)


def test_appearance_score_guard_on_the_emulator(emu):
    T.check_guard_appearance(emu)
