"""The overlay kernels (csrc/s6d_vis.hip) executed on the HOST through the emulated HIP runtime: the bodies of tests/test_gpu_vis.py
at its shapes (the kernel source itself runs: the first-hit loop over the packed words, the merge rule, the LDS halo and the
dilation of the paint tiles with their dword and byte paths, the float32 projection, the ballots, ranks and wave prefix of the
draw kernel's compaction and its int64 coverage test).  sam6d_amd.visualize on top dispatches to the same emulated kernels."""
import pytest

from tests import test_gpu_vis as T


@pytest.fixture
def api(emu):
    return T.KernelApi(emu)


@pytest.mark.parametrize("N", T.OWNER_N)
@pytest.mark.parametrize("B", T.BATCHES)
@pytest.mark.parametrize("hw", T.SIZES)
def test_owner_from_masks_vs_restatement_on_the_emulator(api, hw, B, N):
    T.check_owner(api, hw, B, N)


@pytest.mark.parametrize("B", T.BATCHES)
@pytest.mark.parametrize("hw", T.SIZES)
def test_merge_layers_vs_restatement_and_any_chunking_on_the_emulator(api, hw, B):
    T.check_merge(api, hw, B)


@pytest.mark.parametrize("config", T.PAINT_CONFIGS)
@pytest.mark.parametrize("B", T.BATCHES)
@pytest.mark.parametrize("hw", T.SIZES)
def test_paint_vs_restatement_on_the_emulator(api, hw, B, config):
    T.check_paint(api, hw, B, config)


def test_paint_known_answer_on_the_emulator(api):
    T.check_paint_known_answer(api)


def test_projection_bits_vs_restatement_on_the_emulator(api):
    T.check_project(api)


@pytest.mark.parametrize("B", T.BATCHES)
@pytest.mark.parametrize("hw", T.SIZES)
def test_draw_vs_restatement_on_the_emulator(api, hw, B):
    T.check_draw(api, hw, B)


def test_draw_other_frames_and_empty_list_on_the_emulator(api):
    T.check_draw_other_frames_and_empty(api)


def test_draw_known_answer_on_the_emulator(api):
    T.check_draw_known_answer(api)


@pytest.mark.parametrize("B", T.BATCHES)
@pytest.mark.parametrize("mode", [("box", "points"), ("surface",), ("surface", "box", "points")])
def test_pose_pictures_vs_restatement_on_the_emulator(api, mode, B):
    T.check_pose_pictures(api, mode, B)


@pytest.mark.parametrize("B", T.BATCHES)
@pytest.mark.parametrize("top", [1, None])
def test_detection_pictures_vs_restatement_on_the_emulator(api, top, B):
    T.check_detection_pictures(api, top, B)


def test_a_frame_alone_has_the_bits_it_has_in_the_group_on_the_emulator(api):
    T.check_batch_invariance(api)


def test_arguments_on_the_emulator(api):
    T.check_arguments(api)
