"""The COCO AP kernels (csrc/s6d_cocoeval.hip) executed on the HOST through the emulated HIP runtime: the bodies of
tests/test_gpu_coco_eval.py at the small shapes (the kernel source itself runs: the ballots of the packing, the segment rule, the
wave and LDS sums and the integer atomics of the pair kernel, the float64 chain of the boxes, the 64-bit matched mask).  Lanes are
fibers here: 480 x 640 stays on the GPU."""
import pytest

from tests import test_gpu_coco_eval as T


@pytest.mark.parametrize("N", [1, 3, 65])
@pytest.mark.parametrize("hw", T.SHAPES)
def test_mask_pack_vs_restatement_on_the_emulator(emu, hw, N):
    T.check_pack(emu, hw, N)


@pytest.mark.parametrize("P", [0, 1, 257])
@pytest.mark.parametrize("hw", T.SHAPES)
def test_mask_pair_inter_vs_restatement_on_the_emulator(emu, hw, P):
    T.check_pair_inter(emu, hw, 3, P)


@pytest.mark.parametrize("N", [1, 65])
def test_mask_pair_inter_row_counts_on_the_emulator(emu, N):
    T.check_pair_inter(emu, (5, 13), N, 257)


def test_mask_pair_inter_two_chunks_on_the_emulator(emu):
    T.check_pack(emu, T.TWO_CHUNKS, 2)
    T.check_pair_inter(emu, T.TWO_CHUNKS, 2, 1)


def test_mask_pair_inter_long_runs_on_the_emulator(emu):
    T.check_long_runs(emu)


def test_box_pair_iou_vs_restatement_on_the_emulator(emu):
    T.check_box_iou(emu)


def test_match_situations_on_the_emulator(emu):
    T.check_match_special(emu)


@pytest.mark.parametrize("G", [0, 1, 64])
@pytest.mark.parametrize("D", [0, 1, 17, 100])
def test_match_vs_restatement_on_the_emulator(emu, D, G):
    T.check_match_sizes(emu, D, G)


def test_match_65_ground_truths_take_the_library_route_on_the_emulator(emu):
    T.check_match_oversize(emu)


@pytest.mark.parametrize("extra", [0, 101])
def test_scores_kernel_route_equals_library_route_equals_restatement_on_the_emulator(emu, monkeypatch, extra):
    T.check_scores(emu, monkeypatch, extra)


def test_scores_known_answers_on_the_emulator(emu):
    T.check_scores_known_answers(emu)


def test_scores_perfect_detections_give_one_on_the_emulator(emu):
    T.check_scores_perfect(emu)


def test_arguments_on_the_emulator(emu):
    T.check_arguments(emu)
