"""The run-length mask kernels (csrc/s6d_rle.hip) executed on the HOST through the emulated HIP runtime: the bodies of
tests/test_gpu_rle.py at its small shapes (the kernel source itself runs: the lane-per-column transposition, the carries across
words, columns and bands, the ordered scan of the transition counts, the clipped LDS fills, the ballots of the packed words and the
ORs of the words two bands share).  Lanes are fibers here: 480 x 640 stays on the GPU."""
import pytest

from tests import test_gpu_rle as T


@pytest.fixture
def rle_emu(emu):
    yield emu
    emu.set_rle_band_words(0)


@pytest.mark.parametrize("words", [0, T.SMALL_BAND])
@pytest.mark.parametrize("hw", T.SHAPES)
def test_encode_vs_restatement_and_masks_to_rle_on_the_emulator(rle_emu, hw, words):
    T.check_encode(rle_emu, hw, words)


@pytest.mark.parametrize("words", [0, T.SMALL_BAND])
@pytest.mark.parametrize("hw", T.SHAPES)
def test_runs_to_packed_vs_mask_pack_and_restatement_on_the_emulator(rle_emu, hw, words):
    T.check_packed(rle_emu, hw, words)


@pytest.mark.parametrize("words", [0, T.SMALL_BAND])
@pytest.mark.parametrize("hw", T.SHAPES)
def test_runs_to_dense_on_the_emulator(rle_emu, hw, words):
    T.check_dense(rle_emu, hw, words)


@pytest.mark.parametrize("words", [0, T.SMALL_BAND])
def test_results_do_not_depend_on_the_batch_on_the_emulator(rle_emu, words):
    T.check_batching(rle_emu, T.BANDS, words)


def test_non_canonical_lists_are_accepted_on_the_emulator(rle_emu):
    T.check_noncanonical(rle_emu)


def test_bad_lists_are_refused_with_the_mask_index_on_the_emulator(rle_emu):
    T.check_refused(rle_emu)


def test_arguments_on_the_emulator(rle_emu):
    T.check_arguments(rle_emu)


def test_coco_scores_from_run_lists_equal_the_dense_result_on_the_emulator(rle_emu):
    T.check_coco_scores(rle_emu, "cpu")
