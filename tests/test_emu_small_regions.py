"""The connected-component and small-region kernels (csrc/s6d_ccl.hip) executed on the HOST through the emulated HIP runtime: the
bodies of tests/test_gpu_small_regions.py at its small shapes (the kernel source itself runs: the union-find of a tile in LDS, the
seams between tiles -- the shape BIG is three tiles each way --, the ballots of the per-wave counts, the 64-bit best-component
maximum, the box atomics).  Lanes are fibers here: 480 x 640 stays on the GPU."""
import pytest

from tests import test_gpu_small_regions as T


@pytest.mark.parametrize("hw", T.SHAPES)
def test_remove_small_regions_vs_restatement_on_the_emulator(emu, hw):
    for k, a in enumerate(T.min_areas(hw)):
        T.check_remove(emu, hw, a, as_bool=k % 2 == 1)


@pytest.mark.parametrize("hw", T.SHAPES)
def test_label_components_vs_restatement_on_the_emulator(emu, hw):
    T.check_labels(emu, hw)


def test_results_do_not_depend_on_batch_or_chunk_on_the_emulator(emu, monkeypatch):
    T.check_batching(emu, monkeypatch)


def test_arguments_on_the_emulator(emu):
    T.check_arguments(emu)
