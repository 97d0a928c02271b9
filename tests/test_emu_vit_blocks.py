"""The bodies of tests/test_gpu_vit_blocks.py on the HOST through the emulated HIP runtime: the block loop's launch trace and its
output in every form of the three ViTs."""
import pytest

from tests import test_gpu_vit_blocks as T


@pytest.mark.parametrize("name", list(T.CASES))
def test_block_loop_launches_and_output_on_the_emulator(emu, name):
    T.case_body(name, dev="cpu")


@pytest.mark.parametrize("model", ["sam", "dino"])
def test_folded_form_against_the_add_layernorm_form_on_the_emulator(emu, model):
    T.fold_body(model, dev="cpu")
