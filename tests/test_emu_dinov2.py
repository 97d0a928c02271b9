"""Bodies of tests/test_gpu_dinov2_production.py on the HOST emulator (tests/hipemu.py): the sequence attention at the production
token counts (257 keys in bf16, 197 in IEEE half: one real key or five in the tail tile) with B <= 2 and nh <= 2, every construction
of the device test included, and one block of the folded loop's kernels at 300 rows with C = 256."""
import pytest

from tests import test_gpu_dinov2_production as T

PAIRS = [{0: "dom_last", 1: "grow"}, {0: "dom_cls", 1: "shrink"}, {0: "dom_full", 1: "creep"}, {0: "vscale", 1: "random"}]


@pytest.mark.parametrize("kinds", PAIRS, ids=lambda k: "+".join(k.values()))
def test_seq_attention_bf16_257_tokens_on_the_emulator(emu, kinds):
    T.seq_attention_case(T.BF, 2, 257, 2, 64, kinds, dev="cpu", tag="_emu")


@pytest.mark.parametrize("kinds", PAIRS, ids=lambda k: "+".join(k.values()))
def test_seq_attention_f16_197_tokens_on_the_emulator(emu, kinds):
    T.seq_attention_case(T.F16, 2, 197, 2, 64, kinds, dev="cpu", tag="_emu")


def test_folded_block_kernels_on_the_emulator(emu):
    """300 rows: one full 256-row tile and a ragged one of 44 rows; rows past M hold a sentinel."""
    T.folded_block_case(300, C=256, hidden=512, dev="cpu", pad=64)
