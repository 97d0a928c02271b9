"""Bodies of tests/test_gpu_pem_attention.py on the HOST emulator (tests/hipemu.py), B <= 2 and the small sizes of each list: the
rows kernel's five RPE entry points and the two plain ones with every construction of the device test, the LDS limit (at the
limit for plain attention; the RPE launchers' refusals one above -- their 1 GiB embedding at the limit runs on the device only),
the focus map and the linear attention with every construction, and the B = 3 batch invariance at the ragged sizes."""
import pytest

from tests import test_gpu_pem_attention as T


@pytest.mark.parametrize("kinds", T._pairs(T.RPE_KINDS), ids="+".join)
@pytest.mark.parametrize("N", [7, 1])          # 7 % 4 = 3: a ragged key trip (dom_tail: key 4), 14 rows: a ragged query strip
def test_rpe_attention_entry_points_on_the_emulator(emu, N, kinds):
    T.rpe_case(N, kinds, dev="cpu", tag="_emu")


@pytest.mark.parametrize("kinds", T._pairs(T.MHA_KINDS), ids="+".join)
@pytest.mark.parametrize("N,M", [(1, 1), (3, 3), (4, 4), (5, 5), (2, 15), (2, 16), (2, 17), (5, 22)])
def test_mha_entry_points_on_the_emulator(emu, N, M, kinds):
    T.mha_case(N, M, kinds, dev="cpu", tag="_emu")


def test_mha_lds_limit_on_the_emulator(emu):
    T.mha_lds_limit_case(dev="cpu", tag="_emu")


def test_rpe_lds_limit_refusals_on_the_emulator(emu):
    T.rpe_lds_limit_case(dev="cpu", at_limit=False, layer=False)


@pytest.mark.parametrize("B,I,J", [(1, 65, 29), (1, 1, 1), (2, 5, 3)])
def test_linear_attention_on_the_emulator(emu, B, I, J):
    T.linattn_case(B, I, J, dev="cpu", tag="_emu")


@pytest.mark.parametrize("B,R", [(2, 6), (1, 1)])
def test_linear_attn_focus_on_the_emulator(emu, B, R):
    T.focus_case(B, R, dev="cpu", tag="_emu")


def test_rows_kernel_batch_invariance_on_the_emulator(emu):
    T.rows_batch_invariance_case(7, 5, dev="cpu")
