"""Board power and shader clock while the bf16 GEMM runs back to back under each matrix-instruction shape (s6d_set_gemm_mfma_shape),
lin1 shape 65536 x 1280 -> 5120 with the folded LayerNorm + GELU epilogue of the benched step and with the plain one: the sampling
loop of tools/gemm_power.py (rocm-smi is only read), two interleaved rounds.  The claim under test for the 16x16x32 shape is "same
cycles, higher clock".   python tools/gemm_shape_power.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_power import arm  # noqa: E402

from sam6d_amd import ops  # noqa: E402


def main():
    g = torch.Generator(device="cuda").manual_seed(0)
    M, K, N = 65536, 1280, 5120
    a = torch.randn(M, K, generator=g, device="cuda").to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g, device="cuda") / K ** 0.5).to(torch.bfloat16)
    b = torch.randn(N, generator=g, device="cuda")
    out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    st, cs = ops.row_stats(a, 1e-6), w.float().sum(1).contiguous()
    flop = 2.0 * M * N * K
    try:
        for rnd in range(2):
            for mi in (32, 16):
                ops.set_gemm_mfma_shape(mi)
                arm(f"plain shape {mi} round {rnd}", lambda: ops.gemm_bf16(a, w, b, out=out), flop, 3.0)
                arm(f"lnfold+gelu shape {mi} round {rnd}", lambda: ops.gemm_bf16_lnfold(a, st, w, cs, b, gelu=True), flop, 3.0)
    finally:
        ops.set_gemm_mfma_shape(0)


if __name__ == "__main__":
    main()
