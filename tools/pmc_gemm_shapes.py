"""Launch the ViT-H lin1 GEMM (65536 x 1280 -> 5120, folded LayerNorm + GELU, as in the benched step) and lin2 with the residual epilogue a
few times under each matrix-instruction shape (s6d_set_gemm_mfma_shape): the target of a rocprofv3 --pmc pass.  The two shapes are
different template instances (gemm_bf16_kernel<., ., 32> / <., ., 16>), so one pass gives both columns; fold it with
tools/pmc_sq_summarise.py.
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES --kernel-trace \\
              --output-format csv -d DIR -o s -- python tools/pmc_gemm_shapes.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sam6d_amd import ops  # noqa: E402

g = torch.Generator(device="cuda").manual_seed(0)
M = 65536
a = torch.randn(M, 1280, generator=g, device="cuda").to(torch.bfloat16)
w1 = (torch.randn(5120, 1280, generator=g, device="cuda") / 1280 ** 0.5).to(torch.bfloat16)
b1 = torch.randn(5120, generator=g, device="cuda")
st, cs = ops.row_stats(a, 1e-6), w1.float().sum(1).contiguous()
h = torch.randn(M, 5120, generator=g, device="cuda").to(torch.bfloat16)
w2 = (torch.randn(1280, 5120, generator=g, device="cuda") / 5120 ** 0.5).to(torch.bfloat16)
b2 = torch.randn(1280, generator=g, device="cuda")
x = torch.randn(M, 1280, generator=g, device="cuda").to(torch.bfloat16)
sp = torch.empty(1280 // 32, 2, M, device="cuda")
try:
    for shape in (32, 16):
        ops.set_gemm_mfma_shape(shape)
        for _ in range(4):
            ops.gemm_bf16_lnfold(a, st, w1, cs, b1, gelu=True)
            ops.gemm_bf16(h, w2, b2, residual=x, stats_partial=sp)
        torch.cuda.synchronize()
finally:
    ops.set_gemm_mfma_shape(0)
print("done")
