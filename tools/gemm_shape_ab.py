"""A/B of the two bf16 matrix-instruction shapes of the GEMM kernels in ONE process (s6d_set_gemm_mfma_shape: 32 = v_mfma_f32_32x32x16_bf16,
16 = v_mfma_f32_16x16x32_bf16; csrc/s6d_gemm.hip) on the shapes of tools/gemm4_ab.py, random operands: parity of both shapes against
the float product of the same operands, the share of outputs in which the two shapes differ (the hardware's summation order inside
the two instructions is not documented, so this is recorded, not asserted), then interleaved timing rounds.
Usage: python tools/gemm_shape_ab.py [rounds >= 3] [OUT.json]   (default: results/gemm_shape_ab.json at the repository root)"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm4_ab import SHAPES, event_ms, make  # noqa: E402

from sam6d_amd import _lib, ops  # noqa: E402


def parity(a, w, b, out, kind, extra, rows=2048):
    """values further than one bf16 rounding (2^-8 |ref| + 1e-5, x 1.01) from the float product, on a sample of the rows"""
    idx = torch.randperm(a.shape[0], device="cuda")[:rows]
    if kind.startswith("lnfold"):
        ref = torch.nn.functional.layer_norm(a[idx].float(), (a.shape[1],), eps=1e-6) @ w.float().t() + b
        if kind == "lnfold_gelu":
            ref = torch.nn.functional.gelu(ref)
        got = out
        if kind == "lnfold_cblk":                                          # (N / cb, M, cb) blocks -> (M, N)
            got = out.permute(1, 0, 2).reshape(a.shape[0], -1)
        d = got[idx].float() - ref
        return {"rel_rms_vs_fp32": float(d.norm() / ref.norm())}       # the folded form rounds the weight product differently: rms
    ref = a[idx].float() @ w.float().t() + b
    if kind == "gelu":
        ref = torch.nn.functional.gelu(ref)
    if kind == "res":
        ref = ref + extra[idx].float()
    err = (out[idx].float() - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + 1e-5
    return {"mismatch_vs_fp32": int((err > 1.01 * tol).sum().item()), "max_err": float(err.max().item())}


def main():
    rounds = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 3)
    L = _lib.lib()
    res = []
    try:
        for name, M, K, N, kind in SHAPES:
            a, w, b = make(M, N, K)
            extra = None
            if kind.startswith("lnfold"):
                stats = ops.row_stats(a, 1e-6)
                cs = w.float().sum(1).contiguous()
                cb = 80 if kind == "lnfold_cblk" else 0
                fn = lambda: ops.gemm_bf16_lnfold(a, stats, w, cs, b, gelu=kind == "lnfold_gelu", col_block=cb)   # noqa: E731
            elif kind == "res":
                extra = torch.randn(M, N, device="cuda").to(torch.bfloat16)
                sp = torch.empty(N // 32, 2, M, device="cuda")
                fn = lambda: ops.gemm_bf16(a, w, b, residual=extra, stats_partial=sp)   # noqa: E731
            else:
                fn = lambda: ops.gemm_bf16(a, w, b, gelu=kind == "gelu")   # noqa: E731
            row = {"name": name, "M": M, "K": K, "N": N, "kind": kind}
            out = {}
            for mi in (32, 16):
                assert L.s6d_set_gemm_mfma_shape(mi) == 0
                out[mi] = fn().clone()
                row[f"parity_{mi}"] = parity(a, w, b, out[mi], kind, extra)
                row[f"repeat_identical_{mi}"] = all(torch.equal(fn(), out[mi]) for _ in range(5))
            row["differing_share"] = float((out[16] != out[32]).float().mean().item())
            del out
            fl = 2.0 * M * N * K
            t = {32: [], 16: []}
            for _ in range(rounds):
                for mi in (32, 16):
                    L.s6d_set_gemm_mfma_shape(mi)
                    t[mi].append(event_ms(fn))
            for mi in (32, 16):
                row[f"ms_{mi}"] = [round(x, 4) for x in t[mi]]
                row[f"tflops_median_{mi}"] = round(fl / statistics.median(t[mi]) / 1e9, 1)
                row[f"tflops_best_{mi}"] = round(fl / min(t[mi]) / 1e9, 1)
            row["speedup_median"] = round(statistics.median(t[32]) / statistics.median(t[16]), 4)
            print(row, flush=True)
            res.append(row)
    finally:
        L.s6d_set_gemm_mfma_shape(0)
    path = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(ROOT, "results", "gemm_shape_ab.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
