"""The residual-stream block loop of the three ViTs on the hot path (SAM ViT-H, DINOv2 ViT-L, PEM ViT-B), once.

A model file chooses the form (its own conditions and policy.guard sites) and describes each of its blocks as a BlockView; the
runners below own the order of the launches.  Forms, per block:
  lnfold           row_stats -> gemm_bf16_lnfold -> attention -> gemm_bf16(residual, stats_partial) -> ln_stats_finalize ->
                   gemm_bf16_lnfold(gelu) -> gemm_bf16(residual, stats_partial): neither the adds nor the LayerNorms are passes
  add_layernorm    residual=True: one-read LayerNorm passes, both adds in the epilogues of the proj / fc2 GEMMs;
                   residual=False (round 2; the only form an fp16 stream can take): each add folded into the next LayerNorm pass
  fp8              the LayerNorm-fed GEMMs (qkv, fc1 + GELU) on the fp8 matrix cores; mx: fc2 too, fed by fc1's MX-scaled e4m3
A tap and a model's final norm are the same statement (`tap`): LayerNorm of the stream, taking the pending delta with it."""
import torch

from .. import ops
from . import fp8 as _fp8
from .linear import lnfold_cached


def ln_f32(norm):
    """fp32 copies of a LayerNorm's affine parameters, cached until the parameters change."""
    key = (norm.weight._version, norm.bias._version, norm.weight.data_ptr())
    c = getattr(norm, "_s6d_f32", None)
    if c is None or c[0] != key:
        c = (key, norm.weight.detach().float().contiguous(), norm.bias.detach().float().contiguous())
        norm._s6d_f32 = c
    return c[1], c[2]


class BlockView:
    """One transformer block as the runners see it: small and dumb, made per call.  A model file subclasses it and defines what
    its forms use:
      fc1                         the Linear behind norm2 (norm1, norm2 and qkv carry the same names in the three models)
      proj(), fc2()               -> (weight in the stream's dtype, fp32 bias) of the two Linear layers that feed the stream
      fc2_fp8()                   -> (e4m3 weight bytes, per-channel scales, fp32 bias) of fc2
      attention(qkv)              the attention kernel on the qkv GEMM's output -> (rows, C)
      attn(h, residual=None)      the whole attention branch on the normed tokens, as the module states it (add + LayerNorm forms;
                                  qkv=: the projection is made already, the fp8 loop without residual GEMMs)
      mlp(h, residual=None)       the whole MLP branch; residual: the stream, updated in place by the last GEMM's epilogue
      fc2_linear(h)               fc2 as the module states it (the fp8 loop without residual GEMMs)"""
    norm1 = property(lambda self: self.blk.norm1)
    norm2 = property(lambda self: self.blk.norm2)
    qkv = property(lambda self: self.blk.attn.qkv)

    def __init__(self, blk, shape):
        self.blk, self.shape = blk, shape                            # shape: the token stream's


def tap(x, delta, norm):
    """(x + delta, norm(x + delta)): a tap of the stream, or a model's final norm; delta None: x itself comes back."""
    g, b = ln_f32(norm)
    return ops.add_layernorm(x, delta, g, b, norm.eps)


def lnfold(x, views):
    """x (..., C): this call's own stream tensor, updated in place.  `x + proj(..)` and `x + fc2(..)`: the residual tile rides through
    the matrix cores of the producing GEMM (s6d_gemm_bf16_res), whose epilogue also leaves per-row partial statistics of the new x;
    s6d_ln_stats_finalize turns them into (mean, sigma) per token, and the consuming GEMM (qkv, fc1 + GELU) multiplies the RAW stream
    by gamma * W, starting its accumulators at sigma b' - mean s and dividing by sigma in its epilogue (s6d_gemm_bf16_lnfold).  The
    normalised activations never exist.  The last block leaves no statistics: nothing reads them."""
    if not views:
        return x
    C = x.shape[-1]
    x2 = x.view(-1, C)
    st = ops.row_stats(x2, views[0].norm1.eps)
    sp = torch.empty(C // 32, 2, x2.shape[0], dtype=torch.float32, device=x.device)
    for i, v in enumerate(views):
        qkv = ops.gemm_bf16_lnfold(x2, st, *lnfold_cached(v.qkv, v.norm1))
        ops.gemm_bf16(v.attention(qkv), *v.proj(), residual=x2, out=x2, stats_partial=sp)
        st = ops.ln_stats_finalize(sp, 32, v.norm2.eps)
        h = ops.gemm_bf16_lnfold(x2, st, *lnfold_cached(v.fc1, v.norm2), gelu=True)
        last = i + 1 == len(views)
        ops.gemm_bf16(h, *v.fc2(), residual=x2, out=x2, stats_partial=None if last else sp)
        if not last:
            st = ops.ln_stats_finalize(sp, 32, views[i + 1].norm1.eps)
    return x


def add_layernorm(x, views, residual, taps=(), norm=None):
    """-> (x, pending delta or None, [norm(stream) after each block in `taps`]).  residual=True: x is this call's own tensor and the
    branches add into it; residual=False: x is only read, a branch's output joins the stream in the next LayerNorm pass."""
    delta, out = None, []
    for i, v in enumerate(views):
        g, b = ln_f32(v.norm1)
        x, h = ops.add_layernorm(x, delta, g, b, v.norm1.eps)
        g, b = ln_f32(v.norm2)
        if residual:
            x = v.attn(h, residual=x)
            _, h = ops.add_layernorm(x, None, g, b, v.norm2.eps)
            x = v.mlp(h, residual=x)
        else:
            x, h = ops.add_layernorm(x, v.attn(h).contiguous(), g, b, v.norm2.eps)
            delta = v.mlp(h).contiguous()
        if i in taps:
            x, t = tap(x, delta, norm)
            delta = None
            out.append(t)
    return x, delta, out


def fp8(x, views, mx, residual):
    """-> (x, pending delta or None).  LayerNorm writes its output as e4m3 bytes with one power-of-two scale per token
    (s6d_layernorm_fp8: no extra pass), the weights carry one per output channel (utils/fp8.py), both ride in the matrix
    instruction's block-scale operands (s6d_gemm_fp8).  residual=True: x is this call's own tensor; proj and fc2 stay bf16 with the
    add in their epilogue, so the quantising LayerNorm reads ONE tensor.  mx: fc1's GELU epilogue writes e4m3 with MX block scales
    (one E8M0 byte per token and 32 channels) and fc2 multiplies them on the fp8 matrix cores -- the hidden activations never exist in
    bf16; that kernel has no registers left for the residual epilogue, so fc2's output is a bf16 delta that the next quantising
    LayerNorm adds (s6d_add_layernorm_fp8, which returns a new stream tensor).  residual=False: every add goes that way."""
    C = x.shape[-1]
    x2 = x.view(-1, C)
    delta = None
    for v in views:
        g, b = ln_f32(v.norm1)
        if delta is None:
            h8, hs = ops.layernorm_fp8(x, g, b, v.norm1.eps)
        else:
            x, h8, hs = ops.layernorm_fp8(x, g, b, v.norm1.eps, delta=delta)
            x2 = x.view(-1, C)
        qkv = ops.gemm_fp8(h8, hs, *_fp8.cached_weight(v.qkv))
        g, b = ln_f32(v.norm2)
        if residual:
            ops.gemm_bf16(v.attention(qkv), *v.proj(), residual=x2, out=x2)
            h8, hs = ops.layernorm_fp8(x, g, b, v.norm2.eps)
        else:
            x, h8, hs = ops.layernorm_fp8(x, g, b, v.norm2.eps, delta=v.attn(x, qkv=qkv).contiguous())
        w1 = _fp8.cached_weight(v.fc1)
        if mx:
            delta = ops.gemm_fp8_mxa(*ops.gemm_fp8_gelu_mx(h8, hs, *w1), *v.fc2_fp8()).view(x.shape)
        elif residual:
            ops.gemm_bf16(ops.gemm_fp8(h8, hs, *w1, gelu=True), *v.fc2(), residual=x2, out=x2)
        else:
            delta = v.fc2_linear(ops.gemm_fp8(h8, hs, *w1, gelu=True)).contiguous()
    return x, delta
