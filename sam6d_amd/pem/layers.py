"""Point-transformer layers of the Pose Estimation Model, MI355X build.

Module and attribute names reproduce the reference's state_dict surface
(Pose_Estimation_Model/model/transformer.py) so ``sam-6d-pem-base.pth`` loads unchanged;
the forward passes are re-derived for the hardware rather than transcribed:

  * RPE attention never materialises proj_p(embedding) (B,4,N,M,64): the positional score
    is computed as  (W_p^T q)^T e + q.b_p  -- 64x fewer FLOPs and no 39.7 MB/instance
    intermediate (transformer.py:388-392 computes einsum(q, proj_p(e))).
  * attention cores and the linear-attention tail go through sam6d_amd.ops when a fused
    gfx950 kernel exists (see ops.HAVE) and are expressed with library GEMMs otherwise.
"""
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .. import policy

HEADS = 4


def _plin_weights(owner, lins):
    """(w_hi, w_lo, bias) of one or several nn.Linear with the same input, stacked along the output dim, in the operand format
    of s6d_linear_f32 (bf16 hi / lo parts of the fp32 weight); cached on `owner` until a parameter changes."""
    key = tuple((l.weight._version, l.weight.data_ptr(), l.weight.dtype) +
                ((l.bias._version, l.bias.data_ptr(), l.bias.dtype) if l.bias is not None else (-1, 0, None)) for l in lins)
    name = "_s6d_plin_" + "_".join(str(id(l)) for l in lins)
    c = owner.__dict__.get(name)
    if c is None or c[0] != key:
        with torch.no_grad():
            w = torch.cat([l.weight.detach().float() for l in lins], 0).contiguous()
            b = torch.cat([l.bias.detach().float() if l.bias is not None else w.new_zeros(l.weight.shape[0]) for l in lins]).contiguous()
            hi, lo = ops.split_weight(w)
        c = (key, hi, lo, b)
        owner.__dict__[name] = c
    return c[1], c[2], c[3]


def plinear(owner, lins, x, relu=False, residual=None, norm=None):
    """norm(residual + act(Linear(x))) for the 256-wide fp32 layers: ONE launch of s6d_linear_f32 (split-bf16 matrix cores, fused
    epilogue) when the shapes fit, the library statements otherwise.  `lins`: one nn.Linear or a tuple sharing the input (their
    outputs come back concatenated: q | k | v in one launch).  S6D_DISABLE_FUSED=linear_f32 selects the library path."""
    lins = lins if isinstance(lins, (tuple, list)) else (lins,)
    N = sum(l.weight.shape[0] for l in lins)
    K = lins[0].weight.shape[1]
    if policy.guard("pem.plinear", cuda=x.is_cuda, have=ops.have("linear_f32"), f32=x.dtype == torch.float32, K32=K % 32 == 0,
                    N256=N % 256 == 0, norm_width=norm is None or N == 256, no_grad=not torch.is_grad_enabled()):
        hi, lo, b = _plin_weights(owner, lins)
        x2 = x if x.stride(-1) == 1 and x.is_contiguous() else x.contiguous()
        r2 = None if residual is None else residual.contiguous()
        ln = None if norm is None else (norm.weight.detach(), norm.bias.detach(), norm.eps)
        return ops.linear_f32(x2, hi, lo, b, relu=relu, residual=r2, ln=ln)
    y = torch.cat([l(x) for l in lins], dim=-1) if len(lins) > 1 else lins[0](x)
    if relu:
        y = F.relu(y)
    if residual is not None:
        y = y + residual
    return y if norm is None else norm(y)


def _split(x):  # (B,N,C) -> (B,h,N,c)
    B, N, C = x.shape
    return x.view(B, N, HEADS, C // HEADS).transpose(1, 2)


def _merge(x):  # (B,h,N,c) -> (B,N,C)
    B, h, N, c = x.shape
    return x.transpose(1, 2).reshape(B, N, h * c)


class AttentionOutput(nn.Module):
    """transformer.py:182-197 (ReLU FFN 256->512->256, post-LN)."""

    def __init__(self, d_model):
        super().__init__()
        self.expand = nn.Linear(d_model, d_model * 2)
        self.squeeze = nn.Linear(d_model * 2, d_model)
        self.norm = nn.LayerNorm(d_model)

    def forward(self, x):
        return plinear(self, self.squeeze, plinear(self, self.expand, x, relu=True), residual=x, norm=self.norm)


def _chain_weights(owner, lin):
    """(w_hi, w_lo, bias) of one nn.Linear in the operand format of s6d_attn_output_chain_f32: the split parts of _plin_weights in
    matrix-instruction fragment order; cached on `owner` with the split weights' cache entry as the key."""
    hi, lo, b = _plin_weights(owner, (lin,))
    name = "_s6d_chain_" + str(id(lin))
    c = owner.__dict__.get(name)
    if c is None or c[0] is not hi:
        c = (hi, ops.fragment_weight(hi), ops.fragment_weight(lo), b)
        owner.__dict__[name] = c
    return c[1], c[2], c[3]


def attention_output_chain(layer, output, att, x):
    """``output(layer.norm(layer.linear(att) + x))`` -- what every transformer layer does with its attention core's result
    (transformer.py:182-197 after :200-224 / :409-438 / :567-608) -- as ONE kernel (csrc/s6d_pchain.hip: the strip stays on chip
    from the attention output to the layer output; bit for bit the three plinear launches it replaces), else those launches."""
    if policy.guard("pem.attention_output_chain", cuda=x.is_cuda, have=ops.have("attn_output_chain") and ops.have("linear_f32"),
                    f32=x.dtype == torch.float32 and att.dtype == torch.float32, C256=x.shape[-1] == 256 and att.shape == x.shape,
                    no_grad=not torch.is_grad_enabled()):
        n1, n2 = layer.norm, output.norm
        return ops.attn_output_chain(att, x, _chain_weights(layer, layer.linear), (n1.weight.detach(), n1.bias.detach(), n1.eps),
                                     _chain_weights(output, output.expand), _chain_weights(output, output.squeeze),
                                     (n2.weight.detach(), n2.bias.detach(), n2.eps))
    return output(plinear(layer, layer.linear, att, residual=x, norm=layer.norm))


class MultiHeadAttention(nn.Module):
    """transformer.py:93-148 (no masks / factors are ever passed on the inference path)."""

    def __init__(self, d_model, num_heads=HEADS):
        super().__init__()
        self.proj_q = nn.Linear(d_model, d_model)
        self.proj_k = nn.Linear(d_model, d_model)
        self.proj_v = nn.Linear(d_model, d_model)
        self.scale = 1.0 / math.sqrt(d_model // num_heads)

    def forward(self, xq, xk, xv):
        # (keys: the rows kernel holds a query row's scores in LDS; a longer memory takes the library statements)
        if policy.guard("pem.MultiHeadAttention", cuda=xq.is_cuda, have=ops.have("mha"), C256=xq.shape[-1] == 256,
                        keys=xk.shape[1] <= ops.ATTN_ROWS_MAX_KEYS):
            C = xq.shape[-1]
            q = plinear(self, self.proj_q, xq)
            if xk is xv:                                              # k | v of the memory in one launch
                kv = plinear(self, (self.proj_k, self.proj_v), xk)
                k, v = kv[..., :C], kv[..., C:]                        # column blocks, attended in place (row stride 2 C)
            else:
                k, v = plinear(self, self.proj_k, xk), plinear(self, self.proj_v, xv)
            return ops.mha(q, k, v, self.scale)
        q, k, v = _split(self.proj_q(xq)), _split(self.proj_k(xk)), _split(self.proj_v(xv))
        a = torch.softmax((q @ k.transpose(-1, -2)) * self.scale, dim=-1)
        return _merge(a @ v)


class RPEMultiHeadAttention(nn.Module):
    """transformer.py:352-406 with the proj_p term rewritten (see module docstring)."""

    def __init__(self, d_model, num_heads=HEADS):
        super().__init__()
        self.proj_q = nn.Linear(d_model, d_model)
        self.proj_k = nn.Linear(d_model, d_model)
        self.proj_v = nn.Linear(d_model, d_model)
        self.proj_p = nn.Linear(d_model, d_model)
        self.d_model = d_model
        self.scale = 1.0 / math.sqrt(d_model // num_heads)

    def _fold(self):
        """W_p folded into the q projection (round 4): a Linear-shaped holder of the 1280 x 256 weight whose rows are, per head h,
        the 256 rows of W_p,h^T W_q,h (q~_h = W_p,h^T q_h as a function of x), then the 4 rows b_p,h^T W_q,h (qb_h), then zeros up
        to a whole 256-column tile; biases W_p,h^T b_q,h and b_q,h . b_p,h.  float64 products, cached until a parameter changes."""
        ps = (self.proj_q.weight, self.proj_q.bias, self.proj_p.weight, self.proj_p.bias)
        key = tuple((t._version, t.data_ptr()) for t in ps)
        c = self.__dict__.get("_s6d_fold")
        if c is None or c[0] != key:
            with torch.no_grad():
                C = self.d_model
                c_ = C // HEADS
                wq, bq = self.proj_q.weight.detach().double().view(HEADS, c_, C), self.proj_q.bias.detach().double().view(HEADS, c_)
                wp, bp = self.proj_p.weight.detach().double().view(HEADS, c_, C), self.proj_p.bias.detach().double().view(HEADS, c_)
                w = torch.zeros(HEADS * C + C, C, dtype=torch.float64, device=wq.device)
                b = torch.zeros(HEADS * C + C, dtype=torch.float64, device=wq.device)
                w[:HEADS * C] = torch.einsum("hcj,hck->hjk", wp, wq).reshape(HEADS * C, C)
                b[:HEADS * C] = torch.einsum("hcj,hc->hj", wp, bq).reshape(HEADS * C)
                w[HEADS * C:HEADS * C + HEADS] = torch.einsum("hc,hck->hk", bp, wq)
                b[HEADS * C:HEADS * C + HEADS] = (bp * bq).sum(1)
                lin = torch.nn.Module()
                lin.weight, lin.bias = w.float().contiguous(), b.float().contiguous()
            c = (key, lin)
            self.__dict__["_s6d_fold"] = c
        return c[1]

    def forward(self, x, embed):
        B, N, C = x.shape
        if policy.guard("pem.RPEMultiHeadAttention", cuda=x.is_cuda, have=ops.have("rpe_attention_packed") and ops.have("linear_f32"),
                        f32=x.dtype == torch.float32, C256=C == 256, no_grad=not torch.is_grad_enabled(),
                        keys=N <= ops.ATTN_ROWS_MAX_KEYS, rpe_fold=policy.current().rpe_fold == "1"):
            # q | k | v | q~ | qb from ONE launch of the projection kernel; the attention core reads them in place
            proj = plinear(self, (self.proj_q, self.proj_k, self.proj_v, self._fold()), x)
            return ops.rpe_attention_packed(proj, embed, self.scale)
        qkv = plinear(self, (self.proj_q, self.proj_k, self.proj_v), x)         # q | k | v in one launch
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]             # column blocks, attended in place (row stride 3 C)
        c = C // HEADS
        # q~[b,h,n,:] = W_p[h]^T q[b,h,n,:]   (B,h,N,C);   qb[b,h,n] = q[b,h,n,:] . b_p[h,:]
        qh = _split(q)
        qt = torch.einsum("bhnc,hcj->bhnj", qh, self.proj_p.weight.view(HEADS, c, C))
        qb = torch.einsum("bhnc,hc->bhn", qh, self.proj_p.bias.view(HEADS, c))
        if policy.guard("pem.RPEMultiHeadAttention.core", cuda=x.is_cuda, have=ops.have("rpe_attention"), keys=N <= ops.ATTN_ROWS_MAX_KEYS):
            return ops.rpe_attention(q, k, v, qt, qb, embed, self.scale)
        sp = torch.einsum("bhnj,bnmj->bhnm", qt, embed.float()) + qb.unsqueeze(-1)
        a = torch.softmax((qh @ _split(k).transpose(-1, -2) + sp) * self.scale, dim=-1)
        return _merge(a @ _split(v))


class _AttnLayerBase(nn.Module):
    def __init__(self, attention, d_model):
        super().__init__()
        self.attention = attention
        self.linear = nn.Linear(d_model, d_model)
        self.norm = nn.LayerNorm(d_model)


class AttentionLayer(_AttnLayerBase):
    def __init__(self, d_model):
        super().__init__(MultiHeadAttention(d_model), d_model)

    def forward(self, x, mem):
        return plinear(self, self.linear, self.attention(x, mem, mem), residual=x, norm=self.norm)


class RPEAttentionLayer(_AttnLayerBase):
    def __init__(self, d_model):
        super().__init__(RPEMultiHeadAttention(d_model), d_model)

    def forward(self, x, embed):
        return plinear(self, self.linear, self.attention(x, embed), residual=x, norm=self.norm)


class TransformerLayer(nn.Module):
    def __init__(self, d_model):
        super().__init__()
        self.attention = AttentionLayer(d_model)
        self.output = AttentionOutput(d_model)

    def forward(self, x, mem):
        return attention_output_chain(self.attention, self.output, self.attention.attention(x, mem, mem), x)


class RPETransformerLayer(nn.Module):
    def __init__(self, d_model):
        super().__init__()
        self.attention = RPEAttentionLayer(d_model)
        self.output = AttentionOutput(d_model)

    def forward(self, x, embed):
        return attention_output_chain(self.attention, self.output, self.attention.attention(x, embed), x)


class GeometricTransformer(nn.Module):
    """blocks ['self','cross'], sequential cross-attention (transformer.py:493-513: feats1
    attends to the already-updated feats0)."""

    def __init__(self, d_model):
        super().__init__()
        self.layers = nn.ModuleList([RPETransformerLayer(d_model), TransformerLayer(d_model)])

    def forward(self, f0, e0, f1, e1):
        f0 = self.layers[0](f0, e0)
        f1 = self.layers[0](f1, e1)
        f0 = self.layers[1](f0, f1)
        f1 = self.layers[1](f1, f0)
        return f0, f1


class LinearAttention(nn.Module):
    """Focused linear attention (transformer.py:518-564).  With i=2048 queries and j=196 keys
    the reference takes the kv-first branch (i*j*(c+d) > c*d*(i+j)); this build always does
    (O(N c d), and the branches are algebraically identical)."""

    def __init__(self, d_model, focusing_factor=3):
        super().__init__()
        self.proj_q = nn.Linear(d_model, d_model)
        self.proj_k = nn.Linear(d_model, d_model)
        self.proj_v = nn.Linear(d_model, d_model)
        self.scale = nn.Parameter(torch.zeros(1, 1, d_model))
        self.focusing_factor = focusing_factor

    def _focus(self, t, inv_scale):
        t = (F.relu(t) + 1e-6) * inv_scale
        n = t.norm(dim=-1, keepdim=True)
        t = t ** self.focusing_factor
        return t / t.norm(dim=-1, keepdim=True) * n

    def forward(self, xq, xkv):
        inv_scale = 1.0 / F.softplus(self.scale)
        if policy.guard("pem.LinearAttention.focus", cuda=xq.is_cuda, have=ops.have("linear_attn_focus"), C256=xq.shape[-1] == 256):
            focus = lambda t: ops.linear_attn_focus(t, inv_scale, self.focusing_factor)   # noqa: E731  one fused pass
        else:
            focus = lambda t: self._focus(t, inv_scale)                                    # noqa: E731
        C = xq.shape[-1]
        kv_ = plinear(self, (self.proj_k, self.proj_v), xkv)         # k | v of the memory in one launch
        if policy.guard("pem.LinearAttention", cuda=xq.is_cuda, have=ops.have("linear_attention") and ops.have("linear_attn_focus"),
                        C256=C == 256, f32=xq.dtype == torch.float32):
            # everything behind the projections in two launches (csrc/s6d_linattn.hip): the focus map of q, k^T v, q . sum k, (q kv) z
            # and the head merge; k | v stay the two halves of the one projection output (strided rows)
            return ops.linear_attention(plinear(self, self.proj_q, xq), inv_scale, self.focusing_factor, focus(kv_[..., :C].contiguous()),
                                        kv_[..., C:])
        q = _split(focus(plinear(self, self.proj_q, xq)))            # (B,h,I,c)
        k = _split(focus(kv_[..., :C].contiguous()))                 # (B,h,J,c)
        v = _split(kv_[..., C:])
        z = 1.0 / (q @ k.sum(dim=2).unsqueeze(-1) + 1e-6)            # (B,h,I,1)
        kv = k.transpose(-1, -2) @ v                                 # (B,h,c,d)
        return _merge((q @ kv) * z)


class LinearAttentionLayer(nn.Module):
    def __init__(self, d_model, focusing_factor=3):
        super().__init__()
        self.attention = LinearAttention(d_model, focusing_factor)
        self.linear = nn.Linear(d_model, d_model)
        self.norm = nn.LayerNorm(d_model)

    def forward(self, x, mem):
        return plinear(self, self.linear, self.attention(x, mem), residual=x, norm=self.norm)


class LinearTransformerLayer(nn.Module):
    def __init__(self, d_model, focusing_factor=3):
        super().__init__()
        self.attention = LinearAttentionLayer(d_model, focusing_factor)
        self.output = AttentionOutput(d_model)

    def forward(self, x, mem):
        return attention_output_chain(self.attention, self.output, self.attention.attention(x, mem), x)


class SparseToDenseTransformer(nn.Module):
    """transformer.py:613-673 (with_bg_token, replace_bg_token).  Quirk Q1 is kept on purpose:
    fps_idx addresses the dense tensor WITH the bg token prepended (an off-by-one row gather),
    because the released weights were trained with it."""

    def __init__(self, d_model, focusing_factor=3):
        super().__init__()
        self.sparse_layer = GeometricTransformer(d_model)
        self.dense_layer = LinearTransformerLayer(d_model, focusing_factor)

    @staticmethod
    def _sample(bg, body, fps_idx):
        """The 197-token sparse set: [bg token | rows fps_idx of the bg-prepended dense tensor] (Quirk Q1: index i addresses
        row i of [bg | body], so i = 0 -- FPS always picks it first -- is the bg token again and i > 0 is body row i - 1),
        without materialising the (B, 1 + N, C) concatenation."""
        i = fps_idx.long()
        g = ops.gather_rows(body, (i - 1).clamp(min=0).to(fps_idx.dtype))
        g = torch.where((i == 0).unsqueeze(-1), bg.expand(-1, g.shape[1], -1), g)
        return torch.cat([bg, g], dim=1)

    def forward(self, d0, e0, idx0, d1, e1, idx1):
        """d0 / d1: the dense features with the bg token at row 0, either as ONE (B, 1 + N, C) tensor (the reference's form; the
        result is then one tensor too) or as a pair (bg (B,1,C), body (B,N,C)): FinePointMatching passes pairs so that the three
        blocks do not copy 67 MB per side and block through torch.cat just to prepend one row (round 2: 0.4 ms per cat)."""
        pair = isinstance(d0, (tuple, list))
        (b0, x0), (b1, x1) = (d0, d1) if pair else ((d0[:, 0:1], d0[:, 1:].contiguous()), (d1[:, 0:1], d1[:, 1:].contiguous()))
        s0, s1 = self._sample(b0, x0.contiguous(), idx0), self._sample(b1, x1.contiguous(), idx1)
        s0, s1 = self.sparse_layer(s0, e0, s1, e1)
        n0 = (s0[:, 0:1], self.dense_layer(x0, s0[:, 1:]))
        n1 = (s1[:, 0:1], self.dense_layer(x1, s1[:, 1:]))
        return (n0, n1) if pair else (torch.cat(n0, dim=1), torch.cat(n1, dim=1))


class SinusoidalPositionalEmbedding(nn.Module):
    """transformer.py:257-281; only the ``div_term`` buffer is part of the checkpoint."""

    def __init__(self, d_model):
        super().__init__()
        self.d_model = d_model
        div = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
        self.register_buffer("div_term", div)

    def forward(self, x):
        om = x.unsqueeze(-1) * self.div_term
        return torch.stack([torch.sin(om), torch.cos(om)], dim=-1).reshape(*x.shape, self.d_model)


_GEO_DTYPE_DEFAULT = "fp32"


class GeometricStructureEmbedding(nn.Module):
    """transformer.py:286-349.  cfg: sigma_d, sigma_a, angle_k, reduction_a, hidden_dim."""

    def __init__(self, cfg):
        super().__init__()
        self.sigma_d = cfg.sigma_d
        self.sigma_a = cfg.sigma_a
        self.factor_a = 180.0 / (self.sigma_a * math.pi)
        self.angle_k = cfg.angle_k
        self.embedding = SinusoidalPositionalEmbedding(cfg.hidden_dim)
        self.proj_d = nn.Linear(cfg.hidden_dim, cfg.hidden_dim)
        self.proj_a = nn.Linear(cfg.hidden_dim, cfg.hidden_dim)
        self.reduction_a = cfg.reduction_a
        if self.reduction_a != "max":
            raise ValueError("MI355X build implements reduction_a == 'max' (config/base.yaml:30)")

    def _split_weights(self):
        """(W_d, W_a) as [hi | lo] bf16 parts for s6d_geo_embedding_split, cached until a weight changes (round 5: every workgroup
        of the kernel used to split both matrices again in each of its eight k-steps)."""
        if not (ops.have("geo_embedding_split") and policy.current().geo_presplit == "1"):
            return None
        ws = (self.proj_d.weight, self.proj_a.weight)
        key = tuple((w._version, w.data_ptr(), w.dtype) for w in ws)
        c = self.__dict__.get("_s6d_geo_split")
        if c is None or c[0] != key:
            with torch.no_grad():
                parts = tuple(torch.stack(ops.split_weight(w.detach().float().contiguous())).contiguous() for w in ws)
            c = (key, parts)
            self.__dict__["_s6d_geo_split"] = c
        return c[1]

    @torch.no_grad()
    def get_embedding_indices(self, points):
        B, N, _ = points.shape
        k = self.angle_k
        diff = points.unsqueeze(1) - points.unsqueeze(2)                      # [b,n,m] = p_m - p_n
        xy = points @ points.transpose(1, 2)
        sq = (points ** 2).sum(-1)
        dist = torch.sqrt((sq.unsqueeze(-1) - 2 * xy + sq.unsqueeze(-2)).clamp(min=0.0))
        knn = dist.topk(k=k + 1, dim=2, largest=False)[1][:, :, 1:]           # (B,N,k)
        ref = torch.gather(diff, 2, knn.unsqueeze(-1).expand(B, N, k, 3))     # nbr(n) - p_n
        ref = ref.unsqueeze(2).expand(B, N, N, k, 3)
        anc = diff.unsqueeze(3).expand(B, N, N, k, 3)
        sin_v = torch.linalg.norm(torch.cross(ref, anc, dim=-1), dim=-1)
        cos_v = (ref * anc).sum(-1)
        return dist / self.sigma_d, torch.atan2(sin_v, cos_v) * self.factor_a

    def forward(self, points):
        if policy.guard("pem.GeometricStructureEmbedding", cuda=points.is_cuda, have=ops.have("geo_embedding"), angle_k3=self.angle_k == 3,
                        C256=self.proj_d.weight.shape[0] == 256):
            # S6D_PEM_GEO_DTYPE=fp16: the embedding is STORED in IEEE half (same arithmetic up to the store); its twelve readers
            # (rpe_attention_kernel, bound by streaming it) then move half the bytes.  Measured margins: DESIGN.md 4.
            half = policy.current().pem_geo_dtype == "fp16" and ops.have("geo_embedding_f16")
            weights = (self.proj_d.weight.contiguous(), self.proj_d.bias, self.proj_a.weight.contiguous(), self.proj_a.bias,
                       self.embedding.div_term.contiguous())
            kw = dict(out_dtype=torch.float16 if half else torch.float32, split=self._split_weights())
            # S6D_GEO_FROM_POINTS=1 (default): the index stage runs inside the kernels (pair distances by direct differences, neighbour
            # ties to the lower index) -- no idx4, no (B,N,N,3,3) temporaries, no library launches; "0": the statements below
            # Clouds outside what those kernels serve (N, dtype) keep the path through idx4 as before, strict mode included: a plain `if`,
            # not a guard -- only a library without the entry points is a recorded fall-back.
            served = points.dtype == torch.float32 and points.dim() == 3 and 4 <= points.shape[1] <= ops.GEO_POINTS_MAX_N
            if policy.current().geo_from_points == "1" and served and policy.guard(
                    "pem.GeometricStructureEmbedding.from_points", cuda=points.is_cuda, have=ops.have("geo_embedding_points")):
                return ops.geo_embedding_points(points.contiguous(), self.sigma_d, self.factor_a, *weights, **kw)
            d_idx, a_idx = self.get_embedding_indices(points)
            idx4 = torch.cat([d_idx.unsqueeze(-1), a_idx], dim=-1).contiguous()          # (B,N,N,4)
            return ops.geo_embedding(idx4, *weights, **kw)
        outs = []
        for p in points.split(4, dim=0):     # bound the (b,N,N,k,256) intermediate of the library path
            d_idx, a_idx = self.get_embedding_indices(p)
            d = self.proj_d(self.embedding(d_idx))
            a = self.proj_a(self.embedding(a_idx)).max(dim=3)[0]
            outs.append(d + a)
        return torch.cat(outs, 0)
