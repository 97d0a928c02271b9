"""Thin torch-tensor front-end of the C ABI (include/sam6d_hip.h).

torch is plumbing here: device memory, the current HIP stream and dtype/shape checks.
Every function enqueues hand-written gfx950 kernels on torch's current stream and
returns freshly allocated outputs; none of them has a CPU implementation.
"""
import ctypes

import torch

from . import _lib
from . import policy


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()          # an optional operand that is left out (None) goes as NULL


def _float3(values):
    return (ctypes.c_float * 3)(*[float(v) for v in values])          # a host-side `const float[3]` operand (per-channel mean / std)


def _chk(t, dtype, name, ndim=None):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")  # same wording as the reference's CHECK_CUDA
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous tensor")
    if t.dtype != dtype:
        kind = {torch.float32: "a float", torch.int32: "an int", torch.bfloat16: "a bfloat16"}.get(dtype, str(dtype))
        raise RuntimeError(f"{name} must be {kind} tensor")
    if ndim is not None and t.dim() != ndim:
        raise RuntimeError(f"{name} must have {ndim} dimensions")


def _fn(fn_name, nargs):
    """The entry point under the prototype include/sam6d_hip.h declares for it (attached once per function object: a library a test
    puts in _lib._lib is bound as it is used).  ctypes then converts plain values and refuses what does not fit; it lets surplus
    arguments through, so the count is checked here."""
    fn = getattr(_lib.lib(), fn_name, None)
    if fn is None or fn.argtypes is None:
        fn = _lib.bind(_lib.lib(), fn_name)
    if nargs != len(fn.argtypes):
        raise TypeError(f"{fn_name} takes {len(fn.argtypes)} arguments ({nargs} given)")
    return fn


def _call(fn_name, *args):
    _lib.check(_fn(fn_name, len(args))(*args), fn_name)


def _size(fn_name, *args):
    return _fn(fn_name, len(args))(*args)          # the `long s6d_*_workspace_bytes / _floats / _scratch_bytes` functions


# ------------------------------------------------------------------ PointNet++ ops
def furthest_point_sampling(points, nsamples):
    """(B,N,3) f32 -> (B,nsamples) i32   [pointnet2._ext.furthest_point_sampling]"""
    _chk(points, torch.float32, "points", 3)
    B, N, _ = points.shape
    out = torch.empty(B, nsamples, dtype=torch.int32, device=points.device)
    tmp = torch.empty(B, N, dtype=torch.float32, device=points.device) if N > 4096 else None
    _call("s6d_fps_f32", _ptr(points), B, N, nsamples, _ptr(tmp), _ptr(out), _stream())
    return out


def gather_points(points, idx):
    """(B,C,N) f32, (B,M) i32 -> (B,C,M)   [pointnet2._ext.gather_points]"""
    _chk(points, torch.float32, "points", 3)
    _chk(idx, torch.int32, "idx", 2)
    B, C, N = points.shape
    M = idx.shape[1]
    out = torch.empty(B, C, M, dtype=torch.float32, device=points.device)
    _call("s6d_gather_points_f32", _ptr(points), _ptr(idx), B, C, N, M, _ptr(out), _stream())
    return out


def gather_rows(src, idx):
    """(B,N,C) f32, (B,M) i32 -> (B,M,C)."""
    _chk(src, torch.float32, "src", 3)
    _chk(idx, torch.int32, "idx", 2)
    B, N, C = src.shape
    M = idx.shape[1]
    out = torch.empty(B, M, C, dtype=torch.float32, device=src.device)
    _call("s6d_gather_rows_f32", _ptr(src), _ptr(idx), B, N, C, M, _ptr(out), _stream())
    return out


def ball_query(new_xyz, xyz, radius, nsample):
    """(B,M,3), (B,N,3) -> (B,M,nsample) i32   [pointnet2._ext.ball_query]"""
    _chk(new_xyz, torch.float32, "new_xyz", 3)
    _chk(xyz, torch.float32, "xyz", 3)
    B, M, _ = new_xyz.shape
    N = xyz.shape[1]
    out = torch.empty(B, M, int(nsample), dtype=torch.int32, device=xyz.device)
    _call("s6d_ball_query_f32", _ptr(new_xyz), _ptr(xyz), B, N, M, radius, int(nsample), _ptr(out), _stream())
    return out


def group_points(points, idx):
    """(B,C,N) f32, (B,M,S) i32 -> (B,C,M,S)   [pointnet2._ext.group_points]"""
    _chk(points, torch.float32, "points", 3)
    _chk(idx, torch.int32, "idx", 3)
    B, C, N = points.shape
    _, M, S = idx.shape
    out = torch.empty(B, C, M, S, dtype=torch.float32, device=points.device)
    _call("s6d_group_points_f32", _ptr(points), _ptr(idx), B, C, N, M, S, _ptr(out), _stream())
    return out


# ------------------------------------------------------------------ PEM pose solvers
def rot_from_h(H):
    """(...,3,3) f32 cross-covariances -> proper rotations (Procrustes)."""
    _chk(H, torch.float32, "H")
    n = H.numel() // 9
    out = torch.empty_like(H)
    _call("s6d_rot_from_h_f32", _ptr(H), n, _ptr(out), _stream())
    return out


def weighted_procrustes(src, ref, weights, weight_thresh=0.0, eps=1e-5):
    """src, ref (B,N,3), weights (B,N) f32 -> R (B,3,3), t (B,3): ref ~ src R^T + t (batch-size independent, fixed order)."""
    _chk(src, torch.float32, "src", 3)
    _chk(ref, torch.float32, "ref", 3)
    _chk(weights, torch.float32, "weights", 2)
    B, N, _ = src.shape
    if ref.shape != src.shape or weights.shape != (B, N):
        raise ValueError(f"weighted_procrustes: src {tuple(src.shape)}, ref {tuple(ref.shape)}, weights {tuple(weights.shape)}")
    R = torch.empty(B, 3, 3, dtype=torch.float32, device=src.device)
    t = torch.empty(B, 3, dtype=torch.float32, device=src.device)
    _call("s6d_weighted_procrustes_f32", _ptr(src), _ptr(ref), _ptr(weights), B, N, weight_thresh, eps, _ptr(R), _ptr(t), _stream())
    return R, t


def pose_hypotheses(pts1, pts2, pair):
    """pts1 (B,N1,3), pts2 (B,N2,3) f32, pair (B,3*n) i32 -> R (B,n,3,3), t (B,n,3), dis (B,n)."""
    _chk(pts1, torch.float32, "pts1", 3)
    _chk(pts2, torch.float32, "pts2", 3)
    _chk(pair, torch.int32, "pair", 2)
    B, N1, _ = pts1.shape
    N2 = pts2.shape[1]
    n = pair.shape[1] // 3
    R = torch.empty(B, n, 3, 3, dtype=torch.float32, device=pts1.device)
    t = torch.empty(B, n, 3, dtype=torch.float32, device=pts1.device)
    dis = torch.empty(B, n, dtype=torch.float32, device=pts1.device)
    _call("s6d_pose_hypotheses_f32", _ptr(pts1), _ptr(pts2), _ptr(pair), B, N1, N2, n, _ptr(R), _ptr(t), _ptr(dis), _stream())
    return R, t, dis


def cosine_similarity(f1, f2, temp):
    """f1 (B,M1,C), f2 (B,M2,C) f32 -> atten (B,M1,M2) f32 = normalize(f1) @ normalize(f2)^T / temp (compute_feature_similarity,
    cosine) in one launch with a fixed accumulation order per instance: the bits of an instance do not depend on the batch."""
    _chk(f1, torch.float32, "f1", 3)
    _chk(f2, torch.float32, "f2", 3)
    B, M1, C = f1.shape
    M2 = f2.shape[1]
    if f2.shape[0] != B or f2.shape[2] != C:
        raise ValueError(f"cosine_similarity: f1 {tuple(f1.shape)} and f2 {tuple(f2.shape)} must agree in B and C")
    atten = torch.empty(B, M1, M2, dtype=torch.float32, device=f1.device)
    _call("s6d_cosine_similarity_f32", _ptr(f1), _ptr(f2), B, M1, M2, C, float(temp), _ptr(atten), _stream())
    return atten


def coarse_sample(atten, rand_u):
    """atten (B,M1,M2) f32, rand_u (B,n_u) f32 -> pair (B,n_u) i32 (flat bin index), w1 (B,M1-1) f32."""
    _chk(atten, torch.float32, "atten", 3)
    _chk(rand_u, torch.float32, "rand_u", 2)
    B, M1, M2 = atten.shape
    pair = torch.empty(B, rand_u.shape[1], dtype=torch.int32, device=atten.device)
    w1 = torch.empty(B, M1 - 1, dtype=torch.float32, device=atten.device)
    _call("s6d_coarse_sample_f32", _ptr(atten), _ptr(rand_u), B, M1, M2, rand_u.shape[1], _ptr(pair), _ptr(w1), _stream())
    return pair, w1


def smallest_k(dis, Rs, ts, k):
    """dis (B,n), Rs (B,n,3,3), ts (B,n,3) f32 -> Rk (B,k,3,3), tk (B,k,3), idx (B,k) i32: the k smallest, ascending."""
    _chk(dis, torch.float32, "dis", 2)
    _chk(Rs, torch.float32, "Rs", 4)
    _chk(ts, torch.float32, "ts", 3)
    B, n = dis.shape
    Rk = torch.empty(B, k, 3, 3, dtype=torch.float32, device=dis.device)
    tk = torch.empty(B, k, 3, dtype=torch.float32, device=dis.device)
    idx = torch.empty(B, k, dtype=torch.int32, device=dis.device)
    _call("s6d_smallest_k_f32", _ptr(dis), _ptr(Rs), _ptr(ts), B, n, k, _ptr(Rk), _ptr(tk), _ptr(idx), _stream())
    return Rk, tk, idx


def hypothesis_select(dmin, w1, Rk, tk):
    """dmin (B,P,N), w1 (B,N), Rk (B,P,3,3), tk (B,P,3) f32 -> R (B,3,3), t (B,3) of the best-scoring hypothesis."""
    for a, nm, nd in ((dmin, "dmin", 3), (w1, "w1", 2), (Rk, "Rk", 4), (tk, "tk", 3)):
        _chk(a, torch.float32, nm, nd)
    B, P, N = dmin.shape
    R = torch.empty(B, 3, 3, dtype=torch.float32, device=dmin.device)
    t = torch.empty(B, 3, dtype=torch.float32, device=dmin.device)
    _call("s6d_hypothesis_select_f32", _ptr(dmin), _ptr(w1), _ptr(Rk), _ptr(tk), B, P, N, _ptr(R), _ptr(t), _stream())
    return R, t


def min_dist(pts, R, t, model):
    """pts (B,N,3), R (B,P,3,3), t (B,P,3), model (B,Nm,3) -> (B,P,N)."""
    for a, nm, nd in ((pts, "pts", 3), (R, "R", 4), (t, "t", 3), (model, "model", 3)):
        _chk(a, torch.float32, nm, nd)
    B, N, _ = pts.shape
    P, Nm = R.shape[1], model.shape[1]
    out = torch.empty(B, P, N, dtype=torch.float32, device=pts.device)
    _call("s6d_min_dist_f32", _ptr(pts), _ptr(R), _ptr(t), _ptr(model), B, N, P, Nm, _ptr(out), _stream())
    return out


# ------------------------------------------------------------------ PEM point transformer
def _rows3(t, name):
    """(B, N, 256) f32 with unit channel stride whose rows sit at a constant stride (a column block of a wider contiguous (B, N, L)
    tensor qualifies) -> (tensor, row stride); anything else is made contiguous."""
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 3:
        raise RuntimeError(f"{name} must be a 3-d float32 CUDA tensor")
    B, N, C = t.shape
    if t.stride(2) == 1 and t.stride(1) % 4 == 0 and t.stride(1) >= C and (B == 1 or t.stride(0) == N * t.stride(1)) \
            and t.data_ptr() % 16 == 0:
        return t, t.stride(1)
    t = t.contiguous()
    return t, C


ATTN_ROWS_MAX_KEYS = 1024      # keys the rows kernel serves (csrc/s6d_rpe.hip: a workgroup's 4 waves x 4 heads x 4 B of scores per key, rounded
#                                up to four keys, in 64 KiB of LDS); beyond it s6d_rpe_attention_* / s6d_mha_* return S6D_EUNSUPPORTED


def rpe_attention(q, k, v, qt, qb, embed, scale):
    """q,k,v (B,N,256) (column blocks of one projection output are taken as they are); qt (B,4,N,256); qb (B,4,N);
    embed (B,N,N,256) -> (B,N,256), all f32."""
    (q, ldq), (k, ldk), (v, ldv) = _rows3(q, "q"), _rows3(k, "k"), _rows3(v, "v")
    qt, qb = qt.contiguous(), qb.contiguous()
    for a, nm in ((qt, "qt"), (qb, "qb")):
        _chk(a, torch.float32, nm)
    _chk(embed, embed.dtype if embed.dtype == torch.float16 else torch.float32, "embed", 4)
    B, N, C = q.shape
    out = torch.empty(B, N, C, dtype=torch.float32, device=q.device)
    _call("s6d_rpe_attention_strided_e16_f32" if embed.dtype == torch.float16 else "s6d_rpe_attention_strided_f32", _ptr(q), ldq, _ptr(k),
          ldk, _ptr(v), ldv, _ptr(qt), _ptr(qb), _ptr(embed), B, N, C, 4, scale, _ptr(out), _stream())
    return out


def rpe_attention_packed(proj, embed, scale, q_off=0, k_off=256, v_off=512, qt_off=768, qb_off=1792):
    """rpe_attention on ONE projection output proj (B,N,ld) f32 holding q | k | v | q~ (4 x 256) | qb (4) as column blocks (W_p folded
    into the projection's weights by the caller) -> (B,N,256) f32."""
    _chk(proj, torch.float32, "proj", 3)
    _chk(embed, embed.dtype if embed.dtype == torch.float16 else torch.float32, "embed", 4)
    B, N, ld = proj.shape
    out = torch.empty(B, N, 256, dtype=torch.float32, device=proj.device)
    _call("s6d_rpe_attention_packed_e16_f32" if embed.dtype == torch.float16 else "s6d_rpe_attention_packed_f32", _ptr(proj), ld,
          int(q_off), int(k_off), int(v_off), int(qt_off), int(qb_off), _ptr(embed), B, N, 256, 4, scale, _ptr(out), _stream())
    return out


# ------------------------------------------------------------------ edges of the path
def sam_preprocess(x, mean, std, img_size, out_dtype=torch.bfloat16):
    """(B,3,h,w) f32 -> (B,3,S,S) normalised + zero padded, in `out_dtype` (bf16 or f32).  [Sam.preprocess]"""
    _chk(x, torch.float32, "x", 4)
    B, C, h, w = x.shape
    if C != 3:
        raise RuntimeError("x must have 3 channels")
    out = torch.empty(B, 3, img_size, img_size, dtype=out_dtype, device=x.device)
    _call("s6d_sam_preprocess_f32", _ptr(x), B, h, w, int(img_size), _float3(mean), _float3(std), 1 if out_dtype == torch.bfloat16 else 0,
          _ptr(out), _stream())
    return out


def nonfinite_rows(x):
    """x (B, ...) f32 contiguous -> (B,) bool: does instance b hold an inf or a NaN?  One read of x."""
    _chk(x, torch.float32, "x")
    B = x.shape[0]
    n = x.numel() // max(B, 1)
    flags = torch.empty(B, dtype=torch.int32, device=x.device)
    _call("s6d_nonfinite_rows_f32", _ptr(x), B, n, _ptr(flags), _stream())
    return flags.bool()


def im2col3x3(y):
    """(B,H,W,C) bf16 / f16 -> (B,H,W,9C): the nine shifted views of a zero-padded 3x3 neighbourhood in (dy, dx, c) order -- the A
    operand of a padding-1 3x3 convolution as one GEMM.  [the SAM neck's second Conv2d, image_encoder.py:91-97]"""
    if y.dtype not in (torch.bfloat16, torch.float16) or y.dim() != 4 or not y.is_contiguous():
        raise RuntimeError("im2col3x3: contiguous (B,H,W,C) bf16 / f16 expected")
    B, H, W, C = y.shape
    out = torch.empty(B, H, W, 9 * C, dtype=y.dtype, device=y.device)
    _call("s6d_im2col3x3_b16", _ptr(y), B, H, W, C, _ptr(out), _stream())
    return out


def patchify(x, p):
    """(B,Cin,H,W) bf16 / f16 -> (B,H/p,W/p,Cin*p*p) with a patch's elements in (c, dy, dx) order (Conv2d.weight.flatten(1)'s):
    the A operand of a kernel = stride = p convolution.  [PatchEmbed.forward, image_encoder.py:375-395]"""
    if x.dtype not in (torch.bfloat16, torch.float16) or x.dim() != 4 or not x.is_contiguous():
        raise RuntimeError("patchify: contiguous (B,Cin,H,W) bf16 / f16 expected")
    B, Cin, H, W = x.shape
    out = torch.empty(B, H // p, W // p, Cin * p * p, dtype=x.dtype, device=x.device)
    _call("s6d_patchify_b16", _ptr(x), B, Cin, H, W, int(p), _ptr(out), _stream())
    return out


def crop_resize_pad(image_u8, masks, params, target, mean, std, rgb=True, mask=True):
    """Fused proposal crops [CustomDINOv2.process_rgb_proposals / process_masks_proposals].
    image_u8 (H,W,3) uint8, masks (P,H,W) f32, params (P,12) int32 records (sam6d_amd.ism.dinov2.crop_params)
    -> (rgbs (P,3,T,T) f32 or None, masks (P,T,T) f32 or None)."""
    _chk(masks, torch.float32, "masks", 3)
    _chk(params, torch.int32, "params", 2)
    P, H, W = masks.shape
    if rgb:
        _chk(image_u8, torch.uint8, "image", 3)
        if tuple(image_u8.shape) != (H, W, 3):
            raise RuntimeError("crop_resize_pad: image must be (H,W,3) like the masks")
    if tuple(params.shape) != (P, 12):
        raise RuntimeError("crop_resize_pad: params must be (P,12)")
    T = int(target)
    o_rgb = torch.empty(P, 3, T, T, dtype=torch.float32, device=masks.device) if rgb else None
    o_mask = torch.empty(P, T, T, dtype=torch.float32, device=masks.device) if mask else None
    _call("s6d_crop_resize_pad_f32", _ptr(image_u8) if rgb else None, _ptr(masks), _ptr(params), P, H, W, T, _float3(mean), _float3(std),
          _ptr(o_rgb), _ptr(o_mask), _stream())
    return o_rgb, o_mask


def samdec_img2tok(q, q_add, kexp, vpt, resid, out_bias, ln_w, ln_b, eps, n_tok):
    """Image->token cross attention + folded out_proj + residual + LayerNorm of SAM's two-way block.
    q (1|B,N,128) bf16 (last-dim slice of a wider tensor allowed), q_add (N,128) bf16 or None, kexp (B,64,128) bf16,
    vpt (B,256,64) bf16, resid (1|B,N,256) bf16 -> (B,N,256) bf16."""
    B, N = kexp.shape[0], resid.shape[1]
    for t, nm in ((kexp, "kexp"), (vpt, "vpt"), (resid, "resid")):
        _chk(t, torch.bfloat16, nm, 3)
    for t, nm in ((out_bias, "out_bias"), (ln_w, "ln_w"), (ln_b, "ln_b")):
        _chk(t, torch.float32, nm, 1)
    if q.dtype != torch.bfloat16 or q.dim() != 3 or q.shape[-1] != 128 or q.stride(2) != 1 or not q.is_cuda:
        raise RuntimeError("q must be a (.,N,128) bfloat16 CUDA tensor with unit channel stride")
    q_ld = q.stride(1)
    if q.shape[0] > 1 and q.stride(0) != N * q_ld:
        raise RuntimeError("q batch stride must be N * row stride")
    if q_add is not None:
        _chk(q_add, torch.bfloat16, "q_add", 2)
    if tuple(kexp.shape) != (B, 64, 128) or tuple(vpt.shape) != (B, 256, 64) or resid.shape[2] != 256 or q.shape[1] != N:
        raise RuntimeError("samdec_img2tok: shape mismatch")
    out = torch.empty(B, N, 256, dtype=torch.bfloat16, device=kexp.device)
    _call("s6d_samdec_img2tok_bf16", _ptr(q), _ptr(q_add), _ptr(kexp), _ptr(vpt), _ptr(resid), _ptr(out_bias), _ptr(ln_w), _ptr(ln_b), eps,
          B, N, int(n_tok), q_ld, 1 if q.shape[0] == 1 and B > 1 else 0, 1 if resid.shape[0] == 1 and B > 1 else 0, _ptr(out), _stream())
    return out


def samdec_img2tok_raw(x, pe, kexp256, cbias, vpt, resid, out_bias, ln_w, ln_b, eps, n_tok):
    """samdec_img2tok with the q projection folded into the expanded keys: x (1|B,N,256) bf16 RAW image tokens, pe (N,256) bf16 or
    None (added to x for the scores), kexp256 (B,64,256) bf16 = kexp_128 @ W_q, cbias (B,64) f32 = kexp_128 @ b_q, vpt (B,256,64) bf16,
    resid (1|B,N,256) bf16 -> (B,N,256) bf16.  The projected queries of the B x N image tokens are never written."""
    B, N = kexp256.shape[0], resid.shape[1]
    for t, nm in ((kexp256, "kexp256"), (vpt, "vpt"), (resid, "resid"), (x, "x")):
        _chk(t, torch.bfloat16, nm, 3)
    for t, nm in ((out_bias, "out_bias"), (ln_w, "ln_w"), (ln_b, "ln_b")):
        _chk(t, torch.float32, nm, 1)
    _chk(cbias, torch.float32, "cbias", 2)
    if pe is not None:
        _chk(pe, torch.bfloat16, "pe", 2)
    if (tuple(kexp256.shape) != (B, 64, 256) or tuple(vpt.shape) != (B, 256, 64) or resid.shape[2] != 256 or tuple(x.shape[1:]) != (N, 256)
            or tuple(cbias.shape) != (B, 64) or x.shape[0] not in (1, B) or resid.shape[0] not in (1, B)):
        raise RuntimeError("samdec_img2tok_raw: shape mismatch")
    out = torch.empty(B, N, 256, dtype=torch.bfloat16, device=kexp256.device)
    _call("s6d_samdec_img2tok_raw_bf16", _ptr(x), _ptr(pe), _ptr(kexp256), _ptr(cbias), _ptr(vpt), _ptr(resid), _ptr(out_bias), _ptr(ln_w),
          _ptr(ln_b), eps, B, N, int(n_tok), 256, 1 if x.shape[0] == 1 and B > 1 else 0, 1 if resid.shape[0] == 1 and B > 1 else 0,
          _ptr(out), _stream())
    return out


def samdec_tok2img(qt, kv, k_off, v_off, k_pe, scale):
    """Token->image attention before out_proj.  qt (B,T<=8,128) f32, kv (1|B,N,ld) bf16 holding k / v at column
    offsets k_off / v_off, k_pe (N,128) bf16 or None -> (B,T,128) f32."""
    _chk(kv, torch.bfloat16, "kv", 3)
    B, T, _ = qt.shape
    if qt.dtype != torch.float32 or not qt.is_cuda or qt.shape[2] != 128 or T > 8 or kv.shape[0] not in (1, B):
        raise RuntimeError("samdec_tok2img: qt must be (B,T<=8,128) float32 CUDA, kv (1|B,N,ld)")
    q8 = torch.zeros(B, 8, 128, dtype=torch.float32, device=qt.device)
    q8[:, :T] = qt
    if k_pe is not None:
        _chk(k_pe, torch.bfloat16, "k_pe", 2)
    out = torch.empty(B, 8, 128, dtype=torch.float32, device=qt.device)
    _call("s6d_samdec_tok2img_f32", _ptr(q8), _ptr(kv), kv.shape[2], int(k_off), int(v_off), 1 if kv.shape[0] == 1 and B > 1 else 0,
          _ptr(k_pe), B, kv.shape[1], scale, _ptr(out), _stream())
    return out[:, :T]


def samdec_tok2img_raw(qt, x, pe, wk, wv, bv, scale):
    """Token->image attention before out_proj on the RAW image tokens: the k / v projections are folded into the queries, no
    projected k / v tensor over the image tokens exists.  qt (B,T<=8,128) f32 projected prompt tokens, x (1|B,N,256) bf16 image
    tokens, pe (N,256) bf16 or None (added to x for the scores), wk / wv (128,256), bv (128): the k_proj / v_proj parameters ->
    (B,T,128) f32 = softmax(q (W_k (x + pe))^T * scale) (W_v x + b_v), heads 8 x 16."""
    _chk(x, torch.bfloat16, "x", 3)
    B, T, _ = qt.shape
    if qt.dtype != torch.float32 or not qt.is_cuda or qt.shape[2] != 128 or T > 8 or x.shape[0] not in (1, B) or x.shape[2] != 256:
        raise RuntimeError("samdec_tok2img_raw: qt must be (B,T<=8,128) float32 CUDA, x (1|B,N,256) bfloat16")
    if pe is not None:
        _chk(pe, torch.bfloat16, "pe", 2)
    H, hd = 8, 16
    with torch.autocast(device_type="cuda", enabled=False):          # the two small folds stay float32 inside an autocast region
        # q'[b, h, t, :] = scale * log2(e) * W_k[h]^T q[b, t, h]
        qp = torch.zeros(B, H, 8, 256, dtype=torch.float32, device=qt.device)
        qp[:, :, :T] = torch.einsum("bthd,hdc->bhtc", qt.view(B, T, H, hd) * (scale * 1.4426950408889634), wk.float().view(H, hd, 256))
        qp = qp.to(torch.bfloat16).view(B, 64, 256)
        y = samdec_tok2img_raw_core(qp, x, pe)
        out = torch.einsum("bhtc,hdc->bthd", y.view(B, H, 8, 256)[:, :, :T], wv.float().view(H, hd, 256)) + bv.float().view(1, 1, H, hd)
    return out.reshape(B, T, 128)


def samdec_tokens_pre(queries, pe, add_pe, lin_q, lin_k, lin_v, lin_o, norm1, lin_q2, fold=None):
    """Self-attention + norm1 + token->image query projection of a TwoWayAttentionBlock's sparse tokens in one launch
    (s6d_samdec_tokens_pre_bf16).  queries, pe (B,T<=8,256) f32; lin_* = (fragment-ordered bf16 weight, f32 bias); norm1 =
    (gamma, beta, eps) -> (q1 (B,T,256) f32, qp (B,T,128) f32).
    fold = (wkfold, scale): the attention core's k projection folded into the queries inside the kernel -> (q1, qfold (B,64,256)
    bf16) instead: the query operand of samdec_tok2img_raw_core."""
    _chk(queries, torch.float32, "queries", 3)
    _chk(pe, torch.float32, "pe", 3)
    B, T, C = queries.shape
    if C != 256 or T > 8 or pe.shape != queries.shape:
        raise ValueError("samdec_tokens_pre: queries / pe must be (B, T <= 8, 256)")
    queries, pe = queries.contiguous(), pe.contiguous()
    q1 = torch.empty(B, T, 256, dtype=torch.float32, device=queries.device)
    if fold is None:
        out2 = torch.empty(B, T, 128, dtype=torch.float32, device=queries.device)
        qp_ptr, wk_ptr, sc, qf_ptr = _ptr(out2), None, 0.0, None
    else:
        out2 = torch.empty(B, 64, 256, dtype=torch.bfloat16, device=queries.device)
        qp_ptr, wk_ptr, sc, qf_ptr = None, _ptr(fold[0]), float(fold[1]), _ptr(out2)
    _call("s6d_samdec_tokens_pre_bf16", _ptr(queries), _ptr(pe), B, T, 1 if add_pe else 0, _ptr(lin_q[0]), _ptr(lin_q[1]), _ptr(lin_k[0]),
          _ptr(lin_k[1]), _ptr(lin_v[0]), _ptr(lin_v[1]), _ptr(lin_o[0]), _ptr(lin_o[1]), _ptr(norm1[0]), _ptr(norm1[1]), norm1[2],
          _ptr(lin_q2[0]), _ptr(lin_q2[1]), _ptr(q1), qp_ptr, wk_ptr, sc, qf_ptr, _stream())
    return q1, out2


def samdec_tok2img_raw_core(qfold, x, pe):
    """The attention core of samdec_tok2img_raw alone: qfold (B,64,256) bf16 folded queries (samdec_tokens_pre(fold=...)), x
    (1|B,N,256) bf16 image tokens, pe (N,256) bf16 or None -> y (B,64,256) f32 = sum_n p_jn x_n (samdec_tokens_post(y=...) applies W_v)."""
    _chk(qfold, torch.bfloat16, "qfold", 3)
    _chk(x, torch.bfloat16, "x", 3)
    B = qfold.shape[0]
    if tuple(qfold.shape[1:]) != (64, 256) or x.shape[0] not in (1, B) or x.shape[2] != 256 or not qfold.is_contiguous():
        raise RuntimeError("samdec_tok2img_raw_core: qfold must be contiguous (B,64,256), x (1|B,N,256) bfloat16")
    if pe is not None:
        _chk(pe, torch.bfloat16, "pe", 2)
    y = torch.empty(B, 64, 256, dtype=torch.float32, device=qfold.device)
    _call("s6d_samdec_tok2img_raw_bf16", _ptr(qfold), _ptr(x), x.stride(1), 1 if x.shape[0] == 1 and B > 1 else 0, _ptr(pe), B, x.shape[1],
          _ptr(y), _stream())
    return y


def samdec_tokens_post(q1, att, pe, lin_o2, norm2, lin_1, lin_2, norm3, lin_k3, lin_v3, y=None, vfold=None, expand=None):
    """Attention output projection + norm2 + MLP + norm3 + the image->token attention's k / v projections in one launch
    (s6d_samdec_tokens_post_bf16).  q1, pe (B,T,256) f32, att (B,T,128) f32 -> (q3 (B,T,256), kt (B,T,128), vt (B,T,128)) f32.
    y (B,64,256) f32 + vfold = (wvfold, bv): att is formed in the kernel from the attention core's raw result (att = None).
    expand = dict(wq=wqfold, bq=bias, wo=wofold, fold_q=bool): the operands of the image->token attention kernels are made in the
    kernel as well -> (q3, dict(kexp | k256 + cb, vpt)) instead of (q3, kt, vt)."""
    _chk(q1, torch.float32, "q1", 3)
    _chk(pe, torch.float32, "pe", 3)
    B, T, C = q1.shape
    if C != 256 or T > 8 or pe.shape != q1.shape:
        raise ValueError("samdec_tokens_post: q1 / pe must be (B, T <= 8, 256)")
    if y is None:
        _chk(att, torch.float32, "att", 3)
        if tuple(att.shape) != (B, T, 128):
            raise ValueError("samdec_tokens_post: att must be (B, T, 128)")
        att = att.contiguous()
    else:
        _chk(y, torch.float32, "y", 3)
        if tuple(y.shape) != (B, 64, 256) or not y.is_contiguous() or vfold is None:
            raise ValueError("samdec_tokens_post: y must be contiguous (B, 64, 256) with vfold = (wvfold, bv)")
    q1, pe = q1.contiguous(), pe.contiguous()
    dev = q1.device
    q3 = torch.empty(B, T, 256, dtype=torch.float32, device=dev)
    if expand is None:
        kt = torch.empty(B, T, 128, dtype=torch.float32, device=dev)
        vt = torch.empty(B, T, 128, dtype=torch.float32, device=dev)
        tail = (_ptr(kt), _ptr(vt))
        ex = (None,) * 7
        res = (q3, kt, vt)
    else:
        out = {"vpt": torch.empty(B, 256, 64, dtype=torch.bfloat16, device=dev)}
        if expand["fold_q"]:
            out["k256"] = torch.empty(B, 64, 256, dtype=torch.bfloat16, device=dev)
            out["cb"] = torch.empty(B, 64, dtype=torch.float32, device=dev)
            ex = (_ptr(expand["wq"]), _ptr(expand["bq"]), _ptr(expand["wo"]), None, _ptr(out["k256"]), _ptr(out["cb"]), _ptr(out["vpt"]))
        else:
            out["kexp"] = torch.zeros(B, 64, 128, dtype=torch.bfloat16, device=dev)      # block diagonal: the kernel writes the blocks
            ex = (None, None, _ptr(expand["wo"]), _ptr(out["kexp"]), None, None, _ptr(out["vpt"]))
        tail = (None, None)
        res = (q3, out)
    yargs = (None,) * 3 if y is None else (_ptr(y), _ptr(vfold[0]), _ptr(vfold[1]))
    _call("s6d_samdec_tokens_post_bf16", _ptr(q1), _ptr(att) if y is None else None, _ptr(pe), B, T, _ptr(lin_o2[0]), _ptr(lin_o2[1]),
          _ptr(norm2[0]), _ptr(norm2[1]), norm2[2], _ptr(lin_1[0]), _ptr(lin_1[1]), _ptr(lin_2[0]), _ptr(lin_2[1]), _ptr(norm3[0]),
          _ptr(norm3[1]), norm3[2], _ptr(lin_k3[0]), _ptr(lin_k3[1]), _ptr(lin_v3[0]), _ptr(lin_v3[1]), _ptr(q3), *tail, *yargs, *ex,
          _stream())
    return res


def sam_mask_post(low_res, img_size, input_size, original_size, mask_threshold=0.0, stability_offset=1.0):
    """Fused Sam.postprocess_masks + stability score + threshold + boxes.  low_res (B,C,n,n) f32 -- contiguous, or a channel
    slice ``full[:, c0:c0 + C]`` of a contiguous (B,Ct,n,n) tensor, which is read in place ->
    (masks (B*C,H,W) bool, stability (B*C,) f32, boxes (B*C,4) int64 XYXY, [0,0,0,0] for empty masks)."""
    if not low_res.is_cuda or low_res.dtype != torch.float32 or low_res.dim() != 4:
        raise RuntimeError("low_res must be a 4-d float CUDA tensor")
    B, C, n, n2 = low_res.shape
    if n != n2:
        raise RuntimeError("low_res must be square")
    sb, sc, sy, sx = low_res.stride()
    if not (sx == 1 and sy == n and sc == n * n and sb % (n * n) == 0 and sb >= C * n * n) or B * C == 0:
        low_res = low_res.contiguous()
        sb = C * n * n
    ct = max(sb // (n * n), C, 1)               # planes between consecutive prompts (Ct of the parent tensor for a channel slice)
    Bm, (H, W) = B * C, original_size
    if Bm == 0:                                    # no prompt or no channel: nothing to launch (a clamped channel count would write B rows
        dev = low_res.device                       # into zero-row outputs)
        return (torch.empty(0, H, W, dtype=torch.bool, device=dev), torch.empty(0, dtype=torch.float32, device=dev),
                torch.empty(0, 4, dtype=torch.int64, device=dev))
    masks = torch.empty(Bm, H, W, dtype=torch.bool, device=low_res.device)      # the kernel writes 0 / 1 bytes: no uint8 -> bool pass
    stats = torch.empty(Bm, 6, dtype=torch.int32, device=low_res.device)
    # the slice's data pointer is its first plane: mask (b, c) reads plane b * ct + c from there
    _call("s6d_sam_mask_post_sel_f32", _ptr(low_res), B, ct, 0, max(C, 1), n, int(img_size), int(input_size[0]), int(input_size[1]), H, W,
          mask_threshold, stability_offset, _ptr(masks), _ptr(stats), _stream())
    stability = stats[:, 0] / stats[:, 1]                           # int32 / int32 -> float32, NaN for 0 / 0 like the reference
    empty = (stats[:, 4] < stats[:, 2]) | (stats[:, 5] < stats[:, 3])
    boxes = stats[:, 2:6].long() * (~empty).unsqueeze(-1)
    return masks, stability, boxes


def nms(boxes, scores, iou_threshold):
    """torchvision.ops.nms: indices of the kept boxes, by decreasing score.  boxes (N,4) f32 XYXY, scores (N,)."""
    _chk(boxes, torch.float32, "boxes", 2)
    N = boxes.shape[0]
    if N == 0:
        return torch.empty(0, dtype=torch.int64, device=boxes.device)
    order = torch.sort(scores.float(), descending=True, stable=True)[1].contiguous()
    ws = torch.empty(max(_size("s6d_nms_workspace_bytes", N), 8), dtype=torch.uint8, device=boxes.device)
    keep = torch.empty(N, dtype=torch.uint8, device=boxes.device)
    _call("s6d_nms_f32", _ptr(boxes), _ptr(order), N, iou_threshold, _ptr(ws), _ptr(keep), _stream())
    return order[keep.bool()]


def samdec_upscale_heads(y0, ln_w, ln_b, eps, w2t, b2, hyper, h, w):
    """Output head of SAM's mask decoder after the first transposed conv (columns ordered (dy,dx,c)).
    y0 (B,h*w,256) bf16 (last-dim slice allowed), w2t (128,64) bf16, hyper (B,M,32) f32 -> masks (B,M,4h,4w) f32."""
    if y0.dtype != torch.bfloat16 or y0.dim() != 3 or y0.shape[-1] != 256 or y0.stride(2) != 1 or not y0.is_cuda:
        raise RuntimeError("y0 must be a (B,h*w,256) bfloat16 CUDA tensor with unit channel stride")
    B, N = y0.shape[0], y0.shape[1]
    y_ld = y0.stride(1)
    if B > 1 and y0.stride(0) != N * y_ld:
        raise RuntimeError("y0 batch stride must be N * row stride")
    _chk(w2t, torch.bfloat16, "w2t", 2)
    _chk(hyper, torch.float32, "hyper", 3)
    for t, nm in ((ln_w, "ln_w"), (ln_b, "ln_b"), (b2, "b2")):
        _chk(t, torch.float32, nm, 1)
    M = hyper.shape[1]
    if N != h * w or tuple(w2t.shape) != (128, 64) or hyper.shape[2] != 32 or hyper.shape[0] != B:
        raise RuntimeError("samdec_upscale_heads: shape mismatch")
    masks = torch.empty(B, M, 4 * h, 4 * w, dtype=torch.float32, device=y0.device)
    _call("s6d_samdec_upscale_heads_bf16", _ptr(y0), _ptr(ln_w), _ptr(ln_b), eps, _ptr(w2t), _ptr(b2), _ptr(hyper), B, M, h, w, y_ld,
          _ptr(masks), _stream())
    return masks


def segment_seq_sum(x, start, count):
    """Row-order float32 sums of segments of x (numpy's add.reduce over axis 0; the centroid numerator of the PEM
    pre-processing).  x (N,C) f32 with 2 <= C <= 4, start / count (P,) int64 -> (P,C) f32."""
    _chk(x, torch.float32, "x", 2)
    _chk(start, torch.int64, "start", 1)
    _chk(count, torch.int64, "count", 1)
    P, C = start.shape[0], x.shape[1]
    if count.shape[0] != P or not 2 <= C <= 4:
        raise RuntimeError("segment_seq_sum: start/count must have one entry per segment and C must be 2..4")
    out = torch.zeros(P, C, dtype=torch.float32, device=x.device)
    _call("s6d_segment_seq_sum_f32", _ptr(x), _ptr(start), _ptr(count), P, C, _ptr(out), _stream())
    return out


PEM_SAMPLE_MAX = 6144           # n_sample the sampler kernel serves (include/sam6d_hip.h: s6d_pem_sample_indices_f32)


def pem_sample_indices(keys, count, n_sample):
    """Sampler of the PEM pre-processing (one workgroup per detection: histogram threshold + in-LDS sort).  keys (P,L) f32
    uniforms in [0,1), count (P,) int64 (<= L), n_sample <= PEM_SAMPLE_MAX -> (idx (P,n_sample) int64, overflow (P,) int32)."""
    _chk(keys, torch.float32, "keys", 2)
    _chk(count, torch.int64, "count", 1)
    P, L = keys.shape
    if count.shape[0] != P:
        raise RuntimeError("pem_sample_indices: one count per row of keys")
    idx = torch.zeros(P, n_sample, dtype=torch.int64, device=keys.device)
    overflow = torch.zeros(P, dtype=torch.int32, device=keys.device)
    _call("s6d_pem_sample_indices_f32", _ptr(keys), L, _ptr(count), P, n_sample, _ptr(idx), _ptr(overflow), _stream())
    return idx, overflow


def pem_mask_boxes(mask8, depth, min_points):
    """mask8 (P,H,W) uint8 (non-zero = set), depth (H,W) f32 -> (m8 (P,H,W) uint8 = mask AND depth > 0, cnt (P,) int64,
    ok8 (P,) uint8 = cnt > min_points, box (P,4) int64 [y1,y2,x1,x2] by the reference's get_bbox)."""
    _chk(mask8, torch.uint8, "mask8", 3)
    _chk(depth, torch.float32, "depth", 2)
    P, H, W = mask8.shape
    if tuple(depth.shape) != (H, W):
        raise RuntimeError("pem_mask_boxes: depth must be (H,W)")
    dev = mask8.device
    m8 = torch.empty(P, H, W, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(P, dtype=torch.int64, device=dev)
    ok8 = torch.zeros(P, dtype=torch.uint8, device=dev)
    box = torch.zeros(P, 4, dtype=torch.int64, device=dev)
    _call("s6d_pem_mask_boxes_u8", _ptr(mask8), _ptr(depth), P, H, W, int(min_points), _ptr(m8), _ptr(cnt), _ptr(ok8), _ptr(box), _stream())
    return m8, cnt, ok8, box


def pem_crops(image_u8, m8, kept, box, S, use_mask, mean, std):
    """image (H,W,3) uint8, m8 (P,H,W) uint8, kept (M,) int64, box (P,4) int64 -> (M,3,S,S) f32 normalised masked crops."""
    _chk(image_u8, torch.uint8, "image", 3)
    _chk(m8, torch.uint8, "m8", 3)
    _chk(kept, torch.int64, "kept", 1)
    _chk(box, torch.int64, "box", 2)
    P, H, W = m8.shape
    if tuple(image_u8.shape) != (H, W, 3) or tuple(box.shape) != (P, 4):
        raise RuntimeError("pem_crops: shape mismatch")
    M = kept.shape[0]
    out = torch.empty(M, 3, S, S, dtype=torch.float32, device=m8.device)
    _call("s6d_pem_crops_f32", _ptr(image_u8), _ptr(m8), _ptr(kept), _ptr(box), M, H, W, S, bool(use_mask), _float3(mean), _float3(std),
          _ptr(out), _stream())
    return out


def pem_compact_cloud(m8, depth, box, ok8, fx, fy, cx, cy, cap):
    """m8 (P,H,W) uint8, depth (H,W) f32, box (P,4) int64, ok8 (P,) uint8 -> (choose (P,cap) int32, cloud (P,cap,3) f32,
    n (P,) int64): masked crop pixels in row-major crop order and their back-projections, one fixed-capacity slot each."""
    _chk(m8, torch.uint8, "m8", 3)
    _chk(depth, torch.float32, "depth", 2)
    _chk(box, torch.int64, "box", 2)
    _chk(ok8, torch.uint8, "ok8", 1)
    P, H, W = m8.shape
    if tuple(depth.shape) != (H, W) or tuple(box.shape) != (P, 4) or ok8.shape[0] != P:
        raise RuntimeError("pem_compact_cloud: shape mismatch")
    choose = torch.empty(P, cap, dtype=torch.int32, device=m8.device)
    cloud = torch.empty(P, cap, 3, dtype=torch.float32, device=m8.device)
    n = torch.zeros(P, dtype=torch.int64, device=m8.device)
    _call("s6d_pem_compact_cloud_f32", _ptr(m8), _ptr(depth), _ptr(box), _ptr(ok8), P, H, W, fx, fy, cx, cy, cap, _ptr(choose), _ptr(cloud),
          _ptr(n), _stream())
    return choose, cloud, n


def pem_radius_filter(center, limit, choose, cloud, n):
    """In place on (choose, cloud, n) of pem_compact_cloud: keep, in order, the points within limit[p] of center[p]."""
    _chk(center, torch.float32, "center", 2)
    _chk(limit, torch.float64, "limit", 1)
    _chk(choose, torch.int32, "choose", 2)
    _chk(cloud, torch.float32, "cloud", 3)
    _chk(n, torch.int64, "n", 1)
    P, cap = choose.shape
    if tuple(center.shape) != (P, 3) or limit.shape[0] != P or tuple(cloud.shape) != (P, cap, 3) or n.shape[0] != P:
        raise RuntimeError("pem_radius_filter: shape mismatch")
    _call("s6d_pem_radius_filter_f32", _ptr(center), _ptr(limit), P, cap, _ptr(choose), _ptr(cloud), _ptr(n), _stream())
    return n


# ------------------------------------------------------------------ object onboarding (csrc/s6d_onboard.hip)
def _views(mask8, name):
    _chk(mask8, torch.uint8, "mask", 3)
    T, H, W = mask8.shape
    if H * W >= 2 ** 31:
        raise RuntimeError(f"{name}: a view of {H} x {W} pixels is too large")
    return T, H, W


def template_boxes(mask8):
    """mask8 (T,H,W) uint8 template masks -> (cnt (T,) int64 pixels == 255, box (T,4) int64 [y1,y2,x1,x2] by the reference's
    get_bbox over them, tight (T,4) int64 [x1,y1,x2,y2] = PIL getbbox of the pixels != 0)."""
    T, H, W = _views(mask8, "template_boxes")
    dev = mask8.device
    cnt = torch.zeros(T, dtype=torch.int64, device=dev)
    box = torch.zeros(T, 4, dtype=torch.int64, device=dev)
    tight = torch.zeros(T, 4, dtype=torch.int64, device=dev)
    _call("s6d_template_boxes_u8", _ptr(mask8), T, H, W, _ptr(cnt), _ptr(box), _ptr(tight), _stream())
    return cnt, box, tight


def template_points(mask8, xyz_mm, box, cap):
    """mask8 (T,H,W) uint8, xyz_mm (T,H,W,3) f32, box (T,4) int64 -> (choose (T,cap) int32, pts (T,cap,3) f32 metres, n (T,) int64):
    the pixels == 255 of every square crop in row-major crop order, one fixed-capacity slot per view."""
    T, H, W = _views(mask8, "template_points")
    _chk(xyz_mm, torch.float32, "xyz_mm", 4)
    _chk(box, torch.int64, "box", 2)
    if tuple(xyz_mm.shape) != (T, H, W, 3) or tuple(box.shape) != (T, 4):
        raise RuntimeError("template_points: shape mismatch")
    choose = torch.empty(T, cap, dtype=torch.int32, device=mask8.device)
    pts = torch.empty(T, cap, 3, dtype=torch.float32, device=mask8.device)
    n = torch.zeros(T, dtype=torch.int64, device=mask8.device)
    _call("s6d_template_points_f32", _ptr(mask8), _ptr(xyz_mm), _ptr(box), T, H, W, cap, _ptr(choose), _ptr(pts), _ptr(n), _stream())
    return choose, pts, n


def template_pem_crops(images_u8, mask8, box, S, use_mask, mean, std):
    """images (T,H,W,3) uint8, mask8 (T,H,W) uint8, box (T,4) int64 -> (T,3,S,S) f32 normalised, channel-flipped crops."""
    T, H, W = _views(mask8, "template_pem_crops")
    _chk(images_u8, torch.uint8, "images", 4)
    _chk(box, torch.int64, "box", 2)
    if tuple(images_u8.shape) != (T, H, W, 3) or tuple(box.shape) != (T, 4):
        raise RuntimeError("template_pem_crops: shape mismatch")
    out = torch.empty(T, 3, S, S, dtype=torch.float32, device=mask8.device)
    _call("s6d_template_pem_crops_f32", _ptr(images_u8), _ptr(mask8), _ptr(box), T, H, W, S, bool(use_mask), _float3(mean), _float3(std),
          _ptr(out), _stream())
    return out


def template_ism_crops(images_u8, mask8, params, S, normalize, mean, std):
    """images (T,H,W,3) uint8, mask8 (T,H,W) uint8, params (T,12) int32 records (sam6d_amd.ism.dinov2.crop_params on the tight
    boxes) -> (templates (T,3,S,S) f32, masks (T,S,S) f32)."""
    T, H, W = _views(mask8, "template_ism_crops")
    _chk(images_u8, torch.uint8, "images", 4)
    _chk(params, torch.int32, "params", 2)
    if tuple(images_u8.shape) != (T, H, W, 3) or tuple(params.shape) != (T, 12):
        raise RuntimeError("template_ism_crops: shape mismatch")
    S = int(S)
    o_rgb = torch.empty(T, 3, S, S, dtype=torch.float32, device=mask8.device)
    o_mask = torch.empty(T, S, S, dtype=torch.float32, device=mask8.device)
    _call("s6d_template_ism_crops_f32", _ptr(images_u8), _ptr(mask8), _ptr(params), T, H, W, S, bool(normalize), _float3(mean), _float3(std),
          _ptr(o_rgb), _ptr(o_mask), _stream())
    return o_rgb, o_mask


# ------------------------------------------------------------------ template rendering (csrc/s6d_raster.hip)
def _render_buffers(who, T, F, H, W, dev):
    """The workspace and the outputs that the two full renders share."""
    nbytes = _size("s6d_raster_workspace_bytes", T, F, H, W)
    if nbytes < 0:
        raise RuntimeError(f"{who}: unsupported sizes (T {T}, F {F}, H {H}, W {W})")
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    out = dict(rgb=torch.empty(T, H, W, 3, dtype=torch.uint8, device=dev), mask=torch.empty(T, H, W, dtype=torch.uint8, device=dev),
               xyz=torch.empty(T, H, W, 3, dtype=torch.float32, device=dev), depth=torch.empty(T, H, W, dtype=torch.float32, device=dev),
               face=torch.empty(T, H, W, dtype=torch.int32, device=dev), skipped=torch.zeros(T, dtype=torch.int32, device=dev))
    return ws, out


def render_views(vertices, faces, colors, poses, fx, fy, cx, cy, H, W, ambient, diffuse, znear, check_faces=True):
    """vertices (V,3) f32, faces (F,3) int32, colors (V,3) uint8, poses (T,4,4) f32 object -> camera (OpenCV axes) ->
    dict(rgb (T,H,W,3) uint8, mask (T,H,W) uint8, xyz (T,H,W,3) f32, depth (T,H,W) f32, face (T,H,W) int32, skipped (T,) int32)
    for all T views (include/sam6d_hip.h: s6d_raster_views_f32).  A face index outside [0, V) is refused here, on the host;
    check_faces=False is for a caller that has made that check on the same faces already (it reads the device: a synchronisation)."""
    _chk(vertices, torch.float32, "vertices", 2)
    _chk(faces, torch.int32, "faces", 2)
    _chk(colors, torch.uint8, "colors", 2)
    _chk(poses, torch.float32, "poses", 3)
    V, F, T, H, W = vertices.shape[0], faces.shape[0], poses.shape[0], int(H), int(W)
    if vertices.shape[1] != 3 or faces.shape[1] != 3 or tuple(colors.shape) != (V, 3) or tuple(poses.shape[1:]) != (4, 4):
        raise ValueError(f"render_views: vertices (V,3), faces (F,3), colors (V,3), poses (T,4,4) expected, got {tuple(vertices.shape)}, "
                         f"{tuple(faces.shape)}, {tuple(colors.shape)}, {tuple(poses.shape)}")
    if check_faces and F and (int(faces.min()) < 0 or int(faces.max()) >= V):
        raise ValueError(f"render_views: face indices must lie in [0, {V}), got [{int(faces.min())}, {int(faces.max())}]")
    ws, out = _render_buffers("render_views", T, F, H, W, vertices.device)
    _call("s6d_raster_views_f32", _ptr(vertices), _ptr(faces), _ptr(colors), _ptr(poses), V, F, T, H, W, float(fx), float(fy), float(cx),
          float(cy), float(znear), float(ambient), float(diffuse), _ptr(ws), _ptr(out["rgb"]), _ptr(out["mask"]), _ptr(out["xyz"]),
          _ptr(out["depth"]), _ptr(out["face"]), _ptr(out["skipped"]), _stream())
    return out


def texture_pyramid(image):
    """image (Ht,Wt,3) uint8 RGB, row 0 at the top, 1 <= Ht, Wt <= 8192 -> the box-filtered mip pyramid (N,4) uint8: a texel per
    row (r, g, b, 0), levels 0 .. floor(log2(max(Wt, Ht))) one after another, level l of max(1, Wt >> l) x max(1, Ht >> l) texels
    row-major (include/sam6d_hip.h: s6d_texture_pyramid_u8).  Built once per object; ``render_views_textured`` takes it."""
    _chk(image, torch.uint8, "image", 3)
    Ht, Wt = image.shape[0], image.shape[1]
    nbytes = _size("s6d_texture_pyramid_bytes", Ht, Wt)
    if image.shape[2] != 3 or nbytes < 0:
        raise ValueError(f"texture_pyramid: image (Ht,Wt,3) with 1 <= Ht, Wt <= 8192 expected, got {tuple(image.shape)}")
    pyramid = torch.empty(nbytes // 4, 4, dtype=torch.uint8, device=image.device)
    _call("s6d_texture_pyramid_u8", _ptr(image), Ht, Wt, _ptr(pyramid), _stream())
    return pyramid


def render_views_textured(vertices, faces, uv, pyramid, poses, fx, fy, cx, cy, H, W, ambient, diffuse, znear, tex_size, levels=False):
    """``render_views`` with a texture in place of the vertex colours: uv (F,3,2) f32 per face corner, pyramid (N,4) uint8 =
    ``texture_pyramid(image)``, tex_size = (Ht, Wt) of that image.  -> the dict of ``render_views`` (mask, xyz, depth, face and
    skipped are its bits), with levels=True also ``level`` (T,H,W) int32, the sampled pyramid level, -1 on background
    (include/sam6d_hip.h: s6d_raster_views_tex_f32).  A face index outside [0, V) is refused here, on the host."""
    _chk(vertices, torch.float32, "vertices", 2)
    _chk(faces, torch.int32, "faces", 2)
    _chk(uv, torch.float32, "uv", 3)
    _chk(pyramid, torch.uint8, "pyramid", 2)
    _chk(poses, torch.float32, "poses", 3)
    V, F, T, H, W = vertices.shape[0], faces.shape[0], poses.shape[0], int(H), int(W)
    Ht, Wt = (int(s) for s in tex_size)
    if vertices.shape[1] != 3 or faces.shape[1] != 3 or tuple(uv.shape) != (F, 3, 2) or tuple(poses.shape[1:]) != (4, 4):
        raise ValueError(f"render_views_textured: vertices (V,3), faces (F,3), uv (F,3,2), poses (T,4,4) expected, got "
                         f"{tuple(vertices.shape)}, {tuple(faces.shape)}, {tuple(uv.shape)}, {tuple(poses.shape)}")
    tbytes = _size("s6d_texture_pyramid_bytes", Ht, Wt)
    if tbytes < 0 or tuple(pyramid.shape) != (tbytes // 4, 4):
        raise ValueError(f"render_views_textured: tex_size {(Ht, Wt)} must lie in [1, 8192] and pyramid be texture_pyramid's "
                         f"({max(tbytes, 0) // 4}, 4) for it, got {tuple(pyramid.shape)}")
    if F and (int(faces.min()) < 0 or int(faces.max()) >= V):
        raise ValueError(f"render_views_textured: face indices must lie in [0, {V}), got [{int(faces.min())}, {int(faces.max())}]")
    ws, out = _render_buffers("render_views_textured", T, F, H, W, vertices.device)
    if levels:
        out["level"] = torch.empty(T, H, W, dtype=torch.int32, device=vertices.device)
    _call("s6d_raster_views_tex_f32", _ptr(vertices), _ptr(faces), _ptr(uv), _ptr(pyramid), _ptr(poses), V, F, T, H, W, Ht, Wt, float(fx),
          float(fy), float(cx), float(cy), float(znear), float(ambient), float(diffuse), _ptr(ws), _ptr(out["rgb"]), _ptr(out["mask"]),
          _ptr(out["xyz"]), _ptr(out["depth"]), _ptr(out["face"]), _ptr(out.get("level")), _ptr(out["skipped"]), _stream())
    return out


def render_depth(vertices, faces, poses, cams, H, W, znear, check_faces=True):
    """vertices (V,3) f32, faces (F,3) int32, poses (T,4,4) f32 object -> camera, cams (T,4) f32 = fx fy cx cy per view ->
    dict(depth (T,H,W) f32 camera Z, 0 on background; skipped (T,) int32): the depth bits of ``render_views`` for the same view and
    camera (include/sam6d_hip.h: s6d_raster_depth_f32).  A face index outside [0, V) is refused here, on the host (check_faces=False
    skips that read of the device: for a caller that checked the mesh once, as ``render_views`` allows)."""
    _chk(vertices, torch.float32, "vertices", 2)
    _chk(faces, torch.int32, "faces", 2)
    _chk(poses, torch.float32, "poses", 3)
    _chk(cams, torch.float32, "cams", 2)
    V, F, T, H, W = vertices.shape[0], faces.shape[0], poses.shape[0], int(H), int(W)
    if vertices.shape[1] != 3 or faces.shape[1] != 3 or tuple(poses.shape[1:]) != (4, 4) or tuple(cams.shape) != (T, 4):
        raise ValueError(f"render_depth: vertices (V,3), faces (F,3), poses (T,4,4), cams (T,4) expected, got {tuple(vertices.shape)}, "
                         f"{tuple(faces.shape)}, {tuple(poses.shape)}, {tuple(cams.shape)}")
    if check_faces and F and (int(faces.min()) < 0 or int(faces.max()) >= V):
        raise ValueError(f"render_depth: face indices must lie in [0, {V}), got [{int(faces.min())}, {int(faces.max())}]")
    nbytes = _size("s6d_raster_depth_workspace_bytes", T, F, H, W)
    if nbytes < 0:
        raise RuntimeError(f"render_depth: unsupported sizes (T {T}, F {F}, H {H}, W {W})")
    dev = vertices.device
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    out = dict(depth=torch.empty(T, H, W, dtype=torch.float32, device=dev), skipped=torch.zeros(T, dtype=torch.int32, device=dev))
    _call("s6d_raster_depth_f32", _ptr(vertices), _ptr(faces), _ptr(poses), _ptr(cams), V, F, T, H, W, float(znear), _ptr(ws),
          _ptr(out["depth"]), _ptr(out["skipped"]), _stream())
    return out


# ------------------------------------------------------------------ BOP pose errors (csrc/s6d_boperr.hip)
def pose_errors(vertices, est, gts, cams):
    """vertices (V,3) f32, est (N,4,4) f32 object -> camera, gts (N,S,4,4) f32 ground truths composed with the S symmetries,
    cams (N,4) f32 = fx fy cx cy -> (mssd (N,) f32 model units, mspd (N,) f32 pixels): the minimum over the symmetries of the
    maximum over the vertices (include/sam6d_hip.h: s6d_pose_err_mssd_mspd_f32)."""
    _chk(vertices, torch.float32, "vertices", 2)
    _chk(est, torch.float32, "est", 3)
    _chk(gts, torch.float32, "gts", 4)
    _chk(cams, torch.float32, "cams", 2)
    V, N, S = vertices.shape[0], est.shape[0], gts.shape[1]
    if vertices.shape[1] != 3 or tuple(est.shape[1:]) != (4, 4) or tuple(gts.shape) != (N, S, 4, 4) or tuple(cams.shape) != (N, 4):
        raise ValueError(f"pose_errors: vertices (V,3), est (N,4,4), gts (N,S,4,4), cams (N,4) expected, got {tuple(vertices.shape)}, "
                         f"{tuple(est.shape)}, {tuple(gts.shape)}, {tuple(cams.shape)}")
    mssd = torch.empty(N, dtype=torch.float32, device=vertices.device)
    mspd = torch.empty(N, dtype=torch.float32, device=vertices.device)
    _call("s6d_pose_err_mssd_mspd_f32", _ptr(vertices), _ptr(est), _ptr(gts), _ptr(cams), V, N, S, _ptr(mssd), _ptr(mspd), _stream())
    return mssd, mspd


def vsd_counts(depth_est, depth_gt, depth_test, test_index, cams, delta, taus, scale):
    """depth_est, depth_gt (N,H,W) f32 rendered depths, depth_test (M,H,W) f32 measured depth in the same unit (0 = missing),
    test_index (N,) int32 into M, cams (N,4) f32, delta, taus (a sequence of at most 16 floats), scale (N,) f32 ->
    (union (N,) int32, inter (N,) int32, ge (N,NT) int32): the pixel counts of VSD (include/sam6d_hip.h: s6d_vsd_counts_f32).
    A test_index outside [0, M) is refused here, on the host."""
    _chk(depth_est, torch.float32, "depth_est", 3)
    _chk(depth_gt, torch.float32, "depth_gt", 3)
    _chk(depth_test, torch.float32, "depth_test", 3)
    _chk(test_index, torch.int32, "test_index", 1)
    _chk(cams, torch.float32, "cams", 2)
    _chk(scale, torch.float32, "scale", 1)
    N, H, W = depth_est.shape
    M = depth_test.shape[0]
    tau = [float(x) for x in (taus.tolist() if hasattr(taus, "tolist") else taus)]
    NT = len(tau)
    if tuple(depth_gt.shape) != (N, H, W) or tuple(depth_test.shape[1:]) != (H, W) or tuple(test_index.shape) != (N,) or \
            tuple(cams.shape) != (N, 4) or tuple(scale.shape) != (N,):
        raise ValueError(f"vsd_counts: depth_est, depth_gt (N,H,W), depth_test (M,H,W), test_index (N,), cams (N,4), scale (N,) expected, got "
                         f"{tuple(depth_est.shape)}, {tuple(depth_gt.shape)}, {tuple(depth_test.shape)}, {tuple(test_index.shape)}, "
                         f"{tuple(cams.shape)}, {tuple(scale.shape)}")
    if N and (int(test_index.min()) < 0 or int(test_index.max()) >= M):
        raise ValueError(f"vsd_counts: test_index must lie in [0, {M}), got [{int(test_index.min())}, {int(test_index.max())}]")
    dev = depth_est.device
    union = torch.empty(N, dtype=torch.int32, device=dev)
    inter = torch.empty(N, dtype=torch.int32, device=dev)
    ge = torch.empty(N, NT, dtype=torch.int32, device=dev)
    _call("s6d_vsd_counts_f32", _ptr(depth_est), _ptr(depth_gt), _ptr(depth_test), _ptr(test_index), _ptr(cams), _ptr(scale), N, M, H, W,
          float(delta), (ctypes.c_float * max(NT, 1))(*tau), NT, _ptr(union), _ptr(inter), _ptr(ge), _stream())
    return union, inter, ge


# ------------------------------------------------------------------ BOP ground truth from poses (csrc/s6d_bopgt.hip)
def gt_visibility(canvas, depth_test, test_index, cams, delta, margin=(0, 0)):
    """canvas (N, H + 2 my, W + 2 mx) f32 = ``render_depth`` of every instance at that size with cx + mx, cy + my (camera Z, 0 on
    background), depth_test (M,H,W) f32 measured depth in the same unit (0 = missing), test_index (N,) int32 into M, cams (N,4) f32
    = fx fy cx cy of the IMAGE, delta, margin = (mx, my) >= 0 ->
    dict(mask, mask_visib (N,H,W) uint8 0 / 1; counts (N,4) int32 = all (canvas), in-image, valid, visib; extents (N,2,4) int32 =
    xmin ymin xmax ymax inclusive in image coordinates, row 0 of the object on the canvas, row 1 of the visible part, an empty set
    INT_MAX INT_MAX INT_MIN INT_MIN) (include/sam6d_hip.h: s6d_gt_visibility_f32).  A test_index outside [0, M) is refused here, on
    the host."""
    _chk(canvas, torch.float32, "canvas", 3)
    _chk(depth_test, torch.float32, "depth_test", 3)
    _chk(test_index, torch.int32, "test_index", 1)
    _chk(cams, torch.float32, "cams", 2)
    mx, my = (int(m) for m in margin)
    if mx < 0 or my < 0:
        raise ValueError(f"gt_visibility: margin must be >= 0, got {(mx, my)}")
    N, M, H, W = canvas.shape[0], depth_test.shape[0], depth_test.shape[1], depth_test.shape[2]
    if tuple(canvas.shape[1:]) != (H + 2 * my, W + 2 * mx) or M < 1 or H < 1 or W < 1 or tuple(test_index.shape) != (N,) or \
            tuple(cams.shape) != (N, 4):
        raise ValueError(f"gt_visibility: canvas (N,H+2my,W+2mx), depth_test (M,H,W), test_index (N,), cams (N,4) expected, got "
                         f"{tuple(canvas.shape)}, {tuple(depth_test.shape)}, {tuple(test_index.shape)}, {tuple(cams.shape)} with margin {(mx, my)}")
    if (H + 2 * my) * (W + 2 * mx) >= 2 ** 31:
        raise ValueError(f"gt_visibility: a canvas of {(H + 2 * my) * (W + 2 * mx)} pixels (2^31 or more) is refused")
    if N and (int(test_index.min()) < 0 or int(test_index.max()) >= M):
        raise ValueError(f"gt_visibility: test_index must lie in [0, {M}), got [{int(test_index.min())}, {int(test_index.max())}]")
    dev = canvas.device
    out = dict(mask=torch.empty(N, H, W, dtype=torch.uint8, device=dev), mask_visib=torch.empty(N, H, W, dtype=torch.uint8, device=dev),
               counts=torch.empty(N, 4, dtype=torch.int32, device=dev), extents=torch.empty(N, 2, 4, dtype=torch.int32, device=dev))
    _call("s6d_gt_visibility_f32", _ptr(canvas), _ptr(depth_test), _ptr(test_index), _ptr(cams), N, M, H, W, mx, my, float(delta),
          _ptr(out["mask"]), _ptr(out["mask_visib"]), _ptr(out["counts"]), _ptr(out["extents"]), _stream())
    return out


def model_diameter(vertices):
    """vertices (V,3) f32, V >= 1 -> (1,) f32: the largest distance between two vertices, sqrtf of the maximum of
    (dx dx + dy dy) + dz dz over all pairs; +inf when a squared distance is not finite (include/sam6d_hip.h:
    s6d_model_diameter_f32).  No (V,V) buffer is made."""
    _chk(vertices, torch.float32, "vertices", 2)
    if vertices.shape[1] != 3 or vertices.shape[0] < 1:
        raise ValueError(f"model_diameter: vertices (V,3) with V >= 1 expected, got {tuple(vertices.shape)}")
    out = torch.empty(1, dtype=torch.float32, device=vertices.device)
    _call("s6d_model_diameter_f32", _ptr(vertices), vertices.shape[0], _ptr(out), _stream())
    return out


# ------------------------------------------------------------------ ADD / ADD-S pose errors (csrc/s6d_adderr.hip)
def add_errors(vertices, est, gts, per_vertex=False, which=("add", "adds")):
    """vertices (V,3) f32, V >= 1, est, gts (N,4,4) f32 object -> camera: N pose pairs of ONE object -> dict
    add, adds (N,) f64: the mean over the vertices of |E v_i - G v_i| and of min_j |E v_i - G v_j| (fixed summation order);
    add_max, adds_max (N,) f32: the maxima (adds_max: the one-sided Hausdorff distance);
    add_per_vertex, adds_per_vertex (N,V) f32 when ``per_vertex``, None otherwise (the values then live in a workspace)
    (include/sam6d_hip.h: s6d_pose_err_add_f32, s6d_pose_err_adds_f32).  ``which``: the errors to compute; the keys of the other
    are None.  No (V,V) buffer is made."""
    _chk(vertices, torch.float32, "vertices", 2)
    _chk(est, torch.float32, "est", 3)
    _chk(gts, torch.float32, "gts", 3)
    V, N = vertices.shape[0], est.shape[0]
    if vertices.shape[1] != 3 or V < 1 or tuple(est.shape[1:]) != (4, 4) or tuple(gts.shape) != (N, 4, 4):
        raise ValueError(f"add_errors: vertices (V,3) with V >= 1, est (N,4,4), gts (N,4,4) expected, got {tuple(vertices.shape)}, "
                         f"{tuple(est.shape)}, {tuple(gts.shape)}")
    if N * V >= 2 ** 31:
        raise ValueError(f"add_errors: N * V = {N * V} (2^31 or more) is refused; chunk over N (evaluation.add_errors does)")
    dev = vertices.device
    out = dict(add=None, add_max=None, add_per_vertex=None, adds=None, adds_max=None, adds_per_vertex=None)
    ws = None
    if not per_vertex:
        ws = torch.empty((_size("s6d_pose_err_adds_workspace_bytes", N, V) + 3) // 4, dtype=torch.float32, device=dev)
    for name in which:
        if name not in ("add", "adds"):
            raise ValueError(f"add_errors: which names 'add' and 'adds', got {name!r}")
        pv = torch.empty(N, V, dtype=torch.float32, device=dev) if per_vertex else None
        mean = torch.empty(N, dtype=torch.float64, device=dev)
        top = torch.empty(N, dtype=torch.float32, device=dev)
        args = (_ptr(vertices), V, _ptr(est), _ptr(gts), N, _ptr(pv), _ptr(mean), _ptr(top), _ptr(ws), _stream())
        if name == "add":
            _call("s6d_pose_err_add_f32", *args)
        else:
            _call("s6d_pose_err_adds_f32", *args)
        out[name], out[name + "_max"], out[name + "_per_vertex"] = mean, top, pv
    return out


# ------------------------------------------------------------------ pose refinement against the depth (csrc/s6d_refine.hip)
RF_CHUNK = _lib.header_constant("S6D_RF_CHUNK")          # pixels one workgroup of the normal-equation kernel sums (its reduction order)
RF_TERMS = 28                                            # 21 upper entries of J J^T, 6 of J r, r r


def refine_normal_eq(xyz, face, depth_obs, obs_index, mask, vertices, faces, poses, fx, fy, cx, cy, depth_unit, max_dist, min_cos,
                     check_index=True):
    """xyz (T,H,W,3) f32 and face (T,H,W) int32 of ``render_views`` at poses (T,4,4) f32, depth_obs (M,H,W) f32, obs_index (T,) int32
    into M, mask (T,H,W) uint8 or None, vertices (V,3) f32, faces (F,3) int32 -> (sums (T,28) f64, count (T,) int32): the normal
    equations of one point-to-plane step (include/sam6d_hip.h: s6d_refine_normal_eq_f64).  An obs_index outside [0, M) is refused
    here, on the host; check_index=False leaves that read of the device out (the kernel then gives such an instance zeros)."""
    _chk(xyz, torch.float32, "xyz", 4)
    _chk(face, torch.int32, "face", 3)
    _chk(depth_obs, torch.float32, "depth_obs", 3)
    _chk(obs_index, torch.int32, "obs_index", 1)
    _chk(vertices, torch.float32, "vertices", 2)
    _chk(faces, torch.int32, "faces", 2)
    _chk(poses, torch.float32, "poses", 3)
    if mask is not None:
        _chk(mask, torch.uint8, "mask", 3)
    T, H, W = face.shape
    M, V, F = depth_obs.shape[0], vertices.shape[0], faces.shape[0]
    if tuple(xyz.shape) != (T, H, W, 3) or tuple(depth_obs.shape[1:]) != (H, W) or tuple(obs_index.shape) != (T,) or \
            tuple(poses.shape) != (T, 4, 4) or vertices.shape[1] != 3 or faces.shape[1] != 3 or \
            (mask is not None and tuple(mask.shape) != (T, H, W)):
        raise ValueError(f"refine_normal_eq: xyz (T,H,W,3), face (T,H,W), depth_obs (M,H,W), obs_index (T,), mask (T,H,W), vertices (V,3), "
                         f"faces (F,3), poses (T,4,4) expected, got {tuple(xyz.shape)}, {tuple(face.shape)}, {tuple(depth_obs.shape)}, "
                         f"{tuple(obs_index.shape)}, {None if mask is None else tuple(mask.shape)}, {tuple(vertices.shape)}, "
                         f"{tuple(faces.shape)}, {tuple(poses.shape)}")
    if check_index and T and (int(obs_index.min()) < 0 or int(obs_index.max()) >= M):
        raise ValueError(f"refine_normal_eq: obs_index must lie in [0, {M}), got [{int(obs_index.min())}, {int(obs_index.max())}]")
    nbytes = _size("s6d_refine_workspace_bytes", T, H, W)
    if nbytes < 0:
        raise RuntimeError(f"refine_normal_eq: unsupported sizes (T {T}, H {H}, W {W})")
    dev = xyz.device
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    sums = torch.empty(T, RF_TERMS, dtype=torch.float64, device=dev)
    count = torch.empty(T, dtype=torch.int32, device=dev)
    _call("s6d_refine_normal_eq_f64", _ptr(xyz), _ptr(face), _ptr(depth_obs), _ptr(obs_index), _ptr(mask), _ptr(vertices), _ptr(faces),
          _ptr(poses), V, F, T, M, H, W, float(fx), float(fy), float(cx), float(cy), float(depth_unit), float(max_dist), float(min_cos),
          _ptr(ws), _ptr(sums), _ptr(count), _stream())
    return sums, count


def refine_update(sums, count, poses, min_count, damping, min_pivot):
    """sums (T,28) f64 and count (T,) int32 of ``refine_normal_eq``, poses (T,4,4) f32 -> (poses_out (T,4,4) f32, status (T,) int32,
    rms (T,) f64): the damped, Jacobi-scaled Cholesky solve and the Cayley update (include/sam6d_hip.h: s6d_refine_update_f64).
    status 0 updated, 1 too few correspondences, 2 singular, 3 not finite; a non-zero status returns the input pose."""
    _chk(sums, torch.float64, "sums", 2)
    _chk(count, torch.int32, "count", 1)
    _chk(poses, torch.float32, "poses", 3)
    T = poses.shape[0]
    if tuple(sums.shape) != (T, RF_TERMS) or tuple(count.shape) != (T,) or tuple(poses.shape[1:]) != (4, 4):
        raise ValueError(f"refine_update: sums (T,28), count (T,), poses (T,4,4) expected, got {tuple(sums.shape)}, {tuple(count.shape)}, "
                         f"{tuple(poses.shape)}")
    dev = poses.device
    out = torch.empty_like(poses)
    status = torch.empty(T, dtype=torch.int32, device=dev)
    rms = torch.empty(T, dtype=torch.float64, device=dev)
    _call("s6d_refine_update_f64", _ptr(sums), _ptr(count), _ptr(poses), T, int(min_count), float(damping), float(min_pivot), _ptr(out),
          _ptr(status), _ptr(rms), _stream())
    return out, status, rms


# ------------------------------------------------------------------ COCO AP of ISM results (csrc/s6d_cocoeval.hip)
def _pairs(pairs, n_det, n_gt, what):
    _chk(pairs, torch.int32, "pairs", 2)
    if pairs.shape[1] != 2:
        raise ValueError(f"{what}: pairs (P,2) expected, got {tuple(pairs.shape)}")
    if pairs.shape[0] and (int(pairs.min()) < 0 or int(pairs[:, 0].max()) >= n_det or int(pairs[:, 1].max()) >= n_gt):
        raise ValueError(f"{what}: pairs must index rows [0, {n_det}) and [0, {n_gt})")
    return pairs.shape[0]


def mask_pack(masks):
    """masks (N,H,W) uint8 or bool -> (packed (N, ceil(H W / 64)) int64, area (N,) int32): bit k of word j is pixel 64 j + k in
    row-major order, the bits past H W are zero (include/sam6d_hip.h: s6d_mask_pack_u8)."""
    if masks.dtype == torch.bool and masks.is_cuda and masks.is_contiguous():
        masks = masks.view(torch.uint8)
    _chk(masks, torch.uint8, "masks", 3)
    N, H, W = masks.shape
    if H * W < 1:
        raise ValueError(f"mask_pack: masks (N,H,W) with H W >= 1 expected, got {tuple(masks.shape)}")
    packed = torch.empty(N, (H * W + 63) // 64, dtype=torch.int64, device=masks.device)
    area = torch.empty(N, dtype=torch.int32, device=masks.device)
    _call("s6d_mask_pack_u8", _ptr(masks), N, H * W, _ptr(packed), _ptr(area), _stream())
    return packed, area


def mask_pair_inter(det_packed, gt_packed, pairs):
    """det_packed (Nd,words), gt_packed (Ng,words) int64 (``mask_pack``), pairs (P,2) int32 = (detection row, ground-truth row) ->
    (P,) int32 popcount(d & g).  A pair has the same count whatever else is in the list (include/sam6d_hip.h: s6d_mask_pair_inter).
    Rows outside the arrays are refused here, on the host."""
    _chk(det_packed, torch.int64, "det_packed", 2)
    _chk(gt_packed, torch.int64, "gt_packed", 2)
    if det_packed.shape[1] != gt_packed.shape[1] or det_packed.shape[1] < 1:
        raise ValueError(f"mask_pair_inter: det_packed (Nd,words), gt_packed (Ng,words) expected, got {tuple(det_packed.shape)}, "
                         f"{tuple(gt_packed.shape)}")
    P = _pairs(pairs, det_packed.shape[0], gt_packed.shape[0], "mask_pair_inter")
    inter = torch.empty(P, dtype=torch.int32, device=pairs.device)
    _call("s6d_mask_pair_inter", _ptr(det_packed), det_packed.shape[0], _ptr(gt_packed), gt_packed.shape[0], det_packed.shape[1],
          _ptr(pairs), P, _ptr(inter), _stream())
    return inter


def box_pair_iou(det_boxes, gt_boxes, pairs):
    """det_boxes (Nd,4), gt_boxes (Ng,4) float64 = x y w h, pairs (P,2) int32 -> (P,) float64 IoU in the stated operation order
    (include/sam6d_hip.h: s6d_box_pair_iou_f64)."""
    _chk(det_boxes, torch.float64, "det_boxes", 2)
    _chk(gt_boxes, torch.float64, "gt_boxes", 2)
    if det_boxes.shape[1] != 4 or gt_boxes.shape[1] != 4:
        raise ValueError(f"box_pair_iou: det_boxes (Nd,4), gt_boxes (Ng,4) expected, got {tuple(det_boxes.shape)}, {tuple(gt_boxes.shape)}")
    P = _pairs(pairs, det_boxes.shape[0], gt_boxes.shape[0], "box_pair_iou")
    iou = torch.empty(P, dtype=torch.float64, device=pairs.device)
    _call("s6d_box_pair_iou_f64", _ptr(det_boxes), det_boxes.shape[0], _ptr(gt_boxes), gt_boxes.shape[0], _ptr(pairs), P, _ptr(iou),
          _stream())
    return iou


def coco_match(ious, iou_off, groups, det_area, gt_area, gt_ignore, thresholds, area_ranges):
    """Greedy matching of every group = (image, category).  groups (n,4) int32 = first detection, detections, first ground truth,
    ground truths (at most S6D_COCO_MATCH_MAX_GT = 64); iou_off (n,) int64: where the group's (D,G) row-major block of ``ious``
    (float64) begins; det_area (Dn,), gt_area (Gn,) float64; gt_ignore (Gn,) uint8; thresholds (NT,), area_ranges (NA,2) float64,
    NT NA <= 64 -> (match (Dn,NT,NA) int32: the ground truth's index inside its group or -1, ignore (Dn,NT,NA) uint8)
    (include/sam6d_hip.h: s6d_coco_match).  The group table is checked here, on the host."""
    _chk(ious, torch.float64, "ious", 1)
    _chk(iou_off, torch.int64, "iou_off", 1)
    _chk(groups, torch.int32, "groups", 2)
    _chk(det_area, torch.float64, "det_area", 1)
    _chk(gt_area, torch.float64, "gt_area", 1)
    _chk(gt_ignore, torch.uint8, "gt_ignore", 1)
    _chk(thresholds, torch.float64, "thresholds", 1)
    _chk(area_ranges, torch.float64, "area_ranges", 2)
    n, NT, NA, Dn, Gn = groups.shape[0], thresholds.shape[0], area_ranges.shape[0], det_area.shape[0], gt_area.shape[0]
    if groups.shape[1] != 4 or tuple(iou_off.shape) != (n,) or tuple(gt_ignore.shape) != (Gn,) or area_ranges.shape[1] != 2 or \
            NT < 1 or NA < 1 or NT * NA > 64:
        raise ValueError(f"coco_match: groups (n,4), iou_off (n,), gt_area and gt_ignore (Gn,), thresholds (NT,), area_ranges (NA,2) with "
                         f"NT NA <= 64 expected, got {tuple(groups.shape)}, {tuple(iou_off.shape)}, {tuple(gt_area.shape)}, "
                         f"{tuple(gt_ignore.shape)}, {tuple(thresholds.shape)}, {tuple(area_ranges.shape)}")
    if n:
        g, o = groups.long(), iou_off
        bad = (g < 0).any() | (o < 0).any() | (g[:, 0] + g[:, 1] > Dn).any() | (g[:, 2] + g[:, 3] > Gn).any() | \
            (o + g[:, 1] * g[:, 3] > ious.shape[0]).any()
        if bool(bad):
            raise ValueError("coco_match: a group lies outside the detection, ground-truth or IoU arrays")
        if int(g[:, 3].max()) > _lib.header_constant("S6D_COCO_MATCH_MAX_GT"):
            raise ValueError(f"coco_match: a group has {int(g[:, 3].max())} ground truths, more than S6D_COCO_MATCH_MAX_GT")
    params = torch.cat([thresholds, area_ranges.reshape(-1)]).contiguous()
    match = torch.full((Dn, NT, NA), -1, dtype=torch.int32, device=groups.device)
    ignore = torch.zeros(Dn, NT, NA, dtype=torch.uint8, device=groups.device)
    _call("s6d_coco_match", _ptr(ious), _ptr(iou_off), _ptr(groups), _ptr(det_area), _ptr(gt_area), _ptr(gt_ignore), _ptr(params), n,
          NT, NA, Dn, Gn, ious.shape[0], _ptr(match), _ptr(ignore), _stream())
    return match, ignore


# ------------------------------------------------------------------ connected components / small mask regions (csrc/s6d_ccl.hip)
SMALL_REGIONS_WORKSPACE_BYTES = 512 << 20      # masks go through the kernels in chunks whose workspace (two int32 planes) stays under this
CCL_TILE = (_lib.header_constant("S6D_CCL_TILE_H"), _lib.header_constant("S6D_CCL_TILE_W"))


def _binary_masks(masks, what):
    if masks.dtype == torch.bool and masks.is_cuda and masks.is_contiguous():
        masks = masks.view(torch.uint8)
    _chk(masks, torch.uint8, "masks", 3)
    N, H, W = masks.shape
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"{what}: masks (N,H,W) with 1 <= H W < 2^31 expected, got {tuple(masks.shape)}")
    per_mask = _size("s6d_small_regions_workspace_bytes", 1, H, W)
    return masks, max(1, SMALL_REGIONS_WORKSPACE_BYTES // per_mask)


def label_components(masks, background=False):
    """masks (N,H,W) uint8 or bool (non-zero = set) -> labels (N,H,W) int32: the 8-connected components of the set pixels (of the
    unset ones with ``background``); a pixel's label is the row-major index of the first pixel of its component, -1 on the other
    polarity (include/sam6d_hip.h: s6d_label_components_u8).  Processed in chunks of masks; a mask's labels do not depend on them."""
    masks, chunk = _binary_masks(masks, "label_components")
    N, H, W = masks.shape
    labels = torch.empty(N, H, W, dtype=torch.int32, device=masks.device)
    for a in range(0, N, chunk):
        n = min(chunk, N - a)
        ws = torch.empty(_size("s6d_small_regions_workspace_bytes", n, H, W), dtype=torch.uint8, device=masks.device)
        _call("s6d_label_components_u8", _ptr(masks[a:a + n]), n, H, W, int(bool(background)), _ptr(ws), _ptr(labels[a:a + n]), _stream())
    return labels


def remove_small_regions(masks, min_area):
    """masks (N,H,W) uint8 or bool, min_area >= 1 -> (masks (N,H,W) uint8 0 / 1, changed (N,) bool, boxes (N,4) int32 XYXY, inclusive
    maximum corner, zeros for an empty mask): holes (components of unset pixels) with area < min_area filled, then islands with
    area < min_area removed -- the largest kept when all are small (include/sam6d_hip.h: s6d_remove_small_regions_u8).  Processed in
    chunks of masks; a mask's result does not depend on them."""
    masks, chunk = _binary_masks(masks, "remove_small_regions")
    if int(min_area) != min_area or min_area < 1:
        raise ValueError(f"remove_small_regions: min_area must be an integer >= 1, got {min_area!r}")
    N, H, W = masks.shape
    dev = masks.device
    out = torch.empty(N, H, W, dtype=torch.uint8, device=dev)
    changed = torch.empty(N, dtype=torch.bool, device=dev)
    boxes = torch.empty(N, 4, dtype=torch.int32, device=dev)
    for a in range(0, N, chunk):
        n = min(chunk, N - a)
        ws = torch.empty(_size("s6d_small_regions_workspace_bytes", n, H, W), dtype=torch.uint8, device=dev)
        _call("s6d_remove_small_regions_u8", _ptr(masks[a:a + n]), n, H, W, int(min_area), _ptr(ws), _ptr(out[a:a + n]),
              _ptr(changed[a:a + n]), _ptr(boxes[a:a + n]), _stream())
    return out, changed, boxes


# ------------------------------------------------------------------ run-length masks (csrc/s6d_rle.hip)
RLE_BAND_WORDS = _lib.header_constant("S6D_RLE_BAND_WORDS")
_RLE_OK = 2 ** 31 - 1


def set_rle_band_words(words):
    """LDS capacity of a column band of the run-length kernels in 64-bit words, 0 = the default (include/sam6d_hip.h:
    s6d_set_rle_band_words): lets tests cross band seams at small shapes; same results for every setting."""
    _call("s6d_set_rle_band_words", int(words))


def rle_encode(masks):
    """masks (N,H,W) uint8 or bool (non-zero = set) -> (counts (R,) int32, offsets (N+1,) int64): the canonical column-major run
    lists of every mask, the list of mask n being counts[offsets[n]:offsets[n+1]] (include/sam6d_hip.h: s6d_rle_count_u8,
    s6d_rle_write_u8).  The exclusive scan of the per-mask run counts between the two kernels is ``torch.cumsum``."""
    if masks.dtype == torch.bool and masks.is_cuda and masks.is_contiguous():
        masks = masks.view(torch.uint8)
    _chk(masks, torch.uint8, "masks", 3)
    N, H, W = masks.shape
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"rle_encode: masks (N,H,W) with 1 <= H W < 2^31 expected, got {tuple(masks.shape)}")
    dev = masks.device
    offsets = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    if N == 0:
        return torch.empty(0, dtype=torch.int32, device=dev), offsets
    nbytes = _size("s6d_rle_encode_workspace_bytes", N, H, W)
    if nbytes < 0:
        raise ValueError(f"rle_encode: s6d_rle_encode_workspace_bytes refuses N = {N}, H = {H}, W = {W} (a column of H pixels must fit "
                         f"the band capacity, 64 pixels per word)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    runs =torch.empty(N, dtype=torch.int32, device=dev)
    _call("s6d_rle_count_u8", _ptr(masks), N, H, W, _ptr(ws), _ptr(runs), _stream())
    torch.cumsum(runs, 0, dtype=torch.int64, out=offsets[1:])
    R = int(offsets[-1])
    edges = torch.empty(R, dtype=torch.int32, device=dev)
    counts = torch.empty(R, dtype=torch.int32, device=dev)
    _call("s6d_rle_write_u8", _ptr(masks), N, H, W, _ptr(ws), _ptr(offsets), R, _ptr(edges), _ptr(counts), _stream())
    return counts, offsets


def _rle_operands(counts, offsets, H, W, what):
    _chk(counts, torch.int32, "counts", 1)
    _chk(offsets, torch.int64, "offsets", 1)
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"{what}: 1 <= H W < 2^31 expected, got H = {H}, W = {W}")
    N, R = offsets.shape[0] - 1, counts.shape[0]
    if N < 0:
        raise ValueError(f"{what}: offsets (N+1,) expected, got {tuple(offsets.shape)}")
    o = offsets.cpu()
    if int(o[0]) != 0 or int(o[-1]) != R or (N and bool((o[1:] < o[:-1]).any())):
        raise ValueError(f"{what}: offsets must be non-decreasing from 0 to len(counts) = {R}, got {int(o[0])} .. {int(o[-1])}")
    if N and bool((o[1:] == o[:-1]).any()):
        raise ValueError(f"{what}: mask {int(torch.nonzero(o[1:] == o[:-1])[0, 0])} has an empty run list")
    ends = torch.cumsum(counts, 0, dtype=torch.int64)                     # the run starts: a library scan
    status = torch.empty(N + 1, dtype=torch.int32, device=counts.device)
    return N, R, H, W, ends, status


def _rle_refusal(status, what, H, W):
    bad = int(status[0])
    if bad != _RLE_OK:
        raise ValueError(f"{what}: mask {bad} is not a run list of {H} x {W} pixels (a negative count, or the counts do not sum to "
                         f"{H * W})")


def rle_to_packed(counts, offsets, H, W):
    """counts (R,) int32, offsets (N+1,) int64, run lists in column-major order -> (packed (N, ceil(H W / 64)) int64, area (N,)
    int32), exactly ``mask_pack`` of the dense masks, which are never made (include/sam6d_hip.h: s6d_rle_to_packed).  Zero-length
    runs are accepted anywhere; a negative count, an empty list or a total other than H W raises ValueError naming the first such
    mask."""
    N, R, H, W, ends, status = _rle_operands(counts, offsets, H, W, "rle_to_packed")
    packed = torch.empty(N, (H * W + 63) // 64, dtype=torch.int64, device=counts.device)
    area = torch.empty(N, dtype=torch.int32, device=counts.device)
    if N == 0:
        return packed, area
    _call("s6d_rle_to_packed", _ptr(counts), _ptr(offsets), _ptr(ends), N, R, H, W, _ptr(status), _ptr(packed), _ptr(area), _stream())
    _rle_refusal(status, "rle_to_packed", H, W)
    return packed, area


def rle_to_masks(counts, offsets, H, W):
    """counts (R,) int32, offsets (N+1,) int64 -> dense masks (N,H,W) uint8 0 / 1 (include/sam6d_hip.h: s6d_rle_to_masks_u8); accepts
    and refuses what ``rle_to_packed`` does."""
    N, R, H, W, ends, status = _rle_operands(counts, offsets, H, W, "rle_to_masks")
    masks = torch.empty(N, H, W, dtype=torch.uint8, device=counts.device)
    if N == 0:
        return masks
    _call("s6d_rle_to_masks_u8", _ptr(counts), _ptr(offsets), _ptr(ends), N, R, H, W, _ptr(status), _ptr(masks), _stream())
    _rle_refusal(status, "rle_to_masks", H, W)
    return masks


def upsample_gather(up, choose, H, W, C):
    """up (B,196,16*C) f32, choose (B,n) int64 -> (B,n,C): bilinear x4 of the pixel-shuffled map at chosen pixels."""
    _chk(up, torch.float32, "up", 3)
    _chk(choose, torch.int64, "choose", 2)
    B, T, PC = up.shape
    G = int(round(T ** 0.5))
    P = int(round((PC // C) ** 0.5))
    n = choose.shape[1]
    out = torch.empty(B, n, C, dtype=torch.float32, device=up.device)
    _call("s6d_upsample_gather_f32", _ptr(up), _ptr(choose), B, n, G, P, C, int(H), int(W), _ptr(out), _stream())
    return out


# ------------------------------------------------------------------ SAM image encoder
_REL_PAD = {}


def _padded_rel(rel_h, rel_w, H, window, hd):
    """The zero-padded copies of a (rel_h, rel_w) table pair in the layout the attention kernels read (s6d_win_attention_pad_rel_bf16),
    cached on the identity and version of the two tensors (the modules hand in their own cached bf16 tables)."""
    key = (id(rel_h), id(rel_w), H, window, hd)
    c = _REL_PAD.get(key)
    if c is None or c[0] is not rel_h or c[1] is not rel_w or c[2] != (rel_h._version, rel_w._version):
        pad = torch.empty(_size("s6d_win_attention_scratch_bytes", H, window, hd), dtype=torch.uint8, device=rel_h.device)
        _call("s6d_win_attention_pad_rel_bf16", _ptr(rel_h), _ptr(rel_w), H, window, hd, _ptr(pad), _stream())
        if len(_REL_PAD) > 256:
            _REL_PAD.clear()
        c = (rel_h, rel_w, (rel_h._version, rel_w._version), pad)
        _REL_PAD[key] = c
    return c[3]


def window_attention(qkv, qkv_bias, rel_h, rel_w, num_heads, window, scale, head_major_shape=None):
    """qkv (B,H,W,3C) bf16, qkv_bias (3C) bf16, rel_h/rel_w (2S-1,hd) bf16 or None -> (B,H,W,C) bf16.
    head_major_shape=(B,H,W): qkv is the head-major tensor (3*num_heads, B*H*W, hd) that gemm_bf16(..., col_block=hd) writes."""
    _chk(qkv_bias, torch.bfloat16, "qkv_bias", 1)
    if head_major_shape is None:
        _chk(qkv, torch.bfloat16, "qkv", 4)
        B, H, W, C3 = qkv.shape
        C = C3 // 3
        hd = C // num_heads
    else:
        _chk(qkv, torch.bfloat16, "qkv", 3)
        B, H, W = head_major_shape
        hd = qkv.shape[2]
        C = num_heads * hd
        if tuple(qkv.shape) != (3 * num_heads, B * H * W, hd):
            raise RuntimeError(f"head-major qkv must be (3*heads, B*H*W, hd); got {tuple(qkv.shape)} for B,H,W={head_major_shape}")
    if rel_h is not None:
        _chk(rel_h, torch.bfloat16, "rel_h", 2)
        _chk(rel_w, torch.bfloat16, "rel_w", 2)
        S = window if window > 0 else H
        if rel_h.shape != (2 * S - 1, hd) or rel_w.shape != (2 * S - 1, hd):
            raise RuntimeError("rel_pos tables must be (2S-1, head_dim)")
    out = torch.empty(B, H, W, C, dtype=torch.bfloat16, device=qkv.device)
    if rel_h is not None:
        # the padded copies of the two tables the kernels read are a function of the tables only: made once per (table pair, grid,
        # window) and kept (round 6: the padding ran as a 5-us launch in front of each of the 64 attention launches of a step)
        _call("s6d_win_attention_prepadded_bf16", _ptr(qkv), 0 if head_major_shape is None else 1, _ptr(qkv_bias),
              _ptr(_padded_rel(rel_h, rel_w, H, int(window), int(hd))), B, H, W, int(num_heads), int(hd), int(window), scale, _ptr(out),
              _stream())
        return out
    _call("s6d_win_attention_layout_bf16", _ptr(qkv), 0 if head_major_shape is None else 1, _ptr(qkv_bias), None, None, B, H, W,
          int(num_heads), int(hd), int(window), scale, None, _ptr(out), _stream())
    return out


def _half(t, name, ndim=None):
    """bf16 or IEEE-half tensor -> symbol suffix of the kernel family compiled for that element type."""
    if t.dtype not in (torch.bfloat16, torch.float16):
        raise RuntimeError(f"{name} must be a bfloat16 or float16 tensor")
    _chk(t, t.dtype, name, ndim)
    return "bf16" if t.dtype == torch.bfloat16 else "f16"


def seq_attention(qkv, num_heads, scale, seq_len=None):
    """softmax(scale q k^T) v per head, no positional bias.  qkv (B,N,3C) bf16 or f16 token-major (the raw Linear output), or --
    with ``seq_len`` = N -- HEAD-major (3 * num_heads, B * N, hd), what ``gemm_bf16(..., col_block=hd)`` / ``gemm_bf16_lnfold(...,
    col_block=hd)`` return: the K / V rows of a (sequence, head) are then one contiguous run instead of N pieces of hd elements
    strided by 3C (the fetch of those pieces alone costs 136 us per 150 x 16 x 257 launch).  -> (B,N,C) in qkv's dtype."""
    sfx = _half(qkv, "qkv", 3)
    if seq_len is None:
        B, N, C3 = qkv.shape
        C = C3 // 3
        out = torch.empty(B, N, C, dtype=qkv.dtype, device=qkv.device)
        _call("s6d_seq_attention_" + sfx, _ptr(qkv), B, N, int(num_heads), int(C // num_heads), scale, _ptr(out), _stream())
        return out
    H3, M, hd = qkv.shape
    N = int(seq_len)
    if H3 != 3 * num_heads or M % N:
        raise ValueError(f"head-major qkv must be (3 * num_heads, B * N, hd); got {tuple(qkv.shape)} for {num_heads} heads, N = {N}")
    B = M // N
    out = torch.empty(B, N, num_heads * hd, dtype=qkv.dtype, device=qkv.device)
    _call("s6d_seq_attention_strided_" + sfx, _ptr(qkv), hd, num_heads * M * hd, M * hd, B, N, int(num_heads), hd, scale, _ptr(out),
          _stream())
    return out


def gemm_bf16(a, w, bias=None, gelu=False, out=None, max_blocks=0, col_block=0, residual=None, stats_partial=None):
    """a (..., K) bf16 (rows may be strided), w (N, K) bf16 = nn.Linear.weight, bias (N) f32 or None ->
    act(a @ w.T + bias) (..., N) bf16 with act = exact GELU or identity; N % 128 == 0, K % 64 == 0.
    col_block > 0: the output comes back as (N / col_block, M, col_block) -- column blocks as separate matrices (N % 256 == 0).
    residual (..., N) bf16: returns bf16(a @ w.T + bias + residual), summed in fp32 (N % 256 == 0, no GELU); out may be the residual
    itself.  stats_partial (N / 32, 2, M) f32 (with residual): receives the partial LayerNorm statistics of the result rows
    (ln_stats_finalize turns them into (mean, rstd))."""
    if not a.is_cuda or not w.is_cuda:
        raise RuntimeError("a and w must be CUDA tensors")
    if a.dtype not in (torch.bfloat16, torch.float16) or w.dtype != a.dtype:
        raise RuntimeError("a and w must both be bfloat16 (or both float16) tensors")
    f16 = a.dtype == torch.float16          # IEEE half: the same kernel on v_mfma_f32_32x32x16_f16 (plain / GELU epilogue, N % 256 == 0)
    if f16 and (col_block or residual is not None):
        raise RuntimeError("the float16 GEMM has the plain and the GELU epilogue only")
    K = a.shape[-1]
    N = w.shape[0]
    a2 = a.reshape(-1, K)
    if a2.stride(1) != 1 or a2.stride(0) % 8 or a2.data_ptr() % 16:
        a2 = a2.contiguous()
    if w.dim() != 2 or w.shape[1] != K or w.stride(1) != 1 or w.stride(0) % 8:
        raise RuntimeError("w must be (N, K) with contiguous rows")
    if bias is not None:
        _chk(bias, torch.float32, "bias", 1)
    M = a2.shape[0]
    if col_block:
        if out is not None:
            raise RuntimeError("col_block output is allocated by the call")
        out = torch.empty(N // col_block, M, col_block, dtype=torch.bfloat16, device=a.device)   # (bf16 only: checked above)
        _call("s6d_gemm_bf16_cblk", _ptr(a2), a2.stride(0), _ptr(w), w.stride(0), _ptr(bias), _ptr(out), N, M, N, K, 1 if gelu else 0,
              int(col_block), int(max_blocks), _stream())
        return out
    if out is None:
        out = torch.empty(M, N, dtype=a.dtype, device=a.device)
    else:
        _chk(out, a.dtype, "out", 2)
        if tuple(out.shape) != (M, N) or out.stride(1) != 1 or out.stride(0) % 8 or out.data_ptr() % 16:
            raise ValueError(f"out must be ({M}, {N}) bf16 with contiguous, 16-byte aligned rows (stride % 8 == 0); got "
                             f"{tuple(out.shape)} strides {tuple(out.stride())}")
    # the kernel's staging addresses are 32-bit byte offsets from A: rows go through in slabs below 2 GiB (ViT-H lin2 reaches
    # the limit at 52 frames per call)
    rows = gemm_one_launch_rows(a2.stride(0))
    if residual is not None:
        if gelu or col_block:
            raise RuntimeError("the residual form takes neither GELU nor column blocks")
        _chk(residual, torch.bfloat16, "residual")
        r2 = residual.reshape(-1, N)
        if r2.shape[0] != M:
            raise ValueError(f"residual has {r2.shape[0]} rows, the product {M}")
        if r2.stride(1) != 1 or r2.stride(0) % 8 or r2.data_ptr() % 16:
            raise ValueError("residual rows must be contiguous and 16-byte aligned")
        if stats_partial is not None:
            _chk(stats_partial, torch.float32, "stats_partial")
            if tuple(stats_partial.shape) != (N // 32, 2, M) or not stats_partial.is_contiguous():
                raise ValueError(f"stats_partial must be a contiguous ({N // 32}, 2, {M}) f32 tensor; got {tuple(stats_partial.shape)}")
            if M > rows:
                raise RuntimeError("row statistics are written for one launch: the row count exceeds one 2-GiB slab")
        for r0 in range(0, M, rows):
            r1 = min(M, r0 + rows)
            _call("s6d_gemm_bf16_res", _ptr(a2[r0:r1]), a2.stride(0), _ptr(w), w.stride(0), _ptr(bias), _ptr(r2[r0:r1]), r2.stride(0),
                  _ptr(stats_partial), _ptr(out[r0:r1]), out.stride(0), r1 - r0, N, K, int(max_blocks), _stream())
        return out.reshape(*a.shape[:-1], N)
    if stats_partial is not None:
        raise RuntimeError("stats_partial comes with the residual form")
    for r0 in range(0, M, rows):
        r1 = min(M, r0 + rows)
        _call("s6d_gemm_f16" if f16 else "s6d_gemm_bf16", _ptr(a2[r0:r1]), a2.stride(0), _ptr(w), w.stride(0), _ptr(bias), _ptr(out[r0:r1]),
              out.stride(0), r1 - r0, N, K, 1 if gelu else 0, int(max_blocks), _stream())
    return out.reshape(*a.shape[:-1], N)


def set_geo_embed_form(form):
    """Which kernel serves the pre-split geometric embedding (include/sam6d_hip.h: s6d_set_geo_embed_form): 1 = the two-phase kernel
    of rounds 3-5 (default), 2 = registers-built sinusoid fragments + LDS-DMA weight slices (round 6).  Same bits."""
    _call("s6d_set_geo_embed_form", int(form))


def set_gemm_small_tile(enable):
    """256 x 128 tiles for under-filled plain / GELU GEMM launches (include/sam6d_hip.h: s6d_set_gemm_small_tile); same bits either way."""
    _call("s6d_set_gemm_small_tile", int(enable))                  # False / True / 2 (= also the residual epilogue)


def set_gemm_wave_tile(columns):
    """Which form of the bf16 / f16 GEMM kernel serves the shapes both cover (include/sam6d_hip.h: s6d_set_gemm_wave_tile): 0 = the
    library's choice per shape, 64 = the eight-wave form, 128 = the four-wave form wherever it applies.  Process-wide; for A/B
    measurements and the parity tests (the two forms give the same bits)."""
    _call("s6d_set_gemm_wave_tile", int(columns))


def set_gemm_mfma_shape(rows):
    """Which bf16 matrix instruction the eight-wave and the 256 x 128 GEMM forms use (include/sam6d_hip.h: s6d_set_gemm_mfma_shape):
    0 = the library's choice (16 while the wave tile is not pinned), 16 = 16x16x32, 32 = 32x32x16.  Process-wide."""
    _call("s6d_set_gemm_mfma_shape", int(rows))


def gemm_one_launch_rows(row_stride, elem_bytes=2):
    """Rows ONE launch of the bf16 / f16 GEMM kernels takes for an A operand of ``row_stride`` elements per row: their staging
    addresses are 32-bit byte offsets from A, so a launch stays below 2 GiB, in whole 256-row tiles.  The plain forms walk larger
    inputs in slabs of this many rows; the forms that carry row statistics (residual + stats_partial, lnfold) are one launch, so
    their callers' eligibility checks use this very number (one helper instead of three bounds)."""
    return max(256, ((2 ** 31 - 1) // (elem_bytes * int(row_stride))) // 256 * 256)


def ln_stats_finalize(stats_partial, group_size=32, eps=1e-6):
    """(groups, 2, M) f32 partial statistics (gemm_bf16(..., stats_partial=)) -> (M, 2) f32 rows of (mean, sigma = sqrt(var + eps))."""
    _chk(stats_partial, torch.float32, "stats_partial", 3)
    if not stats_partial.is_contiguous() or stats_partial.shape[1] != 2:
        raise ValueError("stats_partial must be a contiguous (groups, 2, M) tensor")
    G, _, M = stats_partial.shape
    out = torch.empty(M, 2, dtype=torch.float32, device=stats_partial.device)
    _call("s6d_ln_stats_finalize", _ptr(stats_partial), G, int(group_size), M, eps, _ptr(out), _stream())
    return out


def row_stats(x, eps=1e-6):
    """x (..., C) bf16 -> (rows, 2) f32 of (mean, sigma = sqrt(var + eps)) over the last dim: the LayerNorm statistics alone."""
    _chk(x, torch.bfloat16, "x")
    C = x.shape[-1]
    x2 = x.reshape(-1, C)
    if x2.stride(1) != 1 or x2.stride(0) % 8 or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    out = torch.empty(x2.shape[0], 2, dtype=torch.float32, device=x.device)
    _call("s6d_row_stats_bf16", _ptr(x2), x2.stride(0), x2.shape[0], C, eps, _ptr(out), _stream())
    return out


def gemm_bf16_lnfold(a, stats, w_folded, col_sums, bias, gelu=False, col_block=0, max_blocks=0):
    """act(LayerNorm(a) @ W.T + b) without the normalised activations: a (..., K) bf16 raw rows, stats (rows, 2) f32 their
    (mean, sigma), w_folded (N, K) bf16 = gamma * W, col_sums (N) f32 = w_folded.float().sum(1), bias (N) f32 = b + W @ beta
    (sam6d_amd/utils/linear.py::lnfold_weights).  N % 256 == 0.  col_block as gemm_bf16."""
    _chk(a, torch.bfloat16, "a")
    _chk(w_folded, torch.bfloat16, "w_folded", 2)
    _chk(stats, torch.float32, "stats", 2)
    _chk(col_sums, torch.float32, "col_sums", 1)
    _chk(bias, torch.float32, "bias", 1)
    K, N = a.shape[-1], w_folded.shape[0]
    a2 = a.reshape(-1, K)
    if a2.stride(1) != 1 or a2.stride(0) % 8 or a2.data_ptr() % 16:
        a2 = a2.contiguous()
    M = a2.shape[0]
    if w_folded.shape[1] != K or w_folded.stride(1) != 1 or w_folded.stride(0) % 8:
        raise RuntimeError("w_folded must be (N, K) with contiguous rows")
    if tuple(stats.shape) != (M, 2) or not stats.is_contiguous() or col_sums.numel() != N or bias.numel() != N:
        raise ValueError(f"stats must be ({M}, 2), col_sums and bias ({N},)")
    if M > gemm_one_launch_rows(a2.stride(0)):
        raise RuntimeError("one launch: the row count exceeds one 2-GiB slab")
    if col_block:
        out = torch.empty(N // col_block, M, col_block, dtype=torch.bfloat16, device=a.device)
    else:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    _call("s6d_gemm_bf16_lnfold", _ptr(a2), a2.stride(0), _ptr(stats), _ptr(w_folded), w_folded.stride(0), _ptr(col_sums), _ptr(bias),
          _ptr(out), N, M, N, K, 1 if gelu else 0, int(col_block), int(max_blocks), _stream())
    return out if col_block else out.reshape(*a.shape[:-1], N)


def gemm_fp8(a8, a_scale, w8, w_scale, bias=None, gelu=False, max_blocks=0):
    """a8 (..., K) uint8 (e4m3fn bytes) with a_scale (rows,) uint8 (E8M0), w8 (N, K) uint8 with w_scale (N,) uint8, bias (N) f32
    or None -> act(A W^T + bias) (..., N) bf16 on the fp8 matrix cores (sam6d_amd/utils/fp8.py: the operand format).
    N % 256 == 0, K % 128 == 0."""
    for t, nm in ((a8, "a8"), (a_scale, "a_scale"), (w8, "w8"), (w_scale, "w_scale")):
        _chk(t, torch.uint8, nm)
    K, N = a8.shape[-1], w8.shape[0]
    a2 = a8.reshape(-1, K)
    M = a2.shape[0]
    if w8.shape != (N, K) or a_scale.numel() != M or w_scale.numel() != N:
        raise ValueError(f"shapes: a8 {tuple(a8.shape)}, a_scale {tuple(a_scale.shape)}, w8 {tuple(w8.shape)}, w_scale {tuple(w_scale.shape)}")
    if bias is not None:
        _chk(bias, torch.float32, "bias", 1)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=a8.device)
    rows = max(256, ((2 ** 31 - 1) // K) // 256 * 256)
    for r0 in range(0, M, rows):
        r1 = min(M, r0 + rows)
        _call("s6d_gemm_fp8", _ptr(a2[r0:r1]), K, _ptr(a_scale.reshape(-1)[r0:r1]), _ptr(w8), K, _ptr(w_scale), _ptr(bias),
              _ptr(out[r0:r1]), N, r1 - r0, N, K, 1 if gelu else 0, int(max_blocks), _stream())
    return out.reshape(*a8.shape[:-1], N)


def gemm_fp8_gelu_mx(a8, a_scale, w8, w_scale, bias=None, max_blocks=0):
    """lin1 of the fp8 block with an MX output: a8 (..., K) uint8 e4m3 + a_scale (rows,) uint8, w8 (N, K) + w_scale (N,) ->
    (q (rows, N) uint8 = e4m3(GELU(A W^T + bias)), s (rows, N / 32) uint8 = one E8M0 scale per row and 32 columns): the MX A operand
    of gemm_fp8_mxa.  N % 256 == 0, K % 128 == 0; one launch (rows * K < 2^31)."""
    for t, nm in ((a8, "a8"), (a_scale, "a_scale"), (w8, "w8"), (w_scale, "w_scale")):
        _chk(t, torch.uint8, nm)
    K, N = a8.shape[-1], w8.shape[0]
    a2 = a8.reshape(-1, K)
    M = a2.shape[0]
    if w8.shape != (N, K) or a_scale.numel() != M or w_scale.numel() != N:
        raise ValueError(f"shapes: a8 {tuple(a8.shape)}, a_scale {tuple(a_scale.shape)}, w8 {tuple(w8.shape)}, w_scale {tuple(w_scale.shape)}")
    if bias is not None:
        _chk(bias, torch.float32, "bias", 1)
    if M * K >= 2 ** 31:
        raise RuntimeError("one launch: the row count exceeds one 2-GiB slab")
    q = torch.empty(M, N, dtype=torch.uint8, device=a8.device)
    Mp = (M + 255) // 256 * 256                 # the consumer fetches the scale dwords of whole 256-row tiles: the rows exist
    s = torch.zeros(Mp, N // 32, dtype=torch.uint8, device=a8.device)[:M]
    _call("s6d_gemm_fp8_gelu_mx", _ptr(a2), K, _ptr(a_scale.reshape(-1)), _ptr(w8), K, _ptr(w_scale), _ptr(bias), _ptr(q), N, _ptr(s), M, N,
          K, int(max_blocks), _stream())
    return q, s


def gemm_fp8_mxa(a8, a_mx, w8, w_scale, bias=None, gelu=False, max_blocks=0):
    """a8 (rows, K) uint8 e4m3 with a_mx (rows, K / 32) uint8 MX block scales (gemm_fp8_gelu_mx's outputs), w8 (N, K) uint8 with
    w_scale (N,) -> act(A W^T + bias) (rows, N) bf16.  rows % 256 == 0, N % 256 == 0, K % 128 == 0."""
    for t, nm in ((a8, "a8"), (a_mx, "a_mx"), (w8, "w8"), (w_scale, "w_scale")):
        _chk(t, torch.uint8, nm)
    K, N = a8.shape[-1], w8.shape[0]
    a2 = a8.reshape(-1, K)
    M = a2.shape[0]
    if w8.shape != (N, K) or tuple(a_mx.shape) != (M, K // 32) or w_scale.numel() != N:
        raise ValueError(f"shapes: a8 {tuple(a8.shape)}, a_mx {tuple(a_mx.shape)}, w8 {tuple(w8.shape)}, w_scale {tuple(w_scale.shape)}")
    if bias is not None:
        _chk(bias, torch.float32, "bias", 1)
    if M * K >= 2 ** 31:
        raise RuntimeError("one launch: the row count exceeds one 2-GiB slab")
    Mp = (M + 255) // 256 * 256
    if a_mx.untyped_storage().nbytes() - a_mx.storage_offset() < Mp * (K // 32):
        pad = torch.zeros(Mp, K // 32, dtype=torch.uint8, device=a8.device)
        pad[:M] = a_mx
        a_mx = pad[:M]
    out = torch.empty(M, N, dtype=torch.bfloat16, device=a8.device)
    _call("s6d_gemm_fp8_mxa", _ptr(a2), K, _ptr(a_mx), _ptr(w8), K, _ptr(w_scale), _ptr(bias), _ptr(out), N, M, N, K, 1 if gelu else 0,
          int(max_blocks), _stream())
    return out


def layernorm_fp8(x, gamma, beta, eps, delta=None):
    """x (..., C) bf16 -> (LN(x) as e4m3fn bytes (..., C) uint8, one E8M0 scale byte per row (rows,) uint8).
    delta (same shape, bf16): -> (x + delta, bytes, scales) with the residual add folded in, as add_layernorm."""
    _chk(x, torch.bfloat16, "x")
    _chk(gamma, torch.float32, "gamma", 1)
    _chk(beta, torch.float32, "beta", 1)
    C = x.shape[-1]
    if gamma.numel() != C or beta.numel() != C:
        raise ValueError(f"gamma / beta must have {C} elements")
    if delta is not None and delta.shape != x.shape:
        raise ValueError("delta must have x's shape")
    rows = x.numel() // C
    y8 = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    ys = torch.empty(rows, dtype=torch.uint8, device=x.device)
    if delta is None:
        _call("s6d_layernorm_fp8", _ptr(x), _ptr(gamma), _ptr(beta), eps, rows, C, _ptr(y8), _ptr(ys), _stream())
        return y8, ys
    _chk(delta, torch.bfloat16, "delta")
    xo = torch.empty_like(x)
    _call("s6d_add_layernorm_fp8", _ptr(x), _ptr(delta), _ptr(gamma), _ptr(beta), eps, rows, C, _ptr(xo), _ptr(y8), _ptr(ys), _stream())
    return xo, y8, ys


def split_weight(w):
    """W (N,K) f32 -> (hi, lo) bf16 parts for linear_f32 (W = hi + lo up to 2^-17 relative)."""
    _chk(w, torch.float32, "w")
    hi = torch.empty(w.shape, dtype=torch.bfloat16, device=w.device)
    lo = torch.empty(w.shape, dtype=torch.bfloat16, device=w.device)
    _call("s6d_linear_split_weight_f32", _ptr(w), w.numel(), _ptr(hi), _ptr(lo), _stream())
    return hi, lo


def linear_f32(x, w_hi, w_lo, bias=None, relu=False, residual=None, ln=None):
    """y = LN(residual + act(x W^T + bias)) in one kernel: x (..., K) f32, (w_hi, w_lo) = split_weight(W (N,K)), bias (N) or None,
    residual (..., N) or None, ln = (gamma, beta, eps) or None (N == 256).  K % 32 == 0, N % 256 == 0."""
    _chk(x, torch.float32, "x")
    _chk(w_hi, torch.bfloat16, "w_hi", 2)
    _chk(w_lo, torch.bfloat16, "w_lo", 2)
    if w_lo.shape != w_hi.shape:
        raise ValueError(f"w_hi {tuple(w_hi.shape)} and w_lo {tuple(w_lo.shape)} differ in shape")
    N, K = w_hi.shape
    if x.shape[-1] != K:
        raise ValueError(f"x has {x.shape[-1]} columns, W {K}")
    x2 = x.reshape(-1, K)
    M = x2.shape[0]
    y = torch.empty(M, N, dtype=torch.float32, device=x.device)
    r2 = None
    if residual is not None:
        _chk(residual, torch.float32, "residual")
        r2 = residual.reshape(-1, N)
        if r2.shape[0] != M:
            raise ValueError("residual rows != x rows")
    g = bt = None
    eps = 0.0
    if ln is not None:
        g, bt, eps = ln
        _chk(g, torch.float32, "gamma", 1)
        _chk(bt, torch.float32, "beta", 1)
        if g.numel() != N or bt.numel() != N:
            raise ValueError(f"gamma / beta must have {N} elements")
    if bias is not None:
        _chk(bias, torch.float32, "bias", 1)
        if bias.numel() != N:
            raise ValueError(f"bias must have {N} elements")
    _call("s6d_linear_f32", _ptr(x2), x2.stride(0), M, K, _ptr(w_hi), _ptr(w_lo), _ptr(bias), N, 1 if relu else 0, _ptr(r2),
          r2.stride(0) if r2 is not None else 0, _ptr(g), _ptr(bt), eps, _ptr(y), N, _stream())
    return y.reshape(*x.shape[:-1], N)


def fragment_weight(w):
    """w (N, K) bf16 (a part of split_weight's output) -> the same elements in matrix-instruction fragment order (s6d_linear_fragment_weight),
    the weight format of attn_output_chain."""
    _chk(w, torch.bfloat16, "w", 2)
    w = w.contiguous()
    out = torch.empty_like(w)
    _call("s6d_linear_fragment_weight", _ptr(w), w.shape[0], w.shape[1], _ptr(out), _stream())
    return out


def attn_output_chain(a, x, w1, ln1, we, ws, ln2):
    """LN2(h + relu(h We^T + be) Ws^T + bs) with h = LN1(x + a W1^T + b1) in one kernel (s6d_attn_output_chain_f32): a, x (..., 256)
    f32; w1 / we / ws = (w_hi, w_lo, bias) of the (256,256) / (512,256) / (256,512) Linear layers (split_weight, each part through
    fragment_weight); ln1 / ln2 =
    (gamma, beta, eps).  Equals linear_f32 x 3 bit for bit."""
    _chk(a, torch.float32, "a")
    _chk(x, torch.float32, "x")
    if a.shape != x.shape or a.shape[-1] != 256:
        raise ValueError(f"a {tuple(a.shape)} and x {tuple(x.shape)} must be (..., 256)")
    for (hi, lo, b), shp in ((w1, (256, 256)), (we, (512, 256)), (ws, (256, 512))):
        _chk(hi, torch.bfloat16, "w_hi", 2)
        _chk(lo, torch.bfloat16, "w_lo", 2)
        _chk(b, torch.float32, "bias", 1)
        if tuple(hi.shape) != shp or tuple(lo.shape) != shp or b.numel() != shp[0] or not (hi.is_contiguous() and lo.is_contiguous()):
            raise ValueError(f"weight parts must be contiguous {shp}")
    for g, bt, _ in (ln1, ln2):
        _chk(g, torch.float32, "gamma", 1)
        _chk(bt, torch.float32, "beta", 1)
    a2, x2 = a.reshape(-1, 256), x.reshape(-1, 256)
    if a2.stride(1) != 1 or a2.stride(0) % 4 or a2.data_ptr() % 16:
        a2 = a2.contiguous()
    if x2.stride(1) != 1 or x2.stride(0) % 4 or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    M = a2.shape[0]
    y = torch.empty(M, 256, dtype=torch.float32, device=a.device)
    _call("s6d_attn_output_chain_f32", _ptr(a2), a2.stride(0), _ptr(x2), x2.stride(0), M, _ptr(w1[0]), _ptr(w1[1]), _ptr(w1[2]),
          _ptr(ln1[0]), _ptr(ln1[1]), ln1[2], _ptr(we[0]), _ptr(we[1]), _ptr(we[2]), _ptr(ws[0]), _ptr(ws[1]), _ptr(ws[2]), _ptr(ln2[0]),
          _ptr(ln2[1]), ln2[2], _ptr(y), 256, _stream())
    return y.reshape(a.shape)


def layernorm_f32out(x, gamma, beta, eps):
    """x (..., C) bf16 -> LN(x) (..., C) float32 (fp32 statistics, no rounding of the result)."""
    _chk(x, torch.bfloat16, "x")
    _chk(gamma, torch.float32, "gamma", 1)
    _chk(beta, torch.float32, "beta", 1)
    C = x.shape[-1]
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _call("s6d_layernorm_bf16_f32", _ptr(x), _ptr(gamma), _ptr(beta), eps, x.numel() // C, C, _ptr(y), _stream())
    return y


def add_layernorm(x, delta, gamma, beta, eps):
    """x (...,C) bf16 or f16, delta same shape / dtype or None, gamma/beta (C) f32 -> (x + delta, LN(x + delta)) in x's dtype."""
    sfx = _half(x, "x")
    _chk(gamma, torch.float32, "gamma", 1)
    _chk(beta, torch.float32, "beta", 1)
    C = x.shape[-1]
    rows = x.numel() // C
    y = torch.empty_like(x)
    if delta is not None:
        _chk(delta, x.dtype, "delta")
        xo = torch.empty_like(x)
    else:
        xo = x
    _call("s6d_add_layernorm_" + sfx, _ptr(x), _ptr(delta), _ptr(gamma), _ptr(beta), eps, rows, C, _ptr(xo) if delta is not None else None,
          _ptr(y), _stream())
    return xo, y


def geo_embedding(idx4, Wd, bd, Wa, ba, div_term, out_dtype=torch.float32, split=None):
    """idx4 (...,4) f32 [d_idx, a_idx x3] -> (...,256) geometric structure embedding, stored in f32 or (out_dtype=torch.float16) in
    IEEE half for the RPE attention core to stream.  split = (Wd_hilo, Wa_hilo): the weights already split into bf16 hi / lo parts,
    each a (2, 256, 256) bf16 tensor [hi | lo] (the caller caches them per weight version): same bits, half the kernel's vector work."""
    for a, nm in ((idx4, "idx4"), (Wd, "Wd"), (bd, "bd"), (Wa, "Wa"), (ba, "ba"), (div_term, "div_term")):
        _chk(a, torch.float32, nm)
    if out_dtype not in (torch.float32, torch.float16):
        raise RuntimeError("the embedding is stored in float32 or float16")
    NP = idx4.numel() // 4
    out = torch.empty(*idx4.shape[:-1], Wd.shape[0], dtype=out_dtype, device=idx4.device)
    if split is not None and have("geo_embedding_split"):
        for a, nm in ((split[0], "Wd_hilo"), (split[1], "Wa_hilo")):
            _chk(a, torch.bfloat16, nm, 3)
        _call("s6d_geo_embedding_split", _ptr(idx4), NP, _ptr(split[0]), _ptr(bd), _ptr(split[1]), _ptr(ba), _ptr(div_term), Wd.shape[0],
              idx4.shape[-1] - 1, _ptr(out), 1 if out_dtype == torch.float16 else 0, _stream())
        return out
    _call("s6d_geo_embedding_f32" if out_dtype == torch.float32 else "s6d_geo_embedding_f16", _ptr(idx4), NP, _ptr(Wd), _ptr(bd), _ptr(Wa),
          _ptr(ba), _ptr(div_term), Wd.shape[0], idx4.shape[-1] - 1, _ptr(out), _stream())
    return out


GEO_POINTS_MAX_N = 256          # clouds the points-fed geometric kernels serve (include/sam6d_hip.h: s6d_geo_indices_f32), 4 <= N


def geo_knn(points):
    """points (B,N,3) f32 -> (B,N,3) i32: the three nearest neighbours of every point besides itself, nearest first, ties to the
    lower index (the neighbour table of the points-fed geometric embedding)."""
    _chk(points, torch.float32, "points", 3)
    if points.shape[-1] != 3:
        raise RuntimeError("points must be (B,N,3)")
    B, N, _ = points.shape
    knn = torch.empty(B, N, 3, dtype=torch.int32, device=points.device)
    _call("s6d_geo_knn_f32", _ptr(points), B, N, _ptr(knn), _stream())
    return knn


def geo_indices(points, sigma_d, factor_a):
    """points (B,N,3) f32 -> idx4 (B,N,N,4) f32 = [d_idx, a_idx x3] of every pair: get_embedding_indices (transformer.py:303-332) in
    one launch, distances by direct differences (the diagonal is exactly 0), neighbour ties to the lower index."""
    _chk(points, torch.float32, "points", 3)
    if points.shape[-1] != 3:
        raise RuntimeError("points must be (B,N,3)")
    B, N, _ = points.shape
    idx4 = torch.empty(B, N, N, 4, dtype=torch.float32, device=points.device)
    _call("s6d_geo_indices_f32", _ptr(points), B, N, float(sigma_d), float(factor_a), _ptr(idx4), _stream())
    return idx4


def geo_embedding_points(points, sigma_d, factor_a, Wd, bd, Wa, ba, div_term, out_dtype=torch.float32, split=None):
    """points (B,N,3) f32 -> (B,N,N,256): geo_embedding(geo_indices(points, ...), ...) bit for bit without the idx4 tensor -- the
    embedding kernels compute the four indices of a pair in their prologue; the only temporary is the (B,N,3) neighbour table."""
    for a, nm in ((points, "points"), (Wd, "Wd"), (bd, "bd"), (Wa, "Wa"), (ba, "ba"), (div_term, "div_term")):
        _chk(a, torch.float32, nm)
    if points.dim() != 3 or points.shape[-1] != 3:
        raise RuntimeError("points must be (B,N,3)")
    if out_dtype not in (torch.float32, torch.float16):
        raise RuntimeError("the embedding is stored in float32 or float16")
    B, N, _ = points.shape
    knn = torch.empty(B, N, 3, dtype=torch.int32, device=points.device)
    out = torch.empty(B, N, N, Wd.shape[0], dtype=out_dtype, device=points.device)
    head = (_ptr(points), B, N, float(sigma_d), float(factor_a), _ptr(knn))
    if split is not None and have("geo_embedding_points"):
        for a, nm in ((split[0], "Wd_hilo"), (split[1], "Wa_hilo")):
            _chk(a, torch.bfloat16, nm, 3)
        _call("s6d_geo_embedding_points_split", *head, _ptr(split[0]), _ptr(bd), _ptr(split[1]), _ptr(ba), _ptr(div_term), Wd.shape[0], 3,
              _ptr(out), 1 if out_dtype == torch.float16 else 0, _stream())
        return out
    _call("s6d_geo_embedding_points_f32" if out_dtype == torch.float32 else "s6d_geo_embedding_points_f16", *head, _ptr(Wd), _ptr(bd),
          _ptr(Wa), _ptr(ba), _ptr(div_term), Wd.shape[0], 3, _ptr(out), _stream())
    return out


# limits of the accepted domain, from the header: 1 / temp of fine_match (checked by the library: S6D_EUNSUPPORTED beyond), and the
# largest |score| coarse_sample and fine_assign take (NOT checked by them: the caller knows it as 1 / temp)
FINE_MATCH_MAX_INV_TEMP = _lib.header_constant("S6D_FINE_MATCH_MAX_INV_TEMP")
ASSIGN_MAX_ABS_SCORE = _lib.header_constant("S6D_ASSIGN_MAX_ABS_SCORE")


def fine_assign(atten, pts2):
    """atten (B,M1,M2) f32, |atten| <= ASSIGN_MAX_ABS_SCORE, pts2 (B,M2-1,3) f32 -> pred (B,M1-1,3), wsum (B,M1-1), w1 (B,M1-1)."""
    _chk(atten, torch.float32, "atten", 3)
    _chk(pts2, torch.float32, "pts2", 3)
    B, M1, M2 = atten.shape
    dev = atten.device
    ws = torch.empty(_size("s6d_fine_assign_workspace_bytes", B, M1, M2), dtype=torch.uint8, device=dev)
    pred = torch.empty(B, M1 - 1, 3, dtype=torch.float32, device=dev)
    wsum = torch.empty(B, M1 - 1, dtype=torch.float32, device=dev)
    w1 = torch.empty(B, M1 - 1, dtype=torch.float32, device=dev)
    _call("s6d_fine_assign_f32", _ptr(atten), _ptr(pts2), B, M1, M2, _ptr(ws), _ptr(pred), _ptr(wsum), _ptr(w1), _stream())
    return pred, wsum, w1


def fine_match(f1, f2, pts2, temp):
    """f1 (B,M1,256), f2 (B,M2,256) f32 (background token at row 0), pts2 (B,M2-1,3) -> pred (B,M1-1,3), wsum, w1 (B,M1-1):
    feature similarity + dual softmax + labels + normalised assignment without the (B,M1,M2) matrix.  1 / temp above
    FINE_MATCH_MAX_INV_TEMP is refused by the library (S6D_EUNSUPPORTED -> RuntimeError)."""
    for t, nm in ((f1, "f1"), (f2, "f2"), (pts2, "pts2")):
        _chk(t, torch.float32, nm, 3)
    B, M1, C = f1.shape
    M2 = f2.shape[1]
    if f2.shape[0] != B or f2.shape[2] != C or tuple(pts2.shape) != (B, M2 - 1, 3):
        raise ValueError(f"fine_match: shapes {tuple(f1.shape)}, {tuple(f2.shape)}, {tuple(pts2.shape)}")
    dev = f1.device
    ws = torch.empty(_size("s6d_fine_match_workspace_bytes", B, M1, M2), dtype=torch.uint8, device=dev)
    pred = torch.empty(B, M1 - 1, 3, dtype=torch.float32, device=dev)
    wsum = torch.empty(B, M1 - 1, dtype=torch.float32, device=dev)
    w1 = torch.empty(B, M1 - 1, dtype=torch.float32, device=dev)
    _call("s6d_fine_match_f32", _ptr(f1), _ptr(f2), _ptr(pts2), B, M1, M2, C, 1.0 / temp, _ptr(ws), _ptr(pred), _ptr(wsum), _ptr(w1),
          _stream())
    return pred, wsum, w1


def pe_group_mlp(pts, idx, W0, b0, W1, b1, W2, b2):
    """pts (B,N,3) f32, idx (B,N,ns) i32, folded MLP weights -> (B,N,128) f32 (max over neighbours)."""
    _chk(pts, torch.float32, "pts", 3)
    _chk(idx, torch.int32, "idx", 3)
    ws = [w.contiguous() for w in (W0, b0, W1, b1, W2, b2)]
    for w, shp in zip(ws, ((32, 6), (32,), (64, 32), (64,), (128, 64), (128,))):
        _chk(w, torch.float32, "mlp weight")
        if tuple(w.shape) != shp:
            raise RuntimeError(f"SharedMLP [6,32,64,128] expected, got weight of shape {tuple(w.shape)}")
    B, N, _ = pts.shape
    out = torch.empty(B, N, 128, dtype=torch.float32, device=pts.device)
    _call("s6d_pe_group_mlp_f32", _ptr(pts), _ptr(idx), B, N, idx.shape[2], *[_ptr(w) for w in ws], _ptr(out), _stream())
    return out


def mha(q, k, v, scale):
    """q (B,N,256), k/v (B,M,256) f32 (column blocks of one projection output are taken as they are) -> (B,N,256): 4-head softmax
    attention, one wavefront per query row."""
    (q, ldq), (k, ldk), (v, ldv) = _rows3(q, "q"), _rows3(k, "k"), _rows3(v, "v")
    B, N, C = q.shape
    out = torch.empty(B, N, C, dtype=torch.float32, device=q.device)
    _call("s6d_mha_strided_f32", _ptr(q), ldq, _ptr(k), ldk, _ptr(v), ldv, B, N, k.shape[1], C, 4, scale, _ptr(out), _stream())
    return out


def linear_attn_focus(x, inv_scale, power):
    """x (...,256) f32, inv_scale (256) -> focused feature map, same shape."""
    x = x.contiguous()
    _chk(x, torch.float32, "x")
    inv_scale = inv_scale.reshape(-1).contiguous()
    _chk(inv_scale, torch.float32, "inv_scale", 1)
    y = torch.empty_like(x)
    _call("s6d_linear_attn_focus_f32", _ptr(x), _ptr(inv_scale), x.numel() // x.shape[-1], x.shape[-1], int(power), _ptr(y), _stream())
    return y


def linear_attention(q_proj, inv_scale, power, k_focused, v):
    """Focused linear attention behind the projections: q_proj (B,I,256) f32 raw proj_q output, k_focused (B,J,256) f32 (rows may be
    strided), v (B,J,256) f32 (rows may be strided), inv_scale (256) -> (B,I,256) f32."""
    for t, nm in ((q_proj, "q_proj"), (k_focused, "k_focused"), (v, "v")):
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 3:
            raise RuntimeError(f"{nm} must be a 3-d float32 CUDA tensor")
    q_proj = q_proj.contiguous()
    B, I, C = q_proj.shape
    J = k_focused.shape[1]
    for t, nm in ((k_focused, "k_focused"), (v, "v")):
        if t.shape != (B, J, C) or t.stride(2) != 1 or (B > 1 and t.stride(0) != J * t.stride(1)):     # (B == 1: stride(0) is free)
            raise ValueError(f"{nm} must be (B, J, C) with unit channel stride and batch stride J * row stride; got {tuple(t.shape)} "
                             f"strides {tuple(t.stride())}")
    inv_scale = inv_scale.reshape(-1).contiguous()
    _chk(inv_scale, torch.float32, "inv_scale", 1)
    ws = torch.empty(_size("s6d_linear_attention_workspace_floats", B), dtype=torch.float32, device=q_proj.device)
    out = torch.empty_like(q_proj)
    _call("s6d_linear_attention_f32", _ptr(q_proj), _ptr(inv_scale), int(power), _ptr(k_focused), k_focused.stride(1), _ptr(v), v.stride(1),
          B, I, J, C, _ptr(ws), _ptr(out), _stream())
    return out


# ------------------------------------------------------------------ ISM scoring
def pairwise_cosine(query, ref):
    """(P,C), (R,C) f32 -> (P,R) clamp(cos,0,1)."""
    _chk(query, torch.float32, "query", 2)
    _chk(ref, torch.float32, "ref", 2)
    P, C = query.shape
    R = ref.shape[0]
    out = torch.empty(P, R, dtype=torch.float32, device=query.device)
    _call("s6d_pairwise_cosine_f32", _ptr(query), _ptr(ref), P, R, C, _ptr(out), _stream())
    return out


def semantic_select(scores, topk):
    """(P,O,T) f32 -> best_score (P) f32, best_obj (P) i32, best_tmpl (P) i32."""
    _chk(scores, torch.float32, "scores", 3)
    P, O, T = scores.shape
    dev = scores.device
    bs = torch.empty(P, dtype=torch.float32, device=dev)
    bo = torch.empty(P, dtype=torch.int32, device=dev)
    bt = torch.empty(P, dtype=torch.int32, device=dev)
    _call("s6d_semantic_select_f32", _ptr(scores), P, O, T, int(topk), _ptr(bs), _ptr(bo), _ptr(bt), _stream())
    return bs, bo, bt


def patch_scores(query, refstore, obj, tmpl, thred, sel=None):
    """query (S,N1,C), refstore (O,T,N2,C) f32, obj/tmpl (S) i32 -> appe (S), ratio (S).
    sel (S) i32: query is the UN-gathered (P,N1,C) tensor of every proposal and row s reads query[sel[s]] (no gathered copy)."""
    _chk(query, torch.float32, "query", 3)
    _chk(refstore, torch.float32, "refstore", 4)
    _chk(obj, torch.int32, "obj", 1)
    _chk(tmpl, torch.int32, "tmpl", 1)
    S, N1, C = query.shape
    if sel is not None:
        _chk(sel, torch.int32, "sel", 1)
        S = sel.shape[0]
        if obj.shape[0] != S or tmpl.shape[0] != S:
            raise ValueError("patch_scores: obj / tmpl / sel must have one entry per selected proposal")
    _, T, N2, _ = refstore.shape
    ws = torch.empty(max(_size("s6d_patch_scores_workspace_floats", S, N1, N2), 1), dtype=torch.float32, device=query.device)
    appe = torch.empty(S, dtype=torch.float32, device=query.device)
    ratio = torch.empty(S, dtype=torch.float32, device=query.device)
    _call("s6d_patch_scores_sel_f32", _ptr(query), _ptr(sel), _ptr(refstore), _ptr(obj), _ptr(tmpl), S, N1, N2, C, T, thred, _ptr(ws),
          _ptr(appe), _ptr(ratio), _stream())
    return appe, ratio


def masked_depth_mean(masks, depth, K, depth_scale, frame=None, sel=None):
    """sel (S) i32: masks is the UN-gathered (P,H,W) tensor of every proposal and mask s of the call is masks[sel[s]].
    masks (S,H,W) f32, depth (H,W) f32, K 3x3 (any float dtype, host or device) -> (S,3) f32.  The camera matrix goes to
    the device as float64 (the reference's dtype) and is read there: no host copy of a device K and no cache keyed by
    an address (a new frame's K may land on the old one's).  Several frames in one launch: depth (F,H,W), K (F,3,3),
    frame (S) i32 = the frame of every mask."""
    _chk(masks, torch.float32, "masks", 3)
    S, H, W = masks.shape
    if sel is not None:
        _chk(sel, torch.int32, "sel", 1)
        S = sel.shape[0]
    if frame is None:
        _chk(depth, torch.float32, "depth", 2)
        if tuple(K.shape) != (3, 3):
            raise ValueError(f"K must be 3x3, got {tuple(K.shape)}")
    else:
        _chk(depth, torch.float32, "depth", 3)
        _chk(frame, torch.int32, "frame", 1)
        if K.dim() != 3 or tuple(K.shape[1:]) != (3, 3) or K.shape[0] != depth.shape[0] or frame.shape[0] != S:
            raise ValueError(f"batched call: depth (F,H,W), K (F,3,3), frame (S); got {tuple(depth.shape)}, {tuple(K.shape)}, {tuple(frame.shape)}")
    if frame is not None and policy.current().debug and S:          # costs a host round trip: debug runs only
        lo, hi = int(frame.min()), int(frame.max())
        if lo < 0 or hi >= depth.shape[0]:
            raise ValueError(f"frame indices span [{lo}, {hi}] but there are {depth.shape[0]} frames")
    Kd = K.detach().to(device=masks.device, dtype=torch.float64).contiguous()
    out = torch.empty(S, 3, dtype=torch.float32, device=masks.device)
    ws = torch.empty(max(_size("s6d_masked_depth_mean_workspace_bytes", S, H, W), 8), dtype=torch.uint8, device=masks.device)
    _call("s6d_masked_depth_mean_sel_f32", _ptr(masks), _ptr(sel), _ptr(depth), _ptr(frame), S, H, W, depth_scale, _ptr(Kd), _ptr(ws),
          _ptr(out), _stream())
    return out


def project_bbox(pointcloud, poses, obj, tmpl, trans, K, H, W, frame=None):
    """-> uv (S,N,2) i32, bbox (S,4) i32 = (min u, min v, max u, max v).  K (3,3) f32, or (F,3,3) with frame (S) i32."""
    for a, nm, nd in ((pointcloud, "pointcloud", 3), (poses, "poses", 3), (trans, "trans", 2), (K, "K", 2 if frame is None else 3)):
        _chk(a, torch.float32, nm, nd)
    _chk(obj, torch.int32, "obj", 1)
    _chk(tmpl, torch.int32, "tmpl", 1)
    if frame is not None:
        _chk(frame, torch.int32, "frame", 1)
    S, N = obj.shape[0], pointcloud.shape[1]
    uv = torch.empty(S, N, 2, dtype=torch.int32, device=trans.device)
    bbox = torch.empty(S, 4, dtype=torch.int32, device=trans.device)
    _call("s6d_project_bbox_frames_f32", _ptr(pointcloud), _ptr(poses), _ptr(obj), _ptr(tmpl), _ptr(trans), _ptr(K), _ptr(frame), S, N,
          int(H), int(W), _ptr(uv), _ptr(bbox), _stream())
    return uv, bbox


# ------------------------------------------------------------------ fused-op registry
# ------------------------------------------------------------------ overlay pictures (csrc/s6d_vis.hip)
VIS_MAX_HW = 8192
VIS_CLAMP = (-8192, 8191)


def _vis_size(what, H, W):
    if not (1 <= H <= VIS_MAX_HW and 1 <= W <= VIS_MAX_HW):
        raise ValueError(f"{what}: H and W must lie in [1, {VIS_MAX_HW}], got H = {H}, W = {W}")


def _vis_frame_start(what, frame_start, B, total):
    _chk(frame_start, torch.int64, "frame_start", 1)
    if frame_start.shape[0] != B + 1:
        raise ValueError(f"{what}: frame_start must have B + 1 = {B + 1} entries, got {frame_start.shape[0]}")
    fs = frame_start.cpu()
    if int(fs[0]) != 0 or int(fs[-1]) != total or bool((fs[1:] < fs[:-1]).any()):
        raise ValueError(f"{what}: frame_start must rise from 0 to {total}, got {fs.tolist()}")


def vis_owner_from_masks(packed, order, frame_start, H, W):
    """packed (N, ceil(H W / 64)) int64 (``mask_pack`` / ``rle_to_packed``) of the detections of all frames, order (K,) int32 the
    detection indices frame by frame in rank order, frame_start (B+1,) int64 -> owner (B,H,W) int32: the first detection of the
    pixel's frame that covers it, -1 for none (include/sam6d_hip.h: s6d_vis_owner_from_masks)."""
    H, W = int(H), int(W)
    _vis_size("vis_owner_from_masks", H, W)
    _chk(packed, torch.int64, "packed", 2)
    _chk(order, torch.int32, "order", 1)
    N, K, B = packed.shape[0], order.shape[0], frame_start.shape[0] - 1
    if packed.shape[1] != (H * W + 63) // 64:
        raise ValueError(f"vis_owner_from_masks: packed must have ceil(H W / 64) = {(H * W + 63) // 64} words per mask, got {packed.shape[1]}")
    if K > N:
        raise ValueError(f"vis_owner_from_masks: order names {K} detections, packed has {N}")
    _vis_frame_start("vis_owner_from_masks", frame_start, B, K)
    owner = torch.empty(B, H, W, dtype=torch.int32, device=packed.device)
    _call("s6d_vis_owner_from_masks", _ptr(packed), _ptr(order), _ptr(frame_start), B, N, K, H, W, _ptr(owner), _stream())
    return owner


def vis_canvas(B, H, W, device):
    """The empty canvas of ``vis_merge_layers``: dict(zbuf (B,H,W) f32 = 0, owner (B,H,W) int32 = -1, shade (B,H,W,3) uint8 = 0)."""
    return dict(zbuf=torch.zeros(B, H, W, dtype=torch.float32, device=device), owner=torch.full((B, H, W), -1, dtype=torch.int32, device=device),
                shade=torch.zeros(B, H, W, 3, dtype=torch.uint8, device=device))


def vis_merge_layers(canvas, depth, rgb, frame, first):
    """Folds the layers depth (T,H,W) f32, rgb (T,H,W,3) uint8 (``render_views``) of the instances first .. first + T - 1, layer t
    belonging to frame[t] ((T,) int32), into ``canvas`` (``vis_canvas``) IN PLACE: the nearest z > 0 wins, at equal z the lower
    instance index (include/sam6d_hip.h: s6d_vis_merge_layers).  A frame outside [0, B) is refused here, on the host."""
    _chk(depth, torch.float32, "depth", 3)
    _chk(rgb, torch.uint8, "rgb", 4)
    _chk(frame, torch.int32, "frame", 1)
    _chk(canvas["zbuf"], torch.float32, "zbuf", 3)
    _chk(canvas["owner"], torch.int32, "owner", 3)
    _chk(canvas["shade"], torch.uint8, "shade", 4)
    T, H, W = depth.shape
    B = canvas["zbuf"].shape[0]
    _vis_size("vis_merge_layers", H, W)
    if (tuple(rgb.shape) != (T, H, W, 3) or frame.shape[0] != T or tuple(canvas["zbuf"].shape) != (B, H, W)
            or tuple(canvas["owner"].shape) != (B, H, W) or tuple(canvas["shade"].shape) != (B, H, W, 3)):
        raise ValueError(f"vis_merge_layers: depth (T,H,W), rgb (T,H,W,3), frame (T,) and a canvas of (B,H,W) expected, got "
                         f"{tuple(depth.shape)}, {tuple(rgb.shape)}, {tuple(frame.shape)}, {tuple(canvas['zbuf'].shape)}")
    if T and (int(frame.min()) < 0 or int(frame.max()) >= B):
        raise ValueError(f"vis_merge_layers: frame must lie in [0, {B}), got [{int(frame.min())}, {int(frame.max())}]")
    if int(first) < 0:
        raise ValueError(f"vis_merge_layers: first must be >= 0, got {first}")
    _call("s6d_vis_merge_layers", _ptr(depth), _ptr(rgb), _ptr(frame), T, int(first), B, H, W, _ptr(canvas["zbuf"]), _ptr(canvas["owner"]),
          _ptr(canvas["shade"]), _stream())
    return canvas


def vis_paint(image, owner, colors=None, shade=None, alpha=84, gray=True, edge_width=2, edge_color=(255, 255, 255)):
    """image (B,H,W,3) uint8, owner (B,H,W) int32 and either colors (n_ids,3) uint8 or shade (B,H,W,3) uint8 -> the painted picture
    (B,H,W,3) uint8: base (grey or as it is), alpha / 256 of the owner's colour, contours of the owner map in edge_color dilated to
    edge_width (include/sam6d_hip.h: s6d_vis_paint_u8)."""
    _chk(image, torch.uint8, "image", 4)
    _chk(owner, torch.int32, "owner", 3)
    B, H, W, _ = image.shape
    _vis_size("vis_paint", H, W)
    if image.shape[3] != 3 or tuple(owner.shape) != (B, H, W):
        raise ValueError(f"vis_paint: image (B,H,W,3) and owner (B,H,W) expected, got {tuple(image.shape)}, {tuple(owner.shape)}")
    if (colors is None) == (shade is None):
        raise ValueError("vis_paint: exactly one of colors and shade is needed")
    if not 0 <= int(alpha) <= 256:
        raise ValueError(f"vis_paint: alpha must lie in [0, 256] (units of 1/256), got {alpha}")
    if not 0 <= int(edge_width) <= 4:
        raise ValueError(f"vis_paint: edge_width must lie in [0, 4], got {edge_width}")
    edge = [int(c) for c in edge_color]
    if len(edge) != 3 or min(edge) < 0 or max(edge) > 255:
        raise ValueError(f"vis_paint: edge_color must be three values in [0, 255], got {edge_color}")
    n_ids = 0
    if colors is not None:
        _chk(colors, torch.uint8, "colors", 2)
        n_ids = colors.shape[0]
        if n_ids < 1 or colors.shape[1] != 3:
            raise ValueError(f"vis_paint: colors (n_ids,3) with n_ids >= 1 expected, got {tuple(colors.shape)}")
    else:
        _chk(shade, torch.uint8, "shade", 4)
        if tuple(shade.shape) != (B, H, W, 3):
            raise ValueError(f"vis_paint: shade {(B, H, W, 3)} expected, got {tuple(shade.shape)}")
    out = torch.empty_like(image)
    _call("s6d_vis_paint_u8", _ptr(image), _ptr(owner), _ptr(colors), _ptr(shade), n_ids, B, H, W, 1 if gray else 0, int(alpha),
          int(edge_width), edge[0], edge[1], edge[2], _ptr(out), _stream())
    return out


def vis_project(points, inst, R, t, cams, znear):
    """points (M,3) f32, inst (M,) int32 into R (N,3,3) f32, t (N,3) f32, cams (N,4) f32 = fx fy cx cy -> (xy (M,2) int32 pixels
    clamped to [-8192, 8191], valid (M,) uint8) (include/sam6d_hip.h: s6d_vis_project_f32)."""
    _chk(points, torch.float32, "points", 2)
    _chk(inst, torch.int32, "inst", 1)
    _chk(R, torch.float32, "R", 3)
    _chk(t, torch.float32, "t", 2)
    _chk(cams, torch.float32, "cams", 2)
    M, N = points.shape[0], R.shape[0]
    if points.shape[1] != 3 or inst.shape[0] != M or tuple(R.shape[1:]) != (3, 3) or tuple(t.shape) != (N, 3) or tuple(cams.shape) != (N, 4):
        raise ValueError(f"vis_project: points (M,3), inst (M,), R (N,3,3), t (N,3), cams (N,4) expected, got {tuple(points.shape)}, "
                         f"{tuple(inst.shape)}, {tuple(R.shape)}, {tuple(t.shape)}, {tuple(cams.shape)}")
    xy = torch.empty(M, 2, dtype=torch.int32, device=points.device)
    valid = torch.empty(M, dtype=torch.uint8, device=points.device)
    _call("s6d_vis_project_f32", _ptr(points), _ptr(inst), _ptr(R), _ptr(t), _ptr(cams), M, N, float(znear), _ptr(xy), _ptr(valid), _stream())
    return xy, valid


def vis_draw_chunk():
    """How many primitives a workgroup of the draw kernel takes at a time (S6D_VIS_DRAW_CHUNK of include/sam6d_hip.h)."""
    return _lib.header_constant("S6D_VIS_DRAW_CHUNK")


def vis_draw(image, prims, frame_start, check=True):
    """Draws prims (P,8) int32 = frame, x0, y0, x1, y1, size, r | g << 8 | b << 16, valid -- sorted by frame, frame_start (B+1,)
    int64 -- opaque into image (B,H,W,3) uint8 IN PLACE; the covering primitive of highest index wins (include/sam6d_hip.h:
    s6d_vis_draw_u8).  check (it reads the device: a synchronisation) refuses a size outside [0, 64], a frame that is not the one
    frame_start files the entry under, and a coordinate of a valid entry outside [-8192, 8191]."""
    _chk(image, torch.uint8, "image", 4)
    _chk(prims, torch.int32, "prims", 2)
    B, H, W, _ = image.shape
    _vis_size("vis_draw", H, W)
    P = prims.shape[0]
    if image.shape[3] != 3 or prims.shape[1] != 8:
        raise ValueError(f"vis_draw: image (B,H,W,3) and prims (P,8) expected, got {tuple(image.shape)}, {tuple(prims.shape)}")
    _vis_frame_start("vis_draw", frame_start, B, P)
    if check and P:
        if int(prims[:, 5].min()) < 0 or int(prims[:, 5].max()) > 64:
            raise ValueError(f"vis_draw: size must lie in [0, 64], got [{int(prims[:, 5].min())}, {int(prims[:, 5].max())}]")
        want = torch.repeat_interleave(torch.arange(B, device=prims.device), (frame_start[1:] - frame_start[:-1]))
        if bool((prims[:, 0] != want).any()):
            raise ValueError(f"vis_draw: frame must lie in [0, {B}) and the list be sorted by it as frame_start says")
        xy = prims[:, 1:5][prims[:, 7] != 0]
        if xy.numel() and (int(xy.min()) < VIS_CLAMP[0] or int(xy.max()) > VIS_CLAMP[1]):
            raise ValueError(f"vis_draw: coordinates must lie in [{VIS_CLAMP[0]}, {VIS_CLAMP[1]}], got [{int(xy.min())}, {int(xy.max())}]")
    _call("s6d_vis_draw_u8", _ptr(prims), _ptr(frame_start), B, P, H, W, _ptr(image), _stream())
    return image


# ------------------------------------------------------------------ pose verification (csrc/s6d_verify.hip)
def _verify_size(what, H, W):
    if H < 1 or W < 1 or H * W >= 2 ** 29:
        raise ValueError(f"{what}: H, W >= 1 and H W < 2^29 expected, got H = {H}, W = {W}")


def set_verify_lds_words(words):
    """The largest claimed bitmap (words of 64 pixels per frame) ``verify_select`` keeps in LDS; 0 = the default, 4800
    (include/sam6d_hip.h: s6d_set_verify_lds_words): lets tests reach the workspace path at small shapes; same results for every
    setting."""
    _call("s6d_set_verify_lds_words", int(words))


def verify_evidence(render, depth_obs, obs_index, depth_unit, tau, masks=None, check=True):
    """render (N,H,W) f32 = ``render_depth`` of every instance (camera Z in model units, 0 on background), depth_obs (M,H,W) f32
    measured depth, obs_index (N,) int32 into M, depth_unit model units per unit of depth_obs, tau model units, masks (N,H,W) uint8
    or None -> dict(counts (N,8) int32 = rendered, missing, inlier, occluded, behind, det, det and rendered, det and inlier;
    inlier (N, ceil(H W / 64)) int64 in the word layout of ``mask_pack``; span (N,2) int32 = first and last non-zero word,
    (words, -1) for none) (include/sam6d_hip.h: s6d_verify_evidence_f32).  An obs_index outside [0, M) is refused here, on the host
    (check=False skips that read of the device; such an instance then counts every rendered pixel as missing)."""
    _chk(render, torch.float32, "render", 3)
    _chk(depth_obs, torch.float32, "depth_obs", 3)
    _chk(obs_index, torch.int32, "obs_index", 1)
    N, H, W = render.shape
    M = depth_obs.shape[0]
    if M < 1 or tuple(depth_obs.shape[1:]) != (H, W) or tuple(obs_index.shape) != (N,):
        raise ValueError(f"verify_evidence: render (N,H,W), depth_obs (M,H,W), obs_index (N,) expected, got {tuple(render.shape)}, "
                         f"{tuple(depth_obs.shape)}, {tuple(obs_index.shape)}")
    _verify_size("verify_evidence", H, W)
    if masks is not None:
        _chk(masks, torch.uint8, "masks", 3)
        if tuple(masks.shape) != (N, H, W):
            raise ValueError(f"verify_evidence: masks {(N, H, W)} expected, got {tuple(masks.shape)}")
    unit, tau = float(torch.tensor(float(depth_unit), dtype=torch.float32)), float(torch.tensor(float(tau), dtype=torch.float32))
    if not (0 < unit < float("inf")) or not tau >= 0:
        raise ValueError(f"verify_evidence: depth_unit must be positive and finite and tau >= 0, got {depth_unit}, {tau}")
    if check and N and (int(obs_index.min()) < 0 or int(obs_index.max()) >= M):
        raise ValueError(f"verify_evidence: obs_index must lie in [0, {M}), got [{int(obs_index.min())}, {int(obs_index.max())}]")
    dev, words = render.device, (H * W + 63) // 64
    out = dict(counts=torch.empty(N, 8, dtype=torch.int32, device=dev), inlier=torch.empty(N, words, dtype=torch.int64, device=dev),
               span=torch.empty(N, 2, dtype=torch.int32, device=dev))
    _call("s6d_verify_evidence_f32", _ptr(render), _ptr(depth_obs), _ptr(obs_index), _ptr(masks), N, M, H, W, unit, tau,
          _ptr(out["counts"]), _ptr(out["inlier"]), _ptr(out["span"]), _stream())
    return out


def verify_select(inlier, counts, span, order, frame_start, flagged, min_inliers, min_fit, min_fresh, H=None, W=None, check=True):
    """inlier, counts, span of ``verify_evidence``; order (K,) int32 the instance indices frame by frame in visiting order,
    frame_start (B+1,) int64; flagged (N,) uint8 / bool or None -> (status (N,) int32, fresh (N,) int32): per frame a pixel supports at
    most one kept instance (include/sam6d_hip.h: s6d_verify_select; 0 kept, 1 too few inliers, 2 fit below min_fit, 3 explained
    already, 4 not verifiable or not named in order).  H, W: the image size, checked against the word count when given; the kernel
    needs the word count only, so the default is any image of that many words.  An order outside [0, N) or naming an instance twice and
    a frame_start that does not rise from 0 to K are refused here, on the host (check=False skips those reads of the device)."""
    _chk(inlier, torch.int64, "inlier", 2)
    _chk(counts, torch.int32, "counts", 2)
    _chk(span, torch.int32, "span", 2)
    _chk(order, torch.int32, "order", 1)
    N, words = inlier.shape
    K, B = order.shape[0], frame_start.shape[0] - 1
    if tuple(counts.shape) != (N, 8) or tuple(span.shape) != (N, 2) or words < 1:
        raise ValueError(f"verify_select: inlier (N,words), counts (N,8), span (N,2) expected, got {tuple(inlier.shape)}, "
                         f"{tuple(counts.shape)}, {tuple(span.shape)}")
    if H is None or W is None:
        H, W = 1, 64 * words - 63
    H, W = int(H), int(W)
    _verify_size("verify_select", H, W)
    if (H * W + 63) // 64 != words:
        raise ValueError(f"verify_select: inlier must have ceil(H W / 64) = {(H * W + 63) // 64} words per instance, got {words}")
    if K > N:
        raise ValueError(f"verify_select: order names {K} instances, inlier has {N}")
    if flagged is not None:
        flagged = flagged.to(torch.uint8) if flagged.dtype == torch.bool else flagged
        _chk(flagged, torch.uint8, "flagged", 1)
        if flagged.shape[0] != N:
            raise ValueError(f"verify_select: flagged ({N},) expected, got {tuple(flagged.shape)}")
    mi, mf, mr = int(min_inliers), float(min_fit), float(min_fresh)
    if mi < 0 or not mf >= 0 or not mr >= 0:
        raise ValueError(f"verify_select: min_inliers, min_fit and min_fresh must be >= 0, got {min_inliers}, {min_fit}, {min_fresh}")
    if check:
        _vis_frame_start("verify_select", frame_start, B, K)
        if K and (int(order.min()) < 0 or int(order.max()) >= N):
            raise ValueError(f"verify_select: order must lie in [0, {N}), got [{int(order.min())}, {int(order.max())}]")
        if K and int(torch.unique(order).numel()) != K:
            raise ValueError("verify_select: order names an instance more than once")
    else:
        _chk(frame_start, torch.int64, "frame_start", 1)
        if B < 0:
            raise ValueError("verify_select: frame_start must have B + 1 entries")
    dev = inlier.device
    nbytes = _size("s6d_verify_select_workspace_bytes", B, H, W)
    if nbytes < 0:
        raise RuntimeError(f"verify_select: unsupported sizes (B {B}, H {H}, W {W})")
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev) if nbytes else None
    status = torch.empty(N, dtype=torch.int32, device=dev)
    fresh = torch.empty(N, dtype=torch.int32, device=dev)
    _call("s6d_verify_select", _ptr(inlier), _ptr(counts), _ptr(span), _ptr(order), _ptr(frame_start), _ptr(flagged), B, N, K, H, W, mi,
          mf, mr, _ptr(ws), _ptr(status), _ptr(fresh), _stream())
    return status, fresh


# Names of fused gfx950 ops the loaded library exports.  Product modules ask ``have(name)``
# and otherwise express the same math with library GEMMs on the device (never on the CPU).
_FUSED = {}


def have(name):
    if name not in _FUSED:
        sym = {"rpe_attention": "s6d_rpe_attention_f32", "rpe_attention_packed": "s6d_rpe_attention_packed_f32", "geo_embedding": "s6d_geo_embedding_f32", "geo_embedding_f16": "s6d_geo_embedding_f16", "geo_embedding_split": "s6d_geo_embedding_split", "geo_indices": "s6d_geo_indices_f32", "geo_embedding_points": "s6d_geo_embedding_points_split",
               "fine_assign": "s6d_fine_assign_f32", "fine_match": "s6d_fine_match_f32", "pem_pre": "s6d_pem_compact_cloud_f32", "coarse_sample": "s6d_coarse_sample_f32", "cosine_similarity": "s6d_cosine_similarity_f32", "upsample_gather": "s6d_upsample_gather_f32",
               "min_dist": "s6d_min_dist_f32", "rot_from_h": "s6d_rot_from_h_f32", "weighted_procrustes": "s6d_weighted_procrustes_f32", "add_layernorm": "s6d_add_layernorm_bf16", "gemm_bf16": "s6d_gemm_bf16", "gemm_bf16_res": "s6d_gemm_bf16_res", "gemm_bf16_lnfold": "s6d_gemm_bf16_lnfold", "gemm_f16": "s6d_gemm_f16", "gemm_fp8": "s6d_gemm_fp8", "layernorm_fp8": "s6d_layernorm_fp8", "layernorm_f32out": "s6d_layernorm_bf16_f32", "linear_f32": "s6d_linear_f32", "attn_output_chain": "s6d_attn_output_chain_f32", "win_attention": "s6d_win_attention_layout_bf16",
               "pairwise_cosine": "s6d_pairwise_cosine_f32",
               "patch_scores": "s6d_patch_scores_sel_f32", "pose_hypotheses": "s6d_pose_hypotheses_f32",
               "pe_group": "s6d_pe_group_mlp_f32", "masked_depth_mean": "s6d_masked_depth_mean_sel_f32",
               "semantic_select": "s6d_semantic_select_f32", "seq_attention": "s6d_seq_attention_bf16", "sam_preprocess": "s6d_sam_preprocess_f32", "im2col3x3": "s6d_im2col3x3_b16", "nonfinite_rows": "s6d_nonfinite_rows_f32", "patchify": "s6d_patchify_b16", "crop_resize_pad": "s6d_crop_resize_pad_f32", "samdec_img2tok": "s6d_samdec_img2tok_bf16", "samdec_img2tok_raw": "s6d_samdec_img2tok_raw_bf16", "samdec_tok2img": "s6d_samdec_tok2img_f32", "samdec_tok2img_raw": "s6d_samdec_tok2img_raw_bf16", "sam_mask_post": "s6d_sam_mask_post_sel_f32", "gemm_fp8_mx": "s6d_gemm_fp8_mxa", "nms": "s6d_nms_f32", "samdec_upscale_heads": "s6d_samdec_upscale_heads_bf16", "samdec_tokens": "s6d_samdec_tokens_post_bf16", "samdec_token_folds": "s6d_samdec_tokens_post_bf16", "mha": "s6d_mha_f32",
               "linear_attn_focus": "s6d_linear_attn_focus_f32", "linear_attention": "s6d_linear_attention_f32", "project_bbox": "s6d_project_bbox_frames_f32",
               "template_boxes": "s6d_template_boxes_u8", "template_points": "s6d_template_points_f32", "template_pem_crops": "s6d_template_pem_crops_f32",
               "template_ism_crops": "s6d_template_ism_crops_f32", "render_views": "s6d_raster_views_f32", "render_views_textured": "s6d_raster_views_tex_f32",
               "render_depth": "s6d_raster_depth_f32", "pose_errors": "s6d_pose_err_mssd_mspd_f32", "vsd_counts": "s6d_vsd_counts_f32",
               "gt_visibility": "s6d_gt_visibility_f32", "model_diameter": "s6d_model_diameter_f32",
               "add_errors": "s6d_pose_err_add_f32", "adds_errors": "s6d_pose_err_adds_f32",
               "mask_pack": "s6d_mask_pack_u8", "mask_pair_inter": "s6d_mask_pair_inter", "box_pair_iou": "s6d_box_pair_iou_f64", "coco_match": "s6d_coco_match",
               "small_regions": "s6d_remove_small_regions_u8",
               "rle_encode": "s6d_rle_write_u8", "rle_to_packed": "s6d_rle_to_packed", "rle_to_masks": "s6d_rle_to_masks_u8",
               "refine_normal_eq": "s6d_refine_normal_eq_f64", "refine_update": "s6d_refine_update_f64",
               "vis_owner_from_masks": "s6d_vis_owner_from_masks", "vis_merge_layers": "s6d_vis_merge_layers", "vis_paint": "s6d_vis_paint_u8",
               "vis_project": "s6d_vis_project_f32", "vis_draw": "s6d_vis_draw_u8",
               "verify_evidence": "s6d_verify_evidence_f32", "verify_select": "s6d_verify_select"}.get(name)
        _FUSED[name] = sym is not None and hasattr(_lib.lib(), sym)
    # (policy.disable_fused: kernel names the modules must not use -- the tests' way of forcing the library statement)
    if policy.current().disable_fused and name in policy.current().disable_fused.split(","):
        return False
    return _FUSED[name]
