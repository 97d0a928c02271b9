"""Plain numpy restatements of the ISM scoring kernels (csrc/s6d_ism.hip), one function per kernel -- TEST INFRASTRUCTURE ONLY.

Values that are compared within a tolerance are computed in float64 on the float32 operands; values that are compared bit for bit
(the visible ratio given its counts, the projected pixels) follow the float32 operation order the kernel documents.  Nothing here
imports the code under test.  The translation kernels keep oracle.ism.mean_translation_pinned as their comparand."""
import numpy as np

F32, F64 = np.float32, np.float64
INT_MIN = -2 ** 31


def cosine_ref(q, r):
    """PairwiseSimilarity (loss.py:27-44) on (P,C), (R,C): clamp(q.r / (max(|q|, 1e-12) max(|r|, 1e-12)), 0, 1) in float64."""
    q, r = np.asarray(q, F64), np.asarray(r, F64)
    nq = np.maximum(np.sqrt((q * q).sum(-1)), 1e-12)
    nr = np.maximum(np.sqrt((r * r).sum(-1)), 1e-12)
    return np.clip((q @ r.T) / (nq[:, None] * nr[None, :]), 0.0, 1.0)


def semantic_select_ref(scores, topk):
    """compute_semantic_score + best_template_pose (detector.py:260-296, :198-207) on (P,O,T): per object the mean of the
    min(topk, T) largest scores in float64; the best object is the FIRST maximum of those means, the best template the FIRST maximum
    of that object's row.  -> (best_score (P) f64, best_obj (P) i64, best_tmpl (P) i64)."""
    s = np.asarray(scores, F64)
    P, O, T = s.shape
    k = min(int(topk), T)
    per = np.sort(s, axis=-1)[:, :, T - k:].sum(-1) / k
    obj = np.argmax(per, axis=1)
    rows = s[np.arange(P), obj]
    return per[np.arange(P), obj], obj, np.argmax(rows, axis=1)


def patch_scores_ref(q, ref, thred):
    """MaskedPatch_MatrixSimilarity.compute_straight / compute_visible_ratio (loss.py:52-76) on q (S,N1,C) and the GATHERED reference
    (S,N2,C).  sim in float64.  -> dict of
      appe   (S) f64  clamp(sum(rowmax) / (nnz + 1e-6), 0, 1), nnz = query rows whose element sum is non-zero
      ratio  (S) f32  float32(vis) / (float32(valid) + float32(1e-6)): given the counts, the kernel's bits
      nnz, valid, vis (S) i64   valid = #(colmax != 0), vis = #(colmax > thred and colmax != 0)
      col_margin (S) f64   min over the non-zero column maxima of min(|colmax - thred|, |colmax|) (inf when there is none)
      rowsum (S,N1) f64, rowabs (S,N1) f64   element sum of every query row and the sum of its magnitudes (premise of nnz)."""
    q, ref = np.asarray(q, F64), np.asarray(ref, F64)
    sim = q @ ref.transpose(0, 2, 1)
    rowsum = q.sum(-1)
    nnz = np.count_nonzero(rowsum, axis=-1)
    appe = np.clip(sim.max(-1).sum(-1) / (nnz + 1e-6), 0.0, 1.0)
    col = sim.max(1)
    nz = col != 0
    valid = nz.sum(-1)
    vis = ((col > thred) & nz).sum(-1)
    ratio = valid.astype(F32)
    ratio = vis.astype(F32) / (ratio + F32(1e-6))
    dist = np.where(nz, np.minimum(np.abs(col - thred), np.abs(col)), np.inf)
    return dict(appe=appe, ratio=ratio.astype(F32), nnz=nnz, valid=valid, vis=vis, col_margin=dist.min(-1), rowsum=rowsum,
                rowabs=np.abs(q).sum(-1))


def fma32(a, b, c):
    """float32 fma(a, b, c) with ONE rounding.  The product of two float32 is exact in float64; the float64 sum is rounded to odd
    (truncate the exact sum, set the last bit when it was inexact), which with 53 >= 24 + 2 bits makes the final rounding to float32
    the rounding of the exact value -- the plain float64 emulation of tests/test_host_sam_decoder.py without its double rounding."""
    p = np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64)
    c = np.broadcast_to(np.asarray(c, F32).astype(F64), p.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)                       # TwoSum: p + c = s + e exactly
    inexact = np.isfinite(s) & (e != 0)
    bits = s.copy().view(np.uint64)
    down = inexact & ((e > 0) != (s > 0))                   # |s| lies above the exact sum: one step toward zero truncates it
    bits = np.where(down, bits - np.uint64(1), bits)
    bits = np.where(inexact, bits | np.uint64(1), bits)
    with np.errstate(over="ignore"):
        return bits.view(F64).astype(F32)


def to_int_pinned(x):
    """`.to(torch.int)` of the pinned (x86, CPU) reference run on float32: truncation toward zero inside the int range; NaN, +-inf and
    |x| >= 2^31 give -2^31."""
    x = np.asarray(x, F32).astype(F64)
    ok = np.isfinite(x) & (np.abs(x) < 2.0 ** 31)
    return np.where(ok, np.trunc(np.where(ok, x, 0.0)), float(INT_MIN)).astype(np.int64)


def project_ref(pointcloud, R, trans, K, H, W):
    """project_template_to_image (detector.py:209-232) in the operation order of its pinned run, float32 throughout: every 3-term
    product is a k-ascending fma chain (mul, fma, fma), the translation a separate rounded add, the perspective division IEEE, then
    to_int_pinned and the clamp.  pointcloud (S,N,3), R (S,3,3), trans (S,3), K (3,3) or (S,3,3) -> uv (S,N,2) i32, bbox (S,4) i32."""
    pc, R, t = np.asarray(pointcloud, F32), np.asarray(R, F32), np.asarray(trans, F32)
    K = np.asarray(K, F32)
    S = pc.shape[0]
    K = np.broadcast_to(K, (S, 3, 3))
    x, y, z = pc[..., 0], pc[..., 1], pc[..., 2]

    def chain(M, row, a, b, c):
        m = M[:, row, :, None]                              # (S,3,1) against (S,N)
        return fma32(m[:, 2], c, fma32(m[:, 1], b, m[:, 0] * a))
    with np.errstate(all="ignore"):
        px = chain(R, 0, x, y, z) + t[:, 0:1]
        py = chain(R, 1, x, y, z) + t[:, 1:2]
        pz = chain(R, 2, x, y, z) + t[:, 2:3]
        hx, hy, hz = chain(K, 0, px, py, pz), chain(K, 1, px, py, pz), chain(K, 2, px, py, pz)
        u = np.clip(to_int_pinned(hx / hz), 0, W - 1)
        v = np.clip(to_int_pinned(hy / hz), 0, H - 1)
    uv = np.stack((u, v), -1).astype(np.int32)
    return uv, np.concatenate((uv.min(1), uv.max(1)), -1).astype(np.int32)
