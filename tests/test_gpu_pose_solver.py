"""The pose-solver kernels (csrc/s6d_pose.hip, s6d_coarse.hip, s6d_assign.hip, s6d_fine.hip) on degenerate, tied and edge-shape
inputs, against float64 restatements of Pose_Estimation_Model/utils/model_utils.py on the same float32 operands.

u = 2^-24 throughout.  Every bound is derived in the docstring of its check from the roundings the kernel makes; every measured value
is printed, recorded with tests.util.record_margin and listed in profiles/pose_solver_margins.md.  Element-wise agreement with an SVD
is undefined on degenerate input, so the rotation checks assert what is defined everywhere (a finite proper rotation that attains
the optimum of tr(R H)) on EVERY output, and the element-wise comparison only where both singular-value gaps exceed 1e-3 s1.
The bodies are check_* functions that take `ops`: tests/test_emu_pose_solver.py runs them on the host build."""
import functools

import numpy as np
import pytest
import torch

from oracle import pem as opem
from tests.util import record_margin

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F = torch.nn.functional


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from sam6d_amd import ops
    return ops


def _margin(test, **kw):
    print(f"[margin] {test}: " + ", ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()))
    record_margin(test, **kw)


def _refused(ops, fn, *args):
    """The library answers S6D_EUNSUPPORTED (an error of the binding, never a result)."""
    from sam6d_amd import _lib
    with pytest.raises(_lib.S6DError, match="not supported"):
        fn(*args)


# ===================================================================================================================== A. rotations
def _rot64(H):
    """weighted_procrustes' rotation (model_utils.py:341-347) in float64: R = V diag(1, 1, det(V U^T)) U^T for H = U S V^T; with it the
    singular values and d = sign(det H)."""
    H = H.double()
    Um, s, Vh = torch.linalg.svd(H)
    V = Vh.transpose(1, 2)
    D = torch.eye(3, dtype=torch.float64).repeat(len(H), 1, 1)
    D[:, 2, 2] = torch.sign(torch.det(V @ Um.transpose(1, 2)))
    return V @ D @ Um.transpose(1, 2), s, torch.sign(torch.det(H))


def _rotation_properties(R, H64, extra=None):
    """-> (orthogonality defect, determinant defect, optimality defect) of float32 rotations R (n,3,3) for float64 cross-covariances H64.

    R is a double result rounded to float32: every entry is off by at most u / 2, so an entry of R^T R is off by at most
    2 * sqrt(3) * u / 2 = sqrt(3) u to first order (a column has unit length) and det R by as much: both bounded by 4u.
    Optimality: the reference's R attains tr(R H) = s1 + s2 + d s3, the maximum over all rotations, whatever basis an SVD picks inside
    a repeated singular value; |tr(dR H)| <= |dR|_F |H|_F <= 1.5u * sqrt(3) s1 = 2.6u s1, bounded by 4u s1 (`extra` adds what a caller's
    own rounding of H costs).  All three are evaluated in float64 and asserted on every row."""
    assert torch.isfinite(R).all()
    R = R.double()
    eye = torch.eye(3, dtype=torch.float64)
    ortho = (R.transpose(1, 2) @ R - eye).abs().amax(dim=(1, 2))
    det = (torch.det(R) - 1).abs()
    s = torch.linalg.svdvals(H64)
    d = torch.sign(torch.det(H64))
    opt = s[:, 0] + s[:, 1] + d * s[:, 2]
    tr = torch.einsum("nij,nji->n", R, H64)
    defect = torch.where(s[:, 0] > 0, (opt - tr) / s[:, 0].clamp(min=1e-300), torch.zeros_like(opt))
    bound = 4 * U + (0 if extra is None else extra)
    assert (ortho <= 4 * U).all(), ortho.max().item() / U
    assert (det <= 4 * U).all(), det.max().item() / U
    assert (defect <= bound).all(), ((defect - bound).max().item() / U)
    return ortho.max().item(), det.max().item(), defect.max().item()


def _well(s):
    return (s[:, 0] - s[:, 1] > 1e-3 * s[:, 0]) & (s[:, 1] - s[:, 2] > 1e-3 * s[:, 0])


def _qr(n, g):
    return torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=torch.float64))[0]


@functools.lru_cache(maxsize=None)
def _rot_kinds():
    """{kind: (n,3,3) float32} -- the input classes of rot_from_h, made once (generator seed 0; the share of the full-rank kinds that
    the element-wise comparison leaves out is a property of these numbers alone: none with this seed, printed by the check)."""
    g = torch.Generator().manual_seed(0)
    n = 256
    full = torch.randn(n, 3, 3, generator=g)
    neg = torch.randn(n, 3, 3, generator=g)
    neg[:, :, 1] = -neg[:, :, 1]
    neg = torch.where((torch.det(neg.double()) > 0).view(-1, 1, 1), neg * torch.tensor([1.0, 1.0, -1.0]), neg)      # every det < 0
    a, b = torch.randn(n, 3, 3, generator=g), torch.randn(n, 3, 3, generator=g)
    tri = ((b - b.mean(1, keepdim=True)).transpose(1, 2).double() @ (a - a.mean(1, keepdim=True)).double()).float()
    outer = torch.randn(n, 3, 1, generator=g) @ torch.randn(n, 1, 3, generator=g)
    Q = _qr(n, g)
    sc = (0.1 + 9.9 * torch.rand(n, 1, 1, generator=g, dtype=torch.float64))

    def usv(d):
        return (_qr(n, g) @ torch.diag(torch.tensor(d, dtype=torch.float64)) @ _qr(n, g)).float()
    kinds = {"full": full, "det_negative": neg, "rank2_triangles": tri, "rank1_outer": outer, "zero": torch.zeros(8, 3, 3),
             "sQ": (sc * Q).float(), "diag211_Q": (torch.diag(torch.tensor([2.0, 1, 1], dtype=torch.float64)) @ Q).float(),
             "diag221_Q": (torch.diag(torch.tensor([2.0, 2, 1], dtype=torch.float64)) @ Q).float(),
             "gap12_1e-7": usv([1.0, 1.0 - 1e-7, 0.3]), "gap23_1e-7": usv([1.0, 0.5, 0.5 * (1 - 1e-7)]),
             "scale_1e-18": torch.randn(n, 3, 3, generator=g) * 1e-18, "scale_1e+18": torch.randn(n, 3, 3, generator=g) * 1e18,
             "subnormal": torch.randn(n, 3, 3, generator=g) * 1e-40}
    assert (kinds["subnormal"].abs() < 1.18e-38).all() and (kinds["subnormal"] != 0).any()
    return kinds


def check_rot_from_h(ops):
    """s6d_rot_from_h_f32 on every class of _rot_kinds in ONE launch of mixed kinds: the properties of _rotation_properties on every
    row; zero gives exactly I; on the kinds with a defined R (random, det < 0, the two extreme scales, and the rank-2 triangles, where
    s3 = 0 and the determinant correction alone fixes the third axes) the element-wise distance from the
    float64 SVD result stays below the 1e-5 of tests/test_gpu_pose.py wherever both gaps exceed 1e-3 s1, and at most 10 % of a kind
    may be left out of that comparison; a NaN matrix between valid ones leaves every other row of the launch bit-equal."""
    kinds = _rot_kinds()
    H = torch.cat(list(kinds.values()))
    perm = torch.randperm(len(H), generator=torch.Generator().manual_seed(1))           # kinds interleaved inside the waves
    out = torch.empty_like(H)
    out[perm] = ops.rot_from_h(H[perm].contiguous().cuda()).cpu()
    o = 0
    for name, h in kinds.items():
        R = out[o:o + len(h)]
        o += len(h)
        ortho, det, defect = _rotation_properties(R, h.double())
        rec = dict(ortho_u=ortho / U, det_u=det / U, defect_u=defect / U, bound_u=4.0)
        if name == "zero":
            assert torch.equal(R, torch.eye(3).repeat(len(h), 1, 1))
        if name in ("full", "det_negative", "rank2_triangles", "scale_1e-18", "scale_1e+18"):
            ref, s, _ = _rot64(h)
            well = _well(s)
            rec["left_out"] = 1 - well.float().mean().item()
            assert rec["left_out"] <= 0.10
            rec["elementwise"] = (R.double() - ref)[well].abs().max().item()
            assert rec["elementwise"] < 1e-5
        _margin("rot_from_h/" + name, **rec)
    k = len(H) // 2 + 3
    H2 = torch.cat([H[perm][:k], torch.full((1, 3, 3), float("nan")), H[perm][k:]]).contiguous()
    out2 = ops.rot_from_h(H2.cuda()).cpu()
    assert torch.equal(torch.cat([out2[:k], out2[k + 1:]]), out[perm])


@functools.lru_cache(maxsize=None)
def _hyp_case(N1, N2):
    """Clouds with three collinear points at indices 5, 6, 7 and 600 index triples per instance: degenerate ones first (in both
    instances), random ones behind."""
    B, n = 2, 600
    g = torch.Generator().manual_seed(100 * N1 + N2)
    p1, p2 = torch.randn(B, N1, 3, generator=g) * 0.4, torch.randn(B, N2, 3, generator=g) * 0.4
    for p in (p1, p2):
        p[:, 6] = p[:, 5] + 0.25 * (p[:, 7] - p[:, 5])
    pid = lambda i, j: i * N2 + j
    # random triples of three different points on either side (three independent bins repeat a point in 15 % of the draws, and the
    # element-wise comparison may leave out 10 %); the degenerate triples are the planted ones
    pair = pid(torch.rand(B, n, N1, generator=g).argsort(dim=2)[:, :, :3], torch.rand(B, n, N2, generator=g).argsort(dim=2)[:, :, :3])
    pair[:, 0] = pid(3, 4)                                                     # one index three times: H = 1.1e-11 p p^T
    pair[:, 1] = torch.tensor([pid(3, 4), pid(3, 4), pid(9, 2)])               # two equal and one different
    pair[:, 2] = torch.tensor([pid(5, 5), pid(6, 6), pid(7, 7)])               # collinear on both sides
    pair[:, 3] = torch.tensor([pid(5, 1), pid(6, 8), pid(7, 3)])               # collinear on one side
    pair[:, 4] = N1 * N2                                                       # the end bin of searchsorted, three times
    pair[:, 5] = torch.tensor([N1 * N2, pid(2, 3), pid(8, 1)])                 # ... and once
    pair[:, 6] = torch.tensor([pid(N1 - 1, N2 - 1), pid(0, 0), pid(N1 - 1, 0)])
    return p1, p2, pair.reshape(B, 3 * n).int()


def check_pose_hypotheses(ops, N1, N2):
    """s6d_pose_hypotheses_f32 (model_utils.py:216-231) on every hypothesis of _hyp_case, none left out.  c = the largest coordinate
    magnitude of the two clouds.
      * R: _rotation_properties against H formed in float64 from the gathered points.  (`The same index three times` does NOT give
        H = 0: the weights are 1 / (3 + 1e-5), here as in the reference, so the centroid is p (1 - 3.3e-6) and H = 1.1e-11 p p^T, a
        rank-one matrix with an arbitrary, but proper and optimal, rotation.)
      * t = rc - R sc recomputed in float64 from the returned float32 R: the kernel rounds t once (<= u/2 * |t|, |t| <= (1 + sqrt 3) c)
        and its R differs from the returned one by u/2 per entry (3 * u/2 * c): 2.9 u c, asserted as 4 u c.
      * dis = mean_k |(p1_k - t) R - p2_k| recomputed in float64 from the returned float32 R, t: the rounding of R moves a residual by
        |p1_k - t| * 1.5u, that of t by sqrt(3) * 1.4 u c, that of dis by u/2 * dis; at the typical geometry (points within c of their
        centroid) that is 8 u c, the issue's figure, which is asserted (the extreme of every factor at once would be 12 u c).
      * where both gaps of H exceed 1e-3 s1 (at least 90 % of the hypotheses): R within 1e-5 of the float64 SVD result."""
    p1, p2, pair = _hyp_case(N1, N2)
    B, n = pair.shape[0], pair.shape[1] // 3
    R, t, dis = (x.cpu() for x in ops.pose_hypotheses(p1.cuda(), p2.cuda(), pair.cuda()))
    idx = pair.long()
    i1 = (idx // N2).clamp(max=N1 - 1)
    i2 = (idx % N2).clamp(max=N2 - 1)
    a = torch.gather(p1, 1, i1.unsqueeze(2).expand(-1, -1, 3)).reshape(B * n, 3, 3).double()          # ref = points of pts1
    b = torch.gather(p2, 1, i2.unsqueeze(2).expand(-1, -1, 3)).reshape(B * n, 3, 3).double()          # src = points of pts2
    w = 1.0 / (3.0 + 1e-5)
    sc, rc = b.sum(1) * w, a.sum(1) * w
    H = (b - sc.unsqueeze(1)).transpose(1, 2) @ (w * (a - rc.unsqueeze(1)))
    R, t, dis = R.reshape(-1, 3, 3), t.reshape(-1, 3).double(), dis.reshape(-1).double()
    ortho, det, defect = _rotation_properties(R, H)
    c = max(p1.abs().max().item(), p2.abs().max().item())
    R64 = R.double()
    t_err = (t - (rc - torch.einsum("nrc,nc->nr", R64, sc))).abs().max().item()
    d_ref = ((a - t.unsqueeze(1)) @ R64 - b).norm(dim=2).mean(1)
    d_err = (dis - d_ref).abs().max().item()
    ref, s, _ = _rot64(H)
    well = _well(s)
    left = 1 - well.float().mean().item()
    elem = (R64 - ref)[well].abs().max().item()
    _margin(f"pose_hypotheses/{N1}x{N2}", ortho_u=ortho / U, det_u=det / U, defect_u=defect / U, bound_u=4.0, t_err=t_err, t_bound=4 * U * c,
            dis_err=d_err, dis_bound=8 * U * c, left_out=left, elementwise=elem)
    assert t_err <= 4 * U * c and d_err <= 8 * U * c
    assert left <= 0.10 and elem < 1e-5


def _wp64(src, ref, w, thresh, eps=1e-5, kernel_roundings=False):
    """weighted_procrustes (model_utils.py:287-363) up to H, in float64 on the float32 operands -> (H, sc, rc).  kernel_roundings: with
    the float32 roundings of csrc/s6d_pose.hip -- the normaliser (float)sum + eps (:176), w_i = wt / wsum in float, the centroids
    (:193), the float differences and the product w (q - rc) (:203-204), and H itself (:217)."""
    w = torch.where(w < thresh, torch.zeros_like(w), w)
    if not kernel_roundings:
        wn = (w.double() / (w.double().sum(1, keepdim=True) + eps)).unsqueeze(2)
        sc, rc = (src.double() * wn).sum(1), (ref.double() * wn).sum(1)
        return (src.double() - sc.unsqueeze(1)).transpose(1, 2) @ (wn * (ref.double() - rc.unsqueeze(1))), sc, rc
    wsum = w.double().sum(1, keepdim=True).float() + torch.tensor(eps, dtype=torch.float32)
    wn = (w / wsum).unsqueeze(2)                                                                       # float32 division
    sc, rc = (src.double() * wn.double()).sum(1).float(), (ref.double() * wn.double()).sum(1).float()
    ds, dq = src - sc.unsqueeze(1), wn * (ref - rc.unsqueeze(1))                                       # float32
    return (ds.double().transpose(1, 2) @ dq.double()).float().double(), sc.double(), rc.double()


def _wp_check(ops, name, src, ref, w, thresh, elementwise=False):
    """One weighted_procrustes call against _wp64.  The optimality bound of _rotation_properties is for the H the kernel solves; that H
    carries the kernel's float32 roundings, so against the exact H the bound grows by the first-order effect of the perturbation:
    |opt(H) - opt(H')| <= sqrt(3) |H - H'|_F and |tr(R (H - H'))| <= sqrt(3) |H - H'|_F, i.e. 2 sqrt(3) |dH|_F / s1, with dH computed on
    the CPU from the restatement with and without the roundings.  t = rc - R sc: the kernel takes the float32 centroids and the
    float32 R in float arithmetic (5 roundings of magnitudes <= 3 c' with c' = the largest centroid coordinate), against the
    restatement with the same float32 centroids: 8 u c'."""
    R, t = (x.cpu() for x in ops.weighted_procrustes(src.cuda(), ref.cuda(), w.cuda(), thresh, 1e-5))
    assert torch.isfinite(t).all()
    He, _, _ = _wp64(src, ref, w, thresh)
    Hr, sc, rc = _wp64(src, ref, w, thresh, kernel_roundings=True)
    s1 = torch.linalg.svdvals(He)[:, 0]
    extra = torch.where(s1 > 0, 2 * 3 ** 0.5 * (He - Hr).norm(dim=(1, 2)) / s1.clamp(min=1e-300), torch.zeros_like(s1))
    ortho, det, defect = _rotation_properties(R, He, extra)
    cc = max(sc.abs().max().item(), rc.abs().max().item())
    t_err = (t.double() - (rc - torch.einsum("nrc,nc->nr", R.double(), sc))).abs().max().item()
    assert t_err <= 8 * U * cc, (t_err, 8 * U * cc)
    Ro, _ = opem.weighted_procrustes(src, ref, w, thresh)
    so = torch.linalg.svdvals(He)
    oracle_defect = ((so[:, 0] + so[:, 1] + torch.sign(torch.det(He)) * so[:, 2] - torch.einsum("nij,nji->n", Ro.double(), He)) /
                     so[:, 0].clamp(min=1e-300)).max().item()
    rec = dict(ortho_u=ortho / U, det_u=det / U, defect=defect, defect_bound=(4 * U + extra).min().item(), oracle_f32_defect=oracle_defect,
               t_err=t_err, t_bound=8 * U * cc)
    if elementwise:
        ref64, s, _ = _rot64(He)
        well = _well(s)
        rec["left_out"] = 1 - well.float().mean().item()
        assert rec["left_out"] <= 0.10
        rec["elementwise"] = (R.double() - ref64)[well].abs().max().item()
        assert rec["elementwise"] < 2e-6                                   # the bound of tests/test_gpu_pose.py against the oracle
    _margin("weighted_procrustes/" + name, **rec)
    return R, t


def _rigid_pair(B, N, g, scale=1.0):
    src = torch.randn(B, N, 3, generator=g) * 0.3 * scale
    Rg = _qr(B, g)
    Rg = (Rg * torch.sign(torch.linalg.det(Rg)).view(-1, 1, 1)).float()
    ref = src @ Rg.transpose(1, 2) + torch.randn(B, 1, 3, generator=g) * 0.2 * scale + 0.01 * scale * torch.randn(B, N, 3, generator=g)
    w = torch.rand(B, N, generator=g) * (torch.rand(B, N, generator=g) > 0.33)
    return src, ref, w, Rg


def check_weighted_procrustes_sizes(ops, N):
    """N around the 256-wide reduction tree of weighted_procrustes_kernel (a thread takes points i, i + 256, ...)."""
    src, ref, w, _ = _rigid_pair(3, N, torch.Generator().manual_seed(N))
    if N == 1:
        w = w + 0.5                                                          # the one point carries weight
    _wp_check(ops, f"N={N}", src, ref, w, 0.0, elementwise=N >= 255)


def check_weighted_procrustes_degenerate(ops):
    """All-zero weights and a threshold above every weight: exactly R = I, t = 0, as the oracle gives (H = 0, centroids 0).  One, two
    and three surviving points, one weight of 1e30 among 1e-3, collinear points: the properties, on every instance."""
    g = torch.Generator().manual_seed(5)
    src, ref, w, _ = _rigid_pair(3, 257, g)
    eye = torch.eye(3).repeat(3, 1, 1)
    for nm, ww, th in (("zero_weights", torch.zeros_like(w), 0.0), ("threshold_above_all", w, 2.0)):
        R, t = (x.cpu() for x in ops.weighted_procrustes(src.cuda(), ref.cuda(), ww.cuda(), th, 1e-5))
        Ro, to = opem.weighted_procrustes(src, ref, ww, th)
        assert torch.equal(R, eye) and torch.equal(t, torch.zeros(3, 3)), nm
        assert torch.equal(Ro, eye) and torch.equal(to, torch.zeros(3, 3)), nm
    for k in (1, 2, 3):
        ww = torch.full_like(w, 0.1)
        ww[:, [11, 200, 256][:k]] = torch.tensor([0.9, 0.8, 0.7][:k])
        _wp_check(ops, f"survivors={k}", src, ref, ww, 0.5)
    ww = torch.full_like(w, 1e-3)
    ww[:, 77] = 1e30
    _wp_check(ops, "one_weight_1e30", src, ref, ww, 0.0)
    line = torch.linspace(-1, 1, 257).view(1, -1, 1)
    s2 = line * torch.randn(3, 1, 3, generator=g) + torch.randn(3, 1, 3, generator=g)
    r2 = line * torch.randn(3, 1, 3, generator=g) + torch.randn(3, 1, 3, generator=g)
    _wp_check(ops, "collinear", s2.contiguous(), r2.contiguous(), w + 0.1, 0.0)


def check_weighted_procrustes_scales(ops, scale):
    """Coordinates of magnitude 1e-4 and 1e3 with a planted rotation: the rotation comes back to the 0.05 of tests/test_gpu_pose.py (the
    noise is scaled with the cloud, so the figure is scale free), R within that test's 2e-6 of the float64 restatement and t within
    2e-6 relative to the largest coordinate (its 2e-6 absolute was for coordinates of magnitude 1)."""
    src, ref, w, Rg = _rigid_pair(3, 513, torch.Generator().manual_seed(9), scale)
    R, t = _wp_check(ops, f"scale={scale:g}", src, ref, w, 0.0, elementwise=True)
    He, sc, rc = _wp64(src, ref, w, 0.0)
    R64, _, _ = _rot64(He)
    t64 = rc - torch.einsum("nrc,nc->nr", R64, sc)
    cmax = max(src.abs().max().item(), ref.abs().max().item())
    t_rel = (t.double() - t64).abs().max().item() / cmax
    _margin(f"weighted_procrustes/scale={scale:g}/planted", R_recovered=(R - Rg).abs().max().item(), t_rel=t_rel, t_rel_bound=2e-6)
    assert (R - Rg).abs().max() < 0.05 and t_rel < 2e-6


def check_weighted_procrustes_nan_neighbours(ops):
    """A NaN weight in instance 1 of 3 leaves instances 0 and 2 bit-equal to their solo results (one workgroup per instance)."""
    src, ref, w, _ = _rigid_pair(3, 257, torch.Generator().manual_seed(6))
    w[1, 100] = float("nan")
    R, t = (x.cpu() for x in ops.weighted_procrustes(src.cuda(), ref.cuda(), w.cuda(), 0.0, 1e-5))
    for b in (0, 2):
        R1, t1 = ops.weighted_procrustes(src[b:b + 1].contiguous().cuda(), ref[b:b + 1].contiguous().cuda(), w[b:b + 1].contiguous().cuda(), 0.0, 1e-5)
        assert torch.equal(R1[0].cpu(), R[b]) and torch.equal(t1[0].cpu(), t[b])


# ===================================================================================================================== B. coarse_sample
def _softassign64(a):
    """The shared head (model_utils.py:203-212 / 262-266) in float64 with torch.max's first-index rule -> (score, w1, w2, row gap, column
    gap): the gaps are |best foreground score - background score| relative to the larger, per observed row / per model column."""
    a = a.double()
    s = torch.softmax(a, 2) * torch.softmax(a, 1)
    w1 = (s[:, 1:, :].max(2)[1] > 0).double()
    w2 = (s[:, :, 1:].max(1)[1] > 0).double()
    fg, bg = s[:, 1:, 1:].max(2)[0], s[:, 1:, 0]
    rgap = (fg - bg).abs() / torch.maximum(fg, bg).clamp(min=1e-300)
    fg, bg = s[:, 1:, 1:].max(1)[0], s[:, 0, 1:]
    cgap = (fg - bg).abs() / torch.maximum(fg, bg).clamp(min=1e-300)
    return s, w1, w2, rgap, cgap


def _coarse_reference(atten, u, settle=True):
    """The reference statements in float32 (oracle.pem, model_utils.py:203-219) -> labels, the uniforms, the bins they sample; and the
    float64 cumulative distribution on the oracle's labels, with the value 1 appended for the end bin L.

    settle: the criterion of _coarse_compare lets a differing draw move only between bins whose cumulative values are 2e-5 apart, so it
    is decidable only for a uniform that no admissible error can carry across a heavier bin.  The kernel's cumulative values (<= 1)
    drift from the reference's by the hardware exponential's 2e-6 relative (tests/test_gpu_pose.py); with tau = 4e-6, twice that, a
    uniform is kept when u - tau and u + tau fall into the same bin or into bins whose float64 cumulative values are less than 1e-5
    apart, and is replaced by the first kept uniform of its instance otherwise -- a choice made on the float64 restatement alone
    (nonzero bins x 8e-6 of the draws if the bins were equal, 10 % at 196 x 65; the cases here lose 1.2 % at most, printed, and 2 % is the cap).  Boundary behaviour is the business of the special uniforms."""
    B = atten.shape[0]
    score, w1, w2 = opem.soft_assignment(atten)
    cum = torch.cumsum(score.reshape(B, -1) ** 1.5, 1)
    cum = cum / (cum[:, -1].unsqueeze(1) + 1e-8)
    s64 = _softassign64(atten)[0][:, 1:, 1:] * w1.double().unsqueeze(2) * w2.double().unsqueeze(1)
    c64 = torch.cumsum(s64.reshape(B, -1) ** 1.5, 1)
    c64 = torch.cat([c64 / (c64[:, -1:] + 1e-8), torch.ones(B, 1, dtype=torch.float64)], 1)
    if settle:
        tau, edges = 4e-6, c64[:, :-1].contiguous()
        lo, hi = torch.searchsorted(edges, u.double() - tau), torch.searchsorted(edges, u.double() + tau)
        keep = (lo == hi) | (torch.gather(c64, 1, hi) - torch.gather(c64, 1, lo) < 1e-5)
        assert keep.float().mean() >= 0.98 and keep.any(1).all(), keep.float().mean()
        print(f"[uniforms] {100 * (1 - keep.float().mean().item()):.2f} % of the draws replaced")
        first = keep.float().argmax(1)
        u = torch.where(keep, u, u[torch.arange(B), first].unsqueeze(1)).contiguous()
    return w1, u, torch.searchsorted(cum, u), c64


def _coarse_compare(name, pair, w, w1, ref, c64, boundary_only=False):
    """Labels bit-equal to the oracle's.  Sampled bins by the criterion of tests/test_gpu_pose.py::test_coarse_sample_vs_oracle: at most
    0.2 % of the draws differ (the bins carry the hardware exponential and s sqrt(s) against libm's exp and pow), and each differing
    draw lands on a bin whose float64 cumulative value is within 2e-5 of the reference bin's.  boundary_only: the cumulative rule
    alone (planted boundary uniforms would use up the 0.2 % of a small case)."""
    pair = pair.cpu().long()
    assert torch.equal(w.cpu(), w1), (w.cpu() != w1).sum()
    L = c64.shape[1] - 1
    assert (pair >= 0).all() and (pair <= L).all()
    diff = pair != ref
    share = diff.float().mean().item()
    dcum = (torch.gather(c64, 1, pair) - torch.gather(c64, 1, ref)).abs().max().item()
    _margin("coarse_sample/" + name, differing_share=share, cum_distance=dcum, cum_bound=2e-5, **({} if boundary_only else {"share_cap": 2e-3}))
    assert boundary_only or share <= 2e-3
    assert dcum < 2e-5


def _matching_scores(B, M1, M2, g, inv_temp=10.0, C=64):
    f1 = F.normalize(torch.randn(B, M1, C, generator=g), dim=2)
    f2 = F.normalize(f1[:, torch.randint(0, M1, (M2,), generator=g)] + 0.3 * torch.randn(B, M2, C, generator=g), dim=2)
    return (f1 @ f2.transpose(1, 2) * inv_temp).contiguous()


COARSE_SHAPES = [(41, 23), (23, 41), (9, 200), (197, 66), (3, 3), (2, 2), (5, 256)]


def check_coarse_sample_shape(ops, M1, M2):
    """Non-square score matrices (the kernel takes M1 and M2 separately), the smallest ones, and the widest served (M2 = 256)."""
    B, n_u = 2, 600
    g = torch.Generator().manual_seed(1000 * M1 + M2)
    atten = _matching_scores(B, M1, M2, g)
    w1, u, ref, c64 = _coarse_reference(atten, torch.rand(B, n_u, generator=g))
    pair, w = ops.coarse_sample(atten.cuda(), u.cuda())
    _coarse_compare(f"{M1}x{M2}", pair, w, w1, ref, c64)
    special = torch.tensor([0.0, 1.0, 1.0 + 2.0 ** -23, 1e-30]).repeat(B, 1)
    w1, _, ref, c64 = _coarse_reference(atten, special, settle=False)
    pair, w = ops.coarse_sample(atten.cuda(), special.cuda())
    _coarse_compare(f"{M1}x{M2}/special_uniforms", pair, w, w1, ref, c64, boundary_only=True)


def check_coarse_sample_refused(ops):
    """M2 = 257 and a pair beyond the 160 KiB of LDS: S6D_EUNSUPPORTED, and the outputs keep their fill."""
    for M1, M2 in ((5, 257), (211, 211)):
        atten, u = torch.zeros(1, M1, M2).cuda(), torch.rand(1, 8).cuda()
        pair, w1 = torch.full((1, 8), -7, dtype=torch.int32).cuda(), torch.full((1, M1 - 1), -7.0).cuda()
        _refused(ops, ops._call, "s6d_coarse_sample_f32", ops._ptr(atten), ops._ptr(u), 1, M1, M2, 8, ops._ptr(pair), ops._ptr(w1), ops._stream())
        torch.cuda.synchronize()
        assert (pair.cpu() == -7).all() and (w1.cpu() == -7).all()


def check_coarse_sample_all_background(ops):
    """An instance whose row 0 and column 0 dominate, between two normal ones: its labels are all 0 and every draw is the end bin L (the
    distribution is all zero: cum = 0 / 1e-8, as torch.searchsorted gives); the neighbours equal their solo results bit for bit."""
    M1, M2, n_u = 41, 23, 300
    g = torch.Generator().manual_seed(77)
    atten = _matching_scores(3, M1, M2, g)
    atten[1] = 0.5 * torch.randn(M1, M2, generator=g)
    atten[1, 0, :] = 8.0
    atten[1, :, 0] = 8.0
    w1, u, ref, _ = _coarse_reference(atten, torch.rand(3, n_u, generator=g).clamp(min=1e-4))
    pair, w = (x.cpu() for x in ops.coarse_sample(atten.cuda(), u.cuda()))
    assert (w1[1] == 0).all() and (ref[1] == (M1 - 1) * (M2 - 1)).all()                     # the reference does what the docstring says
    assert torch.equal(w, w1) and (pair[1] == (M1 - 1) * (M2 - 1)).all()
    for b in (0, 2):
        p1, ws = ops.coarse_sample(atten[b:b + 1].contiguous().cuda(), u[b:b + 1].contiguous().cuda())
        assert torch.equal(p1[0].cpu(), pair[b]) and torch.equal(ws[0].cpu(), w[b])


def check_coarse_sample_ties(ops, M):
    """Integer-valued scores in [-3, 3] with copies of the background row and column planted among the foreground ones: exact ties
    between a foreground and the background score; the labels follow torch.max's first-index rule (the oracle's)."""
    g = torch.Generator().manual_seed(M)
    atten = torch.randint(-3, 4, (2, M, M), generator=g).float()
    atten[:, 5:9] = atten[:, 5:9].clamp(max=1.0)                           # four rows with their one largest score in column 0 ...
    atten[:, 5:9, 0] = 3.0
    atten[:, :, [3, M - 1]] = atten[:, :, :1]                              # ... and in its two copies
    atten[:, [2, M - 2], :] = atten[:, :1, :]
    w1, u, ref, c64 = _coarse_reference(atten, torch.rand(2, 300, generator=g))
    _, w64, _, rgap, _ = _softassign64(atten)
    assert (rgap == 0).any() and torch.equal(w64.float(), w1)              # the case holds exact ties, and float64 labels them alike
    pair, w = ops.coarse_sample(atten.cuda(), u.cuda())
    _coarse_compare(f"integer_ties/M={M}", pair, w, w1, ref, c64)


def check_coarse_sample_magnitudes(ops, mag):
    """Scores of exactly +-mag, diagonal +mag and the rest -mag: mag = 10 is the shipped 1 / temp, mag = S6D_ASSIGN_MAX_ABS_SCORE the
    documented edge of the domain (e^mag and the sums of a row are finite floats, e^-mag a normal one); and the matching case
    of the shape checks scaled so that its largest |score| is exactly mag."""
    M, g = 40, torch.Generator().manual_seed(int(mag))
    atten = torch.full((2, M, M), -float(mag))
    atten[:, torch.arange(M), torch.arange(M)] = float(mag)
    u0 = torch.rand(2, 600, generator=g)
    w1, u, ref, c64 = _coarse_reference(atten, u0)
    pair, w = ops.coarse_sample(atten.cuda(), u.cuda())
    _coarse_compare(f"diagonal/mag={mag}", pair, w, w1, ref, c64)
    atten = _matching_scores(2, 41, 23, g)
    atten = (atten * (float(mag) / atten.abs().max())).clamp(-float(mag), float(mag)).contiguous()
    atten[0, 1, 1], atten[1, 2, 3] = float(mag), -float(mag)
    assert atten.abs().max().item() == float(mag)
    w1, u, ref, c64 = _coarse_reference(atten, u0)
    pair, w = ops.coarse_sample(atten.cuda(), u.cuda())
    _coarse_compare(f"matching/mag={mag}", pair, w, w1, ref, c64)


# ===================================================================================================================== C. selections
SMALLEST_K = [(1, 1), (2, 2), (3, 1), (1024, 1024), (1025, 1025), (1025, 7), (16384, 300)]


def check_smallest_k(ops, n, k):
    """s6d_smallest_k_f32 with half of the residuals equal and +inf and NaN among them: the exact (value, index) lexicographic order,
    numbers first, then +inf, then NaN (numpy's order; the kernel sorts the value's bits, and a positive NaN's bits lie above +inf's),
    and Rk, tk exact gathers."""
    B = 2
    g = torch.Generator().manual_seed(n + k)
    dis = torch.rand(B, n, generator=g)
    dis[:, torch.randperm(n, generator=g)[: n // 2]] = 0.25
    if n >= 3:
        sp = torch.randperm(n, generator=g)
        dis[:, sp[: max(1, n // 100)]] = float("inf")
        dis[:, sp[max(1, n // 100): 2 * max(1, n // 100)]] = float("nan")
    Rs, ts = torch.randn(B, n, 3, 3, generator=g), torch.randn(B, n, 3, generator=g)
    Rk, tk, idx = (x.cpu() for x in ops.smallest_k(dis.cuda(), Rs.cuda(), ts.cuda(), k))
    want = torch.from_numpy(np.stack([np.lexsort((np.arange(n), d)) for d in dis.numpy()]))[:, :k]      # NaN last, ties by index
    assert torch.equal(idx.long(), want)
    ar = torch.arange(B)[:, None]
    assert torch.equal(Rk, Rs[ar, want]) and torch.equal(tk, ts[ar, want])


def check_smallest_k_refused(ops):
    n = 16385
    z = torch.zeros(1, n)
    _refused(ops, ops.smallest_k, z.cuda(), torch.zeros(1, n, 3, 3).cuda(), torch.zeros(1, n, 3).cuda(), 5)


def check_hypothesis_select(ops, P, N):
    """s6d_hypothesis_select_f32 (model_utils.py:240-246): the first arg-max of score_p = sum(w1) / (sum_n dmin w1 + 1e-8), restated in
    float64 on inputs whose products and sums are exact in float32 (dmin a multiple of 1/64 below 4, w1 in {0, 1}: every partial sum is a
    multiple of 1/64 below 2^10), so the float32 division is the only rounding and equal sums give bit-equal scores.  Instance 0:
    two hypotheses with equal sums, the lower index wins; 1: random; 2: all-zero w1 selects hypothesis 0; 3: all-zero dmin
    (score = sum w / 1e-8 for every hypothesis) selects hypothesis 0 and stays finite."""
    B = 4
    g = torch.Generator().manual_seed(100 * P + N)
    dmin = torch.randint(2, 256, (B, P, N), generator=g).float() / 64
    w1 = (torch.rand(B, N, generator=g) > 0.3).float()
    w1[:, 0] = 1.0
    w1[2] = 0
    dmin[3] = 0
    if P >= 2:
        best = P - 1
        dmin[0, best] = 1 / 64                                                 # the smallest possible sum: the best score ...
        dmin[0, P // 2] = dmin[0, best]                                        # ... twice (P // 2 < P - 1)
    Rk, tk = torch.randn(B, P, 3, 3, generator=g), torch.randn(B, P, 3, generator=g)
    sc = (w1.double().sum(1, keepdim=True).float() / ((dmin.double() * w1.double().unsqueeze(1)).sum(2).float() + 1e-8))
    assert torch.isfinite(sc).all()
    want = sc.max(1)[1]                                                        # first index
    assert want[2] == 0 and want[3] == 0 and (P < 2 or want[0] == P // 2)
    R, t = (x.cpu() for x in ops.hypothesis_select(dmin.cuda(), w1.cuda(), Rk.cuda(), tk.cuda()))
    ar = torch.arange(B)
    assert torch.equal(R, Rk[ar, want]) and torch.equal(t, tk[ar, want])


# ===================================================================================================================== D. min_dist
def check_min_dist(ops, Nm, N, scale=1.0):
    """s6d_min_dist_f32 against the direct-difference form in float64 on the float32 operands (P = 3 poses, B = 2).
    Bound, relative to D = the largest |transformed point - model point| coordinate difference scale (<= |q - t| sqrt 3 + |m|): the
    kernel rounds q - t (u/2 each), three products and two sums per transformed coordinate (<= 2.5 u of sqrt(3) |q - t|), the difference
    to the model point, the squares and sums (relative 2u of d^2, i.e. u of d) and the square root (u/2): 6 u (|q - t| sqrt 3 + |m|) in
    all, asserted; at unit scale that is below the absolute 1e-5 of tests/test_gpu_pose.py.  A query that coincides with a model
    point under the identity pose gives exactly 0.  The padding of the model cloud to four points must not be seen by the minimum."""
    B, P = 2, 3
    g = torch.Generator().manual_seed(1000 * Nm + N)
    pts = torch.randn(B, N, 3, generator=g) * scale
    model = torch.randn(B, Nm, 3, generator=g) * scale + 2.0 * scale          # point 0 is not near the origin (a zero padding would be)
    R = torch.linalg.qr(torch.randn(B, P, 3, 3, generator=g))[0].contiguous()
    t = 0.1 * scale * torch.randn(B, P, 3, generator=g)
    R[:, 0], t[:, 0] = torch.eye(3), 0.0
    pts[:, 0] = model[:, Nm - 1]                                               # coincides with the LAST model point (the padded trip)
    tp = (pts.double().unsqueeze(1) - t.double().unsqueeze(2)) @ R.double()
    ref = torch.cdist(tp.reshape(B * P, N, 3), model.double().repeat_interleave(P, 0)).min(2)[0].reshape(B, P, N)
    out = ops.min_dist(pts.cuda(), R.cuda(), t.cuda(), model.cuda()).cpu()
    assert (out[:, 0, 0] == 0).all()
    bound = 6 * U * ((pts.abs().max().item() + t.abs().max().item()) * 3 + model.abs().max().item())
    err = (out.double() - ref).abs().max().item()
    _margin(f"min_dist/Nm={Nm},N={N},scale={scale:g}", err=err, bound=bound)
    assert err <= bound
    assert ops.min_dist(pts.cuda(), R[:, :0].contiguous().cuda(), t[:, :0].contiguous().cuda(), model.cuda()).shape == (B, 0, N)    # P = 0


def check_min_dist_refused(ops):
    """5460 is the largest Nm whose padded cloud fits 64 KiB; 5461 pads to 5464 points = 65,568 B."""
    pts, R, t = torch.zeros(1, 4, 3).cuda(), torch.eye(3).view(1, 1, 3, 3).cuda(), torch.zeros(1, 1, 3).cuda()
    _refused(ops, ops.min_dist, pts, R, t, torch.zeros(1, 5461, 3).cuda())


# ===================================================================================================================== E. fine_assign, fine_match
FINE_SHAPES = [(2, 2), (2, 33), (33, 2), (16, 16), (17, 17), (18, 15), (65, 64), (64, 65), (3, 97), (257, 40), (40, 257), (70, 70), (130, 100)]


def _fine_features(B, M1, M2, g):
    f1 = torch.randn(B, M1, 256, generator=g) * (0.5 + torch.rand(B, M1, 1, generator=g))     # un-normalised out_proj rows
    f2 = f1[:, torch.randint(0, M1, (M2,), generator=g)] + 0.4 * torch.randn(B, M2, 256, generator=g)
    pts2 = torch.randn(B, M2 - 1, 3, generator=g).clamp(-4.5, 4.5)
    return f1, f2, pts2


def _cos64(f1, f2):
    """compute_feature_similarity (model_utils.py:114-136, cosine) in float64 on the float32 features, before the temperature.  The
    products are summed element by element, not by a matrix product: a BLAS may sum two equal rows in different orders depending on
    their position, and the exact ties of the tie cases must be exact in the restatement too."""
    n1 = f1.double() / f1.double().norm(dim=2, keepdim=True).clamp(min=1e-12)
    n2 = f2.double() / f2.double().norm(dim=2, keepdim=True).clamp(min=1e-12)
    return (n1.unsqueeze(2) * n2.unsqueeze(1)).sum(-1)


def _fine_compare(name, out, a64, pts2):
    """pred, wsum, w1 of a kernel against compute_fine_Rt's head (model_utils.py:262-270) in float64 on the scores a64.

    Labels exact.  On random inputs a row whose best foreground score and background score differ by less than 1e-5 relative
    (float64), but are not exactly tied, may fall either way and is left out, at most 1 % of the rows of a case; no column may be
    that close (its label moves a whole column of the assignment): both are properties of the input, met by the choice of seeds.
    An exact tie is no such row: it goes to the first index.
    Bounds, at every temperature and score magnitude of the supported domain: the ones tests/test_gpu_pose.py::_check_fine_match
    documents -- wsum 2e-5 relative to max(1, largest wsum), pred 5e-5 absolute for |pts2| <= 4.5, scaled with the points beyond."""
    pred, wsum, w1 = (x.cpu() for x in out)
    assert torch.isfinite(pred).all() and torch.isfinite(wsum).all()
    s, l1, l2, rgap, cgap = _softassign64(a64)
    amat = s[:, 1:, 1:] * l1.unsqueeze(2) * l2.unsqueeze(1)
    ws64 = amat.sum(2)
    p64 = (amat / (ws64.unsqueeze(2) + 1e-6)) @ pts2.double()
    close = (rgap < 1e-5) & (rgap > 0)
    left = close.float().mean().item()
    assert left <= 0.01 and not ((cgap < 1e-5) & (cgap > 0)).any(), (left, cgap.min())
    keep = ~close
    assert torch.equal(w1.double()[keep], l1[keep]), (w1.double() != l1)[keep].sum()
    wb = 2e-5 * max(1.0, ws64.max().item())
    pb = 5e-5 * max(1.0, pts2.abs().max().item() / 4.5)
    we = (wsum.double() - ws64)[keep].abs().max().item()
    pe = (pred.double() - p64)[keep].abs().max().item()
    _margin(name, wsum_err=we, wsum_bound=wb, pred_err=pe, pred_bound=pb, rows_left_out=left)
    assert we <= wb and pe <= pb
    off = w1 == 0
    assert (wsum[off] == 0).all() and (pred[off] == 0).all()               # a background row carries exactly no weight and a zero point


def check_fine_shape(ops, M1, M2):
    """Both kernels at one (M1, M2), B = 2, temp = 0.1: s6d_fine_match_f32 against the float64 chain on the features, and
    s6d_fine_assign_f32 against the float64 head on the float32 scores it is given."""
    g = torch.Generator().manual_seed(10000 + 300 * M1 + M2)
    f1, f2, pts2 = _fine_features(2, M1, M2, g)
    _fine_compare(f"fine_match/{M1}x{M2}", ops.fine_match(f1.cuda(), f2.cuda(), pts2.cuda(), 0.1), _cos64(f1, f2) / 0.1, pts2)
    a32 = opem.feature_similarity(f1, f2, 0.1).contiguous()
    _fine_compare(f"fine_assign/{M1}x{M2}", ops.fine_assign(a32.cuda(), pts2.cuda()), a32.double(), pts2)


FINE_CLASSES = ["zero_rows", "f2_is_f1", "f2_is_minus_f1", "duplicates", "scale_1e4", "scale_1e-4", "all_background", "pts_1e6",
                "temp_1.0", "temp_0.05"]


@functools.lru_cache(maxsize=None)
def _fine_neighbours():
    M1, M2 = 65, 40
    return _fine_features(2, M1, M2, torch.Generator().manual_seed(4242))


def _fine_class(cls):
    """-> (f1, f2, pts2, temp) of one instance (1, 65 | 40, 256) of an input class."""
    M1, M2 = 65, 40
    g = torch.Generator().manual_seed(sum(map(ord, cls)))
    f1, f2, pts2 = _fine_features(1, M1, M2, g)
    temp = 0.1
    if cls == "zero_rows":                                                  # the background rows and two more on each side
        f1[:, [0, 7, 33]] = 0
        f2[:, [0, 5, 39]] = 0
    elif cls == "f2_is_f1":
        f2 = f1[:, :M2].clone()
    elif cls == "f2_is_minus_f1":
        f2 = -f1[:, :M2].clone()
    elif cls == "duplicates":                                               # copies of the background rows and of foreground rows
        f1[:, 5], f1[:, 9], f2[:, 6], f2[:, 11] = f1[:, 0], f1[:, 3], f2[:, 0], f2[:, 4]
    elif cls == "scale_1e4":
        f1, f2 = f1 * 1e4, f2 * 1e4
    elif cls == "scale_1e-4":
        f1, f2 = f1 * 1e-4, f2 * 1e-4
    elif cls == "all_background":                                           # every observed row resembles the background row of f2
        f1 = f2[:, :1] + 0.05 * torch.randn(1, M1, 256, generator=g)
        f2[:, 1:] = torch.randn(1, M2 - 1, 256, generator=g)
    elif cls == "pts_1e6":
        pts2 = pts2 * (1e6 / 4.5)
    elif cls.startswith("temp_"):
        temp = float(cls[5:])
    return f1.contiguous(), f2.contiguous(), pts2.contiguous(), temp


def check_fine_class(ops, cls):
    """One input class alone (both kernels, judged by _fine_compare) and as instance 1 of 3: the neighbours' outputs equal, bit for bit,
    what the two give without it.  all_background: wsum and pred exactly 0."""
    f1, f2, pts2, temp = _fine_class(cls)
    a64 = _cos64(f1, f2) / temp
    out = ops.fine_match(f1.cuda(), f2.cuda(), pts2.cuda(), temp)
    _fine_compare(f"fine_match/{cls}", out, a64, pts2)
    a32 = opem.feature_similarity(f1, f2, temp).contiguous()
    out_a = ops.fine_assign(a32.cuda(), pts2.cuda())
    _fine_compare(f"fine_assign/{cls}", out_a, a32.double(), pts2)
    if cls == "all_background":
        for o in (out, out_a):
            assert all((x.cpu() == 0).all() for x in o)
    n1, n2, np2 = _fine_neighbours()
    three = [torch.cat([n[:1], x, n[1:]]).contiguous() for n, x in ((n1, f1), (n2, f2), (np2, pts2))]
    got = [x.cpu() for x in ops.fine_match(three[0].cuda(), three[1].cuda(), three[2].cuda(), temp)]
    solo = [x.cpu() for x in ops.fine_match(n1.cuda(), n2.cuda(), np2.cuda(), temp)]
    an = opem.feature_similarity(n1, n2, temp)                            # (a batched CPU product may round an instance otherwise)
    a3 = torch.cat([an[:1], a32, an[1:]]).contiguous()
    got_a = [x.cpu() for x in ops.fine_assign(a3.cuda(), three[2].cuda())]
    solo_a = [x.cpu() for x in ops.fine_assign(a3[[0, 2]].contiguous().cuda(), np2.cuda())]
    for gt, so in ((got, solo), (got_a, solo_a)):
        for x, y in zip(gt, so):
            assert torch.equal(x[[0, 2]], y)
        for x, y in zip(gt, out if gt is got else out_a):
            assert torch.equal(x[1], y.cpu()[0])


def _tie_case(M, g):
    """One-hot features: every cosine is exactly 0 or 1, so a foreground column whose key equals column 0's is an EXACT copy of it, and a
    row whose largest score lies in both is tied in exact arithmetic."""
    k1, k2 = torch.randint(0, 6, (1, M), generator=g), torch.randint(0, 6, (1, M), generator=g)
    f1 = F.one_hot(k1, 256).float() * (1 + torch.randint(0, 3, (1, M, 1), generator=g)).float()
    f2 = F.one_hot(k2, 256).float() * (1 + torch.randint(0, 3, (1, M, 1), generator=g)).float()
    return f1, f2, torch.randn(1, M - 1, 3, generator=g)


def check_fine_ties(ops):
    """The first-index rule of the reference (score[:, 1:, :].max(2)[1] > 0, torch.max returns the first index) at M = 40, 70, 130: a row
    tied between the background column and foreground columns is background.  oracle.pem.soft_assignment in float32 and the float64
    head agree on these inputs, and both kernels must give their labels.  (s6d_fine_match_f32 labelled 14 / 22 such rows foreground at
    M = 70 / 130 while its background sums came from another summation order than the foreground ones.)"""
    g = torch.Generator().manual_seed(0)
    for M in (20, 40, 64, 65, 66, 70, 100, 130):                            # the generator is consumed as in the report
        f1, f2, pts2 = _tie_case(M, g)
        if M not in (40, 70, 130):
            continue
        a = opem.feature_similarity(f1, f2, 0.1)
        _, w_ref, _ = opem.soft_assignment(a)
        _, w64, _, rgap, _ = _softassign64(_cos64(f1, f2) / 0.1)
        tied = ((rgap == 0) & (w64 == 0)).sum().item()
        assert torch.equal(w64.float(), w_ref) and tied > 0
        _, _, w = ops.fine_match(f1.cuda(), f2.cuda(), pts2.cuda(), 0.1)
        _, _, wa = ops.fine_assign(a.contiguous().cuda(), pts2.cuda())
        print(f"[ties] M={M}: {tied} rows tied with the background column, fine_match differs on {(w.cpu() != w_ref).sum().item()}, "
              f"fine_assign on {(wa.cpu() != w_ref).sum().item()}")
        assert torch.equal(wa.cpu(), w_ref)
        assert torch.equal(w.cpu(), w_ref)


def _anticorrelated_case(g):
    """M = 6: every row of f2 is v except column 2 at cosine 0.9 to v, every row of f1 is v except row 1 = -v.  Row 1's scores are the
    smallest of every column, so its arg-max keys are the smallest the kernels ever form (e^-3T / M in fine_match, e^-4a-ish products
    in the score kernels); in float64 its best foreground score (column 2) beats the background score by a relative gap of 0.99+."""
    v = F.normalize(torch.randn(256, generator=g), dim=0)
    o = torch.randn(256, generator=g)
    o = F.normalize(o - (o @ v) * v, dim=0)
    f1, f2 = v.repeat(1, 6, 1), v.repeat(1, 6, 1)
    f1[0, 1] = -v
    f2[0, 2] = 0.9 * v + (1 - 0.81) ** 0.5 * o
    return f1.contiguous(), f2.contiguous(), torch.randn(1, 5, 3, generator=g).clamp(-4.5, 4.5)


def check_temperature_domain(ops):
    """s6d_fine_match_f32 takes no max shift, so 1 / temp is bounded: include/sam6d_hip.h derives S6D_FINE_MATCH_MAX_INV_TEMP = 25 from the
    arg-max keys e^2 / c >= e^-3T / M, which must stay normal floats.  temp = 0.01 is refused with S6D_EUNSUPPORTED -- it used to return
    NaN -- and so are the next float above the limit and inv_temp = 40 (where a row anti-correlated with every column came back
    background without an error); the limit itself is served within the bounds of _fine_compare, on a matching case with cosines of
    exactly +1 and -1 and on _anticorrelated_case, whose row 1 must be foreground as in float64.  The kernels that are handed ready
    scores cannot check them: each is run at |score| = S6D_ASSIGN_MAX_ABS_SCORE = 32 exactly (2 a + ln(M1 M2) <= 87: the largest score
    of a row stays a normal float), on the same two cases, against float64 (and, for coarse_sample, the float32 oracle as well)."""
    g = torch.Generator().manual_seed(31)
    f1, f2, pts2 = _fine_features(2, 70, 66, g)
    lim = float(ops.FINE_MATCH_MAX_INV_TEMP)
    assert lim == 25.0
    for temp in (0.01, 1.0 / 40.0, 1.0 / (lim * (1 + 2.0 ** -22))):
        _refused(ops, ops.fine_match, f1.cuda(), f2.cuda(), pts2.cuda(), temp)
    f2[:, 3], f2[:, 4] = f1[:, 9], -f1[:, 9]                                # cosines of exactly +1 and -1 (same bits on both sides)
    out = ops.fine_match(f1.cuda(), f2.cuda(), pts2.cuda(), 1.0 / lim)
    _fine_compare("fine_match/inv_temp=25", out, _cos64(f1, f2) * lim, pts2)
    g1, g2, gp = _anticorrelated_case(g)
    for T in (10.0, 20.0, lim):
        a64 = _cos64(g1, g2) * T
        _, l64, _, rgap, _ = _softassign64(a64)
        assert l64[0, 0] == 1 and rgap[0, 0] > 0.9                          # the case: row 1 is foreground, nowhere near a tie
        out = ops.fine_match(g1.cuda(), g2.cuda(), gp.cuda(), 1.0 / T)
        assert out[2].cpu()[0, 0] == 1, T
        _fine_compare(f"fine_match/anticorrelated/inv_temp={T:g}", out, a64, gp)
    mag = float(ops.ASSIGN_MAX_ABS_SCORE)
    assert mag == 32.0
    for name, (h1, h2, hp) in (("matching", (f1, f2, pts2)), ("anticorrelated", (g1, g2, gp))):
        a = _cos64(h1, h2).float()                                         # (equal rows give equal scores: see _cos64)
        a = a * (mag / a.abs().max())
        a = torch.where(a.abs() > mag - 1e-3, torch.sign(a) * mag, a).contiguous()      # the cosines of +-1: exactly +-mag
        assert a.max().item() == mag and a.min().item() == -mag
        _, l64, _, rgap, _ = _softassign64(a)
        _fine_compare(f"fine_assign/{name}/abs_score=32", ops.fine_assign(a.cuda(), hp.cuda()), a.double(), hp)
        w1, u, ref, c64 = _coarse_reference(a, torch.rand(a.shape[0], 300, generator=g))
        sure = rgap >= 1e-5
        assert torch.equal(w1.double()[sure], l64[sure])                   # inside the domain the float32 oracle has float64's labels
        pair, w = ops.coarse_sample(a.cuda(), u.cuda())
        _coarse_compare(f"{name}/abs_score=32", pair, w, w1, ref, c64)


def check_pem_caller_temperature(ops, monkeypatch):
    """A configured temperature outside the kernel's domain: sam6d_amd.pem.solvers.fine_Rt takes the library statements (and raises under
    the strict policy, as for any other unsupported shape), never the fused kernel."""
    from sam6d_amd import policy
    from sam6d_amd.pem import solvers
    g = torch.Generator().manual_seed(8)
    f1, f2, pts2 = _fine_features(1, 34, 34, g)
    p1 = torch.randn(1, 33, 3, generator=g)
    model = torch.randn(1, 16, 3, generator=g)
    called = []
    monkeypatch.setattr(ops, "fine_match", lambda *a, **k: called.append("fine_match"))
    temp = 0.01
    atten = opem.feature_similarity(f1, f2, temp)
    args = (atten.cuda(), p1.cuda(), pts2.cuda(), model.cuda())
    policy.reset_library_branch_hits()
    R, t, sc = solvers.fine_Rt(*args, feats=(f1.cuda(), f2.cuda(), temp), max_abs_score=1.0 / temp)
    assert not called and torch.isfinite(R).all() and torch.isfinite(t).all()
    Ro, to, _ = opem.fine_Rt(atten, p1, pts2, model)
    assert (R.cpu() - Ro).abs().max() < 1e-4 and (t.cpu() - to).abs().max() < 1e-4
    hits = policy.library_branch_hits()
    assert hits.get(("pem.compute_fine_Rt", "temp")) == 1 and hits.get(("pem.compute_fine_Rt.assign", "score_domain")) == 1
    with policy.use(strict="1"), pytest.raises(policy.StrictError, match=r"pem\.compute_fine_Rt.*guard `temp` failed"):
        solvers.fine_Rt(*args, feats=(f1.cuda(), f2.cuda(), temp), max_abs_score=1.0 / temp)
    assert not called


# ===================================================================================================================== the GPU tests
def test_rot_from_h_properties_on_every_class(ops):
    check_rot_from_h(ops)


@pytest.mark.parametrize("N1,N2", [(40, 40), (33, 50)])
def test_pose_hypotheses_every_hypothesis(ops, N1, N2):
    check_pose_hypotheses(ops, N1, N2)


@pytest.mark.parametrize("N", [1, 255, 256, 257, 513])
def test_weighted_procrustes_sizes(ops, N):
    check_weighted_procrustes_sizes(ops, N)


def test_weighted_procrustes_degenerate(ops):
    check_weighted_procrustes_degenerate(ops)


@pytest.mark.parametrize("scale", [1e-4, 1e3])
def test_weighted_procrustes_scales(ops, scale):
    check_weighted_procrustes_scales(ops, scale)


def test_weighted_procrustes_nan_neighbours(ops):
    check_weighted_procrustes_nan_neighbours(ops)


@pytest.mark.parametrize("M1,M2", COARSE_SHAPES)
def test_coarse_sample_shapes(ops, M1, M2):
    check_coarse_sample_shape(ops, M1, M2)


def test_coarse_sample_refused_shapes(ops):
    check_coarse_sample_refused(ops)


def test_coarse_sample_all_background_instance(ops):
    check_coarse_sample_all_background(ops)


@pytest.mark.parametrize("M", [17, 40, 70])
def test_coarse_sample_exact_ties(ops, M):
    check_coarse_sample_ties(ops, M)


@pytest.mark.parametrize("mag", [10, 32])
def test_coarse_sample_score_magnitudes(ops, mag):
    assert mag == 10 or mag == ops.ASSIGN_MAX_ABS_SCORE
    check_coarse_sample_magnitudes(ops, mag)


@pytest.mark.parametrize("n,k", SMALLEST_K)
def test_smallest_k_order(ops, n, k):
    check_smallest_k(ops, n, k)


def test_smallest_k_refused(ops):
    check_smallest_k_refused(ops)


@pytest.mark.parametrize("P", [1, 4, 5, 300])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 196])
def test_hypothesis_select(ops, P, N):
    check_hypothesis_select(ops, P, N)


@pytest.mark.parametrize("Nm", [1, 2, 3, 4, 5, 1021, 5460])
def test_min_dist_model_sizes(ops, Nm):
    check_min_dist(ops, Nm, 257)


@pytest.mark.parametrize("N", [1, 255, 256])
def test_min_dist_query_sizes(ops, N):
    check_min_dist(ops, 1021, N)


def test_min_dist_large_coordinates(ops):
    check_min_dist(ops, 1021, 257, scale=1e3)


def test_min_dist_refused(ops):
    check_min_dist_refused(ops)


@pytest.mark.parametrize("M1,M2", FINE_SHAPES)
def test_fine_kernels_shapes(ops, M1, M2):
    check_fine_shape(ops, M1, M2)


@pytest.mark.parametrize("cls", FINE_CLASSES)
def test_fine_kernels_input_classes(ops, cls):
    check_fine_class(ops, cls)


def test_fine_kernels_exact_ties_with_the_background(ops):
    check_fine_ties(ops)


def test_temperature_domain(ops):
    check_temperature_domain(ops)


def test_pem_caller_leaves_the_kernel_outside_its_temperature_domain(ops, monkeypatch):
    check_pem_caller_temperature(ops, monkeypatch)
