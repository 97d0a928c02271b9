"""The index stage of the geometric structure embedding straight from the points (get_embedding_indices, transformer.py:303-332):
s6d_geo_knn_f32 / s6d_geo_indices_f32 / s6d_geo_embedding_points_* against a float64 restatement with direct differences, their
tie rule, the bit equality of the fused and the two-step form, batch invariance, the module against the CPU oracle and the absence
of any pair-sized temporary.  The bodies take `ops` so that tests/test_emu_geo_points.py runs them on the host build."""
import functools
import math

import pytest
import torch

from oracle import pem as opem

pytestmark = pytest.mark.gpu

SIGMA_D = 0.2
FACTOR_A = 180.0 / (15.0 * math.pi)
# what the kernels (and the fp32 reference statements) are given: the two scalars rounded to float32
SIGMA_D32 = torch.tensor(SIGMA_D, dtype=torch.float32).item()
FACTOR_A32 = torch.tensor(FACTOR_A, dtype=torch.float32).item()
# (2,197): the product's shape, workgroups of 64 pairs straddle anchor rows and the batch boundary; (1,37): less than one 64-pair row,
# B N N no multiple of 64; (3,65): N = 64 + 1, a lane's second candidate slot holds one point; (2,5): N barely above k + 1
SHAPES = [(2, 197), (1, 37), (3, 65), (2, 5)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from sam6d_amd import ops
    return ops


def _points(B, N):
    """The seeded cloud of a shape.  The seeds are chosen on the float64 restatement alone: 2 % of the anchors of the two small shapes
    is less than one anchor, so their clouds must hold no anchor whose 3rd and 4th neighbour are closer than 1e-4 (relative) -- with
    these seeds the smallest gap is 6.8e-4 at (1,37) and 1.8e-3 at (2,5), while (3,65) still leaves one anchor out (gap 5.4e-5)."""
    g = torch.Generator().manual_seed(3000 + 100 * B + N)
    pts = torch.randn(B, N, 3, generator=g) * 0.5
    pts[:, 0] = 100.0                                   # the background point of pose_estimation_model.py:27
    return pts


def _indices64(pts):
    """The stage in float64 on the float32 points, direct differences: d_idx (B,N,N), a_idx (B,N,N,3) with the neighbours nearest
    first (ties to the lower index: the sort is stable), knn (B,N,3), and the relative gap between the 3rd and 4th neighbour."""
    P = pts.double()
    B, N, _ = P.shape
    diff = P.unsqueeze(1) - P.unsqueeze(2)                                   # [b,n,m] = p_m - p_n
    dist = diff.norm(dim=-1)
    dd = dist.clone()
    dd[:, torch.arange(N), torch.arange(N)] = float("inf")                   # the anchor is excluded by its index
    ds, order = torch.sort(dd, dim=2, stable=True)
    knn = order[:, :, :3]
    gap = (ds[:, :, 3] - ds[:, :, 2]) / ds[:, :, 2].clamp(min=1e-300)
    ref = torch.gather(diff, 2, knn.unsqueeze(-1).expand(B, N, 3, 3)).unsqueeze(2).expand(B, N, N, 3, 3)
    anc = diff.unsqueeze(3).expand(B, N, N, 3, 3)
    a = torch.atan2(torch.linalg.cross(ref, anc, dim=-1).norm(dim=-1), (ref * anc).sum(-1)) * FACTOR_A32
    return dict(d=dist / SIGMA_D32, a=a, knn=knn, gap=gap)


@functools.lru_cache(maxsize=None)
def _case(B, N):
    """Points, their float64 indices and the fp32 CPU oracle's, computed once per shape and only read by the tests."""
    pts = _points(B, N)
    r = _indices64(pts)
    od, oa = opem.geo_indices(pts)
    oknn = (od * SIGMA_D).topk(k=4, dim=2, largest=False)[1][:, :, 1:]       # the very topk oracle.pem.geo_indices takes (same values)
    return dict(pts=pts, oracle_d=od, oracle_a=oa, oracle_knn=oknn, **r)


def _same_set(a, b):
    """(B,N,3) neighbour tables -> (B,N): the same three neighbours in any order."""
    return (a.sort(dim=-1)[0] == b.sort(dim=-1)[0]).all(-1)


def check_indices_vs_fp64(ops, B, N):
    """ops.geo_indices / ops.geo_knn against float64.

    d_idx: relative error <= 8 * 2^-24 off the diagonal (three roundings in the squared norm, the sqrt, the division, slack for the
    non-fused order); the diagonal exactly 0.  Neighbour sets equal the float64 sets on every anchor whose 3rd and 4th neighbour are
    more than 1e-4 apart (relative, float64); at most 2 % of the anchors of a case may be left out that way.  a_idx, the three
    angles of a pair sorted (the embedding takes a max over them): within 4 x the error the fp32 CPU oracle (oracle.pem.geo_indices)
    shows against the same float64 values on the same anchors -- the margin covers another atan2f and another contraction.
    Measured on the MI355X at (2,197) / (1,37) / (3,65) / (2,5): oracle error 1.2e-6 / 1.0e-6 / 1.1e-6 / 7.5e-7, ours 1.7e-6 / 1.6e-6 /
    1.7e-6 / 9.8e-7 (host build: 1.2e-6 / 7.5e-7 at the two small shapes); printed below on every run."""
    c = _case(B, N)
    pts = c["pts"].cuda()
    idx4 = ops.geo_indices(pts, SIGMA_D, FACTOR_A).cpu()
    knn = ops.geo_knn(pts).cpu().long()
    assert idx4.shape == (B, N, N, 4) and knn.shape == (B, N, 3)
    assert not torch.isnan(idx4).any()
    d, a = idx4[..., 0].double(), idx4[..., 1:].double()
    eye = torch.eye(N, dtype=torch.bool).expand(B, N, N)
    assert (d[eye] == 0).all(), "the diagonal of d_idx is exactly 0"
    rel = ((d - c["d"]).abs() / c["d"].clamp(min=1e-300))[~eye]
    print(f"[geo_points {B}x{N}] d_idx max relative error {rel.max().item():.3e} (bound {8 * 2.0 ** -24:.3e})")
    assert rel.max() <= 8 * 2.0 ** -24, rel.max().item()
    keep = c["gap"] >= 1e-4
    n_out = int((~keep).sum())
    print(f"[geo_points {B}x{N}] anchors left out for a 3rd/4th-neighbour gap < 1e-4: {n_out} of {B * N}")
    assert n_out <= 0.02 * B * N, n_out
    assert _same_set(knn, c["knn"])[keep].all(), "neighbour sets differ from float64 on an anchor with a clear gap"
    assert ((knn >= 0) & (knn < N)).all() and (knn != torch.arange(N).view(1, N, 1)).all()
    ref_sorted = c["a"].sort(dim=-1)[0]
    okeep = keep & _same_set(c["oracle_knn"], c["knn"])                     # the oracle's own error, where it has the same neighbours
    assert okeep.any()
    oerr = (c["oracle_a"].double().sort(dim=-1)[0] - ref_sorted).abs()[okeep].max().item()
    err = (a.sort(dim=-1)[0] - ref_sorted).abs()[keep].max().item()
    print(f"[geo_points {B}x{N}] a_idx max error vs float64: ours {err:.3e}, fp32 CPU oracle {oerr:.3e} (bound 4 x oracle = {4 * oerr:.3e})")
    assert err <= 4 * oerr, (err, oerr)


def _tie_points():
    """B = 2 clouds of N = 11: the nine points of a 3 x 3 integer grid (equal distances are exact in fp32) in two different index
    orders, plus two duplicates (index 9 repeats point 4, index 10 repeats point 0)."""
    grid = torch.tensor([[x, y, 0.0] for y in range(3) for x in range(3)])
    a = torch.cat([grid, grid[4:5], grid[0:1]])
    perm = torch.tensor([8, 3, 1, 6, 4, 0, 7, 2, 5])
    b = torch.cat([grid[perm] * 2.0 + 1.0, grid[perm][4:5] * 2.0 + 1.0, grid[perm][0:1] * 2.0 + 1.0])
    return torch.stack([a, b]).contiguous()


def check_ties_and_degenerate_points(ops):
    """Equal distances: the neighbours are the three smallest (squared distance, index) pairs over m != n, in that order -- computed
    here in exact integer arithmetic.  Duplicated points: no NaN, a_idx == 0 wherever anc == 0 (m == n or m a duplicate of n) or
    ref == 0 (the neighbour is a duplicate of the anchor)."""
    pts = _tie_points()
    B, N, _ = pts.shape
    ip = pts.long()
    d2 = ((ip.unsqueeze(1) - ip.unsqueeze(2)) ** 2).sum(-1)                  # exact
    key = d2 * N + torch.arange(N).view(1, 1, N)
    key[:, torch.arange(N), torch.arange(N)] = torch.iinfo(torch.int64).max
    want = key.sort(dim=2)[1][:, :, :3]
    knn = ops.geo_knn(pts.cuda()).cpu().long()
    assert torch.equal(knn, want), (knn, want)
    idx4 = ops.geo_indices(pts.cuda(), SIGMA_D, FACTOR_A).cpu()
    assert not torch.isnan(idx4).any() and not torch.isinf(idx4).any()
    d, a = idx4[..., 0], idx4[..., 1:]
    root = d2.double().sqrt().float()
    assert torch.equal(d, root / torch.full_like(root, SIGMA_D)), "integer distances: sqrt and the division are correctly rounded"
    anc0 = (d2 == 0).unsqueeze(-1).expand(B, N, N, 3)
    ref0 = (torch.gather(d2, 2, want) == 0).unsqueeze(2).expand(B, N, N, 3)
    assert anc0.any() and ref0.any()
    assert (a[anc0 | ref0] == 0).all()
    assert (a[~(anc0 | ref0)] >= 0).all() and (a <= 180.0 / 15.0 + 1e-5).all()


def _module(seed=4):
    from sam6d_amd.pem.layers import GeometricStructureEmbedding
    from sam6d_amd.pem.pose_estimation_model import default_cfg
    from sam6d_amd.utils import seeded
    return seeded.load_seeded(GeometricStructureEmbedding(default_cfg().geo_embedding).eval(), seed)


def _weights(geo):
    return (geo.proj_d.weight.contiguous(), geo.proj_d.bias, geo.proj_a.weight.contiguous(), geo.proj_a.bias, geo.embedding.div_term.contiguous())


def check_fused_equals_two_step(ops, B, N):
    """ops.geo_embedding_points(points) == ops.geo_embedding(ops.geo_indices(points)) bit for bit: f32, f16, pre-split weights in both
    storage types, and the pre-split form under s6d_set_geo_embed_form(2)."""
    geo = _module().cuda()
    w = _weights(geo)
    pts = _case(B, N)["pts"].cuda()
    idx4 = ops.geo_indices(pts, SIGMA_D, FACTOR_A)
    split = geo._split_weights()
    assert split is not None
    variants = [dict(), dict(out_dtype=torch.float16), dict(split=split), dict(out_dtype=torch.float16, split=split)]
    for kw in variants:
        two = ops.geo_embedding(idx4, *w, **kw)
        one = ops.geo_embedding_points(pts, SIGMA_D, FACTOR_A, *w, **kw)
        assert one.dtype == two.dtype and one.shape == (B, N, N, 256)
        assert torch.equal(one.cpu(), two.cpu()), kw
    try:
        ops.set_geo_embed_form(2)
        for kw in variants[2:]:
            assert torch.equal(ops.geo_embedding_points(pts, SIGMA_D, FACTOR_A, *w, **kw).cpu(), ops.geo_embedding(idx4, *w, **kw).cpu()), kw
    finally:
        ops.set_geo_embed_form(1)


def check_batch_invariance(ops, B, N):
    """An instance alone gives the bits it gives inside the batch: indices and the points-fed embedding."""
    geo = _module().cuda()
    w = _weights(geo)
    pts = _case(B, N)["pts"].cuda()
    idx4 = ops.geo_indices(pts, SIGMA_D, FACTOR_A).cpu()
    emb = ops.geo_embedding_points(pts, SIGMA_D, FACTOR_A, *w, split=geo._split_weights()).cpu()
    for b in range(B):
        one = pts[b:b + 1].contiguous()
        assert torch.equal(ops.geo_indices(one, SIGMA_D, FACTOR_A).cpu()[0], idx4[b])
        assert torch.equal(ops.geo_embedding_points(one, SIGMA_D, FACTOR_A, *w, split=geo._split_weights()).cpu()[0], emb[b])


def check_module_vs_oracle(ops, B, N):
    """GeometricStructureEmbedding on the device (from the points, strict: a fall-back to library statements is an error) against
    oracle.pem.geo_embedding with the bounds of tests/test_gpu_pose.py::test_geo_embedding_vs_oracle; the whole diagonal is masked:
    there the oracle's expanded square leaves ~1e-3 where the direct form gives 0."""
    from sam6d_amd import policy
    m = _module(2)
    W = {"geo_embedding." + k: v for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(N)
    pts = torch.randn(B, N, 3, generator=g) * 0.5
    pts[:, 0] = 100.0
    with torch.no_grad(), policy.use(strict="1", geo_from_points="1"):
        ref = opem.geo_embedding(W, pts)
        assert ops.have("geo_embedding_points") and ops.have("geo_indices")
        out = m.cuda()(pts.cuda()).cpu()
    mask = ~torch.eye(N, dtype=torch.bool).expand(B, N, N)
    err = (out - ref).abs()[mask]
    print(f"[geo_points {B}x{N}] module vs oracle: max {err.max().item():.3e} mean {err.mean().item():.3e}")
    assert err.max() < 2e-3 and err.mean() < 2e-5, (err.max().item(), err.mean().item())


def check_bad_arguments(ops):
    """N above the served range and a null pointer: S6D_EINVAL, and nothing is launched (the output keeps its fill)."""
    pts = _points(1, 257).cuda()
    out = torch.full((1, 257, 257, 4), -7.0).cuda()
    knn = torch.full((1, 257, 3), -7, dtype=torch.int32).cuda()
    emb = torch.full((1, 8, 8, 256), -7.0).cuda()
    geo = _module().cuda()
    wd, bd, wa, ba, div = _weights(geo)
    P = lambda t: t.data_ptr()
    s = ops._stream()
    f_idx, f_knn, f_emb = ops._fn("s6d_geo_indices_f32", 7), ops._fn("s6d_geo_knn_f32", 5), ops._fn("s6d_geo_embedding_points_f32", 15)
    assert f_idx(P(pts), 1, 257, SIGMA_D, FACTOR_A, P(out), s) == -1
    assert f_knn(P(pts), 1, 257, P(knn), s) == -1
    assert f_idx(P(pts), 1, 3, SIGMA_D, FACTOR_A, P(out), s) == -1                  # fewer than three other points
    assert f_idx(None, 1, 8, SIGMA_D, FACTOR_A, P(out), s) == -1
    assert f_idx(P(pts), 1, 8, SIGMA_D, FACTOR_A, None, s) == -1
    assert f_knn(P(pts), 1, 8, None, s) == -1
    tail = (P(wd), P(bd), P(wa), P(ba), P(div), 256, 3, P(emb), s)
    assert f_emb(P(pts), 1, 257, SIGMA_D, FACTOR_A, P(knn), *tail) == -1
    assert f_emb(P(pts), 1, 8, SIGMA_D, FACTOR_A, None, *tail) == -1                # no neighbour scratch
    assert f_emb(None, 1, 8, SIGMA_D, FACTOR_A, P(knn), *tail) == -1
    assert f_emb(P(pts), 1, 8, SIGMA_D, FACTOR_A, P(knn), P(wd), P(bd), P(wa), P(ba), P(div), 256, 3, None, s) == -1
    assert f_idx(P(pts), 0, 8, SIGMA_D, FACTOR_A, None, s) == 0                     # nothing to do
    torch.cuda.synchronize()
    assert (out.cpu() == -7).all() and (knn.cpu() == -7).all() and (emb.cpu() == -7).all()
    with pytest.raises(RuntimeError, match="s6d_geo_indices_f32"):
        ops.geo_indices(pts, SIGMA_D, FACTOR_A)


# ---------------------------------------------------------------------------------------------------------------- on the MI355X
@pytest.mark.parametrize("B,N", SHAPES)
def test_indices_vs_fp64(ops, B, N):
    check_indices_vs_fp64(ops, B, N)


def test_ties_and_degenerate_points(ops):
    check_ties_and_degenerate_points(ops)


@pytest.mark.parametrize("B,N", SHAPES)
def test_fused_equals_two_step(ops, B, N):
    check_fused_equals_two_step(ops, B, N)


def test_batch_invariance(ops):
    check_batch_invariance(ops, 3, 197)


@pytest.mark.parametrize("B,N", [(2, 197), (1, 37)])
def test_module_vs_oracle(ops, B, N):
    check_module_vs_oracle(ops, B, N)


def test_no_pair_sized_temporary(ops):
    """The module's forward allocates the embedding and O(B N) scratch, nothing of the size of the pairs: the peak rises over the
    level before the call by at most out.nbytes + 64 B N + 8192 bytes (the idx4 tensor alone is 16 B N N).  Counted in the bytes the
    forward ASKS the allocator for (requested_bytes): the caching allocator hands a 79-MB output a block rounded up to 2 MiB
    (211 KB more than out.nbytes, measured), which is no temporary."""
    from sam6d_amd import policy
    B, N = 2, 197
    m = _module(2).cuda()
    pts = _case(B, N)["pts"].cuda()
    with torch.no_grad(), policy.use(strict="1", geo_from_points="1"):
        out = m(pts)                                                            # warm-up: the split weights are cached now
        del out
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_stats()["requested_bytes.all.current"]
        before_blocks = torch.cuda.memory_allocated()
        out = m(pts)
        torch.cuda.synchronize()
        rise = torch.cuda.memory_stats()["requested_bytes.all.peak"] - before
        rise_blocks = torch.cuda.max_memory_allocated() - before_blocks
    nbytes = out.numel() * out.element_size()
    print(f"[geo_points {B}x{N}] peak rise {rise} bytes requested ({rise_blocks} in allocator blocks, max_memory_allocated), out {nbytes} "
          f"bytes, allowance {nbytes + 64 * B * N + 8192}")
    assert out.shape == (B, N, N, 256)
    assert rise <= nbytes + 64 * B * N + 8192, (rise, nbytes)


def test_bad_arguments(ops):
    check_bad_arguments(ops)
