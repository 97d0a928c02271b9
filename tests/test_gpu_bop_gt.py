"""The BOP ground-truth kernels (csrc/s6d_bopgt.hip) and sam6d_amd.groundtruth on top of them against the numpy restatement of
tests/bopgt_ref.py: masks, visible masks, counts and extents EQUAL to its float32 mode; against its float64 mode the visible mask
may differ only on the undecided pixels, which are at most 2 % of the mask area (a condition on the inputs, asserted on the
restatement before any kernel output is looked at); an instance alone has the bits it has in the batch, two chunkings agree,
visib <= mask and in-image <= all; known answers; the diameter bit for bit and within its derived bound; the argument checks.
bop_toolkit is not present; nothing here is compared with it.  The bodies take `ops` so that tests/test_emu_bop_gt.py runs them
on the host build.

Bounds, with u = 2^-24:
  visibility  a pixel is undecided when Dg - Dt lies within 8 u (|Dg| + |Dt|) of delta (tests/test_gpu_bop_eval.py derives it for
              the same statement).
  diameter    |d32 - d64| <= 4 u d64.  Per pair, on the same float32 vertices: dx = fl(xi - xj) carries (1 + e), |e| <= u; the
              product fl(dx dx) carries (1 + e)^3: 3 u; the three products are non-negative, so a sum's relative error is at most
              the larger of its terms' plus its own rounding: fl(dx dx + dy dy) 4 u, fl(.. + dz dz) 5 u.  Three products and two
              sums: d2 within 5 u.  The maximum of values within 5 u is within 5 u of the maximum; the square root halves that
              (2.5 u) and rounds once more: 3.5 u, second-order terms included below 4 u."""
import numpy as np
import pytest
import torch

from tests import bopgt_ref as G
from tests import render_ref as R
from tests import test_gpu_bop_eval as TB
from tests import util

pytestmark = pytest.mark.gpu

ZNEAR = 1.0
DELTA = 15.0
SIZES = dict(TB.SIZES)
SIZES[(5, 7)] = (60.0, 60.0, 3.0, 2.0)
MARGINS = ("none", "image", "small")
DIAMETER_V = (1, 2, 255, 256, 257, 513, 1000)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from sam6d_amd import ops
    return ops


_t, _np = TB._t, TB._np


def margin_of(hw, kind):
    return dict(none=(0, 0), image=(hw[1], hw[0]), small=(3, 2))[kind]


def _mesh(name):
    return R.cube(40.0)[:2] if name == "cube" else R.torus(24, 24)[:2]


def instance_poses(hw, cam, N):
    """N poses at about 400 units (an object of 12 - 25 pixels): instance 0 fully inside the image (of the larger sizes), 1 across
    the left border, 2 wholly left of the image but inside a canvas with the default margin, 3 across the bottom border and nearer,
    4 inside and farther."""
    h, w = hw
    P = R.poses(5, seed=7, t=(0.0, 0.0, 400.0)).astype(np.float64)
    fx, fy, cx, cy = cam

    def at(u, v, z):
        return ((u - cx) / fx * z, (v - cy) / fy * z, z)
    where = [at(w / 2 + 0.25, h / 2 - 0.25, 400.0), at(0.0, h / 2, 400.0), at(-w / 2, h / 2, 400.0), at(w / 2, h - 1.0, 380.0),
             at(w / 2 - 2, h / 2 + 1, 424.0)]
    for n in range(5):
        P[n, :3, 3] = np.round(np.array(where[n]) * 16) / 16
    return P[:N].astype(np.float32)


def canvases(ops, v, f, poses, cams, hw, margin):
    """One ``render_depth`` call at the canvas size with cx + mx, cy + my (float32)."""
    mx, my = margin
    shifted = (np.asarray(cams, np.float32) + np.array([0, 0, mx, my], np.float32)).astype(np.float32)
    out = ops.render_depth(_t(v), _t(f), _t(np.asarray(poses, np.float32)), _t(shifted), hw[0] + 2 * my, hw[1] + 2 * mx, ZNEAR)
    torch.cuda.synchronize()
    return _np(out["depth"]), _np(out["skipped"])


def scene(ops, hw, kind, N, M, name="cube"):
    """Canvases of N instances and M measured depth images: the surface of instance m with a few units of noise, a wall behind, a
    rendered occluder (a cube nearer to the camera, over a part of the image) in front, 10 % missing."""
    h, w = hw
    margin = margin_of(hw, kind)
    cam = np.array(SIZES[hw], np.float32)
    v, f = _mesh(name)
    cams = np.tile(cam, (N, 1))
    canvas, skipped = canvases(ops, v, f, instance_poses(hw, cam, N), cams, hw, margin)
    assert skipped.sum() == 0
    rs = np.random.RandomState(1000 * h + 100 * N + 10 * M + len(kind))
    ov, of = R.cube(30.0)[:2]
    occ_pose = R.poses(M, seed=5, t=(0.0, 0.0, 300.0)).astype(np.float64)
    for m in range(M):
        occ_pose[m, :3, 3] = ((w / 2 + 4 - cam[2]) / cam[0] * 300.0 + 8 * m, (h / 2 + 3 - cam[3]) / cam[1] * 300.0, 300.0)
    occ, _ = canvases(ops, ov, of, occ_pose, np.tile(cam, (M, 1)), hw, (0, 0))
    mx, my = margin
    test = np.full((M, h, w), 460.0, np.float32)
    for m in range(M):
        surf = canvas[m % N, my:my + h, mx:mx + w]
        test[m] = np.where(surf > 0, surf + rs.uniform(-3, 3, (h, w)).astype(np.float32), test[m])
        if h > 1:
            test[m] = np.where(occ[m] > 0, occ[m], test[m])
            test[m][rs.uniform(size=(h, w)) < 0.1] = 0.0
    ti = (np.arange(N) % M).astype(np.int32)
    return canvas, test, ti, cams, margin


def visibility(ops, canvas, test, ti, cams, delta, margin):
    out = ops.gt_visibility(_t(canvas), _t(test), _t(ti), _t(cams), delta, margin)
    torch.cuda.synchronize()
    return {k: _np(x) for k, x in out.items()}


def same(got, ref):
    return all(np.array_equal(got[k].astype(np.int64), ref[k].astype(np.int64)) for k in ("mask", "mask_visib", "counts", "extents"))


def check_visibility(ops, hw, kind, N, M, name="cube"):
    canvas, test, ti, cams, margin = scene(ops, hw, kind, N, M, name)
    r32 = G.gt_visibility(canvas, test, ti, cams, DELTA, margin, np.float32)
    r64 = G.gt_visibility(canvas, test, ti, cams, DELTA, margin, np.float64)
    und = r64["undecided"].sum((1, 2))
    assert (und <= 0.02 * r64["counts"][:, 1]).all(), (und, r64["counts"][:, 1])          # the inputs, before the kernel is looked at
    if hw[0] >= 37:
        assert r64["counts"][0, 1] > 40 and 0 < r64["counts"][0, 3] < r64["counts"][0, 1]          # partly occluded
        if N > 1:
            assert 0 < r64["counts"][1, 1] < r64["counts"][1, 0] or kind != "image"       # across the border
        if N > 2 and kind == "image":
            assert r64["counts"][2, 0] > 40 and r64["counts"][2, 1] == 0                  # outside the image, on the canvas
    got = visibility(ops, canvas, test, ti, cams, DELTA, margin)
    print(f"[bop gt {hw} margin {margin} N {N} M {M} {name}] counts {got['counts'].tolist()} undecided {und.tolist()}")
    assert same(got, r32), (got["counts"], r32["counts"], got["extents"], r32["extents"])
    differs = got["mask_visib"].astype(bool) != r64["mask_visib"].astype(bool)
    assert not (differs & ~r64["undecided"]).any() and np.array_equal(got["mask"], r64["mask"])
    util.record_margin(f"bop_gt_visibility_{hw[0]}x{hw[1]}_{kind}_N{N}_M{M}_{name}",
                       undecided_fraction=float((und / np.maximum(r64["counts"][:, 1], 1)).max()), bound_ratio=0.02)
    # visib <= mask, in-image <= all, valid and visib <= in-image
    assert not (got["mask_visib"] & ~got["mask"]).any()
    c = got["counts"]
    assert (c[:, 1] <= c[:, 0]).all() and (c[:, 2] <= c[:, 1]).all() and (c[:, 3] <= c[:, 1]).all()
    assert np.array_equal(c[:, 1], got["mask"].sum((1, 2))) and np.array_equal(c[:, 3], got["mask_visib"].sum((1, 2)))
    # an instance alone has the bits it has in the batch; two chunkings give equal results
    n = N - 2 if N > 1 else 0
    alone = visibility(ops, canvas[n:n + 1], test, ti[n:n + 1], cams[n:n + 1], DELTA, margin)
    assert all(np.array_equal(alone[k][0], got[k][n]) for k in got)
    if N > 2:
        a, b = (visibility(ops, canvas[s], test, ti[s], cams[s], DELTA, margin) for s in (slice(0, 2), slice(2, N)))
        assert all(np.array_equal(np.concatenate([a[k], b[k]]), got[k]) for k in got)


def check_visibility_known_answers(ops):
    h, w = 48, 64
    cam = np.array([[60.0, 60.0, 32.0, 24.0]], np.float32)
    one = np.zeros(1, np.int32)
    square = np.zeros((1, h, w), np.float32)
    square[0, 10:30, 20:40] = 400.0                                        # 20 x 20 pixels, fronto-parallel
    # half covered by a nearer plane, the rest in front of a farther one
    test = np.full((1, h, w), 500.0, np.float32)
    test[0, :, :30] = 300.0
    got = visibility(ops, square, test, one, cam, DELTA, (0, 0))
    assert got["counts"].tolist() == [[400, 400, 400, 200]]
    assert got["extents"].tolist() == [[[20, 10, 39, 29], [30, 10, 39, 29]]]
    right = np.zeros((h, w), bool)
    right[10:30, 30:40] = True
    assert np.array_equal(got["mask"][0], square[0] > 0) and np.array_equal(got["mask_visib"][0].astype(bool), right)
    # nothing measured: all visible, none valid
    got = visibility(ops, square, np.zeros_like(test), one, cam, DELTA, (0, 0))
    assert got["counts"].tolist() == [[400, 400, 0, 400]] and np.array_equal(got["mask_visib"], got["mask"])
    assert got["extents"].tolist() == [[[20, 10, 39, 29], [20, 10, 39, 29]]]
    # an empty canvas: empty extents
    got = visibility(ops, np.zeros_like(square), test, one, cam, DELTA, (0, 0))
    assert got["counts"].tolist() == [[0, 0, 0, 0]] and got["extents"].tolist() == [[list(G.EMPTY), list(G.EMPTY)]]
    assert not got["mask"].any() and not got["mask_visib"].any()
    # Dg - Dt exactly delta, at the principal point (r = 1): visible; one float32 step nearer: hidden
    dot = np.zeros((1, h, w), np.float32)
    dot[0, 24, 32] = 400.0
    test = np.full((1, h, w), 385.0, np.float32)
    assert visibility(ops, dot, test, one, cam, DELTA, (0, 0))["counts"].tolist() == [[1, 1, 1, 1]]
    test[0, 24, 32] = np.nextafter(np.float32(385.0), np.float32(0.0))
    assert np.float32(400.0) - test[0, 24, 32] > np.float32(DELTA)
    assert visibility(ops, dot, test, one, cam, DELTA, (0, 0))["counts"].tolist() == [[1, 1, 1, 0]]
    # the square three columns across the left border, on a canvas with a margin of (5, 4)
    mx, my = 5, 4
    canvas = np.zeros((1, h + 2 * my, w + 2 * mx), np.float32)
    canvas[0, my + 10:my + 30, mx - 3:mx + 17] = 400.0
    got = visibility(ops, canvas, np.zeros_like(test), one, cam, DELTA, (mx, my))
    assert got["extents"].tolist() == [[[-3, 10, 16, 29], [0, 10, 16, 29]]]
    assert got["counts"].tolist() == [[400, 340, 0, 340]] and got["counts"][0, 0] - got["counts"][0, 1] == 3 * 20
    # and wholly above the image
    canvas[:] = 0
    canvas[0, 0:3, mx + 2:mx + 6] = 400.0
    got = visibility(ops, canvas, np.zeros_like(test), one, cam, DELTA, (mx, my))
    assert got["counts"].tolist() == [[12, 0, 0, 0]] and got["extents"].tolist() == [[[2, -4, 5, -2], list(G.EMPTY)]]


def _bits(a):
    return np.asarray(a, np.float32).reshape(-1).view(np.uint32)


def _vertices(V):
    return np.random.RandomState(V).uniform(-60, 60, (V, 3)).astype(np.float32)


def diameter(ops, v):
    d = ops.model_diameter(_t(v))
    torch.cuda.synchronize()
    return _np(d)


def check_diameter(ops, V):
    """Bit for bit the float32 restatement, within 4 u of the float64 one (the docstring of this file); duplicates and a
    permutation change nothing."""
    v = _vertices(V)
    r32, r64 = G.diameter(v, np.float32), G.diameter(v, np.float64)
    got = diameter(ops, v)
    assert _bits(got)[0] == _bits(r32)[0], (got, r32)
    err = abs(float(got[0]) - r64) / (4 * G.U * r64) if r64 > 0 else float(got[0] != 0)
    print(f"[bop gt diameter V {V}] {float(got[0])!r}, error over the bound {err:.3f}")
    assert err <= 1.0 and (V > 1 or got[0] == 0)
    util.record_margin(f"bop_gt_diameter_V{V}", diameter_err_over_bound=err, bound_ratio=1.0)
    rs = np.random.RandomState(V + 1)
    assert _bits(diameter(ops, v[rs.permutation(V)]))[0] == _bits(got)[0]
    dup = np.concatenate([v, v[rs.randint(0, V, 7)], v[-1:]])
    assert _bits(diameter(ops, dup))[0] == _bits(got)[0]


def check_diameter_hostile(ops):
    """The extreme pair in the last, partial tile; fewer persistent workgroups than steps; a NaN vertex: +inf, and ValueError from
    ``model_info``."""
    from sam6d_amd import _lib, groundtruth
    v = _vertices(1000)
    v[997], v[999] = (-500.0, 3.0, 2.0), (700.0, -1.0, 0.5)
    want = G.diameter(v, np.float32)
    assert abs(float(want) - 1200.0) < 0.1
    got = diameter(ops, v)
    assert _bits(got)[0] == _bits(want)[0]
    assert _lib.lib().s6d_set_persistent_grid_limit(3) == 0                # 16 steps on 3 workgroups
    try:
        assert _bits(diameter(ops, v))[0] == _bits(want)[0]
    finally:
        _lib.lib().s6d_set_persistent_grid_limit(0)
    info = groundtruth.model_info(_t(v))
    assert info["diameter"] == float(want) and info["min_x"] == -500.0 and info["size_x"] == 1200.0
    assert info["min_y"] == float(v[:, 1].min()) and info["size_z"] == float(v[:, 2].max().astype(np.float64) - v[:, 2].min().astype(np.float64))
    for k in (0, 600, 999):
        bad = v.copy()
        bad[k, 1] = np.nan
        assert np.isposinf(diameter(ops, bad)[0]) and np.isposinf(G.diameter(bad, np.float32))
        with pytest.raises(ValueError, match="not finite"):
            groundtruth.model_info(_t(bad))
    bad = v.copy()
    bad[5, 0] = np.inf
    assert np.isposinf(diameter(ops, bad)[0])


def check_arguments(ops):
    """Wrong shapes and dtypes, a test_index out of range and negative margins are refused on the host; the entry points refuse
    bad sizes with -1 / -3 before any launch."""
    canvas, test, ti, cams, margin = scene(ops, (37, 53), "small", 3, 2)
    a = [_t(x) for x in (canvas, test, ti, cams)]
    call = lambda *x, m=margin: ops.gt_visibility(*x, DELTA, m)          # noqa: E731
    with pytest.raises(RuntimeError, match="float"):
        call(a[0].double(), *a[1:])
    with pytest.raises(RuntimeError, match="float"):
        call(a[0], a[1].double(), *a[2:])
    with pytest.raises(RuntimeError, match="an int tensor"):
        call(a[0], a[1], a[2].long(), a[3])
    with pytest.raises(ValueError, match="expected"):
        call(*a, m=(0, 0))                                                 # the canvas does not have the size of the margin
    with pytest.raises(ValueError, match="expected"):
        call(a[0][:2].contiguous(), *a[1:])
    with pytest.raises(ValueError, match="expected"):
        call(*a[:3], a[3][:, :3].contiguous())
    with pytest.raises(ValueError, match="margin must be >= 0"):
        call(*a, m=(-1, 2))
    for bad_index in (2, -1):
        oob = a[2].clone()
        oob[1] = bad_index
        with pytest.raises(ValueError, match=r"test_index must lie in \[0, 2\)"):
            call(a[0], a[1], oob, a[3])
    with pytest.raises(RuntimeError, match="float"):
        ops.model_diameter(_t(_vertices(9)).double())
    with pytest.raises(ValueError, match="expected"):
        ops.model_diameter(_t(_vertices(9))[:, :2].contiguous())
    with pytest.raises(ValueError, match="expected"):
        ops.model_diameter(_t(_vertices(9))[:0].contiguous())
    fn = ops._fn("s6d_gt_visibility_f32", 16)
    P = lambda t: t.data_ptr()                                             # noqa: E731
    out8, out32 = torch.full((3, 37, 53), 7, dtype=torch.uint8).cuda(), torch.full((3, 8), 7, dtype=torch.int32).cuda()
    args = lambda N, M, H, W, mx, my: (P(a[0]), P(a[1]), P(a[2]), P(a[3]), N, M, H, W, mx, my, DELTA, P(out8), P(out8), P(out32), P(out32),   # noqa: E731
                                       ops._stream())
    assert fn(*args(3, 2, 37, 53, -1, 2)) == -1 and fn(*args(3, 2, 37, 53, 3, -2)) == -1
    assert fn(*args(3, 0, 37, 53, 3, 2)) == -1 and fn(*args(3, 2, 0, 53, 3, 2)) == -1 and fn(*args(-1, 2, 37, 53, 3, 2)) == -1
    assert fn(*args(3, 2, 46341, 46341, 0, 0)) == -3                       # a canvas of 2^31 pixels or more
    assert fn(*args(3, 2, 37, 53, 2 ** 30, 2)) == -3
    assert fn(P(a[0]), P(a[1]), P(a[2]), P(a[3]), 3, 2, 37, 53, 3, 2, float("nan"), P(out8), P(out8), P(out32), P(out32), ops._stream()) == -1
    assert fn(None, P(a[1]), P(a[2]), P(a[3]), 3, 2, 37, 53, 3, 2, DELTA, P(out8), P(out8), P(out32), P(out32), ops._stream()) == -1
    assert fn(*args(0, 2, 37, 53, 3, 2)) == 0
    fd = ops._fn("s6d_model_diameter_f32", 4)
    assert fd(P(a[0]), 0, P(out32), ops._stream()) == -1 and fd(None, 5, P(out32), ops._stream()) == -1
    torch.cuda.synchronize()
    assert (out8.cpu() == 7).all() and (out32.cpu() == 7).all()


def dataset(hw=(48, 64)):
    """Two models, five instances in two images -> (models, gt, images) in the layout of ``tools/bop_eval.load_dataset``."""
    cam = np.array(SIZES[hw], np.float32)
    models = {}
    for obj, name in ((1, "cube"), (2, "torus")):
        v, f = _mesh(name)
        models[obj] = dict(vertices=v, faces=f)
    P = instance_poses(hw, cam, 5).astype(np.float64)
    P[4, :3, 3] *= 560.0 / P[4, 2, 3]                                      # the same pixel, behind the torus of instance 0
    gt = dict(im=np.array([0, 1, 0, 1, 0]), obj=np.array([2, 1, 1, 2, 1]), pose=P)
    rs = np.random.RandomState(3)
    depth = np.full((2,) + hw, 460.0, np.float32)
    depth[0, 20:34, 34:50] = 300.0
    depth[1, 30:, :] = 350.0
    depth[rs.uniform(size=depth.shape) < 0.1] = 0.0
    cams = np.stack([cam, cam + np.array([2.0, -1.0, 0.5, -0.5], np.float32)]).astype(np.float32)
    return models, gt, dict(cams=cams, depth=depth)


def restate(ops, models, gt, images, margin, depth="measured"):
    """The result ``instance_ground_truth`` must give, from one canvas per instance and the restatement."""
    hw = images["depth"].shape[1:]
    G_ = len(gt["im"])
    canvas = np.zeros((G_, hw[0] + 2 * margin[1], hw[1] + 2 * margin[0]), np.float32)
    skipped = np.zeros(G_, np.int64)
    for g in range(G_):
        m = models[int(gt["obj"][g])]
        c, s = canvases(ops, m["vertices"], m["faces"], gt["pose"][g:g + 1], images["cams"][gt["im"][g]][None], hw, margin)
        canvas[g], skipped[g] = c[0], s[0]
    test = images["depth"]
    if depth == "rendered":
        test = np.zeros_like(images["depth"])
        win = canvas[:, margin[1]:margin[1] + hw[0], margin[0]:margin[0] + hw[1]]
        for i in range(len(test)):
            z = np.where(win[gt["im"] == i] > 0, win[gt["im"] == i], np.inf).min(0)
            test[i] = np.where(np.isfinite(z), z, 0)
    ref = G.gt_visibility(canvas, test, gt["im"].astype(np.int32), images["cams"][gt["im"]], DELTA, margin, np.float32)
    ref["skipped"] = skipped
    return ref


def matches(result, ref):
    c, empty = ref["counts"], ref["counts"][:, [0, 3]] == 0
    return (np.array_equal(_np(result["mask"]), ref["mask"]) and np.array_equal(_np(result["mask_visib"]), ref["mask_visib"])
            and np.array_equal(result["px_count_all"], c[:, 0]) and np.array_equal(result["px_count_in_image"], c[:, 1])
            and np.array_equal(result["px_count_valid"], c[:, 2]) and np.array_equal(result["px_count_visib"], c[:, 3])
            and np.array_equal(result["extents_obj"], np.where(empty[:, :1], -1, ref["extents"][:, 0]))
            and np.array_equal(result["extents_visib"], np.where(empty[:, 1:], -1, ref["extents"][:, 1]))
            and np.array_equal(result["visib_fract"], G.visib_fract(c)) and np.array_equal(result["skipped"], ref["skipped"]))


def check_modules(ops, monkeypatch):
    """groundtruth.instance_ground_truth under strict mode takes no library branch and gives the restatement's result, whatever
    the chunking and the mask format; rendered depth; the records."""
    from sam6d_amd import groundtruth, policy
    models, gt, images = dataset()
    dev = _t(np.zeros(1, np.float32)).device                               # the host under the emulator fixture
    for margin in (None, (0, 0)):
        m = (64, 48) if margin is None else margin
        ref = restate(ops, models, gt, images, m)
        with policy.use(strict="1"):
            whole = groundtruth.instance_ground_truth(models, gt, images, margin=margin, device=dev)
            single = groundtruth.instance_ground_truth(models, gt, images, margin=margin, device=dev, chunk_bytes=1)
            rle = groundtruth.instance_ground_truth(models, gt, images, margin=margin, device=dev, chunk_bytes=3 * (4 * 9 + 2) * 48 * 64, masks="rle")
        assert not policy.library_branch_hits()
        assert matches(whole, ref) and matches(single, ref)
        rle = dict(rle, mask=rle["mask"].to_dense().to(torch.uint8), mask_visib=rle["mask_visib"].to_dense().to(torch.uint8))
        assert matches(rle, ref)
    assert ref["counts"][2, 0] == 0 and whole["extents_obj"][2].tolist() == [-1, -1, -1, -1]          # off the image, no margin
    ref = restate(ops, models, gt, images, (64, 48))
    assert (ref["counts"][:, 3] < ref["counts"][:, 1]).any() and ref["counts"][2, 0] > 0 and ref["counts"][2, 1] == 0
    recs = groundtruth.gt_info_records(groundtruth.instance_ground_truth(models, gt, images, device=dev))
    assert [r["px_count_all"] for r in recs] == ref["counts"][:, 0].tolist() and recs[2]["bbox_visib"] == [-1, -1, -1, -1]
    assert recs[2]["bbox_obj"][0] < 0 and recs[2]["visib_fract"] == 0.0
    # rendered depth: mutual occlusion only
    ref = restate(ops, models, gt, images, (64, 48), depth="rendered")
    with policy.use(strict="1"):
        got = groundtruth.instance_ground_truth(models, gt, dict(cams=images["cams"], size=(48, 64)), depth="rendered", device=dev, chunk_bytes=1)
    assert matches(got, ref) and np.array_equal(got["px_count_valid"], got["px_count_in_image"])
    assert got["px_count_visib"][4] < got["px_count_in_image"][4] and got["px_count_visib"][0] == got["px_count_in_image"][0]
    # an object that reaches behind znear is reported
    close = dict(gt, pose=gt["pose"].copy())
    close["pose"][0, :3, 3] = (0.0, 0.0, 30.0)
    got = groundtruth.instance_ground_truth(models, close, images, margin=(0, 0), device=dev)
    assert got["skipped"][0] > 0 and (got["skipped"][1:] == 0).all()
    # bop_eval = 0: the torch statements (the ops are made to raise)
    def boom(*a, **k):
        raise AssertionError("the kernel path ran although bop_eval = 0")
    monkeypatch.setenv("S6D_BOP_EVAL", "0")
    for name in ("gt_visibility", "model_diameter"):
        monkeypatch.setattr(ops, name, boom)
    v = _vertices(513)
    assert groundtruth.model_info(_t(v))["diameter"] == float(G.diameter(v, np.float32))


# ---------------------------------------------------------------------------------------------------------------- on the MI355X
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N", [1, 3, 5])
@pytest.mark.parametrize("kind", MARGINS)
@pytest.mark.parametrize("hw", sorted(SIZES))
def test_visibility_vs_restatement(ops, hw, kind, N, M):
    check_visibility(ops, hw, kind, N, M)


def test_visibility_torus(ops):
    check_visibility(ops, (48, 64), "image", 3, 2, "torus")


def test_visibility_known_answers(ops):
    check_visibility_known_answers(ops)


@pytest.mark.parametrize("V", DIAMETER_V)
def test_diameter_vs_restatement(ops, V):
    check_diameter(ops, V)


def test_diameter_hostile_inputs(ops):
    check_diameter_hostile(ops)


def test_arguments(ops):
    check_arguments(ops)


def test_modules(ops, monkeypatch):
    check_modules(ops, monkeypatch)
