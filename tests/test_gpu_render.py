"""ops.render_views / render.render_templates (s6d_raster_views_f32, csrc/s6d_raster.hip) against the numpy restatement of
tests/render_ref.py: coverage and the visible face exactly, xyz and depth within bounds derived from the kernel's roundings
(profiles/render_margins.md), the colour within one level; the fill rule, hostile geometry, both work shapes on either side of
their threshold, determinism and the argument checks.  The bodies take `ops` so that tests/test_emu_render.py runs them on the
host build.

48 x 64 views, fx = fy = 60, c = (32, 24), objects about 400 units in front of the camera.  Bounds, with u = 2^-24 (derivation in
profiles/render_margins.md; none of them was chosen by looking at the kernel's output):
  depth   |Z - Z64| <= 8 u Z64
  xyz     |a - a64| <= 16 u sum_k b_k |a_k|   (b the perspective-correct barycentrics, a_k the vertex coordinate: ``xyz_scale``)
  face    exact, under the precondition -- asserted on the restatement alone -- that at every covered pixel the two nearest
          layers are at least 16 x (8 u) = 7.6e-6 apart, relatively
  rgb     within one level of the rounded float64 value"""
import functools

import numpy as np
import pytest
import torch

from tests import render_ref as R
from tests import util

pytestmark = pytest.mark.gpu

H, W = 48, 64
K = (60.0, 60.0, 32.0, 24.0)
KM = np.array([[60.0, 0.0, 32.0], [0.0, 60.0, 24.0], [0.0, 0.0, 1.0]])
AMBIENT, DIFFUSE, ZNEAR = 0.3, 0.7, 1.0
U = 2.0 ** -24
DEPTH_BOUND, XYZ_BOUND, MIN_GAP = 8 * U, 16 * U, 16 * 8 * U
EYE = np.eye(4, dtype=np.float32)[None]
OUT = ("rgb", "mask", "xyz", "depth", "face", "skipped")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from sam6d_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _mesh(name):
    """(vertices, faces, colors, poses) of a main mesh and its restatement, computed once and only read."""
    v, f, c = R.torus() if name == "torus" else R.cube()
    P = {"torus": lambda: R.poses(3, seed=11), "cube": lambda: R.poses(3, seed=1), "cube-near": lambda: R.poses(3, seed=3, t=(3.0, -2.0, 220.0))}[name]()
    return v, f, c, P, R.render(v, f, c, P, K, H, W, AMBIENT, DIFFUSE, ZNEAR)


def _render(ops, v, f, c, P, znear=ZNEAR):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    out = ops.render_views(t(v), t(f), t(c), t(P), *K, H, W, AMBIENT, DIFFUSE, znear)
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in OUT}


def _grey(v):
    return np.full((len(v), 3), 200, np.uint8)


def _at(px, py, z=60.0):
    """The vertex that projects to pixel (px, py) at depth z under the identity pose (exactly, for the small integers used here)."""
    return [(px - K[2]) * z / K[0], (py - K[3]) * z / K[1], z]


def _compare(got, ref, tag):
    """mask and face exactly, no pixel left out; depth, xyz within the derived bounds; rgb within a level.  -> worst fractions."""
    assert np.array_equal(got["mask"], ref["mask"]), tag
    assert np.array_equal(got["face"], ref["face"]), tag
    assert np.array_equal(got["skipped"], ref["skipped"]), tag
    cov = ref["mask"] == 255
    assert (got["depth"][~cov] == 0).all() and (got["xyz"][~cov] == 0).all() and (got["rgb"][~cov] == 0).all()
    if not cov.any():
        return 0.0, 0.0, 0.0
    fd = (np.abs(got["depth"].astype(np.float64) - ref["depth"])[cov] / (DEPTH_BOUND * ref["depth"][cov])).max()
    err, lim = np.abs(got["xyz"].astype(np.float64) - ref["xyz"])[cov], XYZ_BOUND * ref["xyz_scale"][cov]
    assert (err[lim == 0] == 0).all(), tag
    fx = (err[lim > 0] / lim[lim > 0]).max() if (lim > 0).any() else 0.0
    dc = np.abs(got["rgb"].astype(np.int32) - ref["rgb"].astype(np.int32))[cov]
    print(f"[render {tag}] covered {int(cov.sum())} px; worst fraction of the bound: depth {fd:.3f}, xyz {fx:.3f}; "
          f"rgb off by one in {(dc == 1).mean():.4f} of the values, max {int(dc.max())}")
    assert fd <= 1.0 and fx <= 1.0, (tag, fd, fx)
    assert dc.max() <= 1, tag
    return fd, fx, float((dc == 1).mean())


def check_mesh(ops, name):
    """The torus (576 faces, occludes itself, every triangle walked by one lane) and the cube of half-side 50 (12 faces) at three
    seeded rotations against the restatement.  At 400 units a cube face spans 15 pixels, so only the faces seen at an angle pass
    the 16 x 16 threshold and both kernels draw into the same views; "cube-near" is the same cube at 220 units, where all 12
    faces of every view are shared by a workgroup and the views run over the image border."""
    v, f, c, P, ref = _mesh(name)
    cov = ref["mask"] == 255
    assert cov.sum() > 300 and ref["skipped"].sum() == 0
    # preconditions, on the restatement alone: the visible face is decided far above the depth rounding; closed meshes have an
    # even number of layers at every covered pixel (the rule is watertight)
    two = np.isfinite(ref["z2"])
    gap = ((ref["z2"][two] - ref["z1"][two]) / ref["z1"][two]).min()
    print(f"[render {name}] minimum relative gap of the two nearest layers {gap:.3e} (required {MIN_GAP:.1e}); "
          f"workgroup-shared triangles per view {ref['large'].tolist()}")
    assert gap >= MIN_GAP
    assert (ref["layers"][cov] % 2 == 0).all()
    assert {"torus": (ref["large"] == 0).all(), "cube": 0 < ref["large"].sum() < 36, "cube-near": (ref["large"] == 12).all()}[name]
    fd, fx, share = _compare(_render(ops, v, f, c, P), ref, name)
    util.record_margin(f"render_{name}_48x64", depth_err_over_bound=fd, xyz_err_over_bound=fx, rgb_off_by_one_share=share, bound_ratio=1.0)


def check_fill_rule(ops):
    """Two triangles forming the square of pixels (10, 8) .. (20, 18), vertices exactly on pixel centres: top and left edges in,
    bottom and right edges out, every sample of the shared diagonal covered once, the same image for both windings."""
    v = np.array([_at(10, 8), _at(20, 8), _at(20, 18), _at(10, 18)], np.float32)
    want = np.zeros((1, H, W), np.uint8)
    want[0, 8:18, 10:20] = 255
    images = []
    for faces in ([[0, 1, 2], [0, 2, 3]], [[0, 2, 1], [0, 3, 2]], [[0, 1, 2], [0, 3, 2]]):
        f = np.array(faces, np.int32)
        ref = R.render(v, f, _grey(v), EYE, K, H, W, AMBIENT, DIFFUSE, ZNEAR)
        assert np.array_equal(ref["mask"], want) and (ref["layers"][want == 255] == 1).all()
        assert set(ref["face"][0][np.arange(8, 18), np.arange(10, 20)]) <= {0, 1}          # the diagonal's samples
        got = _render(ops, v, f, _grey(v), EYE)
        assert np.array_equal(got["mask"], want)
        _compare(got, ref, f"square {faces}")
        images.append(got)
    for other in images[1:]:
        assert np.array_equal(other["mask"], images[0]["mask"]) and np.array_equal(other["face"], images[0]["face"])
        assert np.abs(other["rgb"].astype(np.int32) - images[0]["rgb"]).max() <= 1          # (the vertex order permutes the sums)
        assert np.abs(other["depth"] - images[0]["depth"]).max() <= 2 * DEPTH_BOUND * 60.0


HOSTILE = {
    # name: (vertices, faces, covered?, workgroup-shared triangles, skipped)
    "off-screen": ([_at(-50, 5), _at(-30, 5), _at(-40, 30)], [[0, 1, 2]], False, 0, 0),
    "straddles the border": ([_at(-10, 5), _at(15, -7), _at(5, 30)], [[0, 1, 2]], True, 1, 0),
    "straddles the corner": ([_at(55, 40), _at(80, 44), _at(60, 70)], [[0, 1, 2]], True, 0, 0),
    "sub-pixel": ([_at(10.2, 10.2), _at(10.7, 10.3), _at(10.4, 10.8)], [[0, 1, 2]], False, 0, 0),
    "zero area": ([_at(10, 10), _at(15, 15), _at(20, 20), _at(30, 12)], [[0, 1, 2], [3, 3, 0]], False, 0, 0),
    "16 x 16 samples: one lane": ([_at(10, 10), _at(25, 10), _at(10, 25)], [[0, 1, 2]], True, 0, 0),
    "17 x 16 samples: a workgroup": ([_at(10, 10), _at(26, 10), _at(10, 25)], [[0, 1, 2]], True, 1, 0),
    "either side of the threshold, overlapping": ([_at(10, 10, 70.0), _at(25, 10, 70.0), _at(10, 25, 72.0), _at(9, 12, 50.0), _at(25, 11, 55.0),
                                                   _at(12, 27, 60.0)], [[0, 1, 2], [3, 4, 5]], True, 1, 0),
    "behind znear": ([_at(10, 10), _at(25, 10), _at(10, 25), [0.0, 0.0, -5.0]], [[0, 1, 2], [0, 1, 3]], True, 0, 1),
}


def check_hostile(ops, name):
    verts, faces, covered, large, skipped = HOSTILE[name]
    v, f = np.array(verts, np.float32), np.array(faces, np.int32)
    ref = R.render(v, f, _grey(v), EYE, K, H, W, AMBIENT, DIFFUSE, ZNEAR)
    assert bool((ref["mask"] == 255).any()) == covered and int(ref["large"][0]) == large and int(ref["skipped"][0]) == skipped, name
    _compare(_render(ops, v, f, _grey(v), EYE), ref, name)
    if skipped:
        from sam6d_amd import render
        with pytest.raises(ValueError, match=r"view\(s\) 0 \(1\)"):
            render.render_templates(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(EYE).cuda(), KM, (H, W))


def check_determinism(ops):
    """Two runs are equal; a view alone equals the view inside a batch, bit for bit; of two coincident copies of every face the
    lower index is visible."""
    v, f, c, P, ref = _mesh("torus")
    a, b = _render(ops, v, f, c, P), _render(ops, v, f, c, P)
    assert all(np.array_equal(a[k], b[k]) for k in OUT)
    one = _render(ops, v, f, c, P[1:2])
    assert all(np.array_equal(one[k][0], a[k][1]) for k in OUT)
    twice = _render(ops, v, np.concatenate([f, f]), c, P)
    assert all(np.array_equal(twice[k], a[k]) for k in OUT)
    swapped = _render(ops, v, np.concatenate([f[::-1], f]), c, P[:1])      # face i and face 2F-1-i coincide: the lower one wins
    F = len(f)
    vis = a["face"][:1]
    assert np.array_equal(swapped["face"], np.where(vis >= 0, np.minimum(F - 1 - vis, F + vis), -1))
    assert np.array_equal(swapped["depth"], a["depth"][:1])


def check_arguments(ops):
    """Host tensors, other dtypes and shapes, and a face index >= V are refused by the wrapper; the entry point answers -3 for a
    view beyond 32768 pixels a side, -1 for NULL operands and bad sizes, 0 for no views -- before any launch."""
    v, f, c, P, _ = _mesh("cube")
    tv, tf, tc, tp = (torch.from_numpy(a).cuda() for a in (v, f, c, P))
    call = lambda *a: ops.render_views(*a, *K, H, W, AMBIENT, DIFFUSE, ZNEAR)          # noqa: E731
    if not torch.zeros(1).is_cuda:                                                    # (the host build's fixture makes every tensor claim the device)
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            call(tv.cpu(), tf.cpu(), tc.cpu(), tp.cpu())
    with pytest.raises(RuntimeError, match="float"):
        call(tv.double(), tf, tc, tp)
    with pytest.raises(RuntimeError, match="an int tensor"):
        call(tv, tf.long(), tc, tp)
    with pytest.raises(RuntimeError, match="uint8"):
        call(tv, tf, tc.float(), tp)
    with pytest.raises(ValueError, match="expected"):
        call(tv, tf, tc[:4].contiguous(), tp)
    bad = tf.clone()
    bad[3, 1] = len(v)
    with pytest.raises(ValueError, match=r"face indices must lie in \[0, 8\)"):
        call(tv, bad, tc, tp)
    bad[3, 1] = -1
    with pytest.raises(ValueError, match="face indices"):
        call(tv, bad, tc, tp)
    assert ops._size("s6d_raster_workspace_bytes", 3, 12, H, W) >= 3 * H * W * 8 + 3 * 12 * 4
    assert ops._size("s6d_raster_workspace_bytes", 3, 12, 40000, W) == -1
    fn = ops._fn("s6d_raster_views_f32", 24)
    mark = torch.full((3, H, W), 7, dtype=torch.int32).cuda()
    ws = torch.zeros(3 * H * W + 64, dtype=torch.int64).cuda()
    o = dict(rgb=torch.zeros(3, H, W, 3, dtype=torch.uint8).cuda(), mask=torch.zeros(3, H, W, dtype=torch.uint8).cuda(),
             xyz=torch.zeros(3, H, W, 3).cuda(), depth=torch.zeros(3, H, W).cuda(), skipped=torch.zeros(3, dtype=torch.int32).cuda())
    Pp = lambda t: t.data_ptr()                                                       # noqa: E731

    def raw(vp, T, h, znear=ZNEAR, wsp=Pp(ws)):
        return fn(vp, Pp(tf), Pp(tc), Pp(tp), 8, 12, T, h, W, *K, znear, AMBIENT, DIFFUSE, wsp, Pp(o["rgb"]), Pp(o["mask"]), Pp(o["xyz"]),
                  Pp(o["depth"]), Pp(mark), Pp(o["skipped"]), ops._stream())
    assert raw(Pp(tv), 3, 40000) == -3
    assert raw(None, 3, H) == -1
    assert raw(Pp(tv), 3, H, wsp=None) == -1
    assert raw(Pp(tv), 3, 0) == -1
    assert raw(Pp(tv), -1, H) == -1
    assert raw(Pp(tv), 3, H, znear=-1.0) == -1
    assert raw(Pp(tv), 3, H, znear=float("nan")) == -1
    assert raw(Pp(tv), 0, H) == 0
    torch.cuda.synchronize()
    assert (mark.cpu() == 7).all()


# ---------------------------------------------------------------------------------------------------------------- on the MI355X
@pytest.mark.parametrize("name", ["torus", "cube", "cube-near"])
def test_mesh_vs_restatement(ops, name):
    check_mesh(ops, name)


def test_fill_rule(ops):
    check_fill_rule(ops)


@pytest.mark.parametrize("name", sorted(HOSTILE))
def test_hostile_geometry(ops, name):
    check_hostile(ops, name)


def test_determinism(ops):
    check_determinism(ops)


def test_arguments(ops):
    check_arguments(ops)


def test_render_templates_layout(ops):
    """The public call: dtypes and layout as onboarding takes them, a uniform grey without colours, numpy inputs accepted."""
    from sam6d_amd import render
    v, f, c, P, ref = _mesh("cube")
    out = render.render_templates(v, f, P, KM, (H, W), colors=c, ambient=AMBIENT, diffuse=DIFFUSE, znear=ZNEAR)
    assert sorted(out) == ["depth", "face", "mask", "rgb", "xyz_mm"]
    assert out["rgb"].dtype == torch.uint8 and tuple(out["rgb"].shape) == (3, H, W, 3) and out["rgb"].is_cuda
    assert out["mask"].dtype == torch.uint8 and out["xyz_mm"].dtype == torch.float32 and tuple(out["xyz_mm"].shape) == (3, H, W, 3)
    assert np.array_equal(out["mask"].cpu().numpy(), ref["mask"]) and np.array_equal(out["face"].cpu().numpy(), ref["face"])
    grey = render.render_templates(v, f, P, KM, (H, W))
    g = grey["rgb"].cpu().numpy()
    cov = ref["mask"] == 255
    assert (g[cov].max(1) == g[cov].min(1)).all() and g[cov].max() <= render.GREY and g[cov].min() >= int(0.3 * render.GREY)
