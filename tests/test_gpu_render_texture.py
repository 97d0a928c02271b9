"""ops.texture_pyramid / ops.render_views_textured / render.render_templates(uv=, texture=) (s6d_texture_pyramid_u8,
s6d_raster_views_tex_f32, csrc/s6d_raster.hip) against the numpy restatement of tests/texture_ref.py.  The bodies take `ops` so
that tests/test_emu_render_texture.py runs them on the host build.

What is held (bounds derived in profiles/render_margins.md, "texture"; none was chosen by looking at the kernel's output):
  pyramid   equal, every level down to 1 x 1
  geometry  mask, xyz, depth, face, skipped: equal to ops.render_views on the same mesh (bit for bit)
  level     equal wherever the float64 rho^2 is further from every switch 2^(2L-1) than the error bound of the float32 chain
            (``rho2_err`` of the restatement, per pixel); inside it either neighbouring level; at most 1 % of the covered pixels
            may be inside, asserted on the restatement alone
  rgb       within one level of the rounded float64 value at that level, plus the bound the uv error gives,
            (du W_L + dv H_L) 255 shade: far below one level at these sizes, so the values differ by at most 1
48 x 64 views, fx = fy = 60, c = (32, 24), T = 3."""
import functools

import numpy as np
import pytest
import torch

from tests import render_ref as R
from tests import test_gpu_render as G
from tests import texture_ref as X
from tests import util

pytestmark = pytest.mark.gpu

H, W, K, KM = G.H, G.W, G.K, G.KM
AMBIENT, DIFFUSE, ZNEAR = G.AMBIENT, G.DIFFUSE, G.ZNEAR
GEOMETRY = ("mask", "xyz", "depth", "face", "skipped")
MAX_MARGIN_SHARE = 0.01


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from sam6d_amd import ops
    return ops


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _quad(uv0, uv1):
    """A fronto-parallel quad over pixels (8, 8) .. (56, 40) at depth 60, two triangles with a uv chart each."""
    v = np.array([G._at(8, 8), G._at(56, 8), G._at(56, 40), G._at(8, 40)], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), np.array([uv0, uv1], np.float32)


def _tilted():
    """A quad of 120 x 2000 units tilted 60 degrees about the image's x axis, from 70 to 1100 units in front of the camera, the
    texture repeated 1 x 24 times over it: magnified at the near edge, strongly minified at the far one."""
    a = np.deg2rad(60.0)
    y0, z0, length, half = 18.0, 70.0, 2000.0, 60.0
    near, far = np.array([y0, z0]), np.array([y0 - length * np.cos(a), z0 + length * np.sin(a)])
    v = np.array([[-half, near[0], near[1]], [half, near[0], near[1]], [half, far[0], far[1]], [-half, far[0], far[1]]], np.float32)
    uv = np.array([[[0, 0], [1, 0], [1, 24]], [[0, 0], [1, 24], [0, 24]]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), uv


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(vertices, faces, uv, image, poses) and the restatement of a scene, computed once and only read."""
    eye3 = np.repeat(G.EYE, 3, 0)
    if name == "quad":                    # a seam: the second triangle's chart is the first one's turned and shifted
        v, f, uv = _quad([[0, 0], [1, 0], [1, 1]], [[0.25, 1.5], [1.25, 0.5], [0.25, 0.5]])
        img, P = X.texture(4, 4, 5), eye3
    elif name == "wrap":
        v, f, uv = _quad([[-0.75, -0.75], [1.5, -0.75], [1.5, 1.5]], [[-0.75, -0.75], [1.5, 1.5], [-0.75, 1.5]])
        img, P = X.texture(4, 4, 6), eye3
    elif name == "minified":
        v, f, uv = _tilted()
        img, P = X.texture(32, 64, 7), eye3
    elif name == "odd":
        v, f, uv = _quad([[0, 0], [24, 0], [24, 24]], [[0, 0], [3, 3], [0, 3]])          # 2.5 texels a pixel (level 1) beside 0.3 (level 0)
        img, P = X.texture(3, 5, 8), eye3
    elif name == "cube":
        v, f, _ = R.cube()
        uv, img, P = X.cube_uv(), X.texture(32, 64, 9), R.poses(3, seed=3, t=(3.0, -2.0, 220.0))
    elif name == "torus":
        v, f, _ = R.torus()
        uv, img, P = X.expand(X.torus_uv(), f), X.texture(32, 64, 10), R.poses(3, seed=11)
    else:
        raise KeyError(name)
    if name in ("quad", "wrap", "minified", "odd"):          # three views: the quad shifted by a fraction of a pixel
        P = P.copy()
        P[1, 0, 3], P[2, 1, 3] = 0.37, -0.61
    return v, f, uv, img, P, X.render(v, f, uv, img, P, K, H, W, AMBIENT, DIFFUSE, ZNEAR)


def _render(ops, v, f, uv, img, P, pyramid=None):
    pyr = ops.texture_pyramid(_t(img)) if pyramid is None else pyramid
    out = ops.render_views_textured(_t(v), _t(f), _t(uv), pyr, _t(P), *K, H, W, AMBIENT, DIFFUSE, ZNEAR, tex_size=img.shape[:2], levels=True)
    torch.cuda.synchronize()
    return {k: a.cpu().numpy() for k, a in out.items()}


def _untextured(ops, v, f, P):
    out = ops.render_views(_t(v), _t(f), _t(np.full((len(v), 3), 200, np.uint8)), _t(P), *K, H, W, AMBIENT, DIFFUSE, ZNEAR)
    torch.cuda.synchronize()
    return {k: a.cpu().numpy() for k, a in out.items()}


def _compare(ops, name, got=None):
    """Geometry against ops.render_views (equal), level and rgb against the restatement.  -> the textured render."""
    v, f, uv, img, P, ref = _scene(name)
    got = _render(ops, v, f, uv, img, P) if got is None else got
    plain = _untextured(ops, v, f, P)
    for k in GEOMETRY:
        assert np.array_equal(got[k], plain[k], equal_nan=True), (name, k)
    assert np.array_equal(got["mask"], ref["mask"]) and np.array_equal(got["face"], ref["face"]), name
    cov = ref["mask"] == 255
    assert cov.sum() > 300 and (got["rgb"][~cov] == 0).all() and (got["level"][~cov] == -1).all()
    margin = cov & (ref["alt_level"] >= 0)
    share = margin.sum() / cov.sum()
    print(f"[texture {name}] covered {int(cov.sum())} px, levels {sorted(set(ref['level'][cov].tolist()))}, inside the level margin "
          f"{int(margin.sum())} ({share:.4f}), largest relative margin {np.max(ref['rho2_err'][cov] / np.maximum(ref['rho2'][cov], 1e-300), initial=0):.2e}, "
          f"largest uv colour bound {ref['uv_tol'][cov].max():.2e} levels")
    assert share <= MAX_MARGIN_SHARE, (name, share)          # a precondition, on the restatement alone
    sure = cov & ~margin
    assert np.array_equal(got["level"][sure], ref["level"][sure]), name
    took_alt = margin & (got["level"] == ref["alt_level"])
    assert ((got["level"] == ref["level"]) | took_alt)[margin].all(), name
    want = np.where(took_alt[..., None], ref["rgb_alt"], ref["rgb"]).astype(np.int32)
    diff = np.abs(got["rgb"].astype(np.int32) - want)[cov]
    tol = (1.0 + ref["uv_tol"])[cov][:, None]
    print(f"[texture {name}] rgb off by one in {(diff == 1).mean():.4f} of the values, max {int(diff.max())}")
    assert (diff <= tol).all(), (name, int(diff.max()))
    util.record_margin(f"render_texture_{name}_48x64", rgb_off_by_one_share=float((diff == 1).mean()), level_margin_share=float(share),
                       uv_colour_bound_levels=float(ref["uv_tol"][cov].max()), bound_ratio=1.0)
    return got


# ------------------------------------------------------------------------------------------------------------------- bodies
def check_pyramid(ops, shape):
    """Every level down to 1 x 1 equal to the integer restatement; odd sizes drop the last column or row of the finer level."""
    Ht, Wt = shape
    img = X.texture(Ht, Wt, 100 + Ht * 31 + Wt)
    got = ops.texture_pyramid(_t(img))
    torch.cuda.synchronize()
    want = X.pyramid(img)
    assert tuple(got.shape) == (sum(a.shape[0] * a.shape[1] for a in want), 4) and got.dtype == torch.uint8
    levels = X.unpack(got.cpu().numpy(), Ht, Wt)
    assert len(levels) == X.lmax(Ht, Wt) + 1 and levels[-1].shape[:2] == (1, 1)
    for l, (a, b) in enumerate(zip(levels, want)):
        assert np.array_equal(a, b), (shape, l)
    assert np.array_equal(levels[0], img)


def check_quad(ops):
    """Magnified 4 x 4 texture, a seam between the two triangles: bilinear weights, the v flip, per-corner uv, level 0 everywhere."""
    _, _, uv, img, _, ref = _scene("quad")
    cov = ref["mask"] == 255
    assert (ref["level"][cov] == 0).all() and (ref["alt_level"][cov] == -1).all()
    got = _compare(ops, "quad")
    assert (got["level"][cov] == 0).all()
    # a known answer for the v flip: pixel (26, 12) of the first view lies in triangle 0 at uv = (18 / 48, 4 / 32) = (0.375, 0.125),
    # i.e. x = 1, y = 3 exactly: the texel of column 1 in the BOTTOM row, times the shade
    v, f, _, _, P, _ = _scene("quad")
    assert ref["face"][0, 12, 26] == 0 and set(ref["face"][0][cov[0]].tolist()) == {0, 1}
    want = img[3, 1].astype(np.float64) * _shade(v, f, P)[0, 12, 26]
    assert np.allclose(ref["rgb_exact"][0, 12, 26], want, atol=1e-9)
    assert np.abs(got["rgb"][0, 12, 26] - np.rint(want)).max() <= 1


def check_wrap(ops):
    """uv over [-0.75, 1.5]: repeat wrap, negative coordinates, and both wrapped indices (i0 = -1, i1 = W_L) occur."""
    v, f, uv, img, P, ref = _scene("wrap")
    cov = ref["mask"] == 255
    assert (ref["level"][cov] == 0).all()
    # on the restatement: pixels whose footprint wraps around the texture's edge exist in both directions
    b = np.linspace(-0.75, 1.5, 49)[:-1]                      # u at the quad's pixel columns (48 pixels span 2.25)
    x = (b - np.floor(b)) * 4 - 0.5
    assert (x < 0).any() and (np.floor(x) + 1 == 4).any() and (b < 0).any()
    _compare(ops, "wrap")


def check_minified(ops):
    """A 64 x 32 texture on the tilted quad: the restatement's map holds at least the levels 0 to 3."""
    ref = _scene("minified")[5]
    cov = ref["mask"] == 255
    assert {0, 1, 2, 3} <= set(ref["level"][cov].tolist())
    got = _compare(ops, "minified")
    assert {0, 1, 2, 3} <= set(got["level"][cov].tolist())


def check_odd(ops):
    """A render from the 5 x 3 pyramid (levels 5 x 3, 2 x 1, 1 x 1)."""
    ref = _scene("odd")[5]
    assert len(set(ref["level"][ref["mask"] == 255].tolist())) >= 2
    _compare(ops, "odd")


def check_mesh(ops, name):
    """The cube at 220 units with per-corner uv (a workgroup per triangle) and the torus with per-vertex uv expanded (a lane per
    triangle) at three seeded rotations; each view rendered alone has the bits it has in the batch."""
    v, f, uv, img, P, ref = _scene(name)
    assert {"cube": (ref["large"] == 12).all(), "torus": (ref["large"] == 0).all()}[name] and ref["skipped"].sum() == 0
    got = _compare(ops, name)
    pyr = ops.texture_pyramid(_t(img))
    for i in range(len(P)):
        one = _render(ops, v, f, uv, img, P[i:i + 1], pyramid=pyr)
        assert all(np.array_equal(one[k][0], got[k][i]) for k in got), (name, i)


def check_hostile(ops, value):
    """The uv of one visible face of the cube set to NaN, +inf or 1e30: its pixels are black (NaN, inf) or as defined (1e30 -
    floorf(1e30) = 0 for u and v: the point between the four corner texels of the level, weights 1/2, and the level is 0 or Lmax,
    a float32 difference of such values being 0 or at least ulp(1e30) = 7.6e22, whose square overflows); every other pixel keeps
    its bits and so does the geometry; no texel outside the pyramid is read (the values say so: black, or a mean of pyramid
    texels)."""
    v, f, uv, img, P, ref = _scene("cube")
    seen = [int(k) for k in np.unique(ref["face"]) if k >= 0]
    bad = uv.copy()
    hit = seen[0]
    bad[hit] = value
    clean, got = _render(ops, v, f, uv, img, P), _render(ops, v, f, bad, img, P)
    there = ref["face"] == hit
    assert there.sum() > 50
    for k in GEOMETRY:
        assert np.array_equal(got[k], clean[k]), k
    assert np.array_equal(got["rgb"][~there], clean["rgb"][~there]) and np.array_equal(got["level"][~there], clean["level"][~there])
    L = X.lmax(*img.shape[:2])
    if np.isfinite(value):
        assert set(got["level"][there].tolist()) <= {0, L}
        lv = X.pyramid(img)
        corner = {l: lv[l].astype(np.float64)[[0, 0, -1, -1], [0, -1, 0, -1]].mean(0) for l in (0, L)}
        shade = _shade(v, f, P)[there]
        want = np.stack([corner[int(l)] for l in got["level"][there]]) * shade[:, None]
        assert np.abs(got["rgb"][there] - np.rint(want)).max() <= 1
    else:
        assert (got["rgb"][there] == 0).all() and (got["level"][there] == L).all()
        assert (got["mask"][there] == 255).all()


def _shade(v, f, P):
    """ambient + diffuse |n . d| per pixel in float64: render_ref's colour of a white mesh over 255."""
    white = R.render(v, f, np.full((len(v), 3), 255, np.uint8), P, K, H, W, AMBIENT, DIFFUSE, ZNEAR)
    return white["rgb_exact"][..., 0] / 255.0


def check_arguments(ops):
    """uv of the wrong shape or dtype, a pyramid that does not fit tex_size, sizes of 0 or above 8192 and null operands are
    refused before any launch; a texture without uv (and uv without a texture) by render_templates."""
    from sam6d_amd import render
    v, f, uv, img, P, _ = _scene("cube")
    tv, tf, tu, tp = _t(v), _t(f), _t(uv), _t(P)
    pyr = ops.texture_pyramid(_t(img))
    call = lambda *a, size=img.shape[:2]: ops.render_views_textured(*a, *K, H, W, AMBIENT, DIFFUSE, ZNEAR, tex_size=size)          # noqa: E731
    with pytest.raises(ValueError, match=r"uv \(F,3,2\)"):
        call(tv, tf, tu[:5].contiguous(), pyr, tp)
    with pytest.raises(ValueError, match=r"uv \(F,3,2\)"):
        call(tv, tf, tu.reshape(12, 6, 1), pyr, tp)
    with pytest.raises(RuntimeError, match="uv must be a float"):
        call(tv, tf, tu.double(), pyr, tp)
    with pytest.raises(RuntimeError, match="uint8"):
        call(tv, tf, tu, pyr.int(), tp)
    with pytest.raises(ValueError, match="tex_size"):
        call(tv, tf, tu, pyr, tp, size=(64, 64))
    with pytest.raises(ValueError, match="tex_size"):
        call(tv, tf, tu, pyr, tp, size=(0, 64))
    bad = tf.clone()
    bad[3, 1] = len(v)
    with pytest.raises(ValueError, match=r"face indices must lie in \[0, 8\)"):
        call(tv, bad, tu, pyr, tp)
    with pytest.raises(ValueError, match="image"):
        ops.texture_pyramid(torch.zeros(4, 4, 4, dtype=torch.uint8).cuda())
    with pytest.raises(RuntimeError, match="uint8"):
        ops.texture_pyramid(torch.zeros(4, 4, 3).cuda())
    assert ops._size("s6d_texture_pyramid_bytes", 32, 64) == 4 * (2048 + 512 + 128 + 32 + 8 + 2 + 1)
    assert ops._size("s6d_texture_pyramid_bytes", 8192, 8192) == 4 * sum(4 ** k for k in range(14))
    assert ops._size("s6d_texture_pyramid_bytes", 0, 64) == -1 and ops._size("s6d_texture_pyramid_bytes", 64, 8193) == -1
    Pp = lambda t: t.data_ptr()                                                       # noqa: E731
    build = ops._fn("s6d_texture_pyramid_u8", 5)
    timg = _t(img)
    assert build(None, 32, 64, Pp(pyr), ops._stream()) == -1 and build(Pp(timg), 32, 64, None, ops._stream()) == -1
    assert build(Pp(timg), 0, 64, Pp(pyr), ops._stream()) == -1 and build(Pp(timg), 32, 8193, Pp(pyr), ops._stream()) == -1
    fn = ops._fn("s6d_raster_views_tex_f32", 28)
    mark = torch.full((3, H, W), 7, dtype=torch.int32).cuda()
    ws = torch.zeros(3 * H * W + 64, dtype=torch.int64).cuda()
    o = dict(rgb=torch.zeros(3, H, W, 3, dtype=torch.uint8).cuda(), mask=torch.zeros(3, H, W, dtype=torch.uint8).cuda(),
             xyz=torch.zeros(3, H, W, 3).cuda(), depth=torch.zeros(3, H, W).cuda(), skipped=torch.zeros(3, dtype=torch.int32).cuda())

    def raw(uvp, pyrp, T=3, Ht=32, Wt=64, wsp=Pp(ws)):
        return fn(Pp(tv), Pp(tf), uvp, pyrp, Pp(tp), 8, 12, T, H, W, Ht, Wt, *K, ZNEAR, AMBIENT, DIFFUSE, wsp, Pp(o["rgb"]), Pp(o["mask"]),
                  Pp(o["xyz"]), Pp(o["depth"]), Pp(mark), None, Pp(o["skipped"]), ops._stream())
    assert raw(None, Pp(pyr)) == -1 and raw(Pp(tu), None) == -1 and raw(Pp(tu), Pp(pyr), wsp=None) == -1
    assert raw(Pp(tu), Pp(pyr), Ht=0) == -1 and raw(Pp(tu), Pp(pyr), Wt=8193) == -1 and raw(Pp(tu), Pp(pyr), Ht=-4) == -1
    assert raw(Pp(tu), Pp(pyr), T=-1) == -1 and raw(Pp(tu), Pp(pyr), T=0) == 0
    torch.cuda.synchronize()
    assert (mark.cpu() == 7).all()
    with pytest.raises(ValueError, match="uv and texture must be given together"):
        render.render_templates(v, f, P, KM, (H, W), texture=img)
    with pytest.raises(ValueError, match="uv and texture must be given together"):
        render.render_templates(v, f, P, KM, (H, W), uv=uv)


def check_render_templates(ops):
    """The public call: the views of ops.render_views_textured, vertex colours playing no part."""
    from sam6d_amd import render
    v, f, uv, img, P, ref = _scene("cube")
    want = _render(ops, v, f, uv, img, P)
    out = render.render_templates(v, f, P, KM, (H, W), colors=R.cube()[2], ambient=AMBIENT, diffuse=DIFFUSE, znear=ZNEAR, uv=uv, texture=img)
    assert sorted(out) == ["depth", "face", "mask", "rgb", "xyz_mm"] and out["rgb"].dtype == torch.uint8
    for a, b in (("rgb", "rgb"), ("mask", "mask"), ("xyz_mm", "xyz"), ("depth", "depth"), ("face", "face")):
        assert np.array_equal(out[a].cpu().numpy(), want[b]), a


# ---------------------------------------------------------------------------------------------------------------- on the MI355X
@pytest.mark.parametrize("shape", [(3, 5), (7, 1), (8, 8), (32, 64)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_pyramid(ops, shape):
    check_pyramid(ops, shape)


def test_quad_level_0(ops):
    check_quad(ops)


def test_wrap(ops):
    check_wrap(ops)


def test_minification(ops):
    check_minified(ops)


def test_odd_sizes(ops):
    check_odd(ops)


@pytest.mark.parametrize("name", ["cube", "torus"])
def test_mesh_vs_restatement(ops, name):
    check_mesh(ops, name)


@pytest.mark.parametrize("value", [float("nan"), float("inf"), 1e30], ids=["nan", "inf", "1e30"])
def test_hostile_uv(ops, value):
    check_hostile(ops, value)


def test_arguments(ops):
    check_arguments(ops)


def test_render_templates_textured(ops):
    check_render_templates(ops)


def test_textured_render_is_refused_without_its_kernel(ops):
    """No quiet grey: with the kernel switched off the textured render raises."""
    from sam6d_amd import policy, render
    v, f, uv, img, P, _ = _scene("cube")
    with policy.use(disable_fused="render_views_textured"):
        with pytest.raises(RuntimeError, match="textured render"):
            render.render_templates(v, f, P, KM, (H, W), uv=uv, texture=img)


def test_onboard_from_textured_mesh():
    """onboard_from_mesh with a five-element entry equals onboard on the views of render_templates(uv=, texture=), with the models
    and sizes of tests/test_gpu_render_onboarding.py; and the descriptors differ from those of the same mesh rendered grey: the
    texture reached the models."""
    from sam6d_amd import onboarding as ob
    from sam6d_amd import render
    from tests import test_gpu_render_onboarding as O
    dev = torch.device("cuda", 0)
    desc, net = O._models(dev)
    v, f, _ = R.torus()
    uv, img = X.expand(X.torus_uv(), f), X.texture(32, 64, 10)
    T, n_m, n_i = 4, 64, 32
    poses = R.poses(T, seed=7)
    g = torch.Generator().manual_seed(21)
    su = torch.rand(1, n_m + n_i, 3, generator=g)
    keys = torch.rand(1, T, O.H * O.W, generator=g)
    kw = dict(n_view=4, n_sample=600, img_size=224)
    got = render.onboard_from_mesh(desc, net, [(v, f, None, uv, img)], poses, O.KM, (O.H, O.W), surface_uniforms=su, keys=keys,
                                   n_model_points=n_m, n_ism_points=n_i, **kw)
    grey = render.onboard_from_mesh(desc, net, [(v, f, None)], poses, O.KM, (O.H, O.W), surface_uniforms=su, keys=keys,
                                    n_model_points=n_m, n_ism_points=n_i, **kw)
    views = render.render_templates(v, f, poses, O.KM, (O.H, O.W), uv=uv, texture=img)
    pts = render.sample_surface(torch.from_numpy(v), torch.from_numpy(f), n_m + n_i, su[0])[0] / torch.full((1,), 1000.0)
    want = ob.onboard(desc, net, [dict(rgb=views["rgb"], mask=views["mask"], xyz_mm=views["xyz_mm"], model_points=pts[:n_m],
                                       ism_points=pts[n_m:], poses=torch.from_numpy(poses))], keys=keys, **kw)
    for k in ("model", "dense_po", "dense_fo"):
        assert torch.equal(got.pem_templates[k], want.pem_templates[k]), k
    for k in ("descriptors", "appe_descriptors", "poses", "pointcloud"):
        assert torch.equal(got.scorer.ref_data[k], want.scorer.ref_data[k]), k
    assert not torch.equal(got.scorer.ref_data["descriptors"], grey.scorer.ref_data["descriptors"])
    assert not torch.equal(got.pem_templates["dense_fo"], grey.pem_templates["dense_fo"])
