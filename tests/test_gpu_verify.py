"""The pose verification kernels (csrc/s6d_verify.hip) and sam6d_amd.pem.verify on top of them against the plain-loop restatement
of tests/verify_ref.py.  Everything is integer work after two float32 operations per pixel, so everything is compared with EQUAL:
counts, inlier words and span of the evidence; status and fresh of the selection on both homes of the claimed bitmap; the module's
result on device tensors, its library branch and the restatement.  An instance alone has the bits it has in a batch; the four
classes add up to `rendered`; the tail bits are zero; the selection depends on `order` only, not on where the instances are stored.
Hostile pixels are written directly; the known answers are asserted on the restatement before any kernel output is read.  No other
tool's hypothesis verification is compared with.  The bodies take `ops` so that tests/test_emu_verify.py runs them on the host
build."""
import functools

import numpy as np
import pytest
import torch

from tests import render_ref as R
from tests import test_gpu_bop_eval as TB
from tests import test_gpu_bop_gt as TG
from tests import verify_ref as V

pytestmark = pytest.mark.gpu

ZNEAR = 1.0
TAU = 15.0
DEFAULTS = (12, 0.5, 0.5)                                                  # min_inliers, min_fit, min_fresh
SIZES = {(5, 7): (60.0, 60.0, 3.0, 2.0), (8, 8): (60.0, 60.0, 4.0, 4.0), (8, 16): (60.0, 60.0, 8.0, 4.0), (48, 64): TB.SIZES[(48, 64)]}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from sam6d_amd import ops
    return ops


_t, _np = TB._t, TB._np


def _words(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- scenes
def scene(ops, hw, N, M, name="cube", with_masks=False):
    """Renders of N instances (``TG.instance_poses``) and M measured depth images built like ``TG.scene``: the surface of instance
    m with noise (up to 20 units: inliers and both kinds of outliers at tau = 15), a wall behind, an occluder in front (a rendered
    cube nearer to the camera), 10 % missing.  masks: every instance's silhouette moved by a pixel, values 0, 1 and 255."""
    h, w = hw
    cam = np.array(SIZES[hw], np.float32)
    v, f = TG._mesh(name)
    cams = np.tile(cam, (N, 1))
    render, skipped = TG.canvases(ops, v, f, TG.instance_poses(hw, cam, N), cams, hw, (0, 0))
    assert skipped.sum() == 0
    rs = np.random.RandomState(1000 * h + 100 * N + 10 * M + len(name))
    ov, of = R.cube(30.0)[:2]
    occ_pose = R.poses(M, seed=5, t=(0.0, 0.0, 300.0)).astype(np.float64)
    for m in range(M):
        occ_pose[m, :3, 3] = ((w / 2 + 4 - cam[2]) / cam[0] * 300.0 + 8 * m, (h / 2 + 3 - cam[3]) / cam[1] * 300.0, 300.0)
    occ, _ = TG.canvases(ops, ov, of, occ_pose, np.tile(cam, (M, 1)), hw, (0, 0))
    obs = np.full((M, h, w), 460.0, np.float32)
    for m in range(M):
        surf = render[m % N]
        obs[m] = np.where(surf > 0, surf + rs.uniform(-20, 20, (h, w)).astype(np.float32), obs[m])
        obs[m] = np.where((occ[m] > 0) & (np.arange(w)[None] > w // 2), occ[m], obs[m])
        obs[m][rs.uniform(size=(h, w)) < 0.1] = 0.0
    oi = (np.arange(N) % M).astype(np.int32)
    masks = None
    if with_masks:
        masks = (np.roll(render > 0, 1, axis=2) * np.where(np.arange(w) % 2, 1, 255)[None, None]).astype(np.uint8)
    return render, obs, oi, masks


@functools.lru_cache(maxsize=None)
def _restated(key):
    """The restatement of a scene, once per (renders, depth, ...) the tests share; the arrays are handed in through ``_ARGS``."""
    return V.evidence(*_ARGS[key])


_ARGS = {}


def restate(key, *args):
    _ARGS[key] = args
    return _restated(key)


def evidence(ops, render, obs, oi, unit, tau, masks=None):
    out = ops.verify_evidence(_t(render), _t(obs), _t(oi), unit, tau, None if masks is None else _t(masks))
    torch.cuda.synchronize()
    return dict(counts=_np(out["counts"]).astype(np.int64), inlier=_words(_np(out["inlier"])), span=_np(out["span"]).astype(np.int64))


def same(got, ref):
    return all(np.array_equal(got[k], ref[k]) for k in ("counts", "inlier", "span"))


def check_evidence(ops, hw, N, M, with_masks, name="cube"):
    render, obs, oi, masks = scene(ops, hw, N, M, name, with_masks)
    ref = restate(("scene", hw, N, M, with_masks, name), render, obs, oi, 1.0, TAU, masks)
    c = ref["counts"]
    if hw == (48, 64):
        assert (c[0, :5] > 0).all() and c[0, 0] > 40, c[0]                 # every class occurs: the inputs, before the kernel is looked at
        assert not with_masks or (0 < c[0, 7] < c[0, 6] < c[0, 5])
    got = evidence(ops, render, obs, oi, 1.0, TAU, masks)
    print(f"[verify evidence {hw} N {N} M {M} masks {with_masks} {name}] counts {got['counts'].tolist()} span {got['span'].tolist()}")
    assert same(got, ref), (got["counts"], ref["counts"], got["span"], ref["span"])
    g = got["counts"]
    assert np.array_equal(g[:, 1:5].sum(1), g[:, 0]) and (g[:, 6] <= np.minimum(g[:, 5], g[:, 0])).all() and (g[:, 7] <= g[:, 6]).all()
    assert with_masks or not g[:, 5:].any()
    plane, words = hw[0] * hw[1], got["inlier"].shape[1]
    assert words == (plane + 63) // 64
    if plane % 64:
        assert not (got["inlier"][:, -1] >> np.uint64(plane % 64)).any()          # the tail bits
    assert np.array_equal(np.array([[bin(int(x)).count("1") for x in row] for row in got["inlier"]]).sum(1), g[:, 2])
    n = N - 2 if N > 1 else 0                                              # an instance alone has the bits it has in the batch
    alone = evidence(ops, render[n:n + 1], obs, oi[n:n + 1], 1.0, TAU, None if masks is None else masks[n:n + 1])
    assert all(np.array_equal(alone[k][0], got[k][n]) for k in got)


def contraction_probes(count=8, tau=TAU, unit=1000.0):
    """(depth, render) float32 pairs with fl(fl(depth unit) - render) == tau exactly while the fused value
    fl(depth unit - render) exceeds tau: render = fl(depth unit) - tau is exact, and the product's rounding error e = depth unit -
    fl(depth unit) (a float64 holds the product of two float32 exactly) is large enough that fl(tau + e) > tau."""
    rs = np.random.RandomState(19)
    depth = rs.uniform(0.3, 0.5, 4096).astype(np.float32)
    z = (depth * np.float32(unit)).astype(np.float32)
    r = (z - np.float32(tau)).astype(np.float32)
    exact = (z.astype(np.float64) - r.astype(np.float64)) == tau
    fused = (depth.astype(np.float64) * float(np.float32(unit)) - r.astype(np.float64)).astype(np.float32)
    pick = np.nonzero(exact & (fused > np.float32(tau)))[0][:count]
    assert len(pick) == count
    return depth[pick], r[pick]


def check_hostile(ops):
    """Pixels written directly on an (8,16) image of two words: depths that are NaN, +inf, negative and zero; renders that are NaN,
    negative and +inf; |d| exactly tau and one float32 step beyond; tau = 0; the contraction probes at depth_unit = 1000."""
    h, w = 8, 16
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    render = np.zeros((2, h, w), np.float32)
    obs = np.full((1, h, w), 400.0, np.float32)
    oi = np.zeros(2, np.int32)
    render[0, 0, :12] = 400.0
    obs[0, 0, :12] = [nan, inf, -5.0, 0.0, -0.0, 415.0, np.nextafter(np.float32(415.0), inf), 385.0, np.nextafter(np.float32(385.0), np.float32(0)),
                      400.0, 1e-30, 3e38]
    want0 = [0, 0, 0, 0, 0, 1, 3, 1, 2, 1, 2, 3]                           # V.evidence's classes: missing, inlier, occluded, behind
    render[0, 1, :5] = [nan, -3.0, 0.0, inf, -0.0]                          # not rendered, except +inf: occluded (d = -inf)
    render[1, 7, 15] = 400.0                                               # the last pixel of the last word
    ref = V.evidence(render, obs, oi, 1.0, TAU)
    assert ref["cls"][0, 0, :12].tolist() == want0 and ref["cls"][0, 1, :5].tolist() == [-1, -1, -1, 2, -1]
    assert ref["counts"][0].tolist() == [13, 5, 3, 3, 2, 0, 0, 0] and ref["span"].tolist() == [[0, 0], [1, 1]]
    assert int(ref["inlier"][1, 1]) == 1 << 63
    assert same(evidence(ops, render, obs, oi, 1.0, TAU), ref)
    # depth_unit takes 3e38 to +inf: missing
    ref = V.evidence(render, obs, oi, 2.0, TAU)
    assert ref["cls"][0, 0, 11] == 0
    assert same(evidence(ops, render, obs, oi, 2.0, TAU), ref)
    # tau = 0: only d == 0 is an inlier
    ref = V.evidence(render, obs, oi, 1.0, 0.0)
    assert ref["cls"][0, 0, :12].tolist() == [0, 0, 0, 0, 0, 3, 3, 2, 2, 1, 2, 3] and ref["counts"][0, 2] == 1
    assert same(evidence(ops, render, obs, oi, 1.0, 0.0), ref)
    # an empty render: (words, -1)
    ref = V.evidence(np.zeros_like(render), obs, oi, 1.0, TAU)
    assert ref["span"].tolist() == [[2, -1], [2, -1]] and not ref["counts"].any()
    assert same(evidence(ops, np.zeros_like(render), obs, oi, 1.0, TAU), ref)
    # the multiply and the subtraction are two roundings: a fused multiply-subtract would call these pixels BEHIND
    depth, r = contraction_probes()
    render = np.zeros((1, h, w), np.float32)
    obs = np.zeros((1, h, w), np.float32)
    render[0, 3, :len(r)], obs[0, 3, :len(r)] = r, depth
    ref = V.evidence(render, obs, oi[:1], 1000.0, TAU)
    assert (ref["cls"][0, 3, :len(r)] == 1).all() and ref["counts"][0].tolist() == [len(r), 0, len(r), 0, 0, 0, 0, 0]
    got = evidence(ops, render, obs, oi[:1], 1000.0, TAU)
    assert same(got, ref), (got["counts"], ref["counts"])


# ---------------------------------------------------------------------------------------------------------------- selection
def rect_scene(seed, hw=(8, 16), N=7, M=2):
    """Hand-made arrays: a measured plane at 400 with holes, `render` rectangles that overlap, at the plane, slightly off, far in
    front of it and far behind it; one tiny rectangle; one empty render."""
    h, w = hw
    rs = np.random.RandomState(seed)
    obs = np.full((M, h, w), 400.0, np.float32)
    obs[rs.uniform(size=obs.shape) < 0.1] = 0.0
    render = np.zeros((N, h, w), np.float32)
    for n in range(N - 1):
        y0, x0 = rs.randint(0, h - 3), rs.randint(0, w - 5)
        y1, x1 = (y0 + 1, x0 + 2) if n == 2 else (rs.randint(y0 + 3, h + 1), rs.randint(x0 + 5, w + 1))
        render[n, y0:y1, x0:x1] = 400.0 + [0.0, 5.0, -5.0, 0.0, -60.0, 60.0][n % 6]
        render[n, y0:y1, x0:x1] += np.where(rs.uniform(size=(y1 - y0, x1 - x0)) < 0.2, -40.0, 0.0).astype(np.float32)
    frame = rs.randint(0, M, N).astype(np.int32)
    flagged = np.zeros(N, np.uint8)
    flagged[rs.randint(0, N)] = 1
    return render, obs, frame, flagged


def select(ops, ev, order, start, flagged, thresholds, hw=None):
    t64 = lambda a: _t(np.ascontiguousarray(a).view(np.int64))            # noqa: E731
    st, fr = ops.verify_select(t64(ev["inlier"]), _t(ev["counts"].astype(np.int32)), _t(ev["span"].astype(np.int32)), _t(order), _t(start),
                               None if flagged is None else _t(flagged), *thresholds, *(hw or (None, None)))
    torch.cuda.synchronize()
    return _np(st).astype(np.int64), _np(fr).astype(np.int64)


def check_selection(ops, lds_words):
    """Both homes of the bitmap (lds_words = 0: LDS; 1: the workspace, at every shape of more than a word), two frames in one call;
    rows permuted with `order` mapped give the permuted result."""
    seen = set()
    ops.set_verify_lds_words(lds_words)
    try:
        cases = [(rect_scene(s), th) for s in range(6) for th in (DEFAULTS, (4, 0.8, 0.9), (0, 0.0, 0.0))]
        cases += [(rect_scene(11, (5, 7), 5, 1), DEFAULTS), (rect_scene(12, (8, 8), 6, 2), (2, 0.5, 0.5))]
        for (render, obs, frame, flagged), th in cases:
            hw = render.shape[1:]
            ev = restate(("rect", render.tobytes(), obs.tobytes()), render, obs, frame, 1.0, TAU, None)
            order, start = V.default_order(V.scores(ev["counts"], False)[0], ev["counts"], frame, len(obs))
            ref = V.select(ev["inlier"], ev["counts"], order, start, flagged, *th)
            seen |= set(ref[0].tolist())
            got = select(ops, ev, order, start, flagged, th, hw)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (got, ref, order, start)
            assert np.array_equal(select(ops, ev, order, start, flagged, th)[0], ref[0])          # without H, W
            perm = np.random.RandomState(3).permutation(len(render))          # row perm[i] of the new arrays is the old row i
            inv = np.argsort(perm)
            moved = {k: ev[k][inv] for k in ("inlier", "counts", "span")}
            got = select(ops, moved, perm[order].astype(np.int32), start, flagged[inv], th, hw)
            assert np.array_equal(got[0][perm], ref[0]) and np.array_equal(got[1][perm], ref[1])
            # fewer instances named than stored: the others keep status 4, fresh 0
            if start[1] > 1:
                got = select(ops, ev, order[1:].copy(), np.maximum(start - 1, 0), flagged, th, hw)
                assert got[0][order[0]] == 4 and got[1][order[0]] == 0
        # the scene of the evidence test: two frames, real renders, more than one word a row
        render, obs, oi, _ = scene(ops, (48, 64), 5, 2)
        ev = restate(("scene", (48, 64), 5, 2, False, "cube"), render, obs, oi, 1.0, TAU, None)
        order, start = V.default_order(V.scores(ev["counts"], False)[0], ev["counts"], oi, 2)
        for th in (DEFAULTS, (12, 0.1, 0.6)):
            ref = V.select(ev["inlier"], ev["counts"], order, start, None, *th)
            got = select(ops, ev, order, start, None, th, (48, 64))
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (got, ref)
            seen |= set(ref[0].tolist())
    finally:
        ops.set_verify_lds_words(0)
    assert seen == {0, 1, 2, 3, 4}, seen                                   # every status occurred


def truth_scene(ops):
    """(48,64): three true cube poses, the depth they make in front of a wall at 460; a shifted duplicate of each; one pose floating
    in front of everything and one in front of the bare wall.  -> dict(P (8,4,4) f32, render, obs, true (indices))."""
    hw, cam = (48, 64), np.array(SIZES[(48, 64)], np.float32)
    fx, fy, cx, cy = cam
    v, f = R.cube(40.0)[:2]
    at = lambda u, y, z: ((u - cx) / fx * z, (y - cy) / fy * z, z)       # noqa: E731
    P = R.poses(8, seed=7, t=(0.0, 0.0, 400.0)).astype(np.float32)
    true = [1, 3, 7]
    for n, (u, y) in zip(true, ((11.0, 12.0), (32.0, 33.0), (52.0, 13.0))):
        P[n, :3, 3] = at(u, y, 400.0)
    for dup, n in ((0, 1), (4, 3), (6, 7)):
        P[dup] = P[n]
        P[dup, :3, 3] += np.array([14.0, -9.0, 4.0], np.float32)           # two pixels and a few units off
    P[2] = P[1]
    P[2, :3, 3] = at(11.0, 12.0, 250.0)                                    # floating in front of the first object
    P[5, :3, 3] = at(12.0, 38.0, 400.0)                                    # in front of the bare wall
    render, skipped = TG.canvases(ops, v, f, P, np.tile(cam, (8, 1)), hw, (0, 0))
    assert skipped.sum() == 0
    z = np.where(render[true] > 0, render[true], np.inf).min(0)
    obs = np.where(np.isfinite(z), z, 460.0).astype(np.float32)[None]
    return dict(P=P, render=render, obs=obs, true=true, v=v, f=f, cam=cam, hw=hw)


def run(ops, render, obs, frame, flagged, thresholds, order_by=None, unit=1.0):
    """Evidence, order (the restatement's: the order is an INPUT of the kernel) and selection through ``ops``."""
    ev = evidence(ops, render, obs, frame, unit, TAU)
    key = V.scores(ev["counts"], False)[0]
    order, start = V.default_order(key, ev["counts"], frame, len(obs)) if order_by is None else V.key_order(order_by, frame, len(obs))
    st, fr = select(ops, ev, order, start, flagged, thresholds, render.shape[1:])
    return st, fr


def check_known_answers(ops):
    s = truth_scene(ops)
    render, obs, true = s["render"], s["obs"], s["true"]
    one, two = np.zeros(2, np.int32), np.array([0, 1], np.int32)
    twice = render[[1, 1]]
    # the same pose twice in one frame: the first is kept, the second is explained already
    ref = V.verify(twice, obs, one, 1.0, TAU, None, None, *DEFAULTS)
    assert ref["status"].tolist() == [0, 3] and ref["fresh"][1] == 0 and ref["fresh"][0] == ref["counts"][0, 2] > 100
    got = run(ops, twice, obs, one, None, DEFAULTS)
    assert got[0].tolist() == [0, 3] and np.array_equal(got[1], ref["fresh"])
    # ... in two different frames: both kept
    both = np.concatenate([obs, obs])
    ref = V.verify(twice, both, two, 1.0, TAU, None, None, *DEFAULTS)
    assert ref["status"].tolist() == [0, 0] and ref["fresh"][0] == ref["fresh"][1] > 100
    got = run(ops, twice, both, two, None, DEFAULTS)
    assert got[0].tolist() == [0, 0] and np.array_equal(got[1], ref["fresh"])
    # a pose wholly behind the measured wall: every pixel occluded, status 1
    wall = np.full_like(obs, 300.0)
    ref = V.verify(render[1:2], wall, one[:1], 1.0, TAU, None, None, *DEFAULTS)
    assert ref["status"].tolist() == [1] and ref["counts"][0, 3] == ref["counts"][0, 0] > 100
    assert run(ops, render[1:2], wall, one[:1], None, DEFAULTS)[0].tolist() == [1]
    # a pose floating in front of it: every pixel behind, fit 0; status 2 once min_inliers lets it through (status 1 otherwise)
    ref = V.verify(render[2:3], obs, one[:1], 1.0, TAU, None, None, 0, 0.5, 0.5)
    assert ref["status"].tolist() == [2] and ref["fit"].tolist() == [0.0] and ref["counts"][0, 4] == ref["counts"][0, 0] > 100
    assert run(ops, render[2:3], obs, one[:1], None, (0, 0.5, 0.5))[0].tolist() == [2]
    assert V.verify(render[2:3], obs, one[:1], 1.0, TAU, None, None, *DEFAULTS)["status"].tolist() == [1]
    assert run(ops, render[2:3], obs, one[:1], None, DEFAULTS)[0].tolist() == [1]
    # three true poses, a shifted duplicate of each, two unsupported poses: exactly the true ones are kept under the default order
    frame = np.zeros(8, np.int32)
    ref = V.verify(render, obs, frame, 1.0, TAU, None, None, *DEFAULTS)
    assert np.nonzero(ref["keep"])[0].tolist() == true, ref["status"]
    assert all(ref["status"][n] == 3 for n in (0, 4, 6)) and ref["status"][2] in (1, 2) and ref["status"][5] in (1, 2)
    got = run(ops, render, obs, frame, None, DEFAULTS)
    print(f"[verify known answers] status {got[0].tolist()} fresh {got[1].tolist()} fit {ref['fit'].round(3).tolist()}")
    assert np.array_equal(got[0], ref["status"]) and np.array_equal(got[1], ref["fresh"])
    # visited in the caller's order instead (the duplicates first): they are kept and explain the true poses
    key = np.array([9.0, 1.0, 0.0, 1.0, 9.0, 0.0, 9.0, 1.0])
    ref = V.verify(render, obs, frame, 1.0, TAU, None, None, 12, 0.5, 0.9, order_by=key)
    assert np.nonzero(ref["keep"])[0].tolist() == [0, 4, 6] and all(ref["status"][n] == 3 for n in true)
    got = run(ops, render, obs, frame, None, (12, 0.5, 0.9), order_by=key)
    assert np.array_equal(got[0], ref["status"]) and np.array_equal(got[1], ref["fresh"])


# ---------------------------------------------------------------------------------------------------------------- the module
def _same_result(out, ref):
    return (np.array_equal(_np(out["status"]), ref["status"]) and np.array_equal(_np(out["fresh"]), ref["fresh"])
            and np.array_equal(_np(out["counts"]), ref["counts"]) and np.array_equal(_np(out["order"]), ref["order"])
            and np.array_equal(_np(out["frame_start"]), ref["frame_start"]) and np.array_equal(_np(out["keep"]), ref["keep"])
            and all(np.array_equal(_np(out[k]), ref[k]) for k in ("score", "fit", "sil")) and out["score"].dtype == torch.float64
            and out["status"].dtype == torch.int32 and out["keep"].dtype == torch.bool)


def check_modules(ops, monkeypatch):
    """verify_poses under strict mode takes no library branch and gives the restatement's result from the renders of
    ``ops.render_depth``; so do its library statements (``policy.disable_fused``, and CPU tensors on the GPU box); metres with
    depth_unit = 1000; flagged instances; PoseVerifier; the argument checks."""
    from sam6d_amd import policy
    from sam6d_amd.pem import verify
    s = truth_scene(ops)
    hw, cam, P = s["hw"], s["cam"], s["P"].copy()
    tv, tf = TG._mesh("torus")
    meshes = [(s["v"], s["f"]), (tv, tf)]
    obj = [0, 0, 0, 1, 0, 0, 0, 0]                                         # the second true pose is verified as a torus
    frame = np.array([0, 0, 1, 0, 1, 0, 1, 0], np.int32)
    rs = np.random.RandomState(4)
    obs = np.concatenate([s["obs"], s["obs"] + rs.uniform(-9, 9, s["obs"].shape).astype(np.float32)])
    obs[1][rs.uniform(size=obs[1].shape) < 0.1] = 0.0
    masks = np.roll(s["render"] > 0, 1, axis=1)
    render = s["render"].copy()
    render[3] = TG.canvases(ops, tv, tf, P[3:4], cam[None], hw, (0, 0))[0][0]
    dev = _t(np.zeros(1, np.float32)).device                               # the host under the emulator fixture
    Rm, tm = _t(P[:, :3, :3]), _t(P[:, :3, 3])
    K = np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1]], np.float64)
    for with_masks, key in ((False, None), (True, None), (False, np.arange(8.0) % 3)):
        m = masks if with_masks else None
        ref = V.verify(render, obs, frame, 1.0, TAU, m, np.zeros(8, np.uint8), *DEFAULTS, order_by=key)
        kw = dict(masks=None if m is None else _t(m), frame_index=frame, order_by=key)
        policy.reset_library_branch_hits()
        with policy.use(strict="1"):
            out = verify.verify_poses(meshes, obj, Rm, tm, _t(obs), K, **kw)
        assert not policy.library_branch_hits()
        assert _same_result(out, ref), (out["status"], ref["status"], out["order"], ref["order"])
        with policy.use(disable_fused="verify_evidence,verify_select"):
            lib = verify.verify_poses(meshes, obj, Rm, tm, _t(obs), K, **kw)
        assert _same_result(lib, ref)
        if dev.type == "cuda":                                             # CPU tensors: the library statements on the kernel's renders
            cpu = verify.verify_poses(meshes, obj, Rm.cpu(), tm.cpu(), torch.from_numpy(obs), K, masks=None if m is None else torch.from_numpy(m),
                                      frame_index=frame, order_by=key,
                                      render=dict(depth=torch.from_numpy(render), skipped=torch.zeros(8, dtype=torch.int32)))
            assert _same_result(cpu, ref) and not cpu["status"].is_cuda
    assert len(set(ref["status"].tolist())) >= 2
    # disable_fused really routes to the library statements: the ops are made to raise
    def boom(*a, **k):
        raise AssertionError("the kernel path ran although policy.disable_fused names it")
    with monkeypatch.context() as mp, policy.use(disable_fused="verify_evidence,verify_select"):
        mp.setattr(ops, "verify_evidence", boom)
        mp.setattr(ops, "verify_select", boom)
        assert _same_result(verify.verify_poses(meshes, obj, Rm, tm, _t(obs), K, frame_index=frame, order_by=np.arange(8.0) % 3), ref)
    # metres against millimetre meshes: t and depth are converted by one float32 multiply each
    t_m, obs_m = (P[:, :3, 3] / np.float32(1000)).astype(np.float32), (obs / np.float32(1000)).astype(np.float32)
    P2 = P.copy()
    P2[:, :3, 3] = t_m * np.float32(1000)
    r2 = np.stack([TG.canvases(ops, *meshes[obj[n]], P2[n:n + 1], cam[None], hw, (0, 0))[0][0] for n in range(8)])
    ref = V.verify(r2, obs_m, frame, 1000.0, TAU, None, np.zeros(8, np.uint8), *DEFAULTS)
    verifier = verify.PoseVerifier(meshes, device=dev, use_masks=False, depth_unit=1000.0)
    assert verifier.use_masks is False and isinstance(verifier.meshes[0], dict)
    out = verifier(obj, Rm, _t(t_m), _t(obs_m), K, frame_index=frame)
    assert _same_result(out, ref) and 0 < int(ref["keep"].sum()) < 8
    # flagged: a vertex nearer than znear (a skipped triangle), a pose that is not finite -> status 4, whatever else holds
    P3 = P.copy()
    P3[1, :3, 3] = (0.0, 0.0, 30.0)
    P3[7, 0, 0] = np.nan
    out = verify.verify_poses(meshes, obj, _t(P3[:, :3, :3]), _t(P3[:, :3, 3]), _t(obs), K, frame_index=frame)
    st = _np(out["status"])
    assert st[1] == 4 and st[7] == 4 and not _np(out["keep"])[[1, 7]].any() and (st[[0, 3]] != 4).all()
    # a single depth image, no frame_index, a (fx, fy, cx, cy) camera
    ref = V.verify(render, obs[:1], np.zeros(8, np.int32), 1.0, TAU, None, None, *DEFAULTS)
    assert _same_result(verify.verify_poses(meshes, obj, Rm, tm, _t(obs[0]), tuple(float(x) for x in cam)), ref)
    # the argument checks
    d = _t(obs)
    with pytest.raises(ValueError, match="frame_index"):
        verify.verify_poses(meshes, obj, Rm, tm, d, K, frame_index=[2] * 8)
    with pytest.raises(ValueError, match="object_index"):
        verify.verify_poses(meshes, [2] * 8, Rm, tm, d, K)
    with pytest.raises(TypeError, match="float32"):
        verify.verify_poses(meshes, obj, Rm, tm.double(), d, K)
    with pytest.raises(ValueError, match="depth_unit"):
        verify.verify_poses(meshes, obj, Rm, tm, d, K, depth_unit=0.0)
    with pytest.raises(ValueError, match="must be >= 0"):
        verify.verify_poses(meshes, obj, Rm, tm, d, K, tau=-1.0)
    with pytest.raises(ValueError, match="masks"):
        verify.verify_poses(meshes, obj, Rm, tm, d, K, masks=_t(masks[:3]))
    with pytest.raises(ValueError, match="order_by"):
        verify.verify_poses(meshes, obj, Rm, tm, d, K, order_by=[1.0, 2.0])
    with pytest.raises(ValueError, match="render"):
        verify.verify_poses(meshes, obj, Rm, tm, d, K, render=dict(depth=_t(render[:3]), skipped=_t(np.zeros(8, np.int32))))


def check_arguments(ops):
    """Wrong shapes and dtypes, an obs_index or an order out of range, an instance named twice are refused on the host; the entry
    points refuse bad sizes with -1 / -3 before any launch."""
    render, obs, oi, masks = scene(ops, (8, 16), 3, 2, with_masks=True)
    a = [_t(x) for x in (render, obs, oi)]
    with pytest.raises(RuntimeError, match="float"):
        ops.verify_evidence(a[0].double(), a[1], a[2], 1.0, TAU)
    with pytest.raises(RuntimeError, match="an int tensor"):
        ops.verify_evidence(a[0], a[1], a[2].long(), 1.0, TAU)
    with pytest.raises(ValueError, match="expected"):
        ops.verify_evidence(a[0], a[1][:, :4].contiguous(), a[2], 1.0, TAU)
    with pytest.raises(ValueError, match="expected"):
        ops.verify_evidence(a[0], a[1], a[2][:2].contiguous(), 1.0, TAU)
    with pytest.raises(ValueError, match="masks"):
        ops.verify_evidence(a[0], a[1], a[2], 1.0, TAU, _t(masks[:2]))
    with pytest.raises(RuntimeError, match="masks"):
        ops.verify_evidence(a[0], a[1], a[2], 1.0, TAU, _t(masks.astype(np.int32)))
    for unit, tau in ((0.0, TAU), (float("inf"), TAU), (1.0, -1.0), (1.0, float("nan"))):
        with pytest.raises(ValueError, match="depth_unit must be positive"):
            ops.verify_evidence(a[0], a[1], a[2], unit, tau)
    for bad_index in (2, -1):
        oob = a[2].clone()
        oob[1] = bad_index
        with pytest.raises(ValueError, match=r"obs_index must lie in \[0, 2\)"):
            ops.verify_evidence(a[0], a[1], oob, 1.0, TAU)
    ev = ops.verify_evidence(*a, 1.0, TAU)
    order, start = _t(np.array([0, 2, 1], np.int32)), _t(np.array([0, 2, 3], np.int64))
    sel = lambda **k: ops.verify_select(k.get("inlier", ev["inlier"]), k.get("counts", ev["counts"]), k.get("span", ev["span"]),   # noqa: E731
                                        k.get("order", order), k.get("start", start), k.get("flagged"), *k.get("th", DEFAULTS), *k.get("hw", (8, 16)))
    assert sel()[0].shape == (3,)
    with pytest.raises(ValueError, match=r"order must lie in \[0, 3\)"):
        sel(order=_t(np.array([0, 3, 1], np.int32)))
    with pytest.raises(ValueError, match="more than once"):
        sel(order=_t(np.array([0, 1, 1], np.int32)))
    with pytest.raises(ValueError, match="frame_start must rise"):
        sel(start=_t(np.array([0, 2, 2], np.int64)))
    with pytest.raises(ValueError, match="order names 4"):
        sel(order=_t(np.array([0, 1, 2, 0], np.int32)), start=_t(np.array([0, 2, 4], np.int64)))
    with pytest.raises(ValueError, match="words per instance"):
        sel(hw=(8, 8))
    with pytest.raises(ValueError, match="expected"):
        sel(counts=ev["counts"][:, :4].contiguous())
    with pytest.raises(ValueError, match="flagged"):
        sel(flagged=_t(np.zeros(2, np.uint8)))
    with pytest.raises(ValueError, match="must be >= 0"):
        sel(th=(12, -0.5, 0.5))
    with pytest.raises(RuntimeError, match="int64|Long|torch.int64"):
        sel(inlier=ev["inlier"].int())
    P = lambda t: t.data_ptr()                                             # noqa: E731
    fe = ops._fn("s6d_verify_evidence_f32", 14)
    c, w, sp = (torch.full(sh, 7, dtype=dt).cuda() for sh, dt in (((3, 8), torch.int32), ((3, 2), torch.int64), ((3, 2), torch.int32)))
    args = lambda N, M, H, W, unit=1.0, tau=TAU: (P(a[0]), P(a[1]), P(a[2]), None, N, M, H, W, unit, tau, P(c), P(w), P(sp), ops._stream())   # noqa: E731
    assert fe(*args(-1, 2, 8, 16)) == -1 and fe(*args(3, 0, 8, 16)) == -1 and fe(*args(3, 2, 0, 16)) == -1 and fe(*args(3, 2, 8, 0)) == -1
    assert fe(*args(3, 2, 8, 16, unit=0.0)) == -1 and fe(*args(3, 2, 8, 16, unit=float("nan"))) == -1 and fe(*args(3, 2, 8, 16, tau=-1.0)) == -1
    assert fe(*args(3, 2, 8, 16, tau=float("nan"))) == -1
    assert fe(*args(3, 2, 1 << 15, 1 << 14)) == -3 and fe(*args(3, 2, 46341, 46341)) == -3          # 2^29 pixels and more
    assert fe(None, P(a[1]), P(a[2]), None, 3, 2, 8, 16, 1.0, TAU, P(c), P(w), P(sp), ops._stream()) == -1
    assert fe(*args(0, 2, 8, 16)) == 0
    fs = ops._fn("s6d_verify_select", 18)
    st, fr = torch.full((3,), 7, dtype=torch.int32).cuda(), torch.full((3,), 7, dtype=torch.int32).cuda()
    sargs = lambda B, N, K, H, W, mi=12, mf=0.5, mr=0.5, inl=P(ev["inlier"]): (inl, P(ev["counts"]), P(ev["span"]), P(order), P(start), None, B, N, K, H,   # noqa: E731
                                                                            W, mi, mf, mr, None, P(st), P(fr), ops._stream())
    assert fs(*sargs(-1, 3, 3, 8, 16)) == -1 and fs(*sargs(2, -1, 3, 8, 16)) == -1 and fs(*sargs(2, 3, 4, 8, 16)) == -1
    assert fs(*sargs(2, 3, 3, 0, 16)) == -1 and fs(*sargs(2, 3, 3, 1 << 15, 1 << 14)) == -3
    assert fs(*sargs(2, 3, 3, 8, 16, mi=-1)) == -1 and fs(*sargs(2, 3, 3, 8, 16, mf=float("nan"))) == -1 and fs(*sargs(2, 3, 3, 8, 16, mr=-0.5)) == -1
    assert fs(*sargs(2, 3, 3, 8, 16, inl=None)) == -1 and fs(*sargs(2, 0, 0, 8, 16)) == 0
    fw = ops._fn("s6d_verify_select_workspace_bytes", 3)
    assert fw(2, 480, 640) == 0 and fw(2, 480, 641) == 2 * 4808 * 8 and fw(3, 8, 16) == 0 and fw(2, 0, 5) == -1 and fw(-1, 8, 16) == -1
    fl = ops._fn("s6d_set_verify_lds_words", 1)
    assert fl(-1) == -1 and fl(4801) == -1 and fl(1) == 0
    try:
        assert fw(3, 8, 16) == 3 * 2 * 8 and fw(3, 8, 8) == 0
        assert fs(*sargs(2, 3, 3, 8, 16)) == -1                            # the workspace is needed now, and NULL
    finally:
        assert fl(0) == 0
    torch.cuda.synchronize()
    assert all((x.cpu() == 7).all() for x in (c, w, sp, st, fr))


# ---------------------------------------------------------------------------------------------------------------- on the MI355X
@pytest.mark.parametrize("with_masks", [False, True])
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N", [1, 3, 5])
@pytest.mark.parametrize("hw", sorted(SIZES))
def test_evidence_vs_restatement(ops, hw, N, M, with_masks):
    check_evidence(ops, hw, N, M, with_masks)


def test_evidence_torus(ops):
    check_evidence(ops, (48, 64), 3, 2, True, "torus")


def test_evidence_hostile_pixels(ops):
    check_hostile(ops)


@pytest.mark.parametrize("lds_words", [0, 1])
def test_selection_vs_restatement(ops, lds_words):
    check_selection(ops, lds_words)


def test_known_answers(ops):
    check_known_answers(ops)


def test_arguments(ops):
    check_arguments(ops)


def test_modules(ops, monkeypatch):
    check_modules(ops, monkeypatch)
