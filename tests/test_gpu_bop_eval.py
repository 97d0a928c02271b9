"""The BOP pose-error kernels (csrc/s6d_boperr.hip, s6d_raster_depth_f32) and sam6d_amd.evaluation on top of them against the numpy
restatement of tests/bop_ref.py: MSSD / MSPD and the VSD pixel counts bit for bit against its float32 mode, within derived bounds
of its float64 mode (profiles/bop_eval_margins.md; none of them was chosen by looking at the kernels' output), known answers,
batch invariance, hostile inputs, the depth render against ops.render_views, and the argument checks.  bop_toolkit is not present;
nothing here is compared with it.  The bodies take `ops` so that tests/test_emu_bop_eval.py runs them on the host build.

Bounds, with u = 2^-24:
  MSSD   |m32 - m64| <= 10 sqrt(3) u C + 5 u m64,  C = max over poses, symmetries, vertices and rows of sum |r v| + |t|
  MSPD   |m32 - m64| <= 2 sqrt(2) (5 u P + 3 u X) + 4 u m64,  P = max of (f / Z)(1 + max(|X|, |Y|) / Z) (sum |r v| + |t|),
         X = max of |f X / Z| + |c|
  VSD    a pixel is undecided when Dg - Dt (or De - Dt) lies within 8 u (|D| + |Dt|) of delta, or |Dg - De| / scale within
         9 u (Dg + De) / scale of a tau; e_k may differ from the float64 value by undecided / union; the seeds below keep the
         undecided pixels under 2 % of the union (asserted on the restatement alone)."""
import functools

import numpy as np
import pytest
import torch

from tests import bop_ref as B
from tests import render_ref as R
from tests import test_gpu_render as TR
from tests import util

pytestmark = pytest.mark.gpu

ZNEAR = 1.0
DELTA = 15.0
TAUS10 = [np.float32(0.05 * k) for k in range(1, 11)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from sam6d_amd import ops
    return ops


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- MSSD / MSPD
@functools.lru_cache(maxsize=None)
def _pose_case(V, S, N):
    """Seeded inputs and both restatements, computed once and only read."""
    rs = np.random.RandomState(1000 * V + 10 * S + N)
    v = rs.uniform(-60, 60, (V, 3)).astype(np.float32)
    gt = B.seeded_poses(N, seed=V + S + N)
    est = gt.copy()
    for n in range(N):
        est[n, :3, :3] = gt[n, :3, :3] @ B.rotation(rs.standard_normal(3), 0.02 + 0.03 * n)
        est[n, :3, 3] += np.round(rs.uniform(-6, 6, 3) * 16) / 16
    gts = (gt[:, None] @ B.axis_symmetries(S)[None]).astype(np.float32)
    cams = np.stack([[572.4 + 7 * n, 573.6 - 5 * n, 325.3 + n, 242.0 - n] for n in range(N)]).astype(np.float32)
    est = est.astype(np.float32)
    return v, est, gts, cams, B.pose_errors(v, est, gts, cams, np.float32), B.pose_errors(v, est, gts, cams, np.float64)


def _pose_errors(ops, v, est, gts, cams):
    m3, m2 = ops.pose_errors(_t(v), _t(est), _t(gts), _t(cams))
    torch.cuda.synchronize()
    return _np(m3), _np(m2)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def check_pose_errors(ops, V, S, N):
    """Bit for bit the float32 restatement; within the derived bounds of the float64 one; an instance alone has the bits it has in
    the batch.  300 - 1500 units from the camera, the estimate a few degrees and units off."""
    v, est, gts, cams, r32, r64 = _pose_case(V, S, N)
    assert np.isfinite(r64["mssd"]).all() and np.isfinite(r64["mspd"]).all() and (r64["mssd"] > 0).all()
    m3, m2 = _pose_errors(ops, v, est, gts, cams)
    assert np.array_equal(_bits(m3), _bits(r32["mssd"])), (m3, r32["mssd"])
    assert np.array_equal(_bits(m2), _bits(r32["mspd"])), (m2, r32["mspd"])
    f3 = (np.abs(m3.astype(np.float64) - r64["mssd"]) / B.mssd_bound(r64)).max()
    f2 = (np.abs(m2.astype(np.float64) - r64["mspd"]) / B.mspd_bound(r64)).max()
    print(f"[bop pose errors V {V} S {S} N {N}] worst fraction of the bound: mssd {f3:.3f}, mspd {f2:.3f}")
    assert f3 <= 1.0 and f2 <= 1.0, (f3, f2)
    util.record_margin(f"bop_pose_errors_V{V}_S{S}_N{N}", mssd_err_over_bound=f3, mspd_err_over_bound=f2, bound_ratio=1.0)
    n = N - 2 if N > 1 else 0
    a3, a2 = _pose_errors(ops, v, est[n:n + 1], gts[n:n + 1], cams[n:n + 1])
    assert _bits(a3)[0] == _bits(m3)[n] and _bits(a2)[0] == _bits(m2)[n]


def check_pose_known_answers(ops):
    """est = gt: 0.  est = gt S_j: at most the bound (here exactly 0: the same float32 matrix).  A translation of d along one axis:
    MSSD within the bound of d."""
    v, est, gts, cams, _, r64 = _pose_case(257, 7, 5)
    m3, m2 = _pose_errors(ops, v, gts[:, 0].copy(), gts[:, :1].copy(), cams)
    assert (m3 == 0).all() and (m2 == 0).all()
    for j in (3, 6):
        m3, m2 = _pose_errors(ops, v, gts[:, j].copy(), gts, cams)
        assert (m3 <= B.mssd_bound(r64)).all() and (m2 <= B.mspd_bound(r64)).all(), (j, m3, m2)
    for axis in range(3):
        moved = gts[:, 0].copy()
        moved[:, axis, 3] += np.float32(8.0)                               # exact: the translations are multiples of 1/16
        assert np.array_equal(moved[:, axis, 3].astype(np.float64), gts[:, 0, axis, 3].astype(np.float64) + 8.0)
        ref = B.pose_errors(v, moved, gts[:, :1], cams, np.float64)
        m3, _ = _pose_errors(ops, v, moved, gts[:, :1].copy(), cams)
        assert (np.abs(m3.astype(np.float64) - 8.0) <= B.mssd_bound(ref)).all(), (axis, m3)


def check_pose_hostile(ops):
    v, est, gts, cams, _, _ = _pose_case(257, 7, 5)
    inf = np.float32(np.inf)
    # a vertex at Z <= 0: MSPD +inf, MSSD finite (instance 1 only)
    near = est.copy()
    near[1, :3, 3] = (0.0, 0.0, 20.0)
    assert (B._transform(near[1], v, np.float32)[2] <= 0).any()
    m3, m2 = _pose_errors(ops, v, near, gts, cams)
    ref = B.pose_errors(v, near, gts, cams, np.float32)
    assert m2[1] == inf and np.isfinite(m3).all() and np.isfinite(np.delete(m2, 1)).all()
    assert np.array_equal(_bits(m3), _bits(ref["mssd"])) and np.array_equal(_bits(m2), _bits(ref["mspd"]))
    # a NaN pose: +inf for both, the other instances untouched
    bad = est.copy()
    bad[3, 0, 0] = np.nan
    m3, m2 = _pose_errors(ops, v, bad, gts, cams)
    assert m3[3] == inf and m2[3] == inf and np.isfinite(np.delete(m3, 3)).all() and np.isfinite(np.delete(m2, 3)).all()
    bad = gts.copy()
    bad[2, :, 2, 3] = np.nan                                               # every symmetry of one ground truth
    m3, m2 = _pose_errors(ops, v, est, bad, cams)
    assert m3[2] == inf and m2[2] == inf and np.isfinite(np.delete(m3, 2)).all()
    # the maximum sits at the last vertex: in the last, partial wave
    for V in (65, 257):
        v, est, gts, cams, _, first = _pose_case(V, 1, 1)
        far = v.copy()
        far[-1] = 4 * v[first["arg"][0, 0]]                                # four times as far out as the vertex of the maximum
        r32, r64 = B.pose_errors(far, est, gts, cams, np.float32), B.pose_errors(far, est, gts, cams, np.float64)
        assert (r64["arg"] == V - 1).all()
        m3, m2 = _pose_errors(ops, far, est, gts, cams)
        assert np.array_equal(_bits(m3), _bits(r32["mssd"])) and np.array_equal(_bits(m2), _bits(r32["mspd"]))
    # the minimum is at the last symmetry
    v, est, gts, cams, _, _ = _pose_case(257, 7, 5)
    last = gts[:, 6].copy()
    last[:, 0, 3] += np.float32(0.5)
    r32 = B.pose_errors(v, last, gts, cams, np.float32)
    per_sym = np.stack([B.pose_errors(v, last, gts[:, j:j + 1], cams, np.float64)["mssd"] for j in range(7)], 1)
    assert (per_sym.argmin(1) == 6).all()
    m3, m2 = _pose_errors(ops, v, last, gts, cams)
    assert np.array_equal(_bits(m3), _bits(r32["mssd"])) and np.array_equal(_bits(m2), _bits(r32["mspd"]))


# ---------------------------------------------------------------------------------------------------------------- render_depth
H, W = TR.H, TR.W
CAM = np.array(TR.K, np.float32)


def _depth(ops, v, f, P, cams, h=H, w=W, znear=ZNEAR):
    out = ops.render_depth(_t(v), _t(f), _t(np.asarray(P, np.float32)), _t(np.asarray(cams, np.float32)), h, w, znear)
    torch.cuda.synchronize()
    return _np(out["depth"]), _np(out["skipped"])


def _views(ops, v, f, P, cam, znear=ZNEAR):
    out = ops.render_views(_t(v), _t(f), _t(TR._grey(v)), _t(np.asarray(P, np.float32)), *[float(x) for x in cam], H, W, TR.AMBIENT, TR.DIFFUSE, znear)
    torch.cuda.synchronize()
    return _np(out["depth"]), _np(out["skipped"])


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "torus":
        v, f, _ = R.torus(24, 24)
        return v, f, R.poses(3, seed=11)
    v, f, _ = R.cube()
    return v, f, R.poses(3, seed=3, t=(3.0, -2.0, 220.0))                  # every face is shared by a workgroup at 220 units


def check_render_depth(ops, name):
    """One camera for every view: the depth bits and the skipped counts of ops.render_views.  A camera per view: every view equals
    the render_views call with that camera.  The cube at 220 units takes the workgroup-per-triangle kernel, the 24 x 24 torus the
    lane-per-triangle one."""
    v, f, P = _mesh(name)
    want, wskip = _views(ops, v, f, P, CAM)
    got, skip = _depth(ops, v, f, P, np.tile(CAM, (3, 1)))
    assert (want > 0).sum() > 300
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(skip, wskip)
    cams = np.stack([[60.0 + 3 * t, 58.0 + 2 * t, 32.0 - t, 24.0 + t] for t in range(3)]).astype(np.float32)
    got, skip = _depth(ops, v, f, P, cams)
    for t in range(3):
        want, wskip = _views(ops, v, f, P[t:t + 1], cams[t])
        assert np.array_equal(got[t].view(np.uint32), want[0].view(np.uint32)) and skip[t] == wskip[0], t
    assert not np.array_equal(got[0], got[1])


def check_render_depth_skipped(ops):
    verts, faces, _, _, skipped = TR.HOSTILE["behind znear"]
    v, f = np.array(verts, np.float32), np.array(faces, np.int32)
    want, wskip = _views(ops, v, f, TR.EYE, CAM)
    got, skip = _depth(ops, v, f, TR.EYE, CAM[None])
    assert skip.tolist() == [skipped] == wskip.tolist() and np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- VSD
SIZES = {(1, 1): (60.0, 60.0, 0.0, 0.0), (37, 53): (60.0, 60.0, 26.0, 18.0), (48, 64): (60.0, 60.0, 32.0, 24.0)}
DEPTH_OFFSETS = (4.0, 10.0, -7.0, 24.0, 45.0)


def _vsd_scene(ops, hw, N, M, name="cube"):
    """Depths of a cube of side 80 (or the torus) at about 400 units from ``render_depth`` at perturbed poses, and M measured depth
    images: the ground-truth surface with a few units of noise, a wall behind, an occluder in front, 10 % missing."""
    h, w = hw
    cam = np.array(SIZES[hw], np.float32)
    v, f = (R.cube(40.0)[:2] if name == "cube" else R.torus(24, 24)[:2])
    t0 = (0.0, 0.0, 400.0) if hw == (1, 1) else (3.0, -2.0, 400.0)
    gt = R.poses(N, seed=7, t=t0).astype(np.float64)
    est = gt.copy()
    rs = np.random.RandomState(100 * h + 10 * N + M)
    for n in range(N):
        est[n, :3, :3] = gt[n, :3, :3] @ B.rotation(rs.standard_normal(3), 0.03)
        est[n, :3, 3] += (1.5 if hw != (1, 1) else 0.0, -1.0 if hw != (1, 1) else 0.0, DEPTH_OFFSETS[n])
    cams = np.tile(cam, (N, 1))
    de, se = _depth(ops, v, f, est, cams, h, w)
    dg, sg = _depth(ops, v, f, gt, cams, h, w)
    assert se.sum() == 0 and sg.sum() == 0
    test = np.full((M, h, w), 460.0, np.float32)
    for m in range(M):
        surf = dg[m % N]
        test[m] = np.where(surf > 0, surf + rs.uniform(-3, 3, (h, w)).astype(np.float32), test[m])
        if h > 1:
            test[m, h // 2 + 2 * m: h // 2 + 8, w // 2 - 3: w // 2 + 6 + m] = 300.0          # an occluder in front
            test[m][rs.uniform(size=(h, w)) < 0.1] = 0.0
    ti = (np.arange(N) % M).astype(np.int32)
    scale = np.full(N, 80.0 * np.sqrt(3.0), np.float32)
    return de, dg, test, ti, cams, scale


def _counts(ops, de, dg, test, ti, cams, delta, taus, scale):
    un, it, ge = ops.vsd_counts(_t(de), _t(dg), _t(test), _t(ti), _t(cams), delta, taus, _t(scale))
    torch.cuda.synchronize()
    return dict(union=_np(un).astype(np.int64), inter=_np(it).astype(np.int64), ge=_np(ge).astype(np.int64))


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("union", "inter", "ge"))


def check_vsd_counts(ops, hw, N, M, NT, name="cube"):
    """union, inter and ge exactly the float32 restatement's; the errors within undecided / union of the float64 restatement's,
    the undecided pixels at most 2 % of the union (a property of the inputs, asserted before the kernel is looked at); two runs
    give the same integers."""
    de, dg, test, ti, cams, scale = _vsd_scene(ops, hw, N, M, name)
    taus = TAUS10[:NT] if NT > 1 else [np.float32(0.05)]
    r32 = B.vsd_counts(de, dg, test, ti, cams, DELTA, taus, scale, np.float32)
    r64 = B.vsd_counts(de, dg, test, ti, cams, DELTA, taus, scale, np.float64)
    assert (r64["undecided"] <= 0.02 * r64["union"]).all(), (r64["undecided"], r64["union"])
    if hw != (1, 1):
        assert (r64["union"] > 40).all() and (r64["inter"] > 0).all() and (r64["inter"] < r64["union"]).any()
    got = _counts(ops, de, dg, test, ti, cams, DELTA, taus, scale)
    print(f"[bop vsd {hw} N {N} M {M} NT {NT} {name}] union {got['union'].tolist()} inter {got['inter'].tolist()} ge {got['ge'].tolist()} "
          f"undecided {r64['undecided'].tolist()}")
    assert _same(got, r32), (got, r32)
    e, e64 = B.vsd_errors(got), B.vsd_errors(r64)
    lim = np.where(r64["union"] > 0, r64["undecided"] / np.maximum(r64["union"], 1), 0.0)[:, None]
    assert (np.abs(e - e64) <= lim).all(), (e, e64, lim)
    assert _same(_counts(ops, de, dg, test, ti, cams, DELTA, taus, scale), got)


def check_vsd_known_answers(ops):
    de, dg, test, ti, cams, scale = _vsd_scene(ops, (48, 64), 3, 2)
    # est = gt: ge = 0, inter = union, error 0
    got = _counts(ops, dg, dg, test, ti, cams, DELTA, TAUS10, scale)
    assert (got["ge"] == 0).all() and np.array_equal(got["inter"], got["union"]) and (got["union"] > 0).all()
    assert (B.vsd_errors(got) == 0).all()
    # an empty union (nothing rendered; and everything occluded): errors of 1
    zero = np.zeros_like(dg)
    got = _counts(ops, zero, zero, test, ti, cams, DELTA, TAUS10, scale)
    assert (got["union"] == 0).all() and (B.vsd_errors(got) == 1).all()
    got = _counts(ops, de, dg, np.full_like(test, 100.0), ti, cams, DELTA, TAUS10, scale)
    assert (got["union"] == 0).all() and (B.vsd_errors(got) == 1).all()
    # an estimate moved in depth by more than max tau x scale: error 1
    shift = np.float32(1.05 * float(TAUS10[-1]) * float(scale[0]))
    moved = np.where(dg > 0, dg + shift, 0).astype(np.float32)
    got = _counts(ops, moved, dg, np.zeros_like(test), ti, cams, DELTA, TAUS10, scale)
    assert (got["inter"] > 0).all() and np.array_equal(got["ge"], np.repeat(got["inter"][:, None], 10, 1)) and (B.vsd_errors(got) == 1).all()


# ---------------------------------------------------------------------------------------------------------------- arguments
def check_arguments(ops):
    """Wrong dtypes and shapes, a test_index outside [0, M), more than 16 taus and N x S beyond 2^31 are refused: by the wrapper,
    or by the entry point with -1 / -3 before any launch."""
    from sam6d_amd import _lib
    v, est, gts, cams, _, _ = _pose_case(63, 2, 5)
    tv, te, tg, tc = _t(v), _t(est), _t(gts), _t(cams)
    with pytest.raises(RuntimeError, match="float"):
        ops.pose_errors(tv.double(), te, tg, tc)
    with pytest.raises(RuntimeError, match="float"):
        ops.pose_errors(tv, te, tg.double(), tc)
    with pytest.raises(ValueError, match="expected"):
        ops.pose_errors(tv, te[:4].contiguous(), tg, tc)
    with pytest.raises(ValueError, match="expected"):
        ops.pose_errors(tv, te, tg, tc[:, :3].contiguous())
    with pytest.raises(RuntimeError, match="4 dimensions"):
        ops.pose_errors(tv, te, tg[:, 0].contiguous(), tc)
    fn = ops._fn("s6d_pose_err_mssd_mspd_f32", 10)
    out = torch.full((5,), 7.0).cuda()
    P = lambda t: t.data_ptr()                                             # noqa: E731
    assert fn(P(tv), P(te), P(tg), P(tc), 63, 70000, 70000, P(out), P(out), ops._stream()) == -3          # N x S >= 2^31
    assert fn(P(tv), P(te), P(tg), P(tc), 0, 5, 2, P(out), P(out), ops._stream()) == -1
    assert fn(P(tv), P(te), P(tg), P(tc), 63, 5, 0, P(out), P(out), ops._stream()) == -1
    assert fn(None, P(te), P(tg), P(tc), 63, 5, 2, P(out), P(out), ops._stream()) == -1
    assert fn(P(tv), P(te), P(tg), P(tc), 63, 0, 2, P(out), P(out), ops._stream()) == 0
    torch.cuda.synchronize()
    assert (out.cpu() == 7).all()

    mv, mf, mP = _mesh("cube")
    cam3 = _t(np.tile(CAM, (3, 1)))
    with pytest.raises(RuntimeError, match="an int tensor"):
        ops.render_depth(_t(mv), _t(mf).long(), _t(mP), cam3, H, W, ZNEAR)
    with pytest.raises(ValueError, match="expected"):
        ops.render_depth(_t(mv), _t(mf), _t(mP), cam3[:2].contiguous(), H, W, ZNEAR)
    bad = _t(mf).clone()
    bad[3, 1] = len(mv)
    with pytest.raises(ValueError, match="face indices"):
        ops.render_depth(_t(mv), bad, _t(mP), cam3, H, W, ZNEAR)
    with pytest.raises(_lib.S6DError, match="s6d_raster_depth_f32"):
        ops.render_depth(_t(mv), _t(mf), _t(mP), cam3, H, W, -1.0)
    assert ops._size("s6d_raster_depth_workspace_bytes", 3, 12, H, W) == 3 * 12 * 4 + 8          # the list and its length
    assert ops._size("s6d_raster_depth_workspace_bytes", 3, 12, 40000, W) == -1

    de, dg, test, ti, cams, scale = _vsd_scene(ops, (37, 53), 3, 2)
    a = [_t(x) for x in (de, dg, test, ti, cams)]
    call = lambda *x, taus=TAUS10: ops.vsd_counts(*x, DELTA, taus, _t(scale))          # noqa: E731
    with pytest.raises(RuntimeError, match="float"):
        call(a[0].double(), *a[1:])
    with pytest.raises(RuntimeError, match="an int tensor"):
        call(*a[:3], a[3].long(), a[4])
    with pytest.raises(ValueError, match="expected"):
        call(a[0], a[1][:2].contiguous(), *a[2:])
    with pytest.raises(ValueError, match="expected"):
        call(a[0], a[1], a[2][:, :30].contiguous(), *a[3:])
    for bad_index in (2, -1):
        oob = a[3].clone()
        oob[1] = bad_index
        with pytest.raises(ValueError, match=r"test_index must lie in \[0, 2\)"):
            call(*a[:3], oob, a[4])
    with pytest.raises(_lib.S6DError, match="invalid argument"):
        call(*a, taus=[0.01 * k for k in range(17)])
    with pytest.raises(_lib.S6DError, match="invalid argument"):
        call(*a, taus=[])


# ---------------------------------------------------------------------------------------------------------------- the module
def check_modules(ops, monkeypatch):
    """evaluation.mssd / mspd / vsd under strict mode take no library branch and return the kernels' values; with S6D_BOP_EVAL=0
    they take the torch statements (the ops are made to raise) and agree within the bounds."""
    from sam6d_amd import evaluation as ev
    from sam6d_amd import policy
    V, S, N = 257, 7, 5
    v, est, gts, cams, r32, r64 = _pose_case(V, S, N)
    gt = B.seeded_poses(N, seed=V + S + N)
    syms = B.axis_symmetries(S)
    test = _vsd_scene(ops, (48, 64), 3, 2)[2]
    cube_v, cube_f = R.cube(40.0)[:2]
    vgt = R.poses(3, seed=7, t=(3.0, -2.0, 400.0)).astype(np.float64)
    vest = vgt.copy()
    vest[:, 2, 3] += (4.0, 10.0, -7.0)
    vcams = np.tile(np.array(SIZES[(48, 64)], np.float32), (3, 1))
    vti = np.array([0, 1, 0], np.int32)
    diameter = 80.0 * np.sqrt(3.0)

    def run():
        m3 = ev.mssd(_t(v), _t(est), gt, syms)
        m2 = ev.mspd(_t(v), _t(est), gt, syms, _t(cams))
        r = ev.vsd(_t(cube_v), _t(cube_f), _t(vest.astype(np.float32)), vgt, _t(vcams), _t(test), vti, diameter)
        torch.cuda.synchronize()
        return _np(m3), _np(m2), r
    with policy.use(strict="1"):
        m3, m2, r = run()
    assert not policy.library_branch_hits()
    assert np.array_equal(_bits(m3), _bits(r32["mssd"])) and np.array_equal(_bits(m2), _bits(r32["mspd"]))
    assert not r["unrenderable"].any() and (r["union"] > 40).all() and r["errors"].shape == (3, 10)
    de, _ = _depth(ops, cube_v, cube_f, vest, vcams)
    dg, _ = _depth(ops, cube_v, cube_f, vgt, vcams)
    taus = [np.float32(t) for t in ev.BOP19["vsd_taus"]]
    scale = np.full(3, diameter, np.float32)
    r32v = B.vsd_counts(de, dg, test, vti, vcams, DELTA, taus, scale, np.float32)
    assert _same(r, r32v) and np.array_equal(r["errors"], B.vsd_errors(r32v))
    wide = B.vsd_counts(de, dg, test, vti, vcams, DELTA, taus, scale, np.float64, input_rel=8 * B.U)
    assert (wide["undecided"] <= 0.02 * wide["union"]).all()

    def boom(*a, **k):
        raise AssertionError("the kernel path ran although bop_eval = 0")
    kernels = {name: getattr(ops, name) for name in ("pose_errors", "render_depth", "vsd_counts")}
    monkeypatch.setenv("S6D_BOP_EVAL", "0")
    for name in kernels:
        monkeypatch.setattr(ops, name, boom)
    l3, l2, lr = run()
    assert (np.abs(l3.astype(np.float64) - r64["mssd"]) <= B.mssd_bound(r64)).all()
    assert (np.abs(l2.astype(np.float64) - r64["mspd"]) <= B.mspd_bound(r64)).all()
    lim = (wide["undecided"] / wide["union"])[:, None]
    assert (np.abs(lr["errors"] - r["errors"]) <= 2 * lim).all(), (lr["errors"], r["errors"], lim)
    assert (np.abs(lr["union"] - r["union"]) <= wide["undecided"]).all()
    # a pair with a triangle behind znear is reported and given error 1
    monkeypatch.setenv("S6D_BOP_EVAL", "1")
    for name, fn in kernels.items():
        monkeypatch.setattr(ops, name, fn)
    close = vest.astype(np.float32).copy()
    close[1, 2, 3] = 30.0
    r = ev.vsd(_t(cube_v), _t(cube_f), _t(close), vgt, _t(vcams), _t(test), vti, diameter)
    assert r["unrenderable"].tolist() == [False, True, False] and (r["errors"][1] == 1).all() and (r["errors"][0] < 1).any()


# ---------------------------------------------------------------------------------------------------------------- on the MI355X
@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("S", [1, 2, 7, 315])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 257, 1000])
def test_pose_errors_vs_restatement(ops, V, S, N):
    check_pose_errors(ops, V, S, N)


def test_pose_known_answers(ops):
    check_pose_known_answers(ops)


def test_pose_hostile_inputs(ops):
    check_pose_hostile(ops)


@pytest.mark.parametrize("name", ["cube", "torus"])
def test_render_depth_equals_render_views(ops, name):
    check_render_depth(ops, name)


def test_render_depth_counts_skipped(ops):
    check_render_depth_skipped(ops)


@pytest.mark.parametrize("NT", [1, 10])
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N", [1, 3, 5])
@pytest.mark.parametrize("hw", sorted(SIZES))
def test_vsd_counts_vs_restatement(ops, hw, N, M, NT):
    check_vsd_counts(ops, hw, N, M, NT)


def test_vsd_counts_torus(ops):
    check_vsd_counts(ops, (48, 64), 3, 2, 10, "torus")


def test_vsd_known_answers(ops):
    check_vsd_known_answers(ops)


def test_arguments(ops):
    check_arguments(ops)


def test_modules(ops, monkeypatch):
    check_modules(ops, monkeypatch)
