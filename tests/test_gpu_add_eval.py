"""The ADD / ADD-S kernels (csrc/s6d_adderr.hip) and sam6d_amd.evaluation on top of them against the numpy restatement of
tests/add_ref.py: per-vertex values, maxima and both means EQUAL to its float32 mode; every per-vertex value within a derived
bound of its float64 mode; the mean within (V - 1) 2^-53 relative of fsum of the kernel's own values; an estimate alone has the
bits it has in the batch, two chunkings and the three sources-per-lane variants agree; ADD-S <= ADD on the bits; known answers;
hostile inputs; the argument checks; the library statement equal to the kernel.  bop_toolkit is not present; nothing here is
compared with it.  The bodies take `ops` so that tests/test_emu_add_eval.py runs them on the host build.

The bound (profiles/add_eval_margins.md), with u = 2^-24 and second-order terms covered by a factor 1 + 2^-20:
  position   the float32 statement X = ((r0 vx + r1 vy) + r2 vz) + t rounds three products and three sums; the first product passes
             through four roundings, every other term through fewer:  |fl(X) - X| <= 4 u (|r0 vx| + |r1 vy| + |r2 vz| + |t|)  per
             coordinate, p(P, v) = the Euclidean norm of the three, for each of the two points.
  distance   the distance D' of the two ROUNDED points differs from the exact D by at most p_e + p_g (triangle inequality); the
             float32 distance of the rounded points is within 3.5 u relative of D' (three differences, three products, two sums of
             non-negative terms: d2 within 5 u; the root halves that and rounds once: the diameter bound of tests/test_gpu_bop_gt.py):
             |a32_i - a64_i| <= p + 3.5 u (a64_i + p),  p = p_e(i) + p_g(i).
  minimum    min_j is 1-Lipschitz in the maximum norm, so it inherits the bound with the largest target term:
             |s32_i - s64_i| <= p + 3.5 u (s64_i + p),  p = p_e(i) + max_j p_g(j).
  mean       any summation order of V non-negative float64 terms is within (V - 1) 2^-53 relative of their exact sum (V - 1
             additions of two non-zero values, each rounding once; here a term passes through at most ceil(V / 256) + 8 of them):
             the mean is held to (V - 1) 2^-53 relative of fsum(values) / V.  At V = 1 and 2 both sides are exact.
None of these was chosen by looking at the kernels' output."""
import functools

import numpy as np
import pytest
import torch

from tests import add_ref as A
from tests import render_ref as R
from tests import test_gpu_bop_eval as TB
from tests import util

pytestmark = pytest.mark.gpu

SHAPES_V = (1, 2, 255, 256, 257, 513, 1000)
SHAPES_N = (1, 3)
RZ90 = np.array([[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from sam6d_amd import ops
    return ops


_t, _np = TB._t, TB._np


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def mesh(V):
    """The first V vertices of a torus of at least V vertices (tests/render_ref.py); V = 8 is the cube."""
    if V == 8:
        return R.cube(40.0)[0]
    n_minor = 25 if V <= 1000 else 65
    v = R.torus(-(-V // n_minor), n_minor)[0] if V > n_minor else R.torus(3, n_minor)[0]
    assert len(v) >= V
    return np.ascontiguousarray(v[:V])


def pose_pairs(N, seed):
    """Ground truths from render_ref.poses; estimate n turned by 0.03 (n + 1) rad about a seeded axis and moved by a few units, the
    last estimate of a batch of three an unrelated rotation."""
    gt = R.poses(N, seed=seed).astype(np.float64)
    rs = np.random.RandomState(seed)
    est = gt.copy()
    for n in range(N):
        est[n, :3, :3] = gt[n, :3, :3] @ _rot(rs.standard_normal(3), 0.03 * (n + 1))
        est[n, :3, 3] += np.round(rs.uniform(-6, 6, 3) * 16) / 16
    if N == 3:
        est[2, :3, :3] = R.rotations(1, seed + 50)[0]
    return est.astype(np.float32), gt.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(V, N):
    """Seeded inputs, both restatements and the bounds: computed once and only read."""
    v = mesh(V)
    est, gt = pose_pairs(N, seed=V + N)
    r32, r64 = A.errors(v, est, gt, np.float32), A.errors(v, est, gt, np.float64)
    return v, est, gt, r32, r64, A.bounds(v, est, gt, r64)


def run(ops, v, est, gt, per_vertex=True, which=("add", "adds")):
    out = ops.add_errors(_t(v), _t(est), _t(gt), per_vertex=per_vertex, which=which)
    torch.cuda.synchronize()
    return {k: None if x is None else _np(x) for k, x in out.items()}


F32_KEYS = ("add_per_vertex", "adds_per_vertex", "add_max", "adds_max")


def same(got, ref):
    return (all(np.array_equal(_bits(got[k]), _bits(ref[k])) for k in F32_KEYS)
            and all(np.array_equal(np.asarray(got[k], np.float64).view(np.uint64), np.asarray(ref[k], np.float64).view(np.uint64)) for k in ("add", "adds")))


def check_errors(ops, V, N):
    """Equal to the float32 restatement, within the derived bound of the float64 one, the mean against fsum, ADD-S <= ADD, and the
    determinism statements (docstring of this file)."""
    from sam6d_amd import _lib, evaluation
    v, est, gt, r32, r64, (ba, bs) = case(V, N)
    got = run(ops, v, est, gt)
    assert same(got, r32), {k: (got[k], r32[k]) for k in ("add", "adds", "add_max", "adds_max")}
    fa = float((np.abs(got["add_per_vertex"].astype(np.float64) - r64["add_per_vertex"]) / ba).max())
    fs = float((np.abs(got["adds_per_vertex"].astype(np.float64) - r64["adds_per_vertex"]) / bs).max())
    fm = 0.0
    for k in ("add", "adds"):
        fsum = A.mean_fsum(got[k + "_per_vertex"])                         # of the kernel's OWN per-vertex values
        err, lim = np.abs(got[k] - fsum), (V - 1) * 2.0 ** -53 * fsum
        assert (err[lim == 0] == 0).all()
        fm = max([fm] + (err[lim > 0] / lim[lim > 0]).tolist())
    print(f"[add eval V {V} N {N}] add {got['add'].tolist()} adds {got['adds'].tolist()} error over the bound: add {fa:.3f}, adds {fs:.3f}, "
          f"mean vs fsum {fm:.3f}")
    assert fa <= 1.0 and fs <= 1.0 and fm <= 1.0
    util.record_margin(f"add_eval_V{V}_N{N}", add_err_over_bound=fa, adds_err_over_bound=fs, mean_err_over_bound=fm, bound_ratio=1.0)
    assert (_bits(got["adds_per_vertex"]) <= _bits(got["add_per_vertex"])).all()          # pair (i, i) is a candidate
    assert (got["adds"] <= got["add"]).all() and (got["adds_max"] <= got["add_max"]).all()
    # without the per-vertex output (the workspace holds the values): the same means and maxima
    lean = run(ops, v, est, gt, per_vertex=False)
    assert lean["add_per_vertex"] is None and lean["adds_per_vertex"] is None
    assert all(np.array_equal(lean[k], got[k]) for k in ("add", "adds", "add_max", "adds_max"))
    # an estimate alone has the bits it has in the batch
    n = N - 1
    alone = run(ops, v, est[n:n + 1], gt[n:n + 1])
    assert all(np.array_equal(alone[k][0], got[k][n]) for k in got)
    # two chunkings over N (one estimate per call; all in one)
    for chunk_bytes in (1, 1 << 28):
        r = evaluation.add_errors(_t(v), _t(est), gt, chunk_bytes=chunk_bytes, per_vertex=True)
        assert same({k: _np(x) for k, x in r.items()}, r32)
    # the sources-per-lane variants of the all-pairs kernel
    try:
        for spl in (1, 2, 4):
            assert _lib.lib().s6d_set_adds_sources_per_lane(spl) == 0
            r = run(ops, v, est, gt, which=("adds",))
            assert np.array_equal(_bits(r["adds_per_vertex"]), _bits(r32["adds_per_vertex"])) and np.array_equal(r["adds"], r32["adds"]), spl
    finally:
        _lib.lib().s6d_set_adds_sources_per_lane(0)
    assert _lib.lib().s6d_set_adds_sources_per_lane(3) == -1


def check_known_answers(ops):
    """est == gt: zeros.  A pure integer translation (3k, 4k, 0): ADD exactly 5k.  The cube under Rz(90 deg): ADD-S and its maximum 0,
    ADD > 0; symmetry_residuals 0 there and > 0 for Rz(45 deg)."""
    from sam6d_amd import evaluation
    v = mesh(513)
    est, gt = pose_pairs(3, seed=11)
    got = run(ops, v, gt, gt)
    assert all((got[k] == 0).all() for k in got)
    vi = np.round(v).astype(np.float32)
    eye = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    moved = eye.copy()
    for n, k in enumerate((1.0, 7.0, 100.0)):
        moved[n, :3, 3] = (3 * k, 4 * k, 0.0)
    got = run(ops, vi, moved, eye)
    assert (got["add_per_vertex"] == np.array([5.0, 35.0, 500.0], np.float32)[:, None]).all()
    assert got["add"].tolist() == [5.0, 35.0, 500.0] and got["add_max"].tolist() == [5.0, 35.0, 500.0]
    cube = mesh(8)
    est = R.poses(2, seed=3).astype(np.float64)
    gt = (est @ RZ90).astype(np.float32)
    got = run(ops, cube, est.astype(np.float32), gt)
    assert (got["adds_per_vertex"] == 0).all() and (got["adds"] == 0).all() and (got["adds_max"] == 0).all()
    assert (got["add"] > 40).all() and (got["add_per_vertex"] > 40).all()
    syms = np.stack([np.eye(4), RZ90, np.eye(4)])
    syms[2, :3, :3] = _rot((0, 0, 1), np.pi / 4)
    res = evaluation.symmetry_residuals(_t(cube), syms, diameter=80.0 * np.sqrt(3.0))
    assert res["mean"][0] == 0 and res["max"][0] == 0 and res["mean"][1] == 0 and res["max"][1] == 0
    assert res["mean"][2] > 20 and res["max_fraction"][2] > 0.1 and np.array_equal(res["mean_fraction"], res["mean"] / (80.0 * np.sqrt(3.0)))


def check_hostile(ops):
    """A NaN and an inf in ONE estimate's pose: its means are +inf, the other estimates of the batch keep their bits.  A NaN
    vertex: every ADD-S and ADD mean is +inf (the vertex is a source), the other vertices' values are what they are without it as a
    target... with it: a NaN target never wins a minimum.  Duplicate vertices change no per-vertex value.  Nothing is NaN."""
    v, est, gt, r32, _, _ = case(513, 3)
    for bad_value, where in ((np.nan, (0, 1)), (np.inf, (1, 3)), (-np.inf, (2, 2)), (np.nan, (2, 3))):
        bad = est.copy()
        bad[(1,) + where] = bad_value
        got = run(ops, v, bad, gt)
        ref = A.errors(v, bad, gt, np.float32)
        assert same(got, ref) and not any(np.isnan(got[k]).any() for k in got)
        assert np.isposinf(got["add"][1]) and np.isposinf(got["adds"][1]) and np.isposinf(got["adds_max"][1])
        assert np.isposinf(got["adds_per_vertex"][1]).all() and np.isposinf(got["add_per_vertex"][1]).all()
        for n in (0, 2):
            assert all(np.array_equal(got[k][n], r32[k][n]) for k in got)
    bad = gt.copy()
    bad[0, 1, 1] = np.nan                                                  # in the ground truth
    got = run(ops, v, est, bad)
    assert np.isposinf(got["adds"][0]) and np.isposinf(got["add"][0]) and all(np.array_equal(got[k][1:], r32[k][1:]) for k in got)
    for k in (0, 300, 512):                                                # first tile, second tile, the tail tile
        vb = v.copy()
        vb[k, 1] = np.nan
        got = run(ops, vb, est, gt)
        ref = A.errors(vb, est, gt, np.float32)
        assert same(got, ref) and not any(np.isnan(got[key]).any() for key in got)
        assert np.isposinf(got["adds"]).all() and np.isposinf(got["add"]).all() and np.isposinf(got["adds_per_vertex"][:, k]).all()
        rest = np.arange(513) != k
        assert np.isfinite(got["adds_per_vertex"][:, rest]).all()
        # the nearest neighbour of the other sources may only have been the lost target: never nearer than before
        assert (_bits(got["adds_per_vertex"][:, rest]) >= _bits(r32["adds_per_vertex"][:, rest])).all()
    rs = np.random.RandomState(4)
    dup = np.concatenate([v, v[rs.randint(0, 513, 7)], v[-1:]])
    got = run(ops, dup, est, gt)
    assert np.array_equal(_bits(got["adds_per_vertex"][:, :513]), _bits(r32["adds_per_vertex"]))
    assert np.array_equal(_bits(got["add_per_vertex"][:, :513]), _bits(r32["add_per_vertex"])) and np.array_equal(got["adds_max"], r32["adds_max"])


def check_arguments(ops):
    """Wrong dtypes and shapes, V = 0 and N = 0 at the wrapper; the raw entry points' return codes before any launch."""
    v, est, gt, _, _, _ = case(257, 3)
    tv, te, tg = _t(v), _t(est), _t(gt)
    with pytest.raises(RuntimeError, match="float"):
        ops.add_errors(tv.double(), te, tg)
    with pytest.raises(RuntimeError, match="float"):
        ops.add_errors(tv, te, tg.double())
    with pytest.raises(ValueError, match="expected"):
        ops.add_errors(tv[:, :2].contiguous(), te, tg)
    with pytest.raises(ValueError, match="expected"):
        ops.add_errors(tv, te[:2].contiguous(), tg)
    with pytest.raises(ValueError, match="expected"):
        ops.add_errors(tv, te[:, :3].contiguous(), tg)
    with pytest.raises(ValueError, match="expected"):
        ops.add_errors(tv[:0].contiguous(), te, tg)                        # V = 0
    with pytest.raises(ValueError, match="which"):
        ops.add_errors(tv, te, tg, which=("mssd",))
    none = ops.add_errors(tv, te[:0].contiguous(), tg[:0].contiguous(), per_vertex=True)          # N = 0
    assert none["add"].shape == (0,) and none["adds_per_vertex"].shape == (0, 257) and none["adds"].dtype == torch.float64
    P = lambda t: t.data_ptr()                                             # noqa: E731
    pv, mean, top = torch.full((3, 257), 7.0).cuda(), torch.full((3,), 7.0, dtype=torch.float64).cuda(), torch.full((3,), 7.0).cuda()
    for name in ("s6d_pose_err_add_f32", "s6d_pose_err_adds_f32"):
        fn = ops._fn(name, 10)
        s = ops._stream()
        assert fn(P(tv), 0, P(te), P(tg), 3, P(pv), P(mean), P(top), None, s) == -1
        assert fn(P(tv), 257, P(te), P(tg), -1, P(pv), P(mean), P(top), None, s) == -1
        assert fn(None, 257, P(te), P(tg), 3, P(pv), P(mean), P(top), None, s) == -1
        assert fn(P(tv), 257, None, P(tg), 3, P(pv), P(mean), P(top), None, s) == -1
        assert fn(P(tv), 257, P(te), None, 3, P(pv), P(mean), P(top), None, s) == -1
        assert fn(P(tv), 257, P(te), P(tg), 3, P(pv), None, P(top), None, s) == -1
        assert fn(P(tv), 257, P(te), P(tg), 3, P(pv), P(mean), None, None, s) == -1
        assert fn(P(tv), 257, P(te), P(tg), 3, None, P(mean), P(top), None, s) == -1          # neither an output nor a workspace
        assert fn(P(tv), 70000, P(te), P(tg), 70000, P(pv), P(mean), P(top), None, s) == -3   # N V >= 2^31
        assert fn(None, 257, None, None, 0, None, None, None, None, s) == 0                   # N = 0: nothing is looked at
    assert ops._size("s6d_pose_err_adds_workspace_bytes", 3, 257) == 3 * 257 * 4
    assert ops._size("s6d_pose_err_adds_workspace_bytes", 70000, 70000) == -1 and ops._size("s6d_pose_err_adds_workspace_bytes", 3, 0) == -1
    torch.cuda.synchronize()
    assert (pv.cpu() == 7).all() and (mean.cpu() == 7).all() and (top.cpu() == 7).all()


def check_modules(ops, monkeypatch):
    """evaluation.add_errors under strict mode takes no library branch and returns the kernels' values; with S6D_BOP_EVAL=0 it takes
    the torch statement (the op is made to raise), which is EQUAL to the kernel: per-vertex values, maxima and means."""
    from sam6d_amd import evaluation as ev
    from sam6d_amd import policy
    v, est, gt, r32, _, _ = case(513, 3)

    def go(**kw):
        r = ev.add_errors(_t(v), _t(est), gt, per_vertex=True, **kw)
        torch.cuda.synchronize()
        return {k: None if x is None else _np(x) for k, x in r.items()}
    with policy.use(strict="1"):
        got = go()
        only = go(which=("adds",))
    assert not policy.library_branch_hits()
    assert same(got, r32) and only["add"] is None and only["add_per_vertex"] is None and np.array_equal(only["adds"], r32["adds"])
    assert ops.have("add_errors") and ops.have("adds_errors")

    def boom(*a, **k):
        raise AssertionError("the kernel path ran although bop_eval = 0")
    monkeypatch.setenv("S6D_BOP_EVAL", "0")
    monkeypatch.setattr(ops, "add_errors", boom)
    lib = go()
    small = go(chunk_bytes=16 * 513 * 5)                                   # five source rows at a time
    assert same(lib, r32) and same(small, r32)


# ---------------------------------------------------------------------------------------------------------------- on the MI355X
@pytest.mark.parametrize("N", SHAPES_N)
@pytest.mark.parametrize("V", SHAPES_V)
def test_add_errors_vs_restatement(ops, V, N):
    check_errors(ops, V, N)


def test_add_errors_several_source_blocks(ops):
    check_errors(ops, 4099, 2)


def test_known_answers(ops):
    check_known_answers(ops)


def test_hostile_inputs(ops):
    check_hostile(ops)


def test_arguments(ops):
    check_arguments(ops)


def test_modules(ops, monkeypatch):
    check_modules(ops, monkeypatch)
