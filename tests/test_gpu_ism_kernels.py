"""The ISM scoring kernels (csrc/s6d_ism.hip) one by one through sam6d_amd.ops, on ties, exact zeros, cancelling rows, points on and
behind the camera plane and edge shapes, against the plain restatements of tests/ism_ref.py (translations: oracle.ism.
mean_translation_pinned).

Tolerance: where a value is compared at all it is 2e-6 absolute, the bound tests/test_gpu_ism.py already holds these kernels to (the
3-term bf16 split of patch_scores_kernel costs about 3e-7 per unit-vector cosine; C <= 256 here).  Every measured worst case is
printed and recorded with tests.util.record_margin.  Integers, and everything a docstring calls exact, are compared with array_equal.
The bodies are check_* functions that take `ops`: tests/test_emu_ism_kernels.py runs them on the host build of the kernel source."""
import functools

import numpy as np
import pytest
import torch

from oracle import ism as oism
from tests import ism_ref
from tests.util import record_margin

pytestmark = pytest.mark.gpu

TOL = 2e-6
F32 = np.float32
KCAM = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from sam6d_amd import ops
    return ops


def _margin(test, **kw):
    print(f"[margin] {test}: " + ", ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()))
    record_margin(test, **kw)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _np(t):
    return t.cpu().numpy()


def _raises(fn, *a, **k):
    """The C ABI answers with an error code, which the binding raises: never a result."""
    from sam6d_amd import _lib
    with pytest.raises(_lib.S6DError):
        fn(*a, **k)


# ================================================================================================================= pairwise_cosine
COSINE_SHAPES = [(1, 1, 16), (16, 16, 32), (17, 15, 64), (5, 33, 256), (37, 135, 128)]


def _cosine_data(P, R, C):
    rng = np.random.default_rng(100 * P + R)
    return rng.standard_normal((P, C)).astype(F32), rng.standard_normal((R, C)).astype(F32)


def _cosine(ops, q, r):
    return _np(ops.pairwise_cosine(_dev(q), _dev(r)))


def check_cosine(ops, P, R, C):
    """pairwise_cosine_kernel at (P, R, C) against cosine_ref within 2e-6, and one call per hostile row: a zero query row / a zero
    reference row give exactly 0.0 across the row / column (0 * 1e12 * x); a reference row equal to a query row gives a value in
    [1 - 2e-6, 1] and nothing exceeds 1; a negated copy gives exactly 0.0 (the lower clamp); a row shorter than F.normalize's eps
    is divided by the eps, not by its length."""
    q, r = _cosine_data(P, R, C)
    worst = 0.0

    def run(q, r):
        nonlocal worst
        out = _cosine(ops, q, r)
        assert out.shape == (P, R) and out.dtype == F32
        worst = max(worst, float(np.abs(out - ism_ref.cosine_ref(q, r)).max()))
        assert out.min() >= 0.0 and out.max() <= 1.0
        return out
    run(q, r)
    q0 = q.copy(); q0[P - 1] = 0
    assert np.array_equal(run(q0, r)[P - 1], np.zeros(R, F32))
    r0 = r.copy(); r0[R - 1] = 0
    assert np.array_equal(run(q, r0)[:, R - 1], np.zeros(P, F32))
    assert np.array_equal(run(q0, r0), np.where(np.arange(P)[:, None] == P - 1, 0, run(q, r0)))
    rc = r.copy(); rc[R // 2] = q[P // 2]
    same = run(q, rc)[P // 2, R // 2]
    assert 1.0 - TOL <= same <= 1.0, same
    rn = r.copy(); rn[R - 1] = -q[0]
    assert run(q, rn)[0, R - 1] == 0.0
    # rows shorter than F.normalize's eps: |row| 2^-50 ~ 5e-15 < 1e-12, so the quotient is q.r / (1e-12 |r|) ~ 5e-3 cos, not cos
    qt = q.copy(); qt[0] = np.ldexp(q[0], -50)
    rt = r.copy(); rt[R - 1] = q[0]
    tiny = run(qt, rt)[0, R - 1]
    rt = r.copy(); rt[0] = np.ldexp(q[P - 1], -50)
    tiny = max(tiny, run(q, rt)[P - 1, 0])
    assert 0.0 < tiny < 0.1, tiny
    _margin(f"ism_kernels.cosine[{P}-{R}-{C}]", max_abs_err=worst, tol=TOL, one_minus_self_cosine=float(1.0 - same))
    assert worst <= TOL, worst


def check_cosine_power_of_two_scaling(ops, P, R, C):
    """Query row i times 2^k_i and reference row j times 2^m_j (k, m in [-30, 30]) leave every output bit unchanged: the squares,
    the fma chain, the square root of an even power, the reciprocal and the two products all scale exactly (no value leaves the
    normal range: |x| in [1e-6, 6] here, squares down to 2^-100)."""
    q, r = _cosine_data(P, R, C)
    rng = np.random.default_rng(7)
    k, m = rng.integers(-30, 31, P), rng.integers(-30, 31, R)
    k[0], m[R - 1] = -30, 30
    base = _cosine(ops, q, r)
    scaled = _cosine(ops, np.ldexp(q, k[:, None]).astype(F32), np.ldexp(r, m[:, None]).astype(F32))
    assert np.array_equal(base, scaled)


def check_cosine_row_independence(ops):
    """Row p of the (37, 135, 128) call equals the P = 1 call on that row bit for bit (a tile's 16 rows, the clamped rows past P and
    the wave a tile lands on do not reach a row's arithmetic)."""
    q, r = _cosine_data(37, 135, 128)
    full = _cosine(ops, q, r)
    for p in (0, 15, 16, 31, 32, 36):
        assert np.array_equal(_cosine(ops, q[p:p + 1], r), full[p:p + 1]), p


@pytest.mark.parametrize("P,R,C", COSINE_SHAPES)
def test_pairwise_cosine_vs_reference_and_hostile_rows(ops, P, R, C):
    check_cosine(ops, P, R, C)
    check_cosine_power_of_two_scaling(ops, P, R, C)


def test_pairwise_cosine_rows_are_independent(ops):
    check_cosine_row_independence(ops)


# ================================================================================================================= semantic_select
SELECT_SHAPES = [(1, 1, 1), (5, 3, 63), (4, 2, 64), (7, 3, 65), (3, 2, 255), (6, 4, 256)]


def _select(ops, s, topk):
    bs, bo, bt = ops.semantic_select(_dev(s), topk)
    assert bo.dtype == torch.int32 and bt.dtype == torch.int32
    return _np(bs), _np(bo).astype(np.int64), _np(bt).astype(np.int64)


def _check_select(ops, s, topk, what):
    bs, bo, bt = _select(ops, s, topk)
    es, eo, et = ism_ref.semantic_select_ref(s, topk)
    assert np.array_equal(bo, eo), (what, topk, bo, eo)
    assert np.array_equal(bt, et), (what, topk, bt, et)
    err = float(np.abs(bs - es).max())
    assert err < 1e-6, (what, topk, err)
    return err, bo, bt


def check_select(ops, P, O, T):
    """semantic_select_kernel on scores drawn from {0, 1/16, ..., 1}: ties inside every row and between objects, every partial sum
    exact in float32.  Object and template exact (first object on equal means, first template on equal scores), the score within
    1e-6 (one float32 division), for topk = 1, 5 and T."""
    s = (np.random.default_rng(10 * T + O).integers(0, 17, (P, O, T)) / 16.0).astype(F32)
    if T > 1:
        assert (np.sort(s, -1)[..., -1] == np.sort(s, -1)[..., -2]).any()          # duplicated row maxima are in the data
    worst = max(_check_select(ops, s, topk, (P, O, T))[0] for topk in (1, 5, T))
    _margin(f"ism_kernels.select[{P}-{O}-{T}]", max_abs_err=worst, tol=1e-6)


def check_select_ties(ops):
    """Constructed ties at T = 130 (three register slots per lane):
      p0  object 1's row is a permutation of object 0's (its maximum earlier), object 2 the same values again: equal means, object 0
          wins and the template is the first maximum of object 0's OWN row
      p1  all zero: object 0, template 0, score 0
      p2  the maximum at t = 5 and t + 64 = 69 (same lane, next register slot): template 5
      p3  the maximum at t = 70 and 71 (neighbouring lanes): template 70
      p4  the winning object is the LAST one, its maximum duplicated at 63 | 64 (last lane of slot 0, first lane of slot 1)."""
    O, T = 3, 130
    rng = np.random.default_rng(5)
    s = (rng.integers(0, 12, (5, O, T)) / 16.0).astype(F32)
    s[0, 0, 100], s[0, 0, 17] = 1.0, 0.875
    s[0, 1] = s[0, 0][::-1]
    s[0, 2] = np.roll(s[0, 0], 37)
    s[1] = 0
    s[2, 1, 5] = s[2, 1, 69] = 0.9375
    s[3, 0, 70] = s[3, 0, 71] = 1.0
    s[4, 2, 63] = s[4, 2, 64] = 1.0
    s[4, 2, 1] = 0.9375
    for topk in (1, 5, T):
        _, bo, bt = _check_select(ops, s, topk, "ties")
        bs = _select(ops, s, topk)[0]
        assert bo[0] == 0 and bt[0] == 100
        assert (bo[1], bt[1], bs[1]) == (0, 0, 0.0)
        if topk == 1:
            assert (bo[2], bt[2]) == (1, 5) and (bo[3], bt[3]) == (0, 70) and (bo[4], bt[4]) == (2, 63)


def check_select_refused(ops):
    _raises(ops.semantic_select, _dev(np.zeros((2, 1, 257), F32)), 5)


@pytest.mark.parametrize("P,O,T", SELECT_SHAPES)
def test_semantic_select_on_tied_scores(ops, P, O, T):
    check_select(ops, P, O, T)


def test_semantic_select_tie_rules(ops):
    check_select_ties(ops)
    check_select_refused(ops)


# ==================================================================================================================== patch_scores
# (S, N1, N2, C) -> seed of the data.  The seeds are chosen (on the CPU, from the float64 reference alone) so that the premise of the
# bit-for-bit comparisons holds; check_patch_scores asserts that premise on every case.
PATCH_SHAPES = {(1, 1, 1, 32): 1, (2, 16, 16, 32): 0, (3, 17, 15, 64): 0, (2, 32, 256, 64): 0, (3, 33, 255, 64): 0,
                (2, 256, 256, 32): 1, (3, 257, 250, 64): 0, (2, 300, 1, 32): 0}
THRED = 0.5


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _patch_data(S, N1, N2, C, seed):
    """S proposals against a (2, 3, N2, C) store: unit reference rows, query row i = unit(0.7 ref row (i mod N2) + 0.3 unit noise) (the
    construction of sam6d_amd.utils.synth.ism_inputs: column maxima on both sides of the threshold), about 30 % of the query rows and
    of the reference rows zeroed.  -> q (S,N1,C), store, obj (S), tmpl (S), float32 / int32."""
    rng = np.random.default_rng(seed)
    store = _unit(rng.standard_normal((2, 3, N2, C)))
    store *= rng.random((2, 3, N2, 1)) > 0.3
    obj, tmpl = rng.integers(0, 2, S), rng.integers(0, 3, S)
    q = _unit(0.7 * store[obj, tmpl][:, np.arange(N1) % N2] + 0.3 * _unit(rng.standard_normal((S, N1, C))))
    q *= rng.random((S, N1, 1)) > 0.3
    return q.astype(F32), store.astype(F32), obj.astype(np.int32), tmpl.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _patch_constructions(N1, N2, C, seed):
    """Four proposals against a (1, 4, N2, C) store (template s belongs to proposal s):
      a  every query row zero
      b  the chosen template all zero
      c  about a quarter of the query rows are (+a, -a, 0, ...) at two random channels, a = float32(1 / sqrt(2)): non-zero elements that
         sum to exactly 0 in ANY order, so the reference counts the row out of nnz although its similarities are non-zero
      d  nothing zeroed; all rows in the positive orthant with the last channel 0, except reference column j* = min(1, N2 - 1), which is
         anti-correlated with EVERY query row (a negative column maximum: valid, not visible), and query row i* = N1 // 2, which is
         anti-correlated with every reference column (a negative row maximum enters the sum)."""
    rng = np.random.default_rng(seed + 1)
    store = _unit(rng.standard_normal((1, 4, N2, C)))
    store *= rng.random((1, 4, N2, 1)) > 0.3
    mix = np.array([0.7, 0.7, 0.5, 0.7]).reshape(4, 1, 1)      # c: weaker matches, so that its score stays below the upper clamp
    q = _unit(mix * store[0][:, np.arange(N1) % N2] + (1 - mix) * _unit(rng.standard_normal((4, N1, C))))
    q *= rng.random((4, N1, 1)) > 0.3
    q[0] = 0
    store[0, 1] = 0
    a = float(F32(1.0 / np.sqrt(2.0)))
    cancel = np.flatnonzero(rng.random(N1) < 0.25) if N1 > 1 else np.array([0])
    for i in cancel:
        c0, c1 = rng.choice(C, 2, replace=False)
        q[2, i] = 0
        q[2, i, c0], q[2, i, c1] = a, -a
    pos = np.abs(rng.standard_normal((N2, C))); pos[:, -1] = 0
    store[0, 3] = _unit(pos)
    qd = np.abs(rng.standard_normal((N1, C))); qd[:, -1] = 0
    q[3] = _unit(qd)
    js, istar = min(1, N2 - 1), N1 // 2
    anti_r = np.abs(rng.standard_normal(C)); anti_r[-1] = 20.0
    store[0, 3, js] = -_unit(anti_r)
    anti_q = -np.abs(rng.standard_normal(C)); anti_q[-1] = 20.0
    q[3, istar] = _unit(anti_q)
    return q.astype(F32), store.astype(F32), np.zeros(4, np.int32), np.arange(4, dtype=np.int32), cancel


def _patch(ops, q, store, obj, tmpl, sel=None):
    appe, ratio = ops.patch_scores(_dev(q), _dev(store), _dev(obj), _dev(tmpl), THRED, sel=None if sel is None else _dev(sel))
    return _np(appe), _np(ratio)


def _patch_premise(ref, C):
    """What the exact comparisons rest on, asserted on the float64 reference with no case left out: every non-zero column maximum is at
    least 1e-4 away from the threshold and from 0 (300 x the kernel's error), and every query row's element sum is either exactly 0 or
    beyond the worst rounding of a float32 sum of C terms in any order, (C - 1) 2^-24 sum|x|."""
    assert ref["col_margin"].min() >= 1e-4, ref["col_margin"]
    rs, bound = ref["rowsum"], (C - 1) * 2.0 ** -24 * ref["rowabs"]
    assert ((rs == 0) | (np.abs(rs) > bound)).all(), np.abs(rs)[(rs != 0)].min()


def _patch_compare(ops, q, store, obj, tmpl, C):
    ref = ism_ref.patch_scores_ref(q, store[obj, tmpl], THRED)
    _patch_premise(ref, C)
    appe, ratio = _patch(ops, q, store, obj, tmpl)
    assert appe.dtype == F32 and ratio.dtype == F32
    assert np.array_equal(ratio, ref["ratio"]), (ratio, ref["ratio"], ref["vis"], ref["valid"])
    return appe, ratio, ref, float(np.abs(appe - ref["appe"]).max())


def check_patch_scores(ops, S, N1, N2, C):
    """patch_scores_kernel + patch_finalize_kernel at (S, N1, N2, C): the appearance score within 2e-6 of the float64 reference, the
    visible ratio BIT FOR BIT (its two counts are exact given the premise); every proposal of the S-call bit-identical to its own
    S = 1 call; and the four constructions of _patch_constructions, a and b giving exactly (0, 0)."""
    seed = PATCH_SHAPES[(S, N1, N2, C)]
    q, store, obj, tmpl = _patch_data(S, N1, N2, C, seed)
    appe, ratio, ref, err = _patch_compare(ops, q, store, obj, tmpl, C)
    for s in range(S if S > 1 else 0):
        a1, r1 = _patch(ops, q[s:s + 1], store, obj[s:s + 1], tmpl[s:s + 1])
        assert a1[0] == appe[s] and r1[0] == ratio[s], (s, a1, appe[s], r1, ratio[s])
    qc, sc, oc, tc, cancel = _patch_constructions(N1, N2, C, seed)
    appe_c, ratio_c, ref_c, err_c = _patch_compare(ops, qc, sc, oc, tc, C)
    assert appe_c[0] == 0.0 and ratio_c[0] == 0.0 and appe_c[1] == 0.0 and ratio_c[1] == 0.0
    # the constructions are what they claim to be (read off the float64 reference)
    sim_c = qc[2].astype(np.float64) @ sc[0, 2].astype(np.float64).T
    assert ref_c["nnz"][2] <= N1 - len(cancel) and (np.abs(sim_c[cancel]).max() > 0 or not sc[0, 2].any())
    sim_d = qc[3].astype(np.float64) @ sc[0, 3].astype(np.float64).T
    assert sim_d[:, min(1, N2 - 1)].max() < 0 and sim_d[N1 // 2].max() < 0
    assert ref_c["valid"][3] == N2 and ref_c["vis"][3] < N2
    _margin(f"ism_kernels.patch_scores[{S}-{N1}-{N2}-{C}]", appe_max_abs_err=max(err, err_c), tol=TOL,
            col_margin=float(min(ref["col_margin"].min(), ref_c["col_margin"].min())))
    assert err <= TOL and err_c <= TOL, (err, err_c)


def check_patch_sel(ops, N1, N2, C):
    """patch_scores(all, ..., sel=idx) is bit-identical to patch_scores(all[idx], ...), idx unsorted with a repeat."""
    q, store, _, _ = _patch_data(5, N1, N2, C, 11)
    idx = np.array([3, 0, 4, 3, 1], np.int32)
    obj, tmpl = np.array([1, 0, 1, 0, 1], np.int32), np.array([2, 0, 1, 1, 0], np.int32)
    a_sel, r_sel = _patch(ops, q, store, obj, tmpl, sel=idx)
    a_g, r_g = _patch(ops, q[idx], store, obj, tmpl)
    assert a_sel.shape == (5,) and np.array_equal(a_sel, a_g) and np.array_equal(r_sel, r_g)
    assert len(set(a_g.tolist())) > 2                                              # the rows do differ: a wrong row would show


def check_patch_refused(ops):
    for N2, C in ((257, 32), (16, 48)):
        q, store = np.zeros((1, 4, C), F32), np.zeros((1, 1, N2, C), F32)
        _raises(ops.patch_scores, _dev(q), _dev(store), _dev(np.zeros(1, np.int32)), _dev(np.zeros(1, np.int32)), THRED)


@pytest.mark.parametrize("S,N1,N2,C", list(PATCH_SHAPES))
def test_patch_scores_on_zero_cancelling_and_anticorrelated_rows(ops, S, N1, N2, C):
    check_patch_scores(ops, S, N1, N2, C)


def test_patch_scores_selection_form_and_refusals(ops):
    check_patch_sel(ops, 17, 15, 64)
    check_patch_sel(ops, 257, 250, 64)
    check_patch_refused(ops)


# =============================================================================================================== masked_depth_mean
DEPTH_SHAPES = [(2, 4), (37, 44)]


def _depth_case(H, W):
    """A millimetre depth map with holes (every 5th pixel 0) and negative readings (pixel index = 3 mod 7), and six masks: all zero |
    only holes | only negative pixels | negative pixels plus every 2nd valid one | random | everything."""
    rng = np.random.default_rng(H * 100 + W)
    n = H * W
    depth = rng.uniform(300, 1200, n).astype(F32)
    idx = np.arange(n)
    depth[idx % 7 == 3] *= -1
    depth[idx % 5 == 0] = 0
    masks = np.zeros((6, n), F32)
    masks[1] = depth == 0
    masks[2] = depth < 0
    masks[3] = (depth < 0) | ((depth > 0) & (idx % 2 == 0))
    masks[4] = rng.random(n) > 0.5
    masks[5] = 1
    assert (depth > 0).sum() >= 2 and masks[1].any() and masks[2].any()
    return masks.reshape(6, H, W), depth.reshape(H, W)


def _pinned(masks, depth, K):
    return oism.mean_translation_pinned(torch.from_numpy(masks), torch.from_numpy(depth), torch.from_numpy(K), 1.0).numpy()


def check_masked_depth(ops, H, W):
    """masked_depth_l1 / masked_depth_final against mean_translation_pinned BIT FOR BIT on masks without a valid pixel (all zero, only
    depth 0, only negative depth: exactly (0, 0, 0)), masks that mix negative and valid pixels (ignored like the reference's Z > 0),
    S = 1, the sel= form against the gathered form, and the frame= form with every mask on the last frame."""
    masks, depth = _depth_case(H, W)
    want = _pinned(masks, depth, KCAM)
    assert not want[:3].any() and want[3:, 2].all()
    K = torch.from_numpy(KCAM)
    got = _np(ops.masked_depth_mean(_dev(masks), _dev(depth), K, 1.0))
    assert got.dtype == F32 and np.array_equal(got, want), (got, want)
    for s in (0, 3, 5):
        assert np.array_equal(_np(ops.masked_depth_mean(_dev(masks[s:s + 1]), _dev(depth), K, 1.0)), want[s:s + 1]), s
    idx = np.array([4, 2, 5, 4, 0, 3], np.int32)
    by_sel = _np(ops.masked_depth_mean(_dev(masks), _dev(depth), K, 1.0, sel=_dev(idx)))
    gathered = _np(ops.masked_depth_mean(_dev(masks[idx]), _dev(depth), K, 1.0))
    assert np.array_equal(by_sel, gathered) and np.array_equal(gathered, want[idx])
    # three frames, every mask on the last one: the first two (other depth, other camera) must not be read
    depths = np.stack((depth[::-1] * 2, np.abs(depth) + 5, depth))
    Ks = torch.from_numpy(np.stack((KCAM * 1.1, KCAM * 0.9, KCAM)))
    frame = np.full(6, 2, np.int32)
    by_frame = _np(ops.masked_depth_mean(_dev(masks), _dev(depths), Ks, 1.0, frame=_dev(frame)))
    assert np.array_equal(by_frame, want)
    both = _np(ops.masked_depth_mean(_dev(masks), _dev(depths), Ks, 1.0, frame=_dev(frame), sel=_dev(idx)))
    assert np.array_equal(both, want[idx])


def check_masked_depth_refused(ops):
    K = torch.from_numpy(KCAM)
    for H, W in ((4, 6), (1, 4)):
        _raises(ops.masked_depth_mean, _dev(np.ones((2, H, W), F32)), _dev(np.ones((H, W), F32)), K, 1.0)


@pytest.mark.parametrize("H,W", DEPTH_SHAPES)
def test_masked_depth_mean_on_empty_and_negative_masks(ops, H, W):
    check_masked_depth(ops, H, W)


def test_masked_depth_mean_refuses_unsupported_maps(ops):
    check_masked_depth_refused(ops)


# ==================================================================================================================== project_bbox
IMG_H, IMG_W = 480, 640


def _special_points():
    """Model points for the identity pose and translation 0, where hx = fx x + cx z, hy = fy y + cy z, hz = z.  The first one is the
    case a bare (int) cast gets wrong on the device (+inf)."""
    K = KCAM.astype(F32).astype(np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    zq = fx / 3e9                                             # |u| ~ 3e9 at x = +-1
    pts = [(0.3, 0.1, 0.0), (-0.3, -0.1, 0.0), (0.0, 0.0, 0.0), (0.0, 0.2, 0.0), (0.3, -0.1, 0.0),       # on the camera plane
           (0.3, -0.2, 1.0), (-0.3, 0.2, 1.0), (0.0, 0.0, 1.0),                                          # in front
           (0.3, 0.1, -1.0), (-0.3, -0.1, -1.0), (0.0, 0.0, -1.0),                                       # behind
           (1.0, 0.0, zq), (-1.0, 0.0, zq), (0.0, 1.0, zq), (0.0, -1.0, zq),                             # quotients of +-3e9
           ((-0.5 - cx) / fx, (-0.5 - cy) / fy, 1.0),                                                    # quotients in (-1, 0)
           ((IMG_W - 0.25 - cx) / fx, (IMG_H - 0.25 - cy) / fy, 1.0),                                    # just below W, H
           ((IMG_W + 0.25 - cx) / fx, (IMG_H + 0.25 - cy) / fy, 1.0)]                                    # just above
    return np.array(pts, F32)


@functools.lru_cache(maxsize=None)
def _project_case(N):
    rng = np.random.default_rng(N)
    pc = (0.05 * rng.standard_normal((2, N, 3))).astype(F32)
    sp = _special_points()[:N]
    pc[0, :len(sp)] = sp
    poses = np.tile(np.eye(4, dtype=F32), (3, 1, 1))
    poses[1:, :3, :3] = np.linalg.qr(rng.standard_normal((2, 3, 3)))[0].astype(F32)
    obj, tmpl = np.array([0, 1, 0], np.int32), np.array([0, 2, 1], np.int32)
    trans = np.array([[0, 0, 0], [0.1, -0.05, 0.8], [-0.2, 0.1, 0.02]], F32)
    return pc, poses, obj, tmpl, trans


def check_project(ops, N, S):
    """project_bbox_kernel against project_ref, pixels and boxes BIT FOR BIT: N on both sides of the 256-thread block, proposal 0 on
    the identity pose with translation 0 over the points of _special_points (the others rotate and shift them), one camera and the
    frame= form with two."""
    pc, poses, obj, tmpl, trans = _project_case(N)
    obj, tmpl, trans = obj[:S], tmpl[:S], trans[:S]
    K = KCAM.astype(F32)
    want_uv, want_box = ism_ref.project_ref(pc[obj], poses[tmpl][:, :3, :3], trans, K, IMG_H, IMG_W)
    assert tuple(want_uv[0, 0]) == (0, 0)                                          # +inf is pixel 0 in the pinned run
    if N >= 17:
        assert want_uv[0, 11, 0] == 0 and want_uv[0, 12, 0] == 0                   # +-3e9 too
        assert tuple(want_uv[0, 15]) == (0, 0) and tuple(want_uv[0, 16]) == (IMG_W - 1, IMG_H - 1)
    uv, box = ops.project_bbox(_dev(pc), _dev(poses), _dev(obj), _dev(tmpl), _dev(trans), _dev(K), IMG_H, IMG_W)
    assert uv.dtype == torch.int32 and box.dtype == torch.int32
    bad = np.argwhere(_np(uv) != want_uv)
    assert len(bad) == 0, (bad[:8], _np(uv)[tuple(bad[0][:2])], want_uv[tuple(bad[0][:2])])
    assert np.array_equal(_np(box), want_box)
    Ks = np.stack((K, K * np.array([[1.1], [0.9], [1.0]], F32)))
    frame = np.array([1, 0, 1], np.int32)[:S]
    want_uv, want_box = ism_ref.project_ref(pc[obj], poses[tmpl][:, :3, :3], trans, Ks[frame], IMG_H, IMG_W)
    uv, box = ops.project_bbox(_dev(pc), _dev(poses), _dev(obj), _dev(tmpl), _dev(trans), _dev(Ks), IMG_H, IMG_W, frame=_dev(frame))
    assert np.array_equal(_np(uv), want_uv) and np.array_equal(_np(box), want_box)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_project_bbox_on_and_behind_the_camera_plane(ops, N, S):
    check_project(ops, N, S)


# =================================================================================================================== module guards
# Shapes the kernels refuse take the library branch of their module (policy not strict) instead of raising from the C ABI, give the
# oracle's values, and policy.library_branch_hits() names the condition that failed.
def _library_branch(ops, *kernels):
    import contextlib

    from sam6d_amd import policy
    assert all(ops.have(k) for k in kernels)                                       # it is the SHAPE that sends the call to the library

    @contextlib.contextmanager
    def scope():
        with policy.use(strict="0"):
            policy.reset_library_branch_hits()
            yield policy.library_branch_hits
    return scope()


def check_guard_pairwise(ops):
    """PairwiseSimilarity on C = 40 descriptors: pairwise_cosine_kernel needs C % 16 == 0 (guard `C16`)."""
    from sam6d_amd.ism.loss import PairwiseSimilarity
    g = torch.Generator().manual_seed(4)
    q, r = torch.randn(7, 40, generator=g), torch.randn(2, 5, 40, generator=g)
    with _library_branch(ops, "pairwise_cosine") as hits:
        out = PairwiseSimilarity()(q.cuda(), r.cuda())
        assert torch.allclose(out.cpu(), oism.pairwise_similarity(q, r), atol=1e-5)
        assert hits() == {("ism.PairwiseSimilarity", "C16"): 1}


def check_guard_masked_depth(ops):
    """masked_depth_translation on a 3 x 6 frame (W % 4 != 0: guard `W4`) and a 1 x 4 frame (fewer than 8 pixels: `pixels_8_to_2p24`)."""
    from sam6d_amd.ism.scoring import masked_depth_translation
    g = torch.Generator().manual_seed(5)
    K = torch.from_numpy(KCAM)
    for (H, W), cond in (((3, 6), "W4"), ((1, 4), "pixels_8_to_2p24")):
        masks = (torch.rand(3, H, W, generator=g) > 0.3).float()
        masks[0, 0, 0] = 1.0
        depth = torch.rand(H, W, generator=g) * 900 + 300
        depth[0, 1] = 0
        with _library_branch(ops, "masked_depth_mean") as hits:
            t = masked_depth_translation(masks.cuda(), depth.cuda(), K, 1.0)
            assert t.dtype == torch.float32 and torch.allclose(t.cpu(), oism.mean_translation(masks, depth, K, 1.0), atol=1e-5)
            assert hits() == {("ism.masked_depth_mean", cond): 1}


def check_guard_appearance(ops):
    """FrameScorer.compute_appearance_score on C = 48 patch descriptors: patch_scores_kernel needs C % 32 == 0 (guard `C32`, like
    MaskedPatch_MatrixSimilarity, which the library branch then calls and which records its own)."""
    from sam6d_amd.ism.scoring import FrameScorer
    g = torch.Generator().manual_seed(6)
    S, n, C = 4, 20, 48
    store = torch.nn.functional.normalize(torch.randn(2, 3, n, C, generator=g), dim=-1)
    store = store * (torch.rand(2, 3, n, 1, generator=g) > 0.3)
    obj, tmpl = torch.tensor([0, 1, 1, 0]), torch.tensor([2, 0, 1, 1])
    qp = torch.nn.functional.normalize(0.7 * store[obj, tmpl] + 0.3 * torch.randn(S, n, C, generator=g) / C ** 0.5, dim=-1)
    qp = qp * (torch.rand(S, n, 1, generator=g) > 0.3)
    fs = FrameScorer(torch.randn(2, 3, 64, generator=g).cuda(), store.cuda(), torch.eye(4).repeat(3, 1, 1).cuda(),
                     torch.randn(2, 8, 3, generator=g).cuda())
    with _library_branch(ops, "patch_scores") as hits:
        appe, ref = fs.compute_appearance_score(tmpl.cuda(), obj.cuda(), qp.cuda())
        want, want_ref = oism.appearance_score(qp, store, obj, tmpl)
        assert torch.allclose(appe.cpu(), want, atol=1e-5) and torch.equal(ref.cpu(), want_ref)
        assert hits() == {("ism.compute_appearance_score", "C32"): 1, ("ism.MaskedPatch_MatrixSimilarity", "C32"): 1}


def test_pairwise_similarity_guard_sends_odd_channel_counts_to_the_library(ops):
    check_guard_pairwise(ops)


def test_masked_depth_guard_sends_unsupported_maps_to_the_library(ops):
    check_guard_masked_depth(ops)


def test_appearance_score_guard_sends_odd_channel_counts_to_the_library(ops):
    check_guard_appearance(ops)
