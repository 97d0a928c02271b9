"""A numpy restatement of the BOP pose errors for the evaluation tests, written from the DEFINITIONS (the issue text that
sam6d_amd/csrc/s6d_boperr.hip's header also states), not from the kernel source, and a plain-Python greedy matcher.

bop_toolkit is not present and nothing here is pinned to it.  Two modes:

  * ``np.float32``: every operation in float32 in the stated order (numpy rounds each array operation once, divisions and square
    roots correctly): the kernels must give these bits;
  * ``np.float64``: the same formulas on the same float32 inputs, widened: what the float32 operations approximate.  The float64
    functions also return the quantities the derived bounds scale with (profiles/bop_eval_margins.md).
"""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32


def _transform(P, v, dt):
    """P (...,4,4), v (V,3) -> X, Y, Z (...,V):  ((r0 vx + r1 vy) + r2 vz) + t, in dt."""
    P, v = np.asarray(P, np.float32).astype(dt), np.asarray(v, np.float32).astype(dt)
    out = []
    for r in range(3):
        c = [P[..., r, k][..., None] for k in range(4)]
        out.append(((c[0] * v[:, 0] + c[1] * v[:, 1]) + c[2] * v[:, 2]) + c[3])
    return out


def _abs_transform(P, v):
    """sum_k |r_k v_k| + |t| per row, maximum over the rows: the scale of a transformed coordinate's rounding error.  (...,V) f64"""
    P, v = np.abs(np.asarray(P, np.float32).astype(np.float64)), np.abs(np.asarray(v, np.float32).astype(np.float64))
    rows = [((P[..., r, 0][..., None] * v[:, 0] + P[..., r, 1][..., None] * v[:, 1]) + P[..., r, 2][..., None] * v[:, 2]) + P[..., r, 3][..., None]
            for r in range(3)]
    return np.maximum(np.maximum(rows[0], rows[1]), rows[2])


def pose_errors(vertices, est, gts, cams, dt=np.float32):
    """vertices (V,3), est (N,4,4), gts (N,S,4,4), cams (N,4) -> dict: mssd (N,), mspd (N,) in dt; in float64 mode also
    ``coord`` (N,): max over s, v and both poses of sum |r v| + |t|, ``proj`` (N,): max over s, v and both poses of
    (f / Z)(1 + max(|X|, |Y|) / Z) (sum |r v| + |t|), ``pixel`` (N,): max of |f X / Z| + |c| -- the factors of the bounds -- and ``arg`` (N,S): the vertex of the maximum
    3-D distance."""
    est, gts, cams = np.asarray(est, np.float32), np.asarray(gts, np.float32), np.asarray(cams, np.float32).astype(dt)
    inf = dt(np.inf)
    with np.errstate(all="ignore"):
        Xe, Ye, Ze = _transform(est[:, None], vertices, dt)                 # (N,1,V)
        Xg, Yg, Zg = _transform(gts, vertices, dt)                          # (N,S,V)
        dx, dy, dz = Xe - Xg, Ye - Yg, Ze - Zg
        d3 = (dx * dx + dy * dy) + dz * dz
        d3 = np.where(np.isfinite(d3), d3, inf)
        fx, fy, cx, cy = (cams[:, k][:, None, None] for k in range(4))
        du = ((fx * Xe) / Ze + cx) - ((fx * Xg) / Zg + cx)
        dv = ((fy * Ye) / Ze + cy) - ((fy * Yg) / Zg + cy)
        d2 = du * du + dv * dv
        d2 = np.where((Ze > 0) & (Zg > 0) & np.isfinite(d2), d2, inf)
        out = dict(mssd=np.sqrt(d3.max(2)).min(1).astype(dt), mspd=np.sqrt(d2.max(2)).min(1).astype(dt))
        if dt is np.float64:
            Ae, Ag = _abs_transform(est[:, None], vertices), _abs_transform(gts, vertices)
            out["coord"] = np.maximum(Ae.max((1, 2)), Ag.max((1, 2)))
            f = np.maximum(np.abs(fx), np.abs(fy))
            pe = (f / Ze) * (1 + np.maximum(np.abs(Xe), np.abs(Ye)) / Ze) * Ae
            pg = (f / Zg) * (1 + np.maximum(np.abs(Xg), np.abs(Yg)) / Zg) * Ag
            out["proj"] = np.maximum(np.broadcast_to(pe, pg.shape), pg).max((1, 2))
            ce, cg = np.maximum(np.abs((fx * Xe) / Ze), np.abs((fy * Ye) / Ze)), np.maximum(np.abs((fx * Xg) / Zg), np.abs((fy * Yg) / Zg))
            out["pixel"] = np.maximum(ce.max((1, 2)), cg.max((1, 2))) + np.maximum(np.abs(cx), np.abs(cy))[:, 0, 0]
            out["arg"] = d3.argmax(2)
    return out


def mssd_bound(ref64):
    """|mssd32 - mssd64| <= 10 sqrt(3) u C + 5 u mssd64, C = ``coord`` (profiles/bop_eval_margins.md)."""
    return 10 * np.sqrt(3.0) * U * ref64["coord"] + 5 * U * ref64["mssd"]


def mspd_bound(ref64):
    """|mspd32 - mspd64| <= 2 sqrt(2) (5 u P + 3 u X) + 4 u mspd64, P = ``proj``, X = ``pixel`` (profiles/bop_eval_margins.md)."""
    return 2 * np.sqrt(2.0) * (5 * U * ref64["proj"] + 3 * U * ref64["pixel"]) + 4 * U * ref64["mspd"]


def vsd_counts(depth_est, depth_gt, depth_test, test_index, cams, delta, taus, scale, dt=np.float32, input_rel=0.0):
    """-> dict: union (N,), inter (N,) int64, ge (N,NT) int64; in float64 mode also ``undecided`` (N,): the pixels at which a
    compared quantity lies within the rounding margin of its threshold (8 u (Dg + Dt) around delta, 9 u (Dg + De) / scale around
    a tau: profiles/bop_eval_margins.md).  ``input_rel``: a relative uncertainty of the two rendered depths themselves, added to
    both margins (8 u when the renders come from another implementation of the depth statement)."""
    de, dg = np.asarray(depth_est, np.float32).astype(dt), np.asarray(depth_gt, np.float32).astype(dt)
    zt = np.asarray(depth_test, np.float32).astype(dt)[np.asarray(test_index)]
    cams, scale = np.asarray(cams, np.float32).astype(dt), np.asarray(scale, np.float32).astype(dt)
    taus, delta = np.asarray(taus, np.float32).astype(dt), dt(np.float32(delta))
    N, H, W = de.shape
    u, v = np.arange(W, dtype=dt)[None, None, :], np.arange(H, dtype=dt)[None, :, None]
    fx, fy, cx, cy = (cams[:, k][:, None, None] for k in range(4))
    with np.errstate(all="ignore"):
        a, b = (u - cx) / fx, (v - cy) / fy
        r = np.sqrt((a * a + b * b) + dt(1))
        De, Dg, Dt = de * r, dg * r, zt * r
        vis_gt = (dg > 0) & (((Dg - Dt) <= delta) | (zt == 0))
        vis_est = (de > 0) & ((((De - Dt) <= delta) | (zt == 0)) | vis_gt)
        inter, union = vis_gt & vis_est, vis_gt | vis_est
        x = np.abs(Dg - De) / scale[:, None, None]
        ge = np.stack([(inter & (x >= t)).sum((1, 2)) for t in taus], 1)
        out = dict(union=union.sum((1, 2)), inter=inter.sum((1, 2)), ge=ge)
        if dt is np.float64:
            seen = zt != 0
            und = (dg > 0) & seen & (np.abs((Dg - Dt) - delta) <= (8 * U + input_rel) * (np.abs(Dg) + np.abs(Dt)))
            und |= (de > 0) & seen & (np.abs((De - Dt) - delta) <= (8 * U + input_rel) * (np.abs(De) + np.abs(Dt)))
            both = (dg > 0) & (de > 0)
            for t in taus:
                und |= both & (np.abs(x - t) <= (9 * U + input_rel) * (np.abs(Dg) + np.abs(De)) / scale[:, None, None])
            out["undecided"] = und.sum((1, 2))
    return out


def vsd_errors(counts):
    """e_k = (ge_k + union - inter) / union in float64, 1 for an empty union.  (N,NT)"""
    un, it, ge = (np.asarray(counts[k], np.float64) for k in ("union", "inter", "ge"))
    with np.errstate(all="ignore"):
        e = (ge + (un - it)[:, None]) / un[:, None]
    return np.where(un[:, None] > 0, e, 1.0)


def match_and_recall(errors, scores, est_group, gt_group, n_targets, thresholds):
    """The greedy matching, one loop at a time.  errors (E,G): error of estimate e against ground truth g (only pairs of the same
    group count); scores (E,); est_group (E,), gt_group (G,): the (image, object) group ids; n_targets [group]: number of target
    instances; thresholds: a list.  Per threshold: in every group keep the n_targets highest-scoring estimates (ties: the lower
    index), go through them in descending score, each takes the unmatched ground truth of its group with the lowest error below
    the threshold (ties: the lower index).  -> recalls [matched targets / all targets] per threshold."""
    E, G = len(scores), len(gt_group)
    recalls = []
    for th in thresholds:
        matched = 0
        for grp in range(len(n_targets)):
            es = [e for e in range(E) if int(est_group[e]) == grp]
            es.sort(key=lambda e: (-float(scores[e]), e))
            es = es[:int(n_targets[grp])]
            gs = [g for g in range(G) if int(gt_group[g]) == grp]
            taken = set()
            for e in es:
                best = None
                for g in gs:
                    if g in taken or not float(errors[e][g]) < th:
                        continue
                    if best is None or float(errors[e][g]) < float(errors[e][best]):
                        best = g
                if best is not None:
                    taken.add(best)
                    matched += 1
        total = sum(int(n) for n in n_targets)
        recalls.append(matched / total if total else 0.0)
    return recalls


def rotation(axis, angle):
    """Rodrigues, float64."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def seeded_poses(n, seed, zmin=300.0, zmax=1500.0):
    """n object -> camera poses, float64: seeded rotations, translation z in [zmin, zmax], x and y within a fifth of z; rounded to
    1/16 so that float32 holds them and small integer offsets exactly."""
    from tests import render_ref as R
    rs = np.random.RandomState(seed)
    P = np.tile(np.eye(4), (n, 1, 1))
    P[:, :3, :3] = R.rotations(n, seed)
    z = rs.uniform(zmin, zmax, n)
    P[:, 0, 3], P[:, 1, 3], P[:, 2, 3] = rs.uniform(-0.2, 0.2, n) * z, rs.uniform(-0.2, 0.2, n) * z, z
    P[:, :3, 3] = np.round(P[:, :3, 3] * 16) / 16
    return P


def axis_symmetries(S, axis=(0.0, 0.0, 1.0), offset=(0.0, 0.0, 0.0)):
    """S rotations by 2 pi k / S about the axis through ``offset`` -> (S,4,4) float64, the identity first."""
    out = np.tile(np.eye(4), (S, 1, 1))
    off = np.asarray(offset, np.float64)
    for k in range(1, S):
        out[k, :3, :3] = rotation(axis, 2 * np.pi * k / S)
        out[k, :3, 3] = off - out[k, :3, :3] @ off
    return out
