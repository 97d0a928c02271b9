"""A restatement of the point-to-plane refinement step (sam6d_amd/csrc/s6d_refine.hip) for the refine tests.

It is pinned to no other tool: SAM-6D has no refinement.  It restates the DEFINITION in the kernel file's header a second time,
independently: the per-pixel float64 operations one at a time (numpy float64 elementwise operations and Python floats are IEEE
operations rounded on their own; numpy does not contract), the reduction in the stated order -- a lane's visits, the xor butterfly
of a wave, the four waves, the chunks -- and the 6 x 6 solve and Cayley update in plain loops over Python floats.

``normal_eq`` also reports, per predicate, how many pixels it passed and rejected (the tests assert that every predicate has pixels
on both sides somewhere) and the absolute sums sum |term| by ``math.fsum``: the factor of the derived bound
n 2^-52 sum |term| that holds for ANY order of n additions of correctly rounded terms."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
THREADS, WAVE, TERMS = 256, 64, 28
PREDICATES = ("face", "mask", "depth", "area", "grazing", "distance")


def _c(x):
    return float(F32(x))          # a float of the C ABI


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _rot(R, x):
    return [(R[i, 0] * x[0] + R[i, 1] * x[1]) + R[i, 2] * x[2] for i in range(3)]


def pixel_terms(xyz, face, depth, mask, vertices, faces, pose, K, depth_unit, max_dist, min_cos):
    """One instance -> terms (H W, 28) float64, ok (H W,) bool, tally {predicate: [passed, rejected]}."""
    H, W = face.shape
    V, F = len(vertices), len(faces)
    fx, fy, cx, cy = (_c(k) for k in K)
    unit, md, mc = _c(depth_unit), _c(max_dist), _c(min_cos)
    tally = {}
    with np.errstate(all="ignore"):
        f = face.reshape(-1).astype(np.int64)
        alive = np.ones(H * W, bool)

        def gate(name, cond):
            nonlocal alive
            tally[name] = [int((alive & cond).sum()), int((alive & ~cond).sum())]
            alive = alive & cond
        tri = np.asarray(faces, np.int64)[np.clip(f, 0, F - 1)]
        gate("face", (f >= 0) & (f < F) & ((tri >= 0) & (tri < V)).all(1))
        gate("mask", np.ones(H * W, bool) if mask is None else mask.reshape(-1) != 0)
        Zo = depth.reshape(-1).astype(F64) * unit
        gate("depth", Zo > 0)
        u = np.tile(np.arange(W, dtype=F64), H)
        v = np.repeat(np.arange(H, dtype=F64), W)
        q = [((u - cx) / fx) * Zo, ((v - cy) / fy) * Zo, Zo]
        P = np.asarray(pose, F32).astype(F64)
        R, tr = P[:3, :3], P[:3, 3]
        x = xyz.reshape(-1, 3).astype(F64).T
        p = [r + tr[i] for i, r in enumerate(_rot(R, x))]
        vv = np.asarray(vertices, F32).astype(F64)[np.clip(tri, 0, V - 1)]
        a, b = (vv[:, 1] - vv[:, 0]).T, (vv[:, 2] - vv[:, 0]).T
        m = _cross(a, b)
        mm = _dot(m, m)
        gate("area", ~(mm == 0))
        sm = np.sqrt(mm)
        n = _rot(R, [k / sm for k in m])
        npd = _dot(n, p)
        flip = npd > 0
        n = [np.where(flip, -k, k) for k in n]
        npd = np.where(flip, -npd, npd)
        gate("grazing", npd * npd >= (mc * mc) * _dot(p, p))
        d = [q[i] - p[i] for i in range(3)]
        gate("distance", _dot(d, d) <= md * md)
        r = _dot(n, d)
        J = _cross(p, n) + n
        terms = np.stack([J[i] * J[j] for i in range(6) for j in range(i, 6)] + [J[i] * r for i in range(6)] + [r * r], 1)
    return terms, alive, tally


def reduce_ordered(terms, ok, chunk):
    """The stated reduction of one instance -> (sums (28,), count)."""
    n = len(terms)
    chunks = (n + chunk - 1) // chunk
    lanes = np.arange(WAVE)
    total, count = np.zeros(TERMS), 0
    for c in range(chunks):
        acc = np.zeros((THREADS, TERMS))
        for visit in range(chunk // THREADS):                                   # a lane adds in visiting order
            p = c * chunk + visit * THREADS + np.arange(THREADS)
            sel = p < n
            sel[sel] = ok[p[sel]]
            acc[sel] = acc[sel] + terms[p[sel]]
        waves = []
        for w in range(THREADS // WAVE):
            x = acc[w * WAVE:(w + 1) * WAVE]
            for o in (32, 16, 8, 4, 2, 1):                                      # the xor butterfly: every lane adds its partner's value
                x = x + x[lanes ^ o]
            waves.append(x[0])
        part = ((waves[0] + waves[1]) + waves[2]) + waves[3]                    # wave order
        total = total + part                                                    # chunk order
        count += int(ok[c * chunk:(c + 1) * chunk].sum())
    return total, count


def normal_eq(xyz, face, depth_obs, obs_index, mask, vertices, faces, poses, K, depth_unit, max_dist, min_cos, chunk):
    """-> dict(sums (T,28) f64, count (T,) i32, abs (T,28) f64 = fsum |term| over the correspondences, tally)."""
    T = len(poses)
    M = len(depth_obs)
    out = dict(sums=np.zeros((T, TERMS)), count=np.zeros(T, np.int32), abs=np.zeros((T, TERMS)),
               tally={k: [0, 0] for k in PREDICATES})
    for t in range(T):
        ti = int(obs_index[t])
        if not 0 <= ti < M:
            continue
        terms, ok, tally = pixel_terms(xyz[t], face[t], depth_obs[ti], None if mask is None else mask[t], vertices, faces, poses[t], K,
                                       depth_unit, max_dist, min_cos)
        out["sums"][t], out["count"][t] = reduce_ordered(terms, ok, chunk)
        out["abs"][t] = [math.fsum(np.abs(terms[ok, k]).tolist()) for k in range(TERMS)]
        for k in PREDICATES:
            out["tally"][k][0] += tally[k][0]
            out["tally"][k][1] += tally[k][1]
    return out


def bound(ref):
    """n 2^-52 sum |term| per component: any order of the n additions stays within it of any other (each addition's error is at most
    2^-53 of a partial sum that is at most sum |term| (1 + n 2^-53))."""
    return ref["count"][:, None].astype(F64) * 2.0 ** -52 * ref["abs"]


def update_one(S, n, P, min_count, damping, min_pivot):
    """One instance: S 28 floats, n count, P (4,4) float32 -> (P' (4,4) float32, status, rms).  Plain Python floats."""
    S = [float(x) for x in S]
    P = np.asarray(P, F32)
    Pd = [[float(P[i, j]) for j in range(4)] for i in range(4)]
    lam, min_pivot = _c(damping), _c(min_pivot)
    finite = all(math.isfinite(x) for x in S)
    rms = math.sqrt(S[27] / float(n)) if finite and n > 0 else 0.0
    finite = finite and all(math.isfinite(Pd[i][j]) for i in range(3) for j in range(4))
    if not finite:
        return P.copy(), 3, rms
    if n < min_count:
        return P.copy(), 1, rms
    A, k = [[0.0] * 6 for _ in range(6)], 0
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = S[k]
            k += 1
    d = [math.sqrt(A[i][i]) for i in range(6)]
    c = [0.0 if d[i] == 0.0 else S[21 + i] / d[i] for i in range(6)]
    Mx = [[1.0 + lam if i == j else (0.0 if d[i] * d[j] == 0.0 else A[i][j] / (d[i] * d[j])) for j in range(6)] for i in range(6)]
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = Mx[j][j]
        for q in range(j):
            s = s - L[j][q] * L[j][q]
        if not s >= min_pivot:
            return P.copy(), 2, rms
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            s = Mx[i][j]
            for q in range(j):
                s = s - L[i][q] * L[j][q]
            L[i][j] = s / L[j][j]
    z, y = [0.0] * 6, [0.0] * 6
    for i in range(6):
        s = c[i]
        for q in range(i):
            s = s - L[i][q] * z[q]
        z[i] = s / L[i][i]
    for i in range(5, -1, -1):
        s = z[i]
        for q in range(i + 1, 6):
            s = s - L[q][i] * y[q]
        y[i] = s / L[i][i]
    xi = [0.0 if d[i] == 0.0 else y[i] / d[i] for i in range(6)]
    h0, h1, h2 = xi[0] * 0.5, xi[1] * 0.5, xi[2] * 0.5
    hh = (h0 * h0 + h1 * h1) + h2 * h2
    e, g = 1.0 + hh, 1.0 - hh
    xy, xz, yz, x2, y2, z2 = 2.0 * (h0 * h1), 2.0 * (h0 * h2), 2.0 * (h1 * h2), 2.0 * h0, 2.0 * h1, 2.0 * h2
    dR = [[(g + 2.0 * (h0 * h0)) / e, (xy - z2) / e, (xz + y2) / e],
          [(xy + z2) / e, (g + 2.0 * (h1 * h1)) / e, (yz - x2) / e],
          [(xz - y2) / e, (yz + x2) / e, (g + 2.0 * (h2 * h2)) / e]]
    new = P.copy()
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                new[i, j] = F32((dR[i][0] * Pd[0][j] + dR[i][1] * Pd[1][j]) + dR[i][2] * Pd[2][j])
            new[i, 3] = F32(((dR[i][0] * Pd[0][3] + dR[i][1] * Pd[1][3]) + dR[i][2] * Pd[2][3]) + xi[3 + i])
    if not np.isfinite(new[:3]).all():
        return P.copy(), 3, rms
    return new, 0, rms


def update(sums, count, poses, min_count, damping, min_pivot):
    """-> (poses_out (T,4,4) f32, status (T,) i32, rms (T,) f64)."""
    res = [update_one(sums[t], int(count[t]), poses[t], min_count, damping, min_pivot) for t in range(len(poses))]
    return (np.stack([r[0] for r in res]).astype(F32), np.array([r[1] for r in res], np.int32), np.array([r[2] for r in res], F64))


def mssd(vertices, est, gt):
    """max_v |est v - gt v| in float64 (no symmetries)."""
    v = np.asarray(vertices, F64)
    a = v @ np.asarray(est, F64)[:3, :3].T + np.asarray(est, F64)[:3, 3]
    b = v @ np.asarray(gt, F64)[:3, :3].T + np.asarray(gt, F64)[:3, 3]
    return float(np.linalg.norm(a - b, axis=1).max())


def rotation(axis, angle):
    a = np.asarray(axis, F64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * Kx @ Kx
