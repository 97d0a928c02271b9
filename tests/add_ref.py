"""A numpy restatement of the ADD / ADD-S pose errors for their tests, written from the DEFINITIONS (the issue text that
sam6d_amd/csrc/s6d_adderr.hip's header also states), not from the kernel source: loops over the estimates, vectorised vertices, no
kernels and no torch.  bop_toolkit is not present and nothing here is pinned to it.

  E = est[n], G = gts[n] (4 x 4, object -> camera), v_i the V vertices, X = ((r00 vx + r01 vy) + r02 vz) + tx and Y, Z alike;
  ADD    a_i = sqrt((dx dx + dy dy) + dz dz),  d = E v_i - G v_i
  ADD-S  s_i = sqrt(min_j d2(E v_i, G v_j));  a squared distance that is not finite (NaN included) counts as +inf in both
  mean   (sum_i (double)value_i) / V, max = max_i value_i

Two modes:

  * ``np.float32``: every operation in float32 in the stated order (numpy rounds each array operation once, square roots correctly),
    the minimum on the bits as unsigned integers, and the mean in float64 in the STATED ORDER: lane l of 256 adds i = l, l + 256, ...
    in visiting order from +0, each wave of 64 lanes by the xor butterfly x += x[lane ^ o] for o = 32 .. 1, the four waves as
    ((w0 + w1) + w2) + w3, one division by V.  The kernels must give these bits.
  * ``np.float64``: the same formulas on the same float32 inputs widened (positions exact to 2^-53 relative), the mean by
    ``math.fsum``.  Its own error is 2^-29 of the float32 unit and is ignored in the bounds.

``bounds`` gives the derived per-vertex bound of |float32 - float64| (tests/test_gpu_add_eval.py derives it).
"""
import math

import numpy as np

U = 2.0 ** -24                         # unit roundoff of float32
U2 = 1.0 + 2.0 ** -20                  # room for the second-order terms of (1 + u)^k - 1, k <= 5
INF_BITS = np.uint32(0x7f800000)
LANES, WAVE = 256, 64


def transform(P, v, dt):
    """-> (V,3) in dt: X = ((r00 vx + r01 vy) + r02 vz) + tx, one rounding per operation."""
    P, v = np.asarray(P, np.float32).astype(dt), np.asarray(v, np.float32).astype(dt)
    with np.errstate(all="ignore"):
        out = np.stack([((P[r, 0] * v[:, 0] + P[r, 1] * v[:, 1]) + P[r, 2] * v[:, 2]) + P[r, 3] for r in range(3)], 1)
    assert out.dtype == dt
    return out


def _root(d2, dt):
    """sqrt of squared distances with every non-finite one at +inf; in float32 through the bits, as the definition takes it."""
    with np.errstate(all="ignore"):
        if dt is np.float32:
            b = np.minimum(np.ascontiguousarray(d2, np.float32).view(np.uint32), INF_BITS)
            return np.sqrt(b.view(np.float32))
        return np.sqrt(np.where(np.isfinite(d2), d2, np.inf))


def _d2(a, b):
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def per_vertex(vertices, est, gts, dt=np.float32, rows=256):
    """-> (add (N,V), adds (N,V)) in dt."""
    est, gts = np.asarray(est, np.float32), np.asarray(gts, np.float32)
    N, V = len(est), len(vertices)
    add, adds = np.zeros((N, V), dt), np.zeros((N, V), dt)
    with np.errstate(all="ignore"):
        for n in range(N):
            e, g = transform(est[n], vertices, dt), transform(gts[n], vertices, dt)
            add[n] = _root(_d2(e, g), dt)
            for i in range(0, V, rows):
                d2 = _d2(e[i:i + rows, None, :], g[None, :, :])
                if dt is np.float32:                                      # the minimum of the bits, unsigned
                    m = np.ascontiguousarray(d2).view(np.uint32).min(1).view(np.float32)
                else:
                    m = np.where(np.isfinite(d2), d2, np.inf).min(1)
                adds[n, i:i + rows] = _root(m, dt)
    return add, adds


def mean_fixed(values):
    """(N,V) float32 -> (N,) float64 in the stated order (plain loops over the lanes' visits, the butterfly and the waves)."""
    values = np.asarray(values, np.float32)
    N, V = values.shape
    out = np.zeros(N, np.float64)
    lane = np.arange(WAVE)
    with np.errstate(all="ignore"):
        for n in range(N):
            acc = np.zeros(LANES, np.float64)
            for i0 in range(0, V, LANES):
                chunk = values[n, i0:i0 + LANES].astype(np.float64)
                acc[:len(chunk)] = acc[:len(chunk)] + chunk
            waves = []
            for w in range(LANES // WAVE):
                x = acc[w * WAVE:(w + 1) * WAVE].copy()
                o = WAVE // 2
                while o:
                    x = x + x[lane ^ o]
                    o //= 2
                waves.append(x[0])
            s = waves[0]
            for w in waves[1:]:
                s = s + w
            out[n] = s / np.float64(V)
    return out


def mean_fsum(values):
    """(N,V) -> (N,) float64: math.fsum of the values over V (+inf when one is +inf)."""
    out = np.zeros(len(values), np.float64)
    for n, row in enumerate(np.asarray(values, np.float64)):
        out[n] = math.inf if np.isinf(row).any() else math.fsum(row.tolist()) / row.shape[0]
    return out


def errors(vertices, est, gts, dt=np.float32):
    """-> dict(add_per_vertex, adds_per_vertex (N,V) dt; add, adds (N,) float64; add_max, adds_max (N,) dt)."""
    a, s = per_vertex(vertices, est, gts, dt)
    mean = mean_fixed if dt is np.float32 else mean_fsum
    return dict(add_per_vertex=a, adds_per_vertex=s, add=mean(a), adds=mean(s), add_max=a.max(1), adds_max=s.max(1))


def position_bound(P, vertices):
    """(V,) float64: the Euclidean bound of |fl(P v) - P v|.  Per coordinate the float32 statement ((a + b) + c) + t passes its
    first product through four roundings and every other term through fewer: at most 4 u (|r0 vx| + |r1 vy| + |r2 vz| + |t|)."""
    P, v = np.abs(np.asarray(P, np.float32).astype(np.float64)), np.abs(np.asarray(vertices, np.float32).astype(np.float64))
    per = 4 * U * U2 * np.stack([P[r, 0] * v[:, 0] + P[r, 1] * v[:, 1] + P[r, 2] * v[:, 2] + P[r, 3] for r in range(3)], 1)
    return np.sqrt((per * per).sum(1))


def bounds(vertices, est, gts, r64):
    """The derived bounds of |float32 - float64| per vertex -> (add (N,V), adds (N,V)) float64, from the float64 restatement r64."""
    N, V = r64["add_per_vertex"].shape
    ba, bs = np.zeros((N, V)), np.zeros((N, V))
    for n in range(N):
        pe, pg = position_bound(est[n], vertices), position_bound(gts[n], vertices)
        p = pe + pg
        ba[n] = p + 3.5 * U * U2 * (r64["add_per_vertex"][n] + p)
        p = pe + pg.max()
        bs[n] = p + 3.5 * U * U2 * (r64["adds_per_vertex"][n] + p)
    return ba, bs
