"""A numpy restatement of the BOP ground-truth derivation for its tests, written from the DEFINITIONS (the issue text that
sam6d_amd/csrc/s6d_bopgt.hip's header also states), not from the kernel source: a loop over the instances, vectorised pixels, no
kernels and no torch.

bop_toolkit is not present and nothing here is pinned to it.  Two modes:

  * ``np.float32``: every operation in float32 in the stated order (numpy rounds each array operation once, divisions and square
    roots correctly): the kernels must give these bits;
  * ``np.float64``: the same formulas on the same float32 inputs, widened.  It also reports the UNDECIDED pixels: those whose
    Dg - Dt lies within 8 u (|Dg| + |Dt|) of delta (u = 2^-24; the bound tests/test_gpu_bop_eval.py derives for this statement:
    two roundings in a and b, five in r, one each in Dg, Dt and the difference, first order, rounded up) -- only there may a
    float32 evaluation decide otherwise.
"""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
EMPTY = (INT_MAX, INT_MAX, INT_MIN, INT_MIN)


def _extent(where, x0, y0):
    """Inclusive xmin ymin xmax ymax of a boolean (rows, columns) array whose pixel (0, 0) has coordinates (x0, y0); EMPTY for none."""
    ys, xs = np.nonzero(where)
    if len(ys) == 0:
        return EMPTY
    return (int(xs.min()) + x0, int(ys.min()) + y0, int(xs.max()) + x0, int(ys.max()) + y0)


def gt_visibility(canvas, depth_test, test_index, cams, delta, margin=(0, 0), dt=np.float32):
    """canvas (N, H + 2 my, W + 2 mx), depth_test (M,H,W), test_index (N,), cams (N,4), margin (mx, my) -> dict: mask, mask_visib
    (N,H,W) uint8; counts (N,4) int64 = all, in-image, valid, visib; extents (N,2,4) int64 (row 0 all, row 1 visib; EMPTY for an
    empty set); in float64 mode also ``undecided`` (N,H,W) bool."""
    canvas, depth_test = np.asarray(canvas, np.float32), np.asarray(depth_test, np.float32)
    cams = np.asarray(cams, np.float32).astype(dt)
    mx, my = margin
    M, H, W = depth_test.shape
    N = canvas.shape[0]
    assert canvas.shape[1:] == (H + 2 * my, W + 2 * mx)
    delta = dt(np.float32(delta))
    u, v = np.arange(W).astype(dt)[None, :], np.arange(H).astype(dt)[:, None]
    out = dict(mask=np.zeros((N, H, W), np.uint8), mask_visib=np.zeros((N, H, W), np.uint8), counts=np.zeros((N, 4), np.int64),
               extents=np.zeros((N, 2, 4), np.int64))
    if dt is np.float64:
        out["undecided"] = np.zeros((N, H, W), bool)
    for n in range(N):
        every = canvas[n] > 0
        zg = canvas[n, my:my + H, mx:mx + W].astype(dt)
        zt = depth_test[int(test_index[n])].astype(dt)
        fx, fy, cx, cy = cams[n]
        with np.errstate(all="ignore"):
            a, b = (u - cx) / fx, (v - cy) / fy
            r = np.sqrt((a * a + b * b) + dt(1))
            Dg, Dt = zg * r, zt * r
            mask = zg > 0
            valid = mask & (zt > 0)
            visib = mask & (((Dg - Dt) <= delta) | (zt == 0))
            if dt is np.float64:
                out["undecided"][n] = mask & (zt != 0) & (np.abs((Dg - Dt) - delta) <= 8 * U * (np.abs(Dg) + np.abs(Dt)))
        out["mask"][n], out["mask_visib"][n] = mask, visib
        out["counts"][n] = (every.sum(), mask.sum(), valid.sum(), visib.sum())
        out["extents"][n, 0] = _extent(every, -mx, -my)
        out["extents"][n, 1] = _extent(visib, 0, 0)
    return out


def diameter(vertices, dt=np.float32, tile=256):
    """The largest vertex distance: a plain double loop over tiles of the pairs; d2 = (dx dx + dy dy) + dz dz in dt, a d2 that is
    not finite counts as +inf, one square root of the maximum."""
    v = np.asarray(vertices, np.float32).astype(dt)
    V = len(v)
    best = dt(0)
    with np.errstate(all="ignore"):
        for i0 in range(0, V, tile):
            a = v[i0:i0 + tile, None, :]
            for j0 in range(i0, V, tile):
                b = v[None, j0:j0 + tile, :]
                dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
                d2 = (dx * dx + dy * dy) + dz * dz
                d2 = np.where(np.isfinite(d2), d2, dt(np.inf))
                best = max(best, d2.max())
        return dt(np.sqrt(dt(best)))


def visib_fract(counts):
    """px_count_visib / px_count_all in float64, 0 when the denominator is 0."""
    c = np.asarray(counts, np.float64)
    with np.errstate(all="ignore"):
        return np.where(c[:, 0] > 0, c[:, 3] / c[:, 0], 0.0)
