"""A numpy restatement of the textured albedo of the template rasteriser (sam6d_amd/csrc/s6d_raster.hip, "Texture" in its header)
for the texture tests.  Like tests/render_ref.py, from which it takes the float32 vertex stage and the integer edge functions, it is
pinned to no renderer: it restates the definition a second time,

  * the pyramid in integers (so a level is compared with ``equal``);
  * the (u, v) of a pixel and of its two neighbour samples, rho^2 and the bilinear value in float64 from the exact integer
    barycentrics of the winning face -- what the kernel's float32 operations approximate;

and it returns, per pixel, how far the float32 chain can be from these numbers (derivation in profiles/render_margins.md, "texture"):
``rho2_err`` bounds |rho2_f32 - rho2_f64|, ``uv_err`` the error of u and v.  A pixel whose rho2 lies within ``rho2_err`` of a
switch 2^(2L-1) may take either neighbouring level (``alt_level`` >= 0 there, ``rgb_alt`` the value at that level).
"""
import numpy as np

from tests import render_ref as R

U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------- pyramid
def lmax(Ht, Wt):
    return int(np.floor(np.log2(max(Ht, Wt))))


def level_size(side, l):
    return max(1, side >> l)


def pyramid(image):
    """(Ht,Wt,3) uint8 -> [level 0, ..., level Lmax], level l (H_l,W_l,3) uint8; integers."""
    lv = [np.asarray(image, np.uint8)]
    for _ in range(lmax(*lv[0].shape[:2])):
        s = lv[-1].astype(np.int64)
        hs, ws = s.shape[:2]
        hd, wd = max(1, hs >> 1), max(1, ws >> 1)
        j0, j1 = np.minimum(2 * np.arange(hd), hs - 1), np.minimum(2 * np.arange(hd) + 1, hs - 1)
        i0, i1 = np.minimum(2 * np.arange(wd), ws - 1), np.minimum(2 * np.arange(wd) + 1, ws - 1)
        d = (s[j0][:, i0] + s[j0][:, i1] + s[j1][:, i0] + s[j1][:, i1] + 2) >> 2
        lv.append(d.astype(np.uint8))
    return lv


def unpack(buffer, Ht, Wt):
    """The op's storage ((N,4) uint8: r g b 0 per texel, the levels one after another, row-major) -> the list ``pyramid`` gives."""
    buffer = np.asarray(buffer)
    out, at = [], 0
    for l in range(lmax(Ht, Wt) + 1):
        h, w = level_size(Ht, l), level_size(Wt, l)
        assert (buffer[at:at + h * w, 3] == 0).all()
        out.append(buffer[at:at + h * w, :3].reshape(h, w, 3))
        at += h * w
    assert at == len(buffer)
    return out


def bilinear(level, u, v):
    """The sampling of the definition in float64: level (H_L,W_L,3), u, v (N,) finite -> (N,3)."""
    hl, wl = level.shape[:2]
    t = level.astype(np.float64)
    uw, vw = u - np.floor(u), v - np.floor(v)
    x, y = uw * wl - 0.5, (1.0 - vw) * hl - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    ax, ay = (x - x0)[:, None], (y - y0)[:, None]
    i0, j0 = x0.astype(np.int64), y0.astype(np.int64)
    i0, j0 = np.where(i0 < 0, i0 + wl, i0), np.where(j0 < 0, j0 + hl, j0)
    i1, j1 = np.where(i0 + 1 == wl, 0, i0 + 1), np.where(j0 + 1 == hl, 0, j0 + 1)
    assert i0.min(initial=0) >= 0 and i0.max(initial=0) < wl and j0.min(initial=0) >= 0 and j0.max(initial=0) < hl
    top = t[j0, i0] + ax * (t[j0, i1] - t[j0, i0])
    bot = t[j1, i0] + ax * (t[j1, i1] - t[j1, i0])
    return top + ay * (bot - top)


def level_of(rho2, L):
    """clamp(floor(log2(rho) + 1/2), 0, Lmax) of float64 rho2 >= 0 (inf and NaN: Lmax): the level switches at 2^(2L-1)."""
    rho2 = np.asarray(rho2, np.float64)
    ok = np.isfinite(rho2) & (rho2 > 0)
    _, ex = np.frexp(np.where(ok, rho2, 1.0))          # rho2 = m 2^ex, m in [0.5, 1): floor(log2 rho2) = ex - 1
    lv = np.clip(ex >> 1, 0, L)                        # (e + 1) >> 1 with e = ex - 1
    return np.where(ok, lv, np.where(rho2 == 0, 0, L)).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------- render
def _attribute(b, a):
    """b (N,3) barycentrics (may be negative outside the triangle), a (3,) corner values -> value, and the bound of the float32
    value's error: 8 u (sum_k |b_k| |a_k| + (sum_k |b_k|) |value|)  (inside the triangle: <= 16 u sum_k b_k |a_k|, the xyz bound)."""
    val = b @ a
    return val, 8 * U * (np.abs(b) @ np.abs(a) + np.abs(b).sum(-1) * np.abs(val))


def render(vertices, faces, uv, image, poses, K, H, W, ambient, diffuse, znear):
    """The textured views: the geometry of ``render_ref.render`` (a dict with its entries, the colour ones recomputed) plus
    ``level`` (T,H,W) i32 (-1 on background), ``alt_level`` (T,H,W) i32 (-1: none), ``rgb_exact`` / ``rgb`` at ``level``,
    ``rgb_alt_exact`` at ``alt_level``, ``rho2``, ``rho2_err``, ``uv_tol`` (T,H,W): the colour bound of the uv error in levels,
    (du W_L + dv H_L) 255 shade at the finer of ``level`` and ``alt_level``."""
    vertices, faces, uv = np.asarray(vertices, R.F32), np.asarray(faces), np.asarray(uv, R.F32).astype(np.float64)
    image = np.asarray(image, np.uint8)
    Ht, Wt = image.shape[:2]
    L, lv = lmax(Ht, Wt), pyramid(image)
    fx, fy, cx, cy = K
    T = len(poses)
    geo = R.render(vertices, faces, np.full((len(vertices), 3), 255, np.uint8), poses, K, H, W, ambient, diffuse, znear)
    out = dict(geo, level=np.full((T, H, W), -1, np.int32), alt_level=np.full((T, H, W), -1, np.int32), rgb_exact=np.zeros((T, H, W, 3)),
               rgb_alt_exact=np.zeros((T, H, W, 3)), rho2=np.zeros((T, H, W)), rho2_err=np.zeros((T, H, W)), uv_tol=np.zeros((T, H, W)))
    for t in range(T):
        cam32, xi, yi, _ = R.vertex_stage(vertices, poses[t], fx, fy, cx, cy, znear)
        cam = cam32.astype(np.float64)
        for f in np.unique(geo["face"][t][geo["face"][t] >= 0]):
            tri = [int(i) for i in faces[f]]
            x, y = [int(a) for a in xi[tri]], [int(a) for a in yi[tri]]
            a2 = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
            s = 1 if a2 > 0 else -1
            pv, pu = np.nonzero(geo["face"][t] == f)

            def bary(du, dv):
                """Perspective-correct barycentrics at the samples (u + du, v + dv), and iz."""
                px, py = (pu + du).astype(np.int64) * 256, (pv + dv).astype(np.int64) * 256
                w = []
                for k in range(3):
                    a, b = (k + 1) % 3, (k + 2) % 3
                    w.append(s * (x[b] - x[a]) * (py - y[a]) - s * (y[b] - y[a]) * (px - x[a]))
                q = (np.stack(w, -1).astype(np.float64) / float(abs(a2))) / cam[tri, 2]
                iz = q.sum(-1)
                with np.errstate(all="ignore"):
                    return q / iz[:, None], iz
            b0, _ = bary(0, 0)
            bx, izx = bary(1, 0)
            by, izy = bary(0, 1)
            with np.errstate(all="ignore"):
                (u0, eu0), (v0, ev0) = _attribute(b0, uv[f, :, 0]), _attribute(b0, uv[f, :, 1])
                (ux, eux), (vx, evx) = _attribute(bx, uv[f, :, 0]), _attribute(bx, uv[f, :, 1])
                (uy, euy), (vy, evy) = _attribute(by, uv[f, :, 0]), _attribute(by, uv[f, :, 1])
                dxu, dxv, dyu, dyv = (ux - u0) * Wt, (vx - v0) * Ht, (uy - u0) * Wt, (vy - v0) * Ht
                # a difference and a product: one rounding each on top of the operands' errors
                exu, exv = (eux + eu0) * Wt + 2 * U * np.abs(dxu), (evx + ev0) * Ht + 2 * U * np.abs(dxv)
                eyu, eyv = (euy + eu0) * Wt + 2 * U * np.abs(dyu), (evy + ev0) * Ht + 2 * U * np.abs(dyv)
                rx, ry = dxu * dxu + dxv * dxv, dyu * dyu + dyv * dyv
                # (a + e)^2 - a^2 = 2 a e + e^2; two products and a sum: three more roundings
                erx = 2 * (np.abs(dxu) * exu + np.abs(dxv) * exv) + exu * exu + exv * exv + 3 * U * rx
                ery = 2 * (np.abs(dyu) * eyu + np.abs(dyv) * eyv) + eyu * eyu + eyv * eyv + 3 * U * ry
                finite = np.isfinite(u0) & np.isfinite(v0) & np.isfinite(ux) & np.isfinite(vx) & np.isfinite(uy) & np.isfinite(vy)
                rho2 = np.where((izx > 0) & (izy > 0) & finite, np.maximum(rx, ry), np.inf)
                err = np.where(np.isfinite(rho2), np.maximum(erx, ery), 0.0)
            lev = level_of(rho2, L)
            # the other level of a pixel within err of a switch 2^(2l-1), l = 1 .. L
            alt = np.full(len(pu), -1, np.int32)
            for l in range(1, L + 1):
                sw = 2.0 ** (2 * l - 1)
                near = np.isfinite(rho2) & (np.abs(rho2 - sw) <= err)
                alt = np.where(near, np.where(lev >= l, l - 1, l), alt).astype(np.int32)
            ok = np.isfinite(u0) & np.isfinite(v0)
            us, vs = np.where(ok, u0, 0.0), np.where(ok, v0, 0.0)
            # shading: the statement of render_ref.render
            pc = b0 @ cam[tri]
            n = np.cross(cam[tri[1]] - cam[tri[0]], cam[tri[2]] - cam[tri[0]])
            den = np.linalg.norm(n) * np.linalg.norm(pc, axis=-1)
            shade = ambient + diffuse * np.minimum(np.abs(pc @ n) / np.where(den > 0, den, 1.0), 1.0) * (den > 0)
            val, val_alt, tol = np.zeros((len(pu), 3)), np.zeros((len(pu), 3)), np.zeros(len(pu))
            for l in range(L + 1):
                for which, store in ((lev, val), (alt, val_alt)):
                    m = (which == l) & ok
                    if m.any():
                        store[m] = bilinear(lv[l], us[m], vs[m])
                m = np.minimum(lev, np.where(alt >= 0, alt, lev)) == l          # the finer of the two: the larger bound
                # uw, x: three roundings of values <= W_L on top of the error of u
                tol[m] = ((eu0[m] + 3 * U) * level_size(Wt, l) + (ev0[m] + 3 * U) * level_size(Ht, l)) * 255 * shade[m]
            out["level"][t, pv, pu], out["alt_level"][t, pv, pu] = lev, alt
            out["rgb_exact"][t, pv, pu] = np.clip(val * shade[:, None], 0, 255)
            out["rgb_alt_exact"][t, pv, pu] = np.clip(val_alt * shade[:, None], 0, 255)
            out["rho2"][t, pv, pu], out["rho2_err"][t, pv, pu] = rho2, err
            out["uv_tol"][t, pv, pu] = np.where(ok, tol, 0.0)
    out["rgb"] = np.rint(out["rgb_exact"]).astype(np.uint8)
    out["rgb_alt"] = np.rint(out["rgb_alt_exact"]).astype(np.uint8)
    return out


# ------------------------------------------------------------------------------------------------------------------- scenes
def texture(Ht, Wt, seed):
    return np.random.RandomState(seed).randint(0, 256, (Ht, Wt, 3)).astype(np.uint8)


def expand(vertex_uv, faces):
    """Per-vertex (V,2) -> per-corner (F,3,2)."""
    return np.ascontiguousarray(np.asarray(vertex_uv, R.F32)[np.asarray(faces)])


def cube_uv():
    """Per-corner UVs of ``render_ref.cube()``: every quad its own chart (scale and offset differ: seams on all twelve edges)."""
    uv = []
    for q in range(6):
        s, o = 0.5 + 0.25 * q, np.array([0.1 * q, -0.3 * q])
        c = [np.array(p) * s + o for p in ((0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0))]
        uv += [[c[0], c[1], c[2]], [c[0], c[3], c[2]]]
    return np.array(uv, R.F32)


def torus_uv(n_major=24, n_minor=12):
    """Per-vertex UVs of ``render_ref.torus()``: three turns of u around the ring, two of v around the tube; the faces that close
    the ring run backwards over the whole span (what per-vertex coordinates do at a seam): strongly minified."""
    i, j = np.meshgrid(np.arange(n_major), np.arange(n_minor), indexing="ij")
    return np.stack([3.0 * i / n_major, 2.0 * j / n_minor], -1).reshape(-1, 2).astype(R.F32)
