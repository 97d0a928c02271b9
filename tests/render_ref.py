"""A numpy restatement of the template rasteriser (sam6d_amd/csrc/s6d_raster.hip) for the render tests.

It is NOT pinned to any renderer: neither BlenderProc nor pyrender (the reference's two) can be reproduced pixel for pixel, and
none of them is used here.  It restates the DEFINITION in the kernel source's header a second time, independently:

  * the vertex stage in numpy float32, operation by operation in the stated order (so the snapped integer coordinates and the
    float32 camera-space vertices are the kernel's, bit for bit);
  * coverage by the same integer rule (int64 edge functions on the snapped coordinates, winding normalised by the sign of the
    doubled area, top-left fill rule, zero-area triangles cover nothing, no clipping: a triangle with a vertex at Z <= znear or a
    snapped coordinate beyond 2^23 is skipped whole and counted);
  * interpolation and shading in float64 from the exact integer barycentrics -- what the kernel's float32 operations approximate,
    the bounds of profiles/render_margins.md being the distance allowed.

Per pixel it also returns the nearest and the second-nearest depth among the covering faces (``z1``, ``z2``; inf where there is
none) and their number (``layers``): the tests assert on these alone that the visible face is decided by a margin far above the
kernel's depth rounding before they demand ``face`` exactly.
"""
import numpy as np

F32 = np.float32
SNAP_LIMIT = 2 ** 23
LARGE_BOX = 256          # samples of the clamped box above which the kernel hands the triangle to a workgroup


def vertex_stage(vertices, pose, fx, fy, cx, cy, znear):
    """-> cam (V,3) float32, xi, yi (V,) int64, ok (V,) bool: the float32 statement of the kernel, one rounding per operation."""
    v, P = np.asarray(vertices, F32), np.asarray(pose, F32)
    cam = np.stack([((P[r, 0] * v[:, 0] + P[r, 1] * v[:, 1]) + P[r, 2] * v[:, 2]) + P[r, 3] for r in range(3)], 1)
    assert cam.dtype == F32
    Z = cam[:, 2]
    with np.errstate(all="ignore"):
        xs = ((F32(fx) * cam[:, 0]) / Z + F32(cx)) * F32(256)
        ys = ((F32(fy) * cam[:, 1]) / Z + F32(cy)) * F32(256)
        ok = (Z > F32(znear)) & (np.abs(xs) <= F32(SNAP_LIMIT)) & (np.abs(ys) <= F32(SNAP_LIMIT))
    xi = np.rint(np.where(ok, xs, 0)).astype(np.int64)
    yi = np.rint(np.where(ok, ys, 0)).astype(np.int64)
    return cam, xi, yi, ok


def clamped_box(x, y, H, W):
    """The inclusive sample box of a triangle with snapped coordinates x, y (3,), clamped to the image."""
    u0, u1 = max(0, -((-int(x.min())) // 256)), min(W - 1, int(x.max()) // 256)
    v0, v1 = max(0, -((-int(y.min())) // 256)), min(H - 1, int(y.max()) // 256)
    return u0, u1, v0, v1


def render(vertices, faces, colors, poses, K, H, W, ambient, diffuse, znear):
    """-> dict of (T,H,W[,3]) arrays: mask u8, face i32, depth f64, xyz f64, xyz_scale f64 (sum_k b_k |a_k| of the winning face:
    the factor of the xyz bound), rgb u8, rgb_exact f64 (before rounding), z1, z2 f64, layers i32; and skipped (T,) i32,
    large (T,) i32 = triangles over the workgroup threshold."""
    vertices, faces, colors, poses = np.asarray(vertices, F32), np.asarray(faces), np.asarray(colors), np.asarray(poses, F32)
    T = len(poses)
    fx, fy, cx, cy = K
    out = dict(mask=np.zeros((T, H, W), np.uint8), face=np.full((T, H, W), -1, np.int32), depth=np.zeros((T, H, W)),
               xyz=np.zeros((T, H, W, 3)), xyz_scale=np.zeros((T, H, W, 3)), rgb=np.zeros((T, H, W, 3), np.uint8),
               rgb_exact=np.zeros((T, H, W, 3)), z1=np.full((T, H, W), np.inf), z2=np.full((T, H, W), np.inf),
               layers=np.zeros((T, H, W), np.int32), skipped=np.zeros(T, np.int32), large=np.zeros(T, np.int32))
    vm, vc = vertices.astype(np.float64), colors.astype(np.float64)
    for t in range(T):
        cam32, xi, yi, ok = vertex_stage(vertices, poses[t], fx, fy, cx, cy, znear)
        cam = cam32.astype(np.float64)
        z1, z2, layers, face = out["z1"][t], out["z2"][t], out["layers"][t], out["face"][t]
        for f, tri in enumerate(faces):
            tri = [int(i) for i in tri]
            if not all(ok[i] for i in tri):
                out["skipped"][t] += 1
                continue
            x, y = xi[tri], yi[tri]
            a2 = int((x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0]))
            if a2 == 0:
                continue
            s = 1 if a2 > 0 else -1
            u0, u1, v0, v1 = clamped_box(x, y, H, W)
            if u0 > u1 or v0 > v1:
                continue
            out["large"][t] += (u1 - u0 + 1) * (v1 - v0 + 1) > LARGE_BOX
            px, py = np.meshgrid(np.arange(u0, u1 + 1, dtype=np.int64) * 256, np.arange(v0, v1 + 1, dtype=np.int64) * 256)
            w, inside = [], np.ones(px.shape, bool)
            for k in range(3):
                a, b = (k + 1) % 3, (k + 2) % 3
                dx, dy = s * int(x[b] - x[a]), s * int(y[b] - y[a])
                wk = dx * (py - int(y[a])) - dy * (px - int(x[a]))
                own = dy < 0 or (dy == 0 and dx > 0)
                inside &= (wk > 0) | ((wk == 0) & own)
                w.append(wk)
            if not inside.any():
                continue
            lam = np.stack(w, -1).astype(np.float64) / float(abs(a2))          # exact integers below 2^53
            q = lam / cam[tri, 2]
            iz = q.sum(-1)
            z = np.where(inside, 1.0 / np.where(inside, iz, 1.0), np.inf)
            sl = (slice(v0, v1 + 1), slice(u0, u1 + 1))
            layers[sl] += inside
            o1, o2 = z1[sl], z2[sl]
            wins = z < o1                                                      # ascending f: a tie stays with the lower index
            z2[sl] = np.where(wins, o1, np.minimum(o2, z))
            z1[sl] = np.where(wins, z, o1)
            if not wins.any():
                continue
            b = q / np.where(inside, iz, 1.0)[..., None]                       # perspective-correct barycentrics
            pc = b @ cam[tri]
            n = np.cross(cam[tri[1]] - cam[tri[0]], cam[tri[2]] - cam[tri[0]])
            den = np.linalg.norm(n) * np.linalg.norm(pc, axis=-1)
            cosine = np.minimum(np.abs(pc @ n) / np.where(den > 0, den, 1.0), 1.0) * (den > 0)
            val = np.clip((b @ vc[tri]) * (ambient + diffuse * cosine)[..., None], 0.0, 255.0)
            for name, new in (("depth", z), ("xyz", b @ vm[tri]), ("xyz_scale", b @ np.abs(vm[tri])), ("rgb_exact", val)):
                view = out[name][t][sl]
                view[wins] = new[wins]
            face[sl][wins] = f
    out["mask"][out["face"] >= 0] = 255
    out["rgb"] = np.rint(out["rgb_exact"]).astype(np.uint8)
    return out


# ------------------------------------------------------------------------------------------------------------------- meshes
def torus(n_major=24, n_minor=12, R=60.0, r=25.0):
    """A closed torus, 2 * n_major * n_minor faces, consistent winding; colours vary over the surface."""
    a = np.arange(n_major) * (2 * np.pi / n_major)
    b = np.arange(n_minor) * (2 * np.pi / n_minor)
    A, B = np.meshgrid(a, b, indexing="ij")
    v = np.stack([(R + r * np.cos(B)) * np.cos(A), (R + r * np.cos(B)) * np.sin(A), r * np.sin(B)], -1).reshape(-1, 3)
    idx = lambda i, j: (i % n_major) * n_minor + (j % n_minor)          # noqa: E731
    faces = []
    for i in range(n_major):
        for j in range(n_minor):
            faces += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    col = np.stack([128 + 100 * np.cos(A), 128 + 100 * np.sin(B), 60 + 0 * A], -1).reshape(-1, 3)
    return v.astype(F32), np.array(faces, np.int32), np.rint(col).astype(np.uint8)


def cube(h=50.0):
    """A closed cube of half-side h, 12 faces; every other face is wound the other way (the kernel does not cull)."""
    v = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], F32)
    quads = [[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]]
    faces = []
    for q in quads:
        faces += [[q[0], q[1], q[2]], [q[0], q[3], q[2]]]               # the second triangle wound the other way
    col = np.array([[40 + 25 * i, 250 - 20 * i, 90 + 10 * i] for i in range(8)], np.uint8)
    return v, np.array(faces, np.int32), col


def rotations(n, seed):
    """n rotation matrices from a seeded generator (QR of a normal matrix, determinant fixed to +1)."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        q, r = np.linalg.qr(rs.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out.append(q)
    return np.stack(out)


def poses(n, seed, t=(3.0, -2.0, 400.0)):
    P = np.tile(np.eye(4, dtype=F32), (n, 1, 1))
    P[:, :3, :3] = rotations(n, seed)
    P[:, :3, 3] = t
    return P
