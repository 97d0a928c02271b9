"""Plain-loop restatement of the overlay pictures (the header of sam6d_amd/csrc/s6d_vis.hip), independent of
the kernels and of the torch statements of sam6d_amd/visualize.py: Python ints for every pixel operation (an int64 overflow in a
kernel shows as a difference), numpy float32 with one operation per statement for the projection.  Slow on purpose; the tests keep
the shapes small and compute a picture once."""
import numpy as np

F32 = np.float32
CLAMP_LO, CLAMP_HI = -8192, 8191
BOX_EDGES = [(4, 5), (5, 7), (6, 4), (7, 6)] + [(i, i + 4) for i in range(4)] + [(0, 1), (1, 3), (2, 0), (3, 2)]


def unpack(words, HW):
    """words (n_words,) int64 of one mask -> list of HW bools: bit k of word j is pixel 64 j + k."""
    return [bool((int(words[p >> 6]) >> (p & 63)) & 1) for p in range(HW)]


def rank_order(scores, frame, B, top=None):
    """Per frame the detection indices by score descending, then index ascending -> list of lists."""
    out = []
    for b in range(B):
        idx = [n for n in range(len(scores)) if int(frame[n]) == b]
        idx.sort(key=lambda n: (-float(scores[n]), n))
        out.append(idx if top is None else idx[:top])
    return out


def owner_from_masks(masks, ranked, H, W):
    """masks (N,H,W) bool, ranked = rank_order(...) -> owner (B,H,W) int: the covering detection of lowest rank, -1 for none."""
    owner = np.full((len(ranked), H, W), -1, np.int64)
    for b, idx in enumerate(ranked):
        for y in range(H):
            for x in range(W):
                for n in idx:
                    if masks[n][y][x]:
                        owner[b, y, x] = n
                        break
    return owner


def empty_canvas(B, H, W):
    return dict(zbuf=np.zeros((B, H, W), F32), owner=np.full((B, H, W), -1, np.int64), shade=np.zeros((B, H, W, 3), np.uint8))


def merge_layers(canvas, depth, rgb, frame, first):
    """In place: the nearest z > 0 wins, at equal z the lower instance index."""
    T, H, W = depth.shape
    for t in range(T):
        b, idx = int(frame[t]), first + t
        for y in range(H):
            for x in range(W):
                z = depth[t, y, x]
                if not (z > 0):
                    continue
                own, zb = int(canvas["owner"][b, y, x]), canvas["zbuf"][b, y, x]
                if own < 0 or z < zb or (z == zb and idx < own):
                    canvas["zbuf"][b, y, x], canvas["owner"][b, y, x], canvas["shade"][b, y, x] = z, idx, rgb[t, y, x]
    return canvas


def contour(owner):
    """owner (H,W) ints -> (H,W) bool: has an owner and a 4-neighbour inside the image with another owner (-1 counts)."""
    H, W = owner.shape
    out = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            o = int(owner[y, x])
            if o < 0:
                continue
            for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if 0 <= yy < H and 0 <= xx < W and max(int(owner[yy, xx]), -1) != o:
                    out[y, x] = True
    return out


def paint(image, owner, colors=None, shade=None, alpha=84, gray=True, edge_width=2, edge_color=(255, 255, 255)):
    """image (B,H,W,3) uint8, owner (B,H,W) -> (B,H,W,3) uint8."""
    B, H, W, _ = image.shape
    out = np.zeros((B, H, W, 3), np.uint8)
    for b in range(B):
        cont = contour(owner[b])
        for y in range(H):
            for x in range(W):
                px = [int(v) for v in image[b, y, x]]
                if gray:
                    px = [(4899 * px[0] + 9617 * px[1] + 1868 * px[2] + 8192) >> 14] * 3
                o = int(owner[b, y, x])
                if o >= 0:
                    c = shade[b, y, x] if shade is not None else colors[min(o, len(colors) - 1)]
                    px = [(alpha * int(c[k]) + (256 - alpha) * px[k] + 128) >> 8 for k in range(3)]
                if any(cont[y - j, x - i] for j in range(edge_width) for i in range(edge_width) if y - j >= 0 and x - i >= 0):
                    px = [int(v) for v in edge_color]
                out[b, y, x] = px
    return out


def project(points, inst, R, t, cams, znear):
    """float32, one rounding per operation -> (xy (M,2) int64, valid (M,) bool); invalid: pixel (0, 0)."""
    M = len(points)
    xy, valid = np.zeros((M, 2), np.int64), np.zeros(M, bool)
    with np.errstate(all="ignore"):
        for m in range(M):
            n = int(inst[m])
            if not 0 <= n < len(R):
                continue
            x, y, z = (F32(v) for v in points[m])
            r, tt = np.asarray(R[n], F32).reshape(9), np.asarray(t[n], F32)
            fx, fy, cx, cy = (F32(v) for v in cams[n])
            cam = []
            for a in range(3):
                p0 = F32(r[3 * a] * x)
                p1 = F32(r[3 * a + 1] * y)
                p2 = F32(r[3 * a + 2] * z)
                s = F32(p0 + p1)
                s = F32(s + p2)
                cam.append(F32(s + tt[a]))
            u = F32(F32(F32(fx * cam[0]) / cam[2]) + cx)
            v = F32(F32(F32(fy * cam[1]) / cam[2]) + cy)
            if cam[2] >= F32(znear) and np.isfinite(u) and np.isfinite(v):
                valid[m] = True
                xy[m] = [min(max(int(np.floor(float(u))), CLAMP_LO), CLAMP_HI), min(max(int(np.floor(float(v))), CLAMP_LO), CLAMP_HI)]
    return xy, valid


def covers(x0, y0, x1, y1, size, x, y):
    """Python ints: 4 times the squared distance of (x, y) to the segment is at most size^2."""
    dx, dy, ax, ay = x1 - x0, y1 - y0, x - x0, y - y0
    L, uu, s2 = dx * dx + dy * dy, ax * dx + ay * dy, size * size
    if L == 0 or uu <= 0:
        return 4 * (ax * ax + ay * ay) <= s2
    if uu >= L:
        return 4 * ((x - x1) ** 2 + (y - y1) ** 2) <= s2
    cr = ax * dy - ay * dx
    return 4 * cr * cr <= s2 * L


def draw(image, prims):
    """image (B,H,W,3) uint8 (copied), prims: rows (frame, x0, y0, x1, y1, size, rgb word, valid) in painter's order."""
    out = image.copy()
    B, H, W, _ = image.shape
    for e in prims:
        b, x0, y0, x1, y1, size, rgb, ok = (int(v) for v in e)
        if not ok or not 0 <= b < B or not 0 <= size <= 64 or not all(CLAMP_LO <= v <= CLAMP_HI for v in (x0, y0, x1, y1)):
            continue
        r = (size + 1) // 2
        for y in range(max(0, min(y0, y1) - r), min(H, max(y0, y1) + r + 1)):          # outside this box nothing is within size / 2
            for x in range(max(0, min(x0, x1) - r), min(W, max(x0, x1) + r + 1)):
                if covers(x0, y0, x1, y1, size, x, y):
                    out[b, y, x] = [rgb & 255, (rgb >> 8) & 255, (rgb >> 16) & 255]
    return out


def box_corners(vertices, center="extent"):
    v = np.asarray(vertices, F32)
    lo, hi = v.min(0), v.max(0)
    half = ((hi - lo) / F32(2)).astype(F32)
    c = (lo + half).astype(F32) if center == "extent" else v.astype(np.float64).mean(0).astype(F32)
    return np.stack([c + half * np.array([-1 if k & 2 else 1, -1 if k & 4 else 1, -1 if k & 1 else 1], F32) for k in range(8)]).astype(F32)


def model_points(vertices):
    v = np.asarray(vertices, F32)
    return v[::max(1, len(v) // 512)][:512]


def pose_primitives(models, obj_ids, R, t, cams, frame, colors, mode, center="extent", znear=1.0):
    """Per instance in list order: ground edges int(0.3 c), pillars int(0.6 c), top edges c (size 3), then the points (size 2)."""
    prims = []
    for n, o in enumerate(obj_ids):
        c = [int(v) for v in colors[n]]
        word = lambda col: col[0] | (col[1] << 8) | (col[2] << 16)
        if "box" in mode:
            xy, ok = project(box_corners(models[o]["vertices"], center), [n] * 8, R, t, cams, znear)
            for k, (i, j) in enumerate(BOX_EDGES):
                s = (0.3, 0.6, 1.0)[k // 4]
                col = c if s == 1.0 else [int(s * v) for v in c]
                prims.append([int(frame[n]), *xy[i], *xy[j], 3, word(col), int(ok[i] and ok[j])])
        if "points" in mode:
            pts = model_points(models[o]["vertices"])
            xy, ok = project(pts, [n] * len(pts), R, t, cams, znear)
            prims += [[int(frame[n]), *xy[m], *xy[m], 2, word(c), int(ok[m])] for m in range(len(pts))]
    return np.asarray(prims, np.int64).reshape(-1, 8)
