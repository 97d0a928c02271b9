"""Overlay pictures: the detections and the poses of a group of frames drawn over the frames, on the device.

The reference ends its demo with two pictures drawn on the host with cv2, skimage, scipy and distinctipy -- the best mask blended
over the grey frame with its edge in white, and the projected 3-D box and 512 model points of every instance.  None of those
libraries is part of this project.  The pictures here are this project's own DEFINITION, stated operation by operation in the header
of csrc/s6d_vis.hip, all integer and exact after the projection; tests/vis_ref.py restates it independently.  No picture is claimed
to equal cv2's.

  palette              a fixed integer formula: entry k depends on k alone
  overlay_detections   owner map from masks (dense, run-length or packed) -> blend + contours
  overlay_poses        box edges and model points as primitives; ``"surface"``: the rendered silhouettes merged by depth, painted
  overlay_results      both pictures per frame from what ``FramePipeline.run_group`` returned
  side_by_side, save_png

Batched throughout: (B,H,W,3) in and out, detections and instances carry their frame, and a frame has the same bits alone and in a
group.  Device tensors go to the kernels; host tensors to the torch statements below through ``policy.guard`` (sites
``visualize.owner``, ``visualize.paint``, ``visualize.draw``): under strict mode a fall-back on the device is an error.
"""
import numpy as np
import torch

from . import ops, policy
from .ism import handoff

ALPHA = 84                                                                 # 0.33 of the reference, in 1/256 units
CLAMP_LO, CLAMP_HI = ops.VIS_CLAMP
BOX_EDGES = ((4, 5), (5, 7), (6, 4), (7, 6), (0, 4), (1, 5), (2, 6), (3, 7), (0, 1), (1, 3), (2, 0), (3, 2))   # ground, pillars, top
BOX_SHADE = (0.3,) * 4 + (0.6,) * 4 + (1.0,) * 4
BOX_SIZE, POINT_SIZE, MAX_POINTS = 3, 2, 512                               # a disc of radius 1 is size 2


def _kernels(site, t, *names):
    return policy.guard(site, cuda=t.is_cuda, have=all(ops.have(n) for n in names))


# ------------------------------------------------------------------------------------------------------------------- palette
_VALUE = (255, 200, 150)


def palette(n):
    """(n,3) uint8 colours, entry k a function of k alone: the hue wheel at h = 137 k mod 360 degrees (the golden angle, so that
    neighbours in the list are far apart on the wheel) at full saturation -- sector s = h // 60, f = h % 60, rising x = (255 f + 30)
    // 60, falling 255 - x: (255, x, 0), (255 - x, 255, 0), (0, 255, x), (0, 255 - x, 255), (x, 0, 255), (255, 0, 255 - x) for
    s = 0 .. 5 -- scaled channel by channel to the value v = (255, 200, 150)[(k // 12) % 3] as (c v + 127) // 255.  Entry 0 is
    (255, 0, 0), the reference's colour for a single object."""
    out = np.zeros((int(n), 3), np.uint8)
    for k in range(int(n)):
        h = (137 * k) % 360
        s, f = h // 60, h % 60
        x = (255 * f + 30) // 60
        rgb = ((255, x, 0), (255 - x, 255, 0), (0, 255, x), (0, 255 - x, 255), (x, 0, 255), (255, 0, 255 - x))[s]
        v = _VALUE[(k // 12) % 3]
        out[k] = [(c * v + 127) // 255 for c in rgb]
    return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------------------------------- torch statements
def _unpack_library(packed, HW):
    """(N,words) int64 -> (N,HW) bool: bit k of word j is pixel 64 j + k."""
    shifts = torch.arange(64, device=packed.device)
    return (((packed[:, :, None] >> shifts) & 1) != 0).reshape(packed.shape[0], -1)[:, :HW]


def _owner_library(packed, order, frame_start, H, W):
    """The library statement of ``ops.vis_owner_from_masks``."""
    B, dev = frame_start.shape[0] - 1, packed.device
    owner = torch.full((B, H * W), -1, dtype=torch.int32, device=dev)
    fs = frame_start.cpu().tolist()
    for b in range(B):
        sel = order[fs[b]:fs[b + 1]].long()
        n = sel.shape[0]
        if n == 0:
            continue
        cover = _unpack_library(packed[sel], H * W)
        rank = torch.arange(n, device=dev)[:, None]
        first = torch.where(cover, rank, torch.full_like(rank, n)).amin(0)
        owner[b] = torch.where(first < n, sel[first.clamp(max=n - 1)], torch.full_like(first, -1)).int()
    return owner.reshape(B, H, W)


def _merge_library(canvas, depth, rgb, frame, first):
    """The library statement of ``ops.vis_merge_layers`` (in place)."""
    zb, own, shade = canvas["zbuf"], canvas["owner"], canvas["shade"]
    for t, b in enumerate(frame.cpu().tolist()):
        z, idx = depth[t], first + t
        better = (z > 0) & ((own[b] < 0) | (z < zb[b]) | ((z == zb[b]) & (idx < own[b])))
        zb[b] = torch.where(better, z, zb[b])
        own[b] = torch.where(better, torch.full_like(own[b], idx), own[b])
        shade[b] = torch.where(better[..., None], rgb[t], shade[b])
    return canvas


def _contour_library(owner):
    own = torch.where(owner < 0, torch.full_like(owner, -1), owner)
    pad = torch.nn.functional.pad(own, (1, 1, 1, 1), value=-2)
    c = pad[:, 1:-1, 1:-1]
    cont = torch.zeros_like(own, dtype=torch.bool)
    for nb in (pad[:, :-2, 1:-1], pad[:, 2:, 1:-1], pad[:, 1:-1, :-2], pad[:, 1:-1, 2:]):
        cont |= (nb != -2) & (nb != c)
    return cont & (own >= 0), own


def _paint_library(image, owner, colors, shade, alpha, gray, edge_width, edge_color):
    """The library statement of ``ops.vis_paint``."""
    B, H, W, _ = image.shape
    base = image.int()
    if gray:
        y = (4899 * base[..., 0] + 9617 * base[..., 1] + 1868 * base[..., 2] + 8192) >> 14
        base = y[..., None].expand(B, H, W, 3)
    cont, own = _contour_library(owner)
    c = shade.int() if shade is not None else colors.int()[own.clamp(min=0, max=colors.shape[0] - 1).long()]
    out = torch.where((own >= 0)[..., None], (alpha * c + (256 - alpha) * base + 128) >> 8, base)
    edge = torch.zeros_like(cont)
    for j in range(edge_width):
        for i in range(edge_width):
            edge[:, j:, i:] |= cont[:, :H - j, :W - i]
    out = torch.where(edge[..., None], torch.tensor([int(v) for v in edge_color], dtype=torch.int32, device=image.device), out)
    return out.to(torch.uint8)


def _project_library(points, inst, R, t, cams, znear):
    """The library statement of ``ops.vis_project``: every float32 operation a statement of its own."""
    N = R.shape[0]
    inside = (inst >= 0) & (inst < N)
    n = inst.long().clamp(0, max(N - 1, 0))
    if N == 0:
        return torch.zeros(points.shape[0], 2, dtype=torch.int32, device=points.device), torch.zeros(points.shape[0], dtype=torch.uint8, device=points.device)
    r, tt, k = R.reshape(N, 9)[n], t[n], cams[n]
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    cam = []
    for a in range(3):
        s = r[:, 3 * a] * x
        s = s + r[:, 3 * a + 1] * y
        s = s + r[:, 3 * a + 2] * z
        cam.append(s + tt[:, a])
    u = (k[:, 0] * cam[0]) / cam[2] + k[:, 2]
    v = (k[:, 1] * cam[1]) / cam[2] + k[:, 3]
    valid = inside & (cam[2] >= znear) & torch.isfinite(u) & torch.isfinite(v)

    def pixel(f):
        f = torch.where(valid, f, torch.zeros_like(f))
        return torch.floor(f).clamp(CLAMP_LO, CLAMP_HI).int()
    return torch.stack([pixel(u), pixel(v)], 1), valid.to(torch.uint8)


def _draw_library(image, prims, frame_start, chunk_elems=1 << 22):
    """The library statement of ``ops.vis_draw`` (in place): int64 coverage of a chunk of primitives over the whole frame."""
    B, H, W, _ = image.shape
    dev = image.device
    fs = frame_start.cpu().tolist()
    ys = torch.arange(H, device=dev, dtype=torch.int64)[None, :, None]
    xs = torch.arange(W, device=dev, dtype=torch.int64)[None, None, :]
    step = max(1, chunk_elems // (H * W))
    for b in range(B):
        for c0 in range(fs[b], fs[b + 1], step):
            e = prims[c0:min(c0 + step, fs[b + 1])].long()
            x0, y0, x1, y1, size = (e[:, k, None, None] for k in range(1, 6))
            ok = (e[:, 0] == b) & (e[:, 7] != 0) & (e[:, 5] >= 0) & (e[:, 5] <= 64) & (e[:, 1:5] >= CLAMP_LO).all(1) & (e[:, 1:5] <= CLAMP_HI).all(1)
            dx, dy, ax, ay, bx, by = x1 - x0, y1 - y0, xs - x0, ys - y0, xs - x1, ys - y1
            L, uu, s2 = dx * dx + dy * dy, ax * dx + ay * dy, size * size
            cr = ax * dy - ay * dx
            cover = torch.where((L == 0) | (uu <= 0), 4 * (ax * ax + ay * ay) <= s2,
                                torch.where(uu >= L, 4 * (bx * bx + by * by) <= s2, 4 * cr * cr <= s2 * L)) & ok[:, None, None]
            idx = torch.arange(e.shape[0], device=dev)[:, None, None]
            last = torch.where(cover, idx, torch.full_like(idx, -1)).amax(0)
            rgb = e[:, 6][last.clamp(min=0)]
            col = torch.stack([rgb & 255, (rgb >> 8) & 255, (rgb >> 16) & 255], -1).to(torch.uint8)
            image[b] = torch.where((last >= 0)[..., None], col, image[b])
    return image


# ------------------------------------------------------------------------------------------------------------------- dispatch
def owner_from_masks(packed, order, frame_start, H, W):
    if _kernels("visualize.owner", packed, "vis_owner_from_masks"):
        return ops.vis_owner_from_masks(packed.contiguous(), order.contiguous(), frame_start.contiguous(), H, W)
    if packed.shape[1] != (H * W + 63) // 64:
        raise ValueError(f"packed must have ceil(H W / 64) = {(H * W + 63) // 64} words per mask, got {packed.shape[1]}")
    return _owner_library(packed, order, frame_start, H, W)


def paint(image, owner, colors=None, shade=None, alpha=ALPHA, gray=True, edge_width=2, edge_color=(255, 255, 255)):
    if not 0 <= int(alpha) <= 256:
        raise ValueError(f"alpha must lie in [0, 256] (units of 1/256), got {alpha}")
    if not 0 <= int(edge_width) <= 4:
        raise ValueError(f"edge_width must lie in [0, 4], got {edge_width}")
    if max(image.shape[1:3]) > ops.VIS_MAX_HW:
        raise ValueError(f"H and W must lie in [1, {ops.VIS_MAX_HW}], got H = {image.shape[1]}, W = {image.shape[2]}")
    if _kernels("visualize.paint", image, "vis_paint"):
        return ops.vis_paint(image.contiguous(), owner.contiguous(), colors, shade, alpha, gray, edge_width, edge_color)
    return _paint_library(image, owner, colors, shade, int(alpha), gray, int(edge_width), edge_color)


def project(points, inst, R, t, cams, znear):
    if _kernels("visualize.draw", points, "vis_project"):
        return ops.vis_project(points.contiguous(), inst.contiguous(), R.contiguous(), t.contiguous(), cams.contiguous(), znear)
    return _project_library(points, inst, R, t, cams, float(znear))


def draw(image, prims, frame=None):
    """Draws the flat primitive list ``prims`` (P,8) int32 (frame, x0, y0, x1, y1, size, r | g << 8 | b << 16, valid) into ``image``
    (B,H,W,3) IN PLACE, in painter's order.  The list is sorted by frame here (a stable sort: the list order inside a frame
    stays)."""
    B, H, W, _ = image.shape
    if max(H, W) > ops.VIS_MAX_HW:
        raise ValueError(f"H and W must lie in [1, {ops.VIS_MAX_HW}], got H = {H}, W = {W}")
    P = prims.shape[0]
    if P:
        if int(prims[:, 5].min()) < 0 or int(prims[:, 5].max()) > 64:
            raise ValueError(f"size must lie in [0, 64], got [{int(prims[:, 5].min())}, {int(prims[:, 5].max())}]")
        if int(prims[:, 0].min()) < 0 or int(prims[:, 0].max()) >= B:
            raise ValueError(f"frame must lie in [0, {B}), got [{int(prims[:, 0].min())}, {int(prims[:, 0].max())}]")
    prims = prims[torch.sort(prims[:, 0], stable=True).indices].contiguous()
    frame_start = _starts(prims[:, 0].long(), B)
    if _kernels("visualize.draw", image, "vis_draw"):
        return ops.vis_draw(image, prims, frame_start, check=False)
    return _draw_library(image, prims, frame_start)


def _starts(frame, B):
    start = torch.zeros(B + 1, dtype=torch.int64, device=frame.device)
    start[1:] = torch.cumsum(torch.bincount(frame, minlength=B)[:B], 0)
    return start


def _frames(image_u8):
    img = torch.as_tensor(image_u8)
    single = img.dim() == 3
    img = img[None] if single else img
    if img.dim() != 4 or img.shape[3] != 3 or img.dtype != torch.uint8:
        raise ValueError(f"image_u8 must be (B,H,W,3) or (H,W,3) uint8, got {tuple(img.shape)} {img.dtype}")
    if not (1 <= img.shape[1] <= ops.VIS_MAX_HW and 1 <= img.shape[2] <= ops.VIS_MAX_HW):
        raise ValueError(f"H and W must lie in [1, {ops.VIS_MAX_HW}], got H = {img.shape[1]}, W = {img.shape[2]}")
    return img.contiguous(), single


def _frame_index(frame_index, N, B, dev):
    if frame_index is None:
        if B != 1 and N:
            raise ValueError(f"frame_index is needed for a group of {B} frames")
        return torch.zeros(N, dtype=torch.int64, device=dev)
    f = torch.as_tensor(frame_index).to(dev).long().reshape(-1)
    if f.shape[0] != N:
        raise ValueError(f"frame_index must have one entry per instance ({N}), got {f.shape[0]}")
    if N and (int(f.min()) < 0 or int(f.max()) >= B):
        raise ValueError(f"frame_index must lie in [0, {B}), got [{int(f.min())}, {int(f.max())}]")
    return f


# ------------------------------------------------------------------------------------------------------------------- detections
def _packed(masks, H, W, dev):
    """Dense (N,H,W), ``RleMasks``, ``Detections`` or packed words (N, ceil(H W / 64)) int64 -> packed words on ``dev``; no dense
    mask is made of run lists or words."""
    if isinstance(masks, handoff.Detections):
        masks = masks.masks
    if isinstance(masks, handoff.RleMasks):
        if tuple(masks.size) != (H, W):
            raise ValueError(f"masks of size {tuple(masks.size)} for frames of {(H, W)}")
        return masks.to(dev).packed()[0]
    m = torch.as_tensor(masks).to(dev)
    if m.dtype == torch.int64 and m.dim() == 2:
        if m.shape[1] != (H * W + 63) // 64:
            raise ValueError(f"packed masks must have ceil(H W / 64) = {(H * W + 63) // 64} words per mask, got {m.shape[1]}")
        return m.contiguous()
    if m.dim() != 3 or tuple(m.shape[1:]) != (H, W):
        raise ValueError(f"masks must be (N,{H},{W}), run lists or packed words, got {tuple(m.shape)}")
    if m.dtype not in (torch.bool, torch.uint8):
        m = m > 0
    if m.shape[0] == 0:
        return torch.zeros(0, (H * W + 63) // 64, dtype=torch.int64, device=dev)
    if _kernels("visualize.owner", m, "mask_pack"):
        return ops.mask_pack(m.contiguous())[0]
    return handoff._pack_library(m.to(torch.uint8))[0]


def rank_detections(scores, frame, B, top=None):
    """-> (order (K,) int32, frame_start (B+1,) int64, rank (K,) int64): the detections frame by frame, inside a frame by score
    descending, then index ascending (two stable sorts); ``top`` keeps the first ``top`` of every frame."""
    by_score = torch.sort(scores, descending=True, stable=True).indices
    order = by_score[torch.sort(frame[by_score], stable=True).indices]
    start = _starts(frame, B)
    rank = torch.arange(order.shape[0], device=order.device) - start[frame[order]]
    if top is not None:
        if int(top) < 0:
            raise ValueError(f"top must be >= 0, got {top}")
        keep = rank < int(top)
        order, rank = order[keep], rank[keep]
        start = _starts(frame[order], B)
    return order.int().contiguous(), start, rank


@torch.no_grad()
def overlay_detections(image_u8, masks, scores=None, *, frame_index=None, colors=None, alpha=ALPHA, gray=True, edge_width=2, top=None,
                       edge_color=(255, 255, 255)):
    """The detections blended over the frames with their contours in ``edge_color``.

    ``image_u8`` (B,H,W,3) uint8 (or (H,W,3): one frame, and the picture comes back without the batch axis).  ``masks``: (N,H,W)
    bool / uint8, ``handoff.RleMasks``, packed words (N, ceil(H W / 64)) int64 or ``handoff.Detections`` (whose scores are the
    default) of the detections of ALL frames, ``frame_index`` (N,) saying which frame each belongs to (not needed for one frame);
    or a list with one such entry per frame (``scores`` then a list too, or None for ``Detections``).  Inside a frame the
    detections are ranked by score descending, then index ascending; a pixel belongs to the covering detection of lowest rank;
    ``top=1`` is the reference's picture, the best detection only.  ``colors`` (N,3) uint8 per detection; default: ``palette`` by
    the rank inside the frame, so that a frame has the same picture alone and in a group.  ``alpha`` in 1/256 units."""
    img, single = _frames(image_u8)
    B, H, W, _ = img.shape
    dev = img.device
    if isinstance(masks, (list, tuple)):
        if len(masks) != B:
            raise ValueError(f"a list of masks needs one entry per frame ({B}), got {len(masks)}")
        sc = [m.scores if scores is None else scores[i] for i, m in enumerate(masks)]
        parts = [_packed(m, H, W, dev) for m in masks]
        frame_index = torch.cat([torch.full((p.shape[0],), i, dtype=torch.int64) for i, p in enumerate(parts)]) if parts else None
        packed, scores = torch.cat(parts), torch.cat([torch.as_tensor(s).reshape(-1).float().to(dev) for s in sc])
    else:
        if scores is None and isinstance(masks, handoff.Detections):
            scores = masks.scores
        packed = _packed(masks, H, W, dev)
    N = packed.shape[0]
    if scores is None:
        raise ValueError("scores are needed to rank the detections")
    scores = torch.as_tensor(scores).to(dev).float().reshape(-1)
    if scores.shape[0] != N:
        raise ValueError(f"scores must have one entry per mask ({N}), got {scores.shape[0]}")
    frame = _frame_index(frame_index, N, B, dev)
    order, start, rank = rank_detections(scores, frame, B, top)
    if colors is None:
        table = torch.zeros(max(N, 1), 3, dtype=torch.uint8, device=dev)
        if order.shape[0]:
            table[order.long()] = palette(int(rank.max()) + 1).to(dev)[rank]
    else:
        table = torch.as_tensor(colors).to(dev)
        if table.dtype != torch.uint8 or tuple(table.shape) != (N, 3):
            raise ValueError(f"colors must be ({N},3) uint8, got {tuple(table.shape)} {table.dtype}")
        table = table.contiguous() if N else torch.zeros(1, 3, dtype=torch.uint8, device=dev)
    owner = owner_from_masks(packed, order, start, H, W)
    out = paint(img, owner, colors=table, alpha=alpha, gray=gray, edge_width=edge_width, edge_color=edge_color)
    return out[0] if single else out


# ------------------------------------------------------------------------------------------------------------------- poses
def box_corners(vertices, box_center="extent"):
    """The 8 corners (8,3) float32 of a model's box from its extents: corner k = centre + (sx, sy, sz) * extent / 2 with sx = -1 when
    k & 2, sy = -1 when k & 4, sz = -1 when k & 1 (the reference's order: 0-3 the +y face, 4-7 the -y face).  The centre is the
    middle of the extents (``"extent"``) or the mean of the vertices (``"mean"``, the reference's quirk)."""
    if box_center not in ("extent", "mean"):
        raise ValueError(f"box_center must be 'extent' or 'mean', got {box_center!r}")
    v = torch.as_tensor(vertices).float()
    lo, hi = v.amin(0), v.amax(0)
    half = (hi - lo) / 2
    centre = lo + half if box_center == "extent" else v.double().mean(0).float()
    sign = torch.tensor([[-1.0 if k & 2 else 1.0, -1.0 if k & 4 else 1.0, -1.0 if k & 1 else 1.0] for k in range(8)], device=v.device)
    return centre + sign * half


def model_points(vertices, points=None):
    """The points drawn for a model: ``points`` if given, otherwise vertices[::max(1, V // 512)][:512] (fixed; the reference draws a
    random choice)."""
    if points is not None:
        return torch.as_tensor(points).float().reshape(-1, 3)
    v = torch.as_tensor(vertices).float()
    return v[::max(1, v.shape[0] // MAX_POINTS)][:MAX_POINTS]


def _cams(K, N, B, frame, dev):
    k = torch.as_tensor(np.asarray(K.cpu() if torch.is_tensor(K) else K, np.float64)).float()
    if k.shape[-2:] == (3, 3):
        k = torch.stack([k[..., 0, 0], k[..., 1, 1], k[..., 0, 2], k[..., 1, 2]], -1)
    k = k.reshape(-1, 4).to(dev)
    if k.shape[0] == 1:
        return k.expand(N, 4).contiguous()
    if k.shape[0] == N:
        return k.contiguous()
    if k.shape[0] == B:
        return k[frame].contiguous()
    raise ValueError(f"K must be one camera, one per frame ({B}) or one per instance ({N}), as (3,3) or fx fy cx cy; got {tuple(k.shape)}")


def _rgb_word(c):
    c = c.int()
    return c[..., 0] | (c[..., 1] << 8) | (c[..., 2] << 16)


def pose_primitives(models, obj_ids, R, t, cams, frame, colors, mode, box_center, points, znear):
    """The flat primitive list (P,8) int32 of the instances in list order: per instance the 12 box edges (four ground edges in
    int(0.3 c), four pillars in int(0.6 c), four top edges in c, size 3), then the model points as discs of radius 1 in c.
    int(0.3 c) and int(0.6 c) are taken in integers, (3 c) // 10 and (6 c) // 10: the same values for every c in 0 .. 255.  One
    projection call and one block of tensor statements per OBJECT, whatever the number of its instances."""
    dev = R.device
    objs = np.asarray([int(o) for o in (obj_ids.cpu().tolist() if torch.is_tensor(obj_ids) else obj_ids)], np.int64)
    N = len(objs)
    nb = 8 if "box" in mode else 0
    ne = 12 if nb else 0
    cloud, count = {}, np.zeros(N, np.int64)
    for o in sorted(set(objs.tolist())):
        m = models[o]
        box = box_corners(m["vertices"], box_center).cpu() if nb else torch.zeros(0, 3)
        pts = (model_points(m["vertices"], None if points is None else (points[o] if isinstance(points, dict) else points)).cpu()
               if "points" in mode else torch.zeros(0, 3))
        cloud[o] = torch.cat([box, pts]).float()
        count[objs == o] = ne + pts.shape[0]
    first = np.concatenate([[0], np.cumsum(count)])                          # where an instance's primitives begin in the list
    out = torch.zeros(int(first[-1]), 8, dtype=torch.int32, device=dev)
    if first[-1] == 0:
        return out
    edges = torch.tensor(BOX_EDGES, device=dev)
    tenths = torch.tensor([int(round(s * 10)) for s in BOX_SHADE], device=dev)          # 3, 6, 10
    frame = torch.as_tensor(frame, device=dev).int()
    for o, pts in cloud.items():
        idx = torch.as_tensor(np.nonzero(objs == o)[0], device=dev)
        k, c = idx.shape[0], pts.shape[0]
        if c == 0:
            continue
        xy, valid = project(pts.to(dev).repeat(k, 1).contiguous(), idx.int().repeat_interleave(c).contiguous(), R, t, cams, znear)
        xy, valid = xy.reshape(k, c, 2), valid.reshape(k, c).int()
        col = colors[idx].int()                                            # (k,3)
        e = torch.zeros(k, ne + c - nb, 8, dtype=torch.int32, device=dev)
        e[:, :, 0] = frame[idx][:, None]
        if nb:
            e[:, :ne, 1:3], e[:, :ne, 3:5] = xy[:, edges[:, 0]], xy[:, edges[:, 1]]
            e[:, :ne, 5] = BOX_SIZE
            e[:, :ne, 6] = _rgb_word((col[:, None, :] * tenths[None, :, None]) // 10)
            e[:, :ne, 7] = valid[:, edges[:, 0]] & valid[:, edges[:, 1]]
        e[:, ne:, 1:3], e[:, ne:, 3:5] = xy[:, nb:], xy[:, nb:]
        e[:, ne:, 5] = POINT_SIZE
        e[:, ne:, 6] = _rgb_word(col)[:, None]
        e[:, ne:, 7] = valid[:, nb:]
        rows = torch.as_tensor(first[:-1], device=dev)[idx][:, None] + torch.arange(e.shape[1], device=dev)[None, :]
        out[rows.reshape(-1)] = e.reshape(-1, 8)
    return out


def surface_canvas(models, obj_ids, poses, cams, frame, B, H, W, *, ambient=0.3, diffuse=0.7, znear=1.0, chunk_bytes=1 << 28,
                   chunk_order=None):
    """The instances rendered object by object (``ops.render_views``) and folded by depth into one canvas per frame
    (``ops.vis_merge_layers``): dict(zbuf, owner, shade).  The nearest surface wins, at equal depth the lower instance index: the
    canvas does not depend on ``chunk_bytes`` or on the order of the objects.  Needs the device rasteriser."""
    dev = poses.device
    if not (poses.is_cuda and ops.have("render_views") and ops.have("vis_merge_layers")):
        raise ValueError("mode 'surface' needs the device rasteriser (ops.render_views): host tensors cannot be rendered")
    canvas = ops.vis_canvas(B, H, W, dev)
    objs = np.asarray([int(o) for o in (obj_ids.cpu().tolist() if torch.is_tensor(obj_ids) else obj_ids)], np.int64)
    step = max(1, int(chunk_bytes) // (24 * H * W))
    cam_host = cams.cpu().numpy()
    groups = sorted(set(objs.tolist())) if chunk_order is None else list(chunk_order)
    for o in groups:
        m = models[o]
        v = torch.as_tensor(np.asarray(m["vertices"], np.float32)).to(dev).contiguous()
        f = torch.as_tensor(np.asarray(m["faces"])).to(device=dev, dtype=torch.int32).contiguous()
        col = (torch.as_tensor(np.asarray(m["colors"])).to(device=dev, dtype=torch.uint8).contiguous() if m.get("colors") is not None
               else torch.full((v.shape[0], 3), 200, dtype=torch.uint8, device=dev))
        sel = np.nonzero(objs == o)[0]
        # one render call takes one camera; runs of consecutive instance indices keep "first + t" the instance index
        runs, a = [], 0
        while a < len(sel):
            e = a + 1
            while e < len(sel) and e - a < step and sel[e] == sel[e - 1] + 1 and (cam_host[sel[e]] == cam_host[sel[a]]).all():
                e += 1
            runs.append(sel[a:e])
            a = e
        for run in runs:
            k = cam_host[run[0]]
            idx = torch.as_tensor(run, device=dev)
            r = ops.render_views(v, f, col, poses[idx].contiguous(), float(k[0]), float(k[1]), float(k[2]), float(k[3]), H, W, ambient, diffuse,
                                 znear)
            ops.vis_merge_layers(canvas, r["depth"], r["rgb"], frame[idx].int().contiguous(), int(run[0]))
    return canvas


@torch.no_grad()
def overlay_poses(image_u8, models, obj_ids, R, t, K, *, frame_index=None, mode=("box", "points"), colors=None, box_center="extent",
                  points=None, alpha=ALPHA, edge_width=1, znear=1.0, chunk_bytes=1 << 28, gray=False, edge_color=(255, 255, 255)):
    """The poses drawn over the frames: per instance the projected box of the model's extents and its model points
    (``mode`` "box", "points": the reference's picture), and / or the rendered silhouettes merged by depth, blended with their
    shading and outlined ("surface": occlusions between the instances show as contours).

    ``image_u8`` (B,H,W,3) uint8 (or (H,W,3)); ``models`` {obj: dict(vertices (V,3), faces (F,3)[, colors (V,3) uint8])};
    ``obj_ids`` (N,), ``R`` (N,3,3), ``t`` (N,3) object -> camera in model units, ``K`` one camera, one per frame or one per
    instance ((3,3) or fx fy cx cy); ``frame_index`` (N,) for a group.  ``colors`` (N,3) uint8 per instance; default ``palette`` by
    the instance's position inside its frame.  ``points``: the points to draw instead of the fixed choice of up to 512 vertices (an
    array, or {obj: array}).  ``alpha``, ``edge_width``, ``gray``, ``edge_color`` apply to the surface layer; ``gray`` also to the
    base of the other modes."""
    mode = (mode,) if isinstance(mode, str) else tuple(mode)
    if not mode or any(m not in ("box", "points", "surface") for m in mode):
        raise ValueError(f"mode names 'box', 'points' and 'surface', got {mode!r}")
    img, single = _frames(image_u8)
    B, H, W, _ = img.shape
    dev = img.device
    R = torch.as_tensor(R).to(dev).float().reshape(-1, 3, 3).contiguous()
    N = R.shape[0]
    t = torch.as_tensor(t).to(dev).float().reshape(-1, 3).contiguous()
    n_obj = len(obj_ids)
    if t.shape[0] != N or n_obj != N:
        raise ValueError(f"obj_ids, R and t must have one entry per instance, got {n_obj}, {N}, {t.shape[0]}")
    frame = _frame_index(frame_index, N, B, dev)
    cams = _cams(K, N, B, frame, dev) if N else torch.zeros(0, 4, device=dev)
    if colors is None:
        start = _starts(frame, B)
        pos = torch.arange(N, device=dev) - start[frame] if N and bool((frame[1:] >= frame[:-1]).all()) else None
        if pos is None:                                                   # instances not grouped by frame: position by counting
            pos = torch.stack([(frame[:n] == frame[n]).sum() for n in range(N)]) if N else torch.zeros(0, dtype=torch.int64, device=dev)
        colors = palette(int(pos.max()) + 1 if N else 1).to(dev)[pos]
    else:
        colors = torch.as_tensor(colors).to(dev)
        if colors.dtype != torch.uint8 or tuple(colors.shape) != (N, 3):
            raise ValueError(f"colors must be ({N},3) uint8, got {tuple(colors.shape)} {colors.dtype}")
    if not 0 <= int(alpha) <= 256:
        raise ValueError(f"alpha must lie in [0, 256] (units of 1/256), got {alpha}")
    if not 0 <= int(edge_width) <= 4:
        raise ValueError(f"edge_width must lie in [0, 4], got {edge_width}")
    if "surface" in mode:
        poses = torch.zeros(N, 4, 4, device=dev)
        poses[:, :3, :3], poses[:, :3, 3], poses[:, 3, 3] = R, t, 1.0
        canvas = surface_canvas(models, obj_ids, poses, cams, frame, B, H, W, znear=znear, chunk_bytes=chunk_bytes)
        out = paint(img, canvas["owner"], shade=canvas["shade"], alpha=alpha, gray=gray, edge_width=edge_width, edge_color=edge_color)
    else:
        out = paint(img, torch.full((B, H, W), -1, dtype=torch.int32, device=dev), colors=torch.zeros(1, 3, dtype=torch.uint8, device=dev),
                    alpha=0, gray=True, edge_width=0) if gray else img.clone()
    if "box" in mode or "points" in mode:
        prims = pose_primitives(models, obj_ids, R, t, cams, frame, colors, mode, box_center, points, znear)
        out = draw(out, prims)
    return out[0] if single else out


# ------------------------------------------------------------------------------------------------------------------- pictures
def side_by_side(a, b):
    """Two pictures (or two groups of pictures) of one height next to each other: the reference's concatenation."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.dim() != b.dim() or a.shape[:-2] != b.shape[:-2] or a.shape[-1] != b.shape[-1]:
        raise ValueError(f"pictures of one height (and one group size) expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    return torch.cat([a, b.to(a.device)], dim=-2)


def save_png(path, image):
    """image (H,W,3) uint8 on any device -> a PNG file."""
    from PIL import Image
    img = torch.as_tensor(image)
    if img.dim() != 3 or img.shape[2] != 3 or img.dtype != torch.uint8:
        raise ValueError(f"image must be (H,W,3) uint8, got {tuple(img.shape)} {img.dtype}")
    Image.fromarray(img.cpu().numpy()).save(path, format="PNG")


@torch.no_grad()
def overlay_results(frames, results, models, *, obj_ids=None, pose_scale=1.0, top=1, mode=("box", "points"), **pose_kw):
    """Both pictures of every frame of a group: ``frames`` as given to ``FramePipeline.run_group`` (image_u8, depth, K, ...),
    ``results`` the list of (Detections, poses-or-None) it returned, ``models`` {obj: dict(vertices, faces)} in the units of the
    mesh; ``pose_scale`` converts the pipeline's translations to those units (1000 for a pipeline in metres and meshes in
    millimetres).  ``obj_ids`` maps the zero-based ``Detections.object_ids`` to the keys of ``models`` (default: id + 1, the BOP
    numbering).  -> (vis_ism (B,H,W,3), vis_pem (B,H,W,3)) uint8."""
    image = torch.stack([torch.as_tensor(f[0]) for f in frames])
    dev = image.device
    ism = overlay_detections(image, [det for det, _ in results], top=top)
    oid, R, t, fi = [], [], [], []
    for b, (det, poses) in enumerate(results):
        if poses is None:
            continue
        ids = det.object_ids[poses["kept"]].cpu().tolist()
        oid += [int(i) + 1 if obj_ids is None else obj_ids[int(i)] for i in ids]
        R.append(poses["pred_R"].float().to(dev))
        t.append(poses["pred_t"].float().to(dev) * float(pose_scale))
        fi += [b] * len(ids)
    K = torch.stack([torch.as_tensor(f[2]).float().reshape(3, 3).cpu() for f in frames])
    pem = overlay_poses(image, models, oid, torch.cat(R) if R else torch.zeros(0, 3, 3), torch.cat(t) if t else torch.zeros(0, 3), K,
                        frame_index=fi, mode=mode, **pose_kw)
    return ism, pem
