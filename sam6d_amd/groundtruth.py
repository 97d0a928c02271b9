"""BOP ground-truth files from annotated poses: what the BOP toolkit derives from ``scene_gt.json`` and the
depth images -- the masks, the visible masks, their boxes and pixel counts, ``visib_fract`` -- and the ``models_info.json`` record of
a model, computed here on the device so that ``tools/bop_eval.py`` and ``tools/coco_eval.py`` can score a user's own annotated
frames.  bop_toolkit is not part of this project: the quantities are defined operation by operation in csrc/s6d_bopgt.hip and
pinned to an independent restatement (tests/bopgt_ref.py); no equality with the toolkit's files is claimed.

  model_info              diameter (kernel ``ops.model_diameter``, or a chunked torch statement), extents from amin / amax
  instance_ground_truth   one depth render per instance on a canvas with a margin (``ops.render_depth``), then
                          ``ops.gt_visibility``: masks, visible masks, counts, extents, visib_fract
  gt_info_records         the ``scene_gt_info.json`` records of that result

Device tensors go to the kernels; host tensors, and the policy field ``bop_eval`` = "0", to the torch statements below through
``policy.guard`` (sites ``groundtruth.*``): under strict mode a fall-back on the device is an error.
"""
import numpy as np
import torch

from . import evaluation, ops, policy

INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def _kernels(site, t, *names):
    return policy.current().bop_eval == "1" and policy.guard(site, cuda=t.is_cuda, have=all(ops.have(n) for n in names))


# ------------------------------------------------------------------------------------------------------------------- the model
def _model_diameter_library(v, chunk_bytes=1 << 26):
    """The library statement of ``ops.model_diameter``: the same float32 operations, a chunk of rows against all vertices at a
    time (no (V,V) buffer) -> (1,) float32."""
    V = v.shape[0]
    step = max(1, chunk_bytes // (16 * V))
    inf = torch.tensor(float("inf"), device=v.device)
    best = torch.zeros((), device=v.device)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    for i in range(0, V, step):
        dx, dy, dz = x[i:i + step, None] - x[None, i:], y[i:i + step, None] - y[None, i:], z[i:i + step, None] - z[None, i:]
        d2 = (dx * dx + dy * dy) + dz * dz
        best = torch.maximum(best, torch.where(torch.isfinite(d2), d2, inf).max())
    return torch.sqrt(best).reshape(1)


@torch.no_grad()
def model_info(vertices, device=None):
    """The ``models_info.json`` record of a model: vertices (V,3) -> dict(diameter, min_x, min_y, min_z, size_x, size_y, size_z),
    Python floats.  The extents are ``amin`` / ``amax`` of the float32 vertices (exact); the diameter is the largest distance
    between two vertices, float32 (csrc/s6d_bopgt.hip: the maximum of (dx dx + dy dy) + dz dz over all pairs, one square root), by
    the kernel on the device and by the chunked torch statement on the host -- the same bits.  ValueError when a coordinate is not
    finite."""
    dev = torch.device(device) if device is not None else (vertices.device if torch.is_tensor(vertices) else
                                                           torch.device("cuda" if torch.cuda.is_available() else "cpu"))
    v = evaluation._f32(vertices, dev, "vertices", (None, 3))
    if v.shape[0] < 1:
        raise ValueError("model_info: at least one vertex is needed")
    d = ops.model_diameter(v) if _kernels("groundtruth.model_diameter", v, "model_diameter") else _model_diameter_library(v)
    d = float(d.cpu()[0])
    lo, hi = v.amin(0).cpu().double(), v.amax(0).cpu().double()
    if not np.isfinite(d) or not bool(torch.isfinite(lo).all() and torch.isfinite(hi).all()):
        raise ValueError("model_info: a vertex coordinate is not finite (or a squared distance overflows float32)")
    size = hi - lo
    return dict(diameter=d, min_x=float(lo[0]), min_y=float(lo[1]), min_z=float(lo[2]), size_x=float(size[0]), size_y=float(size[1]),
                size_z=float(size[2]))


# ------------------------------------------------------------------------------------------------------------------- visibility
def _gt_visibility_library(canvas, depth_test, test_index, cams, delta, margin):
    """The library statement of ``ops.gt_visibility`` (its dict), for host tensors and for checking."""
    mx, my = margin
    N, (M, H, W), dev = canvas.shape[0], depth_test.shape, canvas.device
    if N and (int(test_index.min()) < 0 or int(test_index.max()) >= M):
        raise ValueError(f"gt_visibility: test_index must lie in [0, {M})")
    every = canvas > 0
    zg = canvas[:, my:my + H, mx:mx + W]
    zt = depth_test[test_index.long()]
    u = torch.arange(W, dtype=torch.float32, device=dev)[None, None, :]
    v = torch.arange(H, dtype=torch.float32, device=dev)[None, :, None]
    fx, fy, cx, cy = (cams[:, k, None, None] for k in range(4))
    a, b = (u - cx) / fx, (v - cy) / fy
    r = torch.sqrt((a * a + b * b) + 1.0)
    Dg, Dt = zg * r, zt * r
    mask = zg > 0
    visib = mask & (((Dg - Dt) <= delta) | (zt == 0))
    counts = torch.stack([every.sum((1, 2)), mask.sum((1, 2)), (mask & (zt > 0)).sum((1, 2)), visib.sum((1, 2))], 1).int()

    def extent(w, x0, y0):
        cols, rows = w.any(1), w.any(2)                                    # (N, width), (N, height)
        xs, ys = torch.arange(w.shape[2], device=dev) + x0, torch.arange(w.shape[1], device=dev) + y0
        big, small = torch.full_like(xs, INT_MAX), torch.full_like(xs, INT_MIN)
        bigy, smally = torch.full_like(ys, INT_MAX), torch.full_like(ys, INT_MIN)
        return torch.stack([torch.where(cols, xs, big).amin(1), torch.where(rows, ys, bigy).amin(1),
                            torch.where(cols, xs, small).amax(1), torch.where(rows, ys, smally).amax(1)], 1)
    extents = torch.stack([extent(every, -mx, -my), extent(visib, 0, 0)], 1).int()
    return dict(mask=mask.to(torch.uint8), mask_visib=visib.to(torch.uint8), counts=counts, extents=extents)


def _render(v, f, poses, cams_c, Hc, Wc, znear, kernels):
    if kernels:
        return ops.render_depth(v, f, poses, cams_c, Hc, Wc, znear)
    return evaluation._render_depth_library(v, f, poses, cams_c, Hc, Wc, znear)


@torch.no_grad()
def instance_ground_truth(models, gt, images, *, delta=15.0, margin=None, depth="measured", masks="dense", chunk_bytes=1 << 30,
                          device=None, znear=1.0):
    """Masks, visible masks, boxes, pixel counts and ``visib_fract`` of every annotated instance.

    ``models`` {obj: dict(vertices (V,3), faces (F,3), ...)}, ``gt`` dict(im (G,), obj (G,), pose (G,4,4) object -> camera) and
    ``images`` dict(cams (I,4) = fx fy cx cy, depth (I,H,W) float32 in model units, 0 = missing) are what
    ``tools/bop_eval.load_dataset`` builds; ``gt["im"]`` indexes ``images``.

    Every instance is rendered ONCE (``ops.render_depth``), on a canvas of (H + 2 my, W + 2 mx) pixels with the image's camera
    moved by the margin (cx + mx, cy + my in float32); ``margin`` = (mx, my), default (W, H): one image on every side, so that the
    parts of an object outside the frame count in ``px_count_all``; (0, 0) is the cheap mode, in which ``px_count_all`` is the
    in-image count.  The image is the window of that canvas, so visible <= mask <= all holds by construction.  A pixel of the mask
    is visible when the measured surface is not more than ``delta`` in front of it along the ray, or missing (csrc/s6d_bopgt.hip;
    the rule of VSD).  Instances are grouped by object and go through in chunks of at most ``chunk_bytes`` of canvas and masks;
    the counts are integers, so the result does not depend on the chunking.

    ``depth="rendered"`` is for datasets without depth images: the test depth of an image is the minimum positive rendered Z over
    that image's own instances (torch statements).  LIMITATION: visibility then reflects only the mutual occlusion of the
    annotated objects -- nothing else in the scene hides anything -- and ``px_count_valid`` equals the in-image count.

    -> dict: ``mask``, ``mask_visib`` (G,H,W) uint8 0 / 1 on the device (``masks="rle"``: ``handoff.RleMasks``, encoded chunk by
    chunk, the dense masks of one chunk at a time only); ``extents_obj``, ``extents_visib`` (G,4) int64 numpy = xmin ymin xmax ymax,
    maximum inclusive, image coordinates (the object's may be negative or >= W), an empty set (-1, -1, -1, -1) with ``empty_obj`` /
    ``empty_visib`` (G,) bool; ``px_count_all``, ``px_count_in_image``, ``px_count_valid``, ``px_count_visib`` (G,) int64;
    ``visib_fract`` (G,) float64 = px_count_visib / px_count_all, 0 when the denominator is 0; ``skipped`` (G,) int64, the
    rasteriser's count of triangles it could not draw: non-zero means the object reaches behind ``znear`` and ``px_count_all``
    is a lower bound; ``size`` = (H, W), ``margin``."""
    if depth not in ("measured", "rendered") or masks not in ("dense", "rle"):
        raise ValueError(f"depth must be 'measured' or 'rendered' and masks 'dense' or 'rle', got {depth!r}, {masks!r}")
    dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    g_im, g_obj = np.asarray(gt["im"], np.int64).reshape(-1), np.asarray(gt["obj"], np.int64).reshape(-1)
    G = len(g_im)
    pose = torch.as_tensor(np.asarray(gt["pose"], np.float64).reshape(G, 4, 4)).float()
    cams = evaluation._f32(images["cams"], dev, "cams", (None, 4))
    I = cams.shape[0]
    if depth == "measured":
        zt = evaluation._f32(images["depth"], dev, "depth", (I, None, None))
        H, W = int(zt.shape[1]), int(zt.shape[2])
    else:
        H, W = (int(s) for s in (images["size"] if "size" in images else np.asarray(images["depth"]).shape[1:]))
    if G and (g_im.min() < 0 or g_im.max() >= I):
        raise ValueError(f"gt['im'] must lie in [0, {I})")
    mx, my = (W, H) if margin is None else (int(m) for m in margin)
    if mx < 0 or my < 0:
        raise ValueError(f"margin must be >= 0, got {(mx, my)}")
    Hc, Wc = H + 2 * my, W + 2 * mx
    if Hc * Wc >= 2 ** 31:
        raise ValueError(f"a canvas of {Hc} x {Wc} pixels (2^31 or more) is refused: use a smaller margin")
    kernels = _kernels("groundtruth.visibility", cams, "gt_visibility", "render_depth")
    shift = torch.tensor([0.0, 0.0, float(mx), float(my)], device=dev)
    step = max(1, int(chunk_bytes) // (4 * Hc * Wc + 2 * H * W))
    order = np.argsort(g_obj, kind="stable")                              # grouped by object, the annotation order inside a group
    chunks = []
    for obj in sorted(set(g_obj.tolist())):
        sel = order[g_obj[order] == obj]
        chunks += [(obj, sel[a:a + step]) for a in range(0, len(sel), step)]
    mesh = {}

    def canvases(obj, sel):
        if obj not in mesh:
            mesh.clear()                                                   # one object's mesh on the device at a time
            mesh[obj] = (evaluation._f32(models[obj]["vertices"], dev, "vertices", (None, 3)),
                         torch.as_tensor(np.asarray(models[obj]["faces"])).to(device=dev, dtype=torch.int32).contiguous())
        k = cams[torch.as_tensor(g_im[sel], device=dev)]
        r = _render(*mesh[obj], pose[sel].to(dev).contiguous(), (k + shift).contiguous(), Hc, Wc, znear, kernels)
        return r["depth"], r["skipped"], k.contiguous()

    if depth == "rendered":
        inf = torch.tensor(float("inf"), device=dev)
        zt = torch.full((I, H, W), float("inf"), device=dev)
        for obj, sel in chunks:                                            # the same renders as below: the same bits
            z = canvases(obj, sel)[0][:, my:my + H, mx:mx + W]
            z = torch.where(z > 0, z, inf)
            for i in np.unique(g_im[sel]).tolist():
                zt[i] = torch.minimum(zt[i], z[torch.as_tensor(g_im[sel] == i, device=dev)].amin(0))
        zt = torch.where(torch.isfinite(zt), zt, torch.zeros_like(zt)).contiguous()
    counts = torch.zeros(G, 4, dtype=torch.int32, device=dev)
    extents = torch.zeros(G, 2, 4, dtype=torch.int32, device=dev)
    skipped = torch.zeros(G, dtype=torch.int32, device=dev)
    dense = {k: torch.empty(G, H, W, dtype=torch.uint8, device=dev) for k in ("mask", "mask_visib")} if masks == "dense" else None
    parts = dict(mask=[], mask_visib=[])
    for obj, sel in chunks:
        canvas, skip, k = canvases(obj, sel)
        ti = torch.as_tensor(g_im[sel], device=dev).int()
        r = ops.gt_visibility(canvas, zt, ti, k, delta, (mx, my)) if kernels else _gt_visibility_library(canvas, zt, ti, k, float(delta), (mx, my))
        where = torch.as_tensor(sel, device=dev)
        counts[where], extents[where], skipped[where] = r["counts"], r["extents"], skip
        for name in parts:
            if masks == "dense":
                dense[name][where] = r[name]
            else:
                from .ism import handoff
                parts[name].append(handoff.RleMasks.from_masks(r[name]))
    c, e = counts.cpu().numpy().astype(np.int64), extents.cpu().numpy().astype(np.int64)
    out = dict(size=(H, W), margin=(mx, my), skipped=skipped.cpu().numpy().astype(np.int64), px_count_all=c[:, 0], px_count_in_image=c[:, 1],
               px_count_valid=c[:, 2], px_count_visib=c[:, 3])
    with np.errstate(all="ignore"):
        out["visib_fract"] = np.where(c[:, 0] > 0, c[:, 3].astype(np.float64) / c[:, 0].astype(np.float64), 0.0)
    for name, row, count in (("obj", 0, c[:, 0]), ("visib", 1, c[:, 3])):
        out["empty_" + name] = count == 0
        out["extents_" + name] = np.where((count == 0)[:, None], -1, e[:, row])
    if masks == "dense":
        out.update(dense)
    else:
        from .ism import handoff
        back = np.argsort(np.concatenate([sel for _, sel in chunks])) if chunks else np.zeros(0, np.int64)
        for name in parts:
            out[name] = handoff.RleMasks.cat(parts[name])[back] if chunks else handoff.RleMasks.from_masks(torch.zeros(0, H, W, dtype=torch.uint8, device=dev))
    return out


def gt_info_records(result, box_rule="span"):
    """The ``scene_gt_info.json`` records of ``instance_ground_truth``'s result, one dict per instance in its order: ``bbox_obj``,
    ``bbox_visib`` (x, y, w, h), ``px_count_all``, ``px_count_valid``, ``px_count_visib``, ``visib_fract``.  The pinned quantity is
    the inclusive extents; ``box_rule`` says how a box is written from them: "span" = [xmin, ymin, xmax - xmin, ymax - ymin] (the
    default: what the author recalls of the public BOP files -- no BOP file was available to confirm it),
    "pixels" = the same with 1 added to both sizes.  An empty set gives [-1, -1, -1, -1]."""
    if box_rule not in ("span", "pixels"):
        raise ValueError(f"box_rule must be 'span' or 'pixels', got {box_rule!r}")
    one = 1 if box_rule == "pixels" else 0

    def box(e, empty):
        return [-1, -1, -1, -1] if empty else [int(e[0]), int(e[1]), int(e[2] - e[0]) + one, int(e[3] - e[1]) + one]
    return [dict(bbox_obj=box(result["extents_obj"][g], result["empty_obj"][g]), bbox_visib=box(result["extents_visib"][g], result["empty_visib"][g]),
                 px_count_all=int(result["px_count_all"][g]), px_count_valid=int(result["px_count_valid"][g]),
                 px_count_visib=int(result["px_count_visib"][g]), visib_fract=float(result["visib_fract"][g]))
            for g in range(len(result["px_count_all"]))]
