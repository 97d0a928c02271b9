"""The small-region clean-up of SAM's mask generator, restated in plain loops from its definition: the oracle
of tests/test_host_small_regions.py, tests/test_gpu_small_regions.py and tests/test_emu_small_regions.py.  Every comparison with
it is `equal`.  Nothing here shares code with sam6d_amd: breadth-first search, Python integers, numpy arrays as storage only."""
from collections import deque

import numpy as np

NEIGHBOURS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def label(mask, background=False):
    """mask (H,W), a pixel is set when it is not 0 -> (labels (H,W) int32, areas {label: pixels}).  The label of a pixel of the chosen
    polarity is the row-major index of the first pixel of its 8-connected component (the scan meets it first), -1 on the others."""
    H, W = mask.shape
    fg = (np.asarray(mask) != 0) != bool(background)
    lab = np.full((H, W), -1, np.int32)
    areas = {}
    for y in range(H):
        for x in range(W):
            if not fg[y, x] or lab[y, x] >= 0:
                continue
            root = y * W + x
            lab[y, x] = root
            n, queue = 0, deque([(y, x)])
            while queue:
                cy, cx = queue.popleft()
                n += 1
                for dy, dx in NEIGHBOURS:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < H and 0 <= nx < W and fg[ny, nx] and lab[ny, nx] < 0:
                        lab[ny, nx] = root
                        queue.append((ny, nx))
            areas[root] = n
    return lab, areas


def box(mask):
    """XYXY box of the set pixels, inclusive maximum corner; [0, 0, 0, 0] for an empty mask."""
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return [0, 0, 0, 0]
    return [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def remove_small_regions_one(mask, min_area):
    """-> (mask (H,W) uint8 0 / 1, changed_h, changed_i, kept_largest, tie): the two steps of the definition on one mask.
    kept_largest: every island was small; tie: and the largest area occurred more than once."""
    m = np.asarray(mask) != 0
    lab, areas = label(m, background=True)
    small = [r for r, a in areas.items() if a < min_area]
    changed_h = len(small) > 0
    if changed_h:
        m = m | np.isin(lab, small)
    lab, areas = label(m, background=False)
    small = [r for r, a in areas.items() if a < min_area]
    changed_i = len(small) > 0
    kept_largest = tie = False
    if changed_i:
        big = [r for r in areas if areas[r] >= min_area]
        if not big:
            kept_largest = True
            top = max(areas.values())
            firsts = sorted(r for r, a in areas.items() if a == top)
            tie = len(firsts) > 1
            big = [firsts[0]]                                   # among equal areas the earlier first pixel
        m = np.isin(lab, big)
    return m.astype(np.uint8), changed_h, changed_i, kept_largest, tie


def remove_small_regions(masks, min_area):
    """masks (N,H,W) -> (masks uint8 (N,H,W), changed bool (N,), boxes int32 (N,4), branches: list of (changed_h, changed_i,
    kept_largest, tie) per mask)."""
    masks = np.asarray(masks)
    N, H, W = masks.shape
    out, changed, boxes, branches = np.zeros((N, H, W), np.uint8), np.zeros(N, bool), np.zeros((N, 4), np.int32), []
    for n in range(N):
        out[n], ch, ci, kl, tie = remove_small_regions_one(masks[n], min_area)
        changed[n] = ch or ci
        boxes[n] = box(out[n])
        branches.append((ch, ci, kl, tie))
    return out, changed, boxes, branches


def nms(boxes, scores, thresh):
    """Greedy box NMS in loops: boxes visited by decreasing score, equal scores in input order; a box is dropped when its IoU with a
    kept box exceeds thresh (float32 arithmetic: area = (x2 - x1)(y2 - y1), IoU = inter / (a + b - inter)) -> kept indices in
    visiting order."""
    b = np.asarray(boxes, np.float32)
    order = sorted(range(len(b)), key=lambda i: -float(scores[i]))               # sorted() is stable
    kept = []
    for i in order:
        ok = True
        for j in kept:
            w = max(np.float32(0), min(b[i, 2], b[j, 2]) - max(b[i, 0], b[j, 0]))
            h = max(np.float32(0), min(b[i, 3], b[j, 3]) - max(b[i, 1], b[j, 1]))
            inter = np.float32(w * h)
            ai = np.float32((b[i, 2] - b[i, 0]) * (b[i, 3] - b[i, 1]))
            aj = np.float32((b[j, 2] - b[j, 0]) * (b[j, 3] - b[j, 1]))
            with np.errstate(divide="ignore", invalid="ignore"):
                if np.float32(inter) / np.float32(ai + aj - inter) > np.float32(thresh):
                    ok = False
                    break
        if ok:
            kept.append(i)
    return kept


def postprocess_small_regions(proposals, min_area, nms_thresh):
    """proposals: dict of numpy arrays with ``masks`` (N,H,W) and ``boxes`` (N,4) among them -> the same dict after the clean-up: the
    fields filtered by the NMS over the new boxes (score 1 unchanged, 0 changed), the changed survivors with new masks and boxes."""
    if len(proposals["masks"]) == 0:
        return proposals
    new_masks, changed, new_boxes, _ = remove_small_regions(proposals["masks"], min_area)
    keep = nms(new_boxes, [0.0 if c else 1.0 for c in changed], nms_thresh)
    out = {k: np.asarray(v)[keep] for k, v in proposals.items()}
    for o, i in enumerate(keep):
        if changed[i]:
            out["masks"][o] = new_masks[i].astype(out["masks"].dtype)
            out["boxes"][o] = new_boxes[i]
    return out


def scipy_statement(mask, min_area, holes):
    """One step of the definition (holes or islands) on scipy.ndimage.label with the full 3 x 3 structure -> (mask bool, changed).
    scipy numbers components in the order a row-major scan meets them, so "the first largest" of argmax is the tie rule of the
    definition; scipy stands in for the cv2 labelling the upstream function (segment_anything/utils/amg.py:267-291) calls."""
    from scipy import ndimage
    mask = np.asarray(mask) != 0
    regions, count = ndimage.label(~mask if holes else mask, structure=np.ones((3, 3), int))
    sizes = np.bincount(regions.ravel(), minlength=count + 1)[1:]            # sizes[i]: component i + 1
    small = np.flatnonzero(sizes < min_area) + 1
    if small.size == 0:
        return mask, False
    if holes:
        return mask | np.isin(regions, small), True
    stay = np.flatnonzero(sizes >= min_area) + 1
    if stay.size == 0:
        stay = np.array([int(np.argmax(sizes)) + 1])
    return np.isin(regions, stay), True
