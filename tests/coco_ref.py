"""An independent restatement of the COCO AP definition of sam6d_amd/evaluation.py in plain numpy and Python
loops: dense boolean masks, one detection, one ground truth, one threshold at a time.  It shares no code with the package.
pycocotools is not present; nothing here is compared with it.

Instances are plain dicts:  detection = dict(im, cat, score, mask (H,W) bool | box (x, y, w, h)),
ground truth = dict(im, cat, mask (H,W) bool, box (x, y, w, h), ignore).  ``im`` is anything sortable (an int, a (scene, image)
tuple)."""
import numpy as np

THRESHOLDS = np.linspace(0.5, 0.95, 10)
AREAS = {"all": (0.0, 1e10), "small": (0.0, 32.0 ** 2), "medium": (32.0 ** 2, 96.0 ** 2), "large": (96.0 ** 2, 1e10)}
MAX_DETS = (1, 10, 100)
RECALLS = np.linspace(0.0, 1.0, 101)


def pack(mask):
    """(H,W) bool -> the list of 64-bit words: bit k of word j is pixel 64 j + k in row-major order."""
    flat = np.asarray(mask).astype(bool).reshape(-1)
    words = []
    for j in range((len(flat) + 63) // 64):
        w = 0
        for k, bit in enumerate(flat[64 * j:64 * j + 64]):
            if bit:
                w |= 1 << k
        words.append(w)
    return words


def mask_counts(d, g):
    d, g = np.asarray(d).astype(bool), np.asarray(g).astype(bool)
    return int(np.logical_and(d, g).sum()), int(d.sum()), int(g.sum())


def mask_iou(d, g):
    inter, a, b = mask_counts(d, g)
    union = a + b - inter
    return np.float64(inter) / np.float64(union) if union > 0 else np.float64(0.0)


def box_iou(d, g):
    dx, dy, dw, dh = (np.float64(v) for v in d)
    gx, gy, gw, gh = (np.float64(v) for v in g)
    w = min(dx + dw, gx + gw) - max(dx, gx)
    h = min(dy + dh, gy + gh) - max(dy, gy)
    if w <= 0 or h <= 0:
        return np.float64(0.0)
    i = w * h
    a = dw * dh
    b = gw * gh
    u = (a + b) - i
    return i / u


def match_group(ious, det_area, gt_area, gt_ignore, t, lo, hi, events=None):
    """The detections in visiting order against the ground truths of their group, at ONE threshold and ONE area range.
    -> (match: per detection the ground truth's index or -1, ignore: per detection).  ``events`` (a set) collects what happened:
    'tie' (an equal IoU replaced the match), 'passed_over_ignored' (a non-ignored match kept a better ignored ground truth out),
    'matched_ignored', 'gt_outside', 'det_outside', 'taken' (a ground truth was already matched)."""
    events = set() if events is None else events
    D, G = len(det_area), len(gt_area)
    ig = []
    for g in range(G):
        outside = gt_area[g] < lo or gt_area[g] > hi
        if outside:
            events.add("gt_outside")
        ig.append(bool(gt_ignore[g]) or outside)
    walk = [g for g in range(G) if not ig[g]] + [g for g in range(G) if ig[g]]
    taken, match, ignore = set(), [], []
    for d in range(D):
        bar, m = min(t, 1 - 1e-10), -1
        for g in walk:
            if g in taken:
                events.add("taken")
                continue
            if m >= 0 and not ig[m] and ig[g]:
                if any(ious[d][x] > bar for x in walk if ig[x] and x not in taken):
                    events.add("passed_over_ignored")
                break
            if ious[d][g] < bar:
                continue
            if m >= 0 and ious[d][g] == bar:
                events.add("tie")
            bar, m = ious[d][g], g
        if m >= 0:
            taken.add(m)
            if ig[m]:
                events.add("matched_ignored")
            ignore.append(ig[m])
        else:
            outside = det_area[d] < lo or det_area[d] > hi
            if outside:
                events.add("det_outside")
            ignore.append(bool(outside))
        match.append(m)
    return match, ignore


def _area(inst, iou_type):
    return float(np.asarray(inst["mask"]).astype(bool).sum()) if iou_type == "segm" else float(np.float64(inst["box"][2]) * np.float64(inst["box"][3]))


def evaluate(dets, gts, iou_type="segm", events=None):
    """-> {(im, cat): dict(scores, match[t][area] lists, ignore[t][area] lists, gt_ignore[area] lists)} with the detections of a
    group in visiting order (stable by descending score, the first 100)."""
    events = set() if events is None else events
    groups = sorted({(x["im"], x["cat"]) for x in list(dets) + list(gts)})
    out = {}
    for key in groups:
        ds = [x for x in dets if (x["im"], x["cat"]) == key]
        gs = [x for x in gts if (x["im"], x["cat"]) == key]
        order = sorted(range(len(ds)), key=lambda i: -ds[i]["score"])          # sorted() is stable
        if len({x["score"] for x in ds}) < len(ds):
            events.add("equal_scores")
        if len(order) > 100:
            events.add("truncated")
        ds = [ds[i] for i in order[:100]]
        ious = [[(mask_iou(d["mask"], g["mask"]) if iou_type == "segm" else box_iou(d["box"], g["box"])) for g in gs] for d in ds]
        d_area = [_area(d, iou_type) for d in ds]
        g_area = [float(np.asarray(g["mask"]).astype(bool).sum()) for g in gs]
        g_flag = [bool(g["ignore"]) for g in gs]
        rec = dict(scores=[d["score"] for d in ds], match={}, ignore={}, gt_ignore={}, ious=ious)
        for name, (lo, hi) in AREAS.items():
            rec["gt_ignore"][name] = [g_flag[g] or g_area[g] < lo or g_area[g] > hi for g in range(len(gs))]
            for ti, t in enumerate(THRESHOLDS):
                m, i = match_group(ious, d_area, g_area, g_flag, t, lo, hi, events)
                rec["match"][ti, name], rec["ignore"][ti, name] = m, i
        out[key] = rec
    return out


def accumulate(groups):
    """-> (precision {(t, cat, area, maxdet): 101 values or None}, recall {(t, cat, area, maxdet): value or None}); None where the
    category has no non-ignored ground truth in the range."""
    cats = sorted({k[1] for k in groups})
    precision, recall = {}, {}
    eps = np.spacing(1)
    for cat in cats:
        keys = [k for k in sorted(groups) if k[1] == cat]
        for name in AREAS:
            n_pos = sum(1 for k in keys for x in groups[k]["gt_ignore"][name] if not x)
            for md in MAX_DETS:
                for ti in range(len(THRESHOLDS)):
                    if n_pos == 0:
                        precision[ti, cat, name, md] = recall[ti, cat, name, md] = None
                        continue
                    rows = []
                    for k in keys:
                        r = groups[k]
                        for d in range(min(md, len(r["scores"]))):
                            rows.append((r["scores"][d], r["match"][ti, name][d] >= 0, r["ignore"][ti, name][d]))
                    rows = [rows[i] for i in sorted(range(len(rows)), key=lambda i: -rows[i][0])]
                    rows = [r for r in rows if not r[2]]
                    tp = fp = 0
                    rc, pr = [], []
                    for _, hit, _ in rows:
                        tp, fp = tp + (1 if hit else 0), fp + (0 if hit else 1)
                        rc.append(np.float64(tp) / np.float64(n_pos))
                        pr.append(np.float64(tp) / (np.float64(fp) + np.float64(tp) + eps))
                    recall[ti, cat, name, md] = float(rc[-1]) if rc else 0.0
                    for i in range(len(pr) - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = []
                    for r in RECALLS:
                        i = 0
                        while i < len(rc) and rc[i] < r:                          # searchsorted(rc, r, side="left")
                            i += 1
                        q.append(float(pr[i]) if i < len(rc) else 0.0)
                    precision[ti, cat, name, md] = q
    return precision, recall


def _mean(values):
    values = list(values)
    return float(np.mean(np.asarray(values, np.float64))) if values else -1.0


def coco_scores(dets, gts, iou_type="segm", events=None):
    groups = evaluate(dets, gts, iou_type, events)
    precision, recall = accumulate(groups)
    cats = sorted({k[1] for k in groups})
    T = range(len(THRESHOLDS))

    def ap(ts, name):
        stack = [precision[t, c, name, 100] for c in cats for t in ts if precision[t, c, name, 100] is not None]
        # (the mean of equally long lists: the flat mean in the (threshold, recall, category) order of the definition)
        arr = np.array([[[precision[t, c, name, 100][r] for c in cats if precision[t, c, name, 100] is not None] for r in range(101)] for t in ts],
                       np.float64)
        return float(arr.reshape(-1).mean()) if stack else -1.0

    def ar(md):
        arr = np.array([[recall[t, c, "all", md] for c in cats if recall[t, c, "all", md] is not None] for t in T], np.float64)
        return float(arr.reshape(-1).mean()) if arr.size else -1.0
    return {"AP": ap(T, "all"), "AP50": ap([0], "all"), "AP75": ap([5], "all"), "AP_small": ap(T, "small"), "AP_medium": ap(T, "medium"),
            "AP_large": ap(T, "large"), "AR1": ar(1), "AR10": ar(10), "AR100": ar(100), "iou_type": iou_type, "detections": len(dets),
            "ground_truths": len(gts), "ignored": sum(1 for g in gts if g["ignore"]), "groups": len(groups)}
