"""BOP pose-error evaluation: MSSD, MSPD, VSD and the average recall over them, computed on the device.

``pem/results.py`` writes BOP result lines; this module scores them.  ``bop_toolkit`` is NOT part of this project and is not used:
the errors are restated here and in ``csrc/s6d_boperr.hip`` as definitions -- in the way the rasteriser and the samplers are
defined rather than imitated -- and the tests pin the kernels to an independent restatement of those definitions
(``tests/bop_ref.py``).  No number produced here is claimed to equal the toolkit's output.

Definitions (E an estimated pose, G a ground-truth pose, both object -> camera; S_j the symmetry transforms of the object; v the
vertices of its evaluation model):

  MSSD  min_j max_v |E v - G S_j v|                     (model units; ``mssd``)
  MSPD  min_j max_v |proj(E v) - proj(G S_j v)|         (pixels; ``mspd``)
  VSD   the object is rendered at E and at G (``ops.render_depth``); with the measured depth image a pixel is visible in a render
        when the rendered surface is at most ``delta`` behind the measurement (or nothing was measured), an estimate's pixel also
        where the ground truth is visible; on the union of the two visibility masks a pixel costs 1 unless it is in both and the
        two distances from the camera centre differ by less than tau; the error is the mean cost (``vsd``; 1 for an empty union).
  AR    per error an estimate is correct when the error is below a threshold; estimates are matched to ground truths greedily by
        score (``match_and_recall``); the recall is averaged over the thresholds (and the taus), AR over the three errors
        (``bop19_scores``).

  ADD   mean_i |E v_i - G v_i|;  ADD-S  mean_i min_j |E v_i - G v_j|  (``add_errors``; csrc/s6d_adderr.hip states the float32
        operations, the minimum on the bits and the fixed-order float64 mean); per target the error of the estimate assigned to it
        (``assign_errors``), recall below a fraction of the diameter and the AUC over absolute thresholds (``add_scores``: ADD,
        ADD-S, and ADD(-S) = ADD-S for objects with a symmetry set); ``symmetry_residuals`` checks a symmetry set against its mesh.

Every error function goes through ``policy.guard("eval.<name>", ...)``: kernels on device tensors, the torch statements below
otherwise (policy field ``bop_eval`` = "0", or CPU tensors).  The torch branch is chunked over the symmetries, so it does not
hold the (N, S, V, 3) tensor either.

COCO AP of ISM results (``coco_scores``).  ``ism/handoff.py`` writes the BOP / COCO detection json; this module
scores it, by the number the Instance Segmentation Model is published by.  ``pycocotools`` and ``bop_toolkit`` are not part of this
project: no number is claimed to equal their output, the following IS the definition, and the tests pin the kernels
(``csrc/s6d_cocoeval.hip``) and the torch statements below to an independent restatement of it (``tests/coco_ref.py``) with `equal`.

  instances   a detection: image index, category (object id), score, and a mask or a box x, y, w, h.  A ground truth: image index,
              category, visible mask, visible box, an ``ignore`` flag (the loader sets it from visib_fract < 0.1).  A group is one
              (image, category).
  mask IoU    inter = popcount(d & g), union = |d| + |g| - inter, integers; iou = double(inter) / double(union), one IEEE division;
              0 when union == 0.
  box IoU     float64, no fused multiply-add:  w = min(dx + dw, gx + gw) - max(dx, gx), h likewise; 0 if w <= 0 or h <= 0; else
              i = w h, u = (dw dh + gw gh) - i, iou = i / u.
  thresholds  T = np.linspace(0.5, 0.95, 10) (the ninth is 0.8999999999999999); a pair matches at t when iou >= min(t, 1 - 1e-10).
  areas       all [0, 1e10], small [0, 32^2], medium [32^2, 96^2], large [96^2, 1e10], both ends inclusive.  The ground-truth area is
              the visible mask's pixel count (both IoU types), the detection's its mask's pixel count (segm) or w h (bbox).  Within a
              range a ground truth is ignored when flagged or when its area is outside.
  matching    per group, threshold and range: the detections stable-sorted by descending score (equal scores keep input order), the
              first 100 visited in that order.  A detection takes the unmatched ground truth of highest IoU at or above the
              threshold; of equal IoUs the later in ground-truth order (non-ignored first, each part in input order); an ignored one
              only when no non-ignored one qualifies.  A detection matched to an ignored ground truth is ignored; so is an unmatched
              one whose area is outside the range.  A ground truth is matched at most once.  No crowd instances.
  accumulate  per category, threshold, range and maxDet in {1, 10, 100}: each image's first maxDet detections, concatenated over the
              images in ascending order, stable-sorted by descending score, the ignored dropped; cumulative tp and fp;
              recall = tp / n_pos (n_pos the non-ignored ground truths; a category with n_pos == 0 is left out of every mean);
              precision = tp / (tp + fp + eps), eps = np.spacing(1), made non-increasing from the right, sampled at
              np.linspace(0, 1, 101) with searchsorted(recall, r, side="left"), 0 beyond the last recall.
  reported    AP (mean over thresholds, recall levels, categories at all / 100), AP50, AP75, AP_small / medium / large (at 100),
              AR1 / AR10 / AR100 (the last recall, or 0, at all); a mean over nothing is -1.

``mask_ious``, ``box_ious`` and ``coco_match`` each have a kernel path and a ``_library`` torch statement of the same definition, used
for CPU tensors, under ``policy.disable_fused`` and -- the matching -- for groups of more than 64 ground truths.
"""
import math

import numpy as np
import torch

from . import _lib, ops, policy

BOP19 = dict(vsd_delta=15.0, vsd_taus=tuple(round(0.05 * k, 2) for k in range(1, 11)), vsd_normalized=True,
             thresholds=tuple(round(0.05 * k, 2) for k in range(1, 11)), mspd_thresholds=tuple(5.0 * k for k in range(1, 11)),
             mspd_width=640.0)


# ------------------------------------------------------------------------------------------------------------------- symmetries
def _rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def symmetry_transforms(model_info, max_sym_disc_step=0.01):
    """The symmetry transforms of one object from its ``models_info.json`` record -> (S,4,4) float64, the identity first.
    ``symmetries_discrete``: row-major 4 x 4 matrices (lists of 16).  ``symmetries_continuous``: {axis, offset}, discretised into
    n = ceil(pi / max_sym_disc_step) rotations by 2 pi k / n about the axis through ``offset``: t = offset - R offset.  Every
    discrete transform, the identity included, is composed with every continuous one:  R = Rc Rd,  t = Rc td + tc."""
    disc = [np.eye(4)] + [np.asarray(m, np.float64).reshape(4, 4) for m in model_info.get("symmetries_discrete", [])]
    cont = [np.eye(4)]
    if model_info.get("symmetries_continuous"):
        n = int(math.ceil(math.pi / max_sym_disc_step))
        cont = []
        for sym in model_info["symmetries_continuous"]:
            off = np.asarray(sym.get("offset", (0.0, 0.0, 0.0)), np.float64)
            for k in range(n):
                T = np.eye(4)
                T[:3, :3] = _rodrigues(sym["axis"], 2.0 * math.pi * k / n) if k else np.eye(3)
                T[:3, 3] = off - T[:3, :3] @ off
                cont.append(T)
    out = []
    for d in disc:
        for c in cont:
            T = np.eye(4)
            T[:3, :3] = c[:3, :3] @ d[:3, :3]
            T[:3, 3] = c[:3, :3] @ d[:3, 3] + c[:3, 3]
            out.append(T)
    return np.stack(out)


# ------------------------------------------------------------------------------------------------------------------- MSSD / MSPD
def _f32(a, dev, name, shape):
    t = torch.as_tensor(a).detach().to(device=dev, dtype=torch.float32).contiguous()
    if t.dim() != len(shape) or any(s is not None and t.shape[i] != s for i, s in enumerate(shape)):
        raise ValueError(f"{name} must have shape {tuple('*' if s is None else s for s in shape)}, got {tuple(t.shape)}")
    return t


def _compose(gt, syms, dev):
    """gt (N,4,4), syms (S,4,4) -> (N,S,4,4) float32 on dev: the products in float64 on the host, rounded once."""
    g = torch.as_tensor(gt).detach().cpu().double()
    s = torch.as_tensor(syms).detach().cpu().double()
    if g.dim() != 3 or tuple(g.shape[1:]) != (4, 4) or s.dim() != 3 or tuple(s.shape[1:]) != (4, 4) or s.shape[0] < 1:
        raise ValueError(f"gt (N,4,4) and syms (S,4,4) expected, got {tuple(g.shape)}, {tuple(s.shape)}")
    return (g[:, None] @ s[None]).float().to(dev).contiguous()


def _pose_errors_library(vertices, est, gts, cams, chunk=8):
    """The library statements of MSSD / MSPD, a chunk of symmetries at a time."""
    R, t = est[:, :3, :3], est[:, :3, 3]
    pe = vertices @ R.transpose(1, 2) + t[:, None]                         # (N,V,3)
    f, c = cams[:, None, None, :2], cams[:, None, None, 2:]
    inf = torch.full((), float("inf"), device=est.device)
    ze_ok = pe[..., 2] > 0
    ue = f[:, 0] * pe[..., :2] / pe[..., 2:] + c[:, 0]
    mssd = torch.full((est.shape[0],), float("inf"), device=est.device)
    mspd = mssd.clone()
    for s0 in range(0, gts.shape[1], chunk):
        G = gts[:, s0:s0 + chunk]
        pg = vertices @ G[..., :3, :3].transpose(2, 3) + G[..., :3, 3][:, :, None]          # (N,s,V,3)
        d3 = (pe[:, None] - pg).norm(dim=3)
        d3 = torch.where(torch.isfinite(d3), d3, inf)
        ug = f * pg[..., :2] / pg[..., 2:] + c
        d2 = (ue[:, None] - ug).norm(dim=3)
        d2 = torch.where(torch.isfinite(d2) & ze_ok[:, None] & (pg[..., 2] > 0), d2, inf)
        mssd = torch.minimum(mssd, d3.max(2)[0].min(1)[0])
        mspd = torch.minimum(mspd, d2.max(2)[0].min(1)[0])
    return mssd, mspd


def _kernels(site, t, name):
    return policy.current().bop_eval == "1" and policy.guard(site, cuda=t.is_cuda, have=ops.have(name))


@torch.no_grad()
def pose_errors(vertices, est, gt, syms, cams, site="eval.pose_errors"):
    """(mssd (N,), mspd (N,)) float32 for N estimates of ONE object: vertices (V,3), est (N,4,4), gt (N,4,4) object -> camera
    (translation in model units), syms (S,4,4) (``symmetry_transforms``), cams (N,4) = fx fy cx cy.  Tensors on the device of
    ``est`` (numpy arrays and other tensors are copied there)."""
    dev = est.device if torch.is_tensor(est) else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    e = _f32(est, dev, "est", (None, 4, 4))
    v = _f32(vertices, dev, "vertices", (None, 3))
    k = _f32(cams, dev, "cams", (e.shape[0], 4))
    g = _compose(gt, syms, dev)
    if g.shape[0] != e.shape[0]:
        raise ValueError(f"{e.shape[0]} estimates but {g.shape[0]} ground truths")
    if e.shape[0] == 0:
        return torch.zeros(0, device=dev), torch.zeros(0, device=dev)
    if _kernels(site, e, "pose_errors"):
        return ops.pose_errors(v, e, g, k)
    return _pose_errors_library(v, e, g, k)


def mssd(vertices, est, gt, syms):
    """Maximum symmetry-aware surface distance of N estimates of one object -> (N,) float32, model units."""
    n = (est.shape[0] if hasattr(est, "shape") else len(est))
    cams = torch.tensor([[1.0, 1.0, 0.0, 0.0]]).repeat(n, 1)
    return pose_errors(vertices, est, gt, syms, cams, site="eval.mssd")[0]


def mspd(vertices, est, gt, syms, cams):
    """Maximum symmetry-aware projection distance of N estimates of one object -> (N,) float32, pixels; +inf where a vertex lies
    at Z <= 0 under every symmetry."""
    return pose_errors(vertices, est, gt, syms, cams, site="eval.mspd")[1]


# ------------------------------------------------------------------------------------------------------------------- ADD / ADD-S
ADD_LANES, ADD_WAVE = 256, 64          # the summation order of csrc/s6d_adderr.hip: 256 lanes striding, waves of 64


def _row_mean_fixed(values):
    """(N,V) float32 -> (N,) float64: the mean in the FIXED order of row_mean_max_kernel.  Lane l adds i = l, l + 256, ... from +0
    (a row is padded with +0, which changes no sum), the wave by the xor butterfly x += x[lane ^ o], o = 32 .. 1, the waves in
    order ((w0 + w1) + w2) + w3; one division by V."""
    N, V = values.shape
    K = -(-V // ADD_LANES)
    x = torch.zeros(N, K * ADD_LANES, dtype=torch.float64, device=values.device)
    x[:, :V] = values.double()
    x = x.view(N, K, ADD_LANES)
    acc = torch.zeros(N, ADD_LANES, dtype=torch.float64, device=values.device)
    for k in range(K):
        acc = acc + x[:, k]
    acc = acc.view(N, ADD_LANES // ADD_WAVE, ADD_WAVE)
    lane = torch.arange(ADD_WAVE, device=values.device)
    o = ADD_WAVE // 2
    while o:
        acc = acc + acc[:, :, lane ^ o]
        o //= 2
    s = acc[:, 0, 0]
    for w in range(1, ADD_LANES // ADD_WAVE):
        s = s + acc[:, w, 0]
    return s / torch.full_like(s, float(V))          # a tensor divisor: one IEEE division (a scalar one becomes a product by 1 / V on the device)


def _add_errors_library(vertices, est, gts, which=("add", "adds"), chunk_bytes=1 << 26):
    """The library statement of ``ops.add_errors`` (its dict, the per-vertex values always given): the same float32 operations, a
    chunk of source rows against all target vertices at a time -- never an (N, V, V) tensor."""
    V, N = vertices.shape[0], est.shape[0]
    vx, vy, vz = vertices[:, 0], vertices[:, 1], vertices[:, 2]
    inf = torch.tensor(float("inf"), device=est.device)

    def transform(P):                                                      # three (N,V): X = ((r00 vx + r01 vy) + r02 vz) + tx
        return [((P[:, r, 0, None] * vx + P[:, r, 1, None] * vy) + P[:, r, 2, None] * vz) + P[:, r, 3, None] for r in range(3)]

    def root(d2):                                                          # the correctly rounded float32 root: through float64 (53 >= 2 * 24 + 2
        return torch.sqrt(torch.where(torch.isfinite(d2), d2, inf).double()).float()   # bits), torch's vectorised float32 sqrt is not

    E, G = transform(est), transform(gts)
    out = dict(add=None, add_max=None, add_per_vertex=None, adds=None, adds_max=None, adds_per_vertex=None)
    for name in which:
        if name == "add":
            dx, dy, dz = E[0] - G[0], E[1] - G[1], E[2] - G[2]
            pv = root((dx * dx + dy * dy) + dz * dz)
        elif name == "adds":
            pv = torch.empty(N, V, dtype=torch.float32, device=est.device)
            step = max(1, chunk_bytes // (16 * V))
            for n in range(N):
                for i in range(0, V, step):
                    dx, dy, dz = (E[c][n, i:i + step, None] - G[c][n, None, :] for c in range(3))
                    d2 = (dx * dx + dy * dy) + dz * dz
                    pv[n, i:i + step] = root(torch.where(torch.isfinite(d2), d2, inf).min(1)[0])
        else:
            raise ValueError(f"add_errors: which names 'add' and 'adds', got {name!r}")
        out[name + "_per_vertex"], out[name], out[name + "_max"] = pv, _row_mean_fixed(pv), pv.max(1)[0]
    return out


@torch.no_grad()
def add_errors(vertices, est, gt, which=("add", "adds"), chunk_bytes=1 << 28, per_vertex=False):
    """ADD and ADD-S of N (estimate, ground truth) pose pairs of ONE object, as defined in csrc/s6d_adderr.hip: vertices (V,3),
    est, gt (N,4,4) object -> camera, translation in model units -> dict of tensors on the device of ``est``:
    add, adds (N,) float64 = the mean over the vertices of |E v_i - G v_i| and of min_j |E v_i - G v_j|; add_max, adds_max (N,)
    float32 (adds_max: the one-sided Hausdorff distance); add_per_vertex, adds_per_vertex (N,V) float32 when ``per_vertex``, else
    None.  The keys of an error not named in ``which`` are None.  The estimates go through the kernels in chunks over N whose
    per-vertex values stay under ``chunk_bytes``; every chunking gives the same bits.  No symmetry set enters: ADD-S needs none."""
    dev = est.device if torch.is_tensor(est) else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    e = _f32(est, dev, "est", (None, 4, 4))
    N = e.shape[0]
    g = _f32(gt, dev, "gt", (N, 4, 4))
    v = _f32(vertices, dev, "vertices", (None, 3))
    V = v.shape[0]
    which = tuple(which)
    if V < 1 or any(w not in ("add", "adds") for w in which):
        raise ValueError(f"add_errors: at least one vertex and which within ('add', 'adds') expected, got V = {V}, which = {which}")
    kernels = N > 0 and policy.current().bop_eval == "1" and policy.guard("eval.add_errors", cuda=e.is_cuda,
                                                                         have=ops.have("add_errors") and ops.have("adds_errors"))
    step = max(1, min(int(chunk_bytes) // (4 * V), (2 ** 31 - 1) // V))
    parts = []
    for i in range(0, N, step):
        if kernels:
            parts.append(ops.add_errors(v, e[i:i + step], g[i:i + step], per_vertex=per_vertex, which=which))
        else:
            parts.append(_add_errors_library(v, e[i:i + step], g[i:i + step], which, chunk_bytes=min(int(chunk_bytes), 1 << 26)))
    out = dict(add=None, add_max=None, add_per_vertex=None, adds=None, adds_max=None, adds_per_vertex=None)
    for w in which:
        for key, dtype, shape in ((w, torch.float64, (0,)), (w + "_max", torch.float32, (0,)), (w + "_per_vertex", torch.float32, (0, V))):
            if per_vertex or key != w + "_per_vertex":
                out[key] = torch.cat([p[key] for p in parts]) if parts else torch.zeros(shape, dtype=dtype, device=dev)
    return out


def _group_ids(estimates, ground_truths):
    """(image, object) groups of the ground truths -> (est_group (E,) with -1 for an estimate in no group, gt_group (G,), keys)."""
    e_im, e_obj = np.asarray(estimates["im"], np.int64), np.asarray(estimates["obj"], np.int64)
    g_im, g_obj = np.asarray(ground_truths["im"], np.int64), np.asarray(ground_truths["obj"], np.int64)
    keys = sorted(set(zip(g_im.tolist(), g_obj.tolist())))
    gid = {k: i for i, k in enumerate(keys)}
    gt_group = np.array([gid[k] for k in zip(g_im.tolist(), g_obj.tolist())], np.int64)
    est_group = np.array([gid.get(k, -1) for k in zip(e_im.tolist(), e_obj.tolist())], np.int64)
    return est_group, gt_group, keys


def assign_errors(errors, scores, est_group, gt_group, n_targets):
    """One error per target instance, on the host in float64.  errors: the triple (pair_est, pair_gt, pair_error) of the computed
    pairs, or an (E,G) array; only pairs whose estimate and ground truth share a group count.  scores (E,); est_group (E,),
    gt_group (G,): group ids in [0, len(n_targets)) (an estimate with another id is in no group); n_targets (groups,).
    Per group the n_targets highest-scoring estimates are kept (ties: the lower index) and visited in descending score; each takes
    the still unmatched ground truth of its group with the lowest error (ties: the lower index).  There is no threshold: the
    assignment does not depend on one.  -> dict(error (G,) float64, +inf for a ground truth no estimate took; estimate (G,) int64,
    -1 there)."""
    scores, est_group, gt_group = np.asarray(scores, np.float64), np.asarray(est_group, np.int64), np.asarray(gt_group, np.int64)
    n_targets = np.asarray(n_targets, np.int64)
    if isinstance(errors, tuple):
        pe, pg, pv = (np.asarray(a) for a in errors)
    else:
        err = np.asarray(errors, np.float64)
        pe, pg = np.nonzero(est_group[:, None] == gt_group[None, :])
        pv = err[pe, pg]
    pe, pg, pv = pe.astype(np.int64), pg.astype(np.int64), np.asarray(pv, np.float64)
    same = est_group[pe] == gt_group[pg] if len(pe) else np.zeros(0, bool)
    pe, pg, pv = pe[same], pg[same], np.where(np.isnan(pv[same]), np.inf, pv[same])          # a NaN error counts as +inf
    by_est = {}
    for i in np.lexsort((pg, pe)):
        by_est.setdefault(int(pe[i]), []).append((int(pg[i]), float(pv[i])))
    error = np.full(len(gt_group), np.inf)
    taker = np.full(len(gt_group), -1, np.int64)
    for grp in range(len(n_targets)):
        es = np.nonzero(est_group == grp)[0]
        es = es[np.lexsort((es, -scores[es]))][:int(n_targets[grp])]
        for e in es:
            best, best_err = -1, float("inf")
            for g, x in by_est.get(int(e), ()):
                if taker[g] < 0 and (best < 0 or x < best_err):             # by ground-truth index: the first stays on ties
                    best, best_err = g, x
            if best >= 0:
                taker[best] = int(e)
                error[best] = best_err
    return dict(error=error, estimate=taker)


def _recall_auc(error, threshold, auc_max):
    """recall = #{e_k < threshold_k} / targets;  AUC = mean_k max(0, 1 - e_k / auc_max): the exact area under the step curve
    t -> #{e_k < t} / targets on [0, auc_max], divided by auc_max.  0 for no targets."""
    if not len(error):
        return 0.0, 0.0
    with np.errstate(all="ignore"):
        return float((error < threshold).mean()), float(np.maximum(0.0, 1.0 - error / float(auc_max)).mean())


def _is_symmetric(model):
    if model.get("symmetric"):
        return True
    syms = model["symmetries"] if "symmetries" in model else symmetry_transforms(model.get("info", {}))
    return len(syms) > 1


@torch.no_grad()
def add_scores(models, estimates, ground_truths, frac=0.1, auc_max=100.0, device=None):
    """ADD, ADD-S and ADD(-S) recall and AUC of a set of estimates.  models, estimates, ground_truths as in ``bop19_scores`` (no
    faces, no images needed); a model may carry ``symmetric=True``.  Every estimate is scored against every ground truth of its
    (image, object) group (``add_errors``), the errors are assigned to the targets by ``assign_errors``, and from the per-target
    errors e_k:  recall = #{e_k < frac * diameter} / targets,  AUC = mean_k max(0, 1 - e_k / auc_max)  (auc_max in model units: 100
    is 10 cm for BOP's millimetre models).  ADD(-S) takes ADD-S for an object whose symmetry set has more than the identity (or
    that is flagged ``symmetric``) and ADD otherwise.
    -> dict(ADD, ADD_S, ADD_or_S: each dict(recall, auc); frac, auc_max, targets, estimates)."""
    dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    est_group, gt_group, keys = _group_ids(estimates, ground_truths)
    g_obj = np.asarray(ground_truths["obj"], np.int64)
    e_pose = np.asarray(estimates["pose"], np.float64).reshape(-1, 4, 4)
    g_pose = np.asarray(ground_truths["pose"], np.float64).reshape(-1, 4, 4)
    n_targets = np.bincount(gt_group, minlength=len(keys))
    E, G = len(est_group), len(gt_group)
    pe, pg = np.nonzero((est_group[:, None] == gt_group[None, :]) & (est_group[:, None] >= 0)) if E and G else (np.zeros(0, np.int64),) * 2
    err = dict(add=np.zeros(len(pe)), adds=np.zeros(len(pe)))
    diameter, symmetric = np.zeros(G), np.zeros(G, bool)
    for obj in sorted(set(g_obj.tolist())):
        m = models[obj]
        diameter[g_obj == obj] = float(m["diameter"] if "diameter" in m else m["info"]["diameter"])
        symmetric[g_obj == obj] = _is_symmetric(m)
        sel = np.nonzero(g_obj[pg] == obj)[0]
        if not len(sel):
            continue
        r = add_errors(m["vertices"], torch.as_tensor(e_pose[pe[sel]]).to(dev).float(), g_pose[pg[sel]])
        err["add"][sel], err["adds"][sel] = r["add"].cpu().numpy(), r["adds"].cpu().numpy()
    scores = np.asarray(estimates["score"], np.float64)
    per_target = {k: assign_errors((pe, pg, err[k]), scores, est_group, gt_group, n_targets)["error"] for k in ("add", "adds")}
    per_target["add_or_s"] = assign_errors((pe, pg, np.where(symmetric[pg], err["adds"], err["add"])), scores, est_group, gt_group,
                                           n_targets)["error"]
    out = {}
    for name, key in (("ADD", "add"), ("ADD_S", "adds"), ("ADD_or_S", "add_or_s")):
        recall, auc = _recall_auc(per_target[key], float(frac) * diameter, auc_max)
        out[name] = dict(recall=recall, auc=auc)
    out.update(frac=float(frac), auc_max=float(auc_max), targets=int(n_targets.sum()), estimates=int(E))
    return out


@torch.no_grad()
def symmetry_residuals(vertices, syms, diameter=None, device=None):
    """Do the symmetry transforms map the mesh onto itself?  vertices (V,3), syms (S,4,4) (``symmetry_transforms``) -> dict(mean (S,)
    float64, max (S,) float64: the mean and the maximum over the vertices of min_k |S_j v_i - v_k| -- one call of the ADD-S path with
    est = S_j and gt = I; with a ``diameter`` also mean_fraction, max_fraction = those over the diameter).  0 for a transform that
    maps the vertex set into itself; MSSD, MSPD and ADD-S are silently wrong for one that does not."""
    s = np.asarray(torch.as_tensor(syms).detach().cpu().double().numpy()).reshape(-1, 4, 4)
    dev = torch.device(device) if device is not None else (vertices.device if torch.is_tensor(vertices) else
                                                           torch.device("cuda" if torch.cuda.is_available() else "cpu"))
    r = add_errors(vertices, torch.as_tensor(s).to(dev).float(), np.tile(np.eye(4), (len(s), 1, 1)), which=("adds",))
    out = dict(mean=r["adds"].cpu().numpy().astype(np.float64), max=r["adds_max"].cpu().numpy().astype(np.float64))
    if diameter is not None:
        out.update(mean_fraction=out["mean"] / float(diameter), max_fraction=out["max"] / float(diameter))
    return out


# ------------------------------------------------------------------------------------------------------------------- VSD
def _render_depth_library(vertices, faces, poses, cams, H, W, znear):
    """Depth renders in torch statements, for checking and for CPU tensors: the vertex stage and the coverage rule of
    csrc/s6d_raster.hip (float32 vertices snapped to 1/256 pixel, integer edge functions, top-left rule, no clipping), the depth
    interpolated in float64.  One pass over the whole frame per face: for small meshes."""
    dev, T = vertices.device, poses.shape[0]
    v = vertices
    P = poses
    cam = [((P[:, r, 0, None] * v[:, 0] + P[:, r, 1, None] * v[:, 1]) + P[:, r, 2, None] * v[:, 2]) + P[:, r, 3, None] for r in range(3)]   # (T,V)
    Z = cam[2]
    xs = ((cams[:, 0, None] * cam[0]) / Z + cams[:, 2, None]) * 256.0
    ys = ((cams[:, 1, None] * cam[1]) / Z + cams[:, 3, None]) * 256.0
    ok = (Z > znear) & (xs.abs() <= 2.0 ** 23) & (ys.abs() <= 2.0 ** 23)
    xi = torch.round(torch.where(ok, xs, torch.zeros_like(xs))).long()
    yi = torch.round(torch.where(ok, ys, torch.zeros_like(ys))).long()
    px = (torch.arange(W, device=dev) * 256)[None, None, :]
    py = (torch.arange(H, device=dev) * 256)[None, :, None]
    depth = torch.full((T, H, W), float("inf"), dtype=torch.float64, device=dev)
    skipped = torch.zeros(T, dtype=torch.int32, device=dev)
    Zd = Z.double()
    for tri in faces.tolist():
        good = ok[:, tri[0]] & ok[:, tri[1]] & ok[:, tri[2]]
        skipped += (~good).int()
        x, y = xi[:, tri], yi[:, tri]                                      # (T,3)
        a2 = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
        s = torch.sign(a2)
        inside = (good & (a2 != 0))[:, None, None].expand(T, H, W).clone()
        iz = torch.zeros(T, H, W, dtype=torch.float64, device=dev)
        for k in range(3):
            a, b = (k + 1) % 3, (k + 2) % 3
            dx, dy = (s * (x[:, b] - x[:, a]))[:, None, None], (s * (y[:, b] - y[:, a]))[:, None, None]
            w = dx * (py - y[:, a, None, None]) - dy * (px - x[:, a, None, None])
            own = (dy < 0) | ((dy == 0) & (dx > 0))
            inside &= (w > 0) | ((w == 0) & own)
            iz += (w.double() / a2.abs().clamp(min=1).double()[:, None, None]) / Zd[:, tri[k], None, None]
        z = torch.where(inside, 1.0 / torch.where(inside, iz, torch.ones_like(iz)), torch.full_like(iz, float("inf")))
        depth = torch.minimum(depth, z)
    return dict(depth=torch.where(torch.isfinite(depth), depth, torch.zeros_like(depth)).float(), skipped=skipped)


def _vsd_counts_library(de, dg, dt, test_index, cams, delta, taus, scale):
    """The library statements of the per-pixel stage."""
    H, W = de.shape[1:]
    zt = dt[test_index.long()]
    u = torch.arange(W, dtype=torch.float32, device=de.device)[None, None, :]
    v = torch.arange(H, dtype=torch.float32, device=de.device)[None, :, None]
    fx, fy, cx, cy = (cams[:, k, None, None] for k in range(4))
    r = torch.sqrt(((u - cx) / fx) ** 2 + ((v - cy) / fy) ** 2 + 1.0)
    De, Dg, Dt = de * r, dg * r, zt * r
    vis_gt = (dg > 0) & (((Dg - Dt) <= delta) | (zt == 0))
    vis_est = (de > 0) & (((De - Dt) <= delta) | (zt == 0) | vis_gt)
    inter, union = vis_gt & vis_est, vis_gt | vis_est
    x = (Dg - De).abs() / scale[:, None, None]
    ge = torch.stack([(inter & (x >= float(np.float32(t)))).sum((1, 2)) for t in taus], 1)
    return union.sum((1, 2)).int(), inter.sum((1, 2)).int(), ge.int()


@torch.no_grad()
def vsd(vertices, faces, est, gt, cams, depth_test, test_index, diameter, *, delta=BOP19["vsd_delta"], taus=BOP19["vsd_taus"],
        normalized=True, znear=1.0):
    """Visible surface discrepancy of N (estimate, ground truth) pairs of ONE object.  vertices (V,3), faces (F,3) int32,
    est, gt (N,4,4) object -> camera, cams (N,4), depth_test (M,H,W) float32 measured depth in model units (0 = missing),
    test_index (N,) into M, diameter of the object; taus: at most 16 tolerances, fractions of the diameter when ``normalized``.
    All estimates go through ONE ``ops.render_depth`` call and all ground truths through another.
    -> dict(errors (N,NT) float64 numpy, unrenderable (N,) bool numpy, union, inter (N,), ge (N,NT) int numpy).  A pair with
    skipped triangles in either render (a vertex behind ``znear``: there is no clipping) is reported in ``unrenderable`` and
    given error 1; it is never silently scored."""
    dev = est.device if torch.is_tensor(est) else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    e = _f32(est, dev, "est", (None, 4, 4))
    N = e.shape[0]
    g = _f32(gt, dev, "gt", (N, 4, 4))
    v = _f32(vertices, dev, "vertices", (None, 3))
    k = _f32(cams, dev, "cams", (N, 4))
    dt = _f32(depth_test, dev, "depth_test", (None, None, None))
    f = torch.as_tensor(faces).detach().to(device=dev, dtype=torch.int32).contiguous()
    ti = torch.as_tensor(test_index).detach().to(device=dev, dtype=torch.int32).contiguous()
    taus = [float(t) for t in taus]
    if tuple(ti.shape) != (N,) or f.dim() != 2 or f.shape[1] != 3 or not 1 <= len(taus) <= 16:
        raise ValueError(f"test_index (N,), faces (F,3) and 1 .. 16 taus expected, got {tuple(ti.shape)}, {tuple(f.shape)}, {len(taus)} taus")
    H, W = dt.shape[1:]
    NT = len(taus)
    if N == 0:
        z = np.zeros(0, np.int64)
        return dict(errors=np.zeros((0, NT)), unrenderable=np.zeros(0, bool), union=z, inter=z, ge=np.zeros((0, NT), np.int64))
    scale = torch.full((N,), float(diameter) if normalized else 1.0, dtype=torch.float32, device=dev)
    if policy.current().bop_eval == "1" and policy.guard("eval.vsd", cuda=e.is_cuda, have=ops.have("vsd_counts") and ops.have("render_depth")):
        re, rg = ops.render_depth(v, f, e, k, H, W, znear), ops.render_depth(v, f, g, k, H, W, znear)
        union, inter, ge = ops.vsd_counts(re["depth"], rg["depth"], dt, ti, k, delta, taus, scale)
    else:
        if N and (int(ti.min()) < 0 or int(ti.max()) >= dt.shape[0]):
            raise ValueError(f"vsd: test_index must lie in [0, {dt.shape[0]})")
        re, rg = _render_depth_library(v, f, e, k, H, W, znear), _render_depth_library(v, f, g, k, H, W, znear)
        union, inter, ge = _vsd_counts_library(re["depth"], rg["depth"], dt, ti, k, float(delta), taus, scale)
    bad = ((re["skipped"] != 0) | (rg["skipped"] != 0)).cpu().numpy()
    un, it, gek = union.cpu().numpy().astype(np.int64), inter.cpu().numpy().astype(np.int64), ge.cpu().numpy().astype(np.int64)
    with np.errstate(all="ignore"):
        err = (gek + (un - it)[:, None]).astype(np.float64) / un[:, None].astype(np.float64)
    err = np.where((un[:, None] > 0) & ~bad[:, None], err, 1.0)
    return dict(errors=err, unrenderable=bad, union=un, inter=it, ge=gek)


# ------------------------------------------------------------------------------------------------------------------- matching
def match_and_recall(errors, scores, est_group, gt_group, n_targets, thresholds):
    """Greedy matching of estimates to ground truths and the recall, per threshold; on the host.

    errors: (E,G) array, the error of estimate e against ground truth g -- or the triple (pair_est, pair_gt, pair_error) of the
    computed pairs; only pairs whose estimate and ground truth share a group count.  scores (E,).  est_group (E,), gt_group (G,):
    ids of the (image, object) groups, integers in [0, len(n_targets)).  n_targets (groups,): the number of target instances of
    every group.  Per threshold and group: the n_targets highest-scoring estimates are kept (ties: the lower index), gone through
    in descending score; each takes the unmatched ground truth of its group with the lowest error below the threshold (ties: the
    lower index).  -> numpy (len(thresholds),): matched targets over all targets."""
    scores, est_group, gt_group = np.asarray(scores, np.float64), np.asarray(est_group, np.int64), np.asarray(gt_group, np.int64)
    n_targets = np.asarray(n_targets, np.int64)
    if isinstance(errors, tuple):
        pe, pg, pv = (np.asarray(a) for a in errors)
    else:
        err = np.asarray(errors, np.float64)
        pe, pg = np.nonzero(est_group[:, None] == gt_group[None, :])
        pv = err[pe, pg]
    same = est_group[pe] == gt_group[pg]
    pe, pg, pv = pe[same].astype(np.int64), pg[same].astype(np.int64), np.asarray(pv, np.float64)[same]
    by_est = {}
    for i in np.lexsort((pg, pe)):
        by_est.setdefault(int(pe[i]), []).append((int(pg[i]), float(pv[i])))
    kept = []
    for grp in range(len(n_targets)):
        es = np.nonzero(est_group == grp)[0]
        es = es[np.lexsort((es, -scores[es]))][:int(n_targets[grp])]
        kept.append([int(e) for e in es])
    total = int(n_targets.sum())
    out = np.zeros(len(thresholds))
    for i, th in enumerate(thresholds):
        matched = 0
        for es in kept:
            taken = set()
            for e in es:
                best, best_err = -1, float("inf")
                for g, v in by_est.get(e, ()):
                    if g not in taken and v < th and v < best_err:
                        best, best_err = g, v
                if best >= 0:
                    taken.add(best)
                    matched += 1
        out[i] = matched / total if total else 0.0
    return out


@torch.no_grad()
def bop19_scores(models, estimates, ground_truths, images, device=None):
    """The BOP19 average recall of a set of estimates.

    models: {obj_id: dict(vertices (V,3), faces (F,3), diameter, symmetries (S,4,4) -- or ``info``, the models_info.json record)}.
    estimates: dict(im (E,), obj (E,), score (E,), pose (E,4,4)); ground_truths: dict(im (G,), obj (G,), pose (G,4,4)), the target
    instances only; ``im`` indexes ``images`` = dict(cams (I,4), depth (I,H,W) float32 in model units).  Poses object -> camera,
    translation in model units (millimetres for BOP models).
    Parameters (BOP19): VSD with delta = 15, taus 0.05 .. 0.5 of the diameter, correct below theta = 0.05 .. 0.5; MSSD correct
    below 0.05 .. 0.5 of the diameter; MSPD correct below 5 .. 50 pixels times W / 640.
    -> dict(AR, AR_VSD, AR_MSSD, AR_MSPD, recalls_VSD (taus, thetas), recalls_MSSD, recalls_MSPD, unrenderable)."""
    dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    e_im, e_obj = np.asarray(estimates["im"], np.int64), np.asarray(estimates["obj"], np.int64)
    g_im, g_obj = np.asarray(ground_truths["im"], np.int64), np.asarray(ground_truths["obj"], np.int64)
    e_pose, g_pose = np.asarray(estimates["pose"], np.float64).reshape(-1, 4, 4), np.asarray(ground_truths["pose"], np.float64).reshape(-1, 4, 4)
    cams = np.asarray(images["cams"], np.float32)
    depth = torch.as_tensor(images["depth"]).to(device=dev, dtype=torch.float32).contiguous()
    W = depth.shape[2]
    keys = sorted(set(zip(g_im.tolist(), g_obj.tolist())))
    gid = {k: i for i, k in enumerate(keys)}
    gt_group = np.array([gid[k] for k in zip(g_im.tolist(), g_obj.tolist())], np.int64)
    est_group = np.array([gid.get(k, -1) for k in zip(e_im.tolist(), e_obj.tolist())], np.int64)
    n_targets = np.bincount(gt_group, minlength=len(keys))
    pe, pg = np.nonzero((est_group[:, None] == gt_group[None, :]) & (est_group[:, None] >= 0)) if len(e_im) and len(g_im) else (np.zeros(0, np.int64),) * 2
    taus, thetas = BOP19["vsd_taus"], BOP19["thresholds"]
    err = dict(mssd=np.zeros(len(pe)), mspd=np.zeros(len(pe)), vsd=np.ones((len(pe), len(taus))))
    unrenderable = 0
    for obj in sorted(set(g_obj.tolist())):
        sel = np.nonzero(g_obj[pg] == obj)[0]
        if not len(sel):
            continue
        m = models[obj]
        syms = m["symmetries"] if "symmetries" in m else symmetry_transforms(m.get("info", {}))
        diameter = float(m["diameter"] if "diameter" in m else m["info"]["diameter"])
        E = torch.as_tensor(e_pose[pe[sel]]).to(dev).float()
        k = torch.as_tensor(cams[g_im[pg[sel]]]).to(dev)
        d3, d2 = pose_errors(m["vertices"], E, g_pose[pg[sel]], syms, k)
        err["mssd"][sel] = d3.cpu().numpy().astype(np.float64) / diameter
        err["mspd"][sel] = d2.cpu().numpy().astype(np.float64)
        r = vsd(m["vertices"], m["faces"], E, g_pose[pg[sel]], k, depth, g_im[pg[sel]], diameter, delta=BOP19["vsd_delta"], taus=taus,
                normalized=BOP19["vsd_normalized"])
        err["vsd"][sel] = r["errors"]
        unrenderable += int(r["unrenderable"].sum())
    scores = np.asarray(estimates["score"], np.float64)
    args = (scores, est_group, gt_group, n_targets)
    rec_mssd = match_and_recall((pe, pg, err["mssd"]), *args, thetas)
    rec_mspd = match_and_recall((pe, pg, err["mspd"]), *args, [t * W / BOP19["mspd_width"] for t in BOP19["mspd_thresholds"]])
    rec_vsd = np.stack([match_and_recall((pe, pg, err["vsd"][:, j]), *args, thetas) for j in range(len(taus))])
    out = {"AR_VSD": float(rec_vsd.mean()), "AR_MSSD": float(rec_mssd.mean()), "AR_MSPD": float(rec_mspd.mean())}
    out["AR"] = (out["AR_VSD"] + out["AR_MSSD"] + out["AR_MSPD"]) / 3.0
    out.update(recalls_VSD=rec_vsd.tolist(), recalls_MSSD=rec_mssd.tolist(), recalls_MSPD=rec_mspd.tolist(), unrenderable=unrenderable,
               targets=int(n_targets.sum()), estimates=int(len(e_im)))
    return out


# ------------------------------------------------------------------------------------------------------------------- result files
def read_bop_csv(path):
    """The inverse of ``pem.results.write_bop_csv``: ``scene,im,obj,score,R (9 values),t (3 values, millimetres),time`` lines ->
    dict(scene (n,), im (n,), obj (n,) int64, score (n,) float32, R (n,3,3) float32, t (n,3) float32 millimetres, time (n,)
    float64).  A header line (``scene_id,...``) is read over."""
    rows = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            line = line.strip()
            if not line or line.startswith("scene_id"):
                continue
            w = line.split(",")
            if len(w) != 7 or len(w[4].split()) != 9 or len(w[5].split()) != 3:
                raise ValueError(f"{path}:{ln}: not a BOP result line")
            rows.append(w)
    n = len(rows)
    return dict(scene=np.array([int(w[0]) for w in rows], np.int64), im=np.array([int(w[1]) for w in rows], np.int64),
                obj=np.array([int(w[2]) for w in rows], np.int64), score=np.array([w[3] for w in rows], np.float32).reshape(n),
                R=np.array([w[4].split() for w in rows], np.float32).reshape(n, 3, 3),
                t=np.array([w[5].split() for w in rows], np.float32).reshape(n, 3), time=np.array([float(w[6]) for w in rows], np.float64))


# ------------------------------------------------------------------------------------------------------------------- COCO AP
COCO_THRESHOLDS = np.linspace(0.5, 0.95, 10)                                # float64; the ninth is 0.8999999999999999
COCO_AREA_RANGES = np.array([[0.0, 1e10], [0.0, 32.0 ** 2], [32.0 ** 2, 96.0 ** 2], [96.0 ** 2, 1e10]])   # all, small, medium, large
COCO_MAX_DETS = (1, 10, 100)
COCO_RECALL_LEVELS = np.linspace(0.0, 1.0, 101)
COCO_MIN_VISIB = 0.1                                                        # a ground truth below this visib_fract is ignored


def _coco_kernels(site, t, *names):
    return policy.guard(site, cuda=t.is_cuda, have=all(ops.have(n) for n in names))


def _coco_device(device, *operands):
    if device is not None:
        return torch.device(device)
    for t in operands:
        if torch.is_tensor(t):
            return t.device
    return torch.device("cuda" if torch.cuda.is_available() else "cpu")


def _masks_u8(m, dev):
    t = torch.as_tensor(m).detach()
    if t.dim() != 3:
        raise ValueError(f"masks must have shape (N,H,W), got {tuple(t.shape)}")
    if t.dtype not in (torch.bool, torch.uint8):
        t = t != 0
    t = t.to(dev).contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def _pairs_i32(pairs, dev, n_det, n_gt):
    p = torch.as_tensor(pairs).detach().to(device=dev, dtype=torch.int32).reshape(-1, 2).contiguous()
    if p.shape[0] and (int(p.min()) < 0 or int(p[:, 0].max()) >= n_det or int(p[:, 1].max()) >= n_gt):
        raise ValueError(f"pairs must index rows [0, {n_det}) and [0, {n_gt})")
    return p


def _mask_counts_library(dm, gm, pairs, chunk_bytes=1 << 28):
    """The library statement of the mask counts: dense products, a chunk of pairs at a time."""
    da, ga = (dm != 0).flatten(1).sum(1).int(), (gm != 0).flatten(1).sum(1).int()
    hw = max(1, dm.shape[1] * dm.shape[2])
    step = max(1, chunk_bytes // hw)
    p = pairs.long()
    inter = [((dm[p[i:i + step, 0]] != 0) & (gm[p[i:i + step, 1]] != 0)).flatten(1).sum(1).int() for i in range(0, p.shape[0], step)]
    return (torch.cat(inter) if inter else torch.zeros(0, dtype=torch.int32, device=dm.device)), da, ga


def _is_rle(m):
    from .ism import handoff
    return isinstance(m, handoff.RleMasks)


def _mask_operand(m, dev):
    """Masks for the counts: run lists (``handoff.RleMasks``) moved to dev as they are, everything else dense (N,H,W) uint8 on dev."""
    return m.to(dev) if _is_rle(m) else _masks_u8(m, dev)


def _mask_shape(m):
    return (len(m),) + tuple(m.size) if _is_rle(m) else tuple(m.shape)


def _mask_areas(m, dev):
    """Set pixels of every mask -> (N,) float64 on dev."""
    m = _mask_operand(m, dev)
    if _is_rle(m):
        return m.packed()[1].double()
    return m.flatten(1).ne(0).sum(1).double()


def _mask_counts(det_masks, gt_masks, pairs, device=None, site="eval.mask_ious"):
    dev = _coco_device(device, *(m.counts if _is_rle(m) else m for m in (det_masks, gt_masks)))
    dm, gm = _mask_operand(det_masks, dev), _mask_operand(gt_masks, dev)
    ds, gs = _mask_shape(dm), _mask_shape(gm)
    if ds[1:] != gs[1:] and ds[0] and gs[0]:
        raise ValueError(f"detection masks are {ds[1:]}, ground-truth masks {gs[1:]}")
    p = _pairs_i32(pairs, dev, ds[0], gs[0])
    need = ["mask_pair_inter"] + ([] if _is_rle(dm) and _is_rle(gm) else ["mask_pack"])
    if ds[1] * ds[2] >= 1 and gs[1] * gs[2] >= 1 and _coco_kernels(site, p if _is_rle(dm) else dm, *need):
        # run lists go straight to the packed words (``RleMasks.packed``: ops.rle_to_packed), dense masks through ops.mask_pack
        dp, da = dm.packed() if _is_rle(dm) else ops.mask_pack(dm)
        gp, ga = gm.packed() if _is_rle(gm) else ops.mask_pack(gm)
        inter = ops.mask_pair_inter(dp, gp, p) if p.shape[0] else torch.zeros(0, dtype=torch.int32, device=dev)
        return inter, da, ga, p
    dm, gm = (m.to_dense().view(torch.uint8) if _is_rle(m) else m for m in (dm, gm))
    return _mask_counts_library(dm, gm, p) + (p,)


def _iou_from_counts(inter, da, ga, p):
    i = inter.long()
    u = da.long()[p[:, 0].long()] + ga.long()[p[:, 1].long()] - i
    return torch.where(u > 0, i.double() / u.clamp(min=1).double(), torch.zeros_like(i, dtype=torch.float64))


@torch.no_grad()
def mask_ious(det_masks, gt_masks, pairs, device=None):
    """IoU of P (detection, ground truth) mask pairs -> (P,) float64 on the device.  det_masks (Nd,H,W), gt_masks (Ng,H,W) bool or
    uint8 (non-zero = set), pairs (P,2) rows into them.  inter = popcount(d & g), union = |d| + |g| - inter, integers;
    iou = double(inter) / double(union), 0 for an empty union.  Kernels on device tensors (``ops.mask_pack``, ``ops.mask_pair_inter``),
    the dense torch statement (``_mask_counts_library``) on CPU tensors or when ``policy.disable_fused`` names a kernel.  Either side
    may be a ``handoff.RleMasks``: its run lists are packed by ``ops.rle_to_packed`` without a dense mask; same counts."""
    return _iou_from_counts(*_mask_counts(det_masks, gt_masks, pairs, device))


def _box_ious_library(db, gb, pairs):
    """The library statement of the box IoU: float64 tensor operations, one rounding each."""
    d, g = db[pairs[:, 0].long()], gb[pairs[:, 1].long()]
    w = torch.minimum(d[:, 0] + d[:, 2], g[:, 0] + g[:, 2]) - torch.maximum(d[:, 0], g[:, 0])
    h = torch.minimum(d[:, 1] + d[:, 3], g[:, 1] + g[:, 3]) - torch.maximum(d[:, 1], g[:, 1])
    ok = (w > 0) & (h > 0)
    i = w * h
    da, ga = d[:, 2] * d[:, 3], g[:, 2] * g[:, 3]
    u = (da + ga) - i
    return torch.where(ok, i / torch.where(ok, u, torch.ones_like(u)), torch.zeros_like(i))


@torch.no_grad()
def box_ious(det_boxes, gt_boxes, pairs, device=None):
    """IoU of P box pairs -> (P,) float64.  Boxes (n,4) = x y w h, float64 (other types are converted):
    w = min(dx + dw, gx + gw) - max(dx, gx), h likewise; 0 when w <= 0 or h <= 0; else i = w h, u = (dw dh + gw gh) - i, i / u, no
    fused multiply-add.  ``ops.box_pair_iou`` on device tensors, ``_box_ious_library`` otherwise."""
    dev = _coco_device(device, det_boxes, gt_boxes)
    db = torch.as_tensor(det_boxes).detach().to(device=dev, dtype=torch.float64).reshape(-1, 4).contiguous()
    gb = torch.as_tensor(gt_boxes).detach().to(device=dev, dtype=torch.float64).reshape(-1, 4).contiguous()
    p = _pairs_i32(pairs, dev, db.shape[0], gb.shape[0])
    if p.shape[0] == 0:
        return torch.zeros(0, dtype=torch.float64, device=dev)
    if _coco_kernels("eval.box_ious", db, "box_pair_iou"):
        return ops.box_pair_iou(db, gb, p)
    return _box_ious_library(db, gb, p)


def _coco_match_library(ious, iou_off, groups, det_area, gt_area, gt_ignore, thresholds, area_ranges, rows=None, cells=1 << 24):
    """The library statement of the matching: the groups side by side, padded to the largest, one step per detection rank.
    rows: the groups to match (default all); the detections of the others stay at -1 / 0."""
    dev = ious.device
    NT, NA = thresholds.shape[0], area_ranges.shape[0]
    match = torch.full((det_area.shape[0], NT, NA), -1, dtype=torch.int32, device=dev)
    ignore = torch.zeros(det_area.shape[0], NT, NA, dtype=torch.uint8, device=dev)
    grp = groups.long() if rows is None else groups.long()[rows]
    off = iou_off if rows is None else iou_off[rows]
    if grp.shape[0] == 0:
        return match, ignore
    bar0 = torch.minimum(thresholds, torch.full_like(thresholds, 1.0 - 1e-10))[None, :, None, None]
    lo, hi = area_ranges[:, 0], area_ranges[:, 1]
    Dm, Gm = int(grp[:, 1].max()), max(1, int(grp[:, 3].max()))              # (a padded column, never open, when no group has a ground truth)
    step = max(1, cells // max(1, NT * NA * max(Gm, 1)))
    for s in range(0, grp.shape[0], step):
        g4, o = grp[s:s + step], off[s:s + step]
        n = g4.shape[0]
        gi = torch.arange(Gm, device=dev)[None]
        gok = gi < g4[:, 3, None]                                                                  # (n,Gm)
        gsel = (g4[:, 2, None] + gi).clamp(max=max(gt_area.shape[0] - 1, 0))
        if gt_area.shape[0]:
            ga, gf = gt_area[gsel], gt_ignore[gsel] != 0
        else:
            ga, gf = torch.zeros(n, Gm, dtype=torch.float64, device=dev), torch.zeros(n, Gm, dtype=torch.bool, device=dev)
        ign = gf[:, None] | (ga[:, None] < lo[None, :, None]) | (ga[:, None] > hi[None, :, None])   # (n,NA,Gm)
        ign = ign[:, None].expand(n, NT, NA, Gm)
        taken = (~gok)[:, None, None].expand(n, NT, NA, Gm).clone()
        for d in range(Dm):
            live = d < g4[:, 1]                                                                    # (n,)
            isel = (o[:, None] + d * g4[:, 3, None] + gi).clamp(min=0, max=max(ious.shape[0] - 1, 0))
            v = ious[isel] if ious.shape[0] else torch.zeros(n, Gm, dtype=torch.float64, device=dev)
            v = v[:, None, None].expand(n, NT, NA, Gm)
            cand = ~taken & (v >= bar0) & live[:, None, None, None]
            m = torch.full((n, NT, NA), -1, dtype=torch.long, device=dev)
            for part in (cand & ~ign, cand & ign):
                w = torch.where(part, v, torch.full_like(v, -1.0))
                best = w.max(3, keepdim=True)[0]
                last = torch.where(part & (w == best), gi[0].expand_as(w), torch.full_like(w, -1, dtype=torch.long)).max(3)[0]
                m = torch.where(m >= 0, m, last)                                                   # the ignored part only when nothing matched
            hit = m >= 0
            mc = m.clamp(min=0)
            taken = taken | (hit[..., None] & (gi[0] == mc[..., None]))
            da = det_area[(g4[:, 0] + d).clamp(max=max(det_area.shape[0] - 1, 0))]
            outside = (da[:, None] < lo[None]) | (da[:, None] > hi[None])                           # (n,NA)
            ig = torch.where(hit, torch.gather(ign, 3, mc[..., None])[..., 0], outside[:, None].expand(n, NT, NA))
            r = (g4[:, 0] + d)[live]
            match[r] = m[live].int()
            ignore[r] = ig[live].to(torch.uint8)
    return match, ignore


@torch.no_grad()
def coco_match(ious, iou_off, groups, det_area, gt_area, gt_ignore, thresholds=COCO_THRESHOLDS, area_ranges=COCO_AREA_RANGES, device=None):
    """The greedy matching of every group = (image, category) at every threshold and area range.

    groups (n,4) = first detection, detections D, first ground truth, ground truths G of the group; the group's detections are
    det rows [first, first + D) ALREADY in visiting order (descending score, truncated to 100); iou_off (n,): ious[iou_off + d G + g]
    is the IoU of the group's detection d and ground truth g; det_area (Dn,), gt_area (Gn,) float64; gt_ignore (Gn,).
    -> (match (Dn,NT,NA) int32, the index of the matched ground truth inside its group or -1; ignore (Dn,NT,NA) uint8).
    Per threshold t and range [lo, hi]: a ground truth is ignored when flagged or its area is outside the range; a detection takes
    the unmatched ground truth of highest IoU >= min(t, 1 - 1e-10) among the non-ignored ones (of equal IoUs the later in input
    order), and only when there is none the same among the ignored ones; it is ignored when its match is, or when it has no match
    and its own area is outside the range.  ``ops.coco_match`` (one workgroup per group, 64-bit matched mask) serves groups of at most
    64 ground truths on device tensors; LARGER GROUPS, CPU tensors and ``policy.disable_fused`` go to ``_coco_match_library``, the same
    definition in torch statements."""
    dev = _coco_device(device, ious)
    f64 = lambda a: torch.as_tensor(a).detach().to(device=dev, dtype=torch.float64).contiguous()
    v, da, ga, th, ar = f64(ious).reshape(-1), f64(det_area).reshape(-1), f64(gt_area).reshape(-1), f64(thresholds).reshape(-1), f64(area_ranges).reshape(-1, 2)
    gr = torch.as_tensor(groups).detach().to(device=dev, dtype=torch.int32).reshape(-1, 4).contiguous()
    off = torch.as_tensor(iou_off).detach().to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    gf = (torch.as_tensor(gt_ignore).detach().to(dev) != 0).to(torch.uint8).reshape(-1).contiguous()
    if off.shape[0] != gr.shape[0] or gf.shape[0] != ga.shape[0]:
        raise ValueError(f"coco_match: {gr.shape[0]} groups but {off.shape[0]} offsets; {ga.shape[0]} areas but {gf.shape[0]} ignore flags")
    if gr.shape[0]:
        g = gr.long()
        if bool((g < 0).any() | (off < 0).any() | (g[:, 0] + g[:, 1] > da.shape[0]).any() | (g[:, 2] + g[:, 3] > ga.shape[0]).any() |
                (off + g[:, 1] * g[:, 3] > v.shape[0]).any()):
            raise ValueError("coco_match: a group lies outside the detection, ground-truth or IoU arrays")
    if gr.shape[0] and da.shape[0] and _coco_kernels("eval.coco_match", v, "coco_match"):
        small = gr[:, 3] <= _lib.header_constant("S6D_COCO_MATCH_MAX_GT")
        if bool(small.all()):
            return ops.coco_match(v, off, gr, da, ga, gf, th, ar)
        big = torch.nonzero(~small)[:, 0]
        keep = torch.nonzero(small)[:, 0]
        m, i = ops.coco_match(v, off[keep].contiguous(), gr[keep].contiguous(), da, ga, gf, th, ar)
        ml, il = _coco_match_library(v, off, gr, da, ga, gf, th, ar, rows=big)
        mine = torch.zeros(da.shape[0], dtype=torch.bool, device=dev)
        for r in gr[big].long().tolist():
            mine[r[0]:r[0] + r[1]] = True
        return torch.where(mine[:, None, None], ml, m), torch.where(mine[:, None, None], il, i)
    return _coco_match_library(v, off, gr, da, ga, gf, th, ar)


def detections_from_records(records, masks="dense", device=None):
    """The records of a BOP result file (``handoff.detection_records`` / ``read_bop_json``) -> the ``detections`` of ``coco_scores``:
    im (n,2) = (scene_id, image_id), category, score, bbox (n,4) x y w h float64, masks (when every record has one): with
    ``masks="dense"`` (n,H,W) bool on the host, decoded one record at a time; with ``masks="rle"`` a ``handoff.RleMasks`` on
    ``device`` (default: the host) -- the run lists as they are in the file, one flat array, never a dense mask."""
    from .ism import handoff
    if masks not in ("dense", "rle"):
        raise ValueError(f"masks must be 'dense' or 'rle', got {masks!r}")
    n = len(records)
    out = dict(im=np.array([[int(r["scene_id"]), int(r["image_id"])] for r in records], np.int64).reshape(n, 2),
               category=np.array([int(r["category_id"]) for r in records], np.int64),
               score=np.array([float(r["score"]) for r in records], np.float64),
               bbox=np.array([r["bbox"] for r in records], np.float64).reshape(n, 4))
    if n and all(r.get("segmentation") is not None for r in records):
        for r in records:
            if isinstance(r["segmentation"].get("counts"), (str, bytes)):
                raise ValueError("the segmentation of a record is a COMPRESSED RLE string: only uncompressed run-length lists "
                                 "(what save_json_bop23 writes) are read")
        if masks == "rle":
            out["masks"] = handoff.RleMasks.from_records([r["segmentation"] for r in records], device)
        else:
            out["masks"] = np.stack([handoff.rle_to_mask(r["segmentation"]) for r in records])
    return out


def detections_from_handoff(frames, dataset_name="ycbv"):
    """A batch of ``handoff.Detections`` (one per frame) -> the ``detections`` of ``coco_scores``, the masks staying dense tensors on
    their device (no RLE round trip); categories and boxes as ``handoff.detection_records`` writes them."""
    from .ism import handoff
    frames = [frames] if isinstance(frames, handoff.Detections) else list(frames)
    im, cat, score, box, masks = [], [], [], [], []
    for f in frames:
        obj = f.object_ids.cpu().numpy()
        b = f.boxes.detach().cpu().double().numpy().reshape(-1, 4)
        im.append(np.tile(np.array([[int(f.scene_id), int(f.image_id)]], np.int64), (len(obj), 1)))
        cat.append(handoff.LMO_OBJECT_IDS[obj] if dataset_name == "lmo" else obj + 1)
        score.append(f.scores.detach().cpu().double().numpy())
        box.append(np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1))
        masks.append(f.masks)
    return dict(im=np.concatenate(im), category=np.concatenate(cat).astype(np.int64), score=np.concatenate(score),
                bbox=np.concatenate(box), masks=torch.cat(masks))


def _as_detections(detections):
    from .ism import handoff
    if isinstance(detections, dict):
        return detections
    if isinstance(detections, handoff.Detections) or (len(detections) and isinstance(detections[0], handoff.Detections)):
        return detections_from_handoff(detections)
    return detections_from_records(list(detections))


def _mean(a):
    return float(np.mean(np.ascontiguousarray(a).reshape(-1))) if np.size(a) else -1.0          # one flat sum, in (threshold, recall, category) order


@torch.no_grad()
def coco_scores(detections, ground_truths, iou_type="segm", device=None):
    """COCO AP / AR of detections against ground truths, by the DEFINITION below (``iou_type`` "segm": mask IoU, "bbox": box IoU).

    detections: dict(im, category, score, masks (D,H,W) | bbox (D,4) x y w h) -- the masks may be dense device tensors, or run
    lists (``handoff.RleMasks``, on either side or both: the same result dict as with the dense masks) --, or a
    batch of ``handoff.Detections``, or the records of a result file (``read_bop_json``).  ground_truths: dict(im, category,
    masks (G,H,W) visible masks, bbox (G,4) visible boxes (bbox only), ignore (G,), optionally area (G,) instead of masks for
    bbox).  ``im`` is (n,) or (n,k) integers (k = 2: scene, image); a group is one (im, category).
    -> dict(AP, AP50, AP75, AP_small, AP_medium, AP_large, AR1, AR10, AR100, detections, ground_truths, ignored, groups).

    Definition.  Thresholds T = linspace(0.5, 0.95, 10); area ranges all [0, 1e10], small [0, 32^2], medium [32^2, 96^2], large
    [96^2, 1e10], both ends inclusive; the ground-truth area is the visible mask's pixel count (both IoU types), the detection's its
    mask's pixel count (segm) or w h (bbox).  Per group the detections are stable-sorted by descending score, the first 100 kept and
    matched as ``coco_match`` states, with the IoUs of ``mask_ious`` / ``box_ious``.  Per category, threshold, range and
    maxDet in {1, 10, 100}: each image's first maxDet detections, concatenated over the images in ascending ``im`` order, are
    stable-sorted by descending score and the ignored ones dropped; tp / fp are cumulative; recall = tp / n_pos (n_pos = the
    category's non-ignored ground truths in the range; a category with n_pos = 0 is left out of every mean), precision =
    tp / (tp + fp + eps) with eps = np.spacing(1), made non-increasing from the right and sampled at the recall levels
    linspace(0, 1, 101) with searchsorted(recall, r, side="left"), 0 beyond the last recall.  AP = the mean over thresholds, recall
    levels and categories at (all, 100); AP50, AP75 at one threshold; AP_small / medium / large at 100; AR1 / 10 / 100 = the mean of
    the last recall (0 without detections) at all; a mean over nothing is -1.  There are no crowd instances.
    Grouping, the sorts, the cumulative sums and the sampling are host code in float64; the IoUs and the matching run on
    ``device`` (kernels on a GPU, the library statements on the CPU)."""
    if iou_type not in ("segm", "bbox"):
        raise ValueError(f"iou_type must be 'segm' or 'bbox', got {iou_type!r}")
    det, gt = _as_detections(detections), ground_truths
    d_masks = det.get("masks") if iou_type == "segm" else None
    dev = _coco_device(device, d_masks.counts if _is_rle(d_masks) else d_masks)
    key = lambda x, n: np.asarray(torch.as_tensor(x).cpu() if torch.is_tensor(x) else x, np.int64).reshape(n, -1)
    d_score = np.asarray(torch.as_tensor(det["score"]).cpu() if torch.is_tensor(det["score"]) else det["score"], np.float64).reshape(-1)
    D, G = d_score.shape[0], np.asarray(gt["category"]).reshape(-1).shape[0]
    d_key = np.concatenate([key(det["im"], D), key(det["category"], D)], 1) if D else None
    g_key = np.concatenate([key(gt["im"], G), key(gt["category"], G)], 1) if G else None
    if D and G and d_key.shape[1] != g_key.shape[1]:
        raise ValueError("detections and ground truths name their images differently")
    both = np.concatenate([d_key, g_key]) if D and G else (d_key if D else g_key if G else np.zeros((0, 2), np.int64))
    uniq, inv = np.unique(both, axis=0, return_inverse=True) if both.shape[0] else (both, np.zeros(0, np.int64))
    inv = np.asarray(inv).reshape(-1)
    NG = uniq.shape[0]
    d_grp, g_grp = (inv[:D], inv[D:]) if D and G else ((inv, inv[:0]) if D else (inv[:0], inv))
    g_ign = np.asarray(gt.get("ignore", np.zeros(G, bool))).astype(bool).reshape(-1)
    # visiting order of the detections: by group, then descending score (stable), the first 100 of a group
    order = np.lexsort((-d_score, d_grp)) if D else np.zeros(0, np.int64)
    first = np.searchsorted(d_grp[order], np.arange(NG), side="left")
    rank = np.arange(D) - first[d_grp[order]] if D else np.zeros(0, np.int64)
    kd = order[rank < COCO_MAX_DETS[-1]]
    k_grp, k_rank = d_grp[kd], rank[rank < COCO_MAX_DETS[-1]]
    go = np.argsort(g_grp, kind="stable")
    Dg, Gg = np.bincount(k_grp, minlength=NG).astype(np.int64), np.bincount(g_grp, minlength=NG).astype(np.int64)
    d_off, g_off = np.cumsum(Dg) - Dg, np.cumsum(Gg) - Gg
    i_off = np.cumsum(Dg * Gg) - Dg * Gg
    # every (detection, ground truth) pair of every group, detection-major: the rows of the IoU blocks
    per_det = Gg[k_grp]
    p_det = np.repeat(np.arange(len(kd)), per_det)
    p_gt = g_off[k_grp[p_det]] + (np.arange(len(p_det)) - np.repeat(np.cumsum(per_det) - per_det, per_det))
    pairs = np.stack([kd[p_det], go[p_gt]], 1).astype(np.int32) if len(p_det) else np.zeros((0, 2), np.int32)
    if iou_type == "segm":
        if D and G:
            inter, da, ga, p = _mask_counts(det["masks"], gt["masks"], pairs, dev, site="eval.coco_scores")
            iou = _iou_from_counts(inter, da, ga, p)
            d_area, g_area = da.double(), ga.double()
        else:
            iou = torch.zeros(0, dtype=torch.float64, device=dev)
            d_area = _mask_areas(det["masks"], dev) if D else torch.zeros(0, dtype=torch.float64, device=dev)
            g_area = _mask_areas(gt["masks"], dev) if G else torch.zeros(0, dtype=torch.float64, device=dev)
    else:
        db = torch.as_tensor(det["bbox"]).detach().to(device=dev, dtype=torch.float64).reshape(-1, 4)
        iou = box_ious(db, gt["bbox"], pairs, dev) if D and G else torch.zeros(0, dtype=torch.float64, device=dev)
        d_area = db[:, 2] * db[:, 3]
        if gt.get("area") is not None:
            g_area = torch.as_tensor(gt["area"]).detach().to(device=dev, dtype=torch.float64).reshape(-1)
        else:
            g_area = _mask_areas(gt["masks"], dev) if G else torch.zeros(0, dtype=torch.float64, device=dev)
    idx = lambda a: torch.as_tensor(a, device=dev)
    k_area, s_area = d_area[idx(kd)] if len(kd) else d_area[:0], g_area[idx(go)] if G else g_area[:0]
    s_ign = g_ign[go]
    table = np.stack([d_off, Dg, g_off, Gg], 1).astype(np.int32)
    if len(kd):
        match, dig = coco_match(iou, i_off, table, k_area, s_area, s_ign.astype(np.uint8), COCO_THRESHOLDS, COCO_AREA_RANGES, dev)
        match, dig = match.cpu().numpy() >= 0, dig.cpu().numpy() != 0                               # (Dk,NT,NA)
    else:
        match = dig = np.zeros((0, len(COCO_THRESHOLDS), len(COCO_AREA_RANGES)), bool)
    # accumulation: host code in float64
    ga_h, k_score = s_area.cpu().numpy(), d_score[kd]
    cat_col = uniq.shape[1] - 1
    g_cat, k_cat = (uniq[g_grp[go], cat_col] if G else np.zeros(0, np.int64)), (uniq[k_grp, cat_col] if len(kd) else np.zeros(0, np.int64))
    cats = np.unique(uniq[:, cat_col]) if NG else np.zeros(0, np.int64)
    NT, NA, NM, NR = len(COCO_THRESHOLDS), len(COCO_AREA_RANGES), len(COCO_MAX_DETS), len(COCO_RECALL_LEVELS)
    precision, recall = -np.ones((NT, NR, len(cats), NA, NM)), -np.ones((NT, len(cats), NA, NM))
    eps = np.spacing(1)
    for ki, c in enumerate(cats):
        gsel = g_cat == c
        for ai, (lo, hi) in enumerate(COCO_AREA_RANGES):
            n_pos = int(np.count_nonzero(~(s_ign[gsel] | (ga_h[gsel] < lo) | (ga_h[gsel] > hi))))
            if n_pos == 0:
                continue
            for mi, md in enumerate(COCO_MAX_DETS):
                sel = np.nonzero((k_cat == c) & (k_rank < md))[0]                                   # by image, then by rank
                sel = sel[np.argsort(-k_score[sel], kind="stable")]
                for ti in range(NT):
                    use = ~dig[sel, ti, ai]
                    hit = match[sel, ti, ai][use]
                    tp, fp = np.cumsum(hit).astype(np.float64), np.cumsum(~hit).astype(np.float64)
                    nd = len(tp)
                    rc, pr = tp / n_pos, tp / (fp + tp + eps)
                    recall[ti, ki, ai, mi] = rc[-1] if nd else 0.0
                    pr = np.maximum.accumulate(pr[::-1])[::-1]                                     # non-increasing from the right
                    at = np.searchsorted(rc, COCO_RECALL_LEVELS, side="left")
                    q = np.zeros(NR)
                    q[at < nd] = pr[at[at < nd]]
                    precision[ti, :, ki, ai, mi] = q
    live = recall[0] > -1                                                                          # (K,NA,NM): n_pos > 0
    ap = lambda ts, ai: _mean(precision[ts][:, :, live[:, ai, NM - 1], ai, NM - 1])
    ar = lambda mi: _mean(recall[:, live[:, 0, mi], 0, mi])
    every = slice(None)
    return {"AP": ap(every, 0), "AP50": ap(slice(0, 1), 0), "AP75": ap(slice(5, 6), 0), "AP_small": ap(every, 1), "AP_medium": ap(every, 2),
            "AP_large": ap(every, 3), "AR1": ar(0), "AR10": ar(1), "AR100": ar(2), "iou_type": iou_type, "detections": int(D),
            "ground_truths": int(G), "ignored": int(g_ign.sum()), "groups": int(NG)}


def read_bop_json(path, masks="dense", device=None):
    """The records ``ism.handoff.save_json_bop23`` writes (a JSON list of scene_id, image_id, category_id, bbox x y w h, score, time,
    segmentation = {"counts": run lengths in column-major order, "size": [H, W]}) -> dict(scene, im, category (n,) int64,
    score (n,) float64, bbox (n,4) float64, time (n,) float64, masks (n,H,W) bool or None when the records carry none), the masks
    decoded through ``handoff.rle_to_mask``; with ``masks="rle"`` they stay run lists, a ``handoff.RleMasks`` on ``device``
    (``coco_scores`` takes either).  A ``counts`` that is a compressed RLE STRING is refused: only the uncompressed lists are
    read."""
    import json
    with open(path) as f:
        records = json.load(f)
    if not isinstance(records, list):
        raise ValueError(f"{path}: a JSON list of detection records expected")
    d = detections_from_records(records, masks, device)
    return dict(scene=d["im"][:, 0].copy(), im=d["im"][:, 1].copy(), category=d["category"], score=d["score"], bbox=d["bbox"],
                time=np.array([float(r.get("time", -1.0)) for r in records], np.float64), masks=d.get("masks"))
