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

Every error function goes through ``policy.guard("eval.<name>", ...)``: kernels on device tensors, the torch statements below
otherwise (policy field ``bop_eval`` = "0", or CPU tensors).  The torch branch is chunked over the symmetries, so it does not
hold the (N, S, V, 3) tensor either.
"""
import math

import numpy as np
import torch

from . import ops, policy

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
