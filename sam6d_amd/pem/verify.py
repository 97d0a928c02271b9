"""Pose verification against the measured depth: per-pose evidence and a scene-level selection on the device.

The PEM returns one pose per detection and nothing afterwards judges it: SAM proposals of one physical object at several
granularities become several poses on the same surface, and a pose that floats in front of the measured surface leaves with the
standing of a good one.  ``verify_poses`` renders every instance at its pose (``ops.render_depth``), classifies its pixels against
the measured depth (``ops.verify_evidence``: missing, inlier, occluded, behind) and visits the instances of every frame in order of
their score; a measured pixel supports at most one kept pose (``ops.verify_select``), so duplicates and unsupported poses drop out.
The step is this project's DEFINITION -- stated operation by operation in the header of csrc/s6d_verify.hip, restated independently
in tests/verify_ref.py -- and no equality with another tool's hypothesis verification is claimed.  The defaults (tau 15 model units,
the ``vsd_delta`` of the evaluation; 12 inliers, the refiner's ``min_count``; min_fit and min_fresh 0.5) are choices, not findings.

``_evidence_library`` and ``_select_library`` hold the same definition in torch and plain statements.  They serve CPU tensors and
the kernels ``policy.disable_fused`` names (an error under the strict policy, like every library branch); both are integer work
after two float32 operations per pixel, so they EQUAL the kernels.
"""
import torch

from .. import ops, policy
from .refine import _camera, device_mesh

DEFAULT_TAU = 15.0                                         # model units (mm for BOP meshes): "the same surface", as vsd_delta
DEFAULT_MIN_INLIERS = 12
DEFAULT_MIN_FIT = 0.5
DEFAULT_MIN_FRESH = 0.5
STATUS = {0: "kept", 1: "too few inliers", 2: "seen through", 3: "explained already", 4: "not verifiable"}
COUNTS = ("rendered", "missing", "inlier", "occluded", "behind", "det", "det_rendered", "det_inlier")


def _f32(x):
    return float(torch.tensor(float(x), dtype=torch.float32))          # the ABI's floats


# ------------------------------------------------------------------------------------------------------------ library statements
def _evidence_library(render, depth_obs, obs_index, depth_unit, tau, masks=None):
    """The per-pixel definition of csrc/s6d_verify.hip in torch statements -> the dict of ``ops.verify_evidence``."""
    N, H, W = render.shape
    M, plane, dev = depth_obs.shape[0], H * W, render.device
    words = (plane + 63) // 64
    unit = torch.tensor(float(depth_unit), dtype=torch.float32, device=dev)
    tau = torch.tensor(float(tau), dtype=torch.float32, device=dev)
    oi = obs_index.long()
    live = (oi >= 0) & (oi < M)
    r = render.reshape(N, plane)
    z = depth_obs.reshape(M, plane)[oi.clamp(0, M - 1)] * unit              # one float32 multiply
    z = torch.where(live[:, None], z, torch.zeros_like(z))
    d = z - r                                                               # one float32 subtraction
    rendered = r > 0
    measured = (z > 0) & (z < float("inf"))
    both = rendered & measured
    inl, occ, beh = both & (d.abs() <= tau), both & (d < -tau), both & (d > tau)
    det = masks.reshape(N, plane) != 0 if masks is not None else torch.zeros_like(rendered)
    counts = torch.stack([x.sum(1) for x in (rendered, rendered & ~measured, inl, occ, beh, det, det & rendered, det & inl)], 1).to(torch.int32)
    bits = torch.zeros(N, words * 64, dtype=torch.int64, device=dev)
    bits[:, :plane] = inl
    inlier = (bits.reshape(N, words, 64) << torch.arange(64, device=dev)).sum(-1)          # bit 63 wraps into the sign: the word's bits
    j = torch.arange(words, device=dev)[None]
    nz = inlier != 0
    first = torch.where(nz, j, torch.full_like(j, words)).min(1).values
    last = torch.where(nz, j, torch.full_like(j, -1)).max(1).values
    return dict(counts=counts, inlier=inlier, span=torch.stack([first, last], 1).to(torch.int32))


def _popcount(words):
    return int(((words[:, None] >> torch.arange(64)) & 1).sum())


def _select_library(inlier, counts, span, order, frame_start, flagged, min_inliers, min_fit, min_fresh):
    """The selection of csrc/s6d_verify.hip in plain statements on host copies -> (status (N,) int32, fresh (N,) int32) on the device
    of ``inlier``.  ``span`` is the kernels' shortcut and is not needed here."""
    N, words = inlier.shape
    I, c = inlier.cpu(), counts.cpu().tolist()
    od, fs = order.cpu().tolist(), frame_start.cpu().tolist()
    fl = [0] * N if flagged is None else flagged.cpu().tolist()
    mi, mf, mr = int(min_inliers), _f32(min_fit), _f32(min_fresh)
    status, fresh = [4] * N, [0] * N
    for b in range(len(fs) - 1):
        claimed = torch.zeros(words, dtype=torch.int64)
        for k in range(max(fs[b], 0), min(fs[b + 1], len(od))):
            n = od[k]
            if not 0 <= n < N:
                continue
            rendered, inl, beh = c[n][0], c[n][2], c[n][4]
            fr = _popcount(I[n] & ~claimed)
            if rendered == 0 or fl[n]:
                st = 4
            elif inl < mi:
                st = 1
            elif float(inl) < mf * float(inl + beh):
                st = 2
            elif float(fr) < mr * float(inl):
                st = 3
            else:
                st = 0
                claimed |= I[n]
            status[n], fresh[n] = st, fr
    dev = inlier.device
    return torch.tensor(status, dtype=torch.int32, device=dev), torch.tensor(fresh, dtype=torch.int32, device=dev)


def evidence(render, depth_obs, obs_index, depth_unit, tau, masks=None):
    """``ops.verify_evidence`` on device tensors, ``_evidence_library`` otherwise; no read of the device either way."""
    if policy.guard("pem.verify_evidence", cuda=render.is_cuda, have=ops.have("verify_evidence")):
        return ops.verify_evidence(render, depth_obs, obs_index, depth_unit, tau, masks, check=False)
    return _evidence_library(render, depth_obs, obs_index, depth_unit, tau, masks)


def select(inlier, counts, span, order, frame_start, flagged, min_inliers, min_fit, min_fresh, H=None, W=None):
    if policy.guard("pem.verify_select", cuda=inlier.is_cuda, have=ops.have("verify_select")):
        return ops.verify_select(inlier, counts, span, order, frame_start, flagged, min_inliers, min_fit, min_fresh, H, W, check=False)
    return _select_library(inlier, counts, span, order, frame_start, flagged, min_inliers, min_fit, min_fresh)


def scores(counts, with_masks):
    """counts (N,8) -> (score, fit, sil) float64, one division each: fit = inlier / max(inlier + behind, 1), sil = (det and rendered)
    / max(det + rendered - (det and rendered), 1) -- the intersection over union of the detection's mask and the silhouette -- or 1
    without masks, score = fit sil."""
    c = counts.long()
    fit = c[:, 2].double() / (c[:, 2] + c[:, 4]).clamp(min=1).double()
    sil = c[:, 6].double() / (c[:, 5] + c[:, 0] - c[:, 6]).clamp(min=1).double() if with_masks else torch.ones_like(fit)
    return fit * sil, fit, sil


def visiting_order(frame, n_frames, *keys):
    """The instances frame by frame, inside a frame by DESCENDING keys[0], then keys[1] ..., then ascending index: stable device sorts
    from the last key to the first -> (order (N,) int32, frame_start (n_frames + 1,) int64).  No read of the device."""
    dev = frame.device
    o = torch.arange(frame.shape[0], device=dev)
    for key in reversed(keys):
        o = o[torch.argsort(-key[o], stable=True)]
    o = o[torch.argsort(frame[o], stable=True)]
    per = (frame[:, None] == torch.arange(n_frames, device=dev)[None]).sum(0)
    frame_start = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(per, 0)])
    return o.to(torch.int32).contiguous(), frame_start.contiguous()


def _render(mesh, poses, cam, H, W, znear):
    v, f = mesh["vertices"], mesh["faces"]
    cams = torch.tensor(cam, dtype=torch.float32, device=poses.device).expand(poses.shape[0], 4).contiguous()
    if policy.guard("pem.verify_render", cuda=poses.is_cuda, have=ops.have("render_depth")):
        return ops.render_depth(v, f, poses, cams, H, W, znear, check_faces=False)
    from .. import evaluation
    return evaluation._render_depth_library(v, f, poses, cams, H, W, znear)


# ------------------------------------------------------------------------------------------------------------ the call
@torch.no_grad()
def verify_poses(meshes, object_index, R, t, depth, K, *, masks=None, frame_index=None, order_by=None, tau=DEFAULT_TAU,
                 min_inliers=DEFAULT_MIN_INLIERS, min_fit=DEFAULT_MIN_FIT, min_fresh=DEFAULT_MIN_FRESH, depth_unit=1.0, znear=1.0,
                 render=None):
    """Verify N poses against the measured depth.

    meshes, object_index, R (N,3,3) f32, t (N,3) f32, depth (H,W) or (M,H,W) f32, K, masks (N,H,W) bool / uint8 and frame_index
    (N,) are those of ``refine_poses``: ``device_mesh`` dicts or (vertices, faces) pairs, one camera for the call, frame_index picks
    the depth frame of every instance (default 0) AND defines the frames of the selection.  depth_unit: model units per unit of
    ``depth`` and of ``t``; t is converted by one float32 multiply with float32(depth_unit), the depth inside the evidence kernel.
    masks: the detections' masks; they enter the score (``sil``) and three of the counts, not the classes.

    order_by: (N,) keys -- for example the PEM's score -- visited in descending order inside a frame, ties by ascending index;
    default: descending ``score``, then descending inlier count, then ascending index.  render: dict(depth (N,H,W) f32, skipped (N,)
    int32) made by the caller with ``ops.render_depth`` at these poses, instead of the one call per object made here.

    An instance with a skipped triangle (a vertex nearer than znear) or a pose that is not finite is flagged: status 4.  No host
    synchronisation is issued before the result.  -> dict(keep (N,) bool, status (N,) int32 (``STATUS``), score, fit, sil (N,) f64,
    counts (N,8) int32 (``COUNTS``), fresh (N,) int32, order (N,) int32, frame_start (M+1,) int64)."""
    if R.dim() != 3 or tuple(R.shape[1:]) != (3, 3) or tuple(t.shape) != (R.shape[0], 3):
        raise ValueError(f"verify_poses: R (N,3,3) and t (N,3) expected, got {tuple(R.shape)}, {tuple(t.shape)}")
    if R.dtype != torch.float32 or t.dtype != torch.float32 or depth.dtype != torch.float32:
        raise TypeError(f"verify_poses: R, t and depth must be float32, got {R.dtype}, {t.dtype}, {depth.dtype}")
    N, dev = R.shape[0], R.device
    depth = (depth[None] if depth.dim() == 2 else depth).contiguous()
    if depth.dim() != 3 or depth.device != dev or t.device != dev:
        raise ValueError(f"verify_poses: depth (H,W) or (M,H,W) on the device of R expected, got {tuple(depth.shape)} on {depth.device}")
    M, H, W = depth.shape
    cam = _camera(K)
    oi = [int(o) for o in (object_index.tolist() if hasattr(object_index, "tolist") else object_index)]
    if len(oi) != N or any(not 0 <= o < len(meshes) for o in oi):
        raise ValueError(f"verify_poses: object_index needs {N} values in [0, {len(meshes)}), got {oi}")
    if frame_index is None:
        fi = torch.zeros(N, dtype=torch.int32, device=dev)
    else:
        fl = [int(x) for x in (frame_index.tolist() if hasattr(frame_index, "tolist") else frame_index)]
        if len(fl) != N or any(not 0 <= x < M for x in fl):
            raise ValueError(f"verify_poses: frame_index needs {N} values in [0, {M}), got {fl}")
        fi = torch.tensor(fl, dtype=torch.int32, device=dev)
    if masks is not None:
        if tuple(masks.shape) != (N, H, W) or masks.dtype not in (torch.bool, torch.uint8) or masks.device != dev:
            raise ValueError(f"verify_poses: masks ({N},{H},{W}) bool or uint8 on the device of R expected, got {tuple(masks.shape)} {masks.dtype}")
        masks = masks.to(torch.uint8).contiguous()
    unit = torch.tensor(float(depth_unit), dtype=torch.float32)
    if not 0 < float(unit) < float("inf"):
        raise ValueError(f"verify_poses: depth_unit must be positive and finite, got {depth_unit}")
    if not _f32(tau) >= 0 or int(min_inliers) < 0 or not _f32(min_fit) >= 0 or not _f32(min_fresh) >= 0:
        raise ValueError(f"verify_poses: tau, min_inliers, min_fit and min_fresh must be >= 0, got {tau}, {min_inliers}, {min_fit}, {min_fresh}")
    if order_by is not None:
        order_by = torch.as_tensor(order_by).to(device=dev, dtype=torch.float64)
        if tuple(order_by.shape) != (N,):
            raise ValueError(f"verify_poses: order_by ({N},) expected, got {tuple(order_by.shape)}")
    P = torch.zeros(N, 4, 4, dtype=torch.float32, device=dev)
    P[:, :3, :3], P[:, :3, 3], P[:, 3, 3] = R, t * unit.to(dev), 1.0
    if render is None:
        ren = torch.zeros(N, H, W, dtype=torch.float32, device=dev)
        skipped = torch.zeros(N, dtype=torch.int32, device=dev)
        for o in sorted(set(oi)):
            mesh = meshes[o] if isinstance(meshes[o], dict) else device_mesh(meshes[o][0], meshes[o][1], dev)
            idx = torch.tensor([i for i, x in enumerate(oi) if x == o], dtype=torch.long, device=dev)
            out = _render(mesh, P[idx].contiguous(), cam, H, W, znear)
            ren[idx], skipped[idx] = out["depth"], out["skipped"].to(torch.int32)
    else:
        ren, skipped = render["depth"], render["skipped"]
        if tuple(ren.shape) != (N, H, W) or ren.dtype != torch.float32 or ren.device != dev or tuple(skipped.shape) != (N,):
            raise ValueError(f"verify_poses: render needs depth ({N},{H},{W}) f32 and skipped ({N},) on the device of R, got "
                             f"{tuple(ren.shape)} {ren.dtype}, {tuple(skipped.shape)}")
        ren = ren.contiguous()
    flagged = ((skipped > 0) | ~torch.isfinite(P[:, :3]).flatten(1).all(1)).to(torch.uint8)
    ev = evidence(ren, depth, fi, float(unit), tau, masks)
    score, fit, sil = scores(ev["counts"], masks is not None)
    keys = (order_by,) if order_by is not None else (score, ev["counts"][:, 2].long())
    order, frame_start = visiting_order(fi, M, *keys)
    status, fresh = select(ev["inlier"], ev["counts"], ev["span"], order, frame_start, flagged, min_inliers, min_fit, min_fresh, H, W)
    return dict(keep=status == 0, status=status, score=score, fit=fit, sil=sil, counts=ev["counts"], fresh=fresh, order=order,
                frame_start=frame_start)


class PoseVerifier:
    """The device meshes of a set of objects and the keyword defaults of ``verify_poses``; ``FramePipeline(verifier=...)`` calls it
    once per frame after the PEM (and the refiner).  use_masks: hand every instance its detection's mask (the ``sil`` term)."""

    def __init__(self, meshes, device=None, use_masks=True, **defaults):
        self.meshes = [m if isinstance(m, dict) else device_mesh(m[0], m[1], device) for m in meshes]
        self.use_masks = use_masks
        self.defaults = defaults

    def __call__(self, object_index, R, t, depth, K, **kw):
        return verify_poses(self.meshes, object_index, R, t, depth, K, **{**self.defaults, **kw})
