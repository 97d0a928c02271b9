"""Pose refinement against the measured depth: projective point-to-plane ICP on the device.

SAM-6D stops at the PEM's fine-matching Procrustes; nothing afterwards looks at the depth frame again.  ``refine_poses`` does: per
iteration it renders every instance at its current pose (``ops.render_views``: per pixel the visible face and the model coordinate
of the surface point), forms the point-to-plane normal equations against the measured depth (``ops.refine_normal_eq``), solves them
and moves the pose (``ops.refine_update``).  The step is this project's DEFINITION -- stated operation by operation in the header of
csrc/s6d_refine.hip, restated independently in tests/refine_ref.py -- and nothing claims equality with another tool.

``_normal_eq_library`` and ``_update_library`` hold the same definition in torch float64 statements on any device.  They serve CPU
tensors and the kernels ``policy.disable_fused`` names (an error under the strict policy, like every library branch); their sums are
the kernels' up to the order of the additions.

What refinement cannot do: a direction the visible surface does not constrain stays where the PEM put it (status 2 when nothing
constrains it at all: a box showing two faces will not slide along their common edge), and a symmetric object keeps its ambiguity.
"""
import torch

from .. import ops, policy

DEFAULT_SCHEDULE = (20.0, 20.0, 10.0, 10.0, 5.0, 5.0)      # max_dist per iteration, model units (mm for BOP meshes)
DEFAULT_MIN_COS = 0.1
DEFAULT_DAMPING = 1e-6                                     # relative: added to the unit diagonal of the Jacobi-scaled system
DEFAULT_MIN_PIVOT = 1e-9                                   # of that scaled system (its pivots lie in (0, 1 + damping])
DEFAULT_MIN_COUNT = 12
MAX_ITERATIONS = 32
STATUS = {0: "updated", 1: "too few correspondences", 2: "singular geometry", 3: "not finite / not renderable"}


# ------------------------------------------------------------------------------------------------------------ library statements
def _rows(R, x):
    """(R x) per pixel, rows accumulated left to right: R (T,3,3), x three (T,P) components -> three (T,P)."""
    return [(R[:, i, 0, None] * x[0] + R[:, i, 1, None] * x[1]) + R[:, i, 2, None] * x[2] for i in range(3)]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _normal_eq_library(xyz, face, depth_obs, obs_index, mask, vertices, faces, poses, fx, fy, cx, cy, depth_unit, max_dist, min_cos):
    """The per-pixel definition of csrc/s6d_refine.hip in torch float64 statements -> (sums (T,28) f64, count (T,) int32).  The sums
    are plain ``sum`` reductions: the kernels' up to the order of the additions."""
    f64, f32 = torch.float64, torch.float32
    T, H, W = face.shape
    M, V, F = depth_obs.shape[0], vertices.shape[0], faces.shape[0]
    c = lambda s: float(torch.tensor(float(s), dtype=f32))                                        # noqa: E731  (the ABI's floats)
    fx, fy, cx, cy, unit, md, mc = (c(s) for s in (fx, fy, cx, cy, depth_unit, max_dist, min_cos))
    oi = obs_index.long()
    live = (oi >= 0) & (oi < M)
    Zo = depth_obs[oi.clamp(0, M - 1)].reshape(T, -1).to(f64) * unit
    f = face.reshape(T, -1).long()
    ok = live[:, None] & (f >= 0) & (f < F) & (Zo > 0)
    if mask is not None:
        ok &= mask.reshape(T, -1) != 0
    tri = faces.long()[f.clamp(0, F - 1)]                                                         # (T,P,3)
    ok &= ((tri >= 0) & (tri < V)).all(-1)
    vv = vertices.to(f64)[tri.clamp(0, V - 1)]                                                    # (T,P,3,3)
    u = torch.arange(W, device=face.device, dtype=f64).repeat(H)[None]
    v = torch.arange(H, device=face.device, dtype=f64).repeat_interleave(W)[None]
    q = [((u - cx) / fx) * Zo, ((v - cy) / fy) * Zo, Zo]
    R, tr = poses[:, :3, :3].to(f64), poses[:, :3, 3].to(f64)
    x = xyz.reshape(T, -1, 3).to(f64).unbind(-1)
    p = [r + tr[:, i, None] for i, r in enumerate(_rows(R, x))]
    a, b = (vv[:, :, 1] - vv[:, :, 0]).unbind(-1), (vv[:, :, 2] - vv[:, :, 0]).unbind(-1)
    m = _cross(a, b)
    mm = _dot(m, m)
    ok &= ~(mm == 0)
    sm = torch.sqrt(mm)
    n = _rows(R, [k / sm for k in m])
    npd = _dot(n, p)
    flip = npd > 0
    n = [torch.where(flip, -k, k) for k in n]
    npd = torch.where(flip, -npd, npd)
    ok &= npd * npd >= (mc * mc) * _dot(p, p)
    d = [q[i] - p[i] for i in range(3)]
    ok &= _dot(d, d) <= md * md
    r = _dot(n, d)
    J = _cross(p, n) + n
    terms = [J[i] * J[j] for i in range(6) for j in range(i, 6)] + [J[i] * r for i in range(6)] + [r * r]
    zero = torch.zeros((), dtype=f64, device=face.device)
    sums = torch.stack([torch.where(ok, k, zero).sum(1) for k in terms], 1)
    return sums, ok.sum(1).to(torch.int32)


def _update_library(sums, count, poses, min_count, damping, min_pivot):
    """The solve and the Cayley update of csrc/s6d_refine.hip in torch float64 statements, the T systems side by side ->
    (poses_out (T,4,4) f32, status (T,) int32, rms (T,) f64)."""
    f64, f32 = torch.float64, torch.float32
    c = lambda s: float(torch.tensor(float(s), dtype=f32))                                        # noqa: E731
    lam, min_pivot = c(damping), c(min_pivot)
    S, P, n = sums.to(f64), poses.to(f32), count.long()
    T = P.shape[0]
    finite = torch.isfinite(S).all(1)
    zero, one = torch.zeros(T, dtype=f64, device=S.device), torch.ones(T, dtype=f64, device=S.device)
    rms = torch.where(finite & (n > 0), torch.sqrt(S[:, 27] / n.clamp(min=1).to(f64)), zero)
    finite = finite & torch.isfinite(P[:, :3]).flatten(1).all(1)
    status = torch.where(~finite, 3, torch.where(n < int(min_count), 1, 0))
    S = torch.where(finite[:, None], S, torch.zeros_like(S))
    A, k = [[None] * 6 for _ in range(6)], 0
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = S[:, k]
            k += 1
    d = [torch.sqrt(A[i][i]) for i in range(6)]
    safe = lambda num, den: torch.where(den == 0, zero, num / torch.where(den == 0, one, den))   # noqa: E731
    cvec = [safe(S[:, 21 + i], d[i]) for i in range(6)]
    Mx = [[one + lam if i == j else safe(A[i][j], d[i] * d[j]) for j in range(6)] for i in range(6)]
    L = [[None] * 6 for _ in range(6)]
    singular = torch.zeros(T, dtype=torch.bool, device=S.device)
    for j in range(6):
        s = Mx[j][j]
        for q in range(j):
            s = s - L[j][q] * L[j][q]
        singular |= ~(s >= min_pivot)
        L[j][j] = torch.sqrt(s)
        for i in range(j + 1, 6):
            s = Mx[i][j]
            for q in range(j):
                s = s - L[i][q] * L[j][q]
            L[i][j] = s / L[j][j]
    z, y = [None] * 6, [None] * 6
    for i in range(6):
        s = cvec[i]
        for q in range(i):
            s = s - L[i][q] * z[q]
        z[i] = s / L[i][i]
    for i in range(5, -1, -1):
        s = z[i]
        for q in range(i + 1, 6):
            s = s - L[q][i] * y[q]
        y[i] = s / L[i][i]
    xi = [safe(y[i], d[i]) for i in range(6)]
    h0, h1, h2 = xi[0] * 0.5, xi[1] * 0.5, xi[2] * 0.5
    hh = (h0 * h0 + h1 * h1) + h2 * h2
    e, g = 1.0 + hh, 1.0 - hh
    xy, xz, yz, x2, y2, z2 = 2.0 * (h0 * h1), 2.0 * (h0 * h2), 2.0 * (h1 * h2), 2.0 * h0, 2.0 * h1, 2.0 * h2
    dR = [[(g + 2.0 * (h0 * h0)) / e, (xy - z2) / e, (xz + y2) / e],
          [(xy + z2) / e, (g + 2.0 * (h1 * h1)) / e, (yz - x2) / e],
          [(xz - y2) / e, (yz + x2) / e, (g + 2.0 * (h2 * h2)) / e]]
    Pd = P.to(f64)
    new = P.clone()
    for i in range(3):
        for j in range(3):
            new[:, i, j] = ((dR[i][0] * Pd[:, 0, j] + dR[i][1] * Pd[:, 1, j]) + dR[i][2] * Pd[:, 2, j]).to(f32)
        new[:, i, 3] = (((dR[i][0] * Pd[:, 0, 3] + dR[i][1] * Pd[:, 1, 3]) + dR[i][2] * Pd[:, 2, 3]) + xi[3 + i]).to(f32)
    status = torch.where((status == 0) & singular, 2, status)
    status = torch.where((status == 0) & ~torch.isfinite(new[:, :3]).flatten(1).all(1), 3, status)
    out = torch.where((status == 0)[:, None, None], new, P)
    return out, status.to(torch.int32), rms


def normal_eq(xyz, face, depth_obs, obs_index, mask, vertices, faces, poses, fx, fy, cx, cy, depth_unit, max_dist, min_cos):
    """``ops.refine_normal_eq`` on device tensors, ``_normal_eq_library`` otherwise; no read of the device either way (an obs_index
    outside [0, M) leaves its instance at zeros)."""
    if policy.guard("refine.normal_eq", cuda=xyz.is_cuda, have=ops.have("refine_normal_eq")):
        return ops.refine_normal_eq(xyz, face, depth_obs, obs_index, mask, vertices, faces, poses, fx, fy, cx, cy, depth_unit, max_dist,
                                    min_cos, check_index=False)
    return _normal_eq_library(xyz, face, depth_obs, obs_index, mask, vertices, faces, poses, fx, fy, cx, cy, depth_unit, max_dist, min_cos)


def update(sums, count, poses, min_count, damping, min_pivot):
    if policy.guard("refine.update", cuda=sums.is_cuda, have=ops.have("refine_update")):
        return ops.refine_update(sums, count, poses, min_count, damping, min_pivot)
    return _update_library(sums, count, poses, min_count, damping, min_pivot)


# ------------------------------------------------------------------------------------------------------------ the loop
def device_mesh(vertices, faces, device=None):
    """vertices (V,3), faces (F,3) (arrays or tensors) -> dict(vertices f32, faces int32, colors uint8 grey) on the device, the face
    indices checked once here so that the loop need not read the device for it."""
    v = torch.as_tensor(vertices).to(device=device, dtype=torch.float32).contiguous()
    f = torch.as_tensor(faces).to(device=device, dtype=torch.int32).contiguous()
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3 or not len(v) or not len(f):
        raise ValueError(f"device_mesh: vertices (V,3) and faces (F,3) expected, got {tuple(v.shape)}, {tuple(f.shape)}")
    if int(f.min()) < 0 or int(f.max()) >= len(v):
        raise ValueError(f"device_mesh: face indices must lie in [0, {len(v)}), got [{int(f.min())}, {int(f.max())}]")
    return dict(vertices=v, faces=f, colors=torch.full((len(v), 3), 128, dtype=torch.uint8, device=v.device))


def _camera(K):
    k = K.detach().cpu().double() if torch.is_tensor(K) else torch.as_tensor(K, dtype=torch.float64)
    if tuple(k.shape) == (3, 3):
        return float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])
    if tuple(k.shape) == (4,):
        return tuple(float(x) for x in k)
    raise ValueError(f"refine_poses: K must be a (3,3) matrix or (fx, fy, cx, cy), got shape {tuple(k.shape)}")


@torch.no_grad()
def refine_poses(meshes, object_index, R, t, depth, K, *, masks=None, frame_index=None, max_dist=DEFAULT_SCHEDULE,
                 min_cos=DEFAULT_MIN_COS, damping=DEFAULT_DAMPING, min_pivot=DEFAULT_MIN_PIVOT, min_count=DEFAULT_MIN_COUNT,
                 depth_unit=1.0, znear=1.0):
    """Refine N poses against the measured depth.

    meshes: a sequence of ``device_mesh`` dicts (or (vertices, faces) pairs, checked and uploaded here); object_index: N indices into
    it (a sequence, or a tensor that is read once before the loop); R (N,3,3) f32, t (N,3) f32 object -> camera; depth (H,W) or
    (M,H,W) f32; K a (3,3) matrix or (fx, fy, cx, cy), one camera for the call; masks (N,H,W) bool / uint8 restricts every instance
    to its own pixels; frame_index (N,) picks the depth frame of every instance (default 0).

    max_dist is the SCHEDULE: one truncation distance (model units) per iteration, its length the iteration count (<= 32).
    depth_unit: model units per unit of ``depth`` AND of ``t`` (1000 for metres against millimetre meshes): t is converted on the
    way in by one float32 multiply with float32(depth_unit) and on the way out by one with float32(1 / depth_unit); an instance
    that never moved gets its own ``t`` back bit for bit.

    Per iteration and object: ONE ``ops.render_views`` over that object's instances, the normal equations, the update.  The loop
    issues no host synchronisation; the caller reads the flags once at the end.  -> dict(R (N,3,3) f32, t (N,3) f32,
    status (N,) int32, rms (N,) f64 model units, count (N,) int32, skipped (N,) int32):
      status 0  every iteration updated the pose; rms / count are those of the last iteration's linearisation point;
      1, 2, 3   too few correspondences / singular geometry / not finite (``STATUS``) in some iteration: the instance is FROZEN at
                the pose it entered that iteration with, for the remaining iterations; rms / count are that iteration's;
      skipped   the rasteriser's count of triangles it could not draw (a vertex nearer than znear), summed over the iterations on
                the device; an instance with a skipped triangle gets status 3 under the same freezing rule."""
    schedule = [float(x) for x in (max_dist if hasattr(max_dist, "__len__") else [max_dist])]
    if not 1 <= len(schedule) <= MAX_ITERATIONS:
        raise ValueError(f"refine_poses: max_dist is the schedule, 1 to {MAX_ITERATIONS} values, got {len(schedule)}")
    if R.dim() != 3 or tuple(R.shape[1:]) != (3, 3) or tuple(t.shape) != (R.shape[0], 3):
        raise ValueError(f"refine_poses: R (N,3,3) and t (N,3) expected, got {tuple(R.shape)}, {tuple(t.shape)}")
    if R.dtype != torch.float32 or t.dtype != torch.float32 or depth.dtype != torch.float32:
        raise TypeError(f"refine_poses: R, t and depth must be float32, got {R.dtype}, {t.dtype}, {depth.dtype}")
    N, dev = R.shape[0], R.device
    depth = (depth[None] if depth.dim() == 2 else depth).contiguous()
    if depth.dim() != 3 or depth.device != dev or t.device != dev:
        raise ValueError(f"refine_poses: depth (H,W) or (M,H,W) on the device of R expected, got {tuple(depth.shape)} on {depth.device}")
    M, H, W = depth.shape
    fx, fy, cx, cy = _camera(K)
    oi = [int(o) for o in (object_index.tolist() if hasattr(object_index, "tolist") else object_index)]
    if len(oi) != N or any(not 0 <= o < len(meshes) for o in oi):
        raise ValueError(f"refine_poses: object_index needs {N} values in [0, {len(meshes)}), got {oi}")
    if frame_index is None:
        fi = torch.zeros(N, dtype=torch.int32, device=dev)
    else:
        fl = [int(x) for x in (frame_index.tolist() if hasattr(frame_index, "tolist") else frame_index)]
        if len(fl) != N or any(not 0 <= x < M for x in fl):
            raise ValueError(f"refine_poses: frame_index needs {N} values in [0, {M}), got {fl}")
        fi = torch.tensor(fl, dtype=torch.int32, device=dev)
    if masks is not None:
        if tuple(masks.shape) != (N, H, W) or masks.dtype not in (torch.bool, torch.uint8) or masks.device != dev:
            raise ValueError(f"refine_poses: masks ({N},{H},{W}) bool or uint8 on the device of R expected, got {tuple(masks.shape)} {masks.dtype}")
        masks = masks.to(torch.uint8).contiguous()
    unit = torch.tensor(float(depth_unit), dtype=torch.float32)
    if not float(unit) > 0:
        raise ValueError(f"refine_poses: depth_unit must be positive, got {depth_unit}")
    P = torch.zeros(N, 4, 4, dtype=torch.float32, device=dev)
    P[:, :3, :3], P[:, :3, 3], P[:, 3, 3] = R, t * unit.to(dev), 1.0
    status = torch.zeros(N, dtype=torch.int32, device=dev)
    count, skipped = torch.zeros_like(status), torch.zeros_like(status)
    rms = torch.zeros(N, dtype=torch.float64, device=dev)
    moved = torch.zeros(N, dtype=torch.bool, device=dev)
    groups = []
    for o in sorted(set(oi)):
        mesh = meshes[o] if isinstance(meshes[o], dict) else device_mesh(meshes[o][0], meshes[o][1], dev)
        idx = torch.tensor([i for i, x in enumerate(oi) if x == o], dtype=torch.long, device=dev)
        groups.append((mesh, idx, fi[idx].contiguous(), None if masks is None else masks[idx].contiguous()))
    three = torch.full((), 3, dtype=torch.int32, device=dev)
    for md in schedule:
        for mesh, idx, gfi, gmask in groups:
            v, f = mesh["vertices"], mesh["faces"]
            Pg = P[idx].contiguous()
            ren = ops.render_views(v, f, mesh["colors"], Pg, fx, fy, cx, cy, H, W, 1.0, 0.0, znear, check_faces=False)
            sums, cnt = normal_eq(ren["xyz"], ren["face"], depth, gfi, gmask, v, f, Pg, fx, fy, cx, cy, float(unit), md, min_cos)
            Pn, st, r = update(sums, cnt, Pg, min_count, damping, min_pivot)
            st = torch.where(ren["skipped"] > 0, three, st)
            old = status[idx]
            go = (old == 0) & (st == 0)
            P[idx] = torch.where(go[:, None, None], Pn, Pg)
            fresh = old == 0                                                    # not frozen before this iteration
            status[idx] = torch.where(fresh, st, old)
            rms[idx] = torch.where(fresh, r, rms[idx])
            count[idx] = torch.where(fresh, cnt, count[idx])
            skipped[idx] = skipped[idx] + ren["skipped"]
            moved[idx] = moved[idx] | go
    inv = (1.0 / unit).to(torch.float32).to(dev)
    t_out = torch.where(moved[:, None], P[:, :3, 3] * inv, t)
    return dict(R=P[:, :3, :3].contiguous(), t=t_out.contiguous(), status=status, rms=rms, count=count, skipped=skipped)


class DepthRefiner:
    """The device meshes of a set of objects and the keyword defaults of ``refine_poses``; ``FramePipeline(refiner=...)`` calls it
    once per frame after the PEM.  use_masks: restrict every instance to its detection's mask."""

    def __init__(self, meshes, device=None, use_masks=True, **defaults):
        self.meshes = [m if isinstance(m, dict) else device_mesh(m[0], m[1], device) for m in meshes]
        self.use_masks = use_masks
        self.defaults = defaults

    def __call__(self, object_index, R, t, depth, K, **kw):
        return refine_poses(self.meshes, object_index, R, t, depth, K, **{**self.defaults, **kw})
