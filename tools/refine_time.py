"""Times of the depth refinement (sam6d_amd/pem/refine.py) on one MI355X, for profiles/refine.md:

python tools/refine_time.py [--out FILE.json] [--no-pipeline]

One iteration (render, normal equations, update; each stage alone and the three together) and the default schedule of
``refine_poses``, for 1 and for 10 instances at 640 x 480, on the 576-face torus of the tests and on a torus of 100352 faces; and,
unless --no-pipeline, the ``pem`` and ``pem_refine`` stage times of ``FramePipeline.times`` of one run with a refiner (the synthetic
frame and seeded models of tools/frame_demo.py: the poses are meaningless and most instances freeze, but a frozen instance is still
rendered in every iteration -- the loop never asks the host -- so the stage is the whole schedule over fewer object pixels).  Device events around enough repetitions to fill a tenth
of a second, after a warm-up; the depth frame is the render at the true pose, the start 4 degrees and (3, -2, 6) off."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sam6d_amd import ops  # noqa: E402
from sam6d_amd.pem import refine  # noqa: E402

H, W, K = 480, 640, (572.4, 573.6, 325.3, 242.0)


def torus(n_major, n_minor, R=60.0, r=25.0):
    a, b = np.arange(n_major) * (2 * np.pi / n_major), np.arange(n_minor) * (2 * np.pi / n_minor)
    A, B = np.meshgrid(a, b, indexing="ij")
    v = np.stack([(R + r * np.cos(B)) * np.cos(A), (R + r * np.cos(B)) * np.sin(A), r * np.sin(B)], -1).reshape(-1, 3)
    idx = lambda i, j: (i % n_major) * n_minor + (j % n_minor)          # noqa: E731
    f = [t for i in range(n_major) for j in range(n_minor)
         for t in ([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)])]
    return v.astype(np.float32), np.array(f, np.int32)


def poses(n, seed):
    rs = np.random.RandomState(seed)
    P = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        q, r = np.linalg.qr(rs.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        P[k, :3, :3], P[k, :3, 3] = q, (3.0 + 40.0 * (k % 5 - 2), -2.0 + 60.0 * (k // 5) - 30.0, 400.0)
    return P


def off(P):
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(4.0)
    S = P.copy()
    S[:, :3, :3] = (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx) @ P[:, :3, :3]
    S[:, :3, 3] += (3.0, -2.0, 6.0)
    return S


def timed(fn, budget_s=0.1):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    reps = max(3, int(budget_s * 1e3 / max(a.elapsed_time(b), 1e-3)))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def measure(mesh_name, v, f, T, dev):
    mesh = refine.device_mesh(v, f, dev)
    true = poses(T, 5)
    tr = torch.from_numpy(true.astype(np.float32)).to(dev)
    ren = ops.render_views(mesh["vertices"], mesh["faces"], mesh["colors"], tr, *K, H, W, 1.0, 0.0, 1.0)
    depth = ren["depth"]                                               # a frame per instance: no neighbour occludes
    start = torch.from_numpy(off(true).astype(np.float32)).to(dev)
    fi = torch.arange(T, dtype=torch.int32, device=dev)
    r0 = ops.render_views(mesh["vertices"], mesh["faces"], mesh["colors"], start, *K, H, W, 1.0, 0.0, 1.0)
    s0, c0 = ops.refine_normal_eq(r0["xyz"], r0["face"], depth, fi, None, mesh["vertices"], mesh["faces"], start, *K, 1.0, 20.0, 0.1)

    def render():
        return ops.render_views(mesh["vertices"], mesh["faces"], mesh["colors"], start, *K, H, W, 1.0, 0.0, 1.0, check_faces=False)

    def neq():
        return ops.refine_normal_eq(r0["xyz"], r0["face"], depth, fi, None, mesh["vertices"], mesh["faces"], start, *K, 1.0, 20.0, 0.1,
                                    check_index=False)

    def upd():
        return ops.refine_update(s0, c0, start, refine.DEFAULT_MIN_COUNT, refine.DEFAULT_DAMPING, refine.DEFAULT_MIN_PIVOT)

    def loop(schedule):
        return refine.refine_poses([mesh], [0] * T, start[:, :3, :3].contiguous(), start[:, :3, 3].contiguous(), depth, K,
                                   frame_index=list(range(T)), max_dist=schedule)
    out = loop(refine.DEFAULT_SCHEDULE)
    end = np.tile(np.eye(4), (T, 1, 1))
    end[:, :3, :3], end[:, :3, 3] = out["R"].cpu().numpy(), out["t"].cpu().numpy()
    vv = v.astype(np.float64)
    mssd = lambda P: [float(np.linalg.norm((vv @ P[k, :3, :3].T + P[k, :3, 3]) - (vv @ true[k, :3, :3].T + true[k, :3, 3]), axis=1).max())  # noqa: E731
                      for k in range(T)]
    # a torus is symmetric about its z axis and the finer it is tessellated, the less its facets say about that angle: the end error
    # is also given as the minimum over rotations of the model about that axis (0.1 degree steps, every 7th vertex)
    sub, ang = vv[::7], np.deg2rad(np.arange(0.0, 360.0, 0.1))

    def mssd_sym(P):
        best = []
        for k in range(T):
            want = sub @ true[k, :3, :3].T + true[k, :3, 3]
            m = np.inf
            for a0 in ang:
                c, s_ = np.cos(a0), np.sin(a0)
                rot = sub @ np.array([[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]]).T
                m = min(m, float(np.linalg.norm((rot @ P[k, :3, :3].T + P[k, :3, 3]) - want, axis=1).max()))
            best.append(round(m, 4))
        return best
    return dict(mesh=mesh_name, faces=int(len(f)), T=T, rms_end=[round(x, 5) for x in out["rms"].cpu().tolist()], mssd_end_sym=mssd_sym(end), correspondences=c0.cpu().tolist(), render_ms=timed(render), normal_eq_ms=timed(neq),
                update_ms=timed(upd), one_iteration_ms=timed(lambda: loop((20.0,))), schedule_ms=timed(lambda: loop(refine.DEFAULT_SCHEDULE)),
                status=out["status"].cpu().tolist(), mssd_start=[round(x, 3) for x in mssd(off(true))], mssd_end=[round(x, 4) for x in mssd(end)])


def pipeline_stage(dev):
    """``pem`` and ``pem_refine`` of FramePipeline.times on the synthetic frame of tools/frame_demo.py with a refiner on the torus."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import frame_demo
    pipe, args = frame_demo.build(dev)
    v, f = torus(24, 12)
    pipe.refiner = refine.DepthRefiner([(v, f)], device=dev, depth_unit=1000.0)
    for _ in range(3):
        det, poses_ = pipe(*args)
    return dict(instances=int(poses_["pred_R"].shape[0]), refine_status=poses_["refine_status"].cpu().tolist(),
                times_ms={k: round(x, 3) for k, x in pipe.times.items()})


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-pipeline", action="store_true")
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "refine_time.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda")
    rows = []
    for name, (nm, nn) in (("torus 24 x 12", (24, 12)), ("torus 224 x 224", (224, 224))):
        v, f = torus(nm, nn)
        for T in (1, 10):
            rows.append(measure(name, v, f, T, dev))
            print(json.dumps(rows[-1]), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), frame=[H, W], chunk=ops.RF_CHUNK, rows=rows)
    if not a.no_pipeline:
        out["pipeline"] = pipeline_stage(dev)
        print(json.dumps(out["pipeline"]), flush=True)
    if a.out:
        with open(a.out, "w") as g:
            json.dump(out, g, indent=1)
    return out


if __name__ == "__main__":
    main()
