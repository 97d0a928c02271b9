"""Times of the pose verification (sam6d_amd/pem/verify.py, csrc/s6d_verify.hip) on one MI355X, for profiles/verify.md:

python tools/verify_time.py [--out FILE.json]

Two cases at 640 x 480 on the 576-face torus of the tests: 32 instances in one frame, and 8 x 32 in eight frames (every fourth
instance a true pose, the others shifted duplicates and poses off the surface; the depth frame is the nearest true render in front
of a wall, 5 % missing).  Per case: the evidence kernel (with and without masks; microseconds and GB/s of the bytes the definition
needs: 8 or 9 per pixel and instance read -- the depth rows counted once per instance, as the kernel asks for them -- and one bit
written), the selection kernel with the claimed bitmap in LDS and in the workspace, the whole ``verify_poses`` call and the
``render_depth`` calls inside it, and the library branch of the same call (``policy.disable_fused``) for the ratio.  Device events
around enough repetitions to fill a fifth of a second, after a warm-up.  The inputs of a case (39 MB and 315 MB of renders) are
re-read by every repetition: the smaller case fits the Infinity Cache, so its rate is not an HBM rate."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refine_time import poses, torus  # noqa: E402
from sam6d_amd import ops, policy  # noqa: E402
from sam6d_amd.pem import refine, verify  # noqa: E402

H, W, K = 480, 640, (572.4, 573.6, 325.3, 242.0)


def timed(fn, budget_s=0.2):
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


def case(frames, per_frame, dev):
    v, f = torus(24, 12)
    mesh = refine.device_mesh(v, f, dev)
    N = frames * per_frame
    P = np.concatenate([poses(per_frame, 5 + b) for b in range(frames)])
    k = np.arange(N) % per_frame
    P[:, 0, 3], P[:, 1, 3] = -140.0 + 40.0 * (k % 8), -90.0 + 60.0 * (k // 8 % 4)      # a grid that stays inside the frame
    true = np.arange(N) % 4 == 0
    rs = np.random.RandomState(2)
    P[~true, :3, 3] += rs.uniform(-12, 12, (int((~true).sum()), 3))
    P[np.arange(N) % 4 == 3, 2, 3] -= 120.0                                 # every fourth floats in front of the surface
    frame = np.repeat(np.arange(frames), per_frame).astype(np.int32)
    Pt = torch.from_numpy(P.astype(np.float32)).to(dev)
    cams = torch.tensor(K, dtype=torch.float32, device=dev).expand(N, 4).contiguous()
    ren = ops.render_depth(mesh["vertices"], mesh["faces"], Pt, cams, H, W, 1.0)["depth"]
    fi = torch.from_numpy(frame).to(dev)
    depth = torch.full((frames, H, W), 700.0, device=dev)
    for b in range(frames):
        r = ren[torch.from_numpy(true & (frame == b)).to(dev)]
        z = torch.where(r > 0, r, torch.full_like(r, float("inf"))).min(0).values
        depth[b] = torch.where(torch.isfinite(z), z, depth[b])
    depth[torch.rand(depth.shape, device=dev, generator=torch.Generator(dev).manual_seed(1)) < 0.05] = 0.0
    masks = (ren > 0).to(torch.uint8)
    R, t = Pt[:, :3, :3].contiguous(), Pt[:, :3, 3].contiguous()
    ev = ops.verify_evidence(ren, depth, fi, 1.0, verify.DEFAULT_TAU, masks)
    score = verify.scores(ev["counts"], True)[0]
    order, start = verify.visiting_order(fi, frames, score, ev["counts"][:, 2].long())
    th = (verify.DEFAULT_MIN_INLIERS, verify.DEFAULT_MIN_FIT, verify.DEFAULT_MIN_FRESH)

    def sel():
        return ops.verify_select(ev["inlier"], ev["counts"], ev["span"], order, start, None, *th, H, W, check=False)

    def whole(**kw):
        return verify.verify_poses([mesh], [0] * N, R, t, depth, K, masks=masks, frame_index=frame, **kw)
    out = whole()
    row = dict(frames=frames, instances=N, status={verify.STATUS[s]: int((out["status"] == s).sum()) for s in verify.STATUS},
               kept_are_true=bool((out["keep"].cpu().numpy() <= true).all()), span_words=ev["span"].cpu().tolist()[:4])
    px = N * H * W
    for name, m, nbytes in (("evidence", None, 8 * px + px // 8), ("evidence_masks", masks, 9 * px + px // 8)):
        us = 1e3 * timed(lambda: ops.verify_evidence(ren, depth, fi, 1.0, verify.DEFAULT_TAU, m, check=False))
        row[name + "_us"], row[name + "_GBps"] = round(us, 2), round(nbytes / us / 1e3, 1)
    row["select_lds_us"] = round(1e3 * timed(sel), 2)
    ops.set_verify_lds_words(1)
    try:
        row["select_workspace_us"] = round(1e3 * timed(sel), 2)
    finally:
        ops.set_verify_lds_words(0)
    row["render_depth_us"] = round(1e3 * timed(lambda: ops.render_depth(mesh["vertices"], mesh["faces"], Pt, cams, H, W, 1.0, check_faces=False)), 2)
    row["verify_poses_us"] = round(1e3 * timed(whole), 2)
    given = dict(render=dict(depth=ren, skipped=torch.zeros(N, dtype=torch.int32, device=dev)))
    row["verify_poses_given_render_us"] = round(1e3 * timed(lambda: whole(**given)), 2)
    fused = whole(**given)
    with policy.use(disable_fused="verify_evidence,verify_select"):
        lib = whole(**given)                                               # the same renders: the two branches must be EQUAL
        row["library_verify_poses_us"] = round(1e3 * timed(whole, 0.5), 2)
        row["library_given_render_us"] = round(1e3 * timed(lambda: whole(**given), 0.5), 2)
    row["library_equal"] = all(bool(torch.equal(lib[key], fused[key])) for key in fused)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "verify_time.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda")
    rows = []
    for frames, per in ((1, 32), (8, 32)):
        rows.append(case(frames, per, dev))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), frame=[H, W], rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as g:
            json.dump(out, g, indent=1)
    return out


if __name__ == "__main__":
    main()
