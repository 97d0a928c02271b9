"""Times of the overlay kernels (csrc/s6d_vis.hip) on the GPU next to the torch statements of the same definitions on the same device
(profiles/vis.md):

python tools/vis_time.py [--hw 480 640] [--counts 1 32 256] [--group 8] [--rounds 3] [--repeats 20] [--kernels-only] [--out FILE]

  owner     N seeded rectangular masks of one frame as packed words -> ``ops.vis_owner_from_masks``
  merge     N rendered layers of a 24 x 24 torus (``ops.render_views``, timed beside it) -> ``ops.vis_merge_layers``
  paint     the merged canvas of one frame and of a group: ``ops.vis_paint`` (table and shade); bytes = 10 per pixel (3 + 4 read,
            3 written; 13 with the shade)
  project   N instances x 520 points -> ``ops.vis_project``
  draw      the 524 primitives (12 box edges of size 3, 512 discs of radius 1) of each of N instances of one frame ->
            ``ops.vis_draw``; ``tile_hits`` = the number of (draw tile, primitive) pairs whose inflated box meets the tile, counted
            from the list on the host, ``tile_tests`` = tiles x primitives, what the binning pass walks
  pictures  both pictures of a group of frames with N / group instances and detections each: ``visualize.overlay_detections`` and
            ``visualize.overlay_poses`` (box and points; and with the surface layer), wall time of the whole call after a
            synchronisation, everything included
Each beside the torch statement of sam6d_amd/visualize.py on the same device tensors, with a check that the two agree; medians over
the rounds after a dropped warm-up round.  ``--kernels-only``: only the kernel calls, the target of a ``rocprofv3 --kernel-trace
--stats`` run.  Prints one JSON line.  There is no CPU path: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--hw", type=int, nargs=2, default=(480, 640))
    ap.add_argument("--counts", type=int, nargs="+", default=(1, 32, 256))
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch

    import bop_gt_time
    from sam6d_amd import ops, policy
    from sam6d_amd import visualize as V
    if not torch.cuda.is_available():
        raise SystemExit("vis_time: needs a GPU")
    dev, (H, W) = torch.device("cuda"), tuple(a.hw)

    def device_ms(fn, n):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def wall_ms(fn, n):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    def pair(kernel, library, n, timer=device_ms):
        tk, tl = [], []
        for _ in range(a.rounds + 1):
            tk.append(timer(kernel, n))
            if library is not None and not a.kernels_only:
                tl.append(timer(library, max(1, n // 10)))
        return dict(kernel_ms=statistics.median(tk[1:]), library_ms=statistics.median(tl[1:]) if tl else None, kernel_rounds=tk[1:], library_rounds=tl[1:])

    def same(x, y):
        return bool(torch.equal(x, y))

    out = dict(hw=[H, W], rounds=a.rounds, repeats=a.repeats, owner=[], merge=[], paint=[], project=[], draw=[], pictures=[])
    v, f = bop_gt_time.torus()
    models = {1: dict(vertices=v, faces=f)}
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    grey = torch.full((len(v), 3), 200, dtype=torch.uint8, device=dev)
    cam = np.array([572.4, 573.6, W / 2 + 5.3, H / 2 + 2.0], np.float32)
    rs = np.random.RandomState(0)
    image = torch.from_numpy(rs.randint(0, 256, (a.group, H, W, 3)).astype(np.uint8)).to(dev)
    canvas1 = None
    for N in a.counts:
        # ---- owner from masks
        masks = torch.zeros(N, H, W, dtype=torch.uint8, device=dev)
        for n in range(N):
            y0, x0 = rs.randint(0, H - 40), rs.randint(0, W - 40)
            masks[n, y0:y0 + rs.randint(20, 200), x0:x0 + rs.randint(20, 200)] = 1
        packed = ops.mask_pack(masks)[0]
        order, start, _ = V.rank_detections(torch.from_numpy(rs.uniform(size=N).astype(np.float32)).to(dev), torch.zeros(N, dtype=torch.int64, device=dev), 1)
        rec = pair(lambda: ops.vis_owner_from_masks(packed, order, start, H, W), lambda: V._owner_library(packed, order, start, H, W), a.repeats)
        if not a.kernels_only:
            rec["equal_library"] = same(ops.vis_owner_from_masks(packed, order, start, H, W), V._owner_library(packed, order, start, H, W))
        out["owner"].append(dict(detections=N, **rec))
        del masks
        # ---- merge of rendered layers
        P = torch.from_numpy(bop_gt_time.poses(N, (H, W), cam)).to(dev)
        frame = torch.zeros(N, dtype=torch.int32, device=dev)
        views = ops.render_views(tv, tf, grey, P, *[float(c) for c in cam], H, W, 0.3, 0.7, 1.0)
        render_ms = device_ms(lambda: ops.render_views(tv, tf, grey, P, *[float(c) for c in cam], H, W, 0.3, 0.7, 1.0), max(1, a.repeats // 4))
        rec = pair(lambda: ops.vis_merge_layers(ops.vis_canvas(1, H, W, dev), views["depth"], views["rgb"], frame, 0),
                   (lambda: V._merge_library(ops.vis_canvas(1, H, W, dev), views["depth"], views["rgb"], frame, 0)) if N <= 32 else None, a.repeats)
        canvas = ops.vis_merge_layers(ops.vis_canvas(1, H, W, dev), views["depth"], views["rgb"], frame, 0)
        if not a.kernels_only and N <= 32:
            lib = V._merge_library(ops.vis_canvas(1, H, W, dev), views["depth"], views["rgb"], frame, 0)
            rec["equal_library"] = all(same(canvas[k], lib[k]) for k in canvas)
        out["merge"].append(dict(layers=N, render_views_ms=render_ms, bytes=N * H * W * 4 + 11 * H * W, **rec))
        canvas1 = canvas if N == 32 or canvas1 is None else canvas1
        del views
        # ---- project and draw
        R, t = P[:, :3, :3].contiguous(), P[:, :3, 3].contiguous()
        cams = torch.from_numpy(np.tile(cam, (N, 1))).to(dev)
        pts = torch.cat([V.box_corners(v), V.model_points(v)]).to(dev)
        M = pts.shape[0]
        pp, ii = pts.repeat(N, 1).contiguous(), torch.arange(N, device=dev).int().repeat_interleave(M).contiguous()
        rec = pair(lambda: ops.vis_project(pp, ii, R, t, cams, 1.0), lambda: V._project_library(pp, ii, R, t, cams, 1.0), a.repeats)
        if not a.kernels_only:
            k, l = ops.vis_project(pp, ii, R, t, cams, 1.0), V._project_library(pp, ii, R, t, cams, 1.0)
            rec["equal_library"] = same(k[0], l[0]) and same(k[1], l[1])
        out["project"].append(dict(instances=N, points=N * M, **rec))
        colors = V.palette(N).to(dev)
        prims = V.pose_primitives(models, [1] * N, R, t, cams, torch.zeros(N, dtype=torch.int64, device=dev), colors, ("box", "points"), "extent", None, 1.0)
        ps = torch.tensor([0, prims.shape[0]], dtype=torch.int64, device=dev)
        base = image[:1].clone()
        rec = pair(lambda: ops.vis_draw(base, prims, ps, check=False), (lambda: V._draw_library(base.clone(), prims, ps)) if N <= 32 else None,
                   a.repeats)
        if not a.kernels_only and N <= 32:
            rec["equal_library"] = same(ops.vis_draw(image[:1].clone(), prims, ps, check=False), V._draw_library(image[:1].clone(), prims, ps))
        e = prims.cpu().numpy().astype(np.int64)
        e = e[e[:, 7] != 0]
        r = (e[:, 5] + 1) // 2
        lox, hix = np.minimum(e[:, 1], e[:, 3]) - r, np.maximum(e[:, 1], e[:, 3]) + r
        loy, hiy = np.minimum(e[:, 2], e[:, 4]) - r, np.maximum(e[:, 2], e[:, 4]) + r
        nx = np.clip(np.minimum(hix, W - 1) // 32 - np.maximum(lox, 0) // 32 + 1, 0, None) * ((hix >= 0) & (lox < W))
        ny = np.clip(np.minimum(hiy, H - 1) // 8 - np.maximum(loy, 0) // 8 + 1, 0, None) * ((hiy >= 0) & (loy < H))
        tiles = ((W + 31) // 32) * ((H + 7) // 8)
        out["draw"].append(dict(instances=N, primitives=int(prims.shape[0]), tile_hits=int((nx * ny).sum()), tile_tests=int(tiles * prims.shape[0]), **rec))
        # ---- both pictures of a group
        G = a.group
        fi = (torch.arange(N) % G).sort().values
        sc = torch.from_numpy(rs.uniform(size=N).astype(np.float32)).to(dev)
        Rn, tn = R.cpu().numpy(), t.cpu().numpy()
        rec = dict(frames=G, instances=N)
        for name, kernel in (("detections", lambda: V.overlay_detections(image, packed, sc, frame_index=fi)),
                             ("poses_box_points", lambda: V.overlay_poses(image, models, [1] * N, Rn, tn, cam, frame_index=fi)),
                             ("poses_surface_box_points", lambda: V.overlay_poses(image, models, [1] * N, Rn, tn, cam, frame_index=fi,
                                                                                  mode=("surface", "box", "points")))):
            r_k = pair(kernel, None, max(1, a.repeats // 4), wall_ms)
            rec[name + "_ms"] = r_k["kernel_ms"]
            rec[name + "_rounds"] = r_k["kernel_rounds"]
            if not a.kernels_only and N <= 32 and name != "poses_surface_box_points":
                with policy.use(disable_fused="vis_owner_from_masks,vis_paint,vis_project,vis_draw"):      # the torch statements, on the device
                    rec[name + "_library_ms"] = wall_ms(kernel, 1)
        out["pictures"].append(rec)
    # ---- paint: one frame and the group, table and shade
    for B in (1, a.group):
        own = canvas1["owner"].expand(B, H, W).contiguous()
        shade = canvas1["shade"].expand(B, H, W, 3).contiguous()
        table = V.palette(256).to(dev)
        img = image[:B].contiguous()
        for name, kw in (("table", dict(colors=table)), ("shade", dict(shade=shade))):
            rec = pair(lambda: ops.vis_paint(img, own, alpha=84, gray=True, edge_width=2, **kw),
                       lambda: V._paint_library(img, own, kw.get("colors"), kw.get("shade"), 84, True, 2, (255, 255, 255)), a.repeats)
            if not a.kernels_only:
                rec["equal_library"] = same(ops.vis_paint(img, own, alpha=84, gray=True, edge_width=2, **kw),
                                            V._paint_library(img, own, kw.get("colors"), kw.get("shade"), 84, True, 2, (255, 255, 255)))
            nbytes = B * H * W * (10 if name == "table" else 13)
            out["paint"].append(dict(frames=B, colour=name, bytes=nbytes, TB_per_s=nbytes / (rec["kernel_ms"] * 1e-3) / 1e12, **rec))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
