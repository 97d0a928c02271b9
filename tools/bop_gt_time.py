"""Times of the ground-truth kernels (csrc/s6d_bopgt.hip) on the GPU next to the torch statements of the same functions on the same
device (profiles/bop_gt.md):

python tools/bop_gt_time.py [--hw 480 640] [--instances 1 32 256] [--vertices 10000 100000 500000] [--rounds 3] [--repeats 20]
                            [--kernels-only] [--out FILE]

  visibility  a 24 x 24 torus at seeded poses (some across the border, some outside the image), one ``ops.render_depth`` canvas per
              instance with the default margin (one image on every side), eight measured depth images (the first instances'
              surfaces in front of a wall, 10 % missing).  ``ops.gt_visibility`` by device events against
              ``groundtruth._gt_visibility_library`` on the same device tensors; the two results must be equal.  Bytes from the
              shapes: 4 per canvas pixel, 2 written per image pixel, 4 more per mask pixel (``bytes_needed``), and the stream's
              upper statement with 4 more for EVERY image pixel (``bytes_stream``); bytes / time is the achieved rate.  The render that
              feeds the kernel is timed beside it.
  diameter    seeded vertices uniform in a box; ``ops.model_diameter`` by device events against
              ``groundtruth._model_diameter_library`` (chunked, no (V,V) buffer); the same bits.  Pairs = V (V + 1) / 2 tile-wise
              (whole 256 x 256 tiles with ti <= tj); 9 float32 lane operations per pair (3 differences, 3 products, 2 sums, 1 maximum).
Per round the two routes run one after the other; the figures are medians over the rounds.  ``--kernels-only``: only the kernel
calls, the target of a ``rocprofv3 --kernel-trace --stats`` run.  Prints one JSON line.  There is no CPU path: without a GPU this
fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def torus(n_major=24, n_minor=24, R=60.0, r=25.0):
    a, b = np.arange(n_major) * (2 * np.pi / n_major), np.arange(n_minor) * (2 * np.pi / n_minor)
    v = np.array([[(R + r * np.cos(y)) * np.cos(x), (R + r * np.cos(y)) * np.sin(x), r * np.sin(y)] for x in a for y in b], np.float32)
    f = []
    for i in range(n_major):
        for j in range(n_minor):
            p, q = i * n_minor + j, i * n_minor + (j + 1) % n_minor
            s, t = ((i + 1) % n_major) * n_minor + j, ((i + 1) % n_major) * n_minor + (j + 1) % n_minor
            f += [[p, s, q], [q, s, t]]
    return v, np.array(f, np.int32)


def poses(n, hw, cam, seed=3):
    """Seeded rotations; centres uniform over the image widened by a quarter on every side, 350 - 900 units away."""
    rs = np.random.RandomState(seed)
    P = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    for k in range(n):
        q, _ = np.linalg.qr(rs.standard_normal((3, 3)))
        P[k, :3, :3] = q * np.sign(np.linalg.det(q))
        z = rs.uniform(350.0, 900.0)
        u, v = rs.uniform(-0.25, 1.25) * hw[1], rs.uniform(-0.25, 1.25) * hw[0]
        P[k, :3, 3] = ((u - cam[2]) / cam[0] * z, (v - cam[3]) / cam[1] * z, z)
    return P


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--hw", type=int, nargs=2, default=(480, 640))
    ap.add_argument("--instances", type=int, nargs="+", default=(1, 32, 256))
    ap.add_argument("--vertices", type=int, nargs="+", default=(10000, 100000, 500000))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch

    from sam6d_amd import groundtruth, ops
    if not torch.cuda.is_available():
        raise SystemExit("bop_gt_time: needs a GPU")
    dev, (H, W) = torch.device("cuda"), tuple(a.hw)
    mx, my = W, H
    Hc, Wc = H + 2 * my, W + 2 * mx

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

    def median_pair(kernel, library, n):
        """Medians of the two routes, alternating; the first round warms both up and is dropped."""
        tk, tl = [], []
        for _ in range(a.rounds + 1):
            tk.append(device_ms(kernel, n))
            if library is not None:
                tl.append(device_ms(library, max(1, n // 10)))
        return statistics.median(tk[1:]), (statistics.median(tl[1:]) if tl else None), tk[1:], tl[1:]

    out = dict(hw=[H, W], margin=[mx, my], rounds=a.rounds, repeats=a.repeats, visibility=[], diameter=[])
    v, f = torus()
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    cam = np.array([572.4, 573.6, W / 2 + 5.3, H / 2 + 2.0], np.float32)
    for N in a.instances:
        P = torch.from_numpy(poses(N, (H, W), cam)).to(dev)
        cams = torch.from_numpy(np.tile(cam, (N, 1))).to(dev)
        shifted = (cams + torch.tensor([0.0, 0.0, float(mx), float(my)], device=dev)).contiguous()
        canvas = ops.render_depth(tv, tf, P, shifted, Hc, Wc, 1.0)["depth"]
        M = min(8, N)
        g = torch.Generator(device="cpu").manual_seed(N)
        test = torch.full((M, H, W), 1000.0, device=dev)
        surf = canvas[:M, my:my + H, mx:mx + W]
        test = torch.where(surf > 0, surf + 2.0, test)
        test[(torch.rand(M, H, W, generator=g) < 0.1).to(dev)] = 0.0
        test = test.contiguous()
        ti = (torch.arange(N, device=dev) % M).int()
        kernel = lambda: ops.gt_visibility(canvas, test, ti, cams, 15.0, (mx, my))                    # noqa: E731
        library = None if a.kernels_only else (lambda: groundtruth._gt_visibility_library(canvas, test, ti, cams, 15.0, (mx, my)))
        ms, lib_ms, all_k, all_l = median_pair(kernel, library, a.repeats)
        render_ms = device_ms(lambda: ops.render_depth(tv, tf, P, shifted, Hc, Wc, 1.0), max(1, a.repeats // 4))
        r = kernel()
        mask_px = int(r["counts"][:, 1].sum())
        needed, stream = N * (4 * Hc * Wc + 2 * H * W) + 4 * mask_px, N * (4 * Hc * Wc + 6 * H * W)
        rec = dict(instances=N, images=M, canvas=[Hc, Wc], gt_visibility_ms=ms, library_ms=lib_ms, render_depth_ms=render_ms, bytes_needed=needed,
                   bytes_stream=stream, needed_TB_per_s=needed / (ms * 1e-3) / 1e12, stream_TB_per_s=stream / (ms * 1e-3) / 1e12,
                   mask_pixels=mask_px, all_pixels=int(r["counts"][:, 0].sum()), visible_pixels=int(r["counts"][:, 3].sum()),
                   all_rounds=dict(kernel=all_k, library=all_l))
        if library is not None:
            ref = library()
            rec["equal_library"] = bool(all(torch.equal(r[k], ref[k]) for k in ("mask", "mask_visib", "counts", "extents")))
            del ref
        out["visibility"].append(rec)
        del canvas, test, r
        torch.cuda.empty_cache()
    for V in a.vertices:
        rs = np.random.RandomState(V)
        verts = torch.from_numpy((rs.uniform(-1, 1, (V, 3)) * np.array([120.0, 80.0, 40.0])).astype(np.float32)).to(dev)
        reps = max(2, min(a.repeats, int(2e10 // (V * V)) or 2))
        kernel = lambda: ops.model_diameter(verts)                                                    # noqa: E731
        library = None if a.kernels_only else (lambda: groundtruth._model_diameter_library(verts, chunk_bytes=1 << 28))
        tk, tl = [], []
        for _ in range(a.rounds + 1):
            tk.append(device_ms(kernel, reps))
            if library is not None:
                tl.append(device_ms(library, 1))
        ms = statistics.median(tk[1:])
        tiles = (V + 255) // 256
        pairs = tiles * (tiles + 1) // 2 * 65536
        rec = dict(vertices=V, model_diameter_ms=ms, library_ms=statistics.median(tl[1:]) if tl else None, tile_pairs=tiles * (tiles + 1) // 2,
                   pairs=pairs, pairs_per_s=pairs / (ms * 1e-3), lane_ops_per_s=9 * pairs / (ms * 1e-3), all_rounds=dict(kernel=tk[1:], library=tl[1:]))
        if library is not None:
            rec["same_bits"] = bool(torch.equal(kernel().view(torch.int32), library().view(torch.int32)))
        rec["diameter"] = float(kernel().cpu()[0])
        out["diameter"].append(rec)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
