"""Times of the ADD / ADD-S kernels (csrc/s6d_adderr.hip) on the GPU next to the chunked torch statement of the same function and to
the diameter kernel's pair rate, all in ONE run on the same device (profiles/add_eval.md):

python tools/add_time.py [--shapes 1x1000 32x8192 256x8192 8x131072] [--rounds 3] [--repeats 20] [--kernels-only] [--out FILE]

  inputs     V seeded vertices uniform in a box, N seeded ground-truth poses, each estimate a few degrees and units off.
  adds       ``ops.add_errors(which=("adds",))`` by device events at every sources-per-lane setting (1, 2, 4;
             ``s6d_set_adds_sources_per_lane``) and at the library's default (0); the window holds the all-pairs kernel and the
             row reduction.  Pairs = N * ceil(V / 256)^2 * 65536 (whole 256 x 256 tiles); 9 float32 lane operations per pair (3
             differences, 3 products, 2 sums, 1 minimum).  The settings are timed alternating, round by round; the first round warms
             up and is dropped; the figures are medians over the rounds.
  add        ``ops.add_errors(which=("add",))``: one lane per (n, i).
  library    ``evaluation._add_errors_library`` (a chunk of source rows against all targets at a time) on the same device tensors;
             its per-vertex values and means must be EQUAL to the kernels'.  One timed call per round (one round at the shapes of
             more than 5 10^10 pairs).
  diameter   ``ops.model_diameter`` on the same vertices: pairs = tiles (tiles + 1) / 2 * 65536, the same nine operations per pair.
``--kernels-only``: only the kernel calls, the target of a ``rocprofv3 --kernel-trace --stats`` run.  Prints one JSON line.  There is
no CPU path: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def rotation(rs, angle=None):
    q, _ = np.linalg.qr(rs.standard_normal((3, 3)))
    q = q * np.sign(np.linalg.det(q))
    if angle is None:
        return q
    a = q[:, 0]
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def inputs(N, V):
    rs = np.random.RandomState(1000 * N + V % 1000)
    v = (rs.uniform(-1, 1, (V, 3)) * np.array([120.0, 80.0, 40.0])).astype(np.float32)
    gt = np.tile(np.eye(4), (N, 1, 1))
    est = gt.copy()
    for n in range(N):
        gt[n, :3, :3], gt[n, :3, 3] = rotation(rs), (rs.uniform(-100, 100), rs.uniform(-100, 100), rs.uniform(400, 900))
        est[n, :3, :3], est[n, :3, 3] = gt[n, :3, :3] @ rotation(rs, 0.05), gt[n, :3, 3] + rs.uniform(-5, 5, 3)
    return v, est.astype(np.float32), gt.astype(np.float32)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", nargs="+", default=("1x1000", "32x8192", "256x8192", "8x131072"), help="N x V")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch

    from sam6d_amd import _lib, evaluation, ops
    if not torch.cuda.is_available():
        raise SystemExit("add_time: needs a GPU")
    dev = torch.device("cuda")

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

    def with_spl(spl, fn):
        def call():
            assert _lib.lib().s6d_set_adds_sources_per_lane(spl) == 0
            try:
                return fn()
            finally:
                _lib.lib().s6d_set_adds_sources_per_lane(0)
        return call

    out = dict(rounds=a.rounds, repeats=a.repeats, shapes=[])
    for shape in a.shapes:
        N, V = (int(x) for x in shape.lower().split("x"))
        v, est, gt = (torch.from_numpy(x).to(dev) for x in inputs(N, V))
        tiles = (V + 255) // 256
        pairs = N * tiles * tiles * 65536
        reps = max(2, min(a.repeats, int(4e11 // pairs) or 2))
        adds = lambda: ops.add_errors(v, est, gt, which=("adds",))                                      # noqa: E731
        routes = {f"adds_spl{s}": with_spl(s, adds) for s in (1, 2, 4)}
        routes["adds_default"] = adds
        routes["add"] = lambda: ops.add_errors(v, est, gt, which=("add",))                              # noqa: E731
        routes["diameter"] = lambda: ops.model_diameter(v)                                              # noqa: E731
        lib_rounds = 0 if a.kernels_only else (1 if pairs > 5e10 else a.rounds)
        library = lambda: evaluation._add_errors_library(v, est, gt, ("adds",), chunk_bytes=1 << 28)    # noqa: E731
        times = {k: [] for k in routes}
        lib_times = []
        for r in range(a.rounds + 1):
            for k, fn in routes.items():
                times[k].append(device_ms(fn, reps if k != "add" else a.repeats))
            if r >= 1 and len(lib_times) < lib_rounds:
                lib_times.append(device_ms(library, 1))                    # (device_ms itself makes one warm-up call)
        ms = {k: statistics.median(t[1:]) for k, t in times.items()}
        dpairs = tiles * (tiles + 1) // 2 * 65536
        rec = dict(N=N, V=V, pairs=pairs, repeats=reps, ms=ms, library_adds_ms=statistics.median(lib_times) if lib_times else None,
                   pairs_per_s={k: pairs / (ms[k] * 1e-3) for k in ms if k.startswith("adds")}, diameter_pairs=dpairs,
                   diameter_pairs_per_s=dpairs / (ms["diameter"] * 1e-3), all_rounds={k: t[1:] for k, t in times.items()}, library_rounds=lib_times)
        rec["adds_over_diameter_rate"] = rec["pairs_per_s"]["adds_default"] / rec["diameter_pairs_per_s"]
        got = ops.add_errors(v, est, gt, per_vertex=True)
        if not a.kernels_only:
            ref = evaluation._add_errors_library(v, est, gt, chunk_bytes=1 << 28)
            rec["equal_library"] = bool(all(torch.equal(got[k].view(torch.int32 if got[k].dtype == torch.float32 else torch.int64),
                                                        ref[k].view(torch.int32 if ref[k].dtype == torch.float32 else torch.int64)) for k in got))
            del ref
        rec["variants_equal"] = bool(all(torch.equal(with_spl(s, lambda: ops.add_errors(v, est, gt, per_vertex=True, which=("adds",)))()["adds_per_vertex"],
                                                     got["adds_per_vertex"]) for s in (1, 2, 4)))
        rec["add_mean"], rec["adds_mean"] = float(got["add"].mean().cpu()), float(got["adds"].mean().cpu())
        out["shapes"].append(rec)
        del got, v, est, gt
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
