"""Verify the poses of a BOP result file against the dataset's depth frames (sam6d_amd/pem/verify.py):

python tools/verify_poses.py --results X.csv --dataset DIR --out Y.csv [--score verify|keep] [--keep-all] [--force]
                             [--split test] [--models models_eval] [--device cuda|cpu]

X.csv: the lines ``pem.results.write_bop_csv`` writes; DIR: a dataset in the BOP layout, read the way tools/refine_poses.py reads it
(scene_camera.json, depth/<im:06d>.png times depth_scale = millimetres, DIR/<models>/obj_<id:06d>.ply).  Every image's estimates are
verified in one call with the defaults of ``verify_poses`` (its camera, its depth frame, all its estimates in the default visiting
order).  Y.csv gets the KEPT lines (status 0) -- all lines with --keep-all -- with the verification score in the score column
(--score keep: the score of X.csv); poses and times are X.csv's (the writer takes metres and writes float32 millimetres: a
translation may change in its last bit).  An estimate whose image the dataset does not have cannot be judged: its line is written
as it is.  Y.csv is never written over without --force.  Prints one JSON line: how many lines each status took.  On the CPU the
torch statements of the same definition run (small datasets)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--results", required=True)
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--score", choices=("verify", "keep"), default="verify", help="the score column: the verification score, or X.csv's")
    ap.add_argument("--keep-all", action="store_true", help="write every line, not only the kept ones")
    ap.add_argument("--force", action="store_true", help="write over an existing Y.csv")
    ap.add_argument("--split", default="test")
    ap.add_argument("--models", default="models_eval", help="the folder of DIR that holds obj_<id:06d>.ply")
    ap.add_argument("--device", default=None, help="cuda (default when there is one) or cpu")
    a = ap.parse_args(argv)
    if os.path.exists(a.out) and not a.force:
        raise SystemExit(f"verify_poses.py: {a.out} exists; --force writes over it")
    import torch
    from PIL import Image

    import bop_eval
    from sam6d_amd import evaluation, render
    from sam6d_amd.pem import refine, results, verify
    dev = torch.device(a.device or ("cuda" if torch.cuda.is_available() else "cpu"))
    t0 = time.time()
    res = evaluation.read_bop_csv(a.results)
    objs = sorted(set(res["obj"].tolist()))
    meshes = []
    for obj in objs:
        v, f, _ = render.load_ply(os.path.join(a.dataset, a.models, f"obj_{obj:06d}.ply"))
        meshes.append(refine.device_mesh(v, f, dev))
    rows = {}
    for k, (s, i) in enumerate(zip(res["scene"].tolist(), res["im"].tolist())):
        rows.setdefault((s, i), []).append(k)
    n = len(res["R"])
    status = np.full(n, -1, np.int64)                                          # -1: the dataset has no such image
    score = res["score"].astype(np.float64)
    for scene, im, d, _, _, cam in bop_eval.walk_scenes(a.dataset, a.split, {s for s, _ in rows}):
        sel = rows.get((scene, im))
        if not sel:
            continue
        depth = np.asarray(Image.open(os.path.join(d, "depth", f"{im:06d}.png")), np.float32) * np.float32(cam.get("depth_scale", 1.0))
        out = verify.verify_poses(meshes, [objs.index(int(o)) for o in res["obj"][sel]], torch.from_numpy(res["R"][sel]).to(dev),
                                  torch.from_numpy(res["t"][sel]).to(dev), torch.from_numpy(depth).to(dev),
                                  np.asarray(cam["cam_K"], np.float64).reshape(3, 3))
        status[sel] = out["status"].cpu().numpy()
        if a.score == "verify":
            score[sel] = out["score"].cpu().numpy()
    lines = []
    for k in range(n):
        if a.keep_all or status[k] <= 0:
            lines += results.bop_csv_lines(res["scene"][k], res["im"][k], [res["obj"][k]], score[k:k + 1].astype(np.float32), res["R"][k:k + 1],
                                           res["t"][k:k + 1] / np.float32(1000), res["time"][k])
    results.write_bop_csv(a.out, lines)
    summary = dict(results=os.path.basename(a.results), out=os.path.basename(a.out), estimates=n, written=len(lines), score=a.score,
                   status={name: int((status == code).sum()) for code, name in list(verify.STATUS.items()) + [(-1, "image not in the dataset")]},
                   seconds=round(time.time() - t0, 3))
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
