"""Refine the poses of a BOP result file against the dataset's depth frames (sam6d_amd/pem/refine.py):

python tools/refine_poses.py --results X.csv --dataset DIR --out Y.csv [--split test] [--models models_eval] [--iterations N]

X.csv: the lines ``pem.results.write_bop_csv`` writes; DIR: a dataset in the BOP layout, read the way tools/bop_eval.py reads it
(scene_camera.json, depth/<im:06d>.png times depth_scale = millimetres, DIR/<models>/obj_<id:06d>.ply).  Every estimate whose image
the dataset has is refined in millimetres with the defaults of ``refine_poses`` (one call per image: its camera, its depth frame, all
its estimates grouped by object); estimates of other images and those the refiner did not move (status != 0) keep their pose.  Y.csv
is written by ``pem.results``' writer with the scores and times of X.csv, so ``tools/bop_eval.py`` on both files shows the average
recall before and after (the writer takes metres and writes float32 millimetres: a kept translation may change in its last bit).
Prints one JSON line: the number of estimates per status and the mean rms of the refined ones.  Needs the GPU."""
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
    ap.add_argument("--split", default="test")
    ap.add_argument("--models", default="models_eval", help="the folder of DIR that holds obj_<id:06d>.ply")
    ap.add_argument("--iterations", type=int, default=None, help="cut (or repeat the last value of) the default schedule to N iterations")
    a = ap.parse_args(argv)
    import torch
    from PIL import Image

    import bop_eval
    from sam6d_amd import evaluation, render
    from sam6d_amd.pem import refine, results
    assert torch.cuda.is_available(), "refine_poses.py runs the kernels; there is no CPU path"
    dev = torch.device("cuda")
    t0 = time.time()
    res = evaluation.read_bop_csv(a.results)
    schedule = list(refine.DEFAULT_SCHEDULE)
    if a.iterations is not None:
        schedule = (schedule + [schedule[-1]] * a.iterations)[:a.iterations]
    objs = sorted(set(res["obj"].tolist()))
    meshes = []
    for obj in objs:
        v, f, _ = render.load_ply(os.path.join(a.dataset, a.models, f"obj_{obj:06d}.ply"))
        meshes.append(refine.device_mesh(v, f, dev))
    rows = {}
    for k, (s, i) in enumerate(zip(res["scene"].tolist(), res["im"].tolist())):
        rows.setdefault((s, i), []).append(k)
    R, t = res["R"].copy(), res["t"].copy()
    status = np.full(len(R), -1, np.int64)                                     # -1: the dataset has no such image
    rms = np.zeros(len(R))
    for scene, im, d, _, _, cam in bop_eval.walk_scenes(a.dataset, a.split, {s for s, _ in rows}):
        sel = rows.get((scene, im))
        if not sel:
            continue
        depth = np.asarray(Image.open(os.path.join(d, "depth", f"{im:06d}.png")), np.float32) * np.float32(cam.get("depth_scale", 1.0))
        out = refine.refine_poses(meshes, [objs.index(int(o)) for o in res["obj"][sel]], torch.from_numpy(R[sel]).to(dev),
                                  torch.from_numpy(t[sel]).to(dev), torch.from_numpy(depth).to(dev),
                                  np.asarray(cam["cam_K"], np.float64).reshape(3, 3), max_dist=schedule)
        R[sel], t[sel] = out["R"].cpu().numpy(), out["t"].cpu().numpy()
        status[sel], rms[sel] = out["status"].cpu().numpy(), out["rms"].cpu().numpy()
    lines = []
    for k in range(len(R)):
        lines += results.bop_csv_lines(res["scene"][k], res["im"][k], [res["obj"][k]], res["score"][k:k + 1], R[k:k + 1],
                                       t[k:k + 1] / np.float32(1000), res["time"][k])
    results.write_bop_csv(a.out, lines)
    done = status == 0
    summary = dict(results=os.path.basename(a.results), out=os.path.basename(a.out), estimates=len(R), iterations=len(schedule),
                   status={name: int((status == code).sum()) for code, name in list(refine.STATUS.items()) + [(-1, "image not in the dataset")]},
                   mean_rms=float(rms[done].mean()) if done.any() else None, seconds=round(time.time() - t0, 3))
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
