"""Score a BOP result file with sam6d_amd.evaluation (MSSD, MSPD, VSD and their average recall, BOP19 parameters):

python tools/bop_eval.py --results X.csv --dataset DIR [--split test] [--device cuda|cpu] [--derive-gt]

X.csv: the lines ``pem.results.write_bop_csv`` writes (``scene,im,obj,score,R,t,time``; what FramePipeline and tools/run_sharded.py
produce).  DIR: a dataset in the BOP layout --
  DIR/models_eval/models_info.json, DIR/models_eval/obj_000001.ply ...      the evaluation models (``render.load_ply`` reads them)
  DIR/<split>/<scene:06d>/scene_gt.json, scene_camera.json, depth/<im:06d>.png      (the scenes directly under DIR when there is no
                                                                                    DIR/<split>)
  DIR/<split>/<scene:06d>/scene_gt_info.json   optional: the targets are the ground truths with visib_fract >= 0.1; all of them when
                                               the file is absent
--derive-gt: where models_eval/models_info.json or a scene's scene_gt_info.json is absent, the diameter and the visib_fract of the
ground truths are derived in memory from the meshes, the poses and the depth images (sam6d_amd.groundtruth; what tools/bop_gt.py
writes); without the flag the tool behaves as described above.
--add: the line gains ``add`` = ``evaluation.add_scores``: recall (error below --add-frac of the diameter) and AUC (thresholds up to
--auc-max model units) of ADD, ADD-S and ADD(-S), as defined in csrc/s6d_adderr.hip and sam6d_amd/evaluation.py.
--check-symmetries: the line gains ``symmetries`` = per object how far its symmetry transforms move the mesh off itself
(``evaluation.symmetry_residuals``), with a warning on stderr above --sym-tol of the diameter.  Without these flags the line is
what it was before they existed.
Every image named in the scenes' ground truth that the result file's scenes cover is scored; depth PNGs are 16 bit, times
``depth_scale`` = millimetres.  Prints one JSON line.

bop_toolkit is not part of this project: the errors follow the definitions restated in sam6d_amd/evaluation.py and
csrc/s6d_boperr.hip, and no equality with the toolkit's numbers is claimed."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def walk_scenes(root, split, scenes):
    """The scene walk the evaluation tools share (tools/coco_eval.py too): for every scene of ``scenes`` in ascending order and every
    image its scene_gt.json names, in ascending order, yields (scene, im, scene directory, the image's ground-truth records, their
    scene_gt_info.json records or None when the file is absent, the image's scene_camera.json record)."""
    base = os.path.join(root, split) if os.path.isdir(os.path.join(root, split)) else root
    for scene in sorted(scenes):
        d = os.path.join(base, f"{scene:06d}")
        with open(os.path.join(d, "scene_gt.json")) as f:
            scene_gt = {int(k): v for k, v in json.load(f).items()}
        with open(os.path.join(d, "scene_camera.json")) as f:
            scene_cam = {int(k): v for k, v in json.load(f).items()}
        gt_info = None
        if os.path.exists(os.path.join(d, "scene_gt_info.json")):
            with open(os.path.join(d, "scene_gt_info.json")) as f:
                gt_info = {int(k): v for k, v in json.load(f).items()}
        for im in sorted(scene_gt):
            yield scene, im, d, scene_gt[im], None if gt_info is None else gt_info[im], scene_cam[im]


def load_dataset(root, split, scenes, min_visib=0.1, derive_gt=False, device=None):
    """-> (models {obj: dict}, ground_truths dict, images dict, index {(scene, im): image number}).  ``derive_gt``: a missing
    models_info.json and the visib_fract of scenes without scene_gt_info.json come from ``sam6d_amd.groundtruth`` (on ``device``)."""
    from PIL import Image

    from sam6d_amd import render
    info = None
    if not derive_gt or os.path.exists(os.path.join(root, "models_eval", "models_info.json")):
        with open(os.path.join(root, "models_eval", "models_info.json")) as f:
            info = {int(k): v for k, v in json.load(f).items()}
    index, cams, depths = {}, [], []
    gt = dict(im=[], obj=[], pose=[])
    derived = []                                                           # positions in gt whose visib_fract is still to be derived
    for scene, im, d, records, gt_info, cam in walk_scenes(root, split, scenes):
        K = np.asarray(cam["cam_K"], np.float64).reshape(3, 3)
        depth = np.asarray(Image.open(os.path.join(d, "depth", f"{im:06d}.png")), np.float32) * np.float32(cam.get("depth_scale", 1.0))
        index[(scene, im)] = len(cams)
        cams.append([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
        depths.append(depth)
        for j, g in enumerate(records):
            if gt_info is not None and float(gt_info[j].get("visib_fract", 1.0)) < min_visib:
                continue
            P = np.eye(4)
            P[:3, :3] = np.asarray(g["cam_R_m2c"], np.float64).reshape(3, 3)
            P[:3, 3] = np.asarray(g["cam_t_m2c"], np.float64).reshape(3)
            if gt_info is None and derive_gt:
                derived.append(len(gt["im"]))
            gt["im"].append(index[(scene, im)])
            gt["obj"].append(int(g["obj_id"]))
            gt["pose"].append(P)
    if len({d.shape for d in depths}) > 1:
        raise ValueError(f"depth images of different sizes: {sorted({d.shape for d in depths})}")
    models = {}
    for obj in sorted(set(gt["obj"])):
        v, f, _ = render.load_ply(os.path.join(root, "models_eval", f"obj_{obj:06d}.ply"))
        if info is None:
            from sam6d_amd import groundtruth
            rec = groundtruth.model_info(v, device=device)
        else:
            rec = info[obj]
        models[obj] = dict(vertices=v, faces=f, info=rec, diameter=float(rec["diameter"]))
    images = dict(cams=np.asarray(cams, np.float32).reshape(-1, 4), depth=np.stack(depths) if depths else np.zeros((0, 1, 1), np.float32))
    gt = dict(im=np.asarray(gt["im"], np.int64), obj=np.asarray(gt["obj"], np.int64), pose=np.asarray(gt["pose"], np.float64).reshape(-1, 4, 4))
    if derived:
        from sam6d_amd import groundtruth
        sel = np.asarray(derived, np.int64)
        res = groundtruth.instance_ground_truth(models, {k: v[sel] for k, v in gt.items()}, images, device=device)
        keep = np.ones(len(gt["im"]), bool)
        keep[sel] = res["visib_fract"] >= min_visib
        gt = {k: v[keep] for k, v in gt.items()}
    return models, gt, images, index


def check_symmetries(models, tol, device=None):
    """{obj: dict(transforms, max_fraction, mean_fraction, worst, ok)}: ``evaluation.symmetry_residuals`` of every object's symmetry
    set; a warning on stderr for an object whose largest residual exceeds ``tol`` of its diameter (MSSD, MSPD and ADD-S are wrong
    for a transform that does not map the mesh onto itself)."""
    from sam6d_amd import evaluation
    out = {}
    for obj, m in sorted(models.items()):
        syms = m["symmetries"] if "symmetries" in m else evaluation.symmetry_transforms(m.get("info", {}))
        r = evaluation.symmetry_residuals(m["vertices"], syms, diameter=m["diameter"], device=device)
        worst = int(np.argmax(r["max_fraction"]))
        ok = bool(r["max_fraction"][worst] <= tol)
        out[str(obj)] = dict(transforms=int(len(syms)), max_fraction=float(r["max_fraction"][worst]), mean_fraction=float(r["mean_fraction"].max()),
                             worst=worst, ok=ok)
        if not ok:
            print(f"bop_eval: warning: symmetry transform {worst} of object {obj} moves a vertex {r['max_fraction'][worst]:.4f} of the diameter "
                  f"off the mesh (tolerance {tol}): MSSD, MSPD and ADD-S of this object are unreliable", file=sys.stderr)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--results", required=True)
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--split", default="test")
    ap.add_argument("--device", default=None, help="cuda (kernels) or cpu (the torch statements); default: cuda when there is one")
    ap.add_argument("--derive-gt", action="store_true", help="derive a missing models_info.json / scene_gt_info.json in memory")
    ap.add_argument("--add", action="store_true", help="also report ADD, ADD-S and ADD(-S): recall below --add-frac of the diameter, AUC up to --auc-max")
    ap.add_argument("--add-frac", type=float, default=0.1)
    ap.add_argument("--auc-max", type=float, default=100.0, help="upper end of the AUC's threshold range, model units (100 = 10 cm for millimetre models)")
    ap.add_argument("--check-symmetries", action="store_true",
                    help="report how far every symmetry transform of models_info.json moves the mesh off itself (evaluation.symmetry_residuals)")
    ap.add_argument("--sym-tol", type=float, default=0.01, help="warn when a transform's largest residual exceeds this fraction of the diameter")
    a = ap.parse_args(argv)
    from sam6d_amd import evaluation
    t0 = time.time()
    res = evaluation.read_bop_csv(a.results)
    models, gt, images, index = load_dataset(a.dataset, a.split, set(res["scene"].tolist()), derive_gt=a.derive_gt, device=a.device)
    keep = np.array([(int(s), int(i)) in index for s, i in zip(res["scene"], res["im"])], bool)
    pose = np.tile(np.eye(4), (int(keep.sum()), 1, 1))
    pose[:, :3, :3], pose[:, :3, 3] = res["R"][keep], res["t"][keep]
    est = dict(im=np.array([index[(int(s), int(i))] for s, i in zip(res["scene"][keep], res["im"][keep])], np.int64), obj=res["obj"][keep],
               score=res["score"][keep], pose=pose)
    out = evaluation.bop19_scores(models, est, gt, images, device=a.device)
    if a.add:
        out["add"] = evaluation.add_scores(models, est, gt, frac=a.add_frac, auc_max=a.auc_max, device=a.device)
    if a.check_symmetries:
        out["symmetries"] = check_symmetries(models, a.sym_tol, a.device)
    out.update(results=os.path.basename(a.results), images=len(index), dropped_estimates=int((~keep).sum()), seconds=round(time.time() - t0, 3))
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
