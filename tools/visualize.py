"""Draw result files over the frames of a dataset with sam6d_amd.visualize:

python tools/visualize.py --dataset DIR --out DIR [--results X.csv ...] [--gt] [--detections X.json] [--masks dense|rle]
                          [--split test] [--mode box,points[,surface]] [--top 1] [--device cuda|cpu] [--force]

--results X.csv: the poses of a BOP result file (``pem.results.write_bop_csv``) as projected boxes and model points; the option can
be given more than once and every file gets its own colour (``visualize.palette``: the first red, the second green ...), --gt adds
the annotated poses of scene_gt.json in the next colour: the poses before and after tools/refine_poses.py and the ground truth
in one picture.  -> OUT/vis_pem_<scene:06d>_<im:06d>.png.
--detections X.json: the masks of a detection file (``ism.handoff.save_json_bop23``) blended over the grey frame with their contours
in white, the best --top per image (0 = all; 1 is the reference's picture).  --masks rle: the run lists go to the device as they
are and no dense mask is made anywhere.  -> OUT/vis_ism_<scene:06d>_<im:06d>.png.
DIR is a dataset in the BOP layout as tools/bop_eval.py reads it (its ``load_dataset``: meshes, cameras, the image list), with the
frames under <scene>/rgb/<im:06d>.png (or .jpg); a frame without an rgb file is drawn over its depth image, scaled to grey.
An existing file is never overwritten without --force: the tool stops before it writes anything.  Prints one JSON line.

The pictures are this project's own definition (csrc/s6d_vis.hip); none is claimed to equal the reference's cv2 drawing."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

GROUP = 8                                          # frames drawn per call


def scene_dirs(root, split):
    base = os.path.join(root, split) if os.path.isdir(os.path.join(root, split)) else root
    return base, sorted(int(d) for d in os.listdir(base) if d.isdigit() and os.path.exists(os.path.join(base, d, "scene_gt.json")))


def load_frame(base, scene, im, depth):
    """(H,W,3) uint8: the rgb file of the frame, or its depth image scaled to grey."""
    from PIL import Image
    for ext in ("png", "jpg"):
        p = os.path.join(base, f"{scene:06d}", "rgb", f"{im:06d}.{ext}")
        if os.path.exists(p):
            return np.asarray(Image.open(p).convert("RGB"), np.uint8)
    top = float(depth.max())
    g = (depth * (255.0 / top)).astype(np.uint8) if top > 0 else np.zeros(depth.shape, np.uint8)
    return np.repeat(g[..., None], 3, 2)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--split", default="test")
    ap.add_argument("--results", action="append", default=[], help="a BOP pose csv; repeatable, one colour per file")
    ap.add_argument("--gt", action="store_true", help="also draw the annotated poses of scene_gt.json")
    ap.add_argument("--detections", default=None, help="a detection json with run-length masks")
    ap.add_argument("--masks", default="rle", choices=("dense", "rle"), help="rle: the run lists are drawn without a dense mask")
    ap.add_argument("--mode", default="box,points", help="comma list of box, points, surface")
    ap.add_argument("--top", type=int, default=1, help="detections drawn per image, best first; 0 = all")
    ap.add_argument("--device", default=None, help="cuda (kernels) or cpu (the torch statements); default: cuda when there is one")
    ap.add_argument("--force", action="store_true", help="overwrite existing files")
    a = ap.parse_args(argv)
    if not a.results and not a.gt and not a.detections:
        ap.error("nothing to draw: give --results, --gt or --detections")
    import torch

    import bop_eval
    from sam6d_amd import evaluation, visualize
    dev = torch.device(a.device if a.device else ("cuda" if torch.cuda.is_available() else "cpu"))
    t0 = time.time()
    base, every = scene_dirs(a.dataset, a.split)
    pose_sets = [evaluation.read_bop_csv(p) for p in a.results]
    det = evaluation.read_bop_json(a.detections, masks=a.masks, device=dev if a.masks == "rle" else None) if a.detections else None
    named = set()
    for r in pose_sets + ([det] if det is not None else []):
        named |= set(int(s) for s in r["scene"].tolist())
    scenes = sorted(named & set(every)) if named else every
    models, gt, images, index = bop_eval.load_dataset(a.dataset, a.split, scenes, min_visib=-1.0)
    keys = sorted(index, key=index.get)                                    # (scene, im) in image-number order
    want_pem, want_ism = bool(pose_sets or a.gt), det is not None
    targets = [os.path.join(a.out, f"vis_{kind}_{s:06d}_{i:06d}.png") for s, i in keys for kind, on in (("pem", want_pem), ("ism", want_ism)) if on]
    if not a.force:
        taken = [p for p in targets if os.path.exists(p)]
        if taken:
            raise FileExistsError(f"{taken[0]} exists ({len(taken)} target file(s) do): pass --force to overwrite")
    os.makedirs(a.out, exist_ok=True)
    # every pose set as (image number, obj, R, t, colour index)
    inst = dict(im=[], obj=[], R=[], t=[], col=[])
    for k, r in enumerate(pose_sets):
        keep = [n for n in range(len(r["im"])) if (int(r["scene"][n]), int(r["im"][n])) in index and int(r["obj"][n]) in models]
        inst["im"] += [index[(int(r["scene"][n]), int(r["im"][n]))] for n in keep]
        inst["obj"] += [int(r["obj"][n]) for n in keep]
        inst["R"] += [r["R"][n] for n in keep]
        inst["t"] += [r["t"][n] for n in keep]
        inst["col"] += [k] * len(keep)
    if a.gt:
        inst["im"] += gt["im"].tolist()
        inst["obj"] += gt["obj"].tolist()
        inst["R"] += [P[:3, :3].astype(np.float32) for P in gt["pose"]]
        inst["t"] += [P[:3, 3].astype(np.float32) for P in gt["pose"]]
        inst["col"] += [len(pose_sets)] * len(gt["im"])
    i_im, i_col = np.asarray(inst["im"], np.int64), np.asarray(inst["col"], np.int64)
    pal = visualize.palette(len(pose_sets) + 1)
    mode = tuple(m for m in a.mode.split(",") if m)
    written = 0
    for g0 in range(0, len(keys), GROUP):
        group = keys[g0:g0 + GROUP]
        nums = [index[k] for k in group]
        frames = torch.from_numpy(np.stack([load_frame(base, s, i, images["depth"][n]) for (s, i), n in zip(group, nums)])).to(dev)
        if want_pem:
            sel = np.nonzero(np.isin(i_im, nums))[0]
            sel = sel[np.argsort(np.searchsorted(nums, i_im[sel]), kind="stable")]          # grouped by frame, the list order inside
            out = visualize.overlay_poses(frames, models, [inst["obj"][n] for n in sel], np.stack([inst["R"][n] for n in sel]).reshape(-1, 3, 3),
                                          np.stack([inst["t"][n] for n in sel]).reshape(-1, 3) if len(sel) else np.zeros((0, 3), np.float32),
                                          images["cams"][i_im[sel]], frame_index=np.searchsorted(nums, i_im[sel]), mode=mode, colors=pal[i_col[sel]]) \
                if len(sel) else frames
            for b, (s, i) in enumerate(group):
                visualize.save_png(os.path.join(a.out, f"vis_pem_{s:06d}_{i:06d}.png"), out[b])
                written += 1
        if want_ism:
            where = {k: b for b, k in enumerate(group)}
            sel = np.array([n for n in range(len(det["im"])) if (int(det["scene"][n]), int(det["im"][n])) in where], np.int64)
            f = np.array([where[(int(det["scene"][n]), int(det["im"][n]))] for n in sel], np.int64)
            if len(sel):
                masks = det["masks"][sel] if a.masks == "rle" else torch.from_numpy(np.asarray(det["masks"])[sel]).to(dev)
                out = visualize.overlay_detections(frames, masks, torch.from_numpy(det["score"][sel]).float(), frame_index=f, top=a.top or None)
            else:
                out = visualize.overlay_detections(frames, torch.zeros(0, *frames.shape[1:3], dtype=torch.uint8, device=dev), torch.zeros(0),
                                                   frame_index=np.zeros(0, np.int64))
            for b, (s, i) in enumerate(group):
                visualize.save_png(os.path.join(a.out, f"vis_ism_{s:06d}_{i:06d}.png"), out[b])
                written += 1
    line = dict(out=a.out, images=len(keys), files=written, pose_sets=len(pose_sets) + int(a.gt), instances=len(inst["im"]),
                detections=0 if det is None else int(len(det["im"])), device=str(dev), seconds=round(time.time() - t0, 3))
    print(json.dumps(line))
    return line


if __name__ == "__main__":
    main()
