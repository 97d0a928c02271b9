"""Score an ISM result file with sam6d_amd.evaluation.coco_scores (COCO AP / AR of the BOP 2D detection and segmentation tasks):

python tools/coco_eval.py --results X.json --dataset DIR [--split test] [--iou-type segm|bbox] [--device cuda|cpu] [--masks dense|rle]
                          [--derive-gt [--models models_eval]]

X.json: the records ``ism.handoff.save_json_bop23`` writes (scene_id, image_id, category_id, bbox x y w h, score, time, segmentation =
uncompressed column-major RLE).  DIR: a dataset in the BOP layout, walked as tools/bop_eval.py walks it --
  DIR/<split>/<scene:06d>/scene_gt.json          obj_id of every instance (the scenes directly under DIR when there is no DIR/<split>)
  DIR/<split>/<scene:06d>/scene_gt_info.json     bbox_visib (x y w h) and visib_fract: an instance below 0.1 is IGNORED, not dropped
  DIR/<split>/<scene:06d>/mask_visib/<im:06d>_<j:06d>.png      the visible mask of instance j (non-zero = set)
Every image named in the ground truth of the scenes the result file covers is scored (test_targets_*.json is not read).  Prints
one JSON line.  --masks rle: the results stay run lists (``handoff.RleMasks``) and the mask_visib PNGs are encoded to run lists on the
device RLE_CHUNK at a time, so the host never holds more than one chunk of dense masks; the same line as --masks dense.
--derive-gt: a scene without scene_gt_info.json, or with a mask_visib PNG missing, gets its boxes, visib_fract and visible masks
derived in memory from the meshes (DIR/<models>/obj_*.ply), the poses and the depth images (sam6d_amd.groundtruth; what
tools/bop_gt.py writes); under --masks rle the derived run lists go straight in, without a PNG round trip.  Without the flag a
missing scene_gt_info.json is a FileNotFoundError, as before.

pycocotools and bop_toolkit are not part of this project: the numbers follow the definition in sam6d_amd/evaluation.py (DESIGN
section 12), and no equality with another tool's output is claimed."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


RLE_CHUNK = 256                                   # mask_visib PNGs held dense at a time under --masks rle


def load_ground_truth(root, split, scenes, min_visib=None, masks="dense", device=None, derive_gt=False, models_dir="models_eval"):
    """-> (ground_truths dict(im (G,2) = scene, image; category, masks (G,H,W) bool, bbox (G,4), ignore), images {(scene, im)}).
    masks="rle": the masks are a ``handoff.RleMasks`` on ``device``, encoded RLE_CHUNK PNGs at a time.  ``derive_gt``: the scenes
    that lack scene_gt_info.json or a mask_visib PNG are derived by ``sam6d_amd.groundtruth`` on ``device``."""
    from PIL import Image

    from bop_eval import walk_scenes
    from sam6d_amd import evaluation
    min_visib = evaluation.COCO_MIN_VISIB if min_visib is None else min_visib
    gt = dict(im=[], category=[], masks=[], bbox=[], ignore=[])
    images = set()
    parts, shapes = [], set()

    def flush():
        import torch

        from sam6d_amd.ism import handoff
        if gt["masks"]:
            parts.append(handoff.RleMasks.from_masks(torch.from_numpy(np.stack(gt["masks"])).to(device or "cpu")))
            gt["masks"].clear()
    models, derived, run = {}, {}, []                      # run: consecutive derived instances whose run lists are still to be taken

    def derive(scene):
        """(result, {(im, j): row}, records by image, dense visible masks or None) of one scene, made once."""
        if scene not in derived:
            import bop_gt
            derived.clear()                                # one scene's result at a time
            res, keys, _ = bop_gt.derive_scene(root, split, scene, models_dir, models, masks=masks, device=device)
            derived[scene] = (res, {k: g for g, k in enumerate(keys)}, bop_gt.info_by_image(res, keys),
                              res["mask_visib"].cpu().numpy() != 0 if masks == "dense" else None)
        return derived[scene]

    def flush_run():
        if run:
            flush()                                        # the dense masks read before them come first
            parts.append(run[0]["mask_visib"][run[1:]])
            run.clear()
    for scene, im, d, records, gt_info, _ in walk_scenes(root, split, scenes):
        if gt_info is None and not derive_gt:
            raise FileNotFoundError(f"{d}/scene_gt_info.json is needed (bbox_visib, visib_fract)")
        images.add((scene, im))
        for j, g in enumerate(records):
            png = os.path.join(d, "mask_visib", f"{im:06d}_{j:06d}.png")
            gt["im"].append((scene, im))
            gt["category"].append(int(g["obj_id"]))
            if derive_gt and (gt_info is None or not os.path.exists(png)):
                res, row, recs, dense = derive(scene)
                rec = recs[im][j] if gt_info is None else gt_info[j]
                shapes.add(tuple(res["size"]))
                if masks == "rle":
                    if run and run[0] is not res:
                        flush_run()
                    run.extend([res, row[(im, j)]] if not run else [row[(im, j)]])
                else:
                    gt["masks"].append(dense[row[(im, j)]])
            else:
                flush_run()
                rec = gt_info[j]
                gt["masks"].append(np.asarray(Image.open(png)) != 0)
                shapes.add(gt["masks"][-1].shape)
            gt["bbox"].append([float(v) for v in rec["bbox_visib"]])
            gt["ignore"].append(float(rec["visib_fract"]) < min_visib)
            if len(shapes) > 1:
                raise ValueError(f"visible masks of different sizes: {sorted(shapes)}")
            if masks == "rle" and len(gt["masks"]) >= RLE_CHUNK:
                flush()
    flush_run()
    n = len(gt["category"])
    if masks == "rle" and n:
        from sam6d_amd.ism import handoff
        flush()
        dense = handoff.RleMasks.cat(parts)
    else:
        dense = np.stack(gt["masks"]) if n else np.zeros((0, 1, 1), bool)
    return dict(im=np.asarray(gt["im"], np.int64).reshape(n, 2), category=np.asarray(gt["category"], np.int64),
                masks=dense, bbox=np.asarray(gt["bbox"], np.float64).reshape(n, 4), ignore=np.asarray(gt["ignore"], bool)), images


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--results", required=True)
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--split", default="test")
    ap.add_argument("--iou-type", default="segm", choices=("segm", "bbox"))
    ap.add_argument("--device", default=None, help="cuda (kernels) or cpu (the torch statements); default: cuda when there is one")
    ap.add_argument("--masks", default="dense", choices=("dense", "rle"),
                    help="rle: results and ground truth stay run lists, packed on the device without dense masks; same output")
    ap.add_argument("--derive-gt", action="store_true", help="derive a missing scene_gt_info.json / mask_visib in memory")
    ap.add_argument("--models", default="models_eval", help="the models directory --derive-gt renders from")
    a = ap.parse_args(argv)
    import torch

    from sam6d_amd import evaluation
    t0 = time.time()
    device = a.device or ("cuda" if torch.cuda.is_available() else "cpu")
    res = evaluation.read_bop_json(a.results, masks=a.masks, device=device if a.masks == "rle" else None)
    gt, images = load_ground_truth(a.dataset, a.split, set(res["scene"].tolist()), masks=a.masks, device=device, derive_gt=a.derive_gt,
                                      models_dir=a.models)
    keep = np.array([(int(s), int(i)) in images for s, i in zip(res["scene"], res["im"])], bool)
    if a.iou_type == "segm" and res["masks"] is None and keep.any():
        raise ValueError(f"{a.results}: the records carry no segmentation; use --iou-type bbox")
    det = dict(im=np.stack([res["scene"], res["im"]], 1)[keep], category=res["category"][keep], score=res["score"][keep], bbox=res["bbox"][keep])
    if res["masks"] is not None:
        det["masks"] = res["masks"][keep]
    out = evaluation.coco_scores(det, gt, a.iou_type, device=device)
    out.update(results=os.path.basename(a.results), images=len(images), dropped_detections=int((~keep).sum()), seconds=round(time.time() - t0, 3))
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
