"""Derive the ground-truth files of a dataset in the BOP layout from its annotated poses (sam6d_amd.groundtruth):

python tools/bop_gt.py --dataset DIR [--split test] [--scenes 1 2 ...] [--models models_eval] [--delta 15] [--no-depth] [--size H,W]
                       [--write info,masks,models_info] [--box-rule span|pixels] [--device cuda|cpu] [--force]

Read, walked as tools/bop_eval.py walks them --
  DIR/<models>/obj_000001.ply ...                                    the models (``render.load_ply``)
  DIR/<split>/<scene:06d>/scene_gt.json, scene_camera.json           poses and cameras (the scenes directly under DIR when there is
                                                                     no DIR/<split>)
  DIR/<split>/<scene:06d>/depth/<im:06d>.png                         16 bit, times ``depth_scale`` = model units; not read with
                                                                     --no-depth (visibility then shows only the mutual occlusion of the
                                                                     annotated objects; the image size comes from --size or rgb/, gray/)
Written (--write, default all three) --
  DIR/<split>/<scene:06d>/scene_gt_info.json                         bbox_obj, bbox_visib, px_count_all / valid / visib, visib_fract
  DIR/<split>/<scene:06d>/mask/<im:06d>_<j:06d>.png, mask_visib/...  values 0 / 255
  DIR/<models>/models_info.json                                      diameter, min_*, size_* of every model the scenes name
An existing file is never overwritten without --force: the tool stops before it writes anything.  Prints one JSON line: instances,
images, seconds, skipped_instances (instances with triangles behind the near plane: their px_count_all is a lower bound).

bop_toolkit is not part of this project: the quantities follow the definitions of csrc/s6d_bopgt.hip, and no equality with the
toolkit's files is claimed; --box-rule says how a box is written from the inclusive pixel extents."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def scene_ids(root, split):
    """The scene numbers of a split: its directories with all-digit names."""
    base = os.path.join(root, split) if os.path.isdir(os.path.join(root, split)) else root
    return sorted(int(d) for d in os.listdir(base) if d.isdigit() and os.path.exists(os.path.join(base, d, "scene_gt.json")))


def load_models(root, models_dir, objs, models=None):
    """{obj: dict(vertices, faces)} of the named objects, added to ``models``."""
    from sam6d_amd import render
    models = {} if models is None else models
    for obj in sorted(set(int(o) for o in objs)):
        if obj not in models:
            v, f, _ = render.load_ply(os.path.join(root, models_dir, f"obj_{obj:06d}.ply"))
            models[obj] = dict(vertices=v, faces=f)
    return models


def _image_size(d, im, size):
    from PIL import Image
    if size is not None:
        return tuple(size)
    for sub in ("rgb", "gray"):
        for ext in ("png", "jpg", "tif"):
            p = os.path.join(d, sub, f"{im:06d}.{ext}")
            if os.path.exists(p):
                w, h = Image.open(p).size
                return (h, w)
    raise FileNotFoundError(f"{d}: no depth is read and no rgb/ or gray/ image gives the size of image {im}: pass --size H,W")


def scene_inputs(root, split, scene, depth=True, size=None):
    """One scene in the layout of ``tools/bop_eval.load_dataset`` with EVERY annotated instance ->
    (gt dict(im, obj, pose), images dict(cams, depth | size), keys [(im, j)], scene directory, gt_info or None)."""
    from PIL import Image

    from bop_eval import walk_scenes
    cams, depths, ims, keys, infos = [], [], [], [], {}
    gt = dict(im=[], obj=[], pose=[])
    sizes, scene_dir = set(), None
    for _, im, d, records, gt_info, cam in walk_scenes(root, split, [scene]):
        scene_dir = d
        K = np.asarray(cam["cam_K"], np.float64).reshape(3, 3)
        if depth:
            depths.append(np.asarray(Image.open(os.path.join(d, "depth", f"{im:06d}.png")), np.float32) * np.float32(cam.get("depth_scale", 1.0)))
            sizes.add(depths[-1].shape)
        else:
            sizes.add(_image_size(d, im, size))
        if gt_info is not None:
            infos[im] = gt_info
        cams.append([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
        for j, g in enumerate(records):
            P = np.eye(4)
            P[:3, :3] = np.asarray(g["cam_R_m2c"], np.float64).reshape(3, 3)
            P[:3, 3] = np.asarray(g["cam_t_m2c"], np.float64).reshape(3)
            gt["im"].append(len(ims))
            gt["obj"].append(int(g["obj_id"]))
            gt["pose"].append(P)
            keys.append((im, j))
        ims.append(im)
    if len(sizes) > 1:
        raise ValueError(f"scene {scene}: images of different sizes: {sorted(sizes)}")
    images = dict(cams=np.asarray(cams, np.float32).reshape(-1, 4))
    if depth:
        images["depth"] = np.stack(depths) if depths else np.zeros((0, 1, 1), np.float32)
    else:
        images["size"] = next(iter(sizes)) if sizes else (1, 1)
    gt = dict(im=np.asarray(gt["im"], np.int64), obj=np.asarray(gt["obj"], np.int64), pose=np.asarray(gt["pose"], np.float64).reshape(-1, 4, 4))
    return gt, images, keys, scene_dir, (infos or None)


def derive_scene(root, split, scene, models_dir, models, *, delta=15.0, depth=True, size=None, masks="dense", device=None):
    """``groundtruth.instance_ground_truth`` of every instance of one scene -> (result, keys [(im, j)], scene directory)."""
    from sam6d_amd import groundtruth
    gt, images, keys, d, _ = scene_inputs(root, split, scene, depth, size)
    load_models(root, models_dir, gt["obj"].tolist(), models)
    res = groundtruth.instance_ground_truth(models, gt, images, delta=delta, depth="measured" if depth else "rendered", masks=masks, device=device)
    return res, keys, d


def info_by_image(result, keys, box_rule="span"):
    """{im: [record of instance 0, 1, ...]}: the content of scene_gt_info.json."""
    from sam6d_amd import groundtruth
    out = {}
    for (im, j), rec in zip(keys, groundtruth.gt_info_records(result, box_rule)):
        assert len(out.setdefault(im, [])) == j
        out[im].append(rec)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--split", default="test")
    ap.add_argument("--scenes", nargs="+", default=None, help="scene numbers, separated by blanks or commas; default: every scene of the split")
    ap.add_argument("--models", default="models_eval")
    ap.add_argument("--delta", type=float, default=15.0)
    ap.add_argument("--no-depth", action="store_true", help="no depth images: visibility from the mutual occlusion of the annotated objects only")
    ap.add_argument("--size", default=None, help="H,W of the images, for --no-depth without rgb/ or gray/ images")
    ap.add_argument("--write", default="info,masks,models_info")
    ap.add_argument("--box-rule", default="span", choices=("span", "pixels"))
    ap.add_argument("--device", default=None, help="cuda (kernels) or cpu (the torch statements); default: cuda when there is one")
    ap.add_argument("--force", action="store_true", help="overwrite existing files")
    a = ap.parse_args(argv)
    from PIL import Image

    from sam6d_amd import groundtruth
    t0 = time.time()
    what = set(w for w in a.write.split(",") if w)
    if what - {"info", "masks", "models_info"}:
        raise ValueError(f"--write takes info, masks, models_info; got {a.write!r}")
    scenes = sorted({int(s) for part in a.scenes for s in part.split(",") if s}) if a.scenes else scene_ids(a.dataset, a.split)
    size = tuple(int(s) for s in a.size.split(",")) if a.size else None
    base = os.path.join(a.dataset, a.split) if os.path.isdir(os.path.join(a.dataset, a.split)) else a.dataset
    # nothing is written before every target is known to be free
    if not a.force:
        from bop_eval import walk_scenes
        taken = [os.path.join(a.dataset, a.models, "models_info.json")] if "models_info" in what else []
        taken += [os.path.join(base, f"{s:06d}", "scene_gt_info.json") for s in scenes] if "info" in what else []
        if "masks" in what:
            for _, im, d, records, _, _ in walk_scenes(a.dataset, a.split, scenes):
                taken += [os.path.join(d, sub, f"{im:06d}_{j:06d}.png") for sub in ("mask", "mask_visib") for j in range(len(records))]
        taken = [p for p in taken if os.path.exists(p)]
        if taken:
            raise FileExistsError(f"{taken[0]} exists ({len(taken)} target file(s) do): pass --force to overwrite")
    models, n_inst, n_im, n_skipped = {}, 0, 0, 0
    for scene in scenes:
        res, keys, d = derive_scene(a.dataset, a.split, scene, a.models, models, delta=a.delta, depth=not a.no_depth, size=size, device=a.device)
        n_inst, n_im, n_skipped = n_inst + len(keys), n_im + len({im for im, _ in keys}), n_skipped + int((res["skipped"] > 0).sum())
        if "info" in what:
            with open(os.path.join(d, "scene_gt_info.json"), "w") as f:
                json.dump({str(im): recs for im, recs in info_by_image(res, keys, a.box_rule).items()}, f)
        if "masks" in what:
            for sub in ("mask", "mask_visib"):
                os.makedirs(os.path.join(d, sub), exist_ok=True)
                dense = res[sub].cpu().numpy()
                for g, (im, j) in enumerate(keys):
                    Image.fromarray(dense[g] * np.uint8(255)).save(os.path.join(d, sub, f"{im:06d}_{j:06d}.png"))
    if "models_info" in what:
        info = {str(obj): groundtruth.model_info(models[obj]["vertices"], device=a.device) for obj in sorted(models)}
        with open(os.path.join(a.dataset, a.models, "models_info.json"), "w") as f:
            json.dump(info, f)
    out = dict(instances=n_inst, images=n_im, seconds=round(time.time() - t0, 3), skipped_instances=n_skipped)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
