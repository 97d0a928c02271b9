"""sam6d_amd.groundtruth on the host (no GPU): the torch statements against the restatement of tests/bopgt_ref.py, the
scene_gt_info.json records under both box rules, tools/bop_gt.py on a BOP-layout dataset written here, and --derive-gt of
tools/bop_eval.py and tools/coco_eval.py against the same tools on the dataset that tools/bop_gt.py filled in."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from sam6d_amd import evaluation as ev
from sam6d_amd import groundtruth as gtm
from sam6d_amd.ism import handoff
from sam6d_amd.pem import results
from tests import bopgt_ref as G
from tests import render_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 48, 64
CAM = np.array([60.0, 60.0, 32.0, 24.0], np.float32)
SCENE, IMS = 48, (3, 11)


def _models():
    v1, f1, _ = R.cube(40.0)
    v2, f2, _ = R.torus(8, 6)
    return {1: dict(vertices=v1, faces=f1), 2: dict(vertices=v2, faces=f2)}


@functools.lru_cache(maxsize=None)
def _dataset_once():
    """Two images: a torus in the middle with a cube behind it, a cube across the left border, a cube hidden behind a near plane
    -> (models, gt, images) in the layout of ``tools/bop_eval.load_dataset``; depths are multiples of 0.1 (the PNG's depth_scale)."""
    def at(u, v, z):
        return ((u - CAM[2]) / CAM[0] * z, (v - CAM[3]) / CAM[1] * z, z)
    where = [(0, 2, at(30.0, 22.0, 400.0)), (0, 1, at(34.0, 26.0, 560.0)), (0, 1, at(1.0, 20.0, 400.0)),
             (1, 1, at(20.0, 24.0, 400.0)), (1, 2, at(48.0, 20.0, 420.0)), (1, 1, at(40.0, 40.0, 500.0))]
    P = R.poses(len(where), seed=4).astype(np.float64)
    for n, (_, _, t) in enumerate(where):
        P[n, :3, 3] = np.round(np.array(t) * 16) / 16
    gt = dict(im=np.array([w[0] for w in where]), obj=np.array([w[1] for w in where]), pose=P)
    models, cams = _models(), np.stack([CAM, CAM + np.array([1.0, -1.0, 0.5, 0.25], np.float32)])
    depth = np.full((2, H, W), 700.0, np.float32)
    surf = _canvases(models, gt, dict(cams=cams), (0, 0))                  # the measured depth shows the objects themselves
    for i in range(2):
        z = np.where(surf[gt["im"] == i] > 0, surf[gt["im"] == i], np.inf).min(0)
        depth[i] = np.where(np.isfinite(z), np.rint(z * 10) / 10, depth[i])
    depth[0, :6, :10] = 0.0
    depth[1, 32:, 30:52] = 300.0                                           # in front of the last instance
    return models, gt, dict(cams=cams, depth=depth)


def _dataset():
    models, gt, images = _dataset_once()
    return models, dict(gt), dict(images)


def _canvases(models, gt, images, margin):
    mx, my = margin
    out = np.zeros((len(gt["im"]), H + 2 * my, W + 2 * mx), np.float32)
    for g in range(len(gt["im"])):
        m = models[int(gt["obj"][g])]
        cam = images["cams"][gt["im"][g]] + np.array([0, 0, mx, my], np.float32)
        out[g] = ev._render_depth_library(torch.from_numpy(m["vertices"]), torch.from_numpy(m["faces"]), torch.from_numpy(gt["pose"][g:g + 1].astype(np.float32)),
                                          torch.from_numpy(cam[None]), H + 2 * my, W + 2 * mx, 1.0)["depth"][0].numpy()
    return out


# ---------------------------------------------------------------------------------------------------------------- statements
@pytest.mark.parametrize("margin", [(0, 0), (W, H), (3, 2)])
def test_library_visibility_equals_the_restatement(margin):
    models, gt, images = _dataset()
    canvas = _canvases(models, gt, images, margin)
    ti, cams = gt["im"].astype(np.int32), images["cams"][gt["im"]]
    ref = G.gt_visibility(canvas, images["depth"], ti, cams, 15.0, margin, np.float32)
    r64 = G.gt_visibility(canvas, images["depth"], ti, cams, 15.0, margin, np.float64)
    assert not r64["undecided"].any() and (ref["counts"][:, 1] > 40).all() and (ref["counts"][:, 3] < ref["counts"][:, 1]).any()
    got = gtm._gt_visibility_library(torch.from_numpy(canvas), torch.from_numpy(images["depth"]), torch.from_numpy(ti), torch.from_numpy(cams), 15.0, margin)
    for k in ("mask", "mask_visib", "counts", "extents"):
        assert np.array_equal(got[k].numpy().astype(np.int64), ref[k].astype(np.int64)), k
    with pytest.raises(ValueError, match="test_index"):
        gtm._gt_visibility_library(torch.from_numpy(canvas), torch.from_numpy(images["depth"]), torch.from_numpy(ti) + 1, torch.from_numpy(cams), 15.0, margin)
    # the module on host tensors: the same, under any chunking and as run lists
    res = gtm.instance_ground_truth(models, gt, images, margin=margin, device="cpu")
    one = gtm.instance_ground_truth(models, gt, images, margin=margin, device="cpu", chunk_bytes=1)
    rle = gtm.instance_ground_truth(models, gt, images, margin=margin, device="cpu", chunk_bytes=1 << 18, masks="rle")
    assert isinstance(rle["mask"], handoff.RleMasks)
    rle = dict(rle, mask=rle["mask"].to_dense().to(torch.uint8), mask_visib=rle["mask_visib"].to_dense().to(torch.uint8))
    for r in (res, one, rle):
        assert np.array_equal(r["mask"].numpy(), ref["mask"]) and np.array_equal(r["mask_visib"].numpy(), ref["mask_visib"])
        assert np.array_equal(np.stack([r["px_count_all"], r["px_count_in_image"], r["px_count_valid"], r["px_count_visib"]], 1), ref["counts"])
        assert np.array_equal(r["visib_fract"], G.visib_fract(ref["counts"])) and (r["skipped"] == 0).all()
        assert np.array_equal(r["extents_obj"], ref["extents"][:, 0]) and not r["empty_obj"].any()
        assert np.array_equal(r["extents_visib"], np.where(ref["counts"][:, 3:4] == 0, -1, ref["extents"][:, 1]))
    if margin == (W, H):
        assert res["px_count_all"][2] > res["px_count_in_image"][2] and res["extents_obj"][2, 0] < 0          # across the border
    assert res["visib_fract"][5] < 0.1 < res["visib_fract"][1] < 0.9 < res["visib_fract"][0]


def test_rendered_depth_is_mutual_occlusion_only():
    models, gt, images = _dataset()
    margin = (3, 2)
    canvas = _canvases(models, gt, images, margin)
    win = canvas[:, 2:2 + H, 3:3 + W]
    test = np.zeros((2, H, W), np.float32)
    for i in range(2):
        z = np.where(win[gt["im"] == i] > 0, win[gt["im"] == i], np.inf).min(0)
        test[i] = np.where(np.isfinite(z), z, 0)
    ref = G.gt_visibility(canvas, test, gt["im"].astype(np.int32), images["cams"][gt["im"]], 15.0, margin, np.float32)
    for chunk in (1 << 30, 1):
        res = gtm.instance_ground_truth(models, gt, dict(cams=images["cams"], size=(H, W)), margin=margin, depth="rendered", device="cpu", chunk_bytes=chunk)
        assert np.array_equal(res["mask_visib"].numpy(), ref["mask_visib"]) and np.array_equal(res["px_count_visib"], ref["counts"][:, 3])
        assert np.array_equal(res["px_count_valid"], res["px_count_in_image"])
    assert res["px_count_visib"][0] == res["px_count_in_image"][0] and res["px_count_visib"][1] < res["px_count_in_image"][1]
    assert res["px_count_visib"][5] == res["px_count_in_image"][5]          # the plane that hid it is not an annotated object
    with pytest.raises(ValueError, match="depth must be"):
        gtm.instance_ground_truth(models, gt, images, depth="none")
    with pytest.raises(ValueError, match="margin must be"):
        gtm.instance_ground_truth(models, gt, images, margin=(-1, 0), device="cpu")


@pytest.mark.parametrize("V", [1, 2, 257, 1000])
def test_library_diameter_has_the_restatement_bits(V):
    v = np.random.RandomState(V).uniform(-60, 60, (V, 3)).astype(np.float32)
    want = G.diameter(v, np.float32)
    for chunk in (1 << 26, 16 * V * 7):
        got = gtm._model_diameter_library(torch.from_numpy(v), chunk_bytes=chunk).numpy()
        assert got.view(np.uint32)[0] == np.float32(want).view(np.uint32)
    info = gtm.model_info(v, device="cpu")
    assert info["diameter"] == float(want) and sorted(info) == ["diameter", "min_x", "min_y", "min_z", "size_x", "size_y", "size_z"]
    assert [info["min_x"], info["min_y"], info["min_z"]] == v.min(0).astype(np.float64).tolist()
    assert [info["size_x"], info["size_y"], info["size_z"]] == (v.max(0).astype(np.float64) - v.min(0).astype(np.float64)).tolist()
    assert abs(info["diameter"] - G.diameter(v, np.float64)) <= 4 * G.U * G.diameter(v, np.float64)
    bad = v.copy()
    bad[V // 2, 2] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        gtm.model_info(bad, device="cpu")


def test_gt_info_records_under_both_box_rules():
    res = dict(extents_obj=np.array([[-3, 10, 16, 29], [-1, -1, -1, -1], [5, 5, 5, 5]]), empty_obj=np.array([False, True, False]),
               extents_visib=np.array([[0, 10, 16, 29], [-1, -1, -1, -1], [-1, -1, -1, -1]]), empty_visib=np.array([False, True, True]),
               px_count_all=np.array([400, 0, 1]), px_count_valid=np.array([300, 0, 1]), px_count_visib=np.array([340, 0, 0]),
               visib_fract=np.array([0.85, 0.0, 0.0]))
    span, pixels = gtm.gt_info_records(res), gtm.gt_info_records(res, box_rule="pixels")
    assert span[0] == dict(bbox_obj=[-3, 10, 19, 19], bbox_visib=[0, 10, 16, 19], px_count_all=400, px_count_valid=300, px_count_visib=340, visib_fract=0.85)
    assert pixels[0]["bbox_obj"] == [-3, 10, 20, 20] and pixels[0]["bbox_visib"] == [0, 10, 17, 20]
    assert span[1]["bbox_obj"] == span[1]["bbox_visib"] == pixels[1]["bbox_obj"] == [-1, -1, -1, -1] and span[1]["visib_fract"] == 0.0
    assert span[2]["bbox_obj"] == [5, 5, 0, 0] and pixels[2]["bbox_obj"] == [5, 5, 1, 1] and span[2]["bbox_visib"] == [-1, -1, -1, -1]
    assert json.loads(json.dumps(span)) == span
    with pytest.raises(ValueError, match="box_rule"):
        gtm.gt_info_records(res, box_rule="xyxy")


# ---------------------------------------------------------------------------------------------------------------- the tools
def _write_ply(path, v, f):
    with open(path, "w") as fh:
        fh.write(f"ply\nformat ascii 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
                 f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
        fh.writelines(f"{a:.9g} {b:.9g} {c:.9g}\n" for a, b, c in v.tolist())
        fh.writelines(f"3 {a} {b} {c}\n" for a, b, c in f.tolist())


def _write_dataset(root):
    """The dataset of ``_dataset`` as files: PLY models, scene_gt.json, scene_camera.json, 16-bit depth PNGs (depth_scale 0.1);
    no scene_gt_info.json, no masks, no models_info.json."""
    from PIL import Image
    models, gt, images = _dataset()
    scene = root / "test" / f"{SCENE:06d}"
    (root / "models_eval").mkdir(parents=True)
    (scene / "depth").mkdir(parents=True)
    for obj, m in models.items():
        _write_ply(root / "models_eval" / f"obj_{obj:06d}.ply", m["vertices"], m["faces"])
    scene_gt = {str(im): [] for im in IMS}
    for g in range(len(gt["im"])):
        scene_gt[str(IMS[gt["im"][g]])].append({"cam_R_m2c": gt["pose"][g, :3, :3].reshape(-1).tolist(), "cam_t_m2c": gt["pose"][g, :3, 3].tolist(),
                                               "obj_id": int(gt["obj"][g])})
    (scene / "scene_gt.json").write_text(json.dumps(scene_gt))
    cams = {}
    for i, im in enumerate(IMS):
        fx, fy, cx, cy = (float(x) for x in images["cams"][i])
        cams[str(im)] = {"cam_K": [fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0], "depth_scale": 0.1}
        Image.fromarray(np.rint(images["depth"][i] * 10).astype(np.uint16)).save(scene / "depth" / f"{im:06d}.png")
    (scene / "scene_camera.json").write_text(json.dumps(cams))
    return models, gt, images, scene


def _tools():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bop_eval
    import bop_gt
    import coco_eval
    return bop_gt, bop_eval, coco_eval


def test_bop_gt_tool_writes_what_the_module_computes(tmp_path, capsys):
    from PIL import Image
    bop_gt = _tools()[0]
    root = tmp_path / "ds"
    models, gt, images, scene = _write_dataset(root)
    images["depth"] = (np.rint(images["depth"] * 10).astype(np.uint16).astype(np.float32) * np.float32(0.1))          # as the PNG gives it back
    out = bop_gt.main(["--dataset", str(root), "--device", "cpu"])
    line = capsys.readouterr().out.strip().splitlines()
    assert len(line) == 1 and json.loads(line[0]) == out
    assert out["instances"] == 6 and out["images"] == 2 and out["skipped_instances"] == 0 and sorted(out) == ["images", "instances", "seconds", "skipped_instances"]
    res = gtm.instance_ground_truth(models, gt, images, device="cpu")
    recs = gtm.gt_info_records(res)
    info = json.loads((scene / "scene_gt_info.json").read_text())
    assert sorted(info) == ["11", "3"] and info["3"] == recs[:3] and info["11"] == recs[3:]
    assert info["3"][2]["bbox_obj"][0] < 0 and info["11"][2]["visib_fract"] < 0.1
    g = 0
    for i, im in enumerate(IMS):
        for j in range(3):
            for sub in ("mask", "mask_visib"):
                png = np.asarray(Image.open(scene / sub / f"{im:06d}_{j:06d}.png"))
                assert png.dtype == np.uint8 and set(np.unique(png).tolist()) <= {0, 255} and np.array_equal(png, res[sub][g].numpy() * 255), (im, j, sub)
            g += 1
    minfo = json.loads((root / "models_eval" / "models_info.json").read_text())
    assert minfo == {str(obj): gtm.model_info(models[obj]["vertices"], device="cpu") for obj in (1, 2)}
    assert minfo["1"]["diameter"] == float(np.float32(np.sqrt(np.float32(19200.0)))) and minfo["1"]["size_x"] == 80.0
    # nothing is overwritten without --force, whichever part exists, and nothing is touched by the refusal
    before = (scene / "scene_gt_info.json").read_text()
    for write in ("info,masks,models_info", "info", "masks", "models_info"):
        with pytest.raises(FileExistsError, match="--force"):
            bop_gt.main(["--dataset", str(root), "--device", "cpu", "--write", write])
    assert (scene / "scene_gt_info.json").read_text() == before
    os.remove(scene / "scene_gt_info.json")
    with pytest.raises(FileExistsError, match="models_info.json"):
        bop_gt.main(["--dataset", str(root), "--device", "cpu"])
    assert not (scene / "scene_gt_info.json").exists()
    bop_gt.main(["--dataset", str(root), "--device", "cpu", "--scenes", str(SCENE), "--box-rule", "pixels", "--force"])
    pix = json.loads((scene / "scene_gt_info.json").read_text())
    assert pix["3"][0]["bbox_visib"][2:] == [recs[0]["bbox_visib"][2] + 1, recs[0]["bbox_visib"][3] + 1]
    # without depth images: the size from --size, visibility from the other objects only
    out = bop_gt.main(["--dataset", str(root), "--device", "cpu", "--no-depth", "--size", f"{H},{W}", "--write", "info", "--force"])
    nod = json.loads((scene / "scene_gt_info.json").read_text())
    assert nod["11"][2]["visib_fract"] == 1.0 and nod["3"][1]["visib_fract"] < 0.9 and nod["3"][0]["px_count_valid"] == nod["3"][0]["px_count_all"] - (
        res["px_count_all"][0] - res["px_count_in_image"][0])
    with pytest.raises(FileNotFoundError, match="--size"):
        bop_gt.main(["--dataset", str(root), "--device", "cpu", "--no-depth", "--write", "info", "--force"])


def _result_files(tmp_path, gt, res):
    """A pose result file (the ground truth, a little off) and a detection result file (the derived visible masks, shifted)."""
    rs = np.random.RandomState(0)
    lines = []
    for g in range(len(gt["im"])):
        P = gt["pose"][g].copy()
        P[:3, 3] += rs.uniform(-4, 4, 3)
        lines += results.bop_csv_lines(SCENE, IMS[gt["im"][g]], [int(gt["obj"][g])], np.float32([0.9 - 0.1 * g]), P[None, :3, :3], P[None, :3, 3] / 1000.0, 0.25)
    results.write_bop_csv(tmp_path / "poses.csv", lines)
    records = []
    for i, im in enumerate(IMS):
        sel = np.nonzero(gt["im"] == i)[0]
        masks = torch.roll(res["mask_visib"][sel].bool(), shifts=(1, -1), dims=(1, 2))
        boxes = torch.tensor([[float(v) for v in (e[0], e[1], e[2] + 1, e[3] + 1)] for e in res["extents_visib"][sel]])
        det = handoff.Detections(scene_id=SCENE, image_id=im, masks=masks, boxes=boxes, scores=torch.linspace(0.9, 0.5, len(sel)),
                                 object_ids=torch.as_tensor(gt["obj"][sel] - 1), runtime=0.125)
        records += handoff.detection_records(det, "ycbv")
    handoff.save_json_bop23(tmp_path / "dets.json", records)


def _line(out):
    return {k: v for k, v in out.items() if k != "seconds"}


def test_derive_gt_equals_the_tools_on_the_filled_in_dataset(tmp_path, capsys):
    """--derive-gt on the bare dataset prints what the same tool prints once tools/bop_gt.py has written the files (``seconds``
    aside); without the flag the bare dataset is refused as before."""
    bop_gt, bop_eval, coco_eval = _tools()
    root = tmp_path / "ds"
    models, gt, images, scene = _write_dataset(root)
    images["depth"] = (np.rint(images["depth"] * 10).astype(np.uint16).astype(np.float32) * np.float32(0.1))
    _result_files(tmp_path, gt, gtm.instance_ground_truth(models, gt, images, device="cpu"))
    poses, dets = ["--results", str(tmp_path / "poses.csv"), "--dataset", str(root), "--device", "cpu"], ["--results", str(tmp_path / "dets.json"),
                                                                                                           "--dataset", str(root), "--device", "cpu"]
    with pytest.raises(FileNotFoundError, match="scene_gt_info.json"):
        coco_eval.main(dets)
    with pytest.raises(FileNotFoundError, match="models_info.json"):
        bop_eval.main(poses)
    derived = dict(bop=bop_eval.main(poses + ["--derive-gt"]),
                   **{f"coco_{t}_{m}": coco_eval.main(dets + ["--derive-gt", "--iou-type", t, "--masks", m]) for t in ("segm", "bbox") for m in ("dense", "rle")})
    assert derived["bop"]["targets"] == 5 and 0.3 < derived["bop"]["AR"] <= 1.0          # the hidden instance is no target
    assert 0.2 < derived["coco_segm_dense"]["AP"] < 1.0 and derived["coco_bbox_dense"]["AP"] > 0.5
    assert not (scene / "scene_gt_info.json").exists() and not (scene / "mask_visib").exists() and not (root / "models_eval" / "models_info.json").exists()
    # only the masks are missing: they alone are derived
    bop_gt.main(["--dataset", str(root), "--device", "cpu", "--write", "info,models_info"])
    assert _line(coco_eval.main(dets + ["--derive-gt"])) == _line(derived["coco_segm_dense"])
    assert _line(coco_eval.main(dets + ["--derive-gt", "--masks", "rle"])) == _line(derived["coco_segm_dense"])
    bop_gt.main(["--dataset", str(root), "--device", "cpu", "--write", "masks"])
    capsys.readouterr()
    for flag in ([], ["--derive-gt"]):
        assert _line(bop_eval.main(poses + flag)) == _line(derived["bop"])
        for t in ("segm", "bbox"):
            for m in ("dense", "rle"):
                assert _line(coco_eval.main(dets + flag + ["--iou-type", t, "--masks", m])) == _line(derived[f"coco_{t}_{m}"]), (flag, t, m)
    assert _line(derived["coco_segm_rle"]) == _line(derived["coco_segm_dense"])
    # without scene_gt_info.json and without the flag the pose tool scores every ground truth, as before
    os.remove(scene / "scene_gt_info.json")
    assert bop_eval.main(poses)["targets"] == 6
