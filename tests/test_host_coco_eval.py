"""sam6d_amd.evaluation's COCO AP on the host (no GPU): the result-file reader against what ism.handoff writes, the refusal of
compressed RLE, the library statements against the restatement of tests/coco_ref.py, and tools/coco_eval.py on a BOP-layout
dataset written here."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from sam6d_amd import evaluation as ev
from sam6d_amd.ism import handoff
from tests import coco_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = (40, 56)


def _rect(y, x, h, w):
    m = np.zeros(HW, bool)
    m[y:y + h, x:x + w] = True
    return m


def _frames():
    """Two frames of detections as the ISM hands them over: XYXY boxes with fractional parts, zero-based object ids."""
    a = handoff.Detections(scene_id=48, image_id=3, masks=torch.from_numpy(np.stack([_rect(2, 3, 10, 12), _rect(20, 30, 8, 9), _rect(0, 0, 5, 5)])),
                           boxes=torch.tensor([[3.0, 2.0, 14.5, 11.25], [30.0, 20.0, 38.0, 27.0], [0.0, 0.0, 4.0, 4.0]]),
                           scores=torch.tensor([0.75, 0.5, 0.25]), object_ids=torch.tensor([0, 1, 0]), runtime=0.125)
    b = handoff.Detections(scene_id=48, image_id=11, masks=torch.from_numpy(np.stack([_rect(5, 6, 20, 20), np.zeros(HW, bool)])),
                           boxes=torch.tensor([[6.0, 5.0, 25.0, 24.0], [1.0, 1.0, 2.0, 2.0]]), scores=torch.tensor([0.875, 0.125]),
                           object_ids=torch.tensor([1, 1]), runtime=0.25)
    return [a, b]


def _records():
    return [r for f in _frames() for r in handoff.detection_records(f, "ycbv")]


def test_read_bop_json_round_trips_detection_records(tmp_path):
    frames, records = _frames(), _records()
    handoff.save_json_bop23(tmp_path / "r.json", records)
    back = ev.read_bop_json(tmp_path / "r.json")
    assert back["scene"].tolist() == [48] * 5 and back["im"].tolist() == [3, 3, 3, 11, 11] and back["category"].tolist() == [1, 2, 1, 2, 2]
    assert back["score"].tolist() == [0.75, 0.5, 0.25, 0.875, 0.125] and back["time"].tolist() == [0.125] * 3 + [0.25] * 2
    assert back["bbox"].tolist() == [[3.0, 2.0, 11.5, 9.25], [30.0, 20.0, 8.0, 7.0], [0.0, 0.0, 4.0, 4.0], [6.0, 5.0, 19.0, 19.0], [1.0, 1.0, 1.0, 1.0]]
    assert back["masks"].dtype == bool and np.array_equal(back["masks"], torch.cat([f.masks for f in frames]).numpy())
    # the same detections straight from the hand-off objects: no RLE round trip
    direct = ev.detections_from_handoff(frames)
    assert np.array_equal(direct["im"], np.stack([back["scene"], back["im"]], 1)) and np.array_equal(direct["category"], back["category"])
    assert np.array_equal(direct["bbox"], back["bbox"]) and np.array_equal(direct["score"], back["score"])
    assert torch.equal(direct["masks"], torch.from_numpy(back["masks"]))
    (tmp_path / "empty.json").write_text("[]")
    assert ev.read_bop_json(tmp_path / "empty.json")["masks"] is None and len(ev.read_bop_json(tmp_path / "empty.json")["score"]) == 0


def test_compressed_rle_is_refused(tmp_path):
    records = _records()
    records[1]["segmentation"] = {"counts": "PPYo1", "size": list(HW)}
    handoff.save_json_bop23(tmp_path / "c.json", records)
    with pytest.raises(ValueError, match="COMPRESSED RLE string"):
        ev.read_bop_json(tmp_path / "c.json")
    (tmp_path / "d.json").write_text("{}")
    with pytest.raises(ValueError, match="JSON list"):
        ev.read_bop_json(tmp_path / "d.json")


def _ground_truth():
    """Two images, two objects, one barely visible instance (ignored)."""
    rows = [(3, 1, _rect(2, 4, 10, 12), 1.0), (3, 2, _rect(21, 30, 8, 9), 0.8), (11, 2, _rect(5, 5, 20, 21), 0.9), (11, 2, _rect(30, 40, 3, 3), 0.02),
            (11, 1, _rect(0, 30, 6, 6), 0.6)]
    out = []
    for im, obj, m, visib in rows:
        ys, xs = np.nonzero(m)
        out.append(dict(im=(48, im), cat=obj, mask=m, box=(float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)),
                        ignore=visib < 0.1, visib=visib))
    return out


def _ref_dets(records):
    return [dict(im=(r["scene_id"], r["image_id"]), cat=r["category_id"], score=r["score"], mask=handoff.rle_to_mask(r["segmentation"]),
                 box=tuple(r["bbox"])) for r in records]


@pytest.mark.parametrize("iou_type", ["segm", "bbox"])
def test_library_route_equals_restatement_on_the_host(iou_type):
    """CPU tensors take the torch statements; records, hand-off objects and plain arrays are the same detections."""
    records, gts = _records(), _ground_truth()
    ref = C.coco_scores(_ref_dets(records), gts, iou_type)
    assert 0 < ref["AP"] < 1 and ref["ignored"] == 1 and ref["groups"] == 4
    g = dict(im=np.array([x["im"] for x in gts]), category=np.array([x["cat"] for x in gts]), masks=np.stack([x["mask"] for x in gts]),
             bbox=np.array([x["box"] for x in gts]), ignore=np.array([x["ignore"] for x in gts]))
    assert ev.coco_scores(records, g, iou_type, device="cpu") == ref
    assert ev.coco_scores(_frames(), g, iou_type, device="cpu") == ref
    with pytest.raises(ValueError, match="iou_type"):
        ev.coco_scores(records, g, "keypoints")


def test_coco_eval_tool_on_a_two_image_dataset(tmp_path, capsys):
    """tools/coco_eval.py --device cpu on a dataset built here: scene_gt.json, scene_gt_info.json with one instance below 0.1 visible,
    mask_visib PNGs; a result file with one detection in an image the dataset does not have.  Equal to the restatement."""
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import coco_eval
    gts, records = _ground_truth(), _records()
    scene = tmp_path / "ds" / "test" / "000048"
    (scene / "mask_visib").mkdir(parents=True)
    scene_gt, scene_info = {"3": [], "11": []}, {"3": [], "11": []}
    for x in gts:
        im = str(x["im"][1])
        Image.fromarray(x["mask"].astype(np.uint8) * 255).save(scene / "mask_visib" / f"{int(im):06d}_{len(scene_gt[im]):06d}.png")
        scene_gt[im].append({"cam_R_m2c": np.eye(3).reshape(-1).tolist(), "cam_t_m2c": [0.0, 0.0, 500.0], "obj_id": x["cat"]})
        scene_info[im].append({"bbox_visib": [int(v) for v in x["box"]], "visib_fract": x["visib"]})
    (scene / "scene_gt.json").write_text(json.dumps(scene_gt))
    (scene / "scene_gt_info.json").write_text(json.dumps(scene_info))
    (scene / "scene_camera.json").write_text(json.dumps({im: {"cam_K": [500.0, 0.0, 28.0, 0.0, 500.0, 20.0, 0.0, 0.0, 1.0], "depth_scale": 1.0}
                                                         for im in scene_gt}))
    stray = dict(records[0], image_id=77)
    handoff.save_json_bop23(tmp_path / "r.json", records + [stray])
    for iou_type in ("segm", "bbox"):
        ref = C.coco_scores(_ref_dets(records), gts, iou_type)
        out = coco_eval.main(["--results", str(tmp_path / "r.json"), "--dataset", str(tmp_path / "ds"), "--iou-type", iou_type, "--device", "cpu"])
        line = capsys.readouterr().out.strip().splitlines()
        assert len(line) == 1 and json.loads(line[0]) == out
        assert out["images"] == 2 and out["dropped_detections"] == 1 and out["ignored"] == 1 and out["ground_truths"] == 5
        assert {k: out[k] for k in ref} == ref, (iou_type, out, ref)
