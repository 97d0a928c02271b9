"""Run-length masks on the host: the restatement itself, ``handoff.RleMasks`` on CPU tensors (the torch statements of
sam6d_amd/ism/handoff.py), the readers of result files with ``masks="rle"``, ``coco_scores`` from run lists, tools/coco_eval.py
--masks rle and the ``detections_from_records`` round trip.  Everything is `equal`."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from sam6d_amd import evaluation as ev
from sam6d_amd import ops, policy
from sam6d_amd.ism import handoff
from tests import rle_ref as R
from tests import test_gpu_rle as T
from tests import test_host_coco_eval as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_on_hand_made_masks():
    assert R.encode([[0, 0], [0, 0]]) == [4] and R.encode([[1, 1], [1, 1]]) == [0, 4]
    m = [[0, 1, 1], [1, 0, 1]]                                             # column-major: 0 1 | 1 0 | 1 1
    assert R.encode(m) == [1, 2, 1, 2]
    assert R.decode([1, 2, 1, 2], 2, 3) == m and R.decode([1, 0, 0, 2, 1, 2, 0], 2, 3) == m
    assert R.packed(m) == ([0b101110], 4)                                  # row-major bits: pixels 1, 2, 3, 5
    assert R.check([], 2, 3) == "empty" and R.check([7, -1], 2, 3) == "negative" and R.check([5], 2, 3) == "sum" and R.check([6], 2, 3) is None
    big = [[1] * 70]
    words, area = R.packed(big)
    assert area == 70 and words == [(1 << 64) - 1, 0b111111] and R.signed64(words[0]) == -1


@pytest.mark.parametrize("hw", T.SHAPES)
def test_rle_masks_on_cpu_tensors(hw):
    """The library statements: the same lists as ``masks_to_rle`` and the restatement, the same words as the restatement, the input
    back as pixels; row selection; ``to_records``."""
    names, masks, lists, ref_words, ref_areas = T.patterns(hw)
    H, W = hw
    for t in (torch.from_numpy(masks != 0), torch.from_numpy(masks * np.uint8(200))):
        rle = handoff.RleMasks.from_masks(t)
        assert rle.counts.dtype == torch.int32 and rle.offsets.dtype == torch.int64 and len(rle) == len(names) and rle.size == hw
        recs = rle.to_records()
        assert recs == handoff.masks_to_rle(t) and [r["counts"] for r in recs] == lists
        packed, area = rle.packed()
        assert np.array_equal(packed.numpy(), ref_words) and np.array_equal(area.numpy(), ref_areas) and area.dtype == torch.int32
        assert torch.equal(rle.to_dense(), torch.from_numpy(masks != 0))
    assert not policy.library_branch_hits()                                # CPU tensors: the library statement is the path
    # row selection: bool, index array with repeats and negatives, list, slice
    n = len(names)
    keep = np.arange(n) % 3 != 1
    idx = np.array([n - 1, 0, 0, -2, n // 2])
    for sel, rows in ((keep, np.nonzero(keep)[0]), (torch.from_numpy(keep), np.nonzero(keep)[0]), (idx, idx % n), (torch.from_numpy(idx), idx % n),
                      ([1, 0], [1, 0]), (slice(1, None, 2), np.arange(n)[1::2]), ([], [])):
        part = rle[sel]
        assert len(part) == len(rows) and part.to_records() == [recs[k] for k in rows]
        assert part.offsets[0] == 0 and int(part.offsets[-1]) == part.counts.shape[0]
    with pytest.raises(IndexError):
        rle[[n]]
    with pytest.raises(IndexError):
        rle[np.ones(n + 1, bool)]
    both = handoff.RleMasks.cat([rle[keep], rle[~keep]])
    assert both.to_records() == [recs[k] for k in np.nonzero(keep)[0]] + [recs[k] for k in np.nonzero(~keep)[0]]


def test_library_decoders_accept_and_refuse_what_the_kernels_do():
    hw = T.BANDS
    H, W = hw
    _, _, lists, _, _ = T.patterns(hw)
    cases = T.noncanonical(lists, hw)
    a, b = handoff.RleMasks(*T._flat([x for x, _ in cases], "cpu"), hw), handoff.RleMasks(*T._flat([y for _, y in cases], "cpu"), hw)
    assert torch.equal(a.to_dense(), b.to_dense()) and all(torch.equal(x, y) for x, y in zip(a.packed(), b.packed()))
    assert a.to_dense()[4].numpy().astype(int).tolist() == R.decode(cases[4][0], H, W)
    good = [[H * W], [0, H * W], [3, 4, H * W - 7]]
    for what, bad in T.refused(hw):
        assert R.check(bad, H, W) is not None, what
        for at in (0, 2, 3):
            rle = handoff.RleMasks(*T._flat(good[:at] + [bad] + good[at:], "cpu"), hw)
            for fn in (rle.to_dense, rle.packed):
                with pytest.raises(ValueError, match=rf"mask {at}\b"):
                    fn()


def test_ops_refuse_cpu_tensors():
    m = torch.zeros(1, 4, 4, dtype=torch.uint8)
    c, o = torch.tensor([16], dtype=torch.int32), torch.tensor([0, 1])
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.rle_encode(m)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.rle_to_packed(c, o, 4, 4)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.rle_to_masks(c, o, 4, 4)
    for name in ("rle_encode", "rle_to_packed", "rle_to_masks"):
        assert ops.have(name)
    assert 1 <= ops.RLE_BAND_WORDS * 8 <= 64 * 1024                        # a band is static LDS


def test_from_records_is_one_flat_array_and_refuses_what_it_cannot_read():
    recs = C._records()
    rle = handoff.RleMasks.from_records([r["segmentation"] for r in recs])
    assert rle.size == C.HW and rle.to_records() == [r["segmentation"] for r in recs]
    assert rle.counts.dtype == torch.int32 and rle.offsets.tolist() == np.concatenate([[0], np.cumsum([len(r["segmentation"]["counts"]) for r in recs])]).tolist()
    with pytest.raises(ValueError, match="share one size"):
        handoff.RleMasks.from_records([recs[0]["segmentation"], {"counts": [6], "size": [2, 3]}])
    with pytest.raises(ValueError, match="COMPRESSED RLE string"):
        handoff.RleMasks.from_records([recs[0]["segmentation"], {"counts": "PPYo1", "size": list(C.HW)}])
    with pytest.raises(ValueError, match="32 bits"):
        handoff.RleMasks.from_records([{"counts": [2 ** 31], "size": [2, 3]}])
    empty = handoff.RleMasks.from_records([], size=(4, 5))
    assert len(empty) == 0 and empty.size == (4, 5) and tuple(empty.to_dense().shape) == (0, 4, 5)
    with pytest.raises(ValueError):
        handoff.RleMasks.from_records([])


def test_read_bop_json_as_run_lists_equals_the_dense_reader(tmp_path):
    records = C._records()
    handoff.save_json_bop23(tmp_path / "r.json", records)
    dense, rle = ev.read_bop_json(tmp_path / "r.json"), ev.read_bop_json(tmp_path / "r.json", masks="rle")
    assert sorted(dense) == sorted(rle)
    for k in dense:
        if k != "masks":
            assert np.array_equal(dense[k], rle[k]) and dense[k].dtype == rle[k].dtype, k
    assert isinstance(rle["masks"], handoff.RleMasks) and rle["masks"].counts.device.type == "cpu"
    assert np.array_equal(rle["masks"].to_dense().numpy(), dense["masks"])
    assert rle["masks"].to_records() == [r["segmentation"] for r in records]
    d = ev.detections_from_records(records, masks="rle")
    assert isinstance(d["masks"], handoff.RleMasks) and np.array_equal(d["im"], ev.detections_from_records(records)["im"])
    (tmp_path / "empty.json").write_text("[]")
    assert ev.read_bop_json(tmp_path / "empty.json", masks="rle")["masks"] is None
    records[1]["segmentation"] = {"counts": "PPYo1", "size": list(C.HW)}
    handoff.save_json_bop23(tmp_path / "c.json", records)
    with pytest.raises(ValueError, match="COMPRESSED RLE string"):
        ev.read_bop_json(tmp_path / "c.json", masks="rle")
    with pytest.raises(ValueError, match="masks"):
        ev.read_bop_json(tmp_path / "r.json", masks="packed")


def _gt_arrays():
    gts = C._ground_truth()
    return dict(im=np.array([x["im"] for x in gts]), category=np.array([x["cat"] for x in gts]), masks=np.stack([x["mask"] for x in gts]),
                bbox=np.array([x["box"] for x in gts]), ignore=np.array([x["ignore"] for x in gts]))


def test_coco_scores_from_run_lists_equal_the_dense_result_on_the_host():
    records, g = C._records(), _gt_arrays()
    want = ev.coco_scores(records, g, "segm", device="cpu")
    assert 0 < want["AP"] < 1
    d_dense, d_rle = ev.detections_from_records(records), ev.detections_from_records(records, masks="rle")
    g_rle = dict(g, masks=handoff.RleMasks.from_masks(torch.from_numpy(g["masks"])))
    assert ev.coco_scores(d_dense, g, "segm", device="cpu") == want
    assert ev.coco_scores(d_rle, g, "segm", device="cpu") == want
    assert ev.coco_scores(d_dense, g_rle, "segm", device="cpu") == want
    assert ev.coco_scores(d_rle, g_rle, "segm", device="cpu") == want
    assert ev.coco_scores(d_rle, g_rle, "bbox", device="cpu") == ev.coco_scores(records, g, "bbox", device="cpu")
    T.check_coco_scores(None, "cpu")
    with pytest.raises(ValueError, match="ground-truth masks"):
        ev.coco_scores(d_rle, dict(g, masks=np.zeros((5, 4, 4), bool)), "segm", device="cpu")


def test_coco_eval_tool_with_run_lists_equals_dense(tmp_path, capsys, monkeypatch):
    """tools/coco_eval.py --masks rle against --masks dense on a BOP-layout directory written here, the ground truth encoded in
    chunks of two PNGs."""
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import coco_eval
    gts, records = C._ground_truth(), C._records()
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
    handoff.save_json_bop23(tmp_path / "r.json", records + [dict(records[0], image_id=77)])
    monkeypatch.setattr(coco_eval, "RLE_CHUNK", 2)
    for iou_type in ("segm", "bbox"):
        args = ["--results", str(tmp_path / "r.json"), "--dataset", str(tmp_path / "ds"), "--iou-type", iou_type, "--device", "cpu"]
        dense = coco_eval.main(args + ["--masks", "dense"])
        rle = coco_eval.main(args + ["--masks", "rle"])
        lines = capsys.readouterr().out.strip().splitlines()
        assert len(lines) == 2 and json.loads(lines[1]) == rle
        assert dense["dropped_detections"] == 1 and dense["ground_truths"] == 5 and dense["AP"] > 0
        assert {k: v for k, v in rle.items() if k != "seconds"} == {k: v for k, v in dense.items() if k != "seconds"}
    gt, _ = coco_eval.load_ground_truth(str(tmp_path / "ds"), "test", {48}, masks="rle", device="cpu")
    assert isinstance(gt["masks"], handoff.RleMasks) and len(gt["masks"]) == 5


def test_detections_from_records_round_trip():
    frames = C._frames()
    for dataset, ids in (("ycbv", None), ("lmo", [torch.tensor([0, 7, 3]), torch.tensor([2, 2])])):
        if ids is not None:
            for f, i in zip(frames, ids):
                f.object_ids = i
        records = [r for f in frames for r in handoff.detection_records(f, dataset)]
        back = handoff.detections_from_records(records, device="cpu", dataset_name=dataset)
        assert len(back) == len(frames)
        for f, b in zip(frames, back):
            assert (b.scene_id, b.image_id, b.runtime) == (f.scene_id, f.image_id, f.runtime) and len(b) == len(f)
            assert b.masks.dtype == torch.bool and torch.equal(b.masks, f.masks)
            assert torch.equal(b.object_ids, f.object_ids) and torch.equal(b.scores, f.scores) and b.scores.dtype == torch.float32
            assert torch.equal(b.boxes, f.boxes)                            # (these boxes are exact in binary: x + (x2 - x) == x2)
            assert handoff.detection_records(b, dataset) == handoff.detection_records(f, dataset)
    assert handoff.detections_from_records([], device="cpu") == []
    with pytest.raises(ValueError, match="LM-O"):
        handoff.detections_from_records([dict(records[0], category_id=2)], device="cpu", dataset_name="lmo")
    # frames come back in the order the file first names them, also when their records are interleaved
    mixed = [records[3], records[0], records[4], records[1], records[2]]
    back = handoff.detections_from_records(mixed, device="cpu", dataset_name="lmo")
    assert [(b.image_id, len(b)) for b in back] == [(11, 2), (3, 3)]
