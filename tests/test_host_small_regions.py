"""The small-region clean-up without a GPU: the plain-loop restatement (tests/small_regions_ref.py) against a scipy statement of the
same definition, the torch library statement of sam6d_amd.sam.amg against the restatement on every pattern of the device tests,
``postprocess_small_regions`` and ``generate_proposals(min_mask_region_area=)`` on canned CPU proposals, the header constants and
the argument checks of the new entry points."""
import ctypes

import numpy as np
import pytest
import torch

from sam6d_amd import _lib, ops, policy
from sam6d_amd.sam import amg
from tests import small_regions_ref as R
from tests import test_gpu_small_regions as T


def test_restatement_agrees_with_the_scipy_statement_on_random_masks():
    """scipy.ndimage.label (3 x 3 structure) stands in for the cv2 labelling of the upstream function; its numbering follows the
    row-major scan, which is the tie rule of the definition.  Every combination of changed_h / changed_i must occur."""
    pytest.importorskip("scipy")
    rng = np.random.default_rng(11)
    seen = {}
    for k in range(400):
        H, W = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        mask = rng.random((H, W)) < rng.choice([0.15, 0.4, 0.6, 0.85, 0.97])
        min_area = int(rng.choice([1, 2, 3, 5, 9, 30]))
        got, ch, ci, _, _ = R.remove_small_regions_one(mask, min_area)
        m1, c1 = R.scipy_statement(mask, min_area, holes=True)
        m2, c2 = R.scipy_statement(m1, min_area, holes=False)
        assert np.array_equal(got != 0, m2) and (ch, ci) == (c1, c2), (k, H, W, min_area)
        seen[(ch, ci)] = seen.get((ch, ci), 0) + 1
    assert len(seen) == 4 and min(seen.values()) >= 20, seen


def test_tie_rule_and_strict_comparison_of_the_restatement():
    m = np.zeros((5, 9), np.uint8)
    m[3, 0:2] = 1                     # starts at index 27
    m[1, 5:7] = 1                     # starts at index 14: the earlier first pixel, although further right
    m[4, 8] = 1
    out, ch, ci, kept, tie = R.remove_small_regions_one(m, 50)
    assert (ch, ci, kept, tie) == (True, True, True, False) and out.all()  # the background, 40 pixels, is a hole below 50: one island of 45
    out, ch, ci, kept, tie = R.remove_small_regions_one(m, 3)
    assert (ch, ci, kept, tie) == (False, True, True, True) and out.sum() == 2 and out[1, 5] and out[1, 6]
    out, ch, ci, kept, tie = R.remove_small_regions_one(m, 2)
    assert (ch, ci, kept, tie) == (False, True, False, False) and out.sum() == 4          # area == min_area is not small
    assert R.remove_small_regions_one(m, 1)[1:3] == (False, False)


def test_inputs_reach_every_branch():
    """On the restatement's outputs: unchanged, holes only, islands only, both, keep-largest and the tie occur among the patterns of
    the device tests (the tiled shape), and the pattern that must give changed = True with equal pixels does."""
    seen = set()
    for a in T.min_areas(T.BIG):
        names, masks, (out, changed, boxes, branches) = T.case(T.BIG, a)
        for k, (ch, ci, kept, tie) in enumerate(branches):
            seen.add(("holes" if ch else "") + ("islands" if ci else "") or "unchanged")
            seen |= {"kept"} if kept else set()
            seen |= {"tie"} if tie else set()
            if a > T.BIG[0] * T.BIG[1]:
                continue                                            # (there the background is a small hole too: everything is set)
            if names[k] == "all small, one blob":
                assert changed[k] and np.array_equal(out[k], (masks[k] != 0).astype(np.uint8)) and not ch
            if names[k] == "all small, two equal":
                assert tie and kept
            if names[k] == "border hole":
                assert ch and out[k].all()
    assert seen == {"unchanged", "holes", "islands", "holesislands", "kept", "tie"}, seen


@pytest.mark.parametrize("hw", T.SHAPES)
def test_library_statement_vs_restatement_on_cpu_tensors(hw):
    for a in T.min_areas(hw):
        names, masks, ref = T.case(hw, a)
        m = torch.from_numpy(np.array(masks))
        T._same(amg.remove_small_regions(m if a % 2 else m != 0, a), ref, names, (hw, a))
    assert policy.library_branch_hits() == {}                      # CPU tensors: the library statement is not a recorded fall-back
    masks, labs = T.label_case(hw)
    for bg in (False, True):
        got = amg._min_index_labels_library(torch.from_numpy((np.array(masks) != 0) != bg))
        assert np.array_equal(got.numpy(), labs[bg])


def test_library_statement_on_empty_batches_and_bad_arguments():
    out, changed, boxes = amg.remove_small_regions(torch.zeros(0, 4, 6, dtype=torch.bool), 3)
    assert tuple(out.shape) == (0, 4, 6) and out.dtype == torch.uint8 and tuple(changed.shape) == (0,) and tuple(boxes.shape) == (0, 4)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="min_area"):
            amg.remove_small_regions(torch.zeros(1, 4, 6, dtype=torch.bool), bad)
    with pytest.raises(ValueError, match="bool or uint8"):
        amg.remove_small_regions(torch.zeros(1, 4, 6), 2)


def test_strict_policy_refuses_the_library_statement_on_device_tensors(monkeypatch):
    monkeypatch.setenv("S6D_DISABLE_FUSED", "small_regions")
    monkeypatch.setenv("S6D_STRICT", "1")
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    with pytest.raises(policy.StrictError, match="amg.remove_small_regions"):
        amg.remove_small_regions(torch.zeros(1, 4, 6, dtype=torch.bool), 2)


# ------------------------------------------------------------------------------------------------ canned proposals
H, W, MIN_AREA = 20, 24, 10


def _rect(y0, y1, x0, x1, extra=(), holes=()):
    m = np.zeros((H, W), bool)
    m[y0:y1 + 1, x0:x1 + 1] = True
    for y, x in extra:
        m[y, x] = True
    for y, x in holes:
        m[y, x] = False
    return m


def canned():
    """Five masks in the order (m1, m2, m0, m3, m4): m0, m4 clean; m1 = m0 + a speck; m2, m3 = one rectangle + a speck / with a
    pin-hole.  After the clean-up m1 duplicates m0 and m3 duplicates m2."""
    m0 = _rect(2, 9, 2, 9)
    m1 = _rect(2, 9, 2, 9, extra=[(18, 22)])
    m2 = _rect(12, 17, 12, 19, extra=[(0, 23)])
    m3 = _rect(12, 17, 12, 19, holes=[(14, 15)])
    m4 = _rect(12, 18, 0, 5)
    masks = np.stack([m1, m2, m0, m3, m4])
    return dict(masks=masks, boxes=np.array([R.box(m) for m in masks], np.int64),
                iou_preds=np.array([0.99, 0.98, 0.97, 0.96, 0.95], np.float32),
                stability_score=np.array([0.91, 0.92, 0.93, 0.94, 0.95], np.float32),
                points=np.arange(10, dtype=np.float64).reshape(5, 2))


def _tensors(d):
    return {k: torch.from_numpy(v.copy()) for k, v in d.items()}


def _equal_dicts(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == torch.from_numpy(np.asarray(want[k])).dtype and np.array_equal(got[k].numpy(), want[k]), k


def test_postprocess_small_regions_on_canned_proposals():
    src = canned()
    got = amg.postprocess_small_regions(_tensors(src), MIN_AREA, 0.7)
    # unchanged survivors first, in input order (m0, m4); m1 lost to m0; of the changed duplicates m2, m3 the earlier survives
    assert got["iou_preds"].tolist() == pytest.approx([0.97, 0.95, 0.98])
    assert got["stability_score"].tolist() == pytest.approx([0.93, 0.95, 0.92]) and got["points"].tolist() == [[4, 5], [8, 9], [2, 3]]
    assert got["boxes"].tolist() == [[2, 2, 9, 9], [0, 12, 5, 18], [12, 12, 19, 17]]           # m2's new box, not [12, 0, 23, 17]
    assert src["boxes"][1].tolist() == [12, 0, 23, 17]
    assert np.array_equal(got["masks"][2].numpy(), _rect(12, 17, 12, 19)) and got["masks"].dtype == torch.bool
    _equal_dicts(got, R.postprocess_small_regions(src, MIN_AREA, 0.7))
    # a threshold nothing exceeds keeps all five: the three changed ones after the two unchanged, each group in input order
    assert amg.postprocess_small_regions(_tensors(src), MIN_AREA, 1.0)["iou_preds"].tolist() == pytest.approx([0.97, 0.95, 0.99, 0.98, 0.96])
    # min_area = 1 changes nothing: NMS over the original boxes in input order
    _equal_dicts(amg.postprocess_small_regions(_tensors(src), 1, 0.7), R.postprocess_small_regions(src, 1, 0.7))
    empty = {k: v[:0] for k, v in _tensors(src).items()}
    assert amg.postprocess_small_regions(empty, MIN_AREA, 0.7) is empty


def _patched_generate(monkeypatch, **kw):
    """generate_proposals on the canned candidates: two prompt batches of (2, 3) candidates; the device NMS is replaced by the torch
    statement of the same rule (CPU tensors)."""
    src = canned()
    parts = [{k: torch.from_numpy(v[a:b].copy()) for k, v in src.items() if k != "points"} for a, b in ((0, 2), (2, 5))]
    parts[0]["point_index"], parts[1]["point_index"] = torch.tensor([0, 1]), torch.tensor([0, 0, 1])
    calls = []

    def fake_batch(pe, md, emb, pts, *a, **k):
        calls.append(pts)
        return dict(parts[len(calls) - 1])
    monkeypatch.setattr(amg, "process_point_batch", fake_batch)
    monkeypatch.setattr(ops, "nms", lambda b, s, t: amg._nms_library(b, s, t))
    out = amg.generate_proposals(None, None, torch.zeros(1, 4, 2, 2), (H, W), img_size=32, points_per_side=2, points_per_batch=2, **kw)
    grid = amg.build_point_grid(2) * [[W, H]]
    src["points"] = grid[[0, 1, 2, 2, 3]]
    assert len(calls) == 2
    return out, src


def test_generate_proposals_without_the_option_never_enters_it(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("remove_small_regions called with min_mask_region_area = 0")
    monkeypatch.setattr(amg, "remove_small_regions", boom)
    monkeypatch.setattr(amg, "postprocess_small_regions", boom)
    out, src = _patched_generate(monkeypatch)
    keep = R.nms(src["boxes"], src["iou_preds"], 0.7)
    assert keep == [0, 1, 2, 3, 4]                                  # the original boxes do not suppress each other
    _equal_dicts(out, {k: v[keep] for k, v in src.items()})
    out, _ = _patched_generate(monkeypatch, min_mask_region_area=0, crop_nms_thresh=0.1)
    _equal_dicts(out, {k: v[keep] for k, v in src.items()})


def test_generate_proposals_with_the_option_equals_the_restatement(monkeypatch):
    out, src = _patched_generate(monkeypatch, min_mask_region_area=MIN_AREA)
    keep = R.nms(src["boxes"], src["iou_preds"], 0.7)
    want = R.postprocess_small_regions({k: v[keep] for k, v in src.items()}, MIN_AREA, 0.7)
    _equal_dicts(out, want)
    assert out["masks"].shape[0] == 3 and out["boxes"].tolist() == [[2, 2, 9, 9], [0, 12, 5, 18], [12, 12, 19, 17]]
    # the threshold is max(box_nms_thresh, crop_nms_thresh): with crop_nms_thresh = 1 nothing is suppressed after the clean-up
    out, _ = _patched_generate(monkeypatch, min_mask_region_area=MIN_AREA, crop_nms_thresh=1.0)
    assert out["masks"].shape[0] == 5


def test_segmentor_class_names_where_the_option_lives():
    from sam6d_amd.ism import segmentor
    with pytest.raises(NotImplementedError, match=r"KeyError.*generate_proposals\(min_mask_region_area=\).*FramePipeline"):
        segmentor.CustomSamAutomaticMaskGenerator(None, min_mask_region_area=10)
    assert "KeyError" in segmentor.__doc__ and "generate_proposals(min_mask_region_area=)" in segmentor.__doc__


# ------------------------------------------------------------------------------------------------ header and entry points
def test_header_constants_and_argument_checks_without_a_gpu():
    th, tw = _lib.header_constant("S6D_CCL_TILE_H"), _lib.header_constant("S6D_CCL_TILE_W")
    assert th >= 1 and tw == 64 and ops.CCL_TILE == (th, tw) and ops.SMALL_REGIONS_WORKSPACE_BYTES >= 2 * 4 * 480 * 640
    L = _lib.lib()
    p, lng = ctypes.c_void_p(4096), ctypes.c_long
    size = L.s6d_small_regions_workspace_bytes
    assert size(1, 480, 640) >= 2 * 4 * 480 * 640 and size(3, 5, 7) >= 3 * size(1, 5, 7) - 16 and size(0, 5, 7) >= 0
    assert size(1, 65536, 32768) == -1 and size(1, 0, 7) == -1 and size(-1, 5, 7) == -1
    rm, lab = L.s6d_remove_small_regions_u8, L.s6d_label_components_u8
    assert rm(None, 2, 5, 7, lng(3), None, None, None, None, None) == -1
    for k in (0, 5, 6, 7, 8):                                     # each operand NULL in turn
        args = [p, 2, 5, 7, lng(3), p, p, p, p, None]
        args[k] = None
        assert rm(*args) == -1, k
    assert rm(None, 0, 5, 7, lng(3), None, None, None, None, None) == 0                      # N = 0: nothing to do
    assert rm(p, 2, 0, 7, lng(3), p, p, p, p, None) == -1 and rm(p, 2, 5, -1, lng(3), p, p, p, p, None) == -1
    assert rm(p, -1, 5, 7, lng(3), p, p, p, p, None) == -1
    assert rm(p, 2, 5, 7, lng(0), p, p, p, p, None) == -1                                     # min_area < 1
    assert rm(p, 1, 65536, 32768, lng(3), p, p, p, p, None) == -1                             # H W = 2^31
    assert lab(None, 2, 5, 7, 0, None, None, None) == -1 and lab(None, 0, 5, 7, 1, None, None, None) == 0
    assert lab(p, 2, 5, 7, 2, p, p, None) == -1 and lab(p, 2, 0, 7, 0, p, p, None) == -1
    assert lab(p, 1, 65536, 32768, 0, p, p, None) == -1
