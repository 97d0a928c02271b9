"""PEM per-detection pre-processing on the device against the oracle's per-detection loop."""
import time

import numpy as np
import pytest
import torch

from oracle import pem_pre as opre
from sam6d_amd.pem import preprocess as pre
from sam6d_amd.utils import synth

pytestmark = pytest.mark.gpu

MEAN, STD = torch.tensor(pre.MEAN), torch.tensor(pre.STD)


# ---- bodies of the direct kernel tests: here with sam6d_amd.ops on the device, in tests/test_emu_pempre.py on the emulator ("cpu").
# Inputs and expected values are made on the host; only the call under test sees `dev`.
def _frame(P=8, seed=3):
    inp = synth.pem_pre_inputs(P=P, seed=seed)
    return inp, (torch.from_numpy(inp["image"]), inp["depth"], inp["K"], inp["masks"])


def mask_boxes_body(api, dev):
    """s6d_pem_mask_boxes_u8 against mask AND depth / count / square_boxes of the library path (itself pinned to the
    reference's get_bbox), incl. empty masks, masks touching the frame edge and a detection below the point threshold."""
    g = torch.Generator().manual_seed(4)
    P, H, W = 9, 48, 64
    masks = torch.zeros(P, H, W, dtype=torch.bool)
    for i, (y1, y2, x1, x2) in enumerate([(0, 48, 0, 64), (0, 5, 0, 64), (10, 40, 60, 64), (47, 48, 0, 1), (5, 45, 3, 9), (20, 21, 10, 50),
                                          (0, 0, 0, 0), (3, 44, 2, 63), (12, 30, 12, 30)]):
        masks[i, y1:y2, x1:x2] = torch.rand(y2 - y1, x2 - x1, generator=g) > 0.3
    depth = torch.rand(H, W, generator=g)
    depth[depth < 0.2] = 0.0
    m8, cnt, ok8, box = [t.cpu() for t in api.pem_mask_boxes(masks.view(torch.uint8).to(dev), depth.to(dev), 32)]
    m = masks & (depth > 0)[None]
    ok = m.flatten(1).sum(1) > 32
    assert torch.equal(m8.bool(), m) and torch.equal(cnt, m.flatten(1).sum(1)) and torch.equal(ok8.bool(), ok)
    assert 0 < int(ok.sum()) < P                                     # both kinds present
    assert torch.equal(box, pre.square_boxes(m | ~ok[:, None, None]))


def crops_library_body(api, dev):
    """s6d_pem_crops_f32 against preprocess._crops, value for value (same float32 operations in the same order)."""
    inp, (image, depth, K, masks) = _frame()
    m = masks & (depth > 0)[None]
    box = pre.square_boxes(m)
    kept = torch.tensor([6, 0, 2, 5])
    on_dev = [image.contiguous().to(dev), m.to(torch.uint8).to(dev), kept.to(dev), box.to(dev)]
    for flag in (True, False):
        want = pre._crops(image, m[kept].float(), box[kept], 224, flag)
        got = api.pem_crops(*on_dev, 224, flag, pre.MEAN, pre.STD).cpu()
        assert torch.equal(got, want), (got - want).abs().max()
    want = pre._crops(image, m[kept].float(), box[kept], 56, True)
    assert torch.equal(api.pem_crops(*on_dev, 56, True, pre.MEAN, pre.STD).cpu(), want)


def crops_cv2_body(api, dev):
    """s6d_pem_crops_f32 and preprocess._crops against oracle.pem_pre.cv2_resize_linear_u8 (cv2.resize INTER_LINEAR restated),
    value for value, at the ratios with their own code path: 1:1 (copy), exactly 2:1 (box mean), up- and down-scaling with odd
    sides, a crop touching the frame border."""
    S = 16
    H, W = 72, 80
    g = torch.Generator().manual_seed(11)
    image = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    sides = [16, 32, 7, 23, 48, 33, 5]
    box = torch.tensor([[y, y + n, x, x + n] for n, (y, x) in zip(sides, [(0, 0), (10, 20), (3, 70), (40, 5), (24, 32), (39, 47), (67, 75)])])
    m = torch.zeros(len(sides), H, W, dtype=torch.uint8)
    for i, (y1, y2, x1, x2) in enumerate(box.tolist()):
        m[i, y1:y2, x1:x2] = (torch.rand(y2 - y1, x2 - x1, generator=g) > 0.3).to(torch.uint8)
    kept = torch.arange(len(sides))
    for flag in (True, False):
        got = api.pem_crops(image.contiguous().to(dev), m.to(dev), kept.to(dev), box.to(dev), S, flag, pre.MEAN, pre.STD).cpu()
        lib = pre._crops(image, m, box, S, flag)
        assert torch.equal(got, lib)
        for i, (y1, y2, x1, x2) in enumerate(box.tolist()):
            rgb = image.numpy()[y1:y2, x1:x2, :][:, :, ::-1]
            if flag:
                rgb = rgb * (m[i].numpy()[y1:y2, x1:x2, None] > 0).astype(np.uint8)
            want = (opre.cv2_resize_linear_u8(rgb, S).astype(np.float32) / np.float32(255) - opre.MEAN) / opre.STD
            assert np.array_equal(got[i].numpy(), want.transpose(2, 0, 1)), (i, flag)


FILL = -7                                                                # what the compaction tests put into every output slot first
CAM = (57.5, 58.25, 31.5, 23.75)                                         # fx, fy, cx, cy


def _small_frame(boxes, seed):
    """A 48 x 64 frame: depth with holes, one mask AND depth > 0 per box (inside the frame's part of it)."""
    H, W = 48, 64
    g = torch.Generator().manual_seed(seed)
    depth = torch.rand(H, W, generator=g) + 0.5
    depth[torch.rand(H, W, generator=g) < 0.2] = 0.0
    m = torch.zeros(len(boxes), H, W, dtype=torch.uint8)
    for i, (y1, y2, x1, x2) in enumerate(boxes):
        m[i, y1:y2, x1:x2] = ((torch.rand(H, W, generator=g) > 0.4) & (depth > 0))[y1:y2, x1:x2].to(torch.uint8)
    return depth, m


def _compact(api, dev, m, depth, box, ok, cap):
    """s6d_pem_compact_cloud_f32 (the call of ops.pem_compact_cloud) into slots that hold FILL -> host (choose, cloud, n)."""
    P, H, W = m.shape
    choose = torch.full((P, cap), FILL, dtype=torch.int32).to(dev)
    cloud = torch.full((P, cap, 3), float(FILL)).to(dev)
    n = torch.full((P,), FILL, dtype=torch.int64).to(dev)
    ins = [m.to(dev), depth.to(dev), box.to(dev), ok.to(dev)]
    api._call("s6d_pem_compact_cloud_f32", *[api._ptr(t) for t in ins], P, H, W, *CAM, cap, api._ptr(choose), api._ptr(cloud), api._ptr(n),
              api._stream())
    return choose.cpu().numpy(), cloud.cpu().numpy(), n.cpu().tolist()


def _compacted(m, depth, box):
    """`mask -> choose -> cloud` of the reference for one detection: (choose, cloud)."""
    y1, y2, x1, x2 = box
    K = np.array([[CAM[0], 0, CAM[2]], [0, CAM[1], CAM[3]], [0, 0, 1]])
    choose = m.numpy()[y1:y2, x1:x2].astype(np.float32).flatten().nonzero()[0]
    return choose, opre.point_cloud(depth.numpy(), K)[y1:y2, x1:x2, :].reshape(-1, 3)[choose, :]


def _is_compacted(got, i, m, depth, box):
    choose, cloud, n = got
    want_choose, want_cloud = _compacted(m[i], depth, box)
    assert n[i] == len(want_choose) > 0
    np.testing.assert_array_equal(choose[i, :n[i]], want_choose)
    np.testing.assert_array_equal(cloud[i, :n[i]], want_cloud)
    assert (choose[i, n[i]:] == FILL).all() and (cloud[i, n[i]:] == FILL).all()


def _untouched(got, i):
    choose, cloud, n = got
    assert n[i] == 0 and (choose[i] == FILL).all() and (cloud[i] == FILL).all()


def compact_cloud_body(api, dev):
    """s6d_pem_compact_cloud_f32 alone against `mask[y1:y2, x1:x2].flatten().nonzero()` and the float32 back-projection in the
    reference's operation order: a 40 x 40 crop (1600 pixels: two chunks, the second partial, so the chunk carry and the wave prefix
    both count), a detection that is not ok, a 5 x 5 crop in the frame's corner."""
    boxes = [(3, 43, 10, 50), (0, 48, 8, 56), (43, 48, 59, 64)]
    depth, m = _small_frame(boxes, seed=21)
    m[1] = 0
    got = _compact(api, dev, m, depth, torch.tensor(boxes), torch.tensor([1, 0, 1], dtype=torch.uint8), cap=48 * 48)
    _is_compacted(got, 0, m, depth, boxes[0])
    assert got[0][0, :got[2][0]].max() >= 1024 > got[0][0, 0]          # kept pixels in both chunks
    _untouched(got, 1)
    _is_compacted(got, 2, m, depth, boxes[2])


def compact_guards_body(api, dev):
    """A box that does not lie inside the frame, or holds more pixels than a slot: n = 0, nothing written, the neighbour served."""
    boxes = [(5, 25, 30, 50), (0, 48 + 4, 0, 20)]
    depth, m = _small_frame(boxes, seed=22)
    got = _compact(api, dev, m, depth, torch.tensor(boxes), torch.ones(2, dtype=torch.uint8), cap=48 * 48)
    _is_compacted(got, 0, m, depth, boxes[0])
    _untouched(got, 1)
    boxes = [(20, 36, 40, 56), (2, 12, 3, 13)]                       # 16 x 16 = 256 > cap = 100 = 10 x 10
    depth, m = _small_frame(boxes, seed=23)
    got = _compact(api, dev, m, depth, torch.tensor(boxes), torch.ones(2, dtype=torch.uint8), cap=100)
    _untouched(got, 0)
    _is_compacted(got, 1, m, depth, boxes[1])


def crops_guard_body(api, dev):
    """A box that does not lie inside the frame: its crop is that of a black crop, (0 - mean) / std, and the neighbour is served."""
    boxes = [(5, 25, 30, 50), (0, 48 + 4, 0, 20)]
    depth, m = _small_frame(boxes, seed=24)
    image = torch.randint(0, 256, (48, 64, 3), generator=torch.Generator().manual_seed(24), dtype=torch.uint8)
    box, kept = torch.tensor(boxes), torch.tensor([1, 0])
    for flag in (True, False):
        got = api.pem_crops(image.to(dev), m.to(dev), kept.to(dev), box.to(dev), 16, flag, pre.MEAN, pre.STD).cpu()
        assert torch.equal(got[0], ((torch.zeros(3) - MEAN) / STD)[:, None, None].expand(3, 16, 16))
        assert torch.equal(got[1], pre._crops(image, m[:1], box[:1], 16, flag)[0])


def crop_resize_pad_guard_body(api, dev):
    """s6d_crop_resize_pad_f32 with a record whose y1 + h exceeds H: an output whose source pixel lies outside the frame is padding
    (rgb 0, mask 0), every other output is what the same record gives on a frame that has those rows."""
    from sam6d_amd.ism import dinov2 as pd
    H, W, T, extra = 48, 64, 16, 12
    g = torch.Generator().manual_seed(25)
    tall_image = torch.randint(1, 256, (H + extra, W, 3), generator=g, dtype=torch.uint8)
    tall_mask = torch.rand(1, H + extra, W, generator=g) + 0.25
    params = torch.from_numpy(pd.crop_params(np.array([[10, 30, 40, H + extra]]), T))          # xyxy: rows 30 .. 60, columns 10 .. 40
    rows = torch.arange(H + extra, dtype=torch.float32)[None, :, None].expand(1, H + extra, W).contiguous()
    src_row = api.crop_resize_pad(None, rows.to(dev), params.to(dev), T, pd.RGB_MEAN, pd.RGB_STD, rgb=False)[1].cpu()
    outside = src_row >= H
    assert outside.any() and (~outside).any()
    want_rgb, want_mask = [t.cpu() for t in api.crop_resize_pad(tall_image.to(dev), tall_mask.to(dev), params.to(dev), T, pd.RGB_MEAN, pd.RGB_STD)]
    rgb, mask = [t.cpu() for t in api.crop_resize_pad(tall_image[:H].contiguous().to(dev), tall_mask[:, :H].contiguous().to(dev), params.to(dev),
                                                      T, pd.RGB_MEAN, pd.RGB_STD)]
    assert want_mask[~outside].min() > 0 and want_rgb.abs().min() > 0          # (so that a zero below is the guard's)
    assert torch.equal(mask, torch.where(outside, torch.zeros(()), want_mask))
    assert torch.equal(rgb, torch.where(outside[:, None], torch.zeros(()), want_rgb))


BODIES = [mask_boxes_body, crops_library_body, crops_cv2_body, compact_cloud_body, compact_guards_body, crops_guard_body,
          crop_resize_pad_guard_body]


@pytest.mark.parametrize("body", BODIES, ids=lambda f: f.__name__[:-5])
def test_kernel_on_the_device(body):
    from sam6d_amd import ops
    body(ops, "cuda")


def test_batched_preprocessing_on_device_matches_oracle_loop():
    inp = synth.pem_pre_inputs(P=8, seed=3)
    kw = dict(radius=0.12, n_sample=2048, img_size=224, min_points=32, min_inliers=4, radius_factor=1.2)
    ref = opre.preprocess_frame(inp["image"], inp["depth"].numpy(), inp["K"].numpy(), inp["masks"].numpy(),
                                keys=inp["keys"].numpy(), **kw)
    out = pre.observed_inputs(torch.from_numpy(inp["image"]).cuda(), inp["depth"].cuda(), inp["K"], inp["masks"].cuda(),
                              keys=inp["keys"].cuda(), **kw)
    assert out["kept"].tolist() == ref["kept"].tolist()
    np.testing.assert_array_equal(out["bbox"].cpu().numpy(), ref["bbox"])
    np.testing.assert_array_equal(out["rgb_choose"].cpu().numpy(), ref["rgb_choose"])
    np.testing.assert_array_equal(out["pts"].cpu().numpy(), ref["pts"])
    np.testing.assert_array_equal(out["rgb"].cpu().numpy(), ref["rgb"])


def test_frame_of_many_detections_runs_in_milliseconds():
    inp = synth.pem_pre_inputs(P=64, seed=9)
    args = (torch.from_numpy(inp["image"]).cuda(), inp["depth"].cuda(), inp["K"], inp["masks"].cuda(), 0.15,
            inp["keys"].cuda())
    out = pre.observed_inputs(*args)
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(3):
        out = pre.observed_inputs(*args)
    torch.cuda.synchronize()
    ms = (time.time() - t0) / 3 * 1e3
    M = out["pts"].shape[0]
    assert M >= 48 and out["pts"].shape == (M, 2048, 3) and out["rgb"].shape == (M, 3, 224, 224)
    assert torch.isfinite(out["pts"]).all() and (out["rgb_choose"] >= 0).all() and (out["rgb_choose"] < 224 * 224).all()
    print(f"PEM pre-processing, 64 detections of one 480x640 frame: {ms:.1f} ms")
    assert ms < 200
