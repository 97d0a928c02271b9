"""Times of the COCO AP evaluation on the GPU (profiles/coco_eval.md):

python tools/coco_eval_times.py [--images 200] [--dets 100] [--gts 15] [--hw 480 640] [--repeats 5] [--out FILE]

A seeded set: per image one object with ``gts`` instances (rectangles) and ``dets`` detections (jittered copies and strays), dense
masks on the device.  Measured: ``evaluation.coco_scores`` (segm) on the kernel route and on the library route (host clock around the
call, which ends in device-to-host copies; the first call of each route is a warm-up and is not counted), the two results compared;
then the kernels alone (device events around ``repeats`` launches after a warm-up), with the bytes each must move.  Prints one JSON
line.  There is no CPU path: without a GPU this fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def make_set(images, dets, gts, hw, device, seed=0):
    import torch
    H, W = hw
    g = torch.Generator(device="cpu").manual_seed(seed)
    ys, xs = torch.arange(H, device=device)[None, :, None], torch.arange(W, device=device)[None, None, :]

    def rects(b):                                                            # (n,4) y x h w -> (n,H,W) bool
        b = b.to(device)[:, :, None, None]
        return (ys >= b[:, 0]) & (ys < b[:, 0] + b[:, 2]) & (xs >= b[:, 1]) & (xs < b[:, 1] + b[:, 3])
    gm, dm, gbox, dbox, score = [], [], [], [], []
    for _ in range(images):
        h, w = torch.randint(8, H // 3, (gts,), generator=g), torch.randint(8, W // 3, (gts,), generator=g)
        y, x = (torch.rand(gts, generator=g) * (H - h)).long(), (torch.rand(gts, generator=g) * (W - w)).long()
        gb = torch.stack([y, x, h, w], 1)
        src = torch.randint(0, gts, (dets,), generator=g)
        db = gb[src] + torch.randint(-2, 3, (dets, 4), generator=g)
        db[:, 2:] = db[:, 2:].clamp(min=2)
        db[:, :2] = db[:, :2].clamp(min=0)
        gm.append(rects(gb))
        dm.append(rects(db))
        gbox.append(gb[:, [1, 0, 3, 2]].double())
        dbox.append(db[:, [1, 0, 3, 2]].double() + 0.25)
        score.append(torch.rand(dets, generator=g).double())
    im_d, im_g = np.repeat(np.arange(images), dets), np.repeat(np.arange(images), gts)
    det = dict(im=im_d, category=np.ones_like(im_d), score=torch.cat(score).numpy(), masks=torch.cat(dm), bbox=torch.cat(dbox).numpy())
    gt = dict(im=im_g, category=np.ones_like(im_g), masks=torch.cat(gm), bbox=torch.cat(gbox).numpy(),
              ignore=(np.arange(len(im_g)) % 7 == 3))
    return det, gt


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--gts", type=int, default=15)
    ap.add_argument("--hw", type=int, nargs=2, default=(480, 640))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch

    from sam6d_amd import evaluation, ops, policy
    if not torch.cuda.is_available():
        raise SystemExit("coco_eval_times: needs a GPU")
    dev = torch.device("cuda")
    det, gt = make_set(a.images, a.dets, a.gts, tuple(a.hw), dev)
    torch.cuda.synchronize()

    def scores(iou_type, n):
        times, res = [], None
        for k in range(n + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = evaluation.coco_scores(det, gt, iou_type, device=dev)
            torch.cuda.synchronize()
            if k:
                times.append(time.perf_counter() - t0)
        return res, times
    out = dict(images=a.images, dets_per_image=a.dets, gts_per_image=a.gts, hw=list(a.hw), repeats=a.repeats)
    res_k, t_k = scores("segm", a.repeats)
    res_kb, t_kb = scores("bbox", a.repeats)
    os.environ["S6D_DISABLE_FUSED"] = "mask_pack,mask_pair_inter,box_pair_iou,coco_match"          # the library statements, on the device
    policy.reload()
    res_l, t_l = scores("segm", 2)
    res_lb, t_lb = scores("bbox", 2)
    del os.environ["S6D_DISABLE_FUSED"]
    policy.reload()
    out.update(coco_scores_segm_kernels_s=t_k, coco_scores_segm_library_s=t_l, coco_scores_bbox_kernels_s=t_kb, coco_scores_bbox_library_s=t_lb,
               routes_equal=bool(res_k == res_l and res_kb == res_lb), AP_segm=res_k["AP"], AP_bbox=res_kb["AP"])
    # the kernels alone
    D, G = det["masks"].shape[0], gt["masks"].shape[0]
    dm, gm = det["masks"].view(torch.uint8), gt["masks"].view(torch.uint8)
    per = np.arange(D * a.gts)
    pairs = torch.from_numpy(np.stack([per // a.gts, (per // (a.dets * a.gts)) * a.gts + per % a.gts], 1).astype(np.int32)).to(dev)
    dp, _ = ops.mask_pack(dm)
    gp, _ = ops.mask_pack(gm)
    inter = ops.mask_pair_inter(dp, gp, pairs)
    iou = evaluation._iou_from_counts(inter, *[ops.mask_pack(m)[1] for m in (dm, gm)], pairs)
    table = torch.tensor([[i * a.dets, a.dets, i * a.gts, a.gts] for i in range(a.images)], dtype=torch.int32, device=dev)
    off = torch.arange(a.images, device=dev) * (a.dets * a.gts)
    da, ga = torch.rand(D, dtype=torch.float64, device=dev) * 2e4, torch.rand(G, dtype=torch.float64, device=dev) * 2e4
    gi = torch.zeros(G, dtype=torch.uint8, device=dev)
    th, ar = torch.from_numpy(evaluation.COCO_THRESHOLDS).to(dev), torch.from_numpy(evaluation.COCO_AREA_RANGES).to(dev)
    db, gb = torch.from_numpy(det["bbox"]).to(dev), torch.from_numpy(gt["bbox"]).to(dev)

    def device_ms(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.repeats):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.repeats
    words = dp.shape[1]
    k = {}
    k["mask_pack_ms"] = device_ms(lambda: ops.mask_pack(dm))
    k["mask_pack_gbytes"] = D * a.hw[0] * a.hw[1] * 1.125 / 1e9                                    # the bytes read and the words written
    k["mask_pair_inter_ms"] = device_ms(lambda: ops.mask_pair_inter(dp, gp, pairs))
    k["mask_pair_inter_pairs"] = int(pairs.shape[0])
    k["mask_pair_inter_gbytes"] = (D + pairs.shape[0]) * words * 8 / 1e9                           # a detection row once per run, a ground-truth row per pair
    k["box_pair_iou_ms"] = device_ms(lambda: ops.box_pair_iou(db, gb, pairs))
    k["coco_match_ms"] = device_ms(lambda: ops.coco_match(iou, off, table, da, ga, gi, th, ar))
    k["coco_match_groups"] = a.images
    out["kernels"] = k
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
