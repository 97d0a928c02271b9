"""Times of the small-region clean-up (csrc/s6d_ccl.hip) on the GPU (profiles/small_regions.md):

python tools/small_regions_time.py [--hw 480 640] [--min-area 100] [--repeats 20] [--kernels-only] [--out FILE]

Seeded masks of a few discs plus speckle and pin-holes, at the mask count the Example frame's proposal stage keeps (the rows of
``sam_masks`` in tests/golden/frame_e2e.npz) and at 256.  Measured per count: ``ops.remove_small_regions`` (the kernels; device events
around ``repeats`` calls after a warm-up), ``amg._remove_small_regions_library`` (the torch statement, on the device) and the scipy
statement of tests/small_regions_ref.py on the host, one mask at a time -- the way the upstream generator calls cv2, which is not
part of this project: scipy stands in.  The three results are compared.  Then the proposals stage (``amg.generate_proposals`` on the
seeded decoder, as tools/sam_decoder_time.py) with min_mask_region_area 0 and ``--min-area``, at box_nms_thresh 0.7 and 1.5.  ``--kernels-only``: only the kernel calls,
the target of a ``rocprofv3 --kernel-trace --stats`` run (per-kernel times).  Bytes per pass are computed from the shapes (below).
Prints one JSON line.  There is no CPU path: without a GPU this fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def make_masks(n, hw, device, seed=7):
    import torch
    H, W = hw
    g = torch.Generator(device="cpu").manual_seed(seed)
    yy, xx = torch.arange(H, device=device).view(1, H, 1), torch.arange(W, device=device).view(1, 1, W)
    m = torch.zeros(n, H, W, dtype=torch.bool, device=device)
    for _ in range(4):
        cy, cx = torch.randint(0, H, (n, 1, 1), generator=g).to(device), torch.randint(0, W, (n, 1, 1), generator=g).to(device)
        r = torch.randint(4, 90, (n, 1, 1), generator=g).to(device)
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    speck = (torch.rand(n, H, W, generator=g) < 0.002).to(device)
    return (m ^ speck).to(torch.uint8)                                      # islands outside the discs, pin-holes inside


def pass_bytes(n, hw):
    """Bytes each pass of one clean-up must move for n masks (mask bytes M = n H W, an int32 plane P = 4 M), from the shapes alone:
    the seam pass touches only the first rows / columns of tiles and the area pass reads one plane and writes at local roots."""
    from sam6d_amd import ops
    M = n * hw[0] * hw[1]
    P = 4 * M
    th, tw = ops.CCL_TILE
    seam = 4 * n * (2 * (hw[0] // th) * hw[1] + 2 * (hw[1] // tw) * hw[0])
    per_polarity = {"tile": M + 2 * P, "seam": seam, "area": P, "apply": M + 2 * P + M}
    return dict(per_polarity=per_polarity, flatten_islands=3 * P, total=2 * sum(per_polarity.values()) + 3 * P)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--hw", type=int, nargs=2, default=(480, 640))
    ap.add_argument("--min-area", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch

    from sam6d_amd import ops, policy
    from sam6d_amd.sam import amg
    if not torch.cuda.is_available():
        raise SystemExit("small_regions_time: needs a GPU")
    dev, hw = torch.device("cuda"), tuple(a.hw)
    n_frame = int(np.load(os.path.join(ROOT, "tests", "golden", "frame_e2e.npz"))["sam_masks"].shape[0])

    def device_ms(fn, n):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n
    out = dict(hw=list(hw), min_area=a.min_area, repeats=a.repeats, frame_masks=n_frame, counts={})
    for n in (n_frame, 256):
        masks = make_masks(n, hw, dev)
        rec = dict(bytes=pass_bytes(n, hw))
        rec["kernels_ms"] = device_ms(lambda: ops.remove_small_regions(masks, a.min_area), a.repeats)
        rec["kernels_gbytes_per_s"] = rec["bytes"]["total"] / rec["kernels_ms"] / 1e6
        rec["label_components_ms"] = device_ms(lambda: ops.label_components(masks), a.repeats)
        if not a.kernels_only:
            got = ops.remove_small_regions(masks, a.min_area)
            rec["changed_masks"] = int(got[1].sum())
            lib = None
            for part in range(0, n, 32):                                    # (the statement's bincount is (n, H W) int64)
                r = amg._remove_small_regions_library(masks[part:part + 32], a.min_area)
                lib = r if lib is None else tuple(torch.cat(p) for p in zip(lib, r))
            rec["library_ms"] = device_ms(lambda: [amg._remove_small_regions_library(masks[p:p + 32], a.min_area) for p in range(0, n, 32)], 2)
            rec["kernels_equal_library"] = all(torch.equal(x, y) for x, y in zip(got, lib))
            try:
                import scipy  # noqa: F401

                from tests import small_regions_ref as R
                host = masks.cpu().numpy()
                t0 = time.perf_counter()
                res = [R.scipy_statement(R.scipy_statement(m, a.min_area, True)[0], a.min_area, False)[0] for m in host]
                rec["scipy_host_ms"] = (time.perf_counter() - t0) * 1e3
                rec["kernels_equal_scipy"] = bool(np.array_equal(np.stack(res), got[0].cpu().numpy() != 0))
            except ImportError:
                rec["scipy_host_ms"] = None                                  # not measured: scipy is not installed
        out["counts"][str(n)] = rec
    if not a.kernels_only:
        from sam6d_amd.sam.mask_decoder import build_sam_decoder
        from sam6d_amd.utils import seeded, synth
        os.environ["S6D_SAM_DECODER_DTYPE"] = "bf16"
        policy.reload()
        m = seeded.load_seeded(build_sam_decoder(), 1).cuda()
        emb = synth.sam_decoder_inputs(dict(dim=256, emb=64, img=1024), 1024, 3)["emb"].cuda()
        kw = dict(pred_iou_thresh=0.05, stability_score_thresh=0.3, stability_score_offset=0.02, points_per_batch=256)
        # box_nms_thresh 0.7: the seeded decoder's boxes are all the frame and one proposal survives; 1.5: nothing is suppressed, so
        # the clean-up sees every candidate that passes the filters (far more masks than a real frame keeps: an upper figure)
        for nms_thresh in (0.7, 1.5):
            stage = {}
            for k in (0, a.min_area):
                fn = lambda: amg.generate_proposals(m.prompt_encoder, m.mask_decoder, emb, hw, min_mask_region_area=k,  # noqa: E731
                                                    box_nms_thresh=nms_thresh, **kw)
                stage[str(k)] = dict(proposals=int(fn()["masks"].shape[0]), ms=device_ms(fn, 5))
            out[f"proposals_stage_nms_{nms_thresh}"] = stage
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
