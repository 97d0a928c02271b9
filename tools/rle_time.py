"""Times of the run-length mask kernels (csrc/s6d_rle.hip) on the GPU against the routes they replace (profiles/rle.md):

python tools/rle_time.py [--n 1024] [--hw 480 640] [--n-worst 64] [--n-big 64] [--big-hw 1080 1920] [--rounds 5] [--repeats 20]
                         [--kernels-only] [--out FILE]

Seeded BLOB masks: the union of three discs of radius 8 .. 45 per mask, a few thousand pixels, as proposal-like masks are.  Per round
the two routes of a comparison run one after the other in the same process; the figures are medians over the rounds.
  1. encode     ``handoff.masks_to_rle(masks)`` (torch statements + a Python loop; the parent's route) against
                ``RleMasks.from_masks(masks).to_records()`` (the kernels + one split of a flat host array); host wall time around a
                synchronise; the lists must be identical.  ``ops.rle_encode`` alone by device events.
  2. decode     for scoring, from the records of a file: ``rle_to_mask`` per record + ``np.stack`` + upload + ``ops.mask_pack`` (the
                parent's route) against ``RleMasks.from_records(...).packed()``; wall time, identical words and areas; the peak host
                and device bytes of each route computed from the shapes.  ``ops.rle_to_packed`` / ``ops.rle_to_masks`` /
                ``ops.mask_pack`` alone by device events.
  3. worst case checkerboards (every run one pixel long: H W + 1 counts a mask) at --n-worst masks, kernels by device events.
  4. bands      one --big-hw (1920 x 1080) batch of --n-big blob masks: kernels by device events, results compared with ``ops.mask_pack`` and
                the input.
``--kernels-only``: only the kernel calls, the target of a ``rocprofv3 --kernel-trace --stats`` run.  Prints one JSON line.  There is
no CPU path: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def blob_masks(n, hw, device, seed=7):
    import torch
    H, W = hw
    g = torch.Generator(device="cpu").manual_seed(seed)
    yy, xx = torch.arange(H, device=device).view(1, H, 1), torch.arange(W, device=device).view(1, 1, W)
    m = torch.zeros(n, H, W, dtype=torch.bool, device=device)
    for a in range(0, n, 128):                                             # (n, H, W) int64 temporaries: a part at a time
        k = min(128, n - a)
        for _ in range(3):
            cy, cx = torch.randint(0, H, (k, 1, 1), generator=g).to(device), torch.randint(0, W, (k, 1, 1), generator=g).to(device)
            r = torch.randint(8, 46, (k, 1, 1), generator=g).to(device)
            m[a:a + k] |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return m


def route_bytes(n, hw, runs):
    """Peak bytes each decode route holds, from the shapes: dense = n H W bytes, packed = n ceil(H W / 64) 8, run lists = 4 bytes a
    count + 8 an offset, their inclusive scan 8 bytes a count."""
    H, W = hw
    dense, packed = n * H * W, n * ((H * W + 63) // 64) * 8
    lists = 4 * runs + 8 * (n + 1)
    return dict(parent=dict(host=2 * dense, device=dense + packed),         # the masks one by one AND their stack; upload + words
                rle=dict(host=8 * (runs + n + 1), device=8 * (runs + n + 1) + lists + 8 * runs + packed))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--hw", type=int, nargs=2, default=(480, 640))
    ap.add_argument("--n-worst", type=int, default=64)
    ap.add_argument("--n-big", type=int, default=64)
    ap.add_argument("--big-hw", type=int, nargs=2, default=(1080, 1920))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch

    from sam6d_amd import ops
    from sam6d_amd.ism import handoff
    if not torch.cuda.is_available():
        raise SystemExit("rle_time: needs a GPU")
    dev, hw = torch.device("cuda"), tuple(a.hw)
    H, W = hw

    def device_ms(fn, n=a.repeats):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def kernels(masks, size):
        u8 = masks.view(torch.uint8)
        counts, offsets = ops.rle_encode(u8)
        rec = dict(masks=int(masks.shape[0]), runs=int(counts.shape[0]), band_columns=None)
        rec["rle_encode_ms"] = device_ms(lambda: ops.rle_encode(u8))
        rec["rle_to_packed_ms"] = device_ms(lambda: ops.rle_to_packed(counts, offsets, *size))
        rec["rle_to_masks_ms"] = device_ms(lambda: ops.rle_to_masks(counts, offsets, *size))
        rec["mask_pack_ms"] = device_ms(lambda: ops.mask_pack(u8))
        if not a.kernels_only:
            p, ar = ops.rle_to_packed(counts, offsets, *size)
            q, br = ops.mask_pack(u8)
            rec["packed_equal_mask_pack"] = bool(torch.equal(p, q) and torch.equal(ar, br))
            rec["dense_equal_input"] = bool(torch.equal(ops.rle_to_masks(counts, offsets, *size), u8))
        return rec

    masks = blob_masks(a.n, hw, dev)
    out = dict(hw=list(hw), n=a.n, rounds=a.rounds, repeats=a.repeats, masks="three discs of radius 8 .. 45 per mask",
               mean_area=float(masks.flatten(1).sum(1).float().mean()))
    out["kernels"] = kernels(masks, hw)
    if not a.kernels_only:
        # 1. encode
        t_old, t_new = [], []
        for _ in range(a.rounds + 1):                                      # the first round warms both routes up and is dropped
            ms, old = wall_ms(lambda: handoff.masks_to_rle(masks))
            t_old.append(ms)
            ms, new = wall_ms(lambda: handoff.RleMasks.from_masks(masks).to_records())
            t_new.append(ms)
        out["encode"] = dict(masks_to_rle_ms=statistics.median(t_old[1:]), rle_masks_ms=statistics.median(t_new[1:]),
                             all_rounds=dict(masks_to_rle=t_old[1:], rle_masks=t_new[1:]), identical=old == new)
        # 2. decode for scoring
        records = new

        def parent():
            dense = np.stack([handoff.rle_to_mask(r) for r in records])
            return ops.mask_pack(torch.from_numpy(dense).to(dev).contiguous())     # (as evaluation._masks_u8 uploads them)

        def rle():
            return handoff.RleMasks.from_records(records, dev).packed()
        t_old, t_new = [], []
        for _ in range(a.rounds + 1):
            ms, old = wall_ms(parent)
            t_old.append(ms)
            ms, new = wall_ms(rle)
            t_new.append(ms)
        runs = sum(len(r["counts"]) for r in records)
        out["decode"] = dict(parent_ms=statistics.median(t_old[1:]), rle_ms=statistics.median(t_new[1:]),
                             all_rounds=dict(parent=t_old[1:], rle=t_new[1:]), runs=runs, bytes=route_bytes(a.n, hw, runs),
                             identical=bool(torch.equal(old[0], new[0]) and torch.equal(old[1], new[1])))
    del masks
    # 3. the maximum-run masks
    yy, xx = torch.arange(H, device=dev).view(1, H, 1), torch.arange(W, device=dev).view(1, 1, W)
    board = (((yy + xx + torch.arange(a.n_worst, device=dev).view(-1, 1, 1)) & 1) != 0).contiguous()
    out["checkerboard"] = kernels(board, hw)
    del board
    # 4. bands: 1920 x 1080
    big = tuple(a.big_hw)
    out["big"] = dict(hw=list(big), **kernels(blob_masks(a.n_big, big, dev, seed=9), big))
    for rec, size in ((out["kernels"], hw), (out["checkerboard"], hw), (out["big"], big)):
        pitch = ((size[0] + 63) // 64) | 1
        bc = ops.RLE_BAND_WORDS // pitch
        rec["band_columns"] = min(size[1], bc - bc % 64 if bc >= 64 else bc)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
