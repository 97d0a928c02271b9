"""Connected components and the small-region clean-up (csrc/s6d_ccl.hip) against the plain-loop restatement of their definition
(tests/small_regions_ref.py), `equal` everywhere.  The bodies are `check_*(ops, ...)`: tests/test_emu_small_regions.py runs the same
ones on the host emulator.  The restatement's outputs are computed once per (shape, min_area) and shared (never modified)."""
import functools

import numpy as np
import pytest
import torch

from sam6d_amd import _lib
from tests import small_regions_ref as R

pytestmark = pytest.mark.gpu

TH, TW = _lib.header_constant("S6D_CCL_TILE_H"), _lib.header_constant("S6D_CCL_TILE_W")
BIG = (2 * TH + 6, 2 * TW + 5)                  # three tiles each way, the last one ragged
SHAPES = [(1, 1), (1, 67), (67, 1), (5, 13), BIG]
DENSITIES = (0.3, 0.5, 0.7)


def min_areas(hw):
    return [1, 2, 9, 50, hw[0] * hw[1] + 1]


def _blob(m, y0, x0, area, bw):
    """`area` pixels in row-major order inside a column band of width bw from (y0, x0): one component.  False when it does not fit."""
    H, W = m.shape
    if area <= 0 or x0 < 0 or x0 + min(bw, area) > W or y0 + (area + bw - 1) // bw > H:
        return False
    for k in range(area):
        m[y0 + k // bw, x0 + k % bw] = 1
    return True


def _band(area, H):
    bw = max(1, int(np.ceil(np.sqrt(area))))
    return bw if (area + bw - 1) // bw <= H else (area + H - 1) // H


def _spiral(H, W):
    m = np.zeros((H, W), np.uint8)
    y = x = d = 0
    m[0, 0] = 1
    dirs = [(0, 1), (1, 0), (0, -1), (-1, 0)]
    inside = lambda a, b: 0 <= a < H and 0 <= b < W
    while True:
        for _ in range(2):
            dy, dx = dirs[d]
            if inside(y + dy, x + dx) and not m[y + dy, x + dx] and (not inside(y + 2 * dy, x + 2 * dx) or not m[y + 2 * dy, x + 2 * dx]):
                y, x = y + dy, x + dx
                m[y, x] = 1
                break
            d = (d + 1) % 4
        else:
            return m


def _corners(H, W):
    return [(cy, cx) for cy in range(TH, H, TH) for cx in range(TW, W, TW)]


def patterns(hw, min_area):
    """-> [(name, mask (H,W) uint8)]: the deterministic patterns (those that depend on min_area where they fit) and the seeded ones."""
    H, W = hw
    Z = lambda: np.zeros((H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    out = [("empty", Z()), ("full", Z() + 1), ("checkerboard", ((yy + xx) % 2).astype(np.uint8)), ("spiral", _spiral(H, W))]
    comb = Z()
    comb[0::2] = 1
    for y in range(1, H, 2):
        comb[y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    out.append(("comb", comb))
    diag, anti, block = Z(), Z(), Z()
    sides = [Z() for _ in range(4)]
    for cy, cx in _corners(H, W):
        for d in range(-5, 5):
            if 0 <= cy + d < H and 0 <= cx + d < W:
                diag[cy + d, cx + d] = 1
            if 0 <= cy + d < H and 0 <= cx - 1 - d < W:
                anti[cy + d, cx - 1 - d] = 1
        for s, (dy, dx) in enumerate([(-1, -1), (-1, 0), (0, -1), (0, 0)]):
            sides[s][cy + dy, cx + dx] = 1
            block[cy + dy, cx + dx] = 1
    out += [("diagonal", diag), ("antidiagonal", anti), ("corner block", block)] + [(f"corner side {s}", m) for s, m in enumerate(sides)]
    # blobs of area exactly min_area and min_area - 1 (the second one across the first tile border when there is one), and their negative
    a = min_area
    bw = _band(a, H)
    blobs = Z()
    if _blob(blobs, 0, 0, a, bw):
        _blob(blobs, 0, max(bw + 2, TW - 3 if W > TW + bw else 0), a - 1, bw)
        out += [("blobs", blobs), ("blob-shaped holes", 1 - blobs)]
    # every component small: two of the same (largest) area, the one that starts later placed lower LEFT, and a smaller third
    e = min(min_area - 1, max(1, H * W // 12))
    if e >= 1:
        bw = _band(e, H)
        rows = (e + bw - 1) // bw
        two = Z()
        low = rows + 1 + rows <= H
        ok = _blob(two, 0, bw + 2, e, bw) and (_blob(two, rows + 1, 0, e, bw) if low else _blob(two, 0, 2 * bw + 4, e, bw))
        if ok:
            _blob(two, 0 if low else H, 3 * bw + 6, e - 1, bw)
            out.append(("all small, two equal", two))
        one = Z()
        if _blob(one, H - rows, 0, e, bw):
            out.append(("all small, one blob", one))
        hole = Z()
        if _blob(hole, H - rows, max(0, W - bw), e, bw) and hole.sum() < H * W:
            out.append(("border hole", 255 * (1 - hole)))
    for p in DENSITIES:
        rng = np.random.default_rng([H, W, int(p * 10)])
        out.append((f"bernoulli {p}", (rng.random((H, W)) < p).astype(np.uint8) * 3))
    return out


@functools.lru_cache(maxsize=None)
def case(hw, min_area):
    """-> (names, masks (P,H,W) uint8 read-only, restatement outputs (masks, changed, boxes, branches))."""
    pats = patterns(hw, min_area)
    masks = np.ascontiguousarray(np.stack([m for _, m in pats]).astype(np.uint8))
    masks.setflags(write=False)
    ref = R.remove_small_regions(masks, min_area)
    for a in ref[:3]:
        a.setflags(write=False)
    return [n for n, _ in pats], masks, ref


@functools.lru_cache(maxsize=None)
def label_case(hw):
    _, masks, _ = case(hw, 9)
    labs = {bg: np.stack([R.label(m, bg)[0] for m in masks]) for bg in (False, True)}
    for a in labs.values():
        a.setflags(write=False)
    return masks, labs


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _same(got, ref, names, what):
    masks, changed, boxes = got
    assert masks.dtype == torch.uint8 and changed.dtype == torch.bool and boxes.dtype == torch.int32
    for k, name in enumerate(names):
        assert np.array_equal(masks[k].cpu().numpy(), ref[0][k]), (what, name, "mask")
        assert bool(changed[k]) == bool(ref[1][k]), (what, name, "changed")
        assert boxes[k].tolist() == ref[2][k].tolist(), (what, name, "box")


def check_remove(ops, hw, min_area, as_bool=False):
    names, masks, ref = case(hw, min_area)
    m = _dev(masks)
    _same(ops.remove_small_regions(m != 0 if as_bool else m, min_area), ref, names, (hw, min_area))


def check_labels(ops, hw):
    masks, labs = label_case(hw)
    for bg in (False, True):
        got = ops.label_components(_dev(masks), background=bg)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), labs[bg]), (hw, bg)
    assert np.array_equal(ops.label_components(_dev(masks) != 0).cpu().numpy(), labs[False])


def check_batching(ops, monkeypatch, hw=BIG, min_area=9):
    """N = 0, 1, 3 and two chunks: a mask's result alone, in a batch and under any chunk size is the same."""
    names, masks, ref = case(hw, min_area)
    m = _dev(masks)
    P, (H, W) = m.shape[0], hw
    e = ops.remove_small_regions(m[:0], min_area)
    assert tuple(e[0].shape) == (0, H, W) and tuple(e[1].shape) == (0,) and tuple(e[2].shape) == (0, 4)
    assert tuple(ops.label_components(m[:0]).shape) == (0, H, W)
    for k in (0, P // 2, P - 1):
        _same(ops.remove_small_regions(m[k:k + 1].contiguous(), min_area), [r[k:k + 1] for r in ref[:3]], names[k:k + 1], ("alone", k))
    _same(ops.remove_small_regions(m[P - 3:].contiguous(), min_area), [r[P - 3:] for r in ref[:3]], names[P - 3:], "three")
    _, labs = label_case(hw)
    per_mask = ops._size("s6d_small_regions_workspace_bytes", 1, H, W)
    monkeypatch.setattr(ops, "SMALL_REGIONS_WORKSPACE_BYTES", (P - 1) * per_mask)       # chunks of P - 1 and 1 masks
    _same(ops.remove_small_regions(m, min_area), ref, names, "two chunks")
    assert np.array_equal(ops.label_components(_dev(label_case(hw)[0]), background=True).cpu().numpy(), labs[True])
    monkeypatch.setattr(ops, "SMALL_REGIONS_WORKSPACE_BYTES", 1)                        # one mask per chunk
    _same(ops.remove_small_regions(m, min_area), ref, names, "one per chunk")


def check_arguments(ops):
    m = torch.zeros(2, 5, 13, dtype=torch.uint8).cuda()
    for bad in (0, -3, 1.5):
        with pytest.raises(ValueError, match="min_area"):
            ops.remove_small_regions(m, bad)
    with pytest.raises(RuntimeError):
        ops.remove_small_regions(m.float(), 2)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.remove_small_regions(m[:, :, ::2], 2)
    with pytest.raises(RuntimeError, match="3 dimensions"):
        ops.label_components(m[0])
    assert ops.have("small_regions")


# ---------------------------------------------------------------------------------------------------------------- on the GPU

@pytest.fixture
def dev_ops():
    from sam6d_amd import ops
    return ops


@pytest.mark.parametrize("hw", SHAPES)
def test_remove_small_regions_vs_restatement(dev_ops, hw):
    for k, a in enumerate(min_areas(hw)):
        check_remove(dev_ops, hw, a, as_bool=k % 2 == 1)


@pytest.mark.parametrize("hw", SHAPES)
def test_label_components_vs_restatement(dev_ops, hw):
    check_labels(dev_ops, hw)


def test_results_do_not_depend_on_batch_or_chunk(dev_ops, monkeypatch):
    check_batching(dev_ops, monkeypatch)


def test_arguments(dev_ops):
    check_arguments(dev_ops)


def production_masks(n=8, hw=(480, 640), seed=7):
    """A few discs per mask plus speckle (single pixels and 2 x 2 dots) and pin-holes punched into the discs."""
    H, W = hw
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W), np.uint8)
    for k in range(n):
        m = np.zeros((H, W), bool)
        for _ in range(int(rng.integers(1, 5))):
            cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(4, 90)
            m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        speck = rng.random((H, W)) < 0.002
        m ^= speck                                                         # islands outside the discs, pin-holes inside
        m[:-1, :-1] ^= speck[1:, 1:] & (rng.random((H - 1, W - 1)) < 0.3)   # some of them two pixels across a diagonal
        out[k] = m
    return out


def test_production_shape_kernel_equals_library_statement(dev_ops):
    """8 masks of 480 x 640, min_area = 100: the kernels against the torch statement of the same definition on the device (the
    plain-loop restatement is too slow here; the statement is pinned to it at the small shapes, tests/test_host_small_regions.py)."""
    from sam6d_amd.sam import amg
    m = torch.from_numpy(production_masks()).cuda()
    got = dev_ops.remove_small_regions(m, 100)
    lib = amg._remove_small_regions_library(m, 100)
    assert bool(got[1].any()) and int(got[0].sum()) > 0
    for g, l in zip(got, lib):
        assert g.dtype == l.dtype and torch.equal(g, l)
    for bg in (False, True):
        want = amg._min_index_labels_library((m != 0) != bg).int()
        assert torch.equal(dev_ops.label_components(m, background=bg), want)
    via = amg.remove_small_regions(m != 0, 100)
    assert all(torch.equal(a, b) for a, b in zip(via, got))


def test_frame_pipeline_with_min_mask_region_area(monkeypatch):
    """FramePipeline(segmentor={"min_mask_region_area": 100}) on the mini frame of tests/test_gpu_zz_pipeline.py: the segmentor stage
    equals ``postprocess_small_regions`` (library route) of the stage without the option, its masks are fixed points of the
    clean-up, and the frame runs through to poses."""
    from sam6d_amd import policy
    from sam6d_amd.sam import amg
    from tests.test_gpu_zz_pipeline import build_mini
    pipe, frame = build_mini(torch.device("cuda", 0))
    img = frame[0]
    emb = pipe._embed([img])
    base = pipe._segment(emb, img)
    pipe.seg_kw = dict(pipe.seg_kw, min_mask_region_area=100)          # what FramePipeline(segmentor={...}) stores
    got = pipe._segment(emb, img)
    assert not [k for k in policy.library_branch_hits() if k[0].startswith("amg.")]           # the clean-up ran on its kernels
    monkeypatch.setenv("S6D_DISABLE_FUSED", "small_regions")
    want = amg.postprocess_small_regions(base, 100, max(pipe.seg_kw["box_nms_thresh"], 0.7))
    monkeypatch.delenv("S6D_DISABLE_FUSED")
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) and got[k].dtype == base[k].dtype for k in want)
    again, _, boxes = amg.remove_small_regions(got["masks"], 100)
    assert torch.equal(again.bool(), got["masks"]) and torch.equal(boxes.long(), got["boxes"])
    assert bool(amg.remove_small_regions(base["masks"], 100)[1].any())                            # (the stage had something to do)
    det, poses = pipe(*frame)
    assert det.masks.shape[0] >= 1 and torch.isfinite(det.scores).all()
