"""The run-length mask kernels (csrc/s6d_rle.hip) against the plain-loop restatement of the format (tests/rle_ref.py), against
``handoff.masks_to_rle`` and against ``ops.mask_pack`` of the dense masks: `equal` everywhere.  The bodies are `check_*(ops, ...)`:
tests/test_emu_rle.py runs the same ones on the host emulator.  Every small shape is run at the default band capacity (one band) and
at SMALL_BAND words, where the shapes cross band seams; the restatement's outputs are computed once per shape and shared (never
modified)."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from sam6d_amd import policy
from sam6d_amd.ism import handoff
from tests import rle_ref as R

pytestmark = pytest.mark.gpu

SMALL_BAND = 16                                  # LDS words of a band under the test switch
POW2 = (128, 20)                                 # two words per column: without the odd pitch the columns would share LDS banks
BANDS = (70, 23)                                 # at SMALL_BAND: 5 columns per band, five bands, the last one 3 columns
SHAPES = [(1, 1), (1, 67), (67, 1), (5, 13), (64, 64), (63, 65), (130, 3), POW2, BANDS]
DENSITIES = (0.02, 0.5, 0.98)


def band_columns(H, W, words):
    """Columns of a decoder band at a capacity of `words` (include/sam6d_hip.h: a column takes ceil(H / 64) | 1 words)."""
    bc = words // (((H + 63) // 64) | 1)
    if bc >= 64:
        bc -= bc % 64
    return min(bc, W)


@contextlib.contextmanager
def band_words(ops, words):
    ops.set_rle_band_words(words)
    try:
        yield
    finally:
        ops.set_rle_band_words(0)


def _from_counts(counts, H, W):
    return np.array(R.decode(counts, H, W), np.uint8)


@functools.lru_cache(maxsize=None)
def patterns(hw):
    """-> (names, masks (P,H,W) uint8 0 / 1, run lists, packed words (P,words) int64, areas): the deterministic patterns (the seam
    ones placed for SMALL_BAND) and the seeded ones, with the restatement's results."""
    H, W = hw
    Z = lambda: np.zeros((H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    out = [("zero", Z()), ("one", Z() + 1)]
    for name, (y, x) in (("top left", (0, 0)), ("top right", (0, W - 1)), ("bottom left", (H - 1, 0)), ("bottom right", (H - 1, W - 1))):
        m = Z()
        m[y, x] = 1
        out.append((name, m))
    out += [("checkerboard", ((yy + xx) % 2).astype(np.uint8)), ("checkerboard from one", ((yy + xx + 1) % 2).astype(np.uint8)),
            ("row stripes", (yy % 2).astype(np.uint8)), ("row stripes from one", ((yy + 1) % 2).astype(np.uint8)),
            ("column stripes", (xx % 2).astype(np.uint8)), ("column stripes from one", ((xx + 1) % 2).astype(np.uint8))]
    bc = band_columns(H, W, SMALL_BAND)
    if W >= 3:
        m = Z()
        m[:, 1:W - 1] = 1                                                  # whole columns: ONE run across every band between
        out.append(("solid columns", m))
    if W >= 3 and H >= 3:
        m = Z()
        m[1:H - 1, 1:min(W - 1, 2 * bc + 2)] = 1                            # a block wider than a band, a run per column
        out.append(("inset block", m))
    seam = bc * H                                                          # the first pixel of the second band
    for d in (-1, 0, 1):
        for lead in (0, 3):
            if bc < W and seam + d - lead >= 1 and H * W - seam - d >= 1:
                out.append((f"run from {lead} to the seam {d:+d}", _from_counts([lead, seam + d - lead, H * W - seam - d], H, W)))
    for p in DENSITIES:
        rng = np.random.default_rng([H, W, int(p * 100)])
        out.append((f"random {p}", (rng.random((H, W)) < p).astype(np.uint8)))
    names = [n for n, _ in out]
    masks = np.stack([m for _, m in out])
    lists = [R.encode(m.tolist()) for m in masks]
    pk = [R.packed(m.tolist()) for m in masks]
    words = np.array([[R.signed64(w) for w in ws] for ws, _ in pk], np.int64).reshape(len(out), (H * W + 63) // 64)
    areas = np.array([a for _, a in pk], np.int32)
    for a in (masks, words, areas):
        a.setflags(write=False)
    return names, masks, lists, words, areas


def _tensor(masks, as_bool):
    """0 / 1 masks -> bool, or uint8 whose set bytes are anything but 0 (2, 255, 128 ...)."""
    if as_bool:
        return torch.from_numpy(masks != 0).cuda()
    values = np.array([2, 255, 128, 1, 77], np.uint8)[np.arange(masks.size).reshape(masks.shape) % 5]
    return torch.from_numpy(masks * values).cuda()


def _flat(lists, dev):
    """Python run lists -> (counts int32, offsets int64) on dev."""
    counts = torch.tensor([c for l in lists for c in l], dtype=torch.int32)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum([len(l) for l in lists])]), dtype=torch.int64)
    return counts.to(dev), offsets.to(dev)


def _kernels_only(ops):
    assert ops.have("rle_encode") and ops.have("rle_to_packed") and ops.have("rle_to_masks") and ops.have("mask_pack")
    policy.reset_library_branch_hits()


def check_encode(ops, hw, words):
    _kernels_only(ops)
    names, masks, lists, _, _ = patterns(hw)
    H, W = hw
    with band_words(ops, words):
        for as_bool in (True, False):
            t = _tensor(masks, as_bool)
            rle = handoff.RleMasks.from_masks(t)
            recs = rle.to_records()
            assert len(rle) == len(names) and rle.size == hw
            assert rle.counts.dtype == torch.int32 and rle.offsets.dtype == torch.int64
            for n, name in enumerate(names):
                assert recs[n] == {"counts": lists[n], "size": [H, W]}, (name, as_bool)
                c = recs[n]["counts"]
                assert len(c) >= 1 and all(v >= 1 for v in c[1:]) and c[0] >= 0 and sum(c) == H * W, name
            assert recs == handoff.masks_to_rle(t)
            counts, offsets = ops.rle_encode(t.view(torch.uint8) if as_bool else t)
            assert torch.equal(counts, rle.counts) and torch.equal(offsets, rle.offsets)
    assert not policy.library_branch_hits()


def check_packed(ops, hw, words):
    _kernels_only(ops)
    names, masks, lists, ref_words, ref_areas = patterns(hw)
    H, W = hw
    t = _tensor(masks, False)
    want_p, want_a = ops.mask_pack(t)
    assert np.array_equal(want_p.cpu().numpy(), ref_words) and np.array_equal(want_a.cpu().numpy(), ref_areas)
    counts, offsets = _flat(lists, t.device)
    with band_words(ops, words):
        got_p, got_a = ops.rle_to_packed(counts, offsets, H, W)
        assert got_p.dtype == torch.int64 and got_a.dtype == torch.int32
        bad = [names[n] for n in range(len(names)) if not torch.equal(got_p[n], want_p[n]) or int(got_a[n]) != int(want_a[n])]
        assert not bad, bad
        # once more straight through the entry point, on outputs whose every bit is set beforehand: every word and area is written
        N, Rn = len(names), counts.shape[0]
        p1 = torch.full_like(want_p, -1)
        a1 = torch.full_like(want_a, -1)
        status = torch.full((N + 1,), -1, dtype=torch.int32, device=t.device)
        ends = torch.cumsum(counts, 0, dtype=torch.int64)
        ops._call("s6d_rle_to_packed", counts.data_ptr(), offsets.data_ptr(), ends.data_ptr(), N, Rn, H, W, status.data_ptr(),
                  p1.data_ptr(), a1.data_ptr(), ops._stream())
        torch.cuda.synchronize()
        assert torch.equal(p1, want_p) and torch.equal(a1, want_a)
        assert int(status[0]) == 2 ** 31 - 1 and not bool(status[1:].any())
        rle = handoff.RleMasks(counts, offsets, hw)
        for a, b in zip(rle.packed(), (want_p, want_a)):
            assert torch.equal(a, b)
    assert not policy.library_branch_hits()


def check_dense(ops, hw, words):
    _kernels_only(ops)
    names, masks, lists, _, _ = patterns(hw)
    H, W = hw
    want = torch.from_numpy(np.array(masks)).cuda()
    counts, offsets = _flat(lists, want.device)
    with band_words(ops, words):
        got = ops.rle_to_masks(counts, offsets, H, W)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (len(names), H, W)
        bad = [names[n] for n in range(len(names)) if not torch.equal(got[n], want[n])]
        assert not bad, bad
        # the round trip from the encoder's own lists
        rle = handoff.RleMasks.from_masks(_tensor(masks, False))
        dense = rle.to_dense()
        assert dense.dtype == torch.bool and torch.equal(dense.view(torch.uint8), want)
    assert not policy.library_branch_hits()


def check_batching(ops, hw=BANDS, words=SMALL_BAND):
    """A mask's lists, words and pixels are the same alone, in the batch, and in the batch in another order; N = 0."""
    _kernels_only(ops)
    names, masks, lists, _, _ = patterns(hw)
    H, W = hw
    t = _tensor(masks, False)
    with band_words(ops, words):
        counts, offsets = ops.rle_encode(t)
        packed, area = ops.rle_to_packed(counts, offsets, H, W)
        dense = ops.rle_to_masks(counts, offsets, H, W)
        o = offsets.tolist()
        order = list(range(len(names)))[::-1]
        order = order[1::2] + order[0::2]
        pc, po = ops.rle_encode(t[order].contiguous())
        pp, pa = ops.rle_to_packed(pc, po, H, W)
        pd = ops.rle_to_masks(pc, po, H, W)
        q = po.tolist()
        for k, n in enumerate(order):
            assert torch.equal(pc[q[k]:q[k + 1]], counts[o[n]:o[n + 1]]), names[n]
            assert torch.equal(pp[k], packed[n]) and int(pa[k]) == int(area[n]) and torch.equal(pd[k], dense[n]), names[n]
        for n in (0, len(names) // 2, len(names) - 1):
            c1, o1 = ops.rle_encode(t[n:n + 1].contiguous())
            assert torch.equal(c1, counts[o[n]:o[n + 1]]) and o1.tolist() == [0, o[n + 1] - o[n]], names[n]
            p1, a1 = ops.rle_to_packed(c1, o1, H, W)
            assert torch.equal(p1[0], packed[n]) and int(a1[0]) == int(area[n]), names[n]
            assert torch.equal(ops.rle_to_masks(c1, o1, H, W)[0], dense[n]), names[n]
        # N = 0
        c0, o0 = ops.rle_encode(t[:0].contiguous())
        assert tuple(c0.shape) == (0,) and c0.dtype == torch.int32 and o0.tolist() == [0] and o0.dtype == torch.int64
        p0, a0 = ops.rle_to_packed(c0, o0, H, W)
        assert tuple(p0.shape) == (0, (H * W + 63) // 64) and tuple(a0.shape) == (0,)
        assert tuple(ops.rle_to_masks(c0, o0, H, W).shape) == (0, H, W)
        empty = handoff.RleMasks.from_masks(t[:0])
        assert len(empty) == 0 and empty.to_records() == [] and tuple(empty.to_dense().shape) == (0, H, W)


def noncanonical(lists, hw):
    """Lists the decoders must accept -> [(list, the canonical list of the same mask)]."""
    H, W = hw
    out = [([0, 0, H * W], [H * W]), ([H * W, 0], [H * W]), ([0, H * W, 0], [0, H * W]), ([0, 0, 0, H * W, 0, 0], [0, H * W])]
    for c in lists:
        if len(c) >= 3:
            k = len(c) // 2
            out.append((c[:k] + [0, 0] + c[k:], c))                       # an empty pair between two runs
            out.append((c + [0], c))                                      # a trailing zero count
            if c[k] >= 2:
                out.append((c[:k] + [1, 0, c[k] - 1] + c[k + 1:], c))     # a run cut in two by an empty run of the other value
    return out


def check_noncanonical(ops, hw=BANDS, words=SMALL_BAND):
    _kernels_only(ops)
    names, masks, lists, _, _ = patterns(hw)
    H, W = hw
    cases = noncanonical(lists, hw)
    dev = torch.zeros(1).cuda().device
    counts, offsets = _flat([a for a, _ in cases], dev)
    ccounts, coffsets = _flat([b for _, b in cases], dev)
    with band_words(ops, words):
        got_p, got_a = ops.rle_to_packed(counts, offsets, H, W)
        want_p, want_a = ops.rle_to_packed(ccounts, coffsets, H, W)
        assert torch.equal(got_p, want_p) and torch.equal(got_a, want_a)
        got = ops.rle_to_masks(counts, offsets, H, W)
        assert torch.equal(got, ops.rle_to_masks(ccounts, coffsets, H, W))
        for n in (0, 1, 2, 3, len(cases) - 1):
            assert got[n].cpu().numpy().tolist() == R.decode(cases[n][0], H, W)


def refused(hw):
    """-> [(what, list)]: lists every decoder refuses."""
    H, W = hw
    return [("a negative count", [H * W + 1, -1]), ("a negative count with the right total", [2, -1, H * W - 1]),
            ("a sum one short", [H * W - 1]), ("a sum one long", [1, H * W]), ("an empty list", [])]


def check_refused(ops, hw=BANDS, words=SMALL_BAND):
    _kernels_only(ops)
    H, W = hw
    good = [[H * W], [0, H * W], [3, 4, H * W - 7]]
    dev = torch.zeros(1).cuda().device
    with band_words(ops, words):
        for what, bad in refused(hw):
            for at in (0, 2, 3):
                lists = good[:at] + [bad] + good[at:]
                counts, offsets = _flat(lists, dev)
                for fn in (ops.rle_to_packed, ops.rle_to_masks):
                    with pytest.raises(ValueError, match=rf"mask {at}\b"):
                        fn(counts, offsets, H, W)
                rle = handoff.RleMasks(counts, offsets, hw)
                for fn in (rle.packed, rle.to_dense):
                    with pytest.raises(ValueError, match=rf"mask {at}\b"):
                        fn()
        # two bad masks: the first one is named
        counts, offsets = _flat([good[0], [H * W - 1], good[1], [1, H * W]], dev)
        with pytest.raises(ValueError, match=r"mask 1\b"):
            ops.rle_to_packed(counts, offsets, H, W)


def check_arguments(ops):
    H, W = 5, 13
    m = torch.zeros(2, H, W, dtype=torch.uint8).cuda()
    counts, offsets = ops.rle_encode(m)
    assert counts.tolist() == [H * W, H * W] and offsets.tolist() == [0, 1, 2]
    with pytest.raises(RuntimeError):
        ops.rle_encode(m.float())
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.rle_encode(m[:, :, ::2])
    with pytest.raises(RuntimeError, match="3 dimensions"):
        ops.rle_encode(m[0])
    for fn in (ops.rle_to_packed, ops.rle_to_masks):
        with pytest.raises(RuntimeError):
            fn(counts.long(), offsets, H, W)
        with pytest.raises(RuntimeError):
            fn(counts, offsets.int(), H, W)
        with pytest.raises(ValueError, match="offsets"):
            fn(counts, torch.tensor([0, 1, 3]).to(counts.device), H, W)          # does not end at len(counts)
        with pytest.raises(ValueError, match="offsets"):
            fn(counts, torch.tensor([1, 1, 2]).to(counts.device), H, W)          # does not begin at 0
        with pytest.raises(ValueError, match="offsets"):
            fn(counts, torch.tensor([0, 2, 1, 2]).to(counts.device), H, W)       # decreasing
        with pytest.raises(ValueError, match="H W"):
            fn(counts, offsets, 0, W)
    with pytest.raises(Exception):
        ops.set_rle_band_words(-1)
    with pytest.raises(Exception):
        ops.set_rle_band_words(ops.RLE_BAND_WORDS + 1)
    with band_words(ops, 1):                                                    # one column of 65 rows does not fit one word
        with pytest.raises(Exception, match="s6d_rle"):
            ops.rle_encode(torch.zeros(1, 65, 2, dtype=torch.uint8).cuda())
        assert ops.rle_encode(torch.ones(1, 64, 2, dtype=torch.uint8).cuda())[0].tolist() == [0, 128]


def check_coco_scores(ops, device):
    """coco_scores with run lists on either side and on both: the dense result, as whole dicts."""
    from sam6d_amd import evaluation
    H, W = 40, 52
    rng = np.random.default_rng(5)
    G, D = 9, 14
    yy, xx = np.mgrid[0:H, 0:W]

    def disc():
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(3, 14)
        return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    gm = np.stack([disc() for _ in range(G)])
    dm = np.stack([np.roll(gm[k % G], (int(rng.integers(-2, 3)), int(rng.integers(-2, 3))), (0, 1)) for k in range(D)])
    gt = dict(im=np.array([[1, k % 3] for k in range(G)]), category=np.array([1 + k % 2 for k in range(G)]), masks=torch.from_numpy(gm).to(device),
              ignore=np.arange(G) % 4 == 3)
    det = dict(im=np.array([[1, k % 3] for k in range(D)]), category=np.array([1 + k % 2 for k in range(D)]), score=rng.random(D),
               masks=torch.from_numpy(dm).to(device))
    want = evaluation.coco_scores(det, gt, "segm", device=device)
    assert want["AP"] > 0
    d_rle, g_rle = dict(det, masks=handoff.RleMasks.from_masks(det["masks"])), dict(gt, masks=handoff.RleMasks.from_masks(gt["masks"]))
    assert evaluation.coco_scores(d_rle, gt, "segm", device=device) == want
    assert evaluation.coco_scores(det, g_rle, "segm", device=device) == want
    assert evaluation.coco_scores(d_rle, g_rle, "segm", device=device) == want
    pairs = np.array([[d, g] for d in range(D) for g in range(G)], np.int32)
    assert torch.equal(evaluation.mask_ious(d_rle["masks"], g_rle["masks"], pairs, device), evaluation.mask_ious(det["masks"], gt["masks"], pairs, device))
    assert evaluation.coco_scores(dict(d_rle, masks=d_rle["masks"][:0], im=det["im"][:0], category=det["category"][:0], score=det["score"][:0]),
                                  g_rle, "segm", device=device) == \
        evaluation.coco_scores(dict(det, masks=det["masks"][:0], im=det["im"][:0], category=det["category"][:0], score=det["score"][:0]),
                               gt, "segm", device=device)


# ---------------------------------------------------------------------------------------------------------------- on the GPU

@pytest.fixture
def dev_ops():
    from sam6d_amd import ops
    yield ops
    ops.set_rle_band_words(0)


@pytest.mark.parametrize("words", [0, SMALL_BAND])
@pytest.mark.parametrize("hw", SHAPES)
def test_encode_vs_restatement_and_masks_to_rle(dev_ops, hw, words):
    check_encode(dev_ops, hw, words)


@pytest.mark.parametrize("words", [0, SMALL_BAND])
@pytest.mark.parametrize("hw", SHAPES)
def test_runs_to_packed_vs_mask_pack_and_restatement(dev_ops, hw, words):
    check_packed(dev_ops, hw, words)


@pytest.mark.parametrize("words", [0, SMALL_BAND])
@pytest.mark.parametrize("hw", SHAPES)
def test_runs_to_dense(dev_ops, hw, words):
    check_dense(dev_ops, hw, words)


@pytest.mark.parametrize("words", [0, SMALL_BAND])
def test_results_do_not_depend_on_the_batch(dev_ops, words):
    check_batching(dev_ops, BANDS, words)


@pytest.mark.parametrize("words", [0, SMALL_BAND])
def test_non_canonical_lists_are_accepted(dev_ops, words):
    check_noncanonical(dev_ops, BANDS, words)


def test_bad_lists_are_refused_with_the_mask_index(dev_ops):
    check_refused(dev_ops)


def test_arguments(dev_ops):
    check_arguments(dev_ops)


def test_coco_scores_from_run_lists_equal_the_dense_result(dev_ops):
    _kernels_only(dev_ops)
    check_coco_scores(dev_ops, "cuda")
    assert not policy.library_branch_hits()


def test_camera_frame_at_the_default_band(dev_ops):
    """480 x 640, N = 8, the default band capacity: 448 + 192 columns, so every word of a row is one band's and nothing is ORed."""
    H, W, N = 480, 640, 8
    assert band_columns(H, W, dev_ops.RLE_BAND_WORDS) == 448
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:H, 0:W]
    masks = np.zeros((N, H, W), np.uint8)
    for n in range(N):
        for _ in range(3):
            cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(5, 60)
            masks[n] |= ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).astype(np.uint8)
    masks[0, :, 447:449] = 1                                               # whole columns on both sides of the seam
    masks[1] = 1
    masks[2] ^= (rng.random((H, W)) < 0.01).astype(np.uint8)
    t = _tensor(masks, False)
    rle = handoff.RleMasks.from_masks(t)
    recs = rle.to_records()
    assert recs == handoff.masks_to_rle(t)
    assert [r["counts"] for r in recs] == [R.encode(m.tolist()) for m in masks]
    got_p, got_a = rle.packed()
    want_p, want_a = dev_ops.mask_pack(t)
    assert torch.equal(got_p, want_p) and torch.equal(got_a, want_a)
    for n in range(N):
        ws, area = R.packed(masks[n].tolist())
        assert int(got_a[n]) == area and got_p[n].tolist() == [R.signed64(w) for w in ws]
    assert torch.equal(rle.to_dense().view(torch.uint8), torch.from_numpy(masks).cuda())
