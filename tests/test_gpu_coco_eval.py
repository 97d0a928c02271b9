"""The COCO AP kernels (csrc/s6d_cocoeval.hip) and sam6d_amd.evaluation on top of them against the plain-loop restatement of
tests/coco_ref.py.  Everything is compared with `equal`: the counts are integers, both IoUs are single float64 operation chains,
the matching is a decision, and AP is float64 arithmetic on integers in a stated order.  pycocotools is not present; nothing here
is compared with it.  The bodies take `ops` so that tests/test_emu_coco_eval.py runs them on the host build."""
import functools

import numpy as np
import pytest
import torch

from tests import coco_ref as C

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 9), (8, 8), (5, 13), (3, 43), (48, 64)]                # 1, 63, 64, 65, 129 and 3072 pixels
TWO_CHUNKS = (3, 43691)                                                     # 131073 pixels = 2049 words: two chunks of the pair kernel
KERNELS = "mask_pack,mask_pair_inter,box_pair_iou,coco_match"
T, RANGES = C.THRESHOLDS, list(C.AREAS.values())


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from sam6d_amd import ops
    return ops


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                 # (a copy: the cached cases are read-only)


def _np(t):
    return t.cpu().numpy()


def _dev():
    return torch.zeros(1).cuda().device                                     # (the emulator fixture leaves tensors on the host)


# ---------------------------------------------------------------------------------------------------------------- packing, counts
@functools.lru_cache(maxsize=None)
def _masks(hw, N, seed=0):
    """Seeded masks of mixed density, computed once and only read: with N >= 3 the first is empty and the second full."""
    rs = np.random.RandomState(1000 * hw[0] + 10 * hw[1] + N + seed)
    m = rs.uniform(size=(N,) + hw) < rs.uniform(0.05, 0.95, (N, 1, 1))
    if N >= 3:
        m[0], m[1] = False, True
    m.setflags(write=False)
    return m


def _words(mask):
    return np.array(C.pack(mask), np.uint64).view(np.int64)


def check_pack(ops, hw, N):
    m = _masks(hw, N)
    for dtype in (np.uint8, bool):
        src = m.astype(dtype) * (dtype(3) if dtype is np.uint8 else True)      # any non-zero byte is a set pixel
        packed, area = ops.mask_pack(_t(src))
        torch.cuda.synchronize()
        assert tuple(packed.shape) == (N, (hw[0] * hw[1] + 63) // 64) and packed.dtype == torch.int64 and area.dtype == torch.int32
        assert np.array_equal(_np(packed), np.stack([_words(x) for x in m]))
        assert np.array_equal(_np(area), m.reshape(N, -1).sum(1))
    tail = hw[0] * hw[1] % 64
    if tail:
        assert (_np(packed)[:, -1].view(np.uint64) >> np.uint64(tail) == 0).all()        # the bits past H W


@functools.lru_cache(maxsize=None)
def _pair_case(hw, N, P):
    d, g = _masks(hw, N, 1), _masks(hw, N, 2).copy()
    g[-1] = d[-1]                                                           # an equal pair of masks
    rs = np.random.RandomState(P + N)
    pairs = np.stack([np.sort(rs.randint(0, N, P)), rs.randint(0, N, P)], 1).astype(np.int32)      # runs of one detection row
    if P:
        pairs[-1] = (N - 1, N - 1)
    inter = np.array([C.mask_counts(d[a], g[b])[0] for a, b in pairs], np.int32).reshape(P)
    return d, g, pairs, inter


def check_pair_inter(ops, hw, N, P):
    """The restatement's counts; the same bits for the list permuted, for the list doubled and for every 16th pair alone."""
    d, g, pairs, ref = _pair_case(hw, N, P)
    dp, da = ops.mask_pack(_t(d))
    gp, ga = ops.mask_pack(_t(g))
    got = _np(ops.mask_pair_inter(dp, gp, _t(pairs)))
    assert got.dtype == np.int32 and np.array_equal(got, ref)
    if P == 0:
        return
    assert ref[-1] == d[-1].sum()                                           # equal masks: the intersection is the area
    perm = np.random.RandomState(7).permutation(P)
    assert np.array_equal(_np(ops.mask_pair_inter(dp, gp, _t(pairs[perm]))), ref[perm])
    twice = np.concatenate([pairs[::-1], pairs])
    assert np.array_equal(_np(ops.mask_pair_inter(dp, gp, _t(twice))), np.concatenate([ref[::-1], ref]))
    for p in range(0, P, 16):
        assert _np(ops.mask_pair_inter(dp, gp, _t(pairs[p:p + 1])))[0] == ref[p]
    from sam6d_amd import evaluation
    iou = _np(evaluation.mask_ious(_t(d), _t(g), pairs, device=_dev()))
    assert iou.dtype == np.float64 and np.array_equal(iou, np.array([C.mask_iou(d[a], g[b]) for a, b in pairs]))


def check_long_runs(ops):
    """One detection row 257 pairs long (segments cut at multiples of 64), then runs of 63, 64 and 65 pairs."""
    hw, N = (5, 13), 3
    d, g = _masks(hw, N, 1), _masks(hw, N, 2)
    rs = np.random.RandomState(3)
    for runs in ([(2, 257)], [(0, 63), (1, 64), (2, 65), (1, 1), (2, 130)], [(1, 5), (2, 200), (0, 64), (0, 0), (1, 127), (2, 128)]):
        pairs = np.concatenate([np.stack([np.full(n, r), rs.randint(0, N, n)], 1) for r, n in runs]).astype(np.int32)
        ref = np.array([C.mask_counts(d[a], g[b])[0] for a, b in pairs], np.int32)
        dp, gp = ops.mask_pack(_t(d))[0], ops.mask_pack(_t(g))[0]
        assert np.array_equal(_np(ops.mask_pair_inter(dp, gp, _t(pairs))), ref), runs


# ---------------------------------------------------------------------------------------------------------------- boxes
BOXES = dict(touching=((10.0, 10.0, 5.0, 5.0), (15.0, 12.0, 4.0, 4.0)), touching_below=((10.0, 10.0, 5.0, 5.0), (11.0, 15.0, 4.0, 4.0)),
             apart=((0.0, 0.0, 3.0, 3.0), (10.0, 10.0, 3.0, 3.0)), nested=((10.0, 10.0, 20.0, 30.0), (15.0, 15.0, 5.0, 7.0)),
             identical=((3.25, 7.5, 11.125, 13.0625), (3.25, 7.5, 11.125, 13.0625)), zero_area=((5.0, 5.0, 0.0, 9.0), (4.0, 4.0, 6.0, 6.0)),
             both_zero=((5.0, 5.0, 0.0, 0.0), (5.0, 5.0, 0.0, 0.0)),
             fractional=((101.30000305175781, 57.70000076293945, 43.400001525878906, 88.0999984741211), (99.5, 60.25, 50.75, 80.1)),
             thirds=((0.1, 0.2, 0.7, 0.3), (0.3, 0.1, 0.7, 0.6)))


def check_box_iou(ops):
    from sam6d_amd import evaluation
    names = sorted(BOXES)
    rs = np.random.RandomState(5)
    rnd_d = np.concatenate([rs.uniform(0, 600, (40, 2)), rs.uniform(1, 200, (40, 2))], 1).astype(np.float32).astype(np.float64)
    rnd_g = rnd_d + rs.uniform(-20, 20, (40, 4))                           # result files carry float32 values, ground truth integers
    db = np.concatenate([np.array([BOXES[n][0] for n in names]), rnd_d])
    gb = np.concatenate([np.array([BOXES[n][1] for n in names]), rnd_g])
    pairs = np.stack([np.arange(len(db)), np.arange(len(db))], 1).astype(np.int32)
    pairs = np.concatenate([pairs, np.stack([rs.randint(0, len(db), 208), rs.randint(0, len(db), 208)], 1).astype(np.int32)])      # P = 257
    ref = np.array([C.box_iou(db[a], gb[b]) for a, b in pairs])
    r = dict(zip(names, ref))
    # the restatement alone: every case holds its situation
    assert r["touching"] == 0 and r["touching_below"] == 0 and r["apart"] == 0 and r["zero_area"] == 0 and r["both_zero"] == 0
    assert r["identical"] == 1.0 and r["nested"] == 35.0 / 600.0 and 0 < r["fractional"] < 1 and 0 < r["thirds"] < 1
    assert min(BOXES["touching"][0][0] + BOXES["touching"][0][2], 1e9) - BOXES["touching"][1][0] == 0          # w == 0 exactly
    assert (ref > 0).sum() > 40 and (ref == 0).sum() > 10                  # the 40 jittered pairs and more overlap, the far ones do not
    got = _np(ops.box_pair_iou(_t(db), _t(gb), _t(pairs)))
    assert got.dtype == np.float64 and np.array_equal(got, ref)
    perm = rs.permutation(len(pairs))
    assert np.array_equal(_np(ops.box_pair_iou(_t(db), _t(gb), _t(pairs[perm]))), ref[perm])
    for p in (0, 5, 100, 256):
        assert _np(ops.box_pair_iou(_t(db), _t(gb), _t(pairs[p:p + 1])))[0] == ref[p]             # alone as in the batch
    assert _np(ops.box_pair_iou(_t(db), _t(gb), _t(pairs[:0]))).shape == (0,)
    assert np.array_equal(_np(evaluation.box_ious(db, gb, pairs, device=_dev())), ref)


# ---------------------------------------------------------------------------------------------------------------- matching
def _group(D, G, seed):
    """One group's arrays: IoUs on a grid of sixteenths (ties), ground truths of every size and some flagged."""
    rs = np.random.RandomState(seed)
    iou = rs.randint(0, 17, (D, G)) / 16.0
    return dict(iou=iou, det_area=rs.choice([10.0, 1024.0, 1025.0, 5000.0, 9216.0, 20000.0], D),
                gt_area=rs.choice([10.0, 1024.0, 1025.0, 5000.0, 9216.0, 9217.0, 20000.0], G), gt_ignore=rs.uniform(size=G) < 0.25)


def _special_groups():
    tie = dict(iou=np.array([[0.75, 0.75]]), det_area=np.array([500.0]), gt_area=np.array([500.0, 500.0]), gt_ignore=np.array([False, False]))
    exact = dict(iou=np.array([[1 / 2, 0, 0], [0, 3 / 5, 0], [0, 0, 9 / 10]]), det_area=np.full(3, 500.0), gt_area=np.full(3, 500.0),
                 gt_ignore=np.zeros(3, bool))
    passed = dict(iou=np.array([[0.95, 0.6]]), det_area=np.array([500.0]), gt_area=np.array([500.0, 500.0]), gt_ignore=np.array([True, False]))
    only_ignored = dict(iou=np.array([[0.8, 0.1]]), det_area=np.array([500.0]), gt_area=np.array([500.0, 500.0]), gt_ignore=np.array([True, False]))
    return dict(tie=tie, exact=exact, passed=passed, only_ignored=only_ignored)


def _ref_match(groups):
    """(match (Dn,10,4), ignore (Dn,10,4), events) by the restatement."""
    ms, igs, events = [], [], set()
    for g in groups:
        D = len(g["det_area"])
        m, i = np.full((D, len(T), len(RANGES)), -1, np.int32), np.zeros((D, len(T), len(RANGES)), np.uint8)
        for ti, t in enumerate(T):
            for ai, (lo, hi) in enumerate(RANGES):
                a, b = C.match_group(g["iou"].tolist(), g["det_area"], g["gt_area"], g["gt_ignore"], t, lo, hi, events)
                m[:, ti, ai], i[:, ti, ai] = a, b
        ms.append(m)
        igs.append(i)
    return np.concatenate(ms), np.concatenate(igs), events


def _tables(groups):
    Dg, Gg = np.array([len(g["det_area"]) for g in groups]), np.array([len(g["gt_area"]) for g in groups])
    table = np.stack([np.cumsum(Dg) - Dg, Dg, np.cumsum(Gg) - Gg, Gg], 1).astype(np.int32)
    off = (np.cumsum(Dg * Gg) - Dg * Gg).astype(np.int64)
    cat = lambda k, dt: np.concatenate([np.asarray(g[k], dt).reshape(-1) for g in groups])
    return cat("iou", np.float64), off, table, cat("det_area", np.float64), cat("gt_area", np.float64), cat("gt_ignore", np.uint8)


def _ops_match(ops, groups):
    iou, off, table, da, ga, gi = _tables(groups)
    m, i = ops.coco_match(_t(iou), _t(off), _t(table), _t(da), _t(ga), _t(gi), _t(T), _t(np.array(RANGES)))
    torch.cuda.synchronize()
    return _np(m), _np(i)


def check_match_special(ops):
    """The situations one at a time; the restatement alone asserts that each case holds its situation."""
    sp = _special_groups()
    for name, want in (("tie", "tie"), ("passed", "passed_over_ignored"), ("only_ignored", "matched_ignored")):
        rm, ri, ev = _ref_match([sp[name]])
        assert want in ev, (name, ev)
        m, i = _ops_match(ops, [sp[name]])
        assert np.array_equal(m, rm) and np.array_equal(i, ri), name
    rm, ri, _ = _ref_match([sp["tie"]])
    assert rm[0, 0, 0] == 1                                                 # of equal IoUs the later ground truth
    rm, ri, _ = _ref_match([sp["passed"]])
    assert rm[0, 0, 0] == 1 and ri[0, 0, 0] == 0 and rm[0, 3, 0] == 0 and ri[0, 3, 0] == 1        # at 0.65 only the ignored one is left
    rm, ri, _ = _ref_match([sp["only_ignored"]])
    assert rm[0, 0, 0] == 0 and ri[0, 0, 0] == 1
    rm, ri, _ = _ref_match([sp["exact"]])
    assert T[0] == 0.5 and T[8] == 0.8999999999999999 and 9 / 10 >= T[8]
    assert rm[0, 0, 0] == 0 and rm[0, 1, 0] == -1                           # 1/2 matches at 0.5 and not at 0.55
    assert rm[1, 2, 0] == (1 if 3 / 5 >= T[2] else -1) and rm[1, 3, 0] == -1
    assert rm[2, 8, 0] == 2 and rm[2, 9, 0] == -1                           # 9/10 matches at 0.8999999999999999
    m, i = _ops_match(ops, [sp["exact"]])
    assert np.array_equal(m, rm) and np.array_equal(i, ri)


def check_match_sizes(ops, D, G):
    """D detections against G ground truths, three such groups in one call and the middle one alone."""
    groups = [_group(D, G, 100 * D + G), _group(max(D - 1, 0), G, 7 + G), _group(D, max(G - 1, 0), 9 + D)]
    rm, ri, ev = _ref_match(groups)
    if D >= 10 and G >= 10:
        assert {"tie", "taken", "gt_outside", "det_outside", "matched_ignored", "passed_over_ignored"} <= ev, ev
    m, i = _ops_match(ops, groups)
    assert m.dtype == np.int32 and i.dtype == np.uint8
    assert np.array_equal(m, rm) and np.array_equal(i, ri), (D, G)
    d0, n = len(groups[0]["det_area"]), len(groups[1]["det_area"])
    m1, i1 = _ops_match(ops, groups[1:2])
    assert np.array_equal(m1, rm[d0:d0 + n]) and np.array_equal(i1, ri[d0:d0 + n])


def check_match_oversize(ops):
    """65 ground truths: refused by the kernel's wrapper, served by the library statement with the restatement's answer; next to a
    small group in one call of the module."""
    from sam6d_amd import evaluation
    groups = [_group(12, 65, 1), _group(9, 7, 2)]
    rm, ri, _ = _ref_match(groups)
    iou, off, table, da, ga, gi = _tables(groups)
    with pytest.raises(ValueError, match="S6D_COCO_MATCH_MAX_GT"):
        _ops_match(ops, groups)
    m, i = evaluation.coco_match(_t(iou), off, table, _t(da), _t(ga), gi, device=_dev())
    assert np.array_equal(_np(m), rm) and np.array_equal(_np(i), ri)


# ---------------------------------------------------------------------------------------------------------------- scores
def _rect(hw, y, x, h, w):
    m = np.zeros(hw, bool)
    m[y:y + h, x:x + w] = True
    return m


def _box(m):
    ys, xs = np.nonzero(m)
    return (float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)) if len(ys) else (0.0, 0.0, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def _scene(seed=0, hw=(48, 64), images=3, cats=3, extra=0):
    """A seeded multi-image, multi-category set: jittered rectangles, equal scores, an ignored instance, a category without ground
    truth (cats + 1, detections only), one without detections; ``extra`` more detections in the first group (101: truncation)."""
    rs = np.random.RandomState(seed)
    dets, gts = [], []
    for im in range(images):
        for cat in range(1, cats + 1):
            for j in range(rs.randint(1, 4)):
                h, w = rs.randint(3, 30), rs.randint(3, 40)
                y, x = rs.randint(0, hw[0] - h), rs.randint(0, hw[1] - w)
                m = _rect(hw, y, x, h, w)
                gts.append(dict(im=im, cat=cat, mask=m, box=_box(m), ignore=bool(rs.uniform() < 0.2)))
                for k in range(rs.randint(0, 3) if cat < cats else 0):
                    dy, dx = rs.randint(-2, 3, 2)
                    dm = _rect(hw, max(y + dy, 0), max(x + dx, 0), h, w)
                    b = _box(dm)
                    dets.append(dict(im=im, cat=cat, score=float(rs.randint(1, 8)) / 8.0, mask=dm,
                                     box=(b[0] + 0.25, b[1] - 0.5, b[2] + 0.125, b[3])))
        m = _rect(hw, 5, 5, 9, 9)
        dets.append(dict(im=im, cat=cats + 1, score=0.5, mask=m, box=_box(m)))
    m, dm = _rect(hw, 6, 20, 36, 36), _rect(hw, 8, 21, 36, 36)                # a medium object (1296 pixels) and its detection
    gts.append(dict(im=1, cat=1, mask=m, box=_box(m), ignore=False))
    dets.append(dict(im=1, cat=1, score=0.7, mask=dm, box=_box(dm)))
    g0 = gts[0]
    for k in range(extra):
        m = _rect(hw, k % 40, (3 * k) % 50, 4 + k % 5, 6)
        dets.append(dict(im=g0["im"], cat=g0["cat"], score=float(k % 13) / 16.0, mask=m, box=_box(m)))
    return dets, gts


def _dicts(dets, gts, dev):
    hw = (gts + dets)[0]["mask"].shape
    stack = lambda xs, k, dt, shape: np.array([x[k] for x in xs], dt).reshape((len(xs),) + shape)
    d = dict(im=stack(dets, "im", np.int64, ()), category=stack(dets, "cat", np.int64, ()), score=stack(dets, "score", np.float64, ()),
             masks=torch.from_numpy(stack(dets, "mask", bool, hw)).to(dev), bbox=stack(dets, "box", np.float64, (4,)))
    g = dict(im=stack(gts, "im", np.int64, ()), category=stack(gts, "cat", np.int64, ()), masks=stack(gts, "mask", bool, hw),
             bbox=stack(gts, "box", np.float64, (4,)), ignore=stack(gts, "ignore", bool, ()))
    return d, g


def check_scores(ops, monkeypatch, extra=0):
    """Kernel route = library route = restatement, segm and bbox, every reported number with `equal`."""
    from sam6d_amd import evaluation
    dets, gts = _scene(extra=extra)
    d, g = _dicts(dets, gts, _dev())
    calls = []
    for name in KERNELS.split(","):
        monkeypatch.setattr(ops, name, (lambda f, n: lambda *a: (calls.append(n), f(*a))[1])(getattr(ops, name), name))
    for iou_type in ("segm", "bbox"):
        events = set()
        ref = C.coco_scores(dets, gts, iou_type, events)
        assert {"equal_scores", "taken", "gt_outside", "det_outside", "matched_ignored"} <= events and ("truncated" in events) == (extra > 0), events
        assert 0 < ref["AP"] < 1 and ref["AP_small"] >= 0 and ref["AP_medium"] >= 0 and ref["AP_large"] == -1 and ref["ignored"] > 0
        del calls[:]
        got = evaluation.coco_scores(d, g, iou_type, device=_dev())
        assert set(calls) == ({"mask_pack", "mask_pair_inter", "coco_match"} if iou_type == "segm" else {"box_pair_iou", "coco_match"}), calls
        assert got == ref, (got, ref)
        monkeypatch.setenv("S6D_DISABLE_FUSED", KERNELS)
        del calls[:]
        lib = evaluation.coco_scores(d, g, iou_type, device=_dev())
        monkeypatch.delenv("S6D_DISABLE_FUSED")
        assert not calls and lib == ref, (lib, ref)


def check_scores_known_answers(ops):
    """Known answers on 112 x 128 frames with a small (10 x 10), a medium (40 x 40) and a large (100 x 100) object, one category each.

    lone      every detection is its ground truth's mask, ONE true positive per category: recall 1 / 1, AR1 = AR10 = AR100 = 1
              exactly.  precision = 1 / (1 + 0 + eps), eps = 2^-52, and 1 + 2^-52 is a float64: every sampled precision is
              1 - 2^-52, so the APs are a mean of such values, just below 1 (equal to the restatement's bits; the perfect set whose
              APs are exactly 1 is check_scores_perfect below).
    none      no detection: recall 0 and precision 0 at every level: every AP of a range with ground truths and every AR = 0.
    fp first  one ground truth; a false positive (IoU 0) scored above the true positive (IoU 1): tp = 0, 1 and fp = 1, 1, recall
              0, 1, precision 0 / 1 = 0, 1 / (2 + eps) = 0.5 (2 + eps rounds to 2); made non-increasing from the right: 0.5, 0.5;
              every recall level samples 0.5: AP = AP50 = AP75 = 0.5.  AR100 = 1, AR1 = 0 (the first detection is the false one).
    ignored   every ground truth flagged: no category has a positive: every number is -1."""
    from sam6d_amd import evaluation
    hw = (112, 128)
    masks = [_rect(hw, 1, 1, 10, 10), _rect(hw, 5, 60, 40, 40), _rect(hw, 10, 20, 100, 100)]
    gts = [dict(im=0, cat=c + 1, mask=m, box=_box(m), ignore=False) for c, m in enumerate(masks)]
    perfect = [dict(im=0, cat=c + 1, score=0.9, mask=m, box=_box(m)) for c, m in enumerate(masks)]
    keys = ("AP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large", "AR1", "AR10", "AR100")
    dev = _dev()

    def run(dets, gts, iou_type):
        d, g = _dicts(dets, gts, dev) if dets else (dict(im=np.zeros(0, np.int64), category=np.zeros(0, np.int64), score=np.zeros(0),
                                                         masks=torch.zeros((0,) + hw, dtype=torch.bool, device=dev), bbox=np.zeros((0, 4))),
                                                    _dicts(perfect, gts, dev)[1])
        got = evaluation.coco_scores(d, g, iou_type, device=dev)
        assert got == C.coco_scores(dets, gts, iou_type), iou_type
        return got
    for iou_type in ("segm", "bbox"):
        got = run(perfect, gts, iou_type)
        assert all(got[k] == 1.0 for k in keys[6:]) and all(got[k] < 1.0 for k in keys[:6]), got
        got = run([], gts, iou_type)
        assert all(got[k] == 0.0 for k in keys) and got["detections"] == 0, got
        far = _rect(hw, 80, 100, 10, 10)
        got = run([dict(im=0, cat=1, score=0.9, mask=far, box=_box(far)), dict(im=0, cat=1, score=0.8, mask=masks[0], box=_box(masks[0]))],
                  gts[:1], iou_type)
        assert got["AP"] == 0.5 and got["AP50"] == 0.5 and got["AP75"] == 0.5 and got["AP_small"] == 0.5, got
        assert got["AP_medium"] == -1 and got["AP_large"] == -1 and got["AR100"] == 1.0 and got["AR10"] == 1.0 and got["AR1"] == 0.0, got
        got = run(perfect, [dict(x, ignore=True) for x in gts], iou_type)
        assert all(got[k] == -1.0 for k in keys) and got["ignored"] == 3, got


def check_scores_perfect(ops):
    """Perfect detections: every AP and AR100 = 1, exactly.

    Two 112 x 128 images, each with a small (10 x 10), a medium (40 x 40) and a large (100 x 100) instance of object 1 and a medium
    instance of object 2; every detection is its ground truth's mask and box, the scores all different.  Per category and range
    there are at least TWO true positives and no false one: tp = 1, 2, ..., fp = 0.  precision = tp / (tp + fp + eps) with
    eps = 2^-52: the first is 1 / (1 + 2^-52) = 1 - 2^-52 (1 + 2^-52 is a float64), but from tp = 2 on tp + 2^-52 is a tie between tp
    and its neighbour and rounds to the even one, tp: those precisions are tp / tp = 1, and making the sequence non-increasing from
    the right lifts the first to 1 as well.  Every recall level samples 1, and a mean of ones is 1: AP = AP50 = AP75 = AP_small =
    AP_medium = AP_large = 1.  The last recall is n / n: AR100 = AR10 = 1; AR1 is not 1 (object 1 has three instances per image and
    one detection is kept).  With a LONE true positive per category the precision stays 1 - 2^-52 and the AP just below 1: that
    case is in check_scores_known_answers, against the restatement."""
    from sam6d_amd import evaluation
    hw = (112, 128)
    masks = [(1, _rect(hw, 1, 1, 10, 10)), (1, _rect(hw, 5, 60, 40, 40)), (1, _rect(hw, 10, 20, 100, 100)), (2, _rect(hw, 60, 5, 40, 40))]
    gts = [dict(im=im, cat=c, mask=m, box=_box(m), ignore=False) for im in range(2) for c, m in masks]
    dets = [dict(im=g["im"], cat=g["cat"], score=(k + 1) / 16.0, mask=g["mask"], box=g["box"]) for k, g in enumerate(gts)]
    assert [int(g["mask"].sum()) for g in gts[:4]] == [100, 1600, 10000, 1600]                  # small, medium, large, medium
    for iou_type in ("segm", "bbox"):
        d, g = _dicts(dets, gts, _dev())
        got = evaluation.coco_scores(d, g, iou_type, device=_dev())
        print(f"[coco perfect detections, {iou_type}] " + ", ".join(f"{k} {got[k]!r}" for k in got if k.startswith("A")))
        assert got == C.coco_scores(dets, gts, iou_type)
        assert all(got[k] == 1.0 for k in ("AP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large", "AR10", "AR100")), got
        assert 0.5 < got["AR1"] < 1.0, got                  # object 1: 2 of 6, object 2: 2 of 2 (the bits: the restatement, above)


# ---------------------------------------------------------------------------------------------------------------- arguments
def check_arguments(ops):
    from sam6d_amd import _lib
    m = _t(np.zeros((2, 4, 5), np.uint8))
    packed, area = ops.mask_pack(m)
    pairs = _t(np.zeros((1, 2), np.int32))
    with pytest.raises(RuntimeError, match="masks must be"):
        ops.mask_pack(m.float())
    with pytest.raises(RuntimeError, match="3 dimensions"):
        ops.mask_pack(m[0])
    with pytest.raises(ValueError, match="H W >= 1"):
        ops.mask_pack(m[:, :0])
    with pytest.raises(RuntimeError, match="det_packed must be"):
        ops.mask_pair_inter(packed.int(), packed, pairs)
    with pytest.raises(ValueError, match="words"):
        ops.mask_pair_inter(packed, torch.cat([packed, packed], 1), pairs)
    with pytest.raises(RuntimeError, match="pairs must be an int"):
        ops.mask_pair_inter(packed, packed, pairs.long())
    with pytest.raises(ValueError, match=r"pairs \(P,2\)"):
        ops.mask_pair_inter(packed, packed, _t(np.zeros((1, 3), np.int32)))
    for bad in ((2, 0), (0, 2), (-1, 0)):
        with pytest.raises(ValueError, match="pairs must index"):
            ops.mask_pair_inter(packed, packed, _t(np.array([bad], np.int32)))
    boxes = _t(np.ones((2, 4)))
    with pytest.raises(RuntimeError, match="det_boxes must be"):
        ops.box_pair_iou(boxes.float(), boxes, pairs)
    with pytest.raises(ValueError, match=r"\(Nd,4\)"):
        ops.box_pair_iou(boxes[:, :3].contiguous(), boxes, pairs)
    with pytest.raises(ValueError, match="pairs must index"):
        ops.box_pair_iou(boxes, boxes, _t(np.array([[0, 2]], np.int32)))
    iou, off, table, da, ga, gi = (_t(a) for a in _tables([_group(3, 2, 0)]))
    th, ar = _t(T), _t(np.array(RANGES))
    with pytest.raises(RuntimeError, match="ious must be"):
        ops.coco_match(iou.float(), off, table, da, ga, gi, th, ar)
    with pytest.raises(RuntimeError, match="gt_ignore must be"):
        ops.coco_match(iou, off, table, da, ga, gi.bool(), th, ar)
    with pytest.raises(ValueError, match="NT NA <= 64"):
        ops.coco_match(iou, off, table, da, ga, gi, torch.cat([th] * 2), ar)
    with pytest.raises(ValueError, match="outside"):
        ops.coco_match(iou[:-1].contiguous(), off, table, da, ga, gi, th, ar)
    with pytest.raises(ValueError, match="outside"):
        ops.coco_match(iou, off, table, da[:-1].contiguous(), ga, gi, th, ar)
    # the entry points themselves: sizes and NULL operands are refused before anything is launched, zero work returns 0
    EINVAL, EUNSUPPORTED = -1, -3
    p = packed.data_ptr()
    f = lambda name, *a: ops._fn(name, len(a))(*a)
    assert f("s6d_mask_pack_u8", None, 0, 20, None, None, None) == 0
    assert f("s6d_mask_pack_u8", None, 2, 20, p, p, None) == EINVAL and f("s6d_mask_pack_u8", p, 2, 0, p, p, None) == EINVAL
    assert f("s6d_mask_pack_u8", p, -1, 20, p, p, None) == EINVAL and f("s6d_mask_pack_u8", p, 2, 2 ** 31, p, p, None) == EUNSUPPORTED
    assert f("s6d_mask_pair_inter", None, 2, None, 2, 1, None, 0, None, None) == 0
    assert f("s6d_mask_pair_inter", p, 2, p, 2, 1, None, 1, p, None) == EINVAL and f("s6d_mask_pair_inter", p, 2, p, 2, 0, p, 1, p, None) == EINVAL
    assert f("s6d_mask_pair_inter", p, 0, p, 2, 1, p, 1, p, None) == EINVAL and f("s6d_mask_pair_inter", p, 2, p, 2, 1, p, -1, p, None) == EINVAL
    assert f("s6d_mask_pair_inter", p, 2, p, 2, 2 ** 25, p, 1, p, None) == EUNSUPPORTED
    assert f("s6d_box_pair_iou_f64", None, 2, None, 2, None, 0, None, None) == 0
    assert f("s6d_box_pair_iou_f64", p, 2, None, 2, p, 1, p, None) == EINVAL and f("s6d_box_pair_iou_f64", p, 2, p, 0, p, 1, p, None) == EINVAL
    assert f("s6d_coco_match", None, None, None, None, None, None, None, 0, 10, 4, 5, 5, 5, None, None, None) == 0
    assert f("s6d_coco_match", p, p, p, p, p, p, p, 1, 10, 4, 5, 5, 5, None, p, None) == EINVAL
    assert f("s6d_coco_match", p, p, p, p, p, p, p, 1, 17, 4, 5, 5, 5, p, p, None) == EINVAL
    assert f("s6d_coco_match", p, p, p, p, None, p, p, 1, 10, 4, 5, 5, 5, p, p, None) == EINVAL
    assert _lib.header_constant("S6D_COCO_MATCH_MAX_GT") == 64


# ---------------------------------------------------------------------------------------------------------------- the GPU tests
@pytest.mark.parametrize("N", [1, 3, 65])
@pytest.mark.parametrize("hw", SHAPES + [TWO_CHUNKS])
def test_mask_pack_vs_restatement(ops, hw, N):
    if hw == TWO_CHUNKS and N == 65:
        N = 2
    check_pack(ops, hw, N)


@pytest.mark.parametrize("P", [0, 1, 257])
@pytest.mark.parametrize("N", [1, 3, 65])
@pytest.mark.parametrize("hw", SHAPES)
def test_mask_pair_inter_vs_restatement(ops, hw, N, P):
    check_pair_inter(ops, hw, N, P)


def test_mask_pair_inter_two_chunks(ops):
    check_pair_inter(ops, TWO_CHUNKS, 2, 257)


def test_mask_pair_inter_long_runs(ops):
    check_long_runs(ops)


def test_masks_at_480_x_640(ops):
    """The production frame: 4800 words, three chunks of the pair kernel."""
    check_pack(ops, (480, 640), 3)
    check_pair_inter(ops, (480, 640), 3, 257)


def test_box_pair_iou_vs_restatement(ops):
    check_box_iou(ops)


def test_match_situations(ops):
    check_match_special(ops)


@pytest.mark.parametrize("G", [0, 1, 64])
@pytest.mark.parametrize("D", [0, 1, 17, 100])
def test_match_vs_restatement(ops, D, G):
    check_match_sizes(ops, D, G)


def test_match_65_ground_truths_take_the_library_route(ops):
    check_match_oversize(ops)


@pytest.mark.parametrize("extra", [0, 101])
def test_scores_kernel_route_equals_library_route_equals_restatement(ops, monkeypatch, extra):
    check_scores(ops, monkeypatch, extra)


def test_scores_known_answers(ops):
    check_scores_known_answers(ops)


def test_scores_perfect_detections_give_one(ops):
    check_scores_perfect(ops)


def test_arguments(ops):
    check_arguments(ops)
