"""The overlay kernels (csrc/s6d_vis.hip) and sam6d_amd.visualize on top of them against the plain-loop restatement of
tests/vis_ref.py.  Every comparison is `equal`: all pixel work is integer, and the projection is pinned bit for bit (float32, one
rounding per operation).  No picture is compared with cv2's.  The bodies take an `api` (the kernels through `ops`, or the torch
statements of sam6d_amd/visualize.py), so that tests/test_emu_vis.py runs them on the host build of the kernels and
tests/test_host_vis.py on the torch statements.

Shapes: (5,7) is smaller than any tile, (16,64) exactly one paint tile, (17,65) one pixel over in both directions, (33,130) rows that
straddle 64-bit words, (48,200) several tiles.  A B = 1 case is frame 1 of the B = 3 case and is compared with that frame of the
B = 3 restatement (which treats the frames one by one): the restatement is computed once per shape, and a frame alone must have the
bits it has in the group."""
import functools

import numpy as np
import pytest
import torch

from sam6d_amd import visualize as V
from sam6d_amd.ism import handoff
from tests import render_ref as R
from tests import test_gpu_bop_gt as GT
from tests import vis_ref as REF

pytestmark = pytest.mark.gpu

SIZES = ((5, 7), (16, 64), (17, 65), (33, 130), (48, 200))
BATCHES = (1, 3)
OWNER_N = (0, 1, 2, 65)
# edge_width, alpha, gray, per-pixel shade (else the colour table)
PAINT_CONFIGS = ((0, 84, True, False), (1, 84, True, False), (2, 84, True, False), (4, 84, True, False), (2, 0, False, False),
                 (2, 256, True, False), (1, 84, False, True), (4, 256, True, True), (2, 0, True, True))
SCENE_HW = (48, 64)
ZNEAR = 1.0


class KernelApi:
    """The kernels through ``ops`` (the library on the GPU, or the emulator's through the `emu` fixture)."""

    def __init__(self, ops):
        self.ops = ops
        self.chunk = ops.vis_draw_chunk()

    @staticmethod
    def t(a):
        return torch.from_numpy(np.array(a, order="C")).cuda()           # a copy: draw and merge work in place

    def pack(self, masks):
        return self.ops.mask_pack(masks)[0]

    def owner(self, packed, order, start, H, W):
        return self.ops.vis_owner_from_masks(packed, order, start, H, W)

    def canvas(self, B, H, W):
        return self.ops.vis_canvas(B, H, W, self.t(np.zeros(1)).device)

    def merge(self, canvas, depth, rgb, frame, first):
        return self.ops.vis_merge_layers(canvas, depth, rgb, frame, first)

    def paint(self, *a, **k):
        return self.ops.vis_paint(*a, **k)

    def project(self, *a):
        return self.ops.vis_project(*a)

    def draw(self, image, prims, start, check=True):
        return self.ops.vis_draw(image, prims, start, check=check)


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available()
    from sam6d_amd import ops
    return KernelApi(ops)


def _np(t):
    return t.cpu().numpy()


def _frames(B):
    """Which frames of the B = 3 case a call with B frames takes."""
    return [1] if B == 1 else [0, 1, 2]


def _image(hw, seed=0):
    return np.random.RandomState(1000 * hw[0] + hw[1] + seed).randint(0, 256, (3, hw[0], hw[1], 3)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------- owner from masks
@functools.lru_cache(None)
def owner_case(hw, N):
    """N masks over 3 frames (mask n in frame n % 3) and the restatement's owner map.  N = 2: a rectangle and a mask that covers
    everything, in ONE frame, with equal scores (the lower index wins).  N = 65: random rectangles that overlap, few distinct scores
    (ties), mask 3 empty, mask 5 covering everything with the lowest score."""
    h, w = hw
    rs = np.random.RandomState(7 * h + w + N)
    masks = np.zeros((N, h, w), bool)
    frame = np.arange(N) % 3
    scores = (rs.randint(0, 4, N) / 4).astype(np.float32)
    for n in range(N):
        y0, x0 = rs.randint(0, h), rs.randint(0, w)
        masks[n, y0:y0 + rs.randint(1, h + 1), x0:x0 + rs.randint(1, w + 1)] = True
    if N == 2:
        frame[:] = 1
        scores[:] = 0.5
        masks[1] = True
    if N == 65:
        masks[3] = False
        masks[5] = True
        scores[5] = -1.0
    ref = REF.owner_from_masks(masks, REF.rank_order(scores, frame, 3), h, w)
    if N == 2:
        assert np.array_equal(ref[1], np.where(masks[0], 0, 1))           # equal scores: index 0 where it covers, 1 elsewhere
    if N == 65:
        assert (ref[2] >= 0).all() and 3 not in ref                       # mask 5 covers its frame; the empty mask owns nothing
    return masks, frame, scores, ref


def check_owner(api, hw, B, N):
    h, w = hw
    masks, frame, scores, ref = owner_case(hw, N)
    fr = _frames(B)
    sel = np.nonzero(np.isin(frame, fr))[0]
    m, f, s = masks[sel], np.searchsorted(fr, frame[sel]), scores[sel]
    dense = api.t(m.astype(np.uint8))
    if len(sel):
        packed = api.pack(dense)
        rle = handoff.RleMasks.from_masks(dense)
        assert torch.equal(rle.packed()[0], packed)                       # run lists and dense masks: the same words
        for given in (dense, rle, packed):
            assert torch.equal(V._packed(given, h, w, dense.device), packed)
    else:
        packed = torch.zeros(0, (h * w + 63) // 64, dtype=torch.int64, device=dense.device)
    order, start, _ = V.rank_detections(api.t(s), api.t(f.astype(np.int64)), B)
    assert [order[a:b].tolist() for a, b in zip(start[:-1].tolist(), start[1:].tolist())] == REF.rank_order(s, f, B)
    got = _np(api.owner(packed, order, start, h, w)).astype(np.int64)
    want = ref[fr]
    back = np.concatenate([sel, [-1]])                                    # the call's indices -> the case's; -1 stays
    assert np.array_equal(back[got], want)


# ------------------------------------------------------------------------------------------------------------------- merge
@functools.lru_cache(None)
def merge_case(hw):
    """7 layers over 3 frames with few distinct depths (equal depths at overlapping pixels), zeros and NaNs."""
    h, w = hw
    rs = np.random.RandomState(11 * h + w)
    T = 7
    depth = rs.choice(np.array([0.0, 300.0, 300.5, 301.0, np.nan], np.float32), (T, h, w), p=[0.4, 0.2, 0.15, 0.15, 0.1]).astype(np.float32)
    rgb = rs.randint(0, 256, (T, h, w, 3)).astype(np.uint8)
    frame = (np.arange(T) % 3).astype(np.int32)
    ref = REF.merge_layers(REF.empty_canvas(3, h, w), depth, rgb, frame, 0)
    assert ((depth[0] == depth[3]) & (depth[0] > 0)).any()                # layers 0 and 3 share frame 0: ties exist
    return depth, rgb, frame, ref


def check_merge(api, hw, B):
    h, w = hw
    depth, rgb, frame, ref = merge_case(hw)
    fr = _frames(B)
    sel = np.nonzero(np.isin(frame, fr))[0]                               # instance index = position in this call's list
    d, c, f = depth[sel], rgb[sel], np.searchsorted(fr, frame[sel]).astype(np.int32)
    T = len(sel)

    def run(chunks):
        canvas = api.canvas(B, h, w)
        for idx in chunks:
            api.merge(canvas, api.t(d[idx]), api.t(c[idx]), api.t(f[idx]), int(idx[0]))
        return {k: _np(v) for k, v in canvas.items()}
    whole = run([np.arange(T)])
    own = whole["owner"].astype(np.int64)
    back = np.concatenate([sel, [-1]])
    assert np.array_equal(back[own], ref["owner"][fr])
    has = own >= 0
    assert np.array_equal(whole["zbuf"][has].view(np.uint32), ref["zbuf"][fr][has].view(np.uint32))
    assert np.array_equal(whole["shade"], ref["shade"][fr])
    assert not whole["zbuf"][~has].any() and not whole["shade"][~has].any()
    for chunks in ([np.arange(t, t + 1) for t in range(T)], [np.arange(t, t + 1) for t in reversed(range(T))],
                   [np.arange(T // 2, T), np.arange(0, T // 2)]):
        other = run(chunks)
        assert all(np.array_equal(other[k].view(np.uint8), whole[k].view(np.uint8)) for k in whole), [len(x) for x in chunks]


# ------------------------------------------------------------------------------------------------------------------- paint
@functools.lru_cache(None)
def paint_inputs(hw):
    """An owner map with contours along and across the tile borders (x = 64, 128; y = 16, 32), along the image border, a region one
    pixel wide, ids up to 70, unowned ground; a shade image."""
    h, w = hw
    rs = np.random.RandomState(13 * h + w)
    owner = np.full((3, h, w), -1, np.int32)
    for b in range(3):
        owner[b, : h // 2, : w // 3] = b                                  # touches the top-left image border
        owner[b, :, min(w - 1, 63 + b):min(w, 64 + b)] = 7                # one pixel wide, on / beside the tile border
        owner[b, min(h - 1, 15):min(h, 17), w // 2:] = 70                 # straddles the tile border y = 16
        owner[b, h - 1, :] = 3                                            # the bottom image border
        blob = rs.uniform(size=(h, w)) < 0.05
        owner[b][blob] = rs.randint(0, 71, int(blob.sum()))
    owner[2, : min(h, 3), : min(w, 3)] = -7                               # any negative id is "none"
    shade = rs.randint(0, 256, (3, h, w, 3)).astype(np.uint8)
    colors = rs.randint(0, 256, (71, 3)).astype(np.uint8)
    return owner, shade, colors


@functools.lru_cache(None)
def paint_ref(hw, config):
    w_, alpha, gray, use_shade = config
    owner, shade, colors = paint_inputs(hw)
    return REF.paint(_image(hw), owner, colors=None if use_shade else colors, shade=shade if use_shade else None, alpha=alpha, gray=gray,
                     edge_width=w_, edge_color=(255, 255, 255) if w_ != 4 else (10, 200, 30))


def check_paint(api, hw, B, config):
    w_, alpha, gray, use_shade = config
    owner, shade, colors = paint_inputs(hw)
    fr = _frames(B)
    got = api.paint(api.t(_image(hw)[fr]), api.t(owner[fr]), colors=None if use_shade else api.t(colors), shade=api.t(shade[fr]) if use_shade else None,
                    alpha=alpha, gray=gray, edge_width=w_, edge_color=(255, 255, 255) if w_ != 4 else (10, 200, 30))
    assert np.array_equal(_np(got), paint_ref(hw, config)[fr])


def check_paint_known_answer(api):
    """A 3 x 3 mask in a 7 x 7 image with edge_width 1: exactly its 8 border pixels white, the centre blended:
    (84 * 255 + 172 * 100 + 128) >> 8 = 151 for colour 255 over grey 100, (84 * 0 + 172 * 100 + 128) >> 8 = 67 for colour 0."""
    img = np.full((1, 7, 7, 3), 100, np.uint8)
    owner = np.full((1, 7, 7), -1, np.int32)
    owner[0, 2:5, 2:5] = 0
    got = _np(api.paint(api.t(img), api.t(owner), colors=api.t(np.array([[255, 0, 0]], np.uint8)), alpha=84, gray=True, edge_width=1))
    want = np.full((7, 7, 3), 100, np.uint8)
    want[2:5, 2:5] = 255
    want[3, 3] = (151, 67, 67)
    assert np.array_equal(got[0], want)
    assert (got[0] == 255).all(2).sum() == 8


# ------------------------------------------------------------------------------------------------------------------- projection
@functools.lru_cache(None)
def project_case():
    rs = np.random.RandomState(5)
    N = 4
    Rm = R.rotations(N, 3).astype(np.float32)
    Rm[0] = Rm[3] = np.eye(3, dtype=np.float32)
    t = np.array([[0, 0, 400], [10, -5, 300], [-3, 2, 500], [0, 0, 0]], np.float32)
    cams = np.array([[60, 60, 32, 24], [600, 590, 320.5, 240.25], [60, 60, 32, 24], [60, 60, 32, 24]], np.float32)
    pts = rs.uniform(-50, 50, (300, 3)).astype(np.float32)               # in front of the camera; more than one workgroup
    inst = rs.randint(0, 3, 300).astype(np.int32)
    one, zn = np.float32(1.0), np.float32(ZNEAR)
    special = [([0, 0, np.nextafter(zn, np.float32(0))], 3), ([0, 0, zn], 3), ([0, 0, np.nextafter(zn, np.float32(2))], 3),   # around znear
               ([1, 1, 0], 3), ([1, 1, -5], 3), ([0, 0, -400], 0),                                                            # zc = 0, behind
               ([1e6, 0, 2], 3), ([-1e6, 0, 2], 3), ([0, 1e6, 2], 3), ([0, -1e6, 2], 3), ([3e38, 3e38, 1], 3),                 # beyond the clamp; inf
               ([137 * one, 0, 1], 3), ([-137 * one, 0, 1], 3),                                                               # 8252, -8188
               ([1, 2, 3], -1), ([1, 2, 3], 4)]                                                                               # no such instance
    pts = np.concatenate([pts, np.array([p for p, _ in special], np.float32)])
    inst = np.concatenate([inst, np.array([n for _, n in special], np.int32)])
    xy, valid = REF.project(pts, inst, Rm, t, cams, ZNEAR)
    assert valid[:300].all() and list(valid[300:306]) == [False, True, True, False, False, False]
    assert xy[306:310].tolist() == [[8191, 24], [-8192, 24], [32, 8191], [32, -8192]] and not valid[310] and not valid[-2:].any()
    assert xy[311].tolist() == [8191, 24] and xy[312].tolist() == [-8188, 24]
    return pts, inst, Rm, t, cams, xy, valid


def check_project(api):
    pts, inst, Rm, t, cams, xy, valid = project_case()
    gxy, gvalid = api.project(api.t(pts), api.t(inst), api.t(Rm), api.t(t), api.t(cams), ZNEAR)
    assert np.array_equal(_np(gvalid).astype(bool), valid)
    assert np.array_equal(_np(gxy).astype(np.int64), xy)


# ------------------------------------------------------------------------------------------------------------------- draw
def _word(r, g, b):
    return r | (g << 8) | (b << 16)


@functools.lru_cache(None)
def draw_prims(hw, chunk):
    """The primitive list of the three frames (sorted by frame) and the restatement's pictures."""
    h, w = hw
    lo, hi = REF.CLAMP_LO, REF.CLAMP_HI
    cx, cy = w // 2, h // 2
    rows = []
    for b in range(3):
        rows += [[b, 1, cy, w - 2, cy, 3, _word(250, 10, b), 1],          # horizontal
                 [b, cx, 0, cx, h - 1, 2, _word(10, 250, b), 1],          # vertical
                 [b, 0, 0, min(h, w) - 1, min(h, w) - 1, 1, _word(10, 10, 250), 1],      # diagonal
                 [b, 0, h - 1, w - 1, h - 1 - min(h - 1, 3), 3, _word(200, 200, b), 1],  # shallow
                 [b, cx, cy, cx, cy, 64, _word(90, 90, 90 + b), 1],       # a = b, the largest size
                 [b, w - 1, 0, w - 1, 0, 0, _word(1, 2, 3), 1],           # size 0: the pixel itself
                 [b, 2, 1, 5, 3, 0, _word(4, 5, 6), 1],                   # size 0: the pixels exactly on the segment
                 [b, 31, 7, 33, 9, 2, _word(7, 8, 9), 1],                 # across the corner of the draw tiles (32, 8)
                 [b, 63, 15, 65, 17, 3, _word(9, 8, 7), 1],               # across the corner of the paint tiles (64, 16)
                 [b, lo, cy, cx, cy - 1, 3, _word(20, 30, 40), 1],        # endpoints at the four clamp extremes
                 [b, hi, cy, cx, cy + 1, 3, _word(30, 40, 50), 1],
                 [b, cx, lo, cx - 1, cy, 2, _word(40, 50, 60), 1],
                 [b, cx + 1, cy, cx, hi, 2, _word(50, 60, 70), 1],
                 [b, lo, lo, hi, hi, 1, _word(60, 70, 80), 1],            # both ends at extremes: the largest products
                 [b, 1, 1, 2, 1, 3, _word(100, 0, 0), 1],                 # painter's order: three primitives over pixel (2, 1) ...
                 [b, 2, 0, 2, 2, 3, _word(0, 100, 0), 0],                 # ... an invalid one between valid ones
                 [b, 2, 1, 2, 1, 2, _word(0, 0, 100 + b), 1],
                 [b, 0, 1, 3, 1, 1, _word(0, 100, 100), 1]]
    # frame 1: one primitive more than a compaction chunk holds over one tile; the last one has to win at pixel (1, 0)
    rows += [[1, 0, 0, 1 + (k % 3), k % 2, 1, _word(k % 251, 77, 1), 1] for k in range(chunk)] + [[1, 1, 0, 1, 0, 0, _word(255, 254, 253), 1]]
    prims = np.asarray(sorted(rows, key=lambda e: e[0]), np.int64)       # (stable: the list order inside a frame stays)
    ref = REF.draw(_image(hw, seed=1), prims)
    assert ref[1, 0, 1].tolist() == [255, 254, 253] and ref[0, 1, 2].tolist() == [0, 100, 100]
    return prims, ref


def check_draw(api, hw, B):
    prims, ref = draw_prims(hw, api.chunk)
    fr = _frames(B)
    p = prims.copy()
    if B == 1:
        p = p[p[:, 0] == 1]
        p[:, 0] = 0
    start = np.concatenate([[0], np.cumsum(np.bincount(p[:, 0], minlength=B))]).astype(np.int64)
    got = api.draw(api.t(_image(hw, seed=1)[fr]), api.t(p.astype(np.int32)), api.t(start))
    assert np.array_equal(_np(got), ref[fr])


def check_draw_other_frames_and_empty(api):
    """Primitives filed under frame 1 whose frame field says 0 or 2 do not show anywhere; an empty list leaves the image as it is."""
    img = _image((17, 65), seed=2)
    rows = np.array([[0, 5, 5, 30, 9, 3, _word(1, 1, 1), 1], [1, 5, 5, 30, 9, 3, _word(2, 2, 2), 1], [2, 5, 5, 30, 9, 3, _word(3, 3, 3), 1]], np.int32)
    start = np.array([0, 0, 3, 3], np.int64)
    got = _np(api.draw(api.t(img), api.t(rows), api.t(start), check=False))          # (the wrapper's own check refuses such a list)
    want = REF.draw(img, rows[1:2])
    assert np.array_equal(got, want) and np.array_equal(got[[0, 2]], img[[0, 2]]) and not np.array_equal(got[1], img[1])
    got = _np(api.draw(api.t(img), api.t(np.zeros((0, 8), np.int32)), api.t(np.zeros(4, np.int64))))
    assert np.array_equal(got, img)


def check_draw_known_answer(api):
    """A disc of size 2 (radius 1) at (3, 3) is the 5-pixel plus."""
    img = np.zeros((1, 7, 7, 3), np.uint8)
    got = _np(api.draw(api.t(img), api.t(np.array([[0, 3, 3, 3, 3, 2, _word(9, 9, 9), 1]], np.int32)), api.t(np.array([0, 1], np.int64))))
    plus = np.zeros((7, 7), bool)
    plus[3, 2:5] = plus[2:5, 3] = True
    assert np.array_equal((got[0] == 9).all(2), plus) and plus.sum() == 5


# ------------------------------------------------------------------------------------------------------------------- whole pictures
def _models():
    cv, cf = GT._mesh("cube")
    tv, tf = GT._mesh("torus")
    return {1: dict(vertices=cv, faces=cf), 2: dict(vertices=tv, faces=tf)}


@functools.lru_cache(None)
def scene():
    """Three frames of SCENE_HW: the five cubes of ``instance_poses`` (inside, across the left border, outside, across the bottom
    border and nearer, inside and farther: it overlaps the first), the five tori, and a mix of both."""
    cam = np.array(GT.SIZES[SCENE_HW], np.float32)
    P = GT.instance_poses(SCENE_HW, cam, 5)
    obj = [1] * 5 + [2] * 5 + [1, 2, 2, 1]
    frame = [0] * 5 + [1] * 5 + [2] * 4
    poses = np.concatenate([P, P, P[[0, 4, 1, 3]]])
    return obj, np.array(frame), poses, cam


def _palette_by_position(frame):
    seen, pos = {}, []
    for f in frame.tolist():
        pos.append(seen.get(f, 0))
        seen[f] = pos[-1] + 1
    return _np(V.palette(max(pos) + 1))[pos]


def _layers(api, obj, poses, cam):
    """(depth, rgb, mask) per instance from ``ops.render_views``, object by object (the rasteriser is pinned by its own tests)."""
    h, w = SCENE_HW
    N = len(obj)
    depth, rgb, mask = np.zeros((N, h, w), np.float32), np.zeros((N, h, w, 3), np.uint8), np.zeros((N, h, w), np.uint8)
    for o, m in _models().items():
        idx = [n for n in range(N) if obj[n] == o]
        if not idx:
            continue
        r = api.ops.render_views(api.t(m["vertices"]), api.t(m["faces"]), api.t(np.full((len(m["vertices"]), 3), 200, np.uint8)), api.t(poses[idx]),
                                 *[float(v) for v in cam], h, w, 0.3, 0.7, ZNEAR)
        depth[idx], rgb[idx], mask[idx] = _np(r["depth"]), _np(r["rgb"]), _np(r["mask"])
    return depth, rgb, mask


def check_pose_pictures(api, mode, B):
    """overlay_poses == the restatement's picture: base, (surface: merged canvas painted with the shade,) primitives drawn."""
    h, w = SCENE_HW
    obj, frame, poses, cam = scene()
    fr = _frames(B)
    sel = np.nonzero(np.isin(frame, fr))[0]
    o, f, P = [obj[n] for n in sel], np.searchsorted(fr, frame[sel]), poses[sel]
    img = _image(SCENE_HW, seed=3)[fr]
    Rm, t = P[:, :3, :3].copy(), P[:, :3, 3].copy()
    cams = np.tile(cam, (len(sel), 1))
    colors = _palette_by_position(f)
    want = img.copy()
    if "surface" in mode:
        depth, rgb, _ = _layers(api, o, P, cam)
        canvas = REF.empty_canvas(B, h, w)
        for n in range(len(sel)):
            REF.merge_layers(canvas, depth[n:n + 1], rgb[n:n + 1], f[n:n + 1], n)
        assert len(np.unique(canvas["owner"])) > 3
        want = REF.paint(img, canvas["owner"], shade=canvas["shade"], alpha=84, gray=False, edge_width=1)
    prim_mode = tuple(m for m in mode if m != "surface")
    if prim_mode:
        want = REF.draw(want, REF.pose_primitives(_models(), o, Rm, t, cams, f, colors, prim_mode, znear=ZNEAR))
    assert not np.array_equal(want, img)
    K = np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1]], np.float32)
    got = V.overlay_poses(api.t(img), _models(), o, api.t(Rm), api.t(t), K, frame_index=f, mode=mode, znear=ZNEAR, chunk_bytes=3 * 24 * h * w)
    assert np.array_equal(_np(got), want)


def check_detection_pictures(api, top, B):
    """overlay_detections (dense masks, run lists, a list of Detections) == the restatement's picture."""
    h, w = SCENE_HW
    obj, frame, poses, cam = scene()
    fr = _frames(B)
    sel = np.nonzero(np.isin(frame, fr))[0]
    o, f = [obj[n] for n in sel], np.searchsorted(fr, frame[sel])
    masks = _layers(api, o, poses[sel], cam)[2].astype(bool)
    scores = np.array([0.5, 0.9, 0.5, 0.7, 0.5, 0.2, 0.8, 0.8, 0.1, 0.8, 0.3, 0.3, 0.6, 0.3], np.float32)[sel]
    img = _image(SCENE_HW, seed=4)[fr]
    ranked = REF.rank_order(scores, f, B, top)
    owner = REF.owner_from_masks(masks, ranked, h, w)
    table = np.zeros((len(sel), 3), np.uint8)
    pal = _np(V.palette(8))
    for idx in ranked:
        for k, n in enumerate(idx):
            table[n] = pal[k]
    want = REF.paint(img, owner, colors=table, alpha=84, gray=True, edge_width=2)
    assert not np.array_equal(want, img)
    dense = api.t(masks.astype(np.uint8))
    got = V.overlay_detections(api.t(img), dense, api.t(scores), frame_index=f, top=top)
    assert np.array_equal(_np(got), want)
    got = V.overlay_detections(api.t(img), handoff.RleMasks.from_masks(dense), api.t(scores), frame_index=f, top=top)
    assert np.array_equal(_np(got), want)
    dets = [handoff.Detections(0, b, dense[torch.from_numpy(f == b).to(dense.device)], None, api.t(scores[f == b]), None) for b in range(B)]
    assert np.array_equal(_np(V.overlay_detections(api.t(img), dets, top=top)), want)


def check_batch_invariance(api):
    """Each frame of a B = 3 call equals its B = 1 call, for both overlays (all three pose modes at once)."""
    h, w = SCENE_HW
    obj, frame, poses, cam = scene()
    img = _image(SCENE_HW, seed=5)
    K = np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1]], np.float32)
    masks = api.t(_layers(api, obj, poses, cam)[2])
    scores = api.t(np.linspace(0.1, 0.9, len(obj)).astype(np.float32))
    mode = ("surface", "box", "points")
    pem = V.overlay_poses(api.t(img), _models(), obj, api.t(poses[:, :3, :3].copy()), api.t(poses[:, :3, 3].copy()), K, frame_index=frame, mode=mode)
    ism = V.overlay_detections(api.t(img), masks, scores, frame_index=frame)
    for b in range(3):
        sel = np.nonzero(frame == b)[0]
        one = V.overlay_poses(api.t(img[b]), _models(), [obj[n] for n in sel], api.t(poses[sel, :3, :3].copy()), api.t(poses[sel, :3, 3].copy()), K, mode=mode)
        assert torch.equal(one, pem[b])
        one = V.overlay_detections(api.t(img[b]), masks[torch.from_numpy(sel).to(masks.device)], scores[torch.from_numpy(sel).to(masks.device)])
        assert torch.equal(one, ism[b])


# ------------------------------------------------------------------------------------------------------------------- arguments
def check_arguments(api):
    """Refused through the wrappers with a message that names the operand."""
    ops = api.ops
    img, owner = api.t(np.zeros((1, 4, 8, 3), np.uint8)), api.t(np.zeros((1, 4, 8), np.int32))
    col = api.t(np.zeros((1, 3), np.uint8))
    with pytest.raises(ValueError, match="H and W"):
        ops.vis_paint(api.t(np.zeros((1, 1, 8193, 3), np.uint8)), api.t(np.zeros((1, 1, 8193), np.int32)), colors=col)
    with pytest.raises(ValueError, match="H and W"):
        ops.vis_draw(api.t(np.zeros((1, 8193, 1, 3), np.uint8)), api.t(np.zeros((0, 8), np.int32)), api.t(np.zeros(2, np.int64)))
    with pytest.raises(ValueError, match="H and W"):
        ops.vis_owner_from_masks(api.t(np.zeros((0, 129), np.int64)), api.t(np.zeros(0, np.int32)), api.t(np.zeros(2, np.int64)), 1, 8193)
    with pytest.raises(ValueError, match="edge_width"):
        ops.vis_paint(img, owner, colors=col, edge_width=5)
    with pytest.raises(ValueError, match="alpha"):
        ops.vis_paint(img, owner, colors=col, alpha=257)
    with pytest.raises(ValueError, match="colors and shade"):
        ops.vis_paint(img, owner)
    prim = np.array([[0, 1, 1, 2, 2, 65, 0, 1]], np.int32)
    with pytest.raises(ValueError, match="size"):
        ops.vis_draw(img, api.t(prim), api.t(np.array([0, 1], np.int64)))
    prim[0, 5], prim[0, 0] = 3, 1
    with pytest.raises(ValueError, match="frame"):
        ops.vis_draw(img, api.t(prim), api.t(np.array([0, 1], np.int64)))
    with pytest.raises(ValueError, match="frame"):
        V.draw(img, api.t(prim))
    prim[0, 0], prim[0, 1] = 0, 8192
    with pytest.raises(ValueError, match="coordinates"):
        ops.vis_draw(img, api.t(prim), api.t(np.array([0, 1], np.int64)))
    with pytest.raises(ValueError, match="words"):
        ops.vis_owner_from_masks(api.t(np.zeros((1, 2), np.int64)), api.t(np.zeros(1, np.int32)), api.t(np.array([0, 1], np.int64)), 4, 8)
    with pytest.raises(ValueError, match="frame"):
        ops.vis_merge_layers(ops.vis_canvas(1, 4, 8, img.device), api.t(np.zeros((1, 4, 8), np.float32)), api.t(np.zeros((1, 4, 8, 3), np.uint8)),
                             api.t(np.array([1], np.int32)), 0)
    with pytest.raises(ValueError, match="frame_index"):
        V.overlay_detections(img, api.t(np.zeros((1, 4, 8), np.uint8)), api.t(np.ones(1, np.float32)), frame_index=[1])
    with pytest.raises(ValueError, match="frame_index"):
        V.overlay_poses(img, _models(), [1], api.t(np.eye(3, dtype=np.float32)[None]), api.t(np.zeros((1, 3), np.float32)), np.eye(3), frame_index=[-1])
    # the C entry points themselves: codes, before any launch
    p = img.data_ptr()
    paint_fn, draw_fn = ops._fn("s6d_vis_paint_u8", 16), ops._fn("s6d_vis_draw_u8", 8)
    assert paint_fn(p, p, p, None, 1, 1, 8193, 8, 1, 84, 2, 255, 255, 255, p, None) == -3
    assert paint_fn(p, p, p, None, 1, 1, 4, 8, 1, 84, 5, 255, 255, 255, p, None) == -1
    assert paint_fn(p, p, p, None, 1, 1, 4, 8, 1, 257, 2, 255, 255, 255, p, None) == -1
    assert draw_fn(p, p, 1, 1, 4, 8193, p, None) == -3


# ------------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("N", OWNER_N)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("hw", SIZES)
def test_owner_from_masks_vs_restatement(api, hw, B, N):
    check_owner(api, hw, B, N)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("hw", SIZES)
def test_merge_layers_vs_restatement_and_any_chunking(api, hw, B):
    check_merge(api, hw, B)


@pytest.mark.parametrize("config", PAINT_CONFIGS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("hw", SIZES)
def test_paint_vs_restatement(api, hw, B, config):
    check_paint(api, hw, B, config)


def test_paint_known_answer(api):
    check_paint_known_answer(api)


def test_projection_bits_vs_restatement(api):
    check_project(api)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("hw", SIZES)
def test_draw_vs_restatement(api, hw, B):
    check_draw(api, hw, B)


def test_draw_other_frames_and_empty_list(api):
    check_draw_other_frames_and_empty(api)


def test_draw_known_answer(api):
    check_draw_known_answer(api)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mode", [("box", "points"), ("surface",), ("surface", "box", "points")])
def test_pose_pictures_vs_restatement(api, mode, B):
    check_pose_pictures(api, mode, B)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("top", [1, None])
def test_detection_pictures_vs_restatement(api, top, B):
    check_detection_pictures(api, top, B)


def test_a_frame_alone_has_the_bits_it_has_in_the_group(api):
    check_batch_invariance(api)


def test_arguments(api):
    check_arguments(api)
