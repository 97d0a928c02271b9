"""Reference restatement of the template onboarding (sam6d_amd/onboarding.py) and the case table its tests share -- TEST
INFRASTRUCTURE ONLY.

PEM side: a numpy loop, one template at a time, restating ``Pose_Estimation_Model/run_inference_custom.py`` _get_template
:117-146 (== provider/bop_test_dataset.py :164-187) from functions pinned in oracle/pem_pre.py only (get_bbox,
cv2_resize_linear_u8, resize_rgb_choose, sample_indices, MEAN, STD).  ISM side: a CPU torch restatement of the template block of
``Instance_Segmentation_Model/run_inference_custom.py`` :129-151 / provider/bop.py :62-83 with ``CropResizePad.__call__``
(utils/bbox_utils.py:98-126) spelled out.  tests/golden/onboarding.npz (tools/gen_onboarding_golden.py) pins get_bbox,
get_resize_rgb_choose, CropResizePad and Pillow's getbbox -- the reference's own code on the case table below.

UNPINNED, as for the frame path (oracle/pem_pre.py): ``cv2.resize(INTER_LINEAR)`` is restated from the published algorithm (no cv2
on the build machine), and the sampling draws are the DEFINED sampler over injected uniform keys (``rng=`` reproduces the
reference's np.random.choice stream instead).
"""
import hashlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import pem_pre as o

H, W, S = 72, 96, 16
N_SAMPLE = 200
# (value-255 rectangle y1, y2, x1, x2): the extent decides the square side get_bbox takes (2 * (max extent // 2)); none is square,
# so that the ISM's CropResizePad (which fails on most exactly square boxes) takes them too
RECTS = [(20, 36, 40, 51),      # 0: extent 16 -> a 16-pixel crop: copy
         (10, 42, 30, 51),      # 1: extent 32 -> 32: box average
         (30, 37, 50, 55),      # 2: extent 7  -> 6: up-scaling
         (25, 48, 60, 74),      # 3: extent 23 -> 22
         (5, 38, 10, 30),       # 4: extent 33 -> 32 off the mask's centre
         (12, 60, 33, 64),      # 5: extent 48 -> 48: down-scaling by 3
         (0, 4, 40, 60),        # 6: pushed back in at the top
         (20, 50, 0, 5),        # 7: ... at the left
         (66, 72, 30, 52),      # 8: ... at the bottom
         (10, 34, 90, 96),      # 9: ... at the right
         (30, 40, 5, 95),       # 10: wider than min(H, W): the side clamps to 72
         (20, 36, 30, 43)]      # 11: a value of 128 right of the 255s (columns 43..49)
GREY_VIEW, SQUARE_VIEW, EMPTY_VIEW = 11, 12, 13
T = 14


def case_templates(seed=7):
    """The case table: T = 14 views of 72 x 96 -> dict(rgb (T,H,W,3) u8, mask (T,H,W) u8, xyz (T,H,W,3) f32 millimetres, keys
    (T,H*W) f32).  Views 0-11 as RECTS (with holes inside, border rows / columns kept), 11 with 128-valued pixels beside the 255s
    (the PEM ignores them, the ISM's box includes them), 12 an exactly square tight box, 13 all zero."""
    r = np.random.RandomState(seed)
    rgb = r.randint(0, 256, (T, H, W, 3)).astype(np.uint8)
    xyz = (r.standard_normal((T, H, W, 3)) * 80).astype(np.float32)
    keys = r.random_sample((T, H * W)).astype(np.float32)
    mask = np.zeros((T, H, W), np.uint8)
    for i, (y1, y2, x1, x2) in enumerate(RECTS):
        m = r.random_sample((y2 - y1, x2 - x1)) > 0.25
        m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = True
        mask[i, y1:y2, x1:x2] = m * 255
    mask[GREY_VIEW, 20:36, 43:50] = 128
    mask[SQUARE_VIEW, 8:24, 8:24] = 255
    return dict(rgb=rgb, mask=mask, xyz=xyz, keys=keys)


def digest(case):
    h = hashlib.sha256()
    for k in ("rgb", "mask", "xyz", "keys"):
        h.update(np.ascontiguousarray(case[k]).tobytes())
    return h.hexdigest()


def pem_template(rgb, mask_u8, xyz_mm, keys=None, rng=None, n_sample=N_SAMPLE, img_size=S, rgb_mask_flag=True):
    """_get_template for one view -> (rgb (3,S,S) f32, rgb_choose (n,) i64, xyz (n,3) f32, bbox)."""
    xyz = xyz_mm.astype(np.float32) / 1000.0
    mask = mask_u8.astype(np.uint8) == 255
    y1, y2, x1, x2 = bbox = [int(v) for v in o.get_bbox(mask)]
    mask = mask[y1:y2, x1:x2]
    c = rgb[:, :, ::-1][y1:y2, x1:x2, :]
    if rgb_mask_flag:
        c = c * (mask[:, :, None] > 0).astype(np.uint8)
    c = o.cv2_resize_linear_u8(c, img_size)
    t = ((c.astype(np.float32) / np.float32(255) - o.MEAN) / o.STD).transpose(2, 0, 1)          # ToTensor + Normalize
    choose = (mask > 0).astype(np.float32).flatten().nonzero()[0]
    if rng is not None:
        idx = rng.choice(np.arange(len(choose)), n_sample) if len(choose) <= n_sample else \
            rng.choice(np.arange(len(choose)), n_sample, replace=False)
    else:
        idx = o.sample_indices(len(choose), n_sample, keys)
    choose = choose[idx]
    pts = xyz[y1:y2, x1:x2, :].reshape((-1, 3))[choose, :]
    return t, o.resize_rgb_choose(choose, bbox, img_size), pts, bbox


def pem_templates(rgb, mask, xyz, keys=None, rng=None, n_view=None, **kw):
    """get_templates over (O,T,...) arrays -> three lists over the chosen views of (O,...) arrays, object-major draws."""
    O, T_ = mask.shape[:2]
    V = T_ if n_view is None else n_view
    views = [int(T_ / V * v) for v in range(V)]
    per = [[pem_template(rgb[ob, i], mask[ob, i], xyz[ob, i], None if keys is None else keys[ob, i], rng, **kw) for i in views]
           for ob in range(O)]
    return tuple([np.stack([per[ob][v][k] for ob in range(O)]) for v in range(V)] for k in (0, 2, 1))


def pil_bbox(mask_u8):
    """Image.getbbox of an L image: [x1,y1,x2,y2] of the pixels != 0, upper bounds exclusive (None when there is none)."""
    ys, xs = np.nonzero(mask_u8)
    return None if len(ys) == 0 else [int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1]


def crop_resize_pad(images, boxes, target):
    """CropResizePad(target).__call__ (bbox_utils.py:98-126) spelled out.  images (T,C,H,W) f32, boxes (T,4) int64 xyxy."""
    scale_factor = target / torch.max(boxes[:, 2:] - boxes[:, :2], dim=-1)[0]
    out = []
    for image, box, scale in zip(images, boxes, scale_factor):
        image = image[:, box[1]:box[3], box[0]:box[2]]
        image = F.interpolate(image.unsqueeze(0), scale_factor=scale.item())[0]
        h, w = image.shape[1:]
        if 1.0 != w / h:
            top = max((target - h) // 2, 0)
            left = max((target - w) // 2, 0)
            image = F.pad(image, (left, target - w - left, top, target - h - top))
        assert image.shape[1] == image.shape[2]
        out.append(F.interpolate(image.unsqueeze(0), scale_factor=target / image.shape[1])[0])
    return torch.stack(out)


def ism_templates(rgb, mask, target=S, normalize=False):
    """The template block for views rgb (T,H,W,3) u8 / mask (T,H,W) u8 -> (templates (T,3,S,S), masks (T,S,S)) f32 tensors."""
    boxes = torch.tensor(np.array([pil_bbox(m) for m in mask]))
    templates, masks = [], []
    for image, m in zip(rgb, mask):
        image = torch.from_numpy(image / 255).float()
        m = torch.from_numpy(m / 255).float()
        templates.append(image * m[:, :, None])
        masks.append(m.unsqueeze(-1))
    templates = crop_resize_pad(torch.stack(templates).permute(0, 3, 1, 2), boxes, target)
    masks = crop_resize_pad(torch.stack(masks).permute(0, 3, 1, 2), boxes, target)
    if normalize:                                                      # T.Normalize after the crop (provider/bop.py:81)
        mean, std = torch.tensor(o.MEAN).view(1, 3, 1, 1), torch.tensor(o.STD).view(1, 3, 1, 1)
        templates = (templates - mean) / std
    return templates, masks[:, 0, :, :]
