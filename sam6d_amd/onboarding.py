"""Onboarding of a new object from its rendered template views, on the device.

The reference renders T views of a CAD model (BlenderProc: ``rgb_i.png``, ``mask_i.png``, ``xyz_i.npy``) and turns them into what
its two models keep per object, in CPU loops of one view at a time:

  * Pose Estimation Model -- ``Pose_Estimation_Model/run_inference_custom.py`` _get_template / get_templates :117-162 (==
    ``provider/bop_test_dataset.py`` :164-208): per view the square ``get_bbox`` crop of the pixels == 255, the channel-flipped,
    masked colour crop through ``cv2.resize(INTER_LINEAR)`` + ToTensor + Normalize, 5000 sampled mask pixels with their model
    points ``xyz / 1000`` and their index in the resized crop (``get_resize_rgb_choose``); then ``get_obj_feats``;
  * Instance Segmentation Model -- ``Instance_Segmentation_Model/run_inference_custom.py`` :125-159 (custom flow) and
    ``provider/bop.py`` :60-83 (BOP flow): per view PIL's ``getbbox`` of the mask, ``rgb / 255 * (mask / 255)``, ``CropResizePad``;
    then the cls and masked-patch descriptors of DINOv2.

Here every view of every object goes through one set of launches (csrc/s6d_onboard.hip + the sampler of csrc/s6d_pempre.hip):
boxes, in-order compaction, sampling, both kinds of crops; ``onboard`` runs the two models on the results and returns exactly the
arguments ``sam6d_amd.pipeline.FramePipeline`` wants.  The same steps are stated with torch ops for host tensors and for
``S6D_ONBOARD=library`` runs, behind ``policy.guard``.

Rendering the views from a mesh and the mesh surface samples (``trimesh.sample``) are ``sam6d_amd.render`` (``onboard_from_mesh``
is mesh -> views -> ``onboard``); here the caller passes views, model points and poses in.  Outside the library, as the reference's
data: the template pose tables.

Defined differently from the reference, on purpose (as for the frame path, sam6d_amd/pem/preprocess.py):
  * sampling uses INJECTED uniforms (``keys``, one per pixel of a view) in the defined form of ``oracle/pem_pre.py``
    sample_indices; ``rng=`` switches to the reference's own ``np.random.choice`` draws, one per template, object-major;
  * ``cv2.resize`` is its published fixed-point algorithm restated (no cv2 here): parity unpinned until vectors exist.
"""
import dataclasses
import os

import numpy as np
import torch

from . import ops, policy
from .ism.dinov2 import RGB_MEAN, RGB_STD, crop_params, crop_valid
from .pem import preprocess as pre


def _use_kernels(site, t):
    return policy.guard(site, cuda=t.is_cuda, policy=policy.current().onboard != "library",
                        have=all(ops.have(k) for k in ("template_boxes", "template_points", "template_pem_crops", "template_ism_crops")))


def _tensor(a, dtype, name):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a))
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype} (got {t.dtype})")
    return t


def _tight_boxes(mask):
    """PIL's Image.getbbox of every mask (T,H,W): [x1,y1,x2,y2] of the pixels != 0, upper bounds exclusive; zeros when there is none."""
    T, H, W = mask.shape
    dev = mask.device
    nz = mask != 0
    rows, cols = nz.any(2), nz.any(1)
    ar_h, ar_w = torch.arange(H, device=dev), torch.arange(W, device=dev)
    y1 = torch.where(rows, ar_h, H).min(1).values
    y2 = torch.where(rows, ar_h, -1).max(1).values + 1
    x1 = torch.where(cols, ar_w, W).min(1).values
    x2 = torch.where(cols, ar_w, -1).max(1).values + 1
    return torch.stack([x1, y1, x2, y2], 1) * rows.any(1)[:, None]


@torch.no_grad()
def pem_template_inputs(rgb_u8, mask_u8, xyz_mm, keys=None, rng=None, n_sample=5000, img_size=224, rgb_mask_flag=True, n_view=None):
    """The PEM's template inputs (get_templates, run_inference_custom.py:149-162) for every chosen view of every object.

    rgb_u8 (T,H,W,3) uint8 RGB, mask_u8 (T,H,W) uint8 (255 = object), xyz_mm (T,H,W,3) f32 model coordinates in millimetres --
    or all three with a leading object dimension (O,T,...); tensors on one device (numpy arrays are taken as host tensors).
    n_view views are used out of the T given (default: all), view v being ``int(T / n_view * v)``.  Exactly one of ``keys``
    ((..., T, H*W) f32 uniforms in [0, 1), one per pixel) / ``rng`` (``numpy.random`` itself or a RandomState: one ``choice`` per
    template, object-major, then view order) selects the sampler.
    -> (tem_rgb, tem_pts, tem_choose): three lists with one entry per chosen view, (O,3,S,S) f32, (O,n_sample,3) f32 metres and
    (O,n_sample) i64, O = 1 without the object dimension -- what ``get_obj_feats`` takes.
    A view without a pixel == 255 raises ValueError (the reference dies with an IndexError in get_bbox there)."""
    if (keys is None) == (rng is None):
        raise ValueError("pass either keys (injected uniforms) or rng (numpy-compatible draws)")
    rgb, mask, xyz = _tensor(rgb_u8, torch.uint8, "rgb_u8"), _tensor(mask_u8, torch.uint8, "mask_u8"), _tensor(xyz_mm, torch.float32, "xyz_mm")
    if mask.dim() == 3:
        rgb, mask, xyz = rgb[None], mask[None], xyz[None]
        keys = None if keys is None else keys[None]
    O, T, H, W = mask.shape
    if tuple(rgb.shape) != (O, T, H, W, 3) or tuple(xyz.shape) != (O, T, H, W, 3):
        raise ValueError(f"rgb_u8 / xyz_mm must be (..., {T}, {H}, {W}, 3) like mask_u8, got {tuple(rgb.shape)} / {tuple(xyz.shape)}")
    V = T if n_view is None else int(n_view)
    views = [int(T / V * v) for v in range(V)]
    dev = mask.device
    vi = torch.tensor(views, device=dev)
    N, S = O * V, int(img_size)
    rgb, mask, xyz = (t[:, vi].reshape((N,) + t.shape[2:]).contiguous() for t in (rgb, mask, xyz))
    if keys is not None:
        keys = _tensor(keys, torch.float32, "keys")
        if tuple(keys.shape) != (O, T, H * W) or H * W < n_sample:
            raise ValueError(f"keys must be (..., {T}, {H * W}) with at least n_sample = {n_sample} uniforms per view, got {tuple(keys.shape)}")
        keys = keys[:, vi].reshape(N, H * W).contiguous()

    def check(cnt):
        empty = torch.nonzero(cnt == 0).squeeze(1).tolist()
        if empty:
            raise ValueError("pem_template_inputs: no mask pixel == 255 in template view(s) " +
                             ", ".join(f"{views[i % V]} of object {i // V}" for i in empty))
    if _use_kernels("onboarding.pem_template_inputs", mask):
        cnt, box, _ = ops.template_boxes(mask)
        check(cnt)
        choose_l, pts_l, n = ops.template_points(mask, xyz, box, min(H, W) ** 2)
        if rng is not None:
            idx = pre._numpy_choice_indices(n, cnt > 0, n_sample, rng).to(dev)
        else:
            idx, overflow = ops.pem_sample_indices(keys, n, n_sample) if n_sample <= ops.PEM_SAMPLE_MAX else (None, None)
            if idx is None or bool(overflow.any()):                  # heavily duplicated keys: the top-k formulation
                idx = pre._keyed_indices_library(n, keys, n_sample)
        pts = torch.gather(pts_l, 1, idx[:, :, None].expand(-1, -1, 3))
        ch = torch.gather(choose_l, 1, idx).long()
        crops = ops.template_pem_crops(rgb, mask, box, S, rgb_mask_flag, pre.MEAN, pre.STD)
    else:
        m = mask == 255
        cnt = m.flatten(1).sum(1)
        check(cnt)
        box = pre.square_boxes(m)
        y1, y2, x1, x2 = box.unbind(1)
        t_, y_, x_ = torch.nonzero(m).unbind(1)                       # (view, y, x) order = row-major inside each crop
        inside = (y_ >= y1[t_]) & (y_ < y2[t_]) & (x_ >= x1[t_]) & (x_ < x2[t_])
        t_, y_, x_ = t_[inside], y_[inside], x_[inside]
        choose = (y_ - y1[t_]) * (x2 - x1)[t_] + (x_ - x1[t_])
        all_pts = xyz[t_, y_, x_] / torch.full((1,), 1000.0, device=dev)            # a tensor divisor: the IEEE quotient
        n = torch.bincount(t_, minlength=N)
        idx = pre._numpy_choice_indices(n, cnt > 0, n_sample, rng).to(dev) if rng is not None else \
            pre._keyed_indices_library(n, keys, n_sample)
        g = (torch.cumsum(n, 0) - n)[:, None] + idx
        pts, ch = all_pts[g], choose[g]
        crops = pre._crops(rgb, m.float(), box, S, rgb_mask_flag)
    rgb_choose = pre.resize_rgb_choose(ch, box, S)
    crops, pts, rgb_choose = crops.view(O, V, 3, S, S), pts.view(O, V, n_sample, 3), rgb_choose.view(O, V, n_sample)
    return ([crops[:, v].contiguous() for v in range(V)], [pts[:, v].contiguous() for v in range(V)],
            [rgb_choose[:, v].contiguous() for v in range(V)])


def _ism_crops_library(rgb, mask, params, S, normalize):
    """The library-op statement of s6d_template_ism_crops_f32 (value for value the same float32 operations)."""
    T, H, W = mask.shape
    dev = mask.device
    x1, y1, h, w, h1, w1, top, left, S2 = params[:, :9].long().unbind(1)
    inv1, inv2 = params[:, 9:11].contiguous().view(torch.float32).unbind(1)

    def near(dst, size, inv):                                          # ATen's nearest source index with the user's scale
        return torch.minimum((dst.float() * inv[:, None]).floor().long(), size[:, None] - 1)
    p2 = near(torch.arange(S, device=dev)[None, :], S2, inv2)         # (T,S): second resize, the same on both axes
    iy, ix = p2 - top[:, None], p2 - left[:, None]
    ok = ((iy >= 0) & (iy < h1[:, None]))[:, :, None] & ((ix >= 0) & (ix < w1[:, None]))[:, None, :]
    sy = (y1[:, None] + near(iy.clamp(min=0), h, inv1)).clamp(0, H - 1)[:, :, None]
    sx = (x1[:, None] + near(ix.clamp(min=0), w, inv1)).clamp(0, W - 1)[:, None, :]
    tt = torch.arange(T, device=dev)[:, None, None]
    c255 = torch.full((1,), 255.0, device=dev)
    zero = torch.zeros((), device=dev)
    mk = torch.where(ok, mask[tt, sy, sx].float() / c255, zero)
    out = torch.where(ok[..., None], (rgb[tt, sy, sx].float() / c255) * mk[..., None], zero).permute(0, 3, 1, 2)
    if normalize:
        out = (out - torch.tensor(RGB_MEAN, device=dev)[None, :, None, None]) / torch.tensor(RGB_STD, device=dev)[None, :, None, None]
    return out.contiguous(), mk


@torch.no_grad()
def ism_template_inputs(rgb_u8, mask_u8, image_size=224, normalize=False):
    """The ISM's template crops for the views of one object: rgb_u8 (T,H,W,3) uint8, mask_u8 (T,H,W) uint8 ->
    (templates (T,3,S,S) f32, masks (T,S,S) f32) = ``CropResizePad`` of ``rgb / 255 * (mask / 255)`` and of ``mask / 255`` on PIL's
    ``getbbox`` of the mask (every pixel != 0; a value below 255 scales its pixel).
    normalize=True is the BOP flow (provider/bop.py:78-83): ``(v - mean) / std`` AFTER the crop, on the zero padding too.
    normalize=False is the custom flow (run_inference_custom.py:134-159), which feeds UN-NORMALISED templates to DINOv2 although
    the query crops are normalised -- the reference's behaviour, kept as it is.
    A view whose crop the reference cannot produce (an empty mask; ``sam6d_amd.ism.dinov2.crop_valid``: CropResizePad raises on
    most exactly square boxes and on slivers) raises ValueError naming it."""
    rgb, mask = _tensor(rgb_u8, torch.uint8, "rgb_u8").contiguous(), _tensor(mask_u8, torch.uint8, "mask_u8").contiguous()
    T, H, W = mask.shape
    if tuple(rgb.shape) != (T, H, W, 3):
        raise ValueError(f"rgb_u8 must be ({T}, {H}, {W}, 3) like mask_u8, got {tuple(rgb.shape)}")
    S = int(image_size)
    kernels = _use_kernels("onboarding.ism_template_inputs", mask)
    tight = ops.template_boxes(mask)[2] if kernels else _tight_boxes(mask)
    boxes = tight.cpu().numpy()
    bad = np.nonzero(~crop_valid(boxes, S))[0].tolist()
    if bad:
        raise ValueError(f"ism_template_inputs: the reference's CropResizePad cannot produce the crop of template view(s) {bad} "
                         f"(boxes xyxy {boxes[bad].tolist()})")
    params = torch.from_numpy(crop_params(boxes, S)).to(mask.device)
    if kernels:
        return ops.template_ism_crops(rgb, mask, params, S, normalize, RGB_MEAN, RGB_STD)
    return _ism_crops_library(rgb, mask, params, S, normalize)


@dataclasses.dataclass
class Onboarded:
    """What ``FramePipeline`` keeps per object set: ``FramePipeline(..., scorer=o.scorer, pem_templates=o.pem_templates,
    object_radius=o.object_radius)``."""
    scorer: object            # sam6d_amd.ism.scoring.FrameScorer over the (O,T,C) cls / (O,T,N,C) masked-patch descriptors
    pem_templates: dict       # model (O,m,3), dense_po (O,n,3), dense_fo (O,n,C)
    object_radius: torch.Tensor          # (O,) max |model_points|

    def save(self, path):
        """The tensors in one file (the reference caches descriptors.pth for the same reason)."""
        mc = self.scorer.matching_config
        torch.save(dict(ref_data={k: v.detach().cpu() for k, v in self.scorer.ref_data.items()},
                        pem_templates={k: v.detach().cpu() for k, v in self.pem_templates.items()},
                        object_radius=self.object_radius.detach().cpu(), confidence_thresh=float(mc.confidence_thresh),
                        aggregation_function=mc.aggregation_function, visible_thred=float(self.scorer.visible_thred)), path)

    @classmethod
    def load(cls, path, device="cpu"):
        from .ism.scoring import FrameScorer
        d = torch.load(path, map_location="cpu", weights_only=True)
        r = {k: v.to(device) for k, v in d["ref_data"].items()}
        scorer = FrameScorer(r["descriptors"], r["appe_descriptors"], r["poses"], r["pointcloud"], confidence_thresh=d["confidence_thresh"],
                             aggregation_function=d["aggregation_function"], visible_thred=d["visible_thred"])
        return cls(scorer, {k: v.to(device) for k, v in d["pem_templates"].items()}, d["object_radius"].to(device))


@torch.no_grad()
def onboard(descriptor_model, pem_net, objects, *, keys=None, rng=None, normalize=False, n_view=42, confidence_thresh=0.2,
            n_sample=5000, img_size=224, rgb_mask_flag=True):
    """Everything the frame pipeline keeps of a set of objects, from their rendered views.

    descriptor_model: sam6d_amd.ism.dinov2.CustomDINOv2; pem_net: sam6d_amd.pem.pose_estimation_model.Net; objects: a list of
    dicts (the same T, H, W for every object) with ``rgb`` (T,H,W,3) uint8, ``mask`` (T,H,W) uint8, ``xyz_mm`` (T,H,W,3) f32,
    ``model_points`` (m,3) f32 metres (the PEM's model cloud), ``ism_points`` (k,3) f32 metres (the cloud the ISM projects) and
    ``poses`` (T,4,4) template poses (the same table for every object, as the reference's ref_data holds it).  keys (O,T,H*W) / rng, n_view, n_sample, img_size, rgb_mask_flag: pem_template_inputs;
    normalize: ism_template_inputs (False = the custom flow, True = the BOP flow).
    The ISM uses all T views (run_inference_custom.py:127-129), the PEM n_view of them (get_templates).  -> Onboarded."""
    from .ism.scoring import FrameScorer
    dev = next(pem_net.parameters()).device
    npoint = getattr(pem_net.feature_extraction, "npoint", 0)
    if n_view * n_sample < npoint:
        raise ValueError(f"onboard: get_obj_feats keeps {npoint} template points per object, n_view * n_sample = {n_view} * {n_sample} "
                         "are fewer than that")
    stack = lambda k, dt: torch.stack([_tensor(o[k], dt, k) for o in objects]).to(dev)          # noqa: E731
    rgb, mask, xyz = stack("rgb", torch.uint8), stack("mask", torch.uint8), stack("xyz_mm", torch.float32)
    tem_rgb, tem_pts, tem_choose = pem_template_inputs(rgb, mask, xyz, keys=None if keys is None else keys.to(dev), rng=rng,
                                                       n_sample=n_sample, img_size=img_size, rgb_mask_flag=rgb_mask_flag, n_view=n_view)
    dense_po, dense_fo = pem_net.feature_extraction.get_obj_feats(tem_rgb, tem_pts, tem_choose)
    model = torch.stack([torch.as_tensor(o["model_points"]).float() for o in objects]).to(dev)
    cls, patch = [], []
    for o in range(len(objects)):
        templates, masks = ism_template_inputs(rgb[o], mask[o], descriptor_model.proposal_size, normalize)
        cls.append(descriptor_model.compute_features(templates, token_name="x_norm_clstoken"))
        patch.append(descriptor_model.compute_masked_patch_feature(templates, masks))
    poses = [torch.as_tensor(o["poses"]).float() for o in objects]
    if any(not torch.equal(p, poses[0]) for p in poses[1:]):          # one table for all objects (the icosphere poses: detector.py ref_data)
        raise ValueError("onboard: the objects' template poses differ; the scorer keeps one (T,4,4) table for all of them")
    scorer = FrameScorer(torch.stack(cls), torch.stack(patch), poses[0].to(dev),
                         torch.stack([torch.as_tensor(o["ism_points"]).float() for o in objects]).to(dev),
                         confidence_thresh=confidence_thresh)
    return Onboarded(scorer, dict(model=model, dense_po=dense_po, dense_fo=dense_fo), model.norm(dim=2).max(dim=1).values)


def load_template_dir(path):
    """The rendered views of one object as the reference's loaders read them (host side): ``rgb_i.png`` through
    ``.convert("RGB")``, ``mask_i.png`` through ``.convert("L")``, ``xyz_i.npy``, for i = 0 .. T-1 (T = the number of xyz files).
    -> (rgb (T,H,W,3) uint8, mask (T,H,W) uint8, xyz_mm (T,H,W,3) float32) numpy arrays."""
    import glob

    from PIL import Image
    T = len(glob.glob(os.path.join(path, "xyz_*.npy")))
    if T == 0:
        raise FileNotFoundError(f"no xyz_*.npy under {path}")
    rgb = np.stack([np.array(Image.open(os.path.join(path, f"rgb_{i}.png")).convert("RGB")) for i in range(T)])
    mask = np.stack([np.array(Image.open(os.path.join(path, f"mask_{i}.png")).convert("L")) for i in range(T)])
    xyz = np.stack([np.load(os.path.join(path, f"xyz_{i}.npy")).astype(np.float32) for i in range(T)])
    return rgb, mask, xyz
