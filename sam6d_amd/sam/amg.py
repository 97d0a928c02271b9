"""SAM's automatic mask generator on MI355X: the per-batch body and the single-crop generator.

``process_point_batch`` is what ``SamAutomaticMaskGenerator._process_batch`` (segment_anything/
automatic_mask_generator.py:266-312) computes between "run the model on this batch of points" and "compress to RLE":
prompt encoder -> mask decoder -> upscaling to the frame -> predicted-IoU filter -> stability score + filter ->
threshold -> boxes.  The reference goes through ``SamPredictor.predict_torch(return_logits=True)`` (predictor.py:169-243),
i.e. it materialises the (64*3, H, W) fp32 logits of every batch; here the decoder's 256 x 256 logits go straight into
``s6d_sam_mask_post_f32`` and only binary masks, two counts and a box per mask exist at frame resolution.  The filters
commute (each is a per-mask predicate), so they are applied together after the one fused pass.
"""
import os
import time

import numpy as np
import torch

from .. import ops
from .. import policy


def _decode_batch(prompt_encoder, mask_decoder, image_embedding, in_points, input_size, original_size, img_size, mask_threshold,
                  stability_score_offset):
    """prompt encoder -> mask decoder -> fused post-processing for one batch of point prompts -> (low_res, iou (B,C), masks
    (B*C,H,W) bool, stability (B*C,), boxes (B*C,4))."""
    B = in_points.shape[0]
    labels = torch.ones(B, 1, dtype=torch.int, device=in_points.device)
    sparse, dense = prompt_encoder(points=(in_points[:, None, :], labels), boxes=None, masks=None)
    low_res, iou = mask_decoder(image_embeddings=image_embedding, image_pe=prompt_encoder.get_dense_pe(),
                                sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense, multimask_output=True)
    masks, stability, boxes = ops.sam_mask_post(low_res.float(), img_size, input_size, original_size, mask_threshold,
                                                stability_score_offset)
    return low_res, iou, masks, stability, boxes


_GRAPHS = {}          # (modules, shapes, dtypes, thresholds, weight fingerprint) -> (graph, static inputs, static outputs)
_GRAPH_MAX = 4        # distinct configurations kept (a segmentor serves one frame size: one entry)


def _weights_key(*modules):
    ver, ptr = 0, 0
    for m in modules:
        for t in list(m.parameters()) + list(m.buffers()):
            ver += t._version
            ptr ^= t.data_ptr()
    return ver, ptr


def _decode_batch_graphed(prompt_encoder, mask_decoder, image_embedding, in_points, input_size, original_size, img_size,
                          mask_threshold, stability_score_offset):
    """``_decode_batch`` replayed as a hipGraph (S6D_AMG_GRAPH=0 turns it off).  The batch is ~150 launches, most of them the small
    token-side operations of the two-way transformer (7 tokens per prompt): measured 19.6 ms per 1024 prompts eager against ~13 ms
    of kernel time (profiles/r04_frame_demo_kernel_stats_first.csv) -- the rest is the host issuing them.  Nothing inside depends on
    a value read back from the device; the filters behind it (torch.nonzero) stay outside the graph.  Static input buffers
    (embedding, prompts) are overwritten before each replay; the outputs are the graph's own buffers, valid until the next call
    with the same configuration (the caller gathers what it keeps right away).  The key carries everything a capture bakes in."""
    dev = image_embedding.device
    key = (id(prompt_encoder), id(mask_decoder), tuple(image_embedding.shape), image_embedding.dtype, tuple(in_points.shape),
           in_points.dtype, tuple(input_size), tuple(original_size), int(img_size), float(mask_threshold), float(stability_score_offset),
           policy.version(),
           torch.is_autocast_enabled(), torch.get_autocast_gpu_dtype(),
           _weights_key(prompt_encoder, mask_decoder), dev.index)
    g = _GRAPHS.get(key)
    if g is None:
        if len(_GRAPHS) >= _GRAPH_MAX:
            _GRAPHS.clear()
        emb_s, pts_s = image_embedding.clone(), in_points.clone()
        args = (prompt_encoder, mask_decoder, emb_s, pts_s, input_size, original_size, img_size, mask_threshold, stability_score_offset)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):                                      # warm every lazily filled cache of the decoder
                _decode_batch(*args)
        torch.cuda.current_stream(dev).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = _decode_batch(*args)
        g = (graph, emb_s, pts_s, outs)
        _GRAPHS[key] = g
    graph, emb_s, pts_s, outs = g
    emb_s.copy_(image_embedding)
    pts_s.copy_(in_points)
    graph.replay()
    return outs


def invalidate_graphs():
    """Drop every captured decoder graph (re-captured on the next call)."""
    _GRAPHS.clear()


@torch.no_grad()
def process_point_batch(prompt_encoder, mask_decoder, image_embedding, in_points, input_size, original_size, img_size=1024,
                        mask_threshold=0.0, pred_iou_thresh=0.88, stability_score_thresh=0.95,
                        stability_score_offset=1.0):
    """image_embedding (1,C,h,w) of the frame; in_points (B,2) point prompts in the resized input frame (what
    ``ResizeLongestSide.apply_coords`` returns, automatic_mask_generator.py:276-277); input_size = (h,w) of the resized
    frame inside the padded img_size square; original_size = (H,W) of the frame.
    -> dict(masks bool (K,H,W), iou_preds (K,), stability_score (K,), boxes (K,4) long XYXY, point_index (K,) long):
    the masks that pass both filters, in the reference's (prompt-major, then the 3 multimask outputs) order."""
    graphed = (torch.cuda.is_available() and image_embedding.is_cuda and policy.current().amg_graph == "1"
               and in_points.shape[0] >= 64 and not torch.cuda.is_current_stream_capturing())
    fn = _decode_batch_graphed if graphed else _decode_batch
    low_res, iou, masks, stability, boxes = fn(prompt_encoder, mask_decoder, image_embedding, in_points, input_size, original_size,
                                               img_size, mask_threshold, stability_score_offset)
    iou = iou.flatten(0, 1)
    keep = torch.ones_like(iou, dtype=torch.bool)
    if pred_iou_thresh > 0.0:
        keep &= iou > pred_iou_thresh
    if stability_score_thresh > 0.0:
        keep &= stability >= stability_score_thresh                  # NaN (empty +-offset masks) fails, as in the reference
    idx = torch.nonzero(keep).squeeze(1)
    C = low_res.shape[1]
    # low_res of the graphed path is the graph's own output buffer, overwritten by the next replay: callers that keep several
    # batches (generate_proposals) get a private copy
    return dict(masks=masks[idx], iou_preds=iou[idx], stability_score=stability[idx], boxes=boxes[idx],
                point_index=idx // C, low_res_logits=low_res.clone() if graphed else low_res)


def build_point_grid(n_per_side):
    """utils/amg.py:179-186: n x n points at the pixel-cell centres of the unit square, (x, y), row-major."""
    offset = 1 / (2 * n_per_side)
    side = np.linspace(offset, 1 - offset, n_per_side)
    return np.stack([np.tile(side[None, :], (n_per_side, 1)), np.tile(side[:, None], (1, n_per_side))], axis=-1).reshape(-1, 2)


def preprocess_shape(oldh, oldw, long_side):
    """ResizeLongestSide.get_preprocess_shape (utils/transforms.py:95-102)."""
    scale = long_side * 1.0 / max(oldh, oldw)
    return int(oldh * scale + 0.5), int(oldw * scale + 0.5)


@torch.no_grad()
def generate_proposals(prompt_encoder, mask_decoder, image_embedding, original_size, img_size=1024, points_per_side=32,
                       points_per_batch=256, mask_threshold=0.0, pred_iou_thresh=0.88, stability_score_thresh=0.95,
                       stability_score_offset=1.0, box_nms_thresh=0.7, min_mask_region_area=0, crop_nms_thresh=0.7):
    """The single-crop path of ``SamAutomaticMaskGenerator._generate_masks`` (crop_n_layers = 0, the configuration the
    ISM uses: model/sam.py:52-75) from the frame's image embedding to the de-duplicated proposals, entirely on the
    device: point grid -> batches of prompts (process_point_batch) -> box NMS on the predicted IoUs.  With one crop
    that spans the frame the crop-edge filter never fires (a box edge near the crop edge is near the image edge too,
    utils/amg.py:78-88) and uncrop_* are identities; the RLE encode / decode round trip of the reference
    (automatic_mask_generator.py:308-310, model/sam.py:146-148) is skipped -- the masks stay binary tensors.
    ``min_mask_region_area`` > 0: ``postprocess_small_regions`` after the NMS, where upstream's ``generate`` applies it
    (automatic_mask_generator.py:163-169), with the NMS threshold max(box_nms_thresh, crop_nms_thresh); ``crop_nms_thresh`` is read
    only there.  0 (the ISM configuration): nothing of it is called.
    -> dict(masks bool (K,H,W), boxes (K,4) long XYXY, iou_preds (K,), stability_score (K,), points (K,2) float64)."""
    H, W = original_size
    input_size = preprocess_shape(H, W, img_size)
    grid = build_point_grid(points_per_side) * [[W, H]]                                   # points in the frame (x, y)
    scale = [[input_size[1] / W, input_size[0] / H]]                                      # apply_coords (transforms.py:33-43)
    pts = torch.as_tensor(grid * scale, device=image_embedding.device)                    # float64, as in the reference
    prof = policy.current().amg_profile                                           # per-step milliseconds on stdout
    tq = [time.perf_counter()]

    def tick(name):
        if prof:
            torch.cuda.synchronize()
            tq.append(time.perf_counter())
            print(f"[amg] {name}: {(tq[-1] - tq[-2]) * 1e3:.1f} ms", flush=True)
    parts = []
    for a in range(0, pts.shape[0], points_per_batch):
        r = process_point_batch(prompt_encoder, mask_decoder, image_embedding, pts[a:a + points_per_batch], input_size,
                                original_size, img_size, mask_threshold, pred_iou_thresh, stability_score_thresh,
                                stability_score_offset)
        r["points"] = torch.as_tensor(grid, device=pts.device)[a:a + points_per_batch][r["point_index"]]
        parts.append(r)
    tick("prompt batches")
    cat = {k: torch.cat([p[k] for p in parts]) for k in ("masks", "boxes", "iou_preds", "stability_score", "points")}
    tick(f"concatenate {cat['masks'].shape[0]} candidates")
    keep = ops.nms(cat["boxes"].float().contiguous(), cat["iou_preds"].float(), box_nms_thresh)
    tick("nms")
    out = {k: v[keep] for k, v in cat.items()}
    tick(f"gather {keep.shape[0]} survivors")
    if min_mask_region_area > 0:
        out = postprocess_small_regions(out, min_mask_region_area, max(box_nms_thresh, crop_nms_thresh))
        tick(f"small regions: {out['masks'].shape[0]} survivors")
    return out


def _min_index_labels_library(fg):
    """fg (N,H,W) bool -> (N,H,W) int64: the minimum row-major index of each pixel's 8-connected component of fg, -1 elsewhere.
    Minimum-index propagation: the negated index plane under a 3 x 3 max_pool2d (its padding is -inf), restricted to fg, until nothing
    moves.  float64 holds every index below 2^31 exactly."""
    N, H, W = fg.shape
    sel = fg[:, None]
    idx = torch.arange(H * W, dtype=torch.float64, device=fg.device).view(1, 1, H, W)
    neg = torch.where(sel, -idx, torch.full_like(idx, -float(H * W)))
    while N:
        nxt = torch.where(sel, torch.nn.functional.max_pool2d(neg, 3, 1, 1), neg)
        if torch.equal(nxt, neg):
            break
        neg = nxt
    return torch.where(fg, (-neg[:, 0]).long(), torch.full((1,), -1, dtype=torch.int64, device=fg.device))


def _component_areas_library(lab):
    """lab (N,H,W) of ``_min_index_labels_library`` -> (cnt (N,HW): pixels of the component whose first pixel this is, 0 elsewhere;
    area (N,H,W): the area of each labelled pixel's component, 0 on the unlabelled)."""
    N, H, W = lab.shape
    flat = lab.view(N, H * W)
    on = flat >= 0
    rows = torch.arange(N, device=lab.device).view(N, 1) * (H * W)
    cnt = torch.bincount((flat + rows)[on], minlength=N * H * W).view(N, H * W)
    area = torch.where(on, cnt.gather(1, flat.clamp(min=0)), torch.zeros_like(flat))
    return cnt, area.view(N, H, W)


def mask_boxes(masks):
    """batched_mask_to_box (utils/amg.py:303-346) of (N,H,W) masks -> (N,4) int32 XYXY, inclusive maximum corner, zeros when empty."""
    m = masks != 0
    N, H, W = m.shape
    cols, rows = m.any(1), m.any(2)
    xs, ys = torch.arange(W, device=m.device), torch.arange(H, device=m.device)
    x1, y1 = torch.where(cols, xs, -1).amax(1), torch.where(rows, ys, -1).amax(1)
    x0, y0 = torch.where(cols, xs, W).amin(1), torch.where(rows, ys, H).amin(1)
    box = torch.stack([x0, y0, x1, y1], 1)
    return (box * (x1 >= 0).view(N, 1)).int()


def _remove_small_regions_library(masks, min_area):
    """The definition of ``remove_small_regions`` in torch statements, step by step (any device)."""
    m = masks != 0
    N, H, W = m.shape
    if N == 0 or H * W == 0:
        return m.to(torch.uint8), torch.zeros(N, dtype=torch.bool, device=m.device), torch.zeros(N, 4, dtype=torch.int32, device=m.device)
    # 1. holes: components of the unset pixels with area < min_area are set
    _, area = _component_areas_library(_min_index_labels_library(~m))
    fill = ~m & (area < min_area)
    changed_h = fill.flatten(1).any(1)
    m = m | fill
    # 2. islands, on that result
    lab = _min_index_labels_library(m)
    cnt, area = _component_areas_library(lab)
    small = m & (area < min_area)
    changed_i = small.flatten(1).any(1)
    any_big = (cnt >= min_area).any(1)
    # every component small: the largest area, and of equal areas the smallest first pixel (cnt (H W) + (H W - 1 - root) is unique)
    root = torch.arange(H * W, device=m.device).view(1, H * W)
    best = (cnt * (H * W) + (H * W - 1 - root)).argmax(1)
    keep = m & torch.where(any_big.view(N, 1, 1), ~small, lab == best.view(N, 1, 1))
    return keep.to(torch.uint8), changed_h | changed_i, mask_boxes(keep)


@torch.no_grad()
def remove_small_regions(masks, min_area):
    """remove_small_regions (utils/amg.py:267-291) of a batch of masks, both modes in the order upstream's ``postprocess_small_regions``
    applies them.  masks (N,H,W) bool or uint8, a pixel is set when it is not 0; min_area an integer >= 1; connectivity 8.
      1. holes: every 8-connected component of the UNSET pixels with area < min_area is set (one that touches the border too);
      2. islands, on that result: the components of the SET pixels with area < min_area are cleared -- unless every component is
         small: then the one of largest area stays, of equal areas the one whose first pixel in row-major order comes first;
      3. changed = a component below min_area existed in 1 or in 2 (also when the pixels end up equal: one small component).
    -> (masks (N,H,W) uint8 0 / 1, changed (N,) bool, boxes (N,4) int32 XYXY, inclusive maximum, zeros for an empty mask).
    ``ops.remove_small_regions`` (csrc/s6d_ccl.hip) on device tensors; the torch statement ``_remove_small_regions_library`` on CPU
    tensors or when ``policy.disable_fused`` names ``small_regions`` (an error under the strict policy, like every library branch)."""
    if int(min_area) != min_area or min_area < 1:
        raise ValueError(f"remove_small_regions: min_area must be an integer >= 1, got {min_area!r}")
    if masks.dim() != 3 or masks.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"remove_small_regions: masks (N,H,W) bool or uint8 expected, got {tuple(masks.shape)} {masks.dtype}")
    if policy.guard("amg.remove_small_regions", cuda=masks.is_cuda, have=ops.have("small_regions")):
        return ops.remove_small_regions(masks.contiguous(), int(min_area))
    return _remove_small_regions_library(masks, int(min_area))


def _nms_library(boxes, scores, iou_threshold):
    """``ops.nms`` in torch statements: boxes (N,4) f32 XYXY visited by decreasing score, EQUAL SCORES IN INPUT ORDER (a stable sort);
    a box is dropped when its IoU with a kept one exceeds the threshold -> kept indices in visiting order."""
    order = torch.sort(scores.float(), descending=True, stable=True)[1]
    b = boxes.float()[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.minimum(b[:, None, 2:], b[None, :, 2:]) - torch.maximum(b[:, None, :2], b[None, :, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    over = (inter / (area[:, None] + area[None, :] - inter) > iou_threshold).cpu()
    dead = torch.zeros(b.shape[0], dtype=torch.bool)
    for i in range(b.shape[0]):
        if not dead[i]:
            dead[i + 1:] |= over[i, i + 1:]
    return order[(~dead).to(order.device)]


@torch.no_grad()
def postprocess_small_regions(proposals, min_area, nms_thresh):
    """SamAutomaticMaskGenerator.postprocess_small_regions (automatic_mask_generator.py:323-372) on the dict ``generate_proposals``
    returns: ``remove_small_regions`` on every mask, then a box NMS on the NEW boxes with score 1 for the unchanged masks and 0 for
    the changed ones, so that an unchanged mask wins over a changed duplicate.  Equal scores are visited in input order (``ops.nms``
    sorts stably; torchvision, which is not part of this project, promises no order).  Every field is filtered by the NMS result in
    its order -- unchanged survivors first --; masks and boxes of the changed survivors are the new ones.  An empty input is returned
    as it is."""
    masks = proposals["masks"]
    if masks.shape[0] == 0:
        return proposals
    new_masks, changed, new_boxes = remove_small_regions(masks, min_area)
    scores = (~changed).float()
    fboxes = new_boxes.float().contiguous()
    if policy.guard("amg.postprocess_small_regions", cuda=fboxes.is_cuda, have=ops.have("nms")):
        keep = ops.nms(fboxes, scores, nms_thresh)
    else:
        keep = _nms_library(fboxes, scores, nms_thresh)
    out = {k: v[keep] for k, v in proposals.items()}
    ch = changed[keep]
    out["masks"] = torch.where(ch.view(-1, 1, 1), new_masks[keep].to(masks.dtype), out["masks"])
    out["boxes"] = torch.where(ch.view(-1, 1), new_boxes[keep].to(proposals["boxes"].dtype), out["boxes"])
    return out


def segmentor_input_size(orig_size, segmentor_width_size):
    """(height, width) the frame is resized to before SAM sees it: CustomSamAutomaticMaskGenerator.preprocess_resize
    (Instance_Segmentation_Model/model/sam.py:75-81; ``segmentor_width_size`` is 640 in configs/model/ISM_sam.yaml).  The
    resize itself is cv2.resize on the host in the reference (bilinear, fixed-point; cv2 is an un-vendored dependency --
    not restated here); for frames that already are that wide -- every 640 x 480 BOP set and the custom demo -- it is the
    identity."""
    return int(segmentor_width_size * orig_size[0] / orig_size[1]), int(segmentor_width_size)


def postprocess_resize(masks, boxes, orig_size, segmentor_width_size):
    """CustomSamAutomaticMaskGenerator.postprocess_resize (model/sam.py:83-100): masks (N,h,w) bool/float found on the
    resized frame -> FLOAT masks (N,H,W) by bilinear interpolation (align_corners=False; the reference keeps the
    fractional edge values, it does not re-threshold), boxes (N,4) -> float, scaled by W / segmentor_width_size and
    clamped to the frame.  Same torch ops as the reference, on whatever device the tensors live."""
    H, W = int(orig_size[0]), int(orig_size[1])
    m = torch.nn.functional.interpolate(masks.unsqueeze(1).float(), size=(H, W), mode="bilinear", align_corners=False)[:, 0]
    b = boxes.float() * (W / segmentor_width_size)
    b[:, [0, 2]] = torch.clamp(b[:, [0, 2]], 0, W - 1)
    b[:, [1, 3]] = torch.clamp(b[:, [1, 3]], 0, H - 1)
    return m, b
