"""Scoring methods of ``Instance_Segmentation_Model`` (model/detector.py) on MI355X.

``ScoringMixin`` carries the six methods that both run_inference_custom.py:168-197 and
detector.py::test_step :362-381 call by name on the model object
(compute_semantic_score :260-296, best_template_pose :198-207, compute_appearance_score :298-308,
compute_geometric_score :310-322, project_template_to_image :209-232,
Calculate_the_query_translation :234-246) with the reference's signatures and attribute
contract (``self.ref_data[...]``, ``self.matching_config``, ``self.visible_thred``).
INTEGRATION.md shows the two-line change that mixes it into the reference class.
"""
import torch

from .. import ops
from .. import policy
from .loss import MaskedPatch_MatrixSimilarity


def compute_iou(bb_a, bb_b):
    """utils/bbox_utils.py:197-221 incl. quirk Q3: one empty intersection -> scalar 0.0 for all."""
    tl = torch.max(bb_a[:, 0:2], bb_b[:, 0:2])
    br = torch.min(bb_a[:, 2:4], bb_b[:, 2:4])
    wh_a, wh_b, wh_i = bb_a[:, 2:4] - bb_a[:, 0:2], bb_b[:, 2:4] - bb_b[:, 0:2], br - tl
    if (wh_i > 0).all():
        ai = wh_i[:, 0] * wh_i[:, 1]
        return ai / (wh_a[:, 0] * wh_a[:, 1] + wh_b[:, 0] * wh_b[:, 1] - ai)
    return 0.0


def masked_depth_translation(masks, depth, K, depth_scale):
    """Mean back-projected point of each mask (utils/trimesh_utils.py:77-105 applied to
    mask*depth, detector.py:234-246) without the (S,H,W) ``repeat``: three masked sums."""
    S, H, W = masks.shape
    # the kernel reads the maps as float4 and follows ATen's 16-row cascade, which holds for 8 <= H*W < 2^24 (csrc/s6d_ism.hip)
    if policy.guard("ism.masked_depth_mean", cuda=masks.is_cuda, have=ops.have("masked_depth_mean"), W4=W % 4 == 0,
                    pixels_8_to_2p24=8 <= H * W < 2 ** 24):
        return ops.masked_depth_mean(masks.to(torch.float32).contiguous(), depth.to(torch.float32).contiguous(), K,
                                     float(depth_scale))
    # dtype trail of the reference: Z float32; X, Y float64 (the camera matrix is a float64 tensor
    # whose 0-dim elements promote `u - K[0,2]`), sums in that dtype, final cast to float32.
    z = masks.to(torch.float32) * depth.to(torch.float32)[None] * depth_scale / 1000
    K = K.to(device=z.device, dtype=torch.float64)
    u = torch.arange(W, device=z.device, dtype=torch.float64)[None, None, :]
    v = torch.arange(H, device=z.device, dtype=torch.float64)[None, :, None]
    valid = z > 0
    n = (valid.sum(dim=(1, 2)) + 1e-8).to(torch.float32)
    x = ((u - K[0, 2]) * z / K[0, 0] * valid).sum(dim=(1, 2)) / n
    y = ((v - K[1, 2]) * z / K[1, 1] * valid).sum(dim=(1, 2)) / n
    zz = (z * valid).sum(dim=(1, 2)) / n
    return torch.stack((x, y, zz.to(torch.float64)), dim=1).to(torch.float32)


class RefPatchHandle:
    """What compute_appearance_score returns as `ref_aux_descriptor` on the fused path: the (object, template)
    selection into the resident descriptor store instead of a gathered (S,256,C) copy (1 MB per proposal).
    compute_geometric_score accepts it; ``materialize()`` gives the reference's tensor if a caller wants it."""

    def __init__(self, store, obj, tmpl, visible_ratio, thred):
        self.store, self.obj, self.tmpl, self.visible_ratio, self.thred = store, obj, tmpl, visible_ratio, thred

    def materialize(self):
        return self.store[self.obj.long(), self.tmpl.long(), ...]


class ScoringMixin:
    def best_template_pose(self, scores, pred_idx_objects):
        best = scores.argmax(dim=-1)                                   # (S,O)
        return torch.gather(best, 1, pred_idx_objects[:, None])[:, 0]

    def compute_semantic_score(self, proposal_decriptors):
        cfg = self.matching_config
        scores = cfg.metric(proposal_decriptors, self.ref_data["descriptors"])     # (P,O,T)
        agg = cfg.aggregation_function
        topk = {"mean": scores.shape[-1], "max": 1, "avg_5": 5}.get(agg)
        if topk is not None and policy.guard("ism.compute_semantic_score", cuda=scores.is_cuda, have=ops.have("semantic_select"),
                                             f32=scores.dtype == torch.float32, T_le_256=scores.shape[-1] <= 256):
            # one kernel: per-object top-k mean, arg-max object, best template of that object
            score_per_proposal, assigned, best_t = ops.semantic_select(scores.contiguous(), topk)
            idx_selected = torch.nonzero(score_per_proposal > cfg.confidence_thresh).squeeze(1)
            return (idx_selected, assigned[idx_selected].long(), score_per_proposal[idx_selected],
                    best_t[idx_selected].long())
        if agg == "mean":
            per_obj = scores.sum(dim=-1) / scores.shape[-1]
        elif agg == "median":
            per_obj = torch.median(scores, dim=-1)[0]
        elif agg == "max":
            per_obj = scores.max(dim=-1)[0]
        elif agg == "avg_5":
            per_obj = torch.topk(scores, k=5, dim=-1)[0].mean(dim=-1)
        else:
            raise NotImplementedError
        score_per_proposal, assigned = per_obj.max(dim=-1)
        idx_selected = torch.arange(len(score_per_proposal), device=score_per_proposal.device)[
            score_per_proposal > cfg.confidence_thresh]
        pred_idx_objects = assigned[idx_selected]
        best_template = self.best_template_pose(scores[idx_selected, ...], pred_idx_objects)
        return idx_selected, pred_idx_objects, score_per_proposal[idx_selected], best_template

    def compute_appearance_score(self, best_pose, pred_objects_idx, qurey_appe_descriptors, sel=None):
        """sel (device path only): ``qurey_appe_descriptors`` holds EVERY proposal and the kernel reads the rows ``sel`` names -- the
        `[idx_selected]` copy of model/detector.py:341-349 (1 MB per selected proposal) is never made."""
        store = self.ref_data["appe_descriptors"]
        thred = getattr(self, "visible_thred", 0.5)
        halfs = (torch.float16, torch.bfloat16)
        if policy.guard("ism.compute_appearance_score", cuda=qurey_appe_descriptors.is_cuda, have=ops.have("patch_scores"),
                        contiguous_store=store.is_contiguous(), patches_le_256=store.shape[2] <= 256, C32=store.shape[-1] % 32 == 0,
                        dtypes=store.dtype in (torch.float32,) + halfs and qurey_appe_descriptors.dtype in (torch.float32,) + halfs):
            # half descriptors (BOP flow under precision=16): the resident store is converted ONCE per store tensor and kept (it
            # is read-only template data); the query of the frame is converted per call.  fp32 arithmetic inside the kernel.
            if store.dtype != torch.float32:
                c = getattr(self, "_store_f32", None)
                if c is None or c[0] is not store:
                    c = (store, store.float())
                    self._store_f32 = c
                store = c[1]
            qdt = qurey_appe_descriptors.dtype
            obj32, tmpl32 = pred_objects_idx.int().contiguous(), best_pose.int().contiguous()
            appe, ratio = ops.patch_scores(qurey_appe_descriptors.float().contiguous(), store, obj32, tmpl32, float(thred),
                                           sel=sel)
            return appe.to(qdt), RefPatchHandle(store, obj32, tmpl32, ratio.to(qdt), thred)
        if sel is not None:
            qurey_appe_descriptors = qurey_appe_descriptors[sel.long()]
        ref = store[pred_objects_idx, best_pose, ...]
        metric = MaskedPatch_MatrixSimilarity(metric="cosine", chunk_size=64)
        appe, ratio = metric.both(qurey_appe_descriptors, ref, thred)
        self._cached_visible = (qurey_appe_descriptors.data_ptr(), ref.data_ptr(), thred, ratio)
        return appe, ref

    def compute_geometric_score(self, image_uv, proposals, appe_descriptors, ref_aux_descriptor, visible_thred=0.5):
        if isinstance(ref_aux_descriptor, RefPatchHandle):
            if ref_aux_descriptor.thred == visible_thred:
                visible_ratio = ref_aux_descriptor.visible_ratio    # produced by the same similarity pass
            else:
                visible_ratio = ops.patch_scores(appe_descriptors.float().contiguous(), ref_aux_descriptor.store,
                                                 ref_aux_descriptor.obj, ref_aux_descriptor.tmpl,
                                                 float(visible_thred))[1].to(appe_descriptors.dtype)
        else:
            c = getattr(self, "_cached_visible", None)
            if c is not None and c[0] == appe_descriptors.data_ptr() and c[1] == ref_aux_descriptor.data_ptr() \
                    and c[2] == visible_thred:
                visible_ratio = c[3]                   # same GEMM as the appearance score: reuse it
            else:
                visible_ratio = MaskedPatch_MatrixSimilarity().compute_visible_ratio(
                    appe_descriptors, ref_aux_descriptor, visible_thred)
        bb = getattr(self, "_cached_bbox", None)
        if bb is not None and bb[0] == image_uv.data_ptr():
            xyxy = bb[1]                               # reduced by the projection kernel
        else:
            xyxy = torch.cat((image_uv.min(dim=1).values, image_uv.max(dim=1).values), dim=-1)
        return compute_iou(xyxy, proposals.boxes), visible_ratio

    def Calculate_the_query_translation(self, proposal, depth, cam_intrinsic, depth_scale):
        proposal = proposal.squeeze_()               # quirk Q7: in-place squeeze of detections.masks
        if proposal.dim() == 2:
            proposal = proposal[None]
        return masked_depth_translation(proposal, depth, cam_intrinsic, depth_scale)

    def project_template_to_image(self, best_pose, pred_object_idx, batch, proposals):
        depth, K = batch["depth"][0], batch["cam_intrinsic"][0]
        t = self.Calculate_the_query_translation(proposals, depth, K, batch["depth_scale"])
        H, W = depth.shape
        poses, pcs = self.ref_data["poses"], self.ref_data["pointcloud"]
        if policy.guard("ism.project_bbox", cuda=t.is_cuda, have=ops.have("project_bbox"), f32=poses.dtype == torch.float32 and pcs.dtype == torch.float32):
            uv, bbox = ops.project_bbox(pcs.contiguous(), poses.contiguous(), pred_object_idx.int().contiguous(),
                                        best_pose.int().contiguous(), t.contiguous(),
                                        K.to(device=t.device, dtype=torch.float32).contiguous(), H, W)
            self._cached_bbox = (uv.data_ptr(), bbox)
            return uv
        R = poses[best_pose, 0:3, 0:3]
        pc = pcs[pred_object_idx, ...]
        posed = pc @ R.transpose(1, 2) + t[:, None, :]
        Kf = K.to(torch.float32)
        homo = posed @ Kf.t()
        uv = (homo / homo[:, :, -1:])[:, :, 0:2].to(torch.int)
        uv[:, :, 0].clamp_(min=0, max=W - 1)
        uv[:, :, 1].clamp_(min=0, max=H - 1)
        return uv


class FrameScorer(ScoringMixin):
    """Stand-alone holder of the mixin's attribute contract (what bench.py and the tests drive
    when the Lightning/Hydra shell of the reference is not installed)."""

    def __init__(self, ref_descriptors, ref_appe_descriptors, poses, pointcloud, confidence_thresh=0.2,
                 aggregation_function="avg_5", visible_thred=0.5):
        from types import SimpleNamespace
        from .loss import PairwiseSimilarity
        self.ref_data = dict(descriptors=ref_descriptors, appe_descriptors=ref_appe_descriptors, poses=poses,
                             pointcloud=pointcloud)
        self.matching_config = SimpleNamespace(metric=PairwiseSimilarity(), aggregation_function=aggregation_function,
                                               confidence_thresh=confidence_thresh)
        self.visible_thred = visible_thred

    def score(self, qry_cls, qry_patch, masks, boxes, depth, K, depth_scale=1.0):
        """Matching stage of run_inference_custom.py:168-200 for one frame.  ``depth`` follows the reference's contract:
        Z [m] = depth * depth_scale / 1000, i.e. a MILLIMETRE map at depth_scale 1 (run_inference_custom.py reads the png as
        int32 mm, trimesh_utils.py:87); a map in metres goes in with depth_scale=1000."""
        from types import SimpleNamespace
        sel, pobj, sem, bt = self.compute_semantic_score(qry_cls)
        qp = qry_patch[sel]
        appe, ref = self.compute_appearance_score(bt, pobj, qp)
        batch = dict(depth=[depth], cam_intrinsic=[K], depth_scale=depth_scale)
        uv = self.project_template_to_image(bt, pobj, batch, masks[sel])
        geo, vr = self.compute_geometric_score(uv, SimpleNamespace(boxes=boxes[sel]), qp, ref, self.visible_thred)
        final = (sem + appe + geo * vr) / (1 + 1 + vr)
        return dict(sel=sel, pred_obj=pobj, semantic=sem, best_template=bt, appearance=appe, iou=geo,
                    visible_ratio=vr, final=final, image_uv=uv)

    def score_frames(self, qry_cls, qry_patch, masks, boxes, depth, K, depth_scale=1.0):
        """The matching stage for F frames in ONE set of launches (frames are independent: SURVEY 8e; the reference loops over
        them, one Lightning step per frame).  qry_cls (F,P,C), qry_patch (F,P,N,C), masks (F,P,H,W), boxes (F,P,4), depth (F,H,W),
        K (F,3,3) or (3,3).  Every per-frame rule of ``score`` holds per frame: a proposal's scores depend on its own frame's depth
        map and camera only, and quirk Q3 of compute_iou (one empty intersection zeroes the IoU of ALL proposals) applies per
        frame.  -> dict of flat tensors over the selected proposals of all frames, in (frame, proposal) order, with ``frame`` (the
        frame of each) and ``sel`` (the proposal index inside its frame): the rows of frame f equal ``score(... frame f ...)``."""
        F_, P = qry_cls.shape[0], qry_cls.shape[1]
        dev = qry_cls.device
        sel, pobj, sem, bt = self.compute_semantic_score(qry_cls.reshape(F_ * P, -1))
        frame = torch.div(sel, P, rounding_mode="floor")
        if sel.numel() == 0:                                  # no proposal above the semantic threshold in any frame
            z = sem.new_zeros(0)
            return dict(frame=frame, sel=sel, pred_obj=pobj, semantic=sem, best_template=bt, appearance=z, iou=z, visible_ratio=z,
                        final=z, image_uv=torch.zeros(0, self.ref_data["pointcloud"].shape[1], 2, dtype=torch.int32, device=dev))
        if not (ops.have("masked_depth_mean") and ops.have("project_bbox") and ops.have("patch_scores") and qry_cls.is_cuda):
            raise RuntimeError("score_frames is the batched device path (fp32 / half descriptors on the GPU); use score() per frame")
        # the selected proposals are NAMED to the kernels (sel32), not copied out: `query_appe_descriptors[idx_selected]` and
        # `masks[idx_selected]` of the reference (detector.py:341-353) moved 1 MB + 1.2 MB per selected proposal through HBM twice
        sel32 = sel.int().contiguous()
        sel_m = sel32
        qall = qry_patch.reshape(F_ * P, *qry_patch.shape[2:])
        if qall.dtype != torch.float32 or not qall.is_contiguous():
            # half descriptors are converted to float32 for the kernel: convert the SELECTED rows only (the index form would convert
            # every proposal's 256 x 1024 descriptors first)
            qall, sel32 = qall[sel].contiguous(), None
        appe, ref = self.compute_appearance_score(bt, pobj, qall, sel=sel32)
        if not isinstance(ref, RefPatchHandle):
            raise RuntimeError("score_frames is the batched device path (fp32 / half descriptors on the GPU); use score() per frame")
        Kf = K if K.dim() == 3 else K[None].expand(F_, 3, 3)
        H, W = depth.shape[-2:]
        mall = masks.reshape(F_ * P, H, W)
        if mall.dtype != torch.float32 or not mall.is_contiguous():
            mall, msel = mall[sel].to(torch.float32).contiguous(), None
        else:
            msel = sel_m
        f32 = frame.int().contiguous()
        poses, pcs = self.ref_data["poses"], self.ref_data["pointcloud"]
        t = ops.masked_depth_mean(mall, depth.to(torch.float32).contiguous(), Kf, float(depth_scale), frame=f32, sel=msel)
        uv, bbox = ops.project_bbox(pcs.contiguous(), poses.contiguous(), pobj.int().contiguous(), bt.int().contiguous(), t.contiguous(),
                                    Kf.to(device=dev, dtype=torch.float32).contiguous(), H, W, frame=f32)
        vr = ref.visible_ratio if ref.thred == self.visible_thred else ops.patch_scores(
            qall.float().contiguous(), ref.store, ref.obj, ref.tmpl, float(self.visible_thred), sel=sel32)[1].to(qall.dtype)
        # compute_iou per proposal, then quirk Q3 per frame: a frame with any empty intersection reports 0.0 for all its proposals
        bb_a, bb_b = bbox.to(boxes.dtype), boxes.reshape(F_ * P, 4)[sel]
        tl = torch.max(bb_a[:, 0:2], bb_b[:, 0:2])
        br = torch.min(bb_a[:, 2:4], bb_b[:, 2:4])
        wh_a, wh_b, wh_i = bb_a[:, 2:4] - bb_a[:, 0:2], bb_b[:, 2:4] - bb_b[:, 0:2], br - tl
        ai = wh_i[:, 0] * wh_i[:, 1]
        iou = ai / (wh_a[:, 0] * wh_a[:, 1] + wh_b[:, 0] * wh_b[:, 1] - ai)
        # per-frame OR as an integer count (accumulating into a bool tensor is backend-defined)
        bad = torch.zeros(F_, dtype=torch.int32, device=dev).index_add_(0, frame, (~(wh_i > 0).all(dim=1)).to(torch.int32)) > 0
        geo = torch.where(bad[frame], torch.zeros_like(iou), iou)
        final = (sem + appe + geo * vr) / (1 + 1 + vr)
        return dict(frame=frame, sel=sel - frame * P, pred_obj=pobj, semantic=sem, best_template=bt, appearance=appe, iou=geo,
                    visible_ratio=vr, final=final, image_uv=uv)

