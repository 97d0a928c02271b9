"""ISM -> PEM hand-off and result records.

The reference passes detections between its two models through files: per-frame ``.npz`` (Detections.save_to_file,
Instance_Segmentation_Model/model/utils.py:162-181), converted to one BOP-style JSON list whose masks are uncompressed
column-major RLE produced by a per-pixel Python loop (``mask_to_rle`` :24-43, ``convert_npz_to_json`` :199-216), which the
PEM data provider decodes again (Pose_Estimation_Model/utils/data_utils.py:72-89).  In one process per GPU the masks can
stay device tensors (``Detections`` below is that hand-off); when the unchanged eval scripts need the files, the same
records are produced from the tensors: the run lengths come from ONE pass of tensor ops over all masks (transitions ->
positions -> differences) instead of H*W Python iterations per mask, byte-identical with the reference's JSON.
"""
import json
from dataclasses import dataclass

import numpy as np
import torch

LMO_OBJECT_IDS = np.array([1, 5, 6, 8, 9, 10, 11, 12])                # model/utils.py:11-22


@dataclass
class Detections:
    """What the PEM stage needs from the ISM stage for one frame (the in-memory replacement of the JSON round trip):
    masks (N,H,W) bool, boxes (N,4) XYXY, scores (N,), object_ids (N,) zero-based, plus the frame identifiers."""
    scene_id: int
    image_id: int
    masks: torch.Tensor
    boxes: torch.Tensor
    scores: torch.Tensor
    object_ids: torch.Tensor
    runtime: float = 0.0

    # ---- the per-frame list operations of the reference's Detections (model/utils.py:80-132) -----------------------------
    _FIELDS = ("masks", "boxes", "scores", "object_ids")

    def __len__(self):
        return self.boxes.shape[0]

    def filter(self, idx):
        """Keep the rows ``idx`` (bool mask or index tensor) of every per-detection tensor (model/utils.py:filter; fields
        that are not filled yet -- scores / object_ids before the scoring stage -- are left alone)."""
        n = len(self)
        for f in self._FIELDS:
            v = getattr(self, f)
            if v is not None and v.shape[0] == n:
                setattr(self, f, v[idx])
        return self

    def remove_very_small_detections(self, min_box_size, min_mask_size):
        """model/utils.py:96-105: keep detections whose box covers more than min_box_size**2 of the frame AND whose mask
        covers more than min_mask_size of it (the asymmetry -- one threshold squared, the other not -- is the
        reference's; configs/model/ISM_sam.yaml:15-16 sets 0.05 and 3e-4)."""
        img_area = self.masks.shape[1] * self.masks.shape[2]
        b = self.boxes
        box_areas = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) / img_area          # torchvision box_area
        mask_areas = self.masks.sum(dim=(1, 2)) / img_area
        return self.filter(torch.logical_and(box_areas > min_box_size ** 2, mask_areas > min_mask_size))

    def apply_nms(self, nms_thresh=0.5, nms_fn=None):
        """model/utils.py:121-126."""
        nms_fn = nms_fn or _device_nms
        return self.filter(nms_fn(self.boxes.float(), self.scores.float(), nms_thresh))

    def apply_nms_per_object_id(self, nms_thresh=0.5, nms_fn=None):
        """model/utils.py:107-119: one NMS per predicted object, survivors concatenated in ascending object id, inside
        an object by decreasing score.  ``nms_fn(boxes, scores, thresh) -> kept indices by decreasing score``; default the
        device kernel (sam6d_amd.ops.nms -> s6d_nms_f32)."""
        nms_fn = nms_fn or _device_nms
        every = torch.arange(len(self), device=self.boxes.device)
        keep = []
        for oid in torch.unique(self.object_ids):
            sel = self.object_ids == oid
            keep.append(every[sel][nms_fn(self.boxes[sel].float(), self.scores[sel].float(), nms_thresh)])
        if not keep:
            return self                                               # nothing to do for an empty frame (the reference raises)
        return self.filter(torch.cat(keep))


def _device_nms(boxes, scores, thresh):
    from .. import ops
    return ops.nms(boxes.contiguous(), scores.contiguous(), thresh)


def masks_to_rle(masks):
    """(N,H,W) bool/0-1 tensor (any device) -> list of {"counts": [...], "size": [H, W]}: uncompressed COCO-style RLE in
    column-major order starting with the zero run (possibly 0 long), exactly model/utils.py:mask_to_rle."""
    m = (masks > 0) if masks.dtype != torch.bool else masks
    N, H, W = m.shape
    flat = m.transpose(1, 2).reshape(N, H * W)                          # column-major ("F") pixel order
    prev = torch.cat([torch.zeros(N, 1, dtype=torch.bool, device=m.device), flat[:, :-1]], dim=1)
    change = flat != prev                                               # a run starts here (virtual 0 before pixel 0)
    idx = torch.nonzero(change)                                         # sorted by mask, then position
    per_mask = torch.bincount(idx[:, 0], minlength=N).cpu().tolist()
    pos = idx[:, 1].cpu().numpy()
    out, a = [], 0
    for n in range(N):
        p = pos[a:a + per_mask[n]]
        a += per_mask[n]
        edges = np.concatenate([[0], p, [H * W]])
        out.append({"counts": np.diff(edges).tolist(), "size": [H, W]})
    return out


def rle_to_mask(rle):
    """Inverse (Pose_Estimation_Model/utils/data_utils.py:72-89), vectorised."""
    h, w = rle["size"]
    counts = np.asarray(rle["counts"], dtype=np.int64)
    vals = (np.arange(len(counts)) % 2).astype(bool)
    return np.repeat(vals, counts).reshape(h, w, order="F")


# ------------------------------------------------------------------------------------------- run lists as tensors
def _rle_kernels(site, t, name):
    from .. import ops, policy
    return policy.guard(site, cuda=t.is_cuda, have=ops.have(name))


def _rle_encode_library(m):
    """The library statement of the encoder: (N,H,W) bool -> (counts (R,) int32, offsets (N+1,) int64), the transitions of
    ``masks_to_rle`` kept as tensors."""
    N, H, W = m.shape
    dev = m.device
    flat = m.transpose(1, 2).reshape(N, H * W)
    prev = torch.cat([torch.zeros(N, 1, dtype=torch.bool, device=dev), flat[:, :-1]], dim=1)
    idx = torch.nonzero(flat != prev)                                   # sorted by mask, then position
    runs = torch.bincount(idx[:, 0], minlength=N) + 1                   # K transitions bound K + 1 runs
    offsets = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    torch.cumsum(runs, 0, out=offsets[1:])
    R = idx.shape[0] + N
    start = torch.zeros(R, dtype=torch.int64, device=dev)               # where every run begins: 0, then the mask's transitions
    start[torch.arange(idx.shape[0], device=dev) + idx[:, 0] + 1] = idx[:, 1]
    end = torch.cat([start[1:], start.new_zeros(1)])
    if N:
        end[offsets[1:] - 1] = H * W
    return (end - start).int(), offsets


def _rle_check_library(counts, offsets, H, W):
    """(ends, base (N,)) of valid lists; ValueError naming the first mask with a negative count, an empty list or a wrong total."""
    N = offsets.shape[0] - 1
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    lens = offsets[1:] - offsets[:-1]
    padded = torch.cat([ends.new_zeros(1), ends])
    total = padded[offsets[1:]] - padded[offsets[:-1]]
    which = torch.repeat_interleave(torch.arange(N, device=counts.device), lens)
    negative = torch.zeros(N, dtype=torch.bool, device=counts.device)
    negative[which[counts < 0]] = True
    bad = torch.nonzero(negative | (lens < 1) | (total != H * W))
    if bad.shape[0]:
        raise ValueError(f"mask {int(bad[0, 0])} is not a run list of {H} x {W} pixels (a negative count, an empty list, or the counts "
                         f"do not sum to {H * W})")
    return which


def _rle_to_masks_library(counts, offsets, H, W):
    """The library statement of the dense decoder -> (N,H,W) uint8: every run's parity repeated its length."""
    N = offsets.shape[0] - 1
    which = _rle_check_library(counts, offsets, H, W)
    parity = ((torch.arange(counts.shape[0], device=counts.device) - offsets[:-1][which]) & 1).to(torch.uint8)
    flat = torch.repeat_interleave(parity, counts.long())
    return flat.reshape(N, W, H).transpose(1, 2).contiguous()


def _pack_library(masks):
    """The library statement of ``ops.mask_pack``: (N,H,W) uint8 -> (packed (N, ceil(H W / 64)) int64, area (N,) int32)."""
    N = masks.shape[0]
    HW = masks.shape[1] * masks.shape[2]
    words = (HW + 63) // 64
    bits = torch.zeros(N, words * 64, dtype=torch.int64, device=masks.device)
    bits[:, :HW] = (masks.reshape(N, HW) != 0).long()
    weight = torch.tensor([1 << k for k in range(63)] + [-(1 << 63)], dtype=torch.int64, device=masks.device)
    return (bits.reshape(N, words, 64) * weight).sum(2), bits.sum(1).int()


@dataclass
class RleMasks:
    """N masks of one size as run lists on one device: ``counts`` (R,) int32, the lists one after the other;
    ``offsets`` (N+1,) int64, the list of mask n being counts[offsets[n]:offsets[n+1]]; ``size`` = (H, W).  Pixel order is
    column-major (p = x H + y); a list starts with its run of zeros.  ``from_masks`` writes the canonical form (what
    ``masks_to_rle`` writes); the decoders also take zero-length runs anywhere and refuse, with a ValueError that names the mask, a
    negative count, an empty list and a total other than H W.  On CUDA tensors the work is done by the kernels of ``ops.rle_*``, on
    CPU tensors and under ``policy.disable_fused`` by the torch statements above."""
    counts: torch.Tensor
    offsets: torch.Tensor
    size: tuple

    def __len__(self):
        return self.offsets.shape[0] - 1

    @property
    def device(self):
        return self.counts.device

    def to(self, device):
        return RleMasks(self.counts.to(device), self.offsets.to(device), self.size)

    @classmethod
    def from_masks(cls, masks):
        """(N,H,W) bool / uint8 (non-zero = set; other dtypes: > 0, as ``masks_to_rle``) on any device."""
        from .. import ops
        m = torch.as_tensor(masks)
        if m.dim() != 3 or m.shape[1] * m.shape[2] < 1:
            raise ValueError(f"masks must have shape (N,H,W) with H W >= 1, got {tuple(m.shape)}")
        if m.dtype not in (torch.bool, torch.uint8):
            m = m > 0
        size = (int(m.shape[1]), int(m.shape[2]))
        if _rle_kernels("handoff.rle_encode", m, "rle_encode"):
            return cls(*ops.rle_encode(m.contiguous()), size)
        return cls(*_rle_encode_library(m if m.dtype == torch.bool else m != 0), size)

    @classmethod
    def from_records(cls, segmentations, device=None, size=None):
        """The ``{"counts": [...], "size": [H, W]}`` dicts of a result file -> RleMasks on ``device``: ONE flat host array (offsets,
        then every count) and one upload.  Mixed sizes and compressed RLE strings are refused; ``size`` is needed only for an empty
        list of records."""
        segs = list(segmentations)
        for n, s in enumerate(segs):
            if isinstance(s.get("counts"), (str, bytes)):
                raise ValueError(f"segmentation {n} is a COMPRESSED RLE string: only uncompressed run-length lists are read")
        sizes = {tuple(int(v) for v in s["size"]) for s in segs}
        if size is not None:
            sizes.add(tuple(int(v) for v in size))
        if len(sizes) != 1:
            raise ValueError(f"the segmentations must share one size, got {sorted(sizes)}" if sizes else "no segmentation and no size")
        N = len(segs)
        lens = np.fromiter((len(s["counts"]) for s in segs), np.int64, N)
        flat = np.zeros(N + 1 + int(lens.sum()), np.int64)
        np.cumsum(lens, out=flat[1:N + 1])
        if N:
            flat[N + 1:] = np.concatenate([np.asarray(s["counts"], np.int64).reshape(-1) for s in segs])
        if flat[N + 1:].size and (flat[N + 1:].max() >= 2 ** 31 or flat[N + 1:].min() < -2 ** 31):
            raise ValueError("a run length does not fit 32 bits")
        dev = torch.from_numpy(flat).to(device if device is not None else "cpu")
        return cls(dev[N + 1:].int(), dev[:N + 1].contiguous(), next(iter(sizes)))

    @classmethod
    def cat(cls, parts):
        """Several batches of one size and device, one after the other."""
        parts = list(parts)
        if not parts or len({tuple(p.size) for p in parts}) != 1:
            raise ValueError(f"batches of one size expected, got {[tuple(p.size) for p in parts]}")
        offsets, base = [parts[0].offsets[:1]], 0
        for p in parts:
            offsets.append(p.offsets[1:] + base)
            base += p.counts.shape[0]
        return cls(torch.cat([p.counts for p in parts]), torch.cat(offsets), parts[0].size)

    def to_records(self):
        """-> [{"counts": [...], "size": [H, W]}]; for lists made by ``from_masks`` exactly ``masks_to_rle`` of the masks."""
        c, o = self.counts.cpu().numpy(), self.offsets.cpu().tolist()
        size = [int(self.size[0]), int(self.size[1])]
        return [{"counts": c[o[n]:o[n + 1]].tolist(), "size": list(size)} for n in range(len(self))]

    def to_dense(self):
        """-> (N,H,W) bool on the lists' device."""
        from .. import ops
        H, W = self.size
        if _rle_kernels("handoff.rle_to_dense", self.counts, "rle_to_masks"):
            return ops.rle_to_masks(self.counts.contiguous(), self.offsets.contiguous(), H, W).view(torch.bool)
        return _rle_to_masks_library(self.counts, self.offsets, H, W).view(torch.bool)

    def packed(self):
        """-> (packed (N, ceil(H W / 64)) int64, area (N,) int32): what ``ops.mask_pack`` makes of the dense masks (bit k of word j =
        row-major pixel 64 j + k), without the dense masks on the kernel path."""
        from .. import ops
        H, W = self.size
        if _rle_kernels("handoff.rle_packed", self.counts, "rle_to_packed"):
            return ops.rle_to_packed(self.counts.contiguous(), self.offsets.contiguous(), H, W)
        return _pack_library(_rle_to_masks_library(self.counts, self.offsets, H, W))

    def __getitem__(self, idx):
        """Rows by a bool mask or an index array / tensor / list / slice -> RleMasks (plain tensor statements on the lists' device)."""
        dev = self.counts.device
        if isinstance(idx, slice):
            idx = torch.arange(len(self), device=dev)[idx]
        idx = torch.as_tensor(np.asarray(idx) if not torch.is_tensor(idx) else idx).to(dev)
        if idx.dtype == torch.bool:
            if idx.shape[0] != len(self):
                raise IndexError(f"a bool selection of {idx.shape[0]} rows for {len(self)} masks")
            idx = torch.nonzero(idx)[:, 0]
        idx = idx.long().reshape(-1)
        if idx.shape[0] and (int(idx.min()) < -len(self) or int(idx.max()) >= len(self)):
            raise IndexError(f"row out of range for {len(self)} masks")
        idx = torch.where(idx < 0, idx + len(self), idx)
        lens = (self.offsets[1:] - self.offsets[:-1])[idx]
        offsets = torch.zeros(idx.shape[0] + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=offsets[1:])
        src = torch.repeat_interleave(self.offsets[:-1][idx] - offsets[:-1], lens) + torch.arange(int(offsets[-1]), device=dev)
        return RleMasks(self.counts[src], offsets, self.size)


def detections_from_records(records, device=None, dataset_name="ycbv"):
    """The records of a result file (``detection_records`` / ``save_json_bop23``) -> a list of ``Detections``, one per
    (scene_id, image_id) in the order the file first names them: the file-driven counterpart of the reference's ISM file -> PEM
    flow (Pose_Estimation_Model/provider/bop_test_dataset.py:110-120).  The masks are decoded on ``device`` from ONE upload of all
    run lists; object_ids invert the category mapping of ``detection_records`` (``LMO_OBJECT_IDS`` for "lmo", otherwise
    category - 1); scores float32; ``runtime`` is the first record's ``time``.  Boxes are (x, y, x + w, y + h) in float32: NOT
    claimed to be the bits of the XYXY box whose x2 - x1 wrote the file (a rounded difference added back need not return x2)."""
    records = list(records)
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    rle = RleMasks.from_records([r["segmentation"] for r in records], device) if records else None
    frames = {}
    for i, r in enumerate(records):
        frames.setdefault((int(r["scene_id"]), int(r["image_id"])), []).append(i)
    out = []
    for (scene, im), rows in frames.items():
        cat = np.array([int(records[i]["category_id"]) for i in rows], np.int64)
        if dataset_name == "lmo":
            obj = np.searchsorted(LMO_OBJECT_IDS, cat).clip(max=len(LMO_OBJECT_IDS) - 1)
            if not np.array_equal(LMO_OBJECT_IDS[obj], cat):
                raise ValueError(f"scene {scene} image {im}: a category_id is not an LM-O object ({sorted(set(cat.tolist()))})")
        else:
            obj = cat - 1
        b = np.array([records[i]["bbox"] for i in rows], np.float64).reshape(-1, 4)
        xyxy = np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1).astype(np.float32)
        out.append(Detections(scene_id=scene, image_id=im, masks=rle[np.asarray(rows, np.int64)].to_dense(),
                              boxes=torch.from_numpy(xyxy).to(device),
                              scores=torch.tensor([float(records[i]["score"]) for i in rows], dtype=torch.float32, device=device),
                              object_ids=torch.from_numpy(obj.astype(np.int64)).to(device),
                              runtime=float(records[rows[0]].get("time", 0.0))))
    return out


def detection_records(det: Detections, dataset_name):
    """The per-detection dicts of convert_npz_to_json (model/utils.py:199-216) for one frame, from device tensors:
    category ids shifted as in save_to_file :171-173, boxes XYXY -> XYWH without the +1 (the (N,4) branch of
    utils/bbox_utils.py:134-136).  The run lists of CUDA masks come from the encoder kernels (``RleMasks.from_masks``), the same
    lists as ``masks_to_rle``'s, which serves CPU masks and ``policy.disable_fused``."""
    obj = det.object_ids.cpu().numpy()
    cat = LMO_OBJECT_IDS[obj] if dataset_name == "lmo" else obj + 1
    b = det.boxes.cpu().numpy()
    xywh = np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], axis=1)
    m = det.masks
    if m.dtype in (torch.bool, torch.uint8) and m.shape[0] and _rle_kernels("handoff.detection_records", m, "rle_encode"):
        rles = RleMasks.from_masks(m).to_records()
    else:
        rles = masks_to_rle(m)
    scores = det.scores.cpu().numpy()
    return [{"scene_id": int(det.scene_id), "image_id": int(det.image_id), "category_id": int(cat[i]),
             "bbox": xywh[i].tolist(), "score": float(scores[i]), "time": float(det.runtime), "segmentation": rles[i]}
            for i in range(len(rles))]


def save_json_bop23(path, records):
    """utils/inout.py:62-65."""
    with open(path, "w") as f:
        json.dump(records, f)
