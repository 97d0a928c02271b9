"""Onboard one object from rendered template views and run a frame on it: ``sam6d_amd.onboarding.onboard`` -> ``FramePipeline``.

    python tools/onboard_demo.py [TEMPLATE_DIR]          (on the GPU box)
    python tools/onboard_demo.py --mesh PATH.ply         mesh file -> rendered views -> onboard -> FramePipeline, in this process

With ``--mesh`` the views are rendered on the device, with the mesh's texture when the file names one (``sam6d_amd.render``: 42 views of 480 x 640 under the LM camera, seeded
rotations at a distance that lets the object fill about two thirds of the view -- the reference's icosphere pose tables are its
data and are not shipped), the model / ISM points are ``sample_surface`` draws of the mesh and the whole onboarding is one
``onboard_from_mesh`` call.  With a directory of ``rgb_i.png`` / ``mask_i.png`` / ``xyz_i.npy`` the views are read from it (``load_template_dir``); without one, 42
synthetic views of an ellipsoid are made at 512 x 512, the size BlenderProc writes when the render script sets none (the
reference's Render/ scripts do not).  Seeded weights at the released model sizes; model / ISM points are taken from the views' xyz
maps and the template poses are identities (the real ones come from the mesh and the icosphere tables, outside this library).

Prints the time of one object's onboarding on the device and its split -- template pre-processing (PEM side, ISM side), the ViT
passes (PEM ViT-B over the views, DINOv2 ViT-L/14 over the templates), furthest point sampling -- and, for scale, the per-template
numpy loop of tests/onboarding_ref.py on the host (the shape of the reference's own computation, the PEM side only).  Each device
time is the median of ``REPEAT`` runs, each ended by a device synchronise, after a warm-up run.  One JSON line at the end."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sam6d_amd import onboarding, ops, pipeline, render  # noqa: E402
from sam6d_amd.ism import dinov2 as pd  # noqa: E402
from sam6d_amd.pem import pose_estimation_model as pm  # noqa: E402
from sam6d_amd.sam.image_encoder import build_vit_h  # noqa: E402
from sam6d_amd.sam.mask_decoder import build_sam_decoder  # noqa: E402
from sam6d_amd.utils import seeded, synth  # noqa: E402

REPEAT = 5


def synthetic_views(T=42, H=512, W=512, seed=0):
    """T views of an ellipsoid (semi-axes 60 / 45 / 35 mm) seen from T directions: rgb (T,H,W,3) u8, mask (T,H,W) u8 {0, 255},
    xyz (T,H,W,3) f32 millimetres in the object frame (0 outside the mask)."""
    g = torch.Generator().manual_seed(seed)
    axes = torch.tensor([60.0, 45.0, 35.0])
    R = torch.linalg.qr(torch.randn(T, 3, 3, generator=g))[0]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    scale = 150.0 / min(H, W)                                          # millimetres per pixel: the object fills about 2/3 of the view
    o = torch.stack([(xs - W / 2) * scale, (ys - H / 2) * scale, torch.full_like(xs, -200.0)], -1)          # ray origins, direction +z
    rgb, mask, xyz = torch.zeros(T, H, W, 3, dtype=torch.uint8), torch.zeros(T, H, W, dtype=torch.uint8), torch.zeros(T, H, W, 3)
    for t in range(T):
        oo, dd = (o @ R[t]) / axes, (torch.tensor([0.0, 0.0, 1.0]) @ R[t]) / axes          # the unit sphere in scaled object coordinates
        a, b, c = (dd * dd).sum(), (oo * dd).sum(-1), (oo * oo).sum(-1) - 1
        disc = b * b - a * c
        hit = disc > 0
        s = (-b - disc.clamp(min=0).sqrt()) / a
        p = (oo + s[..., None] * dd) * axes
        xyz[t] = torch.where(hit[..., None], p, torch.zeros(()))
        mask[t] = hit.to(torch.uint8) * 255
        shade = ((p / axes).abs() * 200 + 40).clamp(0, 255)
        rgb[t] = torch.where(hit[..., None], shade, torch.zeros(())).to(torch.uint8)
    return rgb.numpy(), mask.numpy(), xyz.numpy()


def object_from_views(rgb, mask, xyz, seed=1):
    r = np.random.RandomState(seed)
    surf = xyz[mask == 255] / np.float32(1000.0)
    return dict(rgb=rgb, mask=mask, xyz_mm=xyz, model_points=surf[r.choice(len(surf), 1024, replace=False)],
                ism_points=surf[r.choice(len(surf), 2048, replace=False)], poses=np.tile(np.eye(4, dtype=np.float32), (len(mask), 1, 1)))


MESH_SIZE = (480, 640)
MESH_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])          # the LM camera (pyrender.py:88-91)


def mesh_poses(vertices, T=42, seed=0):
    """T object -> camera poses: seeded rotations about the mesh's centre, which is put on the optical axis at the distance where the
    bounding sphere spans two thirds of the image height."""
    g = torch.Generator().manual_seed(seed)
    R = torch.linalg.qr(torch.randn(T, 3, 3, generator=g, dtype=torch.float64))[0]
    R = R * torch.linalg.det(R)[:, None, None]                          # proper rotations
    c = torch.from_numpy((vertices.max(0) + vertices.min(0)) / 2).double()
    radius = float(np.linalg.norm(vertices - c.numpy(), axis=1).max())
    P = torch.eye(4, dtype=torch.float64).repeat(T, 1, 1)
    P[:, :3, :3] = R
    P[:, :3, 3] = -(R @ c) + torch.tensor([0.0, 0.0, MESH_K[1, 1] * radius / (MESH_SIZE[0] / 3.0)], dtype=torch.float64)
    return P.float()


def object_from_mesh(path, dev):
    """-> (rgb, mask, xyz numpy views, the object dict of ``onboard``, and the arguments of the equivalent ``onboard_from_mesh`` call)."""
    vertices, faces, colors, uv, texture = render.load_textured_ply(path)          # uv, texture: None unless the file names a texture
    poses = mesh_poses(vertices)
    views = render.render_templates(vertices, faces, poses.to(dev), MESH_K, MESH_SIZE, colors=colors, uv=uv, texture=texture)
    su = torch.rand(1, 1024 + 2048, 3, generator=torch.Generator().manual_seed(4))
    pts = render.sample_surface(torch.from_numpy(vertices), torch.from_numpy(faces), 1024 + 2048, su[0])[0] / torch.full((1,), 1000.0)
    rgb, mask, xyz = (views[k].cpu().numpy() for k in ("rgb", "mask", "xyz_mm"))
    obj = dict(rgb=rgb, mask=mask, xyz_mm=xyz, model_points=pts[:1024].numpy(), ism_points=pts[1024:].numpy(), poses=poses.numpy())
    return rgb, mask, xyz, obj, dict(meshes=[(vertices, faces, colors, uv, texture)], poses=poses.to(dev), surface_uniforms=su)


def models(dev):
    dino = pd.CustomDINOv2.__new__(pd.CustomDINOv2)
    torch.nn.Module.__init__(dino)
    dino.model = seeded.load_seeded(pd._make_dinov2_model(arch_name="vit_large").eval(), 6).to(dev)
    dino.patch_size, dino.validpatch_thresh, dino.chunk_size, dino.proposal_size, dino.token_name = 14, 0.5, 128, 224, "x_norm_clstoken"
    return dino, seeded.load_seeded(pm.Net(pm.default_cfg()).eval(), 1).to(dev)


def timed(fn):
    fn()                                                               # warm-up: code objects, allocator, library algorithm choice
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPEAT):
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), out


def main():
    dev = torch.device("cuda", 0)
    mesh = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--mesh" else None
    if mesh:
        rgb, mask, xyz, obj, mesh_args = object_from_mesh(mesh, dev)
    else:
        rgb, mask, xyz = onboarding.load_template_dir(sys.argv[1]) if len(sys.argv) > 1 else synthetic_views()
        obj = object_from_views(rgb, mask, xyz)
    T, H, W = mask.shape
    dino, net = models(dev)
    keys = torch.rand(1, T, H * W, generator=torch.Generator().manual_seed(2)).to(dev)
    d_rgb, d_mask, d_xyz = (torch.from_numpy(a).to(dev) for a in (rgb, mask, xyz))
    res = dict(views=T, height=H, width=W, n_sample=5000, img_size=224)
    if mesh:
        v, f, c, uv, tex = mesh_args["meshes"][0]
        res.update(mesh=os.path.basename(mesh), vertices=len(v), faces=len(f), covered_pixels_per_view=int((mask == 255).sum()) // T,
                   texture=None if tex is None else list(tex.shape[:2]))
        res["render_ms"], _ = timed(lambda: render.render_templates(v, f, mesh_args["poses"], MESH_K, MESH_SIZE, colors=c, uv=uv, texture=tex))
        res["onboard_ms"], onb = timed(lambda: render.onboard_from_mesh(dino, net, mesh_args["meshes"], mesh_args["poses"], MESH_K, MESH_SIZE,
                                                                        surface_uniforms=mesh_args["surface_uniforms"], keys=keys, n_view=T))
        ref = onboarding.onboard(dino, net, [obj], keys=keys, n_view=T)
        res["equals_onboard_on_the_views"] = bool(torch.equal(onb.pem_templates["dense_fo"], ref.pem_templates["dense_fo"]) and
                                                  torch.equal(onb.scorer.ref_data["descriptors"], ref.scorer.ref_data["descriptors"]))
    else:
        res["onboard_ms"], onb = timed(lambda: onboarding.onboard(dino, net, [obj], keys=keys, n_view=T))
    res["pem_pre_ms"], (tem_rgb, tem_pts, tem_choose) = timed(lambda: onboarding.pem_template_inputs(d_rgb, d_mask, d_xyz, keys=keys[0]))
    res["ism_pre_ms"], (tem, msk) = timed(lambda: onboarding.ism_template_inputs(d_rgb, d_mask, 224))
    cnt, box, _ = ops.template_boxes(d_mask)
    res["boxes_kernel_ms"], _ = timed(lambda: ops.template_boxes(d_mask))
    res["points_kernel_ms"], (_, _, n) = timed(lambda: ops.template_points(d_mask, d_xyz, box, min(H, W) ** 2))
    res["sampler_kernel_ms"], _ = timed(lambda: ops.pem_sample_indices(keys[0], n, 5000))
    res["pem_crops_kernel_ms"], _ = timed(lambda: ops.template_pem_crops(d_rgb, d_mask, box, 224, True, onboarding.pre.MEAN, onboarding.pre.STD))
    with torch.no_grad():
        fe = net.feature_extraction
        res["pem_vit_ms"], feats = timed(lambda: [fe.get_img_feats(t, c) for t, c in zip(tem_rgb, tem_choose)])
        pts = torch.cat(tem_pts, 1).contiguous()
        res["fps_ms"], _ = timed(lambda: ops.furthest_point_sampling(pts, fe.npoint))
        res["get_obj_feats_ms"], _ = timed(lambda: fe.get_obj_feats(tem_rgb, tem_pts, tem_choose))
        res["dinov2_ms"], _ = timed(lambda: (dino.compute_features(tem, token_name="x_norm_clstoken"), dino.compute_masked_patch_feature(tem, msk)))
    # the host loop, once (seconds): one template at a time, as the reference's _get_template does
    from tests import onboarding_ref
    k_host = keys[0].cpu().numpy()
    t = time.perf_counter()
    for i in range(T):
        onboarding_ref.pem_template(rgb[i], mask[i], xyz[i], k_host[i], n_sample=5000, img_size=224)
    res["host_numpy_loop_pem_ms"] = (time.perf_counter() - t) * 1e3
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)
    # ---- a frame on the onboarded object -----------------------------------------------------------------------------------------
    enc = seeded.load_seeded(build_vit_h().eval(), 3).to(dev)
    dec = seeded.load_seeded(build_sam_decoder(), 2).to(dev)
    onb.scorer.matching_config.confidence_thresh = -1.0                # seeded descriptors match no template: let every proposal through
    pipe = pipeline.FramePipeline(enc, dec.prompt_encoder, dec.mask_decoder, dino, onb.scorer, net, onb.pem_templates,
                                  object_radius=onb.object_radius, top_k=10,
                                  segmentor=dict(pred_iou_thresh=0.09, stability_score_thresh=0.3, stability_score_offset=0.02))
    frame = synth.pem_pre_inputs(P=128, seed=3)
    args = (torch.from_numpy(frame["image"]).to(dev), frame["depth"].to(dev), frame["K"].to(dev),
            torch.rand(16, 480 * 640, generator=torch.Generator().manual_seed(1)).to(dev), synth.coarse_uniforms(16, 2).to(dev))
    det, poses = pipe(*args)
    torch.cuda.synchronize()
    res["frame_detections"] = int(det.masks.shape[0])
    res["frame_poses"] = 0 if poses is None else int(poses["pred_R"].shape[0])
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
