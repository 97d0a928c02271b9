"""Template onboarding on the MI355X: the case table of tests/onboarding_ref.py through the kernels, bit for bit against the
restatement of the reference, and ``onboard`` with two objects on a seeded PEM Net and a small seeded DINOv2.

The one tolerance: ``dense_fo`` within rtol 1e-3 / atol 1e-4 of ``get_obj_feats`` on the reference-made inputs -- the bound of the
pixels-to-pose onboarding assertion (tests/test_gpu_zz_pipeline_e2e.py, "template features"); everything else is ``equal``."""
import numpy as np
import pytest
import torch

from oracle import pem_pre as o
from sam6d_amd import onboarding as ob
from sam6d_amd import ops, policy
from sam6d_amd.pem import preprocess as pre
from sam6d_amd.utils import seeded
from tests import onboarding_ref as R

pytestmark = pytest.mark.gpu

GOOD = [i for i in range(R.T) if i != R.EMPTY_VIEW]


@pytest.fixture(scope="module")
def case():
    c = R.case_templates()
    return c, {k: torch.from_numpy(v).cuda() for k, v in c.items()}


def test_boxes_and_points_kernels(case):
    c, d = case
    cnt, box, tight = ops.template_boxes(d["mask"])
    choose, pts, n = ops.template_points(d["mask"], d["xyz"], box, min(R.H, R.W) ** 2)
    cnt, box, tight, choose, pts, n = (t.cpu() for t in (cnt, box, tight, choose, pts, n))
    for i in range(R.T):
        m = c["mask"][i]
        assert int(cnt[i]) == int((m == 255).sum())
        assert box[i].tolist() == [int(v) for v in o.get_bbox(m == 255 if i != R.EMPTY_VIEW else np.ones_like(m))], i
        assert tight[i].tolist() == (R.pil_bbox(m) or [0, 0, 0, 0]), i
        y1, y2, x1, x2 = box[i].tolist()
        want = (m[y1:y2, x1:x2] == 255).astype(np.float32).flatten().nonzero()[0]
        assert int(n[i]) == len(want)
        np.testing.assert_array_equal(choose[i, :len(want)].numpy(), want)
        np.testing.assert_array_equal(pts[i, :len(want)].numpy(), (c["xyz"][i] / 1000.0)[y1:y2, x1:x2, :].reshape(-1, 3)[want])


@pytest.mark.parametrize("flag", [True, False])
def test_pem_template_inputs_equal_the_restatement(case, flag):
    c, d = case
    kw = dict(n_sample=R.N_SAMPLE, img_size=R.S, rgb_mask_flag=flag)
    want = R.pem_templates(c["rgb"][None, GOOD], c["mask"][None, GOOD], c["xyz"][None, GOOD], c["keys"][None, GOOD], **kw)
    with policy.use(strict="1"):
        got = ob.pem_template_inputs(d["rgb"][GOOD], d["mask"][GOOD], d["xyz"][GOOD], keys=d["keys"][GOOD], **kw)
    for g_, w_ in zip(got, want):
        for v in range(len(GOOD)):
            np.testing.assert_array_equal(g_[v].cpu().numpy(), w_[v], err_msg=f"view {GOOD[v]}")
    with policy.use(onboard="library"):
        lib = ob.pem_template_inputs(d["rgb"][GOOD], d["mask"][GOOD], d["xyz"][GOOD], keys=d["keys"][GOOD], **kw)
    assert all(torch.equal(a, b) for x, y in zip(got, lib) for a, b in zip(x, y))


def test_pem_crops_kernel_at_odd_sides(case):
    c, d = case
    odd = [(7, (3, 70)), (23, (40, 5)), (33, (39, 47)), (5, (67, 91))]
    box = torch.tensor([[y, y + s, x, x + s] for s, (y, x) in odd])
    views = [5, 10, 5, 9]
    for flag in (True, False):
        got = ops.template_pem_crops(d["rgb"][views].contiguous(), d["mask"][views].contiguous(), box.cuda(), R.S, flag, pre.MEAN, pre.STD).cpu()
        for i, (y1, y2, x1, x2) in enumerate(box.tolist()):
            crop = c["rgb"][views[i]][:, :, ::-1][y1:y2, x1:x2, :]
            if flag:
                crop = crop * (c["mask"][views[i]][y1:y2, x1:x2, None] == 255).astype(np.uint8)
            want = (o.cv2_resize_linear_u8(crop, R.S).astype(np.float32) / np.float32(255) - o.MEAN) / o.STD
            assert np.array_equal(got[i].numpy(), want.transpose(2, 0, 1)), (i, flag)


def test_sampler_kernel_serves_5000_samples():
    g = torch.Generator().manual_seed(12)
    L = 96 * 128
    n = torch.tensor([L, 5000, 4999, L, 9216, L])
    keys = torch.rand(len(n), L, generator=g)
    keys[3] = (keys[3] * 1e4).floor() / 1e4
    keys[4] = (keys[4] * 1e4).floor() / 1e4
    keys[5] = torch.where(keys[5] < 0.9, torch.full_like(keys[5], 0.25), keys[5])
    idx, overflow = ops.pem_sample_indices(keys.cuda(), n.cuda(), 5000)
    assert overflow.tolist() == [0, 0, 0, 0, 0, 1]
    for r in range(5):
        np.testing.assert_array_equal(idx[r].cpu().numpy(), o.sample_indices(int(n[r]), 5000, keys[r].numpy()), err_msg=f"row {r}")
    idx512, ov = ops.pem_sample_indices(keys.cuda(), n.cuda(), 512)
    assert ov.tolist() == [0] * 5 + [1]
    for r in range(5):
        np.testing.assert_array_equal(idx512[r].cpu().numpy(), o.sample_indices(int(n[r]), 512, keys[r].numpy()))
    # the duplicated row through the public call: a whole-view mask (9216 points), the fall-back gives the defined sampler's picks
    rs = np.random.RandomState(3)
    rgb = rs.randint(0, 256, (1, 96, 128, 3)).astype(np.uint8)
    xyz = (rs.standard_normal((1, 96, 128, 3)) * 50).astype(np.float32)
    mask = np.full((1, 96, 128), 255, np.uint8)
    got = ob.pem_template_inputs(torch.from_numpy(rgb).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(xyz).cuda(),
                                 keys=keys[5:6].cuda(), n_sample=5000, img_size=R.S)
    want = R.pem_templates(rgb[None], mask[None], xyz[None], keys[5:6].numpy()[None], n_sample=5000)
    for g_, w_ in zip(got, want):
        np.testing.assert_array_equal(g_[0].cpu().numpy(), w_[0])


@pytest.mark.parametrize("normalize", [False, True])
def test_ism_template_inputs_equal_the_restatement(case, normalize):
    c, d = case
    with policy.use(strict="1"):
        tem, msk = ob.ism_template_inputs(d["rgb"][GOOD], d["mask"][GOOD], R.S, normalize)
    want_t, want_m = R.ism_templates(c["rgb"][GOOD], c["mask"][GOOD], R.S, normalize)
    assert torch.equal(tem.cpu(), want_t) and torch.equal(msk.cpu(), want_m)
    mean, std = torch.tensor(ob.RGB_MEAN), torch.tensor(ob.RGB_STD)
    pad = ((torch.zeros(3) - mean) / std)[:, None].expand(3, R.S) if normalize else torch.zeros(3, R.S)
    assert torch.equal(tem[2][:, :, 0].cpu(), pad)
    with policy.use(onboard="library"):
        lib_t, lib_m = ob.ism_template_inputs(d["rgb"][GOOD], d["mask"][GOOD], R.S, normalize)
    assert torch.equal(lib_t, tem) and torch.equal(lib_m, msk)
    with pytest.raises(ValueError, match=r"template view\(s\) \[13\]"):
        ob.ism_template_inputs(d["rgb"], d["mask"], R.S, normalize)
    with pytest.raises(ValueError, match=r"view\(s\) 13 of object 0"):
        ob.pem_template_inputs(d["rgb"], d["mask"], d["xyz"], keys=d["keys"], n_sample=32, img_size=R.S)


def test_onboard_two_objects(case):
    """onboard -> the PEM's inputs, dense_po / dense_fo and the scorer's descriptors are those of the reference-made inputs; under
    strict mode (the PEM extractor in IEEE half, as benched) the whole call takes no library branch.
    Four views of 600 points each: get_obj_feats of Net(default_cfg()) samples 2048 template points, so three views of 600 (1800
    points) are fewer than it can be given (s6d_fps_f32 refuses M > N)."""
    from sam6d_amd.ism import dinov2 as pd
    from sam6d_amd.pem import pose_estimation_model as pm
    c, d = case
    dev = torch.device("cuda", 0)
    net = seeded.load_seeded(pm.Net(pm.default_cfg()).eval(), 1).to(dev)
    desc = pd.CustomDINOv2.__new__(pd.CustomDINOv2)
    torch.nn.Module.__init__(desc)
    desc.model = seeded.load_seeded(pd.DinoVisionTransformer(img_size=56, patch_size=14, embed_dim=256, depth=2, num_heads=4, mlp_ratio=4,
                                                             init_values=1.0, block_chunks=0).eval(), 6).to(dev)
    desc.patch_size, desc.validpatch_thresh, desc.chunk_size, desc.proposal_size, desc.token_name = 14, 0.5, 64, 56, "x_norm_clstoken"
    pick = [[0, 1, 5, 3, 4, 10], [7, 10, 11, 9, 8, 2]]
    rs = np.random.RandomState(2)
    objects = [dict(rgb=c["rgb"][p], mask=c["mask"][p], xyz_mm=c["xyz"][p], model_points=(rs.standard_normal((64, 3)) * 0.05).astype(np.float32),
                    ism_points=(rs.standard_normal((32, 3)) * 0.05).astype(np.float32), poses=np.tile(np.eye(4, dtype=np.float32), (6, 1, 1)))
               for p in pick]
    keys = torch.from_numpy(c["keys"][pick])
    kw = dict(n_view=4, n_sample=600, img_size=224)
    got = ob.onboard(desc, net, objects, keys=keys, **kw)
    want = R.pem_templates(c["rgb"][pick], c["mask"][pick], c["xyz"][pick], c["keys"][pick], **kw)
    inputs = ob.pem_template_inputs(torch.from_numpy(c["rgb"][pick]).cuda(), torch.from_numpy(c["mask"][pick]).cuda(),
                                    torch.from_numpy(c["xyz"][pick]).cuda(), keys=keys.cuda(), **kw)
    for g_, w_ in zip(inputs, want):
        assert len(g_) == 4
        for v in range(4):
            np.testing.assert_array_equal(g_[v].cpu().numpy(), w_[v])
    with torch.no_grad():
        ref_po, ref_fo = net.feature_extraction.get_obj_feats(*[[torch.from_numpy(a).to(dev) for a in lst] for lst in want])
    assert torch.equal(got.pem_templates["dense_po"], ref_po)
    torch.testing.assert_close(got.pem_templates["dense_fo"], ref_fo, rtol=1e-3, atol=1e-4)
    rd = got.scorer.ref_data
    for ob_i, p in enumerate(pick):
        tem, msk = R.ism_templates(c["rgb"][p], c["mask"][p], 56)
        assert torch.equal(ob.ism_template_inputs(d["rgb"][p], d["mask"][p], 56)[0].cpu(), tem)
        assert torch.equal(rd["descriptors"][ob_i], desc.compute_features(tem.to(dev), token_name="x_norm_clstoken"))
        assert torch.equal(rd["appe_descriptors"][ob_i], desc.compute_masked_patch_feature(tem.to(dev), msk.to(dev)))
    assert rd["poses"].shape == (6, 4, 4) and rd["pointcloud"].shape == (2, 32, 3) and got.pem_templates["model"].shape == (2, 64, 3)
    want_r = [float(np.max(np.linalg.norm(ob_["model_points"], axis=1))) for ob_ in objects]
    np.testing.assert_allclose(got.object_radius.cpu().numpy(), want_r, rtol=1e-6)
    with pytest.raises(ValueError, match="2048 template points"):
        ob.onboard(desc, net, objects, keys=keys, n_view=3, n_sample=600)
    with policy.use(strict="1", pem_vit_dtype="fp16"):
        policy.reset_library_branch_hits()
        half = ob.onboard(desc, net, objects, keys=keys, **kw)
        torch.cuda.synchronize()
        assert policy.library_branch_hits() == {}
    assert torch.equal(half.pem_templates["dense_po"], ref_po) and torch.isfinite(half.pem_templates["dense_fo"]).all()
