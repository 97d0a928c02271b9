"""sam6d_amd/pem/refine.py on a host without a device: the library statements against the restatement (tests/refine_ref.py) on a
render of the numpy rasteriser, the argument checks that need no kernel, and FramePipeline's `refiner` keyword on stand-in models
(the pattern of tests/test_host_pipeline_glue.py)."""
import numpy as np
import pytest
import torch

from tests import refine_ref as RR
from tests import render_ref as R

HW, CAM = (37, 53), (60.0, 60.0, 26.0, 18.0)
MAX_DIST, MIN_COS = 12.0, 0.3


def _scene():
    """The cube near one pose at T = 2 poses (xyz / face of the numpy rasteriser, rounded to float32) and M = 2 observed frames."""
    v, f, c = R.cube()
    P = R.poses(1, seed=7).repeat(2, 0)
    P[1, :3, 3] += (0.5, 0.0, 2.0)
    ren = R.render(v, f, c, P, CAM, HW[0], HW[1], 1.0, 0.0, 1.0)
    P2 = P.copy()
    P2[:, :3, 3] += ((1.5, -1.0, 4.0), (1.0, 0.5, -7.0))
    obs = R.render(v, f, c, P2, CAM, HW[0], HW[1], 1.0, 0.0, 1.0)["depth"].astype(np.float32)
    obs[:, 20:24, 24:30], obs[:, 10:12, 20:26], obs[:, 16, 22:25] = 300.0, 0.0, np.nan
    mask = np.random.RandomState(0).choice(np.array([0, 1, 255], np.uint8), size=(2,) + HW, p=[0.2, 0.4, 0.4])
    return dict(v=v, f=f, P=P, xyz=ren["xyz"].astype(np.float32), face=ren["face"], obs=obs, oi=np.array([1, 0], np.int32), mask=mask)


def test_library_normal_equations_within_the_derived_bound():
    """_normal_eq_library sums in torch's order: the count is the restatement's, every sum within n 2^-52 sum |term| of it."""
    from sam6d_amd import ops
    from sam6d_amd.pem import refine
    s = _scene()
    ref = RR.normal_eq(s["xyz"], s["face"], s["obs"], s["oi"], s["mask"], s["v"], s["f"], s["P"], CAM, 1.0, MAX_DIST, MIN_COS, ops.RF_CHUNK)
    for k in ("face", "mask", "depth", "grazing", "distance"):
        assert ref["tally"][k][0] > 0 and ref["tally"][k][1] > 0, (k, ref["tally"])
    assert (ref["count"] > 50).all()
    t = torch.from_numpy
    sums, count = refine.normal_eq(t(s["xyz"]), t(s["face"]), t(s["obs"]), t(s["oi"]), t(s["mask"]), t(s["v"]), t(s["f"]), t(s["P"]), *CAM, 1.0,
                                   MAX_DIST, MIN_COS)
    assert sums.dtype == torch.float64 and count.dtype == torch.int32
    assert np.array_equal(count.numpy(), ref["count"])
    err = np.abs(sums.numpy() - ref["sums"])
    assert (err <= RR.bound(ref)).all(), (err / RR.bound(ref)).max()
    # an obs_index outside [0, M): zeros, as in the kernel
    sums, count = refine.normal_eq(t(s["xyz"]), t(s["face"]), t(s["obs"]), t(np.array([2, -1], np.int32)), None, t(s["v"]), t(s["f"]), t(s["P"]),
                                   *CAM, 1.0, MAX_DIST, MIN_COS)
    assert count.tolist() == [0, 0] and not bool(sums.any())
    # the library update: the restatement's operations in its order, each correctly rounded -> the same bits
    got = refine.update(t(ref["sums"]), t(ref["count"]), t(s["P"]), 12, 1e-6, 1e-9)
    want = RR.update(ref["sums"], ref["count"], s["P"], 12, 1e-6, 1e-9)
    assert got[1].tolist() == [0, 0] == want[1].tolist()
    assert np.array_equal(got[0].numpy().view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[2].numpy(), want[2])
    bad = ref["sums"].copy()
    bad[0, 3] = np.nan
    got = refine.update(t(bad), t(np.array([100, 3], np.int32)), t(s["P"]), 12, 1e-6, 1e-9)
    assert got[1].tolist() == [3, 1] and np.array_equal(got[0].numpy().view(np.uint32), s["P"].view(np.uint32)) and got[2][0] == 0
    one = np.zeros((1, 28))
    J = np.array([37.25, -411.5, 93.125, 0.36, -0.48, 0.8])
    one[0, :21], one[0, 21:27], one[0, 27] = [J[i] * J[j] for i in range(6) for j in range(i, 6)], J * 1.75, 1.75 * 1.75
    assert refine.update(t(one), t(np.array([100], np.int32)), t(s["P"][:1]), 12, 0.0, 1e-9)[1].tolist() == [2]
    assert refine.update(t(one), t(np.array([100], np.int32)), t(s["P"][:1]), 12, 1e-3, 1e-9)[1].tolist() == [0]


def test_ops_and_refine_poses_refuse_without_a_kernel():
    from sam6d_amd import _lib, ops
    from sam6d_amd.pem import refine
    assert ops.RF_CHUNK == _lib.header_constant("S6D_RF_CHUNK") and ops.RF_CHUNK % 256 == 0
    z = torch.zeros
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.refine_normal_eq(z(1, 4, 4, 3), z(1, 4, 4, dtype=torch.int32), z(1, 4, 4), z(1, dtype=torch.int32), None, z(3, 3),
                             z(1, 3, dtype=torch.int32), z(1, 4, 4), 1.0, 1.0, 0.0, 0.0, 1.0, 5.0, 0.1)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.refine_update(z(1, 28, dtype=torch.float64), z(1, dtype=torch.int32), z(1, 4, 4), 12, 1e-6, 1e-9)
    L = _lib.lib()
    assert L.s6d_refine_workspace_bytes(2, 480, 640) == 2 * 300 * 28 * 8 + 2 * 300 * 4 and L.s6d_refine_workspace_bytes(1, 0, 5) == -1
    mesh = refine.device_mesh(*R.cube()[:2])
    Rm, tv, d = torch.eye(3)[None].contiguous(), z(1, 3), z(4, 4)
    with pytest.raises(ValueError, match="schedule"):
        refine.refine_poses([mesh], [0], Rm, tv, d, CAM, max_dist=[1.0] * 33)
    with pytest.raises(ValueError, match="frame_index"):
        refine.refine_poses([mesh], [0], Rm, tv, d, CAM, frame_index=[1])
    with pytest.raises(ValueError, match="object_index"):
        refine.refine_poses([mesh], [1], Rm, tv, d, CAM)
    with pytest.raises(TypeError, match="float32"):
        refine.refine_poses([mesh], [0], Rm, tv.double(), d, CAM)
    with pytest.raises(ValueError, match="depth_unit"):
        refine.refine_poses([mesh], [0], Rm, tv, d, CAM, depth_unit=0.0)
    assert refine._camera(torch.tensor([[5.0, 0, 2.0], [0, 6.0, 3.0], [0, 0, 1]], dtype=torch.float64)) == (5.0, 6.0, 2.0, 3.0)
    assert len(refine.DEFAULT_SCHEDULE) == 6 and refine.MAX_ITERATIONS == 32


# ---------------------------------------------------------------------------------------------------------------- FramePipeline
def _pipeline(monkeypatch, refiner):
    """The stand-in models of tests/test_host_pipeline_glue.py, reduced to what the PEM stage needs -> (det, poses, pipe)."""
    from sam6d_amd import pipeline
    H, W, S = 120, 160, 256
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    depth = 0.8 + 0.05 * torch.rand(H, W, generator=g)
    K = torch.tensor([[143.0, 0, 80.0], [0, 143.0, 60.0], [0, 0, 1]], dtype=torch.float64)
    monkeypatch.setattr(pipeline, "sam_preprocess", lambda x, img_size: torch.zeros(x.shape[0], 3, img_size, img_size))
    monkeypatch.setattr(pipeline.FramePipeline, "_tick", lambda self, name, t0: self.times.__setitem__(name, 0.0) or t0)
    boxes = torch.tensor([[20, 10, 90, 70], [60, 30, 150, 110], [5, 50, 70, 115], [80, 5, 155, 60]])
    masks = torch.zeros(4, H, W, dtype=torch.bool)
    for i, (x1, y1, x2, y2) in enumerate(boxes.tolist()):
        masks[i, y1:y2 + 1, x1:x2 + 1] = True
    monkeypatch.setattr(pipeline.amg, "generate_proposals", lambda *a, **k: dict(masks=masks, boxes=boxes))

    class Enc:
        img_size = S

        def __call__(self, x):
            return torch.zeros(x.shape[0], 8, S // 16, S // 16)

    class Desc:
        proposal_size = 56

        def __call__(self, image, prop):
            n = prop.masks.shape[0]
            return torch.zeros(n, 4), torch.zeros(n, 16, 4)

    class Scorer:
        def score(self, cls, patch, m, b, d, k, depth_scale=1.0):
            n = m.shape[0]
            return dict(final=torch.linspace(0.2, 0.9, n), sel=torch.arange(n), pred_obj=torch.zeros(n, dtype=torch.long))

    class Pem:
        def __call__(self, ep):
            M = ep["pts"].shape[0]
            return dict(pred_R=torch.eye(3).expand(M, 3, 3).clone(), pred_t=torch.arange(3.0 * M).reshape(M, 3),
                        pred_pose_score=torch.full((M,), 0.5))
    tpl = dict(model=torch.zeros(1, 64, 3), dense_po=torch.zeros(1, 32, 3), dense_fo=torch.zeros(1, 32, 8))
    kw = {} if refiner is None else dict(refiner=refiner)
    pipe = pipeline.FramePipeline(Enc(), None, None, Desc(), Scorer(), Pem(), tpl, object_radius=10.0, top_k=3, points_per_batch=16, **kw)
    det, poses = pipe(img, depth, K, torch.rand(3, H * W, generator=g), torch.rand(3, 18000, generator=g))
    return det, poses, pipe, depth, K


def test_pipeline_without_a_refiner_calls_nothing_of_the_module(monkeypatch):
    from sam6d_amd.pem import refine

    def boom(*a, **k):
        raise AssertionError("pem/refine.py ran although refiner=None")
    for name in ("refine_poses", "normal_eq", "update", "_normal_eq_library", "_update_library", "device_mesh", "DepthRefiner"):
        monkeypatch.setattr(refine, name, boom)
    det, poses, pipe, _, _ = _pipeline(monkeypatch, None)
    assert pipe.refiner is None and sorted(poses) == ["kept", "pred_R", "pred_pose_score", "pred_t"] and "pem_refine" not in pipe.times


def test_pipeline_with_a_refiner_returns_both_poses(monkeypatch):
    seen = {}

    class Refiner:
        use_masks = True

        def __call__(self, object_index, R, t, depth, K, masks=None):
            seen.update(object_index=list(object_index), R=R.clone(), t=t.clone(), depth=depth, K=K, masks=masks)
            n = R.shape[0]
            return dict(R=R.flip(1), t=t + 0.5, status=torch.arange(n, dtype=torch.int32) % 4, rms=torch.full((n,), 2.0, dtype=torch.float64),
                        count=torch.zeros(n, dtype=torch.int32), skipped=torch.zeros(n, dtype=torch.int32))
    det0, plain, _, _, _ = _pipeline(monkeypatch, None)
    det, poses, pipe, depth, K = _pipeline(monkeypatch, Refiner())
    assert sorted(poses) == ["kept", "pred_R", "pred_R_pem", "pred_pose_score", "pred_t", "pred_t_pem", "refine_rms", "refine_status"]
    assert torch.equal(poses["pred_R_pem"], plain["pred_R"]) and torch.equal(poses["pred_t_pem"], plain["pred_t"])
    assert torch.equal(poses["pred_t"], plain["pred_t"] + 0.5) and torch.equal(poses["pred_R"], plain["pred_R"].flip(1))
    assert poses["refine_status"].tolist() == [0, 1, 2] and poses["refine_rms"].tolist() == [2.0] * 3
    assert torch.equal(poses["pred_pose_score"], plain["pred_pose_score"]) and torch.equal(poses["kept"], plain["kept"])
    assert seen["object_index"] == [0, 0, 0] and torch.equal(seen["t"], plain["pred_t"]) and seen["depth"] is depth and seen["K"] is K
    assert torch.equal(seen["masks"], det.masks[poses["kept"]]) and "pem_refine" in pipe.times and "pem" in pipe.times
    Refiner.use_masks = False
    _pipeline(monkeypatch, Refiner())
    assert seen["masks"] is None
