"""sam6d_amd.pem.verify without a GPU and without the emulator: its torch and plain statements against the plain-loop restatement
of tests/verify_ref.py on CPU tensors (EQUAL: the definition is integer work after two float32 operations), ``verify_poses`` on the
renders of the torch rasteriser, the argument checks that need no kernel, FramePipeline's `verifier` keyword on stand-in models,
and tools/verify_poses.py on a tiny synthetic dataset."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import render_ref as R
from tests import test_gpu_verify as T
from tests import verify_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = (24, 32)
CAM = (60.0, 60.0, 16.0, 12.0)
t = torch.from_numpy


def _words(x):
    return np.ascontiguousarray(x.numpy()).view(np.uint64)


def _same_evidence(got, ref):
    return (np.array_equal(got["counts"].numpy(), ref["counts"]) and np.array_equal(_words(got["inlier"]), ref["inlier"])
            and np.array_equal(got["span"].numpy(), ref["span"]) and got["counts"].dtype == torch.int32 and got["inlier"].dtype == torch.int64)


@pytest.mark.parametrize("with_masks", [False, True])
@pytest.mark.parametrize("hw", [(5, 7), (8, 8), (8, 16)])
def test_library_evidence_equals_the_restatement(hw, with_masks):
    from sam6d_amd.pem import verify
    render, obs, frame, _ = T.rect_scene(3, hw, 6, 2)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    obs[0, 0, :5] = [nan, inf, -5.0, 0.0, 415.0]                            # hostile pixels under instance 0 ...
    render[0, 0, :5] = 400.0
    render[1, 1, :4] = [nan, -3.0, inf, 400.0]                              # ... and hostile renders
    frame[:2] = 0
    masks = (render > 380).astype(np.uint8) * 255 if with_masks else None
    for unit, tau in ((1.0, 15.0), (1.0, 0.0), (0.5, 250.0)):
        ref = V.evidence(render, obs, frame, unit, tau, masks)
        got = verify._evidence_library(t(render), t(obs), t(frame), unit, tau, None if masks is None else t(masks))
        assert _same_evidence(got, ref), (got["counts"], ref["counts"])
        assert _same_evidence(verify.evidence(t(render), t(obs), t(frame), unit, tau, None if masks is None else t(masks)), ref)
    depth, r = T.contraction_probes()
    ren, ob = np.zeros((1,) + hw, np.float32), np.zeros((1,) + hw, np.float32)
    ren[0, 2, :5], ob[0, 2, :5] = r[:5], depth[:5]
    ref = V.evidence(ren, ob, frame[:1] * 0, 1000.0, 15.0)
    assert ref["counts"][0].tolist() == [5, 0, 5, 0, 0, 0, 0, 0]
    assert _same_evidence(verify._evidence_library(t(ren), t(ob), t(frame[:1] * 0), 1000.0, 15.0), ref)


def test_library_selection_equals_the_restatement():
    from sam6d_amd.pem import verify
    seen = set()
    for seed in range(6):
        for th in (T.DEFAULTS, (4, 0.8, 0.9), (0, 0.0, 0.0)):
            render, obs, frame, flagged = T.rect_scene(seed)
            ev = V.evidence(render, obs, frame, 1.0, 15.0)
            order, start = V.default_order(V.scores(ev["counts"], False)[0], ev["counts"], frame, len(obs))
            ref = V.select(ev["inlier"], ev["counts"], order, start, flagged, *th)
            lib = verify._evidence_library(t(render), t(obs), t(frame), 1.0, 15.0)
            got = verify.select(lib["inlier"], lib["counts"], lib["span"], t(order), t(start), t(flagged), *th)
            assert np.array_equal(got[0].numpy(), ref[0]) and np.array_equal(got[1].numpy(), ref[1]) and got[0].dtype == torch.int32
            seen |= set(ref[0].tolist())
            # the module's order is the restatement's
            sc = verify.scores(lib["counts"], False)
            o, s = verify.visiting_order(t(frame), len(obs), sc[0], lib["counts"][:, 2].long())
            assert np.array_equal(o.numpy(), order) and np.array_equal(s.numpy(), start) and o.dtype == torch.int32 and s.dtype == torch.int64
    assert seen == {0, 1, 2, 3, 4}


def _scene():
    """Two cubes and a torus-shaped impostor in two frames of HW, rendered by the torch rasteriser."""
    from sam6d_amd import evaluation
    v, f = R.cube(40.0)[:2]
    tv, tf = R.torus(12, 8, 30.0, 12.0)[:2]
    P = R.poses(6, seed=7, t=(0.0, 0.0, 400.0)).astype(np.float32)
    P[0, :3, 3] = (-53.0, -13.0, 400.0)
    P[1, :3, 3] = (53.0, 13.0, 400.0)
    P[2] = P[0]
    P[2, :3, 3] += np.array([14.0, -9.0, 4.0], np.float32)                  # a shifted duplicate
    P[3] = P[0]
    P[3, :3, 3] = (-33.0, -8.0, 250.0)                                     # floating in front
    P[4] = P[1]                                                            # the second cube again, as a torus
    P[5] = P[0]                                                            # the first cube, in the other frame
    obj, frame = [0, 0, 0, 0, 1, 0], np.array([0, 0, 0, 0, 0, 1], np.int32)
    cams = torch.tensor(CAM).expand(6, 4).contiguous()
    ren = np.zeros((6,) + HW, np.float32)
    for o, (mv, mf) in enumerate(((v, f), (tv, tf))):
        idx = [i for i in range(6) if obj[i] == o]
        ren[idx] = evaluation._render_depth_library(t(mv), t(mf), t(P[idx]), cams[:len(idx)], HW[0], HW[1], 1.0)["depth"].numpy()
    z = np.where(ren[:2] > 0, ren[:2], np.inf).min(0)
    obs = np.where(np.isfinite(z), z, 460.0).astype(np.float32)
    rs = np.random.RandomState(1)
    obs = np.stack([obs, obs + rs.uniform(-5, 5, HW).astype(np.float32)])
    return dict(meshes=[(v, f), (tv, tf)], P=P, obj=obj, frame=frame, render=ren, obs=obs)


def test_verify_poses_on_cpu_tensors_equals_the_restatement():
    from sam6d_amd import policy
    from sam6d_amd.pem import verify
    s = _scene()
    P, obs, frame = s["P"], s["obs"], s["frame"]
    masks = np.roll(s["render"] > 0, 1, axis=2)
    K = torch.tensor([[CAM[0], 0, CAM[2]], [0, CAM[1], CAM[3]], [0, 0, 1]], dtype=torch.float64)
    for m, key in ((None, None), (masks, None), (None, [0.5, 0.1, 0.9, 0.2, 0.3, 0.4])):
        ref = V.verify(s["render"], obs, frame, 1.0, 15.0, m, None, *T.DEFAULTS, order_by=key)
        out = verify.verify_poses(s["meshes"], s["obj"], t(P[:, :3, :3].copy()), t(P[:, :3, 3].copy()), t(obs), K,
                                  masks=None if m is None else t(m), frame_index=frame, order_by=key)
        assert T._same_result(out, ref), (out["status"], ref["status"])
    assert not policy.library_branch_hits()                                 # CPU tensors: the library doing its job is not recorded
    ref = V.verify(s["render"], obs, frame, 1.0, 15.0, None, None, *T.DEFAULTS)
    assert ref["status"].tolist() == [0, 0, 3, 1, 3, 0] and ref["fit"][3] == 0.0 and ref["fresh"][5] == ref["counts"][5, 2]
    # a caller's render, flagged by its skipped count
    skipped = torch.tensor([0, 1, 0, 0, 0, 0], dtype=torch.int32)
    out = verify.verify_poses(s["meshes"], s["obj"], t(P[:, :3, :3].copy()), t(P[:, :3, 3].copy()), t(obs), K, frame_index=frame,
                              render=dict(depth=t(s["render"]), skipped=skipped))
    assert out["status"].tolist() == [0, 4, 3, 1, 0, 0]                     # the torus now finds the second cube's pixels free
    verifier = verify.PoseVerifier([verify.device_mesh(*m) for m in s["meshes"]], min_inliers=10 ** 6)
    assert verifier(s["obj"], t(P[:, :3, :3].copy()), t(P[:, :3, 3].copy()), t(obs), K, frame_index=frame)["status"].tolist() == [1] * 6
    assert verify.DEFAULT_TAU == 15.0 and (verify.DEFAULT_MIN_INLIERS, verify.DEFAULT_MIN_FIT, verify.DEFAULT_MIN_FRESH) == T.DEFAULTS
    assert sorted(verify.STATUS) == [0, 1, 2, 3, 4] and verify.COUNTS == V.NAMES


def test_ops_refuse_without_a_kernel():
    from sam6d_amd import _lib, ops
    from sam6d_amd.pem import verify
    z = torch.zeros
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.verify_evidence(z(1, 4, 4), z(1, 4, 4), z(1, dtype=torch.int32), 1.0, 15.0)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.verify_select(z(1, 1, dtype=torch.int64), z(1, 8, dtype=torch.int32), z(1, 2, dtype=torch.int32), z(1, dtype=torch.int32),
                          z(2, dtype=torch.int64), None, 12, 0.5, 0.5)
    L = _lib.lib()
    assert _lib.header_constant("S6D_VERIFY_LDS_WORDS") == 4800 == 480 * 640 // 64
    assert L.s6d_verify_select_workspace_bytes(8, 480, 640) == 0 and L.s6d_verify_select_workspace_bytes(8, 1080, 1920) == 8 * 32400 * 8
    assert L.s6d_verify_select_workspace_bytes(1, 1 << 15, 1 << 14) == -1
    mesh = verify.device_mesh(*R.cube()[:2])
    Rm, tv, d = torch.eye(3)[None].contiguous(), z(1, 3), z(4, 4)
    with pytest.raises(ValueError, match="frame_index"):
        verify.verify_poses([mesh], [0], Rm, tv, d, CAM, frame_index=[1])
    with pytest.raises(ValueError, match="object_index"):
        verify.verify_poses([mesh], [1], Rm, tv, d, CAM)
    with pytest.raises(TypeError, match="float32"):
        verify.verify_poses([mesh], [0], Rm, tv.double(), d, CAM)
    with pytest.raises(ValueError, match="depth_unit"):
        verify.verify_poses([mesh], [0], Rm, tv, d, CAM, depth_unit=float("inf"))
    with pytest.raises(ValueError, match="must be >= 0"):
        verify.verify_poses([mesh], [0], Rm, tv, d, CAM, min_fresh=-0.1)


# ---------------------------------------------------------------------------------------------------------------- FramePipeline
def _pipeline(monkeypatch, verifier, refiner=None):
    """``tests.test_host_refine._pipeline`` with the `verifier` keyword added to what it constructs."""
    from sam6d_amd import pipeline
    from tests import test_host_refine as TR
    orig = pipeline.FramePipeline

    class WithVerifier(orig):
        def __init__(self, *a, **k):
            super().__init__(*a, **k, **({} if verifier is None else dict(verifier=verifier)))
    monkeypatch.setattr(pipeline, "FramePipeline", WithVerifier)
    try:
        return TR._pipeline(monkeypatch, refiner)
    finally:
        monkeypatch.setattr(pipeline, "FramePipeline", orig)


def test_pipeline_without_a_verifier_calls_nothing_of_the_module(monkeypatch):
    from sam6d_amd.pem import verify

    def boom(*a, **k):
        raise AssertionError("pem/verify.py ran although verifier=None")
    for name in ("verify_poses", "evidence", "select", "_evidence_library", "_select_library", "scores", "visiting_order", "PoseVerifier"):
        monkeypatch.setattr(verify, name, boom)
    det, poses, pipe, _, _ = _pipeline(monkeypatch, None)
    assert pipe.verifier is None and sorted(poses) == ["kept", "pred_R", "pred_pose_score", "pred_t"] and "pem_verify" not in pipe.times


def test_pipeline_with_a_verifier_judges_and_drops_nothing(monkeypatch):
    seen = {}

    class Verifier:
        use_masks = True

        def __call__(self, object_index, R, t, depth, K, masks=None):
            seen.update(object_index=list(object_index), R=R.clone(), t=t.clone(), depth=depth, K=K, masks=masks)
            n = R.shape[0]
            return dict(keep=torch.arange(n) % 2 == 0, status=torch.arange(n, dtype=torch.int32) % 2 * 3,
                        score=torch.linspace(1.0, 0.5, n, dtype=torch.float64))

    class Refiner:
        use_masks = False

        def __call__(self, object_index, R, t, depth, K, masks=None):
            n = R.shape[0]
            return dict(R=R, t=t + 0.5, status=torch.zeros(n, dtype=torch.int32), rms=torch.zeros(n, dtype=torch.float64))
    plain = _pipeline(monkeypatch, None)[1]
    det, poses, pipe, depth, K = _pipeline(monkeypatch, Verifier())
    assert sorted(poses) == ["kept", "pred_R", "pred_pose_score", "pred_t", "verify_keep", "verify_score", "verify_status"]
    assert all(torch.equal(poses[k], plain[k]) for k in plain)              # no row dropped, nothing else touched
    assert poses["verify_keep"].tolist() == [True, False, True] and poses["verify_status"].tolist() == [0, 3, 0]
    assert poses["verify_score"].tolist() == [1.0, 0.75, 0.5] and poses["verify_score"].dtype == torch.float64
    assert seen["object_index"] == [0, 0, 0] and torch.equal(seen["t"], plain["pred_t"]) and seen["depth"] is depth and seen["K"] is K
    assert torch.equal(seen["masks"], det.masks[poses["kept"]]) and "pem_verify" in pipe.times and "pem_refine" not in pipe.times
    # after a refiner the verifier sees the refined pose
    det, poses, pipe, _, _ = _pipeline(monkeypatch, Verifier(), Refiner())
    assert torch.equal(seen["t"], plain["pred_t"] + 0.5) and torch.equal(poses["pred_t"], plain["pred_t"] + 0.5)
    assert "pem_verify" in pipe.times and "pem_refine" in pipe.times and "verify_keep" in poses and "refine_status" in poses
    Verifier.use_masks = False
    _pipeline(monkeypatch, Verifier())
    assert seen["masks"] is None


# ---------------------------------------------------------------------------------------------------------------- the tool
SCENE, IMS = 3, (4, 9)


def _write_dataset(root):
    """The scene of ``_scene`` as a BOP dataset (PLY models, scene_gt.json, scene_camera.json, 16-bit depth PNGs with depth_scale
    0.1) and a result file: five estimates in image 4, one in image 9, one in an image the dataset does not have."""
    from PIL import Image

    from sam6d_amd.pem import results
    from tests.test_host_bop_gt import _write_ply
    s = _scene()
    scene = root / "test" / f"{SCENE:06d}"
    (root / "models_eval").mkdir(parents=True)
    (scene / "depth").mkdir(parents=True)
    for obj, (v, f) in zip((1, 2), s["meshes"]):
        _write_ply(root / "models_eval" / f"obj_{obj:06d}.ply", v, f)
    fx, fy, cx, cy = CAM
    (scene / "scene_gt.json").write_text(json.dumps({str(im): [] for im in IMS}))
    (scene / "scene_camera.json").write_text(json.dumps({str(im): {"cam_K": [fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0], "depth_scale": 0.1}
                                                         for im in IMS}))
    for i, im in enumerate(IMS):
        Image.fromarray(np.rint(s["obs"][i] * 10).astype(np.uint16)).save(scene / "depth" / f"{im:06d}.png")
    lines, P = [], s["P"]
    for n in range(6):
        lines += results.bop_csv_lines(SCENE, IMS[s["frame"][n]], [s["obj"][n] + 1], np.array([0.1 * (n + 1)], np.float32), P[n:n + 1, :3, :3],
                                       P[n:n + 1, :3, 3] / np.float32(1000), 0.25)
    lines += results.bop_csv_lines(SCENE, 77, [1], np.array([0.9], np.float32), P[:1, :3, :3], P[:1, :3, 3] / np.float32(1000), 0.25)
    results.write_bop_csv(str(root / "in.csv"), lines)
    return s


def test_verify_poses_tool(tmp_path, capsys):
    from sam6d_amd import evaluation
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import verify_poses as tool
    root = tmp_path / "ds"
    s = _write_dataset(root)
    src, dst = str(root / "in.csv"), str(tmp_path / "out.csv")
    base = ["--results", src, "--dataset", str(root), "--device", "cpu"]
    given = evaluation.read_bop_csv(src)
    # what the tool must find: the restatement on the renders of the poses and the depth AS THE FILES GIVE THEM BACK
    obs = np.rint(s["obs"] * 10).astype(np.uint16).astype(np.float32) * np.float32(0.1)
    cams = torch.tensor(CAM).expand(6, 4).contiguous()
    P = np.tile(np.eye(4, dtype=np.float32), (6, 1, 1))
    P[:, :3, :3], P[:, :3, 3] = given["R"][:6], given["t"][:6]
    ren = np.zeros((6,) + HW, np.float32)
    for o, (mv, mf) in enumerate(s["meshes"]):
        idx = [i for i in range(6) if s["obj"][i] == o]
        ren[idx] = evaluation._render_depth_library(t(mv), t(mf), t(P[idx]), cams[:len(idx)], HW[0], HW[1], 1.0)["depth"].numpy()
    ref = V.verify(ren, obs, s["frame"], 1.0, 15.0, None, None, *T.DEFAULTS)
    assert ref["status"].tolist() == [0, 0, 3, 1, 3, 0]
    summary = tool.main(base + ["--out", dst])
    assert summary["status"] == {"kept": 3, "too few inliers": 1, "seen through": 0, "explained already": 2, "not verifiable": 0,
                                 "image not in the dataset": 1}
    assert summary["estimates"] == 7 and summary["written"] == 4 and json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == summary
    got = evaluation.read_bop_csv(dst)
    keep = [0, 1, 5, 6]                                                     # the kept lines, and the one nobody could judge
    assert got["im"].tolist() == given["im"][keep].tolist() and got["obj"].tolist() == given["obj"][keep].tolist()
    assert np.array_equal(got["R"], given["R"][keep]) and np.allclose(got["t"], given["t"][keep], rtol=1e-6, atol=0)
    assert np.array_equal(got["score"][:3], ref["score"][[0, 1, 5]].astype(np.float32)) and got["score"][3] == given["score"][6]
    assert np.array_equal(got["time"], given["time"][keep])
    # never over an existing file without --force
    before = open(dst).read()
    with pytest.raises(SystemExit, match="exists"):
        tool.main(base + ["--out", dst, "--keep-all"])
    assert open(dst).read() == before
    summary = tool.main(base + ["--out", dst, "--keep-all", "--force"])
    got = evaluation.read_bop_csv(dst)
    assert summary["written"] == 7 and got["im"].tolist() == given["im"].tolist()
    assert np.array_equal(got["score"][:6], ref["score"].astype(np.float32)) and got["score"][6] == given["score"][6]
    tool.main(base + ["--out", dst, "--score", "keep", "--force"])
    got = evaluation.read_bop_csv(dst)
    assert np.array_equal(got["score"], given["score"][keep]) and got["im"].tolist() == given["im"][keep].tolist()
