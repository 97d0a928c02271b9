"""sam6d_amd.evaluation on the host: the symmetry transforms, the greedy matcher against the plain-Python one of tests/bop_ref.py,
the BOP19 scores and the command-line scorer on CPU tensors (the torch statements of the module: no kernel runs here), and the
result-file round trip.  bop_toolkit is not present; nothing is compared with it."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from sam6d_amd import evaluation as ev
from sam6d_amd.pem import results
from tests import bop_ref as B
from tests import render_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 48, 64
CAM = np.array([60.0, 60.0, 32.0, 24.0], np.float32)


# ---------------------------------------------------------------------------------------------------------------- symmetries
def test_symmetry_transforms_identity_only():
    for info in ({}, {"diameter": 10.0}, {"symmetries_discrete": [], "symmetries_continuous": []}):
        s = ev.symmetry_transforms(info)
        assert s.dtype == np.float64 and s.shape == (1, 4, 4) and np.array_equal(s[0], np.eye(4))


def test_symmetry_transforms_one_discrete():
    flip = np.diag([-1.0, -1.0, 1.0, 1.0])
    flip[:3, 3] = (2.0, 0.0, 0.0)
    s = ev.symmetry_transforms({"symmetries_discrete": [flip.reshape(-1).tolist()]})
    assert s.shape == (2, 4, 4) and np.array_equal(s[0], np.eye(4)) and np.array_equal(s[1], flip)


def test_symmetry_transforms_continuous_axis_with_offset():
    axis, off = np.array([0.0, 0.6, 0.8]), np.array([5.0, -2.0, 7.0])
    s = ev.symmetry_transforms({"symmetries_continuous": [{"axis": axis.tolist(), "offset": off.tolist()}]})
    assert s.shape == (315, 4, 4) and np.array_equal(s[0], np.eye(4))          # ceil(pi / 0.01)
    line = off[None] + np.linspace(-50, 50, 7)[:, None] * axis[None]
    for k in range(315):
        Rk, tk = s[k, :3, :3], s[k, :3, 3]
        assert np.allclose(Rk @ Rk.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(Rk) - 1) < 1e-12
        assert np.allclose(line @ Rk.T + tk, line, atol=1e-9)              # the axis line maps to itself, point by point
        assert np.allclose(Rk, B.rotation(axis, 2 * np.pi * k / 315), atol=1e-12)
    assert ev.symmetry_transforms({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}, max_sym_disc_step=0.1).shape[0] == 32


def test_symmetry_transforms_discrete_times_continuous():
    flip = np.diag([1.0, -1.0, -1.0, 1.0])
    flip[:3, 3] = (0.0, 0.0, 4.0)
    info = {"symmetries_discrete": [flip.reshape(-1).tolist()], "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 2]}]}
    s = ev.symmetry_transforms(info)
    cont = ev.symmetry_transforms({"symmetries_continuous": info["symmetries_continuous"]})
    assert s.shape == (630, 4, 4) and np.array_equal(s[0], np.eye(4))
    assert np.array_equal(s[:315], cont)
    assert np.allclose(s[315:], cont @ flip, atol=1e-12)                   # R = Rc Rd, t = Rc td + tc


# ---------------------------------------------------------------------------------------------------------------- the matcher
@pytest.mark.parametrize("seed", range(6))
def test_matcher_equals_the_plain_python_one(seed):
    rs = np.random.RandomState(seed)
    groups, E, G = 5, 40, 14
    est_group, gt_group = rs.randint(0, groups, E), np.concatenate([np.arange(groups), rs.randint(0, groups, G - groups)])
    n_targets = np.bincount(gt_group, minlength=groups)
    scores = np.round(rs.uniform(0, 1, E), 1)                              # ties among the scores
    errors = np.round(rs.uniform(0, 1, (E, G)), 1)                         # and among the errors, and errors equal to a threshold
    th = [0.1, 0.3, 0.5, 0.9, 2.0]
    want = B.match_and_recall(errors, scores, est_group, gt_group, n_targets, th)
    got = ev.match_and_recall(errors, scores, est_group, gt_group, n_targets, th)
    assert got.tolist() == want and 0 < want[1] < want[-1] <= 1
    pe, pg = np.nonzero(est_group[:, None] == gt_group[None, :])
    perm = rs.permutation(len(pe))
    assert ev.match_and_recall((pe[perm], pg[perm], errors[pe, pg][perm]), scores, est_group, gt_group, n_targets, th).tolist() == want


def test_matcher_keeps_the_best_scored_and_matches_one_to_one():
    # one group, two targets, three estimates: the lowest-scored one is dropped although it is the only correct one for g1
    errors = np.array([[0.1, 0.9], [0.2, 0.9], [0.9, 0.1]])
    assert ev.match_and_recall(errors, [0.9, 0.8, 0.7], [0, 0, 0], [0, 0], [2], [0.5]).tolist() == [0.5]
    assert ev.match_and_recall(errors, [0.9, 0.6, 0.7], [0, 0, 0], [0, 0], [2], [0.5]).tolist() == [1.0]
    assert ev.match_and_recall(errors, [0.9, 0.8, 0.7], [0, 0, 0], [0, 0], [2], [0.5, 0.05]).tolist() == [0.5, 0.0]


# ---------------------------------------------------------------------------------------------------------------- scores
def _scene(n_images=2):
    """Two objects (a cube with its discrete symmetries left out, and a smaller cube) in n_images images of 48 x 64, the measured
    depth = the library render of the ground truth in front of a wall."""
    v1, f1, _ = R.cube(40.0)
    v2, f2, _ = R.cube(25.0)
    models = {1: dict(vertices=v1, faces=f1, diameter=80.0 * np.sqrt(3.0), symmetries=np.eye(4)[None]),
              5: dict(vertices=v2, faces=f2, diameter=50.0 * np.sqrt(3.0), info={"diameter": 50.0 * np.sqrt(3.0)})}
    gt = dict(im=[], obj=[], pose=[])
    depth = np.full((n_images, H, W), 700.0, np.float32)
    for im in range(n_images):
        for obj, t in ((1, (-90.0, -20.0, 400.0)), (5, (70.0, 30.0, 420.0 + 10 * im))):
            P = R.poses(1, seed=10 * im + obj, t=t)[0].astype(np.float64)
            gt["im"].append(im)
            gt["obj"].append(obj)
            gt["pose"].append(P)
            m = models[obj]
            d = ev._render_depth_library(torch.from_numpy(m["vertices"]), torch.from_numpy(m["faces"]), torch.from_numpy(P[None].astype(np.float32)),
                                         torch.from_numpy(CAM[None]), H, W, 1.0)
            assert int(d["skipped"].sum()) == 0 and int((d["depth"] > 0).sum()) > 40
            depth[im] = np.where(d["depth"][0].numpy() > 0, d["depth"][0].numpy(), depth[im])
    gt = {k: np.asarray(x) for k, x in gt.items()}
    images = dict(cams=np.tile(CAM, (n_images, 1)), depth=depth)
    return models, gt, images


def _noisy(gt, level, seed=0):
    rs = np.random.RandomState(seed)
    pose = gt["pose"].copy()
    for i in range(len(pose)):
        pose[i, :3, :3] = pose[i, :3, :3] @ B.rotation(rs.standard_normal(3), 0.01 * level)
        d = rs.standard_normal(3)
        pose[i, :3, 3] += level * d / np.linalg.norm(d)
    return dict(im=gt["im"], obj=gt["obj"], score=np.linspace(0.9, 0.5, len(pose)), pose=pose)


def test_bop19_scores_one_for_the_ground_truth_and_falling_with_noise():
    models, gt, images = _scene()
    out = [ev.bop19_scores(models, _noisy(gt, level), gt, images, device="cpu") for level in (0.0, 2.0, 8.0, 30.0, 120.0)]
    assert out[0]["AR"] == 1.0 and out[0]["AR_VSD"] == out[0]["AR_MSSD"] == out[0]["AR_MSPD"] == 1.0 and out[0]["unrenderable"] == 0
    assert out[0]["targets"] == 4 and np.array(out[0]["recalls_VSD"]).shape == (10, 10) and len(out[0]["recalls_MSPD"]) == 10
    for key in ("AR", "AR_VSD", "AR_MSSD", "AR_MSPD"):
        vals = [o[key] for o in out]
        assert all(a >= b for a, b in zip(vals, vals[1:])), (key, vals)
        assert vals[-1] < 0.2 < vals[1], (key, vals)
    assert all(abs(o["AR"] - (o["AR_VSD"] + o["AR_MSSD"] + o["AR_MSPD"]) / 3) < 1e-12 for o in out)
    # an estimate of an object without a target is not counted; of two estimates for one target only the higher-scored is kept
    base = _noisy(gt, 0.0)
    for score, want in ((0.1, 1.0), (1.0, 0.75)):
        extra = dict(im=np.append(base["im"], [0, 0]), obj=np.append(base["obj"], [9, 1]), score=np.append(base["score"], [1.0, score]),
                     pose=np.concatenate([base["pose"], _noisy(gt, 120.0)["pose"][:2]]))
        assert ev.bop19_scores(models, extra, gt, images, device="cpu")["AR"] == want


def test_library_errors_agree_with_the_restatement():
    """The torch statements of MSSD / MSPD (chunked over 315 symmetries) and of the VSD counts on CPU tensors against the float64
    restatement, within the bounds of profiles/bop_eval_margins.md."""
    rs = np.random.RandomState(3)
    v = rs.uniform(-60, 60, (257, 3)).astype(np.float32)
    gt = B.seeded_poses(4, seed=5)
    est = gt.copy()
    est[:, :3, 3] += (3.0, -2.0, 5.0)
    syms = ev.symmetry_transforms({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]})
    cams = np.tile(np.array([572.4, 573.6, 325.3, 242.0], np.float32), (4, 1))
    m3 = ev.mssd(torch.from_numpy(v), torch.from_numpy(est.astype(np.float32)), gt, syms).numpy()
    m2 = ev.mspd(torch.from_numpy(v), torch.from_numpy(est.astype(np.float32)), gt, syms, cams).numpy()
    r64 = B.pose_errors(v, est.astype(np.float32), (gt[:, None] @ syms[None]).astype(np.float32), cams, np.float64)
    assert (np.abs(m3 - r64["mssd"]) <= B.mssd_bound(r64)).all() and (np.abs(m2 - r64["mspd"]) <= B.mspd_bound(r64)).all()
    models, g, images = _scene(1)
    e = _noisy(g, 6.0)
    m = models[1]
    r = ev.vsd(torch.from_numpy(m["vertices"]), m["faces"], torch.from_numpy(e["pose"][:1].astype(np.float32)), g["pose"][:1], CAM[None], images["depth"],
               [0], m["diameter"])
    de = ev._render_depth_library(torch.from_numpy(m["vertices"]), torch.from_numpy(m["faces"]), torch.from_numpy(e["pose"][:1].astype(np.float32)),
                                  torch.from_numpy(CAM[None]), H, W, 1.0)["depth"].numpy()
    dg = ev._render_depth_library(torch.from_numpy(m["vertices"]), torch.from_numpy(m["faces"]), torch.from_numpy(g["pose"][:1].astype(np.float32)),
                                  torch.from_numpy(CAM[None]), H, W, 1.0)["depth"].numpy()
    ref = R.render(m["vertices"], m["faces"], np.zeros((8, 3), np.uint8), g["pose"][:1].astype(np.float32), CAM, H, W, 0.3, 0.7, 1.0)
    assert np.array_equal(dg > 0, ref["mask"] == 255) and (np.abs(dg - ref["depth"])[dg > 0] <= 8 * B.U * ref["depth"][dg > 0]).all()
    taus = [np.float32(t) for t in ev.BOP19["vsd_taus"]]
    r64 = B.vsd_counts(de, dg, images["depth"], [0], CAM[None], 15.0, taus, [m["diameter"]], np.float64)
    assert r64["undecided"][0] == 0 and r64["union"][0] > 40
    assert all(np.array_equal(r[k], r64[k]) for k in ("union", "inter", "ge")) and np.array_equal(r["errors"], B.vsd_errors(r64))
    assert 0 < r["errors"][0, 0] and r["errors"][0, -1] < 1


# ---------------------------------------------------------------------------------------------------------------- result files
def _csv(path, gt, scene_of, im_of, level):
    est = _noisy(gt, level)
    lines = []
    for i in range(len(est["pose"])):
        lines += results.bop_csv_lines(scene_of[est["im"][i]], im_of[est["im"][i]], [est["obj"][i]], np.float32([est["score"][i]]),
                                       est["pose"][i:i + 1, :3, :3], est["pose"][i:i + 1, :3, 3] / 1000.0, 0.25)
    results.write_bop_csv(path, lines)
    return est


def test_read_bop_csv_round_trips(tmp_path):
    _, gt, _ = _scene()
    est = _csv(tmp_path / "r.csv", gt, [48, 48], [3, 11], 2.0)
    back = ev.read_bop_csv(tmp_path / "r.csv")
    assert back["scene"].tolist() == [48] * 4 and back["im"].tolist() == [3, 3, 11, 11] and back["obj"].tolist() == [1, 5, 1, 5]
    assert np.array_equal(back["score"], est["score"].astype(np.float32)) and (back["time"] == 0.25).all()
    assert np.array_equal(back["R"], est["pose"][:, :3, :3].astype(np.float32))
    assert np.array_equal(back["t"], (est["pose"][:, :3, 3] / 1000.0).astype(np.float32) * 1000)
    (tmp_path / "bad.csv").write_text("1,2,3,0.5,1 0 0 0 1 0 0 0,0 0 0,0.1\n")
    with pytest.raises(ValueError, match="bad.csv:1"):
        ev.read_bop_csv(tmp_path / "bad.csv")


def _write_ply(path, v, f):
    with open(path, "w") as fh:
        fh.write(f"ply\nformat ascii 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
                 f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
        fh.writelines(f"{a:.9g} {b:.9g} {c:.9g}\n" for a, b, c in v.tolist())
        fh.writelines(f"3 {a} {b} {c}\n" for a, b, c in f.tolist())


def test_bop_eval_tool_on_a_two_image_dataset(tmp_path, capsys):
    """tools/bop_eval.py on a dataset built here: json files, two small PLY models, 16-bit depth PNGs (depth_scale 0.1), a
    scene_gt_info.json that hides one instance; scored on the CPU."""
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bop_eval
    models, gt, images = _scene()
    root, scene = tmp_path / "ds", tmp_path / "ds" / "test" / "000048"
    (root / "models_eval").mkdir(parents=True)
    (scene / "depth").mkdir(parents=True)
    info = {}
    for obj, m in models.items():
        _write_ply(root / "models_eval" / f"obj_{obj:06d}.ply", m["vertices"], m["faces"])
        info[str(obj)] = {"diameter": float(m["diameter"])}
    (root / "models_eval" / "models_info.json").write_text(json.dumps(info))
    ims = [3, 11]
    scene_gt = {str(ims[i]): [] for i in range(2)}
    for i in range(len(gt["pose"])):
        scene_gt[str(ims[gt["im"][i]])].append({"cam_R_m2c": gt["pose"][i, :3, :3].reshape(-1).tolist(), "cam_t_m2c": gt["pose"][i, :3, 3].tolist(),
                                                "obj_id": int(gt["obj"][i])})
    # a third, barely visible instance in image 11: not a target
    scene_gt["11"].append({"cam_R_m2c": np.eye(3).reshape(-1).tolist(), "cam_t_m2c": [0.0, 0.0, 900.0], "obj_id": 5})
    (scene / "scene_gt.json").write_text(json.dumps(scene_gt))
    (scene / "scene_gt_info.json").write_text(json.dumps({"3": [{"visib_fract": 1.0}, {"visib_fract": 0.8}],
                                                          "11": [{"visib_fract": 0.9}, {"visib_fract": 0.5}, {"visib_fract": 0.02}]}))
    K = [float(CAM[0]), 0.0, float(CAM[2]), 0.0, float(CAM[1]), float(CAM[3]), 0.0, 0.0, 1.0]
    (scene / "scene_camera.json").write_text(json.dumps({str(i): {"cam_K": K, "depth_scale": 0.1} for i in ims}))
    for i, im in enumerate(ims):
        Image.fromarray(np.rint(images["depth"][i] * 10).astype(np.uint16)).save(scene / "depth" / f"{im:06d}.png")
    _csv(tmp_path / "exact.csv", gt, [48, 48], ims, 0.0)
    _csv(tmp_path / "noisy.csv", gt, [48, 48], ims, 30.0)
    exact = bop_eval.main(["--results", str(tmp_path / "exact.csv"), "--dataset", str(root), "--device", "cpu"])
    line = capsys.readouterr().out.strip().splitlines()
    assert len(line) == 1 and json.loads(line[0])["AR"] == exact["AR"]
    assert exact["targets"] == 4 and exact["estimates"] == 4 and exact["images"] == 2 and exact["dropped_estimates"] == 0
    assert exact["AR_MSSD"] == 1.0 and exact["AR_MSPD"] == 1.0 and exact["AR_VSD"] == 1.0 and exact["AR"] == 1.0
    noisy = bop_eval.main(["--results", str(tmp_path / "noisy.csv"), "--dataset", str(root), "--device", "cpu"])
    assert noisy["AR"] < 0.8 and noisy["AR_MSSD"] < 1.0
