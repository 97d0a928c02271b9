"""sam6d_amd.visualize on host tensors: the torch statements of the overlay definitions (csrc/s6d_vis.hip) against the plain-loop
restatement of tests/vis_ref.py through the bodies of tests/test_gpu_vis.py; the palette; the argument checks; strict mode; and
tools/visualize.py on a tiny synthetic dataset.  No GPU and no emulator here: `surface` pictures need the rasteriser and are covered
by tests/test_emu_vis.py and tests/test_gpu_vis.py."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from sam6d_amd import groundtruth as gtm
from sam6d_amd import policy
from sam6d_amd import visualize as V
from tests import test_gpu_vis as T
from tests import test_host_bop_gt as HB
from tests import vis_ref as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class LibraryApi:
    """The torch statements of sam6d_amd/visualize.py on host tensors, behind the interface of ``test_gpu_vis.KernelApi``."""
    chunk = 256

    @staticmethod
    def t(a):
        return torch.from_numpy(np.array(a, order="C"))

    def pack(self, masks):
        from sam6d_amd.ism import handoff
        return handoff._pack_library(masks)[0]

    def owner(self, packed, order, start, H, W):
        return V.owner_from_masks(packed, order, start, H, W)

    def canvas(self, B, H, W):
        return dict(zbuf=torch.zeros(B, H, W), owner=torch.full((B, H, W), -1, dtype=torch.int32), shade=torch.zeros(B, H, W, 3, dtype=torch.uint8))

    def merge(self, canvas, depth, rgb, frame, first):
        return V._merge_library(canvas, depth, rgb, frame, first)

    def paint(self, image, owner, **k):
        return V.paint(image, owner, **k)

    def project(self, *a):
        return V.project(*a)

    def draw(self, image, prims, start, check=True):
        return V._draw_library(image, prims, start, chunk_elems=1 << 16)


@pytest.fixture(scope="module")
def api():
    return LibraryApi()


@pytest.mark.parametrize("N", T.OWNER_N)
@pytest.mark.parametrize("B", T.BATCHES)
@pytest.mark.parametrize("hw", T.SIZES)
def test_owner_statement_vs_restatement(api, hw, B, N):
    T.check_owner(api, hw, B, N)


@pytest.mark.parametrize("B", T.BATCHES)
@pytest.mark.parametrize("hw", T.SIZES[:3])
def test_merge_statement_vs_restatement(api, hw, B):
    T.check_merge(api, hw, B)


@pytest.mark.parametrize("config", T.PAINT_CONFIGS)
@pytest.mark.parametrize("B", T.BATCHES)
@pytest.mark.parametrize("hw", T.SIZES)
def test_paint_statement_vs_restatement(api, hw, B, config):
    T.check_paint(api, hw, B, config)


def test_known_answers(api):
    T.check_paint_known_answer(api)
    T.check_draw_known_answer(api)


def test_projection_statement_bits(api):
    T.check_project(api)


@pytest.mark.parametrize("B", T.BATCHES)
@pytest.mark.parametrize("hw", T.SIZES)
def test_draw_statement_vs_restatement(api, hw, B):
    T.check_draw(api, hw, B)


def test_draw_statement_other_frames_and_empty_list(api):
    T.check_draw_other_frames_and_empty(api)


def _host_scene():
    obj, frame, poses, cam = T.scene()
    K = np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1]], np.float32)
    return obj, frame, poses, cam, K


def test_box_and_point_pictures_on_the_host():
    """overlay_poses without the surface layer needs no rasteriser: the picture of the restatement, default and given colours, both
    box centres (the cube's mean is its centre: the same picture), a frame alone as in the group."""
    obj, frame, poses, cam, K = _host_scene()
    img = T._image(T.SCENE_HW, seed=3)
    Rm, t = poses[:, :3, :3].copy(), poses[:, :3, 3].copy()
    cams = np.tile(cam, (len(obj), 1))
    want = REF.draw(img, REF.pose_primitives(T._models(), obj, Rm, t, cams, frame, T._palette_by_position(frame), ("box", "points")))
    got = V.overlay_poses(torch.from_numpy(img), T._models(), obj, Rm, t, K, frame_index=frame)
    assert not got.is_cuda and np.array_equal(got.numpy(), want)
    colors = np.random.RandomState(0).randint(0, 256, (len(obj), 3)).astype(np.uint8)
    want = REF.draw(img, REF.pose_primitives(T._models(), obj, Rm, t, cams, frame, colors, ("box",), center="mean"))
    got = V.overlay_poses(torch.from_numpy(img), T._models(), obj, Rm, t, cams, frame_index=frame, mode="box", colors=colors, box_center="mean")
    assert np.array_equal(got.numpy(), want)
    sel = np.nonzero(frame == 2)[0]
    one = V.overlay_poses(torch.from_numpy(img[2]), T._models(), [obj[n] for n in sel], Rm[sel], t[sel], K, mode="box", colors=colors[sel], box_center="mean")
    assert torch.equal(one, got[2])
    with pytest.raises(ValueError, match="rasteriser"):
        V.overlay_poses(torch.from_numpy(img), T._models(), obj, Rm, t, K, frame_index=frame, mode=("surface",))
    pts = np.array([[0, 0, 0], [40, 40, 40]], np.float32)
    got = V.overlay_poses(torch.from_numpy(img[:1]), T._models(), [1], Rm[:1], t[:1], K, mode="points", points=pts)
    xy, ok = REF.project(pts, [0, 0], Rm, t, cams, 1.0)
    prims = [[0, *xy[m], *xy[m], 2, 255, int(ok[m])] for m in range(2)]                     # palette entry 0 is (255, 0, 0)
    assert np.array_equal(got.numpy(), REF.draw(img[:1], np.asarray(prims)))


def test_box_corner_order_and_shades():
    c = V.box_corners(np.array([[-1, -2, -3], [3, 4, 5]], np.float32)).numpy()
    assert c.tolist() == [[3, 4, 5], [3, 4, -3], [-1, 4, 5], [-1, 4, -3], [3, -2, 5], [3, -2, -3], [-1, -2, 5], [-1, -2, -3]]
    assert np.array_equal(c, REF.box_corners(np.array([[-1, -2, -3], [3, 4, 5]], np.float32)))
    assert list(V.BOX_EDGES) == REF.BOX_EDGES
    assert all(int(0.3 * v) == (3 * v) // 10 and int(0.6 * v) == (6 * v) // 10 for v in range(256))       # the integer form of int(s c)
    v = np.arange(3 * 2000, dtype=np.float32).reshape(2000, 3)
    assert np.array_equal(V.model_points(v).numpy(), v[::3][:512]) and np.array_equal(V.model_points(v[:100]).numpy(), v[:100])
    assert np.array_equal(REF.model_points(v), v[::3][:512])


def test_palette_is_fixed_and_entry_k_depends_on_k_alone():
    p = V.palette(40).numpy()
    assert p.dtype == np.uint8 and p.shape == (40, 3)
    assert p[:4].tolist() == [[255, 0, 0], [0, 255, 72], [145, 0, 255], [255, 217, 0]]
    assert p[12].tolist() == [(c * 200 + 127) // 255 for c in (0, 255 - (255 * 24 + 30) // 60, 255)]          # h = 204: sector 3, f = 24
    assert np.array_equal(V.palette(7).numpy(), p[:7]) and V.palette(0).shape == (0, 3)
    assert len({tuple(c) for c in p.tolist()}) == 40


def test_side_by_side_and_save_png(tmp_path):
    from PIL import Image
    a, b = torch.zeros(2, 4, 5, 3, dtype=torch.uint8), torch.ones(2, 4, 7, 3, dtype=torch.uint8)
    both = V.side_by_side(a, b)
    assert both.shape == (2, 4, 12, 3) and not both[:, :, :5].any() and both[:, :, 5:].all()
    assert V.side_by_side(a[0], b[0]).shape == (4, 12, 3)
    with pytest.raises(ValueError, match="one height"):
        V.side_by_side(a, b[:, :3])
    img = torch.from_numpy(T._image((5, 7))[0])
    V.save_png(tmp_path / "x.png", img)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "x.png")), img.numpy())
    with pytest.raises(ValueError, match="uint8"):
        V.save_png(tmp_path / "y.png", img.float())


def test_arguments_on_the_host():
    img = torch.zeros(1, 4, 8, 3, dtype=torch.uint8)
    masks, scores = torch.zeros(1, 4, 8, dtype=torch.uint8), torch.ones(1)
    with pytest.raises(ValueError, match="H and W"):
        V.overlay_detections(torch.zeros(1, 1, 8193, 3, dtype=torch.uint8), torch.zeros(0, 1, 8193, dtype=torch.uint8), torch.zeros(0))
    with pytest.raises(ValueError, match="edge_width"):
        V.overlay_detections(img, masks, scores, edge_width=5)
    with pytest.raises(ValueError, match="alpha"):
        V.overlay_detections(img, masks, scores, alpha=257)
    with pytest.raises(ValueError, match="frame_index"):
        V.overlay_detections(img, masks, scores, frame_index=[1])
    with pytest.raises(ValueError, match="frame_index is needed"):
        V.overlay_detections(img.expand(2, 4, 8, 3), masks, scores)
    with pytest.raises(ValueError, match="words"):
        V.overlay_detections(img, torch.zeros(1, 2, dtype=torch.int64), scores)
    with pytest.raises(ValueError, match="scores"):
        V.overlay_detections(img, masks, torch.ones(2))
    with pytest.raises(ValueError, match="size"):
        V.draw(img, torch.tensor([[0, 1, 1, 2, 2, 65, 0, 1]], dtype=torch.int32))
    with pytest.raises(ValueError, match="frame"):
        V.draw(img, torch.tensor([[1, 1, 1, 2, 2, 3, 0, 1]], dtype=torch.int32))
    with pytest.raises(ValueError, match="mode"):
        V.overlay_poses(img, {}, [], np.zeros((0, 3, 3)), np.zeros((0, 3)), np.eye(3), mode=("wire",))
    with pytest.raises(ValueError, match="box_center"):
        V.box_corners(np.zeros((2, 3), np.float32), "median")
    with pytest.raises(ValueError, match="uint8"):
        V.overlay_detections(img.float(), masks, scores)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        from sam6d_amd import ops
        ops.vis_paint(img, torch.zeros(1, 4, 8, dtype=torch.int32), colors=torch.zeros(1, 3, dtype=torch.uint8))
    # no instance and no detection: the base picture
    assert torch.equal(V.overlay_poses(img + 7, {}, [], np.zeros((0, 3, 3)), np.zeros((0, 3)), np.eye(3)), img + 7)
    assert torch.equal(V.overlay_detections(img + 7, torch.zeros(0, 4, 8, dtype=torch.uint8), torch.zeros(0), gray=False), img + 7)


def test_host_tensors_are_not_a_library_branch_and_the_sites_are_named(monkeypatch):
    """Host tensors go to the torch statements without a record; a device tensor without the kernel would be recorded under the
    three sites (seen here by letting a host tensor claim to be a device tensor while the kernels are switched off)."""
    img = torch.zeros(1, 4, 8, 3, dtype=torch.uint8)
    masks, scores = torch.ones(1, 4, 8, dtype=torch.uint8), torch.ones(1)
    V.overlay_detections(img, masks, scores)
    assert not policy.library_branch_hits()
    monkeypatch.setattr(V.ops, "have", lambda name: False)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    V.overlay_detections(img, masks, scores)
    V.draw(img, torch.tensor([[0, 1, 1, 2, 2, 3, 0, 1]], dtype=torch.int32))
    sites = {h[0] if isinstance(h, tuple) else h for h in policy.library_branch_hits()}
    assert {"visualize.owner", "visualize.paint", "visualize.draw"} <= sites
    monkeypatch.setenv("S6D_STRICT", "1")
    with pytest.raises(policy.StrictError, match="visualize.paint"):
        V.paint(img, torch.zeros(1, 4, 8, dtype=torch.int32), colors=torch.zeros(1, 3, dtype=torch.uint8))


def test_overlay_results_takes_what_run_group_returns():
    from sam6d_amd.ism import handoff
    obj, frame, poses, cam, K = _host_scene()
    img = T._image(T.SCENE_HW, seed=6)
    masks = torch.zeros(2, *T.SCENE_HW, dtype=torch.bool)
    masks[0, 5:20, 5:30], masks[1, 10:30, 20:50] = True, True
    det = handoff.Detections(1, 1, masks, torch.zeros(2, 4), torch.tensor([0.3, 0.8]), torch.tensor([0, 1]))
    got = dict(pred_R=torch.from_numpy(poses[[0, 3], :3, :3].copy()), pred_t=torch.from_numpy(poses[[0, 3], :3, 3].copy()) / 1000.0,
               pred_pose_score=torch.ones(2), kept=torch.tensor([1, 0]))
    empty = handoff.Detections(1, 2, masks[:0], torch.zeros(0, 4), torch.zeros(0), torch.zeros(0, dtype=torch.long))
    frames = [(torch.from_numpy(img[b]), None, torch.from_numpy(K)) for b in range(2)]
    ism, pem = V.overlay_results(frames, [(det, got), (empty, None)], T._models(), pose_scale=1000.0)
    assert np.array_equal(ism.numpy(), V.overlay_detections(torch.from_numpy(img[:2]), masks, det.scores, frame_index=[0, 0], top=1).numpy())
    want = V.overlay_poses(torch.from_numpy(img[:2]), T._models(), [2, 1], poses[[0, 3], :3, :3].copy(),
                           (torch.from_numpy(poses[[0, 3], :3, 3].copy()) / 1000.0) * 1000.0, K, frame_index=[0, 0])
    assert torch.equal(pem, want) and not torch.equal(pem[0], frames[0][0]) and torch.equal(pem[1], frames[1][0])
    assert np.array_equal(ism[1].numpy(), REF.paint(img[1:2], np.full((1, *T.SCENE_HW), -1), colors=np.zeros((1, 3), np.uint8))[0])


def _tool():
    spec = importlib.util.spec_from_file_location("s6d_tools_visualize", os.path.join(ROOT, "tools", "visualize.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_writes_both_pictures_for_a_synthetic_dataset(tmp_path, capsys):
    from PIL import Image
    tool = _tool()
    root = tmp_path / "ds"
    models, gt, images, scene = HB._write_dataset(root)
    (root / "models_eval" / "models_info.json").write_text(json.dumps({str(o): gtm.model_info(m["vertices"], device="cpu") for o, m in models.items()}))
    images["depth"] = (np.rint(images["depth"] * 10).astype(np.uint16).astype(np.float32) * np.float32(0.1))          # as the PNG gives it back
    HB._result_files(tmp_path, gt, gtm.instance_ground_truth(models, gt, images, device="cpu"))
    (scene / "rgb").mkdir()
    rgb = np.random.RandomState(1).randint(0, 256, (HB.H, HB.W, 3)).astype(np.uint8)
    Image.fromarray(rgb).save(scene / "rgb" / f"{HB.IMS[0]:06d}.png")                      # the other frame is drawn over its depth
    out = tmp_path / "vis"
    args = ["--dataset", str(root), "--out", str(out), "--device", "cpu", "--results", str(tmp_path / "poses.csv"), "--gt", "--detections",
            str(tmp_path / "dets.json")]
    line = tool.main(args)
    printed = capsys.readouterr().out.strip().splitlines()
    assert len(printed) == 1 and json.loads(printed[0]) == line
    assert line["images"] == 2 and line["files"] == 4 and line["pose_sets"] == 2 and line["instances"] == 12 and line["detections"] == 6
    names = sorted(os.listdir(out))
    assert names == sorted(f"vis_{k}_{HB.SCENE:06d}_{im:06d}.png" for k in ("ism", "pem") for im in HB.IMS)
    # the pictures are what the module draws from the same files' contents
    sel = np.nonzero(gt["im"] == 0)[0]
    from sam6d_amd import evaluation
    res = evaluation.read_bop_csv(tmp_path / "poses.csv")
    mine = [n for n in range(len(res["im"])) if res["im"][n] == HB.IMS[0]]
    pal = V.palette(2)
    R_all = np.concatenate([res["R"][mine], gt["pose"][sel, :3, :3].astype(np.float32)])
    t_all = np.concatenate([res["t"][mine], gt["pose"][sel, :3, 3].astype(np.float32)])
    want = V.overlay_poses(torch.from_numpy(rgb), models, res["obj"][mine].tolist() + gt["obj"][sel].tolist(), R_all, t_all, images["cams"][0],
                           colors=pal[[0] * len(mine) + [1] * len(sel)])
    pem = np.asarray(Image.open(out / f"vis_pem_{HB.SCENE:06d}_{HB.IMS[0]:06d}.png"))
    assert np.array_equal(pem, want.numpy()) and not np.array_equal(pem, rgb)
    assert (pem == pal[0].numpy()).all(2).any() and (pem == pal[1].numpy()).all(2).any()              # both pose sets show, each in its colour
    ism = np.asarray(Image.open(out / f"vis_ism_{HB.SCENE:06d}_{HB.IMS[0]:06d}.png"))
    assert (ism == 255).all(2).any() and not np.array_equal(ism, rgb)
    dense = tool.main(args + ["--masks", "dense", "--force", "--top", "0"])
    capsys.readouterr()
    assert dense["files"] == 4
    # never over an existing file without --force, and nothing is touched by the refusal
    before = (out / names[0]).read_bytes()
    with pytest.raises(FileExistsError, match="--force"):
        tool.main(args)
    assert (out / names[0]).read_bytes() == before
    with pytest.raises(SystemExit):
        tool.main(["--dataset", str(root), "--out", str(out)])
