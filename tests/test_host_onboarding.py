"""Template onboarding on the host: the restatement (tests/onboarding_ref.py) against the reference-made golden, the library-op
statement of sam6d_amd.onboarding on CPU tensors against the restatement (bit for bit), view selection, numpy-compatible draws,
the errors, the directory loader and the save / load round trip."""
import numpy as np
import pytest
import torch

from sam6d_amd import onboarding as ob
from tests import onboarding_ref as R
from tests import util


@pytest.fixture(scope="module")
def case():
    c = R.case_templates()
    return c


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


GOOD = [i for i in range(R.T) if i != R.EMPTY_VIEW]


def test_restatement_equals_the_reference_made_golden(case):
    g = util.golden("onboarding.npz")
    assert str(g["digest"]) == R.digest(case) and g["views"].tolist() == GOOD
    for j, i in enumerate(GOOD):
        _, rgb_choose, _, bbox = R.pem_template(case["rgb"][i], case["mask"][i], case["xyz"][i], case["keys"][i])
        assert bbox == g["square"][j].tolist(), i
        np.testing.assert_array_equal(rgb_choose, g["rgb_choose"][j])
        assert R.pil_bbox(case["mask"][i]) == g["pil"][j].tolist(), i
    assert R.pil_bbox(case["mask"][R.EMPTY_VIEW]) is None
    iv = g["ism_views"].tolist()
    assert R.GREY_VIEW in iv and len(iv) >= 12
    tem, msk = R.ism_templates(case["rgb"][iv], case["mask"][iv])
    np.testing.assert_array_equal(tem.numpy(), g["templates"])
    np.testing.assert_array_equal(msk.numpy(), g["masks"])
    # the square side of every case is the one the table promises, and the grey pixels widen only the ISM's box
    sides = (g["square"][:, 1] - g["square"][:, 0]).tolist()
    assert sides[:6] == [16, 32, 6, 22, 32, 48] and sides[10] == 72 and sides[R.GREY_VIEW] == 16
    assert g["square"][6, 0] == 0 and g["square"][7, 2] == 0 and g["square"][8, 1] == R.H and g["square"][9, 3] == R.W
    assert g["pil"][R.GREY_VIEW].tolist() == [30, 20, 50, 36]


def test_u8_over_255_is_one_float32_division():
    """np.array(image) / 255 is a float64 quotient that .float() rounds again; the kernels divide in float32.  The same 256 values."""
    a = np.arange(256, dtype=np.uint8)
    np.testing.assert_array_equal(torch.from_numpy(a / 255).float().numpy(), a.astype(np.float32) / np.float32(255))


@pytest.mark.parametrize("flag", [True, False])
def test_pem_library_statement_equals_the_restatement(case, flag):
    kw = dict(n_sample=R.N_SAMPLE, img_size=R.S, rgb_mask_flag=flag)
    want = R.pem_templates(case["rgb"][None, GOOD], case["mask"][None, GOOD], case["xyz"][None, GOOD], case["keys"][None, GOOD], **kw)
    got = ob.pem_template_inputs(_t(case["rgb"][GOOD]), _t(case["mask"][GOOD]), _t(case["xyz"][GOOD]), keys=_t(case["keys"][GOOD]), **kw)
    assert [len(x) for x in got] == [len(GOOD)] * 3
    for g_, w_, dt in zip(got, want, (torch.float32, torch.float32, torch.int64)):
        for v in range(len(GOOD)):
            assert g_[v].dtype == dt and g_[v].shape[0] == 1
            np.testing.assert_array_equal(g_[v].numpy(), w_[v], err_msg=f"view {GOOD[v]}")


def test_pem_object_dimension_and_view_selection(case):
    T = 42
    pick = [GOOD[i % len(GOOD)] for i in range(2 * T)]
    rgb, mask, xyz, keys = (case[k][pick].reshape((2, T) + case[k].shape[1:]) for k in ("rgb", "mask", "xyz", "keys"))
    for n_view in (42, 6, 5):
        views = [int(T / n_view * v) for v in range(n_view)]
        assert views == {42: list(range(42)), 6: [0, 7, 14, 21, 28, 35], 5: [0, 8, 16, 25, 33]}[n_view]
        want = R.pem_templates(rgb, mask, xyz, keys, n_view=n_view, n_sample=64)
        got = ob.pem_template_inputs(_t(rgb), _t(mask), _t(xyz), keys=_t(keys), n_sample=64, img_size=R.S, n_view=n_view)
        for g_, w_ in zip(got, want):
            assert len(g_) == n_view
            for v in range(n_view):
                np.testing.assert_array_equal(g_[v].numpy(), w_[v])


def test_rng_draws_equal_a_numpy_loop(case):
    pick = [[0, 5, 2], [10, 3, 1]]
    rgb, mask, xyz = (case[k][pick] for k in ("rgb", "mask", "xyz"))
    want = R.pem_templates(rgb, mask, xyz, rng=np.random.RandomState(5), n_sample=150)
    got = ob.pem_template_inputs(_t(rgb), _t(mask), _t(xyz), rng=np.random.RandomState(5), n_sample=150, img_size=R.S)
    for g_, w_ in zip(got, want):
        for v in range(3):
            np.testing.assert_array_equal(g_[v].numpy(), w_[v])
    with pytest.raises(ValueError, match="either keys"):
        ob.pem_template_inputs(_t(rgb), _t(mask), _t(xyz))
    with pytest.raises(ValueError, match="either keys"):
        ob.pem_template_inputs(_t(rgb), _t(mask), _t(xyz), keys=_t(case["keys"][pick]), rng=np.random)


def test_empty_view_raises_naming_it(case):
    pick = [0, R.EMPTY_VIEW, 2, 3]
    args = [_t(case[k][pick]) for k in ("rgb", "mask", "xyz")]
    with pytest.raises(ValueError, match=r"view\(s\) 1 of object 0"):
        ob.pem_template_inputs(*args, keys=_t(case["keys"][pick]), n_sample=32, img_size=R.S)
    with pytest.raises(ValueError, match=r"view\(s\) 2 of object 0"):          # n_view = 2 of 4 picks views 0 and 2
        ob.pem_template_inputs(args[0][[0, 2, 1, 3]], args[1][[0, 2, 1, 3]], args[2][[0, 2, 1, 3]], rng=np.random.RandomState(0),
                               n_sample=32, img_size=R.S, n_view=2)
    with pytest.raises(ValueError, match=r"template view\(s\) \[1\]"):
        ob.ism_template_inputs(args[0], args[1], R.S)


@pytest.mark.parametrize("normalize", [False, True])
def test_ism_library_statement_equals_the_restatement(case, normalize):
    tem, msk = ob.ism_template_inputs(_t(case["rgb"][GOOD]), _t(case["mask"][GOOD]), R.S, normalize)
    want_t, want_m = R.ism_templates(case["rgb"][GOOD], case["mask"][GOOD], R.S, normalize)
    assert torch.equal(tem, want_t) and torch.equal(msk, want_m)
    # view 2 (a 7 x 5 tight box) is padded left and right: zero without the transform, (0 - mean) / std with it
    pad = tem[2][:, :, 0]
    mean, std = torch.tensor(ob.RGB_MEAN), torch.tensor(ob.RGB_STD)
    assert torch.equal(pad, ((torch.zeros(3) - mean) / std)[:, None].expand(3, R.S) if normalize else torch.zeros(3, R.S))
    assert torch.equal(msk[2][:, 0], torch.zeros(R.S))
    # the 128-valued pixels are inside the crop, scaled by 128 / 255
    assert (msk[R.GREY_VIEW] == torch.tensor(128 / 255).float()).any() and (msk[R.GREY_VIEW] == 1).any()


def test_square_tight_boxes_raise_exactly_where_crop_valid_says(case):
    """CropResizePad fails on some exactly square boxes (at a target of 56: sides 19, 20, 22 of 16 .. 24) and on slivers."""
    from sam6d_amd.ism.dinov2 import crop_valid
    target = 56
    shapes = [(s, s) for s in range(16, 25)] + [(1, 60), (60, 1)]
    valid = crop_valid(np.array([[4, 4, 4 + w, 4 + h] for h, w in shapes]), target).tolist()
    assert valid == [True, True, True, False, False, True, False, True, True, False, False]
    rgb = _t(case["rgb"][:1])
    for (h, w), ok in zip(shapes, valid):
        mask = torch.zeros(1, R.H, R.W, dtype=torch.uint8)
        mask[0, 4:4 + h, 4:4 + w] = 255
        if ok:
            tem, msk = ob.ism_template_inputs(rgb, mask, target)
            want_t, want_m = R.ism_templates(rgb.numpy(), mask.numpy(), target)
            assert torch.equal(tem, want_t) and torch.equal(msk, want_m), (h, w)
        else:
            with pytest.raises(ValueError, match=r"template view\(s\) \[0\]"):
                ob.ism_template_inputs(rgb, mask, target)
            try:                                                       # the reference: an error, or a crop of another size (which
                shape = R.ism_templates(rgb.numpy(), mask.numpy(), target)[0].shape[-2:]          # torch.stack refuses later)
            except (AssertionError, RuntimeError, ValueError):
                shape = None
            assert shape is None or tuple(shape) != (target, target), (h, w)


def test_load_template_dir_round_trips(case, tmp_path):
    from PIL import Image
    for i in range(3):
        Image.fromarray(case["rgb"][i], mode="RGB").save(tmp_path / f"rgb_{i}.png")
        Image.fromarray(case["mask"][i], mode="L").save(tmp_path / f"mask_{i}.png")
        np.save(tmp_path / f"xyz_{i}.npy", case["xyz"][i].astype(np.float64))
    rgb, mask, xyz = ob.load_template_dir(str(tmp_path))
    assert rgb.dtype == np.uint8 and mask.dtype == np.uint8 and xyz.dtype == np.float32
    np.testing.assert_array_equal(rgb, case["rgb"][:3])
    np.testing.assert_array_equal(mask, case["mask"][:3])
    np.testing.assert_array_equal(xyz, case["xyz"][:3])
    with pytest.raises(FileNotFoundError):
        ob.load_template_dir(str(tmp_path / "none"))


class _Desc:
    """Recording stand-in for CustomDINOv2."""
    proposal_size = R.S

    def __init__(self):
        self.seen = []

    def compute_features(self, images, token_name):
        self.seen.append(("cls", images.clone(), token_name))
        return images.flatten(1)[:, :8].clone()

    def compute_masked_patch_feature(self, images, masks):
        self.seen.append(("patch", images.clone(), masks.clone()))
        return masks.flatten(1)[:, :12].reshape(-1, 4, 3).clone()


class _Net(torch.nn.Module):
    """Recording stand-in for the PEM Net: get_obj_feats keeps what it is handed."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.feature_extraction = self
        self.seen = None

    def get_obj_feats(self, tem_rgb, tem_pts, tem_choose):
        self.seen = (tem_rgb, tem_pts, tem_choose)
        pts = torch.cat(tem_pts, 1)
        return pts[:, :10].clone(), torch.cat([c.float()[:, :, None] for c in tem_choose], 1)[:, :10].clone()


def test_onboard_hands_both_models_their_inputs_and_round_trips(case, tmp_path):
    pick = [[0, 1, 5, 3], [7, 10, 11, 9]]
    r = np.random.RandomState(2)
    objects = [dict(rgb=case["rgb"][p], mask=case["mask"][p], xyz_mm=case["xyz"][p], model_points=r.standard_normal((20, 3)).astype(np.float32),
                    ism_points=r.standard_normal((9, 3)).astype(np.float32), poses=np.tile(np.eye(4, dtype=np.float32), (4, 1, 1))) for p in pick]
    keys = _t(case["keys"][pick])
    desc, net = _Desc(), _Net()
    o = ob.onboard(desc, net, objects, keys=keys, n_view=2, n_sample=50, img_size=R.S, confidence_thresh=0.3)
    want = R.pem_templates(case["rgb"][pick], case["mask"][pick], case["xyz"][pick], case["keys"][pick], n_view=2, n_sample=50)
    for g_, w_ in zip(net.seen, want):
        assert len(g_) == 2
        for v in range(2):
            np.testing.assert_array_equal(g_[v].numpy(), w_[v])
    assert [s[0] for s in desc.seen] == ["cls", "patch"] * 2 and desc.seen[0][2] == "x_norm_clstoken"
    for ob_i, p in enumerate(pick):
        tem, msk = R.ism_templates(case["rgb"][p], case["mask"][p], R.S)
        assert torch.equal(desc.seen[2 * ob_i][1], tem) and torch.equal(desc.seen[2 * ob_i + 1][1], tem)
        assert torch.equal(desc.seen[2 * ob_i + 1][2], msk)
    rd = o.scorer.ref_data
    assert rd["descriptors"].shape == (2, 4, 8) and rd["appe_descriptors"].shape == (2, 4, 4, 3)
    assert rd["poses"].shape == (4, 4, 4) and rd["pointcloud"].shape == (2, 9, 3)
    with pytest.raises(ValueError, match="template poses differ"):
        ob.onboard(desc, net, [objects[0], dict(objects[1], poses=2 * objects[1]["poses"])], keys=keys, n_view=2, n_sample=50, img_size=R.S)
    assert o.scorer.matching_config.confidence_thresh == 0.3
    assert set(o.pem_templates) == {"model", "dense_po", "dense_fo"} and o.pem_templates["model"].shape == (2, 20, 3)
    want_r = [float(np.max(np.linalg.norm(ob_["model_points"], axis=1))) for ob_ in objects]
    np.testing.assert_allclose(o.object_radius.numpy(), want_r, rtol=1e-6)
    path = tmp_path / "onboarded.pt"
    o.save(str(path))
    b = ob.Onboarded.load(str(path), "cpu")
    for k in rd:
        assert torch.equal(b.scorer.ref_data[k], rd[k]), k
    for k in o.pem_templates:
        assert torch.equal(b.pem_templates[k], o.pem_templates[k]), k
    assert torch.equal(b.object_radius, o.object_radius)
    assert b.scorer.matching_config.confidence_thresh == 0.3 and b.scorer.visible_thred == o.scorer.visible_thred
    assert b.scorer.matching_config.aggregation_function == o.scorer.matching_config.aggregation_function
