"""The onboarding kernels (csrc/s6d_onboard.hip, the raised sampler of csrc/s6d_pempre.hip) on the emulator, bit for bit against the
restatement of the reference (tests/onboarding_ref.py) and against the library-op statement of sam6d_amd/onboarding.py."""
import numpy as np
import pytest
import torch

from oracle import pem_pre as o
from sam6d_amd import onboarding as ob
from sam6d_amd import policy
from sam6d_amd.pem import preprocess as pre
from tests import onboarding_ref as R


@pytest.fixture(scope="module")
def case():
    return {k: torch.from_numpy(v) for k, v in R.case_templates().items()}


GOOD = [i for i in range(R.T) if i != R.EMPTY_VIEW]


def test_boxes_kernel_equals_get_bbox_and_pil_getbbox(emu, case):
    mask = case["mask"]
    cnt, box, tight = emu.template_boxes(mask)
    for i in range(R.T):
        m = mask[i].numpy()
        assert int(cnt[i]) == int((m == 255).sum())
        assert box[i].tolist() == [int(v) for v in o.get_bbox(m == 255 if i != R.EMPTY_VIEW else np.ones_like(m))], i
        assert tight[i].tolist() == (R.pil_bbox(m) or [0, 0, 0, 0]), i
    assert torch.equal(box[GOOD], pre.square_boxes(mask[GOOD] == 255)) and torch.equal(tight, ob._tight_boxes(mask))
    assert box[R.GREY_VIEW].tolist() == [20, 36, 28, 44] and tight[R.GREY_VIEW].tolist() == [30, 20, 50, 36]


def test_points_kernel_compacts_in_crop_order_and_divides_in_float32(emu, case):
    mask, xyz = case["mask"], case["xyz"]
    _, box, _ = emu.template_boxes(mask)
    cap = min(R.H, R.W) ** 2
    choose, pts, n = emu.template_points(mask, xyz, box, cap)
    for i in range(R.T):
        y1, y2, x1, x2 = box[i].tolist()
        want = (mask[i].numpy()[y1:y2, x1:x2] == 255).astype(np.float32).flatten().nonzero()[0]
        assert int(n[i]) == len(want) and (len(want) > 0) == (i != R.EMPTY_VIEW)
        np.testing.assert_array_equal(choose[i, :len(want)].numpy(), want)
        want_xyz = (xyz[i].numpy().astype(np.float32) / 1000.0)[y1:y2, x1:x2, :].reshape(-1, 3)[want]
        np.testing.assert_array_equal(pts[i, :len(want)].numpy(), want_xyz)
    bad = box.clone()
    bad[0] = torch.tensor([0, R.H + 1, 0, 10])                      # not inside the view: skipped whole
    bad[1] = torch.tensor([10, 5, 0, 10])
    assert emu.template_points(mask, xyz, bad, cap)[2][:3].tolist() == [0, 0, int(n[2])]


@pytest.mark.parametrize("flag", [True, False])
def test_pem_crops_kernel_at_every_ratio(emu, case, flag):
    """The case table's boxes (16: copy, 32: box average, 6 / 22 / 48 / 72, the four borders) and explicit boxes of odd sides."""
    rgb, mask = case["rgb"][GOOD], case["mask"][GOOD]
    _, box, _ = emu.template_boxes(mask)
    odd = [(7, (3, 70)), (23, (40, 5)), (33, (39, 47)), (5, (67, 91))]
    box = torch.cat([box, torch.tensor([[y, y + s, x, x + s] for s, (y, x) in odd])])
    rgb, mask = torch.cat([rgb, rgb[:len(odd)]]), torch.cat([mask, mask[[5, 10, 5, 9]]])
    got = emu.template_pem_crops(rgb.contiguous(), mask.contiguous(), box, R.S, flag, pre.MEAN, pre.STD)
    assert torch.equal(got, pre._crops(rgb, (mask == 255).float(), box, R.S, flag))
    for i, (y1, y2, x1, x2) in enumerate(box.tolist()):
        c = rgb[i].numpy()[:, :, ::-1][y1:y2, x1:x2, :]
        if flag:
            c = c * (mask[i].numpy()[y1:y2, x1:x2, None] == 255).astype(np.uint8)
        want = (o.cv2_resize_linear_u8(c, R.S).astype(np.float32) / np.float32(255) - o.MEAN) / o.STD
        assert np.array_equal(got[i].numpy(), want.transpose(2, 0, 1)), (i, flag)
    bad = box.clone()
    bad[0] = torch.tensor([0, R.H + 4, 0, 20])
    out = emu.template_pem_crops(rgb.contiguous(), mask.contiguous(), bad, R.S, flag, pre.MEAN, pre.STD)
    assert torch.equal(out[1:], got[1:]) and torch.equal(out[0, :, 0, 0], (torch.zeros(3) - torch.tensor(pre.MEAN)) / torch.tensor(pre.STD))


@pytest.mark.parametrize("flag", [True, False])
def test_pem_template_inputs_on_the_kernels(emu, case, flag, monkeypatch):
    kw = dict(n_sample=R.N_SAMPLE, img_size=R.S, rgb_mask_flag=flag)
    args = [case[k][GOOD] for k in ("rgb", "mask", "xyz")]
    want = R.pem_templates(*[a.numpy()[None] for a in args], case["keys"][GOOD].numpy()[None], **kw)
    with policy.use(strict="1"):
        got = ob.pem_template_inputs(*args, keys=case["keys"][GOOD], **kw)
    assert not policy.library_branch_hits()
    for g_, w_ in zip(got, want):
        for v in range(len(GOOD)):
            np.testing.assert_array_equal(g_[v].numpy(), w_[v], err_msg=f"view {GOOD[v]}")
    rng_got = ob.pem_template_inputs(*args, rng=np.random.RandomState(3), **kw)
    rng_want = R.pem_templates(*[a.numpy()[None] for a in args], rng=np.random.RandomState(3), **kw)
    for g_, w_ in zip(rng_got, rng_want):
        np.testing.assert_array_equal(torch.cat(g_).numpy(), np.concatenate(w_))
    monkeypatch.setenv("S6D_ONBOARD", "library")
    lib = ob.pem_template_inputs(*args, keys=case["keys"][GOOD], **kw)
    assert all(torch.equal(a, b) for x, y in zip(got, lib) for a, b in zip(x, y))
    assert ("onboarding.pem_template_inputs", "policy") in policy.library_branch_hits()
    with policy.use(strict="1"), pytest.raises(policy.StrictError, match="onboarding.pem_template_inputs"):
        ob.pem_template_inputs(*args, keys=case["keys"][GOOD], **kw)


def test_empty_view_raises_on_the_kernel_path(emu, case):
    pick = [0, R.EMPTY_VIEW]
    with pytest.raises(ValueError, match=r"view\(s\) 1 of object 0"):
        ob.pem_template_inputs(case["rgb"][pick], case["mask"][pick], case["xyz"][pick], keys=case["keys"][pick], n_sample=32, img_size=R.S)
    with pytest.raises(ValueError, match=r"template view\(s\) \[1\]"):
        ob.ism_template_inputs(case["rgb"][pick], case["mask"][pick], R.S)


# ---- the sampler at the template size: one 96 x 128 view, n_sample = 5000 ---------------------------------------------------------
def _sampler_rows():
    g = torch.Generator().manual_seed(12)
    L = 96 * 128
    n = torch.tensor([L, 5000, 4999, L, 9216, L])
    keys = torch.rand(len(n), L, generator=g)
    keys[3] = (keys[3] * 1e4).floor() / 1e4                          # ties: the position decides
    keys[4] = (keys[4] * 1e4).floor() / 1e4
    keys[5] = torch.where(keys[5] < 0.9, torch.full_like(keys[5], 0.25), keys[5])      # 90 % of the keys equal: more than 8192 candidates
    return n, keys.contiguous()


def test_sampler_kernel_serves_5000_samples(emu):
    n, keys = _sampler_rows()
    idx, overflow = emu.pem_sample_indices(keys, n, 5000)
    assert overflow.tolist() == [0, 0, 0, 0, 0, 1]                   # the duplicated row is flagged, its indices not written
    lib = pre._keyed_indices_library(n, keys, 5000)
    for r in range(5):
        want = o.sample_indices(int(n[r]), 5000, keys[r].numpy())
        np.testing.assert_array_equal(idx[r].numpy(), want, err_msg=f"row {r}")
        assert torch.equal(idx[r], lib[r])
    assert len(set(idx[0].tolist())) == 5000 and len(set(idx[1].tolist())) < 5000          # without / with replacement
    np.testing.assert_array_equal(lib[5].numpy(), o.sample_indices(int(n[5]), 5000, keys[5].numpy()))
    # sizes the entry has always served: the kernel and the answers they have always had
    idx512, ov = emu.pem_sample_indices(keys, n, 512)
    assert ov.tolist() == [0] * 5 + [1]                             # (row 5: 11000 equal keys exceed the 4096 candidates too)
    assert torch.equal(idx512[:5], pre._keyed_indices_library(n, keys, 512)[:5])
    np.testing.assert_array_equal(idx512[0].numpy(), np.argsort(keys[0].numpy(), kind="stable")[:512])
    with pytest.raises(Exception, match="s6d_pem_sample_indices_f32"):
        emu.pem_sample_indices(keys, n, emu.PEM_SAMPLE_MAX + 1)


def test_duplicated_keys_fall_back_through_the_public_call(emu):
    """A whole-view mask of 96 x 128 (crop 96 x 96 = 9216 points), 5000 samples, keys that overflow the in-LDS selection."""
    n, keys = _sampler_rows()
    r = np.random.RandomState(3)
    rgb = r.randint(0, 256, (2, 96, 128, 3)).astype(np.uint8)
    xyz = (r.standard_normal((2, 96, 128, 3)) * 50).astype(np.float32)
    mask = np.full((2, 96, 128), 255, np.uint8)
    k = keys[[0, 5]].contiguous()
    seen = []
    real = emu.pem_sample_indices
    emu.pem_sample_indices = lambda *a, **kw: (seen.append(1), real(*a, **kw))[1]
    try:
        got = ob.pem_template_inputs(torch.from_numpy(rgb), torch.from_numpy(mask), torch.from_numpy(xyz), keys=k, n_sample=5000, img_size=R.S)
    finally:
        emu.pem_sample_indices = real
    assert seen
    want = R.pem_templates(rgb[None], mask[None], xyz[None], k.numpy()[None], n_sample=5000)
    for g_, w_ in zip(got, want):
        for v in range(2):
            np.testing.assert_array_equal(g_[v].numpy(), w_[v])


@pytest.mark.parametrize("normalize", [False, True])
def test_ism_crops_kernel(emu, case, normalize, monkeypatch):
    rgb, mask = case["rgb"][GOOD], case["mask"][GOOD]
    with policy.use(strict="1"):
        tem, msk = ob.ism_template_inputs(rgb, mask, R.S, normalize)
    want_t, want_m = R.ism_templates(rgb.numpy(), mask.numpy(), R.S, normalize)
    assert torch.equal(tem, want_t) and torch.equal(msk, want_m)
    mean, std = torch.tensor(ob.RGB_MEAN), torch.tensor(ob.RGB_STD)
    pad = ((torch.zeros(3) - mean) / std)[:, None].expand(3, R.S) if normalize else torch.zeros(3, R.S)
    assert torch.equal(tem[2][:, :, 0], pad) and torch.equal(tem[10][:, 0, :], pad)          # 7 x 5 and 10 x 90 tight boxes: padded
    assert (msk[R.GREY_VIEW] == torch.tensor(128 / 255).float()).any()
    monkeypatch.setenv("S6D_ONBOARD", "library")
    lib_t, lib_m = ob.ism_template_inputs(rgb, mask, R.S, normalize)
    assert torch.equal(lib_t, tem) and torch.equal(lib_m, msk)
