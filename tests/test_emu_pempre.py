"""The PEM sampler kernel (csrc/s6d_pempre.hip) on the emulator against the library formulation it replaces (the top-k over
64-bit composite keys in sam6d_amd/pem/preprocess.py): identical indices, ties resolved by position, duplicated keys flagged."""
import numpy as np
import torch

from sam6d_amd.pem import preprocess as pre
from tests import test_gpu_pem_pre as T


def _lib_path(n, keys, n_sample, monkeypatch):
    monkeypatch.setenv("S6D_PEM_SAMPLER", "library")                 # the top-k formulation (the kernel is the default on the device)
    try:
        return pre._keyed_indices(n, keys, n_sample)
    finally:
        monkeypatch.delenv("S6D_PEM_SAMPLER")


def test_sampler_kernel_equals_the_library_path(emu, monkeypatch):
    g = torch.Generator().manual_seed(0)
    L, ns = 40000, 512
    n = torch.tensor([0, 1, 100, 512, 513, 600, 1024, 5000, 40000, 2049])
    keys = torch.rand(len(n), L, generator=g)
    keys[5] = (keys[5] * 300).floor() / 300                          # ties among 600 keys: the position decides
    keys[7, :5000] = (keys[7, :5000] * 1e4).floor() / 1e4
    want = _lib_path(n, keys, ns, monkeypatch)
    idx, overflow = emu.pem_sample_indices(keys, n, ns)
    assert overflow.tolist() == [0] * len(n)
    assert torch.equal(idx, want)
    # the selected positions are what a stable argsort gives
    row = 8
    np.testing.assert_array_equal(idx[row].numpy(), np.argsort(keys[row].numpy(), kind="stable")[:ns])
    # through observed_inputs' switch as well
    monkeypatch.setenv("S6D_PEM_SAMPLER", "kernel")
    assert torch.equal(pre._keyed_indices(n, keys, ns), want)


def test_heavily_duplicated_keys_are_flagged_and_fall_back(emu, monkeypatch):
    g = torch.Generator().manual_seed(1)
    n = torch.tensor([30000, 30000])
    keys = torch.rand(2, 30000, generator=g)
    keys[1] = (keys[1] * 4).floor() / 4                              # four distinct values: 7500 keys share the smallest
    want = _lib_path(n, keys, 2048, monkeypatch)
    idx, overflow = emu.pem_sample_indices(keys, n, 2048)
    assert overflow.tolist() == [0, 1] and torch.equal(idx[0], want[0])
    monkeypatch.setenv("S6D_PEM_SAMPLER", "kernel")
    assert torch.equal(pre._keyed_indices(n, keys, 2048), want)     # the switch falls back to the library path for the frame


def test_full_frame_with_the_kernel_sampler_matches_the_oracle(emu, monkeypatch):
    from oracle import pem_pre as opre
    from sam6d_amd.utils import synth
    monkeypatch.setenv("S6D_PEM_SAMPLER", "kernel")
    inp = synth.pem_pre_inputs(P=8, seed=3)
    kw = dict(radius=0.12, n_sample=512, img_size=224, min_points=32, min_inliers=4, radius_factor=1.2)
    ref = opre.preprocess_frame(inp["image"], inp["depth"].numpy(), inp["K"].numpy(), inp["masks"].numpy(),
                                keys=inp["keys"].numpy(), **kw)
    out = pre.observed_inputs(torch.from_numpy(inp["image"]), inp["depth"], inp["K"], inp["masks"], keys=inp["keys"], **kw)
    assert out["kept"].tolist() == ref["kept"].tolist()
    np.testing.assert_array_equal(out["pts"].numpy(), ref["pts"])
    np.testing.assert_array_equal(out["rgb_choose"].numpy(), ref["rgb_choose"])


_frame = T._frame


def test_kernel_path_of_the_whole_preprocessing_matches_the_oracle(emu, monkeypatch):
    """S6D_PEM_PRE=kernels: compaction + back-projection, sequential centroid, radius filter (and the sampler kernel) against
    the oracle's per-detection loop -- bit-identical points, crops, indices and survivors, also at the radii whose sphere cuts
    through dense points (where the default path's float64-accumulated centroid flips boundary points)."""
    from oracle import pem_pre as opre
    monkeypatch.setenv("S6D_PEM_PRE", "kernels")                     # implies the sampler kernel
    called = []
    real = emu.pem_sample_indices
    monkeypatch.setattr(emu, "pem_sample_indices", lambda *a, **k: (called.append(1), real(*a, **k))[1])
    inp, args = _frame()
    kw = dict(n_sample=512, img_size=224, min_points=32, min_inliers=4, radius_factor=1.2)
    for radius in (0.12, np.array([0.12, 0.03, 0.5, 0.12, 0.06, 0.2, 0.07, 0.01])):
        ref = opre.preprocess_frame(inp["image"], inp["depth"].numpy(), inp["K"].numpy(), inp["masks"].numpy(), radius,
                                    keys=inp["keys"].numpy(), **kw)
        r = torch.from_numpy(radius) if isinstance(radius, np.ndarray) else radius
        out = pre.observed_inputs(*args, r, keys=inp["keys"], **kw)
        assert out["kept"].tolist() == ref["kept"].tolist() and len(ref["kept"]) >= 6
        np.testing.assert_array_equal(out["bbox"].numpy(), ref["bbox"])
        np.testing.assert_array_equal(out["pts"].numpy(), ref["pts"])
        np.testing.assert_array_equal(out["rgb_choose"].numpy(), ref["rgb_choose"])
        np.testing.assert_array_equal(out["rgb"].numpy(), ref["rgb"])
    assert len(called) == 2
    # numpy-compatible draws on the kernel path too
    ref = opre.preprocess_frame(inp["image"], inp["depth"].numpy(), inp["K"].numpy(), inp["masks"].numpy(), 0.12,
                                rng=np.random.RandomState(5), **kw)
    out = pre.observed_inputs(*args, 0.12, rng=np.random.RandomState(5), **kw)
    np.testing.assert_array_equal(out["pts"].numpy(), ref["pts"])


def test_kernel_path_with_no_survivor_and_with_empty_masks(emu, monkeypatch):
    monkeypatch.setenv("S6D_PEM_PRE", "kernels")
    inp, args = _frame(P=3, seed=5)
    out = pre.observed_inputs(args[0], args[1] * 0, args[2], args[3], 0.1, inp["keys"])
    assert out["pts"].shape[0] == 0 and out["rgb"].shape == (0, 3, 224, 224) and out["kept"].numel() == 0
    masks = args[3].clone()
    masks[1] = False                                                 # one detection without a single pixel
    out = pre.observed_inputs(args[0], args[1], args[2], masks, 0.3, inp["keys"], n_sample=256)
    assert 1 not in out["kept"].tolist() and out["pts"].shape[1:] == (256, 3)


# ---- the kernels called directly: the bodies are those of tests/test_gpu_pem_pre.py, here on the emulator ----------------------------
def test_mask_boxes_kernel_equals_the_library_ops(emu):
    T.mask_boxes_body(emu, "cpu")


def test_crops_kernel_equals_the_library_statement(emu):
    T.crops_library_body(emu, "cpu")


def test_crops_follow_the_cv2_restatement_at_every_ratio(emu):
    T.crops_cv2_body(emu, "cpu")


def test_compact_cloud_kernel_in_crop_order_with_the_reference_back_projection(emu):
    T.compact_cloud_body(emu, "cpu")


def test_compaction_skips_a_box_outside_the_frame_or_larger_than_a_slot(emu):
    T.compact_guards_body(emu, "cpu")


def test_crop_of_a_box_outside_the_frame_is_a_black_crop(emu):
    T.crops_guard_body(emu, "cpu")


def test_crop_resize_pad_source_outside_the_frame_is_padding(emu):
    T.crop_resize_pad_guard_body(emu, "cpu")
