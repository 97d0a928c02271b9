"""The restatements of tests/ism_ref.py checked on the host, before a kernel test relies on them: no GPU, no emulator."""
import ast
from fractions import Fraction

import numpy as np
import pytest
import torch

from sam6d_amd.utils import synth
from tests import ism_ref, util


@pytest.mark.parametrize("name", ["ism_scoring.npz", "ism_scoring_p128.npz"])
def test_project_ref_gives_the_reference_pixels_bit_for_bit(name):
    """project_ref fed the golden's own translation reproduces `image_uv` of the reference run: the operation order and the
    conversion rule written out there are the pinned run's."""
    g = util.golden(name)
    c = ast.literal_eval(str(g["case"]))
    inp = synth.ism_inputs(P=c["P"], O=c["O"], T=c["T"], seed=c["seed"])
    H, W = inp["depth"].shape
    R = inp["poses"][torch.from_numpy(g["best_template"]).long(), :3, :3].numpy()
    pc = inp["pointcloud"][torch.from_numpy(g["pred_obj"]).long()].numpy()
    uv, bbox = ism_ref.project_ref(pc, R, g["translation"], inp["K"].to(torch.float32).numpy(), H, W)
    assert uv.shape == g["image_uv"].shape and len(uv) > 0
    assert np.array_equal(uv, g["image_uv"])
    assert np.array_equal(bbox, np.concatenate((g["image_uv"].min(1), g["image_uv"].max(1)), -1))


def test_fma32_rounds_once():
    """fma32 against exact rational arithmetic, on operands built to sit on float32 rounding ties of the float64 sum (where the
    plain float64 emulation rounds twice) and on random ones."""
    f = np.float32
    rng = np.random.default_rng(0)
    a = rng.standard_normal(2000).astype(f)
    b = rng.standard_normal(2000).astype(f)
    c = (rng.standard_normal(2000) * 10.0 ** rng.integers(-8, 8, 2000)).astype(f)
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 sits ON a float32 tie; c = +-2^-80 moves the exact sum off it, which a float64 sum loses
    #   (it would then round the tie to even: 1 + 2^-11, wrong for +2^-80)
    # 2^-24 (1 - 2^-46) + (1 + 2^-23) lies just BELOW the tie between 1 + 2^-23 and 1 + 2^-22; float64 rounds it onto the tie, then to even
    # 2^-24 * 1 + 1 is an exact tie: 1 (even)
    x = 1 + 2.0 ** -12
    a = np.concatenate((a, f([x, x, 2.0 ** -12 * (1 + 2.0 ** -23), 2.0 ** -24])))
    b = np.concatenate((b, f([x, x, 2.0 ** -12 * (1 - 2.0 ** -23), 1.0])))
    c = np.concatenate((c, f([2.0 ** -80, -2.0 ** -80, 1 + 2.0 ** -23, 1.0])))
    got = ism_ref.fma32(a, b, c)
    plain = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f)
    assert (plain != got).sum() >= 2                        # the constructed cases do separate the two emulations
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = f(float(exact))                                # float(Fraction) rounds once to float64: only a neighbourhood guess
        cands = {float(lo), float(np.nextafter(lo, f(np.inf))), float(np.nextafter(lo, f(-np.inf)))}
        best = min(cands, key=lambda v: (abs(Fraction(v) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert float(got[i]) == best, (i, a[i], b[i], c[i], got[i], best)


def test_to_int_pinned_is_the_host_conversion():
    """The conversion rule as written out equals what `.to(torch.int)` gives on this host for in-range values, and is INT_MIN for
    everything else (checked against torch only where C++ defines the cast: the rest is the statement of the pinned run)."""
    x = np.array([0.0, -0.0, 0.99, -0.99, 1.5, -1.5, 639.99, 2147483520.0, -2147483648.0, 1e-30], np.float32)
    assert np.array_equal(ism_ref.to_int_pinned(x), torch.from_numpy(x).to(torch.int).numpy().astype(np.int64))
    bad = np.array([np.inf, -np.inf, np.nan, 3e9, -3e9, 2147483648.0], np.float32)
    assert (ism_ref.to_int_pinned(bad) == -2 ** 31).all()
