"""Pins oracle/pn2_oracle.c (the comparand of the device PointNet++ kernels, rows a13 / a19) to the REFERENCE'S OWN kernels:
oracle/build_ref.py compiles sampling_gpu.cu / ball_query_gpu.cu / group_points_gpu.cu from the reference tree for the host
(oracle/_ref/, emulated CUDA runtime) and every case of tests/test_gpu_pn2.py is run through both, bit for bit.  The reference
kernels' outputs for these cases are stored in tests/golden/pn2_ref.npz (oracle/gen_golden.py pn2_ref; the large ones as a
SHA-256 of their bits), so the comparison runs
on every host; where oracle/_ref is built (or the reference tree is there to build it) the live kernels are run as well and must
still equal the stored outputs.

What the reference source does not decide is the contraction of  a*a + b*b + c*c  (nvcc --fmad): the restatement carries three
spellings and is held to the two a host compiler can produce from the unmodified source (none; LLVM's).  The third -- nvcc's
default, fma(c,c, fma(b,b, a*a)), the one the product kernels spell -- differs from them only in the rounding of one product;
`test_where_the_contraction_spellings_diverge` measures how often that reaches an OUTPUT index."""
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

from oracle import pn2 as opn2
from oracle import pn2_ref
from tests import util
from tests.test_gpu_pn2 import _cloud

LIVE = (pn2_ref.available("off") and pn2_ref.available("fast")) or os.path.isdir(os.environ.get("S6D_REFERENCE_ROOT", "/root/reference"))
PAIRS = [(2, "off"), (1, "fast")]          # (pn2_oracle.c contraction mode, _ref build)

FPS_CASES = [(2, 2048, 196, False), (3, 2048, 196, True), (1, 700, 64, True), (2, 64, 64, False), (1, 1, 1, False),
             (2, 3000, 128, True), (1, 4096, 200, False), (1, 5000, 60, True), (1, 37, 20, False), (1, 514, 100, True)]
BQ_CASES = [(2, 2048, 2048, 0.1, 32), (2, 2048, 2048, 0.2, 64), (1, 300, 50, 0.2, 16), (1, 100, 7, 0.5, 128), (1, 5000, 100, 0.05, 8)]


def _fps_input(B, N, dup):
    return _cloud(B, N, 100 + N, dup)


def _bq_input(B, N, M):
    x = _cloud(B, N, 7 + N, dup=True)
    return (x[:, :M].contiguous() if M <= N else _cloud(B, M, 3)), x


def _tie_input():
    y = torch.zeros(1, 600, 3)
    y[0, 520] = 1.0
    y[0, 9] = 1.0
    return y


def _gather_group_input():
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(3, 37, 500, generator=g)
    idx = torch.randint(0, 500, (3, 196), generator=g, dtype=torch.int32)
    gi = torch.randint(0, 500, (3, 60, 16), generator=g, dtype=torch.int32)
    return feats, idx, gi


def reference_outputs():
    """{name: output} of the reference kernels (oracle/_ref) on every input of this module: what tests/golden/pn2_ref.npz holds
    (written by oracle/gen_golden.py pn2_ref)."""
    out = {}
    for _, v in PAIRS:
        for B, N, M, dup in FPS_CASES:
            out[f"fps_{B}_{N}_{M}_{int(dup)}_{v}"] = pn2_ref.furthest_point_sampling(_fps_input(B, N, dup), M, v)
        out[f"fps_temp_{v}"] = pn2_ref.furthest_point_sampling(_cloud(2, 2048, 77), 196, v, with_temp=True)[1]
        out[f"fps_tie_{v}"] = pn2_ref.furthest_point_sampling(_tie_input(), 3, v)
        for B, N, M, r, ns in BQ_CASES:
            q, x = _bq_input(B, N, M)
            out[f"bq_{B}_{N}_{M}_{r}_{ns}_{v}"] = pn2_ref.ball_query(q, x, r, ns, v)
            out[f"bq_far_{B}_{N}_{M}_{r}_{ns}_{v}"] = pn2_ref.ball_query(torch.full((1, 4, 3), 50.0), x[:1], 0.2, 8, v)
    feats, idx, gi = _gather_group_input()
    out["gather"] = pn2_ref.gather_points(feats, idx)
    out["group"] = pn2_ref.group_points(feats, gi)
    return out


SMALL = 1024        # outputs of at most this many elements are stored whole; a larger one as the SHA-256 of its dtype, shape and bytes


def fingerprint(t):
    a = np.ascontiguousarray(t.numpy())
    return np.frombuffer(hashlib.sha256(f"{a.dtype}{a.shape}".encode() + a.tobytes()).digest(), np.uint8)


def golden_arrays(outputs):
    """What tests/golden/pn2_ref.npz stores of reference_outputs(): `name` -> the array, or `name`_sha256 -> its fingerprint."""
    return {(k if v.numel() <= SMALL else k + "_sha256"): (v.numpy() if v.numel() <= SMALL else fingerprint(v)) for k, v in outputs.items()}


@functools.lru_cache(maxsize=None)
def _golden():
    return util.golden("pn2_ref.npz")


def _equals_reference(name, t, live):
    """`t` has the bits of the reference kernels' output `name` as tests/golden/pn2_ref.npz holds it (whole or as a fingerprint);
    where the kernels are at hand, `live()` runs them and must give the same bits."""
    g = _golden()

    def same(x):
        if name + "_sha256" in g:
            return np.array_equal(fingerprint(x), g[name + "_sha256"])
        return torch.equal(x, torch.from_numpy(g[name]))
    if LIVE:
        assert same(live()), f"{name}: the reference kernel no longer gives tests/golden/pn2_ref.npz"
    return same(t)


@pytest.mark.parametrize("mode,variant", PAIRS)
@pytest.mark.parametrize("B,N,M,dup", FPS_CASES)
def test_fps_restatement_equals_reference_kernel(B, N, M, dup, mode, variant):
    x = _fps_input(B, N, dup)
    with opn2.contraction(mode):
        mine = opn2.furthest_point_sampling(x, M)
    assert _equals_reference(f"fps_{B}_{N}_{M}_{int(dup)}_{variant}", mine, lambda: pn2_ref.furthest_point_sampling(x, M, variant))


def test_distance_bits_follow_the_contraction():
    """The kernel's `temp` array (running minimum squared distances) carries the float bits the contraction decides: the
    restatement's equals the reference kernel's in both builds, and the three spellings do differ there (so the index-level
    agreement of `test_where_the_contraction_spellings_diverge` is a statement about robustness, not about identical code)."""
    x = _cloud(2, 2048, 77)
    temps = {}
    for mode in (0, 1, 2):
        with opn2.contraction(mode):
            temps[mode] = opn2.furthest_point_sampling_with_temp(x, 196)[1]
    for mode, variant in PAIRS:
        assert _equals_reference(f"fps_temp_{variant}", temps[mode],
                                 lambda: pn2_ref.furthest_point_sampling(x, 196, variant, with_temp=True)[1])
    assert not torch.equal(temps[0], temps[1]) and not torch.equal(temps[0], temps[2]) and not torch.equal(temps[1], temps[2])
    assert (temps[0] - temps[2]).abs().max() <= 2e-7 * temps[2].abs().max()


def test_fps_tie_break_of_the_reference_tree():
    """Equal distances: the reference's shared-memory tree keeps the lower SLOT (bit-reversed order of thread ids), not the
    lower index -- the rule the device kernel's 64-bit keys encode (tests/test_gpu_pn2.py::test_fps_tie_break_rule)."""
    y = _tie_input()
    for mode, variant in PAIRS:
        with opn2.contraction(mode):
            assert _equals_reference(f"fps_tie_{variant}", opn2.furthest_point_sampling(y, 3),
                                     lambda: pn2_ref.furthest_point_sampling(y, 3, variant))


@pytest.mark.parametrize("mode,variant", PAIRS)
@pytest.mark.parametrize("B,N,M,r,ns", BQ_CASES)
def test_ball_query_restatement_equals_reference_kernel(B, N, M, r, ns, mode, variant):
    q, x = _bq_input(B, N, M)
    with opn2.contraction(mode):
        mine = opn2.ball_query(q, x, r, ns)
    assert _equals_reference(f"bq_{B}_{N}_{M}_{r}_{ns}_{variant}", mine, lambda: pn2_ref.ball_query(q, x, r, ns, variant))
    far = torch.full((1, 4, 3), 50.0)
    assert _equals_reference(f"bq_far_{B}_{N}_{M}_{r}_{ns}_{variant}", torch.zeros(1, 4, 8, dtype=torch.int32),
                             lambda: pn2_ref.ball_query(far, x[:1], 0.2, 8, variant))


def test_gather_and_group_equal_reference_kernels():
    feats, idx, gi = _gather_group_input()
    assert _equals_reference("gather", opn2.gather_points(feats, idx), lambda: pn2_ref.gather_points(feats, idx))
    assert _equals_reference("group", opn2.group_points(feats, gi), lambda: pn2_ref.group_points(feats, gi))


def test_where_the_contraction_spellings_diverge():
    """The three spellings round ONE product differently (a relative 6e-8 on a squared distance).  An FPS index changes only when
    that flips a comparison between near-tied candidates, a ball-query index only when a neighbour sits within 6e-8 of the
    radius.  Over the benched shapes (2048 points, 196 samples; radius 0.1 / 0.2 queries) the divergence is counted and
    written to gpurun_out/pn2_contraction.json (copied to profiles/r03_pn2_contraction.json); the assertion is that it stays
    a rare event, i.e. that the product's dependence on the unpinned nvcc flag is bounded by it."""
    import json
    clouds = torch.cat([_cloud(8, 2048, 1000 + s) for s in range(4)])          # 32 clouds
    res = {}
    for mode in (0, 1, 2):
        with opn2.contraction(mode):
            res[mode] = (opn2.furthest_point_sampling(clouds, 196), opn2.ball_query(clouds[:4, :512].contiguous(), clouds[:4], 0.1, 32),
                         opn2.ball_query(clouds[:4, :512].contiguous(), clouds[:4], 0.2, 64))
    rep = {}
    for other, name in ((1, "llvm"), (2, "none")):
        fps_rows = (res[0][0] != res[other][0]).any(1)
        rep[name] = dict(fps_clouds_differing=int(fps_rows.sum()), fps_clouds=int(clouds.shape[0]),
                         fps_first_divergence=[int((res[0][0][b] != res[other][0][b]).nonzero()[0]) for b in fps_rows.nonzero().flatten().tolist()],
                         ball_query_r01_entries_differing=int((res[0][1] != res[other][1]).sum()), ball_query_r01_entries=int(res[0][1].numel()),
                         ball_query_r02_entries_differing=int((res[0][2] != res[other][2]).sum()), ball_query_r02_entries=int(res[0][2].numel()))
    try:
        os.makedirs("gpurun_out", exist_ok=True)
        json.dump(rep, open("gpurun_out/pn2_contraction.json", "w"), indent=1)
    except OSError:
        pass
    for name, r in rep.items():
        assert r["fps_clouds_differing"] <= r["fps_clouds"] // 4, rep
        assert r["ball_query_r01_entries_differing"] <= r["ball_query_r01_entries"] // 1000, rep
