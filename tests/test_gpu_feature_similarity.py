"""ops.cosine_similarity (s6d_cosine_similarity_f32, csrc/s6d_sim.hip) -- compute_feature_similarity of the matching heads
(model_utils.py:114-136, cosine, normalize_feat=True) as one kernel: against a float64 restatement with a bound derived from the
roundings, on hostile rows, for batch invariance and transpose symmetry bit for bit, into the sampling head on a known-answer case,
through CoarsePointMatching under strict mode, and its argument checks.  The bodies take `ops` so that
tests/test_emu_feature_similarity.py runs them on the host build at the small shapes."""
import functools

import pytest
import torch

from oracle import pem as opem
from sam6d_amd.utils import synth

pytestmark = pytest.mark.gpu

TEMP = 0.1
TEMP32 = torch.tensor(TEMP, dtype=torch.float32).item()          # what the kernel is given: the scalar rounded to float32
# (B, M1, M2, C).  (3,197,197,256): the model's shape, a tail of 5 on both sides; (2,37,21,32): tails on both sides; (1,16,16,16): one
# tile exactly; (1,17,15,16): one over / one under a tile; (2,5,300,64): more than 256 columns, several chunks of f2;
# (1,2049,130,256): many row panels, the height of the fine fallback
SHAPES = [(3, 197, 197, 256), (2, 37, 21, 32), (1, 16, 16, 16), (1, 17, 15, 16), (2, 5, 300, 64), (1, 2049, 130, 256)]
SMALL_SHAPES = SHAPES[1:5]                                       # what the host build runs


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from sam6d_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _features(B, M1, M2, C):
    """f1 random; row j of f2 a noisy copy of row j % M1 of f1 (dominant entries near 1 / temp); f2[:, 0] == f1[:, 0] exactly (an
    identical pair: |a| = 1 / temp up to rounding).  Computed once per shape, only read."""
    g = torch.Generator().manual_seed(1000 * M1 + 10 * M2 + C + B)
    f1 = torch.randn(B, M1, C, generator=g)
    f2 = f1[:, torch.arange(M2) % M1] + 0.2 * torch.randn(B, M2, C, generator=g)
    f2[:, 0] = f1[:, 0]
    return f1.contiguous(), f2.contiguous()


def _unit64(f):
    return f.double() / f.double().norm(dim=2, keepdim=True).clamp(min=1e-12)


def _ref64(f1, f2):
    """The float64 statement x / max(|x|, 1e-12), matmul, / temp -- and the bound (2C + 8) 2^-24 (|x^1| . |x^2|^T) / temp: every
    term of the dot product carries the roundings of the norm sums (C / 2 each after the square root), the square roots and
    divisions of both sides and a C-term fma chain; one more division by temp."""
    x1, x2 = _unit64(f1), _unit64(f2)
    C = f1.shape[2]
    ref = x1 @ x2.transpose(1, 2) / TEMP32
    bound = (2 * C + 8) * 2.0 ** -24 * (x1.abs() @ x2.abs().transpose(1, 2)) / TEMP32
    return ref, bound


@functools.lru_cache(maxsize=None)
def _case(B, M1, M2, C):
    f1, f2 = _features(B, M1, M2, C)
    return (f1, f2) + _ref64(f1, f2)


def check_vs_float64(ops, B, M1, M2, C):
    """Every element within the derived bound of the float64 statement; the identical pair gives |a| ~ 1 / temp.
    Worst fraction of the bound measured on the MI355X: see profiles/coarse_similarity.md; printed on every run."""
    f1, f2, ref, bound = _case(B, M1, M2, C)
    a = ops.cosine_similarity(f1.cuda(), f2.cuda(), TEMP).cpu()
    assert a.shape == (B, M1, M2) and a.dtype == torch.float32
    assert torch.isfinite(a).all()
    frac = ((a.double() - ref).abs() / bound).max().item()
    print(f"[feature_similarity {B}x{M1}x{M2}x{C}] worst fraction of the bound {frac:.4f}, max |a| {a.abs().max().item():.6f}")
    assert frac <= 1.0, frac
    assert abs(a[0, 0, 0].item() - 1.0 / TEMP32) < 1e-4


def check_hostile_rows(ops, B, M1, M2, C):
    """A zero row, a row scaled by 2^70 (its squares overflow float32) and a row scaled by 2^-70 on each side: exact zeros for the
    first two (as torch's CPU statement gives), the float64 statement with its 1e-12 divisor for the third, no NaN / inf anywhere."""
    f1, f2 = (t.clone() for t in _features(B, M1, M2, C))
    z1, big1, tiny1 = 1, 2, 3
    z2, big2, tiny2 = M2 - 1, M2 - 2, M2 - 3
    f1[:, z1] = 0
    f2[:, z2] = 0
    f1[:, big1] *= 2.0 ** 70
    f2[:, big2] *= 2.0 ** 70
    f1[:, tiny1] *= 2.0 ** -70
    f2[:, tiny2] *= 2.0 ** -70
    a = ops.cosine_similarity(f1.cuda(), f2.cuda(), TEMP).cpu()
    assert torch.isfinite(a).all()
    lib = torch.nn.functional.normalize(f1, p=2, dim=2) @ torch.nn.functional.normalize(f2, p=2, dim=2).transpose(1, 2) / TEMP
    assert (lib[:, big1] == 0).all() and (lib[:, :, big2] == 0).all(), "torch's CPU statement gives zeros for the overflowing rows"
    for r in (z1, big1):
        assert (a[:, r] == 0).all(), r
    for c in (z2, big2):
        assert (a[:, :, c] == 0).all(), c
    ref, bound = _ref64(f1, f2)
    keep = torch.ones(B, M1, M2, dtype=torch.bool)
    keep[:, big1] = False                                         # float64 does not overflow there: compared with 0 above
    keep[:, :, big2] = False
    frac = ((a.double() - ref).abs() / bound.clamp(min=1e-300))[keep & (bound > 0)].max().item()
    print(f"[feature_similarity {B}x{M1}x{M2}x{C}] hostile rows: worst fraction of the bound {frac:.4f}; "
          f"tiny row max |a| {a[:, tiny1].abs().max().item():.3e}")
    assert frac <= 1.0, frac
    assert a[:, tiny1].abs().max() > 0 and a[:, :, tiny2].abs().max() > 0          # divided by 1e-12, not flushed away


def check_batch_invariance(ops, M1, M2, C):
    """Instance b of a B = 3 call equals the same instance run at B = 1, bit for bit."""
    f1, f2 = (t.cuda() for t in _features(3, M1, M2, C))
    a = ops.cosine_similarity(f1, f2, TEMP).cpu()
    for b in range(3):
        one = ops.cosine_similarity(f1[b:b + 1].contiguous(), f2[b:b + 1].contiguous(), TEMP).cpu()
        assert torch.equal(one[0], a[b]), b


def check_transpose_symmetry(ops, B, M1, M2, C):
    """cosine_similarity(f2, f1) is the transpose of cosine_similarity(f1, f2) bit for bit: the same terms in the same k order."""
    f1, f2 = (t.cuda() for t in _features(B, M1, M2, C))
    a = ops.cosine_similarity(f1, f2, TEMP).cpu()
    t = ops.cosine_similarity(f2, f1, TEMP).cpu()
    assert t.shape == (B, M2, M1)
    assert torch.equal(t.transpose(1, 2), a)


def check_into_sampling_head(ops, B, N, C, n1, n2):
    """ops.coarse_sample(ops.cosine_similarity(f1, f2, 0.1), u) on the known-answer case of
    tests/test_gpu_pose.py::test_coarse_Rt_kernel_chain_vs_oracle (p1 = p2 Rgt^T + t, features that identify the correspondence):
    solvers.coarse_Rt recovers Rgt within that test's 1e-2 and the labels w1 are oracle.pem.soft_assignment's of the float64
    similarity."""
    from sam6d_amd.pem import solvers
    g = torch.Generator().manual_seed(N + n1)
    p2 = torch.randn(B, N, 3, generator=g) * 0.4
    Rgt = synth.random_rotations(B, g)
    tgt = 0.1 * torch.randn(B, 3, generator=g)
    p1 = p2 @ Rgt.transpose(1, 2) + tgt[:, None, :]
    f1 = torch.nn.functional.normalize(torch.randn(B, N + 1, C, generator=g), dim=2)      # row 0: the background token
    f2 = f1 + 0.2 * torch.randn(B, N + 1, C, generator=g)
    model = p2[:, : max(N // 2, 16)].contiguous()
    u = torch.rand(B, 3 * n1, generator=g)
    atten = ops.cosine_similarity(f1.cuda(), f2.cuda(), TEMP)
    _, w1 = ops.coarse_sample(atten, u.cuda())
    _, w1_ref, _ = opem.soft_assignment(_ref64(f1, f2)[0])
    assert torch.equal(w1.cpu(), w1_ref.float())
    R, _ = solvers.coarse_Rt(atten, p1.cuda(), p2.cuda(), model.cuda(), u.cuda(), n1, n2)
    err = (R.cpu() - Rgt).norm(dim=(1, 2)).max().item()
    print(f"[feature_similarity -> coarse_Rt {B}x{N + 1}x{N + 1}x{C}] |R - Rgt| max {err:.3e}")
    assert err < 1e-2, err


def check_arguments(ops):
    """The wrapper refuses host tensors, other dtypes, operands that disagree in B or C and temp = 0; the entry point answers
    S6D_EUNSUPPORTED (-3) for C = 6 and C = 516 and S6D_OK for B = 0; nothing is launched (the output keeps its fill)."""
    f1, f2 = (t.cuda() for t in _features(2, 37, 21, 32))
    if not torch.zeros(1).is_cuda:                                               # (the host build's fixture makes every tensor claim the device)
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            ops.cosine_similarity(f1.cpu(), f2.cpu(), TEMP)
    with pytest.raises(RuntimeError, match="float"):
        ops.cosine_similarity(f1.double(), f2.double(), TEMP)
    with pytest.raises(RuntimeError, match="float"):
        ops.cosine_similarity(f1, f2.half(), TEMP)
    with pytest.raises(ValueError, match="agree"):
        ops.cosine_similarity(f1, f2[:1].contiguous(), TEMP)
    with pytest.raises(ValueError, match="agree"):
        ops.cosine_similarity(f1, f2[:, :, :16].contiguous(), TEMP)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(RuntimeError, match="s6d_cosine_similarity_f32"):
            ops.cosine_similarity(f1, f2, bad)
    out = torch.full((2, 37, 21), -7.0).cuda()
    P = lambda t: t.data_ptr()
    s = ops._stream()
    fn = ops._fn("s6d_cosine_similarity_f32", 9)
    assert fn(P(f1), P(f2), 2, 37, 21, 6, TEMP, P(out), s) == -3
    assert fn(P(f1), P(f2), 2, 37, 21, 516, TEMP, P(out), s) == -3
    assert fn(P(f1), P(f2), 0, 37, 21, 32, TEMP, P(out), s) == 0
    assert fn(None, None, 0, 37, 21, 32, TEMP, None, s) == 0
    assert fn(None, P(f2), 2, 37, 21, 32, TEMP, P(out), s) == -1
    assert fn(P(f1), P(f2), 2, 37, 21, 32, TEMP, None, s) == -1
    assert fn(P(f1), P(f2), 2, 0, 21, 32, TEMP, P(out), s) == -1
    torch.cuda.synchronize()
    assert (out.cpu() == -7).all()


# ---------------------------------------------------------------------------------------------------------------- on the MI355X
@pytest.mark.parametrize("B,M1,M2,C", SHAPES)
def test_vs_float64(ops, B, M1, M2, C):
    check_vs_float64(ops, B, M1, M2, C)


@pytest.mark.parametrize("B,M1,M2,C", [(2, 37, 21, 32), (3, 197, 197, 256)])
def test_hostile_rows(ops, B, M1, M2, C):
    check_hostile_rows(ops, B, M1, M2, C)


@pytest.mark.parametrize("B,M1,M2,C", SHAPES)
def test_batch_invariance(ops, B, M1, M2, C):
    check_batch_invariance(ops, M1, M2, C)


@pytest.mark.parametrize("B,M1,M2,C", SHAPES)
def test_transpose_symmetry(ops, B, M1, M2, C):
    check_transpose_symmetry(ops, B, M1, M2, C)


@pytest.mark.parametrize("B,N,C,n1,n2", [(3, 196, 256, 6000, 300), (2, 40, 32, 300, 30)])
def test_into_sampling_head(ops, B, N, C, n1, n2):
    check_into_sampling_head(ops, B, N, C, n1, n2)


def test_module_is_batch_invariant_under_strict(ops):
    """CoarsePointMatching at the default config (seeded weights, 196 points) under strict mode with the kernel selected: init_R / init_t
    of instance 0 are the same bits at B = 1 and B = 3, and no library branch is recorded for pem.feature_similarity."""
    from sam6d_amd import policy
    from sam6d_amd.pem.layers import GeometricStructureEmbedding
    from sam6d_amd.pem.pose_estimation_model import CoarsePointMatching, default_cfg
    from sam6d_amd.utils import seeded
    cfg = default_cfg()
    head = seeded.load_seeded(CoarsePointMatching(cfg.coarse_point_matching).eval(), 5).cuda()
    geo = seeded.load_seeded(GeometricStructureEmbedding(cfg.geo_embedding).eval(), 4).cuda()
    B, N = 3, 196
    g = torch.Generator().manual_seed(12)
    p2 = torch.randn(B, N, 3, generator=g) * 0.3
    Rgt = synth.random_rotations(B, g)
    p1 = (p2 @ Rgt.transpose(1, 2) + 0.05 * torch.randn(B, 1, 3, generator=g)).contiguous()
    f1 = torch.randn(B, N, 256, generator=g)
    f2 = f1 + 0.2 * torch.randn(B, N, 256, generator=g)
    radius = torch.ones(B)
    model = p2[:, :128].contiguous()
    u = torch.rand(B, 3 * cfg.coarse_point_matching.nproposal1, generator=g)
    p1, p2, f1, f2, radius, model, u = (t.cuda() for t in (p1, p2, f1, f2, radius, model, u))
    bg = torch.full((B, 1, 3), 100.0, device="cuda")

    def run(sl):
        geo1, geo2 = geo(torch.cat([bg, p1], 1)[sl].contiguous()), geo(torch.cat([bg, p2], 1)[sl].contiguous())
        ep = head(p1[sl].contiguous(), f1[sl].contiguous(), geo1, p2[sl].contiguous(), f2[sl].contiguous(), geo2, radius[sl],
                  dict(model=model[sl].contiguous(), coarse_rand_u=u[sl].contiguous()))
        return ep["init_R"].cpu(), ep["init_t"].cpu()

    policy.reset_library_branch_hits()
    with torch.no_grad(), policy.use(strict="1", coarse_sim="1"):
        assert ops.have("cosine_similarity")
        R3, t3 = run(slice(0, 3))
        R1, t1 = run(slice(0, 1))
    assert torch.isfinite(R3).all() and torch.isfinite(t3).all()
    assert torch.equal(R1[0], R3[0]) and torch.equal(t1[0], t3[0])
    assert not [k for k in policy.library_branch_hits() if k[0] == "pem.feature_similarity"], policy.library_branch_hits()


def test_arguments(ops):
    check_arguments(ops)
