"""The pose model's own fp32 attention kernels, called directly, on inputs built against their trip and tile sizes.

csrc/s6d_rpe.hip -- rpe_attention_kernel: one wavefront per query row (b, n), four rows per workgroup (a "strip": the last one is
ragged when B N % 4 != 0), keys taken four per trip of the score loop (one per trip beyond 5000 rows; the last trip is ragged when
M % 4 != 0 and repeats key M - 1), the scores of the row's four heads in LDS ((M + 3) & ~3 floats per head: at most 1024 keys fit
in 64 KiB), a 16-lane maximum / sum per head, then P.V.  Entry points: s6d_rpe_attention_f32 and its packed / packed_e16 / strided /
strided_e16 forms, s6d_mha_f32 / s6d_mha_strided_f32 (the same kernel without the embedding stream), s6d_linear_attn_focus_f32.
csrc/s6d_linattn.hip -- s6d_linear_attention_f32: linattn_kv_kernel stages 28 keys at a time, linattn_apply_kernel owns 64 query
rows per workgroup.

Every comparison is against a float64 statement of the reference operation on the SAME float32 operands (the half-stored embedding
widened): RPEMultiHeadAttention.forward, Pose_Estimation_Model/model/transformer.py:385-404 (with p = proj_p(embed) written as
q~ . e + q . b_p, see sam6d_amd/pem/layers.py), MultiHeadAttention.forward, transformer.py:128-146, LinearAttention.forward,
transformer.py:541-550 (focus map) and :552-562 (kv-first branch).  The bounds are derived from the kernels' own roundings
(rows_reference, focus_reference, linattn_reference) with u = 2^-24; every measured error / bound is recorded with
util.record_margin and listed in profiles/pem_attention_margins.md.

The case functions take the device so that tests/test_emu_pem_attention.py runs the same bodies on the host emulator."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import util

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                      # unit roundoff of float32
SCALE = 0.125                       # 1 / sqrt(64): d_model 256, 4 heads
C, H, D = 256, 4, 64
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sam6d_amd", "csrc")


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _randn(g, dev, *shape):
    return torch.randn(*shape, generator=g, device=dev)


# ------------------------------------------------------------------------------------------------------------------------------
# rpe_attention_kernel: float64 reference and bound

KS = 14        # roundings on the longest path of one score, see rows_reference


def rows_reference(q, k, v, qt, qb, emb, scale, chunk=64):
    """float64 reference and elementwise bound for ONE instance of the rows kernel: q (N,256), k / v (M,256), and for the RPE form
    qt (4,N,256), qb (4,N), emb (N,M,256) (float32 or half: the operand the kernel reads, widened here); qt = None is plain
    multi-head attention.  -> (ref, bound, vacuity), ref / bound (N,256) float64.

    Reference (transformer.py:390-402 / :132-144): s[h,n,m] = (q_h[n] . k_h[m] + qt[h,n] . emb[n,m] + qb[h,n]) scale,
    w = softmax_m(s), ref = sum_m w v_h[m].

    The kernel's roundings, u = 2^-24:
      * a score is a tree of float32 products and sums -- dot4 (a product and three fused multiply-adds), the two cross-lane
        folds of the embedding term, the sum with the q.k partial, four butterfly steps, + qb, x scale: at most 13 roundings on any
        path from a product to the score, so |s' - s| <= KS u S with KS = 14 (13, and one for the second-order terms) and
        S[h,n,m] = scale (|q_h|.|k_h| + |qt_h|.|emb| + |qb|);
      * p_m = __expf(s'_m - mx): the subtraction (u |x|), the product with log2(e) in front of the hardware exp2 (u |x|) and
        the exp2 itself (1 ulp = 2^-23), x = s'_m - mx ~ log w_m.  An error of mx itself scales every p_m alike and cancels
        in P.V / sum.  So p_m = c w_m exp(e_m), |e_m| <= E_m = KS u S_m + 2 u (|log w_m| + 1) + 2^-23;
      * hence the kernel's weights are w'_m = 1 / (1 + sum_{k != m} exp((ls_k + e_k) - (ls_m + e_m))), ls = log w, which lies between
        1 / (1 + sum_{k != m} exp(ls_k - ls_m + E_k + E_m)) and 1 / (1 + sum_{k != m} exp(ls_k - ls_m - E_k - E_m)) (_interval:
        evaluated with logarithms and the leave-one-out sum, so that a head whose scores are 2^40 apart -- E of order 2^22 -- keeps
        its exact one-hot weights where the second key is still far below the first);  dw_m = the larger distance of the two
        ends from w_m;  sum_m (w'_m - w_m) = 0, so  |sum_m w'_m v_m - ref| <= sum_m dw_m |v_m - ref| <= dw.|v| + |ref| sum_m dw_m;
      * P.V is M fused multiply-adds in sequence, the row sum M / 16 additions and four butterfly steps, then one reciprocal and
        one product: g (A + |ref|) with g = (M + M / 16 + 8) u and A = sum_m w'_m |v_m| <= w.|v| + dw.|v|;
      * p_m below float32's normal range (x < -87) is flushed: an absolute 2^-126 against a row sum >= 1, M 2^-126 max |v|.
    bound = dw.|v| + |ref| sum dw + g (w.|v| + dw.|v| + |ref|) + M 2^-126 max|v|.

    vacuity = max over the instance of (dw.|v| + |ref| sum dw) / (w.|v| + |ref|): a construction whose bound says nothing (two
    keys that float32 cannot tell apart) would show here; the cases assert it stays below 1 %."""
    N, M = q.shape[0], k.shape[0]
    kh, vh = (t.double().view(M, H, D).transpose(0, 1) for t in (k, v))            # (4, M, 64)
    vabs = vh.abs()
    refs, bounds, vac = [], [], 0.0
    g = (M + M / 16 + 8) * U
    for r0 in range(0, N, chunk):
        r1 = min(N, r0 + chunk)
        qh = q[r0:r1].double().view(r1 - r0, H, D).transpose(0, 1)                 # (4, n, 64)
        s = qh @ kh.transpose(1, 2)
        S = qh.abs() @ kh.abs().transpose(1, 2)
        if qt is not None:
            e = emb[r0:r1].double()                                                # (n, M, 256)
            t = qt[:, r0:r1].double()                                              # (4, n, 256)
            s = s + torch.einsum("hnc,nmc->hnm", t, e) + qb[:, r0:r1].double()[..., None]
            S = S + torch.einsum("hnc,nmc->hnm", t.abs(), e.abs()) + qb[:, r0:r1].double().abs()[..., None]
            del e
        s, S = s * scale, S * scale
        ls = torch.log_softmax(s, -1)
        w = ls.exp()
        E = KS * U * S + 2 * U * (ls.abs() + 1) + 2.0 ** -23
        dw = torch.maximum(_interval(ls - E, -ls - E) - w, w - _interval(ls + E, -ls + E))
        ref = w @ vh                                                              # (4, n, 64)
        A = w @ vabs
        first = dw @ vabs + ref.abs() * dw.sum(-1, keepdim=True)
        bound = first + g * (A + dw @ vabs + ref.abs()) + M * 2.0 ** -126 * vabs.amax(1, keepdim=True)
        vac = max(vac, (first / (A + ref.abs()).clamp_min(1e-300)).max().item())
        refs.append(ref.transpose(0, 1).reshape(r1 - r0, C))
        bounds.append(bound.transpose(0, 1).reshape(r1 - r0, C))
    return torch.cat(refs), torch.cat(bounds), vac


def _interval(a, b):
    """1 / (1 + exp(b_m) sum_{k != m} exp(a_k)) over the last axis, without overflow and without cancellation in the leave-one-out
    sum (the largest term is left out by summing the others, every other term by subtracting it from a total that holds the
    largest)."""
    amax, jmax = a.max(-1, keepdim=True)
    ex = (a - amax).exp()
    excl = ex.sum(-1, keepdim=True) - ex
    excl.scatter_(-1, jmax, ex.scatter(-1, jmax, 0.0).sum(-1, keepdim=True))
    return torch.sigmoid(-(b + amax + excl.clamp_min(0.0).log()))


def check_rows(out, q, k, v, qt, qb, emb, what):
    """One instance's kernel output (N,256) against rows_reference.  -> max err / bound."""
    ref, bound, vac = rows_reference(q, k, v, qt, qb, emb, SCALE)
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    assert torch.isfinite(bound).all() and vac < 0.01, f"{what}: the bound says nothing for this construction (vacuity {vac:.3g})"
    err = (out.double() - ref).abs()
    r = (err / bound).max().item()
    if r > 1:
        bad = (err > bound).nonzero()[:5].tolist()
        raise AssertionError(f"{what}: err / bound {r:.3f}; first (query, channel) outside: {bad}")
    return r


def check_mean(out, v, what):
    """Equal scores in a row (q = 0, or the bias alone): exp(0) = 1 exactly, so the output is the mean of v to the roundings of the
    row sum and of P.V, g (mean |v| + |mean v|) with rows_reference's g."""
    M = v.shape[0]
    mean, mabs = v.double().mean(0, keepdim=True), v.double().abs().mean(0, keepdim=True)
    assert ((out.double() - mean).abs() <= (M + M / 16 + 8) * U * (mabs + mean.abs())).all(), f"{what}: not the mean of v"


# ------------------------------------------------------------------------------------------------------------------------------
# constructions (one instance, in place)

TRIP = 4                             # keys per trip of the score loop (KEYS = 4; the one-key form must give the same bits)
STEP = 0.9                           # grow / shrink: 2 x 0.9 x 64 x 0.125 = 14.4 nats = 20.8 log2 units per trip


def tail_key(M):
    """A key of the ragged last trip (M % 4 != 0), not the last one where the tail holds more than one; else of the last full trip."""
    return M - 1 if M % TRIP == 1 else (M // TRIP * TRIP if M % TRIP else max(M - 3, 0))


def construct(kind, q, k, v, qt=None, qb=None):
    """Shape one instance's operands: q (N,256), k / v (M,256), qt (4,N,256), qb (4,N) (None for plain attention).
      dom_first / dom_last / dom_tail: every query gets 1.5 x a +-1 pattern added, key 0 / M - 1 / tail_key(M) IS 1.5 x the
        pattern: its score exceeds the others' by 18 nats in every head;
      grow / shrink: every query gets 2 x the pattern, the keys of trip t get 0.9 t x the pattern plus half their noise (shrink:
        0.9 (T - 1 - t)): each trip's maximum is 20.8 log2 units above (below) the previous one; the row maximum is in the last
        (first) trip and most keys' weights underflow;
      only_qk / only_embed / only_bias: the score is carried by one term, the others are zero (only_embed: q = 0 and q~ x 5;
        only_bias: q = 0, q~ = 0: the softmax is uniform whatever qb is -- qb is constant over a row's keys, so in exact arithmetic
        the output does not depend on it at all; what a wrong qb can still do is poison the row, or cost the other terms their bits);
      head_scaled: head 2's q, k, v, q~ and qb x 2^20 (scores of order 2^40 beside heads of order 1: a maximum or sum shared
        between heads turns the neighbours' weights to zero);
      big_v: v x 2^50;   qzero: q = 0 (and q~ = 0, qb = 0): the output is the mean of v."""
    M = k.shape[0]
    pat = torch.where(torch.arange(C, device=q.device) % 2 == 0, 1.0, -1.0)
    if kind.startswith("dom_"):
        j = {"dom_first": 0, "dom_last": M - 1, "dom_tail": tail_key(M)}[kind]
        q += 1.5 * pat
        k[j] = 1.5 * pat
    elif kind in ("grow", "shrink"):
        t = (torch.arange(M, device=q.device) // TRIP).float()
        gt = STEP * (t if kind == "grow" else t.max() - t)
        q += 2.0 * pat
        k.mul_(0.5).add_(gt[:, None] * pat)
    elif kind == "only_qk":
        if qt is not None:
            qt.zero_(), qb.zero_()
    elif kind == "only_embed":
        q.zero_(), qb.zero_(), qt.mul_(5.0)
    elif kind == "only_bias":
        q.zero_(), qt.zero_(), qb.mul_(3.0)
    elif kind == "head_scaled":
        for t in (q, k, v):
            t[:, 2 * D:3 * D] *= 2.0 ** 20
        if qt is not None:
            qt[2] *= 2.0 ** 20
            qb[2] *= 2.0 ** 20
    elif kind == "big_v":
        v *= 2.0 ** 50
    elif kind == "qzero":
        q.zero_()
        if qt is not None:
            qt.zero_(), qb.zero_()
    else:
        assert kind == "random", kind


RPE_KINDS = ("dom_first", "dom_last", "dom_tail", "grow", "shrink", "only_qk", "only_embed", "only_bias", "head_scaled", "big_v")
MHA_KINDS = ("dom_first", "dom_last", "dom_tail", "grow", "shrink", "head_scaled", "big_v", "qzero")


def _pairs(kinds):
    return [(kinds[i], kinds[i + 1]) for i in range(0, len(kinds), 2)]


def rpe_operands(dev, B, N, kinds, seed):
    """q, k, v (B,N,256), q~ (B,4,N,256) (0.1 x noise, as W_p^T q is small beside q), qb (B,4,N), embedding (B,N,N,256); instance b
    shaped by kinds[b]."""
    g = _gen(dev, seed)
    q, k, v = (_randn(g, dev, B, N, C) for _ in range(3))
    qt, qb, emb = 0.1 * _randn(g, dev, B, H, N, C), _randn(g, dev, B, H, N), _randn(g, dev, B, N, N, C)
    for b, kind in enumerate(kinds):
        construct(kind, q[b], k[b], v[b], qt[b], qb[b])
    return q, k, v, qt, qb, emb


# ------------------------------------------------------------------------------------------------------------------------------
# 1. rpe_attention: the five entry points

def rpe_plain(q, k, v, qt, qb, emb):
    """s6d_rpe_attention_f32 itself (ops.rpe_attention goes through the strided entry point)."""
    from sam6d_amd import ops
    B, N, _ = q.shape
    out = torch.empty(B, N, C, dtype=torch.float32, device=q.device)
    ops._call("s6d_rpe_attention_f32", q.data_ptr(), k.data_ptr(), v.data_ptr(), qt.data_ptr(), qb.data_ptr(), emb.data_ptr(), B, N, C,
              H, SCALE, out.data_ptr(), ops._stream())
    return out


def rpe_packed_operand(q, k, v, qt, qb):
    """q | k | v | q~ (head h at 768 + 256 h) | qb as the column blocks of one (B, N, 1796) tensor."""
    B, N, _ = q.shape
    return torch.cat([q, k, v, qt.permute(0, 2, 1, 3).reshape(B, N, H * C), qb.permute(0, 2, 1)], dim=-1).contiguous()


def rpe_forms(q, k, v, qt, qb, emb):
    """The five entry points on the same operands.  Same kernel, same instantiation, other addressing: the strided form (q, k, v
    as column blocks of one (B,N,768) tensor) and the packed form must equal the plain one bit for bit, and the e16 forms must equal
    the plain form on the half-rounded embedding widened to float32 (tests/test_gpu_pose.py::
    test_half_stored_geo_embedding_and_its_reader claims that for the strided pair).  -> (plain, plain on the widened half embedding,
    that embedding in half)."""
    from sam6d_amd import ops
    plain = rpe_plain(q, k, v, qt, qb, emb)
    qkv = torch.cat([q, k, v], dim=-1)
    sq, sk, sv = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    assert ops._rows3(sk, "k")[1] == 3 * C                                         # attended in place, not copied
    assert torch.equal(ops.rpe_attention(sq, sk, sv, qt, qb, emb, SCALE), plain), "strided form differs from the plain one"
    proj = rpe_packed_operand(q, k, v, qt, qb)
    assert torch.equal(ops.rpe_attention_packed(proj, emb, SCALE), plain), "packed form differs from the plain one"
    e16 = emb.half()
    plain16 = rpe_plain(q, k, v, qt, qb, e16.float())
    assert torch.equal(ops.rpe_attention(sq, sk, sv, qt, qb, e16, SCALE), plain16), "strided e16 form differs from the widened embedding"
    assert torch.equal(ops.rpe_attention_packed(proj, e16, SCALE), plain16), "packed e16 form differs from the widened embedding"
    return plain, plain16, e16


def rpe_case(N, kinds, dev="cuda", tag=""):
    """Two instances of N points in one launch, shaped by `kinds`, through the five entry points; both instances against float64,
    the f32-embedding forms and the e16 forms (whose reference reads the half-rounded embedding: the rounding of the operand is in
    the reference, the products and sums are the float32 ones, so the bound is the same)."""
    B = len(kinds)
    q, k, v, qt, qb, emb = rpe_operands(dev, B, N, kinds, 100 * N + sum(map(ord, "".join(kinds))))
    plain, plain16, e16 = rpe_forms(q, k, v, qt, qb, emb)
    worst = 0.0
    for b, kind in enumerate(kinds):
        worst = max(worst, check_rows(plain[b], q[b], k[b], v[b], qt[b], qb[b], emb[b], f"rpe N={N} {kind}"))
        worst = max(worst, check_rows(plain16[b], q[b], k[b], v[b], qt[b], qb[b], e16[b], f"rpe e16 N={N} {kind}"))
        if kind == "only_bias":
            check_mean(plain[b], v[b], f"rpe N={N} {kind}")
    util.record_margin(f"pem_rpe_attention_N{N}_{'+'.join(kinds)}{tag}", max_err_over_bound=worst, bound_ratio=1.0)


RPE_SIZES = (197, 39, 4, 1)          # production (197 % 4 = 1, 394 rows % 4 = 2); 39 % 4 = 3, 78 rows % 4 = 2; one full trip; smallest


@pytest.mark.parametrize("kinds", _pairs(RPE_KINDS), ids="+".join)
@pytest.mark.parametrize("N", RPE_SIZES)
def test_rpe_attention_entry_points_on_hostile_inputs(N, kinds):
    rpe_case(N, kinds)


def test_rpe_attention_hostile_rows_do_not_depend_on_the_batch_size():
    """tests/test_gpu_pose.py::test_rpe_attention_rows_do_not_depend_on_the_batch_size on hostile instances: 28 x 197 = 5516 rows
    take the one-key-per-trip instantiation, the same two instances alone (394 rows) the four-key one.  Equal bits, and float64."""
    from sam6d_amd import ops
    Bbig, N = 28, 197
    kinds = ["random"] * Bbig
    kinds[5], kinds[6] = "grow", "dom_tail"
    q, k, v, qt, qb, emb = rpe_operands("cuda", Bbig, N, kinds, 12)
    big = ops.rpe_attention(q, k, v, qt, qb, emb, SCALE)
    sl = slice(5, 7)
    small = ops.rpe_attention(*(t[sl].contiguous() for t in (q, k, v, qt, qb, emb)), SCALE)
    assert torch.equal(big[sl], small)
    worst = max(check_rows(big[b], q[b], k[b], v[b], qt[b], qb[b], emb[b], f"rpe one key per trip {kinds[b]}") for b in (5, 6))
    util.record_margin("pem_rpe_attention_5516_rows_grow+dom_tail", max_err_over_bound=worst, bound_ratio=1.0)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. mha / mha_strided

def mha_plain(q, k, v):
    """s6d_mha_f32 itself (ops.mha goes through the strided entry point)."""
    from sam6d_amd import ops
    B, N, _ = q.shape
    out = torch.empty(B, N, C, dtype=torch.float32, device=q.device)
    ops._call("s6d_mha_f32", q.data_ptr(), k.data_ptr(), v.data_ptr(), B, N, k.shape[1], C, H, SCALE, out.data_ptr(), ops._stream())
    return out


def mha_forms(q, k, v):
    """ops.mha on contiguous operands, s6d_mha_f32, and ops.mha on q / k / v as column blocks of projection outputs 768 wide (q of a
    (B,N,768) tensor, k | v of a (B,M,768) one): equal bits."""
    from sam6d_amd import ops
    B, N, _ = q.shape
    M = k.shape[1]
    out = ops.mha(q, k, v, SCALE)
    assert torch.equal(mha_plain(q, k, v), out), "s6d_mha_f32 differs from s6d_mha_strided_f32 at ld = 256"
    pq = torch.cat([q, torch.full((B, N, 2 * C), float("nan"), device=q.device)], dim=-1)
    pkv = torch.cat([torch.full((B, M, C), float("nan"), device=q.device), k, v], dim=-1)
    sq, sk, sv = pq[..., :C], pkv[..., C:2 * C], pkv[..., 2 * C:]
    assert ops._rows3(sv, "v")[1] == 3 * C
    assert torch.equal(ops.mha(sq, sk, sv, SCALE), out), "strided form (ld = 768) differs from the contiguous one"
    return out


def mha_case(N, M, kinds, dev="cuda", tag=""):
    B = len(kinds)
    g = _gen(dev, 1000 * N + M + sum(map(ord, "".join(kinds))))
    q, k, v = _randn(g, dev, B, N, C), _randn(g, dev, B, M, C), _randn(g, dev, B, M, C)
    for b, kind in enumerate(kinds):
        construct(kind, q[b], k[b], v[b])
    out = mha_forms(q, k, v)
    worst = 0.0
    for b, kind in enumerate(kinds):
        worst = max(worst, check_rows(out[b], q[b], k[b], v[b], None, None, None, f"mha ({N},{M}) {kind}"))
        if kind == "qzero":
            check_mean(out[b], v[b], f"mha ({N},{M}) {kind}")
    util.record_margin(f"pem_mha_N{N}_M{M}_{'+'.join(kinds)}{tag}", max_err_over_bound=worst, bound_ratio=1.0)


# (N, M): the cross attention's shapes, one row / one key, and the boundaries of the kernel: the key trip (4), the query strip
# (4 rows per workgroup; B = 2: 6 / 8 / 10 rows), the 16-lane softmax sweep (15 / 16 / 17 keys), 150 % 4 = 2, 77 % 4 = 1
MHA_SHAPES = ((197, 197), (197, 150), (1, 1), (61, 77), (3, 3), (4, 4), (5, 5), (2, 15), (2, 16), (2, 17))


@pytest.mark.parametrize("kinds", _pairs(MHA_KINDS), ids="+".join)
@pytest.mark.parametrize("N,M", MHA_SHAPES)
def test_mha_entry_points_on_hostile_inputs(N, M, kinds):
    mha_case(N, M, kinds)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the LDS limit

def launcher_limits():
    """{launcher: the largest key count it serves}, from each launcher's own statements in csrc/s6d_rpe.hip:
    `constexpr int WAVES = w; ... Np = (X + 3) & ~3; lds = (size_t)WAVES * h * Np * sizeof(float); if (lds > L * 1024) return
    S6D_EUNSUPPORTED;` -- the formula is evaluated here for growing key counts."""
    text = open(os.path.join(CSRC, "s6d_rpe.hip")).read()
    limits = {}
    for name in ("rpe_strided", "rpe_packed", "s6d_mha_strided_f32"):
        body = text[text.index(("static int " if name.startswith("rpe_") else 'extern "C" int ') + name + "("):]
        body = body[:body.index("return launch_status();")]
        waves = int(re.search(r"constexpr int WAVES = (\d+);", body).group(1))
        assert re.search(r"const int Np = \([NM] \+ 3\) & ~3;", body), name
        heads = int(re.search(r"const size_t lds = \(size_t\)WAVES \* (\d+) \* Np \* sizeof\(float\);", body).group(1))
        kib = int(re.search(r"if \(lds > (\d+) \* 1024\) return S6D_EUNSUPPORTED;", body).group(1))
        lds = lambda n: waves * heads * ((n + 3) & ~3) * 4      # noqa: E731
        n = 1
        while lds(n + 1) <= kib * 1024:
            n += 1
        limits[name] = n
    return limits


def _eunsupported():
    text = open(os.path.join(os.path.dirname(CSRC), "..", "include", "sam6d_hip.h")).read()
    return int(re.search(r"#define S6D_EUNSUPPORTED \((-?\d+)\)", text).group(1))


def _layer_ref_mha(m, x, mem):
    d = lambda t: t.detach().double()      # noqa: E731
    B, N, M = x.shape[0], x.shape[1], mem.shape[1]
    q = (d(x) @ d(m.proj_q.weight).t() + d(m.proj_q.bias)).view(B, N, H, D).transpose(1, 2)
    k = (d(mem) @ d(m.proj_k.weight).t() + d(m.proj_k.bias)).view(B, M, H, D).transpose(1, 2)
    v = (d(mem) @ d(m.proj_v.weight).t() + d(m.proj_v.bias)).view(B, M, H, D).transpose(1, 2)
    return (torch.softmax(q @ k.transpose(-1, -2) * SCALE, -1) @ v).transpose(1, 2).reshape(B, N, C)


def mha_lds_limit_case(dev="cuda", tag=""):
    """s6d_mha_strided_f32 at the largest M its LDS formula admits (float64, a dominant last key and growing scores), the entry
    point's S6D_EUNSUPPORTED one above, and MultiHeadAttention there: the library statement, recorded as a library branch."""
    from sam6d_amd import _lib, ops, policy
    from sam6d_amd.pem.layers import MultiHeadAttention
    from sam6d_amd.utils import seeded
    limits = launcher_limits()
    Mmax = limits["s6d_mha_strided_f32"]
    assert ops.ATTN_ROWS_MAX_KEYS == Mmax == limits["rpe_strided"] == limits["rpe_packed"]
    mha_case(5, Mmax, ("dom_last", "grow"), dev=dev, tag=tag)
    g = _gen(dev, 77)
    q, k = _randn(g, dev, 1, 5, C), _randn(g, dev, 1, Mmax + 1, C)
    out = torch.empty(1, 5, C, device=dev)
    for fn, args in (("s6d_mha_f32", (q.data_ptr(), k.data_ptr(), k.data_ptr())), ("s6d_mha_strided_f32", (q.data_ptr(), C, k.data_ptr(), C, k.data_ptr(), C))):
        args = args + (1, 5, Mmax + 1, C, H, SCALE, out.data_ptr(), ops._stream())
        assert ops._fn(fn, len(args))(*args) == _eunsupported(), fn
    with pytest.raises(_lib.S6DError):
        ops.mha(q, k, k, SCALE)
    m = seeded.load_seeded(MultiHeadAttention(C).eval(), 5)
    m = m.cuda() if dev == "cuda" else m
    policy.reset_library_branch_hits()
    with torch.no_grad():
        got = m(q, k, k)
    assert ("pem.MultiHeadAttention", "keys") in policy.library_branch_hits(), policy.library_branch_hits()
    ref = _layer_ref_mha(m, q, k)
    assert ((got.double() - ref).abs() <= 2e-5 * (1 + ref.abs())).all()
    policy.reset_library_branch_hits()
    with torch.no_grad():
        got = m(q, k[:, :Mmax], k[:, :Mmax])
    assert not policy.library_branch_hits(), policy.library_branch_hits()        # at the limit the kernel serves the layer
    ref = _layer_ref_mha(m, q, k[:, :Mmax])
    assert ((got.double() - ref).abs() <= 2e-5 * (1 + ref.abs())).all()


def test_mha_lds_limit():
    mha_lds_limit_case()


def rpe_lds_limit_case(dev="cuda", at_limit=True, layer=True):
    """rpe_strided / rpe_packed at the largest N their LDS formula admits (one instance: a 1 GiB embedding; float64 in row blocks),
    S6D_EUNSUPPORTED from all five entry points one above, and RPEMultiHeadAttention there (both settings of S6D_RPE_FOLD): the
    library statement, recorded as a library branch.  The emulator runs the refusals only (at_limit = layer = False: the embedding
    is then never read)."""
    from sam6d_amd import _lib, ops, policy
    from sam6d_amd.pem.layers import RPEMultiHeadAttention
    from sam6d_amd.utils import seeded
    limits = launcher_limits()
    Nmax = limits["rpe_strided"]
    assert limits["rpe_packed"] == Nmax == ops.ATTN_ROWS_MAX_KEYS
    if at_limit:
        q, k, v, qt, qb, emb = rpe_operands(dev, 1, Nmax, ("dom_tail",), 5)
        out = rpe_plain(q, k, v, qt, qb, emb)
        proj = rpe_packed_operand(q, k, v, qt, qb)
        assert torch.equal(ops.rpe_attention_packed(proj, emb, SCALE), out)
        r = check_rows(out[0], q[0], k[0], v[0], qt[0], qb[0], emb[0], f"rpe N={Nmax}")
        util.record_margin(f"pem_rpe_attention_N{Nmax}_dom_tail", max_err_over_bound=r, bound_ratio=1.0)
        del q, k, v, qt, qb, emb, proj, out
    N = Nmax + 1
    g = _gen(dev, 6)
    x = _randn(g, dev, 1, N, C)
    qt, qb = torch.zeros(1, H, N, C, device=dev), torch.zeros(1, H, N, device=dev)
    proj = torch.zeros(1, N, 3 * C + H * C + H, device=dev)
    emb = (0.5 * _randn(g, dev, 1, N, N, C)) if layer else torch.empty(1, N, N, C, device=dev)
    for e in (emb, emb.half() if layer else torch.empty(1, N, N, C, device=dev, dtype=torch.float16)):
        with pytest.raises(_lib.S6DError, match="not supported"):
            ops.rpe_attention(x, x, x, qt, qb, e, SCALE)
        with pytest.raises(_lib.S6DError, match="not supported"):
            ops.rpe_attention_packed(proj, e, SCALE)
    with pytest.raises(_lib.S6DError, match="not supported"):
        rpe_plain(x, x, x, qt, qb, emb)
    args = (x.data_ptr(), x.data_ptr(), x.data_ptr(), qt.data_ptr(), qb.data_ptr(), emb.data_ptr(), 1, N, C, H, SCALE, x.data_ptr(), ops._stream())
    assert ops._fn("s6d_rpe_attention_f32", len(args))(*args) == _eunsupported()
    if not layer:
        return
    del qt, qb, proj
    m = seeded.load_seeded(RPEMultiHeadAttention(C).eval(), 4)
    m = m.cuda() if dev == "cuda" else m
    d = lambda t: t.detach().double()      # noqa: E731
    with torch.no_grad():
        outs = {}
        for fold in ("1", "0"):
            with policy.use(rpe_fold=fold):
                policy.reset_library_branch_hits()
                outs[fold] = m(x, emb)
                assert ("pem.RPEMultiHeadAttention" + ("" if fold == "1" else ".core"), "keys") in policy.library_branch_hits(), \
                    policy.library_branch_hits()
        # transformer.py:385-404 in float64 on a block of query rows (the whole (4, N, N, 64) tensor p is 2 GiB)
        rows = slice(N - 40, N)
        q, k, v = ((d(x) @ d(l.weight).t() + d(l.bias)).view(N, H, D).transpose(0, 1) for l in (m.proj_q, m.proj_k, m.proj_v))
        p = (d(emb[0, rows]) @ d(m.proj_p.weight).t() + d(m.proj_p.bias)).view(40, N, H, D)
        s = (q[:, rows] @ k.transpose(1, 2) + torch.einsum("hnc,nmhc->hnm", q[:, rows], p)) * SCALE
        ref = (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(40, C)
    for fold, got in outs.items():
        assert ((got[0, rows].double() - ref).abs() <= 2e-5 * (1 + ref.abs())).all(), fold


def test_rpe_lds_limit():
    rpe_lds_limit_case()


# ------------------------------------------------------------------------------------------------------------------------------
# 4. linear_attn_focus / linear_attention

F32_MAX = 3.4028234663852886e38


def focus64(x, inv, p=3):
    """transformer.py:541-550 in float64 on float32 operands (inv = 1 / softplus(scale), the kernel's operand): -> (y, sum of t^2p)."""
    t = (F.relu(x.double()) + 1e-6) * inv.double()
    n = t.norm(dim=-1, keepdim=True)
    t = t ** p
    n3 = (t * t).sum(-1, keepdim=True)
    return t / n3.sqrt() * n, n3


def focus32(x, inv, p=3):
    """The same statements in float32, as the reference runs them."""
    t = (F.relu(x) + 1e-6) * inv
    n = t.norm(dim=-1, keepdim=True)
    t = t ** p
    return t / t.norm(dim=-1, keepdim=True) * n


def focus_reference(x, inv, sums=10):
    """-> (ref float64, relative bound, overflowed rows).  Every quantity of the focus map is positive, so its float32 errors are
    relative ones.  t = (relu(x) + 1e-6) inv: 2 roundings.  t^3: 2 more on 3 x 2 u = 8 u.  t^2: 5 u; t^6: 17 u.  A sum of such
    terms over a row: `sums` more roundings (focus_kernel: 3 in the lane, 6 butterfly steps, + 1 for second order = 10;
    linattn_apply_kernel: 64 fused multiply-adds in sequence and 2 additions across the heads, + 1 = 67).  The square roots halve
    and add one each, the quotient f one more: f within (5 + sums) / 2 + (17 + sums) / 2 + 3 u; y = t^3 f within that + 9 u
    = (23 + sums) u.

    Overflow: where the row's sum of t^6 exceeds float32's range the reference's float32 statements give |t^3| = inf, t^3 / inf = 0
    and 0 x |t| = 0: the whole row is EXACTLY ZERO (an activation of 1e10, or scale = -20 on activations of order 1).  The
    kernel is held to that: sqrtf(inf) = inf, f = |t| / inf = 0, y = t^3 x 0 = 0 (t^3 itself stays finite for t < 7e12).  Rows
    whose sum lies within a factor 2 of the range are not constructed (asserted)."""
    ref, n3 = focus64(x, inv)
    ovf = (n3 > 2 * F32_MAX).squeeze(-1)
    assert bool(((n3.squeeze(-1) < 0.5 * F32_MAX) | ovf).all()), "a row at the edge of float32's range"
    return ref, (23 + sums) * U, ovf


FOCUS_KINDS = ("random", "nonpos", "one_channel", "act1e3", "act1e10", "scale-20", "scale-20_small")


def focus_operand(kind, g, dev, B, R):
    """(x (B,R,256), scale (256)) of one construction: nonpos: no positive entry (t = 1e-6 inv everywhere); one_channel: one positive
    channel per row; act1e3 / act1e10: activations x 1e3 / 1e10; scale-20: softplus(scale) = 2e-9, inv = 5e8 on activations of
    order 1 (t^6 overflows: zero rows) and, _small, on activations of order 1e-4 and non-positive rows (finite)."""
    x = _randn(g, dev, B, R, C)
    scale = 0.3 * _randn(g, dev, C)
    if kind == "nonpos":
        x = -x.abs()
        x[:, ::2, ::3] = 0.0
    elif kind == "one_channel":
        ch = torch.randint(0, C, (B, R, 1), generator=g, device=dev)
        x = (-x.abs()).scatter(-1, ch, 0.5 + torch.rand(B, R, 1, generator=g, device=dev))
    elif kind == "act1e3":
        x = x * 1e3
    elif kind == "act1e10":
        x = x * 1e10
    elif kind.startswith("scale-20"):
        scale = torch.full((C,), -20.0, device=dev)
        if kind.endswith("_small"):
            x = x * 1e-4
            x[:, ::2] = -x[:, ::2].abs()
    return x.contiguous(), scale


def check_focus(y, x, inv, what, sums=10):
    ref, rel, ovf = focus_reference(x, inv, sums)
    assert torch.isfinite(y).all(), what
    if ovf.any():
        assert bool((focus32(x, inv)[ovf] == 0).all()), f"{what}: the float32 reference is not zero on an overflowed row"
        assert bool((y[ovf] == 0).all()), f"{what}: overflowed rows must be exactly zero, as the float32 reference has them"
    ok = ~ovf
    r = ((y.double() - ref).abs()[ok] / (rel * ref[ok] + 1e-44)).max().item() if ok.any() else 0.0
    assert r <= 1, f"{what}: err / bound {r:.3f}"
    return r, ovf


def focus_case(B, R, dev="cuda", tag=""):
    """s6d_linear_attn_focus_f32 on (B, R, 256) for every construction (four rows per workgroup: R = 65 and 29 leave a ragged one)."""
    from sam6d_amd import ops
    worst = {}
    for i, kind in enumerate(FOCUS_KINDS):
        x, scale = focus_operand(kind, _gen(dev, 31 * R + B + i), dev, B, R)
        inv = 1.0 / F.softplus(scale)
        y = ops.linear_attn_focus(x, inv, 3)
        r, ovf = check_focus(y, x, inv, f"focus ({B},{R}) {kind}")
        assert bool(ovf.all()) if kind in ("act1e10", "scale-20") else not bool(ovf.any()), (kind, ovf.float().mean())
        worst[kind] = r
        one = ops.linear_attn_focus(x[B - 1:].contiguous(), inv, 3)              # 5. an instance alone: the same bits
        assert torch.equal(one[0], y[B - 1]), kind
    util.record_margin(f"pem_linear_attn_focus_B{B}_R{R}{tag}", bound_ratio=1.0, **{f"err_over_bound_{k}": r for k, r in worst.items()})


def linattn_call(xq, inv, kf, v, pad_rows=64, sentinel=-7.25):
    """s6d_linear_attention_f32 through ops._call into a buffer of B I + pad_rows rows (and a workspace with 64 floats to spare) that
    hold a sentinel: -> out (B,I,256) after asserting that nothing behind it was written."""
    from sam6d_amd import ops
    B, I, _ = xq.shape
    J = kf.shape[1]
    buf = torch.full((B * I + pad_rows, C), sentinel, device=xq.device)
    nws = ops._size("s6d_linear_attention_workspace_floats", B)
    ws = torch.full((nws + 64,), sentinel, device=xq.device)
    ops._call("s6d_linear_attention_f32", xq.data_ptr(), inv.data_ptr(), 3, kf.data_ptr(), kf.stride(1), v.data_ptr(), v.stride(1), B, I, J,
              C, ws.data_ptr(), buf.data_ptr(), ops._stream())
    assert bool((buf[B * I:] == sentinel).all()), "rows behind the output written"
    assert bool((ws[nws:] == sentinel).all()), "floats behind the workspace written"
    return buf[:B * I].view(B, I, C)


def linattn_reference(xq, inv, kf, v):
    """transformer.py:552-558 in float64 on the kernel's float32 operands (the raw query projection, inv, the FOCUSED keys, v).
    -> (ref (B,I,256), bound, overflowed query rows, q . sum_j k_j (B,4,I,1)).

    The kernel: q = focus(xq) within eq = 90 u relative (focus_reference with the apply kernel's 67-rounding sums).  ksum_c =
    sum_j k_jc, J additions of non-negative terms: J u.  kv_cd = sum_j k_jc v_jd, J fused multiply-adds: J u sum_j k_jc |v_jd|.
    zd = q . ksum, 64 fused multiply-adds of non-negative terms: (eq + J + 64) u; + 1e-6 (float32's 1e-6 is 0.4 u off) and the
    reciprocal: z within (eq + J + 68) u.  acc_d = sum_c q_c kv_cd: (eq + J + 64) u A_d with A_d = sum_c q_c sum_j k_jc |v_jd|;
    out = acc z: one more.  bound = (eq + J + 65) u A_d z + (eq + J + 69) u |ref| <= (J + 160) u (A_d z + |ref|).
    Overflowed query rows (focus_reference): q = 0 exactly, so out = 0 x kv x 1e6 = 0 exactly."""
    B, I, _ = xq.shape
    J = kf.shape[1]
    qf, _, ovf = focus_reference(xq, inv, 67)
    split = lambda t: t.view(t.shape[0], t.shape[1], H, D).transpose(1, 2)      # noqa: E731
    q, k, vv = split(qf), split(kf.double()), split(v.double())
    z = 1.0 / (q @ k.sum(dim=2).unsqueeze(-1) + 1e-6)
    merge = lambda t: t.transpose(1, 2).reshape(B, I, C)      # noqa: E731
    ref = merge((q @ (k.transpose(-1, -2) @ vv)) * z)
    A = merge((q @ (k.transpose(-1, -2) @ vv.abs())) * z)
    return ref, (J + 160) * U * (A + ref.abs()), ovf, q @ k.sum(dim=2).unsqueeze(-1)


LIN_KEY_KINDS = ("random", "nonpos", "tiny_sum")


def linattn_case(B, I, J, dev="cuda", tag=""):
    """s6d_linear_attention_f32 at (B, I, J): every query construction of FOCUS_KINDS against random keys, and random queries
    against keys that are all <= 0 and against focused keys scaled so that q . sum_j k_j is about 1e-6 (z's epsilon is then half
    of the denominator).  k | v are the strided halves of one (B, J, 512) tensor.  The keys are focused by
    s6d_linear_attn_focus_f32 (checked by focus_case); the reference reads the focused float32 keys, the kernel's operand."""
    from sam6d_amd import ops
    worst = {}
    cases = [(qk, "random") for qk in FOCUS_KINDS] + [("random", kk) for kk in LIN_KEY_KINDS[1:]]
    for i, (qkind, kkind) in enumerate(cases):
        g = _gen(dev, 7 * I + J + 13 * B + i)
        xq, scale = focus_operand(qkind, g, dev, B, I)
        inv = 1.0 / F.softplus(scale)
        kvp = _randn(g, dev, B, J, 2 * C)
        xk = kvp[..., :C].contiguous()
        if kkind == "nonpos":
            xk = -xk.abs()
        if qkind == "scale-20_small":
            xk = xk * 1e-4                                                       # inv = 5e8: keys of order 1 would overflow to zero rows
        kf_ = ops.linear_attn_focus(xk, inv, 3)
        check_focus(kf_, xk, inv, f"linear attention keys ({B},{I},{J}) {qkind}/{kkind}")
        if kkind == "tiny_sum":
            qf = focus64(xq, inv)[0].view(B, I, H, D)
            dots = torch.einsum("bihc,bhc->bih", qf, kf_.double().view(B, J, H, D).sum(1))
            kf_ = (kf_ * (1e-6 / dots.median().item())).contiguous()
        kvp[..., :C] = kf_
        kf, v = kvp[..., :C], kvp[..., C:]
        out = linattn_call(xq, inv, kf, v)
        assert torch.equal(ops.linear_attention(xq, inv, 3, kf, v), out)
        ref, bound, ovf, zd = linattn_reference(xq, inv, kf, v)
        assert torch.isfinite(out).all(), (qkind, kkind)
        if kkind == "tiny_sum":
            assert 0.1e-6 < zd.median().item() < 10e-6
        if ovf.any():
            assert bool((out[ovf] == 0).all()), f"{qkind}: rows whose focus map overflows in float32 must be exactly zero"
        ok = ~ovf
        r = ((out.double() - ref).abs()[ok] / (bound[ok] + 1e-44)).max().item() if ok.any() else 0.0
        assert r <= 1, f"linear attention ({B},{I},{J}) {qkind}/{kkind}: err / bound {r:.3f}"
        worst[f"{qkind}/{kkind}"] = r
        # 5. the last instance alone: the same bits
        one = linattn_call(xq[B - 1:].contiguous(), inv, kf[B - 1:], v[B - 1:])
        assert torch.equal(one[0], out[B - 1]), (qkind, kkind)
    util.record_margin(f"pem_linear_attention_B{B}_I{I}_J{J}{tag}", bound_ratio=1.0, **{f"err_over_bound_{k}": r for k, r in worst.items()})


# (B, I, J): (1,65,29) is one row past the 64-row block of linattn_apply_kernel and one key past the 28-row stage of linattn_kv_kernel
LIN_SHAPES = ((2, 100, 37), (1, 64, 28), (1, 65, 29), (1, 1, 1), (3, 65, 29))


@pytest.mark.parametrize("B,I,J", LIN_SHAPES)
def test_linear_attention_on_hostile_inputs(B, I, J):
    linattn_case(B, I, J)


@pytest.mark.parametrize("B,R", [(2, 100), (1, 65), (3, 29), (1, 1)])
def test_linear_attn_focus_on_hostile_inputs(B, R):
    focus_case(B, R)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. batch invariance of the rows kernel (focus_case and linattn_case carry their own)

def rows_batch_invariance_case(N, M, dev="cuda"):
    """Instance b of a B = 3 launch equals the same instance launched alone, bit for bit: rpe_attention (N points) and mha (N x M),
    on a growing, a dominant-tail and a head-scaled instance."""
    from sam6d_amd import ops
    kinds = ("grow", "dom_tail", "head_scaled")
    q, k, v, qt, qb, emb = rpe_operands(dev, 3, N, kinds, 9)
    out = ops.rpe_attention(q, k, v, qt, qb, emb, SCALE)
    for b in range(3):
        one = ops.rpe_attention(*(t[b:b + 1].contiguous() for t in (q, k, v, qt, qb, emb)), SCALE)
        assert torch.equal(one[0], out[b]), f"rpe instance {b} ({kinds[b]}) differs from its B = 1 launch"
    g = _gen(dev, 10)
    q, k, v = _randn(g, dev, 3, N, C), _randn(g, dev, 3, M, C), _randn(g, dev, 3, M, C)
    for b, kind in enumerate(kinds):
        construct(kind, q[b], k[b], v[b])
    out = ops.mha(q, k, v, SCALE)
    for b in range(3):
        one = ops.mha(q[b:b + 1].contiguous(), k[b:b + 1].contiguous(), v[b:b + 1].contiguous(), SCALE)
        assert torch.equal(one[0], out[b]), f"mha instance {b} ({kinds[b]}) differs from its B = 1 launch"


@pytest.mark.parametrize("N,M", [(197, 150), (39, 77)])
def test_rows_kernel_instances_do_not_depend_on_the_batch(N, M):
    rows_batch_invariance_case(N, M)
