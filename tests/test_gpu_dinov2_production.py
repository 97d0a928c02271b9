"""The DINOv2 descriptor kernels at the sizes the ISM stage runs them: ViT-L/14 (C = 1024, 16 heads of 64, 257 tokens per crop,
hidden 4096) on batches of up to 255 crops = 65,535 token rows (the frame batcher's full batch, _FrameBatcher.FULL), and the PEM's
ViT-B sequence attention in IEEE half at its batch of 32 x 197 tokens.  tests/test_gpu_attn.py / test_gpu_gemm.py / test_gpu_dinov2.py
run the same kernels at a few sequences or a few hundred rows.

Every kernel is compared with a float64 statement of the same operation on the same rounded operands, computed on the device in row
blocks; the attention bounds are derived from the kernel's own roundings (see seq_attention_case), the GEMM bounds are the existing
tests'.  Where a kernel gives each sequence / row its own work, sampled sequences of the large launch must equal a B = 1 launch bit
for bit.  The whole descriptor path must give every frame's descriptors the bits of per-frame calls, whichever frames share its
batch.  Every measured value is recorded with util.record_margin.

The case functions take their sizes and the device so that tests/test_emu_dinov2.py runs the same bodies on the host emulator."""
import math
import types

import pytest
import torch
import torch.nn.functional as F

from tests import util

pytestmark = pytest.mark.gpu

BF, F16 = torch.bfloat16, torch.float16
LOG2E = 1.0 / math.log(2.0)


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------------------
# sequence attention (attn_window_kernel without bias: s6d_seq_attention_bf16 / _f16, token-major and head-major)

def _tiles(N):
    """(index of the tail tile, a key inside the last FULL 64-key tile) for N keys: 257 -> (4, 248), 197 -> (3, 184)."""
    nfull = N // 64
    return nfull, 64 * nfull - 8


def dominant_queries(N):
    """Queries that a dominant key must win: the first and last rows of the first strips, one in the middle, the last two rows (257:
    row 256 sits alone in the last 16-row strip; 197: rows 192..196 fill a strip of their own)."""
    return sorted({0, 1, 15, 16, 63, 64, 130 % N, N - 2, N - 1})


def _construct(q, k, v, kind, N, hd, vscale):
    """Shape one sequence's q / k / v (N, heads, hd) float32, in place.
      dom_last / dom_cls / dom_full: key N-1 (the only real key of a 257-token tail tile), key 0 (the cls token) or a key of the last
        full tile gets 1.5 x a +-1 pattern, the dominant_queries get 1.5 x the pattern added: their score against that key exceeds
        every other by ~14 nats, the key holds > 99.9 % of the softmax mass;
      grow / shrink: every query gets 2 x the pattern, the keys of tile t get g_t x the pattern (+ half their noise) with g_t = 0.75 t
        (grow: the row maximum first appears in the tail tile, each tile ~17 log2 units above the last, so the running maximum is
        raised -- O and l rescaled -- at every tile) or 0.75 (tail - t) (shrink: the first tile holds the maximum, no rescale);
      creep: as grow with g_t = 0.15 t (~3.5 log2 units per tile: below the deferral threshold of 6, so P grows past 1 before the
        rescale);
      vscale: creep, and the values multiplied by `vscale` (bf16: 2^100, the accumulators reach ~2^116; f16: 2^10)."""
    pat = torch.where(torch.arange(hd, device=q.device) % 2 == 0, 1.0, -1.0)
    tail, full_key = _tiles(N)
    if kind.startswith("dom_"):
        j = {"dom_last": N - 1, "dom_cls": 0, "dom_full": full_key}[kind]
        qs = torch.tensor(dominant_queries(N), device=q.device)
        q[qs] += 1.5 * pat
        k[j] = 1.5 * pat
        return
    if kind in ("grow", "shrink", "creep", "vscale"):
        q += 2.0 * pat
        t = torch.arange(N, device=q.device) // 64
        gt = {"grow": 0.75 * t, "shrink": 0.75 * (tail - t), "creep": 0.15 * t, "vscale": 0.15 * t}[kind].float()
        k.mul_(0.5).add_(gt[:, None, None] * pat)
        if kind == "vscale":
            v.mul_(vscale)
        return
    assert kind == "random", kind


def _seq_bound(q, k, v, scale, u, N, hd, f16):
    """float64 reference and elementwise bound of the kernel's output for one sequence: q / k / v (N, heads, hd) float64 holding the
    kernel's rounded operands.  -> (ref, bound), (heads, N, hd) each.

    The kernel (process_tile, store_strip) computes the scores s_j = fl(q.k_j) * scale * log2(e) in float32 (exact products, float32
    sums), P_j = round(exp2(s_j - m)) to the element type against a running maximum m <= max_j s_j (raised only when a tile's maximum
    exceeds it by more than 6, so P <= 64), O = sum_j P_j v_j and l = sum_j P_j on the matrix core in float32 (the SAME rounded P in
    both), O and l both rescaled when m is raised, out = round(O / l).  With w_j the exact softmax weights and ref = sum_j w_j v_j:
      * each P_j is w_j times a factor f_j = 2^(e_j) (1 + d_j), |d_j| <= u (u = 2^-8 bf16, 2^-11 half: the rounding of P) and
        |e_j| <= Ds, the float32 error of the score in log2 units, Ds = (hd + 4) 2^-24 log2(e) scale max_j sum_i |q_i k_ji| + 2^-22
        (the sums, the scale product, the subtraction of m and exp2's ulp);
      * O / l - ref = sum_j w_j (f_j - 1)(v_j - ref) / sum_j w_j f_j  (the sum of w_j (v_j - ref) is zero), so with
        rho = (1 + u) 2^Ds - 1:  |O / l - ref| <= rho / (1 - rho) * sum_j w_j |v_j - ref| <= rho / (1 - rho) (A + |ref|),
        A = sum_j w_j |v_j|;
      * the float32 sums of O and l (N terms), up to five rescales of both, 1 / l and the product add g (A + |ref|) with
        g = (N + 16) 2^-23;
      * the output rounding adds u |out|;
      * half only: P below half's smallest subnormal spacing (2^-24) is rounded with an ABSOLUTE error up to 2^-25; against
        l >= 1 (the row's maximal key has P >= 1) that adds N 2^-25 (max_j |v_j| + |ref|).
    bound = (rho / (1 - rho) + g)(A + |ref|)(1 + u) + u |ref| [+ the half term] -- of the form c 2^-8 sum_j p_j |v_j| + 2^-8 |ref|
    with c ~ 1 for bf16.  (bf16 has float32's exponent range: its subnormal P are below 2^-126 and drop out.)"""
    q, k, v = (t.transpose(0, 1) for t in (q, k, v))                         # (heads, N, hd)
    w = torch.softmax((q @ k.transpose(1, 2)) * scale, -1)
    ref = w @ v
    A = w @ v.abs()
    R = ref.abs()
    sabs = ((q.abs() @ k.abs().transpose(1, 2)) * scale * LOG2E).amax(-1, keepdim=True)
    ds = (hd + 4) * 2.0 ** -24 * sabs + 2.0 ** -22
    rho = (1 + u) * torch.exp2(ds) - 1
    g = (N + 16) * 2.0 ** -23
    bound = (rho / (1 - rho) + g) * (A + R) * (1 + u) + u * R
    if f16:
        bound = bound + N * 2.0 ** -25 * (v.abs().amax(1, keepdim=True) + R)
    return ref, bound


def seq_attention_case(dt, B, N, nh, hd, kinds, dev="cuda", tag=""):
    """ops.seq_attention on B sequences of N tokens, token-major (B, N, 3 nh hd) and head-major (3 nh, B N, hd) (seq_len = N): the two
    must agree bit for bit over the whole batch.  `kinds` {sequence: construction (see _construct)} shapes some sequences, the others
    are random; every sequence in `kinds` is compared with float64 over all heads and all query rows at the bound of _seq_bound, and
    must equal a B = 1 launch of itself bit for bit.  That equality covers the padded query rows of the last strip too: they vote in
    the strip's rescale decision, so the kernel stages them from the sequence's own first token; staged from the launch's first
    sequence, as they were, the "creep" sequence 2 of the 255-crop launch differed from its B = 1 launch."""
    from sam6d_amd import ops
    f16 = dt == F16
    u = 2.0 ** -11 if f16 else 2.0 ** -8
    vscale = 2.0 ** 10 if f16 else 2.0 ** 100
    scale = hd ** -0.5
    g = _gen(dev, 7000 + N + 31 * B + nh)
    x = torch.randn(B, N, 3, nh, hd, generator=g, device=dev)
    for b, kind in kinds.items():
        _construct(x[b, :, 0], x[b, :, 1], x[b, :, 2], kind, N, hd, vscale)
    qkv = x.reshape(B, N, 3 * nh * hd).to(dt)
    del x
    out = ops.seq_attention(qkv, nh, scale)
    assert out.shape == (B, N, nh * hd) and out.dtype == dt
    hm = qkv.view(B * N, 3 * nh, hd).transpose(0, 1).contiguous()
    out_hm = ops.seq_attention(hm, nh, scale, seq_len=N)
    assert torch.equal(out_hm, out), "head-major layout differs from token-major"
    del hm, out_hm
    worst, worst_err, s_err, n_err = 0.0, 0.0, 0.0, 0
    for b, kind in sorted(kinds.items()):
        xb = qkv[b].double().view(N, 3, nh, hd)
        ref, bound = _seq_bound(xb[:, 0], xb[:, 1], xb[:, 2], scale, u, N, hd, f16)
        got = out[b].double().view(N, nh, hd).transpose(0, 1)
        assert torch.isfinite(got).all(), (b, kind)
        sc = vscale if kind == "vscale" else 1.0
        err = (got - ref).abs()
        r = (err / bound).max().item()
        worst = max(worst, r)
        worst_err = max(worst_err, err.max().item() / sc)
        s_err += err.sum().item() / sc
        n_err += err.numel()
        if r > 1:
            bad = (err > bound).nonzero()[:5].tolist()                        # (head, query, d)
            raise AssertionError(f"sequence {b} ({kind}): err / bound {r:.3f}; first (head, query, d) outside: {bad}")
        one = ops.seq_attention(qkv[b:b + 1].contiguous(), nh, scale)
        assert torch.equal(one[0], out[b]), f"sequence {b} ({kind}) differs from its B = 1 launch"
    util.record_margin(f"seq_attention_{'f16' if f16 else 'bf16'}_B{B}_N{N}_nh{nh}{tag}", max_err_over_bound=worst, bound_ratio=1.0,
                       max_abs=worst_err, mean_abs=s_err / max(n_err, 1))


# sampled sequences of the production launches and their constructions (the others are random)
DINO_KINDS = {0: "random", 1: "dom_last", 2: "creep", 127: "dom_cls", 128: "dom_full", 200: "vscale", 253: "grow", 254: "shrink"}
PEM_KINDS = {0: "random", 1: "dom_last", 2: "creep", 15: "dom_cls", 16: "dom_full", 20: "vscale", 30: "grow", 31: "shrink"}


def test_seq_attention_bf16_at_255_crops():
    """The descriptor ViT's attention on a full batch of the frame batcher: 255 crops x 16 heads x 257 tokens (4 tiles + 1 key)."""
    seq_attention_case(BF, 255, 257, 16, 64, DINO_KINDS)


def test_seq_attention_f16_at_the_pem_batch():
    """The PEM ViT-B's attention in IEEE half at its batch: 32 sequences x 12 heads x 197 tokens (3 tiles + 5 keys)."""
    seq_attention_case(F16, 32, 197, 12, 64, PEM_KINDS)


# ------------------------------------------------------------------------------------------------------------------------------
# the folded block loop's kernels (DinoVisionTransformer._blocks_fused) at 65,535 and 32,896 token rows

SENTINEL = -3.25


def _stream(g, dev, M, C, pad):
    """A residual stream (M, C) bf16 with rows of different scale and offset, inside a (M + pad, C) buffer whose rows past M hold a
    sentinel."""
    buf = torch.full((M + pad, C), SENTINEL, dtype=BF, device=dev)
    x = torch.randn(M, C, generator=g, device=dev) * (0.5 + 2 * torch.rand(M, 1, generator=g, device=dev))
    buf[:M] = (x + torch.randn(M, 1, generator=g, device=dev)).to(BF)
    return buf


def _linear(g, dev, N, K):
    return (torch.randn(N, K, generator=g, device=dev) / K ** 0.5), torch.randn(N, generator=g, device=dev)


def _ln_params(g, dev, C):
    return 1 + 0.3 * torch.randn(C, generator=g, device=dev), 0.2 * torch.randn(C, generator=g, device=dev)


def _blocks(M, rows=8192):
    return [(r0, min(M, r0 + rows)) for r0 in range(0, M, rows)]


def _stats_errors(st, ref_rows, acc):
    """Accumulate the row-statistics distances of test_residual_gemm_row_statistics: |mean - mean64| and |sigma / sigma64 - 1|."""
    mean = ref_rows.mean(1)
    sigma = torch.sqrt(ref_rows.var(1, unbiased=False) + 1e-6)
    acc["mean"] = max(acc.get("mean", 0.0), (st[:, 0].double() - mean).abs().max().item())
    acc["sigma"] = max(acc.get("sigma", 0.0), ((st[:, 1].double() - sigma).abs() / sigma).max().item())
    acc["amax"] = max(acc.get("amax", 0.0), ref_rows.abs().max().item())


def _check_stats(acc, what, M):
    bm = 2e-6 * (1 + acc["amax"])
    util.record_margin(f"{what}_M{M}", mean_abs=acc["mean"], bound_mean=bm, sigma_rel=acc["sigma"], bound_sigma=2e-5)
    assert acc["mean"] <= bm, (what, acc)
    assert acc["sigma"] <= 2e-5, (what, acc)


def _lnfold_check(x, st, W, b, gamma, beta, gelu, what, M):
    """gemm_bf16_lnfold against the float64 folded form (one bf16 rounding) and float64 LayerNorm -> Linear (relative rms 3e-3)."""
    from sam6d_amd import ops
    from sam6d_amd.utils.linear import lnfold_weights
    from tests.test_gpu_gemm import _check
    wf, cs, bf = lnfold_weights(W, b, gamma, beta)
    out = ops.gemm_bf16_lnfold(x, st, wf, cs, bf, gelu=gelu)
    assert out.shape == (M, W.shape[0])
    wf64, cs64, bf64, W64, b64 = wf.double(), cs.double(), bf.double(), W.double(), b.double()
    num = den = worst = 0.0
    for r0, r1 in _blocks(M):
        xd = x[r0:r1].double()
        mu, rs = st[r0:r1, :1].double(), 1.0 / st[r0:r1, 1:].double()
        folded = rs * (xd @ wf64.t() - mu * cs64[None, :]) + bf64[None, :]
        true = F.layer_norm(xd, (x.shape[1],), gamma.double(), beta.double(), 1e-6) @ W64.t() + b64
        if gelu:
            folded, true = F.gelu(folded), F.gelu(true)
        o = out[r0:r1]
        _check(o, folded.float(), f"{what} rows {r0}")
        worst = max(worst, ((o.double() - folded).abs() / (2.0 ** -8 * folded.abs() + 1e-5)).max().item())
        num += (o.double() - true).pow(2).sum().item()
        den += true.pow(2).sum().item()
    rel = math.sqrt(num / den)
    util.record_margin(f"{what}_M{M}", err_over_one_rounding=worst, bound_rounding=1.01, rel_rms_vs_layernorm_linear=rel, bound_rel=3e-3)
    assert rel <= 3e-3, (what, rel)
    return out


def _residual_check(a, W, b, buf, M, what):
    """gemm_bf16(a, W, b, residual=x, out=x, stats_partial=sp) in place on the stream: the sum within one bf16 rounding of float64,
    ln_stats_finalize at the bounds of test_residual_gemm_row_statistics, rows past M and the words behind sp untouched."""
    from sam6d_amd import ops
    from tests.test_gpu_gemm import _check
    C = W.shape[0]
    x2 = buf[:M]
    before = x2.clone()
    spbuf = torch.full((C // 32 * 2 * M + 4096,), SENTINEL, device=buf.device)
    sp = spbuf[:C // 32 * 2 * M].view(C // 32, 2, M)
    wb = W.to(BF)
    got = ops.gemm_bf16(a, wb, b, residual=x2, out=x2, stats_partial=sp)
    assert got.data_ptr() == x2.data_ptr()
    assert bool((buf[M:] == SENTINEL).all()), f"{what}: rows past M written"
    assert bool((spbuf[sp.numel():] == SENTINEL).all()), f"{what}: words behind the partial statistics written"
    assert torch.isfinite(sp).all()
    st = ops.ln_stats_finalize(sp, 32, 1e-6)
    acc = {}
    worst = 0.0
    w64, b64 = wb.double(), b.double()
    for r0, r1 in _blocks(M):
        ref = a[r0:r1].double() @ w64.t() + b64 + before[r0:r1].double()
        _check(x2[r0:r1], ref.float(), f"{what} rows {r0}")
        worst = max(worst, ((x2[r0:r1].double() - ref).abs() / (2.0 ** -8 * ref.abs() + 1e-5)).max().item())
        _stats_errors(st[r0:r1], ref, acc)
    util.record_margin(f"{what}_sum_M{M}", err_over_one_rounding=worst, bound_rounding=1.01)
    _check_stats(acc, f"{what}_stats", M)
    return st


def folded_block_case(M, C=1024, hidden=4096, dev="cuda", pad=256, seed=0):
    """One block of the folded loop at M rows, in _blocks_fused's call order and shapes: row_stats -> lnfold qkv (N = 3C) -> residual
    proj (K = C) + statistics -> ln_stats_finalize -> lnfold fc1 + GELU (N = hidden) -> residual fc2 (K = hidden) + statistics, then
    the final add_layernorm(x, None, ...).  The attention output that feeds proj is a seeded stand-in (its kernel is tested above)."""
    from sam6d_amd import ops
    g = _gen(dev, 9000 + M + C + seed)
    buf = _stream(g, dev, M, C, pad)
    x2 = buf[:M]
    st = ops.row_stats(x2, 1e-6)
    acc = {}
    for r0, r1 in _blocks(M):
        _stats_errors(st[r0:r1], x2[r0:r1].double(), acc)
    _check_stats(acc, f"row_stats_C{C}", M)
    gamma, beta = _ln_params(g, dev, C)
    W, b = _linear(g, dev, 3 * C, C)
    qkv = _lnfold_check(x2, st, W, b, gamma, beta, False, f"lnfold_qkv_C{C}", M)
    assert bool((buf[M:] == SENTINEL).all())
    del qkv
    o = torch.randn(M, C, generator=g, device=dev).to(BF)
    W, b = _linear(g, dev, C, C)
    st = _residual_check(o, W, b, buf, M, f"residual_proj_K{C}")
    del o
    gamma, beta = _ln_params(g, dev, C)
    W, b = _linear(g, dev, hidden, C)
    h = _lnfold_check(x2, st, W, b, gamma, beta, True, f"lnfold_fc1_gelu_N{hidden}", M)
    W, b = _linear(g, dev, C, hidden)
    _residual_check(h, W, b, buf, M, f"residual_fc2_K{hidden}")
    del h
    # the final norm: add_layernorm(x, None, gamma, beta) on the stream
    gamma, beta = _ln_params(g, dev, C)
    xo, y = ops.add_layernorm(x2, None, gamma, beta, 1e-6)
    assert xo is x2 and y.shape == x2.shape
    assert bool((buf[M:] == SENTINEL).all())
    worst = 0.0
    for r0, r1 in _blocks(M):
        xd = x2[r0:r1].double()
        mean = xd.mean(1, keepdim=True)
        sigma = torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + 1e-6)
        xh = (xd - mean) / sigma
        ref = xh * gamma.double() + beta.double()
        # one bf16 rounding of the output, and the float32 statistics at the row_stats bounds above (mean within 2e-6 (1 + max |x|),
        # sigma within 2e-5 relative) carried through gamma (x - mean) / sigma
        tol = 2.0 ** -8 * ref.abs() + gamma.double().abs() * (2e-6 * (1 + xd.abs().max()) / sigma + 2e-5 * xh.abs()) + 1e-6
        r = ((y[r0:r1].double() - ref).abs() / tol).max().item()
        worst = max(worst, r)
    util.record_margin(f"final_add_layernorm_C{C}_M{M}", err_over_bound=worst, bound=1.01)
    assert worst <= 1.01, worst


@pytest.mark.parametrize("M", [255 * 257, 128 * 257])
def test_folded_block_kernels_at_production_rows(M):
    """65,535 rows (255 crops: 256 row tiles, the last one 255 rows) and 32,896 (128 crops, the per-frame chunk)."""
    folded_block_case(M)


# ------------------------------------------------------------------------------------------------------------------------------
# the whole descriptor path: batch invariance

FRAME_SEEDS = (11, 12, 13)
FRAME_PROPOSALS = (120, 150, 60)          # 330 crops: one batch of 255 (frame 0, frame 1 up to 134), the rest (75) straddles frames 1 / 2
SAMPLED_CROPS = (0, 127, 128, 254, 255, 329)


def _desc(model, chunk=128):
    from tests.test_gpu_dinov2 import _custom
    return _custom(model, 224, chunk=chunk)


def test_descriptor_path_is_batch_invariant(monkeypatch):
    """_FrameBatcher / _detect_group promise the values of per-frame calls: a crop's row depends on no other crop of its batch.  A
    seeded ViT-L in bf16 (default policy) on three frames of 120 / 150 / 60 proposals: forward_frames batches crops 0..254 across
    frames 0 and 1 and runs the remaining 75 (plan_chunks) across frames 1 and 2; forward(frame) runs chunks of 128, 128 + 22 and 60.
    Every frame's cls and patch descriptors must be the per-frame ones bit for bit, and sampled crops run alone (B = 1) must equal
    their rows.  16 sampled crops are also held to the device fp32 path (pinned to the reference golden by test_gpu_dinov2.py) at the
    error model's E_BLOCK_L * sqrt(25), which ties the 255-batch values to the reference and not only to themselves."""
    import numpy as np

    from sam6d_amd.ism import dinov2 as pd
    from sam6d_amd.utils import seeded, synth
    from tests.test_gpu_dinov2 import E_BLOCK_L
    monkeypatch.setenv("S6D_DINO_DTYPE", "bf16")
    m = seeded.load_seeded(pd._make_dinov2_model(arch_name="vit_large").eval(), 3).cuda()
    o = _desc(m)
    frames = [synth.dinov2_inputs(P=p, seed=s) for p, s in zip(FRAME_PROPOSALS, FRAME_SEEDS)]
    for f in frames:
        assert pd.crop_valid(f["boxes"].numpy(), 224).all()
    props = [types.SimpleNamespace(masks=f["masks"].cuda(), boxes=f["boxes"].cuda()) for f in frames]
    assert pd.plan_chunks(sum(FRAME_PROPOSALS) - pd._FrameBatcher.FULL) == [sum(FRAME_PROPOSALS) - pd._FrameBatcher.FULL]
    batched = o.forward_frames([f["image"] for f in frames], props)
    for i, f in enumerate(frames):
        cls, patch = o.forward(f["image"], props[i])
        assert torch.equal(batched[i][0], cls), f"frame {i}: cls descriptors depend on the batch"
        assert torch.equal(batched[i][1], patch), f"frame {i}: patch descriptors depend on the batch"
    cls_all = torch.cat([b[0] for b in batched])
    patch_all = torch.cat([b[1] for b in batched])
    crops = [o._crops(f["image"], p.masks, p.boxes, True, True) for f, p in zip(frames, props)]
    rgbs, masks = torch.cat([c[0] for c in crops]), torch.cat([c[1] for c in crops])
    assert rgbs.shape[0] == cls_all.shape[0] == sum(FRAME_PROPOSALS)
    for i in SAMPLED_CROPS:
        c1, p1 = o.compute_cls_and_patch_features(rgbs[i:i + 1], masks[i:i + 1])
        assert torch.equal(c1[0], cls_all[i]) and torch.equal(p1[0], patch_all[i]), f"crop {i} alone differs from its batched row"
    # the fp32 device path on 16 sampled crops
    pick = sorted(set(SAMPLED_CROPS) | set(torch.randperm(cls_all.shape[0], generator=torch.Generator().manual_seed(5))[:10].tolist()))
    monkeypatch.setenv("S6D_DINO_DTYPE", "fp32")
    c32, p32 = o.compute_cls_and_patch_features(rgbs[pick], masks[pick])
    bound = E_BLOCK_L * 25 ** 0.5
    c16, p16 = cls_all[pick], patch_all[pick]
    rel_c = ((c16 - c32).norm(dim=-1) / c32.norm(dim=-1)).cpu().numpy()
    # patch descriptors (unit vectors, masked rows zero in both): rms of the difference relative to the fp32 rms over the sampled
    # crops, as test_vit_l14_bf16_vs_reference_golden pools its sample
    rel_p = ((p16 - p32).pow(2).sum() / p32.pow(2).sum()).sqrt().item()
    util.record_margin("dinov2_batched_vs_fp32", n_crops=len(pick), cls_rel_max=float(rel_c.max()), patch_rel_rms=rel_p, bound=bound)
    assert np.all(rel_c <= bound), rel_c
    assert rel_p <= bound, rel_p
