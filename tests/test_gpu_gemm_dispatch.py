"""The GEMM launcher (gemm_launch of csrc/s6d_gemm.hip, gemm4_launch of csrc/s6d_gemm4.hip) seen through the C entry points: which
status a call gets, and that every kernel instantiation the launcher can select launches and computes its product.

The shapes are the smallest that still tell the launcher's branches apart: M = 8 (every kernel pads rows to its tile; the four-wave
form takes whole 256-row tiles only, so its runs use M = 256), N = 256 (the 256 x 256 kernels) and 384 (N % 256 == 128: the
256 x 128 kernel), K = 128 (two K tiles of bf16 / half, one of fp8).

STATUS holds the codes of the launcher as it stood BEFORE its macros and ladders were replaced by kernel tables (read from its rules;
this module was run against the host build of that commit, unchanged, and passed there): the table pins behaviour.  One row differs
from what one would first write down: with M = 0 the three entry points that hand everything to gemm_launch return S6D_OK for NULL
operands, but the five that check operands of their own first (scales, residual, row statistics) return S6D_EINVAL for THOSE being
NULL before M is looked at -- both rows are in the table.  Refused calls launch nothing.

Bounds: those of the existing tests of each form, nothing new -- bf16: one bf16 rounding of the float product, 2^-8 |ref| + 1e-5,
times 1.01 (tests/test_emu_gemm.py::_check, tests/test_gpu_gemm.py::_check); half: test_float16_gemm_vs_float; fp8 forms:
tests/test_gpu_fp8.py."""
import pytest
import torch

from sam6d_amd import _lib
from sam6d_amd.utils import fp8

OK, EINVAL, EUNSUPPORTED = 0, -1, -3                 # S6D_OK, S6D_EINVAL, S6D_EUNSUPPORTED of include/sam6d_hip.h

ENTRIES = ("s6d_gemm_bf16", "s6d_gemm_bf16_cblk", "s6d_gemm_f16", "s6d_gemm_bf16_res", "s6d_gemm_bf16_lnfold", "s6d_gemm_fp8",
           "s6d_gemm_fp8_gelu_mx", "s6d_gemm_fp8_mxa")


def _call(ops, entry, o, M, N, K, epilogue=0, col_block=0, lda=None, ldc=None, blocks=0):
    """One call of a C entry point with the operands of dict o (tensors or None = NULL); returns the status."""
    p = {k: ops._ptr(v) for k, v in o.items()}
    lda = K if lda is None else lda                     # strides in elements (the fp8 forms: bytes), as ops.py passes them
    ldc = N if ldc is None else ldc
    st = ops._stream()
    if entry in ("s6d_gemm_bf16", "s6d_gemm_f16"):
        args = (p["a"], lda, p["w"], K, p["bias"], p["c"], ldc, M, N, K, epilogue, blocks, st)
    elif entry == "s6d_gemm_bf16_cblk":
        args = (p["a"], lda, p["w"], K, p["bias"], p["c"], ldc, M, N, K, epilogue, col_block, blocks, st)
    elif entry == "s6d_gemm_bf16_res":
        args = (p["a"], lda, p["w"], K, p["bias"], p["r"], N, p.get("sp"), p["c"], ldc, M, N, K, blocks, st)
    elif entry == "s6d_gemm_bf16_lnfold":
        args = (p["a"], lda, p["rs"], p["w"], K, p["cs"], p["bias"], p["c"], ldc, M, N, K, epilogue, col_block, blocks, st)
    elif entry == "s6d_gemm_fp8":
        args = (p["a"], lda, p["sa"], p["w"], K, p["sw"], p["bias"], p["c"], ldc, M, N, K, epilogue, blocks, st)
    elif entry == "s6d_gemm_fp8_gelu_mx":
        args = (p["a"], lda, p["sa"], p["w"], K, p["sw"], p["bias"], p["c"], ldc, p["sc"], M, N, K, blocks, st)
    elif entry == "s6d_gemm_fp8_mxa":
        args = (p["a"], lda, p["sa"], p["w"], K, p["sw"], p["bias"], p["c"], ldc, M, N, K, epilogue, blocks, st)
    else:
        raise KeyError(entry)
    return ops._fn(entry, len(args))(*args)


def _operands(entry, M, N, K, ldc=None, seed=0):
    """Valid, fully sized operands of one entry point on the device (so that a call the table expects to be refused would still be
    harmless if it were not) -- and, for the launches, what the reference needs."""
    g = torch.Generator().manual_seed(1000 * seed + M + N + K)
    ldc = N if ldc is None else ldc
    rows = max(M, 1)
    o = {}
    if "fp8" in entry:
        if entry == "s6d_gemm_fp8_mxa":              # block scales that differ by up to 2^12 (test_gemm_fp8_mx_activations_vs_float)
            a = torch.randn(rows, K, generator=g) * torch.exp2(torch.randint(-6, 7, (rows, K // 32), generator=g).float()).repeat_interleave(32, 1)
            qa, s = fp8.quantize_blocks(a)
            sa = torch.zeros((rows + 255) // 256 * 256, K // 32, dtype=torch.uint8)     # scale dwords of whole 256-row tiles are read
            sa[:rows] = s
        else:
            a = torch.randn(rows, K, generator=g) * torch.exp2(torch.randint(-3, 4, (rows, 1), generator=g).float())
            qa, sa = fp8.quantize_rows(a)
        w = torch.randn(N, K, generator=g) / K ** 0.5 * torch.exp2(torch.randint(-3, 4, (N, 1), generator=g).float())
        qw, sw = fp8.quantize_rows(w)
        o.update(a=qa, sa=sa, w=qw, sw=sw)
        if entry == "s6d_gemm_fp8_gelu_mx":
            o.update(c=torch.zeros(rows, ldc, dtype=torch.uint8), sc=torch.zeros(rows, max(N // 32, 1), dtype=torch.uint8))
        else:
            o.update(c=torch.zeros(rows, ldc, dtype=torch.bfloat16))
    else:
        dt = torch.float16 if entry == "s6d_gemm_f16" else torch.bfloat16
        o.update(a=torch.randn(rows, K, generator=g).to(dt), w=(torch.randn(N, K, generator=g) / K ** 0.5).to(dt),
                 c=torch.zeros(rows, ldc, dtype=dt))
        if entry == "s6d_gemm_bf16_res":
            o.update(r=torch.randn(rows, N, generator=g).to(dt))
        if entry == "s6d_gemm_bf16_lnfold":
            x = o["a"].float()
            o.update(rs=torch.stack([x.mean(1), torch.sqrt(x.var(1, unbiased=False) + 1e-6)], 1).contiguous(),
                     cs=o["w"].float().sum(1).contiguous())
    o["bias"] = torch.randn(N, generator=g)
    return {k: v.cuda() for k, v in o.items()}


# entry point, M, N, K, epilogue, col_block, what is special, expected status
STATUS = [
    ("s6d_gemm_bf16", 8, 192, 128, 0, 0, "", EINVAL),                    # N is no multiple of 128
    ("s6d_gemm_bf16", 8, 256, 96, 0, 0, "", EINVAL),                     # K is no multiple of the K step
    ("s6d_gemm_bf16", 8, 256, 128, 2, 0, "", EINVAL),                    # the plain entry point has epilogues 0 and 1
    ("s6d_gemm_bf16_cblk", 8, 256, 128, 0, 12, "", EINVAL),              # column blocks are multiples of 8 ...
    ("s6d_gemm_bf16_cblk", 8, 256, 128, 0, 48, "", EINVAL),              # ... that divide N
    ("s6d_gemm_bf16_cblk", 8, 256, 128, 0, -8, "", EINVAL),
    ("s6d_gemm_bf16", 8, 256, 128, 0, 0, "ldc+4", EINVAL),               # output rows of whole 16 bytes
    ("s6d_gemm_bf16", 8, 384, 128, 0, 0, "ldc+4", EINVAL),
    ("s6d_gemm_bf16", 8, 256, 128, 0, 0, "ldc-8", EINVAL),               # ldc < N
    ("s6d_gemm_bf16", 8, 256, 128, 0, 0, "lda-8", EINVAL),               # lda < K
    ("s6d_gemm_bf16", 8, 256, 128, 0, 0, "lda+4", EINVAL),
    ("s6d_gemm_bf16", 8, 256, 128, 0, 0, "null-a", EINVAL),
    ("s6d_gemm_bf16", 8, 256, 128, 0, 0, "null-c", EINVAL),
    ("s6d_gemm_bf16", -1, 256, 128, 0, 0, "", EINVAL),
    ("s6d_gemm_bf16", 8, 256, 128, 0, 0, "lda-huge", EUNSUPPORTED),      # staging addresses are 32-bit byte offsets from A
    ("s6d_gemm_bf16_cblk", 8, 384, 128, 0, 64, "", EUNSUPPORTED),        # column blocks: the 256 x 256 kernel only
    ("s6d_gemm_bf16_res", 8, 384, 128, 0, 0, "", EUNSUPPORTED),
    ("s6d_gemm_bf16_res", 8, 256, 128, 0, 0, "null-r", EINVAL),
    ("s6d_gemm_bf16_lnfold", 8, 384, 128, 0, 0, "", EUNSUPPORTED),
    ("s6d_gemm_bf16_lnfold", 8, 256, 128, 2, 0, "", EINVAL),             # gelu is 0 or 1
    ("s6d_gemm_bf16_lnfold", 8, 256, 128, 0, 0, "null-bias", EINVAL),    # the folded form always has a bias (b + W beta)
    ("s6d_gemm_bf16_lnfold", 8, 256, 128, 0, 48, "", EINVAL),
    ("s6d_gemm_f16", 8, 384, 128, 0, 0, "", EUNSUPPORTED),
    ("s6d_gemm_f16", 8, 256, 128, 2, 0, "", EINVAL),
    ("s6d_gemm_f16", 8, 256, 96, 0, 0, "", EINVAL),
    ("s6d_gemm_fp8", 8, 384, 128, 0, 0, "", EUNSUPPORTED),
    ("s6d_gemm_fp8", 8, 256, 64, 0, 0, "", EUNSUPPORTED),                # the fp8 K step is 128
    ("s6d_gemm_fp8", 8, 256, 128, 2, 0, "", EINVAL),
    ("s6d_gemm_fp8", 8, 256, 128, 0, 0, "null-sa", EINVAL),
    ("s6d_gemm_fp8_gelu_mx", 8, 384, 128, 0, 0, "", EUNSUPPORTED),
    ("s6d_gemm_fp8_gelu_mx", 8, 256, 64, 0, 0, "", EUNSUPPORTED),
    ("s6d_gemm_fp8_gelu_mx", 8, 256, 128, 0, 0, "ldc+8", EINVAL),        # byte rows of whole 16 bytes
    ("s6d_gemm_fp8_mxa", 8, 384, 128, 0, 0, "", EUNSUPPORTED),
    ("s6d_gemm_fp8_mxa", 8, 256, 64, 0, 0, "", EUNSUPPORTED),
    ("s6d_gemm_fp8_mxa", 8, 256, 128, 3, 0, "", EINVAL),
] + [(e, 0, 256, 128, 0, 0, "null-acw", OK) for e in ENTRIES] + [        # an empty row batch: nothing is looked at, nothing launched
    (e, 0, 256, 128, 0, 0, "null-all", OK if e in ("s6d_gemm_bf16", "s6d_gemm_bf16_cblk", "s6d_gemm_f16") else EINVAL) for e in ENTRIES]


def check_status_table(ops):
    bad = []
    for entry, M, N, K, epi, cb, special, want in STATUS:
        ldc = N + 4 if special == "ldc+4" else N + 8 if special == "ldc+8" else N
        o = _operands(entry, max(M, 0), N, K, ldc=ldc)
        lda = {"lda-8": K - 8, "lda+4": K + 4, "lda-huge": 1 << 28}.get(special)
        if special == "ldc-8":
            ldc = N - 8
        if special == "null-all":
            o = {k: None for k in o}
        elif special == "null-acw":
            o.update(a=None, c=None, w=None)
        elif special.startswith("null-"):
            o[special[5:]] = None
        got = _call(ops, entry, o, M, N, K, epi, cb, lda=lda, ldc=ldc)
        if got != want:
            bad.append((entry, M, N, K, epi, cb, special, "expected", want, "got", got))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ every instantiation launches
def _within(out, ref, what, rel=2.0 ** -8, extra=1e-5):
    err = (out.float().cpu().double() - ref.double()).abs()
    tol = rel * ref.double().abs() + extra
    bad = int((err > 1.01 * tol).sum())
    assert bad == 0, f"{what}: {bad} of {ref.numel()} outside the bound (max err / tol {(err / tol).max().item():.3f})"


class _Launch:
    """One (entry point, epilogue, bias) combination at one shape: operands and reference are made once and stay unchanged; run()
    launches into a fresh output under whatever switches are in force and checks status and result."""

    def __init__(self, entry, M, N, K, epi, bias):
        self.entry, self.M, self.N, self.K, self.epi, self.bias = entry, M, N, K, epi, bias
        self.what = f"{entry} N={N} epilogue={epi} bias={bias} M={M}"
        o = self.o = _operands(entry, M, N, K, seed=7 + epi + 10 * bias)
        if not bias:
            o["bias"] = None
        b = 0.0 if o["bias"] is None else o["bias"].cpu().double()
        gelu = torch.nn.functional.gelu
        if "fp8" in entry:
            dw = fp8.dequantize_rows(o["w"].cpu(), o["sw"].cpu()).double()
            if entry == "s6d_gemm_fp8_mxa":
                da = fp8.dequantize_blocks(o["a"].cpu(), o["sa"].cpu()[:M].reshape(M, K // 32)).double()
            else:
                da = fp8.dequantize_rows(o["a"].cpu(), o["sa"].cpu()).double()
            ref = da @ dw.t() + b
            self.mag = (da.abs() @ dw.abs().t()).float()
            self.ref = (gelu(ref) if epi in (1, 5) else ref).float()
            if epi == 5:
                # the inputs keep every block maximum away from a binade edge of the scale rule (448 2^e), where a last-bit difference
                # of the kernel's fp32 GELU would legitimately move the scale byte: a property of the reference alone
                amax = self.ref.view(M, N // 32, 32).abs().amax(2).double()
                frac = torch.log2(amax / 448.0)
                assert ((frac - frac.round()).abs() > 1e-3).all(), "test inputs: a block maximum sits on a binade edge"
            return
        a, w = o["a"].cpu().double(), o["w"].cpu().double()
        if entry == "s6d_gemm_bf16_lnfold":
            mu, rs = o["rs"].cpu()[:, :1].double(), 1.0 / o["rs"].cpu()[:, 1:].double()
            ref = rs * (a @ w.t() - mu * o["cs"].cpu().double()[None, :]) + b
        else:
            ref = a @ w.t() + b
        if entry == "s6d_gemm_bf16_res":
            ref = ref + o["r"].cpu().double()
        self.ref = (gelu(ref) if epi == 1 else ref).float()

    def run(self, ops, tag):
        o, M, N = dict(self.o), self.M, self.N
        o["c"] = torch.zeros_like(self.o["c"])
        if "sc" in o:
            o["sc"] = torch.zeros_like(self.o["sc"])
        what = f"{self.what} [{tag}]"
        st = _call(ops, self.entry, o, M, N, self.K, self.epi)
        assert st == OK, f"{what}: status {st}"
        torch.cuda.synchronize()
        out = o["c"]
        if self.entry == "s6d_gemm_fp8_gelu_mx":                  # the checks of test_gemm_fp8_gelu_mx_output_vs_float
            rq, rs = fp8.quantize_blocks(self.ref)
            s_, q_ = o["sc"].cpu(), out.cpu()
            ds = (s_.int() - rs.int()).abs()
            assert ds.max() <= 1 and (ds != 0).float().mean() < 1e-2, (what, ds.max().item(), (ds != 0).float().mean().item())
            got = fp8.dequantize_blocks(q_, s_)
            amax = self.ref.view(M, N // 32, 32).abs().amax(2, keepdim=True).expand(-1, -1, 32).reshape(M, N)
            assert ((got - self.ref).abs() <= 2.0 ** -4 * amax * 1.01 + 1e-30).all(), what
        elif self.entry == "s6d_gemm_fp8":                        # test_gemm_fp8_vs_float_on_the_quantised_operands
            err = (out.float().cpu() - self.ref).abs()
            tol = 2.0 ** -8 * self.ref.abs() + 2.0 ** -16 * self.mag + 1e-30
            assert (err <= tol * 1.01 + (1e-5 if self.epi == 1 else 0)).all(), (what, (err / tol).max().item())
        elif self.entry == "s6d_gemm_fp8_mxa":                    # test_gemm_fp8_mx_activations_vs_float (block scales 2^12 apart)
            err = (out.float().cpu() - self.ref).abs()
            tol = 2.0 ** -8 * self.ref.abs() + 2.0 ** -14 * self.mag + 1e-30
            assert (err <= tol * 1.01 + (1e-5 if self.epi == 1 else 0)).all(), (what, (err / tol).max().item())
        elif self.entry == "s6d_gemm_f16":                        # test_float16_gemm_vs_float
            err = (out.float().cpu().double() - self.ref.double()).abs()
            assert (err <= 2.0 ** -11 * self.ref.double().abs() * 1.01 + 2e-5).all(), what
        else:
            _within(out, self.ref, what)


def _combos(N):
    """(entry point, epilogue, bias) of every kernel family the launcher serves at this N."""
    c = [("s6d_gemm_bf16", e, b) for e in (0, 1) for b in (True, False)]
    if N % 256 == 0:
        c += [("s6d_gemm_bf16_res", 0, b) for b in (True, False)]                       # EPI 2
        c += [("s6d_gemm_bf16_lnfold", e, True) for e in (0, 1)]                        # EPI 3 / 4: always with a bias
        c += [("s6d_gemm_f16", e, b) for e in (0, 1) for b in (True, False)]
        c += [("s6d_gemm_fp8", e, b) for e in (0, 1) for b in (True, False)]
        c += [("s6d_gemm_fp8_gelu_mx", 5, b) for b in (True, False)]                    # EPI 5
        c += [("s6d_gemm_fp8_mxa", e, b) for e in (0, 1) for b in (True, False)]
    return c


# (N, small_tile, mfma_shape) on the host build: every instantiation of the eight-wave and the 256 x 128 kernels once -- small_tile 0
# keeps N = 256 on the 256 x 256 kernels, 2 sends its plain / GELU / residual launches to the 256 x 128 kernel; the matrix-instruction
# shape matters to the bf16 kernels only; N = 384 under the library's own choices (1, 0)
EMU_SETTINGS = [(256, 0, 32, "all"), (256, 0, 16, "bf16"), (256, 2, 32, "small"), (256, 2, 16, "small-bf16"), (384, 1, 0, "all")]
GPU_SETTINGS = [(N, small, shape, "all") for N in (256, 384) for small in (0, 1, 2) for shape in (0, 16, 32)]


def check_launches(ops, settings, wave_tiles=(0,), K=128):
    cache = {}

    def launch(entry, M, N, epi, bias):
        key = (entry, M, N, epi, bias)
        if key not in cache:
            cache[key] = _Launch(entry, M, N, K, epi, bias)
        return cache[key]

    L = _lib.lib()
    n = 0
    try:
        for wt in wave_tiles:
            assert L.s6d_set_gemm_wave_tile(wt) == OK
            # the four-wave form takes whole 256-row tiles (and 32x32x16 only): under 128 the runs that can reach it use M = 256
            M = 256 if wt == 128 else 8
            for N, small, shape, which in settings:
                assert L.s6d_set_gemm_small_tile(small) == OK and L.s6d_set_gemm_mfma_shape(shape) == OK
                for entry, epi, bias in _combos(N):
                    is_bf16 = entry in ("s6d_gemm_bf16", "s6d_gemm_bf16_res", "s6d_gemm_bf16_lnfold")
                    if "bf16" in which and not is_bf16:
                        continue
                    if "small" in which and (entry == "s6d_gemm_bf16_lnfold" or "fp8" in entry):
                        continue                                         # the small-tile switch does not reach these forms
                    launch(entry, M if "fp8" not in entry else 8, N, epi, bias).run(ops, f"small_tile={small} mfma_shape={shape} wave_tile={wt}")
                    n += 1
    finally:
        L.s6d_set_gemm_wave_tile(0)
        L.s6d_set_gemm_mfma_shape(0)
        L.s6d_set_gemm_small_tile(1)
    return n


@pytest.mark.gpu
def test_status_codes():
    from sam6d_amd import ops
    check_status_table(ops)


@pytest.mark.gpu
@pytest.mark.parametrize("wave_tile", [0, 64, 128])
def test_every_instantiation_launches_and_is_right(wave_tile):
    from sam6d_amd import ops
    n = check_launches(ops, GPU_SETTINGS, (wave_tile,))
    assert n == 9 * (22 + 4)
