"""The block loop of the three ViTs (sam6d_amd/utils/vit_blocks.py) in every form a model can choose: the ordered trace of the
launches against tests/golden/vit_block_traces.json -- recorded from the commit named in that file, before the three models' own
copies of the loop were folded into one (tools/gen_vit_block_traces.py) -- and the output against the float32 statement of the
module.  Shapes: the smallest at which each loop can go wrong, dim 256 so that the 256 x 256-tile kernel takes every GEMM.

Bounds (relative rms against float32), none of them new:
  * 8e-3 for a bf16 stream, and the folded form not further away than 1.1 x the add + LayerNorm form + 5e-4
    (tests/test_emu_sam.py::test_folded_block_loops_against_the_round2_form_and_float);
  * 2e-3 for the PEM extractor's IEEE-half stream (tests/test_emu_attn.py::test_pem_vit_fused_half_pipeline_on_the_emulator: half's
    2^-11 per stored activation).  Its bf16 stream (S6D_GEMM_RES=1) stores the same activations of the same 8 blocks with a
    rounding unit of 2^-8, so it is held to 2^3 x that bound = 1.6e-2: the 8e-3 above is the bound of a 2-block stack and no
    statement about 8 blocks (figures on the emulator: half 1.1e-3, bf16 8.6e-3 at the last tap, the same 1.8 below either bound);
  * the fp8 forms against the bf16 loop, E_BLOCK_FP8 per block in quadrature (tests/test_emu_fp8.py::
    test_fp8_block_loop_on_the_emulator): e4m3 operands cannot meet a bf16 bound against float32.
tests/test_emu_vit_blocks.py runs the same bodies on the emulator."""
import contextlib
import inspect
import json
import os
from functools import partial

import pytest
import torch

from tests.test_gpu_fp8 import E_BLOCK_FP8

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vit_block_traces.json")
TRACED = ("row_stats", "ln_stats_finalize", "gemm_bf16", "gemm_bf16_lnfold", "gemm_fp8", "gemm_fp8_gelu_mx", "gemm_fp8_mxa",
          "layernorm_fp8", "add_layernorm", "window_attention", "seq_attention")
_OFF = {"S6D_LNFOLD": "0"}
_NO_RES = {"S6D_DISABLE_FUSED": "gemm_bf16_res"}
# name -> (model, environment, form); form: what the output is held to (see the module docstring)
CASES = {
    "sam-lnfold": ("sam", {}, "bf16"),
    "sam-lnfold-upto1": ("sam", {}, "bf16"),
    "sam-res": ("sam", dict(_OFF, S6D_GEMM_RES="1"), "bf16"),
    "sam-delta": ("sam", _OFF, "bf16"),
    "sam-fp8": ("sam", {"S6D_SAM_GEMM": "fp8"}, "fp8"),
    "sam-fp8mx": ("sam", {"S6D_SAM_GEMM": "fp8mx"}, "fp8"),
    "sam-fp8-delta": ("sam", dict(_NO_RES, S6D_SAM_GEMM="fp8"), "fp8"),
    "dino-lnfold": ("dino", {}, "bf16"),
    "dino-res": ("dino", _OFF, "bf16"),
    "dino-delta": ("dino", dict(_OFF, **_NO_RES), "bf16"),
    "dino-fp8": ("dino", {"S6D_DINO_GEMM": "fp8"}, "fp8"),
    "dino-fp8mx": ("dino", {"S6D_DINO_GEMM": "fp8mx"}, "fp8"),
    "pem-f16-delta": ("pem", {}, "f16"),
    "pem-bf16-res": ("pem", {"S6D_GEMM_RES": "1"}, "bf16x8"),
}


@contextlib.contextmanager
def configured(env):
    """The S6D_* variables of a case, read into the policy; the environment's own policy afterwards."""
    from sam6d_amd import policy
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    policy.reload()
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        policy.reload()


def _describe(v):
    if torch.is_tensor(v):
        return [list(v.shape), str(v.dtype).replace("torch.", "")]
    if isinstance(v, (tuple, list)):
        return [_describe(e) for e in v]
    assert v is None or isinstance(v, (bool, int, float, str)), type(v)
    return v


@contextlib.contextmanager
def traced():
    """Wraps the ops functions the block loops call -> the ordered list of {op, args by parameter name: [shape, dtype] of a tensor,
    the value of a scalar or flag, None where nothing is given (stats_partial, delta, ...)} and, where there is an `out`, whether it
    is the residual's memory."""
    from sam6d_amd import ops
    trace, real = [], {n: getattr(ops, n) for n in TRACED}

    def wrap(name, fn):
        sig = inspect.signature(fn)

        def wrapped(*a, **k):
            ba = sig.bind(*a, **k)
            ba.apply_defaults()
            e = {"op": name, "args": {n: _describe(v) for n, v in ba.arguments.items()}}
            if "out" in ba.arguments:
                out, res = ba.arguments["out"], ba.arguments.get("residual")
                e["out_is_residual"] = out is not None and res is not None and out.data_ptr() == res.data_ptr()
            trace.append(e)
            return fn(*a, **k)
        return wrapped
    for n, fn in real.items():
        setattr(ops, n, wrap(n, fn))
    try:
        yield trace
    finally:
        for n, fn in real.items():
            setattr(ops, n, fn)


def _perturb_norms(m):
    with torch.no_grad():
        for blk in m.blocks:                                          # non-trivial affine parameters: the fold has work to do
            for n in (blk.norm1, blk.norm2):
                n.weight.add_(0.2 * torch.randn(256, generator=torch.Generator().manual_seed(7)))
                n.bias.add_(0.1 * torch.randn(256, generator=torch.Generator().manual_seed(8)))


def _sam(name, dev):
    """The 2-block encoder of tests/test_emu_sam.py: a window-7 and a global block, 16 x 16 tokens, 4 heads, mlp_ratio 2."""
    from sam6d_amd.sam.image_encoder import ImageEncoderViT
    from sam6d_amd.utils import seeded
    m = ImageEncoderViT(depth=2, embed_dim=256, img_size=256, mlp_ratio=2, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
                        num_heads=4, patch_size=16, qkv_bias=True, use_rel_pos=True, global_attn_indexes=(1,), window_size=7,
                        out_chans=32).eval()
    m = seeded.load_seeded(m, 4)
    _perturb_norms(m)
    x = (0.5 * torch.randn(1, 16, 16, 256, generator=torch.Generator().manual_seed(1)) + 0.3).to(torch.bfloat16)
    upto = 1 if name.endswith("upto1") else None
    ref = x.float()
    for blk in list(m.blocks)[:upto]:
        ref = blk(ref)
    m, xd = m.bfloat16().to(dev), x.to(dev)
    keep = xd.clone()
    with traced() as trace:
        out = m._blocks_fused(xd, upto)
    assert torch.equal(xd, keep)                                      # own=False: the caller's tensor untouched in every form
    return trace, [out], [ref]


def _dino(name, dev):
    """The 2-block model of tests/test_emu_sam.py: B 2, 17 tokens, 4 heads of 64, LayerScale gains away from 1."""
    from sam6d_amd.ism.dinov2 import DinoVisionTransformer
    from sam6d_amd.utils import seeded
    m = DinoVisionTransformer(img_size=56, patch_size=14, embed_dim=256, depth=2, num_heads=4, mlp_ratio=4, init_values=1.0,
                              block_chunks=0).eval()
    m = seeded.load_seeded(m, 6)
    _perturb_norms(m)
    with torch.no_grad():
        for blk in m.blocks:
            blk.ls1.gamma.mul_(0.7)
            blk.ls2.gamma.mul_(1.3)
    x = (0.5 * torch.randn(2, 17, 256, generator=torch.Generator().manual_seed(1)) + 0.2).to(torch.bfloat16)
    ref = x.float()
    for blk in m.blocks:
        ref = blk(ref)
    refn = m.norm(ref)
    m = m.bfloat16().to(dev)
    with traced() as trace:
        out = m._blocks_fused(x.to(dev))
    return trace, list(out), [ref, refn]


def _pem(name, dev):
    """Depth 8: taps after blocks 1, 3, 5, 7, and blocks 0, 2, 4, 6 carry their delta across (at depth 4 every block is a tap)."""
    from sam6d_amd.pem.feature_extraction import ViT
    from sam6d_amd.utils import seeded
    dt = {"f16": torch.float16, "bf16": torch.bfloat16}[name.split("-")[1]]
    m = seeded.load_seeded(ViT(patch_size=16, embed_dim=256, depth=8, num_heads=4, mlp_ratio=2, img_size=64).eval(), 7)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    ref = m(x)
    m = m.to(dt).to(dev)
    with traced() as trace, torch.autocast(device_type=torch.device(dev).type, dtype=dt):
        out = m(x.to(dt).to(dev))
    return trace, out, ref


_RESULTS = {}


def run_case(name, dev="cuda"):
    """-> (trace, [relative rms of each output against float32], outputs on the host); each case runs once per device."""
    if (name, dev) not in _RESULTS:
        model, env, _ = CASES[name]
        with configured(env), torch.no_grad():
            trace, out, ref = {"sam": _sam, "dino": _dino, "pem": _pem}[model](name, dev)
        out = [o.float().cpu() for o in out]
        assert len(out) == len(ref)
        _RESULTS[name, dev] = trace, [((o - r).pow(2).mean() / r.pow(2).mean()).sqrt().item() for o, r in zip(out, ref)], out
    return _RESULTS[name, dev]


def case_body(name, dev="cuda"):
    trace, errs, out = run_case(name, dev)
    print(name, "rel rms vs float:", " ".join("%.3e" % e for e in errs))
    with open(GOLDEN) as f:
        want = json.load(f)["cases"][name]
    got = json.loads(json.dumps(trace))
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
    form = CASES[name][2]
    if form == "fp8":
        bf16 = run_case(name.split("-")[0] + "-lnfold", dev)[2]
        rel = [((o - r).pow(2).mean().sqrt() / r.pow(2).mean().sqrt()).item() for o, r in zip(out, bf16)]
        print(name, "rel rms vs the bf16 loop:", " ".join("%.3e" % e for e in rel))
        assert max(rel) <= E_BLOCK_FP8 * 3 ** 0.5, rel
    else:
        assert max(errs) <= {"bf16": 8e-3, "f16": 2e-3, "bf16x8": 2 ** 3 * 2e-3}[form], errs


def fold_body(model, dev="cuda"):
    e_fold, e_old = run_case(model + "-lnfold", dev)[1], run_case(model + "-delta", dev)[1]
    print(model, "rel rms vs float: folded", e_fold, "add + LayerNorm form", e_old)
    for f, o in zip(e_fold, e_old):
        assert f <= 1.1 * o + 5e-4, (e_fold, e_old)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_block_loop_launches_and_output(name):
    case_body(name)


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["sam", "dino"])
def test_folded_form_not_further_from_float_than_the_add_layernorm_form(model):
    fold_body(model)
