"""bench.py -- frames/s of the SAM-6D per-frame hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]   (N=1)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Workload (BASELINE.json configs[1]: "LM-O single object, 2048 pts, 42 templates, batch=32 bf16"):
one STEP = one batch of 32 synthetic 640x480 RGB-D frames per GPU, each holding one instance of the
single LM-O object.  Per frame the hot path of SURVEY.md section 8(a) runs in full:
  a1-a5   SAM ViT-H image encoder on the 1024x1024 preprocessed frame (bf16)
  a6-a9   proposal-vs-template scoring of P=128 proposals against 1 object x 42 templates
          (semantic + appearance + geometric score)
  a10-a24 PEM Net.forward for the detected instance (2048 observed points, 2048x256 template
          features, 1024 model points) -- the 32 frames form one PEM batch of 32.
Inputs are resident in HBM before the timed region; weights are seeded-random (no checkpoint is
reachable offline), results therefore meaningless but the arithmetic is the full model.
Frames shard across ranks with no data-path collective (weak scaling); the only RCCL traffic is the
final all_gather of the fixed-width pose records, inside the timed region.
A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the JSON line.  --full adds the side
measurements after the timed steps (rank 0, minutes): stage split, PEM extractor dtypes, per-kernel rooflines, host-input
rate, the fp8 configurations, the whole-frame and sharded blocks and the CPU baseline, as extra keys of the same line.
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC: what RCCL needs on this driver (multi-process runs)

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FRAMES_PER_STEP = 32
P_PROPOSALS = 128
SAM_FLOP_PER_FRAME = 5.96e12        # 28 x 176.9 + 4 x 248.3 + 15.6 GFLOP
MFMA_BF16_PEAK = 2.5e15             # dense, /opt/skills/guides/MI355X_MICROARCH.md


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="ranks = GPUs of this node.  Under torch.distributed.run it must equal WORLD_SIZE; started plainly with "
                         "--gpus N > 1 this process becomes the launcher: it re-executes itself as N ranks through "
                         "torch.distributed.run on 127.0.0.1 and rank 0 prints the one JSON line (default: WORLD_SIZE, else 1)")
    ap.add_argument("--steps", type=_count(1), default=3, help="timed steps (at least 1)")
    ap.add_argument("--warmup", type=_count(0), default=1, help="untimed steps before them")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32 / float64, at most "
                         "64 MB in all; a seeded sample of the larger arrays): the inputs are seeded, so two builds run with the same "
                         "arguments can be compared output for output")
    ap.add_argument("--frames", type=int, default=FRAMES_PER_STEP)
    ap.add_argument("--sam-chunk", type=int, default=int(os.environ.get("S6D_SAM_CHUNK", str(SAM_CHUNK))))
    ap.add_argument("--config", choices=("lmo", "fp8", "fp8mx"), default="lmo",
                    help="lmo = BASELINE configs[1] (the headline: bf16 ViTs); fp8 = the fp8 ViT-H MFMA path of configs[4] on the same "
                         "workload (qkv / lin1 GEMMs of the SAM encoder on the fp8 matrix cores) -- its own line, never the headline")
    ap.add_argument("--gemm-wave-tile", type=int, choices=(0, 64, 128), default=0,
                    help="form of the bf16 GEMM kernel (ops.set_gemm_wave_tile): 0 = the library's choice (default), 64 = eight-wave "
                         "form everywhere, 128 = four-wave form wherever it applies -- for same-box A/B runs")
    ap.add_argument("--strict", action="store_true",
                    help="sam6d_amd.policy strict mode: a library (rocBLAS / ATen) branch of a module on a CUDA tensor raises, naming the failed guard")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, the side measurements too (rank 0, minutes): stage split, PEM extractor dtypes, "
                         "per-kernel rooflines, host-input rate, fp8 configurations, whole-frame and sharded blocks, CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the `cpu_baseline` block")
    ap.add_argument("--cpu-baseline-only", action="store_true")
    ap.add_argument("--no-pipeline", action="store_true", help="with --full: skip the whole-frame `pipeline` block (all five models)")
    ap.add_argument("--no-fp8", action="store_true",
                    help="with --full: skip the `configs.fp8` block (BASELINE configs[4] measured next to the headline)")
    ap.add_argument("--no-extras", action="store_true",
                    help="the timed steps only, even with --full: what a run without --full does (the target of the rocprofv3 "
                         "kernel-statistics passes, so that their shares are the step's and not the side measurements')")
    ap.add_argument("--standin", action="store_true",
                    help="TEST INFRASTRUCTURE (tests/test_bench_launcher.py): stand-in stages on the CPU over gloo, to exercise the "
                         "launcher, the barriers, the record gather and the JSON line on a host without GPUs; the line it prints "
                         "says so and is not a measurement")
    return ap.parse_args()


def _count(least):
    def parse(s):
        n = int(s)
        if n < least:
            raise argparse.ArgumentTypeError(f"{n} < {least}")
        return n
    return parse


SAM_CHUNK = 16   # frames per SAM encoder launch group: 16 x 4096 tokens per GEMM (measured on one box: chunk 8 with the
                 # recorded hipBLASLt solutions 199.0 ms / 32 frames, chunk 16 on the default heuristics 193.0, chunk 32 193.6)


def benched_policy():
    """The configuration this file measures, made explicit: sam6d_amd.policy.PrecisionPolicy.benched() = the
    library defaults (bf16 SAM ViT-H / mask decoder / DINOv2) + the PEM's ViT-B extractor in IEEE half.  The process environment
    gets the same value so that the blocks below that re-read it (policy.reload() after switching S6D_SAM_GEMM for the fp8 rows)
    stay on it; an S6D_PEM_VIT_DTYPE the caller exported wins."""
    os.environ.setdefault("S6D_PEM_VIT_DTYPE", "fp16")
    __import__("sam6d_amd.policy").policy.reload()


class HotPath:
    """All device state of one rank: models, replicated template data, one batch of frames."""
    keep_outputs = False      # step() keeps what the stages returned in self.outputs (--dump-outputs)

    def __init__(self, device, frames, sam_chunk):
        from sam6d_amd.ism.scoring import FrameScorer
        from sam6d_amd.pem import pose_estimation_model as pm
        from sam6d_amd.sam.image_encoder import build_vit_h
        from sam6d_amd.utils import seeded, synth

        # PEM ViT-B in IEEE half (fp16) since round 3, through the fused pipeline (s6d_gemm_f16 / s6d_seq_attention_f16 /
        # s6d_add_layernorm_f16): the matrix rate of bf16 with an 11-bit significand.  With bf16 features the translation sits at
        # 1.3e-3 .. 2e-3 mm of the reference's on the well-conditioned golden, over north_star's 1e-3 mm bar (features 7.6e-3 off
        # the fp32 extractor's); half keeps the features within 1e-3 and the pose within the bar (tests/test_gpu_pem.py).  The fp32
        # extractor (library GEMMs) costs 6.4 ms more per 32 instances (profiles/r03_bench_pem_vit_dtype.txt).  The SAM ViT-H -- 87 %
        # of the step -- runs bf16 as configs[1] says.
        # (the extractor's dtype is the caller's policy: bench.py's main() selects fp16 -- benched_policy() below -- and HotPath
        # itself changes neither the environment nor the policy)
        self.dev, self.F, self.chunk = device, frames, sam_chunk
        self.sam = seeded.load_seeded(build_vit_h().eval(), 3).to(device=device, dtype=torch.bfloat16)
        self.pem = seeded.load_seeded(pm.Net(pm.default_cfg()).eval(), 1).to(device)
        ism = synth.ism_inputs(P=P_PROPOSALS, O=1, T=42, seed=11)
        self.ism_in = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in ism.items()}
        self.scorer = FrameScorer(self.ism_in["ref_cls"], self.ism_in["ref_patch"], self.ism_in["poses"],
                                  self.ism_in["pointcloud"])
        # 640x480 frames resized to long side 1024 (ResizeLongestSide, done by the caller) -> (3,768,1024) float RGB
        g = torch.Generator().manual_seed(5)
        self.sam_raw = (torch.rand(frames, 3, 768, 1024, generator=g) * 255).to(device)
        pin = synth.pem_inputs(frames, seed=1)
        self.pem_in = {k: pin[k].to(device) for k in ("pts", "rgb", "rgb_choose", "model", "dense_po", "dense_fo")}
        self.rand_u = synth.coarse_uniforms(frames, 2).to(device)

    @torch.no_grad()
    def sam_stage(self):
        from sam6d_amd.sam.image_encoder import preprocess
        nst = int(os.environ.get("S6D_SAM_STREAMS", "1"))   # measured: 1 = 2 > 4 streams (GEMMs already fill the GPU)
        outs = []                                           # the image embeddings of every launch group, in frame order
        if nst <= 1:
            for i in range(0, self.F, self.chunk):
                x = preprocess(self.sam_raw[i:i + self.chunk], 1024, out_dtype=torch.bfloat16)     # a1: Sam.preprocess
                outs.append(self.sam(x))                                                           # a2-a5
            return outs
        # chunks alternate between HIP streams: one chunk's latency-bound attention / LayerNorm phases run under
        # the other chunk's GEMMs
        if not hasattr(self, "_sam_streams"):
            self._sam_streams = [torch.cuda.Stream(device=self.dev) for _ in range(nst)]
        cur = torch.cuda.current_stream()
        for st in self._sam_streams:
            st.wait_stream(cur)
        for j, i in enumerate(range(0, self.F, self.chunk)):
            with torch.cuda.stream(self._sam_streams[j % nst]):
                x = preprocess(self.sam_raw[i:i + self.chunk], 1024, out_dtype=torch.bfloat16)
                outs.append(self.sam(x))
        for st in self._sam_streams:
            cur.wait_stream(st)
        return outs

    @torch.no_grad()
    def ism_stage(self):
        """Scoring of the step's frames in launch groups of S6D_ISM_CHUNK frames (default 8; FrameScorer.score_frames: the frames of a
        group go through one set of launches with a per-proposal frame index -- like the SAM encoder's groups of 16 frames and the
        PEM's batch of 32 instances; results identical to frame-by-frame scoring, tests/test_gpu_ism.py).  S6D_ISM_CHUNK=0: one
        ``score`` call per frame (round 1)."""
        i = self.ism_in
        c = int(os.environ.get("S6D_ISM_CHUNK", "8"))
        outs = []                                           # the scores of every launch group (every frame for c <= 0)
        if c <= 0:
            for _ in range(self.F):
                outs.append(self.scorer.score(i["qry_cls"], i["qry_patch"], i["masks"], i["boxes"], i["depth"], i["K"]))
            return outs
        if getattr(self, "_ism_group", None) is None or self._ism_group[0] != c:
            # every frame of a group has its own tensors in HBM and its own content (eight copies of one frame made the
            # number of selected proposals S the same for every frame): frame f is the synthetic frame with its proposals
            # permuted, its descriptors perturbed (noise growing with f, so more or fewer proposals pass the semantic threshold)
            # and its depth shifted
            gg = torch.Generator().manual_seed(77)
            fr = {k: [] for k in ("qry_cls", "qry_patch", "masks", "boxes", "depth")}
            for f in range(self.F):            # one synthetic frame per frame of the step (not the same 8 four times)
                perm = torch.randperm(i["qry_cls"].shape[0], generator=gg).to(self.dev)
                amp = 0.15 * (f % 8) + 0.02 * (f // 8)
                fr["qry_cls"].append(i["qry_cls"][perm] + amp * torch.randn(i["qry_cls"].shape, generator=gg).to(self.dev))
                fr["qry_patch"].append(i["qry_patch"][perm])
                fr["masks"].append(i["masks"][perm])
                fr["boxes"].append(i["boxes"][perm])
                fr["depth"].append(i["depth"] + 7.0 * (f % 8) + 1.0 * (f // 8))
            self._ism_group = (c, {k: torch.stack(v).contiguous() for k, v in fr.items()},
                               i["K"].to(self.dev)[None].expand(self.F, 3, 3).contiguous())
        _, g, K = self._ism_group
        for f0 in range(0, self.F, c):
            n = min(c, self.F - f0)
            e = f0 + n
            outs.append(self.scorer.score_frames(g["qry_cls"][f0:e], g["qry_patch"][f0:e], g["masks"][f0:e], g["boxes"][f0:e],
                                                 g["depth"][f0:e], K[f0:e]))
        return outs

    @torch.no_grad()
    def pem_stage(self):
        ep = dict(self.pem_in)
        ep["coarse_rand_u"] = self.rand_u
        return self.pem(ep)

    def step(self):
        """One batch of frames through all three stages.  The stages of a batch are launched on three HIP streams:
        in a running pipeline batch k's SAM encode overlaps batch k-1's scoring and pose estimation (the stages only
        depend on each other through the previous batch's outputs), and the small launch-bound ISM / PEM kernels
        fill the gaps between the SAM GEMMs.  Every stage still runs in full for every batch; the step ends when
        all three streams have drained (S6D_BENCH_SERIAL=1 runs them back to back on one stream).  With ``keep_outputs`` what the
        stages return stays in ``self.outputs`` until the next step (--dump-outputs writes it)."""
        if os.environ.get("S6D_BENCH_SERIAL"):
            sam = self.sam_stage()
            ism = self.ism_stage()
            out = self.pem_stage()
        else:
            if not hasattr(self, "_streams"):
                self._streams = [torch.cuda.Stream(device=self.dev) for _ in range(2)]
            cur = torch.cuda.current_stream()
            for st in self._streams:
                st.wait_stream(cur)
            with torch.cuda.stream(self._streams[0]):
                sam = self.sam_stage()
            # the scoring loop is the only stage with host round trips (one torch.nonzero per frame, as in the
            # reference): it is enqueued LAST, so the host waits on it while the other two streams are already full
            # (measured: no difference either way -- the step is bound by the sum of kernel time, not by the host)
            out = self.pem_stage()                      # current stream
            with torch.cuda.stream(self._streams[1]):
                ism = self.ism_stage()
            for st in self._streams:
                cur.wait_stream(st)
        if self.keep_outputs:
            self.outputs = {"sam": sam, "ism": ism, "pem": {k: v for k, v in out.items() if k not in self.pem_in and k != "coarse_rand_u"}}
        # fixed-width pose record per instance (68 B)
        from sam6d_amd.utils import shard
        return shard.pack_records(0, torch.arange(self.F, device=self.dev), 5, out["pred_pose_score"],
                                  out["pred_R"], out["pred_t"], 0.0)


def stage_ms(fn, n=2):
    """HIP-event time of one stage on torch's current stream (the stream every s6d kernel uses)."""
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


_GEMM_WAVE_TILE = 0        # what --gemm-wave-tile set (0 = the library's choice: the four-wave form wherever it applies)


def _gemm_inst(epi, M):
    """Template instance (as rocprofv3 prints it) that serves a ViT-H Linear with epilogue `epi` at M rows: the four-wave form
    (csrc/s6d_gemm4.hip) covers epilogues 0 - 4 at M % 256 == 0 and runs when --gemm-wave-tile 128 selects it; the library's own
    choice is the eight-wave form (csrc/s6d_gemm.hip): 0.3 % ahead inside the step once both forms had the round-6 epilogue."""
    four = _GEMM_WAVE_TILE == 128 and epi in (0, 1, 2, 3, 4) and M % 256 == 0
    return f"gemm4_bf16_kernel<{epi}, true>" if four else f"gemm_bf16_kernel<{epi}, true>"


def _event_ms(fn, n):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def gemm_ms_inside_the_step(hp):
    """Average duration of every s6d_gemm_bf16 / _res / _lnfold launch of ONE SAM stage pass, by form and shape, from HIP events recorded around the launches
    on the stream they run on -- the kernel in the context the step runs it in (between the attention / LayerNorm launches of its
    block, at the clocks of that mix), which is what the rocprofv3 kernel trace of the same command averages
    (profiles/r02_bench_serial_kernel_stats.csv).  Back-to-back launches of one shape on random operands (kernel_rooflines below)
    hold the socket at its power limit and come out 10-15 % slower."""
    from sam6d_amd import ops
    real = ops.gemm_bf16
    rec = []

    def timed(a, w, bias=None, gelu=False, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = real(a, w, bias, gelu=gelu, **kw)
        e1.record()
        form = "res" if kw.get("residual") is not None else "plain"
        rec.append(((form, a.numel() // a.shape[-1], a.shape[-1], w.shape[0], bool(gelu)), e0, e1))
        return y
    real_f = ops.gemm_bf16_lnfold

    def timed_f(a, st, w, cs, bias, gelu=False, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = real_f(a, st, w, cs, bias, gelu=gelu, **kw)
        e1.record()
        rec.append((("lnfold", a.numel() // a.shape[-1], a.shape[-1], w.shape[0], bool(gelu)), e0, e1))
        return y
    real8 = ops.gemm_fp8

    def timed8(a8, sa, w8, sw, bias=None, gelu=False, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = real8(a8, sa, w8, sw, bias, gelu=gelu, **kw)
        e1.record()
        rec.append((("fp8", a8.numel() // a8.shape[-1], a8.shape[-1], w8.shape[0], bool(gelu)), e0, e1))
        return y
    real_gm, real_mx = ops.gemm_fp8_gelu_mx, ops.gemm_fp8_mxa

    def timed_gm(a8, sa, w8, sw, bias=None, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = real_gm(a8, sa, w8, sw, bias, **kw)
        e1.record()
        rec.append((("fp8_gelu_mx", a8.numel() // a8.shape[-1], a8.shape[-1], w8.shape[0], True), e0, e1))
        return y

    def timed_mx(a8, amx, w8, sw, bias=None, gelu=False, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = real_mx(a8, amx, w8, sw, bias, gelu=gelu, **kw)
        e1.record()
        rec.append((("fp8_mxa", a8.numel() // a8.shape[-1], a8.shape[-1], w8.shape[0], bool(gelu)), e0, e1))
        return y
    hp.sam_stage()                                          # warm
    ops.gemm_bf16, ops.gemm_fp8, ops.gemm_bf16_lnfold, ops.gemm_fp8_gelu_mx, ops.gemm_fp8_mxa = timed, timed8, timed_f, timed_gm, timed_mx
    try:
        hp.sam_stage()
    finally:
        ops.gemm_bf16, ops.gemm_fp8, ops.gemm_bf16_lnfold, ops.gemm_fp8_gelu_mx, ops.gemm_fp8_mxa = real, real8, real_f, real_gm, real_mx
    torch.cuda.synchronize()
    by = {}
    for key, e0, e1 in rec:
        by.setdefault(key, []).append(e0.elapsed_time(e1))
    return {k: (sum(v) / len(v), len(v)) for k, v in by.items()}


def kernel_rooflines(dev, sam_chunk, frames, in_step=None):
    """Per-launch roofline of the hand-written kernels at the exact shapes the step uses, timed with HIP events on
    torch's current stream (the stream every s6d_* kernel is launched on).  Algorithmic work per launch:
      attn_global   4*T^2*hd*nh*Bc FLOP (QK^T + PV), T = 4096, hd = 80, nh = 16, Bc = frames per SAM chunk
      attn_window16 4*196^2*hd * 25 windows * nh * Bc FLOP; HBM-bound: Bc*4096 tokens * (3+1)*1280 * 2 bytes
      rpe_attention B*N * (N*256*4) bytes  (the geometric embedding is streamed exactly once), N = 197
      geo_embed     B*N*N * 4 embeddings * 2*256*256 FLOP (as written in the reference, fp32)
    Peaks: 2.5 PFLOP/s dense bf16 MFMA, 157.3 TFLOP/s fp32, 8.0 TB/s HBM (MI355X_MICROARCH.md)."""
    from sam6d_amd import ops
    g = torch.Generator(device="cpu").manual_seed(0)
    out = []
    nh, hd, H = 16, 80, 64
    qkv = torch.randn(sam_chunk, H, H, 3 * nh * hd, generator=g).to(dev).to(torch.bfloat16)
    bias = torch.randn(3 * nh * hd, generator=g).to(dev).to(torch.bfloat16)
    for name, ws, S in (("attn_global64_kernel<80,8,3>", 0, 64), ("attn_window16p_kernel<80, true>", 14, 14)):
        rh = torch.randn(2 * S - 1, hd, generator=g).to(dev).to(torch.bfloat16)
        rw = torch.randn(2 * S - 1, hd, generator=g).to(dev).to(torch.bfloat16)
        ms = _event_ms(lambda: ops.window_attention(qkv, bias, rh, rw, nh, ws, hd ** -0.5), 10)
        nwin = 1 if ws == 0 else 25
        flop = 4.0 * (S * S) ** 2 * hd * nwin * nh * sam_chunk
        if ws == 0:
            out.append({"kernel": name, "bound": "mfma", "achieved": round(flop / ms / 1e9, 1), "peak": 2500.0,
                        "unit": "TFLOP/s", "frac": round(flop / ms / 1e9 / 2500.0, 4), "avg_ms": round(ms, 4),
                        "launches_per_step": 4 * (frames // sam_chunk)})
        else:
            # 14x14 windows: 39 GFLOP against q,k,v read once + out written once = 117 FLOP/B, below the
            # 2500/8 = 312 FLOP/B ridge -> the HBM roofline (42 us) binds, not the MFMA one (16 us)
            nbytes = float(sam_chunk) * H * H * 4 * nh * hd * 2
            out.append({"kernel": name, "bound": "hbm", "achieved": round(nbytes / ms / 1e6, 1), "peak": 8000.0,
                        "unit": "GB/s", "frac": round(nbytes / ms / 1e6 / 8000.0, 4), "avg_ms": round(ms, 4),
                        "launches_per_step": 28 * (frames // sam_chunk),
                        "mfma_tflops": round(flop / ms / 1e9, 1)})
    B, N = frames, 197
    q, k, v = (torch.randn(B, N, 256, generator=g).to(dev) for _ in range(3))
    qt = torch.randn(B, 4, N, 256, generator=g).to(dev)
    qb = torch.randn(B, 4, N, generator=g).to(dev)
    emb = torch.randn(B, N, N, 256, generator=g).to(dev)
    ms = _event_ms(lambda: ops.rpe_attention(q, k, v, qt, qb, emb, 0.125), 10)
    nbytes = float(B) * N * N * 256 * 4
    out.append({"kernel": "rpe_attention_kernel<4>", "bound": "hbm", "achieved": round(nbytes / ms / 1e6, 1),
                "peak": 8000.0, "unit": "GB/s", "frac": round(nbytes / ms / 1e6 / 8000.0, 4), "avg_ms": round(ms, 4),
                "launches_per_step": 12})
    idx4 = torch.rand(B, N, N, 4, generator=g).to(dev) * 10
    Wd, Wa = torch.randn(256, 256, generator=g).to(dev) / 16, torch.randn(256, 256, generator=g).to(dev) / 16
    bd, ba = torch.randn(256, generator=g).to(dev), torch.randn(256, generator=g).to(dev)
    div = torch.exp(torch.arange(0, 256, 2).float() * (-9.210340371976184 / 256)).to(dev)
    ms = _event_ms(lambda: ops.geo_embedding(idx4, Wd, bd, Wa, ba, div), 5)
    flop = float(B) * N * N * 4 * 2 * 256 * 256
    # executed matrix work = 3 bf16 MFMA terms per algorithmic fp32 product (hi*hi + lo*hi + hi*lo)
    out.append({"kernel": "geo_embed_kernel", "bound": "mfma", "achieved": round(3 * flop / ms / 1e9, 1), "peak": 2500.0,
                "unit": "TFLOP/s (bf16 MFMA executed = 3x the algorithmic fp32 FLOP)",
                "frac": round(3 * flop / ms / 1e9 / 2500.0, 4), "avg_ms": round(ms, 4), "launches_per_step": 2,
                "algorithmic_fp32_tflops": round(flop / ms / 1e9, 1)})
    # fine matching head: similarity + assignment fused (csrc/s6d_fine.hip); executed matrix work = 3 sweeps x 3 bf16 terms per
    # algorithmic fp32 product over the (2080 x 2048 x 256) padded tile space; algorithmic HBM bytes = the two feature sets + outputs
    if ops.have("fine_match"):
        f1 = torch.randn(B, 2049, 256, generator=g).to(dev)
        f2 = torch.randn(B, 2049, 256, generator=g).to(dev)
        p2 = torch.randn(B, 2048, 3, generator=g).to(dev)
        ms = _event_ms(lambda: ops.fine_match(f1, f2, p2, 0.1), 10)
        flop = 9 * 2.0 * B * 2080 * 2048 * 256
        out.append({"kernel": "fine_match (split + 3 x fine_sweep_kernel)", "bound": "mfma", "achieved": round(flop / ms / 1e9, 1),
                    "peak": 2500.0, "unit": "TFLOP/s (bf16 MFMA executed = 9x the algorithmic fp32 similarity FLOP)",
                    "frac": round(flop / ms / 1e9 / 2500.0, 4), "avg_ms": round(ms, 4), "launches_per_step": 1,
                    "algorithmic_bytes": float(B) * (2 * 2049 * 256 * 4 + 2048 * 5 * 4),
                    "matrix_bytes_not_written": float(B) * 2049 * 2049 * 4, "pmc_key": "fine_sweep_kernel<2>"})
    if ops.have("linear_f32"):
        # the fused fp32 Linear of the point transformer at the dense stage's shape (65536 rows, 256 -> 256, + residual + LayerNorm)
        Mp = 2048 * B
        xp = torch.randn(Mp, 256, generator=g).to(dev)
        hi, lo = ops.split_weight((torch.randn(256, 256, generator=g) / 16).to(dev))
        bp, rp = torch.randn(256, generator=g).to(dev), torch.randn(Mp, 256, generator=g).to(dev)
        gm, bt = torch.ones(256, device=dev), torch.zeros(256, device=dev)
        ms = _event_ms(lambda: ops.linear_f32(xp, hi, lo, bp, residual=rp, ln=(gm, bt, 1e-5)), 10)
        flop = 3.0 * 2.0 * Mp * 256 * 256
        nbytes = float(Mp) * 256 * 4 * 3                            # x and the residual read once, y written once
        # HBM-bound: 201 MB in ~63 us = 3.2 TB/s = 0.40 of the HBM peak, against 0.16 of the matrix peak for the
        # executed bf16 products -- the row is priced against the roof that binds it
        out.append({"kernel": "plin_kernel (linear + residual + LayerNorm, M=%d K=256 N=256)" % Mp, "bound": "hbm",
                    "achieved": round(nbytes / ms / 1e6, 1), "peak": 8000.0, "unit": "GB/s", "frac": round(nbytes / ms / 1e6 / 8000.0, 4),
                    "avg_ms": round(ms, 4), "launches_per_step": 36, "algorithmic_bytes": nbytes,
                    "mfma_tflops_executed": round(flop / ms / 1e9, 1), "pmc_key": "plin_kernel"})
    if ops.have("attn_output_chain") and ops.have("linear_f32"):
        # round 6: the post-attention chain of a point-transformer layer in one launch (csrc/s6d_pchain.hip) at the dense stage's
        # shape.  Algorithmic bytes: the attention output and the residual read once, y written once (h and the 512-wide
        # activations stay on chip); executed FLOP = 3 terms x 2 x M x (256*256 + 2*256*512).
        Mp = 2048 * B
        ap, xp2 = torch.randn(Mp, 256, generator=g).to(dev), torch.randn(Mp, 256, generator=g).to(dev)

        def _w(n, k):
            hi_, lo_ = ops.split_weight((torch.randn(n, k, generator=g) / 16).to(dev))
            return ops.fragment_weight(hi_), ops.fragment_weight(lo_), torch.randn(n, generator=g).to(dev)
        w1c, wec, wsc = _w(256, 256), _w(512, 256), _w(256, 512)
        ln_ = (torch.ones(256, device=dev), torch.zeros(256, device=dev), 1e-5)
        ms = _event_ms(lambda: ops.attn_output_chain(ap, xp2, w1c, ln_, wec, wsc, ln_), 10)
        flop = 3.0 * 2.0 * Mp * (256 * 256 + 2 * 256 * 512)
        nbytes = float(Mp) * 256 * 4 * 3
        out.append({"kernel": "pchain_kernel (linear + residual + LN + FFN 256-512-256 + residual + LN, M=%d)" % Mp, "bound": "mfma",
                    "achieved": round(flop / ms / 1e9, 1), "peak": 2500.0, "unit": "TFLOP/s (bf16 MFMA executed = 3x the algorithmic fp32 FLOP)",
                    "frac": round(flop / ms / 1e9 / 2500.0, 4), "avg_ms": round(ms, 4), "launches_per_step": 12,
                    "algorithmic_bytes": nbytes, "hbm_gbps": round(nbytes / ms / 1e6, 1), "pmc_key": "pchain_kernel"})
    # the Linear layers of the ViT-H blocks: the hand-written bf16 GEMM (csrc/s6d_gemm.hip) at the four shapes of a block, and the
    # library GEMM (hipBLASLt through torch) at the largest of them for context.  Algorithmic work 2 M N K FLOP.
    M = sam_chunk * 4096
    groups = frames // sam_chunk
    # Which form of each Linear the block loop runs (sam6d_amd/sam/image_encoder.py): with the folded loop (default) qkv and
    # lin1 + GELU are the LayerNorm-folded instantiations gemm_bf16_kernel<3 / 4, true> and proj / lin2 the residual one <2, true>;
    # S6D_LNFOLD=0: the plain instantiations <0 / 1, true> with add_layernorm passes between them.  FLOP are the algorithmic
    # 2 M N K of the Linear either way (the folded forms do the LayerNorm / the add on top, in the same launch).
    from sam6d_amd.utils.linear import lnfold_eligible, lnfold_weights
    xe = torch.empty(1, 1280, dtype=torch.bfloat16, device=dev)
    res_only = bool(in_step) and any(k[0] == "res" for k in in_step)     # fp8 loop: residual GEMMs without the fold
    if in_step:
        folded = any(k[0] == "lnfold" for k in in_step)
    else:
        folded = lnfold_eligible(xe, 1280, 1280) and not os.environ.get("S6D_SAM_GEMM", "").startswith("fp8")   # (the fp8 loop does not fold)
    for nm, K, N, gelu in (("qkv", 1280, 3840, False), ("proj", 1280, 1280, False), ("lin1+gelu", 1280, 5120, True),
                           ("lin2", 5120, 1280, False)):
        x = torch.randn(M, K, generator=g).to(dev).to(torch.bfloat16)
        W = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
        w = W.to(torch.bfloat16)
        b = torch.randn(N, generator=g).to(dev)
        if not ops.have("gemm_bf16"):
            break
        form = "plain"
        if folded and nm in ("qkv", "lin1+gelu"):
            form = "lnfold"
            wf, cs, bf = lnfold_weights(W, b, torch.ones(K, device=dev), torch.zeros(K, device=dev))
            st = ops.row_stats(x)
            b2b = _event_ms(lambda: ops.gemm_bf16_lnfold(x, st, wf, cs, bf, gelu=gelu), 10)
            inst = _gemm_inst(4 if gelu else 3, M)
        elif folded or (res_only and nm in ("proj", "lin2")):
            form = "res"
            xr = torch.randn(M, N, generator=g).to(dev).to(torch.bfloat16)
            sp = torch.empty(N // 32, 2, M, device=dev) if folded else None
            b2b = _event_ms(lambda: ops.gemm_bf16(x, w, b, residual=xr, out=xr, stats_partial=sp), 10)
            inst = _gemm_inst(2, M)
        else:
            b2b = _event_ms(lambda: ops.gemm_bf16(x, w, b, gelu=gelu), 10)
            inst = _gemm_inst(1 if gelu else 0, M)
        # avg_ms: inside the step (gemm_ms_inside_the_step) when the caller measured it; back_to_back_ms: 10 launches of this shape alone
        ms = in_step[(form, M, K, N, gelu)][0] if in_step and (form, M, K, N, gelu) in in_step else b2b
        flop = 2.0 * M * N * K
        what = {"plain": "", "lnfold": "LayerNorm-folded ", "res": "+ residual + row statistics, " if folded else "+ residual, "}[form]
        out.append({"kernel": f"{inst} ({what}{nm}, M={M} K={K} N={N})", "bound": "mfma", "achieved": round(flop / ms / 1e9, 1),
                    "peak": 2500.0, "unit": "TFLOP/s", "frac": round(flop / ms / 1e9 / 2500.0, 4), "avg_ms": round(ms, 4),
                    "back_to_back_ms": round(b2b, 4), "timed": "inside one SAM stage pass" if ms is not b2b else "back to back",
                    "launches_per_step": 32 * groups,
                    "algorithmic_bytes": 2.0 * (M * K + N * K + M * N) + (2.0 * M * N if form == "res" else 0.0),
                    # the GELU and the LayerNorm-folded instantiations run at one shape each; <0 / 2, true> are shared between shapes
                    # (no per-shape counters)
                    # (the residual instantiation <2, true> runs proj and lin2: the counter summary splits its launches by dispatch order,
                    # tools/pmc_summarise.py)
                    "pmc_key": inst if (gelu or form == "lnfold") else (f"{inst} [{nm}]" if form == "res" else "-"), "form": form,
                    "shape": nm})
    if os.environ.get("S6D_SAM_GEMM", "").startswith("fp8") and ops.have("gemm_fp8"):
        # configs[4]: the two LayerNorm-fed GEMMs on the fp8 matrix cores (dense peak 5 PFLOP/s), and the quantising LayerNorm
        from sam6d_amd.utils import fp8
        for nm, K, N, gelu in (("qkv", 1280, 3840, False), ("lin1+gelu", 1280, 5120, True)):
            qa, sa = fp8.quantize_rows(torch.randn(M, K, generator=g).to(dev))
            qw, sw = fp8.quantize_rows((torch.randn(N, K, generator=g) / K ** 0.5).to(dev))
            b = torch.randn(N, generator=g).to(dev)
            b2b = _event_ms(lambda: ops.gemm_fp8(qa, sa, qw, sw, b, gelu=gelu), 10)
            key = ("fp8", M, K, N, gelu)
            ms = in_step[key][0] if in_step and key in in_step else b2b
            flop = 2.0 * M * N * K
            out.append({"kernel": f"gemm_fp8_kernel ({nm}, M={M} K={K} N={N})", "bound": "mfma", "achieved": round(flop / ms / 1e9, 1),
                        "peak": 5000.0, "unit": "TFLOP/s (fp8 e4m3, v_mfma_scale_f32_32x32x64_f8f6f4)",
                        "frac": round(flop / ms / 1e9 / 5000.0, 4), "avg_ms": round(ms, 4), "back_to_back_ms": round(b2b, 4),
                        "timed": "inside one SAM stage pass" if ms is not b2b else "back to back", "launches_per_step": 32 * groups,
                        "algorithmic_bytes": 1.0 * (M * K + N * K) + 2.0 * M * N, "pmc_key": "gemm_fp8_kernel<1, true>" if gelu else "-"})
        if os.environ.get("S6D_SAM_GEMM") == "fp8mx" and ops.have("gemm_fp8_mx"):
            # lin1 with the MX output, lin2 with MX activations (round 4)
            qa, sa = fp8.quantize_rows(torch.randn(M, 1280, generator=g).to(dev))
            qw, sw = fp8.quantize_rows((torch.randn(5120, 1280, generator=g) / 1280 ** 0.5).to(dev))
            b1 = torch.randn(5120, generator=g).to(dev)
            b2b = _event_ms(lambda: ops.gemm_fp8_gelu_mx(qa, sa, qw, sw, b1), 10)
            key = ("fp8_gelu_mx", M, 1280, 5120, True)
            ms = in_step[key][0] if in_step and key in in_step else b2b
            flop = 2.0 * M * 5120 * 1280
            out.append({"kernel": f"gemm_fp8_kernel<5, true> (lin1 + GELU -> e4m3 with MX block scales, M={M} K=1280 N=5120)", "bound": "mfma",
                        "achieved": round(flop / ms / 1e9, 1), "peak": 5000.0, "unit": "TFLOP/s (fp8 e4m3)", "frac": round(flop / ms / 1e9 / 5000.0, 4),
                        "avg_ms": round(ms, 4), "back_to_back_ms": round(b2b, 4), "launches_per_step": 32 * groups,
                        "algorithmic_bytes": 1.0 * (M * 1280 + 5120 * 1280) + 1.0 * M * 5120 + M * 160.0, "pmc_key": "gemm_fp8_kernel<5, true>"})
            q8, qs = ops.gemm_fp8_gelu_mx(qa, sa, qw, sw, b1)
            qw2, sw2 = fp8.quantize_rows((torch.randn(1280, 5120, generator=g) / 5120 ** 0.5).to(dev))
            bb2 = torch.randn(1280, generator=g).to(dev)
            b2b = _event_ms(lambda: ops.gemm_fp8_mxa(q8, qs, qw2, sw2, bb2), 10)
            key = ("fp8_mxa", M, 5120, 1280, False)
            ms = in_step[key][0] if in_step and key in in_step else b2b
            out.append({"kernel": f"gemm_fp8mx_kernel<0, true> (lin2, MX activations, M={M} K=5120 N=1280)", "bound": "mfma",
                        "achieved": round(flop / ms / 1e9, 1), "peak": 5000.0, "unit": "TFLOP/s (fp8 e4m3)", "frac": round(flop / ms / 1e9 / 5000.0, 4),
                        "avg_ms": round(ms, 4), "back_to_back_ms": round(b2b, 4), "launches_per_step": 32 * groups,
                        "algorithmic_bytes": 1.0 * (M * 5120 + 1280 * 5120) + M * 160.0 + 2.0 * M * 1280, "pmc_key": "gemm_fp8mx_kernel<0, true>"})
            for r in out:                                                   # lin1's bf16-output fp8 form and the bf16 lin2 are off the path here
                if r["kernel"].startswith("gemm_fp8_kernel (lin1+gelu") or (r["kernel"].startswith(("gemm_bf16_kernel", "gemm4_bf16_kernel")) and r.get("shape") == "lin2"):
                    r["launches_per_step"] = 0
        xb = torch.randn(M, 1280, generator=g).to(dev).to(torch.bfloat16)
        gm, bt = torch.ones(1280, device=dev), torch.zeros(1280, device=dev)
        ms = _event_ms(lambda: ops.layernorm_fp8(xb, gm, bt, 1e-6), 10)
        out.append({"kernel": "layernorm_fp8_kernel", "bound": "hbm", "achieved": round(M * 1280 * 3 / ms / 1e6, 1), "peak": 8000.0,
                    "unit": "GB/s", "frac": round(M * 1280 * 3 / ms / 1e6 / 8000.0, 4), "avg_ms": round(ms, 4),
                    "launches_per_step": 64 * groups, "algorithmic_bytes": float(M) * 1280 * 3})
        # in this configuration qkv / lin1 do not run the bf16 kernel: their bf16 rows stay for comparison, off the path
        for r in out:
            if r["kernel"].startswith(("gemm_bf16_kernel", "gemm4_bf16_kernel")) and r.get("shape") in ("qkv", "lin1+gelu"):
                r["launches_per_step"] = 0
    x = torch.randn(M, 1280, generator=g).to(dev).to(torch.bfloat16)
    w = torch.randn(5120, 1280, generator=g).to(dev).to(torch.bfloat16)
    bb = torch.randn(5120, generator=g).to(dev).to(torch.bfloat16)
    ms = _event_ms(lambda: torch.nn.functional.linear(x, w, bb), 10)
    ms_g = _event_ms(lambda: torch.nn.functional.gelu(torch.nn.functional.linear(x, w, bb)), 10)
    flop = 2.0 * M * 1280 * 5120
    out.append({"kernel": "library GEMM (hipBLASLt) mlp.lin1 M=%d" % M, "bound": "mfma",
                "achieved": round(flop / ms / 1e9, 1), "peak": 2500.0, "unit": "TFLOP/s",
                "frac": round(flop / ms / 1e9 / 2500.0, 4), "avg_ms": round(ms, 4), "with_gelu_pass_ms": round(ms_g, 4),
                "launches_per_step": 0})
    return out


def _pmc_traffic(row):
    """HBM bytes per launch of a `kernels` row from the committed rocprofv3 --pmc passes (profiles/r03_pmc_summary.json, else the
    files of the earlier rounds), if present: FETCH_SIZE (doubled: gfx950 half-count of wide coalesced reads, MI355X_MICROARCH.md) + WRITE_SIZE.
    Rows name their counter key (`pmc_key` = the kernel's template instance as rocprofv3 prints it); a template instance that runs
    at several shapes in the counter pass (its average would mix them) has none."""
    key = row.get("pmc_key", row["kernel"])
    for f in ("r06_pmc_summary.json", "r05_pmc_summary.json", "r04_pmc_summary.json", "r03_pmc_summary.json", "r02_pmc_summary.json", "r01_pmc_summary.json"):
        try:
            d = json.load(open(os.path.join(ROOT, "profiles", f)))
        except Exception:  # noqa: BLE001
            continue
        for k, v in d.items():
            if k.replace(" ", "") == key.replace(" ", ""):
                return v.get("hbm_bytes_per_launch")
    return None


def cpu_baseline():
    """The CPU path timed on the host cores on a bounded sample of the same workload: 1 SAM ViT-H frame + 1 ISM frame (P = 128) + a
    PEM batch of 8 instances; per SURVEY 8(d) each leg is 1 warm-up run + the MEDIAN of 3 timed runs, and the core count used is
    stated next to ``nproc``.  Where the reference tree exists (the build container: S6D_REFERENCE_ROOT or /root/reference) the
    REFERENCE's own modules are timed through oracle/ref_timing.py (kind "reference", one process per leg); on the GPU box there is
    no reference tree and the oracle's restatement of the same algorithm is timed (kind "port")."""
    import statistics

    nproc = os.cpu_count()
    cores = min(nproc, 32)          # torch CPU kernels stop scaling (and regress) beyond ~32 threads
    torch.set_num_threads(cores)
    from oracle import refharness as rh
    if rh.available():
        import subprocess
        legs = {}
        for leg in ("sam", "ism", "pem"):
            out = subprocess.run([sys.executable, "-m", "oracle.ref_timing", leg, str(cores)], cwd=ROOT, capture_output=True, text=True, check=True)
            legs[leg] = json.loads(out.stdout.strip().splitlines()[-1])
        t_sam, t_ism, t_pem = legs["sam"]["seconds"], legs["ism"]["seconds"], legs["pem"]["seconds"] / legs["pem"]["unit_count"]
        per_frame = t_sam + t_ism + t_pem
        return {"value": 1.0 / per_frame, "unit": "frames/s", "cores": cores, "nproc": nproc, "kind": "reference",
                "sample": f"the reference's own modules (oracle/ref_timing.py), 1 warm-up + median of 3 per leg: ImageEncoderViT ViT-H on 1 frame "
                          f"({t_sam:.2f}s) + ISM scoring methods on 1 frame P=128 ({t_ism:.3f}s) + Net on a batch of {legs['pem']['unit_count']} "
                          f"({t_pem:.2f}s/instance), fp32 torch CPU, seeded weights"}

    from oracle import ism as oism
    from oracle import pem as opem
    from oracle import sam as osam
    from sam6d_amd.pem import pose_estimation_model as pm
    from sam6d_amd.sam.image_encoder import build_vit_h
    from sam6d_amd.utils import seeded, synth

    def med3(fn):
        fn()                        # warm-up (thread pool, allocator, first-touch of the weights)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), ts

    NB = 8
    with torch.no_grad():
        Wp = {k: v for k, v in seeded.load_seeded(pm.Net(pm.default_cfg()), 1).state_dict().items()}
        inp = synth.pem_inputs(NB, seed=1)
        ep = {k: inp[k] for k in ("pts", "rgb", "rgb_choose", "model", "dense_po", "dense_fo")}
        ru = synth.coarse_uniforms(NB, 2)
        t_pem, pem_runs = med3(lambda: opem.net_forward(Wp, ep, ru))
        t_pem /= NB
        ii = synth.ism_inputs(P=P_PROPOSALS, O=1, T=42, seed=11)
        t_ism, _ = med3(lambda: oism.score_frame(ii))
        with torch.device("cpu"):
            Ws = {k: v for k, v in seeded.load_seeded(build_vit_h(), 3).state_dict().items()}
        x = synth.sam_input(1, 5, 1024)
        t_sam, sam_runs = med3(lambda: osam.encoder_forward(Ws, x, osam.VIT_H))
    # SURVEY 8d says "all host cores (count stated)": the dominant leg (the ViT-H frame, > 85 % of the per-frame time) is timed once
    # more on ALL hardware threads, so that the choice of 32 is a measurement in the line, not a claim
    all_cores = None
    if nproc > cores:
        torch.set_num_threads(nproc)
        with torch.no_grad():
            osam.encoder_forward(Ws, x, osam.VIT_H)
            t0 = time.perf_counter()
            osam.encoder_forward(Ws, x, osam.VIT_H)
            t_all = time.perf_counter() - t0
        torch.set_num_threads(cores)
        all_cores = {"threads": nproc, "sam_frame_s": round(t_all, 2), "sam_frame_s_at_cores": round(t_sam, 2),
                     "faster": "all" if t_all < t_sam else f"{cores} threads"}
        if t_all < t_sam:                                       # the faster setting is the baseline
            t_sam, cores = t_all, nproc
    per_frame = t_sam + t_ism + t_pem
    return {"value": 1.0 / per_frame, "unit": "frames/s", "cores": cores, "nproc": nproc, "kind": "port", "all_cores_check": all_cores,
            "sample": f"1 warm-up + median of 3 per leg: 1 SAM ViT-H frame ({t_sam:.2f}s; runs "
                      f"{'/'.join(f'{t:.2f}' for t in sam_runs)}) + 1 ISM frame P=128 ({t_ism:.3f}s) + PEM batch of {NB} "
                      f"({t_pem:.2f}s/instance; runs {'/'.join(f'{t / NB:.2f}' for t in pem_runs)}), fp32 torch CPU oracle "
                      "(no reference tree on this host: the reference's own modules are timed where it exists, profiles/r05_cpu_baseline_reference.json)"}


def fp8_config(hp, dev, args, mode="fp8"):
    from sam6d_amd import ops
    if not (ops.have("gemm_fp8") and ops.have("layernorm_fp8")) or (mode == "fp8mx" and not ops.have("gemm_fp8_mx")):
        return {"error": "fp8 kernels not in the library"}
    old = os.environ.get("S6D_SAM_GEMM")
    os.environ["S6D_SAM_GEMM"] = mode; __import__("sam6d_amd.policy").policy.reload()
    try:
        for _ in range(max(1, args.warmup)):
            hp.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            hp.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        sam_ms = stage_ms(hp.sam_stage, 1)
        kr = [k for k in kernel_rooflines(dev, args.sam_chunk, args.frames, gemm_ms_inside_the_step(hp))
              if (k["kernel"].startswith(("gemm_fp8", "layernorm_fp8")) or k["kernel"].startswith("gemm_bf16")) and k["launches_per_step"]]
        dom = max((k for k in kr if k["kernel"].startswith("gemm_fp8")), key=lambda k: k["avg_ms"] * k["launches_per_step"])
        return {"headline": False, "workload": "BASELINE configs[4] 'fp8 ViT-H MFMA path' on the configs[1] workload (same frames, same stages)",
                "value": round(args.frames * args.steps / dt, 3), "unit": "frames/s", "ms_per_step": round(dt / args.steps * 1e3, 3),
                "steps": args.steps, "dtype": ("fp8 e4m3 operands / f32 accumulation: SAM ViT-H qkv and lin1 (per-token / per-channel power-of-two "
                                              "scales)" + (", lin2 on lin1's MX-scaled e4m3 output (one E8M0 scale per token and 32 channels)"
                                                           if mode == "fp8mx" else "") + "; proj, attention and everything else as the headline"),
                "sam_encoder_ms": round(sam_ms, 2),
                "roofline": {"kernel": dom["kernel"], "bound": "mfma", "achieved": dom["achieved"], "peak": dom["peak"],
                             "unit": dom["unit"], "frac": dom["frac"], "avg_launch_ms": dom["avg_ms"], "traffic": _pmc_traffic(dom),
                             "traffic_source": "profiles/r0*_pmc_summary.json (stored rocprofv3 --pmc passes, not this run)"},
                "kernels": kr, "accuracy_gate": "tests/test_gpu_fp8.py"}
    finally:
        os.environ.pop("S6D_SAM_GEMM") if old is None else os.environ.__setitem__("S6D_SAM_GEMM", old); __import__("sam6d_amd.policy").policy.reload()



def host_inputs_rate(hp, dev, args):
    """The same step with the batch handed over as HOST buffers (the task contract: the PCIe-inclusive rate is reported beside
    `value`, never as it).  What the reference's drivers upload per frame: the frame resized to long side 1024 as uint8 HWC
    (segment_anything/predictor.py:57-60 `torch.as_tensor(input_image, device=...)` then permute) and the PEM's per-instance
    observed inputs (Pose_Estimation_Model/run_inference_custom.py:266-279 `.cuda()` of pts, rgb, rgb_choose; the template side --
    model, dense_po, dense_fo -- is made on the device once per object by get_obj_feats and stays resident).
    Here: pinned host tensors, uploaded at the head of every step on the step's stream (no overlap with the previous step: the
    upper bound of the cost), then the u8 HWC -> float CHW conversion on the device; the ISM stage's inputs are device products
    of the descriptor model in the real flow and stay resident."""
    F = hp.F
    keep_raw, keep_pem = hp.sam_raw, hp.pem_in
    host_img = keep_raw.permute(0, 2, 3, 1).to(torch.uint8).cpu().pin_memory()                 # (F,768,1024,3) u8
    host_pem = {k: keep_pem[k].cpu().pin_memory() for k in ("pts", "rgb", "rgb_choose")}
    nbytes = host_img.numel() + sum(v.numel() * v.element_size() for v in host_pem.values())

    def upload():
        hp.sam_raw = host_img.to(dev, non_blocking=True).permute(0, 3, 1, 2).float()
        hp.pem_in = dict(keep_pem, **{k: v.to(dev, non_blocking=True) for k, v in host_pem.items()})

    def step():
        upload()
        return hp.step()

    try:
        step()
        torch.cuda.synchronize(dev)
        n = max(2, min(args.steps, 4))
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        torch.cuda.synchronize(dev)
        ms = (time.perf_counter() - t0) * 1e3 / n
        up = _event_ms(upload, 3)
    finally:
        hp.sam_raw, hp.pem_in = keep_raw, keep_pem
    return {"frames_per_s": round(F / (ms * 1e-3), 2), "ms_per_step": round(ms, 2), "host_mb_per_step": round(nbytes / 1e6, 1),
            "upload_ms_alone": round(up, 3), "upload_gb_per_s": round(nbytes / (up * 1e-3) / 1e9, 1),
            "note": "pinned host buffers uploaded at the head of every step on the step's stream (no overlap with compute), u8 HWC -> float CHW on the device"}

def _extras(extra, hp, dev, args, world):
    """Stage split, per-kernel rooflines, whole-frame block and CPU baseline: rank 0, outside the timed region."""
    sam_ms = stage_ms(hp.sam_stage, 1)
    ism_ms = stage_ms(hp.ism_stage, 1)
    pem_ms = stage_ms(hp.pem_stage, 1)
    achieved = SAM_FLOP_PER_FRAME * args.frames / (sam_ms * 1e-3)
    extra["stages_ms"] = {"sam_encoder": round(sam_ms, 2), "ism_scoring": round(ism_ms, 2), "pem": round(pem_ms, 2)}
    # the other two extractor dtypes next to the headline one: fp32 (library GEMMs) and bf16 (misses the 1e-3 mm translation bar)
    cur = os.environ.get("S6D_PEM_VIT_DTYPE")
    alt = {}
    for dt_ in ("fp32", "fp16", "bf16"):
        if dt_ == cur:
            continue
        os.environ["S6D_PEM_VIT_DTYPE"] = dt_; __import__("sam6d_amd.policy").policy.reload()
        try:
            alt[dt_] = round(stage_ms(hp.pem_stage, 1), 2)
        finally:
            os.environ["S6D_PEM_VIT_DTYPE"] = cur; __import__("sam6d_amd.policy").policy.reload()
    # parity of each extractor dtype is NOT measured by this run: tests/test_gpu_pem.py::test_net_forward_well_conditioned_vs_
    # reference_golden holds fp32 / fp16 to 1e-3 mm against tests/golden/pem_wc.npz and records the margins
    # (profiles/r*_parity_margins_final.jsonl)
    extra["pem_vit_dtype"] = {"benched": cur, "library_default": "fp32", "pem_stage_ms": {cur: round(pem_ms, 2), **alt},
                              "parity": "tests/test_gpu_pem.py::test_net_forward_well_conditioned_vs_reference_golden"}
    kr = kernel_rooflines(dev, args.sam_chunk, args.frames, gemm_ms_inside_the_step(hp))
    dom = max((k for k in kr if not k["kernel"].startswith("library")),
              key=lambda k: k["avg_ms"] * k["launches_per_step"])
    # the dominant kernel of the step (largest avg duration x launches per step) -- since round 2 the hand-written bf16 GEMM;
    # the library GEMM is listed in `kernels` for comparison only (it is not on the path)
    extra["roofline"] = {"kernel": dom["kernel"], "bound": dom["bound"], "achieved": dom["achieved"],
                         "peak": dom["peak"], "unit": dom["unit"], "frac": dom["frac"],
                         "avg_launch_ms": dom["avg_ms"], "traffic": _pmc_traffic(dom),
                         "traffic_source": "profiles/r0*_pmc_summary.json (stored rocprofv3 --pmc passes of the same command, not this run)"}
    if "algorithmic_bytes" in dom:
        extra["roofline"]["algorithmic_bytes"] = dom["algorithmic_bytes"]
    extra["kernels"] = kr
    extra["stage_roofline"] = {"stage": f"SAM ViT-H encoder, {args.frames} frames (bf16 GEMMs + fused attention)",
                               "bound": "mfma", "achieved": round(achieved / 1e12, 2), "peak": MFMA_BF16_PEAK / 1e12,
                               "unit": "TFLOP/s", "frac": round(achieved / MFMA_BF16_PEAK, 4)}
    if world == 1:
        try:
            extra["host_inputs"] = host_inputs_rate(hp, dev, args)
        except Exception as e:  # noqa: BLE001
            extra["host_inputs"] = {"error": f"{type(e).__name__}: {e}"}
    if world == 1 and args.config == "lmo" and not args.no_fp8:
        # BASELINE configs[4] ("fp8 ViT-H MFMA path") measured by THIS run, next to the headline and never as it (VERDICT r3 item 8:
        # every fp8 number had been builder-run): the same HotPath with the SAM encoder's GEMMs switched to the fp8 matrix cores,
        # the same timing protocol (warm-up steps, then `steps` steps between device synchronisations), its own roofline row
        # against the 5 PFLOP/s dense fp8 peak.
        extra["configs"] = {}
        for mode in ("fp8", "fp8mx"):                      # fp8: qkv + lin1 (round 3);  fp8mx: + lin2 through MX block scales (round 4)
            try:
                extra["configs"][mode] = fp8_config(hp, dev, args, mode)
            except Exception as e:  # noqa: BLE001
                extra["configs"][mode] = {"error": f"{type(e).__name__}: {e}"}
    if world == 1 and not args.no_pipeline:
        # what a whole frame costs: every stage of the chain incl. mask decoding, DINOv2 descriptors and the PEM
        # pre-processing, K = 10 instances per frame; outside the timed region, reported next to the headline
        try:
            hp.__dict__.clear()                                   # release the step's models before the five-model chain is built
            torch.cuda.empty_cache()
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import frame_demo
            extra["pipeline"] = frame_demo.measure(dev)
            built = extra["pipeline"].pop("_built")
            best = "fp8"            # the configs[4] answer (tests/test_gpu_fp8.py: fp8mx misses the mask-agreement share bound and is opt-in)
            if isinstance(extra.get("configs", {}).get(best), dict) and "error" not in extra["configs"][best]:
                # the same whole frame in the fp8 configuration: SAM ViT-H AND DINOv2 ViT-L on the fp8 cores (fp8mx: lin2 / fc2 too)
                old = {k: os.environ.get(k) for k in ("S6D_SAM_GEMM", "S6D_DINO_GEMM")}
                os.environ.update(S6D_SAM_GEMM=best, S6D_DINO_GEMM=best); __import__("sam6d_amd.policy").policy.reload()
                try:
                    torch.cuda.empty_cache()
                    pf = frame_demo.measure(dev, built=built)
                    extra["configs"][best]["pipeline"] = {k: pf[k] for k in ("frames_per_s", "ms_per_frame", "ms_per_frame_in_groups_of_8", "stages_ms")}
                finally:
                    for k, v in old.items():
                        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        except Exception as e:  # noqa: BLE001
            extra["pipeline"] = {"error": f"{type(e).__name__}: {e}"}
        # BASELINE configs[2]'s program (frames with varying proposal / instance counts through utils/shard.run_sharded) on this one rank
        try:
            built = None
            torch.cuda.empty_cache()
            from tools import run_sharded
            extra["sharded_world1"] = run_sharded.measure_world1(dev)
        except Exception as e:  # noqa: BLE001
            extra["sharded_world1"] = {"error": f"{type(e).__name__}: {e}"}
    if world == 1 and not args.no_cpu_baseline:
        extra["cpu_baseline"] = cpu_baseline()


class StandInPath:
    """TEST INFRASTRUCTURE (--standin): the shape of HotPath.step() without the models -- a deterministic (frames, 17) record block
    per rank on the CPU, so that the launcher, the barriers, the all_gather of the pose records and the JSON line can be run over
    gloo on a host without GPUs.  Never a measurement: the printed line carries "standin": true."""

    def __init__(self, device, frames, rank):
        self.dev, self.F, self.rank = device, frames, rank

    def step(self):
        from sam6d_amd.utils import shard
        g = torch.Generator().manual_seed(100 + self.rank)
        R = torch.randn(self.F, 3, 3, generator=g)
        t = torch.randn(self.F, 3, generator=g)
        return shard.pack_records(self.rank, torch.arange(self.F), 5, torch.full((self.F,), 0.5), R, t, 0.0).to(self.dev)


DUMP_BYTES = 60 * 10 ** 6      # --dump-outputs: the arrays stay under this (64 MB with the .npy headers)
DUMP_SAMPLE = 1 << 20          # at most this many elements per array: a seeded sample of the flat positions of a larger one


def dump_outputs(dirname, outputs, records):
    """--dump-outputs: what the last timed step computed, as DIR/<name>.npy.  Floating point arrays are written as float32
    (float64 stays float64), integer and boolean ones as float64, which holds them exactly.  An array of more than `cap` elements
    is written as the 1-D sample at `cap` flat positions drawn by torch.randint with seed 0 and sorted: the same positions for
    the same shape in every run.  Names: sam_image_embeddings (every frame of the step), ism_group<k>_<key> (one set per
    scoring launch group), pem_<key> (the keys Net.forward adds to its inputs) and pose_records (the gathered 68-byte records
    the step ends with)."""
    import numpy as np
    arrays = {"pose_records": records}
    if outputs:
        arrays["sam_image_embeddings"] = torch.cat(outputs["sam"])
        for k, group in enumerate(outputs["ism"]):
            arrays.update({f"ism_group{k}_{key}": v for key, v in group.items()})
        arrays.update({f"pem_{key}": v for key, v in outputs["pem"].items()})
    os.makedirs(dirname, exist_ok=True)
    cap = min(DUMP_SAMPLE, DUMP_BYTES // (8 * len(arrays)))   # 8 bytes per element at most: the bound holds by construction
    for name, t in sorted(arrays.items()):
        t = torch.as_tensor(t).detach()
        flat = t.reshape(-1)
        sampled = flat.numel() > cap
        if sampled:
            g = torch.Generator().manual_seed(0)
            flat = flat[torch.randint(flat.numel(), (cap,), generator=g).sort().values.to(flat.device)]
        a = flat.cpu().to(torch.float32 if t.is_floating_point() and t.dtype != torch.float64 else torch.float64).numpy()
        a = a if sampled else a.reshape(tuple(t.shape))
        np.save(os.path.join(dirname, name + ".npy"), a)


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_ranks(n, argv=None):
    """`python bench.py --gpus N` (N > 1) started WITHOUT a torch.distributed.run parent: become the launcher.  Re-executes this
    file as N ranks of one node -- one process per GPU, rendezvous on 127.0.0.1 (the container hostname may not resolve), dmabuf
    IPC for RCCL -- exactly the command form the driver uses; rank 0's stdout (the one JSON line) passes through.  The reference
    starts its multi-GPU runs the same way: one Lightning process per device (Instance_Segmentation_Model/run_inference.py:25,
    74-77; Pose_Estimation_Model/test_bop.py:205-206 is single-GPU)."""
    import subprocess
    argv = list(sys.argv[1:] if argv is None else argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or n) // n)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + argv
    return subprocess.call(cmd, env=env)


def main():
    args = parse()
    if args.cpu_baseline_only:
        print(json.dumps(cpu_baseline()))
        return
    if "WORLD_SIZE" not in os.environ and (args.gpus or 1) > 1:
        sys.exit(launch_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus is None:
        args.gpus = world
    if args.gpus != world:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: start it as `python bench.py --gpus N` or as "
                         f"`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`")
    dist = None
    if args.standin:
        dev = torch.device("cpu")
        sync = lambda: None                                     # noqa: E731
        backend = "gloo"
    else:
        assert torch.cuda.is_available(), "bench.py measures the MI355X path; no GPU visible"
        assert torch.cuda.device_count() > local, f"rank {rank}: LOCAL_RANK {local} but {torch.cuda.device_count()} GPU(s) visible"
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)
        sync = torch.cuda.synchronize
        backend = "nccl"
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        assert dist.get_world_size() == args.gpus

    if args.config in ("fp8", "fp8mx"):
        os.environ["S6D_SAM_GEMM"] = args.config; __import__("sam6d_amd.policy").policy.reload()
    if not args.standin:
        benched_policy()
    if args.strict and not args.standin:
        os.environ["S6D_STRICT"] = "1"; __import__("sam6d_amd.policy").policy.reload()
    if args.gemm_wave_tile and not args.standin:
        from sam6d_amd import ops as _ops
        global _GEMM_WAVE_TILE
        _GEMM_WAVE_TILE = args.gemm_wave_tile
        _ops.set_gemm_wave_tile(args.gemm_wave_tile)
    hp = StandInPath(dev, args.frames, rank) if args.standin else HotPath(dev, args.frames, args.sam_chunk)
    hp.keep_outputs = bool(args.dump_outputs)

    def barrier():
        sync()
        if dist is not None:
            dist.barrier()
        sync()

    def run_step():
        rec = hp.step()
        if dist is not None:
            out = torch.empty(world * rec.shape[0], rec.shape[1], device=dev)
            dist.all_gather_into_tensor(out, rec.contiguous())
            return out
        return rec

    for _ in range(args.warmup):
        run_step()
    barrier()
    t0 = time.perf_counter()
    last = None
    for _ in range(args.steps):
        last = run_step()
    barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, getattr(hp, "outputs", None), last)

    ms_step = dt / args.steps * 1e3
    value = world * args.frames * args.steps / dt
    # library (rocBLAS / ATen) branches the modules took on CUDA tensors during warm-up + the timed steps (sam6d_amd/policy.py::guard):
    # the benched step is expected to take none
    lib_hits = {} if args.standin else {f"{s}:{g}": n for (s, g), n in __import__("sam6d_amd.policy").policy.library_branch_hits().items()}
    if dist is not None:
        # the process group ends HERE, with every rank present: with --full rank 0 goes on alone into minutes of side measurements,
        # and a destroy_process_group issued after the other ranks have exited may wait on them
        dist.barrier()
        dist.destroy_process_group()
        dist = None

    # --full: stage breakdown + roofline of the dominant stage and the other side blocks (rank 0 only; outside the timed region)
    extra = {"library_branches_in_the_timed_steps": lib_hits, "strict": bool(args.strict)}
    if args.standin:
        extra["standin"] = True
        extra["gathered_rows"] = int(last.shape[0])
        extra["gathered_ranks"] = sorted({int(v) for v in last[:, 0].tolist()})
    elif rank == 0 and args.full and not args.no_extras:
        try:
            _extras(extra, hp, dev, args, world)
        except Exception as e:  # noqa: BLE001  (the headline line must come out even if a side measurement fails)
            extra["extras_error"] = f"{type(e).__name__}: {e}"

    if rank == 0:
        line = {"metric": "RGB-D frames/sec (SAM-6D per-frame hot path: SAM ViT-H encoder + ISM scoring + PEM)",
                "value": round(value, 3), "unit": "frames/s", "n_gpus": world, "steps": args.steps,
                "warmup": args.warmup, "ms_per_step": round(ms_step, 3), "higher_is_better": True,
                "scaling": "weak", "vs_baseline": None, "dtype": "bf16 (SAM ViT-H: 87 % of the step) + f16 (PEM ViT-B feature extractor) + f32 (ISM scoring, PEM point transformer and pose solvers)",
                "data": "synthetic",
                "config": {"workload": "LM-O single object: 32 frames/step/GPU, 640x480 RGB-D -> 1024^2 SAM input, "
                                       "P=128 proposals x 42 templates (scored in groups of 8 frames), 1 instance/frame, 2048 pts (PEM batch 32)",
                           "frames_per_step_per_gpu": args.frames, "sam_frames_per_launch_group": args.sam_chunk,
                           "pem_vit_dtype": os.environ.get("S6D_PEM_VIT_DTYPE", "fp32") + " (set by bench.py; the library default is fp32)",
                           "sharding": f"frames over {world} rank(s)"}}
        if args.config in ("fp8", "fp8mx"):
            line["dtype"] = ("fp8 e4m3 operands / f32 accumulation (SAM ViT-H qkv and lin1 GEMMs; per-token and per-output-channel "
                             "power-of-two scales) + bf16 (every other ViT op) + f32 (ISM scoring, PEM point transformer and pose solvers)")
            line["config"]["workload"] = ("BASELINE configs[4] 'fp8 ViT-H MFMA path' on the configs[1] workload (the FastSAM segmentor and "
                                          "the 7-dataset sweep of configs[4] are outside the north-star path): " + line["config"]["workload"])
            line["config"]["headline"] = False
        if args.standin:
            line["metric"] = "STAND-IN STAGES ON THE CPU (launcher / gather test, not a measurement)"
            line["data"], line["dtype"] = "stand-in", "-"
        line.update(extra)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
