"""Per-stage wall times of the MI355X PEM path (diagnostic; run on the GPU box):
python tools/stage_times.py [B]
python tools/stage_times.py --geo-ab [result.json]   the geo_embedding stage alone, policy field geo_from_points "0" / "1" alternating
                                                     in this process at 32 and 10 instances (quoted in profiles/geo_from_points.md)
python tools/stage_times.py --coarse-sim-ab [result.json]   the step from the out_proj outputs to atten alone (pm.feature_similarity), policy
                                                     field coarse_sim "0" / "1" alternating in this process at 32 and 10 instances (quoted
                                                     in profiles/coarse_similarity.md)
python tools/stage_times.py --render [result.json [OTHER.so]]   ops.render_views and ops.render_views_textured (2048 x 2048 texture)
                                                     alone: 42 views of 480 x 640 of a 45,600-face torus (one lane per
                                                     triangle) and of a 12-face cube (a workgroup per triangle), the pyramid build,
                                                     beside the time of one device copy of the key buffer -- its bytes read once and
                                                     written once at the copy rate, the floor of the visibility pass; with OTHER.so
                                                     (the parent commit's library) ops.render_views through both builds, alternating
                                                     (quoted in profiles/render.md)
python tools/stage_times.py --bop-eval [result.json]   the BOP pose errors (sam6d_amd.evaluation): kernels beside the library statements in
                                                     this process -- MSSD / MSPD of 256 estimates, 20,000 vertices, 1 and 315 symmetries;
                                                     the two depth renders and the pixel stage of VSD at 480 x 640 with 10 taus --
                                                     with the launches and the peak requested bytes of either branch and the floor of
                                                     the pixel stage (quoted in profiles/bop_eval.md)
python tools/stage_times.py --fine-match-ab OTHER.so [result.json]   ops.fine_match at B = 32, 2049 x 2049 with this tree's library and with
                                                     another build of it (the parent commit's) loaded into the same process,
                                                     alternating, three runs each (quoted in profiles/pose_solver_margins.md)"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from sam6d_amd import policy  # noqa: E402
from sam6d_amd.pem import pose_estimation_model as pm  # noqa: E402
from sam6d_amd.utils import seeded, synth  # noqa: E402


def timed(name, fn, n=3):
    fn()
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(n):
        out = fn()
    torch.cuda.synchronize()
    print(f"{name:28s} {(time.time() - t0) / n * 1e3:9.2f} ms", flush=True)
    return out


def main(B=32):
    net = pm.Net(pm.default_cfg()).eval()
    seeded.load_seeded(net, 1)
    net = net.cuda()
    inp = {k: v.cuda() for k, v in synth.pem_inputs(B, seed=1).items()}
    ru = synth.coarse_uniforms(B, 2).cuda()
    with torch.no_grad():
        fe = net.feature_extraction
        timed("vit tokens_up", lambda: fe.rgb_net.tokens_up(inp["rgb"]))
        dpm, dfm, dpo, dfo, rad = timed("feature_extraction", lambda: fe(inp))
        spm, sfm, im = timed("fps+gather", lambda: pm.sample_pts_feats(dpm, dfm, 196))
        spo, sfo, io = pm.sample_pts_feats(dpo, dfo, 196)
        bg = torch.full((B, 1, 3), 100.0, device="cuda")
        gm = timed("geo_embedding", lambda: net.geo_embedding(torch.cat([bg, spm], 1)))
        go = net.geo_embedding(torch.cat([bg, spo], 1))
        ep = dict(model=inp["model"], coarse_rand_u=ru)
        ep = timed("coarse matching", lambda: net.coarse_point_matching(spm, sfm, gm, spo, sfo, go, rad, dict(ep)))
        timed("fine matching", lambda: net.fine_point_matching(dpm, dfm, gm, im, dpo, dfo, go, io, rad, dict(ep)))
        timed("PE", lambda: net.fine_point_matching.PE(dpo))
        timed("Net.forward", lambda: net(dict(inp, coarse_rand_u=ru)))
    print("max mem GB", torch.cuda.max_memory_allocated() / 2**30)


def _event_ms(fn, calls):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def _launches(fn):
    """Device kernels of one call, by name (torch.profiler, a pass of its own)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = {}
    for ev in prof.events():
        if str(getattr(ev, "device_type", "")).endswith("CUDA") and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower():
            names[ev.name] = names.get(ev.name, 0) + 1
    return names


def geo_ab(path=None, rounds=7, calls=20):
    """net.geo_embedding on the 197-token cloud from the points ("1") against the path through the idx4 tensor ("0"): device-event
    times of alternating rounds, the largest difference of the two embeddings, the device launches of one call of either path."""
    net = seeded.load_seeded(pm.Net(pm.default_cfg()).eval(), 1).cuda()
    geo = net.geo_embedding
    out = {"rounds": rounds, "calls_per_round": calls, "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        for B in (32, 10):
            g = torch.Generator().manual_seed(B)
            pts = torch.randn(B, 197, 3, generator=g) * 0.5
            pts[:, 0] = 100.0
            pts = pts.cuda()
            rows = {"0": [], "1": []}
            for _ in range(rounds):
                for mode in ("0", "1"):
                    with policy.use(geo_from_points=mode):
                        rows[mode].append(round(_event_ms(lambda: geo(pts), calls), 4))
            with policy.use(geo_from_points="0"):
                a = geo(pts)
            with policy.use(geo_from_points="1"):
                b = geo(pts)
            off = ~torch.eye(197, dtype=torch.bool, device="cuda").expand(B, 197, 197)
            d = (a - b).abs()
            r = {"idx4_path_ms": rows["0"], "from_points_ms": rows["1"], "idx4_path_median_ms": statistics.median(rows["0"]),
                 "from_points_median_ms": statistics.median(rows["1"]), "max_abs_diff_off_diagonal": d[off].max().item(),
                 "max_abs_diff_diagonal": d[~off].max().item(), "mean_abs_diff": d.mean().item()}
            print(B, r, flush=True)
            for mode, key in (("0", "idx4_path_launches"), ("1", "from_points_launches")):
                with policy.use(geo_from_points=mode):
                    names = _launches(lambda: geo(pts))
                r[key] = {"total": sum(names.values()), "library": sum(v for k, v in names.items() if "s6d" not in k), "by_name": names}
                print(B, key, r[key]["total"], "library:", r[key]["library"], flush=True)
            out[f"B{B}"] = r
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    else:
        print(json.dumps(out))


def coarse_sim_ab(path=None, rounds=9, calls=50):
    """pm.feature_similarity on (B,197,256) out_proj-shaped features at temp 0.1: the kernel ("1") against the library statements ("0",
    two normalisations, a transpose, a bmm and a divide): device-event times of alternating rounds, their medians, the spread of the
    library rounds (the margin of the comparison), the largest difference of the two results, the device launches of one call."""
    out = {"rounds": rounds, "calls_per_round": calls, "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        for B in (32, 10):
            g = torch.Generator().manual_seed(B)
            o1 = torch.randn(B, 197, 256, generator=g)
            o2 = (o1 + 0.2 * torch.randn(B, 197, 256, generator=g)).cuda()
            o1 = o1.cuda()
            step = lambda: pm.feature_similarity(o1, o2, 0.1)  # noqa: E731
            rows = {"0": [], "1": []}
            for _ in range(rounds):
                for mode in ("0", "1"):
                    with policy.use(coarse_sim=mode):
                        rows[mode].append(round(_event_ms(step, calls) * 1e3, 2))
            with policy.use(coarse_sim="0"):
                a = step()
            with policy.use(coarse_sim="1", strict="1"):
                b = step()
            r = {"library_us": rows["0"], "kernel_us": rows["1"], "library_median_us": statistics.median(rows["0"]),
                 "kernel_median_us": statistics.median(rows["1"]), "library_spread_us": round(max(rows["0"]) - min(rows["0"]), 2),
                 "max_abs_diff": (a - b).abs().max().item()}
            r["kernel_no_slower"] = r["kernel_median_us"] <= r["library_median_us"] + r["library_spread_us"]
            print(B, r, flush=True)
            for mode, key in (("0", "library_launches"), ("1", "kernel_launches")):
                with policy.use(coarse_sim=mode):
                    names = _launches(step)
                r[key] = {"total": sum(names.values()), "library": sum(v for k, v in names.items() if "s6d" not in k), "by_name": names}
                print(B, key, r[key]["total"], "library:", r[key]["library"], flush=True)
            out[f"B{B}"] = r
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    else:
        print(json.dumps(out))


def render_times(path=None, rounds=5, calls=200, other=None):
    """ops.render_views and ops.render_views_textured (a 2048 x 2048 texture) on the two work shapes at the reference's template
    size (42 views, 480 x 640, the LM camera of Instance_Segmentation_Model/utils/poses/pyrender.py:88-91): device-event times per
    call (workspace allocation and the face-index check of the wrapper included), the covered pixels, the triangles the workgroup
    kernel took, the pyramid build and the copy of the key buffer.  other: the library of another build (the parent commit's):
    ops.render_views through both in alternating rounds, and whether the outputs are equal."""
    import ctypes

    import numpy as np

    from sam6d_amd import _lib, ops
    from tests import render_ref as R
    from tests import texture_ref as X
    T, H, W = 42, 480, 640
    K = (572.4114, 573.57043, 325.2611, 242.04899)
    out = {"views": T, "height": H, "width": W, "rounds": rounds, "calls_per_round": calls, "device": torch.cuda.get_device_name(0)}
    # the floor of the visibility pass: the key buffer written once and read once = one copy of it.  Copied back to back, source and
    # destination (2 x 103 MB) stay in the 256 MiB last-level cache, which is also how the three render launches meet the buffer;
    # rotating over eight pairs (1.65 GB) makes every copy come from and go to HBM.
    pairs = [(torch.zeros(T, H, W, dtype=torch.int64, device="cuda"), torch.empty(T, H, W, dtype=torch.int64, device="cuda")) for _ in range(8)]
    out["key_buffer_bytes"] = pairs[0][0].numel() * 8
    state = {"i": 0}

    def rotate():
        src, dst = pairs[state["i"] % 8]
        state["i"] += 1
        dst.copy_(src)
    for key, fn in (("cached", lambda: pairs[0][1].copy_(pairs[0][0])), ("hbm", rotate)):
        rows = [round(_event_ms(fn, 400), 4) for _ in range(rounds)]
        out[f"key_buffer_copy_{key}_ms"] = rows
        out[f"key_buffer_copy_{key}_median_ms"] = statistics.median(rows)
        out[f"copy_rate_{key}_GBps"] = round(2 * out["key_buffer_bytes"] / statistics.median(rows) / 1e6, 1)
    del pairs[:]
    image = torch.from_numpy(X.texture(2048, 2048, 1)).cuda()
    rows = [round(_event_ms(lambda: ops.texture_pyramid(image), 50), 4) for _ in range(rounds)]
    out["texture_pyramid_2048_ms"], out["texture_pyramid_2048_median_ms"] = rows, statistics.median(rows)
    pyramid = ops.texture_pyramid(image)
    libs = {"this": _lib.lib()}
    if other:
        libs["other"] = ctypes.CDLL(other)
    meshes = (("torus_45600_faces", R.torus(152, 150), lambda f: X.expand(X.torus_uv(152, 150), f)), ("cube_12_faces", R.cube(), lambda f: X.cube_uv()))
    for name, (v, f, c), uv_of in meshes:
        P = R.poses(T, seed=1, t=(0.0, 0.0, 300.0))
        tv, tf, tc, tp, tu = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (v, f, c, P, uv_of(f)))
        step = lambda: ops.render_views(tv, tf, tc, tp, *K, H, W, 0.3, 0.7, 1.0)  # noqa: E731
        tex = lambda: ops.render_views_textured(tv, tf, tu, pyramid, tp, *K, H, W, 0.3, 0.7, 1.0, tex_size=(2048, 2048))  # noqa: E731
        ms, res = {k: [] for k in libs}, {}
        try:
            for r in range(rounds + 1):                              # round 0 warms every build up
                for k in sorted(libs):
                    _lib._lib = libs[k]
                    t = _event_ms(step, calls)
                    if r:
                        ms[k].append(round(t, 4))
                    res[k] = step()
        finally:
            _lib._lib = libs["this"]
        rows_tex = [round(_event_ms(tex, calls), 4) for _ in range(rounds)]
        got = tex()
        r = {"faces": int(tf.shape[0]), "ms": ms["this"], "median_ms": statistics.median(ms["this"]), "textured_ms": rows_tex,
             "textured_median_ms": statistics.median(rows_tex), "covered_pixels_per_view": int((res["this"]["mask"] == 255).sum()) // T,
             "skipped": int(res["this"]["skipped"].sum()), "launches": _launches(step), "textured_launches": _launches(tex),
             "textured_geometry_equal": all(bool(torch.equal(got[k], res["this"][k])) for k in ("mask", "xyz", "depth", "face", "skipped"))}
        if other:
            r.update(other_ms=ms["other"], other_median_ms=statistics.median(ms["other"]),
                     ratio_of_medians=round(statistics.median(ms["this"]) / statistics.median(ms["other"]), 4),
                     outputs_equal_other=all(bool(torch.equal(res["this"][k], res["other"][k])) for k in res["this"]))
        print(name, r, flush=True)
        out[name] = r
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    else:
        print(json.dumps(out))


def fine_match_ab(other, path=None, rounds=3, calls=20):
    """ops.fine_match at the benched size through two builds of the library in one process (ctypes keeps two copies of a library apart
    when their paths differ): device-event times of alternating runs, means, the spread of the other build's own runs and whether
    this build's mean lies within it; the labels of the two builds compared."""
    import ctypes

    from sam6d_amd import _lib, ops
    libs = {"this": _lib.lib(), "other": ctypes.CDLL(other)}
    assert libs["other"].s6d_version() == _lib.abi_version()
    g = torch.Generator(device="cuda").manual_seed(0)
    B, M = 32, 2049
    f1 = torch.randn(B, M, 256, generator=g, device="cuda")
    f2 = f1[:, torch.randperm(M, generator=g, device="cuda")] + 0.4 * torch.randn(B, M, 256, generator=g, device="cuda")
    pts2 = torch.randn(B, M - 1, 3, generator=g, device="cuda")
    rows, outs = {"this": [], "other": []}, {}
    try:
        for r in range(rounds + 1):                                  # round 0 warms both builds up
            for name in ("other", "this"):
                _lib._lib = libs[name]
                ms = _event_ms(lambda: ops.fine_match(f1, f2, pts2, 0.1), calls)
                if r:
                    rows[name].append(round(ms, 4))
                outs[name] = ops.fine_match(f1, f2, pts2, 0.1)
    finally:
        _lib._lib = libs["this"]
    mean = {k: sum(v) / len(v) for k, v in rows.items()}
    out = {"device": torch.cuda.get_device_name(0), "B": B, "M": M, "calls_per_run": calls, "this_ms": rows["this"], "other_ms": rows["other"],
           "this_mean_ms": round(mean["this"], 4), "other_mean_ms": round(mean["other"], 4),
           "this_mean_within_other_runs": min(rows["other"]) <= mean["this"] <= max(rows["other"]), "this_mean_not_above_other_max": mean["this"] <= max(rows["other"]),
           "label_differences": int((outs["this"][2] != outs["other"][2]).sum().item()),
           "wsum_max_abs_diff": (outs["this"][1] - outs["other"][1]).abs().max().item(),
           "pred_max_abs_diff": (outs["this"][0] - outs["other"][0]).abs().max().item()}
    print(json.dumps(out), flush=True)
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


def _peak_bytes(fn):
    """requested_bytes.all.peak of one call above what was held before it."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_stats()["requested_bytes.all.current"]
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.memory_stats()["requested_bytes.all.peak"] - before)


def bop_eval_times(path=None, rounds=5):
    """ops.pose_errors / ops.render_depth / ops.vsd_counts beside the torch statements of sam6d_amd.evaluation: device-event times
    (median of `rounds` rounds), device launches of one call, peak requested bytes of one call, and for the pixel stage of VSD the
    time of reading its three depth images once at the measured HBM copy rate."""
    import numpy as np

    from sam6d_amd import evaluation as ev
    from sam6d_amd import ops
    from tests import bop_ref as B
    from tests import render_ref as R
    N, V, H, W = 256, 20000, 480, 640
    out = {"estimates": N, "vertices": V, "height": H, "width": W, "rounds": rounds, "device": torch.cuda.get_device_name(0)}
    rs = np.random.RandomState(0)
    v = torch.from_numpy(rs.uniform(-60, 60, (V, 3)).astype(np.float32)).cuda()
    gt = B.seeded_poses(N, seed=1)
    est = gt.copy()
    est[:, :3, 3] += rs.uniform(-6, 6, (N, 3))
    e = torch.from_numpy(est.astype(np.float32)).cuda()
    cams = torch.tensor([[572.4114, 573.57043, 325.2611, 242.04899]]).repeat(N, 1).cuda()

    def measure(fn, calls):
        rows = [round(_event_ms(fn, calls), 4) for _ in range(rounds)]
        return {"ms": rows, "median_ms": statistics.median(rows), "launches": _launches(fn), "peak_requested_bytes": _peak_bytes(fn)}
    for S in (1, 315):
        g = torch.from_numpy((gt[:, None] @ B.axis_symmetries(S)[None]).astype(np.float32)).cuda()
        r = {"kernel": measure(lambda: ops.pose_errors(v, e, g, cams), 20), "library": measure(lambda: ev._pose_errors_library(v, e, g, cams), 1 if S > 1 else 5)}
        k, lib = ops.pose_errors(v, e, g, cams), ev._pose_errors_library(v, e, g, cams)
        r["max_abs_difference"] = [float((k[0] - lib[0]).abs().max()), float((k[1] - lib[1]).abs().max())]
        print(f"mssd_mspd_S{S}", r, flush=True)
        out[f"mssd_mspd_S{S}"] = r
    # VSD: a 45,600-face torus at 256 perturbed poses, the measured depth = the ground-truth render with noise and holes
    tv, tf, _ = R.torus(152, 150)
    tv, tf = torch.from_numpy(tv).cuda(), torch.from_numpy(tf).cuda()
    pg = R.poses(N, seed=1, t=(0.0, 0.0, 400.0)).astype(np.float64)
    pe = pg.copy()
    pe[:, :3, 3] += rs.uniform(-8, 8, (N, 3))
    pg, pe = torch.from_numpy(pg.astype(np.float32)).cuda(), torch.from_numpy(pe.astype(np.float32)).cuda()
    out["render_depth"] = measure(lambda: ops.render_depth(tv, tf, pe, cams, H, W, 1.0), 10)
    de, dg = ops.render_depth(tv, tf, pe, cams, H, W, 1.0)["depth"], ops.render_depth(tv, tf, pg, cams, H, W, 1.0)["depth"]
    test = torch.where(dg > 0, dg + 3 * torch.randn_like(dg), torch.full_like(dg, 900.0))
    test[torch.rand_like(test) < 0.1] = 0
    ti = torch.arange(N, dtype=torch.int32).cuda()
    scale = torch.full((N,), 170.0).cuda()
    taus = list(ev.BOP19["vsd_taus"])
    out["vsd_counts"] = {"kernel": measure(lambda: ops.vsd_counts(de, dg, test, ti, cams, 15.0, taus, scale), 20),
                         "library": measure(lambda: ev._vsd_counts_library(de, dg, test, ti, cams, 15.0, taus, scale), 2)}
    a, b = ops.vsd_counts(de, dg, test, ti, cams, 15.0, taus, scale), ev._vsd_counts_library(de, dg, test, ti, cams, 15.0, taus, scale)
    out["vsd_counts"]["counts_differ_at_most"] = max(int((x - y).abs().max()) for x, y in zip(a, b))
    out["vsd_counts"]["mean_union"] = float(a[0].float().mean())
    # the floor of the pixel stage: its three inputs read once.  The copy rate comes from copies that rotate over buffers larger than
    # the last-level cache together (4 x 2 x 315 MB)
    nbytes = 3 * de.numel() * 4
    pairs = [(torch.zeros_like(de), torch.empty_like(de)) for _ in range(4)]
    state = {"i": 0}

    def rotate():
        src, dst = pairs[state["i"] % 4]
        state["i"] += 1
        dst.copy_(src)
    rows = [round(_event_ms(rotate, 40), 4) for _ in range(rounds)]
    rate = 2 * de.numel() * 4 / statistics.median(rows) / 1e6
    out["vsd_counts"].update(input_bytes=nbytes, copy_rate_hbm_GBps=round(rate, 1), floor_ms=round(nbytes / rate / 1e6, 4))
    print("vsd", out["render_depth"], out["vsd_counts"], flush=True)
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    else:
        print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--bop-eval":
        bop_eval_times(sys.argv[2] if len(sys.argv) > 2 else None)
    elif len(sys.argv) > 1 and sys.argv[1] == "--render":
        render_times(sys.argv[2] if len(sys.argv) > 2 else None, other=sys.argv[3] if len(sys.argv) > 3 else None)
    elif len(sys.argv) > 1 and sys.argv[1] == "--geo-ab":
        geo_ab(sys.argv[2] if len(sys.argv) > 2 else None)
    elif len(sys.argv) > 2 and sys.argv[1] == "--fine-match-ab":
        fine_match_ab(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    elif len(sys.argv) > 1 and sys.argv[1] == "--coarse-sim-ab":
        coarse_sim_ab(sys.argv[2] if len(sys.argv) > 2 else None)
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 32)
