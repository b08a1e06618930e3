"""The per-image metric stage of the eval harness at 1080p, host path against the fused kernels, on an active-nerfacto and
an active-splatfacto render of the synthetic scenes.

  (a) host   eval.image_metrics_unc(fused=False): torch sorts / cumsums / conv2d and ~20 blocking reads
  (b) fused  eval.image_metrics_unc(fused=True): one unerf_image_metrics call, one copy of its row, numpy finish
Median over --reps HIP-synchronised repetitions after warm-up, both in the same process on the same render.  The fused
entry point is also timed with HIP events, whole and by flag set (the difference between sets prices the kernels behind a
flag: stats + AUCE histogram + NLL; the three radix sorts + cut sums of AUSE; SSIM), and the whole image (render + metrics,
the reference's num_rays_per_sec counter) is timed through eval.get_average_uncertainty_metrics for both.
One JSON -> profiles/<tag>_eval_metrics_fused.json.

    python benchmarks/eval_metrics_fused.py --tag r7
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def _event_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="r7")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--splats", type=int, default=1_000_000)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from uncertainty_nerf_gs_amd import eval as E, lib as L, ops, render, splat, synthetic
    L.build_library()
    L.require_gpu()
    dev = torch.device("cuda:0")
    H, W = args.height, args.width
    cam = dict(fx=1111.0 * W / 1920, fy=1111.0 * W / 1920, cx=W / 2, cy=H / 2, H=H, W=W)

    sd = synthetic.scene_to_device(synthetic.make_scene_tensors(seed=0, kind="active"), dev)
    gp = {k: v.to(dev) for k, v in synthetic.make_splat_tensors(seed=7, N=args.splats).items()}
    bg = torch.zeros(3, device=dev)
    renders = {
        "active-nerfacto": (lambda c2w: render.render_camera(sd, c2w, **cam),
                            [synthetic.orbit_c2w(0.3 * i) for i in range(args.views)]),
        "active-splatfacto": (lambda c2w: splat.active_splatfacto_outputs(gp, c2w, background=bg, **cam),
                              [synthetic.orbit_c2w(2 * math.pi * i / 24, radius=2.5, height=0.5).to(dev) for i in range(args.views)]),
    }
    result = {"height": H, "width": W, "reps": args.reps, "device": torch.cuda.get_device_name(0), "renders": {}}
    gen = torch.Generator(device=dev).manual_seed(0)
    for name, (fn, views) in renders.items():
        gts = [torch.clamp(fn(v)["rgb"] + 0.05 * torch.randn(H, W, 3, device=dev, generator=gen), 0, 1) for v in views]
        outputs = fn(views[0])
        torch.cuda.synchronize()
        r = {}
        r["host_stage_ms"], r["host_stage_min_ms"], r["host_stage_max_ms"] = _median_ms(
            lambda: E.image_metrics_unc(outputs, gts[0]), args.reps, args.warmup)
        r["fused_stage_ms"], r["fused_stage_min_ms"], r["fused_stage_max_ms"] = _median_ms(
            lambda: E.image_metrics_unc(outputs, gts[0], fused=True), args.reps, args.warmup)
        r["host_over_fused"] = r["host_stage_ms"] / r["fused_stage_ms"]
        rgb, std = outputs["rgb"].contiguous(), outputs["rgb_std"].reshape(H, W).contiguous()
        ws = ops.Workspace()
        sets = {"stats_nll_auce": L.METRICS_NLL | L.METRICS_AUCE, "stats_nll_auce_ause": L.METRICS_NLL | L.METRICS_AUCE | L.METRICS_AUSE,
                "stats_ssim": L.METRICS_SSIM, "all": L.METRICS_ALL}
        ev = {k: _event_ms(lambda f=f: ops.image_metrics(rgb, gts[0], std, image_hw=(H, W), clip_max=1.0, nll_min_sigma=3e-2, flags=f,
                                                         workspace=ws), args.reps, args.warmup) for k, f in sets.items()}
        ev["stats_only"] = _event_ms(lambda: ops.image_metrics(rgb, gts[0], std, image_hw=(H, W), clip_max=1.0, nll_min_sigma=3e-2,
                                                               flags=0, workspace=ws), args.reps, args.warmup)
        r["entry_point_event_ms"] = ev
        r["kernel_groups_event_ms"] = {"stats + reduce + finish": ev["stats_only"],
                                       "NLL + AUCE histogram (inside stats)": ev["stats_nll_auce"] - ev["stats_only"],
                                       "AUSE: 3 radix sorts (36 launches) + cut sums": ev["stats_nll_auce_ause"] - ev["stats_nll_auce"],
                                       "SSIM": ev["stats_ssim"] - ev["stats_only"]}
        eval_set = list(zip(views, gts))
        for label, fused in (("host", False), ("fused", True)):
            E.get_average_uncertainty_metrics(fn, eval_set[:1], fused=fused)      # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            avg, _ = E.get_average_uncertainty_metrics(fn, eval_set, fused=fused)
            torch.cuda.synchronize()
            r[f"whole_image_{label}_ms"] = (time.perf_counter() - t0) * 1e3 / len(eval_set)
            r[f"num_rays_per_sec_{label}"] = avg["num_rays_per_sec"]
            r[f"render_rays_per_sec_{label}"] = avg["render_rays_per_sec"]
            r[f"metrics_{label}"] = {k: avg[k] for k in avg if k.startswith(("psnr", "ssim", "rgb_"))}
        result["renders"][name] = r
        print(f"{name}: host stage {r['host_stage_ms']:.2f} ms, fused stage {r['fused_stage_ms']:.2f} ms "
              f"({r['host_over_fused']:.1f}x), entry point {ev['all']:.3f} ms; whole image {r['whole_image_host_ms']:.2f} -> "
              f"{r['whole_image_fused_ms']:.2f} ms")
    result["win"] = all(r["fused_stage_ms"] <= 0.5 * r["host_stage_ms"] for r in result["renders"].values())
    out = args.out or os.path.join(ROOT, "profiles", f"{args.tag}_eval_metrics_fused.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=2)
    print(json.dumps({"out": out, "win": result["win"]}))


if __name__ == "__main__":
    main()
