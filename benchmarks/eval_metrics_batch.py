"""The metric stage behind a view batch of the eval harness: B images scored by a loop of B unerf_image_metrics calls
(B copies of a row to the host) against ONE unerf_image_metrics_batch call (one copy of B rows).

Entry-point cells: B in --images, square frames of --sizes, two forms --
  rgb    C = 3, all flags (AUSE, AUCE, NLL, SSIM), clip 1.0, no mask      (eval.image_metrics_unc)
  depth  C = 1, a mask that leaves out ~10 % of the pixels, no SSIM       (eval.depth_metrics_unc)
Both ways run in this process on the same device tensors, each warmed up, alternated repetition by repetition in the order
loop, batch, loop: the loop is measured TWICE so that its own spread stands next to the ratio.  Per repetition the device
is synchronised in front and behind and the wall time taken (launch work and the copies to the host count: they are what
the harness pays); the median over --reps is recorded.  The device work alone is timed with HIP events around the calls
without the copies.  ratio = loop / batch (above 1: the batch is faster); a cell whose batch is slower than the loop by
more than the loop's own spread is marked "loss".

Whole-harness cells: eval.get_average_uncertainty_metrics(fused=True, view_batch=16, metric_batch=False | True) on 16
active-nerfacto cameras of the synthetic scene of benchmarks/nerf_view_batch.py at --harness-sizes: wall time per image,
same alternation.  One JSON -> profiles/<tag>_eval_metrics_batch.json.

    python benchmarks/eval_metrics_batch.py --tag r8
"""
import argparse
import json
import math
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _alternate(loop, batch, reps, warmup, timer):
    """medians of `timer` over reps of loop, batch, loop -> dict with the ratio and the loop's spread"""
    for _ in range(warmup):
        loop(), batch()
    t = {"loop_a": [], "batch": [], "loop_b": []}
    for _ in range(reps):
        for window, fn in (("loop_a", loop), ("batch", batch), ("loop_b", loop)):
            t[window].append(timer(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    loop_ms = 0.5 * (med["loop_a"] + med["loop_b"])
    spread = abs(med["loop_a"] - med["loop_b"]) / loop_ms
    return {"loop_ms": round(loop_ms, 4), "batch_ms": round(med["batch"], 4), "loop_a_ms": round(med["loop_a"], 4),
            "loop_b_ms": round(med["loop_b"], 4), "ratio_loop_over_batch": round(loop_ms / med["batch"], 4),
            "loop_spread": round(spread, 4), "loss": bool(med["batch"] > loop_ms * (1.0 + spread))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--images", default="1,4,16")
    ap.add_argument("--sizes", default="100,200,400,800")
    ap.add_argument("--harness-sizes", default="200,400")
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from uncertainty_nerf_gs_amd import eval as E, lib as L, ops, render, synthetic
    L.build_library()
    L.require_gpu()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "entry_point": [], "harness": []}

    for size in (int(s) for s in args.sizes.split(",")):
        H = W = size
        for B in (int(b) for b in args.images.split(",")):
            gt = torch.rand(B, H, W, 3, device=dev, generator=gen)
            std = 0.02 + 0.2 * torch.rand(B, H, W, device=dev, generator=gen)
            pred = gt + std[..., None] * torch.randn(B, H, W, 3, device=dev, generator=gen)
            mask = torch.rand(B, H, W, device=dev, generator=gen) > 0.1
            forms = {
                "rgb": (pred, gt, std, None, dict(image_hw=(H, W), clip_max=1.0, nll_min_sigma=3e-2, flags=L.METRICS_ALL)),
                "depth": (pred[..., :1].contiguous(), gt[..., :1].contiguous(), std, mask,
                          dict(nll_min_sigma=1.0, flags=L.METRICS_ALL & ~L.METRICS_SSIM)),
            }
            for form, (p, t, s, m, kw) in forms.items():
                ws_loop, ws_batch = ops.Workspace(), ops.Workspace()

                def loop_dev():
                    return [ops.image_metrics(p[b], t[b], s[b], None if m is None else m[b], workspace=ws_loop, **kw) for b in range(B)]

                def batch_dev():
                    return ops.image_metrics_batch(p, t, s, m, workspace=ws_batch, **kw)

                def loop():                 # as the harness scores per image: a blocking copy behind every call
                    return [ops.image_metrics(p[b], t[b], s[b], None if m is None else m[b], workspace=ws_loop, **kw).cpu()
                            for b in range(B)]

                def batch():
                    return batch_dev().cpu()

                same = torch.equal(torch.stack(loop()).view(torch.int64), batch().view(torch.int64))
                cell = {"form": form, "H": H, "W": W, "B": B, "rows_bit_equal": same,
                        "wall": _alternate(loop, batch, args.reps, args.warmup, _wall_ms),
                        "device_events": _alternate(loop_dev, batch_dev, args.reps, args.warmup, _event_ms)}
                result["entry_point"].append(cell)
                print(json.dumps(cell), flush=True)

    V = args.views
    scene = synthetic.scene_to_device(synthetic.make_scene_tensors(seed=0, kind="active"), dev)
    poses = [synthetic.orbit_c2w(0.25 + 2 * math.pi * v / V) for v in range(V)]
    for size in (int(s) for s in args.harness_sizes.split(",") if s):
        H = W = size
        f = 1111.0 * W / 1920
        cams = [SimpleNamespace(camera_to_worlds=c2w, fx=f, fy=f, cx=W / 2, cy=H / 2, height=H, width=W) for c2w in poses]
        one = lambda cam: render.render_camera(scene, cam.camera_to_worlds, cam.fx, cam.fy, cam.cx, cam.cy, H, W)
        many = lambda b: render.render_cameras(scene, b.camera_to_worlds, float(b.fx[0]), float(b.fy[0]), float(b.cx[0]), float(b.cy[0]),
                                               H, W)
        gts = [torch.clamp(o["rgb"] + 0.05 * torch.randn(H, W, 3, device=dev, generator=gen), 0, 1) for o in many(E.stack_cameras(cams))]
        eval_set = list(zip(cams, gts))
        got = {}

        def harness(mb):
            got[mb] = E.get_average_uncertainty_metrics(one, eval_set, fused=True, view_batch=V, get_outputs_for_cameras=many,
                                                        metric_batch=mb)[0]

        cell = {"method": "active-nerfacto", "H": H, "W": W, "views": V,
                "wall_per_batch": _alternate(lambda: harness(False), lambda: harness(True), args.reps, args.warmup, _wall_ms)}
        cell["loop_ms_per_image"] = round(cell["wall_per_batch"]["loop_ms"] / V, 4)
        cell["batch_ms_per_image"] = round(cell["wall_per_batch"]["batch_ms"] / V, 4)
        timing = ("num_rays_per_sec", "fps", "render_rays_per_sec")
        cell["metrics_equal"] = all(got[True][k] == got[False][k] for k in got[True] if k not in timing)
        result["harness"].append(cell)
        print(json.dumps(cell), flush=True)

    cells = [c["wall"] for c in result["entry_point"]] + [c["wall_per_batch"] for c in result["harness"]]
    result["losses"] = sum(c["loss"] for c in cells)
    out = args.out or os.path.join(ROOT, "profiles", f"{args.tag}_eval_metrics_batch.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({"out": out, "cells": len(cells), "losses": result["losses"]}))


if __name__ == "__main__":
    main()
