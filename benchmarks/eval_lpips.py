"""LPIPS per eval image: the HIP kernels behind ops.lpips_batch against the host definition metrics.lpips (torch's own
convolutions) on the same device, and against metrics.lpips on the CPU.

Cells: B in --images at square frames of --sizes, and B = 1 at 1080 x 1920.  Synthetic weights (synthetic.make_lpips_weights:
no pretrained network exists offline; the arithmetic does not depend on the values), uniform random images in [0, 1].
Both device routes run in this process on the same tensors, each warmed up, alternated repetition by repetition in the
order torch, kernels, torch: the torch route is measured TWICE so that its own spread stands next to the ratio.  Per
repetition the device is synchronised in front and behind and the wall time taken, the copy of the result to the host
included (it is what the harness pays); the median over --reps is recorded, as ms per image.  The CPU route is run --cpu-reps
times per cell (median), up to --cpu-max-pixels pixels per call.  ratio = torch / kernels (above 1: the kernels are
faster).  There is no gate: a cell where torch's convolutions win is recorded like any other ("loss": true when the
kernels are slower by more than torch's own spread).  One JSON -> profiles/<tag>_eval_lpips.json.

    python benchmarks/eval_lpips.py --tag r11
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--images", default="1,4,16")
    ap.add_argument("--sizes", default="100,200,400,800")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--cpu-max-pixels", type=int, default=4 * 800 * 800)
    ap.add_argument("--no-1080p", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from uncertainty_nerf_gs_amd import checkpoints, lib as L, metrics as M, ops, synthetic
    L.build_library()
    L.require_gpu()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    weights = checkpoints.lpips_weights_from_state_dict(synthetic.make_lpips_weights(0))
    shapes = [(int(s), int(s), int(b)) for s in args.sizes.split(",") if s for b in args.images.split(",")]
    if not args.no_1080p:
        shapes.append((1080, 1920, 1))
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "cells": []}
    for H, W, B in shapes:
        target = torch.rand(B, H, W, 3, device=dev, generator=gen)
        pred = torch.clamp(target + 0.1 * torch.randn(B, H, W, 3, device=dev, generator=gen), 0, 1)
        arena = ops.Workspace()
        out = {}

        def kernels():
            out["kernels"] = [M.finish_lpips(r) for r in ops.lpips_batch(pred, target, weights, workspace=arena).cpu().numpy()]

        def torch_route():
            out["torch"] = M.lpips_per_image(pred, target, weights).cpu().tolist()

        for _ in range(args.warmup):
            torch_route(), kernels()
        t = {"torch_a": [], "kernels": [], "torch_b": []}
        for _ in range(args.reps):
            for window, fn in (("torch_a", torch_route), ("kernels", kernels), ("torch_b", torch_route)):
                t[window].append(_wall_ms(fn))
        med = {k: statistics.median(v) for k, v in t.items()}
        torch_ms = 0.5 * (med["torch_a"] + med["torch_b"])
        spread = abs(med["torch_a"] - med["torch_b"]) / torch_ms
        cell = {"H": H, "W": W, "B": B, "kernels_ms_per_image": round(med["kernels"] / B, 4),
                "torch_ms_per_image": round(torch_ms / B, 4), "torch_a_ms_per_image": round(med["torch_a"] / B, 4),
                "torch_b_ms_per_image": round(med["torch_b"] / B, 4), "torch_spread": round(spread, 4),
                "ratio_torch_over_kernels": round(torch_ms / med["kernels"], 4),
                "loss": bool(med["kernels"] > torch_ms * (1.0 + spread)),
                "max_abs_diff_kernels_torch": max(abs(a - b) for a, b in zip(out["kernels"], out["torch"])),
                "workspace_mib": round(arena.nbytes() / 2 ** 20, 1)}
        if B * H * W <= args.cpu_max_pixels:
            pc, tc = pred.cpu(), target.cpu()
            cpu = []
            for _ in range(args.cpu_reps):
                t0 = time.perf_counter()
                M.lpips_per_image(pc, tc, weights)
                cpu.append((time.perf_counter() - t0) * 1e3)
            cell["cpu_ms_per_image"] = round(statistics.median(cpu) / B, 4)
        arena.release()
        result["cells"].append(cell)
        print(json.dumps(cell), flush=True)
    result["losses"] = sum(c["loss"] for c in result["cells"])
    path = args.out or os.path.join(ROOT, "profiles", f"{args.tag}_eval_lpips.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({"out": path, "cells": len(result["cells"]), "losses": result["losses"]}))


if __name__ == "__main__":
    main()
