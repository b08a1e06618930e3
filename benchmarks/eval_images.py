"""The rendered images of the eval harness (eval.save_imgs_rgb): the host route -- four float32 images per eval image
copied to the host (32 B per pixel), normalised, colour-mapped and quantised in numpy (eval.pack_eval_images) -- against
the fused route -- ONE unerf_eval_images_batch call per view batch and one copy of the final bytes (10 B per pixel).

Cells: B in --images at square frames of --sizes, and B = 1 at 1080 x 1920.  Both routes run in this process on the same
device tensors, each warmed up, alternated repetition by repetition in the order host, fused, host: the host route is
measured TWICE so that its own spread stands next to the ratio.  Per repetition the device is synchronised in front and
behind and the wall time taken; the median over the repetitions is recorded, per image.  Two windows per cell:
  pack    save_imgs_rgb(encode=False): everything up to the uint8 arrays on the host
  files   save_imgs_rgb(encode=True): the same plus the PNG encoding (zlib) and the writes, into a temporary directory
          (--file-reps repetitions: zlib dominates and is the same work on both routes)
and, with HIP events, the device time of the ops.eval_images call alone (no copy).  ratio = host / fused (above 1: the
fused route is faster); a cell whose fused route is slower than the host route by more than the host route's own spread
is marked "loss".  Launches per batch are those of the entry point: two kernels and two memsets per call, whatever B is.
The inputs are smooth images with noise on top, so that zlib sees something like a render.
One JSON -> profiles/<tag>_eval_images.json.

    python benchmarks/eval_images.py --tag r9
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
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


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _alternate(host, fused, reps, warmup, B):
    """medians of the wall time over reps of host, fused, host, per image -> dict with the ratio and the host's spread"""
    for _ in range(warmup):
        host(), fused()
    t = {"host_a": [], "fused": [], "host_b": []}
    for _ in range(reps):
        for window, fn in (("host_a", host), ("fused", fused), ("host_b", host)):
            t[window].append(_wall_ms(fn) / B)
    med = {k: statistics.median(v) for k, v in t.items()}
    host_ms = 0.5 * (med["host_a"] + med["host_b"])
    spread = abs(med["host_a"] - med["host_b"]) / host_ms
    return {"host_ms_per_image": round(host_ms, 4), "fused_ms_per_image": round(med["fused"], 4),
            "host_a_ms_per_image": round(med["host_a"], 4), "host_b_ms_per_image": round(med["host_b"], 4),
            "ratio_host_over_fused": round(host_ms / med["fused"], 4), "host_spread": round(spread, 4),
            "loss": bool(med["fused"] > host_ms * (1.0 + spread))}


def _images(B, H, W, dev, gen):
    """smooth ground truth + noisy prediction + a std that follows the noise: [(outputs, gt)] * B on the device"""
    y = torch.linspace(0, 1, H, device=dev)[:, None, None]
    x = torch.linspace(0, 1, W, device=dev)[None, :, None]
    items = []
    for b in range(B):
        phase = torch.tensor([0.0, 2.1, 4.2], device=dev) + 0.37 * b
        gt = 0.5 + 0.45 * torch.sin(6.0 * x + 4.0 * y + phase) * torch.cos(3.0 * y - 2.0 * x)
        std = 0.01 + 0.15 * (0.5 + 0.5 * torch.sin(9.0 * x[..., 0] * y[..., 0] + b)) * torch.rand(H, W, device=dev, generator=gen)
        rgb = gt + std[..., None] * torch.randn(H, W, 3, device=dev, generator=gen)
        items.append(({"rgb": rgb.contiguous(), "rgb_std": std[..., None].contiguous()}, gt.contiguous()))
    return items


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--images", default="1,4,16")
    ap.add_argument("--sizes", default="100,200,400,800")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--file-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-1080p", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from uncertainty_nerf_gs_amd import eval as E, lib as L, ops
    L.build_library()
    L.require_gpu()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    unc = (0.0, 0.2)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "file_reps": args.file_reps,
              "bytes_per_pixel_to_host": {"host": 32, "fused": 10}, "launches_per_batch": {"kernels": 2, "memsets": 2}, "cells": []}
    shapes = [(int(s), int(s), int(b)) for s in args.sizes.split(",") if s for b in args.images.split(",")]
    if not args.no_1080p:
        shapes.append((1080, 1920, 1))
    for H, W, B in shapes:
        items = _images(B, H, W, dev, gen)
        outs, gts, ids = [o for o, _ in items], [g for _, g in items], list(range(B))
        stack = [torch.stack(x) for x in ([o["rgb"] for o in outs], gts, [o["rgb_std"][..., 0] for o in outs])]
        with tempfile.TemporaryDirectory() as tmp:
            run = lambda fused, encode: E.save_imgs_rgb(ids, outs, gts, os.path.join(tmp, "fused" if fused else "host"), *unc,
                                                        fused=fused, encode=encode)
            a, b = run(False, False), run(True, False)
            same = all(np.array_equal(a[i][k], b[i][k]) for i in ids for k in ops.EVAL_IMAGE_PLANES)
            cell = {"H": H, "W": W, "B": B, "bytes_equal": same,
                    "pack": _alternate(lambda: run(False, False), lambda: run(True, False), args.reps, args.warmup, B),
                    "files": _alternate(lambda: run(False, True), lambda: run(True, True), args.file_reps, 1, B)}
            dev_ms = [_event_ms(lambda: ops.eval_images(*stack, *unc)) for _ in range(args.warmup + args.reps)][args.warmup:]
            cell["device_call_ms_per_image"] = round(statistics.median(dev_ms) / B, 5)
        result["cells"].append(cell)
        print(json.dumps(cell), flush=True)
    result["losses"] = sum(c[w]["loss"] for c in result["cells"] for w in ("pack", "files"))
    result["all_bytes_equal"] = all(c["bytes_equal"] for c in result["cells"])
    out = args.out or os.path.join(ROOT, "profiles", f"{args.tag}_eval_images.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({"out": out, "cells": len(result["cells"]), "losses": result["losses"], "all_bytes_equal": result["all_bytes_equal"]}))


if __name__ == "__main__":
    main()
