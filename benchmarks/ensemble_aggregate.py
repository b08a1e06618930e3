"""The aggregation tail of an ensemble view batch: B views of M member outputs reduced by a loop of B ensemble.aggregate calls
(per member key a torch.stack copy, one unerf_moments launch and the torch kernels of the key loop) against ONE
ensemble.aggregate_batch call (one unerf_ensemble_reduce launch that reads the members' tensors where they lie).

Synthetic member outputs, no renders.  Cells: B in --views, square frames of --sizes (and 1920 x 1080 at B = 1), M = --members,
two key sets --
  plain   rgb [3], depth, expected_depth, accumulation [1]: contiguous tensors
  active  the active-nerfacto keys: rgb, accumulation, depth, expected_depth, rgb_var, depth_var as channel slices of one
          [H W, 8] row block per member (as render._unpack hands them out), rgb_std and depth_std contiguous
Both ways run in this process on the same device tensors, each warmed up, alternated repetition by repetition in the order
loop, batch, loop: the loop is measured TWICE so that its own spread stands next to the ratio.  Per repetition the device is
synchronised in front and behind and the wall time taken (the host's launch work is what the loop pays); the median over
--reps is recorded, and the device work alone is timed with HIP events around the calls.  ratio = loop / batch (above 1: the
batch is faster); a cell whose batch is slower than the loop by more than the loop's own spread is marked "loss".
Launches per batch are counted by the profiler on one call of each way (--no-launch-count leaves them out).
One JSON -> profiles/<tag>_ensemble_aggregate.json.

    python benchmarks/ensemble_aggregate.py --tag r9
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


def _launches(fn):
    """device kernels of one call, counted by the profiler"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower())


def _members(form, M, B, H, W, dev, gen):
    """[member][view] output dicts"""
    P = H * W
    r = lambda *shape: torch.rand(*shape, device=dev, generator=gen)
    out = []
    for _ in range(M):
        views = []
        for _ in range(B):
            if form == "plain":
                views.append({"rgb": r(H, W, 3), "depth": 4 * r(H, W, 1), "expected_depth": 4 * r(H, W, 1), "accumulation": r(H, W, 1)})
            else:
                rows = r(P, 8)
                img = lambda a, b: rows[:, a:b].reshape(H, W, b - a)
                views.append({"rgb": img(0, 3), "accumulation": img(3, 4), "depth": img(4, 5), "expected_depth": img(5, 6),
                              "rgb_var": img(6, 7), "rgb_std": r(H, W, 1), "depth_var": img(7, 8), "depth_std": r(H, W, 1)})
        out.append(views)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--views", default="1,4,16")
    ap.add_argument("--sizes", default="100,200,400,800")
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-1080p", action="store_true")
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from uncertainty_nerf_gs_amd import ensemble, lib as L
    L.build_library()
    L.require_gpu()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    M = args.members
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "members": M, "cells": []}
    shapes = [(int(s), int(s), int(b)) for s in args.sizes.split(",") if s for b in args.views.split(",")]
    if not args.no_1080p:
        shapes.append((1080, 1920, 1))
    for H, W, B in shapes:
        for form in ("plain", "active"):
            members = _members(form, M, B, H, W, dev, gen)

            def loop():
                return [ensemble.aggregate([pm[v] for pm in members]) for v in range(B)]

            def batch():
                return ensemble.aggregate_batch(members)

            a, b = loop(), batch()
            plan = ensemble.reduce_plan(list(members[0][0]))
            means_equal = all(torch.equal(a[v][n], b[v][n]) for v in range(B) for n, s, _ in plan if s == "mean")
            derived = max([float(((a[v][n] - b[v][n]).abs() / a[v][n].abs()).max()) for v in range(B) for n, s, _ in plan if s != "mean"])
            cell = {"form": form, "H": H, "W": W, "B": B, "M": M, "means_bit_equal": means_equal,
                    "derived_max_rel_diff": derived,
                    "wall": _alternate(loop, batch, args.reps, args.warmup, _wall_ms),
                    "device_events": _alternate(loop, batch, args.reps, args.warmup, _event_ms)}
            cell["loop_ms_per_view"] = round(cell["wall"]["loop_ms"] / B, 4)
            cell["batch_ms_per_view"] = round(cell["wall"]["batch_ms"] / B, 4)
            if not args.no_launch_count:
                cell["loop_launches_per_batch"], cell["batch_launches_per_batch"] = _launches(loop), _launches(batch)
            result["cells"].append(cell)
            print(json.dumps(cell), flush=True)
            del members, a, b
    result["losses"] = sum(c["wall"]["loss"] for c in result["cells"])
    out = args.out or os.path.join(ROOT, "profiles", f"{args.tag}_ensemble_aggregate.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({"out": out, "cells": len(result["cells"]), "losses": result["losses"]}))


if __name__ == "__main__":
    main()
