"""The per-pixel camera-pose gradient of a splat frame (splat.pose_gradient_camera) on the 1 M-splat synthetic
scene of bench.py, at 200 x 200 and at 1080p, in both rasterize modes.

No earlier path exists to race (torch autograd over a rasteriser would need one backward pass per pixel), so this is a recorded
measurement, not a comparison.  Per cell, medians over --reps repetitions after --warmup, the pose moving along bench.py's
orbit from repetition to repetition:
  tangents_ms   unerf_splat_pose_tangents alone (device events around the call on prepared inputs)
  walk_ms       unerf_splat_pose_grad alone, on the frame's own lists (device events)
  gradient_ms   the whole splat.pose_gradient_camera: wall time between two device synchronisations (projection, shading,
                count, bin-sort, the host read-back of the intersection count, tangents, walk)
  frame_ms      splat.active_splatfacto_outputs on the same scene and poses, the same way, for scale
One JSON -> profiles/<tag>_splat_pose_gradient.json.

    python benchmarks/splat_pose_gradient.py --tag r12
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


def _stats(v):
    v = sorted(v)
    return {"median": round(statistics.median(v), 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--splats", type=int, default=1_000_000)
    ap.add_argument("--sizes", default="200x200,1920x1080")
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from uncertainty_nerf_gs_amd import lib as L, ops, splat, synthetic
    L.build_library()
    L.require_gpu()
    dev = torch.device("cuda:0")
    gp = {k: v.to(dev) for k, v in synthetic.make_splat_tensors(seed=7, N=args.splats).items()}
    n_views = 24
    poses = [synthetic.orbit_c2w(2 * math.pi * i / n_views, radius=2.5, height=0.5) for i in range(n_views)]
    bg = torch.zeros(3, device=dev)
    result = {"device": torch.cuda.get_device_name(0), "splats": args.splats, "reps": args.reps, "warmup": args.warmup,
              "batch": L.SPLAT_POSE_GRAD_BATCH, "cells": []}
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        cam = dict(fx=1111.0 * W / 1920, fy=1111.0 * W / 1920, cx=W / 2, cy=H / 2, H=H, W=W)
        for mode in ("classic", "antialiased"):
            aa = mode == "antialiased"

            def prepared(i):
                """the frame's own projection, colours and lists of pose i (what pose_gradient_camera hands its two kernels)"""
                c2w = poses[i % n_views]
                V = splat.viewmat_from_c2w(c2w)
                logits = gp["opacities"].reshape(-1).contiguous()
                xys, depths, radii, conics, comp, tiles, cov3d, opac = ops.splat_project(
                    gp["means"], gp["scales"], 1.0, gp["quats"], V[:3], cam["fx"], cam["fy"], cam["cx"], cam["cy"], H, W, 16, raw=True,
                    opacity_logits=logits, antialiased=aa)
                cols, _ = ops.splat_shade_inputs(3, gp["means"], c2w[:3, 3], gp["features_dc"], gp["features_rest"], None, 0.0, None,
                                                 comp if aa else None, depths)
                I, _, _, gids, bins = ops.splat_bin_sort(xys, depths, radii, tiles, H, W, 16, want_isect_ids=False, tight=(conics, opac))
                return dict(c2w=c2w, V=V, xys=xys, radii=radii, conics=conics, comp=comp, cov3d=cov3d, opac=opac,
                            cols=cols[:, :3].contiguous(), gids=gids, bins=bins, I=I)

            t = {"tangents_ms": [], "walk_ms": [], "gradient_ms": [], "frame_ms": []}
            isects = []
            for rep in range(-args.warmup, args.reps):
                i = rep % n_views
                p = prepared(i)
                tan = torch.empty(args.splats, L.SPLAT_POSE_Q, 12, device=dev)
                grad = torch.empty(H, W, 3, 4, device=dev)
                times = {
                    "tangents_ms": _event_ms(lambda: ops.splat_pose_tangents(gp["means"], p["cov3d"], p["radii"], p["V"][:3], cam["fx"],
                                                                             cam["fy"], cam["cx"], cam["cy"], H, W, out=tan)),
                    "walk_ms": _event_ms(lambda: ops.splat_pose_grad(p["gids"], p["bins"], p["xys"], p["conics"], p["cols"], p["opac"], tan,
                                                                     H, W, bg, compensation=p["comp"] if aa else None, c2w=p["c2w"],
                                                                     out=grad)),
                    "gradient_ms": _wall_ms(lambda: splat.pose_gradient_camera(gp, p["c2w"], background=bg, rasterize_mode=mode, **cam)),
                    "frame_ms": _wall_ms(lambda: splat.active_splatfacto_outputs(gp, p["c2w"], background=bg, rasterize_mode=mode, **cam)),
                }
                if rep >= 0:
                    for k, v in times.items():
                        t[k].append(v)
                    isects.append(int(p["I"]))
            cell = {"H": H, "W": W, "mode": mode, "intersections_median": int(statistics.median(isects)),
                    **{k: _stats(v) for k, v in t.items()}}
            result["cells"].append(cell)
            print(json.dumps(cell), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", f"{args.tag}_splat_pose_gradient.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({"out": out, "cells": len(result["cells"])}))


if __name__ == "__main__":
    main()
