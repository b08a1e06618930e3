"""The per-pixel pose Jacobian of a splat frame's five channels and its pose variance (splat.pose_jacobian_camera, DESIGN.md
4.6b) on the 1 M-splat synthetic scene of bench.py, at 200 x 200 and at 1080p, in both rasterize modes.

Cells (per size and mode), medians over --reps repetitions after --warmup, the pose moving along bench.py's orbit:
  se3        the Jacobian of all five channels in the six pose parameters (P = 6; out_proj + out_val)
  c2w        the Jacobian in the twelve entries of camera_to_worlds (P = 12; out_proj + out_val)
  variance   the variance only, under a full-rank [6,6] pose covariance (P = 6; out_var + out_val)
each split into
  tangents_ms   unerf_splat_pose_tangents alone (device events around the call on prepared inputs)
  contract_ms   unerf_splat_pose_tangents_proj alone
  walk_ms       unerf_splat_pose_jacobian alone, on the frame's own lists
  camera_ms     the whole splat.pose_jacobian_camera: wall time between two device synchronisations
and, alongside, in the same process on the same poses:
  grad_walk_ms / grad_walk_again_ms   the unchanged unerf_splat_pose_grad walk timed twice (the second run is the spread)
  gradient_ms / gradient_again_ms     the whole splat.pose_gradient_camera, twice
  frame_ms                            splat.active_splatfacto_outputs
  walk_vs_grad_walk                   median walk_ms / median grad_walk_ms per cell: the expectation from the operation count is
                                      <= 1 for se3 (30 running tangents against the gradient walk's 48)
No speed is a pass condition.  One JSON -> profiles/<tag>_splat_pose_jacobian.json.

    python benchmarks/splat_pose_jacobian.py --tag r20
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
    from uncertainty_nerf_gs_amd import lib as L, ops, posegrad, splat, synthetic
    L.build_library()
    L.require_gpu()
    dev = torch.device("cuda:0")
    gp = {k: v.to(dev) for k, v in synthetic.make_splat_tensors(seed=7, N=args.splats).items()}
    n_views = 24
    poses = [synthetic.orbit_c2w(2 * math.pi * i / n_views, radius=2.5, height=0.5) for i in range(n_views)]
    bg = torch.zeros(3, device=dev)
    g = torch.Generator().manual_seed(3)
    a = torch.randn(6, 6, generator=g, dtype=torch.float64)
    cov = (a @ a.T + 6 * torch.eye(6, dtype=torch.float64)) * 1e-4             # full rank
    result = {"device": torch.cuda.get_device_name(0), "splats": args.splats, "reps": args.reps, "warmup": args.warmup,
              "batch": L.SPLAT_POSE_GRAD_BATCH, "cells": []}
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        cam = dict(fx=1111.0 * W / 1920, fy=1111.0 * W / 1920, cx=W / 2, cy=H / 2, H=H, W=W)
        for mode in ("classic", "antialiased"):
            aa = mode == "antialiased"

            def prepared(i):
                """the frame's own projection, colours and lists of pose i (what pose_jacobian_camera hands its three kernels)"""
                c2w = poses[i % n_views]
                V = splat.viewmat_from_c2w(c2w)
                logits = gp["opacities"].reshape(-1).contiguous()
                xys, depths, radii, conics, comp, tiles, cov3d, opac = ops.splat_project(
                    gp["means"], gp["scales"], 1.0, gp["quats"], V[:3], cam["fx"], cam["fy"], cam["cx"], cam["cy"], H, W, 16, raw=True,
                    opacity_logits=logits, antialiased=aa)
                cols, _ = ops.splat_shade_inputs(3, gp["means"], c2w[:3, 3], gp["features_dc"], gp["features_rest"], None, 0.0, None,
                                                 comp if aa else None, depths)
                I, _, _, gids, bins = ops.splat_bin_sort(xys, depths, radii, tiles, H, W, 16, want_isect_ids=False, tight=(conics, opac))
                return dict(c2w=c2w, V=V, xys=xys, depths=depths, radii=radii, conics=conics, comp=comp, cov3d=cov3d, opac=opac,
                            cols=cols[:, :3].contiguous(), gids=gids, bins=bins, I=I)

            kinds = {"se3": dict(proj=lambda c: posegrad.pose_projection(c, None), want=("proj", "val")),
                     "c2w": dict(proj=lambda c: None, want=("proj", "val")),
                     "variance": dict(proj=lambda c: posegrad.pose_projection(c, cov), want=("var", "val"))}
            shared = {k: [] for k in ("tangents_ms", "grad_walk_ms", "grad_walk_again_ms", "gradient_ms", "gradient_again_ms", "frame_ms")}
            t = {kind: {k: [] for k in ("contract_ms", "walk_ms", "camera_ms")} for kind in kinds}
            isects = []
            tan = torch.empty(args.splats, L.SPLAT_POSE_Q, 12, device=dev)
            grad = torch.empty(H, W, 3, 4, device=dev)
            for rep in range(-args.warmup, args.reps):
                p = prepared(rep % n_views)
                comp = p["comp"] if aa else None
                grad_walk = lambda: ops.splat_pose_grad(p["gids"], p["bins"], p["xys"], p["conics"], p["cols"], p["opac"], tan, H, W, bg,
                                                        compensation=comp, c2w=p["c2w"], out=grad)
                gradient = lambda: splat.pose_gradient_camera(gp, p["c2w"], background=bg, rasterize_mode=mode, **cam)
                times = {"tangents_ms": _event_ms(lambda: ops.splat_pose_tangents(gp["means"], p["cov3d"], p["radii"], p["V"][:3], cam["fx"],
                                                                                  cam["fy"], cam["cx"], cam["cy"], H, W, out=tan)),
                         "grad_walk_ms": _event_ms(grad_walk)}
                mine = {}
                for kind, spec in kinds.items():
                    pj = spec["proj"](p["c2w"])
                    M = posegrad.viewmat_jacobian(p["c2w"])
                    M = (M if pj is None else M @ pj).to(torch.float32)
                    P = M.shape[1]
                    ptan = torch.empty(args.splats, L.SPLAT_POSE_PROJ_ROWS, L.splat_pose_pw(P), device=dev)
                    shapes = {"proj": (H, W, 5, P), "var": (H, W, 5), "val": (H, W, 5)}
                    outs = {k: torch.empty(*shapes[k], device=dev) for k in spec["want"]}
                    mine[kind] = {
                        "contract_ms": _event_ms(lambda: ops.splat_pose_tangents_proj(tan, gp["means"], p["radii"], M, out=ptan)),
                        "walk_ms": _event_ms(lambda: ops.splat_pose_jacobian(p["gids"], p["bins"], p["xys"], p["conics"], p["cols"],
                                                                             p["depths"], p["opac"], ptan, P, H, W, bg, compensation=comp,
                                                                             want=spec["want"], out=outs)),
                        "camera_ms": _wall_ms(lambda: splat.pose_jacobian_camera(gp, p["c2w"], background=bg, proj=pj, want=spec["want"],
                                                                                 rasterize_mode=mode, **cam))}
                    del ptan, outs
                times["gradient_ms"] = _wall_ms(gradient)
                times["frame_ms"] = _wall_ms(lambda: splat.active_splatfacto_outputs(gp, p["c2w"], background=bg, rasterize_mode=mode, **cam))
                times["grad_walk_again_ms"] = _event_ms(grad_walk)
                times["gradient_again_ms"] = _wall_ms(gradient)
                if rep >= 0:
                    for k, v in times.items():
                        shared[k].append(v)
                    for kind in kinds:
                        for k, v in mine[kind].items():
                            t[kind][k].append(v)
                    isects.append(int(p["I"]))
            cell = {"H": H, "W": W, "mode": mode, "intersections_median": int(statistics.median(isects)),
                    **{k: _stats(v) for k, v in shared.items()}}
            ref = cell["grad_walk_ms"]["median"]
            for kind in kinds:
                cell[kind] = {k: _stats(v) for k, v in t[kind].items()}
                cell[kind]["walk_vs_grad_walk"] = round(cell[kind]["walk_ms"]["median"] / ref, 3)
            cell["grad_walk_again_vs_grad_walk"] = round(cell["grad_walk_again_ms"]["median"] / ref, 3)
            result["cells"].append(cell)
            print(json.dumps(cell), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", f"{args.tag}_splat_pose_jacobian.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({"out": out, "cells": len(result["cells"])}))


if __name__ == "__main__":
    main()
