"""splat.pose_jacobian_cameras (B views in shared launches) against a loop of the unchanged
splat.pose_jacobian_camera over the same poses, on the 1 M-splat synthetic scene of bench.py and its 24 orbit poses.

Cells: B in {1, 4, 16} x {200 x 200, 400 x 400, 800 x 800, 1920 x 1080} x {classic, antialiased} x
  se3        the Jacobian of all five channels in the six pose parameters (want = proj + val)
  variance   the variance only, under a full-rank [6,6] pose covariance (want = var + val)
Per cell, medians over --reps repetitions after --warmup, every repetition on the next B poses of the orbit, both sides alternated
in one process (loop, batch, loop again), wall time between two device synchronisations divided by B:
  batch_ms_per_view                          splat.pose_jacobian_cameras
  loop_ms_per_view / loop_again_ms_per_view  B calls of splat.pose_jacobian_camera, timed twice: the second is the loop's own spread
  batch_vs_loop, loop_again_vs_loop          ratios of the medians
  slower_than_spread                         batch median > the larger loop median: such a cell must be routed to the loop
                                             (splat.POSE_JACOBIAN_BATCH_LOOP_CELLS)
and the two new kernels alone (device events, on the batch's own prepared inputs), next to B times their single-view counterparts:
  ptangents_batch_ms     unerf_splat_pose_ptangents_batch            tangents_loop_ms   B x (unerf_splat_pose_tangents +
                                                                                        unerf_splat_pose_tangents_proj)
  walk_batch_ms          unerf_splat_pose_jacobian_batch             walk_loop_ms       B x unerf_splat_pose_jacobian
No speed is a pass condition.  One JSON -> profiles/<tag>_splat_pose_jacobian_batch.json.

    python benchmarks/splat_pose_jacobian_batch.py --tag r21
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
    ap.add_argument("--sizes", default="200x200,400x400,800x800,1920x1080")
    ap.add_argument("--views", default="1,4,16")
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from uncertainty_nerf_gs_amd import lib as L, ops, posegrad, splat, synthetic
    L.build_library()
    L.require_gpu()
    dev = torch.device("cuda:0")
    gp = {k: v.to(dev) for k, v in synthetic.make_splat_tensors(seed=7, N=args.splats).items()}
    N = args.splats
    n_views = 24
    poses = [synthetic.orbit_c2w(2 * math.pi * i / n_views, radius=2.5, height=0.5) for i in range(n_views)]
    bg = torch.zeros(3, device=dev)
    g = torch.Generator().manual_seed(3)
    a = torch.randn(6, 6, generator=g, dtype=torch.float64)
    cov = (a @ a.T + 6 * torch.eye(6, dtype=torch.float64)) * 1e-4             # full rank
    kinds = {"se3": (None, ("proj", "val")), "variance": (cov, ("var", "val"))}
    result = {"device": torch.cuda.get_device_name(0), "splats": N, "reps": args.reps, "warmup": args.warmup, "cells": []}
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        cam = dict(fx=1111.0 * W / 1920, fy=1111.0 * W / 1920, cx=W / 2, cy=H / 2, H=H, W=W)
        for mode in ("classic", "antialiased"):
            aa = mode == "antialiased"
            for B in (int(v) for v in args.views.split(",")):
                for kind, (pose_cov, want) in kinds.items():
                    t = {k: [] for k in ("batch", "loop", "loop_again", "ptangents_batch_ms", "tangents_loop_ms", "walk_batch_ms",
                                         "walk_loop_ms")}
                    for rep in range(-args.warmup, args.reps):
                        c2ws = torch.stack([poses[(rep * B + v) % n_views] for v in range(B)])[:, :3, :4]
                        projs = [posegrad.pose_projection(c, pose_cov) for c in c2ws]
                        loop = lambda: [splat.pose_jacobian_camera(gp, c2ws[v], background=bg, proj=projs[v], want=want,
                                                                   rasterize_mode=mode, **cam) for v in range(B)]
                        batch = lambda: splat.pose_jacobian_cameras(gp, c2ws, cam["fx"], cam["fy"], cam["cx"], cam["cy"], H, W, bg,
                                                                    projs=projs, want=want, rasterize_mode=mode)
                        times = {"loop": _wall_ms(loop) / B, "batch": _wall_ms(batch) / B, "loop_again": _wall_ms(loop) / B}
                        # the two new kernels alone, on this batch's own prepared inputs
                        Vs = [splat.viewmat_from_c2w(c) for c in c2ws]
                        views = ops.splat_view_records(Vs, [cam["fx"]] * B, [cam["fy"]] * B, [cam["cx"]] * B, [cam["cy"]] * B,
                                                       [c[:3, 3] for c in c2ws])
                        logits = gp["opacities"].reshape(-1).contiguous()
                        xys, depths, radii, conics, comp, tiles, opac, cov3d = ops.splat_project_batch(
                            gp["means"], gp["scales"], gp["quats"], views, B, H, W, 16, opacity_logits=logits, antialiased=aa,
                            want_cov3d=True)
                        cols, _ = ops.splat_shade_inputs_batch(3, gp["means"], views, B, gp["features_dc"], gp["features_rest"], None, 0.0,
                                                               None, comp if aa else None, depths)
                        count = ops.SplatCountBatch(tiles, radii)
                        totals, _, gids, bins = ops.splat_bin_sort_batch(xys, depths, radii, count, H, W, 16, tight=(conics, opac))
                        Ms = [posegrad.splat_view_projection(c2ws[v], projs[v]) for v in range(B)]
                        P = int(Ms[0].shape[1])
                        PW = L.splat_pose_pw(P)
                        Md = torch.stack(Ms).to(dev)
                        ptan = torch.empty(B, N, L.SPLAT_POSE_PROJ_ROWS, PW, device=dev)
                        tan = torch.empty(N, L.SPLAT_POSE_Q, 12, device=dev)
                        ptan1 = torch.empty(N, L.SPLAT_POSE_PROJ_ROWS, PW, device=dev)
                        shapes = {"proj": (B, H, W, 5, P), "var": (B, H, W, 5), "val": (B, H, W, 5)}
                        outs = {k: torch.empty(*shapes[k], device=dev) for k in want}
                        outs1 = {k: torch.empty(*shapes[k][1:], device=dev) for k in want}
                        cz = comp if aa else None
                        times["ptangents_batch_ms"] = _event_ms(lambda: ops.splat_pose_ptangents_batch(gp["means"], cov3d, radii, views, B,
                                                                                                       Md, H, W, out=ptan))

                        def tangents_loop():
                            for v in range(B):
                                ops.splat_pose_tangents(gp["means"], cov3d[v], radii[v], Vs[v][:3], cam["fx"], cam["fy"], cam["cx"], cam["cy"],
                                                        H, W, out=tan)
                                ops.splat_pose_tangents_proj(tan, gp["means"], radii[v], Ms[v], out=ptan1)

                        times["tangents_loop_ms"] = _event_ms(tangents_loop)
                        times["walk_batch_ms"] = _event_ms(lambda: ops.splat_pose_jacobian_batch(
                            gids, bins, xys, conics, cols, depths, opac, ptan, P, H, W, bg, compensation=cz, want=want, out=outs))
                        # each view's own lists: its segment of the ids, relative to its own arrays
                        offs = [sum(totals[:v]) for v in range(B)]
                        own = [((gids[offs[v]:offs[v] + totals[v]] - v * N).contiguous() if totals[v] else gids[:0],
                                (bins[v] - offs[v]).contiguous(), cols[v, :, :3].contiguous()) for v in range(B)]

                        def walk_loop():
                            for v in range(B):
                                ops.splat_pose_jacobian(own[v][0], own[v][1], xys[v], conics[v], own[v][2], depths[v], opac[v], ptan[v], P,
                                                        H, W, bg, compensation=None if cz is None else cz[v], want=want, out=outs1)

                        times["walk_loop_ms"] = _event_ms(walk_loop)
                        del ptan, tan, ptan1, outs, outs1, own
                        if rep >= 0:
                            for k, v in times.items():
                                t[k].append(v)
                    cell = {"H": H, "W": W, "mode": mode, "B": B, "kind": kind, "intersections_per_view": int(sum(totals) / B),
                            "batch_ms_per_view": _stats(t["batch"]), "loop_ms_per_view": _stats(t["loop"]),
                            "loop_again_ms_per_view": _stats(t["loop_again"]),
                            **{k: _stats(t[k]) for k in ("ptangents_batch_ms", "tangents_loop_ms", "walk_batch_ms", "walk_loop_ms")}}
                    lo = cell["loop_ms_per_view"]["median"]
                    cell["batch_vs_loop"] = round(cell["batch_ms_per_view"]["median"] / lo, 3)
                    cell["loop_again_vs_loop"] = round(cell["loop_again_ms_per_view"]["median"] / lo, 3)
                    cell["slower_than_spread"] = cell["batch_ms_per_view"]["median"] > max(lo, cell["loop_again_ms_per_view"]["median"])
                    cell["ptangents_batch_vs_loop"] = round(cell["ptangents_batch_ms"]["median"] / cell["tangents_loop_ms"]["median"], 3)
                    cell["walk_batch_vs_loop"] = round(cell["walk_batch_ms"]["median"] / cell["walk_loop_ms"]["median"], 3)
                    result["cells"].append(cell)
                    print(json.dumps(cell), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", f"{args.tag}_splat_pose_jacobian_batch.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({"out": out, "cells": len(result["cells"]),
                      "slower_than_spread": [[c["H"], c["W"], c["mode"], c["B"], c["kind"]] for c in result["cells"] if c["slower_than_spread"]]}))


if __name__ == "__main__":
    main()
