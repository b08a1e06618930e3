"""Several camera views per NeRF render call against a loop of single-view calls, on small frames.

For active-nerfacto and nerfacto-mcdropout (K = 8, precision "f16", the bench headline's arithmetic) -- and, with
--methods laplace, nerfacto-laplace (100 + 100 sampled last-layer rows, a set per 32,768-ray eval chunk, precision "f16x2") --
with full-size tables, and 16 cameras at each of --sizes: the 16 views rendered as a loop of render.render_camera and as ONE render.render_cameras
call, both in this process, each form warmed up, the forms alternated pass by pass in the order loop, batch, loop -- the
loop is measured TWICE so that its own run-to-run spread is on record next to the gain.  Wall time around each 16-view pass
with the device synchronised in front and behind (host launch work counts: it is part of what a frame costs); as many
passes per window as reach --seconds.  Prints one JSON line per (method, size) and writes them all to
profiles/<tag>_nerf_view_batch.json: ms per view and Mrays/s of both forms, the ratio, and the spread of the loop.

    python benchmarks/nerf_view_batch.py [--tag r1] [--sizes 100,200,400,800] [--views 16] [--seconds 1.0]
    python benchmarks/nerf_view_batch.py --profile batch --methods active --sizes 200    # a few passes of one form only,
    python benchmarks/nerf_view_batch.py --profile loop --methods active --sizes 200     # for rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uncertainty_nerf_gs_amd import lib, render, synthetic  # noqa: E402

METHODS = {"active": ("active", {}), "mcdropout": ("mcdropout", dict(K=8, seed=1, p_drop=0.2)), "laplace": ("laplace", {})}


def laplace_scene(tensors, dev, rays_per_view, chunk_rays=1 << 15):
    """per-chunk sample sets as the reference draws them: one set of 100 + 100 rows per eval chunk of a frame (both forms
    render every view with these sets: the loop over this scene is what the batch is compared against)"""
    n_sets = -(-rays_per_view // chunk_rays)
    ws = [synthetic.laplace_weight_samples(tensors, seed=40 + i, n_samples=100) for i in range(n_sets)]
    scene = synthetic.scene_to_device(tensors, dev, ws_density=torch.stack([w[0] for w in ws]).to(dev),
                                      ws_rgb=torch.stack([w[1] for w in ws]).to(dev), lap_chunk_rays=chunk_rays)
    scene.chunk_rays, scene.field.precision = chunk_rays, "f16x2"
    return scene


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--sizes", default="100,200,400,800")
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--methods", default="active,mcdropout")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--profile", choices=("batch", "loop"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib.build_library()
    lib.require_gpu()
    dev = torch.device("cuda:0")
    B = args.views
    poses = torch.stack([synthetic.orbit_c2w(0.25 + 2 * math.pi * v / B) for v in range(B)])      # host-resident
    seeds = tuple(1000 + v for v in range(B))
    rows = []
    for name in args.methods.split(","):
        kind, kw = METHODS[name]
        tensors = synthetic.make_scene_tensors(seed=0, kind=kind)
        scene = None if name == "laplace" else synthetic.scene_to_device(tensors, dev, **kw)
        if name == "mcdropout":
            scene.field.precision = "f16"
        for size in (int(s) for s in args.sizes.split(",")):
            H = W = size
            if name == "laplace":       # the number of sets follows the frame size
                scene = laplace_scene(tensors, dev, H * W)
                assert render.view_batch_loop_reason(scene) is None
            f = 1111.0 * W / 1920
            cam = dict(fx=f, fy=f, cx=W / 2, cy=H / 2, H=H, W=W)
            use_seeds = seeds if name == "mcdropout" else None

            def loop():
                saved = scene.field.seed
                for v in range(B):
                    if use_seeds is not None:
                        scene.field.seed = use_seeds[v]
                    render.render_camera(scene, poses[v], **cam)
                scene.field.seed = saved

            def batch():
                render.render_cameras(scene, poses, cam["fx"], cam["fy"], cam["cx"], cam["cy"], H, W, seeds=use_seeds)

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            if args.profile:
                fn = batch if args.profile == "batch" else loop
                for _ in range(args.warmup + 5):
                    fn()
                torch.cuda.synchronize()
                print(json.dumps({"profile": args.profile, "method": name, "size": size, "passes": args.warmup + 5}), flush=True)
                continue
            est = 0.0
            for _ in range(args.warmup):
                est = max(timed(loop), timed(batch))
            passes = max(3, int(math.ceil(args.seconds / max(est, 1e-4))))
            t = {"loop_a": 0.0, "batch": 0.0, "loop_b": 0.0}
            for _ in range(passes):
                for window, fn in (("loop_a", loop), ("batch", batch), ("loop_b", loop)):
                    t[window] += timed(fn)
            ms = {k: v / (passes * B) * 1e3 for k, v in t.items()}
            loop_ms = 0.5 * (ms["loop_a"] + ms["loop_b"])
            groups = render.plan_view_groups(B, H * W, chunk_rays=scene.chunk_rays)
            row = {"method": name, "H": H, "W": W, "views": B, "passes": passes,
                   "views_per_group": None if groups is None else groups[0][1],
                   "loop_ms_per_view": round(loop_ms, 4), "batch_ms_per_view": round(ms["batch"], 4),
                   "loop_a_ms_per_view": round(ms["loop_a"], 4), "loop_b_ms_per_view": round(ms["loop_b"], 4),
                   "loop_mrays_s": round(H * W / loop_ms / 1e3, 2), "batch_mrays_s": round(H * W / ms["batch"] / 1e3, 2),
                   "ratio_batch_over_loop": round(ms["batch"] / loop_ms, 4),
                   "loop_spread": round(abs(ms["loop_a"] - ms["loop_b"]) / loop_ms, 4)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del scene
        torch.cuda.empty_cache()
    if rows:
        out = args.out or os.path.join(ROOT, "profiles", f"{args.tag}_nerf_view_batch.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "views": B, "seconds_per_window": args.seconds, "rows": rows}, fh,
                      indent=1)


if __name__ == "__main__":
    main()
