"""Per-pixel pose gradients of a Laplace frame under a named draw of the last layers (render.pose_gradient_camera_laplace: ray
kernel -> proposal sampler -> unerf_pose_grad_laplace, one launch per group of rays whatever the row counts are) on the
full-table synthetic Laplace scene (log2T = 19, max_res = 2048, S = 48, 100 + 100 sampled rows, a set per 32,768-ray chunk), at
200 x 200 and 1920 x 1080, and again with 1 + 1 rows.

Per frame size and row count: wall ms per frame (median over --reps, device synchronised in front and behind), and on the
frame's own rays and bins (made once, outside the timed region) the gradient launches alone.  In the same process the unchanged
single-head unerf_pose_grad on the nerfacto scene of the same tables is timed TWICE, once as the comparison and once for its
own spread, and the Laplace frame itself (render.render_camera, split-f16) once.
Expectation from the operation count at 100 + 100 rows: about 26 k FMA per sample for the head means, 45 k for their adjoints
with recomputation and 12 k for everything else, 3.6 x pose_grad_kernel's count (the kernel as built walks the colour rows a
second time only for rays behind a closed clamp gate: 2.8 x on this scene).  A recorded measurement, not a gate.
One JSON -> profiles/<tag>_pose_gradient_laplace.json.

    python benchmarks/pose_gradient_laplace.py --tag r16
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

CHUNK = 1 << 15
EXPECTED_OVER_SINGLE_HEAD = 3.6


def _timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", default="lego200,1080p")
    ap.add_argument("--rows", default="100,1")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from uncertainty_nerf_gs_amd import lib as L, ops, render, synthetic
    L.build_library()
    L.require_gpu()
    dev = torch.device("cuda:0")
    cams = {"lego200": synthetic.CAMERA_LEGO200, "1080p": synthetic.CAMERA_1080P}
    names = [f for f in args.frames.split(",") if f]
    sets = max(-(-(cams[n]["H"] * cams[n]["W"]) // CHUNK) for n in names)
    t = synthetic.make_scene_tensors(seed=0, kind="laplace")
    plain = synthetic.scene_to_device(synthetic.make_scene_tensors(seed=0, kind="active"), dev)     # the same tables, one head
    c2w = synthetic.orbit_c2w(0.3)
    rot_inv = torch.linalg.inv(c2w[:3, :3].double()).float()
    rpl = 1 << 20
    med = lambda v: round(statistics.median(v), 3)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
              "scene": f"laplace, log2T 19, max_res 2048, S 48, a sample set per {CHUNK}-ray chunk",
              "expected_over_single_head_from_operation_count": EXPECTED_OVER_SINGLE_HEAD, "frames": []}
    with torch.cuda.device(dev):
        for n in [int(v) for v in args.rows.split(",") if v]:
            rows = [synthetic.laplace_weight_samples(t, seed=42 + k, n_samples=n) for k in range(sets)]
            scene = synthetic.scene_to_device(t, dev, ws_density=torch.stack([r[0] for r in rows]),
                                              ws_rgb=torch.stack([r[1] for r in rows]), lap_chunk_rays=CHUNK)
            kw = dict(rot_inv=rot_inv, spacing=scene.spacing, background=scene.background)
            for name in names:
                cam = cams[name]
                H, W = cam["H"], cam["W"]
                rays = H * W
                groups, plain_groups = [], []      # the frame's rays and bins, as the frame-level entry points make them
                for start in range(0, rays, rpl):
                    o, d, _ = ops.generate_rays(c2w, cam["fx"], cam["fy"], cam["cx"], cam["cy"], H, W, dev, start, min(rpl, rays - start))
                    sb, _ = render.sample_rays(scene, o, d, None, start, want_prop_depth=False, image_width=W)
                    groups.append((start, o, d, sb.clone()))
                    sb, _ = render.sample_rays(plain, o, d, None, start, want_prop_depth=False, image_width=W)
                    plain_groups.append((o, d, sb.clone()))

                def lap():
                    for start, o, d, sb in groups:
                        ops.pose_grad_laplace(o, d, sb, scene.field, scene.near, scene.far, ray_offset=start, **kw)

                def single():
                    for o, d, sb in plain_groups:
                        ops.pose_grad(o, d, sb, plain.field, plain.near, plain.far, rot_inv=rot_inv, spacing=plain.spacing,
                                      background=plain.background)

                frame = _timed(lambda: render.pose_gradient_camera_laplace(scene, c2w, **cam), args.reps)
                t_lap = _timed(lap, args.reps)
                t_a = _timed(single, args.reps)
                t_b = _timed(single, args.reps)
                t_render = _timed(lambda: render.render_camera(scene, c2w, **cam), args.reps)
                g = render.pose_gradient_camera_laplace(scene, c2w, **cam)
                ratio = statistics.median(t_lap) / min(statistics.median(t_a), statistics.median(t_b))
                cell = {"frame": name, "H": H, "W": W, "rays": rays, "n_lap": n, "n_lap_rgb": n, "sets": sets,
                        "wall_ms_per_frame": med(frame), "wall_ms_all": [round(w, 3) for w in frame],
                        "pose_grad_laplace_ms": med(t_lap), "pose_grad_laplace_ms_all": [round(w, 3) for w in t_lap],
                        "single_head_pose_grad_ms": [med(t_a), med(t_b)],
                        "single_head_pose_grad_ms_all": [[round(w, 3) for w in t_a], [round(w, 3) for w in t_b]],
                        "laplace_over_single_head": round(ratio, 3),
                        "laplace_frame_render_ms": med(t_render), "laplace_frame_render_ms_all": [round(w, 3) for w in t_render],
                        "finite": bool(torch.isfinite(g).all()), "grad_rms": float(g.pow(2).mean().sqrt())}
                result["frames"].append(cell)
                print(json.dumps(cell), flush=True)
            del scene
    out = args.out or os.path.join(ROOT, "profiles", f"{args.tag}_pose_gradient_laplace.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({"out": out, "frames": len(result["frames"])}))


if __name__ == "__main__":
    main()
