"""Per-pixel pose gradients of an MC-dropout frame under a named mask draw (render.pose_gradient_camera_mc: ray kernel ->
proposal sampler -> unerf_pose_grad_mc, one launch per group of rays whatever K is) on the full-table synthetic MC-dropout
scene (log2T = 19, max_res = 2048, S = 48, p = 0.2, sites TRUNK | HEAD1), at 200 x 200 and 1920 x 1080, K in {1, 8}.

Per frame size and K: wall ms per frame (median over --reps, device synchronised in front and behind), and on the frame's own
rays and bins (made once, outside the timed region) the gradient launches alone: unerf_pose_grad_mc, and in the same process
K x the unchanged single-pass unerf_pose_grad on that field -- what a loop of K launches would at best cost (it draws no
masks and skips the averaging) -- timed TWICE, for its own spread.
Expectation from the operation count: the K = 8 launch does strictly less work than 8 single passes (the 16 x 8 corner gathers,
forward and backward, and trunk layer 0 once instead of 8 times), so it should not be slower than 8 single-pass launches by
more than that spread, and visibly cheaper than 8 x the new kernel at K = 1.  A recorded measurement, not a gate.
One JSON -> profiles/<tag>_pose_gradient_mc.json.

    python benchmarks/pose_gradient_mc.py --tag r13
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--passes", default="1,8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from uncertainty_nerf_gs_amd import lib as L, ops, render, synthetic
    L.build_library()
    L.require_gpu()
    dev = torch.device("cuda:0")
    t = synthetic.make_scene_tensors(seed=0, kind="mcdropout")
    scene = synthetic.scene_to_device(t, dev, K=8, seed=1234, p_drop=0.2)
    c2w = synthetic.orbit_c2w(0.3)
    rot_inv = torch.linalg.inv(c2w[:3, :3].double()).float()
    cams = {"lego200": synthetic.CAMERA_LEGO200, "1080p": synthetic.CAMERA_1080P}
    rpl = 1 << 20
    med = lambda v: round(statistics.median(v), 3)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
              "scene": "mcdropout, log2T 19, max_res 2048, S 48, p 0.2, sites TRUNK | HEAD1", "frames": []}
    with torch.cuda.device(dev):
        for name in [f for f in args.frames.split(",") if f]:
            cam = cams[name]
            H, W = cam["H"], cam["W"]
            rays = H * W
            groups = []       # the frame's rays and bins, as pose_gradient_camera_mc makes them
            for start in range(0, rays, rpl):
                o, d, _ = ops.generate_rays(c2w, cam["fx"], cam["fy"], cam["cx"], cam["cy"], H, W, dev, start, min(rpl, rays - start))
                sb, _ = render.sample_rays(scene, o, d, None, start, want_prop_depth=False, image_width=W)
                groups.append((start, o, d, sb.clone()))
            kw = dict(rot_inv=rot_inv, spacing=scene.spacing, background=scene.background)
            for K in [int(k) for k in args.passes.split(",") if k]:
                field = dataclasses.replace(scene.field, K=K)
                sk = dataclasses.replace(scene, field=field)

                def mc():
                    for start, o, d, sb in groups:
                        ops.pose_grad_mc(o, d, sb, field, scene.near, scene.far, ray_offset=start, **kw)

                def loop():
                    for _ in range(K):
                        for start, o, d, sb in groups:
                            ops.pose_grad(o, d, sb, field, scene.near, scene.far, **kw)

                frame = _timed(lambda: render.pose_gradient_camera_mc(sk, c2w, **cam), args.reps)
                t_mc = _timed(mc, args.reps)
                t_loop_a = _timed(loop, args.reps)
                t_loop_b = _timed(loop, args.reps)
                g = render.pose_gradient_camera_mc(sk, c2w, **cam)
                cell = {"frame": name, "H": H, "W": W, "rays": rays, "K": K, "wall_ms_per_frame": med(frame),
                        "wall_ms_all": [round(w, 3) for w in frame], "pose_grad_mc_ms": med(t_mc),
                        "pose_grad_mc_ms_all": [round(w, 3) for w in t_mc],
                        "k_single_pass_launches_ms": [med(t_loop_a), med(t_loop_b)],
                        "k_single_pass_launches_ms_all": [[round(w, 3) for w in t_loop_a], [round(w, 3) for w in t_loop_b]],
                        "mc_over_k_single_pass": round(statistics.median(t_mc) / min(statistics.median(t_loop_a), statistics.median(t_loop_b)), 3),
                        "finite": bool(torch.isfinite(g).all()), "grad_rms": float(g.pow(2).mean().sqrt())}
                result["frames"].append(cell)
                print(json.dumps(cell), flush=True)
    by = {(c["frame"], c["K"]): c for c in result["frames"]}
    for name in {c["frame"] for c in result["frames"]}:
        if (name, 1) in by and (name, 8) in by:
            result.setdefault("k8_over_8x_k1", {})[name] = round(by[(name, 8)]["pose_grad_mc_ms"] / (8 * by[(name, 1)]["pose_grad_mc_ms"]), 3)
    out = args.out or os.path.join(ROOT, "profiles", f"{args.tag}_pose_gradient_mc.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({"out": out, "frames": len(result["frames"]), "k8_over_8x_k1": result.get("k8_over_8x_k1")}))


if __name__ == "__main__":
    main()
