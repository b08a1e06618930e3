"""Per-pixel pose Jacobians of one frame (render.pose_jacobian_camera: ray kernel -> proposal sampler -> unerf_pose_jacobian,
one launch per group of rays whatever the number of channels) on the full-table synthetic nerfacto scene (active-nerfacto,
log2T = 19, max_res = 2048, S = 48), at 200 x 200 and 1920 x 1080.

Per frame size, on the frame's own rays and bins (made once, outside the timed region), the launches alone, wall ms with the
device synchronised in front and behind, median over --reps:
  jac_rgb        channels {r, g, b}, want jac                      (D = 12)
  jac_all        all five channels, want jac
  var_all        all five channels, want var only, proj = pose_projection of a diagonal pose covariance (P = 6)
  pose_grad x 1  the unchanged unerf_pose_grad, and x 3 (what per-channel seeds in that entry point would at best cost),
                 each timed TWICE in the same process for its own spread
and the wall ms of the whole frame through render.pose_jacobian_camera (all five channels, jac).
Expectation from the operation count: the {r, g, b} Jacobian shares one forward pass and the compositing among three backward
passes, so it should cost clearly less than three unerf_pose_grad launches.  A recorded measurement, not a gate.
One JSON -> profiles/<tag>_pose_jacobian.json.

    python benchmarks/pose_jacobian.py --tag r17
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from uncertainty_nerf_gs_amd import lib as L, ops, posegrad, render, synthetic
    L.build_library()
    L.require_gpu()
    dev = torch.device("cuda:0")
    t = synthetic.make_scene_tensors(seed=0, kind="active")
    scene = synthetic.scene_to_device(t, dev)
    c2w = synthetic.orbit_c2w(0.3)
    rot_inv = torch.linalg.inv(c2w[:3, :3].double()).float()
    proj = posegrad.pose_projection(c2w, torch.tensor([0.01, 0.01, 0.01, 2e-3, 2e-3, 2e-3]))
    cams = {"lego200": synthetic.CAMERA_LEGO200, "1080p": synthetic.CAMERA_1080P}
    rpl = 1 << 20
    med = lambda v: round(statistics.median(v), 3)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "scene": "active, log2T 19, max_res 2048, S 48", "frames": []}
    with torch.cuda.device(dev):
        for name in [f for f in args.frames.split(",") if f]:
            cam = cams[name]
            H, W = cam["H"], cam["W"]
            rays = H * W
            groups = []       # the frame's rays and bins, as pose_jacobian_camera makes them
            for start in range(0, rays, rpl):
                o, d, _ = ops.generate_rays(c2w, cam["fx"], cam["fy"], cam["cx"], cam["cy"], H, W, dev, start, min(rpl, rays - start))
                sb, _ = render.sample_rays(scene, o, d, None, start, want_prop_depth=False, image_width=W)
                groups.append((o, d, sb.clone()))
            kw = dict(rot_inv=rot_inv, spacing=scene.spacing, background=scene.background)

            def jac(channels, want, pj=None):
                def run():
                    for o, d, sb in groups:
                        ops.pose_jacobian(o, d, sb, scene.field, scene.near, scene.far, channels=channels, proj=pj, want=want, **kw)
                return run

            def grad(n):
                def run():
                    for _ in range(n):
                        for o, d, sb in groups:
                            ops.pose_grad(o, d, sb, scene.field, scene.near, scene.far, **kw)
                return run

            t_g1a, t_g3a = _timed(grad(1), args.reps), _timed(grad(3), args.reps)
            t_rgb = _timed(jac(("r", "g", "b"), ("jac",)), args.reps)
            t_all = _timed(jac(ops.POSE_CHANNELS, ("jac",)), args.reps)
            t_var = _timed(jac(ops.POSE_CHANNELS, ("var",), proj), args.reps)
            t_g1b, t_g3b = _timed(grad(1), args.reps), _timed(grad(3), args.reps)
            frame = _timed(lambda: render.pose_jacobian_camera(scene, c2w, **cam), args.reps)
            out = render.pose_jacobian_camera(scene, c2w, want=("jac", "val"), **cam)
            g3 = [med(t_g3a), med(t_g3b)]
            cell = {"frame": name, "H": H, "W": W, "rays": rays,
                    "jac_rgb_ms": med(t_rgb), "jac_rgb_ms_all": [round(w, 3) for w in t_rgb],
                    "jac_all_ms": med(t_all), "jac_all_ms_all": [round(w, 3) for w in t_all],
                    "var_all_ms": med(t_var), "var_all_ms_all": [round(w, 3) for w in t_var],
                    "pose_grad_x1_ms": [med(t_g1a), med(t_g1b)], "pose_grad_x3_ms": g3,
                    "pose_grad_x1_ms_all": [[round(w, 3) for w in t_g1a], [round(w, 3) for w in t_g1b]],
                    "pose_grad_x3_ms_all": [[round(w, 3) for w in t_g3a], [round(w, 3) for w in t_g3b]],
                    "jac_rgb_over_3x_pose_grad": round(statistics.median(t_rgb) / min(g3), 3),
                    "jac_all_over_jac_rgb": round(statistics.median(t_all) / statistics.median(t_rgb), 3),
                    "pose_grad_x3_spread": round(abs(g3[0] - g3[1]) / min(g3), 3),
                    "frame_wall_ms_all_channels": med(frame), "frame_wall_ms_all": [round(w, 3) for w in frame],
                    "finite": bool(torch.isfinite(out["jac"]).all() and torch.isfinite(out["val"]).all()),
                    "jac_rms_per_channel": [float(out["jac"][:, :, c].pow(2).mean().sqrt()) for c in range(5)]}
            result["frames"].append(cell)
            print(json.dumps(cell), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", f"{args.tag}_pose_jacobian.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({"out": out, "frames": len(result["frames"])}))


if __name__ == "__main__":
    main()
