"""Per-pixel pose gradients of one frame (render.pose_gradient_camera: ray kernel -> proposal sampler -> unerf_pose_grad) on
the full-table synthetic scene (active-nerfacto, log2T = 19, max_res = 2048), at 200 x 200 (the reference script's lego
frame, 40,000 autograd backward passes there) and 1920 x 1080.

Per frame size: wall ms per frame (median over --reps, device synchronised in front and behind) and the HIP-event time of the
unerf_pose_grad launches alone (ops.KernelTimer).  Beside them the instruction-derived floor: forward + backward through the
two MLPs is about 2 x 22.9 kFLOP per sample, x 48 samples ~ 2.2 MFLOP per ray, 4.6 TFLOP at 1080p, so at least 29 ms at the
157.3 TFLOP/s fp32 vector peak of the MI355X (hash-grid gathers, scans and the activation round trips through LDS not
counted).  There is no earlier path in this package to race: a recorded measurement, not a gate.
One JSON -> profiles/<tag>_pose_gradient.json.

    python benchmarks/pose_gradient.py --tag r10
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

FLOP_PER_SAMPLE = 2 * 22.9e3          # forward + backward multiply-adds of the trunk and the colour head, as FLOPs
PEAK_FP32_VECTOR = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", default="lego200,1080p")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from uncertainty_nerf_gs_amd import lib as L, ops, render, synthetic
    L.build_library()
    L.require_gpu()
    dev = torch.device("cuda:0")
    t = synthetic.make_scene_tensors(seed=0, kind="active")
    scene = synthetic.scene_to_device(t, dev)
    c2w = synthetic.orbit_c2w(0.3)
    cams = {"lego200": synthetic.CAMERA_LEGO200, "1080p": synthetic.CAMERA_1080P}
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "scene": "active, log2T 19, max_res 2048, S 48", "frames": []}
    with torch.cuda.device(dev):
        for name in [f for f in args.frames.split(",") if f]:
            cam = cams[name]
            rays = cam["H"] * cam["W"]
            for _ in range(args.warmup):
                g = render.pose_gradient_camera(scene, c2w, **cam)
            wall = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                g = render.pose_gradient_camera(scene, c2w, **cam)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            ops.TIMER = ops.KernelTimer()
            render.pose_gradient_camera(scene, c2w, **cam)
            kernels = ops.TIMER.summary()
            ops.TIMER = None
            floor_ms = rays * scene.num_nerf * FLOP_PER_SAMPLE / PEAK_FP32_VECTOR * 1e3
            cell = {"frame": name, "H": cam["H"], "W": cam["W"], "rays": rays, "wall_ms_per_frame": round(statistics.median(wall), 3),
                    "wall_ms_all": [round(w, 3) for w in wall], "pose_grad_kernel_ms": round(kernels["pose_grad"]["total_ms"], 3),
                    "sampling_ms": round(sum(v["total_ms"] for k, v in kernels.items() if k != "pose_grad"), 3),
                    "flop_floor_ms": round(floor_ms, 3),
                    "kernel_over_floor": round(kernels["pose_grad"]["total_ms"] / floor_ms, 2),
                    "finite": bool(torch.isfinite(g).all()), "grad_rms": float(g.pow(2).mean().sqrt())}
            result["frames"].append(cell)
            print(json.dumps(cell), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", f"{args.tag}_pose_gradient.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({"out": out, "frames": len(result["frames"])}))


if __name__ == "__main__":
    main()
