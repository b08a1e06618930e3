"""The pose normal equations (unerf_pose_normal_eq_accumulate / _finish): H = sum w J J^T, g = sum w r J,
chi2 = sum w r^2 of a frame's [N,C,P] pose Jacobian, reduced in float64 on the device.

1. reduction: the reduction alone on seeded [N,C,P] device tensors (with values, target and [N,C] weights) at 200 x 200,
   800 x 800 and 1920 x 1080, C in {3, 5}, P in {6, 12}.  Wall medians between two device synchronisations, host copy of the
   result included on both sides, both sides alternated in one process (torch, kernel, torch again):
     kernel_ms                 ops.pose_normal_eq_workspace + _accumulate + _finish
     torch_ms / torch_again_ms J.double(), then einsum for H and g and a sum for chi2; timed twice: the second is its own spread
     slower_than_spread        kernel median > the larger torch median
   and by device events: accumulate_ms (the accumulate launch alone), copy_ms (a torch device copy of as many bytes as the
   kernel must read: it reads AND writes them), read_gbps = bytes / accumulate_ms, accumulate_vs_copy = accumulate_ms / copy_ms.
2. nerfacto: render.pose_normal_eq_camera (what get_pose_information_for_camera runs) next to the unchanged
   render.pose_jacobian_camera with the se3 basis (what get_pose_jacobians_for_camera runs), active scene of bench.py, 200 x 200
   and 1080p, rgb.
3. splat: splat.pose_normal_eq_camera next to splat.pose_jacobian_camera on the 1 M-splat scene, 1080p, rgb.
4. refine: posegrad.refine_pose on the splat scene from a seeded twist of norm 1e-2 off a known pose, against that pose's own
   frame: the chi2 and pose-error traces, recorded as they come.  Not a gate.
No speed is a pass condition.  One JSON -> profiles/<tag>_pose_normal_eq.json.

    python benchmarks/pose_normal_eq.py --tag r22
"""
import argparse
import json
import math
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
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


def _pose_error(c2w, ref):
    """(|t - t_ref|, the angle of R_ref^T R in radians)"""
    c2w, ref = c2w.double(), ref.double()
    cosang = float(((ref[:, :3].T @ c2w[:, :3]).diagonal().sum() - 1.0) / 2.0)
    return float((c2w[:, 3] - ref[:, 3]).norm()), math.acos(max(-1.0, min(1.0, cosang)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--splats", type=int, default=1_000_000)
    ap.add_argument("--sizes", default="200x200,800x800,1920x1080")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from uncertainty_nerf_gs_amd import lib as L, ops, posegrad, render, splat, synthetic
    L.build_library()
    L.require_gpu()
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "tile": L.POSE_NEQ_TILE,
              "reduction": [], "nerfacto": [], "splat": [], "refine": None}
    reps = range(-args.warmup, args.reps)
    with torch.cuda.device(dev):
        # -- 1. the reduction alone --
        for size in args.sizes.split(","):
            W, H = (int(v) for v in size.split("x"))
            N = H * W
            for Cn in (3, 5):
                for P in (6, 12):
                    g = torch.Generator(device=dev).manual_seed(N + 10 * Cn + P)
                    J = torch.randn(N, Cn, P, device=dev, generator=g)
                    val = torch.rand(N, Cn, device=dev, generator=g)
                    tgt = val + 0.1 * torch.randn(N, Cn, device=dev, generator=g)
                    w = torch.rand(N, Cn, device=dev, generator=g) + 0.5

                    def kernel():
                        ws = ops.pose_normal_eq_workspace(N, P, dev)
                        ops.pose_normal_eq_accumulate(ws, J, val, tgt, w)
                        return ops.pose_normal_eq_finish(ws)

                    def torch_route():
                        Jd, wd, rd = J.double(), w.double(), val.double() - tgt.double()
                        Hm = torch.einsum("nca,ncb->ab", Jd * wd[..., None], Jd)
                        gv = torch.einsum("nc,nca->a", wd * rd, Jd)
                        return Hm.cpu(), gv.cpu(), float((wd * rd * rd).sum())

                    nbytes = 4 * (N * Cn * P + 3 * N * Cn)
                    src = torch.empty(nbytes // 4, device=dev)
                    dst = torch.empty_like(src)
                    ws1 = ops.pose_normal_eq_workspace(N, P, dev)
                    t = {k: [] for k in ("torch", "kernel", "torch_again", "accumulate", "copy")}
                    for rep in reps:
                        times = {"torch": _wall_ms(torch_route), "kernel": _wall_ms(kernel), "torch_again": _wall_ms(torch_route),
                                 "accumulate": _event_ms(lambda: ops.pose_normal_eq_accumulate(ws1, J, val, tgt, w)),
                                 "copy": _event_ms(lambda: dst.copy_(src))}
                        if rep >= 0:
                            for k, v in times.items():
                                t[k].append(v)
                    got, (Hm, gv, c2) = kernel(), torch_route()
                    cell = {"H": H, "W": W, "C": Cn, "P": P, "bytes_read": nbytes, "kernel_ms": _stats(t["kernel"]),
                            "torch_ms": _stats(t["torch"]), "torch_again_ms": _stats(t["torch_again"]),
                            "accumulate_ms": _stats(t["accumulate"]), "copy_ms": _stats(t["copy"])}
                    cell["kernel_vs_torch"] = round(cell["kernel_ms"]["median"] / cell["torch_ms"]["median"], 3)
                    cell["torch_again_vs_torch"] = round(cell["torch_again_ms"]["median"] / cell["torch_ms"]["median"], 3)
                    cell["slower_than_spread"] = cell["kernel_ms"]["median"] > max(cell["torch_ms"]["median"], cell["torch_again_ms"]["median"])
                    cell["read_gbps"] = round(nbytes / cell["accumulate_ms"]["median"] * 1e-6, 1)
                    cell["copy_gbps_read_plus_write"] = round(2 * nbytes / cell["copy_ms"]["median"] * 1e-6, 1)
                    cell["accumulate_vs_copy"] = round(cell["accumulate_ms"]["median"] / cell["copy_ms"]["median"], 3)
                    cell["max_rel_diff_to_torch"] = float(np.abs(got["information"] / Hm.numpy() - 1).max())
                    result["reduction"].append(cell)
                    print(json.dumps(cell), flush=True)
                    del J, val, tgt, w, src, dst
        # -- 2. the nerfacto frame --
        scene = synthetic.scene_to_device(synthetic.make_scene_tensors(seed=0, kind="active"), dev)
        c2w = synthetic.orbit_c2w(0.3)
        for name, cam in (("lego200", synthetic.CAMERA_LEGO200), ("1080p", synthetic.CAMERA_1080P)):
            basis = posegrad.tangent_basis(c2w)
            jac = lambda: render.pose_jacobian_camera(scene, c2w, channels=("r", "g", "b"), proj=basis, want=("proj", "val"), **cam)
            image = jac()["val"].clone()
            info = lambda: render.pose_normal_eq_camera(scene, c2w, target=image, **cam)
            t = {k: [] for k in ("jacobians", "information", "jacobians_again")}
            for rep in reps:
                times = {"jacobians": _wall_ms(jac), "information": _wall_ms(info), "jacobians_again": _wall_ms(jac)}
                if rep >= 0:
                    for k, v in times.items():
                        t[k].append(v)
            ops.TIMER = ops.KernelTimer()
            out = info()
            kernels = ops.TIMER.summary()
            ops.TIMER = None
            cell = {"frame": name, "H": cam["H"], "W": cam["W"], **{k + "_ms": _stats(v) for k, v in t.items()},
                    "pose_normal_eq_ms": round(kernels["pose_normal_eq"]["total_ms"] + kernels["pose_normal_eq_finish"]["total_ms"], 4),
                    "pose_jacobian_ms": round(kernels["pose_jacobian"]["total_ms"], 4), "chi2": out["chi2"], "rank": out["rank"]}
            cell["information_vs_jacobians"] = round(cell["information_ms"]["median"] / cell["jacobians_ms"]["median"], 3)
            result["nerfacto"].append(cell)
            print(json.dumps(cell), flush=True)
        del scene
        # -- 3. the splat frame, 4. the refinement --
        gp = {k: v.to(dev) for k, v in synthetic.make_splat_tensors(seed=7, N=args.splats).items()}
        bg = torch.zeros(3, device=dev)
        W, H = 1920, 1080
        cam = dict(fx=1111.0, fy=1111.0, cx=W / 2, cy=H / 2, H=H, W=W)
        c2w0 = synthetic.orbit_c2w(0.9, radius=2.5, height=0.5)[:3, :4]
        basis = posegrad.tangent_basis(c2w0)
        jac = lambda: splat.pose_jacobian_camera(gp, c2w0, background=bg, proj=basis, channels=("r", "g", "b"), want=("proj", "val"), **cam)
        image = jac()["val"].clone()
        info = lambda: splat.pose_normal_eq_camera(gp, c2w0, background=bg, target=image, **cam)
        t = {k: [] for k in ("jacobians", "information", "jacobians_again")}
        for rep in reps:
            times = {"jacobians": _wall_ms(jac), "information": _wall_ms(info), "jacobians_again": _wall_ms(jac)}
            if rep >= 0:
                for k, v in times.items():
                    t[k].append(v)
        cell = {"H": H, "W": W, "splats": args.splats, **{k + "_ms": _stats(v) for k, v in t.items()}}
        cell["information_vs_jacobians"] = round(cell["information_ms"]["median"] / cell["jacobians_ms"]["median"], 3)
        result["splat"].append(cell)
        print(json.dumps(cell), flush=True)
        xi = np.random.default_rng(22).standard_normal(6)
        xi *= 1e-2 / np.linalg.norm(xi)
        start = SimpleNamespace(camera_to_worlds=posegrad.apply_pose_step(c2w0, xi))
        ref = posegrad.refine_pose(lambda c, image=None: splat.pose_normal_eq_camera(gp, c.camera_to_worlds, background=bg, target=image, **cam),
                                   start, image, iters=10, damping=1e-3)
        result["refine"] = {"H": H, "W": W, "twist": xi.tolist(), "chi2": ref["chi2"], "accepted": ref["accepted"],
                            "pose_error_t_and_angle": [_pose_error(p, c2w0) for p in ref["poses"]], "rank": ref["rank"],
                            "final_damping": ref["damping"], "covariance_diag": np.diag(ref["covariance"]).tolist()}
        print(json.dumps(result["refine"]), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", f"{args.tag}_pose_normal_eq.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({"out": out, "slower_than_spread": [[c["H"], c["W"], c["C"], c["P"]] for c in result["reduction"] if c["slower_than_spread"]]}))


if __name__ == "__main__":
    main()
