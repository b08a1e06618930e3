"""Batched splat rendering against a loop of single-view calls, at the BASELINE size (1 M splats, 1920 x 1080, tight lists).

For active-splatfacto and plain splatfacto and B in --batches: one splat.active_splatfacto_outputs_batch call of B views vs a
loop of B splat.active_splatfacto_outputs calls, the poses on the host, each form warmed up, the two forms alternated batch
by batch, device events around each whole batch.  Prints one JSON line per (model, B) with ms per view, Mpix/s and the
ratio batch / loop; --reps repeats the whole sweep (the spread between repetitions is the noise to beat).

    python benchmarks/splat_view_batch.py [--batches 1,2,4,8] [--iters 20] [--warmup 3] [--reps 2]
    python benchmarks/splat_view_batch.py --profile-batch 4    # a few B = 4 batches only (for rocprofv3 --kernel-trace --stats)
    python benchmarks/splat_view_batch.py --profile-single 4   # the same frames as single-view calls (same use)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uncertainty_nerf_gs_amd import lib, splat, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--models", default="active,plain")
    ap.add_argument("--profile-batch", type=int, default=0)
    ap.add_argument("--profile-single", type=int, default=0)
    args = ap.parse_args()
    lib.build_library()
    lib.require_gpu()
    dev = torch.device("cuda:0")
    cam = synthetic.CAMERA_1080P
    K = (cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["H"], cam["W"])
    bg = splat.background_for("random").to(dev)      # device-resident, as the model passes it (no H2D copy per call)
    full = {k: v.to(dev) for k, v in synthetic.make_splat_tensors(7, 1_000_000).items()}
    Bmax = max([int(b) for b in args.batches.split(",")] + [args.profile_batch, args.profile_single])
    poses = [synthetic.orbit_c2w(0.25 + 2 * 3.14159265 * v / Bmax) for v in range(Bmax)]     # host-resident
    stacked = torch.stack(poses)

    def batch_call(gp, B):
        return splat.active_splatfacto_outputs_batch(gp, stacked[:B], *K, bg)

    def loop_call(gp, B):
        return [splat.active_splatfacto_outputs(gp, poses[v], *K, bg) for v in range(B)]

    if args.profile_batch or args.profile_single:
        B = args.profile_batch or args.profile_single
        for _ in range(args.warmup + args.iters):
            (batch_call if args.profile_batch else loop_call)(full, B)
        torch.cuda.synchronize()
        print(json.dumps({"profile_batch" if args.profile_batch else "profile_single": B, "batches": args.warmup + args.iters}))
        return
    models = {"active": full, "plain": {k: v for k, v in full.items() if k != "log_uncertainties"}}
    for rep in range(args.reps):
        for name in args.models.split(","):
            gp = models[name]
            for B in [int(b) for b in args.batches.split(",")]:
                for _ in range(args.warmup):
                    batch_call(gp, B)
                    loop_call(gp, B)
                torch.cuda.synchronize()
                t = {"batch": 0.0, "loop": 0.0}
                for _ in range(args.iters):
                    for form, fn in (("batch", batch_call), ("loop", loop_call)):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        fn(gp, B)
                        e1.record()
                        e1.synchronize()
                        t[form] += e0.elapsed_time(e1)
                ms = {f: t[f] / (args.iters * B) for f in t}
                mpix = {f: cam["H"] * cam["W"] / (ms[f] * 1e3) for f in ms}
                print(json.dumps({"rep": rep, "model": name, "B": B, "batch_ms_per_view": round(ms["batch"], 4),
                                  "loop_ms_per_view": round(ms["loop"], 4), "batch_mpix_s": round(mpix["batch"], 1),
                                  "loop_mpix_s": round(mpix["loop"], 1), "ratio": round(ms["batch"] / ms["loop"], 4),
                                  "iters": args.iters}), flush=True)


if __name__ == "__main__":
    main()
