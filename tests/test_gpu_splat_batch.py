"""Batched splat rendering (splat.active_splatfacto_outputs_batch, SplatfactoModel.get_outputs_for_cameras): every view of a
batch is BIT-identical to a single-view render with that view's camera, on every output key -- torch.equal, no tolerance.
The single-view frame itself is held to the bits it had before the kernels gained a view index by a recorded digest
(tests/golden/splat_frame_digest.json)."""
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "splat_frame_digest.json")
DIGEST_K = (120.0, 118.0, 61.0, 52.0, 100, 130)     # fx, fy, cx, cy, H, W: partial edge tiles on both axes


def _scene(N, seed=7, scale_shift=1.5):
    from uncertainty_nerf_gs_amd import synthetic
    gp = synthetic.make_splat_tensors(seed, N)
    gp["scales"] = gp["scales"] + scale_shift
    return gp


def _pose(theta, radius=2.5, height=0.5):
    from uncertainty_nerf_gs_amd import synthetic
    return synthetic.orbit_c2w(theta, radius=radius, height=height)


def splat_frame_digest(dev) -> str:
    """SHA-256 over every output key of two seeded single-view frames: active-splatfacto (classic, tight lists, SH degree 3)
    and plain splatfacto (antialiased, gsplat's lists)"""
    from uncertainty_nerf_gs_amd import splat
    gp = {k: v.to(dev) for k, v in _scene(20000, seed=11).items()}
    plain = {k: v for k, v in gp.items() if k != "log_uncertainties"}
    bg = torch.tensor([0.1490, 0.1647, 0.2157])
    h = hashlib.sha256()
    frames = (splat.active_splatfacto_outputs(gp, _pose(0.7), *DIGEST_K, bg),
              splat.active_splatfacto_outputs(plain, _pose(2.1), *DIGEST_K, bg, rasterize_mode="antialiased", tight=False))
    torch.cuda.synchronize()
    for out in frames:
        for k in sorted(out):
            h.update(k.encode())
            h.update(out[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _look_at(eye, target):
    """3x4 camera-to-world looking from eye at target, up = +z (the convention of synthetic.orbit_c2w)"""
    import numpy as np
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    return torch.from_numpy(np.stack([right, up, -fwd, eye], axis=1).astype(np.float32))


def _assert_views_equal(batch, singles):
    assert len(batch) == len(singles)
    for v, (b, s) in enumerate(zip(batch, singles)):
        assert set(b) == set(s), (v, sorted(b), sorted(s))
        for k in s:
            assert b[k].shape == s[k].shape and torch.equal(b[k], s[k]), f"view {v}: {k}"


def _batch_vs_singles(gp, poses, intr, H, W, bg, **kw):
    from uncertainty_nerf_gs_amd import splat
    fx, fy, cx, cy = intr
    per = lambda x, v: x[v] if isinstance(x, (list, tuple)) else x
    batch = splat.active_splatfacto_outputs_batch(gp, torch.stack(poses), fx, fy, cx, cy, H, W, bg, **kw)
    singles = [splat.active_splatfacto_outputs(gp, poses[v], per(fx, v), per(fy, v), per(cx, v), per(cy, v), H, W, bg, **kw)
               for v in range(len(poses))]
    torch.cuda.synchronize()
    _assert_views_equal(batch, singles)
    return batch


CASES = [("b1", 1, True, {}), ("b3", 3, True, {}), ("b8_aa", 8, True, dict(rasterize_mode="antialiased")),
         ("plain_b3", 3, False, {}), ("plain_b8_aa_box", 8, False, dict(rasterize_mode="antialiased", tight=False)),
         ("sh0", 3, True, dict(config_sh_degree=0)), ("sh_early", 3, True, dict(sh_degree=1)),
         ("box_lists", 3, True, dict(tight=False)), ("crop", 3, True, "crop")]


@pytest.mark.parametrize("tag,B,active,kw", CASES, ids=[c[0] for c in CASES])
def test_batch_views_equal_single_view_calls(dev, tag, B, active, kw):
    gp = {k: v.to(dev) for k, v in _scene(20000).items()}
    if not active:
        gp.pop("log_uncertainties")
    if kw == "crop":
        kw = dict(crop_ids=(gp["means"][:, 0] < 0.4) & (gp["means"][:, 2] > -0.6))
    H, W = 100, 130
    poses = [_pose(0.3 + 0.77 * v, radius=2.5 + 0.1 * v, height=0.5 - 0.1 * v) for v in range(B)]
    fx = [110.0] * B
    fx[-1] = 143.0                                    # one view with other intrinsics
    _batch_vs_singles(gp, poses, (fx, 112.0, [64.0] * (B - 1) + [60.5], 51.0), H, W, torch.tensor([0.1, 0.2, 0.3]), **kw)


# (H, W, view order): 100 x 130 has 63 tiles (the one-pass tile sort); 256 x 256 has 256 (the two-pass segmented tile sort,
# with views of zero chunks between and before the others)
MIXED = [(100, 130, ("normal", "away", "faint")), (256, 256, ("away", "normal", "faint", "normal2"))]


@pytest.mark.parametrize("H,W,order", MIXED, ids=["63_tiles", "256_tiles"])
def test_batch_with_empty_and_all_faint_views(dev, H, W, order):
    """one batch: normal views, a view looking away (get_empty_outputs), and a view whose visible splats are all fainter than
    1/255 (the reference rasterises it: nothing blends, depth 0 -- not the empty picture)"""
    gp = {k: v.clone() for k, v in _scene(20000).items()}
    far = torch.arange(20000) % 10 == 0                # a faint cluster around (10, 0, 0), the rest around the origin
    gp["means"][far] = gp["means"][far] * 0.5 + torch.tensor([10.0, 0.0, 0.0])
    gp["opacities"][far] = -9.0
    gp = {k: v.to(dev) for k, v in gp.items()}
    pose = {"normal": _pose(0.5), "normal2": _pose(2.0, radius=2.2), "away": _look_at([0.0, 5.0, 0.0], [0.0, 9.0, 0.0]),
            "faint": _look_at([7.0, 0.0, 0.2], [10.0, 0.0, 0.0])}
    out = _batch_vs_singles(gp, [pose[k] for k in order], (0.85 * W, 0.85 * W, W / 2, H / 2), H, W, torch.tensor([0.1, 0.2, 0.3]))
    for k, o in zip(order, out):
        if k.startswith("normal"):
            assert "uncertainty" in o and float(o["accumulation"].max()) > 0.5
        elif k == "away":
            assert set(o) == {"rgb", "depth", "accumulation", "background"} and float(o["depth"].min()) == 10.0
        else:
            assert "uncertainty" in o
            assert float(o["depth"].abs().max()) == 0.0 and float(o["accumulation"].max()) == 0.0


@pytest.mark.parametrize("H,W,B", [(256, 256, 1), (1440, 2560, 2)], ids=["two_pass_b1", "beyond_batch_tiles"])
def test_batch_one_view_two_pass_and_large_images(dev, H, W, B):
    """B = 1 through the two-pass segmented tile sort; an image of more than SPLAT_BATCH_MAX_TILES tiles (14,400) is rendered
    view by view with the same results"""
    gp = {k: v.to(dev) for k, v in _scene(20000).items()}
    poses = [_pose(0.4 + 1.3 * v) for v in range(B)]
    _batch_vs_singles(gp, poses, (0.8 * W, 0.8 * W, W / 2, H / 2), H, W, torch.tensor([0.1, 0.2, 0.3]))


def test_batch_at_baseline_size(dev):
    """BASELINE size: 1 M splats, 1920 x 1080, four views, tight lists -- each view equals its single-view call, and a second
    batch render repeats the bits"""
    from uncertainty_nerf_gs_amd import splat, synthetic
    gp = {k: v.to(dev) for k, v in synthetic.make_splat_tensors(7, 1_000_000).items()}
    cam = synthetic.CAMERA_1080P
    K = (cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["H"], cam["W"])
    poses = [synthetic.orbit_c2w(0.25 + 1.1 * v) for v in range(4)]
    bg = splat.background_for("random")
    a = _batch_vs_singles(gp, poses, K[:4], K[4], K[5], bg)
    b = splat.active_splatfacto_outputs_batch(gp, torch.stack(poses), *K, bg)
    _assert_views_equal(b, a)


def test_single_view_frame_matches_the_recorded_digest(dev):
    with open(GOLDEN) as f:
        want = json.load(f)["sha256"]
    assert splat_frame_digest(dev) == want


class _Box:
    """stand-in for a nerfstudio OrientedBox: axis-aligned, `within(points) -> bool [N,1]`"""

    def __init__(self, lo, hi):
        self.lo, self.hi = lo, hi

    def within(self, pts):
        lo, hi = torch.tensor(self.lo, device=pts.device), torch.tensor(self.hi, device=pts.device)
        return ((pts > lo) & (pts < hi)).all(dim=-1, keepdim=True)


@pytest.mark.parametrize("box", [None, _Box([-0.5, -0.5, -0.5], [0.6, 0.6, 0.6])], ids=["full", "obb"])
def test_model_get_outputs_for_cameras(dev, box):
    """get_outputs_for_cameras over 11 cameras in groups of at most 4: element i is get_outputs_for_camera(camera i)"""
    import test_gpu_splat as TS
    from uncertainty_nerf_gs_amd import models
    m, cam, _ = TS._fixture_model(dev)
    B = 11
    c2w = torch.stack([_look_at(_pose(0.4 * v, radius=2.0)[:, 3].numpy(), [0.0, 0.0, 0.0]) if v % 2 else cam.camera_to_worlds
                       for v in range(B)])
    fx = torch.tensor([cam.fx + 2.0 * v for v in range(B)])
    cams = models.Camera(c2w, fx, cam.fy, cam.cx, cam.cy, cam.height, cam.width)
    outs = m.get_outputs_for_cameras(cams, obb_box=box, max_views=4)
    singles = [m.get_outputs_for_camera(models.Camera(c2w[v], float(fx[v]), cam.fy, cam.cx, cam.cy, cam.height, cam.width),
                                        obb_box=box) for v in range(B)]
    torch.cuda.synchronize()
    _assert_views_equal(outs, singles)


if __name__ == "__main__":   # prints the digest of the library in use (UNERF_LIB selects another build)
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from uncertainty_nerf_gs_amd import lib
    lib.build_library()
    print(splat_frame_digest(torch.device("cuda:0")))
