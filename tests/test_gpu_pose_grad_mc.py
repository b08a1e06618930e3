"""unerf_pose_grad_mc on the GPU against the float64 reference of tests/pose_grad_mc_cases.py, the explicit-mask mode against
the counter generator, the K = 1 / all-kept launch against unerf_pose_grad, linearity over the passes at the workload's shape,
launch geometry, repeatability, refusals, and the frame-level entry points.

Tolerance (pose_grad_mc_cases.py): on the rays the reference keeps, max |g - g64| / rms(g64) may be KERNEL_FACTOR = 4 x the
fp32 torch oracle's own error under the same masks, which every test computes itself; out_rgb 4 x the oracle's + 2^-23.

Measured on MI355X (kernel error / oracle error relative to the case's RMS gradient, share of rays left out), DESIGN.md 4.6a:
  S1 1.20e-5 / 1.22e-5 (0.000), S2 2.13e-5 / 2.15e-5 (0.023), S16 0.90e-5 / 0.88e-5 (0.133), tcnn 1.12e-5 / 1.02e-5 (0.055),
  tcnn_half 1.14e-5 / 1.19e-5 (0.109), white 1.98e-5 / 2.19e-5 (0.125), random 1.08e-5 / 1.06e-5 (0.086), aabb 1.06e-5 / 1.10e-5
  (0.133), uniform 0.91e-5 / 0.93e-5 (0.094), S48K2 1.35e-5 / 1.19e-5 (0.117), S64K2 0.77e-5 / 0.72e-5 (0.055), S64K3 0.66e-5 /
  0.68e-5 (0.102), S63K2 0.74e-5 / 0.72e-5 (0.148), S47K2 1.27e-5 / 1.17e-5 (0.148), K16 1.41e-5 / 1.45e-5 (0.062), K64 1.81e-5 /
  1.79e-5 (0.078), head0 1.26e-5 / 1.02e-5 (0.062; the largest ratio, 1.24), trunk_only 0.97e-5 / 1.00e-5 (0.133); the 12-entry
  pose form S16 1.36e-5 / 1.36e-5, tcnn 1.42e-5 / 1.27e-5; out_rgb <= 4.3e-7 (oracle 4.3e-7).  Linearity at K = 8 x S = 48:
  |g8 - mean_k g_k| / rms = 6.0e-7 (allowed 8.0e-5); the eight single passes 0.83 .. 1.14 x their oracles.
  (The sampler of the case builder runs on the host CPU, so the shares differ in the third digit between machines.)"""
import ctypes as C
import dataclasses
import warnings
from types import SimpleNamespace

import pytest
import torch

import pose_grad_cases as PC
import pose_grad_mc_cases as MC

pytestmark = pytest.mark.gpu

GUARD = 12345.0
_SCENES = {}


def _scene(dev, name, K=None, p=None, seed=None):
    """the case's scene (field with the case's K, sites, p and mask seed unless overridden) and rays on the device"""
    from uncertainty_nerf_gs_amd import synthetic
    s = MC.spec(name)
    key = (name, K, p, seed)
    if key not in _SCENES:
        sd = synthetic.scene_to_device(s.c.t, dev, K=s.K if K is None else K, seed=s.seed if seed is None else seed,
                                       p_drop=s.p if p is None else p, drop_sites=0 if s.sites == MC.DEFAULT_SITES else s.sites)
        _SCENES[key] = SimpleNamespace(scene=sd, o=s.c.origins.to(dev), d=s.c.directions.to(dev), sb=s.c.sbins.to(dev), S=s.c.S, R=s.c.R)
    return _SCENES[key]


def _grad(dev, s, r0=0, R=None, field=None, **kw):
    from uncertainty_nerf_gs_amd import ops
    R = s.R - r0 if R is None else R
    sc = s.scene
    with torch.cuda.device(dev):
        out = ops.pose_grad_mc(s.o[r0:r0 + R].contiguous(), s.d[r0:r0 + R].contiguous(), s.sb[r0:r0 + R].contiguous(),
                               sc.field if field is None else field, sc.near, sc.far, spacing=sc.spacing, background=sc.background, **kw)
        torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_matches_float64_reference(dev, name):
    """every float64-held case in counter mode (masks = NULL, the case's mask seed, ray_offset 0): S in {1, 2, 16, 47, 48, 63,
    64}, K in {2, 3, 4, 8, 16, 64}, sites TRUNK | HEAD1, HEAD0 | HEAD1, TRUNK, both grid layouts, the backgrounds, aabb,
    uniform spacing"""
    s = _scene(dev, name)
    got, rgb = _grad(dev, s, want_rgb=True)
    assert got.shape == (s.R, 6) and rgb.shape == (s.R, 3) and torch.isfinite(got).all()
    ref, o32 = MC.reference64(name), MC.oracle32(name)
    yard, err = MC.rel_error(o32.grad, ref), MC.rel_error(got.cpu(), ref)
    rgb_yard = (o32.rgb.double() - ref.rgb).abs().max().item()
    rgb_err = (rgb.cpu().double() - ref.rgb).abs().max().item()
    print(f"[pose_grad_mc] {name}: kernel {err:.3e}, fp32 oracle {yard:.3e}, ratio {err / yard:.2f}, "
          f"{1 - ref.keep.double().mean().item():.3f} left out; rgb kernel {rgb_err:.3e}, oracle {rgb_yard:.3e}")
    assert err <= MC.KERNEL_FACTOR * yard
    assert rgb_err <= MC.KERNEL_FACTOR * rgb_yard + 2.0 ** -23


@pytest.mark.parametrize("name", ["S16", "tcnn"])
def test_pose_epilogue_non_orthonormal(dev, name):
    """rot_inv of a scaled, sheared rotation block: [R,12] = P (R^-1 d) | g_o of the float64 reference; its origin column is
    the six-column launch's, bit for bit"""
    s, c, ref, o32 = _scene(dev, name), MC.spec(name).c, MC.reference64(name), MC.oracle32(name)
    g = torch.Generator().manual_seed(11)
    rot = c.c2w[:, :3].double() @ (torch.eye(3, dtype=torch.float64) * 1.6 + 0.25 * torch.randn(3, 3, generator=g, dtype=torch.float64))
    rot_inv = torch.linalg.inv(rot).float()
    got = _grad(dev, s, rot_inv=rot_inv)
    assert got.shape == (c.R, 12)
    want = PC.pose_from_ray_grad(ref.grad, c.directions, rot_inv).reshape(c.R, 12)
    yard = MC.rel_error(PC.pose_from_ray_grad(o32.grad, c.directions, rot_inv).reshape(c.R, 12), ref, want)
    err = MC.rel_error(got.cpu(), ref, want)
    print(f"[pose_grad_mc] {name} pose: kernel {err:.3e}, fp32 oracle {yard:.3e}, ratio {err / yard:.2f}")
    assert err <= MC.KERNEL_FACTOR * yard
    assert torch.equal(got.view(c.R, 3, 4)[:, :, 3], _grad(dev, s)[:, :3])


@pytest.mark.parametrize("name", ["S16", "head0"])
@pytest.mark.parametrize("a", [0, 1000])
def test_counter_mode_equals_explicit_masks(dev, name, a):
    """masks = NULL with p->seed and ray_offset = a == the explicit mode under ops.mc_keep_bits(field, a * S, R * S)"""
    from uncertainty_nerf_gs_amd import ops
    s = _scene(dev, name)
    with torch.cuda.device(dev):
        km = ops.mc_keep_bits(s.scene.field, a * s.S, s.R * s.S)
    want = _grad(dev, s, ray_offset=a, want_rgb=True)
    got = _grad(dev, s, ray_offset=7, keep_masks=km, want_rgb=True)       # (ray_offset is not read with explicit masks)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    if a:
        assert not torch.equal(want[0], _grad(dev, s, ray_offset=0))


@pytest.mark.parametrize("name", ["S1", "S16", "S48K2", "S64K2"])
def test_single_pass_all_kept_is_unerf_pose_grad(dev, name):
    """the anchor: K = 1, p = 0, all-ones explicit masks -> unerf_pose_grad's bits on the same MCDROPOUT-mode field"""
    from uncertainty_nerf_gs_amd import ops
    s = _scene(dev, name, K=1, p=0.0)
    sc = s.scene
    ones = torch.full((1, s.R * s.S, 2), -1, dtype=torch.int32, device=dev)
    km = ops.KeepMasks(ones, None, ones, None, s.R * s.S, 0)
    for rot_inv in (None, torch.linalg.inv(MC.spec(name).c.c2w[:, :3].double()).float()):
        got = _grad(dev, s, keep_masks=km, rot_inv=rot_inv, want_rgb=True)
        with torch.cuda.device(dev):
            want = ops.pose_grad(s.o, s.d, s.sb, sc.field, sc.near, sc.far, rot_inv=rot_inv, spacing=sc.spacing, background=sc.background,
                                 want_rgb=True)
            torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[0].abs().max() > 0


def test_linear_in_the_passes_at_the_workload_shape(dev):
    """R = 128, S = 48, K = 8, all rays: the K = 8 launch against the float64 host mean of eight K = 1 launches of the same
    kernel, each given pass k's slice of the exported counter masks; every single pass against its own float64 reference.
    Bound: 8 x the fp32 oracle's error of the K = 1, S = 48 case (two fp32 evaluations of one function, each allowed 4 x); of
    the eight single-pass cases the smallest oracle error is taken."""
    from uncertainty_nerf_gs_amd import ops
    s = _scene(dev, "lin48")
    f8 = s.scene.field
    f1 = dataclasses.replace(f8, K=1)
    with torch.cuda.device(dev):
        km = ops.mc_keep_bits(f8, 0, s.R * s.S)
    g8 = _grad(dev, s, keep_masks=km)
    assert torch.equal(g8, _grad(dev, s))                                 # the counter-mode launch of the workload's shape
    singles, yards = [], []
    for k in range(f8.K):
        kmk = ops.KeepMasks(km.trunk[k:k + 1].contiguous(), None, km.head1[k:k + 1].contiguous(), None, km.pass_stride, 0)
        gk = _grad(dev, s, field=f1, keep_masks=kmk)
        ref, o32 = MC.reference64("lin48", (k,)), MC.oracle32("lin48", (k,))
        yard, err = MC.rel_error(o32.grad, ref), MC.rel_error(gk.cpu(), ref)
        print(f"[pose_grad_mc] lin48 pass {k}: kernel {err:.3e}, fp32 oracle {yard:.3e}, ratio {err / yard:.2f}, "
              f"{1 - ref.keep.double().mean().item():.3f} left out")
        assert err <= MC.KERNEL_FACTOR * yard
        singles.append(gk.cpu().double())
        yards.append(yard)
    mean = torch.stack(singles).mean(0)
    dev8 = (g8.cpu().double() - mean).abs().max().item() / mean.pow(2).mean().sqrt().item()
    print(f"[pose_grad_mc] lin48: |g8 - mean_k g_k| / rms = {dev8:.3e}, allowed {8 * min(yards):.3e}")
    assert dev8 <= 8 * min(yards)


@pytest.mark.parametrize("R", MC.R_SUB)
def test_launch_sizes(dev, R):
    """the first R rays of the 257-ray case return the bits of the full launch's rows (one ray per block)"""
    s = _scene(dev, "geom")
    full = _grad(dev, s, want_rgb=True)
    got = _grad(dev, s, R=R, want_rgb=True)
    assert torch.equal(got[0], full[0][:R]) and torch.equal(got[1], full[1][:R])


def test_ray_offset_numbers_the_masks(dev):
    """rays [100, 257) launched alone with ray_offset = 100 return rows 100.. of the full counter-mode launch"""
    s = _scene(dev, "geom")
    full = _grad(dev, s, want_rgb=True)
    part = _grad(dev, s, r0=100, ray_offset=100, want_rgb=True)
    assert torch.equal(part[0], full[0][100:]) and torch.equal(part[1], full[1][100:])
    assert not torch.equal(_grad(dev, s, r0=100, ray_offset=0), full[0][100:])


def _raw_call(dev, s, R, grad, rgb, rot_inv=None, cs=None, km=None, S=None, near=None):
    """the C entry point on caller-owned buffers"""
    from uncertainty_nerf_gs_amd import lib as L, ops
    sc = s.scene
    cs = sc.field.cstruct() if cs is None else cs
    bg_mode, bg_rgb = ops._background(sc.background)
    ri = None if rot_inv is None else (C.c_float * 9)(*[float(v) for v in rot_inv.reshape(-1)])
    return L.load().unerf_pose_grad_mc(s.o.data_ptr(), s.d.data_ptr(), s.sb.data_ptr(), R, s.S if S is None else S,
                                       sc.near if near is None else near, sc.far, sc.spacing, 0, C.byref(cs),
                                       None if km is None else C.byref(km), bg_mode, bg_rgb, ri, grad.data_ptr(),
                                       None if rgb is None else rgb.data_ptr(), torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("pose", [False, True])
def test_guard_rows_dirty_outputs_streams_and_repeats(dev, pose):
    """R = 5 of the 257-ray case into NaN-filled buffers with guard rows behind the last ray; again; again on a side stream:
    the same bits, the guard rows keep theirs; out_rgb = NULL gives the same gradient"""
    s, R = _scene(dev, "geom"), 5
    cols = 12 if pose else 6
    rot_inv = torch.linalg.inv(MC.spec("geom").c.c2w[:, :3].double()).float() if pose else None
    with torch.cuda.device(dev):
        outs = []
        for it in range(3):
            grad = torch.full((R + 3, cols), float("nan"), device=dev)
            rgb = torch.full((R + 3, 3), float("nan"), device=dev)
            grad[R:] = GUARD
            rgb[R:] = GUARD
            if it == 2:
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    assert _raw_call(dev, s, R, grad, rgb, rot_inv) == 0
                side.synchronize()
            else:
                assert _raw_call(dev, s, R, grad, rgb, rot_inv) == 0
            torch.cuda.synchronize()
            assert bool((grad[R:] == GUARD).all()) and bool((rgb[R:] == GUARD).all())
            assert torch.isfinite(grad[:R]).all() and torch.isfinite(rgb[:R]).all()
            outs.append((grad[:R].clone(), rgb[:R].clone()))
        for g, c in outs[1:]:
            assert torch.equal(g, outs[0][0]) and torch.equal(c, outs[0][1])
        if not pose:
            assert torch.equal(outs[0][0], _grad(dev, s)[:R])
        grad = torch.full((R, cols), float("nan"), device=dev)
        assert _raw_call(dev, s, R, grad, None, rot_inv) == 0
        torch.cuda.synchronize()
        assert torch.equal(grad, outs[0][0])


def test_device_refusals(dev):
    from uncertainty_nerf_gs_amd import lib as L, ops, synthetic
    s = _scene(dev, "S16")
    sc, c = s.scene, MC.spec("S16").c
    lib = L.load()
    n = s.R * s.S
    grad = torch.zeros(s.R, 6, device=dev)
    ones = torch.full((8, n, 2), -1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        # HEADIN
        hin = synthetic.scene_to_device(c.t, dev, K=8, seed=1, p_drop=0.2, drop_sites=L.DROP_TRUNK | L.DROP_HEADIN)
        with pytest.raises(L.UnerfError, match="HEADIN"):
            ops.pose_grad_mc(s.o, s.d, s.sb, hin.field, sc.near, sc.far)
        # an any-width field
        tw = synthetic.make_scene_tensors(seed=0, kind="mcdropout", log2T=12, prop_log2T=12, max_res=64, hidden_dim=32)
        noticed = set(ops._warned_any_width)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            wide = synthetic.scene_to_device(tw, dev, K=8, seed=1, p_drop=0.2)
        ops._warned_any_width.intersection_update(noticed)
        with pytest.raises(L.UnerfError, match="widths"):
            ops.pose_grad_mc(s.o, s.d, s.sb, wide.field, sc.near, sc.far)
        # a missing site array, a superfluous one, a pass_stride that is too small
        with pytest.raises(L.UnerfError, match="site HEAD1 is active"):
            ops.pose_grad_mc(s.o, s.d, s.sb, sc.field, sc.near, sc.far, keep_masks=ops.KeepMasks(ones, None, None, None, n, 0))
        with pytest.raises(L.UnerfError, match="site HEAD0, which is not active"):
            ops.pose_grad_mc(s.o, s.d, s.sb, sc.field, sc.near, sc.far, keep_masks=ops.KeepMasks(ones, ones, ones, None, n, 0))
        with pytest.raises(L.UnerfError, match="pass_stride"):
            ops.pose_grad_mc(s.o, s.d, s.sb, sc.field, sc.near, sc.far, keep_masks=ops.KeepMasks(ones, None, ones, None, n, 1))
        # a LAPLACE and an ACTIVE field: at the op and at the C entry point
        tl = synthetic.make_scene_tensors(seed=0, kind="laplace", log2T=12, prop_log2T=12, max_res=64)
        wsd, wsr = synthetic.laplace_weight_samples(tl, n_samples=4)
        lap = synthetic.scene_to_device(tl, dev, ws_density=wsd, ws_rgb=wsr)
        act = synthetic.scene_to_device(synthetic.make_scene_tensors(seed=0, kind="active", log2T=12, prop_log2T=12, max_res=64), dev)
        for other in (lap, act):
            with pytest.raises(L.UnerfError, match="MCDROPOUT"):
                ops.pose_grad_mc(s.o, s.d, s.sb, other.field, sc.near, sc.far)
            assert _raw_call(dev, s, s.R, grad, None, cs=other.field.cstruct()) == -1 and b"mode" in lib.unerf_last_error()
        # K = 0, S beyond a wave, Euclidean bins
        k0 = sc.field.cstruct()
        k0.K = 0
        assert _raw_call(dev, s, s.R, grad, None, cs=k0) == -1 and b"K=0" in lib.unerf_last_error()
        assert _raw_call(dev, s, s.R, grad, None, S=65) == -1 and b"S=65" in lib.unerf_last_error()
        assert _raw_call(dev, s, s.R, grad, None, near=-1.0) == -1 and b"near_plane" in lib.unerf_last_error()
        assert _raw_call(dev, s, 0, grad, None) == 0
        torch.cuda.synchronize()
        assert float(grad.abs().max()) == 0.0                     # refused before any launch


def _mc_model(dev, K=4):
    import test_gpu_models as TM
    from uncertainty_nerf_gs_amd import plugin, synthetic
    cfg = TM._small_cfg(plugin.MODEL_CONFIGS["nerfacto-mcdropout"]())
    cfg.mc_samples = K
    model = cfg._target(cfg, num_train_data=4)
    t = synthetic.make_scene_tensors(seed=2, kind="mcdropout", log2T=14, prop_log2T=12, color_contrast=10.0)
    model.load_state_dict(TM._state_dict_from_tensors(t, "mcdropout"))
    model.seed = 77
    model.invalidate()
    return model.to(dev)


@pytest.mark.parametrize("H,W", [(6, 8), (11, 24)])
def test_frame_level(dev, H, W):
    """render.pose_gradient_camera_mc in several launch groups == one group; the model's method differentiates the frame its
    last render made; another mask seed gives another gradient, the same seed the same bits"""
    from uncertainty_nerf_gs_amd import models, render, synthetic
    model = _mc_model(dev)
    model.precision = "fp32"
    c2w = synthetic.orbit_c2w(0.7)
    kw = dict(fx=20.0, fy=21.0, cx=W / 2 + 0.2, cy=H / 2 - 0.1, H=H, W=W)
    cam = SimpleNamespace(camera_to_worlds=c2w[None], fx=torch.tensor([kw["fx"]]), fy=torch.tensor([kw["fy"]]), cx=torch.tensor([kw["cx"]]),
                          cy=torch.tensor([kw["cy"]]), height=H, width=W)
    with torch.cuda.device(dev):
        scene = model.device_scene()
        one, rgb_one = render.pose_gradient_camera_mc(scene, c2w, want_rgb=True, **kw)
        many, rgb_many = render.pose_gradient_camera_mc(scene, c2w, rays_per_launch=37, want_rgb=True, **kw)
        assert one.shape == (H, W, 3, 4) and rgb_one.shape == (H, W, 3) and one.abs().max() > 0
        assert torch.equal(one, many) and torch.equal(rgb_one, rgb_many)
        # the model: two renders, then the gradient of the second one's frame
        model.get_outputs_for_camera(cam)
        frame = model.get_outputs_for_camera(cam)["rgb"]
        counter, last = model.frame_counter, scene.field.seed
        assert last == models.frame_seed(77, 1)
        got, rgb = model.get_mc_pose_gradients_for_camera(cam, rays_per_launch=50, want_rgb=True)
        assert model.frame_counter == counter and scene.field.seed == last
        assert (frame - rgb).abs().max().item() < 1e-4            # the frame just rendered (both fp32, other summation orders)
        want = render.pose_gradient_camera_mc(scene, c2w, **kw)   # scene.field.seed is that render's
        assert torch.equal(got, want)
        other = model.get_mc_pose_gradients_for_camera(cam, mask_seed=4321)
        assert scene.field.seed == last and not torch.equal(other, got)
        assert torch.equal(other, model.get_mc_pose_gradients_for_camera(cam, mask_seed=4321))
        assert torch.equal(got, model.get_mc_pose_gradients_for_camera(cam, mask_seed=last))


def test_frame_level_refusals(dev):
    from uncertainty_nerf_gs_amd import lib as L, render, synthetic
    sc = _scene(dev, "S16").scene
    c2w = synthetic.orbit_c2w(0.3)
    with torch.cuda.device(dev):
        with pytest.raises(L.UnerfError, match="ORTHOPHOTO"):
            render.pose_gradient_camera_mc(sc, c2w, 10.0, 10.0, 4.0, 3.0, 6, 8, camera_type=L.CAMERA_ORTHOPHOTO)
        with pytest.raises(L.UnerfError, match="obb"):
            render.pose_gradient_camera_mc(sc, c2w, 10.0, 10.0, 4.0, 3.0, 6, 8, obb=(torch.eye(3, 4), torch.ones(3)))
    model = _mc_model(dev)
    cam = SimpleNamespace(camera_to_worlds=c2w, fx=10.0, fy=10.0, cx=4.0, cy=3.0, height=6, width=8)
    with pytest.raises(NotImplementedError, match="colour is the mean"):
        model.get_pose_gradients_for_camera(cam)
