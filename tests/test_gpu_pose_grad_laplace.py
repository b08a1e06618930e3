"""unerf_pose_grad_laplace on the GPU against the float64 reference of tests/pose_grad_laplace_cases.py, the [R,12] form under a
sheared rotation block, launch geometry, per-chunk sample sets, repeatability, refusals, and the frame-level entry points.

Tolerance (pose_grad_laplace_cases.py): on the rays the reference keeps, max |g - g64| / rms(g64) may be KERNEL_FACTOR = 4 x the
fp32 torch oracle's own error, which every test computes itself; out_rgb 4 x the oracle's + 2^-23.

Measured on MI355X (kernel error / oracle error relative to the case's RMS gradient), DESIGN.md 4.6a:
  S1 0.83e-5 / 0.83e-5, S2 1.49e-5 / 1.41e-5, S16 1.14e-5 / 1.14e-5, S47 0.58e-5 / 0.46e-5 (the largest ratio, 1.26), S48 0.60e-5 /
  0.53e-5, S63 0.56e-5 / 0.56e-5, S64 0.58e-5 / 0.63e-5, n1 1.18e-5 / 1.18e-5, n3_0 1.30e-5 / 1.28e-5, n5_7 0.59e-5 / 0.58e-5, softplus
  0.65e-5 / 0.67e-5, mask 1.15e-5 / 1.19e-5, mean_mask 1.18e-5 / 1.25e-5, tcnn 0.74e-5 / 0.81e-5, tcnn_half 0.64e-5 / 0.75e-5, white
  0.59e-5 / 0.60e-5, random 1.32e-5 / 1.25e-5, uniform 1.01e-5 / 0.89e-5, box 1.49e-5 / 1.49e-5, box_mask 1.29e-5 / 1.35e-5, gate
  1.60e-5 / 1.58e-5, gate16 0.76e-5 / 0.80e-5, stack 0.51e-5 / 0.73e-5; the 12-entry pose form S16 1.61e-5 / 1.53e-5, tcnn 1.01e-5 /
  1.07e-5, stack 0.66e-5 / 0.92e-5; out_rgb <= 5.9e-7 (oracle 5.8e-7); frame rgb against the kernel's 2.4e-7.
  (The sampler of the case builder runs on the host CPU, so shares and figures differ in the third digit between machines.)"""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import pose_grad_cases as PC
import pose_grad_laplace_cases as LC

pytestmark = pytest.mark.gpu

GUARD = 12345.0
_SCENES = {}


def _scene(dev, name, only_set=None):
    """the case's scene (field with the case's rows, activation, mask flag and set stack; only_set: that one set alone, with
    lap_chunk_rays = 0) and rays on the device"""
    from uncertainty_nerf_gs_amd import synthetic
    s = LC.spec(name)
    key = (name, only_set)
    if key not in _SCENES:
        stacked = s.chunk > 0 and only_set is None
        k = 0 if only_set is None else only_set
        kw = dict(ws_density=s.ws_density if stacked else s.ws_density[k], ws_rgb=s.ws_rgb if stacked else s.ws_rgb[k],
                  lap_softplus=int(s.softplus), lap_mask_density=int(s.mask))
        if stacked:
            kw["lap_chunk_rays"] = s.chunk
        sd = synthetic.scene_to_device(s.c.t, dev, **kw)
        _SCENES[key] = SimpleNamespace(scene=sd, o=s.c.origins.to(dev), d=s.c.directions.to(dev), sb=s.c.sbins.to(dev), S=s.c.S, R=s.c.R,
                                       offset=s.offset if stacked else 0)
    return _SCENES[key]


def _grad(dev, s, r0=0, R=None, **kw):
    from uncertainty_nerf_gs_amd import ops
    R = s.R - r0 if R is None else R
    sc = s.scene
    kw.setdefault("ray_offset", s.offset + r0)
    with torch.cuda.device(dev):
        out = ops.pose_grad_laplace(s.o[r0:r0 + R].contiguous(), s.d[r0:r0 + R].contiguous(), s.sb[r0:r0 + R].contiguous(), sc.field,
                                    sc.near, sc.far, spacing=sc.spacing, background=sc.background, **kw)
        torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_matches_float64_reference(dev, name):
    """every case: S in {1, 2, 16, 47, 48, 63, 64}, rows (1, 1), (3, 0), (5, 7), (100, 100), softplus, lap_mask_density, both
    grid layouts and the half-stored one, the backgrounds, uniform spacing, the scene box with and without the mask, the stack"""
    s = _scene(dev, name)
    got, rgb = _grad(dev, s, want_rgb=True)
    assert got.shape == (s.R, 6) and rgb.shape == (s.R, 3) and torch.isfinite(got).all()
    ref, o32 = LC.reference64(name), LC.oracle32(name)
    yard, err = LC.rel_error(o32.grad, ref), LC.rel_error(got.cpu(), ref)
    rgb_yard = (o32.rgb.double() - ref.rgb).abs().max().item()
    rgb_err = (rgb.cpu().double() - ref.rgb).abs().max().item()
    print(f"[pose_grad_laplace] {name}: kernel {err:.3e}, fp32 oracle {yard:.3e}, ratio {err / yard:.2f}, "
          f"{1 - ref.keep.double().mean().item():.3f} left out; rgb kernel {rgb_err:.3e}, oracle {rgb_yard:.3e}")
    assert err <= LC.KERNEL_FACTOR * yard
    assert rgb_err <= LC.KERNEL_FACTOR * rgb_yard + 2.0 ** -23


@pytest.mark.parametrize("name", ["S16", "tcnn", "stack"])
def test_pose_epilogue_sheared(dev, name):
    """rot_inv of a scaled, sheared rotation block: [R,12] = P (R^-1 d) | g_o of the float64 reference; its origin column is
    the six-column launch's, bit for bit"""
    s, c, ref, o32 = _scene(dev, name), LC.spec(name).c, LC.reference64(name), LC.oracle32(name)
    g = torch.Generator().manual_seed(11)
    rot = c.c2w[:, :3].double() @ (torch.eye(3, dtype=torch.float64) * 1.6 + 0.25 * torch.randn(3, 3, generator=g, dtype=torch.float64))
    rot_inv = torch.linalg.inv(rot).float()
    got = _grad(dev, s, rot_inv=rot_inv)
    assert got.shape == (c.R, 12)
    want = PC.pose_from_ray_grad(ref.grad, c.directions, rot_inv).reshape(c.R, 12)
    yard = LC.rel_error(PC.pose_from_ray_grad(o32.grad, c.directions, rot_inv).reshape(c.R, 12), ref, want)
    err = LC.rel_error(got.cpu(), ref, want)
    print(f"[pose_grad_laplace] {name} pose: kernel {err:.3e}, fp32 oracle {yard:.3e}, ratio {err / yard:.2f}")
    assert err <= LC.KERNEL_FACTOR * yard
    assert torch.equal(got.view(c.R, 3, 4)[:, :, 3], _grad(dev, s)[:, :3])


@pytest.mark.parametrize("r0", [0, 62, 252])
@pytest.mark.parametrize("R", [r for r in LC.R_SUB if r < 257])
def test_launch_sizes(dev, R, r0):
    """R rays of the 257-ray case from ray r0 on, launched with ray_offset = r0, return the bits of the full launch's rows: one
    wave, a partial block, a full block, one more; r0 = 62 puts a set border (ray 64) inside the sub-launch's first block"""
    s = _scene(dev, "base")
    full = _grad(dev, s, want_rgb=True)
    assert full[0].shape == (257, 6) and torch.isfinite(full[0]).all() and full[0].abs().max() > 0
    got = _grad(dev, s, r0=r0, R=R, want_rgb=True)
    assert torch.equal(got[0], full[0][r0:r0 + R]) and torch.equal(got[1], full[1][r0:r0 + R])
    if r0 == 62 and R >= 3:     # the offset names the set: without it rays 64.. would read set 0
        assert not torch.equal(_grad(dev, s, r0=r0, R=R, ray_offset=0), full[0][r0:r0 + R])


def test_stack_rows_are_the_single_set_calls(dev):
    """lap_chunk_rays = 6, ray_offset = 4, R = 21, five sets: every ray's bits are those of a call that is given only that
    ray's set, with lap_chunk_rays = 0"""
    s = _scene(dev, "stack")
    sets = LC.ray_sets(LC.spec("stack"))
    got, rgb = _grad(dev, s, want_rgb=True)
    seen = set()
    for k in range(LC.spec("stack").sets):
        one, rgb_one = _grad(dev, _scene(dev, "stack", only_set=k), want_rgb=True)
        rows = torch.nonzero(sets == k).flatten().to(got.device)
        assert rows.numel() > 0
        assert torch.equal(got[rows], one[rows]) and torch.equal(rgb[rows], rgb_one[rows])
        others = torch.nonzero(sets != k).flatten().to(got.device)
        assert not torch.equal(got[others], one[others])
        seen.add(k)
    assert seen == {0, 1, 2, 3, 4}


def _raw_call(dev, s, R, grad, rgb, rot_inv=None, cs=None, S=None, near=None, offset=0):
    """the C entry point on caller-owned buffers"""
    from uncertainty_nerf_gs_amd import lib as L, ops
    sc = s.scene
    cs = sc.field.cstruct() if cs is None else cs
    bg_mode, bg_rgb = ops._background(sc.background)
    ri = None if rot_inv is None else (C.c_float * 9)(*[float(v) for v in rot_inv.reshape(-1)])
    return L.load().unerf_pose_grad_laplace(s.o.data_ptr(), s.d.data_ptr(), s.sb.data_ptr(), R, s.S if S is None else S,
                                            sc.near if near is None else near, sc.far, sc.spacing, offset, C.byref(cs), bg_mode, bg_rgb,
                                            ri, grad.data_ptr(), None if rgb is None else rgb.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("pose", [False, True])
def test_guard_rows_dirty_outputs_streams_and_repeats(dev, pose):
    """R = 5 of the 257-ray case into NaN-filled buffers with guard rows behind the last ray; again; again on a side stream:
    the same bits, the guard rows keep theirs; out_rgb = NULL gives the same gradient"""
    s, R = _scene(dev, "base"), 5
    cols = 12 if pose else 6
    rot_inv = torch.linalg.inv(LC.spec("base").c.c2w[:, :3].double()).float() if pose else None
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
    """on real device pointers: another mode at the op and at the C entry point, a set past the stack, S beyond a wave,
    Euclidean bins -- nothing is launched, and unerf_pose_grad keeps refusing the Laplace field"""
    from uncertainty_nerf_gs_amd import lib as L, ops, synthetic
    s = _scene(dev, "stack")
    sc = s.scene
    lib = L.load()
    grad = torch.zeros(s.R, 6, device=dev)
    with torch.cuda.device(dev):
        act = synthetic.scene_to_device(synthetic.make_scene_tensors(seed=0, kind="active", log2T=12, prop_log2T=12, max_res=64), dev)
        with pytest.raises(L.UnerfError, match="LAPLACE"):
            ops.pose_grad_laplace(s.o, s.d, s.sb, act.field, sc.near, sc.far)
        assert _raw_call(dev, s, s.R, grad, None, cs=act.field.cstruct()) == -1 and b"pose_grad_laplace: mode" in lib.unerf_last_error()
        with pytest.raises(L.UnerfError, match="sampled heads are not differentiated"):
            ops.pose_grad(s.o, s.d, s.sb, sc.field, sc.near, sc.far)
        assert _raw_call(dev, s, s.R, grad, None, offset=10) == -1 and b"lap_sets=5" in lib.unerf_last_error()      # ray 30: set 5
        assert _raw_call(dev, s, s.R, grad, None, offset=-1) == -1 and b"ray_offset=-1" in lib.unerf_last_error()
        assert _raw_call(dev, s, s.R, grad, None, S=65) == -1 and b"S=65" in lib.unerf_last_error()
        assert _raw_call(dev, s, s.R, grad, None, near=-1.0) == -1 and b"near_plane" in lib.unerf_last_error()
        assert _raw_call(dev, s, 0, grad, None) == 0
        torch.cuda.synchronize()
        assert float(grad.abs().max()) == 0.0                     # refused before any launch
        assert _raw_call(dev, s, s.R, grad, None, offset=9) == 0  # ray 29: the last row of the last set
        torch.cuda.synchronize()
        assert float(grad.abs().max()) > 0.0


def _laplace_model(dev, chunk=64):
    import test_gpu_models as TM
    from uncertainty_nerf_gs_amd import plugin, synthetic
    cfg = TM._small_cfg(plugin.MODEL_CONFIGS["nerfacto-laplace"]())
    cfg.eval_num_rays_per_chunk = chunk
    model = cfg._target(cfg, num_train_data=4)
    t = synthetic.make_scene_tensors(seed=4, kind="laplace", log2T=14, prop_log2T=12, color_contrast=10.0)
    model.load_state_dict(TM._state_dict_from_tensors(t, "laplace"))
    g = torch.Generator().manual_seed(5)
    model.field.mlp_density_ggn = torch.rand(65, generator=g) * 1e3
    model.field.mlp_rgb_ggn = torch.rand(195, generator=g) * 1e3
    model.invalidate()
    return model            # (on the host, as the generator of the draws: the device copies are the model's own business)


@pytest.mark.parametrize("deterministic", [False, True])
def test_frame_level(dev, deterministic):
    """the model's method describes the frame get_outputs_for_camera_unc renders from an equally seeded generator (11 x 24 =
    264 rays in chunks of 64: five sets), whatever rays_per_launch is; another seed gives another gradient; the model is left
    with its mean heads"""
    model = _laplace_model(dev)
    H, W = 11, 24
    from uncertainty_nerf_gs_amd import synthetic
    c2w = synthetic.orbit_c2w(0.7)
    cam = SimpleNamespace(camera_to_worlds=c2w[None], fx=torch.tensor([20.0]), fy=torch.tensor([21.0]), cx=torch.tensor([W / 2 + 0.2]),
                          cy=torch.tensor([H / 2 - 0.1]), height=H, width=W)
    kw = dict(use_deterministic_density=deterministic, n_samples=9)
    with torch.cuda.device(dev):
        frame = model.get_outputs_for_camera_unc(cam, generator=torch.Generator().manual_seed(9), **kw)["rgb"]
        assert model._ws is None
        got, rgb = model.get_laplace_pose_gradients_for_camera(cam, generator=torch.Generator().manual_seed(9), rays_per_launch=50,
                                                               want_rgb=True, **kw)
        assert model._ws is None and model._deterministic_density is False
        assert got.shape == (H, W, 3, 4) and rgb.shape == (H, W, 3) and torch.isfinite(got).all() and got.abs().max() > 0
        worst = (frame - rgb).abs().max().item()
        print(f"[pose_grad_laplace] frame (deterministic density {deterministic}): |frame rgb - kernel rgb| = {worst:.2e}")
        assert worst < 1e-4               # the frame renders in split-f16, the gradient kernel in fp32
        one, rgb_one = model.get_laplace_pose_gradients_for_camera(cam, generator=torch.Generator().manual_seed(9),
                                                                   rays_per_launch=1 << 20, want_rgb=True, **kw)
        assert torch.equal(one, got) and torch.equal(rgb_one, rgb)
        other = model.get_laplace_pose_gradients_for_camera(cam, generator=torch.Generator().manual_seed(10), **kw)
        assert not torch.equal(other, got)
        # explicit rows: the same draw made by hand
        n_sets = -(-(H * W) // 64)
        rows = model.field.sample_last_layers(n_samples=9, generator=torch.Generator().manual_seed(9),
                                              deterministic_density=deterministic, n_sets=n_sets)
        assert rows[0].shape[0] == n_sets == 5
        by_rows = model.get_laplace_pose_gradients_for_camera(cam, weight_samples=rows, use_deterministic_density=deterministic)
        assert torch.equal(by_rows, got)
        # afterwards the model renders with its mean heads again
        plain = model.get_outputs_for_camera(cam)["rgb"]
        assert torch.isfinite(plain).all() and model._ws is None


def test_frame_level_refusals(dev):
    from uncertainty_nerf_gs_amd import lib as L, render, synthetic
    sc = _scene(dev, "n5_7").scene
    c2w = synthetic.orbit_c2w(0.3)
    with torch.cuda.device(dev):
        with pytest.raises(L.UnerfError, match="ORTHOPHOTO"):
            render.pose_gradient_camera_laplace(sc, c2w, 10.0, 10.0, 4.0, 3.0, 6, 8, camera_type=L.CAMERA_ORTHOPHOTO)
        with pytest.raises(L.UnerfError, match="obb"):
            render.pose_gradient_camera_laplace(sc, c2w, 10.0, 10.0, 4.0, 3.0, 6, 8, obb=(torch.eye(3, 4), torch.ones(3)))
        act = synthetic.scene_to_device(synthetic.make_scene_tensors(seed=0, kind="active", log2T=12, prop_log2T=12, max_res=64), dev)
        with pytest.raises(L.UnerfError, match="not a LAPLACE field"):
            render.pose_gradient_camera_laplace(act, c2w, 10.0, 10.0, 4.0, 3.0, 6, 8)
    model = _laplace_model(dev)
    cam = SimpleNamespace(camera_to_worlds=c2w, fx=10.0, fy=10.0, cx=4.0, cy=3.0, height=6, width=8)
    with pytest.raises(NotImplementedError, match="colour is the mean"):
        model.get_pose_gradients_for_camera(cam)
