"""unerf_pose_jacobian on the GPU against the float64 reference of tests/pose_jac_cases.py.

Tolerance (pose_jac_cases.py): on the rays the reference keeps, the error of row c, max |J_c - J64_c| / rms(J64_c), may be
KERNEL_FACTOR = 4 x the fp32 torch oracle's own error of that row on the same rays, which every test computes itself; a row
whose rms(J64_c) is 0 must be exactly 0.  The channels' values are held to the same rule against the float64 values.  The
contraction with `proj` and its sum of squares are held to the fp32 dot-product bounds of the summation the header states.
Everything else here is bit equality: between launch sizes, channel subsets, requested outputs, streams, repeats, and with
unerf_pose_grad's colour.

Measured on MI355X (largest kernel / oracle ratio of a row over all sixteen cases): r 1.20, g 1.09,
b 1.73 (mc16), accumulation 1.22, expected_depth 2.01 (`empty`: both are rounding noise of 1 - exp(-delta sigma) at
delta sigma ~ 1e-9, 6.3e3 against 3.1e3 of the row's rms; elsewhere <= 1.17); `opaque` 0.97 / 0.99 / 1.04 / (rms 6.6e-16) / 0.96;
the 12-entry form <= 1.15; values <= 1.98 x the oracle's error (aabb r: 3.0e-7 against 1.5e-7);
|(J_r + J_g + J_b) / 3 - unerf_pose_grad| <= 1.6e-6 of the rms gradient."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import pose_grad_cases as PC
import pose_jac_cases as JC

pytestmark = pytest.mark.gpu

GUARD_VALUE = 12345.0
_SCENES = {}


def _scene(dev, name):
    from uncertainty_nerf_gs_amd import synthetic
    if name not in _SCENES:
        c = JC.case(name)
        sd = synthetic.scene_to_device(c.t, dev)
        _SCENES[name] = SimpleNamespace(scene=sd, o=c.origins.to(dev), d=c.directions.to(dev), sb=c.sbins.to(dev))
    return _SCENES[name]


def _jac(dev, name, R=None, rot_inv=None, channels=JC.CHANNELS, proj=None, want=("jac", "val")):
    from uncertainty_nerf_gs_amd import ops
    s = _scene(dev, name)
    R = JC.case(name).R if R is None else R
    sc = s.scene
    with torch.cuda.device(dev):
        out = ops.pose_jacobian(s.o[:R].contiguous(), s.d[:R].contiguous(), s.sb[:R].contiguous(), sc.field, sc.near, sc.far,
                                rot_inv=rot_inv, channels=channels, proj=proj, spacing=sc.spacing, background=sc.background,
                                want=want)
        torch.cuda.synchronize()
    return out


def _check_rows(name, got, label="", j64=None, o32=None):
    """every row within KERNEL_FACTOR x the oracle's own error of that row; -> the largest kernel / oracle ratio"""
    ref = JC.reference64(name)
    yard = JC.row_errors(JC.oracle32(name).jac if o32 is None else o32, ref, j64)
    errs = JC.row_errors(got, ref, j64)
    worst = 0.0
    for ch, ((err, rms), (y, _)) in enumerate(zip(errs, yard)):
        ratio = err / y if y > 0 else (0.0 if err == 0 else float("inf"))
        print(f"[pose_jacobian] {name}{label} {JC.CHANNELS[ch]}: kernel {err:.3e}, fp32 oracle {y:.3e}, ratio {ratio:.2f}, "
              f"rms(J64) {rms:.3e}")
        if rms == 0:
            assert err == 0.0, f"{name} row {JC.CHANNELS[ch]}: every kept ray is clamped, the row must be exactly 0"
        else:
            assert err <= JC.KERNEL_FACTOR * y, f"{name} row {JC.CHANNELS[ch]}: {err:.3e} > {JC.KERNEL_FACTOR} x {y:.3e}"
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("name", sorted(JC.CASES))
def test_matches_float64_reference(dev, name):
    """1. every case of pose_grad_cases (S in {1, 2, 16, 47, 48, 63, 64}, both trunk widths, three grid layouts, the
    backgrounds, aabb, uniform spacing) and the two plants, all five channels, D = 6"""
    c = JC.case(name)
    out = _jac(dev, name)
    assert out["jac"].shape == (c.R, 5, 6) and out["val"].shape == (c.R, 5)
    assert torch.isfinite(out["jac"]).all() and torch.isfinite(out["val"]).all()
    _check_rows(name, out["jac"])
    ref = JC.reference64(name)
    yard = JC.value_errors(JC.oracle32(name).val, ref)
    errs = JC.value_errors(out["val"], ref)
    for ch, (err, y) in enumerate(zip(errs, yard)):
        print(f"[pose_jacobian] {name} value {JC.CHANNELS[ch]}: kernel {err:.3e}, fp32 oracle {y:.3e}")
        assert err <= JC.KERNEL_FACTOR * y


@pytest.mark.parametrize("name", ["S16", "tcnn"])
def test_pose_epilogue_non_orthonormal(dev, name):
    """2. D = 12 under a sheared rotation block against pose_from_ray_grad of every float64 row"""
    c, ref, o32 = JC.case(name), JC.reference64(name), JC.oracle32(name)
    rot_inv = torch.linalg.inv(JC.sheared_rotation().double()).float()
    got = _jac(dev, name, rot_inv=rot_inv)["jac"]
    assert got.shape == (c.R, 5, 12)
    want = JC.pose_rows(ref.jac, c.directions, rot_inv)
    _check_rows(name, got, " pose", j64=want, o32=JC.pose_rows(o32.jac, c.directions, rot_inv))
    six = _jac(dev, name)["jac"]
    assert torch.equal(got.view(c.R, 5, 3, 4)[..., 3], six[..., :3])       # the origin column, bit for bit


@pytest.mark.parametrize("R", [r for r in PC.R_SUB if r != 257])
def test_launch_sizes(dev, R):
    """3. one wave, a partial block, a full block, a block and a wave: the bits of the 257-ray launch's rows"""
    want = ("jac", "val", "proj", "var")
    proj = torch.linspace(-1.0, 1.0, 6 * 5).view(6, 5)
    full = _jac(dev, "base", proj=proj, want=want)
    got = _jac(dev, "base", R=R, proj=proj, want=want)
    for k in want:
        assert torch.equal(got[k], full[k][:R]), k


def _raw(dev, name, R, bits, rot_inv, proj, which, dirty):
    """the C entry point on caller-owned buffers with JC.GUARD guard floats in front of and behind every output
    -> {output: (whole buffer, payload view)}"""
    from uncertainty_nerf_gs_amd import lib as L, ops
    s = _scene(dev, name)
    sc = s.scene
    cs = sc.field.cstruct()
    bg_mode, bg_rgb = ops._background(sc.background)
    D = 6 if rot_inv is None else 12
    Cn = bin(bits).count("1")
    ri = None if rot_inv is None else (C.c_float * 9)(*[float(v) for v in rot_inv.reshape(-1)])
    P = 0 if proj is None else proj.shape[1]
    pj = None if proj is None else (C.c_float * (D * P))(*[float(v) for v in proj.reshape(-1)])
    shapes = {"jac": (R, Cn, D), "proj": (R, Cn, P), "var": (R, Cn), "val": (R, Cn)}
    bufs, ptrs = {}, {}
    for k in ("jac", "proj", "var", "val"):
        if k not in which:
            ptrs[k] = None
            continue
        n = 1
        for v in shapes[k]:
            n *= v
        buf = torch.full((n + 2 * JC.GUARD,), float("nan") if dirty else 0.0, device=dev)
        buf[:JC.GUARD] = GUARD_VALUE
        buf[JC.GUARD + n:] = GUARD_VALUE
        bufs[k] = (buf, buf[JC.GUARD:JC.GUARD + n].view(shapes[k]))
        ptrs[k] = buf.data_ptr() + 4 * JC.GUARD
    rc = L.load().unerf_pose_jacobian(s.o.data_ptr(), s.d.data_ptr(), s.sb.data_ptr(), R, s.sb.shape[1] - 1, sc.near, sc.far,
                                      sc.spacing, C.byref(cs), bg_mode, bg_rgb, ri, bits, pj, P, ptrs["jac"], ptrs["proj"],
                                      ptrs["var"], ptrs["val"], torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.load().unerf_last_error()
    return bufs


def _guards_intact(bufs):
    for k, (buf, view) in bufs.items():
        n = view.numel()
        assert bool((buf[:JC.GUARD] == GUARD_VALUE).all()) and bool((buf[JC.GUARD + n:] == GUARD_VALUE).all()), k
        assert torch.isfinite(view).all(), k


SUBSETS = [("r",), ("g",), ("b",), ("accumulation",), ("expected_depth",), ("r", "b"), ("g", "expected_depth")]


@pytest.mark.parametrize("pose", [False, True])
def test_channel_subsets_outputs_guards_streams(dev, pose):
    """4. each single channel, {R,B}, {G,EDEPTH}, {ACC}: rows and values are the bits of the five-channel call; the jac bits
    do not depend on which other outputs are requested; guard floats around every output stay; NaN-filled buffers, a side
    stream and a second call return the same bits"""
    from uncertainty_nerf_gs_amd import ops
    name, R = "S16", 21
    rot_inv = torch.linalg.inv(JC.sheared_rotation().double()).float() if pose else None
    D = 12 if pose else 6
    proj = torch.cos(torch.arange(D * 7, dtype=torch.float32)).view(D, 7)
    with torch.cuda.device(dev):
        full = _raw(dev, name, R, 31, rot_inv, proj, ("jac", "proj", "var", "val"), dirty=True)
        torch.cuda.synchronize()
        _guards_intact(full)
        assert float(full["jac"][1].abs().max()) > 0
        via_ops = _jac(dev, name, R=R, rot_inv=rot_inv, proj=proj, want=("jac", "proj", "var", "val"))
        for k in full:
            assert torch.equal(full[k][1], via_ops[k]), k
        for names in SUBSETS:
            bits = ops.pose_channel_bits(names)
            rows = [i for i in range(5) if (bits >> i) & 1]
            sub = _raw(dev, name, R, bits, rot_inv, proj, ("jac", "proj", "var", "val"), dirty=True)
            torch.cuda.synchronize()
            _guards_intact(sub)
            for k in sub:
                assert torch.equal(sub[k][1], full[k][1][:, rows]), (names, k)
            # fewer outputs: the same bits in those that remain
            for which in (("jac",), ("val",), ("var",), ("proj", "val"), ("jac", "var")):
                part = _raw(dev, name, R, bits, rot_inv, proj if ("proj" in which or "var" in which) else None, which, dirty=False)
                torch.cuda.synchronize()
                _guards_intact(part)
                for k in which:
                    assert torch.equal(part[k][1], sub[k][1]), (names, which, k)
        # a side stream, and once more
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            again = _raw(dev, name, R, 31, rot_inv, proj, ("jac", "proj", "var", "val"), dirty=True)
        side.synchronize()
        once_more = _raw(dev, name, R, 31, rot_inv, proj, ("jac", "proj", "var", "val"), dirty=False)
        torch.cuda.synchronize()
        for other in (again, once_more):
            _guards_intact(other)
            for k in full:
                assert torch.equal(other[k][1], full[k][1]), k


@pytest.mark.parametrize("name", ["base", "mc16", "tcnn_half", "white", "random", "opaque"])
def test_ties_to_the_pose_gradient_kernel(dev, name):
    """5. the R, G, B values are unerf_pose_grad's colour bit for bit, and (J_r + J_g + J_b) / 3 lies within the sum of the two
    kernels' allowed errors of its gradient"""
    from uncertainty_nerf_gs_amd import ops
    s, c = _scene(dev, name), JC.case(name)
    sc = s.scene
    out = _jac(dev, name)
    with torch.cuda.device(dev):
        grad, rgb = ops.pose_grad(s.o, s.d, s.sb, sc.field, sc.near, sc.far, spacing=sc.spacing, background=sc.background,
                                  want_rgb=True)
        torch.cuda.synchronize()
    assert torch.equal(out["val"][:, :3], rgb)
    ref = JC.reference64(name)
    k = ref.keep
    g64 = ref.jac[:, :3].sum(1) / 3
    scale = g64[k].pow(2).mean().sqrt().item()
    yard = JC.row_errors(JC.oracle32(name).jac, ref)
    allowed_jac = sum(JC.KERNEL_FACTOR * y * rms for y, rms in yard[:3] if rms > 0) / 3 / scale
    o32_mean = JC.oracle32(name).jac[:, :3].double().sum(1) / 3
    allowed_grad = JC.KERNEL_FACTOR * (o32_mean[k] - g64[k]).abs().max().item() / scale
    mean = out["jac"][:, :3].double().cpu().sum(1) / 3
    diff = (mean[k] - grad.double().cpu()[k]).abs().max().item() / scale
    print(f"[pose_jacobian] {name}: |mean of the colour rows - pose_grad| / rms = {diff:.3e}, allowed {allowed_jac:.3e} + "
          f"{allowed_grad:.3e}")
    assert diff <= allowed_jac + allowed_grad


@pytest.mark.parametrize("P", [1, 6, 12])
@pytest.mark.parametrize("pose", [False, True])
def test_contraction_bounds(dev, pose, P):
    """6. out_proj against the float64 product of out_jac and proj, out_var against the float64 sum of out_proj^2: the fp32
    bounds of a dot product summed in order, D 2^-23 sum |jac| |proj| and (P + 2) 2^-23 sum proj^2"""
    name = "S16"
    rot_inv = torch.linalg.inv(JC.sheared_rotation().double()).float() if pose else None
    D = 12 if pose else 6
    g = torch.Generator().manual_seed(100 + P)
    proj = torch.randn(D, P, generator=g)
    out = _jac(dev, name, rot_inv=rot_inv, proj=proj, want=("jac", "proj", "var"))
    jac, pr, var = out["jac"].double().cpu(), out["proj"].double().cpu(), out["var"].double().cpu()
    assert pr.shape == (JC.case(name).R, 5, P) and var.shape == (JC.case(name).R, 5)
    want = jac @ proj.double()
    bound = D * 2.0 ** -23 * (jac.abs() @ proj.double().abs())
    assert bool(((pr - want).abs() <= bound).all()) and float(pr.abs().max()) > 0
    sq = pr.pow(2).sum(-1)
    assert bool(((var - sq).abs() <= (P + 2) * 2.0 ** -23 * sq).all())


def test_camera_through_the_model(dev):
    """7. a 16 x 12 camera through ActiveNerfactoModel: the c2w Jacobian in launch groups of 50 rays = ray kernel -> sampler
    -> unerf_pose_jacobian on all 192 rays at once, bit for bit; the se3 Jacobian = the c2w one contracted with the tangent
    basis in float64 within the bound of test 6; the pose uncertainty's keys and shapes; a zero covariance gives zero std"""
    import test_gpu_models as TM
    from uncertainty_nerf_gs_amd import ops, plugin, posegrad, render, synthetic
    cfg = TM._small_cfg(plugin.MODEL_CONFIGS["active-nerfacto"]())
    model = cfg._target(cfg, num_train_data=4)
    t = synthetic.make_scene_tensors(seed=2, kind="active", log2T=14, prop_log2T=12, color_contrast=10.0)
    model.load_state_dict(TM._state_dict_from_tensors(t, "active"))
    model = model.to(dev)
    H, W = 12, 16
    c2w = synthetic.orbit_c2w(0.7)
    cam = SimpleNamespace(camera_to_worlds=c2w[None], fx=torch.tensor([20.0]), fy=torch.tensor([21.0]), cx=torch.tensor([8.2]),
                          cy=torch.tensor([5.9]), height=H, width=W)
    with torch.cuda.device(dev):
        got = model.get_pose_jacobians_for_camera(cam, basis="c2w", rays_per_launch=50)
        assert sorted(got) == ["jacobian", "values"]
        assert got["jacobian"].shape == (H, W, 5, 12) and got["values"].shape == (H, W, 5) and got["jacobian"].dtype == torch.float32
        scene = model.device_scene()
        o, d, _ = ops.generate_rays(c2w, 20.0, 21.0, 8.2, 5.9, H, W, dev)
        sb, _ = render.sample_rays(scene, o, d, None, 0, want_prop_depth=False, image_width=W)
        want = ops.pose_jacobian(o, d, sb, scene.field, scene.near, scene.far, rot_inv=torch.linalg.inv(c2w[:, :3].double()).float(),
                                 spacing=scene.spacing, background=scene.background, want=("jac", "val"))
        torch.cuda.synchronize()
        assert torch.equal(got["jacobian"].reshape(H * W, 5, 12), want["jac"]) and got["jacobian"].abs().max() > 0
        assert torch.equal(got["values"].reshape(H * W, 5), want["val"])
        other = model.get_pose_jacobians_for_camera(cam, basis="c2w", rays_per_launch=7)
        assert torch.equal(other["jacobian"], got["jacobian"]) and torch.equal(other["values"], got["values"])
        # the six pose parameters
        se3 = model.get_pose_jacobians_for_camera(cam, rays_per_launch=64)
        assert se3["jacobian"].shape == (H, W, 5, 6) and torch.equal(se3["values"], got["values"])
        basis32 = posegrad.tangent_basis(c2w).float().double()          # the values the kernel was handed
        j12 = got["jacobian"].double().cpu()
        bound = 12 * 2.0 ** -23 * (j12.abs() @ basis32.abs())
        assert bool(((se3["jacobian"].double().cpu() - j12 @ basis32).abs() <= bound).all())
        sub = model.get_pose_jacobians_for_camera(cam, channels=("expected_depth", "g"), basis="c2w")
        assert torch.equal(sub["jacobian"], got["jacobian"][:, :, [1, 4]])
        # pose uncertainty
        unc = model.get_pose_uncertainty_for_camera(cam, torch.tensor([0.01, 0.01, 0.02, 2e-3, 1e-3, 3e-3]), rays_per_launch=50)
        assert sorted(unc) == sorted(["rgb_var_pose", "rgb_std_pose", "expected_depth_std_pose", "accumulation_std_pose", "rgb",
                                      "accumulation", "expected_depth"])
        for k, v in unc.items():
            assert v.shape == (H, W, 3 if k == "rgb" else 1) and torch.isfinite(v).all(), k
        assert torch.equal(unc["rgb"], got["values"][..., :3]) and torch.equal(unc["expected_depth"], got["values"][..., 4:5])
        assert float(unc["rgb_std_pose"].max()) > 0 and float(unc["expected_depth_std_pose"].max()) > 0
        assert torch.equal(unc["rgb_std_pose"], unc["rgb_var_pose"].sqrt())
        # against the float64 propagation of the c2w Jacobian: var_c = |J_c proj|^2, rgb_var = mean_c
        proj = posegrad.pose_projection(c2w, torch.tensor([0.01, 0.01, 0.02, 2e-3, 1e-3, 3e-3])).float().double()
        var64 = (j12 @ proj).pow(2).sum(-1)
        # |pr_k - exact_k| <= b_k = 12 2^-23 (|J| |proj|)_k and |exact_k| <= (|J| |proj|)_k: sum_k (2 |exact_k| b_k + b_k^2) <= 3 x 12 2^-23
        # sum_k (|J| |proj|)_k^2; the sum of squares (P + 2 = 8) and the mean over three channels add 12 2^-23 var
        rel = 3 * 12 * 2.0 ** -23 * (j12.abs() @ proj.abs()).pow(2).sum(-1) + 12 * 2.0 ** -23 * var64
        assert bool(((unc["rgb_var_pose"][..., 0].double().cpu() - var64[..., :3].mean(-1)).abs() <= rel[..., :3].mean(-1) + 1e-30).all())
        zero = model.get_pose_uncertainty_for_camera(cam, torch.zeros(6, 6))
        for k in ("rgb_std_pose", "rgb_var_pose", "expected_depth_std_pose", "accumulation_std_pose"):
            assert float(zero[k].abs().max()) == 0.0, k
        assert torch.equal(zero["rgb"], unc["rgb"])


def test_raising_paths(dev):
    """8. through ops, the raw call, the frame level and the models"""
    import test_gpu_models as TM
    from uncertainty_nerf_gs_amd import lib as L, ops, plugin, render, synthetic
    s = _scene(dev, "S16")
    sc = s.scene
    with torch.cuda.device(dev):
        tl = synthetic.make_scene_tensors(seed=0, kind="laplace", log2T=12, prop_log2T=12, max_res=64)
        wsd, wsr = synthetic.laplace_weight_samples(tl, n_samples=4)
        lap = synthetic.scene_to_device(tl, dev, ws_density=wsd, ws_rgb=wsr)
        with pytest.raises(L.UnerfError, match="not built for the Laplace field"):
            ops.pose_jacobian(s.o, s.d, s.sb, lap.field, sc.near, sc.far)
        for kw, text in ((dict(channels=()), "empty"), (dict(channels=("r", "alpha")), "expected some of"),
                         (dict(want=("jac", "hessian")), "want="), (dict(want=("var",)), "need proj"),
                         (dict(proj=torch.zeros(12, 3)), r"proj must be \[6,P\]"), (dict(proj=torch.zeros(6, 13), want=("proj",)), "P=13"),
                         (dict(rot_inv=torch.eye(4)), "rot_inv"), (dict(background=(7, None)), "background")):
            with pytest.raises(L.UnerfError, match=text):
                ops.pose_jacobian(s.o, s.d, s.sb, sc.field, sc.near, sc.far, **kw)
        lib = L.load()
        out = torch.zeros(4 * 5 * 6, device=dev)
        ok = sc.field.cstruct()

        def raw(cs_, S=16, near=sc.near, channels=31, proj=None, P=0, outs=None, R=4):
            outs = (out.data_ptr(), None, None, None) if outs is None else outs
            return lib.unerf_pose_jacobian(s.o.data_ptr(), s.d.data_ptr(), s.sb.data_ptr(), R, S, near, sc.far, 0, C.byref(cs_), 0, None,
                                           None, channels, proj, P, *outs, 0)

        assert raw(lap.field.cstruct()) == -1 and b"pose_jacobian: mode" in lib.unerf_last_error()
        assert raw(ok, S=65) == -1 and b"S=65" in lib.unerf_last_error()
        assert raw(ok, near=-1.0) == -1 and b"near_plane" in lib.unerf_last_error()
        assert raw(ok, channels=0) == -1 and b"channels is empty" in lib.unerf_last_error()
        assert raw(ok, channels=64) == -1 and b"unknown bits" in lib.unerf_last_error()
        assert raw(ok, proj=(C.c_float * 144)(), P=13) == -1 and b"P=13" in lib.unerf_last_error()
        assert raw(ok, outs=(None, out.data_ptr(), None, None)) == -1 and b"need proj" in lib.unerf_last_error()
        assert raw(ok, outs=(None, None, None, None)) == -1 and b"no output requested" in lib.unerf_last_error()
        torch.cuda.synchronize()
        assert float(out.abs().max()) == 0.0                     # refused before any launch
        assert raw(ok, R=0) == 0
        c2w = synthetic.orbit_c2w(0.3)
        with pytest.raises(L.UnerfError, match="ORTHOPHOTO"):
            render.pose_jacobian_camera(sc, c2w, 10.0, 10.0, 4.0, 3.0, 6, 8, camera_type=L.CAMERA_ORTHOPHOTO)
        with pytest.raises(L.UnerfError, match="obb"):
            render.pose_jacobian_camera(sc, c2w, 10.0, 10.0, 4.0, 3.0, 6, 8, obb=(torch.eye(3, 4), torch.ones(3)))
    cam = SimpleNamespace(camera_to_worlds=c2w, fx=10.0, fy=10.0, cx=4.0, cy=3.0, height=6, width=8)
    from uncertainty_nerf_gs_amd import models
    splat_model = SimpleNamespace(get_pose_jacobians_for_camera=lambda cam_: models.SplatfactoModel.get_pose_jacobians_for_camera(None, cam_),
                                  get_pose_uncertainty_for_camera=lambda cam_, cov: models.SplatfactoModel.get_pose_uncertainty_for_camera(None, cam_, cov))
    for method in ("nerfacto-mcdropout", "nerfacto-laplace", "splat"):
        if method == "splat":
            model = splat_model
        else:
            cfg = TM._small_cfg(plugin.MODEL_CONFIGS[method]())
            model = cfg._target(cfg, num_train_data=2)
        with pytest.raises(NotImplementedError, match="not built for"):
            model.get_pose_jacobians_for_camera(cam)
        with pytest.raises(NotImplementedError, match="not built for"):
            model.get_pose_uncertainty_for_camera(cam, torch.zeros(6))
