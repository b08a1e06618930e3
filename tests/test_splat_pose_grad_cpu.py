"""The float64 reference of the splat pose gradient (tests/splat_pose_grad_cases.py) checks itself, and the host layers of
the feature exist: no GPU, no kernel result.

  * the restated projection equals SO.project_gaussians on every live splat within fp32 rounding of the oracle's outputs;
  * central differences of the float64 frame (h = 1e-5) in each of the 12 c2w entries agree with its forward-mode gradient to
    1e-6 x rms (truncation ~h^2, rounding ~1e-16 / h), lists and decisions pinned, for an orthonormal and a sheared R;
  * the closed-form V -> c2w epilogue equals autograd through the restated viewmat_from_c2w;
  * the builders' caps hold for every case;
  * planted mutations of the recurrences fail the comparison the GPU tests make."""
import inspect

import numpy as np
import pytest

import splat_pose_grad_cases as PC
from oracle import splat_oracle as SO


def test_constants_and_surface(lib):
    from uncertainty_nerf_gs_amd import models, ops, splat
    import uncertainty_nerf_gs_amd as pkg
    assert lib.SPLAT_POSE_GRAD_BATCH == PC.B and lib.SPLAT_POSE_Q == 6
    header = open(lib.INCLUDE + "/unerf.h").read()
    assert f"#define UNERF_SPLAT_POSE_GRAD_BATCH {PC.B}\n" in header and "#define UNERF_SPLAT_POSE_Q 6\n" in header
    for name in ("unerf_splat_pose_tangents", "unerf_splat_pose_grad"):
        assert name in lib.SIGNATURES
    # two workgroups' staging records fit a CU's 160 KiB of LDS (antialiased: 3 + 18 16-byte words per record)
    assert 2 * (PC.B * 21 * 16 + PC.B * (4 + 1 + 8)) <= 160 * 1024
    assert callable(ops.splat_pose_tangents) and callable(ops.splat_pose_grad) and "splat pose" in pkg.__doc__
    sig = inspect.signature(splat.pose_gradient_camera)
    assert list(sig.parameters)[:10] == ["gp", "c2w", "fx", "fy", "cx", "cy", "H", "W", "background", "sh_degree"]
    assert sig.parameters["want_rgb"].default is False and sig.parameters["rasterize_mode"].default == "classic"
    assert "get_pose_gradients_for_camera" in vars(models.SplatfactoModel)
    assert models.ActiveSplatfactoModel.get_pose_gradients_for_camera is models.SplatfactoModel.get_pose_gradients_for_camera


def test_model_refuses_bad_cameras_before_any_launch():
    from types import SimpleNamespace
    import torch
    from uncertainty_nerf_gs_amd import plugin
    m = plugin.build_model("active-splatfacto", num_points=4)
    cam = dict(fx=10.0, fy=10.0, cx=4.0, cy=3.0, height=6, width=8)
    with pytest.raises(NotImplementedError, match="pinhole"):
        m.get_pose_gradients_for_camera(SimpleNamespace(camera_to_worlds=torch.eye(4)[:3], camera_type=2, **cam))
    with pytest.raises(ValueError, match="one camera, got a batch of 2"):
        m.get_pose_gradients_for_camera(SimpleNamespace(camera_to_worlds=torch.eye(4)[None, :3].repeat(2, 1, 1), **cam))


def test_restated_projection_equals_the_oracle():
    for name, (means, cov3d, V, pr, pins, cam) in _projections().items():
        q64, _ = PC.tangents_ref(V, means, cov3d, pins, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
        live = pr["radii"] > 0
        assert live.sum() > 100
        want = np.concatenate([pr["xys"], pr["conics"], pr["compensation"][:, None]], 1).astype(np.float64)
        # fp32 rounding of the oracle's ~40-operation chain, relative to the splat's largest entry of each kind; the compensation
        # is a square root of a difference of products: compared as its square, absolutely
        sc_xy = np.maximum(np.abs(want[:, :2]).max(1, keepdims=True), 1.0)
        sc_con = np.abs(want[:, 2:5]).max(1, keepdims=True)
        assert (np.abs(q64[:, :2] - want[:, :2])[live] <= 1e-5 * sc_xy[live]).all(), name
        assert (np.abs(q64[:, 2:5] - want[:, 2:5])[live] <= 1e-4 * sc_con[live]).all(), name
        assert (np.abs(q64[:, 5] ** 2 - want[:, 5] ** 2)[live] <= 1e-5).all(), name
        assert (q64[~live] == 0).all()


def _projections():
    tc = PC.tangent_case()
    f = PC.frame_case("antialiased")
    V = SO.viewmat_from_c2w(f.c2w)[:3]
    pins = PC.projection_pins(f.means, V, f.cam["fx"], f.cam["fy"], f.cam["H"], f.cam["W"], f.proj)
    return {"tangent": (tc.means, tc.proj["cov3d"], tc.V, tc.proj, tc.pins, tc.cam),
            "frame": (f.means, f.proj["cov3d"], V, f.proj, pins, f.cam)}


def test_tangent_case_plants():
    tc = PC.tangent_case()
    r, p, pl = tc.proj["radii"], tc.pins, tc.plants
    assert tc.N % 256 != 0
    assert r[pl["clip_on"]] == 0 and r[pl["clip_below"]] == 0 and r[pl["clip_above"]] > 0
    assert r[pl["behind"]] == 0 and r[pl["offscreen"]] == 0
    for ax, mask in (("x", p.clamp_x), ("y", p.clamp_y)):
        for s in "pm":
            assert r[pl[f"fov{ax}_{s}_on"]] > 0 and r[pl[f"fov{ax}_{s}_in"]] > 0 and r[pl[f"fov{ax}_{s}_out"]] > 0
            assert not mask[pl[f"fov{ax}_{s}_on"]] and not mask[pl[f"fov{ax}_{s}_in"]] and mask[pl[f"fov{ax}_{s}_out"]]
    assert abs(float(p.rx[pl["fovx_p_on"]])) == tc.lim_x and abs(float(p.ry[pl["fovy_m_on"]])) == tc.lim_y
    assert r[pl["needle"]] > 0 and 0 < tc.proj["compensation"][pl["needle"]] < 1e-3
    assert r[pl["flat"]] > 0 and tc.proj["compensation"][pl["flat"]] == 0
    # the clamp changes the derivative, not the value: the tangents of `on` / `in` and `out` differ in conic entries
    _, J = PC.tangents_ref(tc.V, tc.means, tc.proj["cov3d"], p, tc.cam["fx"], tc.cam["fy"], tc.cam["cx"], tc.cam["cy"])
    assert np.isfinite(J).all() and (J[r == 0] == 0).all()
    assert (J[pl["flat"], 5] == 0).all() and np.abs(J[pl["needle"], 5]).max() > 0


@pytest.mark.parametrize("sheared", [False, True])
@pytest.mark.parametrize("mode", ["classic", "antialiased"])
def test_central_differences_agree_with_the_forward_mode_gradient(mode, sheared):
    f = PC.frame_case(mode, sheared=sheared, seed=PC.FD_SEED, fd=True)
    cam = f.cam
    V = SO.viewmat_from_c2w(f.c2w)[:3]
    pins = PC.projection_pins(f.means, V, cam["fx"], cam["fy"], cam["H"], cam["W"], f.proj)
    c0 = f.c2w.astype(np.float64)
    base = PC.frame64(f, c0, pins, want_grad=True)
    keep = PC.keep_mask(base.raw)
    assert np.abs(base.grad).max() > 0
    h = 1e-5
    fd = np.zeros_like(base.grad)
    for a in range(3):
        for b in range(4):
            d = np.zeros((3, 4))
            d[a, b] = h
            fd[..., a, b] = (PC.frame64(f, c0 + d, pins, rec=base.rec).s - PC.frame64(f, c0 - d, pins, rec=base.rec).s) / (2 * h)
    err = PC.rel_error(fd, base.grad, keep)
    print(f"FD {mode} sheared={sheared}: {err:.3e}")
    assert err <= 1e-6
    if sheared:    # a true inverse would give another gradient: the transposition is what is differentiated
        Vinv = np.linalg.inv(np.vstack([c0 @ np.diag([1.0, -1, -1, 1]), [0, 0, 0, 1]]))[:3]
        assert np.abs(Vinv - PC.viewmat_t(PC.torch.as_tensor(c0)).numpy()).max() > 1e-2


def test_epilogue_closed_form_equals_autograd():
    rng = np.random.default_rng(0)
    gV = rng.standard_normal((5, 7, 12))
    for c2w in (PC.frame_c2w(False), PC.frame_c2w(True), PC.case_lists().c2w):
        a, b = PC.epilogue64(gV, c2w), PC.epilogue_autograd(gV, c2w)
        assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max()


@pytest.mark.parametrize("name", list(PC.WALK))
def test_walk_case_caps(name):
    c = PC.WALK[name]()
    assert len(c.zeroed) <= PC.MAX_ZEROED * c.N and c.rounds <= PC.MAX_ROUNDS and not np.isin(c.zeroed, c.protected).any()
    for aa in (False, True):
        for bg in ("none", "black", "color"):
            r64, r32, keep = PC.walk_ref(name, aa, bg)
            assert (~keep).sum() <= PC.MAX_PIXELS_OUT * keep.size, f"{name}: {(~keep).sum()} pixels on the colour clamp"
            assert np.isfinite(r64.gV).all() and np.abs(r64.gV[keep]).max() > 0
            assert (r64.raw >= 1).any(-1).sum() > (0.2 * keep.size if name == "bright" and bg != "none" else -1)
    if name == "lists":
        assert (PC.walk_ref(name, False, "color")[0].raw < 1).all(), "dim: no channel reaches the clamp"
    if name == "stops":
        raw = PC.blend(c.gids, c.bins, c.xys, c.conics, c.colors, c.opac, None, c.H, c.W).T
        assert (raw <= 1e-3).any(), "stoppers must end pixels"


@pytest.mark.parametrize("kw", [dict(mode="classic"), dict(mode="antialiased"), dict(mode="classic", sh0=True),
                                dict(mode="antialiased", crop=True)], ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_frame_case_caps(kw):
    f = PC.frame_case(**kw)
    ref = PC.frame_reference(f)
    assert (~ref.keep).sum() <= PC.MAX_PIXELS_OUT * ref.keep.size and np.abs(ref.grad[ref.keep]).max() > 0
    assert f.rounds <= PC.MAX_ROUNDS and len(f.zeroed) <= PC.MAX_ZEROED * len(f.gp["means"])
    if kw.get("crop"):
        assert 0 < f.crop_ids.sum() < len(f.crop_ids)


@pytest.mark.parametrize("mutation", PC.MUTATIONS)
def test_planted_mutations_fail_the_comparison(mutation):
    """each mutation of the recurrences must exceed KERNEL_FACTOR x the float32 yardstick on the case aimed at it"""
    name, aa, bg = {"no_bg_dT": ("lists", False, "color"), "no_alpha_dT": ("lists", True, "color"),
                    "clamp_grad": ("stops", False, "color"), "diff_stopped": ("stops", True, "color")}[mutation]
    c = PC.WALK[name]()
    r64, r32, keep = PC.walk_ref(name, aa, bg)
    bad = PC.blend(c.gids, c.bins, c.xys, c.conics, c.colors, c.opac, c.tan, c.H, c.W, bg=c.bg, comp=c.comp if aa else None,
                   bw=c.bw, mutate=mutation)
    e32, e_bad = PC.rel_error(r32.gV, r64.gV, keep), PC.rel_error(bad.gV, r64.gV, keep)
    print(f"MUTATION {mutation}: yardstick {e32:.3e}, mutated {e_bad:.3e}")
    assert 0 < e32 < 1e-4
    assert e_bad > PC.KERNEL_FACTOR * e32
