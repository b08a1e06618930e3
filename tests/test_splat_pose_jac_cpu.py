"""The float64 reference of the splat pose Jacobian (tests/splat_pose_jac_cases.py) checks itself, and the host layers of the
feature exist: no GPU, no kernel result.

  * the two entry points are declared, bound and refuse bad arguments before any launch;
  * posegrad.viewmat_jacobian equals autograd through the restated viewmat_from_c2w for an orthonormal and a sheared R;
  * central differences of the float64 frame (h = 1e-5) in the six se3 parameters agree with its rows for every channel to
    1e-6 x rms (the bound DESIGN.md 4.6b uses for the gradient's self-check), lists and decisions pinned;
  * the builders' caps hold for every case, and every pixel with A > 0 has A >= 1/255;
  * planted mutations fail the comparison the GPU tests make;
  * the model methods' host-side shape, key and fill logic, with splat.pose_jacobian_camera replaced."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import splat_pose_grad_cases as SPG
import splat_pose_jac_cases as JC
from conftest import ROOT
from oracle import splat_oracle as SO


# ---------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_and_bound(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "unerf.h")).read(), flags=re.S)
    for name, n_args in (("unerf_splat_pose_tangents_proj", 8), ("unerf_splat_pose_jacobian", 20)):
        m = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/unerf.h"
        assert name in lib.SIGNATURES
        assert len(lib.SIGNATURES[name][1]) == len([a for a in m.group(1).split(",") if a.strip()]) == n_args
        assert getattr(lib.load(), name) is not None
    assert lib.load().unerf_version() == 1420          # additive: same ABI version
    assert re.search(r"#define\s+UNERF_SPLAT_POSE_PROJ_ROWS\s+7\b", header) and lib.SPLAT_POSE_PROJ_ROWS == 7
    assert re.search(r"#define\s+UNERF_SPLAT_POSE_PW\(P\)\s+\(\(P\) <= 6 \? 6 : 12\)", header)
    assert [lib.splat_pose_pw(P) for P in (1, 5, 6, 7, 12)] == [6, 6, 6, 12, 12]
    # the widest record set and the lists fit a third of a CU's 160 KiB of LDS (antialiased, 12 wide: 3 + 21 16-byte words)
    assert 3 * (SPG.B * 24 * 16 + SPG.B * (4 + 1 + 8)) <= 160 * 1024


def test_refusals_come_before_any_launch(lib):
    h = lib.load()
    proj = (C.c_float * 144)()

    def jac(ptr=1, ptan=16, P=6, H=8, W=8, bw=16, flags=0, channels=31, outs=(1, None, None)):
        return h.unerf_splat_pose_jacobian(ptr, ptr, ptr, ptr, ptr, ptr, ptr, None, ptan, None, P, H, W, bw, flags, channels,
                                           *outs, None)

    def refused(text, **kw):
        assert jac(**kw) == -1
        assert text in h.unerf_last_error(), h.unerf_last_error()

    refused(b"splat_pose_jacobian: null pointer", ptr=None)
    refused(b"splat_pose_jacobian: null pointer", ptan=None)
    refused(b"splat_pose_jacobian: P=0 outside [1,12]", P=0)
    refused(b"splat_pose_jacobian: P=13 outside [1,12]", P=13)
    refused(b"splat_pose_jacobian: channels is empty", channels=0)
    refused(b"splat_pose_jacobian: unknown channel bits 32", channels=33)
    refused(b"splat_pose_jacobian: no output asked for", outs=(None, None, None))
    refused(b"splat_pose_jacobian: unknown flags 2", flags=2)
    refused(b"splat_pose_jacobian: block_width=17 outside [1,16]", bw=17)
    refused(b"splat_pose_jacobian: block_width=0 outside [1,16]", bw=0)
    refused(b"splat_pose_jacobian: ptangents must be 8-byte aligned for P=6", ptan=4)
    refused(b"splat_pose_jacobian: ptangents must be 16-byte aligned for P=7", ptan=8, P=7)
    assert jac(H=0) == 0 and jac(W=0, outs=(None, 1, 1)) == 0        # no pixels: not an error, nothing launched

    def con(ptr=1, out=16, P=6, N=5, pj=proj):
        return h.unerf_splat_pose_tangents_proj(ptr and 16, ptr, ptr, N, pj, P, out, None)

    for text, kw in ((b"splat_pose_tangents_proj: null pointer", dict(ptr=None)), (b"splat_pose_tangents_proj: null pointer", dict(pj=None)),
                     (b"splat_pose_tangents_proj: P=0 outside [1,12]", dict(P=0)), (b"splat_pose_tangents_proj: P=13 outside [1,12]", dict(P=13)),
                     (b"ptangents must be 8-byte aligned", dict(out=4)), (b"ptangents must be 16-byte aligned", dict(out=8, P=12))):
        assert con(**kw) == -1
        assert text in h.unerf_last_error(), h.unerf_last_error()
    assert con(N=0, ptr=None, out=None) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the pose map and the reference's self-check
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sheared", [False, True])
def test_viewmat_jacobian_equals_autograd(sheared):
    from uncertainty_nerf_gs_amd import posegrad
    c2w = SPG.frame_c2w(sheared)
    got = posegrad.viewmat_jacobian(torch.from_numpy(c2w))
    assert got.shape == (12, 12) and got.dtype == torch.float64
    want = JC.viewmat_jacobian_autograd(c2w)
    assert np.abs(got.numpy() - want).max() <= 1e-12
    assert np.abs(posegrad.viewmat_jacobian(torch.from_numpy(c2w)[None]).numpy() - want).max() <= 1e-12
    if sheared:    # an inverse would give another map
        Vinv = np.linalg.inv(np.vstack([c2w.astype(np.float64) @ np.diag([1.0, -1, -1, 1]), [0, 0, 0, 1]]))[:3]
        assert np.abs(Vinv - SPG.viewmat_t(torch.as_tensor(c2w.astype(np.float64))).numpy()).max() > 1e-2


@pytest.mark.parametrize("sheared", [False, True])
@pytest.mark.parametrize("mode", ["classic", "antialiased"])
def test_central_differences_in_the_six_pose_parameters(mode, sheared):
    from uncertainty_nerf_gs_amd import posegrad
    f = SPG.frame_case(mode, sheared=sheared, seed=SPG.FD_SEED, fd=True)
    cam = f.cam
    V = SO.viewmat_from_c2w(f.c2w)[:3]
    pins = SPG.projection_pins(f.means, V, cam["fx"], cam["fy"], cam["H"], cam["W"], f.proj)
    c0 = torch.from_numpy(f.c2w.astype(np.float64))
    base = JC.frame_jac64(f, c0.numpy(), pins, want_jac=True)
    keep = SPG.keep_mask(base.raw)
    se3 = base.rows @ posegrad.tangent_basis(c0).numpy()                    # [H,W,5,6]
    h = 1e-5
    fd = np.zeros_like(se3)
    for k in range(6):
        xi = torch.zeros(1, 6, dtype=torch.float64)
        vals = []
        for s in (h, -h):
            xi[0, k] = s
            c = posegrad.pose_multiply(c0, posegrad.exp_map_se3(xi)[0]).numpy()
            vals.append(JC.frame_jac64(f, c, pins, rec=base.rec).val)
        fd[..., k] = (vals[0] - vals[1]) / (2 * h)
    err = JC.channel_errors(fd, se3, keep)
    print(f"FD {mode} sheared={sheared}: " + " ".join(f"{n}={e:.3e}" for n, e in zip(JC.CHANNELS, err)))
    assert (np.abs(se3[keep]).max((0, 2)) > 0).all(), "every channel moves"
    assert (err <= 1e-6).all()


# ---------------------------------------------------------------------------------------------------------------------
# caps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SPG.WALK))
def test_walk_case_caps(name):
    c = SPG.WALK[name]()
    assert len(c.zeroed) <= SPG.MAX_ZEROED * c.N and c.rounds <= SPG.MAX_ROUNDS
    for aa in (False, True):
        for bg in ("none", "color"):
            r64, r32, keep = JC.walk_ref(name, aa, bg)
            assert (~keep).sum() <= SPG.MAX_PIXELS_OUT * keep.size, f"{name}: {(~keep).sum()} pixels on the colour clamp"
            assert np.isfinite(r64.rows).all() and (np.abs(r64.rows[keep]).max((0, 2)) > 0).all()
            A = r64.val[..., 3]
            assert (A[A > 0] >= JC.A_MIN * (1 - 1e-12)).all(), "a blended alpha is at least 1/255"
            assert (r64.val[..., 4][A == 0] == 0).all() and (r64.rows[..., 4, :][A == 0] == 0).all()
            assert JC.within(f"{name} float32", r32.rows, r64.rows, r32.rows, keep, factor=1.0, verbose=False)
    if name in ("lists", "bw8"):
        assert (JC.walk_ref(name, False, "none")[0].val[..., 3] == 0).any(), "the empty list's tile has A == 0 pixels"


@pytest.mark.parametrize("kw", [dict(mode="classic"), dict(mode="antialiased"), dict(mode="classic", sh0=True),
                                dict(mode="antialiased", crop=True), dict(mode="classic", sheared=True)],
                         ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_frame_case_caps(kw):
    f = SPG.frame_case(**kw)
    ref = JC.frame_jac_reference(f)
    assert (~ref.keep).sum() <= SPG.MAX_PIXELS_OUT * ref.keep.size and (np.abs(ref.rows[ref.keep]).max((0, 2)) > 0).all()
    assert f.rounds <= SPG.MAX_ROUNDS and len(f.zeroed) <= SPG.MAX_ZEROED * len(f.gp["means"])
    assert (ref.A[ref.A > 0] >= JC.A_MIN * (1 - 1e-12)).all()
    # the colour rows average to the pose gradient's reference
    g = SPG.frame_reference(f)
    assert np.abs(ref.rows[..., :3, :].mean(-2).reshape(g.grad.shape) - g.grad)[ref.keep].max() <= 1e-10 * np.abs(g.grad).max()


# ---------------------------------------------------------------------------------------------------------------------
# mutations
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutation", JC.MUTATIONS)
def test_planted_mutations_fail_the_comparison(mutation):
    """each mutation must exceed KERNEL_FACTOR x the float32 yardstick on the case aimed at it"""
    if mutation == "proj_transposed":
        tc = SPG.tangent_case()
        cam = tc.cam
        _, J = SPG.tangents_ref(tc.V, tc.means, tc.proj["cov3d"], tc.pins, cam["fx"], cam["fy"], cam["cx"], cam["cy"], torch.float32)
        M = np.random.default_rng(5).standard_normal((12, 12)).astype(np.float32)
        live = tc.proj["radii"] > 0
        a = (J, tc.means, live, M)
        r64, r32, bad = JC.contract(*a), JC.contract(*a, dtype=np.float32), JC.contract(*a, mutate=mutation)
        rows = tuple(f"row{q}" for q in range(7))
        assert JC.within("contraction float32", r32, r64, r32, live, factor=1.0, channels=rows)
        assert not JC.within(f"MUTATION {mutation}", bad, r64, r32, live, channels=rows)
        return
    name, aa = {"no_zdot": ("lists", True), "no_quot_dT": ("stops", False), "acc_sign": ("lists", False),
                "no_live_gate": ("bright", True)}[mutation]
    c, w = SPG.WALK[name](), JC.walk_inputs(name)
    r64, r32, keep = JC.walk_ref(name, aa, "color")
    bad = JC.blend_jac(c.gids, c.bins, c.xys, c.conics, c.colors, w.z, c.opac, w.ptan, c.H, c.W, bg=c.bg, comp=c.comp if aa else None,
                       bw=c.bw, mutate=mutation)
    assert JC.within(f"{name} float32", r32.rows, r64.rows, r32.rows, keep, factor=1.0)
    assert not JC.within(f"MUTATION {mutation}", bad.rows, r64.rows, r32.rows, keep)


# ---------------------------------------------------------------------------------------------------------------------
# model layers, splat.pose_jacobian_camera replaced
# ---------------------------------------------------------------------------------------------------------------------
def test_surface():
    import uncertainty_nerf_gs_amd as pkg
    from uncertainty_nerf_gs_amd import models, ops, plugin, splat
    import inspect
    assert callable(ops.splat_pose_tangents_proj) and callable(ops.splat_pose_jacobian) and "splat pose Jacobian" in pkg.__doc__
    sig = inspect.signature(splat.pose_jacobian_camera)
    assert list(sig.parameters)[:12] == ["gp", "c2w", "fx", "fy", "cx", "cy", "H", "W", "background", "proj", "channels", "want"]
    assert sig.parameters["proj"].default is None and sig.parameters["want"].default == ("proj", "val")
    assert sig.parameters["channels"].default == ops.POSE_CHANNELS
    for name in ("get_splat_pose_jacobians_for_camera", "get_splat_pose_uncertainty_for_camera"):
        assert name in vars(models.SplatfactoModel)
        assert getattr(models.ActiveSplatfactoModel, name) is getattr(models.SplatfactoModel, name)
    for method in ("active-splatfacto", "splatfacto"):
        m = plugin.build_model(method, num_points=4)
        for name in ("get_splat_pose_jacobians_for_camera", "get_splat_pose_uncertainty_for_camera"):
            assert callable(getattr(m, name))
        # the NeRF models' names keep raising on the splat models
        with pytest.raises(NotImplementedError, match="not built for"):
            m.get_pose_jacobians_for_camera(SimpleNamespace())
        with pytest.raises(NotImplementedError, match="not built for"):
            m.get_pose_uncertainty_for_camera(SimpleNamespace(), torch.zeros(6))


def test_models_return_jacobians_and_pose_uncertainty(monkeypatch):
    from uncertainty_nerf_gs_amd import ops, plugin, splat
    H, W = 6, 8
    seen = []

    def fake(gp, c2w, fx, fy, cx, cy, H, W, background, proj=None, channels=ops.POSE_CHANNELS, want=("proj", "val"), **kw):
        Cn = bin(ops.pose_channel_bits(channels)).count("1")
        P = 12 if proj is None else proj.shape[1]
        seen.append(dict(proj=None if proj is None else tuple(proj.shape), channels=tuple(channels), want=tuple(want), kw=kw,
                         n=gp["means"].shape[0]))
        px = torch.arange(H * W, dtype=torch.float32).view(H, W, 1)
        ch = torch.arange(1, Cn + 1, dtype=torch.float32)
        val = px + ch / 8
        if Cn == 5:
            val[..., 3] = (px[..., 0] % 3 > 0) * 0.5                      # accumulation: a third of the pixels blend nothing
            val[..., 4] = torch.where(val[..., 3] > 0, 2.0 + px[..., 0], torch.zeros(()))
        out = {"proj": px[..., None] * torch.ones(H, W, Cn, P), "var": (px % 5) * ch * ch, "val": val}
        return {k: out[k] for k in want}

    monkeypatch.setattr(splat, "pose_jacobian_camera", fake)
    m = plugin.build_model("active-splatfacto", num_points=4)
    cam = SimpleNamespace(camera_to_worlds=torch.from_numpy(SPG.frame_c2w())[None], fx=10.0, fy=10.0, cx=4.0, cy=3.0, height=H, width=W)
    out = m.get_splat_pose_jacobians_for_camera(cam)
    assert sorted(out) == ["jacobian", "values"] and out["jacobian"].shape == (H, W, 5, 6) and out["values"].shape == (H, W, 5)
    assert seen[-1]["proj"] == (12, 6) and seen[-1]["want"] == ("proj", "val") and seen[-1]["n"] == 4
    assert seen[-1]["kw"]["rasterize_mode"] == m.config.rasterize_mode and seen[-1]["kw"]["crop_ids"] is None
    out = m.get_splat_pose_jacobians_for_camera(cam, channels=("accumulation", "g"), basis="c2w")
    assert out["jacobian"].shape == (H, W, 2, 12) and out["values"].shape == (H, W, 2) and seen[-1]["proj"] is None
    with pytest.raises(ValueError, match="basis"):
        m.get_splat_pose_jacobians_for_camera(cam, basis="quaternion")
    with pytest.raises(NotImplementedError, match="pinhole"):
        m.get_splat_pose_jacobians_for_camera(SimpleNamespace(**{**vars(cam), "camera_type": 2}))
    with pytest.raises(ValueError, match="one camera, got a batch of 2"):
        m.get_splat_pose_uncertainty_for_camera(SimpleNamespace(**{**vars(cam), "camera_to_worlds": cam.camera_to_worlds.repeat(2, 1, 1)}),
                                                torch.ones(6))
    unc = m.get_splat_pose_uncertainty_for_camera(cam, torch.tensor([0.01, 0.01, 0.01, 1e-3, 1e-3, 0.0]))
    assert seen[-1]["proj"] == (12, 5) and seen[-1]["want"] == ("var", "val") and seen[-1]["channels"] == ops.POSE_CHANNELS
    assert sorted(unc) == sorted(["rgb_var_pose", "rgb_std_pose", "accumulation_std_pose", "depth_std_pose", "rgb", "accumulation", "depth"])
    for k, v in unc.items():
        assert v.shape == (H, W, 3 if k == "rgb" else 1), k
    px = torch.arange(H * W, dtype=torch.float32).view(H, W, 1)
    assert torch.equal(unc["rgb_var_pose"], (px % 5) * (1 + 4 + 9) / 3) and torch.equal(unc["rgb_std_pose"], unc["rgb_var_pose"].sqrt())
    assert torch.equal(unc["accumulation_std_pose"], ((px % 5) * 16).sqrt()) and torch.equal(unc["depth_std_pose"], ((px % 5) * 25).sqrt())
    hit = px % 3 > 0
    assert torch.equal(unc["accumulation"], hit * 0.5)
    # the frame's fill: where nothing was blended, the largest unnormalised depth sum (here 0.5 x (2 + the last blending pixel))
    last = int(px[hit].max())
    assert torch.equal(unc["depth"][hit], 2.0 + px[hit]) and (unc["depth"][~hit] == 0.5 * (2.0 + last)).all()
    with pytest.raises(ValueError, match="pose_cov"):
        m.get_splat_pose_uncertainty_for_camera(cam, None)
    # a crop box reaches the frame call
    m.eval()
    m.set_crop(SimpleNamespace(within=lambda pts: torch.tensor([[True], [False], [True], [True]])))
    m.get_splat_pose_jacobians_for_camera(cam)
    assert seen[-1]["kw"]["crop_ids"].tolist() == [True, False, True, True]
