"""CPU side of the pose-gradient feature: the float64 reference of tests/pose_grad_cases.py is checked against central
differences and against autograd through the oracle's ray generator, the exclusion cap is asserted for every case, and the
host pieces (perturbed_pose, the export's files, the ABI symbol) are checked without a GPU."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pose_grad_cases as PC
from conftest import ROOT
from oracle import nerf_oracle as O

FD_STEP = 1e-7
# central differences of the float64 render s (|s| <= 1, gradients of the order 0.1): rounding 2^-52 |s| / h = 2e-9 at
# h = 1e-7, truncation h^2 |s'''| / 6 below that for any |s'''| < 1e6.  The step also has to stay inside the piece of the
# piecewise function the kept rays sit in: they keep every ReLU input 1e-6 away from zero, ten times what a pose entry moved
# by h shifts a pre-activation whose slope is below 1.  FD_TOL leaves two decades over the rounding term.
FD_TOL = 1e-6


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_exclusion_cap(name):
    """the reference's own margins leave out at most 15 % of every case's rays"""
    ref = PC.reference64(name)
    excluded = 1.0 - ref.keep.double().mean().item()
    print(f"{name}: {excluded:.3f} of {PC.case(name).R} rays left out")
    assert excluded <= PC.MAX_EXCLUDED
    assert torch.isfinite(ref.grad).all() and ref.grad[ref.keep].abs().max() > 0


def test_case_covers_both_sides_of_the_contraction():
    c = PC.case("base")
    pos = PC.O.sample_positions(c.origins, c.directions, PC.euclid_bins32(c)).abs().amax(-1)
    assert bool((pos[:, 0] < 1).all()) and bool((pos[:, -1] > 1).all())
    a = PC.case("aabb")
    _, sel = PC.O.normalized_positions(PC.O.sample_positions(a.origins, a.directions, PC.euclid_bins32(a)), a.t["aabb"])
    assert 0.05 < (~sel).float().mean().item() < 0.95       # samples inside and outside the scene box


@pytest.mark.parametrize("name", ["S16", "tcnn", "aabb", "white"])
def test_reference_matches_central_differences(name):
    """d s / d c2w of the float64 reference (autograd through o and d, folded by pose_from_ray_grad) against central
    differences of the float64 render in all 12 pose entries, on the kept rays"""
    c = PC.case(name)
    c2w = c.c2w.double()
    rot_inv = torch.linalg.inv(c2w[:, :3])
    d0 = c.directions.double()
    dir_cam = d0 @ rot_inv.t()
    dn = d0 / d0.norm(dim=-1, keepdim=True)       # the direction the unperturbed pose gives in float64
    ref = PC.grad64_at(name, c.origins, dn)
    want = PC.pose_from_ray_grad(ref.grad, dn, rot_inv)
    scale = want[ref.keep].pow(2).mean().sqrt().item()
    worst = 0.0
    for a in range(3):
        for b in range(4):
            s = []
            for sign in (1.0, -1.0):
                m = c2w.clone()
                m[a, b] += sign * FD_STEP
                d = dir_cam @ m[:, :3].t()
                s.append(PC.render64(name, m[:, 3].expand(c.R, 3), d / d.norm(dim=-1, keepdim=True)))
            fd = (s[0] - s[1]) / (2 * FD_STEP)
            worst = max(worst, ((fd - want[:, a, b])[ref.keep].abs().max() / scale).item())
    print(f"{name}: worst |fd - autograd| / rms = {worst:.2e}")
    assert worst <= FD_TOL


def test_epilogue_matches_autograd_through_generate_rays():
    """P (R^-1 d) against autograd through O.generate_rays with a scaled, non-orthonormal rotation block: for any scalar
    function of (origins, directions), d / d c2w[a][b] = P[a] (R^-1 d)[b] and d / d c2w[:, 3] = the origin gradient"""
    g = torch.Generator().manual_seed(5)
    c2w = PC.synthetic.orbit_c2w(0.8).double()
    c2w[:, :3] = c2w[:, :3] @ (torch.eye(3, dtype=torch.float64) * 1.7 + 0.2 * torch.randn(3, 3, generator=g, dtype=torch.float64))
    c2w = c2w.float().requires_grad_(True)
    H, W = 5, 7
    o, d, _ = O.generate_rays(c2w, 9.0, 11.0, 3.3, 2.6, H, W)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    A = torch.randn(H * W, 3, generator=g)
    B = torch.randn(H * W, 3, 3, generator=g)
    # any smooth per-ray function: its (o, d) gradient is known in closed form
    f = (o * A).sum(-1) + torch.einsum("ri,rij,rj->r", d, B, d) + torch.sin(d[:, 0] * 3.0)
    got = []
    for r in range(H * W):
        got.append(torch.autograd.grad(f[r], c2w, retain_graph=True)[0])
    got = torch.stack(got).double()
    dd = d.detach().double()
    gd = torch.einsum("rij,rj->ri", B.double(), dd) + torch.einsum("rji,rj->ri", B.double(), dd)
    gd[:, 0] += 3.0 * torch.cos(dd[:, 0] * 3.0)
    want = PC.pose_from_ray_grad(torch.cat([A.double(), gd], -1), dd, torch.linalg.inv(c2w.detach().double()[:, :3]))
    err = (got - want).abs().max().item() / want.abs().max().item()
    print(f"epilogue vs autograd: {err:.2e}")
    assert err <= 2e-5      # fp32 autograd through the fp32 ray generator: a few hundred ulp


@pytest.mark.parametrize("param", ["tx", "ty", "tz", "angx", "angy", "angz"])
@pytest.mark.parametrize("magnitude", [0.0, 1e-3, -0.3, 2.0])
def test_perturbed_pose_matches_expm(param, magnitude):
    from scipy.linalg import expm
    from uncertainty_nerf_gs_amd import posegrad
    c2w = PC.synthetic.orbit_c2w(1.1)
    got = posegrad.perturbed_pose(c2w, param, magnitude)
    assert got.shape == (3, 4) and got.dtype == torch.float32
    v = np.zeros(6)
    v[posegrad.POSE_PARAMS.index(param)] = magnitude
    twist = np.zeros((4, 4))
    twist[:3, :3] = [[0, -v[5], v[4]], [v[5], 0, -v[3]], [-v[4], v[3], 0]]
    twist[:3, 3] = v[:3]
    base = np.eye(4)
    base[:3] = c2w.double().numpy()
    want = (base @ expm(twist))[:3]
    assert np.abs(got.double().numpy() - want).max() <= 1e-6      # fp32 products of numbers of size <= 2.6
    with pytest.raises(ValueError):
        posegrad.perturbed_pose(c2w, "roll", 0.1)


def test_export_writes_the_reference_files(tmp_path):
    from uncertainty_nerf_gs_amd import posegrad
    H, W = 6, 9
    seen = {}

    class FakeModel:
        def get_pose_gradients_for_camera(self, camera, want_rgb=False):
            seen["c2w"] = camera.camera_to_worlds.clone()
            g = torch.arange(H * W * 12, dtype=torch.float32).view(H, W, 3, 4)
            return g, torch.linspace(0, 1, H * W * 3).view(H, W, 3)

    cam = SimpleNamespace(camera_to_worlds=PC.synthetic.orbit_c2w(0.4), fx=20.0, fy=21.0, cx=4.5, cy=3.0, height=H, width=W)
    files = posegrad.export_pose_gradients(FakeModel(), cam, 32, tmp_path, shift_param="angy", shift_magnitude=0.05, seed=42)
    out = tmp_path / "image_32"
    assert sorted(p.name for p in out.iterdir()) == sorted(
        ["c2w_img32.npy", "c2w_perturbed.npy", "camera_intrinsics.npy", "pred_rgb_perturbed.npy", "c2w_grads_perturbed.npy",
         "image00032_perturbed.png"])
    assert set(files.values()) == set(out.iterdir())
    want = {"c2w_img32.npy": ((3, 4), np.float32), "c2w_perturbed.npy": ((3, 4), np.float32),
            "camera_intrinsics.npy": ((3, 3), np.float32), "pred_rgb_perturbed.npy": ((H, W, 3), np.float32),
            "c2w_grads_perturbed.npy": ((H, W, 3, 4), np.float64)}
    for fname, (shape, dtype) in want.items():
        a = np.load(out / fname)
        assert a.shape == shape and a.dtype == dtype, fname
    assert np.array_equal(np.load(out / "c2w_img32.npy"), cam.camera_to_worlds.numpy())
    assert np.array_equal(np.load(out / "c2w_perturbed.npy"), posegrad.perturbed_pose(cam.camera_to_worlds, "angy", 0.05).numpy())
    assert torch.equal(seen["c2w"], posegrad.perturbed_pose(cam.camera_to_worlds, "angy", 0.05))   # rendered at the perturbed pose
    assert torch.equal(cam.camera_to_worlds, PC.synthetic.orbit_c2w(0.4))                          # the caller's camera is untouched
    assert np.array_equal(np.load(out / "camera_intrinsics.npy"), np.array([[20, 0, 4.5], [0, 21, 3], [0, 0, 1]], np.float32))
    assert np.array_equal(np.load(out / "c2w_grads_perturbed.npy"), np.arange(H * W * 12, dtype=np.float64).reshape(H, W, 3, 4))
    png = (out / "image00032_perturbed.png").read_bytes()
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and int.from_bytes(png[16:20], "big") == W and int.from_bytes(png[20:24], "big") == H


def test_symbol_declared_and_bound():
    from uncertainty_nerf_gs_amd import lib
    header = open(os.path.join(ROOT, "include", "unerf.h")).read()
    m = re.search(r"\bint\s+unerf_pose_grad\s*\(([^;]*)\)\s*;", header)
    assert m, "unerf_pose_grad is not declared in include/unerf.h"
    n_args = len([a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()])
    assert "unerf_pose_grad" in lib.SIGNATURES
    assert len(lib.SIGNATURES["unerf_pose_grad"][1]) == n_args == 15


def test_models_without_a_pose_gradient_say_why():
    from uncertainty_nerf_gs_amd import models
    for cls in (models.NerfactoMCDropoutModel, models.NerfactoLaplaceModel):
        assert isinstance(cls._no_pose_gradient, str) and cls._no_pose_gradient.endswith(".")
        with pytest.raises(NotImplementedError, match="get_pose_gradients_for_camera"):
            cls.get_pose_gradients_for_camera(SimpleNamespace(_no_pose_gradient=cls._no_pose_gradient), None)
    assert models.NerfactoModel._no_pose_gradient is None and models.ActiveNerfactoModel._no_pose_gradient is None


def test_plugin_model_forwards_to_the_mirror(monkeypatch):
    """the nerfstudio-facing model hands camera and keywords to its mirror (render.pose_gradient_camera replaced by a
    recorder: no GPU here); the mc-dropout plugin model raises with its mirror's sentence"""
    import sys
    try:
        import nerfstudio  # noqa: F401
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, "tests", "stubs"))
    from uncertainty_nerf_gs_amd import models, plugin, render
    seen = {}

    def fake(scene, c2w, **kw):
        seen.update(kw, c2w=tuple(c2w.shape))
        return torch.zeros(kw["H"], kw["W"], 3, 4)

    monkeypatch.setattr(render, "pose_gradient_camera", fake)
    monkeypatch.setattr(models._NerfactoBase, "device_scene", lambda self, device=None: object())
    H, W = 6, 9
    cam = models.Camera(torch.eye(4)[None, :3], torch.tensor([[50.0]]), torch.tensor([[50.0]]), torch.tensor([[4.5]]),
                        torch.tensor([[3.0]]), torch.tensor([[H]]), torch.tensor([[W]]))
    specs = plugin.method_specifications()
    for name, ok in (("active-nerfacto", True), ("nerfacto-mcdropout", False)):
        cfg = specs[name].config.pipeline.model
        cfg.log2_hashmap_size = 6
        cfg.proposal_net_args_list = [dict(a, log2_hashmap_size=6) for a in cfg.proposal_net_args_list]
        model = cfg.setup(scene_box=None, num_train_data=1)
        if ok:
            assert model.get_pose_gradients_for_camera(cam, rays_per_launch=50).shape == (H, W, 3, 4)
            assert seen["c2w"] == (3, 4) and seen["rays_per_launch"] == 50 and seen["want_rgb"] is False and seen["W"] == W
        else:
            with pytest.raises(NotImplementedError, match="dropout masks"):
                model.get_pose_gradients_for_camera(cam)
