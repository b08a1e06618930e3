"""CPU side of the MC-dropout pose gradient: the masked float64 reference of tests/pose_grad_mc_cases.py is checked against
the unmasked one, against central differences and against the fp32 oracle; the exclusion cap is asserted for every case; the
ABI symbol, the refusals that need no device and the host plumbing are checked without a GPU."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

import pose_grad_cases as PC
import pose_grad_mc_cases as MC
from conftest import ROOT

FD_STEP, FD_TOL = 1e-7, 1e-6        # as tests/test_pose_grad_cpu.py (the same function class, K of them averaged)
# the masked fp32 oracle against the float64 reference: the unmasked oracle sits at 0.6 .. 2.1e-5 of the RMS gradient
# (tests/test_gpu_pose_grad.py); dropout multiplies kept units by 1.25 and removes the others, which changes no rounding rule
ORACLE_MAX = 5e-5


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_exclusion_cap_and_oracle_error(name):
    """the reference's own margins leave out at most 20 % of every case's rays, and the fp32 oracle under the same masks
    meets the float64 reference at the size it has without dropout"""
    s, ref, o32 = MC.spec(name), MC.reference64(name), MC.oracle32(name)
    excluded = 1.0 - ref.keep.double().mean().item()
    yard = MC.rel_error(o32.grad, ref)
    print(f"[pose_grad_mc] {name}: S={s.c.S} K={s.K} sites={s.sites}: {excluded:.3f} of {s.c.R} rays left out, fp32 oracle {yard:.3e}")
    assert excluded <= MC.MAX_EXCLUDED
    assert torch.isfinite(ref.grad).all() and ref.grad[ref.keep].abs().max() > 0
    assert 0.0 < yard <= ORACLE_MAX
    assert (o32.rgb.double() - ref.rgb).abs().max().item() <= 2e-6


def test_masks_drop_units_at_every_active_site():
    s = MC.spec("head0")
    mk = MC.keep_masks(s.c, s.K, s.sites)
    assert len(mk) == s.K and mk[0][MC.TRUNK] is None
    for b in (MC.HEAD0, MC.HEAD1):
        rate = torch.stack([m[b] for m in mk]).float().mean().item()
        assert abs(rate - (1 - MC.P_DROP)) < 0.01
    assert not torch.equal(mk[0][MC.HEAD1], mk[1][MC.HEAD1]) and not torch.equal(mk[0][MC.HEAD0], mk[0][MC.HEAD1])
    bits = MC.pack_bits(mk[0][MC.HEAD1])
    assert bits.shape == (s.c.R * s.c.S, 2) and bits.dtype == torch.int32
    back = ((bits.to(torch.int64)[:, :, None] >> torch.arange(32)) & 1).reshape(-1, 64).bool()
    assert torch.equal(back, mk[0][MC.HEAD1])


@pytest.mark.parametrize("name", ["S47", "tcnn_half", "uniform"])
def test_all_kept_single_pass_is_the_unmasked_reference(name):
    """K = 1, every unit kept, p = 0: the masked float64 reference is pose_grad_cases.reference64 of the same case"""
    c = PC.case(name)
    assert c.kind == "mcdropout"
    got, want = MC.grad64(c, MC.all_kept(c), 0.0), PC.reference64(name)
    assert not bool((got.keep & ~want.keep).any())      # the same margins (+ the degenerate pinned cells, left out here only)
    assert torch.equal(got.grad, want.grad) and torch.equal(got.rgb, want.rgb)


def test_reference_matches_central_differences():
    """ds/dc2w of the masked float64 reference (folded by pose_from_ray_grad) against central differences of the masked float64
    render in all 12 pose entries, on the kept rays"""
    s = MC.spec("S16")
    c, masks = s.c, MC.keep_masks(s.c, s.K, s.sites)
    c2w = c.c2w.double()
    rot_inv = torch.linalg.inv(c2w[:, :3])
    d0 = c.directions.double()
    dir_cam = d0 @ rot_inv.t()
    dn = d0 / d0.norm(dim=-1, keepdim=True)
    ref = MC.grad64(c, masks, s.p, c.origins, dn)
    want = PC.pose_from_ray_grad(ref.grad, dn, rot_inv)
    scale = want[ref.keep].pow(2).mean().sqrt().item()
    worst = 0.0
    for a in range(3):
        for b in range(4):
            sides = []
            for sign in (1.0, -1.0):
                m = c2w.clone()
                m[a, b] += sign * FD_STEP
                d = dir_cam @ m[:, :3].t()
                sides.append(MC.render64(c, masks, s.p, m[:, 3].expand(c.R, 3), d / d.norm(dim=-1, keepdim=True)))
            fd = (sides[0] - sides[1]) / (2 * FD_STEP)
            worst = max(worst, ((fd - want[:, a, b])[ref.keep].abs().max() / scale).item())
    print(f"[pose_grad_mc] S16: worst |fd - autograd| / rms = {worst:.2e}")
    assert worst <= FD_TOL


def test_single_pass_references_average_to_the_case():
    """the float64 reference is linear in the passes: mean_k of the single-pass gradients is the K-pass gradient"""
    s = MC.spec("S48K2")
    whole = MC.reference64("S48K2")
    parts = [MC.reference64("S48K2", (k,)) for k in range(s.K)]
    mean = torch.stack([p.grad for p in parts]).mean(0)
    assert (mean - whole.grad).abs().max().item() <= 1e-12 * whole.grad.abs().max().item()
    assert torch.equal(whole.keep, parts[0].keep & parts[1].keep)


def test_symbol_declared_and_bound(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "unerf.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+unerf_pose_grad_mc\s*\(([^;]*)\)\s*;", header)
    assert m, "unerf_pose_grad_mc is not declared in include/unerf.h"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    assert "unerf_pose_grad_mc" in lib.SIGNATURES
    assert len(lib.SIGNATURES["unerf_pose_grad_mc"][1]) == n_args == 17
    h = lib.load()
    assert h.unerf_pose_grad_mc is not None
    assert h.unerf_version() == 1420          # additive: same ABI version


def _params(lib, **kw):
    fp = lib.FieldParams()
    for name in ("table", "scalings", "w0t", "b0", "w1t", "b1", "h0t", "hb0", "h1t", "hb1", "h2t", "hb2"):
        setattr(fp, name, 1)
    fp.L, fp.log2T, fp.mode, fp.out1, fp.K, fp.p_drop = 16, 19, lib.FIELD_MCDROPOUT, 16, 4, 0.2
    for k, v in kw.items():
        setattr(fp, k, v)
    return fp


def _masks(lib, sites=(1, 0, 1, 0), stride=10 * 48, offset=0):
    km = lib.KeepMasks()
    for i, on in enumerate(sites):
        km.site[i] = 1 if on else None
    km.pass_stride, km.sample_offset = stride, offset
    return km


def test_refusals_come_before_any_launch(lib):
    """every refusal of include/unerf.h: unerf_pose_grad_mc returns -1 with its reason -- on a machine without a GPU, so
    nothing was launched -- and R = 0 returns 0"""
    h = lib.load()

    def call(fp, km, R=10, S=48, near=0.05):
        return h.unerf_pose_grad_mc(1, 1, 1, R, S, near, 1000.0, 0, 0, C.byref(fp), None if km is None else C.byref(km), 0, None,
                                    None, 1, None, None)

    def refused(fp, km, text, **kw):
        assert call(fp, km, **kw) == -1
        assert text in h.unerf_last_error(), h.unerf_last_error()

    for km in (None, _masks(lib)):
        refused(_params(lib, mode=lib.FIELD_ACTIVE, out1=17), km, b"pose_grad_mc: mode")
        refused(_params(lib, mode=lib.FIELD_LAPLACE, out1=15), km, b"pose_grad_mc: mode")
        refused(_params(lib, K=0), km, b"K=0")
        refused(_params(lib, drop_sites=9), km, b"UNERF_DROP_HEADIN is out of scope")
        refused(_params(lib, hidden=32, hidden_color=64, geo_dim=15, feat_per_level=2, app_dim=32), km, b"widths")
        refused(_params(lib, L=8), km, b"widths")
        refused(_params(lib), km, b"near_plane", near=-1.0)
        refused(_params(lib), km, b"S=65", S=65)
        refused(_params(lib), km, b"S=0", S=0)
    refused(_params(lib), _masks(lib, sites=(1, 0, 0, 0)), b"site HEAD1 is active")            # drop_sites 0 = TRUNK | HEAD1
    refused(_params(lib, drop_sites=7), _masks(lib, sites=(1, 0, 1, 0)), b"site HEAD0 is active")
    refused(_params(lib), _masks(lib, sites=(1, 1, 1, 0)), b"site HEAD0, which is not active")
    refused(_params(lib, drop_sites=1), _masks(lib, sites=(1, 0, 1, 0)), b"site HEAD1, which is not active")
    refused(_params(lib), _masks(lib, stride=10 * 48 - 1), b"pass_stride=479 < sample_offset + R*S")
    refused(_params(lib), _masks(lib, stride=10 * 48, offset=1), b"pass_stride=480 < sample_offset + R*S")
    assert call(_params(lib), _masks(lib, stride=0), R=0) == 0
    assert call(_params(lib), None, R=0) == 0


def _plugin_model(name):
    import sys
    try:
        import nerfstudio  # noqa: F401
    except ImportError:
        stubs = os.path.join(ROOT, "tests", "stubs")
        if stubs not in sys.path:
            sys.path.insert(0, stubs)
    from uncertainty_nerf_gs_amd import plugin
    cfg = plugin.method_specifications()[name].config.pipeline.model
    cfg.log2_hashmap_size = 6
    cfg.proposal_net_args_list = [dict(a, log2_hashmap_size=6) for a in cfg.proposal_net_args_list]
    return cfg.setup(scene_box=None, num_train_data=1)


def test_model_method_names_its_mask_draw(monkeypatch):
    """render.pose_gradient_camera_mc replaced by a recorder (no GPU here): the default seed is the last render's, an explicit
    mask_seed is in force during the call only, frame_counter does not move, torch masks are replayed or reported gone, and
    the plugin model forwards the method"""
    from uncertainty_nerf_gs_amd import models, render
    seen = []
    field = SimpleNamespace(seed=0, K=8, p_drop=0.2)
    scene = SimpleNamespace(field=field, chunk_rays=1 << 15)

    def fake(scene_, c2w, **kw):
        seen.append(dict(kw, seed=scene_.field.seed, c2w=tuple(c2w.shape)))
        g = torch.zeros(kw["H"], kw["W"], 3, 4)
        return (g, torch.zeros(kw["H"], kw["W"], 3)) if kw["want_rgb"] else g

    monkeypatch.setattr(render, "pose_gradient_camera_mc", fake)
    monkeypatch.setattr(models._NerfactoBase, "device_scene", lambda self, device=None: scene)
    H, W = 6, 9
    cam = models.Camera(torch.eye(4)[None, :3], torch.tensor([[50.0]]), torch.tensor([[50.0]]), torch.tensor([[4.5]]),
                        torch.tensor([[3.0]]), torch.tensor([[H]]), torch.tensor([[W]]))
    pm = _plugin_model("nerfacto-mcdropout")
    model = pm._mirror
    model.seed = 77
    # before any render: the base seed (what device_scene gives the field)
    field.seed = model.seed
    assert model.get_mc_pose_gradients_for_camera(cam).shape == (H, W, 3, 4)
    assert seen[-1]["seed"] == 77 and seen[-1].get("keep_masks") is None and model.frame_counter == 0
    # after two renders: the seed _begin_render left, through the plugin model too, and frame_counter stays
    model._begin_render(scene, H * W, scene.chunk_rays)
    model._begin_render(scene, H * W, scene.chunk_rays)
    last = field.seed
    assert last == models.frame_seed(77, 1) and model.frame_counter == 2
    g, rgb = pm.get_mc_pose_gradients_for_camera(cam, rays_per_launch=50, want_rgb=True)
    assert g.shape == (H, W, 3, 4) and rgb.shape == (H, W, 3)
    assert seen[-1]["seed"] == last and seen[-1]["rays_per_launch"] == 50 and seen[-1]["want_rgb"] is True and seen[-1]["W"] == W
    assert seen[-1]["c2w"] == (3, 4) and seen[-1].get("keep_masks") is None
    # an explicit seed holds during the call only
    model.get_mc_pose_gradients_for_camera(cam, mask_seed=4321)
    assert seen[-1]["seed"] == 4321 and field.seed == last and model.frame_counter == 2
    # the old method keeps refusing, and says where to go
    with pytest.raises(NotImplementedError, match="get_mc_pose_gradients_for_camera"):
        pm.get_pose_gradients_for_camera(cam)
    # torch masks: replayed while held, reported gone otherwise
    model.dropout_masks = "torch"
    model._frame_masks = None
    with pytest.raises(Exception, match="torch masks of that frame are gone"):
        model.get_mc_pose_gradients_for_camera(cam)
    token = object()
    model._frame_masks = token
    model.get_mc_pose_gradients_for_camera(cam)
    assert seen[-1]["keep_masks"] is token and model.frame_counter == 2 and field.seed == last
    with pytest.raises(ValueError, match="mask_seed"):
        model.get_mc_pose_gradients_for_camera(cam, mask_seed=1)
    # a mirror without the method
    other = _plugin_model("active-nerfacto")
    with pytest.raises(NotImplementedError, match="MC-dropout pose gradient"):
        other.get_mc_pose_gradients_for_camera(cam)


def test_export_takes_a_gradient_callable(tmp_path):
    import numpy as np
    from uncertainty_nerf_gs_amd import posegrad
    H, W = 4, 5
    calls = []

    class Model:
        def get_pose_gradients_for_camera(self, camera, want_rgb=False):
            calls.append("default")
            return torch.zeros(H, W, 3, 4), torch.zeros(H, W, 3)

        def get_mc_pose_gradients_for_camera(self, camera, mask_seed=None, want_rgb=False):
            calls.append(("mc", mask_seed, want_rgb, camera.camera_to_worlds.clone()))
            return torch.ones(H, W, 3, 4), torch.full((H, W, 3), 0.5)

    m = Model()
    cam = SimpleNamespace(camera_to_worlds=PC.synthetic.orbit_c2w(0.4), fx=20.0, fy=21.0, cx=2.5, cy=2.0, height=H, width=W)
    import functools
    files = posegrad.export_pose_gradients(m, cam, 3, tmp_path / "a", shift_param="tx", shift_magnitude=0.1,
                                           gradient_fn=functools.partial(m.get_mc_pose_gradients_for_camera, mask_seed=9))
    assert len(calls) == 1 and calls[0][:3] == ("mc", 9, True)
    assert torch.equal(calls[0][3], posegrad.perturbed_pose(cam.camera_to_worlds, "tx", 0.1))
    assert np.array_equal(np.load(files["c2w_grads_perturbed"]), np.ones((H, W, 3, 4)))
    assert np.array_equal(np.load(files["pred_rgb_perturbed"]), np.full((H, W, 3), 0.5, np.float32))
    posegrad.export_pose_gradients(m, cam, 3, tmp_path / "b")
    assert calls[-1] == "default" and len(calls) == 2
