"""CPU side of the Laplace pose gradient: the float64 reference of tests/pose_grad_laplace_cases.py is checked against central
differences, against the fp32 oracle and against the deterministic graph; the exclusion cap is asserted for every case; the
power of the cases (sampled rows against mean rows, the last row, the selector mask in the scene box) is measured against the
bound the GPU test allows; the ABI symbol, the refusals that need no device and the host plumbing are checked without a GPU."""
import ctypes as C
import os
import re
import warnings
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import pose_grad_cases as PC
import pose_grad_laplace_cases as LC
from conftest import ROOT
from oracle import nerf_oracle as O

FD_STEP, FD_TOL = 1e-7, 1e-6        # as tests/test_pose_grad_cpu.py (the same function class)
ORACLE_MAX = 5e-5                   # the bound tests/test_pose_grad_mc_cpu.py holds the fp32 oracle to


def _gpu_bound(name):
    """what tests/test_gpu_pose_grad_laplace.py allows the kernel on this case: KERNEL_FACTOR x the fp32 oracle's own error"""
    return LC.KERNEL_FACTOR * LC.rel_error(LC.oracle32(name).grad, LC.reference64(name))


def _moved(a, ref):
    """max |a - ref| over the rays ref keeps / rms(ref)"""
    return LC.rel_error(a.grad, ref)


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_exclusion_cap_and_oracle_error(name):
    s, ref, o32 = LC.spec(name), LC.reference64(name), LC.oracle32(name)
    excluded = 1.0 - ref.keep.double().mean().item()
    yard = LC.rel_error(o32.grad, ref)
    rgb_err = (o32.rgb.double() - ref.rgb).abs().max().item()
    print(f"[pose_grad_laplace] {name}: S={s.c.S} n=({s.n_lap}, {s.n_rgb}): {excluded:.3f} of {s.c.R} rays left out, "
          f"fp32 oracle {yard:.3e}, colour {rgb_err:.2e}")
    assert excluded <= LC.MAX_EXCLUDED
    assert torch.isfinite(ref.grad).all() and ref.grad[ref.keep].abs().max() > 0
    assert 0.0 < yard <= ORACLE_MAX
    assert rgb_err <= 2e-6


@pytest.mark.parametrize("name,shear", [("S16", False), ("S16", True), ("box_mask", False), ("stack", True), ("softplus", False)])
def test_reference_matches_central_differences(name, shear):
    """ds/dc2w of the float64 reference (folded by pose_from_ray_grad) against central differences of the float64 render in all
    12 pose entries, on the kept rays; orthonormal and sheared rotation blocks"""
    s = LC.spec(name)
    c = s.c
    c2w = c.c2w.double().clone()
    dir_cam = c.directions.double() @ torch.linalg.inv(c2w[:, :3]).t()         # the camera-frame directions of the case's rays
    if shear:
        g = torch.Generator().manual_seed(11)
        c2w[:, :3] = c2w[:, :3] @ (torch.eye(3, dtype=torch.float64) * 1.6 + 0.25 * torch.randn(3, 3, generator=g, dtype=torch.float64))
    rot_inv = torch.linalg.inv(c2w[:, :3])
    d0 = dir_cam @ c2w[:, :3].t()
    dn = d0 / d0.norm(dim=-1, keepdim=True)
    ref = LC.grad64(s, c.origins, dn)
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
                sides.append(LC.render64(s, m[:, 3].expand(c.R, 3), d / d.norm(dim=-1, keepdim=True)))
            fd = (sides[0] - sides[1]) / (2 * FD_STEP)
            worst = max(worst, ((fd - want[:, a, b])[ref.keep].abs().max() / scale).item())
    print(f"[pose_grad_laplace] {name} shear={shear}: worst |fd - autograd| / rms = {worst:.2e}")
    assert worst <= FD_TOL


def test_cases_see_the_sampled_rows():
    """S = 48, 100 + 100 rows: the reference under the sampled rows differs from the reference under the mean rows, and from
    the reference without the last row, by >= 100 x what the GPU test allows"""
    s, ref = LC.spec("S48"), LC.reference64("S48")
    bound = _gpu_bound("S48")
    md, mr = LC.mean_rows(s.c.t)
    md, mr = md[None], mr[None]
    both = _moved(LC.grad64(s, ws_density=md, ws_rgb=mr), ref)
    dens = _moved(LC.grad64(s, ws_density=md), ref)
    col = _moved(LC.grad64(s, ws_rgb=mr), ref)
    last = _moved(LC.grad64(s, ws_density=s.ws_density[:, :-1], ws_rgb=s.ws_rgb[:, :-1]), ref)
    last_d = _moved(LC.grad64(s, ws_density=s.ws_density[:, :-1]), ref)
    last_c = _moved(LC.grad64(s, ws_rgb=s.ws_rgb[:, :-1]), ref)
    print(f"[pose_grad_laplace] S48: mean rows move the reference by {both:.2e} (density only {dens:.2e}, colour only {col:.2e}), "
          f"dropping the last row by {last:.2e} (density {last_d:.2e}, colour {last_c:.2e}); GPU bound {bound:.2e}")
    for moved in (both, dens, col, last):
        assert moved >= 100 * bound


def test_scene_box_case_sees_the_selector_mask():
    """the camera lies outside the box: unselected samples stand in front of selected ones, and the masked and unmasked
    references differ by >= 100 x the GPU bound (with the camera inside, everything unselected lies behind and they agree)"""
    s = LC.spec("box_mask")
    c = s.c
    box = torch.tensor(LC.BOX)
    assert bool(((c.origins < box[0]) | (c.origins > box[1])).any(-1).all())
    _, sel = O.normalized_positions(O.sample_positions(c.origins, c.directions, LC.euclid_bins32(c)), c.t["aabb"])
    first = sel.float().argmax(-1)                       # the first selected sample of a ray
    hit = sel.any(-1)
    assert hit.float().mean().item() > 0.5 and bool((first[hit] > 0).all())
    ref = LC.reference64("box_mask")
    moved = _moved(LC.grad64(s, mask=False), ref)
    bound = max(_gpu_bound("box_mask"), _gpu_bound("box"))
    print(f"[pose_grad_laplace] box_mask: {(~sel).float().mean().item():.2f} of the samples unselected, masked against unmasked "
          f"{moved:.2e}, GPU bound {bound:.2e}")
    assert moved >= 100 * bound
    for name in ("box", "box_mask"):
        assert 1.0 - LC.reference64(name).keep.double().mean().item() <= LC.MAX_EXCLUDED


def test_mean_rows_with_mask_are_the_deterministic_graph():
    """(1, 1) mean rows and lap_mask_density: the reference equals float64 autograd through the statements of
    O.laplace_field_deterministic (plain Linear heads, selector-masked density) on the same pinned cells"""
    s = LC.spec("mean_mask")
    c = s.c
    ref = LC.reference64("mean_mask")
    ft = LC._field_tensors(c, torch.float64)
    f = c.t["field"]
    p32 = LC._p32(c, LC._field_tensors(c, torch.float32))
    o = c.origins.double().clone().requires_grad_(True)
    d = c.directions.double().clone().requires_grad_(True)
    eb = LC.euclid_bins32(c).double()
    R, S = c.R, c.S
    p, sel = O.normalized_positions(O.sample_positions(o, d, eb), ft.aabb)
    feat, _ = LC._encode_pinned(c, ft, p.reshape(-1, 3), p32)
    hb = F.linear(feat, ft.w0, ft.b0)
    geo = F.linear(hb, ft.w1, ft.b1).view(R, S, -1)
    density = torch.exp(F.linear(hb, f["density_w"].double(), f["density_b"].double())).view(R, S) * sel
    x = O._color_inputs(d, S, geo, ft.appearance, ft.sh_remap)
    x = F.relu(F.linear(x, ft.head_w[0], ft.head_b[0]))
    x = F.relu(F.linear(x, ft.head_w[1], ft.head_b[1]))
    rgb = torch.sigmoid(F.linear(x, ft.head_w[2], ft.head_b[2])).view(R, S, 3)
    pred = O.render_rgb(rgb, O.get_weights(density, eb[..., 1:] - eb[..., :-1]), c.background)
    go, gd = torch.autograd.grad(pred.mean(-1).sum(), (o, d))
    g = torch.cat([go, gd], dim=-1)
    assert (g - ref.grad).abs().max().item() <= 1e-11 * ref.grad.abs().max().item()
    assert (pred.detach() - ref.rgb).abs().max().item() <= 1e-14


def _gate_shares(name):
    """-> (share of the kept rays with the gates of channels 0 and 1 closed and channel 2's open, share with all three open)"""
    ref = LC.reference64(name)
    rgb = ref.rgb[ref.keep]
    closed = (rgb == 0.0) | (rgb == 1.0)             # the clamp's own values
    assert ref.grad[ref.keep][closed.any(-1)].abs().max() > 0          # channel 2 still carries a gradient there
    return (closed[:, 0] & closed[:, 1] & ~closed[:, 2]).double().mean().item(), (~closed).all(-1).double().mean().item()


def test_gate_cases_have_rays_behind_the_clamp():
    """the constant backgrounds outside [0, 1]: "gate" has a good share of kept rays with unequal channel adjoints and another
    with all gates open, "gate16" nearly only the former"""
    mixed, opened = _gate_shares("gate")
    mixed16, opened16 = _gate_shares("gate16")
    print(f"[pose_grad_laplace] gate: {mixed:.2f} of the kept rays with channels 0 and 1 clamped, {opened:.2f} with none; "
          f"gate16: {mixed16:.2f}, {opened16:.2f}")
    assert mixed >= 0.25 and opened >= 0.25 and mixed16 >= 0.9


def test_stack_case_straddles_sets():
    s = LC.spec("stack")
    sets = LC.ray_sets(s)
    assert s.c.R == 21 and s.chunk == 6 and s.offset == 4 and s.ws_density.shape == (5, 5, 65) and s.ws_rgb.shape == (5, 7, 195)
    assert int(sets[-1]) == s.sets - 1 == (s.offset + s.c.R - 1) // s.chunk
    blocks = [set(sets[b:b + 4].tolist()) for b in range(0, s.c.R, 4)]          # a block is four waves = four rays
    assert sum(len(b) == 2 for b in blocks) >= 2
    assert not torch.equal(s.ws_density[0], s.ws_density[1])


def test_symbol_declared_and_bound(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "unerf.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+unerf_pose_grad_laplace\s*\(([^;]*)\)\s*;", header)
    assert m, "unerf_pose_grad_laplace is not declared in include/unerf.h"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    assert "unerf_pose_grad_laplace" in lib.SIGNATURES
    assert len(lib.SIGNATURES["unerf_pose_grad_laplace"][1]) == n_args == 16
    h = lib.load()
    assert h.unerf_pose_grad_laplace is not None
    assert h.unerf_version() == 1420          # additive: same ABI version


def _params(lib, **kw):
    fp = lib.FieldParams()
    for name in ("table", "scalings", "w0t", "b0", "w1t", "b1", "h0t", "hb0", "h1t", "hb1", "ws_density", "ws_rgb"):
        setattr(fp, name, 1)
    fp.L, fp.log2T, fp.mode, fp.out1, fp.n_lap, fp.n_lap_rgb, fp.lap_sets = 16, 19, lib.FIELD_LAPLACE, 15, 100, 100, 1
    for k, v in kw.items():
        setattr(fp, k, v)
    return fp


def test_refusals_come_before_any_launch(lib):
    """every refusal of include/unerf.h: unerf_pose_grad_laplace returns -1 with its reason -- on a machine without a GPU, so
    nothing was launched -- and R = 0 returns 0; unerf_pose_grad keeps refusing a LAPLACE field"""
    h = lib.load()

    def call(fp, R=10, S=48, near=0.05, offset=0, ptr=1, out=1):
        return h.unerf_pose_grad_laplace(ptr, ptr, ptr, R, S, near, 1000.0, 0, offset, C.byref(fp), 0, None, None, out, None, None)

    def refused(fp, text, **kw):
        assert call(fp, **kw) == -1
        assert text in h.unerf_last_error(), h.unerf_last_error()

    refused(_params(lib, mode=lib.FIELD_ACTIVE, out1=17), b"pose_grad_laplace: mode")
    refused(_params(lib, mode=lib.FIELD_MCDROPOUT, out1=16), b"pose_grad_laplace: mode")
    refused(_params(lib, hidden=32, hidden_color=64, geo_dim=15, feat_per_level=2, app_dim=32), b"widths")
    refused(_params(lib, L=8), b"widths")
    refused(_params(lib, out1=16), b"widths")
    refused(_params(lib), b"near_plane", near=-1.0)
    refused(_params(lib), b"S=65", S=65)
    refused(_params(lib), b"S=0", S=0)
    refused(_params(lib, ws_density=None), b"null ws_density / ws_rgb")
    refused(_params(lib, ws_rgb=None), b"null ws_density / ws_rgb")
    refused(_params(lib, w1t=None), b"null field pointer")
    refused(_params(lib, table=None), b"null field pointer")
    refused(_params(lib), b"pose_grad_laplace: null pointer", out=None)
    refused(_params(lib), b"pose_grad_laplace: null pointer", ptr=None)
    refused(_params(lib, n_lap=0), b"n_lap=0")
    refused(_params(lib, lap_chunk_rays=-32), b"lap_chunk_rays=-32")
    refused(_params(lib, lap_chunk_rays=6, lap_sets=2), b"lap_sets=2", offset=3)          # rays 3 .. 12: set 2 is read
    refused(_params(lib, lap_chunk_rays=32, lap_sets=0), b"lap_sets=0")
    refused(_params(lib), b"ray_offset=-1", offset=-1)
    assert call(_params(lib), R=0) == 0
    assert call(_params(lib, lap_chunk_rays=6, lap_sets=2), R=0, offset=1000) == 0
    # the single-pass entry point keeps refusing the mode
    assert h.unerf_pose_grad(1, 1, 1, 10, 48, 0.05, 1000.0, 0, C.byref(_params(lib)), 0, None, None, 1, None, None) == -1
    assert b"pose_grad: mode" in h.unerf_last_error()


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


def test_render_launches_every_group_at_its_first_ray(monkeypatch):
    """render.pose_gradient_camera_laplace with the op, the ray generator and the sampler replaced by recorders: every group is
    launched with ray_offset = its first ray, and a scene of another mode is refused"""
    from uncertainty_nerf_gs_amd import lib as L, ops, render
    H, W, S = 5, 7, 4
    seen = []

    def fake_rays(c2w, fx, fy, cx, cy, H_, W_, dev, start, n, **kw):
        return torch.zeros(n, 3), torch.zeros(n, 3), None

    def fake_op(o, d, sb, field, near, far, ray_offset=0, rot_inv=None, spacing=0, background=None, want_rgb=False):
        seen.append((int(ray_offset), o.shape[0], rot_inv is not None))
        g = torch.full((o.shape[0], 12), float(ray_offset))
        return (g, torch.zeros(o.shape[0], 3)) if want_rgb else g

    import contextlib
    monkeypatch.setattr(L, "require_gpu", lambda: None)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(ops, "generate_rays", fake_rays)
    monkeypatch.setattr(render, "sample_rays", lambda scene, o, d, clip, start, **kw: (torch.zeros(o.shape[0], S + 1), None))
    monkeypatch.setattr(ops, "pose_grad_laplace", fake_op)
    scene = SimpleNamespace(field=SimpleNamespace(mode=L.FIELD_LAPLACE), near=0.05, far=1000.0, spacing=0, background=None,
                            device=torch.device("cpu"), workspace=None)
    g, rgb = render.pose_gradient_camera_laplace(scene, torch.eye(4)[:3], 10.0, 10.0, 3.5, 2.5, H, W, rays_per_launch=16, want_rgb=True)
    assert g.shape == (H, W, 3, 4) and rgb.shape == (H, W, 3)
    assert seen == [(0, 16, True), (16, 16, True), (32, 3, True)]
    assert g.view(-1, 12)[15, 0] == 0 and g.view(-1, 12)[16, 0] == 16 and g.view(-1, 12)[34, 0] == 32
    scene.field.mode = L.FIELD_MCDROPOUT
    with pytest.raises(L.UnerfError, match="not a LAPLACE field"):
        render.pose_gradient_camera_laplace(scene, torch.eye(4)[:3], 10.0, 10.0, 3.5, 2.5, H, W)


def test_model_method_draws_as_the_unc_render(monkeypatch):
    """render.pose_gradient_camera_laplace replaced by a recorder (no GPU here): the sets come from field.sample_last_layers
    with the caller's generator and get_outputs_for_camera_unc's n_sets rule, weight_samples bypasses the draw, the model's
    state is restored, the plugin model forwards, other mirrors raise and the old method keeps raising"""
    from uncertainty_nerf_gs_amd import models, render
    seen, draws = [], []

    def fake(scene_, c2w, **kw):
        seen.append(dict(kw, c2w=tuple(c2w.shape), ws=model._ws, det=model._deterministic_density, scene=scene_))
        g = torch.zeros(kw["H"], kw["W"], 3, 4)
        return (g, torch.zeros(kw["H"], kw["W"], 3)) if kw["want_rgb"] else g

    monkeypatch.setattr(render, "pose_gradient_camera_laplace", fake)
    monkeypatch.setattr(models._NerfactoBase, "device_scene", lambda self, device=None: ("scene of", self._ws))
    H, W = 6, 9
    cam = models.Camera(torch.eye(4)[None, :3], torch.tensor([[50.0]]), torch.tensor([[50.0]]), torch.tensor([[4.5]]),
                        torch.tensor([[3.0]]), torch.tensor([[H]]), torch.tensor([[W]]))
    pm = _plugin_model("nerfacto-laplace")
    model = pm._mirror
    real = model.field.sample_last_layers

    def recording(**kw):
        draws.append(kw)
        return real(**kw)

    monkeypatch.setattr(model.field, "sample_last_layers", recording)
    invalidated = []
    monkeypatch.setattr(model, "invalidate", lambda: invalidated.append(model._ws))
    # per-chunk sets: ceil(54 / 32) = 2 sets, the caller's generator, the sampling knobs
    model.config.eval_num_rays_per_chunk = 32
    gen = torch.Generator().manual_seed(5)
    out = model.get_laplace_pose_gradients_for_camera(cam, generator=gen, n_samples=3, prior_prec=2.0, eps=1e-8)
    assert out.shape == (H, W, 3, 4)
    assert draws[-1] == dict(n_samples=3, prior_prec=2.0, eps=1e-8, generator=gen, deterministic_density=False, n_sets=2)
    ws = seen[-1]["ws"]
    # (the colour head always draws its default 100 rows: laplace_field.py:516-520 forwards no knob to it)
    assert ws[0].shape == (2, 3, 65) and ws[1].shape == (2, 100, 195) and seen[-1]["scene"] == ("scene of", ws)
    assert seen[-1]["det"] is False and seen[-1]["c2w"] == (3, 4) and seen[-1]["W"] == W and seen[-1]["want_rgb"] is False
    # the same rows as the *_unc render draws from an equally seeded generator
    want = real(n_samples=3, prior_prec=2.0, eps=1e-8, generator=torch.Generator().manual_seed(5), deterministic_density=False, n_sets=2)
    assert torch.equal(ws[0], want[0]) and torch.equal(ws[1], want[1])
    # the model is left with its mean heads, and the device scene was dropped before and after
    assert model._ws is None and model._deterministic_density is False
    assert len(invalidated) == 2 and invalidated[0] is ws and invalidated[1] is None
    # one set per camera; through the plugin model; use_deterministic_density travels
    model.resample = "camera"
    g, rgb = pm.get_laplace_pose_gradients_for_camera(cam, generator=gen, use_deterministic_density=True, rays_per_launch=50, want_rgb=True)
    assert g.shape == (H, W, 3, 4) and rgb.shape == (H, W, 3)
    assert draws[-1]["n_sets"] is None and draws[-1]["deterministic_density"] is True and draws[-1]["n_samples"] == 100
    assert seen[-1]["det"] is True and seen[-1]["rays_per_launch"] == 50 and seen[-1]["ws"][0].dim() == 2
    assert model._ws is None and model._deterministic_density is False
    # a chunk size that is no multiple of 32: one set, with get_outputs_for_camera_unc's warning
    model.resample = "chunk"
    model.config.eval_num_rays_per_chunk = 50
    with pytest.warns(UserWarning, match="not a multiple of 32"):
        model.get_laplace_pose_gradients_for_camera(cam, generator=gen, n_samples=2)
    assert draws[-1]["n_sets"] is None
    # weight_samples: those rows, nothing drawn
    n_draws = len(draws)
    rows = (torch.zeros(4, 65), torch.ones(5, 195))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        model.get_laplace_pose_gradients_for_camera(cam, weight_samples=rows)
    assert len(draws) == n_draws and seen[-1]["ws"][0] is rows[0] and seen[-1]["ws"][1] is rows[1] and model._ws is None
    # the state is restored when the render raises
    monkeypatch.setattr(render, "pose_gradient_camera_laplace", lambda *a, **k: (_ for _ in ()).throw(RuntimeError("boom")))
    with pytest.raises(RuntimeError, match="boom"):
        model.get_laplace_pose_gradients_for_camera(cam, weight_samples=rows, use_deterministic_density=True)
    assert model._ws is None and model._deterministic_density is False
    # the old method keeps refusing, and says where to go
    with pytest.raises(NotImplementedError, match="colour is the mean") as ei:
        pm.get_pose_gradients_for_camera(cam)
    assert "get_laplace_pose_gradients_for_camera" in str(ei.value) and str(ei.value).endswith(".")
    # a mirror without the method
    other = _plugin_model("nerfacto-mcdropout")
    with pytest.raises(NotImplementedError, match="Laplace pose gradient"):
        other.get_laplace_pose_gradients_for_camera(cam)
    with pytest.raises(NotImplementedError, match="MC-dropout pose gradient"):
        pm.get_mc_pose_gradients_for_camera(cam)
