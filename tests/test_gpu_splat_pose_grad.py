"""The splat pose gradient on the GPU, part by part, against the float64 references of tests/splat_pose_grad_cases.py:

  1. splat_pose_tangents_kernel alone on planted projections (clip threshold, fov limits, a needle, a zero covariance, a splat
     behind the camera, an empty tile box): all 6 x 12 entries of every live splat, dead splats exactly 0;
  2. splat_pose_grad_kernel alone on hand-built lists with random tangents: list lengths around the staging batch, stops at
     batch boundaries, overhanging tiles, block_width 8, quadrant culling, alpha on its clamp, bright / dim colours, every
     background, classic against antialiased, the raw dV output against the c2w epilogue;
  3. whole frames through the models, the plugin's classes and posegrad.export_pose_gradients.

A result's error is max |g - g64| / rms(g64) over the compared elements; the kernel is allowed KERNEL_FACTOR = 4 x the error of
the same restatement run in float32.  The forward rgb is held to the float64 blend within test_gpu_splat_raster_edges' 8 x E32.
Every test prints its ratios (DESIGN.md 4.6b records them)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import splat_pose_grad_cases as PC

pytestmark = pytest.mark.gpu
RASTER_FACTOR = 8.0
GUARD = 77.25


def _t(dev, a):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


def _ratio(what, got, r64, r32, keep):
    e32, err = PC.rel_error(r32, r64, keep), PC.rel_error(got, r64, keep)
    print(f"RATIO {what}: error {err:.3e} yardstick {e32:.3e} ratio {err / e32 if e32 > 0 else 0.0:.2f}")
    assert e32 > 0 and err <= PC.KERNEL_FACTOR * e32, f"{what}: error {err:.3e} > {PC.KERNEL_FACTOR} x yardstick {e32:.3e}"


def _rgb_bound(what, got, r64, r32):
    e32, err = float(np.abs(r32.astype(np.float64) - r64).max()), float(np.abs(got - r64).max())
    print(f"RATIO {what} rgb: error {err:.3e} E32 {e32:.3e} ratio {err / e32 if e32 > 0 else 0.0:.2f}")
    assert err <= RASTER_FACTOR * e32, f"{what} rgb: error {err:.3e} > {RASTER_FACTOR} x E32 {e32:.3e}"


# ---------------------------------------------------------------------------------------------------------------------
# 1. the tangent kernel
# ---------------------------------------------------------------------------------------------------------------------
def test_tangent_kernel_matches_the_jacobian(dev):
    from uncertainty_nerf_gs_amd import ops
    tc = PC.tangent_case()
    cam, N = tc.cam, tc.N
    args = (tc.V, tc.means, tc.proj["cov3d"], tc.pins, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    _, J64 = PC.tangents_ref(*args)
    _, J32 = PC.tangents_ref(*args, dtype=torch.float32)
    buf = torch.full((N * 72 + 64,), GUARD, device=dev)
    means, cov3d, radii = _t(dev, tc.means), _t(dev, tc.proj["cov3d"]), _t(dev, tc.proj["radii"])
    call = lambda out: ops.splat_pose_tangents(means, cov3d, radii, torch.from_numpy(tc.V), cam["fx"], cam["fy"], cam["cx"], cam["cy"],
                                               cam["H"], cam["W"], clip_thresh=PC.TAN_CLIP, out=out)
    with torch.cuda.device(dev):
        got_t = call(buf[:N * 72].view(N, 6, 12))
        again = call(None)
        torch.cuda.synchronize()
    assert (buf[N * 72:] == GUARD).all(), "floats behind the array were written"
    assert torch.equal(got_t, again), "two calls must return the same bits"
    got = got_t.cpu().numpy()
    live = tc.proj["radii"] > 0
    assert np.isfinite(got).all() and (got[~live] == 0).all(), "dead splats must be exactly 0"
    # per projected quantity (they have different units): every entry of every live splat
    for q, name in enumerate(("u", "v", "conic_a", "conic_b", "conic_c", "comp")):
        _ratio(f"tangents {name}", got[:, q], J64[:, q], J32[:, q], live)
    # ... and row by row, each 12-vector against its OWN rms, so that the needle's tangents (1e4 x the others') cannot hide a
    # wrong row: the yardstick is the worst row of the float32 restatement by the same measure.  The needle itself is left to
    # the case-wide measure above: its det_orig is 1e-12 of the products it is the difference of, and the float32 restatement
    # is off by 230 % of the row there (conic c).
    rows = live.copy()
    rows[tc.plants["needle"]] = False
    rms = np.sqrt((J64 ** 2).mean(-1))
    row_err = lambda J: np.abs(J - J64).max(-1)[rows] / np.where(rms > 0, rms, 1.0)[rows]
    assert (got[rms == 0] == 0).all(), "a 12-vector that is exactly 0 in the reference (the flat splat's compensation) must be 0"
    for q, name in enumerate(("u", "v", "conic_a", "conic_b", "conic_c", "comp")):
        e32, err = row_err(J32)[:, q].max(), row_err(got)[:, q]
        print(f"RATIO tangent rows {name}: worst {err.max():.3e} yardstick {e32:.3e} ratio {err.max() / e32:.2f}")
        worst = int(np.argmax(err))
        assert err.max() <= PC.KERNEL_FACTOR * e32, f"{name}: live row {worst}: {err.max():.3e} > 4 x {e32:.3e}"
    lib = __import__("uncertainty_nerf_gs_amd").lib.load()
    assert lib.unerf_splat_pose_tangents(None, None, None, 5, None, 1.0, 1.0, 0.0, 0.0, 8, 8, 0.01, None, None) == -1
    assert b"splat_pose_tangents: null pointer" in lib.unerf_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the walk kernel
# ---------------------------------------------------------------------------------------------------------------------
_DEV = {}


def _walk_tensors(dev, name):
    if name not in _DEV:
        c = PC.WALK[name]()
        _DEV[name] = {k: _t(dev, getattr(c, k)) for k in ("gids", "bins", "xys", "conics", "opac", "colors", "tan", "comp", "bg")}
    return _DEV[name]


def _walk(dev, name, aa, bg, c2w=None, cull=True, out=None, tan=None, comp=None):
    from uncertainty_nerf_gs_amd import ops
    c, t = PC.WALK[name](), _walk_tensors(dev, name)
    bgt = {"none": None, "black": torch.zeros(3, device=dev), "color": t["bg"]}[bg]
    return ops.splat_pose_grad(t["gids"], t["bins"], t["xys"], t["conics"], t["colors"], t["opac"], t["tan"] if tan is None else tan,
                               c.H, c.W, bgt, compensation=(t["comp"] if comp is None else comp) if aa else None,
                               c2w=None if c2w is None else torch.from_numpy(c2w), block_width=c.bw, cull=cull, want_rgb=True,
                               want_final_T=True, out=out)


WALKS = [(n, aa, "color") for n in PC.WALK for aa in (False, True)] + [("lists", True, "none"), ("lists", False, "black"),
                                                                        ("bright", True, "black"), ("stops", False, "none")]


@pytest.mark.parametrize("name,aa,bg", WALKS)
def test_walk_matches_f64(dev, name, aa, bg):
    c = PC.WALK[name]()
    r64, r32, keep = PC.walk_ref(name, aa, bg)
    with torch.cuda.device(dev):
        grad, rgb, fT = _walk(dev, name, aa, bg)
        plain = _walk(dev, name, aa, bg, cull=False)
        again = _walk(dev, name, aa, bg)
        torch.cuda.synchronize()
    for a, b, d in zip((grad, rgb, fT), plain, again):
        assert torch.equal(a, b), "culled and unculled walks must give the same bits"
        assert torch.equal(a, d), "two calls must return the same bits"
    assert grad.shape == (c.H, c.W, 12) and rgb.shape == (c.H, c.W, 3)
    what = f"{name} {'antialiased' if aa else 'classic'} bg={bg}"
    _ratio(what, grad.cpu().numpy(), r64.gV, r32.gV, keep)
    _rgb_bound(what, rgb.cpu().numpy(), r64.rgb, r32.rgb)
    _rgb_bound(what + " final_T", fT.cpu().numpy(), r64.T, r32.T)
    if name == "bright":     # a saturated pixel (all three channels at 1 or above) has gradient exactly 0
        sat = (r64.raw > 1 + PC.ONE_BAND).all(-1)
        assert sat.sum() > 0 and (grad.cpu().numpy()[sat] == 0).all()


def test_classic_equals_antialiased_with_unit_compensation(dev):
    c, t = PC.case_lists(), _walk_tensors(dev, "lists")
    tan0 = t["tan"].clone()
    tan0[:, 5] = 0.0
    with torch.cuda.device(dev):
        classic = _walk(dev, "lists", False, "color")
        aa = _walk(dev, "lists", True, "color", tan=tan0, comp=torch.ones_like(t["comp"]))
        torch.cuda.synchronize()
    for a, b in zip(classic, aa):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name,aa", [("lists", True), ("stops", False), ("bw8", True)])
def test_c2w_epilogue_guard_rows_and_side_stream(dev, name, aa):
    c = PC.WALK[name]()
    r64, r32, keep = PC.walk_ref(name, aa, "color")
    n = c.H * c.W * 12
    buf = torch.full((n + 48,), GUARD, device=dev)
    with torch.cuda.device(dev):
        raw, _, _ = _walk(dev, name, aa, "color")
        got, _, _ = _walk(dev, name, aa, "color", c2w=c.c2w, out=buf[:n].view(c.H, c.W, 3, 4))
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            on_side, _, _ = _walk(dev, name, aa, "color", c2w=c.c2w)
        side.synchronize()
    assert (buf[n:] == GUARD).all(), "rows behind out_grad were written"
    assert torch.equal(got, on_side)
    _ratio(f"{name} c2w epilogue", got.cpu().numpy(), PC.epilogue64(r64.gV, c.c2w), PC.epilogue64(r32.gV, c.c2w, np.float32), keep)
    # the kernel's own dV through the host's float64 epilogue: the two outputs differ by the epilogue's fp32 rounding only
    host = PC.epilogue64(raw.cpu().numpy(), c.c2w)
    scale = np.sqrt((host[keep] ** 2).mean())
    assert np.abs(got.cpu().numpy() - host).max() <= 16 * 2.0 ** -24 * max(scale, np.abs(host).max())


def test_walk_argument_checks(dev):
    from uncertainty_nerf_gs_amd import lib as L
    lib = L.load()
    assert lib.unerf_splat_pose_grad(None, None, None, None, None, None, None, None, None, None, 8, 8, 16, 0, None, None, None, None) == -1
    assert b"splat_pose_grad: null pointer" in lib.unerf_last_error()
    assert lib.unerf_splat_pose_grad(1, 1, 1, 1, 1, 1, None, 16, None, None, 8, 8, 17, 0, 16, None, None, None) == -1
    assert b"block_width" in lib.unerf_last_error()
    assert lib.unerf_splat_pose_grad(1, 1, 1, 1, 1, 1, None, 16, None, None, 8, 8, 16, 2, 16, None, None, None) == -1
    assert b"flags" in lib.unerf_last_error()
    assert lib.unerf_splat_pose_grad(1, 1, 1, 1, 1, 1, None, 4, None, None, 8, 8, 16, 0, 16, None, None, None) == -1
    assert b"aligned" in lib.unerf_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# 3. whole frames through the models
# ---------------------------------------------------------------------------------------------------------------------
class _Box:
    def within(self, pts):
        return (pts[:, 0] < 0.4)[:, None]


class _Nothing:
    def within(self, pts):
        return torch.zeros(pts.shape[0], 1, dtype=torch.bool, device=pts.device)


def _model(dev, f, active=True, through_plugin=False):
    from uncertainty_nerf_gs_amd import models, plugin
    if through_plugin:
        cfg = plugin.MODEL_CONFIGS["active-splatfacto" if active else "splatfacto"]()
    else:
        cfg = (models.ActiveSplatfactoModelConfig if active else models.SplatfactoModelConfig)()
    cfg.rasterize_mode = f.mode
    if f.sh0:
        cfg.sh_degree = 0
    m = cfg._target(cfg, num_points=4)
    m.load_state_dict({f"gauss_params.{k}": torch.from_numpy(v) for k, v in f.gp.items() if active or k != "log_uncertainties"})
    return m.to(dev).eval()


def _camera(f, c2w=None, **kw):
    cam = f.cam
    return SimpleNamespace(camera_to_worlds=torch.from_numpy(f.c2w if c2w is None else c2w)[None], fx=torch.tensor([cam["fx"]]),
                           fy=torch.tensor([cam["fy"]]), cx=torch.tensor([cam["cx"]]), cy=torch.tensor([cam["cy"]]),
                           height=cam["H"], width=cam["W"], **kw)


FRAMES = [(dict(mode="classic"), True, False), (dict(mode="antialiased"), True, False), (dict(mode="antialiased"), False, False),
          (dict(mode="classic", sh0=True), False, True), (dict(mode="antialiased", crop=True), True, True),
          (dict(mode="classic", sheared=True), True, False)]


@pytest.mark.parametrize("kw,active,through_plugin", FRAMES,
                         ids=lambda v: "-".join(f"{a}={b}" for a, b in v.items()) if isinstance(v, dict) else str(v))
def test_frame_through_the_model(dev, kw, active, through_plugin):
    f = PC.frame_case(**kw)
    r64, r32 = PC.frame_reference(f), PC.frame_reference(f, np.float32)
    m = _model(dev, f, active, through_plugin)
    H, W = f.cam["H"], f.cam["W"]
    box = _Box() if kw.get("crop") else None
    with torch.cuda.device(dev):
        frame = m.get_outputs_for_camera(_camera(f), obb_box=box)["rgb"]
        grad, rgb = m.get_pose_gradients_for_camera(_camera(f), want_rgb=True)
        only = m.get_pose_gradients_for_camera(_camera(f))
        torch.cuda.synchronize()
    assert grad.shape == (H, W, 3, 4) and grad.dtype == torch.float32 and grad.device.type == "cuda" and rgb.shape == (H, W, 3)
    assert torch.equal(grad, only)
    what = "frame " + " ".join(f"{a}={b}" for a, b in kw.items()) + (" active" if active else " plain")
    _ratio(what, grad.cpu().numpy(), r64.grad, r32.grad, r64.keep)
    _rgb_bound(what, rgb.cpu().numpy(), r64.rgb, r32.rgb)
    e32 = float(np.abs(r32.rgb.astype(np.float64) - r64.rgb).max())
    assert (frame - rgb).abs().max().item() <= RASTER_FACTOR * e32, "the gradient's colour is the frame the model renders"


def test_empty_frames_refusals_and_export(dev, tmp_path):
    from uncertainty_nerf_gs_amd import posegrad
    f = PC.frame_case(mode="classic")
    m = _model(dev, f)
    H, W = f.cam["H"], f.cam["W"]
    bg = torch.from_numpy(PC.FRAME_BG).to(dev)
    away = f.c2w.copy()
    away[:, 3] = (40.0, 0.0, 0.0)
    away[:, 2] = -away[:, 2]          # looks away from the splats: every one is behind the camera
    away[:, 0] = -away[:, 0]
    with torch.cuda.device(dev):
        for cam, box in ((_camera(f, away), None), (_camera(f), _Nothing())):
            m.set_crop(box)
            grad, rgb = m.get_pose_gradients_for_camera(cam, want_rgb=True)
            assert grad.shape == (H, W, 3, 4) and float(grad.abs().max()) == 0.0
            assert rgb.shape == (H, W, 3) and torch.equal(rgb, bg.expand(H, W, 3))
        m.set_crop(None)
        with pytest.raises(NotImplementedError, match="pinhole"):
            m.get_pose_gradients_for_camera(_camera(f, camera_type=2))
        two = _camera(f)
        two.camera_to_worlds = two.camera_to_worlds.repeat(2, 1, 1)
        with pytest.raises(ValueError, match="one camera"):
            m.get_pose_gradients_for_camera(two)
        files = posegrad.export_pose_gradients(m, _camera(f), 3, tmp_path, shift_param="tz", shift_magnitude=0.0)
        want, _ = m.get_pose_gradients_for_camera(_camera(f), want_rgb=True)
    shapes = {"c2w": ((3, 4), np.float32), "c2w_perturbed": ((3, 4), np.float32), "camera_intrinsics": ((3, 3), np.float32),
              "pred_rgb_perturbed": ((H, W, 3), np.float32), "c2w_grads_perturbed": ((H, W, 3, 4), np.float64)}
    assert set(files) == set(shapes) | {"image"}
    assert files["c2w"].name == "c2w_img3.npy" and files["image"].name == "image00003_perturbed.png" and files["image"].exists()
    for k, (shape, dt) in shapes.items():
        a = np.load(files[k])
        assert a.shape == shape and a.dtype == dt and files[k].name == (f"{k}.npy" if k != "c2w" else "c2w_img3.npy")
    np.testing.assert_array_equal(np.load(files["c2w_grads_perturbed"]), want.cpu().numpy().astype(np.float64))
