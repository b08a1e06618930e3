"""The rendered images of the eval harness on a machine without a GPU (scripts/eval_uncertainty.py:209-303, 85-98): the
jet table against matplotlib, `eval.pack_eval_images` against the route the reference takes, the PNG writer, the
refusals of unerf_eval_images_batch (all of them come before the first device call), and `run_eval` with
`save_rendered_images` on a stub model.  The kernel's bytes are held on the GPU (tests/test_gpu_eval_images.py)."""
import re

import numpy as np
import pytest
import torch

import eval_image_cases as K

SPOTS = {0: (0, 0, 128), 31: (0, 0, 255), 32: (0, 1, 255), 95: (19, 253, 228), 96: (22, 255, 225), 159: (225, 255, 22),
         160: (228, 255, 19), 223: (255, 34, 0), 224: (255, 30, 0), 255: (128, 0, 0)}


# ---------------------------------------------------------------- the colour table ----------------------------------

def test_jet_table_spot_entries_and_no_matplotlib_import():
    from uncertainty_nerf_gs_amd import colormaps
    assert colormaps.JET_U8.shape == (256, 3) and colormaps.JET_U8.dtype == np.uint8
    for k, rgb in SPOTS.items():
        assert tuple(int(v) for v in colormaps.JET_U8[k]) == rgb, k
    src = open(colormaps.__file__).read()
    assert not re.search(r"^\s*(import|from)\s+matplotlib", src, re.M)


def test_jet_table_equals_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    from uncertainty_nerf_gs_amd import colormaps
    want = K.q8(matplotlib.colormaps["jet"](np.arange(256))[:, :3])
    np.testing.assert_array_equal(colormaps.JET_U8, want)


# ---------------------------------------------------------------- the host definition -------------------------------

@pytest.mark.parametrize("unc", [(K.UNC_MIN, K.UNC_MAX), (K.UNC_MAX, K.UNC_MIN), (0.0, 1.0)])
def test_pack_eval_images_equals_the_matplotlib_route(unc):
    pytest.importorskip("matplotlib")
    from uncertainty_nerf_gs_amd import eval as E
    pred, gt, std = K.value_case(37, 53)
    got = E.pack_eval_images(pred, gt, std, *unc)
    want, a_max = K.matplotlib_route(pred, gt, std, *unc)
    assert a_max == 1.0 - 2.0 ** -52                                        # the largest pixel stays inside the last bin
    for name in K.PLANES:
        assert got[name].dtype == np.uint8 and got[name].shape == want[name].shape
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    flat = got["std"].reshape(-1, 3)
    assert tuple(flat[22]) == (0, 0, 0)                                     # the NaN std pixel
    assert tuple(flat[18]) == SPOTS[0] and tuple(flat[19]) == SPOTS[255]    # std 0 and std above the range
    assert got["pred"].reshape(-1, 3)[13, 0] == 0 and got["err"].reshape(-1)[13] == 0   # the NaN pred pixel


def test_pack_eval_images_values_by_hand():
    from uncertainty_nerf_gs_amd import eval as E
    pred, gt, std = K.value_case(5, 8)
    got = E.pack_eval_images(pred, gt, std[..., None], K.UNC_MIN, K.UNC_MAX)    # [H, W, 1] std as the models return it
    p8, t8, e8 = got["pred"].reshape(-1, 3), got["gt"].reshape(-1, 3), got["err"].reshape(-1)
    assert tuple(p8[1]) == (0, 255, 0) and tuple(p8[2]) == (255, 0, 255)     # below 0, above 1
    assert tuple(p8[3]) == (128, 127, 128) and tuple(t8[4]) == (128, 127, 128)   # 0.5 * 255 + 0.5 == 128 exactly
    assert tuple(e8[9:13]) == (255, 255, 255, 0)
    s8 = got["std"].reshape(-1, 3)
    assert tuple(s8[14]) == tuple(s8[16]) == tuple(s8[18]) == tuple(s8[21]) == SPOTS[0]      # at and below unc_min
    assert tuple(s8[15]) == tuple(s8[17]) == tuple(s8[19]) == tuple(s8[20]) == SPOTS[255]    # at and above unc_max, +inf


def test_constant_and_all_nan_std_images():
    from uncertainty_nerf_gs_amd import eval as E
    pred, gt, _ = K.value_case(5, 8)
    const = E.pack_eval_images(pred, gt, np.full((5, 8), 0.3, np.float32), K.UNC_MIN, K.UNC_MAX)["std"]
    assert (const.reshape(-1, 3) == np.array(SPOTS[0])).all()                # a = 0 everywhere
    nan = E.pack_eval_images(pred, gt, np.full((5, 8), np.nan, np.float32), K.UNC_MIN, K.UNC_MAX)["std"]
    assert not nan.any()


def test_an_empty_uncertainty_range_raises(tmp_path):
    from uncertainty_nerf_gs_amd import eval as E, ops
    pred, gt, std = K.value_case(5, 8)
    with pytest.raises(ValueError, match="unc_max == unc_min"):
        E.pack_eval_images(pred, gt, std, 0.3, 0.3)
    with pytest.raises(ValueError, match="unc_max == unc_min"):
        E.save_imgs_rgb([0], [{"rgb": torch.from_numpy(pred), "rgb_std": torch.from_numpy(std)}], [torch.from_numpy(gt)],
                        tmp_path / "plots", 0.3, 0.3)
    assert not (tmp_path / "plots").exists()
    x = torch.zeros(1, 4, 4, 3)
    with pytest.raises(ValueError, match="unc_max == unc_min"):
        ops.eval_images(x, x, torch.ones(1, 4, 4), 1.0, 1.0)
    with pytest.raises(ValueError, match="unc_max == unc_min"):
        E.get_average_uncertainty_metrics(lambda cam: cam, [], save_rendered_images=True, plots_path=tmp_path, unc_min=2.0,
                                          unc_max=2.0)


# ---------------------------------------------------------------- the PNG writer ------------------------------------

@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (37, 53), (1, 1, 3), (5, 7, 3), (37, 53, 3)])
def test_write_png_round_trips(tmp_path, shape):
    from uncertainty_nerf_gs_amd import eval as E
    a = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    E._write_png(tmp_path / "a.png", a)
    back = K.decode_png(tmp_path / "a.png")
    assert back.shape == a.shape
    np.testing.assert_array_equal(back, a)


def test_write_png_refuses_what_it_cannot_write(tmp_path):
    from uncertainty_nerf_gs_amd import eval as E
    for bad in (np.zeros((4, 4), np.float32), np.zeros((4, 4, 4), np.uint8), np.zeros((0, 4), np.uint8), np.zeros(4, np.uint8)):
        with pytest.raises(ValueError, match="_write_png"):
            E._write_png(tmp_path / "b.png", bad)


def test_written_png_is_read_by_matplotlib(tmp_path):
    image = pytest.importorskip("matplotlib.image")
    from uncertainty_nerf_gs_amd import eval as E
    a = np.random.default_rng(3).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    E._write_png(tmp_path / "c.png", a)
    np.testing.assert_array_equal(K.q8(image.imread(tmp_path / "c.png")), a)


# ---------------------------------------------------------------- the ABI -------------------------------------------

def test_entry_point_is_exported_and_typed(lib):
    h = lib.load()
    for name in ("unerf_eval_images_workspace_bytes", "unerf_eval_images_batch"):
        assert name in lib.SIGNATURES and getattr(h, name) is not None
    hdr = open(lib.INCLUDE + "/unerf.h").read()
    decl = re.search(r"int unerf_eval_images_batch\((.*?)\);", hdr, re.S).group(1)
    assert len(lib.SIGNATURES["unerf_eval_images_batch"][1]) == len(decl.split(",")) == 15
    assert len(lib.SIGNATURES["unerf_eval_images_workspace_bytes"][1]) == 1
    assert h.unerf_version() == lib.ABI_VERSION == 1420                     # an additive change
    assert all(h.unerf_eval_images_workspace_bytes(B) >= 8 * B for B in (1, 2, 16, 64))


def _call(h, n=100, B=2, lo=0.0, span=1.0, ws_bytes=None, ptr=0x1000, lut=0x1000, ws=0x1000, planes=(0x1000,) * 4):
    """fake (never dereferenced) device pointers: every refusal comes before the first device call"""
    if ws_bytes is None:
        ws_bytes = h.unerf_eval_images_workspace_bytes(max(B, 1))
    return h.unerf_eval_images_batch(ptr, ptr, ptr, n, B, lo, span, lut, *planes, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,needle", [
    (dict(B=0), "B = 0"), (dict(B=65), "B = 65"), (dict(B=-1), "B = -1"),
    (dict(span=0.0), "unc_span = 0"), (dict(span=-1.0), "unc_span = -1"), (dict(span=float("nan")), "unc_span"),
    (dict(span=float("inf")), "unc_span"), (dict(lo=float("nan")), "unc_lo"),
    (dict(ws_bytes=0), "unerf_eval_images_workspace_bytes(2)"), (dict(B=64, ws_bytes=64 * 8 - 1), "unerf_eval_images_workspace_bytes(64)"),
    (dict(n=-1), "n = -1"), (dict(n=(1 << 31) // 3 + 1), "2^31"),
    (dict(ptr=None), "null pointer"), (dict(lut=None), "null pointer"), (dict(ws=None), "null pointer"),
    (dict(ws=0x1002), "4-byte aligned"),
])
def test_refusals_come_before_any_device_call(lib, kw, needle):
    h = lib.load()
    assert _call(h, **kw) == -1
    msg = h.unerf_last_error().decode()
    assert needle in msg and msg.startswith("eval_images_batch:"), msg


def test_zero_pixels_and_no_planes_are_successful_no_ops(lib):
    h = lib.load()
    assert _call(h, n=0, B=3, ptr=None, lut=None, ws=None, ws_bytes=0, planes=(None,) * 4) == 0
    assert _call(h, n=100, B=3, planes=(None,) * 4) == 0


def test_binding_refuses_cpu_tensors_and_bad_shapes(lib):
    from uncertainty_nerf_gs_amd import ops
    x, s = torch.zeros(2, 4, 4, 3), torch.ones(2, 4, 4)
    with pytest.raises(lib.UnerfError, match="no CPU path"):
        ops.eval_images(x, x, s, 0.0, 1.0)
    with pytest.raises(lib.UnerfError, match="eval_images: pred"):
        ops.eval_images(x, x[:, :3], s, 0.0, 1.0)
    with pytest.raises(lib.UnerfError, match="eval_images: pred"):
        ops.eval_images(x[..., :2], x[..., :2], s, 0.0, 1.0)
    with pytest.raises(lib.UnerfError, match="want"):
        ops.eval_images(x, x, s, 0.0, 1.0, want=("gt", "depth"))
    big = torch.zeros(lib.METRICS_MAX_IMAGES + 1, 2, 3)
    with pytest.raises(lib.UnerfError, match="B = 65"):
        ops.eval_images(big, big, torch.ones(lib.METRICS_MAX_IMAGES + 1, 2), 0.0, 1.0)


# ---------------------------------------------------------------- the harness ---------------------------------------

def _eval_set(n=3, H=20, W=24):
    g = torch.Generator().manual_seed(0)
    items = []
    for i in range(n):
        gt = torch.rand(H, W, 3, generator=g)
        std = 0.02 + 0.7 * torch.rand(H, W, 1, generator=g)
        std[1, 1] = 0.9                                                      # above UNC_MAX
        rgb = torch.clamp(gt + 0.1 * torch.randn(H, W, 3, generator=g), -0.1, 1.2)
        items.append(({"rgb": rgb, "rgb_std": std, "accumulation": torch.ones(H, W, 1)}, gt))
    return items


class _Model:
    def get_outputs_for_camera(self, cam):
        return cam


def _run_eval(tmp_path, name, items, **cfg):
    from uncertainty_nerf_gs_amd import eval as E
    ecfg = E.ActiveNerfactoConfig(output_path=tmp_path / name / "metrics.json", eval_depth=False, **cfg)
    return E.run_eval(ecfg, _Model(), [(o, gt) for o, gt in items], method_name="active-nerfacto")


def test_run_eval_saves_the_rendered_images(tmp_path):
    from uncertainty_nerf_gs_amd import eval as E
    items = _eval_set()
    off = _run_eval(tmp_path, "off", items)
    assert sorted(p.name for p in (tmp_path / "off").iterdir()) == ["metrics.json"]       # no plots directory
    on = _run_eval(tmp_path, "on", items, save_rendered_images=True, unc_min=K.UNC_MIN, unc_max=K.UNC_MAX)
    assert list(on) == list(off)
    plots = tmp_path / "on" / "plots"
    images = sorted(p.name for p in plots.iterdir() if not p.name.startswith("plot_"))
    assert images == sorted(f"{i}_rgb_{what}.png" for i in range(3) for what in ("gt", "pred", "abs_err", "std"))
    for i, (o, gt) in enumerate(items):
        want = E.pack_eval_images(o["rgb"].numpy(), gt.numpy(), o["rgb_std"].numpy(), K.UNC_MIN, K.UNC_MAX)
        for plane, stem in (("gt", "rgb_gt"), ("pred", "rgb_pred"), ("err", "rgb_abs_err"), ("std", "rgb_std")):
            np.testing.assert_array_equal(K.decode_png(plots / f"{i}_{stem}.png"), want[plane], err_msg=f"{i} {stem}")
    for k in on:
        if k not in ("num_rays_per_sec", "fps", "render_rays_per_sec"):
            assert on[k] == off[k], k


def test_run_eval_writes_the_test_set_plots_with_matplotlib(tmp_path):
    image = pytest.importorskip("matplotlib.image")
    _run_eval(tmp_path, "on", _eval_set(2), save_rendered_images=True)
    plots = tmp_path / "on" / "plots"
    assert sorted(p.name for p in plots.iterdir() if p.name.startswith("plot_")) == [f"plot_rgb_{et}_all.png" for et in ("mae", "mse", "rmse")]
    assert image.imread(plots / "plot_rgb_mse_all.png").ndim == 3


def test_no_plots_and_one_line_without_matplotlib(tmp_path, monkeypatch, capsys):
    import sys
    from uncertainty_nerf_gs_amd import eval as E
    for name in [m for m in sys.modules if m == "matplotlib" or m.startswith("matplotlib.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "matplotlib", None)                     # `import matplotlib...` now raises ImportError
    curves = {f"rgb_all{v}_ause_{et}": np.zeros(100) for v in ("", "_var") for et in ("mse", "rmse", "mae")}
    assert E.save_sparsification_plots(tmp_path / "plots", curves) == []
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "matplotlib is not installed" in out and not (tmp_path / "plots").exists()


def test_images_are_saved_only_with_rgb_uncertainty(tmp_path):
    from uncertainty_nerf_gs_amd import eval as E
    items = _eval_set(1)
    avg, _ = E.get_average_uncertainty_metrics(lambda cam: cam, items, eval_rgb_unc=False, save_rendered_images=True,
                                               plots_path=tmp_path / "plots")
    assert set(avg) == {"psnr", "ssim", "num_rays_per_sec", "fps", "render_rays_per_sec"} and not (tmp_path / "plots").exists()
    with pytest.raises(ValueError, match="plots_path"):
        E.get_average_uncertainty_metrics(lambda cam: cam, items, save_rendered_images=True)


def test_a_splat_ground_truth_is_saved_as_the_metrics_see_it(tmp_path):
    from uncertainty_nerf_gs_amd import eval as E, models as Mo
    m = Mo.ActiveSplatfactoModel(Mo.ActiveSplatfactoModelConfig(), num_points=4)
    g = torch.Generator().manual_seed(2)
    bg = torch.tensor([0.1, 0.2, 0.9])
    rgba = torch.cat([torch.rand(6, 9, 3, generator=g), (torch.rand(6, 9, 1, generator=g) > 0.5).float()], -1)
    out = {"rgb": torch.rand(6, 9, 3, generator=g), "rgb_std": torch.rand(6, 9, 1, generator=g), "background": bg}
    packed = E.save_imgs_rgb([7], [out], [rgba], tmp_path / "plots", composite_gt=m.composite_gt)
    want = K.q8(m.composite_gt(rgba, bg)[..., :3].numpy())
    np.testing.assert_array_equal(K.decode_png(tmp_path / "plots" / "7_rgb_gt.png"), want)
    np.testing.assert_array_equal(packed[7]["gt"], want)
