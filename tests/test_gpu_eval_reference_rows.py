"""The fused route of the eval metrics against the reference's own per-image functions run on float64 tensors, from
tests/golden/eval_rows.npz alone (see tests/test_eval_reference_rows_cpu.py for what the cases plant and tests/eval_rows.py
for the bounds: AUSE 2e-6 absolute, every other key 4 x the reference's own float32 - float64 distance, AUCE coverage and
counts equal).  Held to the float64 recording: `ops.image_metrics` + `metrics.finish_metrics`; `ops.image_metrics_batch`
with all cases of one shape stacked and with one batch of METRICS_MAX_IMAGES; `eval.image_metrics_unc(fused=True)`,
`image_metrics_unc_batch`, `depth_metrics_unc(fused=True)` and `depth_metrics_unc_batch`.

The recording has no psnr / ssim (get_unc_metrics_rgb computes neither): psnr is held to the float64 mean over the copy
clipped to <= 1 (which copy psnr takes is recorded by the frame part of the fixture and checked on the host route), and
the SSIM kernel needs min(H, W) >= 11, so the routes that always ask for it run the shapes that have it."""
import numpy as np
import pytest
import torch

import eval_rows as ER

pytestmark = pytest.mark.gpu

ROWS = ER.load()
RGB_BY_SHAPE, DEPTH_BY_SHAPE = {}, {}
for _name, _c in ROWS["rgb"].items():
    RGB_BY_SHAPE.setdefault(_c["pred"].shape[:2], []).append(_name)
for _name, _c in ROWS["depth"].items():
    DEPTH_BY_SHAPE.setdefault(_c["gt"].shape, []).append(_name)
WITH_SSIM = [n for n, c in ROWS["rgb"].items() if min(c["pred"].shape[:2]) >= 11]


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _no_ssim():
    from uncertainty_nerf_gs_amd import lib as L
    return L.METRICS_ALL & ~L.METRICS_SSIM


def _check_rgb_row(row, c, flags, what):
    """a finished rgb row against the float64 recording, the AUCE counts against coverage x (n C), psnr against float64"""
    from uncertainty_nerf_gs_amd import lib as L, metrics as M
    md, curves = M.finish_metrics(row, 3, "rgb", flags)
    ER.check(md, curves, c, "f64", what)
    n_el = c["pred"].size
    counts = np.rint(c["f64"][1]["rgb_all_auce_coverage_values"] * n_el)
    np.testing.assert_array_equal(row[L.METRICS_AUCE_OFF:L.METRICS_AUCE_OFF + 99], counts, err_msg=what + " AUCE counts")
    assert row[0] == n_el // 3 and row[1] == 0
    clipped = np.minimum(c["pred"], np.float32(1.0)).astype(np.float64)
    assert abs(md["psnr"] - 10.0 * np.log10(1.0 / np.mean((clipped - c["gt"].astype(np.float64)) ** 2))) <= 1e-9, what
    return md, curves


def _rgb_stack(dev, names):
    cs = [ROWS["rgb"][n] for n in names]
    return (_t(np.stack([c["pred"] for c in cs]), dev), _t(np.stack([c["gt"] for c in cs]), dev),
            _t(np.stack([c["std"][..., 0] for c in cs]), dev))


@pytest.mark.parametrize("name", list(ROWS["rgb"]))
def test_image_metrics_row_matches_get_unc_metrics_rgb(dev, name):
    from uncertainty_nerf_gs_amd import ops
    c = ROWS["rgb"][name]
    pred, gt, std = _rgb_stack(dev, [name])
    row = ops.image_metrics(pred[0], gt[0], std[0], None, clip_max=1.0, nll_min_sigma=ROWS["min_std"]["rgb"], flags=_no_ssim())
    md, curves = _check_rgb_row(row.cpu().numpy(), c, _no_ssim(), f"rgb {name} row")
    if c["pred"].size // 3 < 100:
        assert np.isnan(md["rgb_ause_mse"]) and np.isnan(curves["rgb_all_var_ause_mse"][-1])
    ER.print_worst("fused route")


@pytest.mark.parametrize("shape", list(RGB_BY_SHAPE), ids=lambda s: f"{s[0]}x{s[1]}")
def test_image_metrics_batch_of_one_shape(dev, shape):
    from uncertainty_nerf_gs_amd import ops
    names = RGB_BY_SHAPE[shape]
    pred, gt, std = _rgb_stack(dev, names)
    rows = ops.image_metrics_batch(pred, gt, std, None, clip_max=1.0, nll_min_sigma=ROWS["min_std"]["rgb"], flags=_no_ssim())
    rows = rows.cpu().numpy()
    assert rows.shape[0] == len(names)
    for b, name in enumerate(names):
        _check_rgb_row(rows[b], ROWS["rgb"][name], _no_ssim(), f"rgb {name} row {b} of a batch of {len(names)}")


def test_image_metrics_batch_of_max_images(dev):
    """METRICS_MAX_IMAGES images of 16 x 16, the three recorded cases of that shape in turn, every flag set"""
    from uncertainty_nerf_gs_amd import lib as L, ops
    names = (RGB_BY_SHAPE[(16, 16)] * L.METRICS_MAX_IMAGES)[:L.METRICS_MAX_IMAGES]
    assert len(set(names)) == 3
    pred, gt, std = _rgb_stack(dev, names)
    rows = ops.image_metrics_batch(pred, gt, std, None, image_hw=(16, 16), clip_max=1.0, nll_min_sigma=ROWS["min_std"]["rgb"],
                                   flags=L.METRICS_ALL).cpu().numpy()
    for b, name in enumerate(names):
        if b < 3 or b == L.METRICS_MAX_IMAGES - 1:
            _check_rgb_row(rows[b], ROWS["rgb"][name], L.METRICS_ALL, f"rgb {name} row {b} of {L.METRICS_MAX_IMAGES}")
        else:
            np.testing.assert_array_equal(rows[b], rows[b % 3], err_msg=f"row {b}")


def _outputs(dev, c):
    return {"rgb": _t(c["pred"], dev), "rgb_std": _t(c["std"], dev)}


@pytest.mark.parametrize("name", WITH_SSIM)
def test_image_metrics_unc_fused(dev, name):
    from uncertainty_nerf_gs_amd import eval as E
    c = ROWS["rgb"][name]
    md, curves = E.image_metrics_unc(_outputs(dev, c), _t(c["gt"], dev), min_rgb_std_for_nll=ROWS["min_std"]["rgb"], fused=True)
    ER.check(md, curves, c, "f64", f"rgb {name} image_metrics_unc(fused=True)")
    assert set(md) == set(c["f64"][0]) | {"psnr", "ssim"} and set(curves) == set(c["f64"][1])
    assert list(md)[:5] == ["psnr", "ssim", "rgb_ause_mse", "rgb_ause_mae", "rgb_ause_rmse"]


def test_image_metrics_unc_batch(dev):
    from uncertainty_nerf_gs_amd import eval as E
    names = RGB_BY_SHAPE[(16, 16)]
    cs = [ROWS["rgb"][n] for n in names]
    done = E.image_metrics_unc_batch([_outputs(dev, c) for c in cs], [_t(c["gt"], dev) for c in cs],
                                     min_rgb_std_for_nll=ROWS["min_std"]["rgb"])
    for name, c, (md, curves) in zip(names, cs, done):
        ER.check(md, curves, c, "f64", f"rgb {name} image_metrics_unc_batch")


def _depth_outputs(dev, c):
    return {"depth": _t(c["depth"], dev), "depth_std": _t(c["std"], dev)}


@pytest.mark.parametrize("name", list(ROWS["depth"]))
def test_depth_metrics_unc_fused(dev, name):
    from uncertainty_nerf_gs_amd import eval as E
    c = ROWS["depth"][name]
    md, curves = E.depth_metrics_unc(_depth_outputs(dev, c), c["gt"], c["scale"], min_depth_std_for_nll=ROWS["min_std"]["depth"],
                                     fused=True)
    ER.check(md, curves, c, "f64", f"depth {name} depth_metrics_unc(fused=True)")
    assert list(md) == list(c["f64"][0]) and set(curves) == set(c["f64"][1])
    ER.print_worst("fused route")


@pytest.mark.parametrize("shape", list(DEPTH_BY_SHAPE), ids=lambda s: f"{s[0]}x{s[1]}")
def test_depth_metrics_unc_batch(dev, shape):
    from uncertainty_nerf_gs_amd import eval as E
    names = DEPTH_BY_SHAPE[shape]
    cs = [ROWS["depth"][n] for n in names]
    done = E.depth_metrics_unc_batch([_depth_outputs(dev, c) for c in cs], [c["gt"] for c in cs], [c["scale"] for c in cs],
                                     min_depth_std_for_nll=ROWS["min_std"]["depth"])
    for name, c, (md, curves) in zip(names, cs, done):
        ER.check(md, curves, c, "f64", f"depth {name} depth_metrics_unc_batch of {len(names)}")
