"""The host route of the eval metrics against the reference's own per-image functions, from tests/golden/eval_rows.npz
alone (recorded by tests/golden/make_golden.py: get_unc_metrics_rgb, get_unc_metrics_depth,
get_image_metrics_and_images_unc and get_average_uncertainty_metrics of scripts/eval_uncertainty.py run on seeded images).
`eval.image_metrics_unc`, `eval.depth_metrics_unc` (fused=False) and the averaging of `eval.run_eval` are held to the
float32 recording -- the reference as it runs -- under the bounds of tests/eval_rows.py: key names and order, scalars,
curves, the AUCE arrays, NaN where the reference has NaN (fewer than 100 pixels: the last sparsification cuts keep nothing).

The cases plant what the restatements of the other test files could not tell apart from the reference: predictions above 1
(the reference clips a copy for psnr / ssim / lpips at :681 and computes every uncertainty metric from the render itself,
:316), exactly 1 and below 0, sigma below and on the NLL floor, sigma 0 with and without a residual, depths outside
[1e-3, max GT], GT == 0 pixels, a scale != 1, at the pixel counts on either side of the kernels' boundaries."""
import numpy as np
import pytest
import torch

import eval_rows as ER
from uncertainty_nerf_gs_amd import eval as E
from uncertainty_nerf_gs_amd import metrics as M

ROWS = ER.load()


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


@pytest.mark.parametrize("name", list(ROWS["rgb"]))
def test_rgb_metrics_match_get_unc_metrics_rgb(name, monkeypatch):
    c = ROWS["rgb"][name]
    H, W, _ = c["pred"].shape
    if min(H, W) <= 5:      # metrics.ssim reflect-pads by 5: no SSIM of so small an image, and none in the recording
        monkeypatch.setattr(M, "ssim", lambda pred, gt: float("nan"))
    md, curves = E.image_metrics_unc({"rgb": _t(c["pred"]), "rgb_std": _t(c["std"])}, _t(c["gt"]),
                                     min_rgb_std_for_nll=ROWS["min_std"]["rgb"])
    ER.check(md, curves, c, "f32", f"rgb {name} host")
    assert set(md) == set(c["f32"][0]) | {"psnr", "ssim"} and set(curves) == set(c["f32"][1])
    clipped = np.minimum(c["pred"], np.float32(1.0)).astype(np.float64)
    assert abs(md["psnr"] - 10.0 * np.log10(1.0 / np.mean((clipped - c["gt"].astype(np.float64)) ** 2))) <= 1e-9
    if H * W < 100:
        assert np.isnan(md["rgb_ause_mse"]) and np.isnan(curves["rgb_all_ause_mse"][-1]) and np.isfinite(curves["rgb_all_ause_mse"][0])
    ER.print_worst("host route")


@pytest.mark.parametrize("name", list(ROWS["depth"]))
def test_depth_metrics_match_get_unc_metrics_depth(name):
    c = ROWS["depth"][name]
    md, curves = E.depth_metrics_unc({"depth": _t(c["depth"]), "depth_std": _t(c["std"])}, c["gt"], c["scale"],
                                     min_depth_std_for_nll=ROWS["min_std"]["depth"])
    ER.check(md, curves, c, "f32", f"depth {name} host")
    assert set(md) == set(c["f32"][0]) and set(curves) == set(c["f32"][1])
    ER.print_worst("host route")


def test_the_cases_hold_what_they_are_there_for():
    """the plants are in the fixture, and the float32 and the float64 recording are two runs, not one"""
    rgb = ROWS["rgb"]
    assert sum(1 for c in rgb.values() if c["pred"].max() > 1) >= 10 and any(c["pred"].max() <= 1 for c in rgb.values())
    assert any(int((c["pred"] > 1).all(-1).sum()) >= 1 for c in rgb.values())
    assert all((c["pred"] == 1).any() and (c["pred"] < 0).any() and (c["std"] == 0).any() and (c["std"] == np.float32(0.03)).any()
               and (c["std"] < 0.03).any() for n, c in rgb.items() if not n.endswith("_b"))
    assert {c["pred"].shape[0] * c["pred"].shape[1] for c in rgb.values()} == {35, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097}
    depth = ROWS["depth"]
    assert {c["gt"].size for c in depth.values()} == {35, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097}
    for c in depth.values():
        scaled = c["scale"] * c["depth"][..., 0]
        assert c["scale"] != 1 and (scaled < 1e-3).any() and (scaled > c["gt"].max()).any() and (c["gt"] == 0).any() and (c["std"] == 0).any()
    assert any(0 < int((c["gt"] > 0).sum()) < 100 < c["gt"].size for c in depth.values())
    y = ER.yardsticks()
    assert y["rgb_mse"] > 0 and y["depth_nll"] > 0 and y["rgb_all_auce_coverage_values"] == 0


# ---------------------------------------------------------------- the frame: composition, key order, averaging -------

class _Weights:
    """stands in for checkpoints.LpipsWeights: the fake lpips below never opens it"""


def _fake_quality_metrics(monkeypatch):
    """psnr / ssim / lpips as the recorder's fake model has them: the maximum, the sum and the minimum of the prediction
    they are handed"""
    monkeypatch.setattr(M, "psnr", lambda pred, gt: float(pred.max()))
    monkeypatch.setattr(M, "ssim", lambda pred, gt: float(pred.sum()))
    monkeypatch.setattr(M, "lpips", lambda pred, gt, weights: float(pred.min()))


def _frame_outputs(im):
    return {k: _t(im[k]) for k in ("rgb", "rgb_std", "depth", "depth_std", "accumulation")}


def _frame_case(im):
    """a frame image's recording in the shape ER.check takes; the frame was recorded on float32 alone, which also stands in
    for the float64 values the one-ulp floor is taken from"""
    md = {k: v for k, v in im["metrics"].items() if k not in ("psnr", "ssim", "lpips", "num_rays_per_sec", "fps")}
    rec = (md, im["curves"], float("nan"))
    return {"f32": rec, "f64": rec}


def test_per_image_dictionary_matches_get_image_metrics_and_images_unc(monkeypatch):
    _fake_quality_metrics(monkeypatch)
    f = ROWS["frame"]
    for i, im in enumerate(f["images"]):
        out = _frame_outputs(im)
        assert float(out["rgb"].max()) > 1.0
        md, curves = E.image_metrics_unc(out, _t(im["image"]), min_rgb_std_for_nll=f["min_rgb_std"], lpips_weights=_Weights())
        dmd, dcurves = E.depth_metrics_unc(out, im["depth_gt"], f["scale"], min_depth_std_for_nll=f["min_depth_std"])
        # which copy each metric received: psnr / ssim / lpips the one clipped to <= 1 ...
        assert md["psnr"] == im["metrics"]["psnr"] == 1.0
        assert abs(md["ssim"] - im["metrics"]["ssim"]) <= ER.FACTOR * ER.ULP32 * abs(im["metrics"]["ssim"])
        assert abs(float(out["rgb"].sum()) - im["metrics"]["ssim"]) > 1.0      # ... the sum of the render itself is far off
        assert md["lpips"] == im["metrics"]["lpips"] < 0
        # ... and every uncertainty key the render as it is.  The NLL floor of ER.bound needs the mean |term|, which the
        # frame does not record: y_k of the per-function cases alone bounds it here
        case = _frame_case(im)
        merged = E._with_depth(md, dmd)
        curves.update(dcurves)
        nll_free = {k: v for k, v in case["f32"][0].items() if not k.endswith("_nll")}
        ER.check(merged, curves, {"f32": (nll_free, case["f32"][1], 0.0), "f64": (nll_free, case["f32"][1], 0.0)}, "f32", f"frame image {i}")
        for k in ("rgb_nll", "depth_nll"):
            assert abs(merged[k] - im["metrics"][k]) <= ER.FACTOR * ER.yardsticks()[k], (k, merged[k], im["metrics"][k])
        assert list(merged) == [k for k in f["keys"] if k not in ("num_rays_per_sec", "fps")]


def test_run_eval_averages_like_get_average_uncertainty_metrics(monkeypatch, tmp_path):
    """keys in the reference's order (`render_rays_per_sec`, this project's own, behind them); every average inside the
    worst per-image bound plus 4 float32 ulp of the largest per-image value (the reference's average is a float32
    torch.mean of float32 casts: a cast, two additions and a division, half an ulp each); the averaged curves are what
    the reference hands to plot_errors and plot_auce_curves"""
    _fake_quality_metrics(monkeypatch)
    f = ROWS["frame"]

    class Model:
        lpips_weights = _Weights()

        def get_outputs_for_camera(self, i):
            return _frame_outputs(f["images"][i])

    cfg = E.ActiveNerfactoConfig(output_path=tmp_path / "metrics.json", eval_depth=True, min_rgb_std_for_nll=f["min_rgb_std"],
                                 min_depth_std_for_nll=f["min_depth_std"])
    seen = {}
    real = E.get_average_uncertainty_metrics

    def spy(*a, **kw):
        seen["avg"], seen["curves"] = real(*a, **kw)
        return seen["avg"], seen["curves"]

    monkeypatch.setattr(E, "get_average_uncertainty_metrics", spy)
    got = E.run_eval(cfg, Model(), [(i, _t(im["image"])) for i, im in enumerate(f["images"])],
                     depth_gt_fn=lambda i: (f["images"][i]["depth_gt"], f["scale"]))
    assert list(got) == f["keys"] + ["render_rays_per_sec"]
    y = ER.yardsticks()
    for k in f["keys"]:
        if k in ("num_rays_per_sec", "fps"):
            continue
        per = np.array([im["metrics"][k] for im in f["images"]])
        if k in ("psnr", "lpips"):
            room = 0.0
        elif k == "ssim":
            room = ER.FACTOR * ER.ULP32 * np.abs(per).max()
        elif k.endswith("_nll"):
            room = ER.FACTOR * y[k]
        else:
            room = float(np.max([np.max(ER.bound(k, v, 0.0)) for v in per]))
        room += ER.FACTOR * ER.ULP32 * np.abs(per).max()
        print(f"[frame average] {k}: {got[k]:.9g} reference {f['avg'][k]:.9g} |difference| {abs(got[k] - f['avg'][k]):.2e} bound {room:.2e}")
        assert abs(got[k] - f["avg"][k]) <= room, (k, got[k], f["avg"][k], room)
    n_img = len(f["images"])
    for name, want in f["plots"].items():
        kind, output, rest = name.split("_", 2)
        if kind == "errors":                                # errors_rgb_mse_err / errors_rgb_mse_err_var
            et, which = rest.split("_", 1)
            ours = seen["curves"][f"{output}_all_{'var_' if which == 'err_var' else ''}ause_{et}"]
            np.testing.assert_allclose(ours, want, rtol=0, atol=ER.AUSE_GATE, err_msg=name)
        else:                                               # auce_rgb_coverage_values
            key = f"{output}_all_auce_{rest}"
            ours = seen["curves"][key]
            if any(key.endswith(c) for c in ER.COVERAGE):
                np.testing.assert_array_equal(ours, want, err_msg=name)
            else:
                per = [im["curves"][key] for im in f["images"]]
                room = np.max([ER.bound(key, v, 0.0) for v in per], axis=0)
                assert np.all(np.abs(ours - want) <= room), name
        assert np.asarray(want).shape == np.asarray(ours).shape
    assert n_img == 3 and len(f["plots"]) == 2 * (6 + 5)
