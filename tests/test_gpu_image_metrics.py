"""unerf_image_metrics on the GPU: the row of float64 results against the float64 restatement of
tests/test_metrics_abi_cpu.py (`restate_row`: float32 error definitions, float64 sums, stable sorts) and, finished by
`metrics.finish_metrics`, against the host functions (`metrics.ause`, `auce_torch`, `psnr`, `ssim`, the NLL) on CPU copies of
the same tensors; then `eval.run_eval(fused=True)` against `fused=False` on the three small eval sets of
tests/test_gpu_eval_harness.py and the oracle-render references.

Gates.  Plain sums, psnr: 1e-9 relative (1e-9 dB) -- float64 sums of <= 2^23 terms in another order differ by at most
n 2^-53 relative.  NLL: 1e-9 of the sum of the terms' magnitudes (the terms change sign with log s); the device's float64
log may sit a few ulp from the host's, the measured difference is printed.  AUCE counts: equal.  AUSE: 2e-6 absolute on
scalars and normalised curves against `metrics.ause` (the tolerance test_ause_matches_reference holds that function to),
1e-9 relative on the raw sums against the stable-sort restatement.  SSIM: 1e-9 against the float64 restatement;
`metrics.ssim` (float32, 121 taps) sits 1e-7 .. 6e-5 from it, printed."""
import json
import math

import numpy as np
import pytest
import torch

import test_metrics_abi_cpu as R
from conftest import golden

pytestmark = pytest.mark.gpu


def _images(H, W, Cc, seed, masked):
    """seeded random image pair: predictions above the clip, sigma == 0 with zero and with non-zero residual, a mask
    that removes about 10 % of the pixels"""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(H, W, Cc, generator=g)
    std = 0.02 + 0.2 * torch.rand(H, W, generator=g)
    pred = gt + std[..., None] * torch.randn(H, W, Cc, generator=g) + 0.05      # some values above 1
    flat_s, flat_p, flat_t = std.view(-1), pred.view(-1, Cc), gt.view(-1, Cc)
    flat_s[3:60:7] = 0.0                                                        # sigma == 0, residual != 0
    flat_s[5:80:9] = 0.0
    flat_p[5:80:9] = flat_t[5:80:9]                                             # sigma == 0, residual == 0
    mask = (torch.rand(H, W, generator=g) > 0.1) if masked else None
    return pred, gt, std, mask


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _check_row(row, ref, ex, n_z=99, n_r=100, what=""):
    from uncertainty_nerf_gs_amd import lib as L
    assert row[0] == ref[0] and row[1] == 0.0, (what, row[:2], ref[:2])
    for j, name in ((2, "sum sq"), (3, "sum ab"), (4, "sum var"), (5, "sum sigma"), (6, "sum sq64")):
        print(f"[{what}] {name}: fused {row[j]:.17g} restated {ref[j]:.17g} rel {_rel(row[j], ref[j]):.2e}")
        assert _rel(row[j], ref[j]) <= 1e-9, (what, name)
    d_nll = abs(row[7] - ref[7])
    print(f"[{what}] nll sum: fused {row[7]:.17g} restated {ref[7]:.17g} |diff| {d_nll:.3e} = {d_nll / ex['nll_abs_sum']:.2e} of sum|terms|")
    assert d_nll <= 1e-9 * ex["nll_abs_sum"], what
    np.testing.assert_array_equal(row[8:12], ref[8:12], err_msg=what + " min / max")
    a0 = L.METRICS_AUCE_OFF
    np.testing.assert_array_equal(row[a0:a0 + n_z], ref[a0:a0 + n_z], err_msg=what + " AUCE counts")
    s0 = L.METRICS_AUSE_OFF
    for f in range(4):
        got, want = row[s0 + 128 * f:s0 + 128 * f + n_r], ref[s0 + 128 * f:s0 + 128 * f + n_r]
        worst = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))
        print(f"[{what}] AUSE family {f}: worst relative difference of a raw sum {worst:.2e}")
        assert worst <= 1e-9, (what, f)
    assert np.all(row[14:16] == 0) and np.all(row[a0 + n_z:s0] == 0)             # unused slots stay zero


def _host_metrics(pred, gt, std, mask, clip, min_sigma):
    """the host functions on CPU tensors, as eval.image_metrics_unc / depth_metrics_unc string them together: the copy of
    the prediction clipped to `clip` feeds psnr alone, everything else takes the prediction as given"""
    from uncertainty_nerf_gs_amd import metrics as M
    Cc = pred.shape[-1]
    p = pred.reshape(-1, Cc)
    t, s = gt.reshape(-1, Cc), std.reshape(-1)
    if mask is not None:
        k = mask.reshape(-1)
        p, t, s = p[k], t[k], s[k]
    sq, ab, var = torch.sum((p - t) ** 2, -1), torch.sum((p - t).abs(), -1), s ** 2
    out, curves = {"psnr": M.psnr(torch.clamp(p, max=clip), t), "mse": float(sq.mean()), "avg_var": float(var.mean())}, {}
    for et, err in (("mae", ab), ("mse", sq), ("rmse", sq)):
        _, e, ev, a = M.ause(var, err, et)
        out[f"ause_{et}"], curves[f"ause_{et}"], curves[f"var_ause_{et}"] = float(a), e, ev
    out["nll"] = float(M.negative_gaussian_loglikelihood(p, t, s, eps=min_sigma).mean())
    a = M.auce_torch(p, s[:, None].repeat(1, Cc), t)
    out["auc_abs_error"], out["auc_length"], out["auc_neg_error"] = a["auc_abs_error_values"], a["auc_length_values"], a["auc_neg_error_values"]
    curves["coverage"] = a["coverage_values"]
    return out, curves


@pytest.mark.parametrize("H,W,Cc,masked", [(37, 53, 3, False), (37, 53, 1, True), (256, 256, 3, True), (256, 256, 1, False),
                                           (1080, 1920, 3, False)])
def test_row_matches_the_float64_restatement_and_the_host_functions(dev, H, W, Cc, masked):
    from uncertainty_nerf_gs_amd import lib as L, metrics as M, ops
    pred, gt, std, mask = _images(H, W, Cc, seed=H + Cc, masked=masked)
    clip, min_sigma = (1.0, 3e-2) if Cc == 3 else (float("inf"), 0.1)
    flags = L.METRICS_ALL & ~L.METRICS_SSIM
    dmask = mask.to(dev) if masked else None
    row_dev = ops.image_metrics(pred.to(dev), gt.to(dev), std.to(dev), dmask, clip_max=clip, nll_min_sigma=min_sigma, flags=flags)
    again = ops.image_metrics(pred.to(dev), gt.to(dev), std.to(dev), dmask, clip_max=clip, nll_min_sigma=min_sigma, flags=flags)
    assert torch.equal(row_dev, again), "two calls on the same inputs: the reductions run in a fixed order"
    row = row_dev.cpu().numpy()
    what = f"{H}x{W}x{Cc}{' masked' if masked else ''}"
    ref, ex = R.restate_row(pred, gt, std, mask, clip=clip, min_sigma=min_sigma)
    _check_row(row, ref, ex, what=what)
    # finished, against the host functions
    md, curves = M.finish_metrics(row, Cc, "rgb", flags)
    host, hcurves = _host_metrics(pred, gt, std, mask, clip, min_sigma)
    psnr64 = 10.0 * math.log10(1.0 / (ref[6] / (ref[0] * Cc)))
    assert abs(md["psnr"] - psnr64) <= 1e-9 and abs(md["psnr"] - host["psnr"]) <= 1e-9
    np.testing.assert_array_equal(curves["rgb_all_auce_coverage_values"], hcurves["coverage"])    # auce_torch's coverage
    n_el = ref[0] * Cc
    assert torch.equal(torch.from_numpy(row[L.METRICS_AUCE_OFF:L.METRICS_AUCE_OFF + 99]),
                       torch.from_numpy(np.rint(hcurves["coverage"] * n_el)))
    for et in ("mae", "mse", "rmse"):
        assert abs(md[f"rgb_ause_{et}"] - host[f"ause_{et}"]) <= 2e-6, (what, et, md[f"rgb_ause_{et}"], host[f"ause_{et}"])
        np.testing.assert_allclose(curves[f"rgb_all_ause_{et}"], hcurves[f"ause_{et}"], rtol=0, atol=2e-6)
        np.testing.assert_allclose(curves[f"rgb_all_var_ause_{et}"], hcurves[f"var_ause_{et}"], rtol=0, atol=2e-6)
    for k, hk in (("rgb_mse", "mse"), ("rgb_avg_var", "avg_var"), ("rgb_nll", "nll"), ("rgb_auc_length", "auc_length"),
                  ("rgb_auc_abs_error", "auc_abs_error"), ("rgb_auc_neg_error", "auc_neg_error")):
        print(f"[{what}] {k}: fused {md[k]:.12g}, host float32 path {host[hk]:.12g} (not gated: its own distance)")


def test_golden_vectors(dev):
    """the unc_* / err vectors of tests/golden/metrics.npz: pred = err, target = 0, C = 1 makes ab = err, sigma = sqrt(unc)
    makes var = unc up to a rounding that keeps the order.  `ause` treats mae / mse alike (means of the vector it is given),
    rmse takes their root: all three come from the ab families.  Against metrics.ause on the CPU and the stored reference
    values, 2e-6 each."""
    from uncertainty_nerf_gs_amd import lib as L, metrics as M, ops
    g = golden("metrics.npz")
    err = torch.from_numpy(g["err"]).float()
    assert float(err.min()) >= 0
    for tag in ("good", "bad"):
        unc = torch.from_numpy(g[f"unc_{tag}"]).float()
        assert float(unc.min()) >= 0
        sigma = unc.sqrt()
        row = ops.image_metrics(err[:, None].to(dev), torch.zeros_like(err)[:, None].to(dev), sigma.to(dev), nll_min_sigma=1e-6,
                                flags=L.METRICS_AUSE).cpu().numpy()
        n = err.numel()
        keep = np.array([int((1 - r) * n) for r in M._RATIOS])
        fam = row[L.METRICS_AUSE_OFF:].reshape(4, 128)[:, :100]
        for et in ("rmse", "mae", "mse"):
            _, e, ev, a = M._ause_of_curves(M._curve_of_means(fam[1] / keep, et), M._curve_of_means(fam[3] / keep, et))
            _, e0, ev0, a0 = M.ause(sigma ** 2, err, et)
            assert abs(a - a0) <= 2e-6 and abs(a - float(g[f"ause_{tag}_{et}"])) <= 2e-6, (tag, et, a, a0)
            np.testing.assert_allclose(e, e0, rtol=0, atol=2e-6)
            np.testing.assert_allclose(ev, ev0, rtol=0, atol=2e-6)
            np.testing.assert_allclose(e, g[f"ause_{tag}_{et}_curve"], rtol=0, atol=2e-6)
            np.testing.assert_allclose(ev, g[f"ause_{tag}_{et}_curve_by_var"], rtol=0, atol=2e-6)


def test_ties_follow_the_defined_order(dev):
    """30 % of the pixels with sigma == 0 exactly and a block of equal errors that straddles several cut ranks: the sums
    over the first keep_k pixels depend on which of the tied pixels come first.  Defined: ascending key, ties by ascending
    pixel index = torch.sort(stable=True)."""
    from uncertainty_nerf_gs_amd import lib as L, ops
    H, W = 96, 128
    g = torch.Generator().manual_seed(11)
    gt = torch.rand(H, W, 3, generator=g)
    std = 0.05 + 0.1 * torch.rand(H, W, generator=g)
    std.view(-1)[torch.randperm(H * W, generator=g)[:int(0.3 * H * W)]] = 0.0
    pred = gt + 0.1 * torch.randn(H, W, 3, generator=g)
    tied = torch.randperm(H * W, generator=g)[:int(0.25 * H * W)]               # equal errors: a quarter of the image
    pred.view(-1, 3)[tied] = gt.view(-1, 3)[tied] + 0.0625
    row = ops.image_metrics(pred.to(dev), gt.to(dev), std.to(dev), nll_min_sigma=3e-2, flags=L.METRICS_AUSE | L.METRICS_AUCE).cpu().numpy()
    ref, ex = R.restate_row(pred, gt, std, min_sigma=3e-2)
    s0 = L.METRICS_AUSE_OFF
    for f in range(4):
        got, want = row[s0 + 128 * f:s0 + 128 * f + 100], ref[s0 + 128 * f:s0 + 128 * f + 100]
        worst = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))
        print(f"[ties] AUSE family {f}: worst relative difference of a raw sum {worst:.2e}")
        assert worst <= 1e-9, f
    np.testing.assert_array_equal(row[16:16 + 99], ref[16:16 + 99])


def _ssim_pairs():
    def noisy(x, g):
        return torch.clamp(x + 0.05 * torch.randn(x.shape, generator=g), 0, 1)

    def smooth(H, W):
        y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        return torch.stack([0.5 + 0.4 * torch.sin(x / (7.0 + 3 * c)) * torch.cos(y / (11.0 - 2 * c)) for c in range(3)], -1)

    g = torch.Generator().manual_seed(3)
    kinds = [("white noise 36x48", torch.rand(36, 48, 3, generator=g)), ("white noise 270x480", torch.rand(270, 480, 3, generator=g)),
             ("smooth 270x480", smooth(270, 480)), ("smooth 540x960", smooth(540, 960)),
             ("near-flat 200x200", 0.7 + 1e-3 * torch.randn(200, 200, 3, generator=g))]
    return [(name, noisy(img, g), img) for name, img in kinds]


def test_ssim_matches_the_float64_restatement(dev):
    from uncertainty_nerf_gs_amd import lib as L, metrics as M, ops
    for name, pred, gt in _ssim_pairs():
        H, W, _ = pred.shape
        std = torch.ones(H, W)
        row = ops.image_metrics(pred.to(dev), gt.to(dev), std.to(dev), image_hw=(H, W), clip_max=1.0, nll_min_sigma=3e-2,
                                flags=L.METRICS_SSIM).cpu().numpy()
        s, cnt = R.ssim_sum_f64(torch.clamp(pred, max=1.0), gt)
        fused, want, host = row[12] / row[13], s / cnt, M.ssim(pred, gt)
        print(f"[ssim] {name}: fused {fused:.12f} float64 restatement {want:.12f} |diff| {abs(fused - want):.2e}; "
              f"metrics.ssim (float32, 121 taps) sits {abs(host - want):.2e} from the restatement")
        assert row[13] == cnt == (H - 10) * (W - 10) * 3
        assert abs(fused - want) <= 1e-9, name
    with pytest.raises(L.UnerfError, match="H \\* W == n"):
        ops.image_metrics(pred.to(dev), gt.to(dev), std.to(dev), image_hw=(H, W - 1), nll_min_sigma=3e-2, flags=L.METRICS_SSIM)


def test_fused_rgb_metrics_and_workspace(dev):
    """the one-call host entry, with scratch from an ops.Workspace: same numbers as a fresh allocation"""
    from uncertainty_nerf_gs_amd import metrics as M, ops
    pred, gt, std, _ = _images(64, 80, 3, seed=5, masked=False)
    ws = ops.Workspace()
    a, ca = M.fused_rgb_metrics(pred.to(dev), std[..., None].to(dev), gt.to(dev), workspace=ws)
    b, cb = M.fused_rgb_metrics(pred.to(dev), std[..., None].to(dev), gt.to(dev))
    assert a == b and ws.nbytes() > 0
    for k in ca:
        np.testing.assert_array_equal(ca[k], cb[k])
    assert abs(a["ssim"] - M.ssim(torch.clamp(pred, max=1.0), gt)) <= 6e-5


def test_auce_torch_coverage_is_count_over_n_on_the_device(dev):
    """the host path's coverage is the correctly rounded count / n of metrics/auce.py on either device: the counts are
    divided on the host (a device tensor divided by a host scalar is multiplied by its reciprocal, one ulp off)"""
    from uncertainty_nerf_gs_amd import metrics as M
    pred, gt, std, _ = _images(36, 48, 3, seed=9, masked=False)                 # n = 5184: 1 / n is not a power of two
    p, t, s = pred.reshape(-1, 3), gt.reshape(-1, 3), std.reshape(-1, 1).repeat(1, 3)
    on_dev, on_cpu = M.auce_torch(p.to(dev), s.to(dev), t.to(dev)), M.auce_torch(p, s, t)
    np.testing.assert_array_equal(on_dev["coverage_values"], on_cpu["coverage_values"])
    counts = np.rint(on_cpu["coverage_values"] * p.numel())
    np.testing.assert_array_equal(on_dev["coverage_values"], counts / float(p.numel()))


# ---------------------------------------------------------------- end to end ---------------------------------------

AUSE_KEYS = ("rgb_ause_mae", "rgb_ause_mse", "rgb_ause_rmse")


def _per_image_agreement(outputs, gt, composite_gt=None):
    from uncertainty_nerf_gs_amd import eval as E, metrics as M
    md0, c0 = E.image_metrics_unc(outputs, gt, composite_gt=composite_gt)
    md1, c1 = E.image_metrics_unc(outputs, gt, composite_gt=composite_gt, fused=True)
    assert set(md0) == set(md1) and set(c0) == set(c1)
    for k in AUSE_KEYS:
        assert abs(md0[k] - md1[k]) <= 2e-6, (k, md0[k], md1[k])
    for k in ("rgb_mse", "rgb_avg_var", "rgb_auc_length"):
        assert abs(md0[k] - md1[k]) <= 1e-6 * abs(md0[k]), (k, md0[k], md1[k])
    np.testing.assert_array_equal(c0["rgb_all_auce_coverage_values"], c1["rgb_all_auce_coverage_values"])
    # ssim: within the host filter's own distance from the float64 restatement, + 1e-6
    rgb = torch.clip(outputs["rgb"], max=1.0).cpu()
    image = gt.to(outputs["rgb"].device)
    if composite_gt is not None and "background" in outputs:
        image = composite_gt(image, outputs["background"])
    s, cnt = R.ssim_sum_f64(rgb, image[..., :3].cpu())
    host_dist = abs(md0["ssim"] - s / cnt)
    print(f"[e2e] ssim fused {md1['ssim']:.9f} host {md0['ssim']:.9f}; host sits {host_dist:.2e} from the float64 restatement")
    assert abs(md1["ssim"] - md0["ssim"]) <= host_dist + 1e-6
    assert abs(md1["psnr"] - md0["psnr"]) <= 1e-9


@pytest.mark.parametrize("kind", ["active", "mcdropout"])
def test_run_eval_fused_on_hip_renders(dev, tmp_path, kind):
    from oracle import nerf_oracle as O
    from uncertainty_nerf_gs_amd import eval as E
    from uncertainty_nerf_gs_amd import models, synthetic
    import test_gpu_eval_harness as TH
    import test_gpu_models as TM
    H, W = TH.H, TH.W
    t = synthetic.make_scene_tensors(seed=21, kind=kind, log2T=14, prop_log2T=12)
    sc = O.scene_from_tensors(t)
    K, seed = 8, 0
    if kind == "active":
        cfg = TM._small_cfg(models.ActiveNerfactoModelConfig(average_init_density=0.01))
        ecfg = E.ActiveNerfactoConfig(load_config=None, output_path=tmp_path / "m.json", eval_depth=False)
    else:
        cfg = TM._small_cfg(models.NerfactoMCDropoutModelConfig(average_init_density=0.01, mc_samples=3))
        ecfg = E.MCDropoutConfig(load_config=None, output_path=tmp_path / "m.json", eval_depth=False, mc_samples=K)
    model = cfg._target(cfg, num_train_data=4)
    model.load_state_dict(TM._state_dict_from_tensors(t, kind))
    model = model.to(dev)
    refs, eval_set = [], []
    for i, cam in enumerate(TH._cams(3)):
        o, d, _ = O.generate_rays(cam.camera_to_worlds, cam.fx, cam.fy, cam.cx, cam.cy, H, W)
        if kind == "active":
            ref = O.render_camera(lambda oo, dd, off: O.active_outputs(sc, oo, dd), o, d)
        else:
            fs = models.frame_seed(seed, i)
            ref = O.render_camera(lambda oo, dd, off: O.mcdropout_outputs(sc, oo, dd, K, fs, 0.2, ray_offset=off), o, d)
        gt = TH._gt(ref["rgb"], 100 + i)
        refs.append(TH._cpu_reference_metrics(ref, gt))
        eval_set.append((cam, gt))
    got = E.run_eval(ecfg, model, eval_set, experiment_name="exp", method_name=kind, checkpoint="ckpt", fused=True)
    TH._check(got, refs)
    assert "ssim" in got and json.loads((tmp_path / "m.json").read_text())["results"]["psnr"] == got["psnr"]
    # the same key set as the host path, and agreement with it image by image on one render each
    fn = E.outputs_fn_for(ecfg, model)
    outputs = fn(eval_set[0][0])
    _per_image_agreement(outputs, eval_set[0][1])
    host = E.run_eval(ecfg, model, eval_set[:1], fused=False)
    assert set(host) == set(got)


def test_run_eval_fused_splat(dev, tmp_path):
    from uncertainty_nerf_gs_amd import eval as E
    from oracle import splat_oracle as SO
    import test_gpu_eval_harness as TH
    import test_gpu_splat as TS
    m, cam, g = TS._fixture_model(dev)
    gp = {k[3:]: g[k] for k in g.files if k.startswith("gp_")}
    fx, fy, cx, cy, Hs, Ws = g["intr"]
    ref = {k: torch.from_numpy(np.asarray(v)) for k, v in SO.active_splatfacto_outputs(
        gp, g["c2w"], fx, fy, cx, cy, int(Hs), int(Ws), np.array([0.1490, 0.1647, 0.2157], np.float32)).items() if not k.startswith("_")}
    gen = torch.Generator().manual_seed(5)
    rgba = torch.cat([TH._gt(ref["rgb"], 7), (torch.rand(int(Hs), int(Ws), 1, generator=gen) > 0.2).float()], dim=-1)
    refm = TH._cpu_reference_metrics(ref, m.composite_gt(rgba, ref["background"]).cpu())
    ecfg = E.ActiveSplatfactoConfig(load_config=None, output_path=tmp_path / "s.json")
    got = E.run_eval(ecfg, m, [(cam, rgba)], method_name="active-splatfacto", fused=True)
    TH._check(got, [refm], tol_ause=2e-3)
    host = E.run_eval(ecfg, m, [(cam, rgba)], method_name="active-splatfacto", fused=False)
    assert set(host) == set(got)
    _per_image_agreement(m.get_outputs_for_camera(cam), rgba, composite_gt=m.composite_gt)


def test_depth_metrics_fused_against_host(dev):
    """a masked, resized case like _depth_case of tests/test_eval_harness_cpu.py: GT 18x22 with invalid pixels, render
    12x16 (bilinear resize in front of the call), predictions clipped from below and from above"""
    from uncertainty_nerf_gs_amd import eval as E
    import test_eval_harness_cpu as TC
    out, gt, a = TC._depth_case(H=12, W=16)
    out = {k: v.to(dev) for k, v in out.items()}
    md0, c0 = E.depth_metrics_unc(out, gt, a, min_depth_std_for_nll=1.0)
    md1, c1 = E.depth_metrics_unc(out, gt, a, min_depth_std_for_nll=1.0, fused=True)
    assert set(md0) == set(md1) and set(c0) == set(c1)
    for k in ("depth_ause_mse", "depth_ause_mae", "depth_ause_rmse"):
        assert abs(md0[k] - md1[k]) <= 2e-6, (k, md0[k], md1[k])
    for k in ("depth_mse", "depth_rmse", "depth_avg_var", "depth_auc_length", "depth_nll"):
        assert abs(md0[k] - md1[k]) <= 1e-6 * abs(md0[k]), (k, md0[k], md1[k])
    np.testing.assert_array_equal(c0["depth_all_auce_coverage_values"], c1["depth_all_auce_coverage_values"])
    assert md0["depth_auc_abs_error"] == md1["depth_auc_abs_error"]
