"""Parity metrics: PSNR, AUSE, AUCE, Gaussian NLL.

Host-side mirror of nerfuncertainty/metrics/{ause,auce}.py and of the error definitions in
scripts/eval_uncertainty.py:306-412.  Unlike the reference (100 Python-loop slices + numpy on the
CPU, seconds per 1080p image), AUSE here is one sort + one prefix sum on whatever device the
tensors live on; results agree with the reference implementation to ~1e-7 (golden-vector test).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

_RATIOS = np.linspace(0, 1, 100, endpoint=False)


def _trapz(y: np.ndarray, x: np.ndarray) -> float:
    y = np.asarray(y, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    return float(np.sum((y[1:] + y[:-1]) * np.diff(x) / 2.0))


def _sparsification_curve(err_sorted: torch.Tensor, err_type: str) -> np.ndarray:
    n = err_sorted.numel()
    keep = torch.tensor([int((1 - r) * n) for r in _RATIOS], device=err_sorted.device, dtype=torch.long)
    csum = torch.cumsum(err_sorted.to(torch.float64), dim=0)
    means = csum[(keep - 1).clamp(min=0)] / keep.clamp(min=1).to(torch.float64)
    means = torch.where(keep > 0, means, torch.full_like(means, float("nan")))
    return _curve_of_means(means.cpu().numpy(), err_type)


def _curve_of_means(means: np.ndarray, err_type: str) -> np.ndarray:
    """float64 means of the kept errors (NaN where nothing is kept) -> the float32 curve: sqrt for rmse, in float64 and
    in front of the cast.  Shared by the sort-and-cumsum path above and by finish_metrics."""
    means = np.asarray(means, dtype=np.float64)
    if err_type == "rmse":
        means = np.sqrt(means)
    return means.astype(np.float32)


def _ause_of_curves(oracle: np.ndarray, by_var: np.ndarray, ratios: np.ndarray = _RATIOS):
    """the tail of metrics/ause.py:7-44: both float32 curves normalised by the larger maximum, the area between them.
    -> (ratio_removed, oracle_curve, by_variance_curve, ause)
    Fewer than 100 pixels: the last cuts keep nothing and their means are NaN.  The reference's built-in `max` walks each
    curve from its first (finite) entry and a NaN never compares greater, so the maximum is that of the finite entries:
    the curves are finite up to the empty cuts and NaN there, the area is NaN."""
    by_var = by_var.astype(np.float64)
    max_val = max(float(np.fmax.reduce(oracle)), float(np.fmax.reduce(by_var)))
    oracle = oracle / np.float32(max_val)
    by_var = by_var / max_val
    return ratios, oracle, by_var, _trapz(by_var - oracle, ratios)


def ause(unc_vec: torch.Tensor, err_vec: torch.Tensor, err_type: str = "rmse"):
    """metrics/ause.py:7-44.  -> (ratio_removed, oracle_curve, by_variance_curve, ause)"""
    assert err_type in ("rmse", "mae", "mse")
    err_sorted, _ = torch.sort(err_vec)
    oracle = _sparsification_curve(err_sorted, err_type)
    _, order = torch.sort(unc_vec)
    by_var = _sparsification_curve(err_vec[order], err_type)
    return _ause_of_curves(oracle, by_var)


def _norm_ppf(p: np.ndarray) -> np.ndarray:
    from scipy.stats import norm  # the reference uses scipy.stats.norm.ppf (auce.py:21-22)
    return norm.ppf(p)


def auce(mean_values: np.ndarray, sigma_values: np.ndarray, target_values: np.ndarray) -> Dict[str, np.ndarray]:
    """metrics/auce.py:10-57 (99 two-sided Gaussian intervals, alpha = 0.01..0.99)."""
    n = float(np.prod(target_values.shape))
    alphas = np.arange(start=0.01, stop=1.0, step=0.01)
    z = _norm_ppf(1.0 - alphas / 2)
    dev = np.abs(target_values - mean_values)
    coverage, length = [], []
    for zi in z:
        lo = mean_values - zi * sigma_values
        hi = mean_values + zi * sigma_values
        coverage.append(np.count_nonzero(np.logical_and(target_values >= lo, target_values <= hi)) / n)
        length.append(np.mean(hi - lo))
    coverage = np.array(coverage)
    length = np.array(length)
    cov_err = coverage - (1.0 - alphas)
    abs_err = np.abs(cov_err)
    neg_err = (np.abs(cov_err) - cov_err) / 2.0
    return {
        "coverage_values": coverage, "avg_length_values": length, "coverage_error_values": cov_err,
        "abs_coverage_error_values": abs_err, "neg_coverage_error_values": neg_err,
        "auc_abs_error_values": _trapz(abs_err, alphas), "auc_length_values": _trapz(length, alphas),
        "auc_neg_error_values": _trapz(neg_err, alphas),
    }


def auce_torch(mean_values: torch.Tensor, sigma_values: torch.Tensor, target_values: torch.Tensor) -> Dict[str, np.ndarray]:
    """`auce` on whatever device the tensors live on, in one sort: an interval [m - z s, m + z s] covers the
    target iff |t - m| / s <= z, so the 99 coverages are 99 binary searches into the sorted standardised residuals
    and the 99 mean interval lengths are 2 z mean(s).  Same dictionary as `auce` (the reference's 99-pass numpy
    loop, metrics/auce.py:10-57, takes ~1 s per 1080p image and would dominate the eval loop's rays/s); float64
    throughout, so the coverage counts agree with it except for residuals within 1e-16 of an interval edge."""
    m, sg, t = (x.detach().reshape(-1).to(torch.float64) for x in (mean_values, sigma_values, target_values))
    n = float(t.numel())
    alphas = np.arange(start=0.01, stop=1.0, step=0.01)
    z = torch.as_tensor(_norm_ppf(1.0 - alphas / 2), dtype=torch.float64, device=t.device)
    r = (t - m).abs()
    ratio = torch.where(sg > 0, r / sg, torch.where(r == 0, torch.zeros_like(r), torch.full_like(r, float("inf"))))
    ratio, _ = torch.sort(ratio)
    # the integer counts cross to the host and are divided there: torch divides a device tensor by a host scalar as a
    # multiplication by its reciprocal, one ulp off the reference's count / n for about half the counts
    coverage = torch.searchsorted(ratio, z, right=True).cpu().numpy().astype(np.float64) / n
    length = (2.0 * z * sg.mean()).cpu().numpy()
    return _auce_of_curves(coverage, length, alphas)


def _auce_of_curves(coverage: np.ndarray, length: np.ndarray, alphas: np.ndarray) -> Dict[str, np.ndarray]:
    """the tail of metrics/auce.py:10-57: coverage errors and the three integrals over alpha.  Shared by auce_torch and
    finish_metrics."""
    cov_err = coverage - (1.0 - alphas)
    abs_err = np.abs(cov_err)
    neg_err = (np.abs(cov_err) - cov_err) / 2.0
    return {
        "coverage_values": coverage, "avg_length_values": length, "coverage_error_values": cov_err,
        "abs_coverage_error_values": abs_err, "neg_coverage_error_values": neg_err,
        "auc_abs_error_values": _trapz(abs_err, alphas), "auc_length_values": _trapz(length, alphas),
        "auc_neg_error_values": _trapz(neg_err, alphas),
    }


def psnr(pred: torch.Tensor, gt: torch.Tensor) -> float:
    """torchmetrics PeakSignalNoiseRatio(data_range=1.0) as used via model.psnr
    (scripts/eval_uncertainty.py:683): 10*log10(1/mse) over all elements."""
    mse = torch.mean((pred.to(torch.float64) - gt.to(torch.float64)) ** 2).item()
    return 10.0 * math.log10(1.0 / mse)


def ssim(pred: torch.Tensor, gt: torch.Tensor, data_range=None) -> float:
    """torchmetrics.functional.structural_similarity_index_measure with its defaults, as reached through
    model.ssim (scripts/eval_uncertainty.py:684) on [1,3,H,W] images.  [UPSTREAM-RECALL, torchmetrics is absent
    here]: 11x11 gaussian window, sigma 1.5, k1 0.01, k2 0.03; inputs reflect-padded by 5, depthwise filtered
    (no further padding), the padded border cropped again, mean over everything; data_range=None means
    max(pred.max() - pred.min(), gt.max() - gt.min()).  Runs on the images' device."""
    p, t = pred.to(torch.float32), gt.to(torch.float32)
    if p.dim() == 3:  # [H,W,C] -> [1,C,H,W]
        p, t = p.permute(2, 0, 1)[None], t.permute(2, 0, 1)[None]
    if data_range is None:
        data_range = max(float(p.max() - p.min()), float(t.max() - t.min()))
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    ks, sigma, pad = 11, 1.5, 5
    d = torch.arange((1 - ks) / 2, (1 + ks) / 2, 1, dtype=p.dtype, device=p.device)
    g = torch.exp(-((d / sigma) ** 2) / 2)
    g = (g / g.sum())[None]
    C = p.shape[1]
    kernel = (g.t() @ g).expand(C, 1, ks, ks)
    p = torch.nn.functional.pad(p, (pad, pad, pad, pad), mode="reflect")
    t = torch.nn.functional.pad(t, (pad, pad, pad, pad), mode="reflect")
    stack = torch.cat((p, t, p * p, t * t, p * t))
    out = torch.nn.functional.conv2d(stack, kernel, groups=C)
    B = pred.shape[0] if pred.dim() == 4 else 1
    mu_p, mu_t, e_pp, e_tt, e_pt = out.split(B)
    s_pp, s_tt, s_pt = e_pp - mu_p ** 2, e_tt - mu_t ** 2, e_pt - mu_p * mu_t
    upper, lower = 2 * s_pt + c2, s_pp + s_tt + c2
    idx = ((2 * mu_p * mu_t + c1) * upper) / ((mu_p ** 2 + mu_t ** 2 + c1) * lower)
    return float(idx[..., pad:-pad, pad:-pad].mean().item())


LPIPS_NORM_EPS = 1e-8      # inside the square root of the channel norm (torchmetrics' _normalize_tensor)
LPIPS_MIN_SIDE = 31        # below it the second 3/2 max-pool of the AlexNet trunk has no output
LPIPS_LAYERS = 5


def lpips_map_sizes(H: int, W: int):
    """(h, w) of the five taps of the AlexNet trunk for an H x W image: conv1 11x11 / 4 / pad 2, max-pool 3 / 2 (floor),
    conv2 5x5 / pad 2, max-pool 3 / 2, conv3..5 3x3 / pad 1"""
    c1 = ((H + 4 - 11) // 4 + 1, (W + 4 - 11) // 4 + 1)
    p1 = ((c1[0] - 3) // 2 + 1, (c1[1] - 3) // 2 + 1)
    p2 = ((p1[0] - 3) // 2 + 1, (p1[1] - 3) // 2 + 1)
    return [c1, p1, p2, p2, p2]


def _lpips_operands(pred: torch.Tensor, target: torch.Tensor):
    """[H,W,3] / [B,H,W,3] pairs -> ([B,H,W,3] prediction clipped to <= 1, [B,H,W,3] target), checked as upstream's
    input check under normalize=True does it: every value in [0, 1], no NaN"""
    if pred.dim() == 3:
        pred, target = pred[None], target[None]
    if pred.dim() != 4 or pred.shape[-1] != 3 or target.shape != pred.shape:
        raise ValueError(f"lpips: pred {tuple(pred.shape)}, target {tuple(target.shape)}: expected two [H,W,3] or [B,H,W,3] images")
    H, W = int(pred.shape[1]), int(pred.shape[2])
    if min(H, W) < LPIPS_MIN_SIDE:
        raise ValueError(f"lpips: a {H} x {W} image; the AlexNet trunk needs min(H, W) >= {LPIPS_MIN_SIDE} "
                         "(below it the second max-pool has no output)")
    pred = torch.clip(pred, max=1.0)                        # eval_uncertainty.py:681
    for name, x in (("prediction", pred), ("target", target)):
        bad = int((~((x >= 0) & (x <= 1))).sum().item())    # a NaN fails both comparisons
        if bad:
            raise ValueError(f"lpips: {bad} values of the {name} are outside [0, 1] or NaN")
    return pred, target


def lpips_features(images: torch.Tensor, weights, dtype=torch.float32) -> List[torch.Tensor]:
    """the five ReLU taps [N, C_l, h_l, w_l] of the AlexNet trunk for images [N,H,W,3] in [0, 1], in `dtype`"""
    Fn = torch.nn.functional
    shift, scale, convs, _ = _lpips_tensors(weights, images.device, dtype)
    x = images.to(dtype).permute(0, 3, 1, 2)
    x = 2 * x - 1
    x = (x - shift) / scale
    taps = []
    for l, (stride, pad) in enumerate(((4, 2), (1, 2), (1, 1), (1, 1), (1, 1))):
        if l in (1, 2):
            x = Fn.max_pool2d(x, kernel_size=3, stride=2)
        x = torch.relu(Fn.conv2d(x, convs[l][0], convs[l][1], stride=stride, padding=pad))
        taps.append(x)
    return taps


def _lpips_tensors(weights, device, dtype):
    """the weights as `dtype` tensors on `device`, converted once per LpipsWeights object (its `_device` cache):
    (shift [1,3,1,1], scale [1,3,1,1], [(conv weight, bias)] * 5, [head weights [1,C,1,1]] * 5)"""
    key = ("torch", str(torch.device(device)), str(dtype))
    hit = weights._device.get(key)
    if hit is None:
        to = lambda t: t.to(device, dtype)
        hit = weights._device[key] = (to(weights.shift).view(1, 3, 1, 1), to(weights.scale).view(1, 3, 1, 1),
                                      [(to(w), to(b)) for w, b in weights.convs], [to(l).view(1, -1, 1, 1) for l in weights.lins])
    return hit


def lpips_per_image(pred: torch.Tensor, target: torch.Tensor, weights, dtype=torch.float32) -> torch.Tensor:
    """`lpips` per image of a batch -> [B] tensor of `dtype` on the images' device"""
    pred, target = _lpips_operands(pred, target)
    B = pred.shape[0]
    taps = lpips_features(torch.cat((pred, target)), weights, dtype)
    total = torch.zeros(B, dtype=dtype, device=pred.device)
    for f, lin in zip(taps, _lpips_tensors(weights, pred.device, dtype)[3]):
        f = f / torch.sqrt(LPIPS_NORM_EPS + torch.sum(f ** 2, dim=1, keepdim=True))
        d = (f[:B] - f[B:]) ** 2
        total = total + (d * lin).sum(dim=1).mean(dim=(1, 2))
    return total


def lpips(pred: torch.Tensor, target: torch.Tensor, weights, dtype=torch.float32) -> float:
    """torchmetrics LearnedPerceptualImagePatchSimilarity(net_type="alex", normalize=True) as reached through
    model.lpips (scripts/eval_uncertainty.py:681-689) on [H,W,3] or [B,H,W,3] images (a batch gives the mean over its
    images, the module's reduction), with `weights` a checkpoints.LpipsWeights.  [UPSTREAM-RECALL, torchmetrics is absent
    here]: x = 2 img - 1, then (x - shift) / scale; AlexNet features: conv 11x11 / 4 / pad 2, ReLU (tap), max-pool 3 / 2,
    conv 5x5 / pad 2, ReLU (tap), max-pool 3 / 2, three times conv 3x3 / pad 1 + ReLU (tap each); per tap
    f / sqrt(LPIPS_NORM_EPS + sum_c f^2) for both images, the squared difference, the head's 1x1 weights over the
    channels, the spatial mean; the five means are added.  The prediction is clipped to <= 1 first; a value outside
    [0, 1] or a NaN in either image raises ValueError, as does min(H, W) < LPIPS_MIN_SIDE.  Plain torch on the images'
    device: the CPU path, and with dtype=torch.float64 the yardstick the kernels behind ops.lpips_batch are held to."""
    return float(lpips_per_image(pred, target, weights, dtype).to(torch.float64).mean().item())


def finish_lpips(row_host) -> float:
    """one host copy of a row of ops.lpips_batch (include/unerf.h: unerf_lpips_batch) -> LPIPS: the five layer sums over
    their pixel counts, added.  Raises if the kernels counted a value outside [0, 1] or a NaN."""
    from . import lib as _l
    row = np.asarray(row_host, dtype=np.float64)
    bad = int(row[_l.LPIPS_BAD_OFF])
    if bad:
        raise ValueError(f"lpips: {bad} values of the prediction or the target are outside [0, 1] or NaN")
    return float(sum(row[l] / row[LPIPS_LAYERS + l] for l in range(LPIPS_LAYERS)))


def negative_gaussian_loglikelihood(preds: torch.Tensor, targets: torch.Tensor, stds: torch.Tensor,
                                    eps: float = 1e-6) -> torch.Tensor:
    """scripts/eval_uncertainty.py:404-412"""
    s = torch.clamp_min(stds.reshape(-1, 1), eps)
    c = preds.shape[-1]
    p, t = preds.reshape(-1, c), targets.reshape(-1, c)
    return ((t - p) ** 2) / (2 * s ** 2) + torch.log(s) + 0.5 * math.log(2 * math.pi)


def rgb_uncertainty_metrics(rgb_pred: torch.Tensor, rgb_std: torch.Tensor, rgb_gt: torch.Tensor,
                            min_rgb_std_for_nll: float = 3e-2) -> Dict[str, float]:
    """scripts/eval_uncertainty.py:306-402 without the plotting: error definitions, the three
    AUSE variants, NLL and AUCE for one image [H,W,3] / [H,W,1]."""
    sq = torch.sum((rgb_pred - rgb_gt) ** 2, dim=-1).flatten()
    ab = torch.sum(torch.abs(rgb_pred - rgb_gt), dim=-1).flatten()
    var = (rgb_std ** 2).flatten()
    out = {"avg_var": var.mean().item(), "psnr": psnr(rgb_pred, rgb_gt)}
    out["ause_mae"] = ause(var, ab, "mae")[3]
    out["ause_mse"] = ause(var, sq, "mse")[3]
    out["ause_rmse"] = ause(var, sq, "rmse")[3]
    out["nll_rgb"] = negative_gaussian_loglikelihood(rgb_pred.reshape(-1, 3), rgb_gt.reshape(-1, 3), rgb_std,
                                                     eps=min_rgb_std_for_nll).mean().item()
    std3 = var.sqrt().unsqueeze(-1).repeat(1, 3)
    a = auce(rgb_pred.reshape(-1, 3).cpu().numpy(), std3.cpu().numpy(), rgb_gt.reshape(-1, 3).cpu().numpy())
    out.update({k: v for k, v in a.items() if k.startswith("auc_")})
    return out


# ---- the fused path: one row of float64 partial results from the kernels (ops.image_metrics), finished here ----------

_AUCE_TABLES = None


def _auce_tables():
    """(alphas, z) of metrics/auce.py:10-57, computed once: alpha = 0.01 .. 0.99, z = norm.ppf(1 - alpha / 2)"""
    global _AUCE_TABLES
    if _AUCE_TABLES is None:
        alphas = np.arange(start=0.01, stop=1.0, step=0.01)
        _AUCE_TABLES = (alphas, np.ascontiguousarray(_norm_ppf(1.0 - alphas / 2), dtype=np.float64))
    return _AUCE_TABLES


_AUCE_CURVES = ("coverage_values", "avg_length_values", "coverage_error_values", "abs_coverage_error_values",
                "neg_coverage_error_values")


def metrics_row_from_sums(n_valid: int, sum_sq: float, sum_ab: float, sum_var: float, sum_sigma: float, sum_sq64: float,
                          nll_sum: float, pred_minmax, target_minmax, auce_counts, ause_sums, ssim_sum: float = 0.0,
                          ssim_count: float = 0.0, nonfinite: int = 0) -> np.ndarray:
    """a row in the layout of include/unerf.h (unerf_image_metrics) from its parts; ause_sums [4, n_ratios]"""
    from . import lib as _l
    row = np.zeros(_l.METRICS_ROW, dtype=np.float64)
    row[:14] = [n_valid, nonfinite, sum_sq, sum_ab, sum_var, sum_sigma, sum_sq64, nll_sum, pred_minmax[0], pred_minmax[1],
                target_minmax[0], target_minmax[1], ssim_sum, ssim_count]
    auce_counts = np.asarray(auce_counts, dtype=np.float64)
    row[_l.METRICS_AUCE_OFF:_l.METRICS_AUCE_OFF + auce_counts.size] = auce_counts
    for f, sums in enumerate(np.asarray(ause_sums, dtype=np.float64)):
        o = _l.METRICS_AUSE_OFF + _l.METRICS_MAX_CUTS * f
        row[o:o + sums.size] = sums
    return row


def finish_metrics(row_host, channels: int, prefix: str = "rgb", flags: Optional[int] = None, ratios: np.ndarray = _RATIOS,
                   with_psnr: bool = True):
    """One host copy of the row ops.image_metrics left on the device -> (metrics dict, curves dict) under the key names of
    eval.image_metrics_unc / depth_metrics_unc (`prefix` "rgb" or "depth"), pure numpy.  The means are quotients of the
    device's float64 sums; the curve tails are the helpers `ause` and `auce_torch` end in.  Raises if the kernels counted
    a non-finite input (the torch path's NaN ordering is not imitated)."""
    from . import lib as _l
    row = np.asarray(row_host, dtype=np.float64)
    flags = _l.METRICS_ALL if flags is None else flags
    n_valid, bad = int(row[0]), int(row[1])
    if bad:
        raise ValueError(f"{bad} of {n_valid} pixels have a non-finite prediction, target or standard deviation")
    if n_valid <= 0:
        raise ValueError("no valid pixel: nothing to average")
    md: Dict[str, float] = {}
    curves: Dict[str, np.ndarray] = {}
    if with_psnr:
        md["psnr"] = 10.0 * math.log10(1.0 / (row[6] / (n_valid * channels)))
    if flags & _l.METRICS_SSIM:
        md["ssim"] = float(row[12] / row[13])
    if flags & _l.METRICS_AUSE:
        keep = np.array([int((1 - r) * n_valid) for r in ratios], dtype=np.int64)
        with np.errstate(invalid="ignore", divide="ignore"):
            means = np.where(keep > 0, row[_l.METRICS_AUSE_OFF:_l.METRICS_AUSE_OFF + 4 * _l.METRICS_MAX_CUTS]
                             .reshape(4, _l.METRICS_MAX_CUTS)[:, :len(ratios)] / np.maximum(keep, 1), np.nan)
        # (error type, oracle family, by-variance family): sq sorted by sq / ab by ab; sq / ab sorted by variance
        for et, fo, fv in (("mse", 0, 2), ("mae", 1, 3), ("rmse", 0, 2)):
            _, e, ev, a = _ause_of_curves(_curve_of_means(means[fo], et), _curve_of_means(means[fv], et), ratios)
            md[f"{prefix}_ause_{et}"] = float(a)
            curves[f"{prefix}_all_ause_{et}"], curves[f"{prefix}_all_var_ause_{et}"] = e, ev
    md[f"{prefix}_mse"] = float(row[2] / n_valid)
    md[f"{prefix}_rmse"] = float(np.sqrt(row[2] / n_valid))
    if flags & _l.METRICS_NLL:
        md[f"{prefix}_nll"] = float(row[7] / (n_valid * channels))
    md[f"{prefix}_avg_var"] = float(row[4] / n_valid)
    if flags & _l.METRICS_AUCE:
        alphas, z = _auce_tables()
        coverage = row[_l.METRICS_AUCE_OFF:_l.METRICS_AUCE_OFF + len(z)] / float(n_valid * channels)
        a = _auce_of_curves(coverage, 2.0 * z * (row[5] / n_valid), alphas)
        md[f"{prefix}_auc_abs_error"], md[f"{prefix}_auc_length"] = a["auc_abs_error_values"], a["auc_length_values"]
        md[f"{prefix}_auc_neg_error"] = a["auc_neg_error_values"]
        for k in _AUCE_CURVES:
            curves[f"{prefix}_all_auce_{k}"] = a[k]
    return md, curves


def fused_rgb_metrics(rgb_pred: torch.Tensor, rgb_std: torch.Tensor, rgb_gt: torch.Tensor, min_rgb_std_for_nll: float = 3e-2,
                      clip_max: float = 1.0, with_ssim: bool = True, workspace=None):
    """`eval.image_metrics_unc`'s numbers for one image [H,W,C] on a HIP device through the fused kernels: one
    ops.image_metrics call, one copy of its row to the host, finish_metrics.  -> (metrics dict, curves dict)"""
    from . import lib as _l, ops
    H, W, Cc = rgb_pred.shape
    flags = _l.METRICS_ALL if with_ssim else _l.METRICS_ALL & ~_l.METRICS_SSIM
    row = ops.image_metrics(rgb_pred.contiguous(), rgb_gt.contiguous(), rgb_std.reshape(H, W).contiguous(), None, image_hw=(H, W),
                            clip_max=clip_max, nll_min_sigma=min_rgb_std_for_nll, flags=flags, workspace=workspace)
    return finish_metrics(row.cpu().numpy(), Cc, "rgb", flags)
