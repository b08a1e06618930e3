"""Eval harness: the counterpart of scripts/eval_uncertainty.py for this build.

`get_average_uncertainty_metrics` walks (camera, ground-truth image) pairs, renders each camera with
the method's callable (`model.get_outputs_for_camera`, `get_outputs_for_camera_unc`, an ensemble
closure ...), computes the reference's per-image RGB metrics under the reference's key names
(eval_uncertainty.py:756-771: psnr, rgb_ause_{mse,mae,rmse}, rgb_mse, rgb_rmse, rgb_nll, rgb_avg_var,
rgb_auc_{abs_error,length,neg_error}) plus `num_rays_per_sec` / `fps` (:948-952), averages them over
the images (:1069-1077) and writes the same `metrics.json` envelope (:1156-1169).

`lpips` (eval_uncertainty.py:681-689) is computed from the AlexNet weights the checkpoint itself carries under
`lpips.net.*` (checkpoints.lpips_weights_from_state_dict -> model.lpips_weights; `lpips_weights=` overrides): the
host definition metrics.lpips, or the HIP kernels behind ops.lpips_batch when fused.  A model without those weights
leaves the key out, nothing is downloaded.  The formula is restated from torchmetrics' published source and no
pretrained weights were available to this build, so agreement with torchmetrics on real weights is unverified
(tests/test_lpips_cpu.py holds the comparison, skipped where torchmetrics or its cached weights are absent).

Differences, on purpose: of the plots, the four rendered images per eval image (`save_imgs_rgb`, :209-303) and the test-set
sparsification-error plots (:85-98) are written with `save_rendered_images`, the AUCE curve plot and the depth images
(`save_imgs_depth` returns without writing, :182) are not; and `num_rays_per_sec` is reported twice --
`num_rays_per_sec` covers render + metrics like the reference's counter (so numbers stay comparable with its metrics.json), while
`render_rays_per_sec` times the render alone (HIP-synchronised).  Depth metrics (`depth_metrics_unc`,
eval_uncertainty.py:415-644) take the dataset's `depth_gt_XX.npy` map and `scale_parameters.txt` factor,
read by `load_depth_gt`; pass `depth_gt_fn` to `get_average_uncertainty_metrics` to include them.
"""
from __future__ import annotations

import json
import os
import struct
import time
import zlib
from dataclasses import dataclass
from functools import partial
from pathlib import Path
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import metrics as M


def image_metrics_unc(outputs: Dict[str, torch.Tensor], gt_image: torch.Tensor, eval_rgb_unc: bool = True,
                      min_rgb_std_for_nll: float = 3e-2, composite_gt: Optional[Callable] = None, fused: bool = False,
                      lpips_weights=None):
    """get_image_metrics_and_images_unc (eval_uncertainty.py:647-813), RGB part.
    -> (metrics_dict, curves) where curves carries the per-image sparsification / calibration curves
    that the reference accumulates for its test-set plots.
    fused=True: the same keys and curves from one ops.image_metrics call (HIP kernels, one row of float64 sums, one copy to
    the host) instead of the chain of torch ops below; needs the render on a HIP device.
    lpips_weights (a checkpoints.LpipsWeights): adds `lpips` behind `ssim` -- metrics.lpips on the render's device, or
    ops.lpips_batch when fused (its row rides in the same host copy as the metric row).  None: the key is left out."""
    if fused:
        return _image_metrics_unc_fused(outputs, gt_image, eval_rgb_unc, min_rgb_std_for_nll, composite_gt, lpips_weights)
    rgb = outputs["rgb"]                        # as rendered: what every uncertainty metric takes (eval_uncertainty.py:316)
    image = gt_image.to(rgb.device)
    if "background" in outputs and composite_gt is not None:  # splatfacto: blend GT alpha with the background
        image = composite_gt(image, outputs["background"])
    # psnr / ssim / lpips as at eval_uncertainty.py:681-689, on a copy of the prediction clipped to <= 1 that nothing else
    # sees; lpips with the weights the checkpoint brought, else left out of the dict rather than faked
    clipped = torch.clip(rgb, max=1.0)
    md: Dict[str, float] = {"psnr": M.psnr(clipped, image), "ssim": M.ssim(clipped, image[..., :3])}
    if lpips_weights is not None:
        md["lpips"] = M.lpips(clipped, image[..., :3], lpips_weights)
    curves: Dict[str, np.ndarray] = {}
    if eval_rgb_unc:
        rgb_std = outputs["rgb_std"]
        sq = torch.sum((rgb - image) ** 2, dim=-1).flatten()
        ab = torch.sum(torch.abs(rgb - image), dim=-1).flatten()
        var = (rgb_std ** 2).flatten()
        for et, err in (("mse", sq), ("mae", ab), ("rmse", sq)):
            _, e, ev, a = M.ause(var, err, et)
            md[f"rgb_ause_{et}"] = float(a)
            curves[f"rgb_all_ause_{et}"], curves[f"rgb_all_var_ause_{et}"] = e, ev
        md["rgb_mse"] = float(sq.mean().item())
        md["rgb_rmse"] = float(np.sqrt(sq.mean().item()))
        md["rgb_nll"] = float(M.negative_gaussian_loglikelihood(rgb.reshape(-1, 3), image.reshape(-1, 3), rgb_std,
                                                               eps=min_rgb_std_for_nll).mean().item())
        md["rgb_avg_var"] = float(var.mean().item())
        std3 = var.sqrt().unsqueeze(-1).repeat(1, 3)
        a = M.auce_torch(rgb.reshape(-1, 3), std3, image.reshape(-1, 3))   # = M.auce (reference loop), one sort on device
        md["rgb_auc_abs_error"], md["rgb_auc_length"] = a["auc_abs_error_values"], a["auc_length_values"]
        md["rgb_auc_neg_error"] = a["auc_neg_error_values"]
        for k in ("coverage_values", "avg_length_values", "coverage_error_values", "abs_coverage_error_values",
                  "neg_coverage_error_values"):
            curves[f"rgb_all_auce_{k}"] = a[k]
    return md, curves


def _image_metrics_unc_fused(outputs, gt_image, eval_rgb_unc, min_rgb_std_for_nll, composite_gt, lpips_weights=None):
    """image_metrics_unc through the kernels.  The ground-truth composition stays in torch in front of the call
    (elementwise, no sync); the kernels take the prediction as rendered and clip the copy that psnr and SSIM see to <= 1
    themselves (ops.lpips_batch clips its own)."""
    from . import lib as _l, ops
    rgb, image, std, flags = _rgb_operands(outputs, gt_image, eval_rgb_unc, composite_gt)
    H, W, Cc = rgb.shape
    row = ops.image_metrics(rgb, image, std, None, image_hw=(H, W), clip_max=1.0, nll_min_sigma=min_rgb_std_for_nll, flags=flags)
    if lpips_weights is not None:       # both rows in ONE copy to the host
        row = torch.cat((row, ops.lpips_batch(rgb[None], image[None], lpips_weights)[0]))
    host = row.cpu().numpy()
    md, curves = M.finish_metrics(host[:_l.METRICS_ROW], Cc, "rgb", flags)
    if not eval_rgb_unc:
        md = {"psnr": md["psnr"], "ssim": md["ssim"]}
    if lpips_weights is not None:
        md = _with_lpips(md, M.finish_lpips(host[_l.METRICS_ROW:]))
    return md, curves


def _with_lpips(md: Dict[str, float], value: float) -> Dict[str, float]:
    """md with `lpips` behind `ssim` (the key order of the torch path)"""
    out: Dict[str, float] = {}
    for k, v in md.items():
        out[k] = v
        if k == "ssim":
            out["lpips"] = value
    return out


def _with_depth(md: Dict[str, float], dmd: Dict[str, float]) -> Dict[str, float]:
    """one image's dictionary in the reference's key order (eval_uncertainty.py:688-776): psnr / ssim / lpips, the depth
    keys, the rgb uncertainty keys"""
    out = {k: md[k] for k in ("psnr", "ssim", "lpips") if k in md}
    out.update(dmd)
    out.update(md)
    return out


def _rgb_operands(outputs, gt_image, eval_rgb_unc, composite_gt):
    """one image's operands of the fused rgb metrics: (rgb [H,W,C], composed GT [H,W,C], std [H,W], flags), float32"""
    from . import lib as _l
    rgb = outputs["rgb"].to(torch.float32).contiguous()
    image = gt_image.to(rgb.device)
    if "background" in outputs and composite_gt is not None:
        image = composite_gt(image, outputs["background"])
    image = image[..., :rgb.shape[-1]].to(torch.float32).contiguous()
    H, W, _ = rgb.shape
    if eval_rgb_unc:
        return rgb, image, outputs["rgb_std"].to(torch.float32).reshape(H, W).contiguous(), _l.METRICS_ALL
    return rgb, image, torch.zeros(H, W, device=rgb.device), _l.METRICS_SSIM


def _finish_rows(rows_host, image_ids, finish):
    """finish(row) per row of a batch; a row that cannot be finished (non-finite input, nothing valid) raises as
    finish_metrics does, with the image named in front"""
    done = []
    for b, row in enumerate(rows_host):
        try:
            done.append(finish(row))
        except ValueError as e:
            raise ValueError(f"image {b if image_ids is None else image_ids[b]}: {e}") from None
    return done


def image_metrics_unc_batch(outputs_list: Sequence[Dict[str, torch.Tensor]], gt_images: Sequence[torch.Tensor], eval_rgb_unc: bool = True,
                            min_rgb_std_for_nll: float = 3e-2, composite_gt: Optional[Callable] = None, *,
                            image_ids: Optional[Sequence[int]] = None, lpips_weights=None):
    """image_metrics_unc(fused=True) for B renders of one size (at most lib.METRICS_MAX_IMAGES) -> [(metrics_dict, curves)] * B.
    The ground-truth composition and the float32 casts stay per image; then one torch.stack per operand, ONE
    ops.image_metrics_batch, one copy of its [B, row] result to the host and finish_metrics per row.  Row b of the batch is
    the row of image b alone bit for bit, so every entry equals the per-image call's.  An image with a non-finite input
    raises as finish_metrics does, named by image_ids[b] (default: its position in the batch).
    lpips_weights: ONE ops.lpips_batch for the batch adds `lpips` to every entry; its [B, row] result is joined to the
    metric rows on the device, so the batch still crosses to the host in one copy."""
    from . import lib as _l, ops
    if len(outputs_list) != len(gt_images) or not outputs_list:
        raise ValueError(f"{len(outputs_list)} renders for {len(gt_images)} ground-truth images")
    parts = [_rgb_operands(o, gt, eval_rgb_unc, composite_gt) for o, gt in zip(outputs_list, gt_images)]
    flags = parts[0][3]
    if any(p[0].shape != parts[0][0].shape for p in parts):
        raise ValueError(f"a batch holds renders of one size, got {sorted({tuple(p[0].shape) for p in parts})}")
    rgb, image, std = (torch.stack([p[j] for p in parts]) for j in range(3))
    _, H, W, Cc = rgb.shape
    rows = ops.image_metrics_batch(rgb, image, std, None, image_hw=(H, W), clip_max=1.0, nll_min_sigma=min_rgb_std_for_nll,
                                   flags=flags)
    if lpips_weights is not None:
        rows = torch.cat((rows, ops.lpips_batch(rgb, image, lpips_weights)), dim=1)
    rows = rows.cpu().numpy()
    done = _finish_rows(rows[:, :_l.METRICS_ROW], image_ids, lambda row: M.finish_metrics(row, Cc, "rgb", flags))
    if not eval_rgb_unc:
        done = [({"psnr": md["psnr"], "ssim": md["ssim"]}, curves) for md, curves in done]
    if lpips_weights is not None:
        values = _finish_rows(rows[:, _l.METRICS_ROW:], image_ids, M.finish_lpips)
        done = [(_with_lpips(md, v), curves) for (md, curves), v in zip(done, values)]
    return done


# ---- rendered images (save_imgs_rgb, scripts/eval_uncertainty.py:209-303) ------------------------------------------------

def _q8(x: np.ndarray) -> np.ndarray:
    """float -> uint8 as media.write_image does it: (uint8)(clip(x, 0, 1) * 255 + 0.5) in float64, truncating; NaN -> 0"""
    with np.errstate(invalid="ignore"):
        v = np.clip(np.asarray(x).astype(np.float64), 0.0, 1.0) * 255.0 + 0.5
    return np.where(np.isnan(v), 0.0, v).astype(np.uint8)


def _unc_range(unc_min: float, unc_max: float) -> Tuple[np.float32, np.float32]:
    if float(unc_max) == float(unc_min):
        raise ValueError(f"unc_max == unc_min == {unc_min}: the uncertainty range must not be empty (the reference divides by zero)")
    return np.float32(min(unc_min, unc_max)), np.float32(abs(unc_max - unc_min))


def pack_eval_images(rgb, gt, rgb_std, unc_min: float = 0.0, unc_max: float = 1.0) -> Dict[str, np.ndarray]:
    """The four arrays save_imgs_rgb (eval_uncertainty.py:209-303) hands to media.write_image, as the bytes that reach the
    files, in plain numpy: the CPU path, and the definition ops.eval_images (unerf_eval_images_batch) is held to byte for
    byte.  rgb / gt [H, W, 3] (gt already composed as the metrics see it), rgb_std [H, W] or [H, W, 1], float32 ->
      "gt"   [H, W, 3]  q(gt)
      "pred" [H, W, 3]  q(rgb), not clipped first (:316, :395)
      "err"  [H, W]     q(clip(|d0| + |d1| + |d2|, 0, 1)), d = rgb - gt in float32, channels added left to right (:328, :379)
      "std"  [H, W, 3]  colormaps.JET_U8[min((int)(a * 256), 255)] with s = clip((std - min(unc_min, unc_max)) /
                        |unc_max - unc_min|, 0, 1) in float32 (:265; a NaN stays one) and, in float64 and per image,
                        a = (s - vmin) / (vmax - vmin + DBL_EPSILON), vmin / vmax over the non-NaN pixels of s (:280-281:
                        media.to_rgb without vmin / vmax; a constant image gives a = 0); a NaN pixel is (0, 0, 0)
    with q(x) = (uint8)(clip(x, 0, 1) * 255 + 0.5) in float64, truncating, NaN -> 0.
    [UPSTREAM-RECALL] mediapy is not installed here: q (its float -> uint8 conversion) and the to_rgb normalisation are
    restated from its published source and are not pinned by a test against it; the colour table is matplotlib's `jet`,
    which is pinned (tests/test_eval_images_cpu.py).  unc_max == unc_min raises ValueError."""
    from .colormaps import JET_U8
    lo, span = _unc_range(unc_min, unc_max)
    rgb, gt = np.asarray(rgb, dtype=np.float32), np.asarray(gt, dtype=np.float32)
    std = np.asarray(rgb_std, dtype=np.float32).reshape(rgb.shape[:-1])
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(rgb - gt)
        err = np.clip((d[..., 0] + d[..., 1]) + d[..., 2], 0.0, 1.0)
        s = np.clip((std - lo) / span, np.float32(0), np.float32(1))
    ok = ~np.isnan(s)
    std8 = np.zeros(s.shape + (3,), dtype=np.uint8)
    if ok.any():
        vmin, vmax = np.float64(s[ok].min()), np.float64(s[ok].max())
        a = (np.where(ok, s, vmin).astype(np.float64) - vmin) / ((vmax - vmin) + np.finfo(np.float64).eps)
        std8 = JET_U8[np.minimum((a * 256.0).astype(np.int64), 255)]
        std8[~ok] = 0
    return {"gt": _q8(gt), "pred": _q8(rgb), "err": _q8(err), "std": std8}


def _write_png(path, array_u8: np.ndarray, compress_level: int = 6) -> None:
    """array_u8 [H, W] (8-bit grey) or [H, W, 3] (8-bit RGB) -> a PNG file: IHDR, one IDAT (zlib over the rows, each
    behind filter type 0), IEND.  zlib and struct only."""
    a = np.ascontiguousarray(array_u8)
    if a.dtype != np.uint8 or a.size == 0 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)):
        raise ValueError(f"_write_png: expected a non-empty uint8 [H, W] or [H, W, 3] array, got {a.dtype} {a.shape}")
    H, W = a.shape[:2]
    rows = np.empty((H, 1 + a.size // H), dtype=np.uint8)
    rows[:, 0] = 0
    rows[:, 1:] = a.reshape(H, -1)

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 0 if a.ndim == 2 else 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(rows.tobytes(), compress_level)) + chunk(b"IEND", b""))


RENDERED_IMAGE_FILES = (("gt", "rgb_gt"), ("pred", "rgb_pred"), ("err", "rgb_abs_err"), ("std", "rgb_std"))   # plane, file stem


def save_imgs_rgb(img_nums: Sequence[int], outputs_list: Sequence[Dict[str, torch.Tensor]], gt_images: Sequence[torch.Tensor],
                  plots_path, unc_min: float = 0.0, unc_max: float = 1.0, composite_gt: Optional[Callable] = None,
                  fused: bool = False, encode: bool = True) -> Dict[int, Dict[str, np.ndarray]]:
    """save_imgs_rgb (eval_uncertainty.py:209-303) for a list of eval images: `{i}_rgb_gt.png`, `{i}_rgb_pred.png`,
    `{i}_rgb_abs_err.png`, `{i}_rgb_std.png` under plots_path (created), i = img_nums[b]; the ground truth is composed as
    for the metrics.  -> {i: the four uint8 arrays of pack_eval_images}.
    fused=False: four float32 images per eval image go to the host and through pack_eval_images.
    fused=True: the images (of ONE size) are stacked, ops.eval_images packs them on the device in chunks of at most
    lib.METRICS_MAX_IMAGES, and one copy per chunk brings the final bytes (10 per pixel) to the host; same files, byte for byte.
    encode=False returns the arrays without writing files (benchmarks/eval_images.py times the two halves apart)."""
    _unc_range(unc_min, unc_max)
    if not (len(img_nums) == len(outputs_list) == len(gt_images)):
        raise ValueError(f"{len(img_nums)} image numbers for {len(outputs_list)} renders and {len(gt_images)} ground-truth images")
    plots_path = Path(plots_path)
    if encode:
        plots_path.mkdir(parents=True, exist_ok=True)
    parts = [_rgb_operands(o, gt, True, composite_gt)[:3] for o, gt in zip(outputs_list, gt_images)]
    packed: Dict[int, Dict[str, np.ndarray]] = {}
    if not fused:
        for i, (rgb, image, std) in zip(img_nums, parts):
            packed[int(i)] = pack_eval_images(rgb.cpu().numpy(), image.cpu().numpy(), std.cpu().numpy(), unc_min, unc_max)
    elif parts:
        from . import lib as _l, ops
        if any(p[0].shape != parts[0][0].shape for p in parts):
            raise ValueError(f"a batch holds renders of one size, got {sorted({tuple(p[0].shape) for p in parts})}")
        H, W, _ = parts[0][0].shape
        for c0 in range(0, len(parts), _l.METRICS_MAX_IMAGES):
            chunk = parts[c0:c0 + _l.METRICS_MAX_IMAGES]
            rgb, image, std = (torch.stack([p[j] for p in chunk]) for j in range(3))
            host = ops.eval_images(rgb, image, std, unc_min, unc_max)["buffer"].cpu()
            planes = {name: plane.numpy() for name, plane in ops.eval_image_planes(host, len(chunk), (H, W)).items()}
            for b, i in enumerate(img_nums[c0:c0 + len(chunk)]):
                packed[int(i)] = {name: plane[b] for name, plane in planes.items()}
    if encode:
        for i, planes in packed.items():
            for name, stem in RENDERED_IMAGE_FILES:
                _write_png(plots_path / f"{i}_{stem}.png", planes[name])
    return packed


def save_sparsification_plots(plots_path, curves: Dict[str, np.ndarray], output: str = "rgb") -> List[Path]:
    """plot_errors (eval_uncertainty.py:85-98) as the pipeline calls it for the whole test set (:967-994, :1023-1050):
    `plot_{output}_{mse,rmse,mae}_all.png`, the averaged curve err_by_var - err over the fractions removed.  matplotlib is
    imported here (Agg canvas, no global backend change); without it the plots are skipped with one printed line."""
    try:
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure
    except ImportError:
        print(f"matplotlib is not installed: the {output} sparsification plots are skipped")
        return []
    plots_path = Path(plots_path)
    plots_path.mkdir(parents=True, exist_ok=True)
    ratio = np.linspace(0, 1, 100, endpoint=False)
    written = []
    for et in ("mse", "rmse", "mae"):
        fig = Figure()
        FigureCanvasAgg(fig)
        fig.add_subplot().plot(ratio, np.asarray(curves[f"{output}_all_var_ause_{et}"]) - np.asarray(curves[f"{output}_all_ause_{et}"]), "-g")
        written.append(plots_path / f"plot_{output}_{et}_all.png")
        fig.savefig(written[-1])
    return written


def load_depth_gt(dataset_path: str, img_num: int) -> Tuple[np.ndarray, float]:
    """the two files get_unc_metrics_depth reads (eval_uncertainty.py:432-437): -> (depth_gt [H,W], scale a)"""
    a = float(np.loadtxt(os.path.join(str(dataset_path), "scale_parameters.txt"), delimiter=","))
    return np.load(os.path.join(str(dataset_path), "depth_gt_{:02d}.npy".format(img_num))), a


def depth_metrics_unc(outputs: Dict[str, torch.Tensor], depth_gt, scale: float, min_depth_std_for_nll: float = 1.0,
                      fused: bool = False):
    """get_unc_metrics_depth (eval_uncertainty.py:415-644) without the plots, plus the key renaming of
    get_image_metrics_and_images_unc (:702-733).  depth / depth_std are resized to the GT map if the shapes
    differ (torchvision `resize` on a tensor = bilinear `interpolate`, no antialias), scaled by `scale`;
    NLL uses the prediction clipped to [1e-3, max GT] on the full image and is then masked by `GT > 0`;
    errors, AUSE and AUCE use the masked, clipped prediction.  -> (metrics_dict, curves)
    fused=True: resize / scale / clip stay in torch (elementwise, `gt.max()` stays a tensor: no sync); everything behind
    them is one ops.image_metrics call with mask = GT > 0 (the NLL-then-mask above is the masked NLL, element by
    element).  The ground truth is taken as float32 there."""
    clipped, gt, depth_std = _depth_operands(outputs, depth_gt, scale)
    if fused:
        from . import lib as _l, ops
        flags = _l.METRICS_ALL & ~_l.METRICS_SSIM
        row = ops.image_metrics(clipped.unsqueeze(-1).contiguous(), gt.to(torch.float32).unsqueeze(-1).contiguous(),
                                depth_std.contiguous(), (gt > 0).contiguous(), nll_min_sigma=min_depth_std_for_nll, flags=flags)
        return M.finish_metrics(row.cpu().numpy(), 1, "depth", flags, with_psnr=False)
    nll_img = M.negative_gaussian_loglikelihood(clipped.unsqueeze(-1), gt.unsqueeze(-1), depth_std.unsqueeze(-1),
                                                eps=min_depth_std_for_nll).reshape(clipped.shape)
    mask = gt > 0
    d, g, sd = clipped[mask], gt[mask], depth_std[mask]
    sq, ab, var = (g - d) ** 2, (g - d).abs(), sd ** 2
    md: Dict[str, float] = {}
    curves: Dict[str, np.ndarray] = {}
    for et, err in (("mse", sq), ("mae", ab), ("rmse", sq)):
        _, e, ev, a = M.ause(var, err, et)
        md[f"depth_ause_{et}"] = float(a)
        curves[f"depth_all_ause_{et}"], curves[f"depth_all_var_ause_{et}"] = e, ev
    md["depth_mse"] = float(sq.mean().item())
    md["depth_rmse"] = float(np.sqrt(sq.mean().item()))
    md["depth_nll"] = float(nll_img[mask].mean().item())
    md["depth_avg_var"] = float(var.mean().item())
    a = M.auce_torch(d.flatten(), sd.flatten(), g.flatten())
    md["depth_auc_abs_error"], md["depth_auc_length"] = a["auc_abs_error_values"], a["auc_length_values"]
    md["depth_auc_neg_error"] = a["auc_neg_error_values"]
    for k in ("coverage_values", "avg_length_values", "coverage_error_values", "abs_coverage_error_values",
              "neg_coverage_error_values"):
        curves[f"depth_all_auce_{k}"] = a[k]
    return md, curves


def _depth_operands(outputs, depth_gt, scale):
    """one image's depth operands in torch: resize to the GT map, scale, clip to [1e-3, max GT] (a tensor: no sync)
    -> (clipped depth [H,W], gt [H,W] on the render's device, scaled depth_std [H,W])"""
    depth = outputs["depth"].squeeze(-1).to(torch.float32)
    depth_std = outputs["depth_std"].squeeze(-1).to(torch.float32)
    gt = torch.as_tensor(depth_gt, device=depth.device)

    def _fit(x):
        if gt.shape[-2:] == x.shape[-2:]:
            return x
        return torch.nn.functional.interpolate(x[None, None], size=tuple(gt.shape[-2:]), mode="bilinear",
                                               align_corners=False, antialias=False)[0, 0]

    depth, depth_std = _fit(depth), _fit(depth_std)
    lo, hi = 1e-3, gt.max().float()
    depth = scale * depth
    depth_std = scale * depth_std
    return torch.minimum(torch.clamp_min(depth, lo), hi), gt, depth_std


def depth_metrics_unc_batch(outputs_list: Sequence[Dict[str, torch.Tensor]], depth_gts: Sequence, scales: Sequence[float],
                            min_depth_std_for_nll: float = 1.0, *, image_ids: Optional[Sequence[int]] = None):
    """depth_metrics_unc(fused=True) for B renders whose depth GT maps share ONE shape (at most lib.METRICS_MAX_IMAGES)
    -> [(metrics_dict, curves)] * B.  Resize, scale and clip stay in torch per image (each image's `gt.max()` stays a
    tensor); the masks `gt > 0` go in as the [B, n] mask of one ops.image_metrics_batch without SSIM; one copy to the host,
    finish_metrics per row.  Entries equal the per-image call's; errors name the image as in image_metrics_unc_batch."""
    from . import lib as _l, ops
    if not (len(outputs_list) == len(depth_gts) == len(scales)) or not outputs_list:
        raise ValueError(f"{len(outputs_list)} renders for {len(depth_gts)} depth maps and {len(scales)} scales")
    parts = [_depth_operands(o, gt, a) for o, gt, a in zip(outputs_list, depth_gts, scales)]
    if any(p[1].shape != parts[0][1].shape for p in parts):
        raise ValueError(f"a batch holds depth maps of one shape, got {sorted({tuple(p[1].shape) for p in parts})}")
    flags = _l.METRICS_ALL & ~_l.METRICS_SSIM
    pred = torch.stack([p[0].unsqueeze(-1) for p in parts])
    target = torch.stack([p[1].to(torch.float32).unsqueeze(-1) for p in parts])
    std = torch.stack([p[2] for p in parts])
    mask = torch.stack([p[1] > 0 for p in parts])
    rows = ops.image_metrics_batch(pred, target, std, mask, nll_min_sigma=min_depth_std_for_nll, flags=flags).cpu().numpy()
    return _finish_rows(rows, image_ids, lambda row: M.finish_metrics(row, 1, "depth", flags, with_psnr=False))


def _camera_size(camera) -> Tuple[int, int]:
    one = lambda v: int(v.reshape(-1)[0].item()) if torch.is_tensor(v) else int(v)
    return one(camera.height), one(camera.width)


def stack_cameras(cameras: List[object]):
    """single eval cameras of one image size -> the batch object the models' get_outputs_for_cameras take
    (camera_to_worlds [B,3,4]; fx, fy, cx, cy one per camera; camera_type / distortion_params where any camera has them)"""
    from types import SimpleNamespace
    one = lambda v: float(v.reshape(-1)[0].item()) if torch.is_tensor(v) else float(v)
    c2ws = []
    for cam in cameras:
        c2w = torch.as_tensor(cam.camera_to_worlds)
        c2ws.append((c2w[0] if c2w.dim() == 3 else c2w)[:3, :4])
    H, W = _camera_size(cameras[0])
    batch = SimpleNamespace(camera_to_worlds=torch.stack(c2ws), height=H, width=W,
                            **{k: torch.tensor([one(getattr(cam, k)) for cam in cameras], dtype=torch.float64)
                               for k in ("fx", "fy", "cx", "cy")})
    if any(getattr(cam, "camera_type", None) is not None for cam in cameras):
        def ctype(cam):
            t = getattr(cam, "camera_type", None)
            if t is None:
                return 1        # CameraType.PERSPECTIVE
            return int(torch.as_tensor(t).reshape(-1)[0]) if torch.is_tensor(t) else int(getattr(t, "value", t))
        batch.camera_type = torch.tensor([ctype(cam) for cam in cameras])
    if any(getattr(cam, "distortion_params", None) is not None for cam in cameras):
        rows = [getattr(cam, "distortion_params", None) for cam in cameras]
        batch.distortion_params = torch.stack([torch.zeros(6) if r is None else
                                               torch.as_tensor(r).detach().cpu().to(torch.float32).reshape(6) for r in rows])
    return batch


def get_average_uncertainty_metrics(get_outputs_for_camera: Callable, eval_set: Iterable[Tuple[object, torch.Tensor]],
                                    eval_rgb_unc: bool = True, min_rgb_std_for_nll: float = 3e-2,
                                    composite_gt: Optional[Callable] = None, depth_gt_fn: Optional[Callable] = None,
                                    min_depth_std_for_nll: float = 1.0, fused: bool = False, view_batch: int = 1,
                                    get_outputs_for_cameras: Optional[Callable] = None, metric_batch: bool = True,
                                    save_rendered_images: bool = False, plots_path=None, unc_min: float = 0.0,
                                    unc_max: float = 1.0, lpips_weights="model"):
    """eval_uncertainty.py:816-1079.  -> (averaged metrics dict, averaged curves dict).
    depth_gt_fn(image_index) -> (depth_gt [H,W], scale) switches the depth metrics on (eval_depth_unc).
    fused: the per-image metric stage through the HIP kernels (image_metrics_unc / depth_metrics_unc, fused=True).
    view_batch > 1: that many CONSECUTIVE eval cameras of one image size are rendered by one call of the model's
    get_outputs_for_cameras (`get_outputs_for_cameras=`, else the method of that name on the object
    get_outputs_for_camera is bound to) -- NeRF and splat models alike; a change of image size starts a new batch.  Same
    metric keys; a batch's render time is shared equally between its images for the three timing keys.  The default (1) is
    the reference's per-camera loop.
    metric_batch (with fused and view_batch > 1): the images of a view batch are also SCORED together, by
    image_metrics_unc_batch / depth_metrics_unc_batch in chunks of at most lib.METRICS_MAX_IMAGES -- the kernel launches
    and the one host copy of a single image per chunk; where the depth GT maps of a chunk differ in shape its depth
    metrics are scored image by image.  Every metric key and every curve is bit-equal to metric_batch=False (today's
    per-image fused scoring, kept for comparison in one process); the three timing keys then share the batch's render
    time AND its metric time equally between its images.  An image with a non-finite input raises as finish_metrics does,
    named by its index in the eval set.
    save_rendered_images (with eval_rgb_unc, as at :754, :799): save_imgs_rgb writes the four PNGs of every eval image under
    plots_path with the range unc_min / unc_max -- one image after its metrics, or the view batch after its batched
    metrics (packed on the device when fused).  The saving counts into the metric time of `num_rays_per_sec` / `fps`, as
    in the reference's counter (:898, :948-952), and not into `render_rays_per_sec`.
    lpips_weights: a checkpoints.LpipsWeights adds `lpips` per image (averaged like psnr and ssim); None leaves it out; the
    default "model" takes `lpips_weights` of the object get_outputs_for_camera is bound to (an EnsemblePipeline: of its
    first member) -- what load_state_dict found in the checkpoint -- or None."""
    if isinstance(lpips_weights, str):
        bound = getattr(get_outputs_for_camera, "func", get_outputs_for_camera)      # a functools.partial: its method
        lpips_weights = default_lpips_weights(getattr(bound, "__self__", None))
    if save_rendered_images and eval_rgb_unc:
        if plots_path is None:
            raise ValueError("save_rendered_images needs plots_path")
        _unc_range(unc_min, unc_max)
    save = partial(save_imgs_rgb, plots_path=plots_path, unc_min=unc_min, unc_max=unc_max, composite_gt=composite_gt,
                   fused=fused) if save_rendered_images and eval_rgb_unc else None
    if view_batch < 1:
        raise ValueError(f"view_batch={view_batch}: at least 1")
    if view_batch > 1 and get_outputs_for_cameras is None:
        get_outputs_for_cameras = getattr(getattr(get_outputs_for_camera, "__self__", None), "get_outputs_for_cameras", None)
        if get_outputs_for_cameras is None:
            raise ValueError("view_batch > 1 needs the model's get_outputs_for_cameras (pass get_outputs_for_cameras=)")
    rows: List[Dict[str, float]] = []
    sums: Dict[str, np.ndarray] = {}

    def sync():
        if torch.cuda.is_available():
            torch.cuda.synchronize()

    def record(md, curves, hw, render_s, metric_s):
        H, W = hw
        md["num_rays_per_sec"] = H * W / (render_s + metric_s)
        md["fps"] = md["num_rays_per_sec"] / (H * W)
        md["render_rays_per_sec"] = H * W / render_s
        rows.append(md)
        for k, v in curves.items():
            sums[k] = sums.get(k, 0) + np.asarray(v, dtype=np.float64)

    def score(img_num, outputs, gt, render_s):
        start = time.time()
        md, curves = image_metrics_unc(outputs, gt, eval_rgb_unc, min_rgb_std_for_nll, composite_gt, fused=fused,
                                       lpips_weights=lpips_weights)
        if depth_gt_fn is not None:
            dgt, scale = depth_gt_fn(img_num)
            dmd, dcurves = depth_metrics_unc(outputs, dgt, scale, min_depth_std_for_nll, fused=fused)
            md = _with_depth(md, dmd)
            curves.update(dcurves)
        if save is not None:
            save([img_num], [outputs], [gt])
        record(md, curves, outputs["rgb"].shape[:2], render_s, time.time() - start)

    def score_batch(pending, outs, render_share):
        from . import lib as _l
        start = time.time()
        scored = []
        for c0 in range(0, len(pending), _l.METRICS_MAX_IMAGES):
            ids = [img_num for img_num, _, _ in pending[c0:c0 + _l.METRICS_MAX_IMAGES]]
            chunk = outs[c0:c0 + len(ids)]
            done = image_metrics_unc_batch(chunk, [gt for _, _, gt in pending[c0:c0 + len(ids)]], eval_rgb_unc, min_rgb_std_for_nll,
                                           composite_gt, image_ids=ids, lpips_weights=lpips_weights)
            if depth_gt_fn is not None:
                dgts, scales = zip(*(depth_gt_fn(i) for i in ids))
                if len({tuple(np.shape(d)) for d in dgts}) == 1:
                    ddone = depth_metrics_unc_batch(chunk, dgts, scales, min_depth_std_for_nll, image_ids=ids)
                else:       # maps of several shapes do not stack: this chunk's depth metrics image by image
                    ddone = [depth_metrics_unc(o, d, a, min_depth_std_for_nll, fused=True) for o, d, a in zip(chunk, dgts, scales)]
                for (_, curves), (_, dcurves) in zip(done, ddone):
                    curves.update(dcurves)
                done = [(_with_depth(md, dmd), curves) for (md, curves), (dmd, _) in zip(done, ddone)]
            scored += done
        if save is not None:
            save([img_num for img_num, _, _ in pending], outs, [gt for _, _, gt in pending])
        metric_share = (time.time() - start) / len(pending)
        for (md, curves), outputs in zip(scored, outs):
            record(md, curves, outputs["rgb"].shape[:2], render_share, metric_share)

    def flush(pending):     # [(image index, camera, gt)] of one image size
        if not pending:
            return
        start = time.time()
        outs = get_outputs_for_cameras(stack_cameras([cam for _, cam, _ in pending]))
        sync()
        share = (time.time() - start) / len(pending)
        if fused and metric_batch:
            score_batch(pending, list(outs), share)
            return
        for (img_num, _, gt), outputs in zip(pending, outs):
            score(img_num, outputs, gt, share)

    pending: List[Tuple[int, object, torch.Tensor]] = []
    for img_num, (camera, gt) in enumerate(eval_set):
        if view_batch == 1:
            start = time.time()
            outputs = get_outputs_for_camera(camera)
            sync()
            score(img_num, outputs, gt, time.time() - start)
            continue
        if pending and (len(pending) == view_batch or _camera_size(pending[0][1]) != _camera_size(camera)):
            flush(pending)
            pending = []
        pending.append((img_num, camera, gt))
    flush(pending)
    avg = {k: float(torch.mean(torch.tensor([r[k] for r in rows], dtype=torch.float64))) for k in rows[0]}
    return avg, {k: v / len(rows) for k, v in sums.items()}


def default_lpips_weights(model):
    """`lpips_weights` of a model; of the first member for a list of members or an EnsemblePipeline; None without"""
    if model is None:
        return None
    if isinstance(model, (list, tuple)):
        return default_lpips_weights(model[0]) if model else None
    if getattr(model, "lpips_weights", None) is not None:
        return model.lpips_weights
    members = getattr(model, "models", None)
    if members is not None and len(members):
        return getattr(members[0], "lpips_weights", None)
    return None


def write_metrics_json(path: str, experiment_name: str, method_name: str, checkpoint: str, results: Dict[str, float]):
    """the envelope of eval_uncertainty.py:1156-1169"""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", encoding="utf8") as f:
        json.dump({"experiment_name": experiment_name, "method_name": method_name, "checkpoint": checkpoint,
                   "results": results}, f, indent=2)


# ---- the eval script's configuration surface (scripts/eval_configs.py) and its per-method dispatch ----------

@dataclass
class EvalUncertainty:
    """scripts/eval_configs.py:7-49 (field names and defaults; pinned by tests/golden/eval_configs.json)"""
    load_config: Union[Path, List[Path], None] = None
    dataset_path: Optional[Path] = None
    output_path: Path = Path("output.json")
    render_output_path: Optional[Path] = None
    save_all_ause: bool = False
    seed: int = 42
    eval_depth: bool = True
    eval_rgb: bool = True
    plot_ause: bool = False
    save_rendered_images: bool = False
    min_rgb_std_for_nll: float = 3e-2
    min_depth_std_for_nll: float = 2.0
    unc_max: float = 1.0
    unc_min: float = 0.0


@dataclass
class LaplaceConfig(EvalUncertainty):
    prior_precision: float = 1.0
    n_samples: int = 100
    n_iters: int = 300
    use_deterministic_density: bool = False


@dataclass
class EnsembleConfig(EvalUncertainty):
    pass


@dataclass
class MCDropoutConfig(EvalUncertainty):
    mc_samples: Optional[int] = None


@dataclass
class ActiveNerfactoConfig(EvalUncertainty):
    eval_depth: bool = True


@dataclass
class ActiveSplatfactoConfig(EvalUncertainty):
    eval_depth: bool = False


EvalConfigs = Union[LaplaceConfig, EnsembleConfig, MCDropoutConfig, ActiveNerfactoConfig, ActiveSplatfactoConfig]


def outputs_fn_for(eval_config: EvalConfigs, model, ggn_batches=None, pipeline=None) -> Callable:
    """The per-method callable scripts/eval_uncertainty.py:1086-1134 selects, for this build's Model mirrors.
    `model` is one Model, or a list of member Models for EnsembleConfig (single process; one member per rank goes
    through ensemble.aggregate_distributed instead).  LaplaceConfig loads `ggn_{n_iters}.pt` next to load_config when
    it exists, else fits the GGN (from `pipeline.datamanager` or `ggn_batches`) and saves it there (:1103-1116)."""
    import torch
    if isinstance(eval_config, EnsembleConfig):
        from . import ensemble
        if hasattr(model, "get_ensemble_outputs_for_camera_ray_bundle"):   # an EnsemblePipeline (eval_uncertainty.py:1127)
            return model.get_ensemble_outputs_for_camera_ray_bundle
        return ensemble.EnsemblePipeline(list(model)).get_ensemble_outputs_for_camera_ray_bundle
    if isinstance(eval_config, MCDropoutConfig):
        model.config.mc_samples = eval_config.mc_samples if eval_config.mc_samples is not None else model.config.mc_samples
        model.invalidate()
        return model.get_outputs_for_camera
    if isinstance(eval_config, LaplaceConfig):
        hessian_path = None
        if eval_config.load_config is not None:
            hessian_path = Path(eval_config.load_config).parent / f"ggn_{eval_config.n_iters}.pt"
        if hessian_path is not None and hessian_path.exists():
            saved = torch.load(hessian_path)
            model.field.mlp_density_ggn, model.field.mlp_rgb_ggn = saved["mlp_density_ggn"], saved["mlp_rgb_ggn"]
        else:
            model.compute_hessian_naive(pipeline=pipeline, n_iters=eval_config.n_iters, ray_batches=ggn_batches)
            if hessian_path is not None:
                hessian_path.parent.mkdir(parents=True, exist_ok=True)
                torch.save({"mlp_density_ggn": model.field.mlp_density_ggn.cpu(),
                            "mlp_rgb_ggn": model.field.mlp_rgb_ggn.cpu()}, hessian_path)
        model.prior_prec = eval_config.prior_precision
        return partial(model.get_outputs_for_camera_unc, is_inference=True,
                       use_deterministic_density=eval_config.use_deterministic_density,
                       prior_prec=eval_config.prior_precision, n_samples=eval_config.n_samples)
    return model.get_outputs_for_camera          # ActiveNerfactoConfig, ActiveSplatfactoConfig


def run_eval(eval_config: EvalConfigs, model, eval_set, experiment_name: str = "", method_name: str = "",
             checkpoint: str = "", depth_gt_fn: Optional[Callable] = None, composite_gt: Optional[Callable] = None,
             fused: bool = False, view_batch: int = 1, metric_batch: bool = True, lpips_weights="model",
             **fn_kw) -> Dict[str, float]:
    """main() of scripts/eval_uncertainty.py:1082-1169 without nerfstudio's pipeline loading: pick the method's
    callable, average the per-image metrics, write the metrics.json envelope to eval_config.output_path.
    fused=True computes the per-image metrics with the HIP kernels behind ops.image_metrics (same keys; opt-in).
    view_batch > 1: that many consecutive eval cameras of one size per call of the method's batch callable
    (get_average_uncertainty_metrics) -- model.get_outputs_for_cameras; for LaplaceConfig
    model.get_outputs_for_cameras_unc with the keyword arguments of the per-camera callable (the last-layer samples are
    drawn in the per-camera order, so the metrics are those of view_batch = 1 under the same generator state); for
    EnsembleConfig EnsemblePipeline.get_ensemble_outputs_for_cameras (every member renders the batch, the moments run
    per view).
    metric_batch (with fused=True and view_batch > 1): a view batch is also scored by one batched metric call
    (get_average_uncertainty_metrics); False keeps the per-image fused scoring.  Same numbers either way.
    eval_config.save_rendered_images: the four rendered images per eval image (save_imgs_rgb, with eval_config.unc_min /
    unc_max) and the test-set sparsification plots (save_sparsification_plots; depth ones when depth is evaluated) go to
    `output_path.parent / "plots"` (:699-700).  Off (the default): no directory, the same keys.
    lpips_weights: a checkpoints.LpipsWeights, None (no `lpips` key), or the default "model": the weights the model's
    checkpoint brought (default_lpips_weights: model.lpips_weights, the first member's for an ensemble)."""
    if isinstance(lpips_weights, str):
        lpips_weights = default_lpips_weights(model)
    fn = outputs_fn_for(eval_config, model, **fn_kw)
    batch_fn = None
    if view_batch > 1 and isinstance(eval_config, LaplaceConfig):
        if hasattr(model, "get_outputs_for_cameras_unc"):
            batch_fn = partial(model.get_outputs_for_cameras_unc, **fn.keywords)
    elif view_batch > 1 and isinstance(eval_config, EnsembleConfig):
        batch_fn = getattr(getattr(fn, "__self__", None), "get_ensemble_outputs_for_cameras", None)
    elif view_batch > 1:
        batch_fn = getattr(model, "get_outputs_for_cameras", None)
    if composite_gt is None and hasattr(model, "composite_gt"):   # splat models: GT alpha over the background
        composite_gt = model.composite_gt
    if eval_config.eval_depth and depth_gt_fn is None and eval_config.dataset_path is not None:
        depth_gt_fn = lambda i: load_depth_gt(str(eval_config.dataset_path), i)
    plots_path = Path(eval_config.output_path).parent / "plots" if eval_config.save_rendered_images else None
    metrics, curves = get_average_uncertainty_metrics(
        fn, eval_set, eval_rgb_unc=eval_config.eval_rgb, min_rgb_std_for_nll=eval_config.min_rgb_std_for_nll,
        composite_gt=composite_gt, depth_gt_fn=depth_gt_fn if eval_config.eval_depth else None,
        min_depth_std_for_nll=eval_config.min_depth_std_for_nll, fused=fused,
        view_batch=view_batch if batch_fn is not None else 1, get_outputs_for_cameras=batch_fn, metric_batch=metric_batch,
        save_rendered_images=eval_config.save_rendered_images, plots_path=plots_path, unc_min=eval_config.unc_min,
        unc_max=eval_config.unc_max, lpips_weights=lpips_weights)
    if plots_path is not None:
        for output in ("depth", "rgb"):
            if f"{output}_all_ause_mse" in curves:
                save_sparsification_plots(plots_path, curves, output)
    write_metrics_json(str(eval_config.output_path), experiment_name, method_name, checkpoint, metrics)
    return metrics
