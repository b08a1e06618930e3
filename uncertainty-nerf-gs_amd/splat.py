"""Frame-level active-splatfacto pipeline on the HIP kernels.

Mirrors ActiveSplatfactoModel.get_outputs (models/activesplatfacto/activesplatfacto_model.py:142-367),
eval branch, with the MI355X restructuring: the reference calls gsplat's rasterize_gaussians four
times (rgb, beta, depth, depth-variance), each repeating the bin-and-sort; here the intersections
are binned and sorted ONCE and rgb + beta + depth are blended in one 5-channel pass, followed by
the data-dependent depth-variance pass (it needs the finished depth image, :336).
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional

import torch

from . import lib as _l
from . import ops
from .ops import _check_want


def viewmat_from_c2w(c2w: torch.Tensor) -> torch.Tensor:
    """activesplatfacto_model.py:184-195: flip y/z to gsplat's convention, analytic inverse."""
    c2w = c2w.detach().to("cpu", torch.float32)
    R = c2w[:3, :3] @ torch.diag(torch.tensor([1.0, -1.0, -1.0]))
    T = c2w[:3, 3:4]
    Rinv = R.T
    V = torch.eye(4)
    V[:3, :3] = Rinv
    V[:3, 3:4] = -Rinv @ T
    return V


# [UPSTREAM nerfstudio 1.1.0 SplatfactoModel.populate_modules] the stored eval background: config "random" ->
# the Viser grey, otherwise the named colour (nerfstudio.utils.colors.get_color)
BACKGROUND_RANDOM = (0.1490, 0.1647, 0.2157)
NAMED_COLORS = {"white": (1.0, 1.0, 1.0), "black": (0.0, 0.0, 0.0), "red": (1.0, 0.0, 0.0), "green": (0.0, 1.0, 0.0),
                "blue": (0.0, 0.0, 1.0)}


def background_for(config_background_color: str) -> torch.Tensor:
    if config_background_color == "random":
        return torch.tensor(BACKGROUND_RANDOM, dtype=torch.float32)
    if config_background_color not in NAMED_COLORS:
        raise ValueError(f"unknown background_color {config_background_color!r}; known: random, {', '.join(NAMED_COLORS)}")
    return torch.tensor(NAMED_COLORS[config_background_color], dtype=torch.float32)


def empty_outputs(W: int, H: int, background: torch.Tensor) -> Dict[str, torch.Tensor]:
    """[UPSTREAM SplatfactoModel.get_empty_outputs] what the reference returns when the crop box holds no splat or
    every projected radius is zero (activesplatfacto_model.py:176-177, 239-240): background image, depth 10, zero
    accumulation -- and none of the uncertainty keys."""
    rgb = background.repeat(H, W, 1)
    return {"rgb": rgb, "depth": background.new_ones(H, W, 1) * 10, "accumulation": background.new_zeros(H, W, 1),
            "background": background}


class _Front(NamedTuple):
    """what the front end of a frame (_frame_front) or of a batch of views (_views_front) leaves for the passes behind it: the
    (cropped) means, the projection's and the shading's per-splat arrays and the sorted tile lists"""
    means: torch.Tensor
    xys: torch.Tensor
    depths: torch.Tensor
    radii: torch.Tensor
    conics: torch.Tensor
    comp: Optional[torch.Tensor]            # the compensation factors of an antialiased frame, else None
    cov3d: Optional[torch.Tensor]
    cols: torch.Tensor
    opac: torch.Tensor
    gids: torch.Tensor
    bins: torch.Tensor
    c2w: Optional[torch.Tensor] = None      # single view: the pose and the view matrix on the host
    V: Optional[torch.Tensor] = None
    views: object = None                    # batch: ops.splat_view_records, the per-view "nothing to render" flags and, for
    empty: Optional[List[bool]] = None      # the pose Jacobian, the contracted tangents
    ptan: Optional[torch.Tensor] = None


def _crop(gp: Dict[str, torch.Tensor], crop_ids: Optional[torch.Tensor]) -> Optional[Dict[str, torch.Tensor]]:
    """gp restricted to crop_ids (bool [N] from `crop_box.within(means)`, :174-180, 202-217); None: no splat is left -- none at
    all, or none in the box: the same picture as "nothing visible" (:176-177, 239-240)"""
    if gp["means"].shape[0] == 0:
        return None
    if crop_ids is not None:
        crop_ids = crop_ids.reshape(-1).to(gp["means"].device)
        if int(crop_ids.sum().item()) == 0:
            return None
        gp = {k: v[crop_ids].contiguous() for k, v in gp.items()}
    return gp


def _shade_args(gp: Dict[str, torch.Tensor], sh_degree: int, config_sh_degree: Optional[int], beta_min: Optional[float]):
    """-> the degree the shade kernel is given (config_sh_degree <= 0: -1, colours = sigmoid(features_dc), :247-248), the
    uncertainty logits and beta_min of an active frame (beta_min None -- the pose functions -- or plain splatfacto: no beta row)"""
    if config_sh_degree is not None and config_sh_degree <= 0:
        sh_degree = -1
    if beta_min is None or "log_uncertainties" not in gp:
        return sh_degree, None, 0.0 if beta_min is None else beta_min
    return sh_degree, gp["log_uncertainties"].reshape(-1).contiguous(), beta_min


def _frame_front(gp: Dict[str, torch.Tensor], c2w: torch.Tensor, fx: float, fy: float, cx: float, cy: float, H: int, W: int,
                 sh_degree: int, rasterize_mode: str, block_width: int, crop_ids: Optional[torch.Tensor],
                 config_sh_degree: Optional[int], tight: bool, beta_min: Optional[float] = None) -> Optional[_Front]:
    """The part every single-view frame function shares: crop, projection, intersection count, shading and the bin sort, in the
    order that hides the frame's one host read-back.  None: the frame is the reference's get_empty_outputs (no splat, none in
    the crop box, or nothing visible)."""
    gp = _crop(gp, crop_ids)
    if gp is None:
        return None
    means = gp["means"].contiguous()
    # the pose goes to the host ONCE, here, before anything is queued: a device-resident camera_to_worlds (the normal
    # nerfstudio model path) would otherwise be read back behind the projection and the scan -- a blocking stream sync
    # exactly where the intersection count's read-back is meant to overlap the SH-colour kernel
    c2w = c2w.detach().to("cpu", torch.float32)
    V = viewmat_from_c2w(c2w)
    if rasterize_mode not in ("classic", "antialiased"):
        raise ValueError(f"Unknown rasterize_mode: {rasterize_mode}")
    aa = rasterize_mode == "antialiased"
    # exp(scales) and quats / quats.norm() (:221-223) are taken inside the projection kernel; with `tight` also
    # sigmoid(opacities) [* comp] (:252-256), which the tight tile counts depend on
    logits = gp["opacities"].reshape(-1).contiguous()
    proj = ops.splat_project(means, gp["scales"].contiguous(), 1.0, gp["quats"].contiguous(), V[:3], fx, fy, cx, cy, H, W,
                             block_width, raw=True, opacity_logits=logits if tight else None, antialiased=aa)
    xys, depths, radii, conics, comp, tiles, cov3d = proj[:7]
    # the intersection count (the frame's one host read-back) starts its way to the host now and is awaited inside
    # splat_bin_sort; the SH colours do not depend on it and keep the GPU busy meanwhile
    count = ops.SplatCount(tiles, defer_copy=True)
    degree, log_unc, beta_min = _shade_args(gp, sh_degree, config_sh_degree, beta_min)
    # the reference concatenates features_dc and features_rest first (:242-243); the kernel reads them in place.  One launch
    # leaves the rasteriser's per-splat rows [rgb, (beta), depth] (and the opacities unless the projection made them)
    cols, opac = ops.splat_shade_inputs(degree, means, c2w[:3, 3], gp["features_dc"].contiguous(),
                                        gp["features_rest"].contiguous(), log_unc, beta_min, None if tight else logits,
                                        comp if aa else None, depths)
    count.start_copy()      # (its host-side set-up runs under the SH kernel just queued)
    if tight:
        opac = proj[7]
    # (self.radii).sum() == 0 -> get_empty_outputs (:239-240).  A splat has a non-zero radius exactly when it hits at
    # least one tile, so "no intersections" is the same test and rides on the one host read-back of the frame
    I, _cum, _keys, gids, bins = ops.splat_bin_sort(xys, depths, radii, tiles, H, W, block_width, want_isect_ids=False,
                                                    count=count, tight=(conics, opac) if tight else None)
    # (tight lists can be empty while splats are "visible" by radius -- every opacity below 1/255: the reference then
    # rasterises a frame in which nothing blends, which the empty lists give as well; the extra read-back is on that path
    # only)
    if I == 0 and not (tight and bool((radii > 0).any())):
        return None
    return _Front(means, xys, depths, radii, conics, comp if aa else None, cov3d, cols, opac, gids, bins, c2w=c2w, V=V)


def _views_front(gp: Dict[str, torch.Tensor], c2ws: torch.Tensor, fxs, fys, cxs, cys, H: int, W: int, sh_degree: int,
                 aa: bool, block_width: int, crop_ids: Optional[torch.Tensor], config_sh_degree: Optional[int], tight: bool,
                 beta_min: Optional[float] = None, projs: Optional[torch.Tensor] = None) -> Optional[_Front]:
    """_frame_front for the B views of c2ws [B,3|4,4] (on the host) in shared launches, the crop applied once and the per-view
    intersection totals read back in one copy.  projs [B,12,P]: the pose Jacobian's contracted tangents as well -- they do not
    wait for the count either, so they are queued under its way to the host, in front of the bin sort.  None: every view is
    get_empty_outputs; else `empty` says which are."""
    gp = _crop(gp, crop_ids)
    if gp is None:
        return None
    B = c2ws.shape[0]
    means = gp["means"].contiguous()
    views = ops.splat_view_records([viewmat_from_c2w(c) for c in c2ws], fxs, fys, cxs, cys, [c[:3, 3] for c in c2ws])
    logits = gp["opacities"].reshape(-1).contiguous()
    proj = ops.splat_project_batch(means, gp["scales"].contiguous(), gp["quats"].contiguous(), views, B, H, W, block_width,
                                   opacity_logits=logits if tight else None, antialiased=aa, want_cov3d=projs is not None)
    xys, depths, radii, conics, comp, tiles, opac = proj[:7]
    cov3d = proj[7] if projs is not None else None
    count = ops.SplatCountBatch(tiles, radii if tight else None, defer_copy=True)
    degree, log_unc, beta_min = _shade_args(gp, sh_degree, config_sh_degree, beta_min)
    cols, opac2 = ops.splat_shade_inputs_batch(degree, means, views, B, gp["features_dc"].contiguous(),
                                               gp["features_rest"].contiguous(), log_unc, beta_min, None if tight else logits,
                                               comp if aa else None, depths)
    count.start_copy()
    opac = opac if tight else opac2
    ptan = None if projs is None else ops.splat_pose_ptangents_batch(means, cov3d, radii, views, B, projs, H, W)
    totals, visible, gids, bins = ops.splat_bin_sort_batch(xys, depths, radii, count, H, W, block_width,
                                                           tight=(conics, opac) if tight else None)
    # per view as the single-view call decides: no intersections and (with tight lists) no radius > 0 -> get_empty_outputs
    empty = [totals[v] == 0 and not (tight and visible[v]) for v in range(B)]
    if all(empty):
        return None
    return _Front(means, xys, depths, radii, conics, comp if aa else None, cov3d, cols, opac, gids, bins, views=views,
                  empty=empty, ptan=ptan)


def active_splatfacto_outputs(gp: Dict[str, torch.Tensor], c2w: torch.Tensor, fx: float, fy: float, cx: float,
                              cy: float, H: int, W: int, background: torch.Tensor, beta_min: float = 0.01,
                              sh_degree: int = 3, rasterize_mode: str = "classic",
                              block_width: int = 16, crop_ids: Optional[torch.Tensor] = None,
                              config_sh_degree: Optional[int] = None, tight: bool = True) -> Dict[str, Optional[torch.Tensor]]:
    """gp: gauss_params on the device (means, scales, quats, features_dc, features_rest, opacities,
    log_uncertainties).  Returns the reference's output dict (:359-367) as [H,W,C] tensors.
    Without `log_uncertainties` in gp: plain splatfacto [UPSTREAM nerfstudio 1.1.0 SplatfactoModel.get_outputs, the
    parent the reference extends and the member type of its splat ensembles] -- rgb + depth blended in one 4-channel
    pass, outputs rgb / depth / accumulation / background only.
    crop_ids: bool [N] from `crop_box.within(means)` (:174-180, 202-217) -- only those splats are rendered.
    sh_degree: the active degree n = min(step // interval, config.sh_degree) (:244);
    config_sh_degree == 0 selects the sigmoid(features_dc) colours of :247-248.
    tight: bin each splat into the tiles its alpha >= 1/255 ellipse reaches instead of gsplat's whole radius box (the
    left-out pairs are ones the blend loop skips itself: same output bits, about half the sort and staging work);
    False: gsplat's lists."""
    _l.require_gpu()
    background = background.to(gp["means"].device, torch.float32)
    f = _frame_front(gp, c2w, fx, fy, cx, cy, H, W, sh_degree, rasterize_mode, block_width, crop_ids, config_sh_degree, tight,
                     beta_min=beta_min)
    if f is None:
        return empty_outputs(W, H, background)
    xys, depths, conics, cols, opac, gids, bins = f.xys, f.depths, f.conics, f.cols, f.opac, f.gids, f.bins
    # frame scratch: the background padded to the row length, and the two channel maxima the rasteriser passes leave for
    # their alpha normalisations
    Cn = cols.shape[1]
    scratch = torch.zeros(Cn + 2, device=f.means.device)
    scratch[:3] = background
    bg, mx1, mx2 = scratch[:Cn], scratch[Cn:Cn + 1], scratch[Cn + 1:Cn + 2]
    if "log_uncertainties" not in gp:
        img, fT, _ = ops.splat_rasterize(gids, bins, xys, conics, cols, opac, H, W, bg, block_width, chan_max=(3, mx1))
        # depth = where(alpha > 0, d / alpha, max(d)), rgb clamp and accumulation in one pass over the pixels
        rgb, alpha, _, _ = ops.splat_normalize_outputs(img, 3, fT, mx1, rgb=True, acc=True)
        return {"rgb": rgb, "depth": img[..., 3:4], "accumulation": alpha, "background": background}
    img, fT, fidx = ops.splat_rasterize(gids, bins, xys, conics, cols, opac, H, W, bg, block_width, want_final_idx=True,
                                        chan_max=(4, mx1))
    # depth = where(alpha>0, d/alpha, max(d)) (:319) + clamp(rgb, max=1) (:275), 1 - final_T, uncertainty^2 in the same pass
    rgb, alpha, rgb_var, _ = ops.splat_normalize_outputs(img, 4, fT, mx1, rgb=True, acc=True, sq_ch=3)
    sq = ops.splat_depth_sqdiff(xys, depths, img, 4)       # (z_i - depth[floor(xy_i)])^2            (:325-341)
    # same ids / bins / geometry / opacities as the first pass: every pixel stops at the index that pass ended on
    dv, fT2, _ = ops.splat_rasterize(gids, bins, xys, conics, sq[:, None], opac, H, W, None, block_width,
                                     stop_idx=fidx, chan_max=(0, mx2))
    _, _, _, dstd = ops.splat_normalize_outputs(dv, 0, fT2, mx2, sqrt=True)   # (:356) + depth_std = sqrt(depth_var)
    unc = img[..., 3:4]
    return {"rgb": rgb, "depth": img[..., 4:5], "accumulation": alpha,
            "background": background, "uncertainty": unc, "rgb_var": rgb_var, "rgb_std": unc,
            "depth_var": dv, "depth_std": dstd}


def pose_gradient_camera(gp: Dict[str, torch.Tensor], c2w: torch.Tensor, fx: float, fy: float, cx: float, cy: float,
                         H: int, W: int, background: torch.Tensor, sh_degree: int = 3, rasterize_mode: str = "classic",
                         block_width: int = 16, crop_ids: Optional[torch.Tensor] = None,
                         config_sh_degree: Optional[int] = None, tight: bool = True, want_rgb: bool = False):
    """d mean_c(rgb[y, x]) / d camera_to_worlds of the frame active_splatfacto_outputs renders -> [H,W,3,4] float32 (with
    want_rgb also the frame's rgb [H,W,3] as the gradient kernel blended it): the per-pixel quantity of the reference's
    scripts/estimate_gradient_pose_6dof.py:128-139, for splats.  The projection, shading, count and
    bin-sort calls are the frame's own, so the tile lists are; then one per-splat tangent kernel and one forward-mode walk.
    Held fixed: near-plane cull, radii, lists, skipped pairs, stops, the crop and the (detached, :243) SH colours.  A frame
    answered with empty_outputs has a zero gradient and the background image.  Works with and without
    `log_uncertainties`; only rgb is differentiated."""
    _l.require_gpu()
    dev = gp["means"].device
    background = background.to(dev, torch.float32)
    f = _frame_front(gp, c2w, fx, fy, cx, cy, H, W, sh_degree, rasterize_mode, block_width, crop_ids, config_sh_degree, tight)
    if f is None:
        g = torch.zeros(H, W, 3, 4, device=dev)
        return (g, background.repeat(H, W, 1)) if want_rgb else g
    tan = ops.splat_pose_tangents(f.means, f.cov3d, f.radii, f.V[:3], fx, fy, cx, cy, H, W)
    grad, rgb, _ = ops.splat_pose_grad(f.gids, f.bins, f.xys, f.conics, f.cols[:, :3].contiguous(), f.opac, tan, H, W, background,
                                       compensation=f.comp, c2w=f.c2w[:3, :4], block_width=block_width, want_rgb=want_rgb)
    return (grad, rgb) if want_rgb else grad


def pose_jacobian_camera(gp: Dict[str, torch.Tensor], c2w: torch.Tensor, fx: float, fy: float, cx: float, cy: float,
                         H: int, W: int, background: torch.Tensor, proj=None, channels=ops.POSE_CHANNELS,
                         want=("proj", "val"), sh_degree: int = 3, rasterize_mode: str = "classic", block_width: int = 16,
                         crop_ids: Optional[torch.Tensor] = None, config_sh_degree: Optional[int] = None,
                         tight: bool = True) -> Dict[str, torch.Tensor]:
    """The per-pixel Jacobian of the frame's channels (ops.POSE_CHANNELS order: r, g, b, accumulation, expected_depth) with
    respect to the camera pose, for the frame active_splatfacto_outputs renders.  proj [12,P] in c2w entries
    (row-major 3x4), as posegrad.pose_projection gives it, 1 <= P <= 12; None: the 12 x 12 identity, i.e. d / d c2w.
    -> the requested of  "proj" [H,W,C,P] = J . proj   "var" [H,W,C] = sum_p proj_p^2   "val" [H,W,C] the channels' values.
    The projection, shading, count and bin-sort calls are the frame's own; then the per-splat tangent kernel, their contraction
    with viewmat_jacobian(c2w) @ proj (fp32) and one forward-mode walk.  Held fixed as in pose_gradient_camera.  The expected
    depth is D / accumulation where something was blended and exactly 0 (value and row) elsewhere: the frame's max(depth) fill
    of those pixels is left to the caller.  A frame answered with empty_outputs gives zeros, and the background as the r, g, b
    values."""
    from . import posegrad
    _l.require_gpu()
    background = background.to(gp["means"].device, torch.float32)
    bits = ops.pose_channel_bits(channels)
    want = _check_want("pose_jacobian_camera", want)
    c2w = c2w.detach().to("cpu", torch.float32)
    c2w = c2w[0] if c2w.dim() == 3 else c2w
    try:
        M = posegrad.splat_view_projection(c2w, proj, _l.SPLAT_POSE_MAX_P)
    except ValueError as e:
        raise _l.UnerfError(f"pose_jacobian_camera: {e}") from None
    P = int(M.shape[1])
    f = _frame_front(gp, c2w, fx, fy, cx, cy, H, W, sh_degree, rasterize_mode, block_width, crop_ids, config_sh_degree, tight)
    if f is None:
        rows = [k for k in range(len(ops.POSE_CHANNELS)) if bits >> k & 1]
        return _pose_jacobian_empty(H, W, rows, P, want, background)
    tan = ops.splat_pose_tangents(f.means, f.cov3d, f.radii, f.V[:3], fx, fy, cx, cy, H, W)
    ptan = ops.splat_pose_tangents_proj(tan, f.means, f.radii, M)
    return ops.splat_pose_jacobian(f.gids, f.bins, f.xys, f.conics, f.cols[:, :3].contiguous(), f.depths, f.opac, ptan, P, H, W,
                                   background, compensation=f.comp, channels=channels, want=want, block_width=block_width)


def pose_normal_eq_camera(gp: Dict[str, torch.Tensor], c2w: torch.Tensor, fx: float, fy: float, cx: float, cy: float,
                          H: int, W: int, background: torch.Tensor, target=None, weights=None, mask=None,
                          channels=("r", "g", "b"), pose_cov_prior=None, **frame_kwargs) -> Dict[str, object]:
    """The pose normal equations of the splat frame in the six se3 parameters (posegrad.POSE_PARAMS, c2w . exp(xi)):
    pose_jacobian_camera(want=("proj", "val")) with proj = posegrad.tangent_basis(c2w), then ONE ops.pose_normal_eq_accumulate
    over the frame and the finish.  target / weights / mask, the result and pose_cov_prior as render.pose_normal_eq_camera;
    frame_kwargs go to pose_jacobian_camera (sh_degree, rasterize_mode, block_width, crop_ids, config_sh_degree, tight)."""
    from . import posegrad
    from .render import _frame_rows
    what = "pose_normal_eq_camera"
    Cn = bin(ops.pose_channel_bits(channels)).count("1")
    dev = gp["means"].device
    tg = _frame_rows(what, "target", target, H, W, {Cn}, dev)
    wt = _frame_rows(what, "weights", weights, H, W, {1, Cn}, dev)
    mk = _frame_rows(what, "mask", mask, H, W, {1}, dev, torch.uint8)
    c2w = c2w.detach().to("cpu", torch.float32)
    c2w = c2w[0] if c2w.dim() == 3 else c2w
    r = pose_jacobian_camera(gp, c2w, fx, fy, cx, cy, H, W, background, proj=posegrad.tangent_basis(c2w), channels=channels,
                             want=("proj", "val") if tg is not None else ("proj",), **frame_kwargs)
    ws = ops.pose_normal_eq_workspace(H * W, 6, dev)
    ops.pose_normal_eq_accumulate(ws, r["proj"].reshape(H * W, Cn, 6), None if tg is None else r["val"].reshape(H * W, Cn), tg, wt, mk)
    out = ops.pose_normal_eq_finish(ws)
    out["covariance"], out["rank"] = posegrad.pose_covariance(out["information"], pose_cov_prior)
    return out


def _pose_jacobian_empty(H: int, W: int, rows: List[int], P: int, want, background: torch.Tensor) -> Dict[str, torch.Tensor]:
    """pose_jacobian_camera's answer for a frame that empty_outputs would render: zeros, the background as r, g, b"""
    dev = background.device
    out = {"proj": torch.zeros(H, W, len(rows), P, device=dev), "var": torch.zeros(H, W, len(rows), device=dev)}
    val = torch.zeros(H, W, len(ops.POSE_CHANNELS), device=dev)
    val[..., :3] = background
    out["val"] = val[..., rows].contiguous()
    return {k: out[k] for k in want}


def _per_view(x, B: int, name: str) -> List[float]:
    """a scalar (or one-element tensor) for every view, or B values"""
    t = torch.as_tensor(x).detach().to("cpu", torch.float64).reshape(-1)
    if t.numel() == 1:
        return [float(t[0])] * B
    if t.numel() != B:
        raise ValueError(f"{name}: {t.numel()} values for {B} cameras (give one, or one per camera)")
    return [float(v) for v in t]


def active_splatfacto_outputs_batch(gp: Dict[str, torch.Tensor], c2ws: torch.Tensor, fx, fy, cx, cy, H: int, W: int,
                                    background: torch.Tensor, beta_min: float = 0.01, sh_degree: int = 3,
                                    rasterize_mode: str = "classic", block_width: int = 16,
                                    crop_ids: Optional[torch.Tensor] = None, config_sh_degree: Optional[int] = None,
                                    tight: bool = True) -> List[Dict[str, Optional[torch.Tensor]]]:
    """active_splatfacto_outputs for B cameras of one splat set and one image size, in the same launches: c2ws [B,3|4,4];
    fx, fy, cx, cy: scalars or B values.  Returns B dicts, element v BIT-identical to active_splatfacto_outputs with camera v
    (empty_outputs for a view that sees nothing, the rasterised all-faint frame, the crop applied once for all views).
    The batch reads its per-view intersection totals back in one copy (SplatCountBatch); B <= lib.SPLAT_MAX_VIEWS.
    Images of more than lib.SPLAT_BATCH_MAX_TILES tiles (e.g. 2560 x 1440 at block_width 16) are beyond the batched tile
    sort: their views are rendered one by one with active_splatfacto_outputs (same results, no shared launches)."""
    _l.require_gpu()
    c2ws = c2ws.detach().to("cpu", torch.float32)
    if c2ws.dim() == 2:
        c2ws = c2ws[None]
    B = c2ws.shape[0]
    if not 1 <= B <= _l.SPLAT_MAX_VIEWS:
        raise ValueError(f"active_splatfacto_outputs_batch: {B} cameras, a batch holds 1 to {_l.SPLAT_MAX_VIEWS}")
    fxs, fys, cxs, cys = (_per_view(v, B, n) for v, n in ((fx, "fx"), (fy, "fy"), (cx, "cx"), (cy, "cy")))
    if ((W + block_width - 1) // block_width) * ((H + block_width - 1) // block_width) > _l.SPLAT_BATCH_MAX_TILES:
        return [active_splatfacto_outputs(gp, c2ws[v], fxs[v], fys[v], cxs[v], cys[v], H, W, background, beta_min=beta_min,
                                          sh_degree=sh_degree, rasterize_mode=rasterize_mode, block_width=block_width,
                                          crop_ids=crop_ids, config_sh_degree=config_sh_degree, tight=tight)
                for v in range(B)]
    background = background.to(gp["means"].device, torch.float32)
    if rasterize_mode not in ("classic", "antialiased"):
        raise ValueError(f"Unknown rasterize_mode: {rasterize_mode}")
    f = _views_front(gp, c2ws, fxs, fys, cxs, cys, H, W, sh_degree, rasterize_mode == "antialiased", block_width, crop_ids,
                     config_sh_degree, tight, beta_min=beta_min)
    if f is None:
        return [empty_outputs(W, H, background) for _ in range(B)]
    xys, depths, conics, cols, opac, gids, bins, empty = f.xys, f.depths, f.conics, f.cols, f.opac, f.gids, f.bins, f.empty
    dev, plain = f.means.device, "log_uncertainties" not in gp
    Cn = cols.shape[2]
    bg = torch.zeros(Cn, device=dev)
    bg[:3] = background
    mx = torch.zeros(2, B, device=dev)          # each view's own channel maxima of the two passes
    if plain:
        img, fT, _ = ops.splat_rasterize_batch(gids, bins, xys, conics, cols, opac, H, W, bg, block_width, chan_max=(3, mx[0]))
        rgb, alpha, _, _ = ops.splat_normalize_outputs_batch(img, 3, fT, mx[0], rgb=True, acc=True)
        return [empty_outputs(W, H, background) if empty[v] else
                {"rgb": rgb[v], "depth": img[v, ..., 3:4], "accumulation": alpha[v], "background": background}
                for v in range(B)]
    img, fT, fidx = ops.splat_rasterize_batch(gids, bins, xys, conics, cols, opac, H, W, bg, block_width, want_final_idx=True,
                                              chan_max=(4, mx[0]))
    rgb, alpha, rgb_var, _ = ops.splat_normalize_outputs_batch(img, 4, fT, mx[0], rgb=True, acc=True, sq_ch=3)
    sq = ops.splat_depth_sqdiff_batch(xys, depths, img, 4)
    dv, fT2, _ = ops.splat_rasterize_batch(gids, bins, xys, conics, sq[..., None], opac, H, W, None, block_width,
                                           stop_idx=fidx, chan_max=(0, mx[1]))
    _, _, _, dstd = ops.splat_normalize_outputs_batch(dv, 0, fT2, mx[1], sqrt=True)
    return [empty_outputs(W, H, background) if empty[v] else
            {"rgb": rgb[v], "depth": img[v, ..., 4:5], "accumulation": alpha[v], "background": background,
             "uncertainty": img[v, ..., 3:4], "rgb_var": rgb_var[v], "rgb_std": img[v, ..., 3:4], "depth_var": dv[v],
             "depth_std": dstd[v]}
            for v in range(B)]


# Cells of benchmarks/splat_pose_jacobian_batch.py in which the shared launches were slower per view than the loop of
# pose_jacobian_camera by more than that loop's own spread: (H * W at least, views at least) -> the loop is taken.  None of the
# 48 measured cells is (profiles/r21_splat_pose_jacobian_batch.json).
POSE_JACOBIAN_BATCH_LOOP_CELLS: tuple = ()


def pose_jacobian_cameras(gp: Dict[str, torch.Tensor], c2ws: torch.Tensor, fx, fy, cx, cy, H: int, W: int,
                          background: torch.Tensor, projs=None, pose_covs=None, channels=ops.POSE_CHANNELS,
                          want=("proj", "val"), sh_degree: int = 3, rasterize_mode: str = "classic", block_width: int = 16,
                          crop_ids: Optional[torch.Tensor] = None, config_sh_degree: Optional[int] = None,
                          tight: bool = True) -> List[Dict[str, torch.Tensor]]:
    """pose_jacobian_camera for B cameras of one splat set and one image size in shared launches: c2ws [B,3|4,4]; fx, fy, cx,
    cy: scalars or B values.  Returns B dicts, element v BIT-identical to pose_jacobian_camera with camera v.
    projs: None (d / d c2w, 12 columns), one [12,P] for all views, or B of them ([B,12,P] or a list); pose_covs instead of
    projs: None, one [6,6] / 6-vector or B of them -> posegrad.pose_projection(c2w_v, cov) per view (the se3 basis with
    pose_covs=None is projs=[posegrad.pose_projection(c) for c in c2ws]).  The crop is applied once, the count is read back
    once (SplatCountBatch), and the views share the project, shade, count, bin-sort, tangent and walk launches; a view that
    pose_jacobian_camera answers with zeros gets them here.  B <= lib.SPLAT_MAX_VIEWS.  The per-view loop of
    pose_jacobian_camera is taken (same results) for images of more than lib.SPLAT_BATCH_MAX_TILES tiles, for projections of
    different widths P in one batch, and in the cells of POSE_JACOBIAN_BATCH_LOOP_CELLS."""
    from . import posegrad
    _l.require_gpu()
    c2ws = c2ws.detach().to("cpu", torch.float32)
    if c2ws.dim() == 2:
        c2ws = c2ws[None]
    B = c2ws.shape[0]
    if not 1 <= B <= _l.SPLAT_MAX_VIEWS:
        raise ValueError(f"pose_jacobian_cameras: {B} cameras, a batch holds 1 to {_l.SPLAT_MAX_VIEWS}")
    fxs, fys, cxs, cys = (_per_view(v, B, n) for v, n in ((fx, "fx"), (fy, "fy"), (cx, "cx"), (cy, "cy")))
    per_view = pose_view_projections(c2ws, projs, pose_covs)
    bits = ops.pose_channel_bits(channels)
    want = _check_want("pose_jacobian_cameras", want)
    if rasterize_mode not in ("classic", "antialiased"):
        raise ValueError(f"Unknown rasterize_mode: {rasterize_mode}")
    tiles_n = ((W + block_width - 1) // block_width) * ((H + block_width - 1) // block_width)
    widths = {int(m.shape[1]) for _, m in per_view}
    if (tiles_n > _l.SPLAT_BATCH_MAX_TILES or len(widths) != 1
            or any(H * W >= hw and B >= b for hw, b in POSE_JACOBIAN_BATCH_LOOP_CELLS)):
        return [pose_jacobian_camera(gp, c2ws[v], fxs[v], fys[v], cxs[v], cys[v], H, W, background, proj=per_view[v][0],
                                     channels=channels, want=want, sh_degree=sh_degree, rasterize_mode=rasterize_mode,
                                     block_width=block_width, crop_ids=crop_ids, config_sh_degree=config_sh_degree, tight=tight)
                for v in range(B)]
    background = background.to(gp["means"].device, torch.float32)
    (P,) = widths
    rows = [k for k in range(len(ops.POSE_CHANNELS)) if bits >> k & 1]
    f = _views_front(gp, c2ws, fxs, fys, cxs, cys, H, W, sh_degree, rasterize_mode == "antialiased", block_width, crop_ids,
                     config_sh_degree, tight, projs=torch.stack([m for _, m in per_view]))
    if f is None:
        return [_pose_jacobian_empty(H, W, rows, P, want, background) for _ in range(B)]
    res = ops.splat_pose_jacobian_batch(f.gids, f.bins, f.xys, f.conics, f.cols, f.depths, f.opac, f.ptan, P, H, W, background,
                                        compensation=f.comp, channels=channels, want=want, block_width=block_width)
    return [_pose_jacobian_empty(H, W, rows, P, want, background) if f.empty[v] else {k: res[k][v] for k in want}
            for v in range(B)]


def pose_view_projections(c2ws: torch.Tensor, projs=None, pose_covs=None) -> List[tuple]:
    """per view of c2ws [B,3|4,4]: (the [12,P] projection in c2w entries or None, posegrad.splat_view_projection of it) -- the
    matrices pose_jacobian_camera would be given and would build, camera by camera.  Host only."""
    from . import posegrad
    B = c2ws.shape[0]
    if projs is not None and pose_covs is not None:
        raise ValueError("pose_jacobian_cameras: give projs or pose_covs, not both")

    def one_per_view(x, single, name: str):
        if x is None:
            return [None] * B
        if not isinstance(x, (list, tuple)):
            x = torch.as_tensor(x)
            if single(x):
                return [x] * B
            x = list(x)
        if len(x) != B:
            raise ValueError(f"pose_jacobian_cameras: {len(x)} {name} for {B} cameras (give one, or one per camera)")
        return list(x)

    if pose_covs is not None:
        # one tensor [6] or [6,6] is one covariance for all cameras; a list (or [B,6], [B,6,6] with B != 6) is one per camera
        covs = one_per_view(pose_covs, lambda t: tuple(t.shape) in ((6,), (6, 6)), "pose_covs")
        ps = [posegrad.pose_projection(c2ws[v], covs[v]) for v in range(B)]
    else:
        ps = one_per_view(projs, lambda t: t.dim() == 2, "projs")
    try:
        return [(ps[v], posegrad.splat_view_projection(c2ws[v], ps[v], _l.SPLAT_POSE_MAX_P)) for v in range(B)]
    except ValueError as e:
        raise _l.UnerfError(f"pose_jacobian_cameras: {e}") from None
