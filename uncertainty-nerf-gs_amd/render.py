"""Frame-level NeRF pipelines on the HIP kernels.

One call renders a batch of rays the way the reference renders one eval chunk
(`Model.get_outputs_for_camera_ray_bundle` -> `forward` -> `get_outputs`), but with a launch
granularity chosen for MI355X: `rays_per_launch` (default 2^20: a 1080p frame is two launch groups; the K = 8 sample
buffers of one group are 6.4 GB) rays go through the seven kernels at once -- 288 GB of HBM make the reference's
32768-ray chunking unnecessary (2^18 -> 2^20 is worth 1.5-2 % of a frame: fewer partially filled last rounds; measured
in profiles/r3_12_exp_rays_per_launch.json); the only
place the reference chunk size is observable (DepthRenderer("expected") clips to the chunk's
min/max sample position) is reproduced exactly through `chunk_rays`.

Kernel sequence per launch group:
  sampling stage : proposal_density(256) -> weights_pdf_resample(->96) -> proposal_density(96)
                   -> weights_pdf_resample(->48) -> field_gather (level-major hash-grid lookup)
  shading stage  : field_fwd (hash grid + MLPs on the f16 matrix pipe: "f16" / split-f16 "f16x2" / exact "fp32", see
                   ops.FieldDev.precision) -> [laplace_depth_weights] -> composite_var | composite_moments over K

By default the hash-grid lookup is fused into `field_fwd` and everything runs on the caller's
stream.  Two measured alternatives are kept as options (numbers: DESIGN.md section 4.3):
`scene.split_gather` (level-major gather kernel, one 4-MiB level table = one XCD L2 at a time) and
`render_camera(overlap=True)` (sampling stage of launch group g+1 on a second HIP stream underneath
the shading stage of group g).  On MI355X neither beats the fused single-stream form for these
shapes: the stages contend for the same CUs' issue slots and register file.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import lib as _l
from . import ops


def _linspace_bins(n: int) -> torch.Tensor:
    return torch.linspace(0.0, 1.0, n + 1)


def _pdf_u(m: int) -> torch.Tensor:
    nb = m + 1
    u = torch.linspace(0.0, 1.0 - (1.0 / nb), steps=nb)
    return u + 1.0 / (2 * nb)


@dataclass
class NerfSceneDev:
    """Device-resident nerfacto-family scene: main field + proposal networks + sampler constants
    (NerfactoModelConfig defaults)."""
    field: ops.FieldDev
    props: List[ops.DensityNetDev]
    near: float = 0.05
    far: float = 1000.0
    num_prop: Tuple[int, ...] = (256, 96)
    num_nerf: int = 48
    prop_average_init_density: float = 0.01
    chunk_rays: int = 1 << 15
    # proposal_initial_sampler: lib.SPACING_PIECEWISE (nerfacto default) | lib.SPACING_UNIFORM (README.md:153 of the reference)
    spacing: int = 0
    # RGBRenderer background as (UNERF_BG_* mode, colour | None) from ops.background_of(config.background_color);
    # None = "last_sample"
    background: Optional[Tuple] = None
    split_gather: bool = False  # True: level-major gather kernel + feature planes instead of the fused lookup
    # field outputs as sample-major planes + lane-per-ray composite (ACTIVE / MCDROPOUT).  Measured alternative, off by
    # default: the plane stores cut the field kernel's write traffic to the algorithmic bytes, but the lane-per-ray
    # composite is latency-bound and costs more than the stores gain; UNERF_SAMPLE_MAJOR=1 turns it on
    sample_major: bool = field(default_factory=lambda: os.environ.get("UNERF_SAMPLE_MAJOR", "0") == "1")
    # OverflowGuard: re-render launch groups whose f16 operands overflowed with fp32 kernels (UNERF_OVERFLOW_GUARD=0: off)
    overflow_guard: bool = field(default_factory=lambda: os.environ.get("UNERF_OVERFLOW_GUARD", "1") != "0")
    overflow_rerenders: int = 0      # how many launch groups that has happened to (diagnostic)
    # field outputs as packed (sigma, r, g, b) rows (include/unerf.h: packed_out)
    packed_out: bool = field(default_factory=lambda: os.environ.get("UNERF_PACKED_OUT", "1") != "0")
    # scratch arena of the frame path's per-launch-group temporaries (ops.Workspace; UNERF_WORKSPACE=0: per-call allocations)
    workspace: Optional[ops.Workspace] = field(
        default_factory=lambda: ops.Workspace() if os.environ.get("UNERF_WORKSPACE", "1") != "0" else None)
    _const: Dict[str, torch.Tensor] = field(default_factory=dict)

    @property
    def device(self):
        return self.field.table.device

    def const(self, name: str, n: int) -> torch.Tensor:
        key = f"{name}{n}"
        if key not in self._const:
            t = _linspace_bins(n) if name == "bins" else _pdf_u(n)
            self._const[key] = t.to(self.device)
        return self._const[key]


class OverflowGuard:
    """The f16 matrix kernels (precision "f16x2" / "f16") carry activations as f16 operands: a hidden unit or logit at or
    beyond 65504 becomes hi = inf, lo = -inf and poisons its sample with NaN -- which the renderers' nan_to_num would
    turn into a plausible pixel.  Trained nerfacto fields sit orders of magnitude below that, so nothing is clamped in the
    hot loops; instead every composite call ORs a "saw a NaN density / colour" bit into one device word per launch group
    (unerf_composite_*: nonfinite_flag), the words of a frame are read back ONCE at its end, and a group whose word is
    set is rendered again with the exact-fp32 kernels, which have no such limit.  A NaN the fp32 kernels produce too
    (inf density x selector 0, as in the reference) survives the re-render unchanged."""

    def __init__(self, scene: "NerfSceneDev", n_groups: int):
        f = getattr(scene, "field", None)
        on = (f is not None and f.use_mfma and f.precision != "fp32" and f.mfma16_blob is not None
              and getattr(scene, "overflow_guard", True))
        self.scene = scene
        self.flags = torch.zeros(max(n_groups, 1), dtype=torch.int32, device=scene.device) if on else None
        self.rerendered: List[int] = []

    def flag(self, g: int) -> Optional[torch.Tensor]:
        return None if self.flags is None else self.flags[g:g + 1]

    def offenders(self) -> List[int]:
        """launch groups that saw a NaN -- one device -> host read per frame"""
        if self.flags is None:
            return []
        return [i for i, f in enumerate(self.flags.tolist()) if f]     # one small device -> host copy (the frame's sync)

    def redo(self, g: int, render_group):
        """render_group() again with the exact-fp32 kernels"""
        f = self.scene.field
        saved, f.precision = f.precision, "fp32"
        try:
            out = render_group()
        finally:
            f.precision = saved
        self.rerendered.append(g)
        self.scene.overflow_rerenders += 1
        return out


def sample_rays(scene: NerfSceneDev, origins: torch.Tensor, directions: torch.Tensor, clip: Optional[torch.Tensor],
                ray_offset: int = 0, want_prop_depth: bool = True, image_width: int = 0,
                init_bins: Optional[torch.Tensor] = None, workspace: Optional[ops.Workspace] = None,
                views: Optional[ops.RayViews] = None):
    """ProposalNetworkSampler at eval.  -> (final spacing bins [R,S+1], [prop_depth_0, prop_depth_1])
    views: the rays are several whole views (render_cameras): `clip` holds each view's own chunk rows
    workspace (the frame path only): the bins are a view of that scratch arena, not a tensor of their own
    init_bins [R, num_prop[0]+1]: per-ray first-level bins (a bundle with its own nears / fars: `crop_bins`), else
    the shared uniform row"""
    sb = scene.const("bins", scene.num_prop[0]) if init_bins is None else init_bins
    prop_depths = []
    n_iter = len(scene.props)
    for lvl in range(n_iter):
        dens = ops.proposal_density(origins, directions, sb, scene.props[lvl], scene.near, scene.far,
                                    scene.prop_average_init_density, ray_offset=ray_offset, image_width=image_width,
                                    spacing=scene.spacing, workspace=workspace)
        m = scene.num_prop[lvl + 1] if lvl + 1 < n_iter else scene.num_nerf
        last = lvl + 1 == n_iter
        sb, pd, _ = ops.weights_pdf_resample(dens, sb, scene.const("u", m), scene.near, scene.far,
                                             want_prop_depth=want_prop_depth,
                                             clip_minmax=clip if last else None, ray_offset=ray_offset,
                                             chunk_rays=scene.chunk_rays, spacing=scene.spacing, workspace=workspace,
                                             views=views if last else None)
        prop_depths.append(pd)
    return sb, prop_depths


def _unpack(out: torch.Tensor) -> Dict[str, torch.Tensor]:
    return {
        "rgb": out[:, 0:3], "accumulation": out[:, 3:4], "depth": out[:, 4:5], "expected_depth": out[:, 5:6],
        "rgb_var": out[:, 6:7], "depth_var": out[:, 7:8],
    }


def _uses_split(scene: NerfSceneDev) -> bool:
    f = scene.field
    return bool(scene.split_gather and f.mode != _l.FIELD_LAPLACE and f.use_mfma and f.mfma_blob is not None
                and f.tcnn_levels is None)


def crop_bins(scene: NerfSceneDev, origins, directions, obb=None, nears=None, fars=None) -> Optional[torch.Tensor]:
    """First-level bins for rays whose planes are not the collider's: `obb` = (world_to_box [3,4], S [3]) of an
    OrientedBox -- what Cameras.generate_rays(..., obb_box=box) does to the bundle (laplace_model.py:413,
    ensemble_pipeline.py:157) -- or the bundle's own nears / fars [R,1]."""
    row = scene.const("bins", scene.num_prop[0])
    if obb is not None:
        return ops.ray_box_bins(origins, directions, obb[0], obb[1], scene.near, scene.far, row, spacing=scene.spacing)[0]
    if nears is not None and fars is not None:
        return ops.ray_planes_bins(nears, fars, scene.near, scene.far, row, spacing=scene.spacing)
    return None


def sampling_stage(scene: NerfSceneDev, origins, directions, clip, ray_offset: int, image_width: int = 0,
                   init_bins: Optional[torch.Tensor] = None, scratch: bool = True, views: Optional[ops.RayViews] = None):
    """-> (final spacing bins, prop depths, feature planes | None); the frame path's stage: its temporaries live in
    scene.workspace.  scratch=False (render_camera(overlap=True)): tensors of their own -- there the bins of group g are
    still being read by the shading stream while this stage runs for group g + 1"""
    sb, prop_depths = sample_rays(scene, origins, directions, clip, ray_offset, image_width=image_width,
                                  init_bins=init_bins, workspace=scene.workspace if scratch else None, views=views)
    feats = (ops.field_gather(origins, directions, sb, scene.field, scene.near, scene.far, spacing=scene.spacing)
             if _uses_split(scene) else None)
    return sb, prop_depths, feats


def shading_stage(scene: NerfSceneDev, origins, directions, sb, prop_depths, feats, clip, ray_offset: int = 0,
                  depth_noise: Optional[torch.Tensor] = None, depth_draws: int = 100, depth_seed: int = 0,
                  keep_density: bool = False, image_width: int = 0,
                  nonfinite_flag: Optional[torch.Tensor] = None,
                  keep_masks: Optional[ops.KeepMasks] = None, views: Optional[ops.RayViews] = None,
                  lap_views: Optional[ops.LaplaceViews] = None) -> Dict[str, torch.Tensor]:
    """views: the rays are several whole views (render_cameras): the mask counter and the clip rows are numbered inside
    each view's own frame (ops.RayViews); ray_offset is then 0, the row of the tall image the launch starts at.
    lap_views (LAPLACE with views): every view's first sample set in the field's stacks and the seed of its depth draws
    (ops.LaplaceViews; None: set 0 and depth_seed for every view).
    keep_masks (MCDROPOUT): the FRAME's explicit keep masks (ops.KeepMasks over all its rays, row = ray * S + sample);
    this launch group reads them from row ray_offset * S.  The fp32 re-render of the overflow guard and the two-stream
    path come through here with the same masks."""
    f = scene.field
    # ACTIVE / MCDROPOUT: the field kernel writes sample-major planes (whole 32-byte sectors per store) and the
    # composite walks them with a lane per ray; LAPLACE keeps the ray-major layout its depth-draw kernel reads
    planes = scene.sample_major and feats is None and ops.supports_planes(f)
    # default (ACTIVE / MCDROPOUT): one 16-byte row (sigma, r, g, b) per sample instead of four scattered dwords
    # (unerf_field_params.packed_out; UNERF_PACKED_OUT=0: the [B,R,S] + [B,R,S,3] layout of the Field-level API)
    packed = scene.packed_out and not planes and ops.supports_packed(f)
    density, rgb, aux, aux2 = ops.field_fwd(origins, directions, sb, f, scene.near, scene.far, ray_offset, features=feats,
                                            image_width=image_width, sample_major=planes, spacing=scene.spacing,
                                            nonfinite_flag=nonfinite_flag, packed=packed, workspace=scene.workspace, views=views,
                                            lap_views=lap_views if f.mode == _l.FIELD_LAPLACE else None,
                                            keep_masks=None if keep_masks is None else keep_masks.at(ray_offset * (sb.shape[1] - 1)))
    kw = dict(clip_minmax=clip, ray_offset=ray_offset, chunk_rays=scene.chunk_rays, spacing=scene.spacing,
              background=scene.background, nonfinite_flag=nonfinite_flag)
    if views is not None:
        if planes:
            raise _l.UnerfError("shading_stage: several views per launch are built for the ray-major path")
        kw["views"] = views
    res: Dict[str, torch.Tensor] = {}
    if f.mode == _l.FIELD_ACTIVE:
        if planes:
            out = ops.composite_var_planes(density, rgb, sb, scene.near, scene.far, beta=aux, **kw)[0]
        else:
            out = ops.composite_var(density, rgb, sb, scene.near, scene.far, beta=aux, **kw)[0]
        res = _unpack(out)
        res["rgb_std"] = res["rgb_var"].sqrt()
        res["depth_std"] = res["depth_var"].sqrt()
        if keep_density:   # the reference returns density [R,48,1] (activenerfacto_model.py:115,122)
            # (a copy: the kernel's rows live in scene.workspace and the next launch group overwrites them)
            res["density"] = (rgb[0][..., 0] if packed else (density[0].t() if planes else density[0])).clone(
                memory_format=torch.contiguous_format)
    elif f.mode == _l.FIELD_MCDROPOUT:
        if planes and f.K >= 2:
            mean, var = ops.composite_moments_planes(density, rgb, sb, scene.near, scene.far, **kw)
        elif planes and f.K == 1:
            mean = ops.composite_var_planes(density, rgb, sb, scene.near, scene.far, **kw)[0]
            var = torch.full_like(mean, float("nan"))       # torch.std of one pass (unbiased) is NaN
        elif 0 < f.K <= 16:
            mean, var = ops.composite_moments(density, rgb, sb, scene.near, scene.far, **kw)
        elif f.K > 16:
            out = ops.composite_var(density, rgb, sb, scene.near, scene.far, **kw)  # [B,R,8]
            mean, var = ops.moments(out[:, :, :6].contiguous())
        if f.K > 0:
            res = {"rgb": mean[:, 0:3], "accumulation": mean[:, 3:4], "depth": mean[:, 4:5],
                   "expected_depth": mean[:, 5:6]}
            std = var.sqrt()
            res["rgb_std"] = std[:, 0:3].mean(dim=-1)[..., None]
            res["depth_std"] = std[:, 4:5].mean(dim=-1)[..., None]
            res["expected_depth_std"] = std[:, 5:6].mean(dim=-1)[..., None]
        else:
            comp = ops.composite_var_planes if planes else ops.composite_var
            u = _unpack(comp(density, rgb, sb, scene.near, scene.far, **kw)[0])
            res = {k: u[k] for k in ("rgb", "accumulation", "depth", "expected_depth")}
    else:
        # use_deterministic_density (laplace_model.py:486-507 is skipped): depth from the ordinary weights
        walt = None if f.lap_mask_density else ops.laplace_depth_weights(
            density[0], aux, sb, scene.near, scene.far, depth_noise, depth_draws, depth_seed, ray_offset,
            spacing=scene.spacing, views=views, lap_views=lap_views if views is not None else None)
        out = ops.composite_var(density, rgb, sb, scene.near, scene.far, beta=aux2, weights_alt=walt, **kw)[0]
        u = _unpack(out)
        res = {"rgb": u["rgb"], "rgb_std": u["rgb_var"].sqrt(), "accumulation": u["accumulation"],
               "depth": u["depth"], "depth_std": u["depth_var"].sqrt(), "expected_depth": u["expected_depth"]}
    for i, pd in enumerate(prop_depths):
        if pd is not None:
            res[f"prop_depth_{i}"] = pd
    return res


def render_rays(scene: NerfSceneDev, origins: torch.Tensor, directions: torch.Tensor, ray_offset: int = 0,
                total_rays: Optional[int] = None, clip: Optional[torch.Tensor] = None,
                init_bins: Optional[torch.Tensor] = None, views: Optional[ops.RayViews] = None,
                **shade_kw) -> Dict[str, torch.Tensor]:
    """Render rays [R,3] with the scene's method (field.mode).  Output keys follow the reference:
      ACTIVE     activenerfacto_model.py:117-127   rgb accumulation depth expected_depth rgb_var rgb_std
                                                   depth_var depth_std prop_depth_i (+density)
      MCDROPOUT  mcdropout_models.py:121-126       means of every key + rgb_std depth_std expected_depth_std
      LAPLACE    laplace_model.py:523-530          rgb rgb_std accumulation depth depth_std expected_depth
    keep_masks= (MCDROPOUT, with the other shading arguments): explicit keep masks of the frame, see shading_stage.
    views= (render_cameras): the rays are several whole views of one size; `clip` must then be given, with each view's rows.
    """
    _l.require_gpu()
    R = origins.shape[0]
    if clip is None:
        if views is not None:
            raise _l.UnerfError("render_rays(views=...): pass the clip buffer (clip_rows_per_view rows per view)")
        clip = ops.new_clip_buffer((total_rays or (ray_offset + R)), scene.chunk_rays, origins.device)
    sb, prop_depths, feats = sampling_stage(scene, origins, directions, clip, ray_offset,
                                            image_width=shade_kw.get("image_width", 0), init_bins=init_bins, views=views)
    return shading_stage(scene, origins, directions, sb, prop_depths, feats, clip, ray_offset, views=views, **shade_kw)


def render_camera(scene: NerfSceneDev, c2w: torch.Tensor, fx: float, fy: float, cx: float, cy: float, H: int, W: int,
                  rays_per_launch: int = 1 << 20, overlap: bool = False, obb=None, distortion=None, camera_type: int = 1,
                  **shade_kw) -> Dict[str, torch.Tensor]:
    """get_outputs_for_camera: generate the H*W rays on device, render them in row-major launch
    groups, return images [H,W,C].  With `overlap`, sampling (group g+1) and shading (group g) run on
    two streams.  obb = (world_to_box [3,4], S [3]): the oriented crop box of `obb_box` (see crop_bins).
    distortion = the camera's `distortion_params` (k1, k2, k3, k4, p1, p2) or None: the rays are bent as
    Cameras.generate_rays bends them (unerf_generate_rays).  camera_type: nerfstudio's CameraType value (perspective 1,
    fisheye 2, equirectangular 3, orthophoto 8: include/unerf.h).
    keep_masks= (MCDROPOUT): an ops.KeepMasks over the H*W rays of the frame instead of the counter generator's masks."""
    _l.require_gpu()
    total = H * W
    dev = scene.device
    clip = ops.new_clip_buffer(total, scene.chunk_rays, dev)
    # launch groups must not split a reference chunk (the clip bounds are per chunk)
    rpl = max(scene.chunk_rays, (rays_per_launch // scene.chunk_rays) * scene.chunk_rays)
    starts = list(range(0, total, rpl))
    lists: Dict[str, List[torch.Tensor]] = {}
    with torch.cuda.device(dev):
        cur = torch.cuda.current_stream()
        guard = OverflowGuard(scene, len(starts))

        def group(gi: int, flag=None):
            start = starts[gi]
            o, d, _ = ops.generate_rays(c2w, fx, fy, cx, cy, H, W, dev, start, min(rpl, total - start), distortion=distortion,
                                        camera_type=camera_type)
            return render_rays(scene, o, d, ray_offset=start, total_rays=total, clip=clip, image_width=W,
                               init_bins=crop_bins(scene, o, d, obb), nonfinite_flag=flag, **shade_kw)

        if not overlap or len(starts) == 1:
            for gi in range(len(starts)):
                out = group(gi, guard.flag(gi))
                for k, v in out.items():
                    lists.setdefault(k, []).append(v)
            for gi in guard.offenders():
                # (the sampling stage is fp32 in every precision: it reproduces the group's sample positions, so the
                # per-chunk clip bounds it re-accumulates with atomic min / max do not move)
                out = guard.redo(gi, lambda: group(gi))
                for k, v in out.items():
                    lists[k][gi] = v
        else:
            s_samp, s_shade = _streams(dev)
            s_samp.wait_stream(cur)
            s_shade.wait_stream(cur)
            for gi, start in enumerate(starts):
                with torch.cuda.stream(s_samp):
                    o, d, _ = ops.generate_rays(c2w, fx, fy, cx, cy, H, W, dev, start, min(rpl, total - start), distortion=distortion,
                                        camera_type=camera_type)
                    sb, pds, feats = sampling_stage(scene, o, d, clip, start, image_width=W,
                                                    init_bins=crop_bins(scene, o, d, obb), scratch=False)
                    ev = torch.cuda.Event()
                    ev.record(s_samp)
                    for t in (o, d, sb, feats, *pds):   # handed to the other stream: keep the allocator honest
                        if t is not None:
                            t.record_stream(s_shade)
                with torch.cuda.stream(s_shade):
                    s_shade.wait_event(ev)
                    out = shading_stage(scene, o, d, sb, pds, feats, clip, start, image_width=W,
                                        nonfinite_flag=guard.flag(gi), **shade_kw)
                    for v in out.values():
                        v.record_stream(cur)
                for k, v in out.items():
                    lists.setdefault(k, []).append(v)
            cur.wait_stream(s_shade)
            cur.wait_stream(s_samp)
            for gi in guard.offenders():
                for k, v in guard.redo(gi, lambda: group(gi)).items():
                    lists[k][gi] = v
        return {k: torch.cat(v).view(H, W, -1) for k, v in lists.items()}


def pose_gradient_camera(scene: NerfSceneDev, c2w: torch.Tensor, fx: float, fy: float, cx: float, cy: float, H: int, W: int,
                         rays_per_launch: int = 1 << 20, obb=None, distortion=None, camera_type: int = 1,
                         want_rgb: bool = False):
    """d mean_c(rgb[y, x]) / d c2w for every pixel of one camera -> [H,W,3,4] float32 on the device (with want_rgb:
    also the colour unerf_pose_grad composited, [H,W,3]) -- the per-pixel autograd loop of the reference's
    estimate_gradient_pose_6dof.py:128-139 as ray kernel -> proposal sampler -> one gradient launch per group of
    rays_per_launch rays.  The sample bins are held fixed, as upstream's PDFSampler detaches them: the pose acts through
    the ray origins (c2w[:, 3]) and the directions normalize(c2w[:3, :3] dir_cam) only.  ORTHOPHOTO cameras and `obb`
    crops are refused: their origins / sampling planes depend on the pose themselves."""
    return _pose_gradient_groups("pose_gradient_camera", scene, c2w, fx, fy, cx, cy, H, W, rays_per_launch, obb, distortion,
                                 camera_type, want_rgb,
                                 lambda o, d, sb, start, rot_inv: ops.pose_grad(o, d, sb, scene.field, scene.near, scene.far,
                                                                                rot_inv=rot_inv, spacing=scene.spacing,
                                                                                background=scene.background, want_rgb=want_rgb))


def _pose_gradient_groups(what: str, scene: NerfSceneDev, c2w: torch.Tensor, fx, fy, cx, cy, H: int, W: int, rays_per_launch: int,
                          obb, distortion, camera_type: int, want_rgb: bool, launch):
    """pose_gradient_camera / pose_gradient_camera_mc / pose_gradient_camera_laplace: _pose_group_results' loop, the groups'
    gradients joined to [H,W,3,4]"""
    res = _pose_group_results(what, scene, c2w, fx, fy, cx, cy, H, W, rays_per_launch, obb, distortion, camera_type, launch)
    g = torch.cat([r[0] if want_rgb else r for r in res]).view(H, W, 3, 4)
    return (g, torch.cat([r[1] for r in res]).view(H, W, 3)) if want_rgb else g


def _pose_group_results(what: str, scene: NerfSceneDev, c2w: torch.Tensor, fx, fy, cx, cy, H: int, W: int, rays_per_launch: int,
                        obb, distortion, camera_type: int, launch) -> list:
    """the loop of the pose_gradient_camera* functions and pose_jacobian_camera: rays -> proposal sampler ->
    launch(o, d, sb, start, rot_inv) per group of rays_per_launch rays -> the groups' results in ray order"""
    _l.require_gpu()
    if int(camera_type) == _l.CAMERA_ORTHOPHOTO:
        raise _l.UnerfError(f"{what}: an ORTHOPHOTO camera's ray origins depend on the rotation; not differentiated")
    if obb is not None:
        raise _l.UnerfError(f"{what}: obb crops make the sampling planes depend on the pose; not differentiated")
    total = H * W
    dev = scene.device
    c2w = c2w.detach().cpu().to(torch.float32)
    rot_inv = torch.linalg.inv(c2w[:3, :3].double()).to(torch.float32)
    rpl = max(1, int(rays_per_launch))
    results = []
    with torch.cuda.device(dev):
        for start in range(0, total, rpl):
            o, d, _ = ops.generate_rays(c2w, fx, fy, cx, cy, H, W, dev, start, min(rpl, total - start), distortion=distortion,
                                        camera_type=camera_type)
            sb, _ = sample_rays(scene, o, d, None, start, want_prop_depth=False, image_width=W, workspace=scene.workspace)
            results.append(launch(o, d, sb, start, rot_inv))
    return results


def pose_jacobian_camera(scene: NerfSceneDev, c2w: torch.Tensor, fx: float, fy: float, cx: float, cy: float, H: int, W: int,
                         channels=ops.POSE_CHANNELS, proj=None, want=("jac",), rays_per_launch: int = 1 << 20, obb=None,
                         distortion=None, camera_type: int = 1):
    """ops.pose_jacobian for every pixel of one camera, with respect to c2w (D = 12, row-major 3x4): the loop of
    pose_gradient_camera (bins held fixed; ORTHOPHOTO cameras and `obb` crops refused), one launch per group of
    rays_per_launch rays, which the result does not depend on.  proj: None or [12,P] (posegrad.pose_projection).
    -> {"jac": [H,W,C,12], "proj": [H,W,C,P], "var": [H,W,C], "val": [H,W,C]}, the entries `want` names; the C rows in
    ops.POSE_CHANNELS order.  The expected depth is the unclipped quotient (include/unerf.h: unerf_pose_jacobian)."""
    if scene.field.mode not in (_l.FIELD_ACTIVE, _l.FIELD_MCDROPOUT):
        raise _l.UnerfError("pose_jacobian_camera: the scene's field is not a nerfacto / active-nerfacto field (not built for "
                            "the Laplace field)")
    want = (want,) if isinstance(want, str) else tuple(want)
    res = _pose_group_results("pose_jacobian_camera", scene, c2w, fx, fy, cx, cy, H, W, rays_per_launch, obb, distortion,
                              camera_type,
                              lambda o, d, sb, start, rot_inv: ops.pose_jacobian(o, d, sb, scene.field, scene.near, scene.far,
                                                                                 rot_inv=rot_inv, channels=channels, proj=proj,
                                                                                 spacing=scene.spacing,
                                                                                 background=scene.background, want=want))
    out = {}
    for k in want:
        t = torch.cat([r[k] for r in res])
        out[k] = t.view(H, W, *t.shape[1:])
    return out


def _frame_rows(what: str, name: str, t, H: int, W: int, widths, dev, dtype=torch.float32):
    """an [H,W] / [H,W,k] frame input (k one of `widths`) -> contiguous [H W, k] on the device, or None"""
    if t is None:
        return None
    t = torch.as_tensor(t)
    k = 1 if t.dim() == 2 else (int(t.shape[-1]) if t.dim() == 3 else -1)
    if tuple(t.shape[:2]) != (H, W) or k not in widths:
        raise ValueError(f"{what}: {name} must be [{H},{W}] or [{H},{W},k] with k in {sorted(widths)}, got {tuple(t.shape)}")
    if dtype == torch.uint8:
        t = t != 0
    return t.to(device=dev, dtype=dtype).reshape(H * W, k).contiguous()


def pose_normal_eq_camera(scene: NerfSceneDev, c2w: torch.Tensor, fx: float, fy: float, cx: float, cy: float, H: int, W: int,
                          target=None, weights=None, mask=None, channels=("r", "g", "b"), pose_cov_prior=None,
                          rays_per_launch: int = 1 << 20, obb=None, distortion=None, camera_type: int = 1):
    """The pose normal equations of one camera's frame in the six se3 parameters (posegrad.POSE_PARAMS, c2w . exp(xi)): the loop
    of pose_jacobian_camera with proj = posegrad.tangent_basis(c2w), but every launch group's [R,C,6] Jacobian and values are
    reduced at once (ops.pose_normal_eq_accumulate) and dropped -- the frame's Jacobian is never held or joined.
    target [H,W,C] (C = len(channels), in ops.POSE_CHANNELS order) or None (information only: gradient and chi2 are exactly 0);
    weights None | [H,W] | [H,W,1] | [H,W,C]; mask None | [H,W] (0 = left out).  rays_per_launch must be a multiple of
    lib.POSE_NEQ_TILE; the result does not depend on it, bit for bit.
    -> {"information" [6,6], "gradient" [6], "chi2", "n_used", "n_skipped", "covariance" [6,6], "rank"}: float64 host values,
    covariance = posegrad.pose_covariance(information, pose_cov_prior)."""
    from . import posegrad
    what = "pose_normal_eq_camera"
    if scene.field.mode not in (_l.FIELD_ACTIVE, _l.FIELD_MCDROPOUT):
        raise _l.UnerfError(f"{what}: the scene's field is not a nerfacto / active-nerfacto field (not built for the Laplace field)")
    rpl = int(rays_per_launch)
    if rpl < _l.POSE_NEQ_TILE or rpl % _l.POSE_NEQ_TILE:
        raise ValueError(f"{what}: rays_per_launch = {rpl} must be a positive multiple of POSE_NEQ_TILE = {_l.POSE_NEQ_TILE}")
    Cn = bin(ops.pose_channel_bits(channels)).count("1")
    dev = scene.device
    tg = _frame_rows(what, "target", target, H, W, {Cn}, dev)
    wt = _frame_rows(what, "weights", weights, H, W, {1, Cn}, dev)
    mk = _frame_rows(what, "mask", mask, H, W, {1}, dev, torch.uint8)
    proj = posegrad.tangent_basis(c2w)
    ws = ops.pose_normal_eq_workspace(H * W, 6, dev)

    def launch(o, d, sb, start, rot_inv):
        R = o.shape[0]
        r = ops.pose_jacobian(o, d, sb, scene.field, scene.near, scene.far, rot_inv=rot_inv, channels=channels, proj=proj,
                              spacing=scene.spacing, background=scene.background, want=("proj", "val") if tg is not None else ("proj",))
        ops.pose_normal_eq_accumulate(ws, r["proj"], r.get("val"), None if tg is None else tg[start:start + R],
                                      None if wt is None else wt[start:start + R], None if mk is None else mk[start:start + R],
                                      pixel_offset=start)

    _pose_group_results(what, scene, c2w, fx, fy, cx, cy, H, W, rpl, obb, distortion, camera_type, launch)
    out = ops.pose_normal_eq_finish(ws)
    out["covariance"], out["rank"] = posegrad.pose_covariance(out["information"], pose_cov_prior)
    return out


def pose_gradient_camera_mc(scene: NerfSceneDev, c2w: torch.Tensor, fx: float, fy: float, cx: float, cy: float, H: int, W: int,
                            rays_per_launch: int = 1 << 20, obb=None, distortion=None, camera_type: int = 1,
                            want_rgb: bool = False, keep_masks: Optional[ops.KeepMasks] = None):
    """pose_gradient_camera of an MC-dropout frame under a named mask draw (ops.pose_grad_mc): d mean_c(rgb) / d c2w of
    rgb = the mean of the K dropout passes, one launch per group of rays whatever K is.  The masks are those of the frame
    render_camera makes with the same scene.field.seed: every group is launched with ray_offset = its first ray, the
    numbering render_camera gives the frame's own field launches, so the result does not depend on rays_per_launch.
    keep_masks: an ops.KeepMasks over the H*W rays of the frame (row = ray * S + sample) instead of the counter generator's
    masks; a group reads it from row start * S, as render_camera(keep_masks=) does.  Same refusals as pose_gradient_camera."""
    def launch(o, d, sb, start, rot_inv):
        km = None if keep_masks is None else keep_masks.at(start * (sb.shape[1] - 1))
        return ops.pose_grad_mc(o, d, sb, scene.field, scene.near, scene.far, ray_offset=start, keep_masks=km, rot_inv=rot_inv,
                                spacing=scene.spacing, background=scene.background, want_rgb=want_rgb)

    return _pose_gradient_groups("pose_gradient_camera_mc", scene, c2w, fx, fy, cx, cy, H, W, rays_per_launch, obb, distortion,
                                 camera_type, want_rgb, launch)


def pose_gradient_camera_laplace(scene: NerfSceneDev, c2w: torch.Tensor, fx: float, fy: float, cx: float, cy: float, H: int, W: int,
                                 rays_per_launch: int = 1 << 20, obb=None, distortion=None, camera_type: int = 1,
                                 want_rgb: bool = False):
    """pose_gradient_camera of a Laplace frame under a named draw of the last layers (ops.pose_grad_laplace): d mean_c(rgb) /
    d c2w of rgb = the colour composited from the means over scene.field.ws_density / ws_rgb, one launch per group of rays
    whatever the row counts are.  Every group is launched with ray_offset = its first ray, so with stacked sets a ray reads the
    set render_camera gives it (ray // scene.field.lap_chunk_rays) and the result does not depend on rays_per_launch.  Same
    refusals as pose_gradient_camera."""
    if scene.field.mode != _l.FIELD_LAPLACE:
        raise _l.UnerfError("pose_gradient_camera_laplace: the scene's field is not a LAPLACE field (pose_gradient_camera and "
                            "pose_gradient_camera_mc differentiate the other fields)")
    return _pose_gradient_groups("pose_gradient_camera_laplace", scene, c2w, fx, fy, cx, cy, H, W, rays_per_launch, obb, distortion,
                                 camera_type, want_rgb,
                                 lambda o, d, sb, start, rot_inv: ops.pose_grad_laplace(
                                     o, d, sb, scene.field, scene.near, scene.far, ray_offset=start, rot_inv=rot_inv,
                                     spacing=scene.spacing, background=scene.background, want_rgb=want_rgb))


def plan_view_groups(n_views: int, rays_per_view: int, rays_per_launch: int = 1 << 20, chunk_rays: int = 1 << 15,
                     max_views: int = _l.NERF_MAX_VIEWS) -> Optional[List[Tuple[int, int]]]:
    """How render_cameras fills its launch groups with WHOLE views: [(first view, number of views), ...], or None when a
    view is larger than half a launch group (nothing to share: the per-camera loop).  A group holds
    max(1, rpl // rays_per_view) views, at most max_views (<= lib.NERF_MAX_VIEWS); rpl = rays_per_launch rounded to whole
    chunks as in render_camera.  Pure function of its arguments."""
    rpl = max(chunk_rays, (rays_per_launch // chunk_rays) * chunk_rays)
    if n_views < 1 or rays_per_view < 1:
        raise ValueError(f"plan_view_groups: {n_views} views of {rays_per_view} rays")
    if 2 * rays_per_view > rpl:
        return None
    per = max(1, min(rpl // rays_per_view, max_views, _l.NERF_MAX_VIEWS))
    return [(v0, min(per, n_views - v0)) for v0 in range(0, n_views, per)]


def _per_view(x, B: int, name: str) -> list:
    """one value, or one per camera -> B host values"""
    if torch.is_tensor(x):
        x = x.detach().cpu().reshape(-1).tolist()
    if isinstance(x, (list, tuple)):
        if len(x) == 1:
            return [x[0]] * B
        if len(x) != B:
            raise ValueError(f"render_cameras: {name} has {len(x)} entries for {B} cameras")
        return list(x)
    return [x] * B


def _per_view_distortion(distortion, B: int) -> Optional[list]:
    """None | one 6-vector | B entries (None or 6-vector) -> None (no lens anywhere) | B entries"""
    if distortion is None:
        return None
    if torch.is_tensor(distortion):
        distortion = [distortion] if distortion.dim() == 1 else list(distortion)
    elif len(distortion) == 6 and not any(d is None or hasattr(d, "__len__") for d in distortion):
        distortion = [distortion]
    out = _per_view(list(distortion), B, "distortion")
    return None if all(d is None for d in out) else out


def view_batch_loop_reason(scene: NerfSceneDev, overlap: bool = False, keep_masks=None) -> Optional[str]:
    """Why render_cameras renders this scene camera by camera (None: it shares launches).  The several-views kernels are
    built for the frame path's default form: ACTIVE / MCDROPOUT / LAPLACE on the f16 matrix kernels, fused lookup,
    ray-major rows."""
    f = scene.field
    if keep_masks is not None:
        return "explicit keep masks span one frame"
    if overlap:
        return "overlap=True (two streams)"
    if scene.sample_major:
        return "sample_major planes"
    if scene.split_gather:
        return "split_gather"
    if f.any_width:
        return "an any-width field"
    if not (f.use_mfma and f.precision in ("f16x2", "f16") and f.mfma16_blob is not None):
        return "an fp32 field (no f16 matrix operands)"
    if f.mode == _l.FIELD_MCDROPOUT and f.K > 0 and ops.FieldDev._sites(f.drop_sites) != (_l.DROP_TRUNK | _l.DROP_HEAD1):
        return "non-default dropout sites"
    if f.mode == _l.FIELD_LAPLACE and f.lap16_blob is None:
        return "a Laplace field without f16 head operands (more than 128 sampled rows)"
    return None


def render_cameras(scene: NerfSceneDev, c2ws: torch.Tensor, fx, fy, cx, cy, H: int, W: int, seeds=None,
                   rays_per_launch: int = 1 << 20, overlap: bool = False, obb=None, distortion=None, camera_type=1,
                   max_views: int = _l.NERF_MAX_VIEWS, lap_view_sets=None, depth_seeds=None,
                   **shade_kw) -> List[Dict[str, torch.Tensor]]:
    """get_outputs_for_camera for B cameras of ONE image size: c2ws [B,3|4,4]; fx, fy, cx, cy, camera_type: one value or one
    per camera; distortion: None, one 6-vector or one entry per camera.  -> B dicts of images [H,W,C]; element v is
    bit-identical to render_camera(scene, c2ws[v], ...) -- for MC-dropout with scene.field.seed = seeds[v] (seeds=None:
    every view under the field's own seed).

    Small frames leave most of a launch group empty (a 200 x 200 frame is 40,000 rays of 2^20), so the rays of several
    WHOLE views share one launch group: max(1, rpl // (H W)) views per group (plan_view_groups; a view is never split),
    laid out as one tall row-major image.  The kernels number the clip chunks of the expected depth and the MC-dropout
    mask counter inside each view's own frame (ops.RayViews), which is what keeps a view's bits.  One OverflowGuard word
    per group; the views of a group whose word is set are rendered again one by one with render_camera (which re-renders
    its own offending groups on the fp32 kernels), so they too equal the loop.  scene.workspace, obb and keep_density work
    as in render_camera.

    A Laplace scene (f16 matrix kernels) shares launches too.  lap_view_sets[v] = the first sample set of view v in the
    field's stacks (ws_* / lap16_blob [sets, ...]); view v is rendered with the sets lap_view_sets[v] + [0, sets per view)
    -- sets per view = ceil(H W / field.lap_chunk_rays), 1 without per-chunk sets -- and equals render_camera on the field
    narrowed to those sets (ops.laplace_sets_view).  Default: 0 for every view, the field's own sets, which is what a loop of
    render_camera over the same scene renders.  depth_seeds[v] = the seed of view v's depth draws (default: the depth_seed
    keyword for every view).  The views of a flagged launch group are re-rendered with their own sets and depth seed.

    Rendered as a plain loop over render_camera -- the SAME results, without shared launches -- when H W exceeds half a
    launch group, with keep_masks= (dropout_masks="torch"), with overlap=True, scene.sample_major or scene.split_gather, for
    an any-width or fp32 field, non-default dropout sites, a Laplace field with more than 128 sampled rows, and when the
    camera types of the batch differ (view_batch_loop_reason)."""
    _l.require_gpu()
    B = int(c2ws.shape[0])
    if B < 1:
        return []
    fxs, fys, cxs, cys = (_per_view(v, B, n) for v, n in ((fx, "fx"), (fy, "fy"), (cx, "cx"), (cy, "cy")))
    types = [int(t) for t in _per_view(camera_type, B, "camera_type")]
    dists = _per_view_distortion(distortion, B)
    if seeds is not None and len(seeds) != B:
        raise ValueError(f"render_cameras: {len(seeds)} seeds for {B} cameras")
    total = H * W
    f = scene.field
    c2ws = c2ws.detach().cpu()       # one device -> host copy for the batch (the ray kernels take host camera records)
    laplace = f.mode == _l.FIELD_LAPLACE
    if not laplace and (lap_view_sets is not None or depth_seeds is not None):
        raise ValueError("render_cameras: lap_view_sets / depth_seeds belong to a Laplace scene")
    for name, vals in (("lap_view_sets", lap_view_sets), ("depth_seeds", depth_seeds)):
        if vals is not None and len(vals) != B:
            raise ValueError(f"render_cameras: {len(vals)} {name} for {B} cameras")
    lap_spv = ops.laplace_sets_per_view(f, total) if laplace else 0

    def single(v: int) -> Dict[str, torch.Tensor]:
        saved = f.seed
        if seeds is not None:
            f.seed = int(seeds[v])
        kw = shade_kw
        if depth_seeds is not None:
            kw = dict(shade_kw, depth_seed=int(depth_seeds[v]))
        if lap_view_sets is not None:      # this view's own sets: the stacks narrowed to them
            scene.field = ops.laplace_sets_view(f, int(lap_view_sets[v]), lap_spv)
        try:
            return render_camera(scene, c2ws[v], fxs[v], fys[v], cxs[v], cys[v], H, W, rays_per_launch=rays_per_launch,
                                 overlap=overlap, obb=obb, distortion=None if dists is None else dists[v],
                                 camera_type=types[v], **kw)
        finally:
            f.seed = saved
            scene.field = f

    groups = plan_view_groups(B, total, rays_per_launch, scene.chunk_rays, max_views)
    if (groups is None or len(set(types)) != 1
            or view_batch_loop_reason(scene, overlap, shade_kw.get("keep_masks")) is not None):
        return [single(v) for v in range(B)]
    dev = scene.device
    cpv = ops.clip_rows_per_view(total, scene.chunk_rays)
    clip = ops.new_clip_buffer(B * cpv * scene.chunk_rays, scene.chunk_rays, dev)     # [B * cpv, 2]: every view its own rows
    outs: List[Optional[Dict[str, torch.Tensor]]] = [None] * B
    with torch.cuda.device(dev):
        guard = OverflowGuard(scene, len(groups))
        for gi, (v0, nv) in enumerate(groups):
            o, d = ops.generate_rays_views(c2ws[v0:v0 + nv], fxs[v0:v0 + nv], fys[v0:v0 + nv], cxs[v0:v0 + nv], cys[v0:v0 + nv],
                                           H, W, dev, distortions=None if dists is None else dists[v0:v0 + nv],
                                           camera_type=types[0])
            views = ops.RayViews(nv, total, None if seeds is None else tuple(int(x) for x in seeds[v0:v0 + nv]))
            kw = shade_kw
            if laplace:
                kw = dict(shade_kw, lap_views=ops.LaplaceViews(
                    None if lap_view_sets is None else tuple(int(x) for x in lap_view_sets[v0:v0 + nv]),
                    None if depth_seeds is None else tuple(int(x) for x in depth_seeds[v0:v0 + nv])))
            res = render_rays(scene, o, d, ray_offset=0, clip=clip[v0 * cpv:(v0 + nv) * cpv], image_width=W,
                              init_bins=crop_bins(scene, o, d, obb), nonfinite_flag=guard.flag(gi), views=views, **kw)
            # one contiguous [nv,H,W,C] image stack per key (render_camera's torch.cat), handed out view by view
            stacks = {k: t.reshape(nv, H, W, -1).contiguous() for k, t in res.items()}
            for i in range(nv):
                outs[v0 + i] = {k: t[i] for k, t in stacks.items()}
        for gi in guard.offenders():
            v0, nv = groups[gi]
            for v in range(v0, v0 + nv):
                outs[v] = single(v)
            guard.rerendered.append(gi)
    return outs


_STREAMS: Dict[int, Tuple["torch.cuda.Stream", "torch.cuda.Stream"]] = {}


def _streams(dev):
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx not in _STREAMS:
        _STREAMS[idx] = (torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev))
    return _STREAMS[idx]
