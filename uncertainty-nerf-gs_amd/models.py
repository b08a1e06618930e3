"""Host-side Model mirrors: same class names, config fields, public methods and output-dict keys
as the reference's models; every pixel is produced by the HIP kernels through `render.py` /
`splat.py`.  Eval / inference only (the reference's loss and densification code is training-side
and out of scope).

  ActiveNerfactoModel      models/activenerfacto/activenerfacto_model.py:50-152
  NerfactoMCDropoutModel   models/mcdropout/mcdropout_models.py:51-131
  NerfactoLaplaceModel     models/laplace/laplace_model.py:156-556 (get_outputs_for_camera_unc :403-415)
  ActiveSplatfactoModel    models/activesplatfacto/activesplatfacto_model.py:49-367

nerfstudio is optional: a `Camera` here is any object with `camera_to_worlds` ([3,4] or [1,3,4]),
`fx, fy, cx, cy, height, width` (python numbers or 1-element tensors) -- a nerfstudio `Cameras` of
length 1 satisfies this.
"""
from __future__ import annotations

import re
from dataclasses import dataclass, field
from typing import Any, Dict, List, NamedTuple, Optional, Tuple, Type

import torch
from torch import nn

from . import fields as F
from . import lib as _lib
from . import ops, render, splat
from .render import NerfSceneDev


@dataclass
class Camera:
    camera_to_worlds: torch.Tensor
    fx: float
    fy: float
    cx: float
    cy: float
    height: int
    width: int


def _scalar(v) -> float:
    return float(v.reshape(-1)[0].item()) if torch.is_tensor(v) else float(v)


def _pose_target(what: str, image, channels):
    """the observed image of get_pose_information_for_camera -> [H,W,C] in ops.POSE_CHANNELS order of `channels`: [H,W,C] as it
    is, [H,W,3] with its r / g / b columns picked; None stays None"""
    if image is None:
        return None
    image = torch.as_tensor(image)
    rows = [k for k, n in enumerate(ops.POSE_CHANNELS) if n in ([channels] if isinstance(channels, str) else list(channels))]
    if image.dim() != 3 or image.shape[-1] not in (len(rows), 3):
        raise ValueError(f"{what}: image must be [H,W,3] or [H,W,{len(rows)}] (one column per channel), got {tuple(image.shape)}")
    if image.shape[-1] == len(rows):
        return image
    if any(k > 2 for k in rows):
        raise ValueError(f"{what}: an [H,W,3] image has no column for {[ops.POSE_CHANNELS[k] for k in rows if k > 2]}")
    return image[..., rows]


def _with_pose_step(out: Dict[str, Any], has_image: bool) -> Dict[str, Any]:
    """adds "step" = posegrad.pose_step(information, gradient)[0] where an image was given"""
    if has_image:
        from . import posegrad
        out["step"] = posegrad.pose_step(out["information"], out["gradient"])[0]
    return out


def _camera_args(camera, lens: bool = True) -> Tuple[torch.Tensor, Dict[str, Any]]:
    """[UPSTREAM Cameras.generate_rays] is restated (unerf_generate_rays) for ONE camera of type PERSPECTIVE, FISHEYE,
    EQUIRECTANGULAR or ORTHOPHOTO (what CAMERA_MODEL_TO_TYPE maps a transforms.json camera_model to, as the reference's
    parsers pass it on: dataparsers/sparse_mipnerf360/sparse_mipnerf360_dataparser.py:237-239), with the OPENCV lens
    parameters `distortion_params` = (k1, k2, k3, k4, p1, p2) the dataparsers attach to it (:248-274: every
    `ns-process-data images` scene) -- one eval image at a time is what the reference's eval loops hand over.  Anything
    else a nerfstudio `Cameras` can describe (omnidirectional stereo, VR180, FISHEYE624, camera batches) would silently
    render the wrong rays, so it is refused here.  lens=False (the splat models): perspective only -- gsplat's projection
    is a pinhole -- and the lens parameters are not looked at, as upstream Splatfacto.get_outputs never reads them (its
    datamanager undistorts the images instead)."""
    c2w = camera.camera_to_worlds
    if c2w.dim() == 3 and c2w.shape[0] != 1:
        raise ValueError(f"get_outputs_for_camera takes one camera, got a batch of {c2w.shape[0]}")
    ctype = getattr(camera, "camera_type", None)
    if ctype is not None:
        v = int(torch.as_tensor(ctype).reshape(-1)[0]) if torch.is_tensor(ctype) else int(getattr(ctype, "value", ctype))
        if v not in (_lib.CAMERA_TYPES if lens else (_lib.CAMERA_PERSPECTIVE,)):
            raise NotImplementedError(f"camera_type {v}: " + ("the ray kernel restates PERSPECTIVE 1, FISHEYE 2, EQUIRECTANGULAR 3 "
                                      "and ORTHOPHOTO 8" if lens else "the splat models project through a pinhole (PERSPECTIVE 1) only"))
    else:
        v = _lib.CAMERA_PERSPECTIVE
    c2w = c2w[0] if c2w.dim() == 3 else c2w
    args = dict(fx=_scalar(camera.fx), fy=_scalar(camera.fy), cx=_scalar(camera.cx), cy=_scalar(camera.cy),
                H=int(_scalar(camera.height)), W=int(_scalar(camera.width)))
    if v != _lib.CAMERA_PERSPECTIVE:
        args["camera_type"] = v
    dist_params = getattr(camera, "distortion_params", None) if lens else None
    if dist_params is not None:
        dp = torch.as_tensor(dist_params).detach().cpu().to(torch.float32).reshape(-1)
        if dp.numel() != 6:
            raise ValueError(f"distortion_params: expected 6 values (k1, k2, k3, k4, p1, p2), got {dp.numel()}")
        if bool((dp != 0).any()):
            args["distortion"] = [float(v) for v in dp]
    return c2w[:3, :4], args


def _camera_batch(cameras) -> Tuple[torch.Tensor, int, int, List[Any]]:
    """A batch of cameras of ONE image size (get_outputs_for_cameras: camera_to_worlds [B,3|4,4]; fx, fy, cx, cy,
    camera_type, distortion_params one value or one per camera) -> (c2w [B,3,4], H, W, one single-camera object per view
    that _camera_args reads like a nerfstudio camera)."""
    from types import SimpleNamespace
    c2w = torch.as_tensor(cameras.camera_to_worlds)
    c2w = c2w[None] if c2w.dim() == 2 else c2w
    B = c2w.shape[0]
    per = lambda v: torch.as_tensor(v).detach().cpu().reshape(-1).expand(B)
    sizes = {(int(h), int(w)) for h, w in zip(per(cameras.height).tolist(), per(cameras.width).tolist())}
    if len(sizes) != 1:
        raise ValueError(f"get_outputs_for_cameras renders one image size per batch, got {sorted(sizes)} (H, W)")
    (H, W), = sizes
    intr = {k: per(getattr(cameras, k)) for k in ("fx", "fy", "cx", "cy")}
    ctype = getattr(cameras, "camera_type", None)
    if ctype is not None:
        ctype = per(ctype) if torch.is_tensor(ctype) else per(int(getattr(ctype, "value", ctype)))
    dist = getattr(cameras, "distortion_params", None)
    if dist is not None:
        dist = torch.as_tensor(dist).detach().cpu().to(torch.float32)
        if dist.numel() not in (6, 6 * B):
            raise ValueError(f"distortion_params: expected 6 values (k1, k2, k3, k4, p1, p2) or one row of 6 per camera, got {tuple(dist.shape)}")
        dist = dist.reshape(-1, 6).expand(B, 6)
    singles = []
    for v in range(B):
        cam = SimpleNamespace(camera_to_worlds=c2w[v, :3, :4], height=H, width=W, **{k: intr[k][v] for k in intr})
        if ctype is not None:
            cam.camera_type = ctype[v]
        if dist is not None:
            cam.distortion_params = dist[v]
        singles.append(cam)
    return c2w[:, :3, :4], H, W, singles


def _splat_camera_batch(cameras, max_views: int, what: str):
    """The camera checks of the splat models' *_for_cameras methods, before anything touches the GPU: camera_to_worlds
    [B,3|4,4], PERSPECTIVE only, one image size, fx / fy / cx / cy one value or one per camera, max_views within a batch
    -> (c2w [B,...], B, H, W, {fx, fy, cx, cy: float64 [B]})."""
    c2w = torch.as_tensor(cameras.camera_to_worlds)
    c2w = c2w[None] if c2w.dim() == 2 else c2w
    B = c2w.shape[0]
    if not 1 <= max_views <= _lib.SPLAT_MAX_VIEWS:
        raise ValueError(f"max_views={max_views}: a batch holds 1 to {_lib.SPLAT_MAX_VIEWS} cameras")
    ctype = getattr(cameras, "camera_type", None)
    if ctype is not None:
        types = ({int(v) for v in torch.as_tensor(ctype).reshape(-1)} if torch.is_tensor(ctype)
                 else {int(getattr(ctype, "value", ctype))})
        bad = sorted(types - {_lib.CAMERA_PERSPECTIVE})
        if bad:
            raise NotImplementedError(f"camera_type {bad[0]}: the splat models project through a pinhole (PERSPECTIVE 1) only")
    sizes = {(int(h), int(w)) for h, w in zip(torch.as_tensor(cameras.height).reshape(-1).expand(B).tolist(),
                                              torch.as_tensor(cameras.width).reshape(-1).expand(B).tolist())}
    if len(sizes) != 1:
        raise ValueError(f"{what} renders one image size per batch, got {sorted(sizes)} (H, W)")
    (H, W), = sizes
    intr = {k: torch.as_tensor(getattr(cameras, k)).detach().to("cpu", torch.float64).reshape(-1).expand(B)
            for k in ("fx", "fy", "cx", "cy")}
    return c2w, B, H, W, intr


# ------------------------------------------------------------------ configs ----------------

@dataclass
class NerfactoModelConfig:
    """The nerfstudio 1.1.0 NerfactoModelConfig fields that shape eval rendering."""
    near_plane: float = 0.05
    far_plane: float = 1000.0
    background_color: str = "last_sample"
    hidden_dim: int = 64
    hidden_dim_color: int = 64
    num_levels: int = 16
    base_res: int = 16
    max_res: int = 2048
    log2_hashmap_size: int = 19
    features_per_level: int = 2
    num_proposal_samples_per_ray: Tuple[int, ...] = (256, 96)
    num_nerf_samples_per_ray: int = 48
    num_proposal_iterations: int = 2
    proposal_net_args_list: List[Dict] = field(default_factory=lambda: [
        {"hidden_dim": 16, "log2_hashmap_size": 17, "num_levels": 5, "max_res": 128, "use_linear": False},
        {"hidden_dim": 16, "log2_hashmap_size": 17, "num_levels": 5, "max_res": 256, "use_linear": False}])
    use_average_appearance_embedding: bool = True
    appearance_embed_dim: int = 32
    average_init_density: float = 1.0
    eval_num_rays_per_chunk: int = 1 << 15
    implementation: str = "torch"
    disable_scene_contraction: bool = False
    predict_normals: bool = False
    # "piecewise": UniformLinDispPiecewiseSampler; "uniform": UniformSampler (the reference's few-view runs,
    # /root/reference/README.md:153) [UPSTREAM NerfactoModel.populate_modules]
    proposal_initial_sampler: str = "piecewise"


@dataclass
class PlainNerfactoModelConfig(NerfactoModelConfig):
    """upstream `nerfacto` itself: the member type of the reference's NeRF ensembles (README.md:106-108,
    ensemble_utils.py:149-156)"""
    _target: Type = field(default_factory=lambda: NerfactoModel)


@dataclass
class ActiveNerfactoModelConfig(NerfactoModelConfig):
    _target: Type = field(default_factory=lambda: ActiveNerfactoModel)
    beta_min: float = 0.01
    density_loss_mult: float = 0.01
    rendered_uncertainty_eps: float = 1e-6


@dataclass
class NerfactoMCDropoutModelConfig(NerfactoModelConfig):
    _target: Type = field(default_factory=lambda: NerfactoMCDropoutModel)
    dropout_rate: float = 0.2
    rgb_dropout_layers: List[int] = field(default_factory=lambda: [-1])
    density_dropout_layers: bool = True
    mc_samples: int = 10


@dataclass
class NerfactoLaplaceModelConfig(NerfactoModelConfig):
    _target: Type = field(default_factory=lambda: NerfactoLaplaceModel)
    density_activation: str = "trunc_exp"


@dataclass
class SplatfactoModelConfig:
    """[UPSTREAM nerfstudio 1.1.0 SplatfactoModelConfig] the fields that shape eval rendering"""
    _target: Type = field(default_factory=lambda: SplatfactoModel)
    sh_degree: int = 3
    sh_degree_interval: int = 1000
    rasterize_mode: str = "classic"
    background_color: str = "random"


@dataclass
class ActiveSplatfactoModelConfig(SplatfactoModelConfig):
    _target: Type = field(default_factory=lambda: ActiveSplatfactoModel)
    beta_min: float = 0.01
    opacity_loss_mult: float = 0.01
    rendered_uncertainty_eps: float = 1e-6


# ------------------------------------------------------------------ checkpoints ---------------

MODEL_KEY_PREFIXES = ("field.", "proposal_networks.", "gauss_params.")


class IncompatibleKeys(NamedTuple):
    """what load_state_dict returns: `missing_keys` is always empty on return (a model parameter the checkpoint does
    not cover raises instead); `unexpected_keys` are the checkpoint's model keys (field.* / proposal_networks.* /
    gauss_params.*) this build has no use for; `loaded` / `expected` count distinct tensors."""
    missing_keys: List[str]
    unexpected_keys: List[str]
    loaded: int
    expected: int


def strip_pipeline_prefixes(state_dict) -> Dict[str, torch.Tensor]:
    """nerfstudio pipeline keys carry `_model.` (and, from a DDP run, `module.`): ensemble_pipeline.py:77-91, :134-137"""
    out = {}
    for k, v in state_dict.items():
        k = k[len("_model."):] if k.startswith("_model.") else k
        k = k[len("module."):] if k.startswith("module.") else k
        out[k] = v
    return out


def remap_checkpoint_keys(model: nn.Module, sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Checkpoint key layouts of the upstream modules the mirrors stand for -> the mirrors' own names.
    For every MLPWithHashEncoding `n` of the model (`field.mlp_base`, `proposal_networks.i.mlp_base`):
      * tcnn, fused: `n.model.params` (upstream attribute name; `n.tcnn_encoding.params` is accepted too) holds ONE
        tcnn.NetworkWithInputEncoding vector = FullyFusedMLP weights, then HashGrid parameters [UPSTREAM-RECALL
        tiny-cuda-nn NetworkWithInputEncoding::set_params_impl]; split by size into `n.mlp.tcnn_encoding.params` /
        `n.encoder.tcnn_encoding.params`;
      * the older layout (HashEncoding + MLP in an nn.Sequential, what this reference's own fields still build,
        activenerfacto_field.py:140-157): `P.encoding.*` / `n.0.*` -> `n.encoder.*`, `n.1.*` -> `n.mlp.*`
        (P = the field that owns `n`)."""
    from .fields import MLPWithHashEncoding
    out = dict(sd)
    for name, mod in model.named_modules():
        if not isinstance(mod, MLPWithHashEncoding):
            continue
        parent = name.rsplit(".", 1)[0] + "." if "." in name else ""
        for fused in (f"{name}.model.params", f"{name}.tcnn_encoding.params"):
            if fused in out and mod.implementation == "tcnn":
                vec = out.pop(fused)
                n_mlp, n_grid = mod.fused_tcnn_sizes()
                if vec.numel() != n_mlp + n_grid:
                    raise RuntimeError(f"{fused}: {vec.numel()} values, expected {n_mlp} (FullyFusedMLP) + {n_grid} "
                                       f"(HashGrid) = {n_mlp + n_grid} for this configuration")
                out[f"{name}.mlp.tcnn_encoding.params"] = vec[:n_mlp]
                out[f"{name}.encoder.tcnn_encoding.params"] = vec[n_mlp:]
        # alias rules apply to the exact leaves these modules own -- `hash_table`, `tcnn_encoding.params`,
        # `layers.N.weight|bias` -- and an alias that arrives NEXT TO its canonical key must carry the same tensor:
        # dropping one of two different tensors silently would hide a mixed-up checkpoint
        leaf = re.compile(r"^(hash_table|tcnn_encoding\.params|layers\.\d+\.(weight|bias))$")
        for k in list(out):
            for old, new in ((f"{parent}encoding.", f"{name}.encoder."), (f"{name}.0.", f"{name}.encoder."),
                             (f"{name}.1.", f"{name}.mlp.")):
                if k.startswith(old) and leaf.match(k[len(old):]):
                    canon = new + k[len(old):]
                    if canon in out and canon != k:
                        a, b = out[canon], out[k]
                        if not (torch.is_tensor(a) and torch.is_tensor(b) and a.shape == b.shape and torch.equal(a, b)):
                            raise RuntimeError(f"checkpoint carries both {k} and {canon} with different contents: "
                                               "cannot tell which one this model should load")
                    else:
                        out[canon] = out[k]
                    del out[k]
                    break
    return out


def load_checked(model: nn.Module, state_dict, strict: bool = False) -> IncompatibleKeys:
    """nn.Module.load_state_dict for the mirrors, with the silent cases closed (VERDICT r2 / ADVICE r2):
    every PARAMETER of the model must be covered by the checkpoint after alias mapping (under any of the names it is
    registered as) -- otherwise RuntimeError, naming what is missing: a checkpoint of another implementation (tcnn vs
    torch), another method or another layout must not "load" and then render from random weights.  Buffers
    (aabb, max_res, ...) are loaded when present.  Checkpoint keys under field. / proposal_networks. / gauss_params.
    that the model does not own are returned as unexpected_keys (strict=True: RuntimeError, which is what nerfstudio's
    pipeline catches before retrying with strict=False)."""
    sd = remap_checkpoint_keys(model, strip_pipeline_prefixes(state_dict))
    own = model.state_dict()
    by_ptr: Dict[int, List[str]] = {}      # one entry per distinct parameter, with every name it is registered as
    for n, p in model.named_parameters(remove_duplicate=False):
        by_ptr.setdefault(id(p), []).append(n)
    missing = [names[0] for names in by_ptr.values() if not any(n in sd for n in names)]
    if missing:
        have = sorted(k for k in sd if k.startswith(MODEL_KEY_PREFIXES))
        raise RuntimeError(
            f"{type(model).__name__}.load_state_dict: {len(missing)} of {len(by_ptr)} parameters are not in the checkpoint "
            f"(first: {missing[:6]}); it carries {len(have)} model keys (first: {have[:6]}).  A checkpoint of another "
            "implementation (tcnn / torch), method or key layout does not load into this model")
    for n, p in model.named_parameters(remove_duplicate=False):    # shapes: fail with the key name, before any copy
        if n in sd and tuple(sd[n].shape) != tuple(p.shape):
            raise RuntimeError(f"{type(model).__name__}.load_state_dict: {n} has shape {tuple(sd[n].shape)} in the checkpoint, "
                               f"{tuple(p.shape)} in the model (config mismatch: hash-map size, levels, widths?)")
    unexpected = sorted(k for k, v in sd.items()
                        if k.startswith(MODEL_KEY_PREFIXES) and k not in own and (not torch.is_tensor(v) or v.numel() > 0))
    if strict and unexpected:
        raise RuntimeError(f"{type(model).__name__}.load_state_dict(strict=True): unexpected keys {unexpected[:8]}"
                           + (f" (+{len(unexpected) - 8} more)" if len(unexpected) > 8 else ""))
    nn.Module.load_state_dict(model, {k: v for k, v in sd.items() if k in own}, strict=False)
    if unexpected:
        import warnings
        warnings.warn(f"{type(model).__name__}.load_state_dict: ignored checkpoint keys {unexpected[:8]}"
                      + (f" (+{len(unexpected) - 8} more)" if len(unexpected) > 8 else ""))
    return IncompatibleKeys([], unexpected, len(by_ptr), len(by_ptr))


# ------------------------------------------------------------------ NeRF models --------------


class _ImageMetrics:
    """`model.psnr(image, rgb)` / `model.ssim(image, rgb)` / `model.lpips(image, rgb)` on [1,3,H,W] images, as the eval
    script calls them (scripts/eval_uncertainty.py:683-689; nerfstudio sets them to torchmetrics' PSNR(data_range=1.0),
    SSIM and LearnedPerceptualImagePatchSimilarity(normalize=True)).  `lpips` needs the network's weights: a checkpoint
    that carries `lpips.net.*` supplies them at load_state_dict (checkpoints.lpips_weights_from_state_dict), or
    set_lpips_weights by hand; `lpips_weights` is a plain attribute, neither parameter nor buffer."""
    lpips_weights = None

    @staticmethod
    def psnr(image: torch.Tensor, rgb: torch.Tensor) -> torch.Tensor:
        from . import metrics
        return torch.tensor(metrics.psnr(rgb, image), dtype=torch.float64)

    @staticmethod
    def ssim(image: torch.Tensor, rgb: torch.Tensor) -> torch.Tensor:
        from . import metrics
        return torch.tensor(metrics.ssim(rgb, image), dtype=torch.float64)

    def set_lpips_weights(self, weights) -> None:
        """weights: a checkpoints.LpipsWeights (or None to drop them)"""
        object.__setattr__(self, "lpips_weights", weights)

    def _adopt_lpips_weights(self, state_dict) -> None:
        from .checkpoints import lpips_weights_from_state_dict
        self.set_lpips_weights(lpips_weights_from_state_dict(state_dict))

    def lpips(self, image: torch.Tensor, rgb: torch.Tensor) -> torch.Tensor:
        """[1,3,H,W] (or [B,3,H,W]) images in [0, 1] -> the 0-d float64 LPIPS (metrics.lpips, the host definition)"""
        if self.lpips_weights is None:
            raise NotImplementedError("LPIPS needs the AlexNet weights: load a checkpoint that carries `lpips.net.*` keys "
                                      "(every nerfstudio checkpoint does) or call set_lpips_weights")
        from . import metrics
        return torch.tensor(metrics.lpips(rgb.permute(0, 2, 3, 1), image.permute(0, 2, 3, 1), self.lpips_weights),
                            dtype=torch.float64)


class _NerfactoBase(nn.Module, _ImageMetrics):
    config: NerfactoModelConfig
    # Arithmetic of the main field's dense layers (ops.FieldDev.precision).  None = what the REFERENCE computes this model
    # in at eval (reference_precision()); "f16x2" (fp32-equivalent), "f16" or "fp32" force one form.
    precision: Optional[str] = None

    def __init__(self, config, scene_box=None, num_train_data: int = 1, **_kw):
        super().__init__()
        self.config = config
        self.scene_box = scene_box
        self.num_train_data = num_train_data
        self._dev_scene: Optional[NerfSceneDev] = None
        self.rays_per_launch = 1 << 20
        self.populate_modules()

    # -- construction -------------------------------------------------------------------------
    def _field_kwargs(self):
        c = self.config
        return dict(num_images=self.num_train_data, hidden_dim=c.hidden_dim, num_levels=c.num_levels, max_res=c.max_res,
                    base_res=c.base_res, features_per_level=c.features_per_level,
                    log2_hashmap_size=c.log2_hashmap_size, hidden_dim_color=c.hidden_dim_color,
                    use_average_appearance_embedding=c.use_average_appearance_embedding,
                    appearance_embedding_dim=c.appearance_embed_dim, implementation=c.implementation)

    def populate_modules(self):
        c = self.config
        assert c.num_proposal_iterations == 2 and len(c.proposal_net_args_list) == 2
        self.proposal_networks = nn.ModuleList([
            F.HashMLPDensityField(hidden_dim=a["hidden_dim"], num_levels=a["num_levels"], max_res=a["max_res"],
                                  log2_hashmap_size=a["log2_hashmap_size"],
                                  average_init_density=c.average_init_density, use_linear=bool(a.get("use_linear", False)),
                                  implementation=c.implementation) for a in c.proposal_net_args_list])
        self.field = self._make_field()

    def _make_field(self):
        raise NotImplementedError

    # -- checkpoints --------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict: bool = False, **kw):  # type: ignore[override]
        """Accepts nerfstudio checkpoints: `pipeline` keys carry a `_model.` (and, under DDP, `module.`) prefix
        (ensemble_pipeline.py:77-91); upstream's MLPWithHashEncoding layouts (torch and fused tcnn) and the older
        HashEncoding + Sequential layout load alike (remap_checkpoint_keys).  Non-model keys (camera optimizer, lpips,
        datamanager) are ignored; a model parameter the checkpoint does not cover raises (load_checked)."""
        self._dev_scene = None
        for m in self.modules():
            if hasattr(m, "invalidate") and m is not self:
                m.invalidate()
        report = load_checked(self, state_dict, strict=strict)
        self._adopt_lpips_weights(state_dict)
        return report

    # -- lowering to the device ---------------------------------------------------------------
    def _field_to_device(self, device):
        return self.field.to_device(device)

    def _sampler_opts(self) -> Dict[str, Any]:
        """config.proposal_initial_sampler / config.background_color -> the kernels' spacing and background modes"""
        c = self.config
        if c.proposal_initial_sampler not in ("piecewise", "uniform"):
            raise ValueError(f"proposal_initial_sampler={c.proposal_initial_sampler!r}: expected 'piecewise' or 'uniform'")
        from . import lib as _lib
        return dict(spacing=_lib.SPACING_UNIFORM if c.proposal_initial_sampler == "uniform" else _lib.SPACING_PIECEWISE,
                    background=ops.background_of(c.background_color))

    def reference_precision(self) -> str:
        """The arithmetic the reference runs this model's Linear layers in at eval: tiny-cuda-nn FullyFusedMLPs (fp16
        weights and activations) when config.implementation == "tcnn" -- upstream's default, handed to the field at
        activenerfacto_model.py:77 -- and torch fp32 Linears otherwise.  -> "f16" (one f16 product per MAC, fp32
        accumulate: no narrower than tcnn) | "f16x2" (fp32-equivalent)."""
        return "f16" if self.config.implementation == "tcnn" else "f16x2"

    def device_scene(self, device=None) -> NerfSceneDev:
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self._dev_scene is None or self._dev_scene.device != device:
            fd = self._field_to_device(device)
            want = self.precision or self.reference_precision()
            if want == "f16" and (fd.mfma16_blob is None or not fd.use_mfma):
                want = "fp32"       # weights beyond the f16 range (or a VALU-only layout): the exact kernels
            fd.precision = want
            self._dev_scene = self._build_scene(device, fd)
            kept = getattr(self, "_kept_workspace", None)
            if kept is not None and self._dev_scene.workspace is not None:
                self._dev_scene.workspace = kept     # the scratch arena survives a rebuild of the parameter copies
            self._kept_workspace = None
        return self._dev_scene

    def _build_scene(self, device, fd) -> NerfSceneDev:
        c = self.config
        props = [p.to_device(device) for p in self.proposal_networks]
        if c.disable_scene_contraction:
            # mcdropout_models.py:60-63 / activenerfacto_model.py:57-60: spatial_distortion = None -> every network
            # normalises positions with SceneBox.get_normalized_positions(positions, self.scene_box.aabb)
            if self.scene_box is None or getattr(self.scene_box, "aabb", None) is None:
                raise ValueError("disable_scene_contraction needs scene_box.aabb ([2,3])")
            box = tuple(float(v) for v in torch.as_tensor(self.scene_box.aabb).reshape(-1))
            fd.aabb = box
            for p in props:
                p.aabb = box
        return NerfSceneDev(
            field=fd, props=props,
            near=c.near_plane, far=c.far_plane, num_prop=tuple(c.num_proposal_samples_per_ray),
            num_nerf=c.num_nerf_samples_per_ray, prop_average_init_density=c.average_init_density,
            chunk_rays=c.eval_num_rays_per_chunk, **self._sampler_opts())

    def invalidate(self):
        """call after changing weights or eval-time knobs (mc_samples, GGN, ...).  The device copies of the parameters are
        rebuilt on the next render; the frame path's scratch arena (ops.Workspace, GBs at 1080p) is carried over -- a
        Laplace *_unc call invalidates twice per frame.  release() drops it too."""
        if self._dev_scene is not None and self._dev_scene.workspace is not None:
            self._kept_workspace = self._dev_scene.workspace
        self._dev_scene = None

    def release(self):
        """free the device copies AND the scratch arena (a model that will not render again soon)"""
        for ws in (getattr(self, "_kept_workspace", None), None if self._dev_scene is None else self._dev_scene.workspace):
            if ws is not None:
                ws.release()
        self._kept_workspace = None
        self._dev_scene = None

    def _begin_render(self, scene: NerfSceneDev, total_rays: int = 0, chunk_rays: int = 0) -> None:
        """once per get_outputs_for_camera / get_outputs_for_camera_ray_bundle / get_outputs call: the rays of the frame
        and the rays per reference eval chunk (the whole bundle for get_outputs)"""

    # -- rendering ----------------------------------------------------------------------------
    def _render_kwargs(self) -> Dict[str, Any]:
        return {}

    @torch.no_grad()
    def get_outputs_for_camera(self, camera, obb_box=None) -> Dict[str, torch.Tensor]:
        """[UPSTREAM Model.get_outputs_for_camera] camera.generate_rays(camera_indices=0, keep_shape=True,
        obb_box=obb_box) + the chunked render.  obb_box: anything with `.R` [3,3], `.T` [3], `.S` [3] (nerfstudio's
        OrientedBox); rays get their planes from the box (render.crop_bins), rays that miss it render empty."""
        c2w, cam = _camera_args(camera)
        obb = None if obb_box is None else (ops.world_to_box(obb_box.R, obb_box.T), torch.as_tensor(obb_box.S).detach().cpu())
        scene = self.device_scene()
        self._begin_render(scene, int(cam["H"]) * int(cam["W"]), scene.chunk_rays)
        return render.render_camera(scene, c2w, rays_per_launch=self.rays_per_launch, obb=obb,
                                    **cam, **self._render_kwargs())

    # one sentence saying why this model has no pose gradient (None: it has one)
    _no_pose_gradient: Optional[str] = "this model does not define the rendered colour as one deterministic field evaluation."

    @torch.no_grad()
    def get_pose_gradients_for_camera(self, camera, rays_per_launch: Optional[int] = None, want_rgb: bool = False):
        """d mean_c(rgb[y, x]) / d camera_to_worlds for every pixel of one camera -> [H,W,3,4] float32 on the device (with
        want_rgb also the colour the gradient kernel composited, [H,W,3]): what the reference's
        estimate_gradient_pose_6dof.py:128-139 collects with one autograd backward per pixel, from
        render.pose_gradient_camera (sample bins held fixed, fp32 arithmetic whatever precision the frames render in)."""
        if self._no_pose_gradient is not None:
            raise NotImplementedError(f"{type(self).__name__}.get_pose_gradients_for_camera: {self._no_pose_gradient}")
        c2w, cam = _camera_args(camera)
        scene = self.device_scene()
        return render.pose_gradient_camera(scene, c2w, rays_per_launch=rays_per_launch or self.rays_per_launch,
                                           want_rgb=want_rgb, **cam)

    def _require_pose_jacobian(self, what: str) -> None:
        if self._no_pose_gradient is not None:
            raise NotImplementedError(f"{type(self).__name__}.{what}: pose Jacobians are not built for this model (the "
                                      "Jacobian kernel differentiates one deterministic nerfacto / active-nerfacto field).")

    @torch.no_grad()
    def get_pose_jacobians_for_camera(self, camera, channels=ops.POSE_CHANNELS, basis: str = "se3",
                                      rays_per_launch: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """The per-pixel Jacobian of the rendered channels with respect to the camera pose ->
        {"jacobian": [H,W,C,6 | 12], "values": [H,W,C]} float32 on the device; the C rows in ops.POSE_CHANNELS order
        (r, g, b, accumulation, expected_depth).  basis "se3": the six parameters of posegrad.POSE_PARAMS (tx .. angz of
        c2w . exp(xi), the camera's own frame; contracted in the kernel with posegrad.tangent_basis); "c2w": the twelve
        entries of camera_to_worlds, row-major 3x4.  r / g / b follow get_pose_gradients_for_camera's rules (their mean over
        the channels is its quantity).  expected_depth is the UNCLIPPED quotient sum w t / (sum w + 1e-10): the clip of the
        rendered expected depth to the ray's step range is not applied and not differentiated (it is the identity except
        where the accumulation is of the order of 1e-10).  Sample bins held fixed, fp32."""
        self._require_pose_jacobian("get_pose_jacobians_for_camera")
        if basis not in ("se3", "c2w"):
            raise ValueError(f"get_pose_jacobians_for_camera: basis={basis!r} (expected 'se3' or 'c2w')")
        from . import posegrad
        c2w, cam = _camera_args(camera)
        kw = dict(channels=channels, rays_per_launch=rays_per_launch or self.rays_per_launch, **cam)
        if basis == "se3":
            out = render.pose_jacobian_camera(self.device_scene(), c2w, proj=posegrad.pose_projection(c2w, None),
                                              want=("proj", "val"), **kw)
            return {"jacobian": out["proj"], "values": out["val"]}
        out = render.pose_jacobian_camera(self.device_scene(), c2w, want=("jac", "val"), **kw)
        return {"jacobian": out["jac"], "values": out["val"]}

    @torch.no_grad()
    def get_pose_information_for_camera(self, camera, image=None, weights=None, mask=None, channels=("r", "g", "b"),
                                        rays_per_launch: Optional[int] = None) -> Dict[str, Any]:
        """How well a frame determines the camera pose, and which pose step an observed image asks for: over the pixels and
        `channels` of the frame, in the six parameters of posegrad.POSE_PARAMS (c2w . exp(xi)),
          information [6,6] = sum w J J^T (the Fisher information; Gauss-Newton matrix),  gradient [6] = sum w J r,
          chi2 = sum w r^2 with r = rendered - image,  n_used / n_skipped (terms with a non-finite input or w < 0 are skipped),
          covariance [6,6] = the pseudo-inverse of the information (posegrad.pose_covariance: a Laplace approximation of the
          pose posterior, a valid pose_cov of get_pose_uncertainty_for_camera), rank,
          and with an image: step [6] = posegrad.pose_step(information, gradient), to be applied with posegrad.apply_pose_step.
        All float64 host values.  The Jacobian is get_pose_jacobians_for_camera's (basis "se3"), but it is reduced per launch
        group on the device in float64 (render.pose_normal_eq_camera) and never held as a frame.
        image: [H,W,3], or [H,W,C] matching channels; None: the information alone (gradient and chi2 are exactly 0).
        weights: [H,W], [H,W,1] or [H,W,C]; the intended weight for ActiveNerfactoModel is 1 / rgb_std^2 of its own outputs.
        mask: [H,W], 0 = left out.  rays_per_launch: a multiple of lib.POSE_NEQ_TILE (default: the model's, rounded up to one);
        the result does not depend on it."""
        self._require_pose_jacobian("get_pose_information_for_camera")
        c2w, cam = _camera_args(camera)
        tile = _lib.POSE_NEQ_TILE
        rpl = int(rays_per_launch) if rays_per_launch else -(-int(self.rays_per_launch) // tile) * tile
        target = _pose_target("get_pose_information_for_camera", image, channels)
        out = render.pose_normal_eq_camera(self.device_scene(), c2w, target=target, weights=weights, mask=mask, channels=channels,
                                           rays_per_launch=rpl, **cam)
        return _with_pose_step(out, image is not None)

    @torch.no_grad()
    def get_pose_uncertainty_for_camera(self, camera, pose_cov, rays_per_launch: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """First-order propagation of a pose covariance to every pixel: var_c = J_c Sigma J_c^T per channel, from one kernel
        pass (posegrad.pose_projection(c2w, pose_cov) contracted and squared in the Jacobian kernel).  pose_cov: [6,6] in
        posegrad.POSE_PARAMS order (the camera's own frame), or a 6-vector of standard deviations.  -> [H,W,1] each:
          rgb_var_pose = mean_c var_c and rgb_std_pose = its root (the ensemble's convention, ensemble_pipeline.py:165-174),
          expected_depth_std_pose, accumulation_std_pose,
          and rgb [H,W,3], accumulation, expected_depth as the kernel composited them (expected_depth unclipped, see
          get_pose_jacobians_for_camera)."""
        self._require_pose_jacobian("get_pose_uncertainty_for_camera")
        if pose_cov is None:
            raise ValueError("get_pose_uncertainty_for_camera: pose_cov is needed ([6,6] or 6 standard deviations)")
        from . import posegrad
        c2w, cam = _camera_args(camera)
        out = render.pose_jacobian_camera(self.device_scene(), c2w, proj=posegrad.pose_projection(c2w, pose_cov),
                                          want=("var", "val"), rays_per_launch=rays_per_launch or self.rays_per_launch, **cam)
        var, val = out["var"], out["val"]
        rgb_var = var[..., :3].mean(dim=-1, keepdim=True)
        return {"rgb_var_pose": rgb_var, "rgb_std_pose": rgb_var.sqrt(),
                "accumulation_std_pose": var[..., 3:4].sqrt(), "expected_depth_std_pose": var[..., 4:5].sqrt(),
                "rgb": val[..., :3], "accumulation": val[..., 3:4], "expected_depth": val[..., 4:5]}

    def _begin_render_views(self, scene: NerfSceneDev, n_views: int) -> Tuple[bool, Optional[List[int]]]:
        """once per get_outputs_for_cameras call -> (render the batch through render.render_cameras, mask seed per view |
        None); False: the model renders its cameras one by one through get_outputs_for_camera"""
        return True, None

    @torch.no_grad()
    def get_outputs_for_cameras(self, cameras, obb_box=None, max_views: int = 16) -> List[Dict[str, torch.Tensor]]:
        """get_outputs_for_camera for every camera of a batch, with the argument conventions of
        SplatfactoModel.get_outputs_for_cameras: camera_to_worlds [B,3,4]; fx, fy, cx, cy, distortion_params (and
        camera_type) one value or one per camera; one image size, anything else raises ValueError.  Element v equals
        get_outputs_for_camera(camera v, obb_box) bit for bit, and the model is left as after B such calls.  Up to
        max_views (<= lib.NERF_MAX_VIEWS) small frames share one launch group (render.render_cameras, which also says when
        the batch is rendered camera by camera instead, with the same results)."""
        if not 1 <= max_views <= _lib.NERF_MAX_VIEWS:
            raise ValueError(f"max_views={max_views}: a launch group holds 1 to {_lib.NERF_MAX_VIEWS} cameras")
        c2w, H, W, singles = _camera_batch(cameras)
        args = [_camera_args(cam)[1] for cam in singles]              # validates every camera as get_outputs_for_camera does
        scene = self.device_scene()
        batched, seeds = self._begin_render_views(scene, len(singles))
        if not batched:
            return [self.get_outputs_for_camera(cam, obb_box) for cam in singles]
        obb = None if obb_box is None else (ops.world_to_box(obb_box.R, obb_box.T), torch.as_tensor(obb_box.S).detach().cpu())
        return render.render_cameras(scene, c2w, [a["fx"] for a in args], [a["fy"] for a in args], [a["cx"] for a in args],
                                     [a["cy"] for a in args], H, W, seeds=seeds, rays_per_launch=self.rays_per_launch, obb=obb,
                                     distortion=[a.get("distortion") for a in args],
                                     camera_type=[a.get("camera_type", _lib.CAMERA_PERSPECTIVE) for a in args],
                                     max_views=max_views, **self._render_kwargs())

    @torch.no_grad()
    def get_outputs_for_camera_ray_bundle(self, camera_ray_bundle, directions: Optional[torch.Tensor] = None):
        """Model.get_outputs_for_camera_ray_bundle(camera_ray_bundle: RayBundle) (mcdropout_models.py:94-96): any object
        with `.origins` / `.directions` [H,W,3] -- a nerfstudio RayBundle from `camera.generate_rays(keep_shape=True)` --
        or, for callers without nerfstudio, the two tensors (origins, directions).  A bundle that carries `nears` and
        `fars` (generate_rays with an obb_box) keeps them, as SceneCollider.forward does."""
        nears = fars = None
        if directions is None:
            origins, directions = camera_ray_bundle.origins, camera_ray_bundle.directions
            nears, fars = getattr(camera_ray_bundle, "nears", None), getattr(camera_ray_bundle, "fars", None)
        else:
            origins = camera_ray_bundle
        H, W = origins.shape[:2]
        scene0 = self.device_scene(origins.device if origins.is_cuda else None)
        origins = origins.to(device=scene0.device, dtype=torch.float32)
        directions = directions.to(device=scene0.device, dtype=torch.float32)
        scene = self.device_scene(origins.device)
        self._begin_render(scene, H * W, scene.chunk_rays)
        o, d = origins.reshape(-1, 3).contiguous(), directions.reshape(-1, 3).contiguous()
        init = None
        if nears is not None and fars is not None:
            init = render.crop_bins(scene, o, d, nears=nears.to(device=o.device, dtype=torch.float32).reshape(-1),
                                    fars=fars.to(device=o.device, dtype=torch.float32).reshape(-1))
        rpl = max(scene.chunk_rays, (self.rays_per_launch // scene.chunk_rays) * scene.chunk_rays)
        from .ops import new_clip_buffer
        clip = new_clip_buffer(H * W, scene.chunk_rays, o.device)
        lists: Dict[str, List[torch.Tensor]] = {}
        starts = list(range(0, H * W, rpl))
        guard = render.OverflowGuard(scene, len(starts))

        def group(gi, flag=None):
            s = starts[gi]
            return render.render_rays(scene, o[s:s + rpl], d[s:s + rpl], ray_offset=s, total_rays=H * W, clip=clip,
                                      image_width=W, init_bins=None if init is None else init[s:s + rpl],
                                      nonfinite_flag=flag, **self._render_kwargs())

        for gi in range(len(starts)):
            for k, v in group(gi, guard.flag(gi)).items():
                lists.setdefault(k, []).append(v)
        for gi in guard.offenders():    # f16 operand overflow: that group again on the exact-fp32 kernels
            for k, v in guard.redo(gi, lambda: group(gi)).items():
                lists[k][gi] = v
        return {k: torch.cat(v).view(H, W, -1) for k, v in lists.items()}


    @torch.no_grad()
    def get_outputs(self, ray_bundle) -> Dict[str, torch.Tensor]:
        """Model.get_outputs(ray_bundle) at eval (activenerfacto_model.py:83-152, mcdropout / laplace equivalents):
        a flat bundle of rays -- any object with `.origins` / `.directions` [R,3] (a nerfstudio RayBundle), or an
        (origins, directions) pair -- rendered as ONE reference chunk (the per-chunk expected-depth clip bounds are
        those of this bundle, as in the reference when `forward` is called on a chunk)."""
        nears = fars = None
        if isinstance(ray_bundle, (tuple, list)):
            o, d = ray_bundle
        else:
            o, d = ray_bundle.origins, ray_bundle.directions
            nears, fars = getattr(ray_bundle, "nears", None), getattr(ray_bundle, "fars", None)
        scene = self.device_scene(o.device if o.is_cuda else None)
        self._begin_render(scene, o.reshape(-1, 3).shape[0], max(o.reshape(-1, 3).shape[0], 1))
        o = o.reshape(-1, 3).to(device=scene.device, dtype=torch.float32).contiguous()
        d = d.reshape(-1, 3).to(device=scene.device, dtype=torch.float32).contiguous()
        init = None
        if nears is not None and fars is not None:   # planes already on the bundle: the collider leaves them
            init = render.crop_bins(scene, o, d, nears=nears.to(device=o.device, dtype=torch.float32).reshape(-1),
                                    fars=fars.to(device=o.device, dtype=torch.float32).reshape(-1))
        from .ops import new_clip_buffer
        R = o.shape[0]
        clip = new_clip_buffer(R, max(R, 1), o.device)                 # one chunk = the whole bundle
        saved, scene.chunk_rays = scene.chunk_rays, max(R, 1)
        guard = render.OverflowGuard(scene, 1)
        try:
            run = lambda flag=None: render.render_rays(scene, o, d, ray_offset=0, total_rays=R, clip=clip, init_bins=init,
                                                       nonfinite_flag=flag, **self._render_kwargs())
            out = run(guard.flag(0))
            return guard.redo(0, run) if guard.offenders() else out
        finally:
            scene.chunk_rays = saved

    def forward(self, ray_bundle) -> Dict[str, torch.Tensor]:  # type: ignore[override]
        """Model.forward: collider (near/far planes are the config's) + get_outputs"""
        return self.get_outputs(ray_bundle)


class NerfactoModel(_NerfactoBase):
    """[UPSTREAM nerfstudio 1.1.0 NerfactoModel] plain nerfacto: rgb, accumulation, depth, expected_depth, prop_depth_i.
    The member model of the reference's NeRF ensembles (ensemble_utils.py:149-150)."""
    config: PlainNerfactoModelConfig
    _no_pose_gradient = None

    def _make_field(self):
        return F.NerfactoField(average_init_density=self.config.average_init_density, **self._field_kwargs())


class ActiveNerfactoModel(_NerfactoBase):
    config: ActiveNerfactoModelConfig
    _no_pose_gradient = None

    def _make_field(self):
        return F.ActiveNerfactoField(beta_min=self.config.beta_min, **self._field_kwargs())

    def _render_kwargs(self):
        return {"keep_density": True}  # the reference returns the raw [H,W,48] density too (:115,:122)


def frame_seed(base_seed: int, frame: int) -> int:
    """Mask-stream seed of the `frame`-th render of a model: the reference draws fresh dropout masks in every forward
    (torch's global generator moves on, mcdropout_models.py:116-119), so two cameras never share their masks.  Frame 0
    uses the base seed itself; later frames a hash of (base seed, frame) -- the counter-RNG twin of "the generator has
    advanced" (same unerf_hash32 as the kernels' mask words)."""
    if frame == 0:
        return base_seed & 0xFFFFFFFF

    def h32(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x21F0AAAD) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x735A2D97) & 0xFFFFFFFF
        x ^= x >> 15
        return x

    return h32((base_seed & 0xFFFFFFFF) ^ h32(frame + 0x9E3779B9))


def iter_torch_keep_draws(K: int, total_rays: int, S: int, chunk_rays: int, drop_sites: int, p_drop: float,
                          generator: Optional[torch.Generator] = None, hidden: int = 64, hidden_color: int = 64):
    """The keep masks of one frame drawn as the reference's nn.Dropout modules draw them, IN THE ORDER its modules consume
    torch's generator (mcdropout_models.py:116-119): pass k outermost (the whole camera bundle is rendered per pass),
    inside it the chunks of `chunk_rays` rays in order, inside a chunk the active Dropout modules in forward order --
    trunk [chunk * S, hidden], then HEAD0, then HEAD1 [chunk * S, hidden_color] (the proposal networks hold none).
    nn.Dropout in train mode draws empty_like(x).bernoulli_(1 - p): with a CPU generator seeded s these are the masks the
    reference's modules make on the CPU after torch.manual_seed(s).  Runs on the generator's device (None: the CPU's
    global generator); no GPU needed.  Yields (k, first_ray, n_rays, site index 0 / 1 / 2, keep bool [n_rays * S, units])."""
    dev = torch.device("cpu") if generator is None else generator.device
    sites = drop_sites if drop_sites else (_lib.DROP_TRUNK | _lib.DROP_HEAD1)
    if sites & _lib.DROP_HEADIN:
        raise _lib.UnerfError("dropout_masks='torch': the DROP_HEADIN site has no explicit-mask mode")
    for k in range(K):
        for start in range(0, total_rays, chunk_rays):
            n = min(chunk_rays, total_rays - start)
            for i, units in enumerate((hidden, hidden_color, hidden_color)):
                if (sites >> i) & 1:
                    noise = torch.empty(n * S, units, dtype=torch.float32, device=dev).bernoulli_(1.0 - p_drop, generator=generator)
                    yield k, start, n, i, noise != 0


def torch_keep_mask_bytes(K: int, total_rays: int, S: int, drop_sites: int) -> int:
    """bytes of a frame's packed keep masks (64-unit sites: 8 bytes per pass, sample and site)"""
    sites = drop_sites if drop_sites else (_lib.DROP_TRUNK | _lib.DROP_HEAD1)
    return K * total_rays * S * 8 * bin(sites & 7).count("1")


def draw_torch_keep_masks(device, K: int, total_rays: int, S: int, chunk_rays: int, drop_sites: int, p_drop: float,
                          generator: Optional[torch.Generator] = None) -> ops.KeepMasks:
    """iter_torch_keep_draws packed chunk by chunk (ops.pack_keep_bits) into the frame-wide bit arrays of an
    ops.KeepMasks on `device` (row = ray * S + sample): the bytes of a draw never exist for more than one chunk."""
    sites = ops.FieldDev._sites(drop_sites)
    stride = total_rays * S
    bits = [torch.empty(K, stride, 2, dtype=torch.int32, device=device) if (sites >> i) & 1 else None for i in range(3)]
    for k, start, n, i, keep in iter_torch_keep_draws(K, total_rays, S, max(chunk_rays, 1), drop_sites, p_drop, generator):
        bits[i][k, start * S:(start + n) * S] = ops.pack_keep_bits(keep.to(device))
    return ops.KeepMasks(bits[0], bits[1], bits[2], None, stride, 0)


class NerfactoMCDropoutModel(_NerfactoBase):
    config: NerfactoMCDropoutModelConfig
    seed: int = 0                    # base seed of the dropout-mask stream
    frame_counter: int = 0           # renders made so far: every render draws fresh masks (frame_seed)
    fresh_masks_per_render: bool = True
    # "counter": the kernels' own counter generator (default).  "torch": every frame's masks are drawn with torch's
    # Bernoulli in the order the reference's Dropout modules consume the generator (iter_torch_keep_draws), packed to
    # bits and replayed through the explicit-mask kernels (unerf_field_fwd_masked).
    dropout_masks: str = "counter"
    mask_generator: Optional[torch.Generator] = None     # "torch": None = torch's global CPU generator
    mask_budget_bytes: int = 1 << 34                     # "torch": a frame whose packed masks need more raises (1080p, K = 8: 12.7 GB)
    _frame_masks: Optional[ops.KeepMasks] = None
    _no_pose_gradient = ("its colour is the mean of K passes under fresh dropout masks, and the gradient kernel "
                         "differentiates one deterministic pass; get_mc_pose_gradients_for_camera differentiates the frame "
                         "of a named mask draw.")

    @torch.no_grad()
    def get_mc_pose_gradients_for_camera(self, camera, mask_seed: Optional[int] = None, rays_per_launch: Optional[int] = None,
                                         want_rgb: bool = False):
        """d mean_c(rgb[y, x]) / d camera_to_worlds of the MC-dropout frame of ONE mask draw -> [H,W,3,4] float32 on the device
        (with want_rgb also the mean colour the gradient kernel composited, [H,W,3]): rgb is the mean of the K dropout passes,
        and under a fixed draw it is a deterministic function of the pose (render.pose_gradient_camera_mc; sample bins held
        fixed, fp32 arithmetic).  mask_seed None: the seed of this model's most recent render (the base seed before any
        render), so get_outputs_for_camera(cam) followed by this call differentiates the frame just rendered; an int: that
        seed of the counter generator.  frame_counter does not advance and scene.field.seed is left as found.
        dropout_masks = "torch": the masks of the most recent frame are replayed while the model still holds them."""
        c2w, cam = _camera_args(camera)
        scene = self.device_scene()
        kw = dict(rays_per_launch=rays_per_launch or self.rays_per_launch, want_rgb=want_rgb, **cam)
        if self.dropout_masks == "torch" and scene.field.K > 0 and scene.field.p_drop > 0.0:
            if mask_seed is not None:
                raise ValueError("get_mc_pose_gradients_for_camera: mask_seed names a draw of the counter generator; "
                                 "dropout_masks='torch' replays the masks of the most recent frame")
            if self._frame_masks is None:
                raise _lib.UnerfError("get_mc_pose_gradients_for_camera: the torch masks of that frame are gone (render the "
                                      "camera with get_outputs_for_camera first; a batched or later render drops them)")
            return render.pose_gradient_camera_mc(scene, c2w, keep_masks=self._frame_masks, **kw)
        seed_was = scene.field.seed
        try:
            if mask_seed is not None:
                scene.field.seed = int(mask_seed)
            return render.pose_gradient_camera_mc(scene, c2w, **kw)
        finally:
            scene.field.seed = seed_was

    def _begin_render(self, scene: NerfSceneDev, total_rays: int = 0, chunk_rays: int = 0) -> None:
        if self.dropout_masks not in ("counter", "torch"):
            raise ValueError(f"dropout_masks={self.dropout_masks!r}: expected 'counter' or 'torch'")
        self._frame_masks = None
        if self.dropout_masks == "torch" and scene.field.K > 0 and scene.field.p_drop > 0.0:
            self._frame_masks = self._draw_frame_masks(scene, total_rays, chunk_rays)
        scene.field.seed = frame_seed(self.seed, self.frame_counter if self.fresh_masks_per_render else 0)
        self.frame_counter += 1

    def _begin_render_views(self, scene: NerfSceneDev, n_views: int) -> Tuple[bool, Optional[List[int]]]:
        """view v of the batch is frame frame_counter + v: the seeds B successive _begin_render calls would set.
        dropout_masks="torch": the frames' masks are drawn one frame at a time, so the cameras are too."""
        if self.dropout_masks not in ("counter", "torch"):
            raise ValueError(f"dropout_masks={self.dropout_masks!r}: expected 'counter' or 'torch'")
        if self.dropout_masks == "torch" and scene.field.K > 0 and scene.field.p_drop > 0.0:
            return False, None
        self._frame_masks = None
        seeds = [frame_seed(self.seed, (self.frame_counter + v) if self.fresh_masks_per_render else 0) for v in range(n_views)]
        self.frame_counter += n_views
        return True, seeds

    def _draw_frame_masks(self, scene: NerfSceneDev, total_rays: int, chunk_rays: int) -> ops.KeepMasks:
        f, S = scene.field, scene.num_nerf
        if f.any_width:
            raise _lib.UnerfError("dropout_masks='torch': the any-width kernel has no explicit-mask mode")
        need = torch_keep_mask_bytes(f.K, total_rays, S, f.drop_sites)
        if need > self.mask_budget_bytes:
            raise _lib.UnerfError(f"dropout_masks='torch': the packed keep masks of this frame need {need} bytes "
                                  f"(K={f.K} x {total_rays} rays x {S} samples), mask_budget_bytes={self.mask_budget_bytes}")
        return draw_torch_keep_masks(scene.device, f.K, total_rays, S, chunk_rays, f.drop_sites, f.p_drop, self.mask_generator)

    def _render_kwargs(self) -> Dict[str, Any]:
        return {} if self._frame_masks is None else {"keep_masks": self._frame_masks}

    def reference_precision(self) -> str:
        """mcdropout_models.py:86-92: `forward` wraps every render in torch.autocast(enabled=True) -- the Linear layers run
        in float16 on a GPU whatever the implementation"""
        return "f16"

    def _make_field(self):
        c = self.config
        return F.NerfactoMCDropoutField(dropout_rate=c.dropout_rate, rgb_dropout_layers=c.rgb_dropout_layers,
                                        density_dropout_layers=c.density_dropout_layers, **self._field_kwargs())

    def _field_to_device(self, device):
        return self.field.to_device(device, mc_samples=self.config.mc_samples, seed=self.seed)


class NerfactoLaplaceModel(_NerfactoBase):
    config: NerfactoLaplaceModelConfig
    depth_seed: int = 0
    # How often the last-layer samples are redrawn inside one get_outputs_for_camera_unc frame.  "chunk" (the reference):
    # sample_laplace runs inside get_outputs_unc, i.e. once per eval chunk of config.eval_num_rays_per_chunk rays
    # (laplace_model.py:432-443 -> laplace_field.py:331-339, 468-476, 545) -- a 1080p frame is rendered with 64
    # independent sets of n_samples draws, so its Monte-Carlo error is independent from chunk to chunk.  "camera": one
    # set for the whole frame (no visible seams between chunks; the field kernel keeps its 8x4 pixel-patch tiles).
    resample: str = "chunk"
    _no_pose_gradient = ("its colour is the mean over sampled last layers, which the gradient kernel (one deterministic "
                         "nerfacto head) does not evaluate; get_laplace_pose_gradients_for_camera differentiates the frame of a "
                         "named draw of the last layers.")

    @torch.no_grad()
    def get_laplace_pose_gradients_for_camera(self, camera, generator=None, weight_samples=None,
                                              use_deterministic_density: bool = False, prior_prec: float = 1.0,
                                              n_samples: int = 100, eps: float = 1e-9, rays_per_launch: Optional[int] = None,
                                              want_rgb: bool = False):
        """d mean_c(rgb[y, x]) / d camera_to_worlds of the Laplace frame of ONE draw of the last layers -> [H,W,3,4] float32
        on the device (with want_rgb also the mean colour the gradient kernel composited, [H,W,3]): rgb is the mean over the
        sampled heads, and under a fixed draw it is a deterministic function of the pose (render.pose_gradient_camera_laplace;
        sample bins held fixed, fp32 arithmetic).  The sets are drawn exactly as get_outputs_for_camera_unc draws them (the
        same field.sample_last_layers call: a set per eval chunk with resample = "chunk", one set -- with that method's
        warning -- when eval_num_rays_per_chunk is no multiple of 32), so with a generator seeded like the one a
        get_outputs_for_camera_unc call was given this differentiates that frame.  weight_samples = (ws_density, ws_rgb),
        [n, 65] / [n, 195] or stacks [sets, n, ...] with a set per eval chunk: those rows are used and nothing is drawn.
        The sampled heads belong to this call: afterwards the model renders with its mean heads again."""
        if self.resample not in ("chunk", "camera"):
            raise ValueError(f"NerfactoLaplaceModel.resample={self.resample!r}: expected 'chunk' or 'camera'")
        c2w, cam = _camera_args(camera)
        if weight_samples is not None:
            ws = (weight_samples[0], weight_samples[1])
        else:
            n_sets = None
            if self.resample == "chunk":
                chunk = int(self.config.eval_num_rays_per_chunk)
                if chunk <= 0 or chunk % 32:
                    import warnings
                    warnings.warn(f"eval_num_rays_per_chunk={chunk} is not a multiple of 32: per-chunk Laplace sample sets need "
                                  "that; rendering this frame with one set (model.resample = 'camera')")
                else:
                    n_sets = -(-(cam["H"] * cam["W"]) // chunk)
            ws = self.field.sample_last_layers(n_samples=n_samples, prior_prec=prior_prec, eps=eps, generator=generator,
                                               deterministic_density=use_deterministic_density, n_sets=n_sets)
        self._ws = ws
        self._deterministic_density = bool(use_deterministic_density)
        self.invalidate()
        try:
            return render.pose_gradient_camera_laplace(self.device_scene(), c2w, rays_per_launch=rays_per_launch or self.rays_per_launch,
                                                       want_rgb=want_rgb, **cam)
        finally:
            self._ws, self._deterministic_density = None, False
            self.invalidate()

    def _make_field(self):
        return F.NerfactoLaplaceField(density_activation=self.config.density_activation, **self._field_kwargs())

    def reference_precision(self) -> str:
        """laplace_field.py:305, :460: `.float()` in front of every Linear, no autocast around the model -> fp32"""
        return "f16x2"

    _ws = None                       # sampled last layers of the current *_unc call; None: the mean heads
    _ws_per_chunk = True             # a stack [sets, n, P] in _ws holds one set per eval chunk (False: one per camera)
    _view_sets: Optional[List[int]] = None     # get_outputs_for_cameras_unc: first sample set of every camera of the batch
    _deterministic_density = False

    def _field_to_device(self, device):
        if self._ws is None:
            # get_outputs_for_camera / get_outputs / forward without a preceding *_unc call: the deterministic render
            # of NerfactoLaplaceField.forward (laplace_field.py:317-345, 462-465) -- the mean last layers as the single
            # "sample", selector-masked density
            from torch.nn.utils import parameters_to_vector
            ws_d = parameters_to_vector(self.field.mlp_density.parameters()).detach().reshape(1, -1)
            ws_r = parameters_to_vector(self.field.mlp_rgb_ll.parameters()).detach().reshape(1, -1)
            return self.field.to_device(device, ws_density=ws_d, ws_rgb=ws_r, lap_mask_density=1)
        ws_d, ws_r = self._ws
        fd = self.field.to_device(device, ws_density=ws_d, ws_rgb=ws_r, lap_mask_density=int(self._deterministic_density),
                                  lap_chunk_rays=int(self.config.eval_num_rays_per_chunk) if ws_d.dim() == 3 else 0)
        if ws_d.dim() == 3 and not self._ws_per_chunk:
            fd.lap_chunk_rays = 0      # get_outputs_for_cameras_unc, one set per camera: the stack is indexed by view alone
        return fd

    @torch.no_grad()
    def get_outputs_for_camera(self, camera, obb_box=None):
        """the plain (deterministic, mean-head) render unless called through get_outputs_for_camera_unc"""
        if not getattr(self, "_in_unc_call", False) and self._ws is not None:
            self._ws, self._deterministic_density = None, False     # leave the previous camera's sampled heads behind
            self.invalidate()
        return super().get_outputs_for_camera(camera, obb_box)

    def _begin_render_views(self, scene: NerfSceneDev, n_views: int) -> Tuple[bool, Optional[List[int]]]:
        return True, None       # no mask seeds; the per-view sample sets travel in _render_kwargs

    @torch.no_grad()
    def get_outputs_for_cameras(self, cameras, obb_box=None, max_views: int = 16):
        """the plain (deterministic, mean-head) render of every camera unless called through get_outputs_for_cameras_unc"""
        if not getattr(self, "_in_unc_call", False) and self._ws is not None:
            self._ws, self._deterministic_density = None, False
            self.invalidate()
        return super().get_outputs_for_cameras(cameras, obb_box, max_views)

    @torch.no_grad()
    def get_outputs_for_cameras_unc(self, cameras, obb_box=None, is_inference: bool = True,
                                    use_deterministic_density: bool = False, prior_prec: float = 1.0,
                                    n_samples: int = 100, eps: float = 1e-9, generator=None, max_views: int = 16):
        """get_outputs_for_camera_unc for every camera of a batch (argument conventions of get_outputs_for_cameras).  Element
        v equals the v-th of B successive get_outputs_for_camera_unc calls bit for bit, and the generator is left as after
        those calls: for every max_views cameras the sets of those cameras are drawn in the loop's order (camera by camera,
        chunk by chunk, density then colour: field.sample_last_layers(n_sets=...)), stacked into one device field, and the
        cameras rendered with set_base[v] = v * sets per camera (render.render_cameras: lap_view_sets)."""
        if not is_inference:
            raise NotImplementedError("is_inference=False is the training forward (used by compute_hessian_naive only)")
        if self.resample not in ("chunk", "camera"):
            raise ValueError(f"NerfactoLaplaceModel.resample={self.resample!r}: expected 'chunk' or 'camera'")
        if not 1 <= max_views <= _lib.NERF_MAX_VIEWS:
            raise ValueError(f"max_views={max_views}: a launch group holds 1 to {_lib.NERF_MAX_VIEWS} cameras")
        _, H, W, singles = _camera_batch(cameras)
        for cam in singles:
            _camera_args(cam)
        per_chunk = self.resample == "chunk"
        chunk = int(self.config.eval_num_rays_per_chunk)
        from .eval import stack_cameras
        outs: List[Dict[str, torch.Tensor]] = []
        for v0 in range(0, len(singles), max_views):
            part = singles[v0:v0 + max_views]
            spv = 1
            if per_chunk:
                if chunk <= 0 or chunk % 32:
                    import warnings
                    for _ in part:      # (one warning per camera, as the loop gives)
                        warnings.warn(f"eval_num_rays_per_chunk={chunk} is not a multiple of 32: per-chunk Laplace sample sets need "
                                      "that; rendering this frame with one set (model.resample = 'camera')")
                    per_chunk = False
                else:
                    spv = -(-(H * W) // chunk)
            self._ws = self.field.sample_last_layers(n_samples=n_samples, prior_prec=prior_prec, eps=eps, generator=generator,
                                                     deterministic_density=use_deterministic_density, n_sets=len(part) * spv)
            self._ws_per_chunk = per_chunk
            self._view_sets = [i * spv for i in range(len(part))]
            self._deterministic_density = bool(use_deterministic_density)
            self.invalidate()
            self._in_unc_call = True
            try:
                outs.extend(self.get_outputs_for_cameras(stack_cameras(part), obb_box, max_views))
            finally:
                self._in_unc_call = False
                self._ws, self._deterministic_density, self._view_sets = None, False, None
                self._ws_per_chunk = True
                self.invalidate()
        return outs

    @torch.no_grad()
    def get_outputs_for_camera_unc(self, camera, obb_box=None, is_inference: bool = True,
                                   use_deterministic_density: bool = False, prior_prec: float = 1.0,
                                   n_samples: int = 100, eps: float = 1e-9, generator=None):
        """laplace_model.py:403-415.  Draws the last-layer parameter samples on the host the way
        `sample_laplace` does (one torch.randn per head), then renders with the fused kernels.
        use_deterministic_density=True (eval_configs.py LaplaceConfig): the density is the plain, selector-masked
        mean head (no density samples, no depth draws); the colour head is still sampled."""
        if not is_inference:
            raise NotImplementedError("is_inference=False is the training forward (used by compute_hessian_naive only)")
        if self.resample not in ("chunk", "camera"):
            raise ValueError(f"NerfactoLaplaceModel.resample={self.resample!r}: expected 'chunk' or 'camera'")
        n_sets = None
        if self.resample == "chunk":
            _, cam = _camera_args(camera)
            chunk = int(self.config.eval_num_rays_per_chunk)
            if chunk <= 0 or chunk % 32:
                # a kernel tile is 32 rays and must not straddle two sample sets: such a chunk size renders with ONE set
                # for the frame (what every chunk size did before per-chunk sets existed) instead of failing
                import warnings
                warnings.warn(f"eval_num_rays_per_chunk={chunk} is not a multiple of 32: per-chunk Laplace sample sets need "
                              "that; rendering this frame with one set (model.resample = 'camera')")
            else:
                n_sets = -(-(cam["H"] * cam["W"]) // chunk)
        self._ws = self.field.sample_last_layers(n_samples=n_samples, prior_prec=prior_prec, eps=eps, generator=generator,
                                                 deterministic_density=use_deterministic_density, n_sets=n_sets)
        self._deterministic_density = bool(use_deterministic_density)
        self.invalidate()
        self._in_unc_call = True
        try:
            return self.get_outputs_for_camera(camera, obb_box)
        finally:
            # the sampled heads belong to THIS call: get_outputs(ray_bundle) / forward / get_outputs_for_camera_ray_bundle
            # afterwards (ns-eval image metrics, the viewer) must see the deterministic mean-head field again
            self._in_unc_call = False
            self._ws, self._deterministic_density = None, False
            self.invalidate()

    def _render_kwargs(self):
        kw = {"depth_draws": 100, "depth_seed": self.depth_seed}  # num_samples = 100 (laplace_model.py:487)
        if self._view_sets is not None:     # inside get_outputs_for_cameras_unc (render.render_cameras)
            kw["lap_view_sets"] = list(self._view_sets)
        return kw

    @torch.no_grad()
    def compute_hessian_naive(self, pipeline=None, n_iters: int = 1000, ray_batches=None, device=None):
        """laplace_model.py:343-400: fit the diagonal GGN of the two last layers over `n_iters` training
        batches and store it in `field.mlp_density_ggn` / `field.mlp_rgb_ggn` (what `ggn_{n_iters}.pt` holds,
        eval_uncertainty.py:1104-1116).  The reference runs one GGN-vector product per parameter (260
        double-backwards per batch); here a batch is one deterministic forward plus the closed-form Jacobian
        of the rendered colour (unerf_laplace_ggn_diag).  The GGN of a summed-MSE loss does not depend on the
        target image, so only the rays of a batch are used.

        Batches come from `pipeline.datamanager.next_train(i)` -> (ray_bundle, batch) like the reference, or
        from `ray_batches`, an iterable of (origins [B,3], directions [B,3])."""
        from torch.nn.utils import parameters_to_vector
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        c = self.config
        fd = self.field.to_device(device)
        scene = self._build_scene(device, fd)
        dm = parameters_to_vector(self.field.mlp_density.parameters()).detach()
        rm = parameters_to_vector(self.field.mlp_rgb_ll.parameters()).detach()
        gd = torch.zeros(dm.numel(), device=device, dtype=torch.float32)
        gr = torch.zeros(rm.numel(), device=device, dtype=torch.float32)
        it = iter(ray_batches) if ray_batches is not None else None
        for i in range(n_iters):
            if it is not None:
                try:
                    o, d = next(it)
                except StopIteration:
                    break
            else:
                bundle, _batch = pipeline.datamanager.next_train(i)
                o, d = bundle.origins, bundle.directions
            o = o.reshape(-1, 3).to(device=device, dtype=torch.float32).contiguous()
            d = d.reshape(-1, 3).to(device=device, dtype=torch.float32).contiguous()
            sb, _ = render.sample_rays(scene, o, d, None, want_prop_depth=False)
            ops.laplace_ggn_diag(o, d, sb, fd, dm, rm, c.near_plane, c.far_plane, gd, gr, spacing=scene.spacing,
                                 background=scene.background)
        self.field.mlp_density_ggn = gd
        self.field.mlp_rgb_ggn = gr
        self.invalidate()
        return gd, gr


# ------------------------------------------------------------------ splats --------------------

class SplatfactoModel(nn.Module, _ImageMetrics):
    """[UPSTREAM nerfstudio 1.1.0 SplatfactoModel, eval branch] plain splatfacto: rgb, depth, accumulation, background.
    The member model of the reference's splat ensembles (README.md:106-108, ensemble_utils.py:153-156) and the parent
    of ActiveSplatfactoModel (activesplatfacto_model.py:49), which adds the per-splat uncertainty."""
    config: SplatfactoModelConfig
    GAUSS: Tuple[str, ...] = ("means", "scales", "quats", "features_dc", "features_rest", "opacities")

    def __init__(self, config, num_points: int = 1000, **_kw):
        super().__init__()
        self.config = config
        self.step = 0
        self.populate_modules(num_points)

    def populate_modules(self, num_points: int):
        q = torch.randn(num_points, 4)
        self.gauss_params = nn.ParameterDict({
            "means": nn.Parameter((torch.rand(num_points, 3) - 0.5) * 10), "scales": nn.Parameter(torch.zeros(num_points, 3) - 4),
            "quats": nn.Parameter(q / q.norm(dim=-1, keepdim=True)), "features_dc": nn.Parameter(torch.rand(num_points, 3)),
            "features_rest": nn.Parameter(torch.zeros(num_points, 15, 3)),
            "opacities": nn.Parameter(torch.logit(0.1 * torch.ones(num_points, 1))),
        })
        if "log_uncertainties" in self.GAUSS:
            # optimised in log space, initialised U(0,1) (activesplatfacto_model.py:58-61)
            self.gauss_params["log_uncertainties"] = nn.Parameter(torch.rand(num_points, 1))
        # [UPSTREAM SplatfactoModel.populate_modules] the eval background is a stored colour, not part of the
        # checkpoint: "random" -> the Viser grey (0.1490, 0.1647, 0.2157), otherwise the named colour.  It is blended
        # into rgb wherever alpha < 1 and returned as outputs["background"] (activesplatfacto_model.py:159-173, :363).
        self.register_buffer("background_color", splat.background_for(self.config.background_color), persistent=False)
        self.crop_box = None

    def load_state_dict(self, dict, strict: bool = False, **kwargs):  # type: ignore[override]
        """activesplatfacto_model.py:87-100: resize every gaussian parameter to the checkpoint's point
        count, accept the legacy un-prefixed names, and pin step = 30000 (-> SH degree 3).  A checkpoint that lacks one
        of this model's gaussian parameters (a plain splatfacto run loaded as active-splatfacto has no
        `log_uncertainties`) raises instead of leaving it at its random initial value (load_checked)."""
        self.step = 30000
        lpips_source = dict
        dict = strip_pipeline_prefixes(dict)
        if "means" in dict:
            for p in self.GAUSS:
                if p in dict:
                    dict[f"gauss_params.{p}"] = dict[p]
        if "gauss_params.means" not in dict:
            raise RuntimeError(f"{type(self).__name__}.load_state_dict: no gauss_params.means in the checkpoint "
                               f"(keys: {sorted(dict)[:8]})")
        newp = dict["gauss_params.means"].shape[0]
        for name, param in self.gauss_params.items():
            self.gauss_params[name] = nn.Parameter(torch.zeros((newp,) + param.shape[1:], device=param.device))
        report = load_checked(self, dict, strict=strict)
        self._adopt_lpips_weights(lpips_source)
        return report

    def set_crop(self, crop_box) -> None:
        """[UPSTREAM SplatfactoModel.set_crop] crop_box: None or an object with `.within(points [N,3]) -> bool [N(,1)]`
        (a nerfstudio OrientedBox)"""
        self.crop_box = crop_box

    def set_background(self, background_color: torch.Tensor) -> None:
        assert background_color.shape == (3,)
        self.background_color = background_color.to(self.background_color.device, torch.float32)

    @torch.no_grad()
    def get_outputs(self, camera) -> Dict[str, Optional[torch.Tensor]]:
        c2w, cam = _camera_args(camera, lens=False)
        n, gp, crop_ids = self._splat_scene()
        return splat.active_splatfacto_outputs(gp, c2w, background=self.background_color.to(gp["means"].device),
                                               beta_min=getattr(self.config, "beta_min", 0.01), sh_degree=n,
                                               rasterize_mode=self.config.rasterize_mode, crop_ids=crop_ids,
                                               config_sh_degree=self.config.sh_degree, **cam)

    @torch.no_grad()
    def get_outputs_for_camera(self, camera, obb_box=None) -> Dict[str, Optional[torch.Tensor]]:
        """[UPSTREAM SplatfactoModel.get_outputs_for_camera] set_crop(obb_box), then get_outputs(camera)"""
        self.set_crop(obb_box)
        return self.get_outputs(camera)

    @torch.no_grad()
    def get_pose_gradients_for_camera(self, camera, want_rgb: bool = False):
        """d mean_c(rgb[y, x]) / d camera_to_worlds for every pixel of one camera -> [H,W,3,4] float32 on the device (with
        want_rgb also the colour the gradient kernel blended, [H,W,3]): the per-pixel quantity of the reference's
        estimate_gradient_pose_6dof.py:128-139, from splat.pose_gradient_camera (tile lists, skips and stops held fixed; the
        crop box set by set_crop / get_outputs_for_camera is honoured).  One PERSPECTIVE camera, as get_outputs."""
        gp, c2w, kw = self._splat_pose_frame(camera)
        return splat.pose_gradient_camera(gp, c2w, want_rgb=want_rgb, **kw)

    def get_pose_jacobians_for_camera(self, camera, **kw):
        raise NotImplementedError(f"{type(self).__name__}.get_pose_jacobians_for_camera: the ray-sample Jacobian kernel is not "
                                  "built for splat models; their per-channel pose Jacobian is "
                                  "get_splat_pose_jacobians_for_camera (the depth channel and its fill differ).")

    def get_pose_uncertainty_for_camera(self, camera, pose_cov=None, **kw):
        raise NotImplementedError(f"{type(self).__name__}.get_pose_uncertainty_for_camera: the ray-sample Jacobian kernel is not "
                                  "built for splat models; use get_splat_pose_uncertainty_for_camera.")

    def _splat_scene(self):
        """-> the active SH degree n = min(step // interval, config.sh_degree) (:244), the detached gauss_params and the crop
        set by set_crop (bool [N], or None; eval only, :174-180): what every frame function of the model is given"""
        n = min(self.step // self.config.sh_degree_interval, self.config.sh_degree) if self.config.sh_degree > 0 else 0
        gp = {k: v.detach() for k, v in self.gauss_params.items()}
        crop_ids = None
        if self.crop_box is not None and not self.training:
            crop_ids = self.crop_box.within(gp["means"]).squeeze()
        return n, gp, crop_ids

    def _splat_pose_frame(self, camera):
        """get_pose_gradients_for_camera's camera checks, SH degree and crop -> (gp, c2w, the frame's keyword arguments)"""
        c2w, cam = _camera_args(camera, lens=False)
        n, gp, crop_ids = self._splat_scene()
        return gp, c2w, dict(background=self.background_color.to(gp["means"].device), sh_degree=n,
                             rasterize_mode=self.config.rasterize_mode, crop_ids=crop_ids,
                             config_sh_degree=self.config.sh_degree, **cam)

    def _splat_pose_jacobian(self, camera, proj, channels, want) -> Dict[str, torch.Tensor]:
        """splat.pose_jacobian_camera under get_pose_gradients_for_camera's camera checks, SH degree and crop"""
        gp, c2w, kw = self._splat_pose_frame(camera)
        from . import posegrad
        return splat.pose_jacobian_camera(gp, c2w, proj=proj(posegrad, c2w), channels=channels, want=want, **kw)

    def get_pose_information_for_camera(self, camera, image=None, **kw):
        raise NotImplementedError(f"{type(self).__name__}.get_pose_information_for_camera: the ray-sample Jacobian kernel is not "
                                  "built for splat models; use get_splat_pose_information_for_camera.")

    @torch.no_grad()
    def get_splat_pose_information_for_camera(self, camera, image=None, weights=None, mask=None,
                                              channels=("r", "g", "b")) -> Dict[str, Any]:
        """_NerfactoBase.get_pose_information_for_camera for the splat frame: the same inputs and dictionary, from
        splat.pose_normal_eq_camera (get_splat_pose_jacobians_for_camera's Jacobian in the se3 basis -- tile lists, skips,
        stops, the crop and the SH colours held fixed --, reduced in float64 on the device).  The intended weight for
        ActiveSplatfactoModel is 1 / rgb_std^2 of its own outputs.  One PERSPECTIVE camera, as get_outputs."""
        gp, c2w, kw = self._splat_pose_frame(camera)
        target = _pose_target("get_splat_pose_information_for_camera", image, channels)
        out = splat.pose_normal_eq_camera(gp, c2w, target=target, weights=weights, mask=mask, channels=channels, **kw)
        return _with_pose_step(out, image is not None)

    @torch.no_grad()
    def get_splat_pose_jacobians_for_camera(self, camera, channels=ops.POSE_CHANNELS, basis: str = "se3") -> Dict[str, torch.Tensor]:
        """The per-pixel Jacobian of the frame's channels with respect to the camera pose ->
        {"jacobian": [H,W,C,6 | 12], "values": [H,W,C]} float32 on the device; the C rows in ops.POSE_CHANNELS order
        (r, g, b, accumulation, expected_depth).  basis "se3": the six parameters of posegrad.POSE_PARAMS (tx .. angz of
        c2w . exp(xi), the camera's own frame); "c2w": the twelve entries of camera_to_worlds, row-major 3x4.  r / g / b follow
        get_pose_gradients_for_camera's rules (their mean over the channels is its quantity).  expected_depth is the frame's
        depth-sum quotient D / accumulation where something was blended and 0 (value and row) elsewhere: the frame's
        max(depth) fill is not applied here (get_splat_pose_uncertainty_for_camera's `depth` has it).  Tile lists, skips,
        stops, the crop and the SH colours held fixed, fp32.  One PERSPECTIVE camera, as get_outputs."""
        if basis not in ("se3", "c2w"):
            raise ValueError(f"get_splat_pose_jacobians_for_camera: basis={basis!r} (expected 'se3' or 'c2w')")
        proj = (lambda pg, c2w: pg.pose_projection(c2w, None)) if basis == "se3" else (lambda pg, c2w: None)
        out = self._splat_pose_jacobian(camera, proj, channels, ("proj", "val"))
        return {"jacobian": out["proj"], "values": out["val"]}

    @torch.no_grad()
    def get_splat_pose_uncertainty_for_camera(self, camera, pose_cov) -> Dict[str, torch.Tensor]:
        """First-order propagation of a pose covariance to every pixel of a splat frame: var_c = J_c Sigma J_c^T per channel,
        from one walk (posegrad.pose_projection(c2w, pose_cov) contracted per splat, squared in the walk's epilogue).
        pose_cov: [6,6] in posegrad.POSE_PARAMS order (the camera's own frame), or a 6-vector of standard deviations.
        -> [H,W,1] each: rgb_var_pose = mean_c var_c and rgb_std_pose = its root, accumulation_std_pose, depth_std_pose; and
        rgb [H,W,3], accumulation, depth as the walk blended them -- depth with the frame's fill
        where(accumulation > 0, D / accumulation, max of the unnormalised depth sums) (activesplatfacto_model.py:319)."""
        if pose_cov is None:
            raise ValueError("get_splat_pose_uncertainty_for_camera: pose_cov is needed ([6,6] or 6 standard deviations)")
        out = self._splat_pose_jacobian(camera, lambda pg, c2w: pg.pose_projection(c2w, pose_cov), ops.POSE_CHANNELS,
                                        ("var", "val"))
        return self._splat_pose_uncertainty_dict(out["var"], out["val"])

    @staticmethod
    def _splat_pose_uncertainty_dict(var: torch.Tensor, val: torch.Tensor) -> Dict[str, torch.Tensor]:
        """one view's [H,W,5] variances and values -> get_splat_pose_uncertainty_for_camera's dict"""
        rgb_var = var[..., :3].mean(dim=-1, keepdim=True)
        acc, quot = val[..., 3:4], val[..., 4:5]
        depth = torch.where(acc > 0, quot, (quot * acc).max())
        return {"rgb_var_pose": rgb_var, "rgb_std_pose": rgb_var.sqrt(), "accumulation_std_pose": var[..., 3:4].sqrt(),
                "depth_std_pose": var[..., 4:5].sqrt(), "rgb": val[..., :3], "accumulation": acc, "depth": depth}

    @torch.no_grad()
    def get_outputs_for_cameras(self, cameras, obb_box=None, max_views: int = 8) -> List[Dict[str, Optional[torch.Tensor]]]:
        """get_outputs_for_camera for every camera of a batch (camera_to_worlds [B,3,4]; fx, fy, cx, cy scalar or one per
        camera; one image size), rendered max_views cameras per call (splat.active_splatfacto_outputs_batch): element i
        equals get_outputs_for_camera(camera i, obb_box) bit for bit.  The eval loop of the reference renders its test
        cameras one by one (scripts/eval_uncertainty.py:896-904); here they share the per-frame fixed cost.  Images of more
        than lib.SPLAT_BATCH_MAX_TILES tiles (11,999: 2560 x 1440 has 14,400) are rendered camera by camera, with the same
        results."""
        c2w, B, H, W, intr = _splat_camera_batch(cameras, max_views, "get_outputs_for_cameras")
        self.set_crop(obb_box)
        n, gp, crop_ids = self._splat_scene()                                   # the crop once for all cameras
        outs: List[Dict[str, Optional[torch.Tensor]]] = []
        for b0 in range(0, B, max_views):
            sl = slice(b0, min(b0 + max_views, B))
            outs += splat.active_splatfacto_outputs_batch(
                gp, c2w[sl, :3, :4], intr["fx"][sl], intr["fy"][sl], intr["cx"][sl], intr["cy"][sl], H, W,
                background=self.background_color.to(gp["means"].device), beta_min=getattr(self.config, "beta_min", 0.01),
                sh_degree=n, rasterize_mode=self.config.rasterize_mode, crop_ids=crop_ids,
                config_sh_degree=self.config.sh_degree)
        return outs

    def _splat_pose_jacobians(self, cameras, projs, pose_covs, channels, want, max_views: int, what: str):
        """splat.pose_jacobian_cameras, max_views cameras per call, under get_outputs_for_cameras' camera checks and the
        single-camera methods' SH degree and crop (the one set_crop / get_outputs_for_camera left)"""
        c2w, B, H, W, intr = _splat_camera_batch(cameras, max_views, what)
        if isinstance(pose_covs, (list, tuple)) and len(pose_covs) != B:
            raise ValueError(f"{what}: {len(pose_covs)} pose covariances for {B} cameras (give one, or one per camera)")
        n, gp, crop_ids = self._splat_scene()
        from . import posegrad
        outs: List[Dict[str, torch.Tensor]] = []
        for b0 in range(0, B, max_views):
            sl = slice(b0, min(b0 + max_views, B))
            kw = {}
            # each camera's projection from its own camera_to_worlds as given, as the single-camera methods build it
            if projs == "se3":
                kw["projs"] = [posegrad.pose_projection(c2w[v, :3, :4], None) for v in range(sl.start, sl.stop)]
            elif pose_covs is not None:
                kw["projs"] = [posegrad.pose_projection(c2w[v, :3, :4], pose_covs[v] if isinstance(pose_covs, (list, tuple))
                                                        else pose_covs) for v in range(sl.start, sl.stop)]
            outs += splat.pose_jacobian_cameras(
                gp, c2w[sl, :3, :4], intr["fx"][sl], intr["fy"][sl], intr["cx"][sl], intr["cy"][sl], H, W,
                background=self.background_color.to(gp["means"].device), channels=channels, want=want, sh_degree=n,
                rasterize_mode=self.config.rasterize_mode, crop_ids=crop_ids, config_sh_degree=self.config.sh_degree, **kw)
        return outs

    @torch.no_grad()
    def get_splat_pose_jacobians_for_cameras(self, cameras, channels=ops.POSE_CHANNELS, basis: str = "se3",
                                             max_views: int = 8) -> List[Dict[str, torch.Tensor]]:
        """get_splat_pose_jacobians_for_camera for every camera of a batch (the cameras of get_outputs_for_cameras:
        PERSPECTIVE, one image size, intrinsics one value or one per camera), max_views (1 to lib.SPLAT_MAX_VIEWS) cameras per
        shared launch (splat.pose_jacobian_cameras): element i equals get_splat_pose_jacobians_for_camera(camera i, channels,
        basis) bit for bit."""
        if basis not in ("se3", "c2w"):
            raise ValueError(f"get_splat_pose_jacobians_for_cameras: basis={basis!r} (expected 'se3' or 'c2w')")
        outs = self._splat_pose_jacobians(cameras, "se3" if basis == "se3" else None, None, channels, ("proj", "val"), max_views,
                                          "get_splat_pose_jacobians_for_cameras")
        return [{"jacobian": o["proj"], "values": o["val"]} for o in outs]

    @torch.no_grad()
    def get_splat_pose_uncertainty_for_cameras(self, cameras, pose_cov, max_views: int = 8) -> List[Dict[str, torch.Tensor]]:
        """get_splat_pose_uncertainty_for_camera for every camera of a batch, max_views cameras per shared launch: element i
        equals get_splat_pose_uncertainty_for_camera(camera i, its covariance) bit for bit.  pose_cov: one [6,6] or 6-vector
        of standard deviations for all cameras, or a list of one per camera.  Each view's depth fill is its OWN maximum of
        the unnormalised depth sums."""
        if pose_cov is None:
            raise ValueError("get_splat_pose_uncertainty_for_cameras: pose_cov is needed ([6,6] or 6 standard deviations, "
                             "or a list of one per camera)")
        outs = self._splat_pose_jacobians(cameras, None, pose_cov, ops.POSE_CHANNELS, ("var", "val"), max_views,
                                          "get_splat_pose_uncertainty_for_cameras")
        return [self._splat_pose_uncertainty_dict(o["var"], o["val"]) for o in outs]

    # -- the two helpers the eval script calls on splat models (scripts/eval_uncertainty.py:321-322, 676-677) --
    def get_gt_img(self, image: torch.Tensor) -> torch.Tensor:
        """[UPSTREAM SplatfactoModel.get_gt_img] uint8 -> float / 255, then the training-resolution downscale,
        which is 1 at eval (step is pinned to 30000 on load, past the resolution schedule)."""
        if image.dtype == torch.uint8:
            image = image.float() / 255.0
        return image.to(self.gauss_params["means"].device)

    @staticmethod
    def composite_with_background(image: torch.Tensor, background: torch.Tensor) -> torch.Tensor:
        """[UPSTREAM SplatfactoModel.composite_with_background] RGBA ground truth over the render's background."""
        if image.shape[2] == 4:
            alpha = image[..., -1].unsqueeze(-1).repeat((1, 1, 3))
            return alpha * image[..., :3] + (1 - alpha) * background.to(image.device)
        return image

    def composite_gt(self, image: torch.Tensor, background: torch.Tensor) -> torch.Tensor:
        """the composition the eval script applies: composite_with_background(get_gt_img(image), background)"""
        return self.composite_with_background(self.get_gt_img(image), background)


class ActiveSplatfactoModel(SplatfactoModel):
    """models/activesplatfacto/activesplatfacto_model.py:49-367: splatfacto + gauss_params["log_uncertainties"] and the
    uncertainty / depth-variance outputs"""
    config: ActiveSplatfactoModelConfig
    GAUSS = SplatfactoModel.GAUSS + ("log_uncertainties",)
