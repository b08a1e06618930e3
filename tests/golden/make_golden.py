"""Generate the reference-pinned golden vectors under tests/golden/.

Runs ONLY in the build container, where /root/reference is mounted.  It imports the
reference's own Python modules and records inputs + outputs as small data fixtures; nothing of
the reference's source text is copied.  The GPU box never runs this (no /root/reference there);
it only reads the .npz/.json files.

Importable as-is from the reference: utils.create_mlp, metrics.ause, metrics.auce.
Importable behind a stub shim for the absent third-party packages (nerfstudio, gsplat, backpack,
icecream ...): NerfactoLaplaceField.sample_laplace, laplace_model.ComputeWeightsModule,
EnsemblePipeline.get_ensemble_outputs_for_camera_ray_bundle,
NerfactoMCDropoutModel.get_outputs_for_camera_ray_bundle (aggregation part).

    python tests/golden/make_golden.py [recorder ...]       # e.g. golden_eval_rows; without names: every recorder
"""
import importlib.abc
import importlib.machinery
import json
import os
import sys
import types
import warnings
from types import SimpleNamespace

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
STUB_ROOTS = ("nerfstudio", "gsplat", "backpack", "icecream", "tinycudann", "mediapy", "tyro", "cv2",
              "torchmetrics", "torchvision", "torchtyping", "imageio", "nerfacc")


class _StubModule(types.ModuleType):
    """Module whose every attribute is an empty, subclassable class (cached per name)."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        cls = type(name, (), {"__module__": self.__name__})
        setattr(self, name, cls)
        return cls


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, fullname, path, target=None):
        if fullname.split(".")[0] in STUB_ROOTS:
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        return _StubModule(spec.name)

    def exec_module(self, module):
        pass


def install_stubs():
    sys.meta_path.insert(0, _StubFinder())
    sys.path.insert(0, REF)
    # the two enum members the reference's model code indexes field outputs with
    import nerfstudio.field_components.field_heads as fh
    fh.FieldHeadNames.DENSITY, fh.FieldHeadNames.RGB = "density", "rgb"


def golden_create_mlp():
    from nerfuncertainty.utils import create_mlp
    from torch import nn
    cases = {
        "mcdropout_trunk": dict(in_dim=32, num_layers=2, layer_width=64, out_dim=16, activation=nn.ReLU,
                                out_activation=None, dropout_layers=[-1], dropout_rate=0.2),
        "mcdropout_head": dict(in_dim=63, num_layers=3, layer_width=64, out_dim=3, activation=nn.ReLU,
                               out_activation=nn.Sigmoid, dropout_layers=[-1], dropout_rate=0.2),
        "laplace_base": dict(in_dim=32, num_layers=1, layer_width=64, out_dim=64, activation=nn.ReLU,
                             out_activation=nn.ReLU),
        "laplace_head": dict(in_dim=63, num_layers=2, layer_width=64, out_dim=64, activation=nn.ReLU,
                             out_activation=nn.ReLU),
        "skip_and_mid_dropout": dict(in_dim=8, num_layers=4, layer_width=16, out_dim=2, skip_connections=(2,),
                                     activation=nn.ReLU, out_activation=None, dropout_layers=[1, 3],
                                     dropout_rate=0.5),
    }
    out = {}
    for name, kw in cases.items():
        m = create_mlp(**kw)
        mods = []
        for layer in (m if isinstance(m, nn.Sequential) else [m]):
            d = {"type": type(layer).__name__}
            if isinstance(layer, nn.Linear):
                d.update(in_features=layer.in_features, out_features=layer.out_features)
            if isinstance(layer, nn.Dropout):
                d.update(p=layer.p)
            mods.append(d)
        out[name] = {"kwargs": {k: (v.__name__ if isinstance(v, type) else v) for k, v in kw.items()}, "modules": mods}
    json.dump(out, open(os.path.join(OUT, "create_mlp.json"), "w"), indent=1)


def golden_metrics():
    from nerfuncertainty.metrics.ause import ause
    from nerfuncertainty.metrics.auce import auce
    g = torch.Generator().manual_seed(11)
    n = 4096
    err = torch.rand(n, generator=g) ** 2
    unc_good = err * (0.5 + torch.rand(n, generator=g))
    unc_bad = torch.rand(n, generator=g)
    res = {"err": err.numpy(), "unc_good": unc_good.numpy(), "unc_bad": unc_bad.numpy()}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for tag, unc in (("good", unc_good), ("bad", unc_bad)):
            for et in ("rmse", "mae", "mse"):
                ratio, e, ev, a = ause(unc, err, err_type=et)
                res[f"ause_{tag}_{et}"] = np.float64(a)
                res[f"ause_{tag}_{et}_curve"] = np.asarray(e, dtype=np.float64)
                res[f"ause_{tag}_{et}_curve_by_var"] = np.asarray(ev, dtype=np.float64)
        mean = torch.rand(n, generator=g).numpy()
        sigma = (0.05 + 0.2 * torch.rand(n, generator=g)).numpy()
        target = mean + sigma * torch.randn(n, generator=g).numpy() * 1.3
        d = auce(mean, sigma, target)
    res.update(auce_mean=mean, auce_sigma=sigma, auce_target=target)
    for k, v in d.items():
        res["auce_" + k] = np.asarray(v, dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, "metrics.npz"), **res)


def golden_sample_laplace():
    from nerfuncertainty.models.laplace.laplace_field import NerfactoLaplaceField
    g = torch.Generator().manual_seed(5)
    res = {}
    for tag, out_dim, act in (("density", 1, torch.exp), ("rgb", 3, torch.sigmoid)):
        lin = torch.nn.Linear(64, out_dim)
        with torch.no_grad():
            lin.weight.copy_(torch.randn(out_dim, 64, generator=g) * 0.2)
            lin.bias.copy_(torch.randn(out_dim, generator=g) * 0.2)
        x = torch.randn(257, 64, generator=g)
        ggn = torch.rand(64 * out_dim + out_dim, generator=g) * 1e3
        mu_q = torch.nn.utils.parameters_to_vector(lin.parameters()).detach().clone()
        seed = 1234 + out_dim
        torch.manual_seed(seed)
        mu, var = NerfactoLaplaceField.sample_laplace(None, module=lin, activation=act, diag_ggn=ggn, input=x,
                                                      n_samples=100, prior_prec=1.0, eps=1e-9)
        res.update({f"{tag}_mu_q": mu_q.numpy(), f"{tag}_ggn": ggn.numpy(), f"{tag}_x": x.numpy(),
                    f"{tag}_seed": np.int64(seed), f"{tag}_mean": mu.detach().numpy(),
                    f"{tag}_var": var.detach().numpy()})
    np.savez_compressed(os.path.join(OUT, "sample_laplace.npz"), **res)


def golden_get_weights():
    from nerfuncertainty.models.laplace.laplace_model import ComputeWeightsModule
    g = torch.Generator().manual_seed(3)
    dens = torch.exp(torch.randn(64, 48, 1, generator=g) * 2.0)
    dens[5] = 0.0
    dens[6, 10:] = 1e6
    deltas = torch.rand(64, 48, 1, generator=g) * 0.2
    w = ComputeWeightsModule()(dens, deltas)
    np.savez_compressed(os.path.join(OUT, "get_weights.npz"), density=dens.numpy(), deltas=deltas.numpy(),
                        weights=w.numpy())


def _fake_member_outputs(g, with_std, M=5, H=6, W=7):
    outs = []
    for _ in range(M):
        o = {"rgb": torch.rand(H, W, 3, generator=g), "depth": torch.rand(H, W, 1, generator=g) * 5,
             "expected_depth": torch.rand(H, W, 1, generator=g) * 5, "accumulation": torch.rand(H, W, 1, generator=g)}
        if with_std:
            o["rgb_var"] = torch.rand(H, W, 1, generator=g) * 0.1
            o["rgb_std"] = o["rgb_var"].sqrt()
            o["depth_var"] = torch.rand(H, W, 1, generator=g)
            o["depth_std"] = o["depth_var"].sqrt()
        outs.append(o)
    return outs


def golden_ensemble():
    from nerfuncertainty.models.ensemble.ensemble_pipeline import EnsemblePipeline
    g = torch.Generator().manual_seed(9)
    res = {}
    for tag, with_std in (("plain", False), ("alea", True)):
        members = _fake_member_outputs(g, with_std)
        models = [SimpleNamespace(get_outputs_for_camera=(lambda cam, obb_box=None, o=o: o)) for o in members]
        fake = SimpleNamespace(models=models)
        out = EnsemblePipeline.get_ensemble_outputs_for_camera_ray_bundle(fake, None)
        for i, o in enumerate(members):
            for k, v in o.items():
                res[f"{tag}_in{i}_{k}"] = v.numpy()
        for k, v in out.items():
            res[f"{tag}_out_{k}"] = v.numpy()
    np.savez_compressed(os.path.join(OUT, "ensemble.npz"), **res)


def golden_mc_aggregate():
    import nerfstudio.models.nerfacto as stub_nerfacto
    from nerfuncertainty.models.mcdropout.mcdropout_models import NerfactoMCDropoutModel
    g = torch.Generator().manual_seed(21)
    K = 8
    passes = _fake_member_outputs(g, False, M=K)
    it = iter(passes)
    # the reference calls super().get_outputs_for_camera_ray_bundle K times; hand it the passes
    stub_nerfacto.NerfactoModel.get_outputs_for_camera_ray_bundle = lambda self, b: next(it)
    obj = object.__new__(NerfactoMCDropoutModel)
    obj.training = False
    obj.apply = lambda fn: None
    obj.eval = lambda: None
    obj.config = SimpleNamespace(mc_samples=K)
    out = obj.get_outputs_for_camera_ray_bundle(None)
    res = {}
    for i, o in enumerate(passes):
        for k, v in o.items():
            res[f"in{i}_{k}"] = v.numpy()
    for k, v in out.items():
        res[f"out_{k}"] = v.numpy()
    np.savez_compressed(os.path.join(OUT, "mc_aggregate.npz"), **res)


# ---------------------------------------------------------------------------------------------------------------
# [REF] model glue driven with a fake `self` (the reference's own get_outputs code runs; the upstream primitives it
# calls -- gsplat kernels, nerfstudio samplers / renderers -- are bound to the ORACLE's restatements).  These fixtures
# pin the oracle's model-level functions (active_splatfacto_outputs, laplace_outputs, active_outputs: composition,
# key names, the four-raster-pass structure, the depth-draw averaging, ...) to the reference's text; the primitives
# themselves stay upstream-recall.
# ---------------------------------------------------------------------------------------------------------------

def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def golden_splat_get_outputs():
    """ActiveSplatfactoModel.get_outputs (activesplatfacto_model.py:142-367), eval branch, on a seeded 400-splat set:
    default config, a named background, sh_degree 0, an early SH degree (step < 3000), antialiased mode."""
    import nerfuncertainty.models.activesplatfacto.activesplatfacto_model as M
    from nerfstudio.cameras.cameras import Cameras
    sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
    from oracle import splat_oracle as SO

    def project_gaussians(means, scales, glob_scale, quats, viewmat, fx, fy, cx, cy, H, W, bw, clip_thresh=0.01):
        pr = SO.project_gaussians(_np(means), _np(scales), glob_scale, _np(quats), _np(viewmat), fx, fy, cx, cy, H, W, bw,
                                  clip_thresh)
        return tuple(torch.from_numpy(pr[k]) for k in ("xys", "depths", "radii", "conics", "compensation",
                                                       "num_tiles_hit", "cov3d"))

    def spherical_harmonics(n, viewdirs, coeffs):
        return torch.from_numpy(SO.spherical_harmonics(n, _np(viewdirs), _np(coeffs)))

    def rasterize_gaussians(xys, depths, radii, conics, num_tiles_hit, colors, opacity, H, W, bw, background=None,
                            return_alpha=False):
        I, cum, keys, gids, bins = SO.bin_and_sort(_np(xys), _np(depths), _np(radii), _np(num_tiles_hit), H, W, bw)
        out, fT, _ = SO.rasterize(gids, bins, _np(xys), _np(conics), _np(colors), _np(opacity), H, W,
                                  None if background is None else _np(background), bw)
        out = torch.from_numpy(out)
        return (out, torch.from_numpy(1.0 - fT)) if return_alpha else out

    M.project_gaussians, M.spherical_harmonics, M.rasterize_gaussians = project_gaussians, spherical_harmonics, rasterize_gaussians
    M.renderers.BACKGROUND_COLOR_OVERRIDE = None

    g = torch.Generator().manual_seed(31)
    N, H, W = 400, 40, 56
    q = torch.randn(N, 4, generator=g)
    gp = {"means": (torch.rand(N, 3, generator=g) * 2 - 1) * 0.8, "scales": torch.randn(N, 3, generator=g) * 0.4 - 2.6,
          "quats": q, "features_dc": torch.randn(N, 3, generator=g) * 0.5,
          "features_rest": torch.randn(N, 15, 3, generator=g) * 0.05, "opacities": torch.randn(N, 1, generator=g) * 2,
          "log_uncertainties": torch.rand(N, 1, generator=g)}
    c2w = torch.tensor([[0.8, -0.2, 0.5657, 1.4], [0.6, 0.2667, -0.7542, -1.9], [0.0, 0.9428, 0.3333, 0.8]])
    c2w[:, :3] = torch.linalg.qr(c2w[:, :3])[0]
    fx = fy = 50.0
    res = {"c2w": c2w.numpy(), "intr": np.array([fx, fy, W / 2, H / 2, H, W], dtype=np.float64)}
    for k, v in gp.items():
        res["gp_" + k] = v.numpy()

    def run(tag, background, sh_degree=3, step=30000, rasterize_mode="classic"):
        cam = object.__new__(Cameras)
        cam.shape = (1,)
        cam.width, cam.height = torch.tensor([[W]]), torch.tensor([[H]])
        cam.fx, cam.fy = torch.tensor([[fx]]), torch.tensor([[fy]])
        cam.cx, cam.cy = torch.tensor([[W / 2.0]]), torch.tensor([[H / 2.0]])
        cam.rescale_output_resolution = lambda f: None
        obj = object.__new__(M.ActiveSplatfactoModel)
        obj.training = False
        obj.device = torch.device("cpu")
        obj.step = step
        obj.config = SimpleNamespace(background_color="random", sh_degree=sh_degree, sh_degree_interval=1000,
                                     rasterize_mode=rasterize_mode, beta_min=0.01, output_depth_during_training=False)
        obj.gauss_params = gp
        for k in ("means", "scales", "quats", "features_dc", "features_rest", "opacities"):
            setattr(obj, k, gp[k])
        obj.background_color = background
        obj.crop_box = None
        obj.camera_optimizer = SimpleNamespace(apply_to_camera=lambda c: c2w[None])
        obj._get_downscale_factor = lambda: 1
        obj.activation_uncertainty = torch.nn.Softplus()
        out = obj.get_outputs(cam)
        res[f"{tag}_cfg"] = np.array([sh_degree, step, 1 if rasterize_mode == "antialiased" else 0], dtype=np.int64)
        for k, v in out.items():
            res[f"{tag}_out_{k}"] = _np(v).astype(np.float32)

    run("default", torch.tensor([0.1490, 0.1647, 0.2157]))
    run("white", torch.ones(3))
    run("sh0", torch.zeros(3), sh_degree=0)
    run("early", torch.tensor([0.1490, 0.1647, 0.2157]), step=1500)
    run("aa", torch.tensor([0.1490, 0.1647, 0.2157]), rasterize_mode="antialiased")
    np.savez_compressed(os.path.join(OUT, "splat_get_outputs.npz"), **res)


class _FakeRaySamples:
    """what the reference's model code touches on a nerfstudio RaySamples: frustums.starts / ends and get_weights"""

    def __init__(self, eb):
        self.frustums = SimpleNamespace(starts=eb[:, :-1, None], ends=eb[:, 1:, None])
        self.deltas = eb[:, 1:, None] - eb[:, :-1, None]
        self._get_weights = None

    def get_weights(self, densities):
        from nerfuncertainty.models.laplace.laplace_model import ComputeWeightsModule
        return ComputeWeightsModule()(densities, self.deltas)          # the reference's own copy of get_weights


def _oracle_renderers(O):
    def steps_of(rs):
        return ((rs.frustums.starts + rs.frustums.ends) / 2)[..., 0]
    return dict(
        renderer_rgb=lambda rgb, weights: O.render_rgb(rgb, weights[..., 0]),
        renderer_accumulation=lambda weights: O.render_accumulation(weights[..., 0]),
        renderer_depth=lambda weights, ray_samples: O.render_depth_median(weights[..., 0], steps_of(ray_samples)),
        renderer_expected_depth=lambda weights, ray_samples: O.render_depth_expected(weights[..., 0], steps_of(ray_samples)),
        renderer_uncertainty=lambda betas, weights: O.render_uncertainty(betas[..., 0], weights[..., 0]),
    )


def golden_nerf_model_glue():
    """NerfactoLaplaceModel.get_outputs_unc (laplace_model.py:456-556, both density modes) and
    ActiveNerfactoModel.get_outputs (activenerfacto_model.py:83-152) with a fake `self`: the proposal sampler returns
    seeded bins, the field returns seeded outputs, the renderers are the oracle's; everything in between is the
    reference's code."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
    from oracle import nerf_oracle as O
    from nerfstudio.field_components.field_heads import FieldHeadNames
    import nerfuncertainty.models.laplace.laplace_model as LM
    import nerfuncertainty.models.activenerfacto.activenerfacto_model as AM
    g = torch.Generator().manual_seed(41)
    R, S = 96, 48
    res = {}

    def bins(n):
        sb = torch.sort(torch.rand(R, n + 1, generator=g), dim=-1).values
        return O.spacing_to_euclidean(sb, 0.05, 1000.0)

    eb0, eb1, eb = bins(256), bins(96), bins(S)
    w0 = torch.rand(R, 256, 1, generator=g) / 100
    w1 = torch.rand(R, 96, 1, generator=g) / 40
    density = torch.exp(torch.randn(R, S, 1, generator=g) * 2.0)
    density[0] = 0.0
    rgb = torch.rand(R, S, 3, generator=g)
    res.update(eb0=eb0.numpy(), eb1=eb1.numpy(), eb=eb.numpy(), w0=w0.numpy(), w1=w1.numpy(), density=density.numpy(),
               rgb=rgb.numpy())
    rend = _oracle_renderers(O)

    def sampler(ray_bundle, density_fns=None):
        return _FakeRaySamples(eb), [w0.clone(), w1.clone()], [_FakeRaySamples(eb0), _FakeRaySamples(eb1)]

    # ---- laplace ----
    density_var = torch.rand(R, S, 1, generator=g) * density ** 2 * 0.05
    rgb_var = torch.rand(R, S, 1, generator=g) * 0.01
    res.update(lap_density_var=density_var.numpy(), lap_rgb_var=rgb_var.numpy())
    for tag, det in (("lap", False), ("lapdet", True)):
        obj = object.__new__(LM.NerfactoLaplaceModel)
        obj.training = False
        obj.config = SimpleNamespace(predict_normals=False, use_gradient_scaling=False, num_proposal_iterations=2)
        obj.proposal_sampler = sampler
        obj.density_fns = None
        obj.field = SimpleNamespace(forward_unc=lambda rs, **kw: {FieldHeadNames.DENSITY: density, FieldHeadNames.RGB: rgb,
                                                                  "density_var": density_var, "rgb_var": rgb_var})
        obj.renderer_rgb, obj.renderer_accumulation = rend["renderer_rgb"], rend["renderer_accumulation"]
        obj.renderer_depth, obj.renderer_expected_depth = rend["renderer_depth"], rend["renderer_expected_depth"]
        obj.uncertainty_renderer = rend["renderer_uncertainty"]
        seed = 77
        torch.manual_seed(seed)
        out = obj.get_outputs_unc(None, is_inference=True, use_deterministic_density=det)
        # the draw Normal(loc, scale).sample((100,)) made: same generator state -> loc + scale * randn(100, R, S, 1)
        torch.manual_seed(seed)
        res[f"{tag}_noise"] = torch.randn(100, R, S, 1).numpy()[..., 0]
        for k, v in out.items():
            res[f"{tag}_out_{k}"] = _np(v).astype(np.float32)

    # ---- active-nerfacto ----
    beta = torch.rand(R, S, 1, generator=g) + 0.01
    res["act_beta"] = beta.numpy()
    obj = object.__new__(AM.ActiveNerfactoModel)
    obj.training = False
    obj.config = SimpleNamespace(predict_normals=False, use_gradient_scaling=False, num_proposal_iterations=2)
    obj.proposal_sampler = sampler
    obj.density_fns = None
    obj.field = SimpleNamespace(forward=lambda rs, compute_normals=False: {FieldHeadNames.DENSITY: density,
                                                                           FieldHeadNames.RGB: rgb, "rgb_var": beta})
    obj.renderer_rgb, obj.renderer_accumulation = rend["renderer_rgb"], rend["renderer_accumulation"]
    obj.renderer_depth, obj.renderer_expected_depth = rend["renderer_depth"], rend["renderer_expected_depth"]
    obj.renderer_uncertainty = rend["renderer_uncertainty"]
    out = obj.get_outputs(None)
    for k, v in out.items():
        res[f"act_out_{k}"] = _np(v).astype(np.float32)
    np.savez_compressed(os.path.join(OUT, "nerf_model_glue.npz"), **res)


class _FakeFrustums:
    def __init__(self, o, d, eb):
        R, S = eb.shape[0], eb.shape[1] - 1
        self.origins, self.directions = o[:, None, :].expand(R, S, 3), d[:, None, :].expand(R, S, 3)
        self.starts, self.ends = eb[:, :-1, None], eb[:, 1:, None]
        self.shape = (R, S)

    def get_positions(self):
        return self.origins + self.directions * (self.starts + self.ends) / 2


def golden_field_glue():
    """[REF] Field methods with a fake `self`: NerfactoLaplaceField.get_density / get_outputs / forward_unc /
    sample_laplace (laplace_field.py:279-568, is_inference on and off), ActiveNerfactoField.get_density / forward
    (activenerfacto_field.py:162-215), NerfactoMCDropoutField.get_density (mcdropout_fields.py:146-174).  Upstream
    components (hash encoding, contraction, SH, the parent's colour head) are the oracle's; the Linear / create_mlp
    modules are real torch modules carrying a seeded synthetic field."""
    root = os.path.dirname(os.path.dirname(OUT))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import conftest  # noqa: F401
    from oracle import nerf_oracle as O
    from uncertainty_nerf_gs_amd import synthetic
    from nerfstudio.field_components.field_heads import FieldHeadNames
    import nerfuncertainty.models.laplace.laplace_field as LF
    import nerfuncertainty.models.activenerfacto.activenerfacto_field as AF
    import nerfuncertainty.models.mcdropout.mcdropout_fields as MF
    from torch import nn
    g = torch.Generator().manual_seed(51)
    R, S = 40, 12
    o = torch.randn(R, 3, generator=g) * 0.3
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    eb = torch.sort(torch.rand(R, S + 1, generator=g) * 3.0 + 0.05, dim=-1).values
    eb[:4] = eb[:4] * 400                       # a few rays far outside the box (contraction branch)
    eb[4] = eb[4] * 1e30                        # so far that the contraction returns exactly 2: (2+2)/4 = 1 -> selector off
    res = {"o": o.numpy(), "d": d.numpy(), "eb": eb.numpy()}

    def lin(w, b):
        m = nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            m.weight.copy_(w)
            m.bias.copy_(b)
        return m

    def samples():
        rs = SimpleNamespace(frustums=_FakeFrustums(o, d, eb), camera_indices=torch.zeros(R, S, 1, dtype=torch.long))
        return rs

    def common(obj, fp):
        obj.training = False
        obj.spatial_distortion = O.contract_inf
        obj.geo_feat_dim = 15
        obj.appearance_embedding_dim = 32
        obj.use_average_appearance_embedding = True
        obj.embedding_appearance = SimpleNamespace(mean=lambda dim=0: fp.appearance)
        obj.use_transient_embedding = obj.use_semantics = obj.use_pred_normals = False
        obj.direction_encoding = O.sh16

    for mod in (LF, AF, MF):
        mod.trunc_exp = torch.exp
        if hasattr(mod, "get_normalized_directions"):
            mod.get_normalized_directions = lambda x: (x + 1.0) / 2.0

    # ---- laplace -------------------------------------------------------------------------------------------
    t = synthetic.make_scene_tensors(seed=61, kind="laplace", log2T=9, prop_log2T=8)
    fp = O.scene_from_tensors(t).field
    f = t["field"]
    for k in ("table", "scalings", "w0", "b0", "w1", "b1", "density_w", "density_b", "appearance"):
        res["lap_" + k] = f[k].numpy()
    for i in range(3):
        res[f"lap_head_w{i}"], res[f"lap_head_b{i}"] = f["head_w"][i].numpy(), f["head_b"][i].numpy()
    res["lap_log2T"] = np.int64(f["log2T"])
    obj = object.__new__(LF.NerfactoLaplaceField)
    common(obj, fp)
    obj.base_grid = lambda x: O.grid_encode(x, fp.grid)
    obj.base_mlp = nn.Sequential(lin(f["w0"], f["b0"]))                 # create_mlp(num_layers=1): a bare Linear
    obj.mlp_hidden = lin(f["w1"], f["b1"])
    obj.mlp_density = lin(f["density_w"], f["density_b"])
    obj.mlp_head = nn.Sequential(lin(f["head_w"][0], f["head_b"][0]), nn.ReLU(), lin(f["head_w"][1], f["head_b"][1]), nn.ReLU())
    obj.mlp_rgb_ll = lin(f["head_w"][2], f["head_b"][2])
    obj.density_activation = torch.exp
    obj.rgb_activation = nn.Sigmoid()
    obj.mlp_density_ggn = torch.rand(65, generator=g) * 1e3
    obj.mlp_rgb_ggn = torch.rand(195, generator=g) * 1e3
    res["lap_ggn_density"], res["lap_ggn_rgb"] = obj.mlp_density_ggn.numpy(), obj.mlp_rgb_ggn.numpy()
    for tag, det in (("lapf", False), ("lapf_det", True)):
        seed = 900 + int(det)
        torch.manual_seed(seed)
        with torch.no_grad():
            out = obj.forward_unc(samples(), is_inference=True, use_deterministic_density=det, prior_prec=1.0, n_samples=100)
        torch.manual_seed(seed)          # the draws sample_laplace made, in call order: density head (unless det), colour head
        if not det:
            res[f"{tag}_noise_density"] = torch.randn(100, 65).numpy()
        res[f"{tag}_noise_rgb"] = torch.randn(100, 195).numpy()
        res[f"{tag}_density"] = _np(out[FieldHeadNames.DENSITY])
        res[f"{tag}_rgb"] = _np(out[FieldHeadNames.RGB])
        res[f"{tag}_rgb_var"] = _np(out["rgb_var"])
        if out["density_var"] is not None:
            res[f"{tag}_density_var"] = _np(out["density_var"])
    with torch.no_grad():   # the plain training-style forward pieces: get_density(is_inference=False) + get_outputs(False)
        dens, emb, _ = obj.get_density(samples(), is_inference=False)
        outs = obj.get_outputs(samples(), density_embedding=emb, is_inference=False)
    res["lapf_plain_density"], res["lapf_plain_rgb"] = _np(dens), _np(outs[FieldHeadNames.RGB])

    # ---- active-nerfacto ------------------------------------------------------------------------------------
    t = synthetic.make_scene_tensors(seed=62, kind="active", log2T=9, prop_log2T=8)
    fpa = O.scene_from_tensors(t).field
    f = t["field"]
    for k in ("table", "scalings", "w0", "b0", "w1", "b1", "appearance"):
        res["act_" + k] = f[k].numpy()
    for i in range(3):
        res[f"act_head_w{i}"], res[f"act_head_b{i}"] = f["head_w"][i].numpy(), f["head_b"][i].numpy()
    obj = object.__new__(AF.ActiveNerfactoField)
    common(obj, fpa)
    obj.mlp_base = lambda x: O.mlp_forward(O.grid_encode(x, fpa.grid), fpa.grid.weights, fpa.grid.biases)
    obj.average_init_density = 1.0
    obj.beta_min = 0.01
    obj.activation_uncertainty = nn.Softplus()

    def parent_get_outputs(ray_samples, density_embedding=None):      # [UPSTREAM NerfactoField.get_outputs]
        x = O._color_inputs(d, S, density_embedding, fpa.appearance)
        return {FieldHeadNames.RGB: O.mlp_forward(x, fpa.head_w, fpa.head_b, "sigmoid").view(R, S, 3)}

    obj.get_outputs = parent_get_outputs
    with torch.no_grad():
        out = obj.forward(samples())
    res["actf_density"], res["actf_rgb"], res["actf_rgb_var"] = _np(out[FieldHeadNames.DENSITY]), _np(out[FieldHeadNames.RGB]), _np(out["rgb_var"])

    # ---- mc-dropout get_density (dropout modules in eval mode: the deterministic trunk) ---------------------------
    t = synthetic.make_scene_tensors(seed=63, kind="mcdropout", log2T=9, prop_log2T=8)
    fpm = O.scene_from_tensors(t).field
    f = t["field"]
    for k in ("table", "scalings", "w0", "b0", "w1", "b1"):
        res["mc_" + k] = f[k].numpy()
    obj = object.__new__(MF.NerfactoMCDropoutField)
    common(obj, fpm)
    obj.density_dropout_layers = True
    obj.mlp_base_grid = lambda x: O.grid_encode(x, fpm.grid)
    from nerfuncertainty.utils import create_mlp
    trunk = create_mlp(in_dim=32, num_layers=2, layer_width=64, out_dim=16, activation=nn.ReLU, out_activation=None,
                       dropout_layers=[-1], dropout_rate=0.2).eval()
    with torch.no_grad():
        trunk[0].weight.copy_(f["w0"]); trunk[0].bias.copy_(f["b0"]); trunk[3].weight.copy_(f["w1"]); trunk[3].bias.copy_(f["b1"])
    obj.mlp_base = trunk
    obj.average_init_density = 0.01
    with torch.no_grad():
        dens, emb = obj.get_density(samples())
    res["mcf_density"], res["mcf_embedding"] = _np(dens), _np(emb)
    np.savez_compressed(os.path.join(OUT, "field_glue.npz"), **res)


def golden_eval_configs():
    """field names and defaults of the eval script's configuration dataclasses (scripts/eval_configs.py)"""
    import dataclasses
    from nerfuncertainty.scripts import eval_configs as ec
    out = {}
    for name in ("EvalUncertainty", "LaplaceConfig", "EnsembleConfig", "MCDropoutConfig", "ActiveNerfactoConfig",
                 "ActiveSplatfactoConfig"):
        fields = {}
        for f in dataclasses.fields(getattr(ec, name)):
            d = None if f.default is dataclasses.MISSING else f.default
            fields[f.name] = {"required": f.default is dataclasses.MISSING, "default": str(d) if d is not None and not isinstance(d, (bool, int, float)) else d}
        out[name] = fields
    json.dump(out, open(os.path.join(OUT, "eval_configs.json"), "w"), indent=1)


# ---------------------------------------------------------------------------------------------------------------
# [REF] tests/golden/eval_rows.npz: the reference's own per-image eval functions (scripts/eval_uncertainty.py:
# get_unc_metrics_rgb, get_unc_metrics_depth, get_image_metrics_and_images_unc, get_average_uncertainty_metrics) run on
# seeded images at the smallest pixel counts on either side of the metric kernels' boundaries (wave 64, workgroup 256,
# sort tile 4096; 35 pixels: fewer than 100, where the reference's last sparsification cuts keep nothing and its AUSE is
# NaN).  Every case is recorded twice: on float32 tensors (the reference as it runs) and on the same values as float64
# (the anchor of the tests' yardstick).  Inputs and outputs are plain arrays.
# Left out: a render whose shape differs from the depth GT map (the reference resizes it with torchvision's `resize`,
# which is not installed where this runs), and the splat `background` branch (it calls upstream model code).
# The recorder asserts that every case is well defined by the reference alone: the float32 and the float64 run count
# the same AUCE coverages (no |r| / sigma within rounding of a threshold), and no output moves beyond the float32 -
# float64 distance when the pixels are permuted (nothing rests on the order of tied keys); a case that fails either is
# reseeded.
# ---------------------------------------------------------------------------------------------------------------

EVAL_SHAPES = ((5, 7), (7, 9), (8, 8), (5, 13), (15, 17), (16, 16), (1, 257), (63, 65), (64, 64), (17, 241))
EVAL_CURVES = ("err_mse", "err_rmse", "err_mae", "err_var_mse", "err_var_rmse", "err_var_mae")
EVAL_AUCE = ("coverage_values", "avg_length_values", "coverage_error_values", "abs_coverage_error_values",
             "neg_coverage_error_values")
EVAL_SCALARS = ("ause_mse", "ause_rmse", "ause_mae", "avg_var", "auc_abs_error_values", "auc_length_values",
                "auc_neg_error_values")
EVAL_MIN_RGB_STD, EVAL_MIN_DEPTH_STD = 3e-2, 1.0


def _eval_module():
    """scripts/eval_uncertainty.py behind the shim, its plotting and colour-mapping helpers replaced by pass-throughs"""
    import nerfuncertainty.scripts.eval_uncertainty as eu
    eu.colormaps = SimpleNamespace(apply_colormap=lambda x, **kw: x, apply_depth_colormap=lambda x, **kw: x)
    return eu


def _eval_pack(res, tag, r32, r64):
    """one case's two records as arrays: per precision `_scalars` in the order of `eval_scalar_names`; the float64 run's
    `_f64_curves` [6, 100] in the order of `eval_curve_names` and `_f64_avg_length` [99], and the float32 run's as its
    difference from them, `_d32_curves` / `_d32_avg_length` (float32 run - float64 run, ~1e-8, kept as float32: the
    float32 run is float64 run + difference to 1e-15); the four coverage arrays once, `_coverage` [4, 99] in the order of
    `eval_coverage_names` -- the two runs count the same coverages, so these are equal bit for bit"""
    names = [k for k in r64 if k not in EVAL_CURVES + EVAL_AUCE]
    coverage = [k for k in EVAL_AUCE if k != "avg_length_values"]
    assert res.setdefault("eval_scalar_names", names) == names
    res["eval_curve_names"], res["eval_coverage_names"] = list(EVAL_CURVES), coverage
    for prec, rec in (("f32", r32), ("f64", r64)):
        res[f"{tag}_{prec}_scalars"] = np.array([rec[k] for k in names], dtype=np.float64)
    res[f"{tag}_f64_curves"] = np.stack([r64[k] for k in EVAL_CURVES])
    res[f"{tag}_f64_avg_length"] = r64["avg_length_values"]
    res[f"{tag}_d32_curves"] = (np.stack([r32[k] for k in EVAL_CURVES]) - res[f"{tag}_f64_curves"]).astype(np.float32)
    res[f"{tag}_d32_avg_length"] = (r32["avg_length_values"] - r64["avg_length_values"]).astype(np.float32)
    assert all(np.array_equal(r32[k], r64[k]) for k in coverage)
    res[f"{tag}_coverage"] = np.stack([r64[k] for k in coverage])


def _eval_record(d, nll_key):
    """what the tests read of one call's output dictionary, as float64 arrays"""
    out = {k: np.asarray(d[k], dtype=np.float64) for k in EVAL_SCALARS + EVAL_CURVES + EVAL_AUCE}
    out["nll"] = np.float64(d[nll_key])
    mse_mean = d["mse"].mean().item()                      # eval_uncertainty.py:717-718, :768-769
    out["mse"], out["rmse"] = np.float64(mse_mean), np.float64(np.sqrt(mse_mean))
    return out


def _eval_well_defined(r32, r64, permuted64, nll_abs_mean):
    """the two conditions of the header comment -> None, or what failed"""
    if not np.array_equal(r32["coverage_values"], r64["coverage_values"]):
        return "float32 and float64 coverages differ"
    for k, p64 in ((k, p64) for k in r64 for p64 in permuted64):
        a, b, c = r64[k], p64[k], r32[k]
        if not (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isnan(a), np.isnan(c))):
            return f"{k}: NaN pattern moves"
        scale = nll_abs_mean if k == "nll" else np.abs(a)
        room = np.maximum(np.abs(c - a), 2.0 ** -23 * scale)
        if not np.all(np.nan_to_num(np.abs(b - a) - room) <= 0):
            return f"{k}: moves by {np.nanmax(np.abs(b - a)):.3e} under a permutation of the pixels"
    return None


def _rgb_case(H, W, seed, variant=""):
    """gt on the 8-bit grid, a prediction inside (0, 1), then the plants: above 1 in one channel and in all three, exactly 1,
    below 0; sigma below the NLL floor and exactly on it; sigma 0 with a zero and with a non-zero residual.
    variant "_b": the plants above 1 alone; "_c": every plant but those above 1"""
    g = torch.Generator().manual_seed(seed)
    n = H * W
    gt = torch.round(torch.rand(n, 3, generator=g) * 255) / 255
    std = 0.035 + 0.2 * torch.rand(n, generator=g)
    pred = torch.clamp(gt + std[:, None] * torch.randn(n, 3, generator=g), 0.002, 0.998)
    at = iter(torch.randperm(n, generator=g).tolist())
    if variant != "_c":
        pred[next(at), 1] = 1.31
        pred[next(at), 0] = 1.0 + 2.0 ** -20
        pred[next(at)] = torch.tensor([1.07, 1.6, 1.002])
        pred[next(at)] = torch.tensor([2.5, 1.25, 1.125])
    if variant == "_b":
        return pred.view(H, W, 3), gt.view(H, W, 3), std.view(H, W, 1)
    pred[next(at), 2] = 1.0
    pred[next(at), 0] = -0.05
    std[next(at)] = 0.01
    std[next(at)] = float(np.float32(EVAL_MIN_RGB_STD))
    plants = ["zero", "resid"] if n >= 200 else [("zero", "resid")[n % 2]]    # below 200 pixels a cut keeps one pixel: between the two
    for kind in plants:
        i = next(at)
        std[i] = 0.0
        if kind == "zero":
            pred[i] = gt[i]
    return pred.view(H, W, 3), gt.view(H, W, 3), std.view(H, W, 1)


def _eval_variants(variants):
    """(H, W, variant): every variant at one shape below, on and above the wave and on the workgroup size (they are what a
    batch of one shape stacks), the first alone elsewhere"""
    return [(H, W, v) for H, W in EVAL_SHAPES for v in (variants if (H, W) in ((7, 9), (8, 8), (5, 13), (16, 16)) else variants[:1])]


def _gt_u8(gt):
    """the 8-bit levels k of a ground truth on the 8-bit grid: gt == float32(k) / float32(255), bit for bit"""
    k = torch.round(gt * 255).to(torch.uint8)
    assert torch.equal(k.to(torch.float32) / 255, gt)
    return k.numpy()


def _permuted(tensors, H, W, seed):
    """the pixels in reverse order (every tied pair swaps) and in a seeded random order"""
    for perm in (torch.arange(H * W - 1, -1, -1), torch.randperm(H * W, generator=torch.Generator().manual_seed(seed))):
        yield [t.reshape(H * W, -1)[perm].reshape(t.shape) for t in tensors]


def _run_rgb(eu, pred, gt, std, dtype):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        d = eu.get_unc_metrics_rgb(None, 0, {"image": gt.to(dtype)}, {"rgb": pred.to(dtype), "rgb_std": std.to(dtype)}, None, None,
                                   min_rgb_std_for_nll=EVAL_MIN_RGB_STD)
    rec = _eval_record(d, "nll_rgb")
    rec["nll_abs_mean"] = np.float64(d["neg_log_prob"].abs().mean().item())
    return rec


def golden_eval_rgb(res):
    eu = _eval_module()
    names = []
    for H, W, variant in _eval_variants(("", "_b", "_c")):
        for seed in range(1000 + H * W + 100 * len(names), 1020 + H * W + 100 * len(names)):
            pred, gt, std = _rgb_case(H, W, seed, variant)
            r32, r64 = _run_rgb(eu, pred, gt, std, torch.float32), _run_rgb(eu, pred, gt, std, torch.float64)
            p64 = [_run_rgb(eu, *p, torch.float64) for p in _permuted((pred, gt, std), H, W, seed)]
            why = _eval_well_defined(r32, r64, p64, r64["nll_abs_mean"])
            if why is None:
                break
            print(f"  rgb {H}x{W}{variant} seed {seed}: {why}; reseeding")
        else:
            raise SystemExit(f"rgb {H}x{W}{variant}: no seed gives a well-defined case")
        names.append(f"{H}x{W}{variant}")
        tag = f"rgb_{names[-1]}"
        res.update({f"{tag}_pred": pred.numpy(), f"{tag}_gt_u8": _gt_u8(gt), f"{tag}_std": std.numpy()})
        _eval_pack(res, tag, r32, r64)
    res["rgb_cases"] = np.array(names)
    res["rgb_min_std"] = np.float64(EVAL_MIN_RGB_STD)


def _depth_case(H, W, seed, sparse=False, scale=2.5):
    """depths below 1e-3 and above max GT after scaling; GT == 0 pixels (most of them when `sparse`); a zero std"""
    g = torch.Generator().manual_seed(seed)
    n = H * W
    gt = 1.0 + 4.0 * torch.rand(n, generator=g)
    std = 0.4 + 2.0 * torch.rand(n, generator=g)
    depth = gt + std * torch.randn(n, generator=g)
    at = iter(torch.randperm(n, generator=g).tolist())
    depth[next(at)] = -1.0
    depth[next(at)] = 5e-4                                  # positive, below MIN_DEPTH
    depth[next(at)] = 100.0
    depth[next(at)] = float(gt.max()) + 0.5
    std[next(at)] = 0.0
    invalid = torch.rand(n, generator=g) < (0.7 if sparse else 0.08)
    invalid[[next(at) for _ in range(3)]] = True
    gt[invalid] = 0.0
    return (depth / scale).view(H, W, 1), (std / scale).view(H, W, 1), gt.view(H, W), scale


def _run_depth(eu, depth, std, gt, scale, dtype, min_std=EVAL_MIN_DEPTH_STD):
    import tempfile
    from pathlib import Path
    with tempfile.TemporaryDirectory() as tmp, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Path(tmp, "scale_parameters.txt").write_text(f"{scale}\n")
        np.save(os.path.join(tmp, "depth_gt_07.npy"), gt.to(dtype).numpy())
        plots = Path(tmp, "plots")
        plots.mkdir()
        d = eu.get_unc_metrics_depth(7, {"depth": depth.to(dtype), "depth_std": std.to(dtype)}, Path(tmp), plots,
                                     min_depth_std_for_nll=min_std)
    rec = _eval_record(d, "nll_depth")
    rec["nll_abs_mean"] = np.float64(d["neg_log_prob"][torch.as_tensor(gt > 0)].abs().mean().item())
    return rec


def golden_eval_depth(res):
    eu = _eval_module()
    names = []
    for H, W, variant in _eval_variants(("", "_b")) + [(15, 17, "_sparse")]:
        sparse = variant == "_sparse"
        for seed in range(2000 + H * W + 100 * len(names), 2020 + H * W + 100 * len(names)):
            depth, std, gt, scale = _depth_case(H, W, seed, sparse, 0.4 if variant == "_b" else 2.5)
            r32, r64 = _run_depth(eu, depth, std, gt, scale, torch.float32), _run_depth(eu, depth, std, gt, scale, torch.float64)
            p64 = [_run_depth(eu, *p, scale, torch.float64) for p in _permuted((depth, std, gt), H, W, seed)]
            why = _eval_well_defined(r32, r64, p64, r64["nll_abs_mean"])
            if why is None:
                break
            print(f"  depth {H}x{W}{variant} seed {seed}: {why}; reseeding")
        else:
            raise SystemExit(f"depth {H}x{W}{variant}: no seed gives a well-defined case")
        name = f"{H}x{W}{variant}"
        names.append(name)
        tag = f"depth_{name}"
        res.update({f"{tag}_depth": depth.numpy(), f"{tag}_std": std.numpy(), f"{tag}_gt": gt.numpy(), f"{tag}_scale": np.float64(scale)})
        _eval_pack(res, tag, r32, r64)
    res["depth_cases"] = np.array(names)
    res["depth_min_std"] = np.float64(EVAL_MIN_DEPTH_STD)


def golden_eval_frame(res):
    """get_average_uncertainty_metrics over a three-image fake pipeline: the datamanager's dataloader is a list, the model's
    psnr / ssim / lpips return the maximum, the sum and the minimum of the prediction they are handed (so the record shows
    which copy of the prediction each metric received), the plot functions record their arguments."""
    import tempfile
    from pathlib import Path
    eu = _eval_module()
    H, W, n_img, scale, min_depth_std = 12, 16, 3, 2.5, 2.0
    images = []
    for i in range(n_img):
        pred, gt, std = _rgb_case(H, W, 3000 + i)
        depth, dstd, dgt, _ = _depth_case(H, W, 3100 + i)
        images.append(dict(rgb=pred, rgb_std=std, image=gt, depth=depth, depth_std=dstd, depth_gt=dgt,
                           accumulation=torch.ones(H, W, 1)))
        res.update({f"frame_img{i}_{k}": v.numpy() for k, v in images[-1].items() if k != "image"})
        res[f"frame_img{i}_image_u8"] = _gt_u8(gt)
    res["frame_scale"], res["frame_min_rgb_std"], res["frame_min_depth_std"] = np.float64(scale), np.float64(EVAL_MIN_RGB_STD), np.float64(min_depth_std)
    inner, plot_errors, plot_auce, save_rgb = eu.get_image_metrics_and_images_unc, eu.plot_errors, eu.plot_auce_curves, eu.save_imgs_rgb
    prec, dtype = "f32", torch.float32                      # the frame is recorded in one precision: the reference as it runs
    per_image, plots = [], {}

    def record_image(*a, **kw):
        out = inner(*a, **kw)
        per_image.append((out[0], out[2]))
        return out

    def record_errors(ratio, err, err_by_var, err_type, scene_no, output_path, output):
        plots[f"errors_{output}_{err_type}_err"], plots[f"errors_{output}_{err_type}_err_var"] = err, err_by_var

    def record_auce(save_dir=None, output="rgb", **curves):
        plots.update({f"auce_{output}_{k}": v for k, v in curves.items()})

    eu.get_image_metrics_and_images_unc, eu.plot_errors, eu.plot_auce_curves = record_image, record_errors, record_auce
    eu.save_imgs_rgb = lambda **kw: None
    try:
        with tempfile.TemporaryDirectory() as tmp, warnings.catch_warnings():
            warnings.simplefilter("ignore")
            Path(tmp, "scale_parameters.txt").write_text(f"{scale}\n")
            for i, im in enumerate(images):
                np.save(os.path.join(tmp, "depth_gt_{:02d}.npy".format(i)), im["depth_gt"].to(dtype).numpy())
            model = SimpleNamespace(device=torch.device("cpu"), dataset_path=Path(tmp), output_path=Path(tmp, "out", "metrics.json"),
                                    psnr=lambda image, rgb: rgb.max(), ssim=lambda image, rgb: rgb.sum(),
                                    lpips=lambda image, rgb: rgb.min())
            loader = [(SimpleNamespace(height=torch.tensor(H), width=torch.tensor(W), index=i), {"image": im["image"].to(dtype)})
                      for i, im in enumerate(images)]
            pipeline = SimpleNamespace(model=model, datamanager=SimpleNamespace(fixed_indices_eval_dataloader=loader))
            outputs = [{k: im[k].to(dtype) for k in ("rgb", "rgb_std", "depth", "depth_std", "accumulation")} for im in images]
            avg = eu.get_average_uncertainty_metrics(pipeline, lambda camera: outputs[camera.index], eval_depth_unc=True,
                                                     eval_rgb_unc=True, save_rendered_images=True,
                                                     min_rgb_std_for_nll=EVAL_MIN_RGB_STD, min_depth_std_for_nll=min_depth_std)
    finally:
        eu.get_image_metrics_and_images_unc, eu.plot_errors, eu.plot_auce_curves, eu.save_imgs_rgb = inner, plot_errors, plot_auce, save_rgb
    assert len(per_image) == n_img and list(avg) == list(per_image[0][0])
    # scalars in the order of `_keys`; curves stacked by length (100 sparsification cuts, 99 coverages) under `_keys_<n>`
    res[f"frame_{prec}_keys"] = np.array(list(avg))
    # the two wall-clock keys keep their place in the key order and are stored as NaN: a rerun reproduces the file
    timed = lambda d: np.array([np.nan if k in ("num_rays_per_sec", "fps") else v for k, v in d.items()], dtype=np.float64)
    res[f"frame_{prec}_avg"] = timed(avg)
    for i, (md, curves) in enumerate(per_image):
        assert list(md) == list(avg) and list(curves) == list(per_image[0][1])
        res[f"frame_{prec}_img{i}"] = timed(md)
        _pack_by_length(res, f"frame_{prec}_curve_keys", f"frame_{prec}_img{i}_curves", curves)
    _pack_by_length(res, f"frame_{prec}_plot_keys", f"frame_{prec}_plot", plots)


def _pack_by_length(res, names_tag, tag, arrays):
    for n in (100, 99):
        names = [k for k, v in arrays.items() if len(v) == n]
        res[f"{names_tag}_{n}"] = np.array(names)
        res[f"{tag}_{n}"] = np.stack([np.asarray(arrays[k], dtype=np.float64) for k in names])
    assert all(len(v) in (100, 99) for v in arrays.values())


def golden_eval_rows():
    res = {}
    for fn in (golden_eval_rgb, golden_eval_depth, golden_eval_frame):
        fn(res)
    np.savez_compressed(os.path.join(OUT, "eval_rows.npz"), **res)


RECORDERS = (golden_create_mlp, golden_metrics, golden_sample_laplace, golden_get_weights, golden_ensemble,
             golden_mc_aggregate, golden_eval_configs, golden_splat_get_outputs, golden_nerf_model_glue,
             golden_field_glue, golden_eval_rows)


if __name__ == "__main__":
    if not os.path.isdir(REF):
        raise SystemExit("/root/reference is not mounted: golden vectors can only be regenerated in the build container")
    install_stubs()
    wanted = sys.argv[1:]                   # names of recorders (`golden_eval_rows`); none: all of them
    unknown = set(wanted) - {fn.__name__ for fn in RECORDERS}
    if unknown:
        raise SystemExit(f"no recorder named {sorted(unknown)}")
    for fn in RECORDERS:
        if wanted and fn.__name__ not in wanted:
            continue
        fn()
        print("wrote", fn.__name__)
