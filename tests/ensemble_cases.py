"""Shared by test_ensemble_batch_cpu.py and test_gpu_ensemble_batch.py: the torch statement of an ensemble.reduce_plan (the
`reduce_fn` of aggregate_batch / aggregate_distributed_batch on the CPU) and the member dictionaries the tests aggregate."""
import torch

from conftest import golden


def torch_moments(x):
    return x.mean(dim=0), x.var(dim=0)


def torch_reduce(views, plan):
    """what unerf_ensemble_reduce computes, in the torch operations of ensemble.aggregate / _finish"""
    res = []
    for view in views:
        mom = {k: torch_moments(torch.stack(list(srcs), dim=0).contiguous()) for k, srcs in view.items()}
        epi = lambda k: mom[k][1].mean(dim=-1).unsqueeze(-1)
        alea = lambda k: mom[k + "_var"][0].mean(dim=-1).unsqueeze(-1)
        stat = {"mean": lambda k: mom[k][0], "var": lambda k: mom[k][1], "var_cmean": epi, "alea_cmean": alea,
                "epi_plus_alea": lambda k: epi(k) + alea(k), "sqrt_epi_plus_alea": lambda k: (epi(k) + alea(k)).sqrt(),
                "std_cmean": lambda k: mom[k][1].sqrt().mean(dim=-1).unsqueeze(-1)}
        res.append({name: stat[s](k).contiguous() for name, s, k in plan})
    return res


def golden_members(tag, count):
    g = golden("ensemble.npz")
    return [{k[len(f"{tag}_in{i}_"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"{tag}_in{i}_")}
            for i in range(count)]


def golden_expected(tag):
    g = golden("ensemble.npz")
    return {k[len(f"{tag}_out_"):]: g[k] for k in g.files if k.startswith(f"{tag}_out_")}


def splat_members(M=3, H=5, W=7, seed=4):
    """active-splatfacto member dicts (activesplatfacto_model.py:359-367): images plus the [3] `background`; the values
    test_distributed_cpu.py aggregates"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(M):
        unc = torch.rand(H, W, 1, generator=g)
        dv = torch.rand(H, W, 1, generator=g)
        out.append({"rgb": torch.rand(H, W, 3, generator=g), "depth": torch.rand(H, W, 1, generator=g) * 4,
                    "accumulation": torch.rand(H, W, 1, generator=g), "background": torch.tensor([0.1490, 0.1647, 0.2157]),
                    "uncertainty": unc, "rgb_var": unc ** 2, "rgb_std": unc, "depth_var": dv, "depth_std": dv.sqrt()})
    return out


def nerf_members(kind, M, H, W, seed):
    """synthetic nerfacto member dicts of H x W pixels: kind "plain" (rgb / accumulation / depth / expected_depth) or
    "alea" (the active-nerfacto key order, activenerfacto_model.py:117-127)"""
    g = torch.Generator().manual_seed(seed)
    r = lambda c, s=1.0: torch.rand(H, W, c, generator=g) * s
    out = []
    for _ in range(M):
        if kind == "plain":
            out.append({"rgb": r(3), "accumulation": r(1), "depth": r(1, 4.0), "expected_depth": r(1, 4.0)})
        else:
            rv, dv = r(3, 0.1), r(1, 0.1)
            out.append({"rgb": r(3), "accumulation": r(1), "depth": r(1, 4.0), "rgb_var": rv, "rgb_std": rv.sqrt(),
                        "depth_var": dv, "depth_std": dv.sqrt()})
    return out
