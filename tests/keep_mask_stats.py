"""Shared by tests/test_keep_masks_cpu.py and tests/test_gpu_keep_masks.py: the inputs and the three statistics of the
"counter generator vs torch Bernoulli" comparison of the rendered MC-dropout uncertainty.

Two groups of n = 64 frames of per-pixel rgb_std, one per mask source.  Under H0 (both sources make i.i.d.
Bernoulli(1 - p) keep masks) the groups are two samples of the same distribution, and the gates are quantiles of the
null distributions -- not measurements of the code under test:
  * Welch |t| of the per-seed FRAME MEANS <= 4: two-sided p ~ 1e-4 at ~126 degrees of freedom;
  * largest per-pixel two-sample |z| <= 4.5: Bonferroni-corrected p ~ 7e-4 over the 96 pixels;
  * variance ratio of the per-seed frame means inside [1/2.4, 2.4]: F(63, 63) at two-sided p ~ 1e-3."""
import numpy as np
import torch

from oracle import nerf_oracle as O

N_SEEDS, K, P_DROP, SITES = 64, 8, 0.2, 5
H, W, FOCAL, THETA = 8, 12, 30.0, 0.3
T_GATE, Z_GATE, F_GATE = 4.0, 4.5, 2.4


def scene_tensors():
    from uncertainty_nerf_gs_amd import synthetic
    return synthetic.make_scene_tensors(seed=0, kind="mcdropout", log2T=14, prop_log2T=12)


def camera():
    from uncertainty_nerf_gs_amd import synthetic
    return synthetic.orbit_c2w(THETA), dict(fx=FOCAL, fy=FOCAL, cx=W / 2, cy=H / 2, H=H, W=W)


def oracle_rays():
    c2w, cam = camera()
    o, d, _ = O.generate_rays(c2w, cam["fx"], cam["fy"], cam["cx"], cam["cy"], H, W)
    return o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()


def torch_keep_masks(seed: int, Kp: int, rays: int, S: int, chunk: int, sites: int, p: float):
    """[site][k] -> bool [rays * S, 64] (None: site without Dropout), drawn by the product's host function from a CPU
    generator seeded `seed` -- the reference's draw order (pass, chunk, module)"""
    from uncertainty_nerf_gs_amd import models
    g = torch.Generator().manual_seed(seed)
    out = [[[] for _ in range(Kp)] if (sites >> i) & 1 else None for i in range(3)]
    for k, start, n, i, keep in models.iter_torch_keep_draws(Kp, rays, S, chunk, sites, p, g):
        out[i][k].append(keep)
    return [None if s is None else [torch.cat(c) for c in s] for s in out]


def oracle_rgb_std(sc, o, d, sampled, masks_of_pass) -> torch.Tensor:
    """per-pixel rgb_std [R] of K oracle passes: unbiased std over the passes, mean over the channels
    (mcdropout_models.py:121-126); masks_of_pass(k) -> (keep_trunk, keep_head1)"""
    eb, wl, bl = sampled
    rgbs = []
    for k in range(K):
        kt, kh = masks_of_pass(k)
        density, rgb = O.mcdropout_field(o, d, eb, sc.field, kt, kh, P_DROP)
        rgbs.append(O.nerfacto_pass_outputs(sc, o, d, eb, wl, bl, density, rgb)["rgb"])
    return torch.stack(rgbs).std(dim=0).mean(dim=-1)


def statistics(a, b):
    """a, b [n, pixels] -> (Welch |t| of the frame means, max per-pixel |z|, variance ratio of the frame means)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = a.shape[0], b.shape[0]
    ma, mb = a.mean(axis=1), b.mean(axis=1)
    t = abs(ma.mean() - mb.mean()) / np.sqrt(ma.var(ddof=1) / na + mb.var(ddof=1) / nb)
    se = np.sqrt(a.var(axis=0, ddof=1) / na + b.var(axis=0, ddof=1) / nb)
    z = np.abs(a.mean(axis=0) - b.mean(axis=0)) / np.maximum(se, 1e-30)
    return float(t), float(z.max()), float(ma.var(ddof=1) / mb.var(ddof=1))


def report_and_gate(tag, a, b):
    t, z, f = statistics(a, b)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    se = np.sqrt(a.mean(axis=1).var(ddof=1) / a.shape[0] + b.mean(axis=1).var(ddof=1) / b.shape[0])
    print(f"[{tag}] Welch |t| = {t:.3f} (gate {T_GATE}), max per-pixel |z| = {z:.3f} (gate {Z_GATE}), "
          f"variance ratio = {f:.3f} (gate [{1 / F_GATE:.3f}, {F_GATE}]); mean rgb_std A = {a.mean():.6e}, B = {b.mean():.6e}, "
          f"standard error of the difference = {se:.3e} ({se / a.mean():.3%} of the mean)")
    assert t <= T_GATE, f"{tag}: Welch |t| = {t:.3f} > {T_GATE}"
    assert z <= Z_GATE, f"{tag}: max per-pixel |z| = {z:.3f} > {Z_GATE}"
    assert 1 / F_GATE <= f <= F_GATE, f"{tag}: variance ratio {f:.3f} outside [{1 / F_GATE:.3f}, {F_GATE}]"
    return t, z, f
