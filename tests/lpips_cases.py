"""Shared cases of the LPIPS tests (tests/test_lpips_cpu.py, tests/test_gpu_lpips.py): fixed seeds, the synthetic
weights, image pairs, a direct numpy loop statement of the network, and the derived error bounds.  No pretrained AlexNet
weights exist offline: every test runs on synthetic.make_lpips_weights."""
import functools

import numpy as np
import torch

WEIGHT_SEED = 11
IMAGE_SEED = 23
# (kernel size, stride, padding) of the five convolutions; a 3 / 2 max-pool sits in front of the second and the third
GEOMETRY = ((11, 4, 2), (5, 1, 2), (3, 1, 1), (3, 1, 1), (3, 1, 1))
E2E_SIZES = ((31, 31), (31, 47), (35, 33), (64, 48))
E2E_BATCHES = (1, 3, 16)


@functools.lru_cache(maxsize=None)
def weights(seed=WEIGHT_SEED):
    from uncertainty_nerf_gs_amd import checkpoints, synthetic
    w = checkpoints.lpips_weights_from_state_dict(synthetic.make_lpips_weights(seed))
    assert w is not None
    return w


def image_pair(H, W, B=None, seed=IMAGE_SEED):
    """(prediction, target) [H,W,3] (or [B,H,W,3]) float32: a smooth target in [0, 1] and a noisy prediction whose values
    reach past 1 (the harness clips them) and never below 0"""
    g = torch.Generator().manual_seed(seed + 1000 * H + W + 7919 * (B or 0))
    shape = (H, W, 3) if B is None else (B, H, W, 3)
    target = torch.rand(shape, generator=g)
    pred = torch.clamp(target + 0.15 * torch.randn(shape, generator=g), 0.0, 1.1)
    return pred, target


def gamma(m, u):
    """the standard rounding-error constant gamma_m = m u / (1 - m u)"""
    return m * u / (1.0 - m * u)


# ---- the loop statement: explicit numpy loops over output pixels and taps, no conv2d -----------------------------------

def _conv_loops(x, w, b, stride, pad):
    """x [C_in, H, W], w [C_out, C_in, k, k], b [C_out] float64 -> [C_out, H_out, W_out]; a tap outside the image adds nothing"""
    Co, Ci, k, _ = w.shape
    _, H, W = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = np.zeros((Co, Ho, Wo))
    for oy in range(Ho):
        for ox in range(Wo):
            acc = b.copy()
            for ky in range(k):
                iy = oy * stride - pad + ky
                if iy < 0 or iy >= H:
                    continue
                for kx in range(k):
                    ix = ox * stride - pad + kx
                    if ix < 0 or ix >= W:
                        continue
                    for c in range(Ci):
                        acc = acc + w[:, c, ky, kx] * x[c, iy, ix]
            out[:, oy, ox] = acc
    return out


def _pool_loops(x):
    C, H, W = x.shape
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    out = np.zeros((C, Ho, Wo))
    for oy in range(Ho):
        for ox in range(Wo):
            out[:, oy, ox] = x[:, 2 * oy:2 * oy + 3, 2 * ox:2 * ox + 3].reshape(C, 9).max(axis=1)
    return out


def loop_features(image, w):
    """image [H,W,3] in [0, 1] (numpy float64) -> the five taps [C_l, h_l, w_l]"""
    x = 2.0 * np.transpose(image, (2, 0, 1)) - 1.0
    x = (x - w.shift.double().numpy()[:, None, None]) / w.scale.double().numpy()[:, None, None]
    taps = []
    for l, (k, stride, pad) in enumerate(GEOMETRY):
        if l in (1, 2):
            x = _pool_loops(x)
        cw, cb = w.convs[l]
        x = np.maximum(_conv_loops(x, cw.double().numpy(), cb.double().numpy(), stride, pad), 0.0)
        taps.append(x)
    return taps


def loop_lpips(pred, target, w):
    """the whole metric for one [H,W,3] pair in float64, loops only"""
    from uncertainty_nerf_gs_amd import metrics as M
    p = np.minimum(pred.double().numpy(), 1.0)
    t = target.double().numpy()
    total = 0.0
    for f0, f1, lin in zip(loop_features(p, w), loop_features(t, w), w.lins):
        lin = lin.double().numpy()
        C, h, ww = f0.shape
        s = 0.0
        for y in range(h):
            for x in range(ww):
                a, b = f0[:, y, x], f1[:, y, x]
                a = a / np.sqrt(M.LPIPS_NORM_EPS + np.sum(a * a))
                b = b / np.sqrt(M.LPIPS_NORM_EPS + np.sum(b * b))
                s += np.sum(lin * (a - b) ** 2)
        total += s / (h * ww)
    return total


# ---- the end-to-end yardstick: float64 and float32 host values of every case, computed once ----------------------------

@functools.lru_cache(maxsize=None)
def e2e_reference():
    """{(H, W, B): (pred, target, float64 values [B], float32-on-the-CPU values [B])} and the largest |float32 - float64|
    over the whole case set: the reference's own fp32 arithmetic against the exact statement"""
    from uncertainty_nerf_gs_amd import metrics as M
    cases, gap = {}, 0.0
    for H, W in E2E_SIZES:
        for B in E2E_BATCHES:
            pred, target = image_pair(H, W, B)
            v64 = M.lpips_per_image(pred, target, weights(), torch.float64).numpy()
            v32 = M.lpips_per_image(pred, target, weights(), torch.float32).double().numpy()
            gap = max(gap, float(np.abs(v32 - v64).max()))
            cases[(H, W, B)] = (pred, target, v64, v32)
    return cases, gap
