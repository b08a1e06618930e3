"""Shared by tests/test_eval_images_cpu.py and tests/test_gpu_eval_images.py: seeded inputs of the rendered-image pack
(eval.pack_eval_images on the host, unerf_eval_images_batch on the device), the same images by the route the reference
takes (matplotlib's `jet` on the float image, then the float -> uint8 rule), and a PNG decoder.

The numpy DEFINITION both suites hold the code to is `eval.pack_eval_images` itself; `matplotlib_route` below is the
independent restatement it is pinned against where matplotlib is installed."""
import struct
import zlib

import numpy as np

UNC_MIN, UNC_MAX = 0.05, 0.6
PLANES = ("gt", "pred", "err", "std")
CHANNELS = {"gt": 3, "pred": 3, "err": 1, "std": 3}
_F = np.float32


def q8(x):
    """(uint8)(clip(x, 0, 1) * 255 + 0.5) in float64, truncating; NaN -> 0"""
    with np.errstate(invalid="ignore"):
        v = np.clip(np.asarray(x, dtype=np.float64), 0.0, 1.0) * 255.0 + 0.5
    return np.where(np.isnan(v), 0.0, v).astype(np.uint8)


def _base(H, W, seed):
    g = np.random.default_rng(seed)
    gt = g.random((H, W, 3), dtype=_F)
    pred = (gt + _F(0.08) * g.standard_normal((H, W, 3), dtype=_F)).astype(_F)
    return g, gt, pred


def value_case(H, W, seed=0):
    """one image (H W >= 40) with the values where a byte can go wrong -> (pred, gt, std) float32:
    pred below 0 and above 1; pred and gt at 0.5, where x * 255 + 0.5 is exactly 128, and one float32 to either side; the
    other (m + 0.5) / 255 rounded to float32; a channel sum of exactly 1 and one float32 under and over it; std exactly
    UNC_MIN and exactly UNC_MAX, below and above them, +inf; a NaN std pixel and a NaN pred pixel."""
    assert H * W >= 40
    g, gt, pred = _base(H, W, seed)
    std = (_F(0.02) + _F(0.7) * g.random((H, W), dtype=_F)).astype(_F)
    p, t, s = pred.reshape(-1, 3), gt.reshape(-1, 3), std.reshape(-1)
    half = _F(0.5)
    p[1], p[2] = (-0.25, 1.75, -1e-8), (1.0, 0.0, 1.0000001)
    p[3] = (half, np.nextafter(half, _F(0)), np.nextafter(half, _F(1)))
    t[4] = (half, np.nextafter(half, _F(0)), np.nextafter(half, _F(1)))
    ms = np.array([0, 1, 63, 127, 200, 254], dtype=np.float64)
    p[5], p[6] = ((ms[:3] + 0.5) / 255.0).astype(_F), ((ms[3:] + 0.5) / 255.0).astype(_F)
    t[7], t[8] = p[6], p[5]
    for k, third in ((9, half), (10, np.nextafter(half, _F(0))), (11, np.nextafter(half, _F(1)))):
        t[k] = (0.0, 0.5, 0.25)                              # |d| = 0.25, 0.25, third: the sum is 1, just under, just over
        p[k] = (0.25, 0.25, _F(0.25) + third)
    p[12] = t[12]                                            # no error at all
    p[13] = (np.nan, 0.3, 0.4)
    s[14], s[15] = _F(UNC_MIN), _F(UNC_MAX)
    s[16], s[17] = np.nextafter(_F(UNC_MIN), _F(0)), np.nextafter(_F(UNC_MAX), _F(1))
    s[18], s[19], s[20], s[21] = 0.0, 5.0, np.inf, -0.3
    s[22] = np.nan
    return pred, gt, std


def range_stack(B, H, W, seed=0):
    """B images whose std stays strictly inside (UNC_MIN, UNC_MAX), so nothing is clipped and each image's own minimum and
    maximum decide its colours: the minimum sits in the image's FIRST pixel and the maximum in its LAST; image 0 holds the
    largest std of the stack and image 1 (if there is one) the smallest, so a range that leaks from one image into another
    changes bytes.  With room (H W >= 8) a NaN std pixel sits in the middle.  -> (pred, gt, std) [B, H, W, 3] / [B, H, W]"""
    preds, gts, stds = [], [], []
    for b in range(B):
        g, gt, pred = _base(H, W, 1000 * seed + b)
        lo = _F(0.07) if b == 1 else _F(0.12 + 0.004 * b)
        hi = _F(0.57) if b == 0 else _F(0.50 - 0.004 * b)
        std = (lo + (hi - lo) * (_F(0.05) + _F(0.9) * g.random((H, W), dtype=_F))).astype(_F)
        s = std.reshape(-1)
        s[0] = lo
        if s.size > 1:
            s[-1] = hi
        if s.size >= 8:
            s[s.size // 2] = np.nan
        preds.append(pred), gts.append(gt), stds.append(std)
    return np.stack(preds), np.stack(gts), np.stack(stds)


def matplotlib_route(pred, gt, std, unc_min, unc_max):
    """the four images as scripts/eval_uncertainty.py:209-303 makes them -- torch.clip((std - min) / |max - min|, 0, 1) in
    float32, media.to_rgb's normalisation in float64, matplotlib's jet called on the FLOAT image, [..., :3], then q8"""
    import matplotlib
    lo, span = _F(min(unc_min, unc_max)), _F(abs(unc_max - unc_min))
    with np.errstate(invalid="ignore"):
        d = np.abs(pred - gt)
        err = np.clip((d[..., 0] + d[..., 1]) + d[..., 2], 0, 1)
        s = np.clip((std - lo) / span, _F(0), _F(1))
    vmin = np.amin(np.where(np.isfinite(s), s, np.inf)).astype(np.float64)
    vmax = np.amax(np.where(np.isfinite(s), s, -np.inf)).astype(np.float64)
    a = (s.astype(np.float64) - vmin) / (vmax - vmin + np.finfo(float).eps)
    rgb = matplotlib.colormaps["jet"](a)[..., :3]
    return {"gt": q8(gt), "pred": q8(pred), "err": q8(err), "std": q8(rgb)}, float(np.nanmax(a))


def decode_png(path):
    """an 8-bit grey or RGB PNG whose rows all use filter type 0 -> uint8 [H, W] or [H, W, 3]; checks the signature, the
    chunk order and every CRC"""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(raw):
        (size,), tag = struct.unpack(">I", raw[pos:pos + 4]), raw[pos + 4:pos + 8]
        data = raw[pos + 8:pos + 8 + size]
        assert struct.unpack(">I", raw[pos + 8 + size:pos + 12 + size])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF, tag
        chunks.append((tag, data))
        pos += 12 + size
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[2][1] == b""
    W, H, depth, color, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and color in (0, 2)
    ch = 3 if color == 2 else 1
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(H, 1 + W * ch)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape((H, W, 3) if ch == 3 else (H, W)).copy()
