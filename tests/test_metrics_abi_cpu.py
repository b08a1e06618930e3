"""unerf_image_metrics on a machine without a GPU: the two symbols, every refusal of include/unerf.h (all of them come
before the first launch), and the host half of the fused path -- `metrics.finish_metrics` fed a row assembled here from
float64 torch sums must return what the torch path (`metrics.rgb_uncertainty_metrics`) returns.

`restate_row` is the float64 restatement of the row that tests/test_gpu_image_metrics.py holds the kernels to."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

ALPHAS = np.arange(start=0.01, stop=1.0, step=0.01)


def tables():
    from uncertainty_nerf_gs_amd import metrics as M
    return np.ascontiguousarray(M._RATIOS, dtype=np.float64), np.ascontiguousarray(M._norm_ppf(1.0 - ALPHAS / 2), dtype=np.float64)


def gauss11():
    d = np.arange(-5, 6, dtype=np.float64) / 1.5
    g = np.exp(-(d * d) / 2.0)
    return g / g.sum()


def ssim_sum_f64(p: torch.Tensor, t: torch.Tensor):
    """sum of the SSIM index over the (H-10) x (W-10) x C interior, unpadded 11x11 gaussian windows, float64 throughout;
    p (already clipped) / t [H,W,C] float32.  -> (sum, count)"""
    pf, tf = p.to(torch.float32), t.to(torch.float32)
    rng = max(float(pf.max() - pf.min()), float(tf.max() - tf.min()))      # float32 differences, as metrics.ssim takes them
    c1, c2 = (0.01 * rng) ** 2, (0.03 * rng) ** 2
    p64, t64 = pf.double().permute(2, 0, 1)[:, None], tf.double().permute(2, 0, 1)[:, None]        # [C,1,H,W]
    g = torch.from_numpy(gauss11())
    stack = torch.cat((p64, t64, p64 * p64, t64 * t64, p64 * t64))
    out = torch.nn.functional.conv2d(torch.nn.functional.conv2d(stack, g.view(1, 1, 1, 11)), g.view(1, 1, 11, 1))
    mu_p, mu_t, e_pp, e_tt, e_pt = out.split(p64.shape[0])
    s_pp, s_tt, s_pt = e_pp - mu_p ** 2, e_tt - mu_t ** 2, e_pt - mu_p * mu_t
    idx = ((2 * mu_p * mu_t + c1) * (2 * s_pt + c2)) / ((mu_p ** 2 + mu_t ** 2 + c1) * (s_pp + s_tt + c2))
    return float(idx.sum()), float(idx.numel())


def restate_row(pred, target, sigma, mask=None, clip=float("inf"), min_sigma=3e-2, ratios=None, z=None, image_hw=None):
    """The row of include/unerf.h (unerf_image_metrics), restated with torch on the CPU: float32 error definitions (channels
    added left to right), float64 sums, `torch.sort(stable=True)` for the defined order.  The error vectors, the NLL and the
    AUCE ratios take the prediction as given (scripts/eval_uncertainty.py:316); its copy clipped to `clip` feeds slot 6 (psnr),
    the minimum / maximum of slots 8 / 9 and the SSIM (:681-685; pinned by tests/golden/eval_rows.npz).  -> (row, extras)"""
    from uncertainty_nerf_gs_amd import metrics as M
    r0, z0 = tables()
    ratios = r0 if ratios is None else ratios
    z = z0 if z is None else z
    Cc = pred.shape[-1]
    p_raw = pred.detach().cpu().reshape(-1, Cc).float()
    t = target.detach().cpu().reshape(-1, Cc).float()
    s = sigma.detach().cpu().reshape(-1).float()
    if mask is not None:
        keep = mask.detach().cpu().reshape(-1).bool()
        p_raw, t, s = p_raw[keep], t[keep], s[keep]
    p = torch.clamp(p_raw, max=clip)
    n = s.numel()
    d = p_raw - t
    sq, ab = d[:, 0] * d[:, 0], d[:, 0].abs()
    for c in range(1, Cc):
        sq, ab = sq + d[:, c] * d[:, c], ab + d[:, c].abs()
    var = s * s
    p64, t64, s64 = p.double(), t.double(), s.double()
    d64 = t64 - p_raw.double()
    se = torch.clamp_min(s64, float(np.float32(min_sigma)))[:, None]
    nll_terms = d64 ** 2 / (2.0 * (se * se)) + torch.log(se) + 0.5 * math.log(2 * math.pi)
    r = d64.abs()
    sg = s64[:, None].expand_as(r)
    ratio = torch.where(sg > 0, r / sg, torch.where(r == 0, torch.zeros_like(r), torch.full_like(r, float("inf"))))
    counts = [float((ratio <= float(zk)).sum()) for zk in z]
    keep_k = [min(max(int((1.0 - rr) * float(n)), 0), n) for rr in ratios]

    def first_sums(values, order_key):
        order = torch.sort(order_key, stable=True).indices
        cs = torch.cat((torch.zeros(1, dtype=torch.float64), torch.cumsum(values[order].double(), 0)))
        return [float(cs[k]) for k in keep_k]

    fam = [first_sums(sq, sq), first_sums(ab, ab), first_sums(sq, var), first_sums(ab, var)]
    ssim_sum = ssim_cnt = 0.0
    if image_hw is not None and mask is None:
        H, W = image_hw
        ssim_sum, ssim_cnt = ssim_sum_f64(p.reshape(H, W, Cc), t.reshape(H, W, Cc))
    # nothing valid: the minima / maxima of an empty set, every sum and count 0
    p_mm = (float(p.min()), float(p.max())) if n else (float("inf"), float("-inf"))
    t_mm = (float(t.min()), float(t.max())) if n else (float("inf"), float("-inf"))
    row = M.metrics_row_from_sums(n, float(sq.double().sum()), float(ab.double().sum()), float(var.double().sum()),
                                  float(s64.sum()), float(((t64 - p64) ** 2).sum()), float(nll_terms.sum()),
                                  p_mm, t_mm, counts, fam, ssim_sum, ssim_cnt)
    return row, {"nll_abs_sum": float(nll_terms.abs().sum()), "n": n}


def edge_tables():
    """caller tables at their edges, 128 entries each (the maximum): ratios out of order with 0, 1, values outside [0, 1], a
    duplicate and one so small that keep_k is n_valid - 1; thresholds descending and out of order with duplicates, a zero,
    an infinity and a value below every float32 ratio"""
    ratios = np.concatenate(([0.5, 0.0, 1.0, 1.5, -0.25, 0.5, 0.999, 1e-9], np.linspace(0.01, 0.99, 120)))
    z = np.concatenate(([2.0, 0.0, np.inf, 1.0, 1.0, 1e-300], np.linspace(3.0, 0.01, 122)))
    assert ratios.size == z.size == 128
    return np.ascontiguousarray(ratios, dtype=np.float64), np.ascontiguousarray(z, dtype=np.float64)


# ---------------------------------------------------------------- the ABI ------------------------------------------

def test_symbols_are_exported_and_typed(lib):
    h = lib.load()
    for name in ("unerf_image_metrics_workspace_bytes", "unerf_image_metrics"):
        assert name in lib.SIGNATURES and getattr(h, name) is not None
    assert h.unerf_version() == 1420 == lib.ABI_VERSION                     # an additive change
    assert len(lib.SIGNATURES["unerf_image_metrics"][1]) == 19
    assert "unerf_metrics.hip" in lib.SOURCES
    hdr = open(lib.INCLUDE + "/unerf.h").read()
    for name, val in (("AUSE", lib.METRICS_AUSE), ("AUCE", lib.METRICS_AUCE), ("NLL", lib.METRICS_NLL), ("SSIM", lib.METRICS_SSIM),
                      ("AUCE_OFF", lib.METRICS_AUCE_OFF), ("AUSE_OFF", lib.METRICS_AUSE_OFF), ("ROW", lib.METRICS_ROW)):
        assert f"#define UNERF_METRICS_{name} {val}\n" in hdr
    assert lib.METRICS_AUSE_OFF + 4 * lib.METRICS_MAX_CUTS == lib.METRICS_ROW


def test_workspace_bytes_is_monotone(lib):
    h = lib.load()
    sizes = [h.unerf_image_metrics_workspace_bytes(n) for n in (0, 1, 255, 37 * 53, 4096, 4097, 256 * 256, 1080 * 1920, 1 << 24)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert sizes[-2] >= 28 * 1080 * 1920                                    # seven 32-bit arrays of n


def _call(h, n=100, C_=3, H=10, W=10, flags=7, pred=0x1000, target=0x1000, sigma=0x1000, mask=None, n_ratios=100, n_z=99,
          ws=0x1000, ws_bytes=None, out=0x1000, ratios=True, z=True):
    """fake (never dereferenced) device pointers: every refusal comes before the first launch"""
    r, zz = tables()
    dp = C.POINTER(C.c_double)
    if ws_bytes is None:
        ws_bytes = h.unerf_image_metrics_workspace_bytes(max(n, 0))
    return h.unerf_image_metrics(pred, target, sigma, mask, n, C_, H, W, float("inf"), 0.03, r.ctypes.data_as(dp) if ratios else None,
                                 n_ratios, zz.ctypes.data_as(dp) if z else None, n_z, flags, ws, ws_bytes, out, None)


@pytest.mark.parametrize("kw,needle", [
    (dict(pred=None), "null pointer"), (dict(target=None), "null pointer"), (dict(sigma=None), "null pointer"),
    (dict(out=None), "null pointer"), (dict(ws=None), "null pointer"),
    (dict(C_=0), "C = 0"), (dict(C_=5), "C = 5"),
    (dict(n=(1 << 31) // 3 + 1, ws_bytes=1 << 40), "2^31"), (dict(n=1 << 31, C_=1, ws_bytes=1 << 40), "2^31"),
    (dict(n_ratios=0), "n_ratios"), (dict(n_ratios=129), "n_ratios"), (dict(n_z=0), "n_z"), (dict(n_z=129), "n_z"),
    (dict(ratios=False), "n_ratios"), (dict(z=False), "n_z"),
    (dict(flags=8, n=176, H=11, W=16, mask=0x1000), "takes no mask"),
    (dict(flags=8, n=176, H=11, W=15), "H * W == n"),
    (dict(flags=15, n=160, H=10, W=16), "min(H, W) >= 11"),
    (dict(ws_bytes=1024), "workspace of 1024 bytes"),
    (dict(n=-1), "n = -1"),
])
def test_refusals_come_before_any_launch(lib, kw, needle):
    h = lib.load()
    assert _call(h, **kw) == -1
    assert needle in h.unerf_last_error().decode(), h.unerf_last_error().decode()


def test_zero_pixels_is_a_successful_no_op(lib):
    h = lib.load()
    assert _call(h, n=0, H=0, W=0, pred=None, target=None, sigma=None, ws=None, ws_bytes=0, out=None, flags=15) == 0


def test_cpu_tensors_are_refused(lib):
    from uncertainty_nerf_gs_amd import ops
    x = torch.zeros(4, 4, 3)
    with pytest.raises(lib.UnerfError, match="no CPU path"):
        ops.image_metrics(x, x, torch.ones(4, 4), nll_min_sigma=0.03, flags=lib.METRICS_NLL)


# ---------------------------------------------------------------- the host half ------------------------------------

def _case(H=37, W=53, seed=0):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(H, W, 3, generator=g)
    std = 0.02 + 0.2 * torch.rand(H, W, 1, generator=g)
    pred = torch.clamp(gt + std * torch.randn(H, W, 3, generator=g), 0, 1)
    return pred, std, gt


def test_finish_metrics_on_a_cpu_row_returns_what_the_torch_path_returns(lib):
    """The row comes from float64 torch sums over the float32 error vectors; the torch path sums the same vectors in
    float32 (mse, avg_var, nll: 1e-6 relative covers a float32 mean of 2000 values many times over) and sorts them with
    torch.sort (AUSE: 2e-6, the tolerance test_ause_matches_reference holds `ause` to).  psnr is float64 on both sides.
    `auce` tests t in [m - z s, m + z s] in numpy arithmetic, the row counts |t - m| / s <= z in float64: an element within
    rounding of an interval edge may fall either way; three of them per threshold move an integral by 3 / (n C)."""
    from uncertainty_nerf_gs_amd import metrics as M
    pred, std, gt = _case()
    ref = M.rgb_uncertainty_metrics(pred, std, gt, min_rgb_std_for_nll=3e-2)
    row, ex = restate_row(pred, gt, std, clip=1.0, min_sigma=3e-2, image_hw=(37, 53))
    md, curves = M.finish_metrics(row, 3, "rgb")
    assert abs(md["psnr"] - ref["psnr"]) <= 1e-9
    for et in ("mae", "mse", "rmse"):
        assert abs(md[f"rgb_ause_{et}"] - ref[f"ause_{et}"]) <= 2e-6, et
    assert abs(md["rgb_avg_var"] - ref["avg_var"]) <= 1e-6 * ref["avg_var"]
    assert abs(md["rgb_nll"] - ref["nll_rgb"]) <= 1e-6 * abs(ref["nll_rgb"]) + 1e-6
    edge = 3.0 / (ex["n"] * 3)
    assert abs(md["rgb_auc_abs_error"] - ref["auc_abs_error_values"]) <= edge
    assert abs(md["rgb_auc_neg_error"] - ref["auc_neg_error_values"]) <= edge
    assert abs(md["rgb_auc_length"] - ref["auc_length_values"]) <= 1e-6 * ref["auc_length_values"]
    assert abs(md["ssim"] - M.ssim(pred, gt)) <= 6e-5           # the float32 121-tap filter's distance from float64 (at most 5.5e-5)
    assert abs(md["rgb_rmse"] - math.sqrt(md["rgb_mse"])) <= 1e-15
    # the same keys and curve names as the torch path of the eval harness
    from uncertainty_nerf_gs_amd import eval as E
    md0, curves0 = E.image_metrics_unc({"rgb": pred, "rgb_std": std}, gt)
    assert set(md) == set(md0) and set(curves) == set(curves0)
    for k in curves0:
        assert np.asarray(curves[k]).shape == np.asarray(curves0[k]).shape, k
        assert np.asarray(curves[k]).dtype == np.asarray(curves0[k]).dtype, k
    np.testing.assert_array_equal(curves["rgb_all_auce_coverage_values"], curves0["rgb_all_auce_coverage_values"])
    for et in ("mae", "mse", "rmse"):
        np.testing.assert_allclose(curves[f"rgb_all_ause_{et}"], curves0[f"rgb_all_ause_{et}"], rtol=0, atol=2e-6)
        np.testing.assert_allclose(curves[f"rgb_all_var_ause_{et}"], curves0[f"rgb_all_var_ause_{et}"], rtol=0, atol=2e-6)


def test_finish_metrics_raises_on_non_finite_inputs(lib):
    from uncertainty_nerf_gs_amd import metrics as M
    pred, std, gt = _case(16, 16)
    row, _ = restate_row(pred, gt, std, clip=1.0)
    row[1] = 2.0
    with pytest.raises(ValueError, match="non-finite"):
        M.finish_metrics(row, 3)


# ---------------------------------------------------------------- the restatement itself ---------------------------

@pytest.mark.parametrize("n,Cc,masked,which", [(1, 3, False, "edge"), (2, 1, False, "edge"), (37, 2, True, "edge"), (300, 3, True, "edge"),
                                               (300, 4, False, "edge"), (299, 3, True, "single"), (300, 3, False, "default")])
def test_restate_row_handles_caller_tables_like_a_brute_force_loop(lib, n, Cc, masked, which):
    """`restate_row` (torch.sort, cumsum, vectorised comparisons) against plain loops at the table edges the GPU tests lean
    on: per ratio int((1 - r) n) clamped to [0, n] and the first k of a Python-sorted list of (value, index) pairs, per
    threshold a count element by element.  The error vectors are numpy float32 here (IEEE, channels left to right), the
    sums math.fsum (exact): 1e-12 relative covers a float64 cumsum of 300 non-negative terms (300 2^-53 = 3.4e-14);
    counts, n_valid, minima and maxima are equal."""
    g = torch.Generator().manual_seed(100 * n + Cc)
    gt = torch.rand(n, Cc, generator=g)
    std = 0.02 + 0.2 * torch.rand(n, generator=g)
    pred = gt + std[:, None] * torch.randn(n, Cc, generator=g) + 0.05
    std[3:60:7] = 0.0                                                      # sigma == 0 with a residual: ratio +inf, var ties
    std[5:80:9] = 0.0
    pred[5:80:9] = gt[5:80:9]                                              # sigma == 0 without: ratio 0, sq / ab ties
    pred[100:140] = gt[100:140] + 0.0625                                   # equal errors across several cuts
    mask = (torch.rand(n, generator=g) > 0.3) if masked else None
    ratios, z = {"edge": edge_tables(), "single": (np.array([0.5]), np.array([1.0])), "default": tables()}[which]
    clip = 1.0
    row, ex = restate_row(pred, gt, std, mask, clip=clip, min_sigma=3e-2, ratios=ratios, z=z)

    keep = np.ones(n, bool) if mask is None else mask.numpy()
    p_raw = pred.numpy()[keep]                                              # what the errors and the ratios take
    p = np.minimum(p_raw, np.float32(clip))                                 # what slot 6 and the minimum / maximum take
    t, s = gt.numpy()[keep], std.numpy()[keep]
    nv = int(keep.sum())
    assert p.dtype == t.dtype == s.dtype == np.float32 and row[0] == nv == ex["n"] and row[1] == 0
    assert nv < 100 or p_raw.max() > clip                                   # the two readings differ on these pixels
    sq, ab = np.zeros(nv, np.float32), np.zeros(nv, np.float32)
    for c in range(Cc):
        d = p_raw[:, c] - t[:, c]
        sq, ab = sq + d * d, ab + np.abs(d)
    var = s * s
    assert sq.dtype == ab.dtype == var.dtype == np.float32
    by = {"sq": sorted((float(v), i) for i, v in enumerate(sq)), "ab": sorted((float(v), i) for i, v in enumerate(ab)),
          "var": sorted((float(v), i) for i, v in enumerate(var))}
    from uncertainty_nerf_gs_amd import lib as L
    s0 = L.METRICS_AUSE_OFF
    for k, r in enumerate(ratios):
        kk = min(max(int((1 - r) * nv), 0), nv)
        want = (math.fsum(v for v, _ in by["sq"][:kk]), math.fsum(v for v, _ in by["ab"][:kk]),
                math.fsum(float(sq[i]) for _, i in by["var"][:kk]), math.fsum(float(ab[i]) for _, i in by["var"][:kk]))
        for f in range(4):
            got = row[s0 + 128 * f + k]
            assert abs(got - want[f]) <= 1e-12 * want[f], (k, r, kk, f, got, want[f])
            assert want[f] != 0 or got == 0
    a0 = L.METRICS_AUCE_OFF
    for k, zk in enumerate(z):
        cnt = 0
        for i in range(nv):
            for c in range(Cc):
                res, sg = abs(float(t[i, c]) - float(p_raw[i, c])), float(s[i])
                ratio = res / sg if sg > 0 else (0.0 if res == 0 else math.inf)
                cnt += ratio <= float(zk)
        assert row[a0 + k] == cnt, (k, zk)
    assert np.all(row[a0 + len(z):s0] == 0)
    for f in range(4):
        assert np.all(row[s0 + 128 * f + len(ratios):s0 + 128 * (f + 1)] == 0)
    if which == "edge" and nv:                                             # the edges are where they are meant to be
        fam0 = row[s0:s0 + 128]
        total = math.fsum(float(v) for v in sq)
        assert fam0[2] == fam0[3] == 0.0 and abs(fam0[1] - total) <= 1e-12 * total and fam0[1] == fam0[4]
        assert row[a0 + 2] == nv * Cc and row[a0 + 3] == row[a0 + 4] and row[a0 + 5] == row[a0 + 1]
    assert (row[8], row[9], row[10], row[11]) == (float(p.min()), float(p.max()), float(t.min()), float(t.max()))
    sq64 = [(float(a) - float(b)) ** 2 for a, b in zip(t.reshape(-1), p.reshape(-1))]
    for j, v in ((2, sq), (3, ab), (4, var), (5, s), (6, sq64)):
        w = math.fsum(float(x) for x in v)
        assert abs(row[j] - w) <= 1e-12 * w, j


def test_restate_row_of_nothing_valid(lib):
    """an all-zero mask: counts and sums 0, minima +inf, maxima -inf (the header: "+-inf when nothing is valid")"""
    from uncertainty_nerf_gs_amd import metrics as M
    pred, std, gt = _case(5, 7)
    row, ex = restate_row(pred, gt, std, torch.zeros(5, 7, dtype=torch.bool), clip=1.0)
    assert ex["n"] == 0 and tuple(row[8:12]) == (math.inf, -math.inf, math.inf, -math.inf)
    assert np.all(np.delete(row, [8, 9, 10, 11]) == 0)
    with pytest.raises(ValueError, match="no valid pixel"):
        M.finish_metrics(row, 3)
