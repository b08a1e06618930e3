"""unerf_image_metrics_batch on a machine without a GPU: the two symbols, the workspace size, every refusal of
include/unerf.h (all of them come before the first launch), and the plumbing of the eval harness's batched metric stage
(`eval.image_metrics_unc_batch` / `depth_metrics_unc_batch`, `metric_batch=` of get_average_uncertainty_metrics) with
`ops.image_metrics` / `ops.image_metrics_batch` replaced by stubs that build their rows from `restate_row` of
tests/test_metrics_abi_cpu.py on CPU tensors: what is held here is which call scores which images with which flags and
masks, and that the three ways through the harness return the same numbers; the kernels' rows are held on the GPU
(tests/test_gpu_image_metrics_batch.py)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_metrics_abi_cpu as R

TIMING_KEYS = ("num_rays_per_sec", "fps", "render_rays_per_sec")


# ---------------------------------------------------------------- the ABI ------------------------------------------

def test_symbols_are_exported_and_typed(lib):
    h = lib.load()
    for name in ("unerf_image_metrics_batch_workspace_bytes", "unerf_image_metrics_batch"):
        assert name in lib.SIGNATURES and getattr(h, name) is not None
    assert len(lib.SIGNATURES["unerf_image_metrics_batch"][1]) == 20
    assert len(lib.SIGNATURES["unerf_image_metrics_batch_workspace_bytes"][1]) == 2
    assert h.unerf_version() == lib.ABI_VERSION == 1420                     # an additive change
    hdr = open(lib.INCLUDE + "/unerf.h").read()
    assert "#define UNERF_METRICS_MAX_IMAGES 64\n" in hdr and lib.METRICS_MAX_IMAGES == 64


def test_workspace_bytes(lib):
    h = lib.load()
    ns, Bs = (0, 1, 4096, 4097, 256 * 256, 1080 * 1920), (1, 2, 16, 64)
    size = {(n, B): h.unerf_image_metrics_batch_workspace_bytes(n, B) for n in ns for B in Bs}
    for n in ns:
        assert size[n, 1] >= h.unerf_image_metrics_workspace_bytes(n)
        for B in Bs:
            assert size[n, B] >= 28 * n * B and size[n, B] > 0              # seven 32-bit arrays of n per image
        assert all(size[n, a] <= size[n, b] for a, b in zip(Bs, Bs[1:]))
    for B in Bs:
        assert all(size[a, B] <= size[b, B] for a, b in zip(ns, ns[1:]))


def _call(h, n=100, B=2, C_=3, H=10, W=10, flags=7, pred=0x1000, target=0x1000, sigma=0x1000, mask=None, n_ratios=100, n_z=99,
          ws=0x1000, ws_bytes=None, out=0x1000, ratios=True, z=True):
    """fake (never dereferenced) device pointers: every refusal comes before the first launch"""
    r, zz = R.tables()
    dp = C.POINTER(C.c_double)
    if ws_bytes is None:
        ws_bytes = h.unerf_image_metrics_batch_workspace_bytes(max(n, 0), B)
    return h.unerf_image_metrics_batch(pred, target, sigma, mask, n, B, C_, H, W, float("inf"), 0.03,
                                       r.ctypes.data_as(dp) if ratios else None, n_ratios, zz.ctypes.data_as(dp) if z else None, n_z,
                                       flags, ws, ws_bytes, out, None)


@pytest.mark.parametrize("kw,needle", [
    (dict(B=0), "B = 0"), (dict(B=65), "B = 65"), (dict(B=-1), "B = -1"),
    (dict(pred=None), "null pointer"), (dict(target=None), "null pointer"), (dict(sigma=None), "null pointer"),
    (dict(out=None), "null pointer"), (dict(ws=None), "null pointer"),
    (dict(C_=0), "C = 0"), (dict(C_=5), "C = 5"),
    (dict(n=(1 << 31) // 3 + 1, ws_bytes=1 << 44), "2^31"), (dict(n=1 << 31, C_=1, ws_bytes=1 << 44), "2^31"),
    (dict(n_ratios=0), "n_ratios"), (dict(n_ratios=129), "n_ratios"), (dict(n_z=0), "n_z"), (dict(n_z=129), "n_z"),
    (dict(ratios=False), "n_ratios"), (dict(z=False), "n_z"),
    (dict(flags=8, n=176, H=11, W=16, mask=0x1000), "takes no mask"),
    (dict(flags=8, n=176, H=11, W=15), "H * W == n"),
    (dict(flags=15, n=160, H=10, W=16), "min(H, W) >= 11"),
    (dict(n=-1), "n = -1"),
    (dict(ws=0x1004), "8-byte aligned"), (dict(out=0x1004), "8-byte aligned"),
])
def test_refusals_come_before_any_launch(lib, kw, needle):
    h = lib.load()
    assert _call(h, **kw) == -1
    msg = h.unerf_last_error().decode()
    assert needle in msg and msg.startswith("image_metrics_batch:"), msg


@pytest.mark.parametrize("n,B", [(100, 2), (4097, 16), (100, 64)])
def test_a_workspace_one_byte_short_is_refused_and_names_the_size_function(lib, n, B):
    h = lib.load()
    need = h.unerf_image_metrics_batch_workspace_bytes(n, B)
    assert _call(h, n=n, B=B, ws_bytes=need - 1) == -1
    msg = h.unerf_last_error().decode()
    assert f"workspace of {need - 1} bytes" in msg and f"unerf_image_metrics_batch_workspace_bytes({n}, {B}) = {need}" in msg, msg
    # the single-image size is not enough for two images
    assert _call(h, n=n, B=B, ws_bytes=h.unerf_image_metrics_workspace_bytes(n)) == -1


def test_zero_pixels_is_a_successful_no_op(lib):
    h = lib.load()
    assert _call(h, n=0, B=3, H=0, W=0, pred=None, target=None, sigma=None, ws=None, ws_bytes=0, out=None, flags=15) == 0


def test_cpu_tensors_are_refused(lib):
    from uncertainty_nerf_gs_amd import ops
    x = torch.zeros(2, 4, 4, 3)
    with pytest.raises(lib.UnerfError, match="no CPU path"):
        ops.image_metrics_batch(x, x, torch.ones(2, 4, 4), nll_min_sigma=0.03, flags=lib.METRICS_NLL)


def test_shape_mismatches_and_too_many_images_are_refused_by_the_binding(lib):
    from uncertainty_nerf_gs_amd import ops
    x, s = torch.zeros(2, 4, 4, 3), torch.ones(2, 4, 4)
    kw = dict(nll_min_sigma=0.03, flags=lib.METRICS_NLL)
    with pytest.raises(lib.UnerfError, match="image_metrics_batch: pred"):
        ops.image_metrics_batch(x, x[:, :3], s, **kw)
    with pytest.raises(lib.UnerfError, match="image_metrics_batch: pred"):
        ops.image_metrics_batch(x, x, torch.ones(2, 4, 5), **kw)
    with pytest.raises(lib.UnerfError, match="image_metrics_batch: pred"):
        ops.image_metrics_batch(x, x, torch.ones(4, 4, 2), **kw)
    with pytest.raises(lib.UnerfError, match="mask"):
        ops.image_metrics_batch(x, x, s, torch.ones(2, 4, 3, dtype=torch.bool), **kw)
    big = torch.zeros(lib.METRICS_MAX_IMAGES + 1, 2, 3)
    with pytest.raises(lib.UnerfError, match="B = 65"):
        ops.image_metrics_batch(big, big, torch.ones(lib.METRICS_MAX_IMAGES + 1, 2), **kw)


# ---------------------------------------------------------------- the harness --------------------------------------

SIZES = [(24, 32)] * 4 + [(16, 40)] * 3               # seven eval images: view_batch = 3 makes the batches 3, 1, 3
DEPTH_HW = (12, 20)


class _Model:
    """stand-in: fixed random renders, the image a camera belongs to is carried in its fx"""

    def __init__(self):
        g = torch.Generator().manual_seed(7)
        self.outs, self.gts = [], []
        for H, W in SIZES:
            gt = torch.rand(H, W, 3, generator=g)
            std = 0.02 + 0.1 * torch.rand(H, W, 1, generator=g)
            depth_std = 0.2 + torch.rand(H, W, 1, generator=g)
            self.outs.append({"rgb": torch.clamp(gt + std * torch.randn(H, W, 3, generator=g), 0, 1.2), "rgb_std": std,
                              "depth": 1.0 + 3.0 * torch.rand(H, W, 1, generator=g), "depth_std": depth_std})
            self.gts.append(gt)
        self.cams = [SimpleNamespace(camera_to_worlds=torch.eye(4)[:3], fx=float(i), fy=1.0, cx=0.0, cy=0.0, height=H, width=W)
                     for i, (H, W) in enumerate(SIZES)]
        self.batches = []

    def get_outputs_for_camera(self, cam):
        return self.outs[int(cam.fx)]

    def get_outputs_for_cameras(self, batch):
        ids = [int(v) for v in batch.fx]
        self.batches.append(len(ids))
        return [self.outs[i] for i in ids]

    def eval_set(self):
        return list(zip(self.cams, self.gts))


def _depth_fn(odd=None):
    """depth_gt_fn: maps of DEPTH_HW with some invalid pixels; image `odd` gets a map of another shape"""
    def fn(i):
        h, w = (10, 18) if i == odd else DEPTH_HW
        g = torch.Generator().manual_seed(40 + i)
        gt = 1.0 + 4.0 * torch.rand(h, w, generator=g)
        gt[0, :4] = 0.0
        return gt.numpy(), 1.5 + 0.1 * i
    return fn


@pytest.fixture
def stubs(monkeypatch, lib):
    from uncertainty_nerf_gs_amd import ops
    calls = {"single": [], "batch": []}

    def row_of(pred, target, sigma, mask, image_hw, clip_max, nll_min_sigma, flags):
        assert pred.dtype == target.dtype == sigma.dtype == torch.float32
        row, _ = R.restate_row(pred, target, sigma, mask, clip=clip_max, min_sigma=nll_min_sigma,
                               image_hw=image_hw if flags & lib.METRICS_SSIM else None)
        return torch.from_numpy(row)

    def single(pred, target, sigma, mask=None, *, image_hw=None, clip_max=float("inf"), nll_min_sigma, flags, **kw):
        calls["single"].append(dict(flags=flags, mask=mask is not None))
        return row_of(pred, target, sigma, mask, image_hw, clip_max, nll_min_sigma, flags)

    def batch(pred, target, sigma, mask=None, *, image_hw=None, clip_max=float("inf"), nll_min_sigma, flags, **kw):
        B = pred.shape[0]
        assert target.shape == pred.shape and sigma.shape[0] == B and (mask is None or mask.shape == sigma.shape)
        assert all(t.is_contiguous() for t in (pred, target, sigma))
        calls["batch"].append(dict(B=B, flags=flags, mask=mask is not None))
        return torch.stack([row_of(pred[b], target[b], sigma[b], None if mask is None else mask[b], image_hw, clip_max,
                                   nll_min_sigma, flags) for b in range(B)])

    monkeypatch.setattr(ops, "image_metrics", single)
    monkeypatch.setattr(ops, "image_metrics_batch", batch)
    return calls


def _run(model, stubs, **kw):
    from uncertainty_nerf_gs_amd import eval as E
    stubs["single"].clear(), stubs["batch"].clear(), model.batches.clear()
    avg, curves = E.get_average_uncertainty_metrics(model.get_outputs_for_camera, model.eval_set(), fused=True, **kw)
    return avg, curves, {k: list(v) for k, v in stubs.items()}


def _assert_same(a, b):
    (avg_a, cur_a), (avg_b, cur_b) = a, b
    assert set(avg_a) == set(avg_b) and set(cur_a) == set(cur_b) and set(TIMING_KEYS) <= set(avg_a)
    for k in avg_a:
        if k not in TIMING_KEYS:
            assert avg_a[k] == avg_b[k], k
        else:
            assert avg_a[k] > 0 and avg_b[k] > 0
    for k in cur_a:
        assert np.array_equal(cur_a[k], cur_b[k]), k


def test_harness_scores_a_view_batch_with_one_batched_call(lib, stubs):
    m = _Model()
    avg1, cur1, c1 = _run(m, stubs, view_batch=3, metric_batch=True)
    assert m.batches == [3, 1, 3]
    assert [c["B"] for c in c1["batch"]] == [3, 1, 3] and c1["single"] == []
    assert all(c["flags"] == lib.METRICS_ALL and not c["mask"] for c in c1["batch"])
    avg0, cur0, c0 = _run(m, stubs, view_batch=3, metric_batch=False)
    assert c0["batch"] == [] and len(c0["single"]) == 7
    avgs, curs, cs = _run(m, stubs, view_batch=1)                           # metric_batch (default True) has no say here
    assert cs["batch"] == [] and len(cs["single"]) == 7 and m.batches == []
    _assert_same((avg1, cur1), (avg0, cur0))
    _assert_same((avg1, cur1), (avgs, curs))
    assert "rgb_ause_mse" in avg1 and "ssim" in avg1 and not any(k.startswith("depth_") for k in avg1)


def test_harness_without_rgb_uncertainty_asks_for_ssim_only(lib, stubs):
    m = _Model()
    avg1, cur1, c1 = _run(m, stubs, view_batch=3, metric_batch=True, eval_rgb_unc=False)
    assert [c["B"] for c in c1["batch"]] == [3, 1, 3] and all(c["flags"] == lib.METRICS_SSIM for c in c1["batch"])
    assert set(avg1) == {"psnr", "ssim", *TIMING_KEYS}
    avg0, cur0, _ = _run(m, stubs, view_batch=3, metric_batch=False, eval_rgb_unc=False)
    avgs, curs, _ = _run(m, stubs, view_batch=1, eval_rgb_unc=False)
    _assert_same((avg1, cur1), (avg0, cur0))
    _assert_same((avg1, cur1), (avgs, curs))


def test_harness_depth_maps_of_one_shape_share_a_batched_call(lib, stubs):
    m = _Model()
    no_ssim = lib.METRICS_ALL & ~lib.METRICS_SSIM
    avg1, cur1, c1 = _run(m, stubs, view_batch=3, metric_batch=True, depth_gt_fn=_depth_fn())
    assert c1["single"] == []
    assert [(c["B"], c["flags"], c["mask"]) for c in c1["batch"]] == [
        (3, lib.METRICS_ALL, False), (3, no_ssim, True), (1, lib.METRICS_ALL, False), (1, no_ssim, True),
        (3, lib.METRICS_ALL, False), (3, no_ssim, True)]                     # one rgb and one depth call per flush
    assert "depth_ause_mse" in avg1 and "depth_nll" in avg1
    avg0, cur0, c0 = _run(m, stubs, view_batch=3, metric_batch=False, depth_gt_fn=_depth_fn())
    assert c0["batch"] == [] and len(c0["single"]) == 14
    avgs, curs, _ = _run(m, stubs, view_batch=1, depth_gt_fn=_depth_fn())
    _assert_same((avg1, cur1), (avg0, cur0))
    _assert_same((avg1, cur1), (avgs, curs))


def test_harness_depth_maps_of_two_shapes_in_a_batch_are_scored_per_image(lib, stubs):
    m = _Model()
    no_ssim = lib.METRICS_ALL & ~lib.METRICS_SSIM
    fn = _depth_fn(odd=5)                                                   # inside the last batch (images 4, 5, 6)
    avg1, cur1, c1 = _run(m, stubs, view_batch=3, metric_batch=True, depth_gt_fn=fn)
    assert [(c["B"], c["flags"]) for c in c1["batch"]] == [(3, lib.METRICS_ALL), (3, no_ssim), (1, lib.METRICS_ALL), (1, no_ssim),
                                                           (3, lib.METRICS_ALL)]
    assert c1["single"] == [dict(flags=no_ssim, mask=True)] * 3
    avg0, cur0, _ = _run(m, stubs, view_batch=3, metric_batch=False, depth_gt_fn=fn)
    avgs, curs, _ = _run(m, stubs, view_batch=1, depth_gt_fn=fn)
    _assert_same((avg1, cur1), (avg0, cur0))
    _assert_same((avg1, cur1), (avgs, curs))


def test_a_non_finite_image_is_named_by_its_index_in_the_eval_set(lib, stubs, monkeypatch):
    from uncertainty_nerf_gs_amd import eval as E, ops
    m = _Model()
    inner = ops.image_metrics_batch

    def poisoned(pred, *a, **kw):
        rows = inner(pred, *a, **kw)
        if pred.shape[0] == 3 and pred.shape[1] == 16:                       # the last batch: its second image = eval image 5
            rows[1, 1] = 2.0
        return rows

    monkeypatch.setattr(ops, "image_metrics_batch", poisoned)
    with pytest.raises(ValueError, match=r"image 5: 2 of \d+ pixels have a non-finite"):
        E.get_average_uncertainty_metrics(m.get_outputs_for_camera, m.eval_set(), fused=True, view_batch=3)
    with pytest.raises(ValueError, match=r"image 1: 2 of \d+ pixels have a non-finite"):
        E.image_metrics_unc_batch(m.outs[4:7], m.gts[4:7])
