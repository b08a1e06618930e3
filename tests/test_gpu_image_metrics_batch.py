"""unerf_image_metrics_batch on the GPU: row b of a batch against the row `ops.image_metrics` leaves for image b alone.

The comparison target is the single-image entry, which tests/test_gpu_image_metrics.py and test_gpu_image_metrics_edges.py
hold to the float64 restatement; the gate is equality of all 656 slots as bit patterns (`np.array_equal` on the rows
viewed as int64): the image is an outer grid coordinate of every kernel, so each image keeps the workgroup decomposition
and the reduction order it has alone, and nothing but its own region of the workspace feeds its row.

The images of a batch come from different seeds AND error scales: image b's noise is multiplied by 4^b, so the sort
keys of two images occupy different radix digits and a digit table, key array, counter or slab shared between images
shows up as a wrong row.  (From b = 32 on the float32 squared errors saturate to +inf; the rows are still compared bit
for bit.)  One case also holds row 0 to `restate_row` with the gates of tests/test_gpu_image_metrics_edges.py."""
import json

import numpy as np
import pytest
import torch

import test_metrics_abi_cpu as R

pytestmark = pytest.mark.gpu

TILE = 4096                                                                  # MS_TILE of csrc/unerf_metrics.hip


def _image(n, Cc, seed, b, masked=False, keep=0.5):
    """image b of a batch, [n, Cc]: the pixels of test_gpu_image_metrics_edges._pixels with the noise scaled by 4^b"""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(n, Cc, generator=g)
    std = 0.02 + 0.2 * torch.rand(n, generator=g)
    pred = gt + (4.0 ** b) * (std[:, None] * torch.randn(n, Cc, generator=g) + 0.05)
    std[3:60:7] = 0.0
    std[5:80:9] = 0.0
    pred[5:80:9] = gt[5:80:9]
    mask = (torch.rand(n, generator=g) < keep) if masked else None
    return pred, gt, std, mask


def _images(B, n, Cc, seed, masked=False, keep=0.5):
    return [_image(n, Cc, seed + 17 * b, b, masked, keep) for b in range(B)]


def _params(Cc):
    return (1.0, 3e-2) if Cc % 2 else (float("inf"), 0.1)                    # (clip_max, nll_min_sigma)


def _no_ssim():
    from uncertainty_nerf_gs_amd import lib as L
    return L.METRICS_ALL & ~L.METRICS_SSIM


def _single_rows(dev, imgs, clip, min_sigma, flags, shape=None, **kw):
    """the comparison target: one ops.image_metrics call per image -> [B, 656]"""
    from uncertainty_nerf_gs_amd import ops
    rows = []
    for pred, gt, std, mask in imgs:
        if shape is not None:
            pred, gt, std = pred.view(*shape, -1), gt.view(*shape, -1), std.view(*shape)
        rows.append(ops.image_metrics(pred.to(dev), gt.to(dev), std.to(dev), None if mask is None else mask.to(dev),
                                      image_hw=shape, clip_max=clip, nll_min_sigma=min_sigma, flags=flags, **kw))
    return torch.stack(rows).cpu().numpy()


def _stacks(dev, imgs, shape=None):
    pred, gt, std = (torch.stack([im[j] for im in imgs]).to(dev) for j in range(3))
    if shape is not None:
        B = len(imgs)
        pred, gt, std = pred.view(B, *shape, -1), gt.view(B, *shape, -1), std.view(B, *shape)
    if all(im[3] is None for im in imgs):
        return pred, gt, std, None
    mask = torch.stack([torch.ones(im[2].shape, dtype=torch.bool) if im[3] is None else im[3] for im in imgs]).to(dev)
    return pred, gt, std, mask


def _batch_rows(dev, imgs, clip, min_sigma, flags, shape=None, **kw):
    from uncertainty_nerf_gs_amd import lib as L, ops
    rows = ops.image_metrics_batch(*_stacks(dev, imgs, shape), image_hw=shape, clip_max=clip, nll_min_sigma=min_sigma, flags=flags, **kw)
    assert rows.shape == (len(imgs), L.METRICS_ROW) and rows.dtype == torch.float64 and rows.is_cuda
    return rows.cpu().numpy()


def _assert_rows_equal(got, want, what):
    a, b = np.ascontiguousarray(got).view(np.int64), np.ascontiguousarray(want).view(np.int64)
    differ = np.argwhere(a != b)
    print(f"[{what}] {got.shape[0]} rows of {got.shape[1]} slots: {len(differ)} slots differ from the single-image rows")
    assert np.array_equal(a, b), (what, [(int(i), int(j), got[i, j], want[i, j]) for i, j in differ[:8]])


# ---------------------------------------------------------------- 1: sizes ------------------------------------------

@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("Cc", [1, 3])
@pytest.mark.parametrize("n", [1, 65, 4097, 8193])
def test_sizes_at_the_wave_workgroup_and_tile_edges(dev, n, Cc, masked):
    imgs = _images(3, n, Cc, seed=1000 * Cc + n, masked=masked)
    clip, min_sigma = _params(Cc)
    got = _batch_rows(dev, imgs, clip, min_sigma, _no_ssim())
    _assert_rows_equal(got, _single_rows(dev, imgs, clip, min_sigma, _no_ssim()), f"n {n} C {Cc}{' masked' if masked else ''}")
    if (n, Cc, masked) == (8193, 3, True):                                   # and row 0 against the float64 restatement
        import test_gpu_image_metrics_edges as TE
        ref, ex = R.restate_row(*imgs[0], clip=clip, min_sigma=min_sigma)
        TE._check_row(got[0], ref, ex, "batch of 3, n 8193 C 3 masked, row 0")


def test_sixteen_images(dev):
    imgs = _images(16, TILE + 1, 3, seed=16)
    got = _batch_rows(dev, imgs, 1.0, 3e-2, _no_ssim())
    _assert_rows_equal(got, _single_rows(dev, imgs, 1.0, 3e-2, _no_ssim()), "B 16, n 4097")
    assert len({row.tobytes() for row in got}) == 16


# ---------------------------------------------------------------- 2: per-image masks --------------------------------

def test_each_image_has_its_own_mask(dev):
    n = TILE + 1
    imgs = _images(4, n, 3, seed=21)
    none_valid = torch.zeros(n, dtype=torch.bool)
    last_only = torch.zeros(n, dtype=torch.bool)
    last_only[-1] = True
    some = torch.rand(n, generator=torch.Generator().manual_seed(22)) < 0.7
    for b, m in ((1, none_valid), (2, last_only), (3, some)):                # image 0: no mask
        imgs[b] = imgs[b][:3] + (m,)
    got = _batch_rows(dev, imgs, 1.0, 3e-2, _no_ssim())
    _assert_rows_equal(got, _single_rows(dev, imgs, 1.0, 3e-2, _no_ssim()), "per-image masks")
    inf = float("inf")
    assert tuple(got[1][8:12]) == (inf, -inf, inf, -inf) and not np.any(np.delete(got[1], [8, 9, 10, 11]))
    assert got[0][0] == n and got[2][0] == 1 and got[3][0] == int(some.sum()) and 0.6 * n < got[3][0] < 0.8 * n


# ---------------------------------------------------------------- 3: SSIM -------------------------------------------

@pytest.mark.parametrize("H,W,Cc", [(11, 11, 3), (27, 43, 3), (26, 42, 4)])
def test_ssim(dev, H, W, Cc):
    from uncertainty_nerf_gs_amd import lib as L
    imgs = _images(3, H * W, Cc, seed=100 * H + W)
    clip, min_sigma = 1.0, 3e-2
    got = _batch_rows(dev, imgs, clip, min_sigma, L.METRICS_ALL, shape=(H, W))
    _assert_rows_equal(got, _single_rows(dev, imgs, clip, min_sigma, L.METRICS_ALL, shape=(H, W)), f"ssim {H}x{W}x{Cc}")
    assert np.all(got[:, 13] == (H - 10) * (W - 10) * Cc) and np.all(got[:, 12] != 0)


# ---------------------------------------------------------------- 4: flag subsets -----------------------------------

def test_flag_subsets(dev):
    from uncertainty_nerf_gs_amd import lib as L
    H, W = 27, 43
    imgs = _images(2, H * W, 3, seed=41)
    slots = {L.METRICS_AUSE: np.arange(L.METRICS_AUSE_OFF, L.METRICS_ROW), L.METRICS_AUCE: np.arange(L.METRICS_AUCE_OFF, L.METRICS_AUSE_OFF),
             L.METRICS_NLL: np.array([7]), L.METRICS_SSIM: np.array([12, 13])}
    always = np.array([0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11])
    for flags in (L.METRICS_AUSE, L.METRICS_AUCE, L.METRICS_NLL, L.METRICS_SSIM, 0):
        got = _batch_rows(dev, imgs, 1.0, 3e-2, flags, shape=(H, W))
        _assert_rows_equal(got, _single_rows(dev, imgs, 1.0, 3e-2, flags, shape=(H, W)), f"flags {flags}")
        asked = np.concatenate([always] + [s for f, s in slots.items() if flags & f])
        rest = np.setdiff1d(np.arange(L.METRICS_ROW), asked)
        assert not np.any(got[:, rest]), (flags, "slots that were not asked for")


# ---------------------------------------------------------------- 5: the caller's tables ----------------------------

def test_caller_tables(dev):
    ratios, z = R.edge_tables()
    imgs = _images(2, TILE + 1, 3, seed=51, masked=True)
    got = _batch_rows(dev, imgs, 1.0, 3e-2, _no_ssim(), ratios=ratios, z=z)
    _assert_rows_equal(got, _single_rows(dev, imgs, 1.0, 3e-2, _no_ssim(), ratios=ratios, z=z), "tables of 128 entries")


# ---------------------------------------------------------------- 6: the cap ----------------------------------------

def test_sixty_four_images(dev):
    from uncertainty_nerf_gs_amd import lib as L, ops
    imgs = _images(L.METRICS_MAX_IMAGES, 257, 3, seed=61)
    got = _batch_rows(dev, imgs, 1.0, 3e-2, _no_ssim())
    _assert_rows_equal(got, _single_rows(dev, imgs, 1.0, 3e-2, _no_ssim()), "B 64, n 257")
    pred, gt, std, _ = _stacks(dev, imgs)
    with pytest.raises(L.UnerfError, match="B = 65"):
        ops.image_metrics_batch(torch.cat([pred, pred[:1]]), torch.cat([gt, gt[:1]]), torch.cat([std, std[:1]]), nll_min_sigma=3e-2,
                                flags=_no_ssim())


# ---------------------------------------------------------------- 7: dirty and reused scratch -----------------------

def test_dirty_and_reused_scratch(dev):
    from uncertainty_nerf_gs_amd import lib as L, ops
    ws = ops.Workspace()
    for B, n in ((3, 2 * TILE + 1), (2, 65)):
        imgs = _images(B, n, 3, seed=70 + n, masked=True, keep=0.9)
        fresh = _batch_rows(dev, imgs, 1.0, 3e-2, _no_ssim())
        _assert_rows_equal(fresh, _single_rows(dev, imgs, 1.0, 3e-2, _no_ssim()), f"B {B} n {n}, fresh scratch")
        words = (L.load().unerf_image_metrics_batch_workspace_bytes(n, B) + 7) // 8
        ws.get("image_metrics_batch", (words,), dev, torch.float64).view(torch.uint8).fill_(255)
        _assert_rows_equal(_batch_rows(dev, imgs, 1.0, 3e-2, _no_ssim(), workspace=ws), fresh, f"B {B} n {n}, arena of 0xFF bytes")
    assert ws.nbytes() >= L.load().unerf_image_metrics_batch_workspace_bytes(2 * TILE + 1, 3)


def test_out_is_cleared_by_the_call(dev, lib):
    """the C entry on an `out` full of NaN and a workspace full of 0xFF bytes, flags = AUCE only: the slots nothing writes
    are the call's to clear"""
    import ctypes as C
    B, n = 3, 2 * TILE + 1
    imgs = _images(B, n, 3, seed=75)
    pred, gt, std, _ = _stacks(dev, imgs)
    h = lib.load()
    nbytes = h.unerf_image_metrics_batch_workspace_bytes(n, B)
    ws = torch.full(((nbytes + 7) // 8 * 8,), 255, dtype=torch.uint8, device=dev)
    out = torch.full((B, lib.METRICS_ROW), float("nan"), dtype=torch.float64, device=dev)
    r, z = R.tables()
    dp = C.POINTER(C.c_double)
    with torch.cuda.device(dev):
        rc = h.unerf_image_metrics_batch(pred.data_ptr(), gt.data_ptr(), std.data_ptr(), None, n, B, 3, 0, 0, 1.0, 3e-2,
                                         r.ctypes.data_as(dp), r.size, z.ctypes.data_as(dp), z.size, lib.METRICS_AUCE, ws.data_ptr(),
                                         nbytes, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    lib.check(rc, "image_metrics_batch")
    _assert_rows_equal(out.cpu().numpy(), _single_rows(dev, imgs, 1.0, 3e-2, lib.METRICS_AUCE), "out full of NaN, workspace of 0xFF")


# ---------------------------------------------------------------- 8: a side stream ----------------------------------

def test_a_side_stream(dev):
    from uncertainty_nerf_gs_amd import ops
    imgs = _images(3, 2 * TILE + 77, 3, seed=81, masked=True)
    want = _single_rows(dev, imgs, 1.0, 3e-2, _no_ssim())
    staged = _stacks(dev, imgs)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        p, t, s, m = (x + 0 if x.dtype != torch.bool else x.clone() for x in staged)
        rows = ops.image_metrics_batch(p, t, s, m, clip_max=1.0, nll_min_sigma=3e-2, flags=_no_ssim())
    side.synchronize()
    _assert_rows_equal(rows.cpu().numpy(), want, "side stream")


# ---------------------------------------------------------------- 9: a non-finite input in one image ----------------

def test_a_nan_in_one_image_stays_in_its_row(dev):
    from uncertainty_nerf_gs_amd import eval as E, lib as L
    H, W = 27, 43
    imgs = _images(3, H * W, 3, seed=91)
    imgs[1][0][H * W // 2, 1] = float("nan")
    got = _batch_rows(dev, imgs, 1.0, 3e-2, L.METRICS_ALL, shape=(H, W))
    want = _single_rows(dev, imgs, 1.0, 3e-2, L.METRICS_ALL, shape=(H, W))
    assert got[1][1] == 1 and got[0][1] == 0 and got[2][1] == 0 and got[1][0] == want[1][0] == H * W
    _assert_rows_equal(got[[0, 2]], want[[0, 2]], "the images next to the one with a NaN")
    outs = [{"rgb": p.view(H, W, 3).to(dev), "rgb_std": s.view(H, W, 1).to(dev)} for p, _, s, _ in imgs]
    gts = [g.view(H, W, 3) for _, g, _, _ in imgs]
    with pytest.raises(ValueError, match=f"image 1: 1 of {H * W} pixels have a non-finite"):
        E.image_metrics_unc_batch(outs, gts)
    imgs[1][0][H * W // 2, 1] = 0.5
    outs[1]["rgb"] = imgs[1][0].view(H, W, 3).to(dev)
    done = E.image_metrics_unc_batch(outs, gts)
    for (md, curves), o, g in zip(done, outs, gts):
        md1, curves1 = E.image_metrics_unc(o, g, fused=True)
        assert md == md1 and all(np.array_equal(curves[k], curves1[k]) for k in curves1) and set(curves) == set(curves1)


# ---------------------------------------------------------------- 10: the harness on real renders -------------------

TIMING_KEYS = ("num_rays_per_sec", "fps", "render_rays_per_sec")


def _compare_harness(run, tmp_path):
    res = {}
    for mb in (False, True):
        res[mb] = run(mb, tmp_path / f"m{int(mb)}.json")
        on_disk = json.loads((tmp_path / f"m{int(mb)}.json").read_text())["results"]
        assert on_disk == res[mb]
    assert set(res[True]) == set(res[False]) and set(TIMING_KEYS) <= set(res[True])
    for k in res[True]:
        if k not in TIMING_KEYS:
            assert res[True][k] == res[False][k], k
        else:
            assert res[True][k] > 0
    return res[True]


def test_run_eval_metric_batch_active_nerfacto_with_depth(dev, tmp_path, monkeypatch):
    from uncertainty_nerf_gs_amd import eval as E, ops
    import test_gpu_nerf_view_batch as TV
    _, singles = TV._cameras(5)
    eval_set = [(cam, TV._gt(TV.H, TV.W, 50 + i)) for i, cam in enumerate(singles)]

    def depth_gt_fn(i):                                                       # half-size maps: the renders are resized to them
        g = torch.Generator().manual_seed(60 + i)
        gt = 0.5 + 3.0 * torch.rand(15, 19, generator=g)
        gt[0, :4] = 0.0
        return gt.numpy(), 1.0 + 0.25 * i

    seen, inner = [], ops.image_metrics_batch
    monkeypatch.setattr(ops, "image_metrics_batch", lambda pred, *a, **kw: (seen.append(int(pred.shape[0])), inner(pred, *a, **kw))[1])
    curves = {}

    def run(mb, path):
        model = TV._model(dev, "active", "active-nerfacto")
        ecfg = E.ActiveNerfactoConfig(load_config=None, output_path=path)
        curves[mb] = E.get_average_uncertainty_metrics(model.get_outputs_for_camera, eval_set, depth_gt_fn=depth_gt_fn,
                                                       min_depth_std_for_nll=ecfg.min_depth_std_for_nll, fused=True, view_batch=4,
                                                       metric_batch=mb)[1]
        return E.run_eval(ecfg, model, eval_set, depth_gt_fn=depth_gt_fn, fused=True, view_batch=4, metric_batch=mb)

    got = _compare_harness(run, tmp_path)
    assert seen == [4, 4, 1, 1] * 2 and "depth_ause_mse" in got and "ssim" in got          # rgb + depth per flush, two runs
    assert set(curves[True]) == set(curves[False]) and any(k.startswith("depth_") for k in curves[True])
    for k in curves[True]:
        assert np.array_equal(curves[True][k], curves[False][k]), k


def test_run_eval_metric_batch_active_splatfacto(dev, tmp_path):
    from uncertainty_nerf_gs_amd import eval as E
    from uncertainty_nerf_gs_amd import models, synthetic
    import test_gpu_nerf_view_batch as TV
    import test_gpu_splat as TS
    m, cam, g = TS._fixture_model(dev)
    fx, fy, cx, cy, Hs, Ws = (float(v) for v in g["intr"])
    Hs, Ws = int(Hs), int(Ws)
    cams = [models.Camera(synthetic.orbit_c2w(0.4 + 0.8 * i, radius=2.5, height=0.5), fx + i, fy, cx, cy, Hs, Ws) for i in range(5)]
    gen = torch.Generator().manual_seed(5)
    eval_set = [(c, torch.cat([TV._gt(Hs, Ws, 70 + i), (torch.rand(Hs, Ws, 1, generator=gen) > 0.2).float()], dim=-1))
                for i, c in enumerate(cams)]

    def run(mb, path):
        ecfg = E.ActiveSplatfactoConfig(load_config=None, output_path=path)
        return E.run_eval(ecfg, m, eval_set, method_name="active-splatfacto", fused=True, view_batch=4, metric_batch=mb)

    got = _compare_harness(run, tmp_path)
    assert "rgb_ause_mse" in got and "ssim" in got
