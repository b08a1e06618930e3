"""The LPIPS kernels on the GPU (csrc/unerf_lpips.hip): the input pack, the convolution and max-pool driven directly, the
head on host-made features, the whole metric against the float64 host definition, and the eval harness.  Synthetic
weights and the seeds of lpips_cases.py throughout."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_cases as LC

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24      # unit roundoff of float32
U64 = 2.0 ** -53


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# ---- input pack -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(31, 31), (35, 50)])
@pytest.mark.parametrize("B", [1, 3])
def test_input_pack_is_bit_equal_and_counts_planted_values(dev, H, W, B):
    from uncertainty_nerf_gs_amd import ops
    w = LC.weights()
    pred, target = LC.image_pair(H, W, B)
    nan = float("nan")
    want_bad = [0] * B
    last = B - 1
    pred[last, 0, 0, 0] = nan;      want_bad[last] += 1
    pred[last, H - 1, W - 1, 2] = -0.1;  want_bad[last] += 1
    pred[last, 3, 3, 1] = 1.5                                      # clipped to 1: not counted
    target[0, 1, 2, 0] = 1.5;       want_bad[0] += 1
    target[0, 5, 5, 2] = nan;       want_bad[0] += 1
    target[0, H - 1, 0, 1] = -1e-9; want_bad[0] += 1
    act, bad = ops.lpips_pack(pred.to(dev), target.to(dev), w)
    x = torch.cat((torch.clip(pred, max=1.0), target))
    want = ((2 * x - 1) - w.shift) / w.scale                        # the float32 torch statement, HWC
    assert act.shape == (2 * B, H, W, 3)
    assert torch.equal(_bits(act), _bits(want))
    assert bad.cpu().tolist() == want_bad


# ---- conv2d_bias_relu -------------------------------------------------------------------------------------------------

def _conv_case(dev, layer, N, H, W, seed, relu=True, Ci=None, Co=None, nan_fill=False, side_stream=False):
    """one call of the kernel on random inputs with layer `layer`'s geometry (and weights, unless Ci / Co shrink them)
    against float64 F.conv2d, held to gamma_{K+1} (|bias| + sum |a w|); a second call must give equal bits"""
    from uncertainty_nerf_gs_amd import ops
    ks, stride, pad = LC.GEOMETRY[layer]
    cw, cb = LC.weights().convs[layer]
    if Ci is not None:
        cw, cb = cw[:Co, :Ci].contiguous(), cb[:Co].contiguous()
    Co_, Ci_ = cw.shape[0], cw.shape[1]
    K = ks * ks * Ci_
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, Ci_, generator=g)
    packed = cw.permute(2, 3, 1, 0).reshape(K, Co_).contiguous()
    xd, wd, bd = x.to(dev), packed.to(dev), cb.to(dev)
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    out = torch.full((N, Ho, Wo, Co_), float("nan"), device=dev) if nan_fill else None
    if side_stream:
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            xs = xd * 1.0                                             # made on the side stream: only it sees the value
            got = ops.conv2d_bias_relu(xs, wd, bd, ks, stride, pad, relu=relu)
        side.synchronize()
    else:
        got = ops.conv2d_bias_relu(xd, wd, bd, ks, stride, pad, relu=relu, out=out)
    again = ops.conv2d_bias_relu(xd, wd, bd, ks, stride, pad, relu=relu)
    torch.cuda.synchronize()
    assert got.shape == (N, Ho, Wo, Co_)
    assert torch.equal(_bits(got), _bits(again)), "two calls differ"
    x64 = x.double().permute(0, 3, 1, 2)
    ref = F.conv2d(x64, cw.double(), cb.double(), stride=stride, padding=pad)
    mag = F.conv2d(x64.abs(), cw.double().abs(), cb.double().abs(), stride=stride, padding=pad)
    if relu:
        ref = torch.relu(ref)                                         # 1-Lipschitz: the bound carries over
    err = (got.cpu().double().permute(0, 3, 1, 2) - ref).abs()
    bound = LC.gamma(K + 1, U32) * mag
    worst = float((err / bound).max())
    print(f"conv layer {layer} N={N} {H}x{W} Ci={Ci_} Co={Co_} K={K}: {N * Ho * Wo} pixels, max err / bound = {worst:.3f}")
    assert not torch.isnan(got).any() and worst <= 1.0
    return got


@pytest.mark.parametrize("H,W", [(31, 31), (35, 50)])
@pytest.mark.parametrize("N", [2, 3])
def test_conv1_form(dev, H, W, N):
    """K = 363 (no multiple of the k step); 31 x 31 gives 49 pixels per image, so with three images the row tiles
    straddle image boundaries"""
    _conv_case(dev, 0, N, H, W, seed=100 + N)


@pytest.mark.parametrize("H,W", [(3, 3), (7, 9)])
def test_conv2_form_window_overhangs_every_side(dev, H, W):
    _conv_case(dev, 1, 2, H, W, seed=200 + H)


@pytest.mark.parametrize("layer", [2, 3, 4])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (9, 9)])
def test_conv345_forms(dev, layer, H, W):
    """1 x 1: only the centre tap is live"""
    _conv_case(dev, layer, 2, H, W, seed=300 + 10 * layer + H)


def test_conv_pixel_totals_around_the_row_tile(dev, lib):
    T = lib.LPIPS_CONV_TILE_M
    for total in (1, T - 1, T, T + 1):
        _conv_case(dev, 4, 1, 1, total, seed=400 + total, Ci=24, Co=lib.LPIPS_CONV_TILE_N)


def test_conv_on_nan_filled_output_on_a_side_stream_and_without_relu(dev):
    _conv_case(dev, 1, 3, 7, 9, seed=500, nan_fill=True)
    _conv_case(dev, 0, 3, 31, 31, seed=501, side_stream=True)
    got = _conv_case(dev, 2, 2, 3, 5, seed=502, relu=False)
    assert float(got.min()) < 0.0


def test_conv_refuses_a_column_count_off_the_tile(dev, lib):
    from uncertainty_nerf_gs_amd import ops
    with pytest.raises(lib.UnerfError, match="column tile"):
        ops.conv2d_bias_relu(torch.zeros(1, 4, 4, 3, device=dev), torch.zeros(27, 48, device=dev), torch.zeros(48, device=dev), 3, 1, 1)


# ---- maxpool3s2 -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(7, 7), (8, 11), (3, 3)])
def test_maxpool_is_bit_equal_to_torch(dev, H, W):
    from uncertainty_nerf_gs_amd import ops
    g = torch.Generator().manual_seed(600 + H)
    x = torch.randn(3, H, W, 70, generator=g)
    got = ops.maxpool3s2(x.to(dev))
    want = F.max_pool2d(x.permute(0, 3, 1, 2), kernel_size=3, stride=2).permute(0, 2, 3, 1).contiguous()
    assert got.shape == want.shape == (3, (H - 3) // 2 + 1, (W - 3) // 2 + 1, 70)
    assert torch.equal(_bits(got), _bits(want))


# ---- head -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w,C", [(1, 1, 64), (7, 7, 192), (9, 15, 384)])
def test_head_against_the_float64_statement(dev, lib, h, w, C):
    """features made on the host; the reference in extended precision (its own rounding is then far below the bound):
    gamma_{n + 8} at u = 2^-53 times the sum of the absolute terms, n = h w C the length of the longest sum.  9 x 15 =
    135 pixels is more than two workgroups' ranges, the last one partly filled"""
    from uncertainty_nerf_gs_amd import metrics as M, ops
    assert (h * w > 2 * lib.LPIPS_HEAD_PIXELS) == ((h, w) == (9, 15))
    B = 2
    g = torch.Generator().manual_seed(700 + C)
    feats = torch.relu(torch.randn(2 * B, h, w, C, generator=g))
    lin = torch.rand(C, generator=g) / C
    got = ops.lpips_head(feats.to(dev), lin.to(dev))
    again = ops.lpips_head(feats.to(dev), lin.to(dev))
    assert torch.equal(_bits(got), _bits(again))
    f = feats.numpy().astype(np.longdouble).reshape(2 * B, h * w, C)
    nrm = f / np.sqrt(np.longdouble(M.LPIPS_NORM_EPS) + (f * f).sum(axis=2, keepdims=True))
    terms = lin.numpy().astype(np.longdouble) * (nrm[:B] - nrm[B:]) ** 2
    want, mag = terms.sum(axis=(1, 2)), np.abs(terms).sum(axis=(1, 2))
    bound = LC.gamma(h * w * C + 8, U64) * mag
    err = np.abs(got.cpu().numpy().astype(np.longdouble) - want)
    print(f"head {h}x{w}x{C}: max err / bound = {float((err / bound).max()):.3e}")
    assert (err <= bound).all()


# ---- end to end -------------------------------------------------------------------------------------------------------

def test_end_to_end_against_the_float64_host_definition(dev):
    """finish_lpips(ops.lpips_batch) against metrics.lpips(float64) on every size and batch of lpips_cases; the tolerance
    is 4 x the largest |float32 on the CPU - float64| over the case set (the reference's own fp32 arithmetic in another
    summation order), computed here and printed next to the kernels' worst error"""
    from uncertainty_nerf_gs_amd import metrics as M, ops
    cases, gap = LC.e2e_reference()
    w = LC.weights()
    worst = 0.0
    for (H, W, B), (pred, target, v64, _v32) in cases.items():
        pd, td = pred.to(dev), target.to(dev)
        rows = ops.lpips_batch(pd, td, w)
        rows2 = ops.lpips_batch(pd, td, w)
        assert torch.equal(_bits(rows), _bits(rows2)), (H, W, B)
        host = rows.cpu().numpy()
        sizes = M.lpips_map_sizes(H, W)
        for b in range(B):
            assert host[b, 5:10].tolist() == [float(h * ww) for h, ww in sizes] and host[b, 10] == 0.0
            err = abs(M.finish_lpips(host[b]) - v64[b])
            worst = max(worst, err)
            assert err <= 4 * gap, (H, W, B, b, err, gap)
            single = ops.lpips_batch(pd[b:b + 1], td[b:b + 1], w)
            assert torch.equal(_bits(single[0]), _bits(rows[b])), (H, W, B, b)
    print(f"end to end: float32-vs-float64 gap of the host definition {gap:.3e}, kernels' worst error {worst:.3e} "
          f"(allowed {4 * gap:.3e})")


def test_a_planted_value_makes_finish_lpips_raise_naming_the_image(dev):
    from uncertainty_nerf_gs_amd import eval as E, metrics as M, ops
    pred, target = LC.image_pair(31, 47, 3)
    target[1, 4, 4, 0] = 1.25
    rows = ops.lpips_batch(pred.to(dev), target.to(dev), LC.weights()).cpu().numpy()
    assert rows[:, 10].tolist() == [0.0, 1.0, 0.0]
    M.finish_lpips(rows[0])
    with pytest.raises(ValueError, match="1 values"):
        M.finish_lpips(rows[1])
    outs = [{"rgb": pred[b].to(dev), "rgb_std": torch.full((31, 47, 1), 0.1, device=dev)} for b in range(3)]
    with pytest.raises(ValueError, match="image 12: lpips"):
        E.image_metrics_unc_batch(outs, [target[b] for b in range(3)], image_ids=[11, 12, 13], lpips_weights=LC.weights())


def test_call_on_a_nan_filled_arena_and_a_side_stream(dev):
    """nothing in the workspace is read before it is written, and the kernels run on the stream they are given"""
    from uncertainty_nerf_gs_amd import ops
    pred, target = LC.image_pair(35, 33, 3)
    w = LC.weights()
    pd, td = pred.to(dev), target.to(dev)
    want = ops.lpips_batch(pd, td, w)
    arena = ops.Workspace()
    ops.lpips_batch(pd, td, w, workspace=arena)
    for buf in arena._bufs.values():
        buf.fill_(float("nan"))
    assert torch.equal(_bits(ops.lpips_batch(pd, td, w, workspace=arena)), _bits(want))
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        ps, ts = pd * 1.0, td * 1.0
        got = ops.lpips_batch(ps, ts, w, workspace=arena)
    side.synchronize()
    assert torch.equal(_bits(got), _bits(want))


# ---- the harness ------------------------------------------------------------------------------------------------------

def test_run_eval_reports_lpips_and_leaves_the_other_keys_alone(dev, tmp_path):
    from uncertainty_nerf_gs_amd import eval as E, models, synthetic
    import test_gpu_models as TM
    H, W = 40, 48
    t = synthetic.make_scene_tensors(seed=21, kind="active", log2T=14, prop_log2T=12)
    cfg = TM._small_cfg(models.ActiveNerfactoModelConfig(average_init_density=0.01))
    model = cfg._target(cfg, num_train_data=4)
    sd = TM._state_dict_from_tensors(t, "active")
    sd.update({"_model." + k: v for k, v in synthetic.make_lpips_weights(LC.WEIGHT_SEED).items()})
    model.load_state_dict(sd)
    assert model.lpips_weights is not None
    model = model.to(dev)
    cams = [models.Camera(synthetic.orbit_c2w(0.5 + 1.3 * i), 0.9 * W, 0.9 * W, W / 2, H / 2, H, W) for i in range(4)]
    g = torch.Generator().manual_seed(9)
    eval_set = [(cam, torch.rand(H, W, 3, generator=g)) for cam in cams]

    def run(name, **kw):
        ecfg = E.ActiveNerfactoConfig(load_config=None, output_path=tmp_path / f"{name}.json", eval_depth=False)
        return E.run_eval(ecfg, model, eval_set, **kw)

    fused = run("fused", fused=True, view_batch=4)
    plain = run("plain", fused=False, view_batch=4)
    without = run("without", fused=True, view_batch=4, lpips_weights=None)
    _, gap = LC.e2e_reference()
    print(f"harness: lpips fused {fused['lpips']!r}, torch {plain['lpips']!r}, |diff| {abs(fused['lpips'] - plain['lpips']):.3e}, "
          f"allowed {4 * gap:.3e}")
    timing = {"num_rays_per_sec", "fps", "render_rays_per_sec"}
    assert "lpips" not in without and set(fused) == set(without) | {"lpips"}
    for k in without:
        if k not in timing:
            assert fused[k] == without[k], k
    assert abs(fused["lpips"] - plain["lpips"]) <= 4 * gap
