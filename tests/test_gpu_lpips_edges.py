"""The LPIPS kernels on the GPU at their tile, cap and batch edges: the cases, references and bounds of
tests/lpips_edge_cases.py (checked without a GPU in tests/test_lpips_edge_cases_cpu.py) through ops.lpips_pack,
ops.maxpool3s2, ops.conv2d_bias_relu, ops.lpips_head and ops.lpips_batch.  Every test prints its worst error over its
bound; the file prints its wall time."""
import time

import numpy as np
import pytest
import torch

import lpips_cases as LC
import lpips_edge_cases as EC

pytestmark = pytest.mark.gpu

GUARD = 4096          # NaN-filled floats behind an output buffer that no kernel may touch


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\ntests/test_gpu_lpips_edges.py: wall time {time.perf_counter() - t0:.1f} s")


def _guarded(shape, dev):
    """-> (a NaN-filled view of `shape`, the NaN-filled guard behind it)"""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), float("nan"), device=dev)
    return buf[:n].view(shape), buf[n:]


# ---- pack -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", EC.PACK_CASES, ids=lambda c: c.name)
def test_pack_is_bit_equal_and_counts_exactly_across_its_trips(dev, case):
    from uncertainty_nerf_gs_amd import ops
    w = LC.weights()
    pred, target, want_bad = EC.pack_inputs(case)
    want, bad_ref = EC.pack_reference(pred, target, w)
    assert bad_ref == want_bad
    pd, td = pred.to(dev), target.to(dev)
    act, bad = ops.lpips_pack(pd, td, w)
    act2, bad2 = ops.lpips_pack(pd, td, w)
    assert act.shape == (2 * case.B, case.n, 3)
    differ = int((EC.bits(act) != EC.bits(want)).sum())
    print(f"pack {case.name}: B = {case.B}, 3 n = {3 * case.n} ({EC.ew_trips(3 * case.n)} trips), {differ} values differ, "
          f"counts {bad.cpu().tolist()} (host {want_bad})")
    assert differ == 0
    assert bad.cpu().tolist() == want_bad
    assert torch.equal(EC.bits(act2), EC.bits(act)) and bad2.cpu().tolist() == want_bad


# ---- pool -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", EC.POOL_CASES, ids=lambda c: c.name)
def test_pool_equals_torch_with_nan_and_inf_planted(dev, lib, case):
    """through ops.maxpool3s2, and through the C entry into a NaN-filled buffer with a guard behind it"""
    from uncertainty_nerf_gs_amd import ops
    x = EC.pool_input(case.name)
    want = EC.pool_reference(x)
    xd = x.to(dev)
    got = ops.maxpool3s2(xd)
    out, guard = _guarded(tuple(want.shape), dev)
    with torch.cuda.device(dev):
        rc = lib.load().unerf_maxpool3s2(xd.data_ptr(), out.data_ptr(), case.N, case.H, case.W, case.C,
                                         torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.load().unerf_last_error()
    torch.cuda.synchronize()
    nans = int(torch.isnan(want).sum())
    print(f"pool {case.name}: {want.numel()} outputs ({EC.ew_trips(want.numel())} trips), {nans} NaN in the reference, "
          f"{int(torch.isnan(got).sum())} in the result")
    assert got.shape == want.shape
    assert EC.same_with_nans(got.cpu(), want)
    assert EC.same_with_nans(out.cpu(), want)
    assert bool(torch.isnan(guard).all()), "the guard behind the output was written"


# ---- convolution ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", EC.CONV_CASES, ids=lambda c: c.name)
def test_conv_against_float64_on_every_output(dev, case):
    """three calls with equal bits: a fresh output, a NaN-filled output with a guard behind it, and a side stream"""
    from uncertainty_nerf_gs_amd import ops
    x, _, b, packed = EC.conv_inputs(case.name)
    ref, bound = EC.conv_reference(case.name)
    Ho, Wo, Mtot, K = EC.conv_dims(case)
    xd, wd, bd = x.to(dev), packed.to(dev), b.to(dev)
    got = ops.conv2d_bias_relu(xd, wd, bd, case.ks, case.stride, case.pad, relu=case.relu)
    out, guard = _guarded((case.N, Ho, Wo, case.Co), dev)
    ops.conv2d_bias_relu(xd, wd, bd, case.ks, case.stride, case.pad, relu=case.relu, out=out)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        xs = xd * 1.0                                                 # made on the side stream: only it sees the value
        third = ops.conv2d_bias_relu(xs, wd, bd, case.ks, case.stride, case.pad, relu=case.relu)
    side.synchronize()
    torch.cuda.synchronize()
    ok, worst = EC.conv_check(got, ref, bound)
    print(f"conv {case.name}: M = {Mtot}, K = {K}, C_out = {case.Co}, {int(torch.isnan(ref).sum())} NaN and "
          f"{int(torch.isinf(ref).sum())} inf in the reference, max err / bound = {worst:.3f}")
    assert got.shape == ref.shape
    assert ok
    assert torch.equal(EC.bits(out), EC.bits(got)) and torch.equal(EC.bits(third), EC.bits(got)), "calls differ"
    assert bool(torch.isnan(guard).all()), "the guard behind the output was written"


# ---- head -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", EC.HEAD_CASES, ids=lambda c: c.name)
def test_head_against_the_longdouble_statement(dev, case):
    from uncertainty_nerf_gs_amd import ops
    feats, lin = EC.head_inputs(case.name)
    fd, ld = feats.to(dev), lin.to(dev)
    got = ops.lpips_head(fd, ld)
    again = ops.lpips_head(fd, ld)
    assert got.shape == (case.B,) and got.dtype == torch.float64
    ok, worst = EC.head_inside(got.cpu().numpy(), case.name)
    print(f"head {case.name}: B = {case.B}, P = {case.P}, C = {case.C}, max err / bound = {worst:.3e}")
    assert ok
    assert torch.equal(EC.bits(got), EC.bits(again))
    if case.B > 1:                                                    # image b of the batch is image b alone
        b = case.B - 1
        alone = ops.lpips_head(torch.stack((feats[b], feats[case.B + b])).to(dev), ld)
        assert torch.equal(EC.bits(alone[0]), EC.bits(got[b]))


# ---- the whole metric --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", EC.E2E_CASES, ids=lambda s: "x".join(str(v) for v in s))
def test_whole_metric_per_layer_and_total(dev, size):
    """every image's total and each of its five layer values against the float64 host definition, within E2E_MARGIN x the
    fp32 host definition's own distance from it (per layer and for the total); exact pixel counts; row b = image b alone"""
    from uncertainty_nerf_gs_amd import metrics as M, ops
    H, W, B = size
    cases, gap_l, gap_t = EC.e2e_reference()
    pred, target, l64, t64 = cases[size]
    w = LC.weights()
    pd, td = pred.to(dev), target.to(dev)
    rows = ops.lpips_batch(pd, td, w)
    rows2 = ops.lpips_batch(pd, td, w)
    assert torch.equal(EC.bits(rows), EC.bits(rows2))
    host = rows.cpu().numpy()
    nl = M.LPIPS_LAYERS
    pixels = [float(h * ww) for h, ww in M.lpips_map_sizes(H, W)]
    err_l, err_t = np.zeros(nl), 0.0
    for b in range(B):
        assert host[b, nl:2 * nl].tolist() == pixels and host[b, 2 * nl] == 0.0
        err_l = np.maximum(err_l, np.abs(host[b, :nl] / host[b, nl:2 * nl] - l64[b]))
        err_t = max(err_t, abs(M.finish_lpips(host[b]) - t64[b]))
    print(f"e2e {H} x {W}, B = {B}: launch sizes {EC.e2e_launch_sizes(H, W, B)}")
    print(f"  total: fp32 host gap {gap_t:.3e}, kernels' worst error {err_t:.3e} (allowed {EC.E2E_MARGIN * gap_t:.3e})")
    for l in range(nl):
        print(f"  layer {l}: fp32 host gap {gap_l[l]:.3e}, kernels' worst error {err_l[l]:.3e} (allowed {EC.E2E_MARGIN * gap_l[l]:.3e})")
    assert err_t <= EC.E2E_MARGIN * gap_t
    assert (err_l <= EC.E2E_MARGIN * gap_l).all(), (err_l, gap_l)
    for b in (range(B) if H * W < 10000 else [B - 1]):
        single = ops.lpips_batch(pd[b:b + 1], td[b:b + 1], w)
        assert torch.equal(EC.bits(single[0]), EC.bits(rows[b])), b


def test_one_image_more_than_the_limit_is_refused_before_any_launch(dev, lib):
    from uncertainty_nerf_gs_amd import ops
    side = lib.LPIPS_MIN_SIDE
    x = torch.zeros(EC.BMAX + 1, side, side, 3, device=dev)
    with pytest.raises(lib.UnerfError, match=f"B = {EC.BMAX + 1}"):
        ops.lpips_batch(x, x, LC.weights())
    with pytest.raises(lib.UnerfError, match=f"B = {EC.BMAX + 1}"):
        ops.lpips_pack(x, x, LC.weights())
