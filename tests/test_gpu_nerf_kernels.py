"""Per-kernel parity: each HIP entry point (called through the C ABI) against the CPU oracle on
the same seeded inputs.  Tolerances are stated per test; integer/index results are bit-exact."""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

NEAR, FAR = 0.05, 1000.0


def _scene(kind, dev, log2T=14, prop_log2T=12, **kw):
    from uncertainty_nerf_gs_amd import synthetic
    t = synthetic.make_scene_tensors(seed=0, kind=kind, log2T=log2T, prop_log2T=prop_log2T)
    return t, O.scene_from_tensors(t), synthetic.scene_to_device(t, dev, **kw)


def _rays(H=24, W=32, theta=0.3):
    from uncertainty_nerf_gs_amd import synthetic
    c2w = synthetic.orbit_c2w(theta)
    o, d, _ = O.generate_rays(c2w, 30.0, 30.0, W / 2, H / 2, H, W)
    return o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()


def _close(got, ref, rtol, atol, what, max_bad_frac=0.0):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    bad = ((got - ref).abs() > (atol + rtol * ref.abs())) | (torch.isnan(got) != torch.isnan(ref))      # a NaN on one side only is off (NaN > tol is False)
    frac = bad.double().mean().item()
    worst = (got - ref).abs().max().item()
    assert frac <= max_bad_frac, f"{what}: {frac:.3e} of elements off (worst |diff|={worst:.3e})"


def test_generate_rays_matches_oracle_and_row_major_indexing(dev):
    from uncertainty_nerf_gs_amd import ops, synthetic
    c2w = synthetic.orbit_c2w(1.1)
    H, W = 37, 53
    o_ref, d_ref, pa_ref = O.generate_rays(c2w, 41.0, 43.0, 26.0, 18.0, H, W)
    o, d, pa = ops.generate_rays(c2w, 41.0, 43.0, 26.0, 18.0, H, W, dev, pixel_area=True)
    _close(o, o_ref.reshape(-1, 3), 0, 0, "origins")
    _close(d, d_ref.reshape(-1, 3), 0, 3e-7, "directions")
    _close(pa, pa_ref.reshape(-1, 1), 1e-3, 1e-9, "pixel_area")
    # ray/chunk bookkeeping is exact: a slice [a,b) equals rows a..b of the full bundle, bit for bit
    a, b = 123, 123 + 777
    o2, d2, _ = ops.generate_rays(c2w, 41.0, 43.0, 26.0, 18.0, H, W, dev, ray_start=a, count=b - a)
    assert torch.equal(d2, d[a:b]) and torch.equal(o2, o[a:b])


# (k1, k2, k3, k4, p1, p2): COLMAP-typical OPENCV (an `ns-process-data images` scene), radial only, all six terms
LENSES = [(-0.05, 0.02, 0.0, 0.0, 1e-3, -1e-3), (0.12, -0.03, 0.0, 0.0, 0.0, 0.0), (-0.2, 0.06, -0.01, 0.002, 4e-3, 2e-3),
          (0.0, 0.0, 0.0, 0.0, 2e-3, 0.0)]


@pytest.mark.parametrize("camera_type,lens", [(2, None), (2, [0.05, -0.01, 0.002, -0.0004, 0.0, 0.0]), (3, None),
                                              (3, [0.05, -0.01, 0.0, 0.0, 1e-3, -1e-3]), (8, None)])
def test_generate_rays_of_the_other_camera_models_match_oracle(dev, camera_type, lens):
    """FISHEYE (with and without OPENCV_FISHEYE's k1..k4), EQUIRECTANGULAR (lens parameters ignored, as upstream) and
    ORTHOPHOTO (moving origins) rays of unerf_generate_rays against the oracle's restatement of
    Cameras._generate_rays_from_coords [UPSTREAM-RECALL]; sin / cos differ between the device library and torch's CPU
    kernels by a few ulp, so directions are compared to 2e-6 (perspective rays are exact: the test above)."""
    from uncertainty_nerf_gs_amd import ops, synthetic
    H, W = 37, 51
    c2w = synthetic.orbit_c2w(1.3)
    if camera_type == 3:      # equirect: fx = fy = H = W / 2, principal point at the centre
        H, W = 32, 64
        fx, fy, cx, cy = 32.0, 32.0, 32.0, 16.0
    else:
        fx, fy, cx, cy = 21.0, 22.0, 25.2, 18.4      # fisheye: |(u, v)| up to ~1.5 rad
    o_ref, d_ref, pa_ref = O.generate_rays(c2w, fx, fy, cx, cy, H, W, distortion=lens, camera_type=camera_type)
    o, d, pa = ops.generate_rays(c2w, fx, fy, cx, cy, H, W, dev, pixel_area=True, distortion=lens, camera_type=camera_type)
    assert (d.cpu() - d_ref.reshape(-1, 3)).abs().max() <= 2e-6
    assert (o.cpu() - o_ref.reshape(-1, 3)).abs().max() <= 1e-6
    # (a pixel area is a product of two DIFFERENCES of unit vectors: the few-ulp sin / cos differences are amplified by the
    # cancellation -- 8e-9 of 2e-3 measured)
    assert (pa.cpu() - pa_ref.reshape(-1, 1)).abs().max() <= 2e-5 * max(float(pa_ref.max()), 1e-3) + 1e-9
    assert abs(float(d.norm(dim=-1).mean()) - 1.0) < 1e-6
    if camera_type == 3 and lens is not None:     # the same rays as without the lens
        plain = ops.generate_rays(c2w, fx, fy, cx, cy, H, W, dev, pixel_area=True, camera_type=camera_type)
        assert torch.equal(plain[1], d) and torch.equal(plain[2], pa)
    if camera_type == 8:
        assert float(pa.abs().max()) == 0.0 and float((d - d[0]).abs().max()) == 0.0 and float((o - o[0]).abs().max()) > 0.1
    a, b = 333, 1111       # any row-major sub-range gives the same rays
    o2, d2, _ = ops.generate_rays(c2w, fx, fy, cx, cy, H, W, dev, ray_start=a, count=b - a, distortion=lens, camera_type=camera_type)
    assert torch.equal(o2, o[a:b]) and torch.equal(d2, d[a:b])


@pytest.mark.parametrize("lens", LENSES)
def test_generate_rays_with_lens_distortion_matches_oracle(dev, lens):
    """Cameras.generate_rays with non-zero distortion_params (the reference's ns-process-data / OPENCV cameras,
    dataparsers/sparse_mipnerf360/sparse_mipnerf360_dataparser.py:248-274): origins exact, directions to 3e-7 as for
    the distortion-free camera, pixel_area (two more undistorted coordinates per pixel) to 1e-3 relative; slices of the
    bundle are bit-identical to the full bundle; six zeros are the distortion-free camera bit for bit."""
    from uncertainty_nerf_gs_amd import ops, synthetic
    c2w = synthetic.orbit_c2w(1.1)
    H, W = 54, 96                      # 16:9 at fx = 0.58 W: the field of view of the 1080p bench camera (fx 1111)
    fx, fy, cx, cy = 0.58 * W, 0.57 * W, W / 2 - 0.7, H / 2 + 0.4
    o_ref, d_ref, pa_ref = O.generate_rays(c2w, fx, fy, cx, cy, H, W, distortion=lens)
    o, d, pa = ops.generate_rays(c2w, fx, fy, cx, cy, H, W, dev, pixel_area=True, distortion=lens)
    _close(o, o_ref.reshape(-1, 3), 0, 0, "origins")
    _close(d, d_ref.reshape(-1, 3), 0, 3e-7, "directions")
    _close(pa, pa_ref.reshape(-1, 1), 1e-3, 1e-9, "pixel_area")
    plain = ops.generate_rays(c2w, fx, fy, cx, cy, H, W, dev, pixel_area=True)
    assert (plain[1] - d).abs().max().item() > 1e-4, "the lens parameters did not move the rays"
    a, b = 1234, 1234 + 2000
    o2, d2, pa2 = ops.generate_rays(c2w, fx, fy, cx, cy, H, W, dev, ray_start=a, count=b - a, pixel_area=True, distortion=lens)
    assert torch.equal(d2, d[a:b]) and torch.equal(o2, o[a:b]) and torch.equal(pa2, pa[a:b])
    zero = ops.generate_rays(c2w, fx, fy, cx, cy, H, W, dev, pixel_area=True, distortion=[0.0] * 6)
    assert all(torch.equal(x, y) for x, y in zip(zero, plain))


@pytest.mark.parametrize("L,min_res,max_res,log2T", [(16, 16, 2048, 14), (5, 16, 128, 12), (5, 16, 256, 17), (16, 16, 2048, 19)])
def test_hashgrid_indices_and_features_bit_exact(dev, L, min_res, max_res, log2T):
    from uncertainty_nerf_gs_amd import ops, synthetic
    g = torch.Generator().manual_seed(L * 100 + log2T)
    scal = synthetic.hash_scalings(L, min_res, max_res)
    table = (torch.rand(L << log2T, 2, generator=g) * 2 - 1)
    xyz = torch.rand(4096, 3, generator=g)
    # edge cases: origin (masked positions), exact grid nodes, upper border, tiny values
    xyz[0] = 0.0
    xyz[1] = torch.tensor([0.5, 0.25, 0.125])
    xyz[2] = 1.0 - 2 ** -24
    xyz[3] = torch.tensor([1.0 / 16, 2.0 / 16, 3.0 / 16])
    xyz[4] = 1e-30
    out, idx = ops.hashgrid_fwd(xyz.to(dev), table.to(dev), scal.to(dev), log2T, return_indices=True)
    idx_ref, _ = O.hash_indices(xyz, scal, log2T)
    assert torch.equal(idx.cpu().long(), idx_ref), "hash table row indices must be bit-exact"
    ref = O.hash_encode(xyz, table, scal, log2T)
    assert torch.equal(out.cpu(), ref), f"features differ: max {(out.cpu() - ref).abs().max().item():.3e}"


def test_hashgrid_empty_input(dev):
    from uncertainty_nerf_gs_amd import ops, synthetic
    scal = synthetic.hash_scalings(16, 16, 2048).to(dev)
    out = ops.hashgrid_fwd(torch.empty(0, 3, device=dev), torch.rand(16 << 4, 2, device=dev), scal, 4)
    assert out.shape == (0, 32)


@pytest.mark.parametrize("level", [0, 1])
def test_proposal_density_matches_oracle(dev, level):
    from uncertainty_nerf_gs_amd import ops
    t, sc, sd = _scene("active", dev)
    o, d = _rays()
    n = 256 if level == 0 else 96
    if level == 0:
        sb = O.initial_spacing_bins(n)
        sb_ref = sb[None].expand(o.shape[0], -1)
    else:
        g = torch.Generator().manual_seed(1)
        sb = torch.sort(torch.rand(o.shape[0], n + 1, generator=g), dim=-1).values
        sb_ref = sb
    eb = O.spacing_to_euclidean(sb_ref, NEAR, FAR)
    ref = O.density_field(O.sample_positions(o, d, eb), sc.prop_nets[level], 0.01)
    got = ops.proposal_density(o.to(dev), d.to(dev), sb.contiguous().to(dev), sd.props[level], NEAR, FAR, 0.01)
    _close(got, ref, 3e-5, 1e-9, f"proposal density level {level}")
    # the dense x-paired copy of the coarse levels is pure data movement: identical bits to the hashed lookup
    assert len(sd.props[level].dense_off) >= 3
    sd.props[level].use_dense = False
    hashed = ops.proposal_density(o.to(dev), d.to(dev), sb.contiguous().to(dev), sd.props[level], NEAR, FAR, 0.01)
    assert torch.equal(got, hashed)


@pytest.mark.parametrize("n,m", [(256, 96), (96, 48), (64, 32), (100, 48)])
def test_weights_pdf_resample_matches_oracle(dev, n, m):
    from uncertainty_nerf_gs_amd import ops, render
    g = torch.Generator().manual_seed(n + m)
    R = 203
    dens = torch.exp(torch.randn(R, n, generator=g) * 2.5)
    dens[0] = 0.0               # empty ray -> uniform resampling through the padding branch
    dens[1, : n // 2] = 0.0
    dens[2] = 1e4               # saturates immediately
    dens[3, 5] = float("inf")   # nan_to_num path
    sb = torch.sort(torch.rand(R, n + 1, generator=g), dim=-1).values
    sb[4] = O.initial_spacing_bins(n)
    eb = O.spacing_to_euclidean(sb, NEAR, FAR)
    w_ref = O.get_weights(dens, eb[:, 1:] - eb[:, :-1])
    new_ref = O.pdf_resample(w_ref, sb, m)
    pd_ref = O.render_depth_median(w_ref, (eb[:, :-1] + eb[:, 1:]) / 2)
    clip = ops.new_clip_buffer(R, 64, dev)
    new, pd, w = ops.weights_pdf_resample(dens.to(dev), sb.to(dev), render._pdf_u(m).to(dev), NEAR, FAR,
                                          want_weights=True, clip_minmax=clip, ray_offset=0, chunk_rays=64)
    _close(w, w_ref, 2e-5, 1e-7, "weights")
    _close(new, new_ref, 0, 3e-6, "resampled spacing bins", max_bad_frac=2e-4)
    assert torch.all(new[:, 1:] >= new[:, :-1]), "bins must stay sorted"
    # median depth picks a sample mid-point: identical except where cumsum(w) grazes 0.5
    _close(pd, pd_ref, 1e-5, 0, "prop depth", max_bad_frac=0.02)
    # per-chunk clip bounds == min / max of the new samples' mid-points over each 64-ray chunk
    eb_new = O.spacing_to_euclidean(new.cpu(), NEAR, FAR)
    steps = (eb_new[:, :-1] + eb_new[:, 1:]) / 2
    for c in range(clip.shape[0]):
        rows = steps[c * 64:(c + 1) * 64]
        assert abs(clip[c, 0].item() - rows.min().item()) <= 1e-6 * rows.min().item()
        assert abs(clip[c, 1].item() - rows.max().item()) <= 1e-6 * rows.max().item()


@pytest.mark.parametrize("chunk,offset", [(10, 7), (4, 0), (1, 3), (1000, 123)])
def test_pdf_clip_bounds_across_chunk_borders(dev, chunk, offset):
    """A block reduces the clip bounds of 32 rays before touching memory; chunk borders that fall inside a
    block (or inside one wave's ray sequence) must still land in the right [chunk] row, exactly."""
    from uncertainty_nerf_gs_amd import ops, render
    g = torch.Generator().manual_seed(chunk)
    R, n, m = 157, 96, 48
    dens = torch.exp(torch.randn(R, n, generator=g) * 2.5)
    sb = torch.sort(torch.rand(R, n + 1, generator=g), dim=-1).values
    n_chunks = (offset + R + chunk - 1) // chunk
    clip = torch.empty(n_chunks, 2, device=dev)
    clip[:, 0], clip[:, 1] = float("inf"), 0.0
    new, _, _ = ops.weights_pdf_resample(dens.to(dev), sb.to(dev), render._pdf_u(m).to(dev), NEAR, FAR,
                                         clip_minmax=clip, ray_offset=offset, chunk_rays=chunk)
    eb = O.spacing_to_euclidean(new.cpu(), NEAR, FAR)
    first, last = (eb[:, 0] + eb[:, 1]) / 2, (eb[:, -2] + eb[:, -1]) / 2
    want = torch.empty(n_chunks, 2)
    want[:, 0], want[:, 1] = float("inf"), 0.0
    for r in range(R):
        c = (offset + r) // chunk
        want[c, 0], want[c, 1] = min(want[c, 0], first[r]), max(want[c, 1], last[r])
    torch.testing.assert_close(clip.cpu(), want, rtol=1e-6, atol=0)


def test_weights_pdf_resample_shared_initial_bins(dev):
    from uncertainty_nerf_gs_amd import ops, render
    g = torch.Generator().manual_seed(5)
    dens = torch.exp(torch.randn(64, 256, generator=g) * 2)
    sb = O.initial_spacing_bins(256)
    eb = O.spacing_to_euclidean(sb[None].expand(64, -1), NEAR, FAR)
    ref = O.pdf_resample(O.get_weights(dens, eb[:, 1:] - eb[:, :-1]), sb[None].expand(64, -1), 96)
    new, _, _ = ops.weights_pdf_resample(dens.to(dev), sb.to(dev), render._pdf_u(96).to(dev), NEAR, FAR)
    _close(new, ref, 0, 3e-6, "bins from shared row", max_bad_frac=2e-4)


def _final_bins(sc, o, d):
    bins, wl, bl = O.proposal_sample(o, d, NEAR, FAR, sc.prop_nets, sc.num_prop, sc.num_nerf, 0.01)
    return bins.contiguous()


_KERNELS = [(True, "f16x2"), (True, "fp32"), (False, "fp32")]
_KERNEL_IDS = ["mfma-f16x2", "mfma-fp32", "valu"]


@pytest.mark.parametrize("use_mfma,precision", _KERNELS, ids=_KERNEL_IDS)
def test_field_active_matches_oracle(dev, use_mfma, precision):
    from uncertainty_nerf_gs_amd import ops
    t, sc, sd = _scene("active", dev)
    sd.field.use_mfma, sd.field.precision = use_mfma, precision
    o, d = _rays()
    sb = _final_bins(sc, o, d)
    eb = O.spacing_to_euclidean(sb, NEAR, FAR)
    dens_ref, rgb_ref, beta_ref = O.active_field(o, d, eb, sc.field)
    dens, rgb, beta, _ = ops.field_fwd(o.to(dev), d.to(dev), sb.to(dev), sd.field, NEAR, FAR)
    _close(dens[0], dens_ref, 2e-4, 1e-7, "density")
    _close(rgb[0], rgb_ref, 0, 2e-5, "rgb")
    _close(beta, beta_ref, 1e-4, 1e-6, "beta")


@pytest.mark.parametrize("kind,kw", [("active", {}), ("mcdropout", dict(K=2, seed=5, p_drop=0.2))])
def test_field_level_major_gather_equals_fused_lookup(dev, kind, kw):
    """unerf_field_gather + unerf_field_fwd(features=...) == the fused kernel, bit for bit, and the
    feature planes equal the stand-alone hash grid of the oracle positions."""
    from uncertainty_nerf_gs_amd import ops
    t, sc, sd = _scene(kind, dev, **kw)
    o, d = _rays(20, 28)
    sb = _final_bins(sc, o, d)
    od, dd, sbd = o.to(dev), d.to(dev), sb.to(dev)
    feats = ops.field_gather(od, dd, sbd, sd.field, NEAR, FAR)
    eb = O.spacing_to_euclidean(sb, NEAR, FAR)
    p, _ = O.normalized_positions(O.sample_positions(o, d, eb))
    ref = O.hash_encode(p.reshape(-1, 3), sc.field.grid.table, sc.field.grid.scalings, sc.field.grid.log2_T)
    assert torch.equal(feats.permute(1, 0, 2).reshape(-1, 32).cpu(), ref)
    sd.field.precision = "fp32"   # feature planes feed the exact-fp32 MFMA kernel
    a = ops.field_fwd(od, dd, sbd, sd.field, NEAR, FAR, ray_offset=3)
    b = ops.field_fwd(od, dd, sbd, sd.field, NEAR, FAR, ray_offset=3, features=feats)
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y)


@pytest.mark.parametrize("use_mfma,precision", _KERNELS, ids=_KERNEL_IDS)
@pytest.mark.parametrize("K", [0, 3, 8, 10])
def test_field_mcdropout_matches_oracle(dev, K, use_mfma, precision):
    """K = 8 is the BASELINE config, K = 10 the reference default (mcdropout_models.py:45): pass k's masks are k
    chained mask steps, so every pass up to the largest K in use is compared with the oracle."""
    from uncertainty_nerf_gs_amd import ops
    seed, p = 1234, 0.2
    t, sc, sd = _scene("mcdropout", dev, K=K, seed=seed, p_drop=p)
    sd.field.use_mfma, sd.field.precision = use_mfma, precision
    o, d = _rays(16, 24)
    sb = _final_bins(sc, o, d)
    eb = O.spacing_to_euclidean(sb, NEAR, FAR)
    ray_offset = 1000
    dens, rgb, _, _ = ops.field_fwd(o.to(dev), d.to(dev), sb.to(dev), sd.field, NEAR, FAR, ray_offset=ray_offset)
    R, S = sb.shape[0], sb.shape[1] - 1
    assert dens.shape == (max(K, 1), R, S)
    sidx = ((np.arange(R)[:, None] + ray_offset) * S + np.arange(S)[None]).reshape(-1)
    for k in range(max(K, 1)):
        kt = kh = None
        if K > 0:
            kt = torch.from_numpy(O.mc_keep_mask(seed, k, sidx, 0, 64, p))
            kh = torch.from_numpy(O.mc_keep_mask(seed, k, sidx, 1, 64, p))
            assert 0.75 < kt.float().mean() < 0.85
        dr, cr = O.mcdropout_field(o, d, eb, sc.field, kt, kh, p)
        _close(dens[k], dr, 2e-4, 1e-7, f"density pass {k}")
        _close(rgb[k], cr, 0, 2e-5, f"rgb pass {k}")
    if K > 1:
        assert not torch.equal(dens[0], dens[1]), "passes must use different masks"


@pytest.mark.parametrize("use_mfma,precision", _KERNELS, ids=_KERNEL_IDS)
@pytest.mark.parametrize("sites", [1, 4, 2, 6, 7])
def test_field_mcdropout_dropout_sites_match_oracle(dev, sites, use_mfma, precision):
    """Non-default placements of the Dropout modules (mcdropout_fields.py:112-144 through create_mlp):
    density_dropout_layers=False (no trunk mask), rgb_dropout_layers containing 1 (masks in front of the head's
    Linear 1, RNG stream 2) and / or -1 (in front of the last Linear) -- unerf_field_params.drop_sites"""
    from uncertainty_nerf_gs_amd import ops
    K, seed, p = 3, 77, 0.25
    t, sc, sd = _scene("mcdropout", dev, K=K, seed=seed, p_drop=p, drop_sites=sites)
    sd.field.use_mfma, sd.field.precision = use_mfma, precision
    o, d = _rays(12, 20)
    sb = _final_bins(sc, o, d)
    eb = O.spacing_to_euclidean(sb, NEAR, FAR)
    dens, rgb, _, _ = ops.field_fwd(o.to(dev), d.to(dev), sb.to(dev), sd.field, NEAR, FAR, ray_offset=64)
    R, S = sb.shape[0], sb.shape[1] - 1
    sidx = ((np.arange(R)[:, None] + 64) * S + np.arange(S)[None]).reshape(-1)
    for k in range(K):
        m = lambda stream, bit: torch.from_numpy(O.mc_keep_mask(seed, k, sidx, stream, 64, p)) if sites & bit else None
        dr, cr = O.mcdropout_field(o, d, eb, sc.field, m(0, 1), m(1, 4), p, keep_head0=m(2, 2))
        _close(dens[k], dr, 2e-4, 1e-7, f"density pass {k}")
        _close(rgb[k], cr, 0, 2e-5, f"rgb pass {k}")
    if not sites & 1:
        assert torch.equal(dens[0], dens[1]), "no trunk dropout: the density is the same in every pass"
    assert not torch.equal(rgb[0], rgb[1])
    # changing the sites after the operands were packed (the scale lives in other layers) is refused on the f16 path
    if precision == "f16x2" and use_mfma:
        sd.field.drop_sites = 5 if sites != 5 else 1
        with pytest.raises(Exception, match="rebuild the FieldDev"):
            ops.field_fwd(o.to(dev), d.to(dev), sb.to(dev), sd.field, NEAR, FAR)


@pytest.mark.parametrize("precision", ["f16x2", "f16", "fp32"])
@pytest.mark.parametrize("sites", [8, 13, 15])
def test_field_mcdropout_dropout_on_the_head_inputs(dev, sites, precision):
    """rgb_dropout_layers containing 0 (create_mlp, utils.py:24-25): a Dropout in front of the colour head's Linear 0,
    i.e. on its 63 inputs [SH16 | geo15 | appearance32] -- UNERF_DROP_HEADIN, mask stream 3.  The appearance block then
    cannot ride in the bias; the site is served by the VALU kernel whatever precision is configured.  A non-zero eval
    embedding (use_average_appearance_embedding) makes the appearance masks matter."""
    from uncertainty_nerf_gs_amd import ops, synthetic
    K, seed, p = 3, 41, 0.25
    t = synthetic.make_scene_tensors(seed=0, kind="mcdropout", log2T=14, prop_log2T=12)
    t["field"]["appearance"] = torch.linspace(-0.6, 0.9, 32)         # a mean embedding that is far from zero
    sc = O.scene_from_tensors(t)
    sd = synthetic.scene_to_device(t, dev, K=K, seed=seed, p_drop=p, drop_sites=sites)
    sd.field.precision = precision
    o, d = _rays(12, 20)
    sb = _final_bins(sc, o, d)
    eb = O.spacing_to_euclidean(sb, NEAR, FAR)
    dens, rgb, _, _ = ops.field_fwd(o.to(dev), d.to(dev), sb.to(dev), sd.field, NEAR, FAR, ray_offset=64)
    R, S = sb.shape[0], sb.shape[1] - 1
    sidx = ((np.arange(R)[:, None] + 64) * S + np.arange(S)[None]).reshape(-1)
    for k in range(K):
        m = lambda stream, bit: torch.from_numpy(O.mc_keep_mask(seed, k, sidx, stream, 64, p)) if sites & bit else None
        kin = m(3, 8)
        dr, cr = O.mcdropout_field(o, d, eb, sc.field, m(0, 1), m(1, 4), p, keep_head0=m(2, 2), keep_in=kin[:, :63])
        _close(dens[k], dr, 2e-4, 1e-7, f"density pass {k}")
        _close(rgb[k], cr, 0, 2e-5, f"rgb pass {k}")
        # and the masks do act: without them the colours differ
        _, c0 = O.mcdropout_field(o, d, eb, sc.field, m(0, 1), m(1, 4), p, keep_head0=m(2, 2))
        assert float((c0 - cr).abs().max()) > 1e-3
    assert not torch.equal(rgb[0], rgb[1])


@pytest.mark.parametrize("use_mfma,precision,n_samples",
                         [(True, "f16x2", 100), (True, "fp32", 100), (False, "fp32", 100), (True, "f16x2", 37),
                          (True, "fp32", 37), (True, "f16x2", 128), (True, "f16x2", 4)],
                         ids=["mfma16-100", "mfma32-100", "valu-100", "mfma16-37", "mfma32-37", "mfma16-128", "mfma16-4"])
def test_field_laplace_matches_oracle(dev, use_mfma, precision, n_samples):
    from uncertainty_nerf_gs_amd import ops, synthetic
    t, sc, _ = _scene("laplace", dev)
    wsd, wsr = synthetic.laplace_weight_samples(t, seed=42, n_samples=n_samples)
    sd = synthetic.scene_to_device(t, dev, ws_density=wsd.to(dev), ws_rgb=wsr.to(dev))
    sd.field.use_mfma, sd.field.precision = use_mfma, precision
    assert sd.field.lap_blob is not None and sd.field.lap16_blob is not None
    o, d = _rays(12, 16)
    sb = _final_bins(sc, o, d)
    eb = O.spacing_to_euclidean(sb, NEAR, FAR)
    mu_d, var_d, mu_rgb, var_rgb = O.laplace_field(o, d, eb, sc.field, wsd, wsr)
    dens, rgb, dvar, rvar = ops.field_fwd(o.to(dev), d.to(dev), sb.to(dev), sd.field, NEAR, FAR)
    _close(dens[0], mu_d, 2e-4, 1e-7, "mu_d")
    _close(rgb[0], mu_rgb, 0, 2e-5, "mu_rgb")
    # variances are E[x^2]-E[x]^2 in fp32: compare against the scale of E[x^2]
    _close(dvar, var_d, 0, 2e-5 * float((mu_d ** 2).max()), "var_d")
    _close(rvar, var_rgb, 0, 2e-6, "var_rgb")


@pytest.mark.parametrize("use_mfma,precision", [(True, "f16x2"), (True, "f16"), (True, "fp32"), (False, "fp32")],
                         ids=["mfma16", "mfma16-f16", "mfma32", "valu"])
@pytest.mark.parametrize("kind", ["active", "mcdropout"])
def test_packed_output_rows_hold_the_same_bits(dev, kind, use_mfma, precision):
    """unerf_field_params.packed_out: one 16-byte row (sigma, r, g, b) per (pass, ray, sample) instead of a dword into
    `density` and three into `rgb` -- the same values bit for bit from every kernel set, with and without the pixel-patch
    tile schedule, and the composite entry points give the same images from either layout."""
    from uncertainty_nerf_gs_amd import ops, synthetic
    kw = dict(K=3, seed=5, p_drop=0.2) if kind == "mcdropout" else {}
    t, sc, sd = _scene(kind, dev, **kw)
    sd.field.use_mfma, sd.field.precision = use_mfma, precision
    H, W = 12, 40
    o, d = _rays(H, W)
    sb = _final_bins(sc, o, d).to(dev)
    o, d = o.to(dev), d.to(dev)
    for iw in (0, W):
        dens, rgb, aux, _ = ops.field_fwd(o, d, sb, sd.field, NEAR, FAR, image_width=iw)
        none, rows, aux2, _ = ops.field_fwd(o, d, sb, sd.field, NEAR, FAR, image_width=iw, packed=True)
        assert none is None and rows.shape == dens.shape + (4,)
        assert torch.equal(rows[..., 0], dens) and torch.equal(rows[..., 1:], rgb)
        assert (aux is None and aux2 is None) or torch.equal(aux, aux2)
    if kind == "active":
        a = ops.composite_var(dens, rgb, sb, NEAR, FAR, beta=aux)
        b = ops.composite_var(None, rows, sb, NEAR, FAR, beta=aux)
        assert torch.equal(a, b)
    else:
        for x, y in zip(ops.composite_moments(dens, rgb, sb, NEAR, FAR), ops.composite_moments(None, rows, sb, NEAR, FAR)):
            assert torch.equal(x, y)
        assert torch.equal(ops.composite_var(dens, rgb, sb, NEAR, FAR), ops.composite_var(None, rows, sb, NEAR, FAR))


@pytest.mark.parametrize("use_mfma,precision", [(True, "f16x2"), (True, "f16"), (True, "fp32"), (False, "fp32")],
                         ids=["mfma16", "mfma16-f16", "mfma32", "valu"])
def test_field_laplace_per_chunk_sample_sets(dev, use_mfma, precision):
    """unerf_field_params.lap_chunk_rays: the reference draws a fresh set of last-layer samples in every eval chunk
    (laplace_model.py:432-443 -> laplace_field.py:331-339, 468-476, 545).  A stack of sets [sets, n, P]; ray g is
    evaluated with set g // lap_chunk_rays -- checked per chunk against the oracle with that chunk's set, with a ray
    offset (a later launch group of a frame) and a ragged last chunk; rays beyond the stack are refused."""
    from uncertainty_nerf_gs_amd import lib as L, ops, synthetic
    t, sc, _ = _scene("laplace", dev)
    chunk, n = 64, 40
    H, W = 10, 23                               # 230 rays = 3 chunks of 64 + 38
    o, d = _rays(H, W)
    R = o.shape[0]
    off = 3 * chunk                             # this launch starts at chunk 3 of its frame
    sets = off // chunk + -(-R // chunk)
    ws = [synthetic.laplace_weight_samples(t, seed=100 + i, n_samples=n) for i in range(sets)]
    wsd, wsr = torch.stack([w[0] for w in ws]), torch.stack([w[1] for w in ws])
    sd = synthetic.scene_to_device(t, dev, ws_density=wsd.to(dev), ws_rgb=wsr.to(dev), lap_chunk_rays=chunk)
    sd.field.use_mfma, sd.field.precision = use_mfma, precision
    assert sd.field.lap_blob.shape == sd.field.lap16_blob.shape == (sets, ops.LAP_BLOB_FLOATS)
    sb = _final_bins(sc, o, d)
    eb = O.spacing_to_euclidean(sb, NEAR, FAR)
    dens, rgb, dvar, rvar = ops.field_fwd(o.to(dev), d.to(dev), sb.to(dev), sd.field, NEAR, FAR, ray_offset=off, image_width=W)
    f16 = precision == "f16"
    for c in range(-(-R // chunk)):
        sl = slice(c * chunk, min(R, (c + 1) * chunk))
        mu_d, var_d, mu_rgb, var_rgb = O.laplace_field(o[sl], d[sl], eb[sl], sc.field, wsd[off // chunk + c], wsr[off // chunk + c])
        _close(dens[0][sl], mu_d, 2e-3 if f16 else 2e-4, 1e-7, f"mu_d chunk {c}")
        _close(rgb[0][sl], mu_rgb, 0, 2e-4 if f16 else 2e-5, f"mu_rgb chunk {c}")
        _close(rvar[sl], var_rgb, 0, 2e-5 if f16 else 2e-6, f"var_rgb chunk {c}")
        if c > 0:    # the sets differ: chunk c evaluated with chunk 0's set is somewhere else
            other = O.laplace_field(o[sl], d[sl], eb[sl], sc.field, wsd[off // chunk], wsr[off // chunk])[2]
            assert float((other - mu_rgb).abs().max()) > 1e-3
    with pytest.raises(L.UnerfError, match="reach past"):
        ops.field_fwd(o.to(dev), d.to(dev), sb.to(dev), sd.field, NEAR, FAR, ray_offset=off + chunk)
    with pytest.raises(L.UnerfError, match="multiples of 32"):
        ops.field_fwd(o.to(dev), d.to(dev), sb.to(dev), sd.field, NEAR, FAR, ray_offset=8)


@pytest.mark.parametrize("use_mfma,precision", _KERNELS, ids=_KERNEL_IDS)
def test_field_laplace_softplus_density_activation(dev, use_mfma, precision):
    """density_activation = "softplus" (laplace_model.py:151): the sampled density head goes through softplus instead
    of trunc_exp, in the sampling path and in the use_deterministic_density path"""
    from uncertainty_nerf_gs_amd import ops, synthetic
    import copy
    t, sc, _ = _scene("laplace", dev)
    wsd, wsr = synthetic.laplace_weight_samples(t, seed=42, n_samples=50)
    sd = synthetic.scene_to_device(t, dev, ws_density=wsd.to(dev), ws_rgb=wsr.to(dev), lap_softplus=1)
    sd.field.use_mfma, sd.field.precision = use_mfma, precision
    o, d = _rays(10, 16)
    sb = _final_bins(sc, o, d)
    eb = O.spacing_to_euclidean(sb, NEAR, FAR)
    fp = copy.copy(sc.field)
    fp.density_activation = "softplus"
    mu_d, var_d, mu_rgb, var_rgb = O.laplace_field(o, d, eb, fp, wsd, wsr)
    dens, rgb, dvar, rvar = ops.field_fwd(o.to(dev), d.to(dev), sb.to(dev), sd.field, NEAR, FAR)
    _close(dens[0], mu_d, 2e-4, 1e-6, "mu_d (softplus)")
    _close(dvar, var_d, 0, 2e-5 * float((mu_d ** 2).max()), "var_d")
    _close(rgb[0], mu_rgb, 0, 2e-5, "mu_rgb")
    exp_fp = copy.copy(sc.field)
    assert not torch.allclose(O.laplace_field(o, d, eb, exp_fp, wsd, wsr)[0], mu_d)      # the activation matters
    # GGN fitting takes the activation's derivative (1 - exp(-sigma) instead of sigma); the values are checked against
    # autograd in tests/test_gpu_models.py::test_laplace_compute_hessian_naive_matches_autograd_oracle[softplus]
    gd, gr = torch.zeros(65, device=dev), torch.zeros(195, device=dev)
    ops.laplace_ggn_diag(o.to(dev), d.to(dev), sb.to(dev), sd.field, wsd[0], wsr[0], NEAR, FAR, gd, gr)
    assert torch.isfinite(gd).all() and torch.isfinite(gr).all() and gd.abs().sum() > 0


@pytest.mark.parametrize("B,S", [(1, 48), (3, 48), (1, 96), (2, 16), (1, 256),
                                 (1, 50), (2, 17), (1, 7), (1, 2), (1, 40), (1, 70), (1, 100), (1, 150), (1, 255)])
def test_composite_var_matches_oracle(dev, B, S):
    """S = 16 k: the aligned kernels; every other S: the RAGGED ones (masked trailing slots)"""
    from uncertainty_nerf_gs_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + S)
    R = 131
    dens = torch.exp(torch.randn(B, R, S, generator=g) * 2.0)
    dens[:, 0] = 0.0
    dens[:, 1, S // 3:] = 1e5
    rgb = torch.rand(B, R, S, 3, generator=g)
    rgb[0, 2, min(3, S - 1), 1] = float("nan")
    beta = torch.rand(R, S, generator=g) + 0.01
    sb = torch.sort(torch.rand(R, S + 1, generator=g), dim=-1).values
    eb = O.spacing_to_euclidean(sb, NEAR, FAR)
    deltas, steps = eb[:, 1:] - eb[:, :-1], (eb[:, :-1] + eb[:, 1:]) / 2
    chunk = 50
    clip = torch.empty((R + chunk - 1) // chunk, 2)
    for c in range(clip.shape[0]):
        clip[c, 0], clip[c, 1] = steps[c * chunk:(c + 1) * chunk].min(), steps[c * chunk:(c + 1) * chunk].max()
    out = ops.composite_var(dens.to(dev), rgb.to(dev), sb.to(dev), NEAR, FAR, beta=beta.to(dev),
                            clip_minmax=clip.to(dev), ray_offset=0, chunk_rays=chunk).cpu()
    for b in range(B):
        w = O.get_weights(dens[b], deltas)
        _close(out[b, :, 0:3], O.render_rgb(rgb[b], w), 0, 3e-6, "rgb")
        _close(out[b, :, 3:4], O.render_accumulation(w), 2e-6, 1e-7, "accumulation")
        depth_ref = O.render_depth_median(w, steps)
        _close(out[b, :, 4:5], depth_ref, 1e-6, 0, "median depth", max_bad_frac=0.02)
        ed = torch.cat([O.render_depth_expected(w[c * chunk:(c + 1) * chunk], steps[c * chunk:(c + 1) * chunk])
                        for c in range(clip.shape[0])])
        _close(out[b, :, 5:6], ed, 2e-5, 1e-6, "expected depth")
        _close(out[b, :, 6:7], O.render_uncertainty(beta, w ** 2), 2e-5, 1e-8, "rgb_var")
        same = (out[b, :, 4:5] - depth_ref).abs() <= 1e-6 * depth_ref.abs()
        dv_ref = torch.sum(w * (steps - depth_ref) ** 2, dim=-1, keepdim=True) + 1e-5
        _close(out[b, :, 7:8][same], dv_ref[same], 5e-5, 1e-7, "depth_var")


@pytest.mark.parametrize("B,S", [(1, 48), (3, 48), (2, 17), (1, 2), (5, 96), (9, 40)])
def test_composite_planes_match_oracle_and_the_group_kernels(dev, B, S):
    """sample-major planes + one lane per ray (unerf_composite_var_planes / _moments_planes): against the oracle's
    renderers, and against the 16-lanes-per-ray kernels on the transposed data"""
    from uncertainty_nerf_gs_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + S)
    R = 333
    dens = torch.exp(torch.randn(B, R, S, generator=g) * 2.0)
    dens[:, 0] = 0.0
    dens[:, 1, S // 3:] = 1e5
    dens[:, 4, min(2, S - 1)] = float("inf")
    rgb = torch.rand(B, R, S, 3, generator=g)
    rgb[0, 2, min(3, S - 1), 1] = float("nan")
    beta = torch.rand(R, S, generator=g) + 0.01
    sb = torch.sort(torch.rand(R, S + 1, generator=g), dim=-1).values
    eb = O.spacing_to_euclidean(sb, NEAR, FAR)
    deltas, steps = eb[:, 1:] - eb[:, :-1], (eb[:, :-1] + eb[:, 1:]) / 2
    chunk = 100
    clip = torch.empty((R + chunk - 1) // chunk, 2)
    for c in range(clip.shape[0]):
        clip[c, 0], clip[c, 1] = steps[c * chunk:(c + 1) * chunk].min(), steps[c * chunk:(c + 1) * chunk].max()
    dp = dens.permute(0, 2, 1).contiguous().to(dev)               # [B,S,R]
    cp = rgb.permute(0, 2, 3, 1).contiguous().to(dev)             # [B,S,3,R]
    bp = beta.t().contiguous().to(dev)                            # [S,R]
    kw = dict(clip_minmax=clip.to(dev), ray_offset=0, chunk_rays=chunk)
    out = ops.composite_var_planes(dp, cp, sb.to(dev), NEAR, FAR, beta=bp, **kw).cpu()
    for b in range(B):
        w = O.get_weights(dens[b], deltas)
        _close(out[b, :, 0:3], O.render_rgb(rgb[b], w), 0, 3e-6, "rgb")
        _close(out[b, :, 3:4], O.render_accumulation(w), 2e-6, 1e-7, "accumulation")
        depth_ref = O.render_depth_median(w, steps)
        _close(out[b, :, 4:5], depth_ref, 1e-6, 0, "median depth", max_bad_frac=0.02)
        ed = torch.cat([O.render_depth_expected(w[c * chunk:(c + 1) * chunk], steps[c * chunk:(c + 1) * chunk])
                        for c in range(clip.shape[0])])
        _close(out[b, :, 5:6], ed, 2e-5, 1e-6, "expected depth")
        _close(out[b, :, 6:7], O.render_uncertainty(beta, w ** 2), 2e-5, 1e-8, "rgb_var")
        same = (out[b, :, 4:5] - depth_ref).abs() <= 1e-6 * depth_ref.abs()
        dv_ref = torch.sum(w.double() * (steps.double() - depth_ref.double()) ** 2, dim=-1, keepdim=True) + 1e-5
        _close(out[b, :, 7:8][same], dv_ref[same].float(), 5e-5, 1e-7, "depth_var")
    old = ops.composite_var(dens.to(dev), rgb.to(dev), sb.to(dev), NEAR, FAR, beta=beta.to(dev), **kw).cpu()
    fin = torch.isfinite(old) & torch.isfinite(out)
    assert fin.float().mean() > 0.98
    same_depth = (old[..., 4] - out[..., 4]).abs() <= 1e-6 * old[..., 4].abs()
    assert same_depth.float().mean() >= 0.98                     # a cumsum grazing 0.5 may pick the neighbouring sample
    for c, (rt, at) in enumerate([(0, 3e-6)] * 3 + [(2e-6, 1e-7), (1e-6, 0), (2e-5, 1e-6), (2e-5, 1e-8), (1e-4, 1e-7)]):
        m = same_depth & fin[..., c]
        _close(out[..., c][m], old[..., c][m], rt, at, f"planes vs groups, channel {c}", max_bad_frac=2e-3 if c == 5 else 0.0)
    if B >= 2:
        mean, var = ops.composite_moments_planes(dp, cp, sb.to(dev), NEAR, FAR, **kw)
        ref_out = ops.composite_var_planes(dp, cp, sb.to(dev), NEAR, FAR, **kw).cpu().double()     # beta = None here
        ok = torch.isfinite(ref_out).all(dim=0)
        m_ref, v_ref = ref_out.mean(dim=0), ref_out.var(dim=0)
        _close(mean.cpu()[ok], m_ref[ok].float(), 2e-6, 1e-7, "mean over passes")
        _close(var.cpu()[ok], v_ref[ok].float(), 1e-4, 1e-9 + 1e-6 * float(v_ref[ok].max()), "unbiased variance over passes")


@pytest.mark.parametrize("kind,kw,image_width", [("active", {}, 0), ("active", {}, 24), ("mcdropout", dict(K=3, seed=5, p_drop=0.2), 24)])
@pytest.mark.parametrize("precision", ["f16x2", "fp32"])
def test_field_sample_major_planes_equal_the_ray_major_outputs(dev, kind, kw, image_width, precision):
    """unerf_field_params.sample_major only changes WHERE a value is stored: planes == transposed ray-major, bit for bit"""
    from uncertainty_nerf_gs_amd import ops
    t, sc, sd = _scene(kind, dev, **kw)
    sd.field.precision = precision
    o, d = _rays(20, 24)
    sb = _final_bins(sc, o, d)
    od, dd, sbd = o.to(dev), d.to(dev), sb.to(dev)
    a = ops.field_fwd(od, dd, sbd, sd.field, NEAR, FAR, ray_offset=480, image_width=image_width)
    b = ops.field_fwd(od, dd, sbd, sd.field, NEAR, FAR, ray_offset=480, image_width=image_width, sample_major=True)
    assert b[0].shape == a[0].permute(0, 2, 1).shape and torch.equal(b[0], a[0].permute(0, 2, 1))
    assert torch.equal(b[1], a[1].permute(0, 2, 3, 1))
    if kind == "active":
        assert torch.equal(b[2], a[2].t())
    # planes are refused where no kernel writes them
    sd.field.use_mfma = False
    with pytest.raises(Exception, match="sample_major"):
        ops.field_fwd(od, dd, sbd, sd.field, NEAR, FAR, sample_major=True)


@pytest.mark.parametrize("S", [48, 50, 21])
def test_composite_var_weights_alt(dev, S):
    """laplace: rgb / rgb_var from get_weights(mu_d), depth-side outputs from the mean sampled weights"""
    from uncertainty_nerf_gs_amd import ops
    g = torch.Generator().manual_seed(77)
    R = 64
    dens = torch.exp(torch.randn(1, R, S, generator=g))
    rgb = torch.rand(1, R, S, 3, generator=g)
    var = torch.rand(R, S, generator=g) * 0.01
    walt = torch.rand(R, S, generator=g) / S
    sb = torch.sort(torch.rand(R, S + 1, generator=g), dim=-1).values
    eb = O.spacing_to_euclidean(sb, NEAR, FAR)
    deltas, steps = eb[:, 1:] - eb[:, :-1], (eb[:, :-1] + eb[:, 1:]) / 2
    out = ops.composite_var(dens.to(dev), rgb.to(dev), sb.to(dev), NEAR, FAR, beta=var.to(dev),
                            weights_alt=walt.to(dev)).cpu()[0]
    w = O.get_weights(dens[0], deltas)
    _close(out[:, 0:3], O.render_rgb(rgb[0], w), 0, 3e-6, "rgb")
    _close(out[:, 6:7], O.render_uncertainty(var, w ** 2), 2e-5, 1e-9, "rgb_var")
    _close(out[:, 3:4], O.render_accumulation(walt), 2e-6, 1e-7, "accumulation(alt)")
    _close(out[:, 4:5], O.render_depth_median(walt, steps), 1e-6, 0, "depth(alt)", max_bad_frac=0.02)


@pytest.mark.parametrize("S", [48, 50, 9])
@pytest.mark.parametrize("explicit_noise", [True, False])
def test_laplace_depth_weights_matches_oracle(dev, explicit_noise, S):
    from uncertainty_nerf_gs_amd import ops
    g = torch.Generator().manual_seed(3)
    R, D = 40, 100
    mu = torch.exp(torch.randn(R, S, generator=g))
    var = torch.rand(R, S, generator=g) * mu ** 2
    var[0, 0] = -1e-3   # sqrt -> NaN -> 1e-10 (laplace_model.py:489-494)
    var[0, 1] = 0.0
    sb = torch.sort(torch.rand(R, S + 1, generator=g), dim=-1).values
    eb = O.spacing_to_euclidean(sb, NEAR, FAR)
    deltas = eb[:, 1:] - eb[:, :-1]
    seed, off = 99, 17
    if explicit_noise:
        noise = torch.randn(D, R, S, generator=g)
    else:
        sidx = ((np.arange(R)[:, None] + off) * S + np.arange(S)[None]).reshape(-1)
        noise = torch.from_numpy(np.stack([O.normal_noise(seed, dd, sidx).reshape(R, S) for dd in range(D)]))
        assert abs(noise.mean().item()) < 0.03 and abs(noise.std().item() - 1) < 0.03
    sd = var.sqrt()
    sd = torch.where(torch.isnan(sd), torch.tensor(1e-10), torch.clamp_min(sd, 1e-10))
    samp = torch.relu(mu[None] + sd[None] * noise)
    ref = torch.stack([O.get_weights(samp[i], deltas) for i in range(D)]).mean(0)
    got = ops.laplace_depth_weights(mu.to(dev), var.to(dev), sb.to(dev), NEAR, FAR,
                                    noise.to(dev) if explicit_noise else None, D, seed, off)
    _close(got, ref, 3e-4 if not explicit_noise else 3e-5, 2e-7, "mean sampled weights")


@pytest.mark.parametrize("B,S", [(8, 48), (2, 48), (16, 16), (1, 48), (4, 50), (3, 5), (2, 130)])
def test_composite_moments_equals_composite_then_moments(dev, B, S):
    """fused K-pass composite + mean/var == per-pass composite followed by torch mean / var"""
    from uncertainty_nerf_gs_amd import ops
    g = torch.Generator().manual_seed(B * 100 + S)
    R = 77
    dens = torch.exp(torch.randn(B, R, S, generator=g) * 2.0).to(dev)
    rgb = torch.rand(B, R, S, 3, generator=g).to(dev)
    sb = torch.sort(torch.rand(R, S + 1, generator=g), dim=-1).values.to(dev)
    per = ops.composite_var(dens, rgb, sb, NEAR, FAR)          # [B,R,8]
    mean, var = ops.composite_moments(dens, rgb, sb, NEAR, FAR)
    _close(mean, per.mean(0), 2e-6, 1e-7, "mean over passes")
    if B > 1:
        _close(var[:, :6], per.var(0)[:, :6], 2e-4, 1e-9, "unbiased variance over passes")
    else:
        assert torch.isnan(var).all()   # torch.var of a single sample


@pytest.mark.parametrize("K", [2, 8])
def test_moments_matches_torch(dev, K):
    from uncertainty_nerf_gs_amd import ops
    g = torch.Generator().manual_seed(K)
    x = torch.rand(K, 1000, 6, generator=g)
    mean, var = ops.moments(x.to(dev))
    _close(mean, x.mean(0), 1e-6, 1e-7, "mean")
    _close(var, x.var(0), 2e-5, 1e-8, "var")


def test_laplace_ggn_diag_kernels_match_autograd(dev):
    """unerf_laplace_ggn_diag on the oracle's own sample bins (isolates the capture + Jacobian kernels from
    the sampler): diag GGN = 2 sum J^2 vs one autograd backward per rendered value (laplace_model.py:343-400)."""
    from uncertainty_nerf_gs_amd import ops, synthetic
    t = synthetic.make_scene_tensors(seed=11, kind="laplace", log2T=14, prop_log2T=12)
    sc = O.scene_from_tensors(t)
    sd = synthetic.scene_to_device(t, dev)
    H, W = 5, 7   # 35 rays: one full 32-ray tile block + a ragged one
    o, d, _ = O.generate_rays(synthetic.orbit_c2w(1.1), 0.9 * W, 0.9 * W, W / 2, H / 2, H, W)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    want_d, want_r = O.laplace_ggn_diag(sc, o, d)
    bins, _, _ = O.proposal_sample(o, d, sc.near, sc.far, sc.prop_nets, sc.num_prop, sc.num_nerf,
                                   sc.prop_average_init_density)
    f = t["field"]
    dm = torch.cat([f["density_w"].reshape(-1), f["density_b"].reshape(-1)])
    rm = torch.cat([f["head_w"][2].reshape(-1), f["head_b"][2].reshape(-1)])
    gd, gr = torch.zeros(65, device=dev), torch.zeros(195, device=dev)
    for _ in range(2):   # accumulates: two identical batches = twice the single-batch GGN
        ops.laplace_ggn_diag(o.to(dev), d.to(dev), bins.to(dev).contiguous(), sd.field, dm, rm, sc.near, sc.far, gd, gr)
    # fp32 Jacobian sums with cancellation (the d/dsigma bracket) against float32 autograd: entries far below the
    # largest one carry ~1e-3 relative noise on both sides
    torch.testing.assert_close(gd.cpu() / 2, want_d, rtol=2e-3, atol=2e-5 * want_d.max().item())
    torch.testing.assert_close(gr.cpu() / 2, want_r, rtol=2e-3, atol=2e-5 * want_r.max().item())
    assert (gd >= 0).all() and (gr >= 0).all()
    # argument checking: wrong mode / short workspace are reported, not executed
    from uncertainty_nerf_gs_amd import lib as L
    with pytest.raises(L.UnerfError):
        ops.laplace_ggn_diag(o.to(dev), d.to(dev), bins.to(dev).contiguous(), sd.field, dm[:10], rm, sc.near, sc.far, gd, gr)


@pytest.mark.parametrize("kind,kw", [("active", {}), ("mcdropout", dict(K=4, seed=3, p_drop=0.2))])
def test_split_f16_matrix_kernels_are_fp32_equivalent(dev, kind, kw):
    """The split-f16 kernels (hi/lo halves, three products, fp32 accumulate) against the exact fp32-MFMA kernels
    on identical inputs: the deviation must stay at the level of fp32 rounding itself, far inside the tolerance
    either kernel is held to against the oracle."""
    from uncertainty_nerf_gs_amd import ops
    t, sc, sd = _scene(kind, dev, **kw)
    o, d = _rays(24, 32)
    sb = _final_bins(sc, o, d)
    args = (o.to(dev), d.to(dev), sb.to(dev), sd.field, NEAR, FAR)
    sd.field.precision = "fp32"
    exact = ops.field_fwd(*args, ray_offset=77)
    sd.field.precision = "f16x2"
    split = ops.field_fwd(*args, ray_offset=77)
    dens_e, dens_s = exact[0].double(), split[0].double()
    assert ((dens_s - dens_e).abs() <= 3e-6 * dens_e.abs() + 1e-9).all(), ((dens_s - dens_e).abs() / (dens_e.abs() + 1e-9)).max()
    assert (split[1] - exact[1]).abs().max() <= 1e-6, (split[1] - exact[1]).abs().max()
    if kind == "active":
        assert (split[2] - exact[2]).abs().max() <= 2e-6 * exact[2].abs().max()


@pytest.mark.parametrize("kind,kw,precision", [("active", {}, "f16x2"), ("active", {}, "fp32"),
                                               ("mcdropout", dict(K=2, seed=11, p_drop=0.2), "f16x2")])
@pytest.mark.parametrize("W,R,offset", [(40, 40 * 9, 0), (37, 37 * 6 + 5, 37 * 3 + 11), (64, 300, 64 * 2), (8, 8 * 4, 8)])
def test_pixel_patch_tiles_change_nothing(dev, kind, kw, precision, W, R, offset):
    """image_width only regroups the 32 columns of a tile into 8x4 pixel patches (a locality hint): every
    (ray, sample) result must be bit-identical, for ragged widths, partial bands and mid-row offsets."""
    from uncertainty_nerf_gs_amd import ops
    t, sc, sd = _scene(kind, dev, **kw)
    sd.field.precision = precision
    g = torch.Generator().manual_seed(W * 1000 + R)
    o = torch.randn(R, 3, generator=g) * 0.3
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    sb = _final_bins(sc, o, d)
    args = (o.to(dev), d.to(dev), sb.to(dev), sd.field, NEAR, FAR)
    a = ops.field_fwd(*args, ray_offset=offset)
    b = ops.field_fwd(*args, ray_offset=offset, image_width=W)
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y)


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("W,R,offset", [(40, 40 * 17, 0), (37, 37 * 9 + 5, 37 * 3 + 11), (16, 16 * 8, 16 * 8)])
def test_proposal_pixel_patch_schedule_changes_nothing(dev, level, W, R, offset):
    """image_width only changes which (ray, sample) a thread evaluates (8x8 pixel patch x one sample index per
    wave): bit-identical densities for ragged widths, partial bands, mid-row offsets, shared and per-ray bins."""
    from uncertainty_nerf_gs_amd import ops
    t, sc, sd = _scene("active", dev)
    g = torch.Generator().manual_seed(W + R + level)
    o = torch.randn(R, 3, generator=g) * 0.3
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    n = 256 if level == 0 else 96
    sb = O.initial_spacing_bins(n) if level == 0 else torch.sort(torch.rand(R, n + 1, generator=g), dim=-1).values
    args = (o.to(dev), d.to(dev), sb.contiguous().to(dev), sd.props[level], NEAR, FAR, 0.01)
    a = ops.proposal_density(*args)
    b = ops.proposal_density(*args, ray_offset=offset, image_width=W)
    assert torch.equal(a, b)


@pytest.mark.parametrize("n,shared", [(50, True), (7, False), (3, False), (97, False), (130, True), (1, False)])
def test_proposal_patch_kernel_ragged_sample_counts(dev, n, shared):
    """sample counts that are not a multiple of 4 (scalar-store path, clamped edge staging of the LDS-staged patch
    kernel) and an output that is not 16-byte aligned: same bits as the one-thread-per-sample kernel"""
    from uncertainty_nerf_gs_amd import ops
    t, sc, sd = _scene("active", dev)
    W, R, offset = 24, 24 * 11 + 3, 24 * 2 + 5
    g = torch.Generator().manual_seed(n)
    o = torch.randn(R, 3, generator=g) * 0.3
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    sb = O.initial_spacing_bins(n) if shared else torch.sort(torch.rand(R, n + 1, generator=g), dim=-1).values
    args = (o.to(dev), d.to(dev), sb.contiguous().to(dev), sd.props[0], NEAR, FAR, 0.01)
    a = ops.proposal_density(*args)
    b = ops.proposal_density(*args, ray_offset=offset, image_width=W)
    assert a.shape == (R, n) and torch.equal(a, b)
    ref = O.density_field(O.sample_positions(o, d, O.spacing_to_euclidean(sb.expand(R, -1) if shared else sb, NEAR, FAR)),
                          sc.prop_nets[0], 0.01)
    _close(b, ref, 2e-5, 1e-7, "density")


# ---- round 3: proposal_initial_sampler="uniform" (identity spacing) and the RGBRenderer backgrounds ------------------

_BACKGROUNDS = ["last_sample", "random", "white", "black"]


@pytest.mark.parametrize("background", _BACKGROUNDS)
@pytest.mark.parametrize("B,S", [(1, 48), (3, 48), (2, 17)])
def test_composite_backgrounds_match_oracle(dev, background, B, S):
    """NerfactoModelConfig.background_color through every composite entry point: group kernels, fused K-pass moments,
    the sample-major plane kernels (README.md:153 of the reference trains with background-color random)"""
    from uncertainty_nerf_gs_amd import ops
    g = torch.Generator().manual_seed(B * 77 + S)
    R = 97
    dens = torch.exp(torch.randn(B, R, S, generator=g) * 2.0)
    dens[:, 0] = 0.0                      # empty ray: the pixel IS the background
    rgb = torch.rand(B, R, S, 3, generator=g)
    sb = torch.sort(torch.rand(R, S + 1, generator=g), dim=-1).values
    eb = O.spacing_to_euclidean(sb, NEAR, FAR)
    deltas = eb[:, 1:] - eb[:, :-1]
    bg = ops.background_of(background)
    out = ops.composite_var(dens.to(dev), rgb.to(dev), sb.to(dev), NEAR, FAR, background=bg).cpu()
    refs = []
    for b in range(B):
        ref = O.render_rgb(rgb[b], O.get_weights(dens[b], deltas), background)
        refs.append(ref)
        _close(out[b, :, 0:3], ref, 0, 3e-6, f"rgb, background {background}")
    want0 = {"random": torch.zeros(3), "black": torch.zeros(3), "white": torch.ones(3), "last_sample": rgb[0, 0, -1]}[background]
    _close(out[0, 0, 0:3], want0, 0, 1e-6, "empty ray shows the background")
    dp, cp = dens.permute(0, 2, 1).contiguous().to(dev), rgb.permute(0, 2, 3, 1).contiguous().to(dev)
    outp = ops.composite_var_planes(dp, cp, sb.to(dev), NEAR, FAR, background=bg).cpu()
    _close(outp[..., 0:3], torch.stack(refs), 0, 3e-6, "planes rgb")
    if B >= 2:
        mean, _ = ops.composite_moments(dens.to(dev), rgb.to(dev), sb.to(dev), NEAR, FAR, background=bg)
        _close(mean.cpu()[:, 0:3], torch.stack(refs).mean(0), 0, 3e-6, "K-pass mean rgb")
        meanp, _ = ops.composite_moments_planes(dp, cp, sb.to(dev), NEAR, FAR, background=bg)
        _close(meanp.cpu()[:, 0:3], torch.stack(refs).mean(0), 0, 3e-6, "K-pass mean rgb (planes)")


def test_uniform_spacing_proposal_pdf_composite_match_oracle(dev):
    """UNERF_SPACING_UNIFORM (UniformSampler: euclid = b far + (1 - b) near) in the proposal density, PDF / weights and
    composite kernels, with the few-view planes near 1 / far 100"""
    from uncertainty_nerf_gs_amd import lib as L, ops, render
    near, far = 1.0, 100.0
    t, sc, sd = _scene("active", dev)
    o, d = _rays()
    R = o.shape[0]
    g = torch.Generator().manual_seed(11)
    for level, n in ((0, 256), (1, 96)):
        sb = O.initial_spacing_bins(n) if level == 0 else torch.sort(torch.rand(R, n + 1, generator=g), dim=-1).values
        sb_ref = sb[None].expand(R, -1) if level == 0 else sb
        eb = O.spacing_to_euclidean(sb_ref, near, far, uniform=True)
        if level == 0:
            assert abs(float(eb[0, 0]) - near) < 1e-5 and abs(float(eb[0, -1]) - far) < 1e-3
        ref = O.density_field(O.sample_positions(o, d, eb), sc.prop_nets[level], 0.01)
        for width in (0, 32):   # thread-per-sample and 8x8-patch kernels
            got = ops.proposal_density(o.to(dev), d.to(dev), sb.contiguous().to(dev), sd.props[level], near, far, 0.01,
                                       image_width=width, spacing=L.SPACING_UNIFORM)
            _close(got, ref, 3e-5, 1e-9, f"uniform-spacing proposal density level {level} (image_width {width})")
        dens = ref.clone()
        w_ref = O.get_weights(dens, eb[:, 1:] - eb[:, :-1])
        m = 96 if level == 0 else 48
        new_ref = O.pdf_resample(w_ref, sb_ref, m)
        pd_ref = O.render_depth_median(w_ref, (eb[:, :-1] + eb[:, 1:]) / 2)
        new, pd, w = ops.weights_pdf_resample(dens.to(dev), sb.contiguous().to(dev), render._pdf_u(m).to(dev), near, far,
                                              want_weights=True, spacing=L.SPACING_UNIFORM)
        _close(w, w_ref, 2e-5, 1e-7, "weights (uniform spacing)")
        _close(new, new_ref, 0, 3e-6, "resampled bins (uniform spacing)", max_bad_frac=2e-4)
        _close(pd, pd_ref, 1e-5, 0, "prop depth (uniform spacing)", max_bad_frac=0.02)
    S = 48
    dens = torch.exp(torch.randn(1, R, S, generator=g) * 2.0)
    rgb = torch.rand(1, R, S, 3, generator=g)
    sb = torch.sort(torch.rand(R, S + 1, generator=g), dim=-1).values
    eb = O.spacing_to_euclidean(sb, near, far, uniform=True)
    steps = (eb[:, :-1] + eb[:, 1:]) / 2
    w = O.get_weights(dens[0], eb[:, 1:] - eb[:, :-1])
    out = ops.composite_var(dens.to(dev), rgb.to(dev), sb.to(dev), near, far, spacing=L.SPACING_UNIFORM).cpu()
    _close(out[0, :, 0:3], O.render_rgb(rgb[0], w), 0, 3e-6, "rgb (uniform spacing)")
    _close(out[0, :, 3:4], O.render_accumulation(w), 2e-6, 1e-7, "accumulation (uniform spacing)")
    _close(out[0, :, 4:5], O.render_depth_median(w, steps), 1e-6, 0, "median depth (uniform spacing)", max_bad_frac=0.02)
    ed = torch.sum(w * steps, -1, keepdim=True) / (torch.sum(w, -1, keepdim=True) + 1e-10)
    _close(out[0, :, 5:6], ed, 2e-5, 1e-6, "expected depth (uniform spacing)")


def test_uniform_spacing_crop_box_bins(dev):
    """unerf_ray_box_bins / unerf_ray_planes_bins fold per-ray planes into the first-level bins with the identity
    spacing too: the Euclidean edges under the launch-wide planes are b far_r + (1 - b) near_r"""
    from uncertainty_nerf_gs_amd import lib as L, ops
    near, far = 1.0, 100.0
    g = torch.Generator().manual_seed(3)
    R, n = 77, 256
    nears = 1.0 + torch.rand(R, generator=g) * 5
    fars = nears + 1.0 + torch.rand(R, generator=g) * 50
    row = O.initial_spacing_bins(n)
    bins = ops.ray_planes_bins(nears.to(dev), fars.to(dev), near, far, row.to(dev), spacing=L.SPACING_UNIFORM).cpu()
    eu = O.spacing_to_euclidean(bins, near, far, uniform=True)
    want = O.spacing_to_euclidean(row[None].expand(R, -1), nears[:, None], fars[:, None], uniform=True)
    _close(eu, want, 2e-5, 1e-5, "per-ray planes under uniform spacing")


def test_spacing_and_background_arguments_are_validated(dev):
    from uncertainty_nerf_gs_amd import lib as L, ops
    dens, rgb = torch.rand(1, 4, 16, device=dev), torch.rand(1, 4, 16, 3, device=dev)
    sb = torch.sort(torch.rand(4, 17, device=dev), dim=-1).values
    with pytest.raises(L.UnerfError, match="spacing=5"):
        ops.composite_var(dens, rgb, sb, NEAR, FAR, spacing=5)
    with pytest.raises(L.UnerfError, match="background=9"):
        ops.composite_var(dens, rgb, sb, NEAR, FAR, background=(9, None))
    with pytest.raises(L.UnerfError, match="background_color"):
        ops.background_of("purple-ish")


@pytest.mark.parametrize("K", [0, 3, 8])
def test_field_f16_single_product_mode(dev, K):
    """unerf_field_params.f16_single: every pass of the K-pass kernel against the fp32 oracle (f16 operand rounding:
    relative 5e-4 per operand, logits good to ~2e-3) and against the oracle's autocast(float16) emulation"""
    from uncertainty_nerf_gs_amd import ops
    seed, p = 1234, 0.2
    t, sc, sd = _scene("mcdropout", dev, K=K, seed=seed, p_drop=p)
    sd.field.precision = "f16"
    o, d = _rays(16, 24)
    sb = _final_bins(sc, o, d)
    eb = O.spacing_to_euclidean(sb, NEAR, FAR)
    dens, rgb, _, _ = ops.field_fwd(o.to(dev), d.to(dev), sb.to(dev), sd.field, NEAR, FAR, ray_offset=1000)
    R, S = sb.shape[0], sb.shape[1] - 1
    sidx = ((np.arange(R)[:, None] + 1000) * S + np.arange(S)[None]).reshape(-1)
    for k in range(max(K, 1)):
        kt = kh = None
        if K > 0:
            kt = torch.from_numpy(O.mc_keep_mask(seed, k, sidx, 0, 64, p))
            kh = torch.from_numpy(O.mc_keep_mask(seed, k, sidx, 1, 64, p))
        for ac, dtol, ctol in ((None, 1e-2, 2e-4), (torch.float16, 2e-2, 4e-4)):
            dr, cr = O.mcdropout_field(o, d, eb, sc.field, kt, kh, p, autocast=ac)
            _close(dens[k], dr, dtol, 1e-7, f"density pass {k} vs autocast={ac}", max_bad_frac=1e-3)
            _close(rgb[k], cr, 0, ctol, f"rgb pass {k} vs autocast={ac}")
    # f16 needs the f16 operand blobs: a field whose weights leave the f16 range says so
    sd.field.mfma16_blob = None
    with pytest.raises(Exception, match="precision='f16' needs"):
        ops.field_fwd(o.to(dev), d.to(dev), sb.to(dev), sd.field, NEAR, FAR)


def test_field_f16_single_product_mode_active_and_laplace(dev):
    from uncertainty_nerf_gs_amd import ops, synthetic
    o, d = _rays(12, 16)
    t, sc, sd = _scene("active", dev)
    sd.field.precision = "f16"
    sb = _final_bins(sc, o, d)
    eb = O.spacing_to_euclidean(sb, NEAR, FAR)
    dens, rgb, beta, _ = ops.field_fwd(o.to(dev), d.to(dev), sb.to(dev), sd.field, NEAR, FAR)
    dr, cr, br = O.active_field(o, d, eb, sc.field)
    _close(dens[0], dr, 1e-2, 1e-7, "density", max_bad_frac=1e-3)
    _close(rgb[0], cr, 0, 2e-4, "rgb")
    _close(beta, br, 1e-2, 1e-4, "beta", max_bad_frac=1e-3)
    t, sc, _ = _scene("laplace", dev)
    wsd, wsr = synthetic.laplace_weight_samples(t, seed=42, n_samples=100)
    sd = synthetic.scene_to_device(t, dev, ws_density=wsd.to(dev), ws_rgb=wsr.to(dev))
    sd.field.precision = "f16"
    sb = _final_bins(sc, o, d)
    eb = O.spacing_to_euclidean(sb, NEAR, FAR)
    mu_d, var_d, mu_rgb, var_rgb = O.laplace_field(o, d, eb, sc.field, wsd, wsr)
    dens, rgb, dvar, rvar = ops.field_fwd(o.to(dev), d.to(dev), sb.to(dev), sd.field, NEAR, FAR)
    _close(dens[0], mu_d, 1e-2, 1e-7, "mu_d", max_bad_frac=1e-3)
    _close(rgb[0], mu_rgb, 0, 2e-4, "mu_rgb")
    _close(dvar, var_d, 0, 2e-2 * float((mu_d ** 2).max()), "var_d")
    _close(rvar, var_rgb, 0, 2e-5, "var_rgb")
