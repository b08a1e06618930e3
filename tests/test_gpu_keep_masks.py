"""Explicit MC-dropout keep masks on the GPU (unerf_field_fwd_masked / unerf_pack_keep_bits / unerf_mc_keep_bits and the
layers above them): the packers against numpy and the oracle's generator twin, BIT IDENTITY of every kernel selection
with the counter path when it is fed the counter's own masks, torch-Bernoulli masks against the oracle pass by pass,
row offsets, the frame path, the Model's "torch" mode, and the GPU half of the generator-vs-Bernoulli statistics.
Scenes are the sizes of tests/test_gpu_nerf_kernels.py."""

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

NEAR, FAR = 0.05, 1000.0
KERNELS = [(True, "f16"), (True, "f16x2"), (True, "fp32"), (False, "fp32")]
KERNEL_IDS = ["mfma-f16", "mfma-f16x2", "mfma-fp32", "valu"]


def _scene(dev, scene_seed=0, grid=None, **kw):
    from uncertainty_nerf_gs_amd import synthetic
    t = synthetic.make_scene_tensors(seed=scene_seed, kind="mcdropout", log2T=14, prop_log2T=12, **({"grid": grid} if grid else {}))
    if grid:
        t["grid_precision"] = "f16"
    return t, O.scene_from_tensors(t), synthetic.scene_to_device(t, dev, **kw)


def _rays(H=16, W=24, theta=0.3):
    from uncertainty_nerf_gs_amd import synthetic
    o, d, _ = O.generate_rays(synthetic.orbit_c2w(theta), 30.0, 30.0, W / 2, H / 2, H, W)
    return o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()


def _bins(sc, o, d):
    return O.proposal_sample(o, d, NEAR, FAR, sc.prop_nets, sc.num_prop, sc.num_nerf, 0.01)[0].contiguous()


def _unpack(bits: torch.Tensor, n: int) -> np.ndarray:
    """int32 [..., W] -> bool [..., n]"""
    b = np.ascontiguousarray(bits.cpu().numpy()).view(np.uint8)
    return np.unpackbits(b, axis=-1, bitorder="little")[..., :n].astype(bool)


def _close(got, ref, rtol, atol, what, max_bad_frac=0.0):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    bad = ((got - ref).abs() > (atol + rtol * ref.abs())) | (torch.isnan(got) != torch.isnan(ref))      # a NaN on one side only is off (NaN > tol is False)
    frac = bad.double().mean().item()
    assert frac <= max_bad_frac, f"{what}: {frac:.3e} of elements off (worst |diff|={(got - ref).abs().max().item():.3e})"


# ---- 1 / 2: the two helper kernels ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_units,rows", [(64, 77), (63, 130), (16, 33), (128, 1001)])
def test_pack_keep_bits_equals_numpy_packbits(dev, n_units, rows):
    from uncertainty_nerf_gs_amd import ops
    g = torch.Generator().manual_seed(n_units + rows)
    keep = torch.rand(rows, n_units, generator=g) < 0.7
    W = (n_units + 31) // 32
    padded = np.zeros((rows, 32 * W), dtype=bool)
    padded[:, :n_units] = keep.numpy()
    want = np.packbits(padded, axis=-1, bitorder="little").view(np.uint32)
    for src in (keep, keep.to(torch.uint8) * 3):         # a torch bool tensor, and uint8 with "non-zero = kept"
        got = ops.pack_keep_bits(src.to(dev))
        assert got.shape == (rows, W) and got.dtype == torch.int32
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
    lead = ops.pack_keep_bits(keep.to(dev).reshape(1, rows, n_units))       # leading dimensions are kept
    assert lead.shape == (1, rows, W) and torch.equal(lead[0], got)


@pytest.mark.parametrize("n_units", [64, 128])
@pytest.mark.parametrize("stream", [0, 1, 2])
def test_mc_keep_bits_equals_the_oracle_generator(dev, lib, stream, n_units):
    from uncertainty_nerf_gs_amd import ops
    K, seed, p, first, n, stride = 10, 4321, 0.2, 12345, 3000, 3100
    W = n_units // 32
    bits = torch.full((K, stride, W), -1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        lib.check(lib.load().unerf_mc_keep_bits(seed, K, first, n, stream, n_units, p, bits.data_ptr(), stride,
                                                torch.cuda.current_stream().cuda_stream), "mc_keep_bits")
    got = _unpack(bits, n_units)
    sidx = np.arange(first, first + n)
    for k in range(K):
        assert np.array_equal(got[k, :n], O.mc_keep_mask(seed, k, sidx, stream, n_units, p)), (stream, k)
    assert (bits[:, n:] == -1).all(), "rows between n_samples and pass_stride are not written"
    assert 0.78 < got[:, :n].mean() < 0.82


# ---- 3: bit identity with the counter path --------------------------------------------------------------------------------

def _identity_case(dev, use_mfma, precision, sites=5, K=8, grid=None, layout="plain", seed=1234, p=0.2, ray_offset=64):
    from uncertainty_nerf_gs_amd import ops
    t, sc, sd = _scene(dev, grid=grid, K=K, seed=seed, p_drop=p, drop_sites=sites)
    f = sd.field
    f.use_mfma, f.precision = use_mfma, precision
    o, d = _rays()
    if grid:
        sb = O.proposal_sample(o, d, NEAR, FAR, sc.prop_nets, sc.num_prop, sc.num_nerf, 0.01)[0].contiguous()
    else:
        sb = _bins(sc, o, d)
    od, dd, sbd = o.to(dev), d.to(dev), sb.to(dev)
    R, S = sb.shape[0], sb.shape[1] - 1
    kw = dict(ray_offset=ray_offset)
    if layout == "packed":
        kw.update(packed=True, image_width=24)
    elif layout == "sample_major":
        kw.update(sample_major=True)
    elif layout == "features":
        kw.update(features=ops.field_gather(od, dd, sbd, f, NEAR, FAR))
    masks = ops.mc_keep_bits(f, ray_offset * S, R * S)
    assert [m is not None for m in masks.sites()] == [bool(sites & 1), bool(sites & 2), bool(sites & 4), False]
    a = ops.field_fwd(od, dd, sbd, f, NEAR, FAR, **kw)
    a = [None if x is None else x.clone() for x in a]
    b = ops.field_fwd(od, dd, sbd, f, NEAR, FAR, keep_masks=masks, **kw)
    for name, x, y in zip(("density", "rgb", "aux", "aux2"), a, b):
        assert (x is None) == (y is None), name
        if x is not None:
            assert torch.isfinite(x).all()
            assert torch.equal(x, y), f"{name}: {(x != y).sum().item()} of {x.numel()} values differ from the counter path"
    if K > 1 and sites & 4:
        rgb = a[1]
        assert not torch.equal(rgb[0], rgb[1])
    # the masks matter: all-kept masks give another result
    ones = ops.KeepMasks(*[None if m is None else torch.full_like(m, -1) for m in masks.sites()[:3]], None, masks.pass_stride, 0)
    c = ops.field_fwd(od, dd, sbd, f, NEAR, FAR, keep_masks=ones, **kw)
    assert not torch.equal(c[1], a[1])


@pytest.mark.parametrize("use_mfma,precision", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("sites", [5, 1, 4, 2, 6, 7])
def test_explicit_counter_masks_are_bit_identical_sites(dev, sites, use_mfma, precision):
    _identity_case(dev, use_mfma, precision, sites=sites, K=8)


@pytest.mark.parametrize("use_mfma,precision", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("K", [1, 10])
def test_explicit_counter_masks_are_bit_identical_passes(dev, K, use_mfma, precision):
    _identity_case(dev, use_mfma, precision, K=K)


@pytest.mark.parametrize("use_mfma,precision,layout",
                         [(um, pr, lay) for um, pr in KERNELS for lay in ("packed", "sample_major") if um or lay == "packed"]
                         + [(True, "fp32", "features")])
def test_explicit_counter_masks_are_bit_identical_layouts(dev, use_mfma, precision, layout):
    """packed rows (with the image_width tile hint) in every kernel; sample-major planes in the matrix kernels, the ones
    that write them; pre-gathered feature planes in the exact-fp32 matrix kernel, the one that accepts them"""
    _identity_case(dev, use_mfma, precision, layout=layout)


@pytest.mark.parametrize("use_mfma,precision", KERNELS, ids=KERNEL_IDS)
def test_explicit_counter_masks_are_bit_identical_on_the_tcnn_half_grid(dev, use_mfma, precision):
    _identity_case(dev, use_mfma, precision, grid="tcnn", K=3)


# ---- 4: torch Bernoulli masks against the oracle, pass by pass ------------------------------------------------------------

@pytest.mark.parametrize("use_mfma,precision", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("sites", [5, 7])
def test_torch_masks_match_the_oracle_under_the_same_masks(dev, sites, use_mfma, precision):
    """tolerances: test_field_mcdropout_matches_oracle (fp32-equivalent kernels) and test_field_f16_single_product_mode
    ("f16", both oracle arithmetics), unchanged"""
    from uncertainty_nerf_gs_amd import ops
    K, p = 3, 0.2
    t, sc, sd = _scene(dev, K=K, seed=1, p_drop=p, drop_sites=sites)
    sd.field.use_mfma, sd.field.precision = use_mfma, precision
    o, d = _rays()
    sb = _bins(sc, o, d)
    eb = O.spacing_to_euclidean(sb, NEAR, FAR)
    R, S = sb.shape[0], sb.shape[1] - 1
    g = torch.Generator().manual_seed(99 + sites)
    keep = [torch.bernoulli(torch.full((K, R * S, 64), 1 - p), generator=g).bool() if (sites >> i) & 1 else None for i in range(3)]
    masks = ops.KeepMasks(*[None if m is None else ops.pack_keep_bits(m.to(dev)) for m in keep], None, R * S, 0)
    dens, rgb, _, _ = ops.field_fwd(o.to(dev), d.to(dev), sb.to(dev), sd.field, NEAR, FAR, ray_offset=7, keep_masks=masks)
    assert dens.shape == (K, R, S)
    for k in range(K):
        m = lambda i: None if keep[i] is None else keep[i][k]
        if precision == "f16":
            for ac, dtol, ctol in ((None, 1e-2, 2e-4), (torch.float16, 2e-2, 4e-4)):
                dr, cr = O.mcdropout_field(o, d, eb, sc.field, m(0), m(2), p, keep_head0=m(1), autocast=ac)
                _close(dens[k], dr, dtol, 1e-7, f"density pass {k} vs autocast={ac}", max_bad_frac=1e-3)
                _close(rgb[k], cr, 0, ctol, f"rgb pass {k} vs autocast={ac}")
        else:
            dr, cr = O.mcdropout_field(o, d, eb, sc.field, m(0), m(2), p, keep_head0=m(1))
            _close(dens[k], dr, 2e-4, 1e-7, f"density pass {k}")
            _close(rgb[k], cr, 0, 2e-5, f"rgb pass {k}")


# ---- 5: row offsets -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("use_mfma,precision", [(True, "f16"), (False, "fp32")], ids=["mfma-f16", "valu"])
@pytest.mark.parametrize("extra_stride", [0, 333])
def test_two_calls_into_one_frame_wide_mask_array_equal_one_call(dev, extra_stride, use_mfma, precision):
    from uncertainty_nerf_gs_amd import ops
    K = 4
    t, sc, sd = _scene(dev, K=K, seed=11, p_drop=0.2)
    sd.field.use_mfma, sd.field.precision = use_mfma, precision
    o, d = _rays()
    sb = _bins(sc, o, d)
    od, dd, sbd = o.to(dev), d.to(dev), sb.to(dev)
    R, S = sb.shape[0], sb.shape[1] - 1
    masks = ops.mc_keep_bits(sd.field, 0, R * S, pass_stride=R * S + extra_stride)
    assert masks.pass_stride == R * S + extra_stride and masks.trunk.shape == (K, R * S + extra_stride, 2)
    whole = [x.clone() for x in ops.field_fwd(od, dd, sbd, sd.field, NEAR, FAR, keep_masks=masks)[:2]]
    counter = ops.field_fwd(od, dd, sbd, sd.field, NEAR, FAR)
    assert torch.equal(whole[0], counter[0]) and torch.equal(whole[1], counter[1])
    R1 = 160
    first = [x.clone() for x in ops.field_fwd(od[:R1], dd[:R1], sbd[:R1], sd.field, NEAR, FAR, keep_masks=masks.at(0))[:2]]
    second = ops.field_fwd(od[R1:], dd[R1:], sbd[R1:], sd.field, NEAR, FAR, keep_masks=masks.at(R1 * S))[:2]
    for x, y, z in zip(whole, first, second):
        assert torch.equal(x[:, :R1], y) and torch.equal(x[:, R1:], z)
    # a call that would read past the rows of a pass is refused, not clamped
    with pytest.raises(Exception, match="pass_stride"):
        ops.field_fwd(od, dd, sbd, sd.field, NEAR, FAR, keep_masks=masks.at(extra_stride + 1))


# ---- 6: frame level ------------------------------------------------------------------------------------------------------

FRAME_H, FRAME_W = 32, 40


def _frame_cam():
    return dict(fx=0.9 * FRAME_W, fy=0.9 * FRAME_W, cx=FRAME_W / 2, cy=FRAME_H / 2, H=FRAME_H, W=FRAME_W)


@pytest.mark.parametrize("overlap", [False, True])
def test_render_camera_with_exported_counter_masks_equals_the_counter_frame(dev, overlap):
    from uncertainty_nerf_gs_amd import ops, render, synthetic
    t, sc, sd = _scene(dev, scene_seed=1, K=4, seed=1234, p_drop=0.2)
    sd.chunk_rays = 512
    c2w = synthetic.orbit_c2w(2.1)
    a = render.render_camera(sd, c2w, rays_per_launch=1024, overlap=overlap, **_frame_cam())
    masks = ops.mc_keep_bits(sd.field, 0, FRAME_H * FRAME_W * sd.num_nerf)
    b = render.render_camera(sd, c2w, rays_per_launch=1024, overlap=overlap, keep_masks=masks, **_frame_cam())
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert float(a["rgb_std"].max()) > 0


def _torch_model(dev, t, K, chunk=512):
    from test_gpu_models import _small_cfg, _state_dict_from_tensors
    from uncertainty_nerf_gs_amd import plugin
    cfg = _small_cfg(plugin.MODEL_CONFIGS["nerfacto-mcdropout"]())
    cfg.mc_samples, cfg.eval_num_rays_per_chunk = K, chunk
    model = cfg._target(cfg, num_train_data=4)
    model.load_state_dict(_state_dict_from_tensors(t, "mcdropout"))
    model.rays_per_launch = 2 * chunk
    model.precision = "f16x2"            # fp32-equivalent arithmetic: the tolerances below are those of the fp32 parity test
    model.dropout_masks = "torch"
    return model, cfg


def _frame_camera(theta=2.1):
    from uncertainty_nerf_gs_amd import models, synthetic
    return models.Camera(camera_to_worlds=synthetic.orbit_c2w(theta)[None], fx=torch.tensor([0.9 * FRAME_W]),
                         fy=torch.tensor([0.9 * FRAME_W]), cx=FRAME_W / 2, cy=FRAME_H / 2, height=FRAME_H, width=FRAME_W)


def test_model_in_torch_mask_mode_matches_the_oracle_under_the_same_draws(dev):
    """NerfactoMCDropoutModel(dropout_masks="torch") against the oracle composed of _sample, mcdropout_field,
    nerfacto_pass_outputs and mean / unbiased std, under the masks a CPU generator of the same seed draws in the
    reference's order; tolerances of test_mcdropout_camera_parity"""
    import keep_mask_stats as KS
    from uncertainty_nerf_gs_amd import synthetic
    K, chunk, seed = 4, 512, 2024
    t = synthetic.make_scene_tensors(seed=1, kind="mcdropout", log2T=14, prop_log2T=12)
    sc = O.scene_from_tensors(t)
    model, cfg = _torch_model(dev, t, K, chunk)
    p = cfg.dropout_rate
    model.mask_generator = torch.Generator().manual_seed(seed)
    with torch.cuda.device(dev):
        out = model.get_outputs_for_camera(_frame_camera())
    cam = _frame_cam()
    o, d, _ = O.generate_rays(synthetic.orbit_c2w(2.1), cam["fx"], cam["fy"], cam["cx"], cam["cy"], FRAME_H, FRAME_W)
    S = sc.num_nerf
    keep = KS.torch_keep_masks(seed, K, FRAME_H * FRAME_W, S, chunk, 5, p)

    def chunk_fn(oo, dd, off):
        eb, wl, bl = O._sample(sc, oo, dd)
        rows = slice(off * S, (off + oo.shape[0]) * S)
        outs = []
        for k in range(K):
            density, rgb = O.mcdropout_field(oo, dd, eb, sc.field, keep[0][k][rows], keep[2][k][rows], p)
            outs.append(O.nerfacto_pass_outputs(sc, oo, dd, eb, wl, bl, density, rgb))
        res = {}
        for key in outs[0]:
            el = torch.stack([x[key] for x in outs])
            res[key] = el.mean(dim=0)
            if key in ("rgb", "depth", "expected_depth"):
                res[key + "_std"] = el.std(dim=0).mean(dim=-1)[..., None]
        return res

    ref = O.render_camera(chunk_fn, o, d, chunk=chunk)
    assert set(ref) == set(out), set(ref) ^ set(out)

    def img_close(key, atol, rtol, max_bad_frac=0.0):
        got, want = out[key].cpu().double(), ref[key].double()
        frac = (((got - want).abs() > atol + rtol * want.abs()) | (torch.isnan(got) != torch.isnan(want))).double().mean().item()
        assert frac <= max_bad_frac, f"{key}: {frac:.3e} of pixels off, worst {(got - want).abs().max().item():.3e}"

    img_close("rgb", 5e-5, 0)
    img_close("rgb_std", 1e-5, 5e-3)
    img_close("accumulation", 2e-4, 0)
    img_close("expected_depth", 0, 1e-3, max_bad_frac=2e-3)
    img_close("expected_depth_std", 1e-3, 2e-2, max_bad_frac=1e-2)
    img_close("depth", 0, 1e-3, max_bad_frac=2e-2)


def test_torch_mask_mode_is_reproducible_per_generator_seed_and_bounded_by_its_budget(dev):
    from types import SimpleNamespace
    from uncertainty_nerf_gs_amd import lib as L, ops, synthetic
    t = synthetic.make_scene_tensors(seed=1, kind="mcdropout", log2T=14, prop_log2T=12)
    model, cfg = _torch_model(dev, t, 4)
    cam = _frame_camera()
    frames = []
    with torch.cuda.device(dev):
        for seed in (7, 7, 8):
            model.mask_generator = torch.Generator().manual_seed(seed)
            frames.append(model.get_outputs_for_camera(cam))
        for k in frames[0]:
            assert torch.equal(frames[0][k], frames[1][k]), k           # same generator seed: the same frame
        assert not torch.equal(frames[0]["rgb_std"], frames[2]["rgb_std"])
        # the other two entry points draw for their own ray counts (get_outputs: one chunk = the bundle)
        o, d, _ = ops.generate_rays(cam.camera_to_worlds[0], 0.9 * FRAME_W, 0.9 * FRAME_W, FRAME_W / 2, FRAME_H / 2, FRAME_H, FRAME_W, dev)
        model.mask_generator = torch.Generator().manual_seed(7)
        bundle = model.get_outputs_for_camera_ray_bundle(SimpleNamespace(origins=o.view(FRAME_H, FRAME_W, 3), directions=d.view(FRAME_H, FRAME_W, 3)))
        for k in bundle:
            assert torch.equal(bundle[k], frames[0][k]), k
        flat = model.get_outputs((o[:300], d[:300]))
        assert flat["rgb_std"].shape == (300, 1) and float(flat["rgb_std"].max()) > 0
        # a frame whose packed masks exceed the budget raises before anything is drawn or launched
        need = 4 * FRAME_H * FRAME_W * 48 * 8 * 2
        model.mask_budget_bytes = need - 1
        state = torch.get_rng_state()
        model.mask_generator = g = torch.Generator().manual_seed(7)
        g_state = g.get_state()
        ops.TIMER = ops.KernelTimer()
        try:
            with pytest.raises(L.UnerfError, match=f"need {need} bytes"):
                model.get_outputs_for_camera(cam)
            assert ops.TIMER.events == {}, "nothing may be launched"
        finally:
            ops.TIMER = None
        assert torch.equal(g.get_state(), g_state) and torch.equal(torch.get_rng_state(), state), "nothing may be drawn"
        model.mask_budget_bytes = need
        again = model.get_outputs_for_camera(cam)
        assert torch.equal(again["rgb"], frames[0]["rgb"])
    # the default is the counter generator, and an unknown value is refused
    assert type(model).dropout_masks == "counter"
    model.dropout_masks = "numpy"
    with pytest.raises(ValueError, match="dropout_masks"):
        with torch.cuda.device(dev):
            model.get_outputs_for_camera(cam)


# ---- 7: GPU half of the generator-vs-Bernoulli statistics -------------------------------------------------------------------

def test_rgb_std_of_the_kernels_under_counter_masks_and_torch_bernoulli_have_the_same_distribution(dev):
    """GPU twin of tests/test_keep_masks_cpu.py's oracle test: group A = the "f16x2" kernels with the counter generator
    (seeds 1000 + i), group B = the same kernels fed torch-Bernoulli masks (CPU generators seeded 5000 + i) through the
    explicit path; same frame, same three gates (keep_mask_stats)."""
    import keep_mask_stats as KS
    from uncertainty_nerf_gs_amd import models, render, synthetic
    sd = synthetic.scene_to_device(KS.scene_tensors(), dev, K=KS.K, seed=0, p_drop=KS.P_DROP, drop_sites=KS.SITES)
    sd.field.precision = "f16x2"
    c2w, cam = KS.camera()
    R, S = KS.H * KS.W, sd.num_nerf
    a, b = [], []
    for i in range(KS.N_SEEDS):
        sd.field.seed = 1000 + i
        a.append(render.render_camera(sd, c2w, **cam)["rgb_std"].reshape(-1).cpu().numpy())
        masks = models.draw_torch_keep_masks(dev, KS.K, R, S, sd.chunk_rays, KS.SITES, KS.P_DROP,
                                             torch.Generator().manual_seed(5000 + i))
        b.append(render.render_camera(sd, c2w, keep_masks=masks, **cam)["rgb_std"].reshape(-1).cpu().numpy())
    KS.report_and_gate("kernels f16x2: counter vs torch Bernoulli", np.stack(a), np.stack(b))
