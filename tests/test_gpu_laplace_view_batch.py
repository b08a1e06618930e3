"""Several camera views per Laplace render call (unerf_field_fwd_laplace_views, unerf_laplace_depth_weights_views,
render.render_cameras, NerfactoLaplaceModel.get_outputs_for_cameras_unc, run_eval(view_batch=...) for LaplaceConfig and
EnsembleConfig): every view of a shared launch is BIT-identical to the single-view path with that view's camera, last-layer
sample sets and depth seed -- torch.equal, no tolerance.  The single-view path is what the oracle gates.

Shapes (tests/test_gpu_nerf_view_batch.py: H, W, CHUNK, RPL): 29 x 37 = 1,073 rays per view is no multiple of 16, 32 or 64 --
the last ray block of every view has 17 valid columns and a depth block straddles two views; chunks of 512 rays give three
sample sets per view, the last covering 49 rays; 3 views at rays_per_launch = 2,560 make two launch groups (2 + 1 views)."""
import pytest
import torch

import test_gpu_nerf_view_batch as VB
from test_gpu_nerf_view_batch import CHUNK, H, HW, RPL, W

pytestmark = pytest.mark.gpu

SET_BASE = (3, 0, 6)            # into a stack of 9 sets: three per view at 512 rays per set, views not in stack order
DEPTH_SEEDS = (3, 3, 900001)
D = 20                          # depth draws per ray (an odd / even pair loop either way; 100 is the models' default)


def _lap_scene(dev, n_sets=9, chunk=CHUNK, precision="f16x2", per_chunk=True, n=30, tensors=None, **field_kw):
    """a Laplace scene with a stack of n_sets independent last-layer sample sets of n rows; per_chunk=False: one set per view"""
    from uncertainty_nerf_gs_amd import synthetic
    t = VB._tensors("laplace") if tensors is None else tensors
    ws = [synthetic.laplace_weight_samples(t, seed=40 + i, n_samples=n) for i in range(n_sets)]
    wsd, wsr = torch.stack([w[0] for w in ws]), torch.stack([w[1] for w in ws])
    scene = synthetic.scene_to_device(t, dev, ws_density=wsd.to(dev), ws_rgb=wsr.to(dev), lap_chunk_rays=chunk, **field_kw)
    scene.chunk_rays, scene.field.precision = chunk, precision
    if not per_chunk:
        scene.field.lap_chunk_rays = 0
    return scene


@pytest.mark.parametrize("precision", ["f16x2", "f16"])
@pytest.mark.parametrize("lap_chunk_rays", [CHUNK, 0])
def test_field_views_read_each_views_own_sample_sets(dev, precision, lap_chunk_rays):
    from uncertainty_nerf_gs_amd import ops, render
    scene = _lap_scene(dev, precision=precision, per_chunk=lap_chunk_rays != 0)
    scene.workspace = None
    f, near, far = scene.field, scene.near, scene.far
    spv = ops.laplace_sets_per_view(f, HW)
    assert spv == (3 if lap_chunk_rays else 1)
    singles, o, d = VB._rays(dev, VB._poses(3), VB._intr(3))
    sb, _ = render.sample_rays(scene, o, d, None, 0, want_prop_depth=False)
    views = ops.RayViews(3, HW)
    ws = ops.Workspace()                                  # the outputs live here: pre-filled with NaN
    for tag, shape in (("density", (1, 3 * HW, 48)), ("rgb", (1, 3 * HW, 48, 3)), ("aux", (3 * HW, 48)), ("aux2", (3 * HW, 48))):
        ws.get("field_" + tag, shape, dev).fill_(float("nan"))
    got = ops.field_fwd(o, d, sb, f, near, far, views=views, lap_views=ops.LaplaceViews(SET_BASE), workspace=ws)
    assert got[0].shape == (1, 3 * HW, 48) and got[1].shape == (1, 3 * HW, 48, 3) and got[2].shape == got[3].shape == (3 * HW, 48)
    assert all(torch.isfinite(g).all() for g in got)      # every row of every view was written

    def single(v, base, **kw):
        ov, dv = singles[v]
        sl = slice(v * HW, (v + 1) * HW)
        fv = f if base is None else ops.laplace_sets_view(f, base, spv)
        return ops.field_fwd(ov, dv, sb[sl].contiguous(), fv, near, far, ray_offset=0, image_width=W, **kw)

    for v in range(3):
        want = single(v, SET_BASE[v])
        sl = slice(v * HW, (v + 1) * HW)
        for name, g, w_ in zip(("density", "rgb", "aux", "aux2"), got, want):
            gv = g[:, sl] if name in ("density", "rgb") else g[sl]
            assert torch.equal(gv, w_), (v, name)
    assert float(got[2].max()) > 0 and float(got[3].max()) > 0       # the sampled heads do spread
    # the sets matter: view 0's rays under view 1's sets are another result
    other, mine = single(0, SET_BASE[1]), single(0, SET_BASE[0])
    assert not torch.equal(other[0], mine[0]) and not torch.equal(other[3], mine[3])
    # no per-view table = every view on the field's own sets (set_base = 0), what a loop over the same field computes
    zero = ops.field_fwd(o, d, sb, f, near, far, views=views)
    for v in range(3):
        want = single(v, None)
        sl = slice(v * HW, (v + 1) * HW)
        assert torch.equal(zero[0][:, sl], want[0]) and torch.equal(zero[1][:, sl], want[1])
        assert torch.equal(zero[2][sl], want[2]) and torch.equal(zero[3][sl], want[3])
    # one view = the plain call
    a = single(2, None)
    b = ops.field_fwd(singles[2][0], singles[2][1], sb[2 * HW:].contiguous(), f, near, far, views=ops.RayViews(1, HW))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("S", [48, 20])
def test_depth_weights_views_draw_each_views_own_stream(dev, S):
    """three views with the SAME densities and bins: views 0 and 1 share a seed and come out equal (the stream counter runs
    inside each view's frame), view 2 has another seed and differs; every view equals the single call with its seed"""
    from uncertainty_nerf_gs_amd import ops
    g = torch.Generator().manual_seed(12 + S)
    mu1 = torch.rand(HW, S, generator=g) * 4
    var1 = torch.rand(HW, S, generator=g) * 2
    sb1 = torch.cumsum(torch.rand(HW, S + 1, generator=g) + 0.01, dim=1)
    sb1 = sb1 / sb1[:, -1:] * 0.9
    mu, var, sb = (x.repeat(3, 1).contiguous().to(dev) for x in (mu1, var1, sb1))
    near, far = 0.05, 1000.0
    views = ops.RayViews(3, HW)
    got = ops.laplace_depth_weights(mu, var, sb, near, far, None, D, views=views, lap_views=ops.LaplaceViews(None, DEPTH_SEEDS))
    assert got.shape == (3 * HW, S) and torch.isfinite(got).all() and float(got.max()) > 0
    for v in range(3):
        sl = slice(v * HW, (v + 1) * HW)
        want = ops.laplace_depth_weights(mu[sl].contiguous(), var[sl].contiguous(), sb[sl].contiguous(), near, far, None, D,
                                         seed=DEPTH_SEEDS[v], ray_offset=0)
        assert torch.equal(got[sl], want), v
    assert torch.equal(got[:HW], got[HW:2 * HW]) and not torch.equal(got[:HW], got[2 * HW:])
    # the counter of the single call runs through the tall list instead
    tall = ops.laplace_depth_weights(mu, var, sb, near, far, None, D, seed=3)
    assert torch.equal(tall[:HW], got[:HW]) and not torch.equal(tall[HW:2 * HW], got[HW:2 * HW])
    # no table: `seed` for every view
    same = ops.laplace_depth_weights(mu, var, sb, near, far, None, D, seed=3, views=views)
    assert torch.equal(same[:2 * HW], got[:2 * HW]) and torch.equal(same[2 * HW:], got[:HW])
    # explicit noise has no per-view value: the single call on the whole ray list
    noise = torch.randn(D, 3 * HW, S, generator=g).to(dev)
    assert torch.equal(ops.laplace_depth_weights(mu, var, sb, near, far, noise, D, views=views, lap_views=ops.LaplaceViews(None, DEPTH_SEEDS)),
                       ops.laplace_depth_weights(mu, var, sb, near, far, noise, D))


def _lap_loop(scene, poses, intr, h, w, sets=None, depth_seeds=None, **kw):
    """the single-view path: render_camera per view on the field narrowed to that view's sets, with its depth seed"""
    from uncertainty_nerf_gs_amd import ops, render
    fx, fy, cx, cy = intr
    f, outs = scene.field, []
    spv = ops.laplace_sets_per_view(f, h * w)
    try:
        for v in range(len(poses)):
            if sets is not None:
                scene.field = ops.laplace_sets_view(f, sets[v], spv)
            kv = dict(kw) if depth_seeds is None else dict(kw, depth_seed=depth_seeds[v])
            outs.append(render.render_camera(scene, poses[v], fx[v], fy[v], cx[v], cy[v], h, w, **kv))
    finally:
        scene.field = f
    return outs


def _lap_batch(scene, poses, intr, h, w, groups, depth=True, **kw):
    """render_cameras with the launches it made: `groups` shared ray-generator, field and depth-draw launches"""
    from uncertainty_nerf_gs_amd import ops, render
    ops.TIMER = ops.KernelTimer()
    try:
        outs = render.render_cameras(scene, poses, *intr, h, w, **kw)
        launches = {k: len(v) for k, v in ops.TIMER.events.items()}
    finally:
        ops.TIMER = None
    assert launches.get("generate_rays_views", 0) == groups and "generate_rays" not in launches, launches
    assert launches.get("field_fwd", 0) == groups and launches.get("composite_var", 0) == groups, launches
    assert launches.get("laplace_depth_weights", 0) == (groups if depth else 0), launches
    return outs


@pytest.mark.parametrize("precision", ["f16x2", "f16"])
@pytest.mark.parametrize("per_chunk", [True, False])
def test_render_cameras_equals_the_loop(dev, precision, per_chunk):
    """three views in two launch groups (2 + 1) -- on the parent commit a Laplace scene took the per-camera loop, which
    the launch counts of _lap_batch tell apart; the batch twice on the same scene object (dirty scratch arena) and once on a
    side stream; per-view sets and depth seeds, and the defaults (the field's own sets, one depth seed)"""
    from uncertainty_nerf_gs_amd import render
    scene = _lap_scene(dev, precision=precision, per_chunk=per_chunk)
    assert render.view_batch_loop_reason(scene) is None
    poses, intr = VB._poses(3), VB._intr(3)
    kw = dict(rays_per_launch=RPL, depth_draws=D)
    with torch.cuda.device(dev):
        first = _lap_batch(scene, poses, intr, H, W, 2, lap_view_sets=SET_BASE, depth_seeds=DEPTH_SEEDS, **kw)
        want = _lap_loop(scene, poses, intr, H, W, SET_BASE, DEPTH_SEEDS, **kw)
        again = _lap_batch(scene, poses.to(dev), intr, H, W, 2, lap_view_sets=SET_BASE, depth_seeds=DEPTH_SEEDS, **kw)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            on_side = _lap_batch(scene, poses, intr, H, W, 2, lap_view_sets=SET_BASE, depth_seeds=DEPTH_SEEDS, **kw)
        side.synchronize()
        # defaults: what a loop of render_camera over the same scene renders
        plain = _lap_batch(scene, poses, intr, H, W, 2, depth_seed=11, **kw)
        plain_want = VB._loop(scene, poses, intr, H, W, None, depth_seed=11, **kw)
        torch.cuda.synchronize()
    for got in (first, again, on_side):
        VB._assert_views_equal(got, want)
    VB._assert_views_equal(plain, plain_want)
    assert set(first[0]) >= {"rgb", "rgb_std", "accumulation", "depth", "depth_std", "expected_depth"}
    assert first[0]["rgb"].shape == (H, W, 3) and float(first[1]["rgb_std"].max()) > 0 and float(first[1]["depth_std"].max()) > 0
    assert not torch.equal(first[0]["rgb_std"], plain[0]["rgb_std"])           # view 0 under sets 3.. is not view 0 under sets 0..
    assert scene.field is not None and scene.overflow_rerenders == 0


def test_render_cameras_with_the_deterministic_density(dev):
    """lap_mask_density (use_deterministic_density): selector-masked mean density, no depth kernel; keep_density is not a
    Laplace output"""
    scene = _lap_scene(dev, lap_mask_density=1)
    poses, intr = VB._poses(3), VB._intr(3)
    kw = dict(rays_per_launch=RPL, depth_draws=D)
    with torch.cuda.device(dev):
        got = _lap_batch(scene, poses, intr, H, W, 2, depth=False, lap_view_sets=SET_BASE, depth_seeds=DEPTH_SEEDS, **kw)
        want = _lap_loop(scene, poses, intr, H, W, SET_BASE, DEPTH_SEEDS, **kw)
        torch.cuda.synchronize()
    VB._assert_views_equal(got, want)
    with pytest.raises(ValueError, match="lap_view_sets"):
        from uncertainty_nerf_gs_amd import render
        render.render_cameras(scene, poses, *intr, H, W, lap_view_sets=(0, 1))


def test_sixteen_views_share_one_default_launch_group(dev):
    """16 views of 48 x 64 with default chunking (32,768 rays: one set and one clip row per view) and the default launch group"""
    h, w = 48, 64
    scene = _lap_scene(dev, n_sets=16, chunk=1 << 15)
    poses, intr = VB._poses(16, step=0.37), VB._intr(16, h, w)
    sets, seeds = tuple(range(15, -1, -1)), tuple(range(100, 116))
    with torch.cuda.device(dev):
        got = _lap_batch(scene, poses, intr, h, w, 1, lap_view_sets=sets, depth_seeds=seeds, depth_draws=D)
        want = _lap_loop(scene, poses, intr, h, w, sets, seeds, depth_draws=D)
        torch.cuda.synchronize()
    VB._assert_views_equal(got, want)


def test_views_of_a_flagged_launch_group_are_rerendered_with_their_own_sets(dev):
    """the stress scene of tests/test_gpu_trained_like.py (hidden units past the f16 operand range): the guard flags the launch
    groups, their views are rendered again one by one -- each with its own sets and depth seed -- and equal the loop"""
    import test_gpu_trained_like as TL
    from uncertainty_nerf_gs_amd import ops, render
    t, _, _ = TL._scene("laplace", dev, overflow_units=(5, 41))
    scene = _lap_scene(dev, precision="f16x2", tensors=t)
    assert scene.field.mfma16_blob is not None and scene.overflow_guard
    poses, intr = VB._poses(3), VB._intr(3)
    kw = dict(rays_per_launch=RPL, depth_draws=D)
    with torch.cuda.device(dev):
        ops.TIMER = ops.KernelTimer()
        try:
            got = render.render_cameras(scene, poses, *intr, H, W, lap_view_sets=SET_BASE, depth_seeds=DEPTH_SEEDS, **kw)
            launches = {k: len(v) for k, v in ops.TIMER.events.items()}
        finally:
            ops.TIMER = None
        n_batch = scene.overflow_rerenders
        want = _lap_loop(scene, poses, intr, H, W, SET_BASE, DEPTH_SEEDS, **kw)
        torch.cuda.synchronize()
    assert launches.get("generate_rays_views", 0) == 2 and n_batch >= 1, (launches, n_batch)
    VB._assert_views_equal(got, want)
    assert all(torch.isfinite(v).all() for out in got for v in out.values())
    assert scene.field.precision == "f16x2"


def _ggn(model, seed=3):
    g = torch.Generator().manual_seed(seed)
    model.field.mlp_density_ggn = torch.rand(model.field.mlp_density_ggn.shape, generator=g) * 1e3
    model.field.mlp_rgb_ggn = torch.rand(model.field.mlp_rgb_ggn.shape, generator=g) * 1e3
    return model


def _launch_names(fn):
    from uncertainty_nerf_gs_amd import ops
    ops.TIMER = ops.KernelTimer()
    try:
        out = fn()
        return out, {k: len(v) for k, v in ops.TIMER.events.items()}
    finally:
        ops.TIMER = None


@pytest.mark.parametrize("variant", ["chunk", "deterministic_density", "camera", "n_samples_30"])
def test_model_batch_equals_successive_single_camera_calls(dev, variant):
    """two nerfacto-laplace models, generators seeded alike, chunks of 512 rays: get_outputs_for_cameras_unc against successive
    get_outputs_for_camera_unc calls; the generators end in the same state; the deterministic render afterwards"""
    n_cam = 5 if variant == "chunk" else 3
    a, b = (_ggn(VB._model(dev, "laplace", "nerfacto-laplace", chunk=CHUNK)) for _ in range(2))
    kw = {}
    if variant == "deterministic_density":
        kw = dict(use_deterministic_density=True)
    if variant == "camera":
        a.resample = b.resample = "camera"
    if variant == "n_samples_30":
        kw = dict(n_samples=30)                                 # (the colour head still draws 100 rows)
    ga, gb = (torch.Generator(device=dev).manual_seed(9) for _ in range(2))
    batch, singles = VB._cameras(n_cam)
    with torch.cuda.device(dev):
        got, launches = _launch_names(lambda: a.get_outputs_for_cameras_unc(batch, max_views=2, generator=ga, **kw))
        want = [b.get_outputs_for_camera_unc(cam, generator=gb, **kw) for cam in singles]
        torch.cuda.synchronize()
    assert launches.get("generate_rays_views", 0) == n_cam // 2 + 1 and "generate_rays" not in launches, launches
    VB._assert_views_equal(got, want)
    assert torch.equal(ga.get_state(), gb.get_state())
    assert float(got[1]["rgb_std"].max()) > 0 and not torch.equal(got[0]["rgb_std"], got[1]["rgb_std"])
    assert a._ws is None and a._view_sets is None
    # afterwards both models are the deterministic mean-head field again, one camera or several
    c = VB._model(dev, "laplace", "nerfacto-laplace", chunk=CHUNK)
    with torch.cuda.device(dev):
        det = c.get_outputs_for_camera(singles[0])
        VB._assert_views_equal([a.get_outputs_for_camera(singles[0]), b.get_outputs_for_camera(singles[0])], [det, det])
        many, launches = _launch_names(lambda: a.get_outputs_for_cameras(batch, max_views=2))
        VB._assert_views_equal(many[:1], [det])
        torch.cuda.synchronize()
    assert launches.get("generate_rays_views", 0) == n_cam // 2 + 1 and "laplace_depth_weights" not in launches, launches
    if variant == "chunk":
        with pytest.raises(ValueError, match="max_views"):
            a.get_outputs_for_cameras_unc(batch, max_views=17)


def _same_metrics(res):
    assert set(res[1]) == set(res[4]) and set(VB.TIMING_KEYS) <= set(res[4])
    for k in res[1]:
        if k not in VB.TIMING_KEYS:
            assert res[4][k] == res[1][k], k
        else:
            assert res[4][k] > 0


def test_run_eval_view_batch_laplace(dev, tmp_path):
    from uncertainty_nerf_gs_amd import eval as E
    _, singles = VB._cameras(6)
    eval_set = [(cam, VB._gt(H, W, 50 + i)) for i, cam in enumerate(singles)]
    (tmp_path / "cfg").mkdir()
    g = torch.Generator().manual_seed(1)
    torch.save({"mlp_density_ggn": torch.rand(65, generator=g) * 1e3, "mlp_rgb_ggn": torch.rand(195, generator=g) * 1e3},
               tmp_path / "cfg" / "ggn_7.pt")
    res = {}
    for vb in (1, 4):
        model = VB._model(dev, "laplace", "nerfacto-laplace", chunk=CHUNK)
        ecfg = E.LaplaceConfig(load_config=tmp_path / "cfg" / "config.yml", output_path=tmp_path / f"l{vb}.json", n_iters=7,
                               eval_depth=False)
        torch.manual_seed(123)
        with torch.cuda.device(dev):
            res[vb], launches = _launch_names(lambda: E.run_eval(ecfg, model, eval_set, fused=True, view_batch=vb))
        assert ("generate_rays_views" in launches) == (vb == 4), (vb, launches)
    _same_metrics(res)


def _member(dev, seed):
    from uncertainty_nerf_gs_amd import plugin, synthetic
    import test_gpu_models as TM
    cfg = TM._small_cfg(plugin.MODEL_CONFIGS["active-nerfacto"]())
    model = cfg._target(cfg, num_train_data=4)
    model.load_state_dict(TM._state_dict_from_tensors(synthetic.make_scene_tensors(seed=seed, kind="active", log2T=14, prop_log2T=12),
                                                      "active"))
    model.rays_per_launch = RPL
    return model.to(dev)


def test_ensemble_batch_and_run_eval_view_batch(dev, tmp_path):
    from uncertainty_nerf_gs_amd import ensemble
    from uncertainty_nerf_gs_amd import eval as E
    members = [_member(dev, 5 + i) for i in range(3)]
    batch, singles = VB._cameras(6)
    pipe = ensemble.EnsemblePipeline(members)
    with torch.cuda.device(dev):
        got, launches = _launch_names(lambda: pipe.get_ensemble_outputs_for_cameras(batch, max_views=4))
        want = [pipe.get_ensemble_outputs_for_camera_ray_bundle(cam) for cam in singles]
        torch.cuda.synchronize()
    assert launches.get("generate_rays_views", 0) >= 3 and "generate_rays" not in launches, launches      # every member shares launches
    VB._assert_views_equal(got, want)
    assert float(got[0]["rgb_std"].max()) > 0
    eval_set = [(cam, VB._gt(H, W, 50 + i)) for i, cam in enumerate(singles)]
    res = {}
    for vb in (1, 4):
        ecfg = E.EnsembleConfig(load_config=None, output_path=tmp_path / f"e{vb}.json", eval_depth=False)
        torch.manual_seed(123)
        with torch.cuda.device(dev):
            res[vb], launches = _launch_names(lambda: E.run_eval(ecfg, members, eval_set, fused=True, view_batch=vb))
        assert ("generate_rays_views" in launches) == (vb == 4), (vb, launches)
    _same_metrics(res)
