"""Several camera views per NeRF render call (render.render_cameras, the *_views entry points, get_outputs_for_cameras,
run_eval(view_batch=...)): every view of a shared launch is BIT-identical to the single-view path with that view's camera
and seed -- torch.equal, no tolerance.  The single-view path is what the oracle gates, so no oracle run is needed here.

Shapes, the smallest at which the views kernels can go wrong: 29 x 37 = 1,073 rays per view is no multiple of 32 or 64 (waves
and tiles straddle two views), 37 is no multiple of 8 and 29 none of 4 or 8 (ragged pixel patches), chunk_rays = 512 gives
three clip chunks per view with edges in mid-row, and 3 views at rays_per_launch = 2,560 make two launch groups of
unequal size (2 + 1 views)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 29, 37
HW = H * W
CHUNK, RPL = 512, 2560
SEEDS = (1234, 77, 900001)


def _poses(n, start=0.3, step=0.9):
    from uncertainty_nerf_gs_amd import synthetic
    return torch.stack([synthetic.orbit_c2w(start + step * i, radius=0.6 + 0.02 * i, height=0.15 + 0.03 * i) for i in range(n)])


def _intr(n, h=H, w=W):
    """fx, fy, cx, cy: one of each per view, all different; no principal point on a pixel centre (a fisheye ray through it
    is 0 / 0 = NaN, as upstream, and NaN never compares equal)"""
    return ([0.9 * w + i for i in range(n)], [0.95 * w - i for i in range(n)], [w / 2 + 0.13 + 0.25 * i for i in range(n)],
            [h / 2 - 0.21 - 0.5 * i for i in range(n)])


_TENSORS = {}


def _tensors(kind):
    from uncertainty_nerf_gs_amd import synthetic
    if kind not in _TENSORS:
        _TENSORS[kind] = synthetic.make_scene_tensors(seed=5, kind=kind, log2T=14, prop_log2T=12)
    return _TENSORS[kind]


def _scene(dev, kind, chunk=CHUNK, precision=None, **field_kw):
    """kind: "plain" (nerfacto: the MC-dropout field with K = 0), "active", "mcdropout" (K = 3, p = 0.2)"""
    from uncertainty_nerf_gs_amd import synthetic
    if kind == "mcdropout":
        field_kw = dict(dict(K=3, seed=SEEDS[0], p_drop=0.2), **field_kw)
    scene = synthetic.scene_to_device(_tensors("active" if kind == "active" else "mcdropout"), dev, **field_kw)
    scene.chunk_rays = chunk
    if precision is not None:
        scene.field.precision = precision
    return scene


def _rays(dev, poses, intr, **kw):
    """per-view single-frame rays, and the same from ONE launch"""
    from uncertainty_nerf_gs_amd import ops
    fx, fy, cx, cy = intr
    singles = [ops.generate_rays(poses[v], fx[v], fy[v], cx[v], cy[v], H, W, dev, camera_type=kw.get("camera_type", 1),
                                 distortion=None if kw.get("distortions") is None else kw["distortions"][v])[:2]
               for v in range(len(poses))]
    o, d = ops.generate_rays_views(poses, fx, fy, cx, cy, H, W, dev, **kw)
    return singles, o, d


@pytest.mark.parametrize("camera_type", [1, 2, 8])
def test_ray_generator_views_equal_single_frames(dev, camera_type):
    lens = [None, (-0.05, 0.01, 0.0, 0.0, 0.002, -0.001), (0.08, 0.0, 0.0, 0.0, 0.0, 0.0)]
    singles, o, d = _rays(dev, _poses(3), _intr(3), camera_type=camera_type, distortions=lens)
    assert o.shape == d.shape == (3 * HW, 3)
    for v, (ov, dv) in enumerate(singles):
        assert torch.equal(o[v * HW:(v + 1) * HW], ov) and torch.equal(d[v * HW:(v + 1) * HW], dv), v
    assert torch.isfinite(d).all() and not torch.equal(singles[0][1], singles[1][1])


def test_clip_bounds_are_numbered_inside_each_view(dev):
    """weights_pdf_resample, then composite_var / composite_moments, over three views in one call against three
    single-view calls: bins, prop depths, outputs, and the [9, 2] clip buffer against the three [3, 2] ones"""
    from uncertainty_nerf_gs_amd import ops, render
    scene = _scene(dev, "active")
    scene.workspace = None                              # every result a tensor of its own
    singles, o, d = _rays(dev, _poses(3), _intr(3))
    views = ops.RayViews(3, HW)
    cpv = ops.clip_rows_per_view(HW, CHUNK)
    assert cpv == 3
    clip = ops.new_clip_buffer(3 * cpv * CHUNK, CHUNK, dev)
    sb, pds = render.sample_rays(scene, o, d, clip, 0, image_width=W, views=views)
    one = []
    for ov, dv in singles:
        c = ops.new_clip_buffer(HW, CHUNK, dev)
        one.append((c,) + tuple(render.sample_rays(scene, ov, dv, c, 0, image_width=W)))
    assert clip.shape == (9, 2) and torch.equal(clip, torch.cat([c for c, _, _ in one]))
    assert torch.isfinite(clip).all() and bool((clip[:, 1] > 0).all())                  # every row was filled
    assert torch.equal(sb, torch.cat([s for _, s, _ in one]))
    for lvl in range(2):
        assert torch.equal(pds[lvl], torch.cat([p[lvl] for _, _, p in one]))
    # composite_var on the ACTIVE rows (the field has no per-view value in this mode: one call over all rays)
    near, far = scene.near, scene.far
    _, rows, beta, _ = ops.field_fwd(o, d, sb, scene.field, near, far, 0, packed=True)
    dens, rgb, beta2, _ = ops.field_fwd(o, d, sb, scene.field, near, far, 0)
    for density, colour, b in ((None, rows, beta), (dens, rgb, beta2)):
        got = ops.composite_var(density, colour, sb, near, far, beta=b, clip_minmax=clip, chunk_rays=CHUNK, views=views)
        for v, (c, s, _) in enumerate(one):
            sl = slice(v * HW, (v + 1) * HW)
            want = ops.composite_var(None if density is None else density[:, sl].contiguous(), colour[:, sl].contiguous(), s, near,
                                     far, beta=b[sl].contiguous(), clip_minmax=c, ray_offset=0, chunk_rays=CHUNK)
            assert torch.equal(got[:, sl], want), v
    # composite_moments on K = 3 passes of packed and plain rows
    mc = _scene(dev, "mcdropout")
    mc.workspace = None
    for packed in (True, False):
        parts = [ops.field_fwd(ov, dv, s, mc.field, near, far, 0, packed=packed) for (ov, dv), (_, s, _) in zip(singles, one)]
        density = None if packed else torch.cat([p[0] for p in parts], dim=1)
        colour = torch.cat([p[1] for p in parts], dim=1)
        mean, var = ops.composite_moments(density, colour, sb, near, far, clip_minmax=clip, chunk_rays=CHUNK, views=views)
        for v, (c, s, _) in enumerate(one):
            m1, v1 = ops.composite_moments(parts[v][0], parts[v][1], s, near, far, clip_minmax=c, ray_offset=0, chunk_rays=CHUNK)
            assert torch.equal(mean[v * HW:(v + 1) * HW], m1) and torch.equal(var[v * HW:(v + 1) * HW], v1), (packed, v)


@pytest.mark.parametrize("precision", ["f16", "f16x2"])
@pytest.mark.parametrize("image_width", [W, 0])
def test_field_views_draw_each_views_own_masks(dev, precision, image_width):
    """MCDROPOUT K = 3, p = 0.2, three seeds, packed rows: one call over three views against three single calls with
    `seed` and ray_offset = 0 set per view; and the same call with ONE view against unerf_field_fwd"""
    from uncertainty_nerf_gs_amd import ops, render
    scene = _scene(dev, "mcdropout", precision=precision)
    scene.workspace = None
    f, near, far = scene.field, scene.near, scene.far
    singles, o, d = _rays(dev, _poses(3), _intr(3))
    sb, _ = render.sample_rays(scene, o, d, None, 0, want_prop_depth=False)
    _, rows, _, _ = ops.field_fwd(o, d, sb, f, near, far, 0, image_width=image_width, packed=True,
                                  views=ops.RayViews(3, HW, SEEDS))
    assert rows.shape == (3, 3 * HW, 48, 4) and torch.isfinite(rows).all()
    want = []
    for v, (ov, dv) in enumerate(singles):
        f.seed = SEEDS[v]
        sl = slice(v * HW, (v + 1) * HW)
        want.append(ops.field_fwd(ov, dv, sb[sl].contiguous(), f, near, far, 0, image_width=image_width, packed=True)[1])
        assert torch.equal(rows[:, sl], want[v]), v
    # the seeds matter (same rays and bins would otherwise give the same rows), and so does the frame-local counter
    f.seed = SEEDS[0]
    other = ops.field_fwd(singles[1][0], singles[1][1], sb[HW:2 * HW].contiguous(), f, near, far, 0, packed=True)[1]
    assert not torch.equal(other, want[1])
    shifted = ops.field_fwd(o, d, sb, f, near, far, 0, image_width=image_width, packed=True)[1]       # counter runs through
    assert torch.equal(shifted[:, :HW], want[0]) and not torch.equal(shifted[:, HW:2 * HW], other)
    # one view = the plain call; unpacked outputs too
    f.seed = 4242
    a = ops.field_fwd(singles[2][0], singles[2][1], sb[2 * HW:].contiguous(), f, near, far, 0, image_width=image_width)
    b = ops.field_fwd(singles[2][0], singles[2][1], sb[2 * HW:].contiguous(), f, near, far, 0, image_width=image_width,
                      views=ops.RayViews(1, HW, (4242,)))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # ACTIVE and K = 0 have no per-view value: the views call runs the kernels of the plain call
    for kind in ("active", "plain"):
        sc = _scene(dev, kind, precision=precision)
        sc.workspace = None
        a = ops.field_fwd(o, d, sb, sc.field, near, far, 0, image_width=image_width, packed=True)
        b = ops.field_fwd(o, d, sb, sc.field, near, far, 0, image_width=image_width, packed=True, views=ops.RayViews(3, HW))
        assert torch.equal(a[1], b[1]) and (a[2] is None or torch.equal(a[2], b[2])), kind


def _assert_views_equal(batch, singles):
    assert len(batch) == len(singles)
    for v, (b, s) in enumerate(zip(batch, singles)):
        assert set(b) == set(s), (v, sorted(b), sorted(s))
        for k in s:
            assert b[k].shape == s[k].shape and torch.equal(b[k], s[k]), f"view {v}: {k}"


def _loop(scene, poses, intr, h, w, seeds=None, **kw):
    """the single-view path: render_camera per view, for MC-dropout with scene.field.seed = seeds[v]"""
    from uncertainty_nerf_gs_amd import render
    fx, fy, cx, cy = intr
    dist, ctype = kw.pop("distortion", None), kw.pop("camera_type", 1)
    outs, saved = [], scene.field.seed
    for v in range(len(poses)):
        if seeds is not None:
            scene.field.seed = seeds[v]
        outs.append(render.render_camera(scene, poses[v], fx[v], fy[v], cx[v], cy[v], h, w,
                                         distortion=None if dist is None else dist[v], camera_type=ctype, **kw))
    scene.field.seed = saved
    return outs


def _batch(scene, poses, intr, h, w, seeds=None, groups=None, **kw):
    """render_cameras, with the number of shared ray-generator launches it made"""
    from uncertainty_nerf_gs_amd import ops, render
    ops.TIMER = ops.KernelTimer()
    try:
        outs = render.render_cameras(scene, poses, *intr, h, w, seeds=seeds, **kw)
        launches = {k: len(v) for k, v in ops.TIMER.events.items()}
    finally:
        ops.TIMER = None
    if groups == 0:       # the per-camera loop
        assert "generate_rays_views" not in launches and launches["generate_rays"] >= len(poses), launches
    elif groups is not None:
        assert launches.get("generate_rays_views", 0) == groups and "generate_rays" not in launches, launches
    return outs


E2E_KW = {"plain": {}, "active": dict(keep_density=True), "mcdropout": {}}


@pytest.mark.parametrize("kind", ["plain", "active", "mcdropout"])
def test_render_cameras_equals_the_loop(dev, kind):
    """three views in two launch groups (2 + 1); the batch twice on the same scene object -- the scratch arena is dirty and a
    previous frame's buffers exist -- with the same bits"""
    from uncertainty_nerf_gs_amd import render
    scene = _scene(dev, kind)
    assert render.view_batch_loop_reason(scene) is None
    poses, intr = _poses(3), _intr(3)
    seeds = SEEDS if kind == "mcdropout" else None
    kw = dict(rays_per_launch=RPL, **E2E_KW[kind])
    with torch.cuda.device(dev):
        first = _batch(scene, poses, intr, H, W, seeds, groups=2, **kw)
        want = _loop(scene, poses, intr, H, W, seeds, **kw)
        again = _batch(scene, poses.to(dev), intr, H, W, seeds, groups=2, **kw)
        torch.cuda.synchronize()
    _assert_views_equal(first, want)
    _assert_views_equal(again, want)
    assert first[0]["rgb"].shape == (H, W, 3) and not torch.equal(want[0]["rgb"], want[1]["rgb"])
    if kind == "active":
        assert first[0]["density"].shape == (H, W, 48)
    if kind == "mcdropout":
        assert float(first[1]["rgb_std"].max()) > 0
        with torch.cuda.device(dev):      # seeds=None: every view under the field's own seed
            _assert_views_equal(_batch(scene, poses, intr, H, W, None, groups=2, **kw), _loop(scene, poses, intr, H, W, None, **kw))


@pytest.mark.parametrize("kind", ["active", "mcdropout"])
def test_sixteen_views_share_one_default_launch_group(dev, kind):
    """16 views of 48 x 64 with default chunking (32,768 rays: one clip row per view) and the default launch group"""
    h, w = 48, 64
    scene = _scene(dev, kind, chunk=1 << 15)
    poses, intr = _poses(16, step=0.37), _intr(16, h, w)
    seeds = tuple(range(100, 116)) if kind == "mcdropout" else None
    with torch.cuda.device(dev):
        got = _batch(scene, poses, intr, h, w, seeds, groups=1)
        want = _loop(scene, poses, intr, h, w, seeds)
        torch.cuda.synchronize()
    _assert_views_equal(got, want)


def test_render_cameras_with_a_crop_box_lenses_fisheye_and_a_side_stream(dev):
    from uncertainty_nerf_gs_amd import ops
    scene = _scene(dev, "mcdropout")
    poses, intr = _poses(3), _intr(3)
    kw = dict(rays_per_launch=RPL)
    obb = (ops.world_to_box(torch.eye(3), torch.tensor([0.03, 0.02, -0.01])), torch.tensor([0.4, 0.5, 0.3]))
    lens = [None, (-0.05, 0.01, 0.0, 0.0, 0.002, -0.001), (0.08, 0.0, 0.0, 0.0, 0.0, 0.0)]
    with torch.cuda.device(dev):
        # an oriented crop box that some rays miss
        got = _batch(scene, poses, intr, H, W, SEEDS, groups=2, obb=obb, **kw)
        want = _loop(scene, poses, intr, H, W, SEEDS, obb=obb, **kw)
        _assert_views_equal(got, want)
        acc = torch.stack([o["accumulation"] for o in want])
        assert 0.05 < float((acc.abs() < 1e-6).float().mean()) < 0.95      # some rays miss the box, some hit it
        # per-view lens parameters; fisheye
        _assert_views_equal(_batch(scene, poses, intr, H, W, SEEDS, groups=2, distortion=lens, **kw),
                            _loop(scene, poses, intr, H, W, SEEDS, distortion=lens, **kw))
        _assert_views_equal(_batch(scene, poses, intr, H, W, SEEDS, groups=2, camera_type=2, **kw),
                            _loop(scene, poses, intr, H, W, SEEDS, camera_type=2, **kw))
        # on a side stream
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            on_side = _batch(scene, poses, intr, H, W, SEEDS, groups=2, **kw)
        side.synchronize()
        _assert_views_equal(on_side, _loop(scene, poses, intr, H, W, SEEDS, **kw))
        torch.cuda.synchronize()


def test_render_cameras_loops_where_launches_cannot_be_shared(dev):
    """mixed camera types, an fp32 field, a view larger than half a launch group: the loop, with the loop's results"""
    from uncertainty_nerf_gs_amd import render
    scene = _scene(dev, "mcdropout")
    poses, intr = _poses(3), _intr(3)
    with torch.cuda.device(dev):
        want = _loop(scene, poses, intr, H, W, SEEDS, rays_per_launch=RPL)
        big = _batch(scene, poses, intr, H, W, SEEDS, groups=0, rays_per_launch=2048)          # 1,073 > 2,048 / 2
        _assert_views_equal(big, _loop(scene, poses, intr, H, W, SEEDS, rays_per_launch=2048))
        _assert_views_equal(big, want)
        mixed = _batch(scene, poses, intr, H, W, SEEDS, groups=0, rays_per_launch=RPL, camera_type=[1, 2, 1])
        _assert_views_equal([mixed[0], mixed[2]], [want[0], want[2]])
        scene.field.precision = "fp32"
        assert "fp32" in render.view_batch_loop_reason(scene)
        _assert_views_equal(_batch(scene, poses, intr, H, W, SEEDS, groups=0, rays_per_launch=RPL),
                            _loop(scene, poses, intr, H, W, SEEDS, rays_per_launch=RPL))
        torch.cuda.synchronize()


def _model(dev, kind, method, chunk=None, **attrs):
    from uncertainty_nerf_gs_amd import plugin
    import test_gpu_models as TM
    cfg = TM._small_cfg(plugin.MODEL_CONFIGS[method]())
    if chunk is not None:
        cfg.eval_num_rays_per_chunk = chunk
    if kind == "mcdropout":
        cfg.mc_samples = 3
    model = cfg._target(cfg, num_train_data=4)
    model.load_state_dict(TM._state_dict_from_tensors(_tensors(kind), kind))
    for k, v in attrs.items():
        setattr(model, k, v)
    model.rays_per_launch = RPL
    return model.to(dev)


def _cameras(n, h=H, w=W):
    from types import SimpleNamespace
    fx, fy, cx, cy = _intr(n, h, w)
    poses = _poses(n)
    batch = SimpleNamespace(camera_to_worlds=poses, fx=torch.tensor(fx), fy=torch.tensor(fy), cx=torch.tensor(cx),
                            cy=torch.tensor(cy), height=h, width=w)
    singles = [SimpleNamespace(camera_to_worlds=poses[v][None], fx=torch.tensor([fx[v]]), fy=torch.tensor([fy[v]]),
                               cx=torch.tensor([cx[v]]), cy=torch.tensor([cy[v]]), height=h, width=w) for v in range(n)]
    return batch, singles


@pytest.mark.parametrize("kind,method", [("mcdropout", "nerfacto-mcdropout"), ("active", "active-nerfacto")])
def test_model_batch_equals_successive_single_camera_calls(dev, kind, method):
    """two models with the same seed: get_outputs_for_cameras of 5 cameras, max_views = 2, against five
    get_outputs_for_camera calls; the MC-dropout frame counters both end at 5"""
    attrs = dict(seed=31) if kind == "mcdropout" else {}
    a, b = _model(dev, kind, method, chunk=CHUNK, **attrs), _model(dev, kind, method, chunk=CHUNK, **attrs)
    batch, singles = _cameras(5)
    with torch.cuda.device(dev):
        got = a.get_outputs_for_cameras(batch, max_views=2)
        want = [b.get_outputs_for_camera(cam) for cam in singles]
        torch.cuda.synchronize()
    _assert_views_equal(got, want)
    if kind == "mcdropout":
        assert a.frame_counter == b.frame_counter == 5
        assert not torch.equal(got[0]["rgb_std"], got[1]["rgb_std"])
        with torch.cuda.device(dev):     # and the next frame continues the same stream of seeds
            assert torch.equal(a.get_outputs_for_camera(singles[0])["rgb"], b.get_outputs_for_camera(singles[0])["rgb"])
    with pytest.raises(ValueError, match="max_views"):
        a.get_outputs_for_cameras(batch, max_views=17)


def test_models_that_loop_return_the_loops_results_and_two_sizes_raise(dev):
    from types import SimpleNamespace
    batch, singles = _cameras(3)
    # dropout_masks="torch": the frames' masks come from a torch generator, one frame at a time
    gens = [torch.Generator().manual_seed(9) for _ in range(2)]
    a, b = (_model(dev, "mcdropout", "nerfacto-mcdropout", seed=31, dropout_masks="torch", mask_generator=g) for g in gens)
    with torch.cuda.device(dev):
        _assert_views_equal(a.get_outputs_for_cameras(batch), [b.get_outputs_for_camera(cam) for cam in singles])
    assert a.frame_counter == b.frame_counter == 3
    # Laplace: the deterministic mean-head render, camera by camera
    la, lb = (_model(dev, "laplace", "nerfacto-laplace") for _ in range(2))
    with torch.cuda.device(dev):
        _assert_views_equal(la.get_outputs_for_cameras(batch), [lb.get_outputs_for_camera(cam) for cam in singles])
        torch.cuda.synchronize()
    two = SimpleNamespace(**{**batch.__dict__, "height": torch.tensor([H, H, H + 1])})
    for m in (a, la):
        with pytest.raises(ValueError, match="one image size"):
            m.get_outputs_for_cameras(two)


TIMING_KEYS = ("num_rays_per_sec", "fps", "render_rays_per_sec")


def _gt(h, w, seed):
    return torch.rand(h, w, 3, generator=torch.Generator().manual_seed(seed))


def test_run_eval_view_batch_active_nerfacto(dev, tmp_path):
    from uncertainty_nerf_gs_amd import eval as E
    _, singles = _cameras(6)
    eval_set = [(cam, _gt(H, W, 50 + i)) for i, cam in enumerate(singles)]
    res = {}
    for vb in (1, 4):
        model = _model(dev, "active", "active-nerfacto")
        ecfg = E.ActiveNerfactoConfig(load_config=None, output_path=tmp_path / f"a{vb}.json", eval_depth=False)
        res[vb] = E.run_eval(ecfg, model, eval_set, view_batch=vb)
    assert set(res[1]) == set(res[4]) and set(TIMING_KEYS) <= set(res[4])
    for k in res[1]:
        if k not in TIMING_KEYS:
            assert res[4][k] == res[1][k], k
        else:
            assert res[4][k] > 0


def test_run_eval_view_batch_splat(dev, tmp_path):
    from uncertainty_nerf_gs_amd import eval as E
    from uncertainty_nerf_gs_amd import models, synthetic
    import test_gpu_splat as TS
    m, cam, g = TS._fixture_model(dev)
    fx, fy, cx, cy, Hs, Ws = (float(v) for v in g["intr"])
    Hs, Ws = int(Hs), int(Ws)
    cams = [models.Camera(synthetic.orbit_c2w(0.4 + 0.8 * i, radius=2.5, height=0.5), fx + i, fy, cx, cy, Hs, Ws) for i in range(6)]
    eval_set = [(c, torch.cat([_gt(Hs, Ws, 70 + i), torch.ones(Hs, Ws, 1)], dim=-1)) for i, c in enumerate(cams)]
    res = {}
    for vb in (1, 4):
        ecfg = E.ActiveSplatfactoConfig(load_config=None, output_path=tmp_path / f"s{vb}.json")
        res[vb] = E.run_eval(ecfg, m, eval_set, view_batch=vb)
    assert set(res[1]) == set(res[4])
    for k in res[1]:
        if k not in TIMING_KEYS:
            assert res[4][k] == res[1][k], k
