"""The pose normal equations on the GPU (unerf_pose_normal_eq_accumulate / _finish): every case of pose_normal_eq_cases inside
the derived bound on every entry, exact counts, the exact integer family bit for bit, symmetry, grouping and repeatability,
planted non-finite terms, the mask, guards and streams; then whole frames through the nerfacto and splat models."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pose_normal_eq_cases as NC

pytestmark = pytest.mark.gpu
TILE = NC.TILE
CASES = NC.all_cases()


def _dev(inp, dev):
    return {k: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in inp.items()}


def _solve(dev, inp, groups=None, N_frame=None):
    """inputs -> pose_normal_eq_finish's dictionary; groups: [(start, stop)] launch groups in the order given (default: one)"""
    from uncertainty_nerf_gs_amd import ops
    d = _dev(inp, dev)
    N, _, P = inp["jac"].shape
    N_frame = N if N_frame is None else N_frame
    with torch.cuda.device(dev):
        ws = ops.pose_normal_eq_workspace(N_frame, P, dev)
        for a, b in groups or [(0, N)]:
            ops.pose_normal_eq_accumulate(ws, d["jac"][a:b], None if d["val"] is None else d["val"][a:b],
                                          None if d["target"] is None else d["target"][a:b],
                                          None if d["weight"] is None else d["weight"][a:b], None if d["mask"] is None else d["mask"][a:b],
                                          pixel_offset=a)
        return ops.pose_normal_eq_finish(ws, N_frame, P)


def _bits(out):
    return np.concatenate([out["information"].reshape(-1), out["gradient"], [out["chi2"], out["n_used"], out["n_skipped"]]]).view(np.int64)


def _check(what, out, ref, N_frame=None):
    worst, where = NC.excess(out, ref, N_frame)
    print(f"BOUND {what}: worst |got - ref| / bound = {worst:.3f} at {where}")
    assert worst <= 1.0, (what, worst, where)
    assert (out["n_used"], out["n_skipped"]) == (ref["n_used"], ref["n_skipped"]), what
    assert np.array_equal(out["information"], out["information"].T), what


@pytest.mark.parametrize("N", NC.NS)
def test_parity_counts_and_symmetry(dev, N):
    for c in (c for c in CASES if c.N == N):
        inp = NC.make_inputs(c)
        out = _solve(dev, inp)
        _check(c.id, out, NC.reference(inp))
        assert out["information"].shape == (c.P, c.P) and out["gradient"].shape == (c.P,)
        if not c.resid:
            assert not out["gradient"].any() and out["chi2"] == 0.0 and not np.signbit(out["gradient"]).any()


@pytest.mark.parametrize("C_,P", [(3, 6), (5, 12), (1, 1), (3, 7)])
def test_exact_family_bit_for_bit(dev, C_, P):
    inp = NC.exact_inputs(3 * TILE + 5, C_, P, seed=40 + P)
    H, g, chi2, used = NC.exact_reference(inp)
    out = _solve(dev, inp)
    want = np.concatenate([H.reshape(-1), g, [chi2, used, 0]]).astype(np.float64)
    assert np.array_equal(_bits(out), want.view(np.int64))


@pytest.mark.parametrize("C_,P", [(3, 6), (5, 12), (3, 4), (1, 7)])
def test_grouping_and_repeatability(dev, C_, P):
    N = 3 * TILE + 5
    inp = NC.make_inputs(NC.Case(N, C_, P, "nc", True, True, seed=77 + P))
    groups = [(k * TILE, min((k + 1) * TILE, N)) for k in range(4)]
    one = _bits(_solve(dev, inp))
    assert np.array_equal(one, _bits(_solve(dev, inp)))
    assert np.array_equal(one, _bits(_solve(dev, inp, groups)))
    assert np.array_equal(one, _bits(_solve(dev, inp, groups[::-1])))
    assert np.array_equal(one, _bits(_solve(dev, inp, [groups[2], (0, 2 * TILE), groups[3]])))
    # a tile's partial does not depend on the other tiles: tile 1 alone in a frame = the frame with everything else masked out
    alone = {k: None if v is None else v[TILE:2 * TILE] for k, v in inp.items()}
    rest = dict(inp, mask=inp["mask"] * (np.arange(N) // TILE == 1).astype(np.uint8))
    assert np.array_equal(_bits(_solve(dev, alone)), _bits(_solve(dev, rest)))


PLANTS = (("jac", np.nan), ("jac", np.inf), ("jac", -np.inf), ("val", np.nan), ("val", np.inf), ("target", -np.inf), ("weight", np.nan),
          ("weight", np.inf), ("weight", -np.inf), ("weight", -1.0))


@pytest.mark.parametrize("weights", ["nc", "n"])
@pytest.mark.parametrize("C_,P", [(3, 6), (5, 12)])
def test_planted_non_finite_terms(dev, weights, C_, P):
    N = 2 * TILE + 7
    inp = NC.make_inputs(NC.Case(N, C_, P, weights, False, True, seed=5 + P))
    clean = NC.reference(inp)
    assert clean["n_skipped"] == 0
    spots = [0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, N - 1]       # first and last pixel of a tile and of the frame
    terms = set()
    for i, (key, v) in enumerate(PLANTS + PLANTS[:2]):
        n, c = spots[i % len(spots)], (i + i // len(spots)) % C_
        if key == "jac":
            inp["jac"][n, c, (3 * i) % P] = v
        elif key == "weight" and weights == "n":
            inp["weight"][n] = v
        else:
            inp[key][n, c] = v
        terms |= {(n, cc) for cc in range(C_)} if key == "weight" and weights == "n" else {(n, c)}
    ref = NC.reference(inp)
    assert ref["n_skipped"] == len(terms) and ref["n_used"] == N * C_ - len(terms)
    out = _solve(dev, inp)
    _check(f"planted w={weights} C={C_} P={P}", out, ref)
    assert np.isfinite(_bits(out).view(np.float64)).all()
    assert float(NC.excess(out, clean)[0]) > 1.0                      # the planted terms did carry weight before


def test_masked_pixels_contribute_nothing(dev):
    N, C_, P = TILE + 300, 3, 6
    inp = NC.make_inputs(NC.Case(N, C_, P, "n", True, True, seed=21))
    clean = _bits(_solve(dev, inp))
    off = inp["mask"] == 0
    assert off[0] or off.sum() > 10
    for key in ("jac", "val", "target", "weight"):
        inp[key][off] = np.nan
    inp["weight"][off] = -np.inf
    out = _solve(dev, inp)
    assert out["n_skipped"] == 0 and out["n_used"] == int((~off).sum()) * C_
    assert np.array_equal(_bits(out), clean)


def test_guards_and_streams(dev, lib):
    h = lib.load()
    N, C_, P = 2 * TILE + 3, 3, 7
    inp = NC.make_inputs(NC.Case(N, C_, P, "nc", True, True, seed=31))
    want = _bits(_solve(dev, inp))
    d = _dev(inp, dev)
    row, words = lib.pose_neq_row(P), h.unerf_pose_normal_eq_workspace_bytes(N, P) // 8
    with torch.cuda.device(dev):
        ws = torch.zeros(words + 32, device=dev, dtype=torch.float64)
        ws[words:] = 555.0
        buf = torch.full((row + 16,), 777.0, device=dev, dtype=torch.float64)
        st = torch.cuda.current_stream().cuda_stream
        assert h.unerf_pose_normal_eq_accumulate(d["jac"].data_ptr(), d["val"].data_ptr(), d["target"].data_ptr(), d["weight"].data_ptr(), 1,
                                                 d["mask"].data_ptr(), N, C_, P, 0, N, ws.data_ptr(), (words + 32) * 8, st) == 0
        assert h.unerf_pose_normal_eq_finish(ws.data_ptr(), (words + 32) * 8, N, P, buf.data_ptr() + 8 * 8, st) == 0
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:8] == 777.0).all() and (got[8 + row:] == 777.0).all() and bool((ws[words:] == 555.0).all())
        assert np.array_equal(got[8:8 + row].view(np.int64), want)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            out = _solve(dev, inp)
        side.synchronize()
        assert np.array_equal(_bits(out), want)
        # refused calls launch nothing: the workspace stays as it is
        before = ws.clone()
        assert h.unerf_pose_normal_eq_accumulate(d["jac"].data_ptr(), None, None, None, 0, None, N, C_, P, 5, N + 5, ws.data_ptr(),
                                                 (words + 32) * 8, st) == -1
        torch.cuda.synchronize()
        assert torch.equal(ws, before)


# ---- whole frames --------------------------------------------------------------------------------------------------------
def _camera(H, W, c2w, f):
    return SimpleNamespace(camera_to_worlds=c2w[None], fx=torch.tensor([f]), fy=torch.tensor([f * 1.05]), cx=torch.tensor([W / 2 + 0.2]),
                           cy=torch.tensor([H / 2 - 0.1]), height=H, width=W)


def _nerf_model(dev, method):
    import test_gpu_models as TM
    from uncertainty_nerf_gs_amd import plugin, synthetic
    cfg = TM._small_cfg(plugin.MODEL_CONFIGS[method]())
    model = cfg._target(cfg, num_train_data=4)
    if method == "active-nerfacto":
        t = synthetic.make_scene_tensors(seed=0, kind="active", log2T=14, prop_log2T=12)
        model.load_state_dict(TM._state_dict_from_tensors(t, "active"))
    else:
        t = synthetic.make_scene_tensors(seed=0, kind="mcdropout", log2T=14, prop_log2T=12)
        t["field"]["average_init_density"] = 0.01
        t["field"]["b1"][0] += 4.6
        model.load_state_dict(TM._nerfacto_upstream_state_dict(t), strict=True)
    return model.to(dev)


def _splat_model(dev, active, mode):
    from uncertainty_nerf_gs_amd import models, synthetic
    cfg = (models.ActiveSplatfactoModelConfig if active else models.SplatfactoModelConfig)()
    cfg.rasterize_mode = mode
    gp = synthetic.make_splat_tensors(7, 3000)
    gp["scales"] = gp["scales"] + 1.5
    m = cfg._target(cfg, num_points=4)
    m.load_state_dict({f"gauss_params.{k}": v for k, v in gp.items() if active or k != "log_uncertainties"})
    return m.to(dev).eval()


def _frame_checks(what, info_fn, jac_fn, unc_fn, cam, H, W, rpls):
    """the end-to-end checks of one model and camera; rpls: the rays_per_launch values the result must not depend on"""
    from uncertainty_nerf_gs_amd import posegrad
    kw0 = dict(rays_per_launch=rpls[0]) if rpls else {}
    jv = jac_fn(cam)
    J = jv["jacobian"][..., :3, :].reshape(H * W, 3, 6).cpu().numpy()
    val = jv["values"][..., :3].contiguous()
    assert np.abs(J).max() > 0
    # the image the frame renders itself: nothing to correct
    own = info_fn(cam, image=val, **kw0)
    assert sorted(own) == sorted(["information", "gradient", "chi2", "n_used", "n_skipped", "covariance", "rank", "step"])
    assert own["chi2"] == 0.0 and not own["gradient"].any() and not own["step"].any()
    assert own["n_used"] == H * W * 3 and own["n_skipped"] == 0
    # the information = the float64 reduction of the Jacobian the separately tested kernel returns
    ref = NC.reference(dict(jac=J))
    _check(what + " information", dict(own, gradient=np.zeros(6), chi2=0.0), ref, H * W)
    bare = info_fn(cam, **kw0)
    assert "step" not in bare and np.array_equal(bare["information"], own["information"]) and bare["chi2"] == 0.0
    # a target that asks for the twist xi0, built on the host in float64 from those outputs
    xi0 = np.random.default_rng(12).standard_normal(6)
    xi0 *= 1e-3 / np.linalg.norm(xi0)
    v64 = val.reshape(H * W, 3).cpu().numpy().astype(np.float64)
    target = (v64 + J.astype(np.float64) @ xi0).astype(np.float32)
    got = info_fn(cam, image=torch.from_numpy(target.reshape(H, W, 3)), **kw0)
    J64, r64 = J.astype(np.float64), v64 - target.astype(np.float64)
    H64, g64 = np.einsum("nca,ncb->ab", J64, J64), np.einsum("nc,nca->a", r64, J64)
    host = -np.linalg.solve(H64, g64)
    rel = np.linalg.norm(got["step"] - host) / np.linalg.norm(host)
    print(f"STEP {what}: |step - host solve| / |host solve| = {rel:.3e}; |step - xi0| / |xi0| = "
          f"{np.linalg.norm(got['step'] - xi0) / np.linalg.norm(xi0):.3e}; cond(H) = {np.linalg.cond(H64):.3e}; rank {got['rank']}")
    assert rel <= 1e-9
    _check(what + " target", got, NC.reference(dict(jac=J, val=v64.astype(np.float32), target=target)), H * W)
    # weights and a mask; [H,W] and [H,W,1] are the same thing
    g = np.random.default_rng(13)
    wt = torch.from_numpy(np.exp(g.uniform(-1, 1, (H, W))).astype(np.float32))
    wc = torch.from_numpy(np.exp(g.uniform(-1, 1, (H, W, 3))).astype(np.float32))
    mk = torch.from_numpy(g.uniform(0, 1, (H, W)) < 0.7)
    tg = torch.from_numpy(target.reshape(H, W, 3))
    a = info_fn(cam, image=tg, weights=wt, mask=mk, **kw0)
    b = info_fn(cam, image=tg, weights=wt[..., None], mask=mk, **kw0)
    assert np.array_equal(_bits(a), _bits(b)) and a["n_used"] == int(mk.sum()) * 3
    _check(what + " weights [H,W]", a, NC.reference(dict(jac=J, val=v64.astype(np.float32), target=target, weight=wt.reshape(-1).numpy(),
                                                           mask=mk.reshape(-1).numpy().astype(np.uint8))), H * W)
    cw = info_fn(cam, image=tg, weights=wc, **kw0)
    _check(what + " weights [H,W,C]", cw, NC.reference(dict(jac=J, val=v64.astype(np.float32), target=target,
                                                             weight=wc.reshape(-1, 3).numpy())), H * W)
    for rpl in rpls[1:]:
        assert np.array_equal(_bits(info_fn(cam, image=tg, weights=wc, rays_per_launch=rpl)), _bits(cw)), rpl
    # one channel of the image, by name
    one = info_fn(cam, image=tg, channels=("g",), **kw0)
    _check(what + " channel g", one, NC.reference(dict(jac=J[:, 1:2], val=v64[:, 1:2].astype(np.float32), target=target[:, 1:2])), H * W)
    # the covariance closes the loop with the propagation
    assert own["covariance"].shape == (6, 6) and np.array_equal(own["covariance"], own["covariance"].T)
    unc = unc_fn(cam, torch.from_numpy(own["covariance"]))
    assert all(bool(torch.isfinite(v).all()) for v in unc.values()) and float(unc["rgb_std_pose"].max()) > 0


@pytest.mark.parametrize("method", ["nerfacto", "active-nerfacto"])
@pytest.mark.parametrize("H,W,rpls", [(16, 24, (1 << 20,)), (28, 40, (TILE, 4 * TILE, 1 << 20))])
def test_nerfacto_frames(dev, method, H, W, rpls):
    from uncertainty_nerf_gs_amd import synthetic
    model = _nerf_model(dev, method)
    cam = _camera(H, W, synthetic.orbit_c2w(0.3), 0.9 * W)
    with torch.cuda.device(dev):
        _frame_checks(f"{method} {W}x{H}", model.get_pose_information_for_camera, model.get_pose_jacobians_for_camera,
                      model.get_pose_uncertainty_for_camera, cam, H, W, rpls)
        with pytest.raises(ValueError, match="multiple of POSE_NEQ_TILE"):
            model.get_pose_information_for_camera(cam, rays_per_launch=TILE + 1)


@pytest.mark.parametrize("active", [True, False])
@pytest.mark.parametrize("mode", ["classic", "antialiased"])
def test_splat_frames(dev, active, mode):
    from uncertainty_nerf_gs_amd import synthetic
    model = _splat_model(dev, active, mode)
    H, W = 40, 56
    cam = SimpleNamespace(camera_to_worlds=synthetic.orbit_c2w(0.9, radius=2.5, height=0.5)[None], fx=torch.tensor([50.0]),
                          fy=torch.tensor([50.0]), cx=torch.tensor([W / 2]), cy=torch.tensor([H / 2]), height=H, width=W)
    with torch.cuda.device(dev):
        _frame_checks(f"splat active={active} {mode}", model.get_splat_pose_information_for_camera,
                      model.get_splat_pose_jacobians_for_camera, model.get_splat_pose_uncertainty_for_camera, cam, H, W, ())


def test_refusals_at_model_level(dev):
    import test_gpu_models as TM
    from uncertainty_nerf_gs_amd import models, plugin, synthetic
    cam = _camera(6, 8, synthetic.orbit_c2w(0.3), 10.0)
    for method in ("nerfacto-mcdropout", "nerfacto-laplace"):
        cfg = TM._small_cfg(plugin.MODEL_CONFIGS[method]())
        with pytest.raises(NotImplementedError, match="not built for"):
            cfg._target(cfg, num_train_data=2).get_pose_information_for_camera(cam)
    m = _splat_model(dev, True, "classic")
    with pytest.raises(NotImplementedError, match="get_splat_pose_information_for_camera"):
        m.get_pose_information_for_camera(cam)
    with pytest.raises(ValueError, match="image must be"):
        m.get_splat_pose_information_for_camera(cam, image=torch.zeros(6, 8, 2))
    with pytest.raises(ValueError, match="weights must be"):
        m.get_splat_pose_information_for_camera(cam, weights=torch.zeros(6, 8, 2))
