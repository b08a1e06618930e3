"""The batched splat pose Jacobian without a GPU: the two entry points are declared, exported and bound with the header's argument
lists and refuse bad arguments before any launch; the model methods check a camera batch before anything touches the GPU; the
per-view projection matrices of a batch are those pose_jacobian_camera builds camera by camera, bit for bit."""
import ctypes as C
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import splat_pose_grad_cases as SPG
from conftest import ROOT

NEW = (("unerf_splat_pose_ptangents_batch", 13), ("unerf_splat_pose_jacobian_batch", 23))


def test_symbols_declared_exported_and_bound(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "unerf.h")).read(), flags=re.S)
    raw = C.CDLL(lib.LIB_PATH)
    for name, n_args in NEW:
        m = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/unerf.h"
        args = [a.strip() for a in m.group(1).split(",") if a.strip()]
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == len(args) == n_args
        # the binding's types, argument by argument: pointers, int, int64_t, float
        for a, t in zip(args, lib.SIGNATURES[name][1]):
            if "*" in a:
                assert t in (C.c_void_p, C.POINTER(C.c_float)), (name, a, t)
            else:
                assert t is {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float}[a.split()[0]], (name, a, t)
        assert getattr(raw, name) is not None and getattr(lib.load(), name) is not None
    assert lib.load().unerf_version() == 1420          # additive: same ABI version


def test_refusals_come_before_any_launch(lib):
    h = lib.load()
    views = (C.c_float * (16 * lib.SPLAT_VIEW_FLOATS))()

    def tan(ptr=16, vw=views, B=2, N=5, proj=16, P=6, H=8, W=8, out=16):
        return h.unerf_splat_pose_ptangents_batch(ptr, ptr, ptr, vw, B, N, proj, P, H, W, 0.01, out, None)

    def jac(ptr=16, ptan=16, cs=3, B=2, N=5, P=6, H=8, W=8, bw=16, flags=0, channels=31, outs=(16, None, None)):
        return h.unerf_splat_pose_jacobian_batch(ptr, ptr, ptr, ptr, ptr, cs, ptr, ptr, None, ptan, None, B, N, P, H, W, bw, flags,
                                                 channels, *outs, None)

    def refused(fn, text, **kw):
        assert fn(**kw) == -1, text
        assert text in h.unerf_last_error(), h.unerf_last_error()

    for fn, who in ((tan, b"splat_pose_ptangents_batch: "), (jac, b"splat_pose_jacobian_batch: ")):
        refused(fn, who + b"B=0 outside [1,16]", B=0)
        refused(fn, who + b"B=17 outside [1,16]", B=17)
        refused(fn, who + b"B*N = 536870912 outside [0,2^29)", B=16, N=1 << 25)
        refused(fn, who + b"B*N = 536870912 outside [0,2^29)", B=1, N=1 << 29)
        refused(fn, who + b"P=0 outside [1,12]", P=0)
        refused(fn, who + b"P=13 outside [1,12]", P=13)
        refused(fn, who + b"null pointer", ptr=None)
    refused(tan, b"null pointer (views_host)", vw=None)
    refused(tan, b"null pointer", proj=None)
    refused(tan, b"null pointer", out=None)
    refused(tan, b"ptangents must be 8-byte aligned for P=6", out=4)
    refused(tan, b"ptangents must be 16-byte aligned for P=7", out=8, P=7)
    refused(tan, b"bad H/W", H=0)
    assert tan(N=0, ptr=None, proj=None, out=None) == 0                 # no splats: not an error, nothing launched
    refused(jac, b"null pointer", ptan=None)
    refused(jac, b"color_stride=2 below 3", cs=2)
    refused(jac, b"channels is empty", channels=0)
    refused(jac, b"unknown channel bits 32", channels=33)
    refused(jac, b"no output asked for", outs=(None, None, None))
    refused(jac, b"unknown flags 2", flags=2)
    refused(jac, b"block_width=17 outside [1,16]", bw=17)
    refused(jac, b"block_width=0 outside [1,16]", bw=0)
    refused(jac, b"ptangents must be 8-byte aligned for P=6", ptan=4)
    refused(jac, b"ptangents must be 16-byte aligned for P=12", ptan=8, P=12)
    refused(jac, b"12000 tiles, the batched lists hold 11999", H=16, W=16 * 12000)
    assert jac(H=0) == 0 and jac(W=0, outs=(None, 16, 16)) == 0         # no pixels: not an error, nothing launched


def test_surface():
    import uncertainty_nerf_gs_amd as pkg
    from uncertainty_nerf_gs_amd import models, ops, plugin, posegrad, splat
    assert callable(ops.splat_pose_ptangents_batch) and callable(ops.splat_pose_jacobian_batch)
    assert "pose_jacobian_cameras" in pkg.__doc__
    sig = inspect.signature(ops.splat_project_batch)
    assert sig.parameters["want_cov3d"].default is False
    sig = inspect.signature(splat.pose_jacobian_cameras)
    assert list(sig.parameters)[:13] == ["gp", "c2ws", "fx", "fy", "cx", "cy", "H", "W", "background", "projs", "pose_covs", "channels",
                                         "want"]
    assert sig.parameters["projs"].default is None and sig.parameters["pose_covs"].default is None
    assert sig.parameters["want"].default == ("proj", "val") and sig.parameters["channels"].default == ops.POSE_CHANNELS
    assert callable(posegrad.splat_view_projection)
    for name in ("get_splat_pose_jacobians_for_cameras", "get_splat_pose_uncertainty_for_cameras"):
        assert name in vars(models.SplatfactoModel)
        assert getattr(models.ActiveSplatfactoModel, name) is getattr(models.SplatfactoModel, name)
        assert inspect.signature(getattr(models.SplatfactoModel, name)).parameters["max_views"].default == 8
        for method in ("active-splatfacto", "splatfacto"):
            assert callable(getattr(plugin.build_model(method, num_points=4), name))


def _cameras(B=3, **kw):
    c2w = torch.from_numpy(np.stack([SPG.frame_c2w()] * B))
    base = dict(camera_to_worlds=c2w, fx=torch.full((B, 1), 10.0), fy=torch.full((B, 1), 10.0), cx=torch.full((B, 1), 4.0),
                cy=torch.full((B, 1), 3.0), height=torch.full((B, 1), 6), width=torch.full((B, 1), 8))
    return SimpleNamespace(**{**base, **kw})


def test_camera_batches_are_checked_before_any_gpu_use(monkeypatch):
    from uncertainty_nerf_gs_amd import plugin, splat

    def never(*a, **kw):
        raise AssertionError("the frame call was reached")

    monkeypatch.setattr(splat, "pose_jacobian_cameras", never)
    monkeypatch.setattr(splat, "pose_jacobian_camera", never)
    m = plugin.build_model("active-splatfacto", num_points=4)
    cov = torch.full((6,), 0.01)
    calls = (lambda cams, **kw: m.get_splat_pose_jacobians_for_cameras(cams, **kw),
             lambda cams, **kw: m.get_splat_pose_uncertainty_for_cameras(cams, cov, **kw))
    for call in calls:
        with pytest.raises(ValueError, match="one image size per batch"):
            call(_cameras(height=torch.tensor([[6], [6], [7]])))
        with pytest.raises(NotImplementedError, match="pinhole"):
            call(_cameras(camera_type=torch.tensor([[1], [2], [1]])))
        for mv in (0, 17, -1):
            with pytest.raises(ValueError, match=f"max_views={mv}"):
                call(_cameras(), max_views=mv)
    with pytest.raises(ValueError, match="2 pose covariances for 3 cameras"):
        m.get_splat_pose_uncertainty_for_cameras(_cameras(), [cov, cov])
    with pytest.raises(ValueError, match="pose_cov is needed"):
        m.get_splat_pose_uncertainty_for_cameras(_cameras(), None)
    with pytest.raises(ValueError, match="basis"):
        m.get_splat_pose_jacobians_for_cameras(_cameras(), basis="quaternion")


def test_plugin_classes_forward_and_the_non_splat_mirrors_raise(monkeypatch):
    """the nerfstudio-facing classes (the real nerfstudio when installed, else the stand-in of tests/stubs)"""
    import sys
    try:
        import nerfstudio  # noqa: F401
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, "tests", "stubs"))
    from uncertainty_nerf_gs_amd import plugin
    cov = torch.full((6,), 0.01)
    specs = plugin.method_specifications()
    cfg = specs["active-nerfacto"].config.pipeline.model
    cfg.log2_hashmap_size, cfg.num_levels, cfg.max_res = 8, 16, 64
    cfg.proposal_net_args_list = [dict(a, log2_hashmap_size=6) for a in cfg.proposal_net_args_list]
    nerf = cfg.setup(scene_box=None, num_train_data=1)
    with pytest.raises(NotImplementedError, match="not a splat"):
        nerf.get_splat_pose_jacobians_for_cameras(_cameras())
    with pytest.raises(NotImplementedError, match="not a splat"):
        nerf.get_splat_pose_uncertainty_for_cameras(_cameras(), cov)
    model = specs["active-splatfacto"].config.pipeline.model.setup(scene_box=None, num_train_data=2,
                                                                   seed_points=(torch.rand(9, 3), torch.zeros(9, 3)))
    seen = []
    monkeypatch.setattr(type(model._mirror), "get_splat_pose_jacobians_for_cameras",
                        lambda self, cameras, **kw: seen.append(("jac", cameras, kw)) or ["j"])
    monkeypatch.setattr(type(model._mirror), "get_splat_pose_uncertainty_for_cameras",
                        lambda self, cameras, pose_cov, **kw: seen.append(("unc", cameras, pose_cov, kw)) or ["u"])
    cams = _cameras()
    assert model.get_splat_pose_jacobians_for_cameras(cams, basis="c2w", max_views=2) == ["j"]
    assert seen[-1] == ("jac", cams, dict(basis="c2w", max_views=2))
    assert model.get_splat_pose_uncertainty_for_cameras(cams, cov, max_views=16) == ["u"]
    assert seen[-1][0] == "unc" and seen[-1][2] is cov and seen[-1][3] == dict(max_views=16)


def test_models_hand_each_camera_its_own_projection(monkeypatch):
    """max_views splits the set; every camera's projection is posegrad.pose_projection of its own pose and covariance"""
    from uncertainty_nerf_gs_amd import ops, plugin, posegrad, splat
    H, W, B = 6, 8, 5
    seen = []

    def fake(gp, c2ws, fx, fy, cx, cy, H, W, background, projs=None, pose_covs=None, channels=ops.POSE_CHANNELS, want=("proj", "val"),
             **kw):
        seen.append(dict(c2ws=c2ws.clone(), fx=[float(v) for v in fx], projs=projs, want=tuple(want), kw=kw))
        n, Cn = c2ws.shape[0], len(channels)
        P = 12 if projs is None else projs[0].shape[1]
        out = []
        for v in range(n):
            val = torch.full((H, W, Cn), float(fx[v]))
            if Cn == 5:
                val[0, 0, 3] = 0.0                                      # one pixel that blends nothing
            one = {"proj": torch.zeros(H, W, Cn, P), "var": torch.full((H, W, Cn), 4.0), "val": val}
            out.append({k: one[k] for k in want})
        return out

    monkeypatch.setattr(splat, "pose_jacobian_cameras", fake)
    m = plugin.build_model("active-splatfacto", num_points=4)
    c2w = torch.stack([posegrad.perturbed_pose(torch.from_numpy(SPG.frame_c2w()), "angy", 0.02 * v) for v in range(B)])
    cams = _cameras(B, camera_to_worlds=c2w, fx=torch.arange(10.0, 10.0 + B)[:, None])
    covs = [torch.full((6,), 0.01 * (v + 1)) for v in range(B)]
    for mv, groups in ((1, [1] * 5), (2, [2, 2, 1]), (16, [5])):
        del seen[:]
        out = m.get_splat_pose_jacobians_for_cameras(cams, max_views=mv)
        assert [s["c2ws"].shape[0] for s in seen] == groups and len(out) == B
        assert sorted(out[0]) == ["jacobian", "values"] and out[0]["jacobian"].shape == (H, W, 5, 6)
        got = [p for s in seen for p in s["projs"]]
        assert all(torch.equal(got[v], posegrad.pose_projection(c2w[v], None)) for v in range(B))
        assert [f for s in seen for f in s["fx"]] == [10.0 + v for v in range(B)]
        del seen[:]
        unc = m.get_splat_pose_uncertainty_for_cameras(cams, covs, max_views=mv)
        got = [p for s in seen for p in s["projs"]]
        assert all(torch.equal(got[v], posegrad.pose_projection(c2w[v], covs[v])) for v in range(B)) and seen[0]["want"] == ("var", "val")
        for v in range(B):
            fxv = 10.0 + v
            assert float(unc[v]["depth"][0, 0]) == fxv * fxv and float(unc[v]["depth"][1, 1]) == fxv, "each view's OWN fill"
            assert torch.equal(unc[v]["rgb_std_pose"], unc[v]["rgb_var_pose"].sqrt())
        del seen[:]
        m.get_splat_pose_uncertainty_for_cameras(cams, covs[2], max_views=mv)
        got = [p for s in seen for p in s["projs"]]
        assert all(torch.equal(got[v], posegrad.pose_projection(c2w[v], covs[2])) for v in range(B))
    del seen[:]
    m.get_splat_pose_jacobians_for_cameras(cams, basis="c2w", channels=("g", "accumulation"))
    assert seen[0]["projs"] is None


@pytest.mark.parametrize("sheared", [False, True])
def test_batch_projection_matrices_are_the_single_cameras(sheared):
    """splat.pose_view_projections (what pose_jacobian_cameras contracts with) against the statements of pose_jacobian_camera,
    camera by camera: viewmat_jacobian(c2w) @ proj in float64, then float32"""
    from uncertainty_nerf_gs_amd import posegrad, splat
    base = torch.from_numpy(SPG.frame_c2w(sheared))
    c2ws = torch.stack([posegrad.perturbed_pose(base, p, 0.03 * (k + 1)) for k, p in enumerate(posegrad.POSE_PARAMS)] + [base])
    B = c2ws.shape[0]
    cov = (lambda a: a @ a.T * 1e-4)(torch.from_numpy(np.random.default_rng(8).standard_normal((6, 6))))
    rng = np.random.default_rng(5)
    shared = torch.from_numpy(rng.standard_normal((12, 7)))
    each = [torch.from_numpy(rng.standard_normal((12, 3)).astype(np.float32)) for _ in range(B)]

    def single(c2w, proj):                                              # pose_jacobian_camera's own lines
        c2w = c2w.detach().to("cpu", torch.float32)
        M = posegrad.viewmat_jacobian(c2w)
        if proj is not None:
            M = M @ torch.as_tensor(proj).detach().cpu().to(torch.float64)
        return M.to(torch.float32)

    for kw, projs in ((dict(), [None] * B), (dict(projs=shared), [shared] * B), (dict(projs=each), each),
                      (dict(projs=torch.stack(each)), each),
                      (dict(pose_covs=cov), [posegrad.pose_projection(c, cov) for c in c2ws]),
                      (dict(pose_covs=[cov * (v + 1) for v in range(B)]), [posegrad.pose_projection(c2ws[v], cov * (v + 1)) for v in range(B)]),
                      (dict(projs=[posegrad.pose_projection(c) for c in c2ws]), [posegrad.pose_projection(c) for c in c2ws])):
        got = splat.pose_view_projections(c2ws, **kw)
        assert len(got) == B
        for v in range(B):
            want = single(c2ws[v], projs[v])
            assert got[v][1].dtype == torch.float32 and torch.equal(got[v][1], want), (sorted(kw), v)
            assert torch.equal(posegrad.splat_view_projection(c2ws[v], projs[v]), want)
    with pytest.raises(ValueError, match="2 projs for 7 cameras"):
        splat.pose_view_projections(c2ws, projs=each[:2])
    with pytest.raises(ValueError, match="not both"):
        splat.pose_view_projections(c2ws, projs=shared, pose_covs=cov)
    from uncertainty_nerf_gs_amd import lib
    with pytest.raises(lib.UnerfError, match=r"proj must be \[12,P\]"):
        splat.pose_view_projections(c2ws, projs=torch.zeros(12, 13))
