"""Several camera views per NeRF render call, the parts that need no GPU: the C ABI surface (struct layout, refusals
before any launch), the launch plan of render.render_cameras as a pure function, and the eval harness' view_batch over a
fake model on CPU tensors."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT

VIEWS_SYMBOLS = ("unerf_generate_rays_views", "unerf_weights_pdf_resample_views", "unerf_composite_var_views",
                 "unerf_composite_moments_views", "unerf_field_fwd_views")


def test_view_table_symbols_and_struct_layout(lib, tmp_path):
    h = lib.load()
    for name in VIEWS_SYMBOLS:
        assert name in lib.SIGNATURES and getattr(h, name) is not None
    # sizeof / offsetof as a C compiler sees include/unerf.h (the method of test_keep_mask_symbols_and_struct_layout)
    structs = {"unerf_ray_views": lib.RayViews, "unerf_ray_camera": lib.RayCamera}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "unerf.h"', 'int main(void) {',
             '  printf("MAX_VIEWS x %d\\n", UNERF_NERF_MAX_VIEWS);']
    for cname, ct in structs.items():
        lines.append(f'  printf("{cname} SIZEOF %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));' for f, _ in ct._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    rows = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    assert len(rows) == 1 + sum(len(ct._fields_) + 1 for ct in structs.values())
    for row in rows:
        cname, what, val = row.split()
        if cname == "MAX_VIEWS":
            assert int(val) == lib.NERF_MAX_VIEWS == 16
            continue
        ct = structs[cname]
        assert (C.sizeof(ct) if what == "SIZEOF" else getattr(ct, what).offset) == int(val), row
    assert C.sizeof(lib.RayViews) == 80 and lib.RayViews.seed.size == 64 and C.sizeof(lib.RayCamera) == 88
    assert h.unerf_version() == lib.ABI_VERSION == 1420        # additive: same ABI version


def _views(lib, n=3, per=1073, seeds=()):
    v = lib.RayViews()
    v.n_views, v.rays_per_view = n, per
    for i, s in enumerate(seeds):
        v.seed[i] = s
    return v


def _params(lib, **kw):
    fp = lib.FieldParams()
    for name in ("table", "scalings", "w0t", "b0", "w1t", "b1", "h0t", "hb0", "h1t", "hb1", "h2t", "hb2", "mfma16_blob", "mfma_blob"):
        setattr(fp, name, 1)
    fp.L, fp.log2T, fp.mode, fp.out1, fp.K, fp.p_drop, fp.packed_out = 16, 19, lib.FIELD_MCDROPOUT, 16, 3, 0.2, 1
    for k, v in kw.items():
        setattr(fp, k, v)
    return fp


BAD_TABLES = [(0, 1073, 0, b"n_views=0"), (17, 1073, 17 * 1073, b"n_views=17"), (3, 0, 0, b"rays_per_view=0"),
              (3, -5, -15, b"rays_per_view=-5"), (3, 1073, 3 * 1073 + 1, b"is not n_views x rays_per_view")]


def test_views_entry_points_refuse_bad_view_tables_before_any_launch(lib):
    """0 and 17 views, rays per view <= 0, R != views x rays per view: -1 and a message from each of the four kernels' entry
    points -- on a machine without a GPU, so nothing was launched"""
    h = lib.load()
    fp = _params(lib)
    for n, per, R, text in BAD_TABLES:
        v = _views(lib, n, per)
        calls = {
            "pdf": lambda: h.unerf_weights_pdf_resample_views(1, 1, 0, R, 96, 0.05, 1000.0, 0, 1, 48, 0.01, 1e-5, 1, None, None, 1,
                                                              C.byref(v), 512, None),
            "var": lambda: h.unerf_composite_var_views(None, 1, None, None, 1, 1, R, 48, 0.05, 1000.0, 0, 1, C.byref(v), 512, 0, None,
                                                       None, 1, None),
            "moments": lambda: h.unerf_composite_moments_views(None, 1, 1, 3, R, 48, 0.05, 1000.0, 0, 1, C.byref(v), 512, 0, None,
                                                               None, 1, 1, None),
            "field": lambda: h.unerf_field_fwd_views(1, 1, 1, R, 48, 0.05, 1000.0, 0, C.byref(v), C.byref(fp), None, None, 1, None,
                                                     None, None, None),
        }
        for name, call in calls.items():
            assert call() == -1, (name, n, per, R)
            assert text in h.unerf_last_error(), (name, h.unerf_last_error())
    # a NULL table is refused too; the ray generator counts its views itself
    assert h.unerf_composite_var_views(None, 1, None, None, 1, 1, 10, 48, 0.05, 1000.0, 0, 1, None, 512, 0, None, None, 1, None) == -1
    assert b"null views" in h.unerf_last_error()
    cams = (lib.RayCamera * 17)()
    for n in (0, 17):
        assert h.unerf_generate_rays_views(cams, n, 1, 4, 4, 1, 1, None, None) == -1
        assert b"n_views" in h.unerf_last_error()
    assert h.unerf_generate_rays_views(cams, 2, 5, 4, 4, 1, 1, None, None) == -1 and b"camera_type" in h.unerf_last_error()
    cams[1].distortion[2] = float("nan")
    assert h.unerf_generate_rays_views(cams, 2, 1, 4, 4, 1, 1, None, None) == -1
    assert b"distortion[2] of view 1" in h.unerf_last_error()


def test_field_fwd_views_refuses_what_is_not_built_before_any_launch(lib):
    """LAPLACE, the exact-fp32 / VALU kernels (no mfma16_blob), the any-width kernel, sample-major planes, pre-gathered
    features, other dropout sites and explicit keep masks: each -1 with a message that says so, never another kernel"""
    h = lib.load()
    R = 3 * 1073
    v = _views(lib, seeds=(1, 2, 3))

    def refused(fp, text, masks=None, features=None):
        rc = h.unerf_field_fwd_views(1, 1, 1, R, 48, 0.05, 1000.0, 0, C.byref(v), C.byref(fp), features, None, 1, None, None,
                                     None if masks is None else C.byref(masks), None)
        assert rc == -1
        assert text in h.unerf_last_error(), h.unerf_last_error()

    refused(_params(lib, mode=lib.FIELD_LAPLACE, out1=15), b"LAPLACE renders one frame per call")
    refused(_params(lib, mfma16_blob=None), b"exact-fp32 and VALU kernels render one frame per call")
    refused(_params(lib, mfma16_blob=None, mfma_blob=None), b"exact-fp32 and VALU kernels render one frame per call")
    refused(_params(lib, hidden=32, hidden_color=64, geo_dim=15, feat_per_level=2, app_dim=32), b"any-width kernel is not built")
    refused(_params(lib, sample_major=1), b"sample_major planes are not built")
    refused(_params(lib), b"pre-gathered features are not built", features=1)
    refused(_params(lib, drop_sites=7), b"drop_sites=7 is not built")
    km = lib.KeepMasks()
    km.site[0], km.site[2], km.pass_stride = 1, 1, R * 48
    refused(_params(lib), b"explicit keep masks have no views form", masks=km)
    # the limits of the single-view call still hold: 32-bit sample counter
    big = _views(lib, 16, 1 << 23)
    fp = _params(lib)
    assert h.unerf_field_fwd_views(1, 1, 1, 16 << 23, 48, 0.05, 1000.0, 0, C.byref(big), C.byref(fp), None, None, 1, None, None,
                                   None, None) == -1
    assert b"32 bits" in h.unerf_last_error()


def test_launch_plan_is_a_pure_function_of_the_sizes():
    from uncertainty_nerf_gs_amd import render
    # 3 views of 29 x 37 = 1,073 rays, launch groups of 2,560 rays, chunks of 512: two views fit, the third goes alone
    assert render.plan_view_groups(3, 1073, rays_per_launch=2560, chunk_rays=512) == [(0, 2), (2, 1)]
    # 16 views of 48 x 64 = 3,072 rays with the defaults: one group
    assert render.plan_view_groups(16, 3072) == [(0, 16)]
    # never more than the view table holds, whatever fits
    assert render.plan_view_groups(40, 100) == [(0, 16), (16, 16), (32, 8)]
    assert render.plan_view_groups(5, 100, max_views=2) == [(0, 2), (2, 2), (4, 1)]
    # a view larger than half a launch group shares nothing: the per-camera loop
    assert render.plan_view_groups(4, (1 << 19) + 1) is None
    assert render.plan_view_groups(4, 1 << 19) == [(0, 2), (2, 2)]
    assert render.plan_view_groups(3, 1281, rays_per_launch=2560, chunk_rays=512) is None
    # rays_per_launch is rounded down to whole chunks first, as render_camera does
    assert render.plan_view_groups(4, 1000, rays_per_launch=2100, chunk_rays=1000) == [(0, 2), (2, 2)]
    with pytest.raises(ValueError):
        render.plan_view_groups(0, 100)


def test_clip_rows_and_view_table_of_the_ops_layer(lib):
    from uncertainty_nerf_gs_amd import ops
    assert ops.clip_rows_per_view(1073, 512) == 3 and ops.clip_rows_per_view(1024, 512) == 2
    cs = ops.RayViews(3, 1073, (5, 1 << 32 | 7, 9)).cstruct()
    assert (cs.n_views, cs.rays_per_view, list(cs.seed)[:4]) == (3, 1073, [5, 7, 9, 0])
    assert list(ops.RayViews(2, 10).cstruct(default_seed=42).seed)[:3] == [42, 42, 0]
    with pytest.raises(lib.UnerfError, match="seeds"):
        ops.RayViews(3, 10, (1, 2)).cstruct()


class _FakeModel:
    """renders a camera as an image that depends on the camera alone; records how it was called"""

    def __init__(self):
        self.single_calls, self.batch_calls = 0, []

    @staticmethod
    def _render(c2w, H, W):
        g = torch.Generator().manual_seed(int(c2w[0, 3].item() * 1000))
        return {"rgb": torch.rand(H, W, 3, generator=g), "rgb_std": torch.rand(H, W, 1, generator=g) * 0.2 + 0.01}

    def get_outputs_for_camera(self, camera):
        self.single_calls += 1
        return self._render(camera.camera_to_worlds, camera.height, camera.width)

    def get_outputs_for_cameras(self, cameras, obb_box=None):
        B = cameras.camera_to_worlds.shape[0]
        self.batch_calls.append((B, cameras.height, cameras.width, [float(v) for v in cameras.fx]))
        return [self._render(cameras.camera_to_worlds[v], cameras.height, cameras.width) for v in range(B)]


def _eval_set(sizes):
    out = []
    for i, (H, W) in enumerate(sizes):
        c2w = torch.eye(4)[:3].clone()
        c2w[0, 3] = 0.1 * (i + 1)
        cam = SimpleNamespace(camera_to_worlds=c2w, fx=10.0 + i, fy=11.0, cx=W / 2, cy=H / 2, height=H, width=W)
        out.append((cam, torch.rand(H, W, 3, generator=torch.Generator().manual_seed(5000 + i))))
    return out


TIMING_KEYS = ("num_rays_per_sec", "fps", "render_rays_per_sec")


def test_eval_view_batch_calls_the_batch_method_and_returns_the_loops_metrics():
    from uncertainty_nerf_gs_amd import eval as E
    es = _eval_set([(12, 16)] * 6)
    loop_model, batch_model = _FakeModel(), _FakeModel()
    want, want_curves = E.get_average_uncertainty_metrics(loop_model.get_outputs_for_camera, es)
    got, got_curves = E.get_average_uncertainty_metrics(batch_model.get_outputs_for_camera, es, view_batch=4)
    assert loop_model.single_calls == 6 and loop_model.batch_calls == []
    assert batch_model.single_calls == 0 and [c[0] for c in batch_model.batch_calls] == [4, 2]
    assert batch_model.batch_calls[0][3] == [10.0, 11.0, 12.0, 13.0] and batch_model.batch_calls[1][3] == [14.0, 15.0]
    assert set(got) == set(want) and set(TIMING_KEYS) <= set(got)
    for k in want:
        if k not in TIMING_KEYS:
            assert got[k] == want[k], k
    for k in want_curves:
        assert (got_curves[k] == want_curves[k]).all(), k
    # the default is the per-camera loop, and the batch method can be handed over explicitly
    other = _FakeModel()
    E.get_average_uncertainty_metrics(lambda cam: other.get_outputs_for_camera(cam), es, view_batch=3,
                                      get_outputs_for_cameras=other.get_outputs_for_cameras)
    assert [c[0] for c in other.batch_calls] == [3, 3]
    with pytest.raises(ValueError, match="get_outputs_for_cameras"):
        E.get_average_uncertainty_metrics(lambda cam: other.get_outputs_for_camera(cam), es, view_batch=2)


def test_eval_view_batch_batches_two_image_sizes_separately():
    from uncertainty_nerf_gs_amd import eval as E
    es = _eval_set([(12, 16)] * 3 + [(14, 12)] * 5 + [(12, 16)])
    loop_model, batch_model = _FakeModel(), _FakeModel()
    want, _ = E.get_average_uncertainty_metrics(loop_model.get_outputs_for_camera, es)
    got, _ = E.get_average_uncertainty_metrics(batch_model.get_outputs_for_camera, es, view_batch=4)
    assert [(c[0], c[1], c[2]) for c in batch_model.batch_calls] == [(3, 12, 16), (4, 14, 12), (1, 14, 12), (1, 12, 16)]
    for k in want:
        if k not in TIMING_KEYS:
            assert got[k] == want[k], k


def test_models_and_plugin_expose_the_batch_method():
    from uncertainty_nerf_gs_amd import models
    for cls in (models.NerfactoModel, models.ActiveNerfactoModel, models.NerfactoMCDropoutModel, models.NerfactoLaplaceModel):
        assert callable(getattr(cls, "get_outputs_for_cameras"))
    cams = SimpleNamespace(camera_to_worlds=torch.eye(4)[None, :3].repeat(3, 1, 1), fx=10.0, fy=10.0, cx=8.0, cy=6.0,
                           height=torch.tensor([12, 12, 16]), width=16)
    with pytest.raises(ValueError, match="one image size"):
        models._camera_batch(cams)
    cams.height = 12
    cams.distortion_params = torch.tensor([[0.0] * 6, [0.1, 0, 0, 0, 0, 0], [0.0] * 6])
    c2w, H, W, singles = models._camera_batch(cams)
    assert c2w.shape == (3, 3, 4) and (H, W) == (12, 16) and len(singles) == 3
    args = [models._camera_args(s)[1] for s in singles]
    assert "distortion" not in args[0] and args[1]["distortion"][0] == pytest.approx(0.1) and args[2]["fx"] == 10.0
