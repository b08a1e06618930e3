"""Several camera views per Laplace render call, the parts that need no GPU: the C ABI surface (struct layout, every refusal
before any launch), and the order in which the last-layer sample sets of a batch of cameras consume the generator."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from conftest import ROOT

HW, S = 1073, 48


def test_laplace_view_symbols_and_struct_layout(lib, tmp_path):
    h = lib.load()
    for name in ("unerf_field_fwd_laplace_views", "unerf_laplace_depth_weights_views"):
        assert name in lib.SIGNATURES and getattr(h, name) is not None
        assert getattr(h, name).restype is C.c_int and len(getattr(h, name).argtypes) == len(lib.SIGNATURES[name][1])
    # sizeof / offsetof as a C compiler sees include/unerf.h (the method of test_view_table_symbols_and_struct_layout)
    structs = {"unerf_laplace_views": lib.LaplaceViews, "unerf_ray_views": lib.RayViews}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "unerf.h"', 'int main(void) {']
    for cname, ct in structs.items():
        lines.append(f'  printf("{cname} SIZEOF %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));' for f, _ in ct._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    rows = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    assert len(rows) == sum(len(ct._fields_) + 1 for ct in structs.values())
    for row in rows:
        cname, what, val = row.split()
        ct = structs[cname]
        assert (C.sizeof(ct) if what == "SIZEOF" else getattr(ct, what).offset) == int(val), row
    assert C.sizeof(lib.LaplaceViews) == 128 and lib.LaplaceViews.depth_seed.offset == 64 and C.sizeof(lib.RayViews) == 80
    assert h.unerf_version() == lib.ABI_VERSION == 1420        # additive: same ABI version


def _views(lib, n=3, per=HW):
    v = lib.RayViews()
    v.n_views, v.rays_per_view = n, per
    return v


def _lap(lib, set_base=(0, 0, 0), seeds=()):
    lv = lib.LaplaceViews()
    for i, b in enumerate(set_base):
        lv.set_base[i] = b
    for i, s in enumerate(seeds):
        lv.depth_seed[i] = s
    return lv


def _params(lib, **kw):
    fp = lib.FieldParams()
    for name in ("table", "scalings", "w0t", "b0", "w1t", "b1", "h0t", "hb0", "h1t", "hb1", "h2t", "hb2", "mfma16_blob", "mfma_blob",
                 "lap16_blob", "lap_blob", "ws_density", "ws_rgb"):
        setattr(fp, name, 1)
    fp.L, fp.log2T, fp.mode, fp.out1, fp.n_lap, fp.n_lap_rgb = 16, 19, lib.FIELD_LAPLACE, 15, 30, 30
    fp.lap_chunk_rays, fp.lap_sets = 512, 9
    for k, v in kw.items():
        setattr(fp, k, v)
    return fp


def _field_call(h, lib, fp, views=None, lap="default", R=3 * HW, s=S):
    views = _views(lib) if views is None else views
    lap = _lap(lib) if lap == "default" else lap
    return h.unerf_field_fwd_laplace_views(1, 1, 1, R, s, 0.05, 1000.0, 0, None if views is False else C.byref(views),
                                           None if lap is None else C.byref(lap), C.byref(fp), 1, 1, 1, 1, None)


def test_both_entry_points_refuse_bad_view_tables_before_any_launch(lib):
    h = lib.load()
    fp = _params(lib)
    for n, per, R, text in [(0, HW, 0, b"n_views=0"), (17, HW, 17 * HW, b"n_views=17"), (3, 0, 0, b"rays_per_view=0"),
                            (3, -5, -15, b"rays_per_view=-5"), (3, HW, 3 * HW + 1, b"is not n_views x rays_per_view")]:
        v, lv = _views(lib, n, per), _lap(lib)
        assert _field_call(h, lib, fp, views=v, R=R) == -1 and text in h.unerf_last_error(), h.unerf_last_error()
        assert h.unerf_laplace_depth_weights_views(1, 1, 1, R, S, 0.05, 1000.0, 0, None, 100, C.byref(v), C.byref(lv), 1, None) == -1
        assert text in h.unerf_last_error(), h.unerf_last_error()
    assert _field_call(h, lib, fp, views=False) == -1 and b"null views" in h.unerf_last_error()
    assert h.unerf_laplace_depth_weights_views(1, 1, 1, 3 * HW, S, 0.05, 1000.0, 0, None, 100, None, C.byref(_lap(lib)), 1, None) == -1
    assert b"null views" in h.unerf_last_error()
    # a null per-view table, and the single call's limits on D and S
    v = _views(lib)
    assert _field_call(h, lib, fp, lap=None) == -1 and b"null lap_views" in h.unerf_last_error()
    assert h.unerf_laplace_depth_weights_views(1, 1, 1, 3 * HW, S, 0.05, 1000.0, 0, None, 100, C.byref(v), None, 1, None) == -1
    assert b"null lap_views" in h.unerf_last_error()
    for D, s in ((0, S), (100, 0), (100, 257)):
        assert h.unerf_laplace_depth_weights_views(1, 1, 1, 3 * HW, s, 0.05, 1000.0, 0, None, D, C.byref(v), C.byref(_lap(lib)), 1, None) == -1
        assert b"bad D/S" in h.unerf_last_error()
    assert h.unerf_laplace_depth_weights_views(None, 1, 1, 3 * HW, S, 0.05, 1000.0, 0, None, 100, C.byref(v), C.byref(_lap(lib)), 1, None) == -1
    assert b"null pointer" in h.unerf_last_error()


def test_field_fwd_laplace_views_refuses_what_is_not_built_before_any_launch(lib):
    """every refusal of the entry point: -1 and a message that names the reason, on a machine where nothing can launch"""
    h = lib.load()

    def refused(fp, text, **kw):
        assert _field_call(h, lib, fp, **kw) == -1
        assert text in h.unerf_last_error(), h.unerf_last_error()

    refused(_params(lib, mode=lib.FIELD_ACTIVE, out1=17), b"is not LAPLACE")
    refused(_params(lib, mode=lib.FIELD_MCDROPOUT, out1=16), b"is not LAPLACE")
    refused(_params(lib, mfma16_blob=None), b"exact-fp32 and VALU kernels render one frame per call")
    refused(_params(lib, lap16_blob=None), b"exact-fp32 and VALU kernels render one frame per call")
    refused(_params(lib, hidden=32, hidden_color=64, geo_dim=15, feat_per_level=2, app_dim=32), b"any-width kernel is not built")
    refused(_params(lib, sample_major=1), b"sample_major planes are not built")
    refused(_params(lib, lap_chunk_rays=-512), b"lap_chunk_rays=-512 must be 0 or a positive multiple of 32")
    refused(_params(lib, lap_chunk_rays=500), b"lap_chunk_rays=500 must be 0 or a positive multiple of 32")
    refused(_params(lib), b"set_base[1]=-1 is negative", lap=_lap(lib, (0, -1, 0)))
    # three sets per view (1,073 rays of 512): base 6 is the last that fits nine sets
    assert h.unerf_last_error() and _field_call(h, lib, _params(lib, table=None), lap=_lap(lib, (3, 0, 6))) == -1
    assert b"null weight pointer" in h.unerf_last_error()          # (got past the set checks)
    refused(_params(lib), b"set_base[2] + sets per view > lap_sets", lap=_lap(lib, (3, 0, 7)))
    refused(_params(lib, lap_sets=2), b"set_base[0] + sets per view > lap_sets")
    # one set per view: the base itself must exist (lap_sets = 0 counts as one set)
    refused(_params(lib, lap_chunk_rays=0), b"set_base[1] + sets per view > lap_sets", lap=_lap(lib, (8, 9, 0)))
    refused(_params(lib, lap_chunk_rays=0, lap_sets=0), b"set_base[2] + sets per view > lap_sets", lap=_lap(lib, (0, 0, 1)))
    assert _field_call(h, lib, _params(lib, lap_chunk_rays=0, table=None), lap=_lap(lib, (8, 0, 5))) == -1
    assert b"null weight pointer" in h.unerf_last_error()
    # 32-bit sample counter inside a view
    big = _views(lib, 2, 1 << 26)
    refused(_params(lib, lap_chunk_rays=0), b"sample index of a view exceeds 32 bits", views=big, R=2 << 26, s=64)
    # more sampled rows than the head blobs hold
    refused(_params(lib, n_lap=129, n_lap_rgb=129), b"n_lap=129 rows do not fit the head blobs")
    # unerf_field_fwd_views still refuses LAPLACE, and says where it went
    rc = h.unerf_field_fwd_views(1, 1, 1, 3 * HW, S, 0.05, 1000.0, 0, C.byref(_views(lib)), C.byref(_params(lib)), None, None, 1,
                                 None, None, None, None)
    assert rc == -1 and b"LAPLACE renders one frame per call" in h.unerf_last_error()
    assert b"unerf_field_fwd_laplace_views" in h.unerf_last_error()


def test_ops_layer_tables_and_refusals(lib):
    from uncertainty_nerf_gs_amd import ops
    cs = ops.LaplaceViews((3, 0, 6), (3, 3, 1 << 32 | 900001)).cstruct(3)
    assert list(cs.set_base)[:4] == [3, 0, 6, 0] and list(cs.depth_seed)[:4] == [3, 3, 900001, 0]
    cs = ops.LaplaceViews().cstruct(2, default_seed=11)
    assert list(cs.set_base)[:3] == [0, 0, 0] and list(cs.depth_seed)[:3] == [11, 11, 0]
    with pytest.raises(lib.UnerfError, match="set_base"):
        ops.LaplaceViews((1, 2)).cstruct(3)
    with pytest.raises(lib.UnerfError, match="depth_seeds"):
        ops.LaplaceViews(None, (1, 2, 3, 4)).cstruct(3)
    # pre-gathered features have no several-views form: refused where a caller can pass them
    f = ops.FieldDev(lib.FIELD_LAPLACE, *([torch.zeros(1)] * 2), 14, *([torch.zeros(1)] * 10))
    z = torch.zeros(4, 3)
    with pytest.raises(lib.UnerfError, match="pre-gathered features"):
        ops.field_fwd(z, z, torch.zeros(4, 49), f, 0.05, 1000.0, views=ops.RayViews(1, 4), features=torch.zeros(1))
    f.mode = lib.FIELD_ACTIVE
    with pytest.raises(lib.UnerfError, match="lap_views goes with views= and a LAPLACE field"):
        ops.field_fwd(z, z, torch.zeros(4, 49), f, 0.05, 1000.0, lap_views=ops.LaplaceViews())


def test_sets_of_a_batch_consume_the_generator_as_successive_cameras_do():
    """fields.sample_last_layers draws set by set, density then colour: the sets of B cameras in one call are the
    concatenation of B per-camera calls, and the generators end in the same state"""
    from uncertainty_nerf_gs_amd import fields as F
    field = F.NerfactoLaplaceField(num_images=2, log2_hashmap_size=8, max_res=64)
    g = torch.Generator().manual_seed(3)
    field.mlp_density_ggn = torch.rand(field.mlp_density_ggn.shape, generator=g) * 100
    field.mlp_rgb_ggn = torch.rand(field.mlp_rgb_ggn.shape, generator=g) * 100
    for kw in (dict(), dict(deterministic_density=True), dict(n_samples=30)):
        # three cameras of two chunks each
        g1, g2 = torch.Generator().manual_seed(77), torch.Generator().manual_seed(77)
        d, c = field.sample_last_layers(n_sets=3 * 2, generator=g1, **kw)
        parts = [field.sample_last_layers(n_sets=2, generator=g2, **kw) for _ in range(3)]
        assert d.shape[0] == c.shape[0] == 6 and c.shape[1] == 100 and d.shape[1] == (100 if kw.get("deterministic_density") else kw.get("n_samples", 100))
        assert torch.equal(d, torch.cat([p[0] for p in parts])) and torch.equal(c, torch.cat([p[1] for p in parts]))
        assert torch.equal(g1.get_state(), g2.get_state())
        # three cameras of one set each (resample = "camera"): against three calls without n_sets
        g1, g2 = torch.Generator().manual_seed(78), torch.Generator().manual_seed(78)
        d, c = field.sample_last_layers(n_sets=3, generator=g1, **kw)
        parts = [field.sample_last_layers(generator=g2, **kw) for _ in range(3)]
        assert torch.equal(d, torch.stack([p[0] for p in parts])) and torch.equal(c, torch.stack([p[1] for p in parts]))
        assert torch.equal(g1.get_state(), g2.get_state())
        if not kw.get("deterministic_density"):
            assert not torch.equal(d[0], d[1])
