"""Batched splat entry points (include/unerf.h, "splats, B views per call") and SplatfactoModel.get_outputs_for_cameras
without a GPU: every argument check answers UNERF_ERR_ARG with a message before anything is launched."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch


def _views(lib, B):
    return (C.c_float * (B * lib.SPLAT_VIEW_FLOATS))()


def test_batch_constants_match_the_header(lib):
    import os
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "unerf.h")).read()
    assert f"#define UNERF_SPLAT_MAX_VIEWS {lib.SPLAT_MAX_VIEWS}" in text
    assert f"#define UNERF_SPLAT_VIEW_FLOATS {lib.SPLAT_VIEW_FLOATS}" in text


def test_project_and_shade_batch_argument_checks(lib):
    h = lib.load()
    v = _views(lib, 17)
    rc = h.unerf_splat_project_batch(1, 1, 1.0, 1, None, 2, 16, 16, 16, 0.01, 10, None, 0, None, 1, 1, 1, 1, 1, 1, None, None)
    assert rc == -1 and b"views_host" in h.unerf_last_error()
    for B in (0, 17):
        rc = h.unerf_splat_project_batch(1, 1, 1.0, 1, v, B, 16, 16, 16, 0.01, 10, None, 0, None, 1, 1, 1, 1, 1, 1, None, None)
        assert rc == -1 and f"B={B}".encode() in h.unerf_last_error()
    rc = h.unerf_splat_project_batch(1, 1, 1.0, 1, v, 2, 16, 16, 16, 0.01, 10, None, 0, None, None, 1, 1, 1, 1, 1, None, None)
    assert rc == -1 and b"null pointer" in h.unerf_last_error()
    rc = h.unerf_splat_project_batch(1, 1, 1.0, 1, v, 16, 16, 16, 16, 0.01, 1 << 26, None, 0, None, 1, 1, 1, 1, 1, 1, None, None)
    assert rc == -1 and b"B*N" in h.unerf_last_error()
    # N = 0: a no-op (per-element pointers may be NULL), as the header's conventions say
    assert h.unerf_splat_project_batch(None, None, 1.0, None, v, 3, 16, 16, 16, 0.01, 0, None, 0, None, None, None, None, None,
                                       None, None, None, None) == 0
    rc = h.unerf_splat_shade_inputs_batch(3, 1, v, 0, 1, 1, 1, 0.01, None, None, 1, 4, 5, 1, None, None)
    assert rc == -1 and b"B=0" in h.unerf_last_error()
    rc = h.unerf_splat_shade_inputs_batch(3, 1, v, 2, 1, None, 1, 0.01, None, None, 1, 4, 5, 1, None, None)
    assert rc == -1 and b"needs features_rest" in h.unerf_last_error()
    rc = h.unerf_splat_shade_inputs_batch(3, 1, None, 2, 1, 1, 1, 0.01, None, None, 1, 4, 5, 1, None, None)
    assert rc == -1 and b"views_host" in h.unerf_last_error()
    assert h.unerf_splat_shade_inputs_batch(3, None, v, 2, None, None, None, 0.01, None, None, None, 0, 5, None, None, None) == 0


def test_count_and_sort_batch_argument_checks(lib):
    h = lib.load()
    rc = h.unerf_splat_count_intersects_batch(1, None, 2, 10, 1, None, 1, 1 << 20, None)
    assert rc == -1 and b"null pointer" in h.unerf_last_error()
    rc = h.unerf_splat_count_intersects_batch(1, None, 17, 10, 1, 1, 1, 1 << 20, None)
    assert rc == -1 and b"B=17" in h.unerf_last_error()
    rc = h.unerf_splat_count_intersects_batch(1, None, 2, 10, 1, 1, 1, 0, None)
    assert rc == -1 and b"too small" in h.unerf_last_error()
    assert h.unerf_splat_sort_workspace_bytes_batch(0, 10, 0) == -1
    assert h.unerf_splat_sort_workspace_bytes_batch(17, 10, 0) == -1
    assert h.unerf_splat_sort_workspace_bytes_batch(2, 10, 1 << 31) == -1
    assert h.unerf_splat_sort_workspace_bytes_batch(4, 1000, 5000) > h.unerf_splat_sort_workspace_bytes(1000, 5000)
    ok = (C.c_int64 * 3)(10, 20, 30)
    args = lambda B, isects, H=64, W=64: (1, 1, 1, 1, B, 100, isects, H, W, 16, None, None, 1, 1, 1, 1 << 30, None)
    rc = h.unerf_splat_bin_sort_batch(*args(3, None))
    assert rc == -1 and b"null pointer" in h.unerf_last_error()
    rc = h.unerf_splat_bin_sort_batch(*args(0, ok))
    assert rc == -1 and b"B=0" in h.unerf_last_error()
    rc = h.unerf_splat_bin_sort_batch(*args(17, ok))
    assert rc == -1 and b"B=17" in h.unerf_last_error()
    # every view below 2^31, their sum above: the batch's ids and bins are int32
    over = (C.c_int64 * 3)(1 << 30, 1 << 30, 5)
    rc = h.unerf_splat_bin_sort_batch(*args(3, over))
    assert rc == -1 and b"over the batch" in h.unerf_last_error()
    neg = (C.c_int64 * 3)(10, -1, 30)
    rc = h.unerf_splat_bin_sort_batch(*args(3, neg))
    assert rc == -1 and b"view 1" in h.unerf_last_error()
    rc = h.unerf_splat_bin_sort_batch(*args(3, ok, H=2160, W=3840))
    assert rc == -1 and b"tiles" in h.unerf_last_error()
    # UNERF_SPLAT_BATCH_MAX_TILES = 11,999: one tile more is refused by name, the limit itself gets past this check
    rc = h.unerf_splat_bin_sort_batch(*args(3, ok, H=16, W=16 * 12000))
    assert rc == -1 and b"12000 tiles" in h.unerf_last_error() and b"up to 11999" in h.unerf_last_error()
    rc = h.unerf_splat_bin_sort_batch(1, 1, 1, 1, 3, 100, ok, 16, 16 * 11999, 16, None, None, 1, 1, 1, 0, None)
    msg = h.unerf_last_error()      # (the size refusal itself, not the "tile tables ... workspace layout" one in front of it)
    assert rc == -1 and b"workspace 0 <" in msg and b"unerf_splat_sort_workspace_bytes_batch" in msg, msg
    rc = h.unerf_splat_bin_sort_batch(1, 1, 1, 1, 3, 100, ok, 64, 64, 16, 1, None, 1, 1, 1, 1 << 30, None)
    assert rc == -1 and b"tight lists" in h.unerf_last_error()


def test_batch_workspace_covers_the_padded_tile_tables_at_one_view(lib):
    """The batch pads each view's tile-sort chunks to whole histogram workgroups (16 chunks), B = 1 included; the size query
    must reserve that even where the two-pass tables outgrow the one-pass ones (~12,000 tiles, 30 M pairs).  The batch entry
    point checks its chunk plan against the layout before the workspace size, so a too-small workspace must be what it
    reports -- never its tile tables."""
    h = lib.load()
    for B, isects, tiles_x in ((1, [30_000_000], 11999), (1, [25_000_001], 11999), (2, [15_000_000, 15_000_001], 11998),
                               (3, [1, 2049, 0], 11999)):
        ws = h.unerf_splat_sort_workspace_bytes_batch(B, 100, sum(isects))
        assert ws > 0
        arr = (C.c_int64 * B)(*isects)
        rc = h.unerf_splat_bin_sort_batch(1, 1, 1, 1, B, 100, arr, 16, 16 * tiles_x, 16, None, None, 1, 1, 1, ws - 1, None)
        msg = h.unerf_last_error()
        assert rc == -1 and b"workspace" in msg and b"tile tables" not in msg, (B, isects, msg)


def test_raster_and_epilogue_batch_argument_checks(lib):
    h = lib.load()
    rc = h.unerf_splat_rasterize_batch(1, 1, 1, 1, 1, 1, None, 0, 5, 16, 16, 16, None, 0, -1, None, 1, 1, None, None)
    assert rc == -1 and b"B=0" in h.unerf_last_error()
    rc = h.unerf_splat_rasterize_batch(1, 1, 1, 1, 1, 1, None, 17, 5, 16, 16, 16, None, 0, -1, None, 1, 1, None, None)
    assert rc == -1 and b"B=17" in h.unerf_last_error()
    rc = h.unerf_splat_rasterize_batch(1, None, 1, 1, 1, 1, None, 2, 5, 16, 16, 16, None, 0, -1, None, 1, 1, None, None)
    assert rc == -1 and b"null pointer" in h.unerf_last_error()
    rc = h.unerf_splat_rasterize_batch(1, 1, 1, 1, 1, 1, None, 2, 9, 16, 16, 16, None, 0, -1, None, 1, 1, None, None)
    assert rc == -1 and b"C=9" in h.unerf_last_error()
    rc = h.unerf_splat_normalize_outputs_batch(None, 5, 4, 1, 2, 256, 1, None, None, -1, None, None, None)
    assert rc == -1 and b"null pointer" in h.unerf_last_error()
    rc = h.unerf_splat_normalize_outputs_batch(1, 5, 4, 1, 17, 256, 1, None, None, -1, None, None, None)
    assert rc == -1 and b"B=17" in h.unerf_last_error()
    assert h.unerf_splat_normalize_outputs_batch(1, 5, 4, 1, 2, 0, 1, None, None, -1, None, None, None) == 0
    rc = h.unerf_splat_depth_sqdiff_batch(None, 1, 1, 5, 4, 2, 16, 16, 10, 1, None)
    assert rc == -1 and b"null pointer" in h.unerf_last_error()
    rc = h.unerf_splat_depth_sqdiff_batch(1, 1, 1, 5, 4, 0, 16, 16, 10, 1, None)
    assert rc == -1 and b"B=0" in h.unerf_last_error()
    assert h.unerf_splat_depth_sqdiff_batch(None, None, None, 5, 4, 2, 16, 16, 0, None, None) == 0


def _model():
    from uncertainty_nerf_gs_amd import models
    return models.ActiveSplatfactoModel(models.ActiveSplatfactoModelConfig(), num_points=7)


def _cams(B=3, **kw):
    c = dict(camera_to_worlds=torch.eye(4)[:3].expand(B, 3, 4).clone(), fx=torch.full((B,), 50.0), fy=50.0, cx=16.0, cy=12.0,
             height=24, width=32)
    c.update(kw)
    return SimpleNamespace(**c)


def test_get_outputs_for_cameras_refuses_mixed_sizes_and_other_camera_types(lib):
    m = _model()
    with pytest.raises(ValueError, match="one image size per batch"):
        m.get_outputs_for_cameras(_cams(height=torch.tensor([24, 24, 48])))
    with pytest.raises(ValueError, match="one image size per batch"):
        m.get_outputs_for_cameras(_cams(width=torch.tensor([[32], [64], [32]])))
    with pytest.raises(NotImplementedError, match="camera_type 2"):
        m.get_outputs_for_cameras(_cams(camera_type=torch.tensor([1, 2, 1])))
    with pytest.raises(NotImplementedError, match="PERSPECTIVE"):
        m.get_outputs_for_cameras(_cams(camera_type=8))
    with pytest.raises(ValueError, match="max_views"):
        m.get_outputs_for_cameras(_cams(), max_views=17)
    # the single-camera entry keeps refusing batches exactly as before
    with pytest.raises(ValueError, match="takes one camera, got a batch of 3"):
        m.get_outputs_for_camera(_cams())
