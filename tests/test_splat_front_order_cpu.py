"""The ops calls of the five splat frame functions, in order (CPU, no library): `splat.ops` is replaced by a recorder that logs
the name of every call (and of the count's start_copy) and answers with small CPU tensors of the right arity.

The order is part of what the front end is for: the intersection count's read-back starts behind the projection, travels under
the SH kernel (start_copy directly behind the shade call) and is awaited in the bin sort; the batch tangents of the pose Jacobian
are queued between start_copy and the bin sort.  The sequences below were read off the five functions as they stood when each
carried its own copy of the front end; a change of the shared one that reorders any of them fails here."""
import pytest
import torch

from uncertainty_nerf_gs_amd import ops as real_ops
from uncertainty_nerf_gs_amd import splat

N, H, W, B = 6, 8, 12, 3


class _Count:
    def __init__(self, log):
        self.log = log

    def start_copy(self):
        self.log.append("start_copy")


class Recorder:
    """stands in for the `ops` module: I is the intersection total every bin sort reports (per view in a batch), radius the
    value of every projected radius"""
    POSE_CHANNELS = real_ops.POSE_CHANNELS

    def __init__(self, I=5, radius=2, shade_rows=5):
        self.log, self.I, self.radius, self.shade_rows = [], I, radius, shade_rows

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        answer = getattr(self, "_" + name)

        def call(*a, **kw):
            self.log.append(name)
            return answer(*a, **kw)
        return call

    # host-only argument check: the real one
    def _pose_channel_bits(self, channels):
        return real_ops.pose_channel_bits(channels)

    # ---- one view ----
    def _splat_project(self, means, *a, **kw):
        n = means.shape[0]
        return (torch.zeros(n, 2), torch.ones(n), torch.full((n,), self.radius, dtype=torch.int32), torch.ones(n, 3), torch.ones(n),
                torch.ones(n, dtype=torch.int32), torch.zeros(n, 6), torch.full((n,), 0.5))

    def _SplatCount(self, tiles, defer_copy=False):
        return _Count(self.log)

    def _splat_shade_inputs(self, degree, means, *a):
        return torch.zeros(means.shape[0], self.shade_rows), torch.full((means.shape[0],), 0.5)

    def _splat_bin_sort(self, *a, **kw):
        return self.I, None, None, torch.zeros(max(self.I, 1), dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32)

    def _splat_rasterize(self, gids, bins, xys, conics, cols, opac, H, W, *a, **kw):
        return torch.zeros(H, W, cols.shape[1]), torch.ones(H, W), torch.zeros(H, W, dtype=torch.int32)

    def _splat_normalize_outputs(self, img, *a, **kw):
        h, w = img.shape[:2]
        return torch.zeros(h, w, 3), torch.zeros(h, w, 1), torch.zeros(h, w, 1), torch.zeros(h, w, 1)

    def _splat_depth_sqdiff(self, xys, depths, img, ch):
        return torch.zeros(xys.shape[0])

    def _splat_pose_tangents(self, means, *a, **kw):
        return torch.zeros(means.shape[0], 6, 12)

    def _splat_pose_grad(self, gids, bins, xys, conics, colors, opac, tan, H, W, *a, want_rgb=False, **kw):
        assert colors.shape[1] == 3
        return torch.zeros(H, W, 3, 4), torch.zeros(H, W, 3) if want_rgb else None, None

    def _splat_pose_tangents_proj(self, tan, means, radii, proj):
        return torch.zeros(means.shape[0], 7, 12)

    def _splat_pose_jacobian(self, gids, bins, xys, conics, colors, depths, opac, ptan, P, H, W, *a, channels=None, want=(), **kw):
        assert colors.shape[1] == 3
        return {k: torch.zeros(H, W, 5, P) if k == "proj" else torch.zeros(H, W, 5) for k in want}

    # ---- a batch of views ----
    def _splat_view_records(self, viewmats, *a):
        return object()

    def _splat_project_batch(self, means, scales, quats, views, b, *a, want_cov3d=False, **kw):
        n = means.shape[0]
        out = (torch.zeros(b, n, 2), torch.ones(b, n), torch.full((b, n), self.radius, dtype=torch.int32), torch.ones(b, n, 3),
               torch.ones(b, n), torch.ones(b, n, dtype=torch.int32), torch.full((b, n), 0.5))
        return out + (torch.zeros(b, n, 6),) if want_cov3d else out

    def _SplatCountBatch(self, tiles, radii, defer_copy=False):
        return _Count(self.log)

    def _splat_shade_inputs_batch(self, degree, means, views, b, *a):
        return torch.zeros(b, means.shape[0], self.shade_rows), torch.full((b, means.shape[0]), 0.5)

    def _splat_pose_ptangents_batch(self, means, cov3d, radii, views, b, projs, *a):
        assert cov3d is not None and tuple(projs.shape[:2]) == (b, 12)
        return torch.zeros(b, means.shape[0], 7, 12)

    def _splat_bin_sort_batch(self, xys, *a, **kw):
        b = xys.shape[0]
        return [self.I] * b, [self.radius > 0] * b, torch.zeros(max(self.I, 1), dtype=torch.int32), torch.zeros(b, 1, 2, dtype=torch.int32)

    def _splat_rasterize_batch(self, gids, bins, xys, conics, cols, opac, H, W, *a, **kw):
        b = xys.shape[0]
        return torch.zeros(b, H, W, cols.shape[2]), torch.ones(b, H, W), torch.zeros(b, H, W, dtype=torch.int32)

    def _splat_normalize_outputs_batch(self, img, *a, **kw):
        b, h, w = img.shape[:3]
        return torch.zeros(b, h, w, 3), torch.zeros(b, h, w, 1), torch.zeros(b, h, w, 1), torch.zeros(b, h, w, 1)

    def _splat_depth_sqdiff_batch(self, xys, depths, img, ch):
        return torch.zeros(xys.shape[0], xys.shape[1])

    def _splat_pose_jacobian_batch(self, gids, bins, xys, conics, colors, depths, opac, ptan, P, H, W, *a, want=(), **kw):
        b = xys.shape[0]
        return {k: torch.zeros(b, H, W, 5, P) if k == "proj" else torch.zeros(b, H, W, 5) for k in want}


def _gp(n=N, active=True):
    gp = {"means": torch.zeros(n, 3), "scales": torch.zeros(n, 3), "quats": torch.ones(n, 4), "features_dc": torch.zeros(n, 3),
          "features_rest": torch.zeros(n, 15, 3), "opacities": torch.zeros(n, 1)}
    if active:
        gp["log_uncertainties"] = torch.zeros(n, 1)
    return gp


CAM = (20.0, 20.0, W / 2, H / 2, H, W)
BG = torch.tensor([0.1, 0.2, 0.3])


def _c2w():
    c = torch.eye(4)[:3].clone()
    c[2, 3] = 2.0
    return c


def _c2ws():
    return torch.stack([_c2w() for _ in range(B)])


# function -> (call, what it returns per view)
def _outputs(gp, **kw):
    return splat.active_splatfacto_outputs(gp, _c2w(), *CAM, BG, **kw)


def _outputs_batch(gp, **kw):
    return splat.active_splatfacto_outputs_batch(gp, _c2ws(), *CAM, BG, **kw)


def _gradient(gp, **kw):
    return splat.pose_gradient_camera(gp, _c2w(), *CAM, BG, want_rgb=True, **kw)


def _jacobian(gp, **kw):
    return splat.pose_jacobian_camera(gp, _c2w(), *CAM, BG, **kw)


def _jacobians(gp, **kw):
    return splat.pose_jacobian_cameras(gp, _c2ws(), *CAM, BG, **kw)


FRAME = {
    "outputs": (_outputs, [
        "splat_project", "SplatCount", "splat_shade_inputs", "start_copy", "splat_bin_sort",
        "splat_rasterize", "splat_normalize_outputs", "splat_depth_sqdiff", "splat_rasterize", "splat_normalize_outputs"]),
    "outputs_batch": (_outputs_batch, [
        "splat_view_records", "splat_project_batch", "SplatCountBatch", "splat_shade_inputs_batch", "start_copy",
        "splat_bin_sort_batch",
        "splat_rasterize_batch", "splat_normalize_outputs_batch", "splat_depth_sqdiff_batch", "splat_rasterize_batch",
        "splat_normalize_outputs_batch"]),
    "gradient": (_gradient, [
        "splat_project", "SplatCount", "splat_shade_inputs", "start_copy", "splat_bin_sort",
        "splat_pose_tangents", "splat_pose_grad"]),
    "jacobian": (_jacobian, [
        "pose_channel_bits",
        "splat_project", "SplatCount", "splat_shade_inputs", "start_copy", "splat_bin_sort",
        "splat_pose_tangents", "splat_pose_tangents_proj", "splat_pose_jacobian"]),
    "jacobians": (_jacobians, [
        "pose_channel_bits",
        "splat_view_records", "splat_project_batch", "SplatCountBatch", "splat_shade_inputs_batch", "start_copy",
        "splat_pose_ptangents_batch", "splat_bin_sort_batch",
        "splat_pose_jacobian_batch"]),
}
# plain splatfacto (no log_uncertainties): one rasteriser pass
PLAIN = {
    "outputs": [
        "splat_project", "SplatCount", "splat_shade_inputs", "start_copy", "splat_bin_sort",
        "splat_rasterize", "splat_normalize_outputs"],
    "outputs_batch": [
        "splat_view_records", "splat_project_batch", "SplatCountBatch", "splat_shade_inputs_batch", "start_copy",
        "splat_bin_sort_batch",
        "splat_rasterize_batch", "splat_normalize_outputs_batch"],
}
# nothing to render, decided before anything is queued: no splats, or an all-false crop
EARLY_EMPTY = {
    "outputs": [],
    "outputs_batch": [],
    "gradient": [],
    "jacobian": ["pose_channel_bits"],
    "jacobians": ["pose_channel_bits"],
}
# nothing to render, decided by the bin sort (I == 0, and no radius above 0 where the lists are tight): the front end only
LATE_EMPTY = {
    "outputs": ["splat_project", "SplatCount", "splat_shade_inputs", "start_copy", "splat_bin_sort"],
    "outputs_batch": ["splat_view_records", "splat_project_batch", "SplatCountBatch", "splat_shade_inputs_batch", "start_copy",
                      "splat_bin_sort_batch"],
    "gradient": ["splat_project", "SplatCount", "splat_shade_inputs", "start_copy", "splat_bin_sort"],
    "jacobian": ["pose_channel_bits", "splat_project", "SplatCount", "splat_shade_inputs", "start_copy", "splat_bin_sort"],
    "jacobians": ["pose_channel_bits", "splat_view_records", "splat_project_batch", "SplatCountBatch", "splat_shade_inputs_batch",
                  "start_copy", "splat_pose_ptangents_batch", "splat_bin_sort_batch"],
}


@pytest.fixture
def record(monkeypatch):
    def install(**kw):
        rec = Recorder(**kw)
        monkeypatch.setattr(splat, "ops", rec)
        monkeypatch.setattr(splat._l, "require_gpu", lambda: None)
        return rec
    return install


def _views(name, out):
    return out if name in ("outputs_batch", "jacobians") else [out]


def _is_empty(name, view):
    """the function's answer for a frame the reference renders with get_empty_outputs"""
    if name.startswith("outputs"):
        return "uncertainty" not in view and bool((view["depth"] == 10).all()) and bool((view["rgb"] == BG).all())
    if name == "gradient":
        return not view[0].any() and bool((view[1] == BG).all())
    return not view["proj"].any() and bool((view["val"][..., :3] == BG).all())


@pytest.mark.parametrize("tight", [True, False])
@pytest.mark.parametrize("name", list(FRAME))
def test_a_rendered_frame_makes_the_calls_in_order(record, name, tight):
    rec = record()
    call, want = FRAME[name]
    out = call(_gp(), tight=tight)
    assert rec.log == want
    if name.startswith("outputs"):
        assert all("uncertainty" in v for v in _views(name, out))


@pytest.mark.parametrize("tight", [True, False])
@pytest.mark.parametrize("name", list(PLAIN))
def test_a_plain_frame_makes_one_rasteriser_pass(record, name, tight):
    rec = record(shade_rows=4)
    out = FRAME[name][0](_gp(active=False), tight=tight)
    assert rec.log == PLAIN[name]
    assert all(sorted(v) == ["accumulation", "background", "depth", "rgb"] for v in _views(name, out))


@pytest.mark.parametrize("tight", [True, False])
@pytest.mark.parametrize("why", ["no splats", "all-false crop"])
@pytest.mark.parametrize("name", list(FRAME))
def test_an_empty_scene_queues_nothing(record, name, why, tight):
    rec = record()
    gp = _gp(0) if why == "no splats" else _gp()
    crop = None if why == "no splats" else torch.zeros(N, dtype=torch.bool)
    out = FRAME[name][0](gp, tight=tight, crop_ids=crop)
    assert rec.log == EARLY_EMPTY[name]
    assert all(_is_empty(name, v) for v in _views(name, out))


@pytest.mark.parametrize("tight", [True, False])
@pytest.mark.parametrize("name", list(FRAME))
def test_a_frame_without_intersections_stops_behind_the_bin_sort(record, name, tight):
    rec = record(I=0, radius=0)
    out = FRAME[name][0](_gp(), tight=tight)
    assert rec.log == LATE_EMPTY[name]
    assert all(_is_empty(name, v) for v in _views(name, out))


@pytest.mark.parametrize("name", list(FRAME))
def test_tight_lists_that_are_empty_under_visible_splats_are_still_walked(record, name):
    """every opacity below 1/255: I == 0 with radii > 0 -- the reference rasterises a frame in which nothing blends"""
    rec = record(I=0, radius=2)
    FRAME[name][0](_gp(), tight=True)
    assert rec.log == FRAME[name][1]
    rec.log.clear()
    FRAME[name][0](_gp(), tight=False)
    assert rec.log == LATE_EMPTY[name]


def test_a_partial_crop_reaches_the_projection_cropped(record):
    rec = record()
    seen = []
    rec._splat_project = lambda means, *a, _f=rec._splat_project, **kw: (seen.append(means.shape[0]), _f(means, *a, **kw))[1]
    crop = torch.tensor([True, False, True, True, False, False])
    for name in ("outputs", "gradient", "jacobian"):
        FRAME[name][0](_gp(), crop_ids=crop)
    assert seen == [3, 3, 3]
