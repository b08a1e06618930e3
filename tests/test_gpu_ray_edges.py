"""The ray generation and crop-box kernels (raygen_kernel, raygen_views_kernel, box_bins_kernel behind unerf_generate_rays,
unerf_generate_rays_views, unerf_ray_box_bins and unerf_ray_planes_bins) on the hand-placed cases of tests/ray_cases.py.

nears, fars and bins, and the origins, directions and pixel_area of PERSPECTIVE and ORTHOPHOTO cameras, must equal the fp32
restatement `chain32` BIT FOR BIT (planes up to the sign of a zero), the pixels behind a closed Newton gate included;
test_ray_cases_cpu.py holds chain32 to float64 under derived bounds, which is what gives the bit equality its meaning.
FISHEYE and EQUIRECTANGULAR directions and pixel areas are held to float64 evaluated at the restated fp32 angles under the
derived bound times ray_cases.FACTOR; no element is exempt but the 0 / 0 at the fisheye principal point, which must be NaN.
A ray lying in a slab face (0 / 0) must give finite planes and bins, those of chain32.  Every sub-range equals those rows of
the whole frame and every view of a batched launch equals unerf_generate_rays on its camera, bit for bit.

Every launch goes through the C ABI into outputs that lie between guard floats holding a NaN payload; an output passed
as null keeps its slot, which must come back untouched like the guards.  (The views of one launch share one contiguous
output, so no guard fits between them: a view that bleeds into its neighbour shows in the neighbour's bits.)

Every test prints its worst error / bound against float64 (DESIGN.md section 6.1.2 records them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ray_cases as RC

pytestmark = pytest.mark.gpu
_SENTINEL = 0x7FC0BEEF        # a NaN with a payload: no result has this bit pattern
_GUARD = 8
_FRAMES = {}


class _Slots:
    """float outputs of the given sizes in one buffer, guard floats in front of, between and behind them"""

    def __init__(self, dev, sizes):
        self.sizes, self.starts, at = sizes, [], _GUARD
        for n in sizes:
            self.starts.append(at)
            at += n + _GUARD
        self.buf = torch.full((at,), _SENTINEL, dtype=torch.int32, device=dev)

    def ptr(self, i, null=False):
        return None if null else C.c_void_p(self.buf.data_ptr() + 4 * self.starts[i])

    def read(self, what, null=()):
        """-> the outputs as float32 numpy arrays; everything outside them, and the slots passed as null, is untouched"""
        host = self.buf.cpu().numpy()
        live = np.zeros(host.shape, bool)
        for i, (a, n) in enumerate(zip(self.starts, self.sizes)):
            if i not in null:
                live[a: a + n] = True
        touched = np.flatnonzero(~live & (host != np.int32(_SENTINEL)))
        assert touched.size == 0, f"{what}: floats outside the outputs were written, first at {touched[:4]} (outputs start at {self.starts})"
        return [host[a: a + n].view(np.float32).copy() for a, n in zip(self.starts, self.sizes)]


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same_bits(a, b):
    """bit equality of two float32 arrays; a NaN equals a NaN of any payload"""
    a, b = np.ascontiguousarray(a, np.float32).reshape(-1), np.ascontiguousarray(b, np.float32).reshape(-1)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb])


def _first_off(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    off = np.flatnonzero(~((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))))
    return f"{off.size} of {a.size} elements differ, first at {off[:3]}: {a[off[:3]]} against {b[off[:3]]}"


# ---------------------------------------------------------------------------------------------------------------------- box
def _box_launch(dev, c, want_planes):
    from uncertainty_nerf_gs_amd import lib as L
    lib = L.load()
    R, n = c.R, c.n
    s = _Slots(dev, [R * (n + 1), R, R])
    row = _dev(c.row, dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        if c.kind == "planes":
            nr, fr = _dev(c.nears, dev), _dev(c.fars, dev)
            rc = lib.unerf_ray_planes_bins(p(nr), p(fr), R, c.near0, c.far0, c.lin, p(row), n, s.ptr(0), stream)
            want_planes = False
        else:
            o, d = _dev(c.o, dev), _dev(c.d, dev)
            rc = lib.unerf_ray_box_bins(p(o), p(d), R, (C.c_float * 12)(*c.w2b.tolist()), (C.c_float * 3)(*c.half.tolist()), c.near0, c.far0,
                                        c.lin, p(row), n, s.ptr(0), s.ptr(1, not want_planes), s.ptr(2, not want_planes), stream)
    L.check(rc, c.name)
    bins, nears, fars = s.read(c.name, null=() if want_planes else (1, 2))
    return bins.reshape(R, n + 1), (nears if want_planes else None), (fars if want_planes else None)


@pytest.mark.parametrize("name", list(RC.BOX_CASES))
def test_box_and_planes_bins_equal_chain32_bit_for_bit(dev, name):
    c = RC.box_case(name)
    ref_n, ref_f, ref_b = RC.box_chain32(c)
    bins, nears, fars = _box_launch(dev, c, c.want_planes)
    assert np.isfinite(bins).all(), f"{name}: non-finite bins on rays {[c.ray_names[i] for i in np.flatnonzero(~np.isfinite(bins).all(1))][:5]}"
    r = RC.hold_box(c, nears, fars, bins)
    print(f"RATIO {name}: R {c.R} n {c.n} worst error / bound against float64 {r:.3f}")
    assert _same_bits(bins, ref_b), f"{name}: bins: {_first_off(bins, ref_b)}"
    if c.want_planes:
        assert np.isfinite(nears).all() and np.isfinite(fars).all()
        # value equality: the sign of a zero is the one thing fmaxf(-0, +0) leaves open
        assert np.array_equal(nears, ref_n) and np.array_equal(fars, ref_f), f"{name}: planes differ from chain32"
        other = _box_launch(dev, c, False)[0]
        assert _same_bits(other, bins), f"{name}: the bins change when the planes outputs are null"
    elif c.kind == "box":
        other, nears, fars = _box_launch(dev, c, True)
        assert _same_bits(other, bins) and np.array_equal(nears, ref_n) and np.array_equal(fars, ref_f)


def test_rays_in_a_slab_face_give_finite_planes_and_bins(dev):
    """0 / 0: fminf / fmaxf drop the NaN, the ray is a miss at 1e10 and its bins collapse onto the far plane; upstream's
    amin / amax would return NaN planes (ray_cases.planes_upstream32)"""
    c = RC.box_case("unit-all-short-lin0")
    bins, nears, fars = _box_launch(dev, c, True)
    un, uf = RC.planes_upstream32(c.o, c.d, c.w2b, c.half)
    ref_b = RC.box_chain32(c)[2]
    for k in RC.FACE_RAYS:
        i = c.ray_names.index(k)
        assert np.isnan(un[i]) and np.isnan(uf[i])
        assert nears[i] == RC.INVALID and fars[i] == RC.INVALID and np.isfinite(bins[i]).all(), k
        assert np.all(bins[i] == bins[i, 0]) and _same_bits(bins[i], ref_b[i]), k


# --------------------------------------------------------------------------------------------------------------------- rays
def _rays_launch(dev, cam, start=0, count=None, want_pa=True, lens="own"):
    from uncertainty_nerf_gs_amd import lib as L
    lib = L.load()
    count = cam.H * cam.W - start if count is None else count
    s = _Slots(dev, [3 * count, 3 * count, count])
    lens = cam.lens if lens == "own" else lens
    dist = None if lens is None else (C.c_float * 6)(*[float(t) for t in lens])
    with torch.cuda.device(dev):
        rc = lib.unerf_generate_rays((C.c_float * 12)(*cam.c2w.reshape(-1).tolist()), cam.fx, cam.fy, cam.cx, cam.cy, dist, cam.camera_type,
                                     cam.H, cam.W, start, count, s.ptr(0), s.ptr(1), s.ptr(2, not want_pa),
                                     torch.cuda.current_stream().cuda_stream)
    L.check(rc, cam.name)
    o, d, pa = s.read(f"{cam.name} [{start}, +{count})", null=() if want_pa else (2,))
    return o.reshape(count, 3), d.reshape(count, 3), (pa if want_pa else None)


def _frame(dev, name):
    if name not in _FRAMES:
        _FRAMES[name] = _rays_launch(dev, RC.ray_case(name))
    return _FRAMES[name]


@pytest.mark.parametrize("name", [k for k, v in RC.RAY_CASES.items() if v[0] in (RC.PERSPECTIVE, RC.ORTHOPHOTO)])
def test_perspective_and_orthophoto_rays_equal_chain32_bit_for_bit(dev, name):
    o, d, pa = _frame(dev, name)
    ch = RC.rays_chain32(name)
    r = RC.hold_rays(name, o, d, pa)
    print(f"RATIO {name}: worst error / bound against float64 {r:.3f}; gate closed on {int(ch.closed.sum())} pixels, "
          f"{int(RC.rays_reference(name).undefined_pa.sum())} held to chain32 alone")
    assert _same_bits(o, ch.o), f"{name}: origins: {_first_off(o, ch.o)}"
    assert _same_bits(d, ch.d), f"{name}: directions: {_first_off(d, ch.d)}"
    assert _same_bits(pa, ch.pa), f"{name}: pixel_area: {_first_off(pa, ch.pa)}"


@pytest.mark.parametrize("name", [k for k, v in RC.RAY_CASES.items() if v[0] in (RC.FISHEYE, RC.EQUIRECTANGULAR)])
def test_fisheye_and_equirectangular_rays_within_the_bound_of_float64_at_the_restated_angles(dev, name):
    o, d, pa = _frame(dev, name)
    ch = RC.rays_chain32(name)
    r = RC.hold_rays(name, o, d, pa)          # a NaN on one side only fails
    print(f"RATIO {name}: worst error / (FACTOR x bound) {r:.3f}, without FACTOR {RC.hold_rays(name, o, d, pa, scaled=False):.3f}")
    assert _same_bits(o, ch.o)
    assert np.array_equal(np.isnan(d), np.isnan(ch.d)) and np.array_equal(np.isnan(pa), np.isnan(ch.pa))


@pytest.mark.parametrize("name", ["f-17x31-clip", "f-17x31-clip-lens"])
def test_fisheye_principal_point_is_nan(dev, name):
    """upstream's 0 / 0: u sin(theta) / theta at theta = 0.  The norm is fmaxf(sqrtf(NaN), 1e-7f) = 1e-7, and NaN / 1e-7 must
    still come out as NaN in all three components and in pixel_area"""
    c = RC.ray_case(name)
    u0, v0, _, _ = RC.pixel_coords32(c)
    g = int(np.flatnonzero((u0 == 0) & (v0 == 0))[0])
    o, d, pa = _frame(dev, name)
    assert np.isnan(d[g]).all() and np.isnan(pa[g]) and np.isfinite(o[g]).all()
    assert np.isnan(d).any(1).sum() == 1, "no other direction is NaN"
    o1, d1, pa1 = _rays_launch(dev, c, start=g, count=1)
    assert np.isnan(d1).all() and np.isnan(pa1).all()


def test_pinned_lens_identities(dev):
    """six zeros are the lens-free camera, EQUIRECTANGULAR ignores its lens, ORTHOPHOTO has pixel_area 0 and one direction"""
    plain = _frame(dev, "p-17x31")
    six = _frame(dev, "p-17x31-six-zeros")
    null = _rays_launch(dev, RC.lens_free("p-17x31-six-zeros"))
    assert all(_same_bits(a, b) and _same_bits(a, c) for a, b, c in zip(plain, six, null))
    e, el = _frame(dev, "e-8x16-north"), _frame(dev, "e-8x16-lens")
    assert all(_same_bits(a, b) for a, b in zip(e, el))
    for k in ("o-17x31", "o-17x31-lens"):
        o, d, pa = _frame(dev, k)
        assert np.all(pa.view(np.int32) == 0) and np.all(d.view(np.int32) == d[0].view(np.int32)) and np.abs(o - o[0]).max() > 0.1
    zero = _frame(dev, "p-17x31-zero-rotation")
    assert np.all(zero[1] == 0) and np.all(zero[2] == 0), "the 1e-7 norm clamp: directions exactly 0 (of either sign: 0 / 1e-7)"


@pytest.mark.parametrize("name", list(RC.RAY_CASES))
def test_every_range_equals_those_rows_of_the_whole_frame(dev, name):
    c = RC.ray_case(name)
    o, d, pa = _frame(dev, name)
    for k, (a, n) in enumerate(RC.RANGES[(c.H, c.W)]):
        want_pa = k % 2 == 0
        o2, d2, pa2 = _rays_launch(dev, c, start=a, count=n, want_pa=want_pa)
        assert _same_bits(o2, o[a: a + n]) and _same_bits(d2, d[a: a + n]), f"{name}: rows [{a}, +{n})"
        assert not want_pa or _same_bits(pa2, pa[a: a + n]), f"{name}: pixel_area of rows [{a}, +{n})"


# -------------------------------------------------------------------------------------------------------------------- views
def _views_launch(dev, name, want_pa=True):
    from uncertainty_nerf_gs_amd import lib as L
    lib = L.load()
    t, H, W, cams = RC.view_cameras(name)
    B, n = len(cams), H * W
    rec = (L.RayCamera * B)()
    for v, c in enumerate(cams):
        rec[v].c2w[:] = c.c2w.reshape(-1).tolist()
        rec[v].fx, rec[v].fy, rec[v].cx, rec[v].cy = c.fx, c.fy, c.cx, c.cy
        rec[v].distortion[:] = [0.0] * 6 if c.lens is None else [float(x) for x in c.lens]
    s = _Slots(dev, [3 * B * n, 3 * B * n, B * n])
    with torch.cuda.device(dev):
        rc = lib.unerf_generate_rays_views(rec, B, t, H, W, s.ptr(0), s.ptr(1), s.ptr(2, not want_pa), torch.cuda.current_stream().cuda_stream)
    L.check(rc, name)
    o, d, pa = s.read(name, null=() if want_pa else (2,))
    return cams, o.reshape(B, n, 3), d.reshape(B, n, 3), (pa.reshape(B, n) if want_pa else None)


@pytest.mark.parametrize("name", list(RC.VIEW_CASES))
def test_every_view_equals_generate_rays_on_its_camera(dev, name):
    cams, o, d, pa = _views_launch(dev, name)
    closed = 0
    for v, c in enumerate(cams):
        o1, d1, pa1 = _rays_launch(dev, c)
        assert _same_bits(o[v], o1), f"{name} view {v}: origins: {_first_off(o[v], o1)}"
        assert _same_bits(d[v], d1), f"{name} view {v}: directions: {_first_off(d[v], d1)}"
        assert _same_bits(pa[v], pa1), f"{name} view {v}: pixel_area: {_first_off(pa[v], pa1)}"
        if c.camera_type in (RC.PERSPECTIVE, RC.ORTHOPHOTO):
            ch = RC.camera_chain32(c)
            closed += int(ch.closed.sum())
            assert _same_bits(o[v], ch.o) and _same_bits(d[v], ch.d) and _same_bits(pa[v], ch.pa), f"{name} view {v} against chain32"
    print(f"RATIO {name}: {len(cams)} views of {cams[0].H} x {cams[0].W}, all bits those of unerf_generate_rays; gate closed on {closed} pixels")
    _, o2, d2, _ = _views_launch(dev, name, want_pa=False)
    assert _same_bits(o2, o) and _same_bits(d2, d), "the rays change when pixel_area is null"
