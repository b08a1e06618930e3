"""tests/ray_cases.py without a GPU: the fp32 restatement of the ray and crop-box kernels (`chain32`) lies within its derived
bounds of the float64 reference on every case and element (the undefined ones are named in ray_cases.py), the cases reach
the edges they were placed for, RATIO_MEASURED is what the CPU measures, and chain32 meets the torch oracle the older tests
trust."""
import numpy as np
import pytest
import torch

import ray_cases as RC
from oracle import nerf_oracle as O


def test_cases_reach_the_edges_they_were_placed_for():
    RC.check_coverage()


@pytest.mark.parametrize("name", list(RC.BOX_CASES))
def test_box_chain32_within_its_bounds_of_float64(name):
    c = RC.box_case(name)
    nears, fars, bins = RC.box_chain32(c)
    assert np.isfinite(bins).all() and np.isfinite(nears).all() and np.isfinite(fars).all()
    r = RC.hold_box(c, nears, fars, bins)
    p = RC.box_reference(c)
    print(f"RATIO {name}: chain32 worst error / bound {r:.3f}; largest bin bound {p.d_bins.max() / RC.U:.1f} U, "
          f"largest bin error {np.abs(bins - p.bins).max() / RC.U:.2f} U")
    assert p.d_bins.max() <= 100 * RC.U * max(1.0, np.abs(p.bins).max()), "the bin bound is a few tens of U, not a tolerance"


@pytest.mark.parametrize("name", list(RC.RAY_CASES))
def test_rays_chain32_within_its_bounds_of_float64(name):
    ch = RC.rays_chain32(name)
    r = RC.hold_rays(name, ch.o, ch.d, ch.pa)
    ref = RC.rays_reference(name)
    ok = ~ref.undefined
    print(f"RATIO {name}: chain32 worst error / bound {r:.3f}; largest direction bound {np.nanmax(ref.b_d[ok]) / RC.U:.1f} U; "
          f"undefined {int(ref.undefined.sum())} + pixel_area {int((ref.undefined_pa & ~ref.undefined).sum())} of {ok.size}")


def test_ratio_measured_is_what_the_cpu_measures():
    worst = 0.0
    for name, v in RC.RAY_CASES.items():
        if v[0] in (RC.FISHEYE, RC.EQUIRECTANGULAR):
            ch = RC.rays_chain32(name)
            worst = max(worst, RC.hold_rays(name, ch.o, ch.d, ch.pa, scaled=False))
    print(f"RATIO chain32 with numpy's float32 sin / cos against float64, unscaled: {worst:.4f} (RATIO_MEASURED {RC.RATIO_MEASURED})")
    assert worst <= RC.RATIO_MEASURED <= 1.25 * worst + 0.01
    assert 4 * RC.RATIO_MEASURED <= RC.FACTOR <= 4 * RC.RATIO_MEASURED + 0.05


def test_pinned_values_of_chain32():
    six, plain = RC.rays_chain32("p-17x31-six-zeros"), RC.rays_chain32("p-17x31")
    assert all(np.array_equal(getattr(six, k).view(np.int32), getattr(plain, k).view(np.int32)) for k in ("o", "d", "pa"))
    e, el = RC.rays_chain32("e-8x16-north"), RC.rays_chain32("e-8x16-lens")
    assert all(np.array_equal(getattr(e, k).view(np.int32), getattr(el, k).view(np.int32)) for k in ("o", "d", "pa"))
    for k in ("o-17x31", "o-17x31-lens"):
        o = RC.rays_chain32(k)
        assert np.all(o.pa == 0) and np.all(o.d == o.d[0]) and np.abs(o.o - o.o[0]).max() > 0.1
    assert np.array_equal(RC.rays_chain32("o-17x31").o, RC.rays_chain32("o-17x31-lens").o), "origins: the coordinate before the lens"


def test_the_strong_lens_has_a_root_on_every_pixel_and_a_converged_one_where_regular():
    c = RC.ray_case("p-24x40-strong")
    u0, v0, u1, v2 = RC.pixel_coords32(c)
    ch = RC.rays_chain32("p-24x40-strong")
    for u, v in ((u0, v0), (u1, v0), (u0, v2)):
        s = RC.undistort_reference(u, v, c.lens)
        assert (s.residual <= 1e-13).all(), "the forward model has a float64 root for every pixel, gate open or closed"
    s = RC.undistort_reference(u0, v0, c.lens)
    x32, y32, closed = RC._undistort32(u0, v0, c.lens)
    off = np.hypot(x32 - s.x, y32 - s.y)
    print(f"strong lens: gate closed on {closed.mean():.4f}, regular {s.regular.mean():.3f}; fp32 against the float64 root: regular "
          f"{off[s.regular].max():.2e}, closed {off[closed].max():.2e}, irregular {off[~s.regular & ~closed].max():.2e}")
    assert not (closed & s.regular).any() and ch.closed.any()
    for k in RC.MILD_LENS_CASES:
        c = RC.ray_case(k)
        p = RC.pixel_coords32(c)
        for u, v in ((p[0], p[1]), (p[2], p[1]), (p[0], p[3])):
            s = RC.undistort_reference(u, v, c.lens)
            assert s.regular.all() and (s.residual <= 1e-13).all(), f"{k}: the converged solution exists wherever the gate stays open"


@pytest.mark.parametrize("name", [k for k, v in RC.RAY_CASES.items() if v[0] == RC.PERSPECTIVE and k != "p-24x40-strong"])
def test_perspective_chain32_meets_the_torch_oracle(name):
    c = RC.ray_case(name)
    ch = RC.rays_chain32(name)
    o, d, pa = O.generate_rays(torch.from_numpy(c.c2w), c.fx, c.fy, c.cx, c.cy, c.H, c.W, distortion=c.lens)
    assert np.array_equal(o.reshape(-1, 3).numpy(), ch.o)
    worst = np.abs(d.reshape(-1, 3).numpy() - ch.d).max()
    print(f"{name}: chain32 against O.generate_rays: directions {worst:.2e}")
    assert worst <= 3e-7          # the tolerance of test_generate_rays_matches_oracle_and_row_major_indexing


@pytest.mark.parametrize("name", [k for k, v in RC.BOX_CASES.items() if v[0] == "box" and v[2] > 5])
def test_box_planes_of_chain32_meet_intersect_obb(name):
    """on the non-degenerate rays (no 0 / 0): intersect_obb inverts [R|T] in fp32 and multiplies with torch.matmul, so its
    planes agree to the older test's rtol 2e-5, not bit for bit"""
    c = RC.box_case(name)
    nears, fars, _ = RC.box_chain32(c)
    if c.w2b is RC.IDENTITY_W2B:
        Rm, T, S = torch.eye(3), torch.zeros(3), torch.ones(3)
    else:
        Rm, T, S = torch.from_numpy(RC.ROT_R).float(), torch.from_numpy(RC.ROT_T).float(), torch.from_numpy(2 * RC.ROT_HALF)
    keep = np.array([not (k in RC.FACE_RAYS and c.w2b is RC.IDENTITY_W2B) for k in c.ray_names])
    n_ref, f_ref = O.intersect_obb(torch.from_numpy(c.o), torch.from_numpy(c.d), Rm, T, S)
    n_ref, f_ref = n_ref.reshape(-1).numpy()[keep], f_ref.reshape(-1).numpy()[keep]
    p = RC.planes_reference(c.o, c.d, c.w2b, c.half)
    sure = p.clear[keep]                      # a planted exact tie may fall either way through another inverse
    for got, ref in ((nears[keep], n_ref), (fars[keep], f_ref)):
        assert np.allclose(got[sure], ref[sure], rtol=2e-5, atol=1e-6), name
    un, uf = RC.planes_upstream32(c.o, c.d, c.w2b, c.half)
    assert np.array_equal(np.isnan(un), ~keep) and np.array_equal(np.isnan(uf), ~keep)
