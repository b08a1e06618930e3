"""Hand-placed cases for the ray stage (plain module: tests import it; nothing here needs a GPU).

raygen_kernel / raygen_views_kernel (unerf_generate_rays, unerf_generate_rays_views) and box_bins_kernel (unerf_ray_box_bins,
unerf_ray_planes_bins) of csrc/unerf_nerf.hip, section 1.  Two references:

`chain32` -- the kernels' operation lists restated in numpy float32, in the kernels' order (box_chain32, rays_chain32).  The
library is built with -ffp-contract=off, and fp32 division and sqrtf are correctly rounded by default (prop_cases.py relies
on both), so box_bins_kernel is a fixed list of IEEE operations from the rays to the bins (slab test, clamps,
unerf_spacing_of, the fold; np.fmin / np.fmax drop a NaN as fminf / fmaxf do), and so is raygen_one for PERSPECTIVE and
ORTHOPHOTO (pixel coordinates, the ten gated Newton steps, the rotation sum, the clamped norm, the three divisions,
pixel_area).  The kernels must equal chain32 BIT FOR BIT there, the pixels behind a closed Newton gate included; planes may
differ in the sign of a zero (fmaxf(-0, +0) is either), nothing else.  For FISHEYE and EQUIRECTANGULAR the list is bit-defined up to
the arguments of sinf / cosf (u, v, the undistortion, theta, phi: `angles32`); chain32 goes on with numpy's float32 sin / cos
and is used only to measure FACTOR.  No other operation was found that is not bit-defined on the device.

`reference` -- float64 (box_reference, rays_reference).  Box: the exact slab intersection of the fp32 ray with the fp32 box
transform, and the fold b' = (b s(far_r) + (1 - b) s(near_r) - s(near0)) / (s(far0) - s(near0)) with both planes cut at far0 as
the kernel documents.  Rays: the camera model at the fp32 pixel coordinates; a distorted PERSPECTIVE camera solves the
forward OPENCV model to a residual <= 1e-13 (Newton continued from the distorted point, other starts where that fails) and
does not restate ten steps; FISHEYE / EQUIRECTANGULAR are evaluated at the restated fp32 theta (theta, phi).

Bounds, per element, first order on absolute values in float64, U = 2^-24 (nothing here comes from a kernel):
  * slab parameter t = (+-half - bo) / bd: bo and bd are three products and three (two) sums, d_bo = U (sum |products| + sum
    |partial sums|), likewise d_bd; the numerator adds U |num|, the quotient U |t|: dt = d_num / |bd| + |num| d_bd /
    (|bd| (|bd| - d_bd)) + U |t|.  bd = 0 gives the same infinity on both sides, error 0.
  * planes: max / min over the slabs as intervals: the fp32 maximum lies in [max (lo - d), max (lo + d)].  The clamps are
    1-Lipschitz.  Hit or miss is a discontinuity: build() asserts that every ray is a hit or a miss by more than twice
    the bounds, or is one of the planted exact ties, which chain32 must decide as the reference does (check_margins).
  * s(x): x / 2 is exact; 1 - 1 / (2 x) takes U / (2 x) + U |s|; an input error is carried with the slope 1/2 below 1 and
    1 / (2 (x - dx)^2) above (s is C^1 across 1).
  * fold: e = b sf + (1 - b) sn: de = b d_sf + |1 - b| d_sn + U (|b sf| + 2 |(1 - b) sn| + |e|); where fp32 has sf == sn and takes
    sn, the float64 blend differs by at most b d_sf + |1 - b| d_sn for b in [0, 1], so the same bound holds.  g = e - sn0,
    D = s(far0) - sn0, inv = 1 / D, bin = g inv: each adds U of its result; d_inv = d_D / D^2 + U |inv|.
    A CPU probe gives 2.6 U at (0.05, 1000) and 4.2 U at (0.05, 1.5); the bound is a few tens of U.
  * direction: x = (cx R0 + cy R1) + cz R2: dx = sum |R| d_c + U (sum |products| + |partial sum| + |x|) (PERSPECTIVE without a
    lens: d_c = 0 and cz R2 = -R2 is exact); q = x^2 + y^2 + z^2: dq = sum 2 |x| dx + 3 U q; n = max(sqrt q, 1e-7): dn = dq / (2 n) + U n;
    component x / n: dx / n + |x| dn / n^2 + U |x / n|.  A few U.
  * undistorted coordinate (lens, gate open, `regular` pixels): the last Newton step lands within J^-1 d_f of the root,
    d_f the rounding of the residual: d_d = U (|d| + 16 A), A = r (|k1| + r (|k2| + r (|k3| + r |k4|))) (four Horner stages, two
    roundings each, over r with its own 2 U), d_f = |x| d_d + 6 U (|d x| + |2 p1 x y| + |p2| (r + 2 x^2) + |xd|); twice
    |J^-1| d_f (the step before it started that far off) + 2 U |x| + the truncation of ten steps, |x10 - x*| of the float64
    recurrence itself.
  * pixel_area: e = d0 - d1 per component, d_e = d_d0 + d_d1 + U |e|; | |a| - |b| | <= |a - b|, so d|e| = sqrt(sum d_e^2) + 2.5 U |e|;
    the product: |ex| d|ey| + |ey| d|ex| + d|ex| d|ey| + U pa.  The difference of unit vectors is where the relative bound
    grows: at fx = 1e5 |e| is 1e-5 against d_e of a few U, 1e-2 relative -- why the older test needs 1e-3 at fx = 41.
  * FISHEYE: sin, cos take U |value| (correctly rounded); u sin / theta: |u / theta| d_sin + 2 U |value|.  EQUIRECTANGULAR:
    products of two of them, |a| d_b + |b| d_a + U |a b|.  Then the direction bound above with these d_c.  The whole bound is
    multiplied by FACTOR = 4 x RATIO_MEASURED, the worst error / bound of chain32 (numpy's float32 sin / cos) against the
    reference over all such cases, measured on the CPU; the 4 x covers the device sinf / cosf against a correctly rounded
    one, the margin of prop_cases.FACTOR and pdf_cases.EPS_CDF.  test_ray_cases_cpu.py re-measures it.

Undefined against float64, by name (all of them are still bit-defined and held to chain32 on the GPU):
  * `closed`: pixels of the strong barrel lens on which the gate |det J| > 1e-3 closes in chain32 (0.7 %); the fp32
    result lies up to 3.4 from the float64 root there.
  * `irregular`: pixels of the strong lens beyond the fold of its forward map (|(u, v)| > 0.70: x (1 - 0.3 r) turns back at
    r = 1.11).  The only real root lies on the far branch, the ten steps wander, and the float64 recurrence itself is not
    within 1e-9 of a root after ten steps or passes |det J| < DET_MIN.  A root exists for every pixel (asserted), the
    recurrence just does not reach it.  A pixel is `regular` when all three of its coordinates are neither.
  * the FISHEYE pixel at the exact principal point: upstream's 0 / 0, NaN in the three direction components and in
    pixel_area, and in the pixel_area of its two neighbours that difference against it.  Pinned as NaN, not bounded.

Pinned behaviours that differ from upstream by design:
  * a ray lying IN a slab face (bd = 0, bo = +-half) gives 0 / 0 = NaN for one slab parameter and an infinity for the other;
    fminf / fmaxf drop the NaN, the infinity makes the ray a miss, and nears = fars = 1e10 and all bins are finite.
    upstream's amin / amax propagate the NaN into both planes (planes_upstream32).  The float64 reference takes a ray that
    lies in a face as a miss, too.
  * a miss collapses onto the far plane: all bins equal (s(far0) - s(near0)) inv.
  * ORTHOPHOTO origins use the pixel coordinate BEFORE the undistortion (raygen_one passes u0, v0 by value); the torch
    oracle's generate_rays moves the origin by the undistorted one.  No older test has an ORTHOPHOTO camera with a lens;
    chain32 restates the kernel, and the disagreement is recorded here and in DESIGN.md rather than settled.

Out of reach at test size: R (n + 1) >= 2^31."""
import functools
from types import SimpleNamespace

import numpy as np

f32 = np.float32
U = 2.0 ** -24
PERSPECTIVE, FISHEYE, EQUIRECTANGULAR, ORTHOPHOTO = 1, 2, 3, 8
PI32 = f32(3.14159265358979323846)
NF_LONG, NF_SHORT = (0.05, 1000.0), (0.05, 1.5)
INVALID = f32(1e10)
UNDISTORT_EPS, UNDISTORT_ITERATIONS = f32(1e-3), 10
DET_MIN = 0.05
# (k1, k2, k3, k4, p1, p2): test_gpu_nerf_kernels.LENSES, and the strong barrel lens that closes the gate
LENSES = [(-0.05, 0.02, 0.0, 0.0, 1e-3, -1e-3), (0.12, -0.03, 0.0, 0.0, 0.0, 0.0), (-0.2, 0.06, -0.01, 0.002, 4e-3, 2e-3),
          (0.0, 0.0, 0.0, 0.0, 2e-3, 0.0)]
STRONG = (-0.3, 0.0, 0.0, 0.0, 0.0, 0.0)
FISHEYE_LENS = (0.05, -0.01, 0.002, -0.0004, 0.0, 0.0)
# worst error / unscaled bound of chain32 (numpy float32 sin / cos) over the FISHEYE / EQUIRECTANGULAR cases, measured on the
# CPU against the float64 reference, never a kernel; FACTOR = 4 x it, rounded up
RATIO_MEASURED = 0.38
FACTOR = 1.52
# share of the 200 seeded random box rays that hit (check_coverage asserts it, and that it lies in [0.2, 0.9])
HIT_SHARE = 0.45


def _a32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=f32))


# ======================================================================================================================= box
def spacing32(x, lin):
    """unerf_spacing_of on a float32 array"""
    assert x.dtype == f32
    if lin:
        return x
    with np.errstate(all="ignore"):
        return np.where(x < f32(1), x / f32(2), f32(1) - f32(1) / (f32(2) * x)).astype(f32)


def _slabs32(o, d, w2b, half, fmin, fmax):
    R = o.shape[0]
    tmin, tmax = np.full(R, -np.inf, f32), np.full(R, np.inf, f32)
    ox, oy, oz, dx, dy, dz = o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        for c in range(3):
            m = w2b[4 * c: 4 * c + 4]
            bo = ((m[0] * ox + m[1] * oy) + m[2] * oz) + m[3]
            bd = (m[0] * dx + m[1] * dy) + m[2] * dz
            t0, t1 = (-half[c] - bo) / bd, (half[c] - bo) / bd
            tmin = fmax(tmin, fmin(t0, t1))
            tmax = fmin(tmax, fmax(t0, t1))
        tmin = fmin(fmax(tmin, f32(0)), INVALID)
        tmax = fmin(fmax(tmax, f32(0)), INVALID)
    assert tmin.dtype == f32 and tmax.dtype == f32
    return tmin, tmax


def planes_chain32(o, d, w2b, half):
    """box_bins_kernel's slab test -> nears, fars [R] float32"""
    tmin, tmax = _slabs32(o, d, w2b, half, np.fmin, np.fmax)
    miss = ~(tmax > tmin)
    return np.where(miss, INVALID, tmin), np.where(miss, INVALID, tmax)


def planes_upstream32(o, d, w2b, half):
    """what intersect_obb's amin / amax and clamp give in fp32: a NaN slab parameter reaches both planes"""
    tmin, tmax = _slabs32(o, d, w2b, half, np.minimum, np.maximum)
    with np.errstate(invalid="ignore"):
        cond = tmax <= tmin
    return np.where(cond, INVALID, tmin), np.where(cond, INVALID, tmax)


def bins_chain32(tmin, tmax, near0, far0, lin, row):
    """the fold of box_bins_kernel -> [R, n + 1] float32"""
    near0, far0 = f32(near0), f32(far0)
    one = np.ones(1, f32)
    with np.errstate(all="ignore"):
        sn, sf = spacing32(np.fmin(tmin, far0), lin)[:, None], spacing32(np.fmin(tmax, far0), lin)[:, None]
        sn0 = spacing32(one * near0, lin)
        inv = f32(1) / (spacing32(one * far0, lin) - sn0)
        b = row[None, :]
        e = np.where(sf == sn, sn, b * sf + (f32(1) - b) * sn)
        out = (e - sn0) * inv
    assert out.dtype == f32
    return out


def box_chain32(c):
    """-> nears, fars [R], bins [R, n + 1], all float32"""
    if c.kind == "planes":
        tmin, tmax = c.nears, c.fars
    else:
        tmin, tmax = planes_chain32(c.o, c.d, c.w2b, c.half)
    return tmin, tmax, bins_chain32(tmin, tmax, c.near0, c.far0, c.lin, c.row)


def _dot_err(terms):
    """left-to-right fp32 sum of exact-in-float64 products: value and U x (|products| + |partial sums|)"""
    s, err = 0.0, 0.0
    for i, t in enumerate(terms):
        s = s + t if i else t
        err = err + np.abs(t) + (np.abs(s) if i else 0.0)
    return s, U * err


def planes_reference(o, d, w2b, half):
    """float64 slab intersection -> SimpleNamespace(nears, fars, d_near, d_far, hit, clear): `clear` where hit or miss holds
    by more than twice the bounds"""
    o, d, m, half = (np.asarray(a, np.float64) for a in (o, d, w2b, half))
    R = o.shape[0]
    lo, hi, dlo, dhi = (np.empty((3, R)) for _ in range(4))
    with np.errstate(all="ignore"):
        for c in range(3):
            r = m[4 * c: 4 * c + 4]
            bo, d_bo = _dot_err([r[0] * o[:, 0], r[1] * o[:, 1], r[2] * o[:, 2], r[3] + 0 * o[:, 0]])
            bd, d_bd = _dot_err([r[0] * d[:, 0], r[1] * d[:, 1], r[2] * d[:, 2]])
            par = bd == 0
            ts, dts = [], []
            for sgn in (-1.0, 1.0):
                num = sgn * half[c] - bo
                t = num / bd
                dt = (d_bo + U * np.abs(num)) / np.abs(bd) + np.abs(num) * d_bd / (np.abs(bd) * (np.abs(bd) - d_bd)) + U * np.abs(t)
                dt = np.where(np.abs(bd) > 2 * d_bd, dt, np.inf)
                ts.append(t), dts.append(dt)
            first = ts[0] <= ts[1]
            lo[c], dlo[c] = np.where(first, ts[0], ts[1]), np.where(first, dts[0], dts[1])
            hi[c], dhi[c] = np.where(first, ts[1], ts[0]), np.where(first, dts[1], dts[0])
            inside = np.abs(bo) < half[c]          # a ray IN a face is a miss (module docstring)
            lo[c] = np.where(par, np.where(inside, -np.inf, np.inf), lo[c])
            hi[c] = np.where(par, np.where(inside, np.inf, -np.inf), hi[c])
            dlo[c], dhi[c] = np.where(par, 0.0, dlo[c]), np.where(par, 0.0, dhi[c])
        tmin, tmax = lo.max(0), hi.min(0)
        d_min = np.where(np.isfinite(tmin), np.maximum((lo + dlo).max(0) - tmin, tmin - (lo - dlo).max(0)), 0.0)
        d_max = np.where(np.isfinite(tmax), np.maximum((hi + dhi).min(0) - tmax, tmax - (hi - dhi).min(0)), 0.0)
        d_min, d_max = np.nan_to_num(d_min, nan=np.inf), np.nan_to_num(d_max, nan=np.inf)
    cmin, cmax = np.clip(tmin, 0.0, 1e10), np.clip(tmax, 0.0, 1e10)
    hit = cmax > cmin
    c_min, c_max = _through(lambda t: np.clip(t, 0.0, 1e10), tmin, d_min), _through(lambda t: np.clip(t, 0.0, 1e10), tmax, d_max)
    gap = 2 * (d_min + d_max)
    with np.errstate(invalid="ignore"):
        clear_hit = (cmax - cmin > gap) & (tmax - d_max > 0) & (tmin + d_min < 1e10)
        clear_miss = (tmax + d_max < tmin - d_min) | (tmax + d_max < 0) | (tmin - d_min > 1e10) | (tmin == np.inf) | (tmax == -np.inf)
    big = float(INVALID)
    return SimpleNamespace(nears=np.where(hit, cmin, big), fars=np.where(hit, cmax, big), d_near=np.where(hit, c_min, 0.0),
                           d_far=np.where(hit, c_max, 0.0), hit=hit, clear=np.where(hit, clear_hit, clear_miss), raw=(tmin, tmax))


def _through(fn, x, dx):
    """the error of a monotone 1-Lipschitz fn (a clamp) applied to x +- dx"""
    with np.errstate(invalid="ignore"):
        return np.nan_to_num(np.maximum(fn(x + dx) - fn(x), fn(x) - fn(x - dx)), nan=0.0)


def _spacing64(x, dx, lin):
    """s(x) and its error for an input error dx"""
    x = np.asarray(x, np.float64)
    if lin:
        return x, dx + 0 * x
    with np.errstate(all="ignore"):
        s = np.where(x < 1, x / 2, 1 - 1 / (2 * x))
        xl = x - dx
        slope = np.where(xl < 1, 0.5, 1 / (2 * xl * xl))
        own = np.where(x >= 1, U / (2 * x) + U * np.abs(s), 0.0)
    return s, np.where(dx > 0, slope * dx, 0.0) + own


def bins_reference(near_r, far_r, d_near, d_far, near0, far0, lin, row):
    """float64 fold on the fp32 launch planes and row -> bins [R, n + 1], bound [R, n + 1]"""
    near0, far0 = float(f32(near0)), float(f32(far0))
    b = np.asarray(row, np.float64)[None, :]
    cut = lambda t: np.minimum(t, far0)
    sn, d_sn = _spacing64(cut(near_r), _through(cut, near_r, d_near), lin)
    sf, d_sf = _spacing64(cut(far_r), _through(cut, far_r, d_far), lin)
    sn, d_sn, sf, d_sf = sn[:, None], d_sn[:, None], sf[:, None], d_sf[:, None]
    sn0, d_sn0 = _spacing64(near0, 0.0, lin)
    sf0, d_sf0 = _spacing64(far0, 0.0, lin)
    e = b * sf + (1 - b) * sn
    d_e = b * d_sf + np.abs(1 - b) * d_sn + U * (np.abs(b * sf) + 2 * np.abs((1 - b) * sn) + np.abs(e))
    g = e - sn0
    d_g = d_e + d_sn0 + U * np.abs(g)
    D = sf0 - sn0
    d_D = d_sf0 + d_sn0 + U * abs(D)
    inv = 1 / D
    d_inv = d_D / (D * D) + U * abs(inv)
    out = g * inv
    return out, d_g * abs(inv) + np.abs(g) * d_inv + U * np.abs(out)


def box_reference(c):
    """-> SimpleNamespace(nears, fars, d_near, d_far, bins, d_bins, hit, clear)"""
    if c.kind == "planes":
        z = np.zeros(c.R)
        p = SimpleNamespace(nears=c.nears.astype(np.float64), fars=c.fars.astype(np.float64), d_near=z, d_far=z,
                            hit=np.ones(c.R, bool), clear=np.ones(c.R, bool))
    else:
        p = planes_reference(c.o, c.d, c.w2b, c.half)
    p.bins, p.d_bins = bins_reference(p.nears, p.fars, p.d_near, p.d_far, c.near0, c.far0, c.lin, c.row)
    return p


def ratio(got, ref, bound):
    """worst |got - ref| / bound; a zero bound demands equality, a NaN on one side only is infinitely off"""
    got, ref, bound = (np.asarray(a, np.float64) for a in np.broadcast_arrays(got, ref, bound))
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    both_nan = np.isnan(got) & np.isnan(ref)
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(both_nan, 0.0, r)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


def hold_box(c, nears, fars, bins):
    """worst error / bound of float32 results against box_reference(c); asserts <= 1"""
    p = box_reference(c)
    rs = [ratio(bins, p.bins, p.d_bins)]
    if nears is not None:
        rs += [ratio(nears, p.nears, p.d_near), ratio(fars, p.fars, p.d_far)]
    assert max(rs) <= 1.0, f"{c.name}: worst error / bound {max(rs):.3f} (bins, nears, fars: {rs})"
    return max(rs)


# ---- boxes and rays
IDENTITY_W2B = _a32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
UNIT_HALF = _a32([0.5, 0.5, 0.5])


def _rotated_box():
    """world_to_box of a rotated and translated box, inverted in float64 and rounded once"""
    a, b, g = 0.4, -0.7, 1.1
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(g), -np.sin(g), 0], [np.sin(g), np.cos(g), 0], [0, 0, 1]])
    Rm, T = rz @ ry @ rx, np.array([0.1, -0.05, 0.2])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = Rm, T
    return _a32(np.linalg.inv(M)[:3].reshape(-1)), _a32([0.4, 0.25, 0.55]), Rm, T


ROT_W2B, ROT_HALF, ROT_R, ROT_T = _rotated_box()
NZ = -0.0
# name -> (origin, direction) against the unit box with the identity transform: every product with w2b is exact, so the
# components written as 0 are bd == +-0 and the slab parameters below are exact fp32 numbers
PLANTED_UNIT = {
    "one-zero-inside+0": ((-1, -1.2, 0.25), (0.6, 0.8, 0.0)),          # hit [0.875, 2.125]
    "one-zero-inside-0": ((-1, -1.2, 0.25), (0.6, 0.8, NZ)),
    "one-zero-outside+0": ((-1, -1.2, 0.75), (0.6, 0.8, 0.0)),         # miss
    "one-zero-outside-0": ((-1, -1.2, 0.75), (0.6, 0.8, NZ)),
    "one-zero-face+0": ((-1, -1.2, 0.5), (0.6, 0.8, 0.0)),             # 0 / 0
    "one-zero-face-0": ((-1, -1.2, -0.5), (0.6, 0.8, NZ)),
    "two-zero-inside+0": ((-2, 0.25, 0.125), (1, 0.0, 0.0)),           # hit [1.5, 2.5]
    "two-zero-inside-0": ((-2, 0.25, 0.125), (1, NZ, NZ)),
    "two-zero-inside+-0": ((2, 0.25, 0.125), (-1, 0.0, NZ)),
    "two-zero-outside+0": ((-2, 0.75, 0.125), (1, 0.0, 0.0)),
    "two-zero-outside-0": ((-2, 0.25, -0.75), (1, NZ, NZ)),
    "two-zero-face+0": ((-2, 0.5, 0.125), (1, 0.0, 0.0)),              # 0 / 0 in one slab
    "two-zero-face-0": ((-2, -0.5, 0.125), (1, NZ, NZ)),
    "two-zero-edge-line": ((-2, 0.5, -0.5), (1, 0.0, NZ)),             # 0 / 0 in two slabs
    "through-edge": ((-1.5, -0.5, 0.0), (1, 1, 0.0)),                  # tmax == tmin == 1
    "through-corner": ((-1.5, -0.5, -0.5), (1, 1, 1)),                 # tmax == tmin == 1 in all three
    "origin-inside": ((0.125, -0.25, 0.25), (0.6, 0.25, 0.8)),         # tmin clamps to 0 < near0
    "origin-on-face-in": ((-0.5, 0.125, 0.25), (1, 0.25, 0.125)),      # tmin = 0 exactly
    "origin-on-face-out": ((0.5, 0.125, 0.25), (1, 0.25, 0.125)),      # tmax = 0: 0 > 0 fails, a miss
    "box-behind": ((2, 0.0625, 0.0625), (1, 0.125, 0.125)),
    "box-between": ((-0.8125, 0.125, 0.0625), (1, 0.0625, 0.03125)),   # [0.3125, 1.3125] inside (0.05, 1.5)
    "box-straddles-short": ((-1.25, 0.125, 0.0625), (1, 0.0625, 0.03125)),    # [0.75, 1.75] around 1.5
    "box-beyond-short": ((-2.5, 0.125, 0.0625), (1, 0.03125, 0.03125)),       # [2, 3] beyond 1.5
    "box-straddles-long": ((-1000, 0.125, 0.0625), (1, 0.0, 0.0)),            # [999.5, 1000.5] around 1000
    "box-beyond-long": ((-1500, 0.125, 0.0625), (1, 0.0, 0.0)),               # [1499.5, 1500.5] beyond 1000
    "far-above-1e10": ((0.125, -0.25, 0.25), (0.0, 0.0, 2.0 ** -36)),         # tmax = 0.25 * 2^36 = 1.7e10 clamps to 1e10
}
FACE_RAYS = ("one-zero-face+0", "one-zero-face-0", "two-zero-face+0", "two-zero-face-0", "two-zero-edge-line")
TIE_RAYS = ("through-edge", "through-corner", "origin-on-face-out")


@functools.lru_cache(maxsize=None)
def planted_unit():
    names = list(PLANTED_UNIT)
    return names, _a32([PLANTED_UNIT[k][0] for k in names]), _a32([PLANTED_UNIT[k][1] for k in names])


@functools.lru_cache(maxsize=None)
def rotated_pool():
    """200 seeded random rays around the rotated box and six aimed at its centre from 0.8, 1.4, 3, 900, 1000.3 and 1500 away
    -> names, o, d"""
    rng = np.random.default_rng(20)
    n = 200
    v = rng.standard_normal((n, 3))
    o = ROT_T + 1.3 * v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.6, 1.4, (n, 1))
    w = rng.standard_normal((n, 3))
    target = ROT_T + 0.75 * w / np.linalg.norm(w, axis=1, keepdims=True) * rng.uniform(0, 1, (n, 1)) ** (1 / 3)
    d = target - o
    d[150:] *= -1                      # a quarter look away
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    axis = np.array([0.48, -0.6, 0.64])
    names = [f"random-{i}" for i in range(n)]
    for dist in (0.8, 1.4, 3.0, 900.0, 1000.3, 1500.0):
        o = np.vstack([o, ROT_T - dist * axis])
        d = np.vstack([d, axis])
        names.append(f"aimed-{dist:g}")
    return names, _a32(o), _a32(d)


def sbins_row(n, kind):
    if kind == "linspace":
        return np.linspace(0.0, 1.0, n + 1, dtype=np.float64).astype(f32)
    rng = np.random.default_rng(n)
    r = np.sort(rng.uniform(0, 1, n + 1)).astype(f32)      # non-uniform, repeated edges allowed, ends inside [0, 1]
    r[0] = 0
    if n > 2:
        r[n // 2] = r[n // 2 - 1]
    return r


def _planes_rays(near0, far0, R):
    """planted (near_r, far_r) pairs, then seeded ordinary ones, R rows in all"""
    planted = [("ordinary", 0.3, 0.9), ("equal", 0.7, 0.7), ("reversed", 0.9, 0.3), ("near-below-near0", near0 / 4, 0.8),
               ("near-zero", 0.0, 0.8), ("far-above-far0", 0.5, 2 * far0), ("near-above-far0", 1.5 * far0, 3 * far0),
               ("both-invalid", 1e10, 1e10)]
    rng = np.random.default_rng(R)
    names, nr, fr = [p[0] for p in planted], [p[1] for p in planted], [p[2] for p in planted]
    while len(names) < R:
        a = rng.uniform(near0, 0.6 * min(far0, 6.0))
        names.append(f"random-{len(names)}"), nr.append(a), fr.append(a + rng.uniform(0.05, 0.4 * min(far0, 6.0)))
    return names[:R], _a32(nr[:R]), _a32(fr[:R])


# name -> (kind, rays, R, n, row, (near0, far0), lin, want_planes); rays: "unit" (planted, unit box), "rot" (rotated box:
# the random pool, the aimed rays, then the planted rays as ordinary ones), "planes"
BOX_CASES = {}
for _lin in (0, 1):
    for _nf, _nfn in ((NF_LONG, "long"), (NF_SHORT, "short")):
        BOX_CASES[f"unit-all-{_nfn}-lin{_lin}"] = ("box", "unit", len(PLANTED_UNIT), 64, "linspace", _nf, _lin, True)
        BOX_CASES[f"rot-all-{_nfn}-lin{_lin}"] = ("box", "rot", 206, 65, "nonuniform", _nf, _lin, True)
        BOX_CASES[f"planes-all-{_nfn}-lin{_lin}"] = ("planes", "planes", 85, 65, "linspace", _nf, _lin, False)
BOX_CASES.update({
    "unit-R1-n1": ("box", "unit", 1, 1, "linspace", NF_SHORT, 0, True),
    "unit-R3-n2": ("box", "unit", 3, 2, "nonuniform", NF_SHORT, 1, False),
    "unit-R4-n63": ("box", "unit", 4, 63, "nonuniform", NF_LONG, 0, True),
    "unit-R5-n256": ("box", "unit", 5, 256, "linspace", NF_LONG, 0, False),
    "rot-R257-n64": ("box", "rot", 257, 64, "nonuniform", NF_SHORT, 0, False),
    "rot-R257-n65": ("box", "rot", 257, 65, "linspace", NF_LONG, 1, True),
    "rot-R5-n1": ("box", "rot", 5, 1, "linspace", NF_LONG, 0, True),
    "planes-R1-n2": ("planes", "planes", 1, 2, "linspace", NF_SHORT, 0, False),
    "planes-R3-n63": ("planes", "planes", 3, 63, "nonuniform", NF_LONG, 0, False),
    "planes-R4-n64": ("planes", "planes", 4, 64, "linspace", NF_SHORT, 1, False),
    "planes-R5-n1": ("planes", "planes", 5, 1, "linspace", NF_LONG, 1, False),
    "planes-R257-n256": ("planes", "planes", 257, 256, "nonuniform", NF_SHORT, 0, False),
})


@functools.lru_cache(maxsize=None)
def box_case(name):
    kind, rays, R, n, rowkind, (near0, far0), lin, want = BOX_CASES[name]
    c = SimpleNamespace(name=name, kind=kind, R=R, n=n, near0=near0, far0=far0, lin=lin, want_planes=want, row=sbins_row(n, rowkind),
                        o=None, d=None, w2b=None, half=None, nears=None, fars=None)
    if kind == "planes":
        c.ray_names, c.nears, c.fars = _planes_rays(near0, far0, R)
        return c
    un, uo, ud = planted_unit()
    if rays == "unit":
        c.w2b, c.half = IDENTITY_W2B, UNIT_HALF
        # a short case starts at the rays that reach its edges: R = 1 a 0 / 0 ray, R = 3 ... 5 follow the list
        first = {1: un.index("one-zero-face+0"), 3: un.index("two-zero-face+0"), 4: un.index("through-edge"), 5: un.index("origin-inside")}.get(R, 0)
        sl = slice(first, first + R)
        c.ray_names, c.o, c.d = un[sl], uo[sl].copy(), ud[sl].copy()
    else:
        rn, ro, rd = rotated_pool()
        c.w2b, c.half = ROT_W2B, ROT_HALF
        names, o, d = rn + un, np.vstack([ro, uo]), np.vstack([rd, ud])
        if R == 5:
            pick = [rn.index(k) for k in ("aimed-0.8", "aimed-1.4", "aimed-3", "aimed-1500", "random-0")]
        else:
            pick = [i % len(names) for i in range(R)]
        c.ray_names, c.o, c.d = [names[i] for i in pick], o[pick].copy(), d[pick].copy()
    assert len(c.ray_names) == R == c.o.shape[0]
    return c


def check_margins(c):
    """every ray of a box case is a hit or a miss by more than twice its bounds, or a planted exact tie / face ray that
    chain32 decides as the reference does"""
    if c.kind == "planes":
        return
    p = planes_reference(c.o, c.d, c.w2b, c.half)
    n32, f32_ = planes_chain32(c.o, c.d, c.w2b, c.half)
    for i, k in enumerate(c.ray_names):
        if not p.clear[i]:
            assert c.w2b is IDENTITY_W2B and k in TIE_RAYS + FACE_RAYS, f"{c.name}: ray {k} is within its bounds of a tie"
            assert not p.hit[i] and n32[i] == INVALID and f32_[i] == INVALID, f"{c.name}: tie {k} is not a miss on both sides"


# ====================================================================================================================== rays
def _undistort32(u, v, lens):
    """raygen_undistort on float32 arrays -> x, y, closed (the gate refused at least one step)"""
    k1, k2, k3, k4, p1, p2 = (f32(t) for t in lens)
    one, two, three, four, six = (f32(t) for t in (1, 2, 3, 4, 6))
    xd, yd = u, v
    x, y = xd.copy(), yd.copy()
    closed = np.zeros(x.shape, bool)
    with np.errstate(all="ignore"):
        for _ in range(UNDISTORT_ITERATIONS):
            r = x * x + y * y
            d = one + r * (k1 + r * (k2 + r * (k3 + r * k4)))
            fx = ((d * x + ((two * p1) * x) * y) + p2 * (r + (two * x) * x)) - xd
            fy = ((d * y + ((two * p2) * x) * y) + p1 * (r + (two * y) * y)) - yd
            d_r = k1 + r * (two * k2 + r * (three * k3 + (r * four) * k4))
            d_x = (two * x) * d_r
            d_y = (two * y) * d_r
            fx_x = ((d + d_x * x) + (two * p1) * y) + (six * p2) * x
            fx_y = (d_y * x + (two * p1) * x) + (two * p2) * y
            fy_x = (d_x * y + (two * p2) * y) + (two * p1) * x
            fy_y = ((d + d_y * y) + (two * p2) * x) + (six * p1) * y
            den = fy_x * fx_y - fx_x * fy_y
            xn = fx * fy_y - fy * fx_y
            yn = fy * fx_x - fx * fy_x
            ok = np.abs(den) > UNDISTORT_EPS
            closed |= ~ok
            x = x + np.where(ok, xn / den, f32(0))
            y = y + np.where(ok, yn / den, f32(0))
    assert x.dtype == f32 and y.dtype == f32
    return x, y, closed


def _forward64(x, y, lens):
    """the forward OPENCV model and its Jacobian in float64 -> xd, yd, (fx_x, fx_y, fy_x, fy_y), (d, r)"""
    k1, k2, k3, k4, p1, p2 = (float(f32(t)) for t in lens)
    r = x * x + y * y
    d = 1 + r * (k1 + r * (k2 + r * (k3 + r * k4)))
    xd = d * x + 2 * p1 * x * y + p2 * (r + 2 * x * x)
    yd = d * y + 2 * p2 * x * y + p1 * (r + 2 * y * y)
    d_r = k1 + r * (2 * k2 + r * (3 * k3 + r * 4 * k4))
    d_x, d_y = 2 * x * d_r, 2 * y * d_r
    J = (d + d_x * x + 2 * p1 * y + 6 * p2 * x, d_y * x + 2 * p1 * x + 2 * p2 * y,
         d_x * y + 2 * p2 * y + 2 * p1 * x, d + d_y * y + 2 * p2 * x + 6 * p1 * y)
    return xd, yd, J, (d, r)


def _newton64(xd, yd, x, y, lens, steps, track=None):
    with np.errstate(all="ignore"):
        for it in range(steps):
            fx, fy, (a, b, c, e), _ = _forward64(x, y, lens)
            fx, fy = fx - xd, fy - yd
            det = a * e - b * c
            if track is not None and it < UNDISTORT_ITERATIONS:
                track["mindet"] = np.minimum(track["mindet"], np.abs(det))
            ok = np.abs(det) > float(UNDISTORT_EPS)
            x = x + np.where(ok, (-fx * e + fy * b) / det, 0.0)
            y = y + np.where(ok, (-fy * a + fx * c) / det, 0.0)
            if track is not None and it == UNDISTORT_ITERATIONS - 1:
                track["ten"] = (x.copy(), y.copy())
    return x, y


def undistort_reference(u, v, lens):
    """float64 roots of the forward model for float32 targets (u, v) -> SimpleNamespace(x, y, dx, dy, residual, regular)
    x, y: Newton continued from the distorted point; where that has not converged, the first of a fan of other starts
    that does.  regular: the recurrence itself is within 1e-9 of that root after ten steps and never met |det J| < DET_MIN."""
    xd, yd = u.astype(np.float64), v.astype(np.float64)
    track = {"mindet": np.full(xd.shape, np.inf)}
    x, y = _newton64(xd, yd, xd.copy(), yd.copy(), lens, 200, track)

    def res(x, y):
        with np.errstate(all="ignore"):
            fx, fy, _, _ = _forward64(x, y, lens)
            return np.nan_to_num(np.hypot(fx - xd, fy - yd), nan=np.inf)
    own = res(x, y) <= 1e-13
    for s in (-3.0, -2.5, -2.0, -1.5, -1.0, 1.5, 0.5, 0.25, 0.0, -4.0, -6.0):
        bad = res(x, y) > 1e-13
        if not bad.any():
            break
        rad = np.hypot(xd, yd)
        x2, y2 = _newton64(xd, yd, s * xd / np.maximum(rad, 1e-30), s * yd / np.maximum(rad, 1e-30), lens, 200)
        take = bad & (res(x2, y2) <= 1e-13)
        x, y = np.where(take, x2, x), np.where(take, y2, y)
    tx, ty = track["ten"]
    with np.errstate(all="ignore"):
        trunc = np.nan_to_num(np.hypot(tx - x, ty - y), nan=np.inf)
        _, _, (a, b, c, e), (d, r) = _forward64(x, y, lens)
        det = a * e - b * c
        k1, k2, k3, k4, p1, p2 = (abs(float(f32(t))) for t in lens)
        A = r * (k1 + r * (k2 + r * (k3 + r * k4)))
        d_d = U * (np.abs(d) + 16 * A)
        d_fx = np.abs(x) * d_d + 6 * U * (np.abs(d * x) + 2 * p1 * np.abs(x * y) + p2 * (r + 2 * x * x) + np.abs(xd))
        d_fy = np.abs(y) * d_d + 6 * U * (np.abs(d * y) + 2 * p2 * np.abs(x * y) + p1 * (r + 2 * y * y) + np.abs(yd))
        dx = 2 * (np.abs(e) * d_fx + np.abs(b) * d_fy) / np.abs(det) + 2 * U * np.abs(x) + trunc
        dy = 2 * (np.abs(c) * d_fx + np.abs(a) * d_fy) / np.abs(det) + 2 * U * np.abs(y) + trunc
    regular = own & (trunc <= 1e-9) & (track["mindet"] >= DET_MIN)
    return SimpleNamespace(x=x, y=y, dx=dx, dy=dy, residual=res(x, y), regular=regular)


def pixel_coords32(c, g=None):
    """raygen_one's four image-plane coordinates of pixels g (default: the whole frame) -> u0, v0, u1, v2 float32"""
    g = np.arange(c.H * c.W, dtype=np.int64) if g is None else g
    y, x = (g // c.W).astype(f32) + f32(0.5), (g % c.W).astype(f32) + f32(0.5)
    fx, fy, cx, cy = f32(c.fx), f32(c.fy), f32(c.cx), f32(c.cy)
    return (x - cx) / fx, -(y - cy) / fy, (x - cx + f32(1)) / fx, -(y - cy + f32(1)) / fy


def distorted(c):
    return c.camera_type != EQUIRECTANGULAR and c.lens is not None and any(f32(t) != 0 for t in c.lens)


def angles32(c, u, v):
    """the bit-defined part of raygen_dir up to the arguments of sinf / cosf -> (u, v after the lens, theta, phi | None, closed)"""
    closed = np.zeros(u.shape, bool)
    if distorted(c):
        u, v, closed = _undistort32(u, v, c.lens)
    theta = phi = None
    with np.errstate(all="ignore"):
        if c.camera_type == FISHEYE:
            theta = np.fmin(np.fmax(np.sqrt(u * u + v * v), f32(0)), PI32)
        elif c.camera_type == EQUIRECTANGULAR:
            theta, phi = -PI32 * u, PI32 * (f32(0.5) - v)
    return u, v, theta, phi, closed


def _rotate32(c, cxd, cyd, czd):
    R = c.R9
    with np.errstate(all="ignore"):
        x = (cxd * R[0] + cyd * R[1]) + czd * R[2]
        y = (cxd * R[3] + cyd * R[4]) + czd * R[5]
        z = (cxd * R[6] + cyd * R[7]) + czd * R[8]
        n = np.fmax(np.sqrt((x * x + y * y) + z * z), f32(1e-7))
        out = np.stack([x / n, y / n, z / n], -1)
    assert out.dtype == f32
    return out


def _dir32(c, u, v):
    u, v, theta, phi, closed = angles32(c, u, v)
    czd = np.full(u.shape, -1, f32)
    with np.errstate(all="ignore"):
        if c.camera_type == FISHEYE:
            st = np.sin(theta)
            cxd, cyd, czd = u * st / theta, v * st / theta, -np.cos(theta)
        elif c.camera_type == EQUIRECTANGULAR:
            cxd, cyd, czd = -np.sin(theta) * np.sin(phi), np.cos(phi), -np.cos(theta) * np.sin(phi)
        elif c.camera_type == ORTHOPHOTO:
            cxd, cyd = np.zeros_like(u), np.zeros_like(u)
        else:
            cxd, cyd = u, v
    return _rotate32(c, cxd.astype(f32), cyd.astype(f32), czd.astype(f32)), closed


def _area32(d0, d1, d2):
    with np.errstate(all="ignore"):
        e, f = d0 - d1, d0 - d2
        dxn = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        dyn = np.sqrt((f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2])
        return dxn * dyn


@functools.lru_cache(maxsize=None)
def rays_chain32(name):
    """the whole frame of RAY_CASES[name] -> SimpleNamespace(o [HW,3], d [HW,3], pa [HW], closed [HW] bool), float32"""
    c = ray_case(name)
    u0, v0, u1, v2 = pixel_coords32(c)
    d0, c0 = _dir32(c, u0, v0)
    d1, c1 = _dir32(c, u1, v0)
    d2, c2 = _dir32(c, u0, v2)
    R, T = c.R9, c.T3
    if c.camera_type == ORTHOPHOTO:
        o = np.stack([(u0 * R[0] + v0 * R[1]) + T[0], (u0 * R[3] + v0 * R[4]) + T[1], (u0 * R[6] + v0 * R[7]) + T[2]], -1)
    else:
        o = np.broadcast_to(T, (c.H * c.W, 3)).copy()
    out = SimpleNamespace(o=o.astype(f32), d=d0, pa=_area32(d0, d1, d2), closed=c0 | c1 | c2, closed_centre=c0)
    assert out.o.dtype == f32 and out.d.dtype == f32 and out.pa.dtype == f32
    return out


def _dir64(c, cam, d_cam):
    """rotation, clamped norm and division in float64 with the bound of the fp32 list: cam, d_cam: three arrays each"""
    R = c.R9.astype(np.float64)
    xs, dxs = [], []
    for r in range(3):
        terms = [cam[k] * R[3 * r + k] for k in range(3)]
        s, err = _dot_err(terms)
        if c.camera_type == PERSPECTIVE:         # czd = -1: the third product is exact
            err = err - U * np.abs(terms[2])
        xs.append(s), dxs.append(err + sum(abs(R[3 * r + k]) * d_cam[k] for k in range(3)))
    q = xs[0] ** 2 + xs[1] ** 2 + xs[2] ** 2
    d_q = sum(2 * np.abs(x) * dx for x, dx in zip(xs, dxs)) + 3 * U * q
    n = np.maximum(np.sqrt(q), float(f32(1e-7)))
    d_n = d_q / (2 * n) + U * n
    d = np.stack([x / n for x in xs], -1)
    bd = np.stack([dx / n + np.abs(x) * d_n / (n * n) + U * np.abs(x / n) for x, dx in zip(xs, dxs)], -1)
    return d, bd


def _cam64(c, u32, v32):
    """camera-frame direction in float64 and its fp32 bound for float32 coordinates (before the lens) -> cam, d_cam, undefined"""
    z = np.zeros(u32.shape)
    undefined = np.zeros(u32.shape, bool)
    if c.camera_type in (FISHEYE, EQUIRECTANGULAR):
        u, v, theta, phi, _ = angles32(c, u32, v32)
        u, v, theta = u.astype(np.float64), v.astype(np.float64), theta.astype(np.float64)
        with np.errstate(all="ignore"):
            if c.camera_type == FISHEYE:
                st, ct = np.sin(theta), np.cos(theta)
                cam = [u * st / theta, v * st / theta, -ct]
                d_st = U * np.abs(st)
                d_cam = [np.abs(u / theta) * d_st + 2 * U * np.abs(cam[0]), np.abs(v / theta) * d_st + 2 * U * np.abs(cam[1]), U * np.abs(ct)]
            else:
                phi = phi.astype(np.float64)
                st, ct, sp, cp = np.sin(theta), np.cos(theta), np.sin(phi), np.cos(phi)
                cam = [-st * sp, cp, -ct * sp]
                d_cam = [2 * U * np.abs(st * sp) + U * np.abs(st * sp), U * np.abs(cp), 2 * U * np.abs(ct * sp) + U * np.abs(ct * sp)]
        return cam, d_cam, undefined
    if c.camera_type == ORTHOPHOTO:
        return [z, z, z - 1.0], [z, z, z], undefined
    if distorted(c):
        s = undistort_reference(u32, v32, c.lens)
        return [s.x, s.y, z - 1.0], [s.dx, s.dy, z], ~s.regular
    return [u32.astype(np.float64), v32.astype(np.float64), z - 1.0], [z, z, z], undefined


@functools.lru_cache(maxsize=None)
def rays_reference(name):
    """float64 rays of the whole frame and the fp32 list's bounds -> SimpleNamespace(o, d, pa, b_o, b_d, b_pa, undefined [HW]
    (no float64 statement on d and pa: module docstring), undefined_pa)"""
    c = ray_case(name)
    u0, v0, u1, v2 = pixel_coords32(c)
    ds, bs, und = [], [], []
    for u, v in ((u0, v0), (u1, v0), (u0, v2)):
        cam, d_cam, undefined = _cam64(c, u, v)
        with np.errstate(all="ignore"):
            d, bd = _dir64(c, cam, d_cam)
        ds.append(d), bs.append(bd), und.append(undefined)
    with np.errstate(all="ignore"):
        es = [ds[0] - ds[k] for k in (1, 2)]
        d_es = [bs[0] + bs[k] + U * np.abs(e) for k, e in zip((1, 2), es)]
        ln = [np.sqrt((e * e).sum(-1)) for e in es]
        d_ln = [np.sqrt((de * de).sum(-1)) + 2.5 * U * l for de, l in zip(d_es, ln)]
        pa = ln[0] * ln[1]
        b_pa = ln[0] * d_ln[1] + ln[1] * d_ln[0] + d_ln[0] * d_ln[1] + U * pa
    R, T = c.R9.astype(np.float64), c.T3.astype(np.float64)
    if c.camera_type == ORTHOPHOTO:
        uu, vv = u0.astype(np.float64), v0.astype(np.float64)
        o = np.stack([uu * R[3 * r] + vv * R[3 * r + 1] + T[r] for r in range(3)], -1)
        b_o = np.stack([_dot_err([uu * R[3 * r], vv * R[3 * r + 1], T[r] + 0 * uu])[1] for r in range(3)], -1)
    else:
        o, b_o = np.broadcast_to(T, (c.H * c.W, 3)).copy(), np.zeros((c.H * c.W, 3))
    k = FACTOR if c.camera_type in (FISHEYE, EQUIRECTANGULAR) else 1.0
    return SimpleNamespace(o=o, d=ds[0], pa=pa, b_o=b_o, b_d=bs[0] * k, b_pa=b_pa * k, unscaled=(bs[0], b_pa),
                           undefined=und[0], undefined_pa=und[0] | und[1] | und[2])


def hold_rays(name, o, d, pa, rows=None, scaled=True):
    """worst error / bound of float32 rays (rows `rows` of the frame) against rays_reference(name), the undefined pixels
    left out of d and pa; asserts <= 1 when `scaled`, else returns the ratio under the bound without FACTOR"""
    r = rays_reference(name)
    rows = slice(None) if rows is None else rows
    ok, ok_pa = ~r.undefined[rows], ~r.undefined_pa[rows]
    b_d, b_pa = (r.b_d, r.b_pa) if scaled else r.unscaled
    rs = [ratio(o, r.o[rows], r.b_o[rows]), ratio(d[ok], r.d[rows][ok], b_d[rows][ok])]
    if pa is not None:
        rs.append(ratio(np.asarray(pa).reshape(-1)[ok_pa], r.pa[rows][ok_pa], b_pa[rows][ok_pa]))
    if scaled:
        assert max(rs) <= 1.0, f"{name}: worst error / bound {max(rs):.3f} (origins, directions, pixel_area: {rs})"
    return max(rs)


def orbit_c2w(theta, radius=0.6, height=0.15):
    """synthetic.orbit_c2w: 3x4 camera-to-world on a circle, looking at the origin"""
    eye = np.array([radius * np.cos(theta), radius * np.sin(theta), height])
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    return _a32(np.stack([right, np.cross(right, fwd), -fwd, eye], axis=1))


def _pose(kind):
    if kind == "identity":
        return _a32([[1, 0, 0, 0.25], [0, 1, 0, -0.5], [0, 0, 1, 2]])
    if kind == "zero":
        return _a32([[0, 0, 0, 0.25], [0, 0, 0, -0.5], [0, 0, 0, 2]])
    return orbit_c2w(float(kind))


# name -> (camera_type, H, W, fx, fy, cx, cy, pose, lens)
RAY_CASES = {
    "p-1x1": (PERSPECTIVE, 1, 1, 1.3, 1.1, 0.4, 0.7, 1.1, None),
    "p-1x300": (PERSPECTIVE, 1, 300, 170.0, 165.0, 149.3, 0.4, 1.1, None),
    "p-300x1": (PERSPECTIVE, 300, 1, 170.0, 165.0, 0.4, 150.7, 0.4, None),
    "p-24x40-off": (PERSPECTIVE, 24, 40, 23.2, 22.8, 19.3, 12.4, 1.1, None),
    "p-24x40-centre-identity": (PERSPECTIVE, 24, 40, 23.2, 22.8, 20.5, 12.5, "identity", None),
    "p-17x31": (PERSPECTIVE, 17, 31, 21.0, 22.0, 15.2, 8.4, 1.3, None),
    "p-17x31-fx1e5": (PERSPECTIVE, 17, 31, 1e5, 1e5, 15.2, 8.4, 1.3, None),
    "p-17x31-fx1e5-identity": (PERSPECTIVE, 17, 31, 1e5, 0.9e5, 15.5, 8.5, "identity", None),
    "p-17x31-zero-rotation": (PERSPECTIVE, 17, 31, 21.0, 22.0, 15.2, 8.4, "zero", None),
    "p-17x31-six-zeros": (PERSPECTIVE, 17, 31, 21.0, 22.0, 15.2, 8.4, 1.3, (0.0,) * 6),
    "p-24x40-lens0": (PERSPECTIVE, 24, 40, 23.2, 22.8, 19.3, 12.4, 1.1, LENSES[0]),
    "p-24x40-lens1": (PERSPECTIVE, 24, 40, 23.2, 22.8, 19.3, 12.4, 1.1, LENSES[1]),
    "p-24x40-lens2": (PERSPECTIVE, 24, 40, 23.2, 22.8, 19.3, 12.4, 1.1, LENSES[2]),
    "p-24x40-lens3": (PERSPECTIVE, 24, 40, 23.2, 22.8, 19.3, 12.4, "identity", LENSES[3]),
    "p-17x31-lens2": (PERSPECTIVE, 17, 31, 18.0, 17.5, 15.5, 8.5, 1.3, LENSES[2]),
    "p-24x40-strong": (PERSPECTIVE, 24, 40, 16.0, 16.0, 19.3, 12.4, 1.1, STRONG),
    "f-17x31-clip": (FISHEYE, 17, 31, 4.0, 4.5, 15.5, 8.5, 1.3, None),             # the principal-point pixel; |(u, v)| to 4.3 > pi
    "f-17x31-clip-lens": (FISHEYE, 17, 31, 4.0, 4.5, 15.5, 8.5, 1.3, FISHEYE_LENS),
    "f-17x31-off": (FISHEYE, 17, 31, 21.0, 22.0, 15.2, 8.4, "identity", None),
    "f-24x40-lens": (FISHEYE, 24, 40, 21.0, 22.0, 19.3, 12.4, 1.1, FISHEYE_LENS),
    "e-8x16-north": (EQUIRECTANGULAR, 8, 16, 8.0, 8.0, 7.5, 4.5, 1.3, None),       # row 0: phi = 0; column 15: theta = -pi
    "e-8x16-south": (EQUIRECTANGULAR, 8, 16, 8.0, 8.0, 8.5, 3.5, "identity", None),   # row 7: phi = pi; column 0: theta = pi
    "e-8x16-lens": (EQUIRECTANGULAR, 8, 16, 8.0, 8.0, 7.5, 4.5, 1.3, LENSES[0]),
    "o-17x31": (ORTHOPHOTO, 17, 31, 21.0, 22.0, 15.2, 8.4, 1.3, None),
    "o-17x31-lens": (ORTHOPHOTO, 17, 31, 21.0, 22.0, 15.2, 8.4, 1.3, LENSES[2]),
}
MILD_LENS_CASES = ("p-24x40-lens0", "p-24x40-lens1", "p-24x40-lens2", "p-24x40-lens3", "p-17x31-lens2")
# ray_start, count (None: to the end of the frame) per frame size; every slice must equal those rows of the whole frame
RANGES = {
    (1, 1): [(0, 1)],
    (1, 300): [(0, 255), (0, 256), (0, 257), (43, 257), (299, 1), (0, 300)],
    (300, 1): [(0, 1), (44, 256), (299, 1), (0, 300)],
    (24, 40): [(0, 960), (57, 255), (57, 256), (57, 257), (959, 1), (640, 320)],
    (17, 31): [(0, 527), (40, 1), (40, 256), (270, 257), (526, 1)],
    (8, 16): [(0, 128), (5, 1), (127, 1)],
}


@functools.lru_cache(maxsize=None)
def ray_case(name):
    t, H, W, fx, fy, cx, cy, pose, lens = RAY_CASES[name]
    c2w = _pose(pose)
    c = SimpleNamespace(name=name, camera_type=t, H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy, lens=lens, c2w=c2w,
                        R9=np.ascontiguousarray(c2w[:, :3]).reshape(-1), T3=np.ascontiguousarray(c2w[:, 3]))
    return c


def lens_free(name):
    """the same camera without its lens parameters"""
    c = ray_case(name)
    twin = SimpleNamespace(**vars(c))
    twin.lens = None
    return twin


# views: name -> (camera_type, H, W, [ray case names or (name, overrides)]): every view is a camera of RAY_CASES re-framed to
# H x W, so that a view's rows are unerf_generate_rays on that camera
def _views16():
    names = ["p-24x40-strong", "p-24x40-off", "p-24x40-lens0", "p-17x31", "p-24x40-lens2", "p-17x31-six-zeros", "p-17x31-fx1e5",
             "p-24x40-lens1", "p-24x40-centre-identity", "p-17x31-zero-rotation", "p-24x40-lens3", "p-1x300", "p-17x31-lens2",
             "p-300x1", "p-1x1", "p-17x31-fx1e5-identity"]
    return names


VIEW_CASES = {
    "v1-255": (PERSPECTIVE, 15, 17, ["p-24x40-lens2"]),
    "v2-255-strong-first": (PERSPECTIVE, 15, 17, ["p-24x40-strong", "p-24x40-off"]),
    "v2-256": (PERSPECTIVE, 16, 16, ["p-24x40-off", "p-24x40-lens0"]),
    "v2-257": (PERSPECTIVE, 1, 257, ["p-24x40-lens1", "p-17x31"]),
    "v16-257": (PERSPECTIVE, 257, 1, _views16()),
    "v16-960": (PERSPECTIVE, 24, 40, _views16()),
    "v2-fisheye-255": (FISHEYE, 15, 17, ["f-17x31-clip", "f-17x31-clip-lens"]),
    "v2-equirect-257": (EQUIRECTANGULAR, 1, 257, ["e-8x16-north", "e-8x16-lens"]),
    "v2-ortho-256": (ORTHOPHOTO, 16, 16, ["o-17x31-lens", "o-17x31"]),
}


def view_cameras(name):
    """-> camera_type, H, W, [SimpleNamespace camera per view] (the named ray case with the view case's frame size; a frame
    smaller than the case's keeps its intrinsics, so the strong lens still closes its gate)"""
    t, H, W, names = VIEW_CASES[name]
    cams = []
    for k in names:
        c = SimpleNamespace(**vars(ray_case(k)))
        assert c.camera_type == t
        c.H, c.W, c.name = H, W, f"{name}/{k}"
        cams.append(c)
    return t, H, W, cams


def camera_chain32(c):
    """rays_chain32 for a camera record that is not in RAY_CASES (a view)"""
    u0, v0, u1, v2 = pixel_coords32(c)
    d0, c0 = _dir32(c, u0, v0)
    d1, _ = _dir32(c, u1, v0)
    d2, _ = _dir32(c, u0, v2)
    R, T = c.R9, c.T3
    if c.camera_type == ORTHOPHOTO:
        o = np.stack([(u0 * R[0] + v0 * R[1]) + T[0], (u0 * R[3] + v0 * R[4]) + T[1], (u0 * R[6] + v0 * R[7]) + T[2]], -1)
    else:
        o = np.broadcast_to(T, (c.H * c.W, 3)).copy()
    return SimpleNamespace(o=o.astype(f32), d=d0, pa=_area32(d0, d1, d2), closed=c0)


# ================================================================================================================== coverage
def check_coverage():
    """the properties the cases were placed for; a later edit of the cases cannot silently drop an edge"""
    # ---- box: every planted ray is what its name says, under the launch planes it was planted for
    un, uo, ud = planted_unit()
    p = planes_reference(uo, ud, IDENTITY_W2B, UNIT_HALF)
    n32, f32_ = planes_chain32(uo, ud, IDENTITY_W2B, UNIT_HALF)
    un32, uf32 = planes_upstream32(uo, ud, IDENTITY_W2B, UNIT_HALF)
    at = {k: i for i, k in enumerate(un)}
    zero = lambda k: sum(1 for t in PLANTED_UNIT[k][1] if t == 0)
    assert {zero(k) for k in un if k.startswith("one-zero")} == {1} and {zero(k) for k in un if k.startswith("two-zero")} == {2}
    for stem in ("one-zero", "two-zero"):
        signs = {np.signbit(f32(t)) for k in un if k.startswith(stem) for t in PLANTED_UNIT[k][1] if t == 0}
        assert signs == {True, False}, f"{stem}: both +0 and -0 components"
        for where in ("inside", "outside", "face"):
            assert any(k.startswith(f"{stem}-{where}") for k in un)
    for k in un:
        i = at[k]
        if "inside" in k and "zero" in k:
            assert p.hit[i] and p.clear[i] and abs(n32[i] - p.nears[i]) < 1e-6 and abs(f32_[i] - p.fars[i]) < 1e-6, k
            assert not k.startswith("two-zero") or (n32[i], f32_[i]) == (1.5, 2.5), k
        if "outside" in k:
            assert not p.hit[i] and p.clear[i] and n32[i] == INVALID, k
    for k in FACE_RAYS:      # 0 / 0: finite here (a miss), NaN planes upstream
        i = at[k]
        assert np.isfinite(n32[i]) and np.isfinite(f32_[i]) and n32[i] == INVALID and f32_[i] == INVALID, k
        assert np.isnan(un32[i]) and np.isnan(uf32[i]), f"{k}: upstream's amin / amax must propagate the NaN"
        assert not p.hit[i]
    assert all(np.isfinite(un32[at[k]]) for k in un if k not in FACE_RAYS), "only the face rays differ from upstream"
    for k in TIE_RAYS:
        lo, hi = p.raw[0][at[k]], p.raw[1][at[k]]
        assert not p.hit[at[k]] and n32[at[k]] == INVALID and (hi == lo or max(hi, 0.0) == max(lo, 0.0)), k
    assert p.raw[0][at["origin-inside"]] < 0 and p.hit[at["origin-inside"]] and p.nears[at["origin-inside"]] == 0
    assert p.nears[at["origin-on-face-in"]] == 0 and p.hit[at["origin-on-face-in"]] and p.raw[0][at["origin-on-face-in"]] == 0
    assert p.raw[1][at["box-behind"]] < 0 and not p.hit[at["box-behind"]]
    assert p.raw[1][at["far-above-1e10"]] > 1e10 and p.fars[at["far-above-1e10"]] == 1e10 and p.hit[at["far-above-1e10"]]
    for (near0, far0), tag in ((NF_SHORT, "short"), (NF_LONG, "long")):
        i = at["box-between"]
        assert near0 < p.nears[i] < p.fars[i] < far0
        i = at[f"box-straddles-{tag}"]
        assert near0 < p.nears[i] < far0 < p.fars[i], tag
        i = at[f"box-beyond-{tag}"]
        assert far0 < p.nears[i] < p.fars[i], tag
        c = box_case(f"unit-all-{tag}-lin0")
        b = box_chain32(c)[2]
        assert np.all(b[i] == b[i, 0]), "a box beyond far0: all bins equal"
        assert b[at["origin-inside"], 0] < 0, "an origin inside the box: the first bin lies below near0"
    # ---- box: the random rays
    rn, ro, rd = rotated_pool()
    pr = planes_reference(ro, rd, ROT_W2B, ROT_HALF)
    share = pr.hit[:200].mean()
    assert 0.2 <= share <= 0.9 and abs(share - HIT_SHARE) < 0.0026, f"{share:.3f} of the random rays hit"
    assert len(rn) == 206 and pr.hit[200:].all()
    assert pr.fars[rn.index("aimed-0.8")] < 1.5 < pr.nears[rn.index("aimed-3")] and pr.nears[rn.index("aimed-1.4")] < 1.5 < pr.fars[rn.index("aimed-1.4")]
    assert pr.nears[rn.index("aimed-1000.3")] < 1000 < pr.fars[rn.index("aimed-1000.3")] and pr.nears[rn.index("aimed-1500")] > 1000
    # ---- box: shapes
    cs = [box_case(k) for k in BOX_CASES]
    for kind in ("box", "planes"):
        mine = [c for c in cs if c.kind == kind]
        assert {1, 3, 4, 5, 257} <= {c.R for c in mine} and {1, 2, 63, 64, 65, 256} <= {c.n for c in mine}, kind
        assert {c.lin for c in mine} == {0, 1} and {(c.near0, c.far0) for c in mine} == {NF_LONG, NF_SHORT}
    assert {c.want_planes for c in cs if c.kind == "box"} == {True, False}
    assert any(np.array_equal(c.row, sbins_row(c.n, "linspace")) for c in cs) and any(np.any(np.diff(np.diff(c.row)) != 0) and c.n > 2 for c in cs)
    for c in cs:
        assert c.row.min() >= 0 and c.row.max() <= 1
        check_margins(c)
    c = box_case("planes-all-short-lin0")
    want = {"ordinary": lambda a, b: c.near0 < a < b < c.far0, "equal": lambda a, b: a == b, "reversed": lambda a, b: a > b,
            "near-below-near0": lambda a, b: 0 < a < c.near0, "near-zero": lambda a, b: a == 0, "far-above-far0": lambda a, b: a < c.far0 < b,
            "near-above-far0": lambda a, b: c.far0 < a, "both-invalid": lambda a, b: a == b == INVALID}
    for k, fn in want.items():
        i = c.ray_names.index(k)
        assert fn(float(c.nears[i]), float(c.fars[i])), k
    for k in BOX_CASES:
        if BOX_CASES[k][0] == "planes" and BOX_CASES[k][2] >= 8:
            assert set(want) <= set(box_case(k).ray_names)
    # ---- rays
    frames = {(ray_case(k).H, ray_case(k).W) for k in RAY_CASES}
    assert {(1, 1), (1, 300), (300, 1), (24, 40), (17, 31), (8, 16)} <= frames and frames <= set(RANGES)
    for (H, W), rs in RANGES.items():
        assert all(0 <= a and a + n <= H * W and n >= 1 for a, n in rs) and (0, H * W) in rs and (H * W - 1, 1) in rs
    counts = {n for rs in RANGES.values() for _, n in rs}
    assert {1, 255, 256, 257} <= counts and any(a % W for (H, W), rs in RANGES.items() for a, n in rs if W > 1)
    c = ray_case("p-24x40-centre-identity")
    u0, v0, _, _ = pixel_coords32(c)
    assert np.any((u0 == 0) & (v0 == 0)), "a principal point on a pixel centre"
    assert not np.any((pixel_coords32(ray_case("p-24x40-off"))[0] == 0)) and any(ray_case(k).fx != ray_case(k).fy for k in RAY_CASES)
    assert not ray_case("p-17x31-zero-rotation").R9.any() and np.all(rays_chain32("p-17x31-zero-rotation").d == 0)
    for k in MILD_LENS_CASES:
        assert not rays_chain32(k).closed.any() and not rays_reference(k).undefined_pa.any(), f"{k}: the gate stays open everywhere"
    strong = rays_chain32("p-24x40-strong")
    share = strong.closed_centre.mean()
    assert 0.001 <= share <= 0.05, f"the strong lens closes the gate on {share:.4f} of its pixels"
    r = rays_reference("p-24x40-strong")
    assert not (strong.closed & ~r.undefined_pa).any(), "a closed pixel counts as regular"
    assert 0.2 <= (~r.undefined_pa).mean() <= 0.6, "the regular share of the strong lens"
    # FISHEYE: the principal-point pixel, the clip, with and without k1..k4
    for k in ("f-17x31-clip", "f-17x31-clip-lens"):
        c = ray_case(k)
        u0, v0, _, _ = pixel_coords32(c)
        theta = angles32(c, u0, v0)[2]
        assert np.any((u0 == 0) & (v0 == 0)) and np.any(theta == PI32) and np.hypot(u0, v0).max() > np.pi and np.isfinite(theta).all()
        g = int(np.flatnonzero((u0 == 0) & (v0 == 0))[0])
        ch = rays_chain32(k)
        assert np.isnan(ch.d[g]).all() and np.isnan(ch.pa[g]) and np.isnan(ch.d).any(1).sum() == 1
    for k, row, col in (("e-8x16-north", 0, 15), ("e-8x16-south", 7, 0)):
        c = ray_case(k)
        u0, v0, _, _ = pixel_coords32(c)
        _, _, theta, phi, _ = angles32(c, u0, v0)
        phi, theta = phi.reshape(8, 16), theta.reshape(8, 16)
        assert np.all(phi[row] == (0 if row == 0 else PI32)) and np.all(np.abs(theta[:, col]) == PI32), k
    assert distorted(ray_case("o-17x31-lens")) and not distorted(ray_case("e-8x16-lens")) and not distorted(ray_case("p-17x31-six-zeros"))
    # ---- views
    assert {len(v[3]) for v in VIEW_CASES.values()} == {1, 2, 16} and {v[1] * v[2] for v in VIEW_CASES.values()} == {255, 256, 257, 960}
    for k in ("v16-257", "v16-960"):
        cams = view_cameras(k)[3]
        flags = [distorted(c) for c in cams]
        assert True in flags and False in flags and flags[0] and not flags[1] and cams[0].lens == STRONG
        for f in ("fx", "cx", "cy"):
            assert len({getattr(c, f) for c in cams}) > 4
        assert len({c.c2w.tobytes() for c in cams}) > 4 and len({c.lens for c in cams}) > 4
    assert view_cameras("v2-255-strong-first")[3][0].lens == STRONG and camera_chain32(view_cameras("v2-255-strong-first")[3][0]).closed.any()
