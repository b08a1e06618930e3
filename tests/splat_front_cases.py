"""Hand-placed cases for the front half of the splat frame (plain module: tests import it; nothing here needs a GPU).

csrc/unerf_splat.hip: project_kernel (unerf_splat_project, _raw, _batch), sh_colors_kernel in its six instantiations and the
tight-list geometry (tile_bbox, tight_splat, tight_row, tight_count), which is inlined in the projection's count and again in
map_intersects_kernel's emission.

Camera: identity rotation, fx = fy = 32, principal point on half-integers.  A planted splat sits at depth TZ = 32, where
tz + 1e-6 == tz in fp32 and 1 / tz is a power of two: u = tx + cx and v = ty + cy EXACTLY, so a dyadic mean puts the centre on a
tile border, makes u - r exactly 0, and so on.  Isotropic planted scales are found by a search over the fp32 oracle so that the
radius is the integer the plant asks for (`_scale_for_radius`).  Every plant records the edge it sits on and what the exact
(rational) arithmetic expects there; tests/test_splat_front_cases_cpu.py checks both on the fp32 oracle.

Sizes: N in (1, 3, 255, 256, 257, 515) -- N % 4 in (1, 3, 3, 0, 1, 3), last workgroup of 1, 3, 255, 256, 1, 3 rows.  Images
96 x 80, 37 x 50 and 5 x 50 (W x H), and ONE strip of 21 x 280 for the tall splats: 17 tile rows at block_width 16 need 257 rows
of pixels, so that strip keeps the size limit in pixels (5,880 < 96 x 80), not in height.  block_width in (16, 8, 5).

Float64 reference (`project_ref`, `shade_ref`): written from the formulas of the EWA projection and of the shading, with the RAW
prologue (exp of the log-scales, division by the quaternion norm, sigmoid of the logit [x compensation]).  It is evaluated in a
running-error arithmetic (class E): every value carries a bound on |fp32 result - float64 value| formed from float64 magnitudes
alone.  One operation adds u |result| (u = 2^-24; 4 u for expf / log1pf, whose documented error is 1 - 2 ulp) plus 2^-126 (an
fp32 result in the subnormal range, or flushed), and passes its operands' bounds on through the partial derivatives, second
order included -- unrolled this is gamma_k sum |term| with k the operations behind the output, as composite_cases.py forms its
bounds, but per element and with the conditioning of a cancelling determinant in it.  Nothing in a bound comes from a kernel.

Discrete outputs (visible or not, radius, tile box, num_tiles_hit) are compared with the reference on the rows where the
reference's own margin is wide: |tz - clip|, |det|, the distance of 3 sqrt(lambda) to an integer and of each box edge to an
integer all exceed TWICE the bound of that quantity.  `kept` marks them.  The share of random-fill rows left out is capped at
MAX_EXCLUDED; the CPU test asserts it for every case, and a case's seed (SEEDS) is changed when the reference alone misses it.
Planted rows sit ON their edges, so they are mostly left out here -- and never out of the bit-exact comparison with the fp32
oracle (unerf_splat_project), which covers every finite row.

Decisions pinned here:
  * a radius beyond 2^31: (int)radius saturates on the GPU (v_cvt_i32_f32), as the CUDA cast of gsplat does; the fp32 oracle and
    this reference saturate too (plant "radius beyond 2^31").
  * floor instead of truncation in tile_bbox: an EQUIVALENT mutant.  Both box ends pass through max(0, .), and floor and
    truncation differ only on (-1, 0), where both clamp to 0.  The plant "box starts in (-1, 0)" is there, and the CPU test asserts
    the equivalence on every case instead of claiming to catch it.
  * a mean equal to the camera position at degree >= 1: the view direction is 0 / 0; the kernel's fmaxf(NaN + 0.5, 0) gives 0,
    torch.clamp(min=0) of the reference model gives NaN.  Such a splat has tz = 0 and is always culled (radii == 0, pinned by
    the plant "mean on the camera"), so its colour reaches no pixel; the colour the kernels write is 0 and the tests pin it.
  * non-finite rows: "centre non-finite" means a NaN anywhere in the mean or an Inf in x or y; those rows have
    num_tiles_hit == 0 ((int)NaN is 0 and both box ends of an Inf centre clamp to the same side).  A mean at z = +Inf meets
    Inf x 0 in the clamped ratio and ends the same way; the tests hold it to the in-range property only."""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import splat_oracle as SO

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
FLOOR = 2.0 ** -126
LIB = 4 * U                    # expf / log1pf of the device library: documented at 1 - 2 ulp
CLIP = float(f32(0.01))
FX = 32.0
TZ = 32.0
BWS = (16, 8, 5)
NS = (1, 3, 255, 256, 257, 515)
MAX_EXCLUDED = 0.05
WIDE = 2.0                     # a margin is wide when it exceeds WIDE x the bound of the quantity
INT_MAX = 2 ** 31 - 1
V_ID = np.eye(4, dtype=f32)[:3]
IDQ = f32([1, 0, 0, 0])
SEEDS = {}                     # (case name, bw) -> seed; default 0


def camera(H, W):
    return SimpleNamespace(fx=FX, fy=FX, cx=W // 2 + 0.5, cy=H // 2 + 0.5, H=H, W=W)


def tiles_of(H, W, bw):
    return (W + bw - 1) // bw, (H + bw - 1) // bw


# ------------------------------------------------------------------ running-error arithmetic ------------------------------
class E:
    """float64 value v with a bound e on |fp32 evaluation - v|"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v, self.e = np.broadcast_arrays(np.asarray(v, f64), np.asarray(e, f64))

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E(float(f32(x)) if np.isscalar(x) else x)

    @staticmethod
    def rnd(v, e, u=U):
        return E(v, e + u * np.abs(v) + FLOOR)

    def __add__(a, b):
        b = E.of(b)
        return E.rnd(a.v + b.v, a.e + b.e)

    __radd__ = __add__

    def __sub__(a, b):
        b = E.of(b)
        return E.rnd(a.v - b.v, a.e + b.e)

    def __rsub__(a, b):
        return E.of(b) - a

    def __mul__(a, b):
        b = E.of(b)
        return E.rnd(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e)

    __rmul__ = __mul__

    def __truediv__(a, b):
        b = E.of(b)
        v = a.v / b.v
        d = np.abs(b.v) - b.e
        return E.rnd(v, np.where(d > 0, (a.e + np.abs(v) * b.e) / np.where(d > 0, d, 1.0), np.inf))

    def __rtruediv__(a, b):
        return E.of(b) / a

    def __neg__(a):
        return E(-a.v, a.e)

    def __getitem__(a, k):
        return E(a.v[k], a.e[k])


def esqrt(a):
    return E.rnd(np.sqrt(a.v), np.sqrt(a.v + a.e) - np.sqrt(np.maximum(a.v - a.e, 0.0)))


def eexp(a):
    v = np.exp(a.v)
    return E.rnd(v, v * np.expm1(a.e), LIB)


def elog1p(a):
    d = 1.0 + a.v - a.e
    return E.rnd(np.log1p(a.v), np.where(d > 0, a.e / np.where(d > 0, d, 1.0), np.inf), LIB)


def emax(a, b):
    a, b = E.of(a), E.of(b)
    return E(np.maximum(a.v, b.v), np.maximum(a.e, b.e))      # (1-Lipschitz in each argument)


def emin(a, b):
    a, b = E.of(a), E.of(b)
    return E(np.minimum(a.v, b.v), np.maximum(a.e, b.e))


def esigmoid(x):
    return 1.0 / (1.0 + eexp(-E.of(x)))


def estack(items, axis=-1):
    return E(np.stack([i.v for i in items], axis), np.stack([i.e for i in items], axis))


def _col(a, k):
    return E(np.asarray(a, f32)[:, k].astype(f64))


# ------------------------------------------------------------------ numpy restatements + planted mutations ----------------
def visible_np(tz, clip=CLIP, mutate=None):
    """the near-plane test: a splat with tz <= clip is culled (`lt`: tz < clip)"""
    return ~(tz < f32(clip)) if mutate == "lt" else ~(tz <= f32(clip))


def tile_bbox_np(u, v, radius, bw, H, W, mutate=None):
    """tile_bbox of csrc/unerf_splat.hip in fp32 numpy.  mutate: "floor" (floor for truncation), "no_plus1" (x1 / y1 without the
    + 1), "tbx_floor" (tile counts without rounding up)"""
    u, v, radius = (np.asarray(a, f32) for a in (u, v, radius))
    tbx, tby = (W // bw, H // bw) if mutate == "tbx_floor" else tiles_of(H, W, bw)
    one = f32(0) if mutate == "no_plus1" else f32(1)
    with np.errstate(all="ignore"):
        tcx, tcy, tr = u / f32(bw), v / f32(bw), radius / f32(bw)

        def ti(a):      # (int): truncation, NaN -> 0, saturating
            a = np.nan_to_num(a.astype(f64), nan=0.0, posinf=2.0 ** 31, neginf=-2.0 ** 31)
            a = np.floor(a) if mutate == "floor" else np.trunc(a)
            return np.clip(a, -2.0 ** 31, INT_MAX).astype(np.int64)
        x0 = np.minimum(np.maximum(0, ti(tcx - tr)), tbx)
        x1 = np.minimum(np.maximum(0, ti(tcx + tr + one)), tbx)
        y0 = np.minimum(np.maximum(0, ti(tcy - tr)), tby)
        y1 = np.minimum(np.maximum(0, ti(tcy + tr + one)), tby)
    return x0, y0, x1, y1


def stage_copy_map(nb, mutate=None):
    """the STAGE copy of a workgroup with nb rows as an index map: s_rest[j] = rest[b0 * 45 + map[j]], -1 where LDS keeps
    what it held.  float4 body over nb * 45 // 4 quads, scalar tail behind it (`no_tail`: the tail loop dropped)"""
    m = np.full(256 * 45, -1, np.int64)
    nq4 = nb * 45 // 4
    for tid in range(256):
        for q in range(tid, nq4, 256):
            m[4 * q:4 * q + 4] = np.arange(4 * q, 4 * q + 4)
        if mutate != "no_tail":
            for r in range(nq4 * 4 + tid, nb * 45, 256):
                m[r] = r
    return m


def quads_read(degree, layout):
    """-> floats of the coefficient row that the kernel's 16-byte loads fetch.  layout "unpacked": the 48-float row [dc, rest];
    "split": the 45-float features_rest row (dc is three scalar loads)"""
    if layout == "unpacked":
        return 4 * (1 if degree <= 0 else 3 if degree == 1 else 7 if degree == 2 else 12)
    nq = 0 if degree <= 0 else 3 if degree == 1 else 6 if degree == 2 else 11
    return 4 * nq + (1 if degree >= 3 else 0)


def floats_used(degree, layout, mutate=None):
    """-> floats of the row that may reach a colour: the 3 (degree + 1)^2 of the SH basis (`extra_quad`: one 16-byte quad more)"""
    n = 3 * (max(degree, 0) + 1) ** 2 - (3 if layout == "split" else 0)
    return n + 4 if mutate == "extra_quad" else n


def shade_np(degree, means, cam_pos, dc, rest, layout="split", mutate=None):
    """colours from the floats `floats_used` lets through (the others read as 0), through the fp32 oracle's full basis"""
    N = len(means)
    row = np.concatenate([dc.reshape(N, 3), rest.reshape(N, 45)], 1) if layout == "unpacked" else rest.reshape(N, 45).copy()
    row[:, floats_used(degree, layout, mutate):] = 0
    k = row if layout == "unpacked" else np.concatenate([dc.reshape(N, 3), row], 1)
    with np.errstate(all="ignore"):
        col = SO.spherical_harmonics(3 if degree >= 1 else 0, means - f32(cam_pos), k.reshape(N, 16, 3))
        return np.maximum(col + f32(0.5), f32(0))


MUTATIONS = ("lt", "floor", "no_plus1", "no_tail", "extra_quad_1", "extra_quad_2", "tbx_floor")
EQUIVALENT = ("floor",)     # see the module docstring


def tight_count_np(xys, conics, opac, box, bw):
    """tight_splat / tight_row / tight_count restated in float64 on the fp32 xys, conics and opacities.
    -> (count [N], sure [N], totals: list per splat of the emission's per-round totals (rounds of 8 tile rows)).  `sure`: no
    row end of the splat lies within 0.02 tile of an integer and no gate is near, so the kernel's fast-math evaluation (rcp,
    sqrt, log at ~1 ulp) gives the same count."""
    x0, y0, x1, y1 = (np.asarray(b, np.int64) for b in box)
    N = len(opac)
    cnt, sure, totals = np.zeros(N, np.int64), np.ones(N, bool), [[] for _ in range(N)]
    X, Y, A, B, Cc, O = (a.astype(f64) for a in (xys[:, 0], xys[:, 1], conics[:, 0], conics[:, 1], conics[:, 2], opac))
    for i in range(N):
        w, nrows = x1[i] - x0[i], y1[i] - y0[i]
        if w <= 0 or nrows <= 0:
            continue
        op, a, b, c = O[i], A[i], B[i], Cc[i]
        widths = np.full(nrows, w)
        if not (op >= float(f32(0.0039))):
            if op == op:
                widths[:] = 0
            sure[i] = op != op or abs(op - 0.0039) > 1e-6
        else:
            det = a * c - b * b
            ok = det > 0 and a > 0 and c > 0
            if ok:
                two_tau = 2.0 * (np.log(255.0 * op) * float(f32(1.01)) + float(f32(0.01)))
                hx, k = np.sqrt(two_tau * c / det), two_tau * a
                hy, ry = np.sqrt(k / det), -(b / c) * np.sqrt(two_tau * c / det)
                pad = max(hx, hy) * float(f32(0.01)) + float(f32(0.05))
                ok = all(np.isfinite([hx, hy, ry, 1.0 / a]))
            if not ok:
                sure[i] = False       # (keeps the box: decided by fp32 signs this restatement does not model)
            else:
                for r in range(nrows):
                    ty = y0[i] + r
                    d0, d1 = (ty * bw + 0.5) - Y[i] - pad, (ty * bw + (bw - 0.5)) - Y[i] + pad
                    if d0 > hy or d1 < -hy:
                        sure[i] &= min(abs(d0 - hy), abs(d1 + hy)) > 1e-3
                        widths[r] = 0
                        continue
                    sure[i] &= min(abs(d0 - hy), abs(d1 + hy)) > 1e-3
                    d0, d1 = max(d0, -hy), min(d1, hy)
                    dr, dl = min(max(ry, d0), d1), min(max(-ry, d0), d1)
                    sr, sl = np.sqrt(max(k - det * dr * dr, 0.0)), np.sqrt(max(k - det * dl * dl, 0.0))
                    xr, xl = (-b * dr + sr) / a + pad, (-b * dl - sl) / a - pad
                    gl, gr = (X[i] + xl - 0.5) / bw, (X[i] + xr - 0.5) / bw
                    sure[i] &= min(abs(g - np.round(g)) for g in (gl, gr)) > 0.02
                    t0, t1 = max(x0[i], int(np.floor(max(gl, -1e6)))), min(x1[i], int(np.floor(min(gr, 1e6))) + 1)
                    widths[r] = max(t1 - t0, 0)
        cnt[i] = widths.sum()
        totals[i] = [int(widths[r:r + 8].sum()) for r in range(0, nrows, 8)]
    return cnt, sure, totals


def need_pairs(xys, conics, opac, radii, H, W, bw):
    """float64 brute force over pixel centres: need[t, i] -- tile t holds a pixel at which the blend loop would NOT skip splat i
    (sigma >= 0 and alpha = min(0.999, o exp(-sigma)) >= 1/255, a hair more than the loop keeps), inside gsplat's box.
    -> (need [tiles, N] bool, box [tiles, N] bool)"""
    tbx, tby = tiles_of(H, W, bw)
    N = len(opac)
    py, px = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    tile_of = (np.arange(H)[:, None] // bw) * tbx + np.arange(W)[None, :] // bw
    need, box = np.zeros((tbx * tby, N), bool), np.zeros((tbx * tby, N), bool)
    x0, y0, x1, y1 = tile_bbox_np(xys[:, 0], xys[:, 1], radii.astype(f32), bw, H, W)
    with np.errstate(all="ignore"):
        for i in np.nonzero(radii > 0)[0]:
            tt = (np.arange(y0[i], y1[i])[:, None] * tbx + np.arange(x0[i], x1[i])[None, :]).reshape(-1)
            box[tt, i] = True
            dx, dy = f64(xys[i, 0]) - px, f64(xys[i, 1]) - py
            a, b, c = (f64(v) for v in conics[i])
            sigma = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
            alpha = np.minimum(0.999, f64(opac[i]) * np.exp(-sigma))
            hit = (sigma >= 0) & (alpha >= (1.0 / 255.0) * (1 - 1e-4))
            need[np.unique(tile_of[hit]), i] = True
    return need & box, box


# ------------------------------------------------------------------ float64 references -----------------------------------
def project_ref(means, scales, quats, V, cam, bw, raw, logits=None, antialiased=False, glob_scale=1.0, clip=CLIP):
    """EWA projection in float64 with bounds.  raw: `scales` are log-scales, `quats` unnormalised (the RAW prologue).
    -> namespace: xys, depths, conics, compensation, cov3d, opacities (E or None), each already masked as the kernel leaves it
    (zeros where the splat did not get that far); live, visible, radii (saturated), box, tiles (the box's area), kept."""
    V = np.asarray(V, f32).reshape(-1)[:12].reshape(3, 4)
    H, W = cam.H, cam.W
    fx, fy, cx, cy = (E.of(float(x)) for x in (cam.fx, cam.fy, cam.cx, cam.cy))
    with np.errstate(all="ignore"):
        p = [_col(means, k) for k in range(3)]
        vv = lambda r, c: E.of(float(V[r, c]))
        t = [((vv(r, 0) * p[0] + vv(r, 1) * p[1]) + vv(r, 2) * p[2]) + vv(r, 3) for r in range(3)]
        tx, ty, tz = t
        q = [_col(quats, k) for k in range(4)]
        ss = lambda q: ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]
        if raw:
            qn = esqrt(ss(q))
            q = [qk / qn for qk in q]
        qs = 1.0 / esqrt(ss(q))
        w, x, y, z = (qk * qs for qk in q)
        R = [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
             [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
             [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]]
        sc = [_col(scales, k) for k in range(3)]
        if raw:
            sc = [eexp(s) for s in sc]
        s = [E.of(float(glob_scale)) * k for k in sc]
        M = [[R[r][c] * s[c] for c in range(3)] for r in range(3)]
        Sg = [[(M[r][0] * M[c][0] + M[r][1] * M[c][1]) + M[r][2] * M[c][2] for c in range(3)] for r in range(3)]
        cov3d = estack([Sg[0][0], Sg[0][1], Sg[0][2], Sg[1][1], Sg[1][2], Sg[2][2]])
        C3 = [[Sg[min(r, c)][max(r, c)] for c in range(3)] for r in range(3)]
        lim_x, lim_y = 1.3 * (0.5 * E.of(float(W)) / fx), 1.3 * (0.5 * E.of(float(H)) / fy)
        ex = tz * emin(lim_x, emax(-lim_x, tx / tz))
        ey = tz * emin(lim_y, emax(-lim_y, ty / tz))
        rz = 1.0 / tz
        rz2 = rz * rz
        J00, J02, J11, J12 = fx * rz, (-fx * ex) * rz2, fy * rz, (-fy * ey) * rz2
        T0 = [J00 * vv(0, c) + J02 * vv(2, c) for c in range(3)]
        T1 = [J11 * vv(1, c) + J12 * vv(2, c) for c in range(3)]
        TV0 = [(T0[0] * C3[0][c] + T0[1] * C3[1][c]) + T0[2] * C3[2][c] for c in range(3)]
        TV1 = [(T1[0] * C3[0][c] + T1[1] * C3[1][c]) + T1[2] * C3[2][c] for c in range(3)]
        c00 = (TV0[0] * T0[0] + TV0[1] * T0[1]) + TV0[2] * T0[2]
        c01 = (TV0[0] * T1[0] + TV0[1] * T1[1]) + TV0[2] * T1[2]
        c11 = (TV1[0] * T1[0] + TV1[1] * T1[1]) + TV1[2] * T1[2]
        det_orig = c00 * c11 - c01 * c01
        ca, cb, cc = c00 + 0.3, c01, c11 + 0.3
        det = ca * cc - cb * cb
        comp = esqrt(emax(0.0, det_orig / det))
        inv_det = 1.0 / det
        conics = estack([cc * inv_det, (-cb) * inv_det, ca * inv_det])
        bh = 0.5 * (ca + cc)
        sq = esqrt(emax(0.1, bh * bh - det))
        pre = 3.0 * esqrt(emax(bh + sq, bh - sq))
        rw = 1.0 / (tz + 1e-6)
        u, v = (tx * rw) * fx + cx, (ty * rw) * fy + cy
        # ---- decisions and their margins
        live = tz.v > clip
        wide = np.abs(tz.v - clip) > WIDE * tz.e
        det_ok = det.v != 0
        wide_geo = np.abs(det.v) > WIDE * det.e
        rc = np.ceil(pre.v)
        wide_geo &= np.minimum(pre.v - (rc - 1), rc - pre.v) > WIDE * pre.e
        radius = E(np.where(np.isfinite(rc), rc, 0.0))
        tbx, tby = tiles_of(H, W, bw)
        tr = radius / float(bw)
        box = []
        for ctr, n, plus in ((u, tbx, 0), (u, tbx, 1), (v, tby, 0), (v, tby, 1)):
            a = (ctr / float(bw) + tr) + 1.0 if plus else ctr / float(bw) - tr
            ti = lambda z: np.clip(np.trunc(np.nan_to_num(z, nan=0.0, posinf=1e18, neginf=-1e18)), 0, n).astype(np.int64)
            box.append(ti(a.v))
            wide_geo &= (ti(a.v - WIDE * a.e) == ti(a.v + WIDE * a.e)) & np.isfinite(a.v)
        x0, x1, y0, y1 = box
        tiles = (x1 - x0) * (y1 - y0)
        visible = live & det_ok & (tiles > 0)
        kept = wide & (~live | wide_geo)
        m = lambda e, mask: E(np.where(mask.reshape(mask.shape + (1,) * (e.v.ndim - 1)), e.v, 0.0),
                              np.where(mask.reshape(mask.shape + (1,) * (e.v.ndim - 1)), e.e, 0.0))
        out = SimpleNamespace(live=live, visible=visible, kept=kept, box=(x0, y0, x1, y1),
                              tiles=np.where(visible, tiles, 0), pre=pre, tz=tz,
                              radii=np.where(visible, np.minimum(radius.v, INT_MAX), 0).astype(np.int64),
                              xys=m(estack([u, v]), visible), depths=m(tz, visible), conics=m(conics, live & det_ok),
                              compensation=m(comp, visible), cov3d=m(cov3d, live), opacities=None)
        if logits is not None:
            o = esigmoid(E(np.asarray(logits, f32).reshape(-1).astype(f64)))
            out.opacities = m(o * comp, visible) if antialiased else o
    return out


CONTINUOUS = ("xys", "depths", "conics", "compensation", "cov3d")


def within(got, ref, rows=None):
    """-> (ok, worst share of the bound used) of a kernel / oracle array against an E, over `rows` (bool [N]).  NaN rule: an
    element passes as NaN only where the reference is NaN or its bound is not finite."""
    got = np.asarray(got, f64)
    v, e = ref.v, ref.e
    if rows is not None:
        got, v, e = got[rows], v[rows], e[rows]
    with np.errstate(all="ignore"):
        free = ~np.isfinite(e) | np.isnan(v)
        d = np.abs(got - v)
        bad = ~free & ~(d <= e)
        share = np.where(free | (e == 0), 0.0, d / np.where(e > 0, e, 1.0))
        share = np.where(~free & (e == 0) & (d > 0), np.inf, share)
    return not bad.any(), float(share.max()) if share.size else 0.0


SH_C = [float(f32(c)) for c in (SO.SH_C0, SO.SH_C1)]
SH_C2 = [float(f32(c)) for c in SO.SH_C2]
SH_C3 = [float(f32(c)) for c in SO.SH_C3]


def shade_ref(degree, means, cam_pos, dc, rest, log_unc=None, beta_min=0.01, logits=None, comp=None, depths=None):
    """the shaded rows in float64 with bounds: rgb = max(SH + 0.5, 0) (degree -1: sigmoid(dc)), beta = softplus(log_unc) +
    beta_min (threshold 20), depth as given, opacity = sigmoid(logit) [x comp].  rest may be None at degree <= 0.
    -> namespace rgb [N,3], beta [N] | None, opacities [N] | None (E); rows(C) assembles [rgb, (beta), depth]"""
    N = len(means)
    with np.errstate(all="ignore"):
        K = lambda j: E(np.asarray(dc if j == 0 else rest.reshape(N, 15, 3)[:, j - 1], f32).reshape(N, 3).astype(f64))
        if degree < 0:
            rgb = esigmoid(K(0))
        else:
            col = SH_C[0] * K(0)
            if degree >= 1:
                d = [E(np.asarray(means, f32)[:, k:k + 1].astype(f64)) - float(f32(cam_pos[k])) for k in range(3)]
                nrm = esqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                x, y, z = (k / nrm for k in d)
                xx, xy, xz, yy, yz, zz = x * x, x * y, x * z, y * y, y * z, z * z
                col = col + SH_C[1] * (((-y) * K(1) + z * K(2)) - x * K(3))
                if degree >= 2:
                    col = col + ((((SH_C2[0] * xy * K(4) + SH_C2[1] * yz * K(5)) + SH_C2[2] * ((2.0 * zz - xx) - yy) * K(6))
                                  + SH_C2[3] * xz * K(7)) + SH_C2[4] * (xx - yy) * K(8))
                if degree >= 3:
                    col = col + ((((((SH_C3[0] * y * (3.0 * xx - yy) * K(9) + SH_C3[1] * xy * z * K(10))
                                     + SH_C3[2] * y * ((4.0 * zz - xx) - yy) * K(11))
                                    + SH_C3[3] * z * ((2.0 * zz - 3.0 * xx) - 3.0 * yy) * K(12))
                                   + SH_C3[4] * x * ((4.0 * zz - xx) - yy) * K(13)) + SH_C3[5] * z * (xx - yy) * K(14))
                                 + SH_C3[6] * x * (xx - 3.0 * yy) * K(15))
            rgb = emax(col + 0.5, 0.0)
        out = SimpleNamespace(rgb=rgb, beta=None, opacities=None)
        if log_unc is not None:
            lu = E(np.asarray(log_unc, f32).reshape(-1).astype(f64))
            sp = elog1p(eexp(emin(lu, 20.0)))
            big = lu.v > 20.0
            out.beta = E(np.where(big, lu.v, sp.v), np.where(big, 0.0, sp.e)) + float(f32(beta_min))
        if logits is not None:
            o = esigmoid(E(np.asarray(logits, f32).reshape(-1).astype(f64)))
            out.opacities = o * E(np.asarray(comp, f32).astype(f64)) if comp is not None else o
        dcol = None if depths is None else E(np.asarray(depths, f32).reshape(-1, 1).astype(f64))

        def rows(C):
            parts = [out.rgb] + ([E(out.beta.v[:, None], out.beta.e[:, None])] if C == 5 else []) + [dcol]
            return E(np.concatenate([p.v for p in parts], 1), np.concatenate([p.e for p in parts], 1))
        out.rows = rows
    return out


# ------------------------------------------------------------------ plants ------------------------------------------------
def _scale_for_radius(tx, ty, r, cam):
    """isotropic scale of a splat at (tx, ty, TZ), identity quaternion, whose fp32-oracle radius is r.  The radius does not
    depend on the principal point, so the search projects onto the image centre (the oracle reports radii of visible splats)"""
    s = np.linspace(0.02, (r + 1) / 3.0, 4000).astype(f32)
    n = len(s)
    m = np.tile(f32([tx, ty, TZ]), (n, 1))
    o = SO.project_gaussians(m, np.repeat(s[:, None], 3, 1), 1.0, np.tile(IDQ, (n, 1)), V_ID, FX, FX, cam.W / 2 - tx,
                             cam.H / 2 - ty, cam.H, cam.W, 16)
    idx = np.nonzero(o["radii"] == r)[0]
    assert len(idx), (tx, ty, r)
    return s[idx[len(idx) // 2]]


def _plant(edge, mean, scale, quat=IDQ, logit=2.0, log_scale=None, qfac=1.0, **expect):
    scale = np.broadcast_to(f32(scale), (3,)).astype(f32)
    with np.errstate(all="ignore"):
        ls = np.log(scale).astype(f32) if log_scale is None else np.broadcast_to(f32(log_scale), (3,)).astype(f32)
    return SimpleNamespace(edge=edge, mean=f32(mean), scale=scale, log_scale=ls, quat=f32(quat), logit=f32(logit), qfac=f32(qfac),
                           expect=expect)


def _at(cam, bw, edge, u, v, r, **kw):
    """an isotropic splat at depth TZ with centre (u, v) exactly and radius r; expects the exact-arithmetic tile box"""
    tx, ty = u - cam.cx, v - cam.cy
    tbx, tby = tiles_of(cam.H, cam.W, bw)
    cl = lambda a, n: int(min(max(0, int(a)), n))          # int(): truncation toward zero, on exact rationals
    x0, x1 = cl((u - r) / bw, tbx), cl((u + r) / bw + 1, tbx)
    y0, y1 = cl((v - r) / bw, tby), cl((v + r) / bw + 1, tby)
    area = (x1 - x0) * (y1 - y0)
    return _plant(edge, (tx, ty, TZ), _scale_for_radius(tx, ty, r, cam), xys=(u, v), radii=r if area > 0 else 0,
                  num_tiles_hit=area, box=(x0, y0, x1, y1) if area > 0 else None, **kw)


def bbox_plants(cam, bw):
    H, W = cam.H, cam.W
    tbx, tby = tiles_of(H, W, bw)
    r = bw
    P = [_at(cam, bw, "centre on a tile corner, radius a multiple of bw", 2 * bw if W > 2 * bw else 0, bw, r),
         _at(cam, bw, "u - r == 0", bw, 2 * bw, r),
         _at(cam, bw, "box starts in (-1, 0)", bw - 2, bw - 1, r),
         _at(cam, bw, "wholly left: u + r = -1, x1 = 0", -(r + 1), 2 * bw, r),
         _at(cam, bw, "touching the left side: u + r = 0", -r, 2 * bw, r),
         _at(cam, bw, "wholly right: u - r = tbx bw", tbx * bw + r, 2 * bw, r),
         _at(cam, bw, "touching the right side: u - r = tbx bw - 1", tbx * bw - 1 + r, 2 * bw, r),
         _at(cam, bw, "wholly above: v + r = -1", min(2 * bw, W // 2), -(r + 1), r),
         _at(cam, bw, "touching the top: v + r = 0", min(2 * bw, W // 2), -r, r),
         _at(cam, bw, "wholly below: v - r = tby bw", min(2 * bw, W // 2), tby * bw + r, r),
         _at(cam, bw, "touching the bottom: v - r = tby bw - 1", min(2 * bw, W // 2), tby * bw - 1 + r, r),
         _plant("giant: the box is the whole image", (0, 0, TZ), 64.0, num_tiles_hit=tbx * tby)]
    return P


def near_plants(cam, bw):
    c = f32(CLIP)
    s = 1e-3        # pixel sigma 3.2 at tz = 0.01
    return [_plant("tz == clip: culled", (0, 0, c), s, radii=0),
            _plant("tz one ulp above clip: kept", (0, 0, np.nextafter(c, f32(1))), s, visible=True),
            _plant("tz one ulp below clip: culled", (0, 0, np.nextafter(c, f32(0))), s, radii=0),
            _plant("tz == 0: culled", (0, 0, 0), s, radii=0),
            _plant("tz negative: culled", (0.5, 0.25, -1), s, radii=0),
            _plant("mean on the camera: culled", (0, 0, 0), 0.5, radii=0)]


def fov_plants(cam, bw):
    """tz = 1, so tx / tz = tx: on the clamp, one ulp to either side and far beyond, both signs, x and y.  A clamped splat has
    the conics of the splat ON the limit (J depends on the clamped ratio only); `same_conics_as` names that plant's offset"""
    lx = f32(1.3) * (f32(0.5) * f32(cam.W) / f32(FX))
    ly = f32(1.3) * (f32(0.5) * f32(cam.H) / f32(FX))
    P = []
    for sgn in (1, -1):
        for ax, lim in ((0, lx), (1, ly)):
            def mean(val):
                m = [0.0, 0.0, 1.0]
                m[ax] = sgn * val
                return m
            tag = f"{'+' if sgn > 0 else '-'}{'xy'[ax]}"
            P += [_plant(f"fov clamp {tag}: on the limit", mean(lim), 0.25, on_limit=0),
                  _plant(f"fov clamp {tag}: one ulp inside", mean(np.nextafter(lim, f32(0))), 0.25, differs_from=-1),
                  _plant(f"fov clamp {tag}: one ulp beyond", mean(np.nextafter(lim, f32(9))), 0.25, same_conics_as=-2),
                  _plant(f"fov clamp {tag}: far beyond", mean(f32(8) * lim), 0.25, same_conics_as=-3)]
    return P


def _pre32(s):
    """3 sqrt(lambda_max) of the centred isotropic splat at TZ in the kernel's fp32 operations: c00 = c11 = s^2, c01 = 0, so
    bh^2 - det == 0 and the 0.1 floor is taken"""
    s = f32(s)
    ca = s * s + f32(0.3)
    return f32(3) * np.sqrt(ca + np.sqrt(f32(0.1)))


def radius_plants(cam, bw):
    # 3 sqrt(lambda) == 6 exactly, and the nearest scales whose value is below / above 6
    s = f32(np.sqrt(4.0 - 0.3 - np.sqrt(0.1)))
    cand = s
    for _ in range(64):
        if _pre32(cand) == f32(6):
            break
        cand = np.nextafter(cand, f32(0) if _pre32(cand) > 6 else f32(9))
    assert _pre32(cand) == f32(6)
    lo, hi = cand, cand
    while _pre32(lo) == f32(6):
        lo = np.nextafter(lo, f32(0))
    while _pre32(hi) == f32(6):
        hi = np.nextafter(hi, f32(9))
    P = [_plant("3 sqrt(lambda) == 6: radius 6", (0, 0, TZ), cand, radii=6, pre=6.0),
         _plant("3 sqrt(lambda) just below 6: radius 6", (0, 0, TZ), lo, radii=6),
         _plant("3 sqrt(lambda) just above 6: radius 7", (0, 0, TZ), hi, radii=7)]
    # the 45-degree needle: c00 = c11 = c01 up to the dilation, ca cc - cb^2 cancels
    q45 = f32([np.cos(np.pi / 8), 0, 0, np.sin(np.pi / 8)])
    sx = (2.0 ** np.arange(10, 16, 0.01)).astype(f32)
    n = len(sx)
    sc = np.stack([sx, np.full(n, 1e-3, f32), np.full(n, 1e-3, f32)], 1)
    o = SO.project_gaussians(np.tile(f32([0, 0, TZ]), (n, 1)), sc, 1.0, np.tile(q45, (n, 1)), V_ID, FX, FX, cam.cx, cam.cy, cam.H,
                             cam.W, bw)
    zero = np.nonzero((o["conics"] == 0).all(1) & (o["cov3d"] != 0).any(1))[0]
    neg = np.nonzero(o["conics"][:, 0] < 0)[0]
    assert len(zero) and len(neg)
    P += [_plant("45-degree needle: det == 0 in fp32", (0, 0, TZ), sc[zero[0]], q45, det="zero", radii=0),
          _plant("45-degree needle: det < 0 in fp32", (0, 0, TZ), sc[neg[0]], q45, det="negative"),
          _plant("scale exp(-30)", (0.5, -0.25, TZ), f32(np.exp(-30.0)), log_scale=-30.0, radii=3, comp0=True),
          _plant("radius beyond 2^31", (0, 0, TZ), 1e9, radii=INT_MAX),
          _plant("quaternion 1e-3 from unit length (RAW)", (1, 1, TZ), (1.0, 2.0, 0.5), (0.5, 0.5, -0.5, 0.5), qfac=1e-3, visible=True),
          _plant("quaternion 1e3 from unit length (RAW)", (-1, 1, TZ), (1.0, 2.0, 0.5), (0.5, -0.5, 0.5, 0.5), qfac=1e3, visible=True)]
    return P


def nonfinite_plants(cam, bw):
    n, i = np.nan, np.inf
    P = [_plant("NaN mean x", (n, 0, TZ), 1.0, nonfinite="centre"), _plant("NaN mean z", (0, 0, n), 1.0, nonfinite="centre"),
         _plant("+Inf mean x", (i, 0, TZ), 1.0, nonfinite="centre"), _plant("-Inf mean y", (0, -i, TZ), 1.0, nonfinite="centre"),
         _plant("+Inf mean z", (1, 1, i), 1.0, nonfinite="row"), _plant("-Inf mean z", (1, 1, -i), 1.0, nonfinite="row", radii=0),
         _plant("Inf log-scale", (0, 0, TZ), i, log_scale=i, nonfinite="row"),
         _plant("zero quaternion", (0, 0, TZ), 1.0, (0, 0, 0, 0), nonfinite="row"),
         _plant("NaN opacity logit", (0, 0, TZ), 1.0, logit=n, nonfinite="logit")]
    # a finite neighbour between every two of them
    out = []
    for p in P:
        out += [p, _plant("finite neighbour", (0.5, 0.5, TZ), 1.0, visible=True)]
    return out


def _logit(p):
    return np.log(p / (1 - p))


def tight_wide_plants(cam, bw):
    P = [_plant("opacity 0.00385: under the kernel's 0.0039 gate", (0, 0, TZ), 2.0, logit=_logit(0.00385), listed=False),
         _plant("opacity 0.00391: between the gate and 1/255", (1, 0, TZ), 2.0, logit=_logit(0.00391)),
         _plant("opacity 0.00393: above 1/255", (2, 0, TZ), 2.0, logit=_logit(0.00393)),
         _plant("logit 20: the sigmoid rounds to 1", (3, 1, TZ), 2.0, logit=20.0, opacity=1.0),
         _plant("comp == 0 when antialiased: radius 3, no tile", (0.5, -0.25, TZ), f32(np.exp(-30.0)), log_scale=-30.0, comp0=True)]
    # axis-aligned ellipses (sz tiny: cov2d = diag(sx^2, sy^2) + 0.3) tangent to a pixel-centre row / the first pixel-centre
    # column of a tile, to the fp32 rounding of the scale: half-axis h = sqrt(2 tau (s^2 + 0.3)), tau = ln(255 sigmoid(-1))
    tau = np.log(255.0 / (1.0 + np.e))
    s_for = lambda h: f32(np.sqrt(h * h / (2 * tau) - 0.3))
    u0, v0 = 2 * bw, 2 * bw                      # centre on a tile corner
    h = bw + 0.5                                  # reaches the first pixel centre of the tile after next
    P += [_plant("ellipse tangent to a pixel-centre row", (u0 - cam.cx, v0 - cam.cy, TZ), (1.0, s_for(h), 1e-3), logit=-1.0, tangent="row"),
          _plant("ellipse tangent to a tile's first pixel-centre column", (u0 - cam.cx, v0 - cam.cy, TZ), (s_for(h), 1.0, 1e-3), logit=-1.0,
                 tangent="col"),
          _plant("centre on a tile border", (u0 - cam.cx, bw + 3 - cam.cy, TZ), (2.0, 3.0, 1e-3), logit=0.0)]
    return P + _total_plants(cam, bw)


def _total_plants(cam, bw):
    """axis-aligned splats whose whole tight list is ONE emission round (at most 8 tile rows) of 8, 9, 16 and 17 entries, picked
    from seeded candidates by the float64 restatement of the tight rows (only candidates it is `sure` of)"""
    rng = np.random.default_rng([5, bw])
    n = 1500
    xy = np.round(rng.uniform(0, 1, (n, 2)) * [cam.W, cam.H] * 4) / 4 - [cam.cx, cam.cy]
    sc = np.concatenate([rng.uniform(0.1, 1.6, (n, 2)) * bw, np.full((n, 1), 1e-3)], 1).astype(f32)
    lg = np.round(rng.uniform(-1, 3, n) * 8).astype(f32) / 8
    means = np.concatenate([xy, np.full((n, 1), TZ)], 1).astype(f32)
    o = SO.project_gaussians(means, sc, 1.0, np.tile(IDQ, (n, 1)), V_ID, FX, FX, cam.cx, cam.cy, cam.H, cam.W, bw)
    with np.errstate(all="ignore"):
        opac = (f32(1) / (f32(1) + np.exp(-lg))).astype(f32)
    box = tile_bbox_np(o["xys"][:, 0], o["xys"][:, 1], o["radii"].astype(f32), bw, cam.H, cam.W)
    cnt, sure, totals = tight_count_np(o["xys"], o["conics"], opac, box, bw)
    P = []
    for want in (8, 9, 16, 17):
        i = next(i for i in range(n) if sure[i] and o["radii"][i] > 0 and totals[i] == [want])
        P.append(_plant(f"one emission round of {want} entries", means[i], sc[i], logit=lg[i], round_total=want))
    return P


def tight_strip_plants(cam, bw):
    """tall axis-aligned splats whose alpha >= 1/255 ellipse spans k tile rows: even k centred on a tile border with half-height
    (k / 2 - 1 / 2) bw, odd k centred in a tile with half-height (k - 1) / 2 bw -- both ends in the middle of a tile row"""
    tau = np.log(255.0 / (1.0 + np.e))
    P = []
    for k in (8, 9, 16, 17):
        vc, h = (8 * bw, (k / 2 - 0.5) * bw) if k % 2 == 0 else (8 * bw + bw / 2, (k - 1) / 2 * bw)
        P.append(_plant(f"tall splat spanning {k} tile rows", (0, vc - cam.cy, TZ), (0.5, f32(np.sqrt(h * h / (2 * tau) - 0.3)), 1e-3),
                        logit=-1.0, rows=k))
    return P


def one_plants(cam, bw):
    return [_at(cam, bw, "the only splat: centre on a tile corner", bw, bw, bw)]


def three_plants(cam, bw):
    return near_plants(cam, bw)[:3]


# name -> (N, H, W, plants, wants tight run)
CASES = {"one": (1, 50, 37, one_plants), "three": (3, 80, 96, three_plants), "fov": (255, 50, 37, fov_plants),
         "near": (256, 50, 37, near_plants), "bbox37": (257, 50, 37, bbox_plants), "bbox96": (515, 80, 96, bbox_plants),
         "bbox5": (255, 50, 5, bbox_plants), "radius": (257, 80, 96, radius_plants), "nonfinite": (257, 80, 96, nonfinite_plants),
         "tight_wide": (515, 80, 96, tight_wide_plants), "tight_strip": (257, 280, 21, tight_strip_plants)}
PROJ_CASES = tuple(k for k in CASES if k != "nonfinite")
TIGHT_CASES = ("tight_wide", "tight_strip", "bbox37", "one")


def _fill(rng, n, cam):
    """seeded random splats in front of, around and behind the camera: pixel sigma 0.3 .. 8, any orientation"""
    z = np.where(rng.random(n) < 0.1, rng.uniform(-5, 0.5, n), rng.uniform(2, 40, n))
    half = np.array([cam.W / 2 / FX, cam.H / 2 / FX])
    xy = rng.uniform(-1.25, 1.25, (n, 2)) * half * np.abs(z)[:, None]
    means = np.concatenate([xy, z[:, None]], 1).astype(f32)
    s = (np.abs(z) / FX * rng.uniform(0.3, 8, n))[:, None] * rng.uniform(0.2, 1, (n, 3))
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return means, s.astype(f32), q.astype(f32), rng.normal(0, 3, n).astype(f32), rng.uniform(0.25, 3.25, n).astype(f32)


@functools.lru_cache(maxsize=None)
def case(name, bw):
    N, H, W, plants_fn = CASES[name]
    cam = camera(H, W)
    plants = plants_fn(cam, bw)[:N]
    nf = N - len(plants)
    rng = np.random.default_rng([SEEDS.get((name, bw), 0), sum(map(ord, name)), bw])
    means, scales, quats, logits, qfac = _fill(rng, nf, cam)
    cat = lambda a, b, shape: np.concatenate([a, np.array(b, f32).reshape((len(plants),) + shape)], 0)
    c = SimpleNamespace(name=name, bw=bw, N=N, H=H, W=W, cam=cam, plants=plants, first_plant=nf, V=V_ID)
    c.means = cat(means, [p.mean for p in plants], (3,))
    c.scales = cat(scales, [p.scale for p in plants], (3,))
    with np.errstate(all="ignore"):
        c.log_scales = cat(np.log(scales).astype(f32), [p.log_scale for p in plants], (3,))
    c.quats = cat(quats, [p.quat for p in plants], (4,))
    c.raw_quats = (c.quats * cat(qfac, [p.qfac for p in plants], ())[:, None]).astype(f32)
    c.logits = cat(logits, [p.logit for p in plants], ())
    c.row = {p.edge: nf + k for k, p in enumerate(plants)}
    c.is_fill = np.arange(N) < nf
    c.nonfinite = np.array([nf + k for k, p in enumerate(plants) if "nonfinite" in p.expect], np.int64)
    c.finite = ~np.isin(np.arange(N), c.nonfinite)
    c.K = (cam.fx, cam.fy, cam.cx, cam.cy, H, W)
    c.oracle = SO.project_gaussians(c.means, c.scales, 1.0, c.quats, V_ID, *c.K, bw)
    return c


@functools.lru_cache(maxsize=None)
def raw_ref(name, bw, antialiased=False):
    c = case(name, bw)
    return project_ref(c.means, c.log_scales, c.raw_quats, c.V, c.cam, bw, True, c.logits, antialiased)


@functools.lru_cache(maxsize=None)
def plain_ref(name, bw):
    c = case(name, bw)
    return project_ref(c.means, c.scales, c.quats, c.V, c.cam, bw, False)


def batch_cameras(B):
    """B view matrices: the identity camera, two dyadic translations and one 1024 units in front of every splat (it culls
    everything), cycled"""
    shift = lambda x, y, z: np.concatenate([np.eye(3, dtype=f32), f32([[x], [y], [z]])], 1)
    base = [V_ID, shift(0.5, -0.25, 1.0), shift(0.0, 0.0, -1024.0), shift(-1.0, 0.5, -0.5)]
    return [base[v % 4] for v in range(B)]


def excluded_share(c, ref):
    fill = c.is_fill
    return float((~ref.kept[fill]).mean()) if fill.any() else 0.0


# ------------------------------------------------------------------ shading cases -----------------------------------------
SH_CAM = f32([0.25, -0.5, 1.0])


@functools.lru_cache(maxsize=None)
def shade_case(N):
    """N splats around SH_CAM.  Planted (from the last row backwards, as far as N allows): a mean on the camera, log-uncertainties
    +-40 and on both sides of the softplus switch at 20, opacity logits +-100 and 0"""
    rng = np.random.default_rng([11, N])
    c = SimpleNamespace(N=N, cam_pos=SH_CAM)
    c.means = (SH_CAM + rng.normal(0, 2, (N, 3))).astype(f32)
    c.dc = rng.normal(0, 1, (N, 3)).astype(f32)
    c.rest = rng.normal(0, 0.5, (N, 15, 3)).astype(f32)
    c.log_unc = rng.normal(-2, 3, N).astype(f32)
    c.logits = rng.normal(0, 3, N).astype(f32)
    c.comp = rng.uniform(0, 1, N).astype(f32)
    c.depths = rng.uniform(0.1, 40, N).astype(f32)
    t = f32(20)
    lus = [40, -40, t, np.nextafter(t, f32(99)), np.nextafter(t, f32(0)), 19.5, 20.5]
    los = [100, -100, 0, 20, -20, 1, -1]
    for k in range(min(N, 7)):
        c.log_unc[N - 1 - k], c.logits[N - 1 - k] = lus[k], los[k]
    c.on_camera = None
    if N >= 3:
        c.on_camera = N - 2
        c.means[c.on_camera] = SH_CAM
    return c


def poisoned(c, degree):
    """-> (dc, rest | None, unpacked [N,16,3]) with every coefficient the degree does not use set to NaN; features_rest is None
    at degree <= 0"""
    used = (max(degree, 0) + 1) ** 2
    un = np.concatenate([c.dc[:, None, :], c.rest], 1).copy()
    un[:, used:] = np.nan
    rest = None if degree <= 0 else np.ascontiguousarray(un[:, 1:])
    return c.dc, rest, np.ascontiguousarray(un)
