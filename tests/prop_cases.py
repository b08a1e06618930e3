"""Hand-placed cases for the proposal density kernels (plain module: tests import it; nothing here needs a GPU).

prop_density_kernel<L, HID> and prop_patch_kernel<L, HID> (csrc/unerf_nerf.hip, section 3) turn a ray and a row of bin edges
into n densities: unerf_s2e on both edges, the mid-point o + d * t / 2, unerf_normalize_position (scene contraction or scene
box, then the selector), L levels of a grid (torch hash table, its dense x-paired copy, tcnn layout with fp32 or half rows),
Linear - ReLU - Linear (or one Linear when HID = 0) and avg * exp(o) * sel.  The cases plant samples on the lattice nodes and
cell faces, on the contraction's |x| = 1 switch, on the selector's borders and in the last cell of every (dense) level, and
run all six (L, HID) pairs over every layout, both normalisations, both spacings, the three kinds of bin rows, n in
{1, 2, 3, 4, 5, 7, 8, 13, 16, 256} and the patch geometries of check_coverage().

Reference.  The library is built with -ffp-contract=off and hipcc rounds fp32 divisions correctly by default, so everything
up to the normalised position is a fixed list of IEEE fp32 operations (unerf_s2e, o + d * t / 2,
unerf_normalize_position, the selector; near / far pass through unerf_spacing_of on the host, the same operations).
`positions32` restates that list in numpy float32: P32 and sel.  No step before P32 was found that is not bit-defined, so no
allowance is made for one.  `reference` evaluates everything after P32 in float64 AT P32: the trilinear blend of the fp32
table rows with the reference's own corners (ceil and floor of the exact product p * scale, not the kernel's floor + 1), the
layers, avg * exp(o) * sel.  For half-row tcnn grids every rounding of the features is specified and they are taken from
O.tcnn_hash_encode_half.  The trilinear interpolant is continuous across cell faces and the ReLU is continuous, so the
float64 value at P32 has no ties: no sample is exempt.

Bounds, per sample, forward and in float64 on absolute values (U = 2^-24; nothing here comes from a GPU result):
  * a level's feature: LERP_UNITS U max|corner| for the roundings of the blend -- torch layout: 1 - o, two products and the
    sum per lerp, 4 U, and a corner passes through three of the seven lerps (x, y, z) with weights that sum to one: 12;
    tcnn layout: three complements and two products per corner weight, 5 U, and eight accumulating fma, 8 U: 13 -- plus, per
    axis, U |scaled coordinate| (max corner - min corner) for the fp32 rounding of p * scale (of fma(scale, p, 0.5)), a bound
    on the interpolant's slope along that axis; a rounding never leaves the closed cell, and the interpolant is continuous
    on its faces.  Half rows: 0.
  * the hidden pre-activation a_j: sum_k |W0_jk| dfeat_k + 2L U (|b0_j| + sum_k |W0_jk feat_k|); the ReLU is 1-Lipschitz.
  * o: sum_j |w1_j| da_j + HID U (|b1| + sum_j |w1_j| relu(a_j)); HID = 0: sum_k |w1_k| dfeat_k + 2L U (|b1| + sum |w1 f|).
  * density, relative: do + (|o| + 1) 2^-23 (DESIGN.md's allowance for __expf) + 2 U (the two final products).
One constant, FACTOR, multiplies the whole: 4 x the worst error / bound of `chain32` -- the same chain in fp32 on the CPU, the
kernel's operation order with a correctly rounded exp -- against the float64 reference over all cases (RATIO_MEASURED; the
4 x is the margin pdf_cases.py gives EPS_CDF, for the device exponential and another summation order).
test_prop_cases_cpu.py re-measures it.  Outputs with sel = 0 must be exactly 0.

Out of reach at test size: the R * n >= 2^31 addressing branch of prop_density_kernel (a.small = 0) needs 8 GiB of output."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from oracle import nerf_oracle as O

f32 = np.float32
U = 2.0 ** -24
AVG = 0.01
NF_LONG, NF_SHORT = (0.05, 1000.0), (0.05, 1.5)
WIDE_EXTRA = 3
P1, P2 = 2654435761, 805459861
LERP_UNITS = {"torch": 12.0, "tcnn32": 13.0, "tcnn16": 0.0}
# worst error / unscaled bound of chain32 over all cases, measured on the CPU (fp32 chain against float64, never a kernel),
# and 4 x it rounded up
RATIO_MEASURED = 0.229
FACTOR = 0.92
O_MAX = 20.0
# seeds per case name (default 0): changed when a random P32 coordinate falls on a selector border
SEEDS = {}


# ---------------------------------------------------------------------------------------------------------------- nets
def _linear(rng, out_dim, in_dim, gain=1.0):
    k = 1.0 / np.sqrt(in_dim)
    return (rng.uniform(-k, k, (out_dim, in_dim)) * gain).astype(f32), (rng.uniform(-k, k, out_dim) * gain).astype(f32)


@functools.lru_cache(maxsize=None)
def net(name):
    """name -> SimpleNamespace(L, H, layout, log2T, scalings | levels, table, w0, b0, w1, b1, aabb, use_dense,
    max_level_bytes, dense / dense_off / dense_dim (torch layout: what ops.build_dense_pairs returns))"""
    L, H, layout, log2T, res, box, dense = NETS[name]
    rng = np.random.default_rng(sorted(NETS).index(name) + 1)
    c = SimpleNamespace(name=name, L=L, H=H, layout=layout, log2T=log2T, aabb=(0.0, 0.0, 0.0, 1.0, 1.0, 1.0) if box else None,
                        levels=None, scalings=None, dense=None, dense_off=(), dense_dim=(), use_dense=True, max_level_bytes=0)
    if layout == "torch":
        c.scalings = O.hash_scalings(L, res[0], res[1]).numpy().astype(f32)
        assert np.all(c.scalings == np.floor(c.scalings)) and np.all(np.diff(c.scalings) > 0)
        c.table = (rng.standard_normal((L << log2T, 2)) * 0.5).astype(f32)
        dims = [int(s) + 1 for s in c.scalings]
        if dense == "none":
            c.use_dense = False
            c.max_level_bytes = 16 * dims[0] ** 3
        elif dense == "some":        # the first two levels fit, the third does not
            c.max_level_bytes = 16 * dims[1] ** 3
        else:
            c.max_level_bytes = 16 * dims[-1] ** 3
        from uncertainty_nerf_gs_amd import ops
        d, offs, dd = ops.build_dense_pairs(torch.from_numpy(c.table), torch.from_numpy(c.scalings), log2T, c.max_level_bytes)
        c.dense, c.dense_off, c.dense_dim = d.numpy(), tuple(offs), tuple(dd)
        want = {"none": 1, "some": 2, "all": L}[dense]
        assert len(offs) == want and 0 < want <= L, (name, len(offs))
        c.n_dense = want if c.use_dense else 0
    else:
        c.levels = O.tcnn_grid_levels(L, res[0], res[1], log2T)
        assert any(lv[4] for lv in c.levels) and not all(lv[4] for lv in c.levels), "dense and hashed tcnn levels"
        rows = c.levels[-1][2] + c.levels[-1][3]
        c.table = (rng.standard_normal((rows, 2)) * 0.5).astype(f32)
        c.n_dense = 0
    if H:
        c.w0, c.b0 = _linear(rng, H, 2 * L)
        c.w1, c.b1 = _linear(rng, 1, H, gain=4.0)
    else:
        c.w0 = c.b0 = None
        c.w1, c.b1 = _linear(rng, 1, 2 * L, gain=4.0)
    return c


# name: (levels, hidden, layout, log2T, (min_res, max_res) | (base_res, per_level_scale), scene box, dense levels)
NETS = {
    "t5h16-hashed": (5, 16, "torch", 8, (4, 40), False, "none"),
    "t5h64-dense2": (5, 64, "torch", 9, (4, 64), False, "some"),
    "t8h16-box-dense8": (8, 16, "torch", 10, (4, 24), True, "all"),
    "t8h64-dense2": (8, 64, "torch", 12, (8, 96), False, "some"),
    "t5h0-box-dense5": (5, 0, "torch", 11, (4, 32), True, "all"),
    "t8h0-hashed": (8, 0, "torch", 8, (8, 64), False, "none"),
    "c5h16-f32": (5, 16, "tcnn32", 10, (5, 1.7), False, None),
    "c8h64-f16": (8, 64, "tcnn16", 12, (5, 1.5), False, None),
    "c5h0-box-f16": (5, 0, "tcnn16", 10, (5, 1.7), True, None),
    "c8h16-box-f32": (8, 16, "tcnn32", 12, (5, 1.5), True, None),
}


def grid_mlp(nt):
    """the net as the oracle's GridMLP (torch tensors)"""
    t = torch.from_numpy
    ws, bs = ([t(nt.w0), t(nt.w1)], [t(nt.b0), t(nt.b1)]) if nt.H else ([t(nt.w1)], [t(nt.b1)])
    return O.GridMLP(table=t(nt.table), scalings=None if nt.scalings is None else t(nt.scalings), log2_T=nt.log2T, weights=ws,
                     biases=bs, tcnn_levels=nt.levels, aabb=None if nt.aabb is None else t(np.array(nt.aabb, f32).reshape(2, 3)),
                     grid_half=nt.layout == "tcnn16")


# ------------------------------------------------------------------------------------------- the fp32 list up to P32
def _spacing_of32(x, lin):
    x = f32(x)
    if lin:
        return x
    return x / f32(2) if x < f32(1) else f32(1) - f32(1) / (f32(2) * x)


def s2e32(b, near, far, lin):
    """unerf_s2e on float32 arrays"""
    sn, sf = _spacing_of32(near, lin), _spacing_of32(far, lin)
    t = b * sf + (f32(1) - b) * sn
    if lin:
        return t
    with np.errstate(divide="ignore"):
        return np.where(t < f32(0.5), f32(2) * t, f32(1) / (f32(2) - f32(2) * t))


def positions32(origins, dirs, sb, n, near, far, lin, aabb, mut=None, want_raw=False):
    """origins, dirs [R,3], sb [n+1] | [R, >= n+1] float32 -> (P32 [R,n,3] float32, sel [R,n] bool): the kernel's operations
    (want_raw: and the position before the selector zeroes the masked ones)"""
    origins, dirs, sb = (np.asarray(a, f32) for a in (origins, dirs, sb))
    rows = sb[None, : n + 1] if sb.ndim == 1 else sb[:, : n + 1]
    e = s2e32(rows, near, far, lin)
    t = (e[:, :-1] + e[:, 1:])[..., None]
    step = dirs[:, None, :] * t
    x = origins[:, None, :] + (step if mut == "no_half" else step / f32(2))
    assert x.dtype == f32 and np.isfinite(x).all(), "finite positions only"
    if aabb is not None:
        lo, hi = np.array(aabb[:3], f32), np.array(aabb[3:], f32)
        p = (x - lo) / (hi - lo)
    else:
        mag = np.max(np.abs(x), axis=-1, keepdims=True)
        far_out = ~(mag <= f32(1.5)) if mut == "mag_le_1p5" else ~(mag < f32(1))
        with np.errstate(divide="ignore", invalid="ignore"):
            contracted = (f32(2) - f32(1) / mag) * (x / mag)
        p = (np.where(far_out, contracted, x) + f32(2)) / f32(4)
    sel = np.all((p >= 0) & (p <= 1), axis=-1) if mut == "inclusive_border" else np.all((p > 0) & (p < 1), axis=-1)
    raw, p = p, p * sel[..., None].astype(f32)
    assert p.dtype == f32
    return (p, sel, raw) if want_raw else (p, sel)


# ------------------------------------------------------------------------------------------------- float64 reference
_CORNER_IS_CEIL = np.array([[ch == "c" for ch in pat] for pat in O._CORNERS])      # [8,3]


def _torch_rows(ix, iy, iz, log2T, level):
    return ((ix ^ (iy * P1) ^ (iz * P2)) & ((1 << log2T) - 1)) + (level << log2T)


def _features64(nt, P):
    """P [N,3] float64 -> feat [N,F L], dfeat [N,F L] (the feature bound); F = nt.F features per row, 2 unless the net says
    otherwise (torch layout only)"""
    N, F = P.shape[0], getattr(nt, "F", 2)
    assert F == 2 or nt.layout == "torch"
    feat, dfeat = np.zeros((N, F * nt.L)), np.zeros((N, F * nt.L))
    if nt.layout == "tcnn16":
        feat[:] = O.tcnn_hash_encode_half(torch.from_numpy(P.astype(f32)), torch.from_numpy(nt.table), nt.levels).numpy()
        return feat, dfeat
    tab = nt.table.astype(np.float64)
    for l in range(nt.L):
        if nt.layout == "torch":
            s = P * float(nt.scalings[l])                         # exact in float64
            fl, ce = np.floor(s).astype(np.int64), np.ceil(s).astype(np.int64)
            o = s - fl
            c = []
            for k in range(8):
                pick = [np.where(_CORNER_IS_CEIL[k, a], ce[:, a], fl[:, a]) for a in range(3)]
                c.append(tab[_torch_rows(*pick, nt.log2T, l)])
            ox, oy, oz = o[:, 0:1], o[:, 1:2], o[:, 2:3]
            f03, f12 = c[0] * ox + c[3] * (1 - ox), c[1] * ox + c[2] * (1 - ox)
            f56, f47 = c[5] * ox + c[6] * (1 - ox), c[4] * ox + c[7] * (1 - ox)
            val = (f03 * oy + f12 * (1 - oy)) * oz + (f47 * oy + f56 * (1 - oy)) * (1 - oz)
            coord = s
        else:
            scale, res, offset, size, dense = nt.levels[l]
            pos = P * float(f32(scale)) + 0.5
            cell = np.floor(pos)
            w, ci = pos - cell, cell.astype(np.int64)
            c, val = [], np.zeros((N, 2))
            for k in range(8):
                cx, cy, cz = ci[:, 0] + (k & 1), ci[:, 1] + ((k >> 1) & 1), ci[:, 2] + ((k >> 2) & 1)
                idx = (cx + cy * res + cz * res * res) % size if dense else \
                    (((cx & 0xFFFFFFFF) ^ ((cy * P1) & 0xFFFFFFFF) ^ ((cz * P2) & 0xFFFFFFFF)) % size)
                c.append(tab[idx + offset])
                wk = np.ones(N)
                for d in range(3):
                    wk = wk * (w[:, d] if (k >> d) & 1 else 1 - w[:, d])
                val = val + wk[:, None] * c[-1]
            coord = pos
        c = np.stack(c)                                            # [8,N,2]
        slope = np.abs(coord).sum(axis=1, keepdims=True) * (c.max(axis=0) - c.min(axis=0))
        feat[:, F * l: F * l + F] = val
        dfeat[:, F * l: F * l + F] = U * (LERP_UNITS[nt.layout] * np.abs(c).max(axis=0) + slope)
    return feat, dfeat


def reference(nt, P32, sel):
    """-> SimpleNamespace(dens [..] float64, o, rel (the UNSCALED relative bound), sel)"""
    shp = sel.shape
    feat, dfeat = _features64(nt, P32.reshape(-1, 3).astype(np.float64))
    K = 2 * nt.L
    w1, b1 = nt.w1.astype(np.float64)[0], float(nt.b1[0])
    if nt.H:
        w0, b0 = nt.w0.astype(np.float64), nt.b0.astype(np.float64)
        a = feat @ w0.T + b0
        da = dfeat @ np.abs(w0).T + K * U * (np.abs(b0) + np.abs(feat) @ np.abs(w0).T)
        h = np.maximum(a, 0)
        o = h @ w1 + b1
        do = da @ np.abs(w1) + nt.H * U * (abs(b1) + h @ np.abs(w1))
    else:
        o = feat @ w1 + b1
        do = dfeat @ np.abs(w1) + K * U * (abs(b1) + np.abs(feat) @ np.abs(w1))
    rel = do + (np.abs(o) + 1) * 2.0 ** -23 + 2 * U
    dens = AVG * np.exp(o) * sel.reshape(-1)
    return SimpleNamespace(dens=dens.reshape(shp), o=o.reshape(shp), rel=rel.reshape(shp), sel=sel)


# ------------------------------------------------------------------------------------------------ fp32 restatement
def _fma32(a, b, c):
    """fl32(a * b + c) for float32 arrays: the product is exact in float64 (one extra rounding of the sum, to float64)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _blend32_torch(c, ox, oy, oz):
    """unerf_blend8<FUSED = true>: each lerp fma(a, o, b * (1 - o))"""
    lerp = lambda a, b, o: _fma32(a, np.broadcast_to(o, a.shape), b * (f32(1) - o))
    f03, f12, f56, f47 = lerp(c[0], c[3], ox), lerp(c[1], c[2], ox), lerp(c[5], c[6], ox), lerp(c[4], c[7], ox)
    return lerp(lerp(f03, f12, oy), lerp(f47, f56, oy), oz)


def _features32(nt, p, mut=None):
    """the kernel's lookup restated: floor + 1 for the ceil corner, the dense copy's own indexing, the fused blend"""
    N = p.shape[0]
    if nt.layout == "tcnn16":
        levels = nt.levels
        if mut == "next_level_offset":
            levels = [lv[:2] + (levels[(i + 1) % nt.L][2],) + lv[3:] for i, lv in enumerate(levels)]
        return O.tcnn_hash_encode_half(torch.from_numpy(p), torch.from_numpy(nt.table), levels).numpy()
    F = getattr(nt, "F", 2)              # features per row: 2 unless the net says otherwise (torch layout, hashed levels)
    assert F == 2 or (nt.layout == "torch" and nt.n_dense == 0)
    feat = np.zeros((N, F * nt.L), f32)
    for l in range(nt.L):
        lo = (l + 1) % nt.L if mut == "next_level_offset" else l
        if nt.layout == "torch":
            s = p * nt.scalings[l]
            fl = s.astype(np.int64)                                # positions are >= 0: truncation is floor
            o = s - fl.astype(f32)
            ce = fl if mut == "ceil_is_floor" else fl + 1
            c = [None] * 8
            if l < nt.n_dense:
                dim, cells = nt.dense_dim[lo], nt.dense[nt.dense_off[lo]:]
                for (ky, kz, a, b) in ((1, 1, 3, 0), (0, 1, 2, 1), (1, 0, 7, 4), (0, 0, 6, 5)):
                    y, z = (ce if ky else fl)[:, 1], (ce if kz else fl)[:, 2]
                    quad = cells[(z * dim + y) * dim + fl[:, 0]]
                    c[a], c[b] = quad[:, 0:2], quad[:, 0:2] if mut == "dense_x1_from_x" else quad[:, 2:4]
            else:
                for k in range(8):
                    pick = [np.where(_CORNER_IS_CEIL[k, a], ce[:, a], fl[:, a]) for a in range(3)]
                    c[k] = nt.table[_torch_rows(*pick, nt.log2T, lo)]
            if mut == "swap_corners":
                c[0], c[1] = c[1], c[0]
            val = _blend32_torch(c, o[:, 0:1], o[:, 1:2], o[:, 2:3])
        else:
            scale, res, _, size, dense = nt.levels[l]
            offset = nt.levels[lo][2]
            half = f32(0.0 if mut == "tcnn_no_half" else 0.5)
            pos = (p.astype(np.float64) * float(f32(scale)) + float(half)).astype(f32)
            cell = np.floor(pos)
            w, ci = pos - cell, cell.astype(np.int64)
            m = f32(1) - w
            wxy = [m[:, 0] * m[:, 1], w[:, 0] * m[:, 1], m[:, 0] * w[:, 1], w[:, 0] * w[:, 1]]
            val = np.zeros((N, 2), f32)
            order = [1, 0, 2, 3, 4, 5, 6, 7] if mut == "swap_corners" else range(8)
            for k, kk in enumerate(order):
                step_x = 0 if mut == "ceil_is_floor" else (kk & 1)
                cx, cy, cz = ci[:, 0] + step_x, ci[:, 1] + ((kk >> 1) & 1), ci[:, 2] + ((kk >> 2) & 1)
                idx = (cx + cy * res + cz * res * res) % size if dense else \
                    (((cx & 0xFFFFFFFF) ^ ((cy * P1) & 0xFFFFFFFF) ^ ((cz * P2) & 0xFFFFFFFF)) % size)
                wk = wxy[k & 3] * (w[:, 2] if k & 4 else m[:, 2])
                val = _fma32(np.broadcast_to(wk[:, None], (N, 2)), nt.table[idx + offset], val)
        feat[:, F * l: F * l + F] = val
    return feat


def chain32(nt, origins, dirs, sb, n, near, far, lin, mut=None):
    """The whole chain in float32 on the CPU, the kernel's operations in the kernel's order (sequential fma over the inputs,
    then over the hidden units), a correctly rounded exp.  mut: one of MUTATIONS.  -> [R,n] float32"""
    p, sel = positions32(origins, dirs, sb, n, near, far, lin, nt.aabb, mut)
    feat = _features32(nt, p.reshape(-1, 3), mut)
    N = feat.shape[0]
    o = np.full(N, nt.b1[0], f32)
    if nt.H:
        h = np.broadcast_to(nt.b0, (N, nt.H)).astype(f32)
        for k in range(2 * nt.L):
            h = _fma32(np.broadcast_to(feat[:, k: k + 1], (N, nt.H)), np.broadcast_to(nt.w0[:, k], (N, nt.H)), h)
        h = np.maximum(h, f32(0))
        for j in range(nt.H - 1 if mut == "skip_last_hidden" else nt.H):
            o = _fma32(h[:, j], np.full(N, nt.w1[0, j], f32), o)
    else:
        for k in range(2 * nt.L):
            o = _fma32(feat[:, k], np.full(N, nt.w1[0, k], f32), o)
    e = np.exp(o.astype(np.float64)).astype(f32)
    return ((f32(AVG) * e) * sel.reshape(-1).astype(f32)).reshape(sel.shape)


# mutation -> which cases it can show on (a predicate on the case)
MUTATIONS = {
    "swap_corners": lambda c: c.net.layout != "tcnn16",
    "ceil_is_floor": lambda c: c.net.layout != "tcnn16",
    "next_level_offset": lambda c: c.net.n_dense == 0,
    "no_half": lambda c: True,
    "mag_le_1p5": lambda c: c.net.aabb is None,
    "inclusive_border": lambda c: c.net.n_dense == 0,         # p = 1 indexes past a dense copy
    "dense_x1_from_x": lambda c: c.net.n_dense > 0,
    "skip_last_hidden": lambda c: c.net.H > 0,
    "tcnn_no_half": lambda c: c.net.layout == "tcnn32",
}


# ------------------------------------------------------------------------------------------------------------- cases
def _first_exact(scale, to_world, contracted):
    """the first k above scale / 2 whose world coordinate the fp32 list maps to a p with fl32(p * scale) = k: a cell face
    in the kernel's arithmetic (and, where k / scale is not dyadic, an ulp off it in the reference's)"""
    for k in range(int(scale) // 2 + 1, int(scale)):
        x = f32(to_world(k / scale))
        p = (x + f32(2)) / f32(4) if contracted else x
        if abs(x) <= 1 and f32(p * f32(scale)) == f32(k):
            return float(x)
    raise AssertionError("no exact lattice coordinate")


def planted_points(nt):
    """[(tag, world point)]: direction 0, origin = the point, so P32 follows from the point alone"""
    e24, e23 = 2.0 ** -24, 2.0 ** -23
    pts = []
    if nt.aabb is None:
        pts.append(("origin", (0.0, 0.0, 0.0)))
        for tag, v in (("below1", 1 - e24), ("at1", 1.0), ("above1", 1 + e23)):
            pts += [(tag, (v, 0.3, -0.2)), (tag, (0.25, -v, 0.6))]
        pts.append(("far", (3e8, 1.0, -1.0)))
        to_world = lambda p: 4.0 * p - 2.0
    else:
        pts += [("p0", (0.0, 0.3, 0.6)), ("p1", (0.3, 1.0, 0.6)), ("eps", (e24, e24, e24)), ("last", (1 - e24,) * 3),
                ("last", (e24, 0.5, 1 - e24)), ("last", (1 - e24, 1 - e24, 0.37))]
        to_world = lambda p: p
    if nt.layout == "torch":
        S0 = float(nt.scalings[0])
        for l in sorted({0, nt.L // 2, nt.L - 1}):        # a face of ONE level: the coordinate k / S_l, dyadic or not
            S = float(nt.scalings[l])
            pt = [0.3, -0.45, 0.55] if nt.aabb is None else [0.37, 0.61, 0.83]
            pt[l % 3] = _first_exact(S, to_world, nt.aabb is None)
            pts.append((f"face{l}", tuple(pt)))
        if nt.aabb is not None:
            pts += [("node0", (1 / S0, 2 / S0, 3 / S0)), ("node0", ((S0 - 1) / S0, 1 / S0, 0.5))]
    elif nt.aabb is not None:                                      # tcnn: a node of level 0 is scale p + 0.5 integer
        s0 = float(f32(nt.levels[0][0]))
        assert s0 == 4.0
        pts += [("node0", (0.125, 0.375, 0.625)), ("node0", (0.875, 0.125, 0.375))]
    return pts


def _finish(c):
    nt = c.net
    c.P32, c.sel, raw = positions32(c.origins, c.dirs, c.sb_rows, c.n, c.near, c.far, c.lin, nt.aabb, want_raw=True)
    rnd = raw[c.n_planted:]
    assert not np.any(rnd == 0) and not np.any(rnd == 1), \
        f"{c.name}: a random P32 coordinate on a selector border: change SEEDS[{c.name!r}]"
    c.ref = reference(nt, c.P32, c.sel)
    assert np.abs(c.ref.o).max() < O_MAX, f"{c.name}: |o| = {np.abs(c.ref.o).max():.1f}"
    c.bound = FACTOR * c.ref.rel * c.ref.dens
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    net_name, n, kind, lin, nf, R, iw, off = CASES[name]
    nt = net(net_name)
    rng = np.random.default_rng(7919 * SEEDS.get(name, 0) + sorted(CASES).index(name))
    near, far = nf
    if nt.aabb is None:
        origins = rng.uniform(-1.2, 1.2, (R, 3))
    else:
        origins = rng.uniform(0.05, 0.95, (R, 3))
    dirs = rng.standard_normal((R, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    pts = planted_points(nt)[:R]
    for r, (_, pt) in enumerate(pts):
        origins[r], dirs[r] = pt, 0.0
    own = np.sort(rng.uniform(0, 1, (R, n + 1)), axis=1).astype(f32)
    if kind == "shared":
        row = O.initial_spacing_bins(n).numpy() if n == 256 else own[0]
        sb, sb_rows = row.copy(), np.broadcast_to(row, (R, n + 1)).copy()
    elif kind == "wide":
        sb, sb_rows = np.concatenate([own, np.full((R, WIDE_EXTRA), np.nan, f32)], axis=1), own
    else:
        sb = sb_rows = own
    c = SimpleNamespace(name=name, net=nt, n=n, kind=kind, lin=lin, near=near, far=far, R=R, image_width=iw, ray_offset=off,
                        origins=origins.astype(f32), dirs=dirs.astype(f32), sb=np.ascontiguousarray(sb), sb_rows=sb_rows,
                        tags=[t for t, _ in pts], n_planted=len(pts))
    c.patch = iw >= 8 and R >= 8 * iw
    if c.patch:
        band0, band1 = (off // iw) // 8, ((off + R - 1) // iw) // 8
        c.blocks = (band1 - band0 + 1) * ((iw + 7) // 8) * ((n + 3) // 4)
        c.last_band_rows = (off + R - 1) // iw - 8 * band1 + 1
    return _finish(c)


# name: (net, n, bin rows, spacing (1 = uniform), (near, far), R, image_width, ray_offset)
CASES = {
    "a-n4-own": ("t5h16-hashed", 4, "own", 0, NF_LONG, 64, 8, 0),                 # one workgroup
    "a-n13-shared-9rows": ("t5h16-hashed", 13, "shared", 0, NF_LONG, 72, 8, 0),   # the last band holds one live row
    "a-n1-uniform-63": ("t5h16-hashed", 1, "own", 1, NF_SHORT, 63, 8, 0),         # one ray short of a band: linear kernel
    "a-n7-wide-R1": ("t5h16-hashed", 7, "wide", 0, NF_SHORT, 1, 8, 0),
    "a-n256-shared": ("t5h16-hashed", 256, "shared", 0, NF_LONG, 64, 8, 0),
    "b-n8-w37": ("t5h64-dense2", 8, "own", 0, NF_LONG, 296, 37, 0),               # 10 workgroups
    "b-n5-shared-w9": ("t5h64-dense2", 5, "shared", 1, NF_SHORT, 72, 9, 0),       # 4 workgroups
    "b-n16-wide-offset": ("t5h64-dense2", 16, "wide", 0, NF_LONG, 80, 9, 31),     # starts at row 3, column 4
    "c-n2-own": ("t8h16-box-dense8", 2, "own", 0, NF_SHORT, 64, 8, 0),
    "c-n3-wide-offset": ("t8h16-box-dense8", 3, "wide", 1, NF_SHORT, 100, 9, 13),
    "c-n16-own-offset": ("t8h16-box-dense8", 16, "own", 0, NF_SHORT, 64, 8, 24),
    "d-n4-w64": ("t8h64-dense2", 4, "own", 0, NF_LONG, 512, 64, 0),               # 8 workgroups
    "d-n7-shared-71": ("t8h64-dense2", 7, "shared", 1, NF_SHORT, 71, 9, 0),       # one ray short: linear kernel
    "d-n8-exact72": ("t8h64-dense2", 8, "own", 0, NF_SHORT, 72, 9, 0),
    "e-n8-own": ("t5h0-box-dense5", 8, "own", 0, NF_SHORT, 64, 8, 0),
    "e-n13-wide-offset": ("t5h0-box-dense5", 13, "wide", 0, NF_SHORT, 75, 8, 5),
    "f-n5-own": ("t8h0-hashed", 5, "own", 0, NF_LONG, 64, 8, 0),
    "f-n4-shared-w9": ("t8h0-hashed", 4, "shared", 1, NF_SHORT, 72, 9, 0),
    "g-n4-own": ("c5h16-f32", 4, "own", 0, NF_LONG, 64, 8, 0),
    "g-n13-wide-offset": ("c5h16-f32", 13, "wide", 1, NF_SHORT, 80, 9, 31),
    "g-n1-shared": ("c5h16-f32", 1, "shared", 0, NF_LONG, 64, 8, 0),
    "h-n8-own": ("c8h64-f16", 8, "own", 0, NF_LONG, 64, 8, 0),
    "h-n3-shared-w9": ("c8h64-f16", 3, "shared", 0, NF_SHORT, 72, 9, 0),
    "i-n2-own": ("c5h0-box-f16", 2, "own", 0, NF_SHORT, 64, 8, 0),
    "i-n16-wide-offset": ("c5h0-box-f16", 16, "wide", 0, NF_SHORT, 64, 8, 3),
    "j-n5-own": ("c8h16-box-f32", 5, "own", 0, NF_SHORT, 64, 8, 0),
    "j-n4-shared-w37": ("c8h16-box-f32", 4, "shared", 1, NF_SHORT, 296, 37, 0),
}


def hold(c, got, rows=None):
    """Every sample of a result ([R,n] float32, numpy or a torch tensor) against the case's reference: exactly 0 where
    sel = 0, within its bound elsewhere.  Asserts, and returns the worst error / bound."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    rows = slice(None) if rows is None else rows
    ref, bound, sel = c.ref.dens[rows], c.bound[rows], c.sel[rows]
    assert got.dtype == f32 and got.shape == ref.shape, (got.dtype, got.shape, ref.shape)
    assert not np.isnan(got).any(), f"{c.name}: NaN in the result"
    bad = np.argwhere(~sel & (got != 0))
    assert len(bad) == 0, f"{c.name}: {len(bad)} masked samples are not 0, first (ray, i) {bad[:8].tolist()}"
    err = np.abs(got.astype(np.float64) - ref)
    bad = np.argwhere(err > bound)
    ratio = err[sel] / bound[sel]
    assert len(bad) == 0, (f"{c.name}: {len(bad)} of {sel.sum()} samples beyond their bound, first (ray, i) {bad[:8].tolist()}, "
                           f"worst error / bound {ratio.max():.3g}")
    return float(ratio.max()) if ratio.size else 0.0


def run_chain32(c, mut=None):
    return chain32(c.net, c.origins, c.dirs, c.sb_rows, c.n, c.near, c.far, c.lin, mut)


@functools.lru_cache(maxsize=None)
def measure_chain32():
    """-> worst error of chain32 / the UNSCALED bound (FACTOR = 1) over all cases"""
    worst = 0.0
    for name in CASES:
        c = case(name)
        err = np.abs(run_chain32(c).astype(np.float64) - c.ref.dens)
        live = c.sel
        worst = max(worst, float((err[live] / (c.ref.rel * c.ref.dens)[live]).max()))
    return worst


def check_coverage():
    """each edge the module's header lists is present"""
    cases = [case(k) for k in CASES]
    nets = [net(k) for k in NETS]
    assert {(t.L, t.H) for t in nets} == {(5, 16), (5, 64), (8, 16), (8, 64), (5, 0), (8, 0)}
    assert {t.layout for t in nets} == {"torch", "tcnn32", "tcnn16"}
    assert all(8 <= t.log2T <= 12 for t in nets)
    tn = [t for t in nets if t.layout == "torch"]
    assert any(t.n_dense == 0 for t in tn) and any(0 < t.n_dense < t.L for t in tn) and any(t.n_dense == t.L for t in tn)
    assert any(t.n_dense == 8 for t in tn), "all 8 levels dense"
    for layout in ("torch", "tcnn32", "tcnn16"):
        assert {t.aabb is None for t in nets if t.layout == layout} == {True, False}, "both normalisations per layout"
    used = {c.net.name for c in cases}
    assert used == set(NETS)
    assert {c.n for c in cases} >= {1, 2, 3, 4, 5, 7, 8, 13, 16, 256}
    assert any(c.n == 256 and c.kind == "shared" for c in cases)
    assert {c.kind for c in cases} == {"own", "shared", "wide"} and {c.lin for c in cases} == {0, 1}
    assert {(c.near, c.far) for c in cases} == {NF_LONG, NF_SHORT}
    for k in ("own", "shared", "wide"):
        assert any(c.kind == k and c.patch for c in cases), f"{k} rows on the patch schedule"
    assert any(c.kind == "wide" and c.sb.shape[1] == c.n + 1 + WIDE_EXTRA and np.isnan(c.sb[:, c.n + 1:]).all() for c in cases)
    # patch geometry
    assert {c.image_width for c in cases if c.patch} == {8, 9, 37, 64}
    assert any(c.R == 8 * c.image_width for c in cases) and any(c.R == 8 * c.image_width - 1 and not c.patch for c in cases)
    assert any(c.patch and c.ray_offset % c.image_width and (c.ray_offset // c.image_width) % 8 for c in cases)
    assert any(c.patch and c.blocks < 8 for c in cases) and any(c.patch and c.blocks > 8 and c.blocks % 8 for c in cases)
    assert any(c.patch and c.last_band_rows == 1 for c in cases)
    assert any(c.patch and c.n % 4 == 0 for c in cases) and any(c.patch and c.n % 4 for c in cases)
    # linear schedule
    assert any((c.R * c.n) % 256 for c in cases) and any(c.R == 1 for c in cases)
    # planted positions: tags, and what the fp32 list makes of them
    for c in cases:
        nt, tags = c.net, c.tags
        P = c.P32[: c.n_planted, 0].astype(np.float64)
        sel = c.sel[: c.n_planted, 0]
        for r, tag in enumerate(tags):
            if tag == "origin":
                assert np.all(P[r] == 0.5) and sel[r]
            elif tag in ("below1", "at1", "above1"):
                far_side = np.abs(4 * P[r] - 2).max()          # x + 2 rounds to 3 from either side; -x + 2 is exact
                assert sel[r] and (far_side == 1.0 or (tag == "above1" and far_side == 1 + 2.0 ** -23))
            elif tag in ("far", "p0", "p1"):
                assert not sel[r] and np.all(P[r] == 0) and np.all(c.ref.dens[r] == 0)
            elif tag == "eps":
                assert sel[r] and np.all(P[r] == 2.0 ** -24)
            elif tag == "last":
                assert sel[r] and np.any(P[r] == 1 - 2.0 ** -24)
                if nt.layout == "torch":          # the last cell of every level, and of every dense copy
                    for l in range(nt.L):
                        s = (c.P32[r, 0] * nt.scalings[l]).astype(f32)
                        assert s.max() < nt.scalings[l] and int(s.max()) == int(nt.scalings[l]) - 1
                        assert l >= len(nt.dense_dim) or int(s.max()) + 1 == nt.dense_dim[l] - 1
            elif tag.startswith("face"):
                l = int(tag[4:])
                on = [np.any((c.P32[r, 0] * nt.scalings[k]) % 1 == 0) for k in range(nt.L)]
                assert sel[r] and on[l], f"{c.name}: {tag} is not on a face of level {l}"
            elif tag == "node0":
                s0 = float(nt.scalings[0]) if nt.layout == "torch" else float(f32(nt.levels[0][0]))
                x = P[r] * s0 + (0.0 if nt.layout == "torch" else 0.5)
                assert sel[r] and np.all(x == np.floor(x))
        if c.R >= 16:
            want = {"origin", "below1", "at1", "above1", "far"} if nt.aabb is None else {"p0", "p1", "eps", "last", "node0"}
            assert want <= set(tags), (c.name, want - set(tags))
            if nt.layout == "torch":
                assert sum(t.startswith("face") for t in tags) >= 2
            assert c.sel[c.n_planted:].any(), f"{c.name}: no live random sample"
    # the contraction's far branch, and masked samples, among the random rays too
    assert any(c.net.aabb is None and (~c.sel[c.n_planted:]).sum() == 0 for c in cases)
    assert any(c.net.aabb is not None and (~c.sel[c.n_planted:]).any() for c in cases)
