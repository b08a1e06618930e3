"""Hand-placed cases for the main field kernels (plain module: tests import it; nothing here needs a GPU).

In scope, all reached through unerf_field_fwd / unerf_field_fwd_masked (csrc/unerf_nerf.hip section 5, unerf_field_mfma16.inc):
field_kernel<ACTIVE | MCDROPOUT> (VALU, one wave per 64 samples), field_kernel_mfma<ACTIVE | MCDROPOUT> (exact fp32 matrix
kernel; fused lookup and pre-gathered features, all three grid layouts), field_kernel_mfma16 in its split form ("f16x2":
hi*hi + hi*lo + lo*hi) and its single-product form ("f16"), the three (SITES, DROP) forms, and the explicit-mask (KeepArgs)
instantiations of each.  The LAPLACE kernels and the GGN fit have a module of their own, tests/laplace_cases.py (their
E[x^2] - E[x]^2 outputs carry a bound that scales with the sample's own second moment), and so has field_kernel_generic, the
any-width kernel: tests/width_cases.py (it reuses `reference` and the bound routines here, which take the layer widths from the
net).  OUT of scope: the several-views kernels (tests/test_gpu_nerf_view_batch.py compares them bit for bit with single
launches) and the R * S >= 2^31 addressing, which is out of reach at test size.

Nets (L = 16, 64 / 64 / 15 / 2, log2T 8 .. 12, a non-zero appearance embedding): the torch hash table, the tcnn layout with
fp32 and with half rows, each under the contraction and under a scene box (sh_remap on for tcnn); `plain` weights (about half
of the ReLUs live), `wide` (hidden rows scaled by 2^-12 .. 2^9 and the next layer's columns scaled back, so activations span
about 2^-20 .. 2^10 inside one sample and the lo half of a split operand is an f16 subnormal or zero) and four `planted` nets
whose chosen rows have zero weights, so the pre-activation is exactly the bias: hidden units at 0, -0.0, +-2^-30, 2^-25, 2^-24
and just under 65504, colour logits at 0, +-17, +-90, +-104, density logits at -104, 0, 80, the beta logit at 20, one ulp above
it and -30.  Rays: planted points of prop_cases.planted_points (direction 0: the normalised position is exact), directions on
the axes and on (+-1, +-1, +-1) / sqrt 3, the rest random; nerfacto and uniform spacing, Euclidean pass-through bins.

Reference.  Everything up to the normalised position and the SH inputs is a fixed list of IEEE fp32 operations
(prop_cases.positions32; `sh_inputs32` here), bit-equal to the oracle's.  From there everything is float64 on the fp32
weights: the trilinear features with the reference's own corners (prop_cases._features64; half rows:
O.tcnn_hash_encode_half), SH16, the five Linear layers with the keep masks and 1 / (1 - p), avg * exp(o) * sel, the sigmoid,
softplus + beta_min (the true softplus: torch's switch at 20 jumps by 2.1e-9, which the bound carries).  The appearance block
is folded into the first colour bias in float64.  For the single-product form ("f16") the reference uses the f16-ROUNDED
weights pack_field_mfma16 packs (its hi halves, the dropout scale folded in before the rounding) and unrounded activations.
Given the masks all of this is continuous in its inputs, so no sample is exempt; an output with sel = 0 is exactly 0.

Bounds, per output, forward, float64 on absolute values (U = 2^-24; nothing comes from a GPU result):
  * features: prop_cases' LERP_UNITS and the rounding of p * scale; SH16: 8 U times the component evaluated on absolute
    values (at most 6 fp32 operations on inputs that are themselves exact here, rounded constants included);
  * a Linear layer y = W x + b, its OWN error at exact inputs: U (sum_k |b + sum_{i <= k} w_i x_i| + |b| + |W| |x|) -- the
    per-sample running error of the sum taken in index order (one rounding per partial sum; the VALU kernel's fma chain
    exactly, the matrix kernels' k-steps up to the order inside a step, which the 4 x below covers) plus one rounding of
    x / (1 - p) (fp32 kernels) or of W / (1 - p) (f16 operand blobs) and of the folded bias.  The layer-wide
    (IN + 1) U (|b| + |W| |x|) in its place left the bound blind to a dropped hi * lo product in three of the four layers;
  * carried errors: the network is piecewise linear, so a unit that is live (or dead) by more than a conservative bound on
    its error (the errors carried through |W| layer by layer) passes an error on exactly by its weights.  An earlier
    layer's error vector e reaches an output as |J| e, J the signed product of the weight matrices gated by those units
    and by the keep masks -- never wider than the product of the |W|; a unit within its bound of 0 adds that bound through
    the |J| behind it (ReLU is 1-Lipschitz).  The feature and SH16 errors are carried the same way;
  * split f16, per matrix layer and product: the exact defect |x w - (x_h w_h + x_h w_l + x_l w_h)| from numpy float16 splits
    of the reference's own operands (hi = f16(x), lo = f16(x - hi)), plus one f16 ulp of lo times |w_h| for the kernel's
    operand differing from the reference's.  The 64 -> 3 colour layer runs in fp32 in this form: nothing added there;
  * single f16, per activation operand of all five layers: (2^-11 |x| + 2^-25) |w_h|;
  * density, relative: do + (|o| + 1) 2^-23 (__expf; expf is tighter) + 2 U, plus 2^-126 absolute (flush);
    rgb: do / 4 + s (1 - s) (|o| + 1) 2^-23 + 3 U s + 2^-126 (the add, v_rcp / the division; exp overflow flushes);
    beta: do + sig(o) (|o| + 1) 2^-23 + U (the rounding of 1 + e) + 3 U softplus + U beta + 2.1e-9.
One constant per family multiplies its bound: 4 x the worst error / bound of a CPU chain over all cases -- the same network
in the kernel's precision and operation order (fp32 fma chains; numpy float16 operands and fp32 accumulation per 16-wide
k-step for the two f16 forms), a correctly rounded exp -- against the float64 reference, never against a kernel
(RATIO_MEASURED_*; the 4 x is the margin pdf_cases.py and prop_cases.py give for the device's transcendental functions and
another summation order).  tests/test_field_cases_cpu.py re-measures them."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import prop_cases as PC
from oracle import nerf_oracle as O

f32 = np.float32
U = 2.0 ** -24
AVG, BETA_MIN = 0.01, 0.01
NF_LONG, NF_SHORT = PC.NF_LONG, PC.NF_SHORT
ACTIVE, MCDROPOUT = 0, 1
TRUNK, HEAD0, HEAD1, HEADIN = 1, 2, 4, 8
STREAM = {TRUNK: 0, HEAD1: 1, HEAD0: 2, HEADIN: 3}
FAMILIES = ("valu", "fp32", "f16x2", "f16")
BOUND_OF = {"valu": "fp32", "fp32": "fp32", "f16x2": "f16x2", "f16": "f16"}       # kernel family -> bound family
SENTINEL = 0x7FC0BEEF        # a NaN with a payload: no result has this bit pattern
SOFTPLUS_JUMP = 2.1e-9       # log1p(exp(20)) - 20
# worst error / unscaled bound of the CPU chains over all cases (against float64, never a kernel), and 4 x it rounded up
RATIO_MEASURED = {"fp32": 0.206, "f16x2": 0.994, "f16": 0.386}
FACTOR = {"fp32": 0.83, "f16x2": 3.98, "f16": 1.55}


# ---------------------------------------------------------------------------------------------------------------- nets
def _linear(rng, out_dim, in_dim, gain=1.0):
    k = gain / np.sqrt(in_dim)
    return rng.uniform(-k, k, (out_dim, in_dim)).astype(f32), rng.uniform(-k, k, out_dim).astype(f32)


HIDDEN_PLANTS = [0.0, -0.0, 2.0 ** -30, -2.0 ** -30, 2.0 ** -25, 2.0 ** -24, float(np.nextafter(f32(65504), f32(0)))]
# planted net: (colour logits r, g, b; density logit; beta logit), None = a live row
PLANTS = {
    "a": ((0.0, 17.0, None), 0.0, 20.0),
    "b": ((-17.0, 90.0, None), -104.0, float(np.nextafter(f32(20), f32(21)))),
    "c": ((-90.0, 104.0, None), 80.0, -30.0),
    "d": ((-104.0, None, None), None, None),
}
# name: (layout, log2T, scene box, weight set)
NETS = {
    "t-plain": ("torch", 10, False, "plain"),
    "t-box-plain": ("torch", 9, True, "plain"),
    "c32-plain": ("tcnn32", 11, False, "plain"),
    "c32-box-plain": ("tcnn32", 10, True, "plain"),
    "c16-plain": ("tcnn16", 12, False, "plain"),
    "c16-box-plain": ("tcnn16", 8, True, "plain"),
    "t-wide": ("torch", 8, False, "wide"),
    "c16-box-wide": ("tcnn16", 10, True, "wide"),
    "t-planted-a": ("torch", 10, False, "planted-a"),
    "c32-box-planted-b": ("tcnn32", 9, True, "planted-b"),
    "c16-planted-c": ("tcnn16", 11, False, "planted-c"),
    "t-box-planted-d": ("torch", 12, True, "planted-d"),
}


@functools.lru_cache(maxsize=None)
def net(name):
    """name -> SimpleNamespace: the grid as prop_cases' nets carry it (L, layout, log2T, scalings | levels, table, aabb) and
    the fp32 weights in torch [out, in] layout: w0 [64,32], w1 [17,64] (row 0 density, 1..15 geo, 16 beta: MCDROPOUT uses the
    first 16), h0 [64,63] over [SH16 | geo15 | appearance32], h1 [64,64], h2 [3,64], app [32]"""
    layout, log2T, box, kind = NETS[name]
    rng = np.random.default_rng(100 + sorted(NETS).index(name))
    c = SimpleNamespace(name=name, L=16, H=64, layout=layout, log2T=log2T, kind=kind, levels=None, scalings=None, n_dense=0,
                        dense=None, dense_off=(), dense_dim=(), aabb=(0.0, 0.0, 0.0, 1.0, 1.0, 1.0) if box else None,
                        sh_remap=int(layout != "torch"))
    if layout == "torch":
        c.scalings = O.hash_scalings(16, 16, 512).numpy().astype(f32)
        assert np.all(c.scalings == np.floor(c.scalings)) and (c.scalings[0] + 1) ** 3 > (1 << log2T), "every level wraps"
        c.table = (rng.standard_normal((16 << log2T, 2)) * 0.5).astype(f32)
    else:
        c.levels = O.tcnn_grid_levels(16, 5, 1.5, log2T)
        c.table = (rng.standard_normal((c.levels[-1][2] + c.levels[-1][3], 2)) * 0.5).astype(f32)
    c.w0, c.b0 = _linear(rng, 64, 32, 2.0)
    c.w1, c.b1 = _linear(rng, 17, 64, 1.5)
    c.h0, c.hb0 = _linear(rng, 64, 63, 1.5)
    c.h1, c.hb1 = _linear(rng, 64, 64, 1.5)
    c.h2, c.hb2 = _linear(rng, 3, 64, 3.0)
    c.app = (rng.standard_normal(32) * 0.5).astype(f32)
    c.planted_units = []
    if kind == "wide":           # ReLU is positively homogeneous: the function is unchanged, the operands are not
        e0, e1 = rng.integers(-12, 10, 64), rng.integers(-12, 10, 64)
        e0[:2], e1[:2] = (-12, 9), (-12, 9)
        s0, s1 = (2.0 ** e0).astype(f32), (2.0 ** e1).astype(f32)
        c.w0, c.b0, c.w1 = c.w0 * s0[:, None], c.b0 * s0, c.w1 / s0[None, :]
        c.h1, c.hb1, c.h2 = c.h1 * s1[:, None], c.hb1 * s1, c.h2 / s1[None, :]
    elif kind.startswith("planted"):
        colours, dens, beta = PLANTS[kind[-1]]
        units = list(range(3, 3 + len(HIDDEN_PLANTS)))
        for j, v in zip(units, HIDDEN_PLANTS):
            c.w0[j], c.b0[j] = 0.0, v
            c.h0[j], c.hb0[j] = 0.0, v          # the same plants among the first colour layer's units
        c.w1[:, units[-1]] *= f32(2.0 ** -16)     # the unit just under 65504 stays a small contribution
        c.h1[:, units[-1]] *= f32(2.0 ** -16)
        c.planted_units = units
        for ch, v in enumerate(colours):
            if v is not None:
                c.h2[ch], c.hb2[ch] = 0.0, v
        if dens is not None:
            c.w1[0], c.b1[0] = 0.0, dens
        if beta is not None:
            c.w1[16], c.b1[16] = 0.0, beta
    assert max(np.abs(w).max() for w in (c.w0, c.w1, c.h0, c.h1, c.h2)) * 10 < 65504, "every packed weight stays below 65504"
    return c


def widths(nt):
    """-> (H, HC, G, AD) of a net: the trunk's and the colour head's hidden widths, the geo features and the appearance
    embedding (nerfacto's 64 / 64 / 15 / 32 unless the net says otherwise)"""
    return nt.w0.shape[0], nt.h1.shape[0], getattr(nt, "G", 15), nt.app.shape[0]


def field_params(nt, mode, dtype=torch.float32, aabb="own"):
    """the net as the oracle's FieldParams"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    G = widths(nt)[2]
    out1 = G + 2 if mode == ACTIVE else G + 1
    box = nt.aabb if aabb == "own" else aabb
    g = O.GridMLP(table=t(nt.table), scalings=None if nt.scalings is None else t(nt.scalings), log2_T=nt.log2T,
                  weights=[t(nt.w0), t(nt.w1[:out1])], biases=[t(nt.b0), t(nt.b1[:out1])], tcnn_levels=nt.levels,
                  aabb=None if box is None else t(np.array(box, f32).reshape(2, 3)), grid_half=nt.layout == "tcnn16")
    return O.FieldParams(grid=g, head_w=[t(nt.h0), t(nt.h1), t(nt.h2)], head_b=[t(nt.hb0), t(nt.hb1), t(nt.hb2)], appearance=t(nt.app),
                         average_init_density=AVG, beta_min=BETA_MIN, sh_remap=bool(nt.sh_remap), geo_feat_dim=G)


# ------------------------------------------------------------------------------------------- the fp32 list: SH inputs
def sh_inputs32(dirs, remap):
    """the kernel's (d + 1) / 2 [* 2 - 1] on float32 arrays"""
    u = (np.asarray(dirs, f32) + f32(1)) / f32(2)
    return u * f32(2) - f32(1) if remap else u


_C = O.SH_C


def _sh16(d, absolute=False):
    """O.sh16 in numpy at the input's precision; absolute: every term on absolute values (the magnitude the roundings scale with)"""
    x, y, z = (np.abs(d[..., i]) if absolute else d[..., i] for i in range(3))
    s = 1.0 if absolute else -1.0
    xx, yy, zz = x * x, y * y, z * z
    c = _C
    comps = [np.full_like(x, c["c0"]), c["c1"] * y, c["c1"] * z, c["c1"] * x, c["c2a"] * x * y, c["c2a"] * y * z,
             c["c2b"] * zz + s * c["c2c"], c["c2a"] * x * z, c["c2d"] * (xx + s * yy), c["c3a"] * y * (3 * xx + s * yy),
             c["c3b"] * x * y * z, c["c3c"] * y * (5 * zz + s * 1), c["c3d"] * z * (5 * zz + s * 3), c["c3c"] * x * (5 * zz + s * 1),
             c["c3e"] * z * (xx + s * yy), c["c3a"] * x * (xx + s * 3 * yy)]
    return np.stack(comps, axis=-1)


# -------------------------------------------------------------------------------------------------- masks and weights
def mask_threshold(p):
    return int(round((1.0 - float(f32(p))) * 65536.0))


def masks_generated(K, p):
    """the counter generator drops something: K > 0 and round((1 - p) 65536) < 65536"""
    return K > 0 and mask_threshold(p) < 65536


def drop_scale(K, p):
    """1 / (1 - p) whenever the Dropout modules are active (K > 0), whether or not the 16-bit threshold can drop a unit"""
    return 1.0 / (1.0 - float(f32(p))) if K > 0 else 1.0


def site_set(sites):
    return sites if sites else (TRUNK | HEAD1)


def generator_masks(seed, K, p, sites, first_sample, N):
    """{site bit: bool [B, N, 64]} the counter generator's keep masks; {} when it generates none"""
    if not masks_generated(K, p):
        return {}
    sidx = (np.arange(N, dtype=np.uint64) + np.uint64(first_sample)).astype(np.uint32)
    return {b: np.stack([O.mc_keep_mask(seed, k, sidx, STREAM[b], 64, float(f32(p))) for k in range(K)])
            for b in (TRUNK, HEAD0, HEAD1, HEADIN) if site_set(sites) & b}


def pack_bits(keep):
    """bool [..., 64] -> uint32 [..., 2] in the layout of unerf_keep_masks"""
    return np.packbits(keep, axis=-1, bitorder="little").view(np.uint32)


def packed_weight(w, scale):
    """the fp32 matrix pack_field_mfma16 splits: w * float(scale) as torch computes it"""
    return (torch.from_numpy(np.ascontiguousarray(w)) * float(scale)).numpy() if scale != 1.0 else w


def _hi(w32):
    return w32.astype(np.float16).astype(np.float64)


def _split(x32):
    hi = x32.astype(np.float16)
    lo = (x32 - hi.astype(f32)).astype(np.float16)
    return hi, lo


def _ulp16(lo16):
    return np.spacing(np.abs(lo16)).astype(np.float64)


def split_defect(x, w):
    """[M,IN] x [OUT,IN] float64 -> [M,OUT]: sum_k |x w - (x_h w_h + x_h w_l + x_l w_h)| + ulp16(x_l) |w_h|, on the fp32
    roundings of the reference's operands"""
    xs, ws = x.astype(f32), w.astype(f32)
    (xh, xl), (wh, wl) = _split(xs), _split(ws)
    xs, ws, xh64, xl64, wh, wl = (a.astype(np.float64) for a in (xs, ws, xh, xl, wh, wl))
    out = _ulp16(xl) @ np.abs(wh).T
    for i in range(0, x.shape[0], 256):
        X, H, Lo = xs[i:i + 256, None, :], xh64[i:i + 256, None, :], xl64[i:i + 256, None, :]
        out[i:i + 256] += np.abs(X * ws[None] - (H * wh[None] + H * wl[None] + Lo * wh[None])).sum(axis=-1)
    return out


def running_sums(x, w, b):
    """[M,IN] x [OUT,IN], [OUT] float64 -> [M,OUT]: sum_k |b + sum_{i <= k} w_i x_i|, what the roundings of a sum taken in
    index order scale with"""
    out = np.zeros((x.shape[0], w.shape[0]))
    for i in range(0, x.shape[0], 256):
        out[i:i + 256] = np.abs(np.cumsum(x[i:i + 256, None, :] * w[None], axis=-1) + b[None, :, None]).sum(axis=-1)
    return out


# ------------------------------------------------------------------------------------------------- float64 reference
def _layer(x, w, b, fams, matrix=True):
    """y = w x + b and {family: e}, the layer's OWN error (its roundings at exact inputs)"""
    aw = np.abs(w)
    y = x @ w.T + b
    base = U * (running_sums(x, w, b) + np.abs(b) + np.abs(x) @ aw.T)
    e = {}
    for f in fams:
        e[f] = base
        if matrix and f == "f16x2":
            e[f] = base + split_defect(x, w)
        if f == "f16":
            e[f] = base + (2.0 ** -11 * np.abs(x) + 2.0 ** -25) @ aw.T
    return y, e


def _bm(J, v):
    """|J| v for a batch of matrices [N,o,i] and vectors [N,i]"""
    return np.einsum("noi,ni->no", np.abs(J), v)


def _gate(a, cons, keep):
    """pre-activations a, a conservative bound on their error, the keep mask -> (units that are live whatever the error, the
    error a unit within its bound of 0 can pass on: ReLU is 1-Lipschitz)"""
    d = np.max([cons[f] for f in cons], axis=0)
    return (a > d) * keep, (np.abs(a) <= d) * keep * d


def reference(nt, mode, P32, sel, shin, K, p, sites, keeps, rounded):
    """P32 [N,3], sel [N], shin [N,3] float32; keeps {site: bool [B,N,units]} ({}: none) -> SimpleNamespace(dens [B,N],
    rgb [B,N,3], beta [N] | None and, per bound family, the UNSCALED bounds b_dens / b_rgb / b_beta).  rounded: the
    single-product form's reference (f16-rounded weights), family "f16"; else the exact weights, families "fp32", "f16x2"."""
    fams = ("f16",) if rounded else ("fp32", "f16x2")
    N, B = P32.shape[0], max(K, 1)
    sc = drop_scale(K, p) if mode == MCDROPOUT else 1.0
    on = site_set(sites) if (mode == MCDROPOUT and K > 0) else 0
    d64 = lambda a: a.astype(np.float64)

    def W(w, site):
        s = sc if on & site else 1.0
        return _hi(packed_weight(w, s)) if rounded else d64(w) * s

    H, HC, G, AD = widths(nt)
    INC = 16 + G                 # the folded first colour layer's inputs [SH16 | geo]
    out1 = G + 2 if mode == ACTIVE else G + 1
    feat, dfeat = PC._features64(nt, d64(P32))
    sh = _sh16(d64(shin))
    dsh = 8 * U * _sh16(d64(shin), absolute=True)
    W0 = W(nt.w0, 0)
    a0, e0 = _layer(feat, W0, d64(nt.b0), fams)
    cons0 = {f: dfeat @ np.abs(W0).T + e0[f] for f in fams}
    h = np.maximum(a0, 0)
    hb0 = d64(nt.hb0) + d64(nt.h0[:, INC:]) @ d64(nt.app)
    res = SimpleNamespace(dens=np.zeros((B, N)), rgb=np.zeros((B, N, 3)), beta=None, b_dens={f: np.zeros((B, N)) for f in fams},
                          b_rgb={f: np.zeros((B, N, 3)) for f in fams}, b_beta={}, o=np.zeros((B, N)), c=np.zeros((B, N, 3)))
    for k in range(B):
        keep = lambda site, width: d64(keeps[site][k][:, :width]) if site in keeps else np.ones((N, width))
        # trunk out
        mT = keep(TRUNK, H)
        live0, amb0 = _gate(a0, cons0, mT)
        W1 = W(nt.w1[:out1], TRUNK)
        t, e1 = _layer(h * mT, W1, d64(nt.b1[:out1]), fams)
        Jt = W1[None] * live0[:, None, :]                                    # a0 -> t
        Jtf = Jt @ W0                                                        # features -> t
        dt = {f: e1[f] + _bm(Jt, e0[f]) + _bm(Jtf, dfeat) + amb0 @ np.abs(W1).T for f in fams}
        cons_t = {f: (cons0[f] * mT) @ np.abs(W1).T + e1[f] for f in fams}
        # colour 0
        if on & HEADIN:      # the first colour layer unfolded (VALU kernel only)
            mI = keep(HEADIN, INC + AD)
            H0 = W(nt.h0, HEADIN)
            x = np.concatenate([sh, t[:, 1:1 + G], np.broadcast_to(d64(nt.app), (N, AD))], axis=1) * mI
            c0, e2 = _layer(x, H0, d64(nt.hb0), fams)
        else:
            mI = np.ones((N, INC))
            H0 = W(nt.h0[:, :INC], 0)
            c0, e2 = _layer(np.concatenate([sh, t[:, 1:1 + G]], axis=1), H0, hb0, fams)
        aH0 = np.abs(H0[:, :INC])
        cons_c0 = {f: (np.concatenate([dsh, cons_t[f][:, 1:1 + G]], axis=1) * mI[:, :INC]) @ aH0.T + e2[f] for f in fams}
        # colour 1 and 2
        m0 = keep(HEAD0, HC)
        live1, amb1 = _gate(c0, cons_c0, m0)
        H1 = W(nt.h1, HEAD0)
        c1, e3 = _layer(np.maximum(c0, 0) * m0, H1, d64(nt.hb1), fams)
        cons_c1 = {f: (cons_c0[f] * m0) @ np.abs(H1).T + e3[f] for f in fams}
        m1 = keep(HEAD1, HC)
        live2, amb2 = _gate(c1, cons_c1, m1)
        H2 = W(nt.h2, HEAD1)
        c2, e4 = _layer(np.maximum(c1, 0) * m1, H2, d64(nt.hb2), fams, matrix=False)
        # the Jacobians onto the colour logits: the network is piecewise linear, so a unit that is live (or dead) whatever
        # the error passes it on exactly by its weight; |J| of the signed product, never wider than the product of |W|
        J4 = H2[None] * live2[:, None, :]                                    # c1 -> c2
        J3 = J4 @ (H1[None] * live1[:, None, :])                             # c0 -> c2
        J2 = J3 @ (H0[None, :, 16:INC] * mI[:, None, 16:INC])                # geo -> c2
        Jsh = J3 @ (H0[None, :, :16] * mI[:, None, :16])                     # SH16 -> c2
        J1 = J2 @ Jt[:, 1:1 + G, :]                                          # a0 -> c2
        Jf = J1 @ W0
        amb = amb2 @ np.abs(H2).T + _bm(J4 @ H1[None], amb1) + _bm(J2 @ W1[None, 1:1 + G], amb0)
        dc2 = {f: e4[f] + _bm(J4, e3[f]) + _bm(J3, e2[f]) + _bm(J2, e1[f][:, 1:1 + G]) + _bm(J1, e0[f]) + _bm(Jf, dfeat) + _bm(Jsh, dsh) + amb
               for f in fams}
        o = t[:, 0]
        s = 0.5 * (1 + np.tanh(0.5 * c2))
        res.o[k], res.c[k] = o, c2
        res.dens[k] = AVG * np.exp(o) * sel
        res.rgb[k] = s
        for f in fams:
            res.b_dens[f][k] = res.dens[k] * (dt[f][:, 0] + (np.abs(o) + 1) * 2.0 ** -23 + 2 * U) + 2.0 ** -126
            res.b_rgb[f][k] = dc2[f] / 4 + s * (1 - s) * (np.abs(c2) + 1) * 2.0 ** -23 + 3 * U * s + 2.0 ** -126
        if mode == ACTIVE:
            u = t[:, G + 1]
            sp = np.logaddexp(0.0, u)
            res.beta = sp + BETA_MIN
            sig = 0.5 * (1 + np.tanh(0.5 * u))
            res.b_beta = {f: dt[f][:, G + 1] + sig * (np.abs(u) + 1) * 2.0 ** -23 + U + 3 * U * sp + U * res.beta + SOFTPLUS_JUMP for f in fams}
    return res


# ---------------------------------------------------------------------------------------------------------- CPU chains
def _dense32(x, w, b, fam, drop_hilo=False):
    """x [M,IN], w [OUT,IN], b [OUT] float32 -> [M,OUT] float32 in the family's arithmetic.  fp32: one fma per input, in order.
    f16x2 / f16: float16 operands, exact products, fp32 accumulation per 16-wide k-step (drop_hilo: without x_h w_l)."""
    M, IN = x.shape
    acc = np.broadcast_to(b, (M, w.shape[0])).astype(f32)
    if fam == "fp32":
        for k in range(IN):
            acc = PC._fma32(np.broadcast_to(x[:, k:k + 1], acc.shape), np.broadcast_to(w[:, k], acc.shape), acc)
        return acc
    (xh, xl), (wh, wl) = _split(x), _split(w)
    xh, xl, wh, wl = (a.astype(np.float64) for a in (xh, xl, wh, wl))
    for k in range(0, IN, 16):
        s = slice(k, k + 16)
        step = xh[:, s] @ wh[:, s].T
        if fam == "f16x2":
            step = step + xl[:, s] @ wh[:, s].T + (0 if drop_hilo else xh[:, s] @ wl[:, s].T)
        acc = (acc.astype(np.float64) + step).astype(f32)
    return acc


def _exp32(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(x.astype(np.float64)).astype(f32)


def chain(c, fam, mut=None):
    """The whole network of a case in the family's precision on the CPU ("fp32", "f16x2", "f16"), a correctly rounded exp.
    mut: one of MUTATIONS.  -> {"dens" [B,N], "rgb" [B,N,3], "beta" [N] | None} float32"""
    nt, N, B = c.net, c.N, c.B
    sc = drop_scale(c.K, c.p) if c.mode == MCDROPOUT else 1.0
    on = site_set(c.sites) if (c.mode == MCDROPOUT and c.K > 0) else 0
    out1 = 17 if c.mode == ACTIVE else 16
    feat = PC._features32(nt, c.P32.reshape(-1, 3)).astype(f32)
    sh = _sh16(c.shin.reshape(-1, 3)).astype(f32)
    if mut == "sh_swap":
        sh = np.concatenate([sh[:, 8:], sh[:, :8]], axis=1)
    hb0 = (nt.hb0.astype(np.float64) + (0 if mut == "no_appearance" else nt.h0[:, 31:].astype(np.float64) @ nt.app.astype(np.float64))).astype(f32)

    def masked(x, site, k, width=64):
        """-> the layer input and its weights' scale: fp32 scales the kept activations, the f16 blobs the weights"""
        s = sc if on & site else 1.0
        if site not in c.keeps:
            return ((x * f32(s)).astype(f32), 1.0) if fam == "fp32" else (x, s)
        kk = k - 1 if (mut == "prev_pass_masks" and k > 0) else k
        keep = c.keeps[site][kk][:, :width]
        if mut == "swap_mask_halves":
            keep = keep.copy()
            keep[:, [0, 1]] = keep[:, [1, 0]]
        dropped = x if mut == "dropped_unscaled" else f32(0)
        if fam == "fp32":
            return np.where(keep, (x * f32(s)).astype(f32), dropped).astype(f32), 1.0
        return np.where(keep, x, dropped).astype(f32), s

    def layer(x, w, b, s=1.0, idx=None, matrix=True):
        f = fam if (matrix or fam == "f16") else "fp32"
        return _dense32(x, packed_weight(w, s), b, f, drop_hilo=(mut == f"drop_hilo_{idx}"))

    h = np.maximum(layer(feat, nt.w0, nt.b0, idx=0), f32(0))
    res = {"dens": np.zeros((B, N), f32), "rgb": np.zeros((B, N, 3), f32), "beta": None}
    for k in range(B):
        x, s = masked(h, TRUNK, k)
        if mut == "skip_last_hidden":
            x = x.copy()
            x[:, 63] = 0
        t = layer(x, nt.w1[:out1], nt.b1[:out1], s, idx=1)
        geo = t[:, 2:17] if (mut == "geo_shift" and out1 == 17) else (t[:, 0:15] if mut == "geo_shift" else t[:, 1:16])
        if on & HEADIN:
            x, s = masked(np.concatenate([sh, geo, np.broadcast_to(nt.app, (N, 32))], axis=1).astype(f32), HEADIN, k, 63)
            c0 = layer(x, nt.h0, nt.hb0, s, idx=2)
        else:
            c0 = layer(np.concatenate([sh, geo], axis=1), nt.h0[:, :31], hb0, idx=2)
        x, s = masked(np.maximum(c0, f32(0)), HEAD0, k)
        c1 = layer(x, nt.h1, nt.hb1, s, idx=3)
        x, s = masked(np.maximum(c1, f32(0)), HEAD1, k)
        c2 = layer(x, nt.h2, nt.hb2, s, idx=4, matrix=False)
        if mut == "swap_gb":
            c2 = c2[:, [0, 2, 1]]
        res["dens"][k] = (f32(AVG) * _exp32(t[:, 0])) * c.sel.reshape(-1).astype(f32)
        with np.errstate(divide="ignore"):
            res["rgb"][k] = f32(1) / (f32(1) + _exp32(-c2))
        if c.mode == ACTIVE:
            u = t[:, 15] if mut == "beta_row" else t[:, 16]
            with np.errstate(over="ignore"):
                sp = np.where(u > f32(20), u, np.log1p(_exp32(u).astype(np.float64)).astype(f32))
            res["beta"] = (sp + f32(BETA_MIN)).astype(f32)
    return res


# mutation -> (the bound family whose chain carries it, which cases it can show on)
_mc = lambda c: c.mode == MCDROPOUT and bool(c.keeps)
MUTATIONS = {
    "dropped_unscaled": ("fp32", _mc),
    "swap_mask_halves": ("fp32", _mc),
    "prev_pass_masks": ("fp32", lambda c: _mc(c) and c.K > 1),
    "geo_shift": ("fp32", lambda c: True),
    "sh_swap": ("fp32", lambda c: True),
    "no_appearance": ("fp32", lambda c: True),
    "skip_last_hidden": ("fp32", lambda c: True),
    "swap_gb": ("fp32", lambda c: True),
    "beta_row": ("fp32", lambda c: c.mode == ACTIVE),
    "drop_hilo_0": ("f16x2", lambda c: c.net.layout != "tcnn16"),       # half rows: the features have no lo half
    "drop_hilo_1": ("f16x2", lambda c: True),
    "drop_hilo_2": ("f16x2", lambda c: True),
    "drop_hilo_3": ("f16x2", lambda c: True),
}


# ------------------------------------------------------------------------------------------------------------- cases
AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
DIAGS = [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]


def _case(net_name, mode, R, S, bins="nerfacto", nf=NF_LONG, iw=0, off=0, K=0, sites=0, p=0.2, masks="gen", seed=1234,
          families=FAMILIES):
    return dict(net=net_name, mode=mode, R=R, S=S, bins=bins, nf=nf, iw=iw, off=off, K=K, sites=sites, p=p, masks=masks, seed=seed,
                families=families)


MAX_OFFSET_S3 = (2 ** 32 - 1) // 3 - 33        # R = 33, S = 3: (ray_offset + R) S = 2^32 - 1, the largest the entry point admits
CASES = {
    # A: ACTIVE, the wave and tile edges of the shapes (tiles = ceil(R / 32) S)
    "A-r1-s1": _case("t-plain", ACTIVE, 1, 1),                           # R S = 1, 1 tile
    "A-r63-s1": _case("t-plain", ACTIVE, 63, 1, "uniform", NF_SHORT),    # R S = 63, 2 tiles
    "A-r32-s2": _case("t-plain", ACTIVE, 32, 2),                         # R S = 64
    "A-r65-s1": _case("t-plain", ACTIVE, 65, 1),                         # R S = 65, 3 tiles
    "A-r31-s7": _case("t-plain", ACTIVE, 31, 7, "euclid"),               # 7 tiles: one XCD gets nothing
    "A-r32-s8": _case("t-plain", ACTIVE, 32, 8),                         # 8 tiles
    "A-r65-s3": _case("t-plain", ACTIVE, 65, 3, "uniform"),              # 9 tiles
    "A-r31-s17": _case("t-plain", ACTIVE, 31, 17, nf=NF_SHORT),          # 17 tiles: ceil(17 / 4) = 5 workgroups, 3 surplus
    "A-r65-s11": _case("t-plain", ACTIVE, 65, 11),                       # 33 tiles
    "A-r33-s48": _case("t-plain", ACTIVE, 33, 48),                       # 96 tiles
    # B: the layouts and normalisations
    "B-tbox": _case("t-box-plain", ACTIVE, 33, 3, nf=NF_SHORT),
    "B-c32": _case("c32-plain", ACTIVE, 65, 2, "uniform"),
    "B-c32box": _case("c32-box-plain", ACTIVE, 31, 3, "euclid"),
    "B-c16": _case("c16-plain", ACTIVE, 33, 3),
    "B-c16box": _case("c16-box-plain", ACTIVE, 32, 2, nf=NF_SHORT),
    "B-c16box-mc": _case("c16-box-plain", MCDROPOUT, 33, 2, nf=NF_SHORT, K=3),
    "B-c32-mc": _case("c32-plain", MCDROPOUT, 31, 3, K=2),
    # C: wide-range operands
    "C-twide": _case("t-wide", ACTIVE, 33, 3),
    "C-twide-mc": _case("t-wide", MCDROPOUT, 33, 2, K=2, p=0.5),
    "C-c16wide": _case("c16-box-wide", ACTIVE, 32, 3, nf=NF_SHORT),
    "C-c16wide-mc": _case("c16-box-wide", MCDROPOUT, 31, 2, nf=NF_SHORT, K=3, sites=7),
    # D: planted logits and hidden units
    "D-a": _case("t-planted-a", ACTIVE, 33, 2),
    "D-b": _case("c32-box-planted-b", ACTIVE, 32, 2, nf=NF_SHORT),
    "D-c": _case("c16-planted-c", ACTIVE, 33, 2),
    "D-d": _case("t-box-planted-d", ACTIVE, 31, 2, nf=NF_SHORT),
    "D-a-mc": _case("t-planted-a", MCDROPOUT, 33, 2, K=2),
    "D-c-mc": _case("c16-planted-c", MCDROPOUT, 32, 2, K=2, sites=7),
    # E: the pixel-patch schedule (8 x 4 pixel tiles from image_width; at least one full band of 4 rows, else 1-D tiles)
    "E-w8": _case("t-plain", ACTIVE, 32, 3, iw=8),                       # R = 4 width
    "E-w8-below": _case("t-plain", ACTIVE, 31, 3, iw=8),                 # one below: 1-D tiles
    "E-w9-offset": _case("c32-plain", ACTIVE, 40, 2, iw=9, off=31),      # starts at row 3, column 4: inside a row and a band
    "E-w37": _case("t-box-plain", ACTIVE, 148, 2, nf=NF_SHORT, iw=37),
    "E-w64-mc": _case("c16-plain", MCDROPOUT, 256, 1, iw=64, K=2),
    "E-w9-lastrow": _case("t-plain", MCDROPOUT, 45, 2, iw=9, K=2),       # 5 rows: the last band holds one live row
    # F: the generator's masks: K, drop_sites, p_drop
    "F-k0": _case("t-plain", MCDROPOUT, 33, 2, K=0),
    "F-k1": _case("t-plain", MCDROPOUT, 33, 2, K=1),
    "F-k2-s1": _case("t-box-plain", MCDROPOUT, 31, 3, nf=NF_SHORT, K=2, sites=1),
    "F-k3-s4": _case("c32-plain", MCDROPOUT, 33, 2, K=3, sites=4, p=0.5),
    "F-k8-s2": _case("t-plain", MCDROPOUT, 32, 1, K=8, sites=2, p=0.9),
    "F-k10-s7": _case("c16-plain", MCDROPOUT, 33, 1, K=10, sites=7),
    "F-k2-s13": _case("t-plain", MCDROPOUT, 33, 2, K=2, sites=13, families=("valu",)),     # HEADIN: 63 inputs, VALU only
    "F-k3-p0": _case("t-plain", MCDROPOUT, 33, 2, K=3, p=0.0),
    "F-k2-p2^-16": _case("t-plain", MCDROPOUT, 65, 3, K=2, p=2.0 ** -16),
    "F-k2-p0.9-s7": _case("c32-box-plain", MCDROPOUT, 33, 2, nf=NF_SHORT, K=2, sites=7, p=0.9),
    # G: explicit keep bits (sample 0: every unit dropped at every site, sample 1: every unit kept)
    "G-x-s5": _case("t-plain", MCDROPOUT, 33, 2, K=2, masks="explicit"),
    "G-x-s7": _case("c16-box-plain", MCDROPOUT, 31, 3, nf=NF_SHORT, K=3, sites=7, p=0.5, masks="explicit"),
    "G-x-s2": _case("c32-plain", MCDROPOUT, 32, 1, K=1, sites=2, masks="explicit"),
    # H: the mask counter next to 2^32
    "H-counter-max": _case("t-plain", MCDROPOUT, 33, 3, K=2, off=MAX_OFFSET_S3),
    # I: p_drop = 2^-17: round((1 - p) 65536) = 65536, so the generator keeps every unit, and the module scales by 1 / (1 - p)
    "I-p2^-17": _case("t-plain", MCDROPOUT, 33, 3, K=2, p=2.0 ** -17),
    "I-p2^-17-s7": _case("t-box-plain", MCDROPOUT, 33, 2, nf=NF_SHORT, K=2, sites=7, p=2.0 ** -17),
}


def second_tile_spec(cus):
    """more tiles than 4 x the persistent grid at 3 workgroups per CU, so that waves walk a second tile: 2 rays are one ray
    block, so tiles = S"""
    return _case("t-plain", ACTIVE, 2, 4 * 3 * cus + 8, "uniform", NF_SHORT)


def tiles_of(R, S, iw=0, off=0):
    """make_tiles (csrc/unerf_nerf.hip) -> (tiles, on the patch schedule)"""
    if iw >= 8 and R >= 4 * iw:
        band0, band1 = (off // iw) // 4, ((off + R - 1) // iw) // 4
        return (band1 - band0 + 1) * ((iw + 7) // 8) * S, True
    return (R + 31) // 32 * S, False


def build(name, spec):
    nt = net(spec["net"])
    names = sorted(CASES)
    rng = np.random.default_rng(7919 + (names.index(name) if name in names else len(names)))
    R, S = spec["R"], spec["S"]
    c = SimpleNamespace(name=name, net=nt, **{k: v for k, v in spec.items() if k != "net"})
    c.N, c.B = R * S, max(c.K, 1) if c.mode == MCDROPOUT else 1
    origins = rng.uniform(-1.2, 1.2, (R, 3)) if nt.aabb is None else rng.uniform(0.05, 0.95, (R, 3))
    dirs = rng.standard_normal((R, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    pts = PC.planted_points(nt)[:max(R - 14, 1) if R > 1 else 0]
    for r, (_, pt) in enumerate(pts):
        origins[r], dirs[r] = pt, 0.0
    special = AXES + [tuple(v / np.sqrt(3.0) for v in d) for d in DIAGS]
    for i, d in enumerate(special[:max(R - len(pts), 0)]):
        dirs[len(pts) + i] = d
    c.tags, c.n_planted = [t for t, _ in pts], len(pts)
    c.origins, c.dirs = origins.astype(f32), dirs.astype(f32)
    near, far = c.nf
    if c.bins == "euclid":       # near_plane < 0: the edges pass through (uniform spacing over [0, 1] is the identity)
        c.sb = np.sort(rng.uniform(0.05, 2.5, (R, S + 1)), axis=1).astype(f32)
        c.near, c.far, c.lin, pos_args = -1.0, far, 0, (0.0, 1.0, 1)
    else:
        c.sb = np.sort(rng.uniform(0, 1, (R, S + 1)), axis=1).astype(f32)
        c.lin = int(c.bins == "uniform")
        c.near, c.far, pos_args = near, far, (near, far, c.lin)
    P32, sel = PC.positions32(c.origins, c.dirs, c.sb, S, *pos_args, nt.aabb)
    c.P32, c.sel = P32.reshape(-1, 3), sel.reshape(-1)
    c.shin = np.repeat(sh_inputs32(c.dirs, nt.sh_remap), S, axis=0)
    c.tiles, c.patch = tiles_of(R, S, c.iw, c.off)
    c.first_sample = (c.off * S) & 0xFFFFFFFF
    if c.mode != MCDROPOUT or c.K == 0:
        c.keeps = {}
    elif c.masks == "explicit":
        c.keeps = {}
        for b in (TRUNK, HEAD0, HEAD1):
            if site_set(c.sites) & b:
                k = rng.uniform(0, 1, (c.K, c.N, 64)) >= c.p
                k[:, 0], k[:, 1] = False, True
                c.keeps[b] = k
    else:
        c.keeps = generator_masks(c.seed, c.K, c.p, c.sites, c.off * S, c.N)
    args = (nt, c.mode, c.P32, c.sel, c.shin, c.K, c.p, c.sites, c.keeps)
    exact = reference(*args, rounded=False)
    c.ref = {"fp32": exact, "f16x2": exact}
    if "f16" in c.families:
        c.ref["f16"] = reference(*args, rounded=True)
    assert np.abs(exact.o).max() < 110 and np.isfinite(exact.dens).all(), f"{name}: logits"
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    return build(name, CASES[name])


@functools.lru_cache(maxsize=None)
def second_tile_case(cus):
    return build(f"H-second-tile-{cus}", second_tile_spec(cus))


def bound_families(c):
    return sorted({BOUND_OF[f] for f in c.families})


def _ratios(c, bf, out, factor):
    """-> [(what, error, bound)] with the family's factor applied"""
    ref = c.ref[bf]
    items = [("density", out["dens"], ref.dens, ref.b_dens[bf]), ("rgb", out["rgb"], ref.rgb, ref.b_rgb[bf])]
    if c.mode == ACTIVE:
        items.append(("beta", out["beta"], ref.beta, ref.b_beta[bf]))
    return [(w, np.abs(np.asarray(g, np.float64) - r), factor * b) for w, g, r, b in items]


def hold(c, family, out, rows=None):
    """Every output of a result {"dens" [B,N], "rgb" [B,N,3], "beta" [N] | None} (float32) of kernel family `family`
    ("valu", "fp32", "f16x2", "f16"; the CPU chains go by their bound family) against the case's float64 reference: no launch
    sentinel left, no NaN, density exactly 0 where sel = 0, saturated planted colours exactly 0 or 1, every element within
    its bound.  rows: a slice of the samples the result covers.  Asserts, and returns the worst error / bound."""
    bf = BOUND_OF.get(family, family)
    rows = slice(None) if rows is None else rows
    ref = c.ref[bf]
    sel = c.sel[rows]
    worst = 0.0
    full = {"dens": out["dens"], "rgb": out["rgb"], "beta": out.get("beta")}
    for key, g in full.items():
        if g is None:
            assert key == "beta" and c.mode != ACTIVE
            continue
        g = np.asarray(g)
        assert g.dtype == f32, (key, g.dtype)
        assert not (g.view(np.uint32) == SENTINEL).any(), f"{c.name} {family}: {key} still holds the launch sentinel"
        assert not np.isnan(g).any(), f"{c.name} {family}: NaN in {key}"
    dens = np.asarray(out["dens"])
    assert (dens[:, ~sel] == 0).all(), f"{c.name} {family}: a density with sel = 0 is not exactly 0"
    sat = np.abs(ref.c[:, rows]) >= 90
    if sat.any():
        want = (ref.c[:, rows] > 0).astype(f32)
        assert (np.asarray(out["rgb"])[sat] == want[sat]).all(), f"{c.name} {family}: a saturated sigmoid is not exactly 0 or 1"
    cut = lambda a: a[:, rows] if a.ndim >= 2 else a[rows]
    for what, got, r, b in (("density", out["dens"], ref.dens, ref.b_dens[bf]), ("rgb", out["rgb"], ref.rgb, ref.b_rgb[bf])) + \
            ((("beta", out["beta"], ref.beta, ref.b_beta[bf]),) if c.mode == ACTIVE else ()):
        got = np.asarray(got, np.float64)
        r, b = cut(r), FACTOR[bf] * cut(b)
        assert got.shape == r.shape, (what, got.shape, r.shape)
        err = np.abs(got - r)
        ratio = err / b
        bad = np.argwhere(err > b)
        assert len(bad) == 0, (f"{c.name} {family}: {len(bad)} of {err.size} {what} outputs beyond their bound, first {bad[:6].tolist()}, "
                               f"worst error / bound {ratio.max():.3g}")
        worst = max(worst, float(ratio.max()))
    return worst


@functools.lru_cache(maxsize=None)
def measure_chain(bf):
    """-> worst error / UNSCALED bound (factor 1) of the family's CPU chain over all cases"""
    worst = 0.0
    for name in CASES:
        c = case(name)
        if bf not in bound_families(c):
            continue
        worst = max(worst, hold_ratio_unscaled(c, bf, chain(c, bf)))
    return worst


def hold_ratio_unscaled(c, bf, out):
    return max(float((e / b).max()) for _, e, b in _ratios(c, bf, out, 1.0))


def check_coverage():
    """each edge the module's header lists is present"""
    cases = [case(k) for k in CASES]
    nets = [net(k) for k in NETS]
    assert {c.net.name for c in cases} == set(NETS)
    for layout in ("torch", "tcnn32", "tcnn16"):
        assert {t.aabb is None for t in nets if t.layout == layout} == {True, False}, "both normalisations per layout"
    assert all(8 <= t.log2T <= 12 and np.abs(t.app).min() > 0 for t in nets)
    assert all(t.sh_remap == (t.layout != "torch") for t in nets)
    assert {c.R for c in cases} >= {1, 31, 32, 33, 65} and {c.S for c in cases} >= {1, 2, 3, 17, 48}
    assert {c.N for c in cases} >= {1, 63, 64, 65}
    assert {c.tiles for c in cases if not c.patch} >= {1, 7, 8, 9, 33}
    assert any(((c.tiles + 3) // 4) % 8 for c in cases), "surplus workgroups of the rounded-up grid"
    big = second_tile_spec(256)
    assert tiles_of(big["R"], big["S"])[0] > 4 * 3 * 256
    assert {c.iw for c in cases if c.patch} == {8, 9, 37, 64}
    assert any(c.iw and c.R == 4 * c.iw for c in cases) and any(c.iw and c.R == 4 * c.iw - 1 and not c.patch for c in cases)
    assert any(c.patch and c.off % c.iw and (c.off // c.iw) % 4 for c in cases)
    assert any(c.patch and (c.off + c.R - 1) // c.iw % 4 == 0 and (c.off + c.R) % c.iw == 0 for c in cases), "a last band of one live row"
    assert {c.bins for c in cases} == {"nerfacto", "uniform", "euclid"} and {c.nf for c in cases} == {NF_LONG, NF_SHORT}
    mc = [c for c in cases if c.mode == MCDROPOUT]
    assert {c.K for c in mc} >= {0, 1, 2, 3, 8, 10} and {site_set(c.sites) for c in mc} >= {5, 1, 4, 2, 7, 13}
    assert all(c.families == ("valu",) for c in mc if site_set(c.sites) & HEADIN)
    assert {c.p for c in mc} >= {0.0, 2.0 ** -17, 2.0 ** -16, 0.2, 0.5, 0.9}
    assert mask_threshold(2.0 ** -17) == 65536 and mask_threshold(2.0 ** -16) == 65535
    assert all(not c.keeps for c in mc if c.p in (0.0, 2.0 ** -17) or c.K == 0) and drop_scale(2, 2.0 ** -17) > 1
    for c in mc:
        if c.masks == "explicit":
            assert all(not k[:, 0].any() and k[:, 1].all() for k in c.keeps.values()) and len(c.keeps) == bin(site_set(c.sites)).count("1")
        elif c.keeps and 0.1 <= c.p < 0.6:
            assert all(0.3 < k.mean() < 1 and not k.all() for k in c.keeps.values())
    h = case("H-counter-max")
    assert (h.off + h.R) * h.S == 2 ** 32 - 1 and (h.off + h.R + 1) * h.S >= 2 ** 32
    # planted positions and directions
    for c in cases:
        if c.R >= 31:
            want = {"origin", "below1", "at1", "above1", "far"} if c.net.aabb is None else {"p0", "p1", "eps", "last", "node0"}
            assert want <= set(c.tags), (c.name, want - set(c.tags))
            d = c.dirs[c.n_planted:c.n_planted + 14]
            assert (np.abs(d).max(axis=1)[:6] == 1).all() and np.allclose(np.abs(d[6:14]), 1 / np.sqrt(3))
            assert c.sel.any()
        for r, tag in enumerate(c.tags):
            if tag in ("far", "p0", "p1"):
                assert not c.sel[r * c.S] and (c.ref["fp32"].dens[:, r * c.S] == 0).all()
    assert any((~c.sel).any() for c in cases)
    # planted logits and hidden units, and what the operands of the f16 forms look like
    seen_c, seen_d, seen_b = set(), set(), set()
    for c in cases:
        ref = c.ref["fp32"]
        if c.net.kind.startswith("planted"):
            colours, dens, beta = PLANTS[c.net.kind[-1]]
            for ch, v in enumerate(colours):
                if v is not None:
                    assert (ref.c[..., ch] == v).all()
                    seen_c.add(v)
            if dens is not None:
                assert (ref.o == dens).all()
                seen_d.add(dens)
            if beta is not None and c.mode == ACTIVE:
                seen_b.add(beta)
            assert [float(c.net.b0[j]) for j in c.net.planted_units] == [float(f32(v)) for v in HIDDEN_PLANTS]
            assert np.signbit(c.net.b0[c.net.planted_units[1]]) and 65472 < c.net.b0[c.net.planted_units[-1]] < 65504
    assert seen_c == {0.0, 17.0, -17.0, 90.0, -90.0, 104.0, -104.0} and seen_d == {0.0, -104.0, 80.0}
    assert seen_b == {20.0, float(np.nextafter(f32(20), f32(21))), -30.0}
    with np.errstate(over="ignore"):
        assert np.isinf(f32(np.exp(f32(90)))) and np.isinf(f32(np.exp(f32(104)))) and np.isfinite(f32(np.exp(f32(17))))
    w = case("C-twide")
    feat, _ = PC._features64(w.net, w.P32.astype(np.float64))
    h = np.maximum(feat @ w.net.w0.astype(np.float64).T + w.net.b0, 0).astype(f32)
    live = h[h > 0]
    assert live.min() < 2.0 ** -18 and live.max() > 2.0 ** 8, "hidden activations span the wide range"
    span = np.array([row[row > 0].max() / row[row > 0].min() for row in h])
    assert span.max() > 2.0 ** 20, "... inside one sample"
    hi, lo = _split(live)
    lo = np.abs(lo.astype(np.float64))
    assert ((lo > 0) & (lo < 2.0 ** -14)).any() and (lo == 0).any(), "some lo half is subnormal and some is zero"
    assert (np.abs(live - hi.astype(f32)) > 0).any()
