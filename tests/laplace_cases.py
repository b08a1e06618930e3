"""Hand-placed cases for the LAPLACE field kernels and the GGN fit (plain module: tests import it; nothing here needs a GPU).

In scope, all reached through unerf_field_fwd (csrc/unerf_nerf.hip sections 5a, 5b', unerf_field_lap16.inc): field_kernel<LAPLACE>
(VALU, one wave per 64 samples, the sampled rows from ws_density / ws_rgb), field_kernel_mfma_laplace<false> (exact fp32 matrix
kernel, the rows as lap_blob fragments padded to 128), field_kernel_mfma16_laplace in its split form ("f16x2") and its
single-product form ("f16"), whose rows carry the exp2 base change and whose padding register quads are skipped.  Part 2:
unerf_laplace_ggn_diag = field_kernel_mfma_laplace<true> (the capture forward) + laplace_ggn_kernel + laplace_ggn_reduce_kernel.

Nets (Laplace shape: base 32 -> 64 as a bare Linear, hidden 64 -> 15, colour trunk 31 -> 64 -> 64, no appearance block): the
torch, tcnn32 and tcnn16 grids, each under the contraction and under a box, log2T 8 .. 12.  Weight-sample sets (mean row +
spread x noise), per case: `spread` (logit standard deviation about 0.5), `tight` (about 2^-10: var / mean^2 is about 1e-6 and
E[p^2] - E[p]^2 cancels almost completely), `planted-a / -b / -pad` (sampled rows with zero weights, so the pre-activation is
exactly the bias: density logits -100, 0, 1 and one ulp above 1 (a), 40 (b); colour logits 0, 17, -90 (a), -17, 90 (b); one
colour row whose bias is LAP_PAD_BIAS itself (pad: the f16 blobs cannot hold it, so VALU and fp32 matrix kernel only)),
`exact` (every row zero weights: the sums are n times one exactly known value, so a padded row that contributes anything but
0 shows in the last bit) and `mean` (copies of the mean row, for lap_mask_density).  Every density logit lies in [-104, 40]
(p^2 finite in fp32) and every operand below the f16 limit; build() asserts both.

Reference.  Positions and SH inputs are the fp32 lists (prop_cases.positions32, field_cases.sh_inputs32); from there float64 on
the fp32 weights: per sampled row s, p_s = act(w_s . h + b_s), mu = mean p, m2 = mean p^2, var_d = m2 - mu^2, var_rgb = mean
over channels of max(m2_c - mu_c^2, 0); ray g of a launch with per-chunk sets uses set g // lap_chunk_rays.  For the
single-product form the reference rows are the f16-rounded rows pack_laplace_heads16 packs (base change included).

Bounds, per output, float64 on absolute values (U = 2^-24; nothing comes from a GPU result, no output is exempt):
  * carried error of h: the base output is linear in the features (dfeat |W0| + the layer's own error); the colour hidden
    vector sits behind two ReLUs: field_cases' _layer / _gate / _bm -- a unit live or dead whatever its error passes the error
    on by its weight, one within its bound of 0 adds the bound;
  * dpre_s = |w_s| e_h + U (sum_k |partial sum_k| + |b| + |w||h|) + the exact split defect (f16x2) / (2^-11 |h| + 2^-25) |w_h|
    (f16), both taken on the base-changed row and divided by |log2 e|, + U (|w||h| + |b|), one rounding of the base-changed row;
  * dp_s = act'(pre) (dpre + (|pre| + 1) 2^-23) (__expf; v_exp_f32 after the base change is tighter) + 2 U p (exp) | 3 U p
    (sigmoid: the add and v_rcp_f32) + 2^-126 (flush).  Softplus: mf_softplus_fast is x above 20 (2.1e-9 off the true softplus),
    e (1 - e (1/2 - e / 3)) below e = 1e-3 (the series' next term e^4 / 4 <= 2.5e-10 e, three roundings) and __logf(1 + e)
    between (one rounding of 1 + e: U absolute; v_log_f32: an ulp of a result >= 1e-3): sig(pre) (dpre + (|pre| + 1) 2^-23) + U
    + (3 U + 2.5e-10) softplus + 2.1e-9;
  * dmu = mean dp + (n + 2) U mean |p|; dm2 = mean 2 p dp + (n + 3) U m2; dvar_d = dm2 + 2 |mu| dmu + 2 U (m2 + mu^2): it
    scales with the sample's own second moment; dvar_rgb = (1/3) sum_c dvar_c + U var_rgb (max(., 0) is 1-Lipschitz).
  * density variance may be negative inside its bound; colour variance must be >= 0; under lap_mask_density the density is
    mu sel (exactly 0 where sel = 0) and its variance EXACTLY 0.
One constant per bound family multiplies its bound: 4 x the worst error / bound of a CPU chain over all cases (the same network
in the family's precision and operation order, correctly rounded exp / exp2 / log) against the float64 reference, never a kernel
(RATIO_MEASURED, FACTOR; tests/test_laplace_cases_cpu.py re-measures them)."""
import functools
from types import SimpleNamespace

import numpy as np

import field_cases as FC
import prop_cases as PC
from oracle import nerf_oracle as O

f32 = np.float32
U = 2.0 ** -24
LOG2E = 1.4426950408889634
LAP_PAD_BIAS = -1e30
LAP_ROWS = 128                 # rows of a head in the blobs (LAP_BLOCKS x 32)
F16_LIMIT = 65504.0
EXP2_ROWS = True               # the build the bounds are stated for (bare exp2 in the heads: unerf_build_flags); the GPU test asserts the library's flag
NF_LONG, NF_SHORT = PC.NF_LONG, PC.NF_SHORT
FAMILIES, BOUND_OF, SENTINEL = FC.FAMILIES, FC.BOUND_OF, FC.SENTINEL
SOFTPLUS_JUMP, SERIES = FC.SOFTPLUS_JUMP, 2.5e-10
# worst error / unscaled bound of the CPU chains over all cases (against float64, never a kernel), and 4 x it rounded up
RATIO_MEASURED = {"fp32": 0.107, "f16x2": 0.0995, "f16": 0.072}
FACTOR = {"fp32": 0.43, "f16x2": 0.40, "f16": 0.29}

N_LAP_EDGES = (1, 3, 4, 5, 7, 8, 9, 31, 32, 33, 36, 37, 63, 64, 65, 96, 100, 127, 128)
# name: (layout, log2T, scene box)
NETS = {"t": ("torch", 10, False), "t-box": ("torch", 9, True), "c32": ("tcnn32", 11, False), "c32-box": ("tcnn32", 10, True),
        "c16": ("tcnn16", 12, False), "c16-box": ("tcnn16", 8, True)}
# planted set: (density logits of rows 0.., colour logits (r, g, b) of row 0; None: a live entry)
ONE_UP = float(np.nextafter(f32(1), f32(2)))
PLANTS = {"a": ((-100.0, 0.0, 1.0, ONE_UP), (0.0, 17.0, -90.0)), "b": ((40.0,), (-17.0, 90.0, None)), "pad": ((), (None, None, None))}
EXACT = {"exp": 1.0, "softplus": 30.0}           # the exact set: density bias 0 (exp) | 30 (softplus: above the switch at 20)


# ---------------------------------------------------------------------------------------------------------------- nets
@functools.lru_cache(maxsize=None)
def net(name):
    """name -> the grid as prop_cases' nets carry it and the fp32 weights in torch [out, in] layout: w0 [64,32], w1 [15,64],
    h0 [64,31] over [SH16 | geo15], h1 [64,64], and the mean last layers dmean [65], cmean [195] (rows, then bias)"""
    layout, log2T, box = NETS[name]
    rng = np.random.default_rng(300 + sorted(NETS).index(name))
    c = SimpleNamespace(name=name, L=16, H=64, layout=layout, log2T=log2T, levels=None, scalings=None, n_dense=0, dense=None,
                        dense_off=(), dense_dim=(), aabb=(0.0, 0.0, 0.0, 1.0, 1.0, 1.0) if box else None, sh_remap=int(layout != "torch"))
    if layout == "torch":
        c.scalings = O.hash_scalings(16, 16, 512).numpy().astype(f32)
        c.table = (rng.standard_normal((16 << log2T, 2)) * 0.5).astype(f32)
    else:
        c.levels = O.tcnn_grid_levels(16, 5, 1.5, log2T)
        c.table = (rng.standard_normal((c.levels[-1][2] + c.levels[-1][3], 2)) * 0.5).astype(f32)
    c.w0, c.b0 = FC._linear(rng, 64, 32, 2.0)
    c.w1, c.b1 = FC._linear(rng, 15, 64, 1.5)
    c.h0, c.hb0 = FC._linear(rng, 64, 31, 1.5)
    c.h1, c.hb1 = FC._linear(rng, 64, 64, 1.5)
    dw, db = FC._linear(rng, 1, 64, 1.0)
    cw, cb = FC._linear(rng, 3, 64, 3.0)
    c.dmean = np.concatenate([dw.reshape(-1), db]).astype(f32)
    c.cmean = np.concatenate([cw.reshape(-1), cb]).astype(f32)
    return c


def weight_sets(nt, kind, n, nr, sets, act, seed):
    """-> ws_density [sets, n, 65], ws_rgb [sets, nr, 195] float32"""
    rng = np.random.default_rng(seed)
    spread = {"tight": 0.1 * 2.0 ** -9}.get(kind, 0.1)
    wsd = (nt.dmean[None, None] + spread * rng.standard_normal((sets, n, 65))).astype(f32)
    wsr = (nt.cmean[None, None] + spread * rng.standard_normal((sets, nr, 195))).astype(f32)
    if kind == "mean":
        wsd[:] = nt.dmean
    elif kind == "exact":
        wsd[:], wsr[:] = 0.0, 0.0
        wsd[..., 64] = 0.0 if act == "exp" else EXACT["softplus"]
    elif kind.startswith("planted"):
        dens, colours = PLANTS[kind[8:]]
        assert n >= len(dens) + 1 and nr >= 3
        for s, v in enumerate(dens):
            wsd[:, s], wsd[:, s, 64] = 0.0, v
        for ch, v in enumerate(colours):
            if v is not None:
                wsr[:, 0, 64 * ch:64 * ch + 64], wsr[:, 0, 192 + ch] = 0.0, v
        if kind == "planted-pad":
            wsr[:, 2, 0:64], wsr[:, 2, 192] = 0.0, LAP_PAD_BIAS
    return wsd, wsr


# ------------------------------------------------------------------------------------------------- float64 reference
def _act(pre, dpre, act):
    """-> p, dp: the activation and its error at pre-activation error dpre (header: dp_s)"""
    t = (np.abs(pre) + 1) * 2.0 ** -23
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if act == "exp":
            p = np.exp(pre)
            return p, np.where(p > 0, p * (dpre + t + 2 * U), 0.0) + 2.0 ** -126
        s = 0.5 * (1 + np.tanh(0.5 * pre))
        d1 = s * (1 - s)
        if act == "sigmoid":
            return s, np.where(d1 > 0, d1 * (dpre + t), 0.0) + 3 * U * s + 2.0 ** -126
        sp = np.logaddexp(0.0, pre)
        return sp, np.where(s > 0, s * (dpre + t), 0.0) + U + (3 * U + SERIES) * sp + SOFTPLUS_JUMP + 2.0 ** -126


def head_scale(act):
    """the base change a row of lap16_blob carries"""
    if not EXP2_ROWS:
        return 1.0
    return {"exp": LOG2E, "softplus": 1.0, "sigmoid": -LOG2E}[act]


def scaled_rows(W, b, act):
    """the fp32 rows pack_laplace_heads16 splits: w * scale taken in float64 and rounded once"""
    s = head_scale(act)
    return (W.astype(np.float64) * s).astype(f32), (b.astype(np.float64) * s).astype(f32)


def _head(v, carried, W, b, act, fams):
    """v [M,64] float64, carried(rows [n,64], family) -> [M,n] (the error of the head's input carried onto the rows' dot
    products), W [n,64], b [n] float32 -> p [M,n] and {family: dp [M,n]}"""
    d64 = lambda a: a.astype(np.float64)
    s = head_scale(act)
    Ws, bs = scaled_rows(W, b, act)
    if fams == ("f16",):
        Wr = FC._hi(Ws) / s
        pre = v @ Wr.T + d64(bs) / s
        own = {"f16": FC._layer(v, FC._hi(Ws), d64(bs), fams)[1]["f16"] / abs(s)}
        rows = {"f16": Wr}
    else:
        pre, e = FC._layer(v, d64(W), d64(b), ("fp32",))
        own, rows = {"fp32": e["fp32"]}, {f: d64(W) for f in fams}
        if "f16x2" in fams:
            own["f16x2"] = FC._layer(v, d64(Ws), d64(bs), ("f16x2",))[1]["f16x2"] / abs(s) + U * (np.abs(v) @ np.abs(d64(W)).T + np.abs(d64(b)))
    out = {}
    for f in fams:
        p, out[f] = _act(pre, carried(rows[f], f) + own[f], act)
    return p, out


def _moments(p, dp, n):
    """p, dp [M,n] -> mu, var, dmu, dvar [M]"""
    mu, m2 = p.mean(axis=1), (p * p).mean(axis=1)
    dmu = dp.mean(axis=1) + (n + 2) * U * np.abs(p).mean(axis=1)
    dm2 = (2 * np.abs(p) * dp).mean(axis=1) + (n + 3) * U * m2
    return mu, m2 - mu * mu, dmu, dm2 + 2 * np.abs(mu) * dmu + 2 * U * (m2 + mu * mu)


def trunk64(nt, P32, shin, rounded):
    """-> SimpleNamespace: hb, x [N,64] float64 (the inputs of the two sampled heads), the error sources of every stage and the
    gates of the two ReLUs, from which carried_density / carried_rgb take a row's carried error"""
    fams = ("f16",) if rounded else ("fp32", "f16x2")
    d64 = lambda a: a.astype(np.float64)
    W = (lambda w: FC._hi(w)) if rounded else d64
    t = SimpleNamespace(fams=fams)
    feat, t.dfeat = PC._features64(nt, d64(P32))
    sh, t.dsh = FC._sh16(d64(shin)), 8 * U * FC._sh16(d64(shin), absolute=True)
    t.W0, t.W1, t.H0, t.H1 = W(nt.w0), W(nt.w1), W(nt.h0), W(nt.h1)
    t.hb, t.e0 = FC._layer(feat, t.W0, d64(nt.b0), fams)
    cons_hb = {f: t.dfeat @ np.abs(t.W0).T + t.e0[f] for f in fams}           # a bare Linear: no gate
    geo, t.e1 = FC._layer(t.hb, t.W1, d64(nt.b1), fams)
    cons_geo = {f: cons_hb[f] @ np.abs(t.W1).T + t.e1[f] for f in fams}
    c0, t.e2 = FC._layer(np.concatenate([sh, geo], axis=1), t.H0, d64(nt.hb0), fams)
    cons0 = {f: np.concatenate([t.dsh, cons_geo[f]], axis=1) @ np.abs(t.H0).T + t.e2[f] for f in fams}
    t.live0, t.amb0 = FC._gate(c0, cons0, np.ones_like(c0))
    c1, t.e3 = FC._layer(np.maximum(c0, 0), t.H1, d64(nt.hb1), fams)
    cons1 = {f: cons0[f] @ np.abs(t.H1).T + t.e3[f] for f in fams}
    t.live1, t.amb1 = FC._gate(c1, cons1, np.ones_like(c1))
    t.x = np.maximum(c1, 0)
    return t


def carried_density(t, m, rows, f):
    """the error of hb = W0 feat + b0 on the rows' dot products: |rows W0| dfeat + |rows| e0 (the signed product first)"""
    return t.dfeat[m] @ np.abs(rows @ t.W0).T + t.e0[f][m] @ np.abs(rows).T


def carried_rgb(t, m, rows, f):
    """the errors of every stage behind the colour hidden vector, each through |J|, J the signed product of the weight matrices
    gated by the units that are live whatever their error; a unit within its bound of 0 adds that bound through the |J| behind
    it (field_cases.reference)"""
    A4 = rows[None] * t.live1[m][:, None, :]                      # c1 -> row
    A3 = A4 @ (t.H1[None] * t.live0[m][:, None, :])                # c0 -> row
    Ag, As = A3 @ t.H0[:, 16:], A3 @ t.H0[:, :16]                  # geo, SH16 -> row
    Ah = Ag @ t.W1                                                 # hb -> row
    Af = Ah @ t.W0                                                 # features -> row
    return (FC._bm(A4, t.e3[f][m]) + FC._bm(A3, t.e2[f][m]) + FC._bm(Ag, t.e1[f][m]) + FC._bm(As, t.dsh[m]) + FC._bm(Ah, t.e0[f][m])
            + FC._bm(Af, t.dfeat[m]) + t.amb1[m] @ np.abs(rows).T + FC._bm(A4 @ t.H1[None], t.amb0[m]))


def reference(c, rounded, set_shift=0):
    """-> SimpleNamespace(dens, var_d [N], rgb [N,3], var_rgb [N] float64, the UNSCALED bounds b_* {family: ...}, the logits
    pre_d [N,n], pre_c [N,nr,3]).  set_shift: every chunk evaluated with the set that many chunks earlier (set-distinctness)"""
    nt, N = c.net, c.N
    H, HC = nt.w0.shape[0], nt.h1.shape[0]       # the inputs of the two sampled heads (64 / 64 here; tests/width_cases.py has others)
    t = trunk64(nt, c.P32, c.shin, rounded)
    hb, x, fams = t.hb, t.x, t.fams
    r = SimpleNamespace(dens=np.zeros(N), var_d=np.zeros(N), rgb=np.zeros((N, 3)), var_rgb=np.zeros(N), pre_d=np.zeros((N, c.n)),
                        pre_c=np.zeros((N, c.nr, 3)), b_dens={f: np.zeros(N) for f in fams}, b_var_d={f: np.zeros(N) for f in fams},
                        b_rgb={f: np.zeros((N, 3)) for f in fams}, b_var_rgb={f: np.zeros(N) for f in fams})
    for st in np.unique(c.set_of):
        m = c.set_of == st
        use = max(int(st) - set_shift, 0)
        wd, wr = c.wsd[use], c.wsr[use][:c.nr]
        p, dp = _head(hb[m], lambda rows, f: carried_density(t, m, rows, f), wd[:, :H], wd[:, H], c.act, fams)
        with np.errstate(divide="ignore"):
            r.pre_d[m] = np.log(p) if c.act == "exp" else p
        for f in fams:
            mu, var, dmu, dvar = _moments(p, dp[f], c.n)
            if c.mask:
                mu, var, dmu, dvar = mu * c.sel[m], 0 * var, dmu * c.sel[m], 0 * dvar
            r.dens[m], r.var_d[m], r.b_dens[f][m], r.b_var_d[f][m] = mu, var, dmu, dvar
        vsum, dvsum = {f: 0.0 for f in fams}, {f: 0.0 for f in fams}
        for ch in range(3):
            p, dp = _head(x[m], lambda rows, f: carried_rgb(t, m, rows, f), wr[:, HC * ch:HC * ch + HC], wr[:, 3 * HC + ch], "sigmoid", fams)
            with np.errstate(divide="ignore"):
                r.pre_c[m, :, ch] = np.log(p) - np.log1p(-p)
            for f in fams:
                mu, var, dmu, dvar = _moments(p, dp[f], c.nr)
                r.rgb[m, ch], r.b_rgb[f][m, ch] = mu, dmu
                vsum[f], dvsum[f] = vsum[f] + np.maximum(var, 0), dvsum[f] + dvar
        for f in fams:
            r.var_rgb[m] = vsum[f] / 3
            r.b_var_rgb[f][m] = dvsum[f] / 3 + U * r.var_rgb[m]
    return r


# ---------------------------------------------------------------------------------------------------------- CPU chains
def _exp2_32(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2(x.astype(np.float64)).astype(f32)


def _act32(pre, act, scaled):
    """float32 [M,n] -> the activation with correctly rounded transcendentals; scaled: pre carries the base change"""
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        if act == "softplus":
            return np.where(pre > f32(20), pre, np.log1p(FC._exp32(pre).astype(np.float64)).astype(f32)).astype(f32)
        if act == "exp":
            return _exp2_32(pre) if scaled else FC._exp32(pre)
        e = _exp2_32(pre) if scaled else FC._exp32(-pre)
        return (f32(1) / (f32(1) + e)).astype(f32)


def _rows_used(n, mut):
    """the rows of a head whose activations enter the sums, and the divisor (rows >= n: padding, contributes 0)"""
    rows, div = list(range(n)), n
    if mut == "pad_counted":
        div = LAP_ROWS
    elif mut == "div_n_minus_1":
        div = n - 1
    elif mut == "skip_last_quad":          # quad qd of block b holds rows 32 b + 8 qd + 4 h + (0..3)
        rows = [r for r in rows if r < (n - 1) // 8 * 8]
    elif mut == "half1_twice":
        rows = [r + 4 if r % 8 < 4 else r for r in rows]
    return rows, div


def _head32(v, W, b, act, fam, n, mut, head):
    """-> sum / div of p and of p^2 over the rows, float32 [M]: sequential fp32 sums (an add, an fma) in row order"""
    scaled = fam != "fp32" and head_scale(act) != 1.0
    Wk, bk = scaled_rows(W, b, act) if scaled else (W, b)
    if mut == "no_base_change" and head == "density":
        Wk, bk = W, b
    pre = FC._dense32(v, Wk, bk, fam, drop_hilo=(mut == f"drop_hilo_{head}"))
    p = _act32(pre, act, scaled)
    rows, div = _rows_used(n, mut)
    s1, s2 = np.zeros(v.shape[0], f32), np.zeros(v.shape[0], f32)
    for r in rows:
        if r < n:
            s1 = (s1 + p[:, r]).astype(f32)
            s2 = PC._fma32(p[:, r], p[:, r], s2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (s1 / f32(div)).astype(f32), (s2 / f32(div)).astype(f32)


def chain(c, fam, mut=None):
    """The whole network of a case in the family's precision on the CPU ("fp32", "f16x2", "f16"), correctly rounded
    transcendentals.  mut: one of MUTATIONS.  -> {"dens", "var_d", "var_rgb" [N], "rgb" [N,3]} float32"""
    nt, N = c.net, c.N
    H, HC = nt.w0.shape[0], nt.h1.shape[0]
    feat = PC._features32(nt, c.P32).astype(f32)
    sh = FC._sh16(c.shin).astype(f32)
    hb = FC._dense32(feat, nt.w0, nt.b0, fam)
    geo = FC._dense32(hb, nt.w1, nt.b1, fam)
    c0 = np.maximum(FC._dense32(np.concatenate([sh, geo], axis=1), nt.h0, nt.hb0, fam), f32(0))
    x = np.maximum(FC._dense32(c0, nt.h1, nt.hb1, fam), f32(0))
    set_of = c.set_of
    if mut == "prev_set":
        set_of = np.maximum(set_of - 1, 0)
    elif mut == "wave_first_set":
        set_of = set_of[np.arange(N) // 64 * 64]
    out = {"dens": np.zeros(N, f32), "var_d": np.zeros(N, f32), "rgb": np.zeros((N, 3), f32), "var_rgb": np.zeros(N, f32)}
    sel = c.sel.astype(f32)
    for st in np.unique(set_of):
        m = set_of == st
        wd, wr = c.wsd[st], c.wsr[st]
        nr = c.n if mut == "rgb_cut_at_n_lap" else c.nr
        mu, m2 = _head32(hb[m], wd[:, :H], wd[:, H], c.act, fam, c.n, mut, "density")
        if c.mask:
            masked = (mu * sel[m]).astype(f32)
            out["dens"][m] = mu if mut == "mask_unmasked_mean" else masked
            out["var_d"][m] = (m2 - masked * masked).astype(f32) if mut == "mask_var_unmasked" else f32(0)
        else:
            out["dens"][m], out["var_d"][m] = mu, (m2 - (mu * mu).astype(f32)).astype(f32)
        vs = np.zeros(int(m.sum()), f32)
        for ch in range(3):
            mu, m2 = _head32(x[m], wr[:nr, HC * ch:HC * ch + HC], wr[:nr, 3 * HC + ch], "sigmoid", fam, nr, mut, "rgb")
            out["rgb"][m, ch] = mu
            vs = (vs + np.maximum((m2 - (mu * mu).astype(f32)).astype(f32), f32(0))).astype(f32)
        out["var_rgb"][m] = (vs / f32(3)).astype(f32)
    return out


_chunked = lambda c: c.chunk > 0 and len(np.unique(c.set_of)) > 1
_straddle = lambda c: _chunked(c) and (c.set_of != c.set_of[np.arange(c.N) // 64 * 64]).any()
# mutation -> (the bound family whose chain carries it, which cases it can show on)
MUTATIONS = {
    "pad_counted": ("fp32", lambda c: c.n < LAP_ROWS),
    "skip_last_quad": ("fp32", lambda c: True),
    "half1_twice": ("fp32", lambda c: c.ws in ("spread", "tight")),
    "rgb_cut_at_n_lap": ("fp32", lambda c: c.nr != c.n),
    "prev_set": ("fp32", _chunked),
    "wave_first_set": ("fp32", _straddle),
    "div_n_minus_1": ("fp32", lambda c: c.n > 1),
    "no_base_change": ("f16x2", lambda c: c.act == "exp" and EXP2_ROWS),
    "drop_hilo_density": ("f16x2", lambda c: c.ws in ("spread", "tight")),
    "drop_hilo_rgb": ("f16x2", lambda c: c.ws in ("spread", "tight")),
    "mask_unmasked_mean": ("fp32", lambda c: c.mask and (~c.sel).any()),
    "mask_var_unmasked": ("fp32", lambda c: bool(c.mask)),
}


# ------------------------------------------------------------------------------------------------------------- cases
ALL4 = FAMILIES


def _case(net_name, R, S, n, ws="spread", nr=None, bins="nerfacto", nf=NF_LONG, iw=0, off=0, chunk=0, act="exp", mask=0,
          families=ALL4, rows_rgb=None):
    """n: n_lap; nr: n_lap_rgb as the cstruct carries it (None: n); rows_rgb: the rows ws_rgb holds (None: nr)"""
    nr = n if nr is None else nr
    return dict(net=net_name, R=R, S=S, n=n, nr=nr, rows_rgb=nr if rows_rgb is None else rows_rgb, ws=ws, bins=bins, nf=nf, iw=iw,
                off=off, chunk=chunk, act=act, mask=mask, families=families)


_NETS6 = sorted(NETS)
CASES = {f"N-{n}": _case(_NETS6[i % 6], 33, 2, n, ws=("spread", "tight")[i % 2], nf=(NF_LONG, NF_SHORT)[(i // 2) % 2])
         for i, n in enumerate(N_LAP_EDGES)}
CASES.update({
    # n_lap = 129: the heads do not fit the blobs; use_mfma requests fall back to the VALU kernel, "f16" is refused
    "N-129": _case("t", 33, 2, 129, families=("valu", "fp32", "f16x2")),
    # n_lap_rgb != n_lap, set on the cstruct over five rows of ws_rgb (VALU only: the blobs would hold all five)
    "V-n5-nr3": _case("c32", 33, 2, 5, nr=3, rows_rgb=5, families=("valu",)),
    # A: the wave and tile edges of the shapes at n_lap = 9 (tiles = ceil(R / 32) S)
    "A-r1-s1": _case("t", 1, 1, 9),
    "A-r63-s1": _case("t", 63, 1, 9, "tight", bins="uniform", nf=NF_SHORT),
    "A-r32-s2": _case("c32", 32, 2, 9),
    "A-r65-s1": _case("t-box", 65, 1, 9, "tight", nf=NF_SHORT),
    "A-r31-s7": _case("t", 31, 7, 9, bins="euclid"),
    "A-r32-s8": _case("c16", 32, 8, 9, "tight"),
    "A-r65-s3": _case("c32-box", 65, 3, 9, bins="uniform", nf=NF_SHORT),
    "A-r31-s17": _case("t", 31, 17, 9, "tight", nf=NF_SHORT),
    "A-r33-s1": _case("c16-box", 33, 1, 9, bins="euclid", nf=NF_SHORT),
    "A-r65-s11": _case("t", 65, 11, 9),
    "A-r33-s48": _case("t", 33, 48, 9, "tight"),
    # E: the pixel-patch schedule (image widths 8 and 9, without chunk sets)
    "E-w8": _case("t", 32, 3, 9, iw=8),
    "E-w8-below": _case("c16", 31, 3, 9, "tight", iw=8),
    "E-w9-offset": _case("c32", 40, 2, 9, iw=9, off=31),
    # C: per-chunk sample sets (ray g uses set g // lap_chunk_rays); chunk S % 64 != 0: a VALU wave straddles two sets
    "C-32-s1": _case("t", 70, 1, 9, off=32, chunk=32),                  # 32 samples per set; R ends inside a chunk
    "C-32-s3": _case("c32", 65, 3, 9, chunk=32),               # 96 samples per set
    "C-64-s3": _case("t-box", 100, 3, 9, off=192, chunk=64, nf=NF_SHORT),    # an offset of 3 chunks
    "C-64-s48": _case("c16", 33, 48, 9, off=32, chunk=64),              # the last ray alone in the next set
    "C-96-s1": _case("t", 100, 1, 37, off=96, chunk=96),       # 96 samples per set
    "C-96-s48": _case("c32-box", 33, 48, 5, off=64, chunk=96, nf=NF_SHORT),
    "C-64-s3-sp": _case("t", 70, 3, 33, off=64, chunk=64, act="softplus"),
    # S: the softplus density activation
    "S-n37": _case("c32", 33, 2, 37, "tight", act="softplus"),
    "S-n100": _case("t-box", 33, 3, 100, act="softplus", nf=NF_SHORT),
    "S-n8": _case("c16", 31, 2, 8, act="softplus"),
    # M: lap_mask_density with copies of the mean row
    "M-exp": _case("t", 33, 2, 9, "mean", mask=1),
    "M-exp-box": _case("c16-box", 33, 3, 33, "mean", mask=1, nf=NF_SHORT),
    "M-softplus": _case("c32", 33, 2, 37, "mean", act="softplus", mask=1),
    "M-chunks": _case("t", 65, 2, 5, "mean", mask=1, chunk=32),
    # D: planted logits
    "D-a": _case("t", 33, 2, 9, "planted-a"),
    "D-a-c16": _case("c16-box", 32, 2, 37, "planted-a", nf=NF_SHORT),
    "D-b": _case("c32", 33, 2, 9, "planted-b"),
    "D-a-softplus": _case("t-box", 31, 2, 9, "planted-a", act="softplus", nf=NF_SHORT),
    "D-b-softplus": _case("t", 33, 2, 5, "planted-b", act="softplus"),
    "D-pad": _case("t", 33, 2, 9, "planted-pad", families=("valu", "fp32")),
    # X: every live row contributes one exactly known value; the padded rows must contribute exactly 0
    "X-exp-n5": _case("t", 33, 2, 5, "exact"),
    "X-exp-n37": _case("c32-box", 32, 2, 37, "exact", nf=NF_SHORT),
    "X-exp-n96": _case("c16", 31, 2, 96, "exact"),
    "X-sp-n33": _case("t", 33, 2, 33, "exact", act="softplus"),
    "X-mask-n7": _case("t-box", 33, 2, 7, "exact", mask=1, nf=NF_SHORT),
})


def second_tile_spec(cus):
    """more tiles than 4 x the persistent grid at 3 workgroups per CU, as field_cases.second_tile_spec"""
    return _case("t", 2, 4 * 3 * cus + 8, 9, bins="uniform", nf=NF_SHORT)


def _place_rays(c, rng):
    """origins, directions, bins and from them the fp32 lists: planted points first (direction 0), then directions on the axes
    and on (+-1, +-1, +-1) / sqrt 3, the rest random (as field_cases.build)"""
    nt, R, S = c.net, c.R, c.S
    origins = rng.uniform(-1.2, 1.2, (R, 3)) if nt.aabb is None else rng.uniform(0.05, 0.95, (R, 3))
    dirs = rng.standard_normal((R, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    pts = PC.planted_points(nt)[:max(R - 14, 1) if R > 1 else 0]
    for r, (_, pt) in enumerate(pts):
        origins[r], dirs[r] = pt, 0.0
    special = FC.AXES + [tuple(v / np.sqrt(3.0) for v in d) for d in FC.DIAGS]
    for i, d in enumerate(special[:max(R - len(pts), 0)]):
        dirs[len(pts) + i] = d
    c.tags, c.n_planted = [t for t, _ in pts], len(pts)
    c.origins, c.dirs = origins.astype(f32), dirs.astype(f32)
    near, far = c.nf
    if c.bins == "euclid":
        c.sb = np.sort(rng.uniform(0.05, 2.5, (R, S + 1)), axis=1).astype(f32)
        c.near, c.far, c.lin, pos_args = -1.0, far, 0, (0.0, 1.0, 1)
    else:
        c.sb = np.sort(rng.uniform(0, 1, (R, S + 1)), axis=1).astype(f32)
        c.lin = int(c.bins == "uniform")
        c.near, c.far, pos_args = near, far, (near, far, c.lin)
    P32, sel = PC.positions32(c.origins, c.dirs, c.sb, S, *pos_args, nt.aabb)
    c.P32, c.sel = P32.reshape(-1, 3), sel.reshape(-1)
    c.shin = np.repeat(FC.sh_inputs32(c.dirs, nt.sh_remap), S, axis=0)


def build(name, spec):
    nt = net(spec["net"])
    names = sorted(CASES)
    idx = names.index(name) if name in names else len(names)
    rng = np.random.default_rng(9001 + idx)
    R, S = spec["R"], spec["S"]
    c = SimpleNamespace(name=name, net=nt, **{k: v for k, v in spec.items() if k != "net"})
    c.N = R * S
    _place_rays(c, rng)
    c.tiles, c.patch = FC.tiles_of(R, S, 0 if c.chunk else c.iw, c.off)      # per-chunk sets: 1-D tiles
    # sample sets
    if c.chunk:
        assert c.chunk % 32 == 0 and c.off % 32 == 0 and not c.iw
        c.sets = (c.off + R - 1) // c.chunk + 1
        c.set_of = np.repeat((c.off + np.arange(R)) // c.chunk, S)
    else:
        c.sets, c.set_of = 1, np.zeros(c.N, np.int64)
    c.wsd, c.wsr = weight_sets(nt, c.ws, c.n, c.rows_rgb, c.sets, c.act, 77 + idx)
    c.fallback = c.n > LAP_ROWS
    exact = reference(c, rounded=False)
    c.ref = {"fp32": exact, "f16x2": exact}
    if "f16" in c.families:
        c.ref["f16"] = reference(c, rounded=True)
    # the conditions the bounds are stated under
    live = exact.pre_d[np.isfinite(exact.pre_d)] if c.act == "exp" else np.zeros(1)
    assert live.size and -104 <= live.min() and live.max() <= 40, f"{name}: density logits [{live.min()}, {live.max()}] outside [-104, 40]"
    big = max(np.abs(a).max() for a in (nt.w0, nt.w1, nt.h0, nt.h1))
    if "f16" in c.families or "f16x2" in c.families and not c.fallback:
        big = max(big, LOG2E * max(np.abs(c.wsd).max(), np.abs(c.wsr).max()))
    assert big * 10 < F16_LIMIT, f"{name}: an operand of {big} next to the f16 limit"
    if _chunked(c):      # set-distinctness: chunk c evaluated with set c - 1 leaves the bound somewhere
        other = reference(c, rounded=False, set_shift=1)
        later = c.set_of > c.set_of.min()
        assert later.any() and (np.abs(other.rgb - exact.rgb)[later] > FACTOR_MAX * exact.b_rgb["f16x2"][later]).any(), f"{name}: the sets do not differ"
    return c


FACTOR_MAX = 8.0         # set-distinctness is asserted against a bound factor no family reaches (test_laplace_cases_cpu checks that)


@functools.lru_cache(maxsize=None)
def case(name):
    return build(name, CASES[name])


@functools.lru_cache(maxsize=None)
def second_tile_case(cus):
    return build(f"H-second-tile-{cus}", second_tile_spec(cus))


def bound_families(c):
    return sorted({"fp32" if c.fallback else BOUND_OF[f] for f in c.families})


_OUT = (("density", "dens", "dens", "b_dens"), ("density variance", "var_d", "var_d", "b_var_d"), ("rgb", "rgb", "rgb", "b_rgb"),
        ("rgb variance", "var_rgb", "var_rgb", "b_var_rgb"))


def exact_values(c):
    """the `exact` set: {output: the float32 values a kernel may store} -- sum / n (VALU) or sum * fl(1 / n) (matrix kernels) of
    n equal terms; anything else means a padded row contributed"""
    v = EXACT[c.act]
    both = lambda t, n: {float(f32(t)), float(f32(f32(n * t) * (f32(1) / f32(n))))}
    return {"dens": both(v, c.n), "rgb": both(0.5, c.nr)}


def hold(c, family, out, rows=None):
    """Every output of a result {"dens", "var_d", "var_rgb" [N], "rgb" [N,3]} (float32) of kernel family `family` ("valu",
    "fp32", "f16x2", "f16"; the CPU chains go by their bound family) against the case's float64 reference: no launch sentinel
    left, no NaN, colour variance >= 0, under lap_mask_density the density exactly 0 where sel = 0 and its variance exactly 0
    everywhere, the exact set's means exactly one of their two values, every element within its bound.  rows: a slice of the
    samples the result covers.  Asserts, and returns the worst error / bound."""
    bf = BOUND_OF.get(family, family)
    if c.fallback:
        bf = "fp32"
    rows = slice(None) if rows is None else rows
    ref, sel = c.ref[bf], c.sel[rows]
    for key in ("dens", "var_d", "rgb", "var_rgb"):
        g = np.asarray(out[key])
        assert g.dtype == f32, (key, g.dtype)
        assert not (g.view(np.uint32) == SENTINEL).any(), f"{c.name} {family}: {key} still holds the launch sentinel"
        assert not np.isnan(g).any(), f"{c.name} {family}: NaN in {key}"
    assert (np.asarray(out["var_rgb"]) >= 0).all(), f"{c.name} {family}: a negative colour variance"
    if c.mask:
        assert (np.asarray(out["dens"])[~sel] == 0).all(), f"{c.name} {family}: a masked density with sel = 0 is not exactly 0"
        nz = np.flatnonzero(np.asarray(out["var_d"]) != 0)
        assert len(nz) == 0, f"{c.name} {family}: {len(nz)} density variances under lap_mask_density are not exactly 0, first {np.asarray(out['var_d'])[nz[:4]]}"
    if c.ws == "exact":
        want = exact_values(c)
        d, g = np.asarray(out["dens"], np.float64), np.asarray(out["rgb"], np.float64)
        live = sel if c.mask else np.ones_like(sel)
        assert np.isin(d[live], sorted(want["dens"])).all(), f"{c.name} {family}: density {np.unique(d[live])[:4]} is none of {sorted(want['dens'])}: a padded row counted"
        assert np.isin(g, sorted(want["rgb"])).all(), f"{c.name} {family}: rgb {np.unique(g)[:4]} is none of {sorted(want['rgb'])}: a padded row counted"
    worst = 0.0
    for what, key, rkey, bkey in _OUT:
        got = np.asarray(out[key], np.float64)
        r, b = getattr(ref, rkey)[rows], FACTOR[bf] * getattr(ref, bkey)[bf][rows]
        assert got.shape == r.shape, (what, got.shape, r.shape)
        err = np.abs(got - r)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(err == 0, 0.0, err / b)
        bad = np.argwhere(~(err <= b))
        assert len(bad) == 0, (f"{c.name} {family}: {len(bad)} of {err.size} {what} outputs beyond their bound, first {bad[:6].tolist()}, "
                               f"worst error / bound {np.nanmax(ratio):.3g}")
        worst = max(worst, float(ratio.max()))
    return worst


def hold_ratio_unscaled(c, bf, out):
    worst = 0.0
    for _, key, rkey, bkey in _OUT:
        err = np.abs(np.asarray(out[key], np.float64) - getattr(c.ref[bf], rkey))
        b = getattr(c.ref[bf], bkey)[bf]
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.where(err == 0, 0.0, err / b).max()))
    return worst


@functools.lru_cache(maxsize=None)
def measure_chain(bf):
    """-> worst error / UNSCALED bound (factor 1) of the family's CPU chain over all cases"""
    worst = 0.0
    for name in CASES:
        c = case(name)
        if bf in bound_families(c):
            worst = max(worst, hold_ratio_unscaled(c, bf, chain(c, bf)))
    return worst


def check_coverage():
    """each edge the module's header lists is present"""
    cases = [case(k) for k in CASES]
    assert {c.net.name for c in cases} == set(NETS)
    nets = [net(k) for k in NETS]
    for layout in ("torch", "tcnn32", "tcnn16"):
        assert {t.aabb is None for t in nets if t.layout == layout} == {True, False}, "both normalisations per layout"
    assert all(8 <= t.log2T <= 12 for t in nets) and all(t.h0.shape == (64, 31) and t.w1.shape == (15, 64) for t in nets)
    edge = [c for c in cases if c.name.startswith("N-") and not c.fallback]
    assert tuple(c.n for c in edge) == N_LAP_EDGES and all((c.R, c.S) == (33, 2) and c.families == ALL4 for c in edge)
    assert {c.ws for c in edge} == {"spread", "tight"}
    big = case("N-129")
    assert big.n == LAP_ROWS + 1 and big.fallback and "f16" not in big.families
    v = case("V-n5-nr3")
    assert (v.n, v.nr, v.wsr.shape[1]) == (5, 3, 5) and v.families == ("valu",)
    a = [c for c in cases if c.n == 9 and not c.chunk]
    assert {c.R for c in a} >= {1, 31, 32, 33, 65} and {c.S for c in a} >= {1, 2, 3, 17, 48} and {c.N for c in a} >= {1, 63, 64, 65}
    assert {c.tiles for c in a if not c.patch} >= {1, 7, 8, 9, 17, 33, 96}
    spec = second_tile_spec(256)
    assert FC.tiles_of(spec["R"], spec["S"])[0] > 4 * 3 * 256 and spec["n"] == 9
    assert {c.iw for c in cases if c.patch} == {8, 9} and all(not c.chunk for c in cases if c.iw)
    assert any(c.iw and c.R == 4 * c.iw for c in cases) and any(c.iw and c.R == 4 * c.iw - 1 and not c.patch for c in cases)
    assert any(c.patch and c.off % c.iw for c in cases)
    ch = [c for c in cases if c.chunk]
    assert {c.chunk for c in ch} == {32, 64, 96} and {c.S for c in ch} >= {1, 3, 48}
    assert any((c.off + c.R) % c.chunk for c in ch), "R ends inside a chunk"
    assert any(c.off == 32 for c in ch) and any(c.off == 3 * c.chunk for c in ch)
    assert any((c.chunk * c.S) % 64 for c in ch) and any(_straddle(c) for c in ch), "a VALU wave straddles two sets"
    assert all(c.sets == c.wsd.shape[0] == c.wsr.shape[0] and c.sets > 1 for c in ch)
    assert {c.act for c in cases} == {"exp", "softplus"} and {c.act for c in cases if c.mask} == {"exp", "softplus"}
    for c in cases:
        if c.mask:
            assert (c.wsd == c.net.dmean).all() or c.ws == "exact"
            assert (~c.sel).any() and c.sel.any() and (c.ref["fp32"].var_d == 0).all() and (c.ref["fp32"].dens[~c.sel] == 0).all()
    assert {c.bins for c in cases} == {"nerfacto", "uniform", "euclid"} and {c.nf for c in cases} == {NF_LONG, NF_SHORT}
    # the weight-sample sets
    for c in cases:
        ref = c.ref["fp32"]
        if c.ws in ("spread", "tight") and c.n >= 31 and c.act == "exp":
            sd = ref.pre_d.std(axis=1).mean()
            assert (0.2 < sd < 1.0) if c.ws == "spread" else (2.0 ** -12 < sd < 2.0 ** -8), (c.name, sd)
            if c.ws == "tight":
                rel = ref.var_d / ref.dens ** 2
                assert 1e-8 < np.median(rel) < 1e-5, (c.name, np.median(rel))
    seen_d, seen_c = set(), set()
    for c in cases:
        if c.ws.startswith("planted"):
            dens, colours = PLANTS[c.ws[8:]]
            ref = c.ref["fp32"]
            for s, val in enumerate(dens):
                if c.act == "exp":
                    assert np.allclose(ref.pre_d[:, s], val, rtol=1e-12), (c.name, s)
                assert (c.wsd[:, s, :64] == 0).all() and (c.wsd[:, s, 64] == f32(val)).all()
                seen_d.add(val)
            for chn, val in enumerate(colours):
                if val is not None:
                    assert (c.wsr[:, 0, 64 * chn:64 * chn + 64] == 0).all() and (c.wsr[:, 0, 192 + chn] == f32(val)).all()
                    seen_c.add(val)
    assert seen_d == {-100.0, 0.0, 1.0, ONE_UP, 40.0} and seen_c == {0.0, 17.0, -17.0, 90.0, -90.0}
    assert f32(ONE_UP) - f32(1) == f32(2.0 ** -23)
    pad = case("D-pad")
    assert (pad.wsr[:, 2, :64] == 0).all() and (pad.wsr[:, 2, 192] == f32(LAP_PAD_BIAS)).all() and "f16" not in pad.families
    with np.errstate(over="ignore"):
        assert np.isfinite(f32(np.exp(f32(40))) ** 2) and not np.isfinite(f32(np.exp(f32(45))) ** 2)
    for c in cases:
        if c.ws == "exact":
            assert (c.wsd[..., :64] == 0).all() and (c.wsr == 0).all()
            want = exact_values(c)
            assert (np.isin(c.ref["fp32"].rgb, [0.5])).all() and float(f32(EXACT[c.act])) in want["dens"]


# =================================================================================================== Part 2: the GGN fit
# unerf_laplace_ggn_diag on the nets above, the mean last layers as ws_density[65] / ws_rgb[195], fixed random bins.
# Reference: the closed-form Jacobian of the kernel's header comment (csrc/unerf_nerf.hip 5d) in float64 on the float64
# deterministic forward (sigma = act(.) sel, c = sigmoid(.); the forward is finite for finite inputs, so nan_to_num never acts
# and no NaN is planted); diag = 2 sum over rays and channels of J^2.  tests/test_laplace_cases_cpu.py meets it with float64
# autograd once.
# Bound, per parameter, first order on absolute values:
#   dd = delta sigma: d dd = delta dsigma + 2 U dd;  em = exp(-dd): d em = em (d dd + (dd + 1) 2^-23);  A_i = sum_{j<i} dd_j:
#   dA = sum d dd + (S + 2) U A;  T = exp(-A): dT = T (dA + (A + 1) 2^-23);  w = (1 - em) T: dw = (d em + U) T + (1 - em) dT + 2 U w;
#   Tf = 1 - sum w: dTf = sum dw + (S + 2) U sum w + U;  wc = w c: d wc = dw c + w dc + U wc, its scans (S + 2) U;
#   pred = tot + Tf bg: dpred = dtot + dTf |bg| + Tf dbg + 2 U |pred|abs;
#   bracket B = em T c - (tot - incl) - Tf bg on absolute values |B|abs = em T c + (tot - incl) + Tf |bg|:
#   dB = d em T c + em dT c + em T dc + dtot + dincl + dTf |bg| + Tf dbg + 4 U |B|abs;
#   dsigma/dpre = sigma (exp: error dsigma) | 1 - exp(-sigma) (softplus: exp(-sigma) dsigma + 2 U (.));
#   g = live delta B (dsigma/dpre): dg = delta (dB |.| + |B|abs d(.)) + 4 U |g|abs;  q = live (w + [last] Tf) c (1 - c):
#   dq = (dw + [last] dTf) c (1 - c) + (w + [last] Tf) |1 - 2 c| dc + 3 U q;
#   M = sum_s g_s x_s: dM = sum (dg |x| + |g| dx) + S U sum |g x|, dsigma, dc, dx from Part 1's fp32 bound of the capture forward;
#   entry = 2 sum (2 |M| dM + dM^2) + (rays per wave + waves + 2 + 6) U entry (the 6: three channels squared and summed).
# The gate live = [0 <= pred <= 1] is a discontinuity: ggn_build() asserts that no rendered channel lies within 100 x its own
# dpred of 0 or 1 (a channel of a ray whose g and q are all exactly 0 whatever the gate is exempt: the gate multiplies zeros).
# GGN_FACTOR: 4 x the worst error / bound of the fp32 CPU chain of the kernel's formulas (ggn_chain) over all cases.
BG_LAST, BG_NONE, BG_COLOR = 0, 1, 2
GGN_WAVES_MAX = 4096
GGN_RATIO_MEASURED = 0.032
GGN_FACTOR = 0.13
CLAMP_BG = (1.5, -0.5, 0.5)
INSIDE_BG = (0.45, 0.55, 0.5)
# the tcnn32 feature bound (a rounding of p * scale at scale 7000 times the table's slope) makes dpred about 3e-3 on an opaque
# ray: its cases blend a constant inside [0, 1] over thin rays, so that the gate condition holds
NF_THIN = (0.05, 0.5)


def _ggn_case(net_name, R, S, bg=(BG_LAST, None), act="exp", bins="nerfacto", nf=NF_LONG):
    return dict(net=net_name, R=R, S=S, bg=bg, act=act, bins=bins, nf=nf)


GGN_CASES = {
    "G-r1-s64-last": _ggn_case("t", 1, 64),
    "G-r3-s17-none": _ggn_case("c16", 3, 17, (BG_NONE, None), "softplus", "uniform", NF_SHORT),
    "G-r4-s2-const": _ggn_case("c32", 4, 2, (BG_COLOR, INSIDE_BG), nf=NF_THIN),
    "G-r5-s63-clamp": _ggn_case("t-box", 5, 63, (BG_COLOR, CLAMP_BG), "softplus", nf=NF_SHORT),
    "G-r5-s1-last": _ggn_case("c16-box", 5, 1, nf=NF_SHORT),
    "G-r35-s1-none": _ggn_case("c16-box", 35, 1, (BG_NONE, None), nf=NF_SHORT),
    "G-r35-s17-clamp": _ggn_case("t", 35, 17, (BG_COLOR, CLAMP_BG), bins="uniform", nf=NF_THIN),
    "G-r35-s64-last-sp": _ggn_case("t", 35, 64, act="softplus", nf=NF_SHORT),
    "G-r35-s2-const-sp": _ggn_case("c32-box", 35, 2, (BG_COLOR, INSIDE_BG), "softplus", "uniform", NF_THIN),
    "G-r4099-s2": _ggn_case("c16", 4099, 2, nf=NF_SHORT),
}


def ggn_waves(R):
    """the waves of laplace_ggn_kernel's grid: 4 per block, ceil(R / 4) blocks capped at 1024"""
    return 4 * min(1024, max(1, (R + 3) // 4))


def ggn_workspace_floats(R, S):
    return R * S * (64 + 64 + 1 + 3) + ggn_waves(R) * 260


def _ggn_forward64(c):
    """the deterministic forward in float64 and Part 1's fp32 bound of the capture kernel's outputs"""
    nt, N = c.net, c.N
    z = lambda *shape: np.zeros(shape)
    fw = SimpleNamespace(X=z(N, 64), H=z(N, 64), dX=z(N, 64), dH=z(N, 64), sigma=z(N), dsigma=z(N), col=z(N, 3), dcol=z(N, 3))
    every, f, eye = slice(None), "fp32", np.eye(64)
    for i in range(0, N, 512):
        sl = slice(i, i + 512)
        t = trunk64(nt, c.P32[sl], c.shin[sl], rounded=False)
        fw.X[sl], fw.H[sl] = t.hb, t.x
        fw.dX[sl] = t.dfeat @ np.abs(t.W0).T + t.e0[f]
        fw.dH[sl] = carried_rgb(t, every, eye, f)
        p, dp = _head(t.hb, lambda rows, fam: carried_density(t, every, rows, fam), nt.dmean[None, :64], nt.dmean[64:], c.act, (f,))
        fw.sigma[sl], fw.dsigma[sl] = p[:, 0] * c.sel[sl], dp[f][:, 0] * c.sel[sl]
        for ch in range(3):
            p, dp = _head(t.x, lambda rows, fam: carried_rgb(t, every, rows, fam), nt.cmean[None, 64 * ch:64 * ch + 64], nt.cmean[192 + ch:193 + ch],
                          "sigmoid", (f,))
            fw.col[sl, ch], fw.dcol[sl, ch] = p[:, 0], dp[f][:, 0]
    return fw


def _excl(a):
    return np.concatenate([np.zeros_like(a[:, :1]), np.cumsum(a, axis=1)[:, :-1]], axis=1)


def ggn_reference(c, fw):
    """-> SimpleNamespace(d [65], r [195] float64, b_d, b_r the UNSCALED bounds, pred, dpred [R,3], gated [R,3] bool: the
    channels of rays on which the gate decides something)"""
    R, S = c.R, c.S
    e32 = PC.s2e32(c.sb, c.near, c.far, c.lin)
    delta = e32[:, 1:].astype(np.float64) - e32[:, :-1].astype(np.float64)
    sig, dsg = fw.sigma.reshape(R, S), fw.dsigma.reshape(R, S)
    col, dcol = fw.col.reshape(R, S, 3), fw.dcol.reshape(R, S, 3)
    X, H, dX, dH = (a.reshape(R, S, 64) for a in (fw.X, fw.H, fw.dX, fw.dH))
    last = c.bg[0] == BG_LAST
    dd = delta * sig
    ddd = delta * dsg + 3 * U * dd
    em = np.exp(-dd)
    dem = em * (ddd + (dd + 1) * 2.0 ** -23)
    A = _excl(dd)
    dA = _excl(ddd) + (S + 2) * U * A
    T = np.exp(-A)
    dT = T * (dA + (A + 1) * 2.0 ** -23)
    w = (1 - em) * T
    dw = (dem + U) * T * (dd > 0) + (1 - em) * dT + 2 * U * w
    Tf = 1 - w.sum(axis=1)
    dTf = dw.sum(axis=1) + (S + 2) * U * w.sum(axis=1) + U
    if last:
        bg, dbg = col[:, -1, :], dcol[:, -1, :]
    else:
        bg, dbg = np.broadcast_to(np.array(c.bg[1] if c.bg[0] == BG_COLOR else (0.0, 0.0, 0.0)), (R, 3)), np.zeros((R, 3))
    wc = w[..., None] * col
    dwc = dw[..., None] * col + w[..., None] * dcol + U * wc
    incl = np.cumsum(wc, axis=1)
    dincl = np.cumsum(dwc, axis=1) + (S + 2) * U * incl
    tot, dtot = incl[:, -1], dincl[:, -1]
    pred = tot + Tf[:, None] * bg
    dpred = dtot + dTf[:, None] * np.abs(bg) + Tf[:, None] * dbg + 2 * U * (tot + Tf[:, None] * np.abs(bg))
    live = ((pred >= 0) & (pred <= 1)).astype(np.float64)
    suffix = tot[:, None] - incl
    emT = (em * T)[..., None]
    B = emT * col - suffix - (Tf[:, None] * bg)[:, None]
    Babs = emT * col + suffix + (Tf[:, None] * np.abs(bg))[:, None]
    dB = ((dem * T + em * dT)[..., None] * col + emT * dcol + dtot[:, None] + dincl + (dTf[:, None] * np.abs(bg) + Tf[:, None] * dbg)[:, None]
          + 4 * U * Babs)
    if c.act == "softplus":
        ds, dds = -np.expm1(-sig), np.exp(-sig) * dsg - 2 * U * np.expm1(-sig)
    else:
        ds, dds = sig, dsg
    g0 = delta[..., None] * B * ds[..., None]                       # before the gate
    dg = delta[..., None] * (dB * ds[..., None] + Babs * dds[..., None]) + 4 * U * delta[..., None] * Babs * ds[..., None]
    wt, dwt = w.copy(), dw.copy()
    if last:
        wt[:, -1] += Tf
        dwt[:, -1] += dTf
    q0 = wt[..., None] * col * (1 - col)
    dq = dwt[..., None] * col * (1 - col) + wt[..., None] * np.abs(1 - 2 * col) * dcol + 3 * U * q0
    gated = (np.abs(g0).sum(axis=1) + np.abs(q0).sum(axis=1)) > 0
    g, q, dg, dq = (a * live[:, None, :] for a in (g0, q0, dg, dq))
    # M [R,3,65], N [R,3,65] (bias last) and their errors
    ones = np.ones((R, S, 1))
    X1, H1, dX1, dH1 = np.concatenate([X, ones], 2), np.concatenate([H, ones], 2), np.concatenate([dX, 0 * ones], 2), np.concatenate([dH, 0 * ones], 2)
    M, N = np.einsum("rsc,rsk->rck", g, X1), np.einsum("rsc,rsk->rck", q, H1)
    dM = np.einsum("rsc,rsk->rck", dg, np.abs(X1)) + np.einsum("rsc,rsk->rck", np.abs(g), dX1 + S * U * np.abs(X1))
    dN = np.einsum("rsc,rsk->rck", dq, np.abs(H1)) + np.einsum("rsc,rsk->rck", np.abs(q), dH1 + S * U * np.abs(H1))
    acc = (-(-R // ggn_waves(R)) + ggn_waves(R) + 2 + 6) * U           # + the three channels' squares and sums
    d = 2 * (M * M).sum(axis=(0, 1))
    b_d = 2 * (2 * np.abs(M) * dM + dM * dM).sum(axis=(0, 1)) + acc * d
    r = 2 * (N * N).sum(axis=0)                                        # [3,65]
    b_r = 2 * (2 * np.abs(N) * dN + dN * dN).sum(axis=0) + acc * r
    flat = lambda a: np.concatenate([a[:, :64].reshape(-1), a[:, 64]])
    return SimpleNamespace(d=d, r=flat(r), b_d=b_d, b_r=flat(b_r), pred=pred, dpred=dpred, gated=gated, live=live, Tf=Tf, M=M, N=N)


def ggn_chain(c, mut=None):
    """the capture forward and laplace_ggn_kernel's formulas in float32 on the CPU (sequential scans and sums, one wave per
    ray, the waves' partial sums added in order), correctly rounded exp / expm1.  mut: one of GGN_MUTATIONS -> {"d", "r"} float32"""
    nt, R, S = c.net, c.R, c.S
    feat = PC._features32(nt, c.P32).astype(f32)
    X = FC._dense32(feat, nt.w0, nt.b0, "fp32")
    geo = FC._dense32(X, nt.w1, nt.b1, "fp32")
    c0 = np.maximum(FC._dense32(np.concatenate([FC._sh16(c.shin).astype(f32), geo], axis=1), nt.h0, nt.hb0, "fp32"), f32(0))
    Hc = np.maximum(FC._dense32(c0, nt.h1, nt.hb1, "fp32"), f32(0))
    sig = (_act32(FC._dense32(X, nt.dmean[None, :64], nt.dmean[64:], "fp32"), c.act, False)[:, 0] * c.sel.astype(f32)).reshape(R, S)
    col = _act32(FC._dense32(Hc, nt.cmean[:192].reshape(3, 64), nt.cmean[192:], "fp32"), "sigmoid", False).reshape(R, S, 3)
    X, Hc = X.reshape(R, S, 64), Hc.reshape(R, S, 64)
    e = PC.s2e32(c.sb, c.near, c.far, c.lin)
    delta = (e[:, 1:] - e[:, :-1]).astype(f32)
    last = c.bg[0] == BG_LAST
    dd = (delta * sig).astype(f32)
    em = FC._exp32(-dd)
    T = FC._exp32(-_excl(dd).astype(f32))
    w = ((f32(1) - em) * T).astype(f32)
    Tf = (f32(1) - np.cumsum(w, axis=1, dtype=f32)[:, -1]).astype(f32)
    if c.act == "softplus" and mut != "sigma_as_softplus_derivative":
        ds = (-np.expm1(-sig.astype(np.float64))).astype(f32)
    else:
        ds = sig
    bgc = np.array(c.bg[1] if c.bg[0] == BG_COLOR else (0.0, 0.0, 0.0), f32)
    accd, accr = np.zeros((R, 65), f32), np.zeros((R, 3, 65), f32)
    for k in range(3):
        bg = col[:, -1, k] if last else np.broadcast_to(bgc[k], (R,))
        wc = (w * col[:, :, k]).astype(f32)
        incl = np.cumsum(wc, axis=1, dtype=f32)
        tot = incl[:, -1]
        pred = (tot + (Tf * bg).astype(f32)).astype(f32)
        live = np.ones(R, f32) if mut == "gate_ignored" else ((pred >= 0) & (pred <= 1)).astype(f32)
        br = (((em * T).astype(f32) * col[:, :, k]).astype(f32) - (tot[:, None] - incl).astype(f32)).astype(f32)
        br = (br - (Tf * bg).astype(f32)[:, None]).astype(f32)
        g = ((((live[:, None] * delta).astype(f32)) * br).astype(f32) * ds).astype(f32)
        wt = w.copy()
        if (last and mut != "no_tend_last") or (mut == "bg_takes_gradient" and c.bg[0] == BG_COLOR):
            wt[:, -1] = (wt[:, -1] + Tf).astype(f32)
        q = ((((live[:, None] * wt).astype(f32)) * col[:, :, k]).astype(f32) * (f32(1) - col[:, :, k])).astype(f32)
        M, N = np.zeros((R, 64), f32), np.zeros((R, 64), f32)
        for s in range(S):
            M = PC._fma32(np.broadcast_to(g[:, s:s + 1], M.shape), X[:, s], M)
            N = PC._fma32(np.broadcast_to(q[:, s:s + 1], N.shape), Hc[:, s], N)
        mb, nb = np.cumsum(g, axis=1, dtype=f32)[:, -1], np.cumsum(q, axis=1, dtype=f32)[:, -1]
        accd[:, :64] = (accd[:, :64] + (M * M).astype(f32)).astype(f32)
        accd[:, 64] = (accd[:, 64] + (mb * mb).astype(f32)).astype(f32)
        accr[:, k, :64], accr[:, k, 64] = (f32(2) * N * N).astype(f32), (f32(2) * nb * nb).astype(f32)
    accd = (f32(2) * accd).astype(f32)
    nw = ggn_waves(R)
    rays = R if mut != "second_ray_dropped" else min(R, nw)

    def reduce(per_ray):             # a wave adds its rays in order, the waves are added in order
        part = np.zeros((nw,) + per_ray.shape[1:], f32)
        for r0 in range(0, rays, nw):
            blk = per_ray[r0:min(r0 + nw, rays)]
            part[:len(blk)] = (part[:len(blk)] + blk).astype(f32)
        return np.cumsum(part, axis=0, dtype=f32)[-1]

    d, r = reduce(accd), reduce(accr)
    return {"d": d, "r": np.concatenate([r[:, :64].reshape(-1), r[:, 64]]).astype(f32)}


_clamped = lambda c: ((c.ref.live == 0) & c.ref.gated).any()
GGN_MUTATIONS = {
    "no_tend_last": lambda c: c.bg[0] == BG_LAST,
    "sigma_as_softplus_derivative": lambda c: c.act == "softplus",
    "gate_ignored": _clamped,
    "bg_takes_gradient": lambda c: c.bg[0] == BG_COLOR,
    "second_ray_dropped": lambda c: c.R > ggn_waves(c.R),
}


def ggn_build(name, spec):
    nt = net(spec["net"])
    names = sorted(GGN_CASES)
    rng = np.random.default_rng(4242 + names.index(name))
    c = SimpleNamespace(name=name, net=nt, **{k: v for k, v in spec.items() if k != "net"})
    c.N = c.R * c.S
    _place_rays(c, rng)
    c.fw = _ggn_forward64(c)
    c.ref = ggn_reference(c, c.fw)
    # the gate condition, on the reference alone
    margin = np.minimum(np.abs(c.ref.pred), np.abs(c.ref.pred - 1))
    near_gate = c.ref.gated & ~(margin > 100 * c.ref.dpred)
    assert not near_gate.any(), f"{name}: rendered channels {np.argwhere(near_gate)[:4].tolist()} within 100 x their bound of the clamp gate"
    assert np.isfinite(c.ref.b_d).all() and np.isfinite(c.ref.b_r).all()
    return c


@functools.lru_cache(maxsize=None)
def ggn_case(name):
    return ggn_build(name, GGN_CASES[name])


def ggn_ratio_unscaled(c, out):
    worst = 0.0
    for key, ref, b in (("d", c.ref.d, c.ref.b_d), ("r", c.ref.r, c.ref.b_r)):
        err = np.abs(np.asarray(out[key], np.float64) - ref)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.where(err == 0, 0.0, err / b).max()))
    return worst


def ggn_hold(c, out):
    """{"d" [65], "r" [195]} float32: no NaN, every entry >= 0 and within its bound.  Asserts, returns the worst error / bound"""
    for key, n in (("d", 65), ("r", 195)):
        g = np.asarray(out[key])
        assert g.dtype == f32 and g.shape == (n,) and np.isfinite(g).all() and (g >= 0).all(), (c.name, key)
    worst = ggn_ratio_unscaled(c, out) / GGN_FACTOR
    for key, ref, b in (("d", c.ref.d, c.ref.b_d), ("r", c.ref.r, c.ref.b_r)):
        err = np.abs(np.asarray(out[key], np.float64) - ref)
        bad = np.flatnonzero(~(err <= GGN_FACTOR * b))
        assert len(bad) == 0, f"{c.name}: {len(bad)} entries of ggn_{key} beyond their bound, first {bad[:6].tolist()}, worst error / bound {worst:.3g}"
    return worst


@functools.lru_cache(maxsize=None)
def ggn_measure_chain():
    return max(ggn_ratio_unscaled(ggn_case(k), ggn_chain(ggn_case(k))) for k in GGN_CASES)


def ggn_check_coverage():
    cases = [ggn_case(k) for k in GGN_CASES]
    assert {c.S for c in cases} >= {1, 2, 17, 63, 64} and {c.R for c in cases} >= {1, 3, 4, 5, 35, 4099}
    big = ggn_case("G-r4099-s2")
    assert big.S == 2 and ggn_waves(big.R) == GGN_WAVES_MAX < big.R, "some waves take a second ray"
    assert {c.bg[0] for c in cases} == {BG_LAST, BG_NONE, BG_COLOR}
    inside = [c for c in cases if c.bg[0] == BG_COLOR and all(0 <= v <= 1 for v in c.bg[1])]
    assert inside and all((c.ref.live == 1).all() for c in inside)
    clamp = [c for c in cases if c.bg[1] == CLAMP_BG]
    assert clamp and all(_clamped(c) for c in clamp)
    for c in clamp:      # whole channels removed on both sides, and the middle one kept
        dead = (c.ref.live == 0) & c.ref.gated
        assert (c.ref.pred[dead[:, 0], 0] > 1).any() and (c.ref.pred[dead[:, 1], 1] < 0).any() and (c.ref.live[:, 2] == 1).all()
    assert {c.act for c in cases} == {"exp", "softplus"} and {c.bins for c in cases} == {"nerfacto", "uniform"}
    assert {c.net.layout for c in cases} == {"torch", "tcnn32", "tcnn16"}
    # (S = 1 under the last-sample background renders C = c_0 whatever the density: the density Jacobian vanishes identically)
    assert all(((c.ref.d > 0).any() or (c.S == 1 and c.bg[0] == BG_LAST)) and (c.ref.r > 0).any() for c in cases)
    assert any(c.S == 1 and c.bg[0] == BG_LAST and c.ref.d.max() <= 1e-25 for c in cases)
