"""Hand-placed cases for the any-width field kernel (plain module: tests import it; nothing here needs a GPU).

In scope: field_kernel_generic<ACTIVE | MCDROPOUT | LAPLACE> (csrc/unerf_nerf.hip section 5a'), reached through ops.field_fwd
on a FieldDev.from_torch of a net whose widths are not nerfacto's 64 / 64 / 15 / 2 / 16 (or whose appearance embedding is not 32
wide under UNERF_DROP_HEADIN): one lane per sample, four [rows][64] activation buffers in LDS (rows = generic_rows, restated
here), eight outputs per sweep of a layer's inputs (dense_any), the counter masks applied per unit pair (mask_any).  Out of
scope, as for the kernel itself: explicit masks, several views, the f16 forms.

Nets (`NETS`; random `plain` weights of field_cases._linear, a non-zero appearance vector, log2T 8 .. 10, so every level of
the torch layout wraps).  `check_inventory` asserts what they cover.  Statements about code that runs before the kernel splits
by mode (the levels, the three grid layouts, the launch shapes, the normalisations) are checked over all cases; statements
about the layers are checked per mode:
  * H, HC, the trunk's OUT1 (G + 2 ACTIVE, G + 1 MCDROPOUT) and the LAPLACE geo layer (G outputs) each take a value in every
    residue class {0, 1, 7} mod 8 and one below 8; G = 31 and G = 64 (the cap);
  * L in {1, 2, 15, 17, 32} with F = 2; L in {1, 16, 32} with F = 4 (torch layout; L F = 128 is the widest row);
  * generic_rows = max(L F, H, HC, 16 + G + AD, G + 2): each of the first four is the strict maximum in some net.  G + 2 never
    is: 16 + G + AD > G + 2 for every AD >= 0 (and the host reads AD = 0 as 32), so that term is dead in the maximum; the
    inventory asserts this instead, and the G + 2 rows of the trunk output are covered by G = 64;
  * torch, tcnn fp32 rows and tcnn half rows with other widths than nerfacto's; tcnn nets have a dense and a hashed level, and
    the case T-wrap holds points in the last z-cell of a dense level (b00 + res + res^2 + 1 >= size: the whole wave then
    takes the wrap branch instead of the paired loads) next to points that are not;
  * LDS: rows = 65 (just above 64 KiB, the hipFuncSetAttribute path), H = HC = 128 (the dropout-site limit) and rows = 160
    (163,840 bytes: exactly the cap field_check_nonempty accepts).
Launch shapes: N = R S in {1, 63, 64, 65, 129} from S in {1, 3} (and 2 x 48 = 96: S = 48 has no multiple among them),
ray_offset in {0, 5}, K in {0, 1, 3}; nerfacto and uniform spacing, Euclidean pass-through bins; contraction and scene box.
Every case of more than one ray plants rays whose samples have sel = 0 first, then prop_cases.planted_points (direction 0),
directions on the axes and diagonals, the rest random.  MCDROPOUT: the default site pair, TRUNK alone, HEAD0 | HEAD1, HEADIN
with AD in {8, 32, 33} (29, 54, 56 and 80 units: odd and even, and pairs beyond 31), a site of exactly 128 units; p_drop 0.2
and 2^-18 (every unit kept and still scaled).  LAPLACE: (n_lap, n_lap_rgb) in {(1, 1), (5, 7), (3, 0)} (0: the rgb count
defaults to n_lap), lap_softplus, lap_mask_density, and stacked sets with lap_chunk_rays = 6, ray_offset = 4, 5 sets.

Reference: field_cases.reference (ACTIVE, MCDROPOUT) and laplace_cases.reference (LAPLACE), which take the widths from the net:
fp32 lists up to the normalised position and the SH inputs, float64 on the fp32 weights from there, features with the
oracle's own corners (half rows: O.tcnn_hash_encode_half), the appearance block folded in float64 (unfolded under HEADIN), masks
from O.mc_keep_mask generated for n + (n & 1) units and sliced.  No sample is exempt; a density with sel = 0 is exactly 0 --
except the LAPLACE density without lap_mask_density, which upstream does not mask.

Bounds: field_cases' per-output "fp32" bound and laplace_cases' moment bounds, with the widths of the net.  One constant per
reference multiplies them: 4 x the worst error / bound of a CPU chain over all cases here (`chain`: fp32 fma chains in input
order -- eight outputs per sweep changes no output's own order --, x * scale for the masks, correctly rounded transcendentals)
against the float64 reference, never against a kernel (RATIO_MEASURED, FACTOR; tests/test_width_cases_cpu.py re-measures)."""
import functools
import zlib
from types import SimpleNamespace

import numpy as np
import torch

import field_cases as FC
import laplace_cases as LC
import prop_cases as PC
from oracle import nerf_oracle as O

f32 = np.float32
ACTIVE, MCDROPOUT, LAPLACE = 0, 1, 2
TRUNK, HEAD0, HEAD1, HEADIN = FC.TRUNK, FC.HEAD0, FC.HEAD1, FC.HEADIN
SENTINEL = FC.SENTINEL
NF_LONG, NF_SHORT = PC.NF_LONG, PC.NF_SHORT
LDS_CAP_ROWS = 160                       # field_check_nonempty: rows * 64 lanes * 4 buffers * 4 bytes <= 160 KiB
# worst error / unscaled bound of the CPU chain over all cases (against float64, never a kernel), and 4 x it rounded up
RATIO_MEASURED = {"field": 0.281, "laplace": 0.127}
FACTOR = {"field": 1.13, "laplace": 0.51}

# name: (layout, log2T, scene box, L, F, H, HC, G, AD)
NETS = {
    "a": ("torch", 8, False, 1, 2, 7, 8, 5, 8),
    "b": ("torch", 9, True, 2, 2, 8, 1, 6, 32),
    "c": ("tcnn32", 8, True, 15, 2, 9, 23, 7, 33),
    "d": ("tcnn16", 9, False, 17, 2, 1, 7, 8, 8),            # L F = 34 is the strict maximum
    "e": ("tcnn32", 10, False, 2, 2, 33, 9, 9, 4),           # H = 33 is
    "f": ("torch", 10, False, 32, 2, 16, 15, 31, 33),        # 16 + G + AD = 80 is
    "h": ("torch", 9, True, 16, 4, 64, 64, 15, 32),          # nerfacto's widths but for F = 4
    "i": ("torch", 10, False, 32, 4, 24, 16, 15, 32),        # L F = 128, the widest row
    "j": ("torch", 8, False, 1, 4, 8, 7, 64, 8),             # G = 64, the cap: trunk outputs 66 / 65
    "k": ("tcnn32", 9, True, 15, 2, 31, 65, 7, 32),          # HC = 65 is the strict maximum: 66,560 bytes of LDS
    "m": ("torch", 8, False, 2, 2, 128, 128, 15, 32),        # the dropout-site limit: 128 KiB
    "n": ("torch", 8, True, 2, 2, 160, 8, 7, 8),             # rows = 160: exactly the cap
    "w": ("tcnn16", 9, True, 2, 2, 9, 7, 7, 8),              # both levels dense: the wrap case
}


def generic_rows(L, F, H, HC, G, AD):
    """the host's generic_rows: the widest activation (field_set_widths reads an appearance width of 0 as 32)"""
    return max(L * F, H, HC, 16 + G + (AD or 32), 1 + G + 1)


def widest_activation(nt, mode, headin):
    """the rows any of the four LDS buffers holds at one time: the features, the hidden units, the trunk output (density,
    geo, beta), the head input (with the appearance rows under HEADIN) and the colour head's units"""
    out1 = {ACTIVE: nt.G + 2, MCDROPOUT: nt.G + 1, LAPLACE: nt.G}[mode]
    return max(nt.L * nt.F, nt.H, out1, 16 + nt.G + (nt.AD if headin else 0), nt.HC, 3)


@functools.lru_cache(maxsize=None)
def net(name, lap=False):
    """name -> SimpleNamespace: the grid as prop_cases' nets carry it and the fp32 weights in torch [out, in] layout: w0
    [H, L F], w1 [G + 2, H] (row 0 density, 1 .. G geo, G + 1 beta: MCDROPOUT uses the first G + 1), h0 [HC, 16 + G + AD],
    h1 [HC, HC], h2 [3, HC], app [AD].  lap: the Laplace shape of the same widths -- w0 a bare Linear, w1 [G, H], no appearance
    block, and the mean last layers dmean [H + 1], cmean [3 HC + 3]"""
    layout, log2T, box, L, F, H, HC, G, AD = NETS[name]
    rng = np.random.default_rng(zlib.crc32(f"net-{name}-{int(lap)}".encode()))       # per name: a net added later moves no other
    c = SimpleNamespace(name=name + ("-lap" if lap else ""), L=L, F=F, H=H, HC=HC, G=G, AD=0 if lap else AD, layout=layout, log2T=log2T,
                        kind="plain", levels=None, scalings=None, n_dense=0, dense=None, dense_off=(), dense_dim=(),
                        aabb=(0.0, 0.0, 0.0, 1.0, 1.0, 1.0) if box else None, sh_remap=int(layout != "torch"))
    if layout == "torch":
        c.scalings = O.hash_scalings(L, 16, 512).numpy().astype(f32)
        assert np.all(c.scalings == np.floor(c.scalings)) and (c.scalings[0] + 1) ** 3 > (1 << log2T), "every level wraps"
        c.table = (rng.standard_normal((L << log2T, F)) * 0.5).astype(f32)
    else:
        assert F == 2
        c.levels = O.tcnn_grid_levels(L, 5, 1.5, log2T)
        c.table = (rng.standard_normal((c.levels[-1][2] + c.levels[-1][3], 2)) * 0.5).astype(f32)
    c.w0, c.b0 = FC._linear(rng, H, L * F, 2.0)
    c.w1, c.b1 = FC._linear(rng, G if lap else G + 2, H, 1.5)
    c.h0, c.hb0 = FC._linear(rng, HC, 16 + G + c.AD, 1.5)
    c.h1, c.hb1 = FC._linear(rng, HC, HC, 1.5)
    c.h2, c.hb2 = FC._linear(rng, 3, HC, 3.0)
    c.app = (rng.standard_normal(c.AD) * 0.5).astype(f32)
    c.app[np.abs(c.app) < 0.05] = f32(0.05)
    if lap:
        dw, db = FC._linear(rng, 1, H, 1.0)
        c.dmean = np.concatenate([dw.reshape(-1), db]).astype(f32)
        c.cmean = np.concatenate([c.h2.reshape(-1), c.hb2]).astype(f32)
    c.rows = generic_rows(L, F, H, HC, G, c.AD)
    return c


def weight_sets(nt, n, rows_rgb, sets, seed, mean_only=False):
    """-> ws_density [sets, n, H + 1], ws_rgb [sets, rows_rgb, 3 HC + 3] float32: the mean rows + 0.1 x noise"""
    rng = np.random.default_rng(seed)
    wsd = (nt.dmean[None, None] + 0.1 * rng.standard_normal((sets, n, nt.H + 1))).astype(f32)
    wsr = (nt.cmean[None, None] + 0.1 * rng.standard_normal((sets, rows_rgb, 3 * nt.HC + 3))).astype(f32)
    if mean_only:
        wsd[:] = nt.dmean
    return wsd, wsr


# --------------------------------------------------------------------------------------------------------------- masks
UNITS = {TRUNK: lambda nt: nt.H, HEAD0: lambda nt: nt.HC, HEAD1: lambda nt: nt.HC, HEADIN: lambda nt: 16 + nt.G + nt.AD}


def generator_masks(nt, seed, K, p, sites, first_sample, N):
    """{site bit: bool [K, N, units]} the counter generator's keep masks -- O.mc_keep_mask for n + (n & 1) units, sliced, as
    O.mcdropout_outputs takes them; {} when the generator drops nothing"""
    if not FC.masks_generated(K, p):
        return {}
    sidx = (np.arange(N, dtype=np.uint64) + np.uint64(first_sample)).astype(np.uint32)
    out = {}
    for b in (TRUNK, HEAD0, HEAD1, HEADIN):
        if FC.site_set(sites) & b:
            n = UNITS[b](nt)
            out[b] = np.stack([O.mc_keep_mask(seed, k, sidx, FC.STREAM[b], n + (n & 1), float(f32(p)))[:, :n] for k in range(K)])
    return out


def _chain_mask(nt, seed, k, p, site, sidx, mut):
    """the keep mask of one site and pass as mask_any forms it (one word per unit pair: the low half keeps unit 2 j, the high
    half unit 2 j + 1), restated on the oracle's primitives so that a mutation can be planted"""
    n, stream = UNITS[site](nt), FC.STREAM[site]
    pairs = (n + 1) // 2
    with np.errstate(over="ignore"):
        pre = O._hash32(sidx.astype(np.uint32)) + O._hash32(np.array([seed], dtype=np.uint32))
        b = np.stack([O._hash32(pre + np.uint32(h) * O.GOLDEN) for h in (0, 1)], axis=0)
        j = np.arange(pairs, dtype=np.uint32)
        jc = j if mut == "const_at_j" else j & ~np.uint32(2)
        A = (O._hash32(np.uint32(0xA5A50000) + np.uint32(64 * stream) + jc) & np.uint32(0xFFFFFE)) | np.uint32(1)
        B = (O._hash32(np.uint32(0x5A5A0000) + np.uint32(64 * stream) + jc) & np.uint32(0xFFFFFE)) | np.uint32(1)
        half = np.zeros_like(j) if mut == "bit1_base0" else (j >> np.uint32(1)) & np.uint32(1)
        bb = b[half].T
        r = ((bb & np.uint32(0xFFFFFF)) * A[None, :] + (bb >> np.uint32(8)) * B[None, :]).astype(np.uint32)
    for _ in range(k - 1 if (mut == "prev_pass" and k > 0) else k):
        r = O._mask_step(r)
    thr = np.uint32(FC.mask_threshold(p))
    lo = ((r & np.uint32(0xFFFF)) ^ np.uint32(0x8000)) < thr
    hi = ((r >> np.uint32(16)) ^ np.uint32(0x8000)) < thr
    keep = np.stack([lo, hi], axis=-1).reshape(r.shape[0], 2 * pairs)
    if n & 1:
        if mut == "odd_unmasked":
            keep[:, n - 1] = True
        elif mut == "odd_other_half":        # unit n - 1 = 2 j sits in the LOW half of word j: the defect is reading the high one
            keep[:, n - 1] = keep[:, n]
    return keep[:, :n]


# ---------------------------------------------------------------------------------------------------------- CPU chains
def _dense8(x, w, b, drop_tail=False):
    """dense_any: per output one fp32 fma chain over the inputs in order, eight outputs per sweep.  drop_tail: the last,
    partial group of outputs is never computed (its rows keep 0)"""
    y = FC._dense32(x.astype(f32), w, b, "fp32")
    if drop_tail and w.shape[0] % 8:
        y[:, w.shape[0] // 8 * 8:] = 0
    return y


def _features32(c, mut):
    nt = c.net
    feat = PC._features32(nt, c.P32).astype(f32)
    if mut == "skip_last_level":
        feat[:, nt.F * (nt.L - 1):] = 0
    elif mut == "swap_f23":
        for l in range(nt.L):
            feat[:, [4 * l + 2, 4 * l + 3]] = feat[:, [4 * l + 3, 4 * l + 2]]
    return feat


def chain(c, mut=None):
    """The whole network of a case in the kernel's precision and order on the CPU, correctly rounded transcendentals.
    mut: one of MUTATIONS.  -> the result dict `hold` takes"""
    if c.mode == LAPLACE:
        out = LC.chain(_lap_view(c, mut), "fp32", LAP_MUT.get(mut))
        return {"dens": out["dens"][None], "rgb": out["rgb"][None], "var_d": out["var_d"], "var_rgb": out["var_rgb"]}
    nt, N, B = c.net, c.N, c.B
    G, INC = nt.G, 16 + nt.G
    on = FC.site_set(c.sites) if (c.mode == MCDROPOUT and c.K > 0) else 0
    scale = f32(1.0) / (f32(1.0) - f32(c.p))            # the host's drop_scale, in float
    out1 = G + 2 if c.mode == ACTIVE else G + 1
    sidx = (np.arange(N, dtype=np.uint64) + np.uint64(c.first_sample)).astype(np.uint32)
    masked_sites = FC.masks_generated(c.K, c.p)

    def masked(x, site, k):
        if not on & site:
            return x
        xs = (x * scale).astype(f32)
        if not masked_sites:             # the keep-every-unit bit: scaled, nothing dropped
            return xs
        return np.where(_chain_mask(nt, c.seed, k, c.p, site, sidx, mut), xs, f32(0)).astype(f32)

    sh = FC._sh16(c.shin).astype(f32)
    hb0 = (nt.hb0.astype(np.float64) + nt.h0[:, INC:].astype(np.float64) @ nt.app.astype(np.float64)).astype(f32)
    h = np.maximum(_dense8(_features32(c, mut), nt.w0, nt.b0, mut == "drop_tail_H"), f32(0))
    res = {"dens": np.zeros((B, N), f32), "rgb": np.zeros((B, N, 3), f32), "beta": None}
    sel = np.ones(N, f32) if mut == "no_sel" else c.sel.astype(f32)
    for k in range(B):
        t = _dense8(masked(h, TRUNK, k), nt.w1[:out1], nt.b1[:out1], mut == "drop_tail_OUT1")
        geo = t[:, 0:G] if mut == "geo_row_g" else t[:, 1:1 + G]
        if on & HEADIN:
            app = np.zeros((N, nt.AD), f32) if mut == "no_app_rows" else np.broadcast_to(nt.app, (N, nt.AD))
            c0 = _dense8(masked(np.concatenate([sh, geo, app], axis=1).astype(f32), HEADIN, k), nt.h0, nt.hb0, mut == "drop_tail_HC")
        else:
            c0 = _dense8(np.concatenate([sh, geo], axis=1), nt.h0[:, :INC], hb0, mut == "drop_tail_HC")
        c1 = _dense8(masked(np.maximum(c0, f32(0)), HEAD0, k), nt.h1, nt.hb1, mut == "drop_tail_HC")
        c2 = _dense8(masked(np.maximum(c1, f32(0)), HEAD1, k), nt.h2, nt.hb2)
        res["dens"][k] = (f32(FC.AVG) * FC._exp32(t[:, 0])) * sel
        with np.errstate(divide="ignore"):
            res["rgb"][k] = f32(1) / (f32(1) + FC._exp32(-c2))
        if c.mode == ACTIVE:
            u = t[:, G] if mut == "beta_row_G" else t[:, G + 1]
            with np.errstate(over="ignore"):
                sp = np.where(u > f32(20), u, np.log1p(FC._exp32(u).astype(np.float64)).astype(f32))
            res["beta"] = (sp + f32(FC.BETA_MIN)).astype(f32)
    return res


def _lap_view(c, mut):
    """the case as laplace_cases.chain reads it; the width mutations of the shared trunk are planted in a copy of the net"""
    if mut not in ("drop_tail_H", "drop_tail_HC", "drop_tail_GEO", "skip_last_level", "swap_f23"):
        return c
    nt = SimpleNamespace(**vars(c.net))
    cut = lambda w, b: (np.concatenate([w[:w.shape[0] // 8 * 8], 0 * w[w.shape[0] // 8 * 8:]]), np.concatenate([b[:len(b) // 8 * 8], 0 * b[len(b) // 8 * 8:]]))
    if mut == "drop_tail_H":
        nt.w0, nt.b0 = cut(nt.w0, nt.b0)
    elif mut == "drop_tail_GEO":
        nt.w1, nt.b1 = cut(nt.w1, nt.b1)
    elif mut == "drop_tail_HC":
        nt.h0, nt.hb0 = cut(nt.h0, nt.hb0)
        nt.h1, nt.hb1 = cut(nt.h1, nt.hb1)
    elif mut == "skip_last_level":       # the features of level L - 1 never reach the first layer
        nt.w0 = nt.w0.copy()
        nt.w0[:, nt.F * (nt.L - 1):] = 0
    else:
        nt.w0 = nt.w0.copy()
        for l in range(nt.L):
            nt.w0[:, [4 * l + 2, 4 * l + 3]] = nt.w0[:, [4 * l + 3, 4 * l + 2]]
    return SimpleNamespace(**{**vars(c), "net": nt})


# mutation of this module's chain -> the mutation of laplace_cases.chain that states the same defect
LAP_MUT = {"rgb_from_n_lap": "rgb_cut_at_n_lap", "first_lane_set": "wave_first_set", "no_sel": "mask_unmasked_mean"}
_fld = lambda c: c.mode != LAPLACE
_mc = lambda c: c.mode == MCDROPOUT and bool(c.keeps)
_odd = lambda c: _mc(c) and any(k.shape[-1] & 1 for k in c.keeps.values())
_tail = lambda n: n % 8 != 0
# mutation -> which cases it can show on
MUTATIONS = {
    "drop_tail_H": lambda c: _tail(c.net.H),
    "drop_tail_HC": lambda c: _tail(c.net.HC),
    "drop_tail_OUT1": lambda c: _fld(c) and _tail(c.net.G + (2 if c.mode == ACTIVE else 1)),
    "drop_tail_GEO": lambda c: c.mode == LAPLACE and _tail(c.net.G),
    "odd_unmasked": _odd,
    "odd_other_half": _odd,
    "bit1_base0": lambda c: _mc(c) and any(k.shape[-1] > 4 for k in c.keeps.values()),
    "const_at_j": lambda c: _mc(c) and any(k.shape[-1] > 4 for k in c.keeps.values()),
    "prev_pass": lambda c: _mc(c) and c.K > 1,
    "geo_row_g": _fld,
    "beta_row_G": lambda c: c.mode == ACTIVE,
    "no_app_rows": lambda c: _mc(c) and bool(FC.site_set(c.sites) & HEADIN),
    "skip_last_level": lambda c: True,
    "swap_f23": lambda c: c.net.F == 4,
    "rgb_from_n_lap": lambda c: c.mode == LAPLACE and c.nr != c.n,
    "first_lane_set": lambda c: c.mode == LAPLACE and c.chunk > 0,
    "no_sel": lambda c: (_fld(c) or c.mask) and not c.sel.all(),
}


# ------------------------------------------------------------------------------------------------------------- cases
def _case(net_name, mode, R, S, bins="nerfacto", nf=NF_LONG, off=0, K=0, sites=0, p=0.2, seed=1234, n=0, nr=0, act="exp", mask=0, chunk=0,
          rays="mixed"):
    return dict(net=net_name, mode=mode, R=R, S=S, bins=bins, nf=nf, off=off, K=K, sites=sites, p=p, seed=seed, n=n, nr=nr, act=act, mask=mask,
                chunk=chunk, rays=rays)


A, M, Lp = ACTIVE, MCDROPOUT, LAPLACE
CASES = {
    # A: ACTIVE
    "A-a-n1": _case("a", A, 1, 1),
    "A-a-n63": _case("a", A, 63, 1, nf=NF_SHORT),
    "A-b-n63": _case("b", A, 21, 3, "uniform", NF_SHORT),
    "A-c-n65": _case("c", A, 65, 1, "euclid"),
    "A-d-n129": _case("d", A, 43, 3),
    "A-e-n129": _case("e", A, 43, 3, "uniform"),
    "A-f-n64-off": _case("f", A, 64, 1, off=5),
    "A-h-n96": _case("h", A, 2, 48, nf=NF_SHORT),
    "A-i-n65": _case("i", A, 65, 1),
    "A-j-n63-off": _case("j", A, 21, 3, off=5),
    "A-k-lds65": _case("k", A, 65, 1, nf=NF_SHORT),
    "A-m-lds128": _case("m", A, 63, 1),
    "A-n-lds160": _case("n", A, 65, 1, nf=NF_SHORT),
    # M: MCDROPOUT
    "M-a-k1": _case("a", M, 63, 1, K=1),
    "M-b-k3-off": _case("b", M, 43, 3, nf=NF_SHORT, off=5, K=3),
    "M-c-k3-trunk": _case("c", M, 65, 1, K=3, sites=TRUNK),
    "M-c-k1-head01": _case("c", M, 21, 3, "uniform", K=1, sites=HEAD0 | HEAD1),
    "M-d-k3": _case("d", M, 64, 1, "euclid", K=3),
    "M-a-k3-headin": _case("a", M, 65, 1, K=3, sites=HEADIN | TRUNK | HEAD1),
    "M-b-k1-headin": _case("b", M, 63, 1, nf=NF_SHORT, K=1, sites=HEADIN),
    "M-c-k3-headin-off": _case("c", M, 43, 3, off=5, K=3, sites=15),
    "M-f-k1-headin": _case("f", M, 65, 1, K=1, sites=HEADIN | HEAD0),
    "M-m-k1-128": _case("m", M, 64, 1, K=1, sites=7),
    "M-b-k0": _case("b", M, 65, 1, nf=NF_SHORT, K=0),
    "M-a-k0-headin": _case("a", M, 21, 3, K=0, sites=HEADIN | HEAD0),         # the site asked for and no pass: the folded first colour layer
    "M-c-k3-p2^-18": _case("c", M, 21, 3, K=3, sites=15, p=2.0 ** -18),
    "M-h-k1": _case("h", M, 2, 48, nf=NF_SHORT, K=1),
    "M-j-k1": _case("j", M, 63, 1, K=1),
    "M-e-k1": _case("e", M, 21, 3, "uniform", K=1),
    "M-k-k1-lds65": _case("k", M, 65, 1, nf=NF_SHORT, K=1),
    # L: LAPLACE
    "L-a-1-1": _case("a", Lp, 63, 1, n=1, nr=1),
    "L-b-5-7-sp": _case("b", Lp, 43, 3, nf=NF_SHORT, n=5, nr=7, act="softplus"),
    "L-c-3-0-mask": _case("c", Lp, 65, 1, n=3, nr=0, mask=1),
    "L-d-5-7": _case("d", Lp, 64, 1, "euclid", n=5, nr=7),
    "L-e-1-1-sp-mask": _case("e", Lp, 21, 3, "uniform", n=1, nr=1, act="softplus", mask=1),
    "L-c-chunks": _case("c", Lp, 26, 3, off=4, n=5, nr=7, chunk=6),
    "L-i-n1": _case("i", Lp, 1, 1, n=3, nr=0),
    "L-k-lds65": _case("k", Lp, 65, 1, nf=NF_SHORT, n=5, nr=7),
    "L-n-lds160": _case("n", Lp, 65, 1, nf=NF_SHORT, n=1, nr=1),
    # T: a dense tcnn level's last cell: rays 0 .. 39 stay away from the wrap, rays 40 .. 63 sit in the last z-cell
    "T-wrap-a": _case("w", A, 64, 1, nf=NF_SHORT, rays="wrap"),
    "T-wrap-m": _case("w", M, 64, 1, nf=NF_SHORT, K=1, rays="wrap"),
    "T-wrap-c32": _case("c", A, 64, 1, nf=NF_SHORT, rays="wrap"),
}
WRAP_CLEAR = 40                          # the rays of a T-wrap case that are away from the wrap


def wraps(nt, P32):
    """[N] bool: the sample makes a dense tcnn level take the wrap branch (b00 + res + res^2 + 1 >= size), for its whole wave"""
    hit = np.zeros(P32.shape[0], bool)
    for scale, res, _, size, dense in nt.levels or ():
        if dense:
            cell = np.floor((P32.astype(np.float64) * float(f32(scale)) + 0.5).astype(f32)).astype(np.int64)
            hit |= cell[:, 0] + cell[:, 1] * res + cell[:, 2] * res * res + res + res * res + 1 >= size
    return hit


def _zero_sel_points(nt):
    if nt.aabb is None:
        return [("far", (3e8, 1.0, -1.0)), ("far", (-3e8, 2.0, 0.5))]
    return [("p0", (0.0, 0.3, 0.6)), ("p1", (0.3, 1.0, 0.6))]


def _place_rays(c, rng):
    nt, R, S = c.net, c.R, c.S
    origins = rng.uniform(-1.2, 1.2, (R, 3)) if nt.aabb is None else rng.uniform(0.05, 0.95, (R, 3))
    dirs = rng.standard_normal((R, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    if c.rays == "wrap":                 # direction 0 in a unit box: the position is the origin.  z below / inside the last cell of level 0
        assert nt.aabb is not None
        pz = np.concatenate([rng.uniform(0.05, 0.55, WRAP_CLEAR), rng.uniform(0.9, 0.97, R - WRAP_CLEAR)])
        pxy = rng.uniform(0.05, 0.55, (R, 2))
        origins, dirs = np.concatenate([pxy, pz[:, None]], axis=1), np.zeros((R, 3))
        pts = []
    else:
        zeros = _zero_sel_points(nt)[:min(2, R // 2)]
        rest = [pt for pt in PC.planted_points(nt) if pt not in zeros][:max(R - 14 - len(zeros), 0)]
        pts = zeros + rest
        for r, (_, pt) in enumerate(pts):
            origins[r], dirs[r] = pt, 0.0
        special = FC.AXES + [tuple(v / np.sqrt(3.0) for v in d) for d in FC.DIAGS]
        for i, d in enumerate(special[:max(R - len(pts), 0)] if R > 1 else []):
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
    nt = net(spec["net"], lap=spec["mode"] == LAPLACE)
    idx = zlib.crc32(name.encode())           # per name, so that a case added later moves no other case's rays
    rng = np.random.default_rng(idx)
    c = SimpleNamespace(name=name, net=nt, **{k: v for k, v in spec.items() if k != "net"})
    c.N, c.B = c.R * c.S, max(c.K, 1) if c.mode == MCDROPOUT else 1
    c.family = "laplace" if c.mode == LAPLACE else "field"
    c.headin = c.mode == MCDROPOUT and bool(FC.site_set(c.sites) & HEADIN)
    _place_rays(c, rng)
    c.first_sample = c.off * c.S
    c.keeps = generator_masks(nt, c.seed, c.K, c.p, c.sites, c.first_sample, c.N) if c.mode == MCDROPOUT else {}
    if c.mode == LAPLACE:
        c.nr_rows = c.nr or c.n                                # the rows of ws_rgb, and the count the kernel takes when told 0
        c.nr_arg, c.nr = c.nr, c.nr_rows
        if c.chunk:
            c.sets = (c.off + c.R - 1) // c.chunk + 1
            c.set_of = np.repeat((c.off + np.arange(c.R)) // c.chunk, c.S)
        else:
            c.sets, c.set_of = 1, np.zeros(c.N, np.int64)
        c.wsd, c.wsr = weight_sets(nt, c.n, c.nr_rows, c.sets, idx + 91, mean_only=bool(c.mask))
        c.ref = LC.reference(c, rounded=False)
        live = c.ref.pre_d[np.isfinite(c.ref.pre_d)]
        assert -104 <= live.min() and live.max() <= 40, f"{name}: density logits"
    else:
        c.ref = FC.reference(nt, c.mode, c.P32, c.sel, c.shin, c.K if c.mode == MCDROPOUT else 0, c.p, c.sites, c.keeps, rounded=False)
        assert np.abs(c.ref.o).max() < 110 and np.isfinite(c.ref.dens).all(), f"{name}: logits"
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    return build(name, CASES[name])


def items(c, factor=None):
    """-> [(what, key, reference, bound)]: every output of the case with its float64 reference and its SCALED bound"""
    k = FACTOR[c.family] if factor is None else factor
    r = c.ref
    if c.mode == LAPLACE:
        return [("density", "dens", r.dens[None], k * r.b_dens["fp32"][None]), ("rgb", "rgb", r.rgb[None], k * r.b_rgb["fp32"][None]),
                ("density variance", "var_d", r.var_d, k * r.b_var_d["fp32"]), ("rgb variance", "var_rgb", r.var_rgb, k * r.b_var_rgb["fp32"])]
    out = [("density", "dens", r.dens, k * r.b_dens["fp32"]), ("rgb", "rgb", r.rgb, k * r.b_rgb["fp32"])]
    if c.mode == ACTIVE:
        out.append(("beta", "beta", r.beta, k * r.b_beta["fp32"]))
    return out


def _cut(a, rows):
    return a[:, rows] if a.ndim >= 2 else a[rows]


def ratio_unscaled(c, out):
    """worst error / UNSCALED bound of a result"""
    worst = 0.0
    for _, key, r, b in items(c, 1.0):
        err = np.abs(np.asarray(out[key], np.float64) - r)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.where(err == 0, 0.0, err / b).max()))
    return worst


def hold(c, out, rows=None):
    """Every output of a result ({"dens" [B,N], "rgb" [B,N,3]} and "beta" [N] (ACTIVE) or "var_d", "var_rgb" [N] (LAPLACE),
    float32) against the case's float64 reference: no launch sentinel left, no NaN, a density with sel = 0 exactly 0 (LAPLACE:
    under lap_mask_density, where the density variance is exactly 0 too), colour variances >= 0, every element within its bound.
    rows: a slice of the samples the result covers.  Asserts, and returns the worst error / bound."""
    rows = slice(None) if rows is None else rows
    sel = c.sel[rows]
    for _, key, _, _ in items(c):
        g = np.asarray(out[key])
        assert g.dtype == f32, (key, g.dtype)
        assert not (g.view(np.uint32) == SENTINEL).any(), f"{c.name}: {key} still holds the launch sentinel"
        assert not np.isnan(g).any(), f"{c.name}: NaN in {key}"
    if c.mode != LAPLACE or c.mask:
        assert (np.asarray(out["dens"])[:, ~sel] == 0).all(), f"{c.name}: a density with sel = 0 is not exactly 0"
    if c.mode == LAPLACE:
        assert (np.asarray(out["var_rgb"]) >= 0).all(), f"{c.name}: a negative colour variance"
        if c.mask:
            assert (np.asarray(out["var_d"]) == 0).all(), f"{c.name}: a density variance under lap_mask_density is not exactly 0"
    worst = 0.0
    for what, key, r, b in items(c):
        got = np.asarray(out[key], np.float64)
        r, b = _cut(r, rows), _cut(b, rows)
        assert got.shape == r.shape, (what, got.shape, r.shape)
        err = np.abs(got - r)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(err == 0, 0.0, err / b)
        bad = np.argwhere(~(err <= b))
        assert len(bad) == 0, (f"{c.name}: {len(bad)} of {err.size} {what} outputs beyond their bound, first {bad[:6].tolist()}, "
                               f"worst error / bound {np.nanmax(ratio):.3g}")
        worst = max(worst, float(ratio.max()))
    return worst


@functools.lru_cache(maxsize=None)
def measure_chain(family):
    """-> worst error / UNSCALED bound of the CPU chain over all cases of the family ("field" | "laplace")"""
    return max(ratio_unscaled(case(k), chain(case(k))) for k in CASES if case(k).family == family)


def oracle_params(c):
    """the case's net as the oracle's FieldParams (fp32 torch functions that take their shapes from the weights)"""
    nt = c.net
    if c.mode != LAPLACE:
        return FC.field_params(nt, c.mode)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    g = O.GridMLP(table=t(nt.table), scalings=None if nt.scalings is None else t(nt.scalings), log2_T=nt.log2T, weights=[t(nt.w0)],
                  biases=[t(nt.b0)], tcnn_levels=nt.levels, aabb=None if nt.aabb is None else t(np.array(nt.aabb, f32).reshape(2, 3)),
                  grid_half=nt.layout == "tcnn16")
    return O.FieldParams(grid=g, head_w=[t(nt.h0), t(nt.h1)], head_b=[t(nt.hb0), t(nt.hb1)], appearance=torch.zeros(0), hidden_w=t(nt.w1),
                         hidden_b=t(nt.b1), geo_feat_dim=nt.G, sh_remap=bool(nt.sh_remap), density_activation=c.act)


# ---------------------------------------------------------------------------------------------------------- inventory
def check_inventory():
    """what the header says the nets and cases cover"""
    cases = [case(k) for k in CASES]
    res = lambda vals: ({v % 8 for v in vals}, min(vals))
    for mode in (ACTIVE, MCDROPOUT, LAPLACE):
        mine = [c for c in cases if c.mode == mode]
        out1 = {ACTIVE: lambda nt: nt.G + 2, MCDROPOUT: lambda nt: nt.G + 1, LAPLACE: lambda nt: nt.G}[mode]
        for what, vals in (("H", [c.net.H for c in mine]), ("HC", [c.net.HC for c in mine]), ("OUT1", [out1(c.net) for c in mine])):
            classes, low = res(vals)
            assert classes >= {0, 1, 7} and low < 8, (mode, what, sorted(set(vals)))
        rows = {c.net.name: (c.net.L * c.net.F, c.net.H, c.net.HC, 16 + c.net.G + (c.net.AD or 32)) for c in mine}
        strict = {int(np.argmax(v)) for v in rows.values() if sorted(v)[-1] > sorted(v)[-2]}
        assert strict >= ({0, 1, 2} if mode == LAPLACE else {0, 1, 2, 3}), (mode, rows)      # (no appearance block under LAPLACE)
        assert any(c.net.rows == 65 for c in mine), mode
    for name in NETS:
        for lap in (False, True):
            nt = net(name, lap)
            assert nt.G + 2 < 16 + nt.G + (nt.AD or 32) and nt.rows <= LDS_CAP_ROWS and 8 <= nt.log2T <= 10
            assert lap or np.abs(nt.app).min() > 0
    for c in cases:
        assert c.net.rows >= widest_activation(c.net, c.mode, c.headin), c.name
    assert {c.net.G for c in cases} >= {31, 64}
    assert {c.net.L for c in cases if c.net.F == 2} >= {1, 2, 15, 17, 32}
    assert {c.net.L for c in cases if c.net.F == 4} == {1, 16, 32} and all(c.net.layout == "torch" for c in cases if c.net.F == 4)
    assert max(c.net.L * c.net.F for c in cases) == 128
    for layout in ("torch", "tcnn32", "tcnn16"):
        assert any(c.net.layout == layout and (c.net.H, c.net.HC, c.net.G) != (64, 64, 15) for c in cases), layout
    for c in cases:
        if c.net.levels and c.net.L > 2:
            assert any(lv[4] for lv in c.net.levels) and not all(lv[4] for lv in c.net.levels), "dense and hashed tcnn levels"
    assert any(c.net.rows == 128 and c.net.H == c.net.HC == 128 and c.mode == ACTIVE for c in cases)
    assert any(c.net.rows == LDS_CAP_ROWS and c.mode in (ACTIVE, LAPLACE) for c in cases)
    assert {c.N for c in cases} >= {1, 63, 64, 65, 129, 96} and {c.S for c in cases} == {1, 3, 48} and {c.off for c in cases} >= {0, 5}
    assert {c.bins for c in cases} == {"nerfacto", "uniform", "euclid"} and {c.net.aabb is None for c in cases} == {True, False}
    for c in cases:
        if c.rays == "wrap":
            w = wraps(c.net, c.P32)
            assert not w[:WRAP_CLEAR].any() and w[WRAP_CLEAR:].all() and c.sel.all(), c.name
        elif c.R > 1:
            assert (~c.sel).sum() >= 2 and c.sel.any(), c.name
            assert all((np.atleast_2d(c.ref.dens)[:, r * c.S] == 0).all() for r in range(min(2, c.R // 2)) if c.mode != LAPLACE or c.mask)
    assert {c.net.layout for c in cases if c.rays == "wrap"} == {"tcnn32", "tcnn16"}
    mc = [c for c in cases if c.mode == MCDROPOUT]
    assert {c.K for c in mc} >= {0, 1, 3} and {FC.site_set(c.sites) for c in mc} >= {TRUNK | HEAD1, TRUNK, HEAD0 | HEAD1}
    assert {c.net.AD for c in mc if c.headin} == {8, 32, 33}
    units = {k.shape[-1] for c in mc for k in c.keeps.values()}
    assert 128 in units and any(u & 1 for u in units) and max(c.keeps[HEADIN].shape[-1] for c in mc if HEADIN in c.keeps) > 64
    assert {(16 + c.net.G + c.net.AD) & 1 for c in mc if c.headin} == {0, 1}
    assert {c.p for c in mc} == {0.2, 2.0 ** -18} and FC.mask_threshold(2.0 ** -18) == 65536 and FC.drop_scale(3, 2.0 ** -18) > 1
    assert all(not c.keeps for c in mc if c.K == 0 or c.p < 0.1)
    for c in mc:
        for k in c.keeps.values():
            assert 0.5 < k.mean() < 1 and not k.all()
    lap = [c for c in cases if c.mode == LAPLACE]
    assert {(c.n, c.nr_arg) for c in lap} == {(1, 1), (5, 7), (3, 0)} and {c.act for c in lap} == {"exp", "softplus"} and {c.mask for c in lap} == {0, 1}
    ch = [c for c in lap if c.chunk]
    assert len(ch) == 1 and (ch[0].chunk, ch[0].off, ch[0].sets) == (6, 4, 5)
    assert len(np.unique(ch[0].set_of[:64])) > 2, "a 64-sample workgroup spans several sets"
