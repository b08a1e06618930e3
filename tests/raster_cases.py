"""Hand-built rasteriser cases (plain module: tests import it; nothing here needs a GPU).

The rasteriser takes any (gaussian_ids_sorted, tile_bins): a listed splat need not overlap its tile.  So the per-tile lists are
written by hand and every edge of raster_kernel (csrc/unerf_splat.hip) is placed exactly: list lengths around the 256-splat
staging batch and the two-splats-per-trip walk, pixels that stop at chosen list offsets, splats whose alpha = 1/255 contour
ends at a quadrant border, tiles that hang over the image, narrow tiles.

Every case is deterministic (seeded), built in numpy and cached.  After building, the float64 reference
(oracle.splat_oracle.rasterize_f64) names the splats with a (pixel, splat) pair on which fp32 and float64 could decide
differently (alpha on 1/255, sigma on 0, transmittance on 1e-4); their opacity is set to 0 -- they stay in their lists, so no
list length changes -- and this repeats until none is left.  A case is then free of pairs where a 1-ulp difference flips a
decision, and a GPU result can be held to the reference on EVERY pixel.  The builder asserts, on the reference alone, that at
most 3 % of the splats were zeroed in at most 3 rounds, that no stopper was, and the structural facts of each case.

A case `c` holds 8 colour channels (`colors`, and `colors2` for the bounded pass) and its references WITHOUT background:
c.ref = (pix [H,W,8] f64, final_T f64, final_idx, n_blended) and c.ref32 = SO.rasterize's (pix, final_T, final_idx).  Channels
blend independently, so the reference of a C-channel call is the first C channels; `expected` adds a background."""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import splat_oracle as SO

NCH = 8
LENGTHS = (0, 1, 2, 255, 256, 257, 512, 513, 3, 700, 64, 65)       # row-major over the 3 x 4 tiles of a 41 x 57 image
LONG = {255: 3, 256: 4, 257: 5, 512: 6, 513: 7, 700: 9}            # list length -> tile
# Case B: the whole-tile stopper pairs, list offsets per list length
STOP_PAIRS = {255: (253, 254), 256: (254, 255), 257: (255, 256), 512: (256, 257), 513: (510, 512), 700: (300, 699)}
MAX_ZEROED, MAX_ROUNDS = 0.03, 3


def tiles_of(H, W, bw=16):
    return (W + bw - 1) // bw, (H + bw - 1) // bw


def conic_of(s1, s2, th):
    """conic (a, b, c) of the Gaussian with axes s1, s2 (px) at angle th: sigma = (a dx^2 + c dy^2) / 2 + b dx dy"""
    s1, s2, th = (np.asarray(v, np.float64) for v in (s1, s2, th))
    c, s = np.cos(th), np.sin(th)
    sxx, sxy, syy = c * c * s1 * s1 + s * s * s2 * s2, c * s * (s1 * s1 - s2 * s2), s * s * s1 * s1 + c * c * s2 * s2
    det = sxx * syy - sxy * sxy
    return np.stack([syy / det, -sxy / det, sxx / det], -1).astype(np.float32)


def _origins(H, W, bw):
    tbx, tby = tiles_of(H, W, bw)
    t = np.arange(tbx * tby)
    return np.stack([bw * (t % tbx), bw * (t // tbx)], 1).astype(np.float64)


def _crowd(rng, n, lengths, H, W, bw):
    """n random splats, each with a home tile: centre within -6 .. +22 px of the home tile's origin, axes 0.6 .. 6 px with
    ratio 0.3 .. 1 at any angle, opacity 10 % from [0, 0.0045], 40 % from [0.01, 0.3], 50 % from [0.3, 1]"""
    home = rng.integers(0, len(lengths), n)
    xys = (_origins(H, W, bw)[home] + rng.uniform(-6, 22, (n, 2))).astype(np.float32)
    s1 = rng.uniform(0.6, 6, n)
    conics = conic_of(s1, s1 * rng.uniform(0.3, 1, n), rng.uniform(0, np.pi, n))
    u, v = rng.random(n), rng.random(n)
    opac = np.where(u < 0.1, 0.0045 * v, np.where(u < 0.5, 0.01 + 0.29 * v, 0.3 + 0.7 * v)).astype(np.float32)
    return home, xys, conics, opac


def _lists(rng, home, lengths):
    """per tile: about two thirds of the list from the tile's own splats (all of them where the tile has fewer: a long list is
    mostly splats that lie elsewhere, so the crowd leaves most pixels alive to its end), the rest arbitrary ones, shuffled
    -> (ids, bins [tiles, 2]; an empty tile is (0, 0), as the sort leaves it)"""
    ids, bins, off = [], np.zeros((len(lengths), 2), np.int32), 0
    for t, L in enumerate(lengths):
        if L == 0:
            continue
        own = np.nonzero(home == t)[0]
        mine = rng.choice(own, min(round(2 * L / 3), len(own)), replace=False)
        rest = rng.choice(np.setdiff1d(np.arange(len(home)), mine), L - len(mine), replace=False)
        ids.append(rng.permutation(np.concatenate([mine, rest])))
        bins[t] = (off, off + L)
        off += L
    return np.concatenate(ids).astype(np.int32), bins


def _finish(c, seed, protected=()):
    """colours, the zeroing rounds and the cached references"""
    rng = np.random.default_rng([seed, 77])
    c.N = len(c.opac)
    c.colors = (c.color_floor + (1 - c.color_floor) * rng.random((c.N, NCH))).astype(np.float32)
    c.colors2 = rng.random((c.N, NCH)).astype(np.float32)
    c.bg = rng.random(NCH).astype(np.float32)
    c.protected = np.asarray(sorted(protected), np.int64)
    zeroed = []
    for c.rounds in range(MAX_ROUNDS + 1):
        ref = SO.rasterize_f64(c.gids, c.bins, c.xys, c.conics, c.colors, c.opac, c.H, c.W, bw=c.bw)
        graze = ref[4]
        if len(graze) == 0:
            break
        assert c.rounds < MAX_ROUNDS, f"{c.name}: splats still graze after {MAX_ROUNDS} rounds: {graze}"
        assert not np.isin(graze, c.protected).any(), f"{c.name}: a placed splat grazes: {np.intersect1d(graze, c.protected)}"
        c.opac[graze] = 0
        zeroed += list(graze)
    c.zeroed = np.asarray(zeroed, np.int64)
    assert len(c.zeroed) <= MAX_ZEROED * c.N, f"{c.name}: {len(c.zeroed)} of {c.N} splats zeroed"
    c.ref = ref[:4]
    c.ref32 = SO.rasterize(c.gids, c.bins, c.xys, c.conics, c.colors, c.opac, c.H, c.W, bw=c.bw)
    for a in vars(c).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    for a in c.ref + c.ref32:
        a.setflags(write=False)
    return c


def _new(name, H, W, bw, lengths, gids, bins, xys, conics, opac, color_floor=0.0):
    assert len(lengths) == np.prod(tiles_of(H, W, bw)) and np.array_equal(bins[:, 1] - bins[:, 0], lengths)
    return SimpleNamespace(name=name, H=H, W=W, bw=bw, lengths=tuple(lengths), gids=gids, bins=bins, xys=xys, conics=conics,
                           opac=opac, color_floor=color_floor)


# Seeds: of the first ten, the one whose case needed the fewest zeroed splats (a choice made on the reference alone; most of the
# ten meet the builder's conditions; the others need a fourth round or zero 28 .. 41 splats)
SEEDS = {"A41x57": 2, "A40x56": 4, "A16x16": 7, "A1x1": 0, "D8": 3, "D5": 7}


def _crowd_case(name, H, W, bw, lengths, n=900):
    rng = np.random.default_rng([H, W, bw, len(lengths), SEEDS.get(name, 0)])
    home, xys, conics, opac = _crowd(rng, n, lengths, H, W, bw)
    gids, bins = _lists(rng, home, lengths)
    return _new(name, H, W, bw, lengths, gids, bins, xys, conics, opac)


@functools.lru_cache(maxsize=None)
def case_a(H=41, W=57):
    """"lists": 41 x 57 is 3 x 4 tiles whose last row and column are 9 pixels deep (quadrant row / column 1 holds one pixel
    line); 40 x 56 leaves those quadrants wholly outside; 16 x 16 and 1 x 1 are one tile"""
    lengths = {(41, 57): LENGTHS, (40, 56): LENGTHS, (16, 16): (257,), (1, 1): (2,)}[(H, W)]
    return _finish(_crowd_case(f"A{H}x{W}", H, W, 16, lengths), 1)


@functools.lru_cache(maxsize=None)
def case_b():
    """"termination": case A with the crowd's opacities capped at 0.02 (so the crowd alone leaves T >= 0.25 everywhere), and
    stoppers written into chosen list positions.  A stopper's alpha clamps to 0.999; of a pair, the first blends (T >= 0.25
    -> nT >= 2.5e-4) and the second stops (nT <= 1e-6), so final_idx is the first one's position.
      * whole-tile pairs (flat, 300 px, opacity 2) at STOP_PAIRS: the stop falls on the last entry of a batch, the first of the
        next, either side of them, and in the last entry of a 700 list;
      * a quadrant-local pair (1.6 px, opacity 50, centred in quadrant 0) at offsets 10 and 20 of each long tile.  Its alpha
        clamps within 4.47 px of the centre, which leaves the quadrant's corner pixels (4.95 px) alive;
      * so that a quadrant does finish early, the 700 tile has a second such pair of opacity 200 (clamps within 5.2 px: the
        whole of quadrant 0) at offsets 30 and 40: quadrant 0 is done in batch 0, keeps staging for the others, and its wave
        leaves every later walk at once;
      * so that a workgroup does leave before its last batch, the 513 tile has a third whole-tile stopper at offset 511: every
        pixel is done when batch 2 (the entry at 512) would be staged."""
    c = _crowd_case("A41x57", 41, 57, 16, LENGTHS)       # the same seeds: case A's geometry and lists
    c.name = "B"
    c.opac = np.minimum(c.opac, np.float32(0.02))
    T0 = SO.rasterize_f64(c.gids, c.bins, c.xys, c.conics, np.zeros((len(c.opac), 1), np.float32), c.opac, c.H, c.W)[1]
    assert T0.min() >= 0.25, f"crowd-only transmittance {T0.min():.3f}"
    org = _origins(c.H, c.W, 16)
    xys, conics, opac, gids = list(c.xys), list(c.conics), list(c.opac), c.gids.copy()

    def place(tile, offset, xy, scale, op):
        gids[c.bins[tile, 0] + offset] = len(opac)
        xys.append(np.asarray(xy, np.float32)), conics.append(np.float32([1 / scale ** 2, 0, 1 / scale ** 2])), opac.append(op)

    for L, tile in LONG.items():
        for off in STOP_PAIRS[L]:
            place(tile, off, org[tile] + 8, 300.0, 2.0)
        for off in (10, 20):
            place(tile, off, org[tile] + 4, 1.6, 50.0)
    for off in (30, 40):
        place(LONG[700], off, org[LONG[700]] + 4, 1.6, 200.0)
    place(LONG[513], 511, org[LONG[513]] + 8, 300.0, 2.0)
    n0 = len(c.opac)
    c.gids, c.xys, c.conics, c.opac = gids, np.stack(xys), np.stack(conics), np.asarray(opac, np.float32)
    _finish(c, 2, protected=range(n0, len(opac)))
    fidx, tbx = c.ref[2], tiles_of(c.H, c.W)[0]
    win = lambda t: fidx[16 * (t // tbx):16 * (t // tbx) + 16, 16 * (t % tbx):16 * (t % tbx) + 16]
    for L in (255, 256, 257, 512, 513):               # pixels that stop with the first stopper as their last blended splat
        assert (win(LONG[L]) == c.bins[LONG[L], 0] + STOP_PAIRS[L][0]).any(), L
    t, r0 = LONG[700], c.bins[LONG[700], 0]
    assert win(t)[:8, :8].max() < r0 + 256, "quadrant 0 of the 700 tile must finish within batch 0"
    live = win(t).copy()
    live[:8, :8] = 0
    assert (live >= r0 + 512).any(), "another quadrant of the 700 tile must blend in batch 2"
    assert win(LONG[513]).max() == c.bins[LONG[513], 0] + 510, "every pixel of the 513 tile must stop before batch 2"
    return c


@functools.lru_cache(maxsize=None)
def case_c():
    """"quadrant mask": 32 x 32, 28 low-opacity splats per tile, colours >= 0.25, final T >= 0.5 on every pixel -- so a pair
    that raster_quad_mask culled wrongly moves a pixel by >= 0.25 * 0.5 / 255 = 4.9e-4, a hundred tolerances.
      * 18 per tile: centres at the tile's x0 + {7.5, 8.0, 8.5} and the same in y (twice each), sized so that the bounding box
        of the alpha = 1/255 contour ends within +-0.3 px of the pixel centres next to the quadrant border (x0 + 7.5, x0 + 8.5):
        the comparisons of the mask decide either way;
      * two 45-degree needles; opacities in (0.0039, 1/255) (pass the mask's early-out, blend nowhere) and in [0.00393, 0.0041]
        (blend on one pixel); opacity 0; an all-zero conic (alpha = opacity everywhere; no ellipse: no culling); an indefinite
        conic (b = 5) centred on a pixel centre; a wide splat centred 40 px outside its tile.  No NaN inputs."""
    H = W = 32
    rng = np.random.default_rng(3)
    xys, conics, opac, gids, special = [], [], [], [], []
    tau = lambda o: np.log(255.0 * o)

    def add(xy, conic, op, keep=False):
        if keep:
            special.append(len(opac))
        gids.append(len(opac))
        xys.append(np.asarray(xy, np.float32)), conics.append(np.asarray(conic, np.float32)), opac.append(op)

    for org in _origins(H, W, 16):
        first = len(gids)
        for cx in (7.5, 8.0, 8.5):
            for cy in (7.5, 8.0, 8.5):
                for _ in range(2):
                    # half-extents of the contour's box: up to the border pixel centre on the far side (or either, from 8.0)
                    hx, hy = (abs((8.5 if v <= 8.0 else 7.5) - v) + rng.uniform(-0.3, 0.3) for v in (cx, cy))
                    op, rho = rng.uniform(0.01, 0.04), rng.uniform(-0.6, 0.6)
                    sx, sy = hx / np.sqrt(2 * tau(op)), hy / np.sqrt(2 * tau(op))     # box half-width = sqrt(2 tau) sx
                    det = sx * sx * sy * sy * (1 - rho * rho)
                    add(org + (cx, cy), (sy * sy / det, -rho * sx * sy / det, sx * sx / det), op)
        for th in (np.pi / 4, 3 * np.pi / 4):
            add(org + rng.uniform(6, 10, 2), conic_of(8.0, 0.5, th), 0.05, keep=True)
        for op in (0.003902, 0.003912):
            add(org + rng.uniform(2, 14, 2), conic_of(3.0, 2.0, 0.3), op, keep=True)
        for op, cell in ((0.00393, (3, 12)), (0.0041, (12, 3))):
            add(org + np.add(cell, 0.5), conic_of(0.3, 0.3, 0.0), op, keep=True)
        add(org + (5.0, 5.0), conic_of(3.0, 3.0, 0.0), 0.0)
        add(org + (8.0, 8.0), (0.0, 0.0, 0.0), 0.02, keep=True)
        add(org + (10.5, 5.5), (1.0, 5.0, 1.0), 0.03, keep=True)
        add(org + (8.0, -40.0), conic_of(25.0, 25.0, 0.0), 0.05, keep=True)
        gids[first:] = list(np.asarray(gids[first:])[rng.permutation(len(gids) - first)])
    n = len(gids) // 4
    assert n <= 40
    bins = np.stack([n * np.arange(4), n * np.arange(1, 5)], 1).astype(np.int32)
    c = _new("C", H, W, 16, (n,) * 4, np.asarray(gids, np.int32), bins, np.stack(xys), np.stack(conics),
             np.asarray(opac, np.float32), color_floor=0.25)
    _finish(c, 3, protected=special)
    assert c.ref[1].min() >= 0.5, f"final T {c.ref[1].min():.3f}"
    return c


@functools.lru_cache(maxsize=None)
def case_d(bw):
    """"narrow tiles": 19 x 21 with block_width 8 (3 x 3 tiles, 64 threads of the workgroup own a pixel) and 5 (4 x 5 tiles,
    25 threads): the row-major thread-to-pixel mapping, which never culls"""
    H, W = 19, 21
    ntile = int(np.prod(tiles_of(H, W, bw)))
    return _finish(_crowd_case(f"D{bw}", H, W, bw, tuple((0, 1, 257)[t % 3] for t in range(ntile))), 4)


def expected(c, chans, background=None, ref=None, ref32=None):
    """-> (image f64, image of the fp32 oracle) of the case's colour channels `chans` (a list, or a count: the first ones) over
    `background` [len(chans)]"""
    chans = list(range(chans)) if isinstance(chans, int) else list(chans)
    pix, T = (ref or c.ref)[:2]
    pix32, T32 = (ref32 or c.ref32)[:2]
    if background is None:
        return pix[..., chans], pix32[..., chans]
    bg = np.asarray(background, np.float32)
    return pix[..., chans] + T[..., None] * bg.astype(np.float64), pix32[..., chans] + T32[..., None] * bg


@functools.lru_cache(maxsize=None)
def bounded_ref(c_key):
    """the bounded pass of a case on its second colour set, stopping where the reference's first pass ended
    -> (rasterize_f64's tuple, SO.rasterize's tuple), both without background"""
    c = ALL[c_key]()
    a = (c.gids, c.bins, c.xys, c.conics, c.colors2, c.opac, c.H, c.W)
    return (SO.rasterize_f64(*a, bw=c.bw, stop_idx=c.ref[2])[:4], SO.rasterize(*a, bw=c.bw, stop_idx=c.ref[2]))


ALL = {"A41x57": case_a, "A40x56": lambda: case_a(40, 56), "A16x16": lambda: case_a(16, 16), "A1x1": lambda: case_a(1, 1),
       "B": case_b, "C": case_c, "D8": lambda: case_d(8), "D5": lambda: case_d(5)}
