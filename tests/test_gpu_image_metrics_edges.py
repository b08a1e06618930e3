"""unerf_image_metrics at its block and table edges: the paths of csrc/unerf_metrics.hip that the image-sized cases of
tests/test_gpu_image_metrics.py never reach -- inputs below one wave / workgroup / sort tile (64 / 256 / 4096) and one to
either side, C = 2 and 4, more than 1024 sort tiles (ms_rowscan's carry from one 1024-entry chunk to the next), valid
pixels only in the last tile, nothing valid, the caller's own ratio / threshold tables (128 entries, one entry, out of
order, duplicates, ratios outside [0, 1], a cut on the last segsum block's end), non-finite inputs, every flag subset, a
dirty and reused scratch arena, keys over the whole float32 range including denormals and exact zeros, SSIM interiors of
one row / one column / one tile / one past a tile, and a side stream.

The reference is `restate_row` / `ssim_sum_f64` of tests/test_metrics_abi_cpu.py (float32 error definitions, float64 sums,
torch.sort(stable=True) on the CPU; its table handling is pinned there against a brute-force loop).  Gates, as in
tests/test_gpu_image_metrics.py: float64 sums of non-negative terms 1e-9 relative (another order moves them by at most
n 2^-53 = 4.7e-10 at the largest n here, 4 198 401); NLL 1e-9 of the sum of the terms' magnitudes; n_valid, the non-finite
count, min / max and the AUCE counts equal; raw AUSE sums 1e-9 relative, and exactly 0 where the restatement is exactly 0;
SSIM 1e-9 on the mean index.  Every slot that is not asked for or not used is exactly 0.  Each check prints its worst
difference per family and the worst of the file so far."""
import functools

import numpy as np
import pytest
import torch

import test_metrics_abi_cpu as R

pytestmark = pytest.mark.gpu

TILE = 4096                                                                  # MS_TILE of csrc/unerf_metrics.hip
_WORST = {"sums": 0.0, "nll": 0.0, "ause": 0.0, "ssim": 0.0}


def _pixels(n, Cc, seed, masked=False, keep=0.5):
    """seeded random pixels [n, Cc]: predictions above 1, sigma == 0 with and without a residual, a mask keeping `keep`"""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(n, Cc, generator=g)
    std = 0.02 + 0.2 * torch.rand(n, generator=g)
    pred = gt + std[:, None] * torch.randn(n, Cc, generator=g) + 0.05
    std[3:60:7] = 0.0
    std[5:80:9] = 0.0
    pred[5:80:9] = gt[5:80:9]
    mask = (torch.rand(n, generator=g) < keep) if masked else None
    return pred, gt, std, mask


def _params(Cc):
    return (1.0, 3e-2) if Cc % 2 else (float("inf"), 0.1)                    # (clip_max, nll_min_sigma)


def _flags_no_ssim():
    from uncertainty_nerf_gs_amd import lib as L
    return L.METRICS_ALL & ~L.METRICS_SSIM


def _rel(got, want):
    return abs(got - want) / max(abs(want), 1e-300)


def _note(kind, v):
    _WORST[kind] = max(_WORST[kind], float(v))


def _check_row(row, ref, ex, what, n_z=99, n_r=100, ssim=False):
    """the whole row against the restatement, every gate of the module docstring; the SSIM pair is the caller's"""
    from uncertainty_nerf_gs_amd import lib as L
    a0, s0 = L.METRICS_AUCE_OFF, L.METRICS_AUSE_OFF
    assert row[0] == ref[0] == ex["n"] and row[1] == 0.0, (what, row[:2], ref[:2])
    worst = 0.0
    for j, name in ((2, "sum sq"), (3, "sum ab"), (4, "sum var"), (5, "sum sigma"), (6, "sum sq64")):
        worst = max(worst, _rel(row[j], ref[j]))
        assert _rel(row[j], ref[j]) <= 1e-9 and (ref[j] != 0 or row[j] == 0), (what, name, row[j], ref[j])
    d_nll = abs(row[7] - ref[7])
    nll_share = d_nll / ex["nll_abs_sum"] if ex["nll_abs_sum"] > 0 else 0.0
    assert d_nll <= 1e-9 * ex["nll_abs_sum"], (what, row[7], ref[7])
    np.testing.assert_array_equal(row[8:12], ref[8:12], err_msg=what + " min / max")
    np.testing.assert_array_equal(row[a0:a0 + n_z], ref[a0:a0 + n_z], err_msg=what + " AUCE counts")
    fam_worst = []
    for f in range(4):
        got, want = row[s0 + 128 * f:s0 + 128 * f + n_r], ref[s0 + 128 * f:s0 + 128 * f + n_r]
        w = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))
        fam_worst.append(w)
        assert w <= 1e-9, (what, f, w)
        assert np.all(got[want == 0] == 0), (what, f, "a sum that is exactly 0")
        assert np.all(row[s0 + 128 * f + n_r:s0 + 128 * (f + 1)] == 0), (what, f, "slots behind n_ratios")
    assert np.all(row[14:16] == 0) and np.all(row[a0 + n_z:s0] == 0), (what, "unused slots")
    if not ssim:
        assert row[12] == 0 and row[13] == 0, what
    _note("sums", worst), _note("nll", nll_share), _note("ause", max(fam_worst))
    print(f"[{what}] n_valid {int(row[0])}: plain sums rel {worst:.2e}, nll {nll_share:.2e} of sum|terms|, AUSE raw sums rel "
          + " ".join(f"{w:.2e}" for w in fam_worst) + f"; counts and min / max equal | file so far: sums {_WORST['sums']:.2e} "
          f"nll {_WORST['nll']:.2e} ause {_WORST['ause']:.2e} ssim {_WORST['ssim']:.2e}")


def _run(dev, pred, gt, std, mask, clip, min_sigma, flags, **kw):
    from uncertainty_nerf_gs_amd import ops
    dmask = None if mask is None else mask.to(dev)
    return ops.image_metrics(pred.to(dev), gt.to(dev), std.to(dev), dmask, clip_max=clip, nll_min_sigma=min_sigma, flags=flags, **kw)


def _run_twice(dev, pred, gt, std, mask, clip, min_sigma, flags, **kw):
    a = _run(dev, pred, gt, std, mask, clip, min_sigma, flags, **kw)
    b = _run(dev, pred, gt, std, mask, clip, min_sigma, flags, **kw)
    assert torch.equal(a, b), "two calls on the same inputs: the reductions run in a fixed order"
    return a.cpu().numpy()


# ---------------------------------------------------------------- 1: sizes and channel counts ----------------------

@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("Cc", [1, 2, 3, 4])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193])
def test_sizes_around_wave_workgroup_and_tile(dev, n, Cc, masked):
    """one wave, one workgroup, one sort tile, and one to either side of each; mt_stats_kernel<1..4>"""
    pred, gt, std, mask = _pixels(n, Cc, seed=1000 * Cc + n, masked=masked)
    clip, min_sigma = _params(Cc)
    row = _run_twice(dev, pred, gt, std, mask, clip, min_sigma, _flags_no_ssim())
    ref, ex = R.restate_row(pred, gt, std, mask, clip=clip, min_sigma=min_sigma)
    _check_row(row, ref, ex, f"n {n} C {Cc}{' masked' if masked else ''}")


# ---------------------------------------------------------------- 2: more than 1024 sort tiles ---------------------

N_1024_TILES = 1024 * TILE                                                   # lane 1023 of the row scan's first chunk is live
N_1026_TILES = 1024 * TILE + TILE + 1                                        # a second chunk: two entries + the carry


@functools.lru_cache(maxsize=None)
def _big():
    pred, gt, std, _ = _pixels(N_1026_TILES, 1, seed=77)
    return pred, gt, std


@pytest.mark.parametrize("n,last_two_tiles_only", [(N_1024_TILES, False), (N_1026_TILES, False), (N_1026_TILES, True)])
def test_row_scan_carries_across_1024_tile_chunks(dev, n, last_two_tiles_only):
    """ms_rowscan_kernel scans a digit's per-tile counts 1024 at a time and carries the running total in LDS; an image has
    to exceed 4 194 304 pixels to need the carry.  With the mask, every valid key sits in tiles 1024 and 1025: all of
    the second chunk's counts, none of the first's but the padding digit."""
    from uncertainty_nerf_gs_amd import lib as L
    pred, gt, std = (x[:n] for x in _big())
    mask = None
    if last_two_tiles_only:
        mask = torch.zeros(n, dtype=torch.bool)
        mask[1024 * TILE:] = True
    flags = L.METRICS_AUSE | L.METRICS_AUCE | L.METRICS_NLL
    row = _run(dev, pred, gt, std, mask, float("inf"), 0.1, flags).cpu().numpy()
    ref, ex = R.restate_row(pred, gt, std, mask, min_sigma=0.1)
    _check_row(row, ref, ex, f"n {n} = {(n + TILE - 1) // TILE} tiles{' valid in the last two only' if last_two_tiles_only else ''}")


# ---------------------------------------------------------------- 3: valid pixels only at the end ------------------

@pytest.mark.parametrize("byte", [1, 2, 255])
@pytest.mark.parametrize("which", ["last pixel", "last five", "all but tile 0"])
def test_valid_pixels_only_at_the_end(dev, which, byte):
    """n = 3 tiles + 5: the last tile holds five live lanes of one wave, the tiles in front hold padding keys only (or, in
    the third variant, tile 0 does); any non-zero mask byte means "valid" """
    n = 3 * TILE + 5
    pred, gt, std, _ = _pixels(n, 3, seed=31)
    std[n - 5:] = torch.tensor([0.05, 0.0, 0.11, 0.05, 0.2])
    mask = torch.zeros(n, dtype=torch.uint8)
    mask[{"last pixel": n - 1, "last five": n - 5, "all but tile 0": TILE}[which]:] = byte
    row = _run_twice(dev, pred, gt, std, mask, 1.0, 3e-2, _flags_no_ssim())
    ref, ex = R.restate_row(pred, gt, std, mask, clip=1.0, min_sigma=3e-2)
    assert ex["n"] == {"last pixel": 1, "last five": 5, "all but tile 0": 2 * TILE + 5}[which]
    _check_row(row, ref, ex, f"{which}, mask byte {byte}")


# ---------------------------------------------------------------- 4: nothing valid ---------------------------------

@pytest.mark.parametrize("n", [5, TILE + 1])
def test_nothing_valid(dev, n):
    from uncertainty_nerf_gs_amd import metrics as M
    pred, gt, std, _ = _pixels(n, 3, seed=41)
    mask = torch.zeros(n, dtype=torch.bool)
    row = _run_twice(dev, pred, gt, std, mask, 1.0, 3e-2, _flags_no_ssim())
    inf = float("inf")
    assert row[0] == 0 and row[1] == 0 and tuple(row[8:12]) == (inf, -inf, inf, -inf), row[:12]
    assert np.all(np.delete(row, [8, 9, 10, 11]) == 0)
    ref, ex = R.restate_row(pred, gt, std, mask, clip=1.0, min_sigma=3e-2)
    _check_row(row, ref, ex, f"nothing valid of {n}")
    with pytest.raises(ValueError, match="no valid pixel"):
        M.finish_metrics(row, 3, "rgb", _flags_no_ssim())


# ---------------------------------------------------------------- 5: the caller's tables ---------------------------

@pytest.mark.parametrize("which", ["128 entries", "one entry"])
def test_caller_tables(dev, which):
    """n = 4097 masked: unsorted thresholds with duplicates, 0 and inf find their way back through `perm`; ratios 0, 1 and
    outside [0, 1] run into mt_keep's clamps"""
    ratios, z = R.edge_tables() if which == "128 entries" else (np.array([0.5]), np.array([1.0]))
    pred, gt, std, mask = _pixels(TILE + 1, 3, seed=51, masked=True)
    row = _run_twice(dev, pred, gt, std, mask, 1.0, 3e-2, _flags_no_ssim(), ratios=ratios, z=z)
    ref, ex = R.restate_row(pred, gt, std, mask, clip=1.0, min_sigma=3e-2, ratios=ratios, z=z)
    _check_row(row, ref, ex, f"tables of {which}", n_z=len(z), n_r=len(ratios))


def test_a_cut_on_the_last_segsum_blocks_end(dev):
    """n = 1024 x 256 unmasked: 1024 segsum blocks of 256, n_valid their exact end; ratio 0 (and every ratio below 0) cuts
    there, where no block owns the cut and mt_finish_kernel takes the prefix alone"""
    ratios, z = R.edge_tables()
    n = 1024 * 256
    pred, gt, std, _ = _pixels(n, 1, seed=52)
    row = _run_twice(dev, pred, gt, std, None, float("inf"), 0.1, _flags_no_ssim(), ratios=ratios, z=z)
    ref, ex = R.restate_row(pred, gt, std, None, min_sigma=0.1, ratios=ratios, z=z)
    _check_row(row, ref, ex, "n 262144, cut on the last block's end", n_z=128, n_r=128)
    from uncertainty_nerf_gs_amd import lib as L
    fam = row[L.METRICS_AUSE_OFF:].reshape(4, 128)
    assert _rel(fam[0, 1], row[2]) <= 1e-9 and _rel(fam[2, 1], row[2]) <= 1e-9       # keep everything: the plain sums
    assert _rel(fam[1, 4], row[3]) <= 1e-9 and _rel(fam[3, 4], row[3]) <= 1e-9


# ---------------------------------------------------------------- 6: non-finite inputs -----------------------------

def test_non_finite_inputs_are_counted_once_per_pixel(dev):
    from uncertainty_nerf_gs_amd import metrics as M
    n = 5000
    nan, inf = float("nan"), float("inf")
    pred, gt, std, mask = _pixels(n, 3, seed=61, masked=True, keep=0.8)
    valid = [int(i) for i in torch.nonzero(mask).view(-1)]
    masked_out = [int(i) for i in torch.nonzero(~mask).view(-1)]
    v, m = iter(valid[10::37]), iter(masked_out[3::11])
    pred[next(v), 0] = nan
    pred[next(v), 2] = -inf
    i = next(v); pred[i, 1] = inf                                             # above clip_max = 1.0: clipped to 1, still counts
    gt[next(v), 1] = nan
    gt[next(v), 0] = inf
    gt[next(v), 2] = -inf
    std[next(v)] = nan
    std[next(v)] = inf
    std[next(v)] = -inf
    i = next(v); pred[i, 0] = nan; pred[i, 2] = inf                           # two bad channels: one pixel
    i = next(v); pred[i, 1] = nan; gt[i, 1] = nan; std[i] = nan               # bad everywhere: one pixel
    pred[valid[-1], 2] = nan                                                  # the last valid pixel
    for bad in (nan, inf, -inf):                                              # left out by the mask: not counted
        pred[next(m), 0] = bad
        gt[next(m), 2] = bad
        std[next(m)] = bad
    finite = torch.isfinite(pred).all(-1) & torch.isfinite(gt).all(-1) & torch.isfinite(std)
    n_valid, n_bad = int(mask.sum()), int((mask & ~finite).sum())
    assert n_bad == 12 and int((~mask & ~finite).sum()) == 9
    row = _run_twice_nan(dev, pred, gt, std, mask)
    print(f"[non-finite] n_valid {row[0]:.0f} (host {n_valid}), non-finite count {row[1]:.0f} (host {n_bad})")
    assert row[0] == n_valid and row[1] == n_bad
    with pytest.raises(ValueError, match=f"^{n_bad} of {n_valid} pixels have a non-finite"):
        M.finish_metrics(row, 3, "rgb", _flags_no_ssim())


def _run_twice_nan(dev, pred, gt, std, mask):
    """two calls; the counts must repeat (the sums hold NaN, which torch.equal would call different)"""
    a = _run(dev, pred, gt, std, mask, 1.0, 3e-2, _flags_no_ssim()).cpu().numpy()
    b = _run(dev, pred, gt, std, mask, 1.0, 3e-2, _flags_no_ssim()).cpu().numpy()
    assert a[0] == b[0] and a[1] == b[1]
    return a


# ---------------------------------------------------------------- 7: flag subsets ----------------------------------

def test_flag_subsets_fill_their_slots_and_no_others(dev):
    """one 64 x 80 x 3 image, METRICS_ALL once, then each flag alone and none: what a call asks for is bit-equal to the
    ALL call's, [0..6] and [8..11] always are, everything else is exactly 0"""
    from uncertainty_nerf_gs_amd import lib as L
    H, W = 64, 80
    pred, gt, std, _ = _pixels(H * W, 3, seed=71)
    args = [x.to(dev) for x in (pred.view(H, W, 3), gt.view(H, W, 3), std.view(H, W))]

    def call(flags):
        from uncertainty_nerf_gs_amd import ops
        return ops.image_metrics(*args, image_hw=(H, W), clip_max=1.0, nll_min_sigma=3e-2, flags=flags).cpu().numpy()

    full = call(L.METRICS_ALL)
    ref, ex = R.restate_row(pred, gt, std, clip=1.0, min_sigma=3e-2)
    _check_row(full, ref, ex, "flag subsets, the ALL call", ssim=True)
    assert full[13] == (H - 10) * (W - 10) * 3 and full[7] != 0 and full[12] != 0
    slots = {L.METRICS_AUSE: np.arange(L.METRICS_AUSE_OFF, L.METRICS_ROW), L.METRICS_AUCE: np.arange(L.METRICS_AUCE_OFF, L.METRICS_AUSE_OFF),
             L.METRICS_NLL: np.array([7]), L.METRICS_SSIM: np.array([12, 13])}
    always = np.array([0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11])
    assert L.METRICS_ALL == sum(slots)
    for flags in (L.METRICS_AUSE, L.METRICS_AUCE, L.METRICS_NLL, L.METRICS_SSIM, 0):
        row = call(flags)
        asked = np.concatenate([always] + [s for f, s in slots.items() if flags & f])
        rest = np.setdiff1d(np.arange(L.METRICS_ROW), asked)
        differ = asked[row[asked].view(np.uint64) != full[asked].view(np.uint64)]
        print(f"[flag subsets] flags {flags}: {asked.size} slots asked for, {differ.size} differ from the ALL call; "
              f"{int(np.count_nonzero(row[rest]))} of the other {rest.size} are not 0")
        assert differ.size == 0, (flags, differ, row[differ], full[differ])
        assert not np.any(row[rest]), (flags, rest[row[rest] != 0])


# ---------------------------------------------------------------- 8: dirty and reused scratch ----------------------

@pytest.mark.parametrize("fill", ["0xFF bytes", "NaN"])
def test_dirty_and_reused_scratch(dev, fill):
    """one arena, filled before every call, across images of 70 000, 300 and 70 000 pixels: each row is bit-equal to a call
    on freshly allocated scratch (the result depends on nothing the workspace held)"""
    from uncertainty_nerf_gs_amd import lib as L, ops
    ws = ops.Workspace()
    cases = {n: _pixels(n, 3, seed=81 + n, masked=True, keep=0.9) for n in (70000, 300)}
    fresh = {n: _run(dev, *c, 1.0, 3e-2, _flags_no_ssim()) for n, c in cases.items()}
    for n, c in cases.items():
        ref, ex = R.restate_row(*c, clip=1.0, min_sigma=3e-2)
        _check_row(fresh[n].cpu().numpy(), ref, ex, f"n {n}, fresh scratch")
    for n in (70000, 300, 70000):
        words = (L.load().unerf_image_metrics_workspace_bytes(n) + 7) // 8
        buf = ws.get("image_metrics", (words,), dev, torch.float64)
        if fill == "NaN":
            buf.fill_(float("nan"))
        else:
            buf.view(torch.uint8).fill_(255)
        row = _run(dev, *cases[n], 1.0, 3e-2, _flags_no_ssim(), workspace=ws)
        same = torch.equal(row.view(torch.int64), fresh[n].view(torch.int64))
        print(f"[scratch filled with {fill}] n {n}: row bit-equal to the fresh-scratch row: {same}")
        assert same, (fill, n, torch.nonzero(row.view(torch.int64) != fresh[n].view(torch.int64)).view(-1)[:16])
    assert ws.nbytes() >= L.load().unerf_image_metrics_workspace_bytes(70000)


# ---------------------------------------------------------------- 9: key range -------------------------------------

def _wide(g, n):
    """residuals 10^U(-18, 18) with random sign against a zero target (so they are exact), sigma 10^U(-18, 18): the top
    radix digit of the sq keys takes 114 of its 256 values, of the var keys 121"""
    mag = 10.0 ** (36.0 * torch.rand(n, 3, generator=g, dtype=torch.float64) - 18.0)
    sign = torch.where(torch.rand(n, 3, generator=g) < 0.5, -1.0, 1.0)
    pred = (mag * sign).float()
    std = (10.0 ** (36.0 * torch.rand(n, generator=g, dtype=torch.float64) - 18.0)).float()
    return pred, torch.zeros(n, 3), std


def _tiny(g, n):
    """target 0, predictions 10^U(-23, -19): sq = d d is a float32 denormal for 99 % of the pixels and exactly 0 for a few;
    sigma in the same range makes var alike.  A kernel that flushes denormals sums zeros at the small cuts"""
    pred = (10.0 ** (4.0 * torch.rand(n, 3, generator=g, dtype=torch.float64) - 23.0)).float()
    std = (10.0 ** (4.0 * torch.rand(n, generator=g, dtype=torch.float64) - 23.0)).float()
    return pred, torch.zeros(n, 3), std


def _mostly_exact(g, n):
    """90 % of the pixels with pred == target bit for bit, sigma == 0 on half of those: the zero-key tie run of a perfect
    region, about 4500 equal sq / ab keys and 2250 equal var keys, ordered by pixel index alone"""
    pred, gt, std, _ = _pixels(n, 3, seed=int(torch.randint(1 << 30, (1,), generator=g)))
    exact = torch.rand(n, generator=g) < 0.9
    pred[exact] = gt[exact]
    std[exact & (torch.rand(n, generator=g) < 0.5)] = 0.0
    return pred, gt, std


@pytest.mark.parametrize("kind", ["wide", "tiny", "mostly exact"])
def test_key_range(dev, kind):
    n = 5000
    g = torch.Generator().manual_seed(91)
    pred, gt, std = {"wide": _wide, "tiny": _tiny, "mostly exact": _mostly_exact}[kind](g, n)
    clip = 1.0 if kind == "mostly exact" else float("inf")
    d = torch.clamp(pred, max=clip) - gt
    sq = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    var = std * std
    assert bool(torch.isfinite(sq).all()) and bool(torch.isfinite(var).all())
    tiny32 = float(torch.finfo(torch.float32).tiny)
    denormal, zero = int(((sq > 0) & (sq < tiny32)).sum()), int((sq == 0).sum())
    tops = [int(torch.unique(x.view(torch.int32) >> 24).numel()) for x in (sq, var)]
    print(f"[key range, {kind}] sq: {denormal} denormal, {zero} exactly 0 of {n}; top key byte takes {tops[0]} values (sq), {tops[1]} (var)")
    if kind == "wide":
        assert tops[0] >= 80 and tops[1] >= 110
    elif kind == "tiny":
        assert denormal >= 0.98 * n and zero >= 1 and int((var < tiny32).sum()) == n      # var: denormal, a tenth exactly 0
    else:
        assert zero >= 0.88 * n and int((var == 0).sum()) >= 0.4 * n
    row = _run_twice(dev, pred, gt, std, None, clip, 3e-2, _flags_no_ssim())
    ref, ex = R.restate_row(pred, gt, std, clip=clip, min_sigma=3e-2)
    _check_row(row, ref, ex, f"key range, {kind}")


# ---------------------------------------------------------------- 10: SSIM edges -----------------------------------

@pytest.mark.parametrize("H,W,Cc", [(11, 11, 3), (11, 75, 1), (43, 11, 2), (26, 42, 4), (27, 43, 3)])
def test_ssim_interior_edges(dev, H, W, Cc):
    """a single window; one interior row whose last tile is one column wide; one interior column; exactly one 32 x 16 tile;
    one past the tile in both directions.  METRICS_ALL: the data range comes from the same call's min / max, predictions
    above clip_max = 1.0 are clipped on the way into the windows"""
    from uncertainty_nerf_gs_amd import lib as L, ops
    pred, gt, std, _ = _pixels(H * W, Cc, seed=100 * H + W)
    assert float(pred.max()) > 1.0
    pred, gt, std = pred.view(H, W, Cc), gt.view(H, W, Cc), std.view(H, W)
    rows = [ops.image_metrics(pred.to(dev), gt.to(dev), std.to(dev), image_hw=(H, W), clip_max=1.0, nll_min_sigma=3e-2,
                              flags=L.METRICS_ALL) for _ in range(2)]
    assert torch.equal(rows[0], rows[1])
    row = rows[0].cpu().numpy()
    s, cnt = R.ssim_sum_f64(torch.clamp(pred, max=1.0), gt)
    assert row[13] == cnt == (H - 10) * (W - 10) * Cc
    diff = abs(row[12] / row[13] - s / cnt)
    _note("ssim", diff)
    print(f"[ssim {H}x{W}x{Cc}] {int(cnt)} windows: fused sum {row[12]:.17g} restated {s:.17g}, |diff| of the mean index {diff:.2e}")
    assert diff <= 1e-9
    ref, ex = R.restate_row(pred, gt, std, clip=1.0, min_sigma=3e-2)
    _check_row(row, ref, ex, f"ssim {H}x{W}x{Cc}", ssim=True)


# ---------------------------------------------------------------- 11: a side stream --------------------------------

def test_a_side_stream(dev):
    """inputs produced on a side stream and the call made under it, with nothing waiting on the default stream: the kernels
    have to run on the stream they are given to see their inputs.  Bit-equal to the default-stream row"""
    pred, gt, std, mask = _pixels(2 * TILE + 77, 3, seed=111, masked=True)
    host = (pred, gt, std, mask.view(torch.uint8))
    on_default = _run(dev, *host, 1.0, 3e-2, _flags_no_ssim())
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(device=dev)
    staged = [x.to(dev) for x in host]
    torch.cuda.synchronize(dev)
    from uncertainty_nerf_gs_amd import ops
    with torch.cuda.stream(side):
        p, t, s, m = (x + 0 for x in staged)
        row = ops.image_metrics(p, t, s, m, clip_max=1.0, nll_min_sigma=3e-2, flags=_flags_no_ssim())
    side.synchronize()
    same = torch.equal(row.view(torch.int64), on_default.view(torch.int64))
    print(f"[side stream] row bit-equal to the default-stream row: {same}")
    assert same
    ref, ex = R.restate_row(pred, gt, std, mask, clip=1.0, min_sigma=3e-2)
    _check_row(row.cpu().numpy(), ref, ex, "side stream")
