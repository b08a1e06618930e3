"""The batched splat count and sort (unerf_splat_count_intersects_batch, unerf_splat_bin_sort_batch) called DIRECTLY, with
inputs constructed so that every view has a chosen number of (tile, splat) pairs -- the segment edges of the staged passes:
views of 0 pairs in every position, views of exactly 2048 k and 16 x 2048 k pairs and one pair more (no ragged chunk / a whole
group of 16 empty padding chunks), views that start off a 16-byte key boundary, depth segments with a ragged last chunk, the
digit plans on either side of 128 and 256 tiles, the largest tile count the batch serves (11,999), the second trip of the
radii search, and B = 16 (the size of the by-value segment / camera argument structs).

Every comparison is on integers and exact.  The sorted ids and the tile ranges are held to (a) oracle.splat_oracle.bin_and_sort
run on every view alone (ids shifted by v N, the non-empty tile ranges by the pairs of the views before it) and (b) the
single-view ops.splat_bin_sort on the view's slice, shifted the same way.  tests/test_staged_sort_cpu.py pins the algorithm
of the segmented passes in numpy at the same pair counts; tests/test_gpu_splat_batch.py compares whole frames."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import splat_oracle as SO

pytestmark = pytest.mark.gpu

# tiles -> (H, W): 63 = 7 x 9 with partial edge tiles; 127 the last one-pass size, 128 the first two-pass size (4 + 4 bits);
# 255 / 256: the digit split changes again behind 256 keys (tiles + the sentinel: 4 + 4 -> 4 + 5 bits); 11,999 = 71 x 169:
# UNERF_SPLAT_BATCH_MAX_TILES, the whole-key histogram's 64,384 bytes of LDS
SIZES = {63: (100, 130), 127: (16, 2032), 128: (128, 256), 255: (233, 265), 256: (256, 256), 11999: (1136, 2704)}
DEPTHS = (0.5 + 0.25 * np.arange(40)).astype(np.float32)      # the same ~40 depths in every view: ties everywhere
CYCLE16 = (0, 1, 2047, 2048, 2049, 4096, 7, 0) * 2
PAIRS = [(1,), (2048,), (2049,), (0,), (2048, 0, 2049), (0, 0, 5), (5, 0, 0), (3, 2047, 1), (32768, 32769, 1, 2047), CYCLE16,
         (0,) * 16]
EDGE_PAIRS = [(2048, 0, 2049), CYCLE16]


def _tiles_of(H, W):
    return (W + 15) // 16, (H + 15) // 16


def _view(rng, N, P, H, W, corner, multis=True):
    """one view of N splats with exactly P pairs: single-tile splats (radius 1 at a tile's centre) and, for about half of the
    pairs, 3 x 3-tile splats (radius 16; fewer tiles at the image's edges: the count is the oracle's tile_bbox), at random
    positions among culled splats (radius 0, count 0, a position inside the image).  Tile 0 and the last tile are hit
    (with P = 1: the one `corner` says)."""
    tbx, tby = _tiles_of(H, W)
    tiles = tbx * tby
    centre = lambda t: np.stack([16.0 * (t % tbx) + 8.0, 16.0 * (t // tbx) + 8.0], 1).astype(np.float32)

    def count(xy, r):
        x0, y0, x1, y1 = SO.tile_bbox(xy[:, 0], xy[:, 1], r.astype(np.float32), 16, H, W)
        return ((x1 - x0) * (y1 - y0)).astype(np.int32)

    xys = (rng.random((N, 2)) * [W, H]).astype(np.float32)
    radii, nth = np.zeros(N, np.int32), np.zeros(N, np.int32)
    depths = DEPTHS[rng.integers(0, len(DEPTHS), N)]
    slots = rng.permutation(N)
    nm = 0
    if multis and P >= 20:
        cand = centre(rng.integers(0, tiles, P // 18))
        c = count(cand, np.full(len(cand), 16))
        nm = int(np.searchsorted(np.cumsum(c), P - 2, side="right"))      # two pairs stay for the corner tiles
        xys[slots[:nm]], radii[slots[:nm]], nth[slots[:nm]] = cand[:nm], 16, c[:nm]
    ns = P - int(nth.sum())
    assert nm + ns <= N
    t = rng.integers(0, tiles, ns)
    t[:2] = ([0, tiles - 1] if corner else [tiles - 1, 0])[:ns]
    s = slots[nm:nm + ns]
    xys[s], radii[s] = centre(t), 1
    nth[s] = count(xys[s], radii[s])
    assert np.all(nth[s] == 1) and int(nth.sum()) == P
    return xys, depths, radii, nth


@functools.lru_cache(maxsize=None)
def _case(pairs, tiles, N=None, multis=True):
    """-> the host arrays of a batch with the given per-view pair counts, and reference (a): the numpy oracle on every view alone"""
    H, W = SIZES[tiles]
    N = max(max(pairs), 1) + 37 if N is None else N        # (not a multiple of 4: every later view's depth keys start unaligned)
    rng = np.random.default_rng([len(pairs), sum(pairs), tiles, N])
    views = [_view(rng, N, P, H, W, v % 2 == 0, multis) for v, P in enumerate(pairs)]
    c = dict(pairs=pairs, H=H, W=W, N=N, B=len(pairs), tiles=tiles)
    for i, k in enumerate(("xys", "depths", "radii", "nth")):
        c[k] = np.stack([v[i] for v in views])
    ids, bins, off = [], [], 0
    for v in range(len(pairs)):
        I, _, _, g, b = SO.bin_and_sort(c["xys"][v], c["depths"][v], c["radii"][v], c["nth"][v], H, W)
        assert I == pairs[v]
        ids.append(g.astype(np.int64) + v * N)
        bins.append(_shift(b, off))
        off += I
    c["ref_ids"] = np.concatenate(ids).astype(np.int32)
    c["ref_bins"] = np.stack(bins)
    return c


def _shift(bins, off):
    b = np.array(bins, dtype=np.int32)
    b[b[:, 1] > b[:, 0]] += off          # empty tiles stay (0, 0)
    return b


def _run(dev, c, tight=None, t=None):
    """SplatCountBatch + splat_bin_sort_batch on the case -> (totals, visible, ids, bins, cum) as host values"""
    from uncertainty_nerf_gs_amd import ops
    t = t or {k: torch.from_numpy(c[k]).to(dev) for k in ("xys", "depths", "radii", "nth")}
    count = ops.SplatCountBatch(t["nth"], t["radii"] if tight else None)
    totals, visible, gids, bins = ops.splat_bin_sort_batch(t["xys"], t["depths"], t["radii"], count, c["H"], c["W"], tight=tight)
    I = sum(totals)
    return list(totals), list(visible), gids[:I].cpu().numpy(), bins.cpu().numpy(), count.cum.cpu().numpy()


def _singles(dev, c, tight=None, t=None):
    """reference (b): the single-view sort on every view's slice, shifted into the batch's id and slot ranges"""
    from uncertainty_nerf_gs_amd import ops
    t = t or {k: torch.from_numpy(c[k]).to(dev) for k in ("xys", "depths", "radii", "nth")}
    ids, bins, totals, off = [], [], [], 0
    for v in range(c["B"]):
        tv = (tight[0][v], tight[1][v]) if tight else None
        I, _, _, g, b = ops.splat_bin_sort(t["xys"][v], t["depths"][v], t["radii"][v], t["nth"][v], c["H"], c["W"],
                                           want_isect_ids=False, tight=tv)
        ids.append(g.cpu().numpy().astype(np.int64) + v * c["N"])
        bins.append(_shift(b.cpu().numpy(), off))
        totals.append(I)
        off += I
    return totals, np.concatenate(ids).astype(np.int32), np.stack(bins)


def _check_properties(pairs, N, ids, bins):
    pb = np.concatenate([[0], np.cumsum(pairs)])
    for v, P in enumerate(pairs):
        seg = ids[pb[v]:pb[v + 1]]
        assert np.all((seg >= v * N) & (seg < (v + 1) * N)), f"view {v}: an id of another view"
        b = bins[v][bins[v][:, 1] > bins[v][:, 0]]
        assert np.all(bins[v][bins[v][:, 1] <= bins[v][:, 0]] == 0)
        b = b[np.argsort(b[:, 0])]
        edges = np.concatenate([b[:, 0], b[-1:, 1]]) if len(b) else np.array([pb[v]])
        assert edges[0] == pb[v] and (len(b) == 0) == (P == 0), f"view {v}: first range"
        assert np.array_equal(b[:-1, 1], b[1:, 0]) and (len(b) == 0 or b[-1, 1] == pb[v + 1]), f"view {v}: ranges do not tile its pairs"


def _check(dev, c):
    totals, visible, ids, bins, cum = _run(dev, c)
    pairs = c["pairs"]
    assert totals == list(pairs) and visible == [p > 0 for p in pairs]
    assert np.array_equal(cum.reshape(-1), np.cumsum(c["nth"].reshape(-1).astype(np.int64)).astype(np.int32))
    assert ids.shape == c["ref_ids"].shape and bins.shape == (c["B"], c["tiles"], 2)
    _check_properties(pairs, c["N"], ids, bins)
    assert np.array_equal(ids, c["ref_ids"]), "ids: the numpy oracle on every view alone"
    assert np.array_equal(bins, c["ref_bins"]), "tile ranges: the numpy oracle on every view alone"
    tot1, ids1, bins1 = _singles(dev, c)
    assert tot1 == list(pairs)
    assert np.array_equal(ids, ids1), "ids: the single-view sort of every view"
    assert np.array_equal(bins, bins1), "tile ranges: the single-view sort of every view"
    if max(pairs) >= 2:
        hit = np.nonzero((bins[:, :, 1] > bins[:, :, 0]).any(0))[0]
        assert hit[0] == 0 and hit[-1] == c["tiles"] - 1      # the first and the last tile take part
    if not sum(pairs):
        assert not bins.any()
    return totals, visible, ids, bins


_name = lambda p: "b%d_%s" % (len(p), "cycle" if p == CYCLE16 else "zeros" if len(p) == 16 else "_".join(map(str, p)))


@pytest.mark.parametrize("pairs", PAIRS, ids=_name)
def test_box_lists_at_chunk_and_segment_edges(dev, pairs):
    """63 tiles (one pass over the whole key), every pair-count vector"""
    _check(dev, _case(pairs, 63))


@pytest.mark.parametrize("tiles", [127, 128, 255, 256, 11999])
@pytest.mark.parametrize("pairs", EDGE_PAIRS, ids=_name)
def test_box_lists_at_the_digit_plans_and_the_largest_tile_count(dev, pairs, tiles):
    """one pass at 127 tiles, two from 128; another digit split behind 256 keys; 11,999 tiles fill the histogram's LDS"""
    _check(dev, _case(pairs, tiles))


DEPTH_CASES = [(3, N) for N in (1, 3, 1023, 1024, 1025)] + [(16, 1025)]


@pytest.mark.parametrize("B,N", DEPTH_CASES)
def test_depth_sort_segment_edges(dev, B, N):
    """depth segments of ceil(N / 1024) unpadded chunks, the last one ragged unless N = 1024; a view with every splat culled
    (all keys 0xFFFFFFFF) between live ones, views with every splat live, N not a multiple of 4 (unaligned key starts)"""
    cyc = (min(N, 300), 0, N, min(N, 257), 1, 0, min(N, 1024), min(N, 300))
    pairs = (min(N, 300), 0, N) if B == 3 else cyc * 2
    _check(dev, _case(pairs, 63, N=N, multis=False))


def test_twelve_thousand_tiles_are_refused_before_anything_is_launched(dev, lib):
    """one tile beyond UNERF_SPLAT_BATCH_MAX_TILES: UNERF_ERR_ARG naming the limit, the outputs untouched"""
    from uncertainty_nerf_gs_amd import ops
    h = lib.load()
    H, W, N = 16, 16 * 12000, 4
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=dev, dtype=dt)
    xys, depths, radii, cum = z(1, N, 2), z(1, N), z(1, N, dt=torch.int32), z(1, N, dt=torch.int32)
    bins = torch.full((12000, 2), -7, device=dev, dtype=torch.int32)
    gids = torch.full((16,), -7, device=dev, dtype=torch.int32)
    ws = torch.zeros(int(h.unerf_splat_sort_workspace_bytes_batch(1, N, 1)), device=dev, dtype=torch.uint8)
    rc = h.unerf_splat_bin_sort_batch(xys.data_ptr(), depths.data_ptr(), radii.data_ptr(), cum.data_ptr(), 1, N, (C.c_int64 * 1)(1), H, W,
                                      16, None, None, gids.data_ptr(), bins.data_ptr(), ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream().cuda_stream)
    msg = h.unerf_last_error()
    torch.cuda.synchronize()
    assert rc == -1 and b"12000 tiles" in msg and b"up to 11999" in msg, msg
    assert bool((bins == -7).all()) and bool((gids == -7).all()) and not bool(ws.any())
    count = ops.SplatCountBatch(z(1, N, dt=torch.int32))
    with pytest.raises(lib.UnerfError, match="12000 tiles"):
        ops.splat_bin_sort_batch(xys, depths, radii, count, H, W)
    # 11,999 tiles get past the same check (no pairs here: the bins are cleared and nothing sorts; the parametrised
    # 11999-tile cases above run the sort itself at that size)
    totals, visible, g, b = ops.splat_bin_sort_batch(xys, depths, radii, count, 16, 16 * 11999)
    assert totals == [0] and visible == [False] and b.shape == (1, 11999, 2) and not bool(b.any())


def _pick(counts, P, rng):
    """a subset of the splats whose counts sum to exactly P: greedy over a random order while more than the largest count is
    missing, then topped up with the splat of exactly the remaining count (or, where there is none, the largest one below it)"""
    keep, left, top = np.zeros(len(counts), bool), P, int(counts.max())
    for i in rng.permutation(len(counts)):
        if left <= top:
            break
        if counts[i] > 0:
            keep[i] = True
            left -= int(counts[i])
    while left > 0:
        fits = np.nonzero(~keep & (counts > 0) & (counts <= left))[0]
        assert len(fits), f"the scene has no subset of {P} tight pairs"
        i = fits[np.argmax(counts[fits])]          # (the first of the largest that fit: == left where one exists)
        keep[i] = True
        left -= int(counts[i])
    return keep


def _tight_case(dev, pairs):
    """Tight lists (map_intersects_kernel<uint16_t, 8>: the rows project_kernel counted) of a projected scene, cut down per view
    to splats whose tight counts sum to the wanted pairs -> (case, device tensors, (conics, opacities), kept splats)"""
    import test_gpu_splat_batch as TB
    from uncertainty_nerf_gs_amd import ops, splat
    B, H, W, N = len(pairs), 256, 256, 20000
    gp = {k: v.to(dev) for k, v in TB._scene(N).items()}
    c2ws = [TB._pose(0.4 + 0.9 * v) for v in range(B)]
    views = ops.splat_view_records([splat.viewmat_from_c2w(c) for c in c2ws], [218.0] * B, [218.0] * B, [W / 2] * B, [H / 2] * B,
                                   [c[:3, 3] for c in c2ws])
    xys, depths, radii, conics, comp, nth, opac = ops.splat_project_batch(
        gp["means"].contiguous(), gp["scales"].contiguous(), gp["quats"].contiguous(), views, B, H, W,
        opacity_logits=gp["opacities"].reshape(-1).contiguous())
    rng = np.random.default_rng(sum(pairs))
    keep = torch.from_numpy(np.stack([_pick(nth[v].cpu().numpy(), P, rng) for v, P in enumerate(pairs)])).to(dev)
    radii, nth = torch.where(keep, radii, 0).contiguous(), torch.where(keep, nth, 0).contiguous()
    c = dict(pairs=pairs, H=H, W=W, N=N, B=B, tiles=256)
    return c, dict(xys=xys, depths=depths, radii=radii, nth=nth), (conics, opac), keep


@pytest.mark.parametrize("pairs", [(2048, 0, 2049), (32769, 5, 2048)], ids=_name)
def test_tight_lists_at_chunk_and_segment_edges(dev, pairs):
    """The numpy oracle has no tight rows, so reference (b) alone applies: the single-view tight sort of every view's slice."""
    c, t, (conics, opac), keep = _tight_case(dev, pairs)
    B, N = c["B"], c["N"]
    totals, visible, ids, bins, _ = _run(dev, c, tight=(conics, opac), t=t)
    assert totals == list(pairs) and visible == [p > 0 for p in pairs]
    _check_properties(pairs, N, ids, bins)
    tot1, ids1, bins1 = _singles(dev, c, tight=(conics, opac), t=t)
    assert tot1 == list(pairs)
    assert np.array_equal(ids, ids1) and np.array_equal(bins, bins1)
    owner = np.repeat(np.arange(B), pairs)
    assert bool(keep.cpu().numpy()[owner, ids - owner * N].all())          # only kept splats are listed


# (pairs, tiles, N): pair counts below, at and above one 2,048-pair chunk of the tile passes and above one 16-chunk histogram
# workgroup, at the last two one-pass tile counts and the first two-pass one; one splat, a full and a ragged second 1,024-splat
# chunk of the depth passes (every splat live); no pairs at all
ONE_VIEW = ([(I, tiles, None) for tiles in (63, 127, 128) for I in (1, 2047, 2048, 2049, 32769)] +
            [(N, 63, N) for N in (1, 1024, 1025)] + [(0, 63, None)])


def _batch_of_one_vs_single(dev, c, t=None, tight=None):
    """unerf_splat_bin_sort_batch with B = 1 and unerf_splat_bin_sort on the same inputs: one body, the batch's chunks padded
    to whole histogram workgroups and sorted by the segment kernels, the single view's not -- the same ids and tile ranges"""
    from uncertainty_nerf_gs_amd import ops
    assert c["B"] == 1
    t = t or {k: torch.from_numpy(c[k]).to(dev) for k in ("xys", "depths", "radii", "nth")}
    count = ops.SplatCountBatch(t["nth"], t["radii"] if tight else None)
    totals, _, gids, bins = ops.splat_bin_sort_batch(t["xys"], t["depths"], t["radii"], count, c["H"], c["W"], tight=tight)
    I, _, _, gids1, bins1 = ops.splat_bin_sort(t["xys"][0], t["depths"][0], t["radii"][0], t["nth"][0], c["H"], c["W"],
                                               want_isect_ids=False, tight=(tight[0][0], tight[1][0]) if tight else None)
    assert list(totals) == [I] == list(c["pairs"])
    assert gids1.shape == (I,) and bins.shape == (1, c["tiles"], 2)
    assert torch.equal(gids[:I], gids1), "gaussian_ids_sorted"
    assert torch.equal(bins[0], bins1), "tile_bins"
    if I == 0:
        assert not bool(bins.any()) and not bool(bins1.any())
    else:
        assert int(bins1.max()) == I


@pytest.mark.parametrize("pairs,tiles,N", ONE_VIEW, ids=lambda x: str(x))
def test_a_batch_of_one_view_equals_the_single_view_sort(dev, pairs, tiles, N):
    """box lists"""
    _batch_of_one_vs_single(dev, _case((pairs,), tiles, N=N, multis=N is None))


def test_a_batch_of_one_view_equals_the_single_view_sort_on_tight_lists(dev):
    """2,049 tight pairs at 256 tiles: a ragged second chunk, two passes"""
    c, t, tight, _ = _tight_case(dev, (2049,))
    _batch_of_one_vs_single(dev, c, t=t, tight=tight)


@pytest.mark.parametrize("N", [1, 1023, 1024, 1025, 4097])
@pytest.mark.parametrize("B", [1, 2, 16])
def test_count_batch_scan_totals_and_flags(dev, B, N):
    """the scan over the B N counts against torch.cumsum (int64, then cast), the per-view totals against per-view sums, and with
    no radii given visible[v] == (total[v] > 0) -- all-zero views first, in the middle and last"""
    from uncertainty_nerf_gs_amd import ops
    g = torch.Generator().manual_seed(1000 * B + N)
    for zero in {1: [(), (0,)], 2: [(0,), (1,)], 16: [(0, 7, 15)]}[B]:
        nth = torch.randint(0, 60, (B, N), generator=g, dtype=torch.int32)
        nth[:, 0] = torch.randint(1, 60, (B,), generator=g, dtype=torch.int32)         # (every other view has a pair)
        if zero:
            nth[list(zero)] = 0
        count = ops.SplatCountBatch(nth.to(dev))
        totals, visible = count.wait()
        want = torch.cumsum(nth.reshape(-1).long(), 0).to(torch.int32).reshape(B, N)
        assert torch.equal(count.cum.cpu(), want)
        assert list(totals) == [int(x) for x in nth.long().sum(1)]
        assert list(visible) == [v not in zero for v in range(B)]


@pytest.mark.parametrize("N", [1025, 40000])
def test_count_batch_radius_flag_of_views_without_pairs(dev, N):
    """radii given: a view of zero counts is visible exactly when some radius is positive -- the only one at index 0, at N - 1,
    at 16,384 (the first index of the radii search's second grid-stride trip: 64 workgroups x 256) -- and not when none is"""
    from uncertainty_nerf_gs_amd import ops
    where = [0, N - 1, None, "live", None] + ([16384, 16383, N - 1] if N > 16384 else [])
    B = len(where)
    g = torch.Generator().manual_seed(N)
    nth, radii = torch.zeros(B, N, dtype=torch.int32), torch.zeros(B, N, dtype=torch.int32)
    for v, w in enumerate(where):
        if w == "live":
            nth[v] = torch.randint(0, 60, (N,), generator=g, dtype=torch.int32)
            nth[v, N // 2] = 3
            radii[v] = (nth[v] > 0).to(torch.int32) * 5
        elif w is not None:
            radii[v, w] = 2
        else:
            radii[v] = -torch.randint(0, 3, (N,), generator=g, dtype=torch.int32)      # zero and negative radii: culled
    count = ops.SplatCountBatch(nth.to(dev), radii.to(dev))
    totals, visible = count.wait()
    assert list(totals) == [int(x) for x in nth.long().sum(1)]
    assert list(visible) == [w is not None for w in where]
    assert torch.equal(count.cum.cpu(), torch.cumsum(nth.reshape(-1).long(), 0).to(torch.int32).reshape(B, N))


def test_dirty_scratch_and_a_side_stream_repeat_the_bits(dev, lib):
    """two cases again, each right after a case of another shape and after a freed block of at least the workspace's size was
    filled with 0xFF (best effort: the caching allocator usually hands that block back), and one inside a side stream"""
    a, b = _case((32768, 32769, 1, 2047), 63), _case(CYCLE16, 256)
    first = {id(a): _check(dev, a), id(b): _check(dev, b)}
    h = lib.load()

    def same(x, y):
        assert x[0] == y[0] and x[1] == y[1] and np.array_equal(x[2], y[2]) and np.array_equal(x[3], y[3])

    for c, other in ((a, b), (b, a)):
        _run(dev, other)
        nbytes = int(h.unerf_splat_sort_workspace_bytes_batch(c["B"], c["N"], sum(c["pairs"])))
        junk = torch.full((nbytes + (1 << 20),), 0xFF, device=dev, dtype=torch.uint8)
        torch.cuda.synchronize()
        del junk
        same(_run(dev, c)[:4], first[id(c)])
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = _run(dev, a)[:4]
    side.synchronize()
    same(got, first[id(a)])


def _frames(dev, B, N, active, H=100, W=130, **kw):
    import test_gpu_splat_batch as TB
    gp = {k: v.to(dev) for k, v in TB._scene(N).items()}
    if not active:
        gp.pop("log_uncertainties")
    poses = [TB._pose(0.3 + 0.39 * v, radius=2.5 + 0.05 * v, height=0.5 - 0.05 * v) for v in range(B)]
    fx = [110.0] * B
    fx[-1] = 143.0
    return TB._batch_vs_singles(gp, poses, (fx, 112.0, 64.0, 51.0), H, W, torch.tensor([0.1, 0.2, 0.3]), **kw)


@pytest.mark.parametrize("active", [True, False], ids=["active", "plain"])
@pytest.mark.parametrize("tight", [True, False], ids=["tight", "box"])
def test_whole_frames_of_sixteen_views(dev, active, tight):
    """B = UNERF_SPLAT_MAX_VIEWS: every by-value argument struct full; each view equals its single-view render on every key"""
    out = _frames(dev, 16, 3000, active, tight=tight)
    assert sum("depth" in o and float(o["accumulation"].max()) > 0.5 for o in out) >= 8


@pytest.mark.parametrize("N", [1, 255, 256, 257])
@pytest.mark.parametrize("B", [2, 16])
def test_whole_frames_of_few_splats(dev, B, N):
    """partial and single-row blocks of the batched projection and of the staged SH kernel (degree 3): 1 splat, and one below,
    at and above a 256-thread block"""
    _frames(dev, B, N, True)
