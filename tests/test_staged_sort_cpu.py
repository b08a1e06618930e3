"""The staged LSD radix pass of unerf_splat.hip (rs_hist / rs_rowscan / rs_scatter_kernel), emulated lane by lane in numpy.

No GPU: this pins the ALGORITHM the kernels implement -- per-chunk digit histogram, exclusive prefix over chunks per digit,
and a scatter in which one 64-lane wave ranks a chunk vector by vector through per-digit "peer words" (every lane ORs its
lane bit into its digit's 64-bit word, reads it back, the first peer advances the digit's running slot by their number),
stages the pairs in digit order and writes each digit's pairs as one run at delta[digit] + slot -- against numpy's stable
argsort, for the tile sort (two passes: low digit, high digit) and the depth sort (four 8-bit passes).  The GPU tests
(tests/test_gpu_splat.py) compare the kernels themselves with rocprim's sorts.

The second half restates the SEGMENTED pass of the batched sort -- one segment per view, each with its own chunk range, pair
range, prefix rows, digit totals and output base -- and holds it to a stable argsort of every view on its own, at the pair counts
where the segment bookkeeping has its edges; tests/test_gpu_splat_batch_edges.py holds the kernels to the same cases."""
import numpy as np
import pytest


def wave_stage(k, v, d, lstart, B, kmax):
    """one 64-lane wave ranks a chunk vector by vector and stages it in digit order: -> (staged keys, staged vals)"""
    m = len(k)
    cur = lstart.copy()
    pw = np.zeros(B, np.uint64)
    sval, skey = np.empty(m, v.dtype), np.empty(m, k.dtype)
    for v0 in range(0, m, 64):                # a vector of 64 pairs
        lanes = np.arange(min(64, m - v0))
        dv = d[v0 + lanes]
        for l in lanes:                        # ds_or: every lane ORs its bit into its digit's word
            pw[dv[l]] |= np.uint64(1) << np.uint64(l)
        peers = pw[dv].copy()                  # read back
        pw[dv] = 0                             # cleared
        rank = np.array([bin(int(peers[l]) & ((1 << int(l)) - 1)).count("1") for l in lanes])
        base = cur[dv].copy()                  # the digit's running slot, read by all ...
        for l in lanes:                        # ... and advanced by the first of the peers for all of them
            if rank[l] == 0:
                cur[dv[l]] += bin(int(peers[l])).count("1")
        sval[base + rank] = v[v0 + lanes]
        skey[base + rank] = np.minimum(k[v0 + lanes], kmax)
    return skey, sval


def staged_pass(keys, vals, shift, B, M, kmax):
    """one stable pass by digit (min(key, kmax) >> shift) & (B - 1); chunks of M pairs, a wave per chunk"""
    n = len(keys)
    nchunk = max(1, -(-n // M))
    digit = lambda k: (np.minimum(k, kmax) >> shift) & (B - 1)
    # rs_hist_kernel: table[digit][chunk]
    table = np.zeros((B, nchunk), np.int64)
    for c in range(nchunk):
        np.add.at(table[:, c], digit(keys[c * M:(c + 1) * M]), 1)
    # rs_rowscan_kernel: exclusive prefix over the chunks per digit (in place) + the digit totals
    dtotal = table.sum(1)
    prefix = np.cumsum(table, 1) - table
    dbase = np.cumsum(dtotal) - dtotal
    out_k, out_v = np.empty_like(keys), np.empty_like(vals)
    for c in range(nchunk):                       # rs_scatter_kernel, one wave
        k, v = keys[c * M:(c + 1) * M], vals[c * M:(c + 1) * M]
        m = len(k)
        cnt = (prefix[:, c + 1] if c + 1 < nchunk else dtotal) - prefix[:, c]      # neighbours of the prefix row, as the kernel does
        lstart = np.cumsum(cnt) - cnt
        delta = dbase + prefix[:, c] - lstart
        skey, sval = wave_stage(k, v, digit(k), lstart, B, kmax)
        slot = np.arange(m)                        # write-out: consecutive slots of a digit = consecutive addresses
        dst = delta[digit(skey)] + slot
        out_k[dst], out_v[dst] = skey, sval
    return out_k, out_v


@pytest.mark.parametrize("n,tiles", [(1, 50), (63, 50), (5000, 8160), (4097, 121), (10000, 8160)])
def test_two_pass_tile_sort_is_a_stable_sort(n, tiles):
    rng = np.random.default_rng(n)
    T1 = tiles + 1
    keys = rng.integers(0, T1, n).astype(np.int64)
    keys[rng.random(n) < 0.01] = tiles             # sentinel pairs
    vals = rng.integers(0, 1 << 20, n).astype(np.int64)
    bits = max(1, int(np.ceil(np.log2(T1))))
    b0 = 0 if bits <= 7 else bits // 2
    k, v = keys, vals
    if b0:
        k, v = staged_pass(k, v, 0, 1 << b0, 2048, tiles)
    k, v = staged_pass(k, v, b0, 1 << (bits - b0), 2048, tiles)
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(k, keys[order]) and np.array_equal(v, vals[order])


@pytest.mark.parametrize("n", [3, 1025, 7000])
def test_four_pass_depth_sort_is_a_stable_sort(n):
    rng = np.random.default_rng(n)
    depth = rng.uniform(0.1, 30.0, n).astype(np.float32)
    depth[: n // 3] = depth[n // 3: 2 * (n // 3)]    # equal depths: stability decides
    keys = depth.view(np.uint32).astype(np.int64)
    keys[rng.random(n) < 0.1] = 0xFFFFFFFF           # culled splats last
    vals = np.arange(n, dtype=np.int64)
    k, v = keys, vals
    for p in range(4):
        k, v = staged_pass(k, v, 8 * p, 256, 1024, 0xFFFFFFFF)
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(k, keys[order]) and np.array_equal(v, vals[order])


# ---- the segmented pass of the batched sort (unerf_splat_bin_sort_batch): one segment per view ---------------------------------
# Restated here, nothing called from the library: the chunk and pair ranges of the segments (RsSegs), the chunk -> segment search
# and the chunk's clamped pair range (rs_seg_of, rs_chunk_range), the per-segment prefix rows and digit totals
# (rs_rowscan_kernel, grid.y = segments), and what the scatter takes from them: the neighbour of the prefix row up to the segment's
# own last chunk (cend = cb[g + 1]), the segment's first output slot pb[g], and no work for a padding chunk.

def tile_segments(pairs, M=2048, group=16):
    """the tile passes: view v's chunks padded to whole groups of 16 (a whole-key histogram workgroup never straddles two views)"""
    cb, pb = [0], [0]
    for p in pairs:
        c = -(-p // M)
        cb.append(cb[-1] + -(-c // group) * group)
        pb.append(pb[-1] + p)
    return cb, pb


def depth_segments(B, N, M=1024):
    """the depth passes: ceil(N / M) chunks per view, no padding; view v's splats are [v N, (v + 1) N)"""
    cpv = -(-N // M)
    return [v * cpv for v in range(B + 1)], [v * N for v in range(B + 1)]


def seg_of(cb, c):
    g, n = 0, len(cb) - 1
    while g + 1 < n and c >= cb[g + 1]:
        g += 1
    return g


def chunk_range(cb, pb, g, c, M):
    e = pb[g + 1]
    k0 = min(pb[g] + (c - cb[g]) * M, e)
    return k0, min(k0 + M, e)


def staged_pass_segments(keys, vals, shift, B, M, kmax, cb, pb):
    nseg, nchunk = len(cb) - 1, cb[-1]
    digit = lambda k: (np.minimum(k, kmax) >> shift) & (B - 1)
    table = np.zeros((B, max(nchunk, 1)), np.int64)
    for c in range(nchunk):                       # rs_hist_kernel<SEG>: a padding chunk counts nothing
        k0, k1 = chunk_range(cb, pb, seg_of(cb, c), c, M)
        np.add.at(table[:, c], digit(keys[k0:k1]), 1)
    prefix, dtotal = np.zeros_like(table), np.zeros((nseg, B), np.int64)
    for g in range(nseg):                         # rs_rowscan_kernel: segment g scans its own chunks
        rows = table[:, cb[g]:cb[g + 1]]
        prefix[:, cb[g]:cb[g + 1]] = np.cumsum(rows, 1) - rows
        dtotal[g] = rows.sum(1)
    out_k, out_v = np.full_like(keys, -1), np.full_like(vals, -1)
    for c in range(nchunk):                       # rs_scatter_kernel<SEG>
        g = seg_of(cb, c)
        k0, k1 = chunk_range(cb, pb, g, c, M)
        if k1 <= k0:
            continue
        cend = cb[g + 1]
        cnt = (prefix[:, c + 1] if c + 1 < cend else dtotal[g]) - prefix[:, c]
        lstart = np.cumsum(cnt) - cnt
        delta = pb[g] + np.cumsum(dtotal[g]) - dtotal[g] + prefix[:, c] - lstart
        k, v = keys[k0:k1], vals[k0:k1]
        skey, sval = wave_stage(k, v, digit(k), lstart, B, kmax)
        dst = delta[digit(skey)] + np.arange(k1 - k0)
        assert np.all(out_v[dst] == -1), "two pairs sent to one slot"
        out_k[dst], out_v[dst] = skey, sval
    return out_k, out_v


def tile_bins_segments(keys, tiles, cb, pb, M=2048):
    """rs_hist_kernel<FULL> rows (one per 16 chunks), rs_colsum_kernel's 16 partial sums per view over rps rows each, and
    tile_scan_kernel's starts from the view's first slot -> bins [views][tiles][2], empty tiles (0, 0)"""
    T1, nseg = tiles + 1, len(cb) - 1
    full = np.zeros((max(cb[-1] // 16, 1), T1), np.int64)
    for c in range(cb[-1]):
        k0, k1 = chunk_range(cb, pb, seg_of(cb, c), c, M)
        np.add.at(full[c // 16], np.minimum(keys[k0:k1], tiles), 1)
    bins = np.zeros((nseg, tiles, 2), np.int64)
    for g in range(nseg):
        rlo, rows = cb[g] // 16, (cb[g + 1] + 15) // 16
        rps = (rows - rlo + 15) // 16
        part = np.zeros((16, T1), np.int64)
        for s in range(16):
            r0 = rlo + s * rps
            part[s] = full[r0:min(r0 + rps, rows)].sum(0)
        n = part.sum(0)
        start = pb[g] + np.cumsum(n) - n
        hit = n[:tiles] > 0
        bins[g, hit, 0], bins[g, hit, 1] = start[:tiles][hit], (start + n)[:tiles][hit]
    return bins


def tile_plan(tiles):
    bits = max(1, int(np.ceil(np.log2(tiles + 1))))
    b0 = 0 if bits <= 7 else bits // 2
    return b0, 1 << b0, 1 << (bits - b0)


CYCLE16 = [0, 1, 2047, 2048, 2049, 4096, 7, 0] * 2
PAIR_COUNTS = [[1], [2048], [2049], [0], [2048, 0, 2049], [0, 0, 5], [5, 0, 0], [0, 5, 0], [3, 2047, 1],
               [32768, 32769, 1, 2047], CYCLE16, [0] * 16]


def test_segment_ranges_and_their_clamps():
    cb, pb = tile_segments([2049, 0, 5, 32768, 32769, 0])
    assert cb == [0, 16, 16, 32, 48, 80, 80] and pb == [0, 2049, 2049, 2054, 34822, 67591, 67591]
    assert [seg_of(cb, c) for c in (0, 15, 16, 31, 32, 47, 48, 79)] == [0, 0, 2, 2, 3, 3, 4, 4]      # views of zero chunks skipped
    assert chunk_range(cb, pb, 0, 1, 2048) == (2048, 2049)
    assert chunk_range(cb, pb, 0, 2, 2048) == (2049, 2049) and chunk_range(cb, pb, 0, 15, 2048) == (2049, 2049)   # k0 clamped
    assert chunk_range(cb, pb, 3, 47, 2048) == (34822 - 2048, 34822)                       # 16 full chunks: no ragged one
    assert chunk_range(cb, pb, 4, 64, 2048) == (67590, 67591) and chunk_range(cb, pb, 4, 65, 2048) == (67591, 67591)
    for pairs in PAIR_COUNTS:
        cb, pb = tile_segments(pairs)
        covered = []
        for c in range(cb[-1]):
            g = seg_of(cb, c)
            assert cb[g] <= c < cb[g + 1]
            k0, k1 = chunk_range(cb, pb, g, c, 2048)
            assert pb[g] <= k0 <= k1 <= pb[g + 1]
            covered += list(range(k0, k1))
        assert covered == list(range(pb[-1]))
    cb, pb = depth_segments(3, 1025)
    assert cb == [0, 2, 4, 6] and pb == [0, 1025, 2050, 3075]
    assert chunk_range(cb, pb, 1, 3, 1024) == (2049, 2050)


def _segment_argsort(keys, pb):
    return np.concatenate([pb[g] + np.argsort(keys[pb[g]:pb[g + 1]], kind="stable") for g in range(len(pb) - 1)]
                          + [np.zeros(0, np.int64)]).astype(np.int64)


TILE_CASES = [(p, 63) for p in PAIR_COUNTS] + [(p, t) for t in (127, 128, 255, 256, 11999) for p in ([2048, 0, 2049], CYCLE16)]


@pytest.mark.parametrize("pairs,tiles", TILE_CASES, ids=[f"{'_'.join(map(str, p[:8]))}-b{len(p)}-t{t}" for p, t in TILE_CASES])
def test_segmented_tile_sort_is_a_stable_sort_of_every_view(pairs, tiles):
    rng = np.random.default_rng(len(pairs) * 100003 + sum(pairs) + tiles)
    cb, pb = tile_segments(pairs)
    n = pb[-1]
    keys = rng.integers(0, tiles, n).astype(np.int64)
    keys[rng.random(n) < 0.01] = tiles             # sentinel pairs
    for g in range(len(pairs)):                    # the first and the last tile in every view that has two pairs
        if pairs[g] >= 2:
            keys[pb[g]], keys[pb[g + 1] - 1] = tiles - 1, 0
    vals = rng.integers(0, 1 << 20, n).astype(np.int64)
    b0, B0, B1 = tile_plan(tiles)
    assert (b0 == 0) == (tiles <= 127)
    k, v = keys, vals
    if b0:
        k, v = staged_pass_segments(k, v, 0, B0, 2048, tiles, cb, pb)
    k, v = staged_pass_segments(k, v, b0, B1, 2048, tiles, cb, pb)
    order = _segment_argsort(keys, pb)
    assert np.array_equal(k, keys[order]) and np.array_equal(v, vals[order])
    bins = tile_bins_segments(keys, tiles, cb, pb)
    for g in range(len(pairs)):
        kv = k[pb[g]:pb[g + 1]]
        for t in np.unique(kv[kv < tiles]):
            lo, hi = bins[g, t]
            assert pb[g] <= lo < hi <= pb[g + 1] and np.all(k[lo:hi] == t) and hi - lo == np.sum(kv == t)
        assert not bins[g, np.setdiff1d(np.arange(tiles), kv)].any()


@pytest.mark.parametrize("B,N", [(3, 3), (3, 1023), (3, 1025), (16, 1025)])
def test_segmented_depth_sort_is_a_stable_sort_of_every_view(B, N):
    rng = np.random.default_rng(B * 7919 + N)
    depth = (0.5 + 0.25 * rng.integers(0, 40, B * N)).astype(np.float32)       # ~40 values: stability decides
    keys = depth.view(np.uint32).astype(np.int64)
    keys[rng.random(B * N) < 0.1] = 0xFFFFFFFF           # culled splats last
    keys[N:2 * N] = 0xFFFFFFFF                           # a view with every splat culled between two live ones
    vals = np.arange(B * N, dtype=np.int64)
    cb, pb = depth_segments(B, N)
    k, v = keys, vals
    for p in range(4):
        k, v = staged_pass_segments(k, v, 8 * p, 256, 1024, 0xFFFFFFFF, cb, pb)
    order = _segment_argsort(keys, pb)
    assert np.array_equal(k, keys[order]) and np.array_equal(v, vals[order])
    for g in range(B):
        assert np.all((v[pb[g]:pb[g + 1]] >= g * N) & (v[pb[g]:pb[g + 1]] < (g + 1) * N))
