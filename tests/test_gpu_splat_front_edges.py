"""The front half of the splat frame -- project_kernel (unerf_splat_project, _raw, _batch), sh_colors_kernel in its six
instantiations and the tight-list geometry in its two inlinings (the projection's count, map_intersects_kernel's emission) -- on
the hand-placed cases of tests/splat_front_cases.py: bit-exact to the fp32 oracle where the operations are pinned, inside the
float64 reference's per-element bounds where they are not (expf, the sigmoid, the quaternion norm), discrete outputs on the
reference's wide-margin rows, and the structural facts of the tight lists at block_width 16, 8 and 5.  No tolerance here comes
from a kernel result; tests/test_splat_front_cases_cpu.py holds the fp32 oracle to the same bounds.

Pinned decisions (the reasoning is in the case module's docstring): a radius beyond 2^31 saturates to INT_MAX; a mean on the
camera is culled and its colour is 0 at degree >= 1 (the reference model's torch.clamp would give NaN there: it reaches no
pixel).

Share of each bound in use (worst element over all cases; the fp32 oracle's share is printed by the CPU test):
  output          kernel, RAW   kernel, batch views   fp32 oracle = unerf_splat_project (bit-equal)
  xys             0.78          0.74                  0.78
  depths          0 (exact)     0.87                  0 (exact)
  conics          0.06          0.20                  0.14
  compensation    0.03          0.02                  0.04
  cov3d           0.25          0.16                  0.42
  opacities       0.71          (the RAW call's bits)
  shaded rgb      0.96 (degree 0: two roundings against a bound of two)      fp32 oracle 0.96
  beta            0.72                                                         fp32 oracle 0.72
  shaded opacity  0.69                                                         fp32 oracle 0.69
These two columns are the only measured numbers of the suite; no tolerance is taken from them.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import splat_front_cases as FC

pytestmark = pytest.mark.gpu
f32 = np.float32
NAMES = ("xys", "depths", "radii", "conics", "compensation", "num_tiles_hit", "cov3d")
GUARD = -7.0


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _n(t):
    return t.cpu().numpy()


def _same(g, r):
    return (g == r) | (np.isnan(g) & np.isnan(r))


def _V(c):
    return torch.from_numpy(np.asarray(c.V))


def _raw(dev, c, bw, logits=True, antialiased=False, V=None, rows=None):
    from uncertainty_nerf_gs_amd import ops
    sel = slice(None) if rows is None else rows
    out = ops.splat_project(_t(c.means[sel], dev), _t(c.log_scales[sel], dev), 1.0, _t(c.raw_quats[sel], dev),
                            _V(c) if V is None else torch.from_numpy(V), *c.K, bw, raw=True,
                            opacity_logits=_t(c.logits[sel], dev) if logits else None, antialiased=antialiased)
    return [_n(o) for o in out]


def _held(got, ref, rows, what, shares):
    """continuous outputs inside the bounds on `rows`; discrete ones equal to the reference's there"""
    for k, key in enumerate(NAMES):
        if key in FC.CONTINUOUS:
            ok, share = FC.within(got[k], getattr(ref, key), rows)
            shares[key] = max(shares.get(key, 0.0), share)
            assert ok, f"{what}: {key} leaves its float64 bound (share {share:.3g})"
    assert np.array_equal(got[2][rows], ref.radii[rows].astype(np.int32)), f"{what}: radii"
    assert np.array_equal((got[2] > 0)[rows], ref.visible[rows]), f"{what}: visibility"


def _report(what, shares):
    print(f"[share of bound] {what}: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(shares.items())))


@pytest.mark.parametrize("bw", FC.BWS)
@pytest.mark.parametrize("name", list(FC.CASES))
def test_project_is_bit_exact_to_the_fp32_oracle(dev, name, bw):
    """unerf_splat_project on every case, planted rows included.  The non-finite rows are left to
    test_non_finite_rows_stay_in_range (fmaxf drops a NaN that np.maximum keeps); their finite neighbours are held here"""
    from uncertainty_nerf_gs_amd import ops
    c = FC.case(name, bw)
    got = ops.splat_project(_t(c.means, dev), _t(c.scales, dev), 1.0, _t(c.quats, dev), _V(c), *c.K, bw)
    for key, g in zip(NAMES, got):
        g, r = _n(g)[c.finite], c.oracle[key][c.finite]
        same = _same(g, r)
        assert same.all(), f"{key}: {np.count_nonzero(~same)} of {same.size} entries differ, first row {np.nonzero(~same)[0][0]}"
    for p in c.plants:       # the plant's expectation, on the kernel's own output
        i = c.row[p.edge]
        for key in ("radii", "num_tiles_hit"):
            if key in p.expect and "nonfinite" not in p.expect:
                assert int(_n(got[NAMES.index(key)])[i]) == p.expect[key], (p.edge, key)


@pytest.mark.parametrize("bw", FC.BWS)
@pytest.mark.parametrize("name", FC.PROJ_CASES)
def test_raw_projection_is_inside_the_float64_bounds(dev, name, bw):
    """unerf_splat_project_raw: exp of the log-scales, division by the quaternion norm (factors 1e-3 .. 1e3 from unit length),
    sigmoid of the logit [x compensation] -- continuous outputs and the activated opacity inside the per-element bounds,
    radii / visibility / the box's area equal to the reference's on its wide-margin rows"""
    c = FC.case(name, bw)
    shares = {}
    full = _raw(dev, c, bw, logits=False)
    ref = FC.raw_ref(name, bw)
    rows = ref.kept & c.finite
    _held(full, ref, rows, "raw", shares)
    assert np.array_equal(full[5][rows], ref.tiles[rows]), "num_tiles_hit (gsplat's box)"
    for aa in (False, True):
        ref = FC.raw_ref(name, bw, aa)
        got = _raw(dev, c, bw, antialiased=aa)
        for k in (0, 1, 2, 3, 4, 6):
            assert _same(got[k], full[k]).all(), f"{NAMES[k]} changes with the opacity logits"
        assert ((got[5] >= 0) & (got[5] <= full[5])).all()
        ok, share = FC.within(got[7], ref.opacities, rows)
        shares["opacities"] = max(shares.get("opacities", 0.0), share)
        assert ok, f"opacities (antialiased={aa}) leave their bound (share {share:.3g})"
    for p in c.plants:
        if p.expect.get("comp0"):       # compensation 0: antialiased opacity 0, radius > 0, no tile
            i = c.row[p.edge]
            assert got[4][i] == 0 and got[7][i] == 0 and got[2][i] > 0 and got[5][i] == 0 and full[5][i] > 0
    _report(f"raw {name} bw={bw}", shares)


@pytest.mark.parametrize("B", [1, 2, 16])
@pytest.mark.parametrize("name,bw", [("bbox96", 16), ("bbox37", 5), ("near", 8), ("radius", 8)])
def test_batch_views_equal_their_raw_calls_and_the_reference(dev, name, bw, B):
    """unerf_splat_project_batch: every view bit-equal to unerf_splat_project_raw with that camera (tight counts and
    opacities included), inside the float64 bounds, and a camera in front of every splat culls them all"""
    from uncertainty_nerf_gs_amd import ops
    c = FC.case(name, bw)
    Vs = FC.batch_cameras(B)
    cam = c.cam
    views = ops.splat_view_records(Vs, [cam.fx] * B, [cam.fy] * B, [cam.cx] * B, [cam.cy] * B, [np.zeros(3, f32)] * B)
    shares = {}
    for aa in (False, True):
        out = ops.splat_project_batch(_t(c.means, dev), _t(c.log_scales, dev), _t(c.raw_quats, dev), views, B, c.H, c.W, bw,
                                      opacity_logits=_t(c.logits, dev), antialiased=aa)
        out = [_n(o) for o in out]
        singles = {}
        for v in range(B):
            if v % 4 not in singles:
                singles[v % 4] = _raw(dev, c, bw, antialiased=aa, V=Vs[v])
            one = singles[v % 4]
            for k, j in ((0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (6, 7)):      # (batch has no cov3d)
                assert _same(out[k][v], one[j]).all(), f"view {v}: {NAMES[j] if j < 7 else 'opacities'} differs from the raw call"
        for v in range(min(B, 4)):
            ref = FC.project_ref(c.means, c.log_scales, c.raw_quats, Vs[v], cam, bw, True, c.logits, aa)
            rows = ref.kept & c.finite
            _held(singles[v], ref, rows, f"view {v}", shares)
            if v == 2:
                assert not ref.live.any() and not out[2][v].any() and not out[5][v].any()
    _report(f"batch {name} bw={bw} B={B}", shares)


@pytest.mark.parametrize("bw", FC.BWS)
def test_non_finite_rows_stay_in_range(dev, bw):
    """a NaN or Inf mean, an Inf log-scale, a zero quaternion, a NaN opacity logit on all three entry points.  The emission
    kernel's memory safety rests on radii == 0 or 0 <= num_tiles_hit <= tbx tby for such rows: that is asserted on the host
    and nothing downstream is launched.  num_tiles_hit == 0 wherever the centre is non-finite; the finite neighbours keep the
    bits they have without the bad rows."""
    from uncertainty_nerf_gs_amd import ops
    c = FC.case("nonfinite", bw)
    tbx, tby = FC.tiles_of(c.H, c.W, bw)
    centre = np.array([c.row[p.edge] for p in c.plants if p.expect.get("nonfinite") == "centre"])
    assert len(c.nonfinite) == 9 and len(centre) == 4
    clean = np.nonzero(c.finite)[0]

    def in_range(radii, tiles, what):
        bad = ~((radii == 0) | ((tiles >= 0) & (tiles <= tbx * tby)))
        assert not bad.any(), f"{what}: rows {np.nonzero(bad)[0]} radii {radii[bad]} num_tiles_hit {tiles[bad]}"
        assert (tiles[centre] == 0).all() and (radii[centre] == 0).all(), what
        assert (tiles >= 0).all(), what

    plain = [_n(o) for o in ops.splat_project(_t(c.means, dev), _t(c.scales, dev), 1.0, _t(c.quats, dev), _V(c), *c.K, bw)]
    in_range(plain[2], plain[5], "project")
    i = c.row["-Inf mean z"]
    assert plain[2][i] == 0 and plain[5][i] == 0
    Vs = FC.batch_cameras(2)
    views = ops.splat_view_records(Vs, [c.cam.fx] * 2, [c.cam.fy] * 2, [c.cam.cx] * 2, [c.cam.cy] * 2, [np.zeros(3, f32)] * 2)
    for logits in (False, True):
        for aa in (False, True):
            raw = _raw(dev, c, bw, logits=logits, antialiased=aa)
            in_range(raw[2], raw[5], f"raw logits={logits} antialiased={aa}")
            alone = _raw(dev, c, bw, logits=logits, antialiased=aa, rows=clean)
            for k in range(len(raw)):
                assert _same(raw[k][clean], alone[k]).all(), f"a finite neighbour's {k}-th output moved"
            out = ops.splat_project_batch(_t(c.means, dev), _t(c.log_scales, dev), _t(c.raw_quats, dev), views, 2, c.H, c.W, bw,
                                          opacity_logits=_t(c.logits, dev) if logits else None, antialiased=aa)
            for v in range(2):
                in_range(_n(out[2])[v], _n(out[5])[v], f"batch view {v} logits={logits} antialiased={aa}")
            assert _same(_n(out[5])[0], raw[5]).all()


# ------------------------------------------------------------------ shading ------------------------------------------------
def _shade_all(dev, c, degree, rest_offset=0):
    """every entry point on the poisoned coefficients -> dict of host arrays.  rest_offset: features_rest starts that many
    floats into a larger (16-byte aligned) buffer -- 1 forces the non-STAGE path at degree 3"""
    from uncertainty_nerf_gs_amd import ops
    dc, rest, un = FC.poisoned(c, degree)
    N = c.N
    means, cam = _t(c.means, dev), torch.from_numpy(c.cam_pos)
    lu, lg, comp, dep = _t(c.log_unc, dev), _t(c.logits, dev), _t(c.comp, dev), _t(c.depths, dev)
    tdc = _t(dc, dev)
    trest = None
    if rest is not None:
        buf = torch.full((N * 45 + 8,), float("nan"), device=dev)
        assert buf.data_ptr() % 16 == 0
        buf[rest_offset:rest_offset + N * 45] = _t(rest.reshape(-1), dev)
        trest = buf[rest_offset:rest_offset + N * 45].view(N, 15, 3)
        assert trest.data_ptr() % 16 == 4 * rest_offset and trest.is_contiguous()
    r = {}
    if rest_offset == 0:
        r["unpacked"] = ops.splat_sh_colors(degree, means, cam, _t(un, dev), lu, 0.01)
    r["split"] = ops.splat_sh_colors_split(degree, means, cam, tdc, trest, lu, 0.01)
    r["pack5"] = ops.splat_shade_inputs(degree, means, cam, tdc, trest, lu, 0.01, lg, comp, dep)
    r["pack5_nocomp"] = ops.splat_shade_inputs(degree, means, cam, tdc, trest, lu, 0.01, lg, None, dep)
    r["pack4"] = ops.splat_shade_inputs(degree, means, cam, tdc, trest, None, 0.01, lg, comp, dep)
    cams = [c.cam_pos, c.cam_pos + f32([1, 0.5, -2]), c.cam_pos]
    for B in (1, 3):
        views = ops.splat_view_records([FC.V_ID] * B, [1.0] * B, [1.0] * B, [0.0] * B, [0.0] * B, cams[:B])
        rep = lambda a: a[None].expand(B, N).contiguous()
        r[f"batch{B}"] = ops.splat_shade_inputs_batch(degree, means, views, B, tdc, trest, lu, 0.01, lg, rep(comp), rep(dep))
    torch.cuda.synchronize()
    return {k: tuple(None if x is None else _n(x) for x in v) for k, v in r.items()}


@pytest.mark.parametrize("degree", [-1, 0, 1, 2, 3])
@pytest.mark.parametrize("N", FC.NS)
def test_shading_forms_agree_and_stay_inside_the_bounds(dev, N, degree):
    """degrees -1 .. 3 on unerf_splat_sh_colors, _split, unerf_splat_shade_inputs (C = 5 and 4, with and without the
    compensation) and _batch (B = 1, 3), with every coefficient the degree does not use set to NaN and features_rest NULL at
    degree <= 0: all forms give the same bits, the bits lie inside the float64 bounds, and no NaN reaches an output.  N % 4 != 0
    runs the STAGE copy's scalar tail (degree 3, aligned rows); features_rest one float off 16-byte alignment takes the packed
    4-byte-aligned quads instead and must give the same bits."""
    c = FC.shade_case(N)
    dc, rest, un = FC.poisoned(c, degree)
    r = _shade_all(dev, c, degree)
    ref = FC.shade_ref(degree, c.means, c.cam_pos, dc, rest, c.log_unc, 0.01, c.logits, c.comp, c.depths)
    ref_nc = FC.shade_ref(degree, c.means, c.cam_pos, dc, rest, c.log_unc, 0.01, c.logits, None, c.depths)
    col, beta = r["split"]
    shares = {}
    on = c.on_camera if degree >= 1 else None
    if on is not None:       # 0 / 0 view direction: the kernels' fmaxf(NaN + 0.5, 0) is 0 (the splat is culled: tz = 0)
        assert (col[on] == 0).all()
    for key, got, e in (("rgb", col, ref.rgb), ("beta", beta, ref.beta), ("opacities", r["pack5"][1], ref.opacities),
                        ("opacities", r["pack5_nocomp"][1], ref_nc.opacities)):
        assert not np.isnan(got).any(), f"{key}: a NaN reached an output"
        ok, share = FC.within(got, e)
        shares[key] = max(shares.get(key, 0.0), share)
        assert ok, f"{key} leaves its float64 bound (share {share:.3g})"
    _report(f"shade N={N} degree={degree}", shares)
    # one result, whatever the form
    assert _same(r["unpacked"][0], col).all() and _same(r["unpacked"][1], beta).all()
    rows5 = np.concatenate([col, beta[:, None], c.depths[:, None]], 1)
    rows4 = np.concatenate([col, c.depths[:, None]], 1)
    assert np.array_equal(r["pack5"][0], rows5) and np.array_equal(r["pack5_nocomp"][0], rows5)
    assert np.array_equal(r["pack4"][0], rows4) and np.array_equal(r["pack4"][1], r["pack5"][1])
    assert np.array_equal(r["batch1"][0][0], rows5) and np.array_equal(r["batch1"][1][0], r["pack5"][1])
    for v in (0, 2):
        assert np.array_equal(r["batch3"][0][v], rows5) and np.array_equal(r["batch3"][1][v], r["pack5"][1])
    if degree >= 1:          # view 1 looks from elsewhere: its own reference
        cam1 = c.cam_pos + f32([1, 0.5, -2])
        ref1 = FC.shade_ref(degree, c.means, cam1, dc, rest, c.log_unc, 0.01, c.logits, c.comp, c.depths)
        ok, share = FC.within(r["batch3"][0][1][:, :3], ref1.rgb)
        assert ok and not np.array_equal(r["batch3"][0][1][:, :3], col), f"batch view 1 (share {share:.3g})"
    else:
        assert np.array_equal(r["batch3"][0][1], rows5)
    assert np.array_equal(r["batch3"][0][1][:, 3:], rows5[:, 3:])
    if rest is not None:     # off 16-byte alignment: the non-STAGE kernels, the same bits
        m = _shade_all(dev, c, degree, rest_offset=1)
        for k in m:
            for a, b in zip(m[k], r[k]):
                assert (a is None and b is None) or np.array_equal(a, b), f"{k}: misaligned features_rest changes the result"


def test_misaligned_sh_coeffs_are_refused_before_any_launch(dev, lib):
    from uncertainty_nerf_gs_amd import ops
    c = FC.shade_case(257)
    un = FC.poisoned(c, 3)[2]
    buf = torch.zeros(c.N * 48 + 4, device=dev)
    buf[1:1 + c.N * 48] = _t(un.reshape(-1), dev)
    off = buf[1:1 + c.N * 48].view(c.N, 16, 3)
    assert off.data_ptr() % 16 == 4
    colors = torch.full((c.N, 3), GUARD, device=dev)
    h = lib.load()
    cp = (C.c_float * 3)(*[float(x) for x in c.cam_pos])
    rc = h.unerf_splat_sh_colors(3, _t(c.means, dev).data_ptr(), cp, off.data_ptr(), None, 0.01, c.N, colors.data_ptr(), None,
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0 and b"16-byte aligned" in h.unerf_last_error()
    assert bool((colors == GUARD).all())
    with pytest.raises(lib.UnerfError, match="16-byte aligned"):
        ops.splat_sh_colors(3, _t(c.means, dev), torch.from_numpy(c.cam_pos), off)


@pytest.mark.parametrize("N,degree", [(255, 3), (257, 3), (3, 3), (257, 1), (1, 0)])
def test_shading_guard_rows_streams_and_repeats(dev, lib, N, degree):
    """unerf_splat_shade_inputs through the C ABI into NaN-filled buffers with guard rows behind row N, three times, the second
    on a side stream: the same bits each time (and the ones the wrapper gives), and the guard rows keep their NaN"""
    from uncertainty_nerf_gs_amd import ops
    c = FC.shade_case(N)
    dc, rest, _ = FC.poisoned(c, degree)
    h = lib.load()
    means, tdc, lu, lg, comp, dep = (_t(a, dev) for a in (c.means, dc, c.log_unc, c.logits, c.comp, c.depths))
    trest = None if rest is None else _t(rest, dev)
    cp = (C.c_float * 3)(*[float(x) for x in c.cam_pos])
    want = ops.splat_shade_inputs(degree, means, torch.from_numpy(c.cam_pos), tdc, trest, lu, 0.01, lg, comp, dep)
    side = torch.cuda.Stream(device=dev)
    for it in range(3):
        rows = torch.full((N + 3, 5), float("nan"), device=dev)
        opac = torch.full((N + 3,), float("nan"), device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side if it == 1 else torch.cuda.current_stream()):
            rc = h.unerf_splat_shade_inputs(degree, means.data_ptr(), cp, tdc.data_ptr(), None if trest is None else trest.data_ptr(),
                                            lu.data_ptr(), 0.01, lg.data_ptr(), comp.data_ptr(), dep.data_ptr(), N, 5, rows.data_ptr(),
                                            opac.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0
        assert bool(torch.isnan(rows[N:]).all()) and bool(torch.isnan(opac[N:]).all())
        assert torch.equal(rows[:N], want[0]) and torch.equal(opac[:N], want[1])


# ------------------------------------------------------------------ tight lists --------------------------------------------
def _members(gids, bins, base, total, N, depths, tiles):
    """-> membership [tiles, N] of one view's lists; asserts depth order and no duplicate inside a tile, and that the tile
    ranges cover [base, base + total) exactly once -- so no entry carries the sentinel tile"""
    m = np.zeros((tiles, N), bool)
    spans = sorted((int(a), int(b)) for a, b in bins if b > a)
    at = base
    for a, b in spans:
        assert a == at, "tile ranges leave a gap: some entry belongs to no tile"
        at = b
    assert at == base + total or (total == 0 and not spans)
    for t, (a, b) in enumerate(bins):
        ids = gids[a:b] % N if b > a else gids[:0]
        assert (np.diff(depths[ids]) >= 0).all(), f"tile {t}: depth order"
        assert len(np.unique(ids)) == len(ids), f"tile {t}: duplicate ids"
        m[t, ids] = True
    return m


@pytest.mark.parametrize("mode", ["classic", "antialiased"])
@pytest.mark.parametrize("bw", FC.BWS)
@pytest.mark.parametrize("name", FC.TIGHT_CASES)
def test_tight_lists_at_every_block_width(dev, name, bw, mode):
    """splat_project(raw=True, opacity_logits=...) -> splat_bin_sort(tight=...): need (the float64 brute force over pixel
    centres) is inside the tight lists, those inside gsplat's box; depth order, no duplicates; the total is sum num_tiles_hit
    and every splat is listed exactly num_tiles_hit times (count and emission agree: no sentinel entry); the count equals the
    float64 restatement's wherever that is sure of it; sub-gate and comp == 0 splats are in no list.  The batch form
    (B = 2) gives view 0 the same lists."""
    from uncertainty_nerf_gs_amd import ops
    c = FC.case(name, bw)
    aa = mode == "antialiased"
    N, H, W = c.N, c.H, c.W
    tbx, tby = FC.tiles_of(H, W, bw)
    args = (_t(c.means, dev), _t(c.log_scales, dev), 1.0, _t(c.raw_quats, dev), _V(c)) + c.K + (bw,)
    xys, depths, radii, conics, comp, nth, _, opac = ops.splat_project(*args, raw=True, opacity_logits=_t(c.logits, dev), antialiased=aa)
    nth_full = _n(ops.splat_project(*args, raw=True)[5])
    h = [_n(x) for x in (xys, depths, radii, conics, comp, nth, opac)]
    hx, hd, hr, hc, _, hn, ho = h
    assert ((hn >= 0) & (hn <= nth_full)).all() and (hn[hr == 0] == 0).all()       # in range before anything walks them
    I, _, _, gids, bins = ops.splat_bin_sort(xys, depths, radii, nth, H, W, bw, want_isect_ids=False, tight=(conics, opac))
    assert I == int(hn.sum())
    mt = _members(_n(gids), _n(bins), 0, I, N, hd, tbx * tby)
    assert np.array_equal(mt.sum(0), hn), "a splat is listed in another number of tiles than the projection counted"
    need, box = FC.need_pairs(hx, hc, ho, hr, H, W, bw)
    assert not (mt & ~box).any(), "a tight entry outside gsplat's box"
    missing = need & ~mt
    assert not missing.any(), f"{int(missing.sum())} blending (tile, splat) pairs are not in the tight lists"
    If, _, _, gids_f, bins_f = ops.splat_bin_sort(xys, depths, radii, _t(nth_full, dev), H, W, bw, want_isect_ids=False)
    mf = _members(_n(gids_f), _n(bins_f), 0, If, N, hd, tbx * tby)
    assert np.array_equal(mf, box), "the box lists are not gsplat's box"
    cnt, sure, totals = FC.tight_count_np(hx, hc, ho, FC.tile_bbox_np(hx[:, 0], hx[:, 1], hr.astype(f32), bw, H, W), bw)
    chk = sure & (hr > 0)
    assert np.array_equal(hn[chk], cnt[chk]), f"rows {np.nonzero(chk & (hn != cnt))[0][:8]}: count differs from the restatement"
    for p in c.plants:
        i = c.row[p.edge]
        if p.expect.get("listed") is False or (aa and p.expect.get("comp0")):
            assert hr[i] > 0 and hn[i] == 0 and not mt[:, i].any(), p.edge
        if "rows" in p.expect:
            assert len(np.unique(np.nonzero(need[:, i])[0] // tbx)) == p.expect["rows"], p.edge
            assert len(np.unique(np.nonzero(mt[:, i])[0] // tbx)) >= p.expect["rows"], p.edge
        if "round_total" in p.expect:
            assert hn[i] == p.expect["round_total"], p.edge
        if "opacity" in p.expect and not aa:
            assert ho[i] == f32(p.expect["opacity"]), p.edge
    # the batch form: view 0 = this camera, view 1 shifted
    Vs = FC.batch_cameras(2)
    views = ops.splat_view_records(Vs, [c.cam.fx] * 2, [c.cam.fy] * 2, [c.cam.cx] * 2, [c.cam.cy] * 2, [np.zeros(3, f32)] * 2)
    bx, bd, br, bc, _, bn, bo = ops.splat_project_batch(args[0], args[1], args[3], views, 2, H, W, bw, opacity_logits=_t(c.logits, dev),
                                                        antialiased=aa)
    hbn, hbr = _n(bn), _n(br)
    full_b = _n(ops.splat_project_batch(args[0], args[1], args[3], views, 2, H, W, bw)[5])
    assert ((hbn >= 0) & (hbn <= full_b)).all() and np.array_equal(hbn[0], hn)
    count = ops.SplatCountBatch(bn, br)
    totals_b, visible, bg, bb = ops.splat_bin_sort_batch(bx, bd, br, count, H, W, bw, tight=(bc, bo))
    assert list(totals_b) == [int(hbn[0].sum()), int(hbn[1].sum())]
    bg, bb, hbd = _n(bg), _n(bb), _n(bd)
    assert np.array_equal(bg[:I], _n(gids)) and np.array_equal(bb[0], _n(bins))
    m1 = _members(bg, bb[1], I, totals_b[1], N, hbd[1], tbx * tby)
    assert np.array_equal(m1.sum(0), hbn[1])
    need1, box1 = FC.need_pairs(_n(bx)[1], _n(bc)[1], _n(bo)[1], hbr[1], H, W, bw)
    assert not (m1 & ~box1).any() and not (need1 & ~m1).any()
