"""The hand-placed cases of tests/splat_front_cases.py, checked without a GPU: every plant lands on its edge (on the fp32
oracle's values), the fp32 oracle stays inside the float64 reference's bounds on every kept element, the share of random-fill
rows whose discrete outputs are left out stays under the cap, every planted mutation of the numpy restatements fails on at
least one case (the one equivalent mutant is shown to be equivalent), and the float64 brute force over pixel centres that
defines the blending (tile, splat) pairs is contained in gsplat's box and in the restated tight lists.  That is what lets
tests/test_gpu_splat_front_edges.py hold the kernels to the reference."""
import numpy as np
import pytest

import splat_front_cases as FC
from oracle import splat_oracle as SO

f32 = np.float32
ALL = [(n, bw) for n in FC.CASES for bw in FC.BWS]


def test_sizes_cover_the_awkward_remainders():
    ns = sorted({FC.CASES[k][0] for k in FC.CASES})
    assert ns == sorted(FC.NS)
    assert {n % 4 for n in ns} >= {0, 1, 3} and {n % 256 for n in ns} >= {0, 1, 3, 255}
    assert all(H * W <= 96 * 80 for _, H, W, _ in FC.CASES.values())
    assert {(W, H) for _, H, W, _ in FC.CASES.values()} >= {(37, 50), (5, 50), (96, 80)}


@pytest.mark.parametrize("name,bw", ALL)
def test_plants_land_on_their_edges(name, bw):
    c = FC.case(name, bw)
    o = c.oracle
    assert len(c.plants) == min(len(FC.CASES[name][3](c.cam, bw)), c.N)
    box = FC.tile_bbox_np(o["xys"][:, 0], o["xys"][:, 1], o["radii"].astype(f32), bw, c.H, c.W)
    for k, p in enumerate(c.plants):
        i, ex = c.first_plant + k, p.expect
        if "nonfinite" in ex and ex.get("radii") is None:
            continue
        for key in ("radii", "num_tiles_hit"):
            if key in ex:
                assert o[key][i] == ex[key], (p.edge, key, o[key][i], ex[key])
        if ex.get("xys") is not None and o["radii"][i] > 0:
            assert tuple(o["xys"][i]) == tuple(ex["xys"]), p.edge            # exactly on the planted pixel position
        if ex.get("box") is not None:
            assert tuple(int(b[i]) for b in box) == ex["box"], p.edge
        if ex.get("visible"):
            assert o["radii"][i] > 0 and o["num_tiles_hit"][i] > 0, p.edge
        if "pre" in ex:
            assert FC._pre32(p.scale[0]) == f32(ex["pre"])
        if "same_conics_as" in ex:       # clamped: the conics of the plant ON the limit, bit for bit
            assert np.array_equal(o["conics"][i], o["conics"][i + ex["same_conics_as"]]), p.edge
        if "differs_from" in ex:
            assert not np.array_equal(o["conics"][i], o["conics"][i + ex["differs_from"]]), p.edge
        if ex.get("det") == "zero":
            assert (o["conics"][i] == 0).all() and (o["cov3d"][i] != 0).any() and o["radii"][i] == 0
        if ex.get("det") == "negative":
            assert o["conics"][i, 0] < 0
    if name == "near":       # the three planes really are one ulp apart around fp32(0.01)
        z = c.means[[c.row["tz one ulp below clip: culled"], c.row["tz == clip: culled"], c.row["tz one ulp above clip: kept"]], 2]
        assert z[1] == f32(0.01) and np.nextafter(z[0], f32(1)) == z[1] and np.nextafter(z[1], f32(1)) == z[2]


@pytest.mark.parametrize("name,bw", ALL)
def test_fp32_oracle_is_inside_the_bounds_and_the_cap_holds(name, bw):
    c = FC.case(name, bw)
    ref, o = FC.plain_ref(name, bw), c.oracle
    rows = ref.kept & c.finite
    for key in FC.CONTINUOUS:
        ok, share = FC.within(o[key], getattr(ref, key), rows)
        print(f"{name} bw={bw} {key}: fp32 oracle uses {share:.3f} of the bound")
        assert ok, key
    assert np.array_equal(o["radii"][rows], ref.radii[rows].astype(np.int32))
    assert np.array_equal(o["num_tiles_hit"][rows], ref.tiles[rows])
    assert np.array_equal((o["radii"] > 0)[rows], ref.visible[rows])
    for r, antialiased in ((ref, False), (FC.raw_ref(name, bw), False), (FC.raw_ref(name, bw, True), True)):
        share = FC.excluded_share(c, r)
        print(f"{name} bw={bw}: {share:.3%} of the fill left out of the discrete comparison")
        assert share <= FC.MAX_EXCLUDED
    assert rows.sum() >= 0.9 * c.is_fill.sum()


@pytest.mark.parametrize("degree", [-1, 0, 1, 2, 3])
@pytest.mark.parametrize("N", FC.NS)
def test_fp32_shading_oracle_is_inside_the_bounds(N, degree):
    c = FC.shade_case(N)
    dc, rest, un = FC.poisoned(c, degree)
    ref = FC.shade_ref(degree, c.means, c.cam_pos, dc, rest, c.log_unc, 0.01, c.logits, c.comp, c.depths)
    with np.errstate(all="ignore"):
        if degree < 0:
            col = (f32(1) / (f32(1) + np.exp(-dc))).astype(f32)
        else:
            col = np.maximum(SO.spherical_harmonics(degree, c.means - c.cam_pos, np.nan_to_num(un)) + f32(0.5), f32(0))
        beta = SO.softplus(c.log_unc) + f32(0.01)
        opac = (f32(1) / (f32(1) + np.exp(-c.logits))).astype(f32) * c.comp
    for key, got, r in (("rgb", col, ref.rgb), ("beta", beta, ref.beta), ("opacities", opac, ref.opacities)):
        ok, share = FC.within(got, r)
        print(f"N={N} degree={degree} {key}: fp32 oracle uses {share:.3f} of the bound")
        assert ok, key
    assert not np.isnan(ref.beta.v).any() and not np.isnan(ref.opacities.v).any()
    if degree >= 1 and c.on_camera is not None:
        assert np.isnan(ref.rgb.v[c.on_camera]).all()        # 0 / 0 in the reference; the kernels write 0 (module docstring)
        assert np.isfinite(np.delete(ref.rgb.v, c.on_camera, 0)).all()
    else:
        assert np.isfinite(ref.rgb.v).all()                  # no NaN coefficient reached a colour


def _caught(mut):
    """-> names of the cases on which the mutated restatement differs from the true one (which equals the fp32 oracle)"""
    hits = []
    if mut == "lt":
        for name, bw in ALL:
            c = FC.case(name, bw)
            with np.errstate(all="ignore"):
                if (FC.visible_np(c.means[:, 2], mutate="lt") != FC.visible_np(c.means[:, 2]))[c.finite].any():
                    hits.append((name, bw))
    elif mut in ("floor", "no_plus1", "tbx_floor"):
        for name, bw in ALL:
            c = FC.case(name, bw)
            o = c.oracle
            live = o["radii"] > 0
            args = (o["xys"][:, 0], o["xys"][:, 1], o["radii"].astype(f32), bw, c.H, c.W)
            a, b = FC.tile_bbox_np(*args), FC.tile_bbox_np(*args, mutate=mut)
            area = lambda t: ((t[2] - t[0]) * (t[3] - t[1]))[live]
            assert np.array_equal(area(a), o["num_tiles_hit"][live])          # the restatement IS the oracle's box
            if not np.array_equal(area(a), area(b)):
                hits.append((name, bw))
    elif mut == "no_tail":
        for N in FC.NS:
            nb = N % 256 or 256
            want = np.where(np.arange(256 * 45) < nb * 45, np.arange(256 * 45), -1)
            assert np.array_equal(FC.stage_copy_map(nb), want)
            if not np.array_equal(FC.stage_copy_map(nb, "no_tail"), want):
                hits.append(N)
    else:
        degree = int(mut[-1])
        for N in FC.NS:
            c = FC.shade_case(N)
            dc, rest, un = FC.poisoned(c, 3)      # every coefficient finite: the restatement against the oracle
            for layout in ("split", "unpacked"):
                assert FC.floats_used(degree, layout) <= FC.quads_read(degree, layout)
                want = FC.shade_np(degree, c.means, c.cam_pos, dc, rest, layout)
                with np.errstate(all="ignore"):
                    orc = np.maximum(SO.spherical_harmonics(degree, c.means - c.cam_pos, un) + f32(0.5), f32(0))
                assert np.array_equal(want, orc, equal_nan=True)
                got = FC.shade_np(degree, c.means, c.cam_pos, dc, rest, layout, mutate="extra_quad")
                if not np.array_equal(want, got, equal_nan=True):
                    hits.append((N, layout))
    return hits


@pytest.mark.parametrize("mut", FC.MUTATIONS)
def test_every_planted_mutation_is_caught(mut):
    hits = _caught(mut)
    print(f"{mut}: differs on {len(hits)} cases, e.g. {hits[:4]}")
    if mut in FC.EQUIVALENT:
        assert not hits       # floor and truncation differ on (-1, 0) only, and max(0, .) clamps both: no case can tell them apart
        with np.errstate(all="ignore"):
            a = f32(np.linspace(-3, 3, 2001))
            z = np.zeros_like(a)
            assert np.array_equal(FC.tile_bbox_np(a * 16, z, z, 16, 64, 64)[0], FC.tile_bbox_np(a * 16, z, z, 16, 64, 64, "floor")[0])
    else:
        assert hits


def test_quad_loads_fetch_more_than_the_degree_uses():
    """the surplus the NaN-poisoned coefficients guard: (read, used) floats per degree and layout"""
    got = {(d, l): (FC.quads_read(d, l), FC.floats_used(d, l)) for d in (0, 1, 2, 3) for l in ("unpacked", "split")}
    assert got[(0, "unpacked")] == (4, 3) and got[(1, "unpacked")] == (12, 12) and got[(2, "unpacked")] == (28, 27)
    assert got[(1, "split")] == (12, 9) and got[(2, "split")] == (24, 24) and got[(3, "split")] == (45, 45)
    assert got[(3, "unpacked")] == (48, 48) and got[(0, "split")] == (0, 0)


@pytest.mark.parametrize("name", FC.TIGHT_CASES)
@pytest.mark.parametrize("bw", FC.BWS)
def test_blending_pairs_lie_in_the_box_and_in_the_restated_tight_lists(name, bw):
    """the `need` set of test_tight_tile_lists_are_conservative, generalised to bw, on the fp32 oracle's projection"""
    c = FC.case(name, bw)
    o = c.oracle
    with np.errstate(all="ignore"):
        opac = (f32(1) / (f32(1) + np.exp(-c.logits))).astype(f32)
    need, box = FC.need_pairs(o["xys"], o["conics"], opac, o["radii"], c.H, c.W, bw)
    assert not (need & ~box).any()
    bx = FC.tile_bbox_np(o["xys"][:, 0], o["xys"][:, 1], o["radii"].astype(f32), bw, c.H, c.W)
    cnt, sure, totals = FC.tight_count_np(o["xys"], o["conics"], opac, bx, bw)
    vis = o["radii"] > 0
    assert (need.sum(0)[vis] <= cnt[vis]).all() and (cnt[vis] <= box.sum(0)[vis]).all()
    assert need.sum() > 0.4 * cnt[vis].sum() or name == "one"
    tbx, tby = FC.tiles_of(c.H, c.W, bw)
    for p in c.plants:
        i = c.row[p.edge]
        if "rows" in p.expect:          # the tall splats: the blending pairs span exactly k tile rows
            rows = np.unique(np.nonzero(need[:, i])[0] // tbx)
            assert len(rows) == p.expect["rows"], (p.edge, len(rows))
        if "round_total" in p.expect:
            assert sure[i] and totals[i] == [p.expect["round_total"]], (p.edge, totals[i])
        if p.expect.get("listed") is False:
            assert cnt[i] == 0 and need[:, i].sum() == 0 and o["radii"][i] > 0
        if "opacity" in p.expect:
            assert opac[i] == f32(p.expect["opacity"])
        if "tangent" in p.expect:       # the ellipse's end is within 1e-4 px of the pixel-centre line it is tangent to
            a, cc_ = np.float64(o["conics"][i, 0]), np.float64(o["conics"][i, 2])
            tau = np.log(255.0 * np.float64(opac[i]))
            h = np.sqrt(2 * tau / (cc_ if p.expect["tangent"] == "row" else a))
            assert abs(h - (bw + 0.5)) < 1e-4, (p.edge, h)
    if name == "tight_wide":
        g = [float(opac[c.row[e]]) for e in c.row if e.startswith("opacity 0.003")]
        assert g[0] < 0.0039 < g[1] < 1 / 255 < g[2]
    if name == "tight_wide":
        # the emission's rounds: sure splats whose 8-row round totals are 8 k and 8 k + 1
        seen = {t for i in np.nonzero(sure & vis)[0] for t in totals[i]}
        print(f"{name} bw={bw}: round totals seen {sorted(seen)}")
        assert {8, 9, 16, 17} <= seen
