"""tests/lpips_edge_cases.py without a GPU: every case reaches the edge it is named for (computed from the lib constants),
the planted values are where and what the case says, a numpy twin of each kernel's algorithm stays inside every bound,
and each named planted defect of a twin misses at least one case."""
import numpy as np
import pytest
import torch

import lpips_cases as LC
import lpips_edge_cases as EC
from conftest import ROOT
from uncertainty_nerf_gs_amd import lib as L
from uncertainty_nerf_gs_amd import metrics as M


def test_the_constants_the_cases_are_built_from():
    assert (EC.EW, EC.EW_MAX_WG, EC.KS) == (L.LPIPS_EW_THREADS, L.LPIPS_EW_MAX_WG, L.LPIPS_CONV_STEP_K)
    assert EC.E == L.LPIPS_EW_THREADS * L.LPIPS_EW_MAX_WG and EC.E % 3 != 0     # the channel phase moves from trip to trip
    assert EC.BMAX == L.METRICS_MAX_IMAGES <= EC.WAVE                           # one block of 64 threads: a thread per image
    assert EC.HP % EC.HEAD_WAVES == 0 and EC.EW % EC.WAVE == 0
    # the source takes its constants from the header, and says why 64 images is the limit
    text = open(f"{ROOT}/uncertainty-nerf-gs_amd/csrc/unerf_lpips.hip").read()
    for use in ("EW_THREADS = UNERF_LPIPS_EW_THREADS", "EW_MAX_WG = UNERF_LPIPS_EW_MAX_WG", "CV_BK = UNERF_LPIPS_CONV_STEP_K",
                "static_assert(UNERF_METRICS_MAX_IMAGES <= 64"):
        assert use in text, use


# ---- pack -------------------------------------------------------------------------------------------------------------

def test_pack_cases_sit_on_both_sides_of_a_block_and_of_the_cap():
    c = {p.name: p for p in EC.PACK_CASES}
    grid = {k: EC.ew_grid(3 * v.n) for k, v in c.items()}
    trips = {k: EC.ew_trips(3 * v.n) for k, v in c.items()}
    assert 3 * c["one-block"].n <= EC.EW < 3 * c["two-blocks"].n and (grid["one-block"], grid["two-blocks"]) == (1, 2)
    assert c["two-blocks"].n == c["one-block"].n + 1 and c["cap-plus"].n == c["cap"].n + 1
    assert 3 * c["cap"].n <= EC.E < 3 * c["cap-plus"].n and 3 * c["cap-plus"].n - EC.E == 2
    assert grid["cap"] == grid["cap-plus"] == grid["three-trips"] == EC.EW_MAX_WG
    assert (trips["one-block"], trips["two-blocks"], trips["cap"], trips["cap-plus"], trips["three-trips"]) == (1, 1, 1, 2, 3)
    assert 0 < 3 * c["three-trips"].n - 2 * EC.E < EC.E and c["three-trips"].B == 2
    assert (3 * c["three-trips"].n - 2 * EC.E) % EC.WAVE != 0                   # the last trip ends inside a wave
    for case in EC.PACK_CASES:                                                   # the C entry's own limit
        assert 6 * case.n * case.B < 2 ** 31 and 1 <= case.B <= EC.BMAX


@pytest.mark.parametrize("case", EC.PACK_CASES, ids=lambda c: c.name)
def test_pack_plants_are_where_the_case_says_and_counted_on_the_host(case):
    plants = EC.pack_plants(case)
    n3 = 3 * case.n
    assert len({(b, which, i) for b, which, i, _, _ in plants}) == len(plants), "two plants in one place"
    trip_of = lambda i: i // (EC.ew_grid(n3) * EC.EW)
    trips = EC.ew_trips(n3)
    by_trip = {t: [p for p in plants if trip_of(p[2]) == t] for t in range(trips)}
    assert any(p[2] == n3 - 1 and p[4] for p in plants), "the last element"
    for t in {0, trips - 1}:
        kinds = {(which, "nan" if v != v else "low" if v < 0 else "high") for _, which, _, v, counted in by_trip[t] if counted}
        assert {("pred", "nan"), ("pred", "low"), ("target", "high")} <= kinds, (t, kinds)
    if trips > 1:
        assert any(which == "pred" and v > 1 and not counted and trip_of(i) > 0 for _, which, i, v, counted in plants)
    if trips > 2:
        assert by_trip[1]
    pred, target, want = EC.pack_inputs(case)
    assert pred.shape == target.shape == (case.B, case.n, 3)
    for b, which, i, v, _ in plants:
        got = float((pred if which == "pred" else target)[b].view(-1)[i])
        assert (got != got) if v != v else got == np.float32(v)
    _, bad = EC.pack_reference(pred, target, LC.weights())
    assert bad == want and sum(want) == sum(p[4] for p in plants) > 0


# ---- pool -------------------------------------------------------------------------------------------------------------

def test_pool_cases_reach_their_edges():
    c = {p.name: p for p in EC.POOL_CASES}
    total = lambda p: p.N * EC.pool_out(p.H) * EC.pool_out(p.W) * p.C
    sq, hp = c["cap-square"], c["cap-h-plus-1"]
    assert sq.H == sq.W and total(sq) > EC.E >= sq.N * EC.pool_out(sq.H - 1) ** 2 * sq.C
    assert EC.ew_trips(total(sq)) == 2 and EC.ew_grid(total(sq)) == EC.EW_MAX_WG and EC.ew_trips(total(c["4x6-c65"])) == 1
    assert (hp.H, hp.W) == (sq.H + 1, sq.W) and total(hp) == total(sq)           # the added row is in no window
    for p in (c["4x6-c65"], hp):
        assert 2 * (EC.pool_out(p.H) - 1) + 2 < p.H - 1                          # the last row is never read
        n, y, x, ch, v = p.plants[-1]
        assert (n, y, x, ch) == (p.N - 1, p.H - 1, p.W - 1, p.C - 1) and v != v  # the last input element holds a NaN
    assert c["4x6-c65"].C % EC.WAVE == 1 and 2 * (EC.pool_out(6) - 1) + 2 < 5
    assert {p.name for p in EC.POOL_CASES if (p.N, p.H, p.W, p.C) == (1, 3, 3, 1)} >= {"3x3-nan-first", "3x3-nan-middle", "3x3-nan-last",
                                                                                      "3x3-all-neg-inf", "3x3-inf"}


@pytest.mark.parametrize("case", EC.POOL_CASES, ids=lambda c: c.name)
def test_pool_plants_show_in_the_reference_exactly_where_a_window_holds_them(case):
    """the NaN mask of F.max_pool2d, restated from the plants alone: output (n, oy, ox, c) is NaN iff a planted NaN lies in
    rows 2 oy .. 2 oy + 2 and columns 2 ox .. 2 ox + 2 of that image and channel"""
    x = EC.pool_input(case.name)
    ref = EC.pool_reference(x)
    Ho, Wo = EC.pool_out(case.H), EC.pool_out(case.W)
    assert ref.shape == (case.N, Ho, Wo, case.C)
    assert int((x == 0).sum()) == 0, "no zeros of either sign"
    want = torch.zeros_like(ref, dtype=torch.bool)
    for n, y, xx, ch, v in case.plants:
        if v == v:
            continue
        for oy in range(Ho):
            for ox in range(Wo):
                if 2 * oy <= y <= 2 * oy + 2 and 2 * ox <= xx <= 2 * ox + 2:
                    want[n, oy, ox, ch] = True
    assert torch.equal(torch.isnan(ref), want)
    kinds = {("nan" if v != v else v) for *_, v in case.plants}
    if case.name.startswith(("cap", "4x6")):
        assert "nan" in kinds and int(want.sum()) >= 3
    if case.name.startswith("cap"):
        assert {"nan", EC.INF, -EC.INF} <= kinds
        assert int((ref == -EC.INF).sum()) == 1 and int((ref == EC.INF).sum()) >= 1
        pos = {(y - 2 * min(y // 2, Ho - 1), xx - 2 * min(xx // 2, Wo - 1)) for n, y, xx, ch, v in case.plants if v != v and y < 2 * Ho + 1}
        assert {(0, 0), (1, 1), (2, 2)} <= pos, pos                              # first, middle and last element of a window
    if case.name == "3x3-all-neg-inf":
        assert float(ref) == -EC.INF


# ---- convolution ------------------------------------------------------------------------------------------------------

def test_conv_cases_reach_their_edges():
    c = {q.name: q for q in EC.CONV_CASES}
    dims = {k: EC.conv_dims(v) for k, v in c.items()}
    K = {k: d[3] for k, d in dims.items()}
    Mtot = {k: d[2] for k, d in dims.items()}
    KS, T = EC.KS, EC.T
    # the reduction: below one step, exactly one, a tail of one, exactly two, a tail inside the second
    assert (K["k9"], K["k16"], K["k17"], K["k32"], K["k27"]) == (9, KS, KS + 1, 2 * KS, 27)
    assert K["k9"] < KS and KS < K["k27"] < 2 * KS
    assert {K[k] % KS for k in c} >= {0, 1, 9 % KS, 27 % KS, 363 % KS}
    for k in ("k9", "k16", "k17", "k32", "k27"):
        assert (c[k].N, c[k].H, c[k].W) == (2, 5, 7) and Mtot[k] == 70 and T < Mtot[k] < 2 * T
    assert {q.Co for q in EC.CONV_CASES} == {EC.TN, 2 * EC.TN}
    # geometry
    g = c["corner-one-tap"]
    assert (g.ks, g.stride, g.pad, g.H, g.W) == (7, 3, 6, 4, 5) and g.pad == g.ks - 1
    for o in (0, dims["corner-one-tap"][0] - 1):                                 # first and last output row: one live tap row
        assert len([k for k in range(g.ks) if 0 <= o * g.stride - g.pad + k < g.H]) == 1
    assert [k for k in range(g.ks) if 0 <= k - g.pad < g.W] == [g.ks - 1]       # first output column: one live tap column,
    # so the windows of the two left corners hold one live tap each, the last of their row of taps
    for name, unread_col in (("stride2-8x9", False), ("stride2-8x10", True), ("nonfinite-unread", True)):
        s = c[name]
        Ho, Wo = dims[name][:2]
        assert (s.ks, s.stride, s.pad) == (3, 2, 0) and (Ho - 1) * s.stride + s.ks - 1 < s.H - 1
        assert ((Wo - 1) * s.stride + s.ks - 1 < s.W - 1) == unread_col
    one = c["conv1-33x34"]
    assert (one.ks, one.stride, one.pad) == LC.GEOMETRY[0] and ((one.H + 4 - 11) % 4, (one.W + 4 - 11) % 4) == (2, 3) and K["conv1-33x34"] == 363
    two = c["conv2-1x1"]
    assert (two.ks, two.stride, two.pad) == LC.GEOMETRY[1] and (two.H, two.W) == (1, 1) and K["conv2-1x1"] == 1600
    # row tiles
    r = c["rows-2T+1"]
    assert r.N == 3 and Mtot["rows-2T+1"] == 2 * T + 1 and (dims["rows-2T+1"][0] * dims["rows-2T+1"][1]) % T != 0
    assert dims["rows-T-per-image"][0] * dims["rows-T-per-image"][1] == T and Mtot["rows-T-per-image"] == 2 * T
    for q in EC.CONV_CASES:                                                      # every argument is a valid one
        assert q.Co % EC.TN == 0 and 0 <= q.pad < q.ks and q.H + 2 * q.pad >= q.ks and q.W + 2 * q.pad >= q.ks


def test_conv_nonfinite_cases_show_in_the_reference_as_the_case_says():
    c = {q.name: q for q in EC.CONV_CASES}
    for name in ("nonfinite-relu", "nonfinite-linear"):
        q = c[name]
        assert {(n, y, x, ch) for n, y, x, ch, _ in q.plants} == {(0, 0, 0, 0), (q.N - 1, q.H - 1, q.W - 1, q.Ci - 1)}
        ref, bound = EC.conv_reference(name)
        nan = torch.isnan(ref)
        assert nan[q.N - 1, -2:, -2:].all() and int(nan.sum()) == 4 * q.Co       # the 3 x 3 windows that hold the last pixel
        assert not nan[0].any() and torch.isinf(ref[0, :2, :2]).any()
        hard = torch.isnan(bound)
        assert int(hard.sum()) == 8 * q.Co and torch.isfinite(ref[~hard]).all() and (bound[~hard] > 0).all()
        if q.relu:
            assert ((ref[0, :2, :2] == 0) | (ref[0, :2, :2] == EC.INF)).all() and (ref[0, :2, :2] == 0).any()   # relu(-inf) = 0
        else:
            assert (ref[0, :2, :2] == -EC.INF).any() and (ref[0, :2, :2] == EC.INF).any()
    x1, w1, b1, _ = EC.conv_inputs("nonfinite-relu")
    x2, w2, b2, _ = EC.conv_inputs("nonfinite-linear")
    assert torch.equal(EC.bits(x1), EC.bits(x2)) and torch.equal(w1, w2) and torch.equal(b1, b2)     # the same call without the ReLU
    ref, bound = EC.conv_reference("nonfinite-unread")
    assert len(c["nonfinite-unread"].plants) == 3 and torch.isfinite(ref).all() and not torch.isnan(bound).any()
    linear = EC.conv_reference("nonfinite-linear")[0]
    assert float(linear[torch.isfinite(linear)].min()) < 0.0


# ---- head -------------------------------------------------------------------------------------------------------------

def test_head_cases_reach_their_edges():
    c = {q.name: q for q in EC.HEAD_CASES}
    W, HP = EC.WAVE, EC.HP
    assert [c[k].C for k in ("c1", "c63", "c65", "c130")] == [1, W - 1, W + 1, 2 * W + 2] and all(c[k].P == 5 for k in ("c1", "c63", "c65", "c130"))
    assert sorted(q.P for q in EC.HEAD_CASES if q.C == W + 1 and q.B == 2) == [3, 4, 5, HP - 1, HP, HP + 1, 2 * HP + 1]
    assert all(q.C % W for q in EC.HEAD_CASES)                                   # every case has a partial trip over the channels
    assert (c["b-max"].B, c["b-max"].P, c["b-max"].C) == (L.METRICS_MAX_IMAGES, 5, W + 1)
    groups = lambda P: -(-P // HP)
    assert [groups(P) for P in (HP - 1, HP, HP + 1, 2 * HP + 1)] == [1, 1, 2, 3]
    assert {q.P % EC.HEAD_WAVES for q in EC.HEAD_CASES} == {0, 1, 3}             # waves with unequal pixel counts
    big, over, tiny = np.float32(EC.BIG), np.float32(EC.OVERFLOWING), np.float32(EC.TINY)
    with np.errstate(over="ignore", under="ignore"):
        assert np.isinf(over * over) and np.isfinite(big * big) and np.isfinite(np.float32(130) * big * big)
        assert float(tiny) ** 2 * 130 < M.LPIPS_NORM_EPS * EC.U64 and tiny * tiny < np.finfo(np.float32).tiny
    for q in EC.HEAD_CASES:
        feats, lin = EC.head_inputs(q.name)
        assert feats.shape == (2 * q.B, q.P, q.C) and float(feats.min()) >= 0.0 and float(lin.min()) >= 0.0
        last = q.B - 1
        assert not feats[0, 0].any() and not feats[q.B, 0].any()                 # both stacks zero
        assert not feats[q.B, 1].any() and not feats[last, q.P - 1].any()        # one stack zero, either side
        if q.C > 1:
            assert feats[0, 1].any() and feats[q.B + last, q.P - 1].any()
        assert float(feats[last, 0].min()) >= np.float32(EC.BIG) and float(feats[q.B + last, 0].min()) >= np.float32(EC.OVERFLOWING)
        assert 0 < float(feats[last, 1].max()) <= 2 * EC.TINY and 0 < float(feats[q.B + last, 1].max()) <= 2 * EC.TINY
        want, bound = EC.head_reference(q.name)
        assert np.all(np.isfinite(want.astype(np.float64))) and np.all(want > 0) and np.all(bound < 1e-9 * want)


# ---- the twins ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", sorted(set(EC.MUTATIONS.values())))
def test_the_twin_of_each_kernel_stays_inside_every_bound(family):
    assert EC.twin_failures(family) == []


def test_twin_error_over_bound_is_printed():
    worst = max(EC.conv_check(EC.conv_twin(q.name), *EC.conv_reference(q.name))[1] for q in EC.CONV_CASES)
    head = max(EC.head_inside(EC.head_twin(q.name), q.name)[1] for q in EC.HEAD_CASES)
    print(f"twins: conv worst err / bound {worst:.3f}, head {head:.3e}")
    assert 0 < worst <= 1 and head <= 1


EXPECTED_TO_FAIL = {
    "conv_last_partial_step_dropped": lambda: {"k9", "k17", "k27", "conv1-33x34", "corner-one-tap"},
    "conv_prefetch_guard_one_step_late": lambda: {"k17", "k32", "k27", "conv1-33x34"},
    "conv_image_from_tile_first_row": lambda: {"rows-2T+1", "k17", "nonfinite-relu"},
    "conv_tap_clamped_to_edge": lambda: {"corner-one-tap", "conv1-33x34", "conv2-1x1", "k27"},
    "pack_later_sweeps_dropped": lambda: {"cap-plus", "three-trips"},
    "pack_later_counts_dropped": lambda: {"cap-plus", "three-trips"},
    "pool_nan_rule_removed": lambda: {"3x3-nan-middle", "3x3-nan-last", "4x6-c65", "cap-square", "cap-h-plus-1"},
    "head_channel_tail_dropped": lambda: {q.name for q in EC.HEAD_CASES},
    "head_eps_omitted": lambda: {q.name for q in EC.HEAD_CASES},
    "head_norms_in_float32": lambda: {q.name for q in EC.HEAD_CASES},
}


@pytest.mark.parametrize("mut", list(EC.MUTATIONS))
def test_each_planted_defect_of_a_twin_misses_a_case(mut):
    failed = set(EC.twin_failures(EC.MUTATIONS[mut], mut))
    print(f"MUTATION {mut}: fails {sorted(failed)}")
    assert failed and EXPECTED_TO_FAIL[mut]() <= failed
    if mut.startswith("pack"):
        assert failed == {"cap-plus", "three-trips"}                            # a single trip cannot show it
    if mut == "conv_last_partial_step_dropped":                                  # a K on the step cannot show it
        assert failed <= {q.name for q in EC.CONV_CASES if EC.conv_dims(q)[3] % EC.KS}
    if mut == "conv_prefetch_guard_one_step_late":                               # nor can a single step this one
        assert failed <= {q.name for q in EC.CONV_CASES if EC.conv_dims(q)[3] > EC.KS}
    if mut == "pool_nan_rule_removed":
        assert "3x3-nan-first" not in failed                                     # m = p[0] carries a NaN in the first element


def test_mutations_cover_the_issue_list():
    assert set(EXPECTED_TO_FAIL) == set(EC.MUTATIONS)
    assert sorted(set(EC.MUTATIONS.values())) == ["conv", "head", "pack", "pool"]


# ---- the whole metric --------------------------------------------------------------------------------------------------

def test_e2e_cases_pass_the_caps_they_are_named_for():
    (h0, w0, b0), (h1, w1, b1), (h2, w2, b2) = EC.E2E_CASES
    assert (h0, w0) == (L.LPIPS_MIN_SIDE,) * 2 and b0 == L.METRICS_MAX_IMAGES
    assert h1 == w1 and 3 * (h1 - 1) ** 2 <= EC.E < 3 * h1 * h1 and (h1, b1) == (592, 3)
    s = EC.e2e_launch_sizes(h1, w1, b1)
    assert s["pack"] > EC.E and s["pool1"] > EC.E and s["pool2"] > EC.E and s["head1_groups"] > EC.WAVE
    assert M.lpips_map_sizes(h1, w1)[:3] == [(147, 147), (73, 73), (36, 36)]
    assert h2 != w2 and 0 < 3 * h2 * w2 - EC.E <= 3 * h2 and EC.ew_trips(3 * h2 * w2) == 2
    for H, W, B in EC.E2E_CASES:
        assert 6 * B * H * W < 2 ** 31 and min(H, W) >= L.LPIPS_MIN_SIDE


def test_layer_values_are_the_host_definition_with_its_terms_kept_apart():
    pred, target = LC.image_pair(35, 33, 3)
    for dtype in (torch.float32, torch.float64):
        layers, total = EC.layer_values(pred, target, dtype)
        assert layers.shape == (3, M.LPIPS_LAYERS)
        assert torch.equal(total, M.lpips_per_image(pred, target, LC.weights(), dtype).double())
        assert float((layers.sum(dim=1) - total).abs().max()) <= 1e-7 * float(total.max())
        assert float(layers.min()) > 0.0
