"""The lane-group cases of tests/pdf_group_cases.py, checked without a GPU: every case builds under pdf_cases' own tie rule
(none at R = 37), the fp32 CPU chain passes the very checks tests/test_gpu_pdf_groups.py applies to the kernel, the planted
medians sit on the lane borders of the group layout, and the shapes cover what the module says they cover."""
import pytest
import torch

import pdf_cases as PC
import pdf_group_cases as GC


@pytest.mark.parametrize("key", list(GC.ALL))
def test_case_builds_without_ties_and_fp32_chain_passes_every_check(key):
    c = GC.ALL[key]()
    assert int(c.tie.sum()) == 0, f"{key}: {int(c.tie.sum())} tie rays at the default seed"
    assert key not in PC.SEEDS and c.dens.shape[0] == GC.R == 37
    got = PC.chain32(c.dens, c.sb_rows, c.u, c.near, c.far, c.spacing, c.pad, c.eps)
    rw, rb = PC.hold(c, got.weights, got.new, got.depth)
    print(f"{key}: G {GC.lanes_per_ray(c.n)} EPL {GC.group_epl(c.n)} nb {c.m + 1} fp32 chain error / bound: weights {rw:.3f} bins {rb:.3f}")
    assert rw < 1 and rb < 1
    assert torch.all(got.new[:, 1:] >= got.new[:, :-1])


def test_cases_cover_the_group_edges():
    GC.check_coverage()


@pytest.mark.parametrize("n,m", GC.MEDIAN_SHAPES)
def test_planted_medians_straddle_lane_borders(n, m):
    c = GC.group_medians(n, m)
    epl, ks = GC.group_epl(n), list(c.planted.values())
    assert c.ref.idx[: len(ks)].tolist() == ks
    # the last element of lane 0's run and the first of lane 1's, and the same around the last lane that holds samples
    assert epl - 1 in ks and (epl in ks or epl >= n)
    last = (n - 1) // epl
    assert last * epl in ks and (last * epl - 1 in ks or last == 0) and n - 1 in ks
    assert 8 * epl - 1 in ks and (8 * epl in ks or 8 * epl >= n)
    if GC.lanes_per_ray(n) == 64:      # the DPP row border inside the wave
        assert 16 * epl - 1 in ks and 16 * epl in ks


@pytest.mark.parametrize("n,m", GC.MIXED_SHAPES)
def test_mixed_rays_put_every_kind_in_every_wave(n, m):
    c = GC.mixed(n, m)
    per_wave = 64 // GC.lanes_per_ray(n)
    for first in range(0, GC.R - per_wave + 1, per_wave):
        kinds = {GC.KINDS[r % 5] for r in range(first, first + per_wave)}
        assert len(kinds) == min(per_wave, 5) or per_wave < 2
    assert torch.isinf(c.dens).any() and torch.isnan(c.ref.dd).any()
