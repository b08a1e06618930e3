"""The hand-placed resampler cases of tests/pdf_cases.py, checked without a GPU.  The fp32 CPU chain (the oracle's operations
in float32) goes through the very checks tests/test_gpu_pdf_edges.py applies to the kernel -- every weight and bin within its
bound, the exact family bit for bit, the depth rule -- which proves that the inputs keep the float64 reference within every
condition by themselves; the reference agrees with the oracle at the production shapes; EPS_CDF has its measured basis; and
the kernel's power-of-two descent, restated, is searchsorted on every case."""
import numpy as np
import pytest
import torch

import pdf_cases as PC
from oracle import nerf_oracle as O


@pytest.mark.parametrize("key", list(PC.ALL))
def test_case_builds_and_fp32_chain_passes_every_check(key):
    c = PC.ALL[key]()
    got = PC.chain32(c.dens, c.sb_rows, c.u, c.near, c.far, c.spacing, c.pad, c.eps)
    rw, rb = PC.hold(c, got.weights, got.new, got.depth)
    print(f"{key}: EPL {c.epl} nb {c.nb} ties {int(c.tie.sum())} fp32 chain error / bound: weights {rw:.3f} bins {rb:.3f}")
    assert torch.all(got.new[:, 1:] >= got.new[:, :-1]) or c.family == "exact"


def test_cases_cover_the_kernel_edges():
    PC.check_coverage()


def test_bounds_rest_on_the_measured_fp32_chain():
    wr, ce = PC.measure_chain32()
    print(f"fp32 chain vs float64 over the toleranced cases: weights error / bound {wr:.3f}, worst |dcdf| {ce:.3e}")
    assert PC.EPS_CDF >= 4 * ce and PC.CDF_WORST_MEASURED >= ce
    assert PC.EPS_CDF <= 4.2 * PC.CDF_WORST_MEASURED, "EPS_CDF is 4 x the measured worst, rounded up"
    assert wr <= PC.WEIGHT_RATIO_MEASURED < 1


@pytest.mark.parametrize("n,m", [(256, 96), (96, 48)])
def test_reference_agrees_with_the_oracle_at_production_shapes(n, m):
    g = torch.Generator().manual_seed(n + m)
    R = 203
    dens = torch.exp(torch.randn(R, n, generator=g) * 2.5)
    dens[0], dens[2] = 0.0, 1e4
    dens[1, : n // 2] = 0.0
    dens[3, 5] = float("inf")
    sb = torch.sort(torch.rand(R, n + 1, generator=g), dim=-1).values
    sb[4] = O.initial_spacing_bins(n)
    eb = O.spacing_to_euclidean(sb, PC.NEAR, PC.FAR)
    w = O.get_weights(dens, eb[:, 1:] - eb[:, :-1])
    new = O.pdf_resample(w, sb, m)
    depth = O.render_depth_median(w, (eb[:, :-1] + eb[:, 1:]) / 2)
    u = O.pdf_u(m)
    got = PC.chain32(dens, sb, u)
    assert torch.equal(got.weights, w) and torch.equal(got.new, new) and torch.equal(got.depth, depth), \
        "chain32 is the oracle's own operation sequence"
    ref = PC.reference(dens, sb, u)
    wb = PC.weight_bound(ref)
    bb, K = PC.bin_bound(ref, sb, u)
    assert torch.isfinite(K).all()
    assert ((w.double() - ref.weights).abs() <= wb).all() and ((new.double() - ref.new).abs() <= bb).all()
    tie = PC.ties(ref, wb)
    assert tie.sum() <= PC.MAX_TIES * R
    mids = ref.steps32.double()
    hit = lambda k: (depth.double() - torch.gather(mids, -1, torch.clamp(k, 0, n - 1)[:, None])).abs()[:, 0] <= 1e-5 * depth[:, 0].abs()
    assert (hit(ref.idx) | (tie & (hit(ref.idx - 1) | hit(ref.idx + 1)))).all()


@pytest.mark.parametrize("key", list(PC.ALL))
def test_power_of_two_descent_is_searchsorted(key):
    c = PC.ALL[key]()
    got = PC.chain32(c.dens, c.sb_rows, c.u, c.near, c.far, c.spacing, c.pad, c.eps)
    pos = PC.descent(got.cdf.numpy(), c.u.numpy())
    inds = torch.searchsorted(got.cdf, c.u.expand(c.dens.shape[0], -1).contiguous(), side="right").numpy()
    assert np.array_equal(pos + 1, inds)
    assert np.array_equal(np.clip(pos, 0, c.n), got.below.numpy()) and np.array_equal(np.clip(pos + 1, 0, c.n), got.above.numpy())


def test_oracle_takes_one_sample_per_ray():
    dens, sb = torch.tensor([[0.0], [3.0], [float("inf")]]), torch.tensor([[0.0, 1.0], [0.25, 0.5], [0.1, 0.9]])
    eb = O.spacing_to_euclidean(sb, PC.NEAR, PC.FAR)
    delta = eb[:, 1:] - eb[:, :-1]
    w = O.get_weights(dens, delta)
    assert w.shape == (3, 1) and torch.equal(w, 1 - torch.exp(-delta * dens))
    new = O.pdf_resample(w, sb, 4)
    assert new.shape == (3, 5) and torch.all(new[:, 1:] >= new[:, :-1])
    assert torch.all(new >= sb[:, :1]) and torch.all(new <= sb[:, 1:])
    got = PC.chain32(dens, sb, O.pdf_u(4))
    assert torch.equal(got.weights, w) and torch.equal(got.new, new)
