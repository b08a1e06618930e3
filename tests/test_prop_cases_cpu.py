"""The hand-placed proposal-density cases of tests/prop_cases.py, checked without a GPU.  The fp32 CPU chain (the kernel's
operations restated in numpy float32, a correctly rounded exp) goes through the very `hold` tests/test_gpu_prop_edges.py
applies to the kernels; the cases cover every edge the module lists; FACTOR has its measured basis; the reference agrees with
the fp32 oracle at the production shapes; and each mutation of the fp32 chain fails `hold`, so the bounds are tight enough to
see a kernel that is wrong in that way."""
import numpy as np
import pytest
import torch

import prop_cases as PC
from oracle import nerf_oracle as O


@pytest.mark.parametrize("key", list(PC.CASES))
def test_case_builds_and_fp32_chain_passes_hold(key):
    c = PC.case(key)
    ratio = PC.hold(c, PC.run_chain32(c))
    print(f"{key}: net {c.net.name} live {int(c.sel.sum())} of {c.sel.size} fp32 chain error / bound {ratio:.3f}")
    assert np.isfinite(c.origins).all() and np.isfinite(c.dirs).all() and np.isfinite(c.bound).all()
    assert (c.bound[c.sel] > 0).all() and (c.ref.dens[~c.sel] == 0).all()


def test_cases_cover_the_kernel_edges():
    PC.check_coverage()


def test_bounds_rest_on_the_measured_fp32_chain():
    worst = PC.measure_chain32()
    print(f"fp32 chain vs float64 over all cases: worst error / unscaled bound {worst:.4f}")
    assert PC.RATIO_MEASURED >= worst and PC.FACTOR >= 4 * worst
    assert PC.FACTOR <= 4.1 * PC.RATIO_MEASURED, "FACTOR is 4 x the measured worst, rounded up"


@pytest.mark.parametrize("n,shared", [(256, True), (96, False)])
@pytest.mark.parametrize("name", ["t5h16-hashed", "t8h16-box-dense8", "c5h16-f32", "c8h64-f16"])
def test_reference_agrees_with_the_oracle_at_production_shapes(name, n, shared):
    nt = PC.net(name)
    rng = np.random.default_rng(n)
    R = 24
    lo, hi = (-1.2, 1.2) if nt.aabb is None else (0.05, 0.95)
    o = rng.uniform(lo, hi, (R, 3)).astype(np.float32)
    d = rng.standard_normal((R, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    sb = O.initial_spacing_bins(n)[None].expand(R, -1) if shared else \
        torch.from_numpy(np.sort(rng.uniform(0, 1, (R, n + 1)), axis=1).astype(np.float32))
    near, far = PC.NF_LONG if nt.aabb is None else PC.NF_SHORT
    pos = O.sample_positions(torch.from_numpy(o), torch.from_numpy(d), O.spacing_to_euclidean(sb, near, far))
    g = PC.grid_mlp(nt)
    p_or, sel_or = O.normalized_positions(pos, g.aabb)
    P32, sel = PC.positions32(o, d, sb.numpy(), n, near, far, 0, nt.aabb)
    assert np.array_equal(p_or.numpy(), P32) and np.array_equal(sel_or.numpy(), sel), "positions32 is the oracle's sequence"
    ref = PC.reference(nt, P32, sel)
    got = O.density_field(pos, g, PC.AVG).numpy()
    assert (got[~sel] == 0).all() and sel.any()
    err = np.abs(got.astype(np.float64) - ref.dens)
    assert (err <= PC.FACTOR * ref.rel * ref.dens).all(), (err[sel] / (PC.FACTOR * ref.rel * ref.dens)[sel]).max()
    c32 = PC.chain32(nt, o, d, sb.numpy(), n, near, far, 0)
    assert (np.abs(c32.astype(np.float64) - ref.dens) <= PC.FACTOR * ref.rel * ref.dens).all()


@pytest.mark.parametrize("mut", list(PC.MUTATIONS))
def test_mutated_fp32_chain_fails_hold(mut):
    failed = []
    for key in PC.CASES:
        c = PC.case(key)
        if not PC.MUTATIONS[mut](c):
            continue
        try:
            PC.hold(c, PC.run_chain32(c, mut))
        except AssertionError:
            failed.append(key)
    print(f"{mut}: fails hold on {len(failed)} cases, first {failed[:4]}")
    assert failed, f"the chain with '{mut}' passes every case: the bounds would let such a kernel through"


def test_floor_plus_one_is_ceil_where_it_matters():
    """On an exact integer coordinate the kernel's ceil corner (floor + 1) is another row than the reference's (ceil = floor),
    weighted by exactly 0: the planted nodes and faces give the same feature either way."""
    for key in ("a-n4-own", "c-n2-own", "e-n8-own"):
        c = PC.case(key)
        rows = [r for r, t in enumerate(c.tags) if t in ("origin", "node0") or t.startswith("face")]
        assert rows
        got = PC.run_chain32(c)[rows]
        err = np.abs(got.astype(np.float64) - c.ref.dens[rows])
        assert (err <= c.bound[rows]).all() and c.sel[rows].all()
