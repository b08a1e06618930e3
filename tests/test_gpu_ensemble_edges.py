"""The fused ensemble reduce on the GPU against float64, at its block, group, unroll and channel-walk edges
(unerf_ensemble_reduce through the C ABI on the guarded arena of test_gpu_ensemble_batch._reduce, and through
ops.ensemble_reduce / ensemble.aggregate_batch).  Cases, the float64 reference and the derived bounds are in
tests/ensemble_edge_cases.py; test_ensemble_edge_cases_cpu.py shows on the CPU that the bounds hold for the kernel's order of
operations and that the cases catch wrong ones.  No element is left out of a comparison.

Measured on an MI355X, worst error / bound over all cases: mean 0.52, var 0.08, var_cmean 0.06, alea_cmean 0.31,
epi_plus_alea 0.25, sqrt_epi_plus_alea 0.35, std_cmean 0.07 -- the CPU restatement's figures to the printed digit, case by
case; the exact family, repeat runs, the side stream, ops.ensemble_reduce and unerf_moments all bit-equal."""
import pytest
import torch

import ensemble_edge_cases as EC
from test_gpu_ensemble_batch import ALEA_ORDER, FILL, _bits, _members, _reduce

pytestmark = pytest.mark.gpu


def _codes(lib):
    codes = {"mean": lib.ENS_MEAN, "var": lib.ENS_VAR, "var_cmean": lib.ENS_VAR_CMEAN, "alea_cmean": lib.ENS_ALEA_CMEAN,
             "epi_plus_alea": lib.ENS_EPI_ALEA, "sqrt_epi_plus_alea": lib.ENS_EPI_ALEA_SQRT, "std_cmean": lib.ENS_STD_CMEAN}
    assert [codes[s] for s in EC.STATS] == list(range(len(EC.STATS)))
    return codes


def _same_bits(a, b, what):
    assert len(a) == len(b)
    for v, (x, y) in enumerate(zip(a, b)):
        assert list(x) == list(y), (what, v)
        for name in x:
            assert x[name].shape == y[name].shape and torch.equal(_bits(x[name]), _bits(y[name])), (what, v, name)


def _four_runs(lib, dev, case):
    """the case through the C ABI twice, once on a side stream and once through ops.ensemble_reduce: the same bits four times
    -> (the device views, the first run's result)"""
    from uncertainty_nerf_gs_amd import ops
    vws = EC.views(case, dev)
    plan = EC.coded_plan(case.plan, _codes(lib))
    first = _reduce(lib, vws, plan)
    for res in first:
        for name, t in res.items():
            assert not bool((_bits(t) == FILL).any()), f"{case.name}: {name} holds elements nothing wrote"
    _same_bits(first, _reduce(lib, vws, plan), "second run")
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        side = _reduce(lib, vws, plan)
    torch.cuda.current_stream(dev).wait_stream(s)
    _same_bits(first, side, "side stream")
    through_ops = ops.ensemble_reduce(vws, case.plan)
    torch.cuda.synchronize()
    _same_bits(first, through_ops, "ops.ensemble_reduce")
    return vws, first


def _hold_case(case, got):
    ref, bnd = EC.reference(case.name)
    worst = {}
    for v in range(case.B):
        for s, r in EC.hold(case.name, ref[v], bnd[v], got[v], what=f" view {v}").items():
            worst[s] = max(worst.get(s, 0.0), r)
    print(f"{case.name}: worst error / bound " + ", ".join(f"{s} {worst[s]:.3f}" for s in EC.STATS if s in worst))
    return worst


def _moments_lock(case, vws, got):
    """the second lock: every key with a planned mean and variance against unerf_moments of the stacked sources, bit for bit"""
    from uncertainty_nerf_gs_amd import ops
    names = {(stat, k): name for name, stat, k in case.plan}
    locked = 0
    for k in case.keys:
        if ("mean", k) in names and ("var", k) in names:
            for v in range(case.B):
                mean, var = ops.moments(torch.stack(list(vws[v][k]), dim=0).contiguous())
                assert torch.equal(_bits(got[v][names["mean", k]]), _bits(mean)), (case.name, v, k, "mean")
                assert torch.equal(_bits(got[v][names["var", k]]), _bits(var)), (case.name, v, k, "var")
            locked += 1
    return locked


@pytest.mark.parametrize("name", EC.of_family("groups", "unroll", "walk", "limits", "aux", "values"))
def test_every_block_within_its_bound_of_float64(lib, dev, name):
    case = EC.CASES[name]
    vws, got = _four_runs(lib, dev, case)
    _hold_case(case, got)
    assert _moments_lock(case, vws, got) == sum(1 for k in case.keys if {f"{k}/mean", f"{k}/var"} <= set(got[0]))


@pytest.mark.parametrize("name", EC.of_family("exact"))
def test_identical_members_are_exact(lib, dev, name):
    """mean == x, every variance and epistemic term +0, epi_plus_alea == alea_cmean, sqrt_epi_plus_alea == sqrtf(alea), no NaN"""
    case = EC.CASES[name]
    vws, got = _four_runs(lib, dev, case)
    want = EC.exact_expected(case)
    stat = EC.stat_of(case)
    for v in range(case.B):
        for out, w in want[v].items():
            g = got[v][out].cpu()
            bad = torch.nonzero(_bits(g) != _bits(w))
            assert len(bad) == 0, (f"{name} view {v} {out}: differs from the exact values at {bad[:8].tolist()}: "
                                   f"{[g[tuple(i)].item() for i in bad[:8].tolist()]}")
            assert not bool(g.isnan().any())
            if stat[out] in ("var", "var_cmean", "std_cmean"):
                assert bool((_bits(g) == 0).all()), (name, out, "not +0")
    _hold_case(case, got)
    _moments_lock(case, vws, got)


def test_a_nan_and_an_inf_in_one_member_stay_where_torch_puts_them(lib, dev):
    case = EC.CASES["nonfinite"]
    vws, got = _four_runs(lib, dev, case)
    cpu = EC.views(case)[0]
    hit = 0
    for k in ("long", "c3", "c3_var"):
        x = torch.stack(list(cpu[k]))
        for stat, t in (("mean", x.mean(0)), ("var", x.var(0))):
            if f"{k}/{stat}" in got[0]:
                g = got[0][f"{k}/{stat}"].cpu()
                assert torch.equal(g.isnan(), t.isnan()) and torch.equal(g.isinf(), t.isinf()), (k, stat)
                assert bool((g[t.isinf()] == t[t.isinf()]).all())
                hit += int((~t.isfinite()).sum())
    # every planted element shows once in its mean and once in its variance (c3_var: only the mean is planned)
    assert hit == sum(1 if k == "c3_var" else 2 for _, k, *_ in case.planted) == 16
    long_mean = got[0]["long/mean"].cpu()[:, 0]
    assert bool(long_mean[0].isnan()) and bool(long_mean[2048].isnan()) and bool(long_mean[255].isinf()) and bool(long_mean[2047].isinf())
    assert int((~long_mean.isfinite()).sum()) == 4
    alea = got[0]["c3/alea_cmean"].cpu()[:, 0]
    assert bool(alea[3].isnan()) and bool(alea[7].isinf()) and int((~alea.isfinite()).sum()) == 2
    _hold_case(case, got)                            # every other element within its bound, the planted ones the same non-finite


def test_one_member_has_no_variance(lib, dev):
    case = EC.CASES["single-member"]
    vws, got = _four_runs(lib, dev, case)
    for v in range(case.B):
        for out, stat in EC.stat_of(case).items():
            g = got[v][out]
            if stat in ("mean", "alea_cmean"):
                assert bool(g.isfinite().all()), (out, stat)
            else:
                assert bool(g.isnan().all()), (out, stat)
        assert torch.equal(_bits(got[v]["a/mean"]), _bits(vws[v]["a"][0])) and torch.equal(_bits(got[v]["d/mean"]), _bits(vws[v]["d"][0]))
    _hold_case(case, got)
    _moments_lock(case, vws, got)


@pytest.mark.parametrize("name", [n for n in EC.of_family("groups") if "mixed" in n])
def test_a_view_of_a_batch_equals_that_view_alone(lib, dev, name):
    """row v of the B = 3 launch of the mixed-n key set against a B = 1 launch of view v: the same bits"""
    case = EC.CASES[name]
    vws = EC.views(case, dev)
    plan = EC.coded_plan(case.plan, _codes(lib))
    batch = _reduce(lib, vws, plan)
    for v in range(case.B):
        _same_bits([batch[v]], _reduce(lib, [vws[v]], plan, gap=3, tail=7), f"view {v} alone")


def test_aggregate_batch_of_seventeen_views_makes_two_launches(lib, dev):
    """17 views of the 9 x 31 alea-order member set: launches of 16 views and of 1.  Element v equals ensemble.aggregate of
    that view -- member means bit for bit, the derived keys within their bounds of reference64 from the inputs"""
    from uncertainty_nerf_gs_amd import ensemble, ops
    M, B, Hh, Ww = 5, 17, 9, 31
    per_view = [_members(dev, ALEA_ORDER, M, Hh, Ww, seed=70 + v) for v in range(B)]
    ops.TIMER = ops.KernelTimer()
    try:
        got = ensemble.aggregate_batch([[per_view[v][j] for v in range(B)] for j in range(M)])
        launches = {k: s["launches"] for k, s in ops.TIMER.summary().items()}
    finally:
        ops.TIMER = None
    torch.cuda.synchronize()
    assert launches.get("ensemble_reduce") == 2 and "moments" not in launches, launches
    assert len(got) == B
    plan = ensemble.reduce_plan(ALEA_ORDER)
    worst = {}
    for v in range(B):
        want = ensemble.aggregate(per_view[v])
        assert list(got[v]) == list(want) == [n for n, _, _ in plan]
        cpu = [{k: [m[k].reshape(-1, m[k].shape[-1]).cpu() for m in per_view[v]] for k in ALEA_ORDER}]
        ref, bnd = EC._reference_and_bounds(cpu, plan)
        flat = {}
        for name, stat, _ in plan:
            assert got[v][name].shape == want[name].shape == (Hh, Ww, got[v][name].shape[-1])
            if stat == "mean":
                assert torch.equal(_bits(got[v][name]), _bits(want[name])), (v, name)
            flat[name] = got[v][name].reshape(Hh * Ww, -1)
        for name, r in EC.ratios(ref[0], bnd[0], {k: t.cpu() for k, t in flat.items()}).items():
            s = dict((n, st) for n, st, _ in plan)[name]
            worst[s] = max(worst.get(s, 0.0), r)
        EC.hold("aggregate_batch", ref[0], bnd[0], flat, what=f" view {v}")
    print("aggregate_batch, 17 views: worst error / bound " + ", ".join(f"{s} {r:.3f}" for s, r in worst.items()))
