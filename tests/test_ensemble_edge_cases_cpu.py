"""CPU checks of tests/ensemble_edge_cases.py: the fp32 restatement of the ensemble reduce stays within the derived bounds of the
float64 reference on every case, planted wrong restatements miss them on the cases named here, and the "groups" cases
separate the mutants of the block dealing.  Evidence that the bounds hold for a correct kernel and bite on a wrong one, and
that the shapes are large enough and no larger than needed; the kernel itself is held in test_gpu_ensemble_edges.py."""
import numpy as np
import pytest
import torch

import ensemble_edge_cases as EC
from ensemble_cases import torch_reduce


@pytest.fixture(scope="module")
def restated():
    """restate32 of every case, once"""
    return {name: EC.restate32(EC.views(c), c.plan) for name, c in EC.CASES.items()}


def _case_ratios(name, got):
    c = EC.CASES[name]
    ref, bnd = EC.reference(name)
    worst = {}
    for v in range(c.B):
        for s, r in EC.worst_by_stat(c, EC.ratios(ref[v], bnd[v], got[v])).items():
            worst[s] = max(worst.get(s, 0.0), r)
    return worst


def test_the_case_table_covers_what_it_claims():
    fam = lambda f: [EC.CASES[n] for n in EC.of_family(f)]
    assert sorted(c.keys["x"].n for c in fam("groups") if "x" in c.keys) == list(EC.N_GROUPS)
    mixed = [c for c in fam("groups") if "x" not in c.keys]
    assert len(mixed) == 3 and all(c.B == 3 for c in mixed)
    for c in mixed:
        ns, n_keys = EC.used_ns(c)
        assert sorted(ns) == [1, 300, 300, 2049, 4097] and n_keys == 7
        names = list(c.keys)
        used = {k for _, _, k in c.plan}
        i = names.index("skip")                      # nothing is asked of it, and it lies between two used keys
        assert "skip" not in used and c.keys["skip"].n == 2049 and names[i - 1] in used and names[i + 1] in used
        assert "mid_var" not in used                 # reached only as an aux key, at g = 1
    assert [list(c.keys)[0] for c in mixed if "first" in c.name] == ["long"]
    assert [list(c.keys)[-1] for c in mixed if "last" in c.name] == ["long"]
    assert sorted(c.M for c in fam("unroll")) == list(EC.M_UNROLL)
    assert all(sorted(k.C for k in c.keys.values()) == [1, 3, 4] and c.keys["c1"].n == 257 for c in fam("unroll"))
    assert sorted(c.keys["x"].C for c in fam("walk")) == list(EC.C_WALK)
    assert all({"var_cmean", "std_cmean"} <= set(EC.stat_of(c).values()) and c.M == 5 for c in fam("walk"))
    lim = {c.name: c for c in fam("limits")}
    assert len(lim["limit-keys32"].keys) == EC.MAX_KEYS == len(EC.used_ns(lim["limit-keys32"])[0])
    assert lim["limit-M64-C64"].M == 64 and lim["limit-M64-C64"].keys["x"].C == 64 and lim["limit-B16"].B == 16
    aux = {c.name: c for c in fam("aux")}
    assert [aux[f"aux-c{w}"].keys["a_var"].C for w in (1, 3, 4)] == [1, 3, 4] and all(c.keys["a"].C == 3 for c in aux.values())
    a, b = aux["aux-slice-of-8"].keys, aux["aux-key-slice-of-8"].keys
    assert (a["a"].W, a["a_var"].W, b["a"].W, b["a_var"].W) == (3, 8, 8, 3)
    assert "a_var" not in {k for _, _, k in aux["aux-unasked"].plan}
    assert set(EC.stat_of(aux["aux-alea-only"]).values()) == {"alea_cmean"}
    assert sorted(c.M for c in fam("exact")) == list(EC.M_EXACT)
    planted = {(k, p) for _, k, _, p, _, _ in EC.CASES["nonfinite"].planted}
    assert {("long", 0), ("long", 255), ("long", 2048), ("c3", 0), ("c3", 255)} <= planted
    assert EC.CASES["single-member"].M == 1
    assert EC.channel_groups(7) == [(0, 4), (4, 3)] and EC.channel_groups(6) == [(0, 4), (4, 1), (5, 1)]
    assert EC.channel_groups(3) == [(0, 3)] and EC.channel_groups(2) == [(0, 1), (1, 1)]
    # a few MB at the most per case
    for c in EC.CASES.values():
        assert sum(c.B * c.M * d.n * d.W * 4 for d in c.keys.values()) < 4 << 20, c.name


def test_reference64_agrees_with_the_torch_statement_of_the_plan():
    """reference64 against ensemble_cases.torch_reduce (the torch operations of ensemble.aggregate) on the float64 inputs: two
    statements of the same formulas, to float64 rounding"""
    for name in ("aux-c4", "aux-slice-of-8", "walk-C7", "groups-mixed-longest-mid"):
        c = EC.CASES[name]
        vws = EC.views(c)
        want = torch_reduce([{k: [t.double() for t in srcs] for k, srcs in vw.items()} for vw in vws], c.plan)
        ref, _ = EC.reference(name)
        for v in range(c.B):
            for out, r in ref[v].items():
                assert torch.allclose(r, want[v][out], rtol=1e-12, atol=0), (name, v, out)


def test_the_restatement_stays_within_the_bounds_on_every_case(restated):
    """error / bound of the numpy float32 restatement, per statistic, worst over the cases: above 1 the DERIVATION is wrong"""
    worst, at = {}, {}
    for name, c in EC.CASES.items():
        if c.identical:
            continue
        for s, r in _case_ratios(name, restated[name]).items():
            assert r <= 1.0, f"{name}: the fp32 restatement's {s} is {r:.3g} x its bound"
            if r >= worst.get(s, -1.0):
                worst[s], at[s] = r, name
    for s in EC.STATS:
        print(f"restate32 {s}: worst error / bound {worst[s]:.3f} ({at[s]})")
    assert set(worst) == set(EC.STATS)


def test_the_restatement_gives_the_exact_family_bit_for_bit(restated):
    for name in EC.of_family("exact"):
        c = EC.CASES[name]
        want = EC.exact_expected(c)
        for v in range(c.B):
            for out, w in want[v].items():
                got = restated[name][v][out]
                assert torch.equal(got.view(torch.int32), w.view(torch.int32)), (name, v, out)
                assert not bool(got.isnan().any())
                if EC.stat_of(c)[out] in ("var", "var_cmean", "std_cmean"):
                    assert bool((got.view(torch.int32) == 0).all()), (name, out, "not +0")


def test_nonfinite_placement_is_torchs(restated):
    """the planted NaN / inf: mean and variance are non-finite exactly where torch.stack(...).mean(0) / .var(0) are, in the
    reference and in the restatement; M = 1 leaves every variance statistic NaN"""
    c = EC.CASES["nonfinite"]
    ref, _ = EC.reference("nonfinite")
    vw = EC.views(c)[0]
    for k in ("long", "c3"):
        x = torch.stack(list(vw[k]))
        for stat, t in (("mean", x.mean(0)), ("var", x.var(0))):
            for got in (ref[0][f"{k}/{stat}"], restated["nonfinite"][0][f"{k}/{stat}"]):
                assert torch.equal(got.isnan(), t.isnan()) and torch.equal(got.isinf(), t.isinf()), (k, stat)
        assert 0 < int((~x.mean(0).isfinite()).sum()) <= 4
    s = EC.CASES["single-member"]
    for v in range(s.B):
        for out, stat in EC.stat_of(s).items():
            got = restated["single-member"][v][out]
            assert bool(got.isfinite().all() if stat in ("mean", "alea_cmean") else got.isnan().all()), (out, stat)


# the case each planted wrong restatement must miss its bounds on
MUTANT_FAILS = {"one_pass": "values-stack-M5", "restart_at_U": "unroll-M9", "skip_tail": "unroll-M9", "no_reset": "aux-c1",
                "reset_each_group": "walk-C5", "div3": "walk-C2", "aux_key_stride": "aux-slice-of-8"}


@pytest.mark.parametrize("mutant", EC.MUTANTS)
def test_a_planted_wrong_restatement_misses_the_bounds(mutant):
    name = MUTANT_FAILS[mutant]
    c = EC.CASES[name]
    worst = _case_ratios(name, EC.restate32(EC.views(c), c.plan, mutant=mutant))
    print(f"{mutant} on {name}: " + ", ".join(f"{s} {r:.3g}" for s, r in worst.items()))
    assert max(worst.values()) > 1.0, f"{mutant} passes {name}"
    failing = [n for n, cc in EC.CASES.items()
               if max(_case_ratios(n, EC.restate32(EC.views(cc), cc.plan, mutant=mutant)).values()) > 1.0]
    print(f"{mutant} fails {len(failing)} of {len(EC.CASES)} cases: {failing}")
    assert name in failing


def test_unroll_mutants_are_separated_by_the_member_counts():
    """restart_at_U and skip_tail per (M, width): a body is needed for the first, a tail for the second -- which is why the
    member counts straddle both unroll widths"""
    for M in EC.M_UNROLL:
        name = f"unroll-M{M}"
        c = EC.CASES[name]
        ref, bnd = EC.reference(name)
        for mutant, hit in (("restart_at_U", lambda U: M >= U), ("skip_tail", lambda U: M % U != 0)):
            r = EC.ratios(ref[0], bnd[0], EC.restate32(EC.views(c), c.plan, mutant=mutant)[0])
            for key, U in (("c1", 8), ("c3", 4), ("c4", 4)):
                stat = "var" if mutant == "restart_at_U" else "mean"
                assert (r[f"{key}/{stat}"] > 1.0) == hit(U), (mutant, M, key, r[f"{key}/{stat}"])


def test_the_documented_dealing_owns_every_element_once():
    for name in EC.of_family("groups", "limits", "unroll"):
        ns, _ = EC.used_ns(EC.CASES[name])
        assert all(bool((cnt == 1).all()) for cnt in EC.ownership(ns)), name
        assert EC.grid_blocks(ns) % (EC.XCDS * len(ns)) == 0


@pytest.mark.parametrize("mutant", ["drop_g", "n_keys", "slots7"])
def test_the_groups_cases_separate_the_dealing_mutants(mutant):
    """a mutant must leave some element of a "groups" case unowned or doubly owned (a block that goes to the wrong key shows as
    both).  n <= 2048 is one group: drop_g and slots7 pass it, and fail from element 2048 on; n_keys needs a launch with a
    key that is not in used[]."""
    broken = []
    for name in EC.of_family("groups"):
        ns, n_keys = EC.used_ns(EC.CASES[name])
        if any(bool((cnt != 1).any()) for cnt in EC.ownership(ns, mutant, n_keys)):
            broken.append(name)
    print(f"{mutant} breaks {broken}")
    mixed = [n for n in EC.of_family("groups") if "mixed" in n]
    if mutant == "n_keys":
        assert broken == mixed
    else:
        assert broken == ["groups-n2049", "groups-n4097"] + mixed
    if mutant == "drop_g":
        cnt = EC.ownership([2049], mutant)[0]
        assert cnt[2048] == 0 and bool((cnt[:2048] == 2).all())
