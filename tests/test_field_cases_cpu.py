"""The hand-placed field cases of tests/field_cases.py, checked without a GPU.  The float32 restatement of the positions and
SH inputs equals the oracle's bit for bit; the float64 reference meets O.active_field / O.mcdropout_field run in float64 (two
independently written statements of the network); the CPU chains of the three bound families (fp32 fma chains, split f16,
single f16) go through the very `hold` tests/test_gpu_field_edges.py applies to the kernels, and the recorded ratios are
re-measured; the cases cover every edge the module lists; and each mutation of a chain fails `hold`, so the bounds are tight
enough to see a kernel that is wrong in that way -- for the split form, the hi * lo product dropped in any one matrix layer."""
import numpy as np
import pytest
import torch

import field_cases as FC
import prop_cases as PC
from oracle import nerf_oracle as O


@pytest.mark.parametrize("key", list(FC.CASES))
def test_case_builds_and_cpu_chains_pass_hold(key):
    c = FC.case(key)
    ratios = {bf: FC.hold(c, bf, FC.chain(c, bf)) for bf in FC.bound_families(c)}
    print(f"{key}: net {c.net.name} tiles {c.tiles} live {int(c.sel.sum())} of {c.N} passes {c.B} CPU chain error / bound: "
          + " ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    for ref in c.ref.values():
        for b in list(ref.b_dens.values()) + list(ref.b_rgb.values()) + list(ref.b_beta.values()):
            assert np.isfinite(b).all() and (b > 0).all()
        assert (ref.dens[:, ~c.sel] == 0).all() and np.isfinite(ref.o).all() and np.isfinite(ref.c).all()


def test_cases_cover_the_kernel_edges():
    FC.check_coverage()


@pytest.mark.parametrize("bf", ["fp32", "f16x2", "f16"])
def test_bounds_rest_on_the_measured_cpu_chains(bf):
    worst = FC.measure_chain(bf)
    print(f"{bf} chain vs float64 over all cases: worst error / unscaled bound {worst:.4f}")
    assert FC.RATIO_MEASURED[bf] >= worst and FC.FACTOR[bf] >= 4 * worst
    assert FC.RATIO_MEASURED[bf] <= 1.02 * worst + 1e-3, "the recorded ratio is the re-measured one"
    assert FC.FACTOR[bf] <= 4.1 * FC.RATIO_MEASURED[bf], "FACTOR is 4 x the measured worst, rounded up"


@pytest.mark.parametrize("key", ["A-r33-s48", "A-r31-s7", "B-tbox", "B-c32", "B-c32box", "B-c16", "C-twide", "E-w9-offset", "H-counter-max"])
def test_float32_restatement_is_the_oracles_sequence(key):
    """positions, selector and SH inputs, bit for bit (Euclidean bins pass through the oracle's sample_positions as they are)"""
    c = FC.case(key)
    sb = torch.from_numpy(c.sb)
    eb = sb if c.bins == "euclid" else O.spacing_to_euclidean(sb, c.near, c.far, uniform=bool(c.lin))
    pos = O.sample_positions(torch.from_numpy(c.origins), torch.from_numpy(c.dirs), eb)
    fp = FC.field_params(c.net, c.mode)
    p_or, sel_or = O.normalized_positions(pos, fp.grid.aabb)
    assert np.array_equal(p_or.numpy().reshape(-1, 3), c.P32) and np.array_equal(sel_or.numpy().reshape(-1), c.sel)
    dn = (torch.from_numpy(c.dirs) + 1.0) / 2.0
    if c.net.sh_remap:
        dn = dn * 2.0 - 1.0
    assert np.array_equal(np.repeat(dn.numpy(), c.S, axis=0), c.shin)
    inputs = O._color_inputs(torch.from_numpy(c.dirs), c.S, torch.zeros(c.R, c.S, 15), fp.appearance, fp.sh_remap)
    assert np.array_equal(inputs[:, :16].numpy(), O.sh16(torch.from_numpy(c.shin)).numpy())


def _oracle64(nt, mode, P, dirs, keeps, p):
    """the oracle's field in float64 AT the float32 positions: a unit scene box and all-zero bins make the oracle's own
    position arithmetic exact (p = x), so that only the network is compared"""
    N = P.shape[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    fp = FC.field_params(nt, mode, torch.float64, aabb=(0.0, 0.0, 0.0, 1.0, 1.0, 1.0))
    o, d, eb = t(P), t(dirs), torch.zeros(N, 2, dtype=torch.float64)
    if mode == FC.ACTIVE:
        dens, rgb, beta = O.active_field(o, d, eb, fp)
        return dens.numpy()[:, 0], rgb.numpy()[:, 0], beta.numpy()[:, 0]
    k = lambda site, w=64: torch.from_numpy(keeps[site][:, :w]) if site in keeps else None
    dens, rgb = O.mcdropout_field(o, d, eb, fp, k(FC.TRUNK), k(FC.HEAD1), p, keep_head0=k(FC.HEAD0), keep_in=k(FC.HEADIN, 63))
    return dens.numpy()[:, 0], rgb.numpy()[:, 0], None


@pytest.mark.parametrize("mode,sites", [(FC.ACTIVE, 0), (FC.MCDROPOUT, 5), (FC.MCDROPOUT, 7), (FC.MCDROPOUT, 13), (FC.MCDROPOUT, 2)])
@pytest.mark.parametrize("name", [n for n in FC.NETS if FC.NETS[n][0] == "torch"])
def test_reference_meets_the_oracle_in_float64(name, mode, sites):
    nt = FC.net(name)
    rng = np.random.default_rng(len(name) + sites)
    N, p = 96, 0.5
    P = rng.uniform(0.01, 0.99, (N, 3)).astype(np.float32)
    dirs = rng.standard_normal((N, 3))
    dirs = (np.round(dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * 4096) / 4096).astype(np.float32)   # (d + 1) / 2 is exact
    keeps = {b: rng.uniform(0, 1, (1, N, 64)) >= p for b in (1, 2, 4, 8) if mode == FC.MCDROPOUT and sites & b}
    K = 1 if mode == FC.MCDROPOUT else 0
    ref = FC.reference(nt, mode, P, np.ones(N, bool), FC.sh_inputs32(dirs, nt.sh_remap), K, p, sites, keeps, rounded=False)
    dens, rgb, beta = _oracle64(nt, mode, P, dirs, {b: k[0] for b, k in keeps.items()}, float(np.float32(p)))
    close = lambda a, b: np.all(np.abs(a - b) <= 1e-12 * np.abs(b) + 1e-300)
    assert close(ref.dens[0], dens), np.abs(ref.dens[0] / dens - 1).max()
    assert np.abs(ref.rgb[0] - rgb).max() <= 1e-13
    if mode == FC.ACTIVE:
        assert close(ref.beta, beta) or np.abs(ref.beta - beta).max() <= FC.SOFTPLUS_JUMP     # torch's softplus switches to x at 20


@pytest.mark.parametrize("name", ["c32-plain", "c16-plain", "c16-box-wide"])
def test_reference_holds_the_fp32_oracle_on_the_tcnn_layouts(name):
    """the tcnn lookups of the oracle are fp32 (and half) statements: held to the reference under the fp32 bound"""
    c = FC.case({"c32-plain": "B-c32", "c16-plain": "B-c16", "c16-box-wide": "C-c16wide"}[name])
    sb = torch.from_numpy(c.sb)
    eb = O.spacing_to_euclidean(sb, c.near, c.far, uniform=bool(c.lin))
    dens, rgb, beta = O.active_field(torch.from_numpy(c.origins), torch.from_numpy(c.dirs), eb, FC.field_params(c.net, FC.ACTIVE))
    out = {"dens": dens.numpy().reshape(1, -1), "rgb": rgb.numpy().reshape(1, -1, 3), "beta": beta.numpy().reshape(-1)}
    print(f"{name}: fp32 oracle error / bound {FC.hold(c, 'fp32', out):.3f}")


@pytest.mark.parametrize("mut", list(FC.MUTATIONS))
def test_mutated_chain_fails_hold(mut):
    bf, applies = FC.MUTATIONS[mut]
    failed, tried = [], 0
    for key in FC.CASES:
        c = FC.case(key)
        if bf not in FC.bound_families(c) or not applies(c):
            continue
        tried += 1
        try:
            FC.hold(c, bf, FC.chain(c, bf, mut))
        except AssertionError:
            failed.append(key)
    print(f"{mut} ({bf} chain): fails hold on {len(failed)} of {tried} cases, first {failed[:4]}")
    assert failed, f"the {bf} chain with '{mut}' passes every case: the bounds would let such a kernel through"


def test_hold_rejects_sentinels_nan_and_unmasked_density():
    c = FC.case("B-tbox")
    good = FC.chain(c, "fp32")
    assert (~c.sel).any()
    for key, value in (("dens", np.array([FC.SENTINEL], np.uint32).view(np.float32)[0]), ("rgb", np.float32(np.nan))):
        out = {k: None if v is None else v.copy() for k, v in good.items()}
        out[key].reshape(-1)[int(np.argmax(c.sel)) * (3 if key == "rgb" else 1)] = value
        with pytest.raises(AssertionError):
            FC.hold(c, "fp32", out)
    out = {k: None if v is None else v.copy() for k, v in good.items()}
    out["dens"][0, int(np.argmin(c.sel))] = np.float32(1e-30)
    with pytest.raises(AssertionError, match="sel = 0"):
        FC.hold(c, "fp32", out)


def test_p_drop_edge_rule(monkeypatch):
    """p = 2^-17 rounds the 16-bit keep threshold to 65536: the generator keeps every unit, and the reference still scales by
    1 / (1 - p), as the Dropout modules do.  A network WITHOUT the scale -- what the VALU and fp32 matrix kernels computed at
    this edge while the host had one rule for the masks and ops.FieldDev another for the scale -- is 2^-17 off per scaled
    layer: inside the bound with two scaled layers, beyond it with three, so case I-p2^-17-s7 sees it."""
    ratios = {}
    for key in ("I-p2^-17", "I-p2^-17-s7"):
        c = FC.case(key)
        assert not c.keeps and FC.drop_scale(c.K, c.p) == 1.0 / (1.0 - 2.0 ** -17) and FC.mask_threshold(c.p) == 65536
        monkeypatch.setattr(FC, "drop_scale", lambda K, p: 1.0)
        for bf in FC.bound_families(c):
            ratios[key, bf] = FC.hold_ratio_unscaled(c, bf, FC.chain(c, bf)) / FC.FACTOR[bf]
            print(f"{key}: {bf} chain WITHOUT the scale against the scaled reference: error / bound {ratios[key, bf]:.4f}")
        monkeypatch.undo()
    assert ratios["I-p2^-17-s7", "fp32"] > 1.0, "the unscaled fp32 network is beyond its bound"
    assert ratios["I-p2^-17", "fp32"] < 1.0
