"""The hand-placed Laplace cases of tests/laplace_cases.py, checked without a GPU.  The float64 reference meets O.laplace_field
run in float64 (two independently written statements of the sampled heads); the CPU chains of the three bound families go
through the very `hold` tests/test_gpu_laplace_edges.py applies to the kernels, and the recorded ratios are re-measured; the
cases cover every edge the module lists, with the logit-range and set-distinctness conditions asserted on the reference when
a case is built; and each mutation of a chain fails `hold` on at least one case, so the bounds are tight enough to see a
kernel that is wrong in that way."""
import numpy as np
import pytest
import torch

import field_cases as FC
import laplace_cases as LC
from oracle import nerf_oracle as O


@pytest.mark.parametrize("key", list(LC.CASES))
def test_case_builds_and_cpu_chains_pass_hold(key):
    c = LC.case(key)
    ratios = {bf: LC.hold(c, bf, LC.chain(c, bf)) for bf in LC.bound_families(c)}
    print(f"{key}: net {c.net.name} n_lap {c.n}/{c.nr} sets {c.sets} tiles {c.tiles} live {int(c.sel.sum())} of {c.N} CPU chain error / bound: "
          + " ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    for ref in c.ref.values():
        for name in ("b_dens", "b_rgb", "b_var_rgb") + (() if c.mask else ("b_var_d",)):
            for b in getattr(ref, name).values():
                assert np.isfinite(b).all() and (b[c.sel] > 0).all() if name == "b_dens" else np.isfinite(b).all() and (b > 0).all()
        assert np.isfinite(ref.dens).all() and np.isfinite(ref.var_d).all() and (ref.var_rgb >= 0).all()
        assert (ref.var_d >= 0).all(), "the float64 variance itself is not negative"


def test_cases_cover_the_kernel_edges():
    LC.check_coverage()


@pytest.mark.parametrize("bf", ["fp32", "f16x2", "f16"])
def test_bounds_rest_on_the_measured_cpu_chains(bf):
    worst = LC.measure_chain(bf)
    print(f"{bf} chain vs float64 over all cases: worst error / unscaled bound {worst:.4f}")
    assert LC.RATIO_MEASURED[bf] >= worst and LC.FACTOR[bf] >= 4 * worst
    assert LC.RATIO_MEASURED[bf] <= 1.02 * worst + 1e-3, "the recorded ratio is the re-measured one"
    assert LC.FACTOR[bf] <= 4.1 * LC.RATIO_MEASURED[bf], "FACTOR is 4 x the measured worst, rounded up"
    assert LC.FACTOR[bf] < LC.FACTOR_MAX, "set-distinctness is asserted beyond every family's factor"


@pytest.mark.parametrize("name,act", [("t", "exp"), ("t-box", "softplus")])
def test_reference_meets_the_oracle_in_float64(name, act):
    """the oracle's Laplace field in float64 AT the float32 positions: a unit scene box and all-zero bins make the oracle's own
    position arithmetic exact (p = x), so that only the network is compared"""
    nt = LC.net(name)
    rng = np.random.default_rng(len(name))
    N, n = 96, 11
    P = rng.uniform(0.01, 0.99, (N, 3)).astype(np.float32)
    dirs = rng.standard_normal((N, 3))
    dirs = (np.round(dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * 4096) / 4096).astype(np.float32)
    wsd, wsr = LC.weight_sets(nt, "spread", n, n, 1, act, 5)
    c = LC.SimpleNamespace(net=nt, N=N, n=n, nr=n, P32=P, shin=FC.sh_inputs32(dirs, nt.sh_remap), sel=np.ones(N, bool), act=act, mask=0,
                           set_of=np.zeros(N, np.int64), wsd=wsd, wsr=wsr)
    ref = LC.reference(c, rounded=False)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    g = O.GridMLP(table=t(nt.table), scalings=t(nt.scalings), log2_T=nt.log2T, weights=[t(nt.w0)], biases=[t(nt.b0)], tcnn_levels=None,
                  aabb=t(np.array((0.0, 0.0, 0.0, 1.0, 1.0, 1.0), np.float32).reshape(2, 3)), grid_half=False)
    fp = O.FieldParams(grid=g, head_w=[t(nt.h0), t(nt.h1), t(nt.cmean[:192].reshape(3, 64))], head_b=[t(nt.hb0), t(nt.hb1), t(nt.cmean[192:])],
                       appearance=t(np.zeros(0, np.float32)), average_init_density=1.0, beta_min=0.01, sh_remap=bool(nt.sh_remap))
    fp.hidden_w, fp.hidden_b, fp.density_activation = t(nt.w1), t(nt.b1), act
    mu_d, var_d, mu_rgb, var_rgb = O.laplace_field(t(P), t(dirs), torch.zeros(N, 2, dtype=torch.float64), fp, t(wsd[0]), t(wsr[0]))
    close = lambda a, b, what: np.testing.assert_allclose(a, b.numpy().reshape(a.shape), rtol=1e-9, atol=1e-13, err_msg=what)
    close(ref.dens, mu_d, "mu_d")
    close(ref.rgb, mu_rgb, "mu_rgb")
    assert np.abs(ref.var_d - var_d.numpy().reshape(-1)).max() <= 1e-12 * (ref.dens ** 2).max()
    assert np.abs(ref.var_rgb - var_rgb.numpy().reshape(-1)).max() <= 1e-13


@pytest.mark.parametrize("mut", list(LC.MUTATIONS))
def test_mutated_chain_fails_hold(mut):
    bf, applies = LC.MUTATIONS[mut]
    failed, tried = [], 0
    for key in LC.CASES:
        c = LC.case(key)
        if bf not in LC.bound_families(c) or not applies(c):
            continue
        tried += 1
        try:
            LC.hold(c, bf, LC.chain(c, bf, mut))
        except AssertionError:
            failed.append(key)
    print(f"{mut} ({bf} chain): fails hold on {len(failed)} of {tried} cases, first {failed[:4]}")
    assert failed, f"the {bf} chain with '{mut}' passes every case: the bounds would let such a kernel through"


def test_hold_rejects_sentinels_nan_negative_colour_variance_and_a_residual_under_the_mask():
    c = LC.case("M-exp")
    good = LC.chain(c, "fp32")
    LC.hold(c, "fp32", good)
    for key, value, match in (("dens", np.array([LC.SENTINEL], np.uint32).view(np.float32)[0], "sentinel"), ("rgb", np.float32(np.nan), "NaN"),
                              ("var_rgb", np.float32(-1e-12), "negative colour variance"), ("var_d", np.float32(1e-30), "not exactly 0")):
        out = {k: v.copy() for k, v in good.items()}
        out[key].reshape(-1)[int(np.argmax(c.sel))] = value
        with pytest.raises(AssertionError, match=match):
            LC.hold(c, "fp32", out)
    out = {k: v.copy() for k, v in good.items()}
    out["dens"][int(np.argmin(c.sel))] = np.float32(1e-30)
    with pytest.raises(AssertionError, match="sel = 0"):
        LC.hold(c, "fp32", out)
    x = LC.case("X-exp-n5")
    out = {k: v.copy() for k, v in LC.chain(x, "fp32").items()}
    out["dens"][3] = np.nextafter(np.float32(1), np.float32(2))          # inside the bound, and not one of the two exact values
    with pytest.raises(AssertionError, match="padded row"):
        LC.hold(x, "fp32", out)


# ------------------------------------------------------------------------------------------------------ Part 2: the GGN fit
@pytest.mark.parametrize("key", list(LC.GGN_CASES))
def test_ggn_case_builds_and_the_fp32_chain_passes_hold(key):
    """building a case asserts the gate condition on the reference alone: no rendered channel within 100 x its bound of 0 or 1"""
    c = LC.ggn_case(key)
    margin = np.minimum(np.abs(c.ref.pred), np.abs(c.ref.pred - 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"{key}: net {c.net.name} bg {c.bg} {c.act} waves {LC.ggn_waves(c.R)}; gate margin / bound >= {np.where(c.ref.gated, margin / c.ref.dpred, np.inf).min():.0f}; "
              f"clamped channels {int(((c.ref.live == 0) & c.ref.gated).sum())} of {c.ref.live.size}; fp32 chain error / bound {LC.ggn_hold(c, LC.ggn_chain(c)):.3f}")


def test_ggn_cases_cover_the_kernel_edges():
    LC.ggn_check_coverage()


def test_ggn_bound_rests_on_the_measured_fp32_chain():
    worst = LC.ggn_measure_chain()
    print(f"GGN fp32 chain vs float64 over all cases: worst error / unscaled bound {worst:.4f}")
    assert LC.GGN_RATIO_MEASURED >= worst and LC.GGN_FACTOR >= 4 * worst
    assert LC.GGN_RATIO_MEASURED <= 1.02 * worst + 1e-3 and LC.GGN_FACTOR <= 4.1 * LC.GGN_RATIO_MEASURED


@pytest.mark.parametrize("mut", list(LC.GGN_MUTATIONS))
def test_mutated_ggn_chain_fails_hold(mut):
    failed, tried = [], 0
    for key in LC.GGN_CASES:
        c = LC.ggn_case(key)
        if not LC.GGN_MUTATIONS[mut](c):
            continue
        tried += 1
        try:
            LC.ggn_hold(c, LC.ggn_chain(c, mut))
        except AssertionError:
            failed.append(key)
    print(f"{mut}: fails ggn_hold on {len(failed)} of {tried} cases, first {failed[:4]}")
    assert failed, f"the fp32 chain with '{mut}' passes every case"


@pytest.mark.parametrize("key", ["G-r3-s17-none", "G-r4-s2-const", "G-r5-s63-clamp", "G-r5-s1-last", "G-r35-s2-const-sp"])
def test_ggn_closed_form_meets_float64_autograd(key):
    """the reference's closed-form Jacobian against autograd through the renderer (weights, background blend, clamp) on the
    float64 forward's last-layer inputs: one backward per ray and channel"""
    c = LC.ggn_case(key)
    R, S, nt = c.R, c.S, c.net
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))
    wd, wr = t(nt.dmean).requires_grad_(), t(nt.cmean).requires_grad_()
    X, H, sel = t(c.fw.X), t(c.fw.H), t(c.sel.astype(np.float64))
    pre = X @ wd[:64] + wd[64]
    sigma = ((torch.nn.functional.softplus(pre, threshold=1e9) if c.act == "softplus" else torch.exp(pre)) * sel).reshape(R, S)
    col = torch.sigmoid(H @ wr[:192].reshape(3, 64).T + wr[192:]).reshape(R, S, 3)
    e = LC.PC.s2e32(c.sb, c.near, c.far, c.lin).astype(np.float64)
    dd = t(e[:, 1:] - e[:, :-1]) * sigma
    T = torch.exp(-(torch.cumsum(dd, 1) - dd))
    w = (1 - torch.exp(-dd)) * T
    bg = col[:, -1] if c.bg[0] == LC.BG_LAST else t(np.array(c.bg[1] if c.bg[0] == LC.BG_COLOR else (0.0, 0.0, 0.0))).expand(R, 3)
    pred = torch.clamp((w[..., None] * col).sum(1) + (1 - w.sum(1))[:, None] * bg, 0.0, 1.0)
    d, r = torch.zeros(65, dtype=torch.float64), torch.zeros(195, dtype=torch.float64)
    for i in range(R):
        for k in range(3):
            gd, gr = torch.autograd.grad(pred[i, k], (wd, wr), retain_graph=True, allow_unused=True)
            d += 2 * (0 if gd is None else gd ** 2)
            r += 2 * (0 if gr is None else gr ** 2)
    np.testing.assert_allclose(c.ref.d, d.numpy(), rtol=1e-9, atol=1e-12 * max(float(d.max()), 1e-300))
    np.testing.assert_allclose(c.ref.r, r.numpy(), rtol=1e-9, atol=1e-12 * max(float(r.max()), 1e-300))
