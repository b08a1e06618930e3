"""The hand-placed any-width cases of tests/width_cases.py, checked without a GPU.  The nets and cases cover what the module's
header lists; generic_rows as restated equals what the host computes and holds the widest activation of every case; the
float64 reference meets the oracle's fp32 field functions (which take their shapes from the weights) under the very bound the
kernel is held to; the reference's masks are O.mc_keep_mask sliced, and mask_any's pairing restated gives the same masks; the CPU
chain goes through the `hold` tests/test_gpu_width_edges.py applies to the kernel and the recorded ratios are re-measured; each
mutation of the chain fails `hold` on a named case; and FieldDev.from_torch refuses the widths that cannot be expressed."""
import numpy as np
import pytest
import torch

import field_cases as FC
import width_cases as WC
from oracle import nerf_oracle as O


@pytest.mark.parametrize("key", list(WC.CASES))
def test_case_builds_and_the_cpu_chain_passes_hold(key):
    c = WC.case(key)
    ratio = WC.hold(c, WC.chain(c))
    print(f"{key}: net {c.net.name} rows {c.net.rows} N {c.N} live {int(c.sel.sum())} passes {c.B} CPU chain error / bound {ratio:.3f}")
    for _, _, r, b in WC.items(c):
        assert np.isfinite(r).all() and np.isfinite(b).all() and (b >= 0).all()


def test_cases_cover_the_kernel_edges():
    WC.check_inventory()


def test_rows_restated_hold_the_widest_activation():
    """generic_rows is the maximum of five terms; what the kernel needs is that no buffer ever holds more rows.  The term
    G + 2 can never be the largest (16 + G + AD exceeds it for every AD), so the restated maximum without it is the same"""
    for name, (layout, log2T, box, L, F, H, HC, G, AD) in WC.NETS.items():
        for lap in (False, True):
            nt = WC.net(name, lap)
            assert nt.rows == max(L * F, H, HC, 16 + G + (nt.AD or 32)) == WC.generic_rows(L, F, H, HC, G, nt.AD)
            assert nt.rows * 64 * 4 * 4 <= 160 * 1024
    for key in WC.CASES:
        c = WC.case(key)
        assert c.net.rows >= WC.widest_activation(c.net, c.mode, c.headin), key
    assert WC.net("n").rows * 1024 == 160 * 1024 and WC.net("k").rows * 1024 == 65 * 1024


def _euclid(c):
    sb = torch.from_numpy(c.sb)
    return sb if c.bins == "euclid" else O.spacing_to_euclidean(sb, c.near, c.far, uniform=bool(c.lin))


@pytest.mark.parametrize("key", list(WC.CASES))
def test_reference_holds_the_fp32_oracle(key):
    """O.active_field / O.mcdropout_field / O.laplace_field on the case's own rays, in fp32, with the reference's masks: inside
    the bound the kernel is held to (same factor)"""
    c = WC.case(key)
    o, d, fp = torch.from_numpy(c.origins), torch.from_numpy(c.dirs), WC.oracle_params(c)
    if c.mode == WC.ACTIVE:
        dens, rgb, beta = O.active_field(o, d, _euclid(c), fp)
        out = {"dens": dens.numpy().reshape(1, -1), "rgb": rgb.numpy().reshape(1, -1, 3), "beta": beta.numpy().reshape(-1)}
    elif c.mode == WC.MCDROPOUT:
        out = {"dens": np.zeros((c.B, c.N), np.float32), "rgb": np.zeros((c.B, c.N, 3), np.float32)}
        on = FC.site_set(c.sites) if c.K > 0 else 0
        for k in range(c.B):
            m = lambda site: (torch.from_numpy(c.keeps[site][k]) if site in c.keeps else torch.ones(c.N, WC.UNITS[site](c.net), dtype=torch.bool)) \
                if on & site else None
            dens, rgb = O.mcdropout_field(o, d, _euclid(c), fp, m(WC.TRUNK), m(WC.HEAD1), float(np.float32(c.p)), keep_head0=m(WC.HEAD0),
                                          keep_in=m(WC.HEADIN))
            out["dens"][k], out["rgb"][k] = dens.numpy().reshape(-1), rgb.numpy().reshape(-1, 3)
    else:
        parts = []
        for st in np.unique(c.set_of):       # one call per sample set: the oracle takes one set
            rays = np.flatnonzero(c.set_of.reshape(c.R, c.S)[:, 0] == st)
            r = O.laplace_field(o[rays], d[rays], _euclid(c)[rays], fp, torch.from_numpy(c.wsd[st]), torch.from_numpy(c.wsr[st][:c.nr]))
            parts.append([x.numpy().reshape(len(rays) * c.S, -1) for x in r])
        mu_d, var_d, mu_rgb, var_rgb = (np.concatenate([p[i] for p in parts]) for i in range(4))
        if c.mask:                           # use_deterministic_density: mu sel and no variance (laplace_field.py:317-345)
            mu_d, var_d = mu_d * c.sel[:, None].astype(np.float32), 0 * var_d
        out = {"dens": mu_d.reshape(1, -1), "rgb": mu_rgb.reshape(1, -1, 3), "var_d": var_d.reshape(-1), "var_rgb": var_rgb.reshape(-1)}
    print(f"{key}: fp32 oracle error / bound {WC.hold(c, out):.3f}")


def test_masks_are_the_oracle_generators_sliced():
    seen = 0
    for key in WC.CASES:
        c = WC.case(key)
        sidx = (np.arange(c.N, dtype=np.uint64) + np.uint64(c.first_sample)).astype(np.uint32)
        for site, keep in c.keeps.items():
            n = WC.UNITS[site](c.net)
            assert keep.shape == (c.K, c.N, n)
            for k in range(c.K):
                want = O.mc_keep_mask(c.seed, k, sidx, FC.STREAM[site], n + (n & 1), float(np.float32(c.p)))[:, :n]
                assert np.array_equal(keep[k], want), (key, site, k)
                assert np.array_equal(WC._chain_mask(c.net, c.seed, k, c.p, site, sidx, None), want), (key, site, k, "mask_any restated")
                seen += 1
    assert seen > 20


@pytest.mark.parametrize("family", ["field", "laplace"])
def test_bounds_rest_on_the_measured_cpu_chain(family):
    worst = WC.measure_chain(family)
    print(f"{family}: chain vs float64 over all cases: worst error / unscaled bound {worst:.4f}")
    assert WC.RATIO_MEASURED[family] >= worst and WC.FACTOR[family] >= 4 * worst
    assert WC.RATIO_MEASURED[family] <= 1.02 * worst + 1e-3, "the recorded ratio is the re-measured one"
    assert WC.FACTOR[family] <= 4.1 * WC.RATIO_MEASURED[family], "FACTOR is 4 x the measured worst, rounded up"


@pytest.mark.parametrize("mut", list(WC.MUTATIONS))
def test_mutated_chain_fails_hold(mut):
    failed, tried = [], 0
    for key in WC.CASES:
        c = WC.case(key)
        if not WC.MUTATIONS[mut](c):
            continue
        tried += 1
        try:
            WC.hold(c, WC.chain(c, mut))
        except AssertionError:
            failed.append(key)
    print(f"{mut}: caught on {len(failed)} of {tried} cases, first {failed[:4]}")
    assert failed, f"the chain with '{mut}' passes every case: the bounds would let such a kernel through"


def test_hold_rejects_sentinels_nan_and_unmasked_density():
    c = WC.case("A-b-n63")
    good = WC.chain(c)
    assert (~c.sel).any()
    for key, value in (("dens", np.array([WC.SENTINEL], np.uint32).view(np.float32)[0]), ("rgb", np.float32(np.nan))):
        out = {k: None if v is None else v.copy() for k, v in good.items()}
        out[key].reshape(-1)[int(np.argmax(c.sel)) * (3 if key == "rgb" else 1)] = value
        with pytest.raises(AssertionError):
            WC.hold(c, out)
    out = {k: None if v is None else v.copy() for k, v in good.items()}
    out["dens"][0, int(np.argmin(c.sel))] = np.float32(1e-30)
    with pytest.raises(AssertionError, match="sel = 0"):
        WC.hold(c, out)


def _from_torch(nt, mode, **kw):
    from uncertainty_nerf_gs_amd import ops
    t = torch.from_numpy
    out1 = nt.G + 2 if mode == WC.ACTIVE else nt.G + 1
    return ops.FieldDev.from_torch(mode, t(nt.table), t(nt.scalings), nt.log2T, t(nt.w0), t(nt.b0), t(nt.w1[:out1]), t(nt.b1[:out1]),
                                   [t(nt.h0), t(nt.h1), t(nt.h2)], [t(nt.hb0), t(nt.hb1), t(nt.hb2)], t(nt.app), "cpu", **kw)


def test_widths_that_cannot_be_expressed_are_refused_by_name(monkeypatch):
    """A 0 in unerf_field_params means "the default", so geo_feat_dim = 0 would reach the kernel as 15 and an empty appearance
    embedding under UNERF_DROP_HEADIN as 32 (then refused downstream, about out1 or a null app_embed).  FieldDev.from_torch
    refuses both by name, before any library call; an empty embedding WITHOUT that site stays expressible (an empty block
    folded into the bias: the Laplace nets here)"""
    import warnings
    from types import SimpleNamespace
    from uncertainty_nerf_gs_amd import lib as L, ops
    monkeypatch.setattr(L, "load", lambda: pytest.fail("a library call before the refusal"))
    monkeypatch.setattr(ops, "_warned_any_width", set(ops._warned_any_width))      # the any-width notice stays whoever's comes next
    nt = WC.net("a")
    g0 = SimpleNamespace(**{**vars(nt), "G": 0, "w1": nt.w1[[0, nt.G + 1]], "b1": nt.b1[[0, nt.G + 1]],
                            "h0": np.ascontiguousarray(np.delete(nt.h0, np.s_[16:16 + nt.G], axis=1))})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for mode in (WC.ACTIVE, WC.MCDROPOUT):
            with pytest.raises(L.UnerfError, match="geo_feat_dim = 0"):
                _from_torch(g0, mode)
        a0 = SimpleNamespace(**{**vars(nt), "AD": 0, "app": nt.app[:0], "h0": np.ascontiguousarray(nt.h0[:, :16 + nt.G])})
        with pytest.raises(L.UnerfError, match="appearance_embed_dim = 0"):
            _from_torch(a0, WC.MCDROPOUT, K=2, drop_sites=WC.HEADIN)
        f = _from_torch(a0, WC.MCDROPOUT, K=2)          # the default sites: nothing reads the width
        assert f.any_width and f.app_dim == 0 and torch.equal(f.hb0, torch.from_numpy(nt.hb0))
