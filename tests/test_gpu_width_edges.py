"""The any-width field kernel (field_kernel_generic, csrc/unerf_nerf.hip section 5a') on the hand-placed cases of
tests/width_cases.py: ACTIVE, MCDROPOUT and LAPLACE, every launch through ops.field_fwd on a FieldDev.from_torch of the net.
Every output of every pass is held to a float64 reference under a derived bound: no share of outputs is exempt, and an output
with sel = 0 must be exactly 0 (the LAPLACE density only under lap_mask_density).

What the cases aim at (width_cases.py lists and checks them): H, HC and the trunk's output count in every residue class
{0, 1, 7} mod 8 and below 8 (the tails of dense_any's 8-output sweeps), odd unit counts of a mask site, 128 units, HEADIN with
the appearance rows unfolded at 29, 54, 56 and 80 units, L from 1 to 32 with 2 and 4 features per level, all three grid layouts
and the wrap branch of a dense tcnn level, N = R S in {1, 63, 64, 65, 96, 129} (the partial last workgroup), ray offsets, K in
{0, 1, 3}, p_drop = 2^-18, every Laplace option with per-lane sample sets, and 65, 128 and 160 KiB of dynamic LDS.  The outputs
are views of an arena that holds a NaN payload, with guard floats in front of and behind each: the guards must come back
untouched and no output may keep the payload.

Bounds: width_cases.py states and derives them; none comes from a kernel.  Every test prints its worst error / bound next to
the CPU chain's."""
import dataclasses
import warnings

import numpy as np
import pytest
import torch

import field_cases as FC
import width_cases as WC

pytestmark = pytest.mark.gpu
_GUARD = 8                    # floats in front of an output and behind it
_FIELDS, _RESULT = {}, {}


def _arena(dev):
    """an ops.Workspace whose buffers sit between guard floats and hold the NaN payload: ops.field_fwd writes into views of it"""
    from uncertainty_nerf_gs_amd import ops

    class Guarded(ops.Workspace):
        def __init__(self):
            super().__init__()
            self.raw = {}

        def get(self, tag, shape, device, dtype=torch.float32):
            n = int(np.prod(shape))
            buf = torch.full((_GUARD + n + _GUARD,), WC.SENTINEL, dtype=torch.int32, device=device).view(torch.float32)
            self.raw[tag] = (buf, n)
            return buf[_GUARD:_GUARD + n].view(*shape)

        def check(self, name):
            assert self.raw, "ops.field_fwd took no output from the arena"
            for tag, (buf, n) in self.raw.items():
                bits = buf.cpu().view(torch.int32)
                assert (bits[:_GUARD] == WC.SENTINEL).all(), f"{name}: a float in front of {tag} was written"
                assert (bits[_GUARD + n:] == WC.SENTINEL).all(), f"{name}: a float behind {tag} was written"

    return Guarded()


def _field(dev, c):
    """the case's net as a FieldDev; from_torch gives the any-width notice (once per process and width set: taken here, and
    left to be given to whoever comes next)"""
    from uncertainty_nerf_gs_amd import lib as L, ops
    nt = c.net
    key = (nt.name, c.mode, c.K, c.p, c.sites, c.seed, c.name if c.mode == WC.LAPLACE else None)
    if key in _FIELDS:
        return _FIELDS[key]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    tcnn = nt.layout != "torch"
    common = dict(tcnn_levels=nt.levels, sh_remap=nt.sh_remap, aabb=nt.aabb, grid_precision="f16" if nt.layout == "tcnn16" else "f32")
    noticed = set(ops._warned_any_width)
    ops._warned_any_width.discard((nt.H, nt.HC, nt.G, nt.F, nt.L))
    with pytest.warns(UserWarning, match="any-width kernel"):
        if c.mode == WC.LAPLACE:
            HC = nt.HC
            stacked = c.chunk > 0
            f = ops.FieldDev.from_torch(
                L.FIELD_LAPLACE, t(nt.table), None if tcnn else t(nt.scalings), nt.log2T, t(nt.w0), t(nt.b0), t(nt.w1), t(nt.b1),
                [t(nt.h0), t(nt.h1), t(nt.cmean[:3 * HC].reshape(3, HC))], [t(nt.hb0), t(nt.hb1), t(nt.cmean[3 * HC:])], torch.zeros(0), dev,
                ws_density=t(c.wsd if stacked else c.wsd[0]), ws_rgb=t(c.wsr if stacked else c.wsr[0]), lap_softplus=int(c.act == "softplus"),
                lap_mask_density=c.mask, lap_chunk_rays=c.chunk, **common)
            assert f.lap_blob is None
        else:
            out1 = nt.G + 2 if c.mode == WC.ACTIVE else nt.G + 1
            f = ops.FieldDev.from_torch(
                c.mode, t(nt.table), None if tcnn else t(nt.scalings), nt.log2T, t(nt.w0), t(nt.b0), t(nt.w1[:out1]), t(nt.b1[:out1]),
                [t(nt.h0), t(nt.h1), t(nt.h2)], [t(nt.hb0), t(nt.hb1), t(nt.hb2)], t(nt.app), dev, K=c.K, seed=c.seed, p_drop=float(c.p),
                drop_sites=c.sites, average_init_density=FC.AVG, beta_min=FC.BETA_MIN, **common)
    ops._warned_any_width.intersection_update(noticed)
    assert f.any_width and f.mfma_blob is None and f.mfma16_blob is None
    assert (f.hidden, f.hidden_color, f.geo_dim, f.feat_per_level, f.app_dim) == (nt.H, nt.HC, nt.G, nt.F, nt.AD)
    if c.mode == WC.LAPLACE and c.nr_arg == 0:       # n_lap_rgb = 0 in the parameters: the entry point takes n_lap
        class RgbCountLeftOut(type(f)):
            def cstruct(self):
                cs = super().cstruct()
                cs.n_lap_rgb = 0
                return cs
        f = RgbCountLeftOut(**{fl.name: getattr(f, fl.name) for fl in dataclasses.fields(f)})
    _FIELDS[key] = f
    return f


def _launch(dev, c, rays=None, off=None, field=None, extra=None):
    """one ops.field_fwd on rays [r0, r1) of the case (extra: (origins, dirs, sb) rows put in front of them) -> the result dict
    width_cases.hold takes, float32 numpy; guards checked"""
    from uncertainty_nerf_gs_amd import ops
    field = field or _field(dev, c)
    r0, r1 = (0, c.R) if rays is None else rays
    arrs = [a[r0:r1] for a in (c.origins, c.dirs, c.sb)]
    if extra is not None:
        arrs = [np.concatenate([e, a]) for e, a in zip(extra, arrs)]
    o, d, sb = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs)
    n = o.shape[0] * c.S
    B = max(field.K, 1) if c.mode == WC.MCDROPOUT else 1
    ws = _arena(dev)
    dens, rgb, aux, aux2 = ops.field_fwd(o, d, sb, field, c.near, c.far, ray_offset=(c.off + r0) if off is None else off,
                                         euclidean_bins=c.bins == "euclid", spacing=c.lin, workspace=ws)
    torch.cuda.synchronize(dev)
    ws.check(c.name)
    out = {"dens": dens.cpu().numpy().reshape(B, n).copy(), "rgb": rgb.cpu().numpy().reshape(B, n, 3).copy()}
    assert (aux is None) == (c.mode == WC.MCDROPOUT) and (aux2 is None) == (c.mode != WC.LAPLACE)
    if c.mode == WC.ACTIVE:
        out["beta"] = aux.cpu().numpy().reshape(n).copy()
    elif c.mode == WC.LAPLACE:
        out["var_d"], out["var_rgb"] = aux.cpu().numpy().reshape(n).copy(), aux2.cpu().numpy().reshape(n).copy()
    return out


def _base(dev, key):
    if key not in _RESULT:
        _RESULT[key] = _launch(dev, WC.case(key))
    return _RESULT[key]


def _same(a, b, rows=slice(None), rows_b=slice(None)):
    cut = lambda x, r: x[:, r] if x.ndim >= 2 else x[r]
    return set(a) == set(b) and all(np.array_equal(cut(a[k], rows).view(np.uint32), cut(b[k], rows_b).view(np.uint32)) for k in a)


# ------------------------------------------------------------------------------------------------------- every output
@pytest.mark.parametrize("key", list(WC.CASES))
def test_every_output_within_its_bound_and_a_second_call_gives_the_same_bits(dev, key):
    """The two cases at rows = 160 ask for 163,840 bytes of dynamic LDS, exactly what field_check_nonempty accepts.  Observed on
    an MI355X: the launch is accepted and every output is within its bound (the device's per-block limit is 160 KiB)."""
    c = WC.case(key)
    out = _base(dev, key)
    ratio = WC.hold(c, out)
    assert _same(_launch(dev, c), out), f"{key}: a second call differs"
    mode = {WC.ACTIVE: "ACTIVE", WC.MCDROPOUT: f"MCDROPOUT K={c.K} sites={FC.site_set(c.sites)} p={c.p:g}",
            WC.LAPLACE: f"LAPLACE n_lap {c.n}/{getattr(c, 'nr_arg', 0)} {c.act}{' masked' if c.mask else ''} chunk {c.chunk}"}[c.mode]
    print(f"RATIO {key} (net {c.net.name}: {c.net.layout} L={c.net.L} F={c.net.F} {c.net.H}/{c.net.HC}/{c.net.G}/{c.net.AD}, rows {c.net.rows}; "
          f"{mode}; N={c.N} off={c.off}) worst error / bound: kernel {ratio:.3f}, CPU chain {WC.hold(c, WC.chain(c)):.3f}")


# ---------------------------------------------------------------------------------------------- bit for bit, launch shapes
@pytest.mark.parametrize("key", [k for k, s in WC.CASES.items() if s["R"] * s["S"] in (63, 65, 129)])
def test_a_launch_one_ray_shorter_gives_the_same_rows(dev, key):
    """the partial last workgroup clamps its idle lanes to sample N - 1: with S = 1 the launch of N - 1 samples (with S = 3 the
    launch one ray shorter) must give the bits of the first rows of the whole one"""
    c = WC.case(key)
    part = _launch(dev, c, rays=(0, c.R - 1))
    n = (c.R - 1) * c.S
    assert _same(part, _base(dev, key), rows_b=slice(0, n)), f"{key}: the first {n} rows differ from the launch of {n} samples"
    WC.hold(c, part, rows=slice(0, n))


@pytest.mark.parametrize("key", [k for k, s in WC.CASES.items() if s["off"]])
def test_a_ray_offset_equals_the_later_rows_of_the_longer_launch(dev, key):
    """ray_offset = off with R rays against ray_offset = 0 with off + R rays (the mask counter and the sample-set index both
    count from the offset)"""
    c = WC.case(key)
    extra = [a[-c.off:] for a in (c.origins, c.dirs, c.sb)]
    longer = _launch(dev, c, off=0, extra=extra)
    assert _same(longer, _base(dev, key), rows=slice(c.off * c.S, None)), f"{key}: rows {c.off}.. of the launch at offset 0 differ"
    if c.keeps:
        assert not _same(_launch(dev, c, off=0), _base(dev, key)), f"{key}: the offset does not reach the mask counter"


def test_rays_away_from_the_wrap_give_the_same_bits_with_and_without_wave_mates_in_the_last_cell(dev):
    """a dense tcnn level: one lane whose cell touches the end of the level sends its whole wave through the wrap branch (eight
    single loads, indices reduced modulo the level size) instead of the four paired loads: the same features either way"""
    for key in ("T-wrap-a", "T-wrap-m", "T-wrap-c32"):
        c = WC.case(key)
        w = WC.wraps(c.net, c.P32)
        assert not w[:WC.WRAP_CLEAR].any() and w[WC.WRAP_CLEAR:].all()
        alone = _launch(dev, c, rays=(0, WC.WRAP_CLEAR))
        assert _same(alone, _base(dev, key), rows_b=slice(0, WC.WRAP_CLEAR)), f"{key}: the paired loads and the wrap branch differ"


# ------------------------------------------------------------------------------------------------------ across the passes
def test_no_passes_is_the_unmasked_network(dev):
    """K = 0: one pass, no masks, no scale (held to the unmasked reference above) -- and the bits of K = 1 at p_drop = 0"""
    c = WC.case("M-b-k0")
    assert c.K == 0 and c.B == 1 and not c.keeps and FC.drop_scale(c.K, c.p) == 1.0
    f = _field(dev, c)
    assert _same(_launch(dev, c, field=dataclasses.replace(f, K=1, p_drop=0.0)), _base(dev, "M-b-k0"))


@pytest.mark.parametrize("key", ["M-b-k3-off", "M-c-k3-trunk", "M-a-k3-headin"])
def test_three_passes_differ_where_their_masks_do(dev, key):
    """every pass is held to its own masks above; here: the passes are not copies of one another, and sites without the trunk
    leave the density alone"""
    c = WC.case(key)
    out = _base(dev, key)
    assert c.B == 3 and all(not np.array_equal(out["rgb"][k], out["rgb"][0]) or not np.array_equal(out["dens"][k], out["dens"][0]) for k in (1, 2))
    head = WC.case("M-c-k1-head01")
    assert not FC.site_set(head.sites) & WC.TRUNK
    three = _launch(dev, head, field=dataclasses.replace(_field(dev, head), K=3))
    assert all(np.array_equal(three["dens"][k], three["dens"][0]) for k in (1, 2)) and not np.array_equal(three["rgb"][1], three["rgb"][0])


def test_passes_without_a_dropped_unit_are_identical_and_scaled(dev):
    c = WC.case("M-c-k3-p2^-18")
    out = _base(dev, c.name)
    assert c.B == 3 and not c.keeps and FC.drop_scale(c.K, c.p) > 1
    assert all(np.array_equal(out[k][q], out[k][0]) for k in ("dens", "rgb") for q in (1, 2))
    unscaled = _launch(dev, c, field=dataclasses.replace(_field(dev, c), K=0))
    assert not _same({k: v[:1] for k, v in out.items()}, unscaled), "1 / (1 - p) at p = 2^-18 left no trace: the scale is not applied"


def test_an_active_field_ignores_k_and_writes_beta_once(dev):
    c = WC.case("A-c-n65")
    out = _launch(dev, c, field=dataclasses.replace(_field(dev, c), K=3, p_drop=0.5))
    assert out["dens"].shape == (1, c.N) and out["beta"].shape == (c.N,) and _same(out, _base(dev, c.name))
