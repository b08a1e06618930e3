"""The main field kernels behind unerf_field_fwd / unerf_field_fwd_masked on the hand-placed cases of tests/field_cases.py:
field_kernel (VALU), field_kernel_mfma (exact fp32 matrix kernel), field_kernel_mfma16 in its split ("f16x2") and its
single-product ("f16") form, ACTIVE and MCDROPOUT, generated and explicit masks.  Every output of every pass is held to a
float64 reference under a derived bound: no share of outputs is exempt, and a density with sel = 0 must be exactly 0.

What the cases aim at (field_cases.py lists and checks them): R in {1, 31, 32, 33, 65}, S in {1, 2, 3, 17, 48}, R S in
{1, 63, 64, 65} (the VALU kernel's clamp to N - 1), 1, 7, 8, 9, 17, 33 and 96 tiles (empty, partial and uneven XCD slices, the
surplus workgroups of the rounded-up persistent grid) and more tiles than 4 x the grid (a wave walks a second tile); image
widths 8, 9, 37, 64 with R on 4 x width and one below, a ray_offset inside a row and a band, a last band of one live row; the
three grid layouts under both normalisations; ReLU zeros, f16 range borders, saturated sigmoids and the softplus switch as
planted pre-activations; K in {0, 1, 2, 3, 8, 10}, every drop_sites set, p_drop in {0, 2^-17, 2^-16, 0.2, 0.5, 0.9}, a mask
counter that ends on 2^32 - 1.  Every launch goes through the C ABI; each output buffer sits between guard floats, and output
and guards hold a NaN payload before the launch: the guards must come back untouched (the clamped invalid columns of a tile)
and no output may keep the payload.

Bounds: field_cases.py states and derives them; none comes from a kernel.  Every test prints its worst error / bound
(DESIGN.md section 6.1 records them)."""
import ctypes as C
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import field_cases as FC

pytestmark = pytest.mark.gpu
_GUARD = 8                    # floats in front of an output (32 bytes: keeps the 16-byte alignment of packed rows) and behind it
_FIELDS, _RESULT = {}, {}
KIND = {"valu": (False, "fp32"), "fp32": (True, "fp32"), "f16x2": (True, "f16x2"), "f16": (True, "f16")}


def _field(dev, c, family):
    from uncertainty_nerf_gs_amd import ops
    nt = c.net
    key = (nt.name, c.mode, c.K, c.p, c.sites, c.seed)
    if key not in _FIELDS:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        out1 = 17 if c.mode == FC.ACTIVE else 16
        tcnn = nt.layout != "torch"
        _FIELDS[key] = ops.FieldDev.from_torch(
            c.mode, t(nt.table), None if tcnn else t(nt.scalings), nt.log2T, t(nt.w0), t(nt.b0), t(nt.w1[:out1]), t(nt.b1[:out1]),
            [t(nt.h0), t(nt.h1), t(nt.h2)], [t(nt.hb0), t(nt.hb1), t(nt.hb2)], t(nt.app), dev, tcnn_levels=nt.levels,
            K=c.K, seed=c.seed, p_drop=float(c.p), drop_sites=c.sites, sh_remap=nt.sh_remap, average_init_density=FC.AVG,
            beta_min=FC.BETA_MIN, aabb=nt.aabb, grid_precision="f16" if nt.layout == "tcnn16" else "f32")
        assert _FIELDS[key].mfma16_blob is not None and _FIELDS[key].mfma_blob is not None
    use_mfma, precision = KIND[family]
    return dataclasses.replace(_FIELDS[key], use_mfma=use_mfma, precision=precision)


def _guarded(dev, n):
    buf = torch.full((_GUARD + n + _GUARD,), FC.SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    assert buf.data_ptr() % 16 == 0
    return buf


def _unguard(c, buf, n, what):
    host = buf.cpu()
    bits = host.view(torch.int32)
    assert (bits[:_GUARD] == FC.SENTINEL).all(), f"{c.name}: a float in front of {what} was written"
    assert (bits[_GUARD + n:] == FC.SENTINEL).all(), f"{c.name}: a float behind {what} was written"
    return host[_GUARD:_GUARD + n].numpy().copy()


def _keep_struct(dev, c, first_row, arrays):
    """{site bit: int32 [K, rows, 2] device tensor} -> (unerf_keep_masks, the tensors kept alive)"""
    from uncertainty_nerf_gs_amd import lib as L
    km = L.KeepMasks()
    stride = None
    for i in range(3):
        tns = arrays.get(1 << i)
        if tns is not None:
            assert tns.dtype == torch.int32 and tns.is_contiguous() and tns.shape[0] == c.K and tns.shape[2] == 2
            km.site[i] = tns.data_ptr()
            stride = tns.shape[1]
    km.pass_stride, km.sample_offset = stride, first_row
    return km, arrays


def _explicit_bits(dev, c):
    return {b: torch.from_numpy(FC.pack_bits(k).view(np.int32).copy()).to(dev) for b, k in c.keeps.items()}


def _generator_bits(dev, c, field):
    from uncertainty_nerf_gs_amd import ops
    km = ops.mc_keep_bits(field, c.off * c.S, c.N)
    return {1 << i: tns for i, tns in enumerate(km.sites()[:3]) if tns is not None}


def _launch(dev, c, family, layout="ray", iw=None, features=False, masks=None, rows=None, expect_error=False, extra_offset=0):
    """one call of unerf_field_fwd (masks: {site: bits}: unerf_field_fwd_masked) on rays `rows` of the case -> {"dens" [B,n],
    "rgb" [B,n,3], "beta" [n] | None} float32 numpy in the ray-major order, whatever the layout; guards checked"""
    from uncertainty_nerf_gs_amd import lib as L, ops
    lib, field = L.load(), _field(dev, c, family)
    r0, r1 = (0, c.R) if rows is None else rows
    R, S, B = r1 - r0, c.S, c.B
    n = R * S
    o, d, sb = (torch.from_numpy(np.ascontiguousarray(a[r0:r1])).to(dev) for a in (c.origins, c.dirs, c.sb))
    cs = field.cstruct()
    cs.image_width = c.iw if iw is None else iw
    cs.sample_major = int(layout == "planes")
    cs.packed_out = int(layout == "packed")
    dens = None if layout == "packed" else _guarded(dev, B * n)
    rgb = _guarded(dev, B * n * (4 if layout == "packed" else 3))
    aux = _guarded(dev, n) if c.mode == FC.ACTIVE else None
    feat = ops.field_gather(o, d, sb, field, c.near, c.far, spacing=c.lin) if features else None
    p = lambda tns, skip=_GUARD: None if tns is None else C.c_void_p(tns.data_ptr() + 4 * skip)
    args = [p(o, 0), p(d, 0), p(sb, 0), R, S, c.near, c.far, c.lin, c.off + r0 + extra_offset, C.byref(cs), p(feat, 0), p(dens), p(rgb), p(aux), None]
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        if masks is None:
            rc = lib.unerf_field_fwd(*args, stream)
        else:
            km, alive = _keep_struct(dev, c, r0 * S, masks)
            rc = lib.unerf_field_fwd_masked(*args, C.byref(km), stream)
    if expect_error:
        return rc
    L.check(rc, "field_fwd")
    torch.cuda.synchronize(dev)
    out = {"beta": None}
    raw_rgb = _unguard(c, rgb, rgb.numel() - 2 * _GUARD, "rgb")
    if layout == "packed":
        rows4 = raw_rgb.reshape(B, n, 4)
        out["dens"], out["rgb"] = np.ascontiguousarray(rows4[..., 0]), np.ascontiguousarray(rows4[..., 1:])
    else:
        raw_d = _unguard(c, dens, B * n, "density")
        if layout == "planes":
            out["dens"] = np.ascontiguousarray(raw_d.reshape(B, S, R).transpose(0, 2, 1)).reshape(B, n)
            out["rgb"] = np.ascontiguousarray(raw_rgb.reshape(B, S, 3, R).transpose(0, 3, 1, 2)).reshape(B, n, 3)
        else:
            out["dens"], out["rgb"] = raw_d.reshape(B, n), raw_rgb.reshape(B, n, 3)
    if aux is not None:
        raw_a = _unguard(c, aux, n, "aux")
        out["beta"] = np.ascontiguousarray(raw_a.reshape(S, R).T).reshape(n) if layout == "planes" else raw_a
    return out


def _base(dev, key, family, c=None):
    """the case as it stands: its image_width, its mask source, ray-major outputs"""
    if (key, family) not in _RESULT:
        c = c or FC.case(key)
        masks = _explicit_bits(dev, c) if c.masks == "explicit" else None
        _RESULT[(key, family)] = _launch(dev, c, family, masks=masks)
    return _RESULT[(key, family)]


def _same(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("dens", "rgb", "beta"))


def _sample_rows(c, r0, r1):
    return slice(r0 * c.S, r1 * c.S)


# ------------------------------------------------------------------------------------------------ every output, every family
@pytest.mark.parametrize("key", list(FC.CASES))
def test_every_output_within_its_bound_in_every_family(dev, key):
    c = FC.case(key)
    ratios = {f: FC.hold(c, f, _base(dev, key, f)) for f in c.families}
    print(f"RATIO {key} ({c.net.name}, {'ACTIVE' if c.mode == FC.ACTIVE else 'MCDROPOUT'} K={c.K} sites={FC.site_set(c.sites)} p={c.p:g} "
          f"{c.masks}; {c.tiles} tiles{' patch' if c.patch else ''}) worst error / bound: " + " ".join(f"{f} {r:.3f}" for f, r in ratios.items()))


def test_waves_that_walk_a_second_tile(dev):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    c = FC.second_tile_case(cus)
    assert c.tiles > 4 * 3 * cus
    ratios = {f: FC.hold(c, f, _launch(dev, c, f)) for f in c.families}
    print(f"RATIO {c.name} ({c.tiles} tiles on {cus} CUs) worst error / bound: " + " ".join(f"{f} {r:.3f}" for f, r in ratios.items()))


def test_one_ray_past_the_last_counter_is_refused(dev):
    c = FC.case("H-counter-max")
    for f in c.families:
        assert _launch(dev, c, f, expect_error=True, extra_offset=1) != 0, f"{f}: (ray_offset + R) S = 2^32 + 2 was accepted"


# ---------------------------------------------------------------------------------------- bit for bit inside one family
_LAYOUT_KEYS = ["A-r1-s1", "A-r63-s1", "A-r65-s3", "A-r31-s17", "B-c32box", "B-c16box-mc", "C-twide-mc", "E-w8", "E-w9-offset", "E-w37",
                "E-w64-mc", "E-w9-lastrow", "F-k10-s7", "F-k2-s13", "G-x-s7", "H-counter-max", "I-p2^-17"]


@pytest.mark.parametrize("key", _LAYOUT_KEYS)
def test_tile_schedules_and_output_layouts_give_the_same_bits(dev, key):
    """8 x 4 pixel-patch tiles against 1-D tiles; sample-major planes (the matrix kernels write them) and packed rows against
    the ray-major outputs"""
    c = FC.case(key)
    masks = _explicit_bits(dev, c) if c.masks == "explicit" else None
    for f in c.families:
        base = _base(dev, key, f)
        if c.iw:
            assert _same(_launch(dev, c, f, iw=0, masks=masks), base), f"{f}: 1-D tiles differ from image_width = {c.iw}"
        assert _same(_launch(dev, c, f, layout="packed", masks=masks), base), f"{f}: packed rows differ"
        if f != "valu" and not FC.site_set(c.sites) & FC.HEADIN:
            assert _same(_launch(dev, c, f, layout="planes", masks=masks), base), f"{f}: sample-major planes differ"


@pytest.mark.parametrize("key", ["A-r1-s1", "A-r65-s1", "A-r31-s17", "A-r33-s48", "C-twide-mc", "D-a", "E-w8", "F-k1", "F-k8-s2", "I-p2^-17"])
def test_pregathered_features_give_the_bits_of_the_fused_lookup(dev, key):
    """exact fp32 matrix kernel, torch layout under the contraction (what unerf_field_gather is built for)"""
    c = FC.case(key)
    assert c.net.layout == "torch" and c.net.aabb is None and c.bins != "euclid"
    for layout in ("ray", "planes"):
        assert _same(_launch(dev, c, "fp32", layout=layout, features=True), _base(dev, key, "fp32")), layout


_GEN_KEYS = [k for k, s in FC.CASES.items() if s["mode"] == FC.MCDROPOUT and s["K"] > 0 and s["masks"] == "gen"
             and FC.mask_threshold(s["p"]) < 65536 and not FC.site_set(s["sites"]) & FC.HEADIN]


@pytest.mark.parametrize("key", _GEN_KEYS)
def test_explicit_masks_from_the_generator_give_the_generators_bits(dev, key):
    c = FC.case(key)
    for f in c.families:
        bits = _generator_bits(dev, c, _field(dev, c, f))
        for b, k in c.keeps.items():         # ... and they are the oracle generator's masks
            assert np.array_equal(bits[b].cpu().numpy().view(np.uint32), FC.pack_bits(k)), (f, b)
        assert _same(_launch(dev, c, f, masks=bits), _base(dev, key, f)), f"{f}: unerf_field_fwd_masked differs from the generator path"


@pytest.mark.parametrize("key", ["A-r65-s3", "A-r33-s48", "B-c16", "E-w9-offset", "E-w64-mc", "F-k3-s4", "F-k10-s7", "F-k2-s13", "G-x-s5",
                                 "G-x-s7", "H-counter-max", "C-c16wide-mc"])
def test_two_launches_split_at_a_ray_give_the_bits_of_one(dev, key):
    """ray_offset carries the mask counter (and the rows of explicit masks) across the split"""
    c = FC.case(key)
    cut = c.R // 2 + 1
    masks = _explicit_bits(dev, c) if c.masks == "explicit" else None
    for f in c.families:
        base = _base(dev, key, f)
        for r0, r1 in ((0, cut), (cut, c.R)):
            part = _launch(dev, c, f, masks=masks, rows=(r0, r1))
            rows = _sample_rows(c, r0, r1)
            want = {"dens": base["dens"][:, rows], "rgb": base["rgb"][:, rows], "beta": None if base["beta"] is None else base["beta"][rows]}
            assert _same(part, want), f"{f}: rays [{r0}, {r1}) alone differ from the whole launch"
            FC.hold(c, f, part, rows=rows)


@pytest.mark.parametrize("key", ["A-r33-s48", "B-c32box", "B-c16box-mc", "E-w9-offset", "F-k10-s7", "F-k2-s13", "G-x-s7", "I-p2^-17-s7"])
def test_ops_entry_point_gives_the_same_bits(dev, key):
    from uncertainty_nerf_gs_amd import ops
    c = FC.case(key)
    o, d, sb = (torch.from_numpy(a).to(dev) for a in (c.origins, c.dirs, c.sb))
    for f in c.families:
        field = _field(dev, c, f)
        km = None
        if c.masks == "explicit":
            bits = _explicit_bits(dev, c)
            km = ops.KeepMasks(bits.get(1), bits.get(2), bits.get(4), None, c.N, 0)
        dens, rgb, aux, _ = ops.field_fwd(o, d, sb, field, c.near, c.far, ray_offset=c.off, image_width=c.iw,
                                          euclidean_bins=c.bins == "euclid", spacing=c.lin, keep_masks=km)
        got = {"dens": dens.cpu().numpy().reshape(c.B, c.N), "rgb": rgb.cpu().numpy().reshape(c.B, c.N, 3),
               "beta": None if aux is None else aux.cpu().numpy().reshape(c.N)}
        assert _same(got, _base(dev, key, f)), f


# ------------------------------------------------------------------------------------------------------ across the passes
@pytest.mark.parametrize("key", ["F-k3-p0", "I-p2^-17", "I-p2^-17-s7"])
def test_passes_without_masks_are_identical(dev, key):
    c = FC.case(key)
    assert c.B > 1 and not c.keeps
    for f in c.families:
        out = _base(dev, key, f)
        for k in range(1, c.B):
            assert np.array_equal(out["dens"][k], out["dens"][0]) and np.array_equal(out["rgb"][k], out["rgb"][0]), (f, k)


def test_no_dropout_is_one_pass_of_the_same_network(dev):
    """K = 0 and K = 3 at p_drop = 0 run the same network on the same rays: the same bits in every pass"""
    three = FC.case("F-k3-p0")
    one = SimpleNamespace(**{**vars(three), "K": 0, "B": 1, "name": "F-k3-p0 at K = 0"})
    for f in three.families:
        a, b = _launch(dev, one, f), _base(dev, "F-k3-p0", f)
        assert np.array_equal(a["dens"][0], b["dens"][0]) and np.array_equal(a["rgb"][0], b["rgb"][0]), f


@pytest.mark.parametrize("key", ["F-k3-s4", "F-k8-s2"])
def test_sites_without_the_trunk_leave_the_density_alone(dev, key):
    c = FC.case(key)
    assert not FC.site_set(c.sites) & FC.TRUNK and c.keeps
    for f in c.families:
        out = _base(dev, key, f)
        for k in range(1, c.B):
            assert np.array_equal(out["dens"][k], out["dens"][0]), (f, k)
        assert any(not np.array_equal(out["rgb"][k], out["rgb"][0]) for k in range(1, c.B)), f"{f}: the masks change no colour"
