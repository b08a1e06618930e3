"""The LAPLACE field kernels behind unerf_field_fwd on the hand-placed cases of tests/laplace_cases.py: field_kernel<LAPLACE>
(VALU), field_kernel_mfma_laplace<false> (exact fp32 matrix kernel) and field_kernel_mfma16_laplace in its split ("f16x2") and
its single-product ("f16") form.  The mean and the variance of both sampled heads are held, output by output, to a float64
reference under a derived bound that scales with the sample's own second moment: no output is exempt, the colour variance
must be >= 0, and under lap_mask_density the density is exactly mu sel and its variance exactly 0.

What the cases aim at (laplace_cases.py lists and checks them): n_lap on every edge of the split kernels' padding-quad skip
(multiples of 4 and 8 inside a row block, the block borders 32 / 64 / 96, 1 and 128), n_lap = 129 (the VALU fall-back, and the
single-f16 request refused), n_lap_rgb != n_lap; R in {1, 31, 32, 33, 65}, S in {1, 2, 3, 17, 48}, R S in {1, 63, 64, 65}, 1 to
96 tiles and more tiles than 4 x the grid; image widths 8 and 9; per-chunk sample sets of 32, 64 and 96 rays with a ray offset,
a ragged last chunk and set borders inside a VALU wave; exp and softplus; planted logits; sets whose sums are exactly known,
so that a padded row which contributes anything shows in the last bit.  Every launch goes through the C ABI; each output
sits between guard floats, and output and guards hold a NaN payload before the launch.

Bounds: laplace_cases.py states and derives them; none comes from a kernel.  Every test prints its worst error / bound
(DESIGN.md section 6.1.1 records them)."""
import ctypes as C
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import laplace_cases as LC

pytestmark = pytest.mark.gpu
_GUARD = 8
_FIELDS, _RESULT = {}, {}
KIND = {"valu": (False, "fp32"), "fp32": (True, "fp32"), "f16x2": (True, "f16x2"), "f16": (True, "f16")}


def _field(dev, c, family):
    from uncertainty_nerf_gs_amd import lib as L, ops
    nt = c.net
    if c.name not in _FIELDS:
        assert bool(L.load().unerf_build_flags() & L.BUILD_LAP_EXP2) == LC.EXP2_ROWS, "laplace_cases.EXP2_ROWS states another build"
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        tcnn = nt.layout != "torch"
        stacked = c.chunk > 0
        _FIELDS[c.name] = ops.FieldDev.from_torch(
            L.FIELD_LAPLACE, t(nt.table), None if tcnn else t(nt.scalings), nt.log2T, t(nt.w0), t(nt.b0), t(nt.w1), t(nt.b1),
            [t(nt.h0), t(nt.h1), t(nt.cmean[:192].reshape(3, 64))], [t(nt.hb0), t(nt.hb1), t(nt.cmean[192:])], torch.zeros(0), dev,
            tcnn_levels=nt.levels, sh_remap=nt.sh_remap, aabb=nt.aabb, grid_precision="f16" if nt.layout == "tcnn16" else "f32",
            ws_density=t(c.wsd if stacked else c.wsd[0]), ws_rgb=t(c.wsr if stacked else c.wsr[0]), lap_softplus=int(c.act == "softplus"),
            lap_mask_density=c.mask, lap_chunk_rays=c.chunk)
        f = _FIELDS[c.name]
        assert f.mfma16_blob is not None and f.mfma_blob is not None
        fits = max(c.n, c.wsr.shape[1]) <= LC.LAP_ROWS
        assert (f.lap_blob is not None) == fits and (f.lap16_blob is not None) == (fits and c.ws != "planted-pad")
    use_mfma, precision = KIND[family]
    return dataclasses.replace(_FIELDS[c.name], use_mfma=use_mfma, precision=precision)


def _guarded(dev, n):
    buf = torch.full((_GUARD + n + _GUARD,), LC.SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    assert buf.data_ptr() % 16 == 0
    return buf


def _unguard(c, buf, n, what):
    host = buf.cpu()
    bits = host.view(torch.int32)
    assert (bits[:_GUARD] == LC.SENTINEL).all(), f"{c.name}: a float in front of {what} was written"
    assert (bits[_GUARD + n:] == LC.SENTINEL).all(), f"{c.name}: a float behind {what} was written"
    return host[_GUARD:_GUARD + n].numpy().copy()


def _launch(dev, c, family, iw=None, rows=None, expect_error=False, f16_single=None):
    """one call of unerf_field_fwd on rays `rows` of the case -> {"dens", "var_d", "var_rgb" [n], "rgb" [n,3]} float32 numpy;
    guards checked, and the single-f16 kernel's overflow flag still 0"""
    from uncertainty_nerf_gs_amd import lib as L
    lib, field = L.load(), _field(dev, c, family)
    r0, r1 = (0, c.R) if rows is None else rows
    R, S = r1 - r0, c.S
    n = R * S
    o, d, sb = (torch.from_numpy(np.ascontiguousarray(a[r0:r1])).to(dev) for a in (c.origins, c.dirs, c.sb))
    cs = field.cstruct()
    cs.image_width = c.iw if iw is None else iw
    cs.n_lap_rgb = c.nr
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    cs.overflow_flag = flag.data_ptr()
    if f16_single is not None:
        cs.f16_single = f16_single
    dens, rgb, aux, aux2 = _guarded(dev, n), _guarded(dev, 3 * n), _guarded(dev, n), _guarded(dev, n)
    p = lambda tns, skip=_GUARD: C.c_void_p(tns.data_ptr() + 4 * skip)
    with torch.cuda.device(dev):
        rc = lib.unerf_field_fwd(p(o, 0), p(d, 0), p(sb, 0), R, S, c.near, c.far, c.lin, c.off + r0, C.byref(cs), None, p(dens), p(rgb), p(aux),
                                 p(aux2), torch.cuda.current_stream().cuda_stream)
    if expect_error:
        return rc
    L.check(rc, "field_fwd")
    torch.cuda.synchronize(dev)
    assert int(flag.item()) == 0, f"{c.name} {family}: overflow_flag set"
    return {"dens": _unguard(c, dens, n, "density"), "rgb": _unguard(c, rgb, 3 * n, "rgb").reshape(n, 3), "var_d": _unguard(c, aux, n, "aux"),
            "var_rgb": _unguard(c, aux2, n, "aux2")}


def _base(dev, key, family):
    if (key, family) not in _RESULT:
        _RESULT[(key, family)] = _launch(dev, LC.case(key), family)
    return _RESULT[(key, family)]


def _same(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("dens", "rgb", "var_d", "var_rgb"))


# ------------------------------------------------------------------------------------------------ every output, every family
@pytest.mark.parametrize("key", list(LC.CASES))
def test_every_moment_within_its_bound_in_every_family(dev, key):
    c = LC.case(key)
    ratios = {f: LC.hold(c, f, _base(dev, key, f)) for f in c.families}
    print(f"RATIO {key} ({c.net.name}, n_lap {c.n}/{c.nr} {c.ws} {c.act}{' masked' if c.mask else ''}, {c.sets} sets of {c.chunk}; {c.tiles} tiles"
          f"{' patch' if c.patch else ''}) worst error / bound: " + " ".join(f"{f} {r:.3f}" for f, r in ratios.items()))


def test_waves_that_walk_a_second_tile(dev):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    c = LC.second_tile_case(cus)
    assert c.tiles > 4 * 3 * cus
    ratios = {f: LC.hold(c, f, _launch(dev, c, f)) for f in c.families}
    print(f"RATIO {c.name} ({c.tiles} tiles on {cus} CUs) worst error / bound: " + " ".join(f"{f} {r:.3f}" for f, r in ratios.items()))


def test_129_rows_fall_back_to_the_valu_kernel_and_single_f16_is_refused(dev):
    """the heads no longer fit the blobs: the fp32 and f16x2 requests give the VALU kernel's bits (held above), the single-f16
    request is refused with its error"""
    from uncertainty_nerf_gs_amd import lib as L
    c = LC.case("N-129")
    assert c.families == ("valu", "fp32", "f16x2")
    for f in ("fp32", "f16x2"):
        assert _same(_base(dev, "N-129", f), _base(dev, "N-129", "valu")), f"{f}: not the VALU kernel's bits"
    assert _launch(dev, c, "f16x2", expect_error=True, f16_single=1) != 0, "f16_single with 129 rows was accepted"
    assert "f16_single needs" in L.load().unerf_last_error().decode()


# ---------------------------------------------------------------------------------------- bit for bit inside one family
@pytest.mark.parametrize("key", ["E-w8", "E-w9-offset"])
def test_pixel_patch_tiles_give_the_bits_of_1d_tiles(dev, key):
    c = LC.case(key)
    assert c.patch
    for f in c.families:
        assert _same(_launch(dev, c, f, iw=0), _base(dev, key, f)), f"{f}: 1-D tiles differ from image_width = {c.iw}"


@pytest.mark.parametrize("key", ["C-32-s1", "C-32-s3", "C-64-s3", "C-96-s1", "C-96-s48", "M-chunks", "A-r65-s3"])
def test_two_launches_split_at_a_chunk_border_give_the_bits_of_one(dev, key):
    """ray_offset carries the sample-set index across the split (a multiple of 32 rays, as the entry point asks)"""
    c = LC.case(key)
    cut = 32
    for f in c.families:
        base = _base(dev, key, f)
        for r0, r1 in ((0, cut), (cut, c.R)):
            part = _launch(dev, c, f, rows=(r0, r1))
            rows = slice(r0 * c.S, r1 * c.S)
            assert _same(part, {k: v[rows] for k, v in base.items()}), f"{f}: rays [{r0}, {r1}) alone differ from the whole launch"
            LC.hold(c, f, part, rows=rows)


def test_rays_past_the_last_set_and_an_offset_inside_a_tile_are_refused(dev):
    c = LC.case("C-64-s3")
    for f in c.families:
        field = _field(dev, c, f)
        assert field.ws_density.shape[0] == c.sets
    past = SimpleNamespace(**{**vars(c), "off": c.off + c.chunk})
    inside = SimpleNamespace(**{**vars(c), "off": c.off + 8})
    for f in c.families:
        assert _launch(dev, past, f, expect_error=True) != 0, f"{f}: rays past the last sample set were accepted"
        assert _launch(dev, inside, f, expect_error=True) != 0, f"{f}: a ray_offset that is no multiple of 32 was accepted"


# ------------------------------------------------------------------------------------------------------ Part 2: the GGN fit
# unerf_laplace_ggn_diag = field_kernel_mfma_laplace<true> + laplace_ggn_kernel + laplace_ggn_reduce_kernel on the cases of
# laplace_cases.GGN_CASES: S in {1, 2, 17, 63, 64}, R in {1, 3, 4, 5, 35} and 4099 (more rays than the 4096 waves of the capped
# grid), the last-sample, none and constant backgrounds (one constant outside [0, 1]: the clamp gate removes channels), exp and
# softplus, both spacings, the three grid layouts.  The ggn_* outputs sit between guard floats and start from non-zero values.
_GGN_FIELDS, _GGN_START = {}, {}


def _ggn_field(dev, c):
    from uncertainty_nerf_gs_amd import lib as L, ops
    nt = c.net
    key = (nt.name, c.act)
    if key not in _GGN_FIELDS:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        tcnn = nt.layout != "torch"
        _GGN_FIELDS[key] = ops.FieldDev.from_torch(
            L.FIELD_LAPLACE, t(nt.table), None if tcnn else t(nt.scalings), nt.log2T, t(nt.w0), t(nt.b0), t(nt.w1), t(nt.b1),
            [t(nt.h0), t(nt.h1), t(nt.cmean[:192].reshape(3, 64))], [t(nt.hb0), t(nt.hb1), t(nt.cmean[192:])], torch.zeros(0), dev,
            tcnn_levels=nt.levels, sh_remap=nt.sh_remap, aabb=nt.aabb, grid_precision="f16" if nt.layout == "tcnn16" else "f32",
            ws_density=t(nt.dmean[None]), ws_rgb=t(nt.cmean[None]), lap_softplus=int(c.act == "softplus"))
    return _GGN_FIELDS[key]


def _ggn_start(n, seed, scale):
    return (np.random.default_rng(seed).uniform(0.5, 2.0, n) * scale).astype(np.float32)


def _ggn_launch(dev, c, calls=1, S=None, short_by=0, expect_error=False, start_scale=1.0):
    """`calls` calls of unerf_laplace_ggn_diag in a row on ggn_* buffers that start from _ggn_start (non-zero: the entry point
    adds) -> ({"d", "r"}: what the calls added, float64, the final buffers, float32, the start values); guards checked"""
    from uncertainty_nerf_gs_amd import lib as L
    lib, field = L.load(), _ggn_field(dev, c)
    S = c.S if S is None else S
    o, d = (torch.from_numpy(a).to(dev) for a in (c.origins, c.dirs))
    sb = torch.from_numpy(c.sb if S == c.S else np.sort(np.random.default_rng(1).uniform(0, 1, (c.R, S + 1)), axis=1).astype(np.float32)).to(dev)
    dm, rm = torch.from_numpy(c.net.dmean).to(dev), torch.from_numpy(c.net.cmean).to(dev)
    cs = field.cstruct()
    cs.ws_density, cs.ws_rgb, cs.n_lap, cs.n_lap_rgb, cs.lap_chunk_rays, cs.lap_sets = dm.data_ptr(), rm.data_ptr(), 1, 1, 0, 1
    cs.mfma_blob = field.mfma_blob.data_ptr()
    nbytes = lib.unerf_laplace_ggn_workspace_bytes(c.R, S)
    if S == c.S:
        assert nbytes == 4 * LC.ggn_workspace_floats(c.R, c.S)
    ws = torch.zeros((nbytes + 3) // 4 + _GUARD, device=dev, dtype=torch.float32)
    start = {"d": _ggn_start(65, 11, start_scale), "r": _ggn_start(195, 12, start_scale)}
    bufs = {}
    for key, n in (("d", 65), ("r", 195)):
        bufs[key] = _guarded(dev, n)
        bufs[key][_GUARD:_GUARD + n] = torch.from_numpy(start[key]).to(dev)
    mode, rgb = c.bg
    bg_rgb = None if rgb is None else (C.c_float * 3)(*rgb)
    p = lambda tns, skip=0: C.c_void_p(tns.data_ptr() + 4 * skip)
    rc = 0
    with torch.cuda.device(dev):
        for _ in range(calls):
            rc = rc or lib.unerf_laplace_ggn_diag(p(o), p(d), p(sb), c.R, S, c.near, c.far, c.lin, C.byref(cs), mode, bg_rgb, p(ws), nbytes - short_by,
                                                  p(bufs["d"], _GUARD), p(bufs["r"], _GUARD), torch.cuda.current_stream().cuda_stream)
    if expect_error:
        return rc
    L.check(rc, "laplace_ggn_diag")
    torch.cuda.synchronize(dev)
    final = {key: _unguard(c, bufs[key], n, f"ggn_{key}") for key, n in (("d", 65), ("r", 195))}
    return {k: final[k].astype(np.float64) - start[k] for k in final}, final, start


@pytest.mark.parametrize("key", list(LC.GGN_CASES))
def test_ggn_diagonal_within_its_bound(dev, key):
    """what one call adds to the buffers, entry by entry.  The buffers start from about 2^-60, non-zero and far below
    every bound, so that the sum's own rounding, U (start + entry), stays a small part of the bound it is added to"""
    c = LC.ggn_case(key)
    added, final, start = _ggn_launch(dev, c, start_scale=2.0 ** -60)
    worst = 0.0
    for k, ref, b in (("d", c.ref.d, c.ref.b_d), ("r", c.ref.r, c.ref.b_r)):
        assert np.isfinite(final[k]).all()
        err = np.abs(added[k] - ref)
        bound = LC.GGN_FACTOR * b + LC.U * (start[k] + ref)
        bad = np.flatnonzero(~(err <= bound))
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.where(err == 0, 0.0, err / bound).max()))
        assert len(bad) == 0, f"{key}: {len(bad)} entries of ggn_{k} beyond their bound, first {bad[:6].tolist()}, worst error / bound {worst:.3g}"
    print(f"RATIO {key} ({c.net.name}, bg {c.bg}, {c.act}, {c.bins}, {LC.ggn_waves(c.R)} waves) worst error / bound: {worst:.3f}")


@pytest.mark.parametrize("key", ["G-r5-s63-clamp", "G-r35-s64-last-sp", "G-r4099-s2"])
def test_two_ggn_calls_add_twice_the_single_result(dev, key):
    """the fit accumulates over batches: a second call on the buffers adds the same entries again (the partial sums are
    reduced in a fixed order, so the two contributions are the same float32 numbers)"""
    c = LC.ggn_case(key)
    once, f1, start = _ggn_launch(dev, c)
    twice, f2, _ = _ggn_launch(dev, c, calls=2)
    for k in ("d", "r"):
        sum1 = f1[k].astype(np.float64) - start[k]                   # the rounded single contribution, to U (start + entry)
        tol = 4 * LC.U * (start[k] + 2 * np.abs(sum1))
        assert (np.abs(twice[k] - 2 * once[k]) <= tol).all(), (k, float(np.abs(twice[k] - 2 * once[k]).max()))


def test_ggn_refuses_65_samples_and_a_short_workspace(dev):
    from uncertainty_nerf_gs_amd import lib as L
    c = LC.ggn_case("G-r5-s63-clamp")
    assert _ggn_launch(dev, c, S=65, expect_error=True) != 0, "S = 65 was accepted"
    assert "outside [1,64]" in L.load().unerf_last_error().decode()
    assert _ggn_launch(dev, c, short_by=4, expect_error=True) != 0, "a workspace 4 bytes short was accepted"
    assert "workspace" in L.load().unerf_last_error().decode()
    added, _, _ = _ggn_launch(dev, c, S=64)            # ... and 64 samples of the same rays run
    assert np.isfinite(added["d"]).all() and np.isfinite(added["r"]).all()
