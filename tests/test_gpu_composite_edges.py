"""The compositing kernels (composite_kernel* / composite_moments_kernel* behind ops.composite_var / composite_moments,
composite_sm_kernel behind the *_planes calls, lap_depth_kernel, moments_kernel) on the hand-placed cases of
tests/composite_cases.py, held to a float64 reference on EVERY channel of every ray: no share of values is exempt, and no kernel is
compared only with another kernel (where two forms must agree bit for bit -- packed and plain rows, the views call and the single
call -- that comes on top of the float64 hold).

What the cases aim at: S from the dispatch table (every SPL aligned and RAGGED, S = 1, S = 129 with seven wholly masked lanes,
S = 80 / 112 whose own SPL does not exist), B R = 111 groups (blocks straddle passes, a clamped group in the last block), R = 300
for the planes (a full block, then 44 lanes), B on both sides of the planes kernel's 4-pass walk and up to the group kernel's 16,
clip rows that change inside a block with one row narrowed, planted rays (all zero, opaque tail, inf, NaN density, NaN colour, both
clamps, all weight in the last real sample, the median on the first / last slot of a lane), every background, an exact family bit
for bit, guard rows behind every output, the nonfinite flag, D odd and even for the depth draws, K around the moments unroll.

Bounds: composite_cases.py states and derives them; none comes from a kernel.  Every test prints its worst error / bound
(DESIGN.md section 6.1 records them)."""
import ctypes as C

import pytest
import torch

import composite_cases as CC

pytestmark = pytest.mark.gpu
_SENTINEL = 0x7FC0BEEF        # a NaN with a payload: no result has this bit pattern
_REPORT = "RATIO"


def _views(c):
    from uncertainty_nerf_gs_amd import ops
    return ops.RayViews(CC.N_VIEWS, c.rays_per_view) if c.views else None


def _kw(c, dev):
    from uncertainty_nerf_gs_amd import ops
    kw = dict(clip_minmax=c.clip.to(dev), chunk_rays=CC.CHUNK, spacing=c.spacing, background=ops.background_of(c.bg))
    if c.views:
        kw["views"] = _views(c)
    else:
        kw["ray_offset"] = CC.OFFSET
    return kw


def _packed(c, dev):
    return torch.cat([c.dens[..., None], c.rgb], dim=-1).contiguous().to(dev)


def _opt(t, dev):
    return None if t is None else t.to(dev)


def _composite_var(dev, c, packed=False, repeat=1, **extra):
    from uncertainty_nerf_gs_amd import ops
    dens, rgb = (None, _packed(c, dev)) if packed else (c.dens.to(dev), c.rgb.to(dev))
    if repeat > 1:      # the same pass `repeat` times: [B,R,S] -> [repeat B,R,S]
        dens, rgb = dens.repeat(repeat, 1, 1), rgb.repeat(repeat, 1, 1, 1)
    return ops.composite_var(dens, rgb, c.sb.to(dev), c.near, c.far, beta=_opt(c.beta, dev), weights_alt=_opt(c.walt, dev),
                             **_kw(c, dev), **extra).cpu()


def _hold_passes(key, c, out):
    worst = {k: 0.0 for k in CC.CHANNELS}
    assert out.shape == (c.B, c.R, 8)
    for b in range(c.B):
        for k, v in CC.hold(f"{key} pass {b}", c.refs[b], out[b], expect=c.expect if c.family == "exact" else None).items():
            worst[k] = max(worst[k], v)
    return worst


def _fmt(r):
    return " ".join(f"{k} {v:.3f}" for k, v in r.items())


@pytest.mark.parametrize("key", list({**CC.COMPOSITE, **CC.EXACT}))
def test_composite_var_every_channel_within_its_bound(dev, key):
    c = {**CC.COMPOSITE, **CC.EXACT}[key]()
    out = _composite_var(dev, c)
    print(f"{_REPORT} composite_var {key}: SPL {c.spl} ragged {c.ragged} B {c.B} worst error / bound: {_fmt(_hold_passes(key, c, out))}")
    if c.family == "exact":      # ... and as three passes (B R = 3 R groups)
        for b, o in enumerate(_composite_var(dev, c, repeat=3)):
            CC.hold(f"{key} pass {b} of 3", c.refs[0], o, expect=c.expect)


@pytest.mark.parametrize("key", [k for k, f in CC.COMPOSITE.items() if k.endswith("-B3") and k[0] == "S" and CC.packed_pair(int(k[1:-3]))])
def test_composite_var_packed_rows(dev, key):
    """density=None, rows (sigma, r, g, b): held against the reference, and the same bits as the unpacked call"""
    c = CC.COMPOSITE[key]()
    out = _composite_var(dev, c, packed=True)
    print(f"{_REPORT} composite_var packed {key}: SPL {c.spl} ragged {c.ragged} worst error / bound: {_fmt(_hold_passes(key, c, out))}")
    assert torch.equal(out.view(torch.int32), _composite_var(dev, c).view(torch.int32))


@pytest.mark.parametrize("key", list(CC.ALT))
def test_composite_var_weights_alt(dev, key):
    """the depth-side channels from weights_alt as given: an alt row summing below 0.5 (the median clamps to S - 1), one reaching
    0.5 at slot 0 (`< 0.5` and `<= 0.5` part there)"""
    c = CC.ALT[key]()
    out = _composite_var(dev, c)
    print(f"{_REPORT} composite_var weights_alt {key}: worst error / bound: {_fmt(_hold_passes(key, c, out))}")
    _, steps = CC.geometry(c.sb, c.near, c.far, c.spacing)
    assert out[0, 10, 4] == steps[10, -1] and out[0, 11, 4] == steps[11, 0]


def _moments(dev, c, packed=False):
    from uncertainty_nerf_gs_amd import ops
    dens, rgb = (None, _packed(c, dev)) if packed else (c.dens.to(dev), c.rgb.to(dev))
    mean, var = ops.composite_moments(dens, rgb, c.sb.to(dev), c.near, c.far, **_kw(c, dev))
    return mean.cpu(), var.cpu()


@pytest.mark.parametrize("key", list(CC.MOMENTS))
def test_composite_moments_against_the_float64_pass_moments(dev, key):
    """plain and packed rows; ray 9 is all zero in pass 0 and opaque in the others (the largest spread around pass 0)"""
    c = CC.MOMENTS[key]()
    mr = CC.moments_reference(CC.refs_without_beta(c))
    mean, var = _moments(dev, c)
    rm, rv = CC.hold_moments(key, mr, mean, var)
    print(f"{_REPORT} composite_moments {key}: SPL {c.spl} ragged {c.ragged} worst error / bound: mean {rm:.3f} variance {rv:.3f}")
    pm, pv = _moments(dev, c, packed=True)
    CC.hold_moments(key + " packed", mr, pm, pv)
    assert torch.equal(pm.view(torch.int32), mean.view(torch.int32)) and torch.equal(pv.view(torch.int32), var.view(torch.int32))


def test_composite_moments_refuses_17_passes(dev):
    from uncertainty_nerf_gs_amd import lib as L, ops
    c = CC.toleranced(17, 3, "white")
    dens, rgb = c.dens[:1].expand(17, -1, -1).contiguous().to(dev), c.rgb[:1].expand(17, -1, -1, -1).contiguous().to(dev)
    with pytest.raises(L.UnerfError, match="B=17"):
        ops.composite_moments(dens, rgb, c.sb.to(dev), c.near, c.far)


def _planes(c, dev):
    dp = c.dens.permute(0, 2, 1).contiguous().to(dev)               # [B,S,R]
    cp = c.rgb.permute(0, 2, 3, 1).contiguous().to(dev)             # [B,S,3,R]
    bp = None if c.beta is None else c.beta.t().contiguous().to(dev)
    return dp, cp, bp


@pytest.mark.parametrize("key", list(CC.PLANES))
def test_planes_kernels_every_channel_and_the_pass_moments(dev, key):
    """composite_var_planes per pass (depth variance held on every ray) and composite_moments_planes, R = 300"""
    from uncertainty_nerf_gs_amd import ops
    c = CC.PLANES[key]()
    dp, cp, bp = _planes(c, dev)
    out = ops.composite_var_planes(dp, cp, c.sb.to(dev), c.near, c.far, beta=bp, **_kw(c, dev)).cpu()
    r = _hold_passes(key, c, out)
    mean, var = ops.composite_moments_planes(dp, cp, c.sb.to(dev), c.near, c.far, **_kw(c, dev))
    rm, rv = CC.hold_moments(key, CC.moments_reference(CC.refs_without_beta(c)), mean.cpu(), var.cpu())
    print(f"{_REPORT} planes {key}: B {c.B} worst error / bound: {_fmt(r)} | moments: mean {rm:.3f} variance {rv:.3f}")


@pytest.mark.parametrize("key", [k for k in CC.EXACT if k.endswith("last_sample") or k.endswith("white")])
def test_planes_kernel_exact_family(dev, key):
    from uncertainty_nerf_gs_amd import ops
    c = CC.EXACT[key]()
    dp, cp, bp = _planes(c, dev)
    out = ops.composite_var_planes(dp, cp, c.sb.to(dev), c.near, c.far, beta=bp, **_kw(c, dev)).cpu()
    _hold_passes(key, c, out)


def test_planes_moments_refuse_one_pass(dev):
    from uncertainty_nerf_gs_amd import lib as L, ops
    c = CC.toleranced(17, 1, "white")
    dp, cp, _ = _planes(c, dev)
    with pytest.raises(L.UnerfError, match="B=1"):
        ops.composite_moments_planes(dp, cp, c.sb.to(dev), c.near, c.far)


@pytest.mark.parametrize("key", list(CC.VIEWS))
def test_views_calls_number_the_clip_rows_per_view(dev, key):
    """3 views x 37 rays, 10 rays per chunk: 4 clip rows per view, the last one short, every row with its own narrowed values"""
    from uncertainty_nerf_gs_amd import ops
    c = CC.VIEWS[key]()
    assert ops.clip_rows_per_view(c.rays_per_view, CC.CHUNK) == 4 and c.clip.shape[0] == 12 and len({tuple(r) for r in c.clip.tolist()}) == 12
    out = _composite_var(dev, c)
    r = _hold_passes(key, c, out)
    packed = _composite_var(dev, c, packed=True)
    assert torch.equal(packed.view(torch.int32), out.view(torch.int32))
    mr = CC.moments_reference(CC.refs_without_beta(c))
    mean, var = _moments(dev, c)
    rm, rv = CC.hold_moments(key, mr, mean, var)
    pm, pv = _moments(dev, c, packed=True)
    assert torch.equal(pm.view(torch.int32), mean.view(torch.int32)) and torch.equal(pv.view(torch.int32), var.view(torch.int32))
    print(f"{_REPORT} views {key}: worst error / bound: {_fmt(r)} | moments: mean {rm:.3f} variance {rv:.3f}")


def test_views_calls_refuse_one_view_too_many(dev):
    from uncertainty_nerf_gs_amd import lib as L, ops
    n = L.NERF_MAX_VIEWS + 1
    c = CC.toleranced(17, 1, "white")
    dens, rgb, sb = (t[:, :n] if t.dim() > 2 else t[:n] for t in (c.dens, c.rgb, c.sb))
    clip = torch.zeros(n, 2)
    for call in (ops.composite_var, ops.composite_moments):
        with pytest.raises(L.UnerfError):
            call(dens.contiguous().to(dev), rgb.contiguous().to(dev), sb.contiguous().to(dev), c.near, c.far, clip_minmax=clip.to(dev),
                 chunk_rays=CC.CHUNK, views=ops.RayViews(n, 1))


def _guard(rows, dev):
    return torch.full((rows + 2, 8), _SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def _untouched(buf, rows, what):
    assert (buf[rows:].view(torch.int32) == _SENTINEL).all(), f"{what}: a row past the last one was written"
    assert not (buf[:rows].view(torch.int32) == _SENTINEL).all(dim=-1).any(), f"{what}: a row was not written"


@pytest.mark.parametrize("key", ["S17-B3", "S129-B3", "S256-B3", "S1-B3"])
def test_group_kernels_write_nothing_behind_their_outputs(dev, key):
    """the C ABI as ops calls it, on output buffers two rows longer than [B,R,8] / [R,8] and filled with a sentinel.  B R = 111:
    the last block's 16th group is clamped to group G - 1 with its store off"""
    from uncertainty_nerf_gs_amd import lib as L, ops
    lib, c = L.load(), CC.COMPOSITE[key]()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    dens, rgb, beta, sb, clip = (t.contiguous().to(dev) for t in (c.dens, c.rgb, c.beta, c.sb, c.clip))
    mode, bg = ops._background(ops.background_of(c.bg))
    out, mean, var = _guard(c.B * c.R, dev), _guard(c.R, dev), _guard(c.R, dev)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream().cuda_stream
        L.check(lib.unerf_composite_var(p(dens), p(rgb), p(beta), None, p(sb), c.B, c.R, c.S, c.near, c.far, c.spacing, p(clip),
                                        CC.OFFSET, CC.CHUNK, mode, bg, None, p(out), st), "composite_var")
        L.check(lib.unerf_composite_moments(p(dens), p(rgb), p(sb), c.B, c.R, c.S, c.near, c.far, c.spacing, p(clip), CC.OFFSET,
                                            CC.CHUNK, mode, bg, None, p(mean), p(var), st), "composite_moments")
    out, mean, var = out.cpu(), mean.cpu(), var.cpu()
    for buf, rows, what in ((out, c.B * c.R, "composite_var"), (mean, c.R, "moments mean"), (var, c.R, "moments variance")):
        _untouched(buf, rows, what)
    _hold_passes(key, c, out[:c.B * c.R].reshape(c.B, c.R, 8))
    CC.hold_moments(key, CC.moments_reference(CC.refs_without_beta(c)), mean[:c.R], var[:c.R])


@pytest.mark.parametrize("key", ["planes-S17-B5", "planes-S1-B2"])
def test_planes_kernels_write_nothing_behind_their_outputs(dev, key):
    from uncertainty_nerf_gs_amd import lib as L, ops
    lib, c = L.load(), CC.PLANES[key]()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    dp, cp, bp = _planes(c, dev)
    sb, clip = c.sb.to(dev), c.clip.to(dev)
    mode, bg = ops._background(ops.background_of(c.bg))
    out, mean, var = _guard(c.B * c.R, dev), _guard(c.R, dev), _guard(c.R, dev)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream().cuda_stream
        L.check(lib.unerf_composite_var_planes(p(dp), p(cp), p(bp), p(sb), c.B, c.R, c.S, c.near, c.far, c.spacing, p(clip), CC.OFFSET,
                                               CC.CHUNK, mode, bg, None, p(out), st), "composite_var_planes")
        L.check(lib.unerf_composite_moments_planes(p(dp), p(cp), p(sb), c.B, c.R, c.S, c.near, c.far, c.spacing, p(clip), CC.OFFSET,
                                                   CC.CHUNK, mode, bg, None, p(mean), p(var), st), "composite_moments_planes")
    out, mean, var = out.cpu(), mean.cpu(), var.cpu()
    for buf, rows, what in ((out, c.B * c.R, "composite_var_planes"), (mean, c.R, "moments mean"), (var, c.R, "moments variance")):
        _untouched(buf, rows, what)
    _hold_passes(key, c, out[:c.B * c.R].reshape(c.B, c.R, 8))


@pytest.mark.parametrize("family", ["group", "moments", "planes", "planes_moments"])
@pytest.mark.parametrize("S", [17, 48])
def test_nonfinite_flag(dev, family, S):
    """set by the NaN-density ray and by the NaN-colour ray, each alone; not by the +inf ray, not by clean rays"""
    from uncertainty_nerf_gs_amd import ops
    c = CC.toleranced(S, 3, "last_sample")
    for rows, want in (([3], 1), ([4], 1), ([2], 0), ([0, 1, 5, 6, 7, 8, 12, 30], 0), (list(range(c.R)), 1)):
        dens, rgb, sb = c.dens[:, rows].contiguous().to(dev), c.rgb[:, rows].contiguous().to(dev), c.sb[rows].contiguous().to(dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        if family == "group":
            ops.composite_var(dens, rgb, sb, c.near, c.far, nonfinite_flag=flag)
        elif family == "moments":
            ops.composite_moments(dens, rgb, sb, c.near, c.far, nonfinite_flag=flag)
        else:
            dp, cp = dens.permute(0, 2, 1).contiguous(), rgb.permute(0, 2, 3, 1).contiguous()
            call = ops.composite_var_planes if family == "planes" else ops.composite_moments_planes
            call(dp, cp, sb, c.near, c.far, nonfinite_flag=flag)
        assert flag.item() == want, f"{family}, rays {rows}: flag {flag.item()}"


@pytest.mark.parametrize("key", list(CC.LAPLACE))
def test_laplace_depth_weights_against_float64_draws(dev, key):
    """explicit noise, D in {1, 2, 5} (the odd tail of the two-draw loop), rows with var < 0, var = 0, NaN var, NaN mu, mu = 0;
    the single call and the views call (with explicit noise the rows are launch rows in both)"""
    from uncertainty_nerf_gs_amd import ops
    c = CC.LAPLACE[key]()
    args = (c.mu.to(dev), c.var.to(dev), c.sb.to(dev), c.near, c.far, c.noise.to(dev), c.D)
    got = ops.laplace_depth_weights(*args).cpu()
    ratio = CC.hold_laplace(c, got)
    print(f"{_REPORT} laplace_depth_weights {key}: SPL {CC.spl_for(c.S)} worst error / bound {ratio:.3f}")
    rows = 36      # 3 views of 12 rays
    vargs = (c.mu[:rows].to(dev), c.var[:rows].to(dev), c.sb[:rows].to(dev), c.near, c.far, c.noise[:, :rows].contiguous().to(dev), c.D)
    vgot = ops.laplace_depth_weights(*vargs, views=ops.RayViews(3, 12)).cpu()
    CC.hold_laplace(c, vgot, slice(0, rows))
    assert torch.equal(vgot.view(torch.int32), got[:rows].view(torch.int32))


@pytest.mark.parametrize("K", CC.K_MOMENTS)
def test_moments_over_the_leading_dimension(dev, K):
    """K on both sides of the unroll of 8 (the remainder loop after a full block: 9, 17), K = 1 (NaN variance), want_var=False"""
    from uncertainty_nerf_gs_amd import ops
    c = CC.stack_moments(K)
    mean, var = ops.moments(c.x.to(dev))
    ratios = CC.hold_stack(c, mean, var)
    print(f"{_REPORT} moments K = {K}: worst error / bound {[f'{r:.3f}' for r in ratios]}")
    only, none = ops.moments(c.x.to(dev), want_var=False)
    assert none is None and torch.equal(only.view(torch.int32), mean.view(torch.int32))
