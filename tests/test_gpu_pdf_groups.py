"""The lane-group form of the PDF resampler (pdf_group_kernel<EPL> behind ops.weights_pdf_resample up to n = 128: 16 lanes per
ray, four rays per wave; above it the wave-per-ray pdf_kernel) on the cases of tests/pdf_group_cases.py, every weight, bin and
median depth held to pdf_cases' float64 reference by pdf_cases' own bounds.

What the cases aim at: n and m + 1 on both sides of every multiple of 16 and 32 (lanes past the ray's end, a ragged last
lane, an output loop that ends on a full, a one-lane and an all-but-one-lane trip), the workload's (256, 96) and (96, 48)
with and without the shared row, the median on both sides of the lane borders of the selected layout,
R that leaves one live group in a wave / all but one / a single group in a block's second trip, nothing written past R,
rays of different kinds (zero, saturated, inf, NaN mid-scan) side by side in one wave and the same bits for a ray wherever
it lands, clip rows across groups of one wave that fall into two chunks, and the views entry point at every G."""
import ctypes as C

import pytest
import torch

import pdf_cases as PC
import pdf_group_cases as GC
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu
_RESULT = {}
_SENTINEL = 0x7FC0BEEF        # a NaN with a payload: no result has this bit pattern


def _clip_buffer(rows, dev):
    clip = torch.empty(rows, 2, device=dev)
    clip[:, 0], clip[:, 1] = float("inf"), 0.0
    return clip


def _call(dev, c, rows=slice(None), chunk=5, views=None, clip_rows=None):
    """-> (new, depth, weights, clip) on the CPU, of the case's rays `rows` (a slice or an index tensor)"""
    from uncertainty_nerf_gs_amd import ops
    dens = c.dens[rows].clone().to(dev)
    sb = (c.sb if c.sb.dim() == 1 else c.sb[rows]).clone().to(dev)
    clip = _clip_buffer(clip_rows or (dens.shape[0] + chunk - 1) // chunk, dev)
    new, pd, w = ops.weights_pdf_resample(dens, sb, c.u.clone().to(dev), c.near, c.far, histogram_padding=c.pad, eps=c.eps,
                                          want_weights=True, clip_minmax=clip, ray_offset=0, chunk_rays=chunk,
                                          spacing=c.spacing, views=views)
    return new.cpu(), pd.cpu(), w.cpu(), clip.cpu()


def _whole(dev, key):
    if key not in _RESULT:
        _RESULT[key] = _call(dev, GC.ALL[key]())
    return _RESULT[key]


def _check_clip(c, new, clip, row_of):
    """clip rows == min / max of the returned bins' first / last mid-points, per chunk"""
    eb = O.spacing_to_euclidean(new, c.near, c.far, uniform=bool(c.spacing))
    first, last = (eb[:, 0] + eb[:, 1]) / 2, (eb[:, -2] + eb[:, -1]) / 2
    want = _clip_buffer(clip.shape[0], "cpu")
    for r in range(new.shape[0]):
        k = row_of(r)
        want[k, 0], want[k, 1] = min(want[k, 0], first[r]), max(want[k, 1], last[r])
    torch.testing.assert_close(clip, want, rtol=1e-6, atol=0)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("key", list(GC.ALL))
def test_every_weight_bin_and_depth_within_its_bound(dev, key):
    c = GC.ALL[key]()
    new, pd, w, clip = _whole(dev, key)
    rw, rb = PC.hold(c, w, new, pd)
    print(f"RATIO {key}: G {GC.lanes_per_ray(c.n)} EPL {GC.group_epl(c.n)} nb {c.m + 1} worst error / bound: weights {rw:.3f} bins {rb:.3f}")
    assert torch.all(new[:, 1:] >= new[:, :-1]), "bins must stay sorted"
    _check_clip(c, new, clip, lambda r: r // 5)


@pytest.mark.parametrize("key", ["plain-96-48", "plain-113-96", "plain-256-96", "shared-256-96", "shared-96-48", "mixed-47-17"])
@pytest.mark.parametrize("Rr", GC.SHORT_R)
def test_short_calls_write_nothing_past_their_last_ray(dev, key, Rr):
    """A group past the last ray re-runs ray R - 1 with its stores switched off.  The C ABI is called as ops calls it, on
    output buffers 4 rows longer than R (one clip row longer) and filled with a sentinel: those rows come back untouched,
    and the R rows hold."""
    from uncertainty_nerf_gs_amd import lib as L
    lib, c = L.load(), GC.ALL[key]()
    guard = lambda cols: torch.full((Rr + 4, cols), _SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    new, w, pd = guard(c.m + 1), guard(c.n), guard(1)
    chunk = 3
    n_clip = (Rr + chunk - 1) // chunk
    clip = _clip_buffer(n_clip + 1, dev)
    shared = c.sb.dim() == 1
    dens, u = c.dens[:Rr].clone().to(dev), c.u.clone().to(dev)
    sb = (c.sb if shared else c.sb[:Rr]).clone().to(dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        rc = lib.unerf_weights_pdf_resample(p(dens), p(sb), 0 if shared else sb.shape[1], Rr, c.n, c.near, c.far, c.spacing, p(u),
                                            c.m, c.pad, c.eps, p(new), p(pd), p(w), p(clip), 0, chunk,
                                            torch.cuda.current_stream().cuda_stream)
    L.check(rc, "weights_pdf_resample")
    new, w, pd, clip = new.cpu(), w.cpu(), pd.cpu(), clip.cpu()
    for name, buf in (("bins", new), ("weights", w), ("depth", pd)):
        assert (buf[Rr:].view(torch.int32) == _SENTINEL).all(), f"{name}: a row past R = {Rr} was written"
    assert clip[n_clip].tolist() == [float("inf"), 0.0], "a clip row past the last chunk was written"
    PC.hold(c, w[:Rr], new[:Rr], pd[:Rr], slice(0, Rr))
    _check_clip(c, new[:Rr], clip[:n_clip], lambda r: r // chunk)
    whole = _whole(dev, key)
    for x, y in zip((new, pd, w), whole[:3]):
        assert _same_bits(x[:Rr], y[:Rr]), "a ray's bits depend on how many rays the call has"


@pytest.mark.parametrize("key", list(GC.MIXED_CASES))
def test_no_leakage_between_the_rays_of_a_wave(dev, key):
    """neighbouring rays are all zero / saturated / hold an inf / feed a NaN into the scan mid-ray / random: the same rays in
    a permuted order, and in reverse, give every ray the same bits"""
    c = GC.ALL[key]()
    whole = _whole(dev, key)
    g = torch.Generator().manual_seed(5)
    for perm in (torch.randperm(GC.R, generator=g), torch.arange(GC.R - 1, -1, -1)):
        part = _call(dev, c, perm)
        for x, y in zip(part[:3], whole[:3]):
            assert _same_bits(x, y[perm])


@pytest.mark.parametrize("key", ["plain-96-48", "plain-256-96", "shared-256-96", "plain-33-17"])
@pytest.mark.parametrize("a,b", [(3, 20), (30, 37), (36, 37), (1, 34)])
def test_a_ray_does_not_depend_on_its_group_wave_or_trip(dev, key, a, b):
    whole = _whole(dev, key)
    part = _call(dev, GC.ALL[key](), slice(a, b))
    for x, y in zip(part[:3], whole[:3]):
        assert _same_bits(x, y[a:b])


@pytest.mark.parametrize("key", ["plain-96-48", "plain-256-96", "shared-256-96", "mixed-130-64", "plain-17-31"])
@pytest.mark.parametrize("chunk", [3, 5])
def test_clip_rows_when_the_groups_of_a_wave_fall_into_two_chunks(dev, key, chunk):
    c = GC.ALL[key]()
    new, pd, w, clip = _call(dev, c, chunk=chunk)
    assert clip.shape[0] == (GC.R + chunk - 1) // chunk
    _check_clip(c, new, clip, lambda r: r // chunk)
    for x, y in zip((new, pd, w), _whole(dev, key)[:3]):
        assert _same_bits(x, y), "the chunk size changed a ray's bits"


@pytest.mark.parametrize("key", ["plain-16-15", "plain-96-48", "plain-128-96", "plain-241-96", "plain-256-96", "shared-256-96"])
def test_views_entry_point_at_every_group_width(dev, key):
    """three views of 12 rays: the same bits as the plain call, the clip rows numbered inside each view (3 rows per view at 5
    rays per chunk); the keys take every G the host selects (16 up to n = 128, 64 above)"""
    from uncertainty_nerf_gs_amd import ops
    c, rows = GC.ALL[key](), slice(0, 36)
    assert ops.clip_rows_per_view(12, 5) == 3
    plain = _call(dev, c, rows)
    new, pd, w, clip = _call(dev, c, rows, views=ops.RayViews(3, 12), clip_rows=9)
    for x, y in zip((new, pd, w), plain):
        assert _same_bits(x, y)
    PC.hold(c, w, new, pd, rows)
    _check_clip(c, new, clip, lambda r: 3 * (r // 12) + (r % 12) // 5)


def test_the_view_keys_take_every_group_width_the_host_selects():
    keys = ["plain-16-15", "plain-96-48", "plain-128-96", "plain-241-96", "plain-256-96", "shared-256-96"]
    assert {GC.lanes_per_ray(GC.ALL[k]().n) for k in keys} == {GC.lanes_per_ray(n) for n in range(1, 257)}
