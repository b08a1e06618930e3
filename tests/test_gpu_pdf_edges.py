"""The PDF resampler (pdf_kernel<EPL> and pdf_kernel<EPL, ViewMap> behind ops.weights_pdf_resample) on the hand-placed cases
of tests/pdf_cases.py, held to a float64 reference on EVERY weight, bin and depth: no share of values is exempt.

What the cases aim at: n on both sides of 64 / 128 / 192 (EPL 1 .. 4, with lanes past the ray's end in each, n = 1 .. 3),
m + 1 in {2, 3, 64, 65, 66, 128, 129, 192, 256} around the 64-wide output loop, the median on the first / last element of a
lane's run and clamped to n - 1, R = 37 (a block with one live wave in its second wave-quad), sbins rows wider than n + 1, the
shared row at n = 100 / 130 / 256, the uniform spacing, a NaN that enters the prefix scan mid-ray, and -- bit for bit -- u on
the CDF's knots, on 0 and on 1.0 (the descent's clamped probe, pos = n, both index clamps, nan_to_num(0 / 0)).

Bounds (pdf_cases.py states and derives them; none comes from a kernel): weights 2 [(dd + 1) e^-dd T + (c + 2) w] 2^-23, bins
K EPS_CDF + 2^-23 with K the reference's own d bin / d cdf and EPS_CDF = 4 x the fp32 CPU chain's worst CDF error, median
depth exact except on rays whose margin is within their summed weight bounds.  Every test prints its worst error / bound
(DESIGN.md section 6.1 records them)."""
import ctypes as C

import pytest
import torch

import pdf_cases as PC
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu
CHUNK = 5
_RESULT = {}


def _clip_buffer(rows, dev):
    clip = torch.empty(rows, 2, device=dev)
    clip[:, 0], clip[:, 1] = float("inf"), 0.0
    return clip


def _call(dev, c, rows=slice(None), views=None, clip_rows=None):
    """-> (new, depth, weights, clip) on the CPU, of the case's rays `rows`"""
    from uncertainty_nerf_gs_amd import ops
    dens = c.dens[rows].clone().to(dev)
    sb = (c.sb if c.sb.dim() == 1 else c.sb[rows]).clone().to(dev)
    clip = _clip_buffer(clip_rows or (dens.shape[0] + CHUNK - 1) // CHUNK, dev)
    new, pd, w = ops.weights_pdf_resample(dens, sb, c.u.clone().to(dev), c.near, c.far, histogram_padding=c.pad, eps=c.eps,
                                          want_weights=True, clip_minmax=clip, ray_offset=0, chunk_rays=CHUNK,
                                          spacing=c.spacing, views=views)
    return new.cpu(), pd.cpu(), w.cpu(), clip.cpu()


def _whole(dev, key):
    if key not in _RESULT:
        _RESULT[key] = _call(dev, PC.ALL[key]())
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


@pytest.mark.parametrize("key", list(PC.ALL))
def test_every_weight_bin_and_depth_within_its_bound(dev, key):
    c = PC.ALL[key]()
    new, pd, w, clip = _whole(dev, key)
    rw, rb = PC.hold(c, w, new, pd)
    print(f"RATIO {key} ({c.family}): EPL {c.epl} nb {c.nb} worst error / bound: weights {rw:.3f} bins {rb:.3f}")
    assert torch.all(new[:, 1:] >= new[:, :-1]), "bins must stay sorted"
    _check_clip(c, new, clip, lambda r: r // CHUNK)


@pytest.mark.parametrize("key,epl", [("plain-63-64", 1), ("plain-127-128", 2), ("plain-191-65", 3), ("plain-256-255", 4)])
def test_views_entry_point_at_every_samples_per_lane(dev, key, epl):
    """pdf_kernel<EPL, ViewMap>, EPL 1 .. 4: three views of 12 rays (RayViews holds views of one size): same bits as the plain
    call, the clip rows numbered inside each view (3 rows per view at 5 rays per chunk)"""
    from uncertainty_nerf_gs_amd import ops
    c, rows = PC.ALL[key](), slice(0, 36)
    assert c.epl == epl and c.dens.shape[0] >= 36 and ops.clip_rows_per_view(12, CHUNK) == 3
    plain = _call(dev, c, rows)
    new, pd, w, clip = _call(dev, c, rows, views=ops.RayViews(3, 12), clip_rows=9)
    for a, b in zip((new, pd, w), plain):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    PC.hold(c, w, new, pd, rows)
    _check_clip(c, new, clip, lambda r: 3 * (r // 12) + (r % 12) // CHUNK)


_SENTINEL = 0x7FC0BEEF        # a NaN with a payload: no result has this bit pattern


@pytest.mark.parametrize("key", ["wide-130-64", "plain-63-64"])
@pytest.mark.parametrize("Rr", [1, 2, 3, 5, 33])
def test_dead_waves_write_nothing(dev, key, Rr):
    """A wave past the last ray re-runs ray R - 1 with its stores switched off.  The C ABI is called as ops calls it, on output
    buffers 4 rows longer than R (one clip row longer) and filled with a sentinel: those rows must come back untouched."""
    from uncertainty_nerf_gs_amd import lib as L
    lib, c = L.load(), PC.ALL[key]()
    guard = lambda cols: torch.full((Rr + 4, cols), _SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    new, w, pd = guard(c.nb), guard(c.n), guard(1)
    n_clip = (Rr + CHUNK - 1) // CHUNK
    clip = _clip_buffer(n_clip + 1, dev)
    dens, sb, u = c.dens[:Rr].clone().to(dev), c.sb[:Rr].clone().to(dev), c.u.clone().to(dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        rc = lib.unerf_weights_pdf_resample(p(dens), p(sb), sb.shape[1], Rr, c.n, c.near, c.far, c.spacing, p(u), c.m, c.pad,
                                            c.eps, p(new), p(pd), p(w), p(clip), 0, CHUNK,
                                            torch.cuda.current_stream().cuda_stream)
    L.check(rc, "weights_pdf_resample")
    new, w, pd, clip = new.cpu(), w.cpu(), pd.cpu(), clip.cpu()
    for name, buf in (("bins", new), ("weights", w), ("depth", pd)):
        assert (buf[Rr:].view(torch.int32) == _SENTINEL).all(), f"{name}: a row past R = {Rr} was written"
    assert clip[n_clip].tolist() == [float("inf"), 0.0], "a clip row past the last chunk was written"
    PC.hold(c, w[:Rr], new[:Rr], pd[:Rr], slice(0, Rr))
    _check_clip(c, new[:Rr], clip[:n_clip], lambda r: r // CHUNK)


@pytest.mark.parametrize("key", ["plain-191-65", "plain-63-64", "shared-130-96", "plain-256-255"])
@pytest.mark.parametrize("a,b", [(3, 20), (30, 37), (36, 37), (1, 34)])
def test_a_ray_does_not_depend_on_its_place_in_the_block_walk(dev, key, a, b):
    """rows a .. b as a call of their own land on other blocks, waves and trips: the same bits as in the whole call"""
    whole = _whole(dev, key)
    part = _call(dev, PC.ALL[key](), slice(a, b))
    for x, y in zip(part[:3], whole[:3]):
        assert torch.equal(x.view(torch.int32), y[a:b].view(torch.int32))
