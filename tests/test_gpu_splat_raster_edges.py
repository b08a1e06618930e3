"""The splat rasteriser (raster_kernel<C, BOUNDED> behind ops.splat_rasterize / ops.splat_rasterize_batch) called DIRECTLY on
the hand-built lists of tests/raster_cases.py and held to a float64 blend (oracle.splat_oracle.rasterize_f64) on EVERY pixel:
no share of values is exempt, because the cases hold no (pixel, splat) pair on which fp32 and float64 could decide differently.

What the cases aim at: list lengths 0, 1, 2, 3, 64, 65, 255, 256, 257, 512, 513, 700 (the clamped `entry(k)` and the odd tail
of the two-splats-per-trip walk, the 256-splat staging batches), pixels that stop on the last entry of a batch and the first
of the next, a quadrant that finishes in batch 0 and keeps staging for the others, a workgroup that leaves before its last
batch, the bounded pass's `start > stop` / `start + t > stop` at a batch boundary, raster_quad_mask at the quadrant borders,
tiles whose lower / right quadrants hold one pixel line or none, every C in 1 .. 8, block_width 8 and 5, B = 16 views per
call, the channel maximum, and unerf_splat_depth_sqdiff(_batch) at the image's borders.

Tolerance: per case, E32 = max |SO.rasterize - rasterize_f64| (image and transmittance apart) is the fp32 effect of the
reference's own schedule, with a correctly rounded exp (~2^-24).  The kernel's __expf is a multiply by log2 e and a hardware
exp2, ~(sigma + 1) 2^-23 with sigma <= ln 255 = 5.55: roughly 8 x as much.  The kernel must stay within 8 E32 (2 - 6e-6 here).
final_idx is exact.  Every test prints its worst error / E32 (DESIGN.md section 6.1 records them)."""
import functools

import numpy as np
import pytest
import torch

import raster_cases as RC

pytestmark = pytest.mark.gpu
FACTOR = 8.0
_DEV = {}


def _tensors(dev, key):
    if key not in _DEV:
        c = RC.ALL[key]()
        _DEV[key] = {k: torch.from_numpy(getattr(c, k).copy()).to(dev)
                     for k in ("gids", "bins", "xys", "conics", "opac", "colors", "colors2")}
    return _DEV[key]


def _raster(dev, key, chans, bg=None, cull=True, stop=None, second=False, chan_max=None):
    from uncertainty_nerf_gs_amd import ops
    c, t = RC.ALL[key](), _tensors(dev, key)
    col = t["colors2" if second else "colors"][:, chans].contiguous()
    img, fT, fidx = ops.splat_rasterize(t["gids"], t["bins"], t["xys"], t["conics"], col, t["opac"], c.H, c.W,
                                        None if bg is None else torch.from_numpy(np.array(bg, np.float32)).to(dev),
                                        block_width=c.bw, want_final_idx=True, stop_idx=stop, cull=cull, chan_max=chan_max)
    return img.cpu().numpy(), fT.cpu().numpy(), fidx.cpu().numpy()


def _hold(what, got, want64, want32, fidx_ref):
    """every pixel of (image, final_T, final_idx) against the reference; -> the worst error / E32 of image and transmittance"""
    (img, fT, fidx), (img64, T64), (img32, T32) = got, want64, want32
    assert np.array_equal(fidx, fidx_ref), f"{what}: final_idx differs on {(fidx != fidx_ref).sum()} pixels"
    ratios = []
    for name, g, r64, r32 in (("image", img, img64, img32), ("final_T", fT, T64, T32)):
        assert g.shape == r64.shape and g.dtype == np.float32
        e32, err = float(np.abs(r32 - r64).max()), float(np.abs(g - r64).max())
        ratios.append(err / e32 if e32 > 0 else 0.0)
        print(f"RATIO {what} {name}: error {err:.3e} E32 {e32:.3e} ratio {ratios[-1]:.2f}")
        assert err <= FACTOR * e32, f"{what} {name}: error {err:.3e} > {FACTOR} x E32 {e32:.3e}"
    return ratios


def _want(c, chans, bg, ref=None, ref32=None):
    ref, ref32 = ref or c.ref, ref32 or c.ref32
    i64, i32 = RC.expected(c, chans, bg, ref, ref32)
    return (i64, ref[1]), (i32, ref32[1])


UNBOUNDED = [(k, 3) for k in ("A41x57", "A40x56", "A16x16", "A1x1", "B", "C")] + [("A41x57", C) for C in (1, 2, 4, 5, 6, 7, 8)]


@pytest.mark.parametrize("key,C", UNBOUNDED)
def test_unbounded_pass_matches_f64(dev, key, C):
    c = RC.ALL[key]()
    chans, bg = list(range(C)), c.bg[:C]
    got = _raster(dev, key, chans, bg, cull=True)
    plain = _raster(dev, key, chans, bg, cull=False)
    for a, b in zip(got, plain):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), "culled and unculled walks must give the same bits"
    _hold(f"{key} C={C}", got, *_want(c, chans, bg), c.ref[2])


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("key", ["A41x57", "B"])
def test_bounded_pass_matches_f64(dev, key, C):
    c = RC.ALL[key]()
    ref, ref32 = RC.bounded_ref(key)
    chans, bg = list(range(C)), c.bg[:C]
    _, fT1, fidx1 = _raster(dev, key, [0, 1, 2], None)
    assert np.array_equal(fidx1, c.ref[2])
    for whose, stop in (("reference's", c.ref[2]), ("kernel's own", fidx1)):
        stop_t = torch.from_numpy(stop.copy()).to(dev)
        got = _raster(dev, key, chans, bg, stop=stop_t, second=True)
        plain = _raster(dev, key, chans, bg, stop=stop_t, second=True, cull=False)
        for a, b in zip(got, plain):
            assert np.array_equal(a.view(np.int32), b.view(np.int32))
        assert np.array_equal(got[1].view(np.int32), fT1.view(np.int32)), "the bounded pass must end on the first pass's final_T"
        _hold(f"{key} bounded C={C} stop={whose}", got, *_want(c, chans, bg, ref, ref32), c.ref[2])


@pytest.mark.parametrize("key,C,ch,bg_max", [("A41x57", 5, 4, False), ("A41x57", 5, 0, False), ("A41x57", 3, 0, True),
                                             ("B", 1, 0, False), ("A1x1", 3, 2, False)])
def test_chan_max(dev, key, C, ch, bg_max):
    c = RC.ALL[key]()
    chans, bg = list(range(C)), c.bg[:C].copy()
    if bg_max:
        bg[ch] = 5.0        # above any blended sum (colours < 1): the maximum is a pixel of the empty tile, background alone
    for bounded in (False, True):
        mx = torch.zeros(1, device=dev)
        stop = torch.from_numpy(c.ref[2].copy()).to(dev) if bounded else None
        img, _, _ = _raster(dev, key, chans, bg, stop=stop, second=bounded, chan_max=(ch, mx))
        got = mx.cpu().numpy()[0]
        assert got.view(np.int32) == np.maximum(np.float32(0), img[..., ch].max()).view(np.int32)
        ref, ref32 = RC.bounded_ref(key) if bounded else (c.ref, c.ref32)
        i64, i32 = RC.expected(c, chans, bg, ref, ref32)
        e32 = np.abs(i32 - i64).max()
        assert abs(got - max(0.0, i64[..., ch].max())) <= FACTOR * e32
        if bg_max:
            assert got == 5.0


@pytest.mark.parametrize("bw", [8, 5])
def test_narrow_tiles_match_f64(dev, bw):
    key = f"D{bw}"
    c = RC.ALL[key]()
    chans, bg = [0, 1, 2], c.bg[:3]
    got = _raster(dev, key, chans, bg)
    for a, b in zip(got, _raster(dev, key, chans, bg, cull=False)):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    _hold(key, got, *_want(c, chans, bg), c.ref[2])
    stop_t = torch.from_numpy(c.ref[2].copy()).to(dev)
    again = _raster(dev, key, chans, bg, stop=stop_t)           # the bounded pass of the same colours blends the same pairs
    _hold(f"{key} bounded", again, *_want(c, chans, bg), c.ref[2])
    assert np.array_equal(again[1].view(np.int32), got[1].view(np.int32))


# ---------------------------------------------------------------- B views per call

@functools.lru_cache(maxsize=None)
def _batch(B):
    """-> the host arrays of B views on 41 x 57 cycling cases A and B, with views of no pairs first, in the middle and last
    (B = 1: case B alone).  View v blends the colour channels (v, v + 1, v + 2) mod 8 of its case."""
    a, b = RC.ALL["A41x57"](), RC.ALL["B"]()
    N = b.N
    views = ["B"] if B == 1 else [None if v in (0, B // 2, B - 1) else ("A41x57", "B")[v % 2] for v in range(B)]
    pad = lambda x: np.concatenate([x, np.zeros((N - len(x),) + x.shape[1:], x.dtype)])
    o = dict(views=views, N=N, chans=[[(v + j) % RC.NCH for j in range(3)] for v in range(B)], off=[], ids=[], bins=[])
    for k in ("xys", "conics", "opac", "colors", "colors2"):
        o[k] = []
    off = 0
    for v, key in enumerate(views):
        c = RC.ALL[key or "A41x57"]()
        o["off"].append(off)
        for k in ("xys", "conics", "opac"):
            o[k].append(pad(getattr(c, k)))
        for k in ("colors", "colors2"):
            o[k].append(pad(getattr(c, k))[:, o["chans"][v]])
        if key is None:
            o["bins"].append(np.zeros_like(c.bins))
            continue
        o["ids"].append(c.gids.astype(np.int64) + v * N)
        o["bins"].append((c.bins + off * (c.bins[:, 1:] > c.bins[:, :1])).astype(np.int32))      # empty tiles stay (0, 0)
        off += len(c.gids)
    o["ids"] = np.concatenate(o["ids"]).astype(np.int32)
    for k in ("bins", "xys", "conics", "opac", "colors", "colors2"):
        o[k] = np.ascontiguousarray(np.stack(o[k]))
    return o


@pytest.mark.parametrize("B", [16, 1])
def test_batch_matches_f64_and_single_view(dev, B):
    from uncertainty_nerf_gs_amd import ops
    o = _batch(B)
    a = RC.ALL["A41x57"]()
    H, W, N = a.H, a.W, o["N"]
    bg = a.bg[:3]
    t = {k: torch.from_numpy(o[k]).to(dev) for k in ("ids", "bins", "xys", "conics", "opac", "colors", "colors2")}
    bg_t = torch.from_numpy(bg.copy()).to(dev)
    geo = (t["ids"], t["bins"], t["xys"], t["conics"])
    mx1, mx2 = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    img, fT, fidx = ops.splat_rasterize_batch(*geo, t["colors"], t["opac"], H, W, bg_t, want_final_idx=True, chan_max=(2, mx1))
    img2, fT2, fidx2 = ops.splat_rasterize_batch(*geo, t["colors2"], t["opac"], H, W, bg_t, want_final_idx=True, stop_idx=fidx,
                                                 chan_max=(0, mx2))
    assert img.shape == (B, H, W, 3) and fT.shape == (B, H, W) and fidx.shape == (B, H, W)
    assert torch.equal(fT2, fT) and torch.equal(fidx2, fidx)
    for m, im, ch in ((mx1, img, 2), (mx2, img2, 0)):
        assert torch.equal(m, im[..., ch].amax(dim=(1, 2)).clamp_min(0)), "each view's own channel maximum"
    bits = lambda x: x.cpu().numpy().view(np.int32)
    for v, key in enumerate(o["views"]):
        off, chans = o["off"][v], o["chans"][v]
        if key is None:
            assert torch.all(fT[v] == 1) and torch.all(fidx[v] == 0) and torch.all(img[v] == bg_t) and torch.all(img2[v] == bg_t)
            ids_v, bins_v = t["ids"][:0], torch.zeros_like(t["bins"][v])
        else:
            c = RC.ALL[key]()
            n = len(c.gids)
            ids_v, bins_v = t["ids"][off:off + n] - v * N, torch.from_numpy(c.bins.copy()).to(dev)
            fidx_ref = np.where(c.ref[3] > 0, c.ref[2] + off, 0).astype(np.int32)      # global pair indices; 0: nothing blended
            _hold(f"batch{B} view {v} ({key})", (img[v].cpu().numpy(), fT[v].cpu().numpy(), fidx[v].cpu().numpy()),
                  *_want(c, chans, bg), fidx_ref)
            _hold(f"batch{B} view {v} ({key}) bounded", (img2[v].cpu().numpy(), fT2[v].cpu().numpy(), fidx2[v].cpu().numpy()),
                  *_want(c, chans, bg, *RC.bounded_ref(key)), fidx_ref)
        # the single-view call on the view's slice: ids shifted by -v N, bins by the pairs before it
        one = ops.splat_rasterize(ids_v.contiguous(), bins_v, t["xys"][v], t["conics"][v], t["colors"][v], t["opac"][v], H, W, bg_t,
                                  want_final_idx=True)
        blended = one[2] > 0 if key is None else torch.from_numpy(RC.ALL[key]().ref[3] > 0).to(dev)
        assert np.array_equal(bits(one[0]), bits(img[v])) and np.array_equal(bits(one[1]), bits(fT[v]))
        assert torch.equal(torch.where(blended, one[2] + off, torch.zeros_like(one[2])), fidx[v])
        two = ops.splat_rasterize(ids_v.contiguous(), bins_v, t["xys"][v], t["conics"][v], t["colors2"][v], t["opac"][v], H, W, bg_t,
                                  stop_idx=one[2])
        assert np.array_equal(bits(two[0]), bits(img2[v])) and np.array_equal(bits(two[1]), bits(fT2[v]))


# ---------------------------------------------------------------- per-splat depth difference

def _sqdiff_ref(xys, depths, img, ch):
    """numpy restatement of the reference's per-splat depth difference (activesplatfacto_model.py:325-341, squared at :349)"""
    H, W = img.shape[:2]
    pix = np.floor(xys).astype(np.int64)
    valid = (pix[:, 0] > 0) & (pix[:, 0] < W) & (pix[:, 1] > 0) & (pix[:, 1] < H)
    d = depths.copy()
    d[valid] -= img[pix[valid, 1], pix[valid, 0], ch]
    return d * d


@functools.lru_cache(maxsize=None)
def _sqdiff_inputs(B, H, W):
    """per view: 257 random splats around the image, and the border set: floor(x) in {-1, 0, 1, W - 1, W}, x = -0.5 and 1e10,
    with every such y"""
    rng = np.random.default_rng([B, H, W])
    bx = [-0.75, 0.25, 1.5, W - 0.5, W + 0.25, -0.5, 1e10]
    by = [-0.75, 0.25, 1.5, H - 0.5, H + 0.25, -0.5, 1e10]
    border = np.array([(x, y) for x in bx for y in by], np.float32)
    xys = np.stack([rng.permutation(np.concatenate([rng.uniform(-2, [W + 2, H + 2], (257, 2)).astype(np.float32), border]))
                    for _ in range(B)])
    depths = rng.uniform(0.5, 9, xys.shape[:2]).astype(np.float32)
    return xys, depths, rng.uniform(0.5, 9, (B, H, W, 5)).astype(np.float32)


@pytest.mark.parametrize("stride,ch", [(1, 0), (5, 4)])
def test_depth_sqdiff_bit_equal(dev, stride, ch):
    from uncertainty_nerf_gs_amd import ops
    H, W = 41, 57
    for B in (1, 16):
        xys, depths, img5 = _sqdiff_inputs(B, H, W)
        img = np.ascontiguousarray(img5[..., :stride] if stride == 5 else img5[..., 2:3])
        ref = np.stack([_sqdiff_ref(xys[v], depths[v], img[v], ch) for v in range(B)])
        inside = (np.floor(xys[0]) > 0).all(1) & (np.floor(xys[0, :, 0]) < W) & (np.floor(xys[0, :, 1]) < H)
        assert 128 < inside.sum() < len(inside) - 40          # most random splats fetch a depth, most of the border set does not
        x_t, d_t, i_t = (torch.from_numpy(v).to(dev) for v in (xys, depths, img))
        got = ops.splat_depth_sqdiff_batch(x_t, d_t, i_t, ch).cpu().numpy()
        assert got.shape == ref.shape and np.array_equal(got.view(np.int32), ref.view(np.int32))
        for v in (0, B - 1):
            one = ops.splat_depth_sqdiff(x_t[v], d_t[v], i_t[v], ch).cpu().numpy()
            assert np.array_equal(one.view(np.int32), ref[v].view(np.int32))
