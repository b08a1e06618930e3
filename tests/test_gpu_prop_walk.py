"""prop_patch_kernel<L, HID> walks four consecutive samples per lane: a workgroup is an 8x8 pixel patch x 16 sample indices,
wave wv owns samples 16 g + 4 wv + q, q = 0..3.  What can go wrong there sits at the multiples of 4 (a wave's last live
sample, the edge it takes from the next wave, the 16-byte store) and of 16 (the last sample group of a ray), so n takes
both sides of every one of them: 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 96.  Each n runs with the shared row, own rows and rows
wider than n + 1 (NaN behind edge n: an edge index that is not clamped shows), on one patch (W = 8, R = 64), on W = 9 with
R = 72 (two patch columns, the second one pixel wide, a second band of one live row) and with R = 71 (one ray short of a
band: the linear kernel serves it); spacing and net rotate through both spacings and (L, HID) = (5, 16) and (8, 64) in the
torch-hashed, torch-dense, tcnn fp32 and tcnn half layouts.  On top: a ray_offset inside a row, the output one float off
its 16-byte alignment at n = 16 and n = 96 (four dword stores instead of one vector), and the shared row at n = 256.

Every case asserts: the patch schedule gives the bits of the linear schedule (image_width = 0); every sample is within
prop_cases' bound of its float64 reference and a sample with sel = 0 is exactly 0 (prop_cases.hold); the guard floats
around the output still hold their NaN payload (test_gpu_prop_edges._launch).  Nets, bounds and the reference are
prop_cases'; nothing here comes from a kernel."""
import functools
import itertools
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

import prop_cases as PC

NS = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 96)
KINDS = ("shared", "own", "wide")
SHAPES = ((8, 64), (9, 71), (9, 72))                       # (image width, rays)
NETS = ("t5h16-hashed", "t8h64-dense2", "c5h16-f32", "c8h64-f16")


def _specs():
    """-> [(net, n, bin rows, spacing, R, image width, ray_offset, misalign)]"""
    out = []
    for (ni, n), (ki, kind) in itertools.product(enumerate(NS), enumerate(KINDS)):
        iw, R = SHAPES[(ni + ki) % 3]
        out.append((NETS[(ni + 2 * ki) % 4], n, kind, (ni + ki) % 2, R, iw, 0, 0))
    out += [("t8h64-dense2", 17, "own", 0, 80, 9, 13, 0),        # starts at row 1, column 4: two bands
            ("t5h16-hashed", 33, "wide", 1, 80, 9, 13, 0),
            ("t5h16-hashed", 16, "own", 0, 72, 9, 0, 1),          # n % 4 = 0, the output one float off: dword stores
            ("c8h64-f16", 96, "wide", 1, 64, 8, 0, 1),
            ("t5h16-hashed", 256, "shared", 0, 64, 8, 0, 0)]
    return out


SPECS = _specs()
_ID = lambda s: f"{s[0]}-n{s[1]}-{s[2]}-lin{s[3]}-R{s[4]}-w{s[5]}" + (f"-off{s[6]}" if s[6] else "") + ("-misaligned" if s[7] else "")


@functools.lru_cache(maxsize=None)
def _case(net_name, n, kind, lin, R, iw, off):
    """prop_cases.case for a shape of this file: the same planted rays, bin rows and reference.  The seed moves on when a
    random P32 coordinate falls on a selector border (prop_cases._finish refuses such a case)."""
    nt = PC.net(net_name)
    name = f"walk-{net_name}-n{n}-{kind}-lin{lin}-R{R}-w{iw}-off{off}"
    near, far = PC.NF_SHORT if lin else PC.NF_LONG
    for attempt in range(4):
        rng = np.random.default_rng([zlib.crc32(name.encode()), attempt])
        origins = rng.uniform(-1.2, 1.2, (R, 3))
        dirs = rng.standard_normal((R, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        pts = PC.planted_points(nt)[:R]
        for r, (_, pt) in enumerate(pts):
            origins[r], dirs[r] = pt, 0.0
        own = np.sort(rng.uniform(0, 1, (R, n + 1)), axis=1).astype(PC.f32)
        if kind == "shared":
            row = PC.O.initial_spacing_bins(n).numpy() if n == 256 else own[0]
            sb, sb_rows = row.copy(), np.broadcast_to(row, (R, n + 1)).copy()
        elif kind == "wide":
            sb, sb_rows = np.concatenate([own, np.full((R, PC.WIDE_EXTRA), np.nan, PC.f32)], axis=1), own
        else:
            sb = sb_rows = own
        c = SimpleNamespace(name=name, net=nt, n=n, kind=kind, lin=lin, near=near, far=far, R=R, image_width=iw,
                            ray_offset=off, origins=origins.astype(PC.f32), dirs=dirs.astype(PC.f32),
                            sb=np.ascontiguousarray(sb), sb_rows=sb_rows, tags=[t for t, _ in pts], n_planted=len(pts),
                            patch=iw >= 8 and R >= 8 * iw)
        try:
            return PC._finish(c)
        except AssertionError as e:
            if "selector border" not in str(e):
                raise
    raise AssertionError(f"{name}: no seed keeps the random samples off the selector borders")


def test_the_cases_cover_every_axis_and_build():
    """no GPU: the axes the header lists are all there, and every case builds its reference"""
    rot = SPECS[: len(NS) * len(KINDS)]
    assert {(s[1], s[2]) for s in rot} == set(itertools.product(NS, KINDS))
    assert {(s[1], (s[5], s[4])) for s in rot} == set(itertools.product(NS, SHAPES))
    assert {(s[2], s[3]) for s in rot} == set(itertools.product(KINDS, (0, 1)))
    assert {(s[2], (s[5], s[4])) for s in rot} == set(itertools.product(KINDS, SHAPES))
    assert {(PC.net(s[0]).L, PC.net(s[0]).H) for s in rot} == {(5, 16), (8, 64)}
    assert {(s[2], PC.net(s[0]).L) for s in rot} == set(itertools.product(KINDS, (5, 8)))
    assert {PC.net(s[0]).layout for s in rot} == {"torch", "tcnn32", "tcnn16"}
    assert any(s[6] % s[5] for s in SPECS) and any(s[1] == 256 and s[2] == "shared" and s[4] == 64 for s in SPECS)
    assert {s[1] for s in SPECS if s[7]} == {16, 96}, "misaligned outputs that the vector store would have served"
    for s in SPECS:
        c = _case(*s[:7])
        assert c.patch == ((s[5], s[4]) != (9, 71)) and c.sel.any(), c.name
        assert c.kind != "wide" or np.isnan(c.sb[:, c.n + 1:]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("spec", SPECS, ids=_ID)
def test_patch_schedule_gives_the_linear_bits_within_the_float64_bound(dev, spec, monkeypatch):
    from test_gpu_prop_edges import _launch, _same_bits
    monkeypatch.delenv("UNERF_NO_PATCH_KERNEL", raising=False)
    c, misalign = _case(*spec[:7]), spec[7]
    linear = _launch(dev, c, 0, misalign=misalign)
    patch = _launch(dev, c, c.image_width, misalign=misalign)       # the guards are checked in there
    ratio = PC.hold(c, patch)
    print(f"RATIO {c.name} ({c.net.name}): patch schedule {'yes' if c.patch else 'no (falls back)'} worst error / bound {ratio:.3f}")
    assert _same_bits(patch, linear), "the patch kernel differs from the linear kernel"
