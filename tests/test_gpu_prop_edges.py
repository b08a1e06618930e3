"""The proposal density kernels (prop_density_kernel<L, HID> and prop_patch_kernel<L, HID> behind unerf_proposal_density) on the
hand-placed cases of tests/prop_cases.py, held to a float64 reference on EVERY sample: no share of samples is exempt, and a
sample with sel = 0 must be exactly 0.

What the cases aim at: all six (levels, hidden) pairs; the torch hash table with 0, 2 and all of its levels (5 and 8) read from
the dense x-paired copy, the tcnn layout with fp32 and with half rows; the scene contraction with |x| one ulp to either side
of 1, on 1 and far enough out to round to p = 1, the scene box with p = 0, 1, 2^-24 and 1 - 2^-24 (the last cell of every level
and of every dense copy); the world origin, level-0 nodes and faces of single levels (the kernel's floor + 1 corner against the
reference's ceil); both spacings, the shared row, own rows and wide rows, n in {1, 2, 3, 4, 5, 7, 8, 13, 16, 256}; image widths
8, 9, 37, 64, R on and one below 8 * image_width, a ray_offset inside a row and a band, 1, 4, 10 and 16 workgroups (the XCD
remap's surplus blocks), a last band of one live row, R = 1, and the 16-byte store against an output one float off alignment.
Every launch goes through the C ABI on an output between guard floats that hold a NaN payload.

Bounds: prop_cases.py states and derives them; none comes from a kernel.  Every test prints its worst error / bound
(DESIGN.md section 6.1 records them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import prop_cases as PC

pytestmark = pytest.mark.gpu
_SENTINEL = 0x7FC0BEEF        # a NaN with a payload: no result has this bit pattern
_GUARD = 8                    # floats in front of the output (32 bytes: keeps the 16-byte alignment) and at least as many behind
_NETS, _RESULT = {}, {}


def _net_dev(dev, nt, use_dense=None):
    from uncertainty_nerf_gs_amd import ops
    use_dense = nt.use_dense if use_dense is None else use_dense
    key = (nt.name, use_dense)
    if key not in _NETS:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        w0, b0 = (t(nt.w0), t(nt.b0)) if nt.H else (None, None)
        if nt.layout == "torch":
            f = lambda a: t(a).to(dev)
            w0t, b0d = (f(nt.w0.T), f(nt.b0)) if nt.H else (torch.zeros(0, device=dev), torch.zeros(0, device=dev))
            nd = ops.DensityNetDev(f(nt.table), f(nt.scalings), nt.log2T, w0t, b0d, f(nt.w1.T), f(nt.b1), f(nt.dense),
                                   tuple(nt.dense_off), tuple(nt.dense_dim), use_dense=use_dense)
        else:
            nd = ops.DensityNetDev.from_torch(t(nt.table), None, nt.log2T, w0, b0, t(nt.w1), t(nt.b1), dev, tcnn_levels=nt.levels,
                                              grid_precision="f16" if nt.layout == "tcnn16" else "f32")
        nd.aabb = nt.aabb
        _NETS[key] = nd
    return _NETS[key]


def _launch(dev, c, image_width, misalign=0, use_dense=None):
    """unerf_proposal_density through the C ABI -> [R,n] float32 on the CPU; the guard floats must come back untouched"""
    from uncertainty_nerf_gs_amd import lib as L
    lib, nd = L.load(), _net_dev(dev, c.net, use_dense)
    o, d, sb = (torch.from_numpy(a).to(dev) for a in (c.origins, c.dirs, c.sb))
    stride = 0 if c.sb.ndim == 1 else c.sb.shape[1]
    total = c.R * c.n
    buf = torch.full((_GUARD + total + _GUARD + 4,), _SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    start = _GUARD + misalign
    ptr = buf.data_ptr() + 4 * start
    assert buf.data_ptr() % 16 == 0 and (ptr % 16 == 0) == (misalign == 0)
    cs = nd.cstruct()
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        rc = lib.unerf_proposal_density(p(o), p(d), p(sb), stride, c.R, c.n, c.near, c.far, c.lin, C.byref(cs), PC.AVG,
                                        C.c_void_p(ptr), c.ray_offset, image_width, torch.cuda.current_stream().cuda_stream)
    L.check(rc, "proposal_density")
    host = buf.cpu()
    bits = host.view(torch.int32)
    assert (bits[:start] == _SENTINEL).all(), f"{c.name}: a float in front of the output was written"
    assert (bits[start + total:] == _SENTINEL).all(), f"{c.name}: a float behind the output was written"
    return host[start: start + total].reshape(c.R, c.n).clone()


def _schedules(dev, key, monkeypatch):
    """-> {"linear", "walk", "patch"}: one thread per sample, prop_density_kernel on the patch schedule, the LDS patch kernel"""
    if key not in _RESULT:
        c = PC.case(key)
        monkeypatch.delenv("UNERF_NO_PATCH_KERNEL", raising=False)
        res = {"linear": _launch(dev, c, 0), "patch": _launch(dev, c, c.image_width)}
        monkeypatch.setenv("UNERF_NO_PATCH_KERNEL", "1")
        res["walk"] = _launch(dev, c, c.image_width)
        monkeypatch.delenv("UNERF_NO_PATCH_KERNEL")
        _RESULT[key] = res
    return _RESULT[key]


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("key", list(PC.CASES))
def test_every_sample_within_its_bound_on_all_three_schedules(dev, key, monkeypatch):
    c = PC.case(key)
    res = _schedules(dev, key, monkeypatch)
    ratios = {k: PC.hold(c, v) for k, v in res.items()}
    print(f"RATIO {key} ({c.net.name}): patch schedule {'yes' if c.patch else 'no (falls back)'} worst error / bound: "
          + " ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    assert _same_bits(res["patch"], res["linear"]), "the patch kernel differs from the linear kernel"
    assert _same_bits(res["walk"], res["patch"]), "prop_density_kernel on the patch schedule differs from the LDS patch kernel"


@pytest.mark.parametrize("key", [k for k in PC.CASES if PC.net(PC.CASES[k][0]).n_dense > 0])
def test_dense_copy_gives_the_bits_of_the_hashed_lookup(dev, key, monkeypatch):
    c = PC.case(key)
    res = _schedules(dev, key, monkeypatch)
    for name, iw in (("linear", 0), ("patch", c.image_width)):
        hashed = _launch(dev, c, iw, use_dense=False)
        print(f"RATIO {key} ({c.net.name}) hashed lookup, {name}: worst error / bound {PC.hold(c, hashed):.3f}")
        assert _same_bits(hashed, res[name]), f"{name}: {c.net.n_dense} dense levels differ from the hashed lookup"


@pytest.mark.parametrize("key", [k for k in PC.CASES if PC.CASES[k][1] % 4 == 0])
def test_unaligned_output_gives_the_bits_of_the_vector_store(dev, key, monkeypatch):
    """n % 4 = 0: the patch kernel stores a ray's four densities as one 16-byte vector when the output allows it, as scalars
    when the pointer is one float off"""
    c = PC.case(key)
    res = _schedules(dev, key, monkeypatch)
    for name, iw in (("linear", 0), ("patch", c.image_width)):
        off = _launch(dev, c, iw, misalign=1)
        assert _same_bits(off, res[name]), f"{name}: the unaligned output differs"


@pytest.mark.parametrize("key", ["b-n16-wide-offset", "c-n3-wide-offset", "a-n256-shared", "h-n8-own", "a-n7-wide-R1"])
def test_ops_entry_point_gives_the_same_bits(dev, key, monkeypatch):
    from uncertainty_nerf_gs_amd import ops
    c = PC.case(key)
    res = _schedules(dev, key, monkeypatch)
    o, d, sb = (torch.from_numpy(a).to(dev) for a in (c.origins, c.dirs, c.sb))
    got = ops.proposal_density(o, d, sb, _net_dev(dev, c.net), c.near, c.far, PC.AVG, n=c.n, ray_offset=c.ray_offset,
                               image_width=c.image_width, spacing=c.lin).cpu()
    assert _same_bits(got, res["patch"])
