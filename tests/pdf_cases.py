"""Hand-placed cases for the PDF resampler (plain module: tests import it; nothing here needs a GPU).

pdf_kernel<EPL> (csrc/unerf_nerf.hip, section 4) gives one wave to a ray, lane l the samples [l EPL, (l + 1) EPL) with
EPL = ceil(n / 64), scans three times across the wave and finds each output's CDF interval by a power-of-two descent.  The
cases put n on both sides of every EPL border (64, 128, 192), m + 1 on both sides of the 64-wide output loop (and at the ABI's
ends, m = 1 and m + 1 = 256), the median on the first and last element of a lane's run, R = 37 (a full 32-ray block, then a
block of one full wave-quad and ONE live wave), wide sbins rows, the shared row and the uniform spacing.

Reference: `reference` takes the Euclidean edges from the fp32 oracle (O.spacing_to_euclidean; the kernel's unerf_s2e is the
same fp32 operation sequence, and with near 0.05 / far 1000 the map is too ill-conditioned to compare across precisions) and
does everything after them in float64.  `chain32` is the same chain in float32: the oracle's operations (O.get_weights,
O.pdf_resample, O.render_depth_median) with `u` as an argument.

Bounds, per element, from the reference's own conditioning (nothing here comes from a GPU result):
  * weights.  __expf is allowed (|x| + 1) 2^-23 relative.  With dd_k = delta_k sigma_k, c_k = sum_{j<k} dd_j,
    T_k = exp(-c_k), w_k = (1 - exp(-dd_k)) T_k:
        |dw_k| <= WEIGHT_FACTOR [(dd_k + 1) exp(-dd_k) T_k + (c_k + 2) w_k] 2^-23 + 2^-125.
    The first term is the error of exp(-dd_k) (and of dd_k's own rounding) carried into alpha; it keeps the exp(-dd_k) <= 1 that
    the plain form (dd_k + 1) T_k drops, so a saturated sample (dd = 1e4, inf) is still held.  The second is T's relative error
    and the roundings of alpha and the product.  WEIGHT_FACTOR = 2 is the margin for the fp32 rounding of dd and of the scanned
    prefix.  2^-125 is the fp32 underflow threshold (flushed products).  Where the reference's dd or prefix is NaN the weight is
    0 in any arithmetic (nan_to_num) and the bound is 0.
  * bins.  |dv_j| <= K_j EPS_CDF + 2^-23, K_j = the largest (b[i+1] - b[i]) / (cdf[i+1] - cdf[i]) over the reference's interval
    and any neighbour whose shared knot lies within EPS_CDF of u_j.  EPS_CDF = 4 x the worst |cdf(chain32) - cdf(float64)| over
    all toleranced cases (CDF_WORST_MEASURED, measured on the CPU: fp32 chain against float64, never a kernel); the 4 x allows
    for another summation order and the device exponential.  test_pdf_cases_cpu.py re-measures it.
  * median depth.  A ray is a TIE when its margin min_k |cumsum(w)_k - 0.5| is at most the sum of its weight bounds up to the
    median index.  A non-tie ray must give the mid-point of the reference's index to rtol 1e-5, a tie ray that of the index or
    of a neighbour.

The exact family (lattice, single bin) has outputs known exactly in any summation order and is compared bit for bit."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle import nerf_oracle as O

NEAR, FAR = 0.05, 1000.0
R = 37
PAD, EPS = 0.01, 1e-5
U23, FLT_UNDERFLOW = 2.0 ** -23, 2.0 ** -125
WEIGHT_FACTOR = 2.0
# worst weight error of chain32 / the weight bound over all toleranced cases, measured on the CPU (fp32 chain against float64):
# the oracle's own fp32 arithmetic, with a correctly rounded exp, uses a third of the bound
WEIGHT_RATIO_MEASURED = 0.351
# worst |cdf(chain32) - cdf(float64)| over all toleranced cases (fp32 CPU chain against float64), and 4 x it rounded up
CDF_WORST_MEASURED = 5.81e-7
EPS_CDF = 2.4e-6
MAX_TIES = 0.02
DEPTH_RTOL = 1e-5

N_ALL = (1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
M_ALL = (1, 2, 63, 64, 65, 127, 128, 255)
# every n and every m at least twice; m > n, m < n and (256, 255) among them; (129, 191) adds m + 1 = 192
SHAPES = ((1, 1), (1, 64), (2, 2), (2, 65), (3, 63), (3, 127), (63, 64), (63, 128), (64, 65), (64, 255), (65, 127), (65, 1),
          (127, 128), (127, 2), (128, 255), (128, 63), (129, 1), (129, 64), (129, 191), (191, 2), (191, 65), (192, 63),
          (192, 127), (193, 64), (193, 128), (255, 65), (255, 255), (256, 255), (256, 1))
VARIANTS = (("wide", 130, 64), ("wide", 63, 65), ("wide", 256, 128), ("shared", 100, 48), ("shared", 130, 96),
            ("shared", 256, 96), ("uniform", 129, 63), ("uniform", 64, 2), ("uniform", 200, 127), ("nan", 130, 64),
            ("nan", 65, 128))
WIDE_EXTRA = 5
# generator seeds per case name (default 0): a seed is changed when a case would hold more tie rays than MAX_TIES allows
SEEDS = {}


def epl_of(n):
    return (n + 63) // 64


def _chain(dens, sb, u, near, far, spacing, pad, eps, dtype):
    """get_weights -> median -> pdf -> cdf -> searchsorted -> interpolation, on fp32 Euclidean edges, in `dtype`"""
    dens, sb, u = (torch.as_tensor(a, dtype=torch.float32) for a in (dens, sb, u))
    Rr, n = dens.shape
    assert sb.shape == (Rr, n + 1)
    eb32 = O.spacing_to_euclidean(sb, near, far, uniform=bool(spacing))
    steps32 = (eb32[:, :-1] + eb32[:, 1:]) / 2
    eb, d, b, uu = eb32.to(dtype), dens.to(dtype), sb.to(dtype), u.to(dtype)
    pad, eps = float(np.float32(pad)), float(np.float32(eps))          # the values the kernel is handed
    dd = (eb[:, 1:] - eb[:, :-1]) * d
    c = torch.cat([torch.zeros(Rr, 1, dtype=dtype), torch.cumsum(dd[:, :-1], dim=-1)], dim=-1)
    w = torch.nan_to_num((1 - torch.exp(-dd)) * torch.exp(-c))
    cw = torch.cumsum(w, dim=-1)
    idx = torch.clamp(torch.searchsorted(cw, torch.full((Rr, 1), 0.5, dtype=dtype), side="left"), 0, n - 1)
    margin = (cw - 0.5).abs().min(dim=-1).values
    wp = w + pad
    wsum = torch.sum(wp, dim=-1, keepdim=True)
    padding = torch.relu(eps - wsum)
    wp = wp + padding / n
    wsum = wsum + padding
    pdf = wp / wsum
    cdf = torch.min(torch.ones_like(pdf), torch.cumsum(pdf, dim=-1))
    cdf = torch.cat([torch.zeros_like(cdf[:, :1]), cdf], dim=-1)
    uu = uu.expand(Rr, uu.numel()).contiguous()
    inds = torch.searchsorted(cdf, uu, side="right")
    below, above = torch.clamp(inds - 1, 0, n), torch.clamp(inds, 0, n)
    g0, g1 = torch.gather(cdf, -1, below), torch.gather(cdf, -1, above)
    b0, b1 = torch.gather(b, -1, below), torch.gather(b, -1, above)
    t = torch.clip(torch.nan_to_num((uu - g0) / (g1 - g0), 0), 0, 1)
    new = b0 + t * (b1 - b0)
    return SimpleNamespace(weights=w, c=c, dd=dd, cdf=cdf, below=below, above=above, new=new, idx=idx[:, 0], margin=margin,
                           steps32=steps32, depth=torch.gather(steps32, -1, idx))


def reference(dens32, sb32, u32, near=NEAR, far=FAR, spacing=0, pad=PAD, eps=EPS):
    """float64 on the fp32 oracle's Euclidean edges -> weights [R,n], c (prefix sums), dd, cdf [R,n+1], below / above [R,nb]
    (the chosen interval), new [R,nb], idx [R] (median index), margin [R], steps32 [R,n] (fp32 mid-points), depth [R,1]"""
    return _chain(dens32, sb32, u32, near, far, spacing, pad, eps, torch.float64)


def chain32(dens32, sb32, u32, near=NEAR, far=FAR, spacing=0, pad=PAD, eps=EPS):
    """the oracle's operations in float32 (O.get_weights, O.render_depth_median, O.pdf_resample with `u` as an argument)"""
    return _chain(dens32, sb32, u32, near, far, spacing, pad, eps, torch.float32)


def descent(cdf, u):
    """The kernel's stand-in for searchsorted(cdf, u, side="right") - 1, restated: descend by powers of two from the largest
    one <= n, every probe clamped to n.  cdf [R,n+1], u [nb] -> pos [R,nb], the last index with cdf <= u"""
    cdf, u = np.asarray(cdf), np.asarray(u)
    n = cdf.shape[1] - 1
    pos, step = np.zeros((cdf.shape[0], len(u)), np.int64), 1 << (n.bit_length() - 1)
    while step > 0:
        probe = np.minimum(pos + step, n)
        pos = np.where(np.take_along_axis(cdf, probe, 1) <= u[None], probe, pos)
        step >>= 1
    return pos


def weight_bound(ref):
    dd, c, w = ref.dd, ref.c, ref.weights
    T = torch.exp(-c)
    a = torch.where(torch.isfinite(dd), (dd + 1) * torch.exp(-dd), torch.zeros_like(dd)) * T      # (inf + 1) exp(-inf) = 0
    b = torch.where(w > 0, (c + 2) * w, torch.zeros_like(w))                                       # (inf + 2) 0 = 0
    bound = WEIGHT_FACTOR * (a + b) * U23 + FLT_UNDERFLOW
    return torch.where(torch.isnan(dd) | torch.isnan(c), torch.zeros_like(bound), bound)


def bin_slopes(ref, sb32):
    b = torch.as_tensor(sb32, dtype=torch.float64)
    return (b[:, 1:] - b[:, :-1]) / (ref.cdf[:, 1:] - ref.cdf[:, :-1])


def bin_bound(ref, sb32, u32, eps_cdf=None):
    eps_cdf = EPS_CDF if eps_cdf is None else eps_cdf
    n = ref.cdf.shape[1] - 1
    slope = bin_slopes(ref, sb32)
    u = torch.as_tensor(u32, dtype=torch.float64).expand(ref.below.shape)
    i0 = torch.clamp(ref.below, max=n - 1)               # u >= cdf[n]: the last interval is the candidate
    K = torch.gather(slope, -1, i0)
    left, right = torch.clamp(i0 - 1, min=0), torch.clamp(i0 + 1, max=n - 1)
    near_lo = (u - torch.gather(ref.cdf, -1, i0)).abs() <= eps_cdf
    near_hi = (torch.gather(ref.cdf, -1, i0 + 1) - u).abs() <= eps_cdf
    K = torch.where(near_lo, torch.maximum(K, torch.gather(slope, -1, left)), K)
    K = torch.where(near_hi, torch.maximum(K, torch.gather(slope, -1, right)), K)
    return K * eps_cdf + U23, K


def ties(ref, wb):
    """[R] bool: the margin is within the sum of the weight bounds up to the median index"""
    return ref.margin <= torch.gather(torch.cumsum(wb, dim=-1), -1, ref.idx[:, None])[:, 0]


def hold(c, w, new, depth, rows=None):
    """Every weight, bin and depth of a result (float32 tensors on the CPU) against the case's rules; rows: the case's rays the
    result holds (default all).  Asserts, and returns the worst error / bound of (weights, bins); exact cases are compared
    bit for bit and return (0, 0)."""
    rows = slice(None) if rows is None else rows
    w, new, depth = (a.detach().cpu() for a in (w, new, depth))
    ref = c.ref
    assert w.dtype == new.dtype == depth.dtype == torch.float32
    assert w.shape == ref.weights[rows].shape and new.shape == ref.new[rows].shape and depth.shape == ref.depth[rows].shape
    # median depth
    mids = ref.steps32.double()
    n = mids.shape[1]
    pick = lambda k: torch.gather(mids, -1, torch.clamp(k, 0, n - 1)[:, None])[rows]
    near = lambda k: (depth.double() - pick(k)).abs() <= DEPTH_RTOL * pick(k).abs()
    ok = torch.where(c.tie[rows, None], near(ref.idx) | near(ref.idx - 1) | near(ref.idx + 1), near(ref.idx))
    assert ok.all(), f"{c.name}: median depth off on rays {torch.nonzero(~ok[:, 0])[:, 0].tolist()} (of the rows passed)"
    if c.family == "exact":
        assert torch.equal(w, c.expect_w[rows]), f"{c.name}: weights differ from the exact values"
        bad = torch.nonzero(new != c.expect_new[rows])
        assert torch.equal(new, c.expect_new[rows]), f"{c.name}: bins differ from the exact values at (ray, j) {bad[:8].tolist()}"
        return 0.0, 0.0
    ew, eb = (w.double() - ref.weights[rows]).abs(), (new.double() - ref.new[rows]).abs()
    assert not torch.isnan(w).any() and not torch.isnan(new).any(), f"{c.name}: NaN in the result"
    bad = torch.nonzero(ew > c.wb[rows])
    assert len(bad) == 0, (f"{c.name}: {len(bad)} weights beyond their bound, first (ray, k) {bad[:8].tolist()}, worst error / bound "
                           f"{(ew / c.wb[rows])[c.wb[rows] > 0].max().item():.3g}")
    bad = torch.nonzero(eb > c.bb[rows])
    assert len(bad) == 0, (f"{c.name}: {len(bad)} bins beyond their bound, first (ray, j) {bad[:8].tolist()}, worst error / bound "
                           f"{(eb / c.bb[rows]).max().item():.3g}")
    live = c.wb[rows] > 0
    return (ew[live] / c.wb[rows][live]).max().item(), (eb / c.bb[rows]).max().item()


def _finish(c):
    """the cached float64 reference, the bounds and the builder's assertions (all on the reference alone)"""
    c.epl, c.nb = epl_of(c.n), c.m + 1
    c.ref = reference(c.dens, c.sb_rows, c.u, c.near, c.far, c.spacing, c.pad, c.eps)
    c.wb = weight_bound(c.ref)
    c.tie = ties(c.ref, c.wb)
    assert c.tie.sum().item() <= MAX_TIES * c.dens.shape[0], f"{c.name}: {c.tie.sum().item()} tie rays"
    if c.family == "toleranced":
        c.bb, c.K = bin_bound(c.ref, c.sb_rows, c.u)
        assert torch.isfinite(c.K).all() and torch.isfinite(c.bb).all(), f"{c.name}: a flat CDF interval"
    return c


@functools.lru_cache(maxsize=None)
def toleranced(n, m, variant=None):
    """seeded densities exp(2.5 randn) on sorted uniform bins, with planted rows: 0 all zero, 1 first half zero, 2 all 1e4,
    3 one inf, 4 the initial bins, 5 total weight < 0.5 (median clamps to n - 1), 6 median index 0, 7 median on the last element
    of lane 0's run, 8 on the first of lane 1's, 9 (variant "nan") a zero-width bin with inf density.
    variant: "wide" sbins rows of n + 1 + 5 columns (NaN in the extra ones), "shared" one row for all rays (sstride = 0),
    "uniform" SPACING_UNIFORM with near 1 / far 100, "nan" row 9"""
    name = f"{variant or 'plain'}-{n}-{m}"
    g = torch.Generator().manual_seed(100003 * SEEDS.get(name, 0) + 1000 * n + m)
    epl = epl_of(n)
    near, far, spacing = (1.0, 100.0, 1) if variant == "uniform" else (NEAR, FAR, 0)
    dens = torch.exp(torch.randn(R, n, generator=g) * 2.5)
    sb = torch.sort(torch.rand(R, n + 1, generator=g), dim=-1).values
    if variant == "shared":
        sb = sb[5:6].expand(R, -1).contiguous()
    else:
        sb[4] = O.initial_spacing_bins(n)
    nan_k = n // 3
    if variant == "nan":
        sb[9, nan_k + 1] = sb[9, nan_k]
    eb = O.spacing_to_euclidean(sb, near, far, uniform=bool(spacing)).double()
    delta = eb[:, 1:] - eb[:, :-1]
    dens[0] = 0.0
    dens[1, : n // 2] = 0.0
    dens[2] = 1e4
    dens[3, min(5, n - 1)] = float("inf")
    dens[5] = (0.3 / (eb[5, -1] - eb[5, 0])).float()          # optical depth 0.3 in all: total weight 0.26
    planted = {5: n - 1, 6: 0, 7: min(epl - 1, n - 1), 8: min(epl, n - 1)}
    for r in (6, 7, 8):
        k = planted[r]
        assert delta[r, k] > 0
        dens[r, :k] = 0.0
        dens[r, k] = (2.0 / delta[r, k]).float()              # dd = 2: w_k = 0.86
    if variant == "nan":
        dens[9, nan_k] = float("inf")
    c = SimpleNamespace(name=name, family="toleranced", variant=variant, n=n, m=m, dens=dens, sb_rows=sb, u=O.pdf_u(m), near=near,
                        far=far, spacing=spacing, pad=PAD, eps=EPS, planted=planted)
    c.sb = sb
    if variant == "wide":
        c.sb = torch.cat([sb, torch.full((R, WIDE_EXTRA), float("nan"))], dim=1).contiguous()
    elif variant == "shared":
        c.sb = sb[0].clone()
    _finish(c)
    for r, k in planted.items():
        assert c.ref.idx[r].item() == k, f"{name}: planted median {k} on ray {r}, reference has {c.ref.idx[r].item()}"
    assert c.ref.weights[5].sum().item() < 0.5 and not c.tie[list(planted)].any()
    if variant == "nan":
        assert torch.isnan(c.ref.dd[9, nan_k]) and (c.ref.weights[9, nan_k:] == 0).all() and (c.wb[9, nan_k:] == 0).all()
        assert (c.wb[9, :nan_k] > 0).all()
    return c


def _exact(name, n, dens, sb, u, pad, expect_new, expect_w, shared=False):
    c = SimpleNamespace(name=name, family="exact", variant="shared" if shared else None, n=n, m=len(u) - 1, dens=dens, sb_rows=sb,
                        sb=sb[0].clone() if shared else sb, u=u, near=NEAR, far=FAR, spacing=0, pad=pad, eps=EPS,
                        expect_new=expect_new, expect_w=expect_w)
    _finish(c)
    assert torch.equal(c.ref.new.float(), expect_new) and torch.equal(c.ref.weights.float(), expect_w), name
    return c


LATTICE_RAYS = 6


@functools.lru_cache(maxsize=None)
def lattice(n, part):
    """zero density, histogram_padding = 1 / n, bins k / n: every partial weight sum is dyadic, wsum = 1 and the CDF is k / n
    exactly in any summation order.  u = the knots k / n (0 and 1.0 among them; output sb[k]) and the mid-points (k + 1/2) / n
    (output (sb[k] + sb[k+1]) / 2), in as many equal parts as m + 1 <= 256 needs; n = 256 takes the shared row"""
    assert n in (64, 128, 256)
    u_all = torch.arange(2 * n + 1, dtype=torch.float32) / (2 * n)
    parts = np.array_split(np.arange(2 * n + 1), math.ceil((2 * n + 1) / 256))
    sel = torch.from_numpy(parts[part])
    sb = (torch.arange(n + 1, dtype=torch.float32) / n)[None].expand(LATTICE_RAYS, -1).contiguous()
    expect = (u_all[sel])[None].expand(LATTICE_RAYS, -1).contiguous()       # sb is the identity on the lattice
    return _exact(f"lattice-{n}-{part}", n, torch.zeros(LATTICE_RAYS, n), sb, u_all[sel].contiguous(), 1.0 / n, expect,
                  torch.zeros(LATTICE_RAYS, n), shared=(n == 256))


def lattice_parts(n):
    return math.ceil((2 * n + 1) / 256)


@functools.lru_cache(maxsize=None)
def single_bin(n):
    """histogram_padding = 0 and one saturated sample k per ray (density 1e30: w_k = 1, every other weight 0, in fp32 and in
    float64), k over {0, EPL - 1, EPL, 63 EPL, n - 1}: the CDF is 0 up to k and 1 after it.  u = (0, 0.5, 1.0) -> sb[k] (a
    side="left" search or a descent that stops early gives sb[0]), (sb[k] + sb[k+1]) / 2, and sb[n] through pos = n, both
    clamps and nan_to_num(0 / 0).  The bins are distinct multiples of 2^-13, so the mid-point is exact however it is formed."""
    epl = epl_of(n)
    ks = sorted({k for k in (0, epl - 1, epl, 63 * epl, n - 1) if k < n})
    g = torch.Generator().manual_seed(n)
    sb = torch.sort(torch.randperm(1 << 13, generator=g)[: n + 1].float() / (1 << 13)).values[None].expand(len(ks), -1).contiguous()
    dens, expect_w = torch.zeros(len(ks), n), torch.zeros(len(ks), n)
    expect = torch.empty(len(ks), 3)
    for r, k in enumerate(ks):
        dens[r, k], expect_w[r, k] = 1e30, 1.0
        expect[r] = torch.stack([sb[r, k], (sb[r, k] + sb[r, k + 1]) / 2, sb[r, n]])
    c = _exact(f"single-{n}", n, dens, sb, torch.tensor([0.0, 0.5, 1.0]), 0.0, expect, expect_w)
    assert c.ref.idx.tolist() == ks
    return c


TOLERANCED = {**{f"plain-{n}-{m}": functools.partial(toleranced, n, m) for n, m in SHAPES},
              **{f"{v}-{n}-{m}": functools.partial(toleranced, n, m, v) for v, n, m in VARIANTS}}
EXACT = {**{f"lattice-{n}-{p}": functools.partial(lattice, n, p) for n in (64, 128, 256) for p in range(lattice_parts(n))},
         **{f"single-{n}": functools.partial(single_bin, n) for n in (65, 192, 256)}}
ALL = {**TOLERANCED, **EXACT}


def check_coverage():
    """every n and every m at least twice, every EPL, every 64-multiple of m + 1, EPL = 1 below 64, m > n, m < n"""
    ns, ms = [n for n, _ in SHAPES], [m for _, m in SHAPES]
    assert all(ns.count(n) >= 2 for n in N_ALL) and all(ms.count(m) >= 2 for m in M_ALL)
    assert (256, 255) in SHAPES and any(m > n for n, m in SHAPES) and any(m < n for n, m in SHAPES)
    cases = [f() for f in ALL.values()]
    assert {c.epl for c in cases} == {1, 2, 3, 4} and any(c.epl == 1 and c.n < 64 for c in cases)
    assert {c.nb for c in cases if c.nb % 64 == 0} == {64, 128, 192, 256}
    assert {c.n for c in cases if c.variant == "shared" and c.family == "toleranced"} == {100, 130, 256}
    assert any(c.spacing == 1 for c in cases) and any(c.sb.dim() == 2 and c.sb.shape[1] == c.n + 1 + WIDE_EXTRA for c in cases)


@functools.lru_cache(maxsize=None)
def measure_chain32():
    """-> (worst weight error of chain32 / weight bound, worst |cdf(chain32) - cdf(float64)|) over the toleranced cases"""
    wr, ce = 0.0, 0.0
    for f in TOLERANCED.values():
        c = f()
        got = chain32(c.dens, c.sb_rows, c.u, c.near, c.far, c.spacing, c.pad, c.eps)
        live = c.wb > 0
        wr = max(wr, ((got.weights.double() - c.ref.weights).abs()[live] / c.wb[live]).max().item())
        ce = max(ce, (got.cdf.double() - c.ref.cdf).abs().max().item())
    return wr, ce
