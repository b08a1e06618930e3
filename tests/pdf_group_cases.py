"""Cases for the lane-group form of the PDF resampler (plain module: tests import it; nothing here needs a GPU).

pdf_group_kernel<EPL> (csrc/unerf_nerf.hip, section 4) gives a ray a group of 16 lanes -- a wave holds four rays, a block
trip sixteen -- and lane l of the group the samples [l EPL, (l + 1) EPL) with EPL = ceil(n / 16); the host takes it up to
n = 128 and the wave-per-ray pdf_kernel above (`lanes_per_ray` restates its rule).  The three scans, the sums and the median
count stay inside the group, and the m + 1 outputs are walked 16 at a time.  The cases put n and m + 1 on both sides of every
multiple of 16 and 32 (and n on both sides of the rule's own border and at the ABI's end, 256), the median on both sides of
the lane borders of the layout the host selects, and give the rays of one wave different kinds of data (all zero,
saturated, an inf, a NaN entering the scan mid-ray).

The reference, the bounds, the tie rule and the comparison are tests/pdf_cases.py's own (`reference`, `weight_bound`,
`bin_bound`, `ties`, `hold`): float64 on the fp32 oracle's Euclidean edges, bounds from the reference's conditioning with
EPS_CDF "allowing for another summation order".  Nothing here widens them and nothing comes from a GPU result."""
import functools
from types import SimpleNamespace

import torch

import pdf_cases as PC
from oracle import nerf_oracle as O

R = PC.R
# n: 15 16 17 31 32 33 47 48 49 95 96 97 112 113 128 240 241 255 256; m: 15 16 17 31 32 33 47 48 49 96; the workload's own
# (256, 96) and (96, 48).  Each builds with pdf_cases.toleranced(n, m) and its "shared" variant with ZERO tie rays at the
# default seed (MAX_TIES at R = 37 allows none): test_pdf_group_cases_cpu.py asserts it for every entry.
SHAPES = ((15, 16), (16, 15), (17, 31), (31, 32), (32, 33), (33, 17), (47, 48), (48, 49), (49, 47), (95, 48), (96, 48), (96, 31),
          (96, 47), (96, 49), (97, 96), (112, 48), (113, 96), (128, 96), (240, 96), (241, 96), (255, 96), (256, 96))
N_ALL = (15, 16, 17, 31, 32, 33, 47, 48, 49, 95, 96, 97, 112, 113, 128, 240, 241, 255, 256)
M_ALL = (15, 16, 17, 31, 32, 33, 47, 48, 49, 96)
# rays of a call: one live group in a wave, all but one, a full wave and one more, two waves and one more group (9), a
# block's second trip with a single group (17), a second block with a single group (33)
SHORT_R = (1, 2, 3, 4, 5, 7, 8, 9, 17, 33)
MEDIAN_SHAPES = ((96, 48), (128, 33), (113, 31), (256, 96), (241, 47), (33, 16))
MIXED_SHAPES = ((96, 48), (256, 96), (47, 17), (130, 64))


def lanes_per_ray(n):
    """the host's rule (pdf_lanes_per_ray in csrc/unerf_nerf.hip): 16 = pdf_group_kernel, 64 = the wave-per-ray pdf_kernel"""
    return 16 if n <= 128 else 64


def group_epl(n):
    g = lanes_per_ray(n)
    return (n + g - 1) // g


def _finish(c):
    """float64 reference, bounds and tie rays, by pdf_cases' own functions and under its MAX_TIES rule"""
    c.epl, c.nb = group_epl(c.n), c.m + 1
    c.ref = PC.reference(c.dens, c.sb_rows, c.u, c.near, c.far, c.spacing, c.pad, c.eps)
    c.wb = PC.weight_bound(c.ref)
    c.tie = PC.ties(c.ref, c.wb)
    assert c.tie.sum().item() <= PC.MAX_TIES * c.dens.shape[0], f"{c.name}: {c.tie.sum().item()} tie rays"
    c.bb, c.K = PC.bin_bound(c.ref, c.sb_rows, c.u)
    assert torch.isfinite(c.K).all() and torch.isfinite(c.bb).all(), f"{c.name}: a flat CDF interval"
    return c


def _case(name, n, m, dens, sb, shared=False):
    c = SimpleNamespace(name=name, family="toleranced", variant="shared" if shared else None, n=n, m=m, dens=dens, sb_rows=sb,
                        sb=sb[0].clone() if shared else sb, u=O.pdf_u(m), near=PC.NEAR, far=PC.FAR, spacing=0, pad=PC.PAD,
                        eps=PC.EPS)
    return _finish(c)


def median_slots(n):
    """sample indices on both sides of a lane border of the layout the host selects for n (EPL = ceil(n / lanes_per_ray)):
    lanes 0 | 1, lanes 7 | 8, lanes 15 | 16 (the DPP row border of the wave-per-ray form; past the ray's end in a 16-lane
    group) and the last lane that holds samples, whose run may be ragged"""
    epl = group_epl(n)
    last_lane = (n - 1) // epl
    ks = {epl - 1, epl, 8 * epl - 1, 8 * epl, 16 * epl - 1, 16 * epl, last_lane * epl - 1, last_lane * epl, n - 1}
    return sorted(k for k in ks if 0 <= k < n)


@functools.lru_cache(maxsize=None)
def group_medians(n, m, shared=False):
    """ray i (i < len(median_slots)) has its median planted on sample median_slots(n)[i]: zero density before it, optical
    depth 2 on it (w = 0.86); the other rays are the seeded random ones"""
    g = torch.Generator().manual_seed(7919 * n + m)
    dens = torch.exp(torch.randn(R, n, generator=g) * 2.5)
    sb = torch.sort(torch.rand(R, n + 1, generator=g), dim=-1).values
    if shared:
        sb = sb[5:6].expand(R, -1).contiguous()
    eb = O.spacing_to_euclidean(sb, PC.NEAR, PC.FAR).double()
    delta = eb[:, 1:] - eb[:, :-1]
    ks = median_slots(n)
    assert len(ks) <= R
    for r, k in enumerate(ks):
        assert delta[r, k] > 0
        dens[r, :k] = 0.0
        dens[r, k] = (2.0 / delta[r, k]).float()
    c = _case(f"median-{'shared-' if shared else ''}{n}-{m}", n, m, dens, sb, shared)
    c.planted = dict(enumerate(ks))
    for r, k in c.planted.items():
        assert c.ref.idx[r].item() == k and not c.tie[r], f"{c.name}: planted median {k} on ray {r}"
    return c


KINDS = ("zero", "saturated", "inf", "nan", "random")


@functools.lru_cache(maxsize=None)
def mixed(n, m):
    """neighbouring rays carry different kinds of data, ray i the kind KINDS[i % 5]: all zero, all 1e4, one inf, a NaN that
    enters the prefix scan mid-ray (a zero-width bin with inf density: dd = 0 * inf), random -- so that every wave of every
    group width holds each kind next to another"""
    g = torch.Generator().manual_seed(104729 * n + m)
    dens = torch.exp(torch.randn(R, n, generator=g) * 2.5)
    sb = torch.sort(torch.rand(R, n + 1, generator=g), dim=-1).values
    nan_k = n // 3
    for r in range(R):
        kind = KINDS[r % 5]
        if kind == "zero":
            dens[r] = 0.0
        elif kind == "saturated":
            dens[r] = 1e4
        elif kind == "inf":
            dens[r, (r * 7) % n] = float("inf")
        elif kind == "nan":
            sb[r, nan_k + 1] = sb[r, nan_k]
            dens[r, nan_k] = float("inf")
    c = _case(f"mixed-{n}-{m}", n, m, dens, sb)
    for r in range(R):
        if KINDS[r % 5] == "nan":
            assert torch.isnan(c.ref.dd[r, nan_k]) and (c.ref.weights[r, nan_k:] == 0).all() and (c.wb[r, nan_k:] == 0).all()
        if KINDS[r % 5] == "zero":
            assert (c.ref.weights[r] == 0).all()
    return c


SHAPE_CASES = {**{f"plain-{n}-{m}": functools.partial(PC.toleranced, n, m) for n, m in SHAPES},
               **{f"shared-{n}-{m}": functools.partial(PC.toleranced, n, m, "shared") for n, m in SHAPES}}
MEDIAN_CASES = {**{f"median-{n}-{m}": functools.partial(group_medians, n, m) for n, m in MEDIAN_SHAPES},
                **{f"median-shared-{n}-{m}": functools.partial(group_medians, n, m, True) for n, m in ((96, 48), (256, 96))}}
MIXED_CASES = {f"mixed-{n}-{m}": functools.partial(mixed, n, m) for n, m in MIXED_SHAPES}
ALL = {**SHAPE_CASES, **MEDIAN_CASES, **MIXED_CASES}


def check_coverage():
    """every n and m the group borders ask for, the workload's pairs with and without the shared row, both group widths,
    outputs that end on every residue class of interest: m + 1 = a multiple of 16 / 32, one more, one less"""
    ns, ms = {n for n, _ in SHAPES}, {m for _, m in SHAPES}
    assert ns == set(N_ALL) and ms >= set(M_ALL)
    for key in ("plain-256-96", "shared-256-96", "plain-96-48", "shared-96-48"):
        assert key in ALL
    assert {lanes_per_ray(n) for n in ns} == {16, 64} and 128 in ns      # 129: pdf_cases' own shapes
    assert {group_epl(n) for n in ns if lanes_per_ray(n) == 16} == {1, 2, 3, 4, 6, 7, 8}
    nbs = {m + 1 for m in ms}
    assert {16, 17, 18, 32, 33, 34, 48, 49, 50, 97} <= nbs
    # a ragged last lane (n no multiple of EPL) and a full one
    assert any(n % group_epl(n) for n in ns) and any(n % group_epl(n) == 0 for n in ns)
