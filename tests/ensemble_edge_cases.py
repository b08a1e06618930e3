"""Hand-placed cases for the fused ensemble reduce (plain module: tests import it; nothing here needs a GPU).

csrc/unerf_nerf.hip, section 8: ensemble_reduce_kernel gives a thread to a (view, key, element).  Blocks are dealt
blockIdx.x = ((g n_used + k) 8 + x) over the keys something is asked of, element p = ((t / n_used) 8 + x) 256 + tid: the
first 2048 elements of every key are group g = 0.  A key's channels go through moments_of<4> as long as four are left, then
moments_of<3> for exactly three, else moments_of<1>; the member loop is unrolled by 4 (NC > 1) or 8 (NC = 1), body and tail.  The
thread keeps running channel sums (reset at channel 0) for the derived keys and forms the aleatoric term from ANOTHER key's
sources, with that key's own width and stride.  The cases take their shapes from that: n on both sides of 2048 and 4096, keys of
different lengths in one launch with an unused key between used ones, every body / tail split of both unrolls, every channel
walk, the ABI's limits, aux keys that differ from their key in width, stride and use.

A case names its keys so that the aleatoric key of `k` is `k + "_var"` (what ops.ensemble_reduce expects); its plan is a list of
(output name, statistic, key) in ensemble.reduce_plan's form.  A key's M sources of one view are channel slices [lo, lo + C) of
one [M, n, W] tensor: W = C is the contiguous layout, W > C the slice of wider rows.  views(case, device) hands them out.

reference64: every planned block from the float32 inputs in float64, by the formulas of include/unerf.h (UNERF_ENS_*):
  mean = sum_j x_j / M, var = sum_j (x_j - mean)^2 / (M - 1) (NaN at M = 1), var_cmean = cmean(var),
  alea_cmean = cmean(mean of key + "_var"), epi_plus_alea their sum, sqrt_epi_plus_alea its root, std_cmean = cmean(sqrt(var)),
  cmean = the sum over the key's channels / C.

bounds, per element, from the reference's own conditioning (nothing here comes from a GPU result); u = U24 = 2^-24:
  mean       e_m = (M + 2) u mean_j |x_j|: M - 1 additions of partial sums no larger than sum |x_j| and one division
             (composite_cases.stack_moments, restated for a list of sources).
  var        e_v = [2 sqrt(Q M e_m^2) + M e_m^2] / (M - 1) + MOM_EPS Q / (M - 1), Q = sum_j (x_j - mean)^2: the kernel is
             two-pass, every deviation carries the computed mean's error e_m (Cauchy-Schwarz on sum 2 d_j e_m, plus the squares);
             MOM_EPS Q covers the roundings of the subtractions, squares, the M - 1 additions and the division.
  var_cmean  cmean(e_v) + (C + 1) u cmean(var): the channel mean of C exact terms rounds C - 1 additions and one division, each
             on a partial sum of non-negative terms <= the total, so C u cmean; the + 1 holds the second-order product with e_v.
  alea_cmean cmean(e_m of the aux key) + (C_aux + 1) u cmean(|mean of the aux key|): the same, on terms of either sign.
  epi_plus_alea        the two bounds above + u |epi + alea|: a sum adds one rounding.
  sqrt of a value a known to b:  r(a, b) = min(b / (2 sqrt(a)), sqrt(b)) + u sqrt(a).  sqrt(a + d) - sqrt(a) = d / (sqrt(a + d)
             + sqrt(a)): to first order d / (2 sqrt(a)), and never more than sqrt(|d|), which keeps the bound finite as a -> 0
             (identical members: a = 0, b > 0); u sqrt(a) is the correctly rounded root's own rounding.
  sqrt_epi_plus_alea   r(epi + alea, its bound).
  std_cmean  cmean_c r(var_c, e_v,c) + (C + 1) u cmean(sqrt(var)).
An element whose reference is not finite (a planted NaN or inf, var at M = 1) has no bound: the kernel must show the same
non-finite value there (NaN for NaN, the same infinity); composite_cases._nan_rule holds the placement.

restate32 states the kernel's order of operations in numpy float32 (sources added in member order, s / M, squared deviations in
member order, / (M - 1); channel sums in channel order, IEEE divide and sqrt), reading every source through its descriptor
(base + p stride + c) as the kernel does.  The CPU test holds it to the bounds -- they come from the derivations above, and a
restatement outside one would mean a derivation is wrong -- and shows that planted wrong restatements (MUTANTS) miss them.
block_owner states the block dealing; the CPU test shows that the "groups" cases separate its mutants.

The exact family (identical members on a 2^-10 grid: every partial sum, M x and x - x are exact) is compared bit for bit."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from composite_cases import MOM_EPS, U24, _nan_rule

STATS = ("mean", "var", "var_cmean", "alea_cmean", "epi_plus_alea", "sqrt_epi_plus_alea", "std_cmean")   # UNERF_ENS_* order
ALEA_STATS = ("alea_cmean", "epi_plus_alea", "sqrt_epi_plus_alea")
VAR_STATS = ("var", "var_cmean", "epi_plus_alea", "sqrt_epi_plus_alea", "std_cmean")
XCDS, BLOCK = 8, 256
MAX_KEYS, MAX_MEMBERS, MAX_CHANNELS, MAX_VIEWS = 32, 64, 64, 16
M_UNROLL = (3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64)
C_WALK = (2, 5, 6, 7, 8, 64)
M_EXACT = (2, 4, 8, 64)
N_GROUPS = (2047, 2048, 2049, 4097)
MUTANTS = ("one_pass", "restart_at_U", "skip_tail", "no_reset", "reset_each_group", "div3", "aux_key_stride")


def aux_of(stat, key):
    return key + "_var" if stat in ALEA_STATS else None


def coded_plan(plan, codes):
    """the plan in the form test_gpu_ensemble_batch._reduce takes: (name, lib.ENS_* code, key, aux key or None)"""
    return [(name, codes[stat], key, aux_of(stat, key)) for name, stat, key in plan]


# ---- cases -------------------------------------------------------------------------------------------------------------

def _key(n, C, W=None, lo=0, fill="randn"):
    W = C if W is None else W
    assert lo + C <= W
    return SimpleNamespace(n=n, C=C, W=W, lo=lo, fill=fill)


def _all(key, aux=False):
    """every statistic of `key` (the alea ones with aux)"""
    return [(f"{key}/{s}", s, key) for s in STATS if aux or s not in ALEA_STATS]


def _case(name, family, B, M, keys, plan, seed=0, planted=(), identical=False):
    for _, stat, k in plan:
        assert k in keys and (stat not in ALEA_STATS or (k + "_var" in keys and keys[k + "_var"].n == keys[k].n)), (name, stat, k)
    assert len(keys) <= MAX_KEYS and M <= MAX_MEMBERS and B <= MAX_VIEWS and all(k.C <= MAX_CHANNELS for k in keys.values())
    return SimpleNamespace(name=name, family=family, B=B, M=M, keys=keys, plan=plan, seed=seed, planted=tuple(planted),
                           identical=identical)


def _fill(kind, g, M, n, W):
    """[M, n, W] float32.  randn: N(1, 1/4), either sign.  pos: 0.05 + |N(0, 1)|, what a variance key holds.  stack:
    composite_cases.stack_moments' pattern, 900 + 1e-3 randn in the first half of the channels (a small spread on a large value),
    randn in the others.  decades: channel c spans 1e-6 .. 1e6, positive.  grid: multiples of 2^-10 away from zero, positive for
    a `_var` key (gridpos)."""
    x = torch.randn(M, n, W, generator=g)
    if kind == "randn":
        return 1.0 + 0.5 * x
    if kind == "pos":
        return 0.05 + x.abs()
    if kind == "stack":
        h = max(W // 2, 1)
        x[..., :h] = 900.0 + 1e-3 * x[..., :h]
        return x
    if kind == "decades":
        scale = 10.0 ** torch.linspace(-6, 6, W) if W > 1 else torch.ones(1)
        return (scale * (0.5 + torch.rand(M, n, W, generator=g))).float()
    if kind in ("grid", "gridpos"):
        x = torch.round(x * 1024) / 1024
        x = torch.where(x == 0, torch.full_like(x, 2.0 ** -10), x)
        return x.abs() if kind == "gridpos" else x
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def storage(name):
    """-> [view]{key: [M, n, W] float32 on the CPU}; never written after it is made"""
    c = CASES[name]
    g = torch.Generator().manual_seed(1000 + c.seed)
    out = []
    for v in range(c.B):
        view = {}
        for k, d in c.keys.items():
            x = _fill(d.fill, g, 1 if c.identical else c.M, d.n, d.W)
            view[k] = x.expand(c.M, d.n, d.W).contiguous() if c.identical else x
        for (pv, k, j, p, ch, value) in c.planted:
            if pv == v:
                view[k][j, p, c.keys[k].lo + ch] = value
        out.append(view)
    return out


def views(case, device=None):
    """views[v][key] = the M sources [n, C]: slices of the case's storage (moved to `device` whole, so the strides stay)"""
    out = []
    for view in storage(case.name):
        vw = {}
        for k, d in case.keys.items():
            base = view[k] if device is None else view[k].to(device)
            vw[k] = [base[j, :, d.lo:d.lo + d.C] for j in range(case.M)]
            assert vw[k][0].shape == (d.n, d.C) and (d.n <= 1 or vw[k][0].stride(0) == d.W)
        out.append(vw)
    return out


def _build_cases():
    cs = []
    add = lambda *a, **kw: cs.append(_case(*a, **kw))
    # groups: 2048 = 8 x 256 is one full group, element 2048 the first of g = 1, 4097 reaches g = 2
    for n in N_GROUPS:
        add(f"groups-n{n}", "groups", 1, 3, {"x": _key(n, 1)}, _all("x"), seed=n)
    # one launch, keys of n = 1, 300, 2049, 4097; `skip` (n = 2049, nothing asked) and `mid_var` (n = 2049, aux only) are not
    # in used[], so behind them the position in used[] differs from the key index.  `long` is a slice of 8-wide rows.
    mixed = {"short": _key(300, 3), "short_var": _key(300, 3, fill="pos"), "long": _key(4097, 3, W=8, lo=4),
             "skip": _key(2049, 1), "one": _key(1, 3), "mid": _key(2049, 1), "mid_var": _key(2049, 1, fill="pos")}
    mixed_plan = (_all("short", aux=True) + [("short_var/mean", "mean", "short_var")] + _all("long") + _all("one")
                  + _all("mid", aux=True))
    orders = {"mid": ["short", "short_var", "long", "skip", "one", "mid", "mid_var"],
              "first": ["long", "short", "skip", "short_var", "one", "mid_var", "mid"],
              "last": ["one", "short", "skip", "mid", "short_var", "mid_var", "long"]}
    for tag, order in orders.items():
        add(f"groups-mixed-longest-{tag}", "groups", 3, 3, {k: mixed[k] for k in order}, mixed_plan, seed=7)
    # member unroll: the bodies and tails of both widths (8 for the single-channel path, 4 for the 3- and 4-channel groups)
    for M in M_UNROLL:
        keys = {"c1": _key(257, 1), "c3": _key(257, 3), "c4": _key(257, 4)}
        add(f"unroll-M{M}", "unroll", 1, M, keys, _all("c1") + _all("c3") + _all("c4"), seed=M)
    # channel walk: 4s, then a 3, else singles -- for the key and for its aux key
    for C in C_WALK:
        add(f"walk-C{C}", "walk", 1, 5, {"x": _key(257, C), "x_var": _key(257, C, fill="pos")}, _all("x", aux=True), seed=C)
    # limits of the ABI
    widths = (1, 3, 4, 2)
    keys = {f"k{i:02d}": _key(35, widths[i % 4]) for i in range(MAX_KEYS)}
    add("limit-keys32", "limits", 2, 3, keys, [e for k in keys for e in _all(k)], seed=32)
    add("limit-M64-C64", "limits", 1, MAX_MEMBERS, {"x": _key(35, MAX_CHANNELS)}, _all("x"), seed=64)
    add("limit-B16", "limits", MAX_VIEWS, 3, {"x": _key(257, 3), "x_var": _key(257, 1, fill="pos")}, _all("x", aux=True), seed=16)
    # aux shapes: a C = 3 key with aux keys of other widths, strides and uses
    aux_mean = [("a_var/mean", "mean", "a_var")]
    for tag, a, av, plan in (
            ("c1", _key(257, 3), _key(257, 1, fill="pos"), _all("a", aux=True) + aux_mean),
            ("c3", _key(257, 3), _key(257, 3, fill="pos"), _all("a", aux=True) + aux_mean),
            ("c4", _key(257, 3), _key(257, 4, fill="pos"), _all("a", aux=True) + aux_mean),
            ("slice-of-8", _key(257, 3), _key(257, 3, W=8, lo=5, fill="pos"), _all("a", aux=True) + aux_mean),
            ("key-slice-of-8", _key(257, 3, W=8, lo=1), _key(257, 3, fill="pos"), _all("a", aux=True) + aux_mean),
            ("unasked", _key(257, 3), _key(257, 3, fill="pos"), _all("a", aux=True)),
            ("alea-only", _key(257, 3), _key(257, 3, fill="pos"), [("a/alea_cmean", "alea_cmean", "a")])):
        add(f"aux-{tag}", "aux", 2, 5, {"a": a, "a_var": av}, plan, seed=len(tag))
    # values: a small spread on a large value in the 1-, 3- and 4-channel groups; decades across the channels
    for M in (5, 9):
        keys = {"s1": _key(257, 1, fill="stack"), "s3": _key(257, 3, W=6, fill="stack"), "s6": _key(257, 6, fill="stack"),
                "s8": _key(257, 8, fill="stack")}
        add(f"values-stack-M{M}", "values", 1, M, keys, [e for k in keys for e in _all(k)], seed=900 + M)
    add("values-decades", "values", 1, 5, {"d": _key(257, 7, fill="decades"), "d_var": _key(257, 7, fill="decades")},
        _all("d", aux=True), seed=77)
    # exact: identical members
    for M in M_EXACT:
        keys = {"e1": _key(257, 1, fill="grid"), "e1_var": _key(257, 1, fill="gridpos"), "e3": _key(257, 3, W=8, lo=2, fill="grid"),
                "e3_var": _key(257, 3, fill="gridpos"), "e7": _key(257, 7, fill="grid"), "e7_var": _key(257, 4, fill="gridpos")}
        add(f"exact-M{M}", "exact", 2, M, keys, _all("e1", aux=True) + _all("e3", aux=True) + _all("e7", aux=True), seed=M,
            identical=True)
    # non-finite: one NaN / +inf in ONE member at single elements -- element 0, the last element of a block, element 2048 of
    # the long key (the first of g = 1); (view, key, member, element, channel, value)
    nan, inf = float("nan"), float("inf")
    keys = {"long": _key(2049, 1), "c3": _key(257, 3), "c3_var": _key(257, 3, fill="pos")}
    planted = [(0, "long", 2, 0, 0, nan), (0, "long", 2, 2048, 0, nan), (0, "long", 3, 255, 0, inf), (0, "long", 0, 2047, 0, inf),
               (0, "c3", 0, 255, 1, nan), (0, "c3", 4, 256, 2, inf), (0, "c3", 1, 0, 0, inf),
               (0, "c3_var", 4, 3, 0, nan), (0, "c3_var", 2, 7, 2, inf)]
    add("nonfinite", "nonfinite", 1, 5, keys, _all("long") + _all("c3", aux=True) + [("c3_var/mean", "mean", "c3_var")],
        seed=5, planted=planted)
    # M = 1: var, var_cmean, std_cmean, epi_plus_alea, sqrt_epi_plus_alea are NaN, mean and alea_cmean finite
    add("single-member", "single", 2, 1, {"a": _key(257, 3), "a_var": _key(257, 3, fill="pos"), "d": _key(257, 1)},
        _all("a", aux=True) + _all("d"), seed=1)
    assert len({c.name for c in cs}) == len(cs)
    return {c.name: c for c in cs}


CASES = _build_cases()


def of_family(*families):
    return [n for n, c in CASES.items() if c.family in families]


# ---- float64 reference and bounds ----------------------------------------------------------------------------------------

def _cmean(t):
    return t.sum(dim=-1, keepdim=True) / t.shape[-1]


def _sqrt_bound(a, b):
    """a value a >= 0 known to within b -> its correctly rounded fp32 root to within min(b / (2 sqrt(a)), sqrt(b)) + u sqrt(a)"""
    ra = a.sqrt()
    first = torch.where(a > 0, b / (2 * ra), torch.full_like(b, float("inf")))
    return torch.minimum(first, b.sqrt()) + U24 * ra


def _moments64(srcs):
    x = torch.stack([t.double() for t in srcs])        # [M, n, C], read through the strided views
    M = x.shape[0]
    mean = x.mean(0)
    e_m = (M + 2) * U24 * x.abs().mean(0)
    if M == 1:
        return mean, torch.full_like(mean, float("nan")), e_m, torch.full_like(mean, float("nan"))
    Q = ((x - mean) ** 2).sum(0)
    e_v = (2 * torch.sqrt(Q * M * e_m ** 2) + M * e_m ** 2) / (M - 1) + MOM_EPS * Q / (M - 1)
    return mean, Q / (M - 1), e_m, e_v


def _reference_and_bounds(vws, plan):
    ref, bnd = [], []
    for view in vws:
        mom = {}
        r, b = {}, {}
        for name, stat, k in plan:
            for kk in (k, aux_of(stat, k)):
                if kk is not None and kk not in mom:
                    mom[kk] = _moments64(view[kk])
            mean, var, e_m, e_v = mom[k]
            C = mean.shape[-1]
            epi, e_epi = _cmean(var), _cmean(e_v) + (C + 1) * U24 * _cmean(var)
            if stat in ALEA_STATS:
                am, _, a_em, _ = mom[k + "_var"]
                Ca = am.shape[-1]
                alea, e_alea = _cmean(am), _cmean(a_em) + (Ca + 1) * U24 * _cmean(am.abs())
                tot, e_tot = epi + alea, e_epi + e_alea + U24 * (epi + alea).abs()
            if stat == "mean":
                r[name], b[name] = mean, e_m
            elif stat == "var":
                r[name], b[name] = var, e_v
            elif stat == "var_cmean":
                r[name], b[name] = epi, e_epi
            elif stat == "alea_cmean":
                r[name], b[name] = alea, e_alea
            elif stat == "epi_plus_alea":
                r[name], b[name] = tot, e_tot
            elif stat == "sqrt_epi_plus_alea":
                r[name], b[name] = tot.sqrt(), _sqrt_bound(tot, e_tot)
            elif stat == "std_cmean":
                r[name], b[name] = _cmean(var.sqrt()), _cmean(_sqrt_bound(var, e_v)) + (C + 1) * U24 * _cmean(var.sqrt())
            else:
                raise KeyError(stat)
        ref.append(r)
        bnd.append(b)
    return ref, bnd


def reference64(vws, plan):
    """-> [view]{output name: float64 [n, C_out]} from the float32 sources (CPU tensors, any strides)"""
    return _reference_and_bounds(vws, plan)[0]


def bounds(vws, plan):
    """-> [view]{output name: float64 [n, C_out]}: the module docstring's bounds.  NaN where the reference is not finite."""
    return _reference_and_bounds(vws, plan)[1]


@functools.lru_cache(maxsize=None)
def reference(name):
    """a case's (reference64, bounds), computed once and shared"""
    c = CASES[name]
    return _reference_and_bounds(views(c), c.plan)


def ratios(ref, bnd, got):
    """one view's results {output name: float32 [n, C_out] on the CPU} against its reference -> {output name: worst error /
    bound}; inf where the NaN placement or a non-finite value differs, or a block is missing or misshapen"""
    out = {}
    for name, want in ref.items():
        g = got.get(name)
        if g is None or tuple(g.shape) != tuple(want.shape) or g.dtype != torch.float32:
            out[name] = float("inf")
            continue
        g = g.double()
        fin = torch.isfinite(want)
        same = torch.where(fin, torch.isfinite(g), (g == want) | (torch.isnan(g) & torch.isnan(want)))
        if not bool(same.all()):
            out[name] = float("inf")
            continue
        err, b = (g - want).abs()[fin], bnd[name][fin]
        if bool((err > b).any()) and bool((b[err > b] == 0).any()):
            out[name] = float("inf")
            continue
        live = b > 0
        out[name] = float((err[live] / b[live]).max()) if bool(live.any()) else 0.0
    return out


def hold(case_name, ref, bnd, got, what=""):
    """asserts one view's results within the bounds, no element left out -> {statistic: worst error / bound}"""
    worst = {}
    for name, want in ref.items():
        assert name in got, f"{case_name}{what}: no block {name}"
        g = got[name].detach().cpu()
        assert g.dtype == torch.float32 and tuple(g.shape) == tuple(want.shape), (case_name, name, tuple(g.shape))
        _nan_rule(f"{case_name}{what} {name}", g.double(), want)
    for name, r in ratios(ref, bnd, {k: v.detach().cpu() for k, v in got.items()}).items():
        if not r <= 1.0:
            g, want = got[name].detach().cpu().double(), ref[name]
            fin = torch.isfinite(want) & torch.isfinite(g)
            over = torch.nonzero(~fin & ~((g == want) | (torch.isnan(g) & torch.isnan(want))) | (fin & ((g - want).abs() > bnd[name])))
            i = tuple(over[0].tolist())
            raise AssertionError(f"{case_name}{what}: {name} beyond its bound at {over[:8].tolist()}, worst error / bound {r:.3g} "
                                 f"(got {g[i].item()!r}, reference {want[i].item()!r}, bound {bnd[name][i].item():.3e})")
        stat = name.rsplit("/", 1)[-1]
        worst[stat] = max(worst.get(stat, 0.0), r)
    return worst


def stat_of(case):
    return {name: stat for name, stat, _ in case.plan}


def worst_by_stat(case, per_name):
    out = {}
    for name, r in per_name.items():
        s = stat_of(case)[name]
        out[s] = max(out.get(s, 0.0), r)
    return out


# ---- the exact family ----------------------------------------------------------------------------------------------------

def exact_expected(case):
    """identical members on a 2^-10 grid: mean == x, every variance and epistemic term +0, alea the fp32 channel mean of the aux
    member (channel order, IEEE divide), epi_plus_alea == alea (0 + alea), sqrt_epi_plus_alea == sqrtf(alea)
    -> [view]{output name: float32 [n, C_out]}"""
    assert case.identical
    out = []
    for view in views(case):
        e = {}
        for name, stat, k in case.plan:
            x = view[k][0].numpy()
            if stat == "mean":
                e[name] = x.copy()
            elif stat == "var":
                e[name] = np.zeros_like(x)
            elif stat in ("var_cmean", "std_cmean"):
                e[name] = np.zeros((x.shape[0], 1), np.float32)
            else:
                a = view[k + "_var"][0].numpy()
                s = a[:, 0].copy()
                for c in range(1, a.shape[1]):
                    s = s + a[:, c]
                alea = (s / np.float32(a.shape[1]))[:, None]
                e[name] = np.sqrt(alea) if stat == "sqrt_epi_plus_alea" else alea
            assert e[name].dtype == np.float32
        out.append({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in e.items()})
    return out


# ---- fp32 restatement of the kernel's order of operations (CPU) ----------------------------------------------------------------

def channel_groups(C):
    """the channel walk of ens_element -> [(first channel, channels of the group)]: 4s, then a 3, else singles"""
    out, c = [], 0
    while C - c >= 4:
        out.append((c, 4))
        c += 4
    if C - c == 3:
        out.append((c, 3))
        return out
    return out + [(cc, 1) for cc in range(c, C)]


def _flat(t):
    return torch.empty(0, dtype=torch.float32).set_(t.untyped_storage()).numpy()


def _read(t, stride, c):
    """channel c of every element of source t as the kernel reads it: base[p stride + c] (an index a wrong stride pushes past
    the storage is wrapped, so that a mutant reads other values, not other memory)"""
    flat = _flat(t)
    idx = t.storage_offset() + np.arange(t.shape[0], dtype=np.int64) * stride + c
    return flat[idx % flat.shape[0]]


def _stride(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]     # the descriptor's row stride, as ops.ensemble_reduce sets it


def _moments32(srcs, stride, c, U, want_var, mutant):
    """moments_of for one channel: the loads come U sources at a time, the additions are the plain loop's"""
    M = len(srcs)
    f = np.float32
    x = [_read(t, stride, c) for t in srcs]
    body = M - M % U
    last = body if mutant == "skip_tail" else M
    s = np.zeros_like(x[0])
    for j in range(last):
        s = s + x[j]
    with np.errstate(all="ignore"):
        mean = s / f(M)
        if not want_var:
            return mean, np.zeros_like(mean)
        if mutant == "one_pass":
            s2 = np.zeros_like(mean)
            for j in range(M):
                s2 = s2 + x[j] * x[j]
            return mean, (s2 / f(M) - mean * mean) * f(M) / f(M - 1)
        q = np.zeros_like(mean)
        for j in range(U if (mutant == "restart_at_U" and body) else 0, last):
            d = x[j] - mean
            q = q + d * d
        return mean, q / f(M - 1)


def _element32(srcs, stride, C, want_var, mutant, carry=None):
    """ens_element: every channel in walk order -> per-channel mean / var [n, C] and the running sums (sum_m, sum_v, sum_sd)"""
    f = np.float32
    means, vars_ = [], []
    sums = carry
    for c0, nc in channel_groups(C):
        for c in range(c0, c0 + nc):
            m, v = _moments32(srcs, stride, c, 8 if nc == 1 else 4, want_var, mutant)
            with np.errstate(all="ignore"):
                sd = np.sqrt(v)
                first = (c == c0) if mutant == "reset_each_group" else (c == 0 and mutant != "no_reset")
                if first or sums is None:
                    sums = (m, v, sd)
                else:
                    sums = (sums[0] + m, sums[1] + v, sums[2] + sd)
            means.append(m)
            vars_.append(v)
    return np.stack(means, -1).astype(f), np.stack(vars_, -1).astype(f), sums


def restate32(vws, plan, mutant=None):
    """-> [view]{output name: float32 [n, C_out]}: the kernel's arithmetic in numpy float32.  mutant (MUTANTS) plants one wrong
    statement:
      one_pass          var = (E[x^2] - m^2) M / (M - 1)
      restart_at_U      the variance pass starts at member U instead of 0 when the unroll had a body
      skip_tail         the members behind the last full group of U are left out of both passes
      no_reset          the `first` reset of the running channel sums dropped: the sums of the key's walk run on into the walk
                        over its aux key (zero-initialised sums hide the missing reset inside one walk, so this is where it shows)
      reset_each_group  the reset at the first channel of EVERY group, c == 0 in place of c0 + c == 0
      div3              the channel means divided by 3 whatever C is
      aux_key_stride    the aux key's sources read with the key's row stride"""
    assert mutant is None or mutant in MUTANTS
    f = np.float32
    out = []
    for view in vws:
        asked = {}
        for name, stat, k in plan:
            asked.setdefault(k, {})[stat] = name
        res = {}
        for k, st in asked.items():
            srcs = view[k]
            C = srcs[0].shape[1]
            want_var = any(s in VAR_STATS for s in st)
            mean, var, sums = _element32(srcs, _stride(srcs[0]), C, want_var, mutant)
            div = f(3 if mutant == "div3" else C)
            with np.errstate(all="ignore"):
                epi = sums[1] / div
                std = sums[2] / div
            put = lambda s, a: res.__setitem__(st[s], torch.from_numpy(np.ascontiguousarray(a.reshape(len(a), -1)))) if s in st else None
            put("mean", mean)
            put("var", var)
            put("var_cmean", epi)
            put("std_cmean", std)
            if any(s in ALEA_STATS for s in st):
                aux = view[k + "_var"]
                Ca = aux[0].shape[1]
                a_stride = _stride(srcs[0]) if mutant == "aux_key_stride" else _stride(aux[0])
                _, _, asums = _element32(aux, a_stride, Ca, False, mutant, carry=sums if mutant == "no_reset" else None)
                with np.errstate(all="ignore"):
                    alea = asums[0] / f(3 if mutant == "div3" else Ca)
                    tot = epi + alea
                    put("alea_cmean", alea)
                    put("epi_plus_alea", tot)
                    put("sqrt_epi_plus_alea", np.sqrt(tot))
        out.append({name: res[name] for name, _, _ in plan})
    return out


# ---- the block dealing -----------------------------------------------------------------------------------------------------

def grid_blocks(ns):
    """blocks of one view's launch over used keys of ns elements: the longest key's blocks rounded up to whole groups of 8"""
    most = max((n + BLOCK - 1) // BLOCK for n in ns)
    return (most + XCDS - 1) // XCDS * XCDS * len(ns)


def block_owner(block, n_used, ns, mutant=None, n_keys=None):
    """which elements block index `block` owns: (position in used[], first element, one past the last), or None for a surplus
    block of a short key.  ns[i] = the elements of used[i].  The documented dealing: 8 XCD slots, keys innermost within a
    group -- block = (g n_used + i) 8 + x owns elements [(8 g + x) 256, + 256) of used[i].
    mutant: "drop_g" (the element index without its group term), "n_keys" (the launch's key count n_keys where n_used
    belongs; used[] is zero-filled behind n_used, and position 0 is taken to be key 0), "slots7" (the element index strides its
    groups by 7 slots while the blocks are dealt over 8; 7 in BOTH places, host grid included, is only another dealing)."""
    x, t = block % XCDS, block // XCDS
    per = n_keys if mutant == "n_keys" else n_used
    i, g = t % per, t // per
    if i >= n_used:
        i = 0
    p = ((0 if mutant == "drop_g" else g) * (7 if mutant == "slots7" else XCDS) + x) * BLOCK
    return None if p >= ns[i] else (i, p, min(p + BLOCK, ns[i]))


def ownership(ns, mutant=None, n_keys=None):
    """-> per used key, how many blocks of the launch own each element"""
    count = [np.zeros(n, np.int64) for n in ns]
    for b in range(grid_blocks(ns)):
        o = block_owner(b, len(ns), ns, mutant, n_keys)
        if o is not None:
            count[o[0]][o[1]:o[2]] += 1
    return count


def used_ns(case):
    """(elements of the keys something is asked of, in key order; keys in the launch)"""
    used = {k for _, _, k in case.plan}
    return [d.n for k, d in case.keys.items() if k in used and d.n > 0], len(case.keys)
