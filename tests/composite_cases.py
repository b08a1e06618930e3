"""Hand-placed cases for the compositing stage (plain module: tests import it; nothing here needs a GPU).

csrc/unerf_nerf.hip, sections 6 and 7: composite_kernel* / composite_moments_kernel* give a 16-lane group to a ray, lane l the
samples [l SPL, (l + 1) SPL) with SPL = unerf_spl_for(S) in {1, 2, 3, 4, 6, 8, 16}; S != 16 SPL takes the RAGGED form (slots
k >= S masked, the last real sample in lane (S - 1) / SPL).  composite_sm_kernel walks one ray per lane over sample-major planes,
CSM_G = 4 passes at a time, depth variance from fp64 moments, pass moments as shifted sums around pass 0.  lap_depth_kernel forms
weights as differences of a running product.  moments_kernel unrolls its K sources by 8.  The cases take S from the dispatch
table, not from a workload: every SPL aligned and ragged, S = 1, S = 129 (lanes 9 .. 15 wholly masked), R = 37 (B R = 111 groups:
blocks straddle passes, the last block has 15 live groups and a clamped one), R = 300 for the planes (a full block, then 44
lanes), clip rows that change inside a block (chunk_rays = 10, ray_offset = 7, one row narrowed so that the clip is active).

Reference: `reference` takes the Euclidean edges, deltas and mid-points from the fp32 oracle (O.spacing_to_euclidean, e1 - e0,
(e0 + e1) / 2: the kernels' own fp32 operation sequence) and does everything after them in float64.  `chain32` is the same in
float32 with the oracle's operations (O.get_weights, O.render_*).

Bounds, per element, from the reference's own conditioning (nothing here comes from a GPU result); wb_k = pdf_cases.weight_bound:
  accumulation   sum wb_k + SUM_EPS sum w_k
  rgb            sum wb_k |c_k| + |bg| sum wb_k + SUM_EPS (sum w_k |c_k| + |bg|), before the clamp (clamping cannot increase a
                 difference)
  rgb_var        sum 2 w_k wb_k beta_k + SUM_EPS sum w_k^2 beta_k
  expected depth (sum wb_k t_k + ed sum wb_k) / (acc + 1e-10) + SUM_EPS ed, before the clip
  depth_var      sum wb_k (t_k - d)^2 + SUM_EPS sum w_k (t_k - d)^2 + 2^-24 1e-5, reference and bound evaluated with d = the
                 median mid-point the kernel returned, once that has passed the median check: tie rays are held too
  median depth   a ray is a TIE when min_k |cumsum(w)_k - 0.5| is at most the sum of its weight bounds up to the median index; a
                 non-tie ray must return the mid-point of the reference's index to DEPTH_RTOL, a tie ray that or a neighbour's.
                 With weights_alt the weights are inputs (wb = 0): only the fp32 cumsum rounds, SUM_EPS cumsum_k for k > 0.
  pass moments   E_b the per-pass channel bounds, Q = sum (x_b - m)^2 of the float64 per-pass reference:
                 |dmean| <= mean(E_b) + MOM_EPS max |x_b|
                 |dvar|  <= [2 sqrt(Q sum E_b^2) + sum E_b^2] / (B - 1) + MOM_EPS sum (x_b - x_0)^2 / (B - 1)
                 (the spread around pass 0 is what the planes kernel's shifted sums round; it is >= Q).  A ray with a tie in any
                 pass is held on channels 0 - 3, 5 and 6 only.
SUM_EPS / MOM_EPS / LAP_FACTOR = 4 x the worst error of fp32 CPU restatements against float64 (measure_*; the CPU test re-measures).
NaN rule: exactly one of kernel and reference NaN fails; a non-finite kernel value the reference does not have fails.

The exact family (one opaque sample, the all-zero ray) has outputs known in any summation order and is compared bit for bit."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

import pdf_cases as PC
from oracle import nerf_oracle as O

NEAR, FAR = PC.NEAR, PC.FAR
R_GROUP, R_PLANES = 37, 300
CHUNK, OFFSET = 10, 7
N_VIEWS = 3
U24 = 2.0 ** -24
DEPTH_RTOL, MAX_TIES = PC.DEPTH_RTOL, PC.MAX_TIES
EPS10, EPS5 = float(np.float32(1e-10)), float(np.float32(1e-5))     # the constants as the kernels hold them
SPLS = (1, 2, 3, 4, 6, 8, 16)
S_ALIGNED = (16, 32, 48, 64, 96, 128, 256)
S_RAGGED = (1, 2, 15, 17, 31, 33, 49, 65, 80, 97, 112, 127, 129, 255)
S_MOMENTS = (16, 17, 49, 96, 129, 256)
B_MOMENTS = (1, 2, 3, 15, 16)
S_PLANES = (1, 2, 17, 48, 129, 256)
B_PLANES = (2, 3, 4, 5, 8, 9)
S_ALT = (17, 48, 129)
S_EXACT = (16, 17, 48, 49, 129, 256)
BACKGROUNDS = ("last_sample", "white", "black", "random", (0.25, 0.5, 0.875))
ROW_KINDS = ("zero", "opaque_tail", "inf", "nan_density", "nan_colour", "clamp", "last_sample_only", "lane_first", "lane_last")
# worst summation error / sum |term| of the fp32 CPU chains (chain32's sums and the 16-lane tree order) on the chains' own fp32
# weights, over all toleranced cases; SUM_EPS = 4 x it, rounded up (the 4 x allows for another summation order)
SUM_WORST_MEASURED = 4.5e-7
SUM_EPS = 1.8e-6
# the same for the pass moments (two-pass tree form and shifted sums around pass 0, fp32 against float64)
MOM_WORST_MEASURED = 6.4e-7
MOM_EPS = 2.6e-6
# fp32 running-product restatement of the depth draws (correctly rounded exp2) against float64, in units of
# 2^-23 mean_d [P_i sum_{j<=i} (|x_j| + 2)]; LAP_FACTOR = 2 x (4 x it, rounded up): the 2 x is v_exp_f32's 1 ulp
LAP_WORST_MEASURED = 0.59
LAP_FACTOR = 4.8
# generator seeds per case name (default 0): a seed is changed when a case would hold more tie rays than MAX_TIES allows
SEEDS = {}


def spl_for(S):
    return next(s for s in SPLS if s >= (S + 15) // 16)


def is_ragged(S):
    return spl_for(S) * 16 != S


def background_colour(bg, rgb):
    """-> the colour blended behind the samples [R,3] (rgb already nan_to_num'ed), or None for "random" (no blend)"""
    if isinstance(bg, str) and bg == "random":
        return None
    if isinstance(bg, str) and bg == "last_sample":
        return rgb[:, -1, :]
    vals = O.BACKGROUND_COLORS[bg] if isinstance(bg, str) else bg
    return torch.tensor(vals, dtype=rgb.dtype).expand(rgb.shape[0], 3)


def geometry(sb, near, far, spacing):
    """the fp32 oracle's Euclidean edges -> (deltas, steps) in fp32, the kernels' own operation sequence"""
    eb = O.spacing_to_euclidean(torch.as_tensor(sb, dtype=torch.float32), near, far, uniform=bool(spacing))
    return eb[:, 1:] - eb[:, :-1], (eb[:, :-1] + eb[:, 1:]) / 2


def reference(dens, rgb, beta, sb, lo, hi, bg="last_sample", near=NEAR, far=FAR, spacing=0, weights_alt=None):
    """float64 on the fp32 oracle's deltas and mid-points.  dens [R,S], rgb [R,S,3], beta [R,S] | None, sb [R,S+1], lo / hi [R]
    (the ray's clip row), weights_alt [R,S] | None (the depth-side channels then use those weights as given)"""
    delta32, steps32 = geometry(sb, near, far, spacing)
    f = lambda a: torch.as_tensor(a, dtype=torch.float32).double()
    d, col, delta, t = f(dens), torch.nan_to_num(f(rgb)), delta32.double(), steps32.double()
    Rr, S = d.shape
    dd = delta * d
    c = torch.cat([torch.zeros(Rr, 1, dtype=torch.float64), torch.cumsum(dd[:, :-1], dim=-1)], dim=-1)
    w = torch.nan_to_num((1 - torch.exp(-dd)) * torch.exp(-c))
    ref = SimpleNamespace(weights=w, dd=dd, c=c, steps32=steps32, t=t, col=col, S=S, alt=weights_alt is not None)
    ref.wb = PC.weight_bound(ref)
    ref.bgc = background_colour(bg, col)
    ref.acc_rgb = w.sum(-1)
    comp = (w[..., None] * col).sum(-2)
    ref.rgb_pre = comp if ref.bgc is None else comp + ref.bgc * (1 - ref.acc_rgb)[:, None]
    ref.beta = None if beta is None else f(beta)
    ref.rgb_var = torch.zeros(Rr, dtype=torch.float64) if beta is None else (w * w * ref.beta).sum(-1)
    ref.wd = w if weights_alt is None else f(weights_alt)
    ref.wbd = ref.wb if weights_alt is None else torch.zeros_like(w)
    ref.acc = ref.wd.sum(-1)
    cw = torch.cumsum(ref.wd, dim=-1)
    ref.cw = cw
    ref.idx = torch.clamp(torch.searchsorted(cw, torch.full((Rr, 1), 0.5, dtype=torch.float64), side="left"), 0, S - 1)[:, 0]
    ref.margin = (cw - 0.5).abs().min(dim=-1).values
    ref.depth = torch.gather(t, -1, ref.idx[:, None])[:, 0]
    ref.wt = (ref.wd * t).sum(-1)
    ref.ed_pre = ref.wt / (ref.acc + EPS10)
    ref.lo, ref.hi = f(lo), f(hi)
    if weights_alt is None:
        ref.tie = PC.ties(ref, ref.wb)
    else:      # the weights are inputs: only the fp32 cumsum rounds, and a single term (index 0) does not
        at = torch.gather(cw, -1, ref.idx[:, None])[:, 0]
        ref.tie = (ref.idx > 0) & (ref.margin <= SUM_EPS * at)
    return ref


def ref8(ref, d=None):
    """the eight channels [R,8] in float64 (rgb clamped, expected depth clipped); d: the median mid-point depth_var is taken
    around (default the reference's own)"""
    d = ref.depth if d is None else d
    dv = (ref.wd * (ref.t - d[:, None]) ** 2).sum(-1) + EPS5
    ed = torch.minimum(torch.maximum(ref.ed_pre, ref.lo), ref.hi)
    return torch.cat([torch.clamp(ref.rgb_pre, 0.0, 1.0), torch.stack([ref.acc, d, ed, ref.rgb_var, dv], dim=-1)], dim=-1)


def bounds8(ref, d=None, sum_eps=None):
    """per-element bounds [R,8] (the median channel: DEPTH_RTOL |d|, what a non-tie ray is held to)"""
    e = SUM_EPS if sum_eps is None else sum_eps
    d = ref.depth if d is None else d
    w, wb, wd, wbd, t = ref.weights, ref.wb, ref.wd, ref.wbd, ref.t
    bg = torch.zeros_like(ref.rgb_pre) if ref.bgc is None else ref.bgc.abs()
    ca = ref.col.abs()
    rgb = (wb[..., None] * ca).sum(-2) + bg * wb.sum(-1)[:, None] + e * ((w[..., None] * ca).sum(-2) + bg)
    acc = wbd.sum(-1) + e * wd.sum(-1)
    ed = ((wbd * t).sum(-1) + ref.ed_pre * wbd.sum(-1)) / (ref.acc + EPS10) + e * ref.ed_pre
    uv = torch.zeros_like(acc) if ref.beta is None else (2 * w * wb * ref.beta).sum(-1) + e * (w * w * ref.beta).sum(-1)
    q = (t - d[:, None]) ** 2
    dv = (wbd * q).sum(-1) + e * (wd * q).sum(-1) + U24 * EPS5
    return torch.cat([rgb, torch.stack([acc, DEPTH_RTOL * d.abs(), ed, uv, dv], dim=-1)], dim=-1)


def chain32(dens, rgb, beta, sb, lo, hi, bg="last_sample", near=NEAR, far=FAR, spacing=0, weights_alt=None):
    """the oracle's operations in float32 -> [R,8].  (O.render_depth_expected clips to the min / max of the chunk it is passed;
    here the clip rows are the case's own, so its quotient is restated and clipped with them.)"""
    f = lambda a: torch.as_tensor(a, dtype=torch.float32)
    delta, steps = geometry(sb, near, far, spacing)
    w = O.get_weights(f(dens), delta)
    background = bg if isinstance(bg, (str, tuple)) else tuple(bg)
    col = O.render_rgb(f(rgb), w, background if background != "random" else "random")
    uv = torch.zeros(w.shape[0], 1) if beta is None else O.render_uncertainty(f(beta), w ** 2)
    wd = w if weights_alt is None else f(weights_alt)
    acc = O.render_accumulation(wd)
    depth = O.render_depth_median(wd, steps)
    ed = torch.sum(wd * steps, dim=-1, keepdim=True) / (acc + 1e-10)
    ed = torch.minimum(torch.maximum(ed, f(lo)[:, None]), f(hi)[:, None])
    dv = torch.sum(wd * (steps - depth) ** 2, dim=-1, keepdim=True) + 1e-5
    return torch.cat([col, acc, depth, ed, uv, dv], dim=-1)


CHANNELS = ("rgb", "acc", "depth", "ed", "rgb_var", "depth_var")
_GROUP = (slice(0, 3), slice(3, 4), slice(4, 5), slice(5, 6), slice(6, 7), slice(7, 8))


def _nan_rule(name, got, ref):
    bad = torch.isnan(got) != torch.isnan(ref)
    assert not bad.any(), f"{name}: NaN on one side only at {torch.nonzero(bad)[:8].tolist()}"
    bad = ~torch.isfinite(got) & torch.isfinite(ref)
    assert not bad.any(), f"{name}: non-finite values the reference does not have at {torch.nonzero(bad)[:8].tolist()}"


def hold(name, ref, out, expect=None, rows=None, sum_eps=None):
    """One pass's eight channels (float32 [R,8], on the CPU) against the reference `ref` of the same rays (rows: the rays of
    `ref` the result holds).  Asserts; -> {channel: worst error / bound}.  expect: the exact family's bits."""
    out = out.detach().cpu()
    assert out.dtype == torch.float32 and out.dim() == 2 and out.shape[1] == 8
    rows = slice(None) if rows is None else rows
    if expect is not None:
        bad = torch.nonzero(out.view(torch.int32) != expect[rows].view(torch.int32))
        assert len(bad) == 0, (f"{name}: differs from the exact values at (ray, channel) {bad[:8].tolist()}: "
                               f"{[out[i, j].item() for i, j in bad[:8].tolist()]} for "
                               f"{[expect[rows][i, j].item() for i, j in bad[:8].tolist()]}")
        return {k: 0.0 for k in CHANNELS}
    got = out.double()
    _nan_rule(name, got, ref8(ref)[rows])
    # the median first: depth_var is then taken around the mid-point the kernel returned
    t, S = ref.t[rows], ref.S
    pick = lambda k: torch.gather(t, -1, torch.clamp(k, 0, S - 1)[:, None])[:, 0]
    near = lambda k: (got[:, 4] - pick(k)).abs() <= DEPTH_RTOL * pick(k).abs()
    idx, tie = ref.idx[rows], ref.tie[rows]
    ok = torch.where(tie, near(idx) | near(idx - 1) | near(idx + 1), near(idx))
    assert ok.all(), f"{name}: median depth off on rays {torch.nonzero(~ok)[:, 0].tolist()} (of the rows passed)"
    d = torch.zeros_like(ref.depth)
    d[rows] = got[:, 4]
    want, bnd = ref8(ref, d)[rows], bounds8(ref, d, sum_eps)[rows]
    err = (got - want).abs()
    ratios = {}
    for ch, sl in zip(CHANNELS, _GROUP):
        if ch == "depth":
            ratios[ch] = 0.0
            continue
        e, b = err[:, sl], bnd[:, sl]
        bad = torch.nonzero(e > b)
        assert len(bad) == 0, (f"{name}: {ch} beyond its bound on rays {bad[:8, 0].tolist()}, worst error / bound "
                               f"{(e / b).max().item():.3g} (error {e[bad[0, 0], bad[0, 1]].item():.3e}, bound "
                               f"{b[bad[0, 0], bad[0, 1]].item():.3e})")
        live = b > 0
        ratios[ch] = (e[live] / b[live]).max().item() if live.any() else 0.0
    return ratios


def moments_reference(refs, mom_eps=None):
    """float64 mean / unbiased variance over the per-pass references, their bounds [R,8] and the channels held per ray"""
    m_eps = MOM_EPS if mom_eps is None else mom_eps
    x = torch.stack([ref8(r) for r in refs])                     # [B,R,8]
    E = torch.stack([bounds8(r) for r in refs])
    B = x.shape[0]
    tie = torch.stack([r.tie for r in refs]).any(0)
    mean = x.mean(0)
    Q = ((x - mean) ** 2).sum(0)
    mb = E.mean(0) + m_eps * x.abs().max(0).values
    if B == 1:
        var, vb = torch.full_like(mean, float("nan")), torch.zeros_like(mean)
    else:
        var = Q / (B - 1)
        E2 = (E ** 2).sum(0)
        vb = (2 * torch.sqrt(Q * E2) + E2) / (B - 1) + m_eps * ((x - x[0]) ** 2).sum(0) / (B - 1)
    held = torch.ones_like(mean, dtype=torch.bool)
    held[tie, 4], held[tie, 7] = False, False
    return SimpleNamespace(mean=mean, var=var, mean_bound=mb, var_bound=vb, held=held, tie=tie, B=B)


def hold_moments(name, mr, mean, var, rows=None):
    """mean / var [R,8] of a K-pass kernel against moments_reference.  -> (worst mean ratio, worst var ratio)"""
    rows = slice(None) if rows is None else rows
    mean, var = mean.detach().cpu(), var.detach().cpu()
    assert mean.dtype == var.dtype == torch.float32 and mean.shape == var.shape == mr.mean[rows].shape
    out = []
    for what, got, want, bnd in (("mean", mean.double(), mr.mean[rows], mr.mean_bound[rows]),
                                 ("variance", var.double(), mr.var[rows], mr.var_bound[rows])):
        _nan_rule(f"{name} {what}", got, want)
        if what == "variance" and mr.B == 1:
            assert torch.isnan(got).all(), f"{name}: the variance of one pass is NaN in every channel"
            out.append(0.0)
            continue
        err = torch.where(mr.held[rows], (got - want).abs(), torch.zeros_like(want))
        bad = torch.nonzero(err > bnd)
        assert len(bad) == 0, (f"{name}: {what} beyond its bound at (ray, channel) {bad[:8].tolist()}, worst error / bound "
                               f"{(err / bnd)[bnd > 0].max().item():.3g}")
        live = (bnd > 0) & mr.held[rows]
        out.append((err[live] / bnd[live]).max().item())
    return tuple(out)


# ---- cases -----------------------------------------------------------------------------------------------------------
def clip_row_of(r, offset=OFFSET, chunk=CHUNK):
    return (offset + r) // chunk


def view_clip_row_of(r, rays_per_view, chunk=CHUNK):
    cpv = (rays_per_view + chunk - 1) // chunk
    return (r // rays_per_view) * cpv + (r % rays_per_view) // chunk


def _finish(c):
    """clip rows from the mid-points and pass 0's unclipped expected depth, the cached float64 references, the tie cap"""
    Rr = c.R
    rows = torch.tensor([c.row_of(r) for r in range(Rr)])
    _, steps = geometry(c.sb, c.near, c.far, c.spacing)
    n_rows = int(rows.max()) + 1
    clip = torch.empty(n_rows, 2)
    for j in range(n_rows):
        clip[j, 0], clip[j, 1] = steps[rows == j].min(), steps[rows == j].max()
    inf = torch.full((Rr,), float("inf"))
    free = reference(c.dens[0], c.rgb[0], c.beta, c.sb, -inf, inf, c.bg, c.near, c.far, c.spacing, c.walt)
    for j in (range(n_rows) if c.views else [2] if n_rows > 2 else []):      # narrowed rows: the clip is active there
        ed = torch.sort(free.ed_pre[rows == j]).values.float()
        clip[j, 0], clip[j, 1] = ed[int(0.3 * (len(ed) - 1))], ed[int(0.7 * (len(ed) - 1))]
    c.clip, c.rows = clip, rows
    c.lo, c.hi = clip[rows, 0], clip[rows, 1]
    c.refs = [reference(c.dens[b], c.rgb[b], c.beta, c.sb, c.lo, c.hi, c.bg, c.near, c.far, c.spacing, c.walt) for b in range(c.B)]
    c.n_ties = int(torch.stack([r.tie for r in c.refs]).any(0).sum())
    assert c.n_ties <= MAX_TIES * Rr, f"{c.name}: {c.n_ties} tie rays"
    return c


def refs_without_beta(c):
    """the per-pass references of the K-pass kernels, which take no beta (rgb_var = 0)"""
    if not hasattr(c, "_refs_nobeta"):
        c._refs_nobeta = [reference(c.dens[b], c.rgb[b], None, c.sb, c.lo, c.hi, c.bg, c.near, c.far, c.spacing, c.walt)
                          for b in range(c.B)]
    return c._refs_nobeta


def lane_border(S):
    """-> (first slot of a lane, last slot of the lane before it) for the S's own SPL, inside the ray"""
    spl = spl_for(S)
    j = max(1, ((S - 1) // spl + 1) // 2)
    return min(spl * j, S - 1), min(spl * j - 1, S - 1)


@functools.lru_cache(maxsize=None)
def toleranced(S, B=3, bg="last_sample", variant=None, R=R_GROUP):
    """seeded densities exp(2 randn) on sorted uniform bins, B passes, planted rays 0 - 8 (ROW_KINDS, in every pass), ray 9 (B >= 2)
    all zero in pass 0 and opaque in the others (the largest spread around pass 0), rays >= 20 nearly the same in every pass (a
    small spread on a large value).  variant: "uniform" SPACING_UNIFORM near 1 / far 100, "nobeta", "views" 3 views of R rays
    (clip rows numbered per view, every row narrowed), "alt" weights_alt with an alt row summing below 0.5 (ray 10) and one
    reaching 0.5 at slot 0 (ray 11)"""
    name = f"{variant or 'plain'}-S{S}-B{B}-R{R}-{bg if isinstance(bg, str) else 'colour'}"
    g = torch.Generator().manual_seed(100003 * SEEDS.get(name, 0) + 1000 * S + 10 * B + R)
    views = variant == "views"
    Rr = R * N_VIEWS if views else R
    near, far, spacing = (1.0, 100.0, 1) if variant == "uniform" else (NEAR, FAR, 0)
    dens = torch.exp(torch.randn(B, Rr, S, generator=g) * 2.0)
    rgb = torch.rand(B, Rr, S, 3, generator=g)
    beta = None if variant == "nobeta" else torch.rand(Rr, S, generator=g) + 0.01
    sb = torch.sort(torch.rand(Rr, S + 1, generator=g), dim=-1).values
    delta, _ = geometry(sb, near, far, spacing)
    delta = delta.double()
    if B > 1:
        dens[1:, 20:] = dens[0:1, 20:] * torch.exp(0.01 * torch.randn(B - 1, Rr - 20, S, generator=g))
    kf, kl = lane_border(S)
    planted = {"inf": min(5, S - 1), "nan_density": S // 2, "nan_colour": min(2, S - 1), "lane_first": kf, "lane_last": kl}
    dens[:, 0] = 0.0
    dens[:, 1, S // 3:] = 1e5
    dens[:, 2, planted["inf"]] = float("inf")
    dens[:, 3, planted["nan_density"]] = float("nan")
    rgb[:, 4, planted["nan_colour"], 1] = float("nan")
    for r, tail in ((4, 2.0), (5, 20.0)):      # optical depth 0.2 spread over the ray (every sample has weight), dd = 2 at S // 4 (the
        dens[:, r] = dens[:, r] * (0.2 / (delta[r] * dens[:, r].double()).sum(-1, keepdim=True)).float()      # median, clear of a
        dens[:, r, S // 4] = (2.0 / delta[r, S // 4]).float()                                                  # tie), dd = 20 at the
        dens[:, r, -1] = (tail / delta[r, -1]).float()                                                         # end of the clamp row
    rgb[:, 5, :, 0], rgb[:, 5, :, 1] = 1.7, -0.6
    dens[:, 6, :-1], dens[:, 6, -1] = 0.0, 1e5
    for r, k in ((7, kf), (8, kl)):
        assert delta[r, k] > 0
        dens[:, r, :k] = 0.0
        dens[:, r, k] = (2.0 / delta[r, k]).float()              # dd = 2: w_k = 0.86
    if B > 1:
        dens[0, 9], dens[1:, 9] = 0.0, 1e5
    walt = None
    if variant == "alt":
        walt = torch.rand(Rr, S, generator=g) / S * 1.6
        walt[10] = walt[10] * (0.3 / walt[10].double().sum()).float()
        walt[11, 0] = 0.5
    row_of = (lambda r: view_clip_row_of(r, R)) if views else clip_row_of
    c = SimpleNamespace(name=name, family="toleranced", variant=variant, S=S, B=B, R=Rr, rays_per_view=R, views=views, bg=bg,
                        spl=spl_for(S), ragged=is_ragged(S), dens=dens, rgb=rgb, beta=beta, sb=sb, walt=walt, near=near, far=far,
                        spacing=spacing, row_of=row_of, planted=planted)
    _finish(c)
    ref = c.refs[0]
    if variant != "alt":
        assert ref.idx[7].item() == kf and ref.idx[8].item() == kl and ref.idx[6].item() == S - 1 and ref.idx[0].item() == S - 1
        assert ref.acc[0].item() == 0.0 and ref.weights[6, -1].item() == 1.0 and not ref.tie[:9].any()
        assert (ref.weights[3, planted["nan_density"]:] == 0).all() and ref.weights[4, planted["nan_colour"]] > 0
        assert (ref.rgb_pre[5, 0] > 1) and (ref.rgb_pre[5, 1] < 0), f"{name}: the clamp row does not reach the clamp"
    else:
        assert ref.acc[10] < 0.5 and ref.idx[10].item() == S - 1 and ref.idx[11].item() == 0 and not ref.tie[10:12].any()
    if c.clip.shape[0] > 2:
        live = (ref.ed_pre < ref.lo) | (ref.ed_pre > ref.hi)
        assert live[c.rows == 2].any(), f"{name}: the narrowed clip row is not active"
    return c


@functools.lru_cache(maxsize=None)
def exact(S, bg="last_sample"):
    """evenly spaced bins, every density 0 but one opaque sample k (exp(-delta sigma) = 0 in fp32 and in float64: +inf and
    1e30), k over {0, SPL - 1, SPL, S - 1}; the last ray is all zero.  -> rgb = clamp(colour_k), acc = 1, depth = expected depth
    = steps[k], rgb_var = beta_k, depth_var = float32(1e-5); the all-zero ray: acc = 0, rgb = the background, depth =
    steps[S - 1], expected depth = the clip row's low, rgb_var = 0, depth_var = float32(1e-5)"""
    spl = spl_for(S)
    ks = sorted({k for k in (0, spl - 1, spl, S - 1) if k < S})
    Rr = 2 * len(ks) + 1
    g = torch.Generator().manual_seed(7 * S)
    sb = O.initial_spacing_bins(S)[None].expand(Rr, -1).contiguous()
    rgb = torch.rand(1, Rr, S, 3, generator=g) * 1.5 - 0.25          # some channels beyond the clamp on either side
    beta = torch.rand(Rr, S, generator=g) + 0.01
    dens = torch.zeros(1, Rr, S)
    _, steps = geometry(sb, NEAR, FAR, 0)
    expect = torch.empty(Rr, 8)
    c = SimpleNamespace(name=f"exact-S{S}-{bg if isinstance(bg, str) else 'colour'}", family="exact", variant=None, S=S, B=1, R=Rr,
                        rays_per_view=Rr, views=False, bg=bg, spl=spl, ragged=is_ragged(S), dens=dens, rgb=rgb, beta=beta, sb=sb,
                        walt=None, near=NEAR, far=FAR, spacing=0, row_of=clip_row_of, ks=ks)
    for i, k in enumerate(ks):
        for r, sigma in ((2 * i, float("inf")), (2 * i + 1, 1e30)):
            dens[0, r, k] = sigma
            expect[r, :3] = torch.clamp(rgb[0, r, k], 0.0, 1.0)
            expect[r, 3], expect[r, 4], expect[r, 5], expect[r, 6] = 1.0, steps[r, k], steps[r, k], beta[r, k]
    _finish(c)
    z = Rr - 1
    bgc = background_colour(bg, rgb[0])
    expect[z, :3] = 0.0 if bgc is None else torch.clamp(bgc[z], 0.0, 1.0)
    expect[z, 3], expect[z, 4], expect[z, 5], expect[z, 6] = 0.0, steps[z, S - 1], c.lo[z], 0.0
    expect[:, 7] = torch.tensor(np.float32(1e-5))
    c.expect = expect
    assert torch.equal(ref8(c.refs[0]).float(), expect), f"{c.name}: the float64 reference, rounded, is not the exact value"
    return c


def _bg_cycle(seq, shift=0):
    return {S: BACKGROUNDS[(i + shift) % len(BACKGROUNDS)] for i, S in enumerate(seq)}


# composite_var: every S at B = 3 and B = 1 (another background), the uniform spacing and beta = None at a ragged and an aligned S
COMPOSITE = {}
for _seq in (S_ALIGNED, S_RAGGED):
    for _S, _bg in _bg_cycle(_seq).items():
        COMPOSITE[f"S{_S}-B3"] = functools.partial(toleranced, _S, 3, _bg)
    for _S, _bg in _bg_cycle(_seq, 2).items():
        COMPOSITE[f"S{_S}-B1"] = functools.partial(toleranced, _S, 1, _bg)
for _S in (33, 64):
    COMPOSITE[f"uniform-S{_S}"] = functools.partial(toleranced, _S, 3, "last_sample", "uniform")
    COMPOSITE[f"nobeta-S{_S}"] = functools.partial(toleranced, _S, 1, "white", "nobeta")
ALT = {f"alt-S{S}": functools.partial(toleranced, S, 1, "last_sample", "alt") for S in S_ALT}
# several views: the first and last rows of the samples-per-lane table (SPL 1 ragged, SPL 16 aligned) and two between them
VIEWS = {f"views-S{S}": functools.partial(toleranced, S, 3, "last_sample", "views") for S in (1, 17, 48, 256)}
EXACT = {f"exact-S{S}-{bg if isinstance(bg, str) else 'colour'}": functools.partial(exact, S, bg) for S in S_EXACT for bg in BACKGROUNDS}
MOMENTS = {f"mom-S{S}-B{B}": functools.partial(toleranced, S, B, BACKGROUNDS[(i + j) % 5])
           for i, S in enumerate(S_MOMENTS) for j, B in enumerate(B_MOMENTS)}
PLANES = {f"planes-S{S}-B{B}": functools.partial(toleranced, S, B, BACKGROUNDS[(i + j) % 5], None, R_PLANES)
          for i, S in enumerate(S_PLANES) for j, B in enumerate(B_PLANES)}
TOLERANCED = {**COMPOSITE, **ALT, **VIEWS, **MOMENTS, **PLANES}


def packed_pair(S):
    """one aligned and one ragged S per SPL, for the packed rows"""
    return S in (16, 32, 48, 64, 96, 128, 256, 15, 31, 33, 49, 80, 127, 129)


def check_coverage():
    """every SPL aligned and ragged; every planted row kind and background on a ragged and on an aligned S; the pass counts"""
    for ragged in (False, True):
        cs = [f() for k, f in COMPOSITE.items() if f().ragged == ragged and f().variant is None]
        assert {c.spl for c in cs} == set(SPLS), f"ragged={ragged}: SPL {sorted({c.spl for c in cs})}"
        assert {c.bg for c in cs} == set(BACKGROUNDS)
        assert all(set(c.planted) <= set(ROW_KINDS) and c.family == "toleranced" for c in cs) and len(ROW_KINDS) == 9
        assert {spl_for(S) for S in (S_ALIGNED if not ragged else S_RAGGED) if packed_pair(S)} == set(SPLS)
    assert {spl_for(S) for S in S_RAGGED} == set(SPLS) and all(is_ragged(S) for S in S_RAGGED)
    assert not any(is_ragged(S) for S in S_ALIGNED) and 1 in S_RAGGED and 129 in S_RAGGED and (129 - 1) // 16 == 8
    assert {f().B for f in MOMENTS.values()} == {1, 2, 3, 15, 16} and {f().S for f in MOMENTS.values()} == set(S_MOMENTS)
    assert {f().B for f in PLANES.values()} == {2, 3, 4, 5, 8, 9} and {f().S for f in PLANES.values()} == set(S_PLANES)
    assert all(f().R == R_PLANES for f in PLANES.values()) and all(f().R == R_GROUP for f in MOMENTS.values())
    assert {f().S for f in EXACT.values()} == set(S_EXACT) and {f().bg for f in EXACT.values()} == set(BACKGROUNDS)
    assert any(f().spacing == 1 and f().ragged for f in COMPOSITE.values()) and any(f().spacing == 1 and not f().ragged for f in COMPOSITE.values())
    assert any(f().beta is None for f in COMPOSITE.values())


# ---- fp32 restatements of the summation orders (CPU; they measure SUM_EPS and MOM_EPS, and show that the cases bite) ---------
_PERMS = [np.arange(16) ^ 1, np.arange(16) ^ 2, np.array([7, 6, 5, 4, 3, 2, 1, 0, 15, 14, 13, 12, 11, 10, 9, 8]), np.arange(15, -1, -1)]


def tree_sum(terms, S):
    """[R,S] fp32 terms summed as a 16-lane group does: each lane its SPL slots in order, then group_sum's four exchanges
    (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror); lane 0's value"""
    terms = np.asarray(terms, np.float32)
    spl = spl_for(S)
    pad = np.zeros((terms.shape[0], 16 * spl), np.float32)
    pad[:, :terms.shape[1]] = terms
    lanes = pad.reshape(-1, 16, spl)
    v = np.zeros(lanes.shape[:2], np.float32)
    for e in range(spl):
        v = v + lanes[:, :, e]
    for p in _PERMS:
        v = v + v[:, p]
    return v[:, 0]


def _sum_terms(c, b):
    """the five sums of a pass as fp32 term arrays on the fp32 chain's own weights: (name, terms [R,S])"""
    delta, steps = geometry(c.sb, c.near, c.far, c.spacing)
    w = O.get_weights(c.dens[b], delta)
    wd = w if c.walt is None else c.walt
    col = torch.nan_to_num(c.rgb[b])
    depth = O.render_depth_median(wd, steps)
    out = [("acc", wd), ("wt", wd * steps), ("dv", wd * (steps - depth) ** 2)] + [(f"rgb{i}", w * col[..., i]) for i in range(3)]
    if c.beta is not None:
        out.append(("uvar", w * w * c.beta))
    return out


@functools.lru_cache(maxsize=None)
def measure_sums():
    """-> worst |fp32 sum - float64 sum| / sum |term| of torch.sum (chain32's order) and of tree_sum, over the toleranced cases"""
    worst = 0.0
    for f in TOLERANCED.values():
        c = f()
        for b in range(c.B):
            for _, terms in _sum_terms(c, b):
                exact_sum, scale = terms.double().sum(-1), terms.double().abs().sum(-1)
                for got in (terms.sum(-1).double(), torch.from_numpy(tree_sum(terms.numpy(), c.S)).double()):
                    live = scale > 0
                    if live.any():
                        worst = max(worst, ((got - exact_sum).abs()[live] / scale[live]).max().item())
    return worst


def moments_two_pass32(x):
    """x [B,...] fp32 -> (mean, var) as composite_moments_body: lane b holds pass b's value less pass 0's, two group reductions"""
    x = np.asarray(x, np.float32)
    B = x.shape[0]
    flat = x.reshape(B, -1).T
    d = flat - flat[:, :1]
    inv_b = np.float32(1.0) / np.float32(B)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv_b1 = np.float32(1.0) / np.float32(B - 1)
        dm = tree_sum(d, 16) * inv_b
        dev = d - dm[:, None]
        v = tree_sum(dev * dev, 16) * inv_b1
    return (flat[:, 0] + dm).reshape(x.shape[1:]), v.reshape(x.shape[1:])


def moments_shifted32(x, shift=True, clamp=True):
    """x [B,...] fp32 -> (mean, var) as composite_sm_kernel: sums of (x - x_0) and (x - x_0)^2 in pass order.  shift=False,
    clamp=False: the plain sum-of-squares form, a mutation"""
    x = np.asarray(x, np.float32)
    B = x.shape[0]
    x0 = x[0] if shift else np.zeros_like(x[0])
    sd, sd2 = np.zeros_like(x0), np.zeros_like(x0)
    for b in range(1 if shift else 0, B):
        d = x[b] - x0
        sd = sd + d
        sd2 = sd2 + d * d
    inv_b, inv_b1 = np.float32(1.0) / np.float32(B), np.float32(1.0) / np.float32(B - 1)
    v = sd2 - sd * sd * inv_b
    return x0 + sd * inv_b, (np.maximum(v, np.float32(0)) if clamp else v) * inv_b1


@functools.lru_cache(maxsize=None)
def measure_moments():
    """-> worst fp32 rounding of the two moment forms on the per-pass references rounded to fp32, in the bounds' own units:
    |dmean| / max |x_b| and (B - 1) |dvar| / sum (x_b - x_0)^2 (elements with a spread; where every pass gives the same value the
    variance bound is the E_b terms alone)"""
    worst = 0.0
    for f in {**MOMENTS, **PLANES}.values():
        c = f()
        if c.B < 2:
            continue
        x32 = torch.stack([ref8(r) for r in c.refs]).float()
        x = x32.double()
        mean, var = x.mean(0), x.var(0)
        spread = ((x - x[0]) ** 2).sum(0)
        scale = x.abs().max(0).values
        for form in (moments_two_pass32, moments_shifted32):
            if form is moments_two_pass32 and c.B > 16:
                continue
            m, v = (torch.from_numpy(a).double() for a in form(x32.numpy()))
            live = scale > 0
            worst = max(worst, ((m - mean).abs()[live] / scale[live]).max().item())
            dv = (c.B - 1) * (v - var).abs()
            live = spread > 0
            if live.any():
                worst = max(worst, (dv[live] / spread[live]).max().item())
    return worst


# ---- Laplace depth draws ---------------------------------------------------------------------------------------------
LOG2E32 = float(np.float32(1.4426950408889634))
D_LAPLACE = (1, 2, 5)
S_LAPLACE = (1, 16, 17, 49, 129)


@functools.lru_cache(maxsize=None)
def laplace(S, D):
    """mu = exp(randn), var = rand mu^2, explicit noise [D,R,S]; planted: (0, 0) var < 0, (0, 1 | 0) var = 0, (1, S // 2) NaN var,
    (2, S // 2) NaN mu (that sample and the later ones of the ray weigh 0), (3, *) mu = 0.  Reference: float64 relu(mu + sd z)
    into the float64 weights on the fp32 deltas, mean over the draws.  Bound per element:
    LAP_FACTOR 2^-23 mean_d [P_i sum_{j<=i} (|x_j| + 2)] + 2^-125 (the fp32 underflow threshold), x_j = delta_j log2(e) relu(...), P_i the reference transmittance (the
    kernel forms w_i = P_i - P_{i+1}: its error scales with P_i, not with w_i)"""
    g = torch.Generator().manual_seed(1000 * S + D)
    Rr = R_GROUP
    mu = torch.exp(torch.randn(Rr, S, generator=g))
    var = torch.rand(Rr, S, generator=g) * mu ** 2
    sb = torch.sort(torch.rand(Rr, S + 1, generator=g), dim=-1).values
    noise = torch.randn(D, Rr, S, generator=g)
    var[0, 0] = -1e-3
    var[0, min(1, S - 1)] = 0.0 if S > 1 else -1e-3
    var[1, S // 2] = float("nan")
    mu[2, S // 2] = float("nan")
    mu[3] = 0.0
    c = SimpleNamespace(name=f"laplace-S{S}-D{D}", S=S, D=D, R=Rr, mu=mu, var=var, sb=sb, noise=noise, near=NEAR, far=FAR, spacing=0)
    delta32, _ = geometry(sb, NEAR, FAR, 0)
    c.delta32 = delta32
    delta = delta32.double()
    sd = torch.sqrt(var.double())
    sd = torch.where(torch.isnan(sd), torch.tensor(1e-10, dtype=torch.float64), torch.clamp_min(sd, 1e-10))
    samp = torch.relu(mu.double()[None] + sd[None] * noise.double())            # [D,R,S]
    dd = delta[None] * samp
    cum = torch.cat([torch.zeros(D, Rr, 1, dtype=torch.float64), torch.cumsum(dd[..., :-1], dim=-1)], dim=-1)
    P = torch.exp(-cum)
    c.ref = torch.nan_to_num((1 - torch.exp(-dd)) * P).mean(0)
    x = dd * math.log2(math.e)
    unit = (P * torch.cumsum(x.abs() + 2, dim=-1)).mean(0) * PC.U23
    c.unit = torch.where(torch.isnan(unit), torch.zeros_like(unit), unit)       # behind a NaN the weight is 0 in any arithmetic
    assert (c.ref[2, S // 2:] == 0).all() and (c.unit[2, S // 2:] == 0).all() and torch.isfinite(c.ref).all()
    return c


LAPLACE = {f"laplace-S{S}-D{D}": functools.partial(laplace, S, D) for S in S_LAPLACE for D in D_LAPLACE}


def laplace32(c):
    """lap_depth_kernel's running-product form in fp32 with a correctly rounded exp2 (CPU): per lane the product of its slots'
    factors, the lanes' products scanned, w = carry (lp - lp e), summed over the draws with an fma, / D"""
    f32 = np.float32
    S, D, spl = c.S, c.D, spl_for(c.S)
    nd2 = (-(c.delta32.numpy()) * f32(LOG2E32)).astype(f32)
    with np.errstate(invalid="ignore"):
        s = np.sqrt(c.var.numpy())
    sd = np.where(np.isnan(s), f32(1e-10), np.maximum(s, f32(1e-10))).astype(f32)
    ca, cb = nd2 * sd, nd2 * c.mu.numpy()
    wsum = np.zeros((c.R, S), np.float64)
    for d in range(D):
        arg = (ca.astype(np.float64) * c.noise[d].numpy().astype(np.float64) + cb.astype(np.float64)).astype(f32)      # one fma
        em = np.exp2(np.minimum(arg, f32(0)).astype(np.float64)).astype(f32)       # NaN stays NaN here: the poisoned form
        em = np.where(np.isnan(arg), f32(np.nan), em)
        carry = np.ones(c.R, f32)
        for l in range(16):
            lp = np.ones(c.R, f32)
            for e in range(spl):
                k = l * spl + e
                if k >= S:
                    break
                nx = lp * em[:, k]
                wsum[:, k] = (carry.astype(np.float64) * (lp - nx).astype(np.float64) + wsum[:, k]).astype(f32)
                lp = nx
            carry = carry * lp
    w = (wsum.astype(f32) / f32(D)).astype(f32)
    return torch.from_numpy(np.where(np.isnan(w), f32(0), w))


@functools.lru_cache(maxsize=None)
def measure_laplace():
    worst = 0.0
    for f in LAPLACE.values():
        c = f()
        err = (laplace32(c).double() - c.ref).abs()
        assert (err[c.unit == 0] == 0).all(), c.name
        err = torch.clamp(err - PC.FLT_UNDERFLOW, min=0)
        worst = max(worst, (err[c.unit > 0] / c.unit[c.unit > 0]).max().item())
    return worst


def hold_laplace(c, got, rows=None):
    rows = slice(None) if rows is None else rows
    got = got.detach().cpu().double()
    _nan_rule(c.name, got, c.ref[rows])
    err, bnd = (got - c.ref[rows]).abs(), LAP_FACTOR * c.unit[rows] + PC.FLT_UNDERFLOW
    bad = torch.nonzero(err > bnd)
    assert len(bad) == 0, (f"{c.name}: {len(bad)} mean sampled weights beyond their bound, first (ray, k) {bad[:8].tolist()}, "
                           f"error {err[bad[0, 0], bad[0, 1]].item():.3e} bound {bnd[bad[0, 0], bad[0, 1]].item():.3e}")
    return (err / bnd).max().item()


# ---- moments over the leading dimension --------------------------------------------------------------------------------
K_MOMENTS = (1, 2, 7, 8, 9, 16, 17, 64)
NC_MOMENTS = (257, 6)


@functools.lru_cache(maxsize=None)
def stack_moments(K):
    """x [K,257,6]: 900 + 1e-3 randn in the first three channels (a small spread on a large value), randn in the others.  Bounds:
    mean (K + 2) 2^-24 mean |x|; variance: the kernel is two-pass, every deviation x_k - m carries the computed mean's error
    e_m <= the mean's bound, so the pass-moment bound with E_k = e_m and the spread around the mean:
    [2 sqrt(Q K e_m^2) + K e_m^2] / (K - 1) + MOM_EPS Q / (K - 1)"""
    g = torch.Generator().manual_seed(K)
    x = torch.randn(K, *NC_MOMENTS, generator=g)
    x[..., :3] = 900.0 + 1e-3 * x[..., :3]
    xd = x.double()
    mean = xd.mean(0)
    mb = (K + 2) * U24 * xd.abs().mean(0)
    if K == 1:
        var, vb = torch.full_like(mean, float("nan")), torch.zeros_like(mean)
    else:
        Q = ((xd - mean) ** 2).sum(0)
        var = Q / (K - 1)
        vb = (2 * torch.sqrt(Q * K * mb ** 2) + K * mb ** 2) / (K - 1) + MOM_EPS * Q / (K - 1)
    return SimpleNamespace(name=f"stack-K{K}", K=K, x=x, mean=mean, var=var, mean_bound=mb, var_bound=vb)


def hold_stack(c, mean, var):
    out = []
    for what, got, want, bnd in (("mean", mean, c.mean, c.mean_bound), ("variance", var, c.var, c.var_bound)):
        if got is None:
            continue
        got = got.detach().cpu().double()
        _nan_rule(f"{c.name} {what}", got, want)
        if what == "variance" and c.K == 1:
            assert torch.isnan(got).all()
            continue
        err = (got - want).abs()
        assert (err <= bnd).all(), f"{c.name}: {what} beyond its bound, worst error / bound {(err / bnd).max().item():.3g}"
        out.append((err / bnd).max().item())
    return out
