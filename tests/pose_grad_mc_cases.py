"""Cases and references for the pose gradient of an MC-dropout frame under a named mask draw (plain module: tests import
it; nothing here needs a GPU).  Built on tests/pose_grad_cases.py: the same coarse scenes, rays, pinned grid cells, margins
and error measure.

unerf_pose_grad_mc differentiates s = mean over channels of rgb = (1/K) sum_k clamp(pred_k), pass k evaluated under the
keep masks of that pass.  The masks here are the counter generator's, from its oracle twin:
O.mc_keep_mask(seed, k, r * S + s + first, stream, 64, p) with streams TRUNK 0, HEAD1 1, HEAD0 2.

`reference64`: float64 autograd of mean_k O.render_rgb(...) on cells pinned to the fp32 positions -- pose_grad_cases._forward
with h * keep * scale behind the ReLU of every active site.  `oracle32`: the same through O.mcdropout_field(..., keep_trunk,
keep_head, p, keep_head0=...) in float32.

A ray is left out only by the float64 reference's own margins: those of pose_grad_cases, evaluated PER PASS.  A hidden
pre-activation within PRE_MARGIN of its kink counts only for units that are kept where dropout directly follows that ReLU: a
dropped unit has derivative 0 on both sides of the kink.  One margin is added to those of pose_grad_cases, the reference's own as
well: a selected sample whose fp32 scaled coordinate is an exact integer at some level of a torch-layout grid
(`_degenerate_cells`: the cell the reference pins there has no extent, its derivative is neither one-sided derivative of the
function).  At most MAX_EXCLUDED = 20 % of a case's rays may be left out
(test_pose_grad_mc_cpu.py asserts it for every case).  The rate grows with K * S -- every hidden pre-activation of every pass
may sit at its kink -- so the float64-held cases keep K * S <= 128; the workload's own shape, K = 8 x S = 48, leaves out about
a third of its rays and is covered by the linearity test instead ("lin48": never held to float64 as a whole, each of its
passes alone is).

Tolerance: on the kept rays max |g - g64| / rms(g64) <= KERNEL_FACTOR (4) x the fp32 oracle's own error, which the tests
compute themselves.  Nothing here comes from a kernel result."""
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import pose_grad_cases as PC
from oracle import nerf_oracle as O
from pose_grad_cases import (BOX_MARGIN, COLOR_MARGIN, COORD_MARGIN, KERNEL_FACTOR, PRE_MARGIN, _encode_pinned,  # noqa: F401
                             _field_tensors, _p32, _raw_color, euclid_bins32, make_case, rel_error)

MAX_EXCLUDED = 0.20
P_DROP = 0.2
MASK_SEED = 1234
R_CASE = 128
TRUNK, HEAD0, HEAD1 = 1, 2, 4
DEFAULT_SITES = TRUNK | HEAD1
STREAM = {TRUNK: 0, HEAD1: 1, HEAD0: 2}         # the generator's mask stream of each site
R_SUB = (1, 3, 4, 5)                            # sub-launches of the 257-ray case (one ray per block: any count is an edge)

_mc = dict(kind="mcdropout", R=R_CASE)
# name -> dict(scene = keyword arguments of pose_grad_cases.make_case, K, sites)
CASES = {
    "S1": dict(scene=dict(_mc, S=1, seed=1), K=8),
    "S2": dict(scene=dict(_mc, S=2, seed=1), K=8),
    "S16": dict(scene=dict(_mc, S=16, seed=1), K=8),
    "tcnn": dict(scene=dict(_mc, S=16, seed=1, grid="tcnn"), K=8),
    "tcnn_half": dict(scene=dict(_mc, S=16, seed=3, grid="tcnn", grid_half=True), K=8),
    "white": dict(scene=dict(_mc, S=16, seed=3, background="white"), K=8),
    "random": dict(scene=dict(_mc, S=16, seed=0, background="random"), K=4),
    "aabb": dict(scene=dict(_mc, S=16, seed=0, aabb=PC.AABB), K=8),
    "uniform": dict(scene=dict(_mc, S=16, seed=1, uniform=True, near=0.2, far=6.0), K=8),
    "S48K2": dict(scene=dict(_mc, S=48, seed=3), K=2),
    "S64K2": dict(scene=dict(_mc, S=64, seed=0), K=2),
    "S64K3": dict(scene=dict(_mc, S=64, seed=0), K=3),
    "S63K2": dict(scene=dict(_mc, S=63, seed=0), K=2),
    "S47K2": dict(scene=dict(_mc, S=47, seed=0), K=2),
    "K16": dict(scene=dict(_mc, S=8, seed=1), K=16),
    "K64": dict(scene=dict(_mc, S=2, seed=1), K=64),
    "head0": dict(scene=dict(_mc, S=16, seed=1), K=8, sites=HEAD0 | HEAD1),
    "trunk_only": dict(scene=dict(_mc, S=16, seed=1), K=8, sites=TRUNK),
}
# cases that are not held to float64 as a whole
LIN = dict(scene=dict(_mc, S=48, seed=3), K=8)                           # the workload's shape: linearity over the passes
GEOM = dict(scene=dict(kind="mcdropout", R=257, S=16, seed=1), K=2)      # launch geometry: bits only
EXTRA = {"lin48": LIN, "geom": GEOM}


def spec(name: str) -> SimpleNamespace:
    e = CASES[name] if name in CASES else EXTRA[name]
    return SimpleNamespace(c=make_case(**e["scene"]), K=int(e["K"]), sites=int(e.get("sites", DEFAULT_SITES)), p=P_DROP, seed=MASK_SEED)


def keep_masks(c, K: int, sites: int, seed: int = MASK_SEED, p: float = P_DROP, first: int = 0, rows=None):
    """-> per pass a dict {site bit: bool [n, 64] | None}: the counter generator's masks of samples first + (r * S + s) of the
    case's rays (rows = (first ray, number of rays); None: all)"""
    r0, n = (0, c.R) if rows is None else rows
    sidx = (np.arange(r0 * c.S, (r0 + n) * c.S) + int(first)).astype(np.uint32)
    return [{b: (torch.from_numpy(O.mc_keep_mask(seed, k, sidx, STREAM[b], 64, p)) if sites & b else None) for b in (TRUNK, HEAD0, HEAD1)}
            for k in range(K)]


def all_kept(c, K: int = 1):
    ones = torch.ones(c.R * c.S, 64, dtype=torch.bool)
    return [{TRUNK: ones, HEAD0: None, HEAD1: ones} for _ in range(K)]


def pack_bits(keep: torch.Tensor) -> torch.Tensor:
    """bool [..., 64] -> int32 [..., 2] in the layout of unerf_keep_masks (bit u & 31 of word u >> 5 = unit u kept)"""
    k = keep.to(torch.int64).reshape(*keep.shape[:-1], 2, 32)
    words = (k << torch.arange(32, dtype=torch.int64)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def _forward_mc(c, ft, o, d, eb, p32, masks, p: float, want_margins: bool):
    """pose_grad_cases._forward with the keep masks of every pass -> mean_k clamp(pred_k) [R,3], margins [R] | None"""
    R, S = c.R, c.S
    scale = 1.0 / (1.0 - p)
    pos = O.sample_positions(o, d, eb)
    pn_, sel = O.normalized_positions(pos, ft.aabb)
    feat, scaled = _encode_pinned(c, ft, pn_.reshape(-1, 3), p32)
    pre0 = F.linear(feat, ft.w0, ft.b0)
    h0 = F.relu(pre0)
    deltas = eb[..., 1:] - eb[..., :-1]
    bad = torch.zeros(R, dtype=torch.bool)
    preds = []

    def drop(h, keep):
        return h if keep is None else h * keep.to(h.dtype) * scale

    def kinks(pre, keep):     # a pre-activation at its kink, on a unit whose derivative is not 0 on both sides
        near = pre.abs() < PRE_MARGIN
        if keep is not None:
            near = near & keep
        return near.view(R, S, -1).any(-1).any(-1)

    for mk in masks:
        out = F.linear(drop(h0, mk[TRUNK]), ft.w1, ft.b1).view(R, S, -1)
        density = ft.aid * torch.exp(out[..., 0]) * sel
        x = O._color_inputs(d, S, out[..., 1:16], ft.appearance, ft.sh_remap)
        pre1 = F.linear(x, ft.head_w[0], ft.head_b[0])
        pre2 = F.linear(drop(F.relu(pre1), mk[HEAD0]), ft.head_w[1], ft.head_b[1])
        rgb = torch.sigmoid(F.linear(drop(F.relu(pre2), mk[HEAD1]), ft.head_w[2], ft.head_b[2])).view(R, S, 3)
        w = O.get_weights(density, deltas)
        preds.append(O.render_rgb(rgb, w, c.background))
        if want_margins:
            with torch.no_grad():
                bad |= kinks(pre0, mk[TRUNK]) | kinks(pre1, mk[HEAD0]) | kinks(pre2, mk[HEAD1])
                raw = _raw_color(rgb, w, c.background)
                bad |= ((raw.abs() < COLOR_MARGIN) | ((raw - 1).abs() < COLOR_MARGIN)).any(-1)
    pred = torch.stack(preds).mean(0)
    if not want_margins:
        return pred, None
    with torch.no_grad():     # the pass-independent margins, as pose_grad_cases._forward
        if ft.aabb is None:
            a = pos.abs().sort(dim=-1, descending=True).values
            m = a[..., 0]
            bad |= ((m - 1).abs() < BOX_MARGIN).any(-1)
            bad |= ((m >= 1) & (a[..., 0] - a[..., 1] < BOX_MARGIN)).any(-1)
            pn = (O.contract_inf(pos) + 2.0) / 4.0
        else:
            pn = (pos - ft.aabb[0]) / (ft.aabb[1] - ft.aabb[0])
        bad |= ((pn.abs() < COORD_MARGIN) | ((pn - 1).abs() < COORD_MARGIN)).any(-1).any(-1)
        near_int = ((scaled - torch.round(scaled)).abs() < COORD_MARGIN).any(-1).any(-1).view(R, S)
        bad |= (near_int & sel).any(-1)
        bad |= (_degenerate_cells(c, p32).view(R, S) & sel).any(-1)
    return pred, ~bad


def _degenerate_cells(c, p32: torch.Tensor) -> torch.Tensor:
    """[N] bool: the cell the fp32 position pins is degenerate at some level.  O.hash_indices takes the corners of the torch
    layout from ceil and floor of the fp32 scaled coordinate; where that coordinate is an exact integer both are the same
    vertex, the pinned "cell" has no extent along that axis and the reference's derivative along it is 0 -- neither one-sided
    derivative of the function.  It is the integer kink itself, met in fp32 while the float64 coordinate may stand just
    outside COORD_MARGIN (1.07e-6 was seen), so it is the reference's own margin.  (The tcnn layout pins floor and floor + 1.)"""
    f = c.t["field"]
    if f.get("tcnn_levels") is not None:
        return torch.zeros(p32.shape[0], dtype=torch.bool)
    _, off32 = O.hash_indices(p32, f["scalings"], int(f["log2T"]))
    return (off32 == 0).any(-1).any(-1)


def grad64(c, masks, p: float, origins=None, directions=None) -> SimpleNamespace:
    """float64 autograd of the masked render of case object c -> grad [R,6] = (ds/do, ds/dd), rgb [R,3], keep [R]"""
    ft = _field_tensors(c, torch.float64)
    p32 = _p32(c, _field_tensors(c, torch.float32))
    o = (c.origins if origins is None else origins).double().clone().requires_grad_(True)
    d = (c.directions if directions is None else directions).double().clone().requires_grad_(True)
    pred, keep = _forward_mc(c, ft, o, d, euclid_bins32(c).double(), p32, masks, p, True)
    go, gd = torch.autograd.grad(pred.mean(-1).sum(), (o, d))
    return SimpleNamespace(grad=torch.cat([go, gd], dim=-1), rgb=pred.detach(), keep=keep)


def render64(c, masks, p: float, o: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    """s [R] float64 of the masked render at other origins / directions, the cells pinned to the case's own fp32 positions"""
    p32 = _p32(c, _field_tensors(c, torch.float32))
    with torch.no_grad():
        pred, _ = _forward_mc(c, _field_tensors(c, torch.float64), o, d, euclid_bins32(c).double(), p32, masks, p, False)
    return pred.mean(-1)


def _passes(s, passes):
    mk = keep_masks(s.c, s.K, s.sites, s.seed, s.p)
    return mk if passes is None else [mk[k] for k in passes]


@functools.lru_cache(maxsize=None)
def reference64(name: str, passes=None) -> SimpleNamespace:
    """the float64 reference of a case; passes = a tuple of pass indices: the mean over those passes only"""
    s = spec(name)
    return grad64(s.c, _passes(s, passes), s.p)


@functools.lru_cache(maxsize=None)
def oracle32(name: str, passes=None) -> SimpleNamespace:
    """the fp32 torch oracle's own gradient: autograd through O.mcdropout_field under the same masks, O.get_weights,
    O.render_rgb in float32, the mean over the passes taken in float32 too"""
    s = spec(name)
    c = s.c
    t = dict(c.t)
    if c.grid_half:
        t["field"] = dict(t["field"], table=t["field"]["table"].to(torch.float16).to(torch.float32))
        t["grid_precision"] = "f32"
    sc = O.scene_from_tensors(t)
    o = c.origins.clone().requires_grad_(True)
    d = c.directions.clone().requires_grad_(True)
    eb = euclid_bins32(c)
    preds = []
    for mk in _passes(s, passes):
        density, rgb = O.mcdropout_field(o, d, eb, sc.field, mk[TRUNK], mk[HEAD1], s.p, keep_head0=mk[HEAD0])
        preds.append(O.render_rgb(rgb, O.get_weights(density, eb[..., 1:] - eb[..., :-1]), sc.background))
    pred = torch.stack(preds).mean(0)
    go, gd = torch.autograd.grad(pred.mean(-1).sum(), (o, d))
    return SimpleNamespace(grad=torch.cat([go, gd], dim=-1), rgb=pred.detach())
