"""Cases and references for the per-ray pose Jacobian (plain module: tests import it; nothing here needs a GPU).

unerf_pose_jacobian (csrc/unerf_nerf.hip, section 5e-J) returns one row per rendered channel -- clamp(pred_r), clamp(pred_g),
clamp(pred_b), the accumulation A = sum w, the UNCLIPPED expected depth sum w t / (sum w + 1e-10) with t the bin mid-points --
with respect to the ray origin and direction, the bins held fixed.

Cases: those of tests/pose_grad_cases.py under their names (imported, not copied), and two S = 16 plants built on one of
them with a changed field:
  opaque  the grid table times OPAQUE_TABLE_SCALE: most rays reach delta sigma >= 50 within their first three selected
          samples (everything behind is hidden: the suffix sums of the adjoints are what is tested)
  empty   average_init_density = EMPTY_DENSITY: A < 1e-6 on every ray (the quotient of the expected depth at a vanishing
          denominator)

Reference (`reference64`): float64 autograd of the pinned-cell graph of pose_grad_cases._forward (O.sample_positions ->
O.normalized_positions -> pinned blend -> trunk / head -> O.get_weights) with five outputs per ray: O.render_rgb's three
channels, O.render_accumulation, and the unclipped quotient -> J64 [R,5,6], values [R,5], keep [R].  keep is
pose_grad_cases.reference64(name).keep for the shared names (accumulation and expected depth add no kink, so no margin);
for the plants it comes from the same four margins (pose_grad_cases._forward).

Yardstick (`oracle32`): float32 autograd through O.mcdropout_field for the same five outputs.  Error of row c:
max |J_c - J64_c| / rms(J64_c) over the kept rays; a row whose rms(J64_c) is 0 (every kept ray clamped) must be exactly 0.
The kernel is allowed pose_grad_cases.KERNEL_FACTOR x the oracle's own error of the same row on the same rays.  Nothing here
comes from a kernel result."""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import pose_grad_cases as PC
from oracle import nerf_oracle as O

MAX_EXCLUDED = PC.MAX_EXCLUDED
KERNEL_FACTOR = PC.KERNEL_FACTOR
CHANNELS = ("r", "g", "b", "accumulation", "expected_depth")
GUARD = 16                      # guard floats in front of and behind every output buffer of the GPU tests
OPAQUE_TABLE_SCALE = 9.0
EMPTY_DENSITY = 1e-8

# make_case's keyword arguments, plus the change of the field
PLANTS = {
    "opaque": dict(kind="active", R=PC.R_CASE, S=16, seed=1, table_scale=OPAQUE_TABLE_SCALE),
    "empty": dict(kind="mcdropout", R=PC.R_CASE, S=16, seed=3, average_init_density=EMPTY_DENSITY),
}
CASES = {**PC.CASES, **PLANTS}


@functools.lru_cache(maxsize=None)
def case(name: str) -> SimpleNamespace:
    if name in PC.CASES:
        return PC.case(name)
    kw = dict(PLANTS[name])
    scale, aid = kw.pop("table_scale", None), kw.pop("average_init_density", None)
    base = PC.make_case(**kw)
    t = dict(base.t)
    t["field"] = dict(t["field"])
    if scale is not None:
        t["field"]["table"] = t["field"]["table"] * scale
    if aid is not None:
        t["field"]["average_init_density"] = aid
    c = SimpleNamespace(**vars(base))     # the base case's rays and bins: the proposal networks are not changed
    c.t = t
    return c


def steps_of(eb: torch.Tensor) -> torch.Tensor:
    return (eb[..., :-1] + eb[..., 1:]) / 2


def _forward5(c, ft, o, d, eb, p32):
    """pose_grad_cases._forward's graph -> ([R,5] = rgb, accumulation, unclipped expected depth; weights [R,S];
    delta sigma [R,S])"""
    R, S = c.R, c.S
    pos = O.sample_positions(o, d, eb)
    p, sel = O.normalized_positions(pos, ft.aabb)
    feat, _ = PC._encode_pinned(c, ft, p.reshape(-1, 3), p32)
    out = F.linear(F.relu(F.linear(feat, ft.w0, ft.b0)), ft.w1, ft.b1).view(R, S, -1)
    density = ft.aid * torch.exp(out[..., 0]) * sel
    x = O._color_inputs(d, S, out[..., 1:16], ft.appearance, ft.sh_remap)
    h = F.relu(F.linear(x, ft.head_w[0], ft.head_b[0]))
    h = F.relu(F.linear(h, ft.head_w[1], ft.head_b[1]))
    rgb = torch.sigmoid(F.linear(h, ft.head_w[2], ft.head_b[2])).view(R, S, 3)
    deltas = eb[..., 1:] - eb[..., :-1]
    w = O.get_weights(density, deltas)
    return five_outputs(rgb, w, eb, c.background), w, (deltas * density).detach()


def five_outputs(rgb, w, eb, background):
    acc = O.render_accumulation(w)
    depth = torch.sum(w * steps_of(eb), dim=-1, keepdim=True) / (torch.sum(w, -1, keepdim=True) + 1e-10)
    return torch.cat([O.render_rgb(rgb, w, background).to(w.dtype), acc, depth], dim=-1)


def _pins(c):
    return PC._p32(c, PC._field_tensors(c, torch.float32))


def jac64_at(name: str, origins: torch.Tensor, directions: torch.Tensor, want_keep: bool = True) -> SimpleNamespace:
    """float64 autograd at the given rays (cells pinned to the case's own fp32 positions)
    -> jac [R,5,6], val [R,5], keep [R] | None, weights [R,S], delta_sigma [R,S]"""
    c = case(name)
    ft = PC._field_tensors(c, torch.float64)
    p32 = _pins(c)
    eb = PC.euclid_bins32(c).double()
    o = origins.double().clone().requires_grad_(True)
    d = directions.double().clone().requires_grad_(True)
    out, w, dd = _forward5(c, ft, o, d, eb, p32)
    rows = []
    for k in range(5):
        go, gd = torch.autograd.grad(out[:, k].sum(), (o, d), retain_graph=True)
        rows.append(torch.cat([go, gd], dim=-1))
    keep = None
    if want_keep:
        if name in PC.CASES and origins is c.origins and directions is c.directions:
            keep = PC.reference64(name).keep
        else:
            with torch.no_grad():
                keep = PC._forward(c, ft, o.detach(), d.detach(), eb, p32, True)[1]
    return SimpleNamespace(jac=torch.stack(rows, dim=1), val=out.detach(), keep=keep, weights=w.detach(), delta_sigma=dd)


@functools.lru_cache(maxsize=None)
def reference64(name: str) -> SimpleNamespace:
    c = case(name)
    return jac64_at(name, c.origins, c.directions)


def render64(name: str, o: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    """the five outputs [R,5] float64 at other rays, the cells still pinned (central differences of the same function)"""
    c = case(name)
    with torch.no_grad():
        return _forward5(c, PC._field_tensors(c, torch.float64), o, d, PC.euclid_bins32(c).double(), _pins(c))[0]


@functools.lru_cache(maxsize=None)
def oracle32(name: str) -> SimpleNamespace:
    """the fp32 torch oracle's own Jacobian: autograd through O.mcdropout_field (no masks), O.get_weights and the renderers
    in float32 -> jac [R,5,6] float32, val [R,5], weights [R,S]"""
    c = case(name)
    t = dict(c.t)
    if c.grid_half:
        t["field"] = dict(t["field"], table=t["field"]["table"].to(torch.float16).to(torch.float32))
        t["grid_precision"] = "f32"
    sc = O.scene_from_tensors(t)
    o = c.origins.clone().requires_grad_(True)
    d = c.directions.clone().requires_grad_(True)
    eb = PC.euclid_bins32(c)
    density, rgb = O.mcdropout_field(o, d, eb, sc.field, None, None, 0.0)
    w = O.get_weights(density, eb[..., 1:] - eb[..., :-1])
    out = five_outputs(rgb, w, eb, sc.background)
    rows = []
    for k in range(5):
        go, gd = torch.autograd.grad(out[:, k].sum(), (o, d), retain_graph=True)
        rows.append(torch.cat([go, gd], dim=-1))
    return SimpleNamespace(jac=torch.stack(rows, dim=1), val=out.detach(), weights=w.detach())


def row_errors(jac, ref: SimpleNamespace, j64=None):
    """per row c: (max |J_c - J64_c| over the kept rays / rms(J64_c over the kept rays), rms); a row whose rms is 0 reports
    its max |J_c| unscaled.  jac, j64: [R,5,D]"""
    j64 = ref.jac if j64 is None else j64
    k = ref.keep
    g = torch.as_tensor(jac).double().cpu()
    out = []
    for ch in range(j64.shape[1]):
        rms = j64[k, ch].pow(2).mean().sqrt().item()
        diff = (g[k, ch] - j64[k, ch]).abs().max().item()
        out.append((diff / rms if rms > 0 else diff, rms))
    return out


def value_errors(val, ref: SimpleNamespace):
    """per channel: max |val_c - val64_c| over the kept rays / rms(val64_c) (unscaled where that is 0)"""
    k = ref.keep
    v = torch.as_tensor(val).double().cpu()
    out = []
    for ch in range(ref.val.shape[1]):
        rms = ref.val[k, ch].pow(2).mean().sqrt().item()
        diff = (v[k, ch] - ref.val[k, ch]).abs().max().item()
        out.append(diff / rms if rms > 0 else diff)
    return out


def pose_rows(j6: torch.Tensor, d: torch.Tensor, rot_inv: torch.Tensor) -> torch.Tensor:
    """[R,C,6] -> [R,C,12]: pose_grad_cases.pose_from_ray_grad per row"""
    return torch.stack([PC.pose_from_ray_grad(j6[:, ch], d, rot_inv).reshape(-1, 12) for ch in range(j6.shape[1])], dim=1)


def sheared_rotation() -> torch.Tensor:
    """a scaled, non-orthonormal 3x3 block (the D = 12 epilogue holds for any invertible R)"""
    g = torch.Generator().manual_seed(5)
    R = PC.synthetic.orbit_c2w(0.8).double()[:, :3]
    return (R @ (torch.eye(3, dtype=torch.float64) * 1.7 + 0.2 * torch.randn(3, 3, generator=g, dtype=torch.float64))).float()
