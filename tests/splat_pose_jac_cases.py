"""Cases and float64 references of the splat pose Jacobian (plain module: tests import it; nothing here needs a GPU or reads a
kernel result).  The cases, the projection restatement and the coin-flip-free construction are those of
tests/splat_pose_grad_cases.py (SPG), which is imported and left as it is.

The quantities, per pixel and pose direction p: rows of r, g, b, accumulation and expected depth (ops.POSE_CHANNELS order)

  r, g, b : value min(pix_c + T bg_c, 1)     row live_c (dpix_c + bg_c dT),  live_c = pix_c + T bg_c < 1
  acc     : value A = 1 - T                  row -dT
  depth   : A > 0: value D / A               row dD / A + (D / A) dT / A;     A == 0: value and row 0

with D = sum_i z_i alpha_i T_i the unnormalised depth sum, and for a blended pair the recurrences of DESIGN.md 4.6b plus
dD += z (adot T + alpha dT) + zdot alpha T.

  * `contract`: the per-splat contraction tangents [N,6,12] x proj [12,P] -> [N,7,P] (row 6: the depth tangent (m, 1) . proj[8:12],
    zeros for dead splats).
  * `blend_jac`: the recurrences on the schedule of SO.rasterize_f64 in float64 (or float32: the yardstick), with the kernel's
    fp32 thresholds.
  * `frame_jac_reference`: SPG.tangents_ref, the contraction and the blend composed, V -> c2w by autograd through SPG.viewmat_t.
  * `frame_jac64`: the pure-float64 frame as a function of c2w with pinned decisions (self-check by central differences).

Tolerance: the error of a row set is max |g - g64| / rms(g64) PER CHANNEL over the compared elements (`channel_errors`); a kernel
is allowed SPG.KERNEL_FACTOR x the float32 restatement's error.  Exclusions are SPG's: the zeroed-splat rounds of its builders,
and pixels with a colour channel inside ONE_BAND of the clamp (at most SPG.MAX_PIXELS_OUT of a case's).  Every pixel with A > 0
has A >= 1/255 (a blended alpha is), so no depth row is excluded.

The float32 restatement's exponential.  The walk must blend with raster_kernel's alpha bit for bit (its rgb and final_T are held
bit-equal to the gradient kernel's), and that alpha is o * __expf(-sigma): HIP defines __expf(x) as the hardware's base-2
exponential of the fp32 product x * log2(e).  The rounding of that product, |x| log2(e) 2^-24 in the exponent, reaches alpha as
a relative ln(2) |x log2(e)| 2^-24 -- several half-ulps of alpha, which T = prod (1 - alpha) magnifies by 1 / (1 - alpha) for
the `stops` case's splats that leave the 0.999 clamp inside a quadrant.  A float32 run with a correctly rounded exp (np.exp on
float32) does not carry this term, although no float32 walk that keeps the rasteriser's alpha can avoid it, so the yardstick
takes the exponential in the same float32 steps (`exp_f32`: one rounded product, one correctly rounded exp2).  First written
with np.exp, the yardstick put the accumulation row of `stops` at 8.7 x (classic, no background; colours 1.7 - 2.1 x) on the
GPU; with `exp_f32` the CPU restatement reproduces the kernel's errors of every channel to four digits (4.102e-05 for that
row), which is what identified the term.  `walk_ref_plain_exp` keeps the np.exp run so that the tests can print both."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import splat_pose_grad_cases as SPG
from oracle import splat_oracle as SO

f32, f64 = np.float32, np.float64
CHANNELS = ("r", "g", "b", "accumulation", "expected_depth")
MUTATIONS = ("no_zdot", "no_quot_dT", "acc_sign", "proj_transposed", "no_live_gate")
A_MIN = float(f32(1.0) / f32(255.0))


def exp_f32(x):
    """__expf in float32 steps: the correctly rounded exp2 of the fp32 product x * log2(e)"""
    y = (np.asarray(x, f32) * f32(1.4426950408889634)).astype(f32)
    with np.errstate(over="ignore"):
        return np.exp2(y.astype(f64)).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------
# the per-splat contraction
# ---------------------------------------------------------------------------------------------------------------------
def contract(tan, means, live, M, dtype=f64, mutate=None):
    """tan [N,6,12], means [N,3], live [N] bool, M [12,P] -> [N,7,P] in `dtype` (products and sums in `dtype`, k in order)"""
    dt = dtype
    tan, means, M = np.asarray(tan).astype(dt), np.asarray(means).astype(dt), np.asarray(M).astype(dt)
    if mutate == "proj_transposed":
        assert M.shape == (12, 12)
        M = M.T
    N, P = len(means), M.shape[1]
    out = np.zeros((N, 7, P), dt)
    for k in range(12):
        out[:, :6] += tan[:, :, k, None] * M[k]
    m1 = np.concatenate([means, np.ones((N, 1), dt)], 1)
    z = np.zeros((N, P), dt)
    for c in range(4):
        z += m1[:, c, None] * M[8 + c]
    out[:, 6] = np.where(np.asarray(live)[:, None], z, 0)
    return out


def contract_bound(tan, means, live, M):
    """the forward bound of the fp32 contraction per element: 13 x 2^-24 x sum_k |tangent_k proj_k| (12 products, 11 sums)"""
    tan, means, M = np.abs(np.asarray(tan, f64)), np.abs(np.asarray(means, f64)), np.abs(np.asarray(M, f64))
    out = np.zeros((len(means), 7, M.shape[1]))
    out[:, :6] = tan @ M
    out[:, 6] = np.where(np.asarray(live)[:, None], np.concatenate([means, np.ones((len(means), 1))], 1) @ M[8:12], 0)
    return 13 * 2.0 ** -24 * out


# ---------------------------------------------------------------------------------------------------------------------
# the blend in forward mode, five channels
# ---------------------------------------------------------------------------------------------------------------------
def blend_jac(gids, bins, xys, conics, colors, depths, opac, ptan, H, W, bg=None, comp=None, bw=16, dtype=f64, mutate=None,
              pins=None, record=False, exp_fn=None):
    """The recurrences of unerf_splat_pose_jacobian on the schedule of SO.rasterize_f64, every quantity in `dtype` on the given
    inputs (thresholds: the kernel's fp32 constants).  ptan [N,7,P] (None: forward only); comp [N] (antialiased) or None.
    pins: a record of an earlier run whose blend / clamp decisions are replayed.
    -> SimpleNamespace(rows [H,W,5,P], val [H,W,5], raw [H,W,3] (unclamped colour), T, D [H,W], rec)"""
    dt = dtype
    if exp_fn is None:       # float32: the rasteriser's exponential (see the module's docstring)
        exp_fn = exp_f32 if dt == f32 else np.exp
    xys, conics, colors = (np.asarray(a).astype(dt) for a in (xys, conics, colors))
    opac, zs = np.asarray(opac).reshape(-1).astype(dt), np.asarray(depths).reshape(-1).astype(dt)
    bgv = np.zeros(3, dt) if bg is None else np.asarray(bg).astype(dt)
    tanv = None if ptan is None else np.asarray(ptan).astype(dt)
    P = 1 if tanv is None else tanv.shape[2]
    invc = None if comp is None else (1.0 / np.maximum(np.asarray(comp).astype(dt), dt(1e-30)))
    a_max, a_min, t_min = dt(f32(0.999)), dt(f32(1.0) / f32(255.0)), dt(f32(1e-4))
    tbx, tby = (W + bw - 1) // bw, (H + bw - 1) // bw
    rows, val = np.zeros((H, W, 5, P), dt), np.zeros((H, W, 5), dt)
    raw_img, Tim, Dim = np.zeros((H, W, 3), dt), np.ones((H, W), dt), np.zeros((H, W), dt)
    rec = {}
    half, one = dt(0.5), dt(1)
    for ty in range(tby):
        for tx in range(tbx):
            r0, r1 = bins[ty * tbx + tx]
            ys, xs = np.arange(ty * bw, min((ty + 1) * bw, H)), np.arange(tx * bw, min((tx + 1) * bw, W))
            win = (slice(ys[0], ys[-1] + 1), slice(xs[0], xs[-1] + 1))
            py, px = np.meshgrid(ys.astype(dt) + half, xs.astype(dt) + half, indexing="ij")
            T, pix, D = np.ones(py.shape, dt), np.zeros(py.shape + (3,), dt), np.zeros(py.shape, dt)
            dT, dpix, dD = np.zeros(py.shape + (P,), dt), np.zeros(py.shape + (3, P), dt), np.zeros(py.shape + (P,), dt)
            done = np.zeros(py.shape, bool)
            for idx in range(r0, r1):
                if pins is None and done.all():
                    break
                g = gids[idx]
                dx, dy = xys[g, 0] - px, xys[g, 1] - py
                ca, cb, cc = conics[g]
                sigma = half * (ca * dx * dx + cc * dy * dy) + cb * dx * dy
                with np.errstate(over="ignore", invalid="ignore"):
                    raw = opac[g] * exp_fn(-sigma)
                if pins is None:
                    alpha = np.minimum(a_max, raw)
                    clamped = raw > a_max
                    act = ~done & ~((sigma < 0) | (alpha < a_min))
                    nT = T * (1 - alpha)
                    stop = act & (nT <= t_min)
                    done |= stop
                    act &= ~stop
                    if record:
                        rec[idx] = (act.copy(), clamped.copy())
                else:
                    if idx not in pins:
                        continue
                    act, clamped = pins[idx]
                    alpha = np.where(clamped, a_max, raw)
                    nT = T * (1 - alpha)
                vis = alpha * T
                if tanv is not None and act.any():
                    tq = tanv[g]
                    sd = ((ca * dx + cb * dy)[..., None] * tq[0] + (cc * dy + cb * dx)[..., None] * tq[1]
                          + (half * dx * dx)[..., None] * tq[2] + (dx * dy)[..., None] * tq[3] + (half * dy * dy)[..., None] * tq[4])
                    ad = -alpha[..., None] * sd
                    if invc is not None:
                        ad = ad + (alpha * invc[g])[..., None] * tq[5]
                    ad = np.where(clamped[..., None], 0, ad)
                    wk = ad * T[..., None] + alpha[..., None] * dT
                    dpix[act] += (colors[g][:, None] * wk[:, :, None, :])[act]
                    dz = zs[g] * wk
                    if mutate != "no_zdot":
                        dz = dz + vis[..., None] * tq[6]
                    dD[act] += dz[act]
                    dT[act] = (dT * (1 - alpha)[..., None] - T[..., None] * ad)[act]
                pix[act] += colors[g][None, :] * vis[act][:, None]
                D[act] += zs[g] * vis[act]
                T[act] = nT[act]
            v = pix + T[..., None] * bgv
            live = np.ones(v.shape, bool) if mutate == "no_live_gate" else v < 1
            A = one - T
            hit = A > 0
            As = np.where(hit, A, one)
            e = np.where(hit, D / As, 0)
            r = np.zeros(py.shape + (5, P), dt)
            r[..., :3, :] = np.where(live[..., None], dpix + bgv[:, None] * dT[..., None, :], 0)
            r[..., 3, :] = dT if mutate == "acc_sign" else -dT
            quot = dD / As[..., None]
            if mutate != "no_quot_dT":
                quot = quot + e[..., None] * dT / As[..., None]
            r[..., 4, :] = np.where(hit[..., None], quot, 0)
            rows[win] = r
            val[win] = np.concatenate([np.minimum(v, one), A[..., None], e[..., None]], -1)
            raw_img[win], Tim[win], Dim[win] = v, T, D
    return SimpleNamespace(rows=rows, val=val, raw=raw_img, T=Tim, D=Dim, rec=rec)


def channel_errors(g, g64, keep) -> np.ndarray:
    """[..., C, (P)] results -> per channel max |g - g64| / rms(g64) over the kept pixels"""
    g, g64 = np.asarray(g, f64)[keep], np.asarray(g64, f64)[keep]
    C = g64.shape[1]
    g, g64 = g.reshape(len(g), C, -1), g64.reshape(len(g64), C, -1)
    rms = np.sqrt((g64 ** 2).mean((0, 2)))
    return np.abs(g - g64).max((0, 2)) / np.where(rms > 0, rms, 1.0)


def within(what, got, r64, r32, keep, factor=SPG.KERNEL_FACTOR, channels=CHANNELS, verbose=True) -> bool:
    """every channel of `got` inside factor x the float32 yardstick; prints each ratio"""
    e32, err = channel_errors(r32, r64, keep), channel_errors(got, r64, keep)
    ok = True
    for c, name in enumerate(channels):
        if verbose:
            print(f"RATIO {what} {name}: error {err[c]:.3e} yardstick {e32[c]:.3e} ratio {err[c] / e32[c] if e32[c] > 0 else 0.0:.2f}")
        ok &= bool(e32[c] > 0 and err[c] <= factor * e32[c])
    return ok


# ---------------------------------------------------------------------------------------------------------------------
# walk cases: SPG's hand-built lists with a random projection, depths and depth tangents
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def walk_inputs(name):
    """-> SimpleNamespace(proj [12,12] f32 (its first six columns: the P = 6 call's), ptan [N,7,12] f32 = the fp32 rounding of the
    float64 contraction of the case's tangents (row 6: random), z [N] f32): what the walk kernel and its references both read"""
    c = SPG.WALK[name]()
    rng = np.random.default_rng([SPG.SEEDS[name], 177])
    proj = rng.standard_normal((12, 12)).astype(f32)
    ptan = np.zeros((c.N, 7, 12), f32)
    ptan[:, :6] = (c.tan.astype(f64) @ proj.astype(f64)).astype(f32)
    ptan[:, 6] = (0.5 * rng.standard_normal((c.N, 12))).astype(f32)
    z = rng.uniform(0.5, 6.0, c.N).astype(f32)
    for a in (proj, ptan, z):
        a.setflags(write=False)
    return SimpleNamespace(proj=proj, ptan=ptan, z=z)


@functools.lru_cache(maxsize=None)
def walk_ref(name, aa: bool, bg: str):
    """bg: "none" | "color" -> (float64 run, float32 run, keep [H,W]) of a walk case at P = 12; a P = 6 call's reference is the
    first six columns (the columns are independent)"""
    c, w = SPG.WALK[name](), walk_inputs(name)
    bgv = {"none": None, "color": c.bg}[bg]
    a = (c.gids, c.bins, c.xys, c.conics, c.colors, w.z, c.opac, w.ptan, c.H, c.W)
    r64 = blend_jac(*a, bg=bgv, comp=c.comp if aa else None, bw=c.bw)
    r32 = blend_jac(*a, bg=bgv, comp=c.comp if aa else None, bw=c.bw, dtype=f32)
    return r64, r32, SPG.keep_mask(r64.raw)


def walk_ref_plain_exp(name, aa: bool, bg: str):
    """the float32 run of walk_ref with a correctly rounded exp in place of exp_f32 (printed next to the yardstick, not a bound)"""
    c, w = SPG.WALK[name](), walk_inputs(name)
    return blend_jac(c.gids, c.bins, c.xys, c.conics, c.colors, w.z, c.opac, w.ptan, c.H, c.W, bg={"none": None, "color": c.bg}[bg],
                     comp=c.comp if aa else None, bw=c.bw, dtype=f32, exp_fn=np.exp)


# ---------------------------------------------------------------------------------------------------------------------
# whole frames
# ---------------------------------------------------------------------------------------------------------------------
def depth_tangents_V(means, live, dtype=f64):
    """d z / d V[:3,:4] [N,12] for z = V[2] . (m, 1): (0 x 8, m0, m1, m2, 1); zeros for dead splats"""
    out = np.zeros((len(means), 12), dtype)
    out[:, 8:11], out[:, 11] = means, 1
    return np.where(np.asarray(live)[:, None], out, 0)


def viewmat_jacobian_autograd(c2w) -> np.ndarray:
    """[12 V entries, 12 c2w entries] float64 by autograd through SPG.viewmat_t"""
    c = torch.as_tensor(np.asarray(c2w, f64)[:3, :4])
    return torch.autograd.functional.jacobian(lambda x: SPG.viewmat_t(x).reshape(-1), c).reshape(12, 12).numpy()


def frame_jac_reference(f, dtype=f64):
    """-> SimpleNamespace(rows [H,W,5,12] = d channel / d c2w, val [H,W,5], raw, keep, A [H,W]).
    float64: the frame as a function of the STORED parameters (activations, projection and blend in float64; lists and branch
    decisions the fp32 oracle's), the rows with respect to V mapped to c2w by autograd through SPG.viewmat_t.
    float32 (the yardstick): the fp32 oracle's own projection, depths and colours, the tangents by float32 forward mode, their
    float32 contraction with the fp32 rounding of the same [12,12] map, the blend in float32 -- the order the kernels work in."""
    cam = f.cam
    V = SO.viewmat_from_c2w(f.c2w)[:3]
    pins = SPG.projection_pins(f.means, V, cam["fx"], cam["fy"], cam["H"], cam["W"], f.proj)
    a = (pins, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    Jvc = viewmat_jacobian_autograd(f.c2w)
    if dtype == f64:
        sub = {k: v[f.index] for k, v in f.gp.items()}
        q, J = SPG.tangents_ref(V, f.means, SPG.shape64(sub), *a)
        opac = 1.0 / (1.0 + np.exp(-sub["opacities"].astype(f64).reshape(-1)))
        comp = q[:, 5] if f.comp is not None else None
        z = np.concatenate([f.means.astype(f64), np.ones((len(f.means), 1))], 1) @ V.astype(f64)[2]
        ptan = np.concatenate([J, depth_tangents_V(f.means, pins.live)[:, None, :]], 1)
        r = blend_jac(f.gids, f.bins, q[:, :2], q[:, 2:5], SPG.colors64(sub, f.c2w, f.sh0), z, opac if comp is None else opac * comp,
                      ptan, cam["H"], cam["W"], bg=SPG.FRAME_BG, comp=comp)
        rows = r.rows @ Jvc
    else:
        _, J = SPG.tangents_ref(V, f.means, f.proj["cov3d"], *a, torch.float32)
        ptan = contract(J, f.means, pins.live, Jvc.astype(f32), f32)
        r = blend_jac(f.gids, f.bins, f.xys, f.conics, f.colors, f.proj["depths"], f.opac, ptan, cam["H"], cam["W"], bg=SPG.FRAME_BG,
                      comp=f.comp, dtype=f32)
        rows = r.rows
    return SimpleNamespace(rows=rows, val=r.val, raw=r.raw, keep=SPG.keep_mask(r.raw.astype(f64)), A=r.val[..., 3], D=r.D)


def frame_jac64(f, c2w64: np.ndarray, pins_proj, rec=None, want_jac=False):
    """the five channels [H,W,5] (and their rows with respect to c2w [H,W,5,12]) of the float64 frame at pose c2w64 with lists,
    cull / clamp decisions (pins_proj) and, given `rec`, the blend's per-pair decisions pinned"""
    cam = f.cam
    V = SPG.viewmat_t(torch.as_tensor(np.asarray(c2w64, f64)[:3, :4]))
    a = (f.means, f.proj["cov3d"], pins_proj, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    if want_jac:
        q, J = SPG.tangents_ref(V.numpy(), *a)
        ptan = np.concatenate([J, depth_tangents_V(f.means, pins_proj.live)[:, None, :]], 1)
    else:
        q, ptan = SPG.project_q(V, torch.as_tensor(f.means), torch.as_tensor(f.proj["cov3d"]), *a[2:]).numpy(), None
    z = np.concatenate([f.means.astype(f64), np.ones((len(f.means), 1))], 1) @ V.numpy()[2]
    opac = f.opac.astype(f64)
    comp = None
    if f.comp is not None:
        comp = q[:, 5]
        with np.errstate(all="ignore"):
            base = np.where(f.comp > 0, f.opac.astype(f64) / f.comp.astype(f64), 0.0)
        opac = base * comp
    r = blend_jac(f.gids, f.bins, q[:, :2], q[:, 2:5], f.colors, z, opac, ptan, cam["H"], cam["W"], bg=SPG.FRAME_BG, comp=comp,
                  pins=rec, record=rec is None)
    rows = r.rows @ viewmat_jacobian_autograd(c2w64) if want_jac else None
    return SimpleNamespace(val=r.val, raw=r.raw, rec=r.rec, rows=rows)
