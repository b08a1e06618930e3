"""Cases and float64 references of the splat pose gradient (plain module: tests import it; nothing here needs a GPU or reads a
kernel result).

The quantity: s = mean_c min(pix_c + T_end bg_c, 1) of a pixel, differentiated with respect to the 12 entries of
camera_to_worlds through V = [R'^T | -R'^T t] (R' = R diag(1,-1,-1): the reference's transposition, not an inverse), the
projection of oracle.splat_oracle.project_gaussians and the blend of its rasteriser; near-plane cull, radii, lists, skipped
pairs, stops, the crop and the colours are held fixed.

  * Projection: `project_q` restates SO.project_gaussians behind its cov3d as differentiable torch (any dtype) -> q [N,6] =
    (u, v, conic a, b, c, compensation).  The fov clamp and the compensation's max(0, .) take the fp32 oracle's decisions
    (`projection_pins`).  `tangents_ref` is its Jacobian with respect to V by 12 torch.func.jvp calls.
  * Blend: `blend` runs the forward-mode recurrences on the schedule of SO.rasterize_f64 in float64 (or float32: the yardstick),
    with the kernel's fp32 thresholds.
  * Whole frame: `frame_reference` composes the two and maps dV to dc2w by autograd through `viewmat_t`.

Cases free of coin-flip decisions, as tests/raster_cases.py builds them: SO.rasterize_f64 names the grazing splats, `blend` adds
those with alpha on its 0.999 clamp (|o e^-sigma / 0.999 - 1| < 1e-3), their opacity is set to 0, and this repeats; at most
MAX_ZEROED of the splats in at most MAX_ROUNDS rounds, no placed splat.  Pixels with a channel on the colour clamp
(|pix_c + T bg_c - 1| < 1e-5) are left out, at most MAX_PIXELS_OUT of a case's.  Every other pixel is compared.

Tolerance: the error of a result is max |g - g64| / rms(g64) over the compared elements (`rel_error`); the yardstick is the error
of the same restatement run in float32, and a kernel is allowed KERNEL_FACTOR x that (tests/pose_grad_cases.py's figure and
reason: another summation order, errors of the same origin)."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import raster_cases as RC
from oracle import splat_oracle as SO

f32, f64 = np.float32, np.float64
B = 128                                   # lib.SPLAT_POSE_GRAD_BATCH (the CPU test asserts the two agree)
KERNEL_FACTOR = 4.0
MAX_ZEROED, MAX_ROUNDS = RC.MAX_ZEROED, RC.MAX_ROUNDS
MAX_PIXELS_OUT = 0.01
CLAMP_BAND, ONE_BAND = 1e-3, 1e-5
MUTATIONS = ("no_bg_dT", "no_alpha_dT", "clamp_grad", "diff_stopped")


# ---------------------------------------------------------------------------------------------------------------------
# pose -> view matrix -> projected quantities
# ---------------------------------------------------------------------------------------------------------------------
def viewmat_t(c2w: torch.Tensor) -> torch.Tensor:
    """SO.viewmat_from_c2w, differentiable: [3,4] -> V[:3,:4]"""
    F = torch.diag(torch.tensor([1.0, -1.0, -1.0], dtype=c2w.dtype))
    Rp = c2w[:3, :3] @ F
    return torch.cat([Rp.T, -Rp.T @ c2w[:3, 3:4]], dim=1)


def epilogue64(gV: np.ndarray, c2w, dtype=f64) -> np.ndarray:
    """ds/dV [..., 12] -> ds/dc2w [..., 3, 4] in `dtype` by the closed form: ds/dt = -R' g_t, ds/dR[a,b] = F_bb (G[b,a] - g_t[b] t[a])"""
    c2w = np.asarray(c2w, dtype)[:3, :4]
    g = np.asarray(gV, dtype).reshape(gV.shape[:-1] + (3, 4))
    G, gt = g[..., :3], g[..., 3]
    F = np.array([1.0, -1.0, -1.0], dtype)
    out = np.zeros_like(g)
    out[..., :3] = F * (np.swapaxes(G, -1, -2) - c2w[:, 3][:, None] * gt[..., None, :])
    out[..., 3] = -gt @ (c2w[:, :3] * F).T
    return out


def epilogue_autograd(gV: np.ndarray, c2w) -> np.ndarray:
    """the same map by autograd through viewmat_t (float64)"""
    c = torch.as_tensor(np.asarray(c2w, f64)[:3, :4])
    J = torch.autograd.functional.jacobian(lambda x: viewmat_t(x).reshape(-1), c).reshape(12, 12).numpy()   # [V entry, c2w entry]
    return (np.asarray(gV, f64) @ J).reshape(gV.shape[:-1] + (3, 4))


def projection_pins(means, V, fx, fy, H, W, proj) -> SimpleNamespace:
    """the fp32 oracle's branch decisions: live (radii > 0), fov clamp active in x / y (torch.clamp's derivative: 1 on the closed
    interval), compensation above 0"""
    means, V = np.asarray(means, f32), np.asarray(V, f32).reshape(-1)[:12].reshape(3, 4)
    p0, p1, p2 = means[:, 0], means[:, 1], means[:, 2]
    with np.errstate(all="ignore"):
        t = [((V[r, 0] * p0 + V[r, 1] * p1) + V[r, 2] * p2) + V[r, 3] for r in range(3)]
        lim_x, lim_y = f32(1.3) * (f32(0.5) * f32(W) / f32(fx)), f32(1.3) * (f32(0.5) * f32(H) / f32(fy))
        rx, ry = t[0] / t[2], t[1] / t[2]
    return SimpleNamespace(live=proj["radii"] > 0, clamp_x=(rx > lim_x) | (rx < -lim_x), clamp_y=(ry > lim_y) | (ry < -lim_y),
                           comp_live=proj["compensation"] > 0, lim_x=float(lim_x), lim_y=float(lim_y), tz=t[2], rx=rx, ry=ry)


def project_q(V: torch.Tensor, means: torch.Tensor, cov3d: torch.Tensor, pins, fx, fy, cx, cy) -> torch.Tensor:
    """SO.project_gaussians behind cov3d -> q [N,6] in V's dtype; dead splats (pins.live False) give zeros"""
    dt = V.dtype
    live = torch.as_tensor(pins.live)
    m, cv = means.to(dt), cov3d.to(dt)
    safe = lambda x, fill: torch.where(live, x, torch.full_like(x, fill))
    tx, ty, tz = (m @ V[r, :3] + V[r, 3] for r in range(3))
    tz = safe(tz, 1.0)
    cxm, cym = torch.as_tensor(pins.clamp_x), torch.as_tensor(pins.clamp_y)
    sx = torch.as_tensor(np.where(pins.rx > 0, pins.lim_x, -pins.lim_x)).to(dt)
    sy = torch.as_tensor(np.where(pins.ry > 0, pins.lim_y, -pins.lim_y)).to(dt)
    ex = torch.where(cxm, tz * sx, tz * (tx / tz))
    ey = torch.where(cym, tz * sy, tz * (ty / tz))
    rz = 1.0 / tz
    rz2 = rz * rz
    J00, J02, J11, J12 = fx * rz, (-fx * ex) * rz2, fy * rz, (-fy * ey) * rz2
    T0 = J00[:, None] * V[0, :3] + J02[:, None] * V[2, :3]
    T1 = J11[:, None] * V[1, :3] + J12[:, None] * V[2, :3]
    C3 = torch.stack([cv[:, 0], cv[:, 1], cv[:, 2], cv[:, 1], cv[:, 3], cv[:, 4], cv[:, 2], cv[:, 4], cv[:, 5]], -1).reshape(-1, 3, 3)
    TV0, TV1 = torch.einsum("nr,nrc->nc", T0, C3), torch.einsum("nr,nrc->nc", T1, C3)
    c00, c01, c11 = (TV0 * T0).sum(-1), (TV0 * T1).sum(-1), (TV1 * T1).sum(-1)
    det_orig = c00 * c11 - c01 * c01
    ca, cb, cc = c00 + 0.3, c01, c11 + 0.3
    det = safe(ca * cc - cb * cb, 1.0)
    cl = torch.as_tensor(pins.comp_live) & live
    ratio = torch.where(cl, det_orig / det, torch.ones_like(det))
    comp = torch.where(cl, torch.sqrt(ratio), torch.zeros_like(det))
    rw = 1.0 / (tz + 1e-6)
    q = torch.stack([(tx * rw) * fx + cx, (ty * rw) * fy + cy, cc / det, -cb / det, ca / det, comp], -1)
    return torch.where(live[:, None], q, torch.zeros_like(q))


def tangents_ref(V, means, cov3d, pins, fx, fy, cx, cy, dtype=torch.float64):
    """-> (q [N,6], dq/dV [N,6,12]) by 12 forward-mode passes, numpy arrays of `dtype`"""
    V = torch.as_tensor(np.asarray(V)).reshape(-1)[:12].reshape(3, 4).to(dtype)
    means, cov3d = torch.as_tensor(np.asarray(means)), torch.as_tensor(np.asarray(cov3d))
    fn = lambda v: project_q(v, means, cov3d, pins, fx, fy, cx, cy)
    cols = []
    for k in range(12):
        e = torch.zeros(12, dtype=dtype)
        e[k] = 1.0
        q, jq = torch.func.jvp(fn, (V,), (e.reshape(3, 4),))
        cols.append(jq)
    return q.numpy(), torch.stack(cols, -1).numpy()


# ---------------------------------------------------------------------------------------------------------------------
# the blend in forward mode
# ---------------------------------------------------------------------------------------------------------------------
def blend(gids, bins, xys, conics, colors, opac, tan, H, W, bg=None, comp=None, bw=16, dtype=f64, mutate=None, pins=None,
          record=False):
    """The recurrences of unerf_splat_pose_grad on the schedule of SO.rasterize_f64, every quantity in `dtype` on the fp32 inputs
    (thresholds: the kernel's fp32 constants).  tan [N,6,12] (None: forward only); comp [N] (antialiased) or None (classic).
    pins: a record of an earlier run -- its blend / clamp decisions are replayed (central differences of the pinned function).
    -> SimpleNamespace(gV [H,W,12], rgb [H,W,3], raw [H,W,3] (unclamped), T [H,W], clamp_grazing (splat ids), rec)"""
    dt = dtype
    xys, conics, colors = (np.asarray(a).astype(dt) for a in (xys, conics, colors))
    opac = np.asarray(opac).reshape(-1).astype(dt)
    bgv = np.zeros(3, dt) if bg is None else np.asarray(bg).astype(dt)
    tanv = None if tan is None else np.asarray(tan).astype(dt).reshape(len(opac), 6, 12)
    invc = None if comp is None else (1.0 / np.maximum(np.asarray(comp).astype(dt), dt(1e-30)))
    a_max, a_min, t_min = dt(f32(0.999)), dt(f32(1.0) / f32(255.0)), dt(f32(1e-4))
    tbx, tby = (W + bw - 1) // bw, (H + bw - 1) // bw
    gV, raw_img, Tim = np.zeros((H, W, 12), dt), np.zeros((H, W, 3), dt), np.ones((H, W), dt)
    grazing, rec = set(), {}
    half = dt(0.5)
    for ty in range(tby):
        for tx in range(tbx):
            r0, r1 = bins[ty * tbx + tx]
            ys, xs = np.arange(ty * bw, min((ty + 1) * bw, H)), np.arange(tx * bw, min((tx + 1) * bw, W))
            win = (slice(ys[0], ys[-1] + 1), slice(xs[0], xs[-1] + 1))
            py, px = np.meshgrid(ys.astype(dt) + half, xs.astype(dt) + half, indexing="ij")
            T, pix = np.ones(py.shape, dt), np.zeros(py.shape + (3,), dt)
            dT, dpix = np.zeros(py.shape + (12,), dt), np.zeros(py.shape + (3, 12), dt)
            done = np.zeros(py.shape, bool)
            for idx in range(r0, r1):
                if pins is None and done.all():
                    break
                g = gids[idx]
                dx, dy = xys[g, 0] - px, xys[g, 1] - py
                ca, cb, cc = conics[g]
                sigma = half * (ca * dx * dx + cc * dy * dy) + cb * dx * dy
                with np.errstate(over="ignore", invalid="ignore"):
                    raw = opac[g] * np.exp(-sigma)
                if pins is None:
                    alpha = np.minimum(a_max, raw)
                    clamped = raw > a_max
                    act = ~done & ~((sigma < 0) | (alpha < a_min))
                    nT = T * (1 - alpha)
                    stop = act & (nT <= t_min)
                    done |= stop
                    act &= ~stop
                    with np.errstate(invalid="ignore"):
                        if ((np.abs(raw / a_max - 1) < CLAMP_BAND) & (act | stop)).any():
                            grazing.add(int(g))
                    if record:
                        rec[idx] = (act.copy(), clamped.copy())
                else:
                    if idx not in pins:
                        continue
                    act, clamped = pins[idx]
                    stop = np.zeros_like(act)
                    alpha = np.where(clamped, a_max, raw)
                    nT = T * (1 - alpha)
                upd = act | stop if mutate == "diff_stopped" else act
                if tanv is not None and upd.any():
                    tq = tanv[g]
                    sd = ((ca * dx + cb * dy)[..., None] * tq[0] + (cc * dy + cb * dx)[..., None] * tq[1]
                          + (half * dx * dx)[..., None] * tq[2] + (dx * dy)[..., None] * tq[3] + (half * dy * dy)[..., None] * tq[4])
                    ad = -alpha[..., None] * sd
                    if invc is not None:
                        ad = ad + (alpha * invc[g])[..., None] * tq[5]
                    if mutate != "clamp_grad":
                        ad = np.where(clamped[..., None], 0, ad)
                    wk = ad * T[..., None]
                    if mutate != "no_alpha_dT":
                        wk = wk + alpha[..., None] * dT
                    dpix[upd] += (colors[g][:, None] * wk[:, :, None, :])[upd]
                    dT[upd] = (dT * (1 - alpha)[..., None] - T[..., None] * ad)[upd]
                pix[act] += colors[g][None, :] * (alpha * T)[act][:, None]
                T[act] = nT[act]
            val = pix + T[..., None] * bgv
            livec = (val < 1).astype(dt)
            tot = dpix if mutate == "no_bg_dT" else dpix + bgv[:, None] * dT[..., None, :]
            gV[win] = (livec[..., None] * tot).sum(-2) / dt(3)
            raw_img[win], Tim[win] = val, T
    return SimpleNamespace(gV=gV, rgb=np.minimum(raw_img, dt(1)), raw=raw_img, T=Tim, clamp_grazing=np.array(sorted(grazing), np.int64),
                           rec=rec)


def rel_error(g, g64, keep) -> float:
    """max |g - g64| over the kept pixels / rms(g64 over the kept pixels)"""
    g, g64 = np.asarray(g, f64)[keep], np.asarray(g64, f64)[keep]
    return float(np.abs(g - g64).max() / np.sqrt((g64 ** 2).mean()))


def keep_mask(raw64) -> np.ndarray:
    """pixels with no channel on the colour clamp"""
    return ~(np.abs(raw64 - 1.0) < ONE_BAND).any(-1)


# ---------------------------------------------------------------------------------------------------------------------
# walk cases: hand-built lists with random tangents
# ---------------------------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 2, B - 1, B, B + 1, 2 * B, 2 * B + 1, 3, 346, 64, 65)        # row-major over the 3 x 4 tiles of a 41 x 57 image
LONG = {B - 1: 3, B: 4, B + 1: 5, 2 * B: 6, 2 * B + 1: 7, 346: 9}
# raster_cases.STOP_PAIRS rescaled to B: the stop on the last entry of a batch, the first of the next, either side, the list's last
STOP_PAIRS = {B - 1: (B - 3, B - 2), B: (B - 2, B - 1), B + 1: (B - 1, B), 2 * B: (B, B + 1), 2 * B + 1: (2 * B - 2, 2 * B), 346: (150, 345)}
TAN_SCALE = np.array([1.0, 1.0, 0.1, 0.1, 0.1, 0.3])
# seed of each case's crowd: the first of 0, 1, 2, ... that meets the builder's caps (a choice made on the reference alone)
SEEDS = {"lists": 0, "stops": 0, "bright": 0, "quad": 0, "bw8": 0}


def _finish(c, protected=()):
    rng = np.random.default_rng([SEEDS[c.name], 91])
    c.N = len(c.opac)
    lo, hi = c.color_range
    c.colors = (lo + (hi - lo) * rng.random((c.N, 3))).astype(f32)
    c.tan = (rng.standard_normal((c.N, 6, 12)) * TAN_SCALE[:, None]).astype(f32)
    c.comp = rng.uniform(0.5, 1.0, c.N).astype(f32)
    c.bg = np.array([0.3, 0.55, 0.8], f32)
    c.c2w = np.array([[0.8, -0.36, 0.48, 0.5], [0.6, 0.48, -0.64, -1.25], [0.0, 0.8, 0.6, 2.0]], f32)
    c.protected = np.asarray(sorted(protected), np.int64)
    zeroed = []
    for c.rounds in range(MAX_ROUNDS + 1):
        graze = SO.rasterize_f64(c.gids, c.bins, c.xys, c.conics, c.colors, c.opac, c.H, c.W, bw=c.bw)[4]
        graze = np.union1d(graze, blend(c.gids, c.bins, c.xys, c.conics, c.colors, c.opac, None, c.H, c.W, bw=c.bw).clamp_grazing)
        if len(graze) == 0:
            break
        assert c.rounds < MAX_ROUNDS, f"{c.name}: splats still graze after {MAX_ROUNDS} rounds: {graze}"
        assert not np.isin(graze, c.protected).any(), f"{c.name}: a placed splat grazes: {np.intersect1d(graze, c.protected)}"
        c.opac[graze] = 0
        zeroed += list(graze)
    c.zeroed = np.asarray(zeroed, np.int64)
    assert len(c.zeroed) <= MAX_ZEROED * c.N, f"{c.name}: {len(c.zeroed)} of {c.N} splats zeroed"
    for a in vars(c).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def _new(name, c, color_range):
    return SimpleNamespace(name=name, H=c.H, W=c.W, bw=c.bw, lengths=c.lengths, gids=np.array(c.gids), bins=np.array(c.bins),
                           xys=np.array(c.xys), conics=np.array(c.conics), opac=np.array(c.opac), color_range=color_range)


def _crowd(name, H, W, bw, lengths, n=900):
    rng = np.random.default_rng([H, W, bw, len(lengths), SEEDS[name], 5])
    home, xys, conics, opac = RC._crowd(rng, n, lengths, H, W, bw)
    gids, bins = RC._lists(rng, home, lengths)
    return RC._new(name, H, W, bw, lengths, gids, bins, xys, conics, opac)


@functools.lru_cache(maxsize=None)
def case_lists():
    """list lengths around the staging batch, tiles that hang over the image's right and bottom edges; "dim" colours <= 0.6"""
    return _finish(_new("lists", _crowd("lists", 41, 57, 16, LENGTHS), (0.0, 0.6)))


@functools.lru_cache(maxsize=None)
def case_bright():
    """colours up to 2.5: many channels end above 1 and contribute exactly 0"""
    return _finish(_new("bright", _crowd("bright", 41, 57, 16, LENGTHS), (0.0, 2.5)))


@functools.lru_cache(maxsize=None)
def case_stops():
    """raster_cases.case_b rescaled to B: whole-tile stopper pairs at batch boundaries (their alpha sits on the 0.999 clamp:
    derivative 0), a quadrant-local pair of opacity 50 whose alpha leaves the clamp inside the quadrant"""
    c = _crowd("stops", 41, 57, 16, LENGTHS)
    c.opac = np.minimum(c.opac, f32(0.02))
    org = RC._origins(c.H, c.W, 16)
    xys, conics, opac, gids = list(c.xys), list(c.conics), list(c.opac), c.gids.copy()

    def place(tile, offset, xy, scale, op):
        gids[c.bins[tile, 0] + offset] = len(opac)
        xys.append(np.asarray(xy, f32)), conics.append(f32([1 / scale ** 2, 0, 1 / scale ** 2])), opac.append(op)

    for L, tile in LONG.items():
        for off in STOP_PAIRS[L]:
            place(tile, off, org[tile] + 8, 300.0, 2.0)
        for off in (10, 20):
            place(tile, off, org[tile] + 4, 1.6, 50.0)
    n0 = len(c.opac)
    c.gids, c.xys, c.conics, c.opac = gids, np.stack(xys), np.stack(conics), np.asarray(opac, f32)
    out = _finish(_new("stops", c, (0.1, 0.9)), protected=range(n0, len(opac)))
    out.n_placed = len(opac) - n0
    return out


@functools.lru_cache(maxsize=None)
def case_quad():
    """raster_cases.case_c's geometry: alpha = 1/255 contours that end on a quadrant border (wave-level culling)"""
    return _finish(_new("quad", RC.case_c(), (0.25, 1.0)))


@functools.lru_cache(maxsize=None)
def case_bw8():
    """19 x 21 with block_width 8: 3 x 3 tiles, the row-major thread-to-pixel mapping"""
    return _finish(_new("bw8", _crowd("bw8", 19, 21, 8, tuple((0, 1, B + 1)[t % 3] for t in range(9))), (0.0, 1.2)))


WALK = {"lists": case_lists, "bright": case_bright, "stops": case_stops, "quad": case_quad, "bw8": case_bw8}


@functools.lru_cache(maxsize=None)
def walk_ref(name, aa: bool, bg: str):
    """bg: "none" | "black" | "color" -> (float64 run, float32 run, keep [H,W]) of a walk case"""
    c = WALK[name]()
    bgv = {"none": None, "black": np.zeros(3, f32), "color": c.bg}[bg]
    a = (c.gids, c.bins, c.xys, c.conics, c.colors, c.opac, c.tan, c.H, c.W)
    r64 = blend(*a, bg=bgv, comp=c.comp if aa else None, bw=c.bw)
    r32 = blend(*a, bg=bgv, comp=c.comp if aa else None, bw=c.bw, dtype=f32)
    return r64, r32, keep_mask(r64.raw)


# ---------------------------------------------------------------------------------------------------------------------
# tangent case: planted projections
# ---------------------------------------------------------------------------------------------------------------------
TAN_CAM = dict(fx=32.0, fy=32.0, cx=24.0, cy=20.0, H=40, W=48)          # dyadic: lim = 1.3 * 0.75 / 1.3 * 0.625, exact products
TAN_CLIP = 0.25


@functools.lru_cache(maxsize=None)
def tangent_case():
    """N = 301 splats (N % 256 != 0) in front of an axis-aligned camera at the origin (V = [I | 0] with dyadic entries: t = mean
    exactly), with plants: tz on and either side of the clip threshold, tx / tz (ty / tz) on and either side of both fov limits,
    a needle with det_orig ~ 0 and a degenerate splat with det_orig <= 0 (zero covariance), a splat behind the camera, a splat
    whose tile box is empty (far outside the image)."""
    rng = np.random.default_rng(11)
    N = 301
    cam = TAN_CAM
    means = np.stack([rng.uniform(-1.5, 1.5, N), rng.uniform(-1.2, 1.2, N), rng.uniform(1.0, 4.0, N)], 1).astype(f32)
    scales = rng.uniform(0.02, 0.3, (N, 3)).astype(f32)
    quats = rng.standard_normal((N, 4)).astype(f32)
    quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    lim_x, lim_y = float(f32(1.3) * (f32(0.5) * f32(cam["W"]) / f32(cam["fx"]))), float(f32(1.3) * (f32(0.5) * f32(cam["H"]) / f32(cam["fy"])))
    plants = {}
    k = 0

    def plant(name, mean, scale=None, quat=None):
        nonlocal k
        means[k] = mean
        if scale is not None:
            scales[k] = scale
        if quat is not None:
            quats[k] = quat
        plants[name] = k
        k += 1

    up, dn = lambda v: np.nextafter(f32(v), f32(np.inf)), lambda v: np.nextafter(f32(v), f32(-np.inf))
    for nm, tz in (("clip_on", f32(TAN_CLIP)), ("clip_above", up(TAN_CLIP)), ("clip_below", dn(TAN_CLIP))):
        plant(nm, (0.01, 0.01, tz), scale=(0.01, 0.01, 0.01))
    for sgn, sn in ((1.0, "p"), (-1.0, "m")):
        for nm, r in (("on", f32(lim_x)), ("in", dn(lim_x)), ("out", up(lim_x))):
            plant(f"fovx_{sn}_{nm}", (sgn * float(r) * 2.0, 0.25, 2.0), scale=(0.3, 0.25, 0.2))   # tz = 2: tx / tz = r exactly
        for nm, r in (("on", f32(lim_y)), ("in", dn(lim_y)), ("out", up(lim_y))):
            plant(f"fovy_{sn}_{nm}", (0.25, sgn * float(r) * 2.0, 2.0), scale=(0.3, 0.25, 0.2))
    plant("needle", (0.2, -0.1, 2.0), scale=(0.5, 1e-6, 1e-6), quat=(1, 0, 0, 0))
    plant("flat", (0.1, 0.1, 2.0), scale=(0.0, 0.0, 0.0), quat=(1, 0, 0, 0))
    plant("behind", (0.1, 0.1, -1.0))
    plant("offscreen", (40.0, 0.3, 2.0), scale=(0.01, 0.01, 0.01))
    V = np.eye(4, dtype=f32)[:3]
    pr = SO.project_gaussians(means, scales, 1.0, quats, V, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["H"], cam["W"], 16, TAN_CLIP)
    pins = projection_pins(means, V, cam["fx"], cam["fy"], cam["H"], cam["W"], pr)
    return SimpleNamespace(N=N, means=means, scales=scales, quats=quats, V=V, proj=pr, pins=pins, plants=plants, cam=cam,
                           lim_x=lim_x, lim_y=lim_y)


# ---------------------------------------------------------------------------------------------------------------------
# whole frames
# ---------------------------------------------------------------------------------------------------------------------
FRAME_CAM = dict(fx=42.0, fy=40.0, cx=23.7, cy=20.3, H=40, W=48)
FRAME_BG = np.array([0.1490, 0.1647, 0.2157], f32)
# The central-difference scene.  A step h of a c2w entry moves a splat by about h z / s of its own width (depth z, world size s),
# whatever the focal length, and the truncation of a central difference goes with the square of that: splats three times as wide
# in the world, seen through a third of the focal length (the same ~1 px footprint, so as few grazing pairs), on a smaller image
FD_CAM = dict(fx=14.0, fy=13.3, cx=11.7, cy=10.3, H=20, W=24)
FD_LOG_SCALE, FD_N = -1.6, 60
FD_SEED = 11     # of the first twelve, the one whose four frames need the fewest zeroed splats (1, 0, 0, 0)


def frame_params(seed=3, N=400, log_scale=-2.7):
    """a synthetic splat set in front of the frame camera: splats of about a pixel (sigma) in a 2 x 2 x 1.5 box"""
    g = np.random.default_rng(seed)
    q = g.standard_normal((N, 4))
    return {"means": (g.uniform(-1, 1, (N, 3)) * np.array([1.0, 1.0, 0.75])).astype(f32),
            "scales": (g.standard_normal((N, 3)) * 0.3 + log_scale).astype(f32),
            "quats": (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32),
            "opacities": (g.standard_normal((N, 1)) * 1.5).astype(f32),
            "features_dc": (g.standard_normal((N, 3)) * 0.5).astype(f32),
            "features_rest": (g.standard_normal((N, 15, 3)) * 0.05).astype(f32),
            "log_uncertainties": g.random((N, 1)).astype(f32)}


def frame_c2w(sheared=False):
    """a camera 3 units from the origin looking at it; sheared: a non-orthogonal R (the transposition is differentiated, not
    an inverse)"""
    th = 0.4
    eye = np.array([3 * np.cos(th), 3 * np.sin(th), 0.6])
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(fwd, [0, 0, 1.0])
    right /= np.linalg.norm(right)
    c2w = np.stack([right, np.cross(right, fwd), -fwd, eye], 1)
    if sheared:
        c2w[:, :3] = c2w[:, :3] @ np.array([[1.0, 0.07, 0.0], [0.0, 1.04, -0.05], [0.03, 0.0, 0.97]])
    return c2w.astype(f32)


@functools.lru_cache(maxsize=None)
def frame_case(mode="classic", sh0=False, crop=False, sheared=False, seed=3, fd=False):
    """(seed: of the first ten, the one whose six frames need the fewest zeroed splats -- 4 .. 9 of 400; a choice made on the
    reference alone) -> the fp32 oracle's frame inputs with the grazing splats' opacities zeroed (opacity logit -> -100) under the caps"""
    gp = frame_params(seed, FD_N, FD_LOG_SCALE) if fd else frame_params(seed)
    cam = FD_CAM if fd else FRAME_CAM
    c2w = frame_c2w(sheared)
    crop_ids = (gp["means"][:, 0] < 0.4) if crop else None
    zeroed, N = [], len(gp["means"])
    for rounds in range(MAX_ROUNDS + 1):
        o = SO.active_splatfacto_outputs(gp, c2w, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["H"], cam["W"], FRAME_BG,
                                         sh_degree=3, rasterize_mode=mode, config_sh_degree=0 if sh0 else 3, crop_ids=crop_ids)
        f = frame_inputs(gp, c2w, mode, sh0, crop_ids, o)
        f.cam = cam
        graze = SO.rasterize_f64(f.gids, f.bins, f.xys, f.conics, f.colors, f.opac, cam["H"], cam["W"], FRAME_BG)[4]
        graze = np.union1d(graze, blend(f.gids, f.bins, f.xys, f.conics, f.colors, f.opac, None, cam["H"], cam["W"], bg=FRAME_BG).clamp_grazing)
        if len(graze) == 0:
            break
        assert rounds < MAX_ROUNDS, f"frame: splats still graze after {MAX_ROUNDS} rounds"
        sel = f.index[graze]
        gp["opacities"][sel] = -100.0
        zeroed += list(sel)
    assert len(zeroed) <= MAX_ZEROED * N, f"frame: {len(zeroed)} of {N} splats zeroed"
    f.gp, f.c2w, f.cam, f.mode, f.sh0, f.crop_ids, f.zeroed, f.rounds = gp, c2w, cam, mode, sh0, crop_ids, zeroed, rounds
    return f


def frame_inputs(gp, c2w, mode, sh0, crop_ids, o):
    """what the rasteriser sees, from the fp32 oracle's frame `o`: lists, projected quantities, colours, opacities (of the
    cropped set; index: their rows in the full set)"""
    sel = np.arange(len(gp["means"])) if crop_ids is None else np.nonzero(crop_ids)[0]
    sub = {k: v[sel] for k, v in gp.items()}
    pr = o["_proj"]
    coeffs = np.concatenate([sub["features_dc"][:, None, :], sub["features_rest"]], axis=1)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(f32)))
    if sh0:
        rgbs = torch.sigmoid(tt(coeffs)[:, 0, :]).numpy()
    else:
        rgbs = np.maximum(SO.spherical_harmonics(3, sub["means"] - c2w[:3, 3], coeffs) + f32(0.5), f32(0))
    opac = torch.sigmoid(tt(sub["opacities"])).numpy().reshape(-1)
    if mode == "antialiased":
        opac = opac * pr["compensation"]
    _, _, _, gids, bins = o["_sort"]
    return SimpleNamespace(index=sel, means=sub["means"], proj=pr, gids=gids, bins=bins, xys=pr["xys"], conics=pr["conics"],
                           colors=rgbs.astype(f32), opac=opac.astype(f32), comp=pr["compensation"] if mode == "antialiased" else None)


def shape64(sub) -> np.ndarray:
    """cov3d [N,6] in float64 from the stored parameters: exp(scales), quats / |quats| (activesplatfacto_model.py:221-223) and
    gsplat's scale_rot_to_cov3d"""
    q = sub["quats"].astype(f64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                  2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    M = R * np.exp(sub["scales"].astype(f64))[:, None, :]
    Sg = M @ np.swapaxes(M, 1, 2)
    return np.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], -1)


def colors64(sub, c2w, sh0) -> np.ndarray:
    """the splats' colours in float64: sigmoid(features_dc) (:247-248) or max(SH_3(means - camera position) + 0.5, 0)"""
    dc, rest = sub["features_dc"].astype(f64), sub["features_rest"].astype(f64)
    if sh0:
        return 1.0 / (1.0 + np.exp(-dc))
    k = np.concatenate([dc[:, None, :], rest], axis=1)
    v = sub["means"].astype(f64) - np.asarray(c2w, f64)[:3, 3]
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    x, y, z = v[:, 0:1], v[:, 1:2], v[:, 2:3]
    xx, xy, xz, yy, yz, zz = x * x, x * y, x * z, y * y, y * z, z * z
    C2, C3 = SO.SH_C2, SO.SH_C3
    col = SO.SH_C0 * k[:, 0] + SO.SH_C1 * (-y * k[:, 1] + z * k[:, 2] - x * k[:, 3])
    col = col + (C2[0] * xy * k[:, 4] + C2[1] * yz * k[:, 5] + C2[2] * (2 * zz - xx - yy) * k[:, 6] + C2[3] * xz * k[:, 7]
                 + C2[4] * (xx - yy) * k[:, 8])
    col = col + (C3[0] * y * (3 * xx - yy) * k[:, 9] + C3[1] * xy * z * k[:, 10] + C3[2] * y * (4 * zz - xx - yy) * k[:, 11]
                 + C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * k[:, 12] + C3[4] * x * (4 * zz - xx - yy) * k[:, 13]
                 + C3[5] * z * (xx - yy) * k[:, 14] + C3[6] * x * (xx - 3 * yy) * k[:, 15])
    return np.maximum(col + 0.5, 0.0)


def frame_reference(f, dtype=f64):
    """-> SimpleNamespace(grad [H,W,3,4], rgb, raw, keep, gV): tangents_ref and blend composed, then dV -> dc2w.
    float64: the frame as a function of the STORED parameters -- activations (exp, normalisation, sigmoid, SH), projection and
    blend in float64, lists and branch decisions the fp32 oracle's, dV -> dc2w by autograd.
    float32 (the yardstick): the fp32 oracle's own activations, projection and colours, the Jacobian by float32 forward mode, the
    blend and the closed-form epilogue in float32."""
    cam = f.cam
    V = SO.viewmat_from_c2w(f.c2w)[:3]
    pins = projection_pins(f.means, V, cam["fx"], cam["fy"], cam["H"], cam["W"], f.proj)
    a = (pins, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    if dtype == f64:
        sub = {k: v[f.index] for k, v in f.gp.items()}
        q, J = tangents_ref(V, f.means, shape64(sub), *a)
        opac = 1.0 / (1.0 + np.exp(-sub["opacities"].astype(f64).reshape(-1)))
        comp = q[:, 5] if f.comp is not None else None
        r = blend(f.gids, f.bins, q[:, :2], q[:, 2:5], colors64(sub, f.c2w, f.sh0), opac if comp is None else opac * comp, J,
                  cam["H"], cam["W"], bg=FRAME_BG, comp=comp)
        grad = epilogue_autograd(r.gV, f.c2w)
    else:
        _, J = tangents_ref(V, f.means, f.proj["cov3d"], *a, torch.float32)
        r = blend(f.gids, f.bins, f.xys, f.conics, f.colors, f.opac, J, cam["H"], cam["W"], bg=FRAME_BG, comp=f.comp, dtype=f32)
        grad = epilogue64(r.gV, f.c2w, f32)
    return SimpleNamespace(grad=grad, rgb=r.rgb, raw=r.raw, keep=keep_mask(r.raw.astype(f64)), gV=r.gV)


# ---------------------------------------------------------------------------------------------------------------------
# the pure-float64 frame as a function of c2w (self-check by central differences)
# ---------------------------------------------------------------------------------------------------------------------
def frame64(f, c2w64: np.ndarray, pins_proj, rec=None, want_grad=False):
    """s [H,W] (and ds/dc2w) of the float64 frame at pose c2w64 with lists, cull / clamp decisions (pins_proj) and, given `rec`,
    the blend's per-pair decisions pinned.  Forward values are float64 throughout (the opacity carries the float64 compensation)."""
    cam = f.cam
    V = viewmat_t(torch.as_tensor(np.asarray(c2w64, f64)[:3, :4]))
    a = (f.means, f.proj["cov3d"], pins_proj, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    if want_grad:
        q, J = tangents_ref(V.numpy(), *a)
    else:
        q, J = project_q(V, torch.as_tensor(f.means), torch.as_tensor(f.proj["cov3d"]), *a[2:]).numpy(), None
    opac = f.opac.astype(f64)
    comp = None
    if f.comp is not None:
        comp = q[:, 5]
        with np.errstate(all="ignore"):
            base = np.where(f.comp > 0, f.opac.astype(f64) / f.comp.astype(f64), 0.0)
        opac = base * comp
    r = blend(f.gids, f.bins, q[:, :2], q[:, 2:5], f.colors, opac, J, cam["H"], cam["W"], bg=FRAME_BG, comp=comp, pins=rec,
              record=rec is None)
    return SimpleNamespace(s=r.rgb.mean(-1), raw=r.raw, rec=r.rec, grad=epilogue_autograd(r.gV, c2w64) if want_grad else None)
