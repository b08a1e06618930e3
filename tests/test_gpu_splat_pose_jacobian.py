"""The splat pose Jacobian on the GPU, part by part, against the float64 references of tests/splat_pose_jac_cases.py:

  1. splat_pose_tangents_proj_kernel on the planted projections of SPG.tangent_case (N = 1, 257, 301; P = 1, 5, 6, 7, 12): the
     identity bit for bit, a random projection inside the forward bound, dead rows, padding columns and guard floats;
  2. splat_pose_jac_kernel on SPG's hand-built lists x classic / antialiased x background none / given, P = 6 and P = 12: every
     row of every channel, the values, the variance; culling, repetition, channel and output subsets, widths, streams, guards;
  3. refusals; 4. whole frames through the models.

A row set's error is max |g - g64| / rms(g64) per channel over the compared pixels; the kernel is allowed KERNEL_FACTOR = 4 x the
error of the same restatement run in float32.  Every test prints its ratios (DESIGN.md 4.6b records them)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import splat_pose_grad_cases as SPG
import splat_pose_jac_cases as JC

pytestmark = pytest.mark.gpu
GUARD = 77.25
f64 = np.float64


def _t(dev, a):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the contraction kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 257, 301])
def test_contraction_kernel(dev, lib, N):
    from uncertainty_nerf_gs_amd import ops
    tc = SPG.tangent_case()
    cam = tc.cam
    assert N <= tc.N
    means, cov3d, radii = _t(dev, tc.means[:N]), _t(dev, tc.proj["cov3d"][:N]), _t(dev, tc.proj["radii"][:N])
    live = tc.proj["radii"][:N] > 0
    rng = np.random.default_rng(N)
    with torch.cuda.device(dev):
        tan = ops.splat_pose_tangents(means, cov3d, radii, torch.from_numpy(tc.V), cam["fx"], cam["fy"], cam["cx"], cam["cy"],
                                      cam["H"], cam["W"], clip_thresh=SPG.TAN_CLIP)
        tan_h = tan.cpu().numpy()
        assert np.isfinite(tan_h).all() and (N == 1 or np.abs(tan_h).max() > 0)
        for P in (1, 5, 6, 7, 12):
            PW = lib.splat_pose_pw(P)
            n = N * 7 * PW
            buf = torch.full((n + 64,), GUARD, device=dev)
            eye = torch.eye(12)[:, :P]
            got = ops.splat_pose_tangents_proj(tan, means, radii, eye, out=buf[:n].view(N, 7, PW))
            torch.cuda.synchronize()
            assert (buf[n:] == GUARD).all(), "floats behind the array were written"
            assert got.shape == (N, 7, PW) and (got[..., P:] == 0).all(), "padding columns must be exactly 0"
            assert torch.equal(got[:, :6, :P], tan[..., :P]), f"P={P}: the identity must return the tangents' bits"
            zrow = np.concatenate([np.zeros((N, 8), np.float32), tc.means[:N], np.ones((N, 1), np.float32)], 1)[:, :P]
            zrow[~live] = 0
            assert np.array_equal(got[:, 6, :P].cpu().numpy(), zrow), f"P={P}: the depth row of the identity is (0 x 8, m, 1)"
            assert (got.cpu().numpy()[~live] == 0).all(), "dead splats must be exactly 0"
            M = rng.standard_normal((12, P)).astype(np.float32)
            got = ops.splat_pose_tangents_proj(tan, means, radii, torch.from_numpy(M))
            again = ops.splat_pose_tangents_proj(tan, means, radii, torch.from_numpy(M))
            assert torch.equal(got, again), "two calls must return the same bits"
            g = got.cpu().numpy()
            assert (g[..., P:] == 0).all() and (g[~live] == 0).all()
            want, bound = JC.contract(tan_h, tc.means[:N], live, M), JC.contract_bound(tan_h, tc.means[:N], live, M)
            excess = np.abs(g[..., :P] - want) - bound
            print(f"CONTRACT N={N} P={P}: worst |error| / bound = {np.max(np.abs(g[..., :P] - want) / np.where(bound > 0, bound, 1.0)):.2f}")
            assert (excess <= 0).all(), f"P={P}: outside 13 x 2^-24 x sum |t p|"


# ---------------------------------------------------------------------------------------------------------------------
# 2. the walk kernel
# ---------------------------------------------------------------------------------------------------------------------
_DEV = {}


def _walk_tensors(dev, name):
    if name not in _DEV:
        c, w = SPG.WALK[name](), JC.walk_inputs(name)
        t = {k: _t(dev, getattr(c, k)) for k in ("gids", "bins", "xys", "conics", "opac", "colors", "tan", "comp", "bg")}
        t["z"], t["ptan12"] = _t(dev, w.z), _t(dev, w.ptan)
        t["ptan6"] = t["ptan12"][..., :6].contiguous()
        _DEV[name] = t
    return _DEV[name]


def _walk(dev, name, aa, bg, P=12, ptan=None, **kw):
    from uncertainty_nerf_gs_amd import ops
    c, t = SPG.WALK[name](), _walk_tensors(dev, name)
    bgt = {"none": None, "color": t["bg"]}[bg]
    ptan = t["ptan6" if P <= 6 else "ptan12"] if ptan is None else ptan
    kw.setdefault("want", ("proj", "var", "val"))
    return ops.splat_pose_jacobian(t["gids"], t["bins"], t["xys"], t["conics"], t["colors"], t["z"], t["opac"], ptan, P, c.H, c.W,
                                   bgt, compensation=t["comp"] if aa else None, block_width=c.bw, **kw)


def _same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


@pytest.mark.parametrize("bg", ["none", "color"])
@pytest.mark.parametrize("aa", [False, True], ids=["classic", "antialiased"])
@pytest.mark.parametrize("name", list(SPG.WALK))
def test_walk_matches_f64(dev, name, aa, bg):
    from uncertainty_nerf_gs_amd import ops
    c, t = SPG.WALK[name](), _walk_tensors(dev, name)
    r64, r32, keep = JC.walk_ref(name, aa, bg)
    with torch.cuda.device(dev):
        o12, o6 = _walk(dev, name, aa, bg), _walk(dev, name, aa, bg, P=6)
        _same(o12, _walk(dev, name, aa, bg, cull=False), "culled and unculled walks")
        _same(o12, _walk(dev, name, aa, bg), "two calls")
        _same(o6, _walk(dev, name, aa, bg, P=6, cull=False), "culled and unculled walks, P = 6")
        _, rgb, fT = ops.splat_pose_grad(t["gids"], t["bins"], t["xys"], t["conics"], t["colors"], t["opac"], t["tan"], c.H, c.W,
                                         None if bg == "none" else t["bg"], compensation=t["comp"] if aa else None,
                                         block_width=c.bw, want_rgb=True, want_final_T=True)
        torch.cuda.synchronize()
    assert o12["proj"].shape == (c.H, c.W, 5, 12) and o6["proj"].shape == (c.H, c.W, 5, 6) and o12["val"].shape == (c.H, c.W, 5)
    assert torch.equal(o12["proj"][..., :6], o6["proj"]), "the P = 6 and P = 12 instantiations must agree bit for bit"
    assert torch.equal(o12["val"], o6["val"])
    what = f"{name} {'antialiased' if aa else 'classic'} bg={bg}"
    rows, val = o12["proj"].cpu().numpy(), o12["val"].cpu().numpy()
    assert JC.within(what, rows, r64.rows, r32.rows, keep), f"{what}: a channel's rows exceed {SPG.KERNEL_FACTOR} x the yardstick"
    if name == "stops":      # for the record: the same ratios against a float32 run with a correctly rounded exp (JC's docstring)
        plain = JC.channel_errors(JC.walk_ref_plain_exp(name, aa, bg).rows, r64.rows, keep)
        print(f"PLAIN-EXP {what}: " + " ".join(f"{e / p:.2f}" for e, p in zip(JC.channel_errors(rows, r64.rows, keep), plain)))
    # values: the colour and 1 - final_T are the gradient kernel's bits; the depth is held to the float64 blend
    assert torch.equal(o12["val"][..., :3], rgb) and torch.equal(o12["val"][..., 3], 1.0 - fT)
    assert JC.within(what + " value", val[..., 4:5], r64.val[..., 4:5], r32.val[..., 4:5], keep, channels=("expected_depth",))
    empty = val[..., 3] == 0
    assert np.array_equal(empty, r64.val[..., 3] == 0)
    assert (val[..., 4][empty] == 0).all() and (rows[..., 4, :][empty] == 0).all(), "A == 0: depth value and row exactly 0"
    if name == "bright":     # a saturated channel has a row of exact zeros
        sat = r64.raw > 1 + SPG.ONE_BAND
        assert sat.sum() > 0 and (rows[..., :3, :][sat] == 0).all()
    # the variance: the float64 sum of squares of the call's own rows, a forward bound of non-negative terms
    for o, P in ((o12, 12), (o6, 6)):
        ss = (o["proj"].cpu().numpy().astype(f64) ** 2).sum(-1)
        assert (np.abs(o["var"].cpu().numpy() - ss) <= (P + 1) * 2.0 ** -23 * ss).all(), f"{what}: out_var, P={P}"


@pytest.mark.parametrize("name,aa", [("lists", True), ("stops", False), ("bw8", True), ("bright", False)])
def test_identity_projection_averages_to_the_pose_gradient(dev, name, aa):
    from uncertainty_nerf_gs_amd import ops
    c, t = SPG.WALK[name](), _walk_tensors(dev, name)
    r64, r32, keep = SPG.walk_ref(name, aa, "color")
    with torch.cuda.device(dev):
        ptan = ops.splat_pose_tangents_proj(t["tan"], torch.zeros(c.N, 3, device=dev), torch.ones(c.N, device=dev, dtype=torch.int32),
                                            torch.eye(12))
        assert torch.equal(ptan[:, :6], t["tan"])
        out = _walk(dev, name, aa, "color", ptan=ptan, channels=("r", "g", "b"), want="proj")
        grad, _, _ = ops.splat_pose_grad(t["gids"], t["bins"], t["xys"], t["conics"], t["colors"], t["opac"], t["tan"], c.H, c.W,
                                         t["bg"], compensation=t["comp"] if aa else None, block_width=c.bw)
        torch.cuda.synchronize()
    mean = out["proj"].cpu().numpy().astype(f64).mean(-2)
    e32, err = SPG.rel_error(r32.gV, r64.gV, keep), SPG.rel_error(mean, grad.cpu().numpy(), keep)
    print(f"RATIO {name} mean of the colour rows against splat_pose_grad: {err:.3e} yardstick {e32:.3e} ratio {err / e32:.2f}")
    assert err <= SPG.KERNEL_FACTOR * e32


@pytest.mark.parametrize("name,aa", [("lists", True), ("bw8", False)])
def test_bit_properties(dev, lib, name, aa):
    c, t = SPG.WALK[name](), _walk_tensors(dev, name)
    n = c.H * c.W
    with torch.cuda.device(dev):
        full = _walk(dev, name, aa, "color")
        # a row's bits under every channel subset and every output subset
        order = {ch: k for k, ch in enumerate(JC.CHANNELS)}
        for chans in (("g",), ("expected_depth", "r"), ("accumulation",), ("b", "accumulation", "expected_depth"), ("r", "g", "b")):
            idx = sorted(order[ch] for ch in chans)
            for want in (("proj", "var", "val"), ("var",), ("proj",), ("val", "var")):
                got = _walk(dev, name, aa, "color", channels=chans, want=want)
                assert sorted(got) == sorted(want)
                for k in want:
                    assert torch.equal(got[k], full[k][:, :, idx]), f"channels={chans} want={want}: {k}"
        # widths: P = 1 is column 0, P = 5 the first five; P = 7 runs the 12-wide instantiation
        for P in (1, 5, 7):
            PW = lib.splat_pose_pw(P)
            ptan = torch.zeros(c.N, 7, PW, device=dev)
            ptan[..., :P] = t["ptan12"][..., :P]
            got = _walk(dev, name, aa, "color", P=P, ptan=ptan)
            assert got["proj"].shape == (c.H, c.W, 5, P) and torch.equal(got["proj"], full["proj"][..., :P]), f"P={P}"
            assert torch.equal(got["val"], full["val"])
            ss = (got["proj"].cpu().numpy().astype(f64) ** 2).sum(-1)
            assert (np.abs(got["var"].cpu().numpy() - ss) <= (P + 1) * 2.0 ** -23 * ss).all()
        # columns beyond P in ptangents are not read into the variance
        junk = t["ptan6"].clone()
        junk[..., 5] = 1e3
        got = _walk(dev, name, aa, "color", P=5, ptan=junk, want=("proj", "var"))
        assert torch.equal(got["proj"], full["proj"][..., :5])
        ss = (got["proj"].cpu().numpy().astype(f64) ** 2).sum(-1)
        assert (np.abs(got["var"].cpu().numpy() - ss) <= 6 * 2.0 ** -23 * ss).all()
        # dirty buffers with guard floats on both sides of all three outputs, on a side stream
        sizes = {"proj": n * 5 * 12, "var": n * 5, "val": n * 5}
        bufs = {k: torch.full((s + 128,), GUARD, device=dev) for k, s in sizes.items()}
        shapes = {"proj": (c.H, c.W, 5, 12), "var": (c.H, c.W, 5), "val": (c.H, c.W, 5)}
        outs = {k: bufs[k][64:64 + sizes[k]].view(shapes[k]) for k in sizes}
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            got = _walk(dev, name, aa, "color", out=outs)
        side.synchronize()
        _same(full, got, "dirty buffers on a side stream")
        for k, b in bufs.items():
            assert (b[:64] == GUARD).all() and (b[64 + sizes[k]:] == GUARD).all(), f"floats around out_{k} were written"


# ---------------------------------------------------------------------------------------------------------------------
# 3. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(dev, lib):
    c, t = SPG.case_bw8(), _walk_tensors(dev, "bw8")
    h = lib.load()
    n = c.H * c.W * 5
    with torch.cuda.device(dev):
        outs = [torch.full((n * s,), GUARD, device=dev) for s in (6, 1, 1)]
        good = dict(ids=t["gids"].data_ptr(), ptan=t["ptan6"].data_ptr(), P=6, bw=c.bw, flags=0, channels=31,
                    outs=tuple(o.data_ptr() for o in outs))

        def call(**kw):
            a = {**good, **kw}
            return h.unerf_splat_pose_jacobian(a["ids"], t["bins"].data_ptr(), t["xys"].data_ptr(), t["conics"].data_ptr(),
                                               t["colors"].data_ptr(), t["z"].data_ptr(), t["opac"].data_ptr(), None, a["ptan"],
                                               None, a["P"], c.H, c.W, a["bw"], a["flags"], a["channels"], *a["outs"], None)

        for text, kw in ((b"splat_pose_jacobian: null pointer", dict(ids=None)), (b"splat_pose_jacobian: null pointer", dict(ptan=None)),
                         (b"P=0 outside [1,12]", dict(P=0)), (b"P=13 outside [1,12]", dict(P=13)),
                         (b"channels is empty", dict(channels=0)), (b"unknown channel bits 64", dict(channels=64 + 3)),
                         (b"no output asked for", dict(outs=(None, None, None))), (b"unknown flags 4", dict(flags=4)),
                         (b"block_width=0 outside [1,16]", dict(bw=0)), (b"block_width=32 outside [1,16]", dict(bw=32)),
                         (b"ptangents must be 8-byte aligned for P=6", dict(ptan=t["ptan6"].data_ptr() + 4)),
                         (b"ptangents must be 16-byte aligned for P=12", dict(ptan=t["ptan6"].data_ptr() + 8, P=12))):
            assert call(**kw) == -1, text
            assert text in h.unerf_last_error(), h.unerf_last_error()
        torch.cuda.synchronize()
        for o in outs:
            assert (o == GUARD).all(), "a refused call wrote to an output"
        assert call() == 0          # the same arguments, unbroken, run
        torch.cuda.synchronize()
        assert not (outs[0] == GUARD).any()


# ---------------------------------------------------------------------------------------------------------------------
# 4. whole frames through the models
# ---------------------------------------------------------------------------------------------------------------------
class _Box:
    def within(self, pts):
        return (pts[:, 0] < 0.4)[:, None]


class _Nothing:
    def within(self, pts):
        return torch.zeros(pts.shape[0], 1, dtype=torch.bool, device=pts.device)


def _model(dev, f, active=True, through_plugin=False):
    from uncertainty_nerf_gs_amd import models, plugin
    if through_plugin:
        cfg = plugin.MODEL_CONFIGS["active-splatfacto" if active else "splatfacto"]()
    else:
        cfg = (models.ActiveSplatfactoModelConfig if active else models.SplatfactoModelConfig)()
    cfg.rasterize_mode = f.mode
    if f.sh0:
        cfg.sh_degree = 0
    m = cfg._target(cfg, num_points=4)
    m.load_state_dict({f"gauss_params.{k}": torch.from_numpy(v) for k, v in f.gp.items() if active or k != "log_uncertainties"})
    return m.to(dev).eval()


def _camera(f, c2w=None, **kw):
    cam = f.cam
    return SimpleNamespace(camera_to_worlds=torch.from_numpy(f.c2w if c2w is None else c2w)[None], fx=torch.tensor([cam["fx"]]),
                           fy=torch.tensor([cam["fy"]]), cx=torch.tensor([cam["cx"]]), cy=torch.tensor([cam["cy"]]),
                           height=cam["H"], width=cam["W"], **kw)


def _var_errors(var, ref, keep):
    """[H,W,C] variances -> per channel max |var - ref| / rms(ref) over the kept pixels"""
    return JC.channel_errors(var[..., None], ref[..., None], keep)


FRAMES = [(dict(mode="classic"), True, False), (dict(mode="antialiased"), True, False), (dict(mode="classic", sheared=True), True, False),
          (dict(mode="antialiased", crop=True), True, True), (dict(mode="classic", sh0=True), False, True)]
POSE_COVS = {"diagonal": np.array([0.02, 0.01, 0.03, 4e-3, 2e-3, 3e-3]),
             "full": (lambda a: a @ a.T * 1e-4)(np.random.default_rng(8).standard_normal((6, 6)))}


@pytest.mark.parametrize("kw,active,through_plugin", FRAMES,
                         ids=lambda v: "-".join(f"{a}={b}" for a, b in v.items()) if isinstance(v, dict) else str(v))
def test_frame_through_the_model(dev, kw, active, through_plugin):
    from uncertainty_nerf_gs_amd import posegrad
    f = SPG.frame_case(**kw)
    r64, r32 = JC.frame_jac_reference(f), JC.frame_jac_reference(f, np.float32)
    keep = r64.keep
    m = _model(dev, f, active, through_plugin)
    H, W = f.cam["H"], f.cam["W"]
    B = posegrad.tangent_basis(torch.from_numpy(f.c2w)).numpy()
    with torch.cuda.device(dev):
        frame = m.get_outputs_for_camera(_camera(f), obb_box=_Box() if kw.get("crop") else None)
        c2w = m.get_splat_pose_jacobians_for_camera(_camera(f), basis="c2w")
        se3 = m.get_splat_pose_jacobians_for_camera(_camera(f))
        _, rgb = m.get_pose_gradients_for_camera(_camera(f), want_rgb=True)
        unc = {k: m.get_splat_pose_uncertainty_for_camera(_camera(f), torch.from_numpy(v)) for k, v in POSE_COVS.items()}
        zero = m.get_splat_pose_uncertainty_for_camera(_camera(f), torch.zeros(6))
        torch.cuda.synchronize()
    what = "frame " + " ".join(f"{a}={b}" for a, b in kw.items())
    J = c2w["jacobian"]
    assert J.shape == (H, W, 5, 12) and J.dtype == torch.float32 and J.device.type == "cuda" and c2w["values"].shape == (H, W, 5)
    assert se3["jacobian"].shape == (H, W, 5, 6) and torch.equal(se3["values"], c2w["values"])
    Jh = J.cpu().numpy()
    assert JC.within(what + " d/dc2w", Jh, r64.rows, r32.rows, keep), what
    assert JC.within(what + " value", c2w["values"].cpu().numpy()[..., 3:], r64.val[..., 3:], r32.val[..., 3:], keep,
                     channels=JC.CHANNELS[3:])
    # the six-parameter call contracts per splat, before the walk: against the call's own c2w rows contracted afterwards
    # (two fp32 evaluations of one quantity in different summation orders; the yardstick: the float32 restatement's rows . B)
    e32 = JC.channel_errors(r32.rows.astype(f64) @ B, r64.rows @ B, keep)
    err = JC.channel_errors(se3["jacobian"].cpu().numpy(), Jh.astype(f64) @ B, keep)
    for k, ch in enumerate(JC.CHANNELS):
        print(f"RATIO {what} se3 {ch}: error {err[k]:.3e} yardstick {e32[k]:.3e} ratio {err[k] / e32[k]:.2f}")
    assert (e32 > 0).all() and (err <= SPG.KERNEL_FACTOR * e32).all()
    # the propagated covariance against J Sigma J^T in float64 from the call's own six-parameter Jacobian
    Js = se3["jacobian"].cpu().numpy().astype(f64)
    for name, cov in POSE_COVS.items():
        Sig = np.diag(cov ** 2) if cov.ndim == 1 else cov
        want = np.einsum("hwcp,pq,hwcq->hwc", Js, Sig, Js)
        L = posegrad.pose_projection(torch.from_numpy(f.c2w), torch.from_numpy(cov)).numpy()
        y64, y32 = ((r64.rows @ L) ** 2).sum(-1), ((r32.rows.astype(f64) @ L) ** 2).sum(-1)
        var = np.concatenate([unc[name]["rgb_var_pose"].cpu().numpy().astype(f64), unc[name]["accumulation_std_pose"].cpu().numpy().astype(f64) ** 2,
                              unc[name]["depth_std_pose"].cpu().numpy().astype(f64) ** 2], -1)
        ref = np.concatenate([want[..., :3].mean(-1, keepdims=True), want[..., 3:]], -1)
        yard = _var_errors(np.concatenate([y32[..., :3].mean(-1, keepdims=True), y32[..., 3:]], -1),
                           np.concatenate([y64[..., :3].mean(-1, keepdims=True), y64[..., 3:]], -1), keep)
        err = _var_errors(var, ref, keep)
        for k, ch in enumerate(("rgb", "accumulation", "depth")):
            print(f"RATIO {what} {name} covariance {ch}: error {err[k]:.3e} yardstick {yard[k]:.3e} ratio {err[k] / yard[k]:.2f}")
        assert (yard > 0).all() and (err <= SPG.KERNEL_FACTOR * yard).all()
        assert torch.equal(unc[name]["rgb_std_pose"], unc[name]["rgb_var_pose"].sqrt())
    for k in ("rgb_var_pose", "rgb_std_pose", "accumulation_std_pose", "depth_std_pose"):
        assert zero[k].shape == (H, W, 1) and float(zero[k].abs().max()) == 0.0, "a zero covariance gives exactly 0"
    u = unc["full"]
    assert torch.equal(u["rgb"], rgb), "the colour is the gradient kernel's, bit for bit"
    assert torch.equal(u["rgb"], c2w["values"][..., :3]) and torch.equal(u["accumulation"], c2w["values"][..., 3:4])
    # depth: the frame's where something was blended, its fill elsewhere
    hit = (u["accumulation"] > 0).cpu().numpy()[..., 0]
    assert np.array_equal(hit, frame["accumulation"].cpu().numpy()[..., 0] > 0) and 0 < hit.sum() < hit.size
    d, fd = u["depth"].cpu().numpy().astype(f64)[..., 0], frame["depth"].cpu().numpy().astype(f64)[..., 0]
    e32 = JC.channel_errors(r32.val[..., 4:5], r64.val[..., 4:5], keep)[0]
    err = np.abs(d - fd)[hit & keep].max() / np.sqrt((r64.val[..., 4][keep] ** 2).mean())
    print(f"RATIO {what} depth against the frame's: {err:.3e} yardstick {e32:.3e}")
    assert err <= SPG.KERNEL_FACTOR * e32
    fill = fd[~hit]
    assert (fill == fill[0]).all() and (np.abs(d[~hit] - fill[0]) <= 4 * 2.0 ** -23 * fill[0]).all(), "the frame's max(depth) fill"


def test_all_culled_frames_give_zeros_and_the_background(dev):
    f = SPG.frame_case(mode="classic")
    m = _model(dev, f)
    H, W = f.cam["H"], f.cam["W"]
    bg = torch.from_numpy(SPG.FRAME_BG).to(dev)
    away = f.c2w.copy()
    away[:, 3] = (40.0, 0.0, 0.0)
    away[:, 2] = -away[:, 2]          # looks away from the splats: every one is behind the camera
    away[:, 0] = -away[:, 0]
    with torch.cuda.device(dev):
        for cam, box in ((_camera(f, away), None), (_camera(f), _Nothing())):
            m.set_crop(box)
            out = m.get_splat_pose_jacobians_for_camera(cam)
            assert out["jacobian"].shape == (H, W, 5, 6) and float(out["jacobian"].abs().max()) == 0.0
            assert torch.equal(out["values"][..., :3], bg.expand(H, W, 3)) and float(out["values"][..., 3:].abs().max()) == 0.0
            sub = m.get_splat_pose_jacobians_for_camera(cam, channels=("expected_depth", "g"), basis="c2w")
            assert sub["jacobian"].shape == (H, W, 2, 12) and torch.equal(sub["values"][..., 0], bg[1].expand(H, W))
            unc = m.get_splat_pose_uncertainty_for_camera(cam, torch.full((6,), 0.01))
            assert float(unc["rgb_std_pose"].abs().max()) == 0.0 and float(unc["depth_std_pose"].abs().max()) == 0.0
            assert torch.equal(unc["rgb"], bg.expand(H, W, 3)) and float(unc["depth"].abs().max()) == 0.0
        m.set_crop(None)
        with pytest.raises(NotImplementedError, match="pinhole"):
            m.get_splat_pose_jacobians_for_camera(_camera(f, camera_type=2))
