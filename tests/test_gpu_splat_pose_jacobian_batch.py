"""The batched splat pose Jacobian on the GPU.  Nothing here has a tolerance: the single-view kernels are held to float64 in
tests/test_gpu_splat_pose_jacobian.py, and every view of a batch must return their bits (torch.equal), view by view:

  1. splat_pose_ptangents_batch_kernel against unerf_splat_pose_tangents followed by unerf_splat_pose_tangents_proj;
  2. splat_pose_jac_batch_kernel on SPG's hand-built lists stacked as the views of one batch;
  3. whole frames through splat.pose_jacobian_cameras against splat.pose_jacobian_camera;
  4. the models and the plugin classes; 5. refusals."""
import ctypes as C
import functools
import itertools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import splat_pose_grad_cases as SPG
import splat_pose_jac_cases as JC
from conftest import ROOT

pytestmark = pytest.mark.gpu
GUARD = 77.25
f32 = np.float32


def _t(dev, a):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


def _bits(a, b):
    """equal bit for bit (a NaN equals itself)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), f"{what}: {k} differs"


# ---------------------------------------------------------------------------------------------------------------------
# 1. the tangent stage
# ---------------------------------------------------------------------------------------------------------------------
def _tangent_views(B):
    """view 0: the case's own camera (its planted clip and fov limits are exact there); the others turn and shift it and have
    intrinsics of their own -> [(V [3,4] f32, fx, fy, cx, cy)]"""
    cam = SPG.tangent_case().cam
    out = []
    for v in range(B):
        a, b = 0.04 * v, -0.025 * v
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        V = np.concatenate([Ry @ Rx, np.array([[0.03 * v], [-0.02 * v], [0.05 * v]])], 1).astype(f32)
        out.append((V, cam["fx"] * (1 + 0.03 * v), cam["fy"] * (1 - 0.02 * v), cam["cx"] + 0.5 * v, cam["cy"] - 0.25 * v))
    return out


@pytest.mark.parametrize("B", [1, 2, 3, 16])
@pytest.mark.parametrize("N", [1, 255, 257, 301])
def test_tangent_stage_returns_the_two_kernel_routes_bits(dev, lib, N, B):
    from uncertainty_nerf_gs_amd import ops
    tc = SPG.tangent_case()
    H, W = tc.cam["H"], tc.cam["W"]
    assert N <= tc.N
    with np.errstate(divide="ignore"):
        log_scales = np.log(tc.scales[:N])                       # (the flat plant: log 0 = -inf, exp(-inf) = 0)
    means, scales, quats = _t(dev, tc.means[:N]), _t(dev, log_scales), _t(dev, tc.quats[:N])
    vs = _tangent_views(B)
    rng = np.random.default_rng([N, B])
    with torch.cuda.device(dev):
        views = ops.splat_view_records([torch.from_numpy(v[0]) for v in vs], *zip(*[v[1:] for v in vs]), [torch.zeros(3)] * B)
        pb = ops.splat_project_batch(means, scales, quats, views, B, H, W, 16, clip_thresh=SPG.TAN_CLIP, want_cov3d=True)
        plain = ops.splat_project_batch(means, scales, quats, views, B, H, W, 16, clip_thresh=SPG.TAN_CLIP)
        assert len(pb) == 8 and len(plain) == 7 and pb[7].shape == (B, N, 6)
        for a, b in zip(plain[:6], pb[:6]):
            assert torch.equal(a, b), "want_cov3d must not move the other outputs"
        radii, cov3d = pb[2], pb[7]
        single, tans = [], []
        for v, (V, fx, fy, cx, cy) in enumerate(vs):
            one = ops.splat_project(means, scales, 1.0, quats, torch.from_numpy(V), fx, fy, cx, cy, H, W, 16, clip_thresh=SPG.TAN_CLIP,
                                    raw=True)
            assert torch.equal(one[2], radii[v]) and torch.equal(one[6], cov3d[v]), f"view {v}: radii / cov3d of the single-view projection"
            tans.append(ops.splat_pose_tangents(means, one[6], one[2], torch.from_numpy(V), fx, fy, cx, cy, H, W, clip_thresh=SPG.TAN_CLIP))
        if N == 301:
            assert int((radii[0] > 0).sum()) > 200 and int((radii[0] == 0).sum()) >= 4, "view 0 keeps the case's live and dead plants"
        for P in (1, 6, 7, 12):
            PW = lib.splat_pose_pw(P)
            projs = rng.standard_normal((B, 12, P)).astype(f32)
            want = torch.stack([ops.splat_pose_tangents_proj(tans[v], means, radii[v], torch.from_numpy(projs[v])) for v in range(B)])
            n = B * N * 7 * PW
            buf = torch.full((n + 128,), GUARD, device=dev)
            out = buf[64:64 + n].view(B, N, 7, PW)
            got = ops.splat_pose_ptangents_batch(means, cov3d, radii, views, B, _t(dev, projs), H, W, clip_thresh=SPG.TAN_CLIP, out=out)
            torch.cuda.synchronize()
            assert (buf[:64] == GUARD).all() and (buf[64 + n:] == GUARD).all(), "floats around the array were written"
            for v in range(B):
                assert _bits(got[v], want[v]), f"P={P}: view {v} of {B} differs from the two-kernel route"
            assert (got[..., P:] == 0).all(), "columns P .. PW-1 must be exact zeros"
            assert (got[radii == 0] == 0).all(), "rows of culled splats must be zero"
            assert N == 1 or float(got.abs().max()) > 0
            # the same bits from a NaN-filled buffer on a side stream, from a host matrix, and on a second call
            dirty = torch.full((B, N, 7, PW), float("nan"), device=dev)
            torch.cuda.synchronize()
            side = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(side):
                ops.splat_pose_ptangents_batch(means, cov3d, radii, views, B, torch.from_numpy(projs), H, W, clip_thresh=SPG.TAN_CLIP,
                                               out=dirty)
            side.synchronize()
            assert _bits(dirty, got)
            again = ops.splat_pose_ptangents_batch(means, cov3d, radii, views, B, _t(dev, projs), H, W, clip_thresh=SPG.TAN_CLIP)
            assert _bits(again, got)
    # a view's block depends on nothing but its own camera and matrix: view 0 is the one-view batch's
    if B > 1:
        with torch.cuda.device(dev):
            v0 = ops.splat_view_records([torch.from_numpy(vs[0][0])], *[[x] for x in vs[0][1:]], [torch.zeros(3)])
            alone = ops.splat_pose_ptangents_batch(means, cov3d[:1].contiguous(), radii[:1].contiguous(), v0, 1, _t(dev, projs[:1]), H, W,
                                                   clip_thresh=SPG.TAN_CLIP)
        assert _bits(alone[0], got[0])


# ---------------------------------------------------------------------------------------------------------------------
# 2. the walk
# ---------------------------------------------------------------------------------------------------------------------
EMPTY = "empty"          # a view whose bins are all empty


@functools.lru_cache(maxsize=None)
def _groups():
    """the walk cases that can share a batch: same image and block width -> {(H, W, bw): [names]}"""
    g = {}
    for name, make in SPG.WALK.items():
        c = make()
        g.setdefault((c.H, c.W, c.bw), []).append(name)
    return g


def _group_of(name):
    return next(k for k, v in _groups().items() if name in v)


_ONE = {}


def _view_tensors(dev, name):
    """a case's own arrays on the device (what the single-view call reads)"""
    if name not in _ONE:
        c, w = SPG.WALK[name](), JC.walk_inputs(name)
        t = {k: _t(dev, getattr(c, k)) for k in ("gids", "bins", "xys", "conics", "opac", "colors", "comp", "bg")}
        t["z"], t["ptan12"] = _t(dev, w.z), _t(dev, w.ptan)
        t["ptan6"] = t["ptan12"][..., :6].contiguous()
        t["N"] = c.N
        _ONE[name] = t
    return _ONE[name]


_REF = {}


def _single(dev, name, aa, P, **kw):
    """the single-view walk on a case's own arrays (the full call is computed once and shared, unchanged)"""
    if not kw:
        if (name, aa, P) not in _REF:
            _REF[name, aa, P] = _single(dev, name, aa, P, want=("proj", "var", "val"))
        return _REF[name, aa, P]
    from uncertainty_nerf_gs_amd import ops
    c, t = SPG.WALK[name](), _view_tensors(dev, name)
    kw.setdefault("want", ("proj", "var", "val"))
    return ops.splat_pose_jacobian(t["gids"], t["bins"], t["xys"], t["conics"], t["colors"], t["z"], t["opac"],
                                   t["ptan6" if P <= 6 else "ptan12"], P, c.H, c.W, t["bg"], compensation=t["comp"] if aa else None,
                                   block_width=c.bw, **kw)


def _stack(dev, names, cstride=3):
    """the named cases as the views of one batch: per-view arrays padded to the largest N with NaN (no list names a padding row),
    ids offset by v N, bins offset into the concatenated id array; colour rows of `cstride` floats, NaN behind the three"""
    H, W, bw = _group_of(next(n for n in names if n != EMPTY))
    tiles = ((W + bw - 1) // bw) * ((H + bw - 1) // bw)
    B = len(names)
    N = max(_view_tensors(dev, n)["N"] for n in names if n != EMPTY)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    b = SimpleNamespace(B=B, N=N, H=H, W=W, bw=bw, xys=nan(B, N, 2), conics=nan(B, N, 3), colors=nan(B, N, cstride), z=nan(B, N),
                        opac=nan(B, N), comp=nan(B, N), ptan12=nan(B, N, 7, 12), bins=torch.zeros(B, tiles, 2, device=dev, dtype=torch.int32))
    ids, at = [], 0
    for v, name in enumerate(names):
        if name == EMPTY:
            b.bins[v] = at
            continue
        t = _view_tensors(dev, name)
        n = t["N"]
        for k, src in (("xys", "xys"), ("conics", "conics"), ("z", "z"), ("opac", "opac"), ("comp", "comp"), ("ptan12", "ptan12")):
            getattr(b, k)[v, :n] = t[src]
        b.colors[v, :n, :3] = t["colors"]
        ids.append(t["gids"] + v * N)
        b.bins[v] = t["bins"] + at
        at += t["gids"].numel()
    b.gids = torch.cat(ids) if ids else torch.zeros(1, device=dev, dtype=torch.int32)
    b.ptan6 = b.ptan12[..., :6].contiguous()
    b.bg = _view_tensors(dev, next(n for n in names if n != EMPTY))["bg"]
    return b


def _batch(b, aa, P, **kw):
    from uncertainty_nerf_gs_amd import ops
    kw.setdefault("want", ("proj", "var", "val"))
    return ops.splat_pose_jacobian_batch(b.gids, b.bins, b.xys, b.conics, b.colors, b.z, b.opac, b.ptan6 if P <= 6 else b.ptan12, P,
                                         b.H, b.W, b.bg, compensation=b.comp if aa else None, block_width=b.bw, **kw)


def _empty_view(b, P, want, rows=(0, 1, 2, 3, 4)):
    """what the single-view walk gives on empty lists: the background, zero rows"""
    val = torch.zeros(b.H, b.W, 5, device=b.bg.device)
    val[..., :3] = b.bg
    out = {"proj": torch.zeros(b.H, b.W, len(rows), P, device=b.bg.device), "var": torch.zeros(b.H, b.W, len(rows), device=b.bg.device),
           "val": val[..., list(rows)]}
    return {k: out[k] for k in want}


ANCHORS = ("lists", "quad", "bw8")          # one per image size and block width the walk cases come in (others join their group)


def _group_names(anchor):
    """the anchor first, then the other cases of its image size and block width"""
    return [anchor] + [n for n in _groups()[_group_of(anchor)] if n != anchor]


def _arrangement(anchor, kind):
    names = _group_names(anchor)
    a, z = names[0], names[-1]
    if kind == "all":                                                   # every case of the group, list after list
        return tuple(names)
    if kind == "gap":                                                   # all bins empty between two full views
        return (a, EMPTY, z)
    if kind == "sixteen":                                               # 16 views, the same case first and last
        return tuple([a] + [(names + [EMPTY])[k % (len(names) + 1)] for k in range(1, 15)] + [a])
    return (names[len(names) // 2],)                                    # B = 1


@pytest.mark.parametrize("P", [6, 12])
@pytest.mark.parametrize("aa", [False, True], ids=["classic", "antialiased"])
@pytest.mark.parametrize("kind", ["all", "gap", "sixteen", "one"])
@pytest.mark.parametrize("anchor", ANCHORS)
def test_walk_views_return_the_single_view_bits(dev, anchor, kind, aa, P):
    names = _arrangement(anchor, kind)
    assert {n for a in ANCHORS for n in _group_names(a)} == set(SPG.WALK), "every walk case is in some batch"
    b = _stack(dev, names)
    with torch.cuda.device(dev):
        got = _batch(b, aa, P)
        torch.cuda.synchronize()
        assert got["proj"].shape == (b.B, b.H, b.W, 5, P) and got["var"].shape == got["val"].shape == (b.B, b.H, b.W, 5)
        for v, name in enumerate(names):
            want = _empty_view(b, P, ("proj", "var", "val")) if name == EMPTY else _single(dev, name, aa, P)
            _same({k: got[k][v] for k in got}, want, f"view {v} ({name}) of {names}")
        _same(got, _batch(b, aa, P), "two calls")
        _same(got, _batch(b, aa, P, cull=False), "culled and unculled walks")
    if len(names) == 16:
        assert names[0] == names[15] != EMPTY
        _same({k: got[k][0] for k in got}, {k: got[k][15] for k in got}, "the same case at view 0 and at view 15")
    # the lists meet: a view's last tile ends exactly where the next view's first tile begins
    for v in range(b.B - 1):
        assert int(b.bins[v, -1, 1]) == int(b.bins[v + 1, 0, 0])


def test_walk_view_does_not_depend_on_its_neighbours_or_its_place(dev):
    name = "stops"
    others = [n for n in _groups()[_group_of(name)] if n != name]
    with torch.cuda.device(dev):
        ref = _single(dev, name, True, 12)
        for names in ((name,), (name, others[0]), (others[0], name), (others[-1], EMPTY, name, others[0]), (EMPTY, name, EMPTY)):
            got = _batch(_stack(dev, names), True, 12)
            v = names.index(name)
            _same({k: got[k][v] for k in got}, ref, f"{name} as view {v} of {names}")


@pytest.mark.parametrize("aa", [False, True], ids=["classic", "antialiased"])
def test_walk_channel_output_and_stride_subsets(dev, lib, aa):
    names = ("lists", "stops", EMPTY)
    wants = [w for r in (1, 2, 3) for w in itertools.combinations(("proj", "var", "val"), r)]
    order = {ch: k for k, ch in enumerate(JC.CHANNELS)}
    with torch.cuda.device(dev):
        stacks = {cs: _stack(dev, names, cs) for cs in (3, 4, 5)}
        for P in (6, 12):
            for cs, b in stacks.items():                                # 3-, 4- and 5-float colour rows, NaN in the unused floats
                assert cs == 3 or bool(torch.isnan(b.colors[..., 3:]).all())
                full = _batch(b, aa, P)
                for v, name in enumerate(names[:2]):
                    _same({k: full[k][v] for k in full}, _single(dev, name, aa, P), f"colour stride {cs}, view {v}")
            b = stacks[4]
            for chans in (("g",), ("expected_depth", "r"), ("accumulation",), ("b", "accumulation", "expected_depth"), ("r", "g", "b")):
                rows = sorted(order[ch] for ch in chans)
                for want in wants:
                    got = _batch(b, aa, P, channels=chans, want=want)
                    assert sorted(got) == sorted(want)
                    for v, name in enumerate(names):
                        one = _empty_view(b, P, want, rows) if name == EMPTY else _single(dev, name, aa, P, channels=chans, want=want)
                        _same({k: got[k][v] for k in got}, one, f"channels={chans} want={want} view {v}")
        # widths: P = 1 and 5 run the 6-wide instantiation, P = 7 the 12-wide one; columns beyond P are not read into the variance
        b = stacks[3]
        for P in (1, 5, 7):
            PW = lib.splat_pose_pw(P)
            ptan = torch.full((b.B, b.N, 7, PW), 1e3, device=dev)
            ptan[..., :P] = b.ptan12[..., :P]
            from uncertainty_nerf_gs_amd import ops
            got = ops.splat_pose_jacobian_batch(b.gids, b.bins, b.xys, b.conics, b.colors, b.z, b.opac, ptan, P, b.H, b.W, b.bg,
                                                compensation=b.comp if aa else None, block_width=b.bw, want=("proj", "var", "val"))
            for v, name in enumerate(names[:2]):
                t = _view_tensors(dev, name)
                c = SPG.WALK[name]()
                one = ops.splat_pose_jacobian(t["gids"], t["bins"], t["xys"], t["conics"], t["colors"], t["z"], t["opac"],
                                              ptan[v, :t["N"]].contiguous(), P, c.H, c.W, t["bg"], compensation=t["comp"] if aa else None,
                                              block_width=c.bw, want=("proj", "var", "val"))
                _same({k: got[k][v] for k in got}, one, f"P={P} view {v}")
        # dirty buffers with guard floats around all three outputs, on a side stream
        b, P = stacks[5], 12
        full = _batch(b, aa, P)
        n = b.B * b.H * b.W * 5
        sizes = {"proj": n * P, "var": n, "val": n}
        bufs = {k: torch.full((s + 128,), GUARD, device=dev) for k, s in sizes.items()}
        outs = {k: bufs[k][64:64 + sizes[k]].view(full[k].shape) for k in sizes}
        for o in outs.values():
            o.fill_(float("nan"))
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            got = _batch(b, aa, P, out=outs)
        side.synchronize()
        _same(full, got, "dirty buffers on a side stream")
        for k, buf in bufs.items():
            assert (buf[:64] == GUARD).all() and (buf[64 + sizes[k]:] == GUARD).all(), f"floats around out_{k} were written"


# ---------------------------------------------------------------------------------------------------------------------
# 3. whole frames
# ---------------------------------------------------------------------------------------------------------------------
FRAMES = [dict(mode="classic"), dict(mode="antialiased"), dict(mode="classic", sheared=True), dict(mode="classic", sh0=True),
          dict(mode="antialiased", crop=True)]
COV = (lambda a: a @ a.T * 1e-4)(np.random.default_rng(8).standard_normal((6, 6)))


def _away(c2w):
    away = np.array(c2w)
    away[:, 3] = (40.0, 0.0, 0.0)
    away[:, 2] = -away[:, 2]              # looks away from the splats: every one is behind the camera
    away[:, 0] = -away[:, 0]
    return away


def _poses(f, B):
    """B poses around the case's own, one of them (in the middle, for B >= 3) looking away; per-view intrinsics"""
    from uncertainty_nerf_gs_amd import posegrad
    base = torch.from_numpy(f.c2w)
    params = posegrad.POSE_PARAMS
    c2ws = [posegrad.perturbed_pose(base, params[v % 6], (0.01 if v % 6 < 3 else 0.004) * (1 + v // 6) * (-1) ** v) for v in range(B)]
    if B >= 3:
        c2ws[B // 2] = torch.from_numpy(_away(f.c2w))
    cam = f.cam
    intr = [[cam[k] * (1 + s * 0.01 * v) for v in range(B)] for k, s in (("fx", 1), ("fy", -1), ("cx", 0.5), ("cy", -0.5))]
    return torch.stack(c2ws), intr


def _frame_kw(dev, f, **extra):
    kw = dict(sh_degree=3, rasterize_mode=f.mode, config_sh_degree=0 if f.sh0 else 3,
              crop_ids=None if f.crop_ids is None else torch.from_numpy(f.crop_ids).to(dev))
    kw.update(extra)
    return kw


@pytest.mark.parametrize("kw", FRAMES, ids=lambda v: "-".join(f"{a}={b}" for a, b in v.items()))
def test_frames_match_the_single_camera_call(dev, kw):
    from uncertainty_nerf_gs_amd import posegrad, splat
    f = SPG.frame_case(**kw)
    H, W = f.cam["H"], f.cam["W"]
    gp = {k: torch.from_numpy(v).to(dev) for k, v in f.gp.items()}
    bg = torch.from_numpy(SPG.FRAME_BG).to(dev)
    c2ws, (fx, fy, cx, cy) = _poses(f, 16)
    forms = {"c2w": (dict(), lambda c: None, ("proj", "val")),
             "se3": (dict(projs=[posegrad.pose_projection(c) for c in c2ws]), lambda c: posegrad.pose_projection(c), ("proj", "val")),
             "cov": (dict(pose_covs=torch.from_numpy(COV)), lambda c: posegrad.pose_projection(c, torch.from_numpy(COV)), ("var", "val"))}
    with torch.cuda.device(dev):
        for form, (bkw, proj_of, want) in forms.items():
            single = [splat.pose_jacobian_camera(gp, c2ws[v], fx[v], fy[v], cx[v], cy[v], H, W, bg, proj=proj_of(c2ws[v]), want=want,
                                                 **_frame_kw(dev, f)) for v in range(16)]
            hit = [float(s["val"][..., 3].max()) > 0 for s in single]
            assert not hit[8] and sum(hit) == 15, "one view in the middle sees nothing, the others render"
            for B in (2, 3, 16):
                # B = 3 takes views 7, 8, 9: the empty one in the middle of the batch
                sel = list(range(16)) if B == 16 else [7, 8, 9] if B == 3 else [3, 12]
                sub = {k: ([v[i] for i in sel] if isinstance(v, list) else v) for k, v in bkw.items()}
                got = splat.pose_jacobian_cameras(gp, c2ws[sel], [fx[i] for i in sel], [fy[i] for i in sel], [cx[i] for i in sel],
                                                  [cy[i] for i in sel], H, W, bg, want=want, **sub, **_frame_kw(dev, f))
                assert len(got) == B
                for k, i in enumerate(sel):
                    _same(got[k], single[i], f"{form}: view {k} (pose {i}) of a batch of {B}")
        # a channel subset, one projection for all views, loose lists
        P7 = torch.from_numpy(np.random.default_rng(2).standard_normal((12, 7)))
        sel = [0, 8, 5]
        for extra in (dict(channels=("expected_depth", "g")), dict(tight=False)):
            got = splat.pose_jacobian_cameras(gp, c2ws[sel], fx[0], fy[0], cx[0], cy[0], H, W, bg, projs=P7, want=("proj", "var", "val"),
                                              **_frame_kw(dev, f, **extra))
            for k, i in enumerate(sel):
                one = splat.pose_jacobian_camera(gp, c2ws[i], fx[0], fy[0], cx[0], cy[0], H, W, bg, proj=P7, want=("proj", "var", "val"),
                                                 **_frame_kw(dev, f, **extra))
                _same(got[k], one, f"{extra}: view {k}")


def test_frames_with_nothing_to_render(dev):
    from uncertainty_nerf_gs_amd import ops, splat
    f = SPG.frame_case(mode="classic")
    H, W = f.cam["H"], f.cam["W"]
    gp = {k: torch.from_numpy(v).to(dev) for k, v in f.gp.items()}
    bg = torch.from_numpy(SPG.FRAME_BG).to(dev)
    c2ws, (fx, fy, cx, cy) = _poses(f, 3)
    away = torch.from_numpy(np.stack([_away(f.c2w)] * 3))
    nothing = torch.zeros(len(f.gp["means"]), dtype=torch.bool, device=dev)
    none = {k: v[:0] for k, v in gp.items()}
    with torch.cuda.device(dev):
        for what, a, kw in (("every view looks away", (gp, away), {}), ("a crop that removes every splat", (gp, c2ws), dict(crop_ids=nothing)),
                            ("N == 0", (none, c2ws), {})):
            for want, chans in ((("proj", "val"), ops.POSE_CHANNELS), (("var", "val", "proj"), ("accumulation", "b"))):
                got = splat.pose_jacobian_cameras(*a, fx, fy, cx, cy, H, W, bg, channels=chans, want=want, **kw)
                assert len(got) == 3
                for v in range(3):
                    one = splat.pose_jacobian_camera(a[0], a[1][v], fx[v], fy[v], cx[v], cy[v], H, W, bg, channels=chans, want=want, **kw)
                    _same(got[v], one, f"{what}: view {v}")
                    assert float(got[v]["proj"].abs().max()) == 0.0 and got[v]["proj"].shape == (H, W, len(chans), 12)
                if chans is ops.POSE_CHANNELS:
                    assert torch.equal(got[0]["val"][..., :3], bg.expand(H, W, 3)) and float(got[0]["val"][..., 3:].abs().max()) == 0.0


def test_image_beyond_the_batched_tile_limit_takes_the_loop(dev, lib, monkeypatch):
    from uncertainty_nerf_gs_amd import ops, posegrad, splat
    f = SPG.frame_case(mode="classic")
    H = W = 110                                                         # block_width 1: 12,100 tiles > 11,999
    assert H * W > lib.SPLAT_BATCH_MAX_TILES
    gp = {k: torch.from_numpy(v).to(dev) for k, v in f.gp.items()}
    bg = torch.from_numpy(SPG.FRAME_BG).to(dev)
    c2ws, _ = _poses(f, 2)
    fx, fy, cx, cy = [100.0, 104.0], [98.0, 97.0], [55.3, 54.0], [54.6, 56.0]
    projs = [posegrad.pose_projection(c) for c in c2ws]
    batched = []
    real = ops.splat_pose_jacobian_batch
    monkeypatch.setattr(ops, "splat_pose_jacobian_batch", lambda *a, **kw: batched.append(1) or real(*a, **kw))
    with torch.cuda.device(dev):
        got = splat.pose_jacobian_cameras(gp, c2ws, fx, fy, cx, cy, H, W, bg, projs=projs, block_width=1)
        assert not batched, "12,100 tiles must take the per-view loop"
        for v in range(2):
            one = splat.pose_jacobian_camera(gp, c2ws[v], fx[v], fy[v], cx[v], cy[v], H, W, bg, proj=projs[v], block_width=1)
            _same(got[v], one, f"view {v}")
            assert float(one["val"][..., 3].max()) > 0
        # the same image at block_width 16 shares its launches, with the same results
        got16 = splat.pose_jacobian_cameras(gp, c2ws, fx, fy, cx, cy, H, W, bg, projs=projs)
        assert batched == [1]
        for v in range(2):
            _same(got16[v], splat.pose_jacobian_camera(gp, c2ws[v], fx[v], fy[v], cx[v], cy[v], H, W, bg, proj=projs[v]), f"view {v}")


# ---------------------------------------------------------------------------------------------------------------------
# 4. the models and the plugin
# ---------------------------------------------------------------------------------------------------------------------
class _Box:
    def within(self, pts):
        return (pts[:, 0] < 0.4)[:, None]


def _state(f, active):
    return {f"gauss_params.{k}": torch.from_numpy(v) for k, v in f.gp.items() if active or k != "log_uncertainties"}


def _model(dev, f, active=True, through_plugin=False):
    from uncertainty_nerf_gs_amd import models, plugin
    if through_plugin:
        try:
            import nerfstudio  # noqa: F401
        except ImportError:
            sys.path.insert(0, os.path.join(ROOT, "tests", "stubs"))
        cfg = plugin.method_specifications()["active-splatfacto"].config.pipeline.model
        cfg.rasterize_mode = f.mode
        m = cfg.setup(scene_box=None, num_train_data=2, seed_points=(torch.rand(4, 3), torch.zeros(4, 3)))
        m.load_state_dict({"_model." + k: v for k, v in _state(f, True).items()})
        return m.to(dev).eval()
    cfg = (models.ActiveSplatfactoModelConfig if active else models.SplatfactoModelConfig)()
    cfg.rasterize_mode = f.mode
    if f.sh0:
        cfg.sh_degree = 0
    m = cfg._target(cfg, num_points=4)
    m.load_state_dict(_state(f, active))
    return m.to(dev).eval()


@pytest.mark.parametrize("kw,active,through_plugin", [(dict(mode="classic"), True, False), (dict(mode="antialiased", crop=True), True, True),
                                                      (dict(mode="classic", sh0=True), False, False)],
                         ids=["active", "plugin-antialiased-crop", "plain-sh0"])
def test_models_match_the_single_camera_methods(dev, kw, active, through_plugin):
    f = SPG.frame_case(**kw)
    H, W, B = f.cam["H"], f.cam["W"], 5
    m = _model(dev, f, active, through_plugin)
    c2ws, (fx, fy, cx, cy) = _poses(f, B)
    col = lambda a: torch.tensor(a, dtype=torch.float32)[:, None]
    cams = SimpleNamespace(camera_to_worlds=c2ws, fx=col(fx), fy=col(fy), cx=col(cx), cy=col(cy), height=torch.full((B, 1), H),
                           width=torch.full((B, 1), W))
    cam = lambda v: SimpleNamespace(camera_to_worlds=c2ws[v:v + 1], fx=col(fx)[v], fy=col(fy)[v], cx=col(cx)[v], cy=col(cy)[v], height=H,
                                    width=W)
    covs = [torch.from_numpy(COV * (v + 1)) for v in range(B)]
    std = torch.tensor([0.02, 0.01, 0.03, 4e-3, 2e-3, 3e-3])
    with torch.cuda.device(dev):
        (m._mirror if through_plugin else m).set_crop(_Box() if kw.get("crop") else None)
        one_se3 = [m.get_splat_pose_jacobians_for_camera(cam(v)) for v in range(B)]
        one_c2w = [m.get_splat_pose_jacobians_for_camera(cam(v), channels=("expected_depth", "r"), basis="c2w") for v in range(B)]
        one_unc = [m.get_splat_pose_uncertainty_for_camera(cam(v), covs[v]) for v in range(B)]
        one_std = [m.get_splat_pose_uncertainty_for_camera(cam(v), std) for v in range(B)]
        for mv in (1, 2, 16):
            got = m.get_splat_pose_jacobians_for_cameras(cams, max_views=mv)
            assert len(got) == B
            for v in range(B):
                _same(got[v], one_se3[v], f"max_views={mv} se3 camera {v}")
            got = m.get_splat_pose_jacobians_for_cameras(cams, channels=("expected_depth", "r"), basis="c2w", max_views=mv)
            for v in range(B):
                _same(got[v], one_c2w[v], f"max_views={mv} c2w camera {v}")
            for pose_cov, ones, what in ((covs, one_unc, "one covariance per camera"), (std, one_std, "one for all cameras")):
                got = m.get_splat_pose_uncertainty_for_cameras(cams, pose_cov, max_views=mv)
                for v in range(B):
                    _same(got[v], ones[v], f"max_views={mv} {what}, camera {v}")
                    assert torch.equal(got[v]["rgb_std_pose"], got[v]["rgb_var_pose"].sqrt())
        # each view's depth fill is its own maximum of the unnormalised depth sums
        got = m.get_splat_pose_uncertainty_for_cameras(cams, std)
        fills = []
        for v in range(B):
            acc, d = got[v]["accumulation"], got[v]["depth"]
            miss = acc == 0
            assert bool(miss.any())
            fills.append(float(d[miss][0]))
            if v != B // 2:
                assert bool((d[miss] == fills[-1]).all()) and fills[-1] == float((d * acc)[~miss].max()), f"camera {v}: its own fill"
        assert fills[B // 2] == 0.0 and len(set(fills)) == B, "the empty view fills with 0, the others with different maxima"
        torch.cuda.synchronize()


def test_non_splat_plugin_mirrors_raise():
    try:
        import nerfstudio  # noqa: F401
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, "tests", "stubs"))
    from uncertainty_nerf_gs_amd import plugin
    cfg = plugin.method_specifications()["nerfacto-mcdropout"].config.pipeline.model
    cfg.log2_hashmap_size, cfg.num_levels, cfg.max_res = 8, 16, 64
    cfg.proposal_net_args_list = [dict(a, log2_hashmap_size=6) for a in cfg.proposal_net_args_list]
    model = cfg.setup(scene_box=None, num_train_data=1)
    with pytest.raises(NotImplementedError, match="not a splat"):
        model.get_splat_pose_jacobians_for_cameras(SimpleNamespace())
    with pytest.raises(NotImplementedError, match="not a splat"):
        model.get_splat_pose_uncertainty_for_cameras(SimpleNamespace(), torch.zeros(6))


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(dev, lib):
    from uncertainty_nerf_gs_amd import ops
    b = _stack(dev, ("bw8", "bw8"))
    h = lib.load()
    n = b.B * b.H * b.W * 5
    tc = SPG.tangent_case()
    with torch.cuda.device(dev):
        outs = [torch.full((n * s,), GUARD, device=dev) for s in (6, 1, 1)]
        good = dict(ids=b.gids.data_ptr(), ptan=b.ptan6.data_ptr(), cs=3, B=b.B, N=b.N, P=6, bw=b.bw, flags=0, channels=31,
                    outs=tuple(o.data_ptr() for o in outs))

        def jac(**kw):
            a = {**good, **kw}
            return h.unerf_splat_pose_jacobian_batch(a["ids"], b.bins.data_ptr(), b.xys.data_ptr(), b.conics.data_ptr(), b.colors.data_ptr(),
                                                     a["cs"], b.z.data_ptr(), b.opac.data_ptr(), None, a["ptan"], None, a["B"], a["N"],
                                                     a["P"], b.H, b.W, a["bw"], a["flags"], a["channels"], *a["outs"], None)

        for text, kw in ((b"B=0 outside [1,16]", dict(B=0)), (b"B=17 outside [1,16]", dict(B=17)),
                         (b"B*N = 536870912 outside [0,2^29)", dict(B=16, N=1 << 25)), (b"B*N = 536870912 outside", dict(B=1, N=1 << 29)),
                         (b"null pointer (gaussian_ids_sorted", dict(ids=None)), (b"ptangents)", dict(ptan=None)),
                         (b"color_stride=2 below 3", dict(cs=2)), (b"P=0 outside [1,12]", dict(P=0)), (b"P=13 outside [1,12]", dict(P=13)),
                         (b"channels is empty", dict(channels=0)), (b"unknown channel bits 64", dict(channels=64 + 3)),
                         (b"no output asked for (out_proj, out_var and out_val are NULL)", dict(outs=(None, None, None))),
                         (b"unknown flags 4", dict(flags=4)), (b"block_width=0 outside [1,16]", dict(bw=0)),
                         (b"block_width=32 outside [1,16]", dict(bw=32)),
                         (b"ptangents must be 8-byte aligned for P=6", dict(ptan=b.ptan6.data_ptr() + 4)),
                         (b"ptangents must be 16-byte aligned for P=12", dict(ptan=b.ptan6.data_ptr() + 8, P=12))):
            assert jac(**kw) == -1, text
            assert b"splat_pose_jacobian_batch: " in h.unerf_last_error() and text in h.unerf_last_error(), h.unerf_last_error()
        torch.cuda.synchronize()
        for o in outs:
            assert (o == GUARD).all(), "a refused call wrote to an output"
        assert jac() == 0          # the same arguments, unbroken, run
        torch.cuda.synchronize()
        assert not (outs[0] == GUARD).any()

        # the tangent stage
        N, B, H, W = 64, 2, tc.cam["H"], tc.cam["W"]
        vs = _tangent_views(B)
        views = ops.splat_view_records([torch.from_numpy(v[0]) for v in vs], *zip(*[v[1:] for v in vs]), [torch.zeros(3)] * B)
        means = _t(dev, tc.means[:N])
        cov3d, radii = torch.rand(B, N, 6, device=dev), torch.ones(B, N, device=dev, dtype=torch.int32)
        proj = torch.rand(B, 12, 6, device=dev)
        out = torch.full((B * N * 7 * 6 + 4,), GUARD, device=dev)
        good = dict(means=means.data_ptr(), views=views, B=B, N=N, proj=proj.data_ptr(), P=6, H=H, out=out.data_ptr())

        def tan(**kw):
            a = {**good, **kw}
            return h.unerf_splat_pose_ptangents_batch(a["means"], cov3d.data_ptr(), radii.data_ptr(), a["views"], a["B"], a["N"], a["proj"],
                                                      a["P"], a["H"], W, 0.01, a["out"], None)

        for text, kw in ((b"B=0 outside [1,16]", dict(B=0)), (b"B=17 outside [1,16]", dict(B=17)),
                         (b"B*N = 536870912 outside [0,2^29)", dict(B=16, N=1 << 25)), (b"P=0 outside [1,12]", dict(P=0)),
                         (b"P=13 outside [1,12]", dict(P=13)), (b"null pointer (views_host)", dict(views=None)),
                         (b"null pointer (means3d", dict(means=None)), (b"null pointer (means3d", dict(proj=None)),
                         (b"bad H/W", dict(H=0)), (b"ptangents must be 8-byte aligned for P=6", dict(out=out.data_ptr() + 4)),
                         (b"ptangents must be 16-byte aligned for P=12", dict(out=out.data_ptr() + 8, P=12))):
            assert tan(**kw) == -1, text
            assert b"splat_pose_ptangents_batch: " in h.unerf_last_error() and text in h.unerf_last_error(), h.unerf_last_error()
        torch.cuda.synchronize()
        assert (out == GUARD).all(), "a refused call wrote to the output"
        assert tan() == 0 and tan(N=0) == 0
        torch.cuda.synchronize()
        assert not (out[:B * N * 7 * 6] == GUARD).any() and (out[B * N * 7 * 6:] == GUARD).all()
