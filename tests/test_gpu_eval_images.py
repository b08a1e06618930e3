"""unerf_eval_images_batch on the GPU, through the C ABI and through ops.eval_images / eval.save_imgs_rgb / run_eval: every
byte of every plane equals `eval.pack_eval_images` (the numpy definition; pinned against matplotlib's route in
tests/test_eval_images_cpu.py).  No tolerance: float32 differences, sum and normalisation, float64 colour index and
quantisation are correctly rounded IEEE operations on both sides.

Sizes, the smallest at which the two kernels can go wrong: 1, 3, 35 and 1,961 pixels (n and 3 n no multiple of 4 or 64, so
three of every four images of a stack have their planes start off a 4-byte boundary), 64 x 64, one pixel to either side of a workgroup's
share (EI_THREADS, read from the source), 300 x 300 (352 workgroups share one image's min / max), and one pixel more than
EI_THREADS * EI_MAX_WG, where a workgroup starts to stride."""
import functools
import re

import numpy as np
import pytest
import torch

import eval_image_cases as K

pytestmark = pytest.mark.gpu
GUARD = 64


@functools.lru_cache(maxsize=None)
def _kernel_constants():
    from uncertainty_nerf_gs_amd import lib as L
    src = open(L.CSRC + "/unerf_metrics.hip").read()
    return tuple(int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) for name in ("EI_THREADS", "EI_MAX_WG"))


@functools.lru_cache(maxsize=None)
def _want(kind, B, H, W):
    """inputs and the definition's planes, computed once per case and shared (read-only) by the tests"""
    from uncertainty_nerf_gs_amd import eval as E
    if kind == "values":
        pred, gt, std = (x[None] for x in K.value_case(H, W))
    else:
        pred, gt, std = K.range_stack(B, H, W)
    per = [E.pack_eval_images(pred[b], gt[b], std[b], K.UNC_MIN, K.UNC_MAX) for b in range(B)]
    want = {name: np.stack([p[name] for p in per]) for name in K.PLANES}
    for a in (pred, gt, std, *want.values()):
        a.setflags(write=False)
    return pred, gt, std, want


def _t(a):
    return torch.from_numpy(np.array(a))                                     # a writable copy of a shared, read-only case


def _dev(dev, *arrays):
    return [_t(a).to(dev) for a in arrays]


def _assert_planes(got, want, what):
    for name in K.PLANES:
        g = got[name].cpu().numpy() if torch.is_tensor(got[name]) else got[name]
        assert g.dtype == np.uint8 and g.shape == want[name].shape, (what, name, g.shape, want[name].shape)
        bad = np.flatnonzero((g != want[name]).reshape(-1))
        assert bad.size == 0, (f"{what}: plane {name}: {bad.size} bytes differ, first at {bad[:5]}: got "
                               f"{g.reshape(-1)[bad[:5]]}, want {want[name].reshape(-1)[bad[:5]]}")


def _sizes():
    T, G = _kernel_constants()
    return [(1, 1), (1, 3), (5, 7), (37, 53), (64, 64), (1, T - 1), (1, T + 1), (300, 300), (1, T * G + 1)]


@pytest.mark.parametrize("hw", _sizes(), ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_every_size_equals_the_definition(dev, hw):
    from uncertainty_nerf_gs_amd import ops
    H, W = hw
    for kind in ("range",) + (("values",) if H * W >= 40 else ()):
        pred, gt, std, want = _want(kind, 1, H, W)
        got = ops.eval_images(*_dev(dev, pred, gt, std), K.UNC_MIN, K.UNC_MAX)
        assert got["buffer"].numel() == 10 * H * W
        _assert_planes(got, want, f"{kind} {H}x{W}")


@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("hw", [(37, 53), (1, 257), (300, 300)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_a_batch_equals_its_images_alone(dev, B, hw):
    from uncertainty_nerf_gs_amd import ops
    H, W = hw
    pred, gt, std, want = _want("range", B, H, W)
    dp, dg, ds = _dev(dev, pred, gt, std)
    got = ops.eval_images(dp, dg, ds, K.UNC_MIN, K.UNC_MAX)
    _assert_planes(got, want, f"B={B} {H}x{W}")
    if B > 1:       # the range of an image is its own: image 0 holds the stack's largest std, image 1 the smallest
        assert std[0].reshape(-1)[-1] == np.nanmax(std) and std[1].reshape(-1)[0] == np.nanmin(std)
    for b in range(B):
        one = ops.eval_images(dp[b:b + 1], dg[b:b + 1], ds[b:b + 1], K.UNC_MIN, K.UNC_MAX)
        for name in K.PLANES:
            assert torch.equal(one[name][0], got[name][b]), (b, name)


def _abi_call(lib, dev, pred, gt, std, unc, want_planes, stream=None):
    """straight through the C ABI: one uint8 arena pre-filled with 0xA5, a guard region behind each plane, the workspace
    pre-filled with 0xA5 too -> ({plane: host bytes [B, n * ch] or None}, {plane: guard intact})"""
    from uncertainty_nerf_gs_amd import colormaps
    h = lib.load()
    B, n = std.shape[0], std[0].size
    dp, dg, ds = _dev(dev, pred, gt, std)
    lut = _t(colormaps.JET_U8).to(dev)
    sizes = {name: B * n * K.CHANNELS[name] for name in K.PLANES}
    arena = torch.full((GUARD + sum(sizes.values()) + 4 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    off, where = GUARD, {}
    for name in K.PLANES:
        where[name] = off
        off += sizes[name] + GUARD
    nbytes = h.unerf_eval_images_workspace_bytes(B)
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)
    ptrs = [arena.data_ptr() + where[name] if name in want_planes else None for name in K.PLANES]
    lo, span = float(min(unc)), float(abs(unc[1] - unc[0]))
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    rc = h.unerf_eval_images_batch(dp.data_ptr(), dg.data_ptr(), ds.data_ptr(), n, B, lo, span, lut.data_ptr(), *ptrs,
                                   ws.data_ptr(), nbytes, st)
    assert rc == 0, h.unerf_last_error().decode()
    (stream or torch.cuda.current_stream()).synchronize()
    host = arena.cpu().numpy()
    planes, untouched = {}, host[:GUARD].tolist() == [0xA5] * GUARD
    for name in K.PLANES:
        body = host[where[name]:where[name] + sizes[name]]
        untouched = untouched and (host[where[name] + sizes[name]:where[name] + sizes[name] + GUARD] == 0xA5).all()
        if name in want_planes:
            planes[name] = body.reshape((B,) + std.shape[1:] + ((3,) if K.CHANNELS[name] == 3 else ()))
        else:
            untouched = untouched and (body == 0xA5).all()                   # a NULL plane is not written
    return planes, bool(untouched)


@pytest.mark.parametrize("case", [("values", 1, 37, 53), ("range", 3, 5, 7), ("range", 3, 1, 257)], ids=str)
def test_c_abi_with_guards_and_null_planes(lib, dev, case):
    kind, B, H, W = case
    pred, gt, std, want = _want(kind, B, H, W)
    full, intact = _abi_call(lib, dev, pred, gt, std, (K.UNC_MIN, K.UNC_MAX), K.PLANES)
    assert intact, "bytes outside the planes were written"
    _assert_planes(full, want, f"abi {case}")
    for subset in (("std",), ("gt", "err"), ("pred",), ("err", "std")):
        part, intact = _abi_call(lib, dev, pred, gt, std, (K.UNC_MIN, K.UNC_MAX), subset)
        assert intact, (subset, "a NULL plane or a guard was written")
        for name in subset:
            assert np.array_equal(part[name], full[name]), (subset, name)


def test_swapped_range_constant_and_all_nan_std(lib, dev):
    from uncertainty_nerf_gs_amd import eval as E, ops
    pred, gt, std, want = _want("values", 1, 37, 53)
    dp, dg, ds = _dev(dev, pred, gt, std)
    swapped = ops.eval_images(dp, dg, ds, K.UNC_MAX, K.UNC_MIN)               # unc_min > unc_max: the same images
    _assert_planes(swapped, want, "swapped")
    other = E.pack_eval_images(pred[0], gt[0], std[0], 0.0, 1.0)
    assert not np.array_equal(other["std"], want["std"][0])
    _assert_planes(ops.eval_images(dp, dg, ds, 0.0, 1.0), {k: v[None] for k, v in other.items()}, "0..1")
    # a stack of: a constant image, an all-NaN image, an ordinary one -- the first two must not touch the third's range
    stack = np.stack([np.full((37, 53), 0.3, np.float32), np.full((37, 53), np.nan, np.float32), std[0]])
    p3, g3 = np.repeat(pred, 3, 0), np.repeat(gt, 3, 0)
    per = [E.pack_eval_images(p3[b], g3[b], stack[b], K.UNC_MIN, K.UNC_MAX) for b in range(3)]
    got = ops.eval_images(*_dev(dev, p3, g3, stack), K.UNC_MIN, K.UNC_MAX)
    _assert_planes(got, {name: np.stack([p[name] for p in per]) for name in K.PLANES}, "constant / NaN / ordinary")
    assert not got["std"][1].any() and (got["std"][0].cpu().numpy() == np.array([0, 0, 128])).all()


def test_side_stream_repeat_and_arena(lib, dev):
    from uncertainty_nerf_gs_amd import ops
    pred, gt, std, want = _want("range", 3, 37, 53)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    on_side, intact = _abi_call(lib, dev, pred, gt, std, (K.UNC_MIN, K.UNC_MAX), K.PLANES, stream=side)
    assert intact
    _assert_planes(on_side, want, "side stream")
    dp, dg, ds = _dev(dev, pred, gt, std)
    a = ops.eval_images(dp, dg, ds, K.UNC_MIN, K.UNC_MAX)
    b = ops.eval_images(dp, dg, ds, K.UNC_MIN, K.UNC_MAX)
    assert torch.equal(a["buffer"], b["buffer"]) and a["buffer"].data_ptr() != b["buffer"].data_ptr()
    arena = ops.Workspace()
    arena.get("eval_images", (10 * 3 * 37 * 53 + 999,), dev, dtype=torch.uint8).fill_(0xA5)      # dirty and larger than needed
    c = ops.eval_images(dp, dg, ds, K.UNC_MIN, K.UNC_MAX, workspace=arena)
    d = ops.eval_images(dp, dg, ds, K.UNC_MIN, K.UNC_MAX, workspace=arena)
    assert c["buffer"].data_ptr() == d["buffer"].data_ptr() and torch.equal(c["buffer"], a["buffer"])
    only = ops.eval_images(dp, dg, ds, K.UNC_MIN, K.UNC_MAX, want=("err", "std"))
    assert set(only) == {"err", "std", "buffer"} and torch.equal(only["std"], a["std"]) and torch.equal(only["err"], a["err"])


def _files(path):
    return {p.name: p.read_bytes() for p in sorted(path.iterdir())}


def test_save_imgs_rgb_fused_writes_the_files_of_the_host_route(dev, tmp_path):
    from uncertainty_nerf_gs_amd import eval as E
    pred, gt, std, want = _want("range", 4, 37, 53)
    outs = [{"rgb": _t(pred[b]).to(dev), "rgb_std": _t(std[b][..., None]).to(dev)} for b in range(4)]
    gts = [_t(gt[b]) for b in range(4)]
    ids = [3, 4, 10, 11]
    host = E.save_imgs_rgb(ids, outs, gts, tmp_path / "host", K.UNC_MIN, K.UNC_MAX, fused=False)
    fused = E.save_imgs_rgb(ids, outs, gts, tmp_path / "fused", K.UNC_MIN, K.UNC_MAX, fused=True)
    a, b = _files(tmp_path / "host"), _files(tmp_path / "fused")
    assert sorted(a) == sorted(f"{i}_rgb_{w}.png" for i in ids for w in ("gt", "pred", "abs_err", "std")) and a == b
    for j, i in enumerate(ids):
        _assert_planes(fused[i], {k: v[j] for k, v in want.items()}, f"image {i}")
        _assert_planes(host[i], {k: v[j] for k, v in want.items()}, f"image {i} (host)")
        assert np.array_equal(K.decode_png(tmp_path / "fused" / f"{i}_rgb_std.png"), want["std"][j])


def test_save_imgs_rgb_fused_chunks_a_long_list(dev, tmp_path, monkeypatch):
    from uncertainty_nerf_gs_amd import eval as E, lib as L, ops
    monkeypatch.setattr(L, "METRICS_MAX_IMAGES", 3)                          # the harness's chunk length, not the kernel's limit
    seen, inner = [], ops.eval_images
    monkeypatch.setattr(ops, "eval_images", lambda pred, *a, **kw: (seen.append(int(pred.shape[0])), inner(pred, *a, **kw))[1])
    pred, gt, std, want = _want("range", 4, 37, 53)
    outs = [{"rgb": _t(pred[b]).to(dev), "rgb_std": _t(std[b]).to(dev)} for b in range(4)]
    fused = E.save_imgs_rgb(range(4), outs, [_t(g) for g in gt], tmp_path, K.UNC_MIN, K.UNC_MAX, fused=True, encode=False)
    assert seen == [3, 1] and not any(tmp_path.iterdir())
    for b in range(4):
        _assert_planes(fused[b], {k: v[b] for k, v in want.items()}, f"image {b}")


def test_run_eval_fused_view_batch_saves_the_files_of_the_per_image_host_route(dev, tmp_path):
    from uncertainty_nerf_gs_amd import eval as E
    from uncertainty_nerf_gs_amd import models, synthetic
    import test_gpu_eval_harness as TH
    import test_gpu_models as TM
    t = synthetic.make_scene_tensors(seed=21, kind="active", log2T=14, prop_log2T=12)

    def model():
        cfg = TM._small_cfg(models.ActiveNerfactoModelConfig(average_init_density=0.01))
        m = cfg._target(cfg, num_train_data=4)
        m.load_state_dict(TM._state_dict_from_tensors(t, "active"))
        return m.to(dev)

    cams = TH._cams(6)
    first = model()
    eval_set = [(cam, TH._gt(first.get_outputs_for_camera(cam)["rgb"].cpu(), 100 + i)) for i, cam in enumerate(cams)]
    res = {}
    for name, kw in (("host", dict(fused=False, view_batch=1)), ("fused", dict(fused=True, view_batch=4))):
        ecfg = E.ActiveNerfactoConfig(load_config=None, output_path=tmp_path / name / "m.json", eval_depth=False,
                                      save_rendered_images=True, unc_min=0.0, unc_max=0.2)
        res[name] = E.run_eval(ecfg, model(), eval_set, **kw)
    assert list(res["host"]) == list(res["fused"])
    a = {k: v for k, v in _files(tmp_path / "host" / "plots").items() if not k.startswith("plot_")}
    b = {k: v for k, v in _files(tmp_path / "fused" / "plots").items() if not k.startswith("plot_")}
    assert sorted(a) == sorted(f"{i}_rgb_{w}.png" for i in range(6) for w in ("gt", "pred", "abs_err", "std"))
    assert sorted(b) == sorted(a)
    for k in a:
        assert a[k] == b[k], k
    std0 = K.decode_png(tmp_path / "fused" / "plots" / "0_rgb_std.png")
    assert std0.shape == (TH.H, TH.W, 3) and len(np.unique(std0.reshape(-1, 3), axis=0)) > 8      # a picture, not one colour
