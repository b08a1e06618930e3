"""LPIPS without a GPU: the host definition against a loop statement, the weights a checkpoint carries, model.lpips and
the eval keys, the refusals, and the C ABI of the new entry points (no launch).  Synthetic weights throughout; the one
comparison with torchmetrics itself runs only where torchmetrics and its cached weights exist."""
import ctypes as C
import json
import os
import subprocess
import warnings

import numpy as np
import pytest
import torch

import lpips_cases as LC
from conftest import ROOT
from uncertainty_nerf_gs_amd import checkpoints as CK
from uncertainty_nerf_gs_amd import eval as E
from uncertainty_nerf_gs_amd import metrics as M
from uncertainty_nerf_gs_amd import plugin, synthetic


# ---- the host definition ----------------------------------------------------------------------------------------------

def test_host_definition_equals_the_loop_statement():
    """metrics.lpips in float64 against explicit numpy loops over pixels, taps and channels (lpips_cases.loop_lpips) on a
    31 x 33 pair: the smallest height, a width that is no multiple of the stride, a prediction that is clipped"""
    pred, target = LC.image_pair(31, 33)
    assert float(pred.max()) > 1.0
    got = M.lpips(pred, target, LC.weights(), dtype=torch.float64)
    want = LC.loop_lpips(pred, target, LC.weights())
    print(f"lpips float64 {got!r}, loop statement {want!r}")
    assert want > 1e-3
    assert abs(got - want) <= 1e-12 * abs(want)


def test_map_sizes_follow_the_trunk():
    assert M.lpips_map_sizes(31, 31) == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    assert M.lpips_map_sizes(64, 48) == [(15, 11), (7, 5), (3, 2), (3, 2), (3, 2)]
    taps = M.lpips_features(torch.rand(2, 35, 50, 3), LC.weights())
    assert [tuple(t.shape[2:]) for t in taps] == M.lpips_map_sizes(35, 50)
    assert [t.shape[1] for t in taps] == [64, 192, 384, 256, 256]


def test_a_batch_is_the_mean_of_its_images():
    pred, target = LC.image_pair(31, 40, B=3)
    per = M.lpips_per_image(pred, target, LC.weights(), torch.float64)
    assert per.shape == (3,)
    for b in range(3):
        assert abs(float(per[b]) - M.lpips(pred[b], target[b], LC.weights(), torch.float64)) <= 1e-14
    assert abs(M.lpips(pred, target, LC.weights(), torch.float64) - float(per.mean())) <= 1e-15


def test_refusals():
    w = LC.weights()
    pred, target = LC.image_pair(30, 40)
    with pytest.raises(ValueError, match="31"):
        M.lpips(pred, target, w)
    pred, target = LC.image_pair(32, 40)
    bad = target.clone()
    bad[3, 4, 1] = 1.5
    with pytest.raises(ValueError, match="target"):
        M.lpips(pred, bad, w)
    bad = pred.clone()
    bad[5, 6, 2] = float("nan")
    with pytest.raises(ValueError, match="prediction"):
        M.lpips(bad, target, w)
    over = pred.clone()
    over[0, 0, 0] = 7.0                       # a prediction above 1 is clipped, not refused (eval_uncertainty.py:681)
    assert np.isfinite(M.lpips(over, target, w))


# ---- weights from a checkpoint ----------------------------------------------------------------------------------------

def _assert_same_tensors(w, sd, heads):
    for l, (name, shape) in enumerate(CK.LPIPS_CONVS):
        assert torch.equal(w.convs[l][0], sd[f"lpips.net.net.{name}.weight"]) and tuple(w.convs[l][0].shape) == shape
        assert torch.equal(w.convs[l][1], sd[f"lpips.net.net.{name}.bias"])
        head = f"lin{l}" if heads == "lin" else f"lins.{l}"
        assert torch.equal(w.lins[l], sd[f"lpips.net.{head}.model.1.weight"].reshape(-1))
        assert float(w.lins[l].min()) >= 0.0


@pytest.mark.parametrize("prefix", ["", "_model.", "module.", "_model.module."])
@pytest.mark.parametrize("heads", ["lin", "lins"])
def test_loader_returns_the_tensors_under_every_prefix_and_head_spelling(prefix, heads):
    sd = synthetic.make_lpips_weights(5, heads=heads)
    w = CK.lpips_weights_from_state_dict({prefix + k: v for k, v in sd.items()})
    _assert_same_tensors(w, sd, heads)
    assert torch.equal(w.shift, torch.tensor(CK.LPIPS_SHIFT)) and torch.equal(w.scale, torch.tensor(CK.LPIPS_SCALE))
    sd2 = dict(sd)
    sd2["lpips.net.scaling_layer.shift"] = torch.tensor([0.1, 0.2, 0.3]).view(1, 3, 1, 1)
    sd2["lpips.net.scaling_layer.scale"] = torch.tensor([0.5, 0.6, 0.7]).view(1, 3, 1, 1)
    w2 = CK.lpips_weights_from_state_dict(sd2)
    assert torch.equal(w2.shift, torch.tensor([0.1, 0.2, 0.3])) and torch.equal(w2.scale, torch.tensor([0.5, 0.6, 0.7]))


def test_partial_set_is_none_without_a_warning_and_a_wrong_shape_raises():
    sd = synthetic.make_lpips_weights(5)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert CK.lpips_weights_from_state_dict({"_model.lpips.net.lin0.model.1.weight": torch.zeros(1, 64, 1, 1)}) is None
        assert CK.lpips_weights_from_state_dict({"_model.field.x": torch.zeros(1)}) is None
        for drop in ("lpips.net.net.slice3.6.bias", "lpips.net.lin4.model.1.weight"):
            assert CK.lpips_weights_from_state_dict({k: v for k, v in sd.items() if k != drop}) is None
    bad = dict(sd)
    bad["lpips.net.net.slice2.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(RuntimeError, match=r"slice2\.3\.weight"):
        CK.lpips_weights_from_state_dict(bad)
    bad = dict(sd)
    bad["lpips.net.lin1.model.1.weight"] = torch.zeros(1, 64, 1, 1)
    with pytest.raises(RuntimeError, match=r"lin1\.model\.1\.weight"):
        CK.lpips_weights_from_state_dict(bad)


def _small_model(method):
    cfg = plugin.MODEL_CONFIGS[method]()
    if hasattr(cfg, "log2_hashmap_size"):
        cfg.log2_hashmap_size = 6
        cfg.implementation = "torch"
        cfg.proposal_net_args_list = [dict(a, log2_hashmap_size=5) for a in cfg.proposal_net_args_list]
        return cfg._target(cfg, num_train_data=3)
    return cfg._target(cfg, num_points=20)


@pytest.mark.parametrize("method", ["active-nerfacto", "nerfacto-mcdropout", "active-splatfacto"])
def test_models_adopt_the_weights_without_changing_their_state(method):
    src, dst = _small_model(method), _small_model(method)
    own = {"_model." + k: v for k, v in src.state_dict().items()}
    before_keys = list(dst.state_dict())
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        plain = dst.load_state_dict(dict(own), strict=True)
    assert dst.lpips_weights is None
    with pytest.raises(NotImplementedError, match=r"lpips\.net"):
        dst.lpips(torch.rand(1, 3, 32, 32), torch.rand(1, 3, 32, 32))
    lp = {"_model." + k: v for k, v in synthetic.make_lpips_weights(LC.WEIGHT_SEED).items()}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rep = dst.load_state_dict({**own, **lp}, strict=True)
    assert rep == plain and rep.unexpected_keys == []
    assert list(dst.state_dict()) == before_keys and not any("lpips" in k for k in before_keys)
    assert not any("lpips" in n for n, _ in list(dst.named_parameters()) + list(dst.named_buffers()))
    assert isinstance(dst.lpips_weights, CK.LpipsWeights)
    assert torch.equal(dst.lpips_weights.convs[0][0], LC.weights().convs[0][0])
    # model.lpips(image, rgb) on [1,3,H,W], as the eval script calls it
    pred, target = LC.image_pair(33, 36)
    pred = torch.clip(pred, max=1.0)
    got = dst.lpips(target.permute(2, 0, 1)[None], pred.permute(2, 0, 1)[None])
    assert got.dim() == 0 and got.dtype == torch.float64
    assert float(got) == M.lpips(pred, target, LC.weights())
    dst.set_lpips_weights(None)
    with pytest.raises(NotImplementedError):
        dst.lpips(target.permute(2, 0, 1)[None], pred.permute(2, 0, 1)[None])
    dst.set_lpips_weights(LC.weights())
    assert float(dst.lpips(target.permute(2, 0, 1)[None], pred.permute(2, 0, 1)[None])) == float(got)


# ---- the eval keys ----------------------------------------------------------------------------------------------------

def _fake_eval_set(n=2, H=33, W=40):
    g = torch.Generator().manual_seed(0)
    items = []
    for _ in range(n):
        gt = torch.rand(H, W, 3, generator=g)
        std = 0.02 + 0.1 * torch.rand(H, W, 1, generator=g)
        rgb = torch.clamp(gt + std * torch.randn(H, W, 3, generator=g), 0, 1.2)
        items.append(({"rgb": rgb, "rgb_std": std, "accumulation": torch.ones(H, W, 1)}, gt))
    return items


def test_image_metrics_unc_has_the_key_only_with_weights():
    (o, gt), = _fake_eval_set(1)
    without, curves0 = E.image_metrics_unc(o, gt)
    with_w, curves1 = E.image_metrics_unc(o, gt, lpips_weights=LC.weights())
    assert "lpips" not in without
    assert list(with_w)[:3] == ["psnr", "ssim", "lpips"]
    assert {k: v for k, v in with_w.items() if k != "lpips"} == without and set(curves0) == set(curves1)
    assert with_w["lpips"] == M.lpips(torch.clip(o["rgb"], max=1.0), gt, LC.weights())
    only, _ = E.image_metrics_unc(o, gt, eval_rgb_unc=False, lpips_weights=LC.weights())
    assert list(only) == ["psnr", "ssim", "lpips"]


class _StubModel:
    """what run_eval needs of a model: the per-camera callable and the weights its checkpoint brought"""

    def __init__(self, weights):
        self.lpips_weights = weights

    def get_outputs_for_camera(self, camera):
        return camera


def test_run_eval_writes_lpips_into_metrics_json(tmp_path):
    items = _fake_eval_set(2)
    cfg = E.ActiveNerfactoConfig(output_path=tmp_path / "with" / "metrics.json", eval_depth=False)
    got = E.run_eval(cfg, _StubModel(LC.weights()), items, method_name="active-nerfacto")
    per = [M.lpips(torch.clip(o["rgb"], max=1.0), gt, LC.weights()) for o, gt in items]
    assert abs(got["lpips"] - np.mean(per)) <= 1e-15
    d = json.loads((tmp_path / "with" / "metrics.json").read_text())
    assert d["results"]["lpips"] == got["lpips"] and list(d["results"])[:3] == ["psnr", "ssim", "lpips"]
    # a model without weights, and an explicit None, leave the key out; an explicit argument overrides the model's
    cfg2 = E.ActiveNerfactoConfig(output_path=tmp_path / "without" / "metrics.json", eval_depth=False)
    assert "lpips" not in E.run_eval(cfg2, _StubModel(None), items)
    assert "lpips" not in json.loads((tmp_path / "without" / "metrics.json").read_text())["results"]
    assert "lpips" not in E.run_eval(cfg2, _StubModel(LC.weights()), items, lpips_weights=None)
    other = LC.weights(seed=LC.WEIGHT_SEED + 1)
    over = E.run_eval(cfg2, _StubModel(LC.weights()), items, lpips_weights=other)
    assert abs(over["lpips"] - np.mean([M.lpips(torch.clip(o["rgb"], max=1.0), gt, other) for o, gt in items])) <= 1e-15
    # an ensemble: the first member's weights
    assert E.default_lpips_weights([_StubModel(other), _StubModel(None)]) is other
    avg, _ = E.get_average_uncertainty_metrics(_StubModel(LC.weights()).get_outputs_for_camera, items)
    assert avg["lpips"] == got["lpips"]


# ---- the C ABI --------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("unerf_lpips_pack", "unerf_conv2d_bias_relu", "unerf_maxpool3s2", "unerf_lpips_head", "unerf_lpips_workspace_bytes",
               "unerf_lpips_batch")


def test_new_symbols_are_exported_and_typed(lib):
    h = lib.load()
    for name in NEW_SYMBOLS:
        assert name in lib.SIGNATURES and getattr(h, name).argtypes == lib.SIGNATURES[name][1]
    assert h.unerf_version() == lib.ABI_VERSION == 1420
    text = open(os.path.join(ROOT, "include", "unerf.h")).read()
    for macro, value in (("UNERF_LPIPS_LAYERS", lib.LPIPS_LAYERS), ("UNERF_LPIPS_ROW", lib.LPIPS_ROW), ("UNERF_LPIPS_BAD_OFF", lib.LPIPS_BAD_OFF),
                         ("UNERF_LPIPS_MIN_SIDE", lib.LPIPS_MIN_SIDE), ("UNERF_LPIPS_CONV_TILE_M", lib.LPIPS_CONV_TILE_M),
                         ("UNERF_LPIPS_CONV_TILE_N", lib.LPIPS_CONV_TILE_N), ("UNERF_LPIPS_HEAD_PIXELS", lib.LPIPS_HEAD_PIXELS),
                         ("UNERF_LPIPS_CONV_STEP_K", lib.LPIPS_CONV_STEP_K), ("UNERF_LPIPS_EW_THREADS", lib.LPIPS_EW_THREADS),
                         ("UNERF_LPIPS_EW_MAX_WG", lib.LPIPS_EW_MAX_WG)):
        assert f"#define {macro} {value}" in text, macro
    assert lib.LPIPS_MIN_SIDE == M.LPIPS_MIN_SIDE and lib.LPIPS_LAYERS == M.LPIPS_LAYERS


def test_lpips_weights_struct_matches_the_header_layout(lib, tmp_path):
    """sizeof / offsetof of unerf_lpips_weights as a C compiler sees include/unerf.h, against lib.LpipsWeightsC"""
    cname, ct = "unerf_lpips_weights", lib.LpipsWeightsC
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "unerf.h"', 'int main(void) {',
             f'  printf("SIZEOF %zu\\n", sizeof({cname}));']
    lines += [f'  printf("{fname} %zu\\n", offsetof({cname}, {fname}));' for fname, _ in ct._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    rows = [r.split() for r in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()]
    assert len(rows) == len(ct._fields_) + 1
    for what, val in rows:
        assert (C.sizeof(ct) if what == "SIZEOF" else getattr(ct, what).offset) == int(val), what


def test_argument_refusals_come_before_any_launch(lib):
    """no GPU here: a refusal that reached a device call would report a HIP error (-2), not an argument error (-1)"""
    h = lib.load()
    w = lib.LpipsWeightsC()
    for l in range(lib.LPIPS_LAYERS):
        w.conv_w[l], w.conv_b[l], w.lin_w[l] = 256, 256, 256
    for c in range(3):
        w.shift[c], w.scale[c] = 0.0, 1.0
    need = h.unerf_lpips_workspace_bytes(31, 31, 1)
    assert need > 0 and h.unerf_lpips_workspace_bytes(30, 64, 1) == 0 and h.unerf_lpips_workspace_bytes(64, 64, 0) == 0
    assert h.unerf_lpips_workspace_bytes(31, 31, 2) > need
    assert h.unerf_lpips_batch(None, 256, 31, 31, 1, C.byref(w), 256, need, 256, None) == -1
    assert b"null pointer" in h.unerf_last_error()
    assert h.unerf_lpips_batch(256, 256, 30, 40, 1, C.byref(w), 256, need, 256, None) == -1
    assert b"30 x 40" in h.unerf_last_error() and b"31" in h.unerf_last_error()
    assert h.unerf_lpips_batch(256, 256, 40, 30, 1, C.byref(w), 256, need, 256, None) == -1
    assert h.unerf_lpips_batch(256, 256, 31, 31, 1, C.byref(w), 256, need - 1, 256, None) == -1
    assert b"workspace" in h.unerf_last_error()
    assert h.unerf_lpips_batch(256, 256, 31, 31, 0, C.byref(w), 256, need, 256, None) == -1
    assert h.unerf_lpips_batch(256, 256, 31, 31, lib.METRICS_MAX_IMAGES + 1, C.byref(w), 256, 1 << 40, 256, None) == -1
    w.lin_w[3] = None
    assert h.unerf_lpips_batch(256, 256, 31, 31, 1, C.byref(w), 256, need, 256, None) == -1
    assert b"layer 3" in h.unerf_last_error()
    # the two trunk kernels and the head
    assert h.unerf_conv2d_bias_relu(256, 256, 256, 256, 1, 8, 8, 3, 48, 3, 1, 1, 1, None) == -1
    assert b"column tile" in h.unerf_last_error()
    assert h.unerf_conv2d_bias_relu(None, 256, 256, 256, 1, 8, 8, 3, 64, 3, 1, 1, 1, None) == -1
    assert b"null pointer" in h.unerf_last_error()
    assert h.unerf_conv2d_bias_relu(256, 256, 256, 256, 1, 2, 2, 3, 64, 11, 4, 2, 1, None) == -1
    assert b"smaller than" in h.unerf_last_error()
    assert h.unerf_maxpool3s2(256, 256, 1, 2, 5, 64, None) == -1
    assert h.unerf_maxpool3s2(None, 256, 1, 5, 5, 64, None) == -1
    assert h.unerf_lpips_head(256, 256, 49, 64, 1, 256, 0, 256, 1, None) == -1
    assert b"workspace" in h.unerf_last_error()
    assert h.unerf_lpips_head(256, None, 49, 64, 1, 256, 8, 256, 1, None) == -1
    assert h.unerf_lpips_pack(256, 256, 0, 1, C.byref(w), 256, 256, None) == -1
    assert h.unerf_lpips_pack(256, None, 10, 1, C.byref(w), 256, 256, None) == -1


def test_ops_refuse_small_images_and_cpu_tensors(lib):
    from uncertainty_nerf_gs_amd import ops
    with pytest.raises(ValueError, match="31"):
        ops.lpips_batch(torch.rand(1, 30, 40, 3), torch.rand(1, 30, 40, 3), LC.weights())
    with pytest.raises(lib.UnerfError, match="HIP device"):
        ops.lpips_batch(torch.rand(1, 32, 40, 3), torch.rand(1, 32, 40, 3), LC.weights())
    row = np.zeros(lib.LPIPS_ROW)
    row[:5], row[5:10] = [1.0, 2.0, 3.0, 4.0, 5.0], [2.0, 2.0, 2.0, 2.0, 2.0]
    assert M.finish_lpips(row) == 7.5
    row[lib.LPIPS_BAD_OFF] = 3
    with pytest.raises(ValueError, match="3 values"):
        M.finish_lpips(row)


# ---- torchmetrics itself, where it exists -----------------------------------------------------------------------------

def test_host_definition_against_torchmetrics_on_its_own_weights():
    """Skipped wherever torchmetrics or its cached AlexNet weights are absent (as on the machines this build was made
    on): the module's own state dict through lpips_weights_from_state_dict and metrics.lpips, against the module."""
    pytest.importorskip("torchmetrics")
    pytest.importorskip("torchvision")
    hub = os.path.join(torch.hub.get_dir(), "checkpoints")
    if not (os.path.isdir(hub) and any(f.startswith("alexnet") for f in os.listdir(hub))):
        pytest.skip("torchvision's AlexNet weights are not cached")
    from torchmetrics.image.lpip import LearnedPerceptualImagePatchSimilarity
    module = LearnedPerceptualImagePatchSimilarity(net_type="alex", normalize=True).eval()
    w = CK.lpips_weights_from_state_dict({"lpips." + k: v for k, v in module.state_dict().items()})
    assert w is not None
    pred, target = LC.image_pair(64, 80)
    pred = torch.clip(pred, max=1.0)
    with torch.no_grad():
        want = float(module(pred.permute(2, 0, 1)[None], target.permute(2, 0, 1)[None]))
    assert abs(M.lpips(pred, target, w) - want) <= 1e-5 * max(abs(want), 1e-3)
