"""The fused ensemble reduce on the GPU (unerf_ensemble_reduce, ensemble.aggregate_batch / aggregate_distributed_batch,
EnsemblePipeline(fused=True)): member moments bit-equal to unerf_moments of the stacked inputs, derived keys against a
float64 evaluation of their formulas and against ensemble.aggregate, the reference's recorded ensemble output, the
pipeline surface and the RCCL path at world size 1."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from ensemble_cases import golden_expected, golden_members, torch_moments

pytestmark = pytest.mark.gpu

FILL = 0x7FC12345          # a NaN with a payload no arithmetic produces: what the arena holds where nothing was written
U = 2.0 ** -24             # unit roundoff of float32


def _bits(t):
    return t.contiguous().view(torch.int32)


def _reduce(lib, views, plan, gap=5, tail=64):
    """unerf_ensemble_reduce through the C ABI.  views[v][key] = the M sources [n, C] (row stride free, unit channel stride);
    plan = (output name, lib.ENS_* statistic, key, aux key or None).  Every block is preceded by `gap` floats nothing may
    touch, the arena ends in `tail` more; it is pre-filled with FILL.  Returns per view {name: [n, C_out]} and checks that
    every float outside the blocks still holds FILL."""
    h = lib.load()
    names = list(views[0])
    first = {k: views[0][k][0] for k in names}
    dev = first[names[0]].device
    B, M = len(views), len(views[0][names[0]])
    keys = (lib.EnsKey * len(names))()
    for d, k in zip(keys, names):
        d.channels, d.n = first[k].shape[1], first[k].shape[0]
        d.stride = first[k].stride(0) if first[k].shape[0] > 1 else first[k].shape[1]
    ptrs = []
    for vw in views:
        for d, k in zip(keys, names):
            for t in vw[k]:
                assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (d.n, d.channels)
                assert (d.channels == 1 or t.stride(1) == 1) and (d.n <= 1 or t.stride(0) == d.stride)
                ptrs.append(t.data_ptr())
    outs = (lib.EnsOut * len(plan))()
    blocks, off = [], 0
    for e, (name, stat, key, aux) in zip(outs, plan):
        d = keys[names.index(key)]
        cout = d.channels if stat in (lib.ENS_MEAN, lib.ENS_VAR) else 1
        off += gap
        e.stat, e.key, e.aux, e.offset = stat, names.index(key), (-1 if aux is None else names.index(aux)), off
        blocks.append((name, off, d.n, cout))
        off += d.n * cout
    stride = off + gap
    arena = torch.full((B * stride + tail,), FILL, dtype=torch.int32, device=dev).view(torch.float32)
    table = torch.tensor(ptrs, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = h.unerf_ensemble_reduce(table.data_ptr(), B, len(names), M, keys, outs, len(plan), stride, arena.data_ptr(),
                                     arena.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, h.unerf_last_error()
    torch.cuda.current_stream().synchronize()
    untouched = torch.ones(arena.numel(), dtype=torch.bool, device=dev)
    res = []
    for v in range(B):
        res.append({})
        for name, o, n, c in blocks:
            untouched[v * stride + o:v * stride + o + n * c] = False
            res[v][name] = arena[v * stride + o:v * stride + o + n * c].view(n, c)
    assert bool((_bits(arena)[untouched] == FILL).all()), "a float outside the planned blocks was written"
    return res


def _moments_plan(lib, names):
    return [(k + s, code, k, None) for k in names for s, code in (("/mean", lib.ENS_MEAN), ("/var", lib.ENS_VAR))]


def _assert_moments(lib, views, got):
    """every mean / variance block against unerf_moments of the stacked inputs, bit for bit (the NaN of M = 1 included)"""
    from uncertainty_nerf_gs_amd import ops
    for v, view in enumerate(views):
        for k, srcs in view.items():
            mean, var = ops.moments(torch.stack(list(srcs), dim=0).contiguous())
            assert torch.equal(_bits(got[v][k + "/mean"]), _bits(mean)), (v, k, "mean")
            assert torch.equal(_bits(got[v][k + "/var"]), _bits(var)), (v, k, "var")
            assert not bool((_bits(got[v][k + "/var"]) == FILL).any())
            if len(srcs) == 1:
                assert bool(got[v][k + "/var"].isnan().all())
            else:
                assert bool(got[v][k + "/var"].isfinite().all())


@pytest.mark.parametrize("M", [1, 2, 5, 64])
def test_moments_equal_unerf_moments_bit_for_bit(lib, dev, M):
    """n around the 256-thread block, one to sixteen views, channel counts that take the 1-, 3- and 4-channel groups
    (C = 48: twelve groups of four); M = 5 and 64 pass through the tail and the body of the eight-source load groups"""
    g = torch.Generator().manual_seed(100 + M)
    pool = torch.rand(16 * M * 257 * 48, generator=g).to(dev)
    for n in (1, 35, 255, 256, 257):
        for B in (1, 3, 16):
            for Cc in (1, 3, 48):
                x = pool[: B * M * n * Cc].view(B, M, n, Cc)
                views = [{"x": [x[v, j] for j in range(M)]} for v in range(B)]
                _assert_moments(lib, views, _reduce(lib, views, _moments_plan(lib, ["x"])))


@pytest.mark.parametrize("side_stream", [False, True])
def test_strided_sources_and_a_mixed_key_set(lib, dev, side_stream):
    """sources read in place: channel slices of [n,8] rows (stride 8, channel offsets 4 and 3), next to a contiguous
    48-channel key, a 7-channel key (a group of four, then a group of three) and two non-image keys of one element"""
    g = torch.Generator().manual_seed(7)
    n, M, B = 257, 5, 3
    rows = torch.rand(B, M, n, 8, generator=g).to(dev)
    wide = torch.rand(B, M, n, 48, generator=g).to(dev)
    seven = torch.rand(B, M, n, 7, generator=g).to(dev)
    bg = torch.rand(B, M, 1, 3, generator=g).to(dev)
    one = torch.rand(B, M, 1, 1, generator=g).to(dev)
    views = [{"background": [bg[v, j] for j in range(M)], "rgb": [rows[v, j, :, 4:7] for j in range(M)],
              "acc": [rows[v, j, :, 3:4] for j in range(M)], "one": [one[v, j] for j in range(M)],
              "wide": [wide[v, j] for j in range(M)], "seven": [seven[v, j] for j in range(M)]} for v in range(B)]
    assert views[0]["rgb"][0].stride() == (8, 1) and not views[0]["rgb"][0].is_contiguous()
    if side_stream:
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            got = _reduce(lib, views, _moments_plan(lib, list(views[0])))
    else:
        got = _reduce(lib, views, _moments_plan(lib, list(views[0])))
    _assert_moments(lib, views, got)


def test_keys_nothing_is_asked_of_and_empty_keys_are_passed_over(lib, dev):
    g = torch.Generator().manual_seed(9)
    x = torch.rand(2, 3, 300, 3, generator=g).to(dev)
    views = [{"skipped": [x[v, j, :, :1] for j in range(3)], "empty": [x[v, j, :0] for j in range(3)],
              "x": [x[v, j] for j in range(3)]} for v in range(2)]
    plan = _moments_plan(lib, ["x"]) + [("empty/mean", lib.ENS_MEAN, "empty", None)]
    got = _reduce(lib, views, plan)
    _assert_moments(lib, [{"x": vw["x"]} for vw in views], got)
    assert got[0]["empty/mean"].shape == (0, 3)


# ------------------------------------------------------- derived keys -------------------

def _uniform(g, *shape):
    """uniform in [0.05, 1]: every member variance is a normal float well above zero"""
    return 0.05 + 0.95 * torch.rand(*shape, generator=g)


ALEA_ORDER = ["rgb", "accumulation", "depth", "rgb_var", "rgb_std", "depth_var", "depth_std"]
EARLY_ORDER = ["rgb_var", "rgb_std", "depth_var", "depth_std", "rgb", "depth", "accumulation"]
PLAIN_ORDER = ["rgb", "accumulation", "depth", "expected_depth"]
WIDTH = {"rgb": 3, "rgb_var": 3}       # a 3-channel rgb_var: the aleatoric channel mean has something to average


def _members(dev, order, M, Hh, Ww, seed):
    g = torch.Generator().manual_seed(seed)
    return [{k: _uniform(g, Hh, Ww, WIDTH.get(k, 1)).to(dev) for k in order} for _ in range(M)]


def _rel(a, b):
    a, b = a.double(), b.double()
    return float(((a - b).abs() / b.abs()).max())


@pytest.mark.parametrize("order", [ALEA_ORDER, EARLY_ORDER, PLAIN_ORDER], ids=["alea", "early", "plain"])
def test_derived_keys_against_float64_and_aggregate(lib, dev, order):
    """each derived value against (a) a float64 evaluation of its formula from the kernel's OWN fp32 mean / variance, within
    4 x 2^-24 relative -- at most three roundings for a channel mean of three (two additions, one division), one for the
    addition, one for the square root, which halves the error it is handed; every operand is positive, so relative errors
    do not grow -- and (b) ensemble.aggregate on the same tensors within 2^-20 (torch's channel mean may multiply by a
    rounded reciprocal).  No element is left out of either comparison."""
    from uncertainty_nerf_gs_amd import ensemble, ops
    M, B, Hh, Ww = 5, 3, 9, 31                   # 279 pixels: two blocks, the second partly filled
    per_view = [_members(dev, order, M, Hh, Ww, seed=40 + v) for v in range(B)]
    plan = ensemble.reduce_plan(order)
    stats = {s for _, s, _ in plan}
    assert stats == ({"mean", "std_cmean"} if order is PLAIN_ORDER else
                     {"mean", "alea_cmean", "var_cmean", "epi_plus_alea", "sqrt_epi_plus_alea"} if order is EARLY_ORDER else
                     {"mean", "alea_cmean", "var_cmean"})
    # the kernel's own moments ride along as extra outputs of the same launch (a member mean the plan already holds is
    # read from there: a (key, statistic) pair goes into one block)
    planned = {k: n for n, s, k in plan if s == "mean"}
    extra = [(k + "/var", "var", k) for k in order] + [(k + "/mean", "mean", k) for k in order if k not in planned]
    views = [{k: [m[k].reshape(-1, m[k].shape[-1]) for m in members] for k in order} for members in per_view]
    got = ops.ensemble_reduce(views, plan + extra)
    torch.cuda.synchronize()
    for v, members in enumerate(per_view):
        ref = ensemble.aggregate(members)        # HIP moments + the torch key loop
        assert [n for n, _, _ in plan] == list(ref)
        mean = {k: got[v][planned.get(k, k + "/mean")].double() for k in order}
        var = {k: got[v][k + "/var"].double() for k in order}
        assert all(bool((var[k] > 1e-6).all()) for k in order)
        cmean = lambda t: t.sum(dim=-1, keepdim=True) / t.shape[-1]
        f64 = {"var_cmean": lambda k: cmean(var[k]), "alea_cmean": lambda k: cmean(mean[k + "_var"]),
               "epi_plus_alea": lambda k: cmean(var[k]) + cmean(mean[k + "_var"]),
               "sqrt_epi_plus_alea": lambda k: (cmean(var[k]) + cmean(mean[k + "_var"])).sqrt(),
               "std_cmean": lambda k: cmean(var[k].sqrt())}
        for name, stat, k in plan:
            out = got[v][name]
            assert out.shape == ref[name].reshape(out.shape[0], -1).shape
            if stat == "mean":
                assert torch.equal(out, ref[name].reshape(out.shape)), (v, name)
                continue
            a, b = _rel(out, f64[stat](k)), _rel(out, ref[name].reshape(out.shape))
            print(f"view {v} {name} ({stat}): rel. to float64 {a / U:.3f} x 2^-24, rel. to aggregate {b / U:.3f} x 2^-24")
            assert a <= 4 * U, (v, name, a)
            assert b <= 2.0 ** -20, (v, name, b)


# ------------------------------------------------- fixture and pipeline -----------------

@pytest.mark.parametrize("tag", ["plain", "alea"])
def test_five_members_match_the_reference_recording(dev, tag):
    """M = 5 against the REFERENCE's EnsemblePipeline output (tests/golden/ensemble.npz), at the tolerance
    test_distributed_cpu.py / test_gpu_distributed.py use for it; two views, the second with the members reversed"""
    from uncertainty_nerf_gs_amd import ensemble
    members = [{k: v.to(dev) for k, v in m.items()} for m in golden_members(tag, 5)]
    got = ensemble.aggregate_batch([[m, r] for m, r in zip(members, members[::-1])])
    torch.cuda.synchronize()
    expect = golden_expected(tag)
    loop = ensemble.aggregate(members)
    for out in got:
        assert set(out) == set(expect) and list(out) == list(loop)
        for k, v in expect.items():
            np.testing.assert_allclose(out[k].cpu().numpy(), v, rtol=1e-6, atol=1e-7, err_msg=k)


def _nerf_member(dev, seed):
    from uncertainty_nerf_gs_amd import plugin, synthetic
    import test_gpu_models as TM
    cfg = TM._small_cfg(plugin.MODEL_CONFIGS["active-nerfacto"]())
    model = cfg._target(cfg, num_train_data=4)
    model.load_state_dict(TM._state_dict_from_tensors(synthetic.make_scene_tensors(seed=seed, kind="active", log2T=14, prop_log2T=12),
                                                      "active"))
    model.rays_per_launch = 2560
    return model.to(dev)


def _launch_names(fn):
    from uncertainty_nerf_gs_amd import ops
    ops.TIMER = ops.KernelTimer()
    try:
        out = fn()
        names = {k: v["launches"] for k, v in ops.TIMER.summary().items()}
    finally:
        ops.TIMER = None
    return out, names


def test_fused_pipeline_on_two_nerfacto_members(dev):
    """EnsemblePipeline(fused=True).get_ensemble_outputs_for_cameras, 3 views of 24 x 32, against fused=False: the keys in
    the same order, every member mean bit-equal, the derived keys within 2^-20 -- in ONE ensemble_reduce launch and without
    a moments launch.  The members hand out channel slices of their [R,8] composite rows: read where they lie."""
    from uncertainty_nerf_gs_amd import ensemble
    import test_gpu_nerf_view_batch as VB
    members = [_nerf_member(dev, 5), _nerf_member(dev, 6)]
    batch, singles = VB._cameras(3, h=24, w=32)
    with torch.cuda.device(dev):
        want, loop_launches = _launch_names(lambda: ensemble.EnsemblePipeline(members).get_ensemble_outputs_for_cameras(batch))
        got, launches = _launch_names(lambda: ensemble.EnsemblePipeline(members, fused=True).get_ensemble_outputs_for_cameras(batch))
        one = ensemble.EnsemblePipeline(members, fused=True).get_ensemble_outputs_for_camera_ray_bundle(singles[1])
        torch.cuda.synchronize()
    assert launches.get("ensemble_reduce") == 1 and "moments" not in launches, launches
    assert loop_launches.get("moments", 0) >= 3 and "ensemble_reduce" not in loop_launches, loop_launches
    plan = ensemble.reduce_plan([k for k, t in members[0].get_outputs_for_camera(singles[0]).items() if torch.is_tensor(t)])
    assert len(got) == 3
    for v in range(3):
        assert list(got[v]) == list(want[v]) == [n for n, _, _ in plan]
        for name, stat, _ in plan:
            a, b = got[v][name], want[v][name]
            assert a.shape == b.shape == (24, 32, a.shape[-1])
            if stat == "mean":
                assert torch.equal(a, b), (v, name)
            else:
                assert bool(((a - b).abs() <= 2.0 ** -20 * b.abs()).all()), (v, name)
    assert float(got[0]["rgb_var_epi"].max()) > 0
    for name in one:
        assert torch.equal(one[name], got[1][name]), name


# ------------------------------------------------------- RCCL ---------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rccl_worker(rank, world, port, tag, ret):
    """world size 1: all five members on the one GPU; world size 2: one member per GPU.  The collectives of the batched
    path on device tensors, the fused reduce reading the receive buffer in place.  Two views, the second with other values."""
    import torch.distributed as dist
    from uncertainty_nerf_gs_amd import ensemble, lib
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    lib.build_library()
    torch.cuda.set_device(rank)
    dev = torch.device("cuda", rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    members = golden_members(tag, 5 if world == 1 else world)
    mine = members if world == 1 else members[rank:rank + 1]
    mine = [[{k: v.to(dev) for k, v in m.items()}, {k: (v * 0.5 + 0.125).to(dev) for k, v in m.items()}] for m in mine]
    stages = {}
    got = ensemble.aggregate_distributed_batch(mine, stage_ms=stages)
    loop = [ensemble.aggregate_distributed([pm[v] for pm in mine]) for v in range(2)]
    torch.cuda.synchronize()
    ret[rank] = {"got": [{k: t.cpu().numpy() for k, t in o.items()} for o in got],
                 "loop": [{k: t.cpu().numpy() for k, t in o.items()} for o in loop], "stages": dict(stages)}
    dist.destroy_process_group()


def _check_rccl(ret, world, tag):
    from uncertainty_nerf_gs_amd import ensemble
    plan = {n: s for n, s, _ in ensemble.reduce_plan(list(golden_members(tag, 1)[0]))}
    for r in range(world):
        got, loop = ret[r]["got"], ret[r]["loop"]
        assert {"pack", "all_to_all", "moments", "all_gather", "unpack", "calls"} <= set(ret[r]["stages"])
        for v in range(2):
            assert list(got[v]) == list(loop[v]) == list(plan)
            for k, stat in plan.items():
                if stat == "mean":
                    assert np.array_equal(got[v][k], loop[v][k]), (r, v, k)
                else:
                    assert np.all(np.abs(got[v][k] - loop[v][k]) <= 2.0 ** -20 * np.abs(loop[v][k])), (r, v, k)
                assert np.array_equal(got[v][k], ret[0]["got"][v][k]), f"ranks disagree on {k}"


@pytest.mark.parametrize("tag", ["plain", "alea"])
def test_distributed_batch_over_rccl_on_one_gpu(tag):
    if torch.cuda.device_count() < 1:
        pytest.skip("needs a GPU")
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_rccl_worker, args=(1, _free_port(), tag, ret), nprocs=1, join=True)
        _check_rccl(ret, 1, tag)
        expect = golden_expected(tag)
        assert set(ret[0]["got"][0]) == set(expect)
        for k, v in expect.items():
            np.testing.assert_allclose(ret[0]["got"][0][k], v, rtol=1e-6, atol=1e-7, err_msg=k)


@pytest.mark.parametrize("tag", ["plain", "alea"])
def test_distributed_batch_one_member_per_gpu(tag):
    if torch.cuda.device_count() < 2:          # device_count() does not initialise the GPU in this process
        pytest.skip("needs >= 2 GPUs (one ensemble member per GPU)")
    from uncertainty_nerf_gs_amd import ensemble
    single = ensemble.aggregate(golden_members(tag, 2), moments_fn=torch_moments)
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_rccl_worker, args=(2, _free_port(), tag, ret), nprocs=2, join=True)
        _check_rccl(ret, 2, tag)
        for r in range(2):
            for k, v in single.items():
                np.testing.assert_allclose(ret[r]["got"][0][k], v.numpy(), rtol=1e-6, atol=1e-7, err_msg=f"rank {r}: {k}")
