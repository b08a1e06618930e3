"""The batched ensemble aggregation without a GPU: the C ABI of unerf_ensemble_reduce (exported, argument checks before any
device call), ensemble.reduce_plan against ensemble.aggregate / _finish with a torch statement of the plan injected as
`reduce_fn`, and the collective plumbing of aggregate_distributed_batch over gloo.  The kernel itself is covered by
test_gpu_ensemble_batch.py."""
import ctypes as C
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT
from ensemble_cases import (golden_expected, golden_members, nerf_members, splat_members, torch_moments, torch_reduce)


# ---------------------------------------------------------------- C ABI ----------------

def _declared_arguments(symbol):
    text = open(os.path.join(ROOT, "include", "unerf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = re.search(r"\b%s\s*\((.*?)\)\s*;" % symbol, text, flags=re.S).group(1)
    return [a for a in args.split(",") if a.strip()]


def test_symbol_is_exported_with_the_bound_argument_count(lib):
    h = lib.load()
    assert getattr(h, "unerf_ensemble_reduce") is not None
    res, args = lib.SIGNATURES["unerf_ensemble_reduce"]
    assert res is C.c_int and len(args) == len(_declared_arguments("unerf_ensemble_reduce")) == 11
    assert h.unerf_version() == lib.ABI_VERSION == 1420
    assert (lib.ENS_MAX_KEYS, lib.ENS_MAX_MEMBERS, lib.ENS_MAX_CHANNELS, lib.NERF_MAX_VIEWS) == (32, 64, 64, 16)
    assert C.sizeof(lib.EnsKey) == 16 and C.sizeof(lib.EnsOut) == 24      # include/unerf.h: unerf_ens_key / unerf_ens_out


def _call(lib, B=2, M=3, keys=((3, 3, 10),), plan=((0, 0, -1, 0),), view_stride=None, table=1, arena=1, arena_floats=None,
          n_keys=None):
    """keys: (channels, stride, n); plan: (stat, key, aux, offset).  table / arena: fake non-null addresses -- every case
    here must be decided before anything dereferences them."""
    h = lib.load()
    kd = (lib.EnsKey * max(len(keys), 1))()
    for d, (c, s, n) in zip(kd, keys):
        d.channels, d.stride, d.n = c, s, n
    pd = (lib.EnsOut * max(len(plan), 1))()
    for d, (st, k, aux, off) in zip(pd, plan):
        d.stat, d.key, d.aux, d.offset = st, k, aux, off
    if view_stride is None:
        view_stride = max([off + keys[k][2] * (keys[k][0] if st <= 1 else 1) for st, k, _, off in plan
                           if 0 <= k < len(keys)] + [0])
    if arena_floats is None:
        arena_floats = max(B, 0) * view_stride
    rc = h.unerf_ensemble_reduce(table, B, len(keys) if n_keys is None else n_keys, M, kd, pd, len(plan), view_stride, arena,
                                 arena_floats, None)
    return rc, h.unerf_last_error()


def test_out_of_bound_arguments_fail_before_any_device_call(lib):
    """no GPU here and fake pointers: a call that got as far as a launch or a dereference would not return -1"""
    bad = lambda **kw: _call(lib, **kw)
    rc, msg = bad(B=lib.NERF_MAX_VIEWS + 1)
    assert rc == -1 and b"B=17" in msg
    assert bad(B=-1)[0] == -1
    rc, msg = bad(M=lib.ENS_MAX_MEMBERS + 1)
    assert rc == -1 and b"M=65" in msg
    assert bad(M=0)[0] == -1
    rc, msg = bad(keys=((3, 3, 10),) * 33, n_keys=33)
    assert rc == -1 and b"n_keys=33" in msg
    assert bad(n_keys=0)[0] == -1
    rc, msg = bad(keys=((lib.ENS_MAX_CHANNELS + 1, 65, 10),))
    assert rc == -1 and b"65 channels" in msg
    assert bad(keys=((0, 1, 10),))[0] == -1
    assert bad(keys=((3, 2, 10),))[0] == -1                                   # rows narrower than their channels
    assert bad(keys=((3, 3, -1),))[0] == -1
    rc, msg = bad(table=None)
    assert rc == -1 and b"null table" in msg
    assert bad(arena=None)[0] == -1
    # the plan: unknown statistic / key, a repeated (key, statistic), overlapping or overhanging blocks, a bad aux key
    assert bad(plan=((7, 0, -1, 0),))[0] == -1
    assert bad(plan=((0, 1, -1, 0),))[0] == -1
    rc, msg = bad(plan=((0, 0, -1, 0), (0, 0, -1, 30)))
    assert rc == -1 and b"repeats" in msg
    rc, msg = bad(plan=((0, 0, -1, 0), (1, 0, -1, 29)))
    assert rc == -1 and b"overlap" in msg
    assert bad(plan=((0, 0, -1, 0),), view_stride=29)[0] == -1
    assert bad(plan=((0, 0, -1, -1),))[0] == -1
    assert bad(arena_floats=59)[0] == -1                                      # 2 views x 30 floats
    assert bad(plan=((lib.ENS_EPI_ALEA, 0, -1, 0),))[0] == -1                 # alea statistics need their aux key
    assert bad(keys=((3, 3, 10), (1, 1, 9)), plan=((lib.ENS_ALEA_CMEAN, 0, 1, 0),))[0] == -1   # ... with as many elements


def test_nothing_to_reduce_is_a_successful_no_op(lib):
    assert _call(lib, B=0, table=None, arena=None)[0] == 0
    assert _call(lib, keys=((3, 3, 0),), table=None, arena=None)[0] == 0
    assert _call(lib, plan=(), table=None, arena=None)[0] == 0
    # the bounds themselves are inside
    assert _call(lib, B=16, M=64, keys=((64, 64, 0),) * 32, plan=(), table=None, arena=None)[0] == 0


# ------------------------------------------------------- reduce_plan -------------------

def _views_of(members_per_view):
    """[view][member] dicts -> the per_member_views argument of aggregate_batch ([member][view])"""
    return [[members_per_view[v][j] for v in range(len(members_per_view))] for j in range(len(members_per_view[0]))]


def _assert_same(got, ref, msg=""):
    assert list(got) == list(ref), (msg, list(got), list(ref))                # key set AND key order
    for k in ref:
        assert got[k].shape == ref[k].shape and torch.equal(got[k], ref[k]), (msg, k)


@pytest.mark.parametrize("case", ["alea", "plain", "splat"])
def test_plan_and_torch_reduce_equal_aggregate(case):
    from uncertainty_nerf_gs_amd import ensemble
    if case == "splat":
        per_view = [splat_members(), splat_members(seed=5)]
    else:
        per_view = [golden_members(case, 5), golden_members(case, 4), golden_members(case, 5)[::-1]]
        per_view[1] = per_view[1] + per_view[1][:1]                           # one member count per batch
    got = ensemble.aggregate_batch(_views_of(per_view), reduce_fn=torch_reduce)
    assert len(got) == len(per_view)
    for v, members in enumerate(per_view):
        _assert_same(got[v], ensemble.aggregate(members, moments_fn=torch_moments), (case, v))


def test_plan_states_the_order_dependence_of_the_key_loop():
    from uncertainty_nerf_gs_amd import ensemble
    keys = ["rgb", "accumulation", "depth", "rgb_var", "rgb_std", "depth_var", "depth_std"]
    plan = ensemble.reduce_plan(keys)
    # rgb_var / rgb_std are written while "rgb" is visited and keep that position, but the member means overwrite them
    assert plan == [("rgb", "mean", "rgb"), ("rgb_var_alea", "alea_cmean", "rgb"), ("rgb_var_epi", "var_cmean", "rgb"),
                    ("rgb_var", "mean", "rgb_var"), ("rgb_std", "mean", "rgb_std"), ("accumulation", "mean", "accumulation"),
                    ("depth", "mean", "depth"), ("depth_var_alea", "alea_cmean", "depth"), ("depth_var_epi", "var_cmean", "depth"),
                    ("depth_var", "mean", "depth_var"), ("depth_std", "mean", "depth_std")]
    # members that emit the variance keys BEFORE rgb / depth: the combined values survive
    early = ensemble.reduce_plan(["rgb_var", "rgb_std", "depth_var", "depth_std", "rgb", "depth"])
    assert dict((n, (s, k)) for n, s, k in early)["rgb_var"] == ("epi_plus_alea", "rgb")
    assert dict((n, (s, k)) for n, s, k in early)["depth_std"] == ("sqrt_epi_plus_alea", "depth")
    assert ensemble.reduce_plan(["rgb", "depth", "expected_depth", "accumulation"]) == [
        ("rgb", "mean", "rgb"), ("rgb_std", "std_cmean", "rgb"), ("depth", "mean", "depth"), ("depth_std", "std_cmean", "depth"),
        ("expected_depth", "mean", "expected_depth"), ("expected_depth_std", "std_cmean", "expected_depth"),
        ("accumulation", "mean", "accumulation")]
    with pytest.raises(KeyError):       # _finish fails the same way: rgb_std and depth_std but no rgb_var to average
        ensemble.reduce_plan(["rgb", "rgb_std", "depth_std"])


def test_early_variance_keys_equal_aggregate():
    """the other branch of the order dependence, on values: *_var / *_std keep the combined epistemic + aleatoric terms"""
    from uncertainty_nerf_gs_amd import ensemble
    order = ["rgb_var", "rgb_std", "depth_var", "depth_std", "rgb", "depth", "accumulation"]
    per_view = [[{k: m[k] for k in order} for m in nerf_members("alea", 3, 4, 5, seed=s)] for s in (1, 2)]
    got = ensemble.aggregate_batch(_views_of(per_view), reduce_fn=torch_reduce)
    for v, members in enumerate(per_view):
        ref = ensemble.aggregate(members, moments_fn=torch_moments)
        _assert_same(got[v], ref, v)
        assert not torch.equal(ref["rgb_var"], torch.stack([m["rgb_var"] for m in members]).mean(0).mean(-1, keepdim=True))


@pytest.mark.parametrize("tag", ["plain", "alea"])
def test_five_members_match_the_reference_recording(tag):
    """M = 5 == the reference EnsemblePipeline output recorded in the fixture, at test_distributed_cpu.py's tolerance"""
    from uncertainty_nerf_gs_amd import ensemble
    members = golden_members(tag, 5)
    out = ensemble.aggregate_batch([[m] for m in members], reduce_fn=torch_reduce)[0]
    expect = golden_expected(tag)
    assert set(out) == set(expect)
    for k, v in expect.items():
        np.testing.assert_allclose(out[k].numpy(), v, rtol=1e-6, atol=1e-7, err_msg=k)


def test_views_are_chunked_by_the_abi_bound():
    from uncertainty_nerf_gs_amd import ensemble, lib
    B = 2 * lib.NERF_MAX_VIEWS + 3
    per_view = [nerf_members("plain", 2, 2, 3, seed=v) for v in range(B)]
    sizes = []

    def counting(views, plan):
        sizes.append(len(views))
        return torch_reduce(views, plan)

    got = ensemble.aggregate_batch(_views_of(per_view), reduce_fn=counting)
    assert sizes == [16, 16, 3] and len(got) == B
    for v in (0, 15, 16, B - 1):
        _assert_same(got[v], ensemble.aggregate(per_view[v], moments_fn=torch_moments), v)
    assert ensemble.aggregate_batch([[], []], reduce_fn=counting) == []


class _FakeMember:
    def __init__(self, views):
        self.views = views

    def get_outputs_for_camera(self, camera):
        return self.views[camera]

    def get_outputs_for_cameras(self, cameras, max_views=16):
        return [self.views[c] for c in cameras]


def test_fused_pipeline_equals_the_per_view_pipeline():
    from uncertainty_nerf_gs_amd import ensemble
    per_view = [nerf_members("alea", 3, 4, 5, seed=v) for v in range(3)]
    fakes = [_FakeMember(vs) for vs in _views_of(per_view)]
    loop = ensemble.EnsemblePipeline(fakes, moments_fn=torch_moments)
    fused = ensemble.EnsemblePipeline(fakes, fused=True, reduce_fn=torch_reduce)
    assert not loop.fused and fused.fused
    a, b = loop.get_ensemble_outputs_for_cameras([0, 1, 2]), fused.get_ensemble_outputs_for_cameras([0, 1, 2])
    for v in range(3):
        _assert_same(b[v], a[v], v)
    _assert_same(fused.get_ensemble_outputs_for_camera_ray_bundle(1), loop.get_ensemble_outputs_for_camera_ray_bundle(1))
    with pytest.raises(AssertionError, match="at least two"):
        ensemble.EnsemblePipeline(fakes[:1], fused=True, reduce_fn=torch_reduce).get_ensemble_outputs_for_cameras([0])


# ------------------------------------------------------- gloo ---------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


H, W, B = 5, 7, 3          # 35 pixels: divisible by neither 2 nor 3 ranks


def _dist_members(kind, total):
    """[view][member] for the whole ensemble; every rank builds the same and takes its own members"""
    if kind == "splat":
        return [splat_members(M=total, H=H, W=W, seed=10 + v) for v in range(B)]
    return [nerf_members(kind, total, H, W, seed=20 + v) for v in range(B)]


def _batch_worker(rank, world, port, kind, per_rank, ret):
    import torch.distributed as dist
    from uncertainty_nerf_gs_amd import ensemble
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    per_view = _dist_members(kind, world * per_rank)
    mine = [[per_view[v][rank * per_rank + j] for v in range(B)] for j in range(per_rank)]      # rank-major member order
    loop = [ensemble.aggregate_distributed([pm[v] for pm in mine], moments_fn=torch_moments) for v in range(B)]
    calls = {"all_to_all_single": [], "all_gather": []}
    real = {name: getattr(dist, name) for name in calls}

    def counted(name):
        def fn(*args, **kw):
            calls[name].append(args[1].numel())         # elements this rank puts in
            return real[name](*args, **kw)
        return fn

    for name in calls:
        setattr(dist, name, counted(name))
    try:
        stages = {}
        got = ensemble.aggregate_distributed_batch(mine, reduce_fn=torch_reduce, stage_ms=stages)
    finally:
        for name in calls:
            setattr(dist, name, real[name])
    same = len(got) == B and all(list(got[v]) == list(loop[v]) and all(
        got[v][k].shape == loop[v][k].shape and torch.equal(got[v][k], loop[v][k]) for k in loop[v]) for v in range(B))
    ret[rank] = {"same": same, "calls": {k: list(v) for k, v in calls.items()}, "stages": dict(stages),
                 "out": {k: t.numpy() for k, t in got[B - 1].items()}}
    dist.destroy_process_group()


@pytest.mark.parametrize("world,kind,per_rank", [(2, "alea", 1), (3, "alea", 1), (2, "plain", 2), (3, "plain", 1),
                                                 (2, "splat", 1), (3, "splat", 1)])
def test_distributed_batch_equals_per_view_distributed(world, kind, per_rank):
    from uncertainty_nerf_gs_amd import ensemble
    per_view = _dist_members(kind, world * per_rank)
    single = ensemble.aggregate(per_view[B - 1], moments_fn=torch_moments)
    ctot = sum(t.shape[-1] for t in per_view[0][0].values() if t.dim() == 3)
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_batch_worker, args=(world, _free_port(), kind, per_rank, ret), nprocs=world, join=True)
        assert set(ret.keys()) == set(range(world))
        for r in range(world):
            assert ret[r]["same"], r
            # ONE image exchange and ONE image gather for the whole batch (splat members: one more gather, of the
            # few floats of the non-image keys of all views)
            calls = ret[r]["calls"]
            assert calls["all_to_all_single"] == [per_rank * B * H * W * ctot]
            small = [per_rank * B * 3] if kind == "splat" else []
            rows = -(-H * W // world)
            assert len(calls["all_gather"]) == 1 + len(small)
            assert sorted(calls["all_gather"])[:len(small)] == small and max(calls["all_gather"]) % (rows * B) == 0
            assert ret[r]["stages"]["packed_image_bytes_per_member"] == H * W * ctot * 4
            # ... and the single-process aggregation of the same members, as test_distributed_cpu.py pins the per-view path
            assert list(ret[r]["out"]) == list(single)
            for k, v in single.items():
                assert np.array_equal(ret[r]["out"][k], v.numpy()), (r, k)
