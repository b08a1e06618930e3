"""Ensemble aggregation (models/ensemble/ensemble_pipeline.py:144-191), single- and multi-GPU.

The reference renders its M members sequentially on one device and then does
`torch.stack(...).mean(0) / .var(0) / .std(0)` per output key.  Here:

  * `aggregate(outputs_list)`        -- members already on one device: the stack/mean/var is the
                                        `unerf_moments` kernel (two-pass fp32, like torch).
  * `aggregate_distributed(outputs)` -- ONE MEMBER PER RANK (one process per GPU, RCCL over xGMI):
    every rank renders the same camera with its own member, then the per-pixel moments are formed
    with the exact two-pass formula on a pixel slice per rank:
        all_to_all(pixel slices of the member images)  ->  rank g reduces its rows  ->  all_gather(reduced slices)
    This is SURVEY.md 8(e) option A (exact parity with torch.stack(...).var(0); no E[x^2]-E[x]^2
    cancellation).  Payload per GPU at 1080p, 6 floats per pixel: 7/8 x 50 MB sent and received in the exchange,
    every xGMI link carrying 1/8 of an image at once (point-to-point, not ring-bound), then 7/8 x 100 MB of
    reduced slices gathered -- well under a millisecond each at ~150 GB/s per link, next to a ~110 ms member render.

  * `aggregate_batch(per_member_views)` / `aggregate_distributed_batch(per_member_views)` -- the same for B views at once:
    `reduce_plan` states the key loop once on the host, and ONE `unerf_ensemble_reduce` launch forms the member moments and
    every derived key of all views, reading the members' tensors (or the exchange's receive buffer) where they lie.

The moment math is injected (`moments_fn`, and `reduce_fn` for the batched forms) so that the collective plumbing can be
tested with world_size=2 on the gloo backend without a GPU; the default is the HIP kernel.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

MomentsFn = Callable[[torch.Tensor], Tuple[torch.Tensor, torch.Tensor]]  # [K,N,C] -> mean [N,C], var [N,C]
Plan = List[Tuple[str, str, str]]                                        # (output key, statistic, input key)
# (views[v][input key] = the M members' [n, C] tensors, plan) -> per view {output key: [n, C_out]}
ReduceFn = Callable[[List[Dict[str, List[torch.Tensor]]], Plan], List[Dict[str, torch.Tensor]]]


def _hip_moments(x: torch.Tensor):
    from . import ops
    return ops.moments(x.contiguous())


def _finish(keys: Sequence[str], mean: Dict[str, torch.Tensor], var: Dict[str, torch.Tensor],
            alea: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The key loop of ensemble_pipeline.py:159-189, in the members' key order.  Order matters and is
    kept: the reference writes outputs[k] = mean for EVERY member key in sequence, so when members
    themselves emit rgb_var / rgb_std / depth_var / depth_std after rgb / depth (the active-nerfacto
    order, activenerfacto_model.py:117-127) the combined epistemic+aleatoric values written while
    visiting "rgb"/"depth" are subsequently overwritten by the member means of those keys; only the
    *_var_alea / *_var_epi keys survive.  Reproduced as is (parity), flagged in DESIGN.md."""
    out: Dict[str, torch.Tensor] = {}
    has_std = "rgb_std" in keys and "depth_std" in keys
    for k in keys:
        out[k] = mean[k]
        if has_std:
            if k in ("rgb", "depth"):
                out[k + "_var_alea"] = alea[k].mean(dim=-1).unsqueeze(-1)
                out[k + "_var_epi"] = var[k].mean(dim=-1).unsqueeze(-1)
                out[k + "_var"] = out[k + "_var_epi"] + out[k + "_var_alea"]
                out[k + "_std"] = out[k + "_var"].sqrt()
        elif k in ("rgb", "depth", "expected_depth"):
            out[k + "_std"] = var[k].sqrt().mean(dim=-1).unsqueeze(-1)
    return out


def aggregate(outputs_list: List[Dict[str, torch.Tensor]], moments_fn: Optional[MomentsFn] = None):
    """All members on one device.  Every tensor is [H,W,C]."""
    moments_fn = moments_fn or _hip_moments
    keys = [k for k, v in outputs_list[0].items() if torch.is_tensor(v)]
    mean, var = {}, {}
    for k in keys:
        x = torch.stack([o[k] for o in outputs_list], dim=0)
        shp = x.shape[1:]
        m, v = moments_fn(x.reshape(x.shape[0], -1, shp[-1]).contiguous())   # also [M,1,3] for a splat `background`
        mean[k], var[k] = m.view(shp), v.view(shp)
    alea = {k: mean[k + "_var"] for k in ("rgb", "depth") if k + "_var" in mean}
    return _finish(keys, mean, var, alea)


def reduce_plan(keys: Sequence[str], shapes: Optional[Dict[str, Sequence[int]]] = None) -> Plan:
    """_finish stated once on the host, for unerf_ensemble_reduce: the list, in _finish's output order, of
    (output key, statistic, input key) with statistic one of
        "mean"                 the member mean of the input key
        "var_cmean"            the channel mean of the member variance (the epistemic term)
        "alea_cmean"           the channel mean of the member mean of input key + "_var" (the aleatoric term)
        "epi_plus_alea"        their sum
        "sqrt_epi_plus_alea"   its square root
        "std_cmean"            the channel mean of the member standard deviation
    _finish's order dependence is resolved here: an output written twice keeps its FIRST position and its LAST value, so
    with the active-nerfacto key order the member means of rgb_var / rgb_std / depth_var / depth_std replace the combined
    values and only *_var_alea / *_var_epi survive.  shapes (optional, {key: member tensor shape}): checked where _finish
    would fail -- an aleatoric key must have the elements of the key it belongs to."""
    keys = list(keys)
    has_std = "rgb_std" in keys and "depth_std" in keys
    out: Dict[str, Tuple[str, str]] = {}
    for k in keys:
        out[k] = ("mean", k)
        if has_std:
            if k in ("rgb", "depth"):
                if k + "_var" not in keys:
                    raise KeyError(k + "_var")
                if shapes is not None and tuple(shapes[k][:-1]) != tuple(shapes[k + "_var"][:-1]):
                    raise ValueError(f"{k}_var {tuple(shapes[k + '_var'])} does not match {k} {tuple(shapes[k])}")
                out[k + "_var_alea"] = ("alea_cmean", k)
                out[k + "_var_epi"] = ("var_cmean", k)
                out[k + "_var"] = ("epi_plus_alea", k)
                out[k + "_std"] = ("sqrt_epi_plus_alea", k)
        elif k in ("rgb", "depth", "expected_depth"):
            out[k + "_std"] = ("std_cmean", k)
    return [(name, stat, src) for name, (stat, src) in out.items()]


def _hip_reduce(views, plan):
    from . import ops
    return ops.ensemble_reduce(views, plan)


def _max_views() -> int:
    from . import lib
    return lib.NERF_MAX_VIEWS


def _out_shape(stat: str, shape: Sequence[int]) -> Tuple[int, ...]:
    return tuple(shape) if stat in ("mean", "var") else tuple(shape[:-1]) + (1,)


def aggregate_batch(per_member_views: Sequence[Sequence[Dict[str, torch.Tensor]]], reduce_fn: Optional[ReduceFn] = None):
    """aggregate for every view of a batch: per_member_views[j][v] is member j's output dict of view v (what each member's
    get_outputs_for_cameras returns).  Element v of the result equals aggregate([pm[v] for pm in per_member_views]), keys
    in the same order; the values are views into one arena per launch.  One fused reduce per UNERF_NERF_MAX_VIEWS views,
    which reads the members' tensors where they are (a channel slice of wider rows included: no stack, no copy)."""
    reduce_fn = reduce_fn or _hip_reduce
    B = len(per_member_views[0])
    if B == 0:
        return []
    first = per_member_views[0][0]
    keys = [k for k, v in first.items() if torch.is_tensor(v)]
    shapes = {k: tuple(first[k].shape) for k in keys}
    plan = reduce_plan(keys, shapes)
    res: List[Dict[str, torch.Tensor]] = []
    step = _max_views()
    for v0 in range(0, B, step):
        views = [{k: [pm[v][k].reshape(-1, shapes[k][-1]) for pm in per_member_views] for k in keys}
                 for v in range(v0, min(B, v0 + step))]
        for blocks in reduce_fn(views, plan):
            res.append({name: blocks[name].view(_out_shape(stat, shapes[src])) for name, stat, src in plan})
    return res


def pixel_slice(num_pixels: int, rank: int, world: int) -> Tuple[int, int]:
    """contiguous, balanced split of the flattened pixel axis (bit-exact bookkeeping: the slices
    tile [0,num_pixels) without gaps or overlap for every world size)."""
    base, rem = divmod(num_pixels, world)
    start = rank * base + min(rank, rem)
    return start, start + base + (1 if rank < rem else 0)


def _image_keys(member: Dict[str, torch.Tensor]) -> Tuple[List[str], List[str]]:
    """tensor keys split into per-pixel images [H,W,C] and everything else (active-splatfacto's `background` [3],
    activesplatfacto_model.py:363): the reference stacks and averages every key alike (ensemble_pipeline.py:159-162),
    only the images need the pixel-sliced exchange"""
    keys = [k for k, v in member.items() if torch.is_tensor(v)]
    H, W = next(v.shape[:2] for v in (member[k] for k in keys) if v.dim() == 3)
    img = [k for k in keys if member[k].dim() == 3 and tuple(member[k].shape[:2]) == (H, W)]
    return img, [k for k in keys if k not in img]


class _StageClock:
    """per-stage device times of aggregate_distributed (events on the current stream; the collectives of a NCCL / RCCL
    group make the current stream wait for them, so the event behind a collective is behind its data)"""

    def __init__(self, sink: Optional[dict], device):
        self.sink, self.marks = sink, []
        self.on = sink is not None and torch.device(device).type == "cuda"
        self.mark("start")

    def mark(self, name: str) -> None:
        if self.on:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.marks.append((name, ev))

    def finish(self) -> None:
        if not self.on:
            return
        self.marks[-1][1].synchronize()
        for (_, e0), (name, e1) in zip(self.marks[:-1], self.marks[1:]):
            self.sink[name] = self.sink.get(name, 0.0) + e0.elapsed_time(e1)
        self.sink["calls"] = self.sink.get("calls", 0) + 1


def aggregate_distributed(outputs, group=None, moments_fn: Optional[MomentsFn] = None, stage_ms: Optional[dict] = None):
    """This rank's member outputs -> the ensemble outputs, identical on every rank.
    `outputs` is one member's dict ([H,W,C] per key) or a list of such dicts when a rank holds several
    members (M members over N < M GPUs; every rank must hold the same number).

    Exchange (SURVEY.md 8e option A): ONE all_to_all of pixel slices -- rank g receives rows
    [a_g, b_g) of every member's packed image, (N-1)/N of one packed image sent and received per rank, all xGMI links
    busy at once -- then the exact two-pass moments on the slice (what torch.stack(...).mean(0) / .var(0) compute),
    then ONE all_gather of the reduced slices.  1080p, 6 floats per pixel: 44 MB out, 44 MB in per rank for the
    exchange (the two all_gathers of whole member images this replaces moved 8x that)."""
    import torch.distributed as dist
    moments_fn = moments_fn or _hip_moments
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    members = outputs if isinstance(outputs, (list, tuple)) else [outputs]
    all_keys = [k for k, v in members[0].items() if torch.is_tensor(v)]   # member key order (it matters, see _finish)
    keys, small_keys = _image_keys(members[0])
    widths = [members[0][k].shape[-1] for k in keys]
    H, W = members[0][keys[0]].shape[:2]
    P = H * W
    ml = len(members)
    # one packed [m_local, P, sum(C)] block per rank -> a single collective instead of one per key
    clock = _StageClock(stage_ms, members[0][keys[0]].device)
    packed = torch.stack([torch.cat([m[k].reshape(P, -1) for k in keys], dim=-1) for m in members], dim=0).contiguous()
    Ctot = packed.shape[-1]
    edges = [pixel_slice(P, r, world) for r in range(world)]
    a, b = edges[rank]
    # send block for destination r: this rank's members restricted to r's pixel rows, [m_local * (b_r - a_r), Ctot]
    send = torch.cat([packed[:, ar:br].reshape(-1, Ctot) for ar, br in edges], dim=0).contiguous()
    recv = torch.empty(world * ml * (b - a), Ctot, dtype=packed.dtype, device=packed.device)
    clock.mark("pack")
    dist.all_to_all_single(recv, send, output_split_sizes=[ml * (b - a)] * world,
                           input_split_sizes=[ml * (br - ar) for ar, br in edges], group=group)
    clock.mark("all_to_all")
    stack = recv.view(world * ml, b - a, Ctot)                      # [M, b-a, Ctot], member order = rank-major
    if b > a:
        m, v = moments_fn(stack.contiguous())
    else:
        m = v = torch.zeros(0, Ctot, dtype=packed.dtype, device=packed.device)
    part = torch.cat([m, v], dim=-1).contiguous()                   # [b-a, 2*Ctot]
    # slices differ by at most one row: pad to the largest so all_gather sees equal shapes
    rows = max(br - ar for ar, br in edges)
    padded = torch.zeros(rows, 2 * Ctot, dtype=part.dtype, device=part.device)
    padded[: b - a] = part
    parts = [torch.empty_like(padded) for _ in range(world)]
    clock.mark("moments")
    dist.all_gather(parts, padded, group=group)
    clock.mark("all_gather")
    full = torch.cat([parts[r][: edges[r][1] - edges[r][0]] for r in range(world)], dim=0)
    mean, var, off = {}, {}, 0
    for k, c in zip(keys, widths):
        mean[k] = full[:, off:off + c].reshape(H, W, c)
        var[k] = full[:, Ctot + off:Ctot + off + c].reshape(H, W, c)
        off += c
    if small_keys:   # a few floats per member: gathered whole, reduced on every rank
        flat = torch.stack([torch.cat([m[k].reshape(-1) for k in small_keys]) for m in members], dim=0).contiguous()
        allf = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(allf, flat, group=group)
        sm, sv = moments_fn(torch.cat(allf, dim=0)[:, None, :].contiguous())       # [M, 1, n] -> [1, n]
        off = 0
        for k in small_keys:
            n = members[0][k].numel()
            mean[k], var[k] = sm[0, off:off + n].reshape(members[0][k].shape), sv[0, off:off + n].reshape(members[0][k].shape)
            off += n
    alea = {k: mean[k + "_var"] for k in ("rgb", "depth") if k + "_var" in mean}
    res = _finish(all_keys, mean, var, alea)
    clock.mark("unpack")
    clock.finish()
    if stage_ms is not None:
        stage_ms["bytes_all_to_all_sent_per_rank"] = int(send.numel() * send.element_size() * (world - 1) // max(world, 1))
        stage_ms["bytes_all_gather_received_per_rank"] = int(padded.numel() * padded.element_size() * (world - 1))
        stage_ms["packed_image_bytes_per_member"] = int(P * Ctot * packed.element_size())
    return res


def aggregate_distributed_batch(per_member_views, group=None, reduce_fn: Optional[ReduceFn] = None,
                                stage_ms: Optional[dict] = None):
    """aggregate_distributed for every view of a batch with the collectives of ONE view: per_member_views[j][v] is local
    member j's output dict of view v (every rank holds the same number of members and views).  Element v of the result
    equals aggregate_distributed([pm[v] for pm in per_member_views]).

    ONE all_to_all for all B views -- rank g receives rows [a_g, b_g) of every member's packed image of every view --, then
    ONE fused reduce that reads the receive buffer in place (a key is a channel slice of its packed rows) and writes the
    FINAL keys of the slice, then ONE all_gather of those, padded to the largest slice as aggregate_distributed pads.  The
    returned images are views into the gathered buffer.  Non-image keys (a few floats per member) are gathered whole in one
    small all_gather for the batch and reduced on every rank by the same launch.  stage_ms: aggregate_distributed's stages."""
    import torch.distributed as dist
    reduce_fn = reduce_fn or _hip_reduce
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    B, ml = len(per_member_views[0]), len(per_member_views)
    if B == 0:
        return []
    first = per_member_views[0][0]
    all_keys = [k for k, v in first.items() if torch.is_tensor(v)]   # member key order (it matters, see _finish)
    keys, small_keys = _image_keys(first)
    shapes = {k: tuple(first[k].shape) for k in all_keys}
    plan = reduce_plan(all_keys, shapes)
    widths = [shapes[k][-1] for k in keys]
    H, W = shapes[keys[0]][:2]
    P, Ctot = H * W, sum(widths)
    dev, dtype = first[keys[0]].device, first[keys[0]].dtype
    clock = _StageClock(stage_ms, dev)
    # one packed [m_local, B, P, sum(C)] block per rank -> a single collective for the whole batch
    packed = torch.stack([torch.stack([torch.cat([vw[k].reshape(P, -1) for k in keys], dim=-1) for vw in pm], dim=0)
                          for pm in per_member_views], dim=0)
    edges = [pixel_slice(P, r, world) for r in range(world)]
    a, b = edges[rank]
    n = b - a
    # send block for destination r: this rank's members and views restricted to r's pixel rows, [m_local * B * (b_r - a_r), Ctot]
    send = torch.cat([packed[:, :, ar:br].reshape(-1, Ctot) for ar, br in edges], dim=0).contiguous()
    recv = torch.empty(world * ml * B * n, Ctot, dtype=dtype, device=dev)
    clock.mark("pack")
    dist.all_to_all_single(recv, send, output_split_sizes=[ml * B * n] * world,
                           input_split_sizes=[ml * B * (br - ar) for ar, br in edges], group=group)
    if small_keys:   # a few floats per member and view: gathered whole, reduced on every rank
        sizes = [first[k].numel() for k in small_keys]
        flat = torch.stack([torch.stack([torch.cat([vw[k].reshape(-1) for k in small_keys]) for vw in pm], dim=0)
                            for pm in per_member_views], dim=0).contiguous()               # [m_local, B, sum(sizes)]
        allf = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(allf, flat, group=group)
    clock.mark("all_to_all")
    stack = recv.view(world * ml, B, n, Ctot)                        # member order = rank-major
    offs = [sum(widths[:i]) for i in range(len(keys))]
    step = _max_views()
    reduced: List[Dict[str, torch.Tensor]] = []
    for v0 in range(0, B, step):
        views = []
        for v in range(v0, min(B, v0 + step)):
            src = {}
            for k in all_keys:
                if k in small_keys:
                    i = small_keys.index(k)
                    o = sum(sizes[:i])
                    src[k] = [f[j, v, o:o + sizes[i]].reshape(-1, shapes[k][-1]) for f in allf for j in range(ml)]
                else:
                    i = keys.index(k)
                    src[k] = [stack[j, v, :, offs[i]:offs[i] + widths[i]] for j in range(world * ml)]
            views.append(src)
        reduced.extend(reduce_fn(views, plan))
    img_plan = [(name, stat, src) for name, stat, src in plan if src in keys]
    out_w = [_out_shape(stat, shapes[src])[-1] for _, stat, src in img_plan]
    Fout = sum(out_w)
    # pixel-major [rows, B * Fout] so that the gathered slices line up as whole images; slices differ by at most one row:
    # pad to the largest so all_gather sees equal shapes
    rows = max(br - ar for ar, br in edges)
    padded = torch.zeros(rows, B * Fout, dtype=dtype, device=dev)
    if n > 0:
        torch.cat([reduced[v][name] for v in range(B) for name, _, _ in img_plan], dim=-1, out=padded[:n])
    parts = [torch.empty_like(padded) for _ in range(world)]
    clock.mark("moments")
    dist.all_gather(parts, padded, group=group)
    clock.mark("all_gather")
    full = torch.cat([parts[r][: edges[r][1] - edges[r][0]] for r in range(world)], dim=0)   # [P, B * Fout]
    res = []
    for v in range(B):
        out, off = {}, v * Fout
        col = {}
        for (name, _, _), c in zip(img_plan, out_w):
            col[name] = full[:, off:off + c].reshape(H, W, c)
            off += c
        for name, stat, src in plan:
            out[name] = col[name] if src in keys else reduced[v][name].view(_out_shape(stat, shapes[src]))
        res.append(out)
    clock.mark("unpack")
    clock.finish()
    if stage_ms is not None:
        stage_ms["bytes_all_to_all_sent_per_rank"] = int(send.numel() * send.element_size() * (world - 1) // max(world, 1))
        stage_ms["bytes_all_gather_received_per_rank"] = int(padded.numel() * padded.element_size() * (world - 1))
        stage_ms["packed_image_bytes_per_member"] = int(P * Ctot * packed.element_size())
    return res


class EnsemblePipeline:
    """The render-side surface of models/ensemble/ensemble_pipeline.py: `models` (the members this process holds)
    and `get_ensemble_outputs_for_camera_ray_bundle(camera, obb_box)` (:144-191), which is what
    scripts/eval_uncertainty.py:1127 calls.  The reference keeps all M members in one process and renders them
    in sequence; here a process holds M / world_size of them (all M without torch.distributed, one per GPU under
    `torchrun`), and the per-pixel moments go through aggregate / aggregate_distributed.  Pass built Models; the
    members' checkpoints (ensemble_pipeline.py:62-108, ensemble_utils.py:36-110) are read by
    `checkpoints.load_ensemble(models, config_paths)`."""

    def __init__(self, models: Sequence, group=None, moments_fn: Optional[MomentsFn] = None, fused: bool = False,
                 reduce_fn: Optional[ReduceFn] = None):
        self.models = torch.nn.ModuleList(models) if all(isinstance(m, torch.nn.Module) for m in models) else list(models)
        self.group, self.moments_fn = group, moments_fn
        # fused: end in aggregate_batch / aggregate_distributed_batch (one unerf_ensemble_reduce launch per batch of views)
        # instead of one aggregate / aggregate_distributed per view; reduce_fn is to them what moments_fn is to those
        self.fused, self.reduce_fn = fused, reduce_fn

    def _aggregate_fused(self, per_member: List[List[Dict[str, torch.Tensor]]]) -> List[Dict[str, torch.Tensor]]:
        if self._distributed():
            return aggregate_distributed_batch(per_member, group=self.group, reduce_fn=self.reduce_fn)
        assert len(per_member) > 1, "Ensemble requires at least two models."
        return aggregate_batch(per_member, reduce_fn=self.reduce_fn)

    @property
    def model(self):  # VanillaPipeline.model = the first member (ensemble_pipeline.py:51)
        return self.models[0]

    def _distributed(self) -> bool:
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1

    @torch.no_grad()
    def get_ensemble_outputs_for_camera_ray_bundle(self, camera, obb_box=None) -> Dict[str, torch.Tensor]:
        kw = {} if obb_box is None else {"obb_box": obb_box}
        outs = [m.get_outputs_for_camera(camera, **kw) for m in self.models]
        if self.fused:
            return self._aggregate_fused([[o] for o in outs])[0]
        if self._distributed():
            return aggregate_distributed(outs, group=self.group, moments_fn=self.moments_fn)
        assert len(outs) > 1, "Ensemble requires at least two models."
        return aggregate(outs, moments_fn=self.moments_fn)


    @torch.no_grad()
    def get_ensemble_outputs_for_cameras(self, cameras, obb_box=None, max_views: int = 16) -> List[Dict[str, torch.Tensor]]:
        """get_ensemble_outputs_for_camera_ray_bundle for every camera of a batch of one image size (the argument
        conventions of the members' get_outputs_for_cameras): each member renders the whole batch through its own
        get_outputs_for_cameras -- up to max_views small frames per launch group --, then the moments run per view
        (fused=True: for all views in one launch).  Element v equals the per-camera call for camera v."""
        kw = {} if obb_box is None else {"obb_box": obb_box}
        per_member = [m.get_outputs_for_cameras(cameras, max_views=max_views, **kw) for m in self.models]
        if self.fused:
            return self._aggregate_fused(per_member)
        res = []
        for v in range(len(per_member[0])):
            outs = [pm[v] for pm in per_member]
            if self._distributed():
                res.append(aggregate_distributed(outs, group=self.group, moments_fn=self.moments_fn))
            else:
                assert len(outs) > 1, "Ensemble requires at least two models."
                res.append(aggregate(outs, moments_fn=self.moments_fn))
        return res


def views_for_rank(num_views: int, rank: int, world: int) -> List[int]:
    """View-batch data parallelism for splats / single models: replicas of the scene,
    disjoint cameras per rank, no data-path collective."""
    return list(range(rank, num_views, world))
