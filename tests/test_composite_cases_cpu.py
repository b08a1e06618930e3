"""The hand-placed compositing cases of tests/composite_cases.py, checked without a GPU.  The fp32 CPU chain (the oracle's
operations in float32) goes through the very checks tests/test_gpu_composite_edges.py applies to the kernels -- every channel
within its bound, the exact family bit for bit, the median rule, the pass moments in both summation forms -- which proves that
the inputs keep the float64 reference within every condition by themselves; SUM_EPS, MOM_EPS and LAP_FACTOR have their measured
basis; and a restatement of composite_one's 16-lane LAYOUT (slot ownership, masked slots, last_lane, cnt -> idx -> owner, slot,
the clip row: not its arithmetic, which stays the oracle's) shows that the cases bite: each planted mutation fails named cases."""
import numpy as np
import pytest
import torch

import composite_cases as CC
from oracle import nerf_oracle as O

SINGLE = {**CC.COMPOSITE, **CC.ALT, **CC.VIEWS, **CC.EXACT}


def _chain(c, b):
    return CC.chain32(c.dens[b], c.rgb[b], c.beta, c.sb, c.lo, c.hi, c.bg, c.near, c.far, c.spacing, c.walt)


@pytest.mark.parametrize("key", list(SINGLE))
def test_case_builds_and_fp32_chain_passes_every_check(key):
    c = SINGLE[key]()
    for b in range(c.B):
        ratios = CC.hold(f"{key} pass {b}", c.refs[b], _chain(c, b), expect=c.expect if c.family == "exact" else None)
    print(f"{key}: SPL {c.spl} ragged {c.ragged} ties {c.n_ties} fp32 chain error / bound (last pass): "
          + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


@pytest.mark.parametrize("key", list({**CC.MOMENTS, **CC.PLANES}))
def test_pass_moments_of_the_fp32_chain_pass_in_both_summation_forms(key):
    c = {**CC.MOMENTS, **CC.PLANES}[key]()
    per = torch.stack([_chain(c, b) for b in range(c.B)])
    for b in range(c.B):
        CC.hold(f"{key} pass {b}", c.refs[b], per[b])
    per[..., 6] = 0.0      # the K-pass kernels take no beta
    mr = CC.moments_reference(CC.refs_without_beta(c))
    forms = ([CC.moments_shifted32] if c.B >= 2 else []) + [CC.moments_two_pass32]
    for form in forms:
        m, v = (torch.from_numpy(np.asarray(a)) for a in form(per.numpy()))
        rm, rv = CC.hold_moments(f"{key} {form.__name__}", mr, m, v)
        print(f"{key} {form.__name__}: ties {c.n_ties} error / bound: mean {rm:.3f} variance {rv:.3f}")


def test_cases_cover_the_kernel_edges():
    CC.check_coverage()
    assert {CC.spl_for(S) for S in range(1, 257)} == set(CC.SPLS) and CC.spl_for(80) == 6 and CC.spl_for(112) == 8


def test_bounds_rest_on_the_measured_fp32_chains():
    s, m, l = CC.measure_sums(), CC.measure_moments(), CC.measure_laplace()
    print(f"fp32 CPU restatements vs float64: sums {s:.3e} of sum |term|, pass moments {m:.3e}, depth draws {l:.3f} units")
    assert CC.SUM_WORST_MEASURED >= s and 4 * CC.SUM_WORST_MEASURED <= CC.SUM_EPS <= 4.2 * CC.SUM_WORST_MEASURED
    assert CC.MOM_WORST_MEASURED >= m and 4 * CC.MOM_WORST_MEASURED <= CC.MOM_EPS <= 4.2 * CC.MOM_WORST_MEASURED
    assert CC.LAP_WORST_MEASURED >= l and 8 * CC.LAP_WORST_MEASURED <= CC.LAP_FACTOR <= 8.4 * CC.LAP_WORST_MEASURED


@pytest.mark.parametrize("key", list(CC.LAPLACE))
def test_depth_draws_fp32_running_product_passes(key):
    c = CC.LAPLACE[key]()
    print(f"{key}: fp32 running product error / bound {CC.hold_laplace(c, CC.laplace32(c)):.3f}")


@pytest.mark.parametrize("K", CC.K_MOMENTS)
def test_stack_moments_two_pass_fp32_passes(K):
    c = CC.stack_moments(K)
    x = c.x.numpy()
    s = np.zeros(x.shape[1:], np.float32)
    for k in range(K):
        s = s + x[k]
    m = s / np.float32(K)
    q = np.zeros_like(s)
    for k in range(K):
        q = q + (x[k] - m) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        v = q / np.float32(K - 1)
    print(f"stack K = {K}: fp32 two-pass error / bound {CC.hold_stack(c, torch.from_numpy(m), torch.from_numpy(v))}")


def test_chain32_is_the_oracle_and_the_reference_agrees_with_it():
    c = CC.toleranced(96, 1, "last_sample")
    _, steps = CC.geometry(c.sb, c.near, c.far, c.spacing)
    delta = O.spacing_to_euclidean(c.sb, c.near, c.far)
    w = O.get_weights(c.dens[0], delta[:, 1:] - delta[:, :-1])
    got = _chain(c, 0)
    assert torch.equal(got[:, :3], O.render_rgb(c.rgb[0], w)) and torch.equal(got[:, 3:4], O.render_accumulation(w))
    assert torch.equal(got[:, 4:5], O.render_depth_median(w, steps)) and torch.equal(got[:, 6:7], O.render_uncertainty(c.beta, w ** 2))
    for j in range(c.clip.shape[0]):
        if j != 2:      # (row 2 is narrowed: the oracle's own min / max clip holds on the other rows)
            sel = c.rows == j
            assert torch.equal(got[sel, 5:6], torch.clip(torch.sum(w * steps, -1, keepdim=True) / (w.sum(-1, keepdim=True) + 1e-10),
                                                         steps[sel].min(), steps[sel].max())[sel])


# ---- the 16-lane layout of composite_one, restated (layout only; every sum is the fp32 oracle's) --------------------------
def lane_layout(c, b, mutation=None):
    """-> [R,8] fp32.  Slot k0 = l16 SPL + e belongs to lane l16; RAGGED: slots k >= S are masked (mid-point = edge S, weight 0,
    not counted, not a "last sample"); the background colour comes from lane last_lane's last real sample; the median is slot
    idx = min(cnt, S - 1) of lane idx / SPL, cnt = the number of live slots whose inclusive weight sum is < 0.5; the clip row is
    (ray_offset + r) / chunk_rays, or per view.  mutation: one planted defect"""
    S, spl, ragged = c.S, c.spl, c.ragged
    out = _chain(c, b).clone()
    eb = O.spacing_to_euclidean(c.sb, c.near, c.far, uniform=bool(c.spacing))
    delta, steps = CC.geometry(c.sb, c.near, c.far, c.spacing)
    w = O.get_weights(c.dens[b], delta)
    wd = w if c.walt is None else c.walt
    cw = torch.cumsum(wd, dim=-1)
    slots = torch.arange(16 * spl)
    live = slots < S
    src = torch.clamp(slots, max=S - 1)
    slot_steps = torch.where(live[None], steps[:, src], eb[:, S:S + 1])          # masked: both edges collapse onto edge S
    below = (cw[:, src] <= 0.5) if mutation == "le" else (cw[:, src] < 0.5)
    counted = below if mutation == "count_masked" else below & live[None]
    cnt = counted.sum(-1)
    idx = torch.clamp(cnt, max=S if mutation == "clamp_S" else S - 1)
    owner, slot = (idx // spl) % 16, idx % spl                                   # __shfl(..., owner, 16) wraps
    depth = torch.gather(slot_steps, -1, (owner * spl + slot)[:, None])
    out[:, 4:5] = depth
    out[:, 7:8] = torch.sum(wd * (steps - depth) ** 2, dim=-1, keepdim=True) + 1e-5
    if c.bg == "last_sample":
        last_lane = 15 if (mutation == "lane15" or not ragged) else (S - 1) // spl
        mine = [k for k in range(last_lane * spl, (last_lane + 1) * spl) if k < S]
        col = torch.nan_to_num(c.rgb[b])
        bg = col[:, mine[-1]] if mine else torch.zeros(c.R, 3)                  # a lane without a real sample keeps (0, 0, 0)
        comp = torch.sum(w[..., None] * col, dim=-2)
        out[:, :3] = torch.clamp(comp + bg * (1.0 - w.sum(-1, keepdim=True)), 0.0, 1.0)
    r = torch.arange(c.R)
    row = c.rows
    if mutation == "no_offset" and not c.views:
        row = r // CC.CHUNK
    if mutation == "global_row" and c.views:
        row = r // CC.CHUNK
    acc = wd.sum(-1, keepdim=True)
    ed = torch.sum(wd * steps, dim=-1, keepdim=True) / (acc + 1e-10)
    row = torch.clamp(row, max=c.clip.shape[0] - 1)
    out[:, 5:6] = torch.minimum(torch.maximum(ed, c.clip[row, 0:1]), c.clip[row, 1:2])
    return out


def _fails(c, mutation):
    try:
        for b in range(c.B):
            CC.hold(c.name, c.refs[b], lane_layout(c, b, mutation), expect=c.expect if c.family == "exact" else None)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("key", list(SINGLE))
def test_lane_layout_restated_passes_every_check(key):
    c = SINGLE[key]()
    assert not _fails(c, None)
    for b in range(c.B):      # counting the masked slots as well changes nothing: their inclusive sum is the ray's total, which is
        # below 0.5 only when every live slot is counted already, and min(cnt, S - 1) clamps either count to S - 1
        assert torch.equal(lane_layout(c, b, "count_masked"), lane_layout(c, b))


# mutation -> cases that must fail (the test also reports every case that does)
MUTATIONS = {
    "lane15": ["S17-B1", "S33-B3", "S112-B3", "alt-S129", "exact-S129-last_sample", "exact-S17-last_sample"],
    "clamp_S": ["S16-B3", "S17-B3", "S129-B1", "S256-B3", "alt-S48"],
    "le": ["alt-S17", "alt-S48", "alt-S129"],
    "no_offset": ["S16-B3", "S129-B3", "S255-B1"],
    "global_row": ["views-S1", "views-S17", "views-S48", "views-S256"],
}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_each_mutation_of_the_layout_fails_named_cases(mutation):
    failed = [k for k, f in SINGLE.items() if _fails(f(), mutation)]
    print(f"mutation {mutation}: {len(failed)} of {len(SINGLE)} cases fail: {failed}")
    assert set(MUTATIONS[mutation]) <= set(failed)


def test_plain_sum_of_squares_variance_fails_the_planes_cases():
    """the planes kernel's pass variance without its shift by pass 0 and without fmaxf(..., 0)"""
    failed = []
    for key, f in CC.PLANES.items():
        c = f()
        per = torch.stack([_chain(c, b) for b in range(c.B)])
        per[..., 6] = 0.0
        m, v = (torch.from_numpy(np.asarray(a)) for a in CC.moments_shifted32(per.numpy(), shift=False, clamp=False))
        try:
            CC.hold_moments(key, CC.moments_reference(CC.refs_without_beta(c)), m, v)
        except AssertionError:
            failed.append(key)
    print(f"plain sum-of-squares variance: {len(failed)} of {len(CC.PLANES)} planes cases fail: {failed}")
    assert {"planes-S48-B2", "planes-S256-B9", "planes-S17-B4"} <= set(failed)
