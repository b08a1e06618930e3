"""Edge cases of the LPIPS kernels (csrc/unerf_lpips.hip): the cases, their references, the derived bounds, and numpy
twins of the kernels' algorithms with named planted defects.  Used by tests/test_lpips_edge_cases_cpu.py (no GPU) and
tests/test_gpu_lpips_edges.py.  Nothing here reads a kernel result.

Every size comes from the constants lib.py mirrors from include/unerf.h:

    EW = LPIPS_EW_THREADS          threads per workgroup of the pack and pool kernels
    E  = EW * LPIPS_EW_MAX_WG      values one sweep of their capped grid covers; beyond it a thread strides by E
    T, TN = LPIPS_CONV_TILE_M, _N  the convolution's row and column tile
    KS = LPIPS_CONV_STEP_K         its reduction step
    HP = LPIPS_HEAD_PIXELS         pixels per workgroup of the head
    BMAX = METRICS_MAX_IMAGES      images per call; the per-image kernels run as ONE block of 64 threads

Bounds (none comes from a kernel):
  pack   the float32 torch statement bit for bit, exact counts (tests/test_gpu_lpips.py's rule)
  pool   F.max_pool2d on the CPU: equal NaN masks, equal bits elsewhere
  conv   float64 F.conv2d, every output inside gamma(K + 1, 2^-24) (|b| + sum |a w|): any order of K fp32 products and a
         bias.  Where the float64 value itself is not finite (a NaN or an inf was planted in a window) the bound says
         nothing; there the result must BE that value: NaN where the reference is NaN, the same infinity elsewhere
  head   the longdouble statement, gamma(P C + 8, 2^-53) sum |terms|
  e2e    the fp32 host definition's own |float32 - float64|, for the total and for each layer, the larger of the value
         over lpips_cases' set and over the new cases; the kernels get E2E_MARGIN = 4 x that"""
import functools
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import lpips_cases as LC
from uncertainty_nerf_gs_amd import lib as L
from uncertainty_nerf_gs_amd import metrics as M

EW, EW_MAX_WG = L.LPIPS_EW_THREADS, L.LPIPS_EW_MAX_WG
E = EW * EW_MAX_WG
T, TN, KS, HP = L.LPIPS_CONV_TILE_M, L.LPIPS_CONV_TILE_N, L.LPIPS_CONV_STEP_K, L.LPIPS_HEAD_PIXELS
BMAX = L.METRICS_MAX_IMAGES
WAVE = 64
HEAD_WAVES = 4                 # lp_head_kernel: 256 threads
U32, U64 = 2.0 ** -24, 2.0 ** -53
E2E_MARGIN = 4.0
NAN, INF = float("nan"), float("inf")


def ew_grid(total):
    """workgroups the pack and pool kernels are launched with (lp_ew_grid)"""
    return min((total + EW - 1) // EW, EW_MAX_WG)


def ew_trips(total):
    """sweeps of that grid the busiest thread makes"""
    return (total + ew_grid(total) * EW - 1) // (ew_grid(total) * EW)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# ---- pack -------------------------------------------------------------------------------------------------------------

PackCase = namedtuple("PackCase", "name B n")
PACK_CASES = (
    PackCase("one-block", 1, EW // 3),                       # 3 n <= EW
    PackCase("two-blocks", 3, EW // 3 + 1),
    PackCase("cap", 1, E // 3),                              # 3 n <= E: the full grid, no second trip
    PackCase("cap-plus", 2, E // 3 + 1),                     # a second trip of 3 n - E values
    PackCase("three-trips", 2, 2 * E // 3 + 5),              # the last trip partial
)


def pack_plants(c):
    """[(image, "pred" | "target", index into the image's 3 n values, value, counted)]: a NaN prediction, a negative
    prediction and a target above 1 in the first trip; the last element; and, where the case has later trips (B >= 2
    there, since the second trip of cap-plus has two values), the same three in the last trip, one clipped prediction
    above 1 that must not be counted, and two in the middle trip of a three-trip case"""
    n3, last_img = 3 * c.n, c.B - 1
    plants = [(0, "pred", 1, NAN, 1), (last_img, "pred", 5, -0.25, 1), (0, "target", 7, 1.5, 1), (last_img, "target", n3 - 1, NAN, 1)]
    trips = ew_trips(n3)
    if trips > 1:
        s = (trips - 1) * E
        plants += [(0, "pred", s, NAN, 1), (0, "pred", s + 1, 1.5, 0), (last_img, "pred", s + 1, -1e-9, 1), (0, "target", s, 1.25, 1)]
    if trips > 2:
        plants += [(last_img, "pred", E + 3, NAN, 1), (0, "target", E + 4, -0.5, 1)]
    return plants


@functools.lru_cache(maxsize=None)
def pack_inputs(c):
    """-> (pred, target [B, n, 3] float32 with the plants in, per-image counts of refused values); shared, not to be changed"""
    pred, target = LC.image_pair(c.n, 1, c.B)
    pred, target = pred.reshape(c.B, c.n, 3).contiguous(), target.reshape(c.B, c.n, 3).contiguous()
    want = [0] * c.B
    for b, which, i, v, counted in pack_plants(c):
        (pred if which == "pred" else target)[b].view(-1)[i] = v
        want[b] += counted
    return pred, target, want


def pack_reference(pred, target, w):
    """the float32 torch statement (tests/test_gpu_lpips.py) and the counts by metrics._lpips_operands' rule"""
    x = torch.cat((torch.clip(pred, max=1.0), target))
    act = ((2 * x - 1) - w.shift) / w.scale
    B = pred.shape[0]
    bad = [int((~((x[b] >= 0) & (x[b] <= 1))).sum()) + int((~((x[B + b] >= 0) & (x[B + b] <= 1))).sum()) for b in range(B)]
    return act, bad


def pack_twin(pred, target, w, mut=None):
    """lp_pack_kernel in numpy float32: thread (block, t) of a grid of ew_grid(3 n) blocks visits i = its index, then
    strides by the grid's width; c = i % 3; a thread's count runs across its trips.  -> (act [2 B, n, 3], counts [B])"""
    B, n = pred.shape[0], pred.shape[1]
    n3 = 3 * n
    width = ew_grid(n3) * EW
    shift, scale = w.shift.numpy().astype(np.float32), w.scale.numpy().astype(np.float32)
    act = np.full((2 * B, n3), np.float32(-7.0))                # never-written values stay visibly wrong
    counts = []
    f1, f2 = np.float32(1.0), np.float32(2.0)
    for b in range(B):
        p, t = pred[b].reshape(-1).numpy(), target[b].reshape(-1).numpy()
        count = np.zeros(width, dtype=np.int64)
        for trip in range(ew_trips(n3)):
            if trip and mut == "pack_later_sweeps_dropped":
                break
            i = trip * width + np.arange(min(width, n3 - trip * width))
            c = i % 3
            x = np.where(p[i] > f1, f1, p[i])
            y = t[i]
            with np.errstate(invalid="ignore"):
                here = (~((x >= 0) & (x <= f1))).astype(np.int64) + (~((y >= 0) & (y <= f1))).astype(np.int64)
                if mut == "pack_later_counts_dropped":
                    count[:len(i)] = here
                else:
                    count[:len(i)] += here
                act[b, i] = ((f2 * x - f1) - shift[c]) / scale[c]
                act[B + b, i] = ((f2 * y - f1) - shift[c]) / scale[c]
        counts.append(int(count.sum()))
    return torch.from_numpy(act.reshape(2 * B, n, 3)), counts


# ---- pool -------------------------------------------------------------------------------------------------------------

PoolCase = namedtuple("PoolCase", "name N H W C plants")     # plants: ((n, y, x, c, value), ...)


def pool_out(x):
    return (x - 3) // 2 + 1


def _pool_cap_side(N, C):
    """the smallest square map whose N * Ho * Wo * C outputs exceed one sweep"""
    s = 3
    while N * pool_out(s) ** 2 * C <= E:
        s += 1
    return s


def _window_plants(N, H, W, C):
    """a NaN as the first, the middle and the last element of a window, a window of -inf, a +inf: each in a window of
    its own where the map has the room (the windows of output (oy, ox) and (oy, ox + 2) share nothing), channels off 0"""
    Ho, Wo = pool_out(H), pool_out(W)
    n, c = N - 1, C - 1
    if Wo < 2:
        return ()
    oy, ox = Ho - 1, Wo - 1                                      # the last window: its last element is the last one read
    plants = [(n, 2 * oy + 2, 2 * ox + 2, c, NAN)]
    plants += [(0, 0, 0, 0, NAN)]                                # first element of window (0, 0)
    plants += [(0, 1, 2 * (Wo // 2) + 1, c // 2, NAN)]           # middle of window (0, Wo // 2): in no other window
    if Ho >= 4 and Wo >= 4:
        plants += [(n, 4 + dy, 4 + dx, 1 % C, -INF) for dy in range(3) for dx in range(3)]       # window (2, 2), all -inf
        plants += [(0, 2 * (Ho - 1) + 1, 1, c, INF)]
    return tuple(plants)


def _make_pool_cases():
    cases = []
    for name, plants in (("3x3-plain", ()), ("3x3-nan-first", ((0, 0, 0, 0, NAN),)), ("3x3-nan-middle", ((0, 1, 1, 0, NAN),)),
                         ("3x3-nan-last", ((0, 2, 2, 0, NAN),)), ("3x3-inf", ((0, 1, 2, 0, INF),)),
                         ("3x3-all-neg-inf", tuple((0, y, x, 0, -INF) for y in range(3) for x in range(3)))):
        cases.append(PoolCase(name, 1, 3, 3, 1, plants))
    # even H and W: the last row and column are in no window; the NaN at the last input element must not be read
    cases.append(PoolCase("4x6-c65", 2, 4, 6, WAVE + 1, _window_plants(2, 4, 6, WAVE + 1) + ((1, 3, 5, WAVE, NAN),)))
    s = _pool_cap_side(2, WAVE)
    cases.append(PoolCase("cap-square", 2, s, s, WAVE, _window_plants(2, s, s, WAVE)))
    cases.append(PoolCase("cap-h-plus-1", 2, s + 1, s, WAVE, _window_plants(2, s + 1, s, WAVE) + ((1, s, s - 1, WAVE - 1, NAN),)))
    return tuple(cases)


POOL_CASES = _make_pool_cases()


@functools.lru_cache(maxsize=None)
def pool_input(name):
    c = {p.name: p for p in POOL_CASES}[name]
    g = torch.Generator().manual_seed(6000 + 131 * c.H + 7 * c.W + c.C)
    x = torch.randn(c.N, c.H, c.W, c.C, generator=g)
    x[x == 0] = 0.5                                              # no zero of either sign: which of +-0 wins is not specified
    for n, y, xx, ch, v in c.plants:
        x[n, y, xx, ch] = v
    return x


def pool_reference(x):
    return F.max_pool2d(x.permute(0, 3, 1, 2), kernel_size=3, stride=2).permute(0, 2, 3, 1).contiguous()


def pool_twin(x, mut=None):
    """lp_pool_kernel in numpy: the strided sweep over the outputs, m = p[0], then the nine taps under (v > m || v != v)"""
    N, H, W, C = x.shape
    Ho, Wo = pool_out(H), pool_out(W)
    total = N * Ho * Wo * C
    width = ew_grid(total) * EW
    src = x.numpy().reshape(-1)
    out = np.full(total, np.float32(-7.0))
    for trip in range(ew_trips(total)):
        i = trip * width + np.arange(min(width, total - trip * width), dtype=np.int64)
        c, r = i % C, i // C
        ox, r = r % Wo, r // Wo
        oy, img = r % Ho, r // Ho
        base = ((img * H + 2 * oy) * W + 2 * ox) * C + c
        m = src[base]
        for dy in range(3):
            for dx in range(3):
                v = src[base + (dy * W + dx) * C]
                with np.errstate(invalid="ignore"):
                    take = (v > m) if mut == "pool_nan_rule_removed" else ((v > m) | (v != v))
                m = np.where(take, v, m)
        out[i] = m
    return torch.from_numpy(out.reshape(N, Ho, Wo, C))


def same_with_nans(got, want):
    """equal NaN masks and equal bits elsewhere"""
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool(torch.equal(gn, wn)) and bool(torch.equal(bits(got)[~wn], bits(want)[~wn]))


# ---- convolution ------------------------------------------------------------------------------------------------------

ConvCase = namedtuple("ConvCase", "name N H W Ci Co ks stride pad relu plants")   # plants: ((n, y, x, c, value), ...)


def conv_out(x, ks, stride, pad):
    return (x + 2 * pad - ks) // stride + 1


def _tile_sides():
    h = int(math.isqrt(T))
    while T % h:
        h -= 1
    return h, T // h


def _make_conv_cases():
    cases = []
    two = (TN, 2 * TN)
    # the reduction edges at N = 2, 5 x 7: K below one step, one step exactly, a tail of one, two steps, a tail of KS - 5
    for j, (ks, ci) in enumerate(((3, 1), (1, KS), (1, KS + 1), (1, 2 * KS), (3, 3))):
        cases.append(ConvCase(f"k{ks * ks * ci}", 2, 5, 7, ci, two[j % 2], ks, 1, ks // 2, True, ()))
    cases.append(ConvCase("corner-one-tap", 2, 4, 5, 3, TN, 7, 3, 6, True, ()))
    cases.append(ConvCase("stride2-8x9", 2, 8, 9, 4, 2 * TN, 3, 2, 0, True, ()))       # the last input row is in no window
    cases.append(ConvCase("stride2-8x10", 2, 8, 10, 4, TN, 3, 2, 0, True, ()))         # nor is the last column here
    cases.append(ConvCase("conv1-33x34", 2, 33, 34, 3, TN, 11, 4, 2, True, ()))
    cases.append(ConvCase("conv2-1x1", 2, 1, 1, 64, 2 * TN, 5, 1, 2, True, ()))
    assert (2 * T + 1) % 3 == 0
    cases.append(ConvCase("rows-2T+1", 3, 1, (2 * T + 1) // 3, 5, TN, 3, 1, 1, True, ()))
    th, tw = _tile_sides()
    cases.append(ConvCase("rows-T-per-image", 2, th, tw, 5, 2 * TN, 3, 1, 1, True, ()))
    # non-finite inputs: a +inf beside the padding, a NaN in the last value of the last pixel of the last image
    nf = ((0, 0, 0, 0, INF), (1, 4, 6, 2, NAN))
    cases.append(ConvCase("nonfinite-relu", 2, 5, 7, 3, TN, 3, 1, 1, True, nf))
    cases.append(ConvCase("nonfinite-linear", 2, 5, 7, 3, TN, 3, 1, 1, False, nf))
    # a NaN and an inf where the stride never reaches: they must not show
    unread = ((1, 7, 9, 3, NAN), (0, 7, 2, 0, INF), (0, 3, 9, 1, NAN))
    cases.append(ConvCase("nonfinite-unread", 2, 8, 10, 4, TN, 3, 2, 0, True, unread))
    return tuple(cases)


CONV_CASES = _make_conv_cases()


def conv_dims(c):
    Ho, Wo = conv_out(c.H, c.ks, c.stride, c.pad), conv_out(c.W, c.ks, c.stride, c.pad)
    return Ho, Wo, c.N * Ho * Wo, c.ks * c.ks * c.Ci


@functools.lru_cache(maxsize=None)
def conv_inputs(name):
    """-> (x [N, H, W, Ci], weight [Co, Ci, ks, ks], bias [Co], packed [K, Co]) float32"""
    c = {q.name: q for q in CONV_CASES}[name]
    K = c.ks * c.ks * c.Ci
    g = torch.Generator().manual_seed(8000 + sum(ord(ch) for ch in c.name.replace("linear", "relu")))
    x = torch.randn(c.N, c.H, c.W, c.Ci, generator=g)
    w = torch.randn(c.Co, c.Ci, c.ks, c.ks, generator=g) / math.sqrt(K)
    b = torch.randn(c.Co, generator=g)
    for n, y, xx, ch, v in c.plants:
        x[n, y, xx, ch] = v
    return x, w, b, w.permute(2, 3, 1, 0).reshape(K, c.Co).contiguous()


@functools.lru_cache(maxsize=None)
def conv_reference(name):
    """-> (float64 result [N, Ho, Wo, Co] after the case's ReLU, bound [N, Ho, Wo, Co]); where the result is not
    finite the bound is NaN and `conv_check` asks for the value itself"""
    c = {q.name: q for q in CONV_CASES}[name]
    x, w, b, _ = conv_inputs(name)
    K = c.ks * c.ks * c.Ci
    x64 = x.double().permute(0, 3, 1, 2)
    raw = F.conv2d(x64, w.double(), b.double(), stride=c.stride, padding=c.pad)
    finite_x = torch.where(torch.isfinite(x64), x64, torch.zeros_like(x64))
    mag = F.conv2d(finite_x.abs(), w.double().abs(), b.double().abs(), stride=c.stride, padding=c.pad)
    ref = torch.relu(raw) if c.relu else raw                     # 1-Lipschitz: the bound carries over
    bound = LC.gamma(K + 1, U32) * mag
    bound = torch.where(torch.isfinite(raw), bound, torch.full_like(bound, NAN))
    return ref.permute(0, 2, 3, 1).contiguous(), bound.permute(0, 2, 3, 1).contiguous()


def conv_check(got, ref, bound):
    """-> (ok, worst error / bound over the finite outputs).  NaN exactly where the reference is NaN; where the
    reference (before the ReLU) was infinite, the value the reference has; everything else inside the bound"""
    got = got.detach().cpu().double()
    if got.shape != ref.shape:
        return False, INF
    hard = torch.isnan(bound)
    nan_ok = bool(torch.equal(torch.isnan(got), torch.isnan(ref)))
    inf_ok = bool(torch.equal(got[hard & ~torch.isnan(ref)], ref[hard & ~torch.isnan(ref)]))
    soft = ~hard
    ratio = ((got[soft] - ref[soft]).abs() / bound[soft])
    worst = float(ratio.max()) if ratio.numel() else 0.0
    return nan_ok and inf_ok and not math.isnan(worst) and worst <= 1.0, worst


def conv_twin(name, mut=None):
    """lp_conv_kernel in numpy float32: per row tile the staging registers of step s + 1 are fetched under the guard
    while step s is added, a tap outside the image, a row past M and k >= K give 0, the products of a step are added
    to the accumulator one k at a time, then bias and ReLU.  A fetch that does not happen leaves the registers as they
    were, as in the kernel."""
    c = {q.name: q for q in CONV_CASES}[name]
    x, _, b, packed = conv_inputs(name)
    Ho, Wo, Mtot, K = conv_dims(c)
    src, wk, bias = x.numpy(), packed.numpy(), b.numpy()
    out = np.zeros((Mtot, c.Co), dtype=np.float32)
    for m0 in range(0, Mtot, T):
        m = m0 + np.arange(T)
        live = m < Mtot
        mm = np.where(live, m, 0)
        img = (np.full(T, m0) if mut == "conv_image_from_tile_first_row" else mm) // (Ho * Wo)
        r = mm - (mm // (Ho * Wo)) * (Ho * Wo)
        oy, ox = r // Wo, r - (r // Wo) * Wo
        iy0, ix0 = oy * c.stride - c.pad, ox * c.stride - c.pad

        def fetch(k0):
            k = k0 + np.arange(KS)
            kin = k < K
            tap = np.where(kin, k // c.Ci, 0)
            ch = np.where(kin, k - (k // c.Ci) * c.Ci, 0)
            ky, kx = tap // c.ks, tap - (tap // c.ks) * c.ks
            iy, ix = iy0[:, None] + ky[None, :], ix0[:, None] + kx[None, :]
            inside = (iy >= 0) & (iy < c.H) & (ix >= 0) & (ix < c.W)
            if mut == "conv_tap_clamped_to_edge":
                inside = np.ones_like(inside)
            ok = kin[None, :] & live[:, None] & inside
            a = src[img[:, None], np.clip(iy, 0, c.H - 1), np.clip(ix, 0, c.W - 1), ch[None, :]]
            ra = np.where(ok, a, np.float32(0.0)).astype(np.float32)
            rb = np.zeros((KS, c.Co), dtype=np.float32)
            rb[kin] = wk[k[kin]]
            return ra, rb

        acc = np.zeros((T, c.Co), dtype=np.float32)
        ra, rb = fetch(0)
        k0 = 0
        while (k0 + KS <= K) if mut == "conv_last_partial_step_dropped" else (k0 < K):
            As, Bs = ra, rb
            ahead = 2 * KS if mut == "conv_prefetch_guard_one_step_late" else KS
            if k0 + ahead < K:
                ra, rb = fetch(k0 + KS)
            with np.errstate(invalid="ignore", over="ignore"):
                for kk in range(KS):
                    acc = acc + As[:, kk:kk + 1] * Bs[kk:kk + 1, :]
            k0 += KS
        with np.errstate(invalid="ignore"):
            v = acc + bias[None, :]
            if c.relu:
                v = np.where(v < 0, np.float32(0.0), v)
        out[m0:m0 + T] = v[:min(T, Mtot - m0)]
    return torch.from_numpy(out.reshape(c.N, Ho, Wo, c.Co))


# ---- head -------------------------------------------------------------------------------------------------------------

HeadCase = namedtuple("HeadCase", "name B P C")
BIG, OVERFLOWING, TINY = 1e18, 1e20, 1e-20      # 1e18^2 fits float32, 1e20^2 does not; 1e-20^2 is far below the eps
HEAD_CASES = tuple([HeadCase(f"c{C}", 2, 5, C) for C in (1, WAVE - 1, WAVE + 1, 2 * WAVE + 2)] +
                   [HeadCase(f"p{P}", 2, P, WAVE + 1) for P in (3, 4, HP - 1, HP, HP + 1, 2 * HP + 1)] +
                   [HeadCase("b-max", BMAX, 5, WAVE + 1)])   # p5 at C = WAVE + 1 is case c65


@functools.lru_cache(maxsize=None)
def head_inputs(name):
    """-> (feats [2 B, P, C], lin [C]) float32 with the planted pixels: image 0 pixel 0 zero in both stacks, pixel 1 zero
    in the partner only; the last image pixel 0 BIG in one stack and OVERFLOWING in the other, pixel 1 TINY, and pixel
    P - 1 zero in the first stack only"""
    c = {q.name: q for q in HEAD_CASES}[name]
    g = torch.Generator().manual_seed(7000 + 977 * c.C + 13 * c.P + c.B)
    feats = torch.relu(torch.randn(2 * c.B, c.P, c.C, generator=g))
    lin = torch.rand(c.C, generator=g) / c.C
    last = c.B - 1
    feats[0, 0] = 0.0
    feats[c.B, 0] = 0.0
    feats[c.B, 1] = 0.0
    feats[last, 0] = BIG * (1.0 + torch.rand(c.C, generator=g))
    feats[c.B + last, 0] = OVERFLOWING * (1.0 + torch.rand(c.C, generator=g))
    if last > 0:                                                  # with B = 1 pixel 1 of the last image is image 0's
        feats[last, 1] = TINY * (1.0 + torch.rand(c.C, generator=g))
        feats[c.B + last, 1] = TINY * (1.0 + torch.rand(c.C, generator=g))
    feats[last, c.P - 1] = 0.0
    return feats, lin


@functools.lru_cache(maxsize=None)
def head_reference(name):
    """the longdouble statement of tests/test_gpu_lpips.py -> (value [B], bound [B])"""
    c = {q.name: q for q in HEAD_CASES}[name]
    feats, lin = head_inputs(name)
    f = feats.numpy().astype(np.longdouble)
    nrm = f / np.sqrt(np.longdouble(M.LPIPS_NORM_EPS) + (f * f).sum(axis=2, keepdims=True))
    terms = lin.numpy().astype(np.longdouble) * (nrm[:c.B] - nrm[c.B:]) ** 2
    return terms.sum(axis=(1, 2)), LC.gamma(c.P * c.C + 8, U64) * np.abs(terms).sum(axis=(1, 2))


def _butterfly(v):
    """lp_wave_sum over the last axis (64 lanes): every lane ends with the same bits"""
    lanes = np.arange(WAVE)
    o = WAVE // 2
    while o:
        v = v + v[..., lanes ^ o]
        o //= 2
    return v


def head_twin(name, mut=None):
    """lp_head_kernel + lp_sum_kernel in numpy float64: the lanes of a wave over the channels, the waves over the pixels
    of a workgroup's HP, the waves' sums in wave order, the workgroups' partials in index order"""
    c = {q.name: q for q in HEAD_CASES}[name]
    feats, lin = head_inputs(name)
    full = -(-c.C // WAVE) * WAVE
    sums = np.float32 if mut == "head_norms_in_float32" else np.float64
    f = np.zeros((2 * c.B, c.P, full))
    f[..., :c.C] = feats.numpy()
    w = np.zeros(full)
    w[:c.C] = lin.numpy()
    if mut == "head_channel_tail_dropped":
        f[..., (c.C // WAVE) * WAVE:] = 0.0
        w[(c.C // WAVE) * WAVE:] = 0.0
    eps = 0.0 if mut == "head_eps_omitted" else M.LPIPS_NORM_EPS
    out = np.zeros(c.B)
    with np.errstate(all="ignore"):
        for b in range(c.B):
            v = 0.0
            for p0 in range(0, c.P, HP):
                wsum = np.zeros(HEAD_WAVES)
                for wave in range(HEAD_WAVES):
                    acc = 0.0
                    for p in range(p0 + wave, min(p0 + HP, c.P), HEAD_WAVES):
                        a, d = f[b, p].reshape(-1, WAVE), f[c.B + b, p].reshape(-1, WAVE)
                        s0, s1 = np.zeros(WAVE, dtype=sums), np.zeros(WAVE, dtype=sums)
                        for trip in range(a.shape[0]):
                            s0 = s0 + a[trip].astype(sums) * a[trip].astype(sums)
                            s1 = s1 + d[trip].astype(sums) * d[trip].astype(sums)
                        n0 = np.sqrt(eps + np.float64(_butterfly(s0)[0]))
                        n1 = np.sqrt(eps + np.float64(_butterfly(s1)[0]))
                        s = np.zeros(WAVE)
                        for trip in range(a.shape[0]):
                            dd = a[trip] / n0 - d[trip] / n1
                            s = s + w.reshape(-1, WAVE)[trip] * (dd * dd)
                        acc = acc + _butterfly(s)[0]
                    wsum[wave] = acc
                part = wsum[0]
                for wave in range(1, HEAD_WAVES):
                    part = part + wsum[wave]
                v = v + part
            out[b] = v
    return out


def head_inside(got, name):
    """-> (ok, worst error / bound); a pixel whose terms are all zero has bound 0 and must give 0"""
    want, bound = head_reference(name)
    err = np.abs(np.asarray(got).astype(np.longdouble) - want)
    ok = bool(np.all(np.isfinite(np.asarray(got, dtype=np.float64))) and np.all(err <= bound))
    with np.errstate(all="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
    return ok, float(np.max(ratio))


# ---- the mutations of the twins, each with the family it belongs to ----------------------------------------------------

MUTATIONS = {
    "conv_last_partial_step_dropped": "conv",
    "conv_prefetch_guard_one_step_late": "conv",
    "conv_tap_clamped_to_edge": "conv",
    "conv_image_from_tile_first_row": "conv",
    "pack_later_sweeps_dropped": "pack",
    "pack_later_counts_dropped": "pack",
    "pool_nan_rule_removed": "pool",
    "head_channel_tail_dropped": "head",
    "head_eps_omitted": "head",
    "head_norms_in_float32": "head",
}


def twin_failures(family, mut=None):
    """names of the cases of `family` whose twin (with `mut` planted) misses its check"""
    failed = []
    if family == "pack":
        w = LC.weights()
        for c in PACK_CASES:
            pred, target, want = pack_inputs(c)
            act, bad = pack_reference(pred, target, w)
            got, counts = pack_twin(pred, target, w, mut)
            if not (torch.equal(bits(got), bits(act)) and counts == bad == want):
                failed.append(c.name)
    elif family == "pool":
        for c in POOL_CASES:
            x = pool_input(c.name)
            if not same_with_nans(pool_twin(x, mut), pool_reference(x)):
                failed.append(c.name)
    elif family == "conv":
        for c in CONV_CASES:
            if not conv_check(conv_twin(c.name, mut), *conv_reference(c.name))[0]:
                failed.append(c.name)
    elif family == "head":
        for c in HEAD_CASES:
            if not head_inside(head_twin(c.name, mut), c.name)[0]:
                failed.append(c.name)
    else:
        raise KeyError(family)
    return failed


# ---- the whole metric -------------------------------------------------------------------------------------------------

E2E_SQUARE = math.isqrt(E // 3) + 1            # the smallest square image whose 3 H W values exceed one sweep (592)
# (H, W, B): the batch at the launch limit; the pack and both pools past their caps; one sweep of the pack and a little
E2E_CASES = ((L.LPIPS_MIN_SIDE, L.LPIPS_MIN_SIDE, BMAX), (E2E_SQUARE, E2E_SQUARE, 3), (2 * EW, E // (3 * 2 * EW) + 1, 1))


def e2e_launch_sizes(H, W, B):
    """values per launch: the pack (per image), the two pools (all 2 B images), and the head's workgroups per image"""
    (h1, w1), (h2, w2), (h3, w3) = M.lpips_map_sizes(H, W)[:3]
    return {"pack": 3 * H * W, "pool1": 2 * B * h2 * w2 * 64, "pool2": 2 * B * h3 * w3 * 192, "head1_groups": -(-h1 * w1 // HP)}


def layer_values(pred, target, dtype):
    """the host definition per layer -> ([B, 5] spatial means, [B] their sum in layer order), float64 tensors holding
    `dtype` results: metrics.lpips_per_image with the five terms kept apart"""
    pred, target = M._lpips_operands(pred, target)
    B = pred.shape[0]
    w = LC.weights()
    taps = M.lpips_features(torch.cat((pred, target)), w, dtype)
    total = torch.zeros(B, dtype=dtype)
    layers = []
    for f, lin in zip(taps, M._lpips_tensors(w, pred.device, dtype)[3]):
        f = f / torch.sqrt(M.LPIPS_NORM_EPS + torch.sum(f ** 2, dim=1, keepdim=True))
        v = (((f[:B] - f[B:]) ** 2) * lin).sum(dim=1).mean(dim=(1, 2))
        layers.append(v)
        total = total + v
    return torch.stack(layers, dim=1).double(), total.double()


@functools.lru_cache(maxsize=None)
def e2e_reference():
    """-> ({(H, W, B): (pred, target, float64 layers [B, 5], float64 totals [B])} for E2E_CASES, gap_layers [5],
    gap_total): the largest |float32 - float64| of the host definition per layer and for the total, over lpips_cases'
    set and over E2E_CASES"""
    gap_l, gap_t = np.zeros(M.LPIPS_LAYERS), 0.0

    def measure(pred, target):
        nonlocal gap_l, gap_t
        l64, t64 = layer_values(pred, target, torch.float64)
        l32, t32 = layer_values(pred, target, torch.float32)
        gap_l = np.maximum(gap_l, (l32 - l64).abs().max(dim=0).values.numpy())
        gap_t = max(gap_t, float((t32 - t64).abs().max()))
        return l64.numpy(), t64.numpy()

    for H, W in LC.E2E_SIZES:
        for B in LC.E2E_BATCHES:
            measure(*LC.image_pair(H, W, B))
    cases = {}
    for H, W, B in E2E_CASES:
        pred, target = LC.image_pair(H, W, B)
        cases[(H, W, B)] = (pred, target) + measure(pred, target)
    return cases, gap_l, gap_t
