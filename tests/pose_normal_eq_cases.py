"""Shared cases and the yardstick of the pose normal equations (unerf_pose_normal_eq_accumulate / _finish, include/unerf.h).

Yardstick: the terms w J_a J_b, w r J_a and w r r of every used (pixel, channel), formed from the float32 inputs exactly as
the header states them (r = (double)val - (double)target is a float64 value) and summed in numpy.longdouble (>= 63 mantissa
bits; fractions.Fraction where the platform's long double is no wider than a double), together with sum |term| per entry.

Bound, derived and not measured: |got - ref| <= (3 + A) 2^-53 sum |term| on every entry of H, g and chi2.  A is the longest
chain of float64 additions an entry passes through in the kernel and the reducer (lib.pose_neq_chain: a thread's PPT pixels x C
channels, two butterflies of 6, the waves of both workgroups in order, a reducer thread's share of the tile rows): every
addition contributes a relative 2^-53 of a partial sum that is at most sum |term|.  The 3 covers a term's own roundings
(w J_a or w r, the exact product inside the fma is not rounded, and the yardstick's long-double arithmetic)."""
from dataclasses import dataclass
from fractions import Fraction
from typing import Optional

import numpy as np

from uncertainty_nerf_gs_amd import lib as L

TILE = L.POSE_NEQ_TILE
LD = np.longdouble
WIDE = np.finfo(LD).nmant >= 63
NS = (1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
CS = (1, 3, 5)
PS = (1, 6, 7, 12)
OPTIONS = [(w, m, r) for w in (None, "n", "nc") for m in (False, True) for r in (False, True)]


@dataclass(frozen=True)
class Case:
    N: int
    C: int
    P: int
    weights: Optional[str]      # None | "n" ([N]) | "nc" ([N,C])
    mask: bool
    resid: bool                 # val / target given
    seed: int

    @property
    def id(self):
        return f"N{self.N}-C{self.C}-P{self.P}-w{self.weights or '0'}-m{int(self.mask)}-r{int(self.resid)}"


def all_cases():
    """every (N, C, P) with the weight / mask / residual options cycling through their 12 combinations, and all 12 of them at
    every (C, P) of the largest N (four tiles, the last one of five pixels)"""
    out, k = [], 0
    for N in NS:
        for C in CS:
            for P in PS:
                if N == NS[-1]:
                    out += [Case(N, C, P, *o, seed=1000 + len(out) + i) for i, o in enumerate(OPTIONS)]
                else:
                    out.append(Case(N, C, P, *OPTIONS[k % len(OPTIONS)], seed=1000 + len(out)))
                    k += 5          # 5 and 12 are coprime: every option combination meets every residue
    return out


def make_inputs(c: Case):
    """seeded float32 inputs of a case -> dict(jac [N,C,P], val, target [N,C] | None, weight [N] | [N,C] | None, mask [N] uint8 | None)"""
    g = np.random.default_rng(c.seed)
    jac = (g.standard_normal((c.N, c.C, c.P)) * np.exp(g.uniform(-3, 3, (c.N, 1, 1)))).astype(np.float32)
    val = g.uniform(0, 1, (c.N, c.C)).astype(np.float32) if c.resid else None
    target = (val + 0.1 * g.standard_normal((c.N, c.C))).astype(np.float32) if c.resid else None
    weight = None
    if c.weights:
        weight = np.exp(g.uniform(-2, 2, (c.N,) if c.weights == "n" else (c.N, c.C))).astype(np.float32)
        weight.reshape(-1)[3::7] = 0.0                # a zero weight is a used term that adds nothing
    mask = (g.uniform(0, 1, c.N) < 0.8).astype(np.uint8) if c.mask else None
    return dict(jac=jac, val=val, target=target, weight=weight, mask=mask)


def exact_inputs(N, C, P, seed):
    """the exact family: integer J and r in [-8, 8], w in {0.5, 1, 2} -- every float64 product and partial sum is an integer
    multiple of 0.5 far below 2^53, so ANY summation order gives the same bits"""
    g = np.random.default_rng(seed)
    jac = g.integers(-8, 9, (N, C, P)).astype(np.float32)
    val = g.integers(-4, 5, (N, C)).astype(np.float32)
    target = g.integers(-4, 5, (N, C)).astype(np.float32)
    weight = g.choice(np.array([0.5, 1.0, 2.0], np.float32), (N, C))
    mask = (g.uniform(0, 1, N) < 0.9).astype(np.uint8)
    return dict(jac=jac, val=val, target=target, weight=weight, mask=mask)


def exact_reference(inp):
    """the exact family in integers (everything doubled once so the weights are integers) -> H, g, chi2 as float64"""
    keep = inp["mask"].astype(bool)
    J = inp["jac"].astype(np.int64)[keep]
    r = (inp["val"].astype(np.int64) - inp["target"].astype(np.int64))[keep]
    w2 = np.rint(inp["weight"][keep] * 2).astype(np.int64)
    H2 = np.einsum("nc,nca,ncb->ab", w2, J, J)
    g2 = np.einsum("nc,nc,nca->a", w2, r, J)
    c2 = int((w2 * r * r).sum())
    return H2 / 2.0, g2 / 2.0, c2 / 2.0, int(keep.sum()) * J.shape[1]


def term_tables(inp):
    """-> (keep [N,C] bool: the used terms, skipped: the count of skipped terms, w, r, J as float64 of the kernel's values)"""
    jac = inp["jac"]
    N, C, _ = jac.shape
    J = jac.astype(np.float64)
    ok = np.isfinite(J).all(-1)
    w = np.ones((N, C))
    if inp.get("weight") is not None:
        w = np.broadcast_to(inp["weight"].astype(np.float64).reshape(N, -1), (N, C)).copy()
        ok &= np.isfinite(w) & ~(w < 0)
    r = np.zeros((N, C))
    if inp.get("val") is not None:
        with np.errstate(invalid="ignore"):
            r = inp["val"].astype(np.float64) - inp["target"].astype(np.float64)
        ok &= np.isfinite(r)
    live = np.ones(N, bool) if inp.get("mask") is None else inp["mask"].astype(bool)
    keep = ok & live[:, None]
    return keep, int((~ok & live[:, None]).sum()), w, r, J


def _sums(wv, a, b):
    """sum_t wv_t a_t[i] b_t[j] and the same of absolute values; long double, or exact fractions where that is no wider"""
    if WIDE:
        A = (a.astype(LD) * wv.astype(LD)[:, None])
        return A.T @ b.astype(LD), np.abs(A).T @ np.abs(b.astype(LD))
    S = np.zeros((a.shape[1], b.shape[1]), object)
    SA = np.zeros((a.shape[1], b.shape[1]), object)
    for t in range(a.shape[0]):
        for i in range(a.shape[1]):
            wa = Fraction(float(wv[t])) * Fraction(float(a[t, i]))
            for j in range(b.shape[1]):
                v = wa * Fraction(float(b[t, j]))
                S[i, j] += v
                SA[i, j] += abs(v)
    return S, SA


def reference(inp, drop_tile=None, weight_twice=False):
    """The yardstick.  -> dict(H, g, chi2: long double (or Fraction) sums; H_abs, g_abs, chi2_abs: sum |term|; n_used,
    n_skipped; N, C).  drop_tile / weight_twice are the planted mutations of the self-check."""
    keep, skipped, w, r, J = term_tables(inp)
    if drop_tile is not None:
        keep = keep.copy()
        keep[drop_tile * TILE:(drop_tile + 1) * TILE] = False
    if weight_twice:
        w = w * w
    wv, rv, Jv = w[keep], r[keep], J[keep]
    have_r = inp.get("val") is not None
    H, Ha = _sums(wv, Jv, Jv)
    g, ga = _sums(wv, rv[:, None], Jv) if have_r else (np.zeros((1, J.shape[2]), LD),) * 2
    c, ca = _sums(wv, rv[:, None], rv[:, None]) if have_r else (np.zeros((1, 1), LD),) * 2
    return dict(H=H, g=g[0], chi2=c[0, 0], H_abs=Ha, g_abs=ga[0], chi2_abs=ca[0, 0], n_used=int(keep.sum()), n_skipped=skipped,
                N=J.shape[0], C=J.shape[1])


def bound_factor(N_frame, C):
    return (3 + L.pose_neq_chain(N_frame, C)) * 2.0 ** -53


def _f(x):
    return np.vectorize(float, otypes=[LD])(x) if not WIDE else np.asarray(x, LD)


def excess(got, ref, N_frame=None):
    """got: dict(information, gradient, chi2) float64 -> the largest |got - ref| / bound over every entry (<= 1 passes; an
    entry with sum |term| == 0 must be exactly 0), and that entry's name"""
    fac = LD(bound_factor(ref["N"] if N_frame is None else N_frame, ref["C"]))
    worst, where = 0.0, ""
    for name, g, r, a in (("H", got["information"], ref["H"], ref["H_abs"]), ("g", got["gradient"], ref["g"], ref["g_abs"]),
                          ("chi2", np.array(got["chi2"]), np.array(ref["chi2"]), np.array(ref["chi2_abs"]))):
        err = np.abs(np.asarray(g, np.float64).astype(LD) - _f(r))
        b = fac * _f(a)
        ratio = np.where(b > 0, err / np.where(b > 0, b, 1), np.where(err > 0, np.inf, 0.0))
        if float(ratio.max()) > worst:
            worst, where = float(ratio.max()), f"{name}{list(np.unravel_index(int(ratio.argmax()), ratio.shape))}"
    return worst, where


def einsum_f64(inp):
    """the torch route a caller has today: float64 einsum over the used terms -> dict(information, gradient, chi2)"""
    import torch
    keep, _, w, r, J = term_tables(inp)
    wt = torch.from_numpy(np.where(keep, w, 0.0))
    Jt = torch.from_numpy(np.where(keep[..., None], J, 0.0))
    rt = torch.from_numpy(np.where(keep, r, 0.0))
    return dict(information=torch.einsum("nc,nca,ncb->ab", wt, Jt, Jt).numpy(), gradient=torch.einsum("nc,nc,nca->a", wt, rt, Jt).numpy(),
                chi2=float((wt * rt * rt).sum()))
