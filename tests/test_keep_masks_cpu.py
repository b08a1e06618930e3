"""Explicit MC-dropout keep masks, the parts that need no GPU: the C ABI surface (symbols, struct layout, refusals before
any launch), the host draw in the reference's order against torch's own nn.Dropout modules, and the statement that the
rendered uncertainty has the same distribution under the counter generator's masks as under torch's Bernoulli."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT


def test_keep_mask_symbols_and_struct_layout(lib, tmp_path):
    h = lib.load()
    for name in ("unerf_field_fwd_masked", "unerf_pack_keep_bits", "unerf_mc_keep_bits"):
        assert name in lib.SIGNATURES and getattr(h, name) is not None
    # sizeof / offsetof as a C compiler sees include/unerf.h (the method of test_ctypes_structs_match_the_header_layout)
    ct = lib.KeepMasks
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "unerf.h"', 'int main(void) {',
             '  printf("SIZEOF %zu\\n", sizeof(unerf_keep_masks));']
    lines += [f'  printf("{f} %zu\\n", offsetof(unerf_keep_masks, {f}));' for f, _ in ct._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    rows = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    assert len(rows) == len(ct._fields_) + 1
    for row in rows:
        what, val = row.split()
        assert (C.sizeof(ct) if what == "SIZEOF" else getattr(ct, what).offset) == int(val), row
    assert C.sizeof(ct) == 48 and ct.site.size == 32
    assert h.unerf_version() == 1420          # the mode is additive: same ABI version, unerf_field_params untouched


def _params(lib, **kw):
    fp = lib.FieldParams()
    for name in ("table", "scalings", "w0t", "b0", "w1t", "b1", "h0t", "hb0", "h1t", "hb1", "h2t", "hb2", "mfma16_blob", "mfma_blob"):
        setattr(fp, name, 1)
    fp.L, fp.log2T, fp.mode, fp.out1, fp.K, fp.p_drop = 16, 19, lib.FIELD_MCDROPOUT, 16, 4, 0.2
    for k, v in kw.items():
        setattr(fp, k, v)
    return fp


def _masks(lib, sites=(1, 0, 1, 0), stride=10 * 48, offset=0):
    km = lib.KeepMasks()
    for i, on in enumerate(sites):
        km.site[i] = 1 if on else None
    km.pass_stride, km.sample_offset = stride, offset
    return km


def test_field_fwd_masked_refusals_come_before_any_launch(lib):
    """every refusal of include/unerf.h: unerf_field_fwd_masked returns -1 with its reason -- on a machine without a GPU, so
    nothing was launched -- and R = 0 returns 0"""
    h = lib.load()

    def call(fp, km, R=10, S=48):
        return h.unerf_field_fwd_masked(1, 1, 1, R, S, 0.05, 1000.0, 0, 0, C.byref(fp), None, 1, 1, None, None,
                                        None if km is None else C.byref(km), None)

    def refused(fp, km, text, **kw):
        assert call(fp, km, **kw) == -1
        assert text in h.unerf_last_error(), h.unerf_last_error()

    refused(_params(lib), None, b"null masks")
    refused(_params(lib, mode=lib.FIELD_ACTIVE, out1=17), _masks(lib), b"MCDROPOUT mode")
    refused(_params(lib, K=0), _masks(lib), b"K=0")
    refused(_params(lib), _masks(lib, sites=(1, 0, 0, 0)), b"site HEAD1 is active")            # drop_sites 0 = TRUNK | HEAD1
    refused(_params(lib, drop_sites=7), _masks(lib, sites=(1, 0, 1, 0)), b"site HEAD0 is active")
    refused(_params(lib), _masks(lib, sites=(1, 1, 1, 0)), b"site HEAD0, which is not active")
    refused(_params(lib, drop_sites=1), _masks(lib, sites=(1, 0, 1, 0)), b"site HEAD1, which is not active")
    refused(_params(lib), _masks(lib, stride=10 * 48 - 1), b"pass_stride=479 < sample_offset + R*S")
    refused(_params(lib), _masks(lib, stride=10 * 48, offset=1), b"pass_stride=480 < sample_offset + R*S")
    refused(_params(lib, drop_sites=9, h0_full_t=1, hb0_raw=1, app_embed=1), _masks(lib, sites=(1, 0, 0, 1)),
            b"UNERF_DROP_HEADIN is out of scope")
    refused(_params(lib, hidden=32, hidden_color=64, geo_dim=15, feat_per_level=2, app_dim=32), _masks(lib),
            b"any-width kernel is out of scope")
    refused(_params(lib, L=8), _masks(lib), b"any-width kernel is out of scope")
    # R = 0: UNERF_OK without touching a pointer, like every other entry point
    assert call(_params(lib), _masks(lib, stride=0), R=0) == 0
    # the two helpers validate before launching too, and zero counts are no-ops
    assert h.unerf_pack_keep_bits(None, 0, 64, None, None) == 0
    assert h.unerf_pack_keep_bits(None, 5, 64, None, None) == -1 and b"null pointer" in h.unerf_last_error()
    assert h.unerf_pack_keep_bits(1, 5, 0, 1, None) == -1 and b"n_units=0" in h.unerf_last_error()
    assert h.unerf_mc_keep_bits(1, 4, 0, 0, 0, 64, 0.2, None, 0, None) == 0
    assert h.unerf_mc_keep_bits(1, 4, 0, 10, 0, 64, 0.2, 1, 9, None) == -1 and b"pass_stride=9" in h.unerf_last_error()
    assert h.unerf_mc_keep_bits(1, 4, 0, 10, 4, 64, 0.2, 1, 10, None) == -1 and b"stream_id=4" in h.unerf_last_error()
    assert h.unerf_mc_keep_bits(1, 0, 0, 10, 0, 64, 0.2, 1, 10, None) == -1 and b"K=0" in h.unerf_last_error()


@pytest.mark.parametrize("p", [0.2, 0.5])
@pytest.mark.parametrize("sites", [5, 7])
def test_host_draw_equals_fresh_dropout_modules_in_the_reference_order(lib, sites, p):
    """models.iter_torch_keep_draws with a CPU generator seeded s == a fresh set of nn.Dropout(p) modules in train mode run
    in the reference's order after torch.manual_seed(s): pass k outermost (mcdropout_models.py:116-119 renders the whole
    bundle per pass), the chunks of the bundle in order, inside a chunk trunk -> HEAD0 -> HEAD1."""
    from keep_mask_stats import torch_keep_masks
    Kp, rays, S, chunk, seed = 3, 70, 6, 32, 1234          # 70 = 2 * 32 + 6: a ragged last chunk
    got = torch_keep_masks(seed, Kp, rays, S, chunk, sites, p)
    mods = [torch.nn.Dropout(p).train() if (sites >> i) & 1 else None for i in range(3)]
    want = [[[] for _ in range(Kp)] if m is not None else None for m in mods]
    torch.manual_seed(seed)
    for k in range(Kp):
        for start in range(0, rays, chunk):
            n = min(chunk, rays - start)
            for i, m in enumerate(mods):
                if m is not None:
                    want[i][k].append(m(torch.ones(n * S, 64)) != 0)
    for i in range(3):
        assert (got[i] is None) == (want[i] is None)
        if got[i] is not None:
            for k in range(Kp):
                assert got[i][k].shape == (rays * S, 64)
                assert torch.equal(got[i][k], torch.cat(want[i][k])), (i, k)
            assert abs(float(torch.stack(got[i]).float().mean()) - (1 - p)) < 0.02
    # under torch.autocast("cpu") the module sees a bfloat16 input and keeps the same units
    torch.manual_seed(seed)
    with torch.autocast("cpu"):
        x = torch.nn.functional.linear(torch.ones(32 * S, 8), torch.ones(64, 8))
        assert x.dtype == torch.bfloat16
        first = next(i for i in range(3) if mods[i] is not None)
        assert torch.equal(mods[first](x) != 0, got[first][0][:32 * S])


def test_rgb_std_under_counter_masks_and_torch_bernoulli_have_the_same_distribution(lib):
    """The rendered MC-dropout uncertainty does not depend on WHICH generator made the masks (VERDICT next-round 3(a)).
    fp32 oracle, K = 8, p = 0.2, sites TRUNK | HEAD1, an 8 x 12 frame on proposal-sampled bins: per-pixel rgb_std over
    n = 64 seeds of the counter generator (oracle.mc_keep_mask, seeds 1000 + i) and over n = 64 torch generators (seeds
    5000 + i), compared with the three gates of keep_mask_stats (quantiles of the null distributions).
    Power: the t gate fails with probability > 0.8 for a shift of the mean rgb_std of (4 + 1) standard errors of the
    difference of the two group means -- the printed line states that standard error (about 0.3 % of the mean rgb_std
    here, i.e. a relative shift of roughly 1.5 % is caught); the per-pixel gate catches a shift of ~5.5 standard errors
    in any one pixel, the F gate a 2.4-fold variance of the frame means (e.g. masks correlated between the samples of a ray)."""
    import keep_mask_stats as KS
    from oracle import nerf_oracle as O
    sc = O.scene_from_tensors(KS.scene_tensors())
    o, d = KS.oracle_rays()
    sampled = O._sample(sc, o, d)
    R, S = o.shape[0], sc.num_nerf
    sidx = (np.arange(R)[:, None] * S + np.arange(S)[None]).reshape(-1)
    a, b = [], []
    for i in range(KS.N_SEEDS):
        cm = lambda k, s=1000 + i: (torch.from_numpy(O.mc_keep_mask(s, k, sidx, 0, 64, KS.P_DROP)),
                                    torch.from_numpy(O.mc_keep_mask(s, k, sidx, 1, 64, KS.P_DROP)))
        a.append(KS.oracle_rgb_std(sc, o, d, sampled, cm).numpy())
        tm = KS.torch_keep_masks(5000 + i, KS.K, R, S, 1 << 15, KS.SITES, KS.P_DROP)
        b.append(KS.oracle_rgb_std(sc, o, d, sampled, lambda k: (tm[0][k], tm[2][k])).numpy())
    KS.report_and_gate("oracle: counter vs torch Bernoulli", np.stack(a), np.stack(b))
