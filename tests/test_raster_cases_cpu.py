"""The hand-built rasteriser cases of tests/raster_cases.py, checked without a GPU: every case builds within the builder's
conditions (at most 3 % of its splats zeroed, at most 3 rounds, no placed splat zeroed, its structural facts -- all asserted by
the builder on the float64 reference alone), and the fp32 oracle SO.rasterize agrees with rasterize_f64 on them: final_idx
exactly, image and transmittance within 2e-6 (2.5 x the worst difference measured when the cases were designed, 8e-7; colours
lie in [0, 1)).  That is what lets tests/test_gpu_splat_raster_edges.py hold the kernel to the reference on every pixel."""
import numpy as np
import pytest

import raster_cases as RC
from oracle import splat_oracle as SO


@pytest.mark.parametrize("key", list(RC.ALL))
def test_case_builds_and_fp32_oracle_agrees(key):
    c = RC.ALL[key]()
    assert c.rounds <= RC.MAX_ROUNDS and len(c.zeroed) <= RC.MAX_ZEROED * c.N
    assert not np.isin(c.zeroed, c.protected).any() and np.all(c.opac[c.zeroed] == 0)
    assert np.array_equal(c.bins[:, 1] - c.bins[:, 0], c.lengths) and len(c.gids) == sum(c.lengths)
    assert not np.isnan(c.xys).any() and not np.isnan(c.conics).any() and not np.isnan(c.opac).any()
    pix, T, fidx, nbl = c.ref
    pix32, T32, fidx32 = c.ref32
    assert np.array_equal(fidx, fidx32)
    e_img, e_T = np.abs(pix32 - pix).max(), np.abs(T32 - T).max()
    print(f"{key}: {c.N} splats, {len(c.zeroed)} zeroed in {c.rounds} rounds, E32 image {e_img:.2e} T {e_T:.2e}, "
          f"blended pairs per pixel <= {nbl.max()}")
    assert e_img <= 2e-6 and e_T <= 2e-6
    assert key == "A1x1" or nbl.max() >= 10          # (neither of the two listed splats reaches the one pixel of 1 x 1)


@pytest.mark.parametrize("key", ["A41x57", "B"])
def test_bounded_reference(key):
    """the bounded pass stops where the first pass ended, so it blends the same pairs: same transmittance, index and count"""
    c = RC.ALL[key]()
    (pix, T, fidx, nbl), (pix32, T32, fidx32) = RC.bounded_ref(key)
    assert np.array_equal(T, c.ref[1]) and np.array_equal(fidx, c.ref[2]) and np.array_equal(nbl, c.ref[3])
    assert np.array_equal(T32, c.ref32[1]) and np.array_equal(fidx32, c.ref32[2])
    assert np.abs(pix32 - pix).max() <= 2e-6


def test_grazing_pairs_are_reported():
    """one splat on one pixel: alpha on 1/255, sigma cancelling to ~0, and transmittance on the stop are each reported"""
    bins, px = np.int32([[0, 2]]), np.float32([[0.5, 0.5], [0.5, 0.5]])
    run = lambda xys, conics, opac, ids=(0, 1): SO.rasterize_f64(np.int32(ids), bins, xys, np.float32(conics), np.ones((2, 1)),
                                                               np.float32(opac), 1, 1)
    flat = [[0, 0, 0], [0, 0, 0]]
    assert list(run(px, flat, [0.5, 0.25])[4]) == []
    assert list(run(px, flat, [0.5, 1.0004 / 255])[4]) == [1] and list(run(px, flat, [0.5, 1.002 / 255])[4]) == []
    # sigma = (1e4 * 1 + 1e4 * 1) / 2 - 1e4 * 1 = 0 from terms of 1e4: fp32 could make it negative
    assert list(run(np.float32([[1.5, 1.5], [0.5, 0.5]]), [[1e4, -1e4, 1e4], [0, 0, 0]], [0.5, 0.5])[4]) == [0]
    # T after both = 0.01 * (1 - 0.99) = 1e-4: on the stop; the bounded pass has no stop to graze
    out = run(px, flat, [0.99, 0.99])
    assert list(out[4]) == [1] and out[3][0, 0] in (1, 2)
    assert list(SO.rasterize_f64(np.int32([0, 1]), bins, px, np.float32(flat), np.ones((2, 1)), np.float32([0.99, 0.99]), 1, 1,
                                 stop_idx=np.int32([[1]]))[4]) == []
    # a pixel that has stopped visits nothing more: the grazing splat behind two stoppers is not reported
    bins3 = np.int32([[0, 3]])
    got = SO.rasterize_f64(np.int32([0, 0, 1]), bins3, px, np.float32(flat), np.ones((2, 1)), np.float32([2.0, 1.0004 / 255]), 1, 1)
    assert list(got[4]) == [] and got[2][0, 0] == 0 and abs(got[1][0, 0] - 1e-3) < 1e-6
