"""The "f16" K-pass field kernel (field_kernel_mfma16<MCDROPOUT, 0, false, true, true>, the bench headline's field_fwd) gives
the same bits as the kernel it replaced: a seeded K = 8 frame's raw field_fwd outputs, plain and packed rows, hashed and
compared with the digest recorded from the previous kernel (tests/golden/kpass_f16_digest.json).  The parity tests compare
with the oracle within a tolerance; this one holds the register-budget and instruction-selection work on that kernel to
"not one output bit changes"."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kpass_f16_digest.json")
NEAR, FAR = 0.05, 1000.0
H, W, S = 64, 96, 48


def kpass_f16_digest(dev) -> str:
    from oracle import nerf_oracle as O
    from uncertainty_nerf_gs_amd import ops, synthetic
    t = synthetic.make_scene_tensors(seed=0, kind="mcdropout", log2T=14, prop_log2T=12)
    sd = synthetic.scene_to_device(t, dev, K=8, seed=1234, p_drop=0.2)
    sd.field.precision = "f16"
    o, d, _ = O.generate_rays(synthetic.orbit_c2w(0.3), 80.0, 80.0, W / 2, H / 2, H, W)
    R = H * W
    # spacing-domain bin edges, monotonic in [0, 1), a different offset per ray (no RNG: the same on every machine)
    u = (np.arange(R, dtype=np.float64) * 0.6180339887) % 1.0
    sb = ((np.arange(S + 1)[None, :] + u[:, None]) / (S + 1)).astype(np.float32)
    od, dd, sbd = o.reshape(-1, 3).contiguous().to(dev), d.reshape(-1, 3).contiguous().to(dev), torch.from_numpy(sb).to(dev)
    h = hashlib.sha256()
    dens, rgb, _, _ = ops.field_fwd(od, dd, sbd, sd.field, NEAR, FAR, ray_offset=17)
    _, rows, _, _ = ops.field_fwd(od, dd, sbd, sd.field, NEAR, FAR, image_width=W, packed=True)
    torch.cuda.synchronize()
    for x in (dens, rgb, rows):
        h.update(x.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def test_kpass_f16_field_outputs_match_the_recorded_digest(dev):
    with open(GOLDEN) as f:
        want = json.load(f)["sha256"]
    assert kpass_f16_digest(dev) == want


if __name__ == "__main__":   # prints the digest of the library in use (UNERF_LIB selects another build)
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from uncertainty_nerf_gs_amd import lib
    lib.build_library()
    print(kpass_f16_digest(torch.device("cuda:0")))
