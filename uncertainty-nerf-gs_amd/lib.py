"""ctypes binding of libunerf (include/unerf.h).

The library is built in-tree by ``build_library()`` (called from ``__graft_entry__.build()``)
with ``hipcc --offload-arch=gfx950``.  There is no Python/CPU fallback: if the shared
object is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
# UNERF_LIB: another build of the same ABI, for A/B timing on one box (benchmarks/ab_bench.sh); unset in normal use
LIB_PATH = os.environ.get("UNERF_LIB") or os.path.join(CSRC, "libunerf.so")
SOURCES = ["unerf_nerf.hip", "unerf_splat.hip", "unerf_metrics.hip", "unerf_lpips.hip"]
# -amdgpu-mfma-vgpr-form: gfx950 has one unified register file; let the MFMAs write their accumulators to
# ordinary VGPRs so ReLU / dropout / the next layer's B operand read them without v_accvgpr_read copies
# (97 copies per tile in the K-pass kernel, which is VALU-issue-bound; rocprof r1_04).
# -fno-slp-vectorize: the one KNOWN trigger of run-to-run differences in the split-f16 field kernels is code the SLP
# vectoriser makes (packed v_pk_mul_f32 forms of the position x scale products in front of the hash): an experiment
# build with fused lerps in the field kernels' grid blend differed from launch to launch with it and repeated bit for bit
# without it (docs/experiments.md, profiles/r5_exp_blend_defect.jsonl).  The shipped sources never showed the defect, but the flag costs
# nothing (same frame times, same bits: every hot loop is written on explicit 2-vectors) and removes the trigger class.
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared",
               "-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form"]
# The compiler the kernels' hazard placement (hand-placed wait states inside inline assembly, the internal
# -amdgpu-mfma-vgpr-form switch) was validated with: tests/test_gpu_repeatability.py on MI355X.  Another version builds,
# with a warning -- rerun that test before trusting it.
VALIDATED_HIPCC = "HIP version: 7.2"


class UnerfError(RuntimeError):
    pass


def _source_digest(csrc: str = CSRC) -> str:
    """Content hash of everything a build reads: the flags, every .hip / .hpp / .inc of `csrc` (by name, sorted -- a new
    header counts without being listed anywhere) and include/unerf.h."""
    import hashlib
    h = hashlib.sha256(" ".join(HIPCC_FLAGS).encode())
    names = sorted(n for n in os.listdir(csrc) if n.endswith((".hip", ".hpp", ".inc")))
    for f in [os.path.join(csrc, n) for n in names] + [os.path.join(INCLUDE, "unerf.h")]:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def compile_command(out: str, extra_args=(), replace: Optional[tuple] = None) -> list:
    """The one hipcc command line of a libunerf build: HIPCC_FLAGS, `extra_args` (-D...), every entry of SOURCES.
    replace = (name, path): `path` is compiled in place of csrc/<name> (a patched copy: benchmarks/probe_source.py), with
    csrc/ on the include path so that the copy finds the texts it includes."""
    paths = {s: os.path.join(CSRC, s) for s in SOURCES}
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + HIPCC_FLAGS + list(extra_args) + ["-I", INCLUDE]
    if replace is not None:
        name, path = replace
        if name not in paths:
            raise UnerfError(f"{name} is not one of {SOURCES}")
        paths[name] = path
        cmd += ["-I", CSRC]
    return cmd + ["-o", out] + [paths[s] for s in SOURCES]


def compile_library(out: str, extra_args=(), replace: Optional[tuple] = None, verbose: bool = False) -> str:
    """Compile all of SOURCES for gfx950 into `out` (compile_command) and run the ISA hazard check on the result, which
    is removed if the check refuses it.  The product build and every A/B variant (benchmarks/build_variant.py) come
    through here."""
    cmd = compile_command(out, extra_args, replace)
    ver = subprocess.run([cmd[0], "--version"], capture_output=True, text=True).stdout
    if VALIDATED_HIPCC not in ver:
        import warnings
        warnings.warn(f"libunerf: building with {ver.splitlines()[0] if ver else cmd[0]!r}; the kernels were validated with "
                      f"'{VALIDATED_HIPCC}*' (run tests/test_gpu_repeatability.py on the GPU before trusting this build)")
    if verbose:
        print(" ".join(cmd))
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise UnerfError("hipcc failed:\n" + res.stdout + res.stderr)
    # the listing of what was just built: no MFMA may read a VGPR within two wait states of the VALU instruction that
    # writes it (the compiler guarantees that for its own instructions, nobody does for inline assembly: isa_check.py)
    if not os.environ.get("UNERF_SKIP_ISA_CHECK"):
        from . import isa_check
        try:
            isa_check.check_library(out, verbose=verbose)
        except isa_check.IsaHazard as e:
            os.remove(out)
            raise UnerfError(f"libunerf: refused by the ISA check -- {e}")
        except (FileNotFoundError, subprocess.CalledProcessError) as e:
            import warnings
            warnings.warn(f"libunerf: ISA check skipped ({e})")
    return out


def build_library(force: bool = False, verbose: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 into csrc/libunerf.so (cross-compiles without a GPU).
    Up-to-date-ness is a content hash of sources + flags (mtimes do not survive being copied to the GPU
    box); concurrent callers (one process per GPU) serialise on a lock file and the library is
    replaced atomically, so nobody dlopens a half-written file."""
    import fcntl
    if os.environ.get("UNERF_LIB"):
        # an explicitly chosen build (A/B timing): never rebuilt from the in-tree sources, used as it is
        if not os.path.exists(LIB_PATH):
            raise UnerfError(f"UNERF_LIB={LIB_PATH} does not exist")
        return LIB_PATH
    digest, stamp = _source_digest(), LIB_PATH + ".sha256"

    def fresh():
        return os.path.exists(LIB_PATH) and os.path.exists(stamp) and open(stamp).read().strip() == digest

    if not force and fresh():
        return LIB_PATH
    with open(LIB_PATH + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and fresh():   # another rank built it while we waited
                return LIB_PATH
            tmp = f"{LIB_PATH}.tmp.{os.getpid()}"
            compile_library(tmp, verbose=verbose)
            os.replace(tmp, LIB_PATH)
            with open(stamp, "w") as f:
                f.write(digest)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return LIB_PATH


class TcnnLevel(C.Structure):
    """include/unerf.h: unerf_tcnn_level"""
    _fields_ = [("scale", C.c_float), ("res", C.c_uint32), ("offset", C.c_uint32), ("size", C.c_uint32),
                ("dense", C.c_uint32)]


class DensityNet(C.Structure):
    _fields_ = [
        ("table", C.c_void_p), ("scalings", C.c_void_p), ("L", C.c_int), ("log2T", C.c_int),
        ("w0t", C.c_void_p), ("b0", C.c_void_p), ("w1t", C.c_void_p), ("b1", C.c_void_p), ("hidden", C.c_int),
        ("dense", C.c_void_p), ("n_dense", C.c_int), ("dense_off", C.c_int * 8), ("dense_dim", C.c_int * 8),
        ("tcnn_levels", C.c_void_p), ("use_aabb", C.c_int), ("aabb", C.c_float * 6), ("grid_half", C.c_int),
    ]


class FieldParams(C.Structure):
    _fields_ = [
        ("mode", C.c_int),
        ("table", C.c_void_p), ("scalings", C.c_void_p), ("L", C.c_int), ("log2T", C.c_int),
        ("w0t", C.c_void_p), ("b0", C.c_void_p), ("w1t", C.c_void_p), ("b1", C.c_void_p), ("out1", C.c_int),
        ("h0t", C.c_void_p), ("hb0", C.c_void_p), ("h1t", C.c_void_p), ("hb1", C.c_void_p),
        ("h2t", C.c_void_p), ("hb2", C.c_void_p),
        ("average_init_density", C.c_float), ("beta_min", C.c_float), ("sh_remap", C.c_int),
        ("K", C.c_int), ("seed", C.c_uint32), ("p_drop", C.c_float),
        ("ws_density", C.c_void_p), ("ws_rgb", C.c_void_p), ("n_lap", C.c_int), ("lap_mask_density", C.c_int),
        ("mfma_blob", C.c_void_p), ("lap_blob", C.c_void_p),
        ("tcnn_levels", C.c_void_p),
        ("mfma16_blob", C.c_void_p), ("lap16_blob", C.c_void_p),
        ("image_width", C.c_int), ("sample_major", C.c_int), ("drop_sites", C.c_int), ("lap_softplus", C.c_int), ("use_aabb", C.c_int),
        ("aabb", C.c_float * 6), ("f16_single", C.c_int), ("overflow_flag", C.c_void_p),
        ("h0_full_t", C.c_void_p), ("hb0_raw", C.c_void_p), ("app_embed", C.c_void_p),
        ("lap_chunk_rays", C.c_int), ("lap_sets", C.c_int), ("n_lap_rgb", C.c_int), ("packed_out", C.c_int),
        ("grid_half", C.c_int),
        ("hidden", C.c_int), ("hidden_color", C.c_int), ("geo_dim", C.c_int), ("feat_per_level", C.c_int), ("app_dim", C.c_int),
    ]


class KeepMasks(C.Structure):
    """include/unerf.h: unerf_keep_masks (explicit MC-dropout keep masks, unerf_field_fwd_masked)"""
    _fields_ = [("site", C.c_void_p * 4), ("pass_stride", C.c_int64), ("sample_offset", C.c_int64)]


NERF_MAX_VIEWS = 16                               # include/unerf.h: UNERF_NERF_MAX_VIEWS


class RayViews(C.Structure):
    """include/unerf.h: unerf_ray_views (several whole views of one image size in one launch)"""
    _fields_ = [("n_views", C.c_int32), ("rays_per_view", C.c_int64), ("seed", C.c_uint32 * NERF_MAX_VIEWS)]


class LaplaceViews(C.Structure):
    """include/unerf.h: unerf_laplace_views (per-view sample-set base and depth seed of the LAPLACE *_views entry points)"""
    _fields_ = [("set_base", C.c_int32 * NERF_MAX_VIEWS), ("depth_seed", C.c_uint32 * NERF_MAX_VIEWS)]


class RayCamera(C.Structure):
    """include/unerf.h: unerf_ray_camera (one camera of unerf_generate_rays_views)"""
    _fields_ = [("c2w", C.c_float * 12), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("distortion", C.c_float * 6)]


class EnsKey(C.Structure):
    """include/unerf.h: unerf_ens_key (one input key of unerf_ensemble_reduce)"""
    _fields_ = [("channels", C.c_int32), ("stride", C.c_int32), ("n", C.c_int64)]


class EnsOut(C.Structure):
    """include/unerf.h: unerf_ens_out (one output block per view of unerf_ensemble_reduce)"""
    _fields_ = [("stat", C.c_int32), ("key", C.c_int32), ("aux", C.c_int32), ("reserved", C.c_int32), ("offset", C.c_int64)]


LPIPS_LAYERS = 5                                  # include/unerf.h: UNERF_LPIPS_LAYERS


class LpipsWeightsC(C.Structure):
    """include/unerf.h: unerf_lpips_weights (device pointers to the repacked AlexNet, the scaling constants by value)"""
    _fields_ = [("conv_w", C.c_void_p * LPIPS_LAYERS), ("conv_b", C.c_void_p * LPIPS_LAYERS), ("lin_w", C.c_void_p * LPIPS_LAYERS),
                ("shift", C.c_float * 3), ("scale", C.c_float * 3)]


ABI_VERSION = 1420                                # include/unerf.h: UNERF_ABI_VERSION (struct layouts / argument lists)
FIELD_ACTIVE, FIELD_MCDROPOUT, FIELD_LAPLACE = 0, 1, 2
SPACING_PIECEWISE, SPACING_UNIFORM = 0, 1         # include/unerf.h: UNERF_SPACING_*
BG_LAST_SAMPLE, BG_NONE, BG_COLOR = 0, 1, 2       # include/unerf.h: UNERF_BG_*
# include/unerf.h: UNERF_CAMERA_* = nerfstudio's CameraType values of the camera models the ray kernel restates
CAMERA_PERSPECTIVE, CAMERA_FISHEYE, CAMERA_EQUIRECTANGULAR, CAMERA_ORTHOPHOTO = 1, 2, 3, 8
CAMERA_TYPES = (CAMERA_PERSPECTIVE, CAMERA_FISHEYE, CAMERA_EQUIRECTANGULAR, CAMERA_ORTHOPHOTO)
RASTER_NO_CULL = 1                                # include/unerf.h: UNERF_RASTER_NO_CULL
BUILD_TRUNK_FOLD, BUILD_LAP_EXP2 = 1, 2   # include/unerf.h: UNERF_BUILD_*
DROP_TRUNK, DROP_HEAD0, DROP_HEAD1, DROP_HEADIN = 1, 2, 4, 8     # include/unerf.h: UNERF_DROP_*

_vp, _i, _i64, _f, _u32 = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_uint32
_fp = C.POINTER(C.c_float)

# name -> (restype, argtypes); must list every symbol include/unerf.h declares
SIGNATURES = {
    "unerf_last_error": (C.c_char_p, []),
    "unerf_version": (_i, []),
    "unerf_build_flags": (_i, []),
    "unerf_device_count": (_i, []),
    "unerf_generate_rays": (_i, [_fp, _f, _f, _f, _f, _fp, _i, _i, _i, _i64, _i64, _vp, _vp, _vp, _vp]),
    "unerf_ray_box_bins": (_i, [_vp, _vp, _i64, _fp, _fp, _f, _f, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "unerf_ray_planes_bins": (_i, [_vp, _vp, _i64, _f, _f, _i, _vp, _i, _vp, _vp]),
    "unerf_hashgrid_fwd": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp]),
    "unerf_hashgrid_fwd_tcnn": (_i, [_vp, _vp, C.POINTER(TcnnLevel), _i64, _i, _vp, _vp, _vp]),
    "unerf_hashgrid_fwd_tcnn_half": (_i, [_vp, _vp, C.POINTER(TcnnLevel), _i64, _i, _vp, _vp]),
    "unerf_proposal_density": (_i, [_vp, _vp, _vp, _i64, _i64, _i, _f, _f, _i, C.POINTER(DensityNet), _f, _vp, _i64, _i, _vp]),
    "unerf_weights_pdf_resample": (_i, [_vp, _vp, _i64, _i64, _i, _f, _f, _i, _vp, _i, _f, _f, _vp, _vp, _vp, _vp,
                                        _i64, _i64, _vp]),
    "unerf_field_fwd": (_i, [_vp, _vp, _vp, _i64, _i, _f, _f, _i, _i64, C.POINTER(FieldParams), _vp, _vp, _vp, _vp, _vp,
                             _vp]),
    "unerf_field_fwd_masked": (_i, [_vp, _vp, _vp, _i64, _i, _f, _f, _i, _i64, C.POINTER(FieldParams), _vp, _vp, _vp, _vp, _vp,
                                    C.POINTER(KeepMasks), _vp]),
    "unerf_pack_keep_bits": (_i, [_vp, _i64, _i, _vp, _vp]),
    "unerf_mc_keep_bits": (_i, [_u32, _i, _i64, _i64, _i, _i, _f, _vp, _i64, _vp]),
    "unerf_field_gather": (_i, [_vp, _vp, _vp, _i64, _i, _f, _f, _i, _vp, _vp, _i, _i, _vp, _vp]),
    "unerf_laplace_depth_weights": (_i, [_vp, _vp, _vp, _i64, _i, _f, _f, _i, _vp, _i, _u32, _i64, _vp, _vp]),
    "unerf_laplace_ggn_workspace_bytes": (C.c_size_t, [_i64, _i]),
    "unerf_laplace_ggn_diag": (_i, [_vp, _vp, _vp, _i64, _i, _f, _f, _i, C.POINTER(FieldParams), _i, _fp, _vp, C.c_size_t,
                                    _vp, _vp, _vp]),
    "unerf_pose_grad": (_i, [_vp, _vp, _vp, _i64, _i, _f, _f, _i, C.POINTER(FieldParams), _i, _fp, _fp, _vp, _vp, _vp]),
    "unerf_pose_jacobian": (_i, [_vp, _vp, _vp, _i64, _i, _f, _f, _i, C.POINTER(FieldParams), _i, _fp, _fp, _i, _fp, _i, _vp, _vp, _vp,
                                 _vp, _vp]),
    "unerf_pose_grad_mc": (_i, [_vp, _vp, _vp, _i64, _i, _f, _f, _i, _i64, C.POINTER(FieldParams), C.POINTER(KeepMasks), _i, _fp,
                                _fp, _vp, _vp, _vp]),
    "unerf_pose_grad_laplace": (_i, [_vp, _vp, _vp, _i64, _i, _f, _f, _i, _i64, C.POINTER(FieldParams), _i, _fp, _fp, _vp, _vp, _vp]),
    "unerf_composite_var":(_i, [_vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _f, _f, _i, _vp, _i64, _i64, _i, _fp, _vp, _vp, _vp]),
    "unerf_composite_moments": (_i, [_vp, _vp, _vp, _i, _i64, _i, _f, _f, _i, _vp, _i64, _i64, _i, _fp, _vp, _vp, _vp, _vp]),
    "unerf_composite_var_planes": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _f, _f, _i, _vp, _i64, _i64, _i, _fp, _vp, _vp, _vp]),
    "unerf_composite_moments_planes": (_i, [_vp, _vp, _vp, _i, _i64, _i, _f, _f, _i, _vp, _i64, _i64, _i, _fp, _vp, _vp,
                                            _vp, _vp]),
    "unerf_generate_rays_views": (_i, [C.POINTER(RayCamera), _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "unerf_weights_pdf_resample_views": (_i, [_vp, _vp, _i64, _i64, _i, _f, _f, _i, _vp, _i, _f, _f, _vp, _vp, _vp, _vp,
                                              C.POINTER(RayViews), _i64, _vp]),
    "unerf_composite_var_views": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _f, _f, _i, _vp, C.POINTER(RayViews), _i64, _i, _fp,
                                       _vp, _vp, _vp]),
    "unerf_composite_moments_views": (_i, [_vp, _vp, _vp, _i, _i64, _i, _f, _f, _i, _vp, C.POINTER(RayViews), _i64, _i, _fp, _vp,
                                           _vp, _vp, _vp]),
    "unerf_field_fwd_views": (_i, [_vp, _vp, _vp, _i64, _i, _f, _f, _i, C.POINTER(RayViews), C.POINTER(FieldParams), _vp, _vp, _vp,
                                   _vp, _vp, C.POINTER(KeepMasks), _vp]),
    "unerf_field_fwd_laplace_views": (_i, [_vp, _vp, _vp, _i64, _i, _f, _f, _i, C.POINTER(RayViews), C.POINTER(LaplaceViews),
                                           C.POINTER(FieldParams), _vp, _vp, _vp, _vp, _vp]),
    "unerf_laplace_depth_weights_views": (_i, [_vp, _vp, _vp, _i64, _i, _f, _f, _i, _vp, _i, C.POINTER(RayViews),
                                               C.POINTER(LaplaceViews), _vp, _vp]),
    "unerf_moments": (_i, [_vp, _i, _i64, _i, _vp, _vp, _vp]),
    "unerf_ensemble_reduce": (_i, [_vp, _i, _i, _i, C.POINTER(EnsKey), C.POINTER(EnsOut), _i, _i64, _vp, _i64, _vp]),
    "unerf_image_metrics_workspace_bytes": (C.c_size_t, [_i64]),
    "unerf_image_metrics": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _f, _f, C.POINTER(C.c_double), _i, C.POINTER(C.c_double), _i,
                                 _i, _vp, C.c_size_t, _vp, _vp]),
    "unerf_image_metrics_batch_workspace_bytes": (C.c_size_t, [_i64, _i]),
    "unerf_image_metrics_batch": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _f, _f, C.POINTER(C.c_double), _i, C.POINTER(C.c_double),
                                       _i, _i, _vp, C.c_size_t, _vp, _vp]),
    "unerf_eval_images_workspace_bytes": (C.c_size_t, [_i]),
    "unerf_eval_images_batch": (_i, [_vp, _vp, _vp, _i64, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "unerf_lpips_pack": (_i, [_vp, _vp, _i64, _i, C.POINTER(LpipsWeightsC), _vp, _vp, _vp]),
    "unerf_conv2d_bias_relu": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "unerf_maxpool3s2": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "unerf_lpips_head": (_i, [_vp, _vp, _i64, _i, _i, _vp, C.c_size_t, _vp, _i64, _vp]),
    "unerf_lpips_workspace_bytes": (C.c_size_t, [_i, _i, _i]),
    "unerf_lpips_batch": (_i, [_vp, _vp, _i, _i, _i, C.POINTER(LpipsWeightsC), _vp, C.c_size_t, _vp, _vp]),
    "unerf_splat_project": (_i, [_vp, _vp, _f, _vp, _fp, _f, _f, _f, _f, _i, _i, _i, _f, _i64, _vp, _vp, _vp, _vp,
                                 _vp, _vp, _vp, _vp]),
    "unerf_splat_project_raw": (_i, [_vp, _vp, _f, _vp, _fp, _f, _f, _f, _f, _i, _i, _i, _f, _i64, _vp, _i, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _vp]),
    "unerf_splat_sh_colors": (_i, [_i, _vp, _fp, _vp, _vp, _f, _i64, _vp, _vp, _vp]),
    "unerf_splat_sh_colors_split": (_i, [_i, _vp, _fp, _vp, _vp, _vp, _f, _i64, _vp, _vp, _vp]),
    "unerf_splat_shade_inputs": (_i, [_i, _vp, _fp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _i64, _i, _vp, _vp, _vp]),
    "unerf_splat_sort_workspace_bytes": (_i64, [_i64, _i64]),
    "unerf_splat_count_intersects": (_i, [_vp, _i64, _vp, _vp, _i64, _vp]),
    "unerf_splat_bin_sort": (_i, [_vp, _vp, _vp, _vp, _i64, _i64, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "unerf_splat_rasterize": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp,
                                   _vp]),
    "unerf_splat_alpha_normalize": (_i, [_vp, _i, _i, _vp, _i64, _vp, _i, _vp]),
    "unerf_splat_normalize_outputs": (_i, [_vp, _i, _i, _vp, _i64, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "unerf_splat_depth_sqdiff": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i64, _vp, _vp]),
    "unerf_splat_project_batch": (_i, [_vp, _vp, _f, _vp, _fp, _i, _i, _i, _i, _f, _i64, _vp, _i, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _vp, _vp, _vp]),
    "unerf_splat_shade_inputs_batch": (_i, [_i, _vp, _fp, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _i64, _i, _vp, _vp, _vp]),
    "unerf_splat_sort_workspace_bytes_batch": (_i64, [_i, _i64, _i64]),
    "unerf_splat_count_intersects_batch": (_i, [_vp, _vp, _i, _i64, _vp, _vp, _vp, _i64, _vp]),
    "unerf_splat_bin_sort_batch": (_i, [_vp, _vp, _vp, _vp, _i, _i64, C.POINTER(C.c_int64), _i, _i, _i, _vp, _vp, _vp, _vp, _vp,
                                        _i64, _vp]),
    "unerf_splat_rasterize_batch": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp,
                                         _vp, _vp]),
    "unerf_splat_normalize_outputs_batch": (_i, [_vp, _i, _i, _vp, _i, _i64, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "unerf_splat_depth_sqdiff_batch": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i64, _vp, _vp]),
    "unerf_splat_pose_tangents": (_i, [_vp, _vp, _vp, _i64, _fp, _f, _f, _f, _f, _i, _i, _f, _vp, _vp]),
    "unerf_splat_pose_grad": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _fp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "unerf_splat_pose_tangents_proj": (_i, [_vp, _vp, _vp, _i64, _fp, _i, _vp, _vp]),
    "unerf_splat_pose_jacobian": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp,
                                       _vp]),
    "unerf_splat_pose_ptangents_batch": (_i, [_vp, _vp, _vp, _fp, _i, _i64, _vp, _i, _i, _i, _f, _vp, _vp]),
    "unerf_splat_pose_jacobian_batch": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _i, _i, _i, _i, _i,
                                             _vp, _vp, _vp, _vp]),
    "unerf_pose_normal_eq_workspace_bytes": (C.c_size_t, [_i64, _i]),
    "unerf_pose_normal_eq_accumulate": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _i64, _i, _i, _i64, _i64, _vp, C.c_size_t, _vp]),
    "unerf_pose_normal_eq_finish": (_i, [_vp, C.c_size_t, _i64, _i, _vp, _vp]),
}
# include/unerf.h: UNERF_METRICS_* (flags of unerf_image_metrics, layout of its row of float64 results)
METRICS_AUSE, METRICS_AUCE, METRICS_NLL, METRICS_SSIM = 1, 2, 4, 8
METRICS_ALL = METRICS_AUSE | METRICS_AUCE | METRICS_NLL | METRICS_SSIM
METRICS_AUCE_OFF, METRICS_AUSE_OFF, METRICS_ROW, METRICS_MAX_CUTS = 16, 144, 656, 128
METRICS_MAX_IMAGES = 64                           # include/unerf.h: UNERF_METRICS_MAX_IMAGES (unerf_image_metrics_batch)
# include/unerf.h: UNERF_LPIPS_* (row of unerf_lpips_batch, tiles of its kernels)
LPIPS_ROW, LPIPS_BAD_OFF, LPIPS_MIN_SIDE = 11, 10, 31
LPIPS_CONV_TILE_M, LPIPS_CONV_TILE_N, LPIPS_HEAD_PIXELS = 64, 64, 64
LPIPS_CONV_STEP_K, LPIPS_EW_THREADS, LPIPS_EW_MAX_WG = 16, 256, 4096
# include/unerf.h: UNERF_ENS_* (bounds and statistics of unerf_ensemble_reduce)
ENS_MAX_KEYS, ENS_MAX_MEMBERS, ENS_MAX_CHANNELS = 32, 64, 64
ENS_MEAN, ENS_VAR, ENS_VAR_CMEAN, ENS_ALEA_CMEAN, ENS_EPI_ALEA, ENS_EPI_ALEA_SQRT, ENS_STD_CMEAN = range(7)
ENS_ALEA_STATS = (ENS_ALEA_CMEAN, ENS_EPI_ALEA, ENS_EPI_ALEA_SQRT)
SPLAT_MAX_VIEWS = 16                              # include/unerf.h: UNERF_SPLAT_MAX_VIEWS
SPLAT_VIEW_FLOATS = 19                            # include/unerf.h: UNERF_SPLAT_VIEW_FLOATS
SPLAT_BATCH_MAX_TILES = 11999                     # include/unerf.h: UNERF_SPLAT_BATCH_MAX_TILES
SPLAT_POSE_Q = 6                                  # include/unerf.h: UNERF_SPLAT_POSE_Q
SPLAT_POSE_GRAD_BATCH = 128                       # include/unerf.h: UNERF_SPLAT_POSE_GRAD_BATCH
SPLAT_POSE_PROJ_ROWS, SPLAT_POSE_MAX_P = 7, 12    # include/unerf.h: UNERF_SPLAT_POSE_PROJ_ROWS, UNERF_SPLAT_POSE_MAX_P
# include/unerf.h: UNERF_POSE_NEQ_* (geometry of unerf_pose_normal_eq_accumulate / _finish)
POSE_NEQ_THREADS, POSE_NEQ_PPT, POSE_NEQ_REDUCE_THREADS = 256, 4, 256
POSE_NEQ_TILE = POSE_NEQ_THREADS * POSE_NEQ_PPT
POSE_NEQ_MAX_P, POSE_NEQ_MAX_C = 12, 5


def pose_neq_row(P: int) -> int:
    """include/unerf.h: UNERF_POSE_NEQ_ROW -- H [P,P] | g [P] | chi2 | n_used | n_skipped"""
    return P * P + P + 3


def pose_neq_ws_row(P: int) -> int:
    """include/unerf.h: UNERF_POSE_NEQ_WS_ROW -- a tile's row of partials: the packed upper triangle of H, g, chi2, two counts"""
    return P * (P + 1) // 2 + P + 3


def pose_neq_chain(N_frame: int, C: int) -> int:
    """The longest chain of float64 additions an entry of H, g or chi2 passes through (include/unerf.h states the geometry):
    a thread's PPT pixels x C channels, the wave butterfly (6), the waves of the workgroup in order; then, in the reducer, a
    thread's share of the tile rows, its butterfly and its waves in order."""
    tiles = -(-int(N_frame) // POSE_NEQ_TILE)
    return (POSE_NEQ_PPT * int(C) + 6 + (POSE_NEQ_THREADS // 64 - 1)
            + -(-tiles // POSE_NEQ_REDUCE_THREADS) + 6 + (POSE_NEQ_REDUCE_THREADS // 64 - 1))


def splat_pose_pw(P: int) -> int:
    """include/unerf.h: UNERF_SPLAT_POSE_PW -- the compiled column width of the contracted splat tangents"""
    return 6 if P <= 6 else 12

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """dlopen csrc/libunerf.so and type every entry point.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime (torch/lib/libamdhip64.so); it must be the one that
    # initialises the device, so import torch before dlopen-ing libunerf (same SONAME -> shared).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise UnerfError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    # the ctypes Structures and argument lists above are one ABI: a library of another one (UNERF_LIB pointing at a
    # stale A/B build) would be driven with mismatched layouts and answer with silent garbage
    got = lib.unerf_version()
    if got != ABI_VERSION:
        raise UnerfError(f"{LIB_PATH}: ABI version {got}, this binding is written for {ABI_VERSION} "
                         "(rebuild: python -c 'import __graft_entry__ as g; g.build()')")
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().unerf_last_error().decode(errors="replace")
        raise UnerfError(f"{what or 'libunerf'} failed (rc={rc}): {msg}")


def require_gpu() -> None:
    if load().unerf_device_count() <= 0:
        raise UnerfError("no HIP device visible: libunerf has no CPU path")
