/*
 * libunerf -- C ABI of the MI355X (gfx950) uncertainty-rendering hot path.
 *
 * The reference (AaltoML/uncertainty-nerf-gs) is pure Python and has no FFI of its
 * own: every number on its hot path is produced by nerfstudio 1.1.0 torch ops,
 * tiny-cuda-nn and gsplat 0.1.11 CUDA kernels that it *calls*.  Each entry point
 * below therefore replaces a call site of the reference (cited per function,
 * paths relative to /root/reference/nerfuncertainty) and is what a maintainer
 * would bind from the reference's Model/Field classes (INTEGRATION.md shows the
 * ctypes stubs).
 *
 * Conventions
 *   - every pointer is a caller-owned DEVICE pointer unless it says "host";
 *     the library never allocates, frees or retains caller memory
 *     (exception: unerf_splat_sort_workspace_bytes + caller-provided workspace);
 *   - `stream` is the caller's hipStream_t (NULL = default stream); no hidden sync;
 *   - all functions return 0 on success, <0 on error; unerf_last_error() gives
 *     a thread-local message;
 *   - fp32 everywhere; row-major; rays are in image row-major order;
 *   - a count of zero (R, N, count = 0: an empty chunk, a rank without views, a crop that keeps nothing) is a
 *     successful no-op and the per-element pointers may then be NULL; parameter structs and host pointers must
 *     still be valid.  Exceptions: unerf_splat_count_intersects / unerf_splat_bin_sort need N >= 1;
 *   - there is NO CPU implementation behind these symbols.
 */
#ifndef UNERF_H
#define UNERF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UNERF_OK 0
#define UNERF_ERR_ARG -1     /* bad argument / unsupported shape */
#define UNERF_ERR_HIP -2     /* HIP runtime error (launch, no device) */

const char* unerf_last_error(void);
/* Library/ABI version (major*1000+minor).  A binding built against this header must find exactly UNERF_ABI_VERSION
 * (struct layouts and argument lists change with it; uncertainty-nerf-gs_amd/lib.py::load checks). */
#define UNERF_ABI_VERSION 1420
int unerf_version(void);

/* Spacing function of the proposal sampler's initial sampler, passed behind every (near_plane, far_plane) pair:
 *   UNERF_SPACING_PIECEWISE  UniformLinDispPiecewiseSampler, nerfacto's default (proposal_initial_sampler="piecewise"):
 *                            s(x) = x/2 (x < 1) else 1 - 1/(2x); spacing bin b -> s^-1(b s(far) + (1 - b) s(near))
 *   UNERF_SPACING_UNIFORM    UniformSampler (proposal_initial_sampler="uniform", the reference's few-view configuration,
 *                            /root/reference/README.md:153): identity spacing, b -> b far + (1 - b) near
 * [UPSTREAM nerfstudio 1.1.0 NerfactoModel.populate_modules / ray_samplers.SpacedSampler]. */
#define UNERF_SPACING_PIECEWISE 0
#define UNERF_SPACING_UNIFORM 1

/* RGBRenderer(background_color=config.background_color) at eval (activenerfacto_model.py:98 -> nerfstudio 1.1.0
 * renderers.RGBRenderer.forward / combine_rgb), for the composite and GGN entry points:
 *   UNERF_BG_LAST_SAMPLE  "last_sample" (nerfacto default): comp + rgb[..., -1, :] (1 - accumulation)
 *   UNERF_BG_NONE         "random": at eval the composited colour is returned unblended
 *   UNERF_BG_COLOR        "white" / "black" (or any constant): comp + background_rgb (1 - accumulation);
 *                         background_rgb = 3 HOST floats
 * followed in every case by the eval-mode clamp to [0, 1]. */
#define UNERF_BG_LAST_SAMPLE 0
#define UNERF_BG_NONE 1
#define UNERF_BG_COLOR 2
/* Build switches that change what the operand blobs must look like (bit mask).  UNERF_BUILD_TRUNK_FOLD: the
 * MCDROPOUT split-f16 kernels expect the four trunk-out slabs of mfma16_blob folded (see unerf_field_params). */
#define UNERF_BUILD_TRUNK_FOLD 1
#define UNERF_BUILD_LAP_EXP2 2   /* lap16_blob rows carry their activation's base change (see unerf_field_params) */
int unerf_build_flags(void);
/* Number of visible HIP devices (<=0: none -> every other call fails with UNERF_ERR_HIP). */
int unerf_device_count(void);

/* ------------------------------------------------------------------ rays --
 * Replaces Cameras.generate_rays(camera_indices=0, keep_shape=True) + row-major
 * slicing used by get_outputs_for_camera (scripts/eval_uncertainty.py:1097,1127;
 * models/laplace/laplace_model.py:269-297, 403-415).
 * c2w: HOST pointer to 12 floats (3x4 row-major).  Rays [ray_start, ray_start+count)
 * of the H*W row-major image.  pixel_area may be NULL.
 * distortion: HOST pointer to the camera's 6 OPENCV lens parameters in nerfstudio's order (k1, k2, k3, k4, p1, p2 --
 * camera_utils.get_distortion_params, as the reference's dataparsers hand them to `Cameras`:
 * dataparsers/sparse_mipnerf360/sparse_mipnerf360_dataparser.py:113-125, 248-274; every `ns-process-data images` scene
 * of /root/reference/README.md:52-56 carries them), or NULL.  Non-zero parameters bend the rays the way
 * Cameras._generate_rays_from_coords does for a perspective camera: the image-plane coordinate ((x - cx) / fx,
 * -(y - cy) / fy) of the pixel centre AND of its +1-pixel x / y neighbours (which feed pixel_area) goes through
 * camera_utils.radial_and_tangential_undistort -- UNERF_UNDISTORT_ITERATIONS Newton steps on the 2x2 Jacobian of the
 * forward model, a step taken only where |det| > UNERF_UNDISTORT_EPS -- before it is rotated into the world.  NULL or
 * six zeros: no iteration runs (upstream's `(distortion_params != 0).any()` guard) and the rays are bit-for-bit those
 * of the distortion-free camera. */
#define UNERF_UNDISTORT_ITERATIONS 10
#define UNERF_UNDISTORT_EPS 1e-3f
/* camera_type: nerfstudio's CameraType value of the camera (cameras.py: PERSPECTIVE = 1, FISHEYE = 2, EQUIRECTANGULAR = 3,
 * ORTHOPHOTO = 8), as the reference's dataparsers hand it to `Cameras` (CAMERA_MODEL_TO_TYPE[meta["camera_model"]]:
 * dataparsers/sparse_mipnerf360/sparse_mipnerf360_dataparser.py:237-239, sparse/sparse_nerfstudio_dataparser.py:277-279,
 * nerfonthego, ood_mipnerf360, robustnerf alike).  Camera-frame direction of an (undistorted) image-plane coordinate (u, v)
 * [UPSTREAM-RECALL nerfstudio 1.1.0 Cameras._generate_rays_from_coords]:
 *   PERSPECTIVE      (u, v, -1)
 *   FISHEYE          theta = clip(|(u, v)|, 0, pi):  (u sin(theta) / theta, v sin(theta) / theta, -cos(theta))
 *                    (OPENCV_FISHEYE's k1..k4 act on (u, v) through the same undistortion as the perspective lens)
 *   EQUIRECTANGULAR  theta = -pi u, phi = pi (0.5 - v):  (-sin(theta) sin(phi), cos(phi), -cos(theta) sin(phi));
 *                    distortion parameters are ignored for this type, as upstream does
 *   ORTHOPHOTO       (0, 0, -1) for every pixel, the ORIGIN moves instead: c2w (u, v, 0, 1)
 * then rotated by c2w[:3,:3] and normalised (norm floored at 1e-7); pixel_area from the +1-pixel x / y neighbours as for
 * the perspective camera.  The other CameraType values (omnidirectional stereo, VR180, FISHEYE624) are refused. */
#define UNERF_CAMERA_PERSPECTIVE 1
#define UNERF_CAMERA_FISHEYE 2
#define UNERF_CAMERA_EQUIRECTANGULAR 3
#define UNERF_CAMERA_ORTHOPHOTO 8
int unerf_generate_rays(const float* c2w_host, float fx, float fy, float cx, float cy, const float* distortion_host,
                        int camera_type, int H, int W, int64_t ray_start, int64_t count, float* origins, float* directions,
                        float* pixel_area, void* stream);

/* Oriented crop box (`obb_box` of Model.get_outputs_for_camera / get_outputs_for_camera_unc,
 * models/laplace/laplace_model.py:403-415, models/ensemble/ensemble_pipeline.py:144-157): what
 * Cameras.generate_rays(..., obb_box=box) does to the bundle -- nears / fars from the ray / box slab test
 * (nerfstudio.utils.math.intersect_obb: t clamped to [0,1e10], a miss = 1e10 for both) -- expressed as per-ray
 * first-level spacing bins under the launch-wide planes (near, far):
 *   sbins[r,i] = (b_i s(far_r) + (1-b_i) s(near_r) - s(near)) / (s(far) - s(near)),  b = sbins_row [n+1].
 * Feed sbins [R,n+1] (stride n+1) to unerf_proposal_density / unerf_weights_pdf_resample; every later stage is
 * unchanged.  world_to_box: HOST 12 floats, inverse([R|T]) 3x4 row-major; half_extent: HOST 3 floats (S/2).
 * nears / fars [R] may be NULL.  Rays that miss: planes 1e10 as upstream; their samples collapse onto `far`
 * (upstream they are at infinity, pixels undefined), giving zero accumulation. */
int unerf_ray_box_bins(const float* origins, const float* directions, int64_t R, const float* world_to_box_host,
                       const float* half_extent_host, float near, float far, int spacing, const float* sbins_row, int n,
                       float* sbins, float* nears, float* fars, void* stream);
/* The same fold for a bundle that already carries planes (RayBundle.nears / fars [R], e.g. made by
 * camera.generate_rays(obb_box=...) on the nerfstudio side; SceneCollider.forward keeps planes that are set). */
int unerf_ray_planes_bins(const float* nears, const float* fars, int64_t R, float near, float far, int spacing,
                          const float* sbins_row, int n, float* sbins, void* stream);

/* ------------------------------------------------------------- hash grid --
 * Replaces HashEncoding(implementation="torch").forward called at
 * models/activenerfacto/activenerfacto_field.py:140-147,
 * models/mcdropout/mcdropout_fields.py:115-122, models/laplace/laplace_field.py:129-136.
 * xyz [N,3] in [0,1]; table [L<<log2T, 2]; scalings [L]; out [N, 2L].
 * out_idx (may be NULL) receives the 8 table-row indices per level, [N,L,8] int32,
 * corner order ccc,cfc,ffc,fcc,ccf,cff,fff,fcf (bit-exact bookkeeping check). */
int unerf_hashgrid_fwd(const float* xyz, const float* table, const float* scalings, int64_t N, int L,
                       int log2T, float* out, int32_t* out_idx, void* stream);

/* tiny-cuda-nn `HashGrid` layout, as nerfstudio's HashEncoding(implementation="tcnn") configures it (the
 * reference's default, models/activenerfacto/activenerfacto_field.py:89,146): `table` is then the flat fp32
 * `tcnn_encoding.params` vector viewed as rows of 2 features, and level l is described by one record
 * (host helper: uncertainty-nerf-gs_amd/ops.py::tcnn_grid_levels):
 *   scale  = exp2f(l * log2f(per_level_scale)) * base_res - 1     res = ceilf(scale) + 1
 *   size   = min(next_multiple(res^3, 8), 2^log2_hashmap_size)    rows of this level
 *   offset = sum of the sizes of the levels below                  dense = (res^3 <= size)
 * Lookup: pos = x*scale + 0.5, cell = floor(pos), w = pos - cell; corner k (bit d of k = +1 along dim d) has
 * row (x + y res + z res^2) mod size when dense, else (x ^ y*2654435761 ^ z*805459861) mod size, and weight
 * prod_d (bit ? w_d : 1 - w_d); the 8 corners are accumulated in corner order.  fp32 throughout (tcnn itself
 * interpolates fp16 copies of the same fp32 master parameters: documented divergence). */
typedef struct {
    float scale;
    uint32_t res, offset, size, dense;
} unerf_tcnn_level;

/* xyz [N,3] in [0,1]; params = tcnn_encoding.params (fp32, [rows][2]); levels_host [L]; out [N,2L];
 * out_idx (may be NULL) [N,L,8] int32 = absolute row indices in corner order k = 0..7. */
int unerf_hashgrid_fwd_tcnn(const float* xyz, const float* params, const unerf_tcnn_level* levels_host, int64_t N,
                            int L, float* out, int32_t* out_idx, void* stream);
/* The same lookup the way tiny-cuda-nn computes it when built with TCNN_HALF_PRECISION (its default on every GPU the
 * reference targets; kernel_grid in include/tiny-cuda-nn/encodings/grid.h with T = __half) -- what the reference's
 * HashEncoding(implementation="tcnn") call sites above return: params_half = the parameter vector cast to half
 * ([rows] half2, round to nearest even); positions and the three interpolation weights in fp32 as above; per corner
 * k = 0..7 the fp32 weight product ((w_x w_y) w_z) is rounded to half and result = fma(half weight, row, result) is a
 * HALF fused multiply-add per feature (__hfma2), result starting at 0.  out [N,2L] fp32 holding the half values (rows are
 * those of unerf_hashgrid_fwd_tcnn's out_idx). */
int unerf_hashgrid_fwd_tcnn_half(const float* xyz, const void* params_half, const unerf_tcnn_level* levels_host, int64_t N,
                                 int L, float* out, void* stream);

/* hash grid + small MLP (torch nn.Linear weights pre-transposed to [in][out]). */
typedef struct {
    const float* table;      /* [L<<log2T][2] */
    const float* scalings;   /* [L] */
    int L, log2T;
    const float* w0t;        /* [2L][hidden] */
    const float* b0;         /* [hidden] */
    const float* w1t;        /* [hidden][1] */
    const float* b1;         /* [1] */
    int hidden;              /* 16 (nerfacto proposal nets) or 64; 0 = use_linear=True (HashMLPDensityField's single
                                Linear on the grid features: w1t [2L] and b1 are that layer, w0t / b0 unused) */
    /* Optional dense re-indexing of the first n_dense (coarse) levels, n_dense <= 8 (0 = none).  Level l
       then has (dense_dim[l])^3 cells, dense_dim = scalings[l]+1, stored x-fastest from cell offset
       dense_off[l] in `dense` as float4 = { table[hash(x,y,z)], table[hash(x+1,y,z)] }: the same values the
       hashed lookup returns, but both x-neighbours of a cell edge arrive in ONE 16-byte load (4 instead of 8
       gather instructions per level; the texture-address unit bounds these kernels).  2 <= dense_dim <= 640 (32-bit
       byte offsets); ops.DENSE_LEVEL_BYTES makes copies of the levels up to resolution 128. */
    const float* dense;
    int n_dense;
    int dense_off[8];
    int dense_dim[8];
    /* NULL: nerfstudio torch HashEncoding (above).  Else DEVICE array [L] of level records: `table` is a
       tcnn-layout parameter vector (`scalings`, `log2T`, `dense*` are ignored). */
    const unerf_tcnn_level* tcnn_levels;
    /* use_aabb = 1: spatial_distortion = None (disable_scene_contraction, mcdropout_models.py:60-63): positions are
       normalised with SceneBox.get_normalized_positions, (x - aabb[0..2]) / (aabb[3..5] - aabb[0..2]), instead of
       SceneContraction(inf) followed by (x + 2) / 4.  aabb = {min xyz, max xyz}. */
    int use_aabb;
    float aabb[6];
    /* tcnn_levels only: 1 = `table` points at the HALF copy of the parameter vector ([rows] half2, 4 bytes per row) and
       the level is interpolated in tiny-cuda-nn's own half arithmetic (see unerf_hashgrid_fwd_tcnn_half); the features
       then enter the fp32 MLP as the half values they are.  0: fp32 rows, fp32 blend. */
    int grid_half;
} unerf_density_net;

/* -------------------------------------------------- proposal density --
 * Replaces HashMLPDensityField.density_fn as invoked by ProposalNetworkSampler
 * (call site models/activenerfacto/activenerfacto_model.py:89,
 * models/laplace/laplace_model.py:210,459).  Sample i of ray r sits at the mid-point of
 * spacing bins [i, i+1] (converted to euclidean with the spacing fn `spacing` = UNERF_SPACING_*
 * and near/far).  sbins: [R, n+1] with row stride `sbins_stride`
 * (0 = one shared row, the initial uniform bins).  density_out [R,n]. */
int unerf_proposal_density(const float* origins, const float* directions, const float* sbins,
                           int64_t sbins_stride, int64_t R, int n, float near_plane, float far_plane, int spacing,
                           const unerf_density_net* net /* host struct of device ptrs */,
                           float average_init_density, float* density_out,
                           int64_t ray_offset, int image_width /* scheduling hint, 0 = none: rays [ray_offset,
                           ray_offset + R) are consecutive pixels of a row-major image this wide; a wave then
                           evaluates an 8x8 pixel patch at one sample index.  Same results either way. */,
                           void* stream);

/* ------------------------------------------- weights + PDF resampling --
 * Replaces RaySamples.get_weights + PDFSampler.generate_ray_samples (eval branch) inside
 * ProposalNetworkSampler, and DepthRenderer("median") for prop_depth_i
 * (models/activenerfacto/activenerfacto_model.py:150-151).
 * u: [m+1] = linspace(0,1-1/(m+1),m+1)+1/(2(m+1)) (host computes it the torch way).
 * sbins_out [R,m+1]; prop_depth_out [R] (may be NULL); weights_out [R,n] (may be NULL).
 * clip_minmax (may be NULL): [ceil(R_total/chunk_rays)][2] floats, pre-set to {+inf,0};
 * receives per-chunk min/max of the NEW samples' mid-points (the bounds
 * DepthRenderer("expected") clips to); ray_offset = index of ray 0 inside the frame. */
int unerf_weights_pdf_resample(const float* density, const float* sbins, int64_t sbins_stride, int64_t R,
                               int n, float near_plane, float far_plane, int spacing, const float* u, int m,
                               float histogram_padding, float eps, float* sbins_out, float* prop_depth_out,
                               float* weights_out, float* clip_minmax, int64_t ray_offset,
                               int64_t chunk_rays, void* stream);

/* ------------------------------------------------------- main field --
 * Replaces, per mode:
 *  ACTIVE    ActiveNerfactoField.get_density + NerfactoField.get_outputs
 *            (models/activenerfacto/activenerfacto_field.py:162-215)
 *  MCDROPOUT NerfactoMCDropoutField.get_density + create_mlp heads, K stochastic passes
 *            (models/mcdropout/mcdropout_fields.py:110-174, mcdropout_models.py:116-119,
 *            utils.py:6-43); K=0 means dropout off, one pass.
 *  LAPLACE   NerfactoLaplaceField.forward_unc with is_inference=True
 *            (models/laplace/laplace_field.py:279-362, 365-485, 528-568): ws_* are the
 *            n_lap sampled last-layer parameter rows mu+randn*std ([out,in] row-major, bias).
 */
#define UNERF_FIELD_ACTIVE 0
#define UNERF_FIELD_MCDROPOUT 1
#define UNERF_FIELD_LAPLACE 2

typedef struct {
    int mode;
    /* hash grid (L=16 levels, F=2) */
    const float* table; const float* scalings; int L, log2T;
    /* trunk: w0t [32][64], b0[64]; w1t [64][out1], b1[out1]
       out1 = 17 ACTIVE (density, geo15, beta) | 16 MCDROPOUT | 15 LAPLACE (mlp_hidden) */
    const float* w0t; const float* b0; const float* w1t; const float* b1; int out1;
    /* colour head with the constant eval appearance embedding folded into the first bias:
       h0t [31][64] (rows: SH16 then geo15), hb0[64]; h1t [64][64], hb1[64]; h2t [64][3], hb2[3] */
    const float* h0t; const float* hb0; const float* h1t; const float* hb1; const float* h2t; const float* hb2;
    float average_init_density, beta_min;
    int sh_remap;            /* 0: SH on (d+1)/2 as the torch SHEncoding does; 1: tcnn ([-1,1]) */
    /* MCDROPOUT */
    int K; uint32_t seed; float p_drop;
    /* LAPLACE */
    const float* ws_density;  /* [n_lap][65]  */
    const float* ws_rgb;      /* [n_lap_rgb (n_lap when that is 0)][195] */
    int n_lap;
    int lap_mask_density;     /* 1: multiply the density mean by the box selector (the use_deterministic_density=True
                                 path, laplace_field.py:501-506 / :317-345, fed with n_lap copies of the mean row) */
    /* Optional (ACTIVE / MCDROPOUT): the same MLP weights pre-arranged as fp32-MFMA A-operand
       fragments (layout: uncertainty-nerf-gs_amd/ops.py::pack_field_mfma, UNERF_MFMA_BLOB_FLOATS
       floats).  When non-NULL the fused kernel runs its dense layers on v_mfma_f32_32x32x2_f32
       (exact fp32) with the weights resident in LDS; NULL selects the VALU kernel. */
    const float* mfma_blob;
    /* Optional (LAPLACE, with mfma_blob): the n_lap <= 128 sampled last-layer rows of both heads as MFMA A
       fragments (ops.py::pack_laplace_heads, UNERF_LAP_BLOB_FLOATS floats; streamed from L2, not LDS). */
    const float* lap_blob;
    /* NULL: nerfstudio torch HashEncoding.  Else DEVICE array [16] of tcnn level records: `table` is the flat
       tcnn-layout parameter vector of the main grid (`scalings` / `log2T` ignored). */
    const unerf_tcnn_level* tcnn_levels;
    /* Optional, preferred when present (all modes): the dense layers as SPLIT-F16 matrix operands
       (ops.py::pack_field_mfma16, same size as mfma_blob; LAPLACE additionally lap16_blob,
       ops.py::pack_laplace_heads16, UNERF_LAP_BLOB_FLOATS floats).  Every fp32 weight and activation is carried
       as hi = f16(x), lo = f16(x - hi) and hi*hi + hi*lo + lo*hi is accumulated in fp32 on
       v_mfma_f32_32x32x16_f16: fp32-equivalent results (relative deviation ~1e-7 from the exact kernels) at a
       third of the matrix-pipe time of the fp32-input MFMA, which runs at the vector rate.  NULL selects the
       exact-fp32 kernels above.  With UNERF_BUILD_TRUNK_FOLD (unerf_build_flags) MCDROPOUT expects the four
       trunk-out slabs folded: their second operand holds rows 0..15 = W_hi and rows 16..31 = W_lo, so the 16-row
        layer takes two MFMAs per k-step instead of three (ops.pack_field_mfma16(fold_trunk=True)).  With
       UNERF_BUILD_LAP_EXP2 lap16_blob's rows (weights and bias) carry the base change of their activation: density
       rows x log2(e) (unscaled when lap_softplus = 1), colour rows x -log2(e), and the kernel applies the bare hardware
       exp2 (padded rows: bias -1e30 for the density head, +1e30 for the colour heads -> they contribute 0). */
    const float* mfma16_blob;
    const float* lap16_blob;
    /* Scheduling hint, 0 = none: the rays [ray_offset, ray_offset + R) of this call are consecutive pixels of a
       row-major image `image_width` wide.  The matrix kernels then take 8x4 pixel patches (instead of 32
       consecutive pixels) as the 32 columns of a tile: fewer distinct cache lines per gather instruction.
       Results are identical with and without the hint. */
    int image_width;
    /* Output layout of the ACTIVE / MCDROPOUT matrix kernels.  0: density [B,R,S], rgb [B,R,S,3], aux [R,S] (the
       RaySamples layout).  1: sample-major planes density [B,S,R], rgb [B,S,3,R], aux [S,R]: a kernel tile is 32 rays
       at one sample slot, so its stores then fill whole 32-byte sectors instead of 4 bytes per cache line; consumed
       by unerf_composite_var_planes / unerf_composite_moments_planes. */
    int sample_major;
    /* MCDROPOUT: where the Dropout modules sit (mcdropout_fields.py:112-144 via create_mlp, utils.py:6-43).  0 = the
       reference default UNERF_DROP_TRUNK | UNERF_DROP_HEAD1 (density_dropout_layers=True, rgb_dropout_layers=[-1]).
       UNERF_DROP_TRUNK: after the trunk's hidden ReLU (density_dropout_layers); UNERF_DROP_HEAD0: in front of the
       colour head's Linear 1 (rgb_dropout_layers contains 1); UNERF_DROP_HEAD1: in front of its last Linear (contains
       2 or -1).  Mask streams 0 / 2 / 1 of the counter RNG.  With mfma16_blob the scale 1/(1-p) is expected folded
       into the layer behind each active site (ops.pack_field_mfma16).
       UNERF_DROP_HEADIN: in front of the colour head's Linear 0 (rgb_dropout_layers contains 0), i.e. on its 63 INPUTS
       [SH16 | geo15 | appearance32] -- mask stream 3.  The appearance block can then no longer ride in the bias, so this
       site needs h0_full_t / hb0_raw / app_embed below, and it is served by the VALU kernel only (any precision setting;
       roughly 10 x the time of the matrix kernels -- a rarely used configuration kept correct rather than fast). */
    int drop_sites;
    /* LAPLACE: 1 = density_activation "softplus" (laplace_model.py:151, laplace_field.py:323) instead of trunc_exp on
       the (sampled) density head (unerf_laplace_ggn_diag: dsigma/dpre = 1 - exp(-sigma) instead of sigma). */
    int lap_softplus;
    /* as unerf_density_net: 1 = normalise positions with the scene box instead of the contraction */
    int use_aabb;
    float aabb[6];
    /* 1 (with mfma16_blob / lap16_blob): REFERENCE-PRECISION dense layers -- one f16 product per MAC, fp32 accumulation:
       every operand is rounded to f16 once (the hi halves of the blobs, v_cvt_pk_f16_f32 of the activations) and the lo
       halves are not used.  That is the arithmetic of the Linear layers under torch.autocast(float16), which the
       reference forces at eval (models/mcdropout/mcdropout_models.py:86-92), and no narrower than tiny-cuda-nn's
       FullyFusedMLP (fp16 weights, activations and accumulators; the reference's default implementation="tcnn",
       models/activenerfacto/activenerfacto_field.py:89).  0: the split form above (fp32-equivalent).  Biases, the
       64 -> 3 colour layer and every activation function stay fp32 in both forms. */
    int f16_single;
    /* With mfma16_blob, DEVICE int32 (may be NULL): |= 1 when an f16 OPERAND of the dense layers overflowed (an activation
       beyond 65504).  f16_single: an output pre-activation (density logit, colour sums; LAPLACE: a sampled-head mean)
       comes out inf / NaN -- the trace such an activation leaves in this form, which has no lo halves to turn it into a
       NaN sample.  Split form: the pre-activations of a colour layer are NaN (hi = inf, lo = -inf make every unit of the
       next layer NaN, which the ReLU behind it could otherwise zero; trunk overflows reach the density as NaN and are
       flagged by the composite entry points).  Same word and same host protocol as the composite entry points'
       nonfinite_flag (render.OverflowGuard: fp32 re-render of the launch group). */
    int32_t* overflow_flag;
    /* UNERF_DROP_HEADIN only (else may be NULL): the colour head's first layer unfolded -- weights transposed
       [63][64] over the inputs [SH16 | geo15 | appearance32], its bias [64] WITHOUT the appearance term, and the eval
       appearance embedding [32] (zeros or the mean embedding, [UPSTREAM NerfactoField.get_outputs]). */
    const float* h0_full_t;
    const float* hb0_raw;
    const float* app_embed;
    /* LAPLACE: the reference draws a fresh set of last-layer samples in EVERY eval chunk of a frame -- sample_laplace
       runs inside get_outputs_unc, which get_outputs_for_camera_ray_bundle_unc calls per 32,768-ray chunk
       (models/laplace/laplace_model.py:432-443 -> laplace_field.py:331-339, 468-476, 545).  lap_chunk_rays > 0:
       ws_density [lap_sets][n_lap][65], ws_rgb [lap_sets][n_lap][195], lap_blob / lap16_blob
       [lap_sets][UNERF_LAP_BLOB_FLOATS] are STACKS of sets and ray g = ray_offset + r is evaluated with set
       g / lap_chunk_rays (every ray of the call must map below lap_sets).  lap_chunk_rays and ray_offset must be
       multiples of 32: the matrix kernels then take 32 consecutive rays as a tile (image_width is not used), so no tile
       straddles two sets.  0: one set for every ray (lap_sets ignored). */
    int lap_chunk_rays;
    int lap_sets;
    /* LAPLACE: rows of ws_rgb (and of the colour heads in the blobs) when it differs from n_lap; <= 0: n_lap.  The
       reference's forward_unc does not pass n_samples on to the colour head (laplace_field.py:516-520), which therefore
       always draws its default 100 whatever the density head was asked for. */
    int n_lap_rgb;
    /* ACTIVE / MCDROPOUT, ray-major layout: 1 = the outputs leave as ONE 16-byte row (sigma, r, g, b) per (pass, ray,
       sample): `rgb` is [B,R,S,4] and `density` is not written (may be NULL).  A kernel tile is 32 rays at one sample
       slot, so every store of the [B,R,S] + [B,R,S,3] layout is a lone 4-byte write into its own cache line; the packed
       row is one dwordx4 store, and unerf_composite_var / unerf_composite_moments read it back with one 16-byte load
       (pass density = NULL and the packed rows as rgb).  Same values either way. */
    int packed_out;
    /* tcnn_levels only: 1 = `table` points at the HALF copy of the main grid's parameter vector ([rows] half2) and the
       lookup runs in tiny-cuda-nn's own half arithmetic (unerf_hashgrid_fwd_tcnn_half) -- what
       HashEncoding(implementation="tcnn"), the reference's default (models/activenerfacto/activenerfacto_field.py:89,
       140-147; mcdropout_fields.py:78, 115-122; laplace_field.py:91, 129-136), hands to the MLP.  The f16 matrix kernels
       take the packed half features as their layer-0 operands without a conversion; 4 bytes per gathered corner
       instead of 8.  0: fp32 rows and blend (a tcnn built without TCNN_HALF_PRECISION). */
    int grid_half;
    /* Network widths, 0 = nerfacto's (hidden 64, hidden_color 64, geo_dim 15, feat_per_level 2, app_dim 32).  The reference
       forwards hidden_dim, hidden_dim_color, features_per_level and appearance_embed_dim from its model configs to the
       field (models/activenerfacto/activenerfacto_model.py:63-77, models/mcdropout/mcdropout_models.py:66-80,
       models/laplace/laplace_model.py:169-186); the field classes also take geo_feat_dim.  Any other combination (and
       L != 16) runs the ANY-WIDTH kernel: one lane per sample, every width a run-time loop -- correct, 10-20 x slower than
       the matrix kernels, plain ray-major outputs only (no packed_out / sample_major / feature planes), features_per_level
       4 on the torch-layout grid only (table rows of 4 floats).  Shapes then: w0t [L F][hidden], w1t [hidden][out1] with
       out1 = geo_dim + 2 (ACTIVE) / + 1 (MCDROPOUT) / + 0 (LAPLACE), h0t [16 + geo_dim][hidden_color], h1t
       [hidden_color][hidden_color], h2t [hidden_color][3], ws_density [..][hidden + 1], ws_rgb [..][3 hidden_color + 3],
       h0_full_t [16 + geo_dim + app_dim][hidden_color], app_embed [app_dim].  A dropout site has at most 128 units. */
    int hidden, hidden_color, geo_dim, feat_per_level, app_dim;
} unerf_field_params;
#define UNERF_DROP_TRUNK 1
#define UNERF_DROP_HEAD0 2
#define UNERF_DROP_HEAD1 4
#define UNERF_DROP_HEADIN 8
#define UNERF_MFMA_BLOB_FLOATS 10660
#define UNERF_MFMA16_BLOB_FLOATS 11684   /* mfma16_blob: + the 64 -> 3 colour layer as four f16 operand slabs (f16_single) */
#define UNERF_LAP_BLOB_FLOATS 33280

/* outputs: B = max(K,1) passes
 *   density [B,R,S]; rgb [B,R,S,3];
 *   aux     ACTIVE: beta [R,S] | LAPLACE: density_var [R,S] | else NULL
 *   aux2    LAPLACE: rgb_var [R,S] (relu, channel mean) | else NULL
 * sbins [R,S+1] spacing-domain bins of the final samples; ray_offset keys the dropout RNG.
 * near_plane < 0: sbins holds EUCLIDEAN bin edges instead (the starts / last end of a RaySamples made by the
 * caller's own sampler -- Field.forward(ray_samples)); far_plane is ignored then.  Not with `features`. */
int unerf_field_fwd(const float* origins, const float* directions, const float* sbins, int64_t R, int S,
                    float near_plane, float far_plane, int spacing, int64_t ray_offset,
                    const unerf_field_params* p /* host struct */,
                    const float* features /* NULL, or the planes written by unerf_field_gather */,
                    float* density, float* rgb, float* aux, float* aux2, void* stream);

/* MCDROPOUT under EXPLICIT keep masks (the exact-parity mode: replay masks recorded from the reference's nn.Dropout
 * modules, or the generator's own masks exported by unerf_mc_keep_bits).  Host struct. */
typedef struct {
    /* DEVICE bit arrays, one per Dropout site, indexed by log2 of the UNERF_DROP_* bit:
       [0] TRUNK, [1] HEAD0, [2] HEAD1, [3] HEADIN.  NULL = that site is not active.
       Each is [K][pass_stride][W] uint32, W = ceil(n_units / 32); bit (u & 31) of word (u >> 5) set = unit u KEPT.
       n_units: hidden (TRUNK), hidden_color (HEAD0, HEAD1).  Bits at and above n_units are ignored. */
    const uint32_t* site[4];
    int64_t pass_stride;     /* samples between pass k and pass k + 1 of every array */
    int64_t sample_offset;   /* sample index of (ray 0, sample 0) of this call: sample (r, s) reads row sample_offset + r*S + s */
} unerf_keep_masks;

/* unerf_field_fwd with the keep decision of every (pass, sample, unit) LOADED from `masks` instead of drawn by the counter
 * generator: pass k of sample (r, s) keeps unit u of a site iff its bit is set.  p->p_drop still gives the scale
 * 1/(1-p); p->seed is not read; ray_offset is only the image_width tile hint here.  Same kernels, same arithmetic: with
 * the masks unerf_mc_keep_bits writes for (seed, ray_offset * S) the outputs equal unerf_field_fwd's bit for bit.
 * Served by the matrix kernels (every precision, both grid layouts, every output layout) and the VALU kernel at
 * nerfacto's widths, sites TRUNK / HEAD0 / HEAD1 in any combination.  Refused before any launch: mode != MCDROPOUT,
 * K <= 0, an active site (drop_sites; 0 = TRUNK | HEAD1) without its array, an array for a site that is not active,
 * pass_stride < sample_offset + R*S, UNERF_DROP_HEADIN and the any-width kernel (both out of scope: there is no
 * fall-back to generator masks). */
int unerf_field_fwd_masked(const float* origins, const float* directions, const float* sbins, int64_t R, int S,
                           float near_plane, float far_plane, int spacing, int64_t ray_offset,
                           const unerf_field_params* p /* host struct */, const float* features,
                           float* density, float* rgb, float* aux, float* aux2,
                           const unerf_keep_masks* masks /* host struct */, void* stream);

/* keep [rows][n_units] uint8 (non-zero = kept: the bytes of a torch bool tensor) -> bits [rows][W] uint32 in the layout of
 * unerf_keep_masks (bits at and above n_units written 0).  n_units in [1, 4096]. */
int unerf_pack_keep_bits(const uint8_t* keep, int64_t rows, int n_units, uint32_t* bits, void* stream);

/* The masks the counter generator makes for samples [first_sample, first_sample + n_samples), passes 0..K-1, of mask stream
 * stream_id (TRUNK 0, HEAD1 1, HEAD0 2, HEADIN 3), as bits [K][pass_stride][W] in the layout of unerf_keep_masks
 * (pass_stride >= n_samples; row i = sample first_sample + i).  n_units <= 128.  Made by the functions the field kernels
 * use (csrc/unerf_common.hpp); unerf_field_fwd numbers its samples from ray_offset * S. */
int unerf_mc_keep_bits(uint32_t seed, int K, int64_t first_sample, int64_t n_samples, int stream_id, int n_units,
                       float p_drop, uint32_t* bits, int64_t pass_stride, void* stream);

/* Level-major form of the same HashEncoding lookup for the main field: writes the features of the
 * R*S final samples as planes [L][R*S][2] (level, sample, feature).  Each level table is 4 MiB --
 * one XCD's L2 -- so sweeping level by level runs the gathers out of L2 instead of the Infinity
 * Cache; unerf_field_fwd(features=...) then skips its own lookup.  Same values bit for bit. */
int unerf_field_gather(const float* origins, const float* directions, const float* sbins, int64_t R, int S,
                       float near_plane, float far_plane, int spacing, const float* table, const float* scalings, int L,
                       int log2T, float* feature_planes, void* stream);

/* Laplace depth path: models/laplace/laplace_model.py:486-507.  mean over D draws of
 * get_weights(relu(mu + max(sqrt(var),1e-10) * eps)).  noise [D,R,S] or NULL (then the
 * built-in counter RNG with `seed`).  weights_out [R,S]. */
int unerf_laplace_depth_weights(const float* density_mu, const float* density_var, const float* sbins,
                                int64_t R, int S, float near_plane, float far_plane, int spacing, const float* noise, int D,
                                uint32_t seed, int64_t ray_offset, float* weights_out, void* stream);

/* Laplace GGN fitting: NerfactoLaplaceModel.compute_hessian_naive (models/laplace/laplace_model.py:343-400),
 * one batch of rays.  Adds (+=) the batch's diagonal generalised Gauss-Newton of the summed-MSE loss w.r.t.
 * mlp_density (ggn_density[65]: weight[64], bias) and mlp_rgb_ll (ggn_rgb[195]: weight[3][64] row-major,
 * bias[3]) -- the layout of field.mlp_density_ggn / field.mlp_rgb_ggn (laplace_field.py:231-238).
 * Forward = the deterministic is_inference=False path (laplace_field.py:317-345, 462-465) rendered with the
 * eval-mode RGB renderer.  p: mode LAPLACE with mfma_blob; p->ws_density[65] / p->ws_rgb[195] hold the MEAN
 * last layers ([out,in] row-major, then bias); n_lap / lap_blob are ignored.  sbins [R,S+1] as for
 * unerf_field_fwd, S <= 64.  workspace: unerf_laplace_ggn_workspace_bytes(R, S) bytes of device scratch. */
size_t unerf_laplace_ggn_workspace_bytes(int64_t R, int S);
int unerf_laplace_ggn_diag(const float* origins, const float* directions, const float* sbins, int64_t R, int S,
                           float near_plane, float far_plane, int spacing, const unerf_field_params* p /* host struct */,
                           int background, const float* background_rgb_host /* UNERF_BG_*: the renderer the loss sees */,
                           void* workspace, size_t workspace_bytes, float* ggn_density, float* ggn_rgb,
                           void* stream);

/* Per-ray camera-pose gradient: nerfuncertainty/scripts/estimate_gradient_pose_6dof.py:58-216 (one
 * torch.autograd.grad(pred_rgb.mean(-1), c2w) per pixel of a frame) in one launch, without an autograd tape.
 * s = channel mean of the eval-mode rgb of a ray (nan_to_num as in the forward; the clamp to [0, 1] passes the gradient
 * where 0 <= pred <= 1; background as unerf_laplace_ggn_diag: for UNERF_BG_LAST_SAMPLE the transmittance left behind the
 * last sample flows into that sample's colour).  The sample bins are held FIXED (upstream's PDFSampler detaches them): the
 * pose reaches s through the sample positions o + d t_i and the SH encoding of d only.
 *   rot_inv_host NULL : out_grad [R,6]  = (ds/do, ds/dd), d taken as a free vector
 *   rot_inv_host [9]  : the inverse of c2w[:3,:3], row-major (host); out_grad [R,12] = ds/dc2w, row-major 3x4:
 *                       ds/dc2w[:,3] = ds/do and ds/dc2w[a][b] = P[a] (R^-1 d)[b] with P = (I - d d^T) ds/dd -- autograd
 *                       through d = normalize(R dir_cam) for any invertible R and any camera whose origin is c2w[:,3]
 *   out_rgb           : NULL, or [R,3] <- the colour the kernel composited
 * p: mode ACTIVE (trunk output 17) or MCDROPOUT (16; evaluated without dropout -- plain nerfacto), nerfacto's widths,
 * torch-layout or tcnn-layout grid (grid_half: the half2 rows are widened on read); everything is computed in fp32,
 * the blobs are not read.  sbins [R,S+1] spacing-domain bins, S <= 64.  Anything else (LAPLACE, other widths,
 * near_plane < 0) is UNERF_ERR_ARG before any launch.  Two calls with the same inputs return the same bits. */
int unerf_pose_grad(const float* origins, const float* directions, const float* sbins, int64_t R, int S,
                    float near_plane, float far_plane, int spacing, const unerf_field_params* p /* host struct */,
                    int background, const float* background_rgb_host, const float* rot_inv_host,
                    float* out_grad, float* out_rgb, void* stream);

/* Per-ray pose JACOBIAN of the rendered channels: what the reference's user gets by changing outputs= of the
 * torch.autograd.grad call in estimate_gradient_pose_6dof.py:183-190, one row per selected channel behind one forward pass.
 *   UNERF_POSE_CH_R / _G / _B : d clamp(pred_c) / d. under exactly unerf_pose_grad's rules (nan_to_num, the clamp gate per
 *                               channel -- a clamped channel's row is exactly 0 --, the background rule with the last-sample
 *                               term, bins held fixed); out_val = the clamped colour, unerf_pose_grad's out_rgb bit for bit
 *   UNERF_POSE_CH_ACC         : A = sum_i w_i (RaySamples.get_weights + AccumulationRenderer); out_val = A
 *   UNERF_POSE_CH_EDEPTH      : e = sum_i w_i t_i / (A + 1e-10), t_i = the bin mid-point (DepthRenderer "expected"); out_val = e.
 *                               The renderer's clip of e to the step range of the ray is NOT applied and NOT differentiated:
 *                               it is the identity except where A is of the order of 1e-10.
 * channels: a non-empty subset of the five bits, C = popcount; the rows stand in bit order (R, G, B, ACC, EDEPTH).
 *   rot_inv_host NULL : D = 6, a row is (d./do, d./dd);  [9]: D = 12, a row is d./dc2w row-major 3x4 (unerf_pose_grad's epilogue)
 *   proj_host         : NULL, or [D][P] row-major host floats, 1 <= P <= 12 (e.g. tangent basis x Cholesky factor of a pose
 *                       covariance): out_proj [R,C,P] = row . proj summed over D in order, out_var [R,C] = sum_k out_proj_k^2
 *                       summed over P in order -- the first-order variance of the channel under that covariance
 *   out_jac [R,C,D], out_proj [R,C,P], out_var [R,C], out_val [R,C]: each may be NULL, not all four.
 * p, sbins, background as unerf_pose_grad; fp32 throughout, ONE launch, no atomics, no global scratch.  Two calls return the
 * same bits; a ray's bits do not depend on the other rays of its launch; a row's bits depend neither on the other channels
 * selected nor on which outputs were requested.  R == 0 is UNERF_OK.  UNERF_ERR_ARG before any launch, each with its own
 * message: everything unerf_pose_grad refuses; channels empty or with unknown bits; proj_host with P outside [1, 12];
 * out_proj or out_var without proj_host; all four outputs NULL. */
#define UNERF_POSE_CH_R 1
#define UNERF_POSE_CH_G 2
#define UNERF_POSE_CH_B 4
#define UNERF_POSE_CH_ACC 8
#define UNERF_POSE_CH_EDEPTH 16
int unerf_pose_jacobian(const float* origins, const float* directions, const float* sbins, int64_t R, int S,
                        float near_plane, float far_plane, int spacing, const unerf_field_params* p /* host struct */,
                        int background, const float* background_rgb_host, const float* rot_inv_host,
                        int channels, const float* proj_host, int P,
                        float* out_jac, float* out_proj, float* out_var, float* out_val, void* stream);

/* The same gradient of an MC-DROPOUT frame under a NAMED mask draw: rgb = (1/K) sum_k clamp(pred_k), pass k evaluated with
 * the keep masks of that pass, and out_grad = (1/K) sum_k of unerf_pose_grad's quantity of pass k (each pass with its own
 * clamp gate, nan_to_num, background rule and last-sample term).  One launch whatever K is: the grid lookup and trunk
 * layer 0 lie in front of every Dropout site and are evaluated once, the adjoints of all passes are summed in front of them.
 *   p     : mode MCDROPOUT, K = p->K >= 1, nerfacto's widths, either grid layout (grid_half widened on read); fp32, the
 *           blobs are not read.  Active sites: p->drop_sites (0 = TRUNK | HEAD1), any combination of TRUNK, HEAD0, HEAD1.
 *   masks : NULL = the counter generator (csrc/unerf_common.hpp) for sample index (ray_offset + r) S + s, seed p->seed and
 *           the site's stream id -- the masks unerf_field_fwd draws for these rays; else the bit arrays of
 *           unerf_field_fwd_masked (row sample_offset + r S + s, pass_stride), and ray_offset / p->seed are not read.
 *           A kept unit is multiplied by 1/(1 - p_drop); a dropped one is exactly 0, and so is its adjoint.
 *   out_grad [R,6] / [R,12] as unerf_pose_grad (same rot_inv_host epilogue); out_rgb NULL or [R,3] = the mean colour.
 * With K = 1, p_drop = 0 and all-ones explicit masks both outputs equal unerf_pose_grad's bit for bit.  Two calls with the
 * same inputs return the same bits.  UNERF_ERR_ARG before any launch: another mode, K < 1, UNERF_DROP_HEADIN, other
 * widths, near_plane < 0, S outside [1, 64]; with masks: an active site without its array, an array for an inactive
 * site, pass_stride < sample_offset + R S. */
int unerf_pose_grad_mc(const float* origins, const float* directions, const float* sbins, int64_t R, int S,
                       float near_plane, float far_plane, int spacing, int64_t ray_offset,
                       const unerf_field_params* p /* host struct */,
                       const unerf_keep_masks* masks /* host struct; NULL = the counter generator */,
                       int background, const float* background_rgb_host, const float* rot_inv_host,
                       float* out_grad, float* out_rgb, void* stream);

/* The same gradient of a LAPLACE frame under a NAMED draw of the last layers (laplace_field.py:279-362, 365-485, 528-568;
 * laplace_model.py:456-480): per sample hb = W0 feat + b0 and geo = W1 hb + b1 (no ReLU), the density
 * mu_d = (1/n_lap) sum_q act(w_q . hb + b_q) over the rows p->ws_density [set][q][65] (act = exp, softplus with lap_softplus;
 * NOT multiplied by the selector unless lap_mask_density is set), the colour mu_c = (1/n_rgb) sum_q sigmoid(Wc_q h + bc_q) over
 * p->ws_rgb [set][q][195] behind the two ReLU layers of the colour head (n_rgb = n_lap_rgb, or n_lap when that is <= 0),
 * composited with get_weights(mu_d) under the background, nan_to_num and clamp rules of unerf_pose_grad.  The rows are
 * ordinary tensors (field.sample_last_layers(generator=) reproduces them), so the frame is a deterministic function of the
 * pose.  The set of ray r is (ray_offset + r) / lap_chunk_rays when lap_chunk_rays > 0, else set 0.
 *   p : mode LAPLACE, out1 == 15, nerfacto's widths, L == 16, either grid layout (grid_half widened on read), use_aabb,
 *       sh_remap; fp32 rows ws_density / ws_rgb with n_lap >= 1, n_lap_rgb >= 0, lap_sets, lap_chunk_rays >= 0 (ANY values:
 *       the multiple-of-32 rule of unerf_field_fwd belongs to its 32-ray tiles; here a wave is one ray), lap_softplus,
 *       lap_mask_density.  No blob is read.
 *   out_grad [R,6] / [R,12] as unerf_pose_grad (same rot_inv_host epilogue); out_rgb NULL or [R,3] = the composited mean colour.
 * fp32 throughout, ONE launch whatever n_lap is, no global scratch, no atomics, the heads summed in row order q = 0 .. n-1:
 * two calls return the same bits, and a ray's bits do not depend on the other rays of its launch.  R == 0 is UNERF_OK.
 * UNERF_ERR_ARG before any launch, each with its own message: another mode; other widths or L != 16; near_plane < 0; S
 * outside [1, 64]; null ws_*, field or output pointers; n_lap < 1; lap_chunk_rays < 0; lap_chunk_rays > 0 and
 * (ray_offset + R - 1) / lap_chunk_rays >= lap_sets; ray_offset < 0.  unerf_pose_grad keeps refusing LAPLACE. */
int unerf_pose_grad_laplace(const float* origins, const float* directions, const float* sbins, int64_t R, int S,
                            float near_plane, float far_plane, int spacing, int64_t ray_offset,
                            const unerf_field_params* p /* host struct */,
                            int background, const float* background_rgb_host, const float* rot_inv_host,
                            float* out_grad, float* out_rgb, void* stream);

/* ------------------------------------------------- composite + variance --
 * Replaces RaySamples.get_weights + RGB/Accumulation/Depth(median,expected)/Uncertainty
 * renderers + the depth-variance sum at models/activenerfacto/activenerfacto_model.py:94-112
 * and models/laplace/laplace_model.py:471-521.
 * density [B,R,S], rgb [B,R,S,3], beta [B? no: R,S] (NULL -> rgb_var = 0);
 * weights_alt [R,S] (NULL or the laplace mean sampled weights: then accumulation, depth,
 * expected depth and depth_var use it while rgb and rgb_var use get_weights(density)).
 * clip_minmax as produced by unerf_weights_pdf_resample.  1 <= S <= 256, any value.
 * background / background_rgb_host: UNERF_BG_* (above).
 * nonfinite_flag (DEVICE int32, may be NULL): |= 1 (atomically, once per offending wave) when a density or colour
 * read by this call is NaN.  The renderers turn NaN into 0 (nan_to_num, as upstream does), which would hide the one
 * failure mode of the f16 matrix kernels -- an operand at or beyond 65504 (hi = inf, lo = -inf -> NaN); the host
 * checks the word once per frame and re-renders the launch group with the exact-fp32 kernels (render.OverflowGuard).
 * out [B,R,8] = rgb(3), accumulation, depth(median), expected_depth, rgb_var, depth_var(+1e-5). */
int unerf_composite_var(const float* density, const float* rgb, const float* beta, const float* weights_alt,
                        const float* sbins, int B, int64_t R, int S, float near_plane, float far_plane, int spacing,
                        const float* clip_minmax, int64_t ray_offset, int64_t chunk_rays, int background,
                        const float* background_rgb_host, int32_t* nonfinite_flag, float* out, void* stream);

/* Fused K-pass form of the two calls above/below for MC-dropout: composites the B <= 16 passes of every
 * ray and reduces them in registers.  mean_out / var_out [R,8] over the passes of
 * rgb(3), accumulation, depth, expected_depth, rgb_var, depth_var (var unbiased, B-1). */
int unerf_composite_moments(const float* density, const float* rgb, const float* sbins, int B, int64_t R, int S,
                            float near_plane, float far_plane, int spacing, const float* clip_minmax, int64_t ray_offset,
                            int64_t chunk_rays, int background, const float* background_rgb_host, int32_t* nonfinite_flag,
                            float* mean_out, float* var_out, void* stream);

/* The same two reductions over the sample-major planes unerf_field_fwd writes with sample_major = 1
 * (density [B,S,R], rgb [B,S,3,R], beta [S,R] or NULL): one lane per ray walks the samples front to back, so
 * get_weights is the sequential recurrence of activenerfacto_model.py:94 / RaySamples.get_weights, and the K passes
 * of mcdropout_models.py:116-126 are reduced to mean / unbiased variance in the same thread.
 * out [B,R,8]; mean_out / var_out [R,8] (B >= 2); channel order as unerf_composite_var. */
int unerf_composite_var_planes(const float* density, const float* rgb, const float* beta, const float* sbins, int B,
                               int64_t R, int S, float near_plane, float far_plane, int spacing, const float* clip_minmax,
                               int64_t ray_offset, int64_t chunk_rays, int background, const float* background_rgb_host,
                               int32_t* nonfinite_flag, float* out, void* stream);
int unerf_composite_moments_planes(const float* density, const float* rgb, const float* sbins, int B, int64_t R, int S,
                                   float near_plane, float far_plane, int spacing, const float* clip_minmax,
                                   int64_t ray_offset, int64_t chunk_rays, int background,
                                   const float* background_rgb_host, int32_t* nonfinite_flag, float* mean_out,
                                   float* var_out, void* stream);

/* ------------------------------------------- several whole views per launch --
 * A frame of a few ten thousand rays leaves most of a launch group (2^20 rays) empty; the *_views entry points take the
 * rays of B cameras of ONE image size H x W as one launch: a tall row-major image of B H rows, launch row j = view
 * j / (H W) at frame-local ray j mod (H W).  Everything a kernel numbers by "the ray's index inside its frame" -- the
 * per-chunk clip bounds of the expected depth, the MC-dropout mask counter, the camera of the ray generator -- takes the
 * frame-local index and the view's own values, so that view v of the launch is bit-identical to a launch of its own with
 * ray_offset = 0 (and p->seed = seed[v]).  The image_width tile hints are locality hints that change no bit and keep
 * working on the tall image with the launch-global row.  Each call refuses, before any launch: n_views outside
 * [1, UNERF_NERF_MAX_VIEWS], rays_per_view <= 0, R != n_views * rays_per_view. */
#define UNERF_NERF_MAX_VIEWS 16
typedef struct {            /* host struct */
    int32_t n_views;        /* views in this launch */
    int64_t rays_per_view;  /* H W */
    uint32_t seed[UNERF_NERF_MAX_VIEWS];   /* MC-dropout mask seed of each view (unerf_field_fwd_views; else ignored) */
} unerf_ray_views;
typedef struct {            /* host struct: one camera of unerf_generate_rays_views */
    float c2w[12];          /* [3,4] row-major */
    float fx, fy, cx, cy;
    float distortion[6];    /* k1, k2, k3, k4, p1, p2; all 0 = no lens */
} unerf_ray_camera;

/* unerf_generate_rays for n_views whole frames of H x W pixels and one camera type: origins / directions
 * [n_views H W, 3], pixel_area [n_views H W] or NULL; view v's rows are those of unerf_generate_rays(cameras[v], ...,
 * ray_start = 0, count = H W), bit for bit. */
int unerf_generate_rays_views(const unerf_ray_camera* cameras_host, int n_views, int camera_type, int H, int W,
                              float* origins, float* directions, float* pixel_area, void* stream);

/* unerf_weights_pdf_resample with the clip rows numbered per view: clip_minmax addresses the first view's rows,
 * chunk c of view v is row v * ceil(rays_per_view / chunk_rays) + c (the reference chunks every camera on its own). */
int unerf_weights_pdf_resample_views(const float* density, const float* sbins, int64_t sbins_stride, int64_t R, int n,
                                     float near_plane, float far_plane, int spacing, const float* u, int m,
                                     float histogram_padding, float eps, float* sbins_out, float* prop_depth_out,
                                     float* weights_out, float* clip_minmax, const unerf_ray_views* views /* host struct */,
                                     int64_t chunk_rays, void* stream);

/* unerf_composite_var / unerf_composite_moments reading the clip rows of unerf_weights_pdf_resample_views */
int unerf_composite_var_views(const float* density, const float* rgb, const float* beta, const float* weights_alt,
                              const float* sbins, int B, int64_t R, int S, float near_plane, float far_plane, int spacing,
                              const float* clip_minmax, const unerf_ray_views* views /* host struct */, int64_t chunk_rays,
                              int background, const float* background_rgb_host, int32_t* nonfinite_flag, float* out,
                              void* stream);
int unerf_composite_moments_views(const float* density, const float* rgb, const float* sbins, int B, int64_t R, int S,
                                  float near_plane, float far_plane, int spacing, const float* clip_minmax,
                                  const unerf_ray_views* views /* host struct */, int64_t chunk_rays, int background,
                                  const float* background_rgb_host, int32_t* nonfinite_flag, float* mean_out,
                                  float* var_out, void* stream);

/* unerf_field_fwd over several views: sample (r, s) of view v draws the masks of counter r_local * S + s under seed[v]
 * (p->seed is not read), i.e. what unerf_field_fwd(ray_offset = 0, p->seed = seed[v]) draws for that view alone.
 * Built for the frame kernels: ACTIVE and MCDROPOUT on the split-f16 / single-f16 matrix kernels (mfma16_blob; "f16x2" and
 * "f16"), nerfacto's widths, the default Dropout sites, ray-major outputs (packed_out or not).  ACTIVE, and MCDROPOUT
 * with K = 0 or p_drop = 0, have no per-view value and run the kernels of unerf_field_fwd.  Refused before any launch,
 * with a message that says so: LAPLACE (its views form is unerf_field_fwd_laplace_views, below), no mfma16_blob (the exact-fp32 and VALU kernels), the any-width kernel,
 * sample_major planes, pre-gathered features, other drop_sites than TRUNK | HEAD1, and explicit keep masks (`masks`
 * is there to be refused by name: unerf_field_fwd_masked takes one frame, and nothing falls back to another kernel). */
int unerf_field_fwd_views(const float* origins, const float* directions, const float* sbins, int64_t R, int S,
                          float near_plane, float far_plane, int spacing, const unerf_ray_views* views /* host struct */,
                          const unerf_field_params* p /* host struct */, const float* features /* must be NULL */,
                          float* density, float* rgb, float* aux, float* aux2,
                          const unerf_keep_masks* masks /* must be NULL */, void* stream);

/* LAPLACE over several views.  The Laplace kernels number two more things by the ray's index inside its frame: the sample
 * set of a ray (p->lap_chunk_rays rays per set) and the stream of its depth draws.  Next to unerf_ray_views (n_views,
 * rays_per_view) the two entry points below take the per-view values of both: */
typedef struct {            /* host struct */
    int32_t set_base[UNERF_NERF_MAX_VIEWS];     /* first sample set of view v in the stacks of unerf_field_params */
    uint32_t depth_seed[UNERF_NERF_MAX_VIEWS];  /* seed of view v's depth draws (unerf_laplace_depth_weights_views) */
} unerf_laplace_views;

/* unerf_field_fwd (LAPLACE, f16 matrix kernel) for several views: view v is rendered with the sets set_base[v] +
 * local_ray / lap_chunk_rays (set_base[v] alone when lap_chunk_rays == 0: one set per view) of the stacks lap16_blob /
 * ws_* [lap_sets, ...], i.e. what unerf_field_fwd(ray_offset = 0) computes for that view's rays with the stacks narrowed
 * to its own sets, bit for bit.  The kernel lays its blocks of 32 rays out per view (ceil(rays_per_view / 32) blocks each),
 * so a tile never straddles two views or two sets whatever rays_per_view is.  Outputs as unerf_field_fwd: dense, ray-major,
 * row = launch row; aux = density variance, aux2 = colour variance; p->overflow_flag as there.
 * Refused before any launch, with a message that says why: a bad view table, lap_views == NULL, a mode other than LAPLACE,
 * no mfma16_blob or lap16_blob (the exact-fp32 and VALU kernels render one frame per call), the any-width kernel,
 * sample_major, lap_chunk_rays < 0 or not a multiple of 32, set_base[v] < 0, set_base[v] + ceil(rays_per_view /
 * lap_chunk_rays) > lap_sets (lap_chunk_rays == 0: set_base[v] >= max(lap_sets, 1)), rays_per_view * S >= 2^32.  There is no
 * `features` argument: pre-gathered features have no LAPLACE form. */
int unerf_field_fwd_laplace_views(const float* origins, const float* directions, const float* sbins, int64_t R, int S,
                                  float near_plane, float far_plane, int spacing, const unerf_ray_views* views /* host struct */,
                                  const unerf_laplace_views* lap_views /* host struct */,
                                  const unerf_field_params* p /* host struct */, float* density, float* rgb, float* aux,
                                  float* aux2, void* stream);

/* unerf_laplace_depth_weights for several views: the draws of launch row r (view r / rays_per_view, frame-local ray r mod
 * rays_per_view) are those of unerf_laplace_depth_weights(seed = depth_seed[view], ray_offset = 0) on that view's rows.
 * noise != NULL: [D,R,S] explicit draws indexed by launch row -- no per-view value, the single call on the tall ray list.
 * Same S range (1 to 256, ragged S included) as the single call. */
int unerf_laplace_depth_weights_views(const float* density_mu, const float* density_var, const float* sbins, int64_t R, int S,
                                      float near_plane, float far_plane, int spacing, const float* noise, int D,
                                      const unerf_ray_views* views /* host struct */,
                                      const unerf_laplace_views* lap_views /* host struct */, float* weights_out, void* stream);

/* ------------------------------------------------------ moments over K --
 * Replaces torch.stack(...).mean(0) / .std(0) / .var(0) over MC passes
 * (models/mcdropout/mcdropout_models.py:121-126) and over ensemble members
 * (models/ensemble/ensemble_pipeline.py:159-189).  x [K,N,C] -> mean [N,C],
 * var [N,C] (unbiased, K-1; NULL ok).  Two-pass in fp32 like torch. */
int unerf_moments(const float* x, int K, int64_t N, int C, float* mean, float* var, void* stream);

/* ------------------------------------- fused ensemble reduce over B views --
 * The stack -> unerf_moments -> key loop chain of models/ensemble/ensemble_pipeline.py:159-189 for B views x every member
 * key x M members in ONE launch, whatever B, M and the key count are; no host-device synchronisation.
 *
 * Sources are read in place through `table`, a DEVICE array [B][n_keys][M] of pointers: entry (v, k, j) is member j's
 * tensor of input key k in view v, element p channel c at ptr[p * keys[k].stride + c] (no stacked copy; a channel slice
 * of wider rows, such as columns 4..6 of the composite's [R,8] rows, is stride 8 with the pointer moved to column 4).
 * keys[k] (host) describes input key k: `channels` C, `n` elements (the pixels of an image key, 1 for a non-image key
 * such as a splat member's background [3]) and the element stride in floats (>= C).
 *
 * Per (view, key, element, channel) the mean and unbiased variance over the members are unerf_moments's, bit for bit
 * (the same device function: s += x_j in member order, m = s / M, q += (x_j - m)^2, q / (M - 1); M = 1: NaN variance).
 * plan[o] (host) asks for one output block [keys[key].n, C_out], written contiguously at
 * arena[v * view_stride + plan[o].offset] for every view v:
 *   UNERF_ENS_MEAN          C_out = C   mean
 *   UNERF_ENS_VAR           C_out = C   variance
 *   UNERF_ENS_VAR_CMEAN     C_out = 1   epi  = ((var_0 + var_1) + ...) / C            (channel order, IEEE divide)
 *   UNERF_ENS_ALEA_CMEAN    C_out = 1   alea = ((a_0 + a_1) + ...) / C_aux,  a = the member mean of key `aux`
 *   UNERF_ENS_EPI_ALEA      C_out = 1   epi + alea
 *   UNERF_ENS_EPI_ALEA_SQRT C_out = 1   sqrtf(epi + alea)                              (IEEE square root)
 *   UNERF_ENS_STD_CMEAN     C_out = 1   ((sqrtf(var_0) + sqrtf(var_1)) + ...) / C
 * `aux` is read by the three alea statistics only (keys[aux].n must equal keys[key].n), else ignored.  A (key, statistic)
 * pair may appear once.  Blocks must lie inside [0, view_stride) without overlapping, B * view_stride <= arena_floats.
 *
 * UNERF_ERR_ARG before any launch or device call: B > UNERF_NERF_MAX_VIEWS, n_keys outside [1, UNERF_ENS_MAX_KEYS],
 * M outside [1, UNERF_ENS_MAX_MEMBERS], channels outside [1, UNERF_ENS_MAX_CHANNELS], stride < channels, negative n, a
 * bad plan entry, a null table / arena while there is something to reduce.  B = 0, n_out = 0 or every n = 0: success,
 * nothing launched. */
#define UNERF_ENS_MAX_KEYS 32
#define UNERF_ENS_MAX_MEMBERS 64
#define UNERF_ENS_MAX_CHANNELS 64
#define UNERF_ENS_MEAN 0
#define UNERF_ENS_VAR 1
#define UNERF_ENS_VAR_CMEAN 2
#define UNERF_ENS_ALEA_CMEAN 3
#define UNERF_ENS_EPI_ALEA 4
#define UNERF_ENS_EPI_ALEA_SQRT 5
#define UNERF_ENS_STD_CMEAN 6
#define UNERF_ENS_STATS 7
typedef struct {            /* host struct: one input key */
    int32_t channels;       /* C */
    int32_t stride;         /* floats between consecutive elements of one source (>= C) */
    int64_t n;              /* elements: pixels of an image key, 1 for a non-image key */
} unerf_ens_key;
typedef struct {            /* host struct: one output block per view */
    int32_t stat;           /* UNERF_ENS_* */
    int32_t key;            /* input key whose moments it is made of */
    int32_t aux;            /* input key whose member mean is the aleatoric term (alea statistics only) */
    int32_t reserved;       /* 0 */
    int64_t offset;         /* floats from the start of the view's part of the arena */
} unerf_ens_out;
int unerf_ensemble_reduce(const float* const* table /* device */, int B, int n_keys, int M, const unerf_ens_key* keys /* host */,
                          const unerf_ens_out* plan /* host */, int n_out, int64_t view_stride, float* arena,
                          int64_t arena_floats, void* stream);

/* ------------------------------------------------- per-image eval metrics --
 * Replaces the torch / numpy chain behind one image's entry of metrics.json: get_image_metrics_and_images_unc and
 * get_unc_metrics_depth (scripts/eval_uncertainty.py:306-412, 647-813: error definitions, psnr, mse / rmse, Gaussian
 * NLL, average variance), metrics/ause.py (three sparsification curves) and metrics/auce.py (99 coverages), plus the
 * SSIM the reference reaches through model.ssim.  One call leaves ONE row of float64 partial results in device memory;
 * the host copies it once and finishes every metric (uncertainty-nerf-gs_amd/metrics.py: finish_metrics).
 *
 * pred / target [n, C] (1 <= C <= 4, n C < 2^31), sigma [n] (std per pixel, shared by the channels), mask [n] or NULL
 * (0 = the pixel is left out of everything).  p = pred as given: the reference computes every uncertainty metric from the
 * render itself (scripts/eval_uncertainty.py:316).  pc = min(pred, pred_clip_max) (+inf: no clip; rgb: 1.0) is the copy
 * that psnr and SSIM alone see (:681-685): slots [6], [8], [9] and [12].  Per valid pixel, in float32 as the host
 * computes them: sq = sum_c (p - t)^2, ab = sum_c |p - t| (channels added left to right), var = sigma^2; every sum
 * below is float64, reduced in a fixed order (two calls on the same inputs give equal rows).
 * ratios_host [n_ratios] / z_host [n_z]: HOST float64 arrays, 1..128 entries each, read during the call.
 *
 * out [UNERF_METRICS_ROW] doubles:
 *   [0] n_valid   [1] valid pixels with a non-finite pred / target / sigma (the sums then mean nothing; the host raises)
 *   [2] sum sq    [3] sum ab    [4] sum var    [5] sum sigma
 *   [6] sum over pixel-channels of ((double)t - (double)pc)^2                        (psnr)
 *   [7] sum over pixel-channels of (t - p)^2 / (2 s^2) + log s + log(2 pi) / 2, s = max(sigma, nll_min_sigma), all in
 *       float64                                                                      (UNERF_METRICS_NLL)
 *   [8] min pc  [9] max pc  [10] min target  [11] max target   (+-inf when nothing is valid)
 *   [12] sum of the SSIM index over the (H-10) x (W-10) interior pixels and the C channels, [13] their number
 *       (UNERF_METRICS_SSIM: 11x11 gaussian window, sigma 1.5, k1 0.01, k2 0.03, data_range = max([9] - [8], [11] - [10])
 *       with the differences taken in float32; window sums in float64; needs mask == NULL, H W == n, min(H, W) >= 11)
 *   [UNERF_METRICS_AUCE_OFF + k], k < n_z: number of valid pixel-channels with |t - p| / sigma <= z[k], the ratio in
 *       float64; sigma <= 0 gives 0 for a zero residual and +inf otherwise (metrics/auce.py as one comparison per
 *       element)                                                                     (UNERF_METRICS_AUCE)
 *   [UNERF_METRICS_AUSE_OFF + 128 f + k], k < n_ratios, with keep_k = (int64)((1.0 - ratios[k]) * (double)n_valid)
 *       clamped to [0, n_valid]: f = 0 the sum of the keep_k smallest sq; f = 1 of the keep_k smallest ab; f = 2 / 3 the
 *       sum of sq / of ab over the keep_k pixels of smallest var.  "Smallest" = ascending value, ties by ascending pixel
 *       index (a stable LSD radix sort of the bit patterns)                          (UNERF_METRICS_AUSE)
 * Entries whose flag is not set, and every unused slot, are 0.
 * workspace: unerf_image_metrics_workspace_bytes(n) bytes of device scratch, 8-byte aligned (about 28 n bytes).
 * n = 0 is a successful no-op that leaves `out` alone. */
#define UNERF_METRICS_AUSE 1
#define UNERF_METRICS_AUCE 2
#define UNERF_METRICS_NLL 4
#define UNERF_METRICS_SSIM 8
#define UNERF_METRICS_AUCE_OFF 16
#define UNERF_METRICS_AUSE_OFF 144
#define UNERF_METRICS_ROW 656
size_t unerf_image_metrics_workspace_bytes(int64_t n);
int unerf_image_metrics(const float* pred, const float* target, const float* sigma, const uint8_t* mask, int64_t n, int C,
                        int H, int W, float pred_clip_max, float nll_min_sigma, const double* ratios_host, int n_ratios,
                        const double* z_host, int n_z, int flags, void* workspace, size_t workspace_bytes, double* out,
                        void* stream);

/* The same for a batch of B images of ONE size in one call: the metric stage behind a view batch of the eval loop
 * (scripts/eval_uncertainty.py:306-412, 647-813 once per image there; eval.py: get_average_uncertainty_metrics with
 * view_batch > 1).  pred / target [B, n, C], sigma [B, n], mask [B, n] or NULL: contiguous stacks, image b at b n C
 * (b n) elements; n, C, H, W, the clip, the tables and the flags are shared by the images, 1 <= B <=
 * UNERF_METRICS_MAX_IMAGES, n C < 2^31 per image (the offsets that carry the image index are 64-bit).
 * out [B, UNERF_METRICS_ROW]: row b is the row unerf_image_metrics writes for image b alone, EQUAL BIT FOR BIT in all
 * 656 slots (the zero slots of unset flags and the +-inf minima of an image with nothing valid included) -- the image is
 * an outer grid coordinate of every kernel, each image keeps the workgroup decomposition and the fixed reduction order
 * it has alone, and has its own region of the workspace.  The number of memsets and kernel launches does not depend on B.
 * workspace: unerf_image_metrics_batch_workspace_bytes(n, B) bytes, 8-byte aligned (B times the single-image size).
 * n = 0 is a successful no-op that leaves `out` alone. */
#define UNERF_METRICS_MAX_IMAGES 64
size_t unerf_image_metrics_batch_workspace_bytes(int64_t n, int B);
int unerf_image_metrics_batch(const float* pred, const float* target, const float* sigma, const uint8_t* mask, int64_t n, int B,
                              int C, int H, int W, float pred_clip_max, float nll_min_sigma, const double* ratios_host,
                              int n_ratios, const double* z_host, int n_z, int flags, void* workspace, size_t workspace_bytes,
                              double* out, void* stream);

/* The rendered images of the eval stage: what save_imgs_rgb (scripts/eval_uncertainty.py:209-303) hands to
 * media.write_image per eval image, as final 8-bit planes for a batch of B images of ONE size (eval.py: save_imgs_rgb,
 * host definition eval.pack_eval_images).  pred / target [B, n, 3], sigma [B, n]: contiguous float32 stacks; 1 <= B <=
 * UNERF_METRICS_MAX_IMAGES, 3 n < 2^31 per image (the offsets that carry the image index are 64-bit).
 * With q(x) = (uint8)(clip(x, 0, 1) * 255 + 0.5) in float64, truncating, NaN -> 0:
 *   gt8   [B, n, 3] = q(target)          pred8 [B, n, 3] = q(pred), not clipped first
 *   err8  [B, n]    = q(|d0| + |d1| + |d2|), d = pred - target in float32, channels added left to right
 *   std8  [B, n, 3] = lut[min((int)(a * 256), 255)], a = ((double)s - vmin) / ((vmax - vmin) + DBL_EPSILON) in float64,
 *                     s = clip((sigma - unc_lo) / unc_span, 0, 1) in float32 (a NaN stays one), vmin / vmax the minimum /
 *                     maximum of s over the image's own non-NaN pixels; a NaN pixel is (0, 0, 0)
 * lut: DEVICE [256, 3] bytes (colormaps.JET_U8).  unc_lo = min(unc_min, unc_max), unc_span = |unc_max - unc_min| > 0.
 * Any plane may be NULL and is then skipped; the others do not change.  Two kernels (the per-image range of s, run only
 * when std8 is wanted; the pack) and two memsets of the workspace, whatever B is: the image is an outer grid coordinate.
 * The range is an integer min / max of bit patterns (s >= 0): two calls on the same inputs give equal bytes.
 * workspace: unerf_eval_images_workspace_bytes(B) bytes, 4-byte aligned, initialised inside the call.
 * n = 0 is a successful no-op.  Argument errors are reported before any device call. */
size_t unerf_eval_images_workspace_bytes(int B);
int unerf_eval_images_batch(const float* pred, const float* target, const float* sigma, int64_t n, int B, float unc_lo,
                            float unc_span, const uint8_t* lut, uint8_t* gt8, uint8_t* pred8, uint8_t* err8, uint8_t* std8,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------- LPIPS ------
 * The `lpips` entry of metrics.json (scripts/eval_uncertainty.py:681-689: model.lpips = torchmetrics'
 * LearnedPerceptualImagePatchSimilarity(net_type="alex", normalize=True)) for a batch of B image pairs of ONE size; host
 * definition uncertainty-nerf-gs_amd/metrics.py: lpips.  Exact fp32 arithmetic in the trunk (fp32-input MFMA: each
 * product rounded once, one fixed-order accumulation chain per output), float64 in the head.
 *
 * unerf_lpips_weights: DEVICE pointers to the network as the kernels read it.  conv_w[l]: [K_l, C_out_l] float32 with
 * k = (ky * ks + kx) * C_in + c  (torch's [C_out, C_in, ks, ks] weight permuted to (ky, kx, c, C_out)); conv_b[l]
 * [C_out_l]; lin_w[l] [C_out_l] (the 1x1 head); shift / scale: the ScalingLayer's 3 + 3 constants, by value.
 * Layers: 11x11 / stride 4 / pad 2, 3 -> 64;  5x5 / pad 2, 64 -> 192;  3x3 / pad 1, 192 -> 384, 384 -> 256, 256 -> 256;
 * a 3 / 2 max-pool in front of the second and the third. */
#define UNERF_LPIPS_LAYERS 5
typedef struct {
    const float* conv_w[UNERF_LPIPS_LAYERS];
    const float* conv_b[UNERF_LPIPS_LAYERS];
    const float* lin_w[UNERF_LPIPS_LAYERS];
    float shift[3];
    float scale[3];
} unerf_lpips_weights;

/* Row of float64 results per image: [l] sum over the pixels of tap l of sum_c lin_w[c] (f0_c / n0 - f1_c / n1)^2 with
 * n = sqrt(1e-8 + sum_c f_c^2), everything behind the fp32 features in float64; [5 + l] the pixel count of tap l;
 * [10] the number of values of the (clipped) prediction and of the target outside [0, 1] or NaN.
 * LPIPS = sum_l row[l] / row[5 + l], valid when row[10] == 0 (metrics.py: finish_lpips). */
#define UNERF_LPIPS_ROW 11
#define UNERF_LPIPS_BAD_OFF 10
#define UNERF_LPIPS_MIN_SIDE 31      /* below it the second max-pool has no output */
#define UNERF_LPIPS_CONV_TILE_M 64   /* output pixels per workgroup of the convolution kernel (its row tile) */
#define UNERF_LPIPS_CONV_TILE_N 64   /* output channels per workgroup: C_out must be a multiple */
#define UNERF_LPIPS_HEAD_PIXELS 64   /* pixels per workgroup of the head kernel */
#define UNERF_LPIPS_CONV_STEP_K 16   /* reduction terms per step of the convolution kernel; the last step may be partial */
#define UNERF_LPIPS_EW_THREADS 256   /* threads per workgroup of the pack and max-pool kernels */
#define UNERF_LPIPS_EW_MAX_WG 4096   /* their grid is capped here: beyond EW_THREADS * EW_MAX_WG values a thread strides */

/* The input pack: pred / target [B, n, 3] float32 (HWC) -> act [2 B, n, 3]: prediction b at b, target b at B + b, each
 * ((2 x - 1) - shift[c]) / scale[c] in float32, one rounding per operation, with x = the prediction clipped to <= 1 (a
 * NaN stays one) or the target.  bad [B] uint32 (zeroed inside the call): values of image b outside [0, 1] or NaN,
 * counted with integer atomics (order-free). */
int unerf_lpips_pack(const float* pred, const float* target, int64_t n, int B, const unerf_lpips_weights* w, float* act,
                     uint32_t* bad, void* stream);

/* out[img, oy, ox, co] = relu?(bias[co] + sum_{ky, kx, c} in[img, oy stride - pad + ky, ox stride - pad + kx, c]
 * w[(ky ks + kx) C_in + c, co]), NHWC float32, taps outside the image contributing zero (predicated loads, no padded
 * copy); H_out = (H + 2 pad - ks) / stride + 1 (floor), W_out likewise.  An implicit GEMM on the fp32-input MFMA
 * (32x32x2): rows = the N H_out W_out output pixels of all images in tiles of UNERF_LPIPS_CONV_TILE_M (a tile may
 * straddle images), columns = C_out in tiles of UNERF_LPIPS_CONV_TILE_N (C_out must be a multiple), reduction over
 * K = ks ks C_in in ascending k (any K >= 1).  Every output is ONE accumulation chain in that order, then + bias, then
 * the ReLU: two calls give equal bits.  w: [K, C_out] as in unerf_lpips_weights. */
int unerf_conv2d_bias_relu(const float* in, const float* w, const float* bias, float* out, int N, int H, int W, int C_in,
                           int C_out, int ks, int stride, int pad, int relu, void* stream);

/* max_pool2d(kernel 3, stride 2, no padding, floor mode) on NHWC float32: out [N, (H - 3) / 2 + 1, (W - 3) / 2 + 1, C];
 * exact, a NaN in a window is its result (torch's rule).  H, W >= 3. */
int unerf_maxpool3s2(const float* in, float* out, int N, int H, int W, int C, void* stream);

/* The head for one tap: feats [2 B, P, C] float32 (image b at b, its partner at B + b), lin_w [C] -> out[b * out_stride]
 * = the sum over the P pixels described at UNERF_LPIPS_ROW, float64.  One workgroup per UNERF_LPIPS_HEAD_PIXELS pixels
 * and image (the image is grid.y) writes a partial into the workspace, a second kernel adds an image's partials in index
 * order: no floating-point atomics, the value of image b does not depend on B.
 * workspace: B * ceil(P / UNERF_LPIPS_HEAD_PIXELS) doubles, 8-byte aligned. */
int unerf_lpips_head(const float* feats, const float* lin_w, int64_t P, int C, int B, void* workspace, size_t workspace_bytes,
                     double* out, int64_t out_stride, void* stream);

/* pred / target [B, H, W, 3] float32, 1 <= B <= UNERF_METRICS_MAX_IMAGES, H, W >= UNERF_LPIPS_MIN_SIDE and
 * 6 B H W < 2^31 -> out [B, UNERF_LPIPS_ROW].  Row b equals the row of image b alone bit for bit; two calls give equal
 * rows.  Launches (whatever B is): one memset, the pack, five convolutions, two max-pools, five head pairs, one kernel
 * that fills the counts.  workspace: unerf_lpips_workspace_bytes(H, W, B) bytes (0 for an unsupported size), 256-byte
 * aligned: every activation of the trunk (about 61 bytes per input pixel for each of the 2 B stacked images) and the
 * head's partials; nothing in it is read before it is written.  Argument errors (NULL pointer, H or W < 31, short workspace)
 * are reported before any device call. */
size_t unerf_lpips_workspace_bytes(int H, int W, int B);
int unerf_lpips_batch(const float* pred, const float* target, int H, int W, int B, const unerf_lpips_weights* w,
                      void* workspace, size_t workspace_bytes, double* out, void* stream);

/* ================================================================ splats ==
 * gsplat 0.1.11 call sites in models/activesplatfacto/activesplatfacto_model.py. */

/* :221-234 project_gaussians(means3d, scales, glob_scale, quats, viewmat, fx, fy, cx, cy, H, W, 16).
 * viewmat_host: 12 or 16 floats row-major (first 3 rows used).  Outputs as gsplat:
 * xys[N,2], depths[N], radii[N] i32, conics[N,3], compensation[N], num_tiles_hit[N] i32, cov3d[N,6]. */
int unerf_splat_project(const float* means3d, const float* scales, float glob_scale, const float* quats,
                        const float* viewmat_host, float fx, float fy, float cx, float cy, int H, int W,
                        int block_width, float clip_thresh, int64_t N, float* xys, float* depths, int32_t* radii,
                        float* conics, float* compensation, int32_t* num_tiles_hit, float* cov3d, void* stream);

/* The same projection fed with the model's parameters as stored: log_scales [N,3] (gauss_params.scales) and raw_quats
 * [N,4] (gauss_params.quats, unnormalised).  Replaces torch.exp(scales_crop) and quats_crop / quats_crop.norm(dim=-1,
 * keepdim=True) (:221-223) + project_gaussians: three elementwise launches less per frame.
 * opacity_logits [N] (may be NULL): gauss_params.opacities.  When given, opacities_out [N] receives
 * sigmoid(opacity_logits) (:256), times the compensation when antialiased != 0 (:252-254), and num_tiles_hit becomes
 * TIGHT: it counts only the tiles of gsplat's box in which some pixel centre can have alpha >= 1/255 for that opacity
 * (the ellipse sigma <= ln(255 o); about half of the box for the bench scene).  The pairs left out are pairs the blend
 * loop skips by itself, so every rasterised output is bit-identical -- with shorter lists to sort and stage.  A tight
 * count must be binned by unerf_splat_bin_sort with tight_conics / tight_opacities = these conics / opacities_out.
 * radii, xys, ... stay gsplat's (radii > 0 is still "visible"). */
int unerf_splat_project_raw(const float* means3d, const float* log_scales, float glob_scale, const float* raw_quats,
                            const float* viewmat_host, float fx, float fy, float cx, float cy, int H, int W,
                            int block_width, float clip_thresh, int64_t N, const float* opacity_logits, int antialiased,
                            float* opacities_out, float* xys, float* depths, int32_t* radii, float* conics,
                            float* compensation, int32_t* num_tiles_hit, float* cov3d, void* stream);

/* :245-246 spherical_harmonics(degree, viewdirs, coeffs[N,16,3]) then clamp(+0.5, min 0);
 * and :286 softplus(log_unc)+beta_min.  cam_pos_host: 3 floats.  colors_out [N,3], beta_out [N].
 * degree = -1: the config.sh_degree == 0 branch (:247-248), colors = sigmoid(DC coefficients), no SH, no +0.5.
 * sh_coeffs must be 16-byte aligned (rows of 48 floats are read as 16-byte loads). */
int unerf_splat_sh_colors(int degree, const float* means3d, const float* cam_pos_host, const float* sh_coeffs,
                          const float* log_unc, float beta_min, int64_t N, float* colors_out, float* beta_out,
                          void* stream);

/* The same with the coefficients as the model stores them -- gauss_params.features_dc [N,3] and
 * gauss_params.features_rest [N,15,3] -- i.e. without the torch.cat of activesplatfacto_model.py:242-243
 * (192 B per splat written and read back every frame).  features_rest may be NULL for degree 0. */
int unerf_splat_sh_colors_split(int degree, const float* means3d, const float* cam_pos_host, const float* features_dc,
                                const float* features_rest, const float* log_unc, float beta_min, int64_t N,
                                float* colors_out, float* beta_out, void* stream);

/* Everything the rasteriser reads per splat, in one launch and in its final layout: SH colours (as
 * unerf_splat_sh_colors_split), beta = softplus(log_unc) + beta_min (:286), the depth channel, and
 * opacities = sigmoid(opacity_logits) [* compensation] (:252-256).  Replaces the torch.cat([rgbs, beta, depths]) and
 * torch.sigmoid launches of the frame.  rows_out [N,C]: C = 5 -> [r, g, b, beta, depth]; C = 4 -> [r, g, b, depth]
 * (plain splatfacto; log_unc may be NULL).  compensation may be NULL ("classic").  opacities_out [N].
 * opacity_logits may be NULL (the opacities were made by unerf_splat_project_raw): opacities_out is then not written. */
int unerf_splat_shade_inputs(int degree, const float* means3d, const float* cam_pos_host, const float* features_dc,
                             const float* features_rest, const float* log_unc, float beta_min,
                             const float* opacity_logits, const float* compensation, const float* depths, int64_t N,
                             int C, float* rows_out, float* opacities_out, void* stream);

/* bin-and-sort done ONCE per frame (the reference repeats it inside each of its four
 * rasterize_gaussians calls :260,:289,:306,:343).  cum_tiles_hit [N] i32 (inclusive scan,
 * output), isect_ids [I] i64 + gaussian_ids [I] i32 sorted outputs, tile_bins [tiles,2] i32.
 * Two-step use: call unerf_splat_count_intersects (async; writes the scan and *num_intersects
 * on device), read it back, size the buffers, then unerf_splat_bin_sort.
 * The sorted order is that of gsplat's stable sort of (tile << 32 | depth bits) keys; it is produced by
 * ordering the N splats by depth first and then sorting the intersections by tile id only (stable).
 * isect_ids_sorted may be NULL (the rasteriser needs only gaussian_ids_sorted and tile_bins).
 * tight_conics [N,3] + tight_opacities [N] (both or neither): cum_tiles_hit is the scan of a TIGHT num_tiles_hit
 * (unerf_splat_project_raw with opacity logits) -- each splat then emits exactly the tiles that count was made of.
 * NULL, NULL: gsplat's lists (every tile of the radius box). */
int64_t unerf_splat_sort_workspace_bytes(int64_t N, int64_t num_intersects);
int unerf_splat_count_intersects(const int32_t* num_tiles_hit, int64_t N, int32_t* cum_tiles_hit,
                                 void* workspace, int64_t workspace_bytes, void* stream);
int unerf_splat_bin_sort(const float* xys, const float* depths, const int32_t* radii,
                         const int32_t* cum_tiles_hit, int64_t N, int64_t num_intersects, int H, int W,
                         int block_width, const float* tight_conics, const float* tight_opacities,
                         int64_t* isect_ids_sorted, int32_t* gaussian_ids_sorted,
                         int32_t* tile_bins, void* workspace, int64_t workspace_bytes, void* stream);

/* rasterize_forward / nd_rasterize_forward: C channels blended in one pass.
 * colors [N,C] (C<=8), opacities [N], background [C] DEVICE (NULL = zeros),
 * out_img [H,W,C], final_T [H,W], final_idx [H,W] i32 (may be NULL): index (into gaussian_ids_sorted) of the last splat
 * blended into the pixel, 0 when there is none.
 * stop_idx [H,W] i32 (may be NULL): the final_idx of an earlier pass over the SAME ids / bins / xys / conics / opacities
 * (the reference's depth-variance pass, :343-356, after its rgb pass): each pixel then stops behind that index instead
 * of re-deriving its end from the transmittance -- same blended terms, same result.
 * flags: 0, or UNERF_RASTER_NO_CULL to walk every staged splat in every wave (gsplat's schedule).  By default a wave (a
 * 4-row strip of the 16 x 16 tile) walks only the splats whose alpha >= 1/255 ellipse can reach its strip; the skipped
 * (pixel, splat) pairs are pairs the blend loop would have skipped itself, so both settings give identical bits.
 * chan_max (may be NULL): 1 DEVICE float the caller zeroed; on return it holds max(chan_max, max over the image of
 * out_img[..., max_channel]) -- the `img.max()` that unerf_splat_alpha_normalize(max_ready = 1) then needs not
 * compute.  Values of that channel must be >= 0 (depths, squared differences). */
#define UNERF_RASTER_NO_CULL 1
int unerf_splat_rasterize(const int32_t* gaussian_ids_sorted, const int32_t* tile_bins, const float* xys,
                          const float* conics, const float* colors, const float* opacities,
                          const float* background, int C, int H, int W, int block_width, const int32_t* stop_idx,
                          int flags, int max_channel, float* chan_max, float* out_img, float* final_T,
                          int32_t* final_idx, void* stream);

/* :319 / :356  img = where(alpha>0, img/alpha, max(img)) with alpha = 1-final_T, applied IN PLACE
 * to channel `ch` of an interleaved image [HW, stride]; scratch_max = 1 device float.
 * max_ready = 0: max(img[..., ch]) is computed here into scratch_max;  1: scratch_max already holds it (the chan_max
 * of the unerf_splat_rasterize call that produced img). */
int unerf_splat_alpha_normalize(float* img, int stride, int ch, const float* final_T, int64_t HW,
                                float* scratch_max, int max_ready, void* stream);

/* The frame's per-pixel epilogue in ONE pass over the image (activesplatfacto_model.py:275 rgb clamp, :319 / :356 depth
 * normalisation, :359-367 accumulation / rgb_var / depth_std -- torch calls in the reference).  Channel `ch` of img [HW, stride]
 * is normalised IN PLACE exactly as unerf_splat_alpha_normalize(max_ready = 1) does (scratch_max: the 1 device float that holds
 * max(img[..., ch]), left by the unerf_splat_rasterize call that produced img), and any of these is written (NULL: skipped):
 *   rgb_out  [HW,3] = min(img[..., 0:3], 1)   torch.clamp(max=1.0): NaN stays NaN; needs ch >= 3
 *   acc_out  [HW]   = 1 - final_T
 *   sq_out   [HW]   = img[..., sq_ch]^2       (rgb_var = uncertainty^2; sq_ch != ch)
 *   sqrt_out [HW]   = sqrt(the normalised channel ch)   (depth_std = sqrt(depth_var)) */
int unerf_splat_normalize_outputs(float* img, int stride, int ch, const float* final_T, int64_t HW,
                                  const float* scratch_max, float* rgb_out, float* acc_out, int sq_ch, float* sq_out,
                                  float* sqrt_out, void* stream);
/* :325-341 per-splat (z_i - depth[floor(xy_i)])^2, bounds test with the reference's strict ">0";
 * depth image = channel `ch` of [H,W,stride].  sq_diff_out [N]. */
int unerf_splat_depth_sqdiff(const float* xys, const float* depths, const float* depth_img, int stride, int ch,
                             int H, int W, int64_t N, float* sq_diff_out, void* stream);

/* ---------------------------------------------------------------- splats, B views per call --
 * B cameras of ONE splat set and ONE image size H x W in each launch: the evaluation loop over a test set's cameras
 * (scripts/eval_uncertainty.py:896-904, which calls ActiveSplatfactoModel.get_outputs once per camera,
 * activesplatfacto_model.py:155 asserts one camera) rendered a batch at a time.  Every view's outputs are BIT-identical to the
 * single-view entry points above with that view's camera.  Per-view arrays are view-major: [B, N, ...] / [B, H, W, ...], view v
 * at offset v N / v H W.  Limits: 1 <= B <= UNERF_SPLAT_MAX_VIEWS; B N < UNERF_SPLAT_MAX_BATCH_SPLATS (2^29: ids v N + i are
 * int32 and the rasteriser forms 3 id in 32 bits); the batch's intersections sum to < 2^31 (int32 ids and bins).
 * views_host: B records of UNERF_SPLAT_VIEW_FLOATS HOST floats, [world-to-camera rows 0..2 (12, row-major), fx, fy, cx, cy,
 * camera position (3)] -- the viewmat / intrinsics / cam_pos of the single-view calls. */
#define UNERF_SPLAT_MAX_VIEWS 16
#define UNERF_SPLAT_VIEW_FLOATS 19
#define UNERF_SPLAT_MAX_BATCH_SPLATS (1ll << 29)
/* largest image unerf_splat_bin_sort_batch serves, in tiles (1080p at block_width 16: 8,160) */
#define UNERF_SPLAT_BATCH_MAX_TILES 11999

/* :221-234 as unerf_splat_project_raw, for B views in one launch: each splat's parameters are read once.  Outputs [B,N,...];
 * opacities_out [B,N] (with opacity_logits; antialiased: times each view's compensation); cov3d [B,N,6] may be NULL. */
int unerf_splat_project_batch(const float* means3d, const float* log_scales, float glob_scale, const float* raw_quats,
                              const float* views_host, int B, int H, int W, int block_width, float clip_thresh, int64_t N,
                              const float* opacity_logits, int antialiased, float* opacities_out, float* xys, float* depths,
                              int32_t* radii, float* conics, float* compensation, int32_t* num_tiles_hit, float* cov3d,
                              void* stream);

/* :242-256, :286 as unerf_splat_shade_inputs, for B views in one launch (the camera positions of views_host): the SH
 * coefficients are read once.  compensation [B,N] (may be NULL), depths [B,N]; rows_out [B,N,C], opacities_out [B,N]. */
int unerf_splat_shade_inputs_batch(int degree, const float* means3d, const float* views_host, int B, const float* features_dc,
                                   const float* features_rest, const float* log_unc, float beta_min,
                                   const float* opacity_logits, const float* compensation, const float* depths, int64_t N,
                                   int C, float* rows_out, float* opacities_out, void* stream);

/* Workspace of unerf_splat_count_intersects_batch / unerf_splat_bin_sort_batch for B views of N splats and num_intersects
 * pairs over all views; -1 outside the limits above. */
int64_t unerf_splat_sort_workspace_bytes_batch(int B, int64_t N, int64_t num_intersects);

/* compute_cumulative_intersects for a batch: ONE inclusive scan over the B N tile counts -> cum_tiles_hit [B,N], and the
 * batch's one host read-back, summary [2B] i32 DEVICE: summary[v] = view v's intersections, summary[B + v] = 1 when some
 * radius of view v is > 0 (radii [B,N] may be NULL: then summary[B + v] = (summary[v] > 0)) -- with tight counts a view can
 * have no intersections and still be "visible" (its splats all fainter than 1/255): the reference then rasterises a frame
 * in which nothing blends instead of returning get_empty_outputs (activesplatfacto_model.py:239-240).  Async. */
int unerf_splat_count_intersects_batch(const int32_t* num_tiles_hit, const int32_t* radii, int B, int64_t N,
                                       int32_t* cum_tiles_hit, int32_t* summary, void* workspace, int64_t workspace_bytes,
                                       void* stream);

/* unerf_splat_bin_sort for a batch.  isects_host: the B per-view totals of the summary (HOST int64).  gaussian_ids_sorted
 * [sum of isects_host] holds ids v N + i, view after view, each view in its single-view order; tile_bins [B, tiles, 2] of view
 * v index that whole array.  Serves at most UNERF_SPLAT_BATCH_MAX_TILES tiles (the staged tile sort's
 * LDS tables); gsplat's 64-bit isect ids are not produced. */
int unerf_splat_bin_sort_batch(const float* xys, const float* depths, const int32_t* radii, const int32_t* cum_tiles_hit,
                               int B, int64_t N, const int64_t* isects_host, int H, int W, int block_width,
                               const float* tight_conics, const float* tight_opacities, int32_t* gaussian_ids_sorted,
                               int32_t* tile_bins, void* workspace, int64_t workspace_bytes, void* stream);

/* unerf_splat_rasterize for a batch (grid: tiles x B): tile_bins [B,tiles,2] and ids of unerf_splat_bin_sort_batch; xys,
 * conics, colors, opacities [B,N,...]; background [C] shared; stop_idx / out_img / final_T / final_idx [B,H,W,...];
 * chan_max [B]: each view's own maximum (the reference normalises every image by its own max()). */
int unerf_splat_rasterize_batch(const int32_t* gaussian_ids_sorted, const int32_t* tile_bins, const float* xys,
                                const float* conics, const float* colors, const float* opacities, const float* background,
                                int B, int C, int H, int W, int block_width, const int32_t* stop_idx, int flags,
                                int max_channel, float* chan_max, float* out_img, float* final_T, int32_t* final_idx,
                                void* stream);

/* unerf_splat_normalize_outputs for a batch: img [B,HW,stride], final_T [B,HW], scratch_max [B], outputs [B,HW,...]. */
int unerf_splat_normalize_outputs_batch(float* img, int stride, int ch, const float* final_T, int B, int64_t HW,
                                        const float* scratch_max, float* rgb_out, float* acc_out, int sq_ch, float* sq_out,
                                        float* sqrt_out, void* stream);

/* unerf_splat_depth_sqdiff for a batch: xys [B,N,2], depths [B,N], depth_img [B,H,W,stride], sq_diff_out [B,N]. */
int unerf_splat_depth_sqdiff_batch(const float* xys, const float* depths, const float* depth_img, int stride, int ch, int B,
                                   int H, int W, int64_t N, float* sq_diff_out, void* stream);

/* ------------------------------------------------- splat pose gradient --
 * d mean_c(rgb[y,x]) / d camera_to_worlds of a splat frame per pixel (the quantity of the reference's
 * scripts/estimate_gradient_pose_6dof.py:128-139, which itself serves nerfacto models only), in forward mode: the pose reaches
 * a pixel only through each splat's projected q = (u, v, conic a, conic b, conic c, compensation) -- the SH view directions
 * are detached (activesplatfacto_model.py:243); near-plane cull, radii, tile lists, skipped pairs and stops are held fixed.
 *
 * unerf_splat_pose_tangents: tangents [N, UNERF_SPLAT_POSE_Q, 12] <- d q / d V[r][c] (k = 4 r + c over the 3 x 4 world-to-camera
 * rows `viewmat_host`), through the arithmetic of unerf_splat_project* behind its `cov3d` [N,6] output.  Splats with
 * radii == 0 get zeros.  The fov clamp passes no x (y) sensitivity where it is active, compensation has derivative 0 where
 * det_orig <= 0.  288 bytes per splat; 16-byte aligned. */
#define UNERF_SPLAT_POSE_Q 6
int unerf_splat_pose_tangents(const float* means3d, const float* cov3d, const int32_t* radii, int64_t N,
                              const float* viewmat_host, float fx, float fy, float cx, float cy, int H, int W,
                              float clip_thresh, float* tangents, void* stream);

/* The walk of unerf_splat_rasterize (same lists, same skip and stop decisions, C = 3, flags as there) carrying the 12 tangents
 * of T and of the three colour sums; a tile's list is staged UNERF_SPLAT_POSE_GRAD_BATCH splats at a time.
 * compensation [N] or NULL: given ("antialiased": opacities = sigmoid(.) * compensation) alpha also moves with the
 * compensation's tangent; NULL ("classic") the tangents' last 12 floats per splat are not read.
 * background [3] DEVICE or NULL (zeros).  c2w_host: the 3 x 4 camera-to-world rows V was made from
 * (V = [R'^T | -R'^T t], R' = R diag(1,-1,-1), the reference's transposition :184-195) -> out_grad [H W, 3, 4] = ds / d c2w;
 * NULL -> out_grad [H W, 12] = ds / dV.  s = mean_c min(pix_c + T bg_c, 1): a channel at or above 1 contributes 0; alpha on its
 * 0.999 clamp has derivative 0.  out_rgb [H W,3] (the clamped colour) and final_T [H W] may be NULL.
 * No atomics, no division by 1 - alpha: two calls return the same bits. */
#define UNERF_SPLAT_POSE_GRAD_BATCH 128
int unerf_splat_pose_grad(const int32_t* gaussian_ids_sorted, const int32_t* tile_bins, const float* xys,
                          const float* conics, const float* colors, const float* opacities, const float* compensation,
                          const float* tangents, const float* background, const float* c2w_host, int H, int W,
                          int block_width, int flags, float* out_grad, float* out_rgb, float* final_T, void* stream);

/* ------------------------------------------------- splat pose Jacobian --
 * The per-pixel Jacobian of the frame's five channels (UNERF_POSE_CH_*, rows in bit order) with respect to P pose directions,
 * and its sum of squares (the first-order variance J Sigma J^T when the directions are a basis times a Cholesky factor).  The
 * pose reaches a pixel linearly through the per-splat tangents, so the [12,P] projection is contracted per splat, before the
 * walk, which then carries 5 P running tangents instead of 5 x 12.  fp32, no atomics, no global scratch: two calls return the
 * same bits.
 *
 * unerf_splat_pose_tangents_proj: ptangents [N, UNERF_SPLAT_POSE_PROJ_ROWS, PW] from tangents [N,6,12] (unerf_splat_pose_tangents)
 * and proj_host [12][P] (host, row-major; rows = the entries k = 4 r + c of V[:3,:4]), PW = UNERF_SPLAT_POSE_PW(P):
 *   rows 0..5: out[q][p] = sum_k tangents[q][k] proj[k][p], summed over k in order;
 *   row 6    : the tangent of the splat's camera-space depth z = V[2] . (m, 1): sum_c m[c] proj[8 + c][p], m[3] = 1; zeros where
 *              radii == 0.
 * Columns P .. PW-1 are written as exact zeros.  ptangents is 8-byte aligned for PW = 6, 16-byte aligned for PW = 12. */
#define UNERF_SPLAT_POSE_PROJ_ROWS 7
#define UNERF_SPLAT_POSE_MAX_P 12
#define UNERF_SPLAT_POSE_PW(P) ((P) <= 6 ? 6 : 12)
int unerf_splat_pose_tangents_proj(const float* tangents, const float* means3d, const int32_t* radii, int64_t N,
                                   const float* proj_host, int P, float* ptangents, void* stream);

/* The walk of unerf_splat_pose_grad (same lists, skip and stop decisions, UNERF_SPLAT_POSE_GRAD_BATCH records per staging
 * round, flags as there) carrying T, pix[3], D = sum_i z_i alpha_i T_i (depths [N]: the unnormalised depth sum of the frame) and
 * their PW tangents.  compensation [N] or NULL as there (NULL: row 5 of ptangents is not read).  background [3] DEVICE or NULL.
 * channels: a non-empty set of UNERF_POSE_CH_*; C = its size, rows in bit order; the mask gates stores only, so a row's bits
 * do not depend on which other channels are asked for.
 *   R, G, B : value min(pix_c + T bg_c, 1); row live_c (dpix_c + bg_c dT), live_c = pix_c + T bg_c < 1
 *   ACC     : value A = 1 - T; row -dT
 *   EDEPTH  : A > 0: value D / A, row dD / A + (D / A) dT / A;  A == 0: value and row exactly 0 (the frame's max(depth) fill
 *             of such pixels is a quantity of other pixels and is left to the caller)
 * out_proj [H W, C, P] (the rows), out_var [H W, C] (sum_p row[p]^2 over p < P in order), out_val [H W, C]: each may be NULL,
 * not all three.  H W == 0 or empty lists are not an error. */
int unerf_splat_pose_jacobian(const int32_t* gaussian_ids_sorted, const int32_t* tile_bins, const float* xys,
                              const float* conics, const float* colors, const float* depths, const float* opacities,
                              const float* compensation, const float* ptangents, const float* background, int P, int H, int W,
                              int block_width, int flags, int channels, float* out_proj, float* out_var, float* out_val,
                              void* stream);

/* ------------------------------------------------- splat pose Jacobian, B views per call --
 * The two stages above for B cameras of one splat set and one image size in shared launches, in the view-major layout and under
 * the limits of "splats, B views per call" (1 <= B <= UNERF_SPLAT_MAX_VIEWS, B N < UNERF_SPLAT_MAX_BATCH_SPLATS, intersections
 * < 2^31, at most UNERF_SPLAT_BATCH_MAX_TILES tiles).  Every view's block is BIT-identical to the single-view entry points with
 * that view's camera and matrix.
 *
 * unerf_splat_pose_ptangents_batch: ptangents [B, N, UNERF_SPLAT_POSE_PROJ_ROWS, PW] <- unerf_splat_pose_tangents followed by
 * unerf_splat_pose_tangents_proj for every (view, splat), in one launch and without the 288-byte tangent row in memory.
 * cov3d [B,N,6], radii [B,N]: as unerf_splat_project_batch writes them (rows of splats culled in a view are zero and not read);
 * views_host: the batch's B records (rows 0..2 of the view matrix, fx, fy are used); proj [B,12,P]: DEVICE floats, one [12][P]
 * matrix per view (rows = the entries k = 4 r + c of V[:3,:4]) -- the se3 basis in entries of V depends on each view's pose.
 * Rows 0..5 are summed over k in order, row 6 is the depth row, rows are zero where radii == 0, columns P .. PW-1 are exact
 * zeros; ptangents aligned as for unerf_splat_pose_tangents_proj.  N == 0 is not an error. */
int unerf_splat_pose_ptangents_batch(const float* means3d, const float* cov3d, const int32_t* radii, const float* views_host,
                                     int B, int64_t N, const float* proj, int P, int H, int W, float clip_thresh,
                                     float* ptangents, void* stream);

/* unerf_splat_pose_jacobian for a batch (grid: tiles x B): gaussian_ids_sorted (ids v N + i) and tile_bins [B,tiles,2] of
 * unerf_splat_bin_sort_batch; xys, conics, depths, opacities, compensation [B,N,...]; colors [B,N,color_stride] of which the first
 * three floats of a row are read (color_stride >= 3: the rows of unerf_splat_shade_inputs_batch in place); ptangents
 * [B,N,7,PW]; background [3] shared.  out_proj [B,HW,C,P], out_var [B,HW,C], out_val [B,HW,C]: each may be NULL, not all three.
 * Channels, flags, the A == 0 rule, the clamp rules and "the mask gates stores only" as in unerf_splat_pose_jacobian; N enters
 * the limit check only.  No atomics, no global scratch: two calls return the same bits, and a view's bits depend neither on the
 * other views nor on its place in the batch.  H W == 0 or empty lists are not an error. */
int unerf_splat_pose_jacobian_batch(const int32_t* gaussian_ids_sorted, const int32_t* tile_bins, const float* xys,
                                    const float* conics, const float* colors, int color_stride, const float* depths,
                                    const float* opacities, const float* compensation, const float* ptangents,
                                    const float* background, int B, int64_t N, int P, int H, int W, int block_width, int flags,
                                    int channels, float* out_proj, float* out_var, float* out_val, void* stream);

/* ---- Pose normal equations of a frame: the float64 reduction of a per-pixel pose Jacobian -------------------------------
 * What a consumer of out_proj [R,C,P] (unerf_pose_jacobian, unerf_splat_pose_jacobian) and out_val asks for first, without
 * holding the frame's Jacobian: over the pixels n and channels c of a frame
 *   H = sum w J J^T  [P,P]   the Fisher information of the pose under the weights w (Gauss-Newton matrix)
 *   g = sum w r J    [P]     the gradient of the weighted photometric cost 1/2 sum w r^2, r = val - target
 *   chi2 = sum w r^2
 * Per term, everything in float64 formed from the float32 inputs, in THIS product order:
 *   J_k = (double)jac[n,c,k];  r = (double)val[n,c] - (double)target[n,c];  w = weight ? (double)weight[...] : 1.0
 *   H_ab = fma(w * J_a, J_b, H_ab) for a <= b;   g_a = fma(w * r, J_a, g_a);   chi2 = fma(w * r, r, chi2)
 * With val and target both NULL r is not formed: g and chi2 are exactly 0 and only H is accumulated.
 * A pixel with mask[n] == 0 contributes nothing and is not counted.  A term (n, c) is SKIPPED and counted in n_skipped when
 * one of jac[n,c,0..P-1], r or w is not finite or w < 0; every other term counts in n_used.
 *
 * Geometry: a workgroup of UNERF_POSE_NEQ_THREADS threads owns ONE tile of UNERF_POSE_NEQ_TILE consecutive pixels by the
 * absolute pixel index pixel_offset + n; thread t takes pixels t, t + THREADS, ... of the tile (UNERF_POSE_NEQ_PPT of them) in
 * that order, the channels of a pixel in order; then wave butterfly -> LDS -> the four waves in order -> ONE row of
 * UNERF_POSE_NEQ_WS_ROW(P) doubles of the workspace (the packed upper triangle of H, g, chi2, the two counts).  No atomics.
 * unerf_pose_normal_eq_finish sums the tile rows [0, ceil(N_frame / TILE)) in one fixed order: thread t of
 * UNERF_POSE_NEQ_REDUCE_THREADS takes rows t, t + REDUCE_THREADS, ... in order, then butterfly -> LDS -> the waves in order.
 * So two calls give the same bits, the bits do not depend on how the frame was cut into tile-aligned launch groups or on their
 * order, and a tile's partial does not depend on the other tiles.  The longest chain of additions an entry passes through:
 *   PPT * C  +  6  +  (THREADS / 64 - 1)  +  ceil(tiles / REDUCE_THREADS)  +  6  +  (REDUCE_THREADS / 64 - 1)
 * The caller zero-fills the workspace ONCE per frame, so tiles never written add +0.0.  A tile's row is written whole by the
 * call that covers it: a group that ends inside a tile must be the frame's last.
 *
 *   jac [R,C,P] device floats; val, target [R,C] both or neither; weight NULL | [R] (weight_per_channel == 0) | [R,C];
 *   mask NULL | [R] bytes; workspace: unerf_pose_normal_eq_workspace_bytes(N_frame, P) bytes, 8-byte aligned.
 *   out (device): UNERF_POSE_NEQ_ROW(P) doubles = H [P,P] row-major, the lower triangle copied from the upper (exactly
 *   symmetric) | g [P] | chi2 | n_used | n_skipped.
 * UNERF_ERR_ARG before any launch, each with its own message: P outside [1, 12]; C outside [1, 5]; R < 0 (R == 0 is
 * UNERF_OK); exactly one of val / target; pixel_offset negative or not a multiple of the tile; pixel_offset + R > N_frame;
 * null jac or workspace; workspace_bytes too small.  Instantiated for P <= 6 and P <= 12 (UNERF_SPLAT_POSE_PW). */
#define UNERF_POSE_NEQ_THREADS 256
#define UNERF_POSE_NEQ_PPT 4
#define UNERF_POSE_NEQ_TILE (UNERF_POSE_NEQ_THREADS * UNERF_POSE_NEQ_PPT)
#define UNERF_POSE_NEQ_REDUCE_THREADS 256
#define UNERF_POSE_NEQ_MAX_P 12
#define UNERF_POSE_NEQ_MAX_C 5
#define UNERF_POSE_NEQ_ROW(P) ((P) * (P) + (P) + 3)
#define UNERF_POSE_NEQ_WS_ROW(P) ((P) * ((P) + 1) / 2 + (P) + 3)
size_t unerf_pose_normal_eq_workspace_bytes(int64_t N_frame, int P);
int unerf_pose_normal_eq_accumulate(const float* jac, const float* val, const float* target, const float* weight,
                                    int weight_per_channel, const uint8_t* mask, int64_t R, int C, int P, int64_t pixel_offset,
                                    int64_t N_frame, void* workspace, size_t workspace_bytes, void* stream);
int unerf_pose_normal_eq_finish(const void* workspace, size_t workspace_bytes, int64_t N_frame, int P, double* out,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNERF_H */
