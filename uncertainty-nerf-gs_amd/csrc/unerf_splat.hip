// Gaussian-splat half of libunerf (gsplat 0.1.11 semantics, see include/unerf.h):
// EWA projection, SH colours + per-splat beta, one bin-and-sort per frame, tile rasteriser with
// C interleaved channels, alpha normalisation and the per-splat depth-difference gather.
// Built with -ffp-contract=off: projection / tile boxes / sort keys are bit-exact against the
// numpy oracle (oracle/splat_oracle.py) which performs the same fp32 operations in the same order.
#include "unerf_common.hpp"
#include <type_traits>

#include <hipcub/hipcub.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>

static inline unsigned blocks_for(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// ======================================================================================
// projection
// ======================================================================================
// one camera of a projection: world-to-camera rows and the intrinsics
struct ProjCam {
    float V[12];
    float fx, fy, cx, cy;
};
// NV: camera records the launch carries -- 1 for the single-view entry points (their kernel arguments stay as small as
// before), UNERF_SPLAT_MAX_VIEWS for unerf_splat_project_batch
template <int NV>
struct ProjArgs {
    const float* means;
    const float* scales;
    float glob_scale;
    const float* quats;
    // the views of the launch (1: unerf_splat_project*; up to UNERF_SPLAT_MAX_VIEWS: unerf_splat_project_batch).  Every output
    // is [nv, N, ...]: view v's rows start at v N
    int nv;
    ProjCam cam[NV];
    int H, W, bw;
    float clip;
    int64_t N;
    float* xys;
    float* depths;
    int32_t* radii;
    float* conics;
    float* comp;
    int32_t* tiles;
    float* cov3d;
    // tight binning (unerf_splat_project_raw with opacity logits): the activated opacity leaves this kernel and
    // num_tiles_hit counts only the tiles the splat's alpha >= 1/255 ellipse can reach
    const float* opl;
    float* opac_out;
    int antialiased;
};

__device__ __forceinline__ void tile_bbox(float cx, float cy, float radius, int bw, int tbx, int tby, int& x0, int& y0,
                                          int& x1, int& y1) {
    float tcx = cx / (float)bw, tcy = cy / (float)bw, tr = radius / (float)bw;
    x0 = min(max(0, (int)(tcx - tr)), tbx);
    x1 = min(max(0, (int)(tcx + tr + 1.f)), tbx);
    y0 = min(max(0, (int)(tcy - tr)), tby);
    y1 = min(max(0, (int)(tcy + tr + 1.f)), tby);
}

// ---- tight tile lists ------------------------------------------------------------------------------------------------
// gsplat bins a splat into every tile of the square [xy -+ radius] with radius = ceil(3 sqrt(lambda_max)).  The blend
// loop then skips each (pixel, splat) pair with alpha = min(0.999, o exp(-sigma)) < 1/255, i.e. everything outside the
// ellipse sigma <= ln(255 o): for an anisotropic or faint splat most tiles of the square hold no such pixel (49 % of
// the 37 M pairs of the 1 M-splat bench frame), yet each costs a sort entry and a staging slot in the rasteriser.
// TightSplat describes that ellipse (padded far above fp32 rounding, as raster_quad_mask); tight_row gives, for one
// tile row, the range of tiles whose pixel centres it can reach -- always a subset of gsplat's box, so the lists
// lose only pairs the blend loop would have skipped: images, transmittances and orders of the blended terms are
// bit-identical (tests/test_gpu_splat.py::test_tight_tile_lists_*).
struct TightSplat {
    float x, y, b;          // centre, conic b
    float k, det, inv_a, hy, ry;   // k = 2 tau a; ry = -(b / c) hx: dy of the ellipse's rightmost point (leftmost: -ry)
    float pad;
    int valid;              // 0: keep gsplat's box (not an ellipse / non-finite numbers); -1: never visible
};
// (hardware sqrt / rcp, ~1 ulp: the pad is orders of magnitude above that, and both kernels that walk a splat's rows --
// the count in project_kernel, the emission in map_intersects_kernel -- run this same code on the same stored numbers)

__device__ __forceinline__ TightSplat tight_splat(float x, float y, float op, float a, float b, float c) {
    TightSplat t;
    t.x = x; t.y = y; t.b = b;
    t.valid = 0; t.k = 0.f; t.det = 0.f; t.inv_a = 0.f; t.hy = 0.f; t.ry = 0.f; t.pad = 0.f;
    if (!(op >= 0.0039f)) {            // alpha <= opacity < 1/255 (0.00392...) at every pixel
        t.valid = (op != op) ? 0 : -1;
        return t;
    }
    const float det = a * c - b * b;
    if (!(det > 0.f) || !(a > 0.f) || !(c > 0.f)) return t;
    const float two_tau = 2.f * fmaf(__logf(255.f * op), 1.01f, 0.01f);
    const float inv_det = __builtin_amdgcn_rcpf(det);
    const float hx = __builtin_amdgcn_sqrtf(two_tau * c * inv_det);
    t.k = two_tau * a;
    t.det = det;
    t.inv_a = __builtin_amdgcn_rcpf(a);
    t.hy = __builtin_amdgcn_sqrtf(t.k * inv_det);
    t.ry = -(b * __builtin_amdgcn_rcpf(c)) * hx;
    t.pad = fmaf(fmaxf(hx, t.hy), 0.01f, 0.05f);
    const bool fin = fabsf(hx) < INFINITY && fabsf(t.hy) < INFINITY && fabsf(t.ry) < INFINITY && fabsf(t.inv_a) < INFINITY;   // false for NaN too
    t.valid = fin ? 1 : 0;
    return t;
}

// tiles [tx0, tx1) of tile row ty (inside gsplat's [x0, x1)) holding a pixel centre with sigma <= tau
__device__ __forceinline__ void tight_row(const TightSplat& t, int ty, int bw, int x0, int x1, int& tx0, int& tx1) {
    tx0 = x0; tx1 = x1;
    if (t.valid == 0) return;
    if (t.valid < 0) { tx1 = x0; return; }
    const float fbw = (float)bw, inv_bw = 1.f / fbw;   // (bw is uniform: one scalar division; exact for 16)
    // pixel-centre rows of the tile row, relative to the splat, widened by the pad
    float d0 = ((float)ty * fbw + 0.5f) - t.y - t.pad, d1 = ((float)ty * fbw + (fbw - 0.5f)) - t.y + t.pad;
    if (d0 > t.hy || d1 < -t.hy) { tx1 = x0; return; }
    d0 = fmaxf(d0, -t.hy); d1 = fminf(d1, t.hy);
    // right end (-b dy + sqrt(2 tau a - det dy^2)) / a is concave in dy: its maximum over the rows is at the rightmost
    // point's dy clamped into them; the left end is the mirror image
    const float dr = fminf(fmaxf(t.ry, d0), d1), dl = fminf(fmaxf(-t.ry, d0), d1);
    const float sr = __builtin_amdgcn_sqrtf(fmaxf(t.k - t.det * dr * dr, 0.f));
    const float sl = __builtin_amdgcn_sqrtf(fmaxf(t.k - t.det * dl * dl, 0.f));
    const float xr = (-t.b * dr + sr) * t.inv_a + t.pad, xl = (-t.b * dl - sl) * t.inv_a - t.pad;
    if (!(xr >= xl)) return;   // NaN: keep the box
    // a pixel centre c = j + 0.5 lies in tile floor((c - 0.5) / bw); the pad covers the rounding of the product
    const float fl = floorf((t.x + xl - 0.5f) * inv_bw), fr = floorf((t.x + xr - 0.5f) * inv_bw);
    tx0 = max(x0, (int)fmaxf(fl, -1e6f));
    tx1 = min(x1, (int)fminf(fr, 1e6f) + 1);
    if (tx1 < tx0) tx1 = tx0;
}

__device__ __forceinline__ int tight_count(const TightSplat& t, int bw, int x0, int y0, int x1, int y1) {
    int n = 0;
    for (int ty = y0; ty < y1; ++ty) {
        int a0, a1;
        tight_row(t, ty, bw, x0, x1, a0, a1);
        n += a1 - a0;
    }
    return n;
}

// RAW: `scales` / `quats` are the model's parameters as stored -- log-scales and unnormalised quaternions -- and the
// reference's per-frame torch prologue (activesplatfacto_model.py:221-223: torch.exp(scales_crop),
// quats_crop / quats_crop.norm(dim=-1, keepdim=True)) happens here instead of in three elementwise launches.
// MULTI (unerf_splat_project_batch): the splat's parameters are read ONCE, before the loop over the launch's views; without it
// (one view) they are read where the single-view kernel always read them -- the quaternion and scales behind the near-plane
// test, so a culled splat costs only its mean.
template <bool RAW, bool MULTI = false>
__global__ __launch_bounds__(256) void project_kernel(ProjArgs<MULTI ? UNERF_SPLAT_MAX_VIEWS : 1> a) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    const float p0 = a.means[i * 3], p1 = a.means[i * 3 + 1], p2 = a.means[i * 3 + 2];
    float q4[4], s3[3];
    auto load_shape = [&]() {
        q4[0] = a.quats[i * 4]; q4[1] = a.quats[i * 4 + 1]; q4[2] = a.quats[i * 4 + 2]; q4[3] = a.quats[i * 4 + 3];
        s3[0] = a.scales[i * 3]; s3[1] = a.scales[i * 3 + 1]; s3[2] = a.scales[i * 3 + 2];
    };
    if (MULTI) load_shape();
    const float opl = (MULTI && a.opl) ? a.opl[i] : 0.f;
    const int nv = MULTI ? a.nv : 1;
    for (int v = 0; v < nv; ++v) {
    const ProjCam& cam = a.cam[v];
    const int64_t o = (int64_t)v * a.N + i;
    // gsplat allocates every output zero-filled and a culled splat keeps the zeros of whatever it had not reached yet.  Every
    // output is held in a register (zero until computed) and stored ONCE at the end -- zero-filling the 15 dwords first and
    // overwriting them for visible splats wrote the arrays twice (WRITE_SIZE 119 MB for 60 MB of outputs).
    float o_xy[2] = {0.f, 0.f}, o_depth = 0.f, o_comp = 0.f, o_conic[3] = {0.f, 0.f, 0.f}, o_cov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int o_radius = 0, o_tiles = 0;
    float opac = 0.f, o_opac = 0.f;
    if (a.opl) {   // uniform.  sigmoid(opacities) (:256); "antialiased" multiplies the compensation in below (:252-254)
        opac = unerf_sigmoid(MULTI ? opl : a.opl[i]);
        o_opac = a.antialiased ? 0.f : opac;
    }
    auto per_splat = [&]() {
    const float* V = cam.V;
    float tx = ((V[0] * p0 + V[1] * p1) + V[2] * p2) + V[3];
    float ty = ((V[4] * p0 + V[5] * p1) + V[6] * p2) + V[7];
    float tz = ((V[8] * p0 + V[9] * p1) + V[10] * p2) + V[11];
    if (tz <= a.clip) return;      // (leaves the lambda: the stores are below)

    // scale_rot_to_cov3d
    if (!MULTI) load_shape();
    float qw = q4[0], qx = q4[1], qy = q4[2], qz = q4[3];
    if (RAW) {   // the model's normalisation (a true division, as torch's), then gsplat's own below
        const float qn = sqrtf(((qw * qw + qx * qx) + qy * qy) + qz * qz);
        qw = qw / qn; qx = qx / qn; qy = qy / qn; qz = qz / qn;
    }
    float qs = 1.f / sqrtf(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    float w = qw * qs, x = qx * qs, y = qy * qs, z = qz * qs;
    float Rm[9] = {1.f - 2.f * (y * y + z * z), 2.f * (x * y - w * z),       2.f * (x * z + w * y),
                   2.f * (x * y + w * z),       1.f - 2.f * (x * x + z * z), 2.f * (y * z - w * x),
                   2.f * (x * z - w * y),       2.f * (y * z + w * x),       1.f - 2.f * (x * x + y * y)};
    float sc0 = s3[0], sc1 = s3[1], sc2 = s3[2];
    if (RAW) { sc0 = expf(sc0); sc1 = expf(sc1); sc2 = expf(sc2); }
    float s0 = a.glob_scale * sc0, s1 = a.glob_scale * sc1, s2 = a.glob_scale * sc2;
    float M[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        M[r * 3 + 0] = Rm[r * 3 + 0] * s0;
        M[r * 3 + 1] = Rm[r * 3 + 1] * s1;
        M[r * 3 + 2] = Rm[r * 3 + 2] * s2;
    }
    float Sg[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            Sg[r * 3 + c] = (M[r * 3] * M[c * 3] + M[r * 3 + 1] * M[c * 3 + 1]) + M[r * 3 + 2] * M[c * 3 + 2];
    o_cov[0] = Sg[0]; o_cov[1] = Sg[1]; o_cov[2] = Sg[2]; o_cov[3] = Sg[4]; o_cov[4] = Sg[5]; o_cov[5] = Sg[8];
    // symmetric V from the 6 stored entries (as gsplat rebuilds it)
    float C3[9] = {Sg[0], Sg[1], Sg[2], Sg[1], Sg[4], Sg[5], Sg[2], Sg[5], Sg[8]};
    // project_cov3d_ewa
    float tan_fovx = 0.5f * (float)a.W / cam.fx, tan_fovy = 0.5f * (float)a.H / cam.fy;
    float lim_x = 1.3f * tan_fovx, lim_y = 1.3f * tan_fovy;
    float ex = tz * fminf(lim_x, fmaxf(-lim_x, tx / tz));
    float ey = tz * fminf(lim_y, fmaxf(-lim_y, ty / tz));
    float rz = 1.f / tz, rz2 = rz * rz;
    float J00 = cam.fx * rz, J02 = (-cam.fx * ex) * rz2, J11 = cam.fy * rz, J12 = (-cam.fy * ey) * rz2;
    float T0[3], T1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        T0[c] = J00 * V[0 * 4 + c] + J02 * V[2 * 4 + c];
        T1[c] = J11 * V[1 * 4 + c] + J12 * V[2 * 4 + c];
    }
    float TV0[3], TV1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        TV0[c] = (T0[0] * C3[0 * 3 + c] + T0[1] * C3[1 * 3 + c]) + T0[2] * C3[2 * 3 + c];
        TV1[c] = (T1[0] * C3[0 * 3 + c] + T1[1] * C3[1 * 3 + c]) + T1[2] * C3[2 * 3 + c];
    }
    float c00 = (TV0[0] * T0[0] + TV0[1] * T0[1]) + TV0[2] * T0[2];
    float c01 = (TV0[0] * T1[0] + TV0[1] * T1[1]) + TV0[2] * T1[2];
    float c11 = (TV1[0] * T1[0] + TV1[1] * T1[1]) + TV1[2] * T1[2];
    float det_orig = c00 * c11 - c01 * c01;
    float ca = c00 + 0.3f, cb = c01, cc = c11 + 0.3f;
    float det = ca * cc - cb * cb;
    float comp = sqrtf(fmaxf(0.f, det_orig / det));
    // compute_cov2d_bounds
    if (det == 0.f) return;
    float inv_det = 1.f / det;
    o_conic[0] = cc * inv_det;
    o_conic[1] = -cb * inv_det;
    o_conic[2] = ca * inv_det;
    float bh = 0.5f * (ca + cc);
    float sq = sqrtf(fmaxf(0.1f, bh * bh - det));
    float v1 = bh + sq, v2 = bh - sq;
    float radius = ceilf(3.f * sqrtf(fmaxf(v1, v2)));
    // project_pix
    float rw = 1.f / (tz + 1e-6f);
    float u = (tx * rw) * cam.fx + cam.cx, vv = (ty * rw) * cam.fy + cam.cy;
    int tbx = (a.W + a.bw - 1) / a.bw, tby = (a.H + a.bw - 1) / a.bw;
    int x0, y0, x1, y1;
    tile_bbox(u, vv, radius, a.bw, tbx, tby, x0, y0, x1, y1);
    int area = (x1 - x0) * (y1 - y0);
    if (area <= 0) return;
    if (a.opl) {
        if (a.antialiased) {
            opac = opac * comp;
            o_opac = opac;
        }
        area = tight_count(tight_splat(u, vv, opac, cc * inv_det, -cb * inv_det, ca * inv_det), a.bw, x0, y0, x1, y1);
    }
    o_tiles = area;
    o_depth = tz;
    o_radius = (int)radius;
    o_xy[0] = u;
    o_xy[1] = vv;
    o_comp = comp;
    };
    per_splat();
    a.radii[o] = o_radius;
    a.tiles[o] = o_tiles;
    a.xys[o * 2] = o_xy[0];
    a.xys[o * 2 + 1] = o_xy[1];
    a.depths[o] = o_depth;
    a.comp[o] = o_comp;
#pragma unroll
    for (int c = 0; c < 3; ++c) a.conics[o * 3 + c] = o_conic[c];
    if (a.cov3d) {   // uniform (unerf_splat_project_batch: may be NULL)
#pragma unroll
        for (int c = 0; c < 6; ++c) a.cov3d[o * 6 + c] = o_cov[c];
    }
    if (a.opl) a.opac_out[o] = o_opac;
    }
}

static int splat_project_impl(bool raw, const float* opacity_logits, int antialiased, float* opacities_out,
                              const float* means3d, const float* scales, float glob_scale, const float* quats,
                              const float* viewmat, float fx, float fy, float cx, float cy, int H, int W,
                              int block_width, float clip_thresh, int64_t N, float* xys, float* depths,
                              int32_t* radii, float* conics, float* compensation, int32_t* num_tiles_hit,
                              float* cov3d, void* stream) {
    UNERF_REQUIRE(viewmat && (N == 0 || (means3d && scales && quats && xys && depths && radii && conics && compensation &&
                                       num_tiles_hit && cov3d)),
                  "splat_project: null pointer");
    UNERF_REQUIRE(H > 0 && W > 0 && block_width > 0 && block_width <= 16 && N >= 0, "splat_project: bad H/W/block/N");
    if (N == 0) return UNERF_OK;
    ProjArgs<1> a;
    a.means = means3d; a.scales = scales; a.glob_scale = glob_scale; a.quats = quats;
    a.nv = 1;
    for (int k = 0; k < 12; ++k) a.cam[0].V[k] = viewmat[k];
    a.cam[0].fx = fx; a.cam[0].fy = fy; a.cam[0].cx = cx; a.cam[0].cy = cy;
    a.H = H; a.W = W; a.bw = block_width; a.clip = clip_thresh; a.N = N;
    a.xys = xys; a.depths = depths; a.radii = radii; a.conics = conics; a.comp = compensation;
    a.tiles = num_tiles_hit; a.cov3d = cov3d;
    a.opl = opacity_logits; a.opac_out = opacities_out; a.antialiased = antialiased;
    if (raw) hipLaunchKernelGGL(project_kernel<true>, dim3(blocks_for(N, 256)), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(project_kernel<false>, dim3(blocks_for(N, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return unerf_check_launch("splat_project");
}

extern "C" int unerf_splat_project(const float* means3d, const float* scales, float glob_scale, const float* quats,
                                   const float* viewmat, float fx, float fy, float cx, float cy, int H, int W,
                                   int block_width, float clip_thresh, int64_t N, float* xys, float* depths,
                                   int32_t* radii, float* conics, float* compensation, int32_t* num_tiles_hit,
                                   float* cov3d, void* stream) {
    return splat_project_impl(false, nullptr, 0, nullptr, means3d, scales, glob_scale, quats, viewmat, fx, fy, cx, cy, H, W, block_width,
                              clip_thresh, N, xys, depths, radii, conics, compensation, num_tiles_hit, cov3d, stream);
}

extern "C" int unerf_splat_project_raw(const float* means3d, const float* log_scales, float glob_scale,
                                       const float* raw_quats, const float* viewmat, float fx, float fy, float cx,
                                       float cy, int H, int W, int block_width, float clip_thresh, int64_t N,
                                       const float* opacity_logits, int antialiased, float* opacities_out, float* xys,
                                       float* depths, int32_t* radii, float* conics, float* compensation,
                                       int32_t* num_tiles_hit, float* cov3d, void* stream) {
    UNERF_REQUIRE(!opacity_logits || opacities_out || N <= 0, "splat_project_raw: opacity_logits without opacities_out");
    return splat_project_impl(true, opacity_logits, antialiased, opacities_out, means3d, log_scales, glob_scale, raw_quats, viewmat, fx, fy, cx, cy, H, W, block_width,
                              clip_thresh, N, xys, depths, radii, conics, compensation, num_tiles_hit, cov3d, stream);
}

// view records (unerf.h: UNERF_SPLAT_VIEW_FLOATS floats per view) -> the launch's cameras
static void proj_cams(ProjArgs<UNERF_SPLAT_MAX_VIEWS>& a, const float* views, int B) {
    a.nv = B;
    for (int v = 0; v < B; ++v) {
        const float* r = views + (size_t)v * UNERF_SPLAT_VIEW_FLOATS;
        for (int k = 0; k < 12; ++k) a.cam[v].V[k] = r[k];
        a.cam[v].fx = r[12]; a.cam[v].fy = r[13]; a.cam[v].cx = r[14]; a.cam[v].cy = r[15];
    }
}

extern "C" int unerf_splat_project_batch(const float* means3d, const float* log_scales, float glob_scale, const float* raw_quats,
                                         const float* views_host, int B, int H, int W, int block_width, float clip_thresh,
                                         int64_t N, const float* opacity_logits, int antialiased, float* opacities_out,
                                         float* xys, float* depths, int32_t* radii, float* conics, float* compensation,
                                         int32_t* num_tiles_hit, float* cov3d, void* stream) {
    UNERF_REQUIRE(views_host, "splat_project_batch: null pointer (views_host)");
    UNERF_REQUIRE(B >= 1 && B <= UNERF_SPLAT_MAX_VIEWS, "splat_project_batch: B=%d outside [1,%d]", B, UNERF_SPLAT_MAX_VIEWS);
    UNERF_REQUIRE(N >= 0 && (int64_t)B * N < UNERF_SPLAT_MAX_BATCH_SPLATS, "splat_project_batch: B*N = %lld outside [0,2^29)",
                  (long long)B * (long long)N);
    UNERF_REQUIRE(N == 0 || (means3d && log_scales && raw_quats && xys && depths && radii && conics && compensation &&
                             num_tiles_hit),
                  "splat_project_batch: null pointer");
    UNERF_REQUIRE(!opacity_logits || opacities_out || N == 0, "splat_project_batch: opacity_logits without opacities_out");
    UNERF_REQUIRE(H > 0 && W > 0 && block_width > 0 && block_width <= 16, "splat_project_batch: bad H/W/block");
    if (N == 0) return UNERF_OK;
    ProjArgs<UNERF_SPLAT_MAX_VIEWS> a;
    a.means = means3d; a.scales = log_scales; a.glob_scale = glob_scale; a.quats = raw_quats;
    proj_cams(a, views_host, B);
    a.H = H; a.W = W; a.bw = block_width; a.clip = clip_thresh; a.N = N;
    a.xys = xys; a.depths = depths; a.radii = radii; a.conics = conics; a.comp = compensation;
    a.tiles = num_tiles_hit; a.cov3d = cov3d;
    a.opl = opacity_logits; a.opac_out = opacities_out; a.antialiased = antialiased;
    hipLaunchKernelGGL((project_kernel<true, true>), dim3(blocks_for(N, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return unerf_check_launch("splat_project_batch");
}

// ======================================================================================
// SH colours (+0.5, clamp>=0) and beta = softplus(log_unc) + beta_min
// ======================================================================================
// SPLIT: the coefficients arrive as the model stores them -- features_dc [N,3] and features_rest [N,15,3]
// (`coeffs` = dc, `rest` = the 45-float rows) -- which saves the per-frame torch.cat of 192 B per splat that the
// reference performs (activesplatfacto_model.py:242-243) and this kernel would only read back once.
// PACK (unerf_splat_shade_inputs): everything the rasteriser reads per splat leaves this kernel in its final layout --
// one interleaved row [rgb, (beta), depth] per splat and the activated opacity -- instead of through the reference's
// torch.cat / torch.sigmoid launches (activesplatfacto_model.py:256, 286-305).
struct ShadePack {
    const float* opacity_logits;   // [N]
    const float* compensation;     // [N] or NULL (rasterize_mode == "antialiased": opacities * comp, :252-254)
    const float* depths;           // [N]
    float* opacities;              // [N] out
    int C;                         // row length: 4 = rgb + depth, 5 = rgb + beta + depth
};
// the camera positions of the launch's views: 1, or up to UNERF_SPLAT_MAX_VIEWS (unerf_splat_shade_inputs_batch, PACK only:
// view v's rows, opacities, compensations and depths start at v N)
template <int NV>
struct ShadeCams {
    int nv;
    float pos[NV][3];
};
template <int NV>
static ShadeCams<NV> shade_cams(const float* p, int nv, int stride) {
    ShadeCams<NV> c;
    c.nv = nv;
    for (int v = 0; v < nv; ++v)
        for (int k = 0; k < 3; ++k) c.pos[v][k] = p[(size_t)v * stride + k];
    return c;
}

// STAGE (SPLIT rows, degree 3, 16-byte aligned features_rest): the workgroup's 256 rows of 180 B are one contiguous 46-KB
// block -- it is read with coalesced 16-byte loads into LDS and every thread takes its 45 floats from there (stride 45
// words: conflict-free), instead of 12 loads per thread that touch 64 cache lines each (87 us for 208 MB: 2.4 TB/s).
// MULTI (unerf_splat_shade_inputs_batch): the view loop runs over cams.nv views; without it over view 0 only -- the same
// instruction stream and registers as before the loop existed (the loop kept live across views costs the single-view
// kernel 11 VGPRs and two waves per SIMD).
// (waves per SIMD: the single-view kernels' as they were before the view loop existed)
template <bool SPLIT, bool PACK, bool STAGE = false, bool MULTI = false>
__global__ __launch_bounds__(256, MULTI ? 1 : STAGE ? 3 : (SPLIT && !PACK) ? 6 : 7) void sh_colors_kernel(int degree, const float* __restrict__ means,
                                                        ShadeCams<MULTI ? UNERF_SPLAT_MAX_VIEWS : 1> cams,
                                                        const float* __restrict__ coeffs,
                                                        const float* __restrict__ rest,
                                                        const float* __restrict__ log_unc, float beta_min, int64_t N,
                                                        float* __restrict__ colors, float* __restrict__ beta,
                                                        ShadePack pk) {
    __shared__ float s_rest[STAGE ? 256 * 45 : 1];
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (STAGE) {
        const int64_t b0 = (int64_t)blockIdx.x * 256;
        const int nb = (int)((N - b0 < 256) ? N - b0 : 256);
        const float4* src = reinterpret_cast<const float4*>(rest + b0 * 45);     // (b0 * 180 B is a multiple of 16)
        const int nq4 = nb * 45 / 4;
#pragma unroll 4
        for (int q = threadIdx.x; q < nq4; q += 256) reinterpret_cast<float4*>(s_rest)[q] = src[q];
        for (int r = nq4 * 4 + (int)threadIdx.x; r < nb * 45; r += 256) s_rest[r] = rest[b0 * 45 + r];
        __syncthreads();
    }
    if (i >= N) return;
    const float C0 = 0.28209479177387814f, C1 = 0.4886025119029199f;
    const float C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f,
                         0.5462742152960396f};
    const float C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f,
                         -0.4570457994644658f, 1.445305721320277f, -0.5900435899266435f};
    // the splat's coefficient row (192 B, 16-byte aligned) as 16-byte loads: a thread-per-splat kernel reads with a
    // 192-B stride, so every load instruction touches 64 cache lines -- 12 of them instead of 46 dword loads
    float k[48];
    if (SPLIT && STAGE) {
        const float* dc = coeffs + i * 3;
        k[0] = dc[0]; k[1] = dc[1]; k[2] = dc[2];
#pragma unroll
        for (int j = 0; j < 45; ++j) k[3 + j] = s_rest[threadIdx.x * 45 + j];
    } else if (SPLIT) {
        const float* dc = coeffs + i * 3;
        k[0] = dc[0]; k[1] = dc[1]; k[2] = dc[2];
        // 180-byte rows are only 4-byte aligned: 11 x 16-byte + 1 x 4-byte unaligned-capable global loads
        struct __attribute__((packed, aligned(4))) Q { float x, y, z, w; };
        const Q* r4 = reinterpret_cast<const Q*>(rest + i * 45);
        const int nq = degree <= 0 ? 0 : degree == 1 ? 3 : degree == 2 ? 6 : 11;       // 9 / 24 / 45 floats used
#pragma unroll
        for (int q = 0; q < 11; ++q) {
            Q v = {0.f, 0.f, 0.f, 0.f};
            if (q < nq) v = r4[q];
            k[3 + 4 * q] = v.x; k[4 + 4 * q] = v.y; k[5 + 4 * q] = v.z; k[6 + 4 * q] = v.w;
        }
        k[47] = (degree >= 3) ? rest[i * 45 + 44] : 0.f;
    } else {
        const float4* k4 = reinterpret_cast<const float4*>(coeffs + i * 48);
        const int nq = degree <= 0 ? 1 : degree == 1 ? 3 : degree == 2 ? 7 : 12;   // 3 / 12 / 27 / 48 floats used
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            const float4 v = (q < nq) ? k4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            k[4 * q] = v.x; k[4 * q + 1] = v.y; k[4 * q + 2] = v.z; k[4 * q + 3] = v.w;
        }
    }
    // Every per-splat input is read once; each view of the launch gets its own view directions, colours and rows.  MULTI
    // loads the mean, log-uncertainty and opacity logit here, in front of the view loop; one view keeps the single-view
    // kernel's loads where they always were (its registers and occupancy are unchanged).
    float mp[3] = {0.f, 0.f, 0.f}, lu = 0.f, ol = 0.f;
    if (MULTI) {
        if (degree >= 1) { mp[0] = means[i * 3]; mp[1] = means[i * 3 + 1]; mp[2] = means[i * 3 + 2]; }
        if (PACK && pk.C == 5) lu = log_unc[i];
        if (PACK && pk.opacity_logits) ol = pk.opacity_logits[i];
    }
    const int nv = MULTI ? cams.nv : 1;
    for (int vw = 0; vw < nv; ++vw) {
    const float cxp = cams.pos[vw][0], cyp = cams.pos[vw][1], czp = cams.pos[vw][2];
    const int64_t iv = (int64_t)vw * N + i;
    float col[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) col[c] = C0 * k[c];
    if (degree >= 1) {
        float vx = (MULTI ? mp[0] : means[i * 3]) - cxp, vy = (MULTI ? mp[1] : means[i * 3 + 1]) - cyp,
              vz = (MULTI ? mp[2] : means[i * 3 + 2]) - czp;
        float nrm = sqrtf((vx * vx + vy * vy) + vz * vz);
        float x = vx / nrm, y = vy / nrm, z = vz / nrm;
        float xx = x * x, xy = x * y, xz = x * z, yy = y * y, yz = y * z, zz = z * z;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            col[c] += C1 * (-y * k[1 * 3 + c] + z * k[2 * 3 + c] - x * k[3 * 3 + c]);
            if (degree >= 2) {
                col[c] += (C2[0] * xy * k[4 * 3 + c] + C2[1] * yz * k[5 * 3 + c] +
                           C2[2] * (2.f * zz - xx - yy) * k[6 * 3 + c] + C2[3] * xz * k[7 * 3 + c] +
                           C2[4] * (xx - yy) * k[8 * 3 + c]);
            }
            if (degree >= 3) {
                col[c] += (C3[0] * y * (3.f * xx - yy) * k[9 * 3 + c] + C3[1] * xy * z * k[10 * 3 + c] +
                           C3[2] * y * (4.f * zz - xx - yy) * k[11 * 3 + c] +
                           C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy) * k[12 * 3 + c] +
                           C3[4] * x * (4.f * zz - xx - yy) * k[13 * 3 + c] + C3[5] * z * (xx - yy) * k[14 * 3 + c] +
                           C3[6] * x * (xx - 3.f * yy) * k[15 * 3 + c]);
            }
        }
    }
    const int64_t row = PACK ? iv * pk.C : i * 3;
    if (degree < 0) {  // config.sh_degree == 0: rgbs = sigmoid(features_dc) (activesplatfacto_model.py:247-248)
#pragma unroll
        for (int c = 0; c < 3; ++c) colors[row + c] = unerf_sigmoid(k[c]);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) colors[row + c] = fmaxf(col[c] + 0.5f, 0.f);
    }
    if (PACK) {
        if (pk.C == 5) colors[row + 3] = unerf_softplus(MULTI ? lu : log_unc[i]) + beta_min;
        colors[row + pk.C - 1] = pk.depths[iv];
        if (pk.opacity_logits) {   // uniform
            const float o = unerf_sigmoid(MULTI ? ol : pk.opacity_logits[i]);
            pk.opacities[iv] = pk.compensation ? o * pk.compensation[iv] : o;
        }
    } else if (beta) {
        beta[i] = unerf_softplus(log_unc[i]) + beta_min;
    }
    }
}

extern "C" int unerf_splat_sh_colors(int degree, const float* means3d, const float* cam_pos, const float* sh_coeffs,
                                     const float* log_unc, float beta_min, int64_t N, float* colors_out,
                                     float* beta_out, void* stream) {
    UNERF_REQUIRE(cam_pos && (N <= 0 || (means3d && sh_coeffs && colors_out)), "splat_sh_colors: null pointer");
    UNERF_REQUIRE(degree >= -1 && degree <= 3, "splat_sh_colors: degree %d outside [-1,3]", degree);
    UNERF_REQUIRE(!beta_out || log_unc || N <= 0, "splat_sh_colors: beta_out without log_unc");
    UNERF_REQUIRE(((uintptr_t)sh_coeffs & 15u) == 0, "splat_sh_colors: sh_coeffs must be 16-byte aligned");
    if (N <= 0) return UNERF_OK;
    hipLaunchKernelGGL((sh_colors_kernel<false, false>), dim3(blocks_for(N, 256)), dim3(256), 0, (hipStream_t)stream,
                       degree, means3d, shade_cams<1>(cam_pos, 1, 3), sh_coeffs, nullptr, log_unc, beta_min, N,
                       colors_out, beta_out, ShadePack{});
    return unerf_check_launch("splat_sh_colors");
}

extern "C" int unerf_splat_sh_colors_split(int degree, const float* means3d, const float* cam_pos, const float* features_dc,
                                           const float* features_rest, const float* log_unc, float beta_min, int64_t N,
                                           float* colors_out, float* beta_out, void* stream) {
    UNERF_REQUIRE(cam_pos && (N <= 0 || (means3d && features_dc && colors_out)), "splat_sh_colors_split: null pointer");
    UNERF_REQUIRE(degree >= -1 && degree <= 3, "splat_sh_colors_split: degree %d outside [-1,3]", degree);
    UNERF_REQUIRE(degree <= 0 || N <= 0 || features_rest, "splat_sh_colors_split: degree %d needs features_rest", degree);
    UNERF_REQUIRE(!beta_out || log_unc || N <= 0, "splat_sh_colors_split: beta_out without log_unc");
    if (N <= 0) return UNERF_OK;
    hipLaunchKernelGGL((sh_colors_kernel<true, false>), dim3(blocks_for(N, 256)), dim3(256), 0, (hipStream_t)stream,
                       degree, means3d, shade_cams<1>(cam_pos, 1, 3), features_dc, features_rest, log_unc, beta_min,
                       N, colors_out, beta_out, ShadePack{});
    return unerf_check_launch("splat_sh_colors_split");
}

extern "C" int unerf_splat_shade_inputs(int degree, const float* means3d, const float* cam_pos, const float* features_dc,
                                        const float* features_rest, const float* log_unc, float beta_min,
                                        const float* opacity_logits, const float* compensation, const float* depths,
                                        int64_t N, int C, float* rows_out, float* opacities_out, void* stream) {
    UNERF_REQUIRE(cam_pos && (N <= 0 || (means3d && features_dc && depths && rows_out)), "splat_shade_inputs: null pointer");
    UNERF_REQUIRE(!opacity_logits || opacities_out || N <= 0, "splat_shade_inputs: opacity_logits without opacities_out");
    UNERF_REQUIRE(degree >= -1 && degree <= 3, "splat_shade_inputs: degree %d outside [-1,3]", degree);
    UNERF_REQUIRE(degree <= 0 || N <= 0 || features_rest, "splat_shade_inputs: degree %d needs features_rest", degree);
    UNERF_REQUIRE(C == 4 || C == 5, "splat_shade_inputs: C=%d, rows are [rgb, depth] (4) or [rgb, beta, depth] (5)", C);
    UNERF_REQUIRE(C == 4 || log_unc || N <= 0, "splat_shade_inputs: C=5 needs log_unc");
    if (N <= 0) return UNERF_OK;
    ShadePack pk;
    pk.opacity_logits = opacity_logits; pk.compensation = compensation; pk.depths = depths; pk.opacities = opacities_out;
    pk.C = C;
    if (degree >= 3 && ((uintptr_t)features_rest & 15u) == 0) {      // rows staged through LDS (see sh_colors_kernel)
        hipLaunchKernelGGL((sh_colors_kernel<true, true, true>), dim3(blocks_for(N, 256)), dim3(256), 0, (hipStream_t)stream, degree,
                           means3d, shade_cams<1>(cam_pos, 1, 3), features_dc, features_rest, log_unc, beta_min, N,
                           rows_out, nullptr, pk);
    } else {
        hipLaunchKernelGGL((sh_colors_kernel<true, true>), dim3(blocks_for(N, 256)), dim3(256), 0, (hipStream_t)stream, degree,
                           means3d, shade_cams<1>(cam_pos, 1, 3), features_dc, features_rest, log_unc, beta_min, N,
                           rows_out, nullptr, pk);
    }
    return unerf_check_launch("splat_shade_inputs");
}

extern "C" int unerf_splat_shade_inputs_batch(int degree, const float* means3d, const float* views_host, int B,
                                              const float* features_dc, const float* features_rest, const float* log_unc,
                                              float beta_min, const float* opacity_logits, const float* compensation,
                                              const float* depths, int64_t N, int C, float* rows_out, float* opacities_out,
                                              void* stream) {
    UNERF_REQUIRE(views_host, "splat_shade_inputs_batch: null pointer (views_host)");
    UNERF_REQUIRE(B >= 1 && B <= UNERF_SPLAT_MAX_VIEWS, "splat_shade_inputs_batch: B=%d outside [1,%d]", B, UNERF_SPLAT_MAX_VIEWS);
    UNERF_REQUIRE(N >= 0 && (int64_t)B * N < UNERF_SPLAT_MAX_BATCH_SPLATS, "splat_shade_inputs_batch: B*N = %lld outside [0,2^29)",
                  (long long)B * (long long)N);
    UNERF_REQUIRE(N == 0 || (means3d && features_dc && depths && rows_out), "splat_shade_inputs_batch: null pointer");
    UNERF_REQUIRE(!opacity_logits || opacities_out || N == 0, "splat_shade_inputs_batch: opacity_logits without opacities_out");
    UNERF_REQUIRE(degree >= -1 && degree <= 3, "splat_shade_inputs_batch: degree %d outside [-1,3]", degree);
    UNERF_REQUIRE(degree <= 0 || N == 0 || features_rest, "splat_shade_inputs_batch: degree %d needs features_rest", degree);
    UNERF_REQUIRE(C == 4 || C == 5, "splat_shade_inputs_batch: C=%d, rows are [rgb, depth] (4) or [rgb, beta, depth] (5)", C);
    UNERF_REQUIRE(C == 4 || log_unc || N == 0, "splat_shade_inputs_batch: C=5 needs log_unc");
    if (N == 0) return UNERF_OK;
    ShadePack pk;
    pk.opacity_logits = opacity_logits; pk.compensation = compensation; pk.depths = depths; pk.opacities = opacities_out;
    pk.C = C;
    const ShadeCams<UNERF_SPLAT_MAX_VIEWS> cams = shade_cams<UNERF_SPLAT_MAX_VIEWS>(views_host + 16, B, UNERF_SPLAT_VIEW_FLOATS);
    if (degree >= 3 && ((uintptr_t)features_rest & 15u) == 0) {
        hipLaunchKernelGGL((sh_colors_kernel<true, true, true, true>), dim3(blocks_for(N, 256)), dim3(256), 0, (hipStream_t)stream, degree,
                           means3d, cams, features_dc, features_rest, log_unc, beta_min, N, rows_out, nullptr, pk);
    } else {
        hipLaunchKernelGGL((sh_colors_kernel<true, true, false, true>), dim3(blocks_for(N, 256)), dim3(256), 0, (hipStream_t)stream, degree,
                           means3d, cams, features_dc, features_rest, log_unc, beta_min, N, rows_out, nullptr, pk);
    }
    return unerf_check_launch("splat_shade_inputs_batch");
}

// ======================================================================================
// bin and sort (once per frame)
// ======================================================================================
static inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }
#define SCAN_BLOCK 1024    // own_inclusive_scan: elements per workgroup
#define SCAN_DIRECT_BLOCKS 4096   // up to this many blocks (4 M elements) every block re-sums the earlier blocks' sums itself
#define TS_SEG 32          // one-pass tile sort (below): the prefix over chunks runs in 32 independent row segments
#define TS_MAX_T1 (UNERF_SPLAT_BATCH_MAX_TILES + 1)    // 12,000 = tiles + 1 sentinel: the whole-key counters + 16 waves' digit counters must fit 64 KB of LDS (beyond: rocprim)
struct TileSortPlan {
    int chunk, nblk, rows, T1;
};
static TileSortPlan tile_sort_plan(int64_t I, int tiles) {
    TileSortPlan p;
    p.T1 = tiles + 1;
    // one single-wave workgroup per chunk, four of them per CU (their 32-KB tables): ~1024 chunks fill the chip
    int64_t chunk = (I + 1023) / 1024;
    chunk = ((chunk + 255) / 256) * 256;
    if (chunk < 2048) chunk = 2048;
    p.chunk = (int)chunk;
    p.nblk = (int)((I + chunk - 1) / chunk);
    if (p.nblk < 1) p.nblk = 1;
    p.rows = ((p.nblk + TS_SEG - 1) / TS_SEG) * TS_SEG;
    return p;
}

// ---- staged LSD radix passes (rs_* kernels below): the plan ---------------------------------------------------------------
// One pass = per-chunk digit histogram -> prefix over chunks (per digit) -> scatter; a chunk is the M pairs ONE wave ranks,
// stages in LDS in digit order and writes out as runs of consecutive slots (see rs_scatter_kernel for why).
#define RS_M_TILE 2048      // pairs per wave, tile sort (u16 / u32 keys, <= 128 digits: runs of >= 16 slots per digit)
#define RS_M_DEPTH 1024     // pairs per wave, depth sort (u32 keys, 256 digits: runs of 4)
#define RS_CPW 1            // chunks per wave in the histogram kernels (rs_pass); the whole-key histogram's workgroup = 16 waves = 16 chunks
struct RsTilePlan {
    int nchunk, b0, B0, B1, nhw;      // digit 0 = key & (B0 - 1), digit 1 = key >> b0 (< B1; B0, B1 powers of two <= 128)
};
static RsTilePlan rs_tile_plan(int64_t I, int T1) {
    RsTilePlan p;
    int bits = 1;
    while ((1 << bits) < T1) ++bits;         // keys 0 .. T1 - 1 (the sentinel tile is T1 - 1)
    p.b0 = bits <= 7 ? 0 : bits / 2;         // <= 128 keys: one pass on the whole key
    p.B0 = 1 << p.b0;
    p.B1 = 1 << (bits - p.b0);
    p.nchunk = (int)((I + RS_M_TILE - 1) / RS_M_TILE);
    if (p.nchunk < 1) p.nchunk = 1;
    p.nhw = (p.nchunk + 15) / 16;
    return p;
}

// Segments of a staged pass: segment g holds the chunks [cb[g], cb[g + 1]) and the pairs [pb[g], pb[g + 1]) of the stream, and
// is sorted on its own (its digit prefixes, totals and output slots stay inside it).  One segment: a single view; a batch of
// views: one segment per view, so every view's pairs leave in the order a single-view sort gives them.
// S: segments the launch can carry -- 1 for the single-view sort (kernel arguments of the old size), UNERF_SPLAT_MAX_VIEWS for
// unerf_splat_bin_sort_batch.  The host code (rs_pass, staged_depth_sort, staged_tile_sort, bin_sort_body) is written once over
// SEG = "more than one segment can come": it takes its chunk count, pair count and segment count from the RsSegs it is given,
// and the two entry points differ in how they build theirs.
template <int S>
struct RsSegs {
    int n;
    int cb[S + 1];
    int64_t pb[S + 1];
};
static RsSegs<1> rs_one_seg(int nchunk, int64_t n) {
    RsSegs<1> s;
    s.n = 1; s.cb[0] = 0; s.cb[1] = nchunk; s.pb[0] = 0; s.pb[1] = n;
    return s;
}
// the segment of chunk c (uniform) and the chunk's pairs [k0, k1).  SEG = false (one segment, chunks from pair 0): the
// single-view kernels' own arithmetic, nothing looked up
template <bool SEG, int S>
__device__ __forceinline__ int rs_seg_of(const RsSegs<S>& s, int c) {
    int g = 0;
    if (SEG)
        while (g + 1 < s.n && c >= s.cb[g + 1]) ++g;
    return g;
}
template <bool SEG, int S>
__device__ __forceinline__ void rs_chunk_range(const RsSegs<S>& s, int g, int c, int chunk, int64_t& k0, int64_t& k1) {
    if (!SEG) {
        k0 = (int64_t)c * chunk;
        k1 = (k0 + chunk < s.pb[1]) ? k0 + chunk : s.pb[1];
        return;
    }
    const int64_t e = s.pb[g + 1];
    k0 = s.pb[g] + (int64_t)(c - s.cb[g]) * chunk;
    if (k0 > e) k0 = e;
    k1 = (k0 + chunk < e) ? k0 + chunk : e;
}

static int tile_bits(int H, int W, int bw) {   // bits of the largest key: tiles - 1, and `tiles` itself (the sentinel)
    int64_t tiles = (int64_t)((W + bw - 1) / bw) * ((H + bw - 1) / bw);
    int b = 1;
    while (((int64_t)1 << b) <= tiles) ++b;
    return b;
}

// Workspace of unerf_splat_count_intersects / unerf_splat_bin_sort.  bin_sort orders the N splats by depth
// first (32-bit keys, small), emits the intersections in that order and then needs only a STABLE sort by
// tile id (13 bits at 1080p, 16-bit keys): two 6-byte-per-entry radix passes over the I intersections
// instead of six 12-byte passes over 64-bit (tile | depth) keys.  Same final order, bit for bit: ties in
// depth keep the splat-index order in both schemes.
// (rocprim's default dispatch for the depth sort -- kept behind UNERF_SPLAT_DEPTH_SORT=rocprim -- is a merge sort up to 2^20
// items, where a 1 M-splat scene sits; forcing its Onesweep there was 137 us against 162 for the sort alone
// (benchmarks/exp_depth_sort.hip), net zero inside the frame.  The default is the four staged LSD passes of rs_scatter_kernel;
// making the keys inside the first pass instead of in depth_keys_kernel was measured too: +8 us, its histogram loses the
// 16-byte key loads.)
static hipError_t depth_sort_pairs(void* tmp, size_t& tmp_bytes, const uint32_t* kin, uint32_t* kout, const int32_t* vin,
                                   int32_t* vout, int64_t n, hipStream_t st) {
    return hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, kin, kout, vin, vout, (int)n, 0, 32, st);
}

struct SortWs {
    int64_t tmp, dkey_in, dkey_out, id_in, order, counts, cum, tkey_in, tkey_out, val_in, val_mid, ts_table, ts_segsum, ts_start, ds_table, ds_total, total;
};
// One layout serves both entry points, and bin_sort_body reads it the same way for both (sort_ws_ptrs; the tables of the tile
// passes are carved out of ts_table / ts_segsum by staged_tile_sort from the chunk and segment counts of its RsSegs).
// batch (unerf_splat_*_batch, any B >= 1): N splats in each of B views, I pairs over all views.  Each view's chunks of the tile
// passes are padded to a multiple of 16 (a whole-key histogram workgroup never straddles two views): at most 16 B chunks more
// than the single-view plan, and as many whole-key rows more (rs_tile_tables_fit checks a batch's actual plan against this).
static SortWs sort_ws_layout(int64_t N, int64_t I, int B = 1, bool batch = false) {
    const int64_t NB = N * B;
    size_t scan_tmp = 0, sortN_tmp = 0, sortI_tmp = 0;
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, scan_tmp, (const int32_t*)nullptr, (int32_t*)nullptr, (int)NB);
    (void)depth_sort_pairs(nullptr, sortN_tmp, nullptr, nullptr, nullptr, nullptr, NB, 0);
    if (I > 0)
        (void)hipcub::DeviceRadixSort::SortPairs(nullptr, sortI_tmp, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                 (const int32_t*)nullptr, (int32_t*)nullptr, (int)I, 0, 32);
    (void)hipGetLastError();
    size_t tmp = scan_tmp > sortN_tmp ? scan_tmp : sortN_tmp;
    tmp = tmp > sortI_tmp ? tmp : sortI_tmp;
    const size_t own_scan = (size_t)((NB + SCAN_BLOCK - 1) / SCAN_BLOCK + 1) * 4;      // own_inclusive_scan's block sums
    tmp = tmp > own_scan ? tmp : own_scan;
    SortWs w;
    int64_t off = 0;
    auto take = [&](int64_t bytes) { int64_t o = off; off += align256(bytes); return o; };
    w.tmp = take((int64_t)tmp);
    w.dkey_in = take(NB * 4); w.dkey_out = take(NB * 4); w.id_in = take(NB * 4); w.order = take(NB * 4);
    w.counts = take(NB * 4); w.cum = take(NB * 4);
    w.tkey_in = take(I * 4); w.tkey_out = take(I * 4); w.val_in = take(I * 4); w.val_mid = take(I * 4);
    // the one-pass tile sort's tables, sized for the largest tile count it serves (the image size is not known here)
    const TileSortPlan tp = tile_sort_plan(I, TS_MAX_T1 - 1);
    const RsTilePlan lp = rs_tile_plan(I, TS_MAX_T1);     // the two-pass sort's tables: 2 x [128][nchunk] + [nhw][T1]
    const int64_t nchunk = lp.nchunk + (batch ? 16 * B : 0), nhw = batch ? nchunk / 16 + B : lp.nhw;
    const int64_t onepass_bytes = (int64_t)tp.rows * TS_MAX_T1 * 4, lsd_bytes = ((int64_t)256 * nchunk + nhw * TS_MAX_T1) * 4;
    w.ts_table = take(onepass_bytes > lsd_bytes ? onepass_bytes : lsd_bytes);
    // one-pass: segsum [TS_SEG][T1]; two-pass: dtotal [2][B][256] + total [B][16][T1]
    const int64_t segsum_words = (int64_t)TS_SEG * TS_MAX_T1, lsd_words = (int64_t)512 * B + (int64_t)16 * B * TS_MAX_T1;
    w.ts_segsum = take((segsum_words > lsd_words ? segsum_words : lsd_words) * 4);
    w.ts_start = take((int64_t)(TS_MAX_T1 + 1 + (int64_t)B * (TS_MAX_T1 + 1)) * 4);     // start [B][T1 + 1] + total [T1]
    w.ds_table = take((int64_t)256 * B * ((N + RS_M_DEPTH - 1) / RS_M_DEPTH) * 4);     // the depth sort's [256][chunks] counters
    w.ds_total = take((int64_t)256 * B * 4);
    w.total = off + 1024;
    return w;
}
// the tile passes' tables of a chunk plan -- 2 x [128][nchunk] digit counters + [nchunk / 16][T1] whole-key rows -- against what
// the layout reserved for them
static bool rs_tile_tables_fit(const SortWs& L, int64_t nchunk, int T1, int64_t& need, int64_t& have) {
    need = ((int64_t)256 * nchunk + (nchunk + 15) / 16 * T1) * 4;
    have = L.ts_segsum - L.ts_table;
    return need <= have;
}

// the workspace as typed pointers (the tile keys are uint16_t up to 16 key bits, uint32_t beyond: cast where they are used)
struct SortPtrs {
    void* tmp;              // rocprim's scratch; own_inclusive_scan's block sums
    size_t tmp_bytes;
    uint32_t *dk_in, *dk_out, *ts_table, *ts_segsum, *ts_start, *ds_table, *ds_total;
    int32_t *id_in, *order, *counts, *cum_sorted, *v_in, *v_mid;
    void *tk_in, *tk_out;
};
static SortPtrs sort_ws_ptrs(void* workspace, const SortWs& L) {
    char* ws = (char*)workspace;
    auto u32 = [&](int64_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
    auto i32 = [&](int64_t off) { return reinterpret_cast<int32_t*>(ws + off); };
    SortPtrs p;
    p.tmp = ws + L.tmp; p.tmp_bytes = (size_t)(L.dkey_in - L.tmp);
    p.dk_in = u32(L.dkey_in); p.dk_out = u32(L.dkey_out); p.id_in = i32(L.id_in); p.order = i32(L.order);
    p.counts = i32(L.counts); p.cum_sorted = i32(L.cum);
    p.tk_in = ws + L.tkey_in; p.tk_out = ws + L.tkey_out; p.v_in = i32(L.val_in); p.v_mid = i32(L.val_mid);
    p.ts_table = u32(L.ts_table); p.ts_segsum = u32(L.ts_segsum); p.ts_start = u32(L.ts_start);
    p.ds_table = u32(L.ds_table); p.ds_total = u32(L.ds_total);
    return p;
}

extern "C" int64_t unerf_splat_sort_workspace_bytes(int64_t N, int64_t I) {
    if (N < 1) N = 1;
    if (I < 0) I = 0;
    return sort_ws_layout(N, I).total;
}

extern "C" int64_t unerf_splat_sort_workspace_bytes_batch(int B, int64_t N, int64_t num_intersects) {
    if (B < 1 || B > UNERF_SPLAT_MAX_VIEWS || N < 0 || num_intersects < 0 || num_intersects >= (1ll << 31) ||
        (int64_t)B * N >= UNERF_SPLAT_MAX_BATCH_SPLATS)
        return -1;
    if (N < 1) N = 1;
    return sort_ws_layout(N, num_intersects, B, true).total;
}

// ---- inclusive scan of N int32 in two launches -------------------------------------------------------------------------------
// (rocprim's look-back scan is three launches of 4 - 8 us for the 4 MB the frame scans twice: the tile counts in splat order and
// again in depth order.)  Blocks of 1,024 elements: (1) block sums; (2) every block adds up the sums of the blocks before it
// (at most N / 1024 values) and scans its own elements behind that.  Integer sums: the same numbers whatever the order.
__global__ __launch_bounds__(256) void scan_sums_kernel(const int32_t* __restrict__ in, int64_t n, int32_t* __restrict__ bsum) {
    __shared__ int32_t s_w[4];
    const int64_t e0 = (int64_t)blockIdx.x * SCAN_BLOCK + 4 * threadIdx.x;
    int32_t v = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) v += (e0 + i < n) ? in[e0 + i] : 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// Middle step for MANY blocks (own_inclusive_scan: nb > SCAN_DIRECT_BLOCKS): the block sums become their own exclusive prefix,
// in place, by one workgroup -- each thread sums a contiguous run, the 1,024 run totals are scanned through LDS, each thread
// rewrites its run.  Linear in nb: scan_apply_kernel's re-summing of every earlier block is nb^2 / 2 reads in total, fine at
// the 1 M splats of the bench frame (0.5 M reads) and 50 M reads at 10 M splats.
__global__ __launch_bounds__(1024) void scan_bsum_kernel(int32_t* __restrict__ bsum, int nb) {
    __shared__ int32_t s_run[1024];
    const int per = (nb + 1023) / 1024, b0 = threadIdx.x * per, b1 = min(b0 + per, nb);
    int32_t tot = 0;
    for (int b = b0; b < b1; ++b) tot += bsum[b];
    s_run[threadIdx.x] = tot;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int32_t v = threadIdx.x >= d ? s_run[threadIdx.x - d] : 0;
        __syncthreads();
        s_run[threadIdx.x] += v;
        __syncthreads();
    }
    int32_t run = s_run[threadIdx.x] - tot;
    for (int b = b0; b < b1; ++b) {
        const int32_t v = bsum[b];
        bsum[b] = run;
        run += v;
    }
}

// PRE: bsum holds exclusive prefixes already (scan_bsum_kernel)
template <bool PRE>
__global__ __launch_bounds__(256) void scan_apply_kernel(const int32_t* __restrict__ in, int64_t n, const int32_t* __restrict__ bsum,
                                                         int32_t* __restrict__ out) {
    __shared__ int32_t s_w[4], s_p[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int32_t before = 0;      // sum of the earlier blocks' sums
    if (PRE) {
        before = (threadIdx.x & 63) == 0 && wv == 0 ? bsum[blockIdx.x] : 0;     // one lane carries it into the sum below
    } else {
        for (int b = threadIdx.x; b < (int)blockIdx.x; b += 256) before += bsum[b];
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) before += __shfl_xor(before, m, 64);
    const int64_t e0 = (int64_t)blockIdx.x * SCAN_BLOCK + 4 * threadIdx.x;
    int32_t x[4], mine = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        x[i] = (e0 + i < n) ? in[e0 + i] : 0;
        mine += x[i];
    }
    int32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t v = __shfl_up(incl, d, 64);
        if (lane >= d) incl += v;
    }
    if (lane == 63) s_w[wv] = incl;
    if (lane == 0) s_p[wv] = before;
    __syncthreads();
    int32_t run = s_p[0] + s_p[1] + s_p[2] + s_p[3] + incl - mine;
#pragma unroll
    for (int w = 0; w < 4; ++w) run += w < wv ? s_w[w] : 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        run += x[i];
        if (e0 + i < n) out[e0 + i] = run;
    }
}

// bsum: (n + 1023) / 1024 int32 of scratch
static void own_inclusive_scan(const int32_t* in, int32_t* out, int64_t n, int32_t* bsum, hipStream_t st) {
    const unsigned nb = blocks_for(n, SCAN_BLOCK);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(nb), dim3(256), 0, st, in, n, bsum);
    if (nb > SCAN_DIRECT_BLOCKS) {
        hipLaunchKernelGGL(scan_bsum_kernel, dim3(1), dim3(1024), 0, st, bsum, (int)nb);
        hipLaunchKernelGGL(scan_apply_kernel<true>, dim3(nb), dim3(256), 0, st, in, n, bsum, out);
    } else {
        hipLaunchKernelGGL(scan_apply_kernel<false>, dim3(nb), dim3(256), 0, st, in, n, bsum, out);
    }
}
static bool use_rocprim_scan() {
    const char* env = getenv("UNERF_SPLAT_SCAN");
    return env && strcmp(env, "rocprim") == 0;
}

extern "C" int unerf_splat_count_intersects(const int32_t* num_tiles_hit, int64_t N, int32_t* cum_tiles_hit,
                                            void* workspace, int64_t workspace_bytes, void* stream) {
    UNERF_REQUIRE(num_tiles_hit && cum_tiles_hit && workspace, "splat_count_intersects: null pointer");
    UNERF_REQUIRE(N >= 1 && N < (1ll << 31), "splat_count_intersects: bad N");
    UNERF_REQUIRE(workspace_bytes >= (int64_t)blocks_for(N, SCAN_BLOCK) * 4, "splat_count_intersects: workspace %lld bytes too small",
                  (long long)workspace_bytes);
    if (!use_rocprim_scan()) {      // (UNERF_SPLAT_SCAN=rocprim: hipcub's scan, for A/B runs)
        own_inclusive_scan(num_tiles_hit, cum_tiles_hit, N, reinterpret_cast<int32_t*>(workspace), (hipStream_t)stream);
        return unerf_check_launch("splat_count_intersects");
    }
    size_t tmp = (size_t)workspace_bytes;
    hipError_t e = hipcub::DeviceScan::InclusiveSum(workspace, tmp, num_tiles_hit, cum_tiles_hit, (int)N,
                                                    (hipStream_t)stream);
    if (e != hipSuccess) {
        unerf_set_error("splat_count_intersects: %s", hipGetErrorString(e));
        return UNERF_ERR_HIP;
    }
    return unerf_check_launch("splat_count_intersects");
}

// The per-view numbers a batch's ONE host read-back carries: summary[v] = view v's intersections (the difference of the
// inclusive scan over the B N tile counts at the view's ends), summary[B + v] = 1 when some splat of view v has a radius > 0.
// That flag is known from the total when it is non-zero; otherwise (tight lists can be empty while splats are "visible"
// by radius) the view's radii are searched, by the workgroups of grid.x, each OR-ing its finding in.  summary[B ..] is
// zeroed by the caller.
__global__ __launch_bounds__(256) void count_summary_kernel(const int32_t* __restrict__ cum, const int32_t* __restrict__ radii,
                                                            int64_t N, int B, int32_t* __restrict__ summary) {
    const int v = blockIdx.y;
    const int64_t e = (int64_t)(v + 1) * N - 1;
    const uint32_t tot = (uint32_t)cum[e] - (v > 0 ? (uint32_t)cum[e - N] : 0u);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        summary[v] = (int32_t)tot;
        if (tot != 0u || !radii) summary[B + v] = tot != 0u ? 1 : 0;
    }
    if (tot != 0u || !radii) return;     // (uniform)
    const int32_t* r = radii + (int64_t)v * N;
    int found = 0;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < N; k += (int64_t)gridDim.x * 256) found |= r[k] > 0;
    if (__syncthreads_or(found) && threadIdx.x == 0) atomicOr(&summary[B + v], 1);
}

extern "C" int unerf_splat_count_intersects_batch(const int32_t* num_tiles_hit, const int32_t* radii, int B, int64_t N,
                                                  int32_t* cum_tiles_hit, int32_t* summary, void* workspace,
                                                  int64_t workspace_bytes, void* stream) {
    UNERF_REQUIRE(num_tiles_hit && cum_tiles_hit && summary && workspace, "splat_count_intersects_batch: null pointer");
    UNERF_REQUIRE(B >= 1 && B <= UNERF_SPLAT_MAX_VIEWS, "splat_count_intersects_batch: B=%d outside [1,%d]", B,
                  UNERF_SPLAT_MAX_VIEWS);
    UNERF_REQUIRE(N >= 1 && (int64_t)B * N < UNERF_SPLAT_MAX_BATCH_SPLATS, "splat_count_intersects_batch: bad N (B*N = %lld)",
                  (long long)B * (long long)N);
    UNERF_REQUIRE(workspace_bytes >= (int64_t)blocks_for((int64_t)B * N, SCAN_BLOCK) * 4,
                  "splat_count_intersects_batch: workspace %lld bytes too small", (long long)workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    own_inclusive_scan(num_tiles_hit, cum_tiles_hit, (int64_t)B * N, reinterpret_cast<int32_t*>(workspace), st);
    if (hipMemsetAsync(summary + B, 0, (size_t)B * sizeof(int32_t), st) != hipSuccess)
        return unerf_check_launch("splat_count_intersects_batch memset");
    const unsigned gx = radii ? (blocks_for(N, 256) < 64u ? blocks_for(N, 256) : 64u) : 1u;
    hipLaunchKernelGGL(count_summary_kernel, dim3(gx, B), dim3(256), 0, st, cum_tiles_hit, radii, N, B, summary);
    return unerf_check_launch("splat_count_intersects_batch");
}

// depth key of every splat (culled ones last) + identity payload
__global__ __launch_bounds__(256) void depth_keys_kernel(const float* __restrict__ depths,
                                                         const int32_t* __restrict__ radii, int64_t N,
                                                         uint32_t* __restrict__ keys, int32_t* __restrict__ ids) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    keys[i] = radii[i] > 0 ? (uint32_t)__float_as_int(depths[i]) : 0xFFFFFFFFu;
    ids[i] = (int32_t)i;
}

// tiles hit by the j-th splat in depth order (num_tiles_hit recovered from its inclusive scan)
__global__ __launch_bounds__(256) void sorted_counts_kernel(const int32_t* __restrict__ order,
                                                            const int32_t* __restrict__ radii,
                                                            const int32_t* __restrict__ cum, int64_t N,
                                                            int32_t* __restrict__ counts) {
    int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    const int32_t i = order[j];
    counts[j] = radii[i] > 0 ? cum[i] - (i == 0 ? 0 : cum[i - 1]) : 0;
}

// LPS lanes per splat (8: a tight list is ~20 tiles in ~5 rows on the 1 M-splat bench frame, and the per-splat set-up -- the
// ellipse, a row range per lane, the scan -- is the same instruction stream whether 4 or 8 splats share the wave; 16 lanes per
// splat spent 338 VALU instructions per wave on 4 splats: VALU-bound, 137 of 148 us, rocprofv3 r5).
// Lane t writes entries t, t+LPS, ... of the splat's row-major tile box, so a splat's run of
// (tile, id) pairs leaves as 32-B / 64-B segments instead of one thread trickling out 2-B and 4-B stores (an average
// splat of the 1 M-splat bench scene covers 37 tiles).  Entry index = first + (ty - y0) * w + (tx - x0): the order a
// serial row-major walk produces, which is gsplat's.
template <typename TKey, int LPS>
__global__ __launch_bounds__(256) void map_intersects_kernel(const float* __restrict__ xys,
                                                             const int32_t* __restrict__ radii,
                                                             const int32_t* __restrict__ order,
                                                             const int32_t* __restrict__ cum_sorted, int64_t N, int bw,
                                                             int tbx, int tby, const float* __restrict__ conics,
                                                             const float* __restrict__ opac, TKey* __restrict__ tkeys,
                                                             int32_t* __restrict__ vals) {
    const int l16 = threadIdx.x & (LPS - 1);
    const int64_t j = (int64_t)blockIdx.x * (256 / LPS) + threadIdx.x / LPS;
    if (j >= N) return;
    const int32_t i = order[j];
    if (radii[i] <= 0) return;
    int x0, y0, x1, y1;
    const float sx = xys[(int64_t)i * 2], sy = xys[(int64_t)i * 2 + 1];
    tile_bbox(sx, sy, (float)radii[i], bw, tbx, tby, x0, y0, x1, y1);
    const int w = x1 - x0, count = w * (y1 - y0);
    if (count <= 0) return;
    const int64_t first = (j == 0) ? 0 : cum_sorted[j - 1];
    if (conics) {   // uniform: tight lists -- the rows project_kernel counted, in the same order
        const TightSplat t = tight_splat(sx, sy, opac[i], conics[(int64_t)i * 3], conics[(int64_t)i * 3 + 1],
                                         conics[(int64_t)i * 3 + 2]);
        // The slot [first, end) was sized by project_kernel's tight_count -- a second inlining of tight_row on the same
        // stored numbers.  Should the two ever disagree (another build behind UNERF_LIB, a compiler that contracts one of
        // them), the emission stays inside its slot and pads what is left with the sentinel tile `tbx * tby`, which the
        // sort puts behind every real tile and tile_bins never covers: a wrong count costs pairs, never memory safety.
        const int64_t end = cum_sorted[j];
        const TKey sentinel = (TKey)(tbx * tby);
        // LPS tile rows at a time, one per lane of the splat's lane group; their widths are scanned inside the group and
        // the round's entries go out striped over the lanes like the box form below (a row is only ~5 tiles wide: a
        // lane-per-row or row-by-row emission leaves most lanes of every store idle -- 2.5 x the kernel time)
        const int nrows = y1 - y0;
        int64_t at = first;
        for (int rb = 0; rb < nrows; rb += LPS) {
            int a0 = 0, a1 = 0;
            if (rb + l16 < nrows) tight_row(t, y0 + rb + l16, bw, x0, x1, a0, a1);
            const int wd = a1 - a0;
            int incl = wd;
#pragma unroll
            for (int d = 1; d < LPS; d <<= 1) {
                const int v = __shfl_up(incl, d, LPS);
                if (l16 >= d) incl += v;
            }
            const int total = __shfl(incl, LPS - 1, LPS), excl = incl - wd;
            for (int e0 = 0; e0 < total; e0 += LPS) {          // (uniform inside the group: every lane takes every shuffle)
                const int e = e0 + l16;
                int r = 0;                                    // row of entry e: first lane whose inclusive sum exceeds e
#pragma unroll
                for (int step = LPS / 2; step >= 1; step >>= 1) {
                    const int probe = __shfl(incl, r + step - 1, LPS);
                    if (probe <= e) r += step;
                }
                r = min(r, LPS - 1);
                const int rex = __shfl(excl, r, LPS), ra0 = __shfl(a0, r, LPS);
                if (e < total && at + e < end) {
                    tkeys[at + e] = (TKey)((y0 + rb + r) * tbx + ra0 + (e - rex));
                    vals[at + e] = i;
                }
            }
            at += total;
        }
        for (int64_t e = at + l16; e < end; e += LPS) {        // never taken when the two counts agree
            tkeys[e] = sentinel;
            vals[e] = i;
        }
        return;
    }
    // row = floor(t / w) through the reciprocal, then made exact by one step either way (the estimate is within 1
    // for any box that fits an image)
    const float rw = 1.f / (float)w;
    for (int t = l16; t < count; t += LPS) {
        int row = (int)(((float)t + 0.5f) * rw);
        row -= (row * w > t) ? 1 : 0;
        row += ((row + 1) * w <= t) ? 1 : 0;
        const int col = t - row * w;
        tkeys[first + t] = (TKey)((y0 + row) * tbx + (x0 + col));
        vals[first + t] = i;
    }
}

// tile ranges + the gsplat-style 64-bit ids (tile << 32 | depth bits) of the sorted intersections (rocprim path; entries
// with the sentinel tile `tiles` sort behind every real tile and belong to no range)
template <typename TKey>
__global__ __launch_bounds__(256) void tile_edges_kernel(const TKey* __restrict__ tkeys,
                                                         const int32_t* __restrict__ gids,
                                                         const float* __restrict__ depths, int64_t I, int32_t tiles,
                                                         int32_t* __restrict__ bins, int64_t* __restrict__ isect_ids) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= I) return;
    const int32_t cur = (int32_t)tkeys[i];
    if (isect_ids) isect_ids[i] = ((int64_t)cur << 32) | (int64_t)(uint32_t)__float_as_int(depths[gids[i]]);
    const int32_t prev = i > 0 ? (int32_t)tkeys[i - 1] : -1;
    if (cur >= tiles) {
        if (prev >= 0 && prev < tiles) bins[prev * 2 + 1] = (int32_t)i;
        return;
    }
    if (i == 0) bins[cur * 2] = 0;
    if (i == I - 1) bins[cur * 2 + 1] = (int32_t)I;
    if (i > 0 && prev != cur) {
        bins[prev * 2 + 1] = (int32_t)i;
        bins[cur * 2] = (int32_t)i;
    }
}

// ---- stable ONE-PASS tile sort ---------------------------------------------------------------------------------------
// The emission above leaves (tile, splat) pairs in depth order; what remains is a STABLE sort by tile -- at 1080p 8,160
// tiles, a 13-bit key.  rocprim's radix sort takes 8 bits per pass, i.e. two read-and-scatter sweeps over keys and
// values plus a histogram sweep (0.28 ms for the 20 M pairs of the bench frame).  A key range this small fits a
// workgroup's LDS as ONE digit: 8,161 32-bit counters are 32 KB of the CU's 160 KB.  So: one histogram per chunk of the
// pair stream (tile_hist_kernel), a prefix over chunks and tiles that turns the counts into write offsets -- which are
// also the tile_bins the rasteriser wants, so no edge-detection sweep either -- and ONE scatter sweep in which a single
// wave owns a chunk and its offset table (tile_scatter_kernel).  Stability inside a wave costs nothing here: the pairs
// of one splat name distinct tiles, so a wave hands out slots splat segment by splat segment with plain LDS atomics,
// which the LDS executes in program order.  The sorted tile keys are never written: the bins say where each tile's ids
// sit.  Same lists as the radix sort, bit for bit (tests/test_gpu_splat.py).
template <typename TKey>
__global__ __launch_bounds__(256) void tile_hist_kernel(const TKey* __restrict__ keys, int64_t I, int chunk, int T1,
                                                        uint32_t* __restrict__ table) {
    extern __shared__ uint32_t s_hist[];
    for (int t = threadIdx.x; t < T1; t += 256) s_hist[t] = 0u;
    __syncthreads();
    const int64_t k0 = (int64_t)blockIdx.x * chunk, k1 = (k0 + chunk < I) ? k0 + chunk : I;   // rows past the last chunk: zeros
    // 16 bytes of keys per lane and load (chunk starts are multiples of 256 keys: aligned); the tail key by key
    constexpr int PER = 16 / (int)sizeof(TKey);
    const int64_t nvec = k1 > k0 ? (k1 - k0) / PER : 0;
    const uint4* kv = reinterpret_cast<const uint4*>(keys + k0);
    for (int64_t v = threadIdx.x; v < nvec; v += 256) {
        const uint4 q = kv[v];
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (sizeof(TKey) == 2) {
                const uint32_t a = w[i] & 0xFFFFu, b = w[i] >> 16;
                atomicAdd(&s_hist[a < (uint32_t)T1 ? a : (uint32_t)(T1 - 1)], 1u);
                atomicAdd(&s_hist[b < (uint32_t)T1 ? b : (uint32_t)(T1 - 1)], 1u);
            } else {
                atomicAdd(&s_hist[w[i] < (uint32_t)T1 ? w[i] : (uint32_t)(T1 - 1)], 1u);
            }
        }
    }
    for (int64_t k = k0 + nvec * PER + threadIdx.x; k < k1; k += 256) {
        const uint32_t key = (uint32_t)keys[k];
        atomicAdd(&s_hist[key < (uint32_t)T1 ? key : (uint32_t)(T1 - 1)], 1u);
    }
    __syncthreads();
    uint32_t* row = table + (size_t)blockIdx.x * T1;
    for (int t = threadIdx.x; t < T1; t += 256) row[t] = s_hist[t];
}

// column sums of each row segment: segsum[seg][t] = sum over the segment's rows of table[row][t]
__global__ __launch_bounds__(256) void tile_colsum_kernel(const uint32_t* __restrict__ table, int rows_per_seg, int T1,
                                                          uint32_t* __restrict__ segsum) {
    const int t = blockIdx.x * 256 + threadIdx.x, seg = blockIdx.y;
    if (t >= T1) return;
    const uint32_t* col = table + (size_t)seg * rows_per_seg * T1 + t;
    uint32_t sum = 0u;
#pragma unroll 8
    for (int r = 0; r < rows_per_seg; ++r) sum += col[(size_t)r * T1];
    segsum[(size_t)seg * T1 + t] = sum;
}

// per tile: the exclusive prefix of its segment sums over the segments (in place) and the tile's total
__global__ __launch_bounds__(256) void tile_segscan_kernel(uint32_t* __restrict__ segsum, int T1, uint32_t* __restrict__ total) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T1) return;
    uint32_t x[TS_SEG];
#pragma unroll
    for (int seg = 0; seg < TS_SEG; ++seg) x[seg] = segsum[(size_t)seg * T1 + t];
    uint32_t run = 0u;
#pragma unroll
    for (int seg = 0; seg < TS_SEG; ++seg) {
        segsum[(size_t)seg * T1 + t] = run;
        run += x[seg];
    }
    total[t] = run;
}

// one workgroup: the exclusive prefix of the tile totals over the tiles -> start[t] (start[T1] = all pairs), and the
// tile_bins the rasteriser reads.  A tile's total is the sum of NSEG partial rows total[s][t] (1: already summed).
// One workgroup per view of a batch (blockIdx.x; `base` = its pairs' first slot, read from base_of[view] when given): the
// view's NSEG partial rows, starts and bins follow the previous view's.
template <int NSEG, int S = 1>
__global__ __launch_bounds__(1024) void tile_scan_kernel(const uint32_t* __restrict__ total, int T1, int tiles,
                                                         uint32_t* __restrict__ start, int32_t* __restrict__ bins,
                                                         RsSegs<S> base_of) {
    extern __shared__ uint32_t s_tot[];      // [T1] tile totals, then [16] wave sums
    uint32_t* s_w = s_tot + T1;
    const int g = blockIdx.x;
    total += (size_t)g * NSEG * T1;
    start += (size_t)g * (T1 + 1);
    bins += (size_t)g * tiles * 2;
    for (int t = threadIdx.x; t < T1; t += 1024) {      // (coalesced over the tiles, segment by segment)
        uint32_t n = 0u;
#pragma unroll
        for (int sg = 0; sg < NSEG; ++sg) n += total[(size_t)sg * T1 + t];
        s_tot[t] = n;
    }
    __syncthreads();
    const int per = (T1 + 1023) / 1024;
    const int t0 = threadIdx.x * per, t1 = (t0 + per < T1) ? t0 + per : T1;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t mine = 0u;
    for (int t = t0; t < t1; ++t) mine += s_tot[t];
    uint32_t incl = mine;      // inclusive scan of the 1,024 partial sums: inside each wave, then over the 16 waves
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = __shfl_up(incl, d, 64);
        if (lane >= d) incl += v;
    }
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    uint32_t before = 0u;
#pragma unroll
    for (int w = 0; w < 16; ++w) before += w < wv ? s_w[w] : 0u;
    uint32_t run = (uint32_t)base_of.pb[g] + before + incl - mine;
    for (int t = t0; t < t1; ++t) {
        const uint32_t n = s_tot[t];
        start[t] = run;
        if (t < tiles) {      // an empty tile keeps the (0, 0) of gsplat's zero-filled tile_bins
            bins[t * 2] = n ? (int32_t)run : 0;
            bins[t * 2 + 1] = n ? (int32_t)(run + n) : 0;
        }
        run += n;
    }
    if (threadIdx.x == 1023) start[T1] = run;
}

// counts -> write offsets, in place: table[row][t] = start[t] + segsum[seg][t] + sum of the segment's earlier rows
__global__ __launch_bounds__(256) void tile_apply_kernel(uint32_t* __restrict__ table, int rows_per_seg, int T1,
                                                         const uint32_t* __restrict__ segsum,
                                                         const uint32_t* __restrict__ start) {
    const int t = blockIdx.x * 256 + threadIdx.x, seg = blockIdx.y;
    if (t >= T1) return;
    uint32_t* col = table + (size_t)seg * rows_per_seg * T1 + t;
    uint32_t run = start[t] + segsum[(size_t)seg * T1 + t];
#pragma unroll 8
    for (int r = 0; r < rows_per_seg; ++r) {
        const uint32_t c = col[(size_t)r * T1];
        col[(size_t)r * T1] = run;
        run += c;
    }
}

// One wave per chunk.  Pairs arrive in depth order; within a 64-pair vector the pairs of ONE splat (a run of equal ids)
// name distinct tiles, so all of them can take their slots with one conflict-free LDS atomic; runs are served in order
// (the LDS executes a wave's operations in program order), which makes the scatter stable.  A wave is alone with its
// memory latency (four waves per CU: the 32-KB tables), so it works on four vectors per round and asks for the next
// round's pairs before it ranks this round's.
#define TS_VEC 4
template <typename TKey>
__global__ __launch_bounds__(64) void tile_scatter_kernel(const TKey* __restrict__ keys, const int32_t* __restrict__ vals,
                                                          int64_t I, int chunk, int T1, const uint32_t* __restrict__ table,
                                                          int32_t* __restrict__ out) {
    extern __shared__ uint32_t s_off[];
    const int lane = threadIdx.x;
    // (chunk = blockIdx: an XCD-contiguous chunk order gained nothing, the scatter is bound by the number of store
    // requests, not by where the partially written lines live -- docs/experiments.md 4.5.75)
    const int cid = (int)blockIdx.x;
    {
        const uint32_t* row = table + (size_t)cid * T1;
#pragma unroll 8
        for (int t = lane; t < T1; t += 64) s_off[t] = row[t];
    }
    __syncthreads();
    const int64_t k0 = (int64_t)cid * chunk, k1 = (k0 + chunk < I) ? k0 + chunk : I;
    uint32_t key[TS_VEC], nkey[TS_VEC];
    int32_t id[TS_VEC], nid[TS_VEC];
    auto fetch = [&](int64_t k, uint32_t (&kk)[TS_VEC], int32_t (&ii)[TS_VEC]) {
#pragma unroll
        for (int v = 0; v < TS_VEC; ++v) {
            const int64_t e = k + 64 * v + lane;
            const bool ok = e < k1;
            kk[v] = ok ? (uint32_t)keys[e] : 0u;
            ii[v] = ok ? vals[e] : -1;
        }
    };
    fetch(k0, nkey, nid);
    for (int64_t k = k0; k < k1; k += 64 * TS_VEC) {
#pragma unroll
        for (int v = 0; v < TS_VEC; ++v) {
            key[v] = nkey[v];
            id[v] = nid[v];
        }
        if (k + 64 * TS_VEC < k1) fetch(k + 64 * TS_VEC, nkey, nid);
#pragma unroll
        for (int v = 0; v < TS_VEC; ++v) {
            const bool valid = k + 64 * v + lane < k1;
            const uint32_t kq = key[v] < (uint32_t)T1 ? key[v] : (uint32_t)(T1 - 1);
            const int32_t prev = __shfl_up(id[v], 1, 64);
            uint64_t starts = __builtin_amdgcn_ballot_w64(valid && (lane == 0 || id[v] != prev));
            uint32_t pos = 0u;
            while (starts) {      // uniform: one round per splat run of the vector
                const int lo = __builtin_ctzll(starts);
                starts &= starts - 1;
                const int hi = starts ? __builtin_ctzll(starts) : 64;
                if (valid && lane >= lo && lane < hi) pos = atomicAdd(&s_off[kq], 1u);
            }
            if (valid) out[pos] = id[v];      // (sentinel pairs land behind the last tile's range)
        }
    }
}

// ---- staged LSD radix passes ---------------------------------------------------------------------------------------------
// MI355X retires about 81 G isolated 4-byte stores per second, whatever the occupancy and wherever they land (246 us for
// the 20 M ids of the bench frame, benchmarks/exp_scatter_store.hip; 132 / 77 / 53 / 38 us when 2 / 4 / 8 / 16 consecutive
// lanes write consecutive dwords) -- which is where the one-pass tile sort's scatter sits (279 us: every lane of every
// store on a cache line of its own, because a chunk of the depth-ordered stream holds ~1 pair per tile).  A stable sort by a
// SMALL digit does not have that problem: with <= 128 digit values a wave's 2,048 pairs hold >= 16 per value, so the wave
// ranks them, stages ids and keys in LDS in digit order and writes each digit's pairs as ONE run of consecutive slots.  Two
// such passes (low digit, then high digit: LSD) sort by the 13-bit tile; four of them with 8-bit digits sort the 32-bit
// depth keys.  Ranking: the lanes of a 64-pair vector that share a digit find each other with one ballot per digit bit (a
// lane keeps the lanes that agree with it on every bit); the lowest takes the slots for all with one LDS atomic, the others
// add their position among the peers -- stream order, i.e. stable.  Same lists as the one-pass sort, rocprim's radix sort
// (tile) and rocprim's stable sort (depth), bit for bit (tests/test_gpu_splat.py).
// One wave talks to itself through LDS in these kernels (lane A's atomic, lane B's read of the same word).  The LDS executes a
// wave's instructions in program order, so no wait is needed -- this only tells the COMPILER that the accesses on either side
// may not change places (wavefront-scope fences emit no instruction).
__device__ __forceinline__ void rs_wave_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename TKey, bool FULL, bool SEG = false>
__global__ __launch_bounds__(1024) void rs_hist_kernel(const TKey* __restrict__ keys, RsSegs<SEG ? UNERF_SPLAT_MAX_VIEWS : 1> segs, int chunk, int nchunk, uint32_t kmax,
                                                      int shift, int B, int cpw, uint32_t* __restrict__ table, uint32_t* __restrict__ full) {
    extern __shared__ uint32_t s_rs[];       // [waves][256] digit counters, then FULL: [kmax + 1] whole-key counters of the workgroup
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wpb = (int)(blockDim.x >> 6);
    uint32_t* dig = s_rs + wv * 256;
    uint32_t* fh = s_rs + wpb * 256;
    if (FULL) {
        for (uint32_t t = threadIdx.x; t <= kmax; t += blockDim.x) fh[t] = 0u;
        __syncthreads();
    }
    const uint32_t dmask = (uint32_t)B - 1u;
    constexpr int PER = 16 / (int)sizeof(TKey);
    for (int cc = 0; cc < cpw; ++cc) {
        const int c = ((int)blockIdx.x * wpb + wv) * cpw + cc;
        if (c >= nchunk) break;                   // (uniform per wave)
#pragma unroll
        for (int i = 0; i < 4; ++i) dig[lane + 64 * i] = 0u;
        int64_t k0, k1;
        rs_chunk_range<SEG>(segs, rs_seg_of<SEG>(segs, c), c, chunk, k0, k1);
        auto count = [&](uint32_t key) {
            const uint32_t kq = key < kmax ? key : kmax;
            atomicAdd(&dig[(kq >> shift) & dmask], 1u);
            if (FULL) atomicAdd(&fh[kq], 1u);
        };
        // a segment's first chunk starts where the view before it ended: the keys up to the next 16-byte boundary one by one
        // (a single segment's chunks are multiples of 256 keys: none)
        if (SEG) {
            const int64_t ka = ((k0 + PER - 1) / PER) * PER < k1 ? ((k0 + PER - 1) / PER) * PER : k1;
            for (int64_t k = k0 + lane; k < ka; k += 64) count((uint32_t)keys[k]);
            k0 = ka;
        }
        const int64_t nvec = (k1 - k0) / PER;
        const uint4* kv = reinterpret_cast<const uint4*>(keys + k0);
        for (int64_t v0 = 0; v0 < nvec; v0 += 256) {      // four 16-byte loads per lane in flight
            uint4 q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t v = v0 + 64 * u + lane;
                q[u] = kv[v < nvec ? v : nvec - 1];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (v0 + 64 * u + lane < nvec) {
                    const uint32_t w[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (sizeof(TKey) == 2) {
                            count(w[i] & 0xFFFFu);
                            count(w[i] >> 16);
                        } else {
                            count(w[i]);
                        }
                    }
                }
            }
        }
        for (int64_t k = k0 + nvec * PER + lane; k < k1; k += 64) count((uint32_t)keys[k]);
        rs_wave_order();      // (the reads below see every atomic above)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (lane + 64 * i < B) table[(size_t)(lane + 64 * i) * nchunk + c] = dig[lane + 64 * i];
    }
    if (FULL) {
        __syncthreads();
        uint32_t* row = full + (size_t)blockIdx.x * (kmax + 1);
        for (uint32_t t = threadIdx.x; t <= kmax; t += blockDim.x) row[t] = fh[t];
    }
}

// column sums of the whole-key histogram rows, by row segment: seg[g][s][t] = sum of rows [r0 + s rps, r0 + (s + 1) rps) of
// column t, where segment g (blockIdx.z) owns the histogram rows (16 chunks each) [cb[g] / 16, ceil(cb[g + 1] / 16))
template <int S>
__global__ __launch_bounds__(256) void rs_colsum_kernel(const uint32_t* __restrict__ full, RsSegs<S> segs, int T1,
                                                        uint32_t* __restrict__ seg) {
    const int t = blockIdx.x * 256 + threadIdx.x, sg = blockIdx.y, g = blockIdx.z;
    if (t >= T1) return;
    const int rlo = segs.cb[g] / 16, rows = (segs.cb[g + 1] + 15) / 16;
    const int rps = (rows - rlo + 15) / 16;
    const int r0 = rlo + sg * rps, r1 = (r0 + rps < rows) ? r0 + rps : rows;
    uint32_t sum = 0u;
#pragma unroll 8
    for (int r = r0; r < r1; ++r) sum += full[(size_t)r * T1 + t];
    seg[((size_t)g * 16 + sg) * T1 + t] = sum;
}

// one workgroup per digit: exclusive prefix of its row over the chunks (in place) and the digit's total
// (grid.y: the segments -- segment g scans its own chunks and leaves its totals in dtotal[g][256])
template <int S>
__global__ __launch_bounds__(1024) void rs_rowscan_kernel(uint32_t* __restrict__ table, int nchunk_all, RsSegs<S> segs,
                                                          uint32_t* __restrict__ dtotal) {
    __shared__ uint32_t s_w[16];
    const int g = blockIdx.y;
    uint32_t* row = table + (size_t)blockIdx.x * nchunk_all + segs.cb[g];
    const int nchunk = segs.cb[g + 1] - segs.cb[g];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t carry = 0u;
    for (int base = 0; base < nchunk; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const uint32_t x = i < nchunk ? row[i] : 0u;
        uint32_t incl = x;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        uint32_t before = 0u, all = 0u;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const uint32_t t = s_w[w];
            before += w < wv ? t : 0u;
            all += t;
        }
        if (i < nchunk) row[i] = carry + before + incl - x;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) dtotal[(size_t)g * 256 + blockIdx.x] = carry;
}

// one wave per chunk of M pairs: rank, stage in LDS in digit order, write out digit run by digit run.  DMAX = digit values the
// LDS tables are sized for (128: tile digits, 256: depth digits).
// Ranking a 64-pair vector: every lane ORs its lane bit into its digit's 64-bit word (one LDS instruction), reads the word back
// -- the lanes that share its digit -- and clears it; its slot is the digit's running position (read by all, advanced by the
// first of the peers) plus the number of peers in lower lanes.  The LDS executes a wave's instructions in program order, so the
// five of them need no wait on one another, and four vectors are in flight at a time.
template <int M, int DMAX, typename TKey>
struct RsLds {
    static constexpr int WAVE_WORDS = 4 * DMAX + M + (M * (int)sizeof(TKey) + 3) / 4;     // cur | delta | peer words | vals | keys
};
// COUNTS (the depth sort's last pass): also writes, in output order, how many tiles each splat hits -- num_tiles_hit recovered from
// its inclusive scan, 0 for culled splats -- the gather a separate kernel used to make (21 us, waiting on three random reads per splat).
template <typename TKey, int M, int DMAX, bool KEYS_OUT, bool COUNTS = false, bool SEG = false>
__global__ __launch_bounds__(256) void rs_scatter_kernel(const TKey* __restrict__ keys, const int32_t* __restrict__ vals,
                                                         RsSegs<SEG ? UNERF_SPLAT_MAX_VIEWS : 1> segs,
                                                         int nchunk, uint32_t kmax, int shift, int B,
                                                         const uint32_t* __restrict__ table, const uint32_t* __restrict__ dtotal,
                                                         TKey* __restrict__ keys_out, int32_t* __restrict__ vals_out,
                                                         const int32_t* __restrict__ radii = nullptr, const int32_t* __restrict__ cum = nullptr,
                                                         int32_t* __restrict__ counts_out = nullptr) {
    extern __shared__ uint32_t s_rs[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = (int)blockIdx.x * (int)(blockDim.x >> 6) + wv;      // (1 - 4 waves per workgroup: the launcher's choice)
    if (c >= nchunk) return;
    const int sgi = rs_seg_of<SEG>(segs, c);
    int64_t k0, k1;
    rs_chunk_range<SEG>(segs, sgi, c, M, k0, k1);
    if (SEG && k1 <= k0) return;             // (a padding chunk of a segment: no pairs)
    const int cend = SEG ? segs.cb[sgi + 1] : nchunk;
    if (SEG) dtotal += (size_t)sgi * 256;
    uint32_t* cur = s_rs + (size_t)wv * RsLds<M, DMAX, TKey>::WAVE_WORDS;
    uint32_t* delta = cur + DMAX;
    uint32_t* pw = delta + DMAX;             // [DMAX][2]
    int32_t* sval = reinterpret_cast<int32_t*>(pw + 2 * DMAX);
    TKey* skey = reinterpret_cast<TKey*>(sval + M);
    const uint32_t dmask = (uint32_t)B - 1u;
    constexpr int DPL = DMAX / 64;           // digits per lane in the prologue
    {   // lane l owns digits DPL l .. DPL l + DPL - 1.  For digit d: this chunk's pairs start at slot ls[d] of the staged order
        // (prefix of the chunk's counts over the digits) and at gs[d] = (all pairs with a smaller digit) + (pairs with digit d in
        // earlier chunks) of the output; the chunk's count is the difference of two neighbours of the prefix row
        uint32_t tot[DPL], pre[DPL], cnt[DPL], tsum = 0u, csum = 0u;
#pragma unroll
        for (int i = 0; i < DPL; ++i) {
            const int d = DPL * lane + i;
            tot[i] = pre[i] = cnt[i] = 0u;
            if (d < B) {
                tot[i] = dtotal[d];
                pre[i] = table[(size_t)d * nchunk + c];
                cnt[i] = (c + 1 < cend ? table[(size_t)d * nchunk + c + 1] : tot[i]) - pre[i];
            }
            tsum += tot[i];
            csum += cnt[i];
        }
        uint32_t ti = tsum, ci = csum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t v0 = __shfl_up(ti, d, 64), v1 = __shfl_up(ci, d, 64);
            if (lane >= d) { ti += v0; ci += v1; }
        }
        uint32_t gb = (SEG ? (uint32_t)segs.pb[sgi] : 0u) + ti - tsum, lb = ci - csum;
#pragma unroll
        for (int i = 0; i < DPL; ++i) {
            const int d = DPL * lane + i;
            cur[d] = lb;
            delta[d] = gb + pre[i] - lb;
            pw[2 * d] = 0u;
            pw[2 * d + 1] = 0u;
            gb += tot[i];
            lb += cnt[i];
        }
        rs_wave_order();
    }
    const int m = (int)(k1 - k0);                         // pairs of this chunk
    // every pair of the chunk is requested before the first is ranked (2 registers per vector: the ranking below is a chain
    // of LDS round trips, a global load inside it would cost its whole latency once per vector)
    constexpr int NV = M / 64;
    uint32_t key[NV];
    int32_t val[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int e = 64 * v + lane;
        const int64_t ec = k0 + (e < m ? e : m - 1);       // clamped, not predicated
        key[v] = (uint32_t)keys[ec];
        val[v] = vals[ec];
    }
    const uint32_t mybit = 1u << (lane & 31), half = (uint32_t)lane >> 5;
#pragma unroll
    for (int g = 0; g < NV; g += 4) {
        uint32_t kq[4], d[4], base[4], rank[4];
        uint2 peers[4];
        bool valid[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            valid[i] = 64 * (g + i) + lane < m;
            kq[i] = key[g + i] < kmax ? key[g + i] : kmax;
            d[i] = (kq[i] >> shift) & dmask;
            atomicOr(&pw[2 * d[i] + half], valid[i] ? mybit : 0u);
            rs_wave_order();
            peers[i] = *reinterpret_cast<const uint2*>(&pw[2 * d[i]]);
            *reinterpret_cast<uint2*>(&pw[2 * d[i]]) = make_uint2(0u, 0u);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            rank[i] = __builtin_amdgcn_mbcnt_hi(peers[i].y, __builtin_amdgcn_mbcnt_lo(peers[i].x, 0u));
            const uint32_t cntp = (uint32_t)(__builtin_popcount(peers[i].x) + __builtin_popcount(peers[i].y));
            base[i] = cur[d[i]];
            atomicAdd(&cur[d[i]], (valid[i] && rank[i] == 0u) ? cntp : 0u);      // the first of the peers advances it for all
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (valid[i]) {
                sval[base[i] + rank[i]] = val[g + i];
                skey[base[i] + rank[i]] = (TKey)kq[i];
            }
        }
    }
    rs_wave_order();      // the staged order is complete
#pragma unroll 4
    for (int j = 0; j < M / 64; ++j) {
        const int slot = 64 * j + lane;
        if (slot < m) {
            const uint32_t kq = (uint32_t)skey[slot];
            const uint32_t dst = delta[(kq >> shift) & dmask] + (uint32_t)slot;
            if (KEYS_OUT) keys_out[dst] = (TKey)kq;
            const int32_t i = sval[slot];
            vals_out[dst] = i;
            if (COUNTS) counts_out[dst] = radii[i] > 0 ? cum[i] - (i == 0 ? 0 : cum[i - 1]) : 0;
        }
    }
}

// the gsplat-style 64-bit ids of the sorted lists (on request only): the tile of entry i is found in the tile offsets
__global__ __launch_bounds__(256) void tile_isect_ids_kernel(const uint32_t* __restrict__ start, int T1,
                                                             const int32_t* __restrict__ gids,
                                                             const float* __restrict__ depths, int64_t n,
                                                             int64_t* __restrict__ isect_ids) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = T1;                       // last tile t with start[t] <= i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= (uint32_t)i) lo = mid; else hi = mid;
    }
    isect_ids[i] = ((int64_t)lo << 32) | (int64_t)(uint32_t)__float_as_int(depths[gids[i]]);
}

// ---- the staged passes on the host: one description for the depth sort, the tile sort, one view and a batch ---------------------
// One staged pass: histogram -> row scan -> scatter, over the chunks and segments of `segs` (SEG: the batch's kernels).
//   TKey, M, DMAX, shift, digits: the keys, the pairs per chunk, the digit values the LDS tables are sized for and the digit
//   FULL: the histogram also counts whole keys (<= kmax) into `full`, one row per 16-chunk workgroup; else `full` is unused
//   KEYS_OUT / COUNTS: as in rs_scatter_kernel (kout; radii, cum, counts)
//   SWPB: waves (= chunks) per scatter workgroup -- 4 in the depth sort, 1 in the tile sort (1, 2 or 4 measured alike: 4.5.77);
//   the histogram has 16 waves per workgroup when FULL, else 4
template <bool SEG, typename TKey, int M, int DMAX, int SWPB, bool FULL, bool KEYS_OUT, bool COUNTS = false>
static void rs_pass(const RsSegs<SEG ? UNERF_SPLAT_MAX_VIEWS : 1>& segs, uint32_t kmax, int shift, int digits, const TKey* kin,
                    const int32_t* vin, TKey* kout, int32_t* vout, uint32_t* table, uint32_t* full, uint32_t* dtotal,
                    hipStream_t st, const int32_t* radii = nullptr, const int32_t* cum = nullptr, int32_t* counts = nullptr) {
    constexpr int S = SEG ? UNERF_SPLAT_MAX_VIEWS : 1, HWPB = FULL ? 16 : 4;
    const int nchunk = segs.cb[segs.n];
    const size_t lds_hist = (HWPB * 256 + (FULL ? (size_t)kmax + 1 : 0)) * sizeof(uint32_t);
    const size_t lds_sc = SWPB * (size_t)RsLds<M, DMAX, TKey>::WAVE_WORDS * sizeof(uint32_t);
    hipLaunchKernelGGL((rs_hist_kernel<TKey, FULL, SEG>), dim3(blocks_for(nchunk, HWPB * RS_CPW)), dim3(64 * HWPB), lds_hist, st,
                       kin, segs, M, nchunk, kmax, shift, digits, RS_CPW, table, full);
    hipLaunchKernelGGL(rs_rowscan_kernel<S>, dim3(digits, segs.n), dim3(1024), 0, st, table, nchunk, segs, dtotal);
    hipLaunchKernelGGL((rs_scatter_kernel<TKey, M, DMAX, KEYS_OUT, COUNTS, SEG>), dim3(blocks_for(nchunk, SWPB)), dim3(64 * SWPB),
                       lds_sc, st, kin, vin, segs, nchunk, kmax, shift, digits, table, dtotal, kout, vout, radii, cum, counts);
}

// every segment's splats in depth order (stable: equal depths keep their index order), segment after segment: four staged 8-bit
// LSD passes; the last one writes `order` and, in that order, the tile counts
template <bool SEG>
static void staged_depth_sort(const SortPtrs& P, const RsSegs<SEG ? UNERF_SPLAT_MAX_VIEWS : 1>& segs, const float* depths,
                              const int32_t* radii, const int32_t* cum_tiles_hit, hipStream_t st) {
    const int64_t NB = segs.pb[segs.n];
    hipLaunchKernelGGL(depth_keys_kernel, dim3(blocks_for(NB, 256)), dim3(256), 0, st, depths, radii, NB, P.dk_out, P.order);
    uint32_t* const k[2] = {P.dk_out, P.dk_in};
    int32_t* const v[2] = {P.order, P.id_in};
    for (int p = 0; p < 4; ++p) {      // (dk_out, order) -> (dk_in, id_in) -> (dk_out, order) -> (dk_in, id_in) -> order
        const int i = p & 1, o = i ^ 1;
        if (p < 3)
            rs_pass<SEG, uint32_t, RS_M_DEPTH, 256, 4, false, true>(segs, 0xFFFFFFFFu, 8 * p, 256, k[i], v[i], k[o], v[o], P.ds_table,
                                                                    nullptr, P.ds_total, st);
        else
            rs_pass<SEG, uint32_t, RS_M_DEPTH, 256, 4, false, false, true>(segs, 0xFFFFFFFFu, 8 * p, 256, k[i], v[i], nullptr, P.order,
                                                                           P.ds_table, nullptr, P.ds_total, st, radii, cum_tiles_hit,
                                                                           P.counts);
    }
}

// the (tile, splat) pairs in depth order.  Tight lists: 8 lanes per splat; gsplat's boxes (37 tiles per splat on the bench frame): 16
template <typename TKey>
static void emit_pairs(const SortPtrs& P, const float* xys, const int32_t* radii, const float* conics, const float* opac, int64_t NB,
                       int bw, int tbx, int tby, hipStream_t st) {
    TKey* tk_in = static_cast<TKey*>(P.tk_in);
    if (conics)
        hipLaunchKernelGGL((map_intersects_kernel<TKey, 8>), dim3(blocks_for(NB, 32)), dim3(256), 0, st, xys, radii, P.order,
                           P.cum_sorted, NB, bw, tbx, tby, conics, opac, tk_in, P.v_in);
    else
        hipLaunchKernelGGL((map_intersects_kernel<TKey, 16>), dim3(blocks_for(NB, 16)), dim3(256), 0, st, xys, radii, P.order,
                           P.cum_sorted, NB, bw, tbx, tby, conics, opac, tk_in, P.v_in);
}

// stable sort of the pairs by tile, segment by segment -- one staged pass on the whole key up to 128 keys, else low digit, then
// high digit -- and per segment: tile totals (column sums of the whole-key histograms, 16 row segments summed in parallel;
// tile_scan_kernel adds them up per tile) -> tile starts from the segment's first slot and its tile_bins.
// ts_table: [128][nchunk] x 2 digit counters + [nchunk / 16][T1] whole-key rows; ts_segsum: dtotal [2][B][256] + total [B][16][T1]
template <bool SEG, typename TKey>
static void staged_tile_sort(const SortPtrs& P, const RsSegs<SEG ? UNERF_SPLAT_MAX_VIEWS : 1>& segs, int tiles, const float* depths,
                             int64_t* isect_ids_sorted, int32_t* gaussian_ids_sorted, int32_t* tile_bins, hipStream_t st) {
    constexpr int S = SEG ? UNERF_SPLAT_MAX_VIEWS : 1;
    const int B = segs.n, nchunk = segs.cb[B], T1 = tiles + 1;
    const int64_t I = segs.pb[B];
    const RsTilePlan rp = rs_tile_plan(I, T1);      // (the digit split only: the chunks are the caller's)
    uint32_t *table0 = P.ts_table, *table1 = table0 + (size_t)128 * nchunk, *full = table1 + (size_t)128 * nchunk;
    uint32_t *dtotal0 = P.ts_segsum, *dtotal1 = dtotal0 + (size_t)256 * B, *total = dtotal1 + (size_t)256 * B;
    uint32_t* start = P.ts_start;                   // [B][T1 + 1]
    TKey *tk_in = static_cast<TKey*>(P.tk_in), *tk_mid = static_cast<TKey*>(P.tk_out);
    const uint32_t kmax = (uint32_t)tiles;
    if (rp.b0 == 0) {      // <= 128 keys: one pass
        rs_pass<SEG, TKey, RS_M_TILE, 128, 1, true, false>(segs, kmax, 0, rp.B1, tk_in, P.v_in, nullptr, gaussian_ids_sorted, table1,
                                                           full, dtotal1, st);
    } else {
        rs_pass<SEG, TKey, RS_M_TILE, 128, 1, true, true>(segs, kmax, 0, rp.B0, tk_in, P.v_in, tk_mid, P.v_mid, table0, full, dtotal0,
                                                          st);
        rs_pass<SEG, TKey, RS_M_TILE, 128, 1, false, false>(segs, kmax, rp.b0, rp.B1, tk_mid, P.v_mid, nullptr, gaussian_ids_sorted,
                                                            table1, nullptr, dtotal1, st);
    }
    hipLaunchKernelGGL(rs_colsum_kernel<S>, dim3(blocks_for(T1, 256), 16, B), dim3(256), 0, st, full, segs, T1, total);
    hipLaunchKernelGGL((tile_scan_kernel<16, S>), dim3(B), dim3(1024), ((size_t)T1 + 16) * sizeof(uint32_t), st, total, T1, tiles,
                       start, tile_bins, segs);
    if (isect_ids_sorted)      // (one segment only)
        hipLaunchKernelGGL(tile_isect_ids_kernel, dim3(blocks_for(I, 256)), dim3(256), 0, st, start, T1, gaussian_ids_sorted, depths,
                           I, isect_ids_sorted);
}

static int sort_check(const char* what, const char* step) {
    char label[96];
    snprintf(label, sizeof(label), "%s %s", what, step);
    return unerf_check_launch(label);
}

// The default bin-and-sort of both entry points: dsegs / tsegs are the segments (views) of the depth passes and of the tile
// passes.  All views' splats are one stream (view-major: id v N + i) and every staged pass runs segment by segment, so each
// view's order is exactly its single-view order -- depth, then splat index on ties; tile, then depth order -- and its pairs leave
// contiguous, view after view.  The keys stay the per-view tile ids (13 bits at 1080p): a combined (view, tile) key would outgrow
// the LDS tables from two 1080p views on.  The caller checks the launches of step 3.
template <bool SEG>
static int bin_sort_body(const char* what, const SortPtrs& P, const RsSegs<SEG ? UNERF_SPLAT_MAX_VIEWS : 1>& dsegs,
                         const RsSegs<SEG ? UNERF_SPLAT_MAX_VIEWS : 1>& tsegs, const float* xys, const float* depths,
                         const int32_t* radii, const int32_t* cum_tiles_hit, const float* conics, const float* opac, int bw, int tbx,
                         int tby, int64_t* isect_ids_sorted, int32_t* gaussian_ids_sorted, int32_t* tile_bins, hipStream_t st) {
    const int64_t NB = dsegs.pb[dsegs.n];
    // 1. splats in depth order
    staged_depth_sort<SEG>(P, dsegs, depths, radii, cum_tiles_hit, st);
    int rc = sort_check(what, "depth sort");
    if (rc) return rc;
    // 2. where each depth-ordered splat's intersections start: one scan over all counts (views stay contiguous)
    own_inclusive_scan(P.counts, P.cum_sorted, NB, static_cast<int32_t*>(P.tmp), st);
    // 3. emission in that order, the stable sort by tile, tile ranges (+ ids)
    emit_pairs<uint16_t>(P, xys, radii, conics, opac, NB, bw, tbx, tby, st);
    if ((rc = sort_check(what, "map"))) return rc;
    staged_tile_sort<SEG, uint16_t>(P, tsegs, tbx * tby, depths, isect_ids_sorted, gaussian_ids_sorted, tile_bins, st);
    return UNERF_OK;
}

// ---- single view: the alternates kept for A/B timing and the identity tests (tests/test_gpu_splat.py), and the sort of images
// the staged tile passes do not serve.  Same steps as bin_sort_body, each with its substitute:
//   rocprim_depth (UNERF_SPLAT_DEPTH_SORT=rocprim): rocprim's stable sort + sorted_counts_kernel
//   rocprim_scan (UNERF_SPLAT_SCAN=rocprim): hipcub's scan
//   tile_sort 0: rocprim's radix sort (UNERF_SPLAT_TILE_SORT=radix, more than TS_MAX_T1 - 1 tiles, 32-bit keys) + tile_edges_kernel,
//             1: the round-4 one-pass LDS-digit sort (=onepass), 2: the staged passes
template <typename TKey>
static int bin_sort_alternates(bool rocprim_depth, bool rocprim_scan, int tile_sort, const SortPtrs& P, const RsSegs<1>& dsegs,
                               const RsSegs<1>& tsegs, const float* xys, const float* depths, const int32_t* radii,
                               const int32_t* cum_tiles_hit, const float* conics, const float* opac, int bw, int tbx, int tby,
                               int bits, int64_t* isect_ids_sorted, int32_t* gaussian_ids_sorted, int32_t* tile_bins,
                               hipStream_t st) {
    const int64_t N = dsegs.pb[1], I = tsegs.pb[1];
    const int tiles = tbx * tby;
    size_t tmp_bytes = P.tmp_bytes;      // (hipcub takes it by reference and leaves it alone)
    hipError_t e = hipSuccess;
    if (rocprim_depth) {
        hipLaunchKernelGGL(depth_keys_kernel, dim3(blocks_for(N, 256)), dim3(256), 0, st, depths, radii, N, P.dk_in, P.id_in);
        e = depth_sort_pairs(P.tmp, tmp_bytes, P.dk_in, P.dk_out, P.id_in, P.order, N, st);
        if (e != hipSuccess) {
            unerf_set_error("splat_bin_sort: depth sort: %s", hipGetErrorString(e));
            return UNERF_ERR_HIP;
        }
        hipLaunchKernelGGL(sorted_counts_kernel, dim3(blocks_for(N, 256)), dim3(256), 0, st, P.order, radii, cum_tiles_hit, N,
                           P.counts);
    } else {
        staged_depth_sort<false>(P, dsegs, depths, radii, cum_tiles_hit, st);
        int rc = unerf_check_launch("splat_bin_sort depth sort");
        if (rc) return rc;
    }
    if (!rocprim_scan) {
        own_inclusive_scan(P.counts, P.cum_sorted, N, static_cast<int32_t*>(P.tmp), st);
    } else {
        e = hipcub::DeviceScan::InclusiveSum(P.tmp, tmp_bytes, P.counts, P.cum_sorted, (int)N, st);
        if (e != hipSuccess) {
            unerf_set_error("splat_bin_sort: scan: %s", hipGetErrorString(e));
            return UNERF_ERR_HIP;
        }
    }
    emit_pairs<TKey>(P, xys, radii, conics, opac, N, bw, tbx, tby, st);
    int rc = unerf_check_launch("splat_bin_sort map");
    if (rc) return rc;
    TKey *tk_in = static_cast<TKey*>(P.tk_in), *tk_out = static_cast<TKey*>(P.tk_out);
    if (tile_sort == 2) {
        staged_tile_sort<false, TKey>(P, tsegs, tiles, depths, isect_ids_sorted, gaussian_ids_sorted, tile_bins, st);
        return unerf_check_launch("splat_bin_sort two-pass tile sort");
    }
    if (tile_sort == 1) {
        const TileSortPlan tp = tile_sort_plan(I, tiles);
        uint32_t *table = P.ts_table, *segsum = P.ts_segsum, *start = P.ts_start, *total = start + tp.T1 + 1;
        const size_t lds = (size_t)tp.T1 * sizeof(uint32_t);
        const int rps = tp.rows / TS_SEG;
        hipLaunchKernelGGL((tile_hist_kernel<TKey>), dim3(tp.rows), dim3(256), lds, st, tk_in, I, tp.chunk, tp.T1, table);
        hipLaunchKernelGGL(tile_colsum_kernel, dim3(blocks_for(tp.T1, 256), TS_SEG), dim3(256), 0, st, table, rps, tp.T1, segsum);
        hipLaunchKernelGGL(tile_segscan_kernel, dim3(blocks_for(tp.T1, 256)), dim3(256), 0, st, segsum, tp.T1, total);
        hipLaunchKernelGGL(tile_scan_kernel<1>, dim3(1), dim3(1024), ((size_t)tp.T1 + 16) * sizeof(uint32_t), st, total, tp.T1, tiles,
                           start, tile_bins, rs_one_seg(tp.nblk, I));
        hipLaunchKernelGGL(tile_apply_kernel, dim3(blocks_for(tp.T1, 256), TS_SEG), dim3(256), 0, st, table, rps, tp.T1, segsum,
                           start);
        hipLaunchKernelGGL((tile_scatter_kernel<TKey>), dim3(tp.nblk), dim3(64), lds, st,
                           tk_in, P.v_in, I, tp.chunk, tp.T1, table, gaussian_ids_sorted);
        if (isect_ids_sorted)
            hipLaunchKernelGGL(tile_isect_ids_kernel, dim3(blocks_for(I, 256)), dim3(256), 0, st, start, tp.T1,
                               gaussian_ids_sorted, depths, I, isect_ids_sorted);
        return unerf_check_launch("splat_bin_sort tile sort");
    }
    e = hipcub::DeviceRadixSort::SortPairs(P.tmp, tmp_bytes, tk_in, tk_out, P.v_in, gaussian_ids_sorted, (int)I, 0, bits, st);
    if (e != hipSuccess) {
        unerf_set_error("splat_bin_sort: tile sort: %s", hipGetErrorString(e));
        return UNERF_ERR_HIP;
    }
    hipLaunchKernelGGL((tile_edges_kernel<TKey>), dim3(blocks_for(I, 256)), dim3(256), 0, st, tk_out,
                       gaussian_ids_sorted, depths, I, tiles, tile_bins, isect_ids_sorted);
    return unerf_check_launch("splat_bin_sort edges");
}

extern "C" int unerf_splat_bin_sort(const float* xys, const float* depths, const int32_t* radii,
                                    const int32_t* cum_tiles_hit, int64_t N, int64_t I, int H, int W, int block_width,
                                    const float* tight_conics, const float* tight_opacities,
                                    int64_t* isect_ids_sorted, int32_t* gaussian_ids_sorted, int32_t* tile_bins,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
    UNERF_REQUIRE(xys && depths && radii && cum_tiles_hit && tile_bins && workspace, "splat_bin_sort: null pointer");
    UNERF_REQUIRE((tight_conics == nullptr) == (tight_opacities == nullptr),
                  "splat_bin_sort: tight lists need both the conics and the opacities the tile counts were made with");
    UNERF_REQUIRE(N >= 1 && N < (1ll << 31) && I >= 0 && I < (1ll << 31), "splat_bin_sort: bad N/I");
    hipStream_t st = (hipStream_t)stream;
    int tbx = (W + block_width - 1) / block_width, tby = (H + block_width - 1) / block_width;
    if (hipMemsetAsync(tile_bins, 0, (size_t)tbx * tby * 2 * sizeof(int32_t), st) != hipSuccess)
        return unerf_check_launch("splat_bin_sort memset");
    if (I == 0) return UNERF_OK;
    UNERF_REQUIRE(gaussian_ids_sorted, "splat_bin_sort: null output");
    const SortWs L = sort_ws_layout(N, I);
    UNERF_REQUIRE(workspace_bytes >= L.total, "splat_bin_sort: workspace %lld < %lld bytes (unerf_splat_sort_workspace_bytes)",
                  (long long)workspace_bytes, (long long)L.total);
    const SortPtrs P = sort_ws_ptrs(workspace, L);
    // one segment each: the depth passes' chunks, and the tile passes' -- not padded
    const RsSegs<1> dsegs = rs_one_seg((int)((N + RS_M_DEPTH - 1) / RS_M_DEPTH), N);
    const RsSegs<1> tsegs = rs_one_seg(rs_tile_plan(I, tbx * tby + 1).nchunk, I);
    // the alternates: asked for by the environment, or an image beyond the staged tile passes (more than TS_MAX_T1 - 1 tiles;
    // up to there the keys have 16 bits: the staged passes' LDS images are sized for them)
    const char* denv = getenv("UNERF_SPLAT_DEPTH_SORT");
    const char* tenv = getenv("UNERF_SPLAT_TILE_SORT");
    const bool rocprim_depth = denv && strcmp(denv, "rocprim") == 0, rocprim_scan = use_rocprim_scan();
    int tile_sort = 0;
    if (tbx * tby + 1 <= TS_MAX_T1 && !(tenv && strcmp(tenv, "radix") == 0)) tile_sort = (tenv && strcmp(tenv, "onepass") == 0) ? 1 : 2;
    if (rocprim_depth || rocprim_scan || tile_sort != 2) {
        const int bits = tile_bits(H, W, block_width);      // (the sentinel tile `tbx * tby` included)
        auto alt = bits <= 16 ? bin_sort_alternates<uint16_t> : bin_sort_alternates<uint32_t>;
        return alt(rocprim_depth, rocprim_scan, tile_sort, P, dsegs, tsegs, xys, depths, radii, cum_tiles_hit, tight_conics,
                   tight_opacities, block_width, tbx, tby, bits, isect_ids_sorted, gaussian_ids_sorted, tile_bins, st);
    }
    const int rc = bin_sort_body<false>("splat_bin_sort", P, dsegs, tsegs, xys, depths, radii, cum_tiles_hit, tight_conics,
                                        tight_opacities, block_width, tbx, tby, isect_ids_sorted, gaussian_ids_sorted, tile_bins, st);
    return rc ? rc : unerf_check_launch("splat_bin_sort two-pass tile sort");
}

// B views of one splat set in the same launches: bin_sort_body over one segment per view.  Its own: the checks, each view's
// chunks of the tile passes padded to whole 16-chunk histogram workgroups, and the table-fit check that padding calls for.
extern "C" int unerf_splat_bin_sort_batch(const float* xys, const float* depths, const int32_t* radii,
                                          const int32_t* cum_tiles_hit, int B, int64_t N, const int64_t* isects_host, int H,
                                          int W, int block_width, const float* tight_conics, const float* tight_opacities,
                                          int32_t* gaussian_ids_sorted, int32_t* tile_bins, void* workspace,
                                          int64_t workspace_bytes, void* stream) {
    UNERF_REQUIRE(xys && depths && radii && cum_tiles_hit && isects_host && tile_bins && workspace,
                  "splat_bin_sort_batch: null pointer");
    UNERF_REQUIRE((tight_conics == nullptr) == (tight_opacities == nullptr),
                  "splat_bin_sort_batch: tight lists need both the conics and the opacities the tile counts were made with");
    UNERF_REQUIRE(B >= 1 && B <= UNERF_SPLAT_MAX_VIEWS, "splat_bin_sort_batch: B=%d outside [1,%d]", B, UNERF_SPLAT_MAX_VIEWS);
    UNERF_REQUIRE(N >= 1 && (int64_t)B * N < UNERF_SPLAT_MAX_BATCH_SPLATS, "splat_bin_sort_batch: bad N (B*N = %lld)",
                  (long long)B * (long long)N);
    UNERF_REQUIRE(block_width >= 1 && block_width <= 16 && H > 0 && W > 0, "splat_bin_sort_batch: bad block_width/H/W");
    int64_t I = 0;
    for (int v = 0; v < B; ++v) {
        UNERF_REQUIRE(isects_host[v] >= 0 && isects_host[v] < (1ll << 31), "splat_bin_sort_batch: view %d: %lld intersections", v,
                      (long long)isects_host[v]);
        I += isects_host[v];
    }
    UNERF_REQUIRE(I < (1ll << 31), "splat_bin_sort_batch: %lld intersections over the batch, the ids are int32 (< 2^31)",
                  (long long)I);
    const int tbx = (W + block_width - 1) / block_width, tby = (H + block_width - 1) / block_width, tiles = tbx * tby;
    UNERF_REQUIRE(tiles <= UNERF_SPLAT_BATCH_MAX_TILES, "splat_bin_sort_batch: %d tiles, the batched tile sort serves up to %d",
                  tiles, UNERF_SPLAT_BATCH_MAX_TILES);
    UNERF_REQUIRE(I == 0 || gaussian_ids_sorted, "splat_bin_sort_batch: null output");
    // one segment per view: cpv depth chunks each; the view's own tile chunks, in whole histogram workgroups
    const int cpv = (int)((N + RS_M_DEPTH - 1) / RS_M_DEPTH);
    RsSegs<UNERF_SPLAT_MAX_VIEWS> dsegs, tsegs;
    dsegs.n = tsegs.n = B; dsegs.cb[0] = tsegs.cb[0] = 0; dsegs.pb[0] = tsegs.pb[0] = 0;
    for (int v = 0; v < B; ++v) {
        const int64_t c = (isects_host[v] + RS_M_TILE - 1) / RS_M_TILE;
        dsegs.cb[v + 1] = (v + 1) * cpv; dsegs.pb[v + 1] = (int64_t)(v + 1) * N;
        tsegs.cb[v + 1] = tsegs.cb[v] + (int)(((c + 15) / 16) * 16); tsegs.pb[v + 1] = tsegs.pb[v] + isects_host[v];
    }
    const SortWs L = sort_ws_layout(N, I, B, true);
    int64_t need, have;
    UNERF_REQUIRE(rs_tile_tables_fit(L, tsegs.cb[B], tiles + 1, need, have),
                  "splat_bin_sort_batch: tile tables of %lld bytes exceed the %lld the workspace layout reserves (internal)",
                  (long long)need, (long long)have);
    UNERF_REQUIRE(workspace_bytes >= L.total,
                  "splat_bin_sort_batch: workspace %lld < %lld bytes (unerf_splat_sort_workspace_bytes_batch)",
                  (long long)workspace_bytes, (long long)L.total);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(tile_bins, 0, (size_t)B * tiles * 2 * sizeof(int32_t), st) != hipSuccess)
        return unerf_check_launch("splat_bin_sort_batch memset");
    if (I == 0) return UNERF_OK;
    const int rc = bin_sort_body<true>("splat_bin_sort_batch", sort_ws_ptrs(workspace, L), dsegs, tsegs, xys, depths, radii,
                                       cum_tiles_hit, tight_conics, tight_opacities, block_width, tbx, tby, nullptr,
                                       gaussian_ids_sorted, tile_bins, st);
    return rc ? rc : unerf_check_launch("splat_bin_sort_batch");
}

// ======================================================================================
// rasteriser: one 16x16 tile per workgroup, 256-splat LDS batches, C channels at once
// ======================================================================================
// gsplat's schedule (a tile per workgroup, a pixel per thread, the tile's depth-sorted splats staged through shared
// memory in batches) with two MI355X-side changes that leave every blended term untouched:
//  * WAVE-LEVEL CULLING.  A wave64 of a 16 x 16 tile is one 8 x 8 quadrant of it.  A splat contributes to a pixel
//    only where alpha = min(0.999, o e^-sigma) >= 1/255, i.e. inside the ellipse sigma <= ln(255 o) -- usually a good
//    deal smaller than the 3-sigma square the tile lists are built from (and empty when o < 1/255).  The thread that
//    stages a splat tests the ellipse's bounding box against the tile's four quadrants (conservatively: a margin far
//    above the rounding of the in-loop test) and leaves a 4-bit mask; every wave then compacts the batch into its own
//    index list with ballots and walks only that.  A culled (pixel, splat) pair is one the loop body would have skipped with
//    `continue`, so sums, transmittances and final indices are bit-identical to the uncull loop (test_gpu_splat.py).
//  * BOUNDED second pass.  The depth-variance pass blends with the same alphas as the first, so each pixel stops at the
//    final index the first pass recorded instead of re-deriving it from the transmittance (stop_idx).
struct RasterArgs {
    const int32_t* ids;
    const int32_t* bins;
    const float* xys;
    const float* conics;
    const float* colors;
    const float* opac;
    const float* bg;
    int H, W, bw;
    float* out;
    float* finalT;
    int32_t* final_idx;
    const int32_t* stop_idx;   // BOUNDED: per-pixel last index to visit (a previous pass's final_idx)
    int cull;                  // 0: walk every staged splat (reference schedule; kept for the identity test)
    unsigned int* chan_max;    // NULL, or the running max (float bits, values >= 0) of out[..., max_ch] over the image
    int max_ch;
};

// which of the tile's four 8 x 8 quadrants can see the splat?  Conservative: returns 0xF when in doubt.  (A wave64 of the
// 16 x 16 tile is one quadrant -- bit q = 2 (row half) + (column half) -- instead of a 4-row strip: the square has the
// smallest perimeter a 64-pixel footprint can have, so an r = 2..4 px ellipse reaches fewer of them.)
__device__ __forceinline__ uint32_t raster_quad_mask(float x, float y, float op, float ca, float cb, float cc, float tile_x0,
                                                     float tile_y0) {
    if (!(op >= 0.0039f)) return (op != op) ? 0xFu : 0u;      // alpha <= opacity < 1/255 (0.00392...) everywhere
    const float det = ca * cc - cb * cb;
    if (!(det > 0.f) || !(ca > 0.f) || !(cc > 0.f)) return 0xFu;   // not an ellipse (or NaN): no culling
    // sigma <= tau bounds |dx| <= sqrt(2 tau cc / det), |dy| <= sqrt(2 tau ca / det); tau = ln(255 o) padded by 1 % + 0.01,
    // the box by another 1 % + 0.05 px: orders of magnitude above the fp32 rounding of sigma and of __expf
    const float tau = fmaf(__logf(255.f * op), 1.01f, 0.01f);
    const float inv = 2.f * tau / det;
    const float hx = fmaf(sqrtf(inv * cc), 1.01f, 0.05f), hy = fmaf(sqrtf(inv * ca), 1.01f, 0.05f);
    if (!(hx == hx) || !(hy == hy)) return 0xFu;
    // pixel centres of quadrant (qx, qy): x in [x0 + 8 qx + 0.5, x0 + 8 qx + 7.5], y likewise
    uint32_t mx = 0u, my = 0u;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const float xlo = tile_x0 + 8.f * (float)q + 0.5f, ylo = tile_y0 + 8.f * (float)q + 0.5f;
        if (!(x + hx < xlo || x - hx > xlo + 7.f)) mx |= 1u << q;
        if (!(y + hy < ylo || y - hy > ylo + 7.f)) my |= 1u << q;
    }
    // bit 2 qy + qx
    return ((my & 1u) ? mx : 0u) | ((my & 2u) ? (mx << 2) : 0u);
}

template <int C, bool BOUNDED>
__global__ __launch_bounds__(256) void raster_kernel(RasterArgs a) {
    // one 16-byte + one 8-byte broadcast read per splat instead of six 4-byte ones
    // one record per staged splat, REC4 16-byte words: [x, y, opacity, conic a | conic b, c, colour 0, 1 | colour 2 ...]
    constexpr int REC4 = (6 + C + 3) / 4;
    __shared__ float4 s_rec[256 * REC4];
    __shared__ uint8_t s_mask[256];
    __shared__ uint16_t s_list[4][256];
    const int bw = a.bw;
    const int tbx = (a.W + bw - 1) / bw;
    {   // view blockIdx.z of a batch (unerf_splat_rasterize_batch): its bins, images and maximum; the ids index the whole batch
        const int64_t vw = blockIdx.z, hw = (int64_t)a.H * a.W;
        a.bins += vw * 2 * tbx * (int64_t)((a.H + bw - 1) / bw);
        a.out += vw * hw * C;
        a.finalT += vw * hw;
        if (a.final_idx) a.final_idx += vw * hw;
        if (BOUNDED) a.stop_idx += vw * hw;
        if (a.chan_max) a.chan_max += vw;
    }
    const int bx = blockIdx.x, by = blockIdx.y;
    const int tile = by * tbx + bx;
    const int tr = threadIdx.x;
    // 16-wide tiles: a wave owns one 8 x 8 quadrant (wave w: quadrant column w & 1, row w >> 1; lane l: pixel (l & 7,
    // l >> 3) of it); narrower tiles keep the row-major mapping (no culling there)
    const int ly = bw == 16 ? 8 * (tr >> 7) + ((tr & 63) >> 3) : tr / bw;
    const int lx = bw == 16 ? 8 * ((tr >> 6) & 1) + (tr & 7) : tr - (tr / bw) * bw;
    const int i = by * bw + ly, j = bx * bw + lx;
    const float px = (float)j + 0.5f, py = (float)i + 0.5f;
    const bool inside = (ly < bw) && (i < a.H) && (j < a.W);
    const int64_t p = (int64_t)i * a.W + j;
    bool done = !inside;
    const int r0 = a.bins[tile * 2], r1 = a.bins[tile * 2 + 1];
    const int nbatch = (r1 - r0 + 255) / 256;
    const int stop = (BOUNDED && inside) ? a.stop_idx[p] : 0;
    const bool cull = a.cull && bw == 16;                       // uniform: the quadrant geometry is the 16-wide tile's
    const int wv = __builtin_amdgcn_readfirstlane(tr >> 6), lane = tr & 63;
    const float tile_x0 = (float)(bx * bw), tile_y0 = (float)(by * bw);
    float T = 1.f;
    int cur_idx = 0;
    float pix[C];
#pragma unroll
    for (int c = 0; c < C; ++c) pix[c] = 0.f;
    for (int b = 0; b < nbatch; ++b) {
        const int start = r0 + 256 * b;
        if (BOUNDED) done = done || start > stop;
        if (__syncthreads_count(done ? 1 : 0) >= 256) break;
        const int idx = start + tr;
        if (idx < r1) {
            int g = a.ids[idx];
            const float x = a.xys[g * 2], y = a.xys[g * 2 + 1], op = a.opac[g];
            const float ca = a.conics[g * 3], cb = a.conics[g * 3 + 1], cc = a.conics[g * 3 + 2];
            struct __attribute__((packed, aligned(4))) Q4 { float x, y, z, w; };
            const float* crow = a.colors + (int64_t)g * C;
            float rec[4 * REC4];
            rec[0] = x; rec[1] = y; rec[2] = op; rec[3] = ca; rec[4] = cb; rec[5] = cc;
#pragma unroll
            for (int c4 = 0; c4 + 4 <= C; c4 += 4) {
                const Q4 q = *reinterpret_cast<const Q4*>(crow + c4);
                rec[6 + c4] = q.x; rec[7 + c4] = q.y; rec[8 + c4] = q.z; rec[9 + c4] = q.w;
            }
#pragma unroll
            for (int c = C & ~3; c < C; ++c) rec[6 + c] = crow[c];
#pragma unroll
            for (int c = 6 + C; c < 4 * REC4; ++c) rec[c] = 0.f;
#pragma unroll
            for (int q = 0; q < REC4; ++q) s_rec[tr * REC4 + q] = make_float4(rec[4 * q], rec[4 * q + 1], rec[4 * q + 2], rec[4 * q + 3]);
            if (cull) s_mask[tr] = (uint8_t)raster_quad_mask(x, y, op, ca, cb, cc, tile_x0, tile_y0);
        }
        __syncthreads();
        const int bsz = min(256, r1 - start);
        int n_mine = bsz;
        if (cull) {   // this wave's (order-preserving) list of the staged splats its quadrant can see
            n_mine = 0;
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                const int t = ch * 64 + lane;
                const bool need = t < bsz && ((s_mask[t] >> wv) & 1u);
                const uint64_t m = __builtin_amdgcn_ballot_w64(need);
                if (need) s_list[wv][n_mine + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = (uint16_t)t;
                n_mine += __builtin_popcountll(m);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the list is read back by this wave only
            __builtin_amdgcn_wave_barrier();
        }
        // Hand-pipelined walk, two splats per trip: the record of splat k + 1 and the list entries of k + 2, k + 3 are requested
        // before splat k is blended, so no blend waits for an LDS round trip (the chain list entry -> record -> colours was three
        // of them per visited splat, on the critical path of the tile's slowest quadrant).
        struct Rec { float v[4 * REC4]; };
        auto load_rec = [&](int t, Rec& r) {
#pragma unroll
            for (int q = 0; q < REC4; ++q) {
                const float4 w = s_rec[t * REC4 + q];
                r.v[4 * q] = w.x; r.v[4 * q + 1] = w.y; r.v[4 * q + 2] = w.z; r.v[4 * q + 3] = w.w;
            }
        };
        auto entry = [&](int k) { const int kk = k < n_mine ? k : n_mine - 1; return cull ? (int)s_list[wv][kk] : kk; };
        auto blend = [&](const Rec& r, int t) {
            if (!done) {
                if (BOUNDED && start + t > stop) {   // past this pixel's last blended splat of the first pass
                    done = true;
                } else {
                    float dx = r.v[0] - px, dy = r.v[1] - py, op = r.v[2];
                    float ca = r.v[3], cb = r.v[4], cc = r.v[5];
                    float sigma = 0.5f * (ca * dx * dx + cc * dy * dy) + cb * dx * dy;
                    float alpha = fminf(0.999f, op * __expf(-sigma));
                    if (!(sigma < 0.f || alpha < 1.f / 255.f)) {
                        float nT = T * (1.f - alpha);
                        if (!BOUNDED && nT <= 1e-4f) {
                            done = true;
                        } else {
                            float vis = alpha * T;
#pragma unroll
                            for (int c = 0; c < C; ++c) pix[c] += r.v[6 + c] * vis;
                            T = nT;
                            cur_idx = start + t;
                        }
                    }
                }
            }
        };
        if (n_mine > 0) {
            Rec ra, rb;
            int ta = entry(0), tb = entry(1);
            load_rec(ta, ra);
            for (int k = 0; k < n_mine; k += 2) {
                if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;     // uniform: every pixel of this wave has finished
                load_rec(tb, rb);
                const int ta2 = entry(k + 2), tb2 = entry(k + 3);
                blend(ra, ta);
                load_rec(ta2, ra);
                if (k + 1 < n_mine) blend(rb, tb);
                ta = ta2;
                tb = tb2;
            }
        }
    }
    float vmax = 0.f;
    if (inside) {
        a.finalT[p] = T;
        if (a.final_idx) a.final_idx[p] = cur_idx;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float v = pix[c] + T * (a.bg ? a.bg[c] : 0.f);
            a.out[p * C + c] = v;
            if (c == a.max_ch) vmax = v;
        }
    }
    // The `img.max()` that the alpha normalisation of this channel needs (depth_im.detach().max(), :319 / :356) is
    // taken here, where the values are in registers: one compare per wave, and an atomic only from a wave that raises
    // the maximum (a separate reduction kernel cost 28 us per pass).
    if (a.chan_max) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, m, 64));
        if (lane == 0) {
            const unsigned int bits = __float_as_uint(fmaxf(vmax, 0.f));   // >= 0: bit patterns order like the values
            if (bits > __hip_atomic_load(a.chan_max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(a.chan_max, bits);
        }
    }
}

static int splat_rasterize_impl(const char* what, int B, const int32_t* gaussian_ids_sorted, const int32_t* tile_bins, const float* xys,
                                const float* conics, const float* colors, const float* opacities, const float* background, int C,
                                int H, int W, int block_width, const int32_t* stop_idx, int flags, int max_channel, float* chan_max,
                                float* out_img, float* final_T, int32_t* final_idx, void* stream) {
    UNERF_REQUIRE(tile_bins && xys && conics && colors && opacities && out_img && final_T,
                  "%s: null pointer", what);
    UNERF_REQUIRE(C >= 1 && C <= 8, "%s: C=%d outside [1,8]", what, C);
    UNERF_REQUIRE(block_width >= 1 && block_width <= 16 && H > 0 && W > 0, "%s: bad block_width/H/W", what);
    UNERF_REQUIRE((flags & ~UNERF_RASTER_NO_CULL) == 0, "%s: unknown flags %d", what, flags);
    UNERF_REQUIRE(!chan_max || (max_channel >= 0 && max_channel < C), "%s: max_channel %d outside [0,%d)", what,
                  max_channel, C);
    RasterArgs a;
    a.ids = gaussian_ids_sorted; a.bins = tile_bins; a.xys = xys; a.conics = conics; a.colors = colors;
    a.opac = opacities; a.bg = background; a.H = H; a.W = W; a.bw = block_width; a.out = out_img; a.finalT = final_T;
    a.final_idx = final_idx; a.stop_idx = stop_idx; a.cull = (flags & UNERF_RASTER_NO_CULL) ? 0 : 1;
    a.chan_max = reinterpret_cast<unsigned int*>(chan_max); a.max_ch = chan_max ? max_channel : -1;
    dim3 grid((W + block_width - 1) / block_width, (H + block_width - 1) / block_width, B), block(256);
    hipStream_t st = (hipStream_t)stream;
#define UNERF_RASTER_CASE(N)                                                                       \
    case N:                                                                                        \
        if (stop_idx) hipLaunchKernelGGL((raster_kernel<N, true>), grid, block, 0, st, a);         \
        else hipLaunchKernelGGL((raster_kernel<N, false>), grid, block, 0, st, a);                 \
        break;
    switch (C) {
        UNERF_RASTER_CASE(1)
        UNERF_RASTER_CASE(2)
        UNERF_RASTER_CASE(3)
        UNERF_RASTER_CASE(4)
        UNERF_RASTER_CASE(5)
        UNERF_RASTER_CASE(6)
        UNERF_RASTER_CASE(7)
        default:
            if (stop_idx) hipLaunchKernelGGL((raster_kernel<8, true>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((raster_kernel<8, false>), grid, block, 0, st, a);
            break;
    }
#undef UNERF_RASTER_CASE
    return unerf_check_launch(what);
}

extern "C" int unerf_splat_rasterize(const int32_t* gaussian_ids_sorted, const int32_t* tile_bins, const float* xys,
                                     const float* conics, const float* colors, const float* opacities,
                                     const float* background, int C, int H, int W, int block_width,
                                     const int32_t* stop_idx, int flags, int max_channel, float* chan_max, float* out_img,
                                     float* final_T, int32_t* final_idx, void* stream) {
    return splat_rasterize_impl("splat_rasterize", 1, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background, C, H,
                                W, block_width, stop_idx, flags, max_channel, chan_max, out_img, final_T, final_idx, stream);
}

extern "C" int unerf_splat_rasterize_batch(const int32_t* gaussian_ids_sorted, const int32_t* tile_bins, const float* xys,
                                           const float* conics, const float* colors, const float* opacities,
                                           const float* background, int B, int C, int H, int W, int block_width,
                                           const int32_t* stop_idx, int flags, int max_channel, float* chan_max,
                                           float* out_img, float* final_T, int32_t* final_idx, void* stream) {
    UNERF_REQUIRE(B >= 1 && B <= UNERF_SPLAT_MAX_VIEWS, "splat_rasterize_batch: B=%d outside [1,%d]", B, UNERF_SPLAT_MAX_VIEWS);
    return splat_rasterize_impl("splat_rasterize_batch", B, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background,
                                C, H, W, block_width, stop_idx, flags, max_channel, chan_max, out_img, final_T, final_idx, stream);
}

// ======================================================================================
// alpha normalisation and per-splat depth difference
// ======================================================================================
// grid-stride max with one atomic per workgroup (one per wave cost 370 us on a 1080p image: 32 K atomics
// serialise on a single L2 word)
__global__ __launch_bounds__(256) void chan_max_kernel(const float* __restrict__ img, int stride, int ch, int64_t HW,
                                                       unsigned int* __restrict__ mx) {
    __shared__ float s_max[4];
    float v = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (int64_t)gridDim.x * 256)
        v = fmaxf(v, img[i * stride + ch]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        v = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
        const unsigned int bits = __float_as_uint(v);  // v >= 0: bit patterns order like the values
        if (bits > __hip_atomic_load(mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(mx, bits);
    }
}

__global__ __launch_bounds__(256) void alpha_norm_kernel(float* __restrict__ img, int stride, int ch,
                                                         const float* __restrict__ finalT, int64_t HW,
                                                         const float* __restrict__ mx) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    float alpha = 1.f - finalT[i];
    float v = img[i * stride + ch];
    img[i * stride + ch] = (alpha > 0.f) ? v / alpha : mx[0];
}

extern "C" int unerf_splat_alpha_normalize(float* img, int stride, int ch, const float* final_T, int64_t HW,
                                           float* scratch_max, int max_ready, void* stream) {
    UNERF_REQUIRE(img && final_T && scratch_max, "splat_alpha_normalize: null pointer");
    UNERF_REQUIRE(stride >= 1 && ch >= 0 && ch < stride && HW >= 0, "splat_alpha_normalize: bad stride/ch");
    if (HW == 0) return UNERF_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!max_ready) {   // otherwise the rasteriser that produced img left the channel's maximum in scratch_max
        if (hipMemsetAsync(scratch_max, 0, sizeof(float), st) != hipSuccess)
            return unerf_check_launch("splat_alpha_normalize memset");
        const unsigned max_blocks = 2048;  // 8 workgroups per CU
        const unsigned nblk = blocks_for(HW, 256) < max_blocks ? blocks_for(HW, 256) : max_blocks;
        hipLaunchKernelGGL(chan_max_kernel, dim3(nblk), dim3(256), 0, st, img, stride, ch, HW,
                           reinterpret_cast<unsigned int*>(scratch_max));
    }
    hipLaunchKernelGGL(alpha_norm_kernel, dim3(blocks_for(HW, 256)), dim3(256), 0, st, img, stride, ch, final_T, HW,
                       scratch_max);
    return unerf_check_launch("splat_alpha_normalize");
}

// the frame's per-pixel epilogue in one pass (unerf_splat_normalize_outputs): the alpha normalisation of channel ch as above
// plus the elementwise outputs the reference forms with torch calls around it
__global__ __launch_bounds__(256) void norm_outputs_kernel(float* __restrict__ img, int stride, int ch,
                                                           const float* __restrict__ finalT, int64_t HW,
                                                           const float* __restrict__ mx, float* __restrict__ rgb_out,
                                                           float* __restrict__ acc_out, int sq_ch, float* __restrict__ sq_out,
                                                           float* __restrict__ sqrt_out) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    {   // view blockIdx.y of a batch: its image, transmittances, outputs and maximum
        const int64_t vw = blockIdx.y;
        img += vw * HW * stride; finalT += vw * HW; mx += vw;
        if (rgb_out) rgb_out += vw * HW * 3;
        if (acc_out) acc_out += vw * HW;
        if (sq_out) sq_out += vw * HW;
        if (sqrt_out) sqrt_out += vw * HW;
    }
    const float alpha = 1.f - finalT[i];
    const float v = img[i * stride + ch];
    const float nv = (alpha > 0.f) ? v / alpha : mx[0];
    img[i * stride + ch] = nv;
    if (rgb_out) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float x = img[i * stride + c];
            rgb_out[i * 3 + c] = x > 1.f ? 1.f : x;      // torch.clamp(max=1): a NaN stays a NaN
        }
    }
    if (acc_out) acc_out[i] = alpha;
    if (sq_out) {
        const float u = img[i * stride + sq_ch];
        sq_out[i] = u * u;
    }
    if (sqrt_out) sqrt_out[i] = sqrtf(nv);
}

extern "C" int unerf_splat_normalize_outputs(float* img, int stride, int ch, const float* final_T, int64_t HW,
                                             const float* scratch_max, float* rgb_out, float* acc_out, int sq_ch,
                                             float* sq_out, float* sqrt_out, void* stream) {
    UNERF_REQUIRE(img && final_T && scratch_max, "splat_normalize_outputs: null pointer");
    UNERF_REQUIRE(stride >= 1 && ch >= 0 && ch < stride && HW >= 0, "splat_normalize_outputs: bad stride/ch");
    UNERF_REQUIRE(!rgb_out || (stride >= 3 && ch >= 3), "splat_normalize_outputs: rgb_out needs channels 0..2 beside channel ch");
    UNERF_REQUIRE(!sq_out || (sq_ch >= 0 && sq_ch < stride && sq_ch != ch), "splat_normalize_outputs: bad sq_ch");
    if (HW == 0) return UNERF_OK;
    hipLaunchKernelGGL(norm_outputs_kernel, dim3(blocks_for(HW, 256)), dim3(256), 0, (hipStream_t)stream, img, stride, ch, final_T, HW,
                       scratch_max, rgb_out, acc_out, sq_ch, sq_out, sqrt_out);
    return unerf_check_launch("splat_normalize_outputs");
}

extern "C" int unerf_splat_normalize_outputs_batch(float* img, int stride, int ch, const float* final_T, int B, int64_t HW,
                                                   const float* scratch_max, float* rgb_out, float* acc_out, int sq_ch,
                                                   float* sq_out, float* sqrt_out, void* stream) {
    UNERF_REQUIRE(img && final_T && scratch_max, "splat_normalize_outputs_batch: null pointer");
    UNERF_REQUIRE(B >= 1 && B <= UNERF_SPLAT_MAX_VIEWS, "splat_normalize_outputs_batch: B=%d outside [1,%d]", B, UNERF_SPLAT_MAX_VIEWS);
    UNERF_REQUIRE(stride >= 1 && ch >= 0 && ch < stride && HW >= 0, "splat_normalize_outputs_batch: bad stride/ch");
    UNERF_REQUIRE(!rgb_out || (stride >= 3 && ch >= 3), "splat_normalize_outputs_batch: rgb_out needs channels 0..2 beside channel ch");
    UNERF_REQUIRE(!sq_out || (sq_ch >= 0 && sq_ch < stride && sq_ch != ch), "splat_normalize_outputs_batch: bad sq_ch");
    if (HW == 0) return UNERF_OK;
    hipLaunchKernelGGL(norm_outputs_kernel, dim3(blocks_for(HW, 256), B), dim3(256), 0, (hipStream_t)stream, img, stride, ch, final_T, HW,
                       scratch_max, rgb_out, acc_out, sq_ch, sq_out, sqrt_out);
    return unerf_check_launch("splat_normalize_outputs_batch");
}

__global__ __launch_bounds__(256) void depth_sqdiff_kernel(const float* __restrict__ xys,
                                                           const float* __restrict__ depths,
                                                           const float* __restrict__ dimg, int stride, int ch, int H,
                                                           int W, int64_t N, float* __restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    {   // view blockIdx.y of a batch: its splats and its depth image
        const int64_t vw = blockIdx.y;
        xys += vw * N * 2; depths += vw * N; out += vw * N;
        dimg += vw * H * (int64_t)W * stride;
    }
    float fxp = floorf(xys[i * 2]), fyp = floorf(xys[i * 2 + 1]);
    float z = depths[i];
    // reference uses strict ">0" on both axes (activesplatfacto_model.py:327-332)
    bool valid = fxp > 0.f && fxp < (float)W && fyp > 0.f && fyp < (float)H;
    float d = z;
    if (valid) d = z - dimg[((int64_t)fyp * W + (int64_t)fxp) * stride + ch];
    out[i] = d * d;
}

extern "C" int unerf_splat_depth_sqdiff(const float* xys, const float* depths, const float* depth_img, int stride,
                                        int ch, int H, int W, int64_t N, float* sq_diff_out, void* stream) {
    UNERF_REQUIRE(N <= 0 || (xys && depths && depth_img && sq_diff_out), "splat_depth_sqdiff: null pointer");
    UNERF_REQUIRE(stride >= 1 && ch >= 0 && ch < stride, "splat_depth_sqdiff: bad stride/ch");
    if (N <= 0) return UNERF_OK;
    hipLaunchKernelGGL(depth_sqdiff_kernel, dim3(blocks_for(N, 256)), dim3(256), 0, (hipStream_t)stream, xys, depths,
                       depth_img, stride, ch, H, W, N, sq_diff_out);
    return unerf_check_launch("splat_depth_sqdiff");
}

extern "C" int unerf_splat_depth_sqdiff_batch(const float* xys, const float* depths, const float* depth_img, int stride, int ch,
                                              int B, int H, int W, int64_t N, float* sq_diff_out, void* stream) {
    UNERF_REQUIRE(N <= 0 || (xys && depths && depth_img && sq_diff_out), "splat_depth_sqdiff_batch: null pointer");
    UNERF_REQUIRE(B >= 1 && B <= UNERF_SPLAT_MAX_VIEWS, "splat_depth_sqdiff_batch: B=%d outside [1,%d]", B, UNERF_SPLAT_MAX_VIEWS);
    UNERF_REQUIRE(stride >= 1 && ch >= 0 && ch < stride && H > 0 && W > 0, "splat_depth_sqdiff_batch: bad stride/ch/H/W");
    if (N <= 0) return UNERF_OK;
    hipLaunchKernelGGL(depth_sqdiff_kernel, dim3(blocks_for(N, 256), B), dim3(256), 0, (hipStream_t)stream, xys, depths,
                       depth_img, stride, ch, H, W, N, sq_diff_out);
    return unerf_check_launch("splat_depth_sqdiff_batch");
}

// ======================================================================================
// per-pixel camera-pose gradient of a frame, forward mode
// ======================================================================================
// s = mean_c clamp(pix_c + T_end bg_c, max = 1) of a pixel depends on the pose only through each splat's projected
// q = (u, v, conic a, b, c, compensation): the SH view directions are detached (activesplatfacto_model.py:243) and radii,
// lists, skips and stops are locally constant.  splat_pose_tangents_kernel writes dq / dV for the 12 entries of V[:3,:4];
// splat_pose_grad_kernel walks the tile lists as raster_kernel does and carries dT[12], dpix[3][12] next to T, pix[3].
struct PoseTanArgs {
    const float* means;
    const float* cov3d;
    const int32_t* radii;
    int64_t N;
    float V[12];
    float fx, fy, cx, cy;
    int H, W;
    float clip;
    float* tan;
};

// the arithmetic of project_kernel behind `cov3d`, with the tangent of every intermediate for a unit change of V[r][c]: the six
// tangent rows out[q][k], k = 4 r + c, of one live splat (splat_pose_tangents_kernel stores them, splat_pose_ptangents_batch_kernel
// contracts them in registers)
__device__ __forceinline__ void pose_tangent_rows(const float* V, float fx, float fy, int H, int W, const float (&m)[4], float tx,
                                                  float ty, float tz, const float* cv, float (&out)[UNERF_SPLAT_POSE_Q][12]) {
    const float C3[9] = {cv[0], cv[1], cv[2], cv[1], cv[3], cv[4], cv[2], cv[4], cv[5]};
    const float lim_x = 1.3f * (0.5f * (float)W / fx), lim_y = 1.3f * (0.5f * (float)H / fy);
    const float rx = tx / tz, ry = ty / tz;
    // torch.clamp's derivative: 1 on [-lim, lim] (the ends included), 0 outside
    const bool clamp_x = rx > lim_x || rx < -lim_x, clamp_y = ry > lim_y || ry < -lim_y;
    const float cxr = fminf(lim_x, fmaxf(-lim_x, rx)), cyr = fminf(lim_y, fmaxf(-lim_y, ry));
    const float ex = tz * cxr, ey = tz * cyr;
    const float rz = 1.f / tz, rz2 = rz * rz;
    const float J00 = fx * rz, J02 = (-fx * ex) * rz2, J11 = fy * rz, J12 = (-fy * ey) * rz2;
    float T0[3], T1[3], TV0[3], TV1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        T0[c] = J00 * V[c] + J02 * V[8 + c];
        T1[c] = J11 * V[4 + c] + J12 * V[8 + c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        TV0[c] = (T0[0] * C3[c] + T0[1] * C3[3 + c]) + T0[2] * C3[6 + c];
        TV1[c] = (T1[0] * C3[c] + T1[1] * C3[3 + c]) + T1[2] * C3[6 + c];
    }
    const float c00 = (TV0[0] * T0[0] + TV0[1] * T0[1]) + TV0[2] * T0[2];
    const float c01 = (TV0[0] * T1[0] + TV0[1] * T1[1]) + TV0[2] * T1[2];
    const float c11 = (TV1[0] * T1[0] + TV1[1] * T1[1]) + TV1[2] * T1[2];
    const float det_orig = c00 * c11 - c01 * c01;
    const float ca = c00 + 0.3f, cb = c01, cc = c11 + 0.3f;
    const float det = ca * cc - cb * cb;
    const float inv_det = 1.f / det, inv_det2 = inv_det * inv_det;
    const float ratio = det_orig / det;
    const float comp = sqrtf(fmaxf(0.f, ratio));
    const bool comp_live = det_orig > 0.f && ratio > 0.f;
    const float rw = 1.f / (tz + 1e-6f), rw2 = rw * rw;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const int r = k >> 2, c = k & 3;           // the entry V[r][c] moves
        const float dtx = r == 0 ? m[c] : 0.f, dty = r == 1 ? m[c] : 0.f, dtz = r == 2 ? m[c] : 0.f;
        const float dex = clamp_x ? dtz * cxr : dtx, dey = clamp_y ? dtz * cyr : dty;
        const float drz = -rz2 * dtz, drz2 = 2.f * rz * drz;
        const float dJ00 = fx * drz, dJ11 = fy * drz;
        const float dJ02 = -fx * (dex * rz2 + ex * drz2), dJ12 = -fy * (dey * rz2 + ey * drz2);
        float dT0[3], dT1[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            dT0[j] = dJ00 * V[j] + dJ02 * V[8 + j];
            dT1[j] = dJ11 * V[4 + j] + dJ12 * V[8 + j];
            if (c == j) {                          // (c == 3: the translation column enters through t only)
                if (r == 0) dT0[j] += J00;
                if (r == 1) dT1[j] += J11;
                if (r == 2) { dT0[j] += J02; dT1[j] += J12; }
            }
        }
        const float dc00 = 2.f * ((TV0[0] * dT0[0] + TV0[1] * dT0[1]) + TV0[2] * dT0[2]);
        const float dc11 = 2.f * ((TV1[0] * dT1[0] + TV1[1] * dT1[1]) + TV1[2] * dT1[2]);
        const float dc01 = ((TV1[0] * dT0[0] + TV1[1] * dT0[1]) + TV1[2] * dT0[2])
                         + ((TV0[0] * dT1[0] + TV0[1] * dT1[1]) + TV0[2] * dT1[2]);
        const float ddet_orig = (dc00 * c11 + c00 * dc11) - 2.f * c01 * dc01;
        const float ddet = (dc00 * cc + ca * dc11) - 2.f * cb * dc01;
        out[0][k] = fx * (dtx * rw - tx * rw2 * dtz);
        out[1][k] = fy * (dty * rw - ty * rw2 * dtz);
        out[2][k] = dc11 * inv_det - cc * ddet * inv_det2;
        out[3][k] = cb * ddet * inv_det2 - dc01 * inv_det;
        out[4][k] = dc00 * inv_det - ca * ddet * inv_det2;
        out[5][k] = comp_live ? (0.5f / comp) * (ddet_orig * inv_det - det_orig * ddet * inv_det2) : 0.f;
    }
}

__global__ __launch_bounds__(256) void splat_pose_tangents_kernel(PoseTanArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    float out[UNERF_SPLAT_POSE_Q][12];
#pragma unroll
    for (int q = 0; q < UNERF_SPLAT_POSE_Q; ++q)
#pragma unroll
        for (int k = 0; k < 12; ++k) out[q][k] = 0.f;
    float4* row = reinterpret_cast<float4*>(a.tan + i * (int64_t)(UNERF_SPLAT_POSE_Q * 12));
    const float* V = a.V;
    const float m[4] = {a.means[i * 3], a.means[i * 3 + 1], a.means[i * 3 + 2], 1.f};
    const float tx = ((V[0] * m[0] + V[1] * m[1]) + V[2] * m[2]) + V[3];
    const float ty = ((V[4] * m[0] + V[5] * m[1]) + V[6] * m[2]) + V[7];
    const float tz = ((V[8] * m[0] + V[9] * m[1]) + V[10] * m[2]) + V[11];
    if (a.radii[i] != 0 && !(tz <= a.clip)) pose_tangent_rows(V, a.fx, a.fy, a.H, a.W, m, tx, ty, tz, a.cov3d + i * 6, out);
#pragma unroll
    for (int q = 0; q < UNERF_SPLAT_POSE_Q; ++q)
#pragma unroll
        for (int w = 0; w < 3; ++w) row[q * 3 + w] = make_float4(out[q][4 * w], out[q][4 * w + 1], out[q][4 * w + 2], out[q][4 * w + 3]);
}

extern "C" int unerf_splat_pose_tangents(const float* means3d, const float* cov3d, const int32_t* radii, int64_t N,
                                         const float* viewmat_host, float fx, float fy, float cx, float cy, int H, int W,
                                         float clip_thresh, float* tangents, void* stream) {
    UNERF_REQUIRE(viewmat_host && (N <= 0 || (means3d && cov3d && radii && tangents)), "splat_pose_tangents: null pointer");
    UNERF_REQUIRE(H > 0 && W > 0 && N >= 0, "splat_pose_tangents: bad H/W/N");
    UNERF_REQUIRE((reinterpret_cast<uintptr_t>(tangents) & 15) == 0, "splat_pose_tangents: tangents must be 16-byte aligned");
    if (N == 0) return UNERF_OK;
    PoseTanArgs a;
    a.means = means3d; a.cov3d = cov3d; a.radii = radii; a.N = N;
    for (int k = 0; k < 12; ++k) a.V[k] = viewmat_host[k];
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.H = H; a.W = W; a.clip = clip_thresh; a.tan = tangents;
    hipLaunchKernelGGL(splat_pose_tangents_kernel, dim3(blocks_for(N, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return unerf_check_launch("splat_pose_tangents");
}

// ---- the stages of the forward-mode walk, stated once for splat_pose_grad_kernel and pose_jac_walk ------------------------------
// (raster_kernel keeps its own copy of the pixel mapping, the staging and the list: it is the kernel bench.py times, and its
// compiled code is held byte for byte.)  Pointers, scalars and small structs by value: a by-reference argument struct moved the
// callers' registers.

// A row of PW = 6 or 12 running tangents is three vectors of PoseVec<PW>::T.
template <int PW> struct PoseVec;
template <> struct PoseVec<6> { using T = float2; static constexpr int W = 2; };
template <> struct PoseVec<12> { using T = float4; static constexpr int W = 4; };
__device__ __forceinline__ float pose_vec_get(const float2& v, int e) { return e == 0 ? v.x : v.y; }
__device__ __forceinline__ float pose_vec_get(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
__device__ __forceinline__ void pose_vec_set(float2& v, const float* s) { v = make_float2(s[0], s[1]); }
__device__ __forceinline__ void pose_vec_set(float4& v, const float* s) { v = make_float4(s[0], s[1], s[2], s[3]); }

// raster_kernel's thread-to-pixel mapping, its statements for ly, lx, i, j, px, py, inside and p: a wave is one 8 x 8 quadrant
// of a 16-wide tile, narrower tiles are row-major
struct PosePixel { float px, py; bool inside; int64_t p; };
__device__ __forceinline__ PosePixel pose_walk_pixel(int tr, int bx, int by, int bw, int H, int W) {
    const int ly = bw == 16 ? 8 * (tr >> 7) + ((tr & 63) >> 3) : tr / bw;
    const int lx = bw == 16 ? 8 * ((tr >> 6) & 1) + (tr & 7) : tr - (tr / bw) * bw;
    const int i = by * bw + ly, j = bx * bw + lx;
    PosePixel q;
    q.px = (float)j + 0.5f; q.py = (float)i + 0.5f;
    q.inside = (ly < bw) && (i < H) && (j < W);
    q.p = (int64_t)i * W + j;
    return q;
}

// The per-splat arrays a staged header is read from (depths: read by the walks that carry the depth sum).
struct PoseSplatIn {
    const int32_t* ids;
    const float *xys, *opac, *conics, *colors, *comp, *depths;
};

// Thread tr stages list entry `at`: raster_kernel's loads of a splat's x, y, opacity and conic, and its quadrant mask, into the
// three header words [x, y, o, a | b, c, r, g | b, 1 / comp, z, -] at rec[tr * rec4] (AA: the staged opacity is sigmoid(.) comp,
// and alpha's tangent needs 1 / comp; DEPTH: z, else 0), the splat's id into s_gid for the staging of its tangent rows.
// cstride: floats per colour row.
template <bool AA, bool DEPTH>
__device__ __forceinline__ void pose_stage_header(PoseSplatIn in, int at, int cstride, float4* rec, int rec4, int32_t* s_gid,
                                                  uint8_t* s_mask, int tr, bool cull, float tile_x0, float tile_y0) {
    const int g = in.ids[at];
    const float x = in.xys[g * 2], y = in.xys[g * 2 + 1], op = in.opac[g];
    const float ca = in.conics[g * 3], cb = in.conics[g * 3 + 1], cc = in.conics[g * 3 + 2];
    const float* crow = in.colors + (int64_t)g * cstride;
    rec[tr * rec4] = make_float4(x, y, op, ca);
    rec[tr * rec4 + 1] = make_float4(cb, cc, crow[0], crow[1]);
    rec[tr * rec4 + 2] = make_float4(crow[2], AA ? 1.f / in.comp[g] : 1.f, DEPTH ? in.depths[g] : 0.f, 0.f);
    s_gid[tr] = g;
    if (cull) s_mask[tr] = (uint8_t)raster_quad_mask(x, y, op, ca, cb, cc, tile_x0, tile_y0);
}

// raster_kernel's list statements on a batch of PG: n_mine = the number of staged splats wave wv's quadrant can see (s_mask bit
// wv), their indices in s_list[wv]: an order-preserving list, the blend is front to back.  The list is per wave because a wave is one
// quadrant: it is written and read back by the same wave, so a wave-level fence and barrier are all it needs.  A macro: as a
// function (the list by pointer or by reference, n_mine returned or assigned) it cost all ten kernels two SGPRs.
#define UNERF_POSE_QUADRANT_LIST(n_mine, s_mask, s_list, bsz, wv, lane, PG)                                              \
    {                                                                                                                    \
        (n_mine) = 0;                                                                                                    \
        _Pragma("unroll") for (int ch = 0; ch < (PG) / 64; ++ch) {                                                       \
            const int t = ch * 64 + (lane);                                                                              \
            const bool need = t < (bsz) && (((s_mask)[t] >> (wv)) & 1u);                                                 \
            const uint64_t mm = __builtin_amdgcn_ballot_w64(need);                                                       \
            if (need) (s_list)[wv][(n_mine) + __builtin_popcountll(mm & ((1ull << (lane)) - 1ull))] = (uint16_t)t;       \
            (n_mine) += __builtin_popcountll(mm);                                                                        \
        }                                                                                                                \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                                                           \
        __builtin_amdgcn_wave_barrier();                                                                                 \
    }

// raster_kernel's decisions, on its expressions: the statements of its `blend` lambda from dx, dy to the test of nT (the
// unbounded pass), so the walk skips, blends and stops at exactly the pairs the frame did.  A pixel that is done decides nothing.
// clamped: alpha sits on the 0.999 cap, where its derivative -- and with it the splat's own tangent ad -- is 0; the splat still
// blends, and still carries the tangents of the transmittance in front of it.
struct PoseBlend { float alpha, nT, dx, dy; bool clamped, blend, done; };
__device__ __forceinline__ PoseBlend pose_blend_decision(float4 h0, float4 h1, float px, float py, float T, bool done) {
    PoseBlend r;
    r.alpha = 0.f; r.nT = T; r.dx = 0.f; r.dy = 0.f; r.clamped = false; r.blend = false; r.done = done;
    if (!done) {
        r.dx = h0.x - px; r.dy = h0.y - py;
        const float op = h0.z, ca = h0.w, cb = h1.x, cc = h1.y;
        const float sigma = 0.5f * (ca * r.dx * r.dx + cc * r.dy * r.dy) + cb * r.dx * r.dy;
        const float raw = op * __expf(-sigma);
        r.alpha = fminf(0.999f, raw);
        r.clamped = raw > 0.999f;
        if (!(sigma < 0.f || r.alpha < 1.f / 255.f)) {
            r.nT = T * (1.f - r.alpha);
            if (r.nT <= 1e-4f) r.done = true;
            else r.blend = true;
        }
    }
    return r;
}

// -d sigma = -(wx dx' + wy dy' + wa a' + wb b' + wc c') for the tangents x', y' of the centre and a', b', c' of the conic
struct PoseWeights { float wx, wy, wa, wb, wc; };
__device__ __forceinline__ PoseWeights pose_sigma_weights(float ca, float cb, float cc, float dx, float dy) {
    PoseWeights w;
    w.wx = ca * dx + cb * dy; w.wy = cc * dy + cb * dx;
    w.wa = 0.5f * dx * dx; w.wb = dx * dy; w.wc = 0.5f * dy * dy;
    return w;
}

// One blended splat's step of the running tangents: sd -> ad -> wk -> dpix, (dD,) dT in the PW directions.  tq: the splat's staged
// rows x, y, a, b, c (, comp: AA), three vectors each; inv_comp: the header's 1 / comp; DEPTH: the depth sum's tangents dD as well,
// with the depth row at tq[zrow].  Every lane reads the rows (the reads are uniform), a lane that blends uses them.
template <bool AA, bool DEPTH, int PW>
__device__ __forceinline__ void pose_tangent_step(const typename PoseVec<PW>::T* tq, int zrow, PoseBlend bl, PoseWeights wt, float T,
                                                  float inv_comp, const float (&col)[3], float z, float vis, float (&dT)[PW],
                                                  float (&dpix)[3][PW], float* dD) {
    using VT = typename PoseVec<PW>::T;
    constexpr int VW = PoseVec<PW>::W;
    const float om = 1.f - bl.alpha;
#pragma unroll
    for (int w = 0; w < 3; ++w) {
        const VT vx = tq[w], vy = tq[3 + w], va = tq[6 + w], vb = tq[9 + w], vc = tq[12 + w];
        VT vz = vx, vo = vx;
        if (DEPTH) vz = tq[zrow + w];
        if (AA) vo = tq[15 + w];
        if (bl.blend) {
#pragma unroll
            for (int e = 0; e < VW; ++e) {
                const int k = VW * w + e;
                const float sd = (((wt.wx * pose_vec_get(vx, e) + wt.wy * pose_vec_get(vy, e)) + wt.wa * pose_vec_get(va, e))
                                  + wt.wb * pose_vec_get(vb, e)) + wt.wc * pose_vec_get(vc, e);
                const float eo = AA ? pose_vec_get(vo, e) : 0.f;
                const float ad = bl.clamped ? 0.f : bl.alpha * (inv_comp * eo - sd);
                const float wk = ad * T + bl.alpha * dT[k];
                dpix[0][k] += col[0] * wk;
                dpix[1][k] += col[1] * wk;
                dpix[2][k] += col[2] * wk;
                if (DEPTH) dD[k] += z * wk + pose_vec_get(vz, e) * vis;
                dT[k] = dT[k] * om - T * ad;
            }
        }
    }
}

struct PoseGradArgs {
    const int32_t* ids;
    const int32_t* bins;
    const float* xys;
    const float* conics;
    const float* colors;
    const float* opac;
    const float* comp;
    const float* tan;
    const float* bg;
    int has_c2w;
    float c2w[12];
    int H, W, bw;
    int cull;
    float* grad;
    float* rgb;
    float* finalT;
};

// AA ("antialiased"): the staged opacity is sigmoid(.) comp, so alpha carries comp's tangent as well.
// A staged record is PG_REC4 16-byte words: [x, y, o, a | b, c, r, g | b, 1 / comp, -, - | the tangents of x, y, a, b, c (, comp),
// 12 floats each]; PG_BATCH records of the antialiased kind are 42 KiB, with the lists 43.6 KiB: two (and three) workgroups of a
// CU's 160 KiB.
template <bool AA>
__global__ __launch_bounds__(256) void splat_pose_grad_kernel(PoseGradArgs a) {
    constexpr int PG = UNERF_SPLAT_POSE_GRAD_BATCH;
    constexpr int NT = AA ? 6 : 5;               // tangent 12-vectors per splat
    constexpr int TQ = 3 * NT;                   // ... in 16-byte words
    constexpr int REC4 = 3 + TQ;
    __shared__ float4 s_rec[PG * REC4];
    __shared__ int32_t s_gid[PG];
    __shared__ uint8_t s_mask[PG];
    __shared__ uint16_t s_list[4][PG];
    const int bw = a.bw;
    const int tbx = (a.W + bw - 1) / bw;
    const int bx = blockIdx.x, by = blockIdx.y;
    const int tile = by * tbx + bx;
    const int tr = threadIdx.x;
    const PosePixel at = pose_walk_pixel(tr, bx, by, bw, a.H, a.W);
    const float px = at.px, py = at.py;
    const bool inside = at.inside;
    const int64_t p = at.p;
    bool done = !inside;
    const int r0 = a.bins[tile * 2], r1 = a.bins[tile * 2 + 1];
    const int nbatch = (r1 - r0 + PG - 1) / PG;
    const bool cull = a.cull && bw == 16;
    const int wv = __builtin_amdgcn_readfirstlane(tr >> 6), lane = tr & 63;
    const float tile_x0 = (float)(bx * bw), tile_y0 = (float)(by * bw);
    float T = 1.f, pix[3] = {0.f, 0.f, 0.f};
    float dT[12], dpix[3][12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { dT[k] = 0.f; dpix[0][k] = 0.f; dpix[1][k] = 0.f; dpix[2][k] = 0.f; }
    for (int b = 0; b < nbatch; ++b) {
        const int start = r0 + PG * b;
        if (__syncthreads_count(done ? 1 : 0) >= 256) break;
        const int bsz = min(PG, r1 - start);
        if (tr < bsz)
            pose_stage_header<AA, false>({a.ids, a.xys, a.opac, a.conics, a.colors, a.comp, nullptr}, start + tr, 3, s_rec, REC4, s_gid,
                                         s_mask, tr, cull, tile_x0, tile_y0);
        __syncthreads();
        // the tangent rows, 16 bytes per thread and trip (a row is UNERF_SPLAT_POSE_Q * 12 floats; comp's 12 are its last)
        for (int w = tr; w < bsz * TQ; w += 256) {
            const int rec = w / TQ, q = w - rec * TQ;
            s_rec[rec * REC4 + 3 + q] = reinterpret_cast<const float4*>(a.tan + (int64_t)s_gid[rec] * (UNERF_SPLAT_POSE_Q * 12))[q];
        }
        __syncthreads();
        int n_mine = bsz;
        if (cull) UNERF_POSE_QUADRANT_LIST(n_mine, s_mask, s_list, bsz, wv, lane, PG)
        for (int k0 = 0; k0 < n_mine; ++k0) {
            if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;     // uniform: every pixel of this wave has finished
            const int t = cull ? (int)s_list[wv][k0] : k0;
            const float4 h0 = s_rec[t * REC4], h1 = s_rec[t * REC4 + 1], h2 = s_rec[t * REC4 + 2];
            const PoseBlend bl = pose_blend_decision(h0, h1, px, py, T, done);
            done = bl.done;
            if (__builtin_amdgcn_ballot_w64(bl.blend) == 0ull) continue;  // uniform: nobody needs this splat's tangents
            const PoseWeights wt = pose_sigma_weights(h0.w, h1.x, h1.y, bl.dx, bl.dy);
            const float col[3] = {h1.z, h1.w, h2.x};
            pose_tangent_step<AA, false, 12>(&s_rec[t * REC4 + 3], 0, bl, wt, T, h2.y, col, 0.f, 0.f, dT, dpix, nullptr);
            if (bl.blend) {
                const float vis = bl.alpha * T;
                pix[0] += col[0] * vis; pix[1] += col[1] * vis; pix[2] += col[2] * vis;
                T = bl.nT;
            }
        }
    }
    if (!inside) return;
    float live[3], gV[12];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float bgc = a.bg ? a.bg[c] : 0.f;
        const float v = pix[c] + T * bgc;
        live[c] = v < 1.f ? 1.f : 0.f;           // clamp(max = 1): a saturated channel contributes nothing
        if (a.rgb) a.rgb[p * 3 + c] = fminf(v, 1.f);
    }
    if (a.finalT) a.finalT[p] = T;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) s += live[c] * (dpix[c][k] + (a.bg ? a.bg[c] : 0.f) * dT[k]);
        gV[k] = s * (1.f / 3.f);
    }
    float o[12];
    if (a.has_c2w) {
        // V = [R'^T | -R'^T t], R' = R diag(1, -1, -1):  ds/dt = -R' g_t,  ds/dR[r][c] = F_cc (G[c][r] - g_t[c] t[r])
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float tr_ = a.c2w[r * 4 + 3];
            float st = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float F = c == 0 ? 1.f : -1.f;
                o[r * 4 + c] = F * (gV[c * 4 + r] - gV[c * 4 + 3] * tr_);
                st += (F * a.c2w[r * 4 + c]) * gV[c * 4 + 3];
            }
            o[r * 4 + 3] = -st;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) o[k] = gV[k];
    }
    float4* orow = reinterpret_cast<float4*>(a.grad + p * 12);
#pragma unroll
    for (int w = 0; w < 3; ++w) orow[w] = make_float4(o[4 * w], o[4 * w + 1], o[4 * w + 2], o[4 * w + 3]);
}

extern "C" int unerf_splat_pose_grad(const int32_t* gaussian_ids_sorted, const int32_t* tile_bins, const float* xys,
                                     const float* conics, const float* colors, const float* opacities,
                                     const float* compensation, const float* tangents, const float* background,
                                     const float* c2w_host, int H, int W, int block_width, int flags, float* out_grad,
                                     float* out_rgb, float* final_T, void* stream) {
    UNERF_REQUIRE(gaussian_ids_sorted && tile_bins && xys && conics && colors && opacities && tangents && out_grad,
                  "splat_pose_grad: null pointer");
    UNERF_REQUIRE(block_width >= 1 && block_width <= 16 && H > 0 && W > 0, "splat_pose_grad: bad block_width/H/W");
    UNERF_REQUIRE((flags & ~UNERF_RASTER_NO_CULL) == 0, "splat_pose_grad: unknown flags %d", flags);
    UNERF_REQUIRE((reinterpret_cast<uintptr_t>(tangents) & 15) == 0 && (reinterpret_cast<uintptr_t>(out_grad) & 15) == 0,
                  "splat_pose_grad: tangents and out_grad must be 16-byte aligned");
    PoseGradArgs a;
    a.ids = gaussian_ids_sorted; a.bins = tile_bins; a.xys = xys; a.conics = conics; a.colors = colors; a.opac = opacities;
    a.comp = compensation; a.tan = tangents; a.bg = background;
    a.has_c2w = c2w_host ? 1 : 0;
    for (int k = 0; k < 12; ++k) a.c2w[k] = c2w_host ? c2w_host[k] : 0.f;
    a.H = H; a.W = W; a.bw = block_width; a.cull = (flags & UNERF_RASTER_NO_CULL) ? 0 : 1;
    a.grad = out_grad; a.rgb = out_rgb; a.finalT = final_T;
    const dim3 grid((W + block_width - 1) / block_width, (H + block_width - 1) / block_width), block(256);
    if (compensation) hipLaunchKernelGGL(splat_pose_grad_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(splat_pose_grad_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
    return unerf_check_launch("splat_pose_grad");
}

// ======================================================================================
// per-pixel pose Jacobian of a frame's five channels in P pose directions
// ======================================================================================
// The pose reaches a pixel linearly through the per-splat tangents, so the [12,P] projection is contracted per splat
// (splat_pose_tangents_proj_kernel) and the walk carries PW = 6 or 12 running tangents of each of T, pix[3] and the depth sum D.
// A row of PW floats is three vectors of PoseVec<PW>::T either way.

// ptangents rows are read as PoseVec<PW>::T: 8-byte aligned at PW = 6, 16-byte at PW = 12.  with_p: the message names P.
static int pose_ptangents_aligned(const char* what, const float* ptangents, int P, bool with_p = true) {
    const int bytes = UNERF_SPLAT_POSE_PW(P) == 6 ? 8 : 16;
    const bool ok = (reinterpret_cast<uintptr_t>(ptangents) & (uintptr_t)(bytes - 1)) == 0;
    if (with_p) UNERF_REQUIRE(ok, "%s: ptangents must be %d-byte aligned for P=%d", what, bytes, P);
    else UNERF_REQUIRE(ok, "%s: ptangents must be %d-byte aligned", what, bytes);
    return UNERF_OK;
}

struct PoseProjArgs {
    const float* tan;
    const float* means;
    const int32_t* radii;
    int64_t N;
    float proj[12 * UNERF_SPLAT_POSE_MAX_P];     // [12][PW], columns P .. PW-1 zero
    float* out;
};

// The contraction's two statements on the matrix entries MAT(k, p) -- the padded kernel argument of one view here, the view's
// device matrix in splat_pose_ptangents_batch_kernel: a row's sum over the entries of V in order, and the depth row
// z = V[2] . (m, 1).  Macros: stated as functions (by accessor, or by pointer and stride) they moved this kernel's registers
// (74 -> 60 VGPRs, 165 -> 0 spilled SGPRs at PW = 6), and the single-view kernels keep their compiled code.
#define UNERF_POSE_PROJ_ROW(o, t, MAT)                                              \
    _Pragma("unroll") for (int p = 0; p < PW; ++p) {                                \
        float s = (t)[0] * MAT(0, p);                                               \
        _Pragma("unroll") for (int k = 1; k < 12; ++k) s += (t)[k] * MAT(k, p);     \
        (o)[p] = s;                                                                 \
    }
#define UNERF_POSE_PROJ_DEPTH_ROW(o, live, m0, m1, m2, MAT)                         \
    _Pragma("unroll") for (int p = 0; p < PW; ++p)                                  \
        (o)[p] = (live) ? (((m0) * MAT(8, p) + (m1) * MAT(9, p)) + (m2) * MAT(10, p)) + MAT(11, p) : 0.f;

template <int PW>
__global__ __launch_bounds__(256) void splat_pose_tangents_proj_kernel(PoseProjArgs a) {
    using VT = typename PoseVec<PW>::T;
    constexpr int VW = PoseVec<PW>::W;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    VT* orow = reinterpret_cast<VT*>(a.out + i * (int64_t)(UNERF_SPLAT_POSE_PROJ_ROWS * PW));
    const float4* trow = reinterpret_cast<const float4*>(a.tan + i * (int64_t)(UNERF_SPLAT_POSE_Q * 12));
#define UNERF_POSE_MAT_ARG(k, p) a.proj[(k) * PW + (p)]
#pragma unroll
    for (int q = 0; q < UNERF_SPLAT_POSE_Q; ++q) {
        const float4 t0 = trow[q * 3], t1 = trow[q * 3 + 1], t2 = trow[q * 3 + 2];
        const float t[12] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w};
        float o[PW];
        UNERF_POSE_PROJ_ROW(o, t, UNERF_POSE_MAT_ARG)
#pragma unroll
        for (int w = 0; w < 3; ++w) pose_vec_set(orow[q * 3 + w], o + VW * w);
    }
    // the depth row: z = V[2] . (m, 1)
    float o[PW];
    const bool live = a.radii[i] != 0;
    const float m0 = a.means[i * 3], m1 = a.means[i * 3 + 1], m2 = a.means[i * 3 + 2];
    UNERF_POSE_PROJ_DEPTH_ROW(o, live, m0, m1, m2, UNERF_POSE_MAT_ARG)
#undef UNERF_POSE_MAT_ARG
#pragma unroll
    for (int w = 0; w < 3; ++w) pose_vec_set(orow[UNERF_SPLAT_POSE_Q * 3 + w], o + VW * w);
}

extern "C" int unerf_splat_pose_tangents_proj(const float* tangents, const float* means3d, const int32_t* radii, int64_t N,
                                              const float* proj_host, int P, float* ptangents, void* stream) {
    UNERF_REQUIRE(P >= 1 && P <= UNERF_SPLAT_POSE_MAX_P, "splat_pose_tangents_proj: P=%d outside [1,%d]", P, UNERF_SPLAT_POSE_MAX_P);
    UNERF_REQUIRE(N >= 0, "splat_pose_tangents_proj: bad N");
    UNERF_REQUIRE(proj_host && (N == 0 || (tangents && means3d && radii && ptangents)), "splat_pose_tangents_proj: null pointer");
    const int PW = UNERF_SPLAT_POSE_PW(P);
    UNERF_REQUIRE((reinterpret_cast<uintptr_t>(tangents) & 15) == 0, "splat_pose_tangents_proj: tangents must be 16-byte aligned");
    if (int rc = pose_ptangents_aligned("splat_pose_tangents_proj", ptangents, P, false)) return rc;
    if (N == 0) return UNERF_OK;
    PoseProjArgs a;
    a.tan = tangents; a.means = means3d; a.radii = radii; a.N = N; a.out = ptangents;
    for (int k = 0; k < 12; ++k)
        for (int p = 0; p < PW; ++p) a.proj[k * PW + p] = p < P ? proj_host[k * P + p] : 0.f;
    for (int k = 12 * PW; k < 12 * UNERF_SPLAT_POSE_MAX_P; ++k) a.proj[k] = 0.f;
    const dim3 grid(blocks_for(N, 256)), block(256);
    if (PW == 6) hipLaunchKernelGGL(splat_pose_tangents_proj_kernel<6>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(splat_pose_tangents_proj_kernel<12>, grid, block, 0, (hipStream_t)stream, a);
    return unerf_check_launch("splat_pose_tangents_proj");
}

// The two kernels above for B views in one launch, the 288-byte tangent row kept in registers: one thread per (view, splat)
// fills the six tangent rows (pose_tangent_rows) and contracts each with the view's [12,P] matrix (UNERF_POSE_PROJ_ROW), the statements
// and so the bits of the two kernels.  blockIdx.y is the view, so the camera and the matrix are wave-uniform (scalar loads); a
// culled splat runs the same sums on zeros.
struct PoseTanCam { float V[12]; float fx, fy; };
struct PosePtanBatchArgs {
    const float* means;
    const float* cov3d;
    const int32_t* radii;
    int64_t N;
    const float* proj;                           // [B,12,P] device
    int P, H, W;
    float clip;
    float* out;
    PoseTanCam cam[UNERF_SPLAT_MAX_VIEWS];
};

template <int PW>
__global__ __launch_bounds__(256) void splat_pose_ptangents_batch_kernel(PosePtanBatchArgs a) {
    using VT = typename PoseVec<PW>::T;
    constexpr int VW = PoseVec<PW>::W;
    const int v = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    const int64_t g = (int64_t)v * a.N + i;
    const int P = a.P;
    const float* __restrict__ pj = a.proj + (int64_t)v * 12 * P;
    const float* V = a.cam[v].V;
    float out[UNERF_SPLAT_POSE_Q][12];
#pragma unroll
    for (int q = 0; q < UNERF_SPLAT_POSE_Q; ++q)
#pragma unroll
        for (int k = 0; k < 12; ++k) out[q][k] = 0.f;
    const float m[4] = {a.means[i * 3], a.means[i * 3 + 1], a.means[i * 3 + 2], 1.f};
    const float tx = ((V[0] * m[0] + V[1] * m[1]) + V[2] * m[2]) + V[3];
    const float ty = ((V[4] * m[0] + V[5] * m[1]) + V[6] * m[2]) + V[7];
    const float tz = ((V[8] * m[0] + V[9] * m[1]) + V[10] * m[2]) + V[11];
    const bool live = a.radii[g] != 0;
    if (live && !(tz <= a.clip)) pose_tangent_rows(V, a.cam[v].fx, a.cam[v].fy, a.H, a.W, m, tx, ty, tz, a.cov3d + g * 6, out);
    VT* orow = reinterpret_cast<VT*>(a.out + g * (int64_t)(UNERF_SPLAT_POSE_PROJ_ROWS * PW));
    float o[PW];
#define UNERF_POSE_MAT_VIEW(k, p) ((p) < P ? pj[(k) * P + (p)] : 0.f)   /* uniform */
#pragma unroll
    for (int q = 0; q < UNERF_SPLAT_POSE_Q; ++q) {
        UNERF_POSE_PROJ_ROW(o, out[q], UNERF_POSE_MAT_VIEW)
#pragma unroll
        for (int w = 0; w < 3; ++w) pose_vec_set(orow[q * 3 + w], o + VW * w);
    }
    UNERF_POSE_PROJ_DEPTH_ROW(o, live, m[0], m[1], m[2], UNERF_POSE_MAT_VIEW)
#undef UNERF_POSE_MAT_VIEW
#pragma unroll
    for (int w = 0; w < 3; ++w) pose_vec_set(orow[UNERF_SPLAT_POSE_Q * 3 + w], o + VW * w);
}

extern "C" int unerf_splat_pose_ptangents_batch(const float* means3d, const float* cov3d, const int32_t* radii,
                                                const float* views_host, int B, int64_t N, const float* proj, int P, int H,
                                                int W, float clip_thresh, float* ptangents, void* stream) {
    UNERF_REQUIRE(B >= 1 && B <= UNERF_SPLAT_MAX_VIEWS, "splat_pose_ptangents_batch: B=%d outside [1,%d]", B, UNERF_SPLAT_MAX_VIEWS);
    UNERF_REQUIRE(N >= 0 && (int64_t)B * N < UNERF_SPLAT_MAX_BATCH_SPLATS, "splat_pose_ptangents_batch: B*N = %lld outside [0,2^29)",
                  (long long)B * (long long)N);
    UNERF_REQUIRE(P >= 1 && P <= UNERF_SPLAT_POSE_MAX_P, "splat_pose_ptangents_batch: P=%d outside [1,%d]", P, UNERF_SPLAT_POSE_MAX_P);
    UNERF_REQUIRE(H > 0 && W > 0, "splat_pose_ptangents_batch: bad H/W");
    UNERF_REQUIRE(views_host, "splat_pose_ptangents_batch: null pointer (views_host)");
    UNERF_REQUIRE(N == 0 || (means3d && cov3d && radii && proj && ptangents),
                  "splat_pose_ptangents_batch: null pointer (means3d, cov3d, radii, proj or ptangents)");
    const int PW = UNERF_SPLAT_POSE_PW(P);
    if (int rc = pose_ptangents_aligned("splat_pose_ptangents_batch", ptangents, P)) return rc;
    if (N == 0) return UNERF_OK;
    PosePtanBatchArgs a;
    a.means = means3d; a.cov3d = cov3d; a.radii = radii; a.N = N; a.proj = proj; a.P = P; a.H = H; a.W = W;
    a.clip = clip_thresh; a.out = ptangents;
    for (int v = 0; v < UNERF_SPLAT_MAX_VIEWS; ++v) {
        const float* r = views_host + (size_t)(v < B ? v : 0) * UNERF_SPLAT_VIEW_FLOATS;
        for (int k = 0; k < 12; ++k) a.cam[v].V[k] = r[k];
        a.cam[v].fx = r[12]; a.cam[v].fy = r[13];
    }
    const dim3 grid(blocks_for(N, 256), B), block(256);
    if (PW == 6) hipLaunchKernelGGL(splat_pose_ptangents_batch_kernel<6>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(splat_pose_ptangents_batch_kernel<12>, grid, block, 0, (hipStream_t)stream, a);
    return unerf_check_launch("splat_pose_ptangents_batch");
}

struct PoseJacArgs {
    const int32_t* ids;
    const int32_t* bins;
    const float* xys;
    const float* conics;
    const float* colors;
    const float* depths;
    const float* opac;
    const float* comp;
    const float* ptan;
    const float* bg;
    int P, H, W, bw;
    int cull;
    int channels, C;
    float* proj;
    float* var;
    float* val;
};

// one row of a channel: out_proj [P], out_var = sum_p row[p]^2 over p < P in order
template <int PW>
__device__ __forceinline__ void pose_jac_store_row(const PoseJacArgs& a, int64_t p, int ci, const float* row, float value) {
    const int64_t at = p * a.C + ci;
    if (a.val) a.val[at] = value;
    if (a.proj) {
        float* o = a.proj + at * a.P;
#pragma unroll
        for (int k = 0; k < PW; ++k)
            if (k < a.P) o[k] = row[k];
    }
    if (a.var) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < PW; ++k)
            if (k < a.P) s += row[k] * row[k];
        a.var[at] = s;
    }
}

// splat_pose_grad_kernel's walk, on the same stages (pose_walk_pixel .. pose_tangent_step), with the contracted tangents and the
// depth sum.  A staged record is three 16-byte header words [x, y, o, a | b, c, r, g | b, 1 / comp, z, -] in s_hdr and NT rows of PW floats in
// s_tan: the tangents of x, y, a, b, c (, comp: antialiased only), z.  <true, 12>: 128 x (48 + 336) B = 48 KiB, with the lists
// 49.9 KiB (three workgroups of a CU's 160 KiB); <true, 6>: 128 x (48 + 168) B = 27 KiB, with the lists 28.9 KiB (five).
// The walk is stated once: a view of a batch is the single-view walk on that view's bins and outputs (the ids of a batch
// already index the view-major arrays); MULTI only adds the colour rows' stride.
template <bool AA, int PW, bool MULTI>
__device__ __forceinline__ void pose_jac_walk(const PoseJacArgs& a, int cstride) {
    using VT = typename PoseVec<PW>::T;
    constexpr int VW = PoseVec<PW>::W;
    constexpr int PG = UNERF_SPLAT_POSE_GRAD_BATCH;
    constexpr int NT = AA ? 7 : 6;               // tangent rows per splat
    constexpr int TQ = 3 * NT;                   // ... in vectors
    constexpr int ZR = AA ? 6 : 5;               // the staged depth row
    __shared__ float4 s_hdr[PG * 3];
    __shared__ VT s_tan[PG * TQ];
    __shared__ int32_t s_gid[PG];
    __shared__ uint8_t s_mask[PG];
    __shared__ uint16_t s_list[4][PG];
    const int bw = a.bw;
    const int tbx = (a.W + bw - 1) / bw;
    const int bx = blockIdx.x, by = blockIdx.y;
    const int tile = by * tbx + bx;
    const int tr = threadIdx.x;
    const PosePixel at = pose_walk_pixel(tr, bx, by, bw, a.H, a.W);
    const float px = at.px, py = at.py;
    const bool inside = at.inside;
    const int64_t p = at.p;
    bool done = !inside;
    const int r0 = a.bins[tile * 2], r1 = a.bins[tile * 2 + 1];
    const int nbatch = (r1 - r0 + PG - 1) / PG;
    const bool cull = a.cull && bw == 16;
    const int wv = __builtin_amdgcn_readfirstlane(tr >> 6), lane = tr & 63;
    const float tile_x0 = (float)(bx * bw), tile_y0 = (float)(by * bw);
    float T = 1.f, pix[3] = {0.f, 0.f, 0.f}, D = 0.f;
    float dT[PW], dpix[3][PW], dD[PW];
#pragma unroll
    for (int k = 0; k < PW; ++k) { dT[k] = 0.f; dpix[0][k] = 0.f; dpix[1][k] = 0.f; dpix[2][k] = 0.f; dD[k] = 0.f; }
    for (int b = 0; b < nbatch; ++b) {
        const int start = r0 + PG * b;
        if (__syncthreads_count(done ? 1 : 0) >= 256) break;
        const int bsz = min(PG, r1 - start);
        if (tr < bsz)
            pose_stage_header<AA, true>({a.ids, a.xys, a.opac, a.conics, a.colors, a.comp, a.depths}, start + tr, MULTI ? cstride : 3,
                                        s_hdr, 3, s_gid, s_mask, tr, cull, tile_x0, tile_y0);
        __syncthreads();
        // the tangent rows, one vector per thread and trip (classic: compensation's row, the sixth of seven, is not staged)
        for (int w = tr; w < bsz * TQ; w += 256) {
            const int rec = w / TQ, q = w - rec * TQ;
            const int src = (AA || q < 15) ? q : q + 3;
            s_tan[w] = reinterpret_cast<const VT*>(a.ptan + (int64_t)s_gid[rec] * (UNERF_SPLAT_POSE_PROJ_ROWS * PW))[src];
        }
        __syncthreads();
        int n_mine = bsz;
        if (cull) UNERF_POSE_QUADRANT_LIST(n_mine, s_mask, s_list, bsz, wv, lane, PG)
        for (int k0 = 0; k0 < n_mine; ++k0) {
            if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;     // uniform: every pixel of this wave has finished
            const int t = cull ? (int)s_list[wv][k0] : k0;
            const float4 h0 = s_hdr[t * 3], h1 = s_hdr[t * 3 + 1], h2 = s_hdr[t * 3 + 2];
            const PoseBlend bl = pose_blend_decision(h0, h1, px, py, T, done);
            done = bl.done;
            if (__builtin_amdgcn_ballot_w64(bl.blend) == 0ull) continue;  // uniform: nobody needs this splat's tangents
            const PoseWeights wt = pose_sigma_weights(h0.w, h1.x, h1.y, bl.dx, bl.dy);
            const float col[3] = {h1.z, h1.w, h2.x};
            const float z = h2.z, vis = bl.alpha * T;
            pose_tangent_step<AA, true, PW>(&s_tan[t * TQ], 3 * ZR, bl, wt, T, h2.y, col, z, vis, dT, dpix, dD);
            if (bl.blend) {
                pix[0] += col[0] * vis; pix[1] += col[1] * vis; pix[2] += col[2] * vis;
                D += z * vis;
                T = bl.nT;
            }
        }
    }
    if (!inside) return;
    int ci = 0;
    float row[PW];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float bgc = a.bg ? a.bg[c] : 0.f;
        const float v = pix[c] + T * bgc;
        const bool live = v < 1.f;               // clamp(max = 1): a saturated channel has a zero row
#pragma unroll
        for (int k = 0; k < PW; ++k) row[k] = live ? dpix[c][k] + bgc * dT[k] : 0.f;
        if (a.channels & (UNERF_POSE_CH_R << c)) pose_jac_store_row<PW>(a, p, ci++, row, fminf(v, 1.f));
    }
    const float A = 1.f - T;
    if (a.channels & UNERF_POSE_CH_ACC) {
#pragma unroll
        for (int k = 0; k < PW; ++k) row[k] = -dT[k];
        pose_jac_store_row<PW>(a, p, ci++, row, A);
    }
    if (a.channels & UNERF_POSE_CH_EDEPTH) {
        const bool hit = A > 0.f;
        const float e = hit ? D / A : 0.f;
#pragma unroll
        for (int k = 0; k < PW; ++k) row[k] = hit ? dD[k] / A + e * dT[k] / A : 0.f;
        pose_jac_store_row<PW>(a, p, ci++, row, e);
    }
}

template <bool AA, int PW>
__global__ __launch_bounds__(256) void splat_pose_jac_kernel(PoseJacArgs a) {
    pose_jac_walk<AA, PW, false>(a, 3);
}

// grid: tiles x B.  View blockIdx.z walks tile_bins [v,tiles,2] and writes its own [HW,C(,P)] blocks; the offsets are formed in
// 64 bits ((v HW + p) C P can pass 2^31).
struct PoseJacBatchArgs {
    PoseJacArgs one;
    int cstride;
};

template <bool AA, int PW>
__global__ __launch_bounds__(256) void splat_pose_jac_batch_kernel(PoseJacBatchArgs b) {
    PoseJacArgs a = b.one;
    const int64_t v = blockIdx.z;
    const int64_t tiles = (int64_t)((a.W + a.bw - 1) / a.bw) * ((a.H + a.bw - 1) / a.bw);
    const int64_t at = v * a.H * a.W * a.C;
    a.bins += v * tiles * 2;
    if (a.val) a.val += at;
    if (a.var) a.var += at;
    if (a.proj) a.proj += at * a.P;
    pose_jac_walk<AA, PW, true>(a, b.cstride);
}

// ---- the two Jacobian entries' shared host side (the entry's name goes into every message) ---------------------------------------
static int pose_jac_checks(const char* what, int P, int channels, const float* out_proj, const float* out_var, const float* out_val,
                           int flags, int block_width, int H, int W) {
    constexpr int ALL = UNERF_POSE_CH_R | UNERF_POSE_CH_G | UNERF_POSE_CH_B | UNERF_POSE_CH_ACC | UNERF_POSE_CH_EDEPTH;
    UNERF_REQUIRE(P >= 1 && P <= UNERF_SPLAT_POSE_MAX_P, "%s: P=%d outside [1,%d]", what, P, UNERF_SPLAT_POSE_MAX_P);
    UNERF_REQUIRE(channels != 0, "%s: channels is empty", what);
    UNERF_REQUIRE((channels & ~ALL) == 0, "%s: unknown channel bits %d", what, channels & ~ALL);
    UNERF_REQUIRE(out_proj || out_var || out_val, "%s: no output asked for (out_proj, out_var and out_val are NULL)", what);
    UNERF_REQUIRE((flags & ~UNERF_RASTER_NO_CULL) == 0, "%s: unknown flags %d", what, flags);
    UNERF_REQUIRE(block_width >= 1 && block_width <= 16, "%s: block_width=%d outside [1,16]", what, block_width);
    UNERF_REQUIRE(H >= 0 && W >= 0, "%s: bad H/W", what);
    return UNERF_OK;
}

static PoseJacArgs pose_jac_args(const int32_t* gaussian_ids_sorted, const int32_t* tile_bins, const float* xys, const float* conics,
                                 const float* colors, const float* depths, const float* opacities, const float* compensation,
                                 const float* ptangents, const float* background, int P, int H, int W, int block_width, int flags,
                                 int channels, float* out_proj, float* out_var, float* out_val) {
    PoseJacArgs a;
    a.ids = gaussian_ids_sorted; a.bins = tile_bins; a.xys = xys; a.conics = conics; a.colors = colors; a.depths = depths;
    a.opac = opacities; a.comp = compensation; a.ptan = ptangents; a.bg = background;
    a.P = P; a.H = H; a.W = W; a.bw = block_width; a.cull = (flags & UNERF_RASTER_NO_CULL) ? 0 : 1;
    a.channels = channels; a.C = __builtin_popcount((unsigned)channels);
    a.proj = out_proj; a.var = out_var; a.val = out_val;
    return a;
}

// K<AA, PW>::kernel is the walk's kernel for Args; the instantiation follows the compensation pointer and P's padded width
template <bool AA, int PW> struct PoseJacOne { static constexpr auto kernel = splat_pose_jac_kernel<AA, PW>; };
template <bool AA, int PW> struct PoseJacBatch { static constexpr auto kernel = splat_pose_jac_batch_kernel<AA, PW>; };
template <template <bool, int> class K, typename Args>
static void pose_jac_launch(bool aa, int P, dim3 grid, const Args& a, void* stream) {
    const dim3 block(256);
    const hipStream_t st = (hipStream_t)stream;
    if (UNERF_SPLAT_POSE_PW(P) == 6) {
        if (aa) hipLaunchKernelGGL((K<true, 6>::kernel), grid, block, 0, st, a);
        else hipLaunchKernelGGL((K<false, 6>::kernel), grid, block, 0, st, a);
    } else {
        if (aa) hipLaunchKernelGGL((K<true, 12>::kernel), grid, block, 0, st, a);
        else hipLaunchKernelGGL((K<false, 12>::kernel), grid, block, 0, st, a);
    }
}

extern "C" int unerf_splat_pose_jacobian(const int32_t* gaussian_ids_sorted, const int32_t* tile_bins, const float* xys,
                                         const float* conics, const float* colors, const float* depths, const float* opacities,
                                         const float* compensation, const float* ptangents, const float* background, int P,
                                         int H, int W, int block_width, int flags, int channels, float* out_proj,
                                         float* out_var, float* out_val, void* stream) {
    const char* what = "splat_pose_jacobian";
    UNERF_REQUIRE(gaussian_ids_sorted && tile_bins && xys && conics && colors && depths && opacities && ptangents,
                  "%s: null pointer", what);
    if (int rc = pose_jac_checks(what, P, channels, out_proj, out_var, out_val, flags, block_width, H, W)) return rc;
    if (int rc = pose_ptangents_aligned(what, ptangents, P)) return rc;
    if (H == 0 || W == 0) return UNERF_OK;
    const PoseJacArgs a = pose_jac_args(gaussian_ids_sorted, tile_bins, xys, conics, colors, depths, opacities, compensation, ptangents,
                                        background, P, H, W, block_width, flags, channels, out_proj, out_var, out_val);
    const dim3 grid((W + block_width - 1) / block_width, (H + block_width - 1) / block_width);
    pose_jac_launch<PoseJacOne>(compensation != nullptr, P, grid, a, stream);
    return unerf_check_launch(what);
}

extern "C" int unerf_splat_pose_jacobian_batch(const int32_t* gaussian_ids_sorted, const int32_t* tile_bins, const float* xys,
                                               const float* conics, const float* colors, int color_stride, const float* depths,
                                               const float* opacities, const float* compensation, const float* ptangents,
                                               const float* background, int B, int64_t N, int P, int H, int W, int block_width,
                                               int flags, int channels, float* out_proj, float* out_var, float* out_val,
                                               void* stream) {
    const char* what = "splat_pose_jacobian_batch";
    UNERF_REQUIRE(B >= 1 && B <= UNERF_SPLAT_MAX_VIEWS, "%s: B=%d outside [1,%d]", what, B, UNERF_SPLAT_MAX_VIEWS);
    UNERF_REQUIRE(N >= 0 && (int64_t)B * N < UNERF_SPLAT_MAX_BATCH_SPLATS, "%s: B*N = %lld outside [0,2^29)", what,
                  (long long)B * (long long)N);
    UNERF_REQUIRE(gaussian_ids_sorted && tile_bins && xys && conics && colors && depths && opacities && ptangents,
                  "%s: null pointer (gaussian_ids_sorted, tile_bins, xys, conics, colors, depths, opacities or ptangents)", what);
    UNERF_REQUIRE(color_stride >= 3, "%s: color_stride=%d below 3", what, color_stride);
    if (int rc = pose_jac_checks(what, P, channels, out_proj, out_var, out_val, flags, block_width, H, W)) return rc;
    const int tbx = (W + block_width - 1) / block_width, tby = (H + block_width - 1) / block_width;
    UNERF_REQUIRE((int64_t)tbx * tby <= UNERF_SPLAT_BATCH_MAX_TILES, "%s: %lld tiles, the batched lists hold %d", what,
                  (long long)tbx * tby, UNERF_SPLAT_BATCH_MAX_TILES);
    if (int rc = pose_ptangents_aligned(what, ptangents, P)) return rc;
    if (H == 0 || W == 0) return UNERF_OK;
    PoseJacBatchArgs b;
    b.one = pose_jac_args(gaussian_ids_sorted, tile_bins, xys, conics, colors, depths, opacities, compensation, ptangents, background,
                          P, H, W, block_width, flags, channels, out_proj, out_var, out_val);
    b.cstride = color_stride;
    pose_jac_launch<PoseJacBatch>(compensation != nullptr, P, dim3(tbx, tby, B), b, stream);
    return unerf_check_launch(what);
}
