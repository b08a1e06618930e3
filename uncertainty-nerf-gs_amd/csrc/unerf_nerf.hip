// NeRF half of libunerf: ray generation, hash grid, proposal density, weights+PDF resampling,
// fused main field (active / mc-dropout / laplace heads), composite with variance, moments.
// gfx950 only; wave = 64.  See include/unerf.h for the contract of each entry point.
#include "unerf_common.hpp"

#include <mutex>
#include <type_traits>
#include <unordered_map>

#include <cassert>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>

// ======================================================================================
// host plumbing
// ======================================================================================
static thread_local char g_err[512] = "";

void unerf_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
int unerf_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        unerf_set_error("%s: %s", what, hipGetErrorString(e));
        return UNERF_ERR_HIP;
    }
    return UNERF_OK;
}

extern "C" const char* unerf_last_error(void) { return g_err; }
// The operand layouts the kernels read, for the host to pack to (ops.pack_field_mfma16: fold_trunk; ops.pack_laplace_heads16:
// exp2_rows): the K-pass kernel's 16-row trunk-out layer folded into two MFMAs per k-step, and lap16_blob rows pre-scaled
// by +-log2(e) for a bare exp2 in the Laplace heads' epilogue.
extern "C" int unerf_build_flags(void) { return UNERF_BUILD_TRUNK_FOLD | UNERF_BUILD_LAP_EXP2; }
// 11xx: round-2 ABI (drop_sites, sample_major planes, aabb, ...); 1101: ray_box_bins / ray_planes_bins; 1102: build flags,
// folded trunk-out slabs; 12xx: round-3 ABI -- `spacing` (UNERF_SPACING_*) behind every near / far pair, `background`
// (UNERF_BG_*) on the composite / GGN entry points
extern "C" int unerf_version(void) { return UNERF_ABI_VERSION; }
extern "C" int unerf_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

struct TcnnLevels {
    unerf_tcnn_level v[32];
};

static inline unerf_norm_box make_norm_box(int use_aabb, const float* aabb) {
    unerf_norm_box b;
    b.use_aabb = use_aabb ? 1 : 0;
    for (int c = 0; c < 3; ++c) {
        b.lo[c] = use_aabb ? aabb[c] : 0.f;
        b.len[c] = use_aabb ? aabb[3 + c] - aabb[c] : 1.f;
    }
    return b;
}
// RGBRenderer(background_color=...) at eval [UPSTREAM nerfstudio 1.1.0 renderers.RGBRenderer.combine_rgb / forward]:
// "last_sample": comp + rgb[..., -1, :] (1 - acc); "random": comp as it is (no blending at eval, "as if the background
// were black"); "white" / "black": comp + colour (1 - acc); then clamp to [0, 1].
template <typename Args>
static inline int unerf_set_background(Args& a, int background, const float* rgb_host, const char* what) {
    if (background != UNERF_BG_LAST_SAMPLE && background != UNERF_BG_NONE && background != UNERF_BG_COLOR) {
        unerf_set_error("%s: background=%d (expected UNERF_BG_LAST_SAMPLE / _NONE / _COLOR)", what, background);
        return UNERF_ERR_ARG;
    }
    if (background == UNERF_BG_COLOR && !rgb_host) {
        unerf_set_error("%s: UNERF_BG_COLOR needs background_rgb (3 host floats)", what);
        return UNERF_ERR_ARG;
    }
    a.bg_mode = background;
    for (int c = 0; c < 3; ++c) a.bg[c] = (background == UNERF_BG_COLOR) ? rgb_host[c] : 0.f;
    return UNERF_OK;
}

#define UNERF_REQUIRE_SPACING(sp) \
    UNERF_REQUIRE((sp) == UNERF_SPACING_PIECEWISE || (sp) == UNERF_SPACING_UNIFORM, "spacing=%d (expected UNERF_SPACING_*)", (int)(sp))
// the spacing fields of a kernel's argument struct: the checked UNERF_SPACING_* and the near / far planes in its domain
template <typename Args>
static inline int set_spacing(Args& a, float near_plane, float far_plane, int spacing) {
    UNERF_REQUIRE_SPACING(spacing);
    a.lin = spacing; a.s_near = unerf_spacing_of(near_plane, spacing); a.s_far = unerf_spacing_of(far_plane, spacing);
    return UNERF_OK;
}

// ---- kernel selection: a run-time value as a compile-time constant handed to f, once.  Every host function that picks a
// template instantiation does it through these (one launch expression per kernel family), and nothing else does.
// v in Vs... -> f(std::integral_constant<int, v>{}); false when v is none of them (f is not called)
template <int... Vs, typename F>
static bool with_int(int v, F&& f) {
    return ((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}
// {0, 1, 2}: the TCNN argument of the matrix kernels and the UNERF_FIELD_* mode (checked before: no other value gets here)
template <typename F>
static void with_int3(int v, F&& f) { with_int<0, 1, 2>(v, f); }
template <typename F>
static void with_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
// the trailing argument pack of the *_views kernels: f(make()) when the launch has one, f() for the single-view kernels
template <typename Make, typename F>
static void with_pack(bool on, Make&& make, F&& f) {
    if (on) f(make());
    else f();
}
// Samples per lane of the 16-lane ray groups (composite, depth draws): S = 16 * SPL for SPL in {1,2,3,4,6,8,16} (every
// nerfacto sample count) takes the aligned kernels; any other 1 <= S <= 256 takes the RAGGED instantiation of the next SPL
// up, whose slots k >= S are masked.
static inline int unerf_spl_for(int S) {
    const int want = (S + 15) / 16;
    for (int spl : {1, 2, 3, 4, 6, 8, 16})
        if (spl >= want) return spl;
    return 0;
}
// f(integral_constant<int, SPL>, bool_constant<RAGGED>); the callers have refused S outside [1,256] by name
template <typename F>
static void with_spl(int S, F&& f) {
    const int spl = unerf_spl_for(S);
    const bool built = with_int<1, 2, 3, 4, 6, 8, 16>(spl, [&](auto n) { with_bool(spl * 16 != S, [&](auto ragged) { f(n, ragged); }); });
    assert(built);
    (void)built;
}
static inline unsigned blocks_for(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// Division of an index < 2^31 by a launch-invariant divisor (samples per ray): one multiply-high and a
// shift instead of the ~30 issue slots of the generic 32-bit division (Granlund-Montgomery, N = 31:
// m = floor(2^(31+l) / d) + 1 with l = ceil(log2 d) satisfies 2^(31+l) < m d <= 2^(31+l) + 2^l).
struct FastDiv {
    uint32_t magic;  // 0: d == 1
    uint32_t shift;
    uint32_t d;
};
static inline FastDiv make_fastdiv(uint32_t d) {
    FastDiv f{0u, 0u, d};
    if (d > 1u) {
        uint32_t l = 0;
        while ((1ull << l) < d) ++l;
        f.magic = (uint32_t)((1ull << (31 + l)) / d + 1ull);
        f.shift = l - 1;
    }
    return f;
}
__device__ __forceinline__ uint32_t fastdiv(uint32_t x, const FastDiv& f) {
    return f.magic ? (__umulhi(x, f.magic) >> f.shift) : x;
}

// Several whole views in one launch (include/unerf.h: unerf_ray_views): launch row j is frame-local ray j mod hw of view
// j / hw.  A kernel argument of the *_views instantiations only (a trailing parameter pack that is empty in the
// single-view kernels, which keep their argument list and their code).
struct ViewMap {
    FastDiv div_hw, div_chunk;   // by rays per view, by chunk_rays
    uint32_t hw;
    uint32_t cpv;                // clip rows (chunks) per view: ceil(hw / chunk_rays)
};
__device__ __forceinline__ void view_of(const ViewMap& m, uint32_t j, uint32_t& view, uint32_t& local) {
    view = fastdiv(j, m.div_hw);
    local = j - view * m.hw;
}
// Row of the clip buffer that launch row r reads / updates.  Single view: the chunk of frame ray ray_offset + r.
template <typename Args>
__device__ __forceinline__ int64_t clip_chunk(const Args& a, int64_t r) {
    return (a.ray_offset + r) / a.chunk_rays;
}
template <typename Args>
__device__ __forceinline__ int64_t clip_chunk(const Args&, int64_t r, const ViewMap& m) {
    uint32_t view, local;
    view_of(m, (uint32_t)r, view, local);
    return (int64_t)(view * m.cpv + fastdiv(local, m.div_chunk));
}
static int check_views(const unerf_ray_views* v, int64_t R, const char* what) {
    UNERF_REQUIRE(v, "%s: null views", what);
    UNERF_REQUIRE(v->n_views >= 1 && v->n_views <= UNERF_NERF_MAX_VIEWS, "%s: n_views=%d outside [1,%d]", what, (int)v->n_views,
                  UNERF_NERF_MAX_VIEWS);
    UNERF_REQUIRE(v->rays_per_view > 0, "%s: rays_per_view=%lld must be > 0", what, (long long)v->rays_per_view);
    UNERF_REQUIRE(R == (int64_t)v->n_views * v->rays_per_view, "%s: R=%lld is not n_views x rays_per_view = %d x %lld", what,
                  (long long)R, (int)v->n_views, (long long)v->rays_per_view);
    UNERF_REQUIRE(R < (1ll << 31), "%s: R=%lld rays in one launch (32-bit row index)", what, (long long)R);
    return UNERF_OK;
}
static ViewMap make_view_map(const unerf_ray_views* v, int64_t chunk_rays) {
    ViewMap m;
    const int64_t hw = v->rays_per_view, cr = chunk_rays > 0 ? (chunk_rays < (1ll << 31) ? chunk_rays : (1ll << 31) - 1) : 1;
    m.div_hw = make_fastdiv((uint32_t)hw); m.div_chunk = make_fastdiv((uint32_t)cr);
    m.hw = (uint32_t)hw; m.cpv = (uint32_t)((hw + cr - 1) / cr);
    return m;
}

// ======================================================================================
// wave / group helpers
// ======================================================================================
// Cross-lane traffic on DPP (data-parallel primitives: the lane permutation rides on the consuming VALU
// instruction) instead of __shfl_* (which compile to ds_bpermute_b32 through the LDS crossbar plus address,
// compare and select instructions: ~5 VALU + 1 LDS op per scan step).  The PDF, composite and depth-draw
// kernels are VALU-bound and spend a fifth of their instructions in scans.  gfx9 DPP controls:
// row_shr:n = 0x110+n (within a 16-lane row, zero fill), row_bcast:15 = 0x142, row_bcast:31 = 0x143,
// wave_shr:1 = 0x138, quad_perm = 0x00-0xFF, row_half_mirror = 0x141, row_mirror = 0x140.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ float dpp_f(float v) {  // lanes without a source (or masked-off rows) read 0
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ float dpp_f_or(float v, float fill) {  // lanes without a source lane read `fill`
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ int dpp_i(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xF, true);
}

// sum over a WIDTH-lane group (16: one DPP row; 64: the wave), result in every lane
template <int WIDTH>
__device__ __forceinline__ float group_sum(float v) {
    static_assert(WIDTH == 16 || WIDTH == 64, "group width");
    v += dpp_f<0xB1>(v);    // quad_perm [1,0,3,2]
    v += dpp_f<0x4E>(v);    // quad_perm [2,3,0,1]
    v += dpp_f<0x141>(v);   // row_half_mirror
    v += dpp_f<0x140>(v);   // row_mirror: every lane of a row holds the row sum
    if (WIDTH == 64) {
        v += dpp_f<0x142, 0xA>(v);   // rows 1,3 += row sums of rows 0,2
        v += dpp_f<0x143, 0xC>(v);   // rows 2,3 += sum of rows 0,1  -> lane 63 holds the total
        v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
    }
    return v;
}
template <int WIDTH>
__device__ __forceinline__ int group_sum_i(int v) {
    static_assert(WIDTH == 16 || WIDTH == 64, "group width");
    v += dpp_i<0xB1>(v);
    v += dpp_i<0x4E>(v);
    v += dpp_i<0x141>(v);
    v += dpp_i<0x140>(v);
    if (WIDTH == 64) {
        v += dpp_i<0x142, 0xA>(v);
        v += dpp_i<0x143, 0xC>(v);
        v = __builtin_amdgcn_readlane(v, 63);
    }
    return v;
}
// inclusive scan over a WIDTH-lane group (Hillis-Steele inside the 16-lane rows, then the row totals)
template <int WIDTH>
__device__ __forceinline__ float group_incl_scan(float v, int /*lane_in_group*/) {
    static_assert(WIDTH == 16 || WIDTH == 64, "group width");
    v += dpp_f<0x111>(v);
    v += dpp_f<0x112>(v);
    v += dpp_f<0x114>(v);
    v += dpp_f<0x118>(v);
    if (WIDTH == 64) {
        v += dpp_f<0x142, 0xA>(v);
        v += dpp_f<0x143, 0xC>(v);
    }
    return v;
}

// exclusive scan: the inclusive result shifted by one lane.  (NOT "inclusive - own": that loses
// the low bits of small prefixes behind a large element and turns inf - inf into NaN.)
template <int WIDTH>
__device__ __forceinline__ float group_excl_scan(float v, int lane_in_group) {
    const float incl = group_incl_scan<WIDTH>(v, lane_in_group);
    return WIDTH == 16 ? dpp_f<0x111>(incl) : dpp_f<0x138>(incl);   // row_shr:1 / wave_shr:1, zero fill
}

// ======================================================================================
// 1. rays
// ======================================================================================
struct RayGenArgs {
    float R[9];
    float T[3];
    float fx, fy, cx, cy;
    float k1, k2, k3, k4, p1, p2;   // OPENCV lens parameters, nerfstudio's order
    int distorted;                  // any of the six != 0 (and the camera type takes lens parameters)
    int camera_type;                // UNERF_CAMERA_*
    int H, W;
    int64_t start, count;
    float* o;
    float* d;
    float* pa;
};

// camera_utils.radial_and_tangential_undistort [UPSTREAM nerfstudio 1.1.0, after MultiNeRF]: Newton iterations from the
// distorted point on  f(x, y) = (x d + 2 p1 x y + p2 (r + 2 x^2) - xd,  y d + 2 p2 x y + p1 (r + 2 y^2) - yd),
// r = x^2 + y^2, d = 1 + r (k1 + r (k2 + r (k3 + r k4))); every product and sum in the order the torch expression
// evaluates it (fp32, nothing contracted), a step only where |det J| > eps.
__device__ __forceinline__ void raygen_undistort(const RayGenArgs& a, float& u, float& v) {
    const float xd = u, yd = v;
    float x = xd, y = yd;
#pragma unroll 1
    for (int it = 0; it < UNERF_UNDISTORT_ITERATIONS; ++it) {
        const float r = x * x + y * y;
        const float d = 1.0f + r * (a.k1 + r * (a.k2 + r * (a.k3 + r * a.k4)));
        const float fx = ((d * x + ((2.f * a.p1) * x) * y) + a.p2 * (r + (2.f * x) * x)) - xd;
        const float fy = ((d * y + ((2.f * a.p2) * x) * y) + a.p1 * (r + (2.f * y) * y)) - yd;
        const float d_r = a.k1 + r * (2.0f * a.k2 + r * (3.0f * a.k3 + (r * 4.0f) * a.k4));
        const float d_x = (2.0f * x) * d_r;
        const float d_y = (2.0f * y) * d_r;
        const float fx_x = ((d + d_x * x) + (2.0f * a.p1) * y) + (6.0f * a.p2) * x;
        const float fx_y = (d_y * x + (2.0f * a.p1) * x) + (2.0f * a.p2) * y;
        const float fy_x = (d_x * y + (2.0f * a.p2) * y) + (2.0f * a.p1) * x;
        const float fy_y = ((d + d_y * y) + (2.0f * a.p2) * x) + (6.0f * a.p1) * y;
        const float den = fy_x * fx_y - fx_x * fy_y;
        const float xn = fx * fy_y - fy * fx_y;
        const float yn = fy * fx_x - fx * fy_x;
        const bool ok = fabsf(den) > UNERF_UNDISTORT_EPS;
        x = x + (ok ? xn / den : 0.f);
        y = y + (ok ? yn / den : 0.f);
    }
    u = x;
    v = y;
}

__device__ __forceinline__ void raygen_dir(const RayGenArgs& a, float u, float v, float& dx, float& dy, float& dz) {
    if (a.distorted) raygen_undistort(a, u, v);
    // camera-frame direction (include/unerf.h: camera_type), uniform branch; PERSPECTIVE keeps the exact (u, v, -1)
    float cxd = u, cyd = v, czd = -1.f;
    if (a.camera_type == UNERF_CAMERA_FISHEYE) {
        float theta = sqrtf(u * u + v * v);
        theta = fminf(fmaxf(theta, 0.f), 3.14159265358979323846f);
        const float st = sinf(theta);
        cxd = u * st / theta;     // 0 / 0 at the exact principal point, as upstream
        cyd = v * st / theta;
        czd = -cosf(theta);
    } else if (a.camera_type == UNERF_CAMERA_EQUIRECTANGULAR) {
        const float theta = -3.14159265358979323846f * u, phi = 3.14159265358979323846f * (0.5f - v);
        cxd = -sinf(theta) * sinf(phi);
        cyd = cosf(phi);
        czd = -cosf(theta) * sinf(phi);
    } else if (a.camera_type == UNERF_CAMERA_ORTHOPHOTO) {
        cxd = 0.f;
        cyd = 0.f;
    }
    // sum_c dir[c] * R[r][c]; torch.sum over 3 elements left to right
    float x = (cxd * a.R[0] + cyd * a.R[1]) + czd * a.R[2];
    float y = (cxd * a.R[3] + cyd * a.R[4]) + czd * a.R[5];
    float z = (cxd * a.R[6] + cyd * a.R[7]) + czd * a.R[8];
    float n = fmaxf(sqrtf((x * x + y * y) + z * z), 1e-7f);
    dx = x / n;
    dy = y / n;
    dz = z / n;
}

// pixel g of the frame -> row n of the outputs
__device__ __forceinline__ void raygen_one(const RayGenArgs& a, int64_t g, int64_t n) {
    int i = (int)(g / a.W), j = (int)(g % a.W);
    float y = (float)i + 0.5f, x = (float)j + 0.5f;
    float u0 = (x - a.cx) / a.fx, v0 = -(y - a.cy) / a.fy;
    float u1 = (x - a.cx + 1.f) / a.fx;
    float v2 = -(y - a.cy + 1.f) / a.fy;
    float d0x, d0y, d0z, d1x, d1y, d1z, d2x, d2y, d2z;
    raygen_dir(a, u0, v0, d0x, d0y, d0z);
    if (a.camera_type == UNERF_CAMERA_ORTHOPHOTO) {   // the origin moves over the image plane: c2w (u, v, 0, 1)
        a.o[n * 3 + 0] = (u0 * a.R[0] + v0 * a.R[1]) + a.T[0];
        a.o[n * 3 + 1] = (u0 * a.R[3] + v0 * a.R[4]) + a.T[1];
        a.o[n * 3 + 2] = (u0 * a.R[6] + v0 * a.R[7]) + a.T[2];
    } else {
        a.o[n * 3 + 0] = a.T[0];
        a.o[n * 3 + 1] = a.T[1];
        a.o[n * 3 + 2] = a.T[2];
    }
    a.d[n * 3 + 0] = d0x;
    a.d[n * 3 + 1] = d0y;
    a.d[n * 3 + 2] = d0z;
    if (a.pa) {
        raygen_dir(a, u1, v0, d1x, d1y, d1z);
        raygen_dir(a, u0, v2, d2x, d2y, d2z);
        float ex = d0x - d1x, ey = d0y - d1y, ez = d0z - d1z;
        float fx_ = d0x - d2x, fy_ = d0y - d2y, fz_ = d0z - d2z;
        float dxn = sqrtf((ex * ex + ey * ey) + ez * ez);
        float dyn = sqrtf((fx_ * fx_ + fy_ * fy_) + fz_ * fz_);
        a.pa[n] = dxn * dyn;
    }
}

__global__ __launch_bounds__(256) void raygen_kernel(RayGenArgs a) {
    int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= a.count) return;
    raygen_one(a, a.start + n, n);
}

// Several whole frames of one size and camera type (unerf_generate_rays_views): blockIdx.y = the view, so the camera is
// block-uniform (scalar loads from the argument block) and every pixel runs raygen_one on its own view's record.
struct RayGenCam {
    float R[9], T[3], fx, fy, cx, cy, k1, k2, k3, k4, p1, p2;
    int distorted;
};
struct RayGenViewsArgs {
    RayGenArgs base;   // camera_type, H, W, count = H W, outputs; the camera fields are taken from cam[view]
    RayGenCam cam[UNERF_NERF_MAX_VIEWS];
};
__global__ __launch_bounds__(256) void raygen_views_kernel(RayGenViewsArgs v) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= v.base.count) return;
    const RayGenCam& c = v.cam[blockIdx.y];
    RayGenArgs a = v.base;
    for (int i = 0; i < 9; ++i) a.R[i] = c.R[i];
    for (int i = 0; i < 3; ++i) a.T[i] = c.T[i];
    a.fx = c.fx; a.fy = c.fy; a.cx = c.cx; a.cy = c.cy;
    a.k1 = c.k1; a.k2 = c.k2; a.k3 = c.k3; a.k4 = c.k4; a.p1 = c.p1; a.p2 = c.p2;
    a.distorted = c.distorted;
    raygen_one(a, g, (int64_t)blockIdx.y * v.base.count + g);
}

static int raygen_check_type(int camera_type, const char* what) {
    UNERF_REQUIRE(camera_type == UNERF_CAMERA_PERSPECTIVE || camera_type == UNERF_CAMERA_FISHEYE ||
                      camera_type == UNERF_CAMERA_EQUIRECTANGULAR || camera_type == UNERF_CAMERA_ORTHOPHOTO,
                  "%s: camera_type %d is not built (PERSPECTIVE 1, FISHEYE 2, EQUIRECTANGULAR 3, ORTHOPHOTO 8)", what, camera_type);
    return UNERF_OK;
}

extern "C" int unerf_generate_rays_views(const unerf_ray_camera* cameras, int n_views, int camera_type, int H, int W,
                                         float* origins, float* directions, float* pixel_area, void* stream) {
    UNERF_REQUIRE(n_views >= 1 && n_views <= UNERF_NERF_MAX_VIEWS, "generate_rays_views: n_views=%d outside [1,%d]", n_views,
                  UNERF_NERF_MAX_VIEWS);
    UNERF_REQUIRE(cameras && origins && directions, "generate_rays_views: null pointer");
    if (int rc = raygen_check_type(camera_type, "generate_rays_views")) return rc;
    UNERF_REQUIRE(H > 0 && W > 0 && (int64_t)H * W * n_views < (1ll << 31), "generate_rays_views: %d views of %dx%d", n_views, H, W);
    RayGenViewsArgs v;
    memset(&v, 0, sizeof(v));
    for (int i = 0; i < n_views; ++i) {
        const unerf_ray_camera& s = cameras[i];
        RayGenCam& c = v.cam[i];
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) c.R[r * 3 + k] = s.c2w[r * 4 + k];
            c.T[r] = s.c2w[r * 4 + 3];
        }
        c.fx = s.fx; c.fy = s.fy; c.cx = s.cx; c.cy = s.cy;
        if (camera_type != UNERF_CAMERA_EQUIRECTANGULAR) {   // as unerf_generate_rays
            for (int k = 0; k < 6; ++k) {
                UNERF_REQUIRE(std::isfinite(s.distortion[k]), "generate_rays_views: distortion[%d] of view %d is not finite", k, i);
                c.distorted |= s.distortion[k] != 0.f;
            }
            c.k1 = s.distortion[0]; c.k2 = s.distortion[1]; c.k3 = s.distortion[2]; c.k4 = s.distortion[3];
            c.p1 = s.distortion[4]; c.p2 = s.distortion[5];
        }
    }
    v.base.camera_type = camera_type; v.base.H = H; v.base.W = W; v.base.start = 0; v.base.count = (int64_t)H * W;
    v.base.o = origins; v.base.d = directions; v.base.pa = pixel_area;
    hipLaunchKernelGGL(raygen_views_kernel, dim3(blocks_for(v.base.count, 256), (unsigned)n_views), dim3(256), 0, (hipStream_t)stream, v);
    return unerf_check_launch("generate_rays_views");
}

extern "C" int unerf_generate_rays(const float* c2w, float fx, float fy, float cx, float cy, const float* distortion,
                                   int camera_type, int H, int W, int64_t ray_start, int64_t count, float* origins,
                                   float* directions, float* pixel_area, void* stream) {
    UNERF_REQUIRE(c2w && (count == 0 || (origins && directions)), "generate_rays: null pointer");
    UNERF_REQUIRE(camera_type == UNERF_CAMERA_PERSPECTIVE || camera_type == UNERF_CAMERA_FISHEYE ||
                      camera_type == UNERF_CAMERA_EQUIRECTANGULAR || camera_type == UNERF_CAMERA_ORTHOPHOTO,
                  "generate_rays: camera_type %d is not built (PERSPECTIVE 1, FISHEYE 2, EQUIRECTANGULAR 3, ORTHOPHOTO 8)", camera_type);
    UNERF_REQUIRE(H > 0 && W > 0 && ray_start >= 0 && count >= 0 && ray_start + count <= (int64_t)H * W,
                  "generate_rays: ray range [%lld,+%lld) outside %dx%d", (long long)ray_start, (long long)count, H, W);
    if (count == 0) return UNERF_OK;
    RayGenArgs a;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) a.R[r * 3 + c] = c2w[r * 4 + c];
        a.T[r] = c2w[r * 4 + 3];
    }
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.H = H; a.W = W;
    a.k1 = a.k2 = a.k3 = a.k4 = a.p1 = a.p2 = 0.f;
    a.distorted = 0;
    a.camera_type = camera_type;
    if (distortion && camera_type != UNERF_CAMERA_EQUIRECTANGULAR) {   // upstream: "do not apply distortion for equirectangular images"
        for (int i = 0; i < 6; ++i) {
            UNERF_REQUIRE(std::isfinite(distortion[i]), "generate_rays: distortion[%d] is not finite", i);
            a.distorted |= distortion[i] != 0.f;
        }
        a.k1 = distortion[0]; a.k2 = distortion[1]; a.k3 = distortion[2]; a.k4 = distortion[3];
        a.p1 = distortion[4]; a.p2 = distortion[5];
    }
    a.start = ray_start; a.count = count; a.o = origins; a.d = directions; a.pa = pixel_area;
    hipLaunchKernelGGL(raygen_kernel, dim3(blocks_for(count, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return unerf_check_launch("generate_rays");
}

// ---- oriented crop box: per-ray planes folded into the first level's spacing bins ----
// Cameras.generate_rays(..., obb_box=box) sets RayBundle.nears / fars from the ray / box slab test and the collider then
// keeps them; the sampler maps its [0,1] spacing bins through each ray's own planes.  Every kernel after this one takes
// ONE pair of planes (near0, far0) per launch, so the per-ray planes are folded into the bins instead:
//   b' = (b s(far_r) + (1 - b) s(near_r) - s(near0)) / (s(far0) - s(near0))
// gives the same euclidean edges under (near0, far0), and the pdf resampling is affine in the bins, so every later
// level stays consistent without knowing about the box.
struct BoxBinsArgs {
    const float* o; const float* d; const float* row;   // rays, shared [n+1] spacing row
    float w2b[12];                                       // inverse([R|T]) as 3x4 row-major
    float half[3];
    float near0, far0;
    int lin;                                             // UNERF_SPACING_*
    int64_t R; int n;
    float* bins; float* nears; float* fars;              // [R,n+1], [R], [R] (planes may be null)
    const float* in_nears; const float* in_fars;         // given: the bundle's own planes, no box test
};

__global__ __launch_bounds__(256) void box_bins_kernel(BoxBinsArgs a) {
    int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.R) return;
    const int lane = threadIdx.x & 63;
    float tmin = -INFINITY, tmax = INFINITY;
    if (a.in_nears) {   // the bundle's own planes: a.o / a.d are null here
        tmin = a.in_nears[r];
        tmax = a.in_fars[r];
    } else {
    const float ox = a.o[r * 3], oy = a.o[r * 3 + 1], oz = a.o[r * 3 + 2];
    const float dx = a.d[r * 3], dy = a.d[r * 3 + 1], dz = a.d[r * 3 + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* m = a.w2b + c * 4;
        float bo = ((m[0] * ox + m[1] * oy) + m[2] * oz) + m[3];
        float bd = (m[0] * dx + m[1] * dy) + m[2] * dz;
        float t0 = (-a.half[c] - bo) / bd, t1 = (a.half[c] - bo) / bd;
        tmin = fmaxf(tmin, fminf(t0, t1));
        tmax = fminf(tmax, fmaxf(t0, t1));
    }
    tmin = fminf(fmaxf(tmin, 0.f), 1e10f);
    tmax = fminf(fmaxf(tmax, 0.f), 1e10f);
    if (!(tmax > tmin)) tmin = tmax = 1e10f;             // a miss: both planes at the invalid value
    }
    if (lane == 0) {
        if (a.nears) a.nears[r] = tmin;
        if (a.fars) a.fars[r] = tmax;
    }
    // a miss upstream puts every sample at s_inv(s(1e10)) = s_inv(1.f) = inf, i.e. undefined pixels; here its samples
    // collapse onto the far plane (zero-length intervals -> zero weights, accumulation 0), which keeps everything finite
    const float sn = unerf_spacing_of(fminf(tmin, a.far0), a.lin), sf = unerf_spacing_of(fminf(tmax, a.far0), a.lin);
    const float sn0 = unerf_spacing_of(a.near0, a.lin), inv = 1.f / (unerf_spacing_of(a.far0, a.lin) - sn0);
    for (int i = lane; i <= a.n; i += 64) {
        float b = a.row[i];
        // sf == sn (a miss, or an empty interval): every edge the same float, so all later lerps b0 + t (b1 - b0) and
        // interval lengths are exactly degenerate
        a.bins[r * (a.n + 1) + i] = ((sf == sn ? sn : (b * sf + (1.f - b) * sn)) - sn0) * inv;
    }
}

extern "C" int unerf_ray_box_bins(const float* origins, const float* directions, int64_t R, const float* world_to_box,
                                  const float* half_extent, float near, float far, int spacing, const float* sbins_row,
                                  int n, float* sbins, float* nears, float* fars, void* stream) {
    UNERF_REQUIRE(world_to_box && half_extent && (R == 0 || (origins && directions && sbins_row && sbins)), "ray_box_bins: null pointer");
    UNERF_REQUIRE(R >= 0 && n >= 1 && far > near && near >= 0.f, "ray_box_bins: R=%lld n=%d near=%g far=%g",
                  (long long)R, n, (double)near, (double)far);
    if (R == 0) return UNERF_OK;
    BoxBinsArgs a;
    for (int i = 0; i < 12; ++i) a.w2b[i] = world_to_box[i];
    for (int i = 0; i < 3; ++i) a.half[i] = half_extent[i];
    a.o = origins; a.d = directions; a.row = sbins_row; a.near0 = near; a.far0 = far; UNERF_REQUIRE_SPACING(spacing); a.lin = spacing; a.R = R; a.n = n;
    a.bins = sbins; a.nears = nears; a.fars = fars; a.in_nears = a.in_fars = nullptr;
    hipLaunchKernelGGL(box_bins_kernel, dim3(blocks_for(R, 4)), dim3(256), 0, (hipStream_t)stream, a);
    return unerf_check_launch("ray_box_bins");
}

extern "C" int unerf_ray_planes_bins(const float* nears, const float* fars, int64_t R, float near, float far,
                                     int spacing, const float* sbins_row, int n, float* sbins, void* stream) {
    UNERF_REQUIRE(R == 0 || (nears && fars && sbins_row && sbins), "ray_planes_bins: null pointer");
    UNERF_REQUIRE(R >= 0 && n >= 1 && far > near && near >= 0.f, "ray_planes_bins: R=%lld n=%d near=%g far=%g",
                  (long long)R, n, (double)near, (double)far);
    if (R == 0) return UNERF_OK;
    BoxBinsArgs a = {};
    a.row = sbins_row; a.near0 = near; a.far0 = far; UNERF_REQUIRE_SPACING(spacing); a.lin = spacing; a.R = R; a.n = n;
    a.bins = sbins; a.in_nears = nears; a.in_fars = fars;
    hipLaunchKernelGGL(box_bins_kernel, dim3(blocks_for(R, 4)), dim3(256), 0, (hipStream_t)stream, a);
    return unerf_check_launch("ray_planes_bins");
}

// ======================================================================================
// 2. stand-alone hash grid (parity surface for the index bookkeeping)
// ======================================================================================
__global__ __launch_bounds__(256) void hashgrid_kernel(const float* __restrict__ xyz, const float* __restrict__ table,
                                                       const float* __restrict__ scalings, int64_t N, int L, int log2T,
                                                       float* __restrict__ out, int32_t* __restrict__ out_idx) {
    int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float px = xyz[n * 3 + 0], py = xyz[n * 3 + 1], pz = xyz[n * 3 + 2];
    const uint32_t mask = (1u << log2T) - 1u;
    for (int l = 0; l < L; ++l) {
        const float2* lvl = reinterpret_cast<const float2*>(table) + ((size_t)l << log2T);
        float2 f = unerf_hash_level<true>(lvl, px, py, pz, scalings[l], mask);   // the reference's ceil / floor, any sign
        out[n * (2 * L) + 2 * l + 0] = f.x;
        out[n * (2 * L) + 2 * l + 1] = f.y;
        if (out_idx) {
            uint32_t idx[8];
            float ox, oy, oz;
            unerf_hash_corners<false, true>(px, py, pz, scalings[l], mask, idx, ox, oy, oz);
#pragma unroll
            for (int k = 0; k < 8; ++k) out_idx[(n * L + l) * 8 + k] = (int32_t)((idx[k] >> 3) + ((uint32_t)l << log2T));
        }
    }
}

extern "C" int unerf_hashgrid_fwd(const float* xyz, const float* table, const float* scalings, int64_t N, int L,
                                  int log2T, float* out, int32_t* out_idx, void* stream) {
    UNERF_REQUIRE(L >= 1 && L <= 32 && log2T >= 1 && log2T <= 24 && N >= 0, "hashgrid_fwd: bad L=%d log2T=%d", L, log2T);
    if (N == 0) return UNERF_OK;  // empty input: nothing to read or write (pointers may be null)
    UNERF_REQUIRE(xyz && table && scalings && out, "hashgrid_fwd: null pointer");
    hipLaunchKernelGGL(hashgrid_kernel, dim3(blocks_for(N, 256)), dim3(256), 0, (hipStream_t)stream, xyz, table,
                       scalings, N, L, log2T, out, out_idx);
    return unerf_check_launch("hashgrid_fwd");
}

__global__ __launch_bounds__(256) void hashgrid_tcnn_kernel(const float* __restrict__ xyz,
                                                            const float* __restrict__ params, TcnnLevels lv, int64_t N,
                                                            int L, float* __restrict__ out, int32_t* __restrict__ out_idx) {
    int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float px = xyz[n * 3 + 0], py = xyz[n * 3 + 1], pz = xyz[n * 3 + 2];
    for (int l = 0; l < L; ++l) {
        uint32_t rows[8];
        float wx, wy, wz;
        unerf_tcnn_corners(lv.v[l], px, py, pz, rows, wx, wy, wz);
        float2 f[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = reinterpret_cast<const float2*>(params)[rows[k]];
        float2 r = unerf_tcnn_blend(f, wx, wy, wz);
        out[n * (2 * L) + 2 * l + 0] = r.x;
        out[n * (2 * L) + 2 * l + 1] = r.y;
        if (out_idx) {
#pragma unroll
            for (int k = 0; k < 8; ++k) out_idx[(n * L + l) * 8 + k] = (int32_t)rows[k];
        }
    }
}

static int unerf_tcnn_levels_from_host(TcnnLevels& lv, const unerf_tcnn_level* levels_host, int L, const char* what) {
    for (int l = 0; l < L; ++l) {
        lv.v[l] = levels_host[l];
        UNERF_REQUIRE(lv.v[l].res >= 2 && lv.v[l].size >= 8 && (lv.v[l].dense || (lv.v[l].size & (lv.v[l].size - 1)) == 0),
                      "%s: level %d: res=%u size=%u (hashed levels need a power-of-two size)", what, l,
                      lv.v[l].res, lv.v[l].size);
    }
    return UNERF_OK;
}

extern "C" int unerf_hashgrid_fwd_tcnn(const float* xyz, const float* params, const unerf_tcnn_level* levels_host,
                                       int64_t N, int L, float* out, int32_t* out_idx, void* stream) {
    UNERF_REQUIRE(L >= 1 && L <= 32 && N >= 0, "hashgrid_fwd_tcnn: bad L=%d", L);
    if (N == 0) return UNERF_OK;
    UNERF_REQUIRE(xyz && params && levels_host && out, "hashgrid_fwd_tcnn: null pointer");
    TcnnLevels lv;
    if (int rc = unerf_tcnn_levels_from_host(lv, levels_host, L, "hashgrid_fwd_tcnn")) return rc;
    hipLaunchKernelGGL(hashgrid_tcnn_kernel, dim3(blocks_for(N, 256)), dim3(256), 0, (hipStream_t)stream, xyz, params,
                       lv, N, L, out, out_idx);
    return unerf_check_launch("hashgrid_fwd_tcnn");
}

// the same lookup in tcnn's own half arithmetic: params_half = the half copy of the parameter vector, [rows] half2
__global__ __launch_bounds__(256) void hashgrid_tcnn_half_kernel(const float* __restrict__ xyz,
                                                                 const void* __restrict__ params_half, TcnnLevels lv, int64_t N,
                                                                 int L, float* __restrict__ out) {
    int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float px = xyz[n * 3 + 0], py = xyz[n * 3 + 1], pz = xyz[n * 3 + 2];
    for (int l = 0; l < L; ++l) {
        uint32_t rows[8], c8[8];
        float wx, wy, wz;
        unerf_tcnn_corners(lv.v[l], px, py, pz, rows, wx, wy, wz);
#pragma unroll
        for (int k = 0; k < 8; ++k) c8[k] = reinterpret_cast<const uint32_t*>(params_half)[rows[k]];
        const float2 r = unerf_h2_to_float2(unerf_tcnn_blend_half(c8, wx, wy, wz));
        out[n * (2 * L) + 2 * l + 0] = r.x;
        out[n * (2 * L) + 2 * l + 1] = r.y;
    }
}

extern "C" int unerf_hashgrid_fwd_tcnn_half(const float* xyz, const void* params_half, const unerf_tcnn_level* levels_host,
                                            int64_t N, int L, float* out, void* stream) {
    UNERF_REQUIRE(L >= 1 && L <= 32 && N >= 0, "hashgrid_fwd_tcnn_half: bad L=%d", L);
    if (N == 0) return UNERF_OK;
    UNERF_REQUIRE(xyz && params_half && levels_host && out, "hashgrid_fwd_tcnn_half: null pointer");
    TcnnLevels lv;
    if (int rc = unerf_tcnn_levels_from_host(lv, levels_host, L, "hashgrid_fwd_tcnn_half")) return rc;
    hipLaunchKernelGGL(hashgrid_tcnn_half_kernel, dim3(blocks_for(N, 256)), dim3(256), 0, (hipStream_t)stream, xyz,
                       params_half, lv, N, L, out);
    return unerf_check_launch("hashgrid_fwd_tcnn_half");
}

// ======================================================================================
// 3. proposal density: positions -> contraction -> hash grid (L levels) -> MLP(2L->HID->1)
// ======================================================================================
struct PropArgs {
    const float* origins;
    const float* dirs;
    const float* sbins;
    int64_t sstride;
    int64_t R;
    int n;
    float s_near, s_far;
    int lin;   // UNERF_SPACING_*: 1 = identity spacing (UniformSampler)
    unerf_density_net net;
    float avg;
    float* out;
    FastDiv fd;  // by n; used when R * n < 2^31
    int small;
    // Pixel-patch schedule (image_width hint): a workgroup = an 8x8 pixel patch x a group of consecutive sample indices
    // (prop_density_kernel: 4, one per wave; prop_patch_kernel: 16, four per wave, walked one after the other),
    // a wave = the 64 pixels of the patch at ONE sample index.  Neighbouring pixels at equal depth sit in the
    // same one or two grid cells, so a gather instruction touches a handful of cache lines instead of the
    // ~20 of 64 consecutive samples along one ray (the proposal kernels saturate the texture-address unit).
    uint32_t img_w, pcols, nsg, nblocks;   // img_w = 0: linear schedule; nsg = sample groups per patch, ceil(n / 4) or ceil(n / 16), set per kernel on the host; nblocks: workgroups of the patch schedule
    FastDiv div_nsg, div_pcols;
    int64_t g0, first_row;
    int vec4;   // prop_patch_kernel: n % 4 == 0 and density_out 16-byte aligned
    unerf_norm_box box;
};

template <int L, int HID>
__global__ __launch_bounds__(256) void prop_density_kernel(PropArgs a) {
    int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t r;
    int i;
    if (a.img_w) {  // uniform
        const uint32_t patch = fastdiv(blockIdx.x, a.div_nsg), sg = blockIdx.x - patch * a.nsg;
        const uint32_t band = fastdiv(patch, a.div_pcols), pc = patch - band * a.pcols;
        const uint32_t lane = threadIdx.x & 63u;
        const uint32_t x = pc * 8u + (lane & 7u);
        const int64_t y = a.first_row + (int64_t)band * 8 + (lane >> 3);
        r = y * (int64_t)a.img_w + x - a.g0;
        i = (int)(sg * 4u + (threadIdx.x >> 6));
        if (x >= a.img_w || r < 0 || r >= a.R || i >= a.n) return;
        idx = r * a.n + i;
    } else if (idx >= a.R * a.n) {
        return;
    } else if (a.small) {  // uniform
        const uint32_t r32 = fastdiv((uint32_t)idx, a.fd);
        r = r32;
        i = (int)((uint32_t)idx - r32 * (uint32_t)a.n);
    } else {
        r = idx / a.n;
        i = (int)(idx - r * a.n);
    }
    const float* sb = a.sbins + r * a.sstride;
    float e0 = unerf_s2e(sb[i], a.s_near, a.s_far, a.lin);
    float e1 = unerf_s2e(sb[i + 1], a.s_near, a.s_far, a.lin);
    float t = e0 + e1;
    float px = a.origins[r * 3 + 0] + a.dirs[r * 3 + 0] * t / 2.f;
    float py = a.origins[r * 3 + 1] + a.dirs[r * 3 + 1] * t / 2.f;
    float pz = a.origins[r * 3 + 2] + a.dirs[r * 3 + 2] * t / 2.f;
    float sel = unerf_normalize_position(px, py, pz, a.box);
    const uint32_t mask = (1u << a.net.log2T) - 1u;
    float feat[2 * L];
#pragma unroll
    for (int l = 0; l < L; ++l) {
        float2 f;
        if (a.net.tcnn_levels && a.net.grid_half) {  // uniform: tcnn layout, half2 rows, tcnn's half arithmetic
            f = unerf_tcnn_level_feat_half(a.net.table, a.net.tcnn_levels[l], px, py, pz);
        } else if (a.net.tcnn_levels) {  // uniform: tcnn-layout grid
            f = unerf_tcnn_level_feat(reinterpret_cast<const float2*>(a.net.table), a.net.tcnn_levels[l], px, py, pz);
        } else if (l < a.net.n_dense) {  // wave-uniform: coarse level with a dense, x-paired copy
            f = unerf_dense_level<true>(reinterpret_cast<const float4*>(a.net.dense) + a.net.dense_off[l], a.net.dense_dim[l],
                                        px, py, pz, a.net.scalings[l]);
        } else {
            const float2* lvl = reinterpret_cast<const float2*>(a.net.table) + ((size_t)l << a.net.log2T);
            f = unerf_hash_level<false, true>(lvl, px, py, pz, a.net.scalings[l], mask);
        }
        feat[2 * l] = f.x;
        feat[2 * l + 1] = f.y;
    }
    const float* __restrict__ w0t = a.net.w0t;
    const float* __restrict__ b0 = a.net.b0;
    const float* __restrict__ w1t = a.net.w1t;
    float o = a.net.b1[0];
    if constexpr (HID == 0) {
        // use_linear=True (HashMLPDensityField: `self.linear = nn.Linear(encoding.get_out_dim(), 1)` straight on the grid
        // features, no hidden layer): w1t = that layer's 2L weights
#pragma unroll
        for (int k = 0; k < 2 * L; ++k) o = fmaf(feat[k], w1t[k], o);
    } else {
    // two hidden units per v_pk_fma_f32 (each half is an IEEE fma, same bits as fmaf): the kernel is
    // VALU-issue-bound, and the MLP was a third of its instructions.  Weights arrive as SGPR pairs.
    static_assert(HID % 2 == 0, "hidden width must be even");
    const unerf_v2f* __restrict__ w0p = reinterpret_cast<const unerf_v2f*>(w0t);
    const unerf_v2f* __restrict__ b0p = reinterpret_cast<const unerf_v2f*>(b0);
    unerf_v2f h2[HID / 2 + 1];
#pragma unroll
    for (int j = 0; j < HID / 2; ++j) h2[j] = b0p[j];
#pragma unroll
    for (int k = 0; k < 2 * L; ++k) {
        const unerf_v2f fk = {feat[k], feat[k]};
#pragma unroll
        for (int j = 0; j < HID / 2; ++j) h2[j] = __builtin_elementwise_fma(fk, w0p[k * (HID / 2) + j], h2[j]);
    }
#pragma unroll
    for (int j = 0; j < HID / 2; ++j) {  // ReLU as an integer max on the bit pattern (one op, see mf_relu)
        o = fmaf(__int_as_float(max(__float_as_int(h2[j].x), 0)), w1t[2 * j], o);
        o = fmaf(__int_as_float(max(__float_as_int(h2[j].y), 0)), w1t[2 * j + 1], o);
    }
    }
    a.out[idx] = a.avg * unerf_exp(o) * sel;
}

// Patch-schedule form of prop_density_kernel with the per-RAY work done once per lane.  A workgroup is an 8x8 pixel
// patch x 16 consecutive sample indices; wave wv owns samples i_base + 4 wv + q, q = 0..3, and a lane keeps ITS ray for
// all four.  A wave is still the 64 pixels of the patch at one sample index per gather (the locality the schedule is
// for), but the block decode, the ray, the barrier and the store are paid once per four samples instead of once per
// sample (docs/experiments.md 8.7):
//   * ray: one wave loads the 64 origins / directions (a ray-indexed access costs the texture path one cache line
//     per LANE), every lane reads its own back from LDS (per sample: six more registers live across the loop cost
//     the L = 8 instances a wave per SIMD, and measured the same at L = 5);
//   * bin edges, own rows: every raw edge of the block is loaded once -- a lane loads the four edges its samples
//     start at (one 16-byte load when the row allows) and takes the fifth from the next wave through LDS (the last
//     wave loads it) -- and converted once per lane: five conversions (an IEEE division each) for four samples
//     where a sample alone needs two; shared row: 17 lanes convert the block's edges once for the workgroup;
//   * output: the lane's four adjacent densities leave as one 16-byte store when n % 4 == 0 and the output is
//     aligned, as dwords otherwise; samples >= n are neither computed nor stored.
// The sample loop is a real loop, rolled (asked for 2 or 4 copies the compiler emits this same listing, 8.7); t and the
// density go through a lane-private LDS slot so that no register array is indexed by the loop counter.  unerf_s2e of
// the same edge gives the same bits whoever converts it, and the per-sample arithmetic is prop_density_kernel's on the
// same values: bit-identical to it.
constexpr int PROP_WALK = 4;          // consecutive samples per lane
template <int L, int HID>
__global__ __launch_bounds__(256) void prop_patch_kernel(PropArgs a) {
    __shared__ float s_od[6][64];
    __shared__ float s_e[4][64];             // own rows: [wave][lane] the first raw edge of each wave; shared row: 17 Euclidean edges
    __shared__ float s_io[4][PROP_WALK][64];  // [wave][q][lane]: t of sample q, then its density (lane-private)
    // XCD-aware order: workgroups go to the 8 XCDs round-robin; every XCD takes a CONTIGUOUS
    // eighth of the (patch, sample group) list -- a band of the image -- instead of every eighth workgroup, so the grid lines
    // neighbouring patches share are fetched into one L2 instead of all eight.  Pure scheduling: same values per sample.
    const uint32_t per = (gridDim.x + 7u) >> 3, bid = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
    if (bid >= a.nblocks) return;
    const uint32_t patch = fastdiv(bid, a.div_nsg), sg = bid - patch * a.nsg;
    const uint32_t band = fastdiv(patch, a.div_pcols), pc = patch - band * a.pcols;
    const uint32_t lane = threadIdx.x & 63u, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // uniform, and known to be: the sample loop's trip count hangs on it
    const uint32_t x = pc * 8u + (lane & 7u);
    const int64_t y = a.first_row + (int64_t)band * 8 + (lane >> 3);
    int64_t r = y * (int64_t)a.img_w + x - a.g0;
    const bool ray_ok = x < a.img_w && r >= 0 && r < a.R;
    if (!ray_ok) r = 0;
    const int i_base = (int)(sg * (4u * PROP_WALK));
    const int i0 = i_base + (int)wv * PROP_WALK;   // this wave's first sample
    const int nq = min(PROP_WALK, a.n - i0);       // its live samples (<= 0: none); uniform
    float raw[PROP_WALK + 1];                      // own rows: the lane's raw edges i0 .. i0 + 4 (index clamped to n)
    {   // stage: wave 0 the ray; the bin edges by every wave (own rows) or by 17 lanes of wave 1 (shared row)
        if (wv == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                s_od[c][lane] = a.origins[r * 3 + c];
                s_od[3 + c][lane] = a.dirs[r * 3 + c];
            }
        }
        if (a.sstride == 0) {
            // one shared row of bin edges (the 256 initial bins): the Euclidean edges are the same for every ray, so
            // 17 lanes convert the block's ONCE for the workgroup (a conversion is an IEEE division and the kernel is
            // VALU-issue bound) and every lane reads them back
            if (wv == 1) {
                const float e = unerf_s2e(a.sbins[min(i_base + (int)min(lane, 16u), a.n)], a.s_near, a.s_far, a.lin);
                if (lane <= 16u) s_e[0][lane] = e;
            }
        } else {
            const float* sb = a.sbins + r * a.sstride;
            if (i0 + PROP_WALK <= a.n) {  // uniform
                struct __attribute__((packed, aligned(4))) Q { float x, y, z, w; };
                const Q q = *reinterpret_cast<const Q*>(sb + i0);
                raw[0] = q.x; raw[1] = q.y; raw[2] = q.z; raw[3] = q.w;
            } else {
#pragma unroll
                for (int e = 0; e < PROP_WALK; ++e) raw[e] = sb[min(i0 + e, a.n)];
            }
            if (wv == 3) raw[PROP_WALK] = sb[min(i0 + PROP_WALK, a.n)];
            s_e[wv][lane] = raw[0];
        }
    }
    __syncthreads();
    if (nq <= 0 || !ray_ok) return;   // behind the only barrier
    float* io = &s_io[wv][0][lane];
    {   // t of the lane's samples: the sum of the two Euclidean edges of each, every edge converted once
        float e[PROP_WALK + 1];
        if (a.sstride == 0) {  // uniform: already Euclidean (same bits)
#pragma unroll
            for (int k = 0; k <= PROP_WALK; ++k) e[k] = s_e[0][wv * PROP_WALK + k];
        } else {
            if (wv != 3) raw[PROP_WALK] = s_e[wv + 1][lane];
#pragma unroll
            for (int k = 0; k <= PROP_WALK; ++k) e[k] = unerf_s2e(raw[k], a.s_near, a.s_far, a.lin);
        }
#pragma unroll
        for (int q = 0; q < PROP_WALK; ++q) io[q * 64] = e[q] + e[q + 1];
    }
#pragma unroll 1
    for (int q = 0; q < nq; ++q) {
        // The net as this iteration sees it: read from the kernel arguments at an opaque offset 0 (an empty asm that
        // takes q), so that its fields and what hangs on them (weight and scaling loads, level base pointers, the layout
        // conditions) are loaded and computed where they are used, as in the straight-line form.  Hoisted in front of
        // the loop they stay live across the whole body, spill SGPRs to a VGPR (one v_readlane per use) and cost a
        // wave per SIMD.  The asm is not volatile and clobbers nothing: the uniform loads stay scalar loads.
        int zero = 0;
        asm("" : "+s"(zero) : "s"(q));
        const unerf_density_net& net = (&a.net)[zero];
        const float* od = &s_od[0][lane + zero];   // the ray, read here for the same reason (registers, not SGPRs)
        const float ox = od[0], oy = od[64], oz = od[128], dx = od[192], dy = od[256], dz = od[320];
        const float t = io[q * 64];
        float px = ox + dx * t / 2.f;
        float py = oy + dy * t / 2.f;
        float pz = oz + dz * t / 2.f;
        const float sel = unerf_normalize_position(px, py, pz, a.box);
        const uint32_t mask = (1u << net.log2T) - 1u;
        float feat[2 * L];
#pragma unroll
        for (int l = 0; l < L; ++l) {
            float2 f;
            if (net.tcnn_levels && net.grid_half) {  // uniform: tcnn layout, half2 rows, tcnn's half arithmetic
                f = unerf_tcnn_level_feat_half(net.table, net.tcnn_levels[l], px, py, pz);
            } else if (net.tcnn_levels) {  // uniform: tcnn-layout grid
                f = unerf_tcnn_level_feat(reinterpret_cast<const float2*>(net.table), net.tcnn_levels[l], px, py, pz);
            } else if (l < net.n_dense) {  // wave-uniform: coarse level with a dense, x-paired copy
                f = unerf_dense_level<true>(reinterpret_cast<const float4*>(net.dense) + net.dense_off[l], net.dense_dim[l],
                                            px, py, pz, net.scalings[l]);
            } else {
                const float2* lvl = reinterpret_cast<const float2*>(net.table) + ((size_t)l << net.log2T);
                f = unerf_hash_level<false, true>(lvl, px, py, pz, net.scalings[l], mask);
            }
            feat[2 * l] = f.x;
            feat[2 * l + 1] = f.y;
        }
        const float* __restrict__ w1t = net.w1t;
        float o = net.b1[0];
        if constexpr (HID == 0) {   // use_linear=True: one Linear on the grid features (see prop_density_kernel)
#pragma unroll
            for (int k = 0; k < 2 * L; ++k) o = fmaf(feat[k], w1t[k], o);
        } else {
        static_assert(HID % 2 == 0, "hidden width must be even");
        const unerf_v2f* __restrict__ w0p = reinterpret_cast<const unerf_v2f*>(net.w0t);
        const unerf_v2f* __restrict__ b0p = reinterpret_cast<const unerf_v2f*>(net.b0);
        unerf_v2f h2[HID / 2 + 1];
#pragma unroll
        for (int j = 0; j < HID / 2; ++j) h2[j] = b0p[j];
#pragma unroll
        for (int k = 0; k < 2 * L; ++k) {
            const unerf_v2f fk = {feat[k], feat[k]};
#pragma unroll
            for (int j = 0; j < HID / 2; ++j) h2[j] = __builtin_elementwise_fma(fk, w0p[k * (HID / 2) + j], h2[j]);
        }
        // [probe:prop-mlp-out begin]  (benchmarks/probe_source.py rewrites the marked span in COPIES of this file)
#pragma unroll
        for (int j = 0; j < HID / 2; ++j) {
            o = fmaf(__int_as_float(max(__float_as_int(h2[j].x), 0)), w1t[2 * j], o);
            o = fmaf(__int_as_float(max(__float_as_int(h2[j].y), 0)), w1t[2 * j + 1], o);
        }
        // [probe:prop-mlp-out end]
        }
        io[q * 64] = a.avg * unerf_exp(o) * sel;
    }
    float* out = a.out + r * a.n + i0;
    if (a.vec4) {  // uniform: n % 4 == 0 (so nq == 4) and a 16-byte aligned output: the ray's 4 densities leave as one store
        *reinterpret_cast<float4*>(out) = make_float4(io[0], io[64], io[128], io[192]);
    } else {
#pragma unroll
        for (int q = 0; q < PROP_WALK; ++q)
            if (q < nq) out[q] = io[q * 64];
    }
}

extern "C" int unerf_proposal_density(const float* origins, const float* directions, const float* sbins,
                                      int64_t sbins_stride, int64_t R, int n, float near_plane, float far_plane, int spacing,
                                      const unerf_density_net* net, float average_init_density, float* density_out,
                                      int64_t ray_offset, int image_width, void* stream) {
    UNERF_REQUIRE(net && (R == 0 || (origins && directions && sbins && density_out)), "proposal_density: null pointer");
    UNERF_REQUIRE(net->table && (net->scalings || net->tcnn_levels) && (net->hidden == 0 || (net->w0t && net->b0)) && net->w1t && net->b1,
                  "proposal_density: null pointer inside unerf_density_net");
    UNERF_REQUIRE(R >= 0 && n >= 1, "proposal_density: bad R/n");
    UNERF_REQUIRE(sbins_stride == 0 || sbins_stride >= n + 1, "proposal_density: sbins_stride %lld < n+1",
                  (long long)sbins_stride);
    UNERF_REQUIRE(net->tcnn_levels || (net->log2T >= 1 && net->log2T <= 24), "proposal_density: bad log2T");
    UNERF_REQUIRE(net->n_dense >= 0 && net->n_dense <= 8 && net->n_dense <= net->L && (net->n_dense == 0 || net->dense),
                  "proposal_density: bad dense level description");
    for (int l = 0; l < net->n_dense; ++l)  // a level is addressed with 32-bit byte offsets
        UNERF_REQUIRE(net->dense_dim[l] >= 2 && net->dense_dim[l] <= 640, "proposal_density: dense_dim[%d]=%d outside [2,640]",
                      l, net->dense_dim[l]);
    if (R == 0) return UNERF_OK;
    PropArgs a;
    a.origins = origins; a.dirs = directions; a.sbins = sbins; a.sstride = sbins_stride; a.R = R; a.n = n;
    if (int rc = set_spacing(a, near_plane, far_plane, spacing)) return rc;
    a.net = *net; a.avg = average_init_density; a.out = density_out;
    a.box = make_norm_box(net->use_aabb, net->aabb);
    a.fd = make_fastdiv((uint32_t)n); a.small = (R * (int64_t)n < (1ll << 31)) ? 1 : 0;
    a.img_w = 0; a.pcols = 0; a.nsg = 0; a.nblocks = 0; a.div_nsg = a.div_pcols = make_fastdiv(1); a.g0 = 0; a.first_row = 0;
    a.vec4 = (n % 4 == 0 && ((uintptr_t)density_out & 15u) == 0) ? 1 : 0;
    dim3 grid(blocks_for(R * (int64_t)n, 256)), block(256);
    // image-ordered rays: the LDS-staged patch kernel; anything else (or UNERF_NO_PATCH_KERNEL): one thread per sample
    const bool patch_kernel = !getenv("UNERF_NO_PATCH_KERNEL");
    if (image_width >= 8 && R >= 8 * (int64_t)image_width && ray_offset >= 0) {  // at least one full 8-row band
        const int64_t band0 = (ray_offset / image_width) / 8, band1 = ((ray_offset + R - 1) / image_width) / 8;
        const int64_t per_group = patch_kernel ? 4 * PROP_WALK : 4;   // sample indices per workgroup: the kernels' own decode
        const int64_t pcols = (image_width + 7) / 8, nsg = (n + per_group - 1) / per_group;
        const int64_t blocks = (band1 - band0 + 1) * pcols * nsg;
        if (blocks < (1ll << 31)) {
            a.img_w = (uint32_t)image_width; a.pcols = (uint32_t)pcols; a.nsg = (uint32_t)nsg;
            a.div_nsg = make_fastdiv((uint32_t)nsg); a.div_pcols = make_fastdiv((uint32_t)pcols);
            a.g0 = ray_offset; a.first_row = band0 * 8;
            a.nblocks = (uint32_t)blocks;
            grid = dim3((unsigned)(((blocks + 7) / 8) * 8));
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const bool patch = a.img_w != 0 && patch_kernel;
    // both kernels are built for L in {5, 8} levels x a hidden width in {16, 64, 0}; 0: use_linear=True
    bool built = false;
    with_int<5, 8>(net->L, [&](auto L) {
        built = with_int<16, 64, 0>(net->hidden, [&](auto hidden) {
            const auto kernel = patch ? prop_patch_kernel<decltype(L)::value, decltype(hidden)::value>
                                      : prop_density_kernel<decltype(L)::value, decltype(hidden)::value>;
            hipLaunchKernelGGL(kernel, grid, block, 0, st, a);
        });
    });
    UNERF_REQUIRE(built, "proposal_density: unsupported (L=%d, hidden=%d); built: (5,16) (5,64) (8,16) (8,64) (5,0) (8,0)", net->L,
                  net->hidden);
    return unerf_check_launch("proposal_density");
}

// ======================================================================================
// 4. weights + PDF resampling: a wave (n > 128) or a 16-lane group (n <= 128) per ray, lane owns EPL consecutive samples
// ======================================================================================
struct PdfArgs {
    const float* density;
    const float* sbins;
    int64_t sstride;
    int64_t R;
    int n;
    float s_near, s_far;
    int lin;   // UNERF_SPACING_*: 1 = identity spacing (UniformSampler)
    const float* u;
    int m;
    float pad, eps;
    float* sbins_out;
    float* prop_depth;
    float* weights_out;
    float* clip;
    int64_t ray_offset, chunk_rays;
};

#define PDF_MAXN 256

#define PDF_RAYS_PER_BLOCK 32

// Each wave of the pdf kernel works on its own LDS rows, and a wave's DS operations complete in issue
// order, so a compiler-level fence is all the "barrier" it needs; the four waves of a block are then
// free to drift apart and hide one another's latency (s_barrier kept them in lock-step).
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Thousands of rays share one chunk word: peek first (L2-coherent relaxed load) and only send the atomic
// when it can still win -- a stale peek merely costs a redundant atomic, never a wrong result.
__device__ __forceinline__ void pdf_clip_commit(float* clip, int64_t chunk, unsigned int lo, unsigned int hi) {
    unsigned int* c = reinterpret_cast<unsigned int*>(clip) + chunk * 2;
    if (lo < __hip_atomic_load(c + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(c + 0, lo);
    if (hi > __hip_atomic_load(c + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(c + 1, hi);
}

template <int EPL, typename... VW>   // VW = ViewMap: the clip rows are numbered per view (unerf_weights_pdf_resample_views)
__global__ __launch_bounds__(256) void pdf_kernel(PdfArgs a, VW... vw) {
    __shared__ float s_sb[4][PDF_MAXN + 4];
    __shared__ float s_cdf[4][PDF_MAXN + 4];
    __shared__ float s_nb[4][PDF_MAXN + 4];
    __shared__ unsigned int s_clip[4][2];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = a.n, nb = a.m + 1;
    const int top_step = 1 << (31 - __builtin_clz((unsigned)n));   // largest power of two <= n
    // A block walks PDF_RAYS_PER_BLOCK consecutive rays, four (one per wave) at a time, and keeps the
    // running min/max of the first/last sample positions in registers: one peek + atomic per block and
    // chunk instead of one per ray (2 M same-address L2 reads per frame made this kernel 3.5 ms).
    int64_t cur_chunk = -1;
    unsigned int cmin = 0x7F800000u, cmax = 0u;
    // One shared row of bin edges (sstride == 0: the 256 initial bins): its Euclidean edges are the same for every ray,
    // so each wave converts them ONCE per block into its own LDS row (one conversion = an IEEE division, ~15
    // instructions; per ray that was EPL + 1 of them per lane) and the raw row is staged once as well.  Same values.
    __shared__ float s_eu[4][PDF_MAXN + 4];
    const bool shared_row = a.sstride == 0;
    if (shared_row) {
        for (int k = lane; k <= n; k += 64) {
            const float b = a.sbins[k];
            s_sb[wv][k] = b;
            s_eu[wv][k] = unerf_s2e(b, a.s_near, a.s_far, a.lin);
        }
    }
    for (int it = 0; it < PDF_RAYS_PER_BLOCK / 4; ++it) {
    int64_t r = (int64_t)blockIdx.x * PDF_RAYS_PER_BLOCK + it * 4 + wv;
    const bool ray_ok = r < a.R;
    if (!ray_ok) r = a.R - 1;  // keep the wave alive for the block barrier at the end
    wave_lds_sync();           // previous ray's LDS rows are free again
    if (!shared_row) {
        const float* sb = a.sbins + r * a.sstride;
        for (int k = lane; k <= n; k += 64) s_sb[wv][k] = sb[k];
    }
    wave_lds_sync();

    float eu[EPL + 1], w[EPL], dd[EPL];
    const int k0 = lane * EPL;
    if (shared_row) {
#pragma unroll
        for (int e = 0; e <= EPL; ++e) eu[e] = s_eu[wv][min(k0 + e, n)];
    } else {
#pragma unroll
        for (int e = 0; e <= EPL; ++e) eu[e] = unerf_s2e(s_sb[wv][min(k0 + e, n)], a.s_near, a.s_far, a.lin);
    }
    float lsum = 0.f, lexcl[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int k = k0 + e;
        float dens = (k < n) ? a.density[r * n + k] : 0.f;
        dd[e] = (k < n) ? (eu[e + 1] - eu[e]) * dens : 0.f;
        lexcl[e] = lsum;
        lsum += dd[e];
    }
    float carry = group_excl_scan<64>(lsum, lane);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        float alpha = 1.f - unerf_exp(-dd[e]);
        float T = unerf_exp(-(carry + lexcl[e]));
        w[e] = (k0 + e < n) ? unerf_nan_to_num(alpha * T) : 0.f;
        if (a.weights_out && ray_ok && k0 + e < n) a.weights_out[r * n + k0 + e] = w[e];
    }
    // median depth of this level (prop_depth_i)
    if (a.prop_depth) {
        float ls = 0.f, lc[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            ls += w[e];
            lc[e] = ls;
        }
        float cbase = group_excl_scan<64>(ls, lane);
        int cnt = 0;
#pragma unroll
        for (int e = 0; e < EPL; ++e) cnt += (k0 + e < n && (cbase + lc[e]) < 0.5f) ? 1 : 0;
        cnt = group_sum_i<64>(cnt);
        int idx = min(cnt, n - 1);
        int owner = idx / EPL, slot = idx - owner * EPL;
        float val = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            float st = (eu[e] + eu[e + 1]) / 2.f;
            float got = __shfl(st, owner, 64);
            if (e == slot) val = got;
        }
        if (lane == 0 && ray_ok) a.prop_depth[r] = val;
    }
    // histogram -> pdf -> cdf
    float wp[EPL], lw = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        wp[e] = (k0 + e < n) ? w[e] + a.pad : 0.f;
        lw += wp[e];
    }
    float wsum = group_sum<64>(lw);
    float padding = fmaxf(a.eps - wsum, 0.f);
    float padn = padding / (float)n;
    wsum += padding;
    float lp = 0.f, lcdf[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        float pdf = (k0 + e < n) ? (wp[e] + padn) / wsum : 0.f;
        lp += pdf;
        lcdf[e] = lp;
    }
    float cb = group_excl_scan<64>(lp, lane);
    if (lane == 0) s_cdf[wv][0] = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e)
        if (k0 + e < n) s_cdf[wv][k0 + e + 1] = fminf(1.f, cb + lcdf[e]);
    wave_lds_sync();

    for (int j = lane; j < nb; j += 64) {
        float u = a.u[j];
        // searchsorted(cdf[0..n], u, side="right") = 1 + the last index with cdf <= u (cdf[0] = 0 <= u): descend
        // by powers of two without a data-dependent loop -- 5 instructions per step against ~9 for the
        // lo / hi / mid form, and the kernel is VALU-issue bound.  A probe past the end is clamped to n, whose
        // entry is an ordinary candidate, so the result is the same index.
        int pos = 0;
        for (int step = top_step; step > 0; step >>= 1) {   // uniform trip count
            const int probe = min(pos + step, n);
            pos = (s_cdf[wv][probe] <= u) ? probe : pos;
        }
        const int lo = pos + 1;
        int below = min(max(lo - 1, 0), n), above = min(max(lo, 0), n);
        float g0 = s_cdf[wv][below], g1 = s_cdf[wv][above];
        float b0 = s_sb[wv][below], b1 = s_sb[wv][above];
        float t = (u - g0) / (g1 - g0);
        t = unerf_nan_to_num(t);
        t = fminf(fmaxf(t, 0.f), 1.f);
        float v = b0 + t * (b1 - b0);
        s_nb[wv][j] = v;
        if (ray_ok) a.sbins_out[r * nb + j] = v;
    }
    if (a.clip) {
        wave_lds_sync();
        if (ray_ok) {  // wave-uniform
            // the four edges (first two, last two) converted by lanes 0..3 at once, one conversion stream instead of four
            const int ei = (lane & 2) ? nb - 2 + (lane & 1) : (lane & 1);
            const float ev = unerf_s2e(s_nb[wv][ei], a.s_near, a.s_far, a.lin);
            const float f0 = __shfl(ev, 0, 64), f1 = __shfl(ev, 1, 64), l0 = __shfl(ev, 2, 64), l1 = __shfl(ev, 3, 64);
            float first = (f0 + f1) / 2.f, last = (l0 + l1) / 2.f;
            const int64_t chunk = clip_chunk(a, r, vw...);
            if (chunk != cur_chunk) {
                if (cur_chunk >= 0 && lane == 0) pdf_clip_commit(a.clip, cur_chunk, cmin, cmax);
                cur_chunk = chunk;
                cmin = 0x7F800000u;
                cmax = 0u;
            }
            // positive floats order like their bit patterns
            cmin = min(cmin, __float_as_uint(first));
            cmax = max(cmax, __float_as_uint(last));
        }
    }
    }  // rays of this block
    if (a.clip) {
        // the four waves normally sit in one chunk: merge them through LDS and send one update
        const int64_t blk_chunk = clip_chunk(a, (int64_t)blockIdx.x * PDF_RAYS_PER_BLOCK, vw...);
        const bool mergeable = cur_chunk == blk_chunk;  // this wave never left the block's first chunk
        if (lane == 0) {
            s_clip[wv][0] = mergeable ? cmin : 0x7F800000u;
            s_clip[wv][1] = mergeable ? cmax : 0u;
            if (!mergeable && cur_chunk >= 0) pdf_clip_commit(a.clip, cur_chunk, cmin, cmax);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned int lo = min(min(s_clip[0][0], s_clip[1][0]), min(s_clip[2][0], s_clip[3][0]));
            unsigned int hi = max(max(s_clip[0][1], s_clip[1][1]), max(s_clip[2][1], s_clip[3][1]));
            if (lo != 0x7F800000u || hi != 0u) pdf_clip_commit(a.clip, blk_chunk, lo, hi);
        }
    }
}

// The grouped form (n <= 128): a ray belongs to a group of PDF_GROUP = 16 lanes -- one DPP row, as in composite_kernel --
// so a wave holds four rays and a block trip sixteen; lane l of a group owns the samples [l EPL, (l + 1) EPL),
// EPL = ceil(n / 16).  What a ray costs once -- two sums, the median, the padding division, the clip -- is then paid once
// per wave for four rays.  Every value comes from the formulas of pdf_kernel in the same order inside a lane; only the
// cross-lane sums associate differently (group_*<16>).
// LDS is sized by the launch (pdf_group_lds_bytes): one CDF row per group, and one row of bin edges per group or -- the
// shared row, sstride == 0 -- that row and its Euclidean copy once per block.  The new bins are not staged: the clip
// takes the first two and the last two from the lanes that made them.
__host__ __device__ inline int pdf_row_stride(int n) { return (n + 1) | 1; }   // odd: the groups' rows start on different banks
#define PDF_GROUP 16
static inline size_t pdf_group_lds_bytes(int n, bool shared_row) {
    const int groups = 256 / PDF_GROUP;
    return (size_t)(shared_row ? groups + 2 : 2 * groups) * pdf_row_stride(n) * sizeof(float);
}

template <int EPL, typename... VW>
__global__ __launch_bounds__(256) void pdf_group_kernel(PdfArgs a, VW... vw) {
    constexpr int G = PDF_GROUP;
    constexpr int NG = 256 / G;   // groups of a block = rays of a block trip
    static_assert(PDF_RAYS_PER_BLOCK % NG == 0, "whole trips");
    extern __shared__ float s_rows[];
    __shared__ unsigned int s_clip[NG][2];
    const int lane = threadIdx.x & 63, gl = lane & (G - 1), grp = threadIdx.x / G;
    const int n = a.n, nb = a.m + 1, rs = pdf_row_stride(n);
    const int top_step = 1 << (31 - __builtin_clz((unsigned)n));   // largest power of two <= n
    const bool shared_row = a.sstride == 0;
    float* const s_cdf = s_rows + grp * rs;
    float* const s_sb = s_rows + (shared_row ? NG : NG + grp) * rs;
    float* const s_eu = s_rows + (NG + 1) * rs;   // shared row only
    if (shared_row) {
        for (int k = threadIdx.x; k <= n; k += 256) {
            const float b = a.sbins[k];
            s_sb[k] = b;
            s_eu[k] = unerf_s2e(b, a.s_near, a.s_far, a.lin);
        }
        __syncthreads();
    }
    // the running clip bounds of this GROUP's rays (its lane 0 keeps them), merged per block at the end as in pdf_kernel
    int64_t cur_chunk = -1;
    unsigned int cmin = 0x7F800000u, cmax = 0u;
    for (int it = 0; it < PDF_RAYS_PER_BLOCK / NG; ++it) {
    int64_t r = (int64_t)blockIdx.x * PDF_RAYS_PER_BLOCK + it * NG + grp;
    const bool ray_ok = r < a.R;
    if (!ray_ok) r = a.R - 1;  // a group past the last ray re-runs ray R - 1 with its stores switched off
    wave_lds_sync();           // the rows of a wave's groups are read by that wave alone
    if (!shared_row) {
        const float* sb = a.sbins + r * a.sstride;
        for (int k = gl; k <= n; k += G) s_sb[k] = sb[k];
        wave_lds_sync();
    }

    float eu[EPL + 1], w[EPL], dd[EPL];
    const int k0 = gl * EPL;
    if (shared_row) {
#pragma unroll
        for (int e = 0; e <= EPL; ++e) eu[e] = s_eu[min(k0 + e, n)];
    } else {
#pragma unroll
        for (int e = 0; e <= EPL; ++e) eu[e] = unerf_s2e(s_sb[min(k0 + e, n)], a.s_near, a.s_far, a.lin);
    }
    float lsum = 0.f, lexcl[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int k = k0 + e;
        float dens = (k < n) ? a.density[r * n + k] : 0.f;
        dd[e] = (k < n) ? (eu[e + 1] - eu[e]) * dens : 0.f;
        lexcl[e] = lsum;
        lsum += dd[e];
    }
    float carry = group_excl_scan<G>(lsum, gl);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        float alpha = 1.f - unerf_exp(-dd[e]);
        float T = unerf_exp(-(carry + lexcl[e]));
        w[e] = (k0 + e < n) ? unerf_nan_to_num(alpha * T) : 0.f;
        if (a.weights_out && ray_ok && k0 + e < n) a.weights_out[r * n + k0 + e] = w[e];
    }
    // median depth of this level (prop_depth_i): the lane that owns the median sample writes its mid-point
    if (a.prop_depth) {
        float ls = 0.f, lc[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            ls += w[e];
            lc[e] = ls;
        }
        float cbase = group_excl_scan<G>(ls, gl);
        int cnt = 0;
#pragma unroll
        for (int e = 0; e < EPL; ++e) cnt += (k0 + e < n && (cbase + lc[e]) < 0.5f) ? 1 : 0;
        cnt = group_sum_i<G>(cnt);
        const int idx = min(cnt, n - 1);
        const int owner = idx / EPL, slot = idx - owner * EPL;
        float e0 = eu[0], e1 = eu[1];
#pragma unroll
        for (int e = 1; e < EPL; ++e) {
            e0 = (e == slot) ? eu[e] : e0;
            e1 = (e == slot) ? eu[e + 1] : e1;
        }
        if (gl == owner && ray_ok) a.prop_depth[r] = (e0 + e1) / 2.f;
    }
    // histogram -> pdf -> cdf
    float wp[EPL], lw = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        wp[e] = (k0 + e < n) ? w[e] + a.pad : 0.f;
        lw += wp[e];
    }
    float wsum = group_sum<G>(lw);
    float padding = fmaxf(a.eps - wsum, 0.f);
    float padn = padding / (float)n;
    wsum += padding;
    float lp = 0.f, lcdf[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        float pdf = (k0 + e < n) ? (wp[e] + padn) / wsum : 0.f;
        lp += pdf;
        lcdf[e] = lp;
    }
    float cb = group_excl_scan<G>(lp, gl);
    if (gl == 0) s_cdf[0] = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e)
        if (k0 + e < n) s_cdf[k0 + e + 1] = fminf(1.f, cb + lcdf[e]);
    wave_lds_sync();

    float vfirst = 0.f, vlast = 0.f;   // this lane's first and last output: outputs 0, 1 and nb - 2, nb - 1 are among them
    for (int j = gl; j < nb; j += G) {
        float u = a.u[j];
        // searchsorted(cdf[0..n], u, side="right") by the power-of-two descent of pdf_kernel
        int pos = 0;
        for (int step = top_step; step > 0; step >>= 1) {   // uniform trip count
            const int probe = min(pos + step, n);
            pos = (s_cdf[probe] <= u) ? probe : pos;
        }
        const int lo = pos + 1;
        int below = min(max(lo - 1, 0), n), above = min(max(lo, 0), n);
        float g0 = s_cdf[below], g1 = s_cdf[above];
        float b0 = s_sb[below], b1 = s_sb[above];
        float t = (u - g0) / (g1 - g0);
        t = unerf_nan_to_num(t);
        t = fminf(fmaxf(t, 0.f), 1.f);
        float v = b0 + t * (b1 - b0);
        vfirst = (j == gl) ? v : vfirst;
        vlast = v;
        if (ray_ok) a.sbins_out[r * nb + j] = v;
    }
    if (a.clip) {
        // lanes 0..3 of a group convert the four edges (first two, last two) at once; outputs 0 and 1 are the first of
        // lanes 0 and 1, outputs nb - 2 and nb - 1 the last of the lanes they fell to
        const int src = (lane - gl) + ((gl & 2) ? ((nb - 2 + (gl & 1)) & (G - 1)) : (gl & 1));
        const float xf = __shfl(vfirst, src, 64), xl = __shfl(vlast, src, 64);
        const float ev = unerf_s2e((gl & 2) ? xl : xf, a.s_near, a.s_far, a.lin);
        const float mid = (ev + dpp_f<0xB1>(ev)) / 2.f;   // lane 0: (f0 + f1) / 2, lane 2: (l0 + l1) / 2
        const float last = dpp_f<0xAA>(mid);              // quad_perm [2,2,2,2]
        if (ray_ok && gl == 0) {
            const int64_t chunk = clip_chunk(a, r, vw...);
            if (chunk != cur_chunk) {
                if (cur_chunk >= 0) pdf_clip_commit(a.clip, cur_chunk, cmin, cmax);
                cur_chunk = chunk;
                cmin = 0x7F800000u;
                cmax = 0u;
            }
            // positive floats order like their bit patterns
            cmin = min(cmin, __float_as_uint(mid));
            cmax = max(cmax, __float_as_uint(last));
        }
    }
    }  // rays of this block
    if (a.clip) {
        // the groups of a block normally sit in one chunk: merge them through LDS and send one update
        const int64_t blk_chunk = clip_chunk(a, (int64_t)blockIdx.x * PDF_RAYS_PER_BLOCK, vw...);
        const bool mergeable = cur_chunk == blk_chunk;  // this group never left the block's first chunk
        if (gl == 0) {
            s_clip[grp][0] = mergeable ? cmin : 0x7F800000u;
            s_clip[grp][1] = mergeable ? cmax : 0u;
            if (!mergeable && cur_chunk >= 0) pdf_clip_commit(a.clip, cur_chunk, cmin, cmax);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned int lo = 0x7F800000u, hi = 0u;
            for (int g = 0; g < NG; ++g) {
                lo = min(lo, s_clip[g][0]);
                hi = max(hi, s_clip[g][1]);
            }
            if (lo != 0x7F800000u || hi != 0u) pdf_clip_commit(a.clip, blk_chunk, lo, hi);
        }
    }
}

// Lanes per ray, from n alone: 16 = pdf_group_kernel (EPL = ceil(n / 16) <= 8), 64 = pdf_kernel (a wave per ray,
// EPL = ceil(n / 64) <= 4).  Above n = 128 a group's lane would sum nine and more samples in sequence; a 32-lane group
// (EPL <= 8 up to n = 256) was built and measured, and put one weight of tests/pdf_group_cases.py's plain-256-96 at 1.03 of
// its float64 bound (docs/experiments.md 8.4), so those n stay on the wave.
static inline int pdf_lanes_per_ray(int n) { return n <= 128 ? PDF_GROUP : 64; }

// views = NULL: unerf_weights_pdf_resample
static int pdf_resample_impl(const float* density, const float* sbins, int64_t sbins_stride, int64_t R,
                             int n, float near_plane, float far_plane, int spacing, const float* u, int m,
                             float histogram_padding, float eps, float* sbins_out, float* prop_depth_out,
                             float* weights_out, float* clip_minmax, int64_t ray_offset,
                             int64_t chunk_rays, const unerf_ray_views* views, void* stream) {
    UNERF_REQUIRE(R <= 0 || (density && sbins && u && sbins_out), "weights_pdf_resample: null pointer");
    UNERF_REQUIRE(n >= 1 && n <= PDF_MAXN, "weights_pdf_resample: n=%d outside [1,%d]", n, PDF_MAXN);
    UNERF_REQUIRE(m >= 1 && m + 1 <= PDF_MAXN, "weights_pdf_resample: m=%d outside [1,%d]", m, PDF_MAXN - 1);
    UNERF_REQUIRE(sbins_stride == 0 || sbins_stride >= n + 1, "weights_pdf_resample: sbins_stride < n+1");
    UNERF_REQUIRE(!clip_minmax || chunk_rays > 0, "weights_pdf_resample: chunk_rays must be > 0 with clip_minmax");
    UNERF_REQUIRE(near_plane > 0.f, "weights_pdf_resample: near plane must be > 0");
    if (R <= 0) return UNERF_OK;
    PdfArgs a;
    a.density = density; a.sbins = sbins; a.sstride = sbins_stride; a.R = R; a.n = n;
    if (int rc = set_spacing(a, near_plane, far_plane, spacing)) return rc;
    a.u = u; a.m = m; a.pad = histogram_padding; a.eps = eps; a.sbins_out = sbins_out; a.prop_depth = prop_depth_out;
    a.weights_out = weights_out; a.clip = clip_minmax; a.ray_offset = ray_offset; a.chunk_rays = chunk_rays;
    dim3 grid(blocks_for(R, PDF_RAYS_PER_BLOCK)), block(256);
    hipStream_t st = (hipStream_t)stream;
    // G lanes per ray and EPL = ceil(n / G) samples per lane: pdf_group_kernel<EPL, VW...> at G = 16 (EPL 1 .. 8),
    // pdf_kernel<EPL, VW...> at G = 64 (EPL 3, 4 reached: n > 128); the clip rows are numbered per view only where there is a
    // clip buffer (without one nothing in the kernel is numbered by the frame)
    const bool per_view = views && clip_minmax;
    const int lanes = pdf_lanes_per_ray(n);
    with_pack(per_view, [&] { return make_view_map(views, chunk_rays); }, [&](auto... vm) {
        if (lanes == PDF_GROUP)
            with_int<1, 2, 3, 4, 5, 6, 7, 8>((n + PDF_GROUP - 1) / PDF_GROUP, [&](auto epl) {
                hipLaunchKernelGGL((pdf_group_kernel<decltype(epl)::value, decltype(vm)...>), grid, block,
                                   pdf_group_lds_bytes(n, sbins_stride == 0), st, a, vm...);
            });
        else
            with_int<1, 2, 3, 4>((n + 63) / 64, [&](auto epl) {
                hipLaunchKernelGGL((pdf_kernel<decltype(epl)::value, decltype(vm)...>), grid, block, 0, st, a, vm...);
            });
    });
    return unerf_check_launch(per_view ? "weights_pdf_resample_views" : "weights_pdf_resample");
}

extern "C" int unerf_weights_pdf_resample(const float* density, const float* sbins, int64_t sbins_stride, int64_t R,
                                          int n, float near_plane, float far_plane, int spacing, const float* u, int m,
                                          float histogram_padding, float eps, float* sbins_out, float* prop_depth_out,
                                          float* weights_out, float* clip_minmax, int64_t ray_offset,
                                          int64_t chunk_rays, void* stream) {
    return pdf_resample_impl(density, sbins, sbins_stride, R, n, near_plane, far_plane, spacing, u, m, histogram_padding, eps,
                             sbins_out, prop_depth_out, weights_out, clip_minmax, ray_offset, chunk_rays, nullptr, stream);
}

extern "C" int unerf_weights_pdf_resample_views(const float* density, const float* sbins, int64_t sbins_stride, int64_t R,
                                                int n, float near_plane, float far_plane, int spacing, const float* u, int m,
                                                float histogram_padding, float eps, float* sbins_out, float* prop_depth_out,
                                                float* weights_out, float* clip_minmax, const unerf_ray_views* views,
                                                int64_t chunk_rays, void* stream) {
    if (int rc = check_views(views, R, "weights_pdf_resample_views")) return rc;
    return pdf_resample_impl(density, sbins, sbins_stride, R, n, near_plane, far_plane, spacing, u, m, histogram_padding, eps,
                             sbins_out, prop_depth_out, weights_out, clip_minmax, 0, chunk_rays, views, stream);
}

// ======================================================================================
// 5. main field.  One wave per block; lane = one sample; activations live in LDS as
//    [feature][lane] (bank-conflict free), weights stream through the scalar cache
//    (uniform addresses -> s_load), accumulators are static registers.
// ======================================================================================
// Which 32 rays form the columns of a matrix-kernel tile.  Default: 32 consecutive rays.  When the caller says
// that its rays are consecutive pixels of a row-major image (unerf_field_params.image_width), a tile is an
// 8 x 4 PIXEL PATCH instead: neighbouring samples then sit in fewer distinct grid cells on the fine levels, so a
// gather instruction touches fewer cache lines (the texture-address unit is what binds the split-f16 ACTIVE
// kernel).  Pure scheduling: every (ray, sample) is computed exactly as before.
struct TileMap {
    uint32_t img_w;      // 0: consecutive rays
    uint32_t pcols;      // 8-pixel patch columns per 4-row band
    FastDiv div_pcols;
    int64_t g0;          // index of local ray 0 in the image
    int64_t first_row;   // first image row of the first band touched by this launch
};

struct FieldArgs {
    const float* origins;
    const float* dirs;
    const float* sbins;
    int64_t R;
    int S;
    float s_near, s_far;
    int lin;   // UNERF_SPACING_*: 1 = identity spacing (UniformSampler)
    int64_t ray_offset;
    unerf_field_params p;
    float* density;
    float* rgb;
    float* aux;
    float* aux2;
    int32_t keep_hi;     // MC-dropout keep threshold thr_s << 16 (unerf_keep_lo / unerf_keep_hi); bit 0: keep every unit (field_keep_all)
    uint32_t keep_pk;    // thr_s in both 16-bit halves (packed-f16 masks of the split-f16 kernels)
    int drop_on;         // the mask path runs: K > 0 and the threshold drops units, or explicit masks, or (fp32 kernels) a scale without drops
    int drop_sites;      // UNERF_DROP_* bits actually in use (0 when !drop_on)
    float drop_scale;
    const float* features;  // optional [16][N][2] level-major planes from unerf_field_gather (MFMA kernel)
    TileMap tm;
    unerf_norm_box box;
    FastDiv div_chunk;      // LAPLACE per-chunk sample sets: division by p.lap_chunk_rays
    uint32_t chunk0;        // ... and ray_offset as a 32-bit ray index (the sample counter bound keeps it below 2^31)
};

// EXPLICIT keep masks (unerf_field_fwd_masked): a kernel argument of the XM instantiations only -- the default kernels keep
// their argument list.  Bit arrays as include/unerf.h: unerf_keep_masks lays them out ([K][pass_stride][W] uint32, bit u of
// a row set = unit u kept); all three sites here are 64 units wide, W = 2.
struct KeepArgs {
    const uint32_t* site[3];   // UNERF_DROP_TRUNK, _HEAD0, _HEAD1 (NULL: site not active)
    int64_t pass_stride;       // rows between two passes
    int64_t sample_offset;     // row of (ray 0, sample 0) of this launch
};
#define XM_WORDS 2   // uint32 words per row of a 64-unit site
// The mask WORD of a unit pair from its two keep bits: kept -> the half 0x8000 (the most negative signed 16-bit number),
// dropped -> 0x7FFF (the largest).  Such a word passes / fails unerf_keep_lo / unerf_keep_hi / mf16_keep_diff exactly as
// the bits say at every threshold thr_s in (-32768, 32767] (the host sets thr_s = 0 in this mode), so everything behind
// the making of the words -- selects, AND masks, the sign trick of mf16_split_relu_drop -- is the generator path's code.
__device__ __forceinline__ uint32_t xm_word(uint32_t bits, int pos) {
    return 0x7FFF7FFFu + ((bits >> pos) & 1u) + (((bits >> (pos + 1)) & 1u) << 16);
}
// The XM kernels are the SAME __global__ templates as the default ones with one trailing argument (a parameter pack that is
// empty in the default instantiations, which therefore keep their argument list and their code): xm_of() names it.
__device__ __forceinline__ const KeepArgs& xm_of(const KeepArgs& x) { return x; }
// first word of the row of sample n (r * S + s of this launch) at pass k
__device__ __forceinline__ const uint32_t* xm_row(const KeepArgs& x, int site, int k, int64_t n) {
    return x.site[site] + ((int64_t)k * x.pass_stride + x.sample_offset + n) * XM_WORDS;
}

// SEVERAL VIEWS in one launch (unerf_field_fwd_views): a kernel argument of the views instantiations of field_kernel_mfma16
// only, like KeepArgs.  The mask counter of a sample is numbered inside its own frame and keyed by its view's seed; a tile
// may straddle two views, so both are per-lane values (the keys are staged in LDS and read by view index).
struct FieldViews {
    FastDiv div_hw;   // by rays per view
    uint32_t hw;
    uint32_t key[UNERF_NERF_MAX_VIEWS];   // unerf_mc_key(seed[v], 0)
};
__device__ __forceinline__ const FieldViews& vw_of(const FieldViews& x) { return x; }
// which trailing argument an instantiation carries (none: the default kernels)
template <typename... XA> struct xa_is_keep : std::false_type {};
template <> struct xa_is_keep<KeepArgs> : std::true_type {};
template <typename... XA> struct xa_is_views : std::false_type {};
template <> struct xa_is_views<FieldViews> : std::true_type {};

// Bin edge -> Euclidean distance.  unerf_field_fwd(near_plane < 0) sets s_near = -1: sbins then already holds
// Euclidean edges (RaySamples.frustums.starts / ends of a caller-made sampler) and passes through untouched.
__device__ __forceinline__ float field_bin_edge(const FieldArgs& a, float b) {
    return a.s_near < 0.f ? b : unerf_s2e(b, a.s_near, a.s_far, a.lin);
}

// ray of column j of ray-block rb (a tile is (rb, sample index)); invalid columns are clamped by the caller
__device__ __forceinline__ void tile_ray(const FieldArgs& a, uint32_t rb, int j, int64_t& r, bool& valid) {
    if (a.tm.img_w == 0) {  // uniform
        r = (int64_t)rb * 32 + j;
        valid = r < a.R;
    } else {
        const uint32_t band = fastdiv(rb, a.tm.div_pcols), pc = rb - band * a.tm.pcols;
        const uint32_t x = pc * 8u + (uint32_t)(j & 7);
        const int64_t y = a.tm.first_row + (int64_t)band * 4 + (j >> 3);
        r = y * (int64_t)a.tm.img_w + x - a.tm.g0;
        valid = x < a.tm.img_w && r >= 0 && r < a.R;
    }
}

// One column of a matrix-kernel tile: which (ray, sample) it is and where the sample sits (mid-point of its
// spacing bin, euclidean, before contraction).  Shared by the four field_kernel_mfma* kernels.
struct TileSample {
    int64_t n;        // r * S + s
    int64_t r;        // ray (clamped to a valid one when !valid)
    int s;            // sample slot
    bool valid;       // column maps to a ray of this launch (else clamped to the last ray, results dropped)
    float dx, dy, dz;
    float px, py, pz;
};
// (r: already clamped to a ray of the launch when !valid)
__device__ __forceinline__ TileSample tile_sample_at(const FieldArgs& a, int64_t r, int s, bool valid) {
    TileSample t;
    t.valid = valid;
    t.n = r * a.S + s;
    t.r = r;
    t.s = s;
    const float* sb = a.sbins + r * (a.S + 1);
    const float e0 = field_bin_edge(a, sb[s]), e1 = field_bin_edge(a, sb[s + 1]);
    const float t01 = e0 + e1;
    t.dx = a.dirs[r * 3 + 0];
    t.dy = a.dirs[r * 3 + 1];
    t.dz = a.dirs[r * 3 + 2];
    t.px = a.origins[r * 3 + 0] + t.dx * t01 / 2.f;
    t.py = a.origins[r * 3 + 1] + t.dy * t01 / 2.f;
    t.pz = a.origins[r * 3 + 2] + t.dz * t01 / 2.f;
    return t;
}
__device__ __forceinline__ TileSample tile_sample(const FieldArgs& a, uint32_t tile, const FastDiv& div_s, int j) {
    const uint32_t rb = fastdiv(tile, div_s);
    const int s = (int)(tile - rb * (uint32_t)a.S);
    int64_t r;
    bool valid;
    tile_ray(a, rb, j, r, valid);
    if (!valid) r = a.R - 1;
    return tile_sample_at(a, r, s, valid);
}

// Where one (pass k, ray r, sample s) lands in the outputs.  Default (sample_major = 0): density [B,R,S], rgb [B,R,S,3],
// aux [R,S] -- the RaySamples layout the Field-level API returns.  sample_major = 1: planes density [B,S,R],
// rgb [B,S,3,R], aux [S,R].  A tile's 32 columns are 32 rays at ONE sample slot, so in the ray-major layout each of
// its stores is a lone 4-byte write into its own cache line (2.9 x the algorithmic bytes reached the fabric,
// profiles/r1_11_active_pmc_summary.json); in the plane layout the same store covers whole 32-byte sectors (8
// consecutive rays of a pixel patch, 32 of a 1-D tile), and the composite kernel reads the planes with a lane per ray.
struct OutIndex {
    int64_t dens, rgb, rgb_stride, aux;
};
__device__ __forceinline__ OutIndex out_index(const FieldArgs& a, int k, const TileSample& ts) {
    OutIndex o;
    if (a.p.sample_major) {  // uniform
        const int64_t plane = (int64_t)k * a.S + ts.s;
        o.dens = plane * a.R + ts.r;
        o.rgb = plane * 3 * a.R + ts.r;
        o.rgb_stride = a.R;
        o.aux = (int64_t)ts.s * a.R + ts.r;
    } else {
        o.dens = (int64_t)k * (a.R * (int64_t)a.S) + ts.n;
        o.rgb = o.dens * 3;
        o.rgb_stride = 1;
        o.aux = ts.n;
    }
    return o;
}
// packed_out: ONE 16-byte row (sigma, r, g, b) per (pass, ray, sample) in `rgb` [B,R,S,4] instead of a dword into
// `density` and three into `rgb`.  A tile's columns are 32 rays at one sample slot, so every store of the ray-major
// layouts is a lone write into its own cache line: four 4-byte stores per sample reached the fabric as 1.84 x (K-pass)
// to 3.4 x (ACTIVE) the algorithmic bytes at 2^20-ray launch groups (profiles/traffic_*.json, round 3).
__device__ __forceinline__ void store_packed(const FieldArgs& a, int k, int64_t n, float sigma, float r, float g, float b) {
    reinterpret_cast<float4*>(a.rgb)[(int64_t)k * (a.R * (int64_t)a.S) + n] = make_float4(sigma, r, g, b);
}

// LAPLACE with per-chunk sample sets (unerf_field_params.lap_chunk_rays): the blob of the set a tile's rays belong to.
// Tiles are 1-D there (32 consecutive rays, host: make_tiles without an image width) and chunk / launch boundaries are
// multiples of 32, so the set is uniform over the tile; `tile` is wave-uniform, so this is scalar arithmetic.
__device__ __forceinline__ const float* lap_set_blob(const FieldArgs& a, const float* blob, uint32_t tile, const FastDiv& div_s) {
    if (a.p.lap_chunk_rays == 0) return blob;
    const uint32_t set = fastdiv(a.chunk0 + fastdiv(tile, div_s) * 32u, a.div_chunk);
    return blob + (size_t)set * UNERF_LAP_BLOB_FLOATS;
}

// SEVERAL VIEWS in one LAPLACE launch (unerf_field_fwd_laplace_views): a kernel argument of views_laplace_kernel_mfma16 only.
// The ray blocks are laid out PER VIEW -- bpv = ceil(hw / 32) blocks each, block rb = view rb / bpv at frame-local rays
// (rb % bpv) * 32 + [0, 32) -- so a tile never straddles two views, and inside its view it starts at a multiple of 32 as
// the single-view tiles do: its sample set, set_base[view] + local / lap_chunk_rays, is uniform over the tile.  The columns
// of a view's last block past hw are invalid (clamped, results dropped).
struct LapViews {
    FastDiv div_bpv;   // by ray blocks per view
    uint32_t bpv;
    uint32_t hw;       // rays per view
    int32_t set_base[UNERF_NERF_MAX_VIEWS];   // first sample set of view v in the stacks (staged in LDS, read by view index)
};
__device__ __forceinline__ const LapViews& lv_of(const LapViews& x) { return x; }
template <typename... XV> struct xv_is_lap_views : std::false_type {};
template <> struct xv_is_lap_views<LapViews> : std::true_type {};
__device__ __forceinline__ TileSample tile_sample_views(const FieldArgs& a, uint32_t tile, const FastDiv& div_s, int j, const LapViews& lv) {
    const uint32_t rb = fastdiv(tile, div_s);
    const int s = (int)(tile - rb * (uint32_t)a.S);
    const uint32_t view = fastdiv(rb, lv.div_bpv);
    uint32_t local = (rb - view * lv.bpv) * 32u + (uint32_t)j;
    const bool valid = local < lv.hw;
    if (!valid) local = lv.hw - 1u;
    return tile_sample_at(a, (int64_t)view * lv.hw + local, s, valid);
}
// the blob of a tile's set; vsets = the LDS copy of lv.set_base.  `tile` is wave-uniform and so is everything here: the value
// read from LDS is made a scalar again, so that the head operands keep their scalar base address
__device__ __forceinline__ const float* lap_set_blob_views(const FieldArgs& a, const float* blob, uint32_t tile, const FastDiv& div_s,
                                                           const LapViews& lv, const int32_t* vsets) {
    const uint32_t rb = fastdiv(tile, div_s);
    const uint32_t view = fastdiv(rb, lv.div_bpv);
    uint32_t set = (uint32_t)__builtin_amdgcn_readfirstlane(vsets[view]);
    if (a.p.lap_chunk_rays != 0) set += fastdiv((rb - view * lv.bpv) * 32u, a.div_chunk);
    return blob + (size_t)set * UNERF_LAP_BLOB_FLOATS;
}

// host side: fills a.tm and returns the number of tiles
static int64_t make_tiles(FieldArgs& a, int image_width) {
    a.tm.img_w = 0; a.tm.pcols = 0; a.tm.div_pcols = make_fastdiv(1); a.tm.g0 = 0; a.tm.first_row = 0;
    if (image_width >= 8 && a.R >= 4 * (int64_t)image_width) {   // at least one full band, else 1-D tiles
        const int64_t g0 = a.ray_offset, g1 = a.ray_offset + a.R - 1;
        const int64_t band0 = (g0 / image_width) / 4, band1 = (g1 / image_width) / 4;
        const int64_t pcols = (image_width + 7) / 8;
        const int64_t tiles = (band1 - band0 + 1) * pcols * (int64_t)a.S;
        if (tiles < (1ll << 28)) {
            a.tm.img_w = (uint32_t)image_width; a.tm.pcols = (uint32_t)pcols; a.tm.div_pcols = make_fastdiv((uint32_t)pcols);
            a.tm.g0 = g0; a.tm.first_row = band0 * 4;
            return tiles;
        }
    }
    return ((a.R + 31) / 32) * (int64_t)a.S;
}

// acc[o] = b[o] + sum_i act[i] * Wt[i][o]   (sequential over i, fused multiply-add)
template <int IN, int OUT>
__device__ __forceinline__ void dense_lds(const float* __restrict__ Wt, const float* __restrict__ b,
                                          const float* act, int lane, float (&acc)[OUT]) {
#pragma unroll
    for (int o = 0; o < OUT; ++o) acc[o] = b[o];
#pragma unroll 2
    for (int i = 0; i < IN; ++i) {
        float x = act[i * 64 + lane];
#pragma unroll
        for (int o = 0; o < OUT; ++o) acc[o] = fmaf(x, Wt[i * OUT + o], acc[o]);
    }
}

// FieldArgs.keep_hi = thr_s << 16 has a zero low half; bit 0 set says KEEP EVERY UNIT.  The host sets it where p_drop > 0 is
// so small that round((1 - p) 65536) = 65536: no signed 16-bit threshold keeps every half, and the scale 1 / (1 - p) still
// applies (field_fill_args).  Read by the generator paths of the fp32 kernels; the f16 kernels carry the scale in their operand
// blob and run without masks there.
__device__ __forceinline__ bool field_keep_all(int32_t thr_hi) { return (thr_hi & 1) != 0; }

// same, with an inverted-dropout mask on the IN inputs (mask words: unerf_mask_word0 / unerf_mask_step; unit 2j is the
// low half of word j, unit 2j + 1 the high half)
template <int OUT, int IN = 64>
__device__ __forceinline__ void dense_lds_dropout(const float* __restrict__ Wt, const float* __restrict__ b,
                                                  const float* act, int lane, uint32_t pre, int pass,
                                                  uint32_t stream_id, int32_t thr_hi, float scale, float (&acc)[OUT]) {
#pragma unroll
    for (int o = 0; o < OUT; ++o) acc[o] = b[o];
    const uint32_t bh[2] = {unerf_mc_base_h(pre, 0u), unerf_mc_base_h(pre, 1u)};
    const bool all = field_keep_all(thr_hi);
    for (int j = 0; j < (IN + 1) / 2; ++j) {
        uint32_t rnd = unerf_mask_word0(bh[(j >> 1) & 1], stream_id, (uint32_t)j);
        for (int q = 0; q < pass; ++q) rnd = unerf_mask_step(rnd);
        float x0 = act[(2 * j) * 64 + lane];
        x0 = (all || unerf_keep_lo(rnd, thr_hi)) ? x0 * scale : 0.f;
#pragma unroll
        for (int o = 0; o < OUT; ++o) acc[o] = fmaf(x0, Wt[(2 * j) * OUT + o], acc[o]);
        if (2 * j + 1 < IN) {
            float x1 = act[(2 * j + 1) * 64 + lane];
            x1 = (all || unerf_keep_hi(rnd, thr_hi)) ? x1 * scale : 0.f;
#pragma unroll
            for (int o = 0; o < OUT; ++o) acc[o] = fmaf(x1, Wt[(2 * j + 1) * OUT + o], acc[o]);
        }
    }
}
// the same layer (64 inputs) under EXPLICIT keep bits: `row` = this sample's two words of the site at this pass; the word of
// unit pair j is made of its two bits (xm_word) and takes the same tests, selects and multiply-adds in the same order
template <int OUT>
__device__ __forceinline__ void dense_lds_keepbits(const float* __restrict__ Wt, const float* __restrict__ b,
                                                   const float* act, int lane, const uint32_t* row, int32_t thr_hi,
                                                   float scale, float (&acc)[OUT]) {
#pragma unroll
    for (int o = 0; o < OUT; ++o) acc[o] = b[o];
    const uint32_t bits[XM_WORDS] = {row[0], row[1]};
    for (int j = 0; j < 32; ++j) {
        const uint32_t rnd = xm_word(j < 16 ? bits[0] : bits[1], (2 * j) & 31);
        float x0 = act[(2 * j) * 64 + lane];
        x0 = unerf_keep_lo(rnd, thr_hi) ? x0 * scale : 0.f;
#pragma unroll
        for (int o = 0; o < OUT; ++o) acc[o] = fmaf(x0, Wt[(2 * j) * OUT + o], acc[o]);
        float x1 = act[(2 * j + 1) * 64 + lane];
        x1 = unerf_keep_hi(rnd, thr_hi) ? x1 * scale : 0.f;
#pragma unroll
        for (int o = 0; o < OUT; ++o) acc[o] = fmaf(x1, Wt[(2 * j + 1) * OUT + o], acc[o]);
    }
}

template <int N>
__device__ __forceinline__ void store_act(float* act, int lane, const float (&v)[N], int row0, bool relu) {
#pragma unroll
    for (int o = 0; o < N; ++o) act[(row0 + o) * 64 + lane] = relu ? fmaxf(v[o], 0.f) : v[o];
}

// XA = KeepArgs: explicit keep masks (MCDROPOUT)
template <int MODE, typename... XA>
__global__ __launch_bounds__(64) void field_kernel(FieldArgs a, XA... xa) {
    constexpr bool XM = sizeof...(XA) != 0;
    extern __shared__ float lds[];
    float* A = lds;                 // [64][64]
    float* Bf = lds + 64 * 64;      // [64][64] (MCDROPOUT only)
    const int lane = threadIdx.x;
    const int64_t N = a.R * (int64_t)a.S;
    int64_t n = (int64_t)blockIdx.x * 64 + lane;
    const bool valid = n < N;
    if (!valid) n = N - 1;
    const int64_t r = n / a.S;
    const int s = (int)(n - r * a.S);

    const float* sb = a.sbins + r * (a.S + 1);
    float e0 = field_bin_edge(a, sb[s]), e1 = field_bin_edge(a, sb[s + 1]);
    float t = e0 + e1;
    float dxr = a.dirs[r * 3 + 0], dyr = a.dirs[r * 3 + 1], dzr = a.dirs[r * 3 + 2];
    float px = a.origins[r * 3 + 0] + dxr * t / 2.f;
    float py = a.origins[r * 3 + 1] + dyr * t / 2.f;
    float pz = a.origins[r * 3 + 2] + dzr * t / 2.f;
    const float sel = unerf_normalize_position(px, py, pz, a.box);

    const uint32_t mask = (1u << a.p.log2T) - 1u;
#pragma unroll 4
    for (int l = 0; l < 16; ++l) {
        float2 f;
        if (a.p.tcnn_levels && a.p.grid_half) {   // uniform
            f = unerf_tcnn_level_feat_half(a.p.table, a.p.tcnn_levels[l], px, py, pz);
        } else if (a.p.tcnn_levels) {
            f = unerf_tcnn_level_feat(reinterpret_cast<const float2*>(a.p.table), a.p.tcnn_levels[l], px, py, pz);
        } else {
            const float2* lvl = reinterpret_cast<const float2*>(a.p.table) + ((size_t)l << a.p.log2T);
            f = unerf_hash_level(lvl, px, py, pz, a.p.scalings[l], mask);
        }
        A[(2 * l) * 64 + lane] = f.x;
        A[(2 * l + 1) * 64 + lane] = f.y;
    }

    // direction encoding inputs: get_normalized_directions(d) = (d+1)/2 (torch SHEncoding uses it as is)
    float sh[16];
    {
        float ux = (dxr + 1.f) / 2.f, uy = (dyr + 1.f) / 2.f, uz = (dzr + 1.f) / 2.f;
        if (a.p.sh_remap) {
            ux = ux * 2.f - 1.f;
            uy = uy * 2.f - 1.f;
            uz = uz * 2.f - 1.f;
        }
        unerf_sh16(ux, uy, uz, sh);
    }

    float acc[64];
    dense_lds<32, 64>(a.p.w0t, a.p.b0, A, lane, acc);

    if constexpr (MODE == UNERF_FIELD_ACTIVE) {
        store_act<64>(A, lane, acc, 0, true);
        float o1[17];
        dense_lds<64, 17>(a.p.w1t, a.p.b1, A, lane, o1);
        float density = a.p.average_init_density * expf(o1[0]) * sel;
        float beta = unerf_softplus(o1[16]) + a.p.beta_min;
        store_act<16>(A, lane, sh, 0, false);
#pragma unroll
        for (int g = 0; g < 15; ++g) A[(16 + g) * 64 + lane] = o1[1 + g];
        dense_lds<31, 64>(a.p.h0t, a.p.hb0, A, lane, acc);
        store_act<64>(A, lane, acc, 0, true);
        dense_lds<64, 64>(a.p.h1t, a.p.hb1, A, lane, acc);
        store_act<64>(A, lane, acc, 0, true);
        float c[3];
        dense_lds<64, 3>(a.p.h2t, a.p.hb2, A, lane, c);
        if (valid) {
            a.aux[n] = beta;
            if (a.p.packed_out) {
                store_packed(a, 0, n, density, unerf_sigmoid(c[0]), unerf_sigmoid(c[1]), unerf_sigmoid(c[2]));
            } else {
                a.density[n] = density;
                a.rgb[n * 3 + 0] = unerf_sigmoid(c[0]);
                a.rgb[n * 3 + 1] = unerf_sigmoid(c[1]);
                a.rgb[n * 3 + 2] = unerf_sigmoid(c[2]);
            }
        }
    } else if constexpr (MODE == UNERF_FIELD_MCDROPOUT) {
        store_act<64>(A, lane, acc, 0, true);  // hidden h stays in A for every pass
        const int passes = a.p.K > 0 ? a.p.K : 1;
        const uint32_t sidx = (uint32_t)((uint64_t)a.ray_offset * (uint64_t)a.S + (uint64_t)n);
        for (int k = 0; k < passes; ++k) {
            const uint32_t base = unerf_mc_pre(unerf_mc_key(a.p.seed, 0u), sidx);   // dense_lds_dropout derives both half bases
            float o1[16];
            if constexpr (XM) {
                if (a.drop_sites & UNERF_DROP_TRUNK) dense_lds_keepbits<16>(a.p.w1t, a.p.b1, A, lane, xm_row(xm_of(xa...), 0, k, n), a.keep_hi, a.drop_scale, o1);
                else dense_lds<64, 16>(a.p.w1t, a.p.b1, A, lane, o1);
            } else
            if (a.drop_sites & UNERF_DROP_TRUNK) dense_lds_dropout<16>(a.p.w1t, a.p.b1, A, lane, base, k, 0u, a.keep_hi, a.drop_scale, o1);
            else dense_lds<64, 16>(a.p.w1t, a.p.b1, A, lane, o1);
            float density = a.p.average_init_density * expf(o1[0]) * sel;
            store_act<16>(Bf, lane, sh, 0, false);
#pragma unroll
            for (int g = 0; g < 15; ++g) Bf[(16 + g) * 64 + lane] = o1[1 + g];
            if (a.drop_sites & UNERF_DROP_HEADIN) {   // rgb_dropout_layers contains 0: Dropout on the head's 63 inputs
                for (int e = 0; e < 32; ++e) Bf[(31 + e) * 64 + lane] = a.p.app_embed[e];
                dense_lds_dropout<64, 63>(a.p.h0_full_t, a.p.hb0_raw, Bf, lane, base, k, 3u, a.keep_hi, a.drop_scale, acc);
            } else {
                dense_lds<31, 64>(a.p.h0t, a.p.hb0, Bf, lane, acc);
            }
            store_act<64>(Bf, lane, acc, 0, true);
            if (a.drop_sites & UNERF_DROP_HEAD0) {
                float acc2[64];
                if constexpr (XM) dense_lds_keepbits<64>(a.p.h1t, a.p.hb1, Bf, lane, xm_row(xm_of(xa...), 1, k, n), a.keep_hi, a.drop_scale, acc2);
                else dense_lds_dropout<64>(a.p.h1t, a.p.hb1, Bf, lane, base, k, 2u, a.keep_hi, a.drop_scale, acc2);
                store_act<64>(Bf, lane, acc2, 0, true);
            } else {
                dense_lds<64, 64>(a.p.h1t, a.p.hb1, Bf, lane, acc);
                store_act<64>(Bf, lane, acc, 0, true);
            }
            float c[3];
            if constexpr (XM) {
                if (a.drop_sites & UNERF_DROP_HEAD1) dense_lds_keepbits<3>(a.p.h2t, a.p.hb2, Bf, lane, xm_row(xm_of(xa...), 2, k, n), a.keep_hi, a.drop_scale, c);
                else dense_lds<64, 3>(a.p.h2t, a.p.hb2, Bf, lane, c);
            } else
            if (a.drop_sites & UNERF_DROP_HEAD1) dense_lds_dropout<3>(a.p.h2t, a.p.hb2, Bf, lane, base, k, 1u, a.keep_hi, a.drop_scale, c);
            else dense_lds<64, 3>(a.p.h2t, a.p.hb2, Bf, lane, c);
            if (valid && a.p.packed_out) {
                store_packed(a, k, n, density, unerf_sigmoid(c[0]), unerf_sigmoid(c[1]), unerf_sigmoid(c[2]));
            } else if (valid) {
                int64_t q = (int64_t)k * N + n;
                a.density[q] = density;
                a.rgb[q * 3 + 0] = unerf_sigmoid(c[0]);
                a.rgb[q * 3 + 1] = unerf_sigmoid(c[1]);
                a.rgb[q * 3 + 2] = unerf_sigmoid(c[2]);
            }
        }
    } else {  // LAPLACE: bare Linear base (no ReLU), sampled last layers
        store_act<64>(A, lane, acc, 0, false);
        float geo[15];
        dense_lds<64, 15>(a.p.w1t, a.p.b1, A, lane, geo);
        const int nl = a.p.n_lap, nr = a.p.n_lap_rgb;
        // per-chunk sample sets (unerf_field_params.lap_chunk_rays): a wave of 64 consecutive samples may straddle two
        const size_t set = a.p.lap_chunk_rays ? (size_t)fastdiv(a.chunk0 + (uint32_t)r, a.div_chunk) : 0;
        float mu = 0.f, mu2 = 0.f;
        for (int q = 0; q < nl; ++q) {
            const float* __restrict__ w = a.p.ws_density + (set * nl + (size_t)q) * 65;
            float pre = 0.f;
#pragma unroll
            for (int i = 0; i < 64; ++i) pre = fmaf(acc[i], w[i], pre);
            pre += w[64];
            float pred = a.p.lap_softplus ? unerf_softplus(pre) : expf(pre);
            mu += pred;
            mu2 += pred * pred;
        }
        mu /= (float)nl;
        mu2 /= (float)nl;
        float var_d = a.p.lap_mask_density ? 0.f : mu2 - mu * mu;
        store_act<16>(A, lane, sh, 0, false);
        store_act<15>(A, lane, geo, 16, false);
        dense_lds<31, 64>(a.p.h0t, a.p.hb0, A, lane, acc);
        store_act<64>(A, lane, acc, 0, true);
        dense_lds<64, 64>(a.p.h1t, a.p.hb1, A, lane, acc);
#pragma unroll
        for (int i = 0; i < 64; ++i) acc[i] = fmaxf(acc[i], 0.f);
        float m1[3] = {0.f, 0.f, 0.f}, m2[3] = {0.f, 0.f, 0.f};
        for (int q = 0; q < nr; ++q) {
            const float* __restrict__ w = a.p.ws_rgb + (set * nr + (size_t)q) * 195;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float pre = 0.f;
#pragma unroll
                for (int i = 0; i < 64; ++i) pre = fmaf(acc[i], w[c * 64 + i], pre);
                pre += w[192 + c];
                float pred = unerf_sigmoid(pre);
                m1[c] += pred;
                m2[c] += pred * pred;
            }
        }
        float vsum = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            m1[c] /= (float)nr;
            m2[c] /= (float)nr;
            vsum += fmaxf(m2[c] - m1[c] * m1[c], 0.f);
        }
        if (valid) {
            a.density[n] = a.p.lap_mask_density ? mu * sel : mu;  // inference: NOT selector-masked (laplace_field.py:356-362)
            a.aux[n] = var_d;
            a.aux2[n] = vsum / 3.f;
            a.rgb[n * 3 + 0] = m1[0];
            a.rgb[n * 3 + 1] = m1[1];
            a.rgb[n * 3 + 2] = m1[2];
        }
    }
}

// --------------------------------------------------------------------------------------
// 5a'. ANY-WIDTH field (the slow path).  The reference forwards hidden_dim, hidden_dim_color, features_per_level and
// appearance_embed_dim from the model config to the field (activenerfacto_model.py:63-77, mcdropout_models.py:66-80,
// laplace_model.py:169-186) and the field class takes geo_feat_dim; the matrix kernels and field_kernel above are
// built for nerfacto's 64 / 64 / 2 / 15.  This kernel takes every width at run time (unerf_field_params.hidden, ...):
// one lane per sample, activations in LDS as [unit][lane], weights through the scalar cache, eight outputs per sweep
// of a layer's inputs.  Same arithmetic definitions (mask words, SH, activations) as field_kernel -- roughly 10-20 x the
// time of the matrix kernels: a configuration that is kept CORRECT, and says so once (ops.py warns).
// --------------------------------------------------------------------------------------
__device__ __forceinline__ void dense_any(const float* __restrict__ Wt, const float* __restrict__ b, const float* in,
                                          float* out, int IN, int OUT, int lane, bool relu) {
    for (int o0 = 0; o0 < OUT; o0 += 8) {
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = o0 + j < OUT ? b[o0 + j] : 0.f;
        for (int i = 0; i < IN; ++i) {
            const float x = in[i * 64 + lane];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (o0 + j < OUT) acc[j] = fmaf(x, Wt[i * OUT + o0 + j], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (o0 + j < OUT) out[(o0 + j) * 64 + lane] = relu ? fmaxf(acc[j], 0.f) : acc[j];
    }
}
// inverted dropout of `n` units: dst = keep ? src * scale : 0 (dst may be src)
__device__ __forceinline__ void mask_any(const float* src, float* dst, int n, int lane, uint32_t pre, int pass,
                                         uint32_t stream_id, int32_t thr_hi, float scale) {
    const uint32_t bh[2] = {unerf_mc_base_h(pre, 0u), unerf_mc_base_h(pre, 1u)};
    const bool all = field_keep_all(thr_hi);
    for (int j = 0; 2 * j < n; ++j) {
        uint32_t rnd = unerf_mask_word0(bh[(j >> 1) & 1], stream_id, (uint32_t)j);
        for (int q = 0; q < pass; ++q) rnd = unerf_mask_step(rnd);
        dst[(2 * j) * 64 + lane] = (all || unerf_keep_lo(rnd, thr_hi)) ? src[(2 * j) * 64 + lane] * scale : 0.f;
        if (2 * j + 1 < n) dst[(2 * j + 1) * 64 + lane] = (all || unerf_keep_hi(rnd, thr_hi)) ? src[(2 * j + 1) * 64 + lane] * scale : 0.f;
    }
}
// one level of the torch-layout grid with FOUR features per row (16-byte rows): the same corners and lerp order
__device__ __forceinline__ void unerf_hash_level4(const float4* __restrict__ lvl, float px, float py, float pz, float scale,
                                                  uint32_t mask, float (&f4)[4]) {
    uint32_t off[8];
    float ox, oy, oz;
    unerf_hash_corners<false, false>(px, py, pz, scale, mask, off, ox, oy, oz);
    float2 lo[8], hi[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float4 v = lvl[off[k] >> 3];
        lo[k] = make_float2(v.x, v.y);
        hi[k] = make_float2(v.z, v.w);
    }
    const float2 a = unerf_blend8(lo, ox, oy, oz), c = unerf_blend8(hi, ox, oy, oz);
    f4[0] = a.x; f4[1] = a.y; f4[2] = c.x; f4[3] = c.y;
}

template <int MODE>
__global__ __launch_bounds__(64) void field_kernel_generic(FieldArgs a, int rows) {
    extern __shared__ float lds[];
    float* A = lds;                       // hidden trunk units (pass-invariant)
    float* B = lds + (size_t)rows * 64;   // ping
    float* Cb = B + (size_t)rows * 64;    // head input [SH16 | geo | (appearance)]
    float* D = Cb + (size_t)rows * 64;    // pong / trunk output
    const int lane = threadIdx.x;
    const int H = a.p.hidden, HC = a.p.hidden_color, G = a.p.geo_dim, F = a.p.feat_per_level, L = a.p.L, AD = a.p.app_dim;
    const int IN0 = L * F, OUT1 = a.p.out1, INC = 16 + G;
    const int64_t N = a.R * (int64_t)a.S;
    int64_t n = (int64_t)blockIdx.x * 64 + lane;
    const bool valid = n < N;
    if (!valid) n = N - 1;
    const int64_t r = n / a.S;
    const int s = (int)(n - r * a.S);
    const float* sb = a.sbins + r * (a.S + 1);
    const float t = field_bin_edge(a, sb[s]) + field_bin_edge(a, sb[s + 1]);
    const float dxr = a.dirs[r * 3 + 0], dyr = a.dirs[r * 3 + 1], dzr = a.dirs[r * 3 + 2];
    float px = a.origins[r * 3 + 0] + dxr * t / 2.f;
    float py = a.origins[r * 3 + 1] + dyr * t / 2.f;
    float pz = a.origins[r * 3 + 2] + dzr * t / 2.f;
    const float sel = unerf_normalize_position(px, py, pz, a.box);
    const uint32_t mask = (1u << a.p.log2T) - 1u;
    for (int l = 0; l < L; ++l) {   // grid features -> B rows 0..IN0-1
        if (F == 4) {
            float f4[4];
            unerf_hash_level4(reinterpret_cast<const float4*>(a.p.table) + ((size_t)l << a.p.log2T), px, py, pz, a.p.scalings[l], mask, f4);
#pragma unroll
            for (int e = 0; e < 4; ++e) B[(4 * l + e) * 64 + lane] = f4[e];
        } else {
            float2 f;
            if (a.p.tcnn_levels && a.p.grid_half) f = unerf_tcnn_level_feat_half(a.p.table, a.p.tcnn_levels[l], px, py, pz);
            else if (a.p.tcnn_levels) f = unerf_tcnn_level_feat(reinterpret_cast<const float2*>(a.p.table), a.p.tcnn_levels[l], px, py, pz);
            else f = unerf_hash_level(reinterpret_cast<const float2*>(a.p.table) + ((size_t)l << a.p.log2T), px, py, pz, a.p.scalings[l], mask);
            B[(2 * l) * 64 + lane] = f.x;
            B[(2 * l + 1) * 64 + lane] = f.y;
        }
    }
    float sh[16];
    {
        float ux = (dxr + 1.f) / 2.f, uy = (dyr + 1.f) / 2.f, uz = (dzr + 1.f) / 2.f;
        if (a.p.sh_remap) {
            ux = ux * 2.f - 1.f;
            uy = uy * 2.f - 1.f;
            uz = uz * 2.f - 1.f;
        }
        unerf_sh16(ux, uy, uz, sh);
    }
    dense_any(a.p.w0t, a.p.b0, B, A, IN0, H, lane, MODE != UNERF_FIELD_LAPLACE);   // LAPLACE: bare Linear (utils.py:22-23)
    if constexpr (MODE == UNERF_FIELD_LAPLACE) {
        dense_any(a.p.w1t, a.p.b1, A, D, H, G, lane, false);                       // mlp_hidden: the geo features
        const int nl = a.p.n_lap, nr = a.p.n_lap_rgb;
        const size_t set = a.p.lap_chunk_rays ? (size_t)fastdiv(a.chunk0 + (uint32_t)r, a.div_chunk) : 0;
        float mu = 0.f, mu2 = 0.f;
        for (int q = 0; q < nl; ++q) {
            const float* __restrict__ w = a.p.ws_density + (set * nl + (size_t)q) * (size_t)(H + 1);
            float pre = 0.f;
            for (int i = 0; i < H; ++i) pre = fmaf(A[i * 64 + lane], w[i], pre);
            pre += w[H];
            const float pred = a.p.lap_softplus ? unerf_softplus(pre) : expf(pre);
            mu += pred;
            mu2 += pred * pred;
        }
        mu /= (float)nl;
        mu2 /= (float)nl;
        const float var_d = a.p.lap_mask_density ? 0.f : mu2 - mu * mu;
#pragma unroll
        for (int e = 0; e < 16; ++e) Cb[e * 64 + lane] = sh[e];
        for (int g = 0; g < G; ++g) Cb[(16 + g) * 64 + lane] = D[g * 64 + lane];
        dense_any(a.p.h0t, a.p.hb0, Cb, B, INC, HC, lane, true);
        dense_any(a.p.h1t, a.p.hb1, B, D, HC, HC, lane, true);
        float m1[3] = {0.f, 0.f, 0.f}, m2[3] = {0.f, 0.f, 0.f};
        for (int q = 0; q < nr; ++q) {
            const float* __restrict__ w = a.p.ws_rgb + (set * nr + (size_t)q) * (size_t)(3 * HC + 3);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float pre = 0.f;
                for (int i = 0; i < HC; ++i) pre = fmaf(D[i * 64 + lane], w[c * HC + i], pre);
                pre += w[3 * HC + c];
                const float pred = unerf_sigmoid(pre);
                m1[c] += pred;
                m2[c] += pred * pred;
            }
        }
        float vsum = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            m1[c] /= (float)nr;
            m2[c] /= (float)nr;
            vsum += fmaxf(m2[c] - m1[c] * m1[c], 0.f);
        }
        if (valid) {
            a.density[n] = a.p.lap_mask_density ? mu * sel : mu;
            a.aux[n] = var_d;
            a.aux2[n] = vsum / 3.f;
            a.rgb[n * 3 + 0] = m1[0];
            a.rgb[n * 3 + 1] = m1[1];
            a.rgb[n * 3 + 2] = m1[2];
        }
        return;
    } else {
        const int passes = (MODE == UNERF_FIELD_MCDROPOUT && a.p.K > 0) ? a.p.K : 1;
        const uint32_t sidx = (uint32_t)((uint64_t)a.ray_offset * (uint64_t)a.S + (uint64_t)n);
        const uint32_t pre = unerf_mc_pre(unerf_mc_key(a.p.seed, 0u), sidx);
        for (int k = 0; k < passes; ++k) {
            const float* src = A;
            if (a.drop_sites & UNERF_DROP_TRUNK) {
                mask_any(A, B, H, lane, pre, k, 0u, a.keep_hi, a.drop_scale);
                src = B;
            }
            dense_any(a.p.w1t, a.p.b1, src, D, H, OUT1, lane, false);
            const float density = a.p.average_init_density * expf(D[lane]) * sel;
            const float beta = MODE == UNERF_FIELD_ACTIVE ? unerf_softplus(D[(G + 1) * 64 + lane]) + a.p.beta_min : 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) Cb[e * 64 + lane] = sh[e];
            for (int g = 0; g < G; ++g) Cb[(16 + g) * 64 + lane] = D[(1 + g) * 64 + lane];
            if (a.drop_sites & UNERF_DROP_HEADIN) {   // Dropout on the head's inputs: the appearance block unfolded
                for (int e = 0; e < AD; ++e) Cb[(INC + e) * 64 + lane] = a.p.app_embed[e];
                mask_any(Cb, Cb, INC + AD, lane, pre, k, 3u, a.keep_hi, a.drop_scale);
                dense_any(a.p.h0_full_t, a.p.hb0_raw, Cb, B, INC + AD, HC, lane, true);
            } else {
                dense_any(a.p.h0t, a.p.hb0, Cb, B, INC, HC, lane, true);
            }
            if (a.drop_sites & UNERF_DROP_HEAD0) mask_any(B, B, HC, lane, pre, k, 2u, a.keep_hi, a.drop_scale);
            dense_any(a.p.h1t, a.p.hb1, B, D, HC, HC, lane, true);
            if (a.drop_sites & UNERF_DROP_HEAD1) mask_any(D, D, HC, lane, pre, k, 1u, a.keep_hi, a.drop_scale);
            dense_any(a.p.h2t, a.p.hb2, D, B, HC, 3, lane, false);
            if (valid) {
                const int64_t q = (int64_t)k * N + n;
                a.density[q] = density;
                a.rgb[q * 3 + 0] = unerf_sigmoid(B[lane]);
                a.rgb[q * 3 + 1] = unerf_sigmoid(B[64 + lane]);
                a.rgb[q * 3 + 2] = unerf_sigmoid(B[128 + lane]);
                if (MODE == UNERF_FIELD_ACTIVE) a.aux[n] = beta;
            }
        }
    }
}

// --------------------------------------------------------------------------------------
// 5b. MFMA variant (ACTIVE, MCDROPOUT).  v_mfma_f32_32x32x2_f32 = exact fp32 FMA chains at the
// fp32 vector rate; what it buys is operand delivery: one 256-B A fragment (weights, LDS
// resident for the lifetime of a persistent workgroup) feeds 2048 MACs, where the VALU kernel
// needs the scalar cache to deliver a weight pair for every 128 MACs (56 KB of weights do not
// fit the scalar cache, so that kernel runs at the L2 scalar-fetch rate, rocprof r1_01).
//
// Mapping: a wave owns a tile of 32 samples.  Samples sit on the MFMA columns (lane & 31), layer
// units on the rows, so D of one layer is directly the B operand of the next (no LDS, no
// shuffles).  The two lane halves hold the two k-slices of every step; for the hash grid that
// means half h looks up levels 8h..8h+7 of the same 32 samples.  Fragment/bias layout:
// ops.py::pack_field_mfma (emulated bit for bit in tests/test_mfma_pack_cpu.py).
// --------------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define MF_BIAS_OFF (160 * 64)
#define MF_H2_OFF (MF_BIAS_OFF + 7 * 32)

__device__ __forceinline__ f32x16 mf_bias(const float* lds, int k, int h) {
    const float4* b = reinterpret_cast<const float4*>(lds + MF_BIAS_OFF + (k * 2 + h) * 16);
    float4 b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
    f32x16 v = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w, b3.x, b3.y, b3.z, b3.w};
    return v;
}
// ReLU as a signed-integer max on the bit pattern: one v_max_i32 per element.  fmaxf() costs two
// VALU ops here (a canonicalising v_max before the real one, IEEE maxnum), and with ~10 VALU per
// MFMA the K-pass kernel is issue-bound (rocprof r1_04: MFMA busy 61 % + VALU busy 38 %).
// Negative floats (incl. -0.0) have negative bit patterns -> 0; non-negative ones pass unchanged.
__device__ __forceinline__ f32x16 mf_relu(f32x16 v) {
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = __int_as_float(max(__float_as_int(v[r]), 0));
    return v;
}
// acc += W_frag(frag0 + r) x src[r], r = 0..15 (one 16-step K slab)
__device__ __forceinline__ f32x16 mf_slab(const float* lds, int frag0, int lane, const f32x16& src, f32x16 acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[(frag0 + r) * 64 + lane], src[r], acc, 0, 0, 0);
    return acc;
}
// inverted dropout on one accumulator block (units 32*blk + row(r,h)).  Register pairs (r, r+1) are
// units (u, u+1) = one mask word; the lane keeps its 8 words per block in `st` across the passes.
// (base_h: unerf_mc_base_h of THIS lane half h -- bit 1 of the pair index u >> 1 is h, and the word constants are taken at
// that bit cleared, so they are compile-time literals)
__device__ __forceinline__ void mf_mask_init(uint32_t (&st)[8], int blk, int h, uint32_t base_h, uint32_t stream_id) {
    (void)h;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int r = 2 * q;
        const uint32_t u0 = 32u * blk + (r & 3) + 8 * (r >> 2);   // the unit at h = 0; + 4 h: bit 1 of the pair index
        st[q] = unerf_mask_word0(base_h, stream_id, u0 >> 1);
    }
}
__device__ __forceinline__ void mf_mask_step(uint32_t (&st)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) st[q] = unerf_mask_step(st[q]);
}
// the eight words of one block at pass k, recomputed from the sample's base hash (k chained steps): used only by the
// non-default dropout site UNERF_DROP_HEAD0, which therefore costs the default configuration no registers
__device__ __forceinline__ void mf_mask_words_at(uint32_t (&st)[8], int blk, int h, uint32_t base_h, uint32_t stream_id, int k) {
    mf_mask_init(st, blk, h, base_h, stream_id);
    for (int q = 0; q < k; ++q) mf_mask_step(st);
}
// EXPLICIT keep masks: the same eight words of block blk made of the sample's keep bits (`row`: xm_row) -- word q covers the
// units mf_mask_init states, 32 blk + 2 (q & 1) + 8 (q >> 1) + 4 h and the one after it
__device__ __forceinline__ void mf_xm_words(uint32_t (&st)[8], const uint32_t* row, int blk, int h) {
    const uint32_t bits = row[blk] >> (4 * h);
#pragma unroll
    for (int q = 0; q < 8; ++q) st[q] = xm_word(bits, 2 * (q & 1) + 8 * (q >> 1));
}
__device__ __forceinline__ f32x16 mf_dropout(f32x16 v, const uint32_t (&st)[8], int32_t thr_hi, float scale) {
    const bool all = field_keep_all(thr_hi);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        v[2 * q] = (all || unerf_keep_lo(st[q], thr_hi)) ? v[2 * q] * scale : 0.f;
        v[2 * q + 1] = (all || unerf_keep_hi(st[q], thr_hi)) ? v[2 * q + 1] * scale : 0.f;
    }
    return v;
}

// This half's 8 levels of the main grid for one sample -> the 16 k-steps of layer 0.
// Two batches of 4 levels: all 32 corner rows of a batch are requested back to back (uniform table
// base + 32-bit byte offset per lane), THEN blended.  Left to itself the compiler interleaves
// address math, 4-load groups and waits (about 20 dependent round trips per tile in the r1 ISA).
// PACKED picks the fp32x2 blend (fewer VALU issues, ~18 more VGPRs): right for the K-pass and Laplace
// kernels, which sit at 2 waves/SIMD anyway; the ACTIVE kernel keeps the scalar blend and its third wave
// (packed + 168-VGPR cap: 20 B of scratch, 22.2 vs 21.8 ms/frame).
// The 16 level records of a tcnn-layout grid, staged once per workgroup as five 16-entry LDS rows (scale, res,
// byte offset, size, dense): read per lane from the device array they were 40 vector loads per tile (the level
// index differs between the wave's halves, and loads after stores in the tile loop cannot be scalar).
#define MF_TL_WORDS 80
template <int RS = 3>   // log2 of the row size in bytes: 3 = fp32 rows, 2 = half2 rows (grid_half)
__device__ __forceinline__ void mf_stage_tcnn_levels(const FieldArgs& a, uint32_t* tl) {
    if (threadIdx.x < 16) {
        const unerf_tcnn_level lv = a.p.tcnn_levels[threadIdx.x];
        tl[threadIdx.x] = __float_as_uint(lv.scale);
        tl[16 + threadIdx.x] = lv.res;
        tl[32 + threadIdx.x] = lv.offset << RS;
        tl[48 + threadIdx.x] = lv.size;
        tl[64 + threadIdx.x] = lv.dense;
    }
}

// TCNN: 0 = nerfstudio's torch HashEncoding, 1 = tcnn layout on fp32 rows, 2 = tcnn layout in tcnn's own half arithmetic
// (unerf_field_params.grid_half: half2 rows, unerf_tcnn_blend_half).  TCNN == 2 also hands back the features as they
// come out of the blend -- `packed`[4 hb + q] = level 8 h + 4 hb + q as one half2 = operand quad [4 st .. 4 st + 3] of
// layer 0's k-step st: the f16 matrix kernels take them as they are (the floats returned hold the same values).
typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
template <bool PACKED, int TCNN>
__device__ __forceinline__ f32x16 mf_gather_feats(const FieldArgs& a, float px, float py, float pz, int h, uint32_t mask,
                                                  const uint32_t* tl = nullptr, u32x8* packed = nullptr) {
    f32x16 feat;
    if (TCNN == 2) {
        const char* tbase = reinterpret_cast<const char*>(a.p.table);
        u32x8 pk;
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            uint32_t cd[32];
            float wf[12];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int lev = 8 * h + 4 * hb + q;
                uint32_t off[8];
                unerf_tcnn_offsets<2>(__uint_as_float(tl[lev]), tl[16 + lev], tl[32 + lev], tl[48 + lev], tl[64 + lev], px, py, pz,
                                      off, wf[3 * q], wf[3 * q + 1], wf[3 * q + 2]);
#pragma unroll
                for (int k = 0; k < 8; ++k) cd[8 * q + k] = *reinterpret_cast<const uint32_t*>(tbase + off[k]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t c8[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) c8[k] = cd[8 * q + k];
                const uint32_t f = unerf_tcnn_blend_half(c8, wf[3 * q], wf[3 * q + 1], wf[3 * q + 2]);
                pk[4 * hb + q] = f;
                const float2 ff = unerf_h2_to_float2(f);
                feat[2 * (4 * hb + q)] = ff.x;
                feat[2 * (4 * hb + q) + 1] = ff.y;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (packed) *packed = pk;
        return feat;
    }
    if (TCNN) {  // tcnn-layout grid: same batching (4 levels = 32 corner rows in flight), tcnn indexing + blend
        const char* tbase = reinterpret_cast<const char*>(a.p.table);
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            float2 cd[32];
            float wf[12];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int lev = 8 * h + 4 * hb + q;
                uint32_t off[8];
                unerf_tcnn_offsets<3>(__uint_as_float(tl[lev]), tl[16 + lev], tl[32 + lev], tl[48 + lev], tl[64 + lev], px, py, pz,
                                      off, wf[3 * q], wf[3 * q + 1], wf[3 * q + 2]);
#pragma unroll
                for (int k = 0; k < 8; ++k) cd[8 * q + k] = *reinterpret_cast<const float2*>(tbase + off[k]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float2 c8[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) c8[k] = cd[8 * q + k];
                float2 f = unerf_tcnn_blend(c8, wf[3 * q], wf[3 * q + 1], wf[3 * q + 2]);
                feat[2 * (4 * hb + q)] = f.x;
                feat[2 * (4 * hb + q) + 1] = f.y;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        return feat;
    }
    const char* tbase = reinterpret_cast<const char*>(a.p.table);
#pragma unroll
    for (int hb = 0; hb < 2; ++hb) {
        float2 cd[32];
        float of[12];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int lev = 8 * h + 4 * hb + q;
            uint32_t off[8];
            // lev differs between the wave's halves: the table base stays uniform (SGPR) and the level
            // goes into the 32-bit lane offset (whole table < 2^32 bytes: L * 2^(log2T+3))
            unerf_hash_corners<true>(px, py, pz, a.p.scalings[lev], mask, off, of[3 * q], of[3 * q + 1], of[3 * q + 2],
                                     (uint32_t)lev << (a.p.log2T + 3));
#pragma unroll
            for (int k = 0; k < 8; ++k) cd[8 * q + k] = *reinterpret_cast<const float2*>(tbase + off[k]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float2 c8[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) c8[k] = cd[8 * q + k];
            float2 f = PACKED ? unerf_blend8(c8, of[3 * q], of[3 * q + 1], of[3 * q + 2])
                              : unerf_blend8_scalar(c8, of[3 * q], of[3 * q + 1], of[3 * q + 2]);
            feat[2 * (4 * hb + q)] = f.x;
            feat[2 * (4 * hb + q) + 1] = f.y;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    return feat;
}

template <int MODE, bool FEAT_IN, int TCNN = 0, typename... XA>   // XA = KeepArgs: explicit keep masks (MCDROPOUT)
// ACTIVE is bound by the gather (texture-address unit): three waves per SIMD (<= 168 VGPRs) hide more of
// its latency than two (measured 21.7 vs 23.7 ms/frame when a 176-VGPR build lost the third wave); the
// K-pass mode needs the registers instead.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((MODE == UNERF_FIELD_ACTIVE && TCNN != 1) ? 3 : 2)))
void field_kernel_mfma(FieldArgs a, uint32_t num_tiles, FastDiv div_s, XA... xa) {
    constexpr bool XM = sizeof...(XA) != 0;
    extern __shared__ float lds[];
    {
        const float4* src = reinterpret_cast<const float4*>(a.p.mfma_blob);
        float4* dst = reinterpret_cast<float4*>(lds);
        for (int i = threadIdx.x; i < UNERF_MFMA_BLOB_FLOATS / 4; i += 256) dst[i] = src[i];
    }
    __shared__ uint32_t s_tl[TCNN ? MF_TL_WORDS : 1];
    if (TCNN) mf_stage_tcnn_levels<(TCNN == 2 ? 2 : 3)>(a, s_tl);
    __syncthreads();
    // wave index as a scalar: the tile walk and its divisions then run on the scalar unit
    const int lane_c = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane_c & 31, h = lane_c >> 5;
    const int64_t N = a.R * (int64_t)a.S;
    const uint32_t mask = (1u << a.p.log2T) - 1u;
    // XCD-aware persistent walk: blocks b and b+8 share an XCD (L2); give each XCD one contiguous
    // eighth of the tiles so neighbouring rays (same coarse hash cells) meet in the same L2.
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, bpx = gridDim.x >> 3;
    const uint32_t tpx = (num_tiles + 7u) / 8u;  // num_tiles < 2^28 (the RNG counter bound in unerf_field_fwd)
    const uint32_t tile_end = (xcd + 1) * tpx < num_tiles ? (xcd + 1) * tpx : num_tiles;
    for (uint32_t tile = xcd * tpx + (uint32_t)slot * 4u + (uint32_t)wv; tile < tile_end; tile += (uint32_t)bpx * 4u) {
        // The LDS fragment reads are invariant across tiles; left alone, LICM hoists all 160 of
        // them into registers (490 VGPR+AGPR, scratch spills).  An opaque copy of the lane index
        // keeps them inside the iteration, where each read is consumed by the next MFMA.
        int lane = lane_c;
        asm volatile("" : "+v"(lane));
        // tile -> (block of 32 neighbouring rays, sample index s): the 32 columns of a tile are the SAME
        // sample slot of 32 adjacent pixels, which sit in the same or neighbouring grid cells, so a gather
        // instruction presents few distinct lines to the texture-address unit (it retires ~1 divergent
        // lane per clock: TA_BUSY 74 % with 32 consecutive samples of one ray per tile, rocprof r1_04)
        const TileSample ts = tile_sample(a, tile, div_s, j);
        const bool valid = ts.valid;
        const int64_t n = ts.n;
        const float dxr = ts.dx, dyr = ts.dy, dzr = ts.dz;
        float px = ts.px, py = ts.py, pz = ts.pz;
        const float sel = unerf_normalize_position(px, py, pz, a.box);

        // hash grid: this half's 8 levels -> 16 features = the 16 k-steps of layer 0
        f32x16 feat;
        if (FEAT_IN) {  // features were gathered level-major by field_gather_kernel: coalesced 8-B reads
            const float2* fp = reinterpret_cast<const float2*>(a.features);
#pragma unroll
            for (int l = 0; l < 8; ++l) {
                float2 f = fp[(int64_t)(8 * h + l) * N + n];
                feat[2 * l] = f.x;
                feat[2 * l + 1] = f.y;
            }
        } else {
            feat = mf_gather_feats<(MODE != UNERF_FIELD_ACTIVE), TCNN>(a, px, py, pz, h, mask, s_tl);
        }
        // Colour layer 0 sees [geo(15) | SH(16)]; the SH half does not depend on the MC pass, so its
        // 16 MFMAs (+ bias) are done once per tile and every pass starts from that partial sum.
        f32x16 csh0 = mf_bias(lds, 3, h), csh1 = mf_bias(lds, 4, h);
        {
            float sh[16];
            float ux = (dxr + 1.f) / 2.f, uy = (dyr + 1.f) / 2.f, uz = (dzr + 1.f) / 2.f;
            if (a.p.sh_remap) {
                ux = ux * 2.f - 1.f;
                uy = uy * 2.f - 1.f;
                uz = uz * 2.f - 1.f;
            }
            unerf_sh16(ux, uy, uz, sh);
            // this half feeds components 8h..8h+7.  Bitwise per-half select: a plain
            // `h ? sh[8+k] : sh[k]` is rewritten into a lane-indexed load from a scratch copy of sh[]
            const uint32_t hm = 0u - (uint32_t)h;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                float v = __uint_as_float((__float_as_uint(sh[8 + q]) & hm) | (__float_as_uint(sh[q]) & ~hm));
                csh0 = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[(64 + 8 + q) * 64 + lane], v, csh0, 0, 0, 0);
                csh1 = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[(80 + 8 + q) * 64 + lane], v, csh1, 0, 0, 0);
            }
        }

        // layer 0: 32 -> 64, ReLU
        f32x16 hid0 = mf_relu(mf_slab(lds, 0, lane, feat, mf_bias(lds, 0, h)));
        f32x16 hid1 = mf_relu(mf_slab(lds, 16, lane, feat, mf_bias(lds, 1, h)));

        const int passes = (MODE == UNERF_FIELD_MCDROPOUT && a.p.K > 0) ? a.p.K : 1;
        const bool drop = (MODE == UNERF_FIELD_MCDROPOUT) && a.drop_on;
        const uint32_t sidx = (uint32_t)((uint64_t)a.ray_offset * (uint64_t)a.S + (uint64_t)n);
        uint32_t mk0[8], mk1[8], mk2[8], mk3[8];  // this lane's mask words: trunk blk 0/1, head blk 0/1
        const uint32_t base0 = (drop && !XM) ? unerf_mc_base_h(unerf_mc_pre(unerf_mc_key(a.p.seed, 0u), sidx), (uint32_t)h) : 0u;   // this lane half's
        if (drop && !XM) {
            mf_mask_init(mk0, 0, h, base0, 0u);
            mf_mask_init(mk1, 1, h, base0, 0u);
            mf_mask_init(mk2, 0, h, base0, 1u);
            mf_mask_init(mk3, 1, h, base0, 1u);
        }
        for (int k = 0; k < passes; ++k) {
            asm volatile("" : "+v"(lane));  // same reason: keep the fragment reads inside the pass
            f32x16 m0 = hid0, m1 = hid1;
            if (drop) {
                if constexpr (XM) {   // this pass' words from the keep bits instead of a generator step
                    if (a.drop_sites & UNERF_DROP_TRUNK) {
                        mf_xm_words(mk0, xm_row(xm_of(xa...), 0, k, n), 0, h);
                        mf_xm_words(mk1, xm_row(xm_of(xa...), 0, k, n), 1, h);
                    }
                    if (a.drop_sites & UNERF_DROP_HEAD1) {
                        mf_xm_words(mk2, xm_row(xm_of(xa...), 2, k, n), 0, h);
                        mf_xm_words(mk3, xm_row(xm_of(xa...), 2, k, n), 1, h);
                    }
                } else if (k > 0) {
                    mf_mask_step(mk0);
                    mf_mask_step(mk1);
                    mf_mask_step(mk2);
                    mf_mask_step(mk3);
                }
                if (a.drop_sites & UNERF_DROP_TRUNK) {
                    m0 = mf_dropout(hid0, mk0, a.keep_hi, a.drop_scale);
                    m1 = mf_dropout(hid1, mk1, a.keep_hi, a.drop_scale);
                }
            }
            // trunk out: 64 -> out1 (rows >= out1 are zero-padded): row 0 density, 1..15 geo, 16 beta
            f32x16 t = mf_bias(lds, 2, h);
            t = mf_slab(lds, 32, lane, m0, t);
            t = mf_slab(lds, 48, lane, m1, t);
            // colour 0: the geo rows of t (regs 0..7) on top of the per-tile SH partial sum, ReLU
            f32x16 c0 = csh0, c1 = csh1;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[(64 + q) * 64 + lane], t[q], c0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[(80 + q) * 64 + lane], t[q], c1, 0, 0, 0);
            }
            c0 = mf_relu(c0);
            c1 = mf_relu(c1);
            if (drop && (a.drop_sites & UNERF_DROP_HEAD0)) {   // rgb_dropout_layers contains 1: Dropout in front of Linear 1
                uint32_t mw[8];
                if constexpr (XM) mf_xm_words(mw, xm_row(xm_of(xa...), 1, k, n), 0, h);
                else mf_mask_words_at(mw, 0, h, base0, 2u, k);
                c0 = mf_dropout(c0, mw, a.keep_hi, a.drop_scale);
                if constexpr (XM) mf_xm_words(mw, xm_row(xm_of(xa...), 1, k, n), 1, h);
                else mf_mask_words_at(mw, 1, h, base0, 2u, k);
                c1 = mf_dropout(c1, mw, a.keep_hi, a.drop_scale);
            }
            // colour 1: 64 -> 64, ReLU
            f32x16 d0 = mf_bias(lds, 5, h), d1 = mf_bias(lds, 6, h);
            d0 = mf_slab(lds, 96, lane, c0, d0);
            d0 = mf_slab(lds, 112, lane, c1, d0);
            d1 = mf_slab(lds, 128, lane, c0, d1);
            d1 = mf_slab(lds, 144, lane, c1, d1);
            d0 = mf_relu(d0);
            d1 = mf_relu(d1);
            if (drop && (a.drop_sites & UNERF_DROP_HEAD1)) {
                d0 = mf_dropout(d0, mk2, a.keep_hi, a.drop_scale);
                d1 = mf_dropout(d1, mk3, a.keep_hi, a.drop_scale);
            }
            // colour 2: 64 -> 3 on the VALU: each half sums its 32 units, halves meet by one shuffle
            float rgbv[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* w0p = lds + MF_H2_OFF + ((0 * 2 + h) * 3 + c) * 16;
                const float* w1p = lds + MF_H2_OFF + ((1 * 2 + h) * 3 + c) * 16;
                float acc = 0.f;
#pragma unroll
                for (int q = 0; q < 16; ++q) acc = fmaf(d0[q], w0p[q], acc);
#pragma unroll
                for (int q = 0; q < 16; ++q) acc = fmaf(d1[q], w1p[q], acc);
                acc += __shfl_xor(acc, 32, 64);
                rgbv[c] = unerf_sigmoid(acc + lds[MF_H2_OFF + 192 + c]);
            }
            if (valid && h == 0) {
                const OutIndex q = out_index(a, k, ts);
                const float sigma = a.p.average_init_density * expf(t[0]) * sel;
                if (a.p.packed_out) {   // uniform
                    store_packed(a, k, ts.n, sigma, rgbv[0], rgbv[1], rgbv[2]);
                } else {
                    a.density[q.dens] = sigma;
                    a.rgb[q.rgb] = rgbv[0];
                    a.rgb[q.rgb + q.rgb_stride] = rgbv[1];
                    a.rgb[q.rgb + 2 * q.rgb_stride] = rgbv[2];
                }
                if (MODE == UNERF_FIELD_ACTIVE) a.aux[q.aux] = unerf_softplus(t[8]) + a.p.beta_min;
            }
        }
    }
}

// --------------------------------------------------------------------------------------
// 5b''. Split-f16 variant of 5b (ACTIVE, MCDROPOUT): the same network, same tile mapping, same gathers and
// epilogues, but the dense layers run on v_mfma_f32_32x32x16_f16 with every fp32 operand carried as two
// halves (hi = f16(x), lo = f16(x - hi): 22 mantissa bits) and hi*hi + hi*lo + lo*hi accumulated in fp32.
// Why: the fp32-input MFMA runs at the fp32 VECTOR rate and does not overlap with VALU work (rocprof
// r1_05: MFMA-busy 58 % + VALU-busy 35 % = the elapsed cycles), so the exact-fp32 kernel spends 10.2 k of
// its 17.4 k cycles per tile in 160 MFMAs.  The f16 matrix pipe is 16x faster per k-step; three products
// per step leave 60 MFMAs x ~36 cycles = 2.2 k cycles, plus ~3 VALU per activation element for the split.
// Accuracy: dropped lo*lo term and the rounding of lo are each <= 2^-22 relative per product, i.e. the
// result is fp32-equivalent (|d rgb| ~ 1e-7; tests/test_gpu_nerf_kernels.py bounds it against the exact
// kernel, the e2e PSNR / AUSE gates are unchanged).  f16 subnormal inputs are honoured by the MFMA
// (benchmarks/mfma_f16_probe.hip); operands must stay below 65504 in magnitude (checked for the weights at
// pack time; activations of a trained nerfacto field are orders of magnitude smaller).
// Operand order: accumulator registers 8s..8s+7 of a lane in half g are layer units
// 16s + 4g + (e&3) + 8(e>>2) -- the k order of the next layer's B operand, hence the order
// ops.pack_field_mfma16 packs the A slabs in.  LDS blob: 20 slabs x (hi|lo) x 64 lanes x 16 B = 40 KiB, then
// the same bias rows / rgb layer as the fp32 blob (same offsets, same total size).
// --------------------------------------------------------------------------------------
// MC-dropout on PACKED f16 operands.  The inverted-dropout scale 1/(1-p) is folded into the weights of the layer
// that follows (ops.pack_field_mfma16(drop_scale=...)), so a dropped unit is just a zeroed operand, and an operand
// pair (units 2j, 2j+1 = the two halves of one register of the hi and of the lo quad) is zeroed by ONE and with a
// mask whose halves are 0xFFFF / 0.  That mask costs two packed instructions per RNG word: the saturating signed
// difference half - thr_s is negative exactly when the unit is kept (v_pk_sub_i16 clamp), and an arithmetic shift
// by 15 spreads the sign over the half (v_pk_ashrrev_i16).  Per unit: 1 (mask) + 1 (two ands) instructions, against
// compare + select on the fp32 accumulator (2) in round 1 -- and the trunk layer's input is pass-invariant, so its
// operand split (1.5 per unit) moves out of the K loop altogether.
__device__ __forceinline__ f32x16 mf_dropout_keep(f32x16 v, const uint32_t (&st)[8], int32_t thr_hi) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        v[2 * q] = unerf_keep_lo(st[q], thr_hi) ? v[2 * q] : 0.f;
        v[2 * q + 1] = unerf_keep_hi(st[q], thr_hi) ? v[2 * q + 1] : 0.f;
    }
    return v;
}
typedef short i16x2 __attribute__((ext_vector_type(2)));
// keep test of the two units of a mask word: unit kept <=> its half of the difference is negative
__device__ __forceinline__ uint32_t mf16_keep_diff(uint32_t word, uint32_t thr_pk) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(i16x2, word), __builtin_bit_cast(i16x2, thr_pk)));
}
__device__ __forceinline__ uint32_t mf16_keep_mask(uint32_t word, uint32_t thr_pk) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(i16x2, mf16_keep_diff(word, thr_pk)) >> (short)15);
}
// sigmoid on the hardware exp / rcp (v_exp_f32, v_rcp_f32: ~1e-7 relative each) instead of the ~25-instruction
// exact expf + IEEE division
__device__ __forceinline__ float mf_sigmoid_fast(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
// softplus on the hardware exp / log (density_activation = "softplus", laplace_model.py:151): log1p by its series
// where 1 + e would round e away
__device__ __forceinline__ float mf_softplus_fast(float x) {
    const float e = __expf(x);
    const float small = e * (1.f - e * (0.5f - e * (1.f / 3.f)));
    return x > 20.f ? x : (e < 1e-3f ? small : __logf(1.f + e));
}

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// Two elements per step: hi = v_cvt_pk_f16_f32(x0, x1) (round to nearest even), then each residual
// x - float(hi) is formed and rounded to f16 inside ONE mixed-precision fma (v_fma_mixlo/mixhi_f16: f16 and f32
// sources, exact internal product and sum): 1.5 VALU per element instead of the ~3 of convert-back / subtract /
// convert (the kernels are VALU-issue-bound once the matrix work is on the f16 pipe).
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// F1 (every helper below, and the kernels): the REFERENCE-PRECISION form, `precision = "f16"` / unerf_field_params.f16_single.
// One f16 product per MAC with fp32 accumulation: operands rounded to f16 once (v_cvt_pk_f16_f32 for the activations,
// the hi halves of the packed weights), no lo halves anywhere -- the arithmetic of torch.autocast(float16) Linear layers
// (forced at eval by mcdropout_models.py:86-92) and at least that of tiny-cuda-nn's FullyFusedMLP (fp16 weights,
// activations AND accumulators; the reference's default implementation="tcnn", activenerfacto_field.py:89).  A third of
// the split form's MFMAs and none of its 1.5-instruction-per-element residual splits.
template <bool F1 = false>
__device__ __forceinline__ void mf16_split8(const float (&x)[8], f16x8& hi, f16x8& lo) {
    u32x4 hv, lv;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const f16x2 hh = {(_Float16)x[2 * p], (_Float16)x[2 * p + 1]};
        hv[p] = lv[p] = __builtin_bit_cast(uint32_t, hh);   // F1: lo is never read in this form
    }
    if (!F1) {
        // The eight residuals of a k-step operand in ONE assembly statement that ends in two wait states.  An MFMA must not
        // read a VGPR within two wait states of a VALU write to it (and a VALU instruction not within one of a half-register
        // write); the compiler places those for the instructions it knows, and does not look inside inline assembly: written
        // as one statement per instruction (rounds 2 - 4) the listing had MFMAs ONE instruction behind the v_fma_mixhi_f16
        // that completes their B operand.  No run of the test suite ever differed because of it -- the other wave of the
        // SIMD usually separates the two -- but nothing guaranteed that.
        uint32_t l0, l1, l2, l3;
        asm("v_fma_mixlo_f16 %0, %4, -1.0, %8 op_sel:[0,0,0] op_sel_hi:[1,0,0]\n\t"
            "v_fma_mixlo_f16 %1, %5, -1.0, %10 op_sel:[0,0,0] op_sel_hi:[1,0,0]\n\t"
            "v_fma_mixlo_f16 %2, %6, -1.0, %12 op_sel:[0,0,0] op_sel_hi:[1,0,0]\n\t"
            "v_fma_mixlo_f16 %3, %7, -1.0, %14 op_sel:[0,0,0] op_sel_hi:[1,0,0]\n\t"
            "v_fma_mixhi_f16 %0, %4, -1.0, %9 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
            "v_fma_mixhi_f16 %1, %5, -1.0, %11 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
            "v_fma_mixhi_f16 %2, %6, -1.0, %13 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
            "v_fma_mixhi_f16 %3, %7, -1.0, %15 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
            "s_nop 1"
            : "=&v"(l0), "=&v"(l1), "=&v"(l2), "=&v"(l3)
            : "v"(hv[0]), "v"(hv[1]), "v"(hv[2]), "v"(hv[3]), "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]),
              "v"(x[6]), "v"(x[7]));
        lv[0] = l0; lv[1] = l1; lv[2] = l2; lv[3] = l3;
    }
    hi = __builtin_bit_cast(f16x8, hv);
    lo = __builtin_bit_cast(f16x8, lv);
}
template <bool F1 = false>
__device__ __forceinline__ void mf16_split(const f32x16& v, int s, f16x8& hi, f16x8& lo) {
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = v[8 * s + e];
    mf16_split8<F1>(x, hi, lo);
}
// F1: ReLU AFTER the conversion, on the packed halves: v_pk_max_i16(bits, 0) maps every negative f16 (sign bit = negative
// int16, -0 included) to +0 and leaves the others alone -- relu(cvt(x)) = cvt(relu(x)) exactly, at one instruction per
// TWO units instead of one v_max_i32 per unit on the fp32 accumulators.
__device__ __forceinline__ void mf16_split_relu(const f32x16& v, int s, f16x8& hi) {
    u32x4 hv;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        // (a VECTOR fptrunc: from two scalar conversions behind an integer max the compiler converts the halves one by one
        // and packs them with a v_perm -- three instructions where v_cvt_pk_f16_f32 is one.  Not inline asm: the
        // compiler has to see this read of MFMA results to place the wait states between the two.)
        const unerf_v2f pr = {v[8 * s + 2 * p], v[8 * s + 2 * p + 1]};
        const uint32_t w = __builtin_bit_cast(uint32_t, __builtin_convertvector(pr, f16x2));
        const i16x2 z = {0, 0};
        hv[p] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(i16x2, w), z));
    }
    hi = __builtin_bit_cast(f16x8, hv);
}
// ... and the keep masks of a dropout site with it, one instruction per two units (cvt, sub, bitop3, max): a dropped unit
// (keep difference d = sub_sat(word, thr) >= 0, sign clear) gets its sign bit set, and the integer max maps it to +0 with
// the negatives.  max_i16(x | (~d & 0x80008000), 0) = max_i16(x, 0) & (d >> 15) for every x, NaNs included: the same bits
// as mf16_split_relu + mf16_apply_masks in one instruction less.  d: the four words' mf16_keep_diff.
__device__ __forceinline__ void mf16_split_relu_drop(const f32x16& v, int s, const u32x4& d, f16x8& hi) {
    u32x4 hv;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const unerf_v2f pr = {v[8 * s + 2 * p], v[8 * s + 2 * p + 1]};
        const uint32_t w = __builtin_bit_cast(uint32_t, __builtin_convertvector(pr, f16x2)) | (~d[p] & 0x80008000u);
        const i16x2 z = {0, 0};
        hv[p] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(i16x2, w), z));
    }
    hi = __builtin_bit_cast(f16x8, hv);
}
// one lane's 16-byte operand quad from the LDS blob (every slab offset is a multiple of 16 bytes and the dynamic LDS base is
// 16-byte aligned).  Without the stated alignment the compiler reads some quads (the trunk-out and colour-2 slabs) as two
// ds_read2_b32 + two address adds: 4 VALU and 4 LDS instructions per pass more in the K-pass kernel.
__device__ __forceinline__ f16x8 mf16_lds_op(const float* p) {
    return *reinterpret_cast<const f16x8*>(__builtin_assume_aligned(p, 16));
}
// acc += W(slab) x B: small terms first
template <bool F1 = false>
__device__ __forceinline__ f32x16 mf16_mac(const float* lds, int slab, int lane, const f16x8& bhi, const f16x8& blo,
                                           f32x16 acc) {
    const f16x8 ahi = *reinterpret_cast<const f16x8*>(lds + slab * 512 + lane * 4);
    if (F1) return __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, bhi, acc, 0, 0, 0);
    const f16x8 alo = *reinterpret_cast<const f16x8*>(lds + slab * 512 + 256 + lane * 4);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, bhi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, blo, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, bhi, acc, 0, 0, 0);
    return acc;
}
// two row blocks against one B operand, the two accumulator chains interleaved.  (Round 2 read benchmarks/mfma_data_probe.hip
// as "an MFMA whose SrcC is the result of the MFMA right before it issues 16 cycles late"; round 6's hand-written sweep,
// benchmarks/issue_sweep_probe.hip, measures 32.3 cycles per MFMA on ONE chain as on two at every occupancy.  The interleave
// costs nothing and stays.)
// LOZ: the activations are half values already (tcnn's half grid features): their lo residual is zero and the W_hi x lo
// product is dropped
template <bool F1 = false, bool LOZ = false>
__device__ __forceinline__ void mf16_mac2(const float* lds, int slab_a, int slab_b, int lane, const f16x8& bhi, const f16x8& blo,
                                          f32x16& o0, f32x16& o1) {
    const f16x8 ahi0 = *reinterpret_cast<const f16x8*>(lds + slab_a * 512 + lane * 4);
    const f16x8 ahi1 = *reinterpret_cast<const f16x8*>(lds + slab_b * 512 + lane * 4);
    if (F1) {
        o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi0, bhi, o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi1, bhi, o1, 0, 0, 0);
        return;
    }
    const f16x8 alo0 = *reinterpret_cast<const f16x8*>(lds + slab_a * 512 + 256 + lane * 4);
    const f16x8 alo1 = *reinterpret_cast<const f16x8*>(lds + slab_b * 512 + 256 + lane * 4);
    o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo0, bhi, o0, 0, 0, 0);
    o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo1, bhi, o1, 0, 0, 0);
    if (!LOZ) {
        o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi0, blo, o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi1, blo, o1, 0, 0, 0);
    }
    o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi0, bhi, o0, 0, 0, 0);
    o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi1, bhi, o1, 0, 0, 0);
}
// layer 0's operand quad of k-step st: split (or, F1, rounded) from the fp32 features, or -- TCNN == 2 -- the packed half
// features of mf_gather_feats as they are (no conversion, no residual: mf16_mac2<F1, true>)
template <int TCNN, bool F1>
__device__ __forceinline__ void mf16_feat_operand(const f32x16& feat, const u32x8& pk, int st, f16x8& bhi, f16x8& blo) {
    if (TCNN == 2) {
        const u32x4 q = {pk[4 * st], pk[4 * st + 1], pk[4 * st + 2], pk[4 * st + 3]};
        bhi = blo = __builtin_bit_cast(f16x8, q);
    } else {
        mf16_split<F1>(feat, st, bhi, blo);
    }
}
// Folded slab (ops.pack_field_mfma16: fold_trunk) of a layer with <= 16 output rows: the slab's second operand holds
// rows 0..15 = W_hi and rows 16..31 = W_lo, so one MFMA against the hi halves of the activations produces W_hi a_hi in
// accumulator registers 0..7 and W_lo a_hi in registers 8..15 of the same lane (row(r + 8) = row(r) + 16); the first
// operand (W_hi, rows 16..31 zero) takes the lo halves.  Two MFMAs per k-step instead of three; the caller adds
// registers r + 8 onto r once per layer (mf16_fold_rows).
__device__ __forceinline__ f32x16 mf16_mac_fold_ops(const f16x8& ahi, const f16x8& amix, const f16x8& bhi, const f16x8& blo,
                                                    f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, blo, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(amix, bhi, acc, 0, 0, 0);
    return acc;
}
__device__ __forceinline__ f32x16 mf16_fold_rows(f32x16 acc) {
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] += acc[r + 8];
    return acc;
}
// a 64-wide layer input held as two accumulator blocks (units 0..31 in v0, 32..63 in v1) against the
// 4 k-steps x NB row blocks of slabs starting at `slab0` (slab = slab0 + NB*step + block)
template <int NB, bool F1 = false, bool RELU_PACKED = false>
__device__ __forceinline__ void mf16_layer64(const float* lds, int slab0, int lane, const f32x16& v0, const f32x16& v1,
                                             f32x16& o0, f32x16& o1) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        f16x8 bhi, blo;
        if (RELU_PACKED) {   // (F1 only) the input's ReLU rides on the converted operands
            mf16_split_relu(s < 2 ? v0 : v1, s & 1, bhi);
            blo = bhi;
        } else {
            mf16_split<F1>(s < 2 ? v0 : v1, s & 1, bhi, blo);
        }
        if (NB == 2) mf16_mac2<F1>(lds, slab0 + NB * s, slab0 + NB * s + 1, lane, bhi, blo, o0, o1);
        else o0 = mf16_mac<F1>(lds, slab0 + NB * s, lane, bhi, blo, o0);
    }
}

// split-f16 blob (ops.pack_field_mfma16): 20 operand slabs, then the bias rows and the fp32 rgb layer at the
// offsets of the fp32 blob (same total size)
#define mf16_bias mf_bias
// and both operand quads of k-step `st` (accumulator registers 8 st .. 8 st + 7 = mask words 4 st .. 4 st + 3 of
// the block's eight) with their keep masks
template <bool F1 = false>
__device__ __forceinline__ void mf16_apply_masks(f16x8& hi, f16x8& lo, const uint32_t (&words)[8], int st, uint32_t thr_pk) {
    u32x4 m;
#pragma unroll
    for (int p = 0; p < 4; ++p) m[p] = mf16_keep_mask(words[4 * st + p], thr_pk);
    hi = __builtin_bit_cast(f16x8, __builtin_bit_cast(u32x4, hi) & m);
    if (!F1) lo = __builtin_bit_cast(f16x8, __builtin_bit_cast(u32x4, lo) & m);
}

// SITES = false: the reference's default Dropout placement (trunk + last head layer), every site test a compile-time
// constant.  SITES = true: any other unerf_field_params.drop_sites (run-time site tests, and the words of the
// UNERF_DROP_HEAD0 site recomputed per pass).  A separate instantiation: as run-time branches of the default kernel
// they cost that kernel 50 VGPRs and 84 bytes of scratch (K = 8 field kernel 50 -> 55.6 ms).
// DROP: masks are generated (MCDROPOUT with K > 0 and p > 0).  A compile-time flag: as a run-time (uniform) flag every
// k-step of the masked layers carried a branch and the operand quads were copied to merge the two paths.
// XA = KeepArgs: explicit keep masks (unerf_field_fwd_masked), on the general SITES form
// Which of the three (SITES, DROP) forms a call gets: field_launch(); its LDS bytes: mf16_lds_bytes().
#define UNERF_MFMA16_KERNEL field_kernel_mfma16
#define UNERF_MFMA16_VIEWS false
#include "unerf_field_mfma16.inc"
#undef UNERF_MFMA16_KERNEL
#undef UNERF_MFMA16_VIEWS
// the same kernel under the name its several-views instantiations carry (MCDROPOUT, generated masks, default sites)
#define UNERF_MFMA16_KERNEL views_kpass_kernel_mfma16
#define UNERF_MFMA16_VIEWS true
#include "unerf_field_mfma16.inc"
#undef UNERF_MFMA16_KERNEL
#undef UNERF_MFMA16_VIEWS

// --------------------------------------------------------------------------------------
// 5b'. LAPLACE on the matrix cores.  The reference evaluates the two sampled last layers in a
// 100-iteration Python loop of GEMVs (laplace_field.py:553-560); as a matrix product the weight
// SAMPLES are the output rows: density head 128(100) x 64, colour head 3 x 128(100) x 64 per
// 32-sample tile, followed by exp / sigmoid and the running sums of p and p^2 on the accumulator
// registers (rows = registers + lane half).  Padded rows carry bias -1e30 -> contribute exactly 0.
// The 512 sampled-head fragments (128 KB) do not fit LDS next to the base network; they stream
// from L2 with coalesced 256-B loads (one per MFMA), the base network stays LDS-resident.
// --------------------------------------------------------------------------------------
#define LAP_BLOCKS 4
#define LAP_BIAS_OFF (4 * LAP_BLOCKS * 32 * 64)

// One sampled head (q) over its LAP_BLOCKS row blocks.  The A fragments come from L2 (one coalesced
// 256-B load per MFMA); the 32 fragments of block b+1 are requested BEFORE the 32 MFMAs of block b
// issue, so ~2000 cycles of matrix work cover their latency (without this every MFMA waited on its
// own load: 254 ms/frame instead of the ~70 ms the MFMA count predicts).
template <bool SIGMOID>
__device__ __forceinline__ void mf_lap_head(const float* __restrict__ lap, int q, int lane, int h, const f32x16& s0,
                                            const f32x16& s1, float& sum1, float& sum2, int softplus = 0) {
    sum1 = 0.f;
    sum2 = 0.f;
    float cur[32], nxt[32];
    {
        const float* f = lap + (size_t)((q * LAP_BLOCKS + 0) * 32) * 64 + lane;
#pragma unroll
        for (int r = 0; r < 32; ++r) cur[r] = f[r * 64];
    }
#pragma unroll
    for (int b = 0; b < LAP_BLOCKS; ++b) {
        if (b + 1 < LAP_BLOCKS) {
            const float* f = lap + (size_t)((q * LAP_BLOCKS + b + 1) * 32) * 64 + lane;
#pragma unroll
            for (int r = 0; r < 32; ++r) nxt[r] = f[r * 64];
        }
        const float4* bp = reinterpret_cast<const float4*>(lap + LAP_BIAS_OFF + ((q * LAP_BLOCKS + b) * 2 + h) * 16);
        float4 b0 = bp[0], b1 = bp[1], b2 = bp[2], b3 = bp[3];
        f32x16 acc = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w, b3.x, b3.y, b3.z, b3.w};
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[r], s0[r], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[16 + r], s1[r], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            // hardware exp / rcp (v_exp_f32, v_rcp_f32: ~1e-6 relative) instead of the ~25-instruction exact
            // expf / division: 16 activations follow every 32 MFMAs here and would otherwise take as long as
            // the matrix work.  The results only enter means / variances over the n_lap samples.
            float p = SIGMOID ? __builtin_amdgcn_rcpf(1.f + __expf(-acc[r])) : (softplus ? mf_softplus_fast(acc[r]) : __expf(acc[r]));
            sum1 += p;
            sum2 += p * p;
        }
        __builtin_amdgcn_sched_barrier(0);
        if (b + 1 < LAP_BLOCKS) {
#pragma unroll
            for (int r = 0; r < 32; ++r) cur[r] = nxt[r];
        }
    }
    sum1 += __shfl_xor(sum1, 32, 64);
    sum2 += __shfl_xor(sum2, 32, 64);
}

// store one accumulator block (rows = units 32*blk + (r&3) + 8*(r>>2) + 4h of sample n) to a [N][64] plane
__device__ __forceinline__ void mf_store_units(float* plane, int64_t n, int blk, int h, const f32x16& v) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4*>(plane + n * 64 + 32 * blk + 8 * q + 4 * h) =
            make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}
// this lane's half of a 64-wide dot product with a weight row in global memory (mean last layer)
__device__ __forceinline__ float mf_half_dot(const float* __restrict__ w, int h, const f32x16& v0, const f32x16& v1) {
    float acc = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc = fmaf(v0[r], w[(r & 3) + 8 * (r >> 2) + 4 * h], acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc = fmaf(v1[r], w[32 + (r & 3) + 8 * (r >> 2) + 4 * h], acc);
    return acc + __shfl_xor(acc, 32, 64);
}

// CAPTURE = the deterministic (is_inference=False) forward for GGN fitting: ws_density / ws_rgb hold the MEAN
// last layers, density = exp(.) * selector (laplace_field.py:317-345), rgb = sigmoid(.), and the inputs of the
// two last layers (base_mlp output, colour hidden) are written to [N][64] planes a.aux / a.aux2.
template <bool CAPTURE, int TCNN = 0>
__global__ __launch_bounds__(256) void field_kernel_mfma_laplace(FieldArgs a, uint32_t num_tiles, FastDiv div_s) {
    extern __shared__ float lds[];
    {
        const float4* src = reinterpret_cast<const float4*>(a.p.mfma_blob);
        float4* dst = reinterpret_cast<float4*>(lds);
        for (int i = threadIdx.x; i < UNERF_MFMA_BLOB_FLOATS / 4; i += 256) dst[i] = src[i];
    }
    __shared__ uint32_t s_tl[TCNN ? MF_TL_WORDS : 1];
    if (TCNN) mf_stage_tcnn_levels<(TCNN == 2 ? 2 : 3)>(a, s_tl);
    __syncthreads();
    // wave index as a scalar: the tile walk and its divisions then run on the scalar unit
    const int lane_c = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane_c & 31, h = lane_c >> 5;
    const int64_t N = a.R * (int64_t)a.S;
    const uint32_t mask = (1u << a.p.log2T) - 1u;
    const float inv_n = 1.f / (float)a.p.n_lap, inv_nr = 1.f / (float)a.p.n_lap_rgb;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, bpx = gridDim.x >> 3;
    const uint32_t tpx = (num_tiles + 7u) / 8u;  // num_tiles < 2^28 (the RNG counter bound in unerf_field_fwd)
    const uint32_t tile_end = (xcd + 1) * tpx < num_tiles ? (xcd + 1) * tpx : num_tiles;
    for (uint32_t tile = xcd * tpx + (uint32_t)slot * 4u + (uint32_t)wv; tile < tile_end; tile += (uint32_t)bpx * 4u) {
        int lane = lane_c;  // opaque per iteration: keeps the (tile-invariant) fragment reads in the loop
        asm volatile("" : "+v"(lane));
        // tile -> (block of 32 neighbouring rays, sample index s): the 32 columns of a tile are the SAME
        // sample slot of 32 adjacent pixels, which sit in the same or neighbouring grid cells, so a gather
        // instruction presents few distinct lines to the texture-address unit (it retires ~1 divergent
        // lane per clock: TA_BUSY 74 % with 32 consecutive samples of one ray per tile, rocprof r1_04)
        const TileSample ts = tile_sample(a, tile, div_s, j);
        const bool valid = ts.valid;
        const int64_t n = ts.n;
        const float dxr = ts.dx, dyr = ts.dy, dzr = ts.dz;
        float px = ts.px, py = ts.py, pz = ts.pz;
        // inference: the returned mu_d is NOT selector-masked (laplace_field.py:356-362)
        const float sel = unerf_normalize_position(px, py, pz, a.box);
        f32x16 feat = mf_gather_feats<true, TCNN>(a, px, py, pz, h, mask, s_tl);

        // base_mlp is a bare Linear: no ReLU (utils.py:22-23)
        f32x16 hb0 = mf_slab(lds, 0, lane, feat, mf_bias(lds, 0, h));
        f32x16 hb1 = mf_slab(lds, 16, lane, feat, mf_bias(lds, 1, h));
        // geo = mlp_hidden(hb): rows 0..14
        f32x16 t = mf_bias(lds, 2, h);
        t = mf_slab(lds, 32, lane, hb0, t);
        t = mf_slab(lds, 48, lane, hb1, t);
        // density head: mean / variance of exp(w_s . hb + b_s) over the n_lap sampled rows
        float mu_d, mu2_d = 0.f;
        if (CAPTURE) {
            const float pre_d = mf_half_dot(a.p.ws_density, h, hb0, hb1) + a.p.ws_density[64];
            mu_d = (a.p.lap_softplus ? unerf_softplus(pre_d) : expf(pre_d)) * sel;
            if (valid) {
                mf_store_units(a.aux, n, 0, h, hb0);
                mf_store_units(a.aux, n, 1, h, hb1);
            }
        } else {
            float d1, d2;
            mf_lap_head<false>(lap_set_blob(a, a.p.lap_blob, tile, div_s), 0, lane, h, hb0, hb1, d1, d2, a.p.lap_softplus);
            mu_d = d1 * inv_n;
            mu2_d = d2 * inv_n;
            if (a.p.lap_mask_density) {  // use_deterministic_density: selector-masked mean, no variance
                mu_d *= sel;
                mu2_d = mu_d * mu_d;
            }
        }

        // colour trunk
        f32x16 c0 = mf_bias(lds, 3, h), c1 = mf_bias(lds, 4, h);
        {
            float sh[16];
            float ux = (dxr + 1.f) / 2.f, uy = (dyr + 1.f) / 2.f, uz = (dzr + 1.f) / 2.f;
            if (a.p.sh_remap) {
                ux = ux * 2.f - 1.f;
                uy = uy * 2.f - 1.f;
                uz = uz * 2.f - 1.f;
            }
            unerf_sh16(ux, uy, uz, sh);
            const uint32_t hm = 0u - (uint32_t)h;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[(64 + q) * 64 + lane], t[q], c0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[(80 + q) * 64 + lane], t[q], c1, 0, 0, 0);
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                float v = __uint_as_float((__float_as_uint(sh[8 + q]) & hm) | (__float_as_uint(sh[q]) & ~hm));
                c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[(64 + 8 + q) * 64 + lane], v, c0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[(80 + 8 + q) * 64 + lane], v, c1, 0, 0, 0);
            }
        }
        c0 = mf_relu(c0);
        c1 = mf_relu(c1);
        f32x16 x0 = mf_bias(lds, 5, h), x1 = mf_bias(lds, 6, h);
        x0 = mf_slab(lds, 96, lane, c0, x0);
        x0 = mf_slab(lds, 112, lane, c1, x0);
        x1 = mf_slab(lds, 128, lane, c0, x1);
        x1 = mf_slab(lds, 144, lane, c1, x1);
        x0 = mf_relu(x0);
        x1 = mf_relu(x1);
        // colour head: per channel mean / variance of sigmoid(w_s . x + b_s)
        float mu_c[3], vsum = 0.f;
        if (CAPTURE) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                mu_c[c] = unerf_sigmoid(mf_half_dot(a.p.ws_rgb + c * 64, h, x0, x1) + a.p.ws_rgb[192 + c]);
            if (valid) {
                mf_store_units(a.aux2, n, 0, h, x0);
                mf_store_units(a.aux2, n, 1, h, x1);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float c1s, c2s;
                mf_lap_head<true>(lap_set_blob(a, a.p.lap_blob, tile, div_s), 1 + c, lane, h, x0, x1, c1s, c2s);
                mu_c[c] = c1s * inv_nr;
                vsum += fmaxf(c2s * inv_nr - mu_c[c] * mu_c[c], 0.f);
            }
        }
        if (valid && h == 0) {
            a.density[n] = mu_d;
            if (!CAPTURE) {
                a.aux[n] = mu2_d - mu_d * mu_d;
                a.aux2[n] = vsum / 3.f;
            }
            a.rgb[n * 3 + 0] = mu_c[0];
            a.rgb[n * 3 + 1] = mu_c[1];
            a.rgb[n * 3 + 2] = mu_c[2];
        }
    }
}

// --------------------------------------------------------------------------------------
// 5b-3. Split-f16 variant of the LAPLACE kernel (inference): base network as in field_kernel_mfma16, the 4 x 128
// sampled last-layer rows as 16 (head, block) groups of 4 k-steps x 3 products = 12 MFMAs (instead of 32),
// operands streamed from L2 as 16-byte quads (ops.pack_laplace_heads16), one block prefetched ahead.  With the
// matrix work cut 5x the exp / rcp epilogues (quarter-rate transcendentals) are the larger half, so register
// quads that only hold padding rows (rows >= n_lap) are skipped.
// --------------------------------------------------------------------------------------
// ACT: 0 exp, 1 sigmoid, 2 softplus.  The rows of lap16_blob carry the base change (ops.pack_laplace_heads16: density
// rows x log2 e, colour rows x -log2 e; unerf_build_flags() tells the host), so exp / sigmoid are the bare v_exp_f32
// (+ v_rcp_f32); softplus rows are unscaled.
// The fences keep each row block's MFMAs in front of its activations, as separate scheduling regions (they cost nothing:
// docs/experiments.md 6.4).
#define LAP_FENCE() __builtin_amdgcn_sched_barrier(0)
template <int ACT, bool F1 = false>
__device__ __forceinline__ void mf16_lap_head(const float* __restrict__ lap, int q, int n_lap, int lane,
                                              const f16x8 (&bhi)[4], const f16x8 (&blo)[4], int h, float& sum1,
                                              float& sum2) {
    unerf_v2f s12 = {0.f, 0.f};
    f16x8 cur[8], nxt[8];
    {
        const float* f = lap + (size_t)((q * LAP_BLOCKS + 0) * 8) * 256 + lane * 4;
#pragma unroll
        for (int i = 0; i < 8; i += (F1 ? 2 : 1)) cur[i] = *reinterpret_cast<const f16x8*>(f + i * 256);   // F1: hi quads only
    }
#pragma unroll
    for (int b = 0; b < LAP_BLOCKS; ++b) {
        if (b + 1 < LAP_BLOCKS) {
            const float* f = lap + (size_t)((q * LAP_BLOCKS + b + 1) * 8) * 256 + lane * 4;
#pragma unroll
            for (int i = 0; i < 8; i += (F1 ? 2 : 1)) nxt[i] = *reinterpret_cast<const f16x8*>(f + i * 256);
        }
        const float4* bp = reinterpret_cast<const float4*>(lap + LAP_BIAS_OFF + ((q * LAP_BLOCKS + b) * 2 + h) * 16);
        float4 b0 = bp[0], b1 = bp[1], b2 = bp[2], b3 = bp[3];
        f32x16 acc = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w, b3.x, b3.y, b3.z, b3.w};
        LAP_FENCE();
#pragma unroll
        for (int st = 0; st < 4; ++st) {  // cur[2 st] = hi, cur[2 st + 1] = lo of k-step st
            if (!F1) {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[2 * st + 1], bhi[st], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[2 * st], blo[st], acc, 0, 0, 0);
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[2 * st], bhi[st], acc, 0, 0, 0);
        }
        // register quad qd holds rows 8 qd + 4 h + (0..3) of this block: skip quads that are padding in both halves
        const int rows = n_lap - 32 * b;
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            if (8 * qd < rows) {  // uniform
#pragma unroll
                for (int r = 4 * qd; r < 4 * qd + 4; ++r) {
                    float p;
                    if (ACT == 2) {
                        p = mf_softplus_fast(acc[r]);
                    } else {
                        const float e = __builtin_amdgcn_exp2f(acc[r]);
                        p = ACT == 1 ? __builtin_amdgcn_rcpf(1.f + e) : e;
                    }
                    // the sums of p and p^2 as one add and one fma on their own registers, not one packed fma (the same
                    // roundings as its two halves).  A packed-fp32 instruction cannot run beside an MFMA -- one behind an MFMA
                    // waits for it and costs 18 cycles, the next MFMA waits for the packed instruction in turn
                    // (benchmarks/issue_sweep_probe.hip) -- and at two or three waves per SIMD the other wave's head MFMAs
                    // are always in flight; v_add_f32 / v_fmac_f32 issue in their shadow.
                    s12.x += p;
                    s12.y = __builtin_fmaf(p, p, s12.y);
                }
            }
        }
        LAP_FENCE();
        if (b + 1 < LAP_BLOCKS) {
#pragma unroll
            for (int i = 0; i < 8; i += (F1 ? 2 : 1)) cur[i] = nxt[i];
        }
    }
    sum1 = s12.x + __shfl_xor(s12.x, 32, 64);
    sum2 = s12.y + __shfl_xor(s12.y, 32, 64);
}

// The same head evaluation as ONE operand stream over NHEADS consecutive heads with the loads
// running TWO row blocks ahead of the matrix work (three rotating register buffers instead of two).  The kernel was
// latency-bound on exactly this stream -- 8 KB per wave and block from L2, one block (~0.9 us of two waves' work) of
// lead against ~1.4 us of loaded L2 latency: issue-busy 0.575, SQ_WAIT_ANY 0.34 (profiles/issue_laplace.json, round
// 3) -- and every head started cold; the three colour heads now run as one 12-block stream.
// lds_bias: the 512 bias words of the sample set, staged in LDS per wave and tile (see the kernel).
template <int ACT, bool F1, int NHEADS>
__device__ __forceinline__ void mf16_lap_stream(const float* __restrict__ lap, const float* __restrict__ lds_bias, int q0,
                                                int n_lap, int lane, const f16x8 (&bhi)[4], const f16x8 (&blo)[4], int h,
                                                float (&sum1)[NHEADS], float (&sum2)[NHEADS]) {
    constexpr int NB = NHEADS * LAP_BLOCKS;
    f16x8 buf[3][8];
    const float* base = lap + (size_t)(q0 * LAP_BLOCKS * 8) * 256 + lane * 4;
#pragma unroll
    for (int i = 0; i < 8; i += (F1 ? 2 : 1)) buf[0][i] = *reinterpret_cast<const f16x8*>(base + i * 256);
    if (NB > 1) {
#pragma unroll
        for (int i = 0; i < 8; i += (F1 ? 2 : 1)) buf[1][i] = *reinterpret_cast<const f16x8*>(base + (8 + i) * 256);
    }
    unerf_v2f s12 = {0.f, 0.f};
#pragma unroll
    for (int blk = 0; blk < NB; ++blk) {
        const int b = blk % LAP_BLOCKS, hd = blk / LAP_BLOCKS;
        if (blk + 2 < NB) {
#pragma unroll
            for (int i = 0; i < 8; i += (F1 ? 2 : 1))
                buf[(blk + 2) % 3][i] = *reinterpret_cast<const f16x8*>(base + ((blk + 2) * 8 + i) * 256);
        }
        const f16x8 (&cur)[8] = buf[blk % 3];
        const float4* bp = reinterpret_cast<const float4*>(lds_bias + (((q0 + hd) * LAP_BLOCKS + b) * 2 + h) * 16);
        float4 b0 = bp[0], b1 = bp[1], b2 = bp[2], b3 = bp[3];
        f32x16 acc = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w, b3.x, b3.y, b3.z, b3.w};
        if (b == 0) s12 = unerf_v2f{0.f, 0.f};
        LAP_FENCE();
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            if (!F1) {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[2 * st + 1], bhi[st], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[2 * st], blo[st], acc, 0, 0, 0);
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[2 * st], bhi[st], acc, 0, 0, 0);
        }
        const int rows = n_lap - 32 * b;
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            if (8 * qd < rows) {  // uniform
#pragma unroll
                for (int r = 4 * qd; r < 4 * qd + 4; ++r) {
                    float p;
                    if (ACT == 2) {
                        p = mf_softplus_fast(acc[r]);
                    } else {
                        const float e = __builtin_amdgcn_exp2f(acc[r]);
                        p = ACT == 1 ? __builtin_amdgcn_rcpf(1.f + e) : e;
                    }
                    // (scalar moment sums: see mf16_lap_head)
                    s12.x += p;
                    s12.y = __builtin_fmaf(p, p, s12.y);
                }
            }
        }
        LAP_FENCE();
        if (b == LAP_BLOCKS - 1) {
            sum1[hd] = s12.x + __shfl_xor(s12.x, 32, 64);
            sum2[hd] = s12.y + __shfl_xor(s12.y, 32, 64);
        }
    }
}

#define UNERF_LAP16_KERNEL field_kernel_mfma16_laplace
#define UNERF_LAP16_VIEWS false
#include "unerf_field_lap16.inc"
#undef UNERF_LAP16_KERNEL
#undef UNERF_LAP16_VIEWS
// the same kernel under the name its several-views instantiations carry (unerf_field_fwd_laplace_views)
#define UNERF_LAP16_KERNEL views_laplace_kernel_mfma16
#define UNERF_LAP16_VIEWS true
#include "unerf_field_lap16.inc"
#undef UNERF_LAP16_KERNEL
#undef UNERF_LAP16_VIEWS

// --------------------------------------------------------------------------------------
// 5c. level-major hash-grid gather.  One level of the main grid is 2^19 x 8 B = 4 MiB -- exactly
// one XCD's L2.  Sample-major lookup (all 16 levels per sample) keeps 64 MiB live and runs at the
// Infinity-Cache random-64-B-request rate (40 ms/frame inside the fused kernel, 5.05 ms per 2^18
// rays stand-alone); walking the levels in the SLOW grid dimension makes every XCD sweep one
// 4-MiB table at a time out of its own L2: 2.3 ms per 2^18 rays (benchmarks/exp_level_major.py).
// Features go to level-major planes [16][N] float2 (coalesced 8-B stores here, coalesced 8-B
// loads in field_kernel_mfma<.., FEAT_IN>), and the gather runs on its own stream underneath the
// previous launch group's matrix work (render.py).
// --------------------------------------------------------------------------------------
struct GatherArgs {
    const float* origins;
    const float* dirs;
    const float* sbins;
    int64_t R;
    int S;
    float s_near, s_far;
    int lin;   // UNERF_SPACING_*: 1 = identity spacing (UniformSampler)
    const float* table;
    const float* scalings;
    int L, log2T;
    float* planes;
    unerf_norm_box box;   // contraction path only (unerf_field_gather has no aabb argument)
};

__global__ __launch_bounds__(256) void field_gather_kernel(GatherArgs a) {
    const int64_t N = a.R * (int64_t)a.S;
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int lev = blockIdx.y;
    const int64_t r = n / a.S;
    const int s = (int)(n - r * a.S);
    const float* sb = a.sbins + r * (a.S + 1);
    float e0 = unerf_s2e(sb[s], a.s_near, a.s_far, a.lin), e1 = unerf_s2e(sb[s + 1], a.s_near, a.s_far, a.lin);
    float t01 = e0 + e1;
    float px = a.origins[r * 3 + 0] + a.dirs[r * 3 + 0] * t01 / 2.f;
    float py = a.origins[r * 3 + 1] + a.dirs[r * 3 + 1] * t01 / 2.f;
    float pz = a.origins[r * 3 + 2] + a.dirs[r * 3 + 2] * t01 / 2.f;
    (void)unerf_normalize_position(px, py, pz, a.box);
    const float2* lvl = reinterpret_cast<const float2*>(a.table) + ((size_t)lev << a.log2T);
    float2 f = unerf_hash_level(lvl, px, py, pz, a.scalings[lev], (1u << a.log2T) - 1u);
    reinterpret_cast<float2*>(a.planes)[(int64_t)lev * N + n] = f;
}

extern "C" int unerf_field_gather(const float* origins, const float* directions, const float* sbins, int64_t R, int S,
                                  float near_plane, float far_plane, int spacing, const float* table, const float* scalings, int L,
                                  int log2T, float* feature_planes, void* stream) {
    UNERF_REQUIRE(table && scalings && (R == 0 || (origins && directions && sbins && feature_planes)), "field_gather: null pointer");
    UNERF_REQUIRE(L >= 1 && L <= 32 && log2T >= 1 && log2T <= 24 && R >= 0 && S >= 1, "field_gather: bad L/log2T/R/S");
    if (R == 0) return UNERF_OK;
    GatherArgs a;
    a.origins = origins; a.dirs = directions; a.sbins = sbins; a.R = R; a.S = S;
    if (int rc = set_spacing(a, near_plane, far_plane, spacing)) return rc;
    a.table = table; a.scalings = scalings; a.L = L; a.log2T = log2T; a.planes = feature_planes;
    a.box = make_norm_box(0, nullptr);
    // blockIdx.x runs fastest in dispatch order, so all workgroups of level l are issued before
    // level l+1: the chip works on (at most) two adjacent level tables at any time
    dim3 grid(blocks_for(R * (int64_t)S, 256), L), block(256);
    hipLaunchKernelGGL(field_gather_kernel, grid, block, 0, (hipStream_t)stream, a);
    return unerf_check_launch("field_gather");
}

// Persistent grid of the matrix kernels: exactly as many workgroups as are co-resident (occupancy x CUs, a
// multiple of the 8 XCDs).  The ACTIVE kernels fit 3 per CU (42.6 KB LDS, <= 168 VGPRs), the K-pass and Laplace
// kernels 2; launching 3 per CU for those left a third of the tiles to a half-empty second round.
template <typename Kern>
static int mfma_grid_for(Kern kernel, int64_t num_tiles, size_t lds_bytes) {
    static std::mutex mu;
    static std::unordered_map<const void*, int> cache;
    int cap = 0;
    {
        std::lock_guard<std::mutex> lock(mu);
        auto it = cache.find(reinterpret_cast<const void*>(kernel));
        if (it != cache.end()) cap = it->second;
    }
    if (cap == 0) {
        int per_cu = 0, dev = 0, cus = 256;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, lds_bytes) != hipSuccess || per_cu < 1)
            per_cu = 2;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        (void)hipGetLastError();
        cap = per_cu * cus;
        if (getenv("UNERF_DEBUG_GRID")) fprintf(stderr, "[unerf] persistent grid: %d workgroups/CU x %d CUs\n", per_cu, cus);
        std::lock_guard<std::mutex> lock(mu);
        cache[reinterpret_cast<const void*>(kernel)] = cap;
    }
    int64_t blocks = (num_tiles + 3) / 4;
    if (blocks > cap) blocks = cap;
    return (int)((blocks + 7) / 8 * 8);
}
// one persistent matrix-kernel launch: tile map from the image_width hint, LDS = the operand blob
template <typename Kern, typename... Extra>   // extra: the KeepArgs of the explicit-mask kernels
static void launch_matrix_kernel(Kern kernel, size_t lds_bytes, FieldArgs& a, hipStream_t st, Extra... extra) {
    const int64_t tiles = make_tiles(a, a.p.image_width);
    hipLaunchKernelGGL(kernel, dim3(mfma_grid_for(kernel, tiles, lds_bytes)), dim3(256), lds_bytes, st, a, (uint32_t)tiles,
                       make_fastdiv((uint32_t)a.S), extra...);
}
// Dynamic LDS of a matrix kernel: the fp32-sized operand blob, except that field_kernel_mfma16 gets the "f16" blob
// (+ the colour-2 slabs) when F1 or DROP (explicit masks are a DROP form).
constexpr size_t MF_LDS_BYTES = (size_t)UNERF_MFMA_BLOB_FLOATS * 4;
// only the F1 kernels stage the larger blob; DROP is in the rule because these launches always had this byte count (it sizes the persistent grid)
constexpr size_t mf16_lds_bytes(bool F1, bool DROP) { return (F1 || DROP) ? (size_t)UNERF_MFMA16_BLOB_FLOATS * 4 : MF_LDS_BYTES; }

// --------------------------------------------------------------------------------------
// 5h. Host side of the field kernels (5, 5a', 5b*): check the arguments, fill FieldArgs, select and launch.
// The kernel selection is field_launch() with the launch_* helpers above it, and nothing else (as a table: DESIGN.md 6,
// "Which field kernel a call runs").
// --------------------------------------------------------------------------------------
// (with_int3 / with_bool: "kernel selection" in the host plumbing at the top of the file)
// the TCNN template argument: 0 = torch-layout grid, 1 = tcnn layout, 2 = tcnn layout with half2 rows (grid_half)
static int tcnn_arg(const unerf_field_params& p) { return p.tcnn_levels ? (p.grid_half ? 2 : 1) : 0; }

// field_kernel_mfma16<MODE, tc, SITES, DROP, f1, XA...>: every grid layout and both colour-layer forms of one (MODE, SITES, DROP)
template <int MODE, bool SITES, bool DROP, typename... XA>
static void launch_mfma16(FieldArgs& a, hipStream_t st, XA... xa) {
    with_int3(tcnn_arg(a.p), [&](auto tc) {
        with_bool(a.p.f16_single != 0, [&](auto f1) {
            constexpr bool F1 = decltype(f1)::value;
            launch_matrix_kernel(field_kernel_mfma16<MODE, decltype(tc)::value, SITES, DROP, F1, XA...>, mf16_lds_bytes(F1, DROP), a, st, xa...);
        });
    });
}
// field_kernel_mfma<MODE, FEAT_IN, tc, XA...>: pre-gathered features come from the torch-layout grid only (checked), so
// FEAT_IN exists with tc = 0 alone
template <int MODE, typename... XA>
static void launch_mfma(FieldArgs& a, hipStream_t st, XA... xa) {
    if (a.features) return launch_matrix_kernel(field_kernel_mfma<MODE, true, 0, XA...>, MF_LDS_BYTES, a, st, xa...);
    with_int3(tcnn_arg(a.p), [&](auto tc) {
        launch_matrix_kernel(field_kernel_mfma<MODE, false, decltype(tc)::value, XA...>, MF_LDS_BYTES, a, st, xa...);
    });
}
// field_kernel<MODE, XA...> (VALU, one wave per 64 samples); the K passes keep a second activation buffer in LDS
template <int MODE, typename... XA>
static void launch_valu(FieldArgs& a, hipStream_t st, XA... xa) {
    constexpr size_t lds_bytes = (MODE == UNERF_FIELD_MCDROPOUT ? 2 : 1) * 64 * 64 * 4;
    hipLaunchKernelGGL((field_kernel<MODE, XA...>), dim3(blocks_for(a.R * (int64_t)a.S, 64)), dim3(64), lds_bytes, st, a, xa...);
}
// ACTIVE / MCDROPOUT: the family follows the operand blobs the caller packed -- split-f16 MFMA, else fp32 MFMA (the one
// that reads pre-gathered features), else VALU.  (SITES, DROP) only reaches field_kernel_mfma16.
template <int MODE, bool SITES, bool DROP, typename... XA>
static void launch_by_blob(FieldArgs& a, hipStream_t st, XA... xa) {
    if (a.p.mfma16_blob && !a.features) launch_mfma16<MODE, SITES, DROP, XA...>(a, st, xa...);
    else if (a.p.mfma_blob) launch_mfma<MODE, XA...>(a, st, xa...);
    else launch_valu<MODE, XA...>(a, st, xa...);
}

constexpr int DROP_SITES_KNOWN = UNERF_DROP_TRUNK | UNERF_DROP_HEAD0 | UNERF_DROP_HEAD1 | UNERF_DROP_HEADIN;
constexpr int DROP_SITES_DEFAULT = UNERF_DROP_TRUNK | UNERF_DROP_HEAD1;   // the reference's Dropout placement
// the site set a call asks for; FieldArgs.drop_sites is this set while masks are applied and 0 otherwise
static int requested_drop_sites(const unerf_field_params& p) { return p.drop_sites ? p.drop_sites : DROP_SITES_DEFAULT; }

// Widths left 0 are nerfacto's (only field_kernel_generic reads them).  True: the any-width slow path, widths given and
// different from nerfacto's 64 / 64 / 15 / 2 (or L != 16)
static bool field_set_widths(unerf_field_params& p) {
    if (!p.hidden) p.hidden = 64;
    if (!p.hidden_color) p.hidden_color = 64;
    if (!p.geo_dim) p.geo_dim = 15;
    if (!p.feat_per_level) p.feat_per_level = 2;
    if (!p.app_dim) p.app_dim = 32;
    const bool headin_site = p.mode == UNERF_FIELD_MCDROPOUT && (p.drop_sites & UNERF_DROP_HEADIN);
    return p.hidden != 64 || p.hidden_color != 64 || p.geo_dim != 15 || p.feat_per_level != 2 || p.L != 16 || (p.app_dim != 32 && headin_site);
}
// LDS rows of the any-width kernel: the widest activation (widths range-checked before); 64 lanes x 4 buffers x 4 bytes per row
static int generic_rows(const unerf_field_params& p) {
    int rows = p.L * p.feat_per_level;
    for (int v : {p.hidden, p.hidden_color, 16 + p.geo_dim + p.app_dim, 1 + p.geo_dim + 1}) rows = v > rows ? v : rows;
    return rows;
}
static size_t generic_lds_bytes(int rows) { return (size_t)rows * 64 * 4 * 4; }

// Job 1a, every call (a: the call's arguments as given): what is refused even when R == 0.
static int field_check_args(const FieldArgs& a, float near_plane, bool generic, const unerf_keep_masks* masks) {
    const unerf_field_params& p = a.p;
    const float* features = a.features;
    UNERF_REQUIRE(!p.packed_out || (p.mode != UNERF_FIELD_LAPLACE && !p.sample_major),
                  "field_fwd: packed_out rows are written by the ACTIVE / MCDROPOUT kernels in the ray-major layout only");
    UNERF_REQUIRE(p.table && (p.scalings || p.tcnn_levels) && p.w0t && p.b0 && p.w1t && p.b1 && p.h0t &&
                      p.hb0 && p.h1t && p.hb1 && p.h2t && p.hb2,
                  "field_fwd: null weight pointer");
    UNERF_REQUIRE(generic || p.L == 16, "field_fwd: L=%d", p.L);
    if (generic) {
        UNERF_REQUIRE(p.L >= 1 && p.L <= 32 && (p.feat_per_level == 2 || p.feat_per_level == 4) && p.hidden >= 1 && p.hidden <= 256 &&
                          p.hidden_color >= 1 && p.hidden_color <= 256 && p.geo_dim >= 0 && p.geo_dim <= 64,
                      "field_fwd: widths outside the any-width kernel's range (L=%d F=%d hidden=%d hidden_color=%d geo=%d)", p.L,
                      p.feat_per_level, p.hidden, p.hidden_color, p.geo_dim);
        UNERF_REQUIRE(p.feat_per_level == 2 || !p.tcnn_levels, "field_fwd: features_per_level = 4 is built for the torch-layout grid");
        UNERF_REQUIRE(!features && !p.sample_major && !p.packed_out, "field_fwd: the any-width kernel writes the plain ray-major layout only");
        UNERF_REQUIRE(p.mode != UNERF_FIELD_MCDROPOUT || (p.hidden <= 128 && p.hidden_color <= 128 &&
                                                          (!(p.drop_sites & UNERF_DROP_HEADIN) || 16 + p.geo_dim + p.app_dim <= 128)),
                      "field_fwd: a dropout site has at most 128 units (mask stream layout)");
    }
    UNERF_REQUIRE(!features || (p.mfma_blob && p.mode != UNERF_FIELD_LAPLACE),
                  "field_fwd: pre-gathered features are consumed by the MFMA kernel only (ACTIVE/MCDROPOUT with mfma_blob)");
    UNERF_REQUIRE(p.tcnn_levels || (p.log2T >= 1 && p.log2T <= 24), "field_fwd: bad log2T=%d", p.log2T);
    UNERF_REQUIRE(!(p.tcnn_levels && features), "field_fwd: pre-gathered feature planes are built for the torch-layout grid only");
    UNERF_REQUIRE(!p.grid_half || p.tcnn_levels, "field_fwd: grid_half (half2 rows, tcnn's half arithmetic) needs a tcnn-layout grid");
    UNERF_REQUIRE(a.R >= 0 && a.S >= 1, "field_fwd: bad R/S");
    UNERF_REQUIRE(!(near_plane < 0.f && features), "field_fwd: Euclidean bins (near_plane < 0) cannot be combined with pre-gathered features");
    UNERF_REQUIRE((uint64_t)(a.ray_offset + a.R) * (uint64_t)a.S < (1ull << 32),
                  "field_fwd: sample index exceeds 32 bits (RNG counter)");
    UNERF_REQUIRE(!p.sample_major || (p.mode != UNERF_FIELD_LAPLACE && (p.mfma16_blob || p.mfma_blob)),
                  "field_fwd: sample_major planes are written by the ACTIVE / MCDROPOUT matrix kernels only");
    if (p.mode == UNERF_FIELD_MCDROPOUT) {   // with or without explicit masks
        UNERF_REQUIRE(p.K >= 0 && p.p_drop >= 0.f && p.p_drop < 1.f, "field_fwd MCDROPOUT: bad K/p_drop");
        // (the any-width kernel tests the four known bits and has always let others through)
        UNERF_REQUIRE(generic || (p.drop_sites & ~DROP_SITES_KNOWN) == 0, "field_fwd MCDROPOUT: unknown bits in drop_sites=%d", p.drop_sites);
    }
    if (masks) {   // explicit keep masks: every refusal before any launch; never a fall-back to the generator
        UNERF_REQUIRE(p.mode == UNERF_FIELD_MCDROPOUT, "field_fwd_masked: explicit keep masks are an MCDROPOUT mode (mode=%d)", p.mode);
        UNERF_REQUIRE(p.K > 0, "field_fwd_masked: K=%d, explicit keep masks need K >= 1 passes", p.K);
        UNERF_REQUIRE(!(p.drop_sites & UNERF_DROP_HEADIN),
                      "field_fwd_masked: UNERF_DROP_HEADIN is out of scope of the explicit-mask mode (not built; no generator fall-back)");
        UNERF_REQUIRE(!generic, "field_fwd_masked: the any-width kernel is out of scope of the explicit-mask mode "
                                "(nerfacto widths 64 / 64 / 15 / 2 and L = 16 only; no generator fall-back)");
        const int sites = requested_drop_sites(p);
        static const char* const names[4] = {"TRUNK", "HEAD0", "HEAD1", "HEADIN"};
        for (int i = 0; i < 4; ++i) {
            UNERF_REQUIRE(!((sites >> i) & 1) || masks->site[i], "field_fwd_masked: site %s is active (drop_sites=%d) but its mask array is NULL", names[i], sites);
            UNERF_REQUIRE(((sites >> i) & 1) || !masks->site[i], "field_fwd_masked: a mask array for site %s, which is not active (drop_sites=%d)", names[i], sites);
        }
        UNERF_REQUIRE(masks->sample_offset >= 0 && masks->pass_stride >= masks->sample_offset + a.R * (int64_t)a.S,
                      "field_fwd_masked: pass_stride=%lld < sample_offset + R*S = %lld + %lld", (long long)masks->pass_stride,
                      (long long)masks->sample_offset, (long long)(a.R * (int64_t)a.S));
    }
    return UNERF_OK;
}

// Job 2: the derived fields of FieldArgs (nothing here can fail).
static void field_fill_args(FieldArgs& a, float near_plane, float far_plane, int spacing, const unerf_keep_masks* masks) {
    a.lin = spacing;
    a.s_near = near_plane < 0.f ? -1.f : unerf_spacing_of(near_plane, spacing);   // < 0: sbins are Euclidean edges
    a.s_far = unerf_spacing_of(far_plane, spacing);
    if (a.p.n_lap_rgb <= 0) a.p.n_lap_rgb = a.p.n_lap;
    a.div_chunk = make_fastdiv(a.p.lap_chunk_rays > 0 ? (uint32_t)a.p.lap_chunk_rays : 1u);
    a.chunk0 = (uint32_t)a.ray_offset;
    if (a.p.mode == UNERF_FIELD_LAPLACE && a.p.lap_chunk_rays != 0) a.p.image_width = 0;   // per-chunk sample sets: 1-D tiles that never straddle two sets
    a.box = make_norm_box(a.p.use_aabb, a.p.aabb);
    if (masks) {   // the words are made of the keep bits (xm_word): on at every p, and any threshold in (-32768, 32767] reads them
        a.drop_on = 1;
        a.keep_hi = 0;
        a.keep_pk = 0u;
    } else {   // keep iff (signed 16-bit half) < thr_s = round((1-p) 65536) - 32768; p = 0 keeps everything (no masks)
        const long thr = lrint((1.0 - (double)a.p.p_drop) * 65536.0);
        const bool passes = a.p.mode == UNERF_FIELD_MCDROPOUT && a.p.K > 0;
        a.drop_on = (passes && thr < 65536) ? 1 : 0;
        const int32_t thr_s = (int32_t)(thr < 65536 ? thr : 65535) - 32768;
        a.keep_hi = (int32_t)((uint32_t)thr_s << 16);
        a.keep_pk = ((uint32_t)thr_s & 0xFFFFu) * 0x10001u;
        // 0 < p <= 2^-17: the threshold keeps every unit, and the Dropout modules still scale by 1 / (1 - p) -- the ONE rule for
        // the scale is "K > 0", on both sides: ops.pack_field_mfma16 folds it into the f16 operand blob whenever K > 0, so the f16
        // kernels run without masks here; the kernels that scale at run time (fp32 matrix, VALU, any-width) take the mask path
        // with the keep-every-unit bit (field_keep_all).  UNERF_DROP_HEADIN is served by the VALU kernel whatever the blobs.
        const bool f16_blob = a.p.mfma16_blob && !a.features && !(requested_drop_sites(a.p) & UNERF_DROP_HEADIN);
        if (passes && thr >= 65536 && a.p.p_drop > 0.f && !f16_blob) {
            a.drop_on = 1;
            a.keep_hi |= 1;
        }
    }
    a.drop_sites = a.drop_on ? requested_drop_sites(a.p) : 0;
    a.drop_scale = 1.f / (1.f - a.p.p_drop);
}

// Job 1b, non-empty calls only (a: filled): what an empty call has never been refused for.
static int field_check_nonempty(const FieldArgs& a, int spacing, bool generic) {
    const unerf_field_params& p = a.p;
    UNERF_REQUIRE_SPACING(spacing);
    UNERF_REQUIRE(!(a.features && p.use_aabb), "field_fwd: pre-gathered feature planes are built for the contraction path only");
    UNERF_REQUIRE(!p.f16_single || (p.mfma16_blob && !a.features && (p.mode != UNERF_FIELD_LAPLACE || (p.lap16_blob && p.n_lap <= 32 * LAP_BLOCKS))),
                  "field_fwd: f16_single needs mfma16_blob (and lap16_blob with n_lap <= 128 for LAPLACE), without pre-gathered features");
    if (generic) {
        const size_t lds_bytes = generic_lds_bytes(generic_rows(p));
        UNERF_REQUIRE(lds_bytes <= 160 * 1024, "field_fwd: %zu bytes of LDS for the any-width kernel", lds_bytes);
        const int want1 = p.geo_dim + (p.mode == UNERF_FIELD_ACTIVE ? 2 : (p.mode == UNERF_FIELD_MCDROPOUT ? 1 : 0));
        UNERF_REQUIRE(p.out1 == want1, "field_fwd: out1=%d, expected %d for geo_dim=%d in this mode", p.out1, want1, p.geo_dim);
    }
    switch (p.mode) {
        case UNERF_FIELD_ACTIVE:
            if (generic) UNERF_REQUIRE(a.aux, "field_fwd ACTIVE: aux (beta) must be non-null");
            else UNERF_REQUIRE(p.out1 == 17 && a.aux, "field_fwd ACTIVE: out1 must be 17 and aux (beta) non-null");
            break;
        case UNERF_FIELD_MCDROPOUT:
            UNERF_REQUIRE(generic || p.out1 == 16, "field_fwd MCDROPOUT: out1 must be 16");
            if (a.drop_sites & UNERF_DROP_HEADIN) {   // dropout on the head's inputs (include/unerf.h)
                UNERF_REQUIRE(p.h0_full_t && p.hb0_raw && p.app_embed,
                              "field_fwd MCDROPOUT: UNERF_DROP_HEADIN needs h0_full_t / hb0_raw / app_embed");
                UNERF_REQUIRE(!a.features && !p.sample_major,
                              "field_fwd MCDROPOUT: UNERF_DROP_HEADIN has no feature-plane / sample-major form");
            }
            break;
        case UNERF_FIELD_LAPLACE:
            if (generic) {
                UNERF_REQUIRE(a.aux && a.aux2 && p.ws_density && p.ws_rgb && p.n_lap >= 1, "field_fwd LAPLACE: need aux, aux2, ws_density, ws_rgb, n_lap>=1");
            } else {
                UNERF_REQUIRE(p.out1 == 15 && a.aux && a.aux2 && p.ws_density && p.ws_rgb && p.n_lap >= 1,
                              "field_fwd LAPLACE: need out1=15, aux, aux2, ws_density, ws_rgb, n_lap>=1");
                UNERF_REQUIRE(!(p.lap_blob || p.lap16_blob) || p.n_lap_rgb <= 32 * LAP_BLOCKS || p.n_lap > 32 * LAP_BLOCKS,
                              "field_fwd LAPLACE: n_lap_rgb=%d rows do not fit the head blobs (at most %d); pass them as ws_* only",
                              p.n_lap_rgb, 32 * LAP_BLOCKS);
                UNERF_REQUIRE(p.lap_chunk_rays == 0 || (p.lap_chunk_rays > 0 && p.lap_chunk_rays % 32 == 0 && a.ray_offset % 32 == 0 && p.lap_sets >= 1),
                              "field_fwd LAPLACE: lap_chunk_rays=%d and ray_offset=%lld must be multiples of 32, lap_sets=%d >= 1",
                              p.lap_chunk_rays, (long long)a.ray_offset, p.lap_sets);
            }
            UNERF_REQUIRE(p.lap_chunk_rays == 0 || (a.ray_offset + a.R - 1) / p.lap_chunk_rays < p.lap_sets,
                          "field_fwd LAPLACE: rays [%lld, +%lld) reach past the %d sample sets of %d rays",
                          (long long)a.ray_offset, (long long)a.R, p.lap_sets, p.lap_chunk_rays);
            break;
        default:
            unerf_set_error("field_fwd: unknown mode %d", p.mode);
            return UNERF_ERR_ARG;
    }
    return UNERF_OK;
}

// Job 3: run-time values -> template arguments -> launch, each kernel family in one launch expression.
static void field_launch(FieldArgs& a, bool generic, const unerf_keep_masks* masks, hipStream_t st) {
    const unerf_field_params& p = a.p;
    if (generic) {
        const int rows = generic_rows(p);
        const size_t lds_bytes = generic_lds_bytes(rows);
        with_int3(p.mode, [&](auto mode) {
            const auto kernel = field_kernel_generic<decltype(mode)::value>;
            if (lds_bytes > 64 * 1024)
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
            hipLaunchKernelGGL(kernel, dim3(blocks_for(a.R * (int64_t)a.S, 64)), dim3(64), lds_bytes, st, a, rows);
        });
        return;
    }
    switch (p.mode) {
        case UNERF_FIELD_ACTIVE:
            launch_by_blob<UNERF_FIELD_ACTIVE, false, false>(a, st);
            break;
        case UNERF_FIELD_MCDROPOUT:   // three (SITES, DROP) forms; explicit masks: the general form + the KeepArgs pack
            if (masks)
                launch_by_blob<UNERF_FIELD_MCDROPOUT, true, true>(a, st, KeepArgs{{masks->site[0], masks->site[1], masks->site[2]}, masks->pass_stride, masks->sample_offset});
            else if (a.drop_sites & UNERF_DROP_HEADIN) launch_valu<UNERF_FIELD_MCDROPOUT>(a, st);   // no matrix kernel has this site
            else if (!a.drop_on) launch_by_blob<UNERF_FIELD_MCDROPOUT, false, false>(a, st);       // K = 0 or p_drop = 0: no masks
            else if (a.drop_sites == DROP_SITES_DEFAULT) launch_by_blob<UNERF_FIELD_MCDROPOUT, false, true>(a, st);
            else launch_by_blob<UNERF_FIELD_MCDROPOUT, true, true>(a, st);
            break;
        case UNERF_FIELD_LAPLACE: {
            const bool heads_fit = p.n_lap <= 32 * LAP_BLOCKS;   // the sample sets as head blobs
            if (p.mfma16_blob && p.lap16_blob && heads_fit) {
                with_int3(tcnn_arg(p), [&](auto tc) {
                    with_bool(p.f16_single != 0, [&](auto f1) {
                        launch_matrix_kernel(field_kernel_mfma16_laplace<decltype(tc)::value, decltype(f1)::value>, MF_LDS_BYTES, a, st);
                    });
                });
            } else if (p.mfma_blob && p.lap_blob && heads_fit) {
                with_int3(tcnn_arg(p), [&](auto tc) { launch_matrix_kernel(field_kernel_mfma_laplace<false, decltype(tc)::value>, MF_LDS_BYTES, a, st); });
            } else {
                launch_valu<UNERF_FIELD_LAPLACE>(a, st);
            }
            break;
        }
    }
}

// masks = NULL: unerf_field_fwd.  Else unerf_field_fwd_masked: MC-dropout under explicit keep masks, the same checks, fill
// and selection (field_launch) with the KeepArgs pack appended to the launch.
static int field_fwd_impl(const float* origins, const float* directions, const float* sbins, int64_t R, int S,
                          float near_plane, float far_plane, int spacing, int64_t ray_offset, const unerf_field_params* p,
                          const float* features, float* density, float* rgb, float* aux, float* aux2,
                          const unerf_keep_masks* masks, void* stream) {
    UNERF_REQUIRE(p && (R == 0 || (origins && directions && sbins && (density || p->packed_out) && rgb)), "field_fwd: null pointer");
    FieldArgs a;
    a.origins = origins; a.dirs = directions; a.sbins = sbins; a.R = R; a.S = S; a.ray_offset = ray_offset;
    a.p = *p; a.density = density; a.rgb = rgb; a.aux = aux; a.aux2 = aux2; a.features = features;
    const bool generic = field_set_widths(a.p);
    if (int rc = field_check_args(a, near_plane, generic, masks)) return rc;
    if (R == 0) return UNERF_OK;
    field_fill_args(a, near_plane, far_plane, spacing, masks);
    if (int rc = field_check_nonempty(a, spacing, generic)) return rc;
    field_launch(a, generic, masks, (hipStream_t)stream);
    return unerf_check_launch(generic ? "field_fwd (any-width kernel)" : masks ? "field_fwd_masked" : "field_fwd");
}

extern "C" int unerf_field_fwd(const float* origins, const float* directions, const float* sbins, int64_t R, int S,
                               float near_plane, float far_plane, int spacing, int64_t ray_offset, const unerf_field_params* p,
                               const float* features, float* density, float* rgb, float* aux, float* aux2,
                               void* stream) {
    return field_fwd_impl(origins, directions, sbins, R, S, near_plane, far_plane, spacing, ray_offset, p, features, density, rgb,
                          aux, aux2, nullptr, stream);
}

extern "C" int unerf_field_fwd_masked(const float* origins, const float* directions, const float* sbins, int64_t R, int S,
                                      float near_plane, float far_plane, int spacing, int64_t ray_offset,
                                      const unerf_field_params* p, const float* features, float* density, float* rgb, float* aux,
                                      float* aux2, const unerf_keep_masks* masks, void* stream) {
    UNERF_REQUIRE(masks, "field_fwd_masked: null masks (unerf_field_fwd is the generator path)");
    return field_fwd_impl(origins, directions, sbins, R, S, near_plane, far_plane, spacing, ray_offset, p, features, density, rgb,
                          aux, aux2, masks, stream);
}

// Several views in one launch.  Only MCDROPOUT with generated masks reads a per-view value (counter + seed): that mode runs
// the FieldViews instantiations of field_kernel_mfma16; everything else this entry point accepts has none and goes through
// field_launch() with ray_offset = 0 (the tile map then works on the tall image of all views).
extern "C" int unerf_field_fwd_views(const float* origins, const float* directions, const float* sbins, int64_t R, int S,
                                     float near_plane, float far_plane, int spacing, const unerf_ray_views* views,
                                     const unerf_field_params* p, const float* features, float* density, float* rgb, float* aux,
                                     float* aux2, const unerf_keep_masks* masks, void* stream) {
    UNERF_REQUIRE(!masks, "field_fwd_views: explicit keep masks have no views form (unerf_field_fwd_masked renders one frame per call)");
    UNERF_REQUIRE(p, "field_fwd_views: null params");
    if (int rc = check_views(views, R, "field_fwd_views")) return rc;
    UNERF_REQUIRE(p->mode == UNERF_FIELD_ACTIVE || p->mode == UNERF_FIELD_MCDROPOUT,
                  "field_fwd_views: mode %d is not built for several views (ACTIVE / MCDROPOUT only; LAPLACE renders one frame per call here: unerf_field_fwd_laplace_views)", p->mode);
    UNERF_REQUIRE(p->mfma16_blob, "field_fwd_views: built for the f16 matrix kernels (mfma16_blob, precision f16x2 / f16); the exact-fp32 "
                                  "and VALU kernels render one frame per call");
    UNERF_REQUIRE(!features, "field_fwd_views: pre-gathered features are not built for several views");
    UNERF_REQUIRE(!p->sample_major, "field_fwd_views: sample_major planes are not built for several views");
    UNERF_REQUIRE(origins && directions && sbins && (density || p->packed_out) && rgb, "field_fwd_views: null pointer");
    FieldArgs a;
    a.origins = origins; a.dirs = directions; a.sbins = sbins; a.R = R; a.S = S; a.ray_offset = 0;
    a.p = *p; a.density = density; a.rgb = rgb; a.aux = aux; a.aux2 = aux2; a.features = nullptr;
    const bool generic = field_set_widths(a.p);
    UNERF_REQUIRE(!generic, "field_fwd_views: the any-width kernel is not built for several views (nerfacto widths 64 / 64 / 15 / 2, L = 16)");
    UNERF_REQUIRE(p->mode != UNERF_FIELD_MCDROPOUT || requested_drop_sites(a.p) == DROP_SITES_DEFAULT,
                  "field_fwd_views: drop_sites=%d is not built for several views (TRUNK | HEAD1 only)", p->drop_sites);
    if (int rc = field_check_args(a, near_plane, generic, nullptr)) return rc;
    field_fill_args(a, near_plane, far_plane, spacing, nullptr);
    if (int rc = field_check_nonempty(a, spacing, generic)) return rc;
    if (a.p.mode == UNERF_FIELD_MCDROPOUT && a.drop_on) {
        FieldViews fv;
        fv.div_hw = make_fastdiv((uint32_t)views->rays_per_view);
        fv.hw = (uint32_t)views->rays_per_view;
        for (int v = 0; v < UNERF_NERF_MAX_VIEWS; ++v) fv.key[v] = unerf_mc_key(views->seed[v < views->n_views ? v : 0], 0u);
        with_int3(tcnn_arg(a.p), [&](auto tc) {
            with_bool(a.p.f16_single != 0, [&](auto f1) {
                constexpr bool F1 = decltype(f1)::value;
                launch_matrix_kernel(views_kpass_kernel_mfma16<UNERF_FIELD_MCDROPOUT, decltype(tc)::value, false, true, F1, FieldViews>,
                                     mf16_lds_bytes(F1, true), a, (hipStream_t)stream, fv);
            });
        });
    } else {
        field_launch(a, generic, nullptr, (hipStream_t)stream);
    }
    return unerf_check_launch("field_fwd_views");
}

// LAPLACE over several views: views_laplace_kernel_mfma16 with the ray blocks laid out per view (LapViews) and every view's
// own run of sample sets.  Everything is refused before any launch; nothing falls back to another kernel.
extern "C" int unerf_field_fwd_laplace_views(const float* origins, const float* directions, const float* sbins, int64_t R, int S,
                                             float near_plane, float far_plane, int spacing, const unerf_ray_views* views,
                                             const unerf_laplace_views* lap_views, const unerf_field_params* p, float* density,
                                             float* rgb, float* aux, float* aux2, void* stream) {
    UNERF_REQUIRE(p, "field_fwd_laplace_views: null params");
    if (int rc = check_views(views, R, "field_fwd_laplace_views")) return rc;
    UNERF_REQUIRE(lap_views, "field_fwd_laplace_views: null lap_views (the sample-set base of every view)");
    UNERF_REQUIRE(p->mode == UNERF_FIELD_LAPLACE, "field_fwd_laplace_views: mode %d is not LAPLACE (ACTIVE / MCDROPOUT: unerf_field_fwd_views)", p->mode);
    UNERF_REQUIRE(p->mfma16_blob && p->lap16_blob, "field_fwd_laplace_views: built for the f16 matrix kernel (mfma16_blob and lap16_blob, precision "
                                                   "f16x2 / f16); the exact-fp32 and VALU kernels render one frame per call");
    FieldArgs a;
    a.origins = origins; a.dirs = directions; a.sbins = sbins; a.R = R; a.S = S; a.ray_offset = 0;
    a.p = *p; a.density = density; a.rgb = rgb; a.aux = aux; a.aux2 = aux2; a.features = nullptr;
    const bool generic = field_set_widths(a.p);
    UNERF_REQUIRE(!generic, "field_fwd_laplace_views: the any-width kernel is not built for several views (nerfacto widths 64 / 64 / 15 / 2, L = 16)");
    UNERF_REQUIRE(!p->sample_major, "field_fwd_laplace_views: sample_major planes are not built for several views");
    const int64_t hw = views->rays_per_view, cr = p->lap_chunk_rays;
    UNERF_REQUIRE(cr >= 0 && cr % 32 == 0, "field_fwd_laplace_views: lap_chunk_rays=%d must be 0 or a positive multiple of 32 (a tile of 32 rays has one sample set)",
                  p->lap_chunk_rays);
    const int64_t spv = cr ? (hw + cr - 1) / cr : 1, sets = p->lap_sets > 1 ? p->lap_sets : 1;   // sets per view, sets in the stacks
    for (int v = 0; v < views->n_views; ++v) {
        const int64_t b = lap_views->set_base[v];
        UNERF_REQUIRE(b >= 0, "field_fwd_laplace_views: set_base[%d]=%lld is negative", v, (long long)b);
        UNERF_REQUIRE(b + spv <= sets, "field_fwd_laplace_views: view %d reads sample sets [%lld, %lld) of %lld (set_base[%d] + sets per view > lap_sets)", v,
                      (long long)b, (long long)(b + spv), (long long)sets, v);
    }
    UNERF_REQUIRE((uint64_t)hw * (uint64_t)S < (1ull << 32), "field_fwd_laplace_views: sample index of a view exceeds 32 bits (rays_per_view x S)");
    UNERF_REQUIRE(p->n_lap >= 1 && p->n_lap <= 32 * LAP_BLOCKS, "field_fwd_laplace_views: n_lap=%d rows do not fit the head blobs (1 to %d)", p->n_lap,
                  32 * LAP_BLOCKS);
    const int64_t bpv = (hw + 31) / 32, tiles = (int64_t)views->n_views * bpv * (int64_t)S;
    UNERF_REQUIRE(S >= 1 && tiles < (1ll << 31), "field_fwd_laplace_views: %lld tiles in one launch (32-bit tile index)", (long long)tiles);
    UNERF_REQUIRE(origins && directions && sbins && density && rgb, "field_fwd_laplace_views: null pointer");
    // the single-view checks see one view: the sample counter bound and the reach into the sets are per view here (above)
    FieldArgs one = a;
    one.R = hw;
    one.p.lap_chunk_rays = 0;
    if (int rc = field_check_args(one, near_plane, generic, nullptr)) return rc;
    field_fill_args(a, near_plane, far_plane, spacing, nullptr);
    one = a;
    one.R = hw;
    one.p.lap_chunk_rays = 0;
    if (int rc = field_check_nonempty(one, spacing, generic)) return rc;
    (void)make_tiles(a, 0);   // 1-D tiles: a.tm says "no image width"
    LapViews lv;
    lv.div_bpv = make_fastdiv((uint32_t)bpv); lv.bpv = (uint32_t)bpv; lv.hw = (uint32_t)hw;
    for (int v = 0; v < UNERF_NERF_MAX_VIEWS; ++v) lv.set_base[v] = lap_views->set_base[v < views->n_views ? v : 0];
    with_int3(tcnn_arg(a.p), [&](auto tc) {
        with_bool(a.p.f16_single != 0, [&](auto f1) {
            const auto kernel = views_laplace_kernel_mfma16<decltype(tc)::value, decltype(f1)::value, LapViews>;
            hipLaunchKernelGGL(kernel, dim3(mfma_grid_for(kernel, tiles, MF_LDS_BYTES)), dim3(256), MF_LDS_BYTES, (hipStream_t)stream, a,
                               (uint32_t)tiles, make_fastdiv((uint32_t)a.S), lv);
        });
    });
    return unerf_check_launch("field_fwd_laplace_views");
}

// --------------------------------------------------------------------------------------
// 5c'. Keep-mask bit arrays (include/unerf.h: unerf_keep_masks).  One thread per output word.
// --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_keep_bits_kernel(const uint8_t* __restrict__ keep, int64_t rows, int n_units, int W,
                                                             uint32_t* __restrict__ bits) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * W) return;
    const int64_t row = i / W;
    const int w = (int)(i - row * W);
    const uint8_t* src = keep + row * n_units + 32 * w;
    const int n = n_units - 32 * w < 32 ? n_units - 32 * w : 32;
    uint32_t word = 0u;
    for (int b = 0; b < n; ++b) word |= (src[b] != 0 ? 1u : 0u) << b;
    bits[i] = word;
}

extern "C" int unerf_pack_keep_bits(const uint8_t* keep, int64_t rows, int n_units, uint32_t* bits, void* stream) {
    UNERF_REQUIRE(rows >= 0 && n_units >= 1 && n_units <= 4096, "pack_keep_bits: rows=%lld, n_units=%d outside [1,4096]", (long long)rows, n_units);
    if (rows == 0) return UNERF_OK;
    UNERF_REQUIRE(keep && bits, "pack_keep_bits: null pointer");
    const int W = (n_units + 31) / 32;
    UNERF_REQUIRE(rows * W < (1ll << 39), "pack_keep_bits: %lld words exceed the launch grid", (long long)(rows * W));
    hipLaunchKernelGGL(pack_keep_bits_kernel, dim3(blocks_for(rows * W, 256)), dim3(256), 0, (hipStream_t)stream, keep, rows,
                       n_units, W, bits);
    return unerf_check_launch("pack_keep_bits");
}

// The counter generator's own masks as bit arrays: word w of a sample covers unit pairs 16 w .. 16 w + 15, made and stepped
// by the functions the field kernels use (unerf_mc_pre / unerf_mc_base_h / unerf_mask_word0 / unerf_mask_step) and tested
// by unerf_keep_lo / unerf_keep_hi.  keep_all: p = 0 (the field kernels generate no masks then).
__global__ __launch_bounds__(256) void mc_keep_bits_kernel(uint32_t seed, int K, int64_t first_sample, int64_t n_samples,
                                                           uint32_t stream_id, int n_units, int W, int32_t thr_hi, int keep_all,
                                                           uint32_t* __restrict__ bits, int64_t pass_stride) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_samples * W) return;
    const int64_t smp = i / W;
    const int w = (int)(i - smp * W);
    const uint32_t pre = unerf_mc_pre(unerf_mc_key(seed, 0u), (uint32_t)(uint64_t)(first_sample + smp));
    const uint32_t bh[2] = {unerf_mc_base_h(pre, 0u), unerf_mc_base_h(pre, 1u)};
    uint32_t word[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const uint32_t j = 16u * (uint32_t)w + (uint32_t)q;
        word[q] = unerf_mask_word0(bh[(j >> 1) & 1u], stream_id, j);
    }
    const uint32_t valid = n_units - 32 * w >= 32 ? 0xFFFFFFFFu : ((1u << (n_units - 32 * w)) - 1u);
    for (int k = 0; k < K; ++k) {
        uint32_t out = 0u;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            if (k > 0) word[q] = unerf_mask_step(word[q]);
            out |= (unerf_keep_lo(word[q], thr_hi) ? 1u : 0u) << (2 * q);
            out |= (unerf_keep_hi(word[q], thr_hi) ? 1u : 0u) << (2 * q + 1);
        }
        bits[((int64_t)k * pass_stride + smp) * W + w] = (keep_all ? 0xFFFFFFFFu : out) & valid;
    }
}

extern "C" int unerf_mc_keep_bits(uint32_t seed, int K, int64_t first_sample, int64_t n_samples, int stream_id, int n_units,
                                  float p_drop, uint32_t* bits, int64_t pass_stride, void* stream) {
    UNERF_REQUIRE(K >= 1 && n_samples >= 0 && first_sample >= 0, "mc_keep_bits: bad K=%d / first_sample / n_samples", K);
    UNERF_REQUIRE(stream_id >= 0 && stream_id <= 3 && n_units >= 1 && n_units <= 128,
                  "mc_keep_bits: stream_id=%d outside [0,3] or n_units=%d outside [1,128] (mask stream layout)", stream_id, n_units);
    UNERF_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "mc_keep_bits: bad p_drop");
    UNERF_REQUIRE(pass_stride >= n_samples, "mc_keep_bits: pass_stride=%lld < n_samples=%lld", (long long)pass_stride, (long long)n_samples);
    UNERF_REQUIRE((uint64_t)(first_sample + n_samples) < (1ull << 32), "mc_keep_bits: sample index exceeds 32 bits (RNG counter)");
    if (n_samples == 0) return UNERF_OK;
    UNERF_REQUIRE(bits, "mc_keep_bits: null pointer");
    const long thr = lrint((1.0 - (double)p_drop) * 65536.0);   // as unerf_field_fwd
    const int32_t thr_s = (int32_t)(thr < 65536 ? thr : 65535) - 32768;
    const int W = (n_units + 31) / 32;
    hipLaunchKernelGGL(mc_keep_bits_kernel, dim3(blocks_for(n_samples * W, 256)), dim3(256), 0, (hipStream_t)stream, seed, K,
                       first_sample, n_samples, (uint32_t)stream_id, n_units, W, (int32_t)((uint32_t)thr_s << 16),
                       thr >= 65536 ? 1 : 0, bits, pass_stride);
    return unerf_check_launch("mc_keep_bits");
}

// --------------------------------------------------------------------------------------
// 5d. Laplace GGN fitting (NerfactoLaplaceModel.compute_hessian_naive, laplace_model.py:343-400).
// The reference multiplies the GGN onto each of the 260 unit vectors (one double-backward per
// parameter per batch).  The loss is the summed MSE, so its Hessian w.r.t. a rendered pixel is 2 I
// and the diagonal is 2 * sum_{ray,channel} J^2 with the Jacobian of the rendered colour
//   C_c = sum_i w_i c_ic + (1 - sum_i w_i) c_{S-1,c}          (background = last sample)
// in closed form.  Last colour layer, row c, input unit k (h = colour hidden, s' = c(1-c)):
//   dC_c/dW_ck = sum_i (w_i + [i = S-1] T_end) s'_ic h_ik
// density layer, unit k (x = base_mlp output, sigma = exp(.) * selector so dsigma/dpre = sigma; with the softplus
// activation dsigma/dpre = 1 - exp(-sigma) takes the place of the last factor sigma_i):
//   dC_c/dw_k = sum_i delta_i [ (1 - alpha_i) T_i c_ic - sum_{j>i} w_j c_jc - T_end c_{S-1,c} ] sigma_i x_ik
// (bias: x = h = 1).  One wave per ray: lane i prepares sample i's scalars with wave scans, then lane k
// accumulates unit k over the samples.  Per-wave partial sums, reduced in a fixed order (deterministic).
// --------------------------------------------------------------------------------------
#define GGN_PARAMS 260
struct GgnArgs {
    const float* sbins;
    int64_t R;
    int S;
    float s_near, s_far;
    int lin;   // UNERF_SPACING_*: 1 = identity spacing (UniformSampler)
    const float* sigma;  // [R,S]
    int softplus;        // density activation: 0 trunc_exp (dsigma/dpre = sigma), 1 softplus (dsigma/dpre = 1 - exp(-sigma))
    const float* rgb;    // [R,S,3]
    const float* X;      // [R,S,64] base_mlp output
    const float* Hc;     // [R,S,64] colour hidden (input of mlp_rgb_ll)
    float* partials;     // [waves][260]
    int bg_mode;         // UNERF_BG_*: the renderer's background (LAST_SAMPLE: the formulas above; COLOR / NONE: a constant
    float bg[3];         // colour (zero for NONE) in place of c_{S-1}, which then takes no gradient from the T_end term)
};

__global__ __launch_bounds__(256) void laplace_ggn_kernel(GgnArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t gw = (int64_t)blockIdx.x * 4 + wv, nw = (int64_t)gridDim.x * 4;
    const int S = a.S;
    const bool in = lane < S;
    float acc_d = 0.f, acc_db = 0.f, acc_r[3] = {0.f, 0.f, 0.f}, acc_rb[3] = {0.f, 0.f, 0.f};
    for (int64_t r = gw; r < a.R; r += nw) {
        const float* sb = a.sbins + r * (S + 1);
        const int i = in ? lane : S - 1;
        const float e0 = unerf_s2e(sb[i], a.s_near, a.s_far, a.lin), e1 = unerf_s2e(sb[i + 1], a.s_near, a.s_far, a.lin);
        const float delta = e1 - e0;
        const float sig = in ? a.sigma[r * S + i] : 0.f;
        float c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = unerf_nan_to_num(a.rgb[(r * S + i) * 3 + k]);
        // dsigma / d(pre-activation): exp -> sigma itself; softplus -> sigmoid(pre) = 1 - exp(-softplus(pre)), and the
        // selector (0 or 1) that multiplies sigma carries over (sigma = 0 -> derivative 0)
        const float dsig = a.softplus ? -expm1f(-sig) : sig;
        const float dd = in ? delta * sig : 0.f;
        const float em = expf(-dd);  // 1 - alpha
        const float T = expf(-group_excl_scan<64>(dd, lane));
        const float w = in ? unerf_nan_to_num((1.f - em) * T) : 0.f;
        const float Tf = 1.f - group_sum<64>(w);
        float g[3], q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const bool last_bg = a.bg_mode == UNERF_BG_LAST_SAMPLE;
            const float bg = last_bg ? __shfl(c[k], S - 1, 64) : a.bg[k];
            const float wc = w * c[k];
            const float incl = group_incl_scan<64>(wc, lane);
            const float tot = __shfl(incl, 63, 64);
            const float pred = tot + Tf * bg;
            // eval-mode renderer clamps to [0,1]: the gradient passes only inside (torch.clamp backward)
            const float live = (pred >= 0.f && pred <= 1.f && in) ? 1.f : 0.f;
            g[k] = live * delta * (em * T * c[k] - (tot - incl) - Tf * bg) * dsig;
            const float wt = w + ((last_bg && lane == S - 1) ? Tf : 0.f);
            q[k] = live * wt * c[k] * (1.f - c[k]);
        }
        float M[3] = {0.f, 0.f, 0.f}, N[3] = {0.f, 0.f, 0.f};
        const float* xr = a.X + r * S * 64 + lane;
        const float* hr = a.Hc + r * S * 64 + lane;
        for (int s = 0; s < S; ++s) {
            const float x = xr[s * 64], hh = hr[s * 64];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                M[k] = fmaf(__shfl(g[k], s, 64), x, M[k]);
                N[k] = fmaf(__shfl(q[k], s, 64), hh, N[k]);
            }
        }
        acc_d += 2.f * (M[0] * M[0] + M[1] * M[1] + M[2] * M[2]);
        float mb2 = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            acc_r[k] += 2.f * N[k] * N[k];
            const float mb = group_sum<64>(g[k]), nb = group_sum<64>(q[k]);
            mb2 += mb * mb;
            acc_rb[k] += 2.f * nb * nb;
        }
        acc_db += 2.f * mb2;
    }
    float* out = a.partials + gw * GGN_PARAMS;
    out[lane] = acc_d;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[65 + k * 64 + lane] = acc_r[k];
    if (lane == 0) {
        out[64] = acc_db;
#pragma unroll
        for (int k = 0; k < 3; ++k) out[65 + 192 + k] = acc_rb[k];
    }
}

__global__ void laplace_ggn_reduce_kernel(const float* partials, int waves, float* ggn_density, float* ggn_rgb) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= GGN_PARAMS) return;
    float sum = 0.f;
    for (int w = 0; w < waves; ++w) sum += partials[(size_t)w * GGN_PARAMS + t];
    if (t < 65) ggn_density[t] += sum;
    else ggn_rgb[t - 65] += sum;
}

static int ggn_blocks(int64_t R) {
    int64_t b = (R + 3) / 4;
    return (int)(b > 1024 ? 1024 : (b < 1 ? 1 : b));
}

extern "C" size_t unerf_laplace_ggn_workspace_bytes(int64_t R, int S) {
    if (R <= 0 || S <= 0) return 0;
    const size_t N = (size_t)R * (size_t)S;
    return (N * (64 + 64 + 1 + 3) + (size_t)ggn_blocks(R) * 4 * GGN_PARAMS) * sizeof(float);
}

extern "C" int unerf_laplace_ggn_diag(const float* origins, const float* directions, const float* sbins, int64_t R,
                                      int S, float near_plane, float far_plane, int spacing, const unerf_field_params* p,
                                      int background, const float* background_rgb, void* workspace, size_t workspace_bytes,
                                      float* ggn_density, float* ggn_rgb, void* stream) {
    UNERF_REQUIRE(R >= 0 && S >= 1 && S <= 64, "laplace_ggn_diag: S=%d outside [1,64]", S);
    if (R == 0) return UNERF_OK;
    UNERF_REQUIRE(origins && directions && sbins && p && workspace && ggn_density && ggn_rgb,
                  "laplace_ggn_diag: null pointer");
    UNERF_REQUIRE(p->mode == UNERF_FIELD_LAPLACE && p->out1 == 15 && p->L == 16 && p->mfma_blob && p->ws_density &&
                      p->ws_rgb && p->table && (p->scalings || p->tcnn_levels),
                  "laplace_ggn_diag: needs a LAPLACE field with mfma_blob and the mean last layers in ws_density[65] / "
                  "ws_rgb[195]");
    UNERF_REQUIRE(p->tcnn_levels || (p->log2T >= 1 && p->log2T <= 24), "laplace_ggn_diag: bad log2T=%d", p->log2T);
    UNERF_REQUIRE((uint64_t)R * (uint64_t)S < (1ull << 32), "laplace_ggn_diag: R*S exceeds 32 bits, split the batch");
    UNERF_REQUIRE(workspace_bytes >= unerf_laplace_ggn_workspace_bytes(R, S),
                  "laplace_ggn_diag: workspace %zu < %zu bytes", workspace_bytes,
                  unerf_laplace_ggn_workspace_bytes(R, S));
    const size_t N = (size_t)R * (size_t)S;
    float* X = static_cast<float*>(workspace);
    float* Hc = X + N * 64;
    float* sigma = Hc + N * 64;
    float* col = sigma + N;
    float* partials = col + N * 3;
    hipStream_t st = (hipStream_t)stream;
    FieldArgs a;
    a.origins = origins; a.dirs = directions; a.sbins = sbins; a.R = R; a.S = S;
    if (int rc = set_spacing(a, near_plane, far_plane, spacing)) return rc;
    a.ray_offset = 0;
    a.p = *p; a.density = sigma; a.rgb = col; a.aux = X; a.aux2 = Hc; a.features = nullptr;
    a.keep_hi = 0; a.keep_pk = 0; a.drop_on = 0; a.drop_sites = 0; a.drop_scale = 1.f;
    a.box = make_norm_box(p->use_aabb, p->aabb);
    a.p.image_width = 0;   // 1-D tiles
    with_int3(tcnn_arg(a.p), [&](auto tc) { launch_matrix_kernel(field_kernel_mfma_laplace<true, decltype(tc)::value>, MF_LDS_BYTES, a, st); });
    GgnArgs g;
    g.sbins = sbins; g.R = R; g.S = S; g.s_near = a.s_near; g.s_far = a.s_far; g.lin = a.lin;
    g.sigma = sigma; g.softplus = p->lap_softplus; g.rgb = col; g.X = X; g.Hc = Hc; g.partials = partials;
    if (int rc = unerf_set_background(g, background, background_rgb, "laplace_ggn_diag")) return rc;
    const int blocks = ggn_blocks(R);
    hipLaunchKernelGGL(laplace_ggn_kernel, dim3(blocks), dim3(256), 0, st, g);
    hipLaunchKernelGGL(laplace_ggn_reduce_kernel, dim3(2), dim3(256), 0, st, partials, blocks * 4, ggn_density, ggn_rgb);
    return unerf_check_launch("laplace_ggn_diag");
}

// --------------------------------------------------------------------------------------
// 5e. Per-ray camera-pose gradient of a nerfacto frame (nerfuncertainty/scripts/estimate_gradient_pose_6dof.py:58-216:
// one torch.autograd.grad(pred_rgb.mean(-1), c2w) per pixel).  s = channel mean of the eval-mode rgb of one ray.  The
// sample bins are held fixed (upstream's PDFSampler detaches them), so the pose reaches s only through the sample
// positions x_i = o + d t_i and the SH encoding of d, and the backward pass needs no stored activations: the adjoint of
// a Linear layer is its transposed weights, the adjoint of a ReLU its sign mask (one bit per unit).
// One wave per ray (four rays per block), one lane per sample, everything in fp32:
//   forward   grid lookup -> trunk -> colour head (activations in LDS as [unit][lane], weights through scalar loads;
//             the arithmetic of field_kernel), compositing with wave scans
//   adjoints  ds/dpred_c = live_c / 3 (live: the clamp passes 0 <= pred <= 1, as laplace_ggn_kernel);
//             drgb_ic = ds/dpred_c (w_i + [i = S-1, last_sample] T_end);
//             dsigma_i = sum_c ds/dpred_c delta_i [(1 - alpha_i) T_i (c_ic - bg_c) - sum_{j>i} w_j c_jc + bg_c sum_{j>i} w_j]
//   backward  sigmoid, W3^T, mask, W2^T, mask, W1^T -> (dSH16 | dgeo15); trunk adjoint (dsigma sigma, dgeo, 0 for beta),
//             Wt1^T, mask, Wt0^T -> dfeat[32]; the exact derivative of the trilinear blend at every level (the corner
//             rows are fetched again) x level scale -> d(normalised position); / 4 and the SceneContraction(inf) Jacobian
//             (or / box length) -> dx_i;  g_o = sum_i dx_i,  g_d = sum_i t_i dx_i + the SH term
// The two sums over the ray are DPP reductions in a fixed order: two calls return the same bits.
// --------------------------------------------------------------------------------------
struct PoseGradArgs {
    const float* origins;
    const float* dirs;
    const float* sbins;
    int64_t R;
    int S;
    float s_near, s_far;
    int lin;
    unerf_field_params p;
    unerf_norm_box box;
    int bg_mode;
    float bg[3];
    int pose;          // 1: rinv holds R^-1 and out_grad is [R,12] = ds/dc2w; 0: out_grad is [R,6] = (ds/do, ds/dd)
    float rinv[9];
    float* out_grad;
    float* out_rgb;    // may be NULL
};

// The weights are read through the CONSTANT address space: a uniform load from it is a scalar load (s_load_dwordx16 into
// SGPRs, which the multiply-adds take as their scalar operand), whereas the same load through a global pointer becomes a
// uniform-address VECTOR load in any kernel that also stores to global memory -- a VGPR per weight, 400 VGPRs here.  The
// weights are written before the launch and never by it, which is all the scalar cache asks for.
typedef const float __attribute__((address_space(4)))* pg_cfp;
__device__ __forceinline__ pg_cfp pg_const(const float* p) { return (pg_cfp)(uintptr_t)p; }
// acc[o] = b[o] + sum_i act[i] Wt[i][o], sequential over i (dense_lds's arithmetic)
template <int IN, int OUT>
__device__ __forceinline__ void pg_dense(pg_cfp Wt, pg_cfp b, const float* act, int lane, float (&acc)[OUT]) {
#pragma unroll
    for (int o = 0; o < OUT; ++o) acc[o] = b[o];
#pragma unroll 2
    for (int i = 0; i < IN; ++i) {
        const float x = act[i * 64 + lane];
#pragma unroll
        for (int o = 0; o < OUT; ++o) acc[o] = fmaf(x, Wt[i * OUT + o], acc[o]);
    }
}
// adjoint of that layer: row i of the LDS panel <- sum_o d[o] Wt[i][o], four partial sums combined in a fixed order
template <int IN, int OUT>
__device__ __forceinline__ void pg_dense_bwd(pg_cfp Wt, const float (&d)[OUT], float* act, int lane) {
#pragma unroll 2
    for (int i = 0; i < IN; ++i) {
        float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int o = 0; o < OUT; ++o) s[o & 3] = fmaf(d[o], Wt[i * OUT + o], s[o & 3]);
        act[i * 64 + lane] = (s[0] + s[1]) + (s[2] + s[3]);
    }
}
__device__ __forceinline__ void relu_mask64(const float (&v)[64], uint32_t (&m)[2]) {
    m[0] = m[1] = 0u;
#pragma unroll
    for (int o = 0; o < 64; ++o) m[o >> 5] |= (v[o] > 0.f) ? (1u << (o & 31)) : 0u;
}
__device__ __forceinline__ void load_masked64(const float* act, int lane, const uint32_t (&m)[2], float (&d)[64]) {
#pragma unroll
    for (int o = 0; o < 64; ++o) d[o] = ((m[o >> 5] >> (o & 31)) & 1u) ? act[o * 64 + lane] : 0.f;
}

// the 8 corner rows of one level as fp32 pairs.  GRID 0: torch layout (corner order and offsets of unerf_hash_corners);
// 1 / 2: tcnn layout (unerf_tcnn_corners), fp32 rows / half2 rows widened on read.  -> interpolation weights (wx, wy, wz)
template <int GRID>
__device__ __forceinline__ void pg_level_corners(const PoseGradArgs& a, int l, uint32_t mask, float px, float py, float pz,
                                                 float2 (&f)[8], float& wx, float& wy, float& wz, float& scale) {
    if constexpr (GRID == 0) {
        const float2* lvl = reinterpret_cast<const float2*>(a.p.table) + ((size_t)l << a.p.log2T);
        scale = a.p.scalings[l];
        uint32_t off[8];
        unerf_hash_corners<false, false>(px, py, pz, scale, mask, off, wx, wy, wz);
        unerf_fetch_corners(lvl, off, f);
    } else {
        const unerf_tcnn_level lv = a.p.tcnn_levels[l];
        scale = lv.scale;
        uint32_t rows[8];
        unerf_tcnn_corners(lv, px, py, pz, rows, wx, wy, wz);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if constexpr (GRID == 1) f[k] = reinterpret_cast<const float2*>(a.p.table)[rows[k]];
            else f[k] = unerf_h2_to_float2(reinterpret_cast<const uint32_t*>(a.p.table)[rows[k]]);
        }
    }
}
// d(blend of the scalar corner values v) / d(wx, wy, wz): the blend is linear in the rows, so the adjoint-weighted sum of the
// two features is blended once
template <int GRID>
__device__ __forceinline__ void pg_blend_grad(const float (&v)[8], float wx, float wy, float wz, float& dx, float& dy, float& dz) {
    const float mx = 1.f - wx, my = 1.f - wy, mz = 1.f - wz;
    if constexpr (GRID == 0) {   // f03, f12, f56, f47 -> y -> z (unerf_blend8); the first of each pair takes the offset itself
        const float v03 = v[0] * wx + v[3] * mx, v12 = v[1] * wx + v[2] * mx, v56 = v[5] * wx + v[6] * mx, v47 = v[4] * wx + v[7] * mx;
        dx = wz * (wy * (v[0] - v[3]) + my * (v[1] - v[2])) + mz * (wy * (v[4] - v[7]) + my * (v[5] - v[6]));
        dy = wz * (v03 - v12) + mz * (v47 - v56);
        dz = (v03 * wy + v12 * my) - (v47 * wy + v56 * my);
    } else {                     // corner k steps +1 along dim d where bit d of k is set (unerf_tcnn_blend)
        const float x0 = v[0] * mx + v[1] * wx, x1 = v[2] * mx + v[3] * wx, x2 = v[4] * mx + v[5] * wx, x3 = v[6] * mx + v[7] * wx;
        dx = mz * (my * (v[1] - v[0]) + wy * (v[3] - v[2])) + wz * (my * (v[5] - v[4]) + wy * (v[7] - v[6]));
        dy = mz * (x1 - x0) + wz * (x3 - x2);
        dz = (x2 * my + x3 * wy) - (x0 * my + x1 * wy);
    }
}

// ---- the stages every pose kernel of 5e runs (pose_grad, pose_jac, pose_grad_mc, pose_grad_laplace), each stated once.  The
// bit equalities between those kernels (MC with K = 1 and full masks = pose_grad; the Jacobian's R/G/B values = pose_grad's
// out_rgb) hold because they call the same statements. ----

// These kernels sit at the register ceiling (256 VGPRs, spills in three of the four), and the spill counts follow the
// SHAPE of a helper's signature, not only its statements: pg_ray_sample and pg_pose_row take the ray's values as scalars,
// pointers and a struct by value, not the argument struct or PgSample / PgRaySums by reference: those forms moved the
// spill counts of pose_grad_kernel, pose_jac_kernel and pose_grad_laplace_kernel (docs/experiments.md 8.6).

// sample i of a ray (sb: its S + 1 bins, o / d: its origin and direction): bin width, twice the midpoint, world position
// (x0, y0, z0), normalised position (px, py, pz) and selector
struct PgSample {
    float delta, t2;       // e1 - e0, e0 + e1
    float dx, dy, dz;      // the ray's direction
    float x0, y0, z0;
    float px, py, pz, sel;
};
__device__ __forceinline__ PgSample pg_ray_sample(const float* sb, const float* o, const float* d, float s_near, float s_far, int lin,
                                                 const unerf_norm_box& box, int i) {
    PgSample s;
    const float e0 = unerf_s2e(sb[i], s_near, s_far, lin), e1 = unerf_s2e(sb[i + 1], s_near, s_far, lin);
    s.delta = e1 - e0, s.t2 = e0 + e1;
    const float ox = o[0], oy = o[1], oz = o[2];
    s.dx = d[0], s.dy = d[1], s.dz = d[2];
    // (d t2) / 2, not d (t2 / 2): field_kernel's rounding
    s.x0 = ox + s.dx * s.t2 / 2.f, s.y0 = oy + s.dy * s.t2 / 2.f, s.z0 = oz + s.dz * s.t2 / 2.f;
    s.px = s.x0, s.py = s.y0, s.pz = s.z0;
    s.sel = unerf_normalize_position(s.px, s.py, s.pz, box);
    return s;
}

// grid forward: rows 2l, 2l+1 of the panel <- the two features of level l (field_kernel's arithmetic)
template <int GRID, int UNROLL>
__device__ __forceinline__ void pg_grid_fwd(const PoseGradArgs& a, uint32_t mask, const PgSample& s, float* A, int lane) {
#pragma unroll UNROLL
    for (int l = 0; l < 16; ++l) {
        float2 f[8];
        float wx, wy, wz, scale;
        pg_level_corners<GRID>(a, l, mask, s.px, s.py, s.pz, f, wx, wy, wz, scale);
        const float2 e = GRID == 0 ? unerf_blend8(f, wx, wy, wz) : unerf_tcnn_blend(f, wx, wy, wz);
        A[(2 * l) * 64 + lane] = e.x;
        A[(2 * l + 1) * 64 + lane] = e.y;
    }
}
// grid backward: rows 2l, 2l+1 hold the adjoint of level l's features; the corner rows are fetched again and the exact
// derivative of the trilinear blend x level scale is summed over the levels -> d / d(normalised position)
template <int GRID, int UNROLL>
__device__ __forceinline__ void pg_grid_bwd(const PoseGradArgs& a, uint32_t mask, const PgSample& s, const float* A, int lane,
                                            float& gpx, float& gpy, float& gpz) {
    gpx = gpy = gpz = 0.f;
#pragma unroll UNROLL
    for (int l = 0; l < 16; ++l) {
        float2 f[8];
        float wx, wy, wz, scale;
        pg_level_corners<GRID>(a, l, mask, s.px, s.py, s.pz, f, wx, wy, wz, scale);
        const float g0 = A[(2 * l) * 64 + lane], g1 = A[(2 * l + 1) * 64 + lane];
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = fmaf(g1, f[k].y, g0 * f[k].x);
        float bx, by, bz;
        pg_blend_grad<GRID>(v, wx, wy, wz, bx, by, bz);
        gpx = fmaf(scale, bx, gpx);
        gpy = fmaf(scale, by, gpy);
        gpz = fmaf(scale, bz, gpz);
    }
}

// SH inputs: (d + 1) / 2, mapped back to [-1, 1] by the tcnn encoding (sh_remap); du/dd = 1/2 or 1
__device__ __forceinline__ void pg_sh_inputs(const PoseGradArgs& a, const PgSample& s, float& ux, float& uy, float& uz) {
    ux = (s.dx + 1.f) / 2.f, uy = (s.dy + 1.f) / 2.f, uz = (s.dz + 1.f) / 2.f;
    if (a.p.sh_remap) {
        ux = ux * 2.f - 1.f;
        uy = uy * 2.f - 1.f;
        uz = uz * 2.f - 1.f;
    }
}
// the SH term of d/dd: rows 0..15 of the panel hold the adjoint of the 16 SH outputs (unerf_sh16) at (ux, uy, uz)
__device__ __forceinline__ void pg_sh16_grad(const float* A, int lane, float ux, float uy, float uz, int remap, float& gx, float& gy,
                                             float& gz) {
    float q[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) q[j] = A[j * 64 + lane];
    const float x = ux, y = uy, z = uz, xx = x * x, yy = y * y, zz = z * z;
    const float c1 = 0.4886025119029199f, c2 = 1.0925484305920792f, c6 = 0.9461746957575601f, c8 = 0.5462742152960396f,
                c9 = 0.5900435899266435f, c10 = 2.890611442640554f, c11 = 0.4570457994644658f, c12 = 0.3731763325901154f,
                c14 = 1.445305721320277f;
    const float z5 = 5.f * zz - 1.f, d3 = 3.f * (xx - yy);
    gx = q[3] * c1 + q[4] * (c2 * y) + q[7] * (c2 * z) + q[8] * (2.f * c8 * x) + q[9] * (6.f * c9 * x * y) + q[10] * (c10 * y * z) +
         q[13] * (c11 * z5) + q[14] * (2.f * c14 * x * z) + q[15] * (c9 * d3);
    gy = q[1] * c1 + q[4] * (c2 * x) + q[5] * (c2 * z) - q[8] * (2.f * c8 * y) + q[9] * (c9 * d3) + q[10] * (c10 * x * z) +
         q[11] * (c11 * z5) - q[14] * (2.f * c14 * y * z) - q[15] * (6.f * c9 * x * y);
    gz = q[2] * c1 + q[5] * (c2 * y) + q[6] * (2.f * c6 * z) + q[7] * (c2 * x) + q[10] * (c10 * x * y) + q[11] * (10.f * c11 * y * z) +
         q[12] * (c12 * (15.f * zz - 3.f)) + q[13] * (10.f * c11 * x * z) + q[14] * (c14 * (xx - yy));
    const float du = remap ? 1.f : 0.5f;
    gx *= du;
    gy *= du;
    gz *= du;
}

// sum_{j>i} x_j as a scan over the reversed wave, NOT total - prefix: behind an opaque sample every term of dsigma is
// of the size of the transmittance there, and the rounding of a difference of O(1) sums (2^-24), multiplied by
// delta sigma of a dense sample (1e3 and more), would be the whole error of the gradient
__device__ __forceinline__ float pg_suffix_sum(float x, int lane) {
    const int rl = 63 - lane;
    return __shfl(group_excl_scan<64>(__shfl(x, rl, 64), lane), rl, 64);
}
// compositing of one ray (laplace_ggn_kernel's scans): alpha_i = 1 - em, transmittance T in front of sample i, weight w,
// accumulation, transmittance Tf behind the ray and sw = sum_{j>i} w_j
struct PgWeights {
    float em, T, w, Asum, Tf, sw;
};
__device__ __forceinline__ PgWeights pg_transmittance(bool in, float delta, float sig, int lane) {
    PgWeights c;
    const float dd = in ? delta * sig : 0.f;
    c.em = expf(-dd);
    c.T = expf(-group_excl_scan<64>(dd, lane));
    c.w = in ? unerf_nan_to_num((1.f - c.em) * c.T) : 0.f;
    c.Asum = group_sum<64>(c.w);
    c.Tf = 1.f - c.Asum;
    c.sw = pg_suffix_sum(c.w, lane);
    return c;
}

// d / d(normalised position) -> d / d(world position): the selector, then / box length, or / 4 and the transposed
// Jacobian of SceneContraction(inf) at (x0, y0, z0)
__device__ __forceinline__ void pg_world_grad(const unerf_norm_box& box, const PgSample& s, float gpx, float gpy, float gpz, float& gx,
                                              float& gy, float& gz) {
    const float x0 = s.x0, y0 = s.y0, z0 = s.z0;
    gx = gpx * s.sel, gy = gpy * s.sel, gz = gpz * s.sel;
    if (box.use_aabb) {   // uniform
        gx /= box.len[0];
        gy /= box.len[1];
        gz /= box.len[2];
    } else {
        gx *= 0.25f;
        gy *= 0.25f;
        gz *= 0.25f;
        const float ax = fabsf(x0), ay = fabsf(y0), az = fabsf(z0);
        const float m = fmaxf(fmaxf(ax, ay), az);
        if (!(m < 1.f)) {
            // y = (2 - 1/m) x / m, m = |x_k|: dy_j/dx_j = (2 - 1/m)/m (j != k), dy_k/dx_k = 1/m^2,
            // dy_j/dx_k = x_j sign(x_k) 2 (1 - m) / m^3
            const float inv = 1.f / m, diag = (2.f - inv) * inv, cross = 2.f * (1.f - m) * inv * inv * inv;
            const int k = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
            const float dot = (k == 0 ? 0.f : gx * x0) + (k == 1 ? 0.f : gy * y0) + (k == 2 ? 0.f : gz * z0);
            const float xk = k == 0 ? x0 : (k == 1 ? y0 : z0), gk = k == 0 ? gx : (k == 1 ? gy : gz);
            const float along = gk * inv * inv + cross * (xk < 0.f ? -dot : dot);
            gx = k == 0 ? along : gx * diag;
            gy = k == 1 ? along : gy * diag;
            gz = k == 2 ? along : gz * diag;
        }
    }
}

// the six sums over the ray, DPP reductions in a fixed order: g_o = sum_i dx_i, g_d = sum_i (t_i dx_i + the SH term),
// t_i = t2 / 2 formed here, behind the backward pass
struct PgRaySums {
    float go0, go1, go2, gd0, gd1, gd2;
};
__device__ __forceinline__ PgRaySums pg_ray_sums(bool in, float t2, float gx, float gy, float gz, float gdx, float gdy, float gdz) {
    if (!in) gx = gy = gz = gdx = gdy = gdz = 0.f;
    const float th = t2 / 2.f;
    PgRaySums s;
    s.go0 = group_sum<64>(gx), s.go1 = group_sum<64>(gy), s.go2 = group_sum<64>(gz);
    s.gd0 = group_sum<64>(fmaf(th, gx, gdx)), s.gd1 = group_sum<64>(fmaf(th, gy, gdy)), s.gd2 = group_sum<64>(fmaf(th, gz, gdz));
    return s;
}
// lane j's entry of the ray's row: a.pose: the 12 entries of d/dc2w (row-major 3x4), else the 6 of (d/do, d/dd).  (dx, dy, dz):
// the ray's direction
__device__ __forceinline__ float pg_pose_row(const PoseGradArgs& a, int lane, float dx, float dy, float dz, PgRaySums g) {
    if (a.pose) {
        // d = normalize(R dir_cam): ds/dc2w[a][b] = P[a] (R^-1 d)[b] with P = (I - d d^T) g_d; ds/dc2w[:, 3] = g_o
        const float gdd = g.gd0 * dx + g.gd1 * dy + g.gd2 * dz;
        const float P[3] = {g.gd0 - dx * gdd, g.gd1 - dy * gdd, g.gd2 - dz * gdd};
        const float go[3] = {g.go0, g.go1, g.go2};
        const int row = lane >> 2, col = lane & 3;
        const float Pa = row == 0 ? P[0] : (row == 1 ? P[1] : P[2]);
        const float ga = row == 0 ? go[0] : (row == 1 ? go[1] : go[2]);
        const int cb = col < 3 ? col : 0;
        const float q = a.rinv[cb * 3 + 0] * dx + a.rinv[cb * 3 + 1] * dy + a.rinv[cb * 3 + 2] * dz;
        return col == 3 ? ga : Pa * q;
    }
    return lane == 0 ? g.go0 : lane == 1 ? g.go1 : lane == 2 ? g.go2 : lane == 3 ? g.gd0 : lane == 4 ? g.gd1 : g.gd2;
}
// the store of that row by the three gradient kernels: a vector store of a lane-selected value
__device__ __forceinline__ void pg_store_grad(const PoseGradArgs& a, int64_t r, int lane, float v) {
    if (a.pose) {
        if (lane < 12) a.out_grad[r * 12 + lane] = v;
    } else {
        if (lane < 6) a.out_grad[r * 6 + lane] = v;
    }
}

template <int OUT1, int GRID>
__global__ __launch_bounds__(256, 2) void pose_grad_kernel(PoseGradArgs a) {   // two waves per SIMD: two 64-KiB blocks per CU
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float* A = lds + wv * (64 * 64);   // this wave's panel [64 units][64 lanes]; a lane reads only its own column
    // one ray per wave, no loop over rays: a block's four panels fill its 64 KiB of LDS and two blocks share a CU
    const int64_t r = (int64_t)blockIdx.x * 4 + wv;
    if (r >= a.R) return;   // wave-uniform
    const int S = a.S;
    const bool in = lane < S;
    const int i = in ? lane : S - 1;
    const uint32_t mask = GRID == 0 ? (1u << a.p.log2T) - 1u : 0u;
    {
        // ---- sample position, normalisation ----
        const PgSample s = pg_ray_sample(a.sbins + r * (S + 1), a.origins + r * 3, a.dirs + r * 3, a.s_near, a.s_far, a.lin,
                                         a.box, i);
        const float delta = s.delta, sel = s.sel;

        // ---- forward: grid -> trunk -> head (field_kernel's arithmetic) ----
        pg_grid_fwd<GRID, 2>(a, mask, s, A, lane);
        float acc[64];
        uint32_t m0[2], m1[2], m2[2];
        pg_dense<32, 64>(pg_const(a.p.w0t), pg_const(a.p.b0), A, lane, acc);
        relu_mask64(acc, m0);
        store_act<64>(A, lane, acc, 0, true);
        float o1[OUT1];
        pg_dense<64, OUT1>(pg_const(a.p.w1t), pg_const(a.p.b1), A, lane, o1);
        const float sig = a.p.average_init_density * expf(o1[0]) * sel;
        float ux, uy, uz;
        pg_sh_inputs(a, s, ux, uy, uz);
        {
            float sh[16];
            unerf_sh16(ux, uy, uz, sh);
            store_act<16>(A, lane, sh, 0, false);
        }
#pragma unroll
        for (int g = 0; g < 15; ++g) A[(16 + g) * 64 + lane] = o1[1 + g];
        pg_dense<31, 64>(pg_const(a.p.h0t), pg_const(a.p.hb0), A, lane, acc);
        relu_mask64(acc, m1);
        store_act<64>(A, lane, acc, 0, true);
        pg_dense<64, 64>(pg_const(a.p.h1t), pg_const(a.p.hb1), A, lane, acc);
        relu_mask64(acc, m2);
        store_act<64>(A, lane, acc, 0, true);
        float c[3];
        pg_dense<64, 3>(pg_const(a.p.h2t), pg_const(a.p.hb2), A, lane, c);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = unerf_nan_to_num(unerf_sigmoid(c[k]));

        // ---- compositing and its adjoints (laplace_ggn_kernel's scans) ----
        const PgWeights cw = pg_transmittance(in, delta, sig, lane);
        const float em = cw.em, T = cw.T, w = cw.w, Tf = cw.Tf, sw = cw.sw;
        const bool last_bg = a.bg_mode == UNERF_BG_LAST_SAMPLE;
        float dsig = 0.f, dc[3], pred[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float bg = last_bg ? __shfl(c[k], S - 1, 64) : a.bg[k];
            const float wc = w * c[k];
            const float swc = pg_suffix_sum(wc, lane);
            pred[k] = group_sum<64>(wc) + Tf * bg;
            const float live = (pred[k] >= 0.f && pred[k] <= 1.f && in) ? 1.f / 3.f : 0.f;
            // d pred / d(delta_i sigma_i) of pred = sum_j w_j c_j + bg (1 - sum_j w_j), w_i = (1 - em_i) T_i
            dsig += live * delta * (em * T * (c[k] - bg) - swc + bg * sw);
            const float wt = w + ((last_bg && lane == S - 1) ? Tf : 0.f);
            dc[k] = live * wt * c[k] * (1.f - c[k]);   // through the sigmoid
        }

        // ---- backward: colour head ----
        float d[64];
        const pg_cfp h2t = pg_const(a.p.h2t);
#pragma unroll
        for (int o = 0; o < 64; ++o) {
            const float v = fmaf(dc[2], h2t[o * 3 + 2], fmaf(dc[1], h2t[o * 3 + 1], dc[0] * h2t[o * 3 + 0]));
            d[o] = ((m2[o >> 5] >> (o & 31)) & 1u) ? v : 0.f;
        }
        pg_dense_bwd<64, 64>(pg_const(a.p.h1t), d, A, lane);
        load_masked64(A, lane, m1, d);
        pg_dense_bwd<31, 64>(pg_const(a.p.h0t), d, A, lane);   // rows 0..15: dSH, 16..30: dgeo
        float gdx, gdy, gdz;   // the SH term of ds/dd
        pg_sh16_grad(A, lane, ux, uy, uz, a.p.sh_remap, gdx, gdy, gdz);
        // ---- backward: trunk ----
        float d1[OUT1];
        d1[0] = dsig * sig;   // sigma = aid exp(pre) selector: dsigma/dpre = sigma (zero where the selector is)
#pragma unroll
        for (int g = 0; g < 15; ++g) d1[1 + g] = A[(16 + g) * 64 + lane];
        if constexpr (OUT1 == 17) d1[16] = 0.f;   // the learned-variance logit does not reach the colour
        pg_dense_bwd<64, OUT1>(pg_const(a.p.w1t), d1, A, lane);
        load_masked64(A, lane, m0, d);
        pg_dense_bwd<32, 64>(pg_const(a.p.w0t), d, A, lane);   // rows 2l, 2l+1: adjoint of level l's features

        // ---- backward: grid -> normalised position -> world position, ray sums ----
        float gpx, gpy, gpz, gx, gy, gz;
        pg_grid_bwd<GRID, 2>(a, mask, s, A, lane, gpx, gpy, gpz);
        pg_world_grad(a.box, s, gpx, gpy, gpz, gx, gy, gz);
        const PgRaySums sums = pg_ray_sums(in, s.t2, gx, gy, gz, gdx, gdy, gdz);

        // ---- epilogue: every store is a vector store of a lane-selected value ----
        pg_store_grad(a, r, lane, pg_pose_row(a, lane, s.dx, s.dy, s.dz, sums));
        if (a.out_rgb && lane < 3) {
            const float pv = lane == 0 ? pred[0] : (lane == 1 ? pred[1] : pred[2]);
            a.out_rgb[r * 3 + lane] = fminf(fmaxf(pv, 0.f), 1.f);
        }
    }
}

// ---- host side of 5e: what the four entry points check, fill and launch alike, stated once; `what` is the entry point's
// name in front of every text.  The checks come in pieces because each entry point has checks of its own between them, and
// the first error a call reports stays the one it was: S; (pose_jacobian: channels, projection, outputs;) nothing more for
// R == 0 -- an empty batch has no pointers to give --; the pointers; the field's mode (it reads *p); the field. ----
static int pose_check_samples(const char* what, int64_t R, int S) {
    UNERF_REQUIRE(R >= 0 && S >= 1 && S <= 64, "%s: S=%d outside [1,64]", what, S);
    return UNERF_OK;
}
// have_out: the entry point's output pointer is there
static int pose_check_pointers(const char* what, const float* origins, const float* directions, const float* sbins,
                               const unerf_field_params* p, bool have_out) {
    UNERF_REQUIRE(origins && directions && sbins && p && have_out, "%s: null pointer", what);
    return UNERF_OK;
}
// The field behind them.  out1: the trunk outputs the (checked) mode has.  sampled_heads: the Laplace field, whose trunk
// has the 15 geo outputs only, which its widths text says, and whose last layers are the rows ws_density / ws_rgb in place
// of h2t / hb2.  scope: what the entry point adds to the widths text.
static int pose_check_field(const char* what, const unerf_field_params* p, float near_plane, int out1, bool sampled_heads,
                            const char* scope) {
    UNERF_REQUIRE(p->hidden == 0 && p->hidden_color == 0 && p->geo_dim == 0 && p->feat_per_level == 0 && p->L == 16 &&
                      (!sampled_heads || p->out1 == out1),
                  "%s: nerfacto's widths only (hidden 64 / 64, geo 15%s, 2 features x 16 levels)%s", what,
                  sampled_heads ? " = trunk output 15" : "", scope);
    UNERF_REQUIRE(p->out1 == out1, "%s: trunk output %d does not fit mode %d", what, p->out1, p->mode);
    UNERF_REQUIRE(p->table && p->w0t && p->b0 && p->w1t && p->b1 && p->h0t && p->hb0 && p->h1t && p->hb1 &&
                      (sampled_heads || (p->h2t && p->hb2)) && (p->scalings || p->tcnn_levels),
                  "%s: null field pointer", what);
    UNERF_REQUIRE(!sampled_heads || (p->ws_density && p->ws_rgb),
                  "%s: null ws_density / ws_rgb (the sampled last layers of the named draw)", what);
    UNERF_REQUIRE(p->tcnn_levels || (p->log2T >= 1 && p->log2T <= 24), "%s: bad log2T=%d", what, p->log2T);
    UNERF_REQUIRE(p->tcnn_levels || !p->grid_half, "%s: grid_half needs a tcnn-layout grid", what);
    UNERF_REQUIRE(near_plane >= 0.f, "%s: near_plane=%g (spacing-domain bins only)", what, (double)near_plane);
    return UNERF_OK;
}
// PoseGradArgs of a checked call.  max_rays: what one launch of the entry point's grid takes.
static int pose_fill_args(PoseGradArgs& g, const char* what, const float* origins, const float* directions, const float* sbins,
                          int64_t R, int S, float near_plane, float far_plane, int spacing, const unerf_field_params* p,
                          int background, const float* background_rgb, const float* rot_inv, float* out_grad, float* out_rgb,
                          int64_t max_rays) {
    g.origins = origins; g.dirs = directions; g.sbins = sbins; g.R = R; g.S = S;
    if (int rc = set_spacing(g, near_plane, far_plane, spacing)) return rc;
    g.p = *p;
    g.box = make_norm_box(p->use_aabb, p->aabb);
    if (int rc = unerf_set_background(g, background, background_rgb, what)) return rc;
    g.pose = rot_inv ? 1 : 0;
    for (int k = 0; k < 9; ++k) g.rinv[k] = rot_inv ? rot_inv[k] : 0.f;
    g.out_grad = out_grad; g.out_rgb = out_rgb;
    UNERF_REQUIRE(R < max_rays, "%s: R=%lld rays in one launch, split the batch", what, (long long)R);
    return UNERF_OK;
}
// pose_grad_kernel's geometry, which pose_jac_kernel and pose_grad_laplace_kernel keep: a wave per ray, four rays per
// 256-thread block, whose four 16-KiB panels are 64 KiB of LDS: two blocks per CU
template <typename Kern, typename... Args>
static void pose_launch_rays4(Kern kernel, int64_t R, void* stream, Args... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 4 * 64 * 64 * sizeof(float), (hipStream_t)stream, args...);
}

extern "C" int unerf_pose_grad(const float* origins, const float* directions, const float* sbins, int64_t R, int S,
                               float near_plane, float far_plane, int spacing, const unerf_field_params* p, int background,
                               const float* background_rgb, const float* rot_inv, float* out_grad, float* out_rgb,
                               void* stream) {
    if (int rc = pose_check_samples("pose_grad", R, S)) return rc;
    if (R == 0) return UNERF_OK;
    if (int rc = pose_check_pointers("pose_grad", origins, directions, sbins, p, out_grad != nullptr)) return rc;
    UNERF_REQUIRE(p->mode == UNERF_FIELD_ACTIVE || p->mode == UNERF_FIELD_MCDROPOUT,
                  "pose_grad: mode %d (a nerfacto / active-nerfacto field is needed: the Laplace field's sampled heads are "
                  "not differentiated)", p->mode);
    if (int rc = pose_check_field("pose_grad", p, near_plane, p->mode == UNERF_FIELD_ACTIVE ? 17 : 16, false, "")) return rc;
    PoseGradArgs g;
    if (int rc = pose_fill_args(g, "pose_grad", origins, directions, sbins, R, S, near_plane, far_plane, spacing, p, background,
                                background_rgb, rot_inv, out_grad, out_rgb, 1ll << 32)) return rc;
    with_int3(tcnn_arg(g.p), [&](auto tc) {
        with_bool(g.p.out1 == 17, [&](auto wide) {
            pose_launch_rays4(pose_grad_kernel<decltype(wide)::value ? 17 : 16, decltype(tc)::value>, R, stream, g);
        });
    });
    return unerf_check_launch("pose_grad");
}

// --------------------------------------------------------------------------------------
// 5e-J. Per-ray pose JACOBIAN: one row per selected output channel (clamp(pred_r), clamp(pred_g), clamp(pred_b), the
// accumulation A = sum_i w_i, the unclipped expected depth e = N / (A + 1e-10), N = sum_i w_i t_i) behind ONE forward.  The
// backward of pose_grad_kernel keeps only three ReLU bit masks, the weights and the scans and is linear in its seed, so it is
// run once per channel in a wave-uniform loop; the LDS panel holds adjoints only from then on.
//   row R/G/B  the seed of pose_grad_kernel with live_c in place of live_c / 3 and the other two channels at 0
//   row ACC    dA/d(delta_i sigma_i) = T_end = em_{S-1} T_{S-1} (read off the scan, not 1 - A: behind an opaque sample T_end
//              is far below the rounding of A); no colour head, no SH term
//   row EDEPTH de/d(delta_i sigma_i) = [(1 - alpha_i) T_i u_i - sum_{j>i} w_j u_j] / (A + eps), u = t - e: the quotient rule
//              [(1-alpha_i) T_i t_i - sum_{j>i} w_j t_j] / (A+eps) - N/(A+eps)^2 [(1-alpha_i) T_i - sum_{j>i} w_j] with e taken
//              into the sum first (the depths are centred before they are weighted, as autograd's backward does); the suffix
//              sum is the reversed-wave scan.  The clip of the renderer to the step range is not differentiated.
// Behind a row: out_proj = row . proj (sequential over D in lane k), out_var = sum_k out_proj_k^2 (sequential over P).
// No atomics, no global scratch; every pass is a fixed sequence of the same statements: a row's bits depend neither on the
// other rays, nor on the other channels, nor on which outputs were asked for.
// --------------------------------------------------------------------------------------
struct PoseJacArgs {
    PoseGradArgs g;       // out_grad / out_rgb are not read; g.pose: D = 12, else 6
    int channels;         // UNERF_POSE_CH_* bits; rows in bit order
    int C;                // popcount(channels)
    int P;                // 0: no projection
    float proj[12 * 12];  // [D][P] row-major
    float* out_jac;       // NULL or [R,C,D]
    float* out_proj;      // NULL or [R,C,P]
    float* out_var;       // NULL or [R,C]
    float* out_val;       // NULL or [R,C]
};

template <int OUT1, int GRID>
__global__ __launch_bounds__(256, 2) void pose_jac_kernel(PoseJacArgs ja) {
    extern __shared__ float lds[];
    const PoseGradArgs& a = ja.g;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float* A = lds + wv * (64 * 64);
    const int64_t r = (int64_t)blockIdx.x * 4 + wv;
    if (r >= a.R) return;   // wave-uniform
    const int S = a.S;
    const bool in = lane < S;
    const int i = in ? lane : S - 1;
    const uint32_t mask = GRID == 0 ? (1u << a.p.log2T) - 1u : 0u;
    // ---- sample position, normalisation; forward: grid -> trunk -> head (pose_grad_kernel's, down to the compositing) ----
    const PgSample s = pg_ray_sample(a.sbins + r * (S + 1), a.origins + r * 3, a.dirs + r * 3, a.s_near, a.s_far, a.lin,
                                     a.box, i);
    const float delta = s.delta, sel = s.sel;
    pg_grid_fwd<GRID, 2>(a, mask, s, A, lane);
    uint32_t m0[2], m1[2], m2[2];
    float sig, c[3];
    float ux, uy, uz;
    pg_sh_inputs(a, s, ux, uy, uz);
    {
        float acc[64];
        pg_dense<32, 64>(pg_const(a.p.w0t), pg_const(a.p.b0), A, lane, acc);
        relu_mask64(acc, m0);
        store_act<64>(A, lane, acc, 0, true);
        float o1[OUT1];
        pg_dense<64, OUT1>(pg_const(a.p.w1t), pg_const(a.p.b1), A, lane, o1);
        sig = a.p.average_init_density * expf(o1[0]) * sel;
        {
            float sh[16];
            unerf_sh16(ux, uy, uz, sh);
            store_act<16>(A, lane, sh, 0, false);
        }
#pragma unroll
        for (int g = 0; g < 15; ++g) A[(16 + g) * 64 + lane] = o1[1 + g];
        pg_dense<31, 64>(pg_const(a.p.h0t), pg_const(a.p.hb0), A, lane, acc);
        relu_mask64(acc, m1);
        store_act<64>(A, lane, acc, 0, true);
        pg_dense<64, 64>(pg_const(a.p.h1t), pg_const(a.p.hb1), A, lane, acc);
        relu_mask64(acc, m2);
        store_act<64>(A, lane, acc, 0, true);
        pg_dense<64, 3>(pg_const(a.p.h2t), pg_const(a.p.hb2), A, lane, c);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = unerf_nan_to_num(unerf_sigmoid(c[k]));
    }

    // ---- compositing, once: the weights, the scans and every channel's value ----
    const PgWeights cw = pg_transmittance(in, delta, sig, lane);
    const float em = cw.em, T = cw.T, w = cw.w, Asum = cw.Asum, Tf = cw.Tf, sw = cw.sw;
    const bool last_bg = a.bg_mode == UNERF_BG_LAST_SAMPLE;
    float bg[3], swc[3], pred[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        bg[k] = last_bg ? __shfl(c[k], S - 1, 64) : a.bg[k];
        const float wc = w * c[k];
        swc[k] = pg_suffix_sum(wc, lane);
        pred[k] = group_sum<64>(wc) + Tf * bg[k];
    }
    const float th = s.t2 / 2.f;
    const float Tend = __shfl(em * T, S - 1, 64);              // the transmittance behind the last sample
    const float inv_a = 1.f / (Asum + 1e-10f);
    const float edep = group_sum<64>(w * th) * inv_a;          // unclipped expected depth
    const float swu = pg_suffix_sum(w * (th - edep), lane);    // sum_{j>i} w_j (t_j - e)

    const int D = a.pose ? 12 : 6;
    int row = 0;
#pragma unroll 1
    for (int ch = 0; ch < 5; ++ch) {   // wave-uniform
        if (!((ja.channels >> ch) & 1)) continue;
        const int64_t rc = r * ja.C + row;
        ++row;
        float dsig, val;
        float gdx = 0.f, gdy = 0.f, gdz = 0.f;   // the SH term of d row / dd
        float d[64];
        float d1[OUT1];
#pragma unroll
        for (int g = 0; g < OUT1; ++g) d1[g] = 0.f;
        if (ch < 3) {
            const float ck = ch == 0 ? c[0] : (ch == 1 ? c[1] : c[2]);
            const float bk = ch == 0 ? bg[0] : (ch == 1 ? bg[1] : bg[2]);
            const float sk = ch == 0 ? swc[0] : (ch == 1 ? swc[1] : swc[2]);
            const float pk = ch == 0 ? pred[0] : (ch == 1 ? pred[1] : pred[2]);
            val = fminf(fmaxf(pk, 0.f), 1.f);
            const float live = (pk >= 0.f && pk <= 1.f && in) ? 1.f : 0.f;
            dsig = live * delta * (em * T * (ck - bk) - sk + bk * sw);
            const float wt = w + ((last_bg && lane == S - 1) ? Tf : 0.f);
            const float dck = live * wt * ck * (1.f - ck);   // through the sigmoid
            // ---- backward: colour head, this channel's column of the last layer ----
            const pg_cfp h2t = pg_const(a.p.h2t);
#pragma unroll
            for (int o = 0; o < 64; ++o) d[o] = ((m2[o >> 5] >> (o & 31)) & 1u) ? dck * h2t[o * 3 + ch] : 0.f;
            pg_dense_bwd<64, 64>(pg_const(a.p.h1t), d, A, lane);
            load_masked64(A, lane, m1, d);
            pg_dense_bwd<31, 64>(pg_const(a.p.h0t), d, A, lane);   // rows 0..15: dSH, 16..30: dgeo
            pg_sh16_grad(A, lane, ux, uy, uz, a.p.sh_remap, gdx, gdy, gdz);
#pragma unroll
            for (int g = 0; g < 15; ++g) d1[1 + g] = A[(16 + g) * 64 + lane];
        } else if (ch == 3) {
            val = Asum;
            dsig = in ? delta * Tend : 0.f;
        } else {
            val = edep;
            dsig = in ? delta * inv_a * (em * T * (th - edep) - swu) : 0.f;
        }
        // ---- backward: trunk (the density logit; for a colour row also dgeo) ----
        d1[0] = dsig * sig;
        pg_dense_bwd<64, OUT1>(pg_const(a.p.w1t), d1, A, lane);
        load_masked64(A, lane, m0, d);
        pg_dense_bwd<32, 64>(pg_const(a.p.w0t), d, A, lane);

        // ---- backward: grid -> normalised position -> world position, ray sums ----
        float gpx, gpy, gpz, gx, gy, gz;
        pg_grid_bwd<GRID, 2>(a, mask, s, A, lane, gpx, gpy, gpz);
        pg_world_grad(a.box, s, gpx, gpy, gpz, gx, gy, gz);
        const PgRaySums sums = pg_ray_sums(in, s.t2, gx, gy, gz, gdx, gdy, gdz);

        // ---- epilogue: lane j holds entry j of the row; every store is a vector store of a lane-selected value ----
        const float jv = pg_pose_row(a, lane, s.dx, s.dy, s.dz, sums);
        if (ja.out_jac && lane < D) ja.out_jac[rc * D + lane] = jv;
        if (ja.out_val && lane == 0) ja.out_val[rc] = val;
        if (ja.P > 0 && (ja.out_proj || ja.out_var)) {   // uniform
            const int P = ja.P;
            const int k = lane < P ? lane : 0;
            float pv = 0.f;
            for (int j = 0; j < D; ++j) pv = fmaf(__shfl(jv, j, 64), ja.proj[j * P + k], pv);
            if (ja.out_proj && lane < P) ja.out_proj[rc * P + lane] = pv;
            if (ja.out_var) {
                float var = 0.f;
                for (int q = 0; q < P; ++q) {
                    const float v = __shfl(pv, q, 64);
                    var = fmaf(v, v, var);
                }
                if (lane == 0) ja.out_var[rc] = var;
            }
        }
    }
}

extern "C" int unerf_pose_jacobian(const float* origins, const float* directions, const float* sbins, int64_t R, int S,
                                   float near_plane, float far_plane, int spacing, const unerf_field_params* p, int background,
                                   const float* background_rgb, const float* rot_inv, int channels, const float* proj, int P,
                                   float* out_jac, float* out_proj, float* out_var, float* out_val, void* stream) {
    constexpr int CH_KNOWN = UNERF_POSE_CH_R | UNERF_POSE_CH_G | UNERF_POSE_CH_B | UNERF_POSE_CH_ACC | UNERF_POSE_CH_EDEPTH;
    if (int rc = pose_check_samples("pose_jacobian", R, S)) return rc;
    UNERF_REQUIRE(channels != 0, "pose_jacobian: channels is empty (a non-empty subset of UNERF_POSE_CH_*)");
    UNERF_REQUIRE((channels & ~CH_KNOWN) == 0, "pose_jacobian: unknown bits in channels=%d", channels);
    UNERF_REQUIRE(!proj || (P >= 1 && P <= 12), "pose_jacobian: P=%d outside [1,12]", P);
    UNERF_REQUIRE(proj || (!out_proj && !out_var), "pose_jacobian: out_proj / out_var need proj");
    UNERF_REQUIRE(out_jac || out_proj || out_var || out_val, "pose_jacobian: no output requested (out_jac, out_proj, out_var and out_val are all NULL)");
    if (R == 0) return UNERF_OK;
    if (int rc = pose_check_pointers("pose_jacobian", origins, directions, sbins, p, true)) return rc;
    UNERF_REQUIRE(p->mode == UNERF_FIELD_ACTIVE || p->mode == UNERF_FIELD_MCDROPOUT,
                  "pose_jacobian: mode %d (a nerfacto / active-nerfacto field is needed: the Laplace field's sampled heads are "
                  "not differentiated)", p->mode);
    if (int rc = pose_check_field("pose_jacobian", p, near_plane, p->mode == UNERF_FIELD_ACTIVE ? 17 : 16, false, "")) return rc;
    PoseJacArgs j;
    PoseGradArgs& g = j.g;   // out_grad / out_rgb are not read
    if (int rc = pose_fill_args(g, "pose_jacobian", origins, directions, sbins, R, S, near_plane, far_plane, spacing, p, background,
                                background_rgb, rot_inv, nullptr, nullptr, 1ll << 32)) return rc;
    j.channels = channels;
    j.C = __builtin_popcount((unsigned)channels);
    j.P = proj ? P : 0;
    const int D = rot_inv ? 12 : 6;
    for (int k = 0; k < 144; ++k) j.proj[k] = (proj && k < D * P) ? proj[k] : 0.f;
    j.out_jac = out_jac; j.out_proj = out_proj; j.out_var = out_var; j.out_val = out_val;
    with_int3(tcnn_arg(g.p), [&](auto tc) {
        with_bool(g.p.out1 == 17, [&](auto wide) {
            pose_launch_rays4(pose_jac_kernel<decltype(wide)::value ? 17 : 16, decltype(tc)::value>, R, stream, j);
        });
    });
    return unerf_check_launch("pose_jacobian");
}

// --------------------------------------------------------------------------------------
// 5e'. The same gradient of an MC-DROPOUT frame under a named mask draw: rgb = (1/K) sum_k clamp(pred_k), pass k with the
// keep masks of (seed, pass, sample, unit) -- the counter generator's, or explicit bit arrays (unerf_keep_masks).  Under a
// fixed draw every pass is the deterministic piecewise-smooth function pose_grad_kernel differentiates, with h -> h keep /
// (1 - p) behind the ReLU of each active site; the adjoint of that is the same factor.  Dropout sits BEHIND trunk layer 0, so
// the grid lookup and layer 0 do not depend on the pass, and the adjoints of all passes are summed in front of them:
//   once      grid lookup -> F[32] -> layer 0 -> ReLU bits m0, activations H0 (a second LDS panel, kept for all passes)
//   per pass  A <- H0 keep_T scale; layer 1 -> sigma_k, geo; colour head with keep_0 / keep_1; compositing and its adjoints;
//             head and trunk backward down to the layer-0 pre-activation: G[64] += (m0 & keep_T) scale A   (registers)
//   once      W0^T G -> dfeat[32]; grid backward (the corner rows fetched the second and last time); contraction; ray sums
// One wave = one ray = one block (two 16-KiB panels, 256 VGPRs + 188 AGPRs, no scratch: one wave per SIMD -- DESIGN.md 4.6a);
// the sums over passes run k = 0 .. K-1: two calls return the same bits.
// With K = 1 and every unit kept at scale 1.0 each statement of a pass is pose_grad_kernel's, in its order.
// --------------------------------------------------------------------------------------
struct PoseGradMcArgs {
    KeepArgs xm;          // explicit masks: site[] = TRUNK, HEAD0, HEAD1 (counter mode: all NULL)
    int explicit_masks;
    int K;
    int keep_all;         // counter mode: the threshold keeps every unit (p <= 2^-17)
    int32_t keep_hi;      // counter mode: thr_s << 16
    uint32_t key;         // counter mode: unerf_mc_key(seed, 0)
    uint32_t sample0;     // counter mode: ray_offset * S
    float scale[3];       // 1 / (1 - p) at an active site, 1 at an inactive one (TRUNK, HEAD0, HEAD1)
    int active[3];
    float inv_k;
};

struct PoseGradWeights {   // the layers behind trunk layer 0 (the pass loop of pose_grad_mc_kernel)
    const float *w1t, *b1, *h0t, *hb0, *h1t, *hb1, *h2t, *hb2;
};
// keep bits (bit u = unit u kept) of one 64-unit site of this lane's sample at pass k.  Counter mode: the words of
// mc_keep_bits_kernel, made and stepped by the same functions.
template <uint32_t STREAM>
__device__ __forceinline__ void pgmc_keep_bits(const PoseGradMcArgs& m, int site, const uint32_t (&bh)[2], int k, int64_t n,
                                               uint32_t (&bits)[2]) {
    bits[0] = bits[1] = 0xFFFFFFFFu;
    if (!m.active[site]) return;   // uniform
    if (m.explicit_masks) {
        const uint32_t* row = xm_row(m.xm, site, k, n);
        bits[0] = row[0];
        bits[1] = row[1];
        return;
    }
    if (m.keep_all) return;
    uint32_t word[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) word[j] = unerf_mask_word0(bh[(j >> 1) & 1], STREAM, (uint32_t)j);
    for (int q = 0; q < k; ++q) {
#pragma unroll
        for (int j = 0; j < 32; ++j) word[j] = unerf_mask_step(word[j]);
    }
    bits[0] = bits[1] = 0u;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        bits[j >> 4] |= (unerf_keep_lo(word[j], m.keep_hi) ? 1u : 0u) << ((2 * j) & 31);
        bits[j >> 4] |= (unerf_keep_hi(word[j], m.keep_hi) ? 1u : 0u) << ((2 * j + 1) & 31);
    }
}
// ReLU, then the site's dropout: row o <- keep ? max(v, 0) scale : 0
__device__ __forceinline__ void pgmc_store_relu_keep(float* act, int lane, const float (&v)[64], const uint32_t (&keep)[2], float scale) {
#pragma unroll
    for (int o = 0; o < 64; ++o) act[o * 64 + lane] = ((keep[o >> 5] >> (o & 31)) & 1u) ? fmaxf(v[o], 0.f) * scale : 0.f;
}

template <int GRID>
__global__ __launch_bounds__(64) void pose_grad_mc_kernel(PoseGradArgs a, PoseGradMcArgs m) {
    extern __shared__ float lds[];
    const int lane = threadIdx.x;
    float* A = lds;               // the working panel [64 units][64 lanes] of pose_grad_kernel
    float* H0 = lds + 64 * 64;    // relu(layer 0), kept for every pass
    const int64_t r = blockIdx.x;
    if (r >= a.R) return;
    const int S = a.S;
    const bool in = lane < S;
    const int i = in ? lane : S - 1;
    const uint32_t mask = GRID == 0 ? (1u << a.p.log2T) - 1u : 0u;
    const int64_t n = r * S + i;   // this lane's sample in the launch
    // ---- sample position, normalisation ----
    const PgSample s = pg_ray_sample(a.sbins + r * (S + 1), a.origins + r * 3, a.dirs + r * 3, a.s_near, a.s_far, a.lin,
                                     a.box, i);
    const float delta = s.delta, sel = s.sel;

    // ---- once: grid -> layer 0 ----
    // 4 levels unrolled, not the other kernels' 2: one wave per SIMD, so the gathers of four levels in flight; the registers are there
    pg_grid_fwd<GRID, 4>(a, mask, s, A, lane);
    uint32_t m0[2];
    {
        float acc[64];
        pg_dense<32, 64>(pg_const(a.p.w0t), pg_const(a.p.b0), A, lane, acc);
        relu_mask64(acc, m0);
        store_act<64>(H0, lane, acc, 0, true);
    }
    float ux, uy, uz;
    pg_sh_inputs(a, s, ux, uy, uz);
    uint32_t bh[2] = {0u, 0u};
    if (!m.explicit_masks) {
        const uint32_t pre = unerf_mc_pre(m.key, m.sample0 + (uint32_t)n);
        bh[0] = unerf_mc_base_h(pre, 0u);
        bh[1] = unerf_mc_base_h(pre, 1u);
    }
    const bool last_bg = a.bg_mode == UNERF_BG_LAST_SAMPLE;
    float G[64];   // running adjoint of the layer-0 pre-activation, summed over the passes
#pragma unroll
    for (int o = 0; o < 64; ++o) G[o] = 0.f;
    float gdx = 0.f, gdy = 0.f, gdz = 0.f;   // the SH term of ds/dd, summed over the passes
    float rgb_sum[3] = {0.f, 0.f, 0.f};

#pragma unroll 1
    for (int k = 0; k < m.K; ++k) {
        uint32_t kt[2], k0[2], k1[2];
        pgmc_keep_bits<0u>(m, 0, bh, k, n, kt);
        pgmc_keep_bits<2u>(m, 1, bh, k, n, k0);
        pgmc_keep_bits<1u>(m, 2, bh, k, n, k1);
        // The weight pointers pass an empty asm once per pass: as loop invariants the compiler hoists scalar weight loads
        // out of the pass loop and spills them into VGPR lanes (365 spilled SGPRs without this, 249 with it; the rest are
        // the hoisted multiplier constants of the mask words).  Worth 2 % at K = 1 together with the level unrolling.
        PoseGradWeights wp = {a.p.w1t, a.p.b1, a.p.h0t, a.p.hb0, a.p.h1t, a.p.hb1, a.p.h2t, a.p.hb2};
        asm volatile("" : "+s"(wp.w1t), "+s"(wp.b1), "+s"(wp.h0t), "+s"(wp.hb0), "+s"(wp.h1t), "+s"(wp.hb1), "+s"(wp.h2t), "+s"(wp.hb2));
        // ---- forward: dropout on layer 0's activations -> trunk layer 1 -> colour head ----
#pragma unroll 8
        for (int o = 0; o < 64; ++o) A[o * 64 + lane] = ((kt[o >> 5] >> (o & 31)) & 1u) ? H0[o * 64 + lane] * m.scale[0] : 0.f;
        float o1[16];
        pg_dense<64, 16>(pg_const(wp.w1t), pg_const(wp.b1), A, lane, o1);
        const float sig = a.p.average_init_density * expf(o1[0]) * sel;
        {
            float sh[16];
            unerf_sh16(ux, uy, uz, sh);
            store_act<16>(A, lane, sh, 0, false);
        }
#pragma unroll
        for (int g = 0; g < 15; ++g) A[(16 + g) * 64 + lane] = o1[1 + g];
        float acc[64];
        uint32_t m1[2], m2[2];
        pg_dense<31, 64>(pg_const(wp.h0t), pg_const(wp.hb0), A, lane, acc);
        relu_mask64(acc, m1);
        pgmc_store_relu_keep(A, lane, acc, k0, m.scale[1]);
        pg_dense<64, 64>(pg_const(wp.h1t), pg_const(wp.hb1), A, lane, acc);
        relu_mask64(acc, m2);
        pgmc_store_relu_keep(A, lane, acc, k1, m.scale[2]);
        float c[3];
        pg_dense<64, 3>(pg_const(wp.h2t), pg_const(wp.hb2), A, lane, c);
#pragma unroll
        for (int q = 0; q < 3; ++q) c[q] = unerf_nan_to_num(unerf_sigmoid(c[q]));

        // ---- compositing and its adjoints, per pass ----
        const PgWeights cw = pg_transmittance(in, delta, sig, lane);
        const float em = cw.em, T = cw.T, w = cw.w, Tf = cw.Tf, sw = cw.sw;
        float dsig = 0.f, dc[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float bg = last_bg ? __shfl(c[q], S - 1, 64) : a.bg[q];
            const float wc = w * c[q];
            const float swc = pg_suffix_sum(wc, lane);
            const float pred = group_sum<64>(wc) + Tf * bg;
            const float live = (pred >= 0.f && pred <= 1.f && in) ? 1.f / 3.f : 0.f;
            dsig += live * delta * (em * T * (c[q] - bg) - swc + bg * sw);
            const float wt = w + ((last_bg && lane == S - 1) ? Tf : 0.f);
            dc[q] = live * wt * c[q] * (1.f - c[q]);
            rgb_sum[q] += fminf(fmaxf(pred, 0.f), 1.f);
        }

        // ---- backward: colour head (the adjoint of a dropout site is its own factor) ----
        m2[0] &= k1[0]; m2[1] &= k1[1];
        m1[0] &= k0[0]; m1[1] &= k0[1];
        float d[64];
        const pg_cfp h2t = pg_const(wp.h2t);
#pragma unroll
        for (int o = 0; o < 64; ++o) {
            const float v = fmaf(dc[2], h2t[o * 3 + 2], fmaf(dc[1], h2t[o * 3 + 1], dc[0] * h2t[o * 3 + 0]));
            d[o] = ((m2[o >> 5] >> (o & 31)) & 1u) ? v * m.scale[2] : 0.f;
        }
        pg_dense_bwd<64, 64>(pg_const(wp.h1t), d, A, lane);
        load_masked64(A, lane, m1, d);
#pragma unroll
        for (int o = 0; o < 64; ++o) d[o] *= m.scale[1];
        pg_dense_bwd<31, 64>(pg_const(wp.h0t), d, A, lane);   // rows 0..15: dSH, 16..30: dgeo
        {
            float sx, sy, sz;
            pg_sh16_grad(A, lane, ux, uy, uz, a.p.sh_remap, sx, sy, sz);
            gdx += sx;
            gdy += sy;
            gdz += sz;
        }
        // ---- backward: trunk layer 1, down to the layer-0 pre-activation ----
        float d1[16];
        d1[0] = dsig * sig;
#pragma unroll
        for (int g = 0; g < 15; ++g) d1[1 + g] = A[(16 + g) * 64 + lane];
        pg_dense_bwd<64, 16>(pg_const(wp.w1t), d1, A, lane);
        const uint32_t e0m[2] = {m0[0] & kt[0], m0[1] & kt[1]};
#pragma unroll
        for (int o = 0; o < 64; ++o) G[o] += ((e0m[o >> 5] >> (o & 31)) & 1u) ? A[o * 64 + lane] * m.scale[0] : 0.f;
    }

    // ---- once: layer 0 backward, grid -> normalised position ----
    pg_dense_bwd<32, 64>(pg_const(a.p.w0t), G, A, lane);   // rows 2l, 2l+1: adjoint of level l's features
    float gpx, gpy, gpz, gx, gy, gz;
    pg_grid_bwd<GRID, 4>(a, mask, s, A, lane, gpx, gpy, gpz);   // 4 levels unrolled, for the forward loop's reason
    pg_world_grad(a.box, s, gpx, gpy, gpz, gx, gy, gz);
    PgRaySums sums = pg_ray_sums(in, s.t2, gx, gy, gz, gdx, gdy, gdz);
    sums.go0 *= m.inv_k, sums.go1 *= m.inv_k, sums.go2 *= m.inv_k;   // the mean over the passes: on the sums, before the row
    sums.gd0 *= m.inv_k, sums.gd1 *= m.inv_k, sums.gd2 *= m.inv_k;

    // ---- epilogue: every store is a vector store of a lane-selected value ----
    pg_store_grad(a, r, lane, pg_pose_row(a, lane, s.dx, s.dy, s.dz, sums));
    if (a.out_rgb && lane < 3) {
        const float pv = lane == 0 ? rgb_sum[0] : (lane == 1 ? rgb_sum[1] : rgb_sum[2]);
        a.out_rgb[r * 3 + lane] = pv * m.inv_k;
    }
}

extern "C" int unerf_pose_grad_mc(const float* origins, const float* directions, const float* sbins, int64_t R, int S,
                                  float near_plane, float far_plane, int spacing, int64_t ray_offset, const unerf_field_params* p,
                                  const unerf_keep_masks* masks, int background, const float* background_rgb,
                                  const float* rot_inv, float* out_grad, float* out_rgb, void* stream) {
    if (int rc = pose_check_samples("pose_grad_mc", R, S)) return rc;
    if (R == 0) return UNERF_OK;
    if (int rc = pose_check_pointers("pose_grad_mc", origins, directions, sbins, p, out_grad != nullptr)) return rc;
    UNERF_REQUIRE(p->mode == UNERF_FIELD_MCDROPOUT, "pose_grad_mc: mode %d (an MCDROPOUT field is needed; unerf_pose_grad differentiates "
                  "the deterministic fields, the Laplace field's sampled heads are not differentiated)", p->mode);
    UNERF_REQUIRE(p->K >= 1, "pose_grad_mc: K=%d, the mean over passes needs K >= 1", p->K);
    UNERF_REQUIRE(p->p_drop >= 0.f && p->p_drop < 1.f, "pose_grad_mc: bad p_drop=%g", (double)p->p_drop);
    UNERF_REQUIRE((p->drop_sites & ~DROP_SITES_KNOWN) == 0, "pose_grad_mc: unknown bits in drop_sites=%d", p->drop_sites);
    UNERF_REQUIRE(!(p->drop_sites & UNERF_DROP_HEADIN), "pose_grad_mc: UNERF_DROP_HEADIN is out of scope (not built)");
    if (int rc = pose_check_field("pose_grad_mc", p, near_plane, 16, false, "; the any-width kernel is out of scope")) return rc;
    const int sites = requested_drop_sites(*p);
    PoseGradMcArgs m;
    m.explicit_masks = masks ? 1 : 0;
    m.K = p->K;
    m.inv_k = 1.f / (float)p->K;
    const float scale = 1.f / (1.f - p->p_drop);
    for (int i = 0; i < 3; ++i) {
        m.active[i] = (sites >> i) & 1;
        m.scale[i] = m.active[i] ? scale : 1.f;
        m.xm.site[i] = NULL;
    }
    m.xm.pass_stride = 0;
    m.xm.sample_offset = 0;
    m.keep_all = 0; m.keep_hi = 0; m.key = 0u; m.sample0 = 0u;
    if (masks) {
        static const char* const names[4] = {"TRUNK", "HEAD0", "HEAD1", "HEADIN"};
        for (int i = 0; i < 4; ++i) {
            UNERF_REQUIRE(!((sites >> i) & 1) || masks->site[i], "pose_grad_mc: site %s is active (drop_sites=%d) but its mask array is NULL", names[i], sites);
            UNERF_REQUIRE(((sites >> i) & 1) || !masks->site[i], "pose_grad_mc: a mask array for site %s, which is not active (drop_sites=%d)", names[i], sites);
        }
        UNERF_REQUIRE(masks->sample_offset >= 0 && masks->pass_stride >= masks->sample_offset + R * (int64_t)S,
                      "pose_grad_mc: pass_stride=%lld < sample_offset + R*S = %lld + %lld", (long long)masks->pass_stride,
                      (long long)masks->sample_offset, (long long)(R * (int64_t)S));
        for (int i = 0; i < 3; ++i) m.xm.site[i] = masks->site[i];
        m.xm.pass_stride = masks->pass_stride;
        m.xm.sample_offset = masks->sample_offset;
    } else {   // the counter generator: threshold and key as unerf_field_fwd / unerf_mc_keep_bits make them
        UNERF_REQUIRE(ray_offset >= 0 && (uint64_t)(ray_offset + R) * (uint64_t)S < (1ull << 32),
                      "pose_grad_mc: sample index exceeds 32 bits (RNG counter)");
        const long thr = lrint((1.0 - (double)p->p_drop) * 65536.0);
        const int32_t thr_s = (int32_t)(thr < 65536 ? thr : 65535) - 32768;
        m.keep_hi = (int32_t)((uint32_t)thr_s << 16);
        m.keep_all = thr >= 65536 ? 1 : 0;
        m.key = unerf_mc_key(p->seed, 0u);
        m.sample0 = (uint32_t)((uint64_t)ray_offset * (uint64_t)S);
    }
    PoseGradArgs g;   // a block per ray: the grid's x is R, hence 2^31
    if (int rc = pose_fill_args(g, "pose_grad_mc", origins, directions, sbins, R, S, near_plane, far_plane, spacing, p, background,
                                background_rgb, rot_inv, out_grad, out_rgb, 1ll << 31)) return rc;
    constexpr size_t lds_bytes = 2 * 64 * 64 * sizeof(float);   // the working panel and layer 0's activations
    with_int3(tcnn_arg(g.p), [&](auto tc) {
        hipLaunchKernelGGL((pose_grad_mc_kernel<decltype(tc)::value>), dim3((unsigned)R), dim3(64), lds_bytes, (hipStream_t)stream, g, m);
    });
    return unerf_check_launch("pose_grad_mc");
}

// --------------------------------------------------------------------------------------
// 5e''. The same gradient of a LAPLACE frame under a named draw of the last layers (laplace_field.py:279-362, 365-485,
// 528-568; laplace_model.py:456-480): the rows ws_density [set][q][65] / ws_rgb [set][q][195] are ordinary tensors, so the
// colour is a deterministic piecewise-smooth function of the pose.  Per sample:
//   hb = W0 feat + b0 (no ReLU), geo = W1 hb + b1 (no ReLU),
//   mu_d = (1/n) sum_q act(w_q . hb + b_q)  (act = exp | softplus; x selector only with lap_mask_density),
//   h = relu(H1 relu(H0 [SH16 | geo] + hb0) + hb1),  mu_c = (1/n_rgb) sum_q sigmoid(Wc_q h + bc_q),
// composited with the weights of mu_d.  pose_grad_kernel's geometry is kept (a wave per ray, a lane per sample, one 16-KiB
// panel per wave, two waves per SIMD); a wave has one ray, hence one sample set, so every head row is wave-uniform and is
// read through the constant address space into scalar operands.
//   forward   density rows: mu_d and, in the same pass, J = sum_q act'(pre_q) w_q (64 registers, carried to the trunk
//             backward: d mu_d / d hb = J / n, which spares a second pass over the density rows and the recomputation of hb);
//             colour rows: mu_c from h in registers and, in the same pass, D = sum_q sum_c s (1 - s) Wc_q[c,:] (64 registers)
//   adjoints  pose_grad_kernel's scans give d mu_d and d mu_c
//   backward  dh = d mu_c D / n_rgb when the three clamp gates of the ray are open (the channel adjoints are then equal; always,
//             up to rounding, for a background in [0, 1]); else pass 2 over the colour rows: pre_qc recomputed from h,
//             dh += d mu_c[c] s (1 - s) / n_rgb Wc_q[c,:].  ReLU, H1^T, ReLU, H0^T -> (dSH, dgeo); dhb = d mu_d J / n + W1^T dgeo;
//             W0^T (no mask) -> dfeat; grid, contraction and ray sums as pose_grad_kernel.
// The heads are summed in row order q = 0 .. n-1; no global scratch, no atomics.
// --------------------------------------------------------------------------------------
struct PoseGradLapArgs {
    int64_t ray_offset;   // ray r of the launch is ray ray_offset + r of the frame: its set is that / lap_chunk_rays
    int n_rgb;            // rows of ws_rgb per set (n_lap_rgb, or n_lap when that is <= 0)
};

template <int GRID>
__global__ __launch_bounds__(256, 2) void pose_grad_laplace_kernel(PoseGradArgs a, PoseGradLapArgs la) {
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* A = lds + wv * (64 * 64);   // this wave's panel [64 units][64 lanes]; a lane reads only its own column
    const int64_t r = (int64_t)blockIdx.x * 4 + wv;
    if (r >= a.R) return;   // wave-uniform
    const int S = a.S;
    const bool in = lane < S;
    const int i = in ? lane : S - 1;
    const uint32_t mask = GRID == 0 ? (1u << a.p.log2T) - 1u : 0u;
    const int nl = a.p.n_lap, nr = la.n_rgb;
    const size_t set = a.p.lap_chunk_rays > 0 ? (size_t)((la.ray_offset + r) / a.p.lap_chunk_rays) : 0;   // wave-uniform
    const pg_cfp wd = pg_const(a.p.ws_density) + set * (size_t)nl * 65;
    const pg_cfp wc = pg_const(a.p.ws_rgb) + set * (size_t)nr * 195;

    // ---- sample position, normalisation: pg_ray_sample's statements, and below pg_sh_inputs' and pg_transmittance's with
    // pg_suffix_sum's, IN LINE in this kernel alone.  With the four as calls the metadata is the parent's too (256 VGPRs, 109
    // spilled, 440 B), but the listing is 8 to 58 instructions longer and the kernel 4 % slower at 100 sampled rows (11.65 ->
    // 12.18 ms per 200 x 200 frame, 586 -> 611 ms at 1080p: the register allocation of the row loops moves); in line it has the
    // time it had (docs/experiments.md 8.6).  Keep them in step with the functions.
    const float* sb = a.sbins + r * (S + 1);
    const float e0 = unerf_s2e(sb[i], a.s_near, a.s_far, a.lin), e1 = unerf_s2e(sb[i + 1], a.s_near, a.s_far, a.lin);
    const float delta = e1 - e0, t2 = e0 + e1;
    const float ox = a.origins[r * 3 + 0], oy = a.origins[r * 3 + 1], oz = a.origins[r * 3 + 2];
    const float dxr = a.dirs[r * 3 + 0], dyr = a.dirs[r * 3 + 1], dzr = a.dirs[r * 3 + 2];
    const float x0 = ox + dxr * t2 / 2.f, y0 = oy + dyr * t2 / 2.f, z0 = oz + dzr * t2 / 2.f;
    float px = x0, py = y0, pz = z0;
    const float sel = unerf_normalize_position(px, py, pz, a.box);
    PgSample s;   // for the shared stages below
    s.delta = delta, s.t2 = t2, s.dx = dxr, s.dy = dyr, s.dz = dzr;
    s.x0 = x0, s.y0 = y0, s.z0 = z0, s.px = px, s.py = py, s.pz = pz, s.sel = sel;

    // ---- forward: grid -> bare-Linear trunk (field_kernel's LAPLACE arithmetic) ----
    pg_grid_fwd<GRID, 2>(a, mask, s, A, lane);
    float acc[64];
    pg_dense<32, 64>(pg_const(a.p.w0t), pg_const(a.p.b0), A, lane, acc);
    store_act<64>(A, lane, acc, 0, false);
    float geo[15];
    pg_dense<64, 15>(pg_const(a.p.w1t), pg_const(a.p.b1), A, lane, geo);

    // ---- density rows: the mean and its Jacobian with respect to hb in one pass ----
    float J[64];
#pragma unroll
    for (int o = 0; o < 64; ++o) J[o] = 0.f;
    float mu = 0.f;
    for (int q = 0; q < nl; ++q) {
        const pg_cfp w = wd + (size_t)q * 65;
        float pre = 0.f;
#pragma unroll
        for (int o = 0; o < 64; ++o) pre = fmaf(acc[o], w[o], pre);
        pre += w[64];
        float pred, dact;
        if (a.p.lap_softplus) {   // uniform
            pred = unerf_softplus(pre);
            dact = unerf_sigmoid(pre);   // = 1 - exp(-pred)
        } else {
            pred = expf(pre);
            dact = pred;
        }
        mu += pred;
#pragma unroll
        for (int o = 0; o < 64; ++o) J[o] = fmaf(dact, w[o], J[o]);
    }
    mu /= (float)nl;
    const float dsel = a.p.lap_mask_density ? sel : 1.f;   // inference: NOT selector-masked (laplace_field.py:356-362)
    const float sig = mu * dsel;

    // ---- colour head; rows, pass 1: the mean colour ----
    float ux = (dxr + 1.f) / 2.f, uy = (dyr + 1.f) / 2.f, uz = (dzr + 1.f) / 2.f;
    if (a.p.sh_remap) {
        ux = ux * 2.f - 1.f;
        uy = uy * 2.f - 1.f;
        uz = uz * 2.f - 1.f;
    }
    {
        float sh[16];
        unerf_sh16(ux, uy, uz, sh);
        store_act<16>(A, lane, sh, 0, false);
    }
    store_act<15>(A, lane, geo, 16, false);
    uint32_t m1[2];
    pg_dense<31, 64>(pg_const(a.p.h0t), pg_const(a.p.hb0), A, lane, acc);
    relu_mask64(acc, m1);
    store_act<64>(A, lane, acc, 0, true);
    pg_dense<64, 64>(pg_const(a.p.h1t), pg_const(a.p.hb1), A, lane, acc);
#pragma unroll
    for (int o = 0; o < 64; ++o) acc[o] = fmaxf(acc[o], 0.f);   // h, kept in registers over both passes
    // D = sum_q sum_c s_qc (1 - s_qc) Wc_q[c,:]: the adjoint of h for EQUAL channel adjoints, which is what the compositing
    // hands back whenever all three clamp gates of the ray are open (pred = sum w c + T bg lies in [0, 1] for any colour mean
    // and a background in [0, 1], up to rounding) -- then no second pass over the colour rows is needed
    float c[3] = {0.f, 0.f, 0.f};
    float d[64];
#pragma unroll
    for (int o = 0; o < 64; ++o) d[o] = 0.f;
    for (int q = 0; q < nr; ++q) {
        const pg_cfp w = wc + (size_t)q * 195;
        float g[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float pre = 0.f;
#pragma unroll
            for (int o = 0; o < 64; ++o) pre = fmaf(acc[o], w[k * 64 + o], pre);
            const float s = unerf_sigmoid(pre + w[192 + k]);
            c[k] += s;
            g[k] = s * (1.f - s);
        }
#pragma unroll
        for (int o = 0; o < 64; ++o) d[o] = fmaf(g[2], w[128 + o], fmaf(g[1], w[64 + o], fmaf(g[0], w[o], d[o])));
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = unerf_nan_to_num(c[k] / (float)nr);

    // ---- compositing and its adjoints (pg_transmittance and pg_suffix_sum in line: see the prologue) ----
    const float dd = in ? delta * sig : 0.f;
    const float em = expf(-dd);
    const float T = expf(-group_excl_scan<64>(dd, lane));
    const float wgt = in ? unerf_nan_to_num((1.f - em) * T) : 0.f;
    const float Tf = 1.f - group_sum<64>(wgt);
    const bool last_bg = a.bg_mode == UNERF_BG_LAST_SAMPLE;
    const int rl = 63 - lane;
    const float sw = __shfl(group_excl_scan<64>(__shfl(wgt, rl, 64), lane), rl, 64);
    float dsig = 0.f, dc[3], pred[3];
    bool gates_open = true;   // wave-uniform: pred is the ray's
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float bg = last_bg ? __shfl(c[k], S - 1, 64) : a.bg[k];
        const float wck = wgt * c[k];
        const float swc = __shfl(group_excl_scan<64>(__shfl(wck, rl, 64), lane), rl, 64);
        pred[k] = group_sum<64>(wck) + Tf * bg;
        gates_open = gates_open && pred[k] >= 0.f && pred[k] <= 1.f;
        const float live = (pred[k] >= 0.f && pred[k] <= 1.f && in) ? 1.f / 3.f : 0.f;
        dsig += live * delta * (em * T * (c[k] - bg) - swc + bg * sw);
        const float wt = wgt + ((last_bg && lane == S - 1) ? Tf : 0.f);
        dc[k] = live * wt / (float)nr;   // adjoint of every row's sigmoid output
    }

    // ---- the adjoint of h: dc D with all gates open (dc[0] = dc[1] = dc[2]); else pass 2 over the colour rows, pre_qc
    // recomputed from h and every channel with its own adjoint ----
    if (gates_open) {
#pragma unroll
        for (int o = 0; o < 64; ++o) d[o] *= dc[0];
    } else {
#pragma unroll
        for (int o = 0; o < 64; ++o) d[o] = 0.f;
        for (int q = 0; q < nr; ++q) {
            const pg_cfp w = wc + (size_t)q * 195;
            float g[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float pre = 0.f;
#pragma unroll
                for (int o = 0; o < 64; ++o) pre = fmaf(acc[o], w[k * 64 + o], pre);
                const float s = unerf_sigmoid(pre + w[192 + k]);
                g[k] = dc[k] * s * (1.f - s);
            }
#pragma unroll
            for (int o = 0; o < 64; ++o) d[o] = fmaf(g[2], w[128 + o], fmaf(g[1], w[64 + o], fmaf(g[0], w[o], d[o])));
        }
    }
#pragma unroll
    for (int o = 0; o < 64; ++o) d[o] = acc[o] > 0.f ? d[o] : 0.f;
    pg_dense_bwd<64, 64>(pg_const(a.p.h1t), d, A, lane);
    load_masked64(A, lane, m1, d);
    pg_dense_bwd<31, 64>(pg_const(a.p.h0t), d, A, lane);   // rows 0..15: dSH, 16..30: dgeo
    float gdx, gdy, gdz;   // the SH term of ds/dd
    pg_sh16_grad(A, lane, ux, uy, uz, a.p.sh_remap, gdx, gdy, gdz);
    // ---- backward: trunk (no ReLU: no masks) ----
    float d1[15];
#pragma unroll
    for (int g = 0; g < 15; ++g) d1[g] = A[(16 + g) * 64 + lane];
    pg_dense_bwd<64, 15>(pg_const(a.p.w1t), d1, A, lane);
    const float dmu = dsig * dsel / (float)nl;
#pragma unroll
    for (int o = 0; o < 64; ++o) d[o] = fmaf(dmu, J[o], A[o * 64 + lane]);
    pg_dense_bwd<32, 64>(pg_const(a.p.w0t), d, A, lane);   // rows 2l, 2l+1: adjoint of level l's features

    // ---- backward: grid -> normalised position -> world position, ray sums, epilogue ----
    float gpx, gpy, gpz, gx, gy, gz;
    pg_grid_bwd<GRID, 2>(a, mask, s, A, lane, gpx, gpy, gpz);
    pg_world_grad(a.box, s, gpx, gpy, gpz, gx, gy, gz);
    const PgRaySums sums = pg_ray_sums(in, s.t2, gx, gy, gz, gdx, gdy, gdz);
    pg_store_grad(a, r, lane, pg_pose_row(a, lane, s.dx, s.dy, s.dz, sums));
    if (a.out_rgb && lane < 3) {
        const float pv = lane == 0 ? pred[0] : (lane == 1 ? pred[1] : pred[2]);
        a.out_rgb[r * 3 + lane] = fminf(fmaxf(pv, 0.f), 1.f);
    }
}

extern "C" int unerf_pose_grad_laplace(const float* origins, const float* directions, const float* sbins, int64_t R, int S,
                                       float near_plane, float far_plane, int spacing, int64_t ray_offset,
                                       const unerf_field_params* p, int background, const float* background_rgb,
                                       const float* rot_inv, float* out_grad, float* out_rgb, void* stream) {
    if (int rc = pose_check_samples("pose_grad_laplace", R, S)) return rc;
    if (R == 0) return UNERF_OK;
    if (int rc = pose_check_pointers("pose_grad_laplace", origins, directions, sbins, p, out_grad != nullptr)) return rc;
    UNERF_REQUIRE(p->mode == UNERF_FIELD_LAPLACE, "pose_grad_laplace: mode %d (a LAPLACE field is needed; unerf_pose_grad and "
                  "unerf_pose_grad_mc differentiate the other fields)", p->mode);
    if (int rc = pose_check_field("pose_grad_laplace", p, near_plane, 15, true, "; the any-width kernel is out of scope")) return rc;
    UNERF_REQUIRE(p->n_lap >= 1, "pose_grad_laplace: n_lap=%d, the mean over sampled rows needs n_lap >= 1", p->n_lap);
    UNERF_REQUIRE(ray_offset >= 0, "pose_grad_laplace: ray_offset=%lld < 0", (long long)ray_offset);
    UNERF_REQUIRE(p->lap_chunk_rays >= 0, "pose_grad_laplace: lap_chunk_rays=%d < 0", p->lap_chunk_rays);
    UNERF_REQUIRE(p->lap_chunk_rays == 0 || (ray_offset + R - 1) / p->lap_chunk_rays < p->lap_sets,
                  "pose_grad_laplace: rays [%lld, %lld) reach past the last of lap_sets=%d sample sets of lap_chunk_rays=%d rays",
                  (long long)ray_offset, (long long)(ray_offset + R), p->lap_sets, p->lap_chunk_rays);
    PoseGradArgs g;
    if (int rc = pose_fill_args(g, "pose_grad_laplace", origins, directions, sbins, R, S, near_plane, far_plane, spacing, p,
                                background, background_rgb, rot_inv, out_grad, out_rgb, 1ll << 32)) return rc;
    PoseGradLapArgs la;
    la.ray_offset = ray_offset;
    la.n_rgb = p->n_lap_rgb > 0 ? p->n_lap_rgb : p->n_lap;
    with_int3(tcnn_arg(g.p), [&](auto tc) { pose_launch_rays4(pose_grad_laplace_kernel<decltype(tc)::value>, R, stream, g, la); });
    return unerf_check_launch("pose_grad_laplace");
}

// ======================================================================================
// 6. per-ray groups of 16 lanes x SPL samples: get_weights, composite, laplace depth draws
// ======================================================================================
template <int SPL>
__device__ __forceinline__ void group_weights(const float (&dens)[SPL], const float (&delta)[SPL], int l16,
                                              float (&w)[SPL]) {
    float dd[SPL], lex[SPL], ls = 0.f;
#pragma unroll
    for (int e = 0; e < SPL; ++e) {
        dd[e] = delta[e] * dens[e];
        lex[e] = ls;
        ls += dd[e];
    }
    float carry = group_excl_scan<16>(ls, l16);
#pragma unroll
    for (int e = 0; e < SPL; ++e) {
        float alpha = 1.f - unerf_exp(-dd[e]);
        float T = unerf_exp(-(carry + lex[e]));
        w[e] = unerf_nan_to_num(alpha * T);
    }
}

struct CompArgs {
    const float* density;
    const float* rgb;
    const float* beta;
    const float* walt;
    const float* sbins;
    int B;
    int64_t R;
    int S;
    float s_near, s_far;
    int lin;   // UNERF_SPACING_*: 1 = identity spacing (UniformSampler)
    const float* clip;
    int64_t ray_offset, chunk_rays;
    float* out;
    int bg_mode;      // UNERF_BG_*: what RGBRenderer blends behind the samples
    float bg[3];      // UNERF_BG_COLOR
    int32_t* flag;    // nonfinite_flag (may be null): |= 1 when a density or colour read here is NaN
};

// one (pass b, ray r) composite, executed by a 16-lane group; g = b*R + r.  Results are replicated on all 16 lanes.
// RAGGED: S is not a multiple of 16 (SPL = ceil(S / 16)); the slots k >= S of the last lanes are masked: their bin
// edges collapse onto edge S (delta = 0), density and weight are 0, and they are excluded from the median count
// and from the "last sample" background colour.  The aligned instantiations are unchanged.
// The pass-independent part of a ray's composite: this lane's bin widths and mid-points (SPL + 1 spacing->Euclidean
// conversions, one IEEE division each).  The K-pass kernel computes it once per ray, not once per pass.
template <int SPL>
struct CompGeom {
    float delta[SPL], steps[SPL];
};
template <int SPL, bool RAGGED>
__device__ __forceinline__ CompGeom<SPL> composite_geom(const CompArgs& a, int64_t r, int l16) {
    const int S = a.S, k0 = l16 * SPL;
    const float* sb = a.sbins + r * (S + 1);
    float eu[SPL + 1];
    CompGeom<SPL> gm;
#pragma unroll
    for (int e = 0; e <= SPL; ++e) eu[e] = unerf_s2e(sb[RAGGED ? min(k0 + e, S) : k0 + e], a.s_near, a.s_far, a.lin);
#pragma unroll
    for (int e = 0; e < SPL; ++e) {
        gm.delta[e] = eu[e + 1] - eu[e];
        gm.steps[e] = (eu[e] + eu[e + 1]) / 2.f;
    }
    return gm;
}

template <int SPL, bool RAGGED = false, bool PACKED = false, typename... VW>   // VW = ViewMap: clip rows numbered per view
__device__ __forceinline__ void composite_one(const CompArgs& a, int64_t g, int64_t r, int l16, float (&o8)[8],
                                              const CompGeom<SPL>& gm, const VW&... vw) {
    const int S = a.S, k0 = l16 * SPL;
    float delta[SPL], steps[SPL], dens[SPL], w[SPL];
    struct Rgb { float r, g, b; };
    Rgb col[SPL];
#pragma unroll
    for (int e = 0; e < SPL; ++e) {
        delta[e] = gm.delta[e];
        steps[e] = gm.steps[e];
    }
    if (PACKED) {   // packed rows (sigma, r, g, b) [B,R,S,4] (unerf_field_params.packed_out): one 16-byte load per sample
        // (a compile-time switch: with both layouts in one kernel the K-pass form needs 72 registers instead of 59)
#pragma unroll
        for (int e = 0; e < SPL; ++e) {
            const float4 v = (!RAGGED || k0 + e < S) ? reinterpret_cast<const float4*>(a.rgb)[g * S + k0 + e]
                                                     : make_float4(0.f, 0.f, 0.f, 0.f);
            dens[e] = v.x;
            col[e] = Rgb{v.y, v.z, v.w};
        }
    } else {
#pragma unroll
        for (int e = 0; e < SPL; ++e) dens[e] = (!RAGGED || k0 + e < S) ? a.density[g * S + k0 + e] : 0.f;
        // colours requested with the densities, one 12-byte load per sample (the three channels as separate dword
        // loads tripled the texture-unit work of this kernel), and consumed after the scan
#pragma unroll
        for (int e = 0; e < SPL; ++e)
            col[e] = (!RAGGED || k0 + e < S) ? reinterpret_cast<const Rgb*>(a.rgb)[g * S + k0 + e] : Rgb{0.f, 0.f, 0.f};
    }
    if (a.flag) {   // uniform.  NaN inputs: the signature of an f16 operand overflow in the field kernel (|x| >= 65504 ->
        // hi = inf, lo = -inf -> NaN), which the nan_to_num calls below would otherwise turn into a plausible pixel.
        // One ballot per wave, one atomic per OFFENDING wave.
        bool bad = false;
#pragma unroll
        for (int e = 0; e < SPL; ++e)
            bad |= (dens[e] != dens[e]) | (col[e].r != col[e].r) | (col[e].g != col[e].g) | (col[e].b != col[e].b);
        const uint64_t m = __builtin_amdgcn_ballot_w64(bad);
        if (m != 0 && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(m)) atomicOr(a.flag, 1);
    }
    group_weights<SPL>(dens, delta, l16, w);

    float cr = 0.f, cg = 0.f, cb = 0.f, accw = 0.f, uvar = 0.f, lr = 0.f, lg = 0.f, lb = 0.f;
#pragma unroll
    for (int e = 0; e < SPL; ++e) {
        if (RAGGED && k0 + e >= S) continue;
        float r0 = unerf_nan_to_num(col[e].r), g0 = unerf_nan_to_num(col[e].g), b0 = unerf_nan_to_num(col[e].b);
        cr += w[e] * r0;
        cg += w[e] * g0;
        cb += w[e] * b0;
        accw += w[e];
        if (a.beta) uvar += (w[e] * w[e]) * a.beta[r * S + k0 + e];
        lr = r0; lg = g0; lb = b0;  // after the loop: this lane's last (real) sample
    }
    cr = group_sum<16>(cr);
    cg = group_sum<16>(cg);
    cb = group_sum<16>(cb);
    accw = group_sum<16>(accw);
    uvar = group_sum<16>(uvar);
    if (a.bg_mode == UNERF_BG_LAST_SAMPLE) {   // uniform; background_color = "last_sample", the nerfacto default
        const int last_lane = RAGGED ? (S - 1) / SPL : 15;   // the lane that holds sample S-1
        float bgr = __shfl(lr, last_lane, 16), bgg = __shfl(lg, last_lane, 16), bgb = __shfl(lb, last_lane, 16);
        cr = cr + bgr * (1.f - accw);
        cg = cg + bgg * (1.f - accw);
        cb = cb + bgb * (1.f - accw);
    } else if (a.bg_mode == UNERF_BG_COLOR) {  // "white" / "black"
        cr = cr + a.bg[0] * (1.f - accw);
        cg = cg + a.bg[1] * (1.f - accw);
        cb = cb + a.bg[2] * (1.f - accw);
    }                                          // UNERF_BG_NONE ("random" at eval): no blending
    cr = fminf(fmaxf(cr, 0.f), 1.f);
    cg = fminf(fmaxf(cg, 0.f), 1.f);
    cb = fminf(fmaxf(cb, 0.f), 1.f);

    // depth-side weights: the laplace mean sampled weights when given
    float wd[SPL];
#pragma unroll
    for (int e = 0; e < SPL; ++e)
        wd[e] = (RAGGED && k0 + e >= S) ? 0.f : (a.walt ? a.walt[r * S + k0 + e] : w[e]);
    float ls = 0.f, lc[SPL], wt = 0.f;
#pragma unroll
    for (int e = 0; e < SPL; ++e) {
        ls += wd[e];
        lc[e] = ls;
        wt += wd[e] * steps[e];
    }
    float tot = group_incl_scan<16>(ls, l16);
    float cbase = dpp_f<0x111>(tot);   // row_shr:1, lane 0 of the group reads 0
    float acc = __shfl(tot, 15, 16);
    wt = group_sum<16>(wt);
    int cnt = 0;
#pragma unroll
    for (int e = 0; e < SPL; ++e) cnt += ((!RAGGED || k0 + e < S) && (cbase + lc[e]) < 0.5f) ? 1 : 0;
    cnt = group_sum_i<16>(cnt);
    int idx = min(cnt, S - 1);
    int owner = idx / SPL, slot = idx - owner * SPL;
    float depth = 0.f;
#pragma unroll
    for (int e = 0; e < SPL; ++e) {
        float got = __shfl(steps[e], owner, 16);
        if (e == slot) depth = got;
    }
    float dv = 0.f;
#pragma unroll
    for (int e = 0; e < SPL; ++e) {
        float df = steps[e] - depth;
        dv += wd[e] * (df * df);
    }
    dv = group_sum<16>(dv) + 1e-5f;
    float ed = wt / (acc + 1e-10f);
    if (a.clip) {
        int64_t chunk = clip_chunk(a, r, vw...);
        ed = fminf(fmaxf(ed, a.clip[chunk * 2 + 0]), a.clip[chunk * 2 + 1]);
    }
    o8[0] = cr; o8[1] = cg; o8[2] = cb; o8[3] = acc;
    o8[4] = depth; o8[5] = ed; o8[6] = uvar; o8[7] = dv;
}

template <int SPL, bool RAGGED, bool PACKED, typename... VW>
__device__ __forceinline__ void composite_kernel_body(const CompArgs& a, const VW&... vw) {
    const int l16 = threadIdx.x & 15;
    int64_t g = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int64_t G = (int64_t)a.B * a.R;
    const bool ok = g < G;
    if (!ok) g = G - 1;
    float o8[8];
    const int64_t r = g % a.R;
    composite_one<SPL, RAGGED, PACKED>(a, g, r, l16, o8, composite_geom<SPL, RAGGED>(a, r, l16), vw...);
    if (ok && l16 == 0) {
        float4* o = reinterpret_cast<float4*>(a.out + g * 8);
        o[0] = make_float4(o8[0], o8[1], o8[2], o8[3]);
        o[1] = make_float4(o8[4], o8[5], o8[6], o8[7]);
    }
}
// (a wrapper: with the body itself as the kernel some instantiations compile to other code, docs/experiments.md 8.3)
template <int SPL, bool RAGGED, bool PACKED, typename... VW>   // VW = ViewMap: unerf_composite_var_views with a clip buffer
__global__ __launch_bounds__(256) void composite_kernel(CompArgs a, VW... vw) {
    composite_kernel_body<SPL, RAGGED, PACKED>(a, vw...);
}

// K-pass form: one 16-lane group walks the B <= 16 passes of a ray, lane b keeps pass b's eight
// outputs, and the per-pixel mean and unbiased variance over the passes (two-pass, like
// torch.stack(...).mean(0) / .var(0), mcdropout_models.py:121-126) come out of two group reductions:
// the [B,R,8] per-pass images never touch HBM.  Both passes run on x_b - x_0 (pass 0's value, as the planes
// kernel's shifted sums do): the mean of B equal values is then that value and their variance 0 exactly, where
// sum(x) * (1 / B) rounds the mean off x and left a variance of a few ulp(x)^2.
template <int SPL, bool RAGGED, bool PACKED, typename... VW>
__device__ __forceinline__ void composite_moments_body(const CompArgs& a, float* __restrict__ mean_out,
                                                       float* __restrict__ var_out, const VW&... vw) {
    const int l16 = threadIdx.x & 15;
    int64_t r = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool ok = r < a.R;
    if (!ok) r = a.R - 1;
    float mine[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) mine[c] = 0.f;
    const CompGeom<SPL> gm = composite_geom<SPL, RAGGED>(a, r, l16);   // bin edges are the same in every pass
    for (int b = 0; b < a.B; ++b) {
        float o8[8];
        composite_one<SPL, RAGGED, PACKED>(a, (int64_t)b * a.R + r, r, l16, o8, gm, vw...);
        if (l16 == b) {
#pragma unroll
            for (int c = 0; c < 8; ++c) mine[c] = o8[c];
        }
    }
    const float invB = 1.f / (float)a.B, invB1 = 1.f / (float)(a.B - 1);
    float m8[8], v8[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float x0 = __shfl(mine[c], 0, 16);
        const float d = (l16 < a.B) ? mine[c] - x0 : 0.f;
        const float dm = group_sum<16>(d) * invB;
        m8[c] = x0 + dm;
        const float dev = (l16 < a.B) ? d - dm : 0.f;
        v8[c] = group_sum<16>(dev * dev) * invB1;
    }
    if (ok && l16 == 0) {
        float4* mo = reinterpret_cast<float4*>(mean_out + r * 8);
        float4* vo = reinterpret_cast<float4*>(var_out + r * 8);
        mo[0] = make_float4(m8[0], m8[1], m8[2], m8[3]);
        mo[1] = make_float4(m8[4], m8[5], m8[6], m8[7]);
        vo[0] = make_float4(v8[0], v8[1], v8[2], v8[3]);
        vo[1] = make_float4(v8[4], v8[5], v8[6], v8[7]);
    }
}
template <int SPL, bool RAGGED, bool PACKED, typename... VW>   // VW = ViewMap: unerf_composite_moments_views with a clip buffer
__global__ __launch_bounds__(256) void composite_moments_kernel(CompArgs a, float* __restrict__ mean_out,
                                                                float* __restrict__ var_out, VW... vw) {
    composite_moments_body<SPL, RAGGED, PACKED>(a, mean_out, var_out, vw...);
}

// views = NULL: unerf_composite_var
static int composite_var_impl(const float* density, const float* rgb, const float* beta, const float* weights_alt,
                              const float* sbins, int B, int64_t R, int S, float near_plane, float far_plane, int spacing,
                              const float* clip_minmax, int64_t ray_offset, int64_t chunk_rays, int background,
                              const float* background_rgb, int32_t* nonfinite_flag, float* out, const unerf_ray_views* views,
                              void* stream) {
    UNERF_REQUIRE(R == 0 || (rgb && sbins && out), "composite_var: null pointer");   // density NULL: rgb holds packed rows
    UNERF_REQUIRE(B >= 1 && R >= 0, "composite_var: bad B/R");
    UNERF_REQUIRE(S >= 1 && S <= 256, "composite_var: S=%d outside [1,256]", S);
    UNERF_REQUIRE(!clip_minmax || chunk_rays > 0, "composite_var: chunk_rays must be > 0 with clip_minmax");
    if (R == 0) return UNERF_OK;
    CompArgs a;
    a.density = density; a.rgb = rgb; a.beta = beta; a.walt = weights_alt; a.sbins = sbins; a.B = B; a.R = R; a.S = S;
    if (int rc = set_spacing(a, near_plane, far_plane, spacing)) return rc;
    a.clip = clip_minmax; a.ray_offset = ray_offset; a.chunk_rays = chunk_rays; a.out = out;
    if (int rc = unerf_set_background(a, background, background_rgb, "composite_var")) return rc;
    a.flag = nonfinite_flag;
    dim3 grid(blocks_for((int64_t)B * R, 16)), block(256);
    hipStream_t st = (hipStream_t)stream;
    // composite_kernel<SPL, RAGGED, PACKED, VW...>; per-view clip rows only where there is a clip buffer (without one
    // nothing in the kernel is numbered by the frame)
    const bool per_view = views && clip_minmax;
    with_pack(per_view, [&] { return make_view_map(views, chunk_rays); }, [&](auto... vm) {
        with_spl(S, [&](auto spl, auto ragged) {
            with_bool(density == nullptr, [&](auto packed) {
                hipLaunchKernelGGL((composite_kernel<decltype(spl)::value, decltype(ragged)::value, decltype(packed)::value, decltype(vm)...>),
                                   grid, block, 0, st, a, vm...);
            });
        });
    });
    return unerf_check_launch(per_view ? "composite_var_views" : "composite_var");
}

extern "C" int unerf_composite_var(const float* density, const float* rgb, const float* beta, const float* weights_alt,
                                   const float* sbins, int B, int64_t R, int S, float near_plane, float far_plane, int spacing,
                                   const float* clip_minmax, int64_t ray_offset, int64_t chunk_rays, int background,
                                   const float* background_rgb, int32_t* nonfinite_flag, float* out, void* stream) {
    return composite_var_impl(density, rgb, beta, weights_alt, sbins, B, R, S, near_plane, far_plane, spacing, clip_minmax,
                              ray_offset, chunk_rays, background, background_rgb, nonfinite_flag, out, nullptr, stream);
}

extern "C" int unerf_composite_var_views(const float* density, const float* rgb, const float* beta, const float* weights_alt,
                                         const float* sbins, int B, int64_t R, int S, float near_plane, float far_plane,
                                         int spacing, const float* clip_minmax, const unerf_ray_views* views, int64_t chunk_rays,
                                         int background, const float* background_rgb, int32_t* nonfinite_flag, float* out,
                                         void* stream) {
    if (int rc = check_views(views, R, "composite_var_views")) return rc;
    return composite_var_impl(density, rgb, beta, weights_alt, sbins, B, R, S, near_plane, far_plane, spacing, clip_minmax, 0,
                              chunk_rays, background, background_rgb, nonfinite_flag, out, views, stream);
}

// views = NULL: unerf_composite_moments
static int composite_moments_impl(const float* density, const float* rgb, const float* sbins, int B, int64_t R, int S,
                                  float near_plane, float far_plane, int spacing, const float* clip_minmax, int64_t ray_offset,
                                  int64_t chunk_rays, int background, const float* background_rgb,
                                  int32_t* nonfinite_flag, float* mean_out, float* var_out, const unerf_ray_views* views,
                                  void* stream) {
    UNERF_REQUIRE(R == 0 || (rgb && sbins && mean_out && var_out), "composite_moments: null pointer");   // density NULL: packed rows
    UNERF_REQUIRE(B >= 1 && B <= 16 && R >= 0, "composite_moments: B=%d outside [1,16] (use composite_var + moments)", B);
    UNERF_REQUIRE(S >= 1 && S <= 256, "composite_moments: S=%d outside [1,256]", S);
    UNERF_REQUIRE(!clip_minmax || chunk_rays > 0, "composite_moments: chunk_rays must be > 0 with clip_minmax");
    if (R == 0) return UNERF_OK;
    CompArgs a;
    a.density = density; a.rgb = rgb; a.beta = nullptr; a.walt = nullptr; a.sbins = sbins; a.B = B; a.R = R; a.S = S;
    if (int rc = set_spacing(a, near_plane, far_plane, spacing)) return rc;
    a.clip = clip_minmax; a.ray_offset = ray_offset; a.chunk_rays = chunk_rays; a.out = nullptr;
    if (int rc = unerf_set_background(a, background, background_rgb, "composite_moments")) return rc;
    a.flag = nonfinite_flag;
    dim3 grid(blocks_for(R, 16)), block(256);
    hipStream_t st = (hipStream_t)stream;
    const bool per_view = views && clip_minmax;   // composite_moments_kernel<SPL, RAGGED, PACKED, VW...>, as composite_var_impl
    with_pack(per_view, [&] { return make_view_map(views, chunk_rays); }, [&](auto... vm) {
        with_spl(S, [&](auto spl, auto ragged) {
            with_bool(density == nullptr, [&](auto packed) {
                hipLaunchKernelGGL((composite_moments_kernel<decltype(spl)::value, decltype(ragged)::value, decltype(packed)::value, decltype(vm)...>),
                                   grid, block, 0, st, a, mean_out, var_out, vm...);
            });
        });
    });
    return unerf_check_launch(per_view ? "composite_moments_views" : "composite_moments");
}

extern "C" int unerf_composite_moments(const float* density, const float* rgb, const float* sbins, int B, int64_t R, int S,
                                       float near_plane, float far_plane, int spacing, const float* clip_minmax, int64_t ray_offset,
                                       int64_t chunk_rays, int background, const float* background_rgb,
                                       int32_t* nonfinite_flag, float* mean_out, float* var_out, void* stream) {
    return composite_moments_impl(density, rgb, sbins, B, R, S, near_plane, far_plane, spacing, clip_minmax, ray_offset, chunk_rays,
                                  background, background_rgb, nonfinite_flag, mean_out, var_out, nullptr, stream);
}

extern "C" int unerf_composite_moments_views(const float* density, const float* rgb, const float* sbins, int B, int64_t R, int S,
                                             float near_plane, float far_plane, int spacing, const float* clip_minmax,
                                             const unerf_ray_views* views, int64_t chunk_rays, int background,
                                             const float* background_rgb, int32_t* nonfinite_flag, float* mean_out,
                                             float* var_out, void* stream) {
    if (int rc = check_views(views, R, "composite_moments_views")) return rc;
    return composite_moments_impl(density, rgb, sbins, B, R, S, near_plane, far_plane, spacing, clip_minmax, 0, chunk_rays,
                                  background, background_rgb, nonfinite_flag, mean_out, var_out, views, stream);
}

// ---- composite over sample-major planes: one lane per ray, front to back --------------------------------------
// Input = the planes unerf_field_fwd writes with sample_major = 1: density [B,S,R], rgb [B,S,3,R], beta [S,R].  A lane
// walks its ray's samples in order (every load is a coalesced row of 64 consecutive rays), so get_weights is the
// plain sequential recurrence -- no cross-lane scan -- and the K passes of a ray are reduced to mean / unbiased
// variance in the same thread (MOMENTS).  Passes are walked four at a time so that the bin edges (one IEEE
// division each) are converted once per group, not once per pass.
//   depth_var = sum_i w_i (t_i - d_median)^2 needs d_median, which is only known after the walk; instead of a second
//   walk (two more exp per sample) the three moments sum w, sum w t, sum w t^2 are kept in fp64 (products of fp32
//   numbers are exact there) and combined at the end: sum w t^2 - 2 d sum w t + d^2 sum w.
//   mean / variance over the passes: sums of (x - x_0) and (x - x_0)^2 around the first pass's value x_0 -- the
//   two-pass result of torch.stack(...).var(0) up to fp32 rounding, without keeping the B per-pass values.
struct CompSmArgs {
    const float* density;
    const float* rgb;
    const float* beta;
    const float* sbins;
    int B;
    int64_t R;
    int S;
    float s_near, s_far;
    int lin;   // UNERF_SPACING_*: 1 = identity spacing (UniformSampler)
    const float* clip;
    int64_t ray_offset, chunk_rays;
    float* out;       // [B,R,8] (MOMENTS = false)
    float* mean_out;  // [R,8]
    float* var_out;   // [R,8]
    int bg_mode;      // as CompArgs
    float bg[3];
    int32_t* flag;
};

#define CSM_G 4   // passes per walk

template <bool MOMENTS>
__global__ __launch_bounds__(256) void composite_sm_kernel(CompSmArgs a) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.R) return;
    const int S = a.S;
    const int64_t R = a.R;
    const float* sb = a.sbins + r * (S + 1);
    float clip_lo = 0.f, clip_hi = 0.f;
    if (a.clip) {
        const int64_t chunk = (a.ray_offset + r) / a.chunk_rays;
        clip_lo = a.clip[chunk * 2 + 0];
        clip_hi = a.clip[chunk * 2 + 1];
    }
    bool saw_nan = false;         // -> a.flag (see CompArgs)
    float x0[8], sd[8], sd2[8];   // moments over the passes, around pass 0
#pragma unroll
    for (int c = 0; c < 8; ++c) x0[c] = sd[c] = sd2[c] = 0.f;
    for (int b0 = 0; b0 < a.B; b0 += CSM_G) {
        const int nb = min(CSM_G, a.B - b0);
        float cr[CSM_G], cg[CSM_G], cb[CSM_G], accw[CSM_G], wt[CSM_G], uvar[CSM_G], depth[CSM_G];
        float lr[CSM_G], lg[CSM_G], lb[CSM_G];
        // the optical-depth prefix in fp64: S fp32 additions in a row lose up to S / 2 ulp of the prefix (2.8e-6 of a weight
        // behind 255 thin samples, three times what the scanned prefix of the group kernels is allowed)
        double cum[CSM_G], m0[CSM_G], m1[CSM_G], m2[CSM_G];
        bool found[CSM_G];
#pragma unroll
        for (int j = 0; j < CSM_G; ++j) {
            cr[j] = cg[j] = cb[j] = accw[j] = wt[j] = uvar[j] = depth[j] = 0.f;
            lr[j] = lg[j] = lb[j] = 0.f;
            cum[j] = m0[j] = m1[j] = m2[j] = 0.0;
            found[j] = false;
        }
        float e0 = unerf_s2e(sb[0], a.s_near, a.s_far, a.lin);
        float step = 0.f;
        for (int s = 0; s < S; ++s) {
            const float e1 = unerf_s2e(sb[s + 1], a.s_near, a.s_far, a.lin);
            const float delta = e1 - e0;
            step = (e0 + e1) / 2.f;
            e0 = e1;
            const double t64 = (double)step, t264 = t64 * t64;
            const float bt = a.beta ? a.beta[(int64_t)s * R + r] : 0.f;
#pragma unroll
            for (int j = 0; j < CSM_G; ++j) {
                if (j < nb) {  // uniform
                    const int64_t plane = (int64_t)(b0 + j) * S + s;
                    const float dens = a.density[plane * R + r];
                    const float* cp = a.rgb + plane * 3 * R + r;
                    const float r0 = unerf_nan_to_num(cp[0]), g0 = unerf_nan_to_num(cp[R]), bl0 = unerf_nan_to_num(cp[2 * R]);
                    saw_nan |= (dens != dens) | (cp[0] != cp[0]) | (cp[R] != cp[R]) | (cp[2 * R] != cp[2 * R]);
                    const float dd = delta * dens;
                    const float alpha = 1.f - unerf_exp(-dd);
                    const float T = unerf_exp(-(float)cum[j]);
                    cum[j] += (double)dd;
                    const float w = unerf_nan_to_num(alpha * T);
                    cr[j] += w * r0;
                    cg[j] += w * g0;
                    cb[j] += w * bl0;
                    accw[j] += w;
                    wt[j] += w * step;
                    uvar[j] += (w * w) * bt;
                    if (!found[j] && !(accw[j] < 0.5f)) {   // first index whose inclusive cumsum reaches 0.5
                        found[j] = true;
                        depth[j] = step;
                    }
                    const double w64 = (double)w;
                    m0[j] += w64;
                    m1[j] = fma(w64, t64, m1[j]);
                    m2[j] = fma(w64, t264, m2[j]);
                    lr[j] = r0; lg[j] = g0; lb[j] = bl0;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < CSM_G; ++j) {
            if (j < nb) {
                if (!found[j]) depth[j] = step;   // clamp(searchsorted, 0, S-1): the last sample's mid-point
                float o8[8];
                // RGBRenderer background (see unerf_set_background): last sample | constant colour | none
                const bool ls = a.bg_mode == UNERF_BG_LAST_SAMPLE, none = a.bg_mode == UNERF_BG_NONE;
                const float br = ls ? lr[j] : a.bg[0], bgn = ls ? lg[j] : a.bg[1], bb = ls ? lb[j] : a.bg[2];
                o8[0] = fminf(fmaxf(none ? cr[j] : cr[j] + br * (1.f - accw[j]), 0.f), 1.f);
                o8[1] = fminf(fmaxf(none ? cg[j] : cg[j] + bgn * (1.f - accw[j]), 0.f), 1.f);
                o8[2] = fminf(fmaxf(none ? cb[j] : cb[j] + bb * (1.f - accw[j]), 0.f), 1.f);
                o8[3] = accw[j];
                o8[4] = depth[j];
                float ed = wt[j] / (accw[j] + 1e-10f);
                if (a.clip) ed = fminf(fmaxf(ed, clip_lo), clip_hi);
                o8[5] = ed;
                o8[6] = uvar[j];
                const double d64 = (double)depth[j];
                o8[7] = (float)(m2[j] - 2.0 * d64 * m1[j] + d64 * d64 * m0[j]) + 1e-5f;
                if (!MOMENTS) {
                    float4* o = reinterpret_cast<float4*>(a.out + ((int64_t)(b0 + j) * R + r) * 8);
                    o[0] = make_float4(o8[0], o8[1], o8[2], o8[3]);
                    o[1] = make_float4(o8[4], o8[5], o8[6], o8[7]);
                } else if (b0 + j == 0) {
#pragma unroll
                    for (int c = 0; c < 8; ++c) x0[c] = o8[c];
                } else {
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        const float d = o8[c] - x0[c];
                        sd[c] += d;
                        sd2[c] += d * d;
                    }
                }
            }
        }
    }
    if (a.flag && saw_nan) atomicOr(a.flag, 1);
    if (MOMENTS) {
        const float invB = 1.f / (float)a.B, invB1 = 1.f / (float)(a.B - 1);
        float m8[8], v8[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            m8[c] = x0[c] + sd[c] * invB;
            v8[c] = fmaxf(sd2[c] - sd[c] * sd[c] * invB, 0.f) * invB1;
        }
        float4* mo = reinterpret_cast<float4*>(a.mean_out + r * 8);
        float4* vo = reinterpret_cast<float4*>(a.var_out + r * 8);
        mo[0] = make_float4(m8[0], m8[1], m8[2], m8[3]);
        mo[1] = make_float4(m8[4], m8[5], m8[6], m8[7]);
        vo[0] = make_float4(v8[0], v8[1], v8[2], v8[3]);
        vo[1] = make_float4(v8[4], v8[5], v8[6], v8[7]);
    }
}

static int composite_planes_launch(const float* density, const float* rgb, const float* beta, const float* sbins, int B,
                                   int64_t R, int S, float near_plane, float far_plane, int spacing, const float* clip_minmax,
                                   int64_t ray_offset, int64_t chunk_rays, int background, const float* background_rgb,
                                   int32_t* nonfinite_flag, float* out, float* mean_out, float* var_out, void* stream,
                                   const char* what) {
    UNERF_REQUIRE(R == 0 || (density && rgb && sbins), "%s: null pointer", what);
    UNERF_REQUIRE(B >= 1 && R >= 0 && S >= 1, "%s: bad B/R/S", what);
    UNERF_REQUIRE(!clip_minmax || chunk_rays > 0, "%s: chunk_rays must be > 0 with clip_minmax", what);
    if (R == 0) return UNERF_OK;
    CompSmArgs a;
    a.density = density; a.rgb = rgb; a.beta = beta; a.sbins = sbins; a.B = B; a.R = R; a.S = S;
    if (int rc = set_spacing(a, near_plane, far_plane, spacing)) return rc;
    a.clip = clip_minmax; a.ray_offset = ray_offset; a.chunk_rays = chunk_rays;
    a.out = out; a.mean_out = mean_out; a.var_out = var_out;
    if (int rc = unerf_set_background(a, background, background_rgb, what)) return rc;
    a.flag = nonfinite_flag;
    dim3 grid(blocks_for(R, 256)), block(256);
    with_bool(out == nullptr, [&](auto moments) {
        hipLaunchKernelGGL(composite_sm_kernel<decltype(moments)::value>, grid, block, 0, (hipStream_t)stream, a);
    });
    return unerf_check_launch(what);
}

extern "C" int unerf_composite_var_planes(const float* density, const float* rgb, const float* beta, const float* sbins,
                                          int B, int64_t R, int S, float near_plane, float far_plane, int spacing,
                                          const float* clip_minmax, int64_t ray_offset, int64_t chunk_rays, int background,
                                          const float* background_rgb, int32_t* nonfinite_flag, float* out, void* stream) {
    UNERF_REQUIRE(R == 0 || out, "composite_var_planes: null pointer");
    return composite_planes_launch(density, rgb, beta, sbins, B, R, S, near_plane, far_plane, spacing, clip_minmax, ray_offset,
                                   chunk_rays, background, background_rgb, nonfinite_flag, out, nullptr, nullptr, stream,
                                   "composite_var_planes");
}

extern "C" int unerf_composite_moments_planes(const float* density, const float* rgb, const float* sbins, int B,
                                              int64_t R, int S, float near_plane, float far_plane, int spacing,
                                              const float* clip_minmax, int64_t ray_offset, int64_t chunk_rays,
                                              int background, const float* background_rgb, int32_t* nonfinite_flag,
                                              float* mean_out, float* var_out, void* stream) {
    UNERF_REQUIRE(R == 0 || (mean_out && var_out), "composite_moments_planes: null pointer");
    UNERF_REQUIRE(B >= 2, "composite_moments_planes: B=%d (the unbiased variance needs at least two passes)", B);
    return composite_planes_launch(density, rgb, nullptr, sbins, B, R, S, near_plane, far_plane, spacing, clip_minmax, ray_offset,
                                   chunk_rays, background, background_rgb, nonfinite_flag, nullptr, mean_out, var_out, stream,
                                   "composite_moments_planes");
}

// ---- laplace depth draws --------------------------------------------------------------
struct LapDepthArgs {
    const float* mu;
    const float* var;
    const float* sbins;
    int64_t R;
    int S;
    float s_near, s_far;
    int lin;   // UNERF_SPACING_*: 1 = identity spacing (UniformSampler)
    const float* noise;
    int D;
    uint32_t seed;
    int64_t ray_offset;
    float* out;
};

// Built-in generator of the depth draws (noise == NULL; twin: oracle normal_noise).  The round-2 form spent two full
// 32-bit hashes (four quarter-rate integer multiplies) per draw PAIR and sample -- more issue slots than the Box-Muller
// transform they feed.  Now every (ray, sample) owns ONE xorshift32 stream, seeded by the counter hash of its global sample
// index (so launch grouping still cannot change a draw) and stepped once per draw pair (six full-rate shift / xor
// instructions); the two 16-bit halves of the state are the two uniforms of a Box-Muller pair, BOTH of whose outputs are
// used (cos for the even draw, sin for the odd one).  v_log_f32 is log2, v_sin / v_cos take revolutions: no argument
// scaling.  16-bit uniforms bound |z| by sqrt(34 ln 2) = 4.85 and quantise the radius to 65536 levels -- far below the
// Monte-Carlo error of a 100-draw mean (tests: moments, independence between samples, draws and halves).
__device__ __forceinline__ uint32_t unerf_xorshift32(uint32_t x) {
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 5;
    return x;
}
__device__ __forceinline__ uint32_t unerf_depth_stream_seed(uint32_t seed, uint32_t sample_idx) {
    const uint32_t x = unerf_mc_base(unerf_mc_key(seed, 0u), sample_idx);
    return x ? x : UNERF_GOLDEN;   // 0 is xorshift's fixed point
}
__device__ __forceinline__ void unerf_normal_pair_from_state(uint32_t x, float& z0, float& z1) {
    const float u1 = fmaf((float)(x >> 16), 1.0f / 65536.0f, 0.5f / 65536.0f);
    const float u2 = fmaf((float)(x & 0xFFFFu), 1.0f / 65536.0f, 0.5f / 65536.0f);
    const float rad = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));   // sqrt(-2 ln u1)
    z0 = rad * __builtin_amdgcn_cosf(u2);
    z1 = rad * __builtin_amdgcn_sinf(u2);
}

// get_weights for the Monte-Carlo depth draws.  With e_i = exp(-delta_i sigma_i) the weights are
//   w_i = (1 - e_i) prod_{j<i} e_j = P_i - P_{i+1},   P_i = prod_{j<i} e_j,
// the transmittance as a running product (a 16-lane multiplicative scan of the lanes' own products) instead of a second
// exp of the running sum.  Per draw and sample: the exponent min(a_i z + b_i, 0) with a_i = -delta_i log2(e) sd_i and
// b_i = -delta_i log2(e) mu_i formed once per sample (= -delta log2(e) relu(mu + sd z): -delta <= 0 turns the relu into a
// min), one v_exp_f32, one multiply for the running product, one subtract, and one fma that adds carry * (P_i - P_{i+1})
// to the sample's sum over the draws -- 7 issue slots + 5 DPP multiplies per lane and draw (round 2: 12 + 5).
// NaN: fminf drops a NaN exponent (the factor becomes 1: weight 0 at that sample, the later ones untouched), where
// get_weights' cumsum carries it into every later sample of the ray and nan_to_num zeroes them all.  A NaN exponent comes from
// b_i (a NaN mean or bin edge; a NaN or negative variance becomes sd = 1e-10) and is the same in every draw, so the caller finds
// the first such sample of the ray once and writes 0 from there on; a NaN that still reaches a sum is mapped to 0 there too.
template <int SPL>
__device__ __forceinline__ void group_weights_accumulate(const float (&z)[SPL], const float (&a)[SPL], const float (&b)[SPL],
                                                         float (&wsum)[SPL]) {
    float dl[SPL], lp = 1.f;
#pragma unroll
    for (int e = 0; e < SPL; ++e) {
        const float em = __builtin_amdgcn_exp2f(fminf(fmaf(a[e], z[e], b[e]), 0.f));
        const float nx = lp * em;
        dl[e] = lp - nx;     // this lane's share of w_e: (product before) - (product after)
        lp = nx;
    }
    // exclusive multiplicative scan over the 16 lanes of the ray
    // (DPP row shifts; lanes without a source lane keep the `old` operand = 1)
    float incl = lp;
    incl *= dpp_f_or<0x111>(incl, 1.f);
    incl *= dpp_f_or<0x112>(incl, 1.f);
    incl *= dpp_f_or<0x114>(incl, 1.f);
    incl *= dpp_f_or<0x118>(incl, 1.f);
    const float carry = dpp_f_or<0x111>(incl, 1.f);
#pragma unroll
    for (int e = 0; e < SPL; ++e) wsum[e] = fmaf(carry, dl[e], wsum[e]);
}

// SEVERAL VIEWS (unerf_laplace_depth_weights_views): a kernel argument of lap_depth_kernel<.., LapDepthViews> only.  Launch row r is
// frame-local ray r mod hw of view r / hw; its streams are seeded inside its own frame under its view's seed.
struct LapDepthViews {
    FastDiv div_hw;   // by rays per view
    uint32_t hw;
    uint32_t seed[UNERF_NERF_MAX_VIEWS];   // staged in LDS, read by view index (a block of 16 rays straddles views)
};
__device__ __forceinline__ const LapDepthViews& lap_depth_views_of(const LapDepthViews& x) { return x; }
template <int SPL, bool RAGGED = false, typename... VW>   // VW = LapDepthViews (unerf_laplace_depth_weights_views), else none
__global__ __launch_bounds__(256) void lap_depth_kernel(LapDepthArgs a, VW... vw) {
    const int l16 = threadIdx.x & 15;
    int64_t r = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool ok = r < a.R;
    if (!ok) r = a.R - 1;
    const int S = a.S, k0 = l16 * SPL;
    uint32_t vseed = 0u, vlocal = 0u;   // VW: the seed of this group's view and its ray inside the view's frame
    if constexpr (sizeof...(VW) != 0) {
        __shared__ uint32_t s_seed[UNERF_NERF_MAX_VIEWS];
        const LapDepthViews& dv = lap_depth_views_of(vw...);
        if (threadIdx.x < UNERF_NERF_MAX_VIEWS) s_seed[threadIdx.x] = dv.seed[threadIdx.x];
        __syncthreads();
        const uint32_t view = fastdiv((uint32_t)r, dv.div_hw);
        vseed = s_seed[view];
        vlocal = (uint32_t)r - view * dv.hw;
    }
    const float* sb = a.sbins + r * (S + 1);
    float eu[SPL + 1], ca[SPL], cb[SPL], wsum[SPL];
    uint32_t st[SPL];
#pragma unroll
    for (int e = 0; e <= SPL; ++e) eu[e] = unerf_s2e(sb[RAGGED ? min(k0 + e, S) : k0 + e], a.s_near, a.s_far, a.lin);
#pragma unroll
    for (int e = 0; e < SPL; ++e) {
        const float nd2 = -(eu[e + 1] - eu[e]) * 1.4426950408889634f;
        const bool live = !RAGGED || k0 + e < S;   // masked slots: mu = sd = 0 -> exponent 0, e = 1, weight 0
        const float mu = live ? a.mu[r * S + k0 + e] : 0.f;
        const float s = live ? sqrtf(a.var[r * S + k0 + e]) : 0.f;
        const float sd = !live ? 0.f : (s != s) ? 1e-10f : fmaxf(s, 1e-10f);
        ca[e] = nd2 * sd;
        cb[e] = nd2 * mu;
        wsum[e] = 0.f;
        if constexpr (sizeof...(VW) != 0) st[e] = a.noise ? 0u : unerf_depth_stream_seed(vseed, (uint32_t)((int64_t)vlocal * S + k0 + e));
        else st[e] = a.noise ? 0u : unerf_depth_stream_seed(a.seed, (uint32_t)((a.ray_offset + r) * S + k0 + e));
    }
    int first_nan = S;   // the first sample of the ray whose exponent is NaN in every draw (see group_weights_accumulate)
#pragma unroll
    for (int e = 0; e < SPL; ++e)
        if ((!RAGGED || k0 + e < S) && cb[e] != cb[e]) first_nan = min(first_nan, k0 + e);
    first_nan = min(first_nan, dpp_i<0xB1>(first_nan));
    first_nan = min(first_nan, dpp_i<0x4E>(first_nan));
    first_nan = min(first_nan, dpp_i<0x141>(first_nan));
    first_nan = min(first_nan, dpp_i<0x140>(first_nan));
    for (int d0 = 0; d0 < a.D; d0 += 2) {
        float z[2][SPL];
        if (a.noise) {
#pragma unroll
            for (int e = 0; e < SPL; ++e) {
                const bool live = !RAGGED || k0 + e < S;
                z[0][e] = live ? a.noise[((int64_t)d0 * a.R + r) * S + k0 + e] : 0.f;
                z[1][e] = (live && d0 + 1 < a.D) ? a.noise[((int64_t)(d0 + 1) * a.R + r) * S + k0 + e] : 0.f;
            }
        } else {
#pragma unroll
            for (int e = 0; e < SPL; ++e) {
                unerf_normal_pair_from_state(st[e], z[0][e], z[1][e]);
                st[e] = unerf_xorshift32(st[e]);
            }
        }
        group_weights_accumulate<SPL>(z[0], ca, cb, wsum);
        if (d0 + 1 < a.D) group_weights_accumulate<SPL>(z[1], ca, cb, wsum);
    }
    if (ok) {
#pragma unroll
        for (int e = 0; e < SPL; ++e) {
            const float w = wsum[e] / (float)a.D;
            if (!RAGGED || k0 + e < S) a.out[r * S + k0 + e] = (w != w || k0 + e >= first_nan) ? 0.f : w;
        }
    }
}
// One body behind both entry points (each keeps its own checks): views = lap_views = NULL is unerf_laplace_depth_weights.
static int lap_depth_impl(const float* density_mu, const float* density_var, const float* sbins, int64_t R, int S,
                          float near_plane, float far_plane, int spacing, const float* noise, int D, uint32_t seed,
                          int64_t ray_offset, const unerf_ray_views* views, const unerf_laplace_views* lap_views,
                          float* weights_out, void* stream, const char* what) {
    LapDepthArgs a;
    a.mu = density_mu; a.var = density_var; a.sbins = sbins; a.R = R; a.S = S;
    if (int rc = set_spacing(a, near_plane, far_plane, spacing)) return rc;
    a.noise = noise; a.D = D; a.seed = seed; a.ray_offset = ray_offset; a.out = weights_out;
    auto make_views = [&] {
        LapDepthViews dv;
        dv.div_hw = make_fastdiv((uint32_t)views->rays_per_view); dv.hw = (uint32_t)views->rays_per_view;
        for (int v = 0; v < UNERF_NERF_MAX_VIEWS; ++v) dv.seed[v] = lap_views->depth_seed[v < views->n_views ? v : 0];
        return dv;
    };
    dim3 grid(blocks_for(R, 16)), block(256);
    with_pack(views != nullptr, make_views, [&](auto... dv) {   // lap_depth_kernel<SPL, RAGGED, VW...>
        with_spl(S, [&](auto spl, auto ragged) {
            hipLaunchKernelGGL((lap_depth_kernel<decltype(spl)::value, decltype(ragged)::value, decltype(dv)...>), grid, block, 0,
                               (hipStream_t)stream, a, dv...);
        });
    });
    return unerf_check_launch(what);
}

extern "C" int unerf_laplace_depth_weights(const float* density_mu, const float* density_var, const float* sbins,
                                           int64_t R, int S, float near_plane, float far_plane, int spacing, const float* noise,
                                           int D, uint32_t seed, int64_t ray_offset, float* weights_out, void* stream) {
    UNERF_REQUIRE(R == 0 || (density_mu && density_var && sbins && weights_out), "laplace_depth_weights: null pointer");
    UNERF_REQUIRE(D >= 1 && R >= 0 && S >= 1 && S <= 256, "laplace_depth_weights: bad D/R/S");
    if (R == 0) return UNERF_OK;
    return lap_depth_impl(density_mu, density_var, sbins, R, S, near_plane, far_plane, spacing, noise, D, seed, ray_offset, nullptr,
                          nullptr, weights_out, stream, "laplace_depth_weights");
}

// Several views in one launch: the stream of launch row r, sample k is seeded by (depth_seed[view], local * S + k), i.e. what
// unerf_laplace_depth_weights(seed = depth_seed[view], ray_offset = 0) draws for that view alone.  With explicit `noise` there
// is no per-view value: rows are launch rows, as in the single call on the tall ray list.
extern "C" int unerf_laplace_depth_weights_views(const float* density_mu, const float* density_var, const float* sbins,
                                                 int64_t R, int S, float near_plane, float far_plane, int spacing, const float* noise,
                                                 int D, const unerf_ray_views* views, const unerf_laplace_views* lap_views,
                                                 float* weights_out, void* stream) {
    if (int rc = check_views(views, R, "laplace_depth_weights_views")) return rc;
    UNERF_REQUIRE(lap_views, "laplace_depth_weights_views: null lap_views (the depth seed of every view)");
    UNERF_REQUIRE(density_mu && density_var && sbins && weights_out, "laplace_depth_weights_views: null pointer");
    UNERF_REQUIRE(D >= 1 && S >= 1 && S <= 256, "laplace_depth_weights_views: bad D/S");
    return lap_depth_impl(density_mu, density_var, sbins, R, S, near_plane, far_plane, spacing, noise, D, 0u, 0, views, lap_views,
                          weights_out, stream, "laplace_depth_weights_views");
}

// ======================================================================================
// 7. moments over the leading (pass / member) dimension
// ======================================================================================
// The two-pass fp32 moments of NC neighbouring channels of one element over its K sources, x(k, c) = source k's value of
// channel c: what torch.stack(...).mean(0) / .var(0) compute.  ONE statement of the order of operations for moments_kernel
// and ensemble_reduce_kernel, so that the two agree bit for bit: per channel s += x_k for k = 0 .. K-1, m = s / K,
// q += (x_k - m)^2 in the same order, q / (K - 1).
// The loads of MOMENTS_UNROLL sources are issued together and then added in source order -- the additions are the ones of the
// plain loop, the memory latencies overlap instead of following one another.
// The second pass reads the sources again: K is a run-time count (up to 64 members of up to 4 channels), so the values cannot
// stay in registers without spilling, and the re-read comes from lines the same wave has just fetched (TCP, else L2).
#define MOMENTS_UNROLL 8
template <int NC, class Load>
__device__ __forceinline__ void moments_of(Load x, int K, bool want_var, float (&mean)[NC], float (&var)[NC]) {
    constexpr int U = NC == 1 ? MOMENTS_UNROLL : MOMENTS_UNROLL / 2;
    float s[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) s[c] = 0.f;
    int k = 0;
    for (; k + U <= K; k += U) {
        float t[U][NC];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < NC; ++c) t[u][c] = x(k + u, c);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < NC; ++c) s[c] += t[u][c];
    }
    for (; k < K; ++k)
#pragma unroll
        for (int c = 0; c < NC; ++c) s[c] += x(k, c);
#pragma unroll
    for (int c = 0; c < NC; ++c) mean[c] = s[c] / (float)K;
    if (!want_var) return;
    float q[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) q[c] = 0.f;
    for (k = 0; k + U <= K; k += U) {
        float t[U][NC];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < NC; ++c) t[u][c] = x(k + u, c);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                float d = t[u][c] - mean[c];
                q[c] += d * d;
            }
    }
    for (; k < K; ++k)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            float d = x(k, c) - mean[c];
            q[c] += d * d;
        }
#pragma unroll
    for (int c = 0; c < NC; ++c) var[c] = q[c] / (float)(K - 1);  // K==1 -> NaN, as torch.var(unbiased) does
}

__global__ __launch_bounds__(256) void moments_kernel(const float* __restrict__ x, int K, int64_t NC,
                                                      float* __restrict__ mean, float* __restrict__ var) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= NC) return;
    float m[1], v[1];
    moments_of<1>([&](int k, int) { return x[(int64_t)k * NC + i]; }, K, var != nullptr, m, v);
    mean[i] = m[0];
    if (var) var[i] = v[0];
}

extern "C" int unerf_moments(const float* x, int K, int64_t N, int C, float* mean, float* var, void* stream) {
    UNERF_REQUIRE(N == 0 || (x && mean), "moments: null pointer");
    UNERF_REQUIRE(K >= 1 && N >= 0 && C >= 1, "moments: bad K/N/C");
    if (N == 0) return UNERF_OK;
    hipLaunchKernelGGL(moments_kernel, dim3(blocks_for(N * C, 256)), dim3(256), 0, (hipStream_t)stream, x, K, N * C,
                       mean, var);
    return unerf_check_launch("moments");
}

// ======================================================================================
// 8. fused ensemble reduce: B views x every member key x M members in one launch
// ======================================================================================
// One thread per (view, input key, element): it walks the key's channels, takes their moments over the members with
// moments_of, stores the blocks the plan asks for and keeps the running channel sums of the derived keys, so a derived
// value never leaves the thread.  The aleatoric term is the member mean of ANOTHER key (rgb -> rgb_var): the thread forms it
// again from that key's sources -- the same additions in the same order as the thread that owns the key, hence the same
// bits -- instead of waiting for a second launch.
// Memory: the kernel is bandwidth-bound.  Lanes are consecutive elements, so a [n,1] key is one 256-byte run per wave and
// load.  [n,3] rows (12-byte stride) spread a wave's load over six 128-byte lines; the three channels of a row are loaded
// back to back (moments_of<3>), so the lines are fetched once and the other two loads hit them.  A 3-channel slice of [n,8]
// rows (32-byte stride) touches sixteen lines of which 12 bytes in 32 are used, whatever the mapping is.  Channels go in
// groups of 4, then 3, then 1, each group with 12 to 16 loads in flight per lane.  The variance pass re-reads (see
// moments_of).
// Block order: the keys of a member are often slices of the SAME rows (rgb, accumulation, depth ... of the composite's
// [R,8] rows), so the blocks that work on one pixel range for different keys should meet in one L2.  Blocks are dealt
// round-robin over the 8 XCDs, each with its own L2; blockIdx.x = ((g * keys + k) * 8 + x) puts pixel block 8 g + x of
// every key k on XCD x, one key after the other: the first key's block brings the rows in, the others hit them.  (Key-major
// order -- all blocks of key 0, then key 1 ... -- fetched every row once per key: measured 0.84 x the per-view loop on
// active-nerfacto keys at 800 x 800.)  A key with fewer blocks than the largest leaves its surplus blocks idle.
struct EnsKeyDev {
    int64_t n;                       // elements
    int64_t out[UNERF_ENS_STATS];    // offset of the statistic's block inside a view's part of the arena, -1: not asked for
    int32_t C, stride;
    int32_t aux, aux_C, aux_stride;  // aux < 0: no aleatoric term
    int32_t pad;
};
struct EnsArgs {
    EnsKeyDev key[UNERF_ENS_MAX_KEYS];
    const float* const* table;       // [B][n_keys][M]
    float* arena;
    int64_t view_stride;
    int32_t n_keys, M;
    int32_t n_used;                  // keys something is asked of: used[0 .. n_used)
    uint8_t used[UNERF_ENS_MAX_KEYS];
};
#define ENS_XCDS 8
typedef const float __attribute__((address_space(1)))* ens_src_t;   // the sources are device memory: global, not flat, loads

// channels c0 .. c0 + NC - 1 of element p (e = its first float): moments, the MEAN / VAR blocks, the running channel sums
template <int NC>
__device__ __forceinline__ void ens_channels(const float* const* __restrict__ src, int M, int64_t e, int c0, bool want_var,
                                             float* __restrict__ out, int64_t o_mean, int64_t o_var, int64_t row, float& sum_m,
                                             float& sum_v, float& sum_sd) {
    float m[NC], v[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = 0.f;
    moments_of<NC>([&](int j, int c) { return ((ens_src_t)src[j])[e + c0 + c]; }, M, want_var, m, v);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (o_mean >= 0) out[o_mean + row + c0 + c] = m[c];
        if (o_var >= 0) out[o_var + row + c0 + c] = v[c];
        const float sd = sqrtf(v[c]);
        const bool first = c0 + c == 0;
        sum_m = first ? m[c] : sum_m + m[c];
        sum_v = first ? v[c] : sum_v + v[c];
        sum_sd = first ? sd : sum_sd + sd;
    }
}

// every channel of one element of one key, in channel order: groups of 4, a last group of 3, else single channels
__device__ __forceinline__ void ens_element(const float* const* __restrict__ src, int M, int C, int64_t e, bool want_var,
                                            float* __restrict__ out, int64_t o_mean, int64_t o_var, int64_t row, float& sum_m,
                                            float& sum_v, float& sum_sd) {
    int c = 0;
    for (; C - c >= 4; c += 4) ens_channels<4>(src, M, e, c, want_var, out, o_mean, o_var, row, sum_m, sum_v, sum_sd);
    if (C - c == 3) {
        ens_channels<3>(src, M, e, c, want_var, out, o_mean, o_var, row, sum_m, sum_v, sum_sd);
        return;
    }
    for (; c < C; ++c) ens_channels<1>(src, M, e, c, want_var, out, o_mean, o_var, row, sum_m, sum_v, sum_sd);
}

__global__ __launch_bounds__(256) void ensemble_reduce_kernel(EnsArgs a) {
    const int v = blockIdx.y;
    const uint32_t x = blockIdx.x % ENS_XCDS, t = blockIdx.x / ENS_XCDS;
    const int k = a.used[t % (uint32_t)a.n_used];
    const EnsKeyDev& d = a.key[k];
    const int64_t p = ((int64_t)(t / (uint32_t)a.n_used) * ENS_XCDS + x) * 256 + threadIdx.x;
    if (p >= d.n) return;
    const int M = a.M, C = d.C;
    float* __restrict__ out = a.arena + (int64_t)v * a.view_stride;
    const int64_t o_mean = d.out[UNERF_ENS_MEAN], o_var = d.out[UNERF_ENS_VAR], o_epi = d.out[UNERF_ENS_VAR_CMEAN],
                  o_alea = d.out[UNERF_ENS_ALEA_CMEAN], o_sum = d.out[UNERF_ENS_EPI_ALEA],
                  o_sqrt = d.out[UNERF_ENS_EPI_ALEA_SQRT], o_std = d.out[UNERF_ENS_STD_CMEAN];
    const bool want_var = (o_var & o_epi & o_sum & o_sqrt & o_std) >= 0;   // one of them is asked for (offsets are >= 0 or -1)
    float sum_m = 0.f, sum_v = 0.f, sum_sd = 0.f;
    ens_element(a.table + ((int64_t)v * a.n_keys + k) * M, M, C, p * d.stride, want_var, out, o_mean, o_var, p * C, sum_m, sum_v,
                sum_sd);
    const float epi = sum_v / (float)C;
    if (o_epi >= 0) out[o_epi + p] = epi;
    if (o_std >= 0) out[o_std + p] = sum_sd / (float)C;
    if ((o_alea & o_sum & o_sqrt) >= 0 && d.aux >= 0) {
        float alea = 0.f, unused_v = 0.f, unused_sd = 0.f;
        ens_element(a.table + ((int64_t)v * a.n_keys + d.aux) * M, M, d.aux_C, p * d.aux_stride, false, out, -1, -1, 0, alea,
                    unused_v, unused_sd);
        alea = alea / (float)d.aux_C;
        if (o_alea >= 0) out[o_alea + p] = alea;
        const float sum = epi + alea;
        if (o_sum >= 0) out[o_sum + p] = sum;
        if (o_sqrt >= 0) out[o_sqrt + p] = sqrtf(sum);
    }
}

extern "C" int unerf_ensemble_reduce(const float* const* table, int B, int n_keys, int M, const unerf_ens_key* keys,
                                     const unerf_ens_out* plan, int n_out, int64_t view_stride, float* arena,
                                     int64_t arena_floats, void* stream) {
    UNERF_REQUIRE(B >= 0 && B <= UNERF_NERF_MAX_VIEWS, "ensemble_reduce: B=%d outside [0,%d]", B, UNERF_NERF_MAX_VIEWS);
    UNERF_REQUIRE(n_keys >= 1 && n_keys <= UNERF_ENS_MAX_KEYS, "ensemble_reduce: n_keys=%d outside [1,%d]", n_keys,
                  UNERF_ENS_MAX_KEYS);
    UNERF_REQUIRE(M >= 1 && M <= UNERF_ENS_MAX_MEMBERS, "ensemble_reduce: M=%d outside [1,%d]", M, UNERF_ENS_MAX_MEMBERS);
    UNERF_REQUIRE(keys && n_out >= 0 && (plan || n_out == 0), "ensemble_reduce: null key / plan descriptor");
    UNERF_REQUIRE(view_stride >= 0 && arena_floats >= 0, "ensemble_reduce: negative arena size");
    EnsArgs a;
    a.table = table; a.arena = arena; a.view_stride = view_stride; a.n_keys = n_keys; a.M = M;
    for (int k = 0; k < UNERF_ENS_MAX_KEYS; ++k) {
        EnsKeyDev& d = a.key[k];
        d.n = 0; d.C = 1; d.stride = 1; d.aux = -1; d.aux_C = 1; d.aux_stride = 1; d.pad = 0;
        a.used[k] = 0;
        for (int s = 0; s < UNERF_ENS_STATS; ++s) d.out[s] = -1;
    }
    int64_t most = 0, work = 0;   // most: blocks of the key with the most elements
    a.n_used = 0;
    for (int k = 0; k < n_keys; ++k) {
        UNERF_REQUIRE(keys[k].channels >= 1 && keys[k].channels <= UNERF_ENS_MAX_CHANNELS,
                      "ensemble_reduce: key %d has %d channels, outside [1,%d]", k, keys[k].channels, UNERF_ENS_MAX_CHANNELS);
        UNERF_REQUIRE(keys[k].stride >= keys[k].channels && keys[k].n >= 0,
                      "ensemble_reduce: key %d: stride %d < channels %d, or n < 0", k, keys[k].stride, keys[k].channels);
        a.key[k].n = keys[k].n; a.key[k].C = keys[k].channels; a.key[k].stride = keys[k].stride;
    }
    for (int o = 0; o < n_out; ++o) {
        const unerf_ens_out& e = plan[o];
        UNERF_REQUIRE(e.stat >= 0 && e.stat < UNERF_ENS_STATS && e.key >= 0 && e.key < n_keys,
                      "ensemble_reduce: output %d: statistic %d / key %d", o, e.stat, e.key);
        EnsKeyDev& d = a.key[e.key];
        UNERF_REQUIRE(d.out[e.stat] < 0, "ensemble_reduce: output %d repeats statistic %d of key %d", o, e.stat, e.key);
        const int64_t len = d.n * (e.stat <= UNERF_ENS_VAR ? d.C : 1);
        UNERF_REQUIRE(e.offset >= 0 && e.offset + len <= view_stride, "ensemble_reduce: output %d leaves the view's part of the arena", o);
        for (int q = 0; q < o; ++q) {
            const int64_t lq = a.key[plan[q].key].n * (plan[q].stat <= UNERF_ENS_VAR ? a.key[plan[q].key].C : 1);
            UNERF_REQUIRE(e.offset + len <= plan[q].offset || plan[q].offset + lq <= e.offset,
                          "ensemble_reduce: outputs %d and %d overlap", q, o);
        }
        if (e.stat == UNERF_ENS_ALEA_CMEAN || e.stat == UNERF_ENS_EPI_ALEA || e.stat == UNERF_ENS_EPI_ALEA_SQRT) {
            UNERF_REQUIRE(e.aux >= 0 && e.aux < n_keys && a.key[e.aux].n == d.n && (d.aux < 0 || d.aux == e.aux),
                          "ensemble_reduce: output %d: aux key %d", o, e.aux);
            d.aux = e.aux; d.aux_C = a.key[e.aux].C; d.aux_stride = a.key[e.aux].stride;
        }
        d.out[e.stat] = e.offset;
    }
    for (int k = 0; k < n_keys; ++k) {
        bool used = false;
        for (int s = 0; s < UNERF_ENS_STATS; ++s) used = used || a.key[k].out[s] >= 0;
        if (!used || a.key[k].n == 0) continue;      // nothing asked of this key, or nothing in it: no blocks
        a.used[a.n_used++] = (uint8_t)k;
        const int64_t nb = (a.key[k].n + 255) / 256;
        if (nb > most) most = nb;
        work += a.key[k].n;
    }
    const int64_t blocks = (most + ENS_XCDS - 1) / ENS_XCDS * ENS_XCDS * a.n_used;
    UNERF_REQUIRE(blocks < (int64_t)1 << 31, "ensemble_reduce: too many elements for one launch");
    UNERF_REQUIRE((int64_t)B * view_stride <= arena_floats, "ensemble_reduce: arena of %lld floats for %d views of %lld",
                  (long long)arena_floats, B, (long long)view_stride);
    UNERF_REQUIRE(B == 0 || work == 0 || (table && arena), "ensemble_reduce: null table / arena");
    if (B == 0 || work == 0) return UNERF_OK;
    hipLaunchKernelGGL(ensemble_reduce_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
    return unerf_check_launch("ensemble_reduce");
}
