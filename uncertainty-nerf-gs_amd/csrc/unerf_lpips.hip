// LPIPS (AlexNet) for the eval harness: include/unerf.h, "LPIPS"; host definition metrics.py: lpips.
//
// Five kernels.  lp_pack scales the two image stacks into one NHWC activation stack and counts the values upstream's
// input check refuses.  lp_conv is the one dense-convolution kernel of the project: an implicit GEMM on the fp32-input
// MFMA (v_mfma_f32_32x32x2_f32: every product rounded once, fp32 accumulate -- gfx950 has no TF32 form, and the
// reference computes in fp32).  lp_pool is the 3 / 2 max-pool.  lp_head turns one tap's two feature stacks into
// per-workgroup float64 partials, lp_sum adds an image's partials in index order.  No floating-point atomics anywhere:
// every number is one fixed-order chain, so a call repeats bit for bit and row b of a batch is the row of image b alone
// (the image is grid.y of the head, and a convolution output does not depend on which tile it falls in).
//
// lp_conv: a workgroup of four waves owns a 64 x 64 tile of the [pixels, C_out] output, each wave one 32 x 32 quarter
// with ONE 16-register accumulator (the dependent-accumulator latency of the 32x32x2 form equals its issue interval, so
// one chain per wave already issues back to back).  The reduction runs in steps of 16 over k = (ky ks + kx) C_in + c:
// per step the workgroup stages a [16][64] slice of the im2col matrix (gathered with predicated loads: a tap outside the
// image, a row past the last pixel and k >= K all give 0) and a [16][64] slice of the [K, C_out] weights in LDS, the
// loads of step s + 1 in flight in registers while the eight MFMAs of step s run.  Consecutive k of one tap are
// consecutive floats of the NHWC input, so a row's 16 loads are one 64-byte segment wherever C_in >= 16.
#include "unerf_common.hpp"

#include <algorithm>

namespace {

constexpr int LP_LAYERS = UNERF_LPIPS_LAYERS;
constexpr int CV_BM = UNERF_LPIPS_CONV_TILE_M, CV_BN = UNERF_LPIPS_CONV_TILE_N, CV_BK = UNERF_LPIPS_CONV_STEP_K, CV_THREADS = 256;
constexpr int CV_AROWS = CV_BM * CV_BK / CV_THREADS;     // im2col rows per thread and step (4)
constexpr int CV_BROWS = CV_BK * CV_BN / CV_THREADS;     // weight rows per thread and step (4)
constexpr int HD_PIX = UNERF_LPIPS_HEAD_PIXELS, HD_THREADS = 256, HD_WAVES = HD_THREADS / 64;
constexpr int EW_THREADS = UNERF_LPIPS_EW_THREADS, EW_MAX_WG = UNERF_LPIPS_EW_MAX_WG;   // the elementwise kernels stride beyond EW_MAX_WG workgroups
constexpr double LP_NORM_EPS = 1e-8;                     // metrics.LPIPS_NORM_EPS

static_assert(CV_BM == 64 && CV_BN == 64, "lp_conv_kernel: four waves, one 32 x 32 quarter of a 64 x 64 tile each");

typedef float lp_f32x16 __attribute__((ext_vector_type(16)));

inline size_t lp_al256(size_t x) { return (x + 255) & ~(size_t)255; }

struct lp_consts { float shift[3], scale[3]; };

// ---- input pack -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EW_THREADS) void lp_pack_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                             uint32_t n3 /* 3 n */, lp_consts k, float* __restrict__ act,
                                                             uint32_t* __restrict__ bad) {
    const uint32_t b = blockIdx.y, B = gridDim.y;
    const float* __restrict__ p = pred + (size_t)b * n3;
    const float* __restrict__ t = target + (size_t)b * n3;
    float* __restrict__ ap = act + (size_t)b * n3;
    float* __restrict__ at = act + (size_t)(B + b) * n3;
    uint32_t count = 0;
    for (uint32_t i = blockIdx.x * EW_THREADS + threadIdx.x; i < n3; i += gridDim.x * EW_THREADS) {
        const uint32_t c = i % 3u;
        float x = p[i];
        x = x > 1.f ? 1.f : x;                      // torch.clip(max=1): a NaN stays one
        const float y = t[i];
        count += !(x >= 0.f && x <= 1.f);
        count += !(y >= 0.f && y <= 1.f);
        ap[i] = ((2.f * x - 1.f) - k.shift[c]) / k.scale[c];
        at[i] = ((2.f * y - 1.f) - k.shift[c]) / k.scale[c];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) count += (uint32_t)__shfl_xor((int)count, o);
    if ((threadIdx.x & 63) == 0 && count) atomicAdd(&bad[b], count);
}

// ---- convolution ----------------------------------------------------------------------------------------------------
struct lp_conv_args {
    int N, H, W, Ci, Co, ks, stride, pad, Ho, Wo, M, K, relu;
};

__global__ __launch_bounds__(CV_THREADS) void lp_conv_kernel(const float* __restrict__ in, const float* __restrict__ wk,
                                                             const float* __restrict__ bias, float* __restrict__ out,
                                                             lp_conv_args g) {
    __shared__ float As[CV_BK][CV_BM + 1];      // [k][pixel]; + 1: the staging writes of one pixel walk k, i.e. rows
    __shared__ float Bs[CV_BK][CV_BN];          // [k][channel]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m0 = blockIdx.x * CV_BM, n0 = blockIdx.y * CV_BN;

    // staging roles: thread t gathers k-column (t & 15) of the pixels (t >> 4) + 16 j, and weight row (t >> 6) + 4 j,
    // channel (t & 63)
    const int kl = t & (CV_BK - 1);
    int iy0[CV_AROWS], ix0[CV_AROWS], pix0[CV_AROWS];
#pragma unroll
    for (int j = 0; j < CV_AROWS; ++j) {
        const int m = m0 + (t >> 4) + 16 * j;
        if (m < g.M) {
            const int img = m / (g.Ho * g.Wo), r = m - img * (g.Ho * g.Wo);
            const int oy = r / g.Wo, ox = r - oy * g.Wo;
            iy0[j] = oy * g.stride - g.pad;
            ix0[j] = ox * g.stride - g.pad;
            pix0[j] = img * g.H * g.W;
        } else {                                 // a row past the last pixel: every tap fails the bounds test
            iy0[j] = -(1 << 28);
            ix0[j] = 0;
            pix0[j] = 0;
        }
    }
    float ra[CV_AROWS], rb[CV_BROWS];
    auto fetch = [&](int k0) {
        const int k = k0 + kl;
        const bool kin = k < g.K;
        const int tap = kin ? k / g.Ci : 0, c = k - tap * g.Ci;
        const int ky = tap / g.ks, kx = tap - ky * g.ks;
#pragma unroll
        for (int j = 0; j < CV_AROWS; ++j) {
            const int iy = iy0[j] + ky, ix = ix0[j] + kx;
            const bool ok = kin && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
            ra[j] = ok ? in[(size_t)(pix0[j] + iy * g.W + ix) * g.Ci + c] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < CV_BROWS; ++j) {
            const int kb = k0 + (t >> 6) + 4 * j;
            rb[j] = kb < g.K ? wk[(size_t)kb * g.Co + n0 + (t & 63)] : 0.f;
        }
    };

    lp_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int arow = (wave & 1) * 32 + (lane & 31), bcol = (wave >> 1) * 32 + (lane & 31), khalf = lane >> 5;

    fetch(0);
    for (int k0 = 0; k0 < g.K; k0 += CV_BK) {
        __syncthreads();                         // the MFMAs of the previous step have read the tiles
#pragma unroll
        for (int j = 0; j < CV_AROWS; ++j) As[kl][(t >> 4) + 16 * j] = ra[j];
#pragma unroll
        for (int j = 0; j < CV_BROWS; ++j) Bs[(t >> 6) + 4 * j][t & 63] = rb[j];
        __syncthreads();
        if (k0 + CV_BK < g.K) fetch(k0 + CV_BK);
#pragma unroll
        for (int kk = 0; kk < CV_BK / 2; ++kk)   // lane l supplies A[l & 31][l >> 5] and B[l >> 5][l & 31]
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * kk + khalf][arow], Bs[2 * kk + khalf][bcol], acc, 0, 0, 0);
    }

    // C/D map of the 32 x 32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int n = n0 + bcol;
    const float bn = bias[n];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + (wave & 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
        if (m < g.M) {
            float v = acc[r] + bn;
            if (g.relu) v = v < 0.f ? 0.f : v;
            out[(size_t)m * g.Co + n] = v;
        }
    }
}

// ---- max-pool 3 / 2 -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EW_THREADS) void lp_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W,
                                                             int C, int Ho, int Wo, size_t total) {
    for (size_t i = (size_t)blockIdx.x * EW_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * EW_THREADS) {
        const int c = (int)(i % (size_t)C);
        size_t r = i / (size_t)C;
        const int ox = (int)(r % (size_t)Wo);
        r /= (size_t)Wo;
        const int oy = (int)(r % (size_t)Ho);
        const size_t img = r / (size_t)Ho;
        const float* __restrict__ p = in + ((img * H + 2 * oy) * W + 2 * ox) * (size_t)C + c;
        float m = p[0];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const float v = p[((size_t)dy * W + dx) * C];
                m = (v > m || v != v) ? v : m;
            }
        out[i] = m;
    }
}

// ---- head -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double lp_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);     // a butterfly: every lane ends with the same bits
    return v;
}

// grid (ceil(P / HD_PIX), B).  Wave w of a workgroup walks pixels w, w + 4, ... of the workgroup's range, the lanes over
// the channels; the wave's pixel sums are added in that order, the four waves' sums in wave order.
__global__ __launch_bounds__(HD_THREADS) void lp_head_kernel(const float* __restrict__ feats, const float* __restrict__ lin,
                                                             uint32_t P, int C, double* __restrict__ partial) {
    __shared__ double wsum[HD_WAVES];
    const uint32_t b = blockIdx.y, B = gridDim.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t p0 = blockIdx.x * HD_PIX, p1 = min(p0 + (uint32_t)HD_PIX, P);
    double acc = 0.0;
    for (uint32_t p = p0 + wave; p < p1; p += HD_WAVES) {
        const float* __restrict__ f0 = feats + ((size_t)b * P + p) * C;
        const float* __restrict__ f1 = feats + ((size_t)(B + b) * P + p) * C;
        double s0 = 0.0, s1 = 0.0;
        for (int c = lane; c < C; c += 64) {
            const double a = (double)f0[c], d = (double)f1[c];
            s0 += a * a;
            s1 += d * d;
        }
        const double n0 = sqrt(LP_NORM_EPS + lp_wave_sum(s0)), n1 = sqrt(LP_NORM_EPS + lp_wave_sum(s1));
        double s = 0.0;
        for (int c = lane; c < C; c += 64) {
            const double d = (double)f0[c] / n0 - (double)f1[c] / n1;
            s += (double)lin[c] * (d * d);
        }
        acc += lp_wave_sum(s);
    }
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = wsum[0];
#pragma unroll
        for (int w = 1; w < HD_WAVES; ++w) v += wsum[w];
        partial[(size_t)b * gridDim.x + blockIdx.x] = v;
    }
}

// lp_sum_kernel and lp_counts_kernel have one thread per image and are launched as ONE block of 64 threads
static_assert(UNERF_METRICS_MAX_IMAGES <= 64, "lp_sum_kernel / lp_counts_kernel: one block of 64 threads covers every image of a call");

// one thread per image adds its partials in index order
__global__ void lp_sum_kernel(const double* __restrict__ partial, uint32_t nblk, int B, double* __restrict__ out, int64_t out_stride) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double v = 0.0;
    for (uint32_t i = 0; i < nblk; ++i) v += partial[(size_t)b * nblk + i];
    out[(size_t)b * out_stride] = v;
}

// the slots of a row that are not sums: pixel counts and the count of refused input values
struct lp_counts { double pixels[LP_LAYERS]; };
__global__ void lp_counts_kernel(const uint32_t* __restrict__ bad, lp_counts k, int B, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
#pragma unroll
    for (int l = 0; l < LP_LAYERS; ++l) out[(size_t)b * UNERF_LPIPS_ROW + LP_LAYERS + l] = k.pixels[l];
    out[(size_t)b * UNERF_LPIPS_ROW + UNERF_LPIPS_BAD_OFF] = (double)bad[b];
}

// ---- host -----------------------------------------------------------------------------------------------------------
struct lp_layer { int ks, stride, pad, Ci, Co; };
const lp_layer LP_NET[LP_LAYERS] = {{11, 4, 2, 3, 64}, {5, 1, 2, 64, 192}, {3, 1, 1, 192, 384}, {3, 1, 1, 384, 256}, {3, 1, 1, 256, 256}};

inline int lp_conv_out(int x, int ks, int stride, int pad) { return (x + 2 * pad - ks) / stride + 1; }
inline int lp_pool_out(int x) { return (x - 3) / 2 + 1; }
inline uint32_t lp_ew_grid(size_t total) { return (uint32_t)std::min<size_t>((total + EW_THREADS - 1) / EW_THREADS, EW_MAX_WG); }

struct lp_plan {
    int h[LP_LAYERS], w[LP_LAYERS];      // the taps
    int ph[2], pw[2];                    // the two pooled maps (inputs of conv2 and conv3)
    size_t bad, act, conv[LP_LAYERS], pool[2], partial[LP_LAYERS], total;
    uint32_t nblk[LP_LAYERS];
};

lp_plan lp_make_plan(int H, int W, int B) {
    lp_plan L{};
    const size_t n2 = 2 * (size_t)B;
    L.h[0] = lp_conv_out(H, 11, 4, 2); L.w[0] = lp_conv_out(W, 11, 4, 2);
    L.ph[0] = lp_pool_out(L.h[0]);     L.pw[0] = lp_pool_out(L.w[0]);
    L.h[1] = L.ph[0];                  L.w[1] = L.pw[0];
    L.ph[1] = lp_pool_out(L.h[1]);     L.pw[1] = lp_pool_out(L.w[1]);
    for (int l = 2; l < LP_LAYERS; ++l) { L.h[l] = L.ph[1]; L.w[l] = L.pw[1]; }
    size_t o = 0;
    L.bad = o; o = lp_al256(o + (size_t)B * sizeof(uint32_t));
    L.act = o; o = lp_al256(o + n2 * H * W * 3 * sizeof(float));
    for (int l = 0; l < LP_LAYERS; ++l) {
        L.conv[l] = o; o = lp_al256(o + n2 * L.h[l] * L.w[l] * LP_NET[l].Co * sizeof(float));
        if (l < 2) { L.pool[l] = o; o = lp_al256(o + n2 * L.ph[l] * L.pw[l] * LP_NET[l].Co * sizeof(float)); }
    }
    for (int l = 0; l < LP_LAYERS; ++l) {
        L.nblk[l] = (uint32_t)(((size_t)L.h[l] * L.w[l] + HD_PIX - 1) / HD_PIX);
        L.partial[l] = o; o = lp_al256(o + (size_t)B * L.nblk[l] * sizeof(double));
    }
    L.total = o;
    return L;
}

bool lp_size_ok(int H, int W, int B) {
    return B >= 1 && B <= UNERF_METRICS_MAX_IMAGES && H >= UNERF_LPIPS_MIN_SIDE && W >= UNERF_LPIPS_MIN_SIDE &&
           6 * (int64_t)B * H * W < ((int64_t)1 << 31);
}

int lp_conv_check(const char* who, int N, int H, int W, int Ci, int Co, int ks, int stride, int pad) {
    UNERF_REQUIRE(N >= 1 && H >= 1 && W >= 1 && Ci >= 1 && Co >= 1 && ks >= 1 && stride >= 1 && pad >= 0 && pad < ks,
                  "%s: N = %d, H = %d, W = %d, C_in = %d, C_out = %d, ks = %d, stride = %d, pad = %d", who, N, H, W, Ci, Co, ks, stride, pad);
    UNERF_REQUIRE(Co % CV_BN == 0, "%s: C_out = %d is not a multiple of the column tile (%d)", who, Co, CV_BN);
    UNERF_REQUIRE(H + 2 * pad >= ks && W + 2 * pad >= ks, "%s: a %d x %d map is smaller than the %d x %d window (pad %d)", who, H, W, ks, ks, pad);
    const int64_t Ho = lp_conv_out(H, ks, stride, pad), Wo = lp_conv_out(W, ks, stride, pad);
    UNERF_REQUIRE((int64_t)N * H * W < ((int64_t)1 << 31) && (int64_t)N * Ho * Wo < ((int64_t)1 << 31) - CV_BM &&
                  (int64_t)ks * ks * Ci < ((int64_t)1 << 31) - CV_BK,
                  "%s: more than 2^31 input pixels, output pixels or reduction terms", who);
    return UNERF_OK;
}

void lp_conv_launch(const float* in, const float* w, const float* bias, float* out, int N, int H, int W, int Ci, int Co, int ks,
                    int stride, int pad, int relu, hipStream_t st) {
    lp_conv_args g;
    g.N = N; g.H = H; g.W = W; g.Ci = Ci; g.Co = Co; g.ks = ks; g.stride = stride; g.pad = pad; g.relu = relu;
    g.Ho = lp_conv_out(H, ks, stride, pad);
    g.Wo = lp_conv_out(W, ks, stride, pad);
    g.M = N * g.Ho * g.Wo;
    g.K = ks * ks * Ci;
    const dim3 grid((uint32_t)((g.M + CV_BM - 1) / CV_BM), (uint32_t)(Co / CV_BN));
    hipLaunchKernelGGL(lp_conv_kernel, grid, dim3(CV_THREADS), 0, st, in, w, bias, out, g);
}

void lp_pool_launch(const float* in, float* out, int N, int H, int W, int C, hipStream_t st) {
    const int Ho = lp_pool_out(H), Wo = lp_pool_out(W);
    const size_t total = (size_t)N * Ho * Wo * C;
    hipLaunchKernelGGL(lp_pool_kernel, dim3(lp_ew_grid(total)), dim3(EW_THREADS), 0, st, in, out, H, W, C, Ho, Wo, total);
}

void lp_head_launch(const float* feats, const float* lin, uint32_t P, int C, int B, double* partial, double* out, int64_t out_stride,
                    hipStream_t st) {
    const uint32_t nblk = (P + HD_PIX - 1) / HD_PIX;
    hipLaunchKernelGGL(lp_head_kernel, dim3(nblk, B), dim3(HD_THREADS), 0, st, feats, lin, P, C, partial);
    hipLaunchKernelGGL(lp_sum_kernel, dim3(1), dim3(64), 0, st, (const double*)partial, nblk, B, out, out_stride);
}

lp_consts lp_consts_of(const unerf_lpips_weights* w) {
    lp_consts k;
    for (int c = 0; c < 3; ++c) { k.shift[c] = w->shift[c]; k.scale[c] = w->scale[c]; }
    return k;
}

int lp_scale_check(const char* who, const unerf_lpips_weights* w) {
    for (int c = 0; c < 3; ++c)
        UNERF_REQUIRE(fabsf(w->shift[c]) <= FLT_MAX && fabsf(w->scale[c]) <= FLT_MAX && w->scale[c] != 0.f,
                      "%s: shift[%d] = %g, scale[%d] = %g (expected finite values and a non-zero scale)", who, c, (double)w->shift[c], c,
                      (double)w->scale[c]);
    return UNERF_OK;
}

}  // namespace

extern "C" int unerf_lpips_pack(const float* pred, const float* target, int64_t n, int B, const unerf_lpips_weights* w, float* act,
                                uint32_t* bad, void* stream) {
    const char* who = "lpips_pack";
    UNERF_REQUIRE(n >= 1, "%s: n = %lld", who, (long long)n);
    UNERF_REQUIRE(B >= 1 && B <= UNERF_METRICS_MAX_IMAGES, "%s: B = %d (expected 1..%d images)", who, B, UNERF_METRICS_MAX_IMAGES);
    UNERF_REQUIRE(6 * n * B < ((int64_t)1 << 31), "%s: 6 B n = %lld (must stay below 2^31)", who, (long long)(6 * n * B));
    UNERF_REQUIRE(pred && target && w && act && bad, "%s: null pointer (pred / target / weights / act / bad)", who);
    if (int rc = lp_scale_check(who, w)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(bad, 0, (size_t)B * sizeof(uint32_t), st) != hipSuccess) return unerf_check_launch(who);
    hipLaunchKernelGGL(lp_pack_kernel, dim3(lp_ew_grid((size_t)3 * n), B), dim3(EW_THREADS), 0, st, pred, target, (uint32_t)(3 * n),
                       lp_consts_of(w), act, bad);
    return unerf_check_launch(who);
}

extern "C" int unerf_conv2d_bias_relu(const float* in, const float* w, const float* bias, float* out, int N, int H, int W, int C_in,
                                      int C_out, int ks, int stride, int pad, int relu, void* stream) {
    const char* who = "conv2d_bias_relu";
    if (int rc = lp_conv_check(who, N, H, W, C_in, C_out, ks, stride, pad)) return rc;
    UNERF_REQUIRE(in && w && bias && out, "%s: null pointer (in / w / bias / out)", who);
    lp_conv_launch(in, w, bias, out, N, H, W, C_in, C_out, ks, stride, pad, relu, (hipStream_t)stream);
    return unerf_check_launch(who);
}

extern "C" int unerf_maxpool3s2(const float* in, float* out, int N, int H, int W, int C, void* stream) {
    const char* who = "maxpool3s2";
    UNERF_REQUIRE(N >= 1 && C >= 1 && H >= 3 && W >= 3, "%s: N = %d, H = %d, W = %d, C = %d (expected H, W >= 3)", who, N, H, W, C);
    UNERF_REQUIRE((int64_t)N * H * W < ((int64_t)1 << 31), "%s: more than 2^31 input pixels", who);
    UNERF_REQUIRE(in && out, "%s: null pointer (in / out)", who);
    lp_pool_launch(in, out, N, H, W, C, (hipStream_t)stream);
    return unerf_check_launch(who);
}

extern "C" int unerf_lpips_head(const float* feats, const float* lin_w, int64_t P, int C, int B, void* workspace, size_t workspace_bytes,
                                double* out, int64_t out_stride, void* stream) {
    const char* who = "lpips_head";
    UNERF_REQUIRE(P >= 1 && P < ((int64_t)1 << 31) - HD_PIX && C >= 1 && out_stride >= 1, "%s: P = %lld, C = %d, out_stride = %lld", who,
                  (long long)P, C, (long long)out_stride);
    UNERF_REQUIRE(B >= 1 && B <= UNERF_METRICS_MAX_IMAGES, "%s: B = %d (expected 1..%d images)", who, B, UNERF_METRICS_MAX_IMAGES);
    UNERF_REQUIRE(feats && lin_w && workspace && out, "%s: null pointer (feats / lin_w / workspace / out)", who);
    const size_t need = (size_t)B * (size_t)((P + HD_PIX - 1) / HD_PIX) * sizeof(double);
    UNERF_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    UNERF_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", who);
    lp_head_launch(feats, lin_w, (uint32_t)P, C, B, (double*)workspace, out, out_stride, (hipStream_t)stream);
    return unerf_check_launch(who);
}

extern "C" size_t unerf_lpips_workspace_bytes(int H, int W, int B) { return lp_size_ok(H, W, B) ? lp_make_plan(H, W, B).total : 0; }

extern "C" int unerf_lpips_batch(const float* pred, const float* target, int H, int W, int B, const unerf_lpips_weights* w,
                                 void* workspace, size_t workspace_bytes, double* out, void* stream) {
    const char* who = "lpips_batch";
    UNERF_REQUIRE(B >= 1 && B <= UNERF_METRICS_MAX_IMAGES, "%s: B = %d (expected 1..%d images)", who, B, UNERF_METRICS_MAX_IMAGES);
    UNERF_REQUIRE(H >= UNERF_LPIPS_MIN_SIDE && W >= UNERF_LPIPS_MIN_SIDE, "%s: a %d x %d image (min(H, W) >= %d: below it the second max-pool "
                  "has no output)", who, H, W, UNERF_LPIPS_MIN_SIDE);
    UNERF_REQUIRE(lp_size_ok(H, W, B), "%s: 6 B H W = %lld (must stay below 2^31)", who, (long long)(6 * (int64_t)B * H * W));
    UNERF_REQUIRE(pred && target && w && workspace && out, "%s: null pointer (pred / target / weights / workspace / out)", who);
    for (int l = 0; l < LP_LAYERS; ++l)
        UNERF_REQUIRE(w->conv_w[l] && w->conv_b[l] && w->lin_w[l], "%s: null pointer in the weights of layer %d", who, l);
    if (int rc = lp_scale_check(who, w)) return rc;
    const lp_plan L = lp_make_plan(H, W, B);
    UNERF_REQUIRE(workspace_bytes >= L.total, "%s: workspace of %zu bytes, unerf_lpips_workspace_bytes(%d, %d, %d) = %zu", who,
                  workspace_bytes, H, W, B, L.total);
    UNERF_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", who);
    const int N = 2 * B;
    for (int l = 0; l < LP_LAYERS; ++l) {
        const int ih = l == 0 ? H : l == 1 ? L.ph[0] : L.h[2], iw = l == 0 ? W : l == 1 ? L.pw[0] : L.w[2];
        if (int rc = lp_conv_check(who, N, ih, iw, LP_NET[l].Ci, LP_NET[l].Co, LP_NET[l].ks, LP_NET[l].stride, LP_NET[l].pad)) return rc;
    }

    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    uint32_t* bad = (uint32_t*)(ws + L.bad);
    float* act = (float*)(ws + L.act);
    if (hipMemsetAsync(bad, 0, (size_t)B * sizeof(uint32_t), st) != hipSuccess) return unerf_check_launch(who);
    const size_t n3 = (size_t)3 * H * W;
    hipLaunchKernelGGL(lp_pack_kernel, dim3(lp_ew_grid(n3), B), dim3(EW_THREADS), 0, st, pred, target, (uint32_t)n3, lp_consts_of(w), act, bad);
    const float* x = act;
    int xh = H, xw = W;
    lp_counts counts;
    for (int l = 0; l < LP_LAYERS; ++l) {
        const lp_layer& n = LP_NET[l];
        float* y = (float*)(ws + L.conv[l]);
        lp_conv_launch(x, w->conv_w[l], w->conv_b[l], y, N, xh, xw, n.Ci, n.Co, n.ks, n.stride, n.pad, 1, st);
        lp_head_launch(y, w->lin_w[l], (uint32_t)(L.h[l] * L.w[l]), n.Co, B, (double*)(ws + L.partial[l]), out + l, UNERF_LPIPS_ROW, st);
        counts.pixels[l] = (double)L.h[l] * (double)L.w[l];
        x = y; xh = L.h[l]; xw = L.w[l];
        if (l < 2) {
            float* p = (float*)(ws + L.pool[l]);
            lp_pool_launch(y, p, N, xh, xw, n.Co, st);
            x = p; xh = L.ph[l]; xw = L.pw[l];
        }
    }
    hipLaunchKernelGGL(lp_counts_kernel, dim3(1), dim3(64), 0, st, (const uint32_t*)bad, counts, B, out);
    return unerf_check_launch(who);
}
