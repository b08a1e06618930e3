// Eval-metric half of libunerf: the per-image metric stage of the eval harness (eval.image_metrics_unc /
// depth_metrics_unc) as a handful of kernels that leave ONE row of float64 partial results in device memory.
// gfx950 only; wave = 64.  See include/unerf.h (unerf_image_metrics) for the contract and the row layout.
//
//   mt_stats      one pass over pred / target / sigma / mask: the float32 error vectors (written out as sort keys: a
//                 non-negative finite float orders like its bit pattern), float64 plain sums, NLL, min / max, the count of
//                 non-finite inputs, and the AUCE histogram (each pixel-channel finds its place among the <= 128 sorted
//                 thresholds; per-workgroup LDS histogram, then INTEGER global atomics: order-free, so repeatable)
//   mt_reduce     the per-workgroup slab rows -> row[0..11], fixed order
//   ms_hist / ms_rowscan / ms_scatter   a stable LSD radix sort, 8-bit digits, four passes, run three times
//                 (keys sq, ab alone; key var with the pixel index as payload)
//   mt_segsum     float64 sums of the sorted values over [0, keep_k) for every cut rank: per-block totals + the partial
//                 sum of the one block a cut falls into
//   mt_ssim       11x11 gaussian SSIM, separable through an LDS tile, the five window sums in float64
//   mt_finish     block totals -> prefix -> the AUSE sums; histogram -> AUCE counts; SSIM slab -> sum
// Every float64 sum goes wave butterfly -> LDS -> slab -> one reducer in a fixed order: two calls on the same inputs
// give the same bits.  Built with -ffp-contract=off like the rest: the float32 error definitions and the cut ranks
// (int64)((1 - r) n) are the host's IEEE operations, and the float64 products below fuse only where fma() says so.
//
// A batch (unerf_image_metrics_batch) is B images of one size in ONE grid of each kernel: the image is blockIdx.y, and
// everything an image reads or writes -- its slice of the input stacks, its region of the workspace, its row of `out` --
// is the single-image pointer moved by a 64-bit per-image stride (mt_img).  blockIdx.x, and with it every fixed-order
// reduction, is what it is for that image alone: row b of a batch is the row of image b scored alone, bit for bit.
// unerf_image_metrics is the B = 1 case.
//
// The rendered images of the same stage (unerf_eval_images_batch: ground truth, prediction, absolute error and the
// jet-coloured std as final 8-bit planes) follow: ei_range / ei_pack.  The pose normal equations (unerf_pose_normal_eq_*:
// the float64 reduction of a frame's pose Jacobian, on this file's wave_sum / block_sum) are at the end: pn_accumulate / pn_finish.
#include "unerf_common.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace {

constexpr int MT_THREADS = 256;          // stats / segsum / ssim / sort workgroups: 4 waves
constexpr int MT_WAVES = MT_THREADS / 64;
constexpr int MT_MAX_WG = 1024;          // slab rows (stats, segsum): one reducer workgroup reads them all
constexpr int MT_NSTAT = 12;             // row[0..11], see include/unerf.h
constexpr int MT_MAXK = 128;             // n_ratios, n_z
constexpr int MT_SSIM_WG = 2048;
constexpr int MS_ITEMS = 16;             // keys per lane and pass
constexpr int MS_TILE = MT_THREADS * MS_ITEMS;
constexpr int MT_FAM = 4;                // sq by sq, ab by ab, sq by var, ab by var
constexpr int SS_TW = 32, SS_TH = 16, SS_K = 11, SS_IW = SS_TW + SS_K - 1, SS_IH = SS_TH + SS_K - 1;

struct MtZTable {       // thresholds sorted ascending + where each goes in the caller's order
    double z[MT_MAXK];
    int perm[MT_MAXK];
    int n_z;
};
struct MtRatios {
    double r[MT_MAXK];
    int n;
};
struct MtGauss {
    double g[SS_K];
};

struct MtLayout {
    size_t zeroed, auce_cnt, seg_part, stat_slab, ssim_slab, seg_block, dtot, table, ksq, kab, kvar, tmp0, tmp1, idx0, idx1, total;
    size_t zero_bytes;
    uint32_t nblocks;
    // a batch keeps the accumulated regions of its B images next to each other in front (one memset clears them all) and
    // the B remainders behind them; the offsets above are image 0's, an image's own are these strides further on
    size_t zstride, rstride;
};
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
MtLayout mt_layout(int64_t n, int B) {
    MtLayout L;
    const size_t nb = B > 1 ? (size_t)B : 1;
    const size_t nn = n > 0 ? (size_t)n : 0;
    L.nblocks = (uint32_t)((nn + MS_TILE - 1) / MS_TILE);
    size_t o = 0;
    L.zeroed = o;                                   // one hipMemsetAsync covers the two regions that are accumulated into
    L.auce_cnt = o; o = al256(o + (MT_MAXK + 1) * sizeof(unsigned long long));
    L.seg_part = o; o = al256(o + MT_FAM * MT_MAXK * sizeof(double));
    L.zstride = o;
    L.zero_bytes = o * nb;
    o = L.zero_bytes;
    const size_t rest0 = o;
    L.stat_slab = o; o = al256(o + (size_t)MT_MAX_WG * MT_NSTAT * sizeof(double));
    L.ssim_slab = o; o = al256(o + (size_t)MT_SSIM_WG * sizeof(double));
    L.seg_block = o; o = al256(o + (size_t)MT_FAM * MT_MAX_WG * sizeof(double));
    L.dtot = o; o = al256(o + 256 * sizeof(uint32_t));
    L.table = o; o = al256(o + (size_t)256 * L.nblocks * sizeof(uint32_t));
    size_t* arr[7] = {&L.ksq, &L.kab, &L.kvar, &L.tmp0, &L.tmp1, &L.idx0, &L.idx1};
    for (size_t* a : arr) { *a = o; o = al256(o + nn * sizeof(uint32_t)); }
    L.rstride = o - rest0;
    L.total = rest0 + L.rstride * nb;
    return L;
}

// image blockIdx.y's copy of a per-image array, given image 0's and the distance between two images in BYTES; a pointer
// that is not there (no mask, no keys wanted, no payload) stays null
template <class T>
__device__ __forceinline__ T* mt_img(T* p, size_t stride_bytes) {
    return p ? (T*)((char*)p + (size_t)blockIdx.y * stride_bytes) : nullptr;
}
template <class T>
__device__ __forceinline__ const T* mt_img(const T* p, size_t stride_bytes) {
    return p ? (const T*)((const char*)p + (size_t)blockIdx.y * stride_bytes) : nullptr;
}
struct MtStrides {      // bytes from one image to the next
    size_t z, r;        // workspace: accumulated regions, the rest
};

// ---- fixed-order reductions ----------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// every thread gets the sum; sh holds NW doubles and may be reused right after the call returns
template <int NW>
__device__ __forceinline__ double block_sum(double v, double* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = sh[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) r += sh[w];
    return r;
}
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(x, o);
        if (lane >= o) x += t;
    }
    return x;
}
__device__ __forceinline__ bool mt_finite(float x) { return fabsf(x) <= FLT_MAX; }   // false for NaN and +-inf

// ---- pass 1: error vectors, plain sums, NLL, AUCE histogram ----------------------------
template <int C>
__global__ __launch_bounds__(MT_THREADS) void mt_stats_kernel(const float* __restrict__ pred0, const float* __restrict__ target0,
                                                              const float* __restrict__ sigma0, const uint8_t* __restrict__ mask0,
                                                              uint32_t n, float clip, float min_sigma, int flags, MtZTable zt,
                                                              uint32_t* __restrict__ ksq0, uint32_t* __restrict__ kab0,
                                                              uint32_t* __restrict__ kvar0, double* __restrict__ slab0,
                                                              unsigned long long* __restrict__ auce_cnt0, MtStrides sd) {
    const float* __restrict__ pred = mt_img(pred0, (size_t)n * C * sizeof(float));
    const float* __restrict__ target = mt_img(target0, (size_t)n * C * sizeof(float));
    const float* __restrict__ sigma = mt_img(sigma0, (size_t)n * sizeof(float));
    const uint8_t* __restrict__ mask = mt_img(mask0, (size_t)n);
    uint32_t* __restrict__ ksq = mt_img(ksq0, sd.r);
    uint32_t* __restrict__ kab = mt_img(kab0, sd.r);
    uint32_t* __restrict__ kvar = mt_img(kvar0, sd.r);
    double* __restrict__ slab = mt_img(slab0, sd.r);
    unsigned long long* __restrict__ auce_cnt = mt_img(auce_cnt0, sd.z);
    __shared__ double zs[MT_MAXK];
    __shared__ uint32_t hist[MT_MAXK + 1];
    __shared__ double red[MT_WAVES];
    __shared__ float redf[MT_WAVES];
    const bool want_auce = flags & UNERF_METRICS_AUCE, want_nll = flags & UNERF_METRICS_NLL;
    for (int i = threadIdx.x; i <= MT_MAXK; i += MT_THREADS) {
        hist[i] = 0u;
        if (i < MT_MAXK) zs[i] = i < zt.n_z ? zt.z[i] : 0.0;
    }
    __syncthreads();
    double a_sq = 0, a_ab = 0, a_var = 0, a_sig = 0, a_sq64 = 0, a_nll = 0;
    uint32_t c_valid = 0, c_bad = 0;
    float pmin = INFINITY, pmax = -INFINITY, tmin = INFINITY, tmax = -INFINITY;
    const double half_log_2pi = 0.91893853320467274178;
    for (uint32_t i = blockIdx.x * MT_THREADS + threadIdx.x; i < n; i += gridDim.x * MT_THREADS) {
        const bool valid = mask ? mask[i] != 0 : true;
        uint32_t k_sq = 0xFFFFFFFFu, k_ab = 0xFFFFFFFFu, k_var = 0xFFFFFFFFu;   // left-out pixels sort behind every cut
        if (valid) {
            const float sg = sigma[i];
            float sq = 0.f, ab = 0.f;
            bool bad = !mt_finite(sg);
            const double sg64 = (double)sg;
            const double s = fmax(sg64, (double)min_sigma);
            const double log_s = want_nll ? log(s) : 0.0, two_s2 = 2.0 * (s * s);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float p_raw = pred[(size_t)i * C + c], t = target[(size_t)i * C + c];
                bad = bad || !mt_finite(p_raw) || !mt_finite(t);
                // the clipped copy is what psnr and SSIM see (eval_uncertainty.py:681); the error vectors, the NLL and the
                // AUCE take the prediction as rendered (:316)
                const float p = fminf(p_raw, clip);
                const float d = p_raw - t;
                sq = sq + d * d;
                ab = ab + fabsf(d);
                pmin = fminf(pmin, p); pmax = fmaxf(pmax, p);
                tmin = fminf(tmin, t); tmax = fmaxf(tmax, t);
                const double d64 = (double)t - (double)p_raw;
                const double d2 = d64 * d64;
                const double dc64 = (double)t - (double)p;
                a_sq64 += p == p_raw ? d2 : dc64 * dc64;
                if (want_nll) a_nll += (d2 / two_s2 + log_s) + half_log_2pi;
                if (want_auce) {
                    const double r = fabs(d64);
                    const double ratio = sg64 > 0.0 ? r / sg64 : (r == 0.0 ? 0.0 : (double)INFINITY);
                    int lo = 0, hi = zt.n_z;      // -> the number of thresholds that do NOT cover this element
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (!(ratio <= zs[mid])) lo = mid + 1; else hi = mid;
                    }
                    atomicAdd(&hist[lo], 1u);
                }
            }
            const float var = sg * sg;
            a_sq += (double)sq; a_ab += (double)ab; a_var += (double)var; a_sig += sg64;
            c_valid += 1u; c_bad += bad ? 1u : 0u;
            k_sq = __float_as_uint(sq) == 0x80000000u ? 0u : __float_as_uint(sq);
            k_ab = __float_as_uint(ab) == 0x80000000u ? 0u : __float_as_uint(ab);
            k_var = __float_as_uint(var) == 0x80000000u ? 0u : __float_as_uint(var);
        }
        if (ksq) { ksq[i] = k_sq; kab[i] = k_ab; kvar[i] = k_var; }
    }
    double* row = slab + (size_t)blockIdx.x * MT_NSTAT;
    const double sums[8] = {(double)c_valid, (double)c_bad, a_sq, a_ab, a_var, a_sig, a_sq64, a_nll};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const double r = block_sum<MT_WAVES>(sums[j], red);
        if (threadIdx.x == 0) row[j] = r;
    }
    const float mm[4] = {pmin, pmax, tmin, tmax};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float v = (j & 1) ? wave_max(mm[j]) : wave_min(mm[j]);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) redf[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            float r = redf[0];
            for (int w = 1; w < MT_WAVES; ++w) r = (j & 1) ? fmaxf(r, redf[w]) : fminf(r, redf[w]);
            row[8 + j] = (double)r;
        }
    }
    if (want_auce) {
        __syncthreads();
        for (int i = threadIdx.x; i <= zt.n_z; i += MT_THREADS)
            if (hist[i]) atomicAdd(&auce_cnt[i], (unsigned long long)hist[i]);
    }
}

// slab [nwg, 12] -> out[0..11]; one workgroup of 1024 per image, row t on thread t
__global__ __launch_bounds__(1024) void mt_reduce_kernel(const double* __restrict__ slab0, int nwg, double* __restrict__ out0, MtStrides sd) {
    __shared__ double red[16];
    const double* __restrict__ slab = mt_img(slab0, sd.r);
    double* __restrict__ out = mt_img(out0, UNERF_METRICS_ROW * sizeof(double));
    const int t = threadIdx.x;
    for (int j = 0; j < MT_NSTAT; ++j) {
        if (j < 8) {
            const double r = block_sum<16>(t < nwg ? slab[(size_t)t * MT_NSTAT + j] : 0.0, red);
            if (t == 0) out[j] = r;
        } else {
            const bool is_max = j & 1;
            float v = t < nwg ? (float)slab[(size_t)t * MT_NSTAT + j] : (is_max ? -INFINITY : INFINITY);
            v = is_max ? wave_max(v) : wave_min(v);
            __syncthreads();
            if ((t & 63) == 0) red[t >> 6] = (double)v;
            __syncthreads();
            if (t == 0) {
                double r = red[0];
                for (int w = 1; w < 16; ++w) r = is_max ? fmax(r, red[w]) : fmin(r, red[w]);
                out[j] = r;
            }
        }
    }
}

// ---- stable LSD radix sort, 8-bit digits -------------------------------------------------
// A tile is 4096 consecutive slots; wave w owns slots [1024 w, 1024 (w + 1)) of it and visits them 64 at a time, so
// "tile, wave, step, lane" is slot order and every rank below is taken in that order: equal digits keep their order.
__global__ __launch_bounds__(MT_THREADS) void ms_hist_kernel(const uint32_t* __restrict__ keys0, uint32_t n, int shift,
                                                             uint32_t* __restrict__ table0, uint32_t nblocks, MtStrides sd) {
    __shared__ uint32_t h[256];
    const uint32_t* __restrict__ keys = mt_img(keys0, sd.r);
    uint32_t* __restrict__ table = mt_img(table0, sd.r);
    h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t base = blockIdx.x * MS_TILE;
#pragma unroll 4
    for (int i = 0; i < MS_ITEMS; ++i) {
        const uint32_t pos = base + i * MT_THREADS + threadIdx.x;
        if (pos < n) atomicAdd(&h[(keys[pos] >> shift) & 255u], 1u);
    }
    __syncthreads();
    table[(size_t)threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];   // digit-major
}

// workgroup d: exclusive scan of digit d's row of the table in place, the row's total -> dtot[d]
__global__ __launch_bounds__(1024) void ms_rowscan_kernel(uint32_t* __restrict__ table0, uint32_t nblocks, uint32_t* __restrict__ dtot0,
                                                          MtStrides sd) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t carry_sh;
    uint32_t* __restrict__ table = mt_img(table0, sd.r);
    uint32_t* __restrict__ dtot = mt_img(dtot0, sd.r);
    uint32_t* row = table + (size_t)blockIdx.x * nblocks;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) carry_sh = 0u;
    __syncthreads();
    for (uint32_t base = 0; base < nblocks; base += 1024) {
        const uint32_t i = base + t;
        const uint32_t x = i < nblocks ? row[i] : 0u;
        const uint32_t incl = wave_incl_scan(x);
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        uint32_t before = carry_sh;
        for (int v = 0; v < w; ++v) before += wsum[v];
        if (i < nblocks) row[i] = before + incl - x;
        __syncthreads();
        if (t == 1023) carry_sh = before + incl;
        __syncthreads();
    }
    if (t == 0) dtot[blockIdx.x] = carry_sh;
}

template <bool IDX_IN, bool IDX_OUT>
__global__ __launch_bounds__(MT_THREADS) void ms_scatter_kernel(const uint32_t* __restrict__ kin0, const uint32_t* __restrict__ iin0,
                                                                uint32_t* __restrict__ kout0, uint32_t* __restrict__ iout0, uint32_t n,
                                                                int shift, const uint32_t* __restrict__ table0,
                                                                const uint32_t* __restrict__ dtot0, uint32_t nblocks, MtStrides sd) {
    __shared__ uint32_t cnt[MT_WAVES][256];
    __shared__ uint32_t wsum[MT_WAVES];
    const uint32_t* __restrict__ kin = mt_img(kin0, sd.r);
    const uint32_t* __restrict__ iin = mt_img(iin0, sd.r);
    uint32_t* __restrict__ kout = mt_img(kout0, sd.r);
    uint32_t* __restrict__ iout = mt_img(iout0, sd.r);
    const uint32_t* __restrict__ table = mt_img(table0, sd.r);
    const uint32_t* __restrict__ dtot = mt_img(dtot0, sd.r);
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    volatile uint32_t* mycnt = cnt[w];
#pragma unroll
    for (int v = 0; v < MT_WAVES; ++v) cnt[v][t] = 0u;
    // where digit t starts in the output: exclusive scan of the 256 digit totals
    const uint32_t dv = dtot[t];
    const uint32_t dincl = wave_incl_scan(dv);
    if (lane == 63) wsum[w] = dincl;
    __syncthreads();
    uint32_t dbase = dincl - dv;
    for (int v = 0; v < w; ++v) dbase += wsum[v];

    const unsigned long long lt = (1ull << lane) - 1ull;
    const uint32_t slot0 = blockIdx.x * MS_TILE + w * (64 * MS_ITEMS) + lane;
    uint32_t key[MS_ITEMS], off[MS_ITEMS];
#pragma unroll
    for (int i = 0; i < MS_ITEMS; ++i) {
        const uint32_t pos = slot0 + i * 64;
        const bool valid = pos < n;
        key[i] = valid ? kin[pos] : 0xFFFFFFFFu;
        const uint32_t d = (key[i] >> shift) & 255u;
        unsigned long long peers = __ballot(valid);          // the lanes of this step that hold the same digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const int leader = peers ? __builtin_ctzll(peers) : 0;
        uint32_t pre = 0u;
        if (valid && lane == leader) {                        // one lane per digit moves the wave's counter
            pre = mycnt[d];
            mycnt[d] = pre + (uint32_t)__builtin_popcountll(peers);
        }
        __builtin_amdgcn_wave_barrier();
        pre = __shfl(pre, leader);
        off[i] = pre + (uint32_t)__builtin_popcountll(peers & lt);
    }
    __syncthreads();
    {   // counters -> starts: the digit's start, + this tile's share of the table, + the waves in front
        uint32_t run = dbase + table[(size_t)t * nblocks + blockIdx.x];
#pragma unroll
        for (int v = 0; v < MT_WAVES; ++v) {
            const uint32_t c = cnt[v][t];
            cnt[v][t] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MS_ITEMS; ++i) {
        const uint32_t pos = slot0 + i * 64;
        if (pos < n) {
            const uint32_t dst = cnt[w][(key[i] >> shift) & 255u] + off[i];
            if (dst < n) {      // always true for a consistent table; never store outside the buffer
                kout[dst] = key[i];
                if (IDX_OUT) iout[dst] = IDX_IN ? iin[pos] : pos;
            }
        }
    }
}

// ---- sums of the sorted values over [0, keep_k) --------------------------------------------
// block b owns slots [b per, (b + 1) per).  BY_VAR = false: the sorted keys ARE the values (family fam0).
// BY_VAR = true: idx -> the sq / ab keys of that pixel (families fam0, fam0 + 1).
__device__ __forceinline__ long long mt_keep(double ratio, double n_valid) {
    long long k = (long long)((1.0 - ratio) * n_valid);
    const long long nv = (long long)n_valid;
    return k < 0 ? 0 : (k > nv ? nv : k);
}
template <bool BY_VAR>
__global__ __launch_bounds__(MT_THREADS) void mt_segsum_kernel(const uint32_t* __restrict__ sorted0, const uint32_t* __restrict__ ksq0,
                                                               const uint32_t* __restrict__ kab0, uint32_t n, uint32_t per,
                                                               const double* __restrict__ row0, MtRatios rt, int fam0,
                                                               double* __restrict__ seg_block0, double* __restrict__ seg_part0, MtStrides sd) {
    __shared__ double red[MT_WAVES];
    __shared__ long long keep[MT_MAXK];
    const uint32_t* __restrict__ sorted = mt_img(sorted0, sd.r);
    const uint32_t* __restrict__ ksq = mt_img(ksq0, sd.r);
    const uint32_t* __restrict__ kab = mt_img(kab0, sd.r);
    const double* __restrict__ row = mt_img(row0, UNERF_METRICS_ROW * sizeof(double));     // the image's own n_valid
    double* __restrict__ seg_block = mt_img(seg_block0, sd.r);
    double* __restrict__ seg_part = mt_img(seg_part0, sd.z);
    const double n_valid = row[0];
    for (int k = threadIdx.x; k < rt.n; k += MT_THREADS) keep[k] = mt_keep(rt.r[k], n_valid);
    __syncthreads();
    const uint32_t nv = (uint32_t)n_valid;
    const uint32_t a = blockIdx.x * per;
    const uint32_t b = (a + per < nv && a + per > a) ? a + per : nv;   // values behind n_valid are not values
    constexpr int NF = BY_VAR ? 2 : 1;
    // limit = how far into the block to sum; the same loop gives the block total and a cut's partial sum
    auto range_sum = [&](uint32_t limit, double (&out)[NF]) {
        double acc[NF] = {};
        for (uint32_t j = a + threadIdx.x; j < limit; j += MT_THREADS) {
            if (BY_VAR) {
                const uint32_t px = sorted[j];
                if (px < n) {
                    acc[0] += (double)__uint_as_float(ksq[px]);
                    acc[NF - 1] += (double)__uint_as_float(kab[px]);
                }
            } else {
                acc[0] += (double)__uint_as_float(sorted[j]);
            }
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) out[f] = block_sum<MT_WAVES>(acc[f], red);
    };
    double tot[NF];
    range_sum(b, tot);
    if (threadIdx.x == 0)
        for (int f = 0; f < NF; ++f) seg_block[(size_t)(fam0 + f) * MT_MAX_WG + blockIdx.x] = tot[f];
    for (int k = 0; k < rt.n; ++k) {
        const long long kk = keep[k];
        if (kk / (long long)per != (long long)blockIdx.x) continue;    // uniform
        double part[NF];
        range_sum((uint32_t)kk, part);
        if (threadIdx.x == 0)
            for (int f = 0; f < NF; ++f) seg_part[(size_t)(fam0 + f) * MT_MAXK + k] = part[f];
    }
}

// ---- SSIM -----------------------------------------------------------------------------------
// One work item = a 32 x 16 tile of interior pixels of one channel: its 42 x 26 input pixels go to LDS, the rows are
// filtered into five float64 maps, the columns of those give the window sums.  Work items are dealt to the workgroups
// round-robin, each workgroup leaves one partial sum.
__global__ __launch_bounds__(MT_THREADS) void mt_ssim_kernel(const float* __restrict__ pred0, const float* __restrict__ target0, int H,
                                                             int W, int C, float clip, MtGauss gw, const double* __restrict__ row0,
                                                             double* __restrict__ slab0, MtStrides sd) {
    const size_t image_bytes = (size_t)H * W * C * sizeof(float);
    const float* __restrict__ pred = mt_img(pred0, image_bytes);
    const float* __restrict__ target = mt_img(target0, image_bytes);
    const double* __restrict__ row = mt_img(row0, UNERF_METRICS_ROW * sizeof(double));     // the image's own minima / maxima
    double* __restrict__ slab = mt_img(slab0, sd.r);
    __shared__ float sp[SS_IH][SS_IW], st[SS_IH][SS_IW];
    __shared__ double hor[5][SS_IH][SS_TW];
    __shared__ double red[MT_WAVES];
    const int OW = W - (SS_K - 1), OH = H - (SS_K - 1);
    const int tx_n = (OW + SS_TW - 1) / SS_TW, ty_n = (OH + SS_TH - 1) / SS_TH;
    const long long items = (long long)tx_n * ty_n * C;
    // data_range as metrics.ssim takes it: the float32 differences, the larger one
    const float rp = (float)row[9] - (float)row[8], rtg = (float)row[11] - (float)row[10];
    const double range = (double)fmaxf(rp, rtg);
    const double c1 = (0.01 * range) * (0.01 * range), c2 = (0.03 * range) * (0.03 * range);
    double acc = 0.0;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int c = (int)(it % C);
        const long long tile = it / C;
        const int ox = (int)(tile % tx_n) * SS_TW, oy = (int)(tile / tx_n) * SS_TH;
        __syncthreads();
        for (int e = threadIdx.x; e < SS_IH * SS_IW; e += MT_THREADS) {
            const int ly = e / SS_IW, lx = e % SS_IW;
            const int y = oy + ly, x = ox + lx;
            float p = 0.f, t = 0.f;
            if (y < H && x < W) {
                const size_t g = ((size_t)y * W + x) * C + c;
                p = fminf(pred[g], clip);
                t = target[g];
            }
            sp[ly][lx] = p;
            st[ly][lx] = t;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < SS_IH * SS_TW; e += MT_THREADS) {
            const int ly = e / SS_TW, lx = e % SS_TW;
            double m_p = 0, m_t = 0, e_pp = 0, e_tt = 0, e_pt = 0;
#pragma unroll
            for (int k = 0; k < SS_K; ++k) {
                const double p = (double)sp[ly][lx + k], t = (double)st[ly][lx + k], g = gw.g[k];
                m_p = fma(g, p, m_p);
                m_t = fma(g, t, m_t);
                e_pp = fma(g, p * p, e_pp);
                e_tt = fma(g, t * t, e_tt);
                e_pt = fma(g, p * t, e_pt);
            }
            hor[0][ly][lx] = m_p; hor[1][ly][lx] = m_t; hor[2][ly][lx] = e_pp; hor[3][ly][lx] = e_tt; hor[4][ly][lx] = e_pt;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < SS_TH * SS_TW; e += MT_THREADS) {
            const int ly = e / SS_TW, lx = e % SS_TW;
            if (oy + ly >= OH || ox + lx >= OW) continue;
            double v[5] = {};
#pragma unroll
            for (int k = 0; k < SS_K; ++k) {
                const double g = gw.g[k];
#pragma unroll
                for (int q = 0; q < 5; ++q) v[q] = fma(g, hor[q][ly + k][lx], v[q]);
            }
            const double mu_p = v[0], mu_t = v[1];
            const double s_pp = v[2] - mu_p * mu_p, s_tt = v[3] - mu_t * mu_t, s_pt = v[4] - mu_p * mu_t;
            const double upper = 2.0 * s_pt + c2, lower = (s_pp + s_tt) + c2;
            acc += ((2.0 * mu_p * mu_t + c1) * upper) / (((mu_p * mu_p + mu_t * mu_t) + c1) * lower);
        }
    }
    const double r = block_sum<MT_WAVES>(acc, red);
    if (threadIdx.x == 0) slab[blockIdx.x] = r;
}

// ---- the last kernel: per image, workgroups 0..3 the AUSE families, 4 the AUCE counts, 5 the SSIM sum -----
__global__ __launch_bounds__(1024) void mt_finish_kernel(const double* __restrict__ seg_block0, const double* __restrict__ seg_part0,
                                                         int seg_blocks, uint32_t per, MtRatios rt, const unsigned long long* __restrict__ auce_cnt0,
                                                         MtZTable zt, const double* __restrict__ ssim_slab0, int ssim_wg, double ssim_count,
                                                         int flags, double* __restrict__ out0, MtStrides sd) {
    __shared__ double sc[1025];
    __shared__ double red[16];
    const double* __restrict__ seg_block = mt_img(seg_block0, sd.r);
    const double* __restrict__ seg_part = mt_img(seg_part0, sd.z);
    const unsigned long long* __restrict__ auce_cnt = mt_img(auce_cnt0, sd.z);
    const double* __restrict__ ssim_slab = mt_img(ssim_slab0, sd.r);
    double* __restrict__ out = mt_img(out0, UNERF_METRICS_ROW * sizeof(double));
    const int t = threadIdx.x;
    if (blockIdx.x < MT_FAM) {
        if (!(flags & UNERF_METRICS_AUSE)) return;
        const int f = blockIdx.x;
        // prefix of the block totals: sc[i] = total of blocks [0, i) (wave scans, then the waves in front: a fixed order)
        {
            double x = t < seg_blocks ? seg_block[(size_t)f * MT_MAX_WG + t] : 0.0;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const double up = __shfl_up(x, o);
                if ((t & 63) >= o) x += up;
            }
            if ((t & 63) == 63) red[t >> 6] = x;
            __syncthreads();
            double before = 0.0;
            for (int v = 0; v < (t >> 6); ++v) before += red[v];
            sc[t + 1] = before + x;
            if (t == 0) sc[0] = 0.0;
        }
        __syncthreads();
        if (t < rt.n) {
            const long long kk = mt_keep(rt.r[t], out[0]);
            long long blk = kk / (long long)per;
            if (blk > seg_blocks) blk = seg_blocks;
            // a cut on or behind the last block's end has no owning block: its partial stayed zero
            out[UNERF_METRICS_AUSE_OFF + f * MT_MAXK + t] = sc[blk] + (blk < seg_blocks ? seg_part[(size_t)f * MT_MAXK + t] : 0.0);
        }
    } else if (blockIdx.x == MT_FAM) {
        if (!(flags & UNERF_METRICS_AUCE)) return;
        __shared__ unsigned long long bins[MT_MAXK];
        if (t < MT_MAXK) bins[t] = t < zt.n_z ? auce_cnt[t] : 0ull;
        __syncthreads();
        if (t < zt.n_z) {   // covered by threshold t (ascending) = everything in bins 0..t
            unsigned long long run = 0;
            for (int i = 0; i <= t; ++i) run += bins[i];
            out[UNERF_METRICS_AUCE_OFF + zt.perm[t]] = (double)run;
        }
    } else {
        if (!(flags & UNERF_METRICS_SSIM)) return;
        double v = 0.0;
        for (int i = t; i < ssim_wg; i += 1024) v += ssim_slab[i];
        const double r = block_sum<16>(v, red);
        if (t == 0) { out[12] = r; out[13] = ssim_count; }
    }
}

void ms_sort(hipStream_t st, const MtLayout& L, char* ws, uint32_t n, int B, const uint32_t* keys, bool with_idx) {
    const MtStrides sd{L.zstride, L.rstride};
    uint32_t* table = (uint32_t*)(ws + L.table);
    uint32_t* dtot = (uint32_t*)(ws + L.dtot);
    uint32_t* kbuf[2] = {(uint32_t*)(ws + L.tmp0), (uint32_t*)(ws + L.tmp1)};
    uint32_t* ibuf[2] = {(uint32_t*)(ws + L.idx0), (uint32_t*)(ws + L.idx1)};
    const uint32_t* kin = keys;
    const uint32_t* iin = nullptr;
    for (int pass = 0; pass < 4; ++pass) {   // results end in tmp1 / idx1
        uint32_t* kout = kbuf[pass & 1];
        uint32_t* iout = ibuf[pass & 1];
        const int shift = 8 * pass;
        hipLaunchKernelGGL(ms_hist_kernel, dim3(L.nblocks, B), dim3(MT_THREADS), 0, st, kin, n, shift, table, L.nblocks, sd);
        hipLaunchKernelGGL(ms_rowscan_kernel, dim3(256, B), dim3(1024), 0, st, table, L.nblocks, dtot, sd);
        if (!with_idx)
            hipLaunchKernelGGL((ms_scatter_kernel<false, false>), dim3(L.nblocks, B), dim3(MT_THREADS), 0, st, kin, iin, kout, iout, n, shift, table, dtot, L.nblocks, sd);
        else if (pass == 0)
            hipLaunchKernelGGL((ms_scatter_kernel<false, true>), dim3(L.nblocks, B), dim3(MT_THREADS), 0, st, kin, iin, kout, iout, n, shift, table, dtot, L.nblocks, sd);
        else
            hipLaunchKernelGGL((ms_scatter_kernel<true, true>), dim3(L.nblocks, B), dim3(MT_THREADS), 0, st, kin, iin, kout, iout, n, shift, table, dtot, L.nblocks, sd);
        kin = kout;
        iin = iout;
    }
}

// Both entry points.  `who` names the entry in messages, `batch` selects the wording of the workspace refusal; B = 1 is the
// single image.  Every launch below is one grid over all B images: nothing here loops over them.
int mt_run(const char* who, bool batch, const float* pred, const float* target, const float* sigma, const uint8_t* mask, int64_t n, int B,
           int C, int H, int W, float pred_clip_max, float nll_min_sigma, const double* ratios_host, int n_ratios, const double* z_host,
           int n_z, int flags, void* workspace, size_t workspace_bytes, double* out, void* stream) {
    UNERF_REQUIRE(n >= 0, "%s: n = %lld", who, (long long)n);
    UNERF_REQUIRE(B >= 1 && B <= UNERF_METRICS_MAX_IMAGES, "%s: B = %d (expected 1..%d images)", who, B, UNERF_METRICS_MAX_IMAGES);
    if (n == 0) return UNERF_OK;
    UNERF_REQUIRE(pred && target && sigma && out && workspace, "%s: null pointer (pred / target / sigma / workspace / out) with n > 0", who);
    UNERF_REQUIRE(C >= 1 && C <= 4, "%s: C = %d (expected 1..4)", who, C);
    UNERF_REQUIRE(n * (int64_t)C < ((int64_t)1 << 31), "%s: n * C = %lld (must stay below 2^31)", who, (long long)(n * C));
    UNERF_REQUIRE(n_ratios >= 1 && n_ratios <= MT_MAXK && ratios_host, "%s: n_ratios = %d (expected 1..128 host values)", who, n_ratios);
    UNERF_REQUIRE(n_z >= 1 && n_z <= MT_MAXK && z_host, "%s: n_z = %d (expected 1..128 host values)", who, n_z);
    if (flags & UNERF_METRICS_SSIM) {
        UNERF_REQUIRE(mask == nullptr, "%s: UNERF_METRICS_SSIM takes no mask", who);
        UNERF_REQUIRE((int64_t)H * (int64_t)W == n && H > 0 && W > 0, "%s: UNERF_METRICS_SSIM needs H * W == n (H = %d, W = %d, n = %lld)", who, H,
                      W, (long long)n);
        UNERF_REQUIRE(std::min(H, W) >= SS_K, "%s: UNERF_METRICS_SSIM needs min(H, W) >= 11 (H = %d, W = %d)", who, H, W);
    }
    const MtLayout L = mt_layout(n, B);
    if (batch)
        UNERF_REQUIRE(workspace_bytes >= L.total, "%s: workspace of %zu bytes, unerf_image_metrics_batch_workspace_bytes(%lld, %d) = %zu", who,
                      workspace_bytes, (long long)n, B, L.total);
    else
        UNERF_REQUIRE(workspace_bytes >= L.total, "%s: workspace of %zu bytes, unerf_image_metrics_workspace_bytes(%lld) = %zu", who,
                      workspace_bytes, (long long)n, L.total);
    UNERF_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out & 7) == 0, "%s: workspace / out must be 8-byte aligned", who);

    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const uint32_t un = (uint32_t)n;
    const MtStrides sd{L.zstride, L.rstride};
    MtZTable zt;
    {   // thresholds ascending (ties in the caller's order) and the way back
        int order[MT_MAXK];
        for (int i = 0; i < n_z; ++i) order[i] = i;
        std::stable_sort(order, order + n_z, [&](int a, int b) { return z_host[a] < z_host[b]; });
        for (int i = 0; i < MT_MAXK; ++i) { zt.z[i] = i < n_z ? z_host[order[i]] : 0.0; zt.perm[i] = i < n_z ? order[i] : 0; }
        zt.n_z = n_z;
    }
    MtRatios rt;
    for (int i = 0; i < MT_MAXK; ++i) rt.r[i] = i < n_ratios ? ratios_host[i] : 0.0;
    rt.n = n_ratios;

    // the accumulated regions of all B images lie next to each other, and so do the B rows
    if (hipMemsetAsync(ws + L.zeroed, 0, L.zero_bytes, st) != hipSuccess) return unerf_check_launch(who);
    if (hipMemsetAsync(out, 0, (size_t)B * UNERF_METRICS_ROW * sizeof(double), st) != hipSuccess) return unerf_check_launch(who);
    const bool want_ause = flags & UNERF_METRICS_AUSE;
    uint32_t* ksq = want_ause ? (uint32_t*)(ws + L.ksq) : nullptr;
    uint32_t* kab = (uint32_t*)(ws + L.kab);
    uint32_t* kvar = (uint32_t*)(ws + L.kvar);
    double* stat_slab = (double*)(ws + L.stat_slab);
    unsigned long long* auce_cnt = (unsigned long long*)(ws + L.auce_cnt);
    const int nwg = (int)std::min<int64_t>((n + MT_THREADS - 1) / MT_THREADS, MT_MAX_WG);
#define MT_STATS(CC)                                                                                                              \
    hipLaunchKernelGGL(mt_stats_kernel<CC>, dim3(nwg, B), dim3(MT_THREADS), 0, st, pred, target, sigma, mask, un, pred_clip_max, \
                       nll_min_sigma, flags, zt, ksq, kab, kvar, stat_slab, auce_cnt, sd)
    switch (C) {
        case 1: MT_STATS(1); break;
        case 2: MT_STATS(2); break;
        case 3: MT_STATS(3); break;
        default: MT_STATS(4); break;
    }
#undef MT_STATS
    hipLaunchKernelGGL(mt_reduce_kernel, dim3(1, B), dim3(1024), 0, st, stat_slab, nwg, out, sd);

    // segsum blocks: at most 1024 of them per image, each a whole number of 256-slot strides
    const uint32_t per = (uint32_t)(((n + MT_MAX_WG - 1) / MT_MAX_WG + MT_THREADS - 1) / MT_THREADS) * MT_THREADS;
    const int seg_blocks = (int)((n + per - 1) / per);
    double* seg_block = (double*)(ws + L.seg_block);
    double* seg_part = (double*)(ws + L.seg_part);
    if (want_ause) {
        const uint32_t* sorted_k = (const uint32_t*)(ws + L.tmp1);
        const uint32_t* sorted_i = (const uint32_t*)(ws + L.idx1);
        ms_sort(st, L, ws, un, B, ksq, false);
        hipLaunchKernelGGL(mt_segsum_kernel<false>, dim3(seg_blocks, B), dim3(MT_THREADS), 0, st, sorted_k, ksq, kab, un, per, out, rt, 0, seg_block, seg_part, sd);
        ms_sort(st, L, ws, un, B, kab, false);
        hipLaunchKernelGGL(mt_segsum_kernel<false>, dim3(seg_blocks, B), dim3(MT_THREADS), 0, st, sorted_k, ksq, kab, un, per, out, rt, 1, seg_block, seg_part, sd);
        ms_sort(st, L, ws, un, B, kvar, true);
        hipLaunchKernelGGL(mt_segsum_kernel<true>, dim3(seg_blocks, B), dim3(MT_THREADS), 0, st, sorted_i, ksq, kab, un, per, out, rt, 2, seg_block, seg_part, sd);
    }
    int ssim_wg = 0;
    double ssim_count = 0.0;
    if (flags & UNERF_METRICS_SSIM) {
        MtGauss gw;
        double sum = 0.0;
        for (int k = 0; k < SS_K; ++k) { const double d = (double)(k - SS_K / 2) / 1.5; gw.g[k] = std::exp(-(d * d) / 2.0); sum += gw.g[k]; }
        for (int k = 0; k < SS_K; ++k) gw.g[k] /= sum;
        const int OW = W - (SS_K - 1), OH = H - (SS_K - 1);
        const int64_t items = (int64_t)((OW + SS_TW - 1) / SS_TW) * ((OH + SS_TH - 1) / SS_TH) * C;
        ssim_wg = (int)std::min<int64_t>(items, MT_SSIM_WG);
        ssim_count = (double)OW * (double)OH * (double)C;
        hipLaunchKernelGGL(mt_ssim_kernel, dim3(ssim_wg, B), dim3(MT_THREADS), 0, st, pred, target, H, W, C, pred_clip_max, gw, out,
                           (double*)(ws + L.ssim_slab), sd);
    }
    hipLaunchKernelGGL(mt_finish_kernel, dim3(MT_FAM + 2, B), dim3(1024), 0, st, seg_block, seg_part, seg_blocks, per, rt, auce_cnt, zt,
                       (const double*)(ws + L.ssim_slab), ssim_wg, ssim_count, flags, out, sd);
    return unerf_check_launch(who);
}

}  // namespace

extern "C" size_t unerf_image_metrics_workspace_bytes(int64_t n) { return mt_layout(n, 1).total; }

extern "C" int unerf_image_metrics(const float* pred, const float* target, const float* sigma, const uint8_t* mask, int64_t n, int C,
                                   int H, int W, float pred_clip_max, float nll_min_sigma, const double* ratios_host, int n_ratios,
                                   const double* z_host, int n_z, int flags, void* workspace, size_t workspace_bytes, double* out,
                                   void* stream) {
    return mt_run("image_metrics", false, pred, target, sigma, mask, n, 1, C, H, W, pred_clip_max, nll_min_sigma, ratios_host, n_ratios,
                  z_host, n_z, flags, workspace, workspace_bytes, out, stream);
}

extern "C" size_t unerf_image_metrics_batch_workspace_bytes(int64_t n, int B) { return mt_layout(n, B).total; }

extern "C" int unerf_image_metrics_batch(const float* pred, const float* target, const float* sigma, const uint8_t* mask, int64_t n, int B,
                                         int C, int H, int W, float pred_clip_max, float nll_min_sigma, const double* ratios_host,
                                         int n_ratios, const double* z_host, int n_z, int flags, void* workspace, size_t workspace_bytes,
                                         double* out, void* stream) {
    return mt_run("image_metrics_batch", true, pred, target, sigma, mask, n, B, C, H, W, pred_clip_max, nll_min_sigma, ratios_host, n_ratios,
                  z_host, n_z, flags, workspace, workspace_bytes, out, stream);
}

// ---- rendered eval images: the four 8-bit planes of eval.save_imgs_rgb ------------------------------------------------
// unerf_eval_images_batch (include/unerf.h): what scripts/eval_uncertainty.py:209-303 hands to media.write_image, as final
// bytes.  Two kernels, the image is blockIdx.y of both (mt_img): ei_range leaves each image's min / max of the
// normalised std s over its non-NaN pixels, ei_pack writes every plane that was asked for, one pixel per thread.
// s is in [0, 1] or NaN, so its float32 order is the order of its bit patterns: the range goes wave butterfly -> LDS ->
// one integer atomicMin / atomicMax per workgroup on the image's two words, order-free and so repeatable.  The words are
// set inside the call (min 0xFFFFFFFF, max 0).  Arithmetic is the host definition's (eval.pack_eval_images): float32 for
// the differences, their sum and s, float64 for the colour index and the quantisation, every division IEEE (this file
// is built without fast-math and with hipcc's correctly rounded float32 division).
namespace {

constexpr int EI_THREADS = 256;          // pixels per workgroup and step
constexpr int EI_MAX_WG = 1024;          // workgroups per image; an image of more than EI_THREADS * EI_MAX_WG pixels strides

size_t ei_workspace(int B) { return al256(2 * sizeof(uint32_t) * (size_t)(B > 1 ? B : 1)); }

// clip((sigma - lo) / span, 0, 1) in float32; NaN stays NaN (fminf / fmaxf would drop it), -0 becomes +0
__device__ __forceinline__ float ei_norm(float sigma, float lo, float span) {
    const float x = (sigma - lo) / span;
    if (x != x) return x;
    return fminf(fmaxf(x, 0.f), 1.f) + 0.f;
}
// mediapy's float -> uint8: (uint8)(clip(x, 0, 1) * 255 + 0.5) in float64, truncating; NaN -> 0
__device__ __forceinline__ uint8_t ei_q(float x) {
    if (x != x) return 0;
    const double c = fmin(fmax((double)x, 0.0), 1.0);
    return (uint8_t)(int)(c * 255.0 + 0.5);
}

__global__ __launch_bounds__(EI_THREADS) void ei_range_kernel(const float* __restrict__ sigma0, uint32_t n, float lo, float span,
                                                              uint32_t* __restrict__ range /* [2, B]: min bits, max bits */) {
    __shared__ uint32_t red[2][EI_THREADS / 64];
    const float* __restrict__ sigma = mt_img(sigma0, (size_t)n * sizeof(float));
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
    for (uint32_t i = blockIdx.x * EI_THREADS + threadIdx.x; i < n; i += gridDim.x * EI_THREADS) {
        const float s = ei_norm(sigma[i], lo, span);
        if (s == s) {
            const uint32_t k = __float_as_uint(s);
            kmin = min(kmin, k);
            kmax = max(kmax, k);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, o));
        kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o));
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = kmin; red[1][threadIdx.x >> 6] = kmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < EI_THREADS / 64; ++w) { kmin = min(kmin, red[0][w]); kmax = max(kmax, red[1][w]); }
        if (kmin != 0xFFFFFFFFu) {      // a workgroup without a finite pixel has nothing to say
            atomicMin(&range[blockIdx.y], kmin);
            atomicMax(&range[gridDim.y + blockIdx.y], kmax);
        }
    }
}

__global__ __launch_bounds__(EI_THREADS) void ei_pack_kernel(const float* __restrict__ pred0, const float* __restrict__ target0,
                                                             const float* __restrict__ sigma0, uint32_t n, float lo, float span,
                                                             const uint8_t* __restrict__ lut, const uint32_t* __restrict__ range,
                                                             uint8_t* __restrict__ gt0, uint8_t* __restrict__ pr0,
                                                             uint8_t* __restrict__ er0, uint8_t* __restrict__ sd0) {
    __shared__ uint8_t jet[256 * 3];
    const float* __restrict__ pred = mt_img(pred0, (size_t)n * 3 * sizeof(float));
    const float* __restrict__ target = mt_img(target0, (size_t)n * 3 * sizeof(float));
    const float* __restrict__ sigma = mt_img(sigma0, (size_t)n * sizeof(float));
    uint8_t* __restrict__ gt8 = mt_img(gt0, (size_t)n * 3);
    uint8_t* __restrict__ pred8 = mt_img(pr0, (size_t)n * 3);
    uint8_t* __restrict__ err8 = mt_img(er0, (size_t)n);
    uint8_t* __restrict__ std8 = mt_img(sd0, (size_t)n * 3);
    double vmin = 0.0, denom = 1.0;
    if (std8) {
        for (int i = threadIdx.x; i < 256 * 3; i += EI_THREADS) jet[i] = lut[i];
        // an image without a finite pixel keeps min = 0xFFFFFFFF (a NaN): every pixel of it is NaN and takes the branch below
        vmin = (double)__uint_as_float(range[blockIdx.y]);
        denom = ((double)__uint_as_float(range[gridDim.y + blockIdx.y]) - vmin) + DBL_EPSILON;
        __syncthreads();
    }
    for (uint32_t i = blockIdx.x * EI_THREADS + threadIdx.x; i < n; i += gridDim.x * EI_THREADS) {
        const size_t i3 = (size_t)i * 3;
        if (gt8 || pred8 || err8) {
            float p[3], t[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { p[c] = pred[i3 + c]; t[c] = target[i3 + c]; }
            if (gt8) {
#pragma unroll
                for (int c = 0; c < 3; ++c) gt8[i3 + c] = ei_q(t[c]);
            }
            if (pred8) {
#pragma unroll
                for (int c = 0; c < 3; ++c) pred8[i3 + c] = ei_q(p[c]);
            }
            if (err8) {
                float ab = 0.f;
#pragma unroll
                for (int c = 0; c < 3; ++c) ab = ab + fabsf(p[c] - t[c]);
                err8[i] = ei_q(ab);
            }
        }
        if (std8) {
            const float s = ei_norm(sigma[i], lo, span);
            uint8_t r = 0, g = 0, b = 0;
            if (s == s) {
                const double a = ((double)s - vmin) / denom;
                const int idx = min((int)(a * 256.0), 255);
                r = jet[3 * idx]; g = jet[3 * idx + 1]; b = jet[3 * idx + 2];
            }
            std8[i3] = r; std8[i3 + 1] = g; std8[i3 + 2] = b;
        }
    }
}

}  // namespace

extern "C" size_t unerf_eval_images_workspace_bytes(int B) { return ei_workspace(B); }

extern "C" int unerf_eval_images_batch(const float* pred, const float* target, const float* sigma, int64_t n, int B, float unc_lo,
                                       float unc_span, const uint8_t* lut, uint8_t* gt8, uint8_t* pred8, uint8_t* err8, uint8_t* std8,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "eval_images_batch";
    UNERF_REQUIRE(n >= 0, "%s: n = %lld", who, (long long)n);
    UNERF_REQUIRE(B >= 1 && B <= UNERF_METRICS_MAX_IMAGES, "%s: B = %d (expected 1..%d images)", who, B, UNERF_METRICS_MAX_IMAGES);
    UNERF_REQUIRE(unc_span > 0.f && unc_span <= FLT_MAX && fabsf(unc_lo) <= FLT_MAX,
                  "%s: unc_lo = %g, unc_span = %g (expected finite values and unc_span > 0)", who, (double)unc_lo, (double)unc_span);
    if (n == 0) return UNERF_OK;
    UNERF_REQUIRE(3 * n < ((int64_t)1 << 31), "%s: 3 n = %lld (must stay below 2^31)", who, (long long)(3 * n));
    UNERF_REQUIRE(pred && target && sigma && lut && workspace, "%s: null pointer (pred / target / sigma / lut / workspace) with n > 0", who);
    UNERF_REQUIRE(workspace_bytes >= ei_workspace(B), "%s: workspace of %zu bytes, unerf_eval_images_workspace_bytes(%d) = %zu", who,
                  workspace_bytes, B, ei_workspace(B));
    UNERF_REQUIRE(((uintptr_t)workspace & 3) == 0, "%s: workspace must be 4-byte aligned", who);
    if (!gt8 && !pred8 && !err8 && !std8) return UNERF_OK;

    hipStream_t st = (hipStream_t)stream;
    uint32_t* range = (uint32_t*)workspace;
    const uint32_t un = (uint32_t)n;
    const dim3 grid((uint32_t)std::min<int64_t>((n + EI_THREADS - 1) / EI_THREADS, EI_MAX_WG), B);
    if (std8) {
        if (hipMemsetAsync(range, 0xFF, (size_t)B * sizeof(uint32_t), st) != hipSuccess) return unerf_check_launch(who);
        if (hipMemsetAsync(range + B, 0, (size_t)B * sizeof(uint32_t), st) != hipSuccess) return unerf_check_launch(who);
        hipLaunchKernelGGL(ei_range_kernel, grid, dim3(EI_THREADS), 0, st, sigma, un, unc_lo, unc_span, range);
    }
    hipLaunchKernelGGL(ei_pack_kernel, grid, dim3(EI_THREADS), 0, st, pred, target, sigma, un, unc_lo, unc_span, lut, range, gt8, pred8,
                       err8, std8);
    return unerf_check_launch(who);
}

// ---- pose normal equations: H = sum w J J^T, g = sum w r J, chi2 = sum w r^2 over a frame's [R,C,P] Jacobian -------------
// unerf_pose_normal_eq_* (include/unerf.h states the per-term arithmetic, the geometry and the chain length).  pn_accumulate:
// one workgroup per tile of PN_TILE consecutive pixels; thread t walks pixels t, t + 256, ... of its tile, so the lanes of a
// wave stand on consecutive pixels and the wave's loads of one step cover one contiguous run of 64 C P floats: every cache
// line of it is consumed whole while it is resident.  A row of P floats is read in the widest pieces its alignment allows
// (VEC = 4 when P % 4 == 0, 2 when P % 2 == 0, the base pointer aligned to match): per wave and step C P / VEC load
// instructions instead of C P.  The upper triangle of H, g and chi2 stay in registers (PW (PW + 1) / 2 + PW + 1 doubles;
// columns P .. PW-1 are loaded as zeros and never leave them), then wave butterfly -> LDS -> the four waves in order -> the
// tile's row.  pn_finish: workgroup e sums entry e of the tile rows in a fixed order and writes it where it belongs in out.
namespace {

constexpr int PN_THREADS = UNERF_POSE_NEQ_THREADS, PN_WAVES = PN_THREADS / 64, PN_PPT = UNERF_POSE_NEQ_PPT;
constexpr int PN_TILE = UNERF_POSE_NEQ_TILE, PN_RW = UNERF_POSE_NEQ_REDUCE_THREADS;
constexpr int PN_MAX_NE = UNERF_POSE_NEQ_WS_ROW(UNERF_POSE_NEQ_MAX_P);

inline int64_t pn_tiles(int64_t n_frame) { return n_frame > 0 ? (n_frame + PN_TILE - 1) / PN_TILE : 0; }
inline size_t pn_workspace(int64_t n_frame, int P) { return (size_t)pn_tiles(n_frame) * UNERF_POSE_NEQ_WS_ROW(P) * sizeof(double); }

__device__ __forceinline__ uint32_t pn_wave_count(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// row P floats of one term -> J[0..PW), zeros behind P
template <int PW, int VEC>
__device__ __forceinline__ void pn_load_row(const float* __restrict__ row, int P, float (&J)[PW]) {
    if constexpr (VEC == 4) {
#pragma unroll
        for (int k = 0; k < PW; k += 4) {
            const float4 v = k < P ? *reinterpret_cast<const float4*>(row + k) : make_float4(0.f, 0.f, 0.f, 0.f);
            J[k] = v.x; J[k + 1] = v.y;
            if (k + 2 < PW) { J[k + 2] = v.z; J[k + 3] = v.w; }
        }
    } else if constexpr (VEC == 2) {
#pragma unroll
        for (int k = 0; k < PW; k += 2) {
            const float2 v = k < P ? *reinterpret_cast<const float2*>(row + k) : make_float2(0.f, 0.f);
            J[k] = v.x; J[k + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < PW; ++k) J[k] = k < P ? row[k] : 0.f;
    }
}

template <int PW, int VEC>
__global__ __launch_bounds__(PN_THREADS) void pn_accumulate_kernel(const float* __restrict__ jac, const float* __restrict__ val,
                                                                   const float* __restrict__ target, const float* __restrict__ weight,
                                                                   int weight_per_channel, const uint8_t* __restrict__ mask, int64_t R,
                                                                   int C, int P, double* __restrict__ rows /* the launch's first tile */) {
    constexpr int NT = PW * (PW + 1) / 2;
    __shared__ double sh[PN_WAVES][PN_MAX_NE];
    double h[NT], g[PW], chi2 = 0.0;
#pragma unroll
    for (int i = 0; i < NT; ++i) h[i] = 0.0;
#pragma unroll
    for (int i = 0; i < PW; ++i) g[i] = 0.0;
    uint32_t used = 0u, skipped = 0u;
    const int64_t base = (int64_t)blockIdx.x * PN_TILE + threadIdx.x;
    for (int i = 0; i < PN_PPT; ++i) {
        const int64_t n = base + (int64_t)i * PN_THREADS;
        if (n >= R) break;
        if (mask && mask[n] == 0) continue;
        for (int c = 0; c < C; ++c) {
            const int64_t nc = n * C + c;
            float Jf[PW];
            pn_load_row<PW, VEC>(jac + nc * P, P, Jf);
            bool ok = true;
#pragma unroll
            for (int k = 0; k < PW; ++k) ok = ok && mt_finite(Jf[k]);
            double w = 1.0, r = 0.0;
            if (weight) {
                w = (double)weight[weight_per_channel ? nc : n];
                ok = ok && fabs(w) <= DBL_MAX && !(w < 0.0);
            }
            if (val) {
                r = (double)val[nc] - (double)target[nc];
                ok = ok && fabs(r) <= DBL_MAX;
            }
            if (!ok) { skipped += 1u; continue; }
            used += 1u;
            double J[PW];
#pragma unroll
            for (int k = 0; k < PW; ++k) J[k] = (double)Jf[k];
            int idx = 0;
#pragma unroll
            for (int a = 0; a < PW; ++a) {
                const double wa = w * J[a];
#pragma unroll
                for (int b = a; b < PW; ++b, ++idx) h[idx] = fma(wa, J[b], h[idx]);
            }
            if (val) {
                const double wr = w * r;
#pragma unroll
                for (int a = 0; a < PW; ++a) g[a] = fma(wr, J[a], g[a]);
                chi2 = fma(wr, r, chi2);
            }
        }
    }
    // the row's packed order: (a, b) with a <= b < P by rows, g[0..P), chi2, n_used, n_skipped
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int T = P * (P + 1) / 2;
    {
        int idx = 0;
#pragma unroll
        for (int a = 0; a < PW; ++a) {
#pragma unroll
            for (int b = a; b < PW; ++b, ++idx) {
                if (b < P) {   // uniform; a <= b
                    const double s = wave_sum(h[idx]);
                    if (lane == 0) sh[wv][a * P - a * (a - 1) / 2 + (b - a)] = s;
                }
            }
        }
#pragma unroll
        for (int a = 0; a < PW; ++a) {
            if (a < P) {
                const double s = wave_sum(g[a]);
                if (lane == 0) sh[wv][T + a] = s;
            }
        }
        const double s = wave_sum(chi2);
        const uint32_t cu = pn_wave_count(used), cs = pn_wave_count(skipped);
        if (lane == 0) { sh[wv][T + P] = s; sh[wv][T + P + 1] = (double)cu; sh[wv][T + P + 2] = (double)cs; }
    }
    __syncthreads();
    const int ne = T + P + 3;
    double* __restrict__ row = rows + (size_t)blockIdx.x * ne;
    for (int e = threadIdx.x; e < ne; e += PN_THREADS) {
        double s = sh[0][e];
#pragma unroll
        for (int w2 = 1; w2 < PN_WAVES; ++w2) s += sh[w2][e];
        row[e] = s;
    }
}

// workgroup e: entry e of the tile rows [0, tiles) -> its places in out
__global__ __launch_bounds__(PN_RW) void pn_finish_kernel(const double* __restrict__ rows, int64_t tiles, int P, double* __restrict__ out) {
    __shared__ double red[PN_RW / 64];
    const int T = P * (P + 1) / 2, ne = T + P + 3, e = blockIdx.x;
    double s = 0.0;
    for (int64_t t = threadIdx.x; t < tiles; t += PN_RW) s += rows[(size_t)t * ne + e];
    s = block_sum<PN_RW / 64>(s, red);
    if (threadIdx.x != 0) return;
    if (e < T) {
        int a = 0, first = 0;               // row a of the packed triangle starts at first and holds P - a entries
        while (e >= first + (P - a)) { first += P - a; ++a; }
        const int b = a + (e - first);
        out[a * P + b] = s;
        out[b * P + a] = s;
    } else {
        out[P * P + (e - T)] = s;           // g, chi2, n_used, n_skipped follow H in the row's order
    }
}

template <int PW>
void pn_launch(int vec, dim3 grid, hipStream_t st, const float* jac, const float* val, const float* target, const float* weight, int wpc,
               const uint8_t* mask, int64_t R, int C, int P, double* rows) {
    if (vec == 4)
        hipLaunchKernelGGL((pn_accumulate_kernel<PW, 4>), grid, dim3(PN_THREADS), 0, st, jac, val, target, weight, wpc, mask, R, C, P, rows);
    else if (vec == 2)
        hipLaunchKernelGGL((pn_accumulate_kernel<PW, 2>), grid, dim3(PN_THREADS), 0, st, jac, val, target, weight, wpc, mask, R, C, P, rows);
    else
        hipLaunchKernelGGL((pn_accumulate_kernel<PW, 1>), grid, dim3(PN_THREADS), 0, st, jac, val, target, weight, wpc, mask, R, C, P, rows);
}

}  // namespace

extern "C" size_t unerf_pose_normal_eq_workspace_bytes(int64_t N_frame, int P) {
    if (P < 1 || P > UNERF_POSE_NEQ_MAX_P) return 0;
    return pn_workspace(N_frame, P);
}

extern "C" int unerf_pose_normal_eq_accumulate(const float* jac, const float* val, const float* target, const float* weight,
                                               int weight_per_channel, const uint8_t* mask, int64_t R, int C, int P, int64_t pixel_offset,
                                               int64_t N_frame, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "pose_normal_eq";
    UNERF_REQUIRE(P >= 1 && P <= UNERF_POSE_NEQ_MAX_P, "%s: P = %d (expected 1..%d)", who, P, UNERF_POSE_NEQ_MAX_P);
    UNERF_REQUIRE(C >= 1 && C <= UNERF_POSE_NEQ_MAX_C, "%s: C = %d (expected 1..%d)", who, C, UNERF_POSE_NEQ_MAX_C);
    UNERF_REQUIRE(R >= 0, "%s: R = %lld", who, (long long)R);
    UNERF_REQUIRE((val == nullptr) == (target == nullptr), "%s: val and target go together (%s is missing)", who, val ? "target" : "val");
    UNERF_REQUIRE(pixel_offset >= 0 && pixel_offset % PN_TILE == 0, "%s: pixel_offset = %lld (expected a non-negative multiple of the tile, %d)",
                  who, (long long)pixel_offset, PN_TILE);
    UNERF_REQUIRE(N_frame >= 0 && R <= N_frame && pixel_offset <= N_frame - R, "%s: pixel_offset + R = %lld + %lld exceeds N_frame = %lld", who,
                  (long long)pixel_offset, (long long)R, (long long)N_frame);
    if (R == 0) return UNERF_OK;
    UNERF_REQUIRE(jac && workspace, "%s: null pointer (jac / workspace) with R > 0", who);
    UNERF_REQUIRE(workspace_bytes >= pn_workspace(N_frame, P), "%s: workspace of %zu bytes, unerf_pose_normal_eq_workspace_bytes(%lld, %d) = %zu",
                  who, workspace_bytes, (long long)N_frame, P, pn_workspace(N_frame, P));
    UNERF_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)jac & 3) == 0, "%s: workspace must be 8-byte, jac 4-byte aligned", who);
    const int64_t nblk = (R + PN_TILE - 1) / PN_TILE;
    UNERF_REQUIRE(nblk < ((int64_t)1 << 31), "%s: R = %lld (more than 2^31 tiles)", who, (long long)R);
    const int vec = (P % 4 == 0 && ((uintptr_t)jac & 15) == 0) ? 4 : (P % 2 == 0 && ((uintptr_t)jac & 7) == 0) ? 2 : 1;
    double* rows = (double*)workspace + (size_t)(pixel_offset / PN_TILE) * UNERF_POSE_NEQ_WS_ROW(P);
    const dim3 grid((uint32_t)nblk);
    hipStream_t st = (hipStream_t)stream;
    if (P <= 6) pn_launch<6>(vec, grid, st, jac, val, target, weight, weight_per_channel, mask, R, C, P, rows);
    else pn_launch<12>(vec, grid, st, jac, val, target, weight, weight_per_channel, mask, R, C, P, rows);
    return unerf_check_launch(who);
}

extern "C" int unerf_pose_normal_eq_finish(const void* workspace, size_t workspace_bytes, int64_t N_frame, int P, double* out,
                                           void* stream) {
    const char* who = "pose_normal_eq_finish";
    UNERF_REQUIRE(P >= 1 && P <= UNERF_POSE_NEQ_MAX_P, "%s: P = %d (expected 1..%d)", who, P, UNERF_POSE_NEQ_MAX_P);
    UNERF_REQUIRE(N_frame >= 0, "%s: N_frame = %lld", who, (long long)N_frame);
    UNERF_REQUIRE(out && (workspace || N_frame == 0), "%s: null pointer (workspace / out)", who);
    UNERF_REQUIRE(workspace_bytes >= pn_workspace(N_frame, P), "%s: workspace of %zu bytes, unerf_pose_normal_eq_workspace_bytes(%lld, %d) = %zu",
                  who, workspace_bytes, (long long)N_frame, P, pn_workspace(N_frame, P));
    UNERF_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out & 7) == 0, "%s: workspace / out must be 8-byte aligned", who);
    hipLaunchKernelGGL(pn_finish_kernel, dim3(UNERF_POSE_NEQ_WS_ROW(P)), dim3(PN_RW), 0, (hipStream_t)stream, (const double*)workspace,
                       pn_tiles(N_frame), P, out);
    return unerf_check_launch(who);
}
